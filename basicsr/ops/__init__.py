"""Import shim: `basicsr.ops.*` of the reference resolves to codeformer_amd.bundled (fused_act, upfirdn2d) and codeformer_amd.dcn (HIP, inference only)."""
