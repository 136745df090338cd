from codeformer_amd.facelib.parsing.bisenet import AttentionRefinementModule, BiSeNet, BiSeNetOutput, ContextPath, ConvBNReLU, FeatureFusionModule  # noqa: F401
