from codeformer_amd.facelib.parsing import BiSeNet, ParseNet, init_parsing_model, load_bisenet  # noqa: F401
