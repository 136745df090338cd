from codeformer_amd.metrics import reorder_image, to_y_channel  # noqa: F401
