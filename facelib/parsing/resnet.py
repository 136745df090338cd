from codeformer_amd.facelib.parsing.resnet import BasicBlock, ResNet18, conv3x3, create_layer_basic  # noqa: F401
