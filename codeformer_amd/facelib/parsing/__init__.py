"""Face parsing (reference: facelib/parsing/__init__.py:8-23)."""
import os

import torch

from ...utils.download_util import load_file_from_url
from .bisenet import BiSeNet
from .parsenet import ParseNet

__all__ = ['BiSeNet', 'ParseNet', 'init_parsing_model', 'load_bisenet']

_PARSENET_URL = 'https://github.com/sczhou/CodeFormer/releases/download/v0.1.0/parsing_parsenet.pth'


def load_bisenet(model_path, device='cuda', num_class=19):
    """BiSeNet(num_class) in eval mode on `device` with the state dict at `model_path` loaded strictly.  Nothing is downloaded: without a
    path this raises NotImplementedError, a missing file FileNotFoundError."""
    if model_path is None:
        raise NotImplementedError('bisenet: weights are not downloaded here; pass `model_path`')
    if not os.path.isfile(model_path):
        raise FileNotFoundError(f'BiSeNet checkpoint {model_path} not found (nothing is downloaded)')
    model = BiSeNet(num_class=num_class)
    model.load_state_dict(torch.load(model_path, map_location='cpu', weights_only=True), strict=True)
    return model.eval().to(device)


def init_parsing_model(model_name='bisenet', half=False, device='cuda', model_path=None):
    """Same call as the reference.  'parsenet' (the model face_restoration_helper.py:125 asks for) reads its weights from weights/facelib/
    (no download: load_file_from_url returns an existing file or raises); 'bisenet' loads only from an explicit `model_path`."""
    if model_name == 'bisenet':
        return load_bisenet(model_path, device=device)
    if model_name != 'parsenet':
        raise NotImplementedError(f'{model_name} is not implemented (HIP path: bisenet with a model_path, parsenet).')
    model = ParseNet(in_size=512, out_size=512, parsing_ch=19)
    if model_path is None:
        model_path = load_file_from_url(url=_PARSENET_URL, model_dir=os.path.join('weights', 'facelib'), progress=True,
                                        file_name=None)
    model.load_state_dict(torch.load(model_path, map_location='cpu'), strict=True)
    return model.eval().to(device)
