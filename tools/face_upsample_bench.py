"""Cost of --face_upsample / --draw_box on the device paste-back.

  * ms per 16-face RealESRGANer.enhance_faces call (RealESRGAN_x2plus shape: 23 blocks, seeded random weights) with the CLI's tiles
    (tile 400, tile_pad 40, pre_pad 0) and untiled (tile 0), with f16 operands (`half`, the CLI's GPU default) and in fp32;
  * ms per 1080p -> 4K frame (-s 2) with 3 faces for DeviceFaceHelper.paste_faces_to_input_image alone, with draw_box, and with face
    upsampling (half, 400/40 tiles; the upsampler call of the frame's 3 faces included).
Device time by CUDA events, medians over the repeats.
usage: python tools/face_upsample_bench.py [repeats]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from codeformer_amd import lib  # noqa: E402
from codeformer_amd.archs.rrdbnet_arch import RRDBNet  # noqa: E402
from codeformer_amd.facelib.paste import DeviceFaceHelper  # noqa: E402
from codeformer_amd.utils.realesrgan_utils import RealESRGANer  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5


def ms(fn, n=reps, warmup=1):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def upsampler(tile, half):
    torch.manual_seed(0)
    net = RRDBNet(3, 3, scale=2, num_feat=64, num_block=23, num_grow_ch=32)
    return RealESRGANer(scale=2, model_path=None, model=net, tile=tile, tile_pad=40, pre_pad=0, half=half, device='cuda')


def affine(cx, cy, size, ang):
    s = 512.0 / size
    c, sn = np.cos(ang) * s, np.sin(ang) * s
    return np.array([[c, -sn, 256 - (c * cx - sn * cy)], [sn, c, 256 - (sn * cx + c * cy)]])


lib.load()
rng = np.random.default_rng(0)
print(f'device: {torch.cuda.get_device_name(0)}, {reps} repeats (median)')
faces16 = torch.from_numpy(rng.integers(0, 256, (16, 512, 512, 3), dtype=np.uint8)).cuda()
ups = {}
for half in (True, False):
    for tile in (400, 0):
        up = ups[(tile, half)] = upsampler(tile, half)
        t = ms(lambda: up.enhance_faces(faces16))
        print(f"enhance_faces 16 x 512^2  tile {tile:3d}{'/40' if tile else '   '}  {'half' if half else 'fp32'}: {t:9.1f} ms "
              f'({t / 16:.1f} ms per face)')

frame = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
affs = [affine(500, 400, 260, 0.1), affine(1000, 540, 300, -0.2), affine(1500, 600, 220, 0.0)]
h = DeviceFaceHelper(upscale_factor=2, device='cuda')
h.read_image(frame)
crops = h.align_warp_face(affs)
h.add_restored_faces(crops.clone())
up = ups[(400, True)]
for label, kw in (('paste', {}), ('paste + draw_box', {'draw_box': True}), ('paste + face upsampling (half, 400/40)', {'face_upsampler': up})):
    t = ms(lambda: h.paste_faces_to_input_image(return_tensor=True, **kw))
    print(f'1080p -> 4K, 3 faces, {label}: {t:.2f} ms per frame')
