"""Winograd conv kernel vs fp64 reference and vs the direct kernel (accuracy + time).  GPU box only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from codeformer_amd import ops  # noqa: E402
from conv_case import draw, launch_args, reference, stats_rel_err, t_ms  # noqa: E402


def case(B, H, W, cin, cout, *, c_split=None, prologue=ops.PRO_NONE, epilogue=ops.EPI_NONE, stats=False, seed=0, timing=True,
         direct=True):
    x, w, b, sc, sh, res, ss = draw(B, H, W, cin, cout, seed=seed)
    ref = reference(x, w, b, prologue=prologue, epilogue=epilogue, sc=sc, sh=sh, res=res, ss=ss)
    x1, x2, kw = launch_args(x, sc, sh, res, ss, prologue=prologue, epilogue=epilogue, stats=stats, c_split=c_split)
    pw_d = ops.pack_weight(w.cuda(), b.cuda())
    pw_w = ops.pack_weight(w.cuda(), b.cuda(), bf16=ops.WINOGRAD)
    yw = ops.conv2d(x1, pw_w, x2=x2, **kw)
    yd = ops.conv2d(x1, pw_d, x2=x2, **kw) if direct else yw   # (direct=False: sizes / options the direct kernel does not combine)
    ed = float((yd.cpu().double() - ref).abs().max())
    ew = float((yw.cpu().double() - ref).abs().max())
    msg = f'B{B} {H}x{W} {cin}->{cout} pro{prologue} epi{epilogue}{" cat" if c_split else ""}: direct {ed:.2e} winograd {ew:.2e} (ref max {float(ref.abs().max()):.2f})'
    es = 0.0
    if stats:   # the epilogue's GroupNorm partials must describe exactly the tensor that was written
        es = stats_rel_err(yw)
        msg += f' | stats rel err {es:.1e}'
    if timing:
        td_, tw_ = t_ms(lambda: ops.conv2d(x1, pw_d, x2=x2, **kw)), t_ms(lambda: ops.conv2d(x1, pw_w, x2=x2, **kw))
        fl = 2.0 * B * H * W * cout * cin * 9
        msg += f' | {td_:.3f} ms ({fl / td_ / 1e9:.0f} TF) -> {tw_:.3f} ms ({fl / tw_ / 1e9:.0f} TF-equiv) x{td_ / tw_:.2f}'
    print(msg, flush=True)
    return ed, ew, es, float(ref.abs().max())


if __name__ == '__main__':
    case(1, 16, 16, 16, 64, timing=False)
    case(2, 16, 32, 32, 64, timing=False, seed=1)
    case(2, 16, 16, 64, 128, prologue=ops.PRO_AFFINE_SWISH, epilogue=ops.EPI_RESIDUAL, stats=True, timing=False, seed=2)
    case(2, 32, 32, 128, 64, c_split=64, prologue=ops.PRO_LEAKY, epilogue=ops.EPI_SFT, stats=False, timing=False, seed=3)
    case(2, 16, 16, 512, 512, prologue=ops.PRO_AFFINE_SWISH, stats=True, timing=False, seed=4)
    case(1, 64, 64, 256, 256, prologue=ops.PRO_AFFINE, stats=True, timing=False, seed=5)
    for shape in ((16, 256, 256, 128, 128), (16, 512, 512, 64, 64), (16, 64, 64, 256, 256), (16, 128, 128, 128, 128),
                  (16, 16, 16, 512, 512), (16, 32, 32, 256, 256)):
        case(*shape, prologue=ops.PRO_AFFINE_SWISH, epilogue=ops.EPI_RESIDUAL, stats=True, seed=9)
