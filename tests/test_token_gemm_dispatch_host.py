"""The token-GEMM route of cf_conv2d (taps 1, split-half operands, "images" of at most 1024 pixels: cf_gemm_split_launch), seen from the
host: the sibling of test_conv_dispatch_host.py for the one launch family that used to take no parts-query pointer.  A query
(cf_conv2d_stats_parts with stats_cpg 0) runs every check of a launch and answers 0 partials -- these kernels write no statistics --
without launching, so the table needs no GPU; pointers are dummies that nothing dereferences.

Refusals expect a piece of cf_last_error() copied from the source text of the commit before the route took the pointer (its checks, their
order and their messages must not move); cf_conv2d_tiles / cf_conv2d_workspace_bytes on the accepted shapes expect what a build of that
commit returned (those two never launched there either)."""
import ctypes

import pytest

from codeformer_amd import build as cf_build
from codeformer_amd import lib

PTR = 0x1000  # a non-null pointer for the fields a check only tests for presence


def G(hin, win, k, n, split_k=0, **kw):
    """A token GEMM of hin * win rows, K = k, N = n as a 1x1 descriptor with split-half operands, no statistics."""
    f = dict(hin=hin, win=win, hout=hin, wout=win, c0=k, cout=n, cout_pad=n, taps=1, stride=1, bf16_mfma=3, batch=1, stats_cpg=0, acc_scale=1.0,
             split_k=split_k)
    f.update(kw)
    return f


DENSE = 'cf_conv2d(1x1, f16x2): dense single-input token GEMMs without prologue / statistics only'
EPI = 'cf_conv2d(1x1, f16x2): epilogues are none / GELU / residual'
# (what the row exercises, descriptor, 0 partials | piece of cf_last_error())
ROWS = [
    ('split_k 0: 256 rows', G(16, 16, 256, 64), 0),
    ('split_k 0: 64 rows', G(8, 8, 256, 64), 0),
    ('split_k 1', G(16, 16, 256, 64, split_k=1), 0),
    ('split_k 2 with workspace and counters', G(16, 16, 256, 64, split_k=2, workspace=PTR, counters=PTR), 0),
    ('split_k 4 on K 512', G(16, 16, 512, 128, split_k=4, workspace=PTR, counters=PTR), 0),
    ('split_k -1: 32 rows', G(4, 8, 256, 64, split_k=-1), 0),
    ('split_k -1: K 1024', G(8, 8, 1024, 64, split_k=-1), 0),
    ('GELU epilogue', G(16, 16, 256, 64, epilogue=3), 0),
    ('residual epilogue', G(16, 16, 256, 64, epilogue=1, res=PTR), 0),
    ('in0_alt: alt_cout0 128 of 256', G(16, 16, 256, 256, in0_alt=PTR, alt_cout0=128), 0),
    ('M 32 is no multiple of 64', G(4, 8, 256, 64), 'cf_conv2d(1x1, f16x2): M 32 must be a multiple of 64, N 64 of 64, K 256 of 128'),
    ('split_k -1: M 16 is no multiple of 32', G(4, 4, 256, 64, split_k=-1), 'cf_conv2d(1x1, f16x2): M 16 must be a multiple of 32, N 64 of 64, K 256 of 128'),
    ('N 96', G(16, 16, 256, 96), 'cf_conv2d(1x1, f16x2): M 256 must be a multiple of 64, N 96 of 64, K 256 of 128'),
    ('K 192', G(16, 16, 192, 64), 'cf_conv2d(1x1, f16x2): M 256 must be a multiple of 64, N 64 of 64, K 192 of 128'),
    ('cout_pad 128 for cout 64', G(16, 16, 256, 64, cout_pad=128), 'cf_conv2d(1x1, f16x2): M 256 must be a multiple of 64, N 64 of 64, K 256 of 128'),
    ('a second input', G(16, 16, 128, 64, c1=128, in1=PTR), DENSE),
    ('a prologue', G(16, 16, 256, 64, prologue=3), DENSE),
    ('channel stride on the output', G(16, 16, 256, 64, ld_out=80), DENSE),
    ('channel stride on the input', G(16, 16, 256, 64, ld_in0=320), DENSE),
    ('LEAKY epilogue', G(16, 16, 256, 64, epilogue=4), EPI),
    ('SFT epilogue', G(16, 16, 256, 64, epilogue=2, res=PTR, sft_scale=PTR), EPI),
    ('acc_scale 0', G(16, 16, 256, 64, acc_scale=0.0), 'cf_conv2d(1x1, f16x2): acc_scale must be the inverse of the pack-time weight scale (got 0)'),
    ('in0_alt: alt_cout0 0', G(16, 16, 256, 256, in0_alt=PTR, alt_cout0=0), 'in0_alt needs 0 < alt_cout0 < cout, a multiple of 128 (got 0 of 256)'),
    ('in0_alt: alt_cout0 == cout', G(16, 16, 256, 256, in0_alt=PTR, alt_cout0=256), 'in0_alt needs 0 < alt_cout0 < cout, a multiple of 128 (got 256 of 256)'),
    ('in0_alt: alt_cout0 64', G(16, 16, 256, 256, in0_alt=PTR, alt_cout0=64), 'in0_alt needs 0 < alt_cout0 < cout, a multiple of 128 (got 64 of 256)'),
    ('split_k 3 on K 512', G(16, 16, 512, 64, split_k=3, workspace=PTR, counters=PTR), 'cf_conv2d(1x1, f16x2): split_k 3 must divide K/128 = 4'),
    ('split_k 2 without a workspace', G(16, 16, 256, 64, split_k=2), 'cf_conv2d(1x1, f16x2): split_k > 1 needs workspace and counters'),
    ('split_k -1: K 1152', G(8, 8, 1152, 64, split_k=-1),
     'cf_conv2d(1x1, f16x2, in-workgroup split): K 1152 must be a multiple of 128 up to 1024, M a multiple of 32'),
    ('a statistics query is refused before the route', G(16, 16, 256, 64, stats_cpg=2), 'cf_conv2d(1x1, f16x2): no statistics epilogue'),
    ('so is any query of the streaming 1x1 form (64x64 pixels)', G(64, 64, 64, 64), 'cf_conv2d(1x1, f16x2): no statistics epilogue'),
]
# accepted shapes: (row, cf_conv2d_tiles, cf_conv2d_workspace_bytes)
GEOMETRY = [
    ('split_k 0: 256 rows', 0, 0),
    ('split_k 0: 64 rows', 0, 0),
    ('split_k 1', 4, 0),
    ('split_k 2 with workspace and counters', 4, 131072),
    ('split_k 4 on K 512', 8, 524288),
    ('split_k -1: 32 rows', 0, 0),
    ('split_k -1: K 1024', 0, 0),
    ('GELU epilogue', 0, 0),
    ('residual epilogue', 0, 0),
    ('in0_alt: alt_cout0 128 of 256', 0, 0),
]


@pytest.fixture(scope='module')
def native():
    cf_build.build()
    return lib.load()


@pytest.mark.parametrize('note,fields,expected', ROWS, ids=[r[0] for r in ROWS])
def test_stats_parts_query(native, note, fields, expected):
    d = lib.ConvDesc(**fields)
    got = native.cf_conv2d_stats_parts(ctypes.byref(d))
    if isinstance(expected, int):
        assert got == expected, (note, got, lib.last_error())
    else:
        assert got == -1 and expected in lib.last_error(), (note, got, lib.last_error())


@pytest.mark.parametrize('note,tiles,ws_bytes', GEOMETRY, ids=[r[0] for r in GEOMETRY])
def test_geometry_queries(native, note, tiles, ws_bytes):
    d = lib.ConvDesc(**dict((r[0], r[1]) for r in ROWS)[note])
    assert (native.cf_conv2d_tiles(ctypes.byref(d)), native.cf_conv2d_workspace_bytes(ctypes.byref(d))) == (tiles, ws_bytes), lib.last_error()
