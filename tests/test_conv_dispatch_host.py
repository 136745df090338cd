"""cf_conv2d's validation, routing and tile choice, seen from the host: a table of descriptors, each with the number of statistics partials
cf_conv2d_stats_parts returns for it or a piece of the error it reports.  That query runs the same code as a launch up to the point
where a kernel would start and never launches, so the table needs no GPU -- and a descriptor that wrongly passed validation could not start
a kernel; cf_conv2d itself is never called here.

The expected values are what the library returned for this table BEFORE conv_dispatch was split into validation / routing / argument fill /
tile ladder (produced by running the table against a build of the parent commit): the split must not move a route, a tile shape or the
first failing check."""
import ctypes

import pytest

from codeformer_amd import build as cf_build
from codeformer_amd import lib


def D(hin, win, c0, cout, cout_pad, taps=9, stride=1, upsample=0, bf16_mfma=0, batch=1, stats_cpg=2, **kw):
    """Descriptor fields of a conv on hin x win inputs; hout / wout follow from stride / upsample, everything else defaults to 0 / NULL."""
    hout, wout = (hin // 2, win // 2) if stride == 2 else (hin << upsample, win << upsample)
    return dict(hin=hin, win=win, hout=hout, wout=wout, c0=c0, cout=cout, cout_pad=cout_pad, taps=taps, stride=stride, upsample=upsample,
                bf16_mfma=bf16_mfma, batch=batch, stats_cpg=stats_cpg, **kw)


# (what the row exercises, descriptor, partials per (image, group) | piece of cf_last_error())
ROWS = [
    ('3x3 fp32: cout_pad 64', D(64, 64, 64, 64, 64), 64),
    ('3x3 fp32: cout_pad 128', D(64, 64, 64, 128, 128), 64),
    ('3x3 fp32: cout_pad 128, narrow', D(32, 32, 64, 128, 128, batch=2), 16),
    ('3x3 fp32: cout_pad 192', D(64, 64, 64, 192, 192), 'no kernel for taps=9 stride=1 cout_pad=192'),
    ('up2x fp32: cout_pad 64', D(32, 32, 64, 64, 64, upsample=1), 64),
    ('up2x fp32: cout_pad 128', D(32, 32, 64, 128, 128, upsample=1), 64),
    ('up2x fp32: cout_pad 128, narrow', D(16, 16, 64, 128, 128, upsample=1, batch=2), 16),
    ('up2x fp32: cout_pad 192', D(32, 32, 64, 192, 192, upsample=1), 'upsample path needs cout_pad 64 or a multiple of 128 (got 192)'),
    ('3x3 bf16: cout_pad 64', D(64, 64, 64, 64, 64, bf16_mfma=1), 64),
    ('3x3 bf16: cout_pad 128', D(64, 64, 64, 128, 128, bf16_mfma=1), 64),
    ('3x3 bf16: cout_pad 128, narrow', D(32, 32, 64, 128, 128, bf16_mfma=1, batch=2), 16),
    ('3x3 bf16: cout_pad 192', D(64, 64, 64, 192, 192, bf16_mfma=1), 64),
    ('up2x bf16: cout_pad 64', D(32, 32, 64, 64, 64, upsample=1, bf16_mfma=1), 64),
    ('up2x bf16: cout_pad 128', D(32, 32, 64, 128, 128, upsample=1, bf16_mfma=1), 64),
    ('up2x bf16: cout_pad 128, narrow', D(16, 16, 64, 128, 128, upsample=1, bf16_mfma=1, batch=2), 16),
    ('up2x bf16: cout_pad 192', D(32, 32, 64, 192, 192, upsample=1, bf16_mfma=1), 64),
    ('3x3 f16: cout_pad 64', D(64, 64, 64, 64, 64, bf16_mfma=2), 64),
    ('3x3 f16: cout_pad 128', D(64, 64, 64, 128, 128, bf16_mfma=2), 64),
    ('3x3 f16: cout_pad 128, narrow', D(32, 32, 64, 128, 128, bf16_mfma=2, batch=2), 16),
    ('3x3 f16: cout_pad 192', D(64, 64, 64, 192, 192, bf16_mfma=2), 64),
    ('up2x f16: cout_pad 64', D(32, 32, 64, 64, 64, upsample=1, bf16_mfma=2), 64),
    ('up2x f16: cout_pad 128', D(32, 32, 64, 128, 128, upsample=1, bf16_mfma=2), 64),
    ('up2x f16: cout_pad 128, narrow', D(16, 16, 64, 128, 128, upsample=1, bf16_mfma=2, batch=2), 16),
    ('up2x f16: cout_pad 192', D(32, 32, 64, 192, 192, upsample=1, bf16_mfma=2), 64),
    ('1x1 fp32: cout_pad 64', D(64, 64, 64, 64, 64, taps=1), 64),
    ('1x1 fp32: cout_pad 128', D(64, 64, 64, 128, 128, taps=1), 64),
    ('1x1 fp32: cout_pad 128, narrow', D(32, 32, 64, 128, 128, taps=1, batch=2), 16),
    ('1x1 fp32: cout_pad 192', D(64, 64, 64, 192, 192, taps=1), 'no kernel for taps=1 stride=1 cout_pad=192'),
    ('1x1 fp32: off-grid 40x48 rows', D(40, 48, 64, 64, 64, taps=1), '1x1 rows 1920 (per image 1920) not divisible by 256'),
    ('3x3 fp32: cout_pad 32', D(64, 64, 64, 32, 32), 64),
    ('EXT: channel stride on the output', D(64, 64, 64, 64, 64, stats_cpg=0, ld_out=80), 64),
    ('EXT: LEAKY epilogue, cout_pad 32', D(64, 64, 64, 32, 32, stats_cpg=0, epilogue=4), 64),
    ('EXT: off-grid 40x48', D(40, 48, 64, 64, 64, stats_cpg=0), 36),
    ('EXT: f16 with cout_pad 32', D(64, 64, 64, 32, 32, bf16_mfma=2, stats_cpg=0), 64),
    ('EXT: upsample off-grid, cout_pad 128', D(20, 24, 64, 128, 128, upsample=1, stats_cpg=0), 48),
    ('EXT: upsample, cout_pad 96', D(20, 24, 64, 96, 96, upsample=1, stats_cpg=0), 'general upsample path needs cout_pad % 64 == 0 (got 96)'),
    ('EXT: no statistics', D(40, 48, 64, 64, 64), 'strided slices / leaky|axpy epilogues / off-grid sizes (40x48) need a '),
    ('EXT: stride 2 with pad_lo, cout_pad 128', D(64, 64, 64, 128, 128, stride=2, stats_cpg=0, pad_lo=1), 16),
    ('stride 2: cout_pad 64', D(64, 64, 64, 64, 64, stride=2), 16),
    ('stride 2: 64 wide workgroups -> 64-wide tiles', D(64, 64, 64, 1024, 1024, stride=2), 16),
    ('stride 2: 72 wide workgroups -> 128-wide tiles', D(64, 64, 64, 1152, 1152, stride=2), 16),
    ('in_nchw: vector-ALU first conv', D(64, 64, 3, 64, 64, in_nchw=1), 64),
    ('in_nchw: stats_cpg 4 -> MFMA kernel', D(64, 64, 3, 64, 64, stats_cpg=4, in_nchw=1), 64),
    ('in_nchw: cout_pad 128', D(64, 64, 3, 128, 128, in_nchw=1), 'in_nchw path is built for cout_pad 64 (got 128)'),
    ('out_nchw: 3-channel head has no statistics', D(64, 64, 64, 3, 32, stats_cpg=0, out_nchw=1), 64),
    ('io_bf16: direct bf16 3x3, cout_pad 64', D(64, 64, 64, 64, 64, bf16_mfma=1, io_bf16=1), 64),
    ('io_bf16: folded upsample bf16, cout_pad 128', D(64, 64, 64, 128, 128, upsample=1, bf16_mfma=1, io_bf16=1), 256),
    ('io_bf16: fp32 1x1 on 64x64', D(64, 64, 64, 64, 64, taps=1, io_bf16=1), 64),
    ('io_bf16: fp32 3x3 refused', D(64, 64, 64, 64, 64, io_bf16=1), 'io_bf16 (bf16 tensors) is built for dense stride-1 launches of the bf1'),
    ('split_k 2 divides K/128 = 2', D(16, 16, 256, 64, 64, taps=1, split_k=2), 8),
    ('split_k 3 does not', D(16, 16, 256, 64, 64, taps=1, split_k=3), 'split_k 3 needs cout_pad % 64 == 0, K % 128 == 0 and split_k dividing '),
    ('route: F(2,3) fp32', D(32, 32, 64, 64, 64, winograd=1), 32),
    ('route: F(2,3) split-half', D(32, 32, 64, 64, 64, bf16_mfma=3, winograd=1, acc_scale=1.0), 32),
    ('route: F(4,3) split-half', D(32, 32, 64, 64, 64, bf16_mfma=3, winograd=2, acc_scale=1.0), 4),
    ('route: F(4,3) fp32', D(32, 32, 64, 64, 64, winograd=2), 4),
    ('route: split-half direct', D(64, 64, 64, 64, 64, bf16_mfma=3, acc_scale=1.0), 64),
    ('route: streaming 1x1 writes no statistics', D(64, 64, 64, 64, 64, taps=1, bf16_mfma=3, acc_scale=1.0), 'cf_conv2d(1x1, f16x2): no statistics epilogue'),
    ('bad operand format', D(64, 64, 64, 64, 64, bf16_mfma=7), 'bad operand format 7'),
    ('winograd must be', D(64, 64, 64, 64, 64, winograd=3), 'winograd must be 0, 1 (F(2x2,3x3)) or 2 (F(4x4,3x3)), got 3'),
    # the checks the four launchers share (dense tensors, zero padding, epilogue triple, acc_scale), per family: answers of the commit
    # before the launchers took them from cf_conv_parts.h
    ('F(2,3) fp32: channel stride on the output', D(32, 32, 64, 64, 64, winograd=1, ld_out=192), 'cf_conv2d: winograd reads / writes dense tensors with zero padding'),
    ('F(2,3) fp32: reflect padding', D(32, 32, 64, 64, 64, winograd=1, pad_mode=1), 'cf_conv2d: winograd reads / writes dense tensors with zero padding'),
    ('F(2,3) fp32: LEAKY epilogue', D(32, 32, 64, 64, 64, winograd=1, epilogue=4), 'cf_conv2d: winograd epilogues are none / residual / SFT'),
    ('F(2,3) fp32: acc_scale 0', D(32, 32, 64, 64, 64, winograd=1, acc_scale=0.0), 32),
    ('F(2,3) split-half, eight waves: channel stride on the output', D(32, 32, 64, 128, 128, bf16_mfma=3, winograd=1, stats_cpg=4, acc_scale=1.0, ld_out=192), 'cf_conv2d: winograd reads / writes dense tensors with zero padding'),
    ('F(2,3) split-half, eight waves: reflect padding', D(32, 32, 64, 128, 128, bf16_mfma=3, winograd=1, stats_cpg=4, acc_scale=1.0, pad_mode=1), 'cf_conv2d: winograd reads / writes dense tensors with zero padding'),
    ('F(2,3) split-half, eight waves: LEAKY epilogue', D(32, 32, 64, 128, 128, bf16_mfma=3, winograd=1, stats_cpg=4, acc_scale=1.0, epilogue=4), 'cf_conv2d: winograd epilogues are none / residual / SFT'),
    ('F(2,3) split-half, eight waves: acc_scale 0', D(32, 32, 64, 128, 128, bf16_mfma=3, winograd=1, stats_cpg=4, acc_scale=0.0), 'cf_conv2d(winograd, f16x2): acc_scale must be the inverse of the pack-time weight scale (got 0)'),
    ('F(4,3) split-half: channel stride on the output', D(32, 32, 64, 64, 64, bf16_mfma=3, winograd=2, acc_scale=1.0, ld_out=192), 'cf_conv2d(winograd 2): reads / writes dense tensors with zero padding, no split_k'),
    ('F(4,3) split-half: reflect padding', D(32, 32, 64, 64, 64, bf16_mfma=3, winograd=2, acc_scale=1.0, pad_mode=1), 'cf_conv2d(winograd 2): reads / writes dense tensors with zero padding, no split_k'),
    ('F(4,3) split-half: LEAKY epilogue', D(32, 32, 64, 64, 64, bf16_mfma=3, winograd=2, acc_scale=1.0, epilogue=4), 'cf_conv2d(winograd 2): epilogues are none / residual / SFT'),
    ('F(4,3) split-half: acc_scale 0', D(32, 32, 64, 64, 64, bf16_mfma=3, winograd=2, acc_scale=0.0), 'cf_conv2d(winograd 2): acc_scale must be the inverse of the pack-time weight scale (got 0)'),
    ('split-half direct: channel stride on the output', D(64, 64, 64, 64, 64, bf16_mfma=3, acc_scale=1.0, ld_out=192), 'cf_conv2d(f16x2): dense tensors with zero padding only'),
    ('split-half direct: reflect padding', D(64, 64, 64, 64, 64, bf16_mfma=3, acc_scale=1.0, pad_mode=1), 'cf_conv2d(f16x2): dense tensors with zero padding only'),
    ('split-half direct: LEAKY epilogue', D(64, 64, 64, 64, 64, bf16_mfma=3, acc_scale=1.0, epilogue=4), 'cf_conv2d(f16x2): epilogues are none / residual / SFT'),
    ('split-half direct: acc_scale 0', D(64, 64, 64, 64, 64, bf16_mfma=3, acc_scale=0.0), 'cf_conv2d(f16x2): acc_scale must be the inverse of the pack-time weight scale (got 0)'),
]


@pytest.fixture(scope='module')
def native():
    cf_build.build()
    return lib.load()


def test_table_is_within_its_size():
    assert 40 <= len(ROWS) <= 76 and len({r[0] for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize('note,fields,expected', ROWS, ids=[r[0] for r in ROWS])
def test_stats_parts_query(native, note, fields, expected):
    d = lib.ConvDesc(**fields)
    got = native.cf_conv2d_stats_parts(ctypes.byref(d))
    if isinstance(expected, int):
        assert got == expected, (note, got, lib.last_error())
    else:
        assert got == -1 and expected in lib.last_error(), (note, got, lib.last_error())
