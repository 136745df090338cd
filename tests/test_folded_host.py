"""No GPU: archs/folded.py -- the folding arithmetic against bn(conv(x)) in float64, the conv bias in the operand order VGG has always used, the
centre-tap embedding, the epilogue table of conv_hip, and its refusal of a stride the kernels do not have."""
import itertools

import pytest
import torch
from torch import nn

from codeformer_amd import ops
from codeformer_amd.archs import folded as FD


def conv_and_bn(bias, seed=0):
    """A 2 -> 3 channel 3x3 conv and an eval-mode BatchNorm with non-trivial affine and running statistics, in float64."""
    gen = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(2, 3, 3, padding=1, bias=bias).double()
    bn = nn.BatchNorm2d(3).double().eval()
    with torch.no_grad():
        for p in list(conv.parameters()) + [bn.weight, bn.bias, bn.running_mean]:
            p.copy_(torch.randn(p.shape, generator=gen, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(3, generator=gen, dtype=torch.float64) + 0.5)
    return conv, bn, torch.randn(1, 2, 5, 4, generator=gen, dtype=torch.float64)


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('with_bn', [True, False])
def test_fold_conv_bn_is_bn_of_conv_in_float64(bias, with_bn):
    conv, bn, x = conv_and_bn(bias)
    bn = bn if with_bn else None
    with torch.no_grad():
        want = conv(x) if bn is None else bn(conv(x))
        w, b = FD.fold_conv_bn(conv, bn)
        assert w.dtype == torch.float64 and w.shape == conv.weight.shape and (b is None) == (not bias and bn is None)
        got = nn.functional.conv2d(x, w, b, padding=1)
    assert float((got - want).abs().max()) <= 1e-12
    fold, deps = FD.folded_layer(conv, bn)
    assert all(torch.equal(a, c) for a, c in zip(fold(), (w, b)) if c is not None)
    assert len(deps) == 1 + bias + 4 * with_bn and deps[0] is conv.weight and all(d is not None for d in deps)
    if bn is not None:
        assert [id(d) for d in deps[-4:]] == [id(d) for d in FD.bn_deps(bn)] == [id(bn.weight), id(bn.bias), id(bn.running_mean), id(bn.running_var)]


def test_conv_bias_folds_in_the_order_vgg_used():
    """The float32 parameters of a conv with a bias, folded in float64 and rounded once: bitwise what vgg_arch computed when it patched the
    bias onto the bias-free fold (t + g * bias, g and t from bn_affine)."""
    conv, bn, _ = conv_and_bn(True, seed=1)
    conv, bn = conv.float(), bn.float()
    g, t = FD.bn_affine(bn, torch.float64)
    want_w = (conv.weight.detach().to(torch.float64) * g.view(-1, 1, 1, 1)).float()
    want_b = (t + g * conv.bias.detach().double()).float()
    w, b = FD.fold_conv_bn(conv, bn, torch.float64)
    assert w.dtype == b.dtype == torch.float64
    assert torch.equal(w.float(), want_w) and torch.equal(b.float(), want_b)
    assert not torch.equal(b.float(), t.float())      # (the bias is in it)


def test_centre_tap():
    w = torch.arange(1.0, 7.0).view(3, 2, 1, 1)
    w3 = FD.centre_tap(w)
    assert w3.shape == (3, 2, 3, 3) and w3.dtype == w.dtype
    assert torch.equal(w3[:, :, 1, 1], w[:, :, 0, 0]) and float(w3.abs().sum()) == float(w.abs().sum()) == 21.0
    conv, bn, _ = conv_and_bn(False, seed=2)
    conv1 = nn.Conv2d(2, 3, 1, bias=False).double()
    assert torch.equal(FD.fold_conv_bn(conv1, bn, embed3=True)[0], FD.centre_tap(FD.fold_conv_bn(conv1, bn)[0]))


def test_epilogue_table():
    """(has_res, has_slope, up2x) -> (epilogue, cf_relu follows): the PReLU epilogues on the plain form, the activation as a launch of its own
    after the sub-pixel form."""
    table = {(False, False, False): (ops.EPI_NONE, False), (True, False, False): (ops.EPI_RESIDUAL, False),
             (False, True, False): (ops.EPI_PRELU, False), (True, True, False): (ops.EPI_RES_PRELU, False),
             (False, False, True): (ops.EPI_NONE, False), (True, False, True): (ops.EPI_RESIDUAL, False),
             (False, True, True): (ops.EPI_NONE, True), (True, True, True): (ops.EPI_RESIDUAL, True)}
    assert len({ops.EPI_NONE, ops.EPI_RESIDUAL, ops.EPI_PRELU, ops.EPI_RES_PRELU}) == 4
    for key in itertools.product((False, True), repeat=3):
        assert FD.epilogue_of(*key) == table[key], key


def test_conv_hip_refuses_other_strides_before_any_launch(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError('an ops function was called')
    for name in ('pack_weight', 'conv2d', 'relu'):
        monkeypatch.setattr(ops, name, no_call)

    class Mod:
        def _packed(self, key, build, *deps):
            raise AssertionError('a pack was asked for')
    conv, bn, _ = conv_and_bn(False)
    x = torch.zeros(1, 5, 4, 2)
    for kw in (dict(stride=3), dict(stride=0), dict(stride=2, up2x=True)):
        with pytest.raises(NotImplementedError):
            FD.conv_hip(Mod(), 'w', FD.folded_layer(conv, bn), x, **kw)
