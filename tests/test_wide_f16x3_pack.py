"""Host-side weight pack of the split-precision wide 3-D convolution (ops.pack_conv_wino_fused_f16x3): hi + lo reproduce the
fp64 Winograd weights, the scale is an exact power of two, the padding is zero, and the data-gradient pack is the pack of the
transposed and flipped weight.  CPU only."""
import math

import torch

from latentfusion_amd import ops

G = torch.tensor(ops._WINO_G, dtype=torch.float64)


def _wino(w):
    return torch.einsum('ai,bj,ck,omijk->abcom', G, G, G, w.double()).reshape(64, w.shape[0], w.shape[1])


def _unpack(pk, cout, cin):
    hi = pk[:, :, :, 0].double().reshape(64, pk.shape[1], -1)
    lo = pk[:, :, :, 1].double().reshape(64, pk.shape[1], -1)
    return hi, lo


def test_pack_reconstructs_the_fp64_weights():
    w = torch.randn(72, 68, 3, 3, 3, generator=torch.Generator().manual_seed(0)) * 0.3
    pk, eU = ops.pack_conv_wino_fused_f16x3(w)
    assert pk.dtype == torch.float16 and tuple(pk.shape) == (64, 128, 96 // 32, 2, 32)
    U = _wino(w) * 2.0 ** eU
    hi, lo = _unpack(pk, 72, 68)
    rec = (hi + lo)[:, :72, :68]
    # elements whose lo half is a normal f16 number (|u| >= 2^-14 * 2^11): 22 significant bits
    big = U.abs() >= 2.0 ** -3
    assert big.float().mean() > 0.99
    rel = ((rec - U).abs() / U.abs())[big]
    assert rel.max().item() <= 2.0 ** -21
    # and every element to 2^-21 of the largest
    assert (rec - U).abs().max().item() <= 2.0 ** -21 * U.abs().max().item()


def test_pack_scale_is_a_power_of_two_near_2_12():
    for s in (1e-6, 1.0, 3e4):
        w = torch.randn(64, 64, 3, 3, 3, generator=torch.Generator().manual_seed(1)) * s
        pk, eU = ops.pack_conv_wino_fused_f16x3(w)
        assert isinstance(eU, int)
        m = _wino(w).abs().max().item() * 2.0 ** eU
        assert 2.0 ** 11 <= m < 2.0 ** 12
        assert math.ldexp(1.0, eU) == 2.0 ** eU
        assert torch.isfinite(pk.float()).all()


def test_pack_padding_is_zero():
    w = torch.randn(68, 36, 3, 3, 3, generator=torch.Generator().manual_seed(2))
    pk, _ = ops.pack_conv_wino_fused_f16x3(w)
    assert tuple(pk.shape) == (64, 128, 2, 2, 32)
    hi, lo = _unpack(pk, 68, 36)
    assert not hi[:, 68:].any() and not lo[:, 68:].any()                # output channels 68 .. 127
    assert not hi[:, :, 36:].any() and not lo[:, :, 36:].any()          # input channels 36 .. 63


def test_transposed_pack_is_the_pack_of_the_flipped_transpose():
    w = torch.randn(64, 96, 3, 3, 3, generator=torch.Generator().manual_seed(3))
    a, ea = ops.pack_conv_wino_fused_f16x3(w, transpose=True)
    b, eb = ops.pack_conv_wino_fused_f16x3(w.transpose(0, 1).flip(dims=(2, 3, 4)).contiguous())
    assert ea == eb and torch.equal(a, b)
