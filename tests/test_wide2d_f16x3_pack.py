"""Host-side weight pack of the split-precision wide 2-D convolution (ops.pack_conv_wino_fused_f16x3 on [Cout,Cin,3,3]): 16
frequencies, hi + lo reproduce the fp64 Winograd weights, the scale is an exact power of two, the padding is zero, and the
data-gradient pack is the pack of the transposed and flipped weight.  CPU only."""
import math

import torch

from latentfusion_amd import ops

G = torch.tensor(ops._WINO_G, dtype=torch.float64)


def _wino(w):
    return torch.einsum('bj,ck,omjk->bcom', G, G, w.double()).reshape(16, w.shape[0], w.shape[1])


def _unpack(pk):
    hi = pk[:, :, :, 0].double().reshape(16, pk.shape[1], -1)
    lo = pk[:, :, :, 1].double().reshape(16, pk.shape[1], -1)
    return hi, lo


def test_2d_pack_layout_and_reconstruction():
    w = torch.randn(196, 132, 3, 3, generator=torch.Generator().manual_seed(0)) * 0.3
    pk, eU = ops.pack_conv_wino_fused_f16x3(w)
    assert pk.dtype == torch.float16 and tuple(pk.shape) == (16, 256, 160 // 32, 2, 32)
    U = _wino(w) * 2.0 ** eU
    hi, lo = _unpack(pk)
    rec = (hi + lo)[:, :196, :132]
    big = U.abs() >= 2.0 ** -3                                            # lo is a normal f16 number: 22 significant bits
    assert big.float().mean() > 0.99
    assert (((rec - U).abs() / U.abs())[big]).max().item() <= 2.0 ** -21
    assert (rec - U).abs().max().item() <= 2.0 ** -21 * U.abs().max().item()


def test_2d_pack_scale_is_a_power_of_two_near_2_12():
    for s in (1e-6, 1.0, 3e4):
        w = torch.randn(64, 1024, 3, 3, generator=torch.Generator().manual_seed(1)) * s
        pk, eU = ops.pack_conv_wino_fused_f16x3(w)
        assert isinstance(eU, int) and -100 <= eU <= 100
        m = _wino(w).abs().max().item() * 2.0 ** eU
        assert 2.0 ** 11 <= m < 2.0 ** 12
        assert math.ldexp(1.0, eU) == 2.0 ** eU
        assert torch.isfinite(pk.float()).all()


def test_2d_pack_padding_is_zero():
    w = torch.randn(68, 36, 3, 3, generator=torch.Generator().manual_seed(2))
    pk, _ = ops.pack_conv_wino_fused_f16x3(w)
    assert tuple(pk.shape) == (16, 128, 2, 2, 32)
    hi, lo = _unpack(pk)
    assert not hi[:, 68:].any() and not lo[:, 68:].any()                # output channels 68 .. 127
    assert not hi[:, :, 36:].any() and not lo[:, :, 36:].any()          # input channels 36 .. 63


def test_2d_transposed_pack_is_the_pack_of_the_flipped_transpose():
    w = torch.randn(64, 96, 3, 3, generator=torch.Generator().manual_seed(3))
    a, ea = ops.pack_conv_wino_fused_f16x3(w, transpose=True)
    b, eb = ops.pack_conv_wino_fused_f16x3(w.transpose(0, 1).flip(dims=(2, 3)).contiguous())
    assert ea == eb and torch.equal(a, b) and tuple(a.shape) == (16, 128, 2, 2, 32)


def test_route_table_is_well_formed():
    for (ci, co, h, w), n_min in ops.WIDE2D_F16X3_ROUTE.items():
        assert ci >= 64 and co >= 64 and ci % 4 == 0 and co % 4 == 0 and h >= 1 and w >= 1 and n_min >= 1
        assert ops._wide2d_f16x3_routed(ci, co, h, w, n_min) and not ops._wide2d_f16x3_routed(ci, co, h, w, n_min - 1)
    assert not ops._wide2d_f16x3_routed(64, 64, 128, 128, 128)          # measured slower: stays on the fp32 pair
