"""The forms of the deterministic splat (csrc/splat.hip) at small shapes that leave tiles partial and empty.

lf_resample3d_bwd_vol_det and lf_resample3d_bwd_vol_det_io add the same 64-bit integers in every form -- global atomics, source tiles
found by box culling, source tiles fed from binned lists (a lane quad or 16 lanes per list entry, one pass or several) -- so every form
must give the bits of the global-atomic one.  That is agreement; the global-atomic form itself is held against fp64 autograd of
F.grid_sample.  The coefficients are hand-made so that what they exercise is known beforehand: a confined map that leaves whole source
tiles empty, and an overshooting one whose samples clamp on all six faces."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N, C = 3, 16
# (9, 13, 7): no axis fills a 4x8x8 source tile or a 4x4x4 output block, one partial tile along x.  (20, 24, 40): several 16^3
# super-blocks along x, and tiles with more than 256 list entries: the two-ahead prefetch of the binned kernel runs past its first
# iterations and through its tail.
SHAPES = [(9, 13, 7), (20, 24, 40)]
KINDS = ['o2c', 'c2o']
# per axis g = A + B t, t the lattice coordinate in [0, 1]; OFF * n is added for sample n
CSETS = {'confined': (-0.9, 0.4, -0.01),      # voxel coordinates ((g + 1) S - 1) / 2 <= 0.25 S - 0.5: the far tiles stay empty
         'overshoot': (-1.6, 3.2, 0.0)}       # g in [-1.6, 1.6]: t < 3/16 and t > 13/16 of every axis clamp onto the faces


def close(a, b, atol=1e-4, rtol=1e-4):        # the single-op bar of tests/test_ops_gpu.py
    torch.testing.assert_close(a.detach().cpu().contiguous(), b.detach().cpu().contiguous(), atol=atol, rtol=rtol)


def _coefs(kind, cset):
    """(N, LF_MAP_COEFS) fp32 on the host: the axis maps g = A + B t as an object -> camera block (rows cf[c] + cf[3+c] a + cf[6+c] b +
    cf[9+c] k, no cross terms) or as a camera -> object one (diagonal 4x4 on the lattice l = 2 t - 1, last row (0, 0, 0, 1))."""
    from latentfusion_amd import _lib
    a0, b0, off = CSETS[cset]
    cf = torch.zeros(N, _lib.LF_MAP_COEFS)
    for n in range(N):
        for c in range(3):
            if kind == 'o2c':
                cf[n, c] = a0 + off * n
                cf[n, 3 + 3 * c + c] = b0
            else:
                cf[n, 4 * c + c] = b0 / 2
                cf[n, 4 * c + 3] = a0 + b0 / 2 + off * n
        if kind == 'c2o':
            cf[n, 15] = 1.0
    return cf


def _grid64(kind, cf, shape):
    """(N, D, H, W, 3) fp64 sampling grid of the coefficient blocks (include/lf_hip.h), lattice by torch.linspace in fp32."""
    D, H, W = shape
    k, b, a = torch.meshgrid(torch.linspace(0.0, 1.0, D), torch.linspace(0.0, 1.0, H), torch.linspace(0.0, 1.0, W), indexing='ij')
    a, b, k = a.double(), b.double(), k.double()
    c = cf.double()
    grids = []
    for n in range(N):
        if kind == 'o2c':
            g = [c[n, i] + c[n, 3 + i] * a + c[n, 6 + i] * b + c[n, 9 + i] * k + c[n, 12 + i] * a * k + c[n, 15 + i] * b * k for i in range(3)]
        else:
            lx, ly, lz = 2 * a - 1, 2 * b - 1, 2 * k - 1
            r = [c[n, 4 * i] * lx + c[n, 4 * i + 1] * ly + c[n, 4 * i + 2] * lz + c[n, 4 * i + 3] for i in range(4)]
            g = [r[0] / r[3], r[1] / r[3], r[2]]
        grids.append(torch.stack(g, dim=-1))
    return torch.stack(grids, dim=0)


def _scratch(L, shape):
    D, H, W = shape
    nb = max(L.lf_resample3d_bwd_vol_det_scratch_bytes(v, D, H, W, C) for v in (1, N))
    nb = max([nb] + [L.lf_resample3d_bwd_vol_det_io_scratch_bytes(v, N, D, H, W) for v in (1, N)])
    return torch.empty(nb // 8 + 1, device=DEV, dtype=torch.int64)


def _det(L, gout, cf, kind, vol_n, shape, scr, variant):
    from latentfusion_amd import _lib, ops
    D, H, W = shape
    gv = ops.empty_cl((vol_n, C, D, H, W), DEV)
    prev = L.lf_set_tuning(4, variant)
    try:
        _lib.check(L.lf_resample3d_bwd_vol_det(gout.data_ptr(), cf.data_ptr(), _KIND[kind], gv.data_ptr(), vol_n, scr.data_ptr(), scr.numel() * 8,
                                               N, D, H, W, C, torch.cuda.current_stream().cuda_stream), 'bwd_vol_det')
    finally:
        L.lf_set_tuning(4, prev)
    return gv


_KIND = {'o2c': 0, 'c2o': 1}                   # LF_MAP_O2C, LF_MAP_C2O


@functools.lru_cache(maxsize=None)
def _case(shape, kind, cset):
    """Inputs of a case and the reference gradients (global-atomic form, lf_set_tuning(4, 1)) for vol_n = 1 and N; computed once."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    D, H, W = shape
    gen = torch.Generator().manual_seed(1000 * D + 10 * W + len(kind + cset))
    cf = _coefs(kind, cset).to(DEV)
    gout = ops.cl(ops.round_bf16(torch.randn(N, C, D, H, W, generator=gen).to(DEV)))     # O(1), bf16-representable: io & 1 is exact
    scr = _scratch(L, shape)
    ref = {vol_n: _det(L, gout, cf, kind, vol_n, shape, scr, 1) for vol_n in (1, N)}
    torch.cuda.synchronize()
    return cf, gout, scr, ref


def _b16(t):
    return t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)


@pytest.mark.parametrize('cset', list(CSETS))
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_inputs_exercise_empty_tiles_and_clamping(shape, kind, cset):
    """The conditions that make the hand-made inputs meaningful, on the reference gradient."""
    _, _, _, ref = _case(shape, kind, cset)
    for vol_n in (1, N):
        r = ref[vol_n]
        assert r.abs().max().item() > 0
        if cset == 'confined' and shape == (20, 24, 40):
            # x <= 0.25 * 40 - 0.5 = 9.5: upper corners at x <= 10, so every 4x8x8-aligned source tile with x-origin >= 16 is empty
            assert torch.count_nonzero(r[..., 16:]).item() == 0, vol_n
        if cset == 'overshoot':
            # clamped samples pile up on the faces: the corner voxel against the median of the interior
            assert r[:, :, 0, 0, 0].abs().max().item() > r[:, :, 1:-1, 1:-1, 1:-1].abs().median().item(), vol_n


@pytest.mark.parametrize('cset', list(CSETS))
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_splat_forms_bit_identical(shape, kind, cset):
    """Every form of both entry points gives the bits of the global-atomic form (rounded once to bf16 where the output is stored so)."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    D, H, W = shape
    cf, gout, scr, ref = _case(shape, kind, cset)
    s = torch.cuda.current_stream().cuda_stream
    for vol_n in (1, N):
        want = ref[vol_n]
        assert torch.equal(_det(L, gout, cf, kind, vol_n, shape, scr, 2), want), vol_n
        for io in range(4):
            gi = _b16(gout) if io & 1 else gout
            want_io = want.to(torch.bfloat16) if io & 2 else want
            # key 4 = 2: binned lists, a lane quad per entry; 3: box culling; 4: binned, 16 lanes per entry; key 6 = 2: the binned form in
            # two passes (a volume per sample) or its documented fall-back to box culling (one shared volume)
            for variant, cap in ((2, 0), (3, 0), (4, 0), (2, 2)):
                gv = ops.empty_cl16((vol_n, C, D, H, W), DEV, bool(io & 2))
                prev4, prev6 = L.lf_set_tuning(4, variant), L.lf_set_tuning(6, cap)
                try:
                    _lib.check(L.lf_resample3d_bwd_vol_det_io(gi.data_ptr(), cf.data_ptr(), _KIND[kind], gv.data_ptr(), vol_n, scr.data_ptr(),
                                                              scr.numel() * 8, N, D, H, W, io, s), 'bwd_vol_det_io')
                finally:
                    L.lf_set_tuning(4, prev4)
                    L.lf_set_tuning(6, prev6)
                assert torch.equal(gv, want_io), (vol_n, io, variant, cap)


@pytest.mark.parametrize('cset', list(CSETS))
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES)
def test_reference_form_vs_fp64_grid_sample(shape, kind, cset):
    """The independent anchor: the global-atomic form against fp64 autograd of F.grid_sample(padding_mode='border',
    align_corners=False) on the grid the coefficients define."""
    D, H, W = shape
    cf, gout, _, ref = _case(shape, kind, cset)
    vol = torch.zeros(N, C, D, H, W, dtype=torch.float64, requires_grad=True)
    out = torch.nn.functional.grid_sample(vol, _grid64(kind, cf.cpu(), shape), mode='bilinear', padding_mode='border', align_corners=False)
    out.backward(gout.cpu().double())
    close(ref[N], vol.grad.float())
    close(ref[1], vol.grad.sum(dim=0, keepdim=True).float())


@pytest.mark.parametrize('vol_n', [1, N])
def test_undersized_scratch_is_refused(vol_n):
    """A buffer 8 bytes short of an entry's own query: LF_ENOSPC, nothing launched, the output untouched."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    shape = SHAPES[0]
    D, H, W = shape
    cf, gout, scr, _ = _case(shape, 'o2c', 'confined')
    s = torch.cuda.current_stream().cuda_stream
    gv = ops.empty_cl((vol_n, C, D, H, W), DEV).fill_(7.0)
    nb = L.lf_resample3d_bwd_vol_det_scratch_bytes(vol_n, D, H, W, C)
    assert 8 < nb <= scr.numel() * 8
    assert L.lf_resample3d_bwd_vol_det(gout.data_ptr(), cf.data_ptr(), 0, gv.data_ptr(), vol_n, scr.data_ptr(), nb - 8, N, D, H, W, C, s) == -3
    nb = L.lf_resample3d_bwd_vol_det_io_scratch_bytes(vol_n, N, D, H, W)
    assert 8 < nb <= scr.numel() * 8
    assert L.lf_resample3d_bwd_vol_det_io(gout.data_ptr(), cf.data_ptr(), 0, gv.data_ptr(), vol_n, scr.data_ptr(), nb - 8, N, D, H, W, 0, s) == -3
    torch.cuda.synchronize()
    assert torch.equal(gv, torch.full_like(gv, 7.0))


def test_tuning_keys_of_the_splat():
    """lf_set_tuning key 4 takes 1..4, key 6 takes >= 0; other values leave the setting; the previous value comes back."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    start4, start6 = L.lf_set_tuning(4, 2), L.lf_set_tuning(6, 0)
    try:
        prev = 2
        for v in (1, 2, 3, 4):
            assert L.lf_set_tuning(4, v) == prev
            prev = v
        for bad in (0, 5):
            assert L.lf_set_tuning(4, bad) == 4                     # refused: the value stays ...
        assert L.lf_set_tuning(4, 2) == 4                           # ... as the next call shows
        assert L.lf_set_tuning(6, 3) == 0
        assert L.lf_set_tuning(6, -1) == 3
        assert L.lf_set_tuning(6, 0) == 3
    finally:
        L.lf_set_tuning(4, start4)
        L.lf_set_tuning(6, start6)
