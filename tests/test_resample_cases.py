"""tests/resample_cases.py checked without a GPU: the explicit fp64 restatement of the 3-D resampler against F.grid_sample and its
autograd in fp64 on every finite case of tests/test_resample_fp64_gpu.py; the conditions the lattice family's tight bounds rest
on (fp32 positions equal to the fp64 ones, both sides of the border clamp present); the voxels-per-block rule that the
coefficient-gradient cases count on; and every misreading missing the bounds by 10x or more when the fp32 restatement stands in
for the kernel (a condition on the inputs, not a measurement)."""
import pytest
import torch

import resample_cases as K

FINITE = K.finite_cases()
_id = lambda k: f'{k[0]}-{"o2c" if k[1] == K.O2C else "c2o"}-{"x".join(map(str, k[2]))}-C{k[3]}-N{k[4]}-v{k[5]}'  # noqa: E731


@pytest.mark.parametrize('key', FINITE, ids=_id)
def test_restatement_is_grid_sample_in_fp64(key):
    family, kind, dims, C, N, vol_n = key
    c = K.case(*key)
    ref = c['ref']
    gs = K.grid_sample_restatement(c['vol'], c['cf'], kind, dims, c['gout'], dtype=torch.float64)
    assert (ref['fwd'] - gs['fwd']).abs().max().item() <= 1e-12
    # gradients: rounding of fp64 sums in another order, measured against the sums of absolute terms
    assert ((ref['gvol'] - gs['gvol']).abs() <= 1e-12 * (1 + ref['gvol_abs'])).all()
    if kind == K.O2C:
        assert ((ref['gcoef'] - gs['gcoef']).abs() <= 1e-12 * (1 + ref['A'])).all(), (ref['gcoef'] - gs['gcoef']).abs().max()
    # |gcoef_j| can never exceed its yardstick
    assert (ref['gcoef'].abs() <= ref['A'] * (1 + 1e-12) + 1e-300).all()


@pytest.mark.parametrize('key', [k for k in FINITE if k[0] != 'general'], ids=_id)
def test_lattice_positions_are_exact_in_fp32_and_the_clamp_is_exercised(key):
    family, kind, dims, C, N, vol_n = key
    D, H, W = dims
    _, cf, _ = K.inputs(*key)
    p32, u32 = K.positions(cf, kind, dims)
    p64, u64 = K.positions(cf.double(), kind, dims)
    assert p32.dtype == torch.float32 and torch.equal(p32.double(), p64) and torch.equal(u32.double(), u64)
    g = K.grid(cf.double(), kind, dims)
    sizes = torch.tensor([W, H, D], dtype=torch.float64)
    assert ((g + 1).abs() * sizes < 256).all()
    if family == 'lattice':
        share = K.clamped_share(cf, kind, dims).mean(0)
        for axis, S in enumerate((W, H, D)):
            if S > 1:
                assert 0.2 <= share[axis].item() <= 0.8, (axis, share)


def test_on_face_case_sits_on_the_faces():
    _, cf, _ = K.inputs('on_face', K.O2C, (3, 2, 65), 16, 3, 1)
    p, _ = K.positions(cf.double(), K.O2C, (3, 2, 65))
    assert set(p[..., 1].unique().tolist()) == {0.0, 1.0}


def test_voxels_per_block_of_the_coefficient_gradient_cases():
    for dims, N, vol_n, vpb, form in K.VPB_CASES:
        assert K.bwd_vox_per_block(dims[0] * dims[1] * dims[2], N) == vpb, (dims, N)
    for N, _ in K.NV:
        assert K.bwd_vox_per_block(5 * 9 * 17, N) == 64
    assert K.bwd_vox_per_block(128 ** 3, 8) == 4096                 # the headline shape


def test_degenerate_maps_do_what_the_header_says():
    D, H, W = K.BASE
    for C in (16, 3):
        c = K.degenerate_case('nan', C)
        taps = c['ref']['taps'].reshape(3, D, H, W, 8)
        x, y, z = taps % W, (taps // W) % H, taps // (W * H)
        # tap index = 4 cz + 2 cy + cx: the lower corner is voxel 0 (the upper one, voxel 1, has weight 0)
        assert (x[0][..., 0::2] == 0).all() and (y[1][..., [0, 1, 4, 5]] == 0).all() and (z[2][..., :4] == 0).all()
        assert (x[0][..., 1::2] == 1).all() and (y[1][..., [2, 3, 6, 7]] == 1).all() and (z[2][..., 4:] == 1).all()
        assert (c['ref']['gcoef'][0, 0::3] == 0).all() and (c['ref']['gcoef'][1, 1::3] == 0).all() and (c['ref']['gcoef'][2, 2::3] == 0).all()
        c = K.degenerate_case('inf', C)
        taps = c['ref']['taps'].reshape(3, D, H, W, 8)
        x, y, z = taps % W, (taps // W) % H, taps // (W * H)
        assert (x[0] == W - 1).all() and (y[1][..., [0, 1, 4, 5]] == 0).all()
        assert (z[2][:, :, 0, :4] == 0).all() and (z[2][:, :, 1:] == D - 1).all()
        c = K.degenerate_case('far_outside', C)
        assert (c['ref']['gcoef'] == 0).all() and (c['ref']['A'] == 0).all()
        v = c['vol'][0].double()
        assert torch.equal(c['ref']['fwd'][0], v[D - 1, 0, W - 1].expand(D, H, W, C))
        c = K.degenerate_case('behind_camera', C)
        g = K.grid(c['cf'].double(), K.C2O, K.BASE)
        assert torch.isinf(g).any() and torch.isnan(g).any() and torch.isfinite(c['ref']['fwd']).all()
        c = K.degenerate_case('constant', C)
        assert (c['ref']['taps'] == c['ref']['taps'][:, :1]).all()


@pytest.mark.parametrize('name', K.MISREADINGS)
def test_misreadings_miss_the_bounds_by_10x(name):
    out, key = K.MISREAD_CASES[name]
    c = K.case(*key)
    stand_in = c['r32'][out]
    assert K.misread_ratio(name, stand_in) >= 10.0, K.misread_ratio(name, stand_in)
    # ... on a case where the stand-in itself is accepted against the true reference
    if out == 'fwd':
        assert (stand_in.double() - c['ref']['fwd']).abs().max().item() < 1e-5
    else:
        assert K.gcoef_ratio(stand_in, c['ref'], key[0], c['r32']) <= 1.0
