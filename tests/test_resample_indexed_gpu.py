"""The indexed resampler (lf_resample3d_fwd_indexed / lf_resample3d_bwd_coef_indexed): N = 7 rows over K = 3 volumes through
the table [2,0,0,1,2,1,0].  Every row's output is BIT-identical to lf_resample3d_fwd(vol_n = 1) on that row's volume, every
row's 18 coefficient sums to lf_resample3d_bwd_coef(N = part_n) on a group of rows of its volume; the same comparisons
against a permuted table fail (the table is what selects the volume), two runs agree, and bad arguments come back as
negative LF_E* codes with nothing launched.  Shapes: 16 channels (the specialised gather; coefficient gradient with fewer and
with at least 256 voxels per block), 256 channels (vec4 forms), 6 channels (scalar forms); S = 13 has ragged tiles."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LF_EINVAL, LF_ENOSPC = -1, -3
O2C, C2O = 0, 1
K, N = 3, 7
TABLE = [2, 0, 0, 1, 2, 1, 0]
PERMUTED = [0, 2, 2, 0, 1, 0, 1]          # every row names another volume than TABLE does


def _s():
    return torch.cuda.current_stream().cuda_stream


def _coefs(kind, n, gen):
    """Maps that keep most samples inside the volume and some outside (border clip), different per row."""
    c = torch.zeros(n, 20)
    if kind == O2C:
        c[:, 0:3] = -0.8 + 0.05 * torch.randn(n, 3, generator=gen)
        c[:, 3:6] = torch.tensor([1.6, 0.0, 0.0]) + 0.05 * torch.randn(n, 3, generator=gen)
        c[:, 6:9] = torch.tensor([0.0, 1.6, 0.0]) + 0.05 * torch.randn(n, 3, generator=gen)
        c[:, 9:12] = torch.tensor([0.0, 0.0, 1.6]) + 0.05 * torch.randn(n, 3, generator=gen)
        c[:, 12:18] = 0.05 * torch.randn(n, 6, generator=gen)
    else:
        c[:, :16] = (torch.eye(4) * torch.tensor([1.1, 1.1, 1.1, 1.0])).reshape(1, 16) + 0.05 * torch.randn(n, 16, generator=gen)
    return c.to(DEV).contiguous()


def _volumes(C, S, gen):
    from latentfusion_amd import ops
    return ops.cl(torch.randn(K, C, S, S, S, generator=gen).to(DEV))


def _fwd_rows(L, vols, table, cf, kind):
    """lf_resample3d_fwd(vol_n = 1) row by row on the volume the table names."""
    from latentfusion_amd import ops
    _, C, S = vols.shape[:3]
    rows = []
    for i, k in enumerate(table):
        out = ops.empty_cl((1, C, S, S, S), DEV)
        assert L.lf_resample3d_fwd(vols[k:k + 1].data_ptr(), 1, cf[i:i + 1].data_ptr(), kind, out.data_ptr(), 1, S, S, S, C, _s()) == 0
        rows.append(out)
    torch.cuda.synchronize()
    return torch.cat(rows)


@pytest.mark.parametrize('S', [8, 13, 32])
@pytest.mark.parametrize('C', [16, 256, 6])
@pytest.mark.parametrize('kind', [O2C, C2O])
def test_indexed_forward_is_bit_identical_to_the_one_volume_forward_per_row(kind, C, S):
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    gen = torch.Generator().manual_seed(1000 * kind + 10 * C + S)
    vols = _volumes(C, S, gen)
    cf = _coefs(kind, N, gen)
    want = _fwd_rows(L, vols, TABLE, cf, kind)
    got = ops.resample_fwd_indexed(vols, ops.volume_table(TABLE, K, DEV), cf, kind)
    again = ops.resample_fwd_indexed(vols, ops.volume_table(TABLE, K, DEV), cf, kind)
    torch.cuda.synchronize()
    assert got.shape == want.shape and got.abs().sum() > 0
    for i in range(N):
        assert torch.equal(got[i], want[i]), i
    assert torch.equal(got, again)                                   # run to run
    # control: through another table the same comparison fails in every row
    other = ops.resample_fwd_indexed(vols, ops.volume_table(PERMUTED, K, DEV), cf, kind)
    torch.cuda.synchronize()
    for i in range(N):
        assert not torch.equal(other[i], want[i]), i


def _bwd_groups(L, gout, vols, table, cf, part_n):
    """lf_resample3d_bwd_coef with N = part_n on groups of rows that share a volume (a short group is filled up by repeating its
    rows: a row's sums depend on the partition, not on its group mates)."""
    _, C, S = vols.shape[:3]
    want = torch.empty(len(table), 18, device=DEV)
    nb = L.lf_resample3d_bwd_coef_scratch_bytes(part_n, S, S, S)
    sc = torch.empty(nb // 4 + 1, device=DEV)
    for k in range(vols.shape[0]):
        rows = [i for i, t in enumerate(table) if t == k]
        for b in range(0, len(rows), part_n):
            chunk = rows[b:b + part_n]
            grp = [chunk[j % len(chunk)] for j in range(part_n)]
            g = gout[grp].contiguous(memory_format=torch.channels_last_3d)
            c = cf[grp].contiguous()
            res = torch.empty(part_n, 18, device=DEV)
            assert L.lf_resample3d_bwd_coef(g.data_ptr(), vols[k:k + 1].data_ptr(), 1, c.data_ptr(), res.data_ptr(), sc.data_ptr(), nb,
                                            part_n, S, S, S, C, _s()) == 0
            torch.cuda.synchronize()
            want[chunk] = res[:len(chunk)]
    return want


@pytest.mark.parametrize('part_n', [1, 3])
@pytest.mark.parametrize('C,S', [(16, 8), (16, 13), (16, 32), (16, 64), (256, 8), (256, 13), (256, 32), (6, 8), (6, 13), (6, 32)])
def test_indexed_coefficient_gradient_is_bit_identical_to_bwd_coef_per_group(C, S, part_n):
    """(16, 64) with part_n = 3 reaches 256 voxels per block, the per-voxel dedup kernel; the smaller 16-channel shapes run the
    four-lanes-per-voxel kernel.)"""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    gen = torch.Generator().manual_seed(7 * C + S + part_n)
    vols = _volumes(C, S, gen)
    gout = ops.cl(torch.randn(N, C, S, S, S, generator=gen).to(DEV))
    cf = _coefs(O2C, N, gen)
    want = _bwd_groups(L, gout, vols, TABLE, cf, part_n)
    got = ops.resample_bwd_coef_indexed(gout, vols, ops.volume_table(TABLE, K, DEV), cf, part_n)
    again = ops.resample_bwd_coef_indexed(gout, vols, ops.volume_table(TABLE, K, DEV), cf, part_n)
    torch.cuda.synchronize()
    assert got.abs().sum() > 0
    for i in range(N):
        assert torch.equal(got[i], want[i]), i
    assert torch.equal(got, again)
    other = ops.resample_bwd_coef_indexed(gout, vols, ops.volume_table(PERMUTED, K, DEV), cf, part_n)
    torch.cuda.synchronize()
    for i in range(N):
        assert not torch.equal(other[i], want[i]), i


def test_one_volume_table_equals_the_broadcast_forms():
    """vol_n = 1 with an all-zero table is lf_resample3d_fwd / lf_resample3d_bwd_coef_part with one broadcast volume."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    C, S, n = 16, 32, 2
    gen = torch.Generator().manual_seed(5)
    vol = ops.cl(torch.randn(1, C, S, S, S, generator=gen).to(DEV))
    gout = ops.cl(torch.randn(N, C, S, S, S, generator=gen).to(DEV))
    cf = _coefs(O2C, N, gen)
    table = ops.volume_table([0] * N, 1, DEV)
    want = ops.empty_cl((N, C, S, S, S), DEV)
    assert L.lf_resample3d_fwd(vol.data_ptr(), 1, cf.data_ptr(), O2C, want.data_ptr(), N, S, S, S, C, _s()) == 0
    wantg = torch.empty(N, 18, device=DEV)
    nb = L.lf_resample3d_bwd_coef_part_scratch_bytes(N, n, S, S, S)
    assert L.lf_resample3d_bwd_coef_indexed_scratch_bytes(N, n, S, S, S) == nb
    sc = torch.empty(nb // 4 + 1, device=DEV)
    assert L.lf_resample3d_bwd_coef_part(gout.data_ptr(), vol.data_ptr(), 1, cf.data_ptr(), wantg.data_ptr(), sc.data_ptr(), nb,
                                         N, S, S, S, C, n, _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ops.resample_fwd_indexed(vol, table, cf), want)
    assert torch.equal(ops.resample_bwd_coef_indexed(gout, vol, table, cf, n), wantg)


def test_indexed_entry_points_reject_bad_arguments_before_launching():
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    C, S = 16, 16
    gen = torch.Generator().manual_seed(3)
    vols = _volumes(C, S, gen)
    gout = ops.cl(torch.randn(N, C, S, S, S, generator=gen).to(DEV))
    cf = _coefs(O2C, N, gen)
    table = ops.volume_table(TABLE, K, DEV)
    out = torch.full((N, C, S, S, S), 7.0, device=DEV)
    gc = torch.full((N, 18), 7.0, device=DEV)

    def fwd(vol=vols.data_ptr(), vol_n=K, idx=table.data_ptr(), coef=cf.data_ptr(), kind=O2C, dst=out.data_ptr(), n=N):
        return L.lf_resample3d_fwd_indexed(vol, vol_n, idx, coef, kind, dst, n, S, S, S, C, _s())

    assert fwd(idx=None) == LF_EINVAL                                 # no table
    assert fwd(vol=None) == LF_EINVAL and fwd(coef=None) == LF_EINVAL and fwd(dst=None) == LF_EINVAL
    assert fwd(vol_n=0) == LF_EINVAL and fwd(vol_n=-2) == LF_EINVAL
    assert fwd(n=0) == LF_EINVAL and fwd(kind=7) == LF_EINVAL
    assert fwd(idx=table.data_ptr() + 2) < 0                          # a table that is not int32-aligned

    need = L.lf_resample3d_bwd_coef_indexed_scratch_bytes(N, 1, S, S, S)
    assert need > 0 and L.lf_resample3d_bwd_coef_indexed_scratch_bytes(N, 0, S, S, S) == 0
    scr = torch.empty(need // 4 + 1, device=DEV)

    def bwd(g=gout.data_ptr(), vol=vols.data_ptr(), vol_n=K, idx=table.data_ptr(), coef=cf.data_ptr(), dst=gc.data_ptr(),
            scratch=scr.data_ptr(), nbytes=need, n=N, part_n=1):
        return L.lf_resample3d_bwd_coef_indexed(g, vol, vol_n, idx, coef, dst, scratch, nbytes, n, S, S, S, C, part_n, _s())

    assert bwd(idx=None) == LF_EINVAL
    assert bwd(g=None) == LF_EINVAL and bwd(vol=None) == LF_EINVAL and bwd(dst=None) == LF_EINVAL and bwd(scratch=None) == LF_EINVAL
    assert bwd(vol_n=0) == LF_EINVAL
    assert bwd(part_n=0) == LF_EINVAL and bwd(part_n=-1) == LF_EINVAL
    assert bwd(n=0) == LF_EINVAL
    assert bwd(nbytes=need - 4) == LF_ENOSPC
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((gc == 7.0).all())       # nothing was launched on the rejected calls
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any()) and not bool((gc == 7.0).any())


def test_the_wrapper_rejects_a_table_entry_outside_the_volumes():
    from latentfusion_amd import ops
    with pytest.raises(ValueError, match='outside'):
        ops.volume_table([0, 1, K], K, DEV)                           # index >= vol_n
    with pytest.raises(ValueError, match='outside'):
        ops.volume_table([0, -1, 1], K, DEV)
    vols = _volumes(16, 8, torch.Generator().manual_seed(1))
    cf = _coefs(O2C, N, torch.Generator().manual_seed(2))
    with pytest.raises(ValueError, match='rows'):
        ops.resample_fwd_indexed(vols, ops.volume_table([0, 1], K, DEV), cf)      # 2 table rows, 7 coefficient blocks
    with pytest.raises(ValueError):
        ops.resample_fwd_indexed(vols, torch.zeros(N, dtype=torch.int64, device=DEV), cf)   # not an int32 table
