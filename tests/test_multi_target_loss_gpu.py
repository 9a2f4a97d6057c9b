"""The several-target pose-loss entry points (lf_pose_loss_fwd_mt / _fwd_masked_mt / _bwd_mt) and the coefficient gradient
with a caller-fixed partition (lf_resample3d_bwd_coef_part): per target BIT-identical to the single-target entry points
called on that target's rows alone, and bad arguments rejected with LF_E* codes before anything is launched."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LF_EINVAL, LF_ENOSPC = -1, -3
T, h, w, H, W = 3, 24, 20, 48, 64


def _s():
    return torch.cuda.current_stream().cuda_stream


def _frames(gen):
    """T different target frames [T][H*W]: discs of different centres / radii, depth 1..1.1 inside."""
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing='ij')
    masks, depths = [], []
    for t in range(T):
        m = (((xx - 24 - 6 * t) ** 2 + (yy - 22 + 3 * t) ** 2) <= (14 + 3 * t) ** 2).float()
        masks.append(m.reshape(-1))
        depths.append(((1.0 + 0.1 * torch.rand(H, W, generator=gen)) * m).reshape(-1))
    return torch.stack(depths).to(DEV).contiguous(), torch.stack(masks).to(DEV).contiguous()


def _inputs(N, gen):
    logits = (torch.randn(N, h * w, 2, generator=gen) * 2.0).to(DEV).contiguous()
    coefs = torch.zeros(N, 24)
    coefs[:, :18] = torch.randn(N, 18, generator=gen)
    # crop position of frame pixel (x, y) = (ax x + bx, ay y + by): the crop covers a box of the frame, slightly different per row
    coefs[:, 18] = (w / 36.0) * (1 + 0.1 * torch.rand(N, generator=gen))
    coefs[:, 19] = -8.0 * (w / 36.0) + torch.randn(N, generator=gen)
    coefs[:, 20] = (h / 30.0) * (1 + 0.1 * torch.rand(N, generator=gen))
    coefs[:, 21] = -6.0 * (h / 30.0) + torch.randn(N, generator=gen)
    coefs[:, 22] = 0.05 + 0.01 * torch.rand(N, generator=gen)
    coefs[:, 23] = 1.05 + 0.01 * torch.rand(N, generator=gen)
    return logits, coefs.to(DEV).contiguous()


def _scratch(L, N):
    nb = L.lf_pose_loss_scratch_bytes(N, h, w, H, W)
    return torch.empty(nb // 4 + 1, device=DEV), nb


def _single(L, logits, coefs, td, tm, weights):
    """lf_pose_loss_fwd / _fwd_masked / _bwd on one target's rows."""
    N = logits.shape[0]
    out = {k: torch.empty(N, 8, device=DEV) for k in ('sums', 'losses', 'gsums', 'msums', 'mlosses')}
    sc, nb = _scratch(L, N)
    assert L.lf_pose_loss_fwd(logits.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr(), weights.data_ptr(),
                              out['sums'].data_ptr(), out['losses'].data_ptr(), out['gsums'].data_ptr(), sc.data_ptr(), nb,
                              N, h, w, H, W, _s()) == 0
    assert L.lf_pose_loss_fwd_masked(logits.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr(), weights.data_ptr(),
                                     out['msums'].data_ptr(), out['mlosses'].data_ptr(), sc.data_ptr(), nb, N, h, w, H, W,
                                     _s()) == 0
    out['glogits'] = torch.empty_like(logits)
    out['gcoefs'] = torch.zeros(N, 24, device=DEV)
    assert L.lf_pose_loss_bwd(logits.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr(), out['gsums'].data_ptr(),
                              out['glogits'].data_ptr(), out['gcoefs'].data_ptr(), sc.data_ptr(), nb, N, h, w, H, W, _s()) == 0
    return out


@pytest.mark.parametrize('n', [1, 4])
def test_mt_pose_loss_is_bit_identical_to_single_target_per_target(n):
    from latentfusion_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(10 + n)
    N = T * n
    td, tm = _frames(gen)
    logits, coefs = _inputs(N, gen)
    weights = torch.tensor([1.0, 0.3, 0.2, 0.4], device=DEV)
    got = {k: torch.empty(N, 8, device=DEV) for k in ('sums', 'losses', 'gsums', 'msums', 'mlosses')}
    sc, nb = _scratch(L, N)
    assert L.lf_pose_loss_fwd_mt(logits.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr(), weights.data_ptr(),
                                 got['sums'].data_ptr(), got['losses'].data_ptr(), got['gsums'].data_ptr(), sc.data_ptr(), nb,
                                 N, T, n, h, w, H, W, _s()) == 0
    assert L.lf_pose_loss_fwd_masked_mt(logits.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr(), weights.data_ptr(),
                                        got['msums'].data_ptr(), got['mlosses'].data_ptr(), sc.data_ptr(), nb,
                                        N, T, n, h, w, H, W, _s()) == 0
    got['glogits'] = torch.empty_like(logits)
    got['gcoefs'] = torch.zeros(N, 24, device=DEV)
    assert L.lf_pose_loss_bwd_mt(logits.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr(), got['gsums'].data_ptr(),
                                 got['glogits'].data_ptr(), got['gcoefs'].data_ptr(), sc.data_ptr(), nb,
                                 N, T, n, h, w, H, W, _s()) == 0
    for t in range(T):
        r = slice(t * n, (t + 1) * n)
        want = _single(L, logits[r].contiguous(), coefs[r].contiguous(), td[t].contiguous(), tm[t].contiguous(), weights)
        torch.cuda.synchronize()
        for k, v in want.items():
            assert torch.equal(got[k][r], v), (t, k)
        # the frames differ, so a row scored against another target's frame would not have matched
        assert t == 0 or not torch.equal(got['sums'][r], got['sums'][:n])
    assert torch.isfinite(got['glogits']).all() and got['gcoefs'][:, 18:].abs().sum() > 0


def _o2c_coefs(N, gen):
    """O2C blocks whose sampling grid stays inside the volume: g = c0 + c1 a + c2 b + c3 k + small bilinear terms."""
    c = torch.zeros(N, 20)
    c[:, 0:3] = -0.8 + 0.05 * torch.randn(N, 3, generator=gen)
    c[:, 3:6] = torch.tensor([1.6, 0.0, 0.0]) + 0.05 * torch.randn(N, 3, generator=gen)
    c[:, 6:9] = torch.tensor([0.0, 1.6, 0.0]) + 0.05 * torch.randn(N, 3, generator=gen)
    c[:, 9:12] = torch.tensor([0.0, 0.0, 1.6]) + 0.05 * torch.randn(N, 3, generator=gen)
    c[:, 12:18] = 0.05 * torch.randn(N, 6, generator=gen)
    return c.to(DEV).contiguous()


@pytest.mark.parametrize('n', [1, 4])
@pytest.mark.parametrize('S', [32, 48])
def test_bwd_coef_part_is_bit_identical_to_bwd_coef_per_group(n, S):
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    C = 16
    N = T * n
    gen = torch.Generator().manual_seed(S + n)
    vol = ops.cl(torch.randn(1, C, S, S, S, generator=gen).to(DEV))
    gout = ops.cl(torch.randn(N, C, S, S, S, generator=gen).to(DEV))
    cf = _o2c_coefs(N, gen)
    got = torch.empty(N, 18, device=DEV)
    nb = L.lf_resample3d_bwd_coef_part_scratch_bytes(N, n, S, S, S)
    sc = torch.empty(nb // 4 + 1, device=DEV)
    assert L.lf_resample3d_bwd_coef_part(gout.data_ptr(), vol.data_ptr(), 1, cf.data_ptr(), got.data_ptr(), sc.data_ptr(), nb,
                                         N, S, S, S, C, n, _s()) == 0
    for t in range(T):
        r = slice(t * n, (t + 1) * n)
        want = torch.empty(n, 18, device=DEV)
        nb1 = L.lf_resample3d_bwd_coef_scratch_bytes(n, S, S, S)
        sc1 = torch.empty(nb1 // 4 + 1, device=DEV)
        g1 = gout[r].contiguous(memory_format=torch.channels_last_3d)
        assert L.lf_resample3d_bwd_coef(g1.data_ptr(), vol.data_ptr(), 1, cf[r].contiguous().data_ptr(), want.data_ptr(),
                                        sc1.data_ptr(), nb1, n, S, S, S, C, _s()) == 0
        torch.cuda.synchronize()
        assert torch.equal(got[r], want), t
    assert got.abs().sum() > 0
    # part_n = N is the existing entry point itself
    full = torch.empty(N, 18, device=DEV)
    nbf = L.lf_resample3d_bwd_coef_scratch_bytes(N, S, S, S)
    assert L.lf_resample3d_bwd_coef_part_scratch_bytes(N, N, S, S, S) == nbf
    scf = torch.empty(nbf // 4 + 1, device=DEV)
    part = torch.empty(N, 18, device=DEV)
    assert L.lf_resample3d_bwd_coef(gout.data_ptr(), vol.data_ptr(), 1, cf.data_ptr(), full.data_ptr(), scf.data_ptr(), nbf,
                                    N, S, S, S, C, _s()) == 0
    assert L.lf_resample3d_bwd_coef_part(gout.data_ptr(), vol.data_ptr(), 1, cf.data_ptr(), part.data_ptr(), scf.data_ptr(), nbf,
                                         N, S, S, S, C, N, _s()) == 0
    torch.cuda.synchronize()
    assert torch.equal(part, full)


def test_mt_entry_points_reject_bad_arguments():
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    gen = torch.Generator().manual_seed(3)
    n = 2
    N = T * n
    td, tm = _frames(gen)
    logits, coefs = _inputs(N, gen)
    weights = torch.tensor([1.0, 0.3, 0.2, 0.4], device=DEV)
    sums, losses, gsums = (torch.full((N, 8), 7.0, device=DEV) for _ in range(3))
    glogits = torch.full_like(logits, 7.0)
    gcoefs = torch.full((N, 24), 7.0, device=DEV)
    sc, nb = _scratch(L, N)
    p = (logits.data_ptr(), coefs.data_ptr(), td.data_ptr(), tm.data_ptr())

    def fwd(*args, ptrs=p, wts=weights.data_ptr(), out=sums.data_ptr(), nbytes=nb):
        return L.lf_pose_loss_fwd_mt(*ptrs, wts, out, losses.data_ptr(), gsums.data_ptr(), sc.data_ptr(), nbytes, *args, h, w, H, W,
                                     _s())

    def fwdm(*args, ptrs=p, nbytes=nb):
        return L.lf_pose_loss_fwd_masked_mt(*ptrs, weights.data_ptr(), sums.data_ptr(), losses.data_ptr(), sc.data_ptr(), nbytes,
                                            *args, h, w, H, W, _s())

    def bwd(*args, ptrs=p, gs=gsums.data_ptr(), nbytes=nb):
        return L.lf_pose_loss_bwd_mt(*ptrs, gs, glogits.data_ptr(), gcoefs.data_ptr(), sc.data_ptr(), nbytes, *args, h, w, H, W,
                                     _s())

    for f in (fwd, fwdm, bwd):
        assert f(N + 1, T, n) == LF_EINVAL                          # N != T * n
        assert f(N, 0, n) == LF_EINVAL                              # T < 1
        assert f(N, T, 0) == LF_EINVAL                              # n < 1
        assert f(N, T, -n) == LF_EINVAL
        assert f(N, T, n, ptrs=(None,) + p[1:]) == LF_EINVAL          # NULL logits
        assert f(N, T, n, ptrs=p[:2] + (None, p[3])) == LF_EINVAL     # NULL target frame
        assert f(N, T, n, nbytes=nb - 4) == LF_ENOSPC
    assert fwd(N, T, n, wts=None) == LF_EINVAL
    assert fwd(N, T, n, out=None) == LF_EINVAL
    assert bwd(N, T, n, gs=None) == LF_EINVAL
    # partitioned coefficient gradient
    S, C = 16, 16
    vol = ops.cl(torch.randn(1, C, S, S, S, device=DEV))
    gout = ops.cl(torch.randn(N, C, S, S, S, device=DEV))
    cf = _o2c_coefs(N, gen)
    gc = torch.full((N, 18), 7.0, device=DEV)
    need = L.lf_resample3d_bwd_coef_part_scratch_bytes(N, 1, S, S, S)
    assert need >= L.lf_resample3d_bwd_coef_scratch_bytes(N, S, S, S)     # a smaller partition never needs less scratch
    scr = torch.empty(need // 4 + 1, device=DEV)
    args = (gout.data_ptr(), vol.data_ptr(), 1, cf.data_ptr(), gc.data_ptr(), scr.data_ptr())
    assert L.lf_resample3d_bwd_coef_part(*args, need, N, S, S, S, C, 0, _s()) == LF_EINVAL        # part_n < 1
    assert L.lf_resample3d_bwd_coef_part(*args, need, 0, S, S, S, C, 1, _s()) == LF_EINVAL        # N < 1
    assert L.lf_resample3d_bwd_coef_part(None, *args[1:], need, N, S, S, S, C, 1, _s()) == LF_EINVAL
    assert L.lf_resample3d_bwd_coef_part(*args[:4], None, args[5], need, N, S, S, S, C, 1, _s()) == LF_EINVAL
    assert L.lf_resample3d_bwd_coef_part(*args, need - 4, N, S, S, S, C, 1, _s()) == LF_ENOSPC
    assert L.lf_resample3d_bwd_coef_part(*args[:2], 3, *args[3:], need, N, S, S, S, C, 1, _s()) == LF_EINVAL   # vol_n
    torch.cuda.synchronize()
    for t in (sums, losses, gsums, glogits, gcoefs, gc):                # nothing was launched on the rejected calls
        assert (t == 7.0).all()
