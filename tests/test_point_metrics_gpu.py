"""Pose metrics on the device (csrc/points.hip): lf_nn_dist and lf_points_pair_dist against fp64 brute force, and
pose/metrics.py's camera_metrics_batch on the g13 fixture.

The yardstick is fp64 arithmetic on the fp32 inputs: differences, norm and minimum (with transforms: the fp64 transform of the
fp32 points and maps).  Bounds:
  dist, no transforms   5e-7 relative: at most six roundings of 2^-24 reach d^2, the root halves them and adds one, ~2.4e-7 at
                        worst, times a margin of two (the fp32 torch expressions measure 4.7e-8 .. 9.3e-8 on these inputs);
  dist, transforms      max(4 e32, 2e-6 |d|, 2e-7 max|coordinate|), e32 = the largest error of the same computation in fp32
                        torch with direct differences (not cdist);
  idx                   the fp64 argmin for EVERY query without transforms (the smallest relative gap between nearest and second
                        nearest on these inputs is 2.2e-5, asserted below); with transforms a query may differ only where its
                        fp64 gap is below 1e-5, on at most 1 % of the queries, and the fp32 torch restatement meets the same cap;
  mean                  2e-7 relative of the fp64 mean (no transforms: of the kernel's own dist; transforms: the e32 rule).
Every C-ABI call below runs with NaN poison behind its inputs and sentinels behind its outputs and its scratch.

Measured on an MI355X (COVERAGE.md, row f2): dist 5.0e-9 .. 9.2e-8 relative without maps, 9.7e-8 .. 2.4e-7 with them; mean
<= 1.2e-7; idx equal to the fp64 argmin everywhere; lf_points_pair_dist 9.5e-9 .. 3.8e-7; the fp32 Gram form 3.7e-3."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
SENT, ISENT, GUARD = -777.25, -424242, 96
SHAPES = [(1, 1, 1), (1, 7, 5), (2, 64, 63), (3, 257, 1025), (2, 33, 4099), (1, 1500, 1500)]
LF_EINVAL, LF_EALIGN, LF_ENOSPC = -1, -2, -3


def _L():
    from latentfusion_amd import _lib
    return _lib.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def prod_camera(d, device=DEV):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(d['K'].to(device), None, d['z_span'], d['viewport'].to(device), width=d['width'],
                  height=d['height'], log_quaternion=d['log_q'].to(device), translation=d['t'].to(device))


# ----------------------------------------------------------------------------------------------------------------------
# inputs, the fp64 restatement (computed once per case), the guarded C-ABI call, the comparison
# ----------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _inputs(B, M, Q):
    g = torch.Generator().manual_seed(B * 1000003 + M * 1009 + Q)
    x1 = torch.rand(B, M, 3, generator=g) - 0.5
    x2 = torch.rand(B, Q, 3, generator=g) - 0.5
    return x1, x2


def _rigid(B, seed):
    """(B,3,4) rigid maps: rotations of random unit quaternions, translations up to 2."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, 4, generator=g, dtype=torch.float64)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=1).view(B, 3, 3)
    t = (torch.rand(B, 3, 1, generator=g, dtype=torch.float64) * 2 - 1) * 2
    return torch.cat([R, t], dim=2).float()


def _apply(x, T):
    return x if T is None else x @ T[:, :, :3].transpose(1, 2).to(x.dtype) + T[:, :, 3].unsqueeze(1).to(x.dtype)


def _brute(p1, p2):
    """(B,M,Q) distances from coordinate differences, in the dtype of the points."""
    return (p1[:, :, None, :] - p2[:, None, :, :]).norm(dim=-1)


def _first_argmin(D):
    return (D == D.min(dim=2, keepdim=True).values).to(torch.uint8).argmax(dim=2)          # the smallest index on ties


def _reference(x1, x2, T1=None, T2=None):
    p1, p2 = _apply(x1.double(), T1), _apply(x2.double(), T2)
    D = _brute(p1, p2)
    d = D.min(dim=2).values
    idx = _first_argmin(D)
    if D.shape[2] > 1:
        two = D.topk(2, dim=2, largest=False).values
        gap = (two[..., 1] - two[..., 0]) / two[..., 0].clamp_min(1e-300)
    else:
        gap = torch.full_like(d, math.inf)
    D32 = _brute(_apply(x1, T1), _apply(x2, T2))                      # the same computation in fp32 torch
    d32, idx32 = D32.min(dim=2).values, _first_argmin(D32)
    return dict(d=d, idx=idx, gap=gap, mean=d.mean(dim=1), d32=d32, idx32=idx32, mean32=d32.mean(dim=1),
                coord=float(max(p1.abs().max(), p2.abs().max())), tf=T1 is not None or T2 is not None)


def _case(B, M, Q, tf):
    key = (B, M, Q, tf)
    if key not in _CACHE:
        x1, x2 = _inputs(B, M, Q)
        T1, T2 = (_rigid(B, 11 + B * 7 + M), _rigid(B, 23 + B * 5 + Q)) if tf else (None, None)
        _CACHE[key] = (x1, x2, T1, T2, _reference(x1, x2, T1, T2))
    return _CACHE[key]


def _poisoned(t):
    """A device copy of t's values with 64 floats of NaN behind them."""
    flat = t.reshape(-1)
    out = torch.full((flat.numel() + 64,), NAN, device=DEV)
    out[:flat.numel()] = flat.to(DEV)
    return out


def _nn(x1, x2, T1=None, T2=None, want=('dist', 'idx', 'mean'), B=None):
    """lf_nn_dist through the C ABI on CPU inputs; a 2-D cloud is shared by all batches (batch stride 0).  NaN poison behind
    every input, sentinels behind every output and behind the stated scratch size.  -> dict of CPU tensors."""
    L = _L()
    B = B or max([t.shape[0] for t in (x1, x2, T1, T2) if t is not None and t.dim() == 3] + [1])
    M, Q = x1.shape[-2], x2.shape[-2]
    s1 = M * 3 if x1.dim() == 3 and x1.shape[0] == B and B > 1 else 0
    s2 = Q * 3 if x2.dim() == 3 and x2.shape[0] == B and B > 1 else 0
    bufs = [_poisoned(t) if t is not None else None for t in (x1, T1, x2, T2)]
    dist = torch.full((B * M + GUARD,), SENT, device=DEV) if 'dist' in want else None
    idx = torch.full((B * M + GUARD,), ISENT, device=DEV, dtype=torch.int32) if 'idx' in want else None
    mean = torch.full((B + GUARD,), SENT, device=DEV) if 'mean' in want else None
    nbytes = L.lf_nn_dist_scratch_bytes(B, M, Q)
    assert nbytes == B * ((M + 63) // 64) * 8
    scratch = torch.full((nbytes // 8 + GUARD,), SENT, device=DEV, dtype=torch.float64)
    p = [b.data_ptr() if b is not None else None for b in bufs]
    rc = L.lf_nn_dist(p[0], s1, p[1], p[2], s2, p[3], dist.data_ptr() if dist is not None else None,
                      idx.data_ptr() if idx is not None else None, mean.data_ptr() if mean is not None else None,
                      scratch.data_ptr(), nbytes, B, M, Q, _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {}
    if dist is not None:
        assert (dist[B * M:] == SENT).all()
        out['dist'] = dist[:B * M].view(B, M).cpu()
    if idx is not None:
        assert (idx[B * M:] == ISENT).all()
        out['idx'] = idx[:B * M].view(B, M).cpu()
    if mean is not None:
        assert (mean[B:] == SENT).all()
        out['mean'] = mean[:B].cpu()
    assert (scratch[nbytes // 8:] == SENT).all()
    return out


def _compare(out, ref, show=''):
    """The assertions of this file on a result {dist, idx, mean} (B,M) against _reference()."""
    d, idx, mean = out['dist'].double(), out['idx'].long(), out['mean'].double()
    err = (d - ref['d']).abs()
    e32 = float((ref['d32'].double() - ref['d']).abs().max())
    differs = idx != ref['idx']
    if ref['tf']:
        bound = torch.maximum(torch.full_like(err, max(4 * e32, 2e-7 * ref['coord'])), 2e-6 * ref['d'])
        mean_bound = torch.maximum(torch.full_like(ref['mean'], max(4 * float((ref['mean32'].double() - ref['mean']).abs().max()),
                                                                    2e-7 * ref['coord'])), 2e-6 * ref['mean'])
        mean_ref = ref['mean']
    else:
        bound = 5e-7 * ref['d']
        mean_ref = d.mean(dim=1)                                    # the fp64 mean of the kernel's own distances
        mean_bound = 2e-7 * mean_ref
    print(f'{show} max rel err {float((err / ref["d"].clamp_min(1e-30)).max()):.3g} (fp32 torch {e32:.3g} abs), idx differs on '
          f'{int(differs.sum())}, mean err {float(((mean - mean_ref).abs() / mean_ref.clamp_min(1e-30)).max()):.3g} rel')
    assert (err <= bound).all(), float((err - bound).max())
    if ref['tf']:
        for got in (differs, ref['idx32'] != ref['idx']):            # the kernel, and the fp32 torch restatement
            assert (ref['gap'][got] < 1e-5).all() and float(got.double().mean()) <= 0.01
    else:
        assert not differs.any()
    assert ((mean - mean_ref).abs() <= mean_bound).all()


# ----------------------------------------------------------------------------------------------------------------------
# 1. distances and indices against fp64 brute force
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tf', [False, True], ids=['plain', 'rigid'])
@pytest.mark.parametrize('B,M,Q', SHAPES)
def test_nn_dist_against_fp64(B, M, Q, tf):
    x1, x2, T1, T2, ref = _case(B, M, Q, tf)
    if not tf and Q > 1:
        assert float(ref['gap'].min()) > 2e-5                        # no query of these inputs is near a tie: none is excluded
    out = _nn(x1, x2, T1, T2)
    _compare(out, ref, f'{(B, M, Q)}')
    assert torch.equal(_nn(x1, x2, T1, T2, want=('mean',))['mean'], out['mean'])        # the form without the index: same bits


def test_wrappers_agree_with_the_abi_call():
    from latentfusion_amd import ops
    from latentfusion_amd.pose import metrics
    x1, x2, T1, T2, _ = _case(3, 257, 1025, True)
    want = _nn(x1, x2, T1, T2)
    got = ops.nn_dist(x1.to(DEV), x2.to(DEV), T1.to(DEV), T2.to(DEV), want=('dist', 'idx', 'mean'))
    for k in want:
        assert torch.equal(got[k].cpu(), want[k]), k
    plain = _nn(x1, x2)
    d, i = metrics.best_distance_device(x1.to(DEV), x2.to(DEV), return_index=True)
    assert torch.equal(d.cpu(), plain['dist']) and torch.equal(i.cpu(), plain['idx']) and i.dtype == torch.int32
    d0 = metrics.best_distance_device(x1[0].to(DEV), x2[0].to(DEV))
    assert d0.shape == (257,) and torch.equal(d0.cpu(), plain['dist'][0])


# ----------------------------------------------------------------------------------------------------------------------
# 2. the comparison rejects wrong readings
# ----------------------------------------------------------------------------------------------------------------------
def _as_result(D):
    d = D.min(dim=2).values
    return dict(dist=d.float(), idx=_first_argmin(D).int(), mean=d.mean(dim=1).float())


def test_the_comparison_rejects_wrong_readings():
    x1, x2, _, _, ref = _case(1, 1500, 1500, False)
    D = _brute(x1.double(), x2.double())
    _compare(_as_result(D), ref, 'fp64 restatement')                  # the right reading passes
    with pytest.raises(AssertionError):
        _compare(_as_result(D.transpose(1, 2)), ref, 'roles swapped')  # nearest x1 point per x2 point
    with pytest.raises(AssertionError):
        _compare(_as_result(D * D), ref, 'squared')
    second = D.topk(2, dim=2, largest=False)
    with pytest.raises(AssertionError):
        _compare(dict(dist=second.values[..., 1].float(), idx=second.indices[..., 1].int(),
                      mean=second.values[..., 1].mean(dim=1).float()), ref, 'second nearest')
    x1t, x2t, T1, T2, reft = _case(3, 257, 1025, True)
    _compare(_as_result(_brute(_apply(x1t.double(), T1), _apply(x2t.double(), T2))), reft, 'fp64 restatement, rigid')
    with pytest.raises(AssertionError):
        _compare(_as_result(_brute(_apply(x1t.double(), T2), _apply(x2t.double(), T1))), reft, 'T1 / T2 swapped')


def test_the_comparison_rejects_the_gram_form():
    """torch.cdist's matrix-multiply form |a|^2 + |b|^2 - 2ab in fp32 on a model-sized cloud 1.5 away from the origin: off by
    1e-4 and more of a nearest distance.  The kernel passes the same comparison on the same points."""
    x1, x2 = _inputs(1, 1500, 1500)
    shift = torch.tensor([0.0, 0.0, 1.5])
    x1, x2 = x1 + shift, x2 + shift
    ref = _reference(x1, x2)
    gram = torch.cdist(x1, x2, compute_mode='use_mm_for_euclid_dist')
    with pytest.raises(AssertionError):
        _compare(_as_result(gram), ref, 'Gram form')
    _compare(_nn(x1, x2), ref, 'kernel, translated cloud')


# ----------------------------------------------------------------------------------------------------------------------
# 3. every candidate position; 4. ties
# ----------------------------------------------------------------------------------------------------------------------
def test_every_candidate_position_is_found():
    g = torch.Generator().manual_seed(4099)
    n = 4099                                                          # four LDS tiles and three candidates
    x2 = torch.rand(n, 3, generator=g) - 0.5
    assert torch.unique(x2, dim=0).shape[0] == n
    perm = torch.randperm(n, generator=g)
    out = _nn(x2[perm], x2)
    assert torch.equal(out['idx'][0], perm.int()) and (out['dist'] == 0).all() and float(out['mean']) == 0.0


def _lattice():
    g = torch.Generator().manual_seed(5)
    grid = torch.stack(torch.meshgrid(*[torch.arange(3.0)] * 3, indexing='ij'), dim=-1).view(-1, 3) / 4      # dyadic: exact
    x2 = torch.cat([grid[torch.randperm(27, generator=g)], grid[torch.randperm(27, generator=g)]])          # every point twice
    centres = (torch.stack(torch.meshgrid(*[torch.arange(2.0)] * 3, indexing='ij'), dim=-1).view(-1, 3) + 0.5) / 4
    x1 = torch.cat([grid, centres])                                   # on a candidate (2 ties) / equidistant from 8 (16 ties)
    return x1, x2


def test_ties_return_the_smallest_index():
    x1, x2 = _lattice()
    out = _nn(x1, x2)
    D = _brute(x1.double()[None], x2.double()[None])
    assert ((D == D.min(dim=2, keepdim=True).values).sum(dim=2)[0] == torch.tensor([2] * 27 + [16] * 8)).all()
    assert torch.equal(out['idx'], _first_argmin(D).int())
    exact = torch.cat([torch.zeros(27), torch.full((8,), 3.0 / 64).sqrt()])                 # d^2 = 3/64 exactly, one root
    assert torch.equal(out['dist'][0], exact)
    ref = _reference(x1[None], x2[None])
    _compare(out, ref, 'lattice')
    last = (D == D.min(dim=2, keepdim=True).values).to(torch.uint8).flip(2).argmax(dim=2)
    with pytest.raises(AssertionError):                               # the wrong reading: the largest index on ties
        _compare(dict(out, idx=(D.shape[2] - 1 - last).int()), ref, 'largest index')


# ----------------------------------------------------------------------------------------------------------------------
# 5. independence, bit for bit
# ----------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


def test_results_do_not_depend_on_the_batch_the_tile_or_the_run():
    x1, x2, T1, T2, _ = _case(3, 257, 1025, True)
    full = _nn(x1, x2, T1, T2)
    assert _same(full, _nn(x1, x2, T1, T2))                           # two runs
    for b in range(3):                                                # a batch row alone
        alone = _nn(x1[b:b + 1], x2[b:b + 1], T1[b:b + 1], T2[b:b + 1])
        assert all(torch.equal(alone[k][0], full[k][b]) for k in full), b
    for i in (0, 63, 64, 255, 256):                                   # one query alone (M = 1)
        one = _nn(x1[1:2, i:i + 1], x2[1:2], T1[1:2], T2[1:2])
        assert torch.equal(one['dist'][0, 0], full['dist'][1, i]) and torch.equal(one['idx'][0, 0], full['idx'][1, i])
    for want in (('dist',), ('idx',), ('mean',), ('dist', 'mean')):   # any subset of the outputs
        part = _nn(x1, x2, T1, T2, want=want)
        assert set(part) == set(want) and all(torch.equal(part[k], full[k]) for k in want), want


def test_shared_clouds_equal_materialised_copies():
    x1, x2, T1, T2, _ = _case(3, 257, 1025, True)
    shared = _nn(x1[0], x2[0], T1, T2)                               # batch stride 0: the metrics case
    copies = _nn(x1[0:1].repeat(3, 1, 1), x2[0:1].repeat(3, 1, 1), T1, T2)
    assert _same(shared, copies) and shared['dist'].shape == (3, 257)
    assert not torch.equal(shared['dist'][0], shared['dist'][1])


def test_four_queries_per_thread_give_the_same_bits():
    """A grid that gives every compute unit a workgroup at four queries per thread takes that form of the kernel: same bits as
    the one-query form on the same queries, and the mean of all of them."""
    g = torch.Generator().manual_seed(77)
    M, Q = 1024 * 256 + 5, 19
    x1, x2 = torch.rand(M, 3, generator=g) - 0.5, torch.rand(Q, 3, generator=g) - 0.5
    wide = _nn(x1, x2)
    for lo, hi in ((0, 257), (1024 * 128 - 3, 1024 * 128 + 300), (M - 300, M)):
        small = _nn(x1[lo:hi], x2, want=('dist', 'idx'))
        assert torch.equal(small['dist'][0], wide['dist'][0, lo:hi]) and torch.equal(small['idx'][0], wide['idx'][0, lo:hi])
    for lo in range(0, M, 1 << 16):
        ref = (x1[lo:lo + (1 << 16)].double()[:, None] - x2.double()[None]).norm(dim=-1).min(dim=1)
        assert torch.equal(wide['idx'][0, lo:lo + (1 << 16)].long(), ref.indices)
        assert ((wide['dist'][0, lo:lo + (1 << 16)].double() - ref.values).abs() <= 5e-7 * ref.values).all()
    mean_ref = wide['dist'][0].double().mean()
    assert abs(float(wide['mean']) - float(mean_ref)) <= 2e-7 * float(mean_ref)
    assert torch.equal(_nn(x1, x2, want=('mean',))['mean'], wide['mean'])


# ----------------------------------------------------------------------------------------------------------------------
# 6. non-finite input
# ----------------------------------------------------------------------------------------------------------------------
def test_nan_stays_in_its_query_or_its_batch():
    x1, x2, T1, T2, _ = _case(3, 257, 1025, True)
    clean = _nn(x1, x2, T1, T2)
    bad = x1.clone()
    bad[1, 70, 2] = NAN
    bad[2, 256, 0] = NAN
    out = _nn(bad, x2, T1, T2)
    keep = torch.ones(3, 257, dtype=torch.bool)
    keep[1, 70] = keep[2, 256] = False
    assert torch.equal(out['dist'][keep], clean['dist'][keep]) and torch.equal(out['idx'][keep], clean['idx'][keep])
    assert torch.isnan(out['dist'][~keep]).all() and (out['idx'][~keep] == -1).all()
    assert torch.equal(out['mean'][0], clean['mean'][0]) and torch.isnan(out['mean'][1:]).all()
    for j in (0, 1023, 1024):                                         # a NaN candidate: its whole batch, as torch.min would
        bad = x2.clone()
        bad[1, j, 1] = NAN
        out = _nn(x1, bad, T1, T2)
        assert torch.isnan(torch.cdist(x1[1], bad[1]).min(dim=1).values).all()
        assert torch.isnan(out['dist'][1]).all() and (out['idx'][1] == -1).all() and torch.isnan(out['mean'][1])
        for b in (0, 2):
            assert all(torch.equal(out[k][b], clean[k][b]) for k in clean)
    badT = T2.clone()
    badT[0, 1, 3] = NAN                                               # a NaN in a map is a NaN in every point it maps
    out = _nn(x1, x2, T1, badT)
    assert torch.isnan(out['dist'][0]).all() and (out['idx'][0] == -1).all()
    assert all(torch.equal(out[k][1:], clean[k][1:]) for k in clean)


# ----------------------------------------------------------------------------------------------------------------------
# 8. ABI errors: a negative code, nothing launched, nothing written
# ----------------------------------------------------------------------------------------------------------------------
def test_nn_dist_abi_errors_leave_the_outputs_alone():
    L = _L()
    B, M, Q = 2, 70, 33
    x1, x2 = torch.rand(B, M, 3, device=DEV), torch.rand(B, Q, 3, device=DEV)
    T = torch.eye(3, 4, device=DEV).repeat(B, 1, 1).contiguous()
    dist = torch.full((B * M,), SENT, device=DEV)
    idx = torch.full((B * M,), ISENT, device=DEV, dtype=torch.int32)
    mean = torch.full((B,), SENT, device=DEV)
    nbytes = L.lf_nn_dist_scratch_bytes(B, M, Q)
    scratch = torch.full((nbytes // 8,), SENT, device=DEV, dtype=torch.float64)
    good = dict(x1=x1.data_ptr(), s1=M * 3, T1=T.data_ptr(), x2=x2.data_ptr(), s2=Q * 3, T2=T.data_ptr(), dist=dist.data_ptr(),
                idx=idx.data_ptr(), mean=mean.data_ptr(), scratch=scratch.data_ptr(), nbytes=nbytes, B=B, M=M, Q=Q)

    def call(**over):
        a = dict(good, **over)
        return L.lf_nn_dist(a['x1'], a['s1'], a['T1'], a['x2'], a['s2'], a['T2'], a['dist'], a['idx'], a['mean'], a['scratch'],
                            a['nbytes'], a['B'], a['M'], a['Q'], _s())
    cases = [(dict(x1=None), LF_EINVAL), (dict(x2=None), LF_EINVAL), (dict(dist=None, idx=None, mean=None), LF_EINVAL),
             (dict(B=0), LF_EINVAL), (dict(M=0), LF_EINVAL), (dict(Q=0), LF_EINVAL), (dict(B=-1), LF_EINVAL),
             (dict(M=-5), LF_EINVAL), (dict(Q=-1), LF_EINVAL), (dict(s1=-3), LF_EINVAL), (dict(s2=-3), LF_EINVAL),
             (dict(B=1 << 20, M=1 << 12), LF_EINVAL),
             (dict(nbytes=nbytes - 4), LF_ENOSPC), (dict(nbytes=0), LF_ENOSPC), (dict(scratch=None), LF_ENOSPC)]
    cases += [({k: good[k] + 2}, LF_EALIGN) for k in ('x1', 'T1', 'x2', 'T2', 'dist', 'idx', 'mean')]
    cases += [(dict(scratch=good['scratch'] + 4), LF_EALIGN)]
    for over, want in cases:
        assert call(**over) == want, over
    torch.cuda.synchronize()
    assert (dist == SENT).all() and (idx == ISENT).all() and (mean == SENT).all() and (scratch == SENT).all()
    assert L.lf_nn_dist_scratch_bytes(0, M, Q) == 0 and L.lf_nn_dist_scratch_bytes(B, 0, Q) == 0
    assert call(mean=None, scratch=None, nbytes=0) == 0               # scratch serves the mean alone
    assert call() == 0
    torch.cuda.synchronize()
    assert not (dist == SENT).any() and not (idx == ISENT).any() and not (mean == SENT).any()


def test_points_pair_dist_abi_errors_leave_the_outputs_alone():
    L = _L()
    R, P = 3, 130
    pts = torch.rand(P, 3, device=DEV)
    A = torch.eye(4, device=DEV).repeat(R, 1, 1).contiguous()
    mean = torch.full((R,), SENT, device=DEV)
    nbytes = L.lf_points_pair_dist_scratch_bytes(R, P)
    assert nbytes == R * 3 * 8
    scratch = torch.full((nbytes // 8,), SENT, device=DEV, dtype=torch.float64)
    good = dict(pts=pts.data_ptr(), sr=0, A=A.data_ptr(), Bm=A.data_ptr(), rows=4, mean=mean.data_ptr(),
                scratch=scratch.data_ptr(), nbytes=nbytes, R=R, P=P)

    def call(**over):
        a = dict(good, **over)
        return L.lf_points_pair_dist(a['pts'], a['sr'], a['A'], a['Bm'], a['rows'], a['mean'], a['scratch'], a['nbytes'], a['R'],
                                     a['P'], _s())
    cases = [(dict(pts=None), LF_EINVAL), (dict(A=None), LF_EINVAL), (dict(Bm=None), LF_EINVAL), (dict(mean=None), LF_EINVAL),
             (dict(R=0), LF_EINVAL), (dict(P=0), LF_EINVAL), (dict(R=-2), LF_EINVAL), (dict(P=-1), LF_EINVAL),
             (dict(rows=2), LF_EINVAL), (dict(rows=5), LF_EINVAL), (dict(rows=0), LF_EINVAL), (dict(sr=-1), LF_EINVAL),
             (dict(R=65536), LF_EINVAL),
             (dict(nbytes=nbytes - 4), LF_ENOSPC), (dict(nbytes=0), LF_ENOSPC), (dict(scratch=None), LF_ENOSPC)]
    cases += [({k: good[k] + 2}, LF_EALIGN) for k in ('pts', 'A', 'Bm', 'mean')] + [(dict(scratch=good['scratch'] + 4), LF_EALIGN)]
    for over, want in cases:
        assert call(**over) == want, over
    torch.cuda.synchronize()
    assert (mean == SENT).all() and (scratch == SENT).all()
    assert L.lf_points_pair_dist_scratch_bytes(0, P) == 0 and L.lf_points_pair_dist_scratch_bytes(R, 0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert (mean == 0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 9. lf_points_pair_dist against fp64
# ----------------------------------------------------------------------------------------------------------------------
def _pair_inputs(P, R, rows):
    """Model-sized points and g13-like cameras: rigid poses 1.2 in front of a 500-pixel pinhole.  rows = 4: the 4x4 pose times a
    homogeneous scale per row (so that the division matters); rows = 3: the 3x4 projection."""
    g = torch.Generator().manual_seed(P * 31 + R * 7 + rows)
    pts = (torch.rand(P, 3, generator=g) - 0.5) * 0.2
    K = torch.tensor([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])
    out = []
    for seed in (1, 2):
        E = _rigid(R, 100 * seed + P + R)
        E[:, :, 3] = E[:, :, 3] * 0.15 + torch.tensor([0.0, 0.0, 1.2])
        if rows == 3:
            out.append((K @ E).contiguous())
        else:
            E4 = torch.cat([E, torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(R, 1, 4)], dim=1)
            out.append((E4 * (0.5 + torch.rand(R, 1, 1, generator=g))).contiguous())
    return pts, out[0], out[1]


def _pair_formula(pts, A, Bm, divide=True, rows=None):
    rows = rows or A.shape[1]
    h = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
    pa, pb = h @ A[:, :rows].transpose(1, 2), h @ Bm[:, :rows].transpose(1, 2)               # (R,P,rows)
    if divide:
        pa, pb = pa[..., :-1] / pa[..., -1:], pb[..., :-1] / pb[..., -1:]
    return (pa - pb).norm(dim=-1).mean(dim=1)


def _pair(pts, A, Bm, R=None):
    L = _L()
    R, rows, P = R or A.shape[0], A.shape[1], pts.shape[-2]
    bufs = [_poisoned(t) for t in (pts, A, Bm)]
    mean = torch.full((R + GUARD,), SENT, device=DEV)
    nbytes = L.lf_points_pair_dist_scratch_bytes(R, P)
    scratch = torch.full((nbytes // 8 + GUARD,), SENT, device=DEV, dtype=torch.float64)
    rc = L.lf_points_pair_dist(bufs[0].data_ptr(), P * 3 if pts.dim() == 3 else 0, bufs[1].data_ptr(), bufs[2].data_ptr(), rows,
                               mean.data_ptr(), scratch.data_ptr(), nbytes, R, P, _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (mean[R:] == SENT).all() and (scratch[nbytes // 8:] == SENT).all()
    return mean[:R].cpu()


@pytest.mark.parametrize('rows', [3, 4])
@pytest.mark.parametrize('R', [1, 3, 7])
@pytest.mark.parametrize('P', [1, 63, 1500])
def test_points_pair_dist_against_fp64(P, R, rows):
    pts, A, Bm = _pair_inputs(P, R, rows)
    ref = _pair_formula(pts.double(), A.double(), Bm.double())
    e32 = (_pair_formula(pts, A, Bm).double() - ref).abs()

    def check(got):
        assert ((got.double() - ref).abs() <= torch.maximum(4 * e32, 2e-6 * ref)).all()
    got = _pair(pts, A, Bm)
    print(f'P {P} R {R} rows {rows}: max rel err {float(((got.double() - ref).abs() / ref).max()):.3g}, '
          f'fp32 torch {float((e32 / ref).max()):.3g}')
    check(got)
    with pytest.raises(AssertionError):
        check(_pair_formula(pts.double(), A.double(), Bm.double(), divide=False).float())        # no perspective division
    with pytest.raises(AssertionError):                                                           # rows misread
        check((_pair_formula(pts.double(), A.double(), Bm.double(), rows=3) if rows == 4
               else _pair_formula(pts.double(), A.double(), Bm.double(), divide=False) * 1.0).float())
    assert torch.equal(got, _pair(pts, A, Bm))                                                    # two runs
    for r in range(R):                                                                           # a row alone
        assert torch.equal(_pair(pts, A[r:r + 1], Bm[r:r + 1])[0], got[r])
    assert torch.equal(_pair(pts[None].repeat(R, 1, 1), A, Bm), got)                              # a cloud per row
    from latentfusion_amd import ops
    assert torch.equal(ops.points_pair_dist(pts.to(DEV), A.to(DEV), Bm.to(DEV)).cpu(), got)


# ----------------------------------------------------------------------------------------------------------------------
# 10. camera_metrics_batch on the g13 fixture
# ----------------------------------------------------------------------------------------------------------------------
KEYS = ('rotation_dist', 'translation_dist', 'add', 'add_s', 'add_sym', 'proj2d')


def _launches(fn):
    """{entry point: launches} of liblf_hip.so while fn() runs (counted by _lib.check, as tests/test_ibr_fused_gpu.py does)."""
    from latentfusion_amd import _lib
    _lib.BYTE_LOG = {}
    try:
        out = fn()
        return out, {k: v[0] for k, v in _lib.BYTE_LOG.items()}
    finally:
        _lib.BYTE_LOG = None


def _metrics_formula(gt, ev, points, scale, dt):
    """camera_metrics' point metrics restated with direct differences in dtype dt, from the cameras' fp32 matrices."""
    from latentfusion_amd.pose import metrics
    B = len(ev)
    e_gt, e_ev = gt.obj_to_cam.expand(B, 4, 4), ev.obj_to_cam                 # the fp32 matrices as the device forms them
    i_gt, i_ev = gt.obj_to_image.expand(B, 3, 4).cpu().to(dt), ev.obj_to_image.cpu().to(dt)
    e_sym = (e_gt @ metrics._rot_z180(e_gt)).cpu().to(dt)
    e_gt, e_ev, pts = e_gt.cpu().to(dt), e_ev.cpu().to(dt), points.to(dt)
    add = _pair_formula(pts, e_gt, e_ev)
    p_gt, p_ev = _apply(pts.expand(B, -1, 3), e_gt[:, :3]), _apply(pts.expand(B, -1, 3), e_ev[:, :3])
    return {'add': add * scale, 'add_s': _brute(p_gt, p_ev).min(dim=2).values.mean(dim=1) * scale,
            'add_sym': torch.minimum(add, _pair_formula(pts, e_sym, e_ev)) * scale, 'proj2d': _pair_formula(pts, i_gt, i_ev)}


def test_camera_metrics_batch_on_the_fixture(golden):
    from latentfusion_amd.pose import metrics
    g = golden('g13_metrics')
    gt, ev, gt_cpu, ev_cpu = prod_camera(g['gt']), prod_camera(g['ev']), prod_camera(g['gt'], 'cpu'), prod_camera(g['ev'], 'cpu')
    points, scale = g['points'], g['scale']
    before = metrics.camera_metrics(gt_cpu, ev_cpu, points, scale)
    for B in (1, 3):
        got, n = _launches(lambda: metrics.camera_metrics_batch(gt[:B], ev[:B], points.to(DEV), scale))
        assert n.get('lf_nn_dist') == 1 and 1 <= n.get('lf_points_pair_dist') <= 2 and set(n) == {'lf_nn_dist', 'lf_points_pair_dist'}
        assert tuple(got) == KEYS
        ref64 = _metrics_formula(gt[:B], ev[:B], points, scale, torch.float64)
        ref32 = _metrics_formula(gt[:B], ev[:B], points, scale, torch.float32)
        for k in KEYS:
            assert got[k].shape == (B,) and got[k].dtype == torch.float32 and got[k].is_cuda
            for i in range(B):                                        # the fixture, at the bound of test_pose_metrics_golden
                v = g['metrics'][i][k]
                assert abs(float(got[k][i]) - v) <= 1e-5 * max(1.0, abs(v)), (k, i, float(got[k][i]), v)
        for k in KEYS[2:]:
            err, e32 = (got[k].cpu().double() - ref64[k]).abs(), (ref32[k].double() - ref64[k]).abs()
            print(f'B {B} {k}: rel err {float((err / ref64[k]).max()):.3g}, fp32 torch {float((e32 / ref64[k]).max()):.3g}')
            assert (err <= torch.maximum(4 * e32, 2e-6 * ref64[k])).all(), k
        assert (got['add_s'] <= got['add']).all() and (got['add_sym'] <= got['add']).all()
    full = got
    # one ground truth against all hypotheses
    one = metrics.camera_metrics_batch(gt[0:1], ev, points.to(DEV), scale)
    want = [metrics.camera_metrics(gt_cpu[0], ev_cpu[i], points, scale) for i in range(3)]
    for k in KEYS:
        for i in range(3):
            v = float(want[i][k])
            assert abs(float(one[k][i]) - v) <= 1e-5 * max(1.0, abs(v)), (k, i)
        assert torch.equal(one[k][0], full[k][0])
    # the switches hold for every pair, host points are accepted, CPU cameras with device= too
    for off in KEYS[2:]:
        part, n = _launches(lambda: metrics.camera_metrics_batch(gt, ev, points, scale, **{'use_' + off: False}))
        assert set(part) == set(KEYS) - {off} and all(torch.equal(part[k], full[k]) for k in part)
        assert n.get('lf_nn_dist', 0) == (off != 'add_s') and n.get('lf_points_pair_dist', 0) == 2 - (off == 'proj2d')
    moved = metrics.camera_metrics_batch(gt_cpu, ev_cpu, points, scale, device=DEV)
    assert all(moved[k].is_cuda and torch.allclose(moved[k], full[k], rtol=1e-5, atol=1e-7) for k in KEYS)
    assert tuple(metrics.camera_metrics_batch(gt, ev, None, scale)) == KEYS[:2]
    # identical cameras score exactly zero
    same = metrics.camera_metrics_batch(gt, gt, points.to(DEV), scale)
    for k in ('add', 'add_s', 'add_sym', 'proj2d', 'translation_dist'):
        assert (same[k] == 0).all(), k
    # no ATen distance matrix on the way
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        metrics.camera_metrics_batch(gt, ev, points.to(DEV), scale)
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    assert names and not [n for n in names if 'cdist' in n.lower() or 'euclidean_dist' in n.lower()]
    # the existing API still returns what it returned
    after = metrics.camera_metrics(gt_cpu, ev_cpu, points, scale)
    for m0, m1 in zip(before, after):
        assert set(m0) == set(m1) and all(float(m0[k]) == float(m1[k]) for k in m0)
