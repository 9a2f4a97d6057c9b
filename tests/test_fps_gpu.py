"""lf_farthest_points (csrc/fps.hip, ops.farthest_points, three.utils.farthest_points(kernel='fused'), pointcloud.eval_points)
against the fp32 restatement of its contract on the CPU (tests/eval_cloud_cases.py fps_restate: elementwise torch operations in
the contract's order and the correctly rounded root -- torch.sqrt in fp64 rounded once: torch.sqrt on a float32 CPU tensor is
one ulp off for about 0.6 % of the values, see rounded_sqrt there) -- torch.equal on centers, owner and nearest, in BOTH forms
at every case -- and, at the four clouds that tests/test_eval_cloud_cases.py proves conditioned, against the composed path over
F.pairwise_distance.

Every call of the entry point goes through `_run`: NaN-poisoned outputs and scratch with sentinels behind each of them."""
import pytest
import torch
import torch.nn.functional as F

import eval_cloud_cases as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT, ISENT, GUARD = -777.25, -424242, 64
LF_EINVAL, LF_EALIGN, LF_ENOSPC = -1, -2, -3
RESIDENT, STREAMED = 1, 2
RESIDENT_MAX = (160 * 1024 - 256) // 16


def _L():
    from latentfusion_amd import _lib
    return _lib.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dtype):
    buf = torch.empty(n + GUARD, device=DEV, dtype=dtype)
    buf.view(torch.uint8)[:n * buf.element_size()] = 0xff
    buf[n:] = SENT if dtype.is_floating_point else ISENT
    return buf, buf[:n]


def _intact(buf, n):
    return bool((buf[n:] == (SENT if buf.dtype.is_floating_point else ISENT)).all())


def _untouched(view):
    return bool((view.contiguous().view(torch.uint8) == 0xff).all())


def _call(x, k, form, B=None, want=(True, True, True), over=None):
    """One call on a CPU cloud x (N,3) shared by B batches (stride 0) or (B,N,3).  -> (rc, guarded views, sentinels intact)."""
    L = _L()
    shared = x.dim() == 2
    B = (1 if B is None else B) if shared else x.shape[0]
    N = x.shape[-2]
    xd = x.to(DEV).contiguous()
    cb, centers = _guarded(B * max(k, 1), torch.int32)
    ob, owner = _guarded(B * N, torch.int32)
    nb, nearest = _guarded(B * N, torch.float32)
    nbytes = L.lf_farthest_points_scratch_bytes(B, N, k, form)
    xb, scratch = _guarded(nbytes // 4, torch.float32)
    args = [xd.data_ptr(), 0 if shared else N * 3, centers.data_ptr() if want[0] else None, owner.data_ptr() if want[1] else None,
            nearest.data_ptr() if want[2] else None, scratch.data_ptr(), nbytes, B, N, k, form, _s()]
    if over is not None:
        over(args)
    rc = L.lf_farthest_points(*args)
    torch.cuda.synchronize()
    ok = _intact(cb, B * max(k, 1)) and _intact(ob, B * N) and _intact(nb, B * N) and _intact(xb, nbytes // 4)
    return rc, dict(centers=centers.view(B, max(k, 1)), owner=owner.view(B, N), nearest=nearest.view(B, N)), ok


def _run(x, k, form, B=None, want=(True, True, True)):
    """-> (centers (B,k) int32, owner (B,N) int32, nearest (B,N) float32) on the CPU; None where not asked for."""
    rc, out, ok = _call(x, k, form, B=B, want=want)
    assert rc == 0, rc
    assert ok
    for name, asked in zip(('centers', 'owner', 'nearest'), want):
        assert asked or _untouched(out[name]), name
    return tuple(out[name].cpu() if asked else None for name, asked in zip(('centers', 'owner', 'nearest'), want))


def _both_forms(x, k, B=None):
    a = _run(x, k, RESIDENT, B=B)
    b = _run(x, k, STREAMED, B=B)
    for u, v, name in zip(a, b, ('centers', 'owner', 'nearest')):
        assert torch.equal(u, v), name
    return a


def _equals_restatement(got, expected, b=0):
    centers, owner, nearest = expected
    assert torch.equal(got[0][b], centers), 'centers'
    assert torch.equal(got[1][b], owner), 'owner'
    assert torch.equal(got[2][b], nearest), 'nearest'


@pytest.mark.parametrize('i', range(len(K.FPS_SIZES)))
def test_both_forms_equal_the_restatement_bit_for_bit(i):
    x, k = K.fps_clouds()[i]
    if x.shape[0] <= RESIDENT_MAX:
        got = _both_forms(x, k)
    else:                                                            # 20000 points: the resident form does not take them
        got = _run(x, k, STREAMED)
        rc, out, ok = _call(x, k, RESIDENT)
        assert rc == LF_EINVAL and ok and all(_untouched(v) for v in out.values())
    _equals_restatement(got, K.fps_expected(i))
    auto = _run(x, k, 0)
    for u, v in zip(auto, got):
        assert torch.equal(u, v)


@pytest.mark.parametrize('i', range(K.FPS_CONDITIONED))
def test_conditioned_clouds_against_the_composed_path(i):
    x, k = K.fps_clouds()[i]
    centers, owner, nearest = _both_forms(x, k)
    c_centers, c_owner, c_nearest = K.fps_composed(x, k)
    assert torch.equal(centers[0].long(), c_centers) and torch.equal(owner[0].long(), c_owner)
    err = float((nearest[0] - c_nearest).abs().max())
    print(f'fps cloud {tuple(x.shape)} K={k}: max |nearest - composed| {err:.3e}')
    assert err <= 4e-6


@pytest.mark.parametrize('j', range(2))
def test_ties_pick_the_smallest_index_and_the_last_centre_owns(j):
    x, k = K.fps_tie_clouds()[j]
    got = _both_forms(x, k)
    expected = K.fps_restate(x, k)
    _equals_restatement(got, expected)
    assert not torch.equal(got[0][0], K.fps_restate(x, k, tie='largest')[0])
    assert not torch.equal(got[1][0], K.fps_restate(x, k, owner_rule='first')[1])


def test_k_1_and_k_n():
    x = K.fps_clouds()[2][0]                                         # 257 points
    for k in (1, 257):
        _equals_restatement(_both_forms(x, k), K.fps_restate(x, k))
    one = _both_forms(x, 1)
    assert one[0].tolist() == [[0]] and not bool(one[1].any())
    every = _both_forms(x, 257)
    assert sorted(every[0][0].tolist()) == list(range(257)) and not bool(every[2].any())
    single = torch.tensor([[0.5, -1.0, 2.0]])                        # one point
    got = _both_forms(single, 1)
    assert got[0].tolist() == [[0]] and got[1].tolist() == [[0]] and got[2].tolist() == [[0.0]]


def test_batches_shared_cloud_and_slices():
    x, k = K.fps_clouds()[3]                                         # 1025 points: two streamed slices, the second of one point
    expected = K.fps_expected(3)
    shared = _both_forms(x, k, B=3)                                  # stride 0
    for b in range(3):
        _equals_restatement(shared, expected, b)
    g = torch.Generator().manual_seed(21)
    clouds = torch.stack((x, torch.randn(1025, 3, generator=g).clamp(-4, 4), x.flip(0)))
    batch = _both_forms(clouds, 77)
    for b in range(3):
        alone = _run(clouds[b], 77, 0)
        for u, v in zip(batch, alone):
            assert torch.equal(u[b], v[0])
        _equals_restatement(batch, K.fps_restate(clouds[b], 77), b)
    x3, k3 = K.fps_clouds()[4]                                       # 4099 = 4 * 1024 + 3
    part = _run(x3[:2049], 33, STREAMED)
    _equals_restatement(part, K.fps_restate(x3[:2049], 33))


def test_runs_repeat_and_null_outputs():
    x, k = K.fps_clouds()[4]
    first = _run(x, k, STREAMED)
    for form in (RESIDENT, STREAMED):
        again = _run(x, k, form)
        for u, v in zip(first, again):
            assert torch.equal(u, v)
        for want in ((True, False, False), (False, True, False), (False, False, True)):
            only = _run(x, 64, form, want=want)
            full = _run(x, 64, form)
            for u, v in zip(only, full):
                assert u is None or torch.equal(u, v)


def test_abi_errors_leave_the_outputs_intact():
    x = K.fps_clouds()[2][0]
    big = torch.zeros(RESIDENT_MAX + 1, 3)

    def bad(expect, cloud=x, k=8, form=STREAMED, **edits):
        def over(args):
            for pos, fn in edits.items():
                args[int(pos[1:])] = fn(args[int(pos[1:])])
        rc, out, ok = _call(cloud, k, form, over=over)
        assert rc == expect, (rc, expect, edits)
        assert ok and all(_untouched(v) for v in out.values()), edits

    bad(LF_EINVAL, a0=lambda p: None)
    bad(LF_EINVAL, a2=lambda p: None, a3=lambda p: None, a4=lambda p: None)      # nothing asked for
    bad(LF_EINVAL, a1=lambda v: -3)                                  # negative stride
    bad(LF_EINVAL, a7=lambda v: 0)                                   # B
    bad(LF_EINVAL, a9=lambda v: 0)                                   # K < 1
    bad(LF_EINVAL, a9=lambda v: 258)                                 # K > N
    bad(LF_EINVAL, a10=lambda v: 3)                                  # form
    bad(LF_EINVAL, a10=lambda v: -1)
    bad(LF_EINVAL, a7=lambda v: 1 << 23, a8=lambda v: 1 << 8)        # B * N = 2^31
    bad(LF_EINVAL, cloud=big, form=RESIDENT)                         # above the resident limit
    for form in (RESIDENT, STREAMED):
        bad(LF_EALIGN, form=form, a0=lambda p: p + 2)
        bad(LF_EALIGN, form=form, a2=lambda p: p + 1)
        bad(LF_EALIGN, form=form, a3=lambda p: p + 2)
        bad(LF_EALIGN, form=form, a4=lambda p: p + 2)
        bad(LF_EALIGN, form=form, a5=lambda p: p + 2)
    bad(LF_ENOSPC, a6=lambda v: v - 1)
    bad(LF_ENOSPC, a5=lambda p: None)
    L = _L()
    assert L.lf_farthest_points_scratch_bytes(1, RESIDENT_MAX, 4, 0) == 0
    assert L.lf_farthest_points_scratch_bytes(1, RESIDENT_MAX + 1, 4, 0) == (RESIDENT_MAX + 1 + 4 * 10) * 4
    assert L.lf_farthest_points_scratch_bytes(1, RESIDENT_MAX + 1, 4, 1) == 0
    at_limit = torch.randn(RESIDENT_MAX, 3, generator=torch.Generator().manual_seed(5)).clamp(-4, 4)
    _equals_restatement(_both_forms(at_limit, 16), K.fps_restate(at_limit, 16))      # the largest resident cloud: all of LDS


def test_python_plumbing():
    from latentfusion_amd import ops
    from latentfusion_amd.three.utils import farthest_points
    x, k = K.fps_clouds()[2]
    expected = K.fps_expected(2)
    xd = x.to(DEV)
    out = ops.farthest_points(xd, k, want=('centers', 'owner', 'nearest'))
    assert out['centers'].shape == (k,) and out['centers'].dtype == torch.int32
    assert torch.equal(out['centers'].cpu(), expected[0]) and torch.equal(out['owner'].cpu(), expected[1])
    assert torch.equal(out['nearest'].cpu(), expected[2])
    for form in ('resident', 'streamed'):
        assert torch.equal(ops.farthest_points(xd, k, form=form)['centers'], out['centers'])
    shared = ops.farthest_points(xd.unsqueeze(0).expand(3, -1, -1), k, want='owner')['owner']
    assert shared.shape == (3, 257) and all(torch.equal(shared[b].cpu(), expected[1]) for b in range(3))
    # the tuple forms and dtypes of the composed call
    for kwargs in (dict(), dict(return_center_indexes=True), dict(return_center_indexes=True, return_distances=True),
                   dict(return_distances=True)):
        host = farthest_points(x, k, F.pairwise_distance, **kwargs)
        fused = farthest_points(xd, k, F.pairwise_distance, kernel='fused', **kwargs)
        host, fused = (host if isinstance(host, tuple) else (host,)), (fused if isinstance(fused, tuple) else (fused,))
        assert isinstance(fused, tuple) and len(host) == len(fused)
        for h, f in zip(host, fused):
            assert f.is_cuda and f.dtype == h.dtype and f.shape == h.shape
            if h.dtype == torch.long:
                assert torch.equal(f.cpu(), h)                      # a conditioned cloud
            else:
                assert float((f.cpu() - h).abs().max()) <= 4e-6
    ids, centers = farthest_points(xd, 300, None, return_center_indexes=True, kernel='fused')      # n_clusters >= N
    assert ids.is_cuda and torch.equal(ids.cpu(), torch.arange(257)) and torch.equal(centers.cpu(), torch.arange(257))
    assert farthest_points(xd, 257, None, kernel='fused').dtype == torch.long
    with pytest.raises(ValueError, match='dist_func'):
        farthest_points(xd, k, F.cosine_similarity, kernel='fused')
    with pytest.raises(ValueError, match='device tensor'):
        farthest_points(x, k, None, kernel='fused')
    with pytest.raises(ValueError, match=r'float32 \(N,3\)'):
        farthest_points(xd.double(), k, None, kernel='fused')
    with pytest.raises(ValueError, match='k must be'):
        ops.farthest_points(xd, 258)
    with pytest.raises(ValueError, match='k must be'):
        ops.farthest_points(xd, 0)
    with pytest.raises(ValueError, match="form='resident'"):
        ops.farthest_points(torch.zeros(RESIDENT_MAX + 1, 3, device=DEV), 2, form='resident')
    with pytest.raises(ValueError, match='must be shaped'):
        ops.farthest_points(xd[:, :2], 2)
    # the composed path serves device tensors too, on their device
    owner, cen = farthest_points(xd, k, F.pairwise_distance, return_center_indexes=True)
    assert owner.is_cuda and torch.equal(cen.cpu(), expected[0].long())


def test_eval_points_end_to_end():
    from latentfusion_amd import pointcloud, synth
    from latentfusion_amd.pose.metrics import camera_metrics_batch
    obs = synth.make_observation(4, 3)
    dev = obs.to(DEV)
    # the synthetic depth is 0 outside the mask: the composed path keeps whichever of those pixels' 0/0 re-projections happen to
    # land on the mask (every one of them a copy of the camera centre), the kernel keeps none -- the documented departure
    points_host, _, index_host, _ = K.composed(obs)
    live = obs.depth.reshape(-1)[index_host.long()] != 0
    print(f'eval_points: the composed path keeps {int((~live).sum())} zero-depth pixels besides the {int(live.sum())} of the mask')
    cloud_host = points_host[live]
    cloud = dev.pointcloud(kernel='fused')
    assert cloud.shape == cloud_host.shape                           # the same pixels (1 / 639 px margins, a few 1e-4 px of error)
    assert float((cloud.cpu() - cloud_host).abs().max()) <= 2e-5      # two fp32 chains of ~20 operations on |coordinates| <= 1.5
    pts = pointcloud.eval_points(dev, n_points=256, kernel='fused')
    assert pts.is_cuda and pts.shape == (256, 3) and pts.dtype == torch.float32
    centers = K.fps_restate(cloud.cpu(), 256)[0]
    assert torch.equal(pts.cpu(), cloud.cpu()[centers.long()])       # bit for bit the restatement on the fused cloud
    host = cloud_host[K.fps_composed(cloud_host, 256)[0]]            # the composed sampling of the same pixels on the CPU
    assert host.shape == (256, 3)
    # greedy farthest-point sampling is a 2-approximation of the optimal covering radius, so the two runs' radii (near-ties may
    # send their picks apart) are within a factor of 2 of each other
    def radius(picks):
        return max(float(torch.cdist(part.double(), picks.double()).amin(dim=1).max()) for part in cloud_host.split(32768))
    r_fused, r_host = radius(pts.cpu()), radius(host)
    print(f'eval_points: covering radius fused {r_fused:.5f}, composed {r_host:.5f}, same picks: {torch.equal(pts.cpu(), host)}')
    assert 0.5 * r_host <= r_fused * (1 + 1e-4) and r_fused <= 2.0 * r_host * (1 + 1e-4)
    cams = dev.camera
    m = camera_metrics_batch(cams[:1], cams, pts, 1.0)
    for name in ('add', 'add_s', 'add_sym', 'proj2d'):
        assert m[name].shape == (4,) and bool(torch.isfinite(m[name]).all()), name
    assert float(m['add'][0]) == 0.0 and float(m['add_s'][0]) == 0.0 and float(m['add'][1]) > 0.0
