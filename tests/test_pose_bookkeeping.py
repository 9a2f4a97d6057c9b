"""CPU: the per-target bookkeeping of the gradient pose loop (GradientPoseEstimator._bookkeep: ranking, histories, statistics,
convergence counter) on synthetic host rows.  Two records side by side, a converged one frozen as the batched driver freezes
it, end up exactly as two one-target runs on the same rows."""
import torch

T, n, STEPS = 2, 3, 6
KEYS = ('depth', 'ov_depth', 'iou', 'mask')
WEIGHTS = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}


def _obs(h=48, w=64):
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    K = torch.tensor([[[500.0, 0.0, w / 2], [0.0, 500.0, h / 2], [0.0, 0.0, 1.0]]])
    E = torch.eye(4).unsqueeze(0).clone()
    E[:, 2, 3] = 1.0
    return Observation(torch.zeros(1, 3, h, w), torch.ones(1, 1, h, w), torch.ones(1, 1, h, w), Camera(K, E, width=w, height=h))


def _cams(n):
    from latentfusion_amd.modules.geometry import Camera
    return Camera(torch.eye(3).expand(n, -1, -1), None, log_quaternion=torch.zeros(n, 3),
                  translation=torch.tensor([[0.0, 0.0, 1.0]]).expand(n, -1))


def _est():
    from latentfusion_amd.pose import estimation
    return estimation.GradientPoseEstimator(model=None, learning_rate=0.01, num_samples=n, num_iters=STEPS, ranking_size=2,
                                            converge_threshold=1e-3, converge_patience=1, loss_weights=WEIGHTS,
                                            track_stats=True, return_camera_history=True)


def _rows():
    """Per step: rank loss (T*n,), components {name: (T*n,)}, log-quaternions and translations (T*n, 3).  The best loss of
    target 0 improves by 0.5, then by 1e-4 (< the threshold: it converges at step 2), then by 0.2 per step -- which a frozen
    record must not see; target 1's improves by 0.1 every step."""
    g = torch.Generator().manual_seed(0)
    best0 = [1.0, 0.5, 0.4999, 0.3, 0.1, 0.05]
    out = []
    for step in range(STEPS):
        rank = torch.cat((best0[step] + torch.tensor([0.0, 0.25, 0.5]), 2.0 - 0.1 * step + torch.tensor([0.5, 0.0, 0.25])))
        comp = {k: torch.rand(T * n, generator=g) for k in KEYS}
        out.append((rank, comp, torch.randn(T * n, 3, generator=g) * 0.1, torch.randn(T * n, 3, generator=g) * 0.1 + 1.0))
    return out


def _run(est, targets, rows, freeze):
    """Drives the records of `targets` (indices into the T x n rows) over the steps; returns them and each one's last step."""
    recs = [est._record(_obs(), None, _cams(n)) for _ in targets]
    last = [None] * len(targets)
    for step, (rank, comp, lq, tr) in enumerate(rows):
        for i, t in enumerate(targets):
            if recs[i].get('done'):
                continue
            r = slice(t * n, (t + 1) * n)
            cams = recs[i]['template_cpu']._like(log_quaternion=lq[r].clone(), translation=tr[r].clone(), viewport=None)
            done = est._bookkeep(recs[i], step, rank[r], cams, WEIGHTS, {k: v[r] for k, v in comp.items()}, comp['depth'][r])
            last[i] = step
            if freeze:
                recs[i]['done'] = done
    return recs, last


def _same_record(a, b):
    assert a['converge_count'] == b['converge_count']
    assert [(e, s) for _, e, s in a['ranking']] == [(e, s) for _, e, s in b['ranking']]
    for (ca, _, _), (cb, _, _) in zip(a['ranking'], b['ranking']):
        assert torch.equal(ca.log_quaternion, cb.log_quaternion) and torch.equal(ca.translation, cb.translation)
    assert a['stat_history'].keys() == b['stat_history'].keys()
    for k in a['stat_history']:
        assert torch.equal(a['stat_history'][k], b['stat_history'][k]), k
    assert len(a['camera_history']) == len(b['camera_history'])
    for (ra, ca), (rb, cb) in zip(a['camera_history'], b['camera_history']):
        assert torch.equal(ra, rb) and torch.equal(ca.log_quaternion, cb.log_quaternion) and torch.equal(ca.translation, cb.translation)


def test_two_records_side_by_side_equal_two_one_target_runs():
    est, rows = _est(), _rows()
    both, last = _run(est, [0, 1], rows, freeze=True)
    for t in range(T):
        alone, last_alone = _run(est, [t], rows, freeze=True)
        assert last[t] == last_alone[0]
        _same_record(both[t], alone[0])
    # target 0 converged at step 2 and was frozen there; target 1 ran all the steps
    assert last == [2, STEPS - 1]
    assert both[0]['converge_count'] == 1 and both[0]['done'] and not both[1]['done']
    assert len(both[0]['camera_history']) == 3 and len(both[1]['camera_history']) == STEPS
    assert both[0]['stat_history']['rank_loss'].shape == (3, n) and both[1]['stat_history']['rank_loss'].shape == (STEPS, n)
    assert [s for _, _, s in both[0]['ranking']] == [2, 1] and [s for _, _, s in both[1]['ranking']] == [5, 4]
    assert both[0]['stat_history']['converge_count'].tolist() == [0, 0, 0]      # (the count BEFORE each step's update)


def test_a_record_that_is_not_frozen_goes_on_ranking():
    """iterate() never freezes: after convergence a one-target state goes on ranking and recording (the benchmark and the
    tools call it past convergence), and the counter falls back to 0 on the next real improvement."""
    est, rows = _est(), _rows()
    (rec,), last = _run(est, [0], rows, freeze=False)
    assert last == [STEPS - 1] and 'done' not in rec
    assert len(rec['camera_history']) == STEPS and [s for _, _, s in rec['ranking']] == [5, 4]
    assert rec['stat_history']['converge_count'].tolist() == [0, 0, 0, 1, 0, 0]
