"""bench.py --dump-outputs and --steps: the arrays written after the timed steps are what the headline loop computed in its
last timed iteration, the same from run to run, and the timed region holds exactly --steps iterations."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine_state(N=4, step=7):
    """The loop state GradientPoseEstimator.iterate leaves on the fused engine, with synthetic values."""
    from latentfusion_amd.modules.geometry import Camera
    g = torch.Generator().manual_seed(3)
    P = torch.randn(N, 10, generator=g).requires_grad_(True)
    P.grad = torch.randn(N, 10, generator=g)
    pinned = {0: torch.randn(N, 16, generator=g), 1: torch.randn(N, 16, generator=g)}
    cams = Camera(torch.eye(3).expand(N, 3, 3), None, log_quaternion=torch.randn(N, 3, generator=g),
                  translation=torch.randn(N, 3, generator=g))
    ranking = sorted(((c, float(l), s) for c, l, s in zip(cams, torch.rand(N, generator=g), range(N))), key=lambda r: r[1])
    return {'params': [P], 'P': P, 'pinned': pinned, 'step': step, 'ranking': ranking}


def test_last_step_outputs_are_copies_of_the_last_iteration(tmp_path):
    import bench
    st = _engine_state()
    got = bench.last_step_outputs(st)
    last = st['pinned'][(st['step'] - 1) & 1]
    assert np.array_equal(got['losses'], last[:, :6].numpy())
    assert np.array_equal(got['camera_params'], last[:, 6:].numpy())
    assert np.array_equal(got['camera_grad'], st['P'].grad.numpy())
    assert np.array_equal(got['camera_params_updated'], st['P'].detach().numpy())
    assert np.array_equal(got['ranking_loss'], np.array([r[1] for r in st['ranking']]))
    assert np.array_equal(got['ranking_step'], np.array([r[2] for r in st['ranking']], dtype=np.float64))
    assert got['ranking_log_quaternion'].shape == (4, 3) and got['ranking_translation'].shape == (4, 3)
    assert np.array_equal(got['ranking_translation'][0], st['ranking'][0][0].translation[0].numpy())
    # host copies: later iterations overwrite the loop's buffers, not the snapshot
    before = {k: v.copy() for k, v in got.items()}
    with torch.no_grad():
        st['P'].add_(1.0)
    for t in st['pinned'].values():
        t.zero_()
    assert all(np.array_equal(got[k], before[k]) for k in got)

    names, nbytes = bench.write_outputs(str(tmp_path / 'out'), got)
    assert names == sorted(got) and nbytes == sum(v.nbytes for v in got.values())
    for k in names:
        back = np.load(tmp_path / 'out' / (k + '.npy'))
        assert back.dtype in (np.float32, np.float64) and np.array_equal(back, got[k])
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / 'bad'), {'i': np.arange(3)})
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / 'big'), {'x': np.zeros(1024, np.float32)}, limit=1000)
    assert not (tmp_path / 'bad').exists() and not (tmp_path / 'big').exists()


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + args, capture_output=True, text=True, timeout=600,
                       env={k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE')})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_and_times_exactly_steps(tmp_path):
    """Two runs with the same arguments write the same arrays; splitting the timed iterations into blocks changes neither
    their number nor what the loop computes."""
    small = ['--gpus', '1', '--warmup', '2', '--size', '32', '--views', '2', '--samples', '4', '--no-cpu-baseline', '--no-alt',
             '--no-cfg3', '--no-cfg5', '--no-variants', '--no-live-pmc']
    one = _bench(small + ['--steps', '3', '--dump-outputs', str(tmp_path / 'a')])
    three = _bench(small + ['--steps', '3', '--repeats', '3', '--dump-outputs', str(tmp_path / 'b')])
    for d in (one, three):
        assert d['steps'] == 3
        assert abs(d['ms_per_step'] * 3 - d['timing']['gpu_timed_total_s'] * 1e3) < 1e-6 * d['ms_per_step']
    assert len(one['timing']['ms_per_step_blocks']) == 1 and len(three['timing']['ms_per_step_blocks']) == 3
    names = sorted(f for f in os.listdir(tmp_path / 'a'))
    assert names == sorted(f for f in os.listdir(tmp_path / 'b'))
    assert {'losses.npy', 'camera_params.npy', 'camera_grad.npy', 'camera_params_updated.npy', 'ranking_loss.npy'} <= set(names)
    assert one['dump_outputs']['arrays'] == [n[:-4] for n in names]
    for n in names:
        x, y = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and np.isfinite(x).all(), n
        assert x.shape[0] == 4, n
        np.testing.assert_allclose(x, y, rtol=1e-5, atol=1e-6, err_msg=n)


def test_full_is_off_by_default():
    """A plain bench.py run is the headline alone; `--full` adds the secondary measurements and checks."""
    import bench
    assert bench.parse([]).full is False
    assert bench.parse(['--full']).full is True


@pytest.mark.gpu
def test_plain_bench_run_is_the_headline_alone():
    """Without --full the line carries the headline and its timing, and none of the secondary blocks: they are not run."""
    d = _bench(['--gpus', '1', '--warmup', '1', '--steps', '2', '--size', '32', '--views', '2', '--samples', '4'])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'timing', 'roofline'):
        assert k in d, k
    assert d['steps'] == 2 and d['warmup'] == 1 and d['roofline']['launches_timed'] > 0
    for k in ('cpu_baseline', 'alt', 'cfg3', 'cfg5', 'renderer_variants', 'reference_trace_parity', 'sharded_build', 'rccl',
              'summary'):
        assert k not in d, k
    assert 'kernels' not in d['roofline_iter'] and d['roofline']['traffic_live'] is None
