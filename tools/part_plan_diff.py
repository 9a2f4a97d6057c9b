"""Which stage of an evaluation makes a target's rows depend on its batch mates?  Runs T targets x n hypotheses once through
engine_multi.MultiTargetEngine and once per target through engine.RenderLoopEngine on the released architecture (seeded
random weights and volume), records what every stage of RenderLoopEngine._forward_backward_group returns -- resample, each
camera-block convolution, the tail, the decoder / logits, the loss, each data gradient, the camera gradient -- and prints, per
stage, how many elements of the batched rows differ from the single-target rows, and the first stage that differs.
With --per-target-plan (MultiTargetEngine(per_target_plan=True)) every stage is expected to be bit-equal; without it the first
difference is the first wide convolution whose frequency split follows the batch (lf_wino_fused_gemm).

    python tools/part_plan_diff.py [--targets 3] [--n 2] [--per-target-plan] [--ranking] [--proj-kernel mfma|library]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _tensors(out):
    """The tensors of a stage's return value whose first axis is the hypothesis axis, flattened in order."""
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _tensors(o)]
    return []


class _Recorder:
    """Wraps the stage methods of one engine (and of its camera-block plan) so that every call appends (stage, tensors)."""
    STAGES = ('_resample', '_tail_fwd', '_decoder_fwd', '_decoder_autograd', '_decoder_bwd', '_tail_bwd', '_finish_backward')

    def __init__(self, eng):
        self.log = []
        for name in self.STAGES:
            self._wrap(eng, name, name.strip('_'))
        # (_loss_fwd(lg, coefs, masked_depth) -> (losses, gsums, scratch): the scratch has no row axis, and the forward-only
        # masked form leaves gsums unwritten)
        self._wrap(eng, '_loss_fwd', 'loss_fwd', pick=lambda out, a: out[:1] if a[2] else out[:2])
        self._wrap(eng.plan, 'forward', 'block_fwd', index=True)
        self._wrap(eng.plan, 'data_grad', 'block_data_grad', index=True)

    def _wrap(self, obj, name, label, index=False, pick=None):
        fn = getattr(obj, name)

        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            kept = out if pick is None else pick(out, a)
            tag = f'{label}[{a[0]}]' if index else label
            self.log.append((tag, [t.detach().clone() for t in _tensors(kept)]))
            return out
        setattr(obj, name, wrapped)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--targets', type=int, default=3)
    ap.add_argument('--n', type=int, default=2)
    ap.add_argument('--per-target-plan', action='store_true')
    ap.add_argument('--ranking', action='store_true', help='the forward-only masked-depth form')
    ap.add_argument('--proj-kernel', default=None)
    a = ap.parse_args()
    from latentfusion_amd import synth
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.engine_multi import MultiTargetEngine
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.pose import utils as pu
    dev = 'cuda'
    model, _ = synth.build_released_model(dev, seed=0)
    model.freeze()
    z_obj = torch.randn(1, 1, 256, 16, 16, 16, generator=torch.Generator().manual_seed(5)).to(dev)
    targets = []
    for t in range(a.targets):
        d = synth.make_observation_data(1, seed=200 + t)
        targets.append(Observation(d['color'], d['depth'], d['mask'], Camera(d['intrinsic'], d['extrinsic'])).to(dev))
    torch.manual_seed(300)
    cams = [pu.sample_cameras_with_estimate(a.n, t.camera.to('cpu')).zoom(None, model.input_size, model.camera_dist).to(dev)
            for t in targets]
    weights = {'depth': 1.0, 'ov_depth': 0.3, 'iou': 0.2, 'mask': 0.4}
    kw = dict(need_grad=not a.ranking, masked_depth=a.ranking)
    multi = MultiTargetEngine(model.photographer, z_obj, targets, weights, proj_kernel=a.proj_kernel, per_target_plan=a.per_target_plan)
    rec = _Recorder(multi)
    multi.forward_backward(Camera.cat(cams), a.n, **kw)
    torch.cuda.synchronize()
    singles = []
    for tg, c in zip(targets, cams):
        one = RenderLoopEngine(model.photographer, z_obj, tg, weights, proj_kernel=a.proj_kernel)
        r = _Recorder(one)
        one.forward_backward(c, **kw)
        torch.cuda.synchronize()
        singles.append(r.log)
    first = None
    N = a.targets * a.n
    for i, (tag, tens) in enumerate(rec.log):
        differ = total = 0
        for j, tb in enumerate(tens):
            if tb.dim() == 0 or tb.shape[0] != N:
                continue
            for t in range(a.targets):
                ts = singles[t][i][1][j]
                rows = tb[t * a.n:(t + 1) * a.n]
                differ += int((rows != ts).sum().item())
                total += rows.numel()
        print(f'{i:3d} {tag:24s} {differ:10d} of {total} elements differ')
        if differ and first is None:
            first = tag
    print('first stage whose rows differ:', first)


if __name__ == '__main__':
    main()
