"""Host side of the fused observation preprocessing (ops.observation_prepare, Observation.zoom `kernel`, observation.KERNEL,
LatentFusionModel `preprocess_kernel`, Sculptor.encode `x`): the wrapper's argument checks (which raise before any library
call), the option values and the switch, what 'fused' does without a GPU or on host tensors, and the binding table.  No GPU."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_observation(B=2, H=8, W=10):
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    g = torch.Generator().manual_seed(0)
    K = torch.tensor([[12.0, 0.0, 5.0], [0.0, 12.0, 4.0], [0.0, 0.0, 1.0]]).expand(B, -1, -1).clone()
    E = torch.eye(4).expand(B, -1, -1).clone()
    E[:, 2, 3] = 1.0
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.4).float()
    return Observation(torch.rand(B, 3, H, W, generator=g), torch.rand(B, 1, H, W, generator=g) + 0.5, mask,
                       Camera(K, E, width=W, height=H))


def test_wrapper_checks_raise_before_any_library_call(monkeypatch):
    from latentfusion_amd import _lib, ops

    def no_library():
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'lib', no_library)
    host = torch.ones(2, 1, 8, 8)
    with pytest.raises(ValueError, match='device'):
        ops.observation_prepare(None, host, host, torch.zeros(2, 4), 4)          # host tensors
    with pytest.raises(ValueError):
        ops.observation_prepare(None, host.tolist(), host, torch.zeros(2, 4), 4)  # not a tensor
    # the rules on meta tensors that claim to be on the device (see tests/test_depth_init_args.py): nothing reaches the library
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: self.device.type == 'meta'))

    def meta(*shape, dtype=torch.float32):
        return torch.empty(*shape, device='meta', dtype=dtype)
    c, d, mk, bx, z = meta(2, 3, 8, 8), meta(2, 1, 8, 8), meta(2, 1, 8, 8), meta(2, 4), meta(2)
    good = dict(color=c, depth=d, mask=mk, boxes=bx, target_size=4, zn=z, zf=z, prepare=True, normalize=True, stack='color_mask')
    bad = [dict(depth=d.double()), dict(depth=d.half()), dict(mask=mk.double()), dict(mask=mk.to(torch.int32)),
           dict(mask=mk.to(torch.int8)), dict(depth=meta(2, 2, 8, 8), mask=meta(2, 2, 8, 8)), dict(depth=meta(8, 8), mask=meta(8, 8)),
           dict(depth=meta(0, 1, 8, 8), mask=meta(0, 1, 8, 8), color=meta(0, 3, 8, 8)), dict(mask=meta(2, 1, 8, 9)),
           dict(mask=meta(3, 1, 8, 8)), dict(mask=host), dict(depth=host),
           dict(color=c.double()), dict(color=meta(2, 3, 8, 9)), dict(color=meta(3, 3, 8, 8)), dict(color=meta(3, 8, 8)),
           dict(color=torch.ones(2, 3, 8, 8)), dict(color=[[1.0]]),
           dict(boxes=torch.zeros(2, 4)), dict(boxes=meta(2, 4, dtype=torch.float64)), dict(boxes=meta(3, 4)), dict(boxes=meta(2, 5)),
           dict(boxes=meta(8)), dict(boxes=[[0.0, 0.0, 4.0, 4.0]] * 2), dict(boxes=None),
           dict(target_size=0), dict(target_size=-4), dict(target_size=4.0), dict(target_size=None), dict(target_size=True),
           dict(zn=None), dict(zf=None), dict(zn=meta(3)), dict(zf=meta(2, 1)), dict(zn=meta(2, dtype=torch.float64)),
           dict(zf=torch.zeros(2)), dict(zn=1.0),
           dict(prepare=1), dict(normalize=None), dict(normalize='yes'),
           dict(stack='mask'), dict(stack='color'), dict(stack=True), dict(stack=['color_mask']),
           # B * max(C, 1) * H * W and B * (C + 2) * T^2 stay below 2^31
           dict(color=None, depth=meta(1 << 15, 1 << 8, 1 << 8), mask=meta(1 << 15, 1 << 8, 1 << 8, dtype=torch.uint8),
                boxes=meta(1 << 15, 4), zn=meta(1 << 15), zf=meta(1 << 15)),
           dict(target_size=1 << 14)]
    for over in bad:
        with pytest.raises(ValueError):
            ops.observation_prepare(**dict(good, **over))
    # and the forms it accepts get as far as the library
    for kw in (good, dict(good, color=None, stack=None), dict(good, mask=meta(2, 8, 8, dtype=torch.bool), depth=meta(2, 8, 8)),
               dict(good, mask=mk.to(torch.uint8), stack='color_depth_mask', target_size=1),
               dict(color=c, depth=d, mask=mk, boxes=bx, target_size=3),
               dict(color=c, depth=d, mask=mk, boxes=bx, target_size=3, prepare=True, zn=None, zf=None)):
        with pytest.raises(AssertionError, match='the library was asked for'):
            ops.observation_prepare(**kw)


def test_option_values_and_the_switch(monkeypatch):
    from latentfusion_amd import observation as obsmod
    from latentfusion_amd import ops
    from latentfusion_amd.recon.inference import LatentFusionModel
    assert obsmod.KERNEL == 'composed' and obsmod.KERNELS == ('composed', 'fused')
    assert ops.OBS_STACKS == (None, 'color_mask', 'color_depth_mask')
    assert inspect.signature(obsmod.Observation.zoom).parameters['kernel'].default is None
    assert inspect.signature(obsmod.Observation.zoom_estimate).parameters['zoom_kernel'].default is None
    for fn in (LatentFusionModel.__init__, LatentFusionModel.from_checkpoint):
        assert inspect.signature(fn).parameters['preprocess_kernel'].default == 'composed'
    p = inspect.signature(ops.observation_prepare).parameters
    assert list(p) == ['color', 'depth', 'mask', 'boxes', 'target_size', 'zn', 'zf', 'prepare', 'normalize', 'stack']
    assert (p['zn'].default, p['zf'].default, p['prepare'].default, p['normalize'].default, p['stack'].default) == \
        (None, None, False, False, None)
    obs = _host_observation()
    for bad in ('hip', 'Fused', '', 0, True):
        with pytest.raises(ValueError, match='kernel'):
            obs.zoom(1.0, 4, kernel=bad)
        with pytest.raises(ValueError, match='kernel'):
            obs.zoom_estimate(1.0, 4, zoom_kernel=bad)
    # the default is the composed path, and the module switch is what None resolves to
    a, b = obs.zoom(1.0, 4), obs.zoom(1.0, 4, kernel='composed')
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in ('color', 'depth', 'mask'))
    assert a.meta['is_zoomed'] and not a.meta['is_prepared'] and not a.meta['is_normalized']
    reached = []
    monkeypatch.setattr(obsmod, 'fused_preprocess', lambda *args, **kw: (reached.append(kw), (None, None))[1])
    monkeypatch.setattr(obsmod, 'KERNEL', 'fused')
    assert obs.zoom(1.0, 4) is None and len(reached) == 1
    c = obs.zoom(1.0, 4, kernel='composed')
    assert torch.equal(c.color, a.color) and len(reached) == 1
    monkeypatch.setattr(obsmod, 'KERNEL', 'hip')
    with pytest.raises(ValueError, match='kernel'):
        obs.zoom(1.0, 4)


class _Net(torch.nn.Module):
    in_size = 4
    input_color = input_mask = True
    input_depth = False

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def _model(**kw):
    from latentfusion_amd.recon.inference import LatentFusionModel
    return LatentFusionModel(_Net(), _Net(), _Net(), 1.0, 'cpu', **kw)


def test_model_option_and_host_observations(monkeypatch):
    from latentfusion_amd.recon import inference
    assert _model().preprocess_kernel == 'composed' and _model(preprocess_kernel='fused').preprocess_kernel == 'fused'
    for bad in ('hip', None, '', 'Fused'):
        with pytest.raises(ValueError, match='preprocess_kernel'):
            _model(preprocess_kernel=bad)
    # a host observation, or one with any meta flag set, takes the composed steps under either value: same results
    monkeypatch.setattr(inference, 'fused_preprocess', lambda *a, **k: (_ for _ in ()).throw(AssertionError('fused was taken')))
    obs = _host_observation()
    ref = _model().preprocess_observation(obs)
    assert all(ref.meta[k] for k in ('is_zoomed', 'is_prepared', 'is_normalized'))
    got = _model(preprocess_kernel='fused').preprocess_observation(obs)
    assert all(torch.equal(getattr(ref, k), getattr(got, k)) for k in ('color', 'depth', 'mask'))
    # ... and the decision itself: device tensors and no flag
    m = _model(preprocess_kernel='fused')
    monkeypatch.setattr(torch.Tensor, 'is_cuda', property(lambda self: True))
    assert m._fused_applies(obs) and not _model()._fused_applies(obs)
    for flag in ('is_zoomed', 'is_prepared', 'is_normalized'):
        o = obs.clone()
        o.meta[flag] = True
        assert not m._fused_applies(o)


def test_fused_without_a_gpu_or_on_host_tensors_raises(monkeypatch):
    """No silent fall-back: 'fused' on host tensors is an error that says so, on every way in."""
    from latentfusion_amd import _lib
    monkeypatch.setattr(_lib, 'lib', lambda: (_ for _ in ()).throw(AssertionError('the library was asked for')))
    obs = _host_observation()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    for call in (lambda: obs.zoom(1.0, 4, kernel='fused'), lambda: obs.zoom(1.0, 4, camera=obs.camera, kernel='fused'),
                 lambda: obs.zoom_estimate(1.0, 4, zoom_kernel='fused')):
        with pytest.raises(RuntimeError, match='GPU'):
            call()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)                # a GPU in the process, the tensors on the host
    with pytest.raises(ValueError, match='device tensors'):
        obs.zoom(1.0, 4, kernel='fused')


def test_entry_point_is_bound_with_the_headers_argument_count():
    from latentfusion_amd import _lib
    from latentfusion_amd.csrc import build
    assert 'obs_prepare.hip' in build.SOURCES and 'obs_prepare.hip' not in build.EXTRA          # the default flags only
    header = open(os.path.join(ROOT, 'include', 'lf_hip.h')).read()
    for cite in ('modules/geometry.py:20-44,287-354', 'observation.py:225-282', 'recon/models.py'):
        assert cite in header, cite
    assert re.search(r'#define\s+LF_OBS_PREPARE\s+1\b', header) and re.search(r'#define\s+LF_OBS_NORMALIZE\s+2\b', header)
    assert (_lib.LF_OBS_PREPARE, _lib.LF_OBS_NORMALIZE) == (1, 2)
    header = re.sub(r'/\*.*?\*/', ' ', header, flags=re.S)
    proto = re.search(r'\blf_obs_prepare\s*\(([^)]*)\)', header)
    assert proto is not None
    assert len(_lib.SIGNATURES['lf_obs_prepare'][1]) == len(proto.group(1).split(',')) == 20
    binding = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    row = [ln for ln in binding.split('\n') if ln.startswith('|') and '`lf_obs_prepare`' in ln]
    assert len(row) == 1 and 'observation.py:225-282' in row[0]
    # the argument rules are decided on the host, before anything is launched: no GPU is needed to see them
    L = _lib.lib()
    n = None
    assert L.lf_obs_prepare(n, n, n, 0, n, n, n, n, n, n, n, 0, 0, 1, 0, 1, 1, 1, 0, n) == -1
    one = 16                                                                     # an aligned non-NULL address that is never read
    args = dict(color=n, depth=one, mask=one, u8=0, boxes=one, zn=n, zf=n, co=n, do=one, mo=one, stack=n, stride=0, sd=0, B=1, C=0,
                H=1, W=1, T=1, stages=0)

    def call(**over):
        return L.lf_obs_prepare(*dict(args, **over).values(), n)
    for over in (dict(B=0), dict(H=0), dict(W=0), dict(T=0), dict(C=-1), dict(C=1), dict(u8=2), dict(stages=4), dict(stages=2),
                 dict(stages=3, zn=one), dict(sd=2), dict(stack=one, stride=1, sd=1), dict(B=1 << 15, H=1 << 8, W=1 << 8),
                 dict(B=1 << 11, T=1 << 10), dict(H=1 << 16, W=1 << 16), dict(T=1 << 16), dict(depth=n), dict(mask=n), dict(boxes=n),
                 dict(do=n), dict(mo=n)):
        assert call(**over) == -1, over
    for over in (dict(depth=18), dict(mask=17), dict(boxes=18), dict(do=19), dict(mo=18), dict(stack=18, stride=1),
                 dict(stages=2, zn=18, zf=one), dict(stages=2, zn=one, zf=17), dict(C=1, color=18, co=one), dict(C=1, color=one, co=17)):
        assert call(**over) == -2, over


def test_encode_takes_the_stacked_input():
    """Sculptor.encode(x=...) equals the concatenated form (the default path is untouched)."""
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import gan_normalize
    from latentfusion_amd.recon.models import Sculptor
    seen = []

    class Probe(Sculptor):
        def __init__(self, input_depth):
            torch.nn.Module.__init__(self)
            self.input_color, self.input_depth, self.input_mask = True, input_depth, True
            self.in_channels = 4 + int(input_depth)
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x, camera):
            seen.append(x)
            return x, [], []

    def fuser(z, z_cam_mid, z_obj_mid, camera):
        return z, None
    g = torch.Generator().manual_seed(1)
    color, depth = torch.rand(1, 3, 3, 5, 5, generator=g) * 2 - 1, torch.rand(1, 3, 1, 5, 5, generator=g) * 2 - 1
    mask = (torch.rand(1, 3, 1, 5, 5, generator=g) > 0.5).float()
    cam = Camera(torch.eye(3).expand(3, -1, -1).clone(), torch.eye(4).expand(3, -1, -1).clone(), width=5, height=5)
    for input_depth in (False, True):
        net = Probe(input_depth)
        parts = [color[0]] + ([depth[0]] if input_depth else []) + [gan_normalize(mask[0])]
        x = torch.cat(parts, dim=1)
        del seen[:]
        a, _ = net.encode(fuser, cam, color, depth, mask)
        b, _ = net.encode(fuser, cam, color, depth, mask, x=x.clone())
        assert torch.equal(a, b) and torch.equal(seen[0], seen[1]) and tuple(a.shape) == (1, 3, 4 + int(input_depth), 5, 5)
        for bad in (x[:, :-1], x[0], x.unsqueeze(0)):
            with pytest.raises(ValueError, match='x must be'):
                net.encode(fuser, cam, color, depth, mask, x=bad)
    assert inspect.signature(Sculptor.encode).parameters['x'].default is None
