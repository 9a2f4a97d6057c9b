"""Split-precision (f16x3) wide 3-D camera blocks: lf_wino3d_input_transform_f16x3 + lf_wino_fused_f16x3_gemm (the per-frequency
Winograd products from three f16 MFMAs per fp32 product) against fp64, against the fp32 kernel's own error, across gradient
scales, layouts and runs; the C ABI's argument checks; and RenderLoopEngine / the estimators with conv_mode='f16x3' on the
released-width (g20) and released-architecture (g25) models against the reference's goldens."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SHAPES = [(64, 64, 8, 2), (72, 132, 6, 1), (260, 64, 5, 3), (256, 256, 16, 2)]


def _problem(cin, cout, S, N):
    from latentfusion_amd import ops
    g = torch.Generator().manual_seed(cin * 10 + cout)
    x = torch.randn((N, cin) + (S,) * 3, generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), generator=g)
    b = torch.randn(cout, generator=g) * 0.1
    gin = torch.randn((N, cout) + (S,) * 3, generator=torch.Generator().manual_seed(1))
    return x, w, b, gin, ops.he_constant(w)


def _fwd_ref(x, w, b, he):
    pre = torch.nn.functional.conv3d(x.double(), w.double(), None, 1, 1) * he + b.double().view(1, -1, 1, 1, 1)
    act = torch.nn.functional.leaky_relu(pre, 0.2)
    return act / torch.sqrt((act ** 2).mean(dim=1, keepdim=True) + 1e-8)


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item()


@pytest.mark.parametrize('cin,cout,S,N', SHAPES)
def test_f16x3_matches_fp64_within_twice_the_fp32_kernel(cin, cout, S, N):
    """Forward (LeakyReLU + PixelNorm + bias) and data gradient: max error <= max(2 x the fp32 kernel's, 4e-6 max|ref|)."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    x, w, b, gin, he = _problem(cin, cout, S, N)
    xd, wd, bd, gd = ops.cl(x.to(DEV)), w.to(DEV), b.to(DEV), ops.cl(gin.to(DEV))
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
    want = _fwd_ref(x, w, b, he)
    gwant = torch.nn.functional.conv_transpose3d(gin.double(), w.double(), None, 1, 1) * he
    y32, _ = ops.wide_conv(xd, wd, bd, he, flags)
    g32, _ = ops.wide_conv(gd, wd, None, he, 0, transpose=True)
    y16, n16 = ops.wide_conv_f16x3(xd, wd, bd, he, flags)
    g16, _ = ops.wide_conv_f16x3(gd, wd, None, he, 0, transpose=True)
    torch.cuda.synchronize()
    e32, e16 = _err(y32, want), _err(y16, want)
    assert e16 <= max(2 * e32, 4e-6 * want.abs().max().item()), (e16, e32)
    ge32, ge16 = _err(g32, gwant), _err(g16, gwant)
    assert ge16 <= max(2 * ge32, 4e-6 * gwant.abs().max().item()), (ge16, ge32)
    assert n16 is not None and torch.isfinite(n16).all()


@pytest.mark.parametrize('k', [-30, -12, 0, 9])
def test_f16x3_gradient_scale_is_exact(k):
    """gx(g 2^k) == 2^k gx(g) bit for bit: the input scale is a power of two derived from the measured max, undone exactly."""
    from latentfusion_amd import ops
    x, w, _b, gin, he = _problem(256, 256, 8, 2)
    wd, gd = w.to(DEV), ops.cl(gin.to(DEV))
    g0, _ = ops.wide_conv_f16x3(gd, wd, None, he, 0, transpose=True)
    gk, _ = ops.wide_conv_f16x3(gd * 2.0 ** k, wd, None, he, 0, transpose=True)
    assert torch.equal(gk, g0 * 2.0 ** k)
    if k == -30:
        gwant = torch.nn.functional.conv_transpose3d(gin.double() * 2.0 ** k, w.double(), None, 1, 1) * he
        g32, _ = ops.wide_conv(ops.cl((gin * 2.0 ** k).to(DEV)), wd, None, he, 0, transpose=True)
        assert _err(gk, gwant) <= max(2 * _err(g32, gwant), 4e-6 * gwant.abs().max().item())


def test_f16x3_depth_inner_layout():
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU
    for cin, cout, S, N in ((256, 256, 16, 2), (72, 132, 6, 1)):
        x, w, b, _gin, he = _problem(cin, cout, S, N)
        xd, wd, bd = ops.cl(x.to(DEV)), w.to(DEV), b.to(DEV)
        y, _ = ops.wide_conv_f16x3(xd, wd, bd, he, LF_EPI_LRELU)
        yi, _ = ops.wide_conv_f16x3(xd, wd, bd, he, LF_EPI_LRELU, depth_inner=True)
        assert tuple(yi.shape) == (N, S, S, S, cout)
        assert torch.equal(yi, y.permute(0, 3, 4, 2, 1))                # (N, C, D, H, W) -> (N, H, W, D, C)


def test_f16x3_run_to_run_identical():
    """128-render 256 -> 256 forward and data gradient, twice: bit-identical."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    g = torch.Generator(device=DEV).manual_seed(3)
    xd = ops.cl(torch.randn(128, 256, 16, 16, 16, device=DEV, generator=g))
    gd = ops.cl(torch.randn(128, 256, 16, 16, 16, device=DEV, generator=g) * 1e-7)
    wd = torch.randn(256, 256, 3, 3, 3, device=DEV, generator=g)
    bd = torch.randn(256, device=DEV, generator=g) * 0.1
    he = ops.he_constant(wd)
    outs = []
    for _ in range(2):
        y, _n = ops.wide_conv_f16x3(xd, wd, bd, he, LF_EPI_LRELU | LF_EPI_PIXELNORM)
        gx, _ = ops.wide_conv_f16x3(gd, wd, None, he, 0, transpose=True)
        outs.append((y, gx))
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_f16x3_abi_rejects_bad_arguments():
    """NULL operands, Cin / Cout not multiples of 4, bad flags and short scratch return negative codes and write nothing."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    N, S, cin, cout = 1, 4, 64, 64
    x = ops.cl(torch.randn(N, cin, S, S, S, device=DEV))
    w = torch.randn(cout, cin, 3, 3, 3, device=DEV)
    U2, eU = ops.pack_conv_wino_fused_f16x3(w)
    T = L.lf_wino3d_tiles(N, S, S, S)
    V = torch.zeros(64, T, L.lf_wino_f16x3_cin_padded(cin) * 2, device=DEV, dtype=torch.float16)
    amax = ops.amax_buffer(x.abs().amax(), DEV)
    assert L.lf_wino3d_input_transform_f16x3(x.data_ptr(), amax.data_ptr(), V.data_ptr(), N, S, S, S, cin, None) == 0
    y = torch.full((N, S, S, S, cout), 1234.5, device=DEV)
    nscr = L.lf_wino_fused_f16x3_scratch_bytes(N, S, S, S, cout)
    assert nscr > 0                                                       # a small problem: split over the frequencies
    scr = torch.empty(nscr // 4, device=DEV)
    torch.cuda.synchronize()

    def call(V_=V.data_ptr(), U_=U2.data_ptr(), y_=y.data_ptr(), scr_=scr.data_ptr(), nb=nscr, ci=cin, co=cout, flags=1):
        return L.lf_wino_fused_f16x3_gemm(V_, U_, eU, amax.data_ptr(), None, y_, None, scr_, nb, N, S, S, S, ci, co, 1.0, flags,
                                          0.2, None)
    for kw in (dict(V_=None), dict(U_=None), dict(y_=None), dict(ci=62), dict(co=66), dict(flags=2), dict(ci=0)):
        assert call(**kw) < 0, kw
    assert call(scr_=None) < 0 and call(nb=nscr - 16) < 0
    assert L.lf_wino3d_input_transform_f16x3(None, amax.data_ptr(), V.data_ptr(), N, S, S, S, cin, None) < 0
    assert L.lf_wino3d_input_transform_f16x3(x.data_ptr(), amax.data_ptr(), V.data_ptr(), N, S, S, S, 62, None) < 0
    torch.cuda.synchronize()
    assert bool((y == 1234.5).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((y == 1234.5).any())


# ----------------------------------------------------------------------------------------------------------------------
# engine and estimators
# ----------------------------------------------------------------------------------------------------------------------
def _rw():
    import test_released_width_gpu as rw
    return rw


def test_g20_engine_f16x3(golden):
    """RenderLoopEngine(conv_mode='f16x3') on the released-width model: every camera-block convolution on the new kernel, loss
    components, camera gradients and loss order within the bars of the fp32 wide branch."""
    from latentfusion_amd.engine import RenderLoopEngine, _WideWinogradF16x3
    rw = _rw()
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = rw._model(g)
    L = g['loss']
    eng = RenderLoopEngine(model.photographer, g['z_obj'].to(DEV), rw._target(t7), L['weights'], conv_mode='f16x3')
    assert eng.conv_mode == 'f16x3' and type(eng.plan) is _WideWinogradF16x3
    zc = rw.prod_camera(L['zoomed'])
    (losses, gparams), tags = rw._wide_kernels_used(lambda: eng.forward_backward(zc))
    assert 'wino3d_fused_f16x3' in tags and 'wino3d_fused' not in tags, tags
    for i, k in enumerate(eng.LOSS_KEYS):
        rw.close(losses[:, i], L['components'][k], atol=2e-5, rtol=1e-3)
    rw.close(losses[:, 4], L['total'], atol=2e-5, rtol=1e-3)
    want = torch.cat((L['g_log_q'], L['g_t'], L['g_viewport']), dim=1)
    rel = ((gparams.cpu() - want).norm(dim=1) / want.norm(dim=1)).max().item()
    assert rel < 1e-2, rel
    assert torch.equal(torch.argsort(losses[:, 4].cpu()), torch.argsort(L['total']))
    # the ranking form (forward only: the last block depth-innermost) runs on the new kernel as well
    (lr_, _), tags = rw._wide_kernels_used(lambda: eng.forward_backward(zc, need_grad=False))
    assert 'wino3d_fused_f16x3' in tags and 'wino3d_fused' not in tags, tags
    rw.close(lr_[:, 4], L['total'], atol=2e-5, rtol=1e-3)


def test_g20_engine_f16x3_keeps_the_unsupported_combinations_refused(golden):
    from latentfusion_amd.engine import RenderLoopEngine
    rw = _rw()
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = rw._model(g)
    ph = model.photographer
    ph.projection_type, old = 'sum', ph.projection_type
    try:
        with pytest.raises(NotImplementedError):
            RenderLoopEngine(ph, g['z_obj'].to(DEV), rw._target(t7), g['loss']['weights'], conv_mode='f16x3')
    finally:
        ph.projection_type = old


def test_g20_gradient_estimator_f16x3(golden):
    from latentfusion_amd.pose import estimation
    rw = _rw()
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = rw._model(g)
    L = g['loss']
    est = estimation.GradientPoseEstimator(model=model, learning_rate=0.01, num_samples=4, num_iters=2, ranking_size=4,
                                           converge_threshold=1e-6, converge_patience=10, optimizer='adam',
                                           loss_weights=L['weights'], conv_mode='f16x3', track_stats=True)
    best, stats = est.estimate(g['z_obj'].to(DEV), rw._target(t7, 'cpu'), camera=rw.prod_camera(L['init'], 'cpu'))
    rw.close(stats['rank_loss'][0], L['total'], atol=2e-5, rtol=1e-3)
    assert int(torch.argmin(stats['rank_loss'][0])) == int(torch.argmin(L['total']))
    assert all(torch.isfinite(r).all() for r in stats['rank_loss'])
    assert torch.isfinite(best.log_quaternion).all() and torch.isfinite(best.translation).all()


def test_cfg3_released_architecture_f16x3(golden):
    """The 68 M-parameter architecture (golden g25): evaluate_samples with conv_mode='f16x3' meets the loss / order bars of the
    fp32 path; the full cross_entropy_linemod preset (N = 128, 2 iterations) twice: finite and identical."""
    import numpy as np

    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation
    import test_fullshape_gpu as fs
    g = golden('g25_released_arch')
    seed = g['seed']
    model, _cks = synth.build_released_model(DEV, seed, 0.1)
    ref = fs._observation(synth.make_observation_data(g['views'], seed + 10))
    target = fs._observation(synth.make_observation_data(1, seed + 20))
    z_obj = model.build_latent_object(ref)
    est = estimation.CrossEntropyPoseEstimator(model=model, num_samples=16, num_elites=6, num_iters=1, num_gmm_components=2,
                                               learning_rate=0.9, sample_flipped=True, ranking_size=4, loss_weights=g['weights'],
                                               conv_mode='f16x3')
    cams, loss = est.evaluate_samples(z_obj, target, fs.prod_camera(g['cams']))
    fs.close(loss, g['loss'], atol=2e-5, rtol=1e-3)
    assert fs.same_order_up_to_ties(loss, g['loss'], 2e-5) and int(torch.argmin(loss)) == int(g['order'][0])
    cfg = estimation._load_toml(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs',
                                             'cross_entropy_linemod.toml'))
    cfg['args']['num_iters'] = 2
    runs = []
    for _ in range(2):
        torch.manual_seed(7)
        np.random.seed(7)
        est = estimation.load_from_config(cfg, model, conv_mode='f16x3')
        best = est.estimate(z_obj, target, camera=target.camera)
        runs.append(torch.cat((best.log_quaternion, best.translation), dim=1).cpu())
    assert torch.isfinite(runs[0]).all() and len(runs[0]) == cfg['args']['ranking_size']
    assert torch.equal(runs[0], runs[1])
