"""Split-precision (f16x3) wide 2-D convolutions: lf_wino2d_input_transform_f16x3 (per-tile power-of-two input scale) +
lf_wino_fused2d_f16x3_gemm against fp64 and against the fp32 kernel's own error, across tile magnitudes, gradient scales,
non-finite inputs and runs; the C ABI's argument checks; the ops.wide2d_f16x3 scope and the decoder routing of
RenderLoopEngine(conv_mode='f16x3') on the released-width (g20) and released-architecture (g25) models against the goldens."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (Cin, Cout, H, W, N): the released decoder's layers at the resolution they run at, g20's, and an odd unaligned one
SHAPES = [(256, 512, 16, 16, 2), (512, 512, 16, 16, 1), (512, 512, 8, 8, 2), (512, 512, 4, 4, 2), (1024, 512, 8, 8, 2),
          (512, 256, 16, 16, 2), (256, 196, 32, 32, 1), (196, 128, 64, 64, 1), (128, 64, 128, 128, 1), (64, 64, 128, 128, 1),
          (64, 96, 16, 16, 2), (72, 132, 7, 9, 2)]


def _problem(cin, cout, H, W, N):
    from latentfusion_amd import ops
    g = torch.Generator().manual_seed(cin * 10 + cout + H)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    b = torch.randn(cout, generator=g) * 0.1
    gin = torch.randn(N, cout, H, W, generator=torch.Generator().manual_seed(1))
    return x, w, b, gin, ops.he_constant(w)


def _fwd_ref(x, w, b, he):
    pre = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1) * he + b.double().view(1, -1, 1, 1)
    act = torch.nn.functional.leaky_relu(pre, 0.2)
    return act / torch.sqrt((act ** 2).mean(dim=1, keepdim=True) + 1e-8)


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item()


def _bar(e32, ref):
    return max(2 * e32, 4e-6 * ref.abs().max().item())


@pytest.mark.parametrize('cin,cout,H,W,N', SHAPES)
def test_f16x3_2d_matches_fp64_within_twice_the_fp32_kernel(cin, cout, H, W, N):
    """Forward (bias + LeakyReLU + PixelNorm) and data gradient: max error <= max(2 x the fp32 kernel's, 4e-6 max|ref|)."""
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    x, w, b, gin, he = _problem(cin, cout, H, W, N)
    xd, wd, bd, gd = ops.cl(x.to(DEV)), w.to(DEV), b.to(DEV), ops.cl(gin.to(DEV))
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM
    want = _fwd_ref(x, w, b, he)
    gwant = torch.nn.functional.conv_transpose2d(gin.double(), w.double(), None, 1, 1) * he
    y32, _ = ops.wide_conv(xd, wd, bd, he, flags)
    g32, _ = ops.wide_conv(gd, wd, None, he, 0, transpose=True)
    y16, n16 = ops.wide_conv_f16x3(xd, wd, bd, he, flags)
    g16, _ = ops.wide_conv_f16x3(gd, wd, None, he, 0, transpose=True)
    torch.cuda.synchronize()
    assert tuple(y16.shape) == (N, cout, H, W) and tuple(g16.shape) == (N, cin, H, W)
    e32, e16 = _err(y32, want), _err(y16, want)
    assert e16 <= _bar(e32, want), (e16, e32)
    ge32, ge16 = _err(g32, gwant), _err(g16, gwant)
    assert ge16 <= _bar(ge32, gwant), (ge16, ge32)
    assert n16 is not None and torch.isfinite(n16).all()


def _single_launch(cin, cout, H, W, N):
    """True when both the forward (Cin -> Cout) and the data gradient (Cout -> Cin) run as ONE GEMM launch whose epilogue writes y
    (no frequency split: lf_wino_fused2d_f16x3_scratch_bytes == 0)."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    return L.lf_wino_fused2d_f16x3_scratch_bytes(N, H, W, cout) == 0 and L.lf_wino_fused2d_f16x3_scratch_bytes(N, H, W, cin) == 0


@pytest.mark.parametrize('cin,cout,H,W,N', [(128, 64, 128, 128, 8), (196, 128, 64, 64, 32)])
def test_f16x3_2d_single_launch_matches_fp64(cin, cout, H, W, N):
    """The direct-write epilogue (per-tile 2^-eV, then bias, LeakyReLU; PixelNorm after) at sizes that need no frequency split --
    the form the routed layers take at cfg 3's batch; 196 -> 128 on 64^2 at N = 32 is itself routed -- forward and data gradient
    against fp64 at the bar of the split form."""
    assert _single_launch(cin, cout, H, W, N)
    test_f16x3_2d_matches_fp64_within_twice_the_fp32_kernel(cin, cout, H, W, N)


@pytest.mark.parametrize('N', [1, 128])
def test_f16x3_2d_scale_is_per_tile(N):
    """Blocks of 8 x 8 pixels whose magnitudes differ by 2^+-30 (one all zero): the outputs of every tile whose 4 x 4 patch lies
    inside one block meet the bar relative to THAT block's magnitude.  A single scale for the whole tensor flushes the 2^-30
    blocks to zero in f16 and fails this.  N = 1: frequency-split GEMM + finish kernel; N = 128: one launch."""
    from latentfusion_amd import ops
    C, S = 64, 32
    assert _single_launch(C, C, S, S, N) == (N == 128)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(N, C, S, S, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g)
    he = ops.he_constant(w)
    exps = [[-30, 0, 30, None], [30, -30, None, 0], [0, None, -30, 30], [None, 30, 0, -30]]
    for i in range(4):
        for j in range(4):
            blk = x[:, :, 8 * i:8 * i + 8, 8 * j:8 * j + 8]
            blk.mul_(0.0 if exps[i][j] is None else 2.0 ** exps[i][j])
    ref = torch.nn.functional.conv2d(x.double(), w.double(), None, 1, 1) * he
    xd, wd = ops.cl(x.to(DEV)), w.to(DEV)
    y16 = ops.wide_conv_f16x3(xd, wd, None, he, 0)[0].double().cpu()
    y32 = ops.wide_conv(xd, wd, None, he, 0)[0].double().cpu()
    for i in range(4):
        for j in range(4):
            # output tiles (by, bx) with rows 2by-1 .. 2by+2 inside the block (or in the zero padding): by = 4i .. 4i+2 minus edges
            rows = [r for by in range(4 * i, 4 * i + 4) if (2 * by - 1 >= 8 * i or by == 0) and (2 * by + 2 <= 8 * i + 7 or by == 15)
                    for r in (2 * by, 2 * by + 1)]
            cols = [c for bx in range(4 * j, 4 * j + 4) if (2 * bx - 1 >= 8 * j or bx == 0) and (2 * bx + 2 <= 8 * j + 7 or bx == 15)
                    for c in (2 * bx, 2 * bx + 1)]
            r_ = ref[:, :, rows][:, :, :, cols]
            e16 = (y16[:, :, rows][:, :, :, cols] - r_).abs().max().item()
            e32 = (y32[:, :, rows][:, :, :, cols] - r_).abs().max().item()
            if exps[i][j] is None:
                assert e16 == 0.0
            else:
                assert r_.abs().max().item() > 0
                assert e16 <= _bar(e32, r_), (i, j, e16, e32, r_.abs().max().item())


@pytest.mark.parametrize('k', [-30, -12, 0, 9])
def test_f16x3_2d_gradient_scale_is_exact(k):
    """gx(g 2^k) == 2^k gx(g) bit for bit, in the frequency-split forms (the first two) and the single-launch form (the last)."""
    from latentfusion_amd import ops
    assert _single_launch(196, 128, 64, 64, 32) and not _single_launch(512, 512, 4, 4, 2)
    for cin, cout, H, W, N in ((256, 512, 16, 16, 8), (512, 512, 4, 4, 2), (196, 128, 64, 64, 32)):
        _x, w, _b, gin, he = _problem(cin, cout, H, W, N)
        wd, gd = w.to(DEV), ops.cl(gin.to(DEV))
        g0, _ = ops.wide_conv_f16x3(gd, wd, None, he, 0, transpose=True)
        gk, _ = ops.wide_conv_f16x3(gd * 2.0 ** k, wd, None, he, 0, transpose=True)
        assert torch.equal(gk, g0 * 2.0 ** k)


def test_f16x3_2d_nonfinite_inputs_stay_nonfinite_where_fp32_does():
    from latentfusion_amd import ops
    from latentfusion_amd._lib import LF_EPI_LRELU
    assert _single_launch(128, 64, 128, 128, 8)
    for cin, cout, H, W, N in ((64, 64, 12, 12, 1), (256, 196, 10, 14, 2), (128, 64, 128, 128, 8)):
        x, w, b, gin, he = _problem(cin, cout, H, W, N)
        x[0, 3, 4, 5] = float('nan')
        x[N - 1, 7, 9, 2] = float('inf')
        x[0, 1, 0, H - 1] = 3e5                                          # finite, beyond f16's range without a scale
        gin[0, 2, 6, 6] = float('-inf')
        xd, wd, bd, gd = ops.cl(x.to(DEV)), w.to(DEV), b.to(DEV), ops.cl(gin.to(DEV))
        y32, _ = ops.wide_conv(xd, wd, bd, he, LF_EPI_LRELU)
        y16, _ = ops.wide_conv_f16x3(xd, wd, bd, he, LF_EPI_LRELU)
        g32, _ = ops.wide_conv(gd, wd, None, he, 0, transpose=True)
        g16, _ = ops.wide_conv_f16x3(gd, wd, None, he, 0, transpose=True)
        m32, m16 = torch.isfinite(y32), torch.isfinite(y16)
        assert not m32.all() and torch.equal(m16, m32)
        assert not torch.isfinite(g32).all() and torch.equal(torch.isfinite(g16), torch.isfinite(g32))


def test_f16x3_2d_run_to_run_identical():
    """The 128-render 128 -> 64 layer on 128^2 (one launch per direction) and a small frequency-split problem, twice."""
    from latentfusion_amd import _lib, ops
    from latentfusion_amd._lib import LF_EPI_LRELU, LF_EPI_PIXELNORM
    L = _lib.lib()
    assert L.lf_wino_fused2d_f16x3_scratch_bytes(2, 4, 4, 512) > 0 and L.lf_wino_fused2d_f16x3_scratch_bytes(128, 128, 128, 64) == 0
    g = torch.Generator(device=DEV).manual_seed(3)
    for cin, cout, S, N in ((128, 64, 128, 128), (512, 512, 4, 2)):
        xd = ops.cl(torch.randn(N, cin, S, S, device=DEV, generator=g))
        gd = ops.cl(torch.randn(N, cout, S, S, device=DEV, generator=g) * 1e-7)
        wd = torch.randn(cout, cin, 3, 3, device=DEV, generator=g)
        bd = torch.randn(cout, device=DEV, generator=g) * 0.1
        he = ops.he_constant(wd)
        outs = []
        for _ in range(2):
            y, _n = ops.wide_conv_f16x3(xd, wd, bd, he, LF_EPI_LRELU | LF_EPI_PIXELNORM)
            gx, _ = ops.wide_conv_f16x3(gd, wd, None, he, 0, transpose=True)
            outs.append((y, gx))
        assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        del xd, gd, outs


def test_f16x3_2d_abi_rejects_bad_arguments():
    """NULL operands, sizes < 1, Cin / Cout not multiples of 4, bad flags, misaligned buffers and short scratch return negative
    codes and write nothing."""
    from latentfusion_amd import _lib, ops
    L = _lib.lib()
    N, S, cin, cout = 1, 4, 64, 64
    x = ops.cl(torch.randn(N, cin, S, S, device=DEV))
    w = torch.randn(cout, cin, 3, 3, device=DEV)
    U2, eU = ops.pack_conv_wino_fused_f16x3(w)
    T = L.lf_wino2d_tiles(N, S, S)
    V = torch.zeros(16, T, L.lf_wino_f16x3_cin_padded(cin) * 2, device=DEV, dtype=torch.float16)
    eV = torch.full((T + 1,), -7, device=DEV, dtype=torch.int32)
    xp, Vp, ep = x.data_ptr(), V.data_ptr(), eV.data_ptr()
    for args in ((None, Vp, ep, N, S, S, cin), (xp, None, ep, N, S, S, cin), (xp, Vp, None, N, S, S, cin), (xp, Vp, ep, 0, S, S, cin),
                 (xp, Vp, ep, N, S, 0, cin), (xp, Vp, ep, N, S, S, 0), (xp, Vp, ep, N, S, S, 62), (xp + 4, Vp, ep, N, S, S, cin),
                 (xp, Vp + 8, ep, N, S, S, cin), (xp, Vp, ep + 2, N, S, S, cin)):
        assert L.lf_wino2d_input_transform_f16x3(*args, None) < 0, args
    torch.cuda.synchronize()
    assert bool((eV == -7).all()) and not V.any()
    assert L.lf_wino2d_input_transform_f16x3(xp, Vp, ep, N, S, S, cin, None) == 0
    y = torch.full((N, S, S, cout), 1234.5, device=DEV)
    nscr = L.lf_wino_fused2d_f16x3_scratch_bytes(N, S, S, cout)
    assert nscr > 0                                                       # a small problem: split over the frequencies
    scr = torch.empty(nscr // 4 + 4, device=DEV)
    torch.cuda.synchronize()

    def call(V_=Vp, e_=ep, U_=U2.data_ptr(), y_=y.data_ptr(), scr_=scr.data_ptr(), nb=nscr, ci=cin, co=cout, flags=1, n=N, eu=eU):
        return L.lf_wino_fused2d_f16x3_gemm(V_, e_, U_, eu, None, y_, scr_, nb, n, S, S, ci, co, 1.0, flags, 0.2, None)
    for kw in (dict(V_=None), dict(e_=None), dict(U_=None), dict(y_=None), dict(ci=62), dict(co=66), dict(ci=0), dict(co=0), dict(n=0),
               dict(flags=2), dict(eu=1000), dict(V_=Vp + 8), dict(U_=U2.data_ptr() + 8), dict(y_=y.data_ptr() + 4), dict(e_=ep + 2),
               dict(scr_=None), dict(nb=nscr - 16), dict(scr_=scr.data_ptr() + 4)):
        assert call(**kw) < 0, kw
    torch.cuda.synchronize()
    assert bool((y == 1234.5).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((y == 1234.5).any())


# ----------------------------------------------------------------------------------------------------------------------
# the scope, the routing and the engine
# ----------------------------------------------------------------------------------------------------------------------
def _rw():
    import test_released_width_gpu as rw
    return rw


def _run_tagged(fn, decoder):
    """Runs fn() with the per-kernel timer on: (result, tags in launch order, decoder conv shapes (Cin, Cout, H, W, N) seen)."""
    from latentfusion_amd import ops
    shapes, hooks = [], []
    for m in decoder.modules():
        w = getattr(getattr(m, 'module', None), 'weight', None)
        if w is not None and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3):
            hooks.append(m.register_forward_hook(lambda mod, inp, out: shapes.append(
                (inp[0].shape[1], out.shape[1], inp[0].shape[2], inp[0].shape[3], inp[0].shape[0]))))
    ops.KERNEL_TIMER = []
    try:
        out = fn()
        torch.cuda.synchronize()
        tags = [str(n) for n, _, _ in ops.KERNEL_TIMER]
    finally:
        ops.KERNEL_TIMER = None
        for h in hooks:
            h.remove()
    return out, tags, shapes


def _check_routing(tags, shapes, grad):
    """Every wide decoder convolution ran exactly once per direction, on f16x3 where ops.WIDE2D_F16X3_ROUTE lists its shape for its
    batch and on the fp32 pair otherwise; returns the number of f16x3 launches."""
    from latentfusion_amd import ops
    wide = [s for s in shapes if s[0] >= 64 and s[1] >= 64]
    calls = [s for s in wide] + ([(co, ci, h, w, n) for ci, co, h, w, n in wide] if grad else [])
    want16 = sum(1 for s in calls if ops._wide2d_f16x3_routed(*s))
    assert tags.count('wino2d_fused_f16x3') == want16, (tags, calls)
    assert tags.count('wino2d_input_f16x3') == want16
    assert tags.count('wino2d_fused') == len(calls) - want16, (tags, calls)
    return want16


def test_g20_engine_routes_the_decoder_to_f16x3(golden):
    """RenderLoopEngine(conv_mode='f16x3') on the released-width model: the routed decoder layers (forward and data gradient)
    on the split-precision kernel, the others (all of them at this width and N = 4, measured slower) on the fp32 pair; loss components, camera gradients and loss order within the bars of the fp32 path; the
    ranking form as well.  conv_mode='winograd' launches no f16x3 kernel."""
    from latentfusion_amd import ops
    from latentfusion_amd.engine import RenderLoopEngine
    rw = _rw()
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = rw._model(g)
    L = g['loss']
    dec = model.photographer.image_decoder
    eng = RenderLoopEngine(model.photographer, g['z_obj'].to(DEV), rw._target(t7), L['weights'], conv_mode='f16x3')
    zc = rw.prod_camera(L['zoomed'])
    (losses, gparams), tags, shapes = _run_tagged(lambda: eng.forward_backward(zc), dec)
    _check_routing(tags, shapes, True)
    for i, k in enumerate(eng.LOSS_KEYS):
        rw.close(losses[:, i], L['components'][k], atol=2e-5, rtol=1e-3)
    rw.close(losses[:, 4], L['total'], atol=2e-5, rtol=1e-3)
    want = torch.cat((L['g_log_q'], L['g_t'], L['g_viewport']), dim=1)
    rel = ((gparams.cpu() - want).norm(dim=1) / want.norm(dim=1)).max().item()
    assert rel < 1e-2, rel
    assert torch.equal(torch.argsort(losses[:, 4].cpu()), torch.argsort(L['total']))
    (lr_, _), tags, shapes = _run_tagged(lambda: eng.forward_backward(zc, need_grad=False), dec)
    _check_routing(tags, shapes, False)
    rw.close(lr_[:, 4], L['total'], atol=2e-5, rtol=1e-3)
    assert not ops.WIDE2D_F16X3
    eng_w = RenderLoopEngine(model.photographer, g['z_obj'].to(DEV), rw._target(t7), L['weights'], conv_mode='winograd')
    for ng in (True, False):
        _, tags, _s = _run_tagged(lambda: eng_w.forward_backward(zc, need_grad=ng), dec)
        assert not any('f16x3' in t for t in tags) and 'wino2d_fused' in tags, tags


def test_scope_ends_with_the_engine_call_even_when_it_raises(golden):
    from latentfusion_amd import ops
    from latentfusion_amd.engine import RenderLoopEngine
    rw = _rw()
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = rw._model(g)
    ph = model.photographer
    L = g['loss']
    eng = RenderLoopEngine(ph, g['z_obj'].to(DEV), rw._target(t7), L['weights'], conv_mode='f16x3')
    zc = rw.prod_camera(L['zoomed'])
    (ci, co, h, w_), n = sorted(ops.WIDE2D_F16X3_ROUTE.items())[0]
    x = ops.cl(torch.randn(n, ci, h, w_, device=DEV))
    w = torch.randn(co, ci, 3, 3, device=DEV)

    def plain_conv_tags():
        _, tags, _s = _run_tagged(lambda: ops.conv3x3(x, w, None), ph.image_decoder)
        return tags
    with ops.wide2d_f16x3():
        assert 'wino2d_fused_f16x3' in plain_conv_tags()
    eng.forward_backward(zc)
    assert not ops.WIDE2D_F16X3 and 'wino2d_fused' in plain_conv_tags() and 'wino2d_fused_f16x3' not in plain_conv_tags()
    seen = []

    def boom(z):
        seen.append(ops.WIDE2D_F16X3)
        raise RuntimeError('decoder failure')
    ph.decode_features = boom
    try:
        with pytest.raises(RuntimeError, match='decoder failure'):
            eng.forward_backward(zc)
    finally:
        del ph.decode_features
    assert seen == [True] and not ops.WIDE2D_F16X3
    tags = plain_conv_tags()
    assert 'wino2d_fused' in tags and 'wino2d_fused_f16x3' not in tags


def test_g20_gradient_estimator_f16x3_decoder(golden):
    from latentfusion_amd import ops
    from latentfusion_amd.pose import estimation
    rw = _rw()
    g, t7 = golden('g20_released_width'), golden('g7_adam_trace')
    model = rw._model(g)
    L = g['loss']
    est = estimation.GradientPoseEstimator(model=model, learning_rate=0.01, num_samples=4, num_iters=2, ranking_size=4,
                                           converge_threshold=1e-6, converge_patience=10, optimizer='adam',
                                           loss_weights=L['weights'], conv_mode='f16x3', track_stats=True)
    (best, stats), tags, shapes = _run_tagged(
        lambda: est.estimate(g['z_obj'].to(DEV), rw._target(t7, 'cpu'), camera=rw.prod_camera(L['init'], 'cpu')),
        model.photographer.image_decoder)
    assert not any(ops._wide2d_f16x3_routed(*s) for s in shapes) and 'wino2d_fused_f16x3' not in tags
    rw.close(stats['rank_loss'][0], L['total'], atol=2e-5, rtol=1e-3)
    assert int(torch.argmin(stats['rank_loss'][0])) == int(torch.argmin(L['total']))
    assert all(torch.isfinite(r).all() for r in stats['rank_loss'])
    assert torch.isfinite(best.log_quaternion).all() and torch.isfinite(best.translation).all()


def test_cfg3_released_architecture_f16x3_decoder(golden):
    """The 68 M-parameter architecture (golden g25): evaluate_samples with conv_mode='f16x3' meets the loss / order bars of the
    fp32 path and routes exactly the layers the table lists for its batch, as does the gradient form; the full
    cross_entropy_linemod preset (N = 128, 2 iterations) routes the >= 196-channel layers and, run twice, is finite and identical."""
    import numpy as np

    from latentfusion_amd import synth
    from latentfusion_amd.engine import RenderLoopEngine
    from latentfusion_amd.pose import estimation
    import test_fullshape_gpu as fs
    g = golden('g25_released_arch')
    seed = g['seed']
    model, _cks = synth.build_released_model(DEV, seed, 0.1)
    dec = model.photographer.image_decoder
    ref = fs._observation(synth.make_observation_data(g['views'], seed + 10))
    target = fs._observation(synth.make_observation_data(1, seed + 20))
    z_obj = model.build_latent_object(ref)
    est = estimation.CrossEntropyPoseEstimator(model=model, num_samples=16, num_elites=6, num_iters=1, num_gmm_components=2,
                                               learning_rate=0.9, sample_flipped=True, ranking_size=4, loss_weights=g['weights'],
                                               conv_mode='f16x3')
    (cams, loss), tags, shapes = _run_tagged(lambda: est.evaluate_samples(z_obj, target, fs.prod_camera(g['cams'])), dec)
    _check_routing(tags, shapes, False)                                  # (4 cameras: below every N_min, all fp32)
    fs.close(loss, g['loss'], atol=2e-5, rtol=1e-3)
    assert fs.same_order_up_to_ties(loss, g['loss'], 2e-5) and int(torch.argmin(loss)) == int(g['order'][0])
    eng = RenderLoopEngine(model.photographer, z_obj, target, g['weights'], conv_mode='f16x3')
    cam = fs.prod_camera(g['cams']).zoom(None, model.input_size, model.camera_dist).to(DEV)
    (_l, gp), tags, shapes = _run_tagged(lambda: eng.forward_backward(cam), dec)
    _check_routing(tags, shapes, True)
    assert torch.isfinite(gp).all()
    cfg = estimation._load_toml(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'configs',
                                             'cross_entropy_linemod.toml'))
    cfg['args']['num_iters'] = 2
    runs = []
    for r in range(2):
        torch.manual_seed(7)
        np.random.seed(7)
        est = estimation.load_from_config(cfg, model, conv_mode='f16x3')
        if r == 0:                                                       # 128 renders per iteration: the routed layers run f16x3
            best, tags, shapes = _run_tagged(lambda: est.estimate(z_obj, target, camera=target.camera), dec)
            assert _check_routing(tags, shapes, False) > 0
        else:
            best = est.estimate(z_obj, target, camera=target.camera)
        runs.append(torch.cat((best.log_quaternion, best.translation), dim=1).cpu())
    assert torch.isfinite(runs[0]).all() and len(runs[0]) == cfg['args']['ranking_size']
    assert torch.equal(runs[0], runs[1])
