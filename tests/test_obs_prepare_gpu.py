"""The fused observation preprocessing on the device: lf_obs_prepare / ops.observation_prepare, Observation.zoom(kernel='fused'),
LatentFusionModel(preprocess_kernel='fused').

1. bit for bit against the composed operations (ops.grid_sample2d + the prepare / normalize expressions of observation.py) on
   the kernel's own lattice, which the test builds in torch from the arithmetic include/lf_hip.h states, one torch op per kernel op;
2. against the real composed path Observation.zoom(kernel='composed').prepare().normalize(), whose lattice is ATen's linspace:
   on boxes whose truncated width and height are coprime to T - 1 the nearest maps are equal at every pixel, colour is held to
   an fp64 restatement within max(4 * e32, 2e-6 + 2e-5 * |fp64|), e32 = the composed device path's own distance from fp64;
3. misreadings of the chain are told apart by those comparisons; 4. properties; 5. ABI errors; 6. plumbing.
Measured on an MI355X (test 2, white-noise colour, frames 97x131 and 480x640, T in 2..128): see COVERAGE.md row a15."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
LF_EINVAL, LF_EALIGN = -1, -2


# ---------------------------------------------------------------------------------------------
# the header's lattice in torch: every line is one kernel operation (divisors are device tensors: ATen turns a division by a
# Python number into a multiplication by its reciprocal)
# ---------------------------------------------------------------------------------------------
def kernel_grid(boxes, H, W, T, corners='trunc'):
    B, dev = boxes.shape[0], boxes.device
    c = boxes.trunc() if corners == 'trunc' else boxes.round()

    def axis(c0, c1, size):
        size64 = torch.tensor(float(size), dtype=torch.float64, device=dev)
        start = (c0.double() / size64).float()
        end = (c1.double() / size64).float()
        if T == 1:
            lat = start[:, None]
        else:
            step = (end - start) / torch.tensor(float(T - 1), device=dev)
            i = torch.arange(T, device=dev)
            lo = start[:, None] + step[:, None] * i.float()[None]
            hi = end[:, None] - step[:, None] * (T - 1 - i).float()[None]
            lat = torch.where((i < T // 2)[None], lo, hi)
        return lat * 2 - 1
    gx, gy = axis(c[:, 0], c[:, 2], W), axis(c[:, 1], c[:, 3], H)
    return torch.stack((gx[:, None, :].expand(B, T, T), gy[:, :, None].expand(B, T, T)), dim=-1).contiguous()


def chain(color, depth, mask, zn, zf, prepare, normalize, clamp=True):
    """The prepare / normalize expressions of observation.py and Camera.normalize_depth on cropped maps."""
    from latentfusion_amd.observation import gan_denormalize, gan_normalize
    if prepare:
        if color is not None:
            color = gan_denormalize(gan_normalize(color) * mask) if clamp else (gan_normalize(color) * mask + 1.0) / 2.0
        depth = depth * mask
    if normalize:
        color = gan_normalize(color) if color is not None else None
        depth = ((depth - zn.view(-1, 1, 1, 1)) / (zf - zn).view(-1, 1, 1, 1)).clamp(0, 1) * 2.0 - 1.0
    return color, depth, mask


def composed_on_grid(color, depth, mask, grid, zn, zf, prepare, normalize):
    from latentfusion_amd import ops
    c = ops.grid_sample2d(color, grid, 'bilinear', 'zeros') if color is not None and color.shape[1] > 0 else None
    d = ops.grid_sample2d(depth, grid, 'nearest', 'zeros')
    m = ops.grid_sample2d(mask.float(), grid, 'nearest', 'zeros')
    return chain(c, d, m, zn, zf, prepare, normalize)


def stacked(c, d, m, with_depth):
    from latentfusion_amd.observation import gan_normalize
    return torch.cat(([c] if c is not None else []) + ([d] if with_depth else []) + [gan_normalize(m)], dim=1)


def same(a, b):
    """torch.equal that takes a NaN as equal to a NaN."""
    if a is None or b is None:
        return a is None and (b is None or b.numel() == 0)
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.where(a.isnan(), 7.0, a),
                                                                                     torch.where(b.isnan(), 7.0, b))


BOX_KINDS = ('inside', 'left', 'top', 'right', 'bottom', 'outside', 'outside_neg', 'zero_width', 'inverted', 'fractional', 'full')


def box_of(kind, H, W):
    return {'inside': (0.21 * W, 0.17 * H, 0.83 * W, 0.79 * H), 'left': (-0.31 * W, 0.1 * H, 0.52 * W, 0.93 * H),
            'top': (0.12 * W, -0.43 * H, 0.9 * W, 0.6 * H), 'right': (0.5 * W, 0.2 * H, 1.37 * W, 0.8 * H),
            'bottom': (0.1 * W, 0.45 * H, 0.77 * W, 1.6 * H), 'outside': (1.5 * W, 1.6 * H, 2.5 * W, 2.7 * H),
            'outside_neg': (-2.2 * W, -1.9 * H, -1.2 * W, -1.1 * H), 'zero_width': (int(0.5 * W) + 0.1, 0.2 * H, int(0.5 * W) + 0.8, 0.8 * H),
            'inverted': (0.81 * W, 0.9 * H, 0.13 * W, 0.22 * H), 'fractional': (-0.7, -1.5, W - 0.5, H + 0.6),
            'full': (0.0, 0.0, float(W), float(H))}[kind]


_FRAMES = {}


def frames(H, W):
    """7 frames of 4 colour planes, depth and a mask with holes at H x W, made once (white noise: every tap matters)."""
    if (H, W) not in _FRAMES:
        g = torch.Generator().manual_seed(H * 1000 + W)
        color = torch.rand(7, 4, H, W, generator=g)
        depth = torch.rand(7, 1, H, W, generator=g) * 0.4 + 0.8
        mask = (torch.rand(7, 1, H, W, generator=g) > 0.3).float()
        zn = 0.75 + 0.1 * torch.rand(7, generator=g)
        _FRAMES[(H, W)] = tuple(t.to(DEV) for t in (color, depth, mask, zn, zn + 0.5))
    return _FRAMES[(H, W)]


def inputs(H, W, B, C, mask_dtype, kinds):
    color, depth, mask, zn, zf = frames(H, W)
    boxes = torch.tensor([box_of(kinds[b % len(kinds)], H, W) for b in range(B)], dtype=torch.float32, device=DEV)
    mk = mask[:B]
    if mask_dtype is torch.uint8:
        mk = (mk * 3).to(torch.uint8)                                           # bytes count as their value
    elif mask_dtype is torch.bool:
        mk = mk.bool()
    return (color[:B, :C].contiguous() if C > 0 else None), depth[:B], mk, boxes, zn[:B].contiguous(), zf[:B].contiguous()


def check_case(H, W, T, B, C, mask_dtype, prepare, normalize, stack, kinds):
    from latentfusion_amd import ops
    color, depth, mask, boxes, zn, zf = inputs(H, W, B, C, mask_dtype, kinds)
    out = ops.observation_prepare(color, depth, mask, boxes, T, zn=zn if normalize else None, zf=zf if normalize else None,
                                  prepare=prepare, normalize=normalize, stack=stack)
    grid = kernel_grid(boxes, H, W, T)
    c, d, m = composed_on_grid(color, depth, mask, grid, zn, zf, prepare, normalize)
    tag = (H, W, T, B, C, mask_dtype, prepare, normalize, stack)
    assert (out['color'] is None) == (C == 0), tag
    if C > 0:
        assert torch.equal(out['color'], c), ('color', tag, float((out['color'] - c).abs().max()))
    assert torch.equal(out['depth'], d), ('depth', tag)
    assert torch.equal(out['mask'], m), ('mask', tag)
    if stack is not None:
        assert torch.equal(out['stack'], stacked(c, d, m, stack == 'color_depth_mask')), ('stack', tag)
    else:
        assert 'stack' not in out


STAGES = ((False, False), (True, False), (False, True), (True, True))
SHAPES = [(5, 7), (33, 65), (97, 131), (480, 640)]
SIZES = [1, 2, 3, 16, 17, 128]


# ---------------------------------------------------------------------------------------------
# 1. bit for bit against the composed operations on the kernel's own lattice
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', SIZES)
@pytest.mark.parametrize('shape', SHAPES)
def test_bit_equal_to_the_composed_operations_on_the_kernels_lattice(shape, T):
    """Every stage combination per (frame, T); B in {1, 3, 7}, C in {0, 1, 3, 4}, the three mask types, the stacked forms and
    the box kinds rotate through the cases so that each value meets each frame size and each T."""
    H, W = shape
    k = SHAPES.index(shape) * len(SIZES) + SIZES.index(T)
    for s, (prepare, normalize) in enumerate(STAGES):
        j = k + s
        kinds = BOX_KINDS[j % len(BOX_KINDS):] + BOX_KINDS[:j % len(BOX_KINDS)]
        check_case(H, W, T, (1, 3, 7)[j % 3], (0, 1, 3, 4)[(j + j // 3) % 4], (torch.float32, torch.bool, torch.uint8)[(j + j // 4) % 3],
                   prepare, normalize, (None, 'color_mask', 'color_depth_mask')[(j + j // 5) % 3], kinds)


@pytest.mark.parametrize('mask_dtype', [torch.float32, torch.bool, torch.uint8])
@pytest.mark.parametrize('C', [0, 1, 3, 4])
def test_every_box_kind_channel_count_and_mask_type(C, mask_dtype):
    """All box kinds in one batch (7 frames at a time), each B, every stage and stacked form, at two frame sizes."""
    for H, W, T in ((33, 65, 17), (97, 131, 16)):
        for start in (0, 4):
            for s, (prepare, normalize) in enumerate(STAGES):
                for stack in (None, 'color_mask', 'color_depth_mask'):
                    check_case(H, W, T, (7, 3, 1, 7)[s], C, mask_dtype, prepare, normalize, stack, BOX_KINDS[start:start + 7])


def test_box_kinds_are_what_they_say():
    """The cases above hold what the issue lists: truncation toward zero on both signs, zero width, inverted, outside."""
    H, W = 33, 65
    t = {k: [math.trunc(v) for v in box_of(k, H, W)] for k in BOX_KINDS}
    assert t['fractional'] == [0, -1, W - 1, H] and box_of('fractional', H, W)[0] < 0             # -0.7 -> -0, -1.5 -> -1 (not -2)
    assert t['zero_width'][0] == t['zero_width'][2] and t['inverted'][0] > t['inverted'][2] and t['inverted'][1] > t['inverted'][3]
    assert t['outside'][0] >= W and t['outside'][1] >= H and t['outside_neg'][2] < 0 and t['outside_neg'][3] < 0
    assert t['left'][0] < 0 and t['top'][1] < 0 and t['right'][2] > W and t['bottom'][3] > H
    assert 0 < t['inside'][0] < t['inside'][2] < W and 0 < t['inside'][1] < t['inside'][3] < H
    grid = kernel_grid(torch.tensor([box_of('inside', H, W)], device=DEV), H, W, 17)
    x0, y0, x1, y1 = t['inside']
    assert float(grid[0, 0, 0, 0]) == float(torch.tensor(x0 / W, dtype=torch.float32) * 2 - 1)  # point 0 is exactly start
    assert float(grid[0, -1, -1, 1]) == float(torch.tensor(y1 / H, dtype=torch.float32) * 2 - 1)  # point T - 1 exactly end


# ---------------------------------------------------------------------------------------------
# 2. against the real composed path
# ---------------------------------------------------------------------------------------------
WIDTHS = (23, 37, 41)             # odd, no multiple of 3, 5 or 127: coprime to T - 1 for every T below


def coprime_observation(H, W, T, dist=2.0):
    """3 frames whose zoom boxes have the truncated widths / heights WIDTHS (scaled up on the large frame), from cameras
    built for it: box side = dist * T / z, centred on the projected origin."""
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    color, depth, mask, _, _ = frames(H, W)
    scale = 1 if W < 200 else 7                                                  # 161, 259, 287 = 7 * WIDTHS: still coprime
    side = torch.tensor([float(w * scale) for w in WIDTHS])
    f = 100.0
    z = dist * T / side
    x0 = torch.tensor([0.3 * W, 0.1 * W, 0.55 * W]).floor() + 0.3                # the right / bottom edges may overhang
    y0 = torch.tensor([0.2 * H, 0.5 * H, 0.05 * H]).floor() + 0.4
    cu, cv = x0 + side / 2, y0 + side / 2
    K = torch.tensor([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]).expand(3, -1, -1).clone()
    E = torch.eye(4).expand(3, -1, -1).clone()
    E[:, 0, 3], E[:, 1, 3], E[:, 2, 3] = (cu - W / 2.0) / f * z, (cv - H / 2.0) / f * z, z
    cam = Camera(K, E, width=W, height=H)
    dep = z.view(3, 1, 1, 1).to(DEV) + (depth[:3] - 1.0) * 2.0                   # inside z -+ z_span (0.5)
    return Observation(color[:3, :3].clone(), dep, mask[:3].clone(), cam).to(DEV), dist


def assert_coprime(boxes, T):
    t = boxes.double().trunc().tolist()
    for x0, y0, x1, y1 in t:
        w, h = int(x1 - x0), int(y1 - y0)
        assert T == 1 or (math.gcd(abs(w), T - 1) == 1 and math.gcd(abs(h), T - 1) == 1), (w, h, T)


def fp64_chain(obs, boxes, T, mask):
    """zoom -> prepare -> normalize of the colour restated in fp64 on the host (exact corners, fp64 lattice, taps and chain).
    mask: the cropped mask of the composed path, exact values that the nearest comparison holds equal on both paths (an fp64
    lattice would put the first and last lattice lines on exact rounding ties, where the fp32 lattices are not)."""
    H, W = obs.color.shape[-2:]
    c = boxes.double().trunc().cpu()
    grids = []
    for x0, y0, x1, y1 in c.tolist():
        gy = torch.linspace(y0 / H, y1 / H, T, dtype=torch.float64) * 2 - 1
        gx = torch.linspace(x0 / W, x1 / W, T, dtype=torch.float64) * 2 - 1
        grids.append(torch.stack((gx[None, :].expand(T, -1), gy[:, None].expand(-1, T)), dim=-1))
    grid = torch.stack(grids)
    col = F.grid_sample(obs.color.double().cpu(), grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    m = mask.double().cpu()
    col = (((col * 2 - 1) * m + 1) / 2).clamp(0, 1)
    return col * 2 - 1


def colour_errors(fused, composed, ref64):
    e32 = float((composed.double().cpu() - ref64).abs().max())
    err = (fused.double().cpu() - ref64).abs()
    bound = torch.maximum(torch.full_like(ref64, 4 * e32), 2e-6 + 2e-5 * ref64.abs())
    return e32, float(err.max()), bool((err <= bound).all())


@pytest.mark.parametrize('T', [1, 2, 3, 16, 17, 128])
@pytest.mark.parametrize('shape', [(97, 131), (480, 640)])
def test_against_the_composed_path(shape, T):
    H, W = shape
    obs, dist = coprime_observation(H, W, T)
    boxes = obs.camera.zoom_viewport(T, dist)
    assert_coprime(boxes, T)                                                     # the condition under which no pixel is excluded
    ref = obs.zoom(dist, T, kernel='composed').prepare().normalize()
    got = obs.zoom(dist, T, kernel='fused').prepare().normalize()                # the crop fused, the chains composed
    from latentfusion_amd.observation import fused_preprocess
    one, x = fused_preprocess(obs, dist, T, prepare=True, normalize=True, stack='color_depth_mask')     # everything fused
    assert all(one.meta[k] for k in ('is_zoomed', 'is_prepared', 'is_normalized'))
    assert got.meta == ref.meta == one.meta
    assert float(ref.mask.mean()) > 0.05 and float((ref.depth > -1).float().mean()) > 0.05            # the crop sees the object
    for o in (got, one):
        assert torch.equal(o.depth, ref.depth) and torch.equal(o.mask, ref.mask)
        assert torch.equal(o.camera.viewport, ref.camera.viewport) and torch.equal(o.camera.translation, ref.camera.translation)
    assert torch.equal(one.color, got.color)
    assert torch.equal(x[:, 3:4], ref.depth) and torch.equal(x[:, 4:5], ref.mask * 2.0 - 1.0) and torch.equal(x[:, :3], one.color)
    e32, err, ok = colour_errors(one.color, ref.color, fp64_chain(obs, boxes, T, ref.mask))
    print(f'obs_prepare colour {H}x{W} T={T}: composed-fp64 e32={e32:.3e} fused-fp64={err:.3e} '
          f'fused-composed={float((one.color - ref.color).abs().max()):.3e}')
    assert ok, (e32, err)


# ---------------------------------------------------------------------------------------------
# 3. misreadings: each one is told apart by the comparisons of 1 and 2 on these inputs
# ---------------------------------------------------------------------------------------------
def test_misreadings_are_told_apart():
    from latentfusion_amd import ops
    H, W, T, B = 33, 65, 17, 7
    kinds = ('fractional', 'left', 'inside', 'right', 'top', 'bottom', 'full')
    color, depth, mask, boxes, zn, zf = inputs(H, W, B, 3, torch.float32, kinds)
    boxes = boxes + torch.tensor([0.0, 0.0, 0.3, 0.3], device=DEV)              # corners with fractions above one half among them
    out = ops.observation_prepare(color, depth, mask, boxes, T, zn=zn, zf=zf, prepare=True, normalize=True)
    grid = kernel_grid(boxes, H, W, T)
    c, d, m = composed_on_grid(color, depth, mask, grid, zn, zf, True, True)
    assert torch.equal(out['color'], c) and torch.equal(out['depth'], d) and torch.equal(out['mask'], m)

    def sample(img, g, mode, padding='zeros', align=False):
        return F.grid_sample(img, g, mode=mode, padding_mode=padding, align_corners=align)

    def variant(g=grid, cmode='bilinear', dmode='nearest', padding='zeros', align=False, mask_first=False, clamp=True, eps=0.01):
        col, dep = color, depth
        if mask_first:
            from latentfusion_amd.observation import gan_denormalize, gan_normalize
            col, dep = gan_denormalize(gan_normalize(color) * mask), depth * mask
        cc, dd, mm = sample(col, g, cmode, padding, align), sample(dep, g, dmode, padding, align), sample(mask, g, 'nearest', padding, align)
        zn_, zf_ = zn + 0.01 - eps, zf - 0.01 + eps
        return chain(cc, dd, mm, zn_, zf_, not mask_first, True, clamp=clamp)
    # the variant with nothing changed is the chain itself (ATen's sampler against the HIP one: equal up to rounding)
    base = variant()
    assert float((base[1] != d).float().mean()) < 0.01 and float((base[2] != m).float().mean()) < 0.01
    assert float((base[0] - c).abs().max()) < 1e-4
    wrong = {'corners rounded': variant(g=kernel_grid(boxes, H, W, T, corners='round')), 'align_corners=True': variant(align=True),
             'border padding': variant(padding='border'), 'depth bilinear': variant(dmode='bilinear'),
             'mask before the crop': variant(mask_first=True), 'zn / zf without the 0.01': variant(eps=0.0)}
    for name, (wc, wd, wm) in wrong.items():
        gap = max(float((wc - c).abs().max()), float((wd - d).abs().max()), float((wm - m).abs().max()))
        print(f'misreading {name}: max difference {gap:.3e}')
        assert gap > 1e-3, name
    # the clamp of gan_denormalize matters only where colour leaves [0, 1]: an over-range frame tells its absence apart
    hot = color * 3 - 1
    o2 = ops.observation_prepare(hot, depth, mask, boxes, T, prepare=True)
    c2, _, _ = composed_on_grid(hot, depth, mask, grid, zn, zf, True, False)
    assert torch.equal(o2['color'], c2) and float(c2.max()) == 1.0 and float(c2.min()) == 0.0
    loose, _, _ = chain(ops.grid_sample2d(hot, grid, 'bilinear', 'zeros'), d, m, zn, zf, True, False, clamp=False)
    gap = float((loose - c2).abs().max())
    print(f'misreading no clamp in gan_denormalize: max difference {gap:.3e}')
    assert gap > 1e-3


# ---------------------------------------------------------------------------------------------
# 4. properties
# ---------------------------------------------------------------------------------------------
def test_frame_alone_equals_frame_in_batch_and_runs_repeat():
    from latentfusion_amd import ops
    H, W, T, B = 97, 131, 17, 7
    color, depth, mask, boxes, zn, zf = inputs(H, W, B, 3, torch.bool, BOX_KINDS)
    kw = dict(prepare=True, normalize=True, stack='color_depth_mask')
    full = ops.observation_prepare(color, depth, mask, boxes, T, zn=zn, zf=zf, **kw)
    again = ops.observation_prepare(color, depth, mask, boxes, T, zn=zn, zf=zf, **kw)
    for k in full:
        assert torch.equal(full[k], again[k]), k
    for b in range(B):
        s = slice(b, b + 1)
        one = ops.observation_prepare(color[s], depth[s], mask[s], boxes[s], T, zn=zn[s], zf=zf[s], **kw)
        for k in full:
            assert torch.equal(one[k], full[k][s]), (k, b)


def test_non_finite_boxes_and_depths():
    """NaN / +-inf boxes (a degenerate initial pose yields them) and NaN / inf depths: no fault, the composed operations' values."""
    from latentfusion_amd import ops
    H, W, T = 33, 65, 16
    nan, inf = float('nan'), float('inf')
    rows = [(nan, nan, nan, nan), (inf, 2.0, 40.0, 30.0), (3.0, -inf, 40.0, 30.0), (3.0, 2.0, inf, 30.0), (3.0, 2.0, 40.0, -inf),
            (-inf, -inf, inf, inf), (nan, 2.0, 40.0, 30.0), (3.0, 2.0, 40.0, nan), (3.0, 2.0, 40.0, 30.0), (1e30, 2.0, 3e38, 30.0)]
    for start in (0, 5):
        B = 5
        color, depth, mask, _, zn, zf = inputs(H, W, B, 3, torch.float32, BOX_KINDS)
        depth = depth.clone()
        depth[:, :, ::3, ::4] = nan
        depth[:, :, 1::5, 1::3] = inf
        depth[:, :, 2::7, ::5] = -inf
        boxes = torch.tensor(rows[start:start + B], dtype=torch.float32, device=DEV)
        for prepare, normalize in STAGES:
            out = ops.observation_prepare(color, depth, mask, boxes, T, zn=zn, zf=zf, prepare=prepare, normalize=normalize,
                                          stack='color_depth_mask')
            torch.cuda.synchronize()
            c, d, m = composed_on_grid(color, depth, mask, kernel_grid(boxes, H, W, T), zn, zf, prepare, normalize)
            assert same(out['color'], c) and same(out['depth'], d) and same(out['mask'], m), (start, prepare, normalize)
            assert same(out['stack'], stacked(c, d, m, True))
    # a NaN zn / zf row stays that row's own
    zn2 = zn.clone()
    zn2[1] = nan
    boxes = torch.tensor([box_of('inside', H, W)] * 5, dtype=torch.float32, device=DEV)
    out = ops.observation_prepare(color, depth, mask, boxes, T, zn=zn2, zf=zf, normalize=True)
    c, d, m = composed_on_grid(color, depth, mask, kernel_grid(boxes, H, W, T), zn2, zf, False, True)
    assert same(out['depth'], d) and bool(out['depth'][1].isnan().all()) and not bool(out['depth'][0].isnan().all())


def _raw(lib, color, depth, mask, u8, boxes, zn, zf, co, do, mo, stack, stride, sd, B, C, H, W, T, stages):
    def p(t):
        return t.data_ptr() if isinstance(t, torch.Tensor) else t
    return lib.lf_obs_prepare(p(color), p(depth), p(mask), u8, p(boxes), p(zn), p(zf), p(co), p(do), p(mo), p(stack), stride, sd,
                              B, C, H, W, T, stages, torch.cuda.current_stream().cuda_stream)


def test_sentinels_and_the_planes_not_asked_for():
    """Nothing is written behind an output, nor into floats of a stacked row beyond the planes asked for."""
    from latentfusion_amd import _lib
    L = _lib.lib()
    H, W, T, B, C = 33, 65, 17, 3, 3
    color, depth, mask, boxes, zn, zf = inputs(H, W, B, C, torch.float32, BOX_KINDS)
    TT, pad, S = T * T, 1000, -12345.0
    for sd in (0, 1):
        planes = C + 1 + sd
        stride = (C + 3) * TT + 5                                               # a row longer than the planes written
        co, do, mo = (torch.full((n * TT + pad,), S, device=DEV) for n in (B * C, B, B))
        st = torch.full((B * stride + pad,), S, device=DEV)
        assert _raw(L, color, depth, mask, 0, boxes, zn, zf, co, do, mo, st, stride, sd, B, C, H, W, T, 3) == 0
        torch.cuda.synchronize()
        c, d, m = composed_on_grid(color, depth, mask, kernel_grid(boxes, H, W, T), zn, zf, True, True)
        assert torch.equal(co[:B * C * TT].view(B, C, T, T), c) and torch.equal(do[:B * TT].view(B, 1, T, T), d)
        assert torch.equal(mo[:B * TT].view(B, 1, T, T), m)
        for buf, n in ((co, B * C), (do, B), (mo, B)):
            assert bool((buf[n * TT:] == S).all())
        rows = st[:B * stride].view(B, stride)
        assert torch.equal(rows[:, :planes * TT].reshape(B, planes, T, T), stacked(c, d, m, sd == 1))
        assert bool((rows[:, planes * TT:] == S).all()) and bool((st[B * stride:] == S).all())
    # C = 0: no colour plane is touched, the stacked row is [depth | mask]
    do, mo, st = (torch.full((n * TT + pad,), S, device=DEV) for n in (B, B, 2 * B))
    assert _raw(L, None, depth, mask, 0, boxes, zn, zf, None, do, mo, st, 2 * TT, 1, B, 0, H, W, T, 1) == 0
    torch.cuda.synchronize()
    _, d, m = composed_on_grid(None, depth, mask, kernel_grid(boxes, H, W, T), zn, zf, True, False)
    assert torch.equal(st[:2 * B * TT].view(B, 2, T, T), stacked(None, d, m, True)) and bool((st[2 * B * TT:] == S).all())
    assert bool((do[B * TT:] == S).all()) and bool((mo[B * TT:] == S).all())


def test_poison_outside_the_box_is_never_seen():
    """Each frame is read only where its box lies: NaN everywhere but the box (and the one-pixel rim the bilinear taps reach)."""
    from latentfusion_amd import ops
    H, W, T = 97, 131, 16
    color, depth, mask, _, zn, zf = inputs(H, W, 3, 3, torch.float32, BOX_KINDS)
    corners = [(20, 11, 90, 70), (1, 1, 130, 96), (64, 40, 66, 90)]
    boxes = torch.tensor(corners, dtype=torch.float32, device=DEV) + 0.4
    color, depth, mask = color.clone(), depth.clone(), mask.clone()
    for b, (x0, y0, x1, y1) in enumerate(corners):
        keep = torch.zeros(H, W, dtype=torch.bool, device=DEV)
        keep[max(y0 - 1, 0):y1 + 1, max(x0 - 1, 0):x1 + 1] = True
        for t in (color, depth, mask):
            t[b, :, ~keep] = float('nan')
    assert bool(color.isnan().any()) and bool(depth.isnan().any()) and bool(mask.isnan().any())
    for prepare, normalize in STAGES:
        out = ops.observation_prepare(color, depth, mask, boxes, T, zn=zn, zf=zf, prepare=prepare, normalize=normalize,
                                      stack='color_depth_mask')
        for k, v in out.items():
            assert not bool(v.isnan().any()), (k, prepare, normalize)


# ---------------------------------------------------------------------------------------------
# 5. ABI: every rejected argument returns its code with the outputs intact
# ---------------------------------------------------------------------------------------------
def test_abi_rejections_leave_the_outputs_intact():
    from latentfusion_amd import _lib
    L = _lib.lib()
    H, W, T, B, C = 5, 7, 3, 2, 3
    color, depth, mask, boxes, zn, zf = inputs(H, W, B, C, torch.float32, BOX_KINDS)
    S = -7.0
    co, do, mo, st = (torch.full((n * T * T + 4,), S, device=DEV) for n in (B * C, B, B, B * (C + 2)))
    good = dict(color=color, depth=depth, mask=mask, u8=0, boxes=boxes, zn=zn, zf=zf, co=co, do=do, mo=mo, stack=st,
                stride=(C + 2) * T * T, sd=1, B=B, C=C, H=H, W=W, T=T, stages=3)
    einval = [dict(depth=None), dict(mask=None), dict(boxes=None), dict(do=None), dict(mo=None), dict(color=None), dict(co=None),
              dict(B=0), dict(H=0), dict(W=-1), dict(T=0), dict(C=-1), dict(u8=2), dict(u8=-1), dict(stages=4), dict(stages=7),
              dict(stages=-1), dict(zn=None), dict(zf=None), dict(stages=2, zn=None), dict(sd=2), dict(sd=-1),
              dict(stride=(C + 2) * T * T - 1), dict(stride=0), dict(stride=-5),
              dict(B=1 << 20, H=1 << 6, W=1 << 5), dict(B=1 << 27, C=0, stack=None, T=2), dict(H=1 << 16, W=1 << 16),
              dict(T=1 << 16), dict(B=1 << 30, C=4)]
    ealign = [dict(color=color.data_ptr() + 2), dict(depth=depth.data_ptr() + 1), dict(mask=mask.data_ptr() + 2),
              dict(mask=mask.data_ptr() + 1, u8=1), dict(boxes=boxes.data_ptr() + 2), dict(zn=zn.data_ptr() + 2),
              dict(zf=zf.data_ptr() + 1), dict(co=co.data_ptr() + 2), dict(do=do.data_ptr() + 2), dict(mo=mo.data_ptr() + 3),
              dict(stack=st.data_ptr() + 2)]
    for code, cases in ((LF_EINVAL, einval), (LF_EALIGN, ealign)):
        for over in cases:
            assert _raw(L, *dict(good, **over).values()) == code, over
    torch.cuda.synchronize()
    assert all(bool((t == S).all()) for t in (co, do, mo, st))
    with pytest.raises(_lib.LFHipError):
        _lib.check(LF_EINVAL, 'lf_obs_prepare')
    assert _raw(L, *good.values()) == 0                                          # and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert not bool((co[:B * C * T * T] == S).any())


# ---------------------------------------------------------------------------------------------
# 6. plumbing
# ---------------------------------------------------------------------------------------------
def _tags(fn):
    from latentfusion_amd import ops
    ops.KERNEL_TIMER = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [str(name) for name, _, _ in ops.KERNEL_TIMER]
    finally:
        ops.KERNEL_TIMER = None


def _trace(fn):
    """(result, names of the device kernels, the device-to-host copies) of fn under the profiler."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    from torch.autograd import DeviceType
    events = list(prof.events())
    kernels = [e.name for e in events if e.device_type == DeviceType.CUDA]
    # (device events only: an .item() or .cpu() of a device tensor shows as one; aten::item alone may be a host tensor's)
    d2h = [n for n in kernels if 'dtoh' in n.lower().replace(' ', '').replace('_', '') or 'devicetohost' in n.lower().replace(' ', '')]
    return out, kernels, d2h


@pytest.fixture(scope='module')
def model():
    from latentfusion_amd import synth
    m, _ = synth.build_model(32, 16, 'pool:mean', seed=4, device=DEV, bias_std=0.05)
    return m


def test_preprocess_observation_is_one_launch_without_a_host_copy(model, monkeypatch):
    from latentfusion_amd import synth
    obs = synth.make_observation(3, 11, DEV)
    T, dist = model.input_size, model.camera_dist
    boxes = obs.camera.zoom_viewport(T, dist)
    assert_coprime(boxes, T)                                                     # 743 wide and high against T - 1 = 31: no tie line
    assert model.preprocess_kernel == 'composed'
    ref, ref_tags = _tags(lambda: model.preprocess_observation(obs))
    assert 'obs_prepare' not in ref_tags
    steps = obs.zoom(dist, T).prepare().normalize()                              # 'composed' is the parent's three steps, untouched
    assert all(torch.equal(getattr(ref, k), getattr(steps, k)) for k in ('color', 'depth', 'mask'))
    _, _, copies = _trace(lambda: model.preprocess_observation(obs))
    assert len(copies) >= 3                                                       # the detector sees the composed path's .cpu() calls
    monkeypatch.setattr(model, 'preprocess_kernel', 'fused')
    model.preprocess_observation(obs)                                            # (warm)
    got, tags = _tags(lambda: model.preprocess_observation(obs))
    assert tags.count('obs_prepare') == 1 and not [t for t in tags if 'grid_sample' in t]
    got, names, copies = _trace(lambda: model.preprocess_observation(obs))
    assert len([n for n in names if 'obs_prepare_kernel' in n]) == 1, [n for n in names if 'kernel' in n.lower()][:20]
    assert not copies, copies
    assert all(got.meta[k] for k in ('is_zoomed', 'is_prepared', 'is_normalized')) and got.meta == ref.meta
    assert torch.equal(got.depth, ref.depth) and torch.equal(got.mask, ref.mask)
    assert torch.equal(got.camera.viewport, ref.camera.viewport)
    e32, err, ok = colour_errors(got.color, ref.color, fp64_chain(obs, boxes, T, ref.mask))
    print(f'preprocess_observation colour: composed-fp64 e32={e32:.3e} fused-fp64={err:.3e}')
    assert ok, (e32, err)
    # any flag already set: the composed steps, whatever the option says
    z = obs.zoom(dist, T)
    a, tags = _tags(lambda: model.preprocess_observation(z))
    assert 'obs_prepare' not in tags and torch.equal(a.color, ref.color) and torch.equal(a.depth, ref.depth)
    # Observation.zoom on its own, and the module switch
    from latentfusion_amd import observation as obsmod
    zf_, names, copies = _trace(lambda: obs.zoom(dist, T, kernel='fused'))
    assert not copies and zf_.meta['is_zoomed'] and not zf_.meta['is_prepared'] and not zf_.meta['is_normalized']
    assert torch.equal(zf_.depth, z.depth) and torch.equal(zf_.mask, z.mask)
    monkeypatch.setattr(obsmod, 'KERNEL', 'fused')
    assert torch.equal(obs.zoom(dist, T).color, zf_.color)
    with pytest.raises(ValueError, match='device tensors'):
        obs.to('cpu').zoom(dist, T)


def test_zoom_estimate_fused_chain(model):
    from latentfusion_amd import synth
    obs = synth.make_observation(2, 12, DEV)
    T, dist = model.input_size, model.camera_dist
    ref = obs.zoom_estimate(dist, T)
    got, names, copies = _trace(lambda: obs.zoom_estimate(dist, T, kernel='fused', zoom_kernel='fused'))
    assert len([n for n in names if 'obs_prepare_kernel' in n]) == 1
    print(f'zoom_estimate fused + fused: {len(copies)} device-to-host copies (the count check of the initial pose)')
    assert len(copies) <= 1, copies
    assert torch.equal(got.camera.viewport, ref.camera.viewport)                 # the initial pose is bit-equal, so are the boxes
    assert_coprime(ref.camera.viewport, T)
    assert torch.equal(got.depth, ref.depth) and torch.equal(got.mask, ref.mask)
    assert float((got.color - ref.color).abs().max()) < 1e-3


def test_build_latent_object_and_the_other_callers(model, monkeypatch):
    from latentfusion_amd import synth
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    obs = synth.make_observation(4, 13, DEV)
    T, dist = model.input_size, model.camera_dist
    boxes = obs.camera.zoom_viewport(T, dist)
    with torch.no_grad():
        z_ref, ref_tags = _tags(lambda: model.build_latent_object(obs))
        pre = model.preprocess_observation(obs)
        # the composed path's own distance: the same encoder fed the fp64-preprocessed colour (rounded once to fp32)
        exact = Observation(fp64_chain(obs, boxes, T, pre.mask).float().to(DEV), pre.depth, pre.mask, pre.camera, **pre.meta)
        z_exact = model.build_latent_object(exact)
        monkeypatch.setattr(model, 'preprocess_kernel', 'fused')
        z_fused, tags = _tags(lambda: model.build_latent_object(obs))
        assert 'obs_prepare' not in ref_tags and tags.count('obs_prepare') == 1
        assert [t for t in tags if t != 'obs_prepare'] == [t for t in ref_tags if 'grid_sample' not in t]

        def rel(a, b):
            return float((a.double() - b.double()).norm() / b.double().norm())
        own, gap = rel(z_ref, z_exact), rel(z_fused, z_ref)
        print(f'build_latent_object: rel-L2 fused-composed={gap:.3e}, composed-fp64-preprocessed={own:.3e}')
        assert z_fused.shape == z_ref.shape and gap <= 10 * own, (gap, own)
        # bit-equal preprocessed maps give a bit-equal volume: the stacked input against the concatenation
        fused_obs = model.preprocess_observation(obs)
        z_again = model.build_latent_object(fused_obs)                           # flags set: the composed steps + torch.cat
        assert torch.equal(z_again, z_fused)
        # compute_latent_code and render_ibr_basic run under the option
        cams = model.preprocess_observation(synth.make_observation(2, 14, DEV)).camera
        feats = model.compute_latent_code(obs[:2], cams)
        monkeypatch.setattr(model, 'preprocess_kernel', 'composed')
        feats_ref = model.compute_latent_code(obs[:2], cams)
        assert feats.shape == feats_ref.shape and rel(feats, feats_ref) < 1e-3
        y_ref, _ = model.render_ibr_basic(z_ref, obs, cams)
        monkeypatch.setattr(model, 'preprocess_kernel', 'fused')
        y, _ = model.render_ibr_basic(z_ref, obs, cams)
        assert set(y) == set(y_ref) and all(y[k].shape == y_ref[k].shape for k in y)
        for k in y:                                                              # (NaN where the reference has NaN: compared as such)
            u, v = y[k].float(), y_ref[k].float()
            fin = v.isfinite()
            gap = float((u[fin] - v[fin]).abs().max()) if bool(fin.any()) else 0.0
            print(f'render_ibr_basic {k}: max difference fused-composed {gap:.3e}, finite share {float(fin.float().mean()):.3f}')
            assert torch.equal(u.isfinite(), fin) and gap <= 1e-3 * (1.0 + float(v[fin].abs().max() if bool(fin.any()) else 0.0)), k
