"""Initial pose on the device (csrc/depth_init.hip, ops.depth_init, pose/initialization.py kernel='fused') against the host
functions of pose/initialization.py run on CPU copies of the same inputs: _masks_to_viewports(mask, 0), the median / MAD
expressions of _reject_outliers_mad and estimate_translation.  Every comparison is torch.equal -- on trans, on every stats
entry (NaN positions compared as positions) and on every counts entry: all quantities are order statistics, minima / maxima,
counts or single correctly rounded fp32 operations, so there is no tolerance.

Every call of the entry point in this file goes through `_run`, which hands it NaN-poisoned scratch and output buffers with
sentinels behind each of them and checks the sentinels afterwards.

1x1 frames: _masks_to_viewports squeezes the mask, which drops both axes of a 1x1 (or one of a 1xW / Hx1) frame, so for such
frames the same nonzero / min / max expressions are applied to the (H,W) mask directly.  A 1x1 frame holds at most one valid
depth, whose MAD is 0: it appears among the reported cases only."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
INF = float('inf')
SENT, ISENT, GUARD = -777.25, -424242, 64
LF_EINVAL, LF_EALIGN, LF_ENOSPC = -1, -2, -3
FRAMES = [(1, 1), (3, 5), (17, 23), (64, 64), (97, 131), (240, 320)]
BATCHES = [1, 3, 7]
PATTERNS = ['smooth', 'mm', 'lowbyte', 'exponent', 'specials']


def _L():
    from latentfusion_amd import _lib
    return _lib.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _ini():
    from latentfusion_amd.pose import initialization
    return initialization


# ----------------------------------------------------------------------------------------------------------------------
# the entry point, on poisoned buffers with sentinels
# ----------------------------------------------------------------------------------------------------------------------
def _guarded(n, dtype):
    """n elements (NaN bit patterns: all bytes 0xff) followed by GUARD sentinels -> (whole buffer, view of the n elements)."""
    buf = torch.empty(n + GUARD, device=DEV, dtype=dtype)
    buf.view(torch.uint8)[:n * buf.element_size()] = 0xff
    buf[n:] = SENT if dtype.is_floating_point else ISENT
    return buf, buf[:n]


def _intact(buf, n):
    return bool((buf[n:] == (SENT if buf.dtype.is_floating_point else ISENT)).all())


def _run(depth, mask, K=None, m=3.0, r=0):
    """lf_depth_init on CPU inputs: depth (B,H,W) fp32, mask (B,H,W) fp32 / bool / uint8, K None or (1 or B, 3, 3).
    -> (trans (B,3) or None, stats (B,8), counts (B,8)) on the CPU."""
    L = _L()
    B, H, W = depth.shape
    d = depth.to(DEV).contiguous()
    mk = mask.to(DEV).contiguous()
    u8 = mk.dtype != torch.float32
    if mk.dtype == torch.bool:
        mk = mk.view(torch.uint8)
    intr = None
    if K is not None:
        intr = torch.stack((K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]), dim=-1).to(DEV).contiguous()
    tb, trans = _guarded(B * 3, torch.float32)
    sb, stats = _guarded(B * 8, torch.float32)
    cb, counts = _guarded(B * 8, torch.int32)
    nbytes = L.lf_depth_init_scratch_bytes(B, H, W)
    assert nbytes >= B * H * W * 4 and nbytes % 4 == 0
    xb, _ = _guarded(nbytes // 4, torch.float32)
    rc = L.lf_depth_init(d.data_ptr(), mk.data_ptr(), int(u8), intr.data_ptr() if intr is not None else None,
                         intr.shape[0] if intr is not None else 1, m, r, trans.data_ptr() if intr is not None else None,
                         stats.data_ptr(), counts.data_ptr(), xb.data_ptr(), nbytes, B, H, W, _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert _intact(tb, B * 3) and _intact(sb, B * 8) and _intact(cb, B * 8) and _intact(xb, nbytes // 4)
    if intr is None:
        assert bool(torch.isnan(trans).all())                                   # not touched without intrinsics
    return (trans.view(B, 3).cpu() if intr is not None else None), stats.view(B, 8).cpu(), counts.view(B, 8).cpu()


def _same(a, b):
    """torch.equal with NaN positions compared as positions."""
    na, nb = torch.isnan(a), torch.isnan(b)
    zero = torch.zeros((), dtype=a.dtype)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(torch.where(na, zero, a), torch.where(nb, zero, b))


# ----------------------------------------------------------------------------------------------------------------------
# the yardstick: the host functions on one frame; the degenerate frames filled in as the header specifies them
# ----------------------------------------------------------------------------------------------------------------------
def _erode_conv2d(fg, r):
    """The conv2d form of initialization._erode_mask (before its guard discards the result): fg (H,W) bool."""
    k = _ini()._disk(r, 'cpu')
    m = F.pad(fg.float()[None, None], (r, r, r, r), value=1.0)
    return (F.conv2d(m, k[None, None]) >= k.sum() - 0.5)[0, 0]


def _viewport(fg):
    H, W = fg.shape
    if H > 1 and W > 1:
        return _ini()._masks_to_viewports(fg[None, None], 0)[0]
    coords = torch.nonzero(fg).float()                                          # (see the module docstring)
    return torch.stack([coords[:, 1].min(), coords[:, 0].min(), coords[:, 1].max(), coords[:, 0].max()])


def _host_row(depth, mask, K=None, m=3.0, r=0, variant=None):
    """Expected (trans (3,) or None, stats (8,), counts (8,)) of one frame: depth (H,W), mask (H,W), K (3,3).
    variant: a deliberate misreading of the contract (the wrong-reading controls)."""
    fg = mask.bool()
    n_mask = int(fg.sum())
    stats = torch.full((8,), NAN)
    stats[7] = 0.0
    counts = torch.tensor([n_mask, 0, 0, -1, -1, -1, -1, 0], dtype=torch.int32)
    inside = _erode_conv2d(fg, r) if r > 0 else fg
    if n_mask:
        box_of = inside if variant == 'bbox_eroded' and bool(inside.any()) else fg
        vp = _viewport(box_of)
        counts[3:7] = vp.to(torch.int32)
        stats[5], stats[6] = (vp[2] + vp[0]) / 2.0, (vp[3] + vp[1]) / 2.0
        if variant == 'centroid':
            coords = torch.nonzero(fg).float()
            stats[5], stats[6] = coords[:, 1].mean(), coords[:, 0].mean()
    positive = depth >= 0.0 if variant == 'depth_ge_0' else depth > 0.0
    vals = depth[inside & fg & positive]
    counts[1] = vals.numel()
    if vals.numel():
        median = vals.median()                                                  # _reject_outliers_mad's expressions
        if variant == 'upper_median':
            median = vals.sort().values[vals.numel() // 2]
        if variant == 'mean':
            median = vals.mean()
        mad = torch.median(torch.abs(vals - median))
        keep = torch.abs(vals - median) / mad <= m if variant == 'le_m' else torch.abs(vals - median) / mad < m
        kept = vals[keep]
        stats[1], stats[2] = median, mad
        counts[2] = kept.numel()
        if kept.numel():
            stats[3], stats[4] = kept.min(), kept.max()
            stats[0] = (kept.min() + kept.max()) / 2.0                          # _estimate_camera_dist
    trans = None
    if K is not None:
        z = stats[0]
        trans = torch.stack(((stats[5] - K[0, 2]) / K[0, 0] * z, (stats[6] - K[1, 2]) / K[1, 1] * z, z))   # estimate_translation
        if counts[2] == 0:
            trans = torch.full((3,), NAN)
    return trans, stats, counts


def _host(depth, mask, K=None, m=3.0, r=0, variant=None):
    rows = [_host_row(depth[b], mask[b], None if K is None else K[b if K.shape[0] > 1 else 0], m, r, variant)
            for b in range(depth.shape[0])]
    return (None if K is None else torch.stack([t for t, _, _ in rows]), torch.stack([s for _, s, _ in rows]),
            torch.stack([c for _, _, c in rows]))


def _assert_regular(counts):
    """A regular case, decided on the CPU from the host expressions' counts (_host): at least three valid depths, of which the
    MAD filter keeps at least half -- a case cannot pass by rejecting everything."""
    assert bool((counts[:, 2] * 2 >= counts[:, 1]).all()) and bool((counts[:, 1] >= 3).all()), counts[:, :3]


def _assert_equal(got, want, what=''):
    for g, w, name in zip(got, want, ('trans', 'stats', 'counts')):
        if w is None:
            assert g is None, (what, name)
        elif name == 'counts':
            assert torch.equal(g, w), (what, name, g, w)
        else:
            assert _same(g, w), (what, name, g, w)


# ----------------------------------------------------------------------------------------------------------------------
# committed cases
# ----------------------------------------------------------------------------------------------------------------------
def _blob_mask(B, H, W, g):
    """An off-centre ellipse per frame (about a third of the frame), clipped by the frame; tiny frames: all but a corner."""
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    out = torch.zeros(B, H, W)
    for b in range(B):
        cy, cx = (0.35 + 0.3 * torch.rand(2, generator=g)).tolist()
        out[b] = (((y - cy * H) / (0.36 * H)) ** 2 + ((x - cx * W) / (0.3 * W)) ** 2 <= 1.0).float()
        if H * W <= 15:
            out[b] = 1.0
            out[b, 0, 0] = 0.0
    return out


def _bits(t):
    return t.to(torch.int32).view(torch.float32)


def _depth(pattern, B, H, W, mask, g):
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing='ij')
    if pattern in ('smooth', 'specials'):                                        # a surface plus 2 % far outliers
        d = 0.8 + 0.1 * x / W + 0.05 * y / H + 0.002 * torch.rand(B, H, W, generator=g)
        far = torch.rand(B, H, W, generator=g) < 0.02
        d = torch.where(far, d * 3.0, d)
        if pattern == 'specials':                                                # zeros, negatives, NaN and +inf inside the mask
            u = torch.rand(B, H, W, generator=g)
            for lo, v in ((0.00, 0.0), (0.04, -0.7), (0.08, NAN), (0.12, INF)):
                d = torch.where((u >= lo) & (u < lo + 0.04), torch.full_like(d, v), d)
        return d
    if pattern == 'mm':                                                          # millimetres: many ties in the median's bucket
        d = 0.7 + 0.04 * x / W + 0.02 * torch.rand(B, H, W, generator=g)
        return torch.round(d * 1000.0) / 1000.0
    if pattern == 'lowbyte':                                                     # only the lowest mantissa byte differs
        return _bits(0x3f800000 + torch.randint(0, 256, (B, H, W), generator=g))
    if pattern == 'exponent':                                                    # only the exponent differs
        return _bits((torch.randint(118, 134, (B, H, W), generator=g) << 23) | 0x2aaaaa)
    raise KeyError(pattern)


def _intrinsics(B, H, W, g):
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = 500.0 + 100.0 * torch.rand(B, generator=g)
    K[:, 1, 1] = 480.0 + 100.0 * torch.rand(B, generator=g)
    K[:, 0, 2] = W / 2.0 + torch.rand(B, generator=g)
    K[:, 1, 2] = H / 2.0 + torch.rand(B, generator=g)
    K[:, 2, 2] = 1.0
    return K


def _case(H, W, B, pattern, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + 31 * B + PATTERNS.index(pattern))
    mask = _blob_mask(B, H, W, g)
    return _depth(pattern, B, H, W, mask, g), mask, _intrinsics(B, H, W, g)


@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('frame', FRAMES[1:])
def test_regular_frames_equal_the_host_functions(frame, B):
    ini = _ini()
    H, W = frame
    for pattern in PATTERNS:
        depth, mask, K = _case(H, W, B, pattern)
        want = _host(depth, mask, K)
        _assert_regular(want[2])
        # the restated rows ARE the host path: estimate_translation on the CPU batch gives the same translation
        host = torch.stack(ini.estimate_translation(depth[:, None], mask[:, None], K), dim=-1)
        assert torch.equal(host, want[0]), pattern
        vp = ini._masks_to_viewports(mask[:, None], 0)
        assert torch.equal(vp.to(torch.int32), want[2][:, 3:7])
        for mk in (mask, mask.bool(), mask.to(torch.uint8)):                    # both mask forms of the ABI (bool rides as bytes)
            _assert_equal(_run(depth, mk, K), want, (pattern, mk.dtype, 'intr_n=B'))
        want1 = _host(depth, mask, K[:1])
        _assert_equal(_run(depth, mask, K[:1]), want1, (pattern, 'intr_n=1'))
        _assert_equal(_run(depth, mask.bool(), None), (None,) + want1[1:], (pattern, 'no intrinsics'))


def test_even_and_odd_counts_and_the_three_value_frame():
    depth, mask, K = _case(17, 23, 1, 'smooth', seed=3)
    seen = set()
    for drop in range(2):
        d = depth.clone()
        ys, xs = torch.nonzero(mask[0].bool() & (d[0] > 0), as_tuple=True)
        for i in range(drop):
            d[0, ys[i], xs[i]] = 0.0
        want = _host(d, mask, K)
        _assert_regular(want[2])
        seen.add(int(want[2][0, 1]) % 2)
        _assert_equal(_run(d, mask, K), want, drop)
    assert seen == {0, 1}
    # [1, 2, 4]: median 2, MAD 1, all kept, z = 2.5
    d = torch.zeros(1, 3, 5)
    mk = torch.zeros(1, 3, 5)
    for (yy, xx), v in zip(((0, 1), (2, 4), (1, 2)), (1.0, 2.0, 4.0)):
        d[0, yy, xx], mk[0, yy, xx] = v, 1.0
    got = _run(d, mk, K)
    _assert_equal(got, _host(d, mk, K))
    assert got[1][0, :5].tolist() == [2.5, 2.0, 1.0, 1.0, 4.0] and got[2][0].tolist() == [3, 3, 3, 1, 0, 4, 2, 0]
    assert got[1][0, 5:].tolist() == [2.5, 1.0, 0.0]


def test_float_mask_with_fractions_and_nan_is_foreground():
    depth, mask, K = _case(17, 23, 3, 'smooth', seed=4)
    odd = mask.clone()
    fg = odd.bool()
    odd[fg & (depth > 0.85)] = 0.5
    odd[fg & (depth > 0.9)] = NAN
    odd[0, 0, 22] = NAN                                                          # a NaN outside the blob widens the box
    assert bool(torch.isnan(odd).any()) and bool((odd == 0.5).any())
    want = _host(depth, odd, K)
    assert torch.equal(want[2][1:], _host(depth, mask, K)[2][1:]) and int(want[2][0, 5]) == 22
    _assert_regular(want[2])
    _assert_equal(_run(depth, odd, K), want)


# ----------------------------------------------------------------------------------------------------------------------
# reported, not raised
# ----------------------------------------------------------------------------------------------------------------------
def _reported_cases():
    """name -> (depth (1,H,W), mask (1,H,W), expected (n_mask, n_valid, n_kept), NaN pattern of stats[:7])."""
    H, W = 17, 23
    depth, mask, _ = _case(H, W, 1, 'smooth', seed=5)
    n_mask = int(mask.sum())
    cases = {}
    box_only = [True] * 5 + [False, False]
    cases['empty mask'] = (depth, torch.zeros_like(mask), (0, 0, 0), [True] * 7)
    cases['no positive depth'] = (torch.where(depth > 0.82, torch.full_like(depth, NAN), -depth), mask, (n_mask, 0, 0), box_only)
    for n in (1, 2):
        d = torch.zeros_like(depth)
        ys, xs = torch.nonzero(mask[0].bool(), as_tuple=True)
        for i in range(n):
            d[0, ys[7 * i], xs[7 * i]] = 0.5 + 0.25 * i
        cases[f'n_valid = {n}'] = (d, mask, (n_mask, n, 0), [True, False, False, True, True, False, False])
    cases['constant depth'] = (torch.full_like(depth, 0.75), mask, (n_mask, n_mask, 0),
                               [True, False, False, True, True, False, False])
    d = depth.clone()
    d[0, :, : W // 2 + 3] = INF
    assert int(((d == INF) & mask.bool()).sum()) * 2 > n_mask
    cases['more than half +inf'] = (d, mask, (n_mask, n_mask, 0), [True, False, True, True, True, False, False])
    one = torch.ones(1, 1, 1)
    cases['1x1 foreground'] = (one * 0.6, one, (1, 1, 0), [True, False, False, True, True, False, False])
    cases['1x1 zero depth'] = (one * 0.0, one, (1, 0, 0), box_only)
    cases['1x1 background'] = (one * 0.6, one * 0.0, (0, 0, 0), [True] * 7)
    return cases


@pytest.mark.parametrize('name', ['empty mask', 'no positive depth', 'n_valid = 1', 'n_valid = 2', 'constant depth',
                                  'more than half +inf', '1x1 foreground', '1x1 zero depth', '1x1 background'])
def test_degenerate_frames_are_reported(name):
    ini = _ini()
    depth, mask, n3, nan7 = _reported_cases()[name]
    H, W = depth.shape[-2:]
    K = _intrinsics(1, H, W, torch.Generator().manual_seed(1))
    for mk in (mask, mask.to(torch.uint8)):
        trans, stats, counts = _run(depth, mk, K)
        assert counts[0, :3].tolist() == list(n3), name
        assert torch.isnan(stats[0, :7]).tolist() == nan7 and float(stats[0, 7]) == 0.0 and int(counts[0, 7]) == 0
        assert bool(torch.isnan(trans).all())
        if n3[0] == 0:
            assert counts[0, 3:7].tolist() == [-1, -1, -1, -1]
        _assert_equal((trans, stats, counts), _host(depth, mask, K), name)
        if name == 'n_valid = 2':                                                # the lower median of two, and its MAD of 0
            assert stats[0, 1:3].tolist() == [0.5, 0.0]
        if name == 'more than half +inf':
            assert float(stats[0, 1]) == INF
    # the same input sends the host path into an error (or, where torch lets a NaN comparison through, into a NaN translation):
    # these are the frames the composed path does not answer
    try:
        host = torch.stack(ini.estimate_translation(depth[:, None], mask[:, None], K), dim=-1)
    except (RuntimeError, IndexError, ValueError):
        host = None
    assert host is None, (name, host)
    # and inside a batch such a frame leaves its neighbours alone
    good = _case(H, W, 1, 'smooth', seed=6) if H > 1 else None
    if good is not None:
        d3, m3 = torch.cat([good[0], depth, good[0]]), torch.cat([good[1], mask, good[1]])
        K3 = _intrinsics(3, H, W, torch.Generator().manual_seed(2))
        _assert_equal(_run(d3, m3, K3), _host(d3, m3, K3), name)


# ----------------------------------------------------------------------------------------------------------------------
# g14: the reference's record
# ----------------------------------------------------------------------------------------------------------------------
def test_g14_fixture(golden):
    ini = _ini()
    g = golden('g14_initial_pose')
    depth, mask, K = g['depth'], g['mask'], g['K']
    assert tuple(depth.shape[-2:]) == (240, 320)
    host = torch.stack(ini.estimate_translation(depth, mask.float(), K), dim=-1)
    for mk in (mask.float(), mask.bool()):
        got = _run(depth[:, 0].contiguous(), mk[:, 0].contiguous(), K)
        assert torch.equal(got[0], host)
        assert float((got[0] - g['translation']).abs().max()) <= 1e-6
        _assert_equal(got, _host(depth[:, 0], mk[:, 0], K))


# ----------------------------------------------------------------------------------------------------------------------
# erosion
# ----------------------------------------------------------------------------------------------------------------------
def _holes(b, H, W):
    """(y, x) of the single-pixel holes of frame b: inside the foreground right of the band, a second one in wide frames."""
    return [(H // 3 + b, 6)] + ([(2 * H // 3, W // 4 + b)] if W >= 64 else [])


def _eroding_mask(B, H, W):
    """Foreground that touches every border, a two-column background band crossed by a one-pixel bridge, and single-pixel
    holes (_holes) inside the foreground."""
    mask = torch.ones(B, H, W)
    for b in range(B):
        mask[b, :, 2:4] = 0.0
        mask[b, H // 2 + b, 2:4] = 1.0                                           # the bridge
        for y, x in _holes(b, H, W):
            mask[b, y, x] = 0.0
    return mask


@pytest.mark.parametrize('frame', [(17, 23), (64, 64), (97, 131)])
@pytest.mark.parametrize('r', [1, 3, 8])
def test_erosion_equals_the_conv2d_form(frame, r):
    H, W = frame
    B = 3
    g = torch.Generator().manual_seed(H + r)
    depth = _depth('specials', B, H, W, None, g)
    mask = _eroding_mask(B, H, W)
    K = _intrinsics(B, H, W, g)
    for b in range(B):                                                           # the masks are what the docstring says
        fg = mask[b].bool()
        assert bool(fg[0].any() and fg[-1].any() and fg[:, 0].any() and fg[:, -1].any()) and not bool(fg.all())
        assert int(fg[:, 2].sum()) == 1 and int(fg[:, 3].sum()) == 1 and bool(fg[H // 2 + b, 2:4].all())      # the bridge
        for y, x in _holes(b, H, W):                                             # each hole: one background pixel, foreground all round
            assert not bool(fg[y, x]) and int(fg[y - 1:y + 2, x - 1:x + 2].sum()) == 8
    want = _host(depth, mask, K, r=r)
    plain = _host(depth, mask, K)
    _assert_regular(want[2])
    assert bool((want[2][:, 1] < plain[2][:, 1]).all()) and torch.equal(want[2][:, 3:7], plain[2][:, 3:7])
    for mk in (mask, mask.to(torch.uint8)):
        _assert_equal(_run(depth, mk, K, r=r), want, (r, mk.dtype))
    _assert_equal(_run(depth, mask, K, r=0), _run(depth, mask, K), 'r = 0')
    _assert_equal(_run(depth, mask, K, r=0), plain, 'r = 0')
    # a mask the disk erases entirely: reported
    thin = torch.zeros(1, H, W)
    thin[0, H // 2, 1:W - 1] = 1.0
    got = _run(depth[:1], thin, K[:1], r=r)
    assert got[2][0, :3].tolist() == [W - 2, 0, 0] and got[2][0, 3:7].tolist() == [1, H // 2, W - 2, H // 2]
    _assert_equal(got, _host(depth[:1], thin, K[:1], r=r))


# ----------------------------------------------------------------------------------------------------------------------
# wrong-reading controls: each misreading of the contract fails, on a committed case, the comparison the kernel passes
# ----------------------------------------------------------------------------------------------------------------------
def _control_cases():
    cases = [(*_case(17, 23, 3, 'smooth'), 0), (*_case(64, 64, 3, 'specials'), 0), (*_case(97, 131, 1, 'mm'), 0)]
    d = torch.zeros(1, 3, 5)                                                    # a depth at exactly m MADs: 6 of [1 2 2 3 3 3 4 4 6]
    d[0].view(-1)[:9] = torch.tensor([1.0, 2.0, 2.0, 3.0, 3.0, 3.0, 4.0, 4.0, 6.0])
    cases.append((d, (d > 0).float(), _intrinsics(1, 3, 5, torch.Generator().manual_seed(3)), 0))
    g = torch.Generator().manual_seed(11)
    cases.append((_depth('smooth', 2, 17, 23, None, g), _eroding_mask(2, 17, 23), _intrinsics(2, 17, 23, g), 3))
    return cases


@pytest.mark.parametrize('variant', ['upper_median', 'mean', 'le_m', 'centroid', 'bbox_eroded', 'depth_ge_0'])
def test_wrong_readings_fail_the_comparison(variant):
    failed = 0
    for depth, mask, K, r in _control_cases():
        got = _run(depth, mask, K, r=r)
        _assert_equal(got, _host(depth, mask, K, r=r))                           # the kernel passes
        wrong = _host(depth, mask, K, r=r, variant=variant)
        failed += not (_same(got[0], wrong[0]) and _same(got[1], wrong[1]) and torch.equal(got[2], wrong[2]))
    assert failed >= 1, variant


# ----------------------------------------------------------------------------------------------------------------------
# independence
# ----------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_or_the_run():
    H, W, B = 97, 131, 7
    parts = [_case(H, W, 1, p, seed=8 + i) for i, p in enumerate(PATTERNS + ['smooth', 'mm'])]
    depth, mask, K = (torch.cat([p[k] for p in parts]) for k in range(3))
    depth[5, :, :] = 0.0                                                        # a reported row among the regular ones
    whole = _run(depth, mask, K, r=1)
    again = _run(depth, mask, K, r=1)
    _assert_equal(again, whole, 'second run')
    _assert_equal(whole, _host(depth, mask, K, r=1))
    assert whole[2][5, 1] == 0
    for b in range(B):
        one = _run(depth[b:b + 1], mask[b:b + 1], K[b:b + 1], r=1)
        _assert_equal(one, tuple(t[b:b + 1] for t in whole), b)


# ----------------------------------------------------------------------------------------------------------------------
# ABI errors: a negative code, nothing launched, nothing written
# ----------------------------------------------------------------------------------------------------------------------
def test_abi_errors_leave_the_outputs_alone():
    L = _L()
    B, H, W = 3, 17, 23
    depth, mask, K = _case(H, W, B, 'smooth')
    d, mk = depth.to(DEV), mask.to(DEV)
    intr = torch.rand(B, 4, device=DEV) + 100.0
    trans = torch.full((B * 3,), SENT, device=DEV)
    stats = torch.full((B * 8,), SENT, device=DEV)
    counts = torch.full((B * 8,), ISENT, device=DEV, dtype=torch.int32)
    nbytes = L.lf_depth_init_scratch_bytes(B, H, W)
    scratch = torch.full((nbytes // 4 + 2,), SENT, device=DEV)
    assert scratch.data_ptr() % 8 == 0
    good = dict(depth=d.data_ptr(), mask=mk.data_ptr(), u8=0, intr=intr.data_ptr(), intr_n=B, m=3.0, r=0, trans=trans.data_ptr(),
                stats=stats.data_ptr(), counts=counts.data_ptr(), scratch=scratch.data_ptr(), nbytes=nbytes, B=B, H=H, W=W)

    def call(**over):
        a = dict(good, **over)
        return L.lf_depth_init(a['depth'], a['mask'], a['u8'], a['intr'], a['intr_n'], a['m'], a['r'], a['trans'], a['stats'],
                               a['counts'], a['scratch'], a['nbytes'], a['B'], a['H'], a['W'], _s())
    cases = [(dict(depth=None), LF_EINVAL), (dict(mask=None), LF_EINVAL), (dict(stats=None), LF_EINVAL),
             (dict(counts=None), LF_EINVAL), (dict(scratch=None), LF_EINVAL), (dict(trans=None), LF_EINVAL),
             (dict(intr=None), LF_EINVAL),                                       # intrinsics and trans go together
             (dict(B=0), LF_EINVAL), (dict(H=0), LF_EINVAL), (dict(W=0), LF_EINVAL), (dict(B=-1), LF_EINVAL),
             (dict(H=-17), LF_EINVAL), (dict(W=-23), LF_EINVAL),
             (dict(B=1 << 15, H=1 << 8, W=1 << 8, intr_n=1), LF_EINVAL),         # B * H * W = 2^31
             (dict(B=1, H=1 << 16, W=1 << 16, intr_n=1), LF_EINVAL),             # H * W = 2^32 (0 as a 32-bit product)
             (dict(r=-1), LF_EINVAL), (dict(r=9), LF_EINVAL), (dict(m=0.0), LF_EINVAL), (dict(m=-3.0), LF_EINVAL),
             (dict(m=NAN), LF_EINVAL), (dict(intr_n=2), LF_EINVAL), (dict(intr_n=0), LF_EINVAL), (dict(intr_n=B + 1), LF_EINVAL),
             (dict(u8=2), LF_EINVAL), (dict(u8=-1), LF_EINVAL),
             (dict(nbytes=nbytes - 4), LF_ENOSPC), (dict(nbytes=0), LF_ENOSPC)]
    cases += [({k: good[k] + off}, LF_EALIGN) for k in ('depth', 'mask', 'intr', 'trans', 'stats', 'counts') for off in (1, 2)]
    cases += [(dict(mask=good['mask'] + 1, u8=1), LF_EALIGN), (dict(scratch=good['scratch'] + 4), LF_EALIGN),
              (dict(scratch=good['scratch'] + 2), LF_EALIGN)]
    for over, want in cases:
        assert call(**over) == want, over
    torch.cuda.synchronize()
    assert (trans == SENT).all() and (stats == SENT).all() and (counts == ISENT).all() and (scratch == SENT).all()
    for bad in ((0, H, W), (B, 0, W), (B, H, 0), (-1, H, W), (1 << 15, 1 << 8, 1 << 8)):
        assert L.lf_depth_init_scratch_bytes(*bad) == 0, bad
    assert call(intr=None, trans=None, intr_n=0) == 0                            # intr_n is not read without intrinsics
    assert call(intr_n=1) == 0 and call() == 0
    torch.cuda.synchronize()
    assert not (trans == SENT).any() and not (stats == SENT).any() and not (counts == ISENT).any()
    assert (scratch[nbytes // 4:] == SENT).all()                                 # (the elements past the query's answer)
    _assert_equal((trans.view(B, 3).cpu(), stats.view(B, 8).cpu(), counts.view(B, 8).cpu()),
                  _host(depth, mask, _k_of(intr.cpu())))


def _k_of(intr):
    K = torch.zeros(intr.shape[0], 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 1.0
    return K


# ----------------------------------------------------------------------------------------------------------------------
# plumbing: ops.depth_init, estimate_initial_pose, Observation, the estimators
# ----------------------------------------------------------------------------------------------------------------------
def _sections(fn):
    from latentfusion_amd import ops
    ops.KERNEL_TIMER = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [str(name) for name, _, _ in ops.KERNEL_TIMER]
    finally:
        ops.KERNEL_TIMER = None


def test_wrapper_equals_the_entry_point_and_times_one_section():
    from latentfusion_amd import ops
    for B in (1, 7):
        depth, mask, K = _case(64, 64, B, 'specials')
        want = _run(depth, mask, K)
        for d, mk, k in ((depth[:, None], mask[:, None], K), (depth, mask.bool(), K[:1]), (depth, mask.to(torch.uint8)[:, None], None)):
            out, names = _sections(lambda: ops.depth_init(d.to(DEV), mk.to(DEV), None if k is None else k.to(DEV)))
            assert names == ['depth_init'], names
            assert ('trans' in out) == (k is not None) and out['counts'].dtype == torch.int32 and out['stats'].shape == (B, 8)
            exp = want if k is K else _run(depth, mask, k)
            got = (out['trans'].cpu() if k is not None else None, out['stats'].cpu(), out['counts'].cpu())
            _assert_equal(got, exp)
        odd = mask.to(torch.uint8).to(DEV).flatten()
        odd = torch.cat([odd.new_zeros(1), odd])[1:].view(B, 64, 64)            # a byte mask on an odd address
        assert odd.data_ptr() % 4 == 1
        out = ops.depth_init(depth.to(DEV), odd, K.to(DEV), m=3.0, erode_radius=2)
        _assert_equal((out['trans'].cpu(), out['stats'].cpu(), out['counts'].cpu()), _run(depth, mask, K, r=2))


def test_fused_pose_equals_composed_on_g14_and_synthetic_frames(golden):
    from latentfusion_amd import synth
    ini = _ini()
    g = golden('g14_initial_pose')
    for dev in ('cpu', DEV):
        depth, mask, K = g['depth'].to(dev), g['mask'].float().to(dev), g['K'].to(dev)
        a = ini.estimate_initial_pose(depth, mask, K, g['width'], g['height'])
        b = ini.estimate_initial_pose(depth, mask, K, g['width'], g['height'], kernel='fused')
        assert b.translation.device == a.translation.device
        for f in ('translation', 'log_quaternion', 'intrinsic', 'viewport'):
            assert torch.equal(getattr(a, f), getattr(b, f)), (dev, f)
        assert float((b.translation.cpu() - g['translation']).abs().max()) <= 1e-6
    obs = synth.make_observation(2, 5, 'cpu')
    for o in (obs, obs.to(DEV)):
        a, b = o.estimate_camera(), o.estimate_camera(kernel='fused')
        assert torch.equal(a.translation, b.translation) and torch.equal(a.extrinsic, b.extrinsic)
        assert b.translation.device == a.translation.device
        za, zb = o.zoom_estimate(1.5, 32), o.zoom_estimate(1.5, 32, kernel='fused')
        assert torch.equal(za.depth, zb.depth) and torch.equal(za.camera.viewport, zb.camera.viewport)
    with pytest.raises(ValueError, match='erode_radius'):
        obs.estimate_camera(erode_radius=3)
    c = obs.to(DEV).estimate_camera(kernel='fused', erode_radius=3)
    assert bool(torch.isfinite(c.translation).all())
    saved = ini.KERNEL
    try:                                                                         # the module switch is what None resolves to
        ini.KERNEL = 'fused'
        out, names = _sections(lambda: obs.to(DEV).estimate_camera())
        assert names == ['depth_init'] and torch.equal(out.translation.cpu(), obs.estimate_camera(kernel='composed').translation)
    finally:
        ini.KERNEL = saved


def test_check_names_the_bad_rows_and_without_it_they_are_nan():
    ini = _ini()
    depth, mask, K = _case(64, 64, 4, 'smooth', seed=9)
    mask[1] = 0.0
    depth[3] = 0.75
    n3 = int(mask[3].sum())
    d, mk, k = depth[:, None].to(DEV), mask[:, None].to(DEV), K.to(DEV)
    with pytest.raises(ValueError) as e:
        ini.estimate_translation(d, mk, k, kernel='fused')
    msg = str(e.value)
    assert '1 (n_mask=0, n_valid=0, n_kept=0)' in msg and f'3 (n_mask={n3}, n_valid={n3}, n_kept=0)' in msg
    assert '0 (' not in msg and '2 (' not in msg
    t = torch.stack(ini.estimate_translation(d, mk, k, kernel='fused', check=False), dim=-1).cpu()
    assert torch.isnan(t).all(dim=1).tolist() == [False, True, False, True]
    good = torch.stack(ini.estimate_translation(depth[[0, 2], None], mask[[0, 2], None], K[[0, 2]]), dim=-1)
    assert torch.equal(t[[0, 2]], good)
    cam = ini.estimate_initial_pose(d, mk, k, 64, 64, kernel='fused', check=False)
    assert torch.isnan(cam.translation[1]).all() and torch.equal(cam.translation[0].cpu(), good[0])


def _multi():
    """tests/test_multi_target_estimator_gpu.py as a module: its _shifted targets, _setup() model and _estimator()."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_multi_target_estimator_gpu.py')
    spec = importlib.util.spec_from_file_location('_multi_target_estimator_cases', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_initial_pose_batch_equals_initial_pose_per_target():
    from latentfusion_amd import synth
    from latentfusion_amd.pose import estimation
    mt = _multi()
    tg0 = synth.make_observation(1, 5, 'cpu')
    targets = [mt._shifted(tg0, 0, 0), mt._shifted(tg0, 9, -14), mt._shifted(tg0, -7, 11)]
    est = estimation.PoseEstimator(model=None, ranking_size=1, loss_weights={})
    want = [estimation.PoseEstimator.initial_pose(t) for t in targets]
    assert len({tuple(w.translation[0].tolist()) for w in want}) == 3           # the shifts move the estimate
    for tgs in (targets, [t.to(DEV) for t in targets]):
        got, names = _sections(lambda: est.initial_pose_batch(tgs, kernel='fused'))
        assert names == ['depth_init'] and len(got) == 3
        for gc, wc, t in zip(got, want, tgs):
            assert len(gc) == 1 and gc.translation.device == t.depth.device
            assert torch.equal(gc.translation.cpu(), wc.translation) and torch.equal(gc.extrinsic.cpu(), wc.extrinsic)
            assert torch.equal(gc.intrinsic.cpu(), wc.intrinsic) and (gc.width, gc.height) == (wc.width, wc.height)
        got, names = _sections(lambda: est.initial_pose_batch(tgs))            # the default: the per-target host loop
        assert names == [] and all(torch.equal(gc.translation.cpu(), wc.translation) for gc, wc in zip(got, want))
    fused = estimation.PoseEstimator(model=None, ranking_size=1, loss_weights={}, init_kernel='fused')
    got, names = _sections(lambda: fused.initial_pose_batch(targets))
    assert names == ['depth_init'] and all(torch.equal(gc.translation, wc.translation) for gc, wc in zip(got, want))
    assert torch.equal(fused._initial_pose(targets[1]).translation, want[1].translation)


def test_estimate_batch_with_drawn_cameras_is_the_same_under_both_init_kernels():
    mt = _multi()
    model, z_obj, targets, _ = mt._setup()
    runs = {}
    for kernel in ('fused', 'composed'):
        est = mt._estimator(model, num_iters=4, return_camera_history=False, init_kernel=kernel)
        torch.manual_seed(0)
        runs[kernel], names = _sections(lambda: est.estimate_batch(z_obj, targets))
        assert names.count('depth_init') == (kernel == 'fused')
    default = mt._estimator(model, num_iters=4, return_camera_history=False)
    assert default.init_kernel == 'composed'
    for (best_f, stats_f), (best_c, stats_c) in zip(runs['fused'], runs['composed']):
        for f in ('log_quaternion', 'translation', 'viewport', 'intrinsic'):
            assert torch.equal(getattr(best_f, f), getattr(best_c, f)), f
        assert set(stats_f) == set(stats_c)
        for k in stats_c:
            assert torch.equal(stats_f[k], stats_c[k]), k
