"""What tests/test_resample_fp64_gpu.py and tests/test_resample_cases.py share: an fp64 restatement of the 3-D resampler of
include/lf_hip.h (lf_resample3d_fwd, lf_resample3d_bwd_coef, lf_resample3d_bwd_vol(_det)), the same expressions in fp32 through
F.grid_sample and autograd (e32, and the stand-in for the kernel where there is no GPU), the input families, the case tables,
the bounds and the misreadings the comparison has to reject.  Nothing here needs a GPU.

THE RESTATEMENT (`reference`) is explicit: lattice, grid, position, taps, weights, mask, sums, written out in plain torch, so that
what happens to a NaN or an infinite coordinate and to a position on a face comes from the header and not from an ATen build:

    lattice      torch.linspace(0, 1, S) ([0] for S = 1)
    grid         LF_MAP_O2C  g = c0 + c1 a + c2 b + c3 k + c4 a k + c5 b k,  c_j = coef[n][3 j .. 3 j + 2]
                 LF_MAP_C2O  l = (2 a - 1, 2 b - 1, 2 k - 1, 1), g = (A0.l / A3.l, A1.l / A3.l, A2.l), A_r = coef[n][4 r ..]
                 (row stride LF_MAP_COEFS)
    position     p = ((g + 1) S - 1) / 2, NaN -> 0, clamped to [0, S - 1]
    taps         floor(p) and min(floor(p) + 1, S - 1)
    mask, gain   d p / d g = S / 2 where 0 < p < S - 1 (strict, on the unclamped p), 0 elsewhere

Volumes are channels-last, [n][D][H][W][C], as the C ABI has them.  tests/test_resample_cases.py ties the restatement to
F.grid_sample(mode='bilinear', padding_mode='border', align_corners=False) in fp64 -- the call of the reference project
(modules/geometry.py:625-690) -- on every finite case.

TWO FAMILIES OF INPUTS.  `lattice`: sizes 2^m + 1 (and 1), coefficients that are small multiples of 1/16, so that every grid value
and every position is exactly representable in fp32 however the multiply-adds are contracted; kernel and fp64 then interpolate
at the SAME position and only the arithmetic behind it differs, which gives bounds of a few ulp (`fwd_ratio`, `gvol_ratio`,
`gcoef_ratio` with family='lattice').  `general`: the product's sizes with rotations, scales and perspective terms, under the
project's standing bounds with e32.

The yardstick of a coefficient sum is not its own size -- the 18 sums cancel -- but the sum of the absolute values of its terms,
    A_j = sum over voxels |basis_j| gain mask sum_c |gout_c| sum over corner pairs |v_hi - v_lo| w,
so that a dropped or doubled voxel (about A_j / voxels) stands far above the 2e-5 A_j that rounding is allowed.
"""
import functools

import torch
import torch.nn.functional as F

O2C, C2O = 0, 1
LF_MAP_COEFS = 20
LF_EINVAL = -1
U = 2.0 ** -24                      # unit roundoff of fp32

MISREADINGS = ('align_corners', 'zeros_padding', 'step_1_over_S', 'ak_bk_swapped', 'gz_divided', 'half_voxel', 'mask_nonstrict',
               'mask_absent', 'size1_at_1')


# ---- ordinary maps (moved here from tests/test_resample_staged_gpu.py, which imports them) --------------------------------------
def _rot(gen):
    q = torch.randn(4, generator=gen, dtype=torch.float64)
    w, x, y, z = (q / q.norm()).tolist()
    return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=torch.float64)


def o2c_coefs(N, gen, scales, persp=0.1, shift=0.1):
    """(N,20) blocks: g = t + s R (2 (a,b,k) - 1) + perspective-like a*k, b*k terms."""
    cf = torch.zeros(N, 20, dtype=torch.float64)
    for n in range(N):
        R, s = _rot(gen), scales[n % len(scales)]
        t = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * 2 * shift
        M = 2 * s * R
        cf[n, 0:3] = t - s * R.sum(dim=1)
        cf[n, 3:6], cf[n, 6:9], cf[n, 9:12] = M[:, 0], M[:, 1], M[:, 2]
        cf[n, 12:15] = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * 2 * persp
        cf[n, 15:18] = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * 2 * persp
    return cf


def c2o_coefs(N, gen, scales, persp=0.15):
    cf = torch.zeros(N, 20, dtype=torch.float64)
    for n in range(N):
        R, s = _rot(gen), scales[n % len(scales)]
        A = torch.zeros(4, 4, dtype=torch.float64)
        A[:3, :3] = s * R
        A[:3, 3] = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * 0.2
        A[3, :3] = (torch.rand(3, generator=gen, dtype=torch.float64) - 0.5) * 2 * persp
        A[3, 3] = 1.0
        cf[n, :16] = A.reshape(-1)
    return cf


# ---- the map ---------------------------------------------------------------------------------------------------------------------
def lattice01(S, dtype=torch.float64, misread=None):
    if S == 1:
        return torch.full((1,), 1.0 if misread == 'size1_at_1' else 0.0, dtype=dtype)
    if misread == 'step_1_over_S':
        return torch.arange(S, dtype=dtype) / S
    return torch.linspace(0, 1, S, dtype=dtype)


def basis(dims, dtype=torch.float64, misread=None):
    """The six basis functions (1, a, b, k, a k, b k) of the O2C map on the (D,H,W) lattice, each (D,H,W)."""
    D, H, W = dims
    k, b, a = torch.meshgrid(lattice01(D, dtype, misread), lattice01(H, dtype, misread), lattice01(W, dtype, misread), indexing='ij')
    ak, bk = a * k, b * k
    if misread == 'ak_bk_swapped':
        ak, bk = bk, ak
    return torch.ones_like(a), a, b, k, ak, bk


def grid(cf, kind, dims, misread=None):
    """(N,D,H,W,3) normalised coordinates (x, y, z) in cf's dtype; every product is written out (inf * 0 is NaN, as in the kernel)."""
    B = basis(dims, cf.dtype, misread)
    if kind == O2C:
        c = cf[:, :18].reshape(-1, 6, 3)
        g = 0
        for j in range(6):
            g = g + c[:, j].reshape(-1, 1, 1, 1, 3) * B[j].reshape(1, *dims, 1)
        return g
    _, a, b, k, _, _ = B
    lx, ly, lz = 2 * a - 1, 2 * b - 1, 2 * k - 1
    A = cf[:, :16].reshape(-1, 4, 4)
    r = [A[:, i, 0].reshape(-1, 1, 1, 1) * lx + A[:, i, 1].reshape(-1, 1, 1, 1) * ly + A[:, i, 2].reshape(-1, 1, 1, 1) * lz
         + A[:, i, 3].reshape(-1, 1, 1, 1) for i in range(4)]
    return torch.stack((r[0] / r[3], r[1] / r[3], r[2] / r[3] if misread == 'gz_divided' else r[2]), dim=-1)


def position(g, S, misread=None):
    """One axis: (unclamped p, the position the taps use, d p / d g including the mask)."""
    if misread == 'align_corners':
        p, gain = (g + 1) / 2 * (S - 1), (S - 1) / 2
    elif misread == 'half_voxel':
        p, gain = (g + 1) * S / 2, S / 2
    else:
        p, gain = ((g + 1) * S - 1) / 2, S / 2
    if misread == 'mask_absent' or misread == 'zeros_padding':
        m = torch.ones_like(p)
    elif misread == 'mask_nonstrict':
        m = ((p >= 0) & (p <= S - 1)).to(p.dtype)
    else:
        m = ((p > 0) & (p < S - 1)).to(p.dtype)
    pc = p if misread == 'zeros_padding' else p.clamp(0, S - 1)
    pc = torch.where(pc != pc, torch.zeros_like(pc), pc)
    return p, pc, m * gain


def positions(cf, kind, dims, misread=None):
    """(unclamped, used) positions, (N,D,H,W,3) each, in cf's dtype."""
    D, H, W = dims
    g = grid(cf, kind, dims, misread)
    pp = [position(g[..., c], S, misread) for c, S in enumerate((W, H, D))]
    return torch.stack([p[0] for p in pp], -1), torch.stack([p[1] for p in pp], -1)


# ---- the fp64 restatement ----------------------------------------------------------------------------------------------------------
def reference(vol, cf, kind, dims, gout=None, misread=None):
    """vol (vol_n,D,H,W,C), cf (N,20), gout (N,D,H,W,C) or None -- any float dtype, evaluated in fp64.  Returns a dict of fp64 tensors:
         fwd (N,D,H,W,C); maxcorner (N,D,H,W,C) = largest |corner value| of the element; taps (N,DHW,8) flat corner voxel indices;
       and with gout
         gcoef (N,18), A (N,18) (the absolute-sum yardstick of every coefficient sum);
         gvol (vol_n,D,H,W,C), gvol_abs (same shape: sum of |contributions|), ncontrib (vol_n,D,H,W): taps of non-zero weight."""
    D, H, W = dims
    vol, cf = vol.double(), cf.double()
    N, vol_n, C, nvox = cf.shape[0], vol.shape[0], vol.shape[-1], D * H * W
    g = grid(cf, kind, dims, misread)
    Bs = [b.reshape(-1) for b in basis(dims, torch.float64, misread)]
    zero_pad = misread == 'zeros_padding'
    out = {'fwd': torch.empty(N, nvox, C, dtype=torch.float64), 'maxcorner': torch.empty(N, nvox, C, dtype=torch.float64),
           'taps': torch.empty(N, nvox, 8, dtype=torch.long)}
    if gout is not None:
        gout = gout.double().reshape(N, nvox, C)
        out.update(gcoef=torch.zeros(N, 18, dtype=torch.float64), A=torch.zeros(N, 18, dtype=torch.float64),
                   gvol=torch.zeros(vol_n, nvox, C, dtype=torch.float64), gvol_abs=torch.zeros(vol_n, nvox, C, dtype=torch.float64),
                   ncontrib=torch.zeros(vol_n, nvox, dtype=torch.float64))
    for n in range(N):
        vn = n if vol_n > 1 else 0
        V = vol[vn].reshape(nvox, C)
        i0, i1, w0, w1, dm = [], [], [], [], []
        for c, S in enumerate((W, H, D)):
            _, p, m = position(g[n, ..., c].reshape(-1), S, misread)
            f = p.floor()
            t = p - f
            lo, hi = f.long(), f.long() + 1
            wl, wh = 1 - t, t
            if zero_pad:                                          # corners outside the volume read 0
                wl = wl * ((lo >= 0) & (lo <= S - 1))
                wh = wh * ((hi >= 0) & (hi <= S - 1))
                lo = lo.clamp(0, S - 1)
            hi = hi.clamp(0, S - 1) if zero_pad else hi.clamp(max=S - 1)
            i0.append(lo); i1.append(hi); w0.append(wl); w1.append(wh); dm.append(m)
        ix, iy, iz, wx, wy, wz = (i0[0], i1[0]), (i0[1], i1[1]), (i0[2], i1[2]), (w0[0], w1[0]), (w0[1], w1[1]), (w0[2], w1[2])
        v, w, idx = {}, {}, {}
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    key = (cz, cy, cx)
                    idx[key] = (iz[cz] * H + iy[cy]) * W + ix[cx]
                    v[key] = V[idx[key]]
                    w[key] = wx[cx] * wy[cy] * wz[cz]
        keys = sorted(v)
        out['taps'][n] = torch.stack([idx[k_] for k_ in keys], -1)
        out['fwd'][n] = sum(v[k_] * w[k_][:, None] for k_ in keys)
        out['maxcorner'][n] = torch.stack([v[k_].abs() for k_ in keys]).amax(0)
        if gout is None:
            continue
        go = gout[n]
        # d out / d position along each axis: differences of the corner pairs along it, weighted by the other two axes
        pair_w = {0: lambda cz, cy: wy[cy] * wz[cz], 1: lambda cz, cx: wx[cx] * wz[cz], 2: lambda cy, cx: wx[cx] * wy[cy]}
        for c in range(3):
            d = torch.zeros(nvox, dtype=torch.float64)
            dabs = torch.zeros(nvox, dtype=torch.float64)
            for u in (0, 1):
                for s in (0, 1):
                    if c == 0:
                        hi_, lo_, pw = v[(u, s, 1)], v[(u, s, 0)], pair_w[0](u, s)
                    elif c == 1:
                        hi_, lo_, pw = v[(u, 1, s)], v[(u, 0, s)], pair_w[1](u, s)
                    else:
                        hi_, lo_, pw = v[(1, u, s)], v[(0, u, s)], pair_w[2](u, s)
                    d = d + (go * (hi_ - lo_)).sum(1) * pw
                    dabs = dabs + (go.abs() * (hi_ - lo_).abs()).sum(1) * pw
            # a masked-out axis contributes exactly 0, whatever the (possibly non-finite) derivative is: the kernels multiply by a
            # mask of 0 only finite derivatives in every finite case, and the comparison of non-finite cases is on `fwd`
            h = torch.where(dm[c] != 0, d * dm[c], torch.zeros_like(d))
            habs = torch.where(dm[c] != 0, dabs * dm[c], torch.zeros_like(d))
            for j in range(6):
                out['gcoef'][n, 3 * j + c] = (Bs[j] * h).sum()
                out['A'][n, 3 * j + c] = (Bs[j].abs() * habs).sum()
        for k_ in keys:
            contrib = go * w[k_][:, None]
            out['gvol'][vn].index_add_(0, idx[k_], contrib)
            out['gvol_abs'][vn].index_add_(0, idx[k_], contrib.abs())
            out['ncontrib'][vn].index_add_(0, idx[k_], (w[k_] != 0).double())
    for key in ('fwd', 'maxcorner'):
        out[key] = out[key].reshape(N, D, H, W, C)
    if gout is not None:
        for key in ('gvol', 'gvol_abs'):
            out[key] = out[key].reshape(vol_n, D, H, W, C)
        out['ncontrib'] = out['ncontrib'].reshape(vol_n, D, H, W)
    return out


def grid_sample_restatement(vol, cf, kind, dims, gout=None, dtype=torch.float32):
    """The same operation as the reference project writes it -- the grid in `dtype`, F.grid_sample(bilinear, border,
    align_corners=False), autograd -- channels-last in and out.  fp32: e32 of the bounds and the stand-in for the kernel on a
    machine without a GPU; fp64: what the explicit restatement is checked against.  Returns fwd, and with gout gcoef, gvol."""
    N = cf.shape[0]
    v = vol.to(dtype).permute(0, 4, 1, 2, 3).contiguous().requires_grad_(gout is not None)
    c = cf.to(dtype).clone().requires_grad_(gout is not None)
    g = grid(c, kind, dims)
    o = F.grid_sample(v.expand(N, -1, -1, -1, -1) if v.shape[0] == 1 else v, g, mode='bilinear', padding_mode='border',
                      align_corners=False)
    out = {'fwd': o.detach().permute(0, 2, 3, 4, 1).contiguous()}
    if gout is not None:
        (o * gout.to(dtype).permute(0, 4, 1, 2, 3)).sum().backward()
        out['gcoef'] = c.grad[:, :18].clone()
        out['gvol'] = v.grad.permute(0, 2, 3, 4, 1).contiguous()
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _sixteenths(gen, shape, bound):
    """Seeded integer multiples of 1/16 in [-bound, bound]."""
    m = int(round(bound * 16))
    return torch.randint(-m, m + 1, shape, generator=gen).double() / 16


def clamped_share(cf, kind, dims):
    """Per sample and axis (x, y, z) the share of positions that the border clamp moved (or held on a face), (N,3)."""
    p, _ = positions(cf.double(), kind, dims)
    D, H, W = dims
    hi = torch.tensor([W - 1, H - 1, D - 1], dtype=torch.float64)
    return ((p <= 0) | (p >= hi)).double().mean(dim=(1, 2, 3))


def lattice_coefs(N, kind, dims, gen):
    """(N,20) fp64 coefficient blocks of the lattice family.  O2C: multiples of 1/16, constant and linear terms in +-1.5, a k and
    b k terms in +-0.25.  C2O: rows 0-2 multiples of 1/16 (linear part +-1.5, constant +-0.5), row 3 = (0, 0, 0, d), d in
    {0.5, 1, 2}: the division is exact.  A sample is redrawn until |g + 1| S < 256 everywhere (with it every position is exact in
    fp32) and the border clamp holds 25 .. 75 % of its positions on every axis of size > 1, so that both sides of the mask are
    exercised at every shape (seeded: the draws are part of the case)."""
    D, H, W = dims
    cf = torch.zeros(N, LF_MAP_COEFS, dtype=torch.float64)
    live = torch.tensor([W > 1, H > 1, D > 1])
    for n in range(N):
        for _ in range(10000):
            row = torch.zeros(LF_MAP_COEFS, dtype=torch.float64)
            if kind == O2C:
                row[0:12] = _sixteenths(gen, (12,), 1.5)
                row[12:18] = _sixteenths(gen, (6,), 0.25)
            else:
                A = torch.zeros(4, 4, dtype=torch.float64)
                A[:3, :3] = _sixteenths(gen, (3, 3), 1.5)
                A[:3, 3] = _sixteenths(gen, (3,), 0.5)
                A[3, 3] = (0.5, 1.0, 2.0)[int(torch.randint(0, 3, (1,), generator=gen))]
                row[:16] = A.reshape(-1)
            share = clamped_share(row[None], kind, dims)[0]
            small = ((grid(row[None], kind, dims) + 1).abs() * torch.tensor([W, H, D], dtype=torch.float64) < 256).all()
            if bool(small) and bool(((share[live] >= 0.25) & (share[live] <= 0.75)).all()):
                break
        else:
            raise RuntimeError('no lattice draw with the clamped share asked for')
        cf[n] = row
    return cf


GENERAL_SCALES = [1.0, 0.3, 2.5]


@functools.lru_cache(maxsize=None)
def inputs(family, kind, dims, C, N, vol_n, seed=0):
    """fp32 inputs of one case: vol (vol_n,D,H,W,C), cf (N,20), gout (N,D,H,W,C).  Cached and shared: treat as read-only."""
    D, H, W = dims
    gen = torch.Generator().manual_seed(1000 * seed + 7 * D + 11 * H + 13 * W + 17 * C + 19 * N + 23 * vol_n + kind)
    if family == 'lattice':
        cf = lattice_coefs(N, kind, dims, gen)
    elif family == 'on_face':
        cf = on_face_coefs(N, dims, gen)
    else:
        cf = (o2c_coefs if kind == O2C else c2o_coefs)(N, gen, GENERAL_SCALES)
    vol = smooth_volume(vol_n, dims, C, gen) if family == 'general' else torch.randn(vol_n, D, H, W, C, generator=gen)
    gout = torch.randn(N, D, H, W, C, generator=gen)
    return vol, cf.float(), gout


def smooth_volume(vol_n, dims, C, gen):
    """(vol_n,D,H,W,C) fp32: per channel three plane waves of unit amplitude, wavelengths of 12 voxels and more.
    The general family's positions are rounded in fp32 (about 1e-5 voxel at these sizes and scales).  The trilinear interpolant of
    white noise has a slope of O(1) per voxel that jumps by O(1) at every cell boundary: there a position within rounding of a
    boundary takes the other cell's slope, and ONE such tap moves a coefficient sum over 32^3 voxels by 3.5e-3 of its largest
    component (measured: kernel 3.5e-3, fp32 torch 1e-8 on one draw) -- the 2e-3 bound would record the draw, not the
    kernel.  On a band-limited volume the slope and its jumps are an order of magnitude smaller, position rounding stays far
    below every bound, and a wrong tap, weight or voxel still costs O(0.1) per element.  (White noise with exact positions:
    the lattice family.)"""
    D, H, W = dims
    z, y, x = torch.meshgrid(torch.arange(D, dtype=torch.float64), torch.arange(H, dtype=torch.float64),
                             torch.arange(W, dtype=torch.float64), indexing='ij')
    vol = torch.zeros(vol_n, D, H, W, C, dtype=torch.float64)
    for _ in range(3):
        kvec = torch.randn(vol_n, C, 3, generator=gen, dtype=torch.float64)
        kvec = kvec / kvec.norm(dim=-1, keepdim=True) * (2 * torch.pi / (12 + 12 * torch.rand(vol_n, C, 1, generator=gen, dtype=torch.float64)))
        phase = 2 * torch.pi * torch.rand(vol_n, C, generator=gen, dtype=torch.float64)
        arg = (kvec[..., 0].reshape(vol_n, 1, 1, 1, C) * x[None, ..., None] + kvec[..., 1].reshape(vol_n, 1, 1, 1, C) * y[None, ..., None]
               + kvec[..., 2].reshape(vol_n, 1, 1, 1, C) * z[None, ..., None] + phase.reshape(vol_n, 1, 1, 1, C))
        vol = vol + torch.sin(arg)
    return vol.float()


@functools.lru_cache(maxsize=None)
def case(family, kind, dims, C, N, vol_n, seed=0, with_gout=True):
    """inputs + the fp64 restatement (`ref`) + the fp32 restatement (`r32`) of one case, computed once per process."""
    vol, cf, gout = inputs(family, kind, dims, C, N, vol_n, seed)
    return {'vol': vol, 'cf': cf, 'gout': gout, 'ref': reference(vol, cf, kind, dims, gout if with_gout else None),
            'r32': grid_sample_restatement(vol, cf, kind, dims, gout if with_gout else None)}


NV = [(1, 1), (3, 1), (3, 3)]                                     # (N, vol_n) of every case of the matrix

BASE = (5, 9, 17)
SIZE1_SHAPES = [(1, 5, 9), (5, 1, 9), (5, 9, 1), (1, 1, 1)]
LATTICE_SHAPES = [BASE, (17, 33, 9), (3, 2, 65), (33, 33, 33)] + SIZE1_SHAPES
GENERAL_SHAPES = [(16, 16, 16), (32, 32, 32), (9, 21, 13)]

# forward: (lf_set_tuning(1, .), C) -> the kernel form of csrc/resample.hip's dispatch that the call reaches
FWD_FORMS = [
    (3, 1, 'resample_fwd_kernel<KIND,1>'), (3, 3, 'resample_fwd_kernel<KIND,1>'), (3, 6, 'resample_fwd_kernel<KIND,1>'),
    (3, 4, 'resample_fwd_lean_kernel'), (3, 20, 'resample_fwd_lean_kernel'), (3, 64, 'resample_fwd_lean_kernel'),
    (3, 256, 'resample_fwd_lean_kernel'), (3, 16, 'resample_fwd_c16_kernel'),
    (3, 257, 'resample_fwd_kernel<KIND,1>, lpt = 256, two trips of the channel loop'),
    (1, 4, 'resample_fwd_kernel<KIND,4>'), (1, 16, 'resample_fwd_kernel<KIND,4>'), (1, 20, 'resample_fwd_kernel<KIND,4>'),
    (1, 3, 'resample_fwd_kernel<KIND,1>'), (2, 16, 'resample_fwd_lean_kernel'),
    (4, 16, 'resample_fwd_staged_kernel'), (5, 16, 'resample_fwd_c16_dedup_kernel'),
]
# coefficient gradient at BASE: C -> form
COEF_FORMS = [(1, 'resample_bwd_coef_kernel<1>'), (3, 'resample_bwd_coef_kernel<1>, lpv = 4, one lane idle'),
              (6, 'resample_bwd_coef_kernel<1>, lpv = 8, two lanes idle'), (4, 'resample_bwd_coef_kernel<4>'),
              (20, 'resample_bwd_coef_kernel<4>, lpv = 8, three lanes idle'), (256, 'resample_bwd_coef_kernel<4>, lpv = 64'),
              (16, 'resample_bwd_coef_c16_kernel<8,1>')]
# the voxels-per-block switch at C = 16: (dims, N, vol_n, voxels per block, form)
VPB_CASES = [((17, 17, 17), 1, 1, 64, 'resample_bwd_coef_c16_kernel<8,1>'),
             ((33, 33, 33), 8, 1, 128, 'resample_bwd_coef_c16_kernel<8,1>'),
             ((33, 33, 33), 16, 1, 256, 'resample_bwd_coef_c16_dedup_kernel<2,1,true>')]


def bwd_vox_per_block(nvox, N):
    """Restates bwd_vox_per_block of csrc/resample.hip: 64 .. 4096 voxels per block, the largest power of two with
    2048 blocks' worth of voxels still there."""
    v = nvox * N // 2048
    p = 64
    while p < 4096 and p * 2 <= v:
        p *= 2
    return p


# ---- bounds ------------------------------------------------------------------------------------------------------------------------
def _ratio(got, want, bound):
    """max |got - want| / bound over the elements (0 / 0 = 0, x / 0 = inf); inf where the non-finite patterns differ."""
    got, want = got.double(), want.double()
    fin = torch.isfinite(want)
    if not torch.equal(torch.isfinite(got), fin) or not torch.equal(torch.isnan(got), torch.isnan(want)):
        return float('inf')
    if not torch.equal(got[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)]):
        return float('inf')
    if not bool(fin.any()):
        return 0.0
    err, bound = (got - want).abs()[fin], bound.expand_as(want)[fin]
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)            # x / 0 = inf for x > 0
    return float(r.max())


def fwd_ratio(got, ref, family, r32=None):
    """Forward.  lattice: per element 12 * 2^-24 * max|corner value| -- the positions are exact, the three weight pairs, the eight
    products and the seven additions of quantities no larger than the largest corner are at most ten roundings, two to spare.
    general: max(4 e32, 2e-6 + 2e-5 |fp64|) per element, e32 = the fp32 restatement's largest error over the sample.  (Not its
    error at the same element: kernel and restatement round the position on their own -- different operation orders, contraction --
    so at an element the two errors are independent draws of slope x position rounding, and the one the restatement drew there
    says nothing about the kernel's; measured with e32 per element: up to 2.8 x the bound on white noise.  What the restatement
    does measure is the size of that rounding for the sample's map, its largest error.)"""
    want = ref['fwd']
    if family != 'general':
        bound = 12 * U * ref['maxcorner']
    else:
        e32 = (r32['fwd'].double() - want).abs().amax(dim=(1, 2, 3, 4), keepdim=True)
        bound = torch.maximum(4 * e32, 2e-6 + 2e-5 * want.abs())
    return _ratio(got, want, bound)


def gvol_ratio(got, ref, family, r32=None, quantum=0.0):
    """Volume gradient.  lattice: (12 + n) * 2^-24 * sum|contributions| per element, n = the number of contributions the voxel
    receives (fp32 atomics add them in any order: (n - 1) u sum|terms| is the summation bound); `quantum` = 2^-38 max|gout| for
    the fixed-point form: it rounds every contribution to a multiple of 2^(e - 38), 2^(e - 1) <= max|gout| < 2^e (fixed_scale of
    csrc/splat.hip; include/lf_hip.h), so by at most half of that, which is at most 2^-38 max|gout| -> + n * quantum.
    general: max(4 e32, 2e-6 + 2e-5 sum|contributions|), e32 = the fp32 restatement's largest error over the volume (as in
    fwd_ratio)."""
    want = ref['gvol']
    if family != 'general':
        n = ref['ncontrib'][..., None]
        bound = (12 + n) * U * ref['gvol_abs'] + n * quantum
    else:
        e32 = (r32['gvol'].double() - want).abs().amax(dim=(1, 2, 3, 4), keepdim=True)
        bound = torch.maximum(4 * e32, 2e-6 + 2e-5 * ref['gvol_abs'])
    return _ratio(got, want, bound)


def gcoef_ratio(got, ref, family, r32, e32_ref=None):
    """Coefficient gradient.  lattice: per coefficient max(4 e32_j, 2e-5 A_j).  general: per sample, the largest error against
    max(4 max e32, 2e-3 of the largest component).  e32 is the fp32 restatement's distance from the TRUE fp64 value (`e32_ref`,
    default `ref`): a property of the inputs, also when `ref` is a misreading."""
    want = ref['gcoef']
    e32 = (r32['gcoef'].double() - (e32_ref or ref)['gcoef']).abs()
    if family != 'general':
        return _ratio(got, want, torch.maximum(4 * e32, 2e-5 * ref['A']))
    err = (got.double() - want).abs().amax(1)
    if not bool(torch.isfinite(got).all()):
        return float('inf')
    bound = torch.maximum(4 * e32.amax(1), 2e-3 * want.abs().amax(1))
    return float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())


# ---- degenerate and non-finite maps (C ABI semantics from the header; compared within the lattice bounds) -------------------------
def degenerate_coefs(name, dims=BASE):
    """(kind, (N,20) fp32 block).  Every finite coefficient is a multiple of 1/16 (positions exact, as in the lattice family)."""
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == 'nan':                                             # a NaN coefficient: every tap of that axis reads voxel 0, mask 0
        cf = lattice_coefs(3, O2C, dims, gen)
        cf[0, 0] = float('nan')                                   # constant term, x
        cf[1, 7] = float('nan')                                   # b term, y: 0 * NaN is NaN, the whole axis
        cf[2, 14] = float('nan')                                  # a k term, z
        return O2C, cf.float()
    if name == 'inf':                                             # +inf -> far face, -inf -> near face, inf * 0 -> NaN -> voxel 0
        cf = lattice_coefs(3, O2C, dims, gen)
        cf[0, 0] = float('inf')
        cf[1, 1] = float('-inf')
        cf[2, 5] = float('inf')                                   # a term, z: NaN on the a = 0 plane, far face elsewhere
        return O2C, cf.float()
    if name == 'behind_camera':                                   # the denominator crosses zero inside the volume: +-inf and 0/0
        cf = lattice_coefs(3, C2O, dims, gen)
        # dn = lz takes -1, -0.5, 0, 0.5, 1 on the five planes of BASE: powers of two, the divisions stay exact
        cf[:, 12:16] = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64)
        cf[0, 0:4] = torch.tensor([1.0, 0.0, 0.5, 0.0], dtype=torch.float64)       # n0 = lx on the dn = 0 plane: 0/0 at its centre
        return C2O, cf.float()
    if name == 'far_outside':                                     # shifted by 7: clamped corner values, gradient exactly 0
        cf = lattice_coefs(3, O2C, dims, gen)
        cf[:, 0:3] += torch.tensor([7.0, -7.0, 7.0], dtype=torch.float64)
        return O2C, cf.float()
    if name == 'constant':                                        # every voxel of a sample reads the same position
        cf = lattice_coefs(3, O2C, dims, gen)
        cf[:, 3:18] = 0.0
        cf[:, 0:3] = _sixteenths(gen, (3, 3), 0.75)
        return O2C, cf.float()
    raise KeyError(name)


DEGENERATE = ('nan', 'inf', 'behind_camera', 'far_outside', 'constant')


def on_face_coefs(N, dims, gen):
    """O2C lattice blocks whose y position lies exactly ON a face for every voxel (H = 2: g_y = -0.5 -> p = 0, g_y = 0.5 ->
    p = 1 = H - 1): the strict mask gives 0 there, a non-strict one the full slope."""
    assert dims[1] == 2
    cf = lattice_coefs(N, O2C, dims, gen)
    for n in range(N):
        cf[n, 1:18:3] = 0.0
        cf[n, 1] = -0.5 if n % 2 == 0 else 0.5
    return cf


@functools.lru_cache(maxsize=None)
def degenerate_case(name, C, dims=BASE):
    """One shared volume, three samples.  e32 is not used here (`r32` = the reference: F.grid_sample is not asked about NaNs)."""
    kind, cf = degenerate_coefs(name, dims)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + C)
    vol = torch.randn(1, *dims, C, generator=gen)
    gout = torch.randn(3, *dims, C, generator=gen)
    ref = reference(vol, cf, kind, dims, gout)
    return {'kind': kind, 'vol': vol, 'cf': cf, 'gout': gout, 'ref': ref, 'r32': ref}


def finite_cases():
    """Every (family, kind, dims, C, N, vol_n) that tests/test_resample_fp64_gpu.py runs through `case` -- the CPU module checks the
    restatement, the exact positions and the clamped share on each of them."""
    keys = []
    for kind in (O2C, C2O):
        for N, vol_n in NV:
            for C in sorted({c for _, c, _ in FWD_FORMS} | {1, 3, 16, 20}):
                keys.append(('lattice', kind, BASE, C, N, vol_n))
            for dims in LATTICE_SHAPES[1:]:
                for C in (16, 3):
                    keys.append(('lattice', kind, dims, C, N, vol_n))
            for C in (1, 3, 16, 20):
                keys.append(('lattice', kind, SIZE1_SHAPES[0], C, N, vol_n))
            for dims in GENERAL_SHAPES:
                for C in (16, 3):
                    keys.append(('general', kind, dims, C, N, vol_n))
    for N, vol_n in NV:
        keys.append(('lattice', O2C, BASE, 64, N, vol_n))
        keys.append(('on_face', O2C, (3, 2, 65), 16, N, vol_n))
    for dims, N, vol_n, _, _ in VPB_CASES:
        keys.append(('lattice', O2C, dims, 16, N, vol_n))
    return sorted(set(keys))


# misreading -> (output compared, the case that exposes it)
MISREAD_CASES = {
    'align_corners': ('fwd', ('lattice', O2C, BASE, 16, 3, 1)),
    'zeros_padding': ('fwd', ('lattice', O2C, BASE, 16, 3, 1)),
    'step_1_over_S': ('fwd', ('lattice', O2C, BASE, 16, 3, 1)),
    'ak_bk_swapped': ('fwd', ('lattice', O2C, BASE, 16, 3, 1)),
    'gz_divided': ('fwd', ('lattice', C2O, BASE, 16, 3, 1)),
    'half_voxel': ('fwd', ('lattice', C2O, BASE, 16, 3, 1)),
    'mask_nonstrict': ('gcoef', ('on_face', O2C, (3, 2, 65), 16, 3, 1)),
    'mask_absent': ('gcoef', ('lattice', O2C, BASE, 16, 3, 1)),
    'size1_at_1': ('fwd', ('lattice', O2C, (1, 5, 9), 16, 3, 1)),
}


@functools.lru_cache(maxsize=None)
def misread_reference(name):
    out, key = MISREAD_CASES[name]
    vol, cf, gout = inputs(*key)
    return reference(vol, cf, key[1], key[2], gout if out == 'gcoef' else None, misread=name)


def misread_ratio(name, got):
    """How far `got` (the kernel's output on the misreading's case) is from the misread reference, in units of the bound that
    accepts it against the true one."""
    out, key = MISREAD_CASES[name]
    c = case(*key)
    wrong = misread_reference(name)
    if out == 'fwd':
        return fwd_ratio(got, wrong, key[0])
    return gcoef_ratio(got, wrong, key[0], c['r32'], e32_ref=c['ref'])
