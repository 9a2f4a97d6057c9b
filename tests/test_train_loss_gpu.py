"""The fused training losses on the GPU: lf_recon_loss_fwd / lf_recon_loss_bwd (csrc/train_loss.hip) against torch and fp64, and
the options that reach them (losses.HardPixelLoss `kernel`, GeneratorStep `loss_kernel`).

YARDSTICKS.  Hard-pixel part: per-pixel loss = F.l1_loss / F.smooth_l1_loss(reduction='none').mean(dim=1), the k largest of every
image by torch.topk, their mean; in fp32 on the CPU (the selection, and for C = 1 the threshold bit for bit) and in fp64 (the
values).  Mask part: max(z, 0) - z t + log1p(exp(-|z|)) and the clamped Beta prior on sigmoid(z), in fp64, gradients by fp64
autograd.  BOUND, forward and per element of the gradient: |kernel - fp64| <= max(4 e32, 2e-6 + 2e-5 |fp64|), e32 = the distance
of the same torch expressions in fp32 from fp64.  So that the bound bites on the gradients the upstream gradient of a term is
the term's own denominator (B * k, Mn): the elements are then base' / C and (m - t), of order 1, not of order 1e-5.

INPUTS of the hard-pixel cases: one CPU generator seeded 1000 B + 10 C + H, first x = 1.5 tanh(randn), then y = tanh(randn)
(about 40 % of the elements on smooth-L1's linear branch).  The relative gap between the k-th and (k+1)-th largest per-pixel loss
of every image is asserted to exceed 1e-5, so the comparison with torch.topk's selection is never a tie lottery; ties are
tested as properties on built images instead.

The Beta prior's gradient jumps where a clamp switches (m or 1 - m at 1e-4, the negated log-density at 0); an element whose
fp64 value lies within 1e-3 (relative, inner clamps) or 1e-4 (absolute, outer clamp) of a switch may fall on either side in fp32
and is left out of the GRADIENT comparison (its loss value is continuous and stays in); at most one element per thousand, counted.

MEASURED (MI355X): see the `[train_loss]` lines this file prints and COVERAGE.md row f4."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BASES = ('l1', 'smooth_l1')
CASES = [(1, 1, 5, 7, (1, 17, 35)), (3, 1, 33, 65, (1, 500, 2144, 2145)), (7, 1, 97, 131, (3000,)),
         (2, 1, 128, 128, (4096, 16384)), (2, 3, 33, 65, (500,)), (3, 4, 5, 7, (17,))]
SENT = -7.5


# ---- inputs and references (CPU) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(B, C, H, W):
    gen = torch.Generator().manual_seed(1000 * B + 10 * C + H)
    x = 1.5 * torch.tanh(torch.randn(B, C, H, W, generator=gen))
    y = torch.tanh(torch.randn(B, C, H, W, generator=gen))
    return x, y


def per_pixel(x, y, base, dtype=torch.float32, branch=1.0):
    """(B, H*W) per-pixel loss of the torch expressions in `dtype` (branch: smooth-L1's beta, 1 everywhere but in a misreading)."""
    x, y = x.to(dtype), y.to(dtype)
    l = F.l1_loss(x, y, reduction='none') if base == 'l1' else F.smooth_l1_loss(x, y, reduction='none', beta=branch)
    return l.mean(dim=1).reshape(x.shape[0], -1)


def ref_hard(x, y, base, k, dtype, idx=None, g0=1.0):
    """(term, d(g0 * term)/dx, indices of the selection) in `dtype`; idx: a given selection instead of this precision's top-k."""
    xr = x.to(dtype).clone().requires_grad_(True)
    l = per_pixel(xr, y, base, dtype)
    if k == 0:
        term = l.mean()
    else:
        if idx is None:
            idx = torch.topk(l.detach(), k, dim=1).indices
        term = l.gather(1, idx).mean()
    g, = torch.autograd.grad(term * g0, xr)
    return term.detach(), g, idx


def excess(got, ref64, ref32):
    """(max of |got - fp64| - bound, max error, max e32) over the elements; <= 0 passes, a NaN counts as +inf."""
    got, ref64, ref32 = got.double().cpu(), ref64.double(), ref32.double()
    err, e32 = (got - ref64).abs(), (ref32 - ref64).abs()
    ex = err - torch.maximum(4 * e32, 2e-6 + 2e-5 * ref64.abs())
    return float(torch.nan_to_num(ex, nan=float('inf')).max()), float(err.max()), float(e32.max())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run_hard(x, y, base, k, g0=1.0):
    """terms (3,), gx, and the forward's side outputs of the kernels, on the CPU."""
    from latentfusion_amd import ops
    xd, yd = x.to(DEV).requires_grad_(True), y.to(DEV)
    terms = ops.recon_losses(xd, yd, base, k)
    (terms[0] * g0).backward()
    aux = ops.recon_losses_fwd(xd.detach(), yd, base, k)
    assert same_bits(aux['terms'][:3], terms.detach())
    return terms.detach().cpu(), xd.grad.cpu(), {n: v.cpu() for n, v in aux.items()}


def min_gap(l32, k):
    s = l32.sort(dim=1, descending=True).values
    return float(((s[:, k - 1] - s[:, k]) / s[:, k - 1]).min())


# ---- 1. against torch and fp64 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,H,W,ks', CASES)
def test_hard_pixel_terms_and_gradients_vs_torch_and_fp64(B, C, H, W, ks):
    x, y = inputs(B, C, H, W)
    HW = H * W
    for base in BASES:
        l32 = per_pixel(x, y, base)
        for k in ks + (0,):
            if 0 < k < HW:
                gap = min_gap(l32, k)
                assert gap > 1e-5, (base, k, gap)                                 # the tie condition of the inputs
            n = k if k > 0 else HW
            g0 = float(B * n)
            idx32 = torch.topk(l32, k, dim=1).indices if k > 0 else None
            t64, _, _ = ref_hard(x, y, base, k, torch.float64)
            _, g64, _ = ref_hard(x, y, base, k, torch.float64, idx32, g0)
            t32, g32, _ = ref_hard(x, y, base, k, torch.float32, idx32, g0)
            terms, gx, aux = run_hard(x, y, base, k, g0)
            ex_t, err_t, e32_t = excess(terms[0], t64, t32)
            ex_g, err_g, e32_g = excess(gx, g64, g32)
            l64 = per_pixel(x, y, base, torch.float64)
            s64 = torch.topk(l64, n, dim=1).values.sum(1)
            s32 = torch.topk(l32, n, dim=1).values.sum(1)
            ex_s, err_s, e32_s = excess(aux['img_sum'], s64, s32)
            print(f'[train_loss] hard {B}x{C}x{H}x{W} {base} k={k}: term err {err_t:.2e} (e32 {e32_t:.2e}), img_sum err {err_s:.2e} '
                  f'(e32 {e32_s:.2e}), gx err {err_g:.2e} (e32 {e32_g:.2e})')
            assert ex_t <= 0 and ex_s <= 0 and ex_g <= 0, (base, k, ex_t, ex_s, ex_g)
            assert float(terms[1]) == 0.0 and float(terms[2]) == 0.0             # the absent part
            if k == 0:
                assert torch.equal(aux['sel'], torch.tensor([[HW, 0]] * B, dtype=torch.int32))
                continue
            keep = torch.zeros(B, HW, dtype=torch.bool).scatter_(1, idx32, True)
            g = gx.reshape(B, C, HW)
            assert bool((g[~keep[:, None, :].expand(B, C, HW)] == 0).all()), (base, k)        # exactly 0 outside the selection
            assert int((g != 0).sum(dim=(1, 2)).max()) <= k * C
            assert bool((aux['sel'].sum(1) == k).all()) and bool((aux['sel'][:, 1] >= 1).all())
            if C == 1:                                                           # bit for bit torch's threshold and its counts
                want = torch.topk(l32, k, dim=1).values[:, -1]
                assert torch.equal(aux['thresh'], want), (base, k)
                n_gt = (l32 > want[:, None]).sum(1).to(torch.int32)
                assert torch.equal(aux['sel'][:, 0], n_gt) and torch.equal(aux['sel'][:, 1], k - n_gt)


# ---- 2. the mask part against fp64 ----------------------------------------------------------------------------------------------
def mask_inputs(Mn, soft, with_inf=False):
    gen = torch.Generator().manual_seed(77 + Mn)
    z = torch.randn(Mn, generator=gen) * 4
    special = [0.0, 17.0, -17.0, 80.0, -80.0] + ([float('inf'), -float('inf')] * 2 if with_inf else [])
    n = min(len(special), Mn)
    z[:n] = torch.tensor(special[:n])
    t = torch.rand(Mn, generator=gen)
    return z, t if soft else (t > 0.5).float()


def ref_mask(z, t, bp, dtype, g=(1.0, 1.0)):
    """(bce, beta, d(g[0] bce + g[1] beta)/dz, mask of the elements near a switch of a clamp) of the restated expressions."""
    zr, tt = z.to(dtype).clone().requires_grad_(True), t.to(dtype)
    bce = (zr.clamp(min=0) - zr * tt + torch.log1p(torch.exp(-zr.abs()))).mean()
    m = torch.sigmoid(zr)
    lb = 2 * math.lgamma(bp) - math.lgamma(2 * bp)
    nv = -((bp - 1.0) * torch.log(m.clamp(min=1e-4)) + (bp - 1.0) * torch.log((1.0 - m).clamp(min=1e-4)) - lb)
    beta = nv.clamp(min=0).mean()
    # the gradient of the BCE term is that of the smooth function, sigmoid(z) - t: autograd through max(z, 0) and |z| would
    # return their subgradients at z = 0 exactly (1 - t instead of 0.5 - t), so it goes through torch's own node
    gz, = torch.autograd.grad(g[0] * F.binary_cross_entropy_with_logits(zr, tt) + g[1] * beta, zr)
    md = m.detach()
    near = ((md - 1e-4).abs() < 1e-7) | ((1.0 - md - 1e-4).abs() < 1e-7) | (nv.detach().abs() < 1e-4)
    return bce.detach(), beta.detach(), gz, near


def composed_mask(z, t, bp, g=(1.0, 1.0)):
    """Today's fp32 path: BCEWithLogitsLoss and losses.beta_prior_loss on sigmoid(z)."""
    from latentfusion_amd import losses
    zr = z.clone().requires_grad_(True)
    bce = F.binary_cross_entropy_with_logits(zr, t)
    beta = losses.beta_prior_loss(torch.sigmoid(zr), alpha=bp, beta=bp)
    gz, = torch.autograd.grad(g[0] * bce + g[1] * beta, zr)
    return bce.detach(), beta.detach(), gz


def run_mask(z, t, bp, g):
    from latentfusion_amd import ops
    zd = z.to(DEV).requires_grad_(True)
    terms = ops.recon_losses(None, None, 'l1', 0, zd, t.to(DEV), bp)
    (g[0] * terms[1] + g[1] * terms[2]).backward()
    return terms.detach().cpu(), zd.grad.cpu()


def same_nonfinite(a, b):
    a, b = a.double().cpu(), b.double()
    return all(torch.equal(f(a), f(b)) for f in (torch.isnan, torch.isposinf, torch.isneginf))


@pytest.mark.parametrize('Mn', [1, 63, 4097, 8 * 128 * 128])
def test_mask_terms_and_gradients_vs_fp64(Mn):
    for bp in (0.01, 2.0):
        for soft in (False, True):
            z, t = mask_inputs(Mn, soft)
            clamped = unclamped = 0
            for gw in ((1.0, 0.0), (0.0, 1.0), (1.0, 0.5)):
                g = (gw[0] * Mn, gw[1] * Mn)
                bce64, beta64, g64, near = ref_mask(z, t, bp, torch.float64, g)
                bce32, beta32, g32 = composed_mask(z, t, bp, g)
                terms, gz = run_mask(z, t, bp, g)
                assert float(terms[0]) == 0.0 and int(near.sum()) <= max(1, Mn // 1000), int(near.sum())
                ex_a, err_a, e32_a = excess(terms[1], bce64, bce32)
                ex_b, err_b, e32_b = excess(terms[2], beta64, beta32)
                ex_g, err_g, e32_g = excess(gz[~near], g64[~near], g32[~near])
                print(f'[train_loss] mask Mn={Mn} beta_param={bp} soft={soft} g={gw}: bce err {err_a:.2e} (e32 {e32_a:.2e}), beta err '
                      f'{err_b:.2e} (e32 {e32_b:.2e}), gmlogit err {err_g:.2e} (e32 {e32_g:.2e}), left out {int(near.sum())}')
                assert ex_a <= 0 and ex_b <= 0 and ex_g <= 0, (bp, soft, gw, ex_a, ex_b, ex_g)
                assert bool(torch.isfinite(gz).all())
            m = torch.sigmoid(z.double())
            nv = -((bp - 1.0) * (torch.log(m.clamp(min=1e-4)) + torch.log((1 - m).clamp(min=1e-4))) - (2 * math.lgamma(bp) - math.lgamma(2 * bp)))
            clamped, unclamped = int((nv < 0).sum()), int((nv > 0).sum())
            if Mn >= 63:
                assert clamped > 0 and unclamped > 0, (bp, clamped, unclamped)   # both branches of the outer clamp occur


@pytest.mark.parametrize('Mn', [63, 4097])
def test_mask_nonfinite_pattern_is_that_of_the_fp32_expressions(Mn):
    for bp in (0.01, 2.0):
        for soft in (False, True):
            z, t = mask_inputs(Mn, soft, with_inf=True)
            assert int(torch.isinf(z).sum()) == 4
            g = (float(Mn), 0.5 * Mn)
            bce32, beta32, g32, _ = ref_mask(z, t, bp, torch.float32, g)        # the same expressions, in fp32
            _, beta64, g64, near = ref_mask(z, t, bp, torch.float64, g)
            terms, gz = run_mask(z, t, bp, g)
            assert not math.isfinite(float(bce32))
            assert same_nonfinite(terms[1], bce32) and same_nonfinite(terms[2], beta32) and same_nonfinite(gz, g32), (bp, soft)
            fin = torch.isfinite(g64) & ~near
            assert int(fin.sum()) >= Mn - 5
            assert excess(terms[2], beta64, beta32)[0] <= 0 and excess(gz[fin], g64[fin], g32[fin])[0] <= 0


# ---- 3. misreadings are rejected ------------------------------------------------------------------------------------------------
def test_misreadings_fail_the_bound_the_kernel_passes():
    B, C, H, W = 3, 1, 33, 65
    k, HW = 500, 33 * 65
    x, y = inputs(B, C, H, W)
    base = 'smooth_l1'
    g0 = float(B * k)
    l32, l64 = per_pixel(x, y, base), per_pixel(x, y, base, torch.float64)
    idx32 = torch.topk(l32, k, dim=1).indices
    t64, _, _ = ref_hard(x, y, base, k, torch.float64)
    _, g64, _ = ref_hard(x, y, base, k, torch.float64, idx32, g0)
    t32, g32, _ = ref_hard(x, y, base, k, torch.float32, idx32, g0)
    terms, gx, _ = run_hard(x, y, base, k, g0)
    assert excess(terms[0], t64, t32)[0] <= 0 and excess(gx, g64, g32)[0] <= 0
    wrong_terms = {
        'top-k over the whole batch': torch.topk(l64.reshape(-1), B * k).values.mean(),
        'the k smallest': torch.topk(l64, k, dim=1, largest=False).values.mean(),
        'mean over H*W instead of k': torch.topk(l64, k, dim=1).values.sum() / (B * HW),
        'L1 where smooth-L1 was asked': torch.topk(per_pixel(x, y, 'l1', torch.float64), k, dim=1).values.mean(),
        'smooth-L1 with the branch at 0.5': torch.topk(per_pixel(x, y, base, torch.float64, branch=0.5), k, dim=1).values.mean(),
    }
    for name, w in wrong_terms.items():
        assert excess(terms[0], w, w)[0] > 0, name                               # (e32 = 0: the fixed member of the bound alone)
    assert excess(gx, g64 * (k / HW), g64 * (k / HW))[0] > 0, 'gradient divided by B*H*W'


# ---- 4. ties, as properties -----------------------------------------------------------------------------------------------------
def plateau_image(H, W, n_above, n_plateau, d_plateau, seed):
    """x (y = 0): n_above pixels with distinct |d| in (2.5, 3.5), n_plateau pixels with |d| = d_plateau exactly, the rest with
    distinct 0 < |d| < d_plateau (none when the plateau is at 0), at random places, random signs.  -> x, the plateau's indices."""
    gen = torch.Generator().manual_seed(seed)
    HW = H * W
    perm = torch.randperm(HW, generator=gen)
    d = torch.empty(HW)
    d[perm[:n_above]] = 2.5 + torch.rand(n_above, generator=gen)
    d[perm[n_above:n_above + n_plateau]] = d_plateau
    rest = HW - n_above - n_plateau
    d[perm[n_above + n_plateau:]] = (0.05 + 0.9 * torch.rand(rest, generator=gen)) * (d_plateau if d_plateau > 0 else 1.0)
    sign = torch.where(torch.rand(HW, generator=gen) < 0.5, -1.0, 1.0)
    return (d * sign).reshape(1, 1, H, W), perm[n_above:n_above + n_plateau].sort().values


@pytest.mark.parametrize('d_plateau', [2.0, 0.0])
def test_ties_keep_the_lowest_indices_and_repeat_bit_for_bit(d_plateau):
    H, W = 70, 70                                                                # 4900 pixels: two rounds of the backward's walk
    n_above, n_plateau = (300, 900) if d_plateau > 0 else (1500, 3400)           # (a plateau at 0 has nothing below it)
    xs, plats = zip(*(plateau_image(H, W, n_above, n_plateau, d_plateau, 31 + b) for b in range(2)))
    x, y = torch.cat(xs), torch.zeros(2, 1, H, W)
    for base in BASES:
        for n_tie in (1, 411, n_plateau):
            k = n_above + n_tie
            l32 = per_pixel(x, y, base)
            assert bool(((l32 > l32[0, plats[0][0]]).sum(1) == n_above).all())
            t64, _, _ = ref_hard(x, y, base, k, torch.float64)
            t32, _, _ = ref_hard(x, y, base, k, torch.float32)
            terms, gx, aux = run_hard(x, y, base, k, float(2 * k))
            terms2, gx2, aux2 = run_hard(x, y, base, k, float(2 * k))
            assert excess(terms[0], t64, t32)[0] <= 0                            # the value is torch's whatever the choice among the ties
            assert torch.equal(aux['thresh'], torch.topk(l32, k, dim=1).values[:, -1])
            assert torch.equal(aux['sel'], torch.tensor([[n_above, n_tie]] * 2, dtype=torch.int32))
            assert torch.equal(terms, terms2) and torch.equal(gx, gx2) and all(torch.equal(aux[n], aux2[n]) for n in aux)
            nz = gx.reshape(2, -1) != 0
            for b in range(2):
                above = l32[b] > aux['thresh'][b]
                assert bool(nz[b][above].all())                                  # everything above the threshold is kept
                if d_plateau > 0:
                    want = torch.zeros(H * W, dtype=torch.bool)
                    want[plats[b][:n_tie]] = True                                # the n_tie plateau pixels of lowest index
                    assert torch.equal(nz[b] & ~above, want), (base, n_tie, b)
                    xb = x[b].reshape(-1)
                    # base' = sign at d = 2 under both bases; 2k * fl(1 / 2k) is 1 to an ulp
                    torch.testing.assert_close(gx[b].reshape(-1)[want], torch.sign(xb[want]), rtol=2e-7, atol=0)
                else:
                    assert torch.equal(nz[b], above)                             # ties at loss 0 carry a zero gradient


# ---- 5. independence ------------------------------------------------------------------------------------------------------------
def test_an_image_does_not_depend_on_its_batch():
    x7, y7 = inputs(7, 1, 97, 131)
    k = 3000
    for base in BASES:
        for B in (4, 2, 1):
            x, y = x7[:B].contiguous(), y7[:B].contiguous()
            terms, gx, aux = run_hard(x, y, base, k)
            for b in range(B):
                t1, g1, a1 = run_hard(x[b:b + 1], y[b:b + 1], base, k)
                assert all(torch.equal(aux[n][b:b + 1], a1[n]) for n in ('thresh', 'sel', 'img_sum')), (base, B, b)
                assert torch.equal(gx[b:b + 1] * B, g1), (base, B, b)           # 1 / B is exact for a power of two
        # three channels, an odd batch: the side outputs again, the gradient through its one rounding of 1 / (B k C)
        x, y = inputs(2, 3, 33, 65)
        x, y = torch.cat((x, x[:1] * 0.5)), torch.cat((y, y[:1]))
        terms, gx, aux = run_hard(x, y, base, 500)
        for b in range(3):
            t1, g1, a1 = run_hard(x[b:b + 1], y[b:b + 1], base, 500)
            assert all(torch.equal(aux[n][b:b + 1], a1[n]) for n in ('thresh', 'sel', 'img_sum'))
            assert torch.equal(gx[b:b + 1] != 0, g1 != 0)
            torch.testing.assert_close(gx[b:b + 1] * 3, g1, rtol=4e-7, atol=0)


def test_a_nan_stays_in_its_image():
    x, y = (t.clone() for t in inputs(3, 1, 33, 65))
    k = 500
    for base in BASES:
        _, _, clean = run_hard(x, y, base, k)
        xn = x.clone()
        xn[1, 0, 5, 5] = float('nan')
        terms, gx, aux = run_hard(xn, y, base, k)
        assert math.isnan(float(terms[0])) and math.isnan(float(aux['img_sum'][1]))
        for b in (0, 2):
            assert all(torch.equal(aux[n][b], clean[n][b]) for n in ('thresh', 'sel', 'img_sum')), (base, b)
        assert int(aux['sel'][1, 0]) == k - 1 and int(aux['sel'][1, 1]) == 1    # the NaN orders above everything, as in torch.topk
        assert torch.equal(torch.topk(per_pixel(xn, y, base), k, dim=1).values[1, -1], aux['thresh'][1])


def _ptr(t):
    return None if t is None else t.data_ptr()


class Raw:
    """Both entry points on tensors carved out of poisoned / sentinel-filled buffers."""

    def __init__(self, B, C, H, W, Mn, k, bp=0.01, pad=64):
        from latentfusion_amd import _lib, ops
        self.L = _lib.lib()
        self.dims, self.Mn, self.k, self.pad = (B, C, H, W), Mn, k, pad
        self.a, self.b, self.lb = ops._recon_beta(bp)
        self.bufs = {}
        n = B * C * H * W
        self.x, self.y = self.carve('x', n, float('nan')), self.carve('y', n, float('nan'))
        self.z, self.t = self.carve('z', Mn, float('nan')), self.carve('t', Mn, float('nan'))
        self.thresh, self.img_sum, self.terms = self.carve('thresh', B, SENT), self.carve('img_sum', B, SENT), self.carve('terms', 4, SENT)
        self.sel = self.carve('sel', 2 * B, -77, torch.int32)
        self.gx, self.gz, self.g_terms = self.carve('gx', n, SENT), self.carve('gz', Mn, SENT), self.carve('g_terms', 3, float('nan'))
        self.need = self.L.lf_recon_loss_scratch_bytes(B, C, H, W, Mn)
        assert self.need > 0 and self.need % 4 == 0
        self.scratch = self.carve('scratch', self.need // 4, SENT)
        assert self.scratch.data_ptr() % 8 == 0
        self.stream = torch.cuda.current_stream().cuda_stream

    def carve(self, name, n, fill, dtype=torch.float32):
        buf = torch.full((n + 2 * self.pad,), fill, device=DEV, dtype=dtype)
        self.bufs[name] = (buf, buf.clone(), n)
        return buf[self.pad:self.pad + n]

    def borders_intact(self, names=None, whole=()):
        """The pads of `names` (default all) hold their fill bit for bit; `whole`: the tensor between them too."""
        torch.cuda.synchronize()
        for name, (buf, orig, n) in self.bufs.items():
            if names is not None and name not in names and name not in whole:
                continue
            a, b = buf.view(torch.int32), orig.view(torch.int32)
            if name in whole:
                assert torch.equal(a, b), name
            else:
                assert torch.equal(a[:self.pad], b[:self.pad]) and torch.equal(a[self.pad + n:], b[self.pad + n:]), name

    def fwd(self, **over):
        B, C, H, W = self.dims
        a = dict(x=_ptr(self.x), y=_ptr(self.y), base=1, k=self.k, z=_ptr(self.z), t=_ptr(self.t), alpha=self.a, beta=self.b, lb=self.lb,
                 thresh=_ptr(self.thresh), sel=_ptr(self.sel), img_sum=_ptr(self.img_sum), terms=_ptr(self.terms),
                 scratch=_ptr(self.scratch), nbytes=self.need, B=B, C=C, H=H, W=W, Mn=self.Mn)
        a.update(over)
        return self.L.lf_recon_loss_fwd(a['x'], a['y'], a['base'], a['k'], a['z'], a['t'], a['alpha'], a['beta'], a['lb'], a['thresh'],
                                        a['sel'], a['img_sum'], a['terms'], a['scratch'], a['nbytes'], a['B'], a['C'], a['H'], a['W'],
                                        a['Mn'], self.stream)

    def bwd(self, **over):
        B, C, H, W = self.dims
        a = dict(g=_ptr(self.g_terms), x=_ptr(self.x), y=_ptr(self.y), base=1, k=self.k, thresh=_ptr(self.thresh), sel=_ptr(self.sel),
                 z=_ptr(self.z), t=_ptr(self.t), alpha=self.a, beta=self.b, lb=self.lb, gx=_ptr(self.gx), gz=_ptr(self.gz),
                 B=B, C=C, H=H, W=W, Mn=self.Mn)
        a.update(over)
        return self.L.lf_recon_loss_bwd(a['g'], a['x'], a['y'], a['base'], a['k'], a['thresh'], a['sel'], a['z'], a['t'], a['alpha'],
                                        a['beta'], a['lb'], a['gx'], a['gz'], a['B'], a['C'], a['H'], a['W'], a['Mn'], self.stream)


def test_poison_is_never_read_and_sentinels_stay():
    from latentfusion_amd import ops
    B, C, H, W, k, Mn, bp = 2, 3, 33, 65, 500, 4097, 0.01
    x, y = inputs(B, C, H, W)
    z, t = mask_inputs(Mn, True)
    r = Raw(B, C, H, W, Mn, k, bp)
    r.x.copy_(x.reshape(-1)), r.y.copy_(y.reshape(-1)), r.z.copy_(z), r.t.copy_(t)
    r.g_terms.copy_(torch.tensor([3.0, 5.0, 7.0]))
    assert r.fwd() == 0 and r.bwd() == 0
    r.borders_intact()
    xd, zd = x.to(DEV).requires_grad_(True), z.to(DEV).requires_grad_(True)
    terms = ops.recon_losses(xd, y.to(DEV), 'smooth_l1', k, zd, t.to(DEV), bp)
    (terms * torch.tensor([3.0, 5.0, 7.0], device=DEV)).sum().backward()
    assert torch.equal(r.terms[:3], terms.detach()) and float(r.terms[3]) == 0.0 and bool(torch.isfinite(terms).all())
    assert torch.equal(r.gx, xd.grad.reshape(-1)) and torch.equal(r.gz, zd.grad)


# ---- 6. the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_errors_leave_everything_untouched():
    from latentfusion_amd import _lib
    EINVAL, EALIGN, ENOSPC = -1, -2, -3
    B, C, H, W, Mn, k = 2, 1, 9, 11, 130, 20
    r = Raw(B, C, H, W, Mn, k)
    r.x.normal_(), r.y.normal_(), r.z.normal_(), r.t.uniform_()
    r.g_terms.fill_(1.0)
    for n in ('x', 'y', 'z', 't', 'g_terms'):                                    # (the inputs' present state is what must stay)
        r.bufs[n] = (r.bufs[n][0], r.bufs[n][0].clone(), r.bufs[n][2])
    outs = ('thresh', 'sel', 'img_sum', 'terms', 'gx', 'gz', 'scratch')
    fwd_ptrs, bwd_ptrs = ('x', 'y', 'z', 't', 'thresh', 'sel', 'img_sum', 'terms'), ('g', 'x', 'y', 'thresh', 'sel', 'z', 't', 'gx', 'gz')
    inval = [dict(terms=None), dict(scratch=None), dict(x=None, z=None), dict(y=None), dict(thresh=None), dict(sel=None),
             dict(img_sum=None), dict(t=None), dict(B=0), dict(B=-1), dict(C=0), dict(C=5), dict(H=0), dict(W=0), dict(W=-3),
             dict(Mn=0), dict(Mn=-1), dict(Mn=(1 << 40) + 1), dict(k=-1), dict(k=H * W + 1), dict(base=2), dict(base=-1),
             dict(H=1 << 16, W=1 << 15, k=1), dict(H=46341, W=46341, k=1), dict(B=1 << 20, H=1 << 10, W=1 << 10)]
    for over in inval:
        assert r.fwd(**over) == EINVAL, over
    inval_b = [dict(g=None), dict(x=None, z=None), dict(y=None), dict(thresh=None), dict(sel=None), dict(gx=None), dict(t=None),
               dict(gz=None)] + [o for o in inval if not ({'terms', 'scratch', 'img_sum'} & set(o)) and o not in inval[2:8]]
    for over in inval_b:
        assert r.bwd(**over) == EINVAL, over
    # a part that is absent takes its sizes and pointers with it
    for over in (dict(x=None, B=0, C=9, H=0, W=-1, k=-5, base=7, y=None, thresh=None, sel=None, img_sum=None),):
        assert r.fwd(**over) == 0
    r.terms.fill_(SENT)
    r.scratch.fill_(SENT)
    torch.cuda.synchronize()
    for name in fwd_ptrs:
        base_ptr = getattr(r, name).data_ptr()
        assert r.fwd(**{name: base_ptr + 2}) == EALIGN, name
    assert r.fwd(scratch=r.scratch.data_ptr() + 4, nbytes=r.need + 64) == EALIGN
    for name in bwd_ptrs:
        base_ptr = (r.g_terms if name == 'g' else getattr(r, name)).data_ptr()
        assert r.bwd(**{name: base_ptr + 2}) == EALIGN, name
    assert r.fwd(nbytes=r.need - 4) == ENOSPC and r.fwd(nbytes=0) == ENOSPC
    r.borders_intact(whole=outs + ('x', 'y', 'z', 't', 'g_terms'))
    q = r.L.lf_recon_loss_scratch_bytes
    for args in ((0, 0, 0, 0, 0), (0, 1, 9, 11, 0), (2, 0, 9, 11, 0), (2, 5, 9, 11, 0), (2, 1, 0, 11, 5), (2, 1, 9, -1, 5),
                 (2, 1, 9, 11, -1), (1, 1, 1 << 16, 1 << 15, 0), (1 << 20, 1, 1 << 10, 1 << 10, 0), (0, 0, 0, 0, (1 << 40) + 1)):
        assert q(*args) == 0, args
    assert _lib._ERR[EINVAL].startswith('LF_EINVAL') and _lib._ERR[EALIGN].startswith('LF_EALIGN') and _lib._ERR[ENOSPC].startswith('LF_ENOSPC')
    # and the same arguments, unspoilt, run: every k of the domain's edge, both bases, either part alone
    for kw in (dict(k=0), dict(k=1), dict(k=H * W), dict(base=0, k=k), dict(x=None), dict(z=None)):
        assert r.fwd(**kw) == 0 and r.bwd(**kw) == 0, kw
    r.borders_intact()
    assert bool(torch.isfinite(r.terms).all()) and bool(torch.isfinite(r.gx).all()) and bool(torch.isfinite(r.gz).all())


# ---- 7. plumbing ----------------------------------------------------------------------------------------------------------------
def test_hard_pixel_loss_module_fused_equals_composed():
    from latentfusion_amd import losses
    x4, y4 = inputs(2, 3, 33, 65)
    x, y = x4.reshape(1, 2, 3, 33, 65).to(DEV), y4.reshape(1, 2, 3, 33, 65).to(DEV)          # 5-D, as the training step passes them
    for base, name in ((nn.L1Loss, 'l1'), (nn.SmoothL1Loss, 'smooth_l1')):
        fused, composed = losses.HardPixelLoss(base, 500, kernel='fused'), losses.HardPixelLoss(base, 500)
        for k in (500, 250):                                                     # k is read at every call
            fused.k = composed.k = k
            xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
            a, b = fused(xa, y), composed(xb, y)
            assert a.shape == b.shape == () and a.dtype == b.dtype
            (a * (2.0 * k)).backward(), (b * (2.0 * k)).backward()
            idx32 = torch.topk(per_pixel(x4, y4, name), k, dim=1).indices
            t64, _, _ = ref_hard(x4, y4, name, k, torch.float64)
            _, g64, _ = ref_hard(x4, y4, name, k, torch.float64, idx32, 2.0 * k)
            assert excess(a.detach(), t64, b.detach().cpu())[0] <= 0
            assert excess(xa.grad.reshape(2, 3, 33, 65), g64, xb.grad.reshape(2, 3, 33, 65).cpu())[0] <= 0
    with pytest.raises(ValueError, match='composed'):
        losses.HardPixelLoss(nn.L1Loss, 5, kernel='fused')(x.cpu(), y.cpu())
    with pytest.raises(ValueError):
        losses.HardPixelLoss(nn.L1Loss, 33 * 65 + 1, kernel='fused')(x, y)      # where torch.topk raises


# total = 25 depth_recon + 25 mask_recon + w mask_beta, w <= 0.5: the fixed members of the three terms' bounds weigh
# (25 + 25 + 0.5) * 2e-6, the relative members 2e-5 of the total, and twice that leaves room for the roundings of the sum itself
TOTAL_FIXED = 50.5 * 2e-6


def _trace(fn):
    """(result, names of every profiler event, names of the device kernels) of fn."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    events = list(prof.events())
    return out, [e.name for e in events], [e.name for e in events if e.device_type == DeviceType.CUDA]


def _syn_step(amp, loss_kernel, S=16, k=64, seed=3, **kw):
    from latentfusion_amd import synth
    from latentfusion_amd.recon import training
    model, _ = synth.build_model(S, 16, 'gru', seed=seed, device=DEV, bias_std=0.05)
    oi = model.preprocess_observation(synth.make_observation(3, seed + 1, DEV))
    oo = model.preprocess_observation(synth.make_observation(2, seed + 2, DEV))
    step = training.GeneratorStep(model.sculptor, model.fuser, model.photographer, g_depth_recon_loss_k=k, use_amp=amp,
                                  loss_kernel=loss_kernel, **kw)
    batch = {'in': {'camera': oi.camera, 'image': oi.color.unsqueeze(0), 'mask': oi.mask.unsqueeze(0)},
             'out_gt': {'camera': oo.camera, 'depth': oo.depth.unsqueeze(0), 'mask': oo.mask.unsqueeze(0)}}
    names = [k + '.' + n for k, m in (('s', model.sculptor), ('f', model.fuser), ('p', model.photographer)) for n, _ in m.named_parameters()]
    params = [p for m in (model.sculptor, model.fuser, model.photographer) for p in m.parameters()]
    return step, batch, names, params


def _fp64_tail(step, batch):
    """The composed step's forward with its loss tail evaluated in fp64 from y[...].double(); gradients into the flat buffer."""
    from latentfusion_amd import losses
    step.flat.zero_grad()
    _, y = step.losses(batch)
    b_out = batch['out_gt']
    crit = losses.HardPixelLoss(nn.SmoothL1Loss, step.depth_criterion.k)
    out = {'depth_recon': crit(y['depth'].double(), b_out['depth'].double()),
           'mask_recon': F.binary_cross_entropy_with_logits(y['mask_logits'].double(), b_out['mask'].double()),
           'mask_beta': losses.beta_prior_loss(torch.sigmoid(y['mask_logits'].double()), alpha=step.beta_param, beta=step.beta_param)}
    total = (step.w_depth * out['depth_recon'] + step.w_mask * out['mask_recon'] + step.w_beta * out['mask_beta']) / step.batch_groups
    total.backward()
    return {n: v.detach() for n, v in out.items()}


@pytest.mark.parametrize('amp', [False, True])
def test_generator_step_fused_vs_composed(amp):
    comp, batch, names, params = _syn_step(amp, None)
    assert comp.loss_kernel == 'composed'
    (out_c, comp_names, _) = _trace(lambda: comp.run_iteration(batch, is_step=False))
    g_c = [p.grad.detach().clone() for p in params]
    out64 = _fp64_tail(comp, batch)
    g_64 = [p.grad.detach().clone() for p in params]
    assert any('topk' in n.lower() for n in comp_names) and any('binary_cross_entropy_with_logits' in n for n in comp_names)

    fused, batch_f, _, params_f = _syn_step(amp, 'fused')
    fused.run_iteration(batch_f, is_step=False)                                  # (warm)
    (out_f, all_names, kernels) = _trace(lambda: fused.run_iteration(batch_f, is_step=False))
    g_f = [p.grad.detach().clone() for p in params_f]
    for word in ('topk', 'sort', 'binary_cross_entropy_with_logits'):
        assert not [n for n in all_names if word in n.lower()], word
    count = {w: len([n for n in kernels if w in n]) for w in ('tl_pixel_kernel', 'tl_select_kernel', 'tl_finish_kernel', 'tl_bwd_kernel')}
    assert count == {'tl_pixel_kernel': 1, 'tl_select_kernel': 1, 'tl_finish_kernel': 1, 'tl_bwd_kernel': 1}, count
    assert out_f.keys() == out_c.keys()
    for n in out_c:
        assert out_f[n].shape == out_c[n].shape == () and out_f[n].dtype == out_c[n].dtype and out_f[n].device == out_c[n].device
    for n in ('depth_recon', 'mask_recon', 'mask_beta'):
        ex, err, e32 = excess(out_f[n], out64[n].cpu(), out_c[n].cpu())
        print(f'[train_loss] step amp={amp} {n}: fused-fp64 {err:.2e}, composed-fp64 {e32:.2e}')
        assert ex <= 0, (n, ex)
    assert abs(float(out_f['total']) - float(out_c['total'])) <= TOTAL_FIXED + 4e-5 * abs(float(out_c['total']))

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))
    worst = (0.0, 0.0, None)
    for name, a, b, c in zip(names, g_f, g_c, g_64):
        gap, own = rel(a, b), rel(b, c)
        if gap >= worst[0]:
            worst = (gap, own, name)
        assert gap <= 10 * own, (name, gap, own)
    own_all = rel(torch.cat([g.reshape(-1) for g in g_c]), torch.cat([g.reshape(-1) for g in g_64]))
    gap_all = rel(torch.cat([g.reshape(-1) for g in g_f]), torch.cat([g.reshape(-1) for g in g_c]))
    print(f'[train_loss] step amp={amp} gradient rel-L2: fused-composed {gap_all:.2e}, composed-fp64 tail {own_all:.2e}; largest '
          f'per-parameter fused-composed {worst[0]:.2e} (its composed-fp64 {worst[1]:.2e}, {worst[2]})')

    # two fresh fused steps, optimiser step included: the same bits
    runs = []
    for _ in range(2):
        s, b, _, ps = _syn_step(amp, 'fused')
        o = s.run_iteration(b)
        runs.append(([o[n].clone() for n in sorted(o)], s.flat.data.clone()))
    assert all(torch.equal(p, q) for p, q in zip(runs[0][0], runs[1][0])) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize('depth_type', ['l1', 'smooth_l1', 'hard_l1'])
def test_generator_step_other_depth_terms(depth_type):
    res = {}
    for kernel in ('composed', 'fused'):
        step, batch, _, params = _syn_step(False, kernel, g_depth_recon_loss_type=depth_type, g_mask_beta_loss_weight=0.5)
        res[kernel] = step.run_iteration(batch, is_step=False)
        assert bool(torch.isfinite(step.flat.grad).all()) and float(step.flat.grad.abs().max()) > 0
    for n in ('depth_recon', 'mask_recon', 'mask_beta'):
        a, b = float(res['fused'][n]), float(res['composed'][n])
        assert abs(a - b) <= 2e-6 + 2e-5 * abs(b), (n, a, b)
    a, b = float(res['fused']['total']), float(res['composed']['total'])
    assert abs(a - b) <= TOTAL_FIXED + 4e-5 * abs(b), (a, b)


@pytest.mark.parametrize('amp', [False, True])
def test_generator_step_fused_vs_the_reference_fixture(golden, amp):
    """tests/test_autocast_gpu.py::test_generator_step_vs_the_reference_fixture with loss_kernel='fused', its bounds unchanged."""
    from latentfusion_amd import synth
    from latentfusion_amd.modules.geometry import Camera
    from latentfusion_amd.observation import Observation
    from latentfusion_amd.recon import training
    g = golden('g27_training_gradients')
    S, C, seed = g['S'], g['C'], g['seed']
    model, _ = synth.build_model(S, C, 'gru', seed=seed, device=DEV, bias_std=g['bias_std'])

    def obs(n, sd):
        d = synth.make_observation_data(n, sd)
        return model.preprocess_observation(Observation(d['color'], d['depth'], d['mask'], Camera(d['intrinsic'], d['extrinsic'])).to(DEV))
    oi, oo = obs(g['views_in'], seed + 1), obs(g['views_out'], seed + 2)
    step = training.GeneratorStep(model.sculptor, model.fuser, model.photographer, g_depth_recon_loss_k=S * S // 4, use_amp=amp,
                                  loss_kernel='fused')
    batch = {'in': {'camera': oi.camera, 'image': oi.color.unsqueeze(0), 'mask': oi.mask.unsqueeze(0)},
             'out_gt': {'camera': oo.camera, 'depth': oo.depth.unsqueeze(0), 'mask': oo.mask.unsqueeze(0)}}
    out = step.run_iteration(batch, is_step=False)
    mods = {'s': model.sculptor, 'f': model.fuser, 'p': model.photographer}
    got = {k + '.' + n: p.grad.detach().cpu() for k, m in mods.items() for n, p in m.named_parameters()}
    ref32 = g['grad_fp32']
    cat = lambda d: torch.cat([d[k].reshape(-1) for k in ref32]).double()      # noqa: E731
    if not amp:
        assert abs(float(out['depth_recon']) - float(g['loss_fp32']['depth_recon'])) < 1e-4 * float(g['loss_fp32']['depth_recon'])
        assert abs(float(out['mask_recon']) - float(g['loss_fp32']['mask_recon'])) < 1e-4 * float(g['loss_fp32']['mask_recon'])
        for key, want in ref32.items():
            rel = float((got[key] - want).norm() / want.norm().clamp_min(1e-30))
            assert rel < 1e-2, (key, rel)
        assert F.cosine_similarity(cat(got), cat(ref32), dim=0).item() > 0.9999
    else:
        want16 = float(g['loss_autocast_bf16']['total'])
        assert abs(float(out['total']) - want16) < 2e-2 * want16, (float(out['total']), want16)
        cos_hip = F.cosine_similarity(cat(got), cat(ref32), dim=0).item()
        cos_ref = F.cosine_similarity(cat(g['grad_autocast_bf16']), cat(ref32), dim=0).item()
        assert cos_hip > cos_ref - 0.03, (cos_hip, cos_ref)
