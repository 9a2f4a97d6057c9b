// Loss tail of the generator's training step (gfx950): the hard-pixel-mined depth term, the BCE mask term and the Beta prior on
// the predicted mask in three launches forward and one backward (reference losses.py:33-57,94-99,
// train_reconstruct.py:491-521).  No float atomics, no waiting between workgroups, no device-to-host copy.
//   tl_pixel_kernel   per-pixel loss l[b][p] = mean_c base(x, y) into scratch (a NaN as the positive quiet NaN 0x7fc00000, which
//                     orders above +inf like every other key here: the losses are non-negative floats and order like their
//                     bits), and, in the same launch, the mask part's partial sums: workgroup j sums elements
//                     [j * 2048, (j + 1) * 2048) in fp64, a split that depends on Mn alone.
//   tl_select_kernel  one workgroup per image: an 8-bit-digit radix select, most significant digit first, on the bit patterns
//                     (the scheme of di_radix_select in depth_init.hip) finds the k-th largest loss t_b; one more pass counts
//                     n_gt and sums the losses above t_b in fp64 (thread i takes pixels i, i + 1024, ..; then a fixed butterfly
//                     and the 16 waves in order), kept sum = that + n_tie * t_b.  The split follows (H, W) alone, and nothing
//                     of another image enters: image b of a batch has the bits of a call on that image alone.
//   tl_finish_kernel  one wavefront: the images' sums and the mask partials in a fixed order in fp64 -> terms[4].
//   tl_bwd_kernel     workgroups 0 .. B-1: one per image, the pixels in index order; the rank of a pixel among those equal to t_b
//                     comes from the ballot / mbcnt prefix of di_compact_kernel, a scan over the waves and a running count, so
//                     the n_tie tied pixels of lowest index are kept and gx is a pure function of the inputs.  The workgroups
//                     behind them: gmlogit, 4096 elements each.
// The per-pixel expression is written with __fsub_rn / __fmul_rn / __fadd_rn / __fdiv_rn: the compiler contracts none of these
// into an FMA, so for C = 1 the loss has the bits of torch's |x - y| and of d < 1 ? 0.5f * d * d : d - 0.5f (0.5f * d is exact,
// the product rounds once), and the backward recomputes exactly the forward's keys.
#include <math.h>
#include "lf_common.h"

namespace {

constexpr int TL_PT = 256;             // threads of the per-pixel / mask-partial kernel
constexpr int TL_MITER = 8;            // mask elements per thread and partial sum
constexpr int TL_MSLICE = TL_PT * TL_MITER;
constexpr int TL_ST = 1024;            // threads of the select and backward kernels
constexpr int TL_WAVES = TL_ST / 64;
constexpr int TL_UNR = 4;              // values per thread in flight (the passes are bound by load latency)
constexpr unsigned TL_QNAN = 0x7fc00000u;
constexpr float TL_EPS = 1e-4f;        // beta_prior_loss's eps
constexpr long TL_MAX_GRID = 0x7fffffffL;
constexpr long TL_MAX_MN = 1L << 40;   // far beyond any grid that passes the check; keeps the slice arithmetic in range

__device__ __forceinline__ int tl_lane_prefix(unsigned long long m) {            // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ double tl_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// base(x, y) of one element and the difference it came from; every operation rounded on its own
template <int BASE>
__device__ __forceinline__ float tl_base(float x, float y, float* diff) {
  const float df = __fsub_rn(x, y);
  *diff = df;
  const float d = fabsf(df);
  if constexpr (BASE == 0) return d;
  else return d < 1.0f ? __fmul_rn(__fmul_rn(0.5f, d), d) : __fsub_rn(d, 0.5f);
}

// key of pixel p of an image: the bits of mean_c base, channels summed in the order 0 .. C-1; diff[c] = x - y
template <int BASE>
__device__ __forceinline__ unsigned tl_pixel_key(const float* __restrict__ x, const float* __restrict__ y, long HW, long p, int C,
                                                 float* diff) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c < C) {
      const float v = tl_base<BASE>(x[c * HW + p], y[c * HW + p], &diff[c]);
      s = c == 0 ? v : __fadd_rn(s, v);
    }
  }
  if (C > 1) s = __fdiv_rn(s, (float)C);
  return s != s ? TL_QNAN : __float_as_uint(s);
}

// max(v, lo) of torch.clamp(min=lo): a NaN stays
__device__ __forceinline__ float tl_clamp_min(float v, float lo) { return v < lo ? lo : v; }

__device__ __forceinline__ float tl_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// Beta prior of one element: the loss and d(loss)/d(m); am1 = alpha - 1, bm1 = beta - 1
__device__ __forceinline__ float tl_beta(float m, float am1, float bm1, float log_beta, float* dm) {
  const float om = 1.0f - m;
  const float v = am1 * logf(tl_clamp_min(m, TL_EPS)) + bm1 * logf(tl_clamp_min(om, TL_EPS)) - log_beta;
  const float nv = -v;
  float g = 0.f;
  if (nv >= 0.f) {                                                               // clamp's gradient passes where input >= min
    if (m >= TL_EPS) g -= am1 / m;
    if (om >= TL_EPS) g += bm1 / om;
  }
  *dm = nv != nv ? nv : g;
  return tl_clamp_min(nv, 0.f);
}

// workgroups [0, pix_blocks): a pixel per thread; workgroups behind them: slice j of the mask part -> mpart[2 j + (0, 1)]
template <int BASE>
__global__ void __launch_bounds__(TL_PT) tl_pixel_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                        float* __restrict__ lbuf, long npix, int HW, int C, long pix_blocks,
                                                        const float* __restrict__ z, const float* __restrict__ t, long Mn,
                                                        float am1, float bm1, float log_beta, double* __restrict__ mpart) {
  const int tid = threadIdx.x;
  if ((long)blockIdx.x < pix_blocks) {
    const long i = (long)blockIdx.x * TL_PT + tid;
    if (i < npix) {
      const long b = i / HW, p = i - b * HW;
      float diff[4];
      lbuf[i] = __uint_as_float(tl_pixel_key<BASE>(x + b * C * HW, y + b * C * HW, HW, p, C, diff));
    }
    return;
  }
  __shared__ double s_w[TL_PT / 64][2];
  const long j = (long)blockIdx.x - pix_blocks;
  double bce = 0.0, bet = 0.0;
#pragma unroll
  for (int it = 0; it < TL_MITER; ++it) {
    const long i = j * TL_MSLICE + it * TL_PT + tid;
    if (i < Mn) {
      const float zi = z[i], ti = t[i];
      bce += (double)(fmaxf(zi, 0.f) - zi * ti + log1pf(expf(-fabsf(zi))));
      float dm;
      bet += (double)tl_beta(tl_sigmoid(zi), am1, bm1, log_beta, &dm);
    }
  }
  bce = tl_wave_sum_f64(bce);
  bet = tl_wave_sum_f64(bet);
  if ((tid & 63) == 0) {
    s_w[tid >> 6][0] = bce;
    s_w[tid >> 6][1] = bet;
  }
  __syncthreads();
  if (tid < 2) mpart[2 * j + tid] = ((s_w[0][tid] + s_w[1][tid]) + s_w[2][tid]) + s_w[3][tid];
}

// The key of rank `rank` (0-based, ascending, < n) among the n values of v, by all TL_ST threads.  s_hist: 256 ints, s_sel: 2.
__device__ unsigned tl_radix_select(const float* __restrict__ v, int n, int rank, int* s_hist, int* s_sel) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned prefix = 0;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (long base = 0; base < n; base += TL_ST * TL_UNR) {                      // (uniform: the ballots see every lane)
      unsigned key[TL_UNR];
#pragma unroll
      for (int u = 0; u < TL_UNR; ++u) {
        const long i = base + u * TL_ST + tid;
        key[u] = i < n ? __float_as_uint(v[i]) : 0u;
      }
#pragma unroll
      for (int u = 0; u < TL_UNR; ++u) {
        const bool act = base + u * TL_ST + tid < n && (pass == 0 || (key[u] >> (shift + 8)) == prefix);
        const unsigned digit = (key[u] >> shift) & 255u;
        const unsigned long long am = __ballot(act);
        if (am != 0) {                                                           // one add per wave where its lanes agree on the digit
          const int first = __ffsll((long long)am) - 1;
          const unsigned d0 = (unsigned)__shfl((int)digit, first, 64);
          const unsigned long long same = __ballot(act && digit == d0);
          if (same == am) {
            if (lane == first) atomicAdd(&s_hist[d0], __popcll(am));
          } else if (act) {
            atomicAdd(&s_hist[digit], 1);
          }
        }
      }
    }
    __syncthreads();
    if (tid < 64) {                                                              // the bucket that holds `rank`: lane l scans bins 4l .. 4l + 3
      const int c0 = s_hist[4 * lane], c1 = s_hist[4 * lane + 1], c2 = s_hist[4 * lane + 2], c3 = s_hist[4 * lane + 3];
      const int sum = c0 + c1 + c2 + c3;
      int incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      const int excl = incl - sum;
      if (rank >= excl && rank < incl) {                                         // exactly one lane (0 <= rank < the pass's total)
        int rem = rank - excl, bin = 4 * lane;
        if (rem >= c0) {
          rem -= c0;
          ++bin;
          if (rem >= c1) {
            rem -= c1;
            ++bin;
            if (rem >= c2) {
              rem -= c2;
              ++bin;
            }
          }
        }
        s_sel[0] = bin;
        s_sel[1] = rem;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | (unsigned)s_sel[0];
    rank = s_sel[1];
    __syncthreads();                                                             // s_sel and s_hist are rewritten by the next pass
  }
  return prefix;
}

__global__ void __launch_bounds__(TL_ST) tl_select_kernel(const float* __restrict__ lbuf, int HW, int k, float* __restrict__ thresh,
                                                         int* __restrict__ sel, float* __restrict__ img_sum,
                                                         double* __restrict__ isum) {
  __shared__ int s_hist[256];
  __shared__ int s_sel[2];
  __shared__ double s_sum[TL_WAVES];
  __shared__ int s_cnt[TL_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long b = blockIdx.x;
  const float* v = lbuf + b * HW;
  // k = 0: no mining, everything is "above the threshold"
  const unsigned tk = k > 0 ? tl_radix_select(v, HW, HW - k, s_hist, s_sel) : 0u;
  double acc = 0.0;
  int cnt = 0;
  for (long base = 0; base < HW; base += TL_ST * TL_UNR) {
    float val[TL_UNR];
#pragma unroll
    for (int u = 0; u < TL_UNR; ++u) {
      const long i = base + u * TL_ST + tid;
      val[u] = i < HW ? v[i] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < TL_UNR; ++u) {
      if (base + u * TL_ST + tid < HW && (k == 0 || __float_as_uint(val[u]) > tk)) {
        acc += (double)val[u];
        ++cnt;
      }
    }
  }
  acc = tl_wave_sum_f64(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) {
    s_sum[wave] = acc;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    int n_gt = 0;
#pragma unroll
    for (int w = 0; w < TL_WAVES; ++w) {
      s += s_sum[w];
      n_gt += s_cnt[w];
    }
    const int n_tie = k > 0 ? k - n_gt : 0;
    const float t = __uint_as_float(tk);
    if (n_tie > 0) s += (double)n_tie * (double)t;
    thresh[b] = t;
    sel[2 * b] = n_gt;
    sel[2 * b + 1] = n_tie;
    img_sum[b] = (float)s;
    isum[b] = s;
  }
}

// one wavefront: terms = (sum_b isum[b] / denom, sum_j mpart[2j] / Mn, sum_j mpart[2j + 1] / Mn, 0); an absent part gives 0
__global__ void __launch_bounds__(64) tl_finish_kernel(const double* __restrict__ isum, int B, double denom,
                                                      const double* __restrict__ mpart, long slices, long Mn,
                                                      float* __restrict__ terms) {
  const int lane = threadIdx.x;
  double r = 0.0, bce = 0.0, bet = 0.0;
  for (int b = lane; b < B; b += 64) r += isum[b];
  for (long j = lane; j < slices; j += 64) {
    bce += mpart[2 * j];
    bet += mpart[2 * j + 1];
  }
  r = tl_wave_sum_f64(r);
  bce = tl_wave_sum_f64(bce);
  bet = tl_wave_sum_f64(bet);
  if (lane == 0) {
    terms[0] = B > 0 ? (float)(r / denom) : 0.f;
    terms[1] = slices > 0 ? (float)(bce / (double)Mn) : 0.f;
    terms[2] = slices > 0 ? (float)(bet / (double)Mn) : 0.f;
    terms[3] = 0.f;
  }
}

// d base / d x of one element from its difference
template <int BASE>
__device__ __forceinline__ float tl_base_grad(float df) {
  const float sgn = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
  if constexpr (BASE == 0) return sgn;
  else return fabsf(df) >= 1.0f ? sgn : df;                                      // (a NaN difference stays a NaN, as in torch)
}

template <int BASE>
__global__ void __launch_bounds__(TL_ST) tl_bwd_kernel(const float* __restrict__ g_terms, const float* __restrict__ x,
                                                      const float* __restrict__ y, const float* __restrict__ thresh,
                                                      const int* __restrict__ sel, float* __restrict__ gx, int B, int C, int HW,
                                                      int k, float inv_n, const float* __restrict__ z, const float* __restrict__ t,
                                                      float* __restrict__ gz, long Mn, float am1, float bm1, float log_beta) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if ((int)blockIdx.x >= B) {                                                    // the mask part, 4 elements per thread
    const float gb = g_terms[1] / (float)Mn, gp = g_terms[2] / (float)Mn;
#pragma unroll
    for (int u = 0; u < TL_UNR; ++u) {
      const long i = (((long)blockIdx.x - B) * TL_UNR + u) * TL_ST + tid;
      if (i < Mn) {
        const float m = tl_sigmoid(z[i]);
        float dm;
        (void)tl_beta(m, am1, bm1, log_beta, &dm);
        gz[i] = gb * (m - t[i]) + gp * dm * (m * (1.0f - m));
      }
    }
    return;
  }
  __shared__ int s_off[TL_UNR * TL_WAVES + 1];
  const long b = blockIdx.x;
  const float* xb = x + b * C * HW;
  const float* yb = y + b * C * HW;
  float* gb = gx + b * C * HW;
  const float scale = g_terms[0] * inv_n;
  const unsigned tk = k > 0 ? __float_as_uint(thresh[b]) : 0u;
  const int n_tie = k > 0 ? sel[2 * b + 1] : 0;
  int running = 0;                                                               // pixels equal to t_b before this round
  for (long base = 0; base < HW; base += TL_ST * TL_UNR) {
    float diff[TL_UNR][4];
    bool gt[TL_UNR], eq[TL_UNR];
    unsigned long long bal[TL_UNR];
#pragma unroll
    for (int u = 0; u < TL_UNR; ++u) {
      const long p = base + u * TL_ST + tid;
      gt[u] = eq[u] = false;
      if (p < HW) {
        const unsigned key = tl_pixel_key<BASE>(xb, yb, HW, p, C, diff[u]);
        gt[u] = k == 0 || key > tk;
        eq[u] = k > 0 && key == tk;
      }
      bal[u] = __ballot(eq[u]);
      if (lane == 0) s_off[u * TL_WAVES + wave] = __popcll(bal[u]);
    }
    __syncthreads();
    if (tid < 64) {                                                              // exclusive scan of the 64 (u, wave) counts, index order
      const int c = s_off[tid];
      int incl = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (tid >= o) incl += up;
      }
      s_off[tid] = incl - c;
      if (tid == 63) s_off[64] = incl;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TL_UNR; ++u) {
      const long p = base + u * TL_ST + tid;
      if (p < HW) {
        const int rank = running + s_off[u * TL_WAVES + wave] + tl_lane_prefix(bal[u]);
        const bool keep = gt[u] || (eq[u] && rank < n_tie);
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (c < C) gb[c * (long)HW + p] = keep ? scale * tl_base_grad<BASE>(diff[u][c]) : 0.f;
      }
    }
    running += s_off[64];
    __syncthreads();                                                             // s_off is rewritten by the next round
  }
}

static_assert(TL_UNR * TL_WAVES == 64, "tl_bwd_kernel scans its (u, wave) counts with one wavefront");

inline bool tl_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

struct TlPlan {
  long pix_blocks, slices;
  size_t isum_off, mpart_off, lbuf_off, bytes;
};

// domain of the two parts (hard: the hard-pixel part is present, mask: the mask part) and the scratch layout:
// [isum: B doubles][mpart: 2 * slices doubles][lbuf: B * H * W floats]
int tl_plan(bool hard, bool mask, int B, int C, int H, int W, long Mn, TlPlan* pl) {
  if (!hard && !mask) return LF_EINVAL;
  *pl = TlPlan{0, 0, 0, 0, 0, 0};
  long npix = 0;
  if (hard) {
    if (B < 1 || C < 1 || C > 4 || H < 1 || W < 1 || (long)H * W >= 0x7fffffffL) return LF_EINVAL;
    npix = (long)B * H * W;                                                      // (< 2^62; the grid check below bounds it)
    pl->pix_blocks = (npix + TL_PT - 1) / TL_PT;
  }
  if (mask) {
    if (Mn < 1 || Mn > TL_MAX_MN) return LF_EINVAL;
    pl->slices = (Mn + TL_MSLICE - 1) / TL_MSLICE;
  }
  const long bwd_grid = (hard ? B : 0) + (mask ? (Mn + TL_ST * TL_UNR - 1) / (TL_ST * TL_UNR) : 0);
  if (pl->pix_blocks + pl->slices > TL_MAX_GRID || bwd_grid > TL_MAX_GRID) return LF_EINVAL;
  pl->isum_off = 0;
  pl->mpart_off = (size_t)(hard ? B : 0) * sizeof(double);
  pl->lbuf_off = pl->mpart_off + (size_t)pl->slices * 2 * sizeof(double);
  pl->bytes = pl->lbuf_off + (size_t)npix * sizeof(float);
  return 0;
}

}  // namespace

extern "C" size_t lf_recon_loss_scratch_bytes(int B, int C, int H, int W, long Mn) {
  const bool hard = !(B == 0 && C == 0 && H == 0 && W == 0), mask = Mn != 0;
  TlPlan pl;
  if (tl_plan(hard, mask, B, C, H, W, Mn, &pl)) return 0;
  return pl.bytes;
}

extern "C" int lf_recon_loss_fwd(const float* x, const float* y, int base, int k, const float* mlogit, const float* mtarget,
                                 float alpha, float beta, float log_beta, float* thresh, int* sel, float* img_sum, float* terms,
                                 void* scratch, size_t scratch_bytes, int B, int C, int H, int W, long Mn, void* stream) {
  lf_clear_error();
  const bool hard = x != nullptr, mask = mlogit != nullptr;
  if (terms == nullptr || scratch == nullptr) return LF_EINVAL;
  if (hard && (y == nullptr || thresh == nullptr || sel == nullptr || img_sum == nullptr)) return LF_EINVAL;
  if (mask && mtarget == nullptr) return LF_EINVAL;
  TlPlan pl;
  const int bad = tl_plan(hard, mask, B, C, H, W, Mn, &pl);
  if (bad) return bad;
  if (hard && ((base != 0 && base != 1) || k < 0 || (long)k > (long)H * W)) return LF_EINVAL;
  if (!tl_aligned4(x) || !tl_aligned4(y) || !tl_aligned4(mlogit) || !tl_aligned4(mtarget) || !tl_aligned4(thresh) ||
      !tl_aligned4(sel) || !tl_aligned4(img_sum) || !tl_aligned4(terms) || (((uintptr_t)scratch) & 7u) != 0)
    return LF_EALIGN;
  if (scratch_bytes < pl.bytes) return LF_ENOSPC;
  hipStream_t s = (hipStream_t)stream;
  double* isum = (double*)((char*)scratch + pl.isum_off);
  double* mpart = (double*)((char*)scratch + pl.mpart_off);
  float* lbuf = (float*)((char*)scratch + pl.lbuf_off);
  const int HW = hard ? H * W : 1;
  const float am1 = (float)((double)alpha - 1.0), bm1 = (float)((double)beta - 1.0);
  const auto pix = base == 1 ? tl_pixel_kernel<1> : tl_pixel_kernel<0>;
  hipLaunchKernelGGL(pix, dim3((unsigned)(pl.pix_blocks + pl.slices)), dim3(TL_PT), 0, s, x, y, lbuf, hard ? (long)B * HW : 0L, HW,
                     C, pl.pix_blocks, mlogit, mtarget, mask ? Mn : 0L, am1, bm1, log_beta, mpart);
  int st = lf_launch_status();
  if (st) return st;
  if (hard) {
    hipLaunchKernelGGL(tl_select_kernel, dim3((unsigned)B), dim3(TL_ST), 0, s, (const float*)lbuf, HW, k, thresh, sel, img_sum,
                       isum);
    st = lf_launch_status();
    if (st) return st;
  }
  const double denom = (double)(hard ? B : 1) * (double)(k > 0 ? k : HW);
  hipLaunchKernelGGL(tl_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)isum, hard ? B : 0, denom, (const double*)mpart,
                     pl.slices, mask ? Mn : 1L, terms);
  return lf_launch_status();
}

extern "C" int lf_recon_loss_bwd(const float* g_terms, const float* x, const float* y, int base, int k, const float* thresh,
                                 const int* sel, const float* mlogit, const float* mtarget, float alpha, float beta,
                                 float log_beta, float* gx, float* gmlogit, int B, int C, int H, int W, long Mn, void* stream) {
  lf_clear_error();
  const bool hard = x != nullptr, mask = mlogit != nullptr;
  if (g_terms == nullptr) return LF_EINVAL;
  if (hard && (y == nullptr || thresh == nullptr || sel == nullptr || gx == nullptr)) return LF_EINVAL;
  if (mask && (mtarget == nullptr || gmlogit == nullptr)) return LF_EINVAL;
  TlPlan pl;
  const int bad = tl_plan(hard, mask, B, C, H, W, Mn, &pl);
  if (bad) return bad;
  if (hard && ((base != 0 && base != 1) || k < 0 || (long)k > (long)H * W)) return LF_EINVAL;
  if (!tl_aligned4(g_terms) || !tl_aligned4(x) || !tl_aligned4(y) || !tl_aligned4(thresh) || !tl_aligned4(sel) ||
      !tl_aligned4(mlogit) || !tl_aligned4(mtarget) || !tl_aligned4(gx) || !tl_aligned4(gmlogit))
    return LF_EALIGN;
  const int HW = hard ? H * W : 1;
  const int nb = hard ? B : 0;
  const long mblocks = mask ? (Mn + TL_ST * TL_UNR - 1) / (TL_ST * TL_UNR) : 0;
  const float inv_n = (float)(1.0 / ((double)(hard ? B : 1) * (double)(k > 0 ? k : HW) * (double)(hard ? C : 1)));
  const float am1 = (float)((double)alpha - 1.0), bm1 = (float)((double)beta - 1.0);
  const auto kern = base == 1 ? tl_bwd_kernel<1> : tl_bwd_kernel<0>;
  hipLaunchKernelGGL(kern, dim3((unsigned)(nb + mblocks)), dim3(TL_ST), 0, (hipStream_t)stream, g_terms, x, y, thresh, sel, gx, nb,
                     C, HW, k, inv_n, mlogit, mtarget, gmlogit, mask ? Mn : 0L, am1, bm1, log_beta);
  return lf_launch_status();
}
