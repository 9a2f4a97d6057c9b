// Latent loss term of the pose loop (gfx950): cosine distance between the renderer's projected latent zp and the target's
// latent code zt, per hypothesis (reference pose/estimation.py:111-114, distances.py:5-9), and its gradient folded into the
// projection's epilogue backward.
//   lf_latent_cosine_fwd      two launches: per-workgroup partial sums (dot, |zp|^2, |zt|^2) of a row's slice, then a
//                             fixed-order fp64 finish per row.  A row is cut into slices of LAT_ITERS * (256 / lanes-per-pixel)
//                             pixels, a function of (P, C) alone: row i of a batch sums exactly as a call on that row does.
//   lf_latent_cosine_bwd_epi  one streaming pass: gp = Epi'(g_in + gscale * d(dist)/d(zp); zp, norm, flags), the three forms of
//                             lf_epilogue_bwd (pointwise.hip) plus flags = 0.
// zp is channels-last [N][P][C]; as in pointwise.hip a group of lanes owns a pixel (f32x4 per lane along the channels, xor-shuffle
// reduction inside the group), here for every C % 4 == 0 up to 256: the group is the next power of two >= C / 4 lanes and the
// lanes past the last channel idle.  zt is read through element strides (NCHW-contiguous and channels-last alike, no copy):
// f32x4 loads where its channel stride is 1 and everything is 16-byte aligned, four scalar loads per lane otherwise.
#include "lf_common.h"

namespace {

constexpr float LAT_EPS = 1e-8f;     // torch.cosine_similarity's eps as the pose estimators pass it
constexpr int LAT_ITERS = 4;         // block iterations per partial sum: 4 x 256 lanes x 16 B = 16 KiB of zp per workgroup

__device__ __forceinline__ float lat_group_sum(float v, int lanes) {
  for (int o = lanes >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool VEC>
__device__ __forceinline__ f32x4 lat_load_zt(const float* __restrict__ p, long sc) {
  if constexpr (VEC) return *(const f32x4*)p;
  else return (f32x4){p[0], p[sc], p[2 * sc], p[3 * sc]};
}

int lat_lanes(int C) {
  int l = 1;
  while (l * 4 < C) l <<= 1;
  return l;
}

long lat_slices(long P, int C) {
  const long per = (long)LAT_ITERS * (256 / lat_lanes(C));
  return (P + per - 1) / per;
}

// workgroup (n, k): slice k of row n -> partial[(n * K + k) * 4 + (0, 1, 2)] = (dot, |zp|^2, |zt|^2)
template <bool VEC>
__global__ void __launch_bounds__(256) latent_partial_kernel(const float* __restrict__ zp, const float* __restrict__ zt, long zt_sn,
                                                            long zt_sp, long zt_sc, float* __restrict__ partial, long P, int C,
                                                            int lpr, long K) {
  __shared__ float wsum[4][4];
  const int rpb = 256 / lpr;
  const int q = threadIdx.x % lpr, slot = threadIdx.x / lpr;
  const long n = blockIdx.x / K, k = blockIdx.x - n * K;
  const float* zrow = zp + n * P * C + q * 4;
  const float* trow = zt + n * zt_sn + (long)q * 4 * zt_sc;
  float d = 0.f, zz = 0.f, tt = 0.f;
  if (q * 4 < C) {
#pragma unroll
    for (int it = 0; it < LAT_ITERS; ++it) {
      const long p = (k * LAT_ITERS + it) * rpb + slot;
      if (p < P) {
        const f32x4 a = *(const f32x4*)(zrow + p * C);
        const f32x4 b = lat_load_zt<VEC>(trow + p * zt_sp, zt_sc);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          d += a[e] * b[e];
          zz += a[e] * a[e];
          tt += b[e] * b[e];
        }
      }
    }
  }
  d = lf_wave_sum(d);
  zz = lf_wave_sum(zz);
  tt = lf_wave_sum(tt);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wsum[wave][0] = d;
    wsum[wave][1] = zz;
    wsum[wave][2] = tt;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int j = threadIdx.x;
    partial[(n * K + k) * 4 + j] = ((wsum[0][j] + wsum[1][j]) + wsum[2][j]) + wsum[3][j];
  }
}

// max(v, eps) that keeps a NaN (fmax would drop it: a NaN in a row must stay visible in that row)
template <typename T>
__device__ __forceinline__ T lat_clamp(T v) { return v < (T)LAT_EPS ? (T)LAT_EPS : v; }

__device__ __forceinline__ double lat_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one wavefront per row: the K partial sums in a fixed order (lane l takes l, l + 64, .., then the butterfly), in fp64
__global__ void __launch_bounds__(64) latent_finish_kernel(const float* __restrict__ partial, long K, float* __restrict__ sums,
                                                          float* __restrict__ losses, float w_latent) {
  const long n = blockIdx.x;
  const int lane = threadIdx.x;
  double d = 0.0, zz = 0.0, tt = 0.0;
  for (long k = lane; k < K; k += 64) {
    const float* s = partial + (n * K + k) * 4;
    d += (double)s[0];
    zz += (double)s[1];
    tt += (double)s[2];
  }
  d = lat_wave_sum_f64(d);
  zz = lat_wave_sum_f64(zz);
  tt = lat_wave_sum_f64(tt);
  if (lane == 0) {
    const double a = lat_clamp(sqrt(zz)), b = lat_clamp(sqrt(tt));
    const float dist = (float)(1.0 - d / (a * b));
    *(f32x4*)(sums + n * 4) = (f32x4){(float)d, (float)zz, (float)tt, dist};
    if (losses != nullptr) {
      losses[n * 8 + 5] = dist;
      losses[n * 8 + 4] += w_latent * dist;
    }
  }
}

// gp = Epi'(g_in + c1 * zt + c2 * zp; zp, norm): c1 = -gscale / (a b), c2 = gscale * dot / (a^2 b |zp|), a = max(|zp|, eps),
// b = max(|zt|, eps): torch.cosine_similarity clamps its norms in place outside the graph, so d(a)/d(zp) stays zp / |zp| below the
// clamp too (a^3 b above it), and 0 at |zp| = 0, the norm's subgradient there
template <bool VEC>
__global__ void __launch_bounds__(256) latent_bwd_epi_kernel(const float* g_in, const float* __restrict__ zp,
                                                            const float* __restrict__ norm, const float* __restrict__ zt,
                                                            long zt_sn, long zt_sp, long zt_sc, const float* __restrict__ sums,
                                                            float gscale, float* gp, long rows, long P, int C,
                                                            int lpr, unsigned flags, float slope) {
  const int rpb = 256 / lpr;
  const int q = threadIdx.x % lpr, slot = threadIdx.x / lpr;
  const bool chan = q * 4 < C;
  const long iters = (rows + (long)gridDim.x * rpb - 1) / ((long)gridDim.x * rpb);
  for (long it = 0; it < iters; ++it) {
    const long row = (it * gridDim.x + blockIdx.x) * rpb + slot;
    const bool live = row < rows && chan;
    f32x4 x = (f32x4){0.f, 0.f, 0.f, 0.f}, y = x;
    float r = 1.f;
    if (live) {
      const long n = row / P, p = row - n * P;
      const f32x4 s = *(const f32x4*)(sums + n * 4);
      const float na = sqrtf(s[1]);
      const float a = lat_clamp(na), b = lat_clamp(sqrtf(s[2]));
      const float c1 = -gscale / (a * b);
      const float c2 = na > 0.f ? gscale * (((s[0] / (a * b)) / a) / na) : 0.f;
      y = *(const f32x4*)(zp + row * C + q * 4);
      const f32x4 t = lat_load_zt<VEC>(zt + n * zt_sn + p * zt_sp + (long)q * 4 * zt_sc, zt_sc);
      if (g_in != nullptr) x = *(const f32x4*)(g_in + row * C + q * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) x[e] += c1 * t[e] + c2 * y[e];
      if (flags & LF_EPI_PIXELNORM) r = norm[row];
    }
    f32x4 g = x;
    if (flags & LF_EPI_PIXELNORM) {
      float dot = x[0] * y[0] + x[1] * y[1] + x[2] * y[2] + x[3] * y[3];
      dot = lat_group_sum(dot, lpr) / (float)C;
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = (x[e] - y[e] * dot) / r;
    }
    if (flags & LF_EPI_LRELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = y[e] > 0.f ? g[e] : g[e] * slope;
    }
    if (live) *(f32x4*)(gp + row * C + q * 4) = g;
  }
}

// argument rules shared by the two entry points; *vec: zt can be read with f32x4 loads
int lat_check(const float* zp, const float* zt, int zt_n, long zt_sn, long zt_sp, long zt_sc, int N, long P, int C, bool* vec) {
  if (zp == nullptr || zt == nullptr || N < 1 || P < 1 || C < 4 || C > 256) return LF_EINVAL;
  if (zt_n != 1 && zt_n != N) return LF_EINVAL;
  if (zt_sn < 0 || zt_sp < 0 || zt_sc < 0) return LF_EINVAL;
  if (C % 4 != 0 || !lf_aligned16(zp)) return LF_EALIGN;
  *vec = zt_sc == 1 && lf_aligned16(zt) && zt_sp % 4 == 0 && (zt_n == 1 || zt_sn % 4 == 0);
  return 0;
}

}  // namespace

extern "C" size_t lf_latent_cosine_scratch_bytes(int N, long P, int C) {
  if (N < 1 || P < 1 || C < 4 || C > 256 || C % 4 != 0) return 0;
  return (size_t)N * (size_t)lat_slices(P, C) * 4 * sizeof(float);
}

extern "C" int lf_latent_cosine_fwd(const float* zp, const float* zt, int zt_n, long zt_sn, long zt_sp, long zt_sc, float* sums,
                                    float* losses, float w_latent, void* scratch, size_t scratch_bytes, int N, long P, int C,
                                    void* stream) {
  lf_clear_error();
  bool vec = false;
  const int bad = lat_check(zp, zt, zt_n, zt_sn, zt_sp, zt_sc, N, P, C, &vec);
  if (bad) return bad;
  if (sums == nullptr) return LF_EINVAL;
  if (!lf_aligned16(sums) || !lf_aligned16(scratch)) return LF_EALIGN;
  const long K = lat_slices(P, C);
  if ((long)N * K > 0x7fffffffL) return LF_EINVAL;
  if (scratch == nullptr || scratch_bytes < (size_t)N * (size_t)K * 4 * sizeof(float)) return LF_ENOSPC;
  hipStream_t s = (hipStream_t)stream;
  const long sn = zt_n == 1 ? 0 : zt_sn;
  const int lpr = lat_lanes(C);
  const auto partial = vec ? latent_partial_kernel<true> : latent_partial_kernel<false>;
  hipLaunchKernelGGL(partial, dim3((unsigned)(N * K)), dim3(256), 0, s, zp, zt, sn, zt_sp, zt_sc, (float*)scratch, P, C, lpr, K);
  const int st = lf_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(latent_finish_kernel, dim3((unsigned)N), dim3(64), 0, s, (const float*)scratch, K, sums, losses, w_latent);
  return lf_launch_status();
}

extern "C" int lf_latent_cosine_bwd_epi(const float* g_in, const float* zp, const float* norm, const float* zt, int zt_n,
                                        long zt_sn, long zt_sp, long zt_sc, const float* sums, float gscale, float* gp, int N,
                                        long P, int C, unsigned flags, float slope, void* stream) {
  lf_clear_error();
  bool vec = false;
  const int bad = lat_check(zp, zt, zt_n, zt_sn, zt_sp, zt_sc, N, P, C, &vec);
  if (bad) return bad;
  if (sums == nullptr || gp == nullptr) return LF_EINVAL;
  if (flags & ~(LF_EPI_LRELU | LF_EPI_PIXELNORM)) return LF_EINVAL;
  if ((flags & LF_EPI_PIXELNORM) && norm == nullptr) return LF_EINVAL;
  if (!lf_aligned16(sums) || !lf_aligned16(gp) || (g_in != nullptr && !lf_aligned16(g_in))) return LF_EALIGN;
  const long rows = (long)N * P;
  const int lpr = lat_lanes(C), rpb = 256 / lpr;
  const long blocks = (rows + rpb - 1) / rpb;
  const unsigned grid = (unsigned)(blocks < 16384 ? blocks : 16384);
  const long sn = zt_n == 1 ? 0 : zt_sn;
  const auto kern = vec ? latent_bwd_epi_kernel<true> : latent_bwd_epi_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, (hipStream_t)stream, g_in, zp, norm, zt, sn, zt_sp, zt_sc, sums, gscale, gp,
                     rows, P, C, lpr, flags, slope);
  return lf_launch_status();
}
