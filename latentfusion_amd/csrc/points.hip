// Pose metrics on model point clouds (gfx950): ADD-S's nearest-point search and the point-pair means of ADD / ADD-sym / proj2d
// (reference pose/metrics.py:79-109), batched over camera pairs.
//   lf_nn_dist           brute force over coordinate DIFFERENCES (not the Gram form |a|^2 + |b|^2 - 2ab, whose fp32 cancellation
//                        costs 3e-3 .. 1.4e-2 of a nearest distance on a model cloud): a workgroup owns 256 * QPT queries of one
//                        batch, each thread keeps QPT of them in registers, and the batch's candidates stream past in tiles of
//                        NN_TC through LDS, every lane reading the same 16 bytes (a broadcast, conflict-free: four candidates' x, y or z).  The affine maps are
//                        applied while a tile is staged, the NaN test of the candidates too: nothing but three subtractions, a
//                        multiply, two FMAs and the minimum (with the index: a compare and two selects) is in the inner loop.
//                        min over d^2 is exact in any order, so a query's bits do not depend on QPT, on the tiling or on its
//                        place in the batch; one root per query at the end.
//   lf_points_pair_dist  memory-trivial: one thread per point and row, both maps, the perspective division, one root.
// Means: the 64 distances of a wavefront are summed by the fixed butterfly, in fp64, into one partial sum per 64 consecutive
// queries (a function of the query index alone), then one wavefront per row adds the partial sums in a fixed order.  No atomics.
#include <math.h>
#include "lf_common.h"

namespace {

constexpr int NN_TC = 1024;          // candidates per LDS tile (12 KiB as three coordinate arrays: one 16-byte read serves four)
constexpr int PP_PPT = 4;            // points per thread of the pair kernel

// 3x4 row-major affine map as a fixed fmaf chain; t == nullptr: identity
__device__ __forceinline__ void pts_affine(const float* __restrict__ t, float& x, float& y, float& z) {
  if (t == nullptr) return;
  const float a = fmaf(t[0], x, fmaf(t[1], y, fmaf(t[2], z, t[3])));
  const float b = fmaf(t[4], x, fmaf(t[5], y, fmaf(t[6], z, t[7])));
  const float c = fmaf(t[8], x, fmaf(t[9], y, fmaf(t[10], z, t[11])));
  x = a;
  y = b;
  z = c;
}

// fixed-order butterfly over the 64 lanes in fp64: the mean's only fp32 rounding is its last
__device__ __forceinline__ double pts_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ bool pts_isnan3(float x, float y, float z) { return x != x || y != y || z != z; }

// workgroup (b, tile): queries tile * 256 * QPT + k * 256 + thread, k < QPT, of batch b
template <int QPT, bool WANT_IDX>
__global__ void __launch_bounds__(256) nn_dist_kernel(const float* __restrict__ x1, long x1_sb, const float* __restrict__ T1,
                                                     const float* __restrict__ x2, long x2_sb, const float* __restrict__ T2,
                                                     float* __restrict__ dist, int* __restrict__ idx, double* __restrict__ partial,
                                                     int M, int Q, int tiles, int chunks) {
  __shared__ __attribute__((aligned(16))) float cx[NN_TC], cy[NN_TC], cz[NN_TC];
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int tid = threadIdx.x;
  const float* t1 = T1 != nullptr ? T1 + (long)b * 12 : nullptr;
  const float* t2 = T2 != nullptr ? T2 + (long)b * 12 : nullptr;
  const float* q1 = x1 + (long)b * x1_sb;
  const float* c2 = x2 + (long)b * x2_sb;

  float qx[QPT], qy[QPT], qz[QPT], best[QPT];
  int bi[QPT];
  bool qnan[QPT];
#pragma unroll
  for (int k = 0; k < QPT; ++k) {
    const long i = ((long)tile * QPT + k) * 256 + tid;
    qx[k] = qy[k] = qz[k] = 0.f;
    if (i < M) {
      qx[k] = q1[i * 3];
      qy[k] = q1[i * 3 + 1];
      qz[k] = q1[i * 3 + 2];
      pts_affine(t1, qx[k], qy[k], qz[k]);
    }
    qnan[k] = pts_isnan3(qx[k], qy[k], qz[k]);
    best[k] = INFINITY;
    bi[k] = -1;
  }

  int bad = 0;                       // a NaN among this batch's candidates, seen by this thread while staging
  const float fnan = __int_as_float(0x7fc00000);
  for (int base = 0; base < Q; base += NN_TC) {
    const int n = Q - base < NN_TC ? Q - base : NN_TC;
    const int n4 = (n + 3) & ~3;
    __syncthreads();
    for (int j = tid; j < n4; j += 256) {
      float x = fnan, y = fnan, z = fnan;        // padding up to the unroll width: d^2 = NaN never wins
      if (j < n) {
        const long c = (long)(base + j) * 3;
        x = c2[c];
        y = c2[c + 1];
        z = c2[c + 2];
        pts_affine(t2, x, y, z);
        bad |= pts_isnan3(x, y, z);
      }
      cx[j] = x;
      cy[j] = y;
      cz[j] = z;
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < n4; j += 4) {
      const f32x4 vx = *(const f32x4*)&cx[j], vy = *(const f32x4*)&cy[j], vz = *(const f32x4*)&cz[j];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int k = 0; k < QPT; ++k) {
          const float dx = qx[k] - vx[u], dy = qy[k] - vy[u], dz = qz[k] - vz[u];
          const float d2 = fmaf(dz, dz, fmaf(dy, dy, __fmul_rn(dx, dx)));
          if constexpr (WANT_IDX) {
            if (d2 < best[k]) {      // strict: an exact tie keeps the smallest index
              best[k] = d2;
              bi[k] = base + j + u;
            }
          } else {
            best[k] = fminf(best[k], d2);          // (a NaN d^2, the padding's, leaves best as it is)
          }
        }
      }
    }
  }
  bad = __syncthreads_or(bad);

#pragma unroll
  for (int k = 0; k < QPT; ++k) {
    const long i = ((long)tile * QPT + k) * 256 + tid;
    const bool lost = bad || qnan[k];
    const float d = lost ? fnan : sqrtf(best[k]);
    if (i < M) {
      if (dist != nullptr) dist[(long)b * M + i] = d;
      if constexpr (WANT_IDX) idx[(long)b * M + i] = lost ? -1 : bi[k];
    }
    if (partial != nullptr) {
      const double s = pts_wave_sum_f64(i < M ? (double)d : 0.0);
      const long chunk = ((long)tile * QPT + k) * 4 + (tid >> 6);           // 64 consecutive queries
      if ((tid & 63) == 0 && chunk < chunks) partial[(long)b * chunks + chunk] = s;
    }
  }
}

// workgroup (chunk, r): points chunk * 1024 + k * 256 + thread of row r; ROWS = 4: 3-D points, ROWS = 3: 2-D points
template <int ROWS>
__global__ void __launch_bounds__(256) pair_dist_kernel(const float* __restrict__ pts, long pts_sr, const float* __restrict__ A,
                                                       const float* __restrict__ Bm, double* __restrict__ partial, int P,
                                                       int chunks) {
  const int r = blockIdx.y, tid = threadIdx.x;
  const float* a = A + (long)r * ROWS * 4;
  const float* bm = Bm + (long)r * ROWS * 4;
  const float* p = pts + (long)r * pts_sr;
#pragma unroll
  for (int k = 0; k < PP_PPT; ++k) {
    const long i = ((long)blockIdx.x * PP_PPT + k) * 256 + tid;
    float d = 0.f;
    if (i < P) {
      const float x = p[i * 3], y = p[i * 3 + 1], z = p[i * 3 + 2];
      float ha[ROWS], hb[ROWS];
#pragma unroll
      for (int e = 0; e < ROWS; ++e) {
        ha[e] = fmaf(a[e * 4], x, fmaf(a[e * 4 + 1], y, fmaf(a[e * 4 + 2], z, a[e * 4 + 3])));
        hb[e] = fmaf(bm[e * 4], x, fmaf(bm[e * 4 + 1], y, fmaf(bm[e * 4 + 2], z, bm[e * 4 + 3])));
      }
      float d2 = 0.f;
#pragma unroll
      for (int e = 0; e < ROWS - 1; ++e) {
        const float v = ha[e] / ha[ROWS - 1] - hb[e] / hb[ROWS - 1];
        d2 = e == 0 ? __fmul_rn(v, v) : fmaf(v, v, d2);
      }
      d = sqrtf(d2);
    }
    const double s = pts_wave_sum_f64((double)d);
    const long chunk = ((long)blockIdx.x * PP_PPT + k) * 4 + (tid >> 6);
    if ((tid & 63) == 0 && chunk < chunks) partial[(long)r * chunks + chunk] = s;
  }
}

// one wavefront per row: the K partial sums in a fixed order (lane l takes l, l + 64, .., then the butterfly) in fp64, over count
__global__ void __launch_bounds__(64) pts_mean_kernel(const double* __restrict__ partial, int K, int count, float* __restrict__ mean) {
  const long n = blockIdx.x;
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += 64) s += partial[n * K + k];
  s = pts_wave_sum_f64(s);
  if (threadIdx.x == 0) mean[n] = (float)(s / (double)count);
}

inline int pts_chunks(int n) { return (int)(((long)n + 63) / 64); }
inline bool pts_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

template <int QPT>
void nn_launch(bool want_idx, unsigned grid, hipStream_t s, const float* x1, long x1_sb, const float* T1, const float* x2,
               long x2_sb, const float* T2, float* dist, int* idx, double* partial, int M, int Q, int tiles, int chunks) {
  const auto kern = want_idx ? nn_dist_kernel<QPT, true> : nn_dist_kernel<QPT, false>;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, x1, x1_sb, T1, x2, x2_sb, T2, dist, idx, partial, M, Q, tiles, chunks);
}

}  // namespace

extern "C" size_t lf_nn_dist_scratch_bytes(int B, int M, int Q) {
  if (B < 1 || M < 1 || Q < 1) return 0;
  return (size_t)B * (size_t)pts_chunks(M) * sizeof(double);
}

extern "C" int lf_nn_dist(const float* x1, long x1_sb, const float* T1, const float* x2, long x2_sb, const float* T2, float* dist,
                          int* idx, float* mean, void* scratch, size_t scratch_bytes, int B, int M, int Q, void* stream) {
  lf_clear_error();
  if (x1 == nullptr || x2 == nullptr || B < 1 || M < 1 || Q < 1) return LF_EINVAL;
  if (dist == nullptr && idx == nullptr && mean == nullptr) return LF_EINVAL;
  if (x1_sb < 0 || x2_sb < 0) return LF_EINVAL;
  if ((long)B * M > 0x7fffffffL || (long)B * (((long)M + 255) / 256) > 0x7fffffffL) return LF_EINVAL;
  if (!pts_aligned4(x1) || !pts_aligned4(x2) || !pts_aligned4(T1) || !pts_aligned4(T2) || !pts_aligned4(dist) ||
      !pts_aligned4(idx) || !pts_aligned4(mean) || (((uintptr_t)scratch) & 7u) != 0)
    return LF_EALIGN;
  const int chunks = pts_chunks(M);
  if (mean != nullptr && (scratch == nullptr || scratch_bytes < (size_t)B * (size_t)chunks * sizeof(double))) return LF_ENOSPC;
  hipStream_t s = (hipStream_t)stream;
  // four queries per thread once that still gives every compute unit a workgroup, one per thread below that (the results are
  // the same bits either way)
  const long tiles4 = ((long)M + 1023) / 1024;
  const bool wide = (long)B * tiles4 >= lf_cu_count();
  const int tiles = wide ? (int)tiles4 : (int)(((long)M + 255) / 256);
  double* partial = mean != nullptr ? (double*)scratch : nullptr;
  const unsigned grid = (unsigned)((long)B * tiles);
  if (wide) nn_launch<4>(idx != nullptr, grid, s, x1, x1_sb, T1, x2, x2_sb, T2, dist, idx, partial, M, Q, tiles, chunks);
  else nn_launch<1>(idx != nullptr, grid, s, x1, x1_sb, T1, x2, x2_sb, T2, dist, idx, partial, M, Q, tiles, chunks);
  const int st = lf_launch_status();
  if (st || mean == nullptr) return st;
  hipLaunchKernelGGL(pts_mean_kernel, dim3((unsigned)B), dim3(64), 0, s, (const double*)scratch, chunks, M, mean);
  return lf_launch_status();
}

extern "C" size_t lf_points_pair_dist_scratch_bytes(int R, int P) {
  if (R < 1 || P < 1) return 0;
  return (size_t)R * (size_t)pts_chunks(P) * sizeof(double);
}

extern "C" int lf_points_pair_dist(const float* pts, long pts_sr, const float* A, const float* Bm, int rows, float* mean,
                                   void* scratch, size_t scratch_bytes, int R, int P, void* stream) {
  lf_clear_error();
  if (pts == nullptr || A == nullptr || Bm == nullptr || mean == nullptr || R < 1 || P < 1 || pts_sr < 0) return LF_EINVAL;
  if (rows != 3 && rows != 4) return LF_EINVAL;
  if (R > 65535) return LF_EINVAL;
  if (!pts_aligned4(pts) || !pts_aligned4(A) || !pts_aligned4(Bm) || !pts_aligned4(mean) || (((uintptr_t)scratch) & 7u) != 0) return LF_EALIGN;
  const int chunks = pts_chunks(P);
  if (scratch == nullptr || scratch_bytes < (size_t)R * (size_t)chunks * sizeof(double)) return LF_ENOSPC;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)(((long)P + 256 * PP_PPT - 1) / (256 * PP_PPT)), (unsigned)R);
  const auto kern = rows == 4 ? pair_dist_kernel<4> : pair_dist_kernel<3>;
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, pts, pts_sr, A, Bm, (double*)scratch, P, chunks);
  const int st = lf_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(pts_mean_kernel, dim3((unsigned)R), dim3(64), 0, s, (const double*)scratch, chunks, P, mean);
  return lf_launch_status();
}
