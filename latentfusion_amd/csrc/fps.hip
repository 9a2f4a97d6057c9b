// Greedy farthest-point sampling of B clouds (gfx950; reference three/utils.py:4-49 farthest_points with F.pairwise_distance,
// as tools/dataset/moped_eval_pointclouds.py and the BOP / RealSense readers call it).  The contract of include/lf_hip.h:
//   d^2 = (dx * dx + dy * dy) + dz * dz from direct differences, each operation rounded once (this file is compiled with
//   fp contraction off -- the pragma below: the __f*_rn intrinsics are plain operators here and would be fused);
//   the running minimum is held on d^2 and starts at 1e14f; pick k = the SMALLEST index among the maxima of the running
//   minimum; owner[i] = k whenever pick k's d^2 <= the minimum before the update; nearest = sqrtf(min d^2), the correctly
//   rounded root (__fsqrt_rn is the approximate one here).
// The maximum of a set of floats is exact and the tie rule names one index, so the order of the reduction cannot show in the
// result: the two forms below give the same bits.
//   resident  one workgroup of 1024 threads per cloud, all K picks in one launch.  Coordinates and running minima live in LDS
//             (16 bytes per point, thread t owns points t, t + 1024, ..), so a pick is: read the centre (a broadcast), update the
//             own points, reduce (value, index) over the wave by the butterfly and over the 16 waves through a double-buffered
//             LDS slot -- ONE workgroup barrier per pick.  owner is written through to memory by the owning thread as it changes.
//   streamed  one launch per pick over ceil(N / FPS_SLICE) workgroups per cloud.  A workgroup first reduces the previous
//             launch's per-workgroup partial maxima from scratch (every workgroup derives the same pick), updates its slice of
//             the running minima (kept in scratch) and writes its own partial; the partials are double-buffered by the parity of
//             the pick.  K launches and one that takes the roots, queued back to back.
// No kernel waits for another workgroup: the only ordering between workgroups is the order of the launches on the stream.
#include <math.h>
#include "lf_common.h"

#pragma clang fp contract(off)      // to the end of the file: no multiply-add of this file is fused

namespace {

constexpr int FPS_RT = 1024;                    // threads of the resident workgroup
constexpr int FPS_RW = FPS_RT / 64;             // its waves
constexpr int FPS_RED_BYTES = 2 * FPS_RW * 8;   // double-buffered (value, index) per wave
constexpr int FPS_LDS_BYTES = 160 * 1024;
static_assert(LF_FPS_RESIDENT_MAX == (FPS_LDS_BYTES - FPS_RED_BYTES) / 16, "lf_hip.h: LF_FPS_RESIDENT_MAX");
constexpr int FPS_ST = 256;                     // threads of a streamed workgroup
constexpr int FPS_PPT = 4;
constexpr int FPS_SLICE = FPS_ST * FPS_PPT;     // points of a streamed workgroup
constexpr float FPS_START = 1e14f;

__device__ __forceinline__ float fps_d2(float x, float y, float z, float cx, float cy, float cz) {
  const float dx = x - cx, dy = y - cy, dz = z - cz;
  return (dx * dx + dy * dy) + dz * dz;
}

// (v, i) <- the larger value, the smaller index among equals
__device__ __forceinline__ void fps_take(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) {
    v = v2;
    i = i2;
  }
}

__device__ __forceinline__ void fps_wave_max(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, 64);
    const int i2 = __shfl_xor(i, o, 64);
    fps_take(v, i, v2, i2);
  }
}

// a pick outside [0, N) can only come from NaN coordinates (outside the contract): no fault
__device__ __forceinline__ int fps_clamp(int i, int N) { return (unsigned)i < (unsigned)N ? i : 0; }

__global__ void __launch_bounds__(FPS_RT) fps_resident_kernel(const float* __restrict__ x, long x_sb, int* __restrict__ centers,
                                                              int* __restrict__ owner, float* __restrict__ nearest, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fps_lds[];
  float* red_v = (float*)fps_lds;                       // [2][FPS_RW]
  int* red_i = (int*)(fps_lds + FPS_RED_BYTES / 2);     // [2][FPS_RW]
  float* px = (float*)(fps_lds + FPS_RED_BYTES);
  float* py = px + N;
  float* pz = py + N;
  float* pm = pz + N;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* xb = x + (long)b * x_sb;
  for (int i = tid; i < N; i += FPS_RT) {
    px[i] = xb[(long)i * 3];
    py[i] = xb[(long)i * 3 + 1];
    pz[i] = xb[(long)i * 3 + 2];
    pm[i] = FPS_START;
  }
  __syncthreads();
  int* own = owner != nullptr ? owner + (long)b * N : nullptr;
  int c = 0;
  for (int k = 0; k < K; ++k) {
    if (tid == 0 && centers != nullptr) centers[(long)b * K + k] = c;
    const float cx = px[c], cy = py[c], cz = pz[c];
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int i = tid; i < N; i += FPS_RT) {
      const float d2 = fps_d2(px[i], py[i], pz[i], cx, cy, cz);
      float m = pm[i];
      if (d2 <= m) {
        m = d2;
        pm[i] = d2;
        if (own != nullptr) own[i] = k;
      }
      if (m > bv) {                 // strict, i ascending: the smallest index of this thread's maxima
        bv = m;
        bi = i;
      }
    }
    fps_wave_max(bv, bi);
    const int par = (k & 1) * FPS_RW;
    if ((tid & 63) == 0) {
      red_v[par + (tid >> 6)] = bv;
      red_i[par + (tid >> 6)] = bi;
    }
    __syncthreads();                // the slot of pick k - 1 is the other one: nobody is still reading what pick k + 1 overwrites
    bv = red_v[par];
    bi = red_i[par];
#pragma unroll
    for (int w = 1; w < FPS_RW; ++w) fps_take(bv, bi, red_v[par + w], red_i[par + w]);
    c = fps_clamp(bi, N);
  }
  if (nearest != nullptr)
    for (int i = tid; i < N; i += FPS_RT) nearest[(long)b * N + i] = sqrtf(pm[i]);
}

// launch k of the streamed form; workgroup (b, g): points g * FPS_SLICE + j * FPS_ST + thread, j < FPS_PPT, of cloud b.
// part_v / part_i: [2][B][G]
__global__ void __launch_bounds__(FPS_ST) fps_stream_kernel(const float* __restrict__ x, long x_sb, int* __restrict__ centers,
                                                            int* __restrict__ owner, float* __restrict__ mins,
                                                            float* __restrict__ part_v, int* __restrict__ part_i, int B, int N, int K,
                                                            int G, int k) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int b = blockIdx.x / G, g = blockIdx.x - b * G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* xb = x + (long)b * x_sb;
  int c = 0;
  if (k > 0) {
    const long prev = ((long)((k - 1) & 1) * B + b) * G;
    float v = -1.f;
    int i = 0x7fffffff;
    for (int j = tid; j < G; j += FPS_ST) fps_take(v, i, part_v[prev + j], part_i[prev + j]);
    fps_wave_max(v, i);
    if (lane == 0) {
      sv[wave] = v;
      si[wave] = i;
    }
    __syncthreads();
    v = sv[0];
    i = si[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) fps_take(v, i, sv[w], si[w]);
    c = fps_clamp(i, N);
    __syncthreads();
  }
  if (g == 0 && tid == 0 && centers != nullptr) centers[(long)b * K + k] = c;
  const float cx = xb[(long)c * 3], cy = xb[(long)c * 3 + 1], cz = xb[(long)c * 3 + 2];
  float bv = -1.f;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < FPS_PPT; ++j) {
    const int i = g * FPS_SLICE + j * FPS_ST + tid;
    if (i < N) {
      const float d2 = fps_d2(xb[(long)i * 3], xb[(long)i * 3 + 1], xb[(long)i * 3 + 2], cx, cy, cz);
      float m = k > 0 ? mins[(long)b * N + i] : FPS_START;
      if (d2 <= m) {
        m = d2;
        if (owner != nullptr) owner[(long)b * N + i] = k;
      }
      mins[(long)b * N + i] = m;
      if (m > bv) {
        bv = m;
        bi = i;
      }
    }
  }
  fps_wave_max(bv, bi);
  if (lane == 0) {
    sv[wave] = bv;
    si[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    bv = sv[0];
    bi = si[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) fps_take(bv, bi, sv[w], si[w]);
    const long cur = ((long)(k & 1) * B + b) * G + g;
    part_v[cur] = bv;
    part_i[cur] = bi;
  }
}

__global__ void __launch_bounds__(256) fps_root_kernel(const float* __restrict__ mins, float* __restrict__ nearest, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) nearest[i] = sqrtf(mins[i]);
}

inline bool fps_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }
inline int fps_slices(int N) { return (int)(((long)N + FPS_SLICE - 1) / FPS_SLICE); }
inline bool fps_domain(int B, int N, int K, int form) {
  return B >= 1 && N >= 1 && K >= 1 && K <= N && (long)B * N <= 0x7fffffffL && form >= 0 && form <= 2 &&
         !(form == 1 && N > LF_FPS_RESIDENT_MAX);
}
inline int fps_form(int N, int form) { return form != 0 ? form : (N <= LF_FPS_RESIDENT_MAX ? 1 : 2); }
// streamed: running minima [B][N] fp32, then the partial maxima [2][B][G] fp32 and [2][B][G] int32
inline size_t fps_stream_bytes(int B, int N) { return ((size_t)B * N + 4 * (size_t)B * fps_slices(N)) * 4; }

lf_devmask_t fps_lds_done{0};

}  // namespace

extern "C" size_t lf_farthest_points_scratch_bytes(int B, int N, int K, int form) {
  if (!fps_domain(B, N, K, form)) return 0;
  return fps_form(N, form) == 1 ? 0 : fps_stream_bytes(B, N);
}

extern "C" int lf_farthest_points(const float* x, long x_sb, int* centers, int* owner, float* nearest, void* scratch,
                                  size_t scratch_bytes, int B, int N, int K, int form, void* stream) {
  lf_clear_error();
  if (x == nullptr || x_sb < 0 || !fps_domain(B, N, K, form)) return LF_EINVAL;
  if (centers == nullptr && owner == nullptr && nearest == nullptr) return LF_EINVAL;
  if (!fps_aligned4(x) || !fps_aligned4(centers) || !fps_aligned4(owner) || !fps_aligned4(nearest) || !fps_aligned4(scratch))
    return LF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  if (fps_form(N, form) == 1) {
    const hipError_t e = lf_ensure_dyn_lds(fps_lds_done, (const void*)fps_resident_kernel, FPS_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    const size_t lds = (size_t)FPS_RED_BYTES + (size_t)N * 16;
    hipLaunchKernelGGL(fps_resident_kernel, dim3((unsigned)B), dim3(FPS_RT), lds, s, x, x_sb, centers, owner, nearest, N, K);
    return lf_launch_status();
  }
  if (scratch == nullptr || scratch_bytes < fps_stream_bytes(B, N)) return LF_ENOSPC;
  const int G = fps_slices(N);
  if ((long)B * G > 0x7fffffffL) return LF_EINVAL;
  float* mins = (float*)scratch;
  float* part_v = mins + (size_t)B * N;
  int* part_i = (int*)(part_v + 2 * (size_t)B * G);
  for (int k = 0; k < K; ++k) {
    hipLaunchKernelGGL(fps_stream_kernel, dim3((unsigned)((long)B * G)), dim3(FPS_ST), 0, s, x, x_sb, centers, owner, mins, part_v,
                       part_i, B, N, K, G, k);
    const int st = lf_launch_status();
    if (st) return st;
  }
  if (nearest == nullptr) return 0;
  const long n = (long)B * N;
  hipLaunchKernelGGL(fps_root_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)mins, nearest, n);
  return lf_launch_status();
}
