// Weight gradient of the WIDE He-equalised convolutions (64 .. 1024 channels: the released architecture's encoder / decoder
// levels, 256-channel 3-D camera blocks, 515 -> 256 ConvGRU gates, K = 4096 factor projections) -- the training-step side of
//   Equalized.forward   latentfusion/modules/equalized.py:57-64   (y = conv(x, W) * he + b)
//   Block.forward       latentfusion/modules/blocks.py:152-158
// which the reference gets from autograd (tools/train/train_reconstruct.py:421-535).  Same math, layouts and output as
// lf_conv_bwd_weight (wgrad.hip):
//
//   gw[tap][co][ci] = scale * sum_v gpre[v][co] * x[v + tap][ci]         (zero padding, channels-last)
//
// Organisation:
//   * a 256-thread workgroup owns a 64 Cout x 64 Cin tile, one tap ROW (fixed dz, dy; the three dx taps; dims = 0: the one
//     tap) and a run of voxel tiles of 4 rows x 16 columns of one (sample, z) plane;
//   * per voxel tile the gpre tile (64 voxels) and the x halo row (4 x 18 voxels, shifted by dz, dy) are staged ONCE into LDS
//     as 64-channel rows (zero fill outside the volume and past ragged channels); the three taps read shifted windows of
//     the same halo.  Rows are 80 floats apart, so the two 16-lane k-groups of a ds_read_b32 half-wave land on opposite
//     16-bank halves: conflict-free;
//   * wave w contracts voxel row w of every tile over the whole 64 x 64 tile: 3 taps x 16 v_mfma_f32_16x16x4_f32
//     accumulators (192 floats), A = gpre (shared by the three taps), B = the shifted x window;
//   * a run is 16 tiles (x2 while there would be more than 512 runs, /2 while there would be fewer than 1024 workgroups),
//     i.e. at most the fp32 accumulation length per lane of wgrad_partial_kernel's chunks; the four waves' sums are added through LDS in a fixed order, one 64 x 64 partial per
//     (run, tap, tile pair) goes to scratch, and wgrad_wide_reduce_kernel sums the runs in a fixed order in fp64.
// fp32 products are exact, so the same kernel serves the fp32 policy and the autocast policy (bf16-valued operands).
#include "lf_common.h"

namespace {

constexpr int WW_TY = 4, WW_TX = 16, WW_HX = WW_TX + 2;        // tile rows (one per wave), columns, halo columns
constexpr int WW_RS = 80;                                       // LDS row stride (floats): 64 channels + 16 pad
constexpr int WW_GROWS = WW_TY * WW_TX;                         // 64 gpre rows
constexpr int WW_XROWS = WW_TY * WW_HX;                         // 72 x halo rows
constexpr int WW_STAGE = (WW_GROWS + WW_XROWS) * WW_RS * 4;    // 43,520 B
constexpr int WW_RED = 4 * 64 * 64 * 4;                         // 65,536 B: the four waves' 64 x 64 sums of one tap
constexpr int WW_LDS = WW_STAGE > WW_RED ? WW_STAGE : WW_RED;
constexpr int WW_RUN0 = 16, WW_MAXRUNS = 512, WW_MINWGS = 1024;

// four channels [c, c + 4) of row `gv` of a channels-last [rows][C] array; zeros outside the volume / past C
__device__ __forceinline__ f32x4 ww_load(const float* __restrict__ p, long gv, int C, int c, bool ok, bool vec) {
  f32x4 r = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (!ok || c >= C) return r;
  const float* q = p + gv * C + c;
  if (vec) return *(const f32x4*)q;                             // C % 4 == 0 and a 16-B aligned base
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (c + e < C) r[e] = q[e];
  return r;
}

template <int DIMS>
__global__ void __launch_bounds__(256) wgrad_wide_kernel(
    const float* __restrict__ x, const float* __restrict__ gp, float* __restrict__ partial,
    int N, int D, int H, int W, int Cin, int Cout, int tiles_x, int tiles_y, int ntiles, int run, int ncit, int taps) {
  constexpr int G = DIMS == 0 ? 1 : 3;                          // taps of the workgroup: dx = -1, 0, 1
  extern __shared__ __attribute__((aligned(16))) float wlds[];
  float* gs = wlds;
  float* xs = wlds + WW_GROWS * WW_RS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = lane & 15, k = lane >> 4;
  const int tp = blockIdx.x, ntp = gridDim.x;
  const int ct = tp / ncit, cit = tp - ct * ncit;
  const int co0 = ct * 64, ci0 = cit * 64;
  const int trow = blockIdx.y;                                  // tap row: (dz + 1) * 3 + (dy + 1)  (2-D: dy + 1)
  const int dz = DIMS == 3 ? trow / 3 - 1 : 0;
  const int dy = DIMS == 0 ? 0 : trow % 3 - 1;
  const int t_begin = blockIdx.z * run, t_end = min(t_begin + run, ntiles);
  const bool vx = (Cin & 3) == 0, vg = (Cout & 3) == 0;
  const long rows = (long)N * D * H * W;

  f32x4 acc[G][4][4];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[g][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int t = t_begin; t < t_end; ++t) {
    int bx = 0, by = 0, z = 0, n = 0;
    if (DIMS != 0) {
      int r = t;
      bx = r % tiles_x; r /= tiles_x;
      by = r % tiles_y; r /= tiles_y;
      z = r % D; n = r / D;
    }
    // gpre tile: 64 voxels x 16 channel quads
    for (int s = tid; s < WW_GROWS * 16; s += 256) {
      const int vl = s >> 4, q = s & 15;
      long gv;
      bool ok;
      if (DIMS == 0) {
        gv = (long)t * WW_GROWS + vl;
        ok = gv < rows;
      } else {
        const int gy = by * WW_TY + (vl >> 4), gx = bx * WW_TX + (vl & 15);
        ok = gy < H && gx < W;
        gv = (((long)n * D + z) * H + gy) * W + gx;
      }
      *(f32x4*)(gs + vl * WW_RS + 4 * q) = ww_load(gp, gv, Cout, co0 + 4 * q, ok, vg);
    }
    // x: the same 64 rows (dims 0) or the halo row (4 x 18 voxels at z + dz, rows + dy, columns - 1 .. 16)
    const int xrows = DIMS == 0 ? WW_GROWS : WW_XROWS;
    for (int s = tid; s < xrows * 16; s += 256) {
      const int hv = s >> 4, q = s & 15;
      long gv;
      bool ok;
      if (DIMS == 0) {
        gv = (long)t * WW_GROWS + hv;
        ok = gv < rows;
      } else {
        const int ly = hv / WW_HX, lx = hv - ly * WW_HX;
        const int sy = by * WW_TY + ly + dy, sx = bx * WW_TX + lx - 1, sz = z + dz;
        ok = (unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H && (unsigned)sz < (unsigned)D;
        gv = (((long)n * D + sz) * H + sy) * W + sx;
      }
      *(f32x4*)(xs + hv * WW_RS + 4 * q) = ww_load(x, gv, Cin, ci0 + 4 * q, ok, vx);
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {                            // 4 voxels of the wave's row per step: lane (m, k) -> voxel 4ks + k
      const int c = 4 * ks + k;
      const float* ga = gs + (wave * WW_TX + c) * WW_RS + m;
      float a[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = ga[16 * i];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float* xb = xs + (DIMS == 0 ? (wave * WW_TX + c) : (wave * WW_HX + c + g)) * WW_RS + m;
        float b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = xb[16 * j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[g][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[g][i][j], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // per tap: the four waves' 64 x 64 sums through LDS, (w0 + w1) + (w2 + w3), one coalesced partial
  float* red = wlds;
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave * 4096 + (16 * i + 4 * k + e) * 64 + 16 * j + m] = acc[g][i][j][e];   // D[co][ci]
    __syncthreads();
    const int tap = DIMS == 0 ? 0 : trow * 3 + g;
    float* dst = partial + (((long)blockIdx.z * taps + tap) * ntp + tp) * 4096;
    for (int o = tid; o < 4096; o += 256) dst[o] = (red[o] + red[4096 + o]) + (red[8192 + o] + red[12288 + o]);
    __syncthreads();
  }
}

// gw[tap][co][ci] = scale * sum over the runs in order, in fp64.  grid (16, tile pairs, taps): one output per thread
__global__ void __launch_bounds__(256) wgrad_wide_reduce_kernel(const float* __restrict__ partial, float* __restrict__ gw, int nruns,
                                                                int taps, int ntp, int ncit, int Cin, int Cout, float scale) {
  const int o = blockIdx.x * 256 + threadIdx.x, tp = blockIdx.y, tap = blockIdx.z;
  const int ct = tp / ncit, cit = tp - ct * ncit;
  const int co = ct * 64 + (o >> 6), ci = cit * 64 + (o & 63);
  if (co >= Cout || ci >= Cin) return;
  const long stride = (long)taps * ntp * 4096;
  const float* src = partial + ((long)tap * ntp + tp) * 4096 + o;
  double s = 0.0;
  int b = 0;
  for (; b + 8 <= nruns; b += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(long)(b + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += (double)v[u];
  }
  for (; b < nruns; ++b) s += (double)src[(long)b * stride];
  gw[((long)tap * Cout + co) * Cin + ci] = (float)(s * (double)scale);
}

struct WideWgradPlan { int taps, trows, nct, ncit, tiles_x, tiles_y, ntiles, run, nruns; };

bool wide_wgrad_plan(int dims, int N, int D, int H, int W, int Cin, int Cout, WideWgradPlan& p) {
  if (dims != 0 && dims != 2 && dims != 3) return false;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin < 16 || Cout < 16) return false;
  const long rows = (long)N * D * H * W;
  if (rows >= 0x7fffffffL || (long)Cin * rows >= (1L << 47) || (long)Cout * rows >= (1L << 47)) return false;
  p.taps = dims == 3 ? 27 : (dims == 2 ? 9 : 1);
  p.trows = dims == 3 ? 9 : (dims == 2 ? 3 : 1);
  p.nct = (Cout + 63) / 64;
  p.ncit = (Cin + 63) / 64;
  long ntiles;
  if (dims == 0) {
    p.tiles_x = p.tiles_y = 1;
    ntiles = (rows + WW_GROWS - 1) / WW_GROWS;
  } else {
    p.tiles_x = (W + WW_TX - 1) / WW_TX;
    p.tiles_y = (H + WW_TY - 1) / WW_TY;
    ntiles = (long)p.tiles_x * p.tiles_y * D * N;
  }
  if (ntiles >= 0x7fffffffL || (long)p.nct * p.ncit > 65535) return false;
  p.ntiles = (int)ntiles;
  long run = WW_RUN0;
  while ((ntiles + run - 1) / run > WW_MAXRUNS) run *= 2;
  // small problems: shorter runs until there are WW_MINWGS workgroups (8 x 8 images of 8 views, 2048-row pointwise layers:
  // 48 - 128 workgroups at 16 tiles per run left the chip idle and ran slower than lf_conv_bwd_weight)
  while (run > 1 && (long)p.nct * p.ncit * p.trows * ((ntiles + run - 1) / run) < WW_MINWGS) run /= 2;
  p.run = (int)run;
  p.nruns = (int)((ntiles + run - 1) / run);
  return true;
}

size_t wide_wgrad_scratch(const WideWgradPlan& p) {
  return (size_t)p.nruns * p.taps * p.nct * p.ncit * 4096 * sizeof(float);
}

}  // namespace

extern "C" size_t lf_conv_bwd_weight_wide_scratch_bytes(int dims, int N, int D, int H, int W, int Cin, int Cout) {
  WideWgradPlan p;
  if (!wide_wgrad_plan(dims, N, D, H, W, Cin, Cout, p)) return 0;
  return wide_wgrad_scratch(p);
}

extern "C" int lf_conv_bwd_weight_wide(const float* x, const float* gpre, float* gw, void* scratch, size_t scratch_bytes,
                                       int dims, int N, int D, int H, int W, int Cin, int Cout, float scale, void* stream) {
  lf_clear_error();
  if (x == nullptr || gpre == nullptr || gw == nullptr || scratch == nullptr) return LF_EINVAL;
  WideWgradPlan p;
  if (!wide_wgrad_plan(dims, N, D, H, W, Cin, Cout, p)) return LF_EINVAL;
  if (!lf_aligned16(x) || !lf_aligned16(gpre) || !lf_aligned16(gw) || !lf_aligned16(scratch)) return LF_EALIGN;
  if (scratch_bytes < wide_wgrad_scratch(p)) return LF_ENOSPC;
  typedef void (*kern_t)(const float*, const float*, float*, int, int, int, int, int, int, int, int, int, int, int, int);
  const kern_t kern = dims == 3 ? wgrad_wide_kernel<3> : (dims == 2 ? wgrad_wide_kernel<2> : wgrad_wide_kernel<0>);
  static lf_devmask_t attr_set[3];
  {
    hipError_t e = lf_ensure_dyn_lds(attr_set[dims == 3 ? 2 : (dims == 2 ? 1 : 0)], (const void*)kern, WW_LDS);
    if (e != hipSuccess) return (int)e;
  }
  hipStream_t s = (hipStream_t)stream;
  const int ntp = p.nct * p.ncit;
  hipLaunchKernelGGL(kern, dim3(ntp, p.trows, p.nruns), dim3(256), WW_LDS, s, x, gpre, (float*)scratch, N, D, H, W, Cin, Cout,
                     p.tiles_x, p.tiles_y, p.ntiles, p.run, p.ncit, p.taps);
  int st = lf_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(wgrad_wide_reduce_kernel, dim3(16, ntp, p.taps), dim3(256), 0, s, (const float*)scratch, gw, p.nruns, p.taps,
                     ntp, p.ncit, Cin, Cout, scale);
  return lf_launch_status();
}
