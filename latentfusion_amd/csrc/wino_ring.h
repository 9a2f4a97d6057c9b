// What the wide Winograd convolutions (wino_fused.hip, wino_fused_f16x3.hip, wino_gemm.hip) share as C++: the value helpers of
// the fused GEMM kernels' skeleton (the skeleton itself is text: wino_ring.inc), the body of their finish kernels, the host
// side of a fused-GEMM launch, and the column step of the F(2,3) input transforms (the patch load and row step: wino_xform.inc).
#pragma once
#include "lf_common.h"

namespace wino_ring {

constexpr int KC = 32;      // input channels per stage
constexpr int NSTAGE = 4;   // LDS ring depth (stages of A + B chunks); a power of two

typedef unsigned u32;

// byte offset of 16-byte chunk c (0..7) of row r in a rows x 128-byte LDS tile
__device__ __forceinline__ int lds_chunk(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

// A^T = [[1, 1, 1, 0], [0, 1, -1, -1]]: coefficient of frequency component a in output o
__device__ __forceinline__ float at_coef(int o, int a) {
  return o == 0 ? (a < 3 ? 1.f : 0.f) : (a == 0 ? 0.f : (a == 1 ? 1.f : -1.f));
}

// Before stage s of S is read, with ahead = min(NSTAGE - 2, S - 1 - s) later stages issued: this wave's pieces of stage s have
// landed when at most the pieces of those later stages are outstanding (PPW DMA instructions per stage and wave); then the
// workgroup barrier makes every wave's pieces visible AND certifies that everybody is done reading stage s-1, whose ring slot
// the next issue overwrites
template <int PPW>
__device__ __forceinline__ void wait(int ahead) {
  if (ahead >= 2) __builtin_amdgcn_s_waitcnt(0x0f70 | ((2 * PPW) & 15) | (((2 * PPW) >> 4) << 14));     // vmcnt(2 PPW), the rest open
  else if (ahead == 1) __builtin_amdgcn_s_waitcnt(0x0f70 | (PPW & 15));                                  // vmcnt(PPW)
  else __builtin_amdgcn_s_waitcnt(0x0f70);                                                                // vmcnt(0)
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// Element i (a channel quad) of a frequency-split launch's output: the zs partials added in a fixed order, then the epilogue of
// the direct store (for the forms without a per-tile exponent)
template <class Epi>
__device__ __forceinline__ f32x4 finish_value(const f32x4* __restrict__ partial, const float* __restrict__ bias, long i, long ysize4,
                                              int zs, int c4, Epi& epi) {
  f32x4 acc = partial[i];
  for (int z = 1; z < zs; ++z) acc += partial[i + z * ysize4];
  f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr) bv = *(const f32x4*)(bias + (i % c4) * 4);
  return epi(acc, bv, 0);
}

// ---- F(2,3) input transforms (wino_xform.inc) ----
// frequency (y b, x c) of a channel quad from its row-transformed patch vx[dy][c]: the transform d0-d2, d1+d2, d2-d1, d1-d3 down
// the columns
#define WINO_XFORM_COL(vx, b, c) \
  (((b) == 0) ? (vx[0][c] - vx[2][c]) : ((b) == 1) ? (vx[1][c] + vx[2][c]) : ((b) == 2) ? (vx[2][c] - vx[1][c]) : (vx[1][c] - vx[3][c]))

// ---- host side of a fused-GEMM launch ----
// Winograd tiles of 2 x 2 (x 2) outputs over N samples
struct Tiles {
  int tz, ty, tx;
  long T;
  Tiles(int dims, int N, int D, int H, int W) : tz(dims == 3 ? (D + 1) / 2 : 1), ty((H + 1) / 2), tx((W + 1) / 2), T((long)N * tz * ty * tx) {}
};

// Grid and frequency split of one launch: Plan p(...); p.split(F, MT, NT, want); p.check(K, scratch, bytes) == 0; then grid() and
// partial go to the kernel, and with zs > 1 the finish kernel runs behind it (finish)
struct Plan : Tiles {
  int CoutP, gy = 0, zs = 1;
  long gx = 0, ysize;
  float* partial = nullptr;
  Plan(int dims, int N, int D, int H, int W, int Cout)
      : Tiles(dims, N, D, H, W), CoutP(lf_wino_fused_cout_padded(Cout)), ysize((long)N * D * H * W * Cout) {}
  // workgroups of MT tiles x NT output channels; a small problem is split over the F frequencies until `want` workgroups exist
  void split(int F, int MT, int NT, long want) {
    gx = (T + MT - 1) / MT, gy = (CoutP + NT - 1) / NT;
    for (zs = 1; zs < F && gx * gy * zs < want;) zs <<= 1;
  }
  size_t scratch_bytes() const { return zs > 1 ? (size_t)zs * ysize * sizeof(float) : 0; }
  // K: row length of V and U2 in 4-byte units (32-bit byte offsets inside one frequency slab)
  int check(int K, void* scratch, size_t bytes) {
    if (T * K * 4 > 0xffffffffL || (long)CoutP * K * 4 > 0xffffffffL) return LF_EINVAL;
    if (gx > 0x7fffffffL || gy > 65535) return LF_EINVAL;
    if (zs > 1 && (scratch == nullptr || bytes < scratch_bytes() || !lf_aligned16(scratch))) return LF_ENOSPC;
    partial = zs > 1 ? (float*)scratch : nullptr;
    return 0;
  }
  dim3 grid() const { return dim3((unsigned)gx, (unsigned)gy, (unsigned)zs); }
};

// one launch of GEMM kernel Kern with `lds` bytes of dynamic LDS (the attribute is set once per kernel and device)
template <auto Kern, class... Args>
int launch(dim3 grid, int threads, int lds, hipStream_t s, Args... args) {
  static lf_devmask_t attr_set;
  const hipError_t e = lf_ensure_dyn_lds(attr_set, (const void*)Kern, lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(Kern, grid, dim3(threads), lds, s, args...);
  return lf_launch_status();
}

// the finish kernel of a frequency-split launch: Kern(partial, bias, y, n4, args...) over the n4 = ysize / 4 channel quads
template <auto Kern, class... Args>
int finish(const Plan& p, hipStream_t s, const float* bias, float* y, Args... args) {
  const long n4 = p.ysize / 4;
  hipLaunchKernelGGL(Kern, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const f32x4*)p.partial, bias, (f32x4*)y, n4, args...);
  return lf_launch_status();
}

}  // namespace wino_ring
