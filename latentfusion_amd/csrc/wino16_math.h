// What the Winograd 16-channel kernels (conv_wino.hip, which describes the organisation) use as plain C++ below the MFMA
// phase: the build switches of the A/B tools, the tile / halo / LDS geometry, the barrier, the DPP and reciprocal helpers, the
// packed fp32 add / subtract with the wait-state rules R1 - R3, and the pinned epilogue roundings of the fixed forms.  The MFMA
// phase itself is wino16_compute.h.
#pragma once
#include "lf_common.h"

// ---- Build switches (-D... on the command line of the A/B tools; the library is built with none of them).  Every bit the
// code tests is described here and nowhere else. ----
//
// WINO_ABL: ablations for tools/wino_ab.py and the cycle stamps for tools/wino_timeline.py.  With any bit but 16 / 32 the
// results are WRONG: timings only.
//    1   no epilogue arithmetic: the exchanged sums are stored as they are (upper bound on what moving the epilogue to other
//        waves could give: they would still issue it on the shared pipe)
//    2   no z-frequency exchange / z output transform: each wave stores from its own partials
//    4   every MFMA chain 1.5x as long (the MFMA count of F(2,3) in y,x with direct z taps)
//    8   f16x3 kernel only: timing proxy of a THREE-piece split -- a third f16 piece of every B operand and six product terms
//        instead of three
//   16   cycle stamps TS(k): lane 0 of every wave of workgroup 11 writes the cycle counter at the phase boundaries of
//        each tile into norm_out (16 unsigned per wave and tile, slots 0 - 8; the PixelNorm denominators are not stored then)
//   32   with 16: cycle stamps CTS(k) inside the MFMA phase (wino_compute), slots 9 - 12 of the same record: behind the halo
//        reads / input transforms and behind the partial stores of each of the two 16-tile groups
//   64   one LDS read per value and no z combination (upper bound on staging z-COMBINED planes in LDS)
#ifndef WINO_ABL
#define WINO_ABL 0
#endif
#define TS(k) do { if ((WINO_ABL & 16) && blockIdx.x == 11 && lane == 0) ((unsigned*)norm_out)[((t - t_begin) * 4 + fa) * 16 + (k)] = (unsigned)__builtin_readcyclecounter(); } while (0)
#define CTS(k) do { if ((WINO_ABL & 32) && tsp != nullptr) tsp[k] = (unsigned)__builtin_readcyclecounter(); } while (0)
// WINO_PJ_ABL: ablations of the fused projection backward (wino16_projbwd.inc; tools/proj_fuse_ab.py --variants,
// tools/projbwd_ab.py; results WRONG, timings only):
//    1   no activation / norm loads (the HBM streams of the halo phase)
//    2   no MFMAs / epilogue arithmetic
//    4   no slide copy
#ifndef WINO_PJ_ABL
#define WINO_PJ_ABL 0
#endif
// WINO_PL / WINO_PM / WINO_PN: wave priorities (s_setprio) of the three phases of a tile: halo reads + input transforms
// (latency-bound: LDS), the MFMA chains (throughput-bound) and the exchange / epilogue / halo fetch (latency-bound: LDS, HBM)
#ifndef WINO_PL
#define WINO_PL 2
#endif
#ifndef WINO_PM
#define WINO_PM 1
#endif
#ifndef WINO_PN
#define WINO_PN 3
#endif

namespace {

constexpr int TZw = 2, TYw = 8, TXw = 16;
constexpr int HZw = TZw + 2, HYw = TYw + 2, HXw = TXw + 2;     // 4 x 10 x 18 halo (720 voxels)
constexpr int HALFw = 2 * HYw * HXw;                            // 360 voxels: two z planes of the halo
constexpr int HALFBw = HALFw * 64;                              // 23,040 B
constexpr int NSLOTw = (HALFw * 4 + 63) / 64;                   // 23 pieces of 1 KiB per half (the last one half full)
constexpr int NITw = (NSLOTw + 3) / 4;                          // 6 pieces per wave and half
constexpr int BUFw = 2 * HALFBw;                                // 46,080 B halo buffer
// z-staged forms (ZST, conv_wino.hip section 6): the same buffer as four z-FREQUENCY planes of 180 voxel slots
constexpr int PLANEw = HYw * HXw;                               // 180 voxels: one plane of the halo
constexpr int PLANEBw = PLANEw * 64;                            // 11,520 B
constexpr int NITZw = ((PLANEw * 4 + 63) / 64 + 3) / 4;         // 12 pieces of 1 KiB per plane (the last a quarter full): 3 per wave
static_assert(4 * PLANEBw == BUFw && 2 * NITZw == NITw, "the staged forms reuse the halo buffer and the fetch registers");
constexpr int PXw = 4 * 8192;                                   // 32,768 B partial-exchange region
constexpr int LDSw = BUFw + PXw + 1024;                         // + 1 KiB DMA scratch = 79,872 B (two workgroups per CU)

__device__ __forceinline__ void lds_barrier() {
  // all LDS traffic of this wave retired, then workgroup barrier; global loads/stores and the LDS-DMA of
  // the next tile stay in flight (a __syncthreads() would drain vmcnt as well)
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// sum over the four lanes of a quad (4q .. 4q+3) with DPP quad_perm, same value in all four
__device__ __forceinline__ float quad_sum(float v) {
  const float a = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));   // [1,0,3,2]
  return a + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0x4E, 0xF, 0xF, true));            // [2,3,0,1]
}

// v_rsq_f32 / v_rcp_f32 (1 ulp) + one Newton step
__device__ __forceinline__ float fast_rsqrt(float x) {
  const float r = __builtin_amdgcn_rsqf(x);
  return r * (1.5f - 0.5f * x * r * r);
}
__device__ __forceinline__ float fast_rcp(float x) {
  const float r = __builtin_amdgcn_rcpf(x);
  return r * (2.f - x * r);
}

// a - b as two v_pk_add_f32 with negated second source.  (LLVM packs <4 x float> fadd into v_pk_add_f32 but
// scalarises fsub; on this kernel every VALU instruction competes with the fp32 MFMAs for the issue pipe: a packed
// add costs 1.2x a scalar one there and does the work of two, profiles/wino_pack_rates.txt.)
// The compiler pads MFMA <-> VALU wait states only between instructions it can see, and it does not look inside asm.
// pk_sub itself is for operands that are not MFMA results and results that do not feed an MFMA.  The forms next to
// an MFMA (wino_rows_packed, wino16_compute.h) keep the wait states by construction; the rules, read from the compiler's own
// padding of the scalar form (ROCm 7.2, gfx950):
//   R1  VALU write -> v_mfma_f32_16x16x4_f32 reading it as B: 2 wait states.  The packed values of an MFMA pair pass
//       through pk_fence (an `s_nop 1` every producer feeds and every MFMA of the pair reads from).
//   R2  v_mfma_f32_16x16x4_f32 result -> VALU read: 10 wait states (40 clk).  The MFMA holds the pipe for 8 passes (32 clk),
//       so an instruction behind TWO later MFMAs of the same wave is >= 64 clk behind the result's MFMA; sched_barrier(0)
//       on both sides of those two MFMAs keeps the reader behind them.  The last row of a group has no later MFMA: its
//       readers sit behind a compiler-visible read of the same registers, which the compiler pads, and take that read's
//       value as an operand (`gate`).
//   R3  VALU write over a register an MFMA in flight still reads: every packed op here writes IN PLACE over its first
//       source (a transform value no MFMA reads, or an accumulator whose MFMAs have retired by R2), so the register
//       allocator never hands an asm result a register that an MFMA has just released.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x4 pk_sub(f32x4 a, f32x4 b) {
  f32x2 lo, hi;
  const f32x2 alo = {a[0], a[1]}, ahi = {a[2], a[3]}, blo = {b[0], b[1]}, bhi = {b[2], b[3]};
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(alo), "v"(blo));
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(ahi), "v"(bhi));
  return (f32x4){lo[0], lo[1], hi[0], hi[1]};
}

// a -= b / a += b in place, two packed instructions each (R3 above); `gate` is an ordering operand only (R2)
__device__ __forceinline__ void pk_sub_to(f32x4& a, const f32x4 b, int gate = 0) {
  f32x2 alo = {a[0], a[1]}, ahi = {a[2], a[3]};
  const f32x2 blo = {b[0], b[1]}, bhi = {b[2], b[3]};
  asm("v_pk_add_f32 %0, %0, %1 neg_lo:[0,1] neg_hi:[0,1]" : "+v"(alo) : "v"(blo), "s"(gate));
  asm("v_pk_add_f32 %0, %0, %1 neg_lo:[0,1] neg_hi:[0,1]" : "+v"(ahi) : "v"(bhi), "s"(gate));
  a = (f32x4){alo[0], alo[1], ahi[0], ahi[1]};
}
__device__ __forceinline__ void pk_add_to(f32x4& a, const f32x4 b, int gate = 0) {
  f32x2 alo = {a[0], a[1]}, ahi = {a[2], a[3]};
  const f32x2 blo = {b[0], b[1]}, bhi = {b[2], b[3]};
  asm("v_pk_add_f32 %0, %0, %1" : "+v"(alo) : "v"(blo), "s"(gate));
  asm("v_pk_add_f32 %0, %0, %1" : "+v"(ahi) : "v"(bhi), "s"(gate));
  a = (f32x4){alo[0], alo[1], ahi[0], ahi[1]};
}
// R1: both B operands of an MFMA pair pass through here after their last packed write
__device__ __forceinline__ void pk_fence(f32x4& a, f32x4& b) { asm("s_nop 1" : "+v"(a), "+v"(b)); }

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// The epilogue arithmetic of the fixed forms (WF_*, wino16_compute.h), spelled out.  The generic kernels leave fp
// contraction to the compiler, and which products it fuses into v_fma / v_pk_fma depends on the code around them: with the
// runtime tests folded away the same source lines come out with OTHER fusions (sum of squares without fmas, every
// `v - yp * dot` fused, ...) and the results differ in the last bit.  These functions pin, with contraction off, exactly the
// roundings the generic kernels are compiled to; tests/test_wino_forms_gpu.py holds the two together bit for bit, so a
// compiler that changes its mind about the generic kernels shows there.  To re-derive the pattern then: the device listing of
// conv_wino.hip (command line in tools/wino_isa_count.py), kernel conv3d_c16_wino_kernel<true>, behind its last v_mfma: the block
// with v_rsq_f32 is the forward epilogue (which product opens the v_fmac chain of the sum of squares, whether the Newton step is
// a v_fmaak), the block with v_rcp_f32 the previous layer's backward (which of the four `v - yp * dot` are v_pk_fma and which a
// v_mul + v_pk_add neg; whether 2 - pn * r is a v_sub); conv3d_c16_wino_projfwd_kernel<true> has the forward block once more.
// quad_sum with its two instructions pinned: the compiler is free to split a step into v_mov_dpp + v_add with the operands the
// other way round, which hands on the OTHER lane's NaN where both are NaNs (sign and payload; found by the NaN case of the
// test).  (s_nop 4: the compiler cannot pad hazards inside asm; five wait states cover a DPP read behind a VALU write of the
// register, 2, and behind a VALU write of EXEC, 5.)
__device__ __forceinline__ float quad_sum_pinned(float v) {
  float a, b;
  asm("s_nop 4\n\tv_add_f32_dpp %0, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(a) : "v"(v));
  asm("s_nop 4\n\tv_add_f32_dpp %0, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1" : "=v"(b) : "v"(a));
  return b;
}
//   forward block: u = fma(scale, o, b); LeakyReLU as max(u, u * slope); ss = fma(u3, u3, fma(u2, u2, fma(u0, u0, u1 * u1)));
//                  tq = fma(quad_sum(ss), 1/16, eps); rinv = r * fma(r, (-0.5 tq) r, 1.5), r = v_rsq(tq)
__device__ __forceinline__ void wino_epi_fwd_block(const f32x4 o, const f32x4 b, float scale, float slope, float eps,
                                                   f32x4& v, float& rn) {
#pragma clang fp contract(off)
  f32x4 u;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float t = __builtin_fmaf(scale, o[e], b[e]);
    u[e] = fmaxf(t, t * slope);
  }
  const float ss = __builtin_fmaf(u[3], u[3], __builtin_fmaf(u[2], u[2], __builtin_fmaf(u[0], u[0], u[1] * u[1])));
  const float tq = __builtin_fmaf(quad_sum_pinned(ss), 1.f / 16.f, eps);
  const float r = __builtin_amdgcn_rsqf(tq);
  const float rinv = r * __builtin_fmaf(r, (-0.5f * tq) * r, 1.5f);
  rn = tq * rinv;
  v = u * rinv;
}
//   previous layer's PixelNorm' / LeakyReLU': plain products and sums for v = o * scale, the dot product and the Newton step
//   of the reciprocal; `v - yp * dot` fused for channels 0, 1 of the quarter and not for 2, 3
__device__ __forceinline__ f32x4 wino_epi_dgrad_prev(const f32x4 o, const f32x4 yp, float pn, float scale, float slope) {
#pragma clang fp contract(off)
  f32x4 v = o * scale;
  const float dot = quad_sum_pinned(((v[0] * yp[0] + v[1] * yp[1]) + v[2] * yp[2]) + v[3] * yp[3]) * (1.f / 16.f);
  const float r = __builtin_amdgcn_rcpf(pn);
  const float rinv = r * (2.f - pn * r);
  v[0] = __builtin_fmaf(-yp[0], dot, v[0]) * rinv;
  v[1] = __builtin_fmaf(-yp[1], dot, v[1]) * rinv;
  v[2] = (v[2] - yp[2] * dot) * rinv;
  v[3] = (v[3] - yp[3] * dot) * rinv;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = yp[e] > 0.f ? v[e] : v[e] * slope;
  return v;
}
//   plain data gradient: fma(scale, o, +0) -- the generic kernel's `o * scale + bias` with the zero it holds for a missing
//   bias (a product of -0 comes out as +0)
__device__ __forceinline__ f32x4 wino_epi_dgrad_plain(const f32x4 o, float scale) {
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(scale, o[e], 0.f);
  return v;
}

}  // namespace
