// The MFMA phase of the Winograd 16-channel kernels (conv_wino.hip): wino_compute, one wave's z-frequency of one tile from
// the halo in LDS to its partial outputs in the exchange region, with its packed row form wino_rows_packed; and what the
// kernels' body is parameterised by: the argument block of the fused projection forms (WinoProj, tr_swz) and the fixed
// epilogue forms WF_*.
#pragma once
#include "wino16_math.h"

namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// The MFMA phase of one 16-tile group in the packed form: rows b = 0..3 of the y input transform, their 16 MFMAs each
// and the x / y output transforms, as eight MFMA pairs p = (b, cp) of 2 x 4 chained MFMAs.  Per pair:
//   [barrier] the pair's first two MFMAs [barrier] output-transform ops on the PREVIOUS pair's results (R2: two MFMAs
//   behind them), B operands of the NEXT pair (in place, fenced: R1, R3), the pair's other six MFMAs.
// Between the barriers the compiler schedules freely.
__device__ __forceinline__ void wino_rows_packed(f32x4 (&vx)[4][4], const float (&wt)[64], f32x4 (&Yg)[4]) {
  f32x4 m[4][4];                                               // [b][c]
  f32x4 vb[8][2];                                              // B operands of pair p
  auto operands = [&](int p) {
    const int b = p >> 1, cp = (p & 1) * 2;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = cp + h;
      if (b == 0) { pk_sub_to(vx[0][c], vx[2][c]); vb[p][h] = vx[0][c]; }      // vx[0] is not read again
      if (b == 1) vb[p][h] = vx[1][c] + vx[2][c];                             // (compiler-visible: padded by the compiler)
      if (b == 2) { pk_sub_to(vx[2][c], vx[1][c]); vb[p][h] = vx[2][c]; }      // vx[2] is not read again
      if (b == 3) { pk_sub_to(vx[1][c], vx[3][c]); vb[p][h] = vx[1][c]; }
    }
    if (b != 1) pk_fence(vb[p][0], vb[p][1]);
  };
  // x output transform t0 = (m0 + m1) + m2, t1 = (m1 - m2) - m3 of row b, then the y output transform accumulates
  auto row_first = [&](int b) { pk_add_to(m[b][0], m[b][1]); };                // m0 <- m0 + m1
  auto row_rest = [&](int b, int gate = 0) {
    pk_add_to(m[b][0], m[b][2], gate);                                        // t0
    pk_sub_to(m[b][1], m[b][2], gate);
    pk_sub_to(m[b][1], m[b][3], gate);                                        // t1
    const f32x4 t0 = m[b][0], t1 = m[b][1];
    if (b == 0) { Yg[0] = t0; Yg[1] = t1; }
    if (b == 1) { pk_add_to(Yg[0], t0); pk_add_to(Yg[1], t1); Yg[2] = t0; Yg[3] = t1; }
    if (b == 2) { pk_add_to(Yg[0], t0); pk_add_to(Yg[1], t1); pk_sub_to(Yg[2], t0); pk_sub_to(Yg[3], t1); }
    if (b == 3) { pk_sub_to(Yg[2], t0); pk_sub_to(Yg[3], t1); }
  };
  operands(0);
#pragma unroll
  for (int p = 0; p < 8; ++p) {
    const int b = p >> 1, cp = (p & 1) * 2;
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int h = 0; h < 2; ++h)
      m[b][cp + h] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[(b * 4 + cp + h) * 4], vb[p][h][0], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (p > 0) {
      if (p & 1) row_first(b);
      else row_rest(b - 1);
    }
    if (p < 7) operands(p + 1);
#pragma unroll
    for (int i = 1; i < 4; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        m[b][cp + h] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[(b * 4 + cp + h) * 4 + i], vb[p][h][i], m[b][cp + h], 0, 0, 0);
    if constexpr ((WINO_ABL & 4) != 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h)
          m[b][cp + h] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[(b * 4 + cp + h) * 4 + i], vb[p][h][i], m[b][cp + h], 0, 0, 0);
    }
  }
  // R2, last row: no later MFMA to stand behind.  One compiler-visible VALU read of each of the two last results (the
  // compiler pads it and then knows the results have landed); every packed op that reads them takes that read's value
  // as an operand, so it cannot be scheduled ahead of it.
  const int landed = __builtin_amdgcn_readfirstlane(__float_as_int(m[3][2][0])) | __builtin_amdgcn_readfirstlane(__float_as_int(m[3][3][0]));
  row_rest(3, landed);
}

// SPLIT = false: all-fp32 products, wt = U[a][(b,c)][k-chunk] for v_mfma_f32_16x16x4_f32.
// SPLIT = true : every Winograd-domain product U.V from three v_mfma_f32_16x16x16_f16 accumulating in fp32,
//                U_hi.V_hi + U_hi.V_lo + U_lo.V_hi  (x = x_hi + x_lo, both f16; dropped term <= 2^-22 |U||V|);
//                whi / wlo = the two halves of U, V is split on the fly after scaling by the power of two in_scale.
// OFFX (the fused forms, which have no registers to spare): only off[r][0] is kept; the rows dy = 2, 3, whose quarter
// swizzle differs in bit 0, derive their offset with one v_xor per read instead of a second register per residue.
// PACK (all-fp32 path only): the y input transform that feeds the B operands and the x / y output transforms on the MFMA
// results as packed asm (rules R1 - R3 at pk_sub), same operations in the same order and association as the scalar
// form, which stays selectable (lf_set_tuning key 7) for the bit-identity test and the A/B.
// ZST (z-staged fixed forms): the halo buffer holds z-FREQUENCY planes (halo_commit combined them once per halo point), so
// plane A is read as it is: one ds_read_b128 per value instead of two and no z combination here.
template <int A, bool SPLIT, bool OFFX = false, bool PACK = false, bool ZST = false>
__device__ __forceinline__ void wino_compute(const unsigned char* __restrict__ buf, const int (&off)[8][2],
                                              const float (&wt)[64], const f16x4 (&whi)[16], const f16x4 (&wlo)[16],
                                              float in_scale, unsigned char* __restrict__ pdst,
                                              const int (&pw)[2], unsigned* tsp = nullptr) {
  // z input transform of frequency A: d0-d2, d1+d2, d2-d1, d1-d3
  constexpr int DZ0 = (A == 0) ? 0 : (A == 2 ? 2 : 1);
  constexpr int DZ1 = (A == 0) ? 2 : (A == 1 ? 2 : (A == 2 ? 1 : 3));
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    f32x4 Yg[4];                                              // (j, i) outputs of this group, z-frequency A
    f32x4 vx[4][4];                                           // [dy][x-frequency c]
    // the halo is read half a row (2 z planes x 2 x positions = 4 ds_read_b128) ahead of the half row being
    // transformed; the fences stop the scheduler from folding this back into load-wait-use pairs, which
    // exposes the full LDS latency sixteen times per group
    f32x4 raw[2][ZST ? 2 : 4];
    auto load_half = [&](int hh, f32x4 (&r)[ZST ? 2 : 4]) {
      const int dy = hh >> 1;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int dx = (hh & 1) * 2 + e;
        const int ca = ((DZ0 * 10 + 4 * g + dy) * 18 + (dx & 1) * 9 + (dx >> 1));
        if constexpr (ZST) {                                   // the frequency index takes the place of z in the slot
          const int cf = ca + (A - DZ0) * 180;
          if constexpr (OFFX) {
            int oa = off[cf & 7][0];
            if (dy >> 1) {
              asm volatile("" : "+v"(oa));
              oa ^= 16;
            }
            r[e] = *(const f32x4*)(buf + oa + cf * 64);
          } else {
            r[e] = *(const f32x4*)(buf + off[cf & 7][dy >> 1] + cf * 64);
          }
        } else {
          const int cb = ((DZ1 * 10 + 4 * g + dy) * 18 + (dx & 1) * 9 + (dx >> 1));
          if constexpr ((WINO_ABL & 64) != 0) {                  // ablation: ONE plane read per value, no z combination
            r[2 * e] = *(const f32x4*)(buf + off[ca & 7][dy >> 1] + ca * 64);
            r[2 * e + 1] = r[2 * e];
          } else if constexpr (OFFX) {
            int oa = off[ca & 7][0], ob = off[cb & 7][0];
            if (dy >> 1) {
              asm volatile("" : "+v"(oa), "+v"(ob));               // (opaque: or the xor-ed copies are hoisted back into registers)
              oa ^= 16;
              ob ^= 16;
            }
            r[2 * e] = *(const f32x4*)(buf + oa + ca * 64);
            r[2 * e + 1] = *(const f32x4*)(buf + ob + cb * 64);
          } else {
            r[2 * e] = *(const f32x4*)(buf + off[ca & 7][dy >> 1] + ca * 64);
            r[2 * e + 1] = *(const f32x4*)(buf + off[cb & 7][dy >> 1] + cb * 64);
          }
        }
      }
    };
    __builtin_amdgcn_s_setprio(WINO_PL);
    load_half(0, raw[0]);
    f32x4 d[4];
#pragma unroll
    for (int hh = 0; hh < 8; ++hh) {
      if (hh < 7) load_half(hh + 1, raw[(hh + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
      const int dy = hh >> 1;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        if constexpr (ZST) {
          d[(hh & 1) * 2 + e] = raw[hh & 1][e];
        } else {
          const f32x4 va = raw[hh & 1][2 * e], vb = raw[hh & 1][2 * e + 1];
          if constexpr ((WINO_ABL & 64) != 0) d[(hh & 1) * 2 + e] = va;
          else d[(hh & 1) * 2 + e] = (A == 1) ? (va + vb) : pk_sub(va, vb);
        }
      }
      if (hh & 1) {
        vx[dy][0] = pk_sub(d[0], d[2]);
        vx[dy][1] = d[1] + d[2];
        vx[dy][2] = pk_sub(d[2], d[1]);
        vx[dy][3] = pk_sub(d[1], d[3]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    CTS(9 + 2 * g);
    __builtin_amdgcn_s_setprio(WINO_PM);
    if constexpr (PACK && !SPLIT) {
      wino_rows_packed(vx, wt, Yg);
    } else {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        f32x4 m[4];
        // two frequencies of the row advance together, one k-chunk at a time: a 16x16x4 f32 MFMA can issue every
        // 32 cycles but its result feeds a dependent one only after 40, so a single back-to-back chain would bubble
#pragma unroll
        for (int cp = 0; cp < 4; cp += 2) {
          f32x4 v[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int c = cp + h;
            v[h] = (b == 0) ? (vx[0][c] - vx[2][c])
                 : (b == 1) ? (vx[1][c] + vx[2][c])
                 : (b == 2) ? (vx[2][c] - vx[1][c])
                            : (vx[1][c] - vx[3][c]);
            m[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
          }
          if constexpr (!SPLIT) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int h = 0; h < 2; ++h)
                m[cp + h] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[(b * 4 + cp + h) * 4 + i], v[h][i], m[cp + h], 0, 0, 0);
            if constexpr ((WINO_ABL & 4) != 0) {
#pragma unroll
              for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                  m[cp + h] = __builtin_amdgcn_mfma_f32_16x16x4f32(wt[(b * 4 + cp + h) * 4 + i], v[h][i], m[cp + h], 0, 0, 0);
            }
          } else {
            // fp32 Winograd-domain value -> f16 hi + lo (exact to 22 bits), three product terms
            f16x4 vhi[2], vlo[2], vl2[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const f32x4 vs = v[h] * in_scale;
              vhi[h] = __builtin_convertvector(vs, f16x4);
              const f32x4 r1 = vs - __builtin_convertvector(vhi[h], f32x4);
              vlo[h] = __builtin_convertvector(r1, f16x4);
              if constexpr ((WINO_ABL & 8) != 0)                  // timing proxy of a THREE-piece split: third piece + 6 products
                vl2[h] = __builtin_convertvector(r1 - __builtin_convertvector(vlo[h], f32x4), f16x4);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) m[cp + h] = __builtin_amdgcn_mfma_f32_16x16x16f16(whi[b * 4 + cp + h], vlo[h], m[cp + h], 0, 0, 0);
#pragma unroll
            for (int h = 0; h < 2; ++h) m[cp + h] = __builtin_amdgcn_mfma_f32_16x16x16f16(wlo[b * 4 + cp + h], vhi[h], m[cp + h], 0, 0, 0);
#pragma unroll
            for (int h = 0; h < 2; ++h) m[cp + h] = __builtin_amdgcn_mfma_f32_16x16x16f16(whi[b * 4 + cp + h], vhi[h], m[cp + h], 0, 0, 0);
            if constexpr ((WINO_ABL & 8) != 0) {
#pragma unroll
              for (int h = 0; h < 2; ++h) m[cp + h] = __builtin_amdgcn_mfma_f32_16x16x16f16(wlo[b * 4 + cp + h], vlo[h], m[cp + h], 0, 0, 0);
#pragma unroll
              for (int h = 0; h < 2; ++h) m[cp + h] = __builtin_amdgcn_mfma_f32_16x16x16f16(whi[b * 4 + cp + h], vl2[h], m[cp + h], 0, 0, 0);
#pragma unroll
              for (int h = 0; h < 2; ++h) m[cp + h] = __builtin_amdgcn_mfma_f32_16x16x16f16(wlo[b * 4 + cp + h], vl2[h], m[cp + h], 0, 0, 0);
            }
          }
        }
        // x output transform, then accumulate the y output transform
        const f32x4 t0 = m[0] + m[1] + m[2];
        const f32x4 t1 = m[1] - m[2] - m[3];
        if (b == 0) { Yg[0] = t0; Yg[1] = t1; }
        if (b == 1) { Yg[0] += t0; Yg[1] += t1; Yg[2] = t0; Yg[3] = t1; }
        if (b == 2) { Yg[0] += t0; Yg[1] += t1; Yg[2] = pk_sub(Yg[2], t0); Yg[3] = pk_sub(Yg[3], t1); }
        if (b == 3) { Yg[2] = pk_sub(Yg[2], t0); Yg[3] = pk_sub(Yg[3], t1); }
      }
    }
    // partial outputs of z-frequency A -> the exchange region (separate from the halo, free since the last
    // barrier of the previous tile): 1 KiB blocks [wave][g][tyb][j], 64 float4 slots each at (L ^ ((L >> 3) & 7)),
    // L = x*4 + channel quarter -- the writers' 8-lane groups and the readers' 16-lane groups both hit distinct
    // bank slots, and a reader wave gets one x-contiguous 1 KiB output row per instruction
#pragma unroll
    for (int ji = 0; ji < 4; ++ji) *(f32x4*)(pdst + g * 4096 + (ji >> 1) * 1024 + pw[ji & 1]) = Yg[ji];
    CTS(10 + 2 * g);
  }
}

// The renderer's factor projection (reference modules/geometry.py:731-749: the depth axis folded into the channels of a
// 1x1 convolution, C*D -> 16) sits directly behind the last camera block and contracts exactly the axis a workgroup of
// this kernel walks (a column of tiles along z).  Two fused forms remove its HBM round trips (round 4):
//   FUSE = 1 (forward, wino16_projfwd.inc): the finished output records of a tile (after LeakyReLU / PixelNorm) are also
//     contracted with the projection weights of their two depth planes into a per-wave 2 rows x 16 x x 16 cout accumulator (16
//     extra MFMAs per wave and tile; the records cross from the epilogue's lane = (x, quarter) order to the MFMA's B-operand
//     order through the wave's own, already consumed slices of the exchange region); at the top of the column the projection's
//     own epilogue (He, bias, LeakyReLU, PixelNorm) runs and the (H, W, 16) latent image rows are stored.  Same
//     operands in the same accumulation order as lf_conv1x1_fwd on the stored volume: bit-identical.
//   FUSE = 2 (backward, wino16_projbwd.inc): the input gradient volume of the first data-gradient convolution never exists in
//     HBM.  It is g(z, y, x, :) = LReLU'/PixelNorm'[ he_p * Wt_p(z) . gp(y, x, :) ] with the saved activation / norm of the last
//     camera block; a workgroup forms the two new z planes of its halo per tile from the block's activation record
//     (same bytes the gradient volume would have cost), the 16-float projection gradient of the pixel (resident in
//     registers for the whole column) and the plane's 16 x 16 weight slice: 24 extra MFMAs per wave and tile instead of a
//     2.1 GB kernel.  Same arithmetic as lf_conv1x1_bwd_data's epilogue.
struct WinoProj {
  const float* wA;        // FUSE 1: [D][64 lanes][4] = Wp[cout = lane & 15][d][c = 4 (lane >> 4) + i]; FUSE 2: the transposed slices
  const float* bias;      // FUSE 1: projection bias (16) or null
  float* zp;              // FUSE 1: out, (N, H, W, 16) projected latent image
  float* pnorm;           // FUSE 1: out, (N * H * W) PixelNorm denominators of zp (or null)
  const float* gp;        // FUSE 2: in, (N, H, W, 16) gradient w.r.t. the projection's pre-activation
  const float* xnorm;     // FUSE 2: in, (N * D * H * W) PixelNorm denominators saved with the activation passed as `x`
  float he;               // the projection's He constant
  unsigned flags;         // FUSE 1: the projection's epilogue; FUSE 2: the epilogue of the layer that produced `x`
};

// 2-bit table p = (0, 2, 3, 1): a 16-byte quarter q of record v (16 records of 64 B) stored at position q ^ p(v >> 2) is read
// conflict-free by ds_read_b128 with lane = q * 16 + v (the hardware's lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...)
__device__ __forceinline__ int tr_swz(int v) { return (0x78 >> (2 * ((v >> 2) & 3))) & 3; }

// FORM: the per-tile path behind the MFMA phase (z output transform, epilogue, previous-layer backward, stores, next-halo
// fetch / commit, projection) compiled for ONE combination of the epilogue arguments instead of generic over their runtime
// values.  Generic, every launch carries the live ranges and the branches of every form (242 VGPRs, 527 VALU and 66
// branches behind the last MFMA); a fixed form carries its own only (profiles/wino_forms_isa.txt).  The forms are the ones
// the render loop launches; the host entry points pick one from their runtime arguments (wino_form_of) and send every other
// combination to WF_GENERIC.  Everything but the epilogue arithmetic is the generic path's source with the arguments pinned;
// the arithmetic is wino_epi_* (wino16_math.h), the generic kernels' roundings spelled out: bit-identical.
enum : int {
  WF_GENERIC = 0,
  WF_FWD_BLOCK = 1,     // flags = LReLU | PixelNorm, bias and norm_out present, no prev_y, no amax_out
  WF_DGRAD_PREV = 2,    // flags = 0, no bias, prev_y and prev_norm present, prev_flags = LReLU | PixelNorm, no amax_out
  WF_DGRAD_PLAIN = 3,   // flags = 0, no bias, no prev_y, no amax_out
};

}  // namespace
