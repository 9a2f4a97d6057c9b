// Winograd F(2x2x2, 3x3x3) form of the fused 16 -> 16 channel conv3d block step (gfx950).
//
//   y = PixelNorm(LeakyReLU(conv3d(x, W) * he + b))            latentfusion/modules/blocks.py:152-158
//                                                              latentfusion/modules/equalized.py:57-64
// and, with transposed/flipped weights and `prev_*` set, the data gradient fused with the previous
// layer's LeakyReLU'/PixelNorm' (autograd of the same lines).
//
// All arithmetic is fp32 (v_mfma_f32_16x16x4_f32 + fp32 VALU transforms).  The minimal-filtering
// identity  Y = A^T[(G w G^T) . (B^T d B)]A  applied along z, y and x needs 64 multiplies per 2x2x2
// outputs instead of 216, so the MFMA work per voxel drops 3.375x; measured against fp64 the result is
// as close as the direct fp32 kernel's (tests/test_ops_gpu.py::test_winograd_conv3d_*).
//
// Work split: 256-thread workgroups, TWO per CU (2 x 79,872 B of LDS), each persistent over its own range
// of 2 x 8 x 16-voxel tiles.  The two workgroups of a CU are not synchronised with each other, so one's
// exchange / epilogue / DMA-wait phases run under the other's MFMA phase (on gfx950 the fp32 MFMA and the
// fp32 VALU share the SIMD's issue pipe -- measured: they do not overlap -- so everything that is not an
// MFMA has to be either few instructions or hidden this way).
//   * wave w owns z-frequency a = w of the tile; the 16 (y,x)-frequency matrices U[a][b][c]
//     (16 cout x 16 cin each) live in 64 VGPRs for the whole launch;
//   * MFMA columns = 16 Winograd tiles (2 in y x 8 in x), lane group kg = lane >> 4 carries input
//     channels 4kg..4kg+3 (B operand) and receives output channels 4kg..4kg+3 (D operand);
//   * per 16-tile group: 32 ds_read_b128 of the fp32 halo (two z planes combined on the fly),
//     x/y input transforms in registers, 64 MFMAs, y/x output transform in registers;
//   * the four z-frequency partials of a tile meet through LDS, then every wave finishes a quarter of the
//     outputs: z output transform, He scale, bias, LeakyReLU, PixelNorm (DPP quad reduction), and one
//     x-contiguous 1 KiB row per store instruction.
// The halo (4 x 10 x 18 voxels, fp32) slides along z: a workgroup walks up a column of tiles, moves the upper two
// planes of the halo LDS -> LDS and fetches only the two new planes (22.5 KiB) per tile, staged through registers
// under the exchange / epilogue phase.  LDS layout: voxel slot = (z*10 + y)*18 + (x&1)*9 + (x>>1), 16-byte quarter
// q stored at q ^ s, s = 2*((slot>>2)&1) + ((y>>1)&1)  ->  every ds_read_b128 lane group hits 16 distinct slots
// (SQ_LDS_BANK_CONFLICT = 0).
//
// Files: wino16_math.h (build switches of the A/B tools, geometry, packed fp32 helpers, pinned epilogue roundings),
// wino16_compute.h (the MFMA phase wino_compute / wino_rows_packed; WinoProj, WF_*), this file (the kernels' body: the
// product algorithm top to bottom, then the kernels and the host side), and the two fused projection forms as text sections
// the body includes where their code runs: wino16_projfwd.inc (FUSE == 1), wino16_projbwd.inc (FUSE == 2).  Each .inc opens
// with its contract.  The split is checked instruction for instruction (profiles/wino_body_split_isa.txt).
#include "wino16_compute.h"

namespace {

// SPLIT: the f16x3 product step (wino_compute; experimental entry point).  FUSE: 0, or one of the fused projection forms
// (WinoProj).  PACK: packed transforms next to the MFMAs (wino_rows_packed).  FORM: WF_*.
// OPT (fixed forms only) = 1: the registers a fixed form frees are spent on dropping the two optimiser fences that exist only
// because hoisting used to spill (hrel[] in fetch_half, the projection's lane index) and on keeping the bias quarter resident
// across tiles; 0 = fences and per-tile bias read as in the generic kernel (lf_set_tuning(8, 2), for the A/B).
// ZST (fixed forms only) = 1: z-staged halo.  The halo buffer holds the four z-FREQUENCY planes of the tile instead of its four
// raw z planes: the z input transform runs once per halo point in halo_commit instead of once per overlapping (y,x) tile in
// the MFMA phase, which then reads one value where it read two (section 6).  Same operations on the same operands: bit-identical.
template <bool SPLIT, int FUSE = 0, bool PACK = false, int FORM = WF_GENERIC, int OPT = 0, int ZST = 0>
__device__ __forceinline__ void conv3d_c16_wino_body(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out,
    int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z, int ntiles,
    float he, unsigned flags, float slope, float eps,
    const float* __restrict__ prev_y, const float* __restrict__ prev_norm, unsigned prev_flags,
    const float* __restrict__ amax_in, float* __restrict__ amax_out, const WinoProj pj = WinoProj()) {
  static_assert(FORM == WF_GENERIC || (!SPLIT && FUSE != 2 && PACK), "fixed forms: the packed all-fp32 kernels only");
  static_assert(OPT == 0 || OPT == 1, "");
  static_assert(FORM != WF_GENERIC || OPT == 0, "the generic kernel stays as it is");
  static_assert(ZST == 0 || (ZST == 1 && FORM != WF_GENERIC), "z-staged halo: the fixed forms only");
  // ---- 1. form pinning ----
  // a fixed form pins the arguments it is defined by: every test on them below folds at compile time
  constexpr bool HAS_BIAS = FORM == WF_FWD_BLOCK;              // (fixed forms; the generic form tests the pointer)
  if constexpr (FORM == WF_FWD_BLOCK) {
    flags = LF_EPI_LRELU | LF_EPI_PIXELNORM;
    prev_y = nullptr; prev_norm = nullptr; prev_flags = 0u; amax_out = nullptr;
  } else if constexpr (FORM == WF_DGRAD_PREV) {
    flags = 0u; prev_flags = LF_EPI_LRELU | LF_EPI_PIXELNORM;
    bias = nullptr; norm_out = nullptr; amax_out = nullptr;
  } else if constexpr (FORM == WF_DGRAD_PLAIN) {
    flags = 0u; prev_flags = 0u;
    bias = nullptr; norm_out = nullptr; prev_y = nullptr; prev_norm = nullptr; amax_out = nullptr;
  }
  // ---- 2. lane roles and tile range ----
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* const buf = smem;                              // halo
  unsigned char* const px = smem + BUFw;                        // partial exchange

  const int tid = threadIdx.x, lane = tid & 63;
  const int fa = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave = z-frequency
  const int n = lane & 15, kg = lane >> 4;
  const int tx = n & 7, tyb = n >> 3;

  // workgroups b, b+8, b+16, ... run on the same XCD (one L2 each): give them consecutive tile ranges so
  // that the z-halo planes shared by neighbouring ranges are fetched from HBM once
  const int nb = gridDim.x;
  const int lb = (nb % 8 == 0) ? (blockIdx.x % 8) * (nb / 8) + blockIdx.x / 8 : blockIdx.x;
  // (the fused forms keep per-column state: their ranges are whole columns of tiles)
  const int per = (FUSE != 0) ? ((ntiles / tiles_z + nb - 1) / nb) * tiles_z : (ntiles + nb - 1) / nb;
  const int t_begin = lb * per;
  const int t_end = min(t_begin + per, ntiles);
  if (t_begin >= t_end) return;

  const long nvox = (long)D * H * W;
  const unsigned sample_bytes = (unsigned)(nvox * 64);

  // ---- 3. halo addressing.  Piece constants: within a half (two z planes), LDS slot p = piece*64 + lane holds quarter (p&3)^s of
  // voxel slot p>>2.  (360 slots per half is a multiple of 8, so the swizzle is the same in both halves.)
  // Per piece a lane keeps only its byte offset relative to the half's first voxel; x / y range violations (possible
  // only in the first / last tile of a row or column of tiles) are five flag bits per piece in one register, z range
  // violations fall outside the buffer descriptor's range on their own and read zeros.
  // ZST: a lane owns the SAME (y, x, quarter) in all four z planes, so that it can combine them: piece it = 3 lz' + k is item
  // i = (fa + 4k) * 64 + lane of the 10 x 18 plane (720 items, k < 3) in z plane lz' of the half; the quarter is (i & 3) ^ s with
  // the swizzle s of the EVEN planes (a plane is 45 groups of four slots, so bit 1 of s alternates from plane to plane: an odd
  // plane's copy goes to LDS position i ^ 2, halo_commit). ----
  enum { F_XLO = 1, F_XHI = 2, F_YLO = 4, F_YHI = 8, F_PAD = 16, F_ALL6 = 0x2108421 };
  const int xlim = W - (tiles_x - 1) * TXw + 1, ylim = H - (tiles_y - 1) * TYw + 1;   // first invalid lx / ly in the last tile
  int hrel[NITw];
  unsigned hflags = 0;
#pragma unroll
  for (int it = 0; it < NITw; ++it) {
    const int p = ZST ? (fa + 4 * (it % NITZw)) * 64 + lane : (fa + 4 * it) * 64 + lane;
    const int vs = p >> 2;
    const int row = vs / HXw, rem = vs - row * HXw;
    const int xl = rem / 9, xa = rem - xl * 9;
    const int lx = 2 * xa + xl, ly = ZST ? row : row % HYw, lz = ZST ? it / NITZw : row / HYw;
    const int sw = (((vs >> 2) & 1) << 1) | ((ly >> 1) & 1);
    const int q = (p & 3) ^ sw;
    const bool pad = vs >= (ZST ? PLANEw : HALFw);
    hrel[it] = pad ? 0 : ((lz * H + ly) * W + lx) * 64 + q * 16;
    const unsigned f = pad ? F_PAD : ((lx == 0 ? F_XLO : 0) | (lx >= xlim ? F_XHI : 0) | (ly == 0 ? F_YLO : 0) | (ly >= ylim ? F_YHI : 0));
    hflags |= f << (5 * it);
  }
  const bool last_piece_ok = ZST ? ((fa + 4 * (NITZw - 1)) * 64 + lane) < PLANEw * 4      // piece 11: lanes 0-15
                                 : ((fa + 4 * (NITw - 1)) * 64 + lane) < HALFw * 4;      // piece 22: lanes 0-31; 23: none

  // ---- 4. operand and exchange addressing.  B operands: byte offset of (lane's tile, channel quarter) for the 8 slot residues ----
  // (rows dy = 2,3 sit one (y>>1) step further: their quarter swizzle differs in bit 0)
  int off[8][2];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int dyb = 0; dyb < 2; ++dyb) {
      const int bit = ((36 * tyb + tx + r) >> 2) & 1;
      const int quarter = (kg ^ tyb ^ dyb) ^ (bit << 1);
      off[r][dyb] = (36 * tyb + tx) * 64 + quarter * 16;
    }

  // partial exchange
  int pw[2];                                                   // writer: lane part of the slot, per x parity i
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int L = (2 * tx + i) * 4 + kg;
    pw[i] = tyb * 2048 + (L ^ ((L >> 3) & 7)) * 16;
  }
  const int pr = (lane ^ ((lane >> 3) & 7)) * 16;              // reader: lane = x*4 + quarter
  const int ex = lane >> 2, eq = lane & 3;

  // ---- 5. weights: the transformed weights of this wave's z-frequency, lane-major in memory: fp32 [16 (b,c)][4 k-chunks], or
  // f16 [16 (b,c)][hi, lo] x 4 cin per lane (A operands, K = 4 cin per lane group) ----
  float wt[64];
  f16x4 whi[16], wlo[16];
  float in_scale = 1.f;
  if constexpr (!SPLIT) {
    const float* up = upack + (long)fa * 64 * 64 + lane;
#pragma unroll
    for (int k = 0; k < 64; ++k) wt[k] = up[k * 64];
  } else {
    const f16x4* up = (const f16x4*)upack + (long)fa * 16 * 2 * 64 + lane;
#pragma unroll
    for (int k = 0; k < 16; ++k) { whi[k] = up[(k * 2 + 0) * 64]; wlo[k] = up[(k * 2 + 1) * 64]; }
    // power-of-two input scale from the tensor's max-abs (gradient launches); 1 otherwise
    if (amax_in != nullptr) {
      const float am = lf_amax_read(amax_in, lane);
      if (am > 0.f && am < 3.0e38f) {
        int ex;
        frexpf(am, &ex);                                          // am = m * 2^ex, m in [0.5, 1)
        in_scale = ldexpf(1.f, 9 - ex);                           // max maps into [2^8, 2^9): x8 transform growth stays in f16 range
      }
    }
  }

  // tile coordinates are stepped, not divided: (cx, cy, cz, cn) = tile t, (nx, ny, nz, nn) = tile t + 1
  int cx, cy, cz, cn;
  {
    int tt = t_begin;                                            // z fastest: a workgroup walks up columns of tiles
    cz = tt % tiles_z; tt /= tiles_z;
    cx = tt % tiles_x; tt /= tiles_x;
    cy = tt % tiles_y; cn = tt / tiles_y;
  }
  // ---- 6. halo staging (fetch_half / halo_fetch / halo_commit) ----
  // The halo slides along z: the upper two planes of a tile's halo are the lower two of the next tile up the
  // column, so they are moved LDS -> LDS and only two new planes (22.5 KiB) are fetched per tile; at the bottom of a
  // column all four planes are fetched.  Everything is staged through registers: requested right after the
  // barrier that frees the halo buffer, in flight under the exchange / epilogue arithmetic, written to LDS
  // (linear: piece * 1 KiB + lane * 16 within a half) just before the tile's last barrier.  (The vector-memory
  // path of a CU sustains only ~16 B/clk on this access pattern and blocks the issuing wave while its queue is
  // full, so halving the bytes shortens the non-MFMA phase of every tile.)
  // ZST: the upper two planes of the previous tile are still in the lane's registers (hhi), so a slide is a register rename and
  // no LDS read; halo_commit forms the four z frequencies F0 = d0 - d2, F1 = d1 + d2, F2 = d2 - d1, F3 = d1 - d3 of the lane's
  // three items -- wino_compute's operations on the values it would have read -- and writes plane a at a * 11,520 B.
  u32x4 hlo[NITw], hhi[NITw];
  auto fetch_half = [&](u32x4 (&dst)[NITw], __amdgpu_buffer_rsrc_t rs, int base, unsigned sel) {
    // (opaque to the optimiser, or base + hrel[] of every branch is hoisted out of the tile loop into registers)
    if constexpr (!(OPT & 1)) {
#pragma unroll
      for (int i = 0; i < NITw; ++i) asm volatile("" : "+v"(hrel[i]));
    }
    if (sel == 0) {                                             // wave-uniform: interior tile, one VALU add per piece
#pragma unroll
      for (int it = 0; it < NITw; ++it) dst[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, base + hrel[it], 0, 0);
    } else {
      const unsigned bad = hflags & sel;
#pragma unroll
      for (int it = 0; it < NITw; ++it)
        dst[it] = __builtin_amdgcn_raw_buffer_load_b128(rs, (bad & (31u << (5 * it))) ? 0x7fffffff : base + hrel[it], 0, 0);
    }
  };
  auto halo_fetch = [&](int bx, int by, int bz, int bn, bool on, bool slide) {
    // everything wave-uniform here runs on the scalar unit
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (long)(on ? bn : 0) * nvox * 16), 0,
                                                                        on ? sample_bytes : 0u, 0x00020000);
    const int base = (((bz * TZw - 1) * H + (by * TYw - 1)) * W + (bx * TXw - 1)) * 64;
    unsigned sel = 0;
    if (bx == 0) sel |= F_XLO * F_ALL6;
    if (bx == tiles_x - 1) sel |= F_XHI * F_ALL6;
    if (by == 0) sel |= F_YLO * F_ALL6;
    if (by == tiles_y - 1) sel |= F_YHI * F_ALL6;
    if (slide) {
#pragma unroll
      for (int it = 0; it < NITw; ++it) {
        if constexpr (ZST) hlo[it] = hhi[it];
        else hlo[it] = *(const u32x4*)(buf + HALFBw + (fa + 4 * it) * 1024 + lane * 16);
      }
    } else {
      fetch_half(hlo, rs, base, sel);
    }
    fetch_half(hhi, rs, base + 2 * H * W * 64, sel);
  };
  auto halo_commit = [&]() {
    if constexpr (ZST) {
#pragma unroll
      for (int k = 0; k < NITZw; ++k) {
        const f32x4 d0 = __builtin_bit_cast(f32x4, hlo[k]), d1 = __builtin_bit_cast(f32x4, hlo[NITZw + k]);
        const f32x4 d2 = __builtin_bit_cast(f32x4, hhi[k]), d3 = __builtin_bit_cast(f32x4, hhi[NITZw + k]);
        const f32x4 f0 = pk_sub(d0, d2), f1 = d1 + d2, f2 = pk_sub(d2, d1), f3 = pk_sub(d1, d3);
        const int o = (fa + 4 * k) * 1024 + lane * 16;
        if (k < NITZw - 1 || last_piece_ok) {
          *(f32x4*)(buf + o) = f0;
          *(f32x4*)(buf + PLANEBw + (o ^ 32)) = f1;
          *(f32x4*)(buf + 2 * PLANEBw + o) = f2;
          *(f32x4*)(buf + 3 * PLANEBw + (o ^ 32)) = f3;
        }
      }
      return;
    }
#pragma unroll
    for (int it = 0; it < NITw; ++it) {
      unsigned char* dst = buf + (fa + 4 * it) * 1024 + lane * 16;
      if (it < NITw - 1 || last_piece_ok) {
        *(u32x4*)dst = hlo[it];
        *(u32x4*)(dst + HALFBw) = hhi[it];
      }
    }
  };
  const float out_scale = he / in_scale;
  const bool addmode = prev_y != nullptr && (prev_flags & LF_EPI_ADD);      // prev_y is an addend, not a saved activation
  float wave_amax = 0.f;
  // (the state of the fused forms is declared in every form, between these statements as it always was: unused, it folds away)
#define WINO16_PROJBWD_STATE
#include "wino16_projbwd.inc"
  f32x4 bv_res = (f32x4){0.f, 0.f, 0.f, 0.f};
  if constexpr (HAS_BIAS && (OPT & 1)) bv_res = *(const f32x4*)(bias + eq * 4);
#define WINO16_PROJFWD_ACC
#include "wino16_projfwd.inc"

  // ---- 7. prime: the first tile's halo ----
  if constexpr (FUSE == 2) {
#define WINO16_PROJBWD_PRIME
#include "wino16_projbwd.inc"
  } else {
    halo_fetch(cx, cy, cz, cn, true, false);
    halo_commit();
  }
  lds_barrier();

  // ---- 8. per tile (TS / CTS: cycle stamps of the WINO_ABL = 16 / 32 builds, nothing otherwise) ----
  for (int t = t_begin; t < t_end; ++t) {
    // MFMA phase: this wave's z-frequency of the tile, halo -> partial outputs in the exchange region
    TS(0);
    unsigned* const tsp = ((WINO_ABL & 16) && blockIdx.x == 11 && lane == 0) ? (unsigned*)norm_out + ((t - t_begin) * 4 + fa) * 16 : nullptr;
    switch (fa) {
      case 0: wino_compute<0, SPLIT, FUSE != 0, PACK, ZST != 0>(buf, off, wt, whi, wlo, in_scale, px + fa * 8192, pw, tsp); break;
      case 1: wino_compute<1, SPLIT, FUSE != 0, PACK, ZST != 0>(buf, off, wt, whi, wlo, in_scale, px + fa * 8192, pw, tsp); break;
      case 2: wino_compute<2, SPLIT, FUSE != 0, PACK, ZST != 0>(buf, off, wt, whi, wlo, in_scale, px + fa * 8192, pw, tsp); break;
      default: wino_compute<3, SPLIT, FUSE != 0, PACK, ZST != 0>(buf, off, wt, whi, wlo, in_scale, px + fa * 8192, pw, tsp); break;
    }
    TS(1);
    lds_barrier();                                  // every wave is done reading the halo; all partials are in LDS
    TS(2);
    __builtin_amdgcn_s_setprio(WINO_PN);

    // next coordinates.  (The next tile's halo is in flight during the exchange / epilogue below and, for the CU, under the
    // MFMA phase of the other resident workgroup.)
    int nx = cx, ny = cy, nz = cz + 1, nn = cn;
    if (nz == tiles_z) { nz = 0; ++nx; }
    if (nx == tiles_x) { nx = 0; ++ny; }
    if (ny == tiles_y) { ny = 0; ++nn; }
    TS(3);

    // output rows, with the previous layer's loads and the bias: this wave finishes rows y = 2fa, 2fa+1 of the tile,
    // lane = x*4 + channel quarter
    const int bx = cx, by = cy, bz = cz, tt = cn;
    const int gx = bx * TXw + ex;
    const bool xok = gx < W;
    int voxi[4];
    bool okv[4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int zo = 0; zo < 2; ++zo) {
        const int gz = bz * TZw + zo, gy = by * TYw + 2 * fa + j;       // wave-uniform: scalar unit
        const bool rowok = gy < H && gz < D;
        const int rowbase = rowok ? (gz * H + gy) * W : 0;
        okv[j * 2 + zo] = xok && rowok;
        voxi[j * 2 + zo] = okv[j * 2 + zo] ? rowbase + gx : 0;
      }
    f32x4 pyv[4];
    float pnv[4];
    if (prev_y != nullptr) {
      const float* pybase = prev_y + (long)tt * nvox * 16;
      const float* pnbase = (FORM == WF_DGRAD_PREV || prev_norm) ? prev_norm + (long)tt * nvox : nullptr;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        pyv[k] = okv[k] ? *(const f32x4*)(pybase + voxi[k] * 16 + eq * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
        pnv[k] = (okv[k] && (FORM == WF_DGRAD_PREV || pnbase)) ? pnbase[voxi[k]] : 1.f;
      }
    }
    // (bias is re-read per tile -- an L1 hit queued ahead of the halo -- rather than held in four registers)
    // (a fixed form with OPT bit 0 has the registers: bv_res, loaded once)
    f32x4 bv4 = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (HAS_BIAS && (OPT & 1)) {
      bv4 = bv_res;
    } else if constexpr (FORM == WF_GENERIC || HAS_BIAS) {
      const float* bp = bias;
      asm volatile("" : "+s"(bp));
      if (HAS_BIAS || bp != nullptr) bv4 = *(const f32x4*)(bp + eq * 4);
    }
    TS(4);
    // next-halo fetch (FUSE = 2 forms its planes behind the stores, below)
    if constexpr (FUSE != 2) halo_fetch(nx, ny, nz, nn, t + 1 < t_end, nz != 0);
    TS(5);

    // exchange read with the z output transform
    f32x4 o[4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      f32x4 p[4];
      if constexpr ((WINO_ABL & 2) != 0) {
        o[j * 2 + 0] = *(const f32x4*)(px + fa * 8192 + fa * 2048 + j * 1024 + pr);
        o[j * 2 + 1] = *(const f32x4*)(px + fa * 8192 + ((fa + 1) & 3) * 2048 + j * 1024 + pr);
      } else {
#pragma unroll
        for (int a2 = 0; a2 < 4; ++a2)
          p[a2] = *(const f32x4*)(px + a2 * 8192 + fa * 2048 + j * 1024 + pr);
        o[j * 2 + 0] = p[0] + p[1] + p[2];                        // z output transform
        o[j * 2 + 1] = pk_sub(pk_sub(p[1], p[2]), p[3]);
      }
    }

    // forward epilogue: He scale, bias, addend, LeakyReLU, PixelNorm
    unsigned char* ybase = (unsigned char*)(y + (long)tt * nvox * 16) + eq * 16;
    float* nbase = (FORM == WF_FWD_BLOCK || norm_out) ? norm_out + (long)tt * nvox : nullptr;
    f32x4 v[4];
    float rn[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      rn[k] = 1.f;
      if constexpr ((WINO_ABL & 1) != 0) { v[k] = o[k]; continue; }
      if constexpr (FORM == WF_FWD_BLOCK) {
        wino_epi_fwd_block(o[k], bv4, out_scale, slope, eps, v[k], rn[k]);
      } else if constexpr (FORM == WF_DGRAD_PLAIN) {
        v[k] = wino_epi_dgrad_plain(o[k], out_scale);
      } else if (prev_y == nullptr || addmode) {
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float u = o[k][e] * out_scale + bv4[e];
          if (addmode) u += pyv[k][e];
          if (flags & LF_EPI_LRELU) u = fmaxf(u, u * slope);
          v[k][e] = u;
          ss += u * u;
        }
        if (flags & LF_EPI_PIXELNORM) {
          const float tq = quad_sum(ss) * (1.f / 16.f) + eps;
          const float rinv = fast_rsqrt(tq);
          rn[k] = tq * rinv;
          v[k] *= rinv;
        }
      }
    }
    // commit: the next halo (and, for the gradient form, the previous layer's activations) must have arrived
    // before the tile's last barrier; this tile's stores are issued after the wait so they stay out of it
    // and drain behind the next tile's MFMAs
    TS(6);
    if constexpr (FUSE != 2) halo_commit();
    TS(7);
    // previous layer's backward (data-gradient launches), stores, amax
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (FORM == WF_DGRAD_PREV) {
        if (!(WINO_ABL & 1)) v[k] = wino_epi_dgrad_prev(o[k], pyv[k], pnv[k], out_scale, slope);
      } else if (!(WINO_ABL & 1) && prev_y != nullptr && !addmode) {
        const f32x4 yp = pyv[k];
        v[k] = o[k] * out_scale;
        if (prev_flags & LF_EPI_PIXELNORM) {
          const float dot = quad_sum(v[k][0] * yp[0] + v[k][1] * yp[1] + v[k][2] * yp[2] + v[k][3] * yp[3]) * (1.f / 16.f);
          const float rinv = fast_rcp(pnv[k]);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[k][e] = (v[k][e] - yp[e] * dot) * rinv;
        }
        if (prev_flags & LF_EPI_LRELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[k][e] = yp[e] > 0.f ? v[k][e] : v[k][e] * slope;
        }
      }
      if (okv[k]) {
        __builtin_nontemporal_store(v[k], (f32x4*)(ybase + (unsigned)(voxi[k] * 64)));   // streamed: L2 is for halos
        if (!(WINO_ABL & 16) && (prev_y == nullptr || addmode) && (flags & LF_EPI_PIXELNORM) && (FORM == WF_FWD_BLOCK || nbase != nullptr) && eq == 0) nbase[voxi[k]] = rn[k];
        if (amax_out != nullptr)
          wave_amax = fmaxf(wave_amax, fmaxf(fmaxf(fabsf(v[k][0]), fabsf(v[k][1])), fmaxf(fabsf(v[k][2]), fabsf(v[k][3]))));
      }
    }
    // fused projection hooks: the next tile's computed halo planes (backward), the tile's projection step (forward)
    if constexpr (FUSE == 2) {
#define WINO16_PROJBWD_NEXT
#include "wino16_projbwd.inc"
    }
    if constexpr (FUSE == 1) {
#define WINO16_PROJFWD_TILE
#include "wino16_projfwd.inc"
    }
    TS(8);
    // barrier and step
    lds_barrier();                                              // next halo visible to all; partials consumed
    cx = nx; cy = ny; cz = nz; cn = nn;
    if constexpr (FUSE == 2) {
#define WINO16_PROJBWD_COLUMN
#include "wino16_projbwd.inc"
    }
  }
  // ---- 9. amax publish ----
  if (amax_out != nullptr) {
    float m = wave_amax;
#pragma unroll
    for (int o2 = 32; o2 > 0; o2 >>= 1) m = fmaxf(m, __shfl_xor(m, o2, 64));
    lf_amax_publish(amax_out, m, lane);
  }
}

template <bool PACK>
__global__ void __launch_bounds__(256, 2) conv3d_c16_wino_kernel(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out, int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z,
    int ntiles, float he, unsigned flags, float slope, float eps, const float* __restrict__ prev_y,
    const float* __restrict__ prev_norm, unsigned prev_flags, float* __restrict__ amax_out) {
  conv3d_c16_wino_body<false, 0, PACK>(x, upack, bias, y, norm_out, N, D, H, W, tiles_x, tiles_y, tiles_z, ntiles, he, flags, slope, eps,
                              prev_y, prev_norm, prev_flags, nullptr, amax_out);
}

__global__ void __launch_bounds__(256, 2) conv3d_c16_wino_f16x3_kernel(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out, int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z,
    int ntiles, float he, unsigned flags, float slope, float eps, const float* __restrict__ prev_y,
    const float* __restrict__ prev_norm, unsigned prev_flags, const float* __restrict__ amax_in,
    float* __restrict__ amax_out) {
  conv3d_c16_wino_body<true>(x, upack, bias, y, norm_out, N, D, H, W, tiles_x, tiles_y, tiles_z, ntiles, he, flags, slope, eps,
                             prev_y, prev_norm, prev_flags, amax_in, amax_out);
}

template <bool PACK>
__global__ void __launch_bounds__(256, 2) conv3d_c16_wino_projfwd_kernel(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out, int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z,
    int ntiles, float he, unsigned flags, float slope, float eps, const float* __restrict__ prev_y,
    const float* __restrict__ prev_norm, unsigned prev_flags, WinoProj pj) {
  conv3d_c16_wino_body<false, 1, PACK>(x, upack, bias, y, norm_out, N, D, H, W, tiles_x, tiles_y, tiles_z, ntiles, he, flags, slope,
                                 eps, prev_y, prev_norm, prev_flags, nullptr, nullptr, pj);
}

template <bool PACK>
__global__ void __launch_bounds__(256, 2) conv3d_c16_wino_projbwd_kernel(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out, int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z,
    int ntiles, float he, unsigned flags, float slope, float eps, const float* __restrict__ prev_y,
    const float* __restrict__ prev_norm, unsigned prev_flags, WinoProj pj) {
  conv3d_c16_wino_body<false, 2, PACK>(x, upack, bias, y, norm_out, N, D, H, W, tiles_x, tiles_y, tiles_z, ntiles, he, flags, slope,
                                 eps, prev_y, prev_norm, prev_flags, nullptr, nullptr, pj);
}

// The fixed forms (packed transforms only: under lf_set_tuning key 7 = 0 every call runs the generic scalar kernel).
template <int FORM, int OPT>
__global__ void __launch_bounds__(256, 2) conv3d_c16_wino_form_kernel(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out, int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z,
    int ntiles, float he, unsigned flags, float slope, float eps, const float* __restrict__ prev_y,
    const float* __restrict__ prev_norm, unsigned prev_flags, float* __restrict__ amax_out) {
  conv3d_c16_wino_body<false, 0, true, FORM, OPT>(x, upack, bias, y, norm_out, N, D, H, W, tiles_x, tiles_y, tiles_z, ntiles, he, flags,
                                                 slope, eps, prev_y, prev_norm, prev_flags, nullptr, amax_out);
}

template <int FORM, int OPT>
__global__ void __launch_bounds__(256, 2) conv3d_c16_wino_projfwd_form_kernel(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out, int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z,
    int ntiles, float he, unsigned flags, float slope, float eps, const float* __restrict__ prev_y,
    const float* __restrict__ prev_norm, unsigned prev_flags, WinoProj pj) {
  conv3d_c16_wino_body<false, 1, true, FORM, OPT>(x, upack, bias, y, norm_out, N, D, H, W, tiles_x, tiles_y, tiles_z, ntiles, he, flags,
                                                 slope, eps, prev_y, prev_norm, prev_flags, nullptr, nullptr, pj);
}

// The fixed forms on the z-staged halo (ZST = 1, OPT = 1; kernels of their own, so that the ones above keep their names).
template <int FORM, int OPT>
__global__ void __launch_bounds__(256, 2) conv3d_c16_wino_zst_form_kernel(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out, int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z,
    int ntiles, float he, unsigned flags, float slope, float eps, const float* __restrict__ prev_y,
    const float* __restrict__ prev_norm, unsigned prev_flags, float* __restrict__ amax_out) {
  conv3d_c16_wino_body<false, 0, true, FORM, OPT, 1>(x, upack, bias, y, norm_out, N, D, H, W, tiles_x, tiles_y, tiles_z, ntiles, he, flags,
                                                    slope, eps, prev_y, prev_norm, prev_flags, nullptr, amax_out);
}

template <int FORM, int OPT>
__global__ void __launch_bounds__(256, 2) conv3d_c16_wino_projfwd_zst_form_kernel(
    const float* __restrict__ x, const float* __restrict__ upack, const float* __restrict__ bias,
    float* __restrict__ y, float* __restrict__ norm_out, int N, int D, int H, int W, int tiles_x, int tiles_y, int tiles_z,
    int ntiles, float he, unsigned flags, float slope, float eps, const float* __restrict__ prev_y,
    const float* __restrict__ prev_norm, unsigned prev_flags, WinoProj pj) {
  conv3d_c16_wino_body<false, 1, true, FORM, OPT, 1>(x, upack, bias, y, norm_out, N, D, H, W, tiles_x, tiles_y, tiles_z, ntiles, he, flags,
                                                    slope, eps, prev_y, prev_norm, prev_flags, nullptr, nullptr, pj);
}

// lf_set_tuning key 7: 1 = packed transforms next to the MFMAs (wino_rows_packed; default), 0 = the scalar form.  Bit-identical.
int g_wino_pack = 1;
// lf_set_tuning key 8: 1 = calls that match a fixed form run it, OPT = 1 (default), 0 = every call runs the generic kernel,
// 2 = the fixed forms with OPT = 0, 3 = the fixed forms, OPT = 1, all on the raw-plane halo (the staging before ZST),
// 4 = all on the z-staged halo.  Bit-identical.  Under 1 a form runs z-staged where that measured faster (wino_zst_default).
int g_wino_forms = 1;
// index: WF_FWD_BLOCK, WF_DGRAD_PREV, WF_DGRAD_PLAIN, the forward block with the projection (profiles/wino_zstage_ab.json)
constexpr bool wino_zst_default[4] = {true, false, false, true};
bool wino_zst(int idx) { return g_wino_forms == 4 || (g_wino_forms == 1 && wino_zst_default[idx]); }

// The fixed form a call may run, from ALL the arguments a form pins: a call that differs in any of them (add mode, amax_out,
// LeakyReLU alone, flags without a bias, ...) is WF_GENERIC.
int wino_form_of(const float* bias, const float* norm_out, unsigned flags, const float* prev_y, const float* prev_norm,
                 unsigned prev_flags, const float* amax_out) {
  const unsigned full = LF_EPI_LRELU | LF_EPI_PIXELNORM;
  if (!g_wino_pack || !g_wino_forms || amax_out != nullptr) return WF_GENERIC;
  if (flags == full && bias != nullptr && norm_out != nullptr && prev_y == nullptr) return WF_FWD_BLOCK;
  if (flags == 0u && bias == nullptr && prev_y != nullptr && prev_norm != nullptr && prev_flags == full) return WF_DGRAD_PREV;
  if (flags == 0u && bias == nullptr && prev_y == nullptr) return WF_DGRAD_PLAIN;
  return WF_GENERIC;
}

template <auto kernel, bool COLUMNS = false, typename... Extra>
int launch_wino(const float* x, const void* upack, const float* bias, float* y, float* norm_out, int N, int D,
                int H, int W, float he, unsigned flags, float slope, float eps, const float* prev_y, const float* prev_norm,
                unsigned prev_flags, void* stream, Extra... extra) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return LF_EINVAL;
  if ((long)D * H * W * 64 >= 0x7fffffffL || !(slope > 0.f && slope < 1.f)) return LF_EINVAL;
  if (!lf_aligned16(x) || !lf_aligned16(y) || !lf_aligned16(upack) || (bias && !lf_aligned16(bias))) return LF_EALIGN;
  const bool add = prev_y != nullptr && (prev_flags & LF_EPI_ADD);
  if (add && prev_flags != LF_EPI_ADD) return LF_EINVAL;
  if (prev_y != nullptr && !add && (flags != 0 || bias != nullptr)) return LF_EINVAL;
  if ((prev_flags & LF_EPI_PIXELNORM) && prev_y != nullptr && prev_norm == nullptr) return LF_EINVAL;
  const int ptx = (W + TXw - 1) / TXw, pty = (H + TYw - 1) / TYw, ptz = (D + TZw - 1) / TZw;
  const long pt = (long)ptx * pty * ptz * N;
  if (pt > 0x7fffffffL) return LF_EINVAL;
  const int cus = lf_cu_count();
  const size_t shmem = (size_t)LDSw;
  static lf_devmask_t attr_set;                                   // (one instance per kernel: the template is per kernel)
  {
    hipError_t e = lf_ensure_dyn_lds(attr_set, (const void*)kernel, (int)shmem);
    if (e != hipSuccess) return (int)e;
  }
  const long want = 2L * cus;                                     // two resident workgroups per CU
  const long units = COLUMNS ? pt / ptz : pt;                     // (the fused forms hand out whole columns of tiles)
  const unsigned grid = (unsigned)(units < want ? units : want);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), shmem, (hipStream_t)stream, x, (const float*)upack, bias, y, norm_out, N, D,
                     H, W, ptx, pty, ptz, (int)pt, he, flags, slope, eps, prev_y, prev_norm, prev_flags, extra...);
  return lf_launch_status();
}

}  // namespace

// tuning hooks for lf_set_tuning (keys 7 and 8, resample.hip)
int lf_internal_wino_set_pack(int v) {
  const int prev = g_wino_pack;
  if (v == 0 || v == 1) g_wino_pack = v;
  return prev;
}
int lf_internal_wino_set_forms(int v) {
  const int prev = g_wino_forms;
  if (v >= 0 && v <= 4) g_wino_forms = v;
  return prev;
}

// floats of the transformed-weight pack: [4 z-freq][16 (y,x)-freq][4 k-chunks][64 lanes]
extern "C" size_t lf_conv3d_c16_wino_upack_floats(void) { return (size_t)4 * 16 * 4 * 64; }

extern "C" int lf_conv3d_c16_wino(const float* x, const float* upack, const float* bias, float* y, float* norm_out,
                                  int N, int D, int H, int W, float he, unsigned flags, float slope, float eps,
                                  const float* prev_y, const float* prev_norm, unsigned prev_flags,
                                  float* amax_out, void* stream) {
  lf_clear_error();
#define LF_WINO_FORM(F, O) \
  launch_wino<conv3d_c16_wino_form_kernel<F, O>>(x, upack, bias, y, norm_out, N, D, H, W, he, flags, slope, eps, prev_y, prev_norm, \
                                                 prev_flags, stream, amax_out)
#define LF_WINO_ZST(F) \
  launch_wino<conv3d_c16_wino_zst_form_kernel<F, 1>>(x, upack, bias, y, norm_out, N, D, H, W, he, flags, slope, eps, prev_y, prev_norm, \
                                                     prev_flags, stream, amax_out)
#define LF_WINO_OPTS(F) (g_wino_forms == 2 ? LF_WINO_FORM(F, 0) : wino_zst(F - WF_FWD_BLOCK) ? LF_WINO_ZST(F) : LF_WINO_FORM(F, 1))
  switch (wino_form_of(bias, norm_out, flags, prev_y, prev_norm, prev_flags, amax_out)) {
    case WF_FWD_BLOCK: return LF_WINO_OPTS(WF_FWD_BLOCK);
    case WF_DGRAD_PREV: return LF_WINO_OPTS(WF_DGRAD_PREV);
    case WF_DGRAD_PLAIN: return LF_WINO_OPTS(WF_DGRAD_PLAIN);
    default: break;
  }
#undef LF_WINO_OPTS
#undef LF_WINO_ZST
#undef LF_WINO_FORM
  return g_wino_pack ? launch_wino<conv3d_c16_wino_kernel<true>>(x, upack, bias, y, norm_out, N, D, H, W, he, flags, slope, eps, prev_y,
                                                                  prev_norm, prev_flags, stream, amax_out)
                     : launch_wino<conv3d_c16_wino_kernel<false>>(x, upack, bias, y, norm_out, N, D, H, W, he, flags, slope, eps, prev_y,
                                                                   prev_norm, prev_flags, stream, amax_out);
}

// halfs of the split transformed-weight pack: [4 z-freq][16 (y,x)-freq][hi, lo][64 lanes][4 cin]
extern "C" size_t lf_conv3d_c16_wino_split_upack_halfs(void) { return (size_t)4 * 16 * 2 * 64 * 4; }

extern "C" int lf_conv3d_c16_wino_split(const float* x, const void* upack, const float* bias, float* y, float* norm_out,
                                        int N, int D, int H, int W, float he, unsigned flags, float slope, float eps,
                                        const float* prev_y, const float* prev_norm, unsigned prev_flags,
                                        const float* amax_in, float* amax_out, void* stream) {
  lf_clear_error();
  return launch_wino<conv3d_c16_wino_f16x3_kernel>(x, upack, bias, y, norm_out, N, D, H, W, he, flags, slope, eps, prev_y,
                     prev_norm, prev_flags, stream, amax_in, amax_out);
}

// floats of a projection slice pack of the fused forms: [D][64 lanes][4]
extern "C" size_t lf_conv3d_c16_wino_proj_pack_floats(int D) { return (size_t)(D > 0 ? D : 0) * 64 * 4; }

extern "C" int lf_conv3d_c16_wino_projfwd(const float* x, const float* upack, const float* bias, float* y, float* norm_out,
                                          int N, int D, int H, int W, float he, unsigned flags, float slope, float eps,
                                          const float* proj_wA, const float* proj_bias, float* zp, float* pnorm,
                                          float proj_he, unsigned proj_flags, void* stream) {
  lf_clear_error();
  if (proj_wA == nullptr || zp == nullptr) return LF_EINVAL;
  if (!lf_aligned16(proj_wA) || !lf_aligned16(zp) || (proj_bias && !lf_aligned16(proj_bias))) return LF_EALIGN;
  if ((proj_flags & ~(LF_EPI_LRELU | LF_EPI_PIXELNORM)) != 0) return LF_EINVAL;
  WinoProj pj = {proj_wA, proj_bias, zp, pnorm, nullptr, nullptr, proj_he, proj_flags};
  if (wino_form_of(bias, norm_out, flags, nullptr, nullptr, 0u, nullptr) == WF_FWD_BLOCK) {
#define LF_WINO_FORM(O) \
  launch_wino<conv3d_c16_wino_projfwd_form_kernel<WF_FWD_BLOCK, O>, true>(x, upack, bias, y, norm_out, N, D, H, W, he, flags, slope, eps, \
                                                                          nullptr, nullptr, 0u, stream, pj)
    if (g_wino_forms != 2 && wino_zst(3))
      return launch_wino<conv3d_c16_wino_projfwd_zst_form_kernel<WF_FWD_BLOCK, 1>, true>(x, upack, bias, y, norm_out, N, D, H, W, he, flags,
                                                                                         slope, eps, nullptr, nullptr, 0u, stream, pj);
    return g_wino_forms == 2 ? LF_WINO_FORM(0) : LF_WINO_FORM(1);
#undef LF_WINO_FORM
  }
  return g_wino_pack ? launch_wino<conv3d_c16_wino_projfwd_kernel<true>, true>(x, upack, bias, y, norm_out, N, D, H, W, he, flags, slope,
                                                                                eps, nullptr, nullptr, 0u, stream, pj)
                     : launch_wino<conv3d_c16_wino_projfwd_kernel<false>, true>(x, upack, bias, y, norm_out, N, D, H, W, he, flags, slope,
                                                                                 eps, nullptr, nullptr, 0u, stream, pj);
}

extern "C" int lf_conv3d_c16_wino_projbwd(const float* gp, const float* proj_wtA, float proj_he, const float* act,
                                          const float* act_norm, unsigned act_flags, const float* upack, float* y,
                                          int N, int D, int H, int W, float he, float slope, const float* prev_y,
                                          const float* prev_norm, unsigned prev_flags, void* stream) {
  lf_clear_error();
  if (gp == nullptr || proj_wtA == nullptr || act == nullptr) return LF_EINVAL;
  if ((act_flags & LF_EPI_PIXELNORM) && act_norm == nullptr) return LF_EINVAL;
  if ((act_flags & ~(LF_EPI_LRELU | LF_EPI_PIXELNORM)) != 0) return LF_EINVAL;
  if (!lf_aligned16(gp) || !lf_aligned16(proj_wtA) || (prev_y && !lf_aligned16(prev_y))) return LF_EALIGN;
  if (prev_y != nullptr && (prev_flags & LF_EPI_ADD)) return LF_EINVAL;
  WinoProj pj = {proj_wtA, nullptr, nullptr, nullptr, gp, act_norm, proj_he, act_flags};
  return g_wino_pack ? launch_wino<conv3d_c16_wino_projbwd_kernel<true>, true>(act, upack, nullptr, y, nullptr, N, D, H, W, he, 0u, slope,
                                                                                0.f, prev_y, prev_norm, prev_flags, stream, pj)
                     : launch_wino<conv3d_c16_wino_projbwd_kernel<false>, true>(act, upack, nullptr, y, nullptr, N, D, H, W, he, 0u, slope,
                                                                                 0.f, prev_y, prev_norm, prev_flags, stream, pj);
}
