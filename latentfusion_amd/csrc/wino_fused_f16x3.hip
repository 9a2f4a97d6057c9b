// Wide 3-D Winograd convolutions with three-term f16 products ("f16x3"): the work of lf_wino_fused_gemm for dims = 3
// (wino_fused.hip) -- per-frequency products M[f] = V[f] . U[f]^T, output transform A^T M A folded into the frequency loop,
// He scale / bias / LeakyReLU in the store -- with every fp32 product formed on v_mfma_f32_16x16x32_f16 from the hi/lo split
// of conv_split.hip: x = hi + lo, hi = (f16)x, lo = (f16)(x - hi), a*b ~= a_lo*b_hi + a_hi*b_lo + a_hi*b_hi, accumulated
// in fp32 (22-bit operands; the dropped lo*lo term is <= 2^-22 |a b|).  The f16 MFMA runs at 16x the fp32 MFMA rate.
// Layers: modules/blocks.py:152-158 with modules/equalized.py:57-64 at 256 -> 256 on 16^3 (the released architecture).
//
// Where the split happens: ONCE, in the input transform (lf_wino3d_input_transform_f16x3), which reads x and writes every V
// element anyway.  V goes to memory as hi / lo f16 planes interleaved per 32-channel chunk -- row (f, tile) is CinP / 32
// records of [32 hi][32 lo] halfs, 128 B each -- the same 4 bytes per element as fp32 V, so the GEMM stages it exactly as the
// fp32 kernel does (buffer_load_dwordx4 ... lds straight into a 4-stage LDS ring, no staging registers) and the MFMA loop
// carries no conversion VALU at all.  Splitting fp32 V while staging it instead would need register staging (measured at
// ~15 % of peak for the fp32 kernel) or an LDS -> VGPR -> LDS pass per stage, and splitting inside the MFMA loop costs ~3 VALU
// per element per use against the 8 issue cycles an MFMA leaves free.  The weights are split on the host (fp64) into the same
// record layout: U2s [64][CoutP][CinP/32][hi 32 | lo 32].
//
// In LDS a stage row (one output channel of U, one tile of V) is one 128-B record: 16-byte chunks 0-3 hold hi k = 0..31,
// chunks 4-7 lo, XOR-swizzled by (row >> 1) & 7 like the fp32 kernel.  Lane group kg = lane >> 4 reads chunk kg (hi) and
// chunk 4 + kg (lo) of its row: 8 consecutive k each, the same k for A and B, so the contraction over 32 channels is ONE
// 16x16x32 MFMA per term.  A stage feeds 3 MFMAs per 16 x 16 block (12 per wave) instead of the fp32 kernel's 32 fp32 MFMAs.
//
// Range: f16's normal range ends at 2^-14 and its maximum is 65504.  U is scaled by 2^eU (per layer, chosen on the host in
// fp64: max|U| * 2^eU in [2^11, 2^12)); V by 2^eV with 8 * amax_in * 2^eV in [2^11, 2^12), read on the device from amax_in
// (a max-abs side-channel buffer, include/lf_hip.h; |V| <= 8 max|x| for F(2x2x2,3x3x3)) -- no host synchronisation.  The
// epilogue multiplies by he * 2^-(eU + eV): both scales are undone exactly.
#include "lf_common.h"

namespace {

constexpr int KC = 32;      // input channels per stage
constexpr int NSTAGE = 4;   // LDS ring depth; a power of two

typedef unsigned u32;
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(const h16x8 a, const h16x8 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int lds_chunk(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

__device__ __forceinline__ float at_coef(int o, int a) {
  return o == 0 ? (a < 3 ? 1.f : 0.f) : (a == 0 ? 0.f : (a == 1 ? 1.f : -1.f));
}

// exponent eV of the V scale from the input bound: 8 * amax * 2^eV in [2^11, 2^12); 0 for a zero / non-finite bound or no
// buffer.  Whole-wave call (lf_amax_read shuffles).
__device__ __forceinline__ int v_scale_exp(const float* amax_in, int lane) {
  if (amax_in == nullptr) return 0;
  const float b = 8.f * lf_amax_read(amax_in, lane);
  if (!(b > 0.f) || !(b < 3.0e38f)) return 0;
  int ex;
  frexpf(b, &ex);                                                // b = m 2^ex, m in [0.5, 1)
  return 12 - ex;
}

__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}

// one wave per (tile, z-frequency a), lanes over channel quads of the padded record (CP = CinP); the arithmetic of
// wino3d_input_kernel (wino_gemm.hip) in fp32, then scale and split
__global__ void __launch_bounds__(256) wino3d_input_f16x3_kernel(const float* __restrict__ x, const float* __restrict__ amax_in,
                                                                _Float16* __restrict__ V, int D, int H, int W, int C, int CP,
                                                                int tz, int ty, int tx, long T) {
  const int lane = threadIdx.x & 63, a = threadIdx.x >> 6;
  const long tile = blockIdx.x;
  long r = tile;
  const int bx = (int)(r % tx); r /= tx;
  const int by = (int)(r % ty); r /= ty;
  const int bz = (int)(r % tz);
  const int n = (int)(r / tz);
  const int z0 = 2 * bz - 1, y0 = 2 * by - 1, x0 = 2 * bx - 1;
  const int dza = (a == 0) ? 0 : (a == 2 ? 2 : 1);
  const int dzb = (a == 0) ? 2 : (a == 1 ? 2 : (a == 2 ? 1 : 3));
  const float sb = (a == 1) ? 1.f : -1.f;
  const int za = z0 + dza, zb = z0 + dzb;
  const bool za_ok = (unsigned)za < (unsigned)D, zb_ok = (unsigned)zb < (unsigned)D;
  const float* xs = x + (long)n * D * H * W * C;
  const float sc = ldexpf(1.f, v_scale_exp(amax_in, lane));
  for (int q = lane; q * 4 < CP; q += 64) {
    const bool live = q * 4 < C;                                 // channels C .. CP-1: zero padding of the record
    f32x4 vx[4][4];
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
      const int yy = y0 + dy;
      const bool y_ok = live && (unsigned)yy < (unsigned)H;
      f32x4 d[4];
#pragma unroll
      for (int dx = 0; dx < 4; ++dx) {
        const int xx = x0 + dx;
        const bool ok = y_ok && (unsigned)xx < (unsigned)W;
        f32x4 va = (f32x4){0.f, 0.f, 0.f, 0.f}, vb = va;
        if (ok && za_ok) va = *(const f32x4*)(xs + (((long)za * H + yy) * W + xx) * C + q * 4);
        if (ok && zb_ok) vb = *(const f32x4*)(xs + (((long)zb * H + yy) * W + xx) * C + q * 4);
        d[dx] = va + vb * sb;
      }
      vx[dy][0] = d[0] - d[2];
      vx[dy][1] = d[1] + d[2];
      vx[dy][2] = d[2] - d[1];
      vx[dy][3] = d[1] - d[3];
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 v = ((b == 0) ? (vx[0][c] - vx[2][c]) : (b == 1) ? (vx[1][c] + vx[2][c])
                       : (b == 2) ? (vx[2][c] - vx[1][c]) : (vx[1][c] - vx[3][c])) * sc;
        const h16x4 hi = __builtin_convertvector(v, h16x4);
        const h16x4 lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x4), h16x4);
        _Float16* p = V + ((long)(a * 16 + b * 4 + c) * T + tile) * CP * 2 + (q >> 3) * 64 + (q & 7) * 4;
        *(h16x4*)p = hi;
        *(h16x4*)(p + 32) = lo;
      }
  }
}

// F(2x2,3x3) input transform of channels c .. c+3 of the 4 x 4 patch at (y0, x0): v[b*4 + c'] (the arithmetic of
// wino2d_input_kernel, wino_gemm.hip, in fp32); live = false: zeros (channel padding of the record)
__device__ __forceinline__ void wino2d_xform4(const float* __restrict__ xs, int y0, int x0, int H, int W, int C, int c, bool live,
                                              f32x4 v[16]) {
  f32x4 vx[4][4];
#pragma unroll
  for (int dy = 0; dy < 4; ++dy) {
    const int yy = y0 + dy;
    f32x4 d[4];
#pragma unroll
    for (int dx = 0; dx < 4; ++dx) {
      const int xx = x0 + dx;
      d[dx] = (live && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? *(const f32x4*)(xs + ((long)yy * W + xx) * C + c)
                                                                                  : (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    vx[dy][0] = d[0] - d[2];
    vx[dy][1] = d[1] + d[2];
    vx[dy][2] = d[2] - d[1];
    vx[dy][3] = d[1] - d[3];
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
      v[b * 4 + cc] = (b == 0) ? (vx[0][cc] - vx[2][cc]) : (b == 1) ? (vx[1][cc] + vx[2][cc])
                    : (b == 2) ? (vx[2][cc] - vx[1][cc]) : (vx[1][cc] - vx[3][cc]);
}

// 2-D: one wave per tile.  The tile's input scale is its own: pass 1 takes the largest FINITE |V| of the tile over all
// channels and frequencies (eV: that maximum times 2^eV in [2^11, 2^12); 0 for an all-zero tile) -- no bound has to be handed
// over by a producer, and a tile of small values keeps its precision next to one of large values.  Non-finite values are
// left out of the maximum and pass through as inf / NaN, so exactly the frequencies they reach become non-finite, as in the
// fp32 kernel.  Pass 2 recomputes the transform (the patch is cache-hot), scales, splits and stores 8 channels per lane:
// one 16-byte store of hi and one of lo.
__global__ void __launch_bounds__(256) wino2d_input_f16x3_kernel(const float* __restrict__ x, _Float16* __restrict__ V,
                                                                int* __restrict__ eVt, int H, int W, int C, int CP, int ty, int tx,
                                                                long T) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long tile = (long)blockIdx.x * 4 + wave;
  if (tile >= T) return;                                         // wave-uniform
  long r = tile;
  const int bx = (int)(r % tx); r /= tx;
  const int by = (int)(r % ty);
  const long n = r / ty;
  const int y0 = 2 * by - 1, x0 = 2 * bx - 1;
  const float* xs = x + n * H * W * C;
  float m = 0.f;
  for (int q = lane; q * 4 < C; q += 64) {
    f32x4 v[16];
    wino2d_xform4(xs, y0, x0, H, W, C, q * 4, true, v);
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float a = fabsf(v[i][e]);
        m = a < __builtin_inff() ? fmaxf(m, a) : m;
      }
  }
  m = wave_max(m);
  int eV = 0;
  if (m > 0.f) {
    int ex;
    frexpf(m, &ex);                                              // m = f 2^ex, f in [0.5, 1)
    eV = 12 - ex;
  }
  if (lane == 0) eVt[tile] = eV;
  for (int g = lane; g * 8 < CP; g += 64) {
    f32x4 v0[16], v1[16];
    wino2d_xform4(xs, y0, x0, H, W, C, g * 8, g * 8 < C, v0);
    wino2d_xform4(xs, y0, x0, H, W, C, g * 8 + 4, g * 8 + 4 < C, v1);
    _Float16* p = V + tile * CP * 2 + (g >> 2) * 64 + (g & 3) * 8;
#pragma unroll
    for (int f = 0; f < 16; ++f) {
      h16x8 hi, lo;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float s = ldexpf(e < 4 ? v0[f][e] : v1[f][e - 4], eV);
        hi[e] = (_Float16)s;
        lo[e] = (_Float16)(s - (float)hi[e]);
      }
      *(h16x8*)(p + (long)f * T * CP * 2) = hi;
      *(h16x8*)(p + (long)f * T * CP * 2 + 32) = lo;
    }
  }
}

// Workgroup shape: WM x WN waves, each owning BA x BB blocks of 16 couts x 16 tiles.  3-D: the 128 x 64 shape that the fp32
// kernel uses for the 128-render 256 -> 256 launch (8 waves, one workgroup per CU); smaller problems are split over the
// frequencies.  2-D (F(2x2,3x3), 4 output accumulators per block instead of 8): 128 x 128, or 64 x 128 when CoutP = 64.
// The body is a template; every shape has its own NON-template __global__ entry point (hipcc 7.2 emitted no host stub for
// a __global__ template of this kernel).
//   eVt == nullptr (3-D): one input scale 2^eV from amax_in, osc = he 2^-(eU+eV).
//   eVt != nullptr (2-D): per-tile input scale 2^eVt[tile] chosen by lf_wino2d_input_transform_f16x3; y = 2^-eVt[tile] (he 2^-eU M).
constexpr int WM = 4, WN = 2, BA = 2, BB = 2;
constexpr int NT = WM * BA * 16, MT = WN * BB * 16, NTHR = WM * WN * 64;
constexpr int LDS_BYTES = NSTAGE * (NT + MT) * 128;
constexpr int NT2 = 128, MT2 = 128, NT2S = 64, MT2S = 128;      // 2-D shapes: <2,4,2,2,4> and <2,2,4,2,2>
constexpr int LDS2_BYTES = NSTAGE * (NT2 + MT2) * 128, LDS2S_BYTES = NSTAGE * (NT2S + MT2S) * 128;

template <int DIMS, int WM, int WN, int BA, int BB>
__device__ __forceinline__ void f16x3_gemm_body(
    const _Float16* __restrict__ V, const _Float16* __restrict__ U2, const float* __restrict__ bias, float* __restrict__ y,
    long T, int tz, int ty, int tx, int D, int H, int W, int CinP, int Cout, int CoutP, float he, int eU,
    const float* __restrict__ amax_in, const int* __restrict__ eVt, unsigned flags, float slope, float* __restrict__ partial,
    long ysize, float* __restrict__ amax_out) {
  constexpr int F = DIMS == 3 ? 64 : 16, NO = DIMS == 3 ? 8 : 4;
  constexpr int NTc = WM * BA * 16, MTc = WN * BB * 16, NW = WM * WN;
  constexpr int A_BYTES = NTc * 128, STAGE_BYTES = (NTc + MTc) * 128;
  constexpr int PA = NTc / 8, PB = MTc / 8;
  constexpr int PPW = (PA + PB) / NW;
  static_assert((PA + PB) % NW == 0 && PPW <= BA * BB, "pieces must split evenly over the waves and fit the issue slots");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w / WN, wc = w % WN;
  const int lr = lane & 15, kg = lane >> 4;
  // XCD-aware order of wino_fused_kernel: the channel blocks of one tile block run side by side on one XCD
  int bxi = blockIdx.x, byi = blockIdx.y;
  if (gridDim.y > 1 && (gridDim.x & 7) == 0) {
    const unsigned L = blockIdx.x + gridDim.x * blockIdx.y, slot = L >> 3;
    byi = (int)(slot % gridDim.y);
    bxi = (int)((slot / gridDim.y) * 8 + (L & 7));
  }
  const long m0 = (long)bxi * MTc;
  const int n0 = byi * NTc;

  // LDS-DMA staging, swizzle applied on the global side (see wino_fused.hip); rows are CinP * 4 bytes (hi + lo records)
  const u32 slabV = (u32)((long)T * CinP * 4);
  const u32 slabU = (u32)((long)CoutP * CinP * 4);
  int voff[PPW], ldso[PPW];
  bool isA[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int p = w * PPW + i;
    isA[i] = p < PA;
    const int piece = isA[i] ? p : p - PA;
    const int pos = piece * 64 + lane, r = pos >> 3, c = (pos & 7) ^ ((r >> 1) & 7);
    if (isA[i]) {
      const long off = (long)(n0 + r) * CinP * 4 + c * 16;
      voff[i] = off < (long)slabU ? (int)(u32)off : 0x7fffffff;
      ldso[i] = piece * 1024;
    } else {
      const long row = m0 + r;
      voff[i] = row < T ? (int)((u32)row * (u32)CinP * 4u + (u32)c * 16u) : 0x7fffffff;
      ldso[i] = A_BYTES + piece * 1024;
    }
  }
  const int nk = CinP / KC;
  const int fper = F / gridDim.z, f_first = blockIdx.z * fper;
  const int S = fper * nk;
  const long strideU = (long)slabU, strideV = (long)T * CinP * 4;             // bytes per frequency slab
  const unsigned char* pU = (const unsigned char*)U2 + (long)f_first * strideU;
  const unsigned char* pV = (const unsigned char*)V + (long)f_first * strideV;
  __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)pU, 0, slabU, 0x00020000);
  __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)pV, 0, slabV, 0x00020000);
  int ik = 0, islot = 0, issued = 0;
  auto issue_piece = [&](int q) {
    unsigned char* slot = smem + islot * STAGE_BYTES;
    const int k0b = ik * KC * 4;                                 // byte offset of the 32-channel record
    if (isA[q])
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ru, (__attribute__((address_space(3))) void*)(slot + ldso[q]), 16, voff[q], k0b, 0, 0);
    else
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void*)(slot + ldso[q]), 16, voff[q], k0b, 0, 0);
    if (q == PPW - 1) {
      ++issued;
      islot = (islot + 1) & (NSTAGE - 1);
      if (++ik == nk) {
        ik = 0;
        pU += strideU;
        pV += strideV;
        ru = __builtin_amdgcn_make_buffer_rsrc((void*)pU, 0, slabU, 0x00020000);
        rv = __builtin_amdgcn_make_buffer_rsrc((void*)pV, 0, slabV, 0x00020000);
      }
    }
  };

  // operand addresses: [row block][0 = hi chunk kg, 1 = lo chunk 4 + kg]
  int rdA[BA][2], rdB[BB][2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int t = 0; t < BA; ++t) rdA[t][j] = lds_chunk(wr * (BA * 16) + t * 16 + lr, j * 4 + kg);
#pragma unroll
    for (int t = 0; t < BB; ++t) rdB[t][j] = A_BYTES + lds_chunk(wc * (BB * 16) + t * 16 + lr, j * 4 + kg);
  }

  f32x4 Y[NO][BA][BB];
#pragma unroll
  for (int o = 0; o < NO; ++o)
#pragma unroll
    for (int a = 0; a < BA; ++a)
#pragma unroll
      for (int b = 0; b < BB; ++b) Y[o][a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 acc[BA][BB];
#pragma unroll
  for (int a = 0; a < BA; ++a)
#pragma unroll
    for (int b = 0; b < BB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  for (int s0 = 0; s0 < NSTAGE - 1 && s0 < S; ++s0)
#pragma unroll
    for (int q = 0; q < PPW; ++q) issue_piece(q);
  int kc = 0, f = f_first;
  for (int s = 0; s < S; ++s) {
    const int ahead = min(NSTAGE - 2, S - 1 - s);
    if (ahead >= 2) __builtin_amdgcn_s_waitcnt(0x0f70 | ((2 * PPW) & 15) | (((2 * PPW) >> 4) << 14));
    else if (ahead == 1) __builtin_amdgcn_s_waitcnt(0x0f70 | (PPW & 15));
    else __builtin_amdgcn_s_waitcnt(0x0f70);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const bool more = issued < S;
    const unsigned char* base = smem + (s % NSTAGE) * STAGE_BYTES;
    h16x8 ah[BA], al[BA], bh[BB], bl[BB];
#pragma unroll
    for (int t = 0; t < BA; ++t) {
      ah[t] = *(const h16x8*)(base + rdA[t][0]);
      al[t] = *(const h16x8*)(base + rdA[t][1]);
    }
#pragma unroll
    for (int t = 0; t < BB; ++t) {
      bh[t] = *(const h16x8*)(base + rdB[t][0]);
      bl[t] = *(const h16x8*)(base + rdB[t][1]);
    }
    // three terms per block, small ones first; one DMA piece of stage s+3 after each block's three MFMAs
#pragma unroll
    for (int a = 0; a < BA; ++a)
#pragma unroll
      for (int b = 0; b < BB; ++b) {
        acc[a][b] = mfma16(al[a], bh[b], acc[a][b]);
        acc[a][b] = mfma16(ah[a], bl[b], acc[a][b]);
        acc[a][b] = mfma16(ah[a], bh[b], acc[a][b]);
        const int slot_ = a * BB + b;
        __builtin_amdgcn_sched_barrier(0);
        if (slot_ < PPW && more) issue_piece(slot_);
        __builtin_amdgcn_sched_barrier(0);
      }
    if (++kc == nk) {
      kc = 0;
      const int fc = f & 3, fb_ = (f >> 2) & 3, fa_ = (f >> 4) & 3;
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        float cf = at_coef(o & 1, fc) * at_coef((o >> 1) & 1, fb_);
        if (DIMS == 3) cf *= at_coef((o >> 2) & 1, fa_);
        if (cf != 0.f) {
#pragma unroll
          for (int a = 0; a < BA; ++a)
#pragma unroll
            for (int b = 0; b < BB; ++b) Y[o][a][b] += acc[a][b] * cf;
        }
      }
#pragma unroll
      for (int a = 0; a < BA; ++a)
#pragma unroll
        for (int b = 0; b < BB; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
      ++f;
    }
  }

  // ---- epilogue: he * 2^-(eU + eV), bias, LeakyReLU ----
  const float osc = DIMS == 3 ? ldexpf(he, -(eU + v_scale_exp(amax_in, lane))) : ldexpf(he, -eU);
  float m = 0.f;
#pragma unroll
  for (int b = 0; b < BB; ++b) {
    const long tile = m0 + wc * (BB * 16) + b * 16 + lr;
    if (tile >= T) continue;
    long r = tile;
    const int bx = (int)(r % tx); r /= tx;
    const int by = (int)(r % ty); r /= ty;
    const int bz = DIMS == 3 ? (int)(r % tz) : 0;
    const long n = DIMS == 3 ? r / tz : r;
    const int etile = DIMS == 3 ? 0 : eVt[tile];
#pragma unroll
    for (int a = 0; a < BA; ++a) {
      const int co = n0 + wr * (BA * 16) + a * 16 + kg * 4;
      if (co >= Cout) continue;
      f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (bias != nullptr) bv = *(const f32x4*)(bias + co);
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const int gx = 2 * bx + (o & 1), gy = 2 * by + ((o >> 1) & 1), gz = 2 * bz + (DIMS == 3 ? ((o >> 2) & 1) : 0);
        if (gx >= W || gy >= H || gz >= D) continue;
        const long vox = (flags & LF_OUT_DEPTH_INNER) ? ((n * H + gy) * W + gx) * D + gz : ((n * D + gz) * H + gy) * W + gx;
        if (partial != nullptr) {
          *(f32x4*)(partial + (long)blockIdx.z * ysize + vox * Cout + co) = Y[o][a][b];
          continue;
        }
        f32x4 v = Y[o][a][b] * osc;
        if (DIMS == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = ldexpf(v[e], -etile);              // exact (a power of two)
        }
        v += bv;
        if (flags & LF_EPI_LRELU) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], v[e] * slope);
        }
        if (DIMS == 3) {
#pragma unroll
          for (int e = 0; e < 4; ++e) m = fmaxf(m, fabsf(v[e]));
        }
        *(f32x4*)(y + vox * Cout + co) = v;
      }
    }
  }
  if (DIMS == 3 && amax_out != nullptr) lf_amax_publish(amax_out, wave_max(m), lane);
}

__global__ void __launch_bounds__(NTHR, 1) wino_fused_f16x3_kernel(
    const _Float16* __restrict__ V, const _Float16* __restrict__ U2, const float* __restrict__ bias, float* __restrict__ y,
    long T, int tz, int ty, int tx, int D, int H, int W, int CinP, int Cout, int CoutP, float he, int eU,
    const float* __restrict__ amax_in, unsigned flags, float slope, float* __restrict__ partial, long ysize,
    float* __restrict__ amax_out) {
  f16x3_gemm_body<3, WM, WN, BA, BB>(V, U2, bias, y, T, tz, ty, tx, D, H, W, CinP, Cout, CoutP, he, eU, amax_in, nullptr, flags, slope,
                                     partial, ysize, amax_out);
}

__global__ void __launch_bounds__(512, 1) wino_fused2d_f16x3_kernel(
    const _Float16* __restrict__ V, const _Float16* __restrict__ U2, const float* __restrict__ bias, float* __restrict__ y,
    long T, int ty, int tx, int H, int W, int CinP, int Cout, int CoutP, float he, int eU, const int* __restrict__ eVt,
    unsigned flags, float slope, float* __restrict__ partial, long ysize) {
  f16x3_gemm_body<2, 4, 2, 2, 4>(V, U2, bias, y, T, 1, ty, tx, 1, H, W, CinP, Cout, CoutP, he, eU, nullptr, eVt, flags, slope, partial,
                                 ysize, nullptr);
}

__global__ void __launch_bounds__(512, 1) wino_fused2d_f16x3_c64_kernel(
    const _Float16* __restrict__ V, const _Float16* __restrict__ U2, const float* __restrict__ bias, float* __restrict__ y,
    long T, int ty, int tx, int H, int W, int CinP, int Cout, int CoutP, float he, int eU, const int* __restrict__ eVt,
    unsigned flags, float slope, float* __restrict__ partial, long ysize) {
  f16x3_gemm_body<2, 2, 4, 2, 2>(V, U2, bias, y, T, 1, ty, tx, 1, H, W, CinP, Cout, CoutP, he, eU, nullptr, eVt, flags, slope, partial,
                                 ysize, nullptr);
}

// y = epilogue(he 2^-(eU+eV) * sum_z partial[z] + bias), partials added in a fixed order
__global__ void __launch_bounds__(256) wino_fused_f16x3_finish_kernel(const f32x4* __restrict__ partial, const float* __restrict__ bias,
                                                                     f32x4* __restrict__ y, long n4, int zs, int c4, float he, int eU,
                                                                     const float* __restrict__ amax_in, unsigned flags, float slope,
                                                                     float* __restrict__ amax_out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const float osc = ldexpf(he, -(eU + v_scale_exp(amax_in, lane)));
  float m = 0.f;
  if (i < n4) {
    f32x4 acc = partial[i];
    for (int z = 1; z < zs; ++z) acc += partial[i + z * n4];
    f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (bias != nullptr) bv = *(const f32x4*)(bias + (i % c4) * 4);
    f32x4 v = acc * osc + bv;
    if (flags & LF_EPI_LRELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], v[e] * slope);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) m = fmaxf(m, fabsf(v[e]));
    y[i] = v;
  }
  if (amax_out != nullptr) lf_amax_publish(amax_out, wave_max(m), lane);
}

// 2-D: y = epilogue(2^-eVt[tile] (he 2^-eU sum_z partial[z]) + bias), partials added in a fixed order
__global__ void __launch_bounds__(256) wino_fused2d_f16x3_finish_kernel(const f32x4* __restrict__ partial, const float* __restrict__ bias,
                                                                       f32x4* __restrict__ y, long n4, int zs, int c4, int H, int W,
                                                                       int ty, int tx, float heU, const int* __restrict__ eVt,
                                                                       unsigned flags, float slope) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  f32x4 acc = partial[i];
  for (int z = 1; z < zs; ++z) acc += partial[i + z * n4];
  const long p = i / c4;
  const int gx = (int)(p % W), gy = (int)((p / W) % H);
  const long n = p / ((long)W * H);
  const int e = eVt[(n * ty + gy / 2) * tx + gx / 2];
  f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (bias != nullptr) bv = *(const f32x4*)(bias + (i % c4) * 4);
  f32x4 v = acc * heU;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = ldexpf(v[k], -e);
  v += bv;
  if (flags & LF_EPI_LRELU) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], v[k] * slope);
  }
  y[i] = v;
}

int zsplit(long gx, int gy, int F = 64) {                        // enough workgroups for one per CU
  int zs = 1;
  while (zs < F && gx * gy * zs < 256) zs <<= 1;
  return zs;
}

// 2-D workgroup shape: 64 x 128 for 64-channel outputs (no half-empty A blocks), else 128 x 128
int nt2d(int CoutP) { return CoutP == 64 ? NT2S : NT2; }

void tiles_of(int D, int H, int W, int& tz, int& ty, int& tx) { tz = (D + 1) / 2, ty = (H + 1) / 2, tx = (W + 1) / 2; }

}  // namespace

extern "C" int lf_wino_f16x3_cin_padded(int Cin) { return (Cin + 31) / 32 * 32; }

extern "C" int lf_wino3d_input_transform_f16x3(const float* x, const float* amax_in, void* V, int N, int D, int H, int W, int C,
                                               void* stream) {
  lf_clear_error();
  if (x == nullptr || V == nullptr || N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return LF_EINVAL;
  if (!lf_aligned16(x) || !lf_aligned16(V)) return LF_EALIGN;
  int tz, ty, tx;
  tiles_of(D, H, W, tz, ty, tx);
  const long T = (long)N * tz * ty * tx;
  if (T >= 0x7fffffffL) return LF_EINVAL;
  hipLaunchKernelGGL(wino3d_input_f16x3_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, x, amax_in, (_Float16*)V, D, H,
                     W, C, lf_wino_f16x3_cin_padded(C), tz, ty, tx, T);
  return lf_launch_status();
}

extern "C" size_t lf_wino_fused_f16x3_scratch_bytes(int N, int D, int H, int W, int Cout) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  int tz, ty, tx;
  tiles_of(D, H, W, tz, ty, tx);
  const long T = (long)N * tz * ty * tx;
  const int CoutP = lf_wino_fused_cout_padded(Cout);
  const int zs = zsplit((T + MT - 1) / MT, (CoutP + NT - 1) / NT);
  return zs > 1 ? (size_t)zs * N * D * H * W * Cout * sizeof(float) : 0;
}

extern "C" int lf_wino_fused_f16x3_gemm(const void* V, const void* U2, int eU, const float* amax_in, const float* bias, float* y,
                                        float* amax_out, void* scratch, size_t scratch_bytes, int N, int D, int H, int W, int Cin,
                                        int Cout, float he, unsigned flags, float slope, void* stream) {
  lf_clear_error();
  if (V == nullptr || U2 == nullptr || y == nullptr) return LF_EINVAL;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 3) || (Cout & 3)) return LF_EINVAL;
  if ((flags & ~(LF_EPI_LRELU | LF_OUT_DEPTH_INNER)) || eU < -100 || eU > 100) return LF_EINVAL;
  if (!lf_aligned16(V) || !lf_aligned16(U2) || !lf_aligned16(y) || (bias && !lf_aligned16(bias))) return LF_EALIGN;
  int tz, ty, tx;
  tiles_of(D, H, W, tz, ty, tx);
  const long T = (long)N * tz * ty * tx;
  const int CoutP = lf_wino_fused_cout_padded(Cout), CinP = lf_wino_f16x3_cin_padded(Cin);
  if (T * CinP * 4 > 0xffffffffL || (long)CoutP * CinP * 4 > 0xffffffffL) return LF_EINVAL;
  const long gx = (T + MT - 1) / MT;
  const int gy = (CoutP + NT - 1) / NT;
  if (gx > 0x7fffffffL || gy > 65535) return LF_EINVAL;
  const int zs = zsplit(gx, gy);
  const long ysize = (long)N * D * H * W * Cout;
  if (zs > 1 && (scratch == nullptr || scratch_bytes < (size_t)zs * ysize * sizeof(float) || !lf_aligned16(scratch))) return LF_ENOSPC;
  float* partial = zs > 1 ? (float*)scratch : nullptr;
  hipStream_t s = (hipStream_t)stream;
  static lf_devmask_t attr_set;
  {
    hipError_t e = lf_ensure_dyn_lds(attr_set, (const void*)wino_fused_f16x3_kernel, LDS_BYTES);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(wino_fused_f16x3_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)zs), dim3(NTHR), LDS_BYTES, s,
                     (const _Float16*)V, (const _Float16*)U2, bias, y, T, tz, ty, tx, D, H, W, CinP, Cout, CoutP, he, eU, amax_in,
                     flags, slope, partial, ysize, amax_out);
  const int st = lf_launch_status();
  if (st || zs == 1) return st;
  const long n4 = ysize / 4;
  hipLaunchKernelGGL(wino_fused_f16x3_finish_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const f32x4*)partial, bias,
                     (f32x4*)y, n4, zs, Cout / 4, he, eU, amax_in, flags & LF_EPI_LRELU, slope, amax_out);
  return lf_launch_status();
}

// ---- 2-D, F(2x2,3x3): decoder layers (modules/blocks.py:152-158 with modules/equalized.py:57-64, 2-D) ----
extern "C" int lf_wino2d_input_transform_f16x3(const float* x, void* V, int* eV, int N, int H, int W, int C, void* stream) {
  lf_clear_error();
  if (x == nullptr || V == nullptr || eV == nullptr || N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return LF_EINVAL;
  if (!lf_aligned16(x) || !lf_aligned16(V) || ((uintptr_t)eV & 3)) return LF_EALIGN;
  const long T = (long)N * ((H + 1) / 2) * ((W + 1) / 2);
  if (T >= 0x7fffffffL || (long)N * H * W * C >= (1L << 40)) return LF_EINVAL;
  hipLaunchKernelGGL(wino2d_input_f16x3_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, (_Float16*)V, eV,
                     H, W, C, lf_wino_f16x3_cin_padded(C), (H + 1) / 2, (W + 1) / 2, T);
  return lf_launch_status();
}

extern "C" size_t lf_wino_fused2d_f16x3_scratch_bytes(int N, int H, int W, int Cout) {
  if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  const long T = (long)N * ((H + 1) / 2) * ((W + 1) / 2);
  const int CoutP = lf_wino_fused_cout_padded(Cout), nt = nt2d(CoutP);
  const int zs = zsplit((T + MT2 - 1) / MT2, (CoutP + nt - 1) / nt, 16);
  return zs > 1 ? (size_t)zs * N * H * W * Cout * sizeof(float) : 0;
}

extern "C" int lf_wino_fused2d_f16x3_gemm(const void* V, const int* eV, const void* U2, int eU, const float* bias, float* y,
                                          void* scratch, size_t scratch_bytes, int N, int H, int W, int Cin, int Cout, float he,
                                          unsigned flags, float slope, void* stream) {
  lf_clear_error();
  if (V == nullptr || eV == nullptr || U2 == nullptr || y == nullptr) return LF_EINVAL;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 3) || (Cout & 3)) return LF_EINVAL;
  if ((flags & ~LF_EPI_LRELU) || eU < -100 || eU > 100) return LF_EINVAL;
  if (!lf_aligned16(V) || !lf_aligned16(U2) || !lf_aligned16(y) || (bias && !lf_aligned16(bias)) || ((uintptr_t)eV & 3)) return LF_EALIGN;
  const int ty = (H + 1) / 2, tx = (W + 1) / 2;
  const long T = (long)N * ty * tx;
  const int CoutP = lf_wino_fused_cout_padded(Cout), CinP = lf_wino_f16x3_cin_padded(Cin);
  if (T * CinP * 4 > 0xffffffffL || (long)CoutP * CinP * 4 > 0xffffffffL) return LF_EINVAL;
  const int nt = nt2d(CoutP);
  const long gx = (T + MT2 - 1) / MT2;
  const int gy = (CoutP + nt - 1) / nt;
  if (gx > 0x7fffffffL || gy > 65535) return LF_EINVAL;
  const int zs = zsplit(gx, gy, 16);
  const long ysize = (long)N * H * W * Cout;
  if (zs > 1 && (scratch == nullptr || scratch_bytes < (size_t)zs * ysize * sizeof(float) || !lf_aligned16(scratch))) return LF_ENOSPC;
  float* partial = zs > 1 ? (float*)scratch : nullptr;
  hipStream_t s = (hipStream_t)stream;
  const void* kern = nt == NT2 ? (const void*)wino_fused2d_f16x3_kernel : (const void*)wino_fused2d_f16x3_c64_kernel;
  const int lds = nt == NT2 ? LDS2_BYTES : LDS2S_BYTES;
  static lf_devmask_t attr_big, attr_c64;
  {
    hipError_t e = lf_ensure_dyn_lds(nt == NT2 ? attr_big : attr_c64, kern, lds);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)zs);
  if (nt == NT2)
    hipLaunchKernelGGL(wino_fused2d_f16x3_kernel, grid, dim3(512), lds, s, (const _Float16*)V, (const _Float16*)U2, bias, y, T, ty, tx,
                       H, W, CinP, Cout, CoutP, he, eU, eV, flags, slope, partial, ysize);
  else
    hipLaunchKernelGGL(wino_fused2d_f16x3_c64_kernel, grid, dim3(512), lds, s, (const _Float16*)V, (const _Float16*)U2, bias, y, T, ty,
                       tx, H, W, CinP, Cout, CoutP, he, eU, eV, flags, slope, partial, ysize);
  const int st = lf_launch_status();
  if (st || zs == 1) return st;
  const long n4 = ysize / 4;
  hipLaunchKernelGGL(wino_fused2d_f16x3_finish_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const f32x4*)partial, bias,
                     (f32x4*)y, n4, zs, Cout / 4, H, W, ty, tx, ldexpf(he, -eU), eV, flags, slope);
  return lf_launch_status();
}
