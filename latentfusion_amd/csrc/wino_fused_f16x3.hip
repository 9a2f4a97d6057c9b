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
#include "wino_ring.h"

namespace {

using wino_ring::KC;
using wino_ring::NSTAGE;
using wino_ring::at_coef;
using wino_ring::lds_chunk;
using wino_ring::u32;

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16(const h16x8 a, const h16x8 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
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

// one wave per (tile, z-frequency a), lanes over channel quads of the padded record (CP = CinP); the transform of
// wino3d_input_kernel (wino_gemm.hip; wino_xform.inc) in fp32, then scale and split
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
#define WINO_XFORM_DIMS 3
#define WINO_XFORM_LIVE live
#define WINO_XFORM_CH (q * 4)
#include "wino_xform.inc"
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const f32x4 v = WINO_XFORM_COL(vx, b, c) * sc;
        const h16x4 hi = __builtin_convertvector(v, h16x4);
        const h16x4 lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x4), h16x4);
        _Float16* p = V + ((long)(a * 16 + b * 4 + c) * T + tile) * CP * 2 + (q >> 3) * 64 + (q & 7) * 4;
        *(h16x4*)p = hi;
        *(h16x4*)(p + 32) = lo;
      }
  }
}

// F(2x2,3x3) input transform of channels c .. c+3 of the 4 x 4 patch at (y0, x0): v[b*4 + c'] (wino_xform.inc);
// live = false: zeros (channel padding of the record)
__device__ __forceinline__ void wino2d_xform4(const float* __restrict__ xs, int y0, int x0, int H, int W, int C, int c, bool live,
                                              f32x4 v[16]) {
#define WINO_XFORM_DIMS 2
#define WINO_XFORM_LIVE live
#define WINO_XFORM_CH c
#include "wino_xform.inc"
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int cc = 0; cc < 4; ++cc)
      v[b * 4 + cc] = WINO_XFORM_COL(vx, b, cc);
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

// per-value epilogue of the direct store and of the finish kernels: osc = he 2^-(eU + eV) (3-D) or he 2^-eU followed by the
// exact 2^-eVt[tile] (2-D), bias, LeakyReLU; 3-D keeps the running max |y| in m
template <int DIMS>
struct EpiF16x3 {
  float osc, slope;
  unsigned flags;
  const int* __restrict__ eVt;
  float m;
  __device__ __forceinline__ int tile_exp(long tile) const { return DIMS == 3 ? 0 : eVt[tile]; }
  __device__ __forceinline__ f32x4 operator()(const f32x4 yv, const f32x4 bv, int etile) {
    f32x4 v = yv * osc;
    if (DIMS == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ldexpf(v[e], -etile);                  // exact (a power of two)
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
    return v;
  }
};

template <int DIMS, int WM, int WN, int BA, int BB>
__device__ __forceinline__ void f16x3_gemm_body(
    const _Float16* __restrict__ V, const _Float16* __restrict__ U2, const float* __restrict__ bias, float* __restrict__ y,
    long T, int tz, int ty, int tx, int D, int H, int W, int CinP, int Cout, int CoutP, float he, int eU,
    const float* __restrict__ amax_in, const int* __restrict__ eVt, unsigned flags, float slope, float* __restrict__ partial,
    long ysize, float* __restrict__ amax_out) {
#define WINO_RING_K CinP
#define WINO_RING_RAGGED 0
#define WINO_RING_SETUP
#include "wino_ring.inc"
  static_assert(PPW <= BA * BB, "one issue slot per piece");
  for (int s = 0; s < S; ++s) {
    wino_ring::wait<PPW>(min(NSTAGE - 2, S - 1 - s));
    const bool more = issued < S;
    const unsigned char* base = smem + (s % NSTAGE) * STAGE_BYTES;
    // product step: a stage row is one record, chunks 0-3 hi and 4-7 lo; lane group kg reads chunk kg (rdA/rdB [..][0]) and
    // chunk 4 + kg ([..][1]): 8 consecutive k each, so the contraction over the 32 channels is ONE 16x16x32 MFMA per term
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
#define WINO_RING_FOLD
#include "wino_ring.inc"
  }
  EpiF16x3<DIMS> epi{DIMS == 3 ? ldexpf(he, -(eU + v_scale_exp(amax_in, lane))) : ldexpf(he, -eU), slope, flags, eVt, 0.f};
#define WINO_RING_STORE
#include "wino_ring.inc"
#undef WINO_RING_K
#undef WINO_RING_RAGGED
  if (DIMS == 3 && amax_out != nullptr) lf_amax_publish(amax_out, wave_max(epi.m), lane);
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
  EpiF16x3<3> epi{ldexpf(he, -(eU + v_scale_exp(amax_in, lane))), slope, flags, nullptr, 0.f};
  if (i < n4) y[i] = wino_ring::finish_value(partial, bias, i, n4, zs, c4, epi);
  if (amax_out != nullptr) lf_amax_publish(amax_out, wave_max(epi.m), lane);
}

// 2-D: y = epilogue(2^-eVt[tile] (he 2^-eU sum_z partial[z]) + bias), partials added in a fixed order.  (Spelled out, not
// finish_value + EpiF16x3<2>: through the functor the compiler swaps the operands of the bias add in this one kernel.)
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

constexpr long WANT = 256;                                       // workgroups before a launch stops splitting: one per CU

// 2-D workgroup shape: 64 x 128 for 64-channel outputs (no half-empty A blocks), else 128 x 128
int nt2d(int CoutP) { return CoutP == 64 ? NT2S : NT2; }

}  // namespace

extern "C" int lf_wino_f16x3_cin_padded(int Cin) { return (Cin + 31) / 32 * 32; }

extern "C" int lf_wino3d_input_transform_f16x3(const float* x, const float* amax_in, void* V, int N, int D, int H, int W, int C,
                                               void* stream) {
  lf_clear_error();
  if (x == nullptr || V == nullptr || N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3)) return LF_EINVAL;
  if (!lf_aligned16(x) || !lf_aligned16(V)) return LF_EALIGN;
  const wino_ring::Tiles t(3, N, D, H, W);
  if (t.T >= 0x7fffffffL) return LF_EINVAL;
  hipLaunchKernelGGL(wino3d_input_f16x3_kernel, dim3((unsigned)t.T), dim3(256), 0, (hipStream_t)stream, x, amax_in, (_Float16*)V, D, H,
                     W, C, lf_wino_f16x3_cin_padded(C), t.tz, t.ty, t.tx, t.T);
  return lf_launch_status();
}

extern "C" size_t lf_wino_fused_f16x3_scratch_bytes(int N, int D, int H, int W, int Cout) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cout <= 0) return 0;
  wino_ring::Plan p(3, N, D, H, W, Cout);
  p.split(64, MT, NT, WANT);
  return p.scratch_bytes();
}

extern "C" int lf_wino_fused_f16x3_gemm(const void* V, const void* U2, int eU, const float* amax_in, const float* bias, float* y,
                                        float* amax_out, void* scratch, size_t scratch_bytes, int N, int D, int H, int W, int Cin,
                                        int Cout, float he, unsigned flags, float slope, void* stream) {
  lf_clear_error();
  if (V == nullptr || U2 == nullptr || y == nullptr) return LF_EINVAL;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 3) || (Cout & 3)) return LF_EINVAL;
  if ((flags & ~(LF_EPI_LRELU | LF_OUT_DEPTH_INNER)) || eU < -100 || eU > 100) return LF_EINVAL;
  if (!lf_aligned16(V) || !lf_aligned16(U2) || !lf_aligned16(y) || (bias && !lf_aligned16(bias))) return LF_EALIGN;
  const int CinP = lf_wino_f16x3_cin_padded(Cin);
  wino_ring::Plan p(3, N, D, H, W, Cout);
  p.split(64, MT, NT, WANT);
  if (const int st = p.check(CinP, scratch, scratch_bytes)) return st;
  hipStream_t s = (hipStream_t)stream;
  const int st = wino_ring::launch<wino_fused_f16x3_kernel>(p.grid(), NTHR, LDS_BYTES, s, (const _Float16*)V, (const _Float16*)U2, bias, y,
                                                            p.T, p.tz, p.ty, p.tx, D, H, W, CinP, Cout, p.CoutP, he, eU, amax_in, flags,
                                                            slope, p.partial, p.ysize, amax_out);
  if (st || p.zs == 1) return st;
  return wino_ring::finish<wino_fused_f16x3_finish_kernel>(p, s, bias, y, p.zs, Cout / 4, he, eU, amax_in, flags & LF_EPI_LRELU, slope,
                                                           amax_out);
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
  wino_ring::Plan p(2, N, 1, H, W, Cout);
  p.split(16, MT2, nt2d(p.CoutP), WANT);
  return p.scratch_bytes();
}

extern "C" int lf_wino_fused2d_f16x3_gemm(const void* V, const int* eV, const void* U2, int eU, const float* bias, float* y,
                                          void* scratch, size_t scratch_bytes, int N, int H, int W, int Cin, int Cout, float he,
                                          unsigned flags, float slope, void* stream) {
  lf_clear_error();
  if (V == nullptr || eV == nullptr || U2 == nullptr || y == nullptr) return LF_EINVAL;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin & 3) || (Cout & 3)) return LF_EINVAL;
  if ((flags & ~LF_EPI_LRELU) || eU < -100 || eU > 100) return LF_EINVAL;
  if (!lf_aligned16(V) || !lf_aligned16(U2) || !lf_aligned16(y) || (bias && !lf_aligned16(bias)) || ((uintptr_t)eV & 3)) return LF_EALIGN;
  const int CinP = lf_wino_f16x3_cin_padded(Cin);
  wino_ring::Plan p(2, N, 1, H, W, Cout);
  const int nt = nt2d(p.CoutP);
  p.split(16, MT2, nt, WANT);
  if (const int st = p.check(CinP, scratch, scratch_bytes)) return st;
  hipStream_t s = (hipStream_t)stream;
#define LF_FUSED2D(KERN_, LDS_)                                                                                                      \
  wino_ring::launch<KERN_>(p.grid(), 512, LDS_, s, (const _Float16*)V, (const _Float16*)U2, bias, y, p.T, p.ty, p.tx, H, W, CinP, Cout, \
                           p.CoutP, he, eU, eV, flags, slope, p.partial, p.ysize)
  const int st = nt == NT2 ? LF_FUSED2D(wino_fused2d_f16x3_kernel, LDS2_BYTES) : LF_FUSED2D(wino_fused2d_f16x3_c64_kernel, LDS2S_BYTES);
#undef LF_FUSED2D
  if (st || p.zs == 1) return st;
  return wino_ring::finish<wino_fused2d_f16x3_finish_kernel>(p, s, bias, y, p.zs, Cout / 4, H, W, p.ty, p.tx, ldexpf(he, -eU), eV, flags,
                                                             slope);
}
