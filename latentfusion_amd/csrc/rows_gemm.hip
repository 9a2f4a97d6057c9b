// Row-major GEMM with the Block epilogue in the store (gfx950):
//   y[m][co] = epilogue( he * sum_k x[m][k] * W[co][k] + bias[co] ),   epilogue = [LeakyReLU] ; [PixelNorm over co]
// = FactorProjection3d2d (view -> 1x1 conv -> LeakyReLU -> PixelNorm; latentfusion/modules/geometry.py:744-749,
// modules/equalized.py:57-64, modules/__init__.py:14-15) over the depth-innermost rows that LF_OUT_DEPTH_INNER makes the last
// camera block write: the ranking path's projection in ONE launch instead of a library GEMM + leaky_relu_ + lf_pixelnorm_fwd.
// All products and sums on v_mfma_f32_16x16x4_f32 (exact fp32).
//
// Work split: a 512-thread workgroup owns BM = 128 rows and ALL output channels of them (NP = 16 * NB <= 256), so the
// PixelNorm sum never leaves the workgroup and y is written once.  Wave w of 8 owns rows w*16 .. w*16+15 as NB MFMA
// blocks; two waves share a SIMD, so one wave's LDS reads and stage hand-over sit under the other's MFMAs.  All waves read
// the same weight tile.  MFMA roles are swapped w.r.t. a textbook GEMM, as in wino_fused.hip -- A = weights [16 couts][k],
// B = rows [k][16 rows] -- so a lane ends up with 4 CONSECUTIVE output channels of one row: the store is a float4 per lane,
// and a row's PixelNorm sum is the lane's own blocks plus two cross-lane adds (lane groups l >> 4), always in the same order.
// K runs in stages of KC = 32: the x (128 x 32) and W (NP x 32) chunks of stage s+1 are fetched global -> registers before
// the NB * 8 MFMAs per wave of stage s and written to the other half of a double-buffered LDS tile after them (one barrier
// per stage).  LDS: 2 * (128 + NP) * 128 B = 96 KiB at NP = 256; rows are 128 B with the eight 16-byte chunks XOR-swizzled by
// (row >> 1) & 7, which puts the 16-lane groups of a ds_read_b128 on distinct banks (the layout of wino_ring.h).  Within a
// 16-wide k-group lane group kg = lane >> 4 takes k = kg*4 + i in MFMA step i, so one ds_read_b128 feeds four MFMA steps.
// Registers at NB = 16: 64 first-level + 64 second-level accumulators (below), 68 fragment, 24 staging: 198 VGPRs, two
// waves per SIMD.
// The contraction order of an output element is a function of K alone: stages ascending, two k-groups per stage, four steps
// per group, the running sum of every 4 stages added to a second-level sum; a K tail is filled with zeros (exact).
// Rows >= M are neither read nor written (no padding asked of the caller); weight rows >= Cout of the pack are zero and take
// no part in the norm.
#include "lf_common.h"
#include <limits.h>

namespace {

constexpr int BM = 128;             // rows per workgroup
constexpr int KC = 32;              // floats of K per stage: one 128-byte LDS row
constexpr int FLUSH = 4;            // stages per first-level accumulation (128 k)
constexpr int THREADS = BM / 16 * 64;   // one 16-row MFMA block per wave
constexpr int RPS = THREADS / 8;    // rows one staging pass of the workgroup covers (8 threads per 128-byte row)

__device__ __forceinline__ int lds_off(int row, int chunk) { return row * (KC * 4) + ((chunk ^ ((row >> 1) & 7)) << 4); }

template <int NB>
__global__ void __launch_bounds__(THREADS, THREADS / 256) rows_gemm_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y,
    float* __restrict__ norm_out, long M, int K, int Cout, float he, unsigned flags, float slope, float eps) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int NP = NB * 16;                                   // weight rows of the pack
  constexpr int STAGE = (BM + NP) * KC * 4;                     // bytes of one stage: x rows, then weight rows
  constexpr int XPT = BM / RPS;                                 // 16-byte x chunks per thread and stage
  constexpr int WPT = (NP + RPS - 1) / RPS;                     // 16-byte weight chunks per thread and stage
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, kg = lane >> 4;
  const long row0 = (long)blockIdx.x * BM;
  const int c8 = t & 7, r8 = t >> 3;                            // staging: chunk of a row, row within a group of RPS
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const int S = (K + KC - 1) / KC;

  // a chunk past the operands (row >= M, weight row >= NP, k >= K; K % 4 == 0: a chunk is inside K or past it) is loaded from
  // the last row / chunk INSIDE them and replaced by zeros: no branch around a load, nothing read outside x and wpack
  f32x4 sx[XPT], sw[WPT];
  const float* xrow[XPT];
  const float* wrow[WPT];
  bool xin[XPT], win[WPT];
#pragma unroll
  for (int i = 0; i < XPT; ++i) {
    const long row = row0 + r8 + RPS * i;
    xin[i] = row < M;
    xrow[i] = x + (xin[i] ? row : M - 1) * K;
  }
#pragma unroll
  for (int i = 0; i < WPT; ++i) {
    const int co = r8 + RPS * i;
    win[i] = co < NP;
    wrow[i] = w + (long)(win[i] ? co : NP - 1) * K;
  }
  auto fetch = [&](int s) {
    const int k = s * KC + c8 * 4;
    const bool kin = k < K;
    const int kc = kin ? k : K - 4;
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
      const f32x4 v = *(const f32x4*)(xrow[i] + kc);
      sx[i] = (kin && xin[i]) ? v : zero4;
    }
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const f32x4 v = *(const f32x4*)(wrow[i] + kc);
      sw[i] = (kin && win[i]) ? v : zero4;
    }
  };
  auto stash = [&](int buf) {
    unsigned char* b = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < XPT; ++i) *(f32x4*)(b + lds_off(r8 + RPS * i, c8)) = sx[i];
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int co = r8 + RPS * i;
      if (co < NP) *(f32x4*)(b + BM * KC * 4 + lds_off(co, c8)) = sw[i];
    }
  };

  // two levels of accumulation: `acc` takes the MFMAs of FLUSH stages (128 k) and is then added to `tot` -- the rounding
  // error of a K = 4096 sum falls ~3.5x against one running sum (measured against fp64: tests/test_rows_gemm_gpu.py); the
  // schedule is a function of the stage index alone
  f32x4 acc[NB], tot[NB];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb) acc[cb] = tot[cb] = zero4;

  fetch(0);
  stash(0);
  __syncthreads();
  for (int s0 = 0; s0 < S; s0 += FLUSH) {
    const int s1 = min(s0 + FLUSH, S);
    for (int s = s0; s < s1; ++s) {
      const bool more = s + 1 < S;
      if (more) fetch(s + 1);
      const unsigned char* b = smem + (s & 1) * STAGE;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // fragments are read in the order the MFMAs take them (the row block, then weight blocks ascending): the first
        // products wait for two reads, not for all 1 + NB
        f32x4 fa[NB];
        const f32x4 fb = *(const f32x4*)(b + lds_off(wave * 16 + lr, j * 4 + kg));
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) fa[cb] = *(const f32x4*)(b + BM * KC * 4 + lds_off(cb * 16 + lr, j * 4 + kg));
#pragma unroll
        for (int cb = 0; cb < NB; ++cb)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[cb][i], fb[i], acc[cb], 0, 0, 0);
      }
      if (more) stash((s + 1) & 1);
      __syncthreads();
    }
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      tot[cb] += acc[cb];
      acc[cb] = zero4;
    }
  }

  // epilogue: lane (lr, kg) holds row wave*16 + lr, channels cb*16 + kg*4 .. +3 of every block cb
  const long row = row0 + wave * 16 + lr;
  float ss = 0.f;
#pragma unroll
  for (int cb = 0; cb < NB; ++cb) {
    const int co = cb * 16 + kg * 4;
    const bool in = co < Cout;                                  // (Cout % 4 == 0: four channels are inside or past it)
    f32x4 v = tot[cb];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = v[e] * he + ((bias != nullptr && in) ? bias[co + e] : 0.f);
      if (flags & LF_EPI_LRELU) v[e] = lf_lrelu(v[e], slope);
      if (in) ss += v[e] * v[e];
    }
    tot[cb] = v;
  }
  float r = 1.f;
  if (flags & LF_EPI_PIXELNORM) {
    ss += __shfl_xor(ss, 16, 64);
    ss += __shfl_xor(ss, 32, 64);
    r = sqrtf(ss / (float)Cout + eps);
  }
  if (row < M) {
#pragma unroll
    for (int cb = 0; cb < NB; ++cb) {
      const int co = cb * 16 + kg * 4;
      if (co < Cout) {
        f32x4 v = tot[cb];
        if (flags & LF_EPI_PIXELNORM) v = (f32x4){v[0] / r, v[1] / r, v[2] / r, v[3] / r};
        *(f32x4*)(y + row * Cout + co) = v;
      }
    }
    if ((flags & LF_EPI_PIXELNORM) && norm_out != nullptr && kg == 0) norm_out[row] = r;
  }
}

template <int NB>
int launch_rows_gemm(const float* x, const float* w, const float* bias, float* y, float* norm_out, long M, int K, int Cout,
                     float he, unsigned flags, float slope, float eps, hipStream_t stream) {
  static lf_devmask_t attr_done{0};
  constexpr int lds = 2 * (BM + NB * 16) * KC * 4;
  const hipError_t e = lf_ensure_dyn_lds(attr_done, (const void*)rows_gemm_kernel<NB>, lds);
  if (e != hipSuccess) return (int)e;
  const unsigned grid = (unsigned)((M + BM - 1) / BM);
  hipLaunchKernelGGL(rows_gemm_kernel<NB>, dim3(grid), dim3(THREADS), lds, stream, x, w, bias, y, norm_out, M, K, Cout, he, flags,
                     slope, eps);
  return lf_launch_status();
}

}  // namespace

// weight rows of the pack: 16, 32, 64, then multiples of 64 (the kernel's instantiations); 0 outside the domain
extern "C" int lf_rows_gemm_cout_padded(int Cout) {
  if (Cout < 1 || Cout > 256) return 0;
  if (Cout <= 16) return 16;
  if (Cout <= 32) return 32;
  return (Cout + 63) / 64 * 64;
}

extern "C" int lf_rows_gemm_epi(const float* x, const float* wpack, const float* bias, float* y, float* norm_out,
                                long M, int K, int Cout, float he, unsigned flags, float slope, float eps, void* stream) {
  lf_clear_error();
  if (x == nullptr || wpack == nullptr || y == nullptr) return LF_EINVAL;
  if (M < 1 || M > (long)INT_MAX * BM) return LF_EINVAL;           // 32-bit workgroup count; addresses are 64-bit
  if (K < 4 || (K & 3) != 0 || Cout < 16 || Cout > 256 || (Cout & 3) != 0) return LF_EINVAL;
  if (flags & ~(LF_EPI_LRELU | LF_EPI_PIXELNORM)) return LF_EINVAL;
  if (!lf_aligned16(x) || !lf_aligned16(wpack) || !lf_aligned16(y)) return LF_EALIGN;
  if (!(flags & LF_EPI_PIXELNORM)) norm_out = nullptr;
  hipStream_t st = (hipStream_t)stream;
  switch (lf_rows_gemm_cout_padded(Cout) / 16) {
    case 1: return launch_rows_gemm<1>(x, wpack, bias, y, norm_out, M, K, Cout, he, flags, slope, eps, st);
    case 2: return launch_rows_gemm<2>(x, wpack, bias, y, norm_out, M, K, Cout, he, flags, slope, eps, st);
    case 4: return launch_rows_gemm<4>(x, wpack, bias, y, norm_out, M, K, Cout, he, flags, slope, eps, st);
    case 8: return launch_rows_gemm<8>(x, wpack, bias, y, norm_out, M, K, Cout, he, flags, slope, eps, st);
    case 12: return launch_rows_gemm<12>(x, wpack, bias, y, norm_out, M, K, Cout, he, flags, slope, eps, st);
    case 16: return launch_rows_gemm<16>(x, wpack, bias, y, norm_out, M, K, Cout, he, flags, slope, eps, st);
  }
  return LF_EINVAL;
}
