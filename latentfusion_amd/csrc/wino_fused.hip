// Wide Winograd convolutions, stage 2 + 3 in one kernel (gfx950): the per-frequency products
//   M[f] = V[f] (tiles x Cin) . U[f] (Cin x Cout),   f = 0 .. F-1   (F = 64 for F(2x2x2,3x3x3), 16 for F(2x2,3x3))
// on the fp32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32 products and accumulation) with the OUTPUT TRANSFORM
// Y = A^T M A (x, y[, z]) folded into the frequency loop and the conv epilogue (He scale, bias, LeakyReLU) into the
// store -- the Winograd-domain products M (8x / 4x the size of the output) never exist in memory, and no library GEMM
// sits on the hot path of the released-width model (latentfusion/modules/blocks.py:152-158 at 64-512 channels,
// tools/train/train.sh:28-66; the same kernel evaluates the data gradients with transposed / flipped weight packs).
//
// Work split: a 256-thread workgroup owns 64 output channels x 64 Winograd tiles for ALL frequencies; wave (wr, wc)
// owns the 32 x 32 block (couts wr*32.., tiles wc*32..) as 2 x 2 MFMA tiles.  MFMA roles are swapped w.r.t. a textbook
// GEMM -- A = weights [16 couts][k], B = inputs [k][16 tiles] -- so a lane ends up with 4 CONSECUTIVE output channels
// of one tile and the channels-last store is a float4 per lane (64 B contiguous per 4 lanes).
// The (f, k) loop is flattened into stages of KC = 32 input channels: the A (64 x 32) and B (64 x 32) chunks of a
// stage are DMA'd global -> LDS (buffer_load_dwordx4 ... lds) into a ring of 4 stages, three stages ahead of the one
// that feeds the 32 MFMAs per wave, with ONE workgroup barrier per stage (measured: with a register-staged double
// buffer, one stage ahead, the kernel ran at ~15 % of the fp32 MFMA peak -- bound by the latency of each stage's
// loads); LDS rows are 128 B with the eight 16-byte chunks XOR-swizzled by (row >> 1) & 7, which makes the hardware's
// 16-lane ds_read_b128 groups hit distinct banks.  Within a 16-wide k-group a
// lane group kg = lane >> 4 takes k = kg*4 + i in MFMA step i (the contraction index may be permuted freely as long as
// A and B agree), so one ds_read_b128 feeds four MFMA steps.
// After the last chunk of a frequency the 2 x 2 accumulators are folded into the 2^dims output accumulators with the
// (wave-uniform) coefficients A^T[o][f] in {-1, 0, 1}.
// Everything but the product step and the epilogue -- workgroup order, staging plan and issue cursor, ring wait, operand
// tables, fold, store loop, launch plan -- is shared with the f16x3 form (wino_fused_f16x3.hip): wino_ring.inc, wino_ring.h.
#include "wino_ring.h"

namespace {

using wino_ring::KC;
using wino_ring::NSTAGE;
using wino_ring::at_coef;
using wino_ring::lds_chunk;
using wino_ring::u32;

// per-value epilogue of the direct store and of the finish kernel: He scale, bias, LeakyReLU
struct EpiF32 {
  float he, slope;
  unsigned flags;
  __device__ __forceinline__ int tile_exp(long) const { return 0; }
  __device__ __forceinline__ f32x4 operator()(const f32x4 yv, const f32x4 bv, int) const {
    f32x4 v = yv * he + bv;
    if (flags & LF_EPI_LRELU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], v[e] * slope);
    }
    return v;
  }
};

// Workgroup shape: WM x WN waves, each owning BA x BB MFMA blocks (16 couts x 16 tiles each):
//   NT = WM*BA*16 output channels (A rows) x MT = WN*BB*16 Winograd tiles (B rows) per workgroup.
// The global -> LDS bytes per MFMA fall with the block area -- 64 x 64: (64+64)*128 B per stage for 32 MFMAs per wave and
// four waves = 16 B per CU clock at the full fp32 MFMA rate, which is all the vector-memory path of a CU delivers
// (measured: 0.50 of the MFMA peak); 128 x 64: 12 B/clk; 128 x 128: 8 B/clk -- but the 2^dims output accumulators per
// block bound the blocks per wave (3-D: 36 VGPRs per block).
template <int DIMS, int WM, int WN, int BA, int BB>
__global__ void __launch_bounds__(WM * WN * 64, (WM * WN == 4 ? 2 : 1)) wino_fused_kernel(
    const float* __restrict__ V, const float* __restrict__ U2, const float* __restrict__ bias, float* __restrict__ y,
    long T, int tz, int ty, int tx, int D, int H, int W, int Cin, int Cout, int CoutP, float he, unsigned flags, float slope,
    float* __restrict__ partial, long ysize) {
#define WINO_RING_K Cin
#define WINO_RING_RAGGED 1
#define WINO_RING_SETUP
#include "wino_ring.inc"
  static_assert(PPW <= 8, "one issue slot per piece");
  for (int s = 0; s < S; ++s) {
    wino_ring::wait<PPW>(min(NSTAGE - 2, S - 1 - s));
    const bool more = issued < S;                                // wave-uniform
    const unsigned char* base = smem + (s % NSTAGE) * STAGE_BYTES;
    // product step: a stage row is 32 floats = two 16-wide k-groups; within k-group j, lane group kg takes k = kg*4 + i in MFMA
    // step i, so one ds_read_b128 feeds four v_mfma_f32_16x16x4_f32
    f32x4 fa[2][BA], fb[2][BB];                                  // [k-group j][row block]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int t = 0; t < BA; ++t) fa[j][t] = *(const f32x4*)(base + rdA[t][j]);
#pragma unroll
      for (int t = 0; t < BB; ++t) fb[j][t] = *(const f32x4*)(base + rdB[t][j]);
    }
#if defined(WF_ABL_XFORM) && WF_ABL_XFORM
    // ABLATION (tools/wino_fused_ab.py; never in the shipped library): the instruction stream of forming every B fragment
    // from the 8 raw halo records of its Winograd frequency INSIDE this kernel -- 7 more ds_read_b128
    // and 7 packed add/sub pairs per fragment -- on top of the unchanged DMA of a same-sized chunk: an upper bound on what
    // an in-kernel input transform could reach (its halo staging would cost extra on top).  Results are garbage.
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < BB; ++t)
#pragma unroll
        for (int r = 1; r < 8; ++r) {
          const f32x4 e = *(const f32x4*)(base + A_BYTES + ((rdB[t][j] - A_BYTES + r * 1040) & (MTc * 128 - 16)));
          fb[j][t] = (r & 1) ? fb[j][t] + e : fb[j][t] - e;
        }
#endif
    // the DMA pieces of stage s+3 are issued BETWEEN groups of MFMAs: an LDS-DMA instruction holds the issuing
    // (in-order) wave for ~60-180 cycles, which the matrix work already queued ahead of it covers
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int a = 0; a < BA; ++a)
#pragma unroll
          for (int b = 0; b < BB; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[j][a][i], fb[j][b][i], acc[a][b], 0, 0, 0);
        // issue slots: after every second k-step (<= 4 pieces per wave) or after every k-step (more)
        constexpr int SLOT_EVERY = PPW <= 4 ? 2 : 1;
        if ((i + 1) % SLOT_EVERY == 0) {
          const int slot_ = (j * 4 + i) / SLOT_EVERY;
          __builtin_amdgcn_sched_barrier(0);
          if (slot_ < PPW && more) issue_piece(slot_);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#define WINO_RING_FOLD
#include "wino_ring.inc"
  }
  const EpiF32 epi{he, slope, flags};
#define WINO_RING_STORE
#include "wino_ring.inc"
#undef WINO_RING_K
#undef WINO_RING_RAGGED
}

// y = epilogue(he * sum_z partial[z] + bias): fixed-order sum of the frequency-split partial outputs
__global__ void __launch_bounds__(256) wino_fused_finish_kernel(const f32x4* __restrict__ partial, const float* __restrict__ bias,
                                                               f32x4* __restrict__ y, long n4, long ysize4, int zs, int c4,
                                                               float he, unsigned flags, float slope) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const EpiF32 epi{he, slope, flags};
  y[i] = wino_ring::finish_value(partial, bias, i, ysize4, zs, c4, epi);
}

// Workgroup shapes (NT output channels x MT tiles): 0 = 64 x 64 (4 waves, two workgroups per CU), 1 = 128 x 64,
// 2 = 64 x 128, 3 = 128 x 128, 4 = 64 x 256 (8 waves, one workgroup per CU; 3 and 4 are 2-D only: the 3-D kernel keeps 8 output
// accumulators per block)
struct FusedCfg { int nt, mt, waves; };
constexpr int NCFG = 5;
constexpr FusedCfg kCfg[NCFG] = {{64, 64, 4}, {128, 64, 8}, {64, 128, 8}, {128, 128, 8}, {64, 256, 8}};
int g_fused_cfg = -1;                                             // lf_set_tuning(3, v): -1 = pick by shape

int pick_fused_cfg(int dims, long T, int CoutP) {
  if (g_fused_cfg >= 0 && g_fused_cfg < NCFG && !(dims == 3 && g_fused_cfg >= 3)) return g_fused_cfg;
  // measured per layer shape of the released model at N = 8 / 32 / 128 (tools/wide_conv_probe.py --cfgs,
  // profiles/r02_wide_conv_cfgs_*.jsonl): the large shapes pay (+10..20 % on the GEMM stage) once there are >= 1-2 k tiles
  // and >= 128 output channels; 64-channel layers and tiny maps stay on 64 x 64 with two workgroups per CU
  if (CoutP >= 128 && dims == 2 && T >= 1024) return 3;
  if (CoutP < 128 && dims == 2 && T >= 200000) return 4;        // 64-channel layers on the largest maps: 64 x 256
  if (CoutP >= 128 && dims == 3 && T >= 32768) return 1;
  if (CoutP >= 128 && dims == 3 && T >= 2048) return 2;
  return 0;
}

// workgroups wanted before a launch stops splitting over the frequencies: two (4-wave) / one (8-wave) resident per CU
long fused_want(int cfg) { return kCfg[cfg].waves == 4 ? 512 : 256; }

// The launch plan of N samples whose frequency split is the one a launch of part_n samples chooses (part_n = N: the plain
// plan).  The split decides how the F frequency contributions of an output value are grouped into partial sums, so it alone
// ties a sample's rounding to the batch it shares a launch with; the workgroup shape does not change a bit and follows the
// whole batch, as do the grid and the finish launch.
struct PartPlan {
  wino_ring::Plan p;
  int cfg;
  PartPlan(int dims, int N, int D, int H, int W, int Cout, int part_n) : p(dims, N, D, H, W, Cout) {
    cfg = pick_fused_cfg(dims, p.T, p.CoutP);
    wino_ring::Plan q(dims, part_n, D, H, W, Cout);              // what lf_wino_fused_gemm does with N = part_n
    const int qc = pick_fused_cfg(dims, q.T, q.CoutP);
    q.split(dims == 3 ? 64 : 16, kCfg[qc].mt, kCfg[qc].nt, fused_want(qc));
    p.split(dims == 3 ? 64 : 16, kCfg[cfg].mt, kCfg[cfg].nt, fused_want(cfg));
    p.zs = q.zs;
  }
};

size_t fused_scratch_bytes(int dims, int N, int D, int H, int W, int Cout, int part_n) {
  if ((dims != 2 && dims != 3) || N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cout <= 0 || part_n <= 0 || N % part_n) return 0;
  wino_ring::Plan p(dims, N, D, H, W, Cout), q(dims, part_n, D, H, W, Cout);
  int zs = 1;
  for (int c = 0; c < NCFG; ++c) {
    if (dims == 3 && c >= 3) continue;
    q.split(dims == 3 ? 64 : 16, kCfg[c].mt, kCfg[c].nt, fused_want(c));
    zs = q.zs > zs ? q.zs : zs;
  }
  p.zs = zs;
  return p.scratch_bytes();
}

int fused_gemm(const float* V, const float* U2, const float* bias, float* y, void* scratch, size_t scratch_bytes, int dims, int N,
               int D, int H, int W, int Cin, int Cout, float he, unsigned flags, float slope, int part_n, void* stream) {
  lf_clear_error();
  if ((dims != 2 && dims != 3) || N <= 0 || D <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return LF_EINVAL;
  if ((Cin & 3) || (Cout & 3) || (dims == 2 && D != 1) || (flags & ~(LF_EPI_LRELU | LF_OUT_DEPTH_INNER))) return LF_EINVAL;
  if (part_n <= 0 || N % part_n) return LF_EINVAL;
  if (!lf_aligned16(V) || !lf_aligned16(U2) || !lf_aligned16(y) || (bias && !lf_aligned16(bias))) return LF_EALIGN;
  PartPlan pp(dims, N, D, H, W, Cout, part_n);
  wino_ring::Plan& p = pp.p;
  const int cfg = pp.cfg;
  if (const int st = p.check(Cin, scratch, scratch_bytes)) return st;
  hipStream_t s = (hipStream_t)stream;
#define LF_FUSED(DIMS_, WM_, WN_, BA_, BB_)                                                                                         \
  wino_ring::launch<wino_fused_kernel<DIMS_, WM_, WN_, BA_, BB_>>(p.grid(), WM_ * WN_ * 64, NSTAGE * (WM_ * BA_ + WN_ * BB_) * 16 * 128, s, \
                                                                  V, U2, bias, y, p.T, p.tz, p.ty, p.tx, D, H, W, Cin, Cout, p.CoutP, he,   \
                                                                  flags, slope, p.partial, p.ysize)
  int st;
  if (dims == 3) st = cfg == 1 ? LF_FUSED(3, 4, 2, 2, 2) : (cfg == 2 ? LF_FUSED(3, 2, 4, 2, 2) : LF_FUSED(3, 2, 2, 2, 2));
  else st = cfg == 1 ? LF_FUSED(2, 4, 2, 2, 2) : (cfg == 2 ? LF_FUSED(2, 2, 4, 2, 2) : (cfg == 3 ? LF_FUSED(2, 4, 2, 2, 4) :
            (cfg == 4 ? LF_FUSED(2, 1, 8, 4, 2) : LF_FUSED(2, 2, 2, 2, 2))));
#undef LF_FUSED
  if (st || p.zs == 1) return st;
  return wino_ring::finish<wino_fused_finish_kernel>(p, s, bias, y, p.ysize / 4, p.zs, Cout / 4, he, flags & LF_EPI_LRELU, slope);
}

}  // namespace

extern "C" int lf_wino_fused_cout_padded(int Cout) { return (Cout + 63) / 64 * 64; }

// bytes of scratch lf_wino_fused_gemm needs for this shape (0: none).  (An upper bound over the workgroup shapes.)
extern "C" size_t lf_wino_fused_scratch_bytes(int dims, int N, int D, int H, int W, int Cout) {
  return fused_scratch_bytes(dims, N, D, H, W, Cout, N);
}

// y = epilogue(output_transform(V[f] . U2[f]^T)):  V [F][T][Cin] from lf_wino{2,3}d_input_transform;
// scratch: lf_wino_fused_scratch_bytes(...) bytes (small problems are split over the frequencies);
// U2 [F][CoutP][Cin] (output-channel major, CoutP = lf_wino_fused_cout_padded(Cout), zero padded);
// y channels-last [N][D][H][W][Cout].  flags: LF_EPI_LRELU (PixelNorm: run lf_pixelnorm_fwd on y afterwards).
extern "C" int lf_wino_fused_gemm(const float* V, const float* U2, const float* bias, float* y, void* scratch,
                                  size_t scratch_bytes, int dims, int N, int D, int H, int W, int Cin, int Cout, float he,
                                  unsigned flags, float slope, void* stream) {
  return fused_gemm(V, U2, bias, y, scratch, scratch_bytes, dims, N, D, H, W, Cin, Cout, he, flags, slope, N, stream);
}

// The same over N samples in N / part_n parts of part_n consecutive samples, with the frequency split of a launch of ONE part
// (as lf_resample3d_bwd_coef_part does for the coefficient gradient): every output value is formed by the operations, in the
// order, of lf_wino_fused_gemm called on its part alone with N = part_n -- one GEMM launch and at most one finish launch for
// the whole batch.  scratch: lf_wino_fused_scratch_bytes_part(...) bytes.  part_n = N: lf_wino_fused_gemm.
extern "C" size_t lf_wino_fused_scratch_bytes_part(int dims, int N, int D, int H, int W, int Cout, int part_n) {
  return fused_scratch_bytes(dims, N, D, H, W, Cout, part_n);
}

extern "C" int lf_wino_fused_gemm_part(const float* V, const float* U2, const float* bias, float* y, void* scratch,
                                       size_t scratch_bytes, int dims, int N, int D, int H, int W, int Cin, int Cout, float he,
                                       unsigned flags, float slope, int part_n, void* stream) {
  return fused_gemm(V, U2, bias, y, scratch, scratch_bytes, dims, N, D, H, W, Cin, Cout, he, flags, slope, part_n, stream);
}

// tuning hook for lf_set_tuning (key 3, resample.hip): workgroup shape of the fused GEMM, -1 = by shape
int lf_internal_fused_set_cfg(int v) {
  const int prev = g_fused_cfg;
  if (v >= -1 && v < NCFG) g_fused_cfg = v;
  return prev;
}
