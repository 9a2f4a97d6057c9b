// Deterministic splat for gfx950: the gradient of the trilinear gather (resample.hip) with respect to the sampled volume,
// accumulated in 64-bit fixed point so that every execution order gives the same bits.  Three forms of the same integer sums:
// global atomics, source tiles in LDS found by box culling, and source tiles in LDS fed from binned lists.
#include "resample_map.h"
#include <type_traits>

namespace {

// Sample evaluation for the deterministic splats with floating-point contraction OFF: every operation is rounded on its own,
// so the kernels that must agree with each other -- the bounding-box pass and the tile pass of the tiled form (a corner voxel
// outside its block's box would be dropped), and the tiled and the atomic form -- get the same corner indices, fractions and
// weights no matter how the surrounding code is scheduled (with contraction on, the backend fuses multiply-adds per call site).
struct SplatTap { int x0, y0, z0, x1, y1, z1; float w[8]; };     // w index = z*4 + y*2 + x

// What splat_eval and splat_eval_quad both compute, written once AS TEXT: the forms of the splat are bit-identical only while both
// round the same operations in the same order.  The pieces expand under the `#pragma clang fp contract(off)` of the function that
// uses them (the pragma is lexical: a helper function, lattice01 of resample.hip included, would be compiled with contraction on).
// lattice coordinates a, b, k in [0,1] of voxel (x, y, z): torch.linspace(0, 1, S) by ATen's symmetric formula; the only point of
// a size-1 axis counts as first half ([0]), as in lattice01 of resample.hip
#define SPLAT_LATTICE                                                                           \
  const float a = (x < max(W / 2, 1)) ? st.w * (float)x : 1.f - st.w * (float)(W - 1 - x);      \
  const float b = (y < max(H / 2, 1)) ? st.h * (float)y : 1.f - st.h * (float)(H - 1 - y);      \
  const float k = (z < max(D / 2, 1)) ? st.d * (float)z : 1.f - st.d * (float)(D - 1 - z)
// axis c of the object -> camera map (ak = a * k, bk = b * k)
#define SPLAT_O2C_ROW(c) (((((cf[c] + cf[3 + (c)] * a) + cf[6 + (c)] * b) + cf[9 + (c)] * k) + cf[12 + (c)] * ak) + cf[15 + (c)] * bk)
// row r of the camera -> object matrix on the lattice in [-1,1]
#define SPLAT_C2O_LATTICE const float lx = 2.f * a - 1.f, ly = 2.f * b - 1.f, lz = 2.f * k - 1.f
#define SPLAT_C2O_ROW(r) (((cf[4 * (r)] * lx + cf[4 * (r) + 1] * ly) + cf[4 * (r) + 2] * lz) + cf[4 * (r) + 3])
// one axis: normalised coordinate g -> fraction t and clamped corners i0, i1
#define SPLAT_AXIS(g, size, t, i0, i1)                                                                             \
  do {                                                                                                             \
    float p = (((g) + 1.f) * (float)(size) - 1.f) * 0.5f;         /* grid_sampler_unnormalize (align_corners=False) */ \
    p = fminf(fmaxf(p, 0.f), (float)((size) - 1));                /* border clip */                                \
    if (!(p == p)) p = 0.f;                                       /* NaN samples voxel 0 (ATen clip semantics) */  \
    const float f = floorf(p);                                                                                     \
    t = p - f;                                                                                                     \
    i0 = (int)f;                                                                                                   \
    i1 = min(i0 + 1, (size) - 1);                                                                                  \
  } while (0)
// the 8 corner weights from the three fractions
#define SPLAT_WEIGHTS(s, t0, t1, t2)                                                                               \
  do {                                                                                                             \
    const float wx[2] = {1.f - (t0), (t0)}, wy[2] = {1.f - (t1), (t1)}, wz[2] = {1.f - (t2), (t2)};                \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) s.w[i] = (wx[i & 1] * wy[(i >> 1) & 1]) * wz[i >> 2];            \
  } while (0)

template <int KIND>
__device__ __forceinline__ SplatTap splat_eval(const float* __restrict__ cf, int x, int y, int z, int W, int H, int D, Steps st) {
#pragma clang fp contract(off)
  SPLAT_LATTICE;
  float g[3];
  if (KIND == LF_MAP_O2C) {
    const float ak = a * k, bk = b * k;
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = SPLAT_O2C_ROW(c);
  } else {
    SPLAT_C2O_LATTICE;
    const float n0 = SPLAT_C2O_ROW(0), n1 = SPLAT_C2O_ROW(1), n2 = SPLAT_C2O_ROW(2), dn = SPLAT_C2O_ROW(3);
    g[0] = n0 / dn;
    g[1] = n1 / dn;
    g[2] = n2;
  }
  const int size[3] = {W, H, D};
  int i0[3], i1[3];
  float t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) SPLAT_AXIS(g[c], size[c], t[c], i0[c], i1[c]);
  SplatTap s;
  s.x0 = i0[0]; s.y0 = i0[1]; s.z0 = i0[2]; s.x1 = i1[0]; s.y1 = i1[1]; s.z1 = i1[2];
  SPLAT_WEIGHTS(s, t[0], t[1], t[2]);
  return s;
}

// The same evaluation shared by the four lanes of a quad that work on ONE sample (the binned tile pass: a lane quad per list entry,
// round 6): lane q < 3 evaluates axis q -- its numerator, for the projective axes the denominator and the division, the un-normalise /
// clip / floor chain -- lane 3 repeats axis 2; three quad broadcasts (v_mov_b32 dpp quad_perm) per value hand every lane all three
// axes.  Every operation an axis sees is the one splat_eval performs for it, in the same order, contraction off: the same bits, for
// about 55 % of the instructions (the evaluation was a quarter of the tile pass, profiles/r06_splat_ab.txt).
template <int CTRL>
__device__ __forceinline__ int quad_bcast_i(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ float quad_bcast_f(float v) { return __int_as_float(quad_bcast_i<CTRL>(__float_as_int(v))); }

template <int KIND>
__device__ __forceinline__ SplatTap splat_eval_quad(const float* __restrict__ cf, int x, int y, int z, int W, int H, int D, Steps st, int q) {
#pragma clang fp contract(off)
  SPLAT_LATTICE;
  const int c = q < 3 ? q : 2;                                     // this lane's axis
  float g;
  if (KIND == LF_MAP_O2C) {
    const float ak = a * k, bk = b * k;
    g = SPLAT_O2C_ROW(c);
  } else {
    SPLAT_C2O_LATTICE;
    const float num = SPLAT_C2O_ROW(c);
    const float dn = SPLAT_C2O_ROW(3);
    g = c < 2 ? num / dn : num;
  }
  const int size = c == 0 ? W : (c == 1 ? H : D);
  float tm;
  int i0m, i1m;
  SPLAT_AXIS(g, size, tm, i0m, i1m);
  SplatTap s;
  s.x0 = quad_bcast_i<0x00>(i0m); s.y0 = quad_bcast_i<0x55>(i0m); s.z0 = quad_bcast_i<0xaa>(i0m);
  s.x1 = quad_bcast_i<0x00>(i1m); s.y1 = quad_bcast_i<0x55>(i1m); s.z1 = quad_bcast_i<0xaa>(i1m);
  const float t0 = quad_bcast_f<0x00>(tm), t1 = quad_bcast_f<0x55>(tm), t2 = quad_bcast_f<0xaa>(tm);
  SPLAT_WEIGHTS(s, t0, t1, t2);
  return s;
}

// ---- deterministic splat: the same scatter, accumulated in 64-bit fixed point ----------------------------------
// Float atomics make the result depend on the order in which the hardware retires them.  Integer addition is
// associative, so accumulating round(contribution * 2^K) with 64-bit integer atomics gives bit-identical results
// for every execution order; K is chosen from max|gout| so that 2^24 contributions (every output voxel of every
// sample landing on ONE source voxel -- border clamping can do that) cannot overflow: the quantum is 2^-38 of the
// largest gradient, finer than fp32's own resolution of any sum it could be added to.
__global__ void __launch_bounds__(256) absmax_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ out) {
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f && m < 3.0e38f) atomicMax(out, __float_as_uint(m));   // max is order-independent
}

// (n a multiple of 16 and x 16-byte aligned: channels-last 16-channel records; a lane reads 8 values per load)
__global__ void __launch_bounds__(256) absmax_bf16_kernel(const __bf16* __restrict__ x, long n, unsigned* __restrict__ out) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  float m = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n / 8; i += (long)gridDim.x * 256) {
    const u32x4 r = ((const u32x4*)x)[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                  // |bf16| as fp32: the 16 bits shifted into the high half, sign cleared
      m = fmaxf(m, __uint_as_float((r[k] << 16) & 0x7fffffffu));
      m = fmaxf(m, __uint_as_float(r[k] & 0x7fff0000u));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.f && m < 3.0e38f) atomicMax(out, __float_as_uint(m));
}

__device__ __forceinline__ float fixed_scale(const unsigned* amax) {
  const float am = __uint_as_float(*amax);
  if (!(am > 0.f)) return 1.f;
  int ex;
  frexpf(am, &ex);                                               // am = m * 2^ex, m in [0.5, 1)
  // |contribution| * scale < 2^38; the exponent is capped so that tiny gradients (max|g| < 2^-88) keep a FINITE scale
  // (2^126: they then simply use fewer of the 64 bits) instead of inf * 0 = NaN
  return ldexpf(1.f, min(38 - ex, 126));
}

// round-to-nearest-even of v (|v| < 2^39) as a 64-bit integer in 3 instructions (the generic float -> int64 conversion takes ~20, half
// of the tiled kernel's arithmetic).  v is exact in fp64; adding 1.5 * 2^52 leaves a double in [2^52, 2^53) whose unit in the last
// place is 1, so the fp64 add itself rounds v to the nearest integer (ties to even, the mode of rintf) and the mantissa field then
// holds 2^51 + that integer.  Subtracting the bit pattern of the constant (its low word is zero: one 32-bit add on the high word)
// leaves the integer in two's complement.  (profiles/r06_splat_ab.txt: same checksums as the 8-instruction form it replaced.)
__device__ __forceinline__ unsigned long long fixed_round(float v) {
  const double d = (double)v + 6755399441055744.0;
  return (unsigned long long)__double_as_longlong(d) - 0x4338000000000000ull;
}

template <int KIND>
__global__ void __launch_bounds__(256) resample_bwd_vol_fixed_kernel(
    const float* __restrict__ gout, const float* __restrict__ coef, unsigned long long* __restrict__ acc,
    long acc_bstride, const unsigned* __restrict__ amax, int N, int D, int H, int W, int C, Steps st) {
  const long per_sample = (long)D * H * W * C;
  const int n = blockIdx.y;
  const float* cf = coef + (long)n * LF_MAP_COEFS;
  const float scale = fixed_scale(amax);
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < per_sample; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    long v = idx / C;
    const int x = (int)(v % W); v /= W;
    const int y = (int)(v % H);
    const int z = (int)(v / H);
    const SplatTap t = splat_eval<KIND>(cf, x, y, z, W, H, D, st);
    const float go = gout[(long)n * per_sample + idx] * scale;   // exact: power-of-two scale
    unsigned long long* base = acc + (long)n * acc_bstride + c;
    const long sW = C, sH = (long)W * C, sD = (long)H * W * C;
#define SPLAT(Z, Y, X, WI) atomicAdd(base + (Z) * sD + (Y) * sH + (X) * sW, (unsigned long long)__float2ll_rn(go * t.w[WI]))
    SPLAT(t.z0, t.y0, t.x0, 0); SPLAT(t.z0, t.y0, t.x1, 1);
    SPLAT(t.z0, t.y1, t.x0, 2); SPLAT(t.z0, t.y1, t.x1, 3);
    SPLAT(t.z1, t.y0, t.x0, 4); SPLAT(t.z1, t.y0, t.x1, 5);
    SPLAT(t.z1, t.y1, t.x0, 6); SPLAT(t.z1, t.y1, t.x1, 7);
#undef SPLAT
  }
}

__global__ void __launch_bounds__(256) fixed_to_float_kernel(const long long* __restrict__ acc, const unsigned* __restrict__ amax,
                                                            float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  out[i] = (float)((double)acc[i] * (1.0 / (double)fixed_scale(amax)));   // (the scale is a power of two: its reciprocal is exact)
}

// ---- the same sums without global atomics (C == 16): every SOURCE tile is owned by one workgroup ---------------------
// The fixed-point scatter above is bound by the L2's atomic units (2.1e9 64-bit atomics per 8 x 128^3 x 16 launch: 16-19 ms,
// a quarter of a training step).  Integer addition being associative, the same totals can be formed in any grouping:
//   pass 1  one wave per 4x4x4 block of OUTPUT voxels: bounding box of the (clamped) corner voxels its samples touch;
//   pass 2  one workgroup per 4x8x8 tile of SOURCE voxels: 64-bit accumulators for the tile in LDS (32 KB); it culls the
//           output blocks in two levels (boxes of 16^3 super-blocks, then the 64 block boxes of those that overlap; a
//           ballot per 64 boxes, every wave redundantly: no exchange, no barriers), re-evaluates the
//           samples of the blocks that touch it and adds the contributions that land inside the tile with LDS atomics;
//           border clamping needs no special case (the boxes are boxes of clamped indices); with one volume shared by all
//           samples (vol_n == 1) the workgroup walks all samples, so their contributions meet in the same accumulators;
//           finally the tile is converted and written with plain stores.
// Same quantisation, same integer totals, same conversion => bit-identical to the atomic kernel.
constexpr int STZ = 4, STY = 8, STX = 8;                          // source tile owned by a workgroup: 256 voxels
#ifndef SACC
#define SACC 17                                                   // 64-bit accumulators per voxel record (16 + padding)
#endif

// A box of clamped corner indices, 16 bits a bound: per axis lo | hi << 16.  An empty box is lo = 0x7fff > hi = 0xffff (-1 as
// signed 16 bit).
#define SPLAT_BOX_WORD(lo, hi) ((unsigned)(lo) | ((unsigned)((hi) & 0xffff) << 16))
#define SPLAT_BOX_LO(word) ((short)((word) & 0xffff))
#define SPLAT_BOX_HI(word) ((short)((word) >> 16))
// every lane's box -> the union of the wave's 64
__device__ __forceinline__ void splat_box_wave_union(int (&lo)[3], int (&hi)[3]) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = min(lo[c], __shfl_xor(lo[c], o, 64));
      hi[c] = max(hi[c], __shfl_xor(hi[c], o, 64));
    }
}

// Sections that the tile kernels below share as text (a C++ function in their place renumbers registers and moves instructions in
// all of them: tools/resample_isa_diff.py).  They use the kernels' names: tile, tid, q, t, acc, gvol, nvox, ntx, nty, D, H, W.
// origin of source tile `tile`
#define SPLAT_TILE_ORIGIN const int tx0 = (tile % ntx) * STX, ty0 = ((tile / ntx) % nty) * STY, tz0 = (tile / (ntx * nty)) * STZ
// the list kernels: a volume per sample: blockIdx.y is the sample; one volume shared by the m samples: the workgroup walks their m lists
#define SPLAT_LIST_RANGE                                                                                       \
  const int nl_first = shared ? 0 : (int)blockIdx.y, nl_last = shared ? m : (int)blockIdx.y + 1;               \
  const long n_out = shared ? 0 : n0 + (long)blockIdx.y
// the tile's voxel whose record thread tid converts and stores
#define SPLAT_TILE_VOXEL                                                                                       \
  const int lx = tid % STX, ly = (tid / STX) % STY, lz = tid / (STX * STY);                                   \
  const int x = tx0 + lx, y = ty0 + ly, z = tz0 + lz
// corner (Z, Y, X) of weight t.w[WI]: if it lands in the tile, the 4 channels of lane quad q go to its accumulators.  G: the scaled
// gradient of channel e, or the plain one where the scale goes in here; SKIP0: corners of weight zero are left out
#define SPLAT_ADD(Z, Y, X, WI, G, SKIP0)                                                                       \
  do {                                                                                                         \
    const int lz_ = (Z) - tz0, ly_ = (Y) - ty0, lx_ = (X) - tx0;                                               \
    if ((!(SKIP0) || t.w[WI] != 0.f) && (unsigned)lz_ < (unsigned)STZ && (unsigned)ly_ < (unsigned)STY && (unsigned)lx_ < (unsigned)STX) { \
      unsigned long long* d_ = acc + ((lz_ * STY + ly_) * STX + lx_) * SACC + q * 4;                           \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) atomicAdd(d_ + e, fixed_round((G) * t.w[WI]));             \
    }                                                                                                          \
  } while (0)
#define SPLAT_ADD8(G, SKIP0)                                                                                   \
  SPLAT_ADD(t.z0, t.y0, t.x0, 0, G, SKIP0); SPLAT_ADD(t.z0, t.y0, t.x1, 1, G, SKIP0);                          \
  SPLAT_ADD(t.z0, t.y1, t.x0, 2, G, SKIP0); SPLAT_ADD(t.z0, t.y1, t.x1, 3, G, SKIP0);                          \
  SPLAT_ADD(t.z1, t.y0, t.x0, 4, G, SKIP0); SPLAT_ADD(t.z1, t.y0, t.x1, 5, G, SKIP0);                          \
  SPLAT_ADD(t.z1, t.y1, t.x0, 6, G, SKIP0); SPLAT_ADD(t.z1, t.y1, t.x1, 7, G, SKIP0)
// a tile on which nothing lands: zeros, no LDS pass
#define SPLAT_STORE_ZERO(IO)                                                                                   \
  do {                                                                                                         \
    SPLAT_TILE_VOXEL;                                                                                          \
    if (x < W && y < H && z < D) {                                                                             \
      constexpr int OREC_ = ((IO) & 2) ? 32 : 64;                                                              \
      f32x4* dst = (f32x4*)((char*)gvol + (n_out * nvox + (((long)z * H + y) * W + x)) * OREC_);               \
      _Pragma("unroll") for (int k = 0; k < OREC_ / 16; ++k) dst[k] = (f32x4){0.f, 0.f, 0.f, 0.f};            \
    }                                                                                                          \
  } while (0)
// the finished tile: one thread per voxel (those with LIVE), 16 channels = 4 float4 (bf16: 4 x 8-byte) stores into the volume that
// starts VOL voxels into gvol
#define SPLAT_STORE_TILE(IO, LIVE, VOL)                                                                        \
  do {                                                                                                         \
    SPLAT_TILE_VOXEL;                                                                                          \
    if ((LIVE) && x < W && y < H && z < D) {                                                                   \
      constexpr int OREC_ = ((IO) & 2) ? 32 : 64;                                                              \
      char* dst = (char*)gvol + ((VOL) + (((long)z * H + y) * W + x)) * OREC_;                                 \
      const double inv = 1.0 / (double)scale;                     /* exact: the scale is a power of two (2^-90 .. 2^126) */ \
      _Pragma("unroll") for (int c4 = 0; c4 < 4; ++c4) {                                                       \
        f32x4 o;                                                                                               \
        _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = (float)((double)(long long)acc[tid * SACC + c4 * 4 + e] * inv); \
        if constexpr (((IO) & 2) != 0) *(bf16x4r*)(dst + c4 * 8) = __builtin_convertvector(o, bf16x4r);        \
        else *(f32x4*)(dst + c4 * 16) = o;                                                                     \
      }                                                                                                        \
    }                                                                                                          \
  } while (0)

template <int KIND>
__global__ void __launch_bounds__(256) splat_bbox_kernel(const float* __restrict__ coef, uint3* __restrict__ bbox, int nblk, int nbx,
                                                         int nby, int D, int H, int W, Steps st) {
  const int lane = threadIdx.x & 63;
  const int blk = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y;
  if (blk >= nblk) return;                                        // (wave-uniform)
  const int bx = blk % nbx, by = (blk / nbx) % nby, bz = blk / (nbx * nby);
  const int x = bx * 4 + (lane & 3), y = by * 4 + ((lane >> 2) & 3), z = bz * 4 + (lane >> 4);
  const bool live = x < W && y < H && z < D;
  const SplatTap t = splat_eval<KIND>(coef + (long)n * LF_MAP_COEFS, live ? x : 0, live ? y : 0, live ? z : 0, W, H, D, st);
  int lo[3] = {live ? t.x0 : 0x7fff, live ? t.y0 : 0x7fff, live ? t.z0 : 0x7fff};
  int hi[3] = {live ? t.x1 : -1, live ? t.y1 : -1, live ? t.z1 : -1};
  splat_box_wave_union(lo, hi);
  if (lane == 0) bbox[(long)n * nblk + blk] = make_uint3(SPLAT_BOX_WORD(lo[0], hi[0]), SPLAT_BOX_WORD(lo[1], hi[1]), SPLAT_BOX_WORD(lo[2], hi[2]));
}

// union of the boxes of the 4x4x4 blocks of a super-block (16^3 output voxels): one wave per super-block
__global__ void __launch_bounds__(256) splat_bbox2_kernel(const uint3* __restrict__ bbox, uint3* __restrict__ sbox, int nblk, int nsb,
                                                          int nbx, int nby, int nbz, int nsx, int nsy) {
  const int lane = threadIdx.x & 63;
  const int sb = blockIdx.x * 4 + (threadIdx.x >> 6), n = blockIdx.y;
  if (sb >= nsb) return;                                          // (wave-uniform)
  const int bx = (sb % nsx) * 4 + (lane & 3), by = ((sb / nsx) % nsy) * 4 + ((lane >> 2) & 3), bz = (sb / (nsx * nsy)) * 4 + (lane >> 4);
  int lo[3] = {0x7fff, 0x7fff, 0x7fff}, hi[3] = {-1, -1, -1};
  if (bx < nbx && by < nby && bz < nbz) {
    const uint3 r = bbox[(long)n * nblk + ((long)bz * nby + by) * nbx + bx];
    lo[0] = SPLAT_BOX_LO(r.x); hi[0] = SPLAT_BOX_HI(r.x);
    lo[1] = SPLAT_BOX_LO(r.y); hi[1] = SPLAT_BOX_HI(r.y);
    lo[2] = SPLAT_BOX_LO(r.z); hi[2] = SPLAT_BOX_HI(r.z);
  }
  splat_box_wave_union(lo, hi);
  if (lane == 0)                                                  // (lo came through a signed unpack: masked, unlike the first pass's)
    sbox[(long)n * nsb + sb] = make_uint3(SPLAT_BOX_WORD(lo[0] & 0xffff, hi[0]), SPLAT_BOX_WORD(lo[1] & 0xffff, hi[1]), SPLAT_BOX_WORD(lo[2] & 0xffff, hi[2]));
}

template <int KIND, int IO = 0>                                   // IO: bit 0 -- gout, bit 1 -- gvol stored as bf16 records
__global__ void __launch_bounds__(256) splat_tile_kernel(const float* __restrict__ gout, const float* __restrict__ coef,
                                                         const uint3* __restrict__ bbox, const uint3* __restrict__ sbox,
                                                         const unsigned* __restrict__ amax, float* __restrict__ gvol, int vol_n, int N,
                                                         int nblk, int nsb, int nbx, int nby, int nbz, int nsx, int nsy, int ntx, int nty,
                                                         int D, int H, int W, Steps st) {
  __shared__ unsigned long long acc[STZ * STY * STX * SACC];       // 34 KB: records padded to 17 (an 128-byte stride puts the
                                                                   // 16 voxels of an atomic instruction on two sets of banks)
  const int tid = threadIdx.x, lane = tid & 63;
  const int tile = blockIdx.x;
  SPLAT_TILE_ORIGIN;
  for (int i = tid; i < STZ * STY * STX * SACC; i += 256) acc[i] = 0ull;
  const float scale = fixed_scale(amax);
  const long nvox = (long)D * H * W;
  const int q = tid & 3, v = tid >> 2;                             // lane quad = one output voxel of the block, 4 channels each
  const int px = v & 3, py = (v >> 2) & 3, pz = v >> 4;
  const int n_first = vol_n == 1 ? 0 : blockIdx.y, n_last = vol_n == 1 ? N : blockIdx.y + 1;
  auto overlaps = [&](const uint3 r) {
    return SPLAT_BOX_LO(r.x) < tx0 + STX && SPLAT_BOX_HI(r.x) >= tx0 && SPLAT_BOX_LO(r.y) < ty0 + STY && SPLAT_BOX_HI(r.y) >= ty0 &&
           SPLAT_BOX_LO(r.z) < tz0 + STZ && SPLAT_BOX_HI(r.z) >= tz0;
  };
  __syncthreads();
  // Two-level culling, done redundantly by every wave (same data -> same masks -> same walk; no LDS exchange, no barriers:
  // the LDS atomics commute): 64 super-block boxes per test, then the 64 block boxes of a super-block that overlaps the tile.
  for (int n = n_first; n < n_last; ++n) {
    const float* cf = coef + (long)n * LF_MAP_COEFS;
    const float* gs = (const float*)((const char*)gout + (long)n * nvox * ((IO & 1) ? 32 : 64));
    const uint3* bb = bbox + (long)n * nblk;
    const uint3* sbb = sbox + (long)n * nsb;
    for (int sbase = 0; sbase < nsb; sbase += 64) {
      unsigned long long sm = __ballot(sbase + lane < nsb && overlaps(sbb[min(sbase + lane, nsb - 1)]));
      while (sm) {
        const int sbit = __builtin_ctzll(sm);
        sm &= sm - 1;
        const int sb = sbase + sbit;
        const int cbx = (sb % nsx) * 4 + (lane & 3), cby = ((sb / nsx) % nsy) * 4 + ((lane >> 2) & 3), cbz = (sb / (nsx * nsy)) * 4 + (lane >> 4);
        const bool cok = cbx < nbx && cby < nby && cbz < nbz;
        const long cid = ((long)cbz * nby + cby) * nbx + cbx;
        unsigned long long cm = __ballot(cok && overlaps(bb[cok ? cid : 0]));
        while (cm) {
          const int cbit = __builtin_ctzll(cm);
          cm &= cm - 1;
          const int bx = (sb % nsx) * 4 + (cbit & 3), by = ((sb / nsx) % nsy) * 4 + ((cbit >> 2) & 3), bz = (sb / (nsx * nsy)) * 4 + (cbit >> 4);
          const int x = bx * 4 + px, y = by * 4 + py, z = bz * 4 + pz;
          if (x < W && y < H && z < D) {
            const SplatTap t = splat_eval<KIND>(cf, x, y, z, W, H, D, st);
            f32x4 g4;
            if constexpr ((IO & 1) != 0)
              g4 = __builtin_convertvector(*(const bf16x4r*)((const char*)gs + (((long)z * H + y) * W + x) * 32 + q * 8), f32x4);
            else
              g4 = *(const f32x4*)(gs + (((long)z * H + y) * W + x) * 16 + q * 4);
            SPLAT_ADD8(g4[e] * scale, false);
          }
        }
      }
    }
  }
  __syncthreads();
  SPLAT_STORE_TILE(IO, true, vol_n == 1 ? 0 : (long)blockIdx.y * nvox);
}

// ---- binned form of the same sums (round 5: the camera -> object splat of the training step, a volume per sample, and the
// object -> camera one, all samples into one volume).  The tile form above finds the output voxels that touch a source tile by culling boxes: at 128^3 a workgroup
// walks 512 super-block boxes and then re-evaluates 40-75 blocks of 64 samples of which a tenth lands in its tile (12.4 ms for
// 32 views, the largest kernel of the step).  Here the output voxels are BINNED by the source tiles their corners touch first
// (count, scan, fill: 1.6 list entries per voxel on average, 8 at most), and a tile's workgroup evaluates exactly its list:
//   bin<FILL = false>  per output voxel: the <= 8 distinct tiles of its corner voxels, one wave-aggregated atomic add per tile
//                      and wave on the tile's counter;
//   scan               exclusive prefix of a sample's tile counters;
//   bin<FILL = true>   the same walk, now storing the voxel (z << 20 | y << 10 | x) at offset[tile] + slot;
//   binned tile        64-bit LDS accumulators as above, one LANE per list entry (all 16 channels), conversion and store as above.
// The order of a list depends on the atomics; the integer sums do not: bit-identical to the other two forms.
template <int KIND, bool FILL>
__global__ void __launch_bounds__(256) splat_bin_kernel(const float* __restrict__ coef, unsigned* __restrict__ cnt,
                                                        const unsigned* __restrict__ off, unsigned* __restrict__ list, int n0, long nvox,
                                                        long cap, int ntiles, int ntx, int nty, int D, int H, int W, Steps st) {
  const int lane = threadIdx.x & 63;
  const int nl = blockIdx.y;                                       // sample within the chunk
  // a wave takes a 4x4x4 block of output voxels: its samples land in one or two tiles per axis (a row of 64 voxels would
  // cross four to eight), so the aggregation loop below runs once or twice per corner combination
  const int nbx = (W + 3) >> 2, nby = (H + 3) >> 2, nbz = (D + 3) >> 2;
  const long blk = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool wave_live = blk < (long)nbx * nby * nbz;
  const long bq = wave_live ? blk : 0;
  const int x = (int)(bq % nbx) * 4 + (lane & 3), y = (int)((bq / nbx) % nby) * 4 + ((lane >> 2) & 3), z = (int)(bq / ((long)nbx * nby)) * 4 + (lane >> 4);
  const bool live = wave_live && x < W && y < H && z < D;
  const SplatTap t = splat_eval<KIND>(coef + (long)(n0 + nl) * LF_MAP_COEFS, min(x, W - 1), min(y, H - 1), min(z, D - 1), W, H, D, st);
  const int tx[2] = {t.x0 / STX, t.x1 / STX}, ty[2] = {t.y0 / STY, t.y1 / STY}, tz[2] = {t.z0 / STZ, t.z1 / STZ};
  unsigned* c = cnt + (long)nl * ntiles;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int kx = k & 1, ky = (k >> 1) & 1, kz = k >> 2;
    // a combination is a NEW tile iff every axis it takes the upper corner on really changes tile there
    const bool act = live && (!kx || tx[1] != tx[0]) && (!ky || ty[1] != ty[0]) && (!kz || tz[1] != tz[0]);
    const int tile = (tz[kz] * nty + ty[ky]) * ntx + tx[kx];
    unsigned long long todo = __ballot(act);
    while (todo) {                                                 // (wave-uniform loop: one atomic per distinct tile and wave)
      const int leader = __builtin_ctzll(todo);
      const int lt = __shfl(tile, leader, 64);
      const unsigned long long same = __ballot(act && tile == lt);
      unsigned base = 0;
      if (lane == leader) base = atomicAdd(c + lt, (unsigned)__builtin_popcountll(same));
      if (FILL) {
        base = __shfl(base, leader, 64);
        if (act && tile == lt) {
          const unsigned slot = base + (unsigned)__builtin_popcountll(same & ((1ull << lane) - 1ull));
          list[(long)nl * cap + off[(long)nl * ntiles + lt] + slot] = ((unsigned)z << 20) | ((unsigned)y << 10) | (unsigned)x;
        }
      }
      todo &= ~same;
    }
  }
}

// exclusive prefix sums of each sample's tile counters (one workgroup per sample)
__global__ void __launch_bounds__(256) splat_scan_kernel(const unsigned* __restrict__ cnt, unsigned* __restrict__ off, int ntiles) {
  __shared__ unsigned part[256];
  const unsigned* c = cnt + (long)blockIdx.x * ntiles;
  unsigned* o = off + (long)blockIdx.x * ntiles;
  const int per = (ntiles + 255) / 256, b = threadIdx.x * per, e = min(b + per, ntiles);
  unsigned sum = 0;
  for (int i = b; i < e; ++i) sum += c[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int i = 0; i < 256; ++i) { const unsigned p = part[i]; part[i] = run; run += p; }
  }
  __syncthreads();
  unsigned run = part[threadIdx.x];
  for (int i = b; i < e; ++i) { o[i] = run; run += c[i]; }
}

// threads per source tile: 512 = eight waves share the tile's accumulators, 32 waves per CU at four resident workgroups (LDS-bound
// residency): 2.39 -> 2.34 ms (training geometry), 2.06 -> 1.93 ms (one shared volume), 3.25 -> 3.14 ms (wide) against 256
#ifndef SBT_THREADS
#define SBT_THREADS 512
#endif
template <int KIND, int IO>
__global__ void __launch_bounds__(SBT_THREADS) splat_binned_tile_kernel(const float* __restrict__ gout, const float* __restrict__ coef,
                                                                const unsigned* __restrict__ cnt, const unsigned* __restrict__ off,
                                                                const unsigned* __restrict__ list, const unsigned* __restrict__ amax,
                                                                float* __restrict__ gvol, int n0, int m, int shared, long nvox, long cap,
                                                                int ntiles, int ntx, int nty, int D, int H, int W, Steps st) {
  __shared__ unsigned long long acc[STZ * STY * STX * SACC];
  const int tid = threadIdx.x;
  const int tile = blockIdx.x;
  SPLAT_LIST_RANGE;
  SPLAT_TILE_ORIGIN;
  unsigned total = 0;
  for (int nl = nl_first; nl < nl_last; ++nl) total |= cnt[(long)nl * ntiles + tile];
  if (total == 0) {
    if (tid >= STZ * STY * STX) return;                            // nothing lands here (more than half of the camera volume's tiles
    SPLAT_STORE_ZERO(IO);                                          // when the object fills part of it)
    return;
  }
  for (int i = tid; i < STZ * STY * STX * SACC; i += SBT_THREADS) acc[i] = 0ull;
  const float scale = fixed_scale(amax);
  __syncthreads();
  // a lane quad per list entry, four channels each (as the tile form: the lanes of one atomic instruction then spread over 16
  // records x 4 slots; one lane per entry measured 2.7x slower -- clamped samples pile up on border voxels and 64 lanes on one
  // address serialise); corners of weight zero (the far corner on an axis a sample was clamped on) add nothing and are skipped
  const int q = tid & 3;
  for (int nl = nl_first; nl < nl_last; ++nl) {
    const float* cf = coef + (long)(n0 + nl) * LF_MAP_COEFS;
    const char* gs = (const char*)gout + (long)(n0 + nl) * nvox * ((IO & 1) ? 32 : 64);
    const unsigned count = cnt[(long)nl * ntiles + tile];
    const unsigned* mine = list + (long)nl * cap + off[(long)nl * ntiles + tile];
    // two list entries ahead, one gradient record ahead (round 6): the chain list word -> record address -> record is two HBM / L2
    // latencies long and a workgroup holds only four waves; with the loads of the next entries in flight behind the arithmetic of
    // this one the pass is no longer latency-bound (tools/splat_ab.py)
    typedef typename std::conditional<(IO & 1) != 0, bf16x4r, f32x4>::type graw_t;
    auto g_of = [&](unsigned pk_) -> graw_t {
      const long v_ = ((long)(pk_ >> 20) * H + (long)((pk_ >> 10) & 1023u)) * W + (long)(pk_ & 1023u);
      return *(const graw_t*)(gs + v_ * ((IO & 1) ? 32 : 64) + q * ((IO & 1) ? 8 : 16));
    };
    const unsigned i0 = tid >> 2;
    unsigned pk1 = i0 < count ? mine[i0] : 0u, pk2 = i0 + SBT_THREADS / 4 < count ? mine[i0 + SBT_THREADS / 4] : 0u;
    graw_t gnext = g_of(pk1);
    constexpr unsigned EPI = SBT_THREADS / 4;                      // entries per iteration of the workgroup
    for (unsigned i = i0; i < count; i += EPI) {
      const unsigned pk = pk1;                                      // z << 20 | y << 10 | x
      const graw_t graw = gnext;
      pk1 = pk2;
      if (i + EPI < count) gnext = g_of(pk1);
      pk2 = i + 2 * EPI < count ? mine[i + 2 * EPI] : 0u;
      const int x = (int)(pk & 1023u), y = (int)((pk >> 10) & 1023u), z = (int)(pk >> 20);
      const SplatTap t = splat_eval_quad<KIND>(cf, x, y, z, W, H, D, st, q);   // (the quad's lanes are all live or all past the list's end)
      f32x4 g4;
      if constexpr ((IO & 1) != 0) g4 = __builtin_convertvector(graw, f32x4);
      else g4 = graw;
      g4 = g4 * scale;
      SPLAT_ADD8(g4[e], true);
    }
  }
  __syncthreads();
  SPLAT_STORE_TILE(IO, tid < STZ * STY * STX, n_out * nvox);
}

// ---- round 6 A/B (NOT the default: lf_set_tuning(4, 4)): the binned tile pass with ONE LANE PER CHANNEL (16 lanes per entry) ------
// tools/ub/lds_atomic2.hip: 64-bit LDS atomics retire at 8-9 lane-atomics per clock and CU whatever the shape of the access -- as
// long as the lanes of one instruction do not meet on an address.  The quad-per-entry form above puts 16 list entries into one
// instruction; neighbouring entries come from one 4x4x4 block of output voxels and land on the same few source voxels, clamped
// samples pile up on border records: on ONE record it falls to 2.0 per clock.  With 16 lanes per entry an instruction covers
// 4 entries x 128 contiguous bytes, which the LDS serves at 8.0 per clock even when all four are the SAME record.  To keep the
// arithmetic per entry from growing 4x with the lanes, a wave works in two phases per 64 entries: (A) lane-per-entry: list word,
// the sample's gradient record, splat_eval, in-tile test -> a table in LDS (8 weights, 8 record numbers or 0xffff, the record);
// (B) 16 lanes per entry read their entry's row (broadcast reads) and issue the 8 adds.  Same quantisation, same integer totals,
// same conversion => bit-identical to the other forms.
// MEASURED (profiles/r06_splat_ab.txt, 8 x 128^3 x 16, training geometry): 2.82 ms against 2.50 ms of the quad form before its
// loads were pipelined (2.36 after).  Ablations of THIS kernel: without the atomics -0.30 ms, without splat_eval -0.42 ms, without
// the conversion -0.07 ms of 1.9 ms: the atomics were never the bound -- the dependent loads (list word -> record) and the
// per-entry arithmetic at four waves per workgroup are; which is what the pipelined loads in the quad form address.
template <int KIND, int IO>
__global__ void __launch_bounds__(256) splat_binned_tile16_kernel(const float* __restrict__ gout, const float* __restrict__ coef,
                                                                  const unsigned* __restrict__ cnt, const unsigned* __restrict__ off,
                                                                  const unsigned* __restrict__ list, const unsigned* __restrict__ amax,
                                                                  float* __restrict__ gvol, int n0, int m, int shared, long nvox, long cap,
                                                                  int ntiles, int ntx, int nty, int D, int H, int W, Steps st) {
  constexpr bool IN16 = (IO & 1) != 0, OUT16 = (IO & 2) != 0;
  constexpr int NREC = STZ * STY * STX, GREC = IN16 ? 32 : 64;
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  __shared__ unsigned long long acc[NREC * 16];                    // 32 KB: record stride 128 B (the shape is conflict-free as it is)
  __shared__ __attribute__((aligned(16))) float tw[4][64][8];      // per wave and entry: the 8 corner weights
  __shared__ __attribute__((aligned(16))) unsigned short tr[4][64][8];   // the 8 records (0xffff: outside the tile or weight zero)
  __shared__ __attribute__((aligned(16))) unsigned char tg[4][64][GREC]; // the sample's 16-channel gradient record as stored
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, grp = lane >> 4, ch = lane & 15;
  const int tile = blockIdx.x;
  SPLAT_LIST_RANGE;
  SPLAT_TILE_ORIGIN;
  constexpr int OREC = OUT16 ? 32 : 64;
  unsigned total = 0;
  for (int nl = nl_first; nl < nl_last; ++nl) total |= cnt[(long)nl * ntiles + tile];
  if (total == 0) {
    SPLAT_STORE_ZERO(IO);
    return;
  }
  for (int i = tid; i < NREC * 16; i += 256) acc[i] = 0ull;
  const float scale = fixed_scale(amax);
  __syncthreads();
  for (int nl = nl_first; nl < nl_last; ++nl) {
    const float* cf = coef + (long)(n0 + nl) * LF_MAP_COEFS;
    const char* gs = (const char*)gout + (long)(n0 + nl) * nvox * GREC;
    const unsigned count = cnt[(long)nl * ntiles + tile];
    const unsigned* mine = list + (long)nl * cap + off[(long)nl * ntiles + tile];
    for (unsigned b0 = (unsigned)wv * 64u; b0 < count; b0 += 256u) {
      // ---- phase A: lane = list entry
      if (b0 + lane < count) {
        const unsigned pk = mine[b0 + lane];                        // z << 20 | y << 10 | x
        const int x = (int)(pk & 1023u), y = (int)((pk >> 10) & 1023u), z = (int)(pk >> 20);
        const u32x4* src = (const u32x4*)(gs + (((long)z * H + y) * W + x) * GREC);
        u32x4 rec[GREC / 16];
#pragma unroll
        for (int k = 0; k < GREC / 16; ++k) rec[k] = src[k];
        const SplatTap t = splat_eval<KIND>(cf, x, y, z, W, H, D, st);
        const int lz[2] = {t.z0 - tz0, t.z1 - tz0}, ly[2] = {t.y0 - ty0, t.y1 - ty0}, lx[2] = {t.x0 - tx0, t.x1 - tx0};
        unsigned r16[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int cz = lz[c >> 2], cy = ly[(c >> 1) & 1], cx = lx[c & 1];
          const bool in = t.w[c] != 0.f && (unsigned)cz < (unsigned)STZ && (unsigned)cy < (unsigned)STY && (unsigned)cx < (unsigned)STX;
          r16[c] = in ? (unsigned)((cz * STY + cy) * STX + cx) : 0xffffu;
        }
        *(f32x4*)&tw[wv][lane][0] = (f32x4){t.w[0], t.w[1], t.w[2], t.w[3]};
        *(f32x4*)&tw[wv][lane][4] = (f32x4){t.w[4], t.w[5], t.w[6], t.w[7]};
        *(u32x4*)&tr[wv][lane][0] = (u32x4){r16[0] | (r16[1] << 16), r16[2] | (r16[3] << 16), r16[4] | (r16[5] << 16), r16[6] | (r16[7] << 16)};
#pragma unroll
        for (int k = 0; k < GREC / 16; ++k) *(u32x4*)&tg[wv][lane][k * 16] = rec[k];
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // ---- phase B: 16 lanes = the channels of one entry, four entries per instruction
      const int nb = (int)min(64u, count - b0);
#pragma unroll 4
      for (int j = 0; j < 16; ++j) {
        const int e = j * 4 + grp;
        if (e < nb) {
          const f32x4 w0 = *(const f32x4*)&tw[wv][e][0], w1 = *(const f32x4*)&tw[wv][e][4];
          const u32x4 r4 = *(const u32x4*)&tr[wv][e][0];
          float g;
          if constexpr (IN16) g = __uint_as_float((unsigned)(*(const unsigned short*)&tg[wv][e][ch * 2]) << 16);
          else g = *(const float*)&tg[wv][e][ch * 4];
          g = g * scale;
          const float w8[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const unsigned r = (r4[c >> 1] >> (16 * (c & 1))) & 0xffffu;
            if (r != 0xffffu) atomicAdd(acc + r * 16 + ch, fixed_round(g * w8[c]));
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();                             // (the table is rewritten by the next batch)
    }
  }
  __syncthreads();
  // conversion and store, 16 lanes per record (a record's 128 bytes in one access; four x-neighbours per instruction)
  const double inv = 1.0 / (double)scale;                       // exact: the scale is a power of two (2^-90 .. 2^126)
#pragma unroll 4
  for (int j = 0; j < 16; ++j) {
    const int r = wv * 64 + j * 4 + grp;
    const int lx = r % STX, ly = (r / STX) % STY, lz = r / (STX * STY);
    const int x = tx0 + lx, y = ty0 + ly, z = tz0 + lz;
    if (x < W && y < H && z < D) {
      char* dst = (char*)gvol + (n_out * nvox + (((long)z * H + y) * W + x)) * OREC;
      const float o = (float)((double)(long long)acc[r * 16 + ch] * inv);
      if constexpr (OUT16) ((__bf16*)dst)[ch] = __builtin_convertvector((f32x4){o, o, o, o}, bf16x4r)[0];
      else ((float*)dst)[ch] = o;
    }
  }
}

// samples per pass of the binned form: the lists are sized for the worst case (8 entries per voxel), 512 MB at most
int g_splat_chunk_cap = 0;                                        // lf_set_tuning key 6: samples per pass at most (0 = by memory only)
int splat_bin_chunk(int N, long nvox) {
  long cv = (512L << 20) / (nvox * 32);
  if (cv < 1) cv = 1;
  if (g_splat_chunk_cap > 0 && cv > g_splat_chunk_cap) cv = g_splat_chunk_cap;
  return (int)(cv < N ? cv : N);
}

int g_splat_variant = 2;      // deterministic splat (lf_set_tuning key 4): 1 = global 64-bit atomics, 2 = source tiles in LDS (C == 16;
                              // lf_resample3d_bwd_vol_det_io: binned lists, a lane quad per list entry), 3 = as 2 without the binned form,
                              // 4 = as 2 with 16 lanes per list entry (round-6 A/B: slower)

bool splat_binned_ok(int vol_n, int N, int D, int H, int W) {
  if (g_splat_variant == 3 || W > 1024 || H > 1024 || D > 4096) return false;
  // a volume per sample: passes of `chunk` samples; one shared volume: its tile accumulators live for ONE pass, all samples in it
  return vol_n == N || splat_bin_chunk(N, (long)D * H * W) == N;
}

// the <KIND, IO> instance of a kernel template for `kind` and `io` (0..3)
#define SPLAT_IO4(KERNEL, KIND) KERNEL<KIND, 0>, KERNEL<KIND, 1>, KERNEL<KIND, 2>, KERNEL<KIND, 3>
#define SPLAT_BY_KIND_IO(KERNEL)                                                                                                  \
  ([&] {                                                                                                                          \
    static constexpr decltype(&KERNEL<LF_MAP_O2C, 0>) t[2][4] = {{SPLAT_IO4(KERNEL, LF_MAP_O2C)}, {SPLAT_IO4(KERNEL, LF_MAP_C2O)}}; \
    return t[kind == LF_MAP_O2C ? 0 : 1][io];                                                                                     \
  }())
// the two passes of splat_bin_kernel as templates of KIND alone, for LAUNCH_BY_KIND
template <int KIND> constexpr auto splat_bin_count = &splat_bin_kernel<KIND, false>;
template <int KIND> constexpr auto splat_bin_fill = &splat_bin_kernel<KIND, true>;

void launch_absmax(const void* gout, long ng, bool bf16, unsigned* amax, hipStream_t s) {
  const dim3 grid((unsigned)min((ng + 255) / 256, 4096L));
  if (bf16) hipLaunchKernelGGL(absmax_bf16_kernel, grid, dim3(256), 0, s, (const __bf16*)gout, ng, amax);
  else hipLaunchKernelGGL(absmax_kernel, grid, dim3(256), 0, s, (const float*)gout, ng, amax);
}

// Shape rules and scratch of the tile form, shared by both entry points and the scratch query of the second.
// scratch = [amax (256 B)] [block boxes: N x blocks x 12 B] [super-block boxes: N x super-blocks x 12 B]
struct SplatTilePlan {
  int nbx, nby, nbz, nsx, nsy, ntx, nty;                           // 4^3 output blocks, 16^3 super-blocks, source tiles along the axes
  long nblk, nsb, ntiles;                                          // ... and per sample
  size_t bytes;                                                    // scratch the form needs
  bool in_range;
  bool fits(size_t scratch_bytes) const { return in_range && scratch_bytes >= bytes; }
};
SplatTilePlan splat_tile_plan(int N, int D, int H, int W) {
  SplatTilePlan p;
  p.nbx = (W + 3) / 4; p.nby = (H + 3) / 4; p.nbz = (D + 3) / 4;
  p.nblk = (long)p.nbx * p.nby * p.nbz;
  p.nsx = (p.nbx + 3) / 4; p.nsy = (p.nby + 3) / 4;
  p.nsb = (long)p.nsx * p.nsy * ((p.nbz + 3) / 4);
  p.ntx = (W + STX - 1) / STX; p.nty = (H + STY - 1) / STY;
  p.ntiles = (long)p.ntx * p.nty * ((D + STZ - 1) / STZ);
  p.bytes = 256 + (size_t)N * (size_t)(p.nblk + p.nsb) * sizeof(uint3);
  p.in_range = D < 0x7fff && H < 0x7fff && W < 0x7fff && p.nblk < 0x7fffffffL / 4 && p.ntiles < 0x7fffffffL && N <= 65535;
  return p;
}

// absmax, block boxes, super-block boxes, tile pass (the caller has checked p.fits)
int splat_tile_launch(const SplatTilePlan& p, const void* gout, int io, const float* coef, int kind, void* gvol, int vol_n, void* scratch,
                      int N, int D, int H, int W, hipStream_t s) {
  unsigned* amax = (unsigned*)scratch;
  uint3* bbox = (uint3*)((char*)scratch + 256);
  uint3* sbox = bbox + (size_t)N * p.nblk;
  hipError_t e = hipMemsetAsync(scratch, 0, 256, s);
  if (e != hipSuccess) return (int)e;
  launch_absmax(gout, (long)D * H * W * 16 * N, (io & 1) != 0, amax, s);
  const Steps stp = make_steps(D, H, W);
  const int nblk = (int)p.nblk, nsb = (int)p.nsb;
  LAUNCH_BY_KIND(splat_bbox_kernel, dim3((unsigned)((nblk + 3) / 4), (unsigned)N), coef, bbox, nblk, p.nbx, p.nby, D, H, W, stp);
  hipLaunchKernelGGL(splat_bbox2_kernel, dim3((unsigned)((nsb + 3) / 4), (unsigned)N), dim3(256), 0, s, bbox, sbox, nblk, nsb, p.nbx, p.nby,
                     p.nbz, p.nsx, p.nsy);
  hipLaunchKernelGGL(SPLAT_BY_KIND_IO(splat_tile_kernel), dim3((unsigned)p.ntiles, (unsigned)vol_n), dim3(256), 0, s, (const float*)gout, coef,
                     bbox, sbox, amax, (float*)gvol, vol_n, N, nblk, nsb, p.nbx, p.nby, p.nbz, p.nsx, p.nsy, p.ntx, p.nty, D, H, W, stp);
  return lf_launch_status();
}

}  // namespace

int lf_internal_splat_set_variant(int v) {
  const int prev = g_splat_variant;
  if (v >= 1 && v <= 4) g_splat_variant = v;
  return prev;
}

int lf_internal_splat_set_chunk_cap(int v) {
  const int prev = g_splat_chunk_cap;
  if (v >= 0) g_splat_chunk_cap = v;
  return prev;
}

// Deterministic form of lf_resample3d_bwd_vol (no float atomics): see resample_bwd_vol_fixed_kernel.  gvol is
// overwritten (no zero-initialisation needed).  scratch: lf_resample3d_bwd_vol_det_scratch_bytes(...) bytes.
extern "C" size_t lf_resample3d_bwd_vol_det_scratch_bytes(int vol_n, int D, int H, int W, int C) {
  if (vol_n <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return (size_t)vol_n * D * H * W * C * sizeof(long long) + 256;
}

extern "C" int lf_resample3d_bwd_vol_det(const float* gout, const float* coef, int kind, float* gvol, int vol_n, void* scratch,
                                         size_t scratch_bytes, int N, int D, int H, int W, int C, void* stream) {
  lf_clear_error();
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return LF_EINVAL;
  if ((vol_n != 1 && vol_n != N) || (kind != LF_MAP_O2C && kind != LF_MAP_C2O)) return LF_EINVAL;
  const long items = (long)D * H * W * C, total = items * vol_n;
  if (scratch == nullptr || scratch_bytes < lf_resample3d_bwd_vol_det_scratch_bytes(vol_n, D, H, W, C)) return LF_ENOSPC;
  if ((((uintptr_t)scratch) & 7u) != 0) return LF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  if (g_splat_variant >= 2 && C == 16 && lf_aligned16(gout) && lf_aligned16(gvol)) {
    const SplatTilePlan p = splat_tile_plan(N, D, H, W);
    if (p.fits(scratch_bytes)) return splat_tile_launch(p, gout, 0, coef, kind, gvol, vol_n, scratch, N, D, H, W, s);
  }
  // global-atomic form: scratch = [accumulators: total x 8 B] [amax (256 B)]
  unsigned long long* acc = (unsigned long long*)scratch;
  unsigned* amax = (unsigned*)((char*)scratch + (size_t)total * sizeof(long long));
  hipError_t e = hipMemsetAsync(scratch, 0, (size_t)total * sizeof(long long) + 256, s);
  if (e != hipSuccess) return (int)e;
  launch_absmax(gout, items * N, false, amax, s);
  int st = lf_launch_status();
  if (st) return st;
  const long bstride = vol_n == 1 ? 0 : items;
  const dim3 grid((unsigned)min((items + 255) / 256, (long)65535 * 16), N);
  LAUNCH_BY_KIND(resample_bwd_vol_fixed_kernel, grid, gout, coef, acc, bstride, amax, N, D, H, W, C, make_steps(D, H, W));
  st = lf_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(fixed_to_float_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const long long*)acc, amax, gvol, total);
  return lf_launch_status();
}

// ---- storage-type variant for the training step's bf16 storage policy (16-channel volumes only) ----
// scratch: the tile form: SplatTilePlan::bytes (a few MB); the binned form: [amax (256 B)] [counters | cursors | offsets:
// 3 x chunk x tiles u32] [lists: chunk x voxels x 8 u32], chunk = samples per pass (lists of at most 512 MB)
extern "C" size_t lf_resample3d_bwd_vol_det_io_scratch_bytes(int vol_n, int N, int D, int H, int W) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  const SplatTilePlan p = splat_tile_plan(N, D, H, W);
  const long nvox = (long)D * H * W;
  const long cv = splat_bin_chunk(N, nvox);
  const size_t lists = 256 + (size_t)(3 * cv * p.ntiles * 4) + (size_t)(cv * nvox * 32);
  // (sized for either form: lf_set_tuning may switch between them after the caller asked)
  return p.bytes > lists ? p.bytes : lists;
}

extern "C" int lf_resample3d_bwd_vol_det_io(const void* gout, const float* coef, int kind, void* gvol, int vol_n, void* scratch,
                                            size_t scratch_bytes, int N, int D, int H, int W, int io, void* stream) {
  lf_clear_error();
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || io < 0 || io > 3) return LF_EINVAL;
  if ((vol_n != 1 && vol_n != N) || (kind != LF_MAP_O2C && kind != LF_MAP_C2O)) return LF_EINVAL;
  if (scratch == nullptr || scratch_bytes < lf_resample3d_bwd_vol_det_io_scratch_bytes(vol_n, N, D, H, W)) return LF_ENOSPC;
  if ((((uintptr_t)scratch) & 7u) != 0 || !lf_aligned16(gout) || !lf_aligned16(gvol)) return LF_EALIGN;
  hipStream_t s = (hipStream_t)stream;
  const SplatTilePlan p = splat_tile_plan(N, D, H, W);
  if (!splat_binned_ok(vol_n, N, D, H, W)) {
    if (!p.fits(scratch_bytes)) return LF_EINVAL;
    return splat_tile_launch(p, gout, io, coef, kind, gvol, vol_n, scratch, N, D, H, W, s);
  }
  // binned form (list entries pack z | y | x into 12 + 10 + 10 bits)
  const long nvox = (long)D * H * W, nt = p.ntiles;
  if (nvox >= 0xffffffffL || nt >= 0x7fffffffL || N > 65535) return LF_EINVAL;
  const int cv = splat_bin_chunk(N, nvox);
  const long cap = nvox * 8;
  unsigned* amax = (unsigned*)scratch;
  unsigned* cnt = (unsigned*)((char*)scratch + 256);
  unsigned* cur = cnt + (size_t)cv * nt;
  unsigned* off = cur + (size_t)cv * nt;
  unsigned* list = off + (size_t)cv * nt;
  hipError_t e = hipMemsetAsync(scratch, 0, 256, s);
  if (e != hipSuccess) return (int)e;
  launch_absmax(gout, nvox * 16 * N, (io & 1) != 0, amax, s);
  const Steps stp = make_steps(D, H, W);
  const bool lanes16 = g_splat_variant == 4;
  const auto tile_kernel = lanes16 ? SPLAT_BY_KIND_IO(splat_binned_tile16_kernel) : SPLAT_BY_KIND_IO(splat_binned_tile_kernel);
  for (int n0 = 0; n0 < N; n0 += cv) {
    const int m = min(cv, N - n0);
    e = hipMemsetAsync(cnt, 0, (size_t)2 * cv * nt * 4, s);
    if (e != hipSuccess) return (int)e;
    const dim3 gbin((unsigned)((p.nblk + 3) / 4), (unsigned)m);
    LAUNCH_BY_KIND(splat_bin_count, gbin, coef, cnt, off, list, n0, nvox, cap, (int)nt, p.ntx, p.nty, D, H, W, stp);
    hipLaunchKernelGGL(splat_scan_kernel, dim3((unsigned)m), dim3(256), 0, s, cnt, off, (int)nt);
    LAUNCH_BY_KIND(splat_bin_fill, gbin, coef, cur, off, list, n0, nvox, cap, (int)nt, p.ntx, p.nty, D, H, W, stp);
    const int shared = vol_n == 1 && N > 1;
    hipLaunchKernelGGL(tile_kernel, dim3((unsigned)nt, (unsigned)(shared ? 1 : m)), dim3(lanes16 ? 256 : SBT_THREADS), 0, s, (const float*)gout,
                       coef, cnt, off, list, amax, (float*)gvol, n0, m, shared, nvox, cap, (int)nt, p.ntx, p.nty, D, H, W, stp);
  }
  return lf_launch_status();
}
