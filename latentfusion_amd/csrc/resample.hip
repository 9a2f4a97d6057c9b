// Camera <-> object voxel resampling for gfx950 (trilinear gather / coefficient-gradient
// reduction / float-atomic splat; the deterministic splat is splat.hip).  Replaces F.grid_sample(…, padding_mode='border', align_corners=False) of
//   ObjectToCameraTransform.forward  latentfusion/modules/geometry.py:669-690
//   CameraToObjectTransform.forward  latentfusion/modules/geometry.py:625-657
// The sampling grid is evaluated per voxel from a per-sample coefficient block (see lf_hip.h);
// volumes are channels-last so that every trilinear tap is one contiguous C-float record.
#include "resample_map.h"

namespace {

typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

struct Tap {
  int x0, y0, z0, x1, y1, z1;   // clamped integer corners
  float tx, ty, tz;             // fractional offsets
  float mx, my, mz;             // d(ix)/d(gx) incl. border-clip mask (0 outside the volume)
};

// i-th point of torch.linspace(0, 1, size): start + step*i in the first half, end - step*(size-1-i) in the
// second (ATen's symmetric formula), step = 1/(size-1) computed once on the host.  linspace(0, 1, 1) is [0]: the only point of
// a size-1 axis counts as first half (max(size / 2, 1) is size / 2 for every other size; one scalar instruction)
__device__ __forceinline__ float lattice01(int i, int size, float step) {
  return (i < max(size / 2, 1)) ? step * (float)i : 1.f - step * (float)(size - 1 - i);
}


template <int KIND>
__device__ __forceinline__ void eval_grid(const float* __restrict__ cf, int x, int y, int z,
                                          int W, int H, int D, Steps st, float& gx, float& gy, float& gz,
                                          float& a, float& b, float& k) {
  // lattice coordinates in [0,1] (torch.linspace(0,1,S): geometry.py:476-480)
  a = lattice01(x, W, st.w);
  b = lattice01(y, H, st.h);
  k = lattice01(z, D, st.d);
  if (KIND == LF_MAP_O2C) {
    const float ak = a * k, bk = b * k;
    gx = cf[0] + cf[3] * a + cf[6] * b + cf[9] * k + cf[12] * ak + cf[15] * bk;
    gy = cf[1] + cf[4] * a + cf[7] * b + cf[10] * k + cf[13] * ak + cf[16] * bk;
    gz = cf[2] + cf[5] * a + cf[8] * b + cf[11] * k + cf[14] * ak + cf[17] * bk;
  } else {
    // lattice in [-1,1] (torch.linspace(-c/2,c/2,S) / (c/2): geometry.py:599-611)
    const float lx = 2.f * a - 1.f, ly = 2.f * b - 1.f, lz = 2.f * k - 1.f;
    const float n0 = cf[0] * lx + cf[1] * ly + cf[2] * lz + cf[3];
    const float n1 = cf[4] * lx + cf[5] * ly + cf[6] * lz + cf[7];
    const float n2 = cf[8] * lx + cf[9] * ly + cf[10] * lz + cf[11];
    const float dn = cf[12] * lx + cf[13] * ly + cf[14] * lz + cf[15];
    gx = n0 / dn;
    gy = n1 / dn;
    gz = n2;
  }
}

__device__ __forceinline__ void unnormalize_clip(float g, int size, float& pos, float& mult) {
  // grid_sampler_unnormalize (align_corners=False) + clip_coordinates_set_grad (border)
  float p = ((g + 1.f) * (float)size - 1.f) * 0.5f;
  const float hi = (float)(size - 1);
  mult = (p > 0.f && p < hi) ? 0.5f * (float)size : 0.f;
  p = fminf(fmaxf(p, 0.f), hi);
  pos = p;
}

__device__ __forceinline__ Tap make_tap(float gx, float gy, float gz, int W, int H, int D) {
  Tap t;
  float px, py, pz;
  unnormalize_clip(gx, W, px, t.mx);
  unnormalize_clip(gy, H, py, t.my);
  unnormalize_clip(gz, D, pz, t.mz);
  // NaN coordinates (degenerate cameras) sample voxel 0, like ATen's clip of NaN
  if (!(px == px)) px = 0.f;
  if (!(py == py)) py = 0.f;
  if (!(pz == pz)) pz = 0.f;
  const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
  t.tx = px - fx; t.ty = py - fy; t.tz = pz - fz;
  t.x0 = (int)fx; t.y0 = (int)fy; t.z0 = (int)fz;
  t.x1 = min(t.x0 + 1, W - 1); t.y1 = min(t.y0 + 1, H - 1); t.z1 = min(t.z0 + 1, D - 1);
  return t;
}

// Workgroups are dispatched round-robin over the 8 XCDs (one L2 each): flat workgroup id b runs on XCD b % 8.
// Giving XCD k the k-th contiguous eighth of the work list keeps neighbouring tiles -- whose gather footprints
// overlap -- behind one L2 instead of eight.  (Measured neutral for these kernels: the gathered volume lives in the
// 256 MB Infinity Cache either way; kept for the coefficient gradient, whose blocks are large.)
__device__ __forceinline__ unsigned xcd_contiguous(unsigned b, unsigned nb) {
  return (nb % 8 == 0) ? (b % 8) * (nb / 8) + b / 8 : b;
}

// ---- backward w.r.t. the O2C coefficient block ------------------------------------------------
// stage 1 (the resample_bwd_coef* kernels of resample_gather.inc): every block reduces a contiguous run of voxels of one sample to 18 partial sums.
// voxels per block: 4096 for big volumes, down to 64 so that small ones (16^3 x 256 channels) still
// launch a few hundred blocks.  A pure function of the shapes -> the reduction order is reproducible.
static int bwd_vox_per_block(long nvox, int N) {
  long v = nvox * N / 2048;
  int p = 64;
  while (p < 4096 && p * 2 <= v) p <<= 1;
  return p;
}
// the block's voxels form a compact tile of 2^bx x 2^by x 2^bz voxels (4096 -> 16^3 ... 64 -> 4^3) walked in
// 4x4x4 sub-tiles, so the 8-corner footprints overlap in L1 / L2 instead of spanning a whole plane
struct BwdTile { int lx, ly, lz, ntx, nty, ntz; };
static BwdTile bwd_tile(int vpb, int D, int H, int W) {
  int lg = 0;
  while ((1 << lg) < vpb) ++lg;                               // vpb = 2^lg, 6 <= lg <= 12
  BwdTile t;
  t.lx = (lg + 2) / 3; t.ly = (lg + 1) / 3; t.lz = lg / 3;
  t.ntx = (W + (1 << t.lx) - 1) >> t.lx; t.nty = (H + (1 << t.ly) - 1) >> t.ly; t.ntz = (D + (1 << t.lz) - 1) >> t.lz;
  return t;
}

// stage 2: fixed-order fp64 reduction of the per-block partials -> gcoef[n][18]
__global__ void __launch_bounds__(256) resample_bwd_coef_reduce(const float* __restrict__ partial,
                                                                int nblk, float* __restrict__ gcoef) {
  const int n = blockIdx.x;
  __shared__ double red[256];
  const int comp = threadIdx.x % 18;        // threads 0..251 -> 14 strided groups of 18
  const int grp = threadIdx.x / 18;
  double s = 0.0;
  if (grp < 14)
    for (int b = grp; b < nblk; b += 14) s += (double)partial[((long)n * nblk + b) * 18 + comp];
  red[threadIdx.x] = (grp < 14) ? s : 0.0;
  __syncthreads();
  if (threadIdx.x < 18) {
    double tot = 0.0;
    for (int g = 0; g < 14; ++g) tot += red[g * 18 + threadIdx.x];
    gcoef[(long)n * 18 + threadIdx.x] = (float)tot;
  }
}

// ---- backward w.r.t. the sampled volume (splat) -----------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(256) resample_bwd_vol_kernel(
    const float* __restrict__ gout, const float* __restrict__ coef, float* __restrict__ gvol,
    long gvol_bstride, int N, int D, int H, int W, int C, Steps st) {
  const long per_sample = (long)D * H * W * C;
  const int n = blockIdx.y;
  const float* cf = coef + (long)n * LF_MAP_COEFS;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < per_sample;
       idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    long v = idx / C;
    const int x = (int)(v % W); v /= W;
    const int y = (int)(v % H);
    const int z = (int)(v / H);
    float gx, gy, gz, a, b, k;
    eval_grid<KIND>(cf, x, y, z, W, H, D, st, gx, gy, gz, a, b, k);
    const Tap t = make_tap(gx, gy, gz, W, H, D);
    const float go = gout[(long)n * per_sample + idx];
    float* base = gvol + (long)n * gvol_bstride + c;
    const long sW = C, sH = (long)W * C, sD = (long)H * W * C;
    const float wx1 = t.tx, wx0 = 1.f - t.tx, wy1 = t.ty, wy0 = 1.f - t.ty, wz1 = t.tz, wz0 = 1.f - t.tz;
    atomicAdd(base + t.z0 * sD + t.y0 * sH + t.x0 * sW, go * (wx0 * wy0 * wz0));
    atomicAdd(base + t.z0 * sD + t.y0 * sH + t.x1 * sW, go * (wx1 * wy0 * wz0));
    atomicAdd(base + t.z0 * sD + t.y1 * sH + t.x0 * sW, go * (wx0 * wy1 * wz0));
    atomicAdd(base + t.z0 * sD + t.y1 * sH + t.x1 * sW, go * (wx1 * wy1 * wz0));
    atomicAdd(base + t.z1 * sD + t.y0 * sH + t.x0 * sW, go * (wx0 * wy0 * wz1));
    atomicAdd(base + t.z1 * sD + t.y0 * sH + t.x1 * sW, go * (wx1 * wy0 * wz1));
    atomicAdd(base + t.z1 * sD + t.y1 * sH + t.x0 * sW, go * (wx0 * wy1 * wz1));
    atomicAdd(base + t.z1 * sD + t.y1 * sH + t.x1 * sW, go * (wx1 * wy1 * wz1));
  }
}

// ================================================================================================================
// Helpers of the lean variants (default; the kernels are in resample_gather.inc): the same arithmetic for the sampling position, but
//   * every address is a 32-bit byte offset into a buffer resource of ONE sample (scalar base + vector offset; the
//     generic kernels spend a third of their VALU on 64-bit multiply-adds per tap) -- needs D*H*W*C*4 < 2^32;
//   * the second corner along an axis is the first + a conditional stride (no second multiply);
//   * the coefficient gradient first contracts the 4 channels of a lane with the gradient for each of the 8 corners
//     (32 FMAs), sums those 8 scalars over the voxel's lanes with DPP row shuffles, and only then forms the three
//     spatial derivatives -- instead of 3 x 4 difference-products per channel (144 ops);
//   * the tile walk of the gradient kernel is wave-uniform (scalar unit) except for a per-thread constant.
// Both are bound by the vector-memory path (8 x 64-byte gathers per output voxel through L1) once the VALU is lean.
typedef unsigned u32;

struct Tap32 {
  u32 o000, o001, o010, o011, o100, o101, o110, o111;          // byte offsets of the 8 corners (record start)
  float tx, ty, tz, mx, my, mz;
};

__device__ __forceinline__ void axis_tap(float g, int size, u32 stride, u32& o0, u32& d1, float& t, float& m) {
  float p;
  unnormalize_clip(g, size, p, m);
  if (!(p == p)) p = 0.f;                                        // NaN samples voxel 0 (ATen clip semantics)
  const float f = floorf(p);
  t = p - f;
  const int i0 = (int)f;
  o0 = (u32)i0 * stride;
  d1 = (i0 + 1 <= size - 1) ? stride : 0u;                       // clamped upper corner = same record
}

__device__ __forceinline__ Tap32 make_tap32(float gx, float gy, float gz, int W, int H, int D, u32 rec_bytes) {
  Tap32 t;
  u32 x0, dx, y0, dy, z0, dz;
  axis_tap(gx, W, rec_bytes, x0, dx, t.tx, t.mx);
  axis_tap(gy, H, rec_bytes * (u32)W, y0, dy, t.ty, t.my);
  axis_tap(gz, D, rec_bytes * (u32)W * (u32)H, z0, dz, t.tz, t.mz);
  const u32 b00 = z0 + y0, b01 = b00 + dy, b10 = b00 + dz, b11 = b01 + dz;
  t.o000 = b00 + x0; t.o001 = t.o000 + dx;
  t.o010 = b01 + x0; t.o011 = t.o010 + dx;
  t.o100 = b10 + x0; t.o101 = t.o100 + dx;
  t.o110 = b11 + x0; t.o111 = t.o110 + dx;
  return t;
}

__device__ __forceinline__ f32x4 ldrec(__amdgpu_buffer_rsrc_t rs, u32 off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
}

typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
template <bool B16>
__device__ __forceinline__ f32x4 ldrec_t(__amdgpu_buffer_rsrc_t rs, u32 off) {
  if constexpr (B16)
    return __builtin_convertvector(__builtin_bit_cast(bf16x4r, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)off, 0, 0)), f32x4);
  else
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, 0));
}

// sum over the 4 lanes of a quad (all four receive it)
__device__ __forceinline__ float quad_sum4(float v) {
  const float a = v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, true));   // [1,0,3,2]
  return a + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(a), 0x4E, 0xF, 0xF, true));            // [2,3,0,1]
}

// Element offset of sample n's volume in the indexed kernels.  n is workgroup-uniform in every one of them, so this is one scalar
// load per workgroup; the index is clamped into [0, vol_n) -- a bad table can never leave the buffer -- and the offset is formed in
// 64 bits.
__device__ __forceinline__ long vol_offset(int n, long vol_bstride, const int* __restrict__ vol_idx, int vol_n) {
  const int v = vol_idx[n];
  return (long)(v < 0 ? 0 : (v >= vol_n ? vol_n - 1 : v)) * vol_bstride;
}

// The six default kernels, once per addressing form (resample_gather.inc explains why the sharing is textual): sample n reads
// volume n (or the one volume all samples share: vol_bstride 0), then volume vol_idx[n] of a table.
#define GATHER_KERNEL(stem) stem##_kernel
#define GATHER_TABLE_PARAMS
#define GATHER_VOL_OFFSET ((long)n * vol_bstride)
#include "resample_gather.inc"
#undef GATHER_KERNEL
#undef GATHER_TABLE_PARAMS
#undef GATHER_VOL_OFFSET
#define GATHER_KERNEL(stem) stem##_indexed_kernel
#define GATHER_TABLE_PARAMS const int* __restrict__ vol_idx, int vol_n,
#define GATHER_VOL_OFFSET vol_offset(n, vol_bstride, vol_idx, vol_n)
#include "resample_gather.inc"
#undef GATHER_KERNEL
#undef GATHER_TABLE_PARAMS
#undef GATHER_VOL_OFFSET

// 16-channel gather with the per-voxel arithmetic done once per voxel (variant 5 of lf_set_tuning key 1).  The default
// gather (resample_fwd_c16_kernel) is bound by VALU issue as much as by the L1 (PMC: VALU busy 93 % of its run time): map, clip and corner offsets are
// evaluated in all four lanes of a voxel.  Here a wave owns a 4x4x4 tile: phase A, lane = voxel, evaluates the 64 maps with
// one instruction stream and leaves (offset of corner 000, the three corner strides, the three fractions) in 2 KB of
// wave-private LDS; phase B, four passes of 16 voxels with lane = (voxel, channel quarter) as before, reads them back (one
// broadcast read per quad), forms the 8 weights and fetches the coalesced 64-byte records.  Same operations per voxel in the
// same order: bit-identical to resample_fwd_c16_kernel.
template <int KIND>
__global__ void __launch_bounds__(256) resample_fwd_c16_dedup_kernel(
    const float* __restrict__ vol, long vol_bstride, const float* __restrict__ coef,
    float* __restrict__ out, int D, int H, int W, int nbx, int nby, int nbz, Steps st) {
  __shared__ u32x4_t tapo[4][64];                                 // o000 | dead, dx, dy, dz (bytes; 0 if clamped)
  __shared__ f32x4 tapf[4][64];                                   // tx, ty, tz, -
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // tile index: 4 x-adjacent 4^3 tiles per workgroup (one per wave)
  const int n = blockIdx.z / nbz, bz = blockIdx.z - n * nbz;
  const int x0 = ((blockIdx.x << 2) + wave) << 2, y0 = blockIdx.y << 2, z0 = bz << 2;
  const u32 sample_bytes = (u32)D * (u32)H * (u32)W * 64u;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(vol + (long)n * vol_bstride), 0, sample_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)(out + (long)n * D * H * W * 16), 0, sample_bytes, 0x00020000);
  const float* cf = coef + n * LF_MAP_COEFS;
  {
    const int x = x0 + (lane & 3), y = y0 + ((lane >> 2) & 3), z = z0 + (lane >> 4);
    const bool live = x < W && y < H && z < D;
    float gx, gy, gz, a, b, k;
    eval_grid<KIND>(cf, live ? x : 0, live ? y : 0, live ? z : 0, W, H, D, st, gx, gy, gz, a, b, k);
    const Tap32 t = make_tap32(gx, gy, gz, W, H, D, 64u);
    u32x4_t o;
    o[0] = live ? t.o000 : 0xffffffffu;
    o[1] = t.o001 - t.o000; o[2] = t.o010 - t.o000; o[3] = t.o100 - t.o000;
    tapo[wave][lane] = o;
    tapf[wave][lane] = (f32x4){t.tx, t.ty, t.tz, 0.f};
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const int q = lane & 3, vq = lane >> 2;
  const u32 co = (u32)q * 16u;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int vi = 16 * i + vq;
    const u32x4_t o = tapo[wave][vi];
    const f32x4 f = tapf[wave][vi];
    if (o[0] == 0xffffffffu) continue;                            // voxel outside the volume (ragged tiles)
    const u32 b00 = o[0] + co, b01 = b00 + o[2], b10 = b00 + o[3], b11 = b01 + o[3];
    const f32x4 v000 = ldrec(rs, b00), v001 = ldrec(rs, b00 + o[1]), v010 = ldrec(rs, b01), v011 = ldrec(rs, b01 + o[1]);
    const f32x4 v100 = ldrec(rs, b10), v101 = ldrec(rs, b10 + o[1]), v110 = ldrec(rs, b11), v111 = ldrec(rs, b11 + o[1]);
    const float wx1 = f[0], wx0 = 1.f - f[0], wy1 = f[1], wy0 = 1.f - f[1], wz1 = f[2], wz0 = 1.f - f[2];
    const float w000 = wx0 * wy0 * wz0, w001 = wx1 * wy0 * wz0, w010 = wx0 * wy1 * wz0, w011 = wx1 * wy1 * wz0;
    const float w100 = wx0 * wy0 * wz1, w101 = wx1 * wy0 * wz1, w110 = wx0 * wy1 * wz1, w111 = wx1 * wy1 * wz1;
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float acc = v000[e] * w000;
      asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v001[e]), "v"(w001));
      asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v010[e]), "v"(w010));
      asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v011[e]), "v"(w011));
      asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v100[e]), "v"(w100));
      asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v101[e]), "v"(w101));
      asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v110[e]), "v"(w110));
      asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v111[e]), "v"(w111));
      r[e] = acc;
    }
    const int x = x0 + (vi & 3), y = y0 + ((vi >> 2) & 3), z = z0 + (vi >> 4);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, r), ro, (int)((u32)((z * H + y) * W + x) * 64u + co), 0, 2);
  }
}

#include "resample_staged.inc"

#ifdef STAGED_TPW_OVERRIDE
constexpr int STAGED_TPW = STAGED_TPW_OVERRIDE;
#else
constexpr int STAGED_TPW = 16;   // tiles per workgroup of the staged coefficient gradient
#endif

int g_bwd_coef_variant = 10;   // lean coefficient gradient: 1 = one sub-tile in flight (6 waves/SIMD), 2 = two (4 waves/SIMD; r02 default),
                              // 3 = as 2 with a 128-register cap, 4 / 5 = one in flight capped at 6 / 8 waves/SIMD
int g_resample_variant = 3;   // 1 = generic kernels, 2 = lean kernels, 3 = lean + 16-channel gather, 4 = LDS-staged footprint (16 channels;
                              // other shapes as 3) (lf_set_tuning)

}  // namespace

// Shape rules and launch geometry of the gather, shared by lf_resample3d_fwd and lf_resample3d_fwd_indexed.  With 16 channels
// (vec) a voxel takes 4 threads and the tile is 4x4x4, so grid and nbz are also those of the 16-channel kernels.
struct FwdPlan {
  bool vec;                                              // 4-channel groups (C % 4 == 0, 16-byte aligned)
  int lpt, tlx, tly, tlz, nbz;                           // threads cooperating on one voxel; log2 tile extents; tiles along z
  dim3 grid;
  Steps st;
};
static int fwd_plan(const float* vol, const float* out, int N, int D, int H, int W, int C, FwdPlan& p) {
  if ((long)D * H * W >= 0x7fffffffL) return LF_EINVAL;
  p.vec = (C % 4 == 0) && lf_aligned16(vol) && lf_aligned16(out);
  const int lpv = p.vec ? C / 4 : C;
  p.lpt = lpv < 256 ? lpv : 256;
  int lg = 0;                                            // log2(voxels per block), rounded down
  while ((2 << lg) * p.lpt <= 256) ++lg;
  if (lg >= 6) { p.tlx = (lg + 2) / 3; p.tly = (lg + 1) / 3; p.tlz = lg / 3; }      // 6:(2,2,2) 7:(3,2,2) 8:(3,3,2)
  else         { p.tlx = lg < 2 ? lg : 2; p.tly = lg - p.tlx < 2 ? lg - p.tlx : 2; p.tlz = lg - p.tlx - p.tly; }   // 5:(2,2,1) 4:(2,2,0) ...
  p.nbz = (D + (1 << p.tlz) - 1) >> p.tlz;
  const int nby = (H + (1 << p.tly) - 1) >> p.tly;
  if ((long)p.nbz * N > 65535 || nby > 65535) return LF_EINVAL;
  p.grid = dim3((unsigned)((W + (1 << p.tlx) - 1) >> p.tlx), (unsigned)nby, (unsigned)(p.nbz * N));
  p.st = make_steps(D, H, W);
  return 0;
}

extern "C" int lf_resample3d_fwd(const float* vol, int vol_n, const float* coef, int kind, float* out,
                                 int N, int D, int H, int W, int C, void* stream) {
  lf_clear_error();
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return LF_EINVAL;
  if (vol_n != 1 && vol_n != N) return LF_EINVAL;
  if (kind != LF_MAP_O2C && kind != LF_MAP_C2O) return LF_EINVAL;
  const long bstride = vol_n == 1 ? 0 : (long)D * H * W * C;
  FwdPlan p;
  if (int e = fwd_plan(vol, out, N, D, H, W, C, p)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (g_resample_variant == 4 && p.vec && C == 16 && (long)D * H * W * 64 < 0xffffffffL && W <= 65535) {
    const int ntx = (W + LT_X - 1) / LT_X, nty = (H + LT_Y - 1) / LT_Y, ntz = (D + LT_Z - 1) / LT_Z;
    const long nwg = (long)ntx * nty * ntz * N;
    if (nwg > 0x7fffffffL) return LF_EINVAL;
    LAUNCH_BY_KIND(resample_fwd_staged_kernel, dim3((unsigned)nwg), vol, bstride, coef, out, D, H, W, ntx, nty, ntz, p.st);
    return lf_launch_status();
  }
  if (g_resample_variant == 5 && p.vec && C == 16 && (long)D * H * W * 64 < 0xffffffffL) {
    const int nbz4 = (D + 3) >> 2, nbx16 = (W + 15) >> 4, nby4 = (H + 3) >> 2;
    if ((long)nbz4 * N > 65535 || nby4 > 65535) return LF_EINVAL;
    dim3 g5((unsigned)nbx16, (unsigned)nby4, (unsigned)(nbz4 * N));
    LAUNCH_BY_KIND(resample_fwd_c16_dedup_kernel, g5, vol, bstride, coef, out, D, H, W, nbx16, nby4, nbz4, p.st);
    return lf_launch_status();
  }
  if (g_resample_variant >= 3 && p.vec && C == 16 && (long)D * H * W * 64 < 0xffffffffL) {
    LAUNCH_BY_KIND(resample_fwd_c16_kernel, p.grid, vol, bstride, coef, out, D, H, W, p.nbz, p.st);
  } else if (g_resample_variant >= 2 && p.vec && (long)D * H * W * C * 4 < 0xffffffffL) {
    LAUNCH_BY_KIND(resample_fwd_lean_kernel, p.grid, vol, bstride, coef, out, D, H, W, C, p.lpt, p.tlx, p.tly, p.tlz, p.nbz, p.st);
  } else {
#define LAUNCH(K, V) hipLaunchKernelGGL((resample_fwd_kernel<K, V>), p.grid, dim3(256), 0, s, vol, bstride, coef, out, N, D, H, W, C, p.lpt, p.tlx, p.tly, p.tlz, p.nbz, p.st)
    if (kind == LF_MAP_O2C) { if (p.vec) LAUNCH(LF_MAP_O2C, 4); else LAUNCH(LF_MAP_O2C, 1); }
    else                    { if (p.vec) LAUNCH(LF_MAP_C2O, 4); else LAUNCH(LF_MAP_C2O, 1); }
#undef LAUNCH
  }
  return lf_launch_status();
}

static long staged_bwd_blocks(int D, int H, int W) {
  const long nt = (long)((W + LT_X - 1) / LT_X) * ((H + LT_Y - 1) / LT_Y) * ((D + LT_Z - 1) / LT_Z);
  return (nt + STAGED_TPW - 1) / STAGED_TPW;
}

// part_n: the sample count the voxels per block are chosen for (N for lf_resample3d_bwd_coef; the caller's group size for
// lf_resample3d_bwd_coef_part, whose samples then sum exactly as a launch of part_n samples would)
static size_t bwd_coef_scratch_bytes(int N, int part_n, int D, int H, int W) {
  const long nvox = (long)D * H * W;
  const int vpb = bwd_vox_per_block(nvox, part_n);
  const BwdTile bt = bwd_tile(vpb, D, H, W);
  const long nblk = (long)bt.ntx * bt.nty * bt.ntz;
  const long nblk_staged = staged_bwd_blocks(D, H, W);             // whichever form runs (lf_set_tuning) must fit
  return (size_t)N * (nblk > nblk_staged ? nblk : nblk_staged) * 18 * sizeof(float);
}

extern "C" size_t lf_resample3d_bwd_coef_scratch_bytes(int N, int D, int H, int W) {
  return bwd_coef_scratch_bytes(N, N, D, H, W);
}

extern "C" size_t lf_resample3d_bwd_coef_part_scratch_bytes(int N, int part_n, int D, int H, int W) {
  if (N <= 0 || part_n <= 0) return 0;
  return bwd_coef_scratch_bytes(N, part_n, D, H, W);
}

// Shape rules and launch geometry of the coefficient gradient's stage 1, shared by bwd_coef_launch and
// lf_resample3d_bwd_coef_indexed.
struct BwdCoefPlan {
  long nvox;
  int vpb, nblk, lpv;                                    // voxels per block; blocks per sample; lanes per voxel
  BwdTile bt;
  bool vec;                                              // 4-channel groups (C % 4 == 0, 16-byte aligned)
  dim3 grid;
  Steps st;
};
static int bwd_coef_plan(const float* gout, const float* vol, size_t scratch_bytes, int N, int part_n, int D, int H, int W, int C,
                         BwdCoefPlan& p) {
  if (scratch_bytes < bwd_coef_scratch_bytes(N, part_n, D, H, W)) return LF_ENOSPC;
  if ((long)D * H * W >= 0x7fffffffL) return LF_EINVAL;
  p.nvox = (long)D * H * W;
  p.vpb = bwd_vox_per_block(p.nvox, part_n);
  p.bt = bwd_tile(p.vpb, D, H, W);
  const long nblk_l = (long)p.bt.ntx * p.bt.nty * p.bt.ntz;
  if (nblk_l * N > 0x7fffffffL) return LF_EINVAL;
  p.nblk = (int)nblk_l;
  p.grid = dim3((unsigned)(nblk_l * N));
  // lanes per voxel: next power of two covering the channel groups (idle lanes contribute 0)
  p.vec = (C % 4 == 0) && lf_aligned16(gout) && lf_aligned16(vol);
  const int groups = p.vec ? C / 4 : C;
  p.lpv = 1;
  while (p.lpv < groups) p.lpv <<= 1;
  if (p.lpv > 64) return LF_EINVAL;                      // C > 256 (vec) / C > 64 (scalar)
  p.st = make_steps(D, H, W);
  return 0;
}

// stage 2 behind a stage-1 launch: the fixed-order sum of the nblk partials of every sample
static int bwd_coef_finish(const float* partial, int nblk, float* gcoef, int N, hipStream_t s) {
  if (int e = lf_launch_status()) return e;
  hipLaunchKernelGGL(resample_bwd_coef_reduce, dim3(N), dim3(256), 0, s, partial, nblk, gcoef);
  return lf_launch_status();
}

static int bwd_coef_launch(const float* gout, const float* vol, int vol_n, const float* coef,
                           float* gcoef, void* scratch, size_t scratch_bytes,
                           int N, int part_n, int D, int H, int W, int C, void* stream) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return LF_EINVAL;
  if (vol_n != 1 && vol_n != N) return LF_EINVAL;
  BwdCoefPlan p;
  if (int e = bwd_coef_plan(gout, vol, scratch_bytes, N, part_n, D, H, W, C, p)) return e;
  const long bstride = vol_n == 1 ? 0 : p.nvox * C;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)scratch;
  if (g_resample_variant == 4 && p.vec && C == 16 && p.nvox * 64 < 0xffffffffL && W <= 65535) {
    const int ntx = (W + LT_X - 1) / LT_X, nty = (H + LT_Y - 1) / LT_Y, ntz = (D + LT_Z - 1) / LT_Z;
    const long nb = staged_bwd_blocks(D, H, W);
    if (nb * N > 0x7fffffffL) return LF_EINVAL;
    hipLaunchKernelGGL((resample_bwd_coef_staged_kernel<STAGED_TPW>), dim3((unsigned)(nb * N)), dim3(256), 0, s, gout, vol, bstride, coef,
                       partial, (int)nb, D, H, W, ntx, nty, ntz, p.st);
    return bwd_coef_finish(partial, (int)nb, gcoef, N, s);
  }
  if (g_resample_variant >= 2 && p.vec && C == 16 && p.vpb >= 64 && p.nvox * 64 < 0xffffffffL) {
    const int v = g_bwd_coef_variant;
    const bool big = p.vpb >= 256;                       // the dedup forms need a sub-tile per wave
#define LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), p.grid, dim3(256), 0, s, gout, vol, bstride, coef, partial, p.nblk, p.vpb, p.bt, D, H, W, p.st)
    if (v == 1)              LAUNCH(resample_bwd_coef_c16_kernel<1, 1>);
    else if (v == 2)         LAUNCH(resample_bwd_coef_c16_kernel<1, 2>);
    else if (v == 3)         LAUNCH(resample_bwd_coef_c16_kernel<4, 2>);
    else if (v == 6 && big)  LAUNCH(resample_bwd_coef_c16_dedup_kernel<2, 1>);
    else if (v == 7 && big)  LAUNCH(resample_bwd_coef_c16_dedup_kernel<1, 1>);
    else if (v == 8 && big)  LAUNCH(resample_bwd_coef_c16_dedup_kernel<2, 4>);
    else if (v == 9 && big)  LAUNCH(resample_bwd_coef_c16_dedup_kernel<1, 5>);
    else if (v == 10 && big) LAUNCH(resample_bwd_coef_c16_dedup_kernel<2, 1, true>);
    else if (v == 11 && big) LAUNCH(resample_bwd_coef_c16_dedup_kernel<1, 1, true>);
    else if (v == 4)         LAUNCH(resample_bwd_coef_c16_kernel<6, 1>);
    else                     LAUNCH(resample_bwd_coef_c16_kernel<8, 1>);
#undef LAUNCH
  } else if (p.vec) {
    hipLaunchKernelGGL((resample_bwd_coef_kernel<4>), p.grid, dim3(256), 0, s, gout, vol, bstride, coef, partial, p.nblk, p.vpb, p.bt, N, D, H, W, C, p.lpv, p.st);
  } else {
    hipLaunchKernelGGL((resample_bwd_coef_kernel<1>), p.grid, dim3(256), 0, s, gout, vol, bstride, coef, partial, p.nblk, p.vpb, p.bt, N, D, H, W, C, p.lpv, p.st);
  }
  return bwd_coef_finish(partial, p.nblk, gcoef, N, s);
}

extern "C" int lf_resample3d_bwd_coef(const float* gout, const float* vol, int vol_n, const float* coef,
                                      float* gcoef, void* scratch, size_t scratch_bytes,
                                      int N, int D, int H, int W, int C, void* stream) {
  lf_clear_error();
  return bwd_coef_launch(gout, vol, vol_n, coef, gcoef, scratch, scratch_bytes, N, N, D, H, W, C, stream);
}

extern "C" int lf_resample3d_bwd_coef_part(const float* gout, const float* vol, int vol_n, const float* coef,
                                           float* gcoef, void* scratch, size_t scratch_bytes,
                                           int N, int D, int H, int W, int C, int part_n, void* stream) {
  lf_clear_error();
  if (!gout || !vol || !coef || !gcoef || !scratch) return LF_EINVAL;
  if (part_n <= 0 || N <= 0) return LF_EINVAL;
  return bwd_coef_launch(gout, vol, vol_n, coef, gcoef, scratch, scratch_bytes, N, part_n, D, H, W, C, stream);
}

// ---- several source volumes behind one launch: sample i reads volume vol_idx[i] (lf_hip.h) ----------------------------------
// The plan is lf_resample3d_fwd's; the kernels are the indexed instances of resample_gather.inc.  The lf_set_tuning forms that
// have no indexed kernel (staged footprint, per-voxel dedup gather) run the default form here.
extern "C" int lf_resample3d_fwd_indexed(const float* vol, int vol_n, const int* vol_idx, const float* coef, int kind, float* out,
                                         int N, int D, int H, int W, int C, void* stream) {
  lf_clear_error();
  if (!vol || !vol_idx || !coef || !out) return LF_EINVAL;
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0 || vol_n < 1) return LF_EINVAL;
  if (kind != LF_MAP_O2C && kind != LF_MAP_C2O) return LF_EINVAL;
  if (((uintptr_t)vol_idx & 3) != 0) return LF_EALIGN;
  const long bstride = (long)D * H * W * C;                // every volume is addressed through the table, vol_n == 1 included
  FwdPlan p;
  if (int e = fwd_plan(vol, out, N, D, H, W, C, p)) return e;
  hipStream_t s = (hipStream_t)stream;
  if (g_resample_variant >= 3 && p.vec && C == 16 && (long)D * H * W * 64 < 0xffffffffL) {
    LAUNCH_BY_KIND(resample_fwd_c16_indexed_kernel, p.grid, vol, bstride, vol_idx, vol_n, coef, out, D, H, W, p.nbz, p.st);
  } else if (g_resample_variant >= 2 && p.vec && (long)D * H * W * C * 4 < 0xffffffffL) {
    LAUNCH_BY_KIND(resample_fwd_lean_indexed_kernel, p.grid, vol, bstride, vol_idx, vol_n, coef, out, D, H, W, C, p.lpt, p.tlx, p.tly, p.tlz, p.nbz, p.st);
  } else {
#define LAUNCH(K, V) hipLaunchKernelGGL((resample_fwd_indexed_kernel<K, V>), p.grid, dim3(256), 0, s, vol, bstride, vol_idx, vol_n, coef, out, N, D, H, W, C, p.lpt, p.tlx, p.tly, p.tlz, p.nbz, p.st)
    if (kind == LF_MAP_O2C) { if (p.vec) LAUNCH(LF_MAP_O2C, 4); else LAUNCH(LF_MAP_O2C, 1); }
    else                    { if (p.vec) LAUNCH(LF_MAP_C2O, 4); else LAUNCH(LF_MAP_C2O, 1); }
#undef LAUNCH
  }
  return lf_launch_status();
}

extern "C" size_t lf_resample3d_bwd_coef_indexed_scratch_bytes(int N, int part_n, int D, int H, int W) {
  if (N <= 0 || part_n <= 0) return 0;
  return bwd_coef_scratch_bytes(N, part_n, D, H, W);
}

// lf_resample3d_bwd_coef_part over a table of volumes: the plan and the fixed-order finish are bwd_coef_launch's.
// 16 channels run the default forms (lf_set_tuning key 2 = 10: the per-voxel dedup kernel when a block holds >= 256 voxels, else
// the four-lanes-per-voxel kernel); other values of that key run these two as well.
extern "C" int lf_resample3d_bwd_coef_indexed(const float* gout, const float* vol, int vol_n, const int* vol_idx, const float* coef,
                                              float* gcoef, void* scratch, size_t scratch_bytes,
                                              int N, int D, int H, int W, int C, int part_n, void* stream) {
  lf_clear_error();
  if (!gout || !vol || !vol_idx || !coef || !gcoef || !scratch) return LF_EINVAL;
  if (part_n <= 0 || N <= 0 || vol_n < 1) return LF_EINVAL;
  if (D <= 0 || H <= 0 || W <= 0 || C <= 0) return LF_EINVAL;
  if (((uintptr_t)vol_idx & 3) != 0) return LF_EALIGN;
  BwdCoefPlan p;
  if (int e = bwd_coef_plan(gout, vol, scratch_bytes, N, part_n, D, H, W, C, p)) return e;
  const long bstride = p.nvox * C;                         // every volume is addressed through the table, vol_n == 1 included
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)scratch;
  if (g_resample_variant >= 2 && p.vec && C == 16 && p.vpb >= 64 && p.nvox * 64 < 0xffffffffL) {
    if (p.vpb >= 256)
      hipLaunchKernelGGL((resample_bwd_coef_c16_dedup_indexed_kernel<2, 1, true>), p.grid, dim3(256), 0, s, gout, vol, bstride, vol_idx, vol_n, coef, partial, p.nblk, p.vpb, p.bt, D, H, W, p.st);
    else
      hipLaunchKernelGGL((resample_bwd_coef_c16_indexed_kernel<8, 1>), p.grid, dim3(256), 0, s, gout, vol, bstride, vol_idx, vol_n, coef, partial, p.nblk, p.vpb, p.bt, D, H, W, p.st);
  } else if (p.vec) {
    hipLaunchKernelGGL((resample_bwd_coef_indexed_kernel<4>), p.grid, dim3(256), 0, s, gout, vol, bstride, vol_idx, vol_n, coef, partial, p.nblk, p.vpb, p.bt, N, D, H, W, C, p.lpv, p.st);
  } else {
    hipLaunchKernelGGL((resample_bwd_coef_indexed_kernel<1>), p.grid, dim3(256), 0, s, gout, vol, bstride, vol_idx, vol_n, coef, partial, p.nblk, p.vpb, p.bt, N, D, H, W, C, p.lpv, p.st);
  }
  return bwd_coef_finish(partial, p.nblk, gcoef, N, s);
}

extern "C" int lf_resample3d_bwd_vol(const float* gout, const float* coef, int kind, float* gvol, int vol_n,
                                     int N, int D, int H, int W, int C, void* stream) {
  lf_clear_error();
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return LF_EINVAL;
  if (vol_n != 1 && vol_n != N) return LF_EINVAL;
  const long bstride = vol_n == 1 ? 0 : (long)D * H * W * C;
  const long items = (long)D * H * W * C;
  dim3 grid((unsigned)min((items + 255) / 256, (long)65535 * 16), N), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (kind == LF_MAP_O2C)
    hipLaunchKernelGGL((resample_bwd_vol_kernel<LF_MAP_O2C>), grid, block, 0, s, gout, coef, gvol, bstride, N, D, H, W, C, make_steps(D, H, W));
  else if (kind == LF_MAP_C2O)
    hipLaunchKernelGGL((resample_bwd_vol_kernel<LF_MAP_C2O>), grid, block, 0, s, gout, coef, gvol, bstride, N, D, H, W, C, make_steps(D, H, W));
  else
    return LF_EINVAL;
  return lf_launch_status();
}

#ifdef STAGE_TS
extern "C" int lf_debug_stage_ts(void* dst) {                      // experimental builds only (tools/stage_timeline.py)
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_stage_ts), sizeof(unsigned long long) * 256 * 16, 0, hipMemcpyDeviceToHost);
}
#endif

// Tuning / A-B switch (not part of the functional interface): key 1 = resampler variant (1 generic, 2 lean, 3 lean + 16-channel
// gather, 4 LDS-staged footprint, 5 per-voxel dedup gather).  Returns the previous value, or LF_EINVAL for an unknown key.
extern "C" int lf_set_tuning(int key, int value) {
  if (key == 1) {
    const int prev = g_resample_variant;
    if (value >= 1 && value <= 5) g_resample_variant = value;
    return prev;
  }
  if (key == 4) return lf_internal_splat_set_variant(value);        // deterministic splat: form 1..4
  if (key == 6) return lf_internal_splat_set_chunk_cap(value);      // binned splat: samples per pass at most, 0 = by memory only
  if (key == 3) return lf_internal_fused_set_cfg(value);            // fused wide-conv GEMM: workgroup shape 0..3, -1 = by shape
  if (key == 7) return lf_internal_wino_set_pack(value);            // fp32 Winograd 16-channel kernels: 1 = packed transforms (default), 0 = scalar
  if (key == 8) return lf_internal_wino_set_forms(value);           // same kernels: 1 = compile-time epilogue forms (default), 0 = generic, 2 = forms, freed registers unspent, 3 / 4 = forms on the raw-plane / z-staged halo
  if (key == 5) return lf_internal_ring_bf16_set_wgs(value);        // bf16 ring convolution: resident workgroups per CU
  if (key == 2) {
    const int prev = g_bwd_coef_variant;
    if (value >= 1 && value <= 11) g_bwd_coef_variant = value;
    return prev;
  }
  return LF_EINVAL;
}

// ---- storage-type variants for the training step's bf16 storage policy (16-channel volumes only) ----
extern "C" int lf_resample3d_fwd_io(const void* vol, int vol_n, const float* coef, int kind, void* out,
                                    int N, int D, int H, int W, int io, void* stream) {
  lf_clear_error();
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || io < 0 || io > 3) return LF_EINVAL;
  if ((vol_n != 1 && vol_n != N) || (kind != LF_MAP_O2C && kind != LF_MAP_C2O)) return LF_EINVAL;
  if (!lf_aligned16(vol) || !lf_aligned16(out)) return LF_EALIGN;
  if ((long)D * H * W * 64 >= 0xffffffffL) return LF_EINVAL;
  const long bstride = vol_n == 1 ? 0 : (long)D * H * W * 16;
  const int nbz4 = (D + 3) >> 2;
  if ((long)nbz4 * N > 65535 || ((H + 3) >> 2) > 65535) return LF_EINVAL;
  dim3 g4((unsigned)((W + 3) >> 2), (unsigned)((H + 3) >> 2), (unsigned)(nbz4 * N)), block(256);
  const Steps st = make_steps(D, H, W);
  typedef void (*kern_t)(const float*, long, const float*, float*, int, int, int, int, Steps);
  static const kern_t kerns[2][4] = {
      {resample_fwd_c16_kernel<LF_MAP_O2C, 0>, resample_fwd_c16_kernel<LF_MAP_O2C, 1>, resample_fwd_c16_kernel<LF_MAP_O2C, 2>, resample_fwd_c16_kernel<LF_MAP_O2C, 3>},
      {resample_fwd_c16_kernel<LF_MAP_C2O, 0>, resample_fwd_c16_kernel<LF_MAP_C2O, 1>, resample_fwd_c16_kernel<LF_MAP_C2O, 2>, resample_fwd_c16_kernel<LF_MAP_C2O, 3>}};
  hipLaunchKernelGGL(kerns[kind == LF_MAP_O2C ? 0 : 1][io], g4, block, 0, (hipStream_t)stream, (const float*)vol, bstride, coef, (float*)out, D, H, W, nbz4, st);
  return lf_launch_status();
}
