// The six default resampler kernels (trilinear gather and its coefficient gradient), written once and compiled twice.
// resample.hip includes this file two times inside its anonymous namespace, under three macros:
//   GATHER_KERNEL(stem)    the kernel's name: stem_kernel (plain), stem_indexed_kernel (indexed);
//   GATHER_TABLE_PARAMS    the extra parameters after vol_bstride: nothing, or `const int* __restrict__ vol_idx, int vol_n,`;
//   GATHER_VOL_OFFSET      element offset of sample n's source volume: n * vol_bstride, or vol_offset(n, vol_bstride, vol_idx, vol_n)
//                          (sample n reads volume vol_idx[n] of vol_n volumes laid back to back: several objects' hypotheses in
//                          one launch, lf_resample3d_fwd_indexed / lf_resample3d_bwd_coef_indexed).
// Everything else -- helpers, the kernels that have no indexed form -- lives in resample.hip.
//
// The sharing is textual on purpose: the compiler sees the token streams of two hand-written sets of kernels, so the plain
// kernels' device code cannot move when the indexed form is touched and the two forms cannot drift apart (per sample the operations
// and their order are the same, so the outputs are bit-identical: tests/test_resample_indexed_gpu.py).  The C++ routes were
// measured with tools/resample_isa_diff.py and all re-scheduled kernels nobody has timed:
//   * one __forceinline__ body taking a null table: changed the plain kernels' register allocation and instruction order;
//   * a `template <..., bool IDX>` device body behind two thin __global__ wrappers, `if constexpr` around the base offset: 31 of
//     84 symbols differed (resample_fwd_kernel<*,4> re-scheduled, every resample_bwd_coef* kernel 1 to 5 instructions longer or
//     shorter, resample_fwd_c16_kernel with swapped operands);
//   * the kernels themselves templated on `bool IDX` with a VolSrc<IDX> struct in place of (vol, vol_bstride): 33 of 84 symbols
//     differed, the plain resample_fwd_c16_kernel 3 instructions longer.
// A change here is checked the same way: tools/resample_isa_diff.py (profiles/resample_shared_isa.txt: 84 symbols, no difference
// against the two hand-written copies this file replaced).

// VEC = 4: one thread per (voxel, 4-channel group), C % 4 == 0.  VEC = 1: one thread per (voxel, channel).
// A block covers a compact 2^lx x 2^ly x 2^lz output tile (4x4x4 for C = 16), so that the 8-corner
// footprints of its voxels overlap in L1; 32-bit index math only.
template <int KIND, int VEC>
__global__ void __launch_bounds__(256) GATHER_KERNEL(resample_fwd)(
    const float* __restrict__ vol, long vol_bstride, GATHER_TABLE_PARAMS const float* __restrict__ coef,
    float* __restrict__ out, int N, int D, int H, int W, int C, int lpt, int lx, int ly, int lz, int nbz, Steps st) {
  // lpt = threads cooperating on one voxel (<= 256); tile = (1<<lx, 1<<ly, 1<<lz) voxels per block
  const int lpv = C / VEC;
  const int n = blockIdx.z / nbz, bz = blockIdx.z - n * nbz;
  const int slot = threadIdx.x / lpt, q0 = threadIdx.x - slot * lpt;
  if (slot >= (1 << (lx + ly + lz))) return;
  const int x = (blockIdx.x << lx) + (slot & ((1 << lx) - 1));
  const int y = (blockIdx.y << ly) + ((slot >> lx) & ((1 << ly) - 1));
  const int z = (bz << lz) + (slot >> (lx + ly));
  if (x >= W || y >= H || z >= D) return;
  const float* cf = coef + (long)n * LF_MAP_COEFS;
  float gx, gy, gz, a, b, k;
  eval_grid<KIND>(cf, x, y, z, W, H, D, st, gx, gy, gz, a, b, k);
  const Tap t = make_tap(gx, gy, gz, W, H, D);
  const float wx1 = t.tx, wx0 = 1.f - t.tx, wy1 = t.ty, wy0 = 1.f - t.ty, wz1 = t.tz, wz0 = 1.f - t.tz;
  const float w000 = wx0 * wy0 * wz0, w001 = wx1 * wy0 * wz0, w010 = wx0 * wy1 * wz0, w011 = wx1 * wy1 * wz0;
  const float w100 = wx0 * wy0 * wz1, w101 = wx1 * wy0 * wz1, w110 = wx0 * wy1 * wz1, w111 = wx1 * wy1 * wz1;
  const int r00 = (t.z0 * H + t.y0) * W, r01 = (t.z0 * H + t.y1) * W;        // voxel indices of the 4 rows
  const int r10 = (t.z1 * H + t.y0) * W, r11 = (t.z1 * H + t.y1) * W;
  const float* base = vol + GATHER_VOL_OFFSET;
  float* orow = out + ((long)n * D * H * W + ((long)z * H + y) * W + x) * C;
  for (int q = q0; q < lpv; q += lpt) {
    const int co = q * VEC;
    if (VEC == 4) {
      const f32x4 v000 = *(const f32x4*)(base + (long)(r00 + t.x0) * C + co), v001 = *(const f32x4*)(base + (long)(r00 + t.x1) * C + co);
      const f32x4 v010 = *(const f32x4*)(base + (long)(r01 + t.x0) * C + co), v011 = *(const f32x4*)(base + (long)(r01 + t.x1) * C + co);
      const f32x4 v100 = *(const f32x4*)(base + (long)(r10 + t.x0) * C + co), v101 = *(const f32x4*)(base + (long)(r10 + t.x1) * C + co);
      const f32x4 v110 = *(const f32x4*)(base + (long)(r11 + t.x0) * C + co), v111 = *(const f32x4*)(base + (long)(r11 + t.x1) * C + co);
      const f32x4 r = v000 * w000 + v001 * w001 + v010 * w010 + v011 * w011 + v100 * w100 + v101 * w101 + v110 * w110 +
                      v111 * w111;
      __builtin_nontemporal_store(r, (f32x4*)(orow + co));     // streamed output: keep L2 for the gathered volume
    } else {
      // the roundings of resample_fwd_c16's fmac chain, spelled out (first product rounded, the other seven fused in corner
      // order): a 16-channel volume that is not 16-byte aligned lands here and gets the bits of the aligned call; left to the
      // compiler's contraction the same sum fused the first product and rounded the second
      float r = base[(long)(r00 + t.x0) * C + co] * w000;
      r = __builtin_fmaf(base[(long)(r00 + t.x1) * C + co], w001, r);
      r = __builtin_fmaf(base[(long)(r01 + t.x0) * C + co], w010, r);
      r = __builtin_fmaf(base[(long)(r01 + t.x1) * C + co], w011, r);
      r = __builtin_fmaf(base[(long)(r10 + t.x0) * C + co], w100, r);
      r = __builtin_fmaf(base[(long)(r10 + t.x1) * C + co], w101, r);
      r = __builtin_fmaf(base[(long)(r11 + t.x0) * C + co], w110, r);
      r = __builtin_fmaf(base[(long)(r11 + t.x1) * C + co], w111, r);
      orow[co] = r;
    }
  }
}

// coefficient gradient, stage 1, generic form (block geometry: bwd_vox_per_block / bwd_tile; stage 2: resample_bwd_coef_reduce)
template <int VEC>
__global__ void __launch_bounds__(256) GATHER_KERNEL(resample_bwd_coef)(
    const float* __restrict__ gout, const float* __restrict__ vol, long vol_bstride, GATHER_TABLE_PARAMS
    const float* __restrict__ coef, float* __restrict__ partial, int nblk, int vpb, BwdTile bt,
    int N, int D, int H, int W, int C, int lpv, Steps st) {
  // lpv = lanes cooperating on one voxel: a power of two <= 64 with lpv * VEC >= C
  const unsigned fb = xcd_contiguous(blockIdx.x, gridDim.x);
  const int n = fb / nblk, blk = fb - n * nblk;
  const float* cf = coef + (long)n * LF_MAP_COEFS;
  const int nvox = D * H * W;                                  // < 2^31 (checked by the launcher)
  const int tx = blk % bt.ntx, ty = (blk / bt.ntx) % bt.nty, tz = blk / (bt.ntx * bt.nty);
  const int q = threadIdx.x % lpv;
  const int vslot = threadIdx.x / lpv;
  const int vstep = blockDim.x / lpv;
  float acc[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) acc[i] = 0.f;
  // all lanes of a wave iterate the same number of times so the shuffles below are convergent
  const int iters = (vpb + vstep - 1) / vstep;
  for (int it = 0; it < iters; ++it) {
    // i-th voxel of the tile: low 6 bits = position inside a 4x4x4 sub-tile, the rest = sub-tile, x fastest
    const int i = it * vstep + vslot;
    const int sub = i >> 6;
    const int sbx = bt.lx - 2, sby = bt.ly - 2;                 // log2 sub-tiles along x, y
    const int x = (tx << bt.lx) + ((sub & ((1 << sbx) - 1)) << 2) + (i & 3);
    const int y = (ty << bt.ly) + (((sub >> sbx) & ((1 << sby) - 1)) << 2) + ((i >> 2) & 3);
    const int z = (tz << bt.lz) + ((sub >> (sbx + sby)) << 2) + ((i >> 4) & 3);
    const bool live = i < vpb && x < W && y < H && z < D;
    const int v = (z * H + y) * W + x;
    float hx = 0.f, hy = 0.f, hz = 0.f, a = 0.f, b = 0.f, k = 0.f;
    if (live && q * VEC < C) {
      float gx, gy, gz;
      eval_grid<LF_MAP_O2C>(cf, x, y, z, W, H, D, st, gx, gy, gz, a, b, k);
      const Tap t = make_tap(gx, gy, gz, W, H, D);
      const float* base = vol + GATHER_VOL_OFFSET + (long)q * VEC;
      const float* g = gout + (((long)n * nvox + v) * C) + (long)q * VEC;
      const long o00 = (long)((t.z0 * H + t.y0) * W) * C, o01 = (long)((t.z0 * H + t.y1) * W) * C;
      const long o10 = (long)((t.z1 * H + t.y0) * W) * C, o11 = (long)((t.z1 * H + t.y1) * W) * C;
      const long x0 = (long)t.x0 * C, x1 = (long)t.x1 * C;
      const float wx1 = t.tx, wx0 = 1.f - t.tx, wy1 = t.ty, wy0 = 1.f - t.ty, wz1 = t.tz, wz0 = 1.f - t.tz;
      float dx = 0.f, dy = 0.f, dz = 0.f;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float go = __builtin_nontemporal_load(g + e);     // streamed once: keep L2 for the gathered volume
        const float v000 = base[o00 + x0 + e], v001 = base[o00 + x1 + e];
        const float v010 = base[o01 + x0 + e], v011 = base[o01 + x1 + e];
        const float v100 = base[o10 + x0 + e], v101 = base[o10 + x1 + e];
        const float v110 = base[o11 + x0 + e], v111 = base[o11 + x1 + e];
        dx += go * ((v001 - v000) * (wy0 * wz0) + (v011 - v010) * (wy1 * wz0) +
                    (v101 - v100) * (wy0 * wz1) + (v111 - v110) * (wy1 * wz1));
        dy += go * ((v010 - v000) * (wx0 * wz0) + (v011 - v001) * (wx1 * wz0) +
                    (v110 - v100) * (wx0 * wz1) + (v111 - v101) * (wx1 * wz1));
        dz += go * ((v100 - v000) * (wx0 * wy0) + (v101 - v001) * (wx1 * wy0) +
                    (v110 - v010) * (wx0 * wy1) + (v111 - v011) * (wx1 * wy1));
      }
      hx = dx * t.mx; hy = dy * t.my; hz = dz * t.mz;
    }
    // sum the channel-group lanes of this voxel (xor butterfly stays inside the lpv-lane group)
    for (int o = lpv >> 1; o > 0; o >>= 1) {
      hx += __shfl_xor(hx, o, 64);
      hy += __shfl_xor(hy, o, 64);
      hz += __shfl_xor(hz, o, 64);
    }
    if (q == 0 && live) {
      const float ak = a * k, bk = b * k;
      acc[0] += hx;       acc[1] += hy;       acc[2] += hz;
      acc[3] += hx * a;   acc[4] += hy * a;   acc[5] += hz * a;
      acc[6] += hx * b;   acc[7] += hy * b;   acc[8] += hz * b;
      acc[9] += hx * k;   acc[10] += hy * k;  acc[11] += hz * k;
      acc[12] += hx * ak; acc[13] += hy * ak; acc[14] += hz * ak;
      acc[15] += hx * bk; acc[16] += hy * bk; acc[17] += hz * bk;
    }
  }
  __shared__ float red[4][18];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    const float s = lf_wave_sum(acc[i]);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 18) {
    const float s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    partial[((long)n * nblk + blk) * 18 + threadIdx.x] = s;
  }
}

// lean gather (what makes the lean variants lean: above Tap32 in resample.hip):
// one thread per (voxel, 4-channel group); block = compact 2^lx x 2^ly x 2^lz tile; C % 4 == 0
template <int KIND>
__global__ void __launch_bounds__(256) GATHER_KERNEL(resample_fwd_lean)(
    const float* __restrict__ vol, long vol_bstride, GATHER_TABLE_PARAMS const float* __restrict__ coef,
    float* __restrict__ out, int D, int H, int W, int C, int lpt, int lx, int ly, int lz, int nbz, Steps st) {
  const int lpv = C >> 2;
  const int n = blockIdx.z / nbz, bz = blockIdx.z - n * nbz;
  const int slot = threadIdx.x / lpt, q0 = threadIdx.x - slot * lpt;
  if (slot >= (1 << (lx + ly + lz))) return;
  const int x = (blockIdx.x << lx) + (slot & ((1 << lx) - 1));
  const int y = (blockIdx.y << ly) + ((slot >> lx) & ((1 << ly) - 1));
  const int z = (bz << lz) + (slot >> (lx + ly));
  if (x >= W || y >= H || z >= D) return;
  const u32 rec = (u32)C * 4u;
  const u32 sample_bytes = (u32)D * (u32)H * (u32)W * rec;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(vol + GATHER_VOL_OFFSET), 0, sample_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)(out + (long)n * D * H * W * C), 0, sample_bytes, 0x00020000);
  const float* cf = coef + n * LF_MAP_COEFS;
  float gx, gy, gz, a, b, k;
  eval_grid<KIND>(cf, x, y, z, W, H, D, st, gx, gy, gz, a, b, k);
  const Tap32 t = make_tap32(gx, gy, gz, W, H, D, rec);
  const float wx1 = t.tx, wx0 = 1.f - t.tx, wy1 = t.ty, wy0 = 1.f - t.ty, wz1 = t.tz, wz0 = 1.f - t.tz;
  const float w000 = wx0 * wy0 * wz0, w001 = wx1 * wy0 * wz0, w010 = wx0 * wy1 * wz0, w011 = wx1 * wy1 * wz0;
  const float w100 = wx0 * wy0 * wz1, w101 = wx1 * wy0 * wz1, w110 = wx0 * wy1 * wz1, w111 = wx1 * wy1 * wz1;
  const u32 orow = (u32)((z * H + y) * W + x) * rec;
  for (int q = q0; q < lpv; q += lpt) {
    const u32 co = (u32)q * 16u;
    const f32x4 v000 = ldrec(rs, t.o000 + co), v001 = ldrec(rs, t.o001 + co), v010 = ldrec(rs, t.o010 + co), v011 = ldrec(rs, t.o011 + co);
    const f32x4 v100 = ldrec(rs, t.o100 + co), v101 = ldrec(rs, t.o101 + co), v110 = ldrec(rs, t.o110 + co), v111 = ldrec(rs, t.o111 + co);
    const f32x4 r = v000 * w000 + v001 * w001 + v010 * w010 + v011 * w011 + v100 * w100 + v101 * w101 + v110 * w110 + v111 * w111;
    // streamed output (nt): keep L2 for the gathered volume
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, r), ro, (int)(orow + co), 0, 2);
  }
}

// C == 16 specialisation of the lean gather (variant 3): fixed 4x4x4 tile, no integer division, no channel loop, one
// scalar-weight FMA per channel and corner (the generic form lets the compiler pack the FMAs in pairs, which costs
// a register move per weight to build the pairs).
// IO (round 5, training step under the bf16 storage policy): bit 0 -- the sampled volume, bit 1 -- the output are bf16
// channels-last records (32 B per voxel); the interpolation itself is the same fp32 arithmetic.
template <int KIND, int IO = 0>
__global__ void __launch_bounds__(256) GATHER_KERNEL(resample_fwd_c16)(
    const float* __restrict__ vol, long vol_bstride, GATHER_TABLE_PARAMS const float* __restrict__ coef,
    float* __restrict__ out, int D, int H, int W, int nbz, Steps st) {
  constexpr bool IN16 = (IO & 1) != 0, OUT16 = (IO & 2) != 0;
  constexpr u32 IREC = IN16 ? 32u : 64u, OREC = OUT16 ? 32u : 64u;
  const int n = blockIdx.z / nbz, bz = blockIdx.z - n * nbz;
  const int q = threadIdx.x & 3, vs = threadIdx.x >> 2;
  const int x = (blockIdx.x << 2) + (vs & 3), y = (blockIdx.y << 2) + ((vs >> 2) & 3), z = (bz << 2) + (vs >> 4);
  if (x >= W || y >= H || z >= D) return;
  const u32 nvox = (u32)D * (u32)H * (u32)W;
  // (vol_bstride counts ELEMENTS; the pointers are declared float*: byte arithmetic for the bf16 forms)
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)vol + GATHER_VOL_OFFSET * (IN16 ? 2 : 4)), 0, nvox * IREC, 0x00020000);
  const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)out + (long)n * nvox * OREC), 0, nvox * OREC, 0x00020000);
  const float* cf = coef + n * LF_MAP_COEFS;
  float gx, gy, gz, a, b, k;
  eval_grid<KIND>(cf, x, y, z, W, H, D, st, gx, gy, gz, a, b, k);
  const Tap32 t = make_tap32(gx, gy, gz, W, H, D, IREC);
  const u32 co = (u32)q * (IREC / 4u);
  const f32x4 v000 = ldrec_t<IN16>(rs, t.o000 + co), v001 = ldrec_t<IN16>(rs, t.o001 + co), v010 = ldrec_t<IN16>(rs, t.o010 + co), v011 = ldrec_t<IN16>(rs, t.o011 + co);
  const f32x4 v100 = ldrec_t<IN16>(rs, t.o100 + co), v101 = ldrec_t<IN16>(rs, t.o101 + co), v110 = ldrec_t<IN16>(rs, t.o110 + co), v111 = ldrec_t<IN16>(rs, t.o111 + co);
  const float wx1 = t.tx, wx0 = 1.f - t.tx, wy1 = t.ty, wy0 = 1.f - t.ty, wz1 = t.tz, wz0 = 1.f - t.tz;
  const float w000 = wx0 * wy0 * wz0, w001 = wx1 * wy0 * wz0, w010 = wx0 * wy1 * wz0, w011 = wx1 * wy1 * wz0;
  const float w100 = wx0 * wy0 * wz1, w101 = wx1 * wy0 * wz1, w110 = wx0 * wy1 * wz1, w111 = wx1 * wy1 * wz1;
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float acc = v000[e] * w000;
    // (inline asm keeps these as v_fmac_f32 with the weight as a plain operand)
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v001[e]), "v"(w001));
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v010[e]), "v"(w010));
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v011[e]), "v"(w011));
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v100[e]), "v"(w100));
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v101[e]), "v"(w101));
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v110[e]), "v"(w110));
    asm("v_fmac_f32 %0, %1, %2" : "+v"(acc) : "v"(v111[e]), "v"(w111));
    r[e] = acc;
  }
  if constexpr (OUT16)
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2_t, __builtin_convertvector(r, bf16x4r)), ro,
                                          (int)((u32)((z * H + y) * W + x) * 32u + (u32)q * 8u), 0, 2);
  else
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, r), ro, (int)((u32)((z * H + y) * W + x) * 64u + (u32)q * 16u), 0, 2);
}

// coefficient gradient, C == 16 (4 lanes per voxel, 64 voxels per block-iteration): block = 2^lg-voxel tile walked in
// 4x4x4 sub-tiles; thread (v = tid >> 2, q = tid & 3) keeps its position inside the sub-tile, the sub-tile index is
// wave-uniform
template <int MINW, int UNR>
__global__ void __launch_bounds__(256, MINW) GATHER_KERNEL(resample_bwd_coef_c16)(
    const float* __restrict__ gout, const float* __restrict__ vol, long vol_bstride, GATHER_TABLE_PARAMS
    const float* __restrict__ coef, float* __restrict__ partial, int nblk, int vpb, BwdTile bt,
    int D, int H, int W, Steps st) {
  const unsigned fb = xcd_contiguous(blockIdx.x, gridDim.x);
  const int n = fb / nblk, blk = fb - n * nblk;
  const float* cf = coef + n * LF_MAP_COEFS;
  const u32 rec = 64u;
  const u32 sample_bytes = (u32)D * (u32)H * (u32)W * rec;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(vol + GATHER_VOL_OFFSET), 0, sample_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)(gout + (long)n * D * H * W * 16), 0, sample_bytes, 0x00020000);
  const int tx = blk % bt.ntx, ty = (blk / bt.ntx) % bt.nty, tz = blk / (bt.ntx * bt.nty);
  const int q = threadIdx.x & 3, vs = threadIdx.x >> 2;          // vs = position inside a 4x4x4 sub-tile
  const int px = vs & 3, py = (vs >> 2) & 3, pz = vs >> 4;
  const int sbx = bt.lx - 2, sby = bt.ly - 2;
  // the 18 sums (hx, hy, hz) x (1, a, b, k, ak, bk) are split over the voxel's four lanes -- after the quad sums every
  // lane holds the same (hx, hy, hz) -- so a lane carries 6 accumulators instead of 18: lane q owns basis functions
  // 2q and 2q+1 (lane 3 idles)
  float acc[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[i] = 0.f;
  const int nsub = vpb >> 6;
  const u32 co = (u32)q * 16u;
  // UNR sub-tiles are in flight per iteration: the 9 loads of a voxel have nothing to overlap with inside one
  // sub-tile (a block walks its tile serially), so with one sub-tile at a time the kernel is bound by memory latency,
  // not by bandwidth (measured: 0.64 ms at 4 waves/SIMD; the loads alone need ~0.3 ms of the L1 path)
  for (int sub0 = 0; sub0 < nsub; sub0 += UNR) {                 // wave-uniform
    Tap32 t[UNR];
    float a[UNR], b[UNR], k[UNR];
    f32x4 go[UNR], v[UNR][8];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int sub = sub0 + u;
      const int x = (tx << bt.lx) + ((sub & ((1 << sbx) - 1)) << 2) + px;
      const int y = (ty << bt.ly) + (((sub >> sbx) & ((1 << sby) - 1)) << 2) + py;
      const int z = (tz << bt.lz) + ((sub >> (sbx + sby)) << 2) + pz;
      const bool live = sub < nsub && x < W && y < H && z < D;
      float gx, gy, gz;
      eval_grid<LF_MAP_O2C>(cf, live ? x : 0, live ? y : 0, live ? z : 0, W, H, D, st, gx, gy, gz, a[u], b[u], k[u]);
      t[u] = make_tap32(gx, gy, gz, W, H, D, rec);
      // out-of-tile lanes read offset 0xffffffff: outside the descriptor's range -> zeros, no branch
      const u32 dead = live ? 0u : 0xffffffffu;
      go[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
          rg, (int)(((u32)((z * H + y) * W + x) * rec + co) | dead), 0, 2));      // streamed once (nt)
      v[u][0] = ldrec(rs, (t[u].o000 + co) | dead); v[u][1] = ldrec(rs, (t[u].o001 + co) | dead);
      v[u][2] = ldrec(rs, (t[u].o010 + co) | dead); v[u][3] = ldrec(rs, (t[u].o011 + co) | dead);
      v[u][4] = ldrec(rs, (t[u].o100 + co) | dead); v[u][5] = ldrec(rs, (t[u].o101 + co) | dead);
      v[u][6] = ldrec(rs, (t[u].o110 + co) | dead); v[u][7] = ldrec(rs, (t[u].o111 + co) | dead);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      float p[8];
#pragma unroll
      for (int c8 = 0; c8 < 8; ++c8)
        p[c8] = quad_sum4((go[u][0] * v[u][c8][0] + go[u][1] * v[u][c8][1]) + (go[u][2] * v[u][c8][2] + go[u][3] * v[u][c8][3]));
      const float wx1 = t[u].tx, wx0 = 1.f - wx1, wy1 = t[u].ty, wy0 = 1.f - wy1, wz1 = t[u].tz, wz0 = 1.f - wz1;
      // p index = z*4 + y*2 + x
      const float dxv = (p[1] - p[0]) * (wy0 * wz0) + (p[3] - p[2]) * (wy1 * wz0) + (p[5] - p[4]) * (wy0 * wz1) + (p[7] - p[6]) * (wy1 * wz1);
      const float dyv = (p[2] - p[0]) * (wx0 * wz0) + (p[3] - p[1]) * (wx1 * wz0) + (p[6] - p[4]) * (wx0 * wz1) + (p[7] - p[5]) * (wx1 * wz1);
      const float dzv = (p[4] - p[0]) * (wx0 * wy0) + (p[5] - p[1]) * (wx1 * wy0) + (p[6] - p[2]) * (wx0 * wy1) + (p[7] - p[3]) * (wx1 * wy1);
      const float hx = dxv * t[u].mx, hy = dyv * t[u].my, hz = dzv * t[u].mz;
      const float B0 = q == 0 ? 1.f : (q == 1 ? b[u] : (q == 2 ? a[u] * k[u] : 0.f));
      const float B1 = q == 0 ? a[u] : (q == 1 ? k[u] : (q == 2 ? b[u] * k[u] : 0.f));
      acc[0] += hx * B0; acc[1] += hy * B0; acc[2] += hz * B0;
      acc[3] += hx * B1; acc[4] += hy * B1; acc[5] += hz * B1;
    }
  }
  // workgroup reduction in fp64: a thread's fp32 sum runs over its 64 voxels only; from there on (64 lanes x 4 waves,
  // then the blocks in the finish kernel) nothing is rounded until the final conversion -- the 18 sums cancel to a
  // small fraction of their terms' magnitude, so summation rounding would otherwise show in the camera gradients
  __shared__ double red[4][18];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = (double)acc[i];
#pragma unroll
    for (int o = 32; o >= 4; o >>= 1) s += __shfl_xor(s, o, 64);     // over the 16 lanes that share this q
    // lane q (0..2) of the first quad: basis 2q + i/3, component i%3 -> output index basis*3 + component
    if (lane < 3) red[wave][(2 * lane + i / 3) * 3 + (i % 3)] = s;
  }
  __syncthreads();
  if (threadIdx.x < 18) {
    const double s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    partial[((long)n * nblk + blk) * 18 + threadIdx.x] = (float)s;
  }
}

// coefficient gradient, C == 16, per-voxel arithmetic done ONCE per voxel (variant 6 of lf_set_tuning key 2).
// The kernel above spends most of its VALU issue on work that is identical in the four lanes sharing a voxel (map, taps,
// derivative algebra: ~3/4 of its ~200 instructions per lane and voxel), and VALU issue is what bounds it (DESIGN 4.4).
// Here a WAVE owns a 4x4x4 sub-tile and works on it in three phases that only meet through 3 KB of wave-private LDS:
//   A  lane = voxel (64 voxels per instruction): map, clip, corner offsets -> one 16-byte record per voxel in LDS
//      (fractions, clip masks and lattice coordinates stay in the lane's registers for phase C);
//   B  four passes of 16 voxels, lane = (voxel, channel quarter) as before: the gathers stay coalesced 64-byte records
//      through L1 (a lane-per-voxel gather would quadruple the L1 look-ups), contraction with the gradient, quad sums;
//      the 8 per-corner scalars of a voxel go back to LDS;
//   C  lane = voxel again: spatial derivatives, clip masks, the 18 basis sums.
// No workgroup barrier; waves walk their own sub-tiles.  Same value as the kernel above, different summation order.
template <int PIF, int MINW, bool GOPF = false>
__global__ void __launch_bounds__(256, MINW) GATHER_KERNEL(resample_bwd_coef_c16_dedup)(
    const float* __restrict__ gout, const float* __restrict__ vol, long vol_bstride, GATHER_TABLE_PARAMS
    const float* __restrict__ coef, float* __restrict__ partial, int nblk, int vpb, BwdTile bt,
    int D, int H, int W, Steps st) {
  __shared__ u32x4_t tapbuf[4][64];                             // per wave: o000 | dead, x / y / z corner strides (bytes, 0 if clamped)
  __shared__ float pbuf[4][64 * 8];                             // per wave: p[corner] of every voxel
  __shared__ double red[4][18];
  const unsigned fb = xcd_contiguous(blockIdx.x, gridDim.x);
  const int n = fb / nblk, blk = fb - n * nblk;
  const float* cf = coef + n * LF_MAP_COEFS;
  const u32 rec = 64u;
  const u32 sample_bytes = (u32)D * (u32)H * (u32)W * rec;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(vol + GATHER_VOL_OFFSET), 0, sample_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)(gout + (long)n * D * H * W * 16), 0, sample_bytes, 0x00020000);
  const int tx = blk % bt.ntx, ty = (blk / bt.ntx) % bt.nty, tz = blk / (bt.ntx * bt.nty);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int px = lane & 3, py = (lane >> 2) & 3, pz = lane >> 4;  // phase A / C: lane = voxel of the sub-tile
  const int q = lane & 3, vq = lane >> 2;                         // phase B: lane = (voxel 16 i + vq, quarter q)
  const int sbx = bt.lx - 2, sby = bt.ly - 2;
  const int nsub = vpb >> 6;
  const u32 co = (u32)q * 16u;
  float acc[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) acc[i] = 0.f;
  u32x4_t* tb = tapbuf[wave];
  float* pb = pbuf[wave];
  // GOPF: the gradient records (streamed from HBM: the longest latency of an iteration; the gathered volume sits in the
  // Infinity Cache) are requested one sub-tile ahead
  f32x4 gnext[4];
  auto load_go = [&](int sub_, f32x4 (&dst)[4]) {
    const int bx0 = (tx << bt.lx) + ((sub_ & ((1 << sbx) - 1)) << 2);
    const int by0 = (ty << bt.ly) + (((sub_ >> sbx) & ((1 << sby) - 1)) << 2);
    const int bz0 = (tz << bt.lz) + ((sub_ >> (sbx + sby)) << 2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int vi = 16 * i + vq;
      const int vx = bx0 + (vi & 3), vy = by0 + ((vi >> 2) & 3), vz = bz0 + (vi >> 4);
      const u32 dead = (sub_ < nsub && vx < W && vy < H && vz < D) ? 0u : 0xffffffffu;
      dst[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
          rg, (int)(((u32)((vz * H + vy) * W + vx) * rec + co) | dead), 0, 2));
    }
  };
  if (GOPF) load_go(wave, gnext);
  for (int sub = wave; sub < nsub; sub += 4) {                    // wave-uniform
    const int x0 = (tx << bt.lx) + ((sub & ((1 << sbx) - 1)) << 2);
    const int y0 = (ty << bt.ly) + (((sub >> sbx) & ((1 << sby) - 1)) << 2);
    const int z0 = (tz << bt.lz) + ((sub >> (sbx + sby)) << 2);
    f32x4 gcur[4];
    if (GOPF) {
#pragma unroll
      for (int i = 0; i < 4; ++i) gcur[i] = gnext[i];
      load_go(sub + 4, gnext);
    }
    // ---- A ----
    const int x = x0 + px, y = y0 + py, z = z0 + pz;
    const bool live = x < W && y < H && z < D;
    float gx, gy, gz, a, b, k;
    eval_grid<LF_MAP_O2C>(cf, live ? x : 0, live ? y : 0, live ? z : 0, W, H, D, st, gx, gy, gz, a, b, k);
    u32 ox, dx, oy, dy, oz, dz;
    float tx_, ty_, tz_, mx, my, mz;
    axis_tap(gx, W, rec, ox, dx, tx_, mx);
    axis_tap(gy, H, rec * (u32)W, oy, dy, ty_, my);
    axis_tap(gz, D, rec * (u32)W * (u32)H, oz, dz, tz_, mz);
    u32x4_t tr;
    tr[0] = live ? (oz + oy + ox) : 0xffffffffu;                  // dead voxels: every offset out of range -> zeros
    tr[1] = live ? dx : 0u; tr[2] = live ? dy : 0u; tr[3] = live ? dz : 0u;
    tb[lane] = tr;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // ---- B ---- (PIF passes in flight; a real loop, so that no more than PIF x 9 loads are live)
#pragma unroll 1
    for (int i0 = 0; i0 < 4; i0 += (GOPF ? 4 : PIF)) {
      if (GOPF) {
        // passes unrolled (static indices into gcur), PIF gathers in flight
#pragma unroll
        for (int j0 = 0; j0 < 4; j0 += PIF) {
          f32x4 v[PIF][8];
#pragma unroll
          for (int u = 0; u < PIF; ++u) {
            const u32x4_t t = tb[16 * (j0 + u) + vq];
            const u32 dead = t[0] == 0xffffffffu ? 0xffffffffu : 0u;
            const u32 b00 = (t[0] + co) | dead, b01 = b00 + t[2], b10 = b00 + t[3], b11 = b01 + t[3];
            v[u][0] = ldrec(rs, b00); v[u][1] = ldrec(rs, b00 + t[1]);
            v[u][2] = ldrec(rs, b01); v[u][3] = ldrec(rs, b01 + t[1]);
            v[u][4] = ldrec(rs, b10); v[u][5] = ldrec(rs, b10 + t[1]);
            v[u][6] = ldrec(rs, b11); v[u][7] = ldrec(rs, b11 + t[1]);
          }
#pragma unroll
          for (int u = 0; u < PIF; ++u) {
            const f32x4 go = gcur[j0 + u];
            float p[8];
#pragma unroll
            for (int c8 = 0; c8 < 8; ++c8)
              p[c8] = quad_sum4((go[0] * v[u][c8][0] + go[1] * v[u][c8][1]) + (go[2] * v[u][c8][2] + go[3] * v[u][c8][3]));
            const float e0 = q == 0 ? p[0] : (q == 1 ? p[2] : (q == 2 ? p[4] : p[6]));
            const float e1 = q == 0 ? p[1] : (q == 1 ? p[3] : (q == 2 ? p[5] : p[7]));
            *(float2*)(pb + (16 * (j0 + u) + vq) * 8 + 2 * q) = make_float2(e0, e1);
          }
          __builtin_amdgcn_sched_barrier(0);                      // keep at most PIF x 8 gathers live
        }
        continue;
      }
      f32x4 go[PIF], v[PIF][8];
#pragma unroll
      for (int u = 0; u < PIF; ++u) {
        const int vi = 16 * (i0 + u) + vq;                        // voxel of the sub-tile: same numbering as phase A's lane
        const u32x4_t t = tb[vi];
        const int vx = x0 + (vi & 3), vy = y0 + ((vi >> 2) & 3), vz = z0 + (vi >> 4);
        const u32 dead = t[0] == 0xffffffffu ? 0xffffffffu : 0u;
        go[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
            rg, (int)(((u32)((vz * H + vy) * W + vx) * rec + co) | dead), 0, 2));        // streamed once (nt)
        const u32 b00 = (t[0] + co) | dead, b01 = b00 + t[2], b10 = b00 + t[3], b11 = b01 + t[3];
        v[u][0] = ldrec(rs, b00); v[u][1] = ldrec(rs, b00 + t[1]);
        v[u][2] = ldrec(rs, b01); v[u][3] = ldrec(rs, b01 + t[1]);
        v[u][4] = ldrec(rs, b10); v[u][5] = ldrec(rs, b10 + t[1]);
        v[u][6] = ldrec(rs, b11); v[u][7] = ldrec(rs, b11 + t[1]);
      }
#pragma unroll
      for (int u = 0; u < PIF; ++u) {
        float p[8];
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8)
          p[c8] = quad_sum4((go[u][0] * v[u][c8][0] + go[u][1] * v[u][c8][1]) + (go[u][2] * v[u][c8][2] + go[u][3] * v[u][c8][3]));
        // every lane of a quad holds the voxel's 8 sums; lane q stores corners 2q, 2q+1 (one contiguous 32 bytes per voxel)
        const float e0 = q == 0 ? p[0] : (q == 1 ? p[2] : (q == 2 ? p[4] : p[6]));
        const float e1 = q == 0 ? p[1] : (q == 1 ? p[3] : (q == 2 ? p[5] : p[7]));
        *(float2*)(pb + (16 * (i0 + u) + vq) * 8 + 2 * q) = make_float2(e0, e1);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // ---- C ----
    {
      const f32x4 pa = *(const f32x4*)(pb + lane * 8), pc = *(const f32x4*)(pb + lane * 8 + 4);
      const float wx1 = tx_, wx0 = 1.f - wx1, wy1 = ty_, wy0 = 1.f - wy1, wz1 = tz_, wz0 = 1.f - wz1;
      // corner index = z*4 + y*2 + x: pa = corners 0..3 (z0), pc = corners 4..7 (z1)
      const float dxv = (pa[1] - pa[0]) * (wy0 * wz0) + (pa[3] - pa[2]) * (wy1 * wz0) + (pc[1] - pc[0]) * (wy0 * wz1) + (pc[3] - pc[2]) * (wy1 * wz1);
      const float dyv = (pa[2] - pa[0]) * (wx0 * wz0) + (pa[3] - pa[1]) * (wx1 * wz0) + (pc[2] - pc[0]) * (wx0 * wz1) + (pc[3] - pc[1]) * (wx1 * wz1);
      const float dzv = (pc[0] - pa[0]) * (wx0 * wy0) + (pc[1] - pa[1]) * (wx1 * wy0) + (pc[2] - pa[2]) * (wx0 * wy1) + (pc[3] - pa[3]) * (wx1 * wy1);
      const float hx = live ? dxv * mx : 0.f, hy = live ? dyv * my : 0.f, hz = live ? dzv * mz : 0.f;
      const float ak = a * k, bk = b * k;
      acc[0] += hx;       acc[1] += hy;       acc[2] += hz;
      acc[3] += hx * a;   acc[4] += hy * a;   acc[5] += hz * a;
      acc[6] += hx * b;   acc[7] += hy * b;   acc[8] += hz * b;
      acc[9] += hx * k;   acc[10] += hy * k;  acc[11] += hz * k;
      acc[12] += hx * ak; acc[13] += hy * ak; acc[14] += hz * ak;
      acc[15] += hx * bk; acc[16] += hy * bk; acc[17] += hz * bk;
    }
    asm volatile("" ::: "memory");                               // the next sub-tile's phase A overwrites tb after phase B's reads (program order)
  }
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    double s = (double)acc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) red[wave][i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 18) {
    const double s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    partial[((long)n * nblk + blk) * 18 + threadIdx.x] = (float)s;
  }
}
