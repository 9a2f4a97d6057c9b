// The skeleton of the fused wide Winograd GEMM kernels -- wino_fused_kernel (wino_fused.hip: fp32 MFMA) and f16x3_gemm_body
// (wino_fused_f16x3.hip: three f16 MFMAs per product) -- written once and included by both, in three sections:
//
//     template <int DIMS, int WM, int WN, int BA, int BB> ... (V, U2, bias, y, T, tz, ty, tx, D, H, W, Cout, CoutP, flags,
//                                                              partial, ysize, ...) {
//     #define WINO_RING_SETUP
//     #include "wino_ring.inc"       // workgroup / lane roles, XCD order, LDS-DMA piece table, issue cursor (issue_piece),
//                                    // operand address tables rdA / rdB, accumulators Y / acc, the first NSTAGE-1 stages
//       for (int s = 0; s < S; ++s) {
//         wino_ring::wait<PPW>(min(NSTAGE - 2, S - 1 - s));
//         const bool more = issued < S;
//         const unsigned char* base = smem + (s % NSTAGE) * STAGE_BYTES;
//         ... the file's product step: LDS rows at base + rdA / rdB -> MFMAs into acc, issue_piece(q) in its issue slots ...
//     #define WINO_RING_FOLD
//     #include "wino_ring.inc"       // after the last k-chunk of a frequency: Y[o] += A^T[o][f] acc, acc = 0
//       }
//       Epilogue epi{...};
//     #define WINO_RING_STORE
//     #include "wino_ring.inc"       // tile decode, guards, LF_OUT_DEPTH_INNER, frequency-split partials, epi(Y, bias, tile exp)
//     }
//
// under two macros that stay defined for all three sections:
//   WINO_RING_K        row length of V and U2 in 4-byte units (Cin floats; CinP: hi + lo f16 records)
//   WINO_RING_RAGGED   1: rows are not padded to KC, the last k-chunk of a frequency may be ragged (fp32); 0: whole records
// A section un-defines its own selector.  The value helpers (KC, NSTAGE, lds_chunk, at_coef, wait) are in wino_ring.h.
//
// The sharing is textual for the reason resample_gather.inc gives: every C++ route that was tried moved the device code of
// the existing kernels (tools/resample_isa_diff.py --src wino_fused.hip: the XCD order alone as a __forceinline__ function
// returning through references re-ordered 37 instructions in each of the 8 fp32 kernels; the operand tables, the fold and the
// store loop as functions over array references changed 20-4900 lines per kernel, the store loop adding 11-33 instructions;
// one struct holding the whole state added 19-62).  As text, all symbols are identical to the two hand-written copies this
// file replaced (profiles/wide_wino_shared_isa.txt).

#if defined(WINO_RING_SETUP)
#undef WINO_RING_SETUP
  constexpr int F = DIMS == 3 ? 64 : 16;
  constexpr int NO = DIMS == 3 ? 8 : 4;                          // outputs per tile
  constexpr int NTc = WM * BA * 16, MTc = WN * BB * 16, NW = WM * WN;
  constexpr int A_BYTES = NTc * 128, STAGE_BYTES = (NTc + MTc) * 128;
  constexpr int PA = NTc / 8, PB = MTc / 8;                      // 1 KiB DMA pieces of the A / B chunk of a stage
  constexpr int PPW = (PA + PB) / NW;                            // pieces per wave and stage
  static_assert((PA + PB) % NW == 0, "pieces must split evenly over the waves");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = w / WN, wc = w % WN;
  const int lr = lane & 15, kg = lane >> 4;
  // XCD-aware order: the workgroups of ONE tile block -- one per output-channel block, all reading the same slice of V --
  // are dispatched x-fastest, i.e. gridDim.x dispatches apart, and each re-read V from HBM (9.8 GB per 128-render launch of the
  // released architecture against 4.8 GB of V + y).  Dispatch L goes to XCD L % 8: re-numbered so that the channel blocks of a tile
  // block follow each other ON ONE XCD, they stream V through that XCD's L2 together.
  int bxi = blockIdx.x, byi = blockIdx.y;
  if (gridDim.y > 1 && (gridDim.x & 7) == 0) {
    const unsigned L = blockIdx.x + gridDim.x * blockIdx.y, slot = L >> 3;
    byi = (int)(slot % gridDim.y);
    bxi = (int)((slot / gridDim.y) * 8 + (L & 7));
  }
  const long m0 = (long)bxi * MTc;                               // first tile of this workgroup
  const int n0 = byi * NTc;                                      // first output channel

  // ---- global -> LDS staging by LDS-DMA (buffer_load_dwordx4 ... lds): a wave-instruction deposits 64 x 16 B = 1 KiB
  // linearly at a wave-uniform LDS address, so the swizzle is applied on the GLOBAL side: the lane that lands on
  // LDS position pos = piece*64 + lane (row r = pos >> 3, slot pos & 7) fetches logical chunk c = slot ^ ((r >> 1) & 7)
  // of that row.  A stage = PA pieces of A + PB of B; wave w issues pieces w*PPW .. +PPW-1 of the concatenated list.
  // No staging registers, no ds_write; out-of-range chunks (k >= row length, tile >= T, cout >= CoutP) get an out-of-range
  // offset and the DMA writes zeros. ----
#if WINO_RING_RAGGED
  const u32 slabV = (u32)((long)T * WINO_RING_K * 4 <= 0xffffffffL ? (long)T * WINO_RING_K * 4 : 0xffffffffL);
#else
  const u32 slabV = (u32)((long)T * WINO_RING_K * 4);
#endif
  const u32 slabU = (u32)((long)CoutP * WINO_RING_K * 4);
#if WINO_RING_RAGGED
  int voff[PPW], kch[PPW], ldso[PPW];
#else
  int voff[PPW], ldso[PPW];
#endif
  bool isA[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int p = w * PPW + i;                                   // wave-uniform
    isA[i] = p < PA;
    const int piece = isA[i] ? p : p - PA;
    const int pos = piece * 64 + lane, r = pos >> 3, c = (pos & 7) ^ ((r >> 1) & 7);
#if WINO_RING_RAGGED
    kch[i] = c * 4;
#endif
    if (isA[i]) {
      const long off = (long)(n0 + r) * WINO_RING_K * 4 + c * 16;        // U2[f][n0 + r][k0 + 4c ..]
      voff[i] = off < (long)slabU ? (int)(u32)off : 0x7fffffff;
      ldso[i] = piece * 1024;
    } else {
      const long row = m0 + r;
      voff[i] = row < T ? (int)((u32)row * (u32)WINO_RING_K * 4u + (u32)c * 16u) : 0x7fffffff;
      ldso[i] = A_BYTES + piece * 1024;
    }
  }
#if WINO_RING_RAGGED
  const int nk = (WINO_RING_K + KC - 1) / KC;
#else
  const int nk = WINO_RING_K / KC;
#endif
  // frequency split (small problems: few tile / channel blocks): workgroup z handles frequencies
  // [z * F / gridDim.z, (z + 1) * F / gridDim.z) and writes its un-scaled partial outputs; lf's finish kernel adds the
  // partials in a fixed order and applies the epilogue
  const int fper = F / gridDim.z, f_first = blockIdx.z * fper;
  const int S = fper * nk;
  // The issue side keeps its own cursor (frequency, k-chunk, ring slot) three stages ahead of the compute side, so a
  // piece costs one LDS-DMA instruction and no address arithmetic: the per-lane byte offset inside the frequency slab
  // is a loop invariant (voffset), the k-chunk advances through the instruction's SCALAR offset, and the two buffer
  // descriptors are rebuilt only when the cursor enters the next frequency.  (First version: stage index -> (f, k) by
  // division and fresh descriptors per piece = 4.6 scalar instructions per MFMA, MFMA pipe 54 % busy.)
  // (the slab strides in two spellings, floats and bytes, as the two kernels had them: the compiler emits different code for each)
#if WINO_RING_RAGGED
  const long strideU = (long)CoutP * WINO_RING_K, strideV = (long)T * WINO_RING_K;
  const float* pU = U2 + (long)f_first * strideU;
  const float* pV = V + (long)f_first * strideV;
#else
  const long strideU = (long)slabU, strideV = (long)T * WINO_RING_K * 4;
  const unsigned char* pU = (const unsigned char*)U2 + (long)f_first * strideU;
  const unsigned char* pV = (const unsigned char*)V + (long)f_first * strideV;
#endif
  __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)pU, 0, slabU, 0x00020000);
  __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)pV, 0, slabV, 0x00020000);
  int ik = 0, islot = 0, issued = 0;                             // cursor: k-chunk of the stage being issued, its ring slot
#if WINO_RING_RAGGED
  const bool ktail = (WINO_RING_K % KC) != 0;
#endif
  // piece q (0 .. PPW-1) of the cursor's stage for this wave
  auto issue_piece = [&](int q) {
    unsigned char* slot = smem + islot * STAGE_BYTES;
    const int k0b = ik * KC * 4;                                 // scalar byte offset of the k-chunk
    int vo = voff[q];
#if WINO_RING_RAGGED
    if (ktail && ik == nk - 1) vo = (ik * KC + kch[q] < WINO_RING_K) ? vo : 0x7fffffff;   // ragged last chunk: lanes beyond the row read zeros
#endif
    if (isA[q])
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ru, (__attribute__((address_space(3))) void*)(slot + ldso[q]), 16, vo, k0b, 0, 0);
    else
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (__attribute__((address_space(3))) void*)(slot + ldso[q]), 16, vo, k0b, 0, 0);
    if (q == PPW - 1) {                                          // stage complete: advance the cursor
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

  // ---- MFMA operand addressing: row of this lane in A (cout) and B (tile) for the 16-row blocks of the wave ----
  int rdA[BA][2], rdB[BB][2];                                    // [row block][j]: chunk j * 4 + kg of the lane's row
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

  // ring of NSTAGE stages: stages s+1 .. s+NSTAGE-1 are in flight while stage s feeds the MFMAs
  for (int s0 = 0; s0 < NSTAGE - 1 && s0 < S; ++s0)
#pragma unroll
    for (int q = 0; q < PPW; ++q) issue_piece(q);
  int kc = 0, f = f_first;

#elif defined(WINO_RING_FOLD)
#undef WINO_RING_FOLD
    if (++kc == nk) {
      // frequency f complete: fold it into the outputs, Y[o] += A^T[o][f] * M[f]
      kc = 0;
      const int fc = f & 3, fb_ = (f >> 2) & 3, fa_ = (f >> 4) & 3;      // x, y, z frequency (DIMS == 2: fa_ unused)
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        float cf = at_coef(o & 1, fc) * at_coef((o >> 1) & 1, fb_);
        if (DIMS == 3) cf *= at_coef((o >> 2) & 1, fa_);
        if (cf != 0.f) {                                         // wave-uniform
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

#elif defined(WINO_RING_STORE)
#undef WINO_RING_STORE
  // ---- the lane holds couts n0 + wr*BA*16 + a*16 + kg*4 .. +3 of tile column lr; epi.tile_exp(tile) is asked once per tile,
  // epi(Y, bias quad, that value) gives the four values to store ----
#pragma unroll
  for (int b = 0; b < BB; ++b) {
    const long tile = m0 + wc * (BB * 16) + b * 16 + lr;
    if (tile >= T) continue;
    long r = tile;
    const int bx = (int)(r % tx); r /= tx;
    const int by = (int)(r % ty); r /= ty;
    const int bz = DIMS == 3 ? (int)(r % tz) : 0;
    const long n = DIMS == 3 ? r / tz : r;
    const int etile = epi.tile_exp(tile);
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
        // LF_OUT_DEPTH_INNER: y as [N][H][W][D][Cout] -- the factor projection then reads a pixel's D x Cout column as ONE row
        const long vox = (flags & LF_OUT_DEPTH_INNER) ? ((n * H + gy) * W + gx) * D + gz : ((n * D + gz) * H + gy) * W + gx;
        if (partial != nullptr) {                                // frequency-split launch: raw partial sums
          *(f32x4*)(partial + (long)blockIdx.z * ysize + vox * Cout + co) = Y[o][a][b];
          continue;
        }
        *(f32x4*)(y + vox * Cout + co) = epi(Y[o][a][b], bv, etile);
      }
    }
  }

#else
#error "wino_ring.inc: define WINO_RING_SETUP, WINO_RING_FOLD or WINO_RING_STORE"
#endif
