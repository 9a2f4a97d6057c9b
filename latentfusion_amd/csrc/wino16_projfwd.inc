// The forward-fused factor projection of conv3d_c16_wino_body (conv_wino.hip, FUSE == 1; WinoProj in wino16_compute.h says
// what it computes): a product path, lf_conv3d_c16_wino_projfwd.  Included as text by the body in two sections:
//
//     template <...> void conv3d_c16_wino_body(... D, H, W, tiles_z, slope, eps, pj ...) {
//       px; lane, fa
//     #define WINO16_PROJFWD_ACC
//     #include "wino16_projfwd.inc"  // every form (unused, it folds away): pacc[2], the wave's projection sums of the column
//       for (int t = t_begin; t < t_end; ++t) {
//         ... MFMA phase, barrier, exchange, epilogue, stores: v[4] (finished records), okv[4], (bx, by, bz, tt) ...
//         if constexpr (FUSE == 1) {
//     #define WINO16_PROJFWD_TILE
//     #include "wino16_projfwd.inc"  // v[] -> B-operand order through the wave's consumed exchange slices, 16 MFMAs into
//         }                          // pacc; at the top of a column (bz == tiles_z - 1) the projection's own epilogue, the
//         lds_barrier();             // stores of pj.zp / pj.pnorm, pacc = 0
//       }
//     }
//
// A section un-defines its own selector.  The sharing is textual: as a __forceinline__ function over references the per-tile
// section changed the device code of all four projfwd kernels (DESIGN.md, next to the ring convolutions' paragraph).

#if defined(WINO16_PROJFWD_ACC)
#undef WINO16_PROJFWD_ACC
  // FUSE = 1: per-wave projection accumulators (2 output rows x 16 x x 16 cout), summed up the column of tiles
  f32x4 pacc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};

#elif defined(WINO16_PROJFWD_TILE)
#undef WINO16_PROJFWD_TILE
      // finished records -> B-operand order through this wave's own (consumed) slices of the exchange region
      __builtin_amdgcn_sched_barrier(0);
      int lop = lane;
      if constexpr (!(OPT & 1)) asm volatile("" : "+v"(lop));     // (opaque: or per-lane 64-bit addresses are hoisted out of the loop and spilled)
      const int trn = lop & 15, trk = lop >> 4;
      f32x4 pw_a[2];                                             // L2-resident weight slices of the tile's two planes
#pragma unroll
      for (int zo = 0; zo < 2; ++zo)
        pw_a[zo] = *(const f32x4*)((const char*)pj.wA + (long)min(bz * TZw + zo, D - 1) * 1024 + (unsigned)(lop * 16));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const f32x4 vz = okv[k] ? v[k] : (f32x4){0.f, 0.f, 0.f, 0.f};
        *(f32x4*)(px + (k >> 1) * 8192 + fa * 2048 + (k & 1) * 1024 + (lop >> 2) * 64 + (((lop & 3) ^ tr_swz(lop >> 2)) * 16)) = vz;
      }
      f32x4 bq[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        bq[k] = *(const f32x4*)(px + (k >> 1) * 8192 + fa * 2048 + (k & 1) * 1024 + trn * 64 + ((trk ^ tr_swz(trn)) * 16));
#pragma unroll
      for (int zo = 0; zo < 2; ++zo)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            pacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(pw_a[zo][i], bq[j * 2 + zo][i], pacc[j], 0, 0, 0);
      if (bz == tiles_z - 1) {                                   // top of the column: the projection's own epilogue
        f32x4 pb = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (pj.bias != nullptr) pb = *(const f32x4*)(pj.bias + trk * 4);
        const int pgx = bx * TXw + trn;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int pgy = by * TYw + 2 * fa + j;
          float ss = 0.f;
          f32x4 u;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float q = pacc[j][e] * pj.he + pb[e];
            if (pj.flags & LF_EPI_LRELU) q = lf_lrelu(q, slope);
            u[e] = q;
            ss += q * q;
          }
          float r = 1.f, rinv = 1.f;
          if (pj.flags & LF_EPI_PIXELNORM) {
            ss += __shfl_xor(ss, 16, 64);
            ss += __shfl_xor(ss, 32, 64);
            r = sqrtf(ss / 16.f + eps);
            rinv = 1.0f / r;
          }
          if (pgy < H && pgx < W) {
            const long pix = ((long)tt * H + pgy) * W + pgx;
            if (pj.flags & LF_EPI_PIXELNORM) { u[0] *= rinv; u[1] *= rinv; u[2] *= rinv; u[3] *= rinv; }
            *(f32x4*)(pj.zp + pix * 16 + trk * 4) = u;
            if ((pj.flags & LF_EPI_PIXELNORM) && pj.pnorm != nullptr && trk == 0) pj.pnorm[pix] = r;
          }
          pacc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      }

#else
#error "wino16_projfwd.inc: define WINO16_PROJFWD_ACC or WINO16_PROJFWD_TILE"
#endif
