// The backward-fused factor projection of conv3d_c16_wino_body (conv_wino.hip, FUSE == 2; WinoProj in wino16_compute.h says
// what it computes; an experimental entry point, lf_conv3d_c16_wino_projbwd): the halo of the data-gradient convolution is
// COMPUTED from the projection's gradient instead of fetched.  Included as text by the body in four sections:
//
//     template <...> void conv3d_c16_wino_body(... x, D, H, W, slope, pj ...) {
//       buf; lane, fa, n, kg; nvox, sample_bytes; the first tile (cx, cy, cz, cn)
//     #define WINO16_PROJBWD_STATE
//     #include "wino16_projbwd.inc"  // every form (unused state folds away): pj_lo / pj_pix / pj_b / pj_aw / pj_yp / pj_nr,
//                                    // pj_last_ok, pj_column(bx, by, bn), pj_issue(z0, bn), pj_issue_hot(z0, bn),
//                                    // pj_finish(half_base), pj_slide()
//       if constexpr (FUSE == 2) {
//     #define WINO16_PROJBWD_PRIME
//     #include "wino16_projbwd.inc"  // pj_lo; the first tile's column and its four halo planes formed in LDS
//       } else { halo_fetch; halo_commit; }
//       lds_barrier();
//       for (int t = t_begin; t < t_end; ++t) {
//         ... MFMA phase, barrier, (nx, ny, nz, nn), exchange, epilogue, previous-layer backward, stores ...
//         if constexpr (FUSE == 2) {
//     #define WINO16_PROJBWD_NEXT
//     #include "wino16_projbwd.inc"  // reads t, t_end, nz, nn: the upper half slid down and the next tile's two new planes
//         }                          // formed, in a phase of its own behind the stores
//         lds_barrier();  (cx, cy, cz, cn) = (nx, ny, nz, nn);
//         if constexpr (FUSE == 2) {
//     #define WINO16_PROJBWD_COLUMN
//     #include "wino16_projbwd.inc"  // reads t, t_end, nz and the stepped (cx, cy, cn): at the bottom of a new column its
//         }                          // pixels and all four planes, and a second barrier
//       }
//     }
//
// A section un-defines its own selector.  No pj_ name is used by the body outside these sections.  The sharing is textual for
// the reason ring_walk.inc gives: this is the one form at the register limit (254 of 256 VGPRs, no spills), and the position
// of each section among the body's statements is part of what keeps it there.  WINO_PJ_ABL (wino16_math.h) cuts pieces out
// for the A/B tools.

#if defined(WINO16_PROJBWD_STATE)
#undef WINO16_PROJBWD_STATE
  // ---- FUSE = 2: the halo is COMPUTED, not fetched.  A z plane of the halo (180 voxel slots) is cut into 12 groups of 16
  // consecutive slots (the last one holds 4); wave fa owns groups fa, fa + 4, fa + 8 of both planes of a half: lane =
  // kg * 16 + n is (channel quarter kg, slot 16 * group + n) -- the D-operand order of the MFMA that forms the record and
  // the order of lf_conv1x1_bwd_data's epilogue.  Every LDS byte of a group region (1 KiB per plane) is read (slide) and
  // written by its owner wave only, so the slide needs no barrier of its own. ----
  int pj_lo[3];                                                // LDS byte offset of (slot, quarter) in plane 0 of a half
  int pj_pix[3];                                               // per column: pixel index gy * W + gx of the slot, -1 = outside
  f32x4 pj_b[3];                                               // per tile: B operands = gp(pixel, 4 kg .. 4 kg + 3)
  f32x4 pj_aw[2], pj_yp[6];
  float pj_nr[6];
  const bool pj_last_ok = n < 4;                               // group 11 = slots 176 .. 179
  auto pj_column = [&](int bx, int by, int bn) {
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const int sl = (fa + 4 * it) * 16 + n;
      const int ly = sl / HXw, rem = sl - ly * HXw;
      const int xl = rem / 9, xa = rem - xl * 9;
      const int gy = by * TYw - 1 + ly, gx = bx * TXw - 1 + 2 * xa + xl;
      const bool ok = sl < HYw * HXw && gy >= 0 && gy < H && gx >= 0 && gx < W;
      pj_pix[it] = ok ? gy * W + gx : -1;
    }
  };
  // the loads of a half in two parts: the HBM streams (activation records, norms) are requested early, under the
  // exchange / epilogue arithmetic; the L2-resident operands (the pixels' gradient records, the planes' weight slices)
  // late, behind that arithmetic, when its registers are free
  auto pj_issue_hot = [&](int z0, int bn) {
#pragma unroll
    for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(pj_pix[i]));
    const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc((void*)(pj.gp + (long)bn * H * W * 16), 0,
                                                                        (unsigned)(H * W * 64), 0x00020000);
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rg, pj_pix[it] >= 0 ? pj_pix[it] * 64 + kg * 16 : 0x7fffffff, 0, 0);
      pj_b[it] = (f32x4){__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3])};
    }
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      const int gz = z0 + pl;                                    // wave-uniform
      const bool pok = gz >= 0 && gz < D;
      pj_aw[pl] = *(const f32x4*)(pj.wA + ((long)(pok ? gz : 0) * 64 + lane) * 4);
      if (!pok) pj_aw[pl] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };
  auto pj_issue = [&](int z0, int bn) {
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (long)bn * nvox * 16), 0, sample_bytes, 0x00020000);
    const bool has_norm = pj.xnorm != nullptr;                   // (wave-uniform)
    const __amdgpu_buffer_rsrc_t rn = __builtin_amdgcn_make_buffer_rsrc((void*)(has_norm ? pj.xnorm + (long)bn * nvox : x), 0,
                                                                        has_norm ? (unsigned)(nvox * 4) : 0u, 0x00020000);
    // (the pixels' gradient records are re-read per tile -- 11.5 KB per workgroup, L1 / L2 hits -- rather than held in 12
    // registers across the MFMA phase, where the kernel has none to spare)
#pragma unroll
    for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(pj_pix[i]));
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      const int gz = z0 + pl;                                    // wave-uniform
      const bool pok = gz >= 0 && gz < D;
#pragma unroll
      for (int it = 0; it < 3; ++it) {
        const bool ok = pok && pj_pix[it] >= 0 && !(WINO_PJ_ABL & 1);
        const int vox = gz * H * W + pj_pix[it];
        const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(ra, ok ? vox * 64 + kg * 16 : 0x7fffffff, 0, 0);
        pj_yp[pl * 3 + it] = (f32x4){__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[3])};
        const float nv = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rn, (ok && has_norm) ? vox * 4 : 0x7fffffff, 0, 0));
        pj_nr[pl * 3 + it] = (ok && has_norm) ? nv : 1.f;
      }
    }
  };
  auto pj_finish = [&](int half_base) {
#pragma unroll
    for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(pj_lo[i]));
#pragma unroll
   for (int pl0 = 0; pl0 < 2; ++pl0) {
    f32x4 g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr ((WINO_PJ_ABL & 2) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        g[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(pj_aw[pl0][i], pj_b[k][i], g[k], 0, 0, 0);
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = pj_b[k] + pj_aw[pl0];
    }
#pragma unroll
    for (int k = pl0 * 3; k < pl0 * 3 + 3; ++k) {
      const f32x4 yp = pj_yp[k];
      f32x4 v = g[k - pl0 * 3] * pj.he;
      if ((pj.flags & LF_EPI_PIXELNORM) && !(WINO_PJ_ABL & 2)) {
        float dot = v[0] * yp[0] + v[1] * yp[1] + v[2] * yp[2] + v[3] * yp[3];
        dot += __shfl_xor(dot, 16, 64);
        dot += __shfl_xor(dot, 32, 64);
        dot *= (1.f / 16.f);
        const float rinv = fast_rcp(pj_nr[k]);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (v[e] - yp[e] * dot) * rinv;
      }
      if (pj.flags & LF_EPI_LRELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = yp[e] > 0.f ? v[e] : v[e] * slope;
      }
      const int pl = k / 3, it = k % 3;
      if (it < 2 || fa < 3 || pj_last_ok)
        *(f32x4*)(buf + half_base + pl * (HYw * HXw * 64) + (pj_lo[it] ^ (pl * 32))) = v;
    }
   }
  };
  // slide: the upper half's group regions of this wave -> the lower half, LDS -> LDS through three registers at a time (the
  // buffer is free once the tile's first barrier has passed, and the regions are this wave's own)
  auto pj_slide = [&]() {
    int sbase = fa * 1024 + lane * 16;
    asm volatile("" : "+v"(sbase));
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
      u32x4 tmp[3];
#pragma unroll
      for (int it = 0; it < 3; ++it) tmp[it] = *(const u32x4*)(buf + HALFBw + pl * (HYw * HXw * 64) + it * 4096 + sbase);
#pragma unroll
      for (int it = 0; it < 3; ++it)
        if (it < 2 || fa < 3 || lane < 16) *(u32x4*)(buf + pl * (HYw * HXw * 64) + it * 4096 + sbase) = tmp[it];
    }
  };

#elif defined(WINO16_PROJBWD_PRIME)
#undef WINO16_PROJBWD_PRIME
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const int sl = (fa + 4 * it) * 16 + n;
      const int ly = sl / HXw;
      const int q0 = kg ^ ((((sl >> 2) & 1) << 1) | ((ly >> 1) & 1));
      pj_lo[it] = sl * 64 + q0 * 16;
    }
    pj_column(cx, cy, cn);
    pj_issue(cz * TZw - 1, cn);
    pj_issue_hot(cz * TZw - 1, cn);
    pj_finish(0);
    pj_issue(cz * TZw + 1, cn);
    pj_issue_hot(cz * TZw + 1, cn);
    pj_finish(HALFBw);

#elif defined(WINO16_PROJBWD_NEXT)
#undef WINO16_PROJBWD_NEXT
      // the next tile's two new planes, in a phase of their own behind this tile's stores: the kernel sits at the register
      // limit (254 of 256, no spills) and every placement that keeps the plane loads in flight under the exchange /
      // epilogue arithmetic spills 11 - 115 registers into the MFMA phase (measured, round 4); here nothing else is
      // live.  The loads' latency is exposed to this wave -- the SIMD's other wave (the CU's second workgroup) issues
      // its MFMAs meanwhile, which is what the two-workgroup organisation is for.
      __builtin_amdgcn_sched_barrier(0);
      if (t + 1 < t_end && nz != 0) {
        if constexpr ((WINO_PJ_ABL & 4) == 0) pj_slide();
        pj_issue(nz * TZw + 1, nn);
        pj_issue_hot(nz * TZw + 1, nn);
        __builtin_amdgcn_sched_barrier(0);
        pj_finish(HALFBw);
      }
      __builtin_amdgcn_sched_barrier(0);

#elif defined(WINO16_PROJBWD_COLUMN)
#undef WINO16_PROJBWD_COLUMN
      if (t + 1 < t_end && nz == 0) {                            // bottom of a new column: its pixels, all four halo planes
        pj_column(cx, cy, cn);
        pj_issue(-1, cn);
        pj_issue_hot(-1, cn);
        pj_finish(0);
        pj_issue(1, cn);
        pj_issue_hot(1, cn);
        pj_finish(HALFBw);
        lds_barrier();
      }

#else
#error "wino16_projbwd.inc: define WINO16_PROJBWD_STATE, _PRIME, _NEXT or _COLUMN"
#endif
