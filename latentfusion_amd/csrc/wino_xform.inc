// The F(2,3) input transform of one channel quad of a 4 x 4 (x z pair) patch, written once and included by the four input
// transform kernels (wino_gemm.hip: wino3d_input_kernel, wino2d_input_kernel; wino_fused_f16x3.hip: wino3d_input_f16x3_kernel
// and wino2d_xform4 for wino2d_input_f16x3_kernel), inside their loop over channel quads, under three macros:
//   WINO_XFORM_DIMS   2: patch at (y0, x0) of xs [H][W][C];  3: at (y0, x0) of the planes za, zb of xs [D][H][W][C], combined
//                     as x[za] + sb x[zb] (the z transform of the kernel's z-frequency; za_ok / zb_ok: the plane exists)
//   WINO_XFORM_LIVE   false: the quad reads zeros (channel padding of a record); `true` where there is no padding
//   WINO_XFORM_CH     first channel of the quad
// It loads the patch with zero padding, applies the row transform d0-d2, d1+d2, d2-d1, d1-d3 and leaves f32x4 vx[dy][c];
// frequency (y b, x c) is then WINO_XFORM_COL(vx, b, c), the same transform down the columns.
// Textual like wino_ring.inc and for the same reason: as __forceinline__ functions filling v[16] (through a d[4][4] patch) all
// four kernels changed, three of them one instruction longer (tools/resample_isa_diff.py --src wino_gemm.hip wino_fused_f16x3.hip).
    f32x4 vx[4][4];
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
      const int yy = y0 + dy;
#if WINO_XFORM_DIMS == 3
      const bool y_ok = WINO_XFORM_LIVE && (unsigned)yy < (unsigned)H;
#endif
      f32x4 d[4];
#pragma unroll
      for (int dx = 0; dx < 4; ++dx) {
        const int xx = x0 + dx;
#if WINO_XFORM_DIMS == 3
        const bool ok = y_ok && (unsigned)xx < (unsigned)W;
        f32x4 va = (f32x4){0.f, 0.f, 0.f, 0.f}, vb = va;
        if (ok && za_ok) va = *(const f32x4*)(xs + (((long)za * H + yy) * W + xx) * C + WINO_XFORM_CH);
        if (ok && zb_ok) vb = *(const f32x4*)(xs + (((long)zb * H + yy) * W + xx) * C + WINO_XFORM_CH);
        d[dx] = va + vb * sb;
#else
        d[dx] = (WINO_XFORM_LIVE && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
                    ? *(const f32x4*)(xs + ((long)yy * W + xx) * C + WINO_XFORM_CH)
                    : (f32x4){0.f, 0.f, 0.f, 0.f};
#endif
      }
      vx[dy][0] = d[0] - d[2];
      vx[dy][1] = d[1] + d[2];
      vx[dy][2] = d[2] - d[1];
      vx[dy][3] = d[1] - d[3];
    }
#undef WINO_XFORM_DIMS
#undef WINO_XFORM_LIVE
#undef WINO_XFORM_CH
