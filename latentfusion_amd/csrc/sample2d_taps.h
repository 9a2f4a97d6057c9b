// Bilinear taps of F.grid_sample(align_corners=False) on a planar H x W image, shared by the grid sampler
// (sample2d.hip) and the fused IBR reprojection (ibr.hip): pixel coordinate -> the four taps, their validity
// under zeros padding and the fractional offsets.  A non-finite coordinate takes whatever this yields (the
// float -> int conversion of NaN is 0, of +-inf the saturated int), identically in both files.
#pragma once
#include "lf_common.h"

// grid value in [-1, 1] -> pixel coordinate (align_corners=False)
__device__ __forceinline__ float lf_unnorm2d(float g, int size) { return ((g + 1.f) * (float)size - 1.f) * 0.5f; }

struct lf_taps2d {
  int x0, y0, x1, y1;
  float tx, ty;
  bool vx0, vx1, vy0, vy1;
};

// taps from the floor of the pixel coordinate (a float holding an integer, NaN or +-inf) and the offsets from it
__device__ __forceinline__ lf_taps2d lf_taps_from_floor(float fx, float fy, float tx, float ty, int H, int W) {
  lf_taps2d t;
  t.x0 = (int)fx; t.y0 = (int)fy; t.x1 = t.x0 + 1; t.y1 = t.y0 + 1;
  t.tx = tx; t.ty = ty;
  t.vx0 = (unsigned)t.x0 < (unsigned)W; t.vx1 = (unsigned)t.x1 < (unsigned)W;
  t.vy0 = (unsigned)t.y0 < (unsigned)H; t.vy1 = (unsigned)t.y1 < (unsigned)H;
  return t;
}

__device__ __forceinline__ lf_taps2d lf_bilinear_taps(float px, float py, int H, int W) {
  const float fx = floorf(px), fy = floorf(py);
  return lf_taps_from_floor(fx, fy, px - fx, py - fy, H, W);
}

struct lf_weights2d { float w00, w01, w10, w11; };

__device__ __forceinline__ lf_weights2d lf_bilinear_weights(const lf_taps2d& t) {
  return {(1.f - t.tx) * (1.f - t.ty), t.tx * (1.f - t.ty), (1.f - t.tx) * t.ty, t.tx * t.ty};
}

// weighted sum of the in-frame taps of one plane (an out-of-frame tap adds nothing, whatever its weight)
__device__ __forceinline__ float lf_bilinear_gather(const float* __restrict__ s, int W, const lf_taps2d& t,
                                                    const lf_weights2d& w) {
  float v = 0.f;
  if (t.vy0 && t.vx0) v += s[t.y0 * W + t.x0] * w.w00;
  if (t.vy0 && t.vx1) v += s[t.y0 * W + t.x1] * w.w01;
  if (t.vy1 && t.vx0) v += s[t.y1 * W + t.x0] * w.w10;
  if (t.vy1 && t.vx1) v += s[t.y1 * W + t.x1] * w.w11;
  return v;
}

// the four tap values of one plane, 0 outside the frame
__device__ __forceinline__ void lf_tap_values(const float* __restrict__ s, int W, const lf_taps2d& t, float& v00, float& v01,
                                              float& v10, float& v11) {
  v00 = (t.vy0 && t.vx0) ? s[t.y0 * W + t.x0] : 0.f; v01 = (t.vy0 && t.vx1) ? s[t.y0 * W + t.x1] : 0.f;
  v10 = (t.vy1 && t.vx0) ? s[t.y1 * W + t.x0] : 0.f; v11 = (t.vy1 && t.vx1) ? s[t.y1 * W + t.x1] : 0.f;
}
