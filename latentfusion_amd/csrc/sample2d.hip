// 2-D grid sampling of planar (NCHW) images: the F.grid_sample(align_corners=False) calls of
//   crop_to_viewport / Camera.zoom      latentfusion/modules/geometry.py:20-44,287-354   (zeros padding)
//   Camera.uncrop                        latentfusion/modules/geometry.py:261-285         (border padding)
//   ibr.reproject_views                  latentfusion/ibr.py:52-93                        (zeros padding)
// grid: [N][Ho][Wo][2] = (x, y) in [-1, 1]; modes bilinear / nearest (round-half-even like ATen).
// One thread per output pixel, looping over the (few) channels; backward w.r.t. the grid is a plain
// per-pixel sum, backward w.r.t. the image scatters with float atomics (not used on any ranking path).
// The tap / validity logic lives in sample2d_taps.h, shared with the fused IBR reprojection (ibr.hip).
#include "sample2d_taps.h"

namespace {

// border padding: clip to [0, size-1]; returns d(clipped)/d(p)
__device__ __forceinline__ float clip_border(float& p, int size) {
  const float hi = (float)(size - 1);
  const float d = (p > 0.f && p < hi) ? 1.f : 0.f;
  p = fminf(fmaxf(p, 0.f), hi);
  return d;
}

template <bool BILINEAR, bool BORDER>
__global__ void __launch_bounds__(256) sample2d_fwd_kernel(const float* __restrict__ img, const float* __restrict__ grid,
                                                           float* __restrict__ out, int N, int C, int H, int W, int Ho,
                                                           int Wo) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * Ho * Wo) return;
  const int n = idx / (Ho * Wo), pix = idx - n * Ho * Wo;
  float px = lf_unnorm2d(grid[(long)idx * 2 + 0], W), py = lf_unnorm2d(grid[(long)idx * 2 + 1], H);
  if (BORDER) { clip_border(px, W); clip_border(py, H); }
  const float* src = img + (long)n * C * H * W;
  float* dst = out + (long)n * C * Ho * Wo + pix;
  if (BILINEAR) {
    const lf_taps2d t = lf_bilinear_taps(px, py, H, W);
    const lf_weights2d w = lf_bilinear_weights(t);
    for (int c = 0; c < C; ++c) dst[(long)c * Ho * Wo] = lf_bilinear_gather(src + (long)c * H * W, W, t, w);
  } else {
    const int xn = (int)nearbyintf(px), yn = (int)nearbyintf(py);
    const bool ok = (unsigned)xn < (unsigned)W && (unsigned)yn < (unsigned)H;
    for (int c = 0; c < C; ++c) dst[(long)c * Ho * Wo] = ok ? src[(long)c * H * W + yn * W + xn] : 0.f;
  }
}

template <bool BILINEAR, bool BORDER>
__global__ void __launch_bounds__(256) sample2d_bwd_kernel(const float* __restrict__ img, const float* __restrict__ grid,
                                                           const float* __restrict__ gout, float* __restrict__ gimg,
                                                           float* __restrict__ ggrid, int N, int C, int H, int W, int Ho,
                                                           int Wo) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * Ho * Wo) return;
  const int n = idx / (Ho * Wo), pix = idx - n * Ho * Wo;
  float px = lf_unnorm2d(grid[(long)idx * 2 + 0], W), py = lf_unnorm2d(grid[(long)idx * 2 + 1], H);
  float mx = 0.5f * (float)W, my = 0.5f * (float)H;            // d(p)/d(grid)
  if (BORDER) { mx *= clip_border(px, W); my *= clip_border(py, H); }
  const float* src = img + (long)n * C * H * W;
  float* gsrc = gimg ? gimg + (long)n * C * H * W : nullptr;
  const float* go = gout + (long)n * C * Ho * Wo + pix;
  float gx = 0.f, gy = 0.f;
  if (BILINEAR) {
    const lf_taps2d t = lf_bilinear_taps(px, py, H, W);
    const int x0 = t.x0, y0 = t.y0, x1 = t.x1, y1 = t.y1;
    const float tx = t.tx, ty = t.ty;
    const bool vx0 = t.vx0, vx1 = t.vx1, vy0 = t.vy0, vy1 = t.vy1;
    for (int c = 0; c < C; ++c) {
      const float g = go[(long)c * Ho * Wo];
      float v00, v01, v10, v11;
      lf_tap_values(src + (long)c * H * W, W, t, v00, v01, v10, v11);
      gx += g * ((v01 - v00) * (1.f - ty) + (v11 - v10) * ty);
      gy += g * ((v10 - v00) * (1.f - tx) + (v11 - v01) * tx);
      if (gsrc) {
        float* d = gsrc + (long)c * H * W;
        if (vy0 && vx0) atomicAdd(d + y0 * W + x0, g * (1.f - tx) * (1.f - ty));
        if (vy0 && vx1) atomicAdd(d + y0 * W + x1, g * tx * (1.f - ty));
        if (vy1 && vx0) atomicAdd(d + y1 * W + x0, g * (1.f - tx) * ty);
        if (vy1 && vx1) atomicAdd(d + y1 * W + x1, g * tx * ty);
      }
    }
  } else if (gsrc) {
    const int xn = (int)nearbyintf(px), yn = (int)nearbyintf(py);
    if ((unsigned)xn < (unsigned)W && (unsigned)yn < (unsigned)H)
      for (int c = 0; c < C; ++c) atomicAdd(gsrc + (long)c * H * W + yn * W + xn, go[(long)c * Ho * Wo]);
  }
  if (ggrid) {
    ggrid[(long)idx * 2 + 0] = gx * mx;
    ggrid[(long)idx * 2 + 1] = gy * my;
  }
}

}  // namespace

extern "C" int lf_grid_sample2d_fwd(const float* img, const float* grid, float* out, int N, int C, int H, int W, int Ho,
                                    int Wo, int bilinear, int border, void* stream) {
  lf_clear_error();
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return LF_EINVAL;
  if ((long)N * Ho * Wo >= 0x7fffffffL || (long)H * W >= 0x7fffffffL) return LF_EINVAL;
  dim3 g((unsigned)(((long)N * Ho * Wo + 255) / 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(B, P) hipLaunchKernelGGL((sample2d_fwd_kernel<B, P>), g, b, 0, s, img, grid, out, N, C, H, W, Ho, Wo)
  if (bilinear) { if (border) LAUNCH(true, true); else LAUNCH(true, false); }
  else          { if (border) LAUNCH(false, true); else LAUNCH(false, false); }
#undef LAUNCH
  return lf_launch_status();
}

extern "C" int lf_grid_sample2d_bwd(const float* img, const float* grid, const float* gout, float* gimg, float* ggrid,
                                    int N, int C, int H, int W, int Ho, int Wo, int bilinear, int border, void* stream) {
  lf_clear_error();
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return LF_EINVAL;
  if ((long)N * Ho * Wo >= 0x7fffffffL || (long)H * W >= 0x7fffffffL) return LF_EINVAL;
  dim3 g((unsigned)(((long)N * Ho * Wo + 255) / 256)), b(256);
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(B, P) hipLaunchKernelGGL((sample2d_bwd_kernel<B, P>), g, b, 0, s, img, grid, gout, gimg, ggrid, N, C, H, W, Ho, Wo)
  if (bilinear) { if (border) LAUNCH(true, true); else LAUNCH(true, false); }
  else          { if (border) LAUNCH(false, true); else LAUNCH(false, false); }
#undef LAUNCH
  return lf_launch_status();
}
