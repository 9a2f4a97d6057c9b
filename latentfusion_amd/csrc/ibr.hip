// Fused depth-based reprojection of image-based rendering (reference latentfusion/ibr.py:11-93: depth_to_warp_field +
// reproject_views): for every (object b, output view o, input view i, output pixel)
//   1. unproject the output pixel with its denormalised depth, carry it to object space and project it into input view i
//      -> the sampling coordinate;
//   2. bilinearly sample the C channels of image_in[b][i] there (align_corners=False, zeros padding);
//   3. sample the transformed input depth there too, each of the four taps formed on the fly from depth_in[b][i] at that
//      tap (unproject, carry into output camera o, z, normalise with the OUTPUT camera's bounds, clamp to [0,1], *2-1).
// No grid, no point set and no expanded image is materialised: the kernel reads V_i*(C+1)*H*W + V_o*H*W floats per object
// and writes V_o*V_i*(C+1)*H*W.  It is bound by those stores: one thread per (b, o, i, pixel), lanes along W, so every
// store instruction of a wave covers 256 contiguous bytes of one output plane; the gathers hit rows the neighbouring lanes
// also touch (L2).  No MFMA, no LDS.  Record layout: include/lf_hip.h.
#include "sample2d_taps.h"

namespace {

// linspace(0, 1, n)[k]
__device__ __forceinline__ float lattice(int k, int n) { return n > 1 ? (float)k / (float)(n - 1) : 0.f; }

// torch.clamp(v, 0, 1): NaN stays NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// entry k of a record's coordinate part: the fp64 value the host split into a leading float and the float of the remainder
__device__ __forceinline__ double wide_pair(const float* __restrict__ rec, int k) {
  return (double)rec[k] + (double)rec[k + LF_IBR_PAIR_SPLIT];
}
__device__ __forceinline__ double wide_view(const float* __restrict__ rec, int k) {
  return (double)rec[k] + (double)rec[k + LF_IBR_VIEW_SPLIT];
}

struct Coord {
  float fx, fy;      // floor of the pixel coordinate in the input view (align_corners=False)
  float tx, ty;      // offset from it
  float dsx, dsy;    // d(coordinate) / d(depth_out)
};

// Output pixel (x, y) of view o with normalised depth d -> pixel coordinate in input view i.  The chain runs in fp64 on the
// two-float record entries and splits into floor + offset before it returns to fp32: at the zero-padded frame edge the
// sampled value changes by |image| per pixel, and a relative error e of the chain moves the far edge by e*W pixels -- with
// fp32 arithmetic or singly rounded fp32 records (e ~ 1e-7) several 1e-6 pixels at W = 65, more than the forward bound of the
// tests leaves.  The records are uniform over a block (scalar loads); ~40 fp64 operations per thread, under the stores.
template <bool GRAD>
__device__ __forceinline__ Coord reproject(const float* __restrict__ pr, const float* __restrict__ vo, int x, int y, int H,
                                           int W, double step_x, double step_y, float d) {
  const double lx = (double)x * step_x, ly = (double)y * step_y;      // linspace(0, 1): step = 1 / (n - 1), 0 for n = 1
  const double xn = lx * wide_view(vo, 0) + wide_view(vo, 1), yn = ly * wide_view(vo, 2) + wide_view(vo, 3);
  const double z = (double)d * wide_view(vo, 4) + wide_view(vo, 5);
  const double q0 = wide_pair(pr, 0) * xn + wide_pair(pr, 1) * yn + wide_pair(pr, 2);
  const double q1 = wide_pair(pr, 4) * xn + wide_pair(pr, 5) * yn + wide_pair(pr, 6);
  const double q2 = wide_pair(pr, 8) * xn + wide_pair(pr, 9) * yn + wide_pair(pr, 10);
  const double p0 = z * q0 + wide_pair(pr, 3), p1 = z * q1 + wide_pair(pr, 7), p2 = z * q2 + wide_pair(pr, 11);
  const double rp2 = 1.0 / p2;                                        // the chain's one fp64 division
  const double nx = p0 * rp2, ny = p1 * rp2;
  const double sx = nx * (double)W - 0.5, sy = ny * (double)H - 0.5;
  const double fx = floor(sx), fy = floor(sy);
  Coord c;
  c.fx = (float)fx; c.fy = (float)fy;
  c.tx = (float)(sx - fx); c.ty = (float)(sy - fy);
  if (GRAD) {
    c.dsx = (float)((double)W * wide_view(vo, 4) * (q0 - nx * q2) * rp2);
    c.dsy = (float)((double)H * wide_view(vo, 4) * (q1 - ny * q2) * rp2);
  }
  return c;
}

// normalised depth of input pixel (x, y) of view i as output camera o sees it, BEFORE the clamp; slope = d(value)/d(depth_in)
__device__ __forceinline__ float tap_depth(const float* __restrict__ pr, const float* __restrict__ vi, int x, int y, int H, int W,
                                           float din, float& slope) {
  const float xn = lattice(x, W) * vi[0] + vi[1], yn = lattice(y, H) * vi[2] + vi[3];
  slope = pr[12] * xn + pr[13] * yn + pr[14];
  return din * slope + pr[15];
}

struct DepthTaps { float v00, v01, v10, v11, s00, s01, s10, s11; };   // clamped, mapped to [-1,1]; 2*slope where the clamp is idle, else 0

__device__ __forceinline__ void depth_tap(const float* __restrict__ pr, const float* __restrict__ vi, const float* __restrict__ din,
                                          bool valid, int x, int y, int H, int W, float& v, float& s) {
  v = 0.f; s = 0.f;
  if (!valid) return;
  float slope;
  const float raw = tap_depth(pr, vi, x, y, H, W, din[y * W + x], slope);
  v = clamp01(raw) * 2.f - 1.f;
  s = (raw >= 0.f && raw <= 1.f) ? 2.f * slope : 0.f;
}

__device__ __forceinline__ DepthTaps depth_taps(const float* __restrict__ pr, const float* __restrict__ vi,
                                                const float* __restrict__ din, const lf_taps2d& t, int H, int W) {
  DepthTaps d;
  depth_tap(pr, vi, din, t.vy0 && t.vx0, t.x0, t.y0, H, W, d.v00, d.s00);
  depth_tap(pr, vi, din, t.vy0 && t.vx1, t.x1, t.y0, H, W, d.v01, d.s01);
  depth_tap(pr, vi, din, t.vy1 && t.vx0, t.x0, t.y1, H, W, d.v10, d.s10);
  depth_tap(pr, vi, din, t.vy1 && t.vx1, t.x1, t.y1, H, W, d.v11, d.s11);
  return d;
}

// image_re * m and (depth_re + 1) * m - 1, each operation rounded on its own like the torch expressions
__device__ __forceinline__ float mask_image(float v, float m) {
#pragma clang fp contract(off)
  return v * m;
}
__device__ __forceinline__ float mask_depth(float v, float m) {
#pragma clang fp contract(off)
  const float a = v + 1.f;
  const float b = a * m;
  return b - 1.f;
}

// grid: rows * nblk blocks, row = (b*Vo + o)*Vi + i, a block never straddles two rows
template <bool MASK>
__global__ void __launch_bounds__(256) ibr_fwd_kernel(const float* __restrict__ image_in, const float* __restrict__ depth_in,
                                                      const float* __restrict__ depth_out, const float* __restrict__ mask_out,
                                                      const float* __restrict__ pair_rec, const float* __restrict__ in_rec,
                                                      const float* __restrict__ out_rec, float* __restrict__ image_re,
                                                      float* __restrict__ depth_re, int Vo, int Vi, int C, int H, int W,
                                                      unsigned nblk, double step_x, double step_y, long image_stride,
                                                      long depth_stride) {
  const unsigned row = blockIdx.x / nblk;
  const int pix = (int)((blockIdx.x - row * nblk) * 256u + threadIdx.x);
  const int HW = H * W;
  if (pix >= HW) return;
  const unsigned bo = row / (unsigned)Vi, i = row - bo * (unsigned)Vi, b = bo / (unsigned)Vo;
  const long bi = (long)b * Vi + i;
  const int y = pix / W, x = pix - y * W;
  const float* pr = pair_rec + (long)row * LF_IBR_PAIR_FLOATS;
  const float* vi = in_rec + bi * LF_IBR_VIEW_FLOATS;
  const float* vo = out_rec + (long)bo * LF_IBR_VIEW_FLOATS;
  const float d = depth_out[(long)bo * HW + pix];
  const Coord c = reproject<false>(pr, vo, x, y, H, W, step_x, step_y, d);
  const lf_taps2d t = lf_taps_from_floor(c.fx, c.fy, c.tx, c.ty, H, W);
  const lf_weights2d w = lf_bilinear_weights(t);
  const float m = MASK ? mask_out[(long)bo * HW + pix] : 1.f;
  const float* src = image_in + bi * C * HW;
  float* dst = image_re + (long)row * image_stride + pix;
  for (int ch = 0; ch < C; ++ch) {
    const float v = lf_bilinear_gather(src + (long)ch * HW, W, t, w);
    dst[(long)ch * HW] = MASK ? mask_image(v, m) : v;
  }
  const DepthTaps dt = depth_taps(pr, vi, depth_in + bi * HW, t, H, W);
  float v = 0.f;
  if (t.vy0 && t.vx0) v += dt.v00 * w.w00;
  if (t.vy0 && t.vx1) v += dt.v01 * w.w01;
  if (t.vy1 && t.vx0) v += dt.v10 * w.w10;
  if (t.vy1 && t.vx1) v += dt.v11 * w.w11;
  depth_re[(long)row * depth_stride + pix] = MASK ? mask_depth(v, m) : v;
}

// one thread per (b, o, pixel), looping over the input views and the channels in a fixed order: g_depth_out is a plain
// in-thread sum (run-to-run identical); g_image_in / g_depth_in scatter with float atomics
template <bool MASK>
__global__ void __launch_bounds__(256) ibr_bwd_kernel(const float* __restrict__ image_in, const float* __restrict__ depth_in,
                                                      const float* __restrict__ depth_out, const float* __restrict__ mask_out,
                                                      const float* __restrict__ pair_rec, const float* __restrict__ in_rec,
                                                      const float* __restrict__ out_rec, const float* __restrict__ g_image_re,
                                                      const float* __restrict__ g_depth_re, float* __restrict__ g_image_in,
                                                      float* __restrict__ g_depth_in, float* __restrict__ g_depth_out, int Vo,
                                                      int Vi, int C, int H, int W, unsigned nblk, double step_x,
                                                      double step_y) {
  const unsigned bo = blockIdx.x / nblk;
  const int pix = (int)((blockIdx.x - bo * nblk) * 256u + threadIdx.x);
  const int HW = H * W;
  if (pix >= HW) return;
  const unsigned b = bo / (unsigned)Vo;
  const int y = pix / W, x = pix - y * W;
  const float* vo = out_rec + (long)bo * LF_IBR_VIEW_FLOATS;
  const float d = depth_out[(long)bo * HW + pix];
  const float m = MASK ? mask_out[(long)bo * HW + pix] : 1.f;
  float gd = 0.f;
  for (int i = 0; i < Vi; ++i) {
    const long row = (long)bo * Vi + i, bi = (long)b * Vi + i;
    const float* pr = pair_rec + row * LF_IBR_PAIR_FLOATS;
    const Coord c = reproject<true>(pr, vo, x, y, H, W, step_x, step_y, d);
    const lf_taps2d t = lf_taps_from_floor(c.fx, c.fy, c.tx, c.ty, H, W);
    const float tx = t.tx, ty = t.ty;
    float gx = 0.f, gy = 0.f;
    if (g_image_re) {
      const float* src = image_in + bi * C * HW;
      const float* go = g_image_re + row * C * HW + pix;
      float* gsrc = g_image_in ? g_image_in + bi * C * HW : nullptr;
      for (int ch = 0; ch < C; ++ch) {
        const float g = go[(long)ch * HW] * m;
        float v00, v01, v10, v11;
        lf_tap_values(src + (long)ch * HW, W, t, v00, v01, v10, v11);
        gx += g * ((v01 - v00) * (1.f - ty) + (v11 - v10) * ty);
        gy += g * ((v10 - v00) * (1.f - tx) + (v11 - v01) * tx);
        if (gsrc) {
          float* p = gsrc + (long)ch * HW;
          if (t.vy0 && t.vx0) atomicAdd(p + t.y0 * W + t.x0, g * (1.f - tx) * (1.f - ty));
          if (t.vy0 && t.vx1) atomicAdd(p + t.y0 * W + t.x1, g * tx * (1.f - ty));
          if (t.vy1 && t.vx0) atomicAdd(p + t.y1 * W + t.x0, g * (1.f - tx) * ty);
          if (t.vy1 && t.vx1) atomicAdd(p + t.y1 * W + t.x1, g * tx * ty);
        }
      }
    }
    if (g_depth_re) {
      const float g = g_depth_re[row * HW + pix] * m;
      const DepthTaps dt = depth_taps(pr, in_rec + bi * LF_IBR_VIEW_FLOATS, depth_in + bi * HW, t, H, W);
      gx += g * ((dt.v01 - dt.v00) * (1.f - ty) + (dt.v11 - dt.v10) * ty);
      gy += g * ((dt.v10 - dt.v00) * (1.f - tx) + (dt.v11 - dt.v01) * tx);
      if (g_depth_in) {
        float* p = g_depth_in + bi * HW;      // (a tap in the clamp has slope 0: nothing is added there)
        if (t.vy0 && t.vx0 && dt.s00 != 0.f) atomicAdd(p + t.y0 * W + t.x0, g * (1.f - tx) * (1.f - ty) * dt.s00);
        if (t.vy0 && t.vx1 && dt.s01 != 0.f) atomicAdd(p + t.y0 * W + t.x1, g * tx * (1.f - ty) * dt.s01);
        if (t.vy1 && t.vx0 && dt.s10 != 0.f) atomicAdd(p + t.y1 * W + t.x0, g * (1.f - tx) * ty * dt.s10);
        if (t.vy1 && t.vx1 && dt.s11 != 0.f) atomicAdd(p + t.y1 * W + t.x1, g * tx * ty * dt.s11);
      }
    }
    gd += gx * c.dsx + gy * c.dsy;
  }
  if (g_depth_out) g_depth_out[(long)bo * HW + pix] = gd;
}

// rows * ceil(H*W / 256) blocks; 0 if the shape is outside what the index arithmetic covers
unsigned grid_blocks(long rows, int H, int W, unsigned* nblk) {
  if ((long)H * W >= 0x7fffffffL) return 0;
  const long n = ((long)H * W + 255) / 256;
  if (rows * n >= 0x7fffffffL) return 0;
  *nblk = (unsigned)n;
  return (unsigned)(rows * n);
}

}  // namespace

extern "C" int lf_ibr_reproject_fwd(const float* image_in, const float* depth_in, const float* depth_out, const float* mask_out,
                                    const float* pair_rec, const float* in_rec, const float* out_rec, float* image_re,
                                    float* depth_re, int B, int Vo, int Vi, int C, int H, int W, long image_row_stride,
                                    long depth_row_stride, void* stream) {
  lf_clear_error();
  if (!image_in || !depth_in || !depth_out || !pair_rec || !in_rec || !out_rec || !image_re || !depth_re) return LF_EINVAL;
  if (B < 1 || Vo < 1 || Vi < 1 || C < 1 || H < 1 || W < 1) return LF_EINVAL;
  if (image_row_stride < (long)C * H * W || depth_row_stride < (long)H * W) return LF_EINVAL;
  unsigned nblk = 0;
  const unsigned blocks = grid_blocks((long)B * Vo * Vi, H, W, &nblk);
  if (!blocks) return LF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const double step_x = W > 1 ? 1.0 / (double)(W - 1) : 0.0, step_y = H > 1 ? 1.0 / (double)(H - 1) : 0.0;
#define LAUNCH(M) hipLaunchKernelGGL((ibr_fwd_kernel<M>), dim3(blocks), dim3(256), 0, s, image_in, depth_in, depth_out, mask_out, \
                                     pair_rec, in_rec, out_rec, image_re, depth_re, Vo, Vi, C, H, W, nblk, step_x, step_y,     \
                                     image_row_stride, depth_row_stride)
  if (mask_out) LAUNCH(true); else LAUNCH(false);
#undef LAUNCH
  return lf_launch_status();
}

extern "C" int lf_ibr_reproject_bwd(const float* image_in, const float* depth_in, const float* depth_out, const float* mask_out,
                                    const float* pair_rec, const float* in_rec, const float* out_rec, const float* g_image_re,
                                    const float* g_depth_re, float* g_image_in, float* g_depth_in, float* g_depth_out, int B,
                                    int Vo, int Vi, int C, int H, int W, void* stream) {
  lf_clear_error();
  if (!image_in || !depth_in || !depth_out || !pair_rec || !in_rec || !out_rec) return LF_EINVAL;
  if (!g_image_re && !g_depth_re) return LF_EINVAL;
  if (B < 1 || Vo < 1 || Vi < 1 || C < 1 || H < 1 || W < 1) return LF_EINVAL;
  unsigned nblk = 0;
  const unsigned blocks = grid_blocks((long)B * Vo, H, W, &nblk);
  if (!blocks || !grid_blocks((long)B * Vo * Vi, H, W, &nblk)) return LF_EINVAL;
  if (!g_image_in && !g_depth_in && !g_depth_out) return 0;
  hipStream_t s = (hipStream_t)stream;
  const double step_x = W > 1 ? 1.0 / (double)(W - 1) : 0.0, step_y = H > 1 ? 1.0 / (double)(H - 1) : 0.0;
#define LAUNCH(M) hipLaunchKernelGGL((ibr_bwd_kernel<M>), dim3(blocks), dim3(256), 0, s, image_in, depth_in, depth_out, mask_out, \
                                     pair_rec, in_rec, out_rec, g_image_re, g_depth_re, g_image_in, g_depth_in, g_depth_out, Vo, \
                                     Vi, C, H, W, nblk, step_x, step_y)
  if (mask_out) LAUNCH(true); else LAUNCH(false);
#undef LAUNCH
  return lf_launch_status();
}
