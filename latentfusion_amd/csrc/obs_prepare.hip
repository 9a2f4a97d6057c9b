// Observation preprocessing for B frames in one launch (gfx950): the crop of colour, depth and mask to each frame's zoomed
// viewport and the element-wise chains of Observation.prepare / normalize, written as the three maps and, when asked, as the
// encoder's stacked input (reference modules/geometry.py:20-44,287-354 crop_to_viewport / Camera.zoom, observation.py:225-282
// zoom / prepare / normalize, recon/models.py Sculptor.encode).  The contract, op by op, is in include/lf_hip.h.
//   One thread per output pixel of one frame; a workgroup holds 256 consecutive pixels of ONE frame (grid = B * tiles), so the
//   frame index, the box, the lattice constants and zn / zf are wave-uniform (the box and zn / zf arrive through scalar loads)
//   and consecutive lanes store consecutive addresses of the T-wide output rows.  The four lattice constants are derived
//   redundantly by every thread: two fp64 divisions and two fp32 ones per axis, nothing next to the launch itself.
//   The kernel is a gather of B * (C + 2) * T^2 values that reads each frame only inside its box.  There is no reuse between
//   threads that LDS could serve (neighbouring bilinear taps hit the same cache lines already) and nothing matrix shaped, so
//   neither LDS nor MFMA is used.  No scratch, no atomics: every output is a function of its own frame alone.
//   Taps and their validity come from sample2d_taps.h exactly as in lf_grid_sample2d_fwd, compiled under the same flags;
//   every operation that is this file's own is rounded separately (contraction is switched off below the include, where it
//   cannot reach the shared header's functions).
#include <math.h>
#include "sample2d_taps.h"

#pragma clang fp contract(off)

namespace {

constexpr int OP_T = 256;             // threads per workgroup = output pixels per tile
constexpr long OP_MAX_GRID = 1L << 20;  // workgroups per launch at most; beyond it the workgroups walk the tiles with a grid stride
//                                        (reachable only with tiny T and B > 2^20; not exercised by the tests)

// lattice constants of one axis: start, end, step (header: "per-frame lattice")
struct op_axis { float start, end, step; };

__device__ __forceinline__ op_axis op_axis_of(float c0, float c1, int size, int T) {
  op_axis a;
  a.start = (float)((double)truncf(c0) / (double)size);
  a.end = (float)((double)truncf(c1) / (double)size);
  a.step = T > 1 ? (a.end - a.start) / (float)(T - 1) : 0.f;
  return a;
}

// grid value of lattice point i: the lattice, then * 2, then - 1
__device__ __forceinline__ float op_grid(const op_axis& a, int i, int T) {
  float l;
  if (T == 1) {
    l = a.start;
  } else if (i < T / 2) {
    const float o = a.step * (float)i;
    l = a.start + o;
  } else {
    const float o = a.step * (float)(T - 1 - i);
    l = a.end - o;
  }
  const float l2 = l * 2.f;
  return l2 - 1.f;
}

// torch.clamp(v, 0, 1): a NaN stays NaN
__device__ __forceinline__ float op_clamp01(float v) { return v != v ? v : fminf(fmaxf(v, 0.f), 1.f); }

template <bool U8>
__global__ void __launch_bounds__(OP_T) obs_prepare_kernel(const float* __restrict__ color, const float* __restrict__ depth,
                                                           const void* __restrict__ mask, const float* __restrict__ boxes,
                                                           const float* __restrict__ zn, const float* __restrict__ zf,
                                                           float* __restrict__ color_out, float* __restrict__ depth_out,
                                                           float* __restrict__ mask_out, float* __restrict__ stack,
                                                           long stack_row_stride, int stack_depth, int C, int H, int W, int T,
                                                           int tiles, long items, int stages) {
  const int TT = T * T;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {                 // one pass unless B * tiles > OP_MAX_GRID
    const int b = (int)(item / tiles), tile = (int)(item - (long)b * tiles);
    const int pix = tile * OP_T + threadIdx.x;
    if (pix >= TT) continue;
    const int oy = pix / T, ox = pix - oy * T;
    const float* box = boxes + (long)b * 4;
    const op_axis ax = op_axis_of(box[0], box[2], W, T), ay = op_axis_of(box[1], box[3], H, T);
    const float px = lf_unnorm2d(op_grid(ax, ox, T), W), py = lf_unnorm2d(op_grid(ay, oy, T), H);
    const bool prepare = (stages & LF_OBS_PREPARE) != 0, normalize = (stages & LF_OBS_NORMALIZE) != 0;
    const long HW = (long)H * W;

    // depth and mask: nearest, round-half-even, zeros outside the frame
    const int xn = (int)nearbyintf(px), yn = (int)nearbyintf(py);
    const bool ok = (unsigned)xn < (unsigned)W && (unsigned)yn < (unsigned)H;
    float m = 0.f, d = 0.f;
    if (ok) {
      const long at = (long)b * HW + (long)yn * W + xn;
      if constexpr (U8) m = (float)((const unsigned char*)mask)[at];
      else m = ((const float*)mask)[at];
      d = depth[at];
    }
    if (prepare) d = d * m;
    if (normalize) {
      const float lo = zn[b], span = zf[b] - lo;
      const float q = (d - lo) / span;
      const float c2 = op_clamp01(q) * 2.f;
      d = c2 - 1.f;
    }
    const long obase = (long)b * TT + pix;
    depth_out[obase] = d;
    mask_out[obase] = m;
    float* srow = stack != nullptr ? stack + (long)b * stack_row_stride + pix : nullptr;
    if (srow != nullptr) {
      if (stack_depth) srow[(long)C * TT] = d;
      const float m2 = m * 2.f;
      srow[(long)(C + (stack_depth ? 1 : 0)) * TT] = m2 - 1.f;
    }

    // colour: bilinear, zeros outside the frame
    if (C > 0) {
      const lf_taps2d t = lf_bilinear_taps(px, py, H, W);
      const lf_weights2d w = lf_bilinear_weights(t);
      const float* src = color + (long)b * C * HW;
      float* dst = color_out + (long)b * C * TT + pix;
      for (int c = 0; c < C; ++c) {
        float v = lf_bilinear_gather(src + (long)c * HW, W, t, w);
        if (prepare) {
          const float g2 = v * 2.f;
          const float g = g2 - 1.f;
          const float gm = g * m;
          const float g1 = gm + 1.f;
          v = op_clamp01(g1 / 2.f);
        }
        if (normalize) {
          const float v2 = v * 2.f;
          v = v2 - 1.f;
        }
        dst[(long)c * TT] = v;
        if (srow != nullptr) srow[(long)c * TT] = v;
      }
    }
  }
}

inline bool op_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

}  // namespace

extern "C" int lf_obs_prepare(const float* color, const float* depth, const void* mask, int mask_u8, const float* boxes,
                              const float* zn, const float* zf, float* color_out, float* depth_out, float* mask_out,
                              float* stack, long stack_row_stride, int stack_depth, int B, int C, int H, int W, int T,
                              int stages, void* stream) {
  lf_clear_error();
  if (depth == nullptr || mask == nullptr || boxes == nullptr || depth_out == nullptr || mask_out == nullptr) return LF_EINVAL;
  if (B < 1 || H < 1 || W < 1 || T < 1 || C < 0) return LF_EINVAL;
  if (C > 0 && (color == nullptr || color_out == nullptr)) return LF_EINVAL;
  if (mask_u8 != 0 && mask_u8 != 1) return LF_EINVAL;
  if ((stages & ~(LF_OBS_PREPARE | LF_OBS_NORMALIZE)) != 0) return LF_EINVAL;
  if ((stages & LF_OBS_NORMALIZE) != 0 && (zn == nullptr || zf == nullptr)) return LF_EINVAL;
  const long lim = 0x80000000L;
  const long bc = (long)B * (C > 1 ? C : 1), hw = (long)H * W, bp = (long)B * ((long)C + 2), tt = (long)T * T;
  if (bc >= lim || hw >= lim || bc * hw >= lim) return LF_EINVAL;
  if (bp >= lim || tt >= lim || bp * tt >= lim) return LF_EINVAL;
  if (stack_depth != 0 && stack_depth != 1) return LF_EINVAL;
  if (stack != nullptr && stack_row_stride < ((long)C + stack_depth + 1) * tt) return LF_EINVAL;
  if (!op_aligned4(color) || !op_aligned4(depth) || !op_aligned4(mask) || !op_aligned4(boxes) || !op_aligned4(zn) ||
      !op_aligned4(zf) || !op_aligned4(color_out) || !op_aligned4(depth_out) || !op_aligned4(mask_out) || !op_aligned4(stack))
    return LF_EALIGN;
  const int tiles = (int)((tt + OP_T - 1) / OP_T);
  const long items = (long)B * tiles;
  const dim3 grid((unsigned)(items < OP_MAX_GRID ? items : OP_MAX_GRID)), block(OP_T);
  const auto kern = mask_u8 ? obs_prepare_kernel<true> : obs_prepare_kernel<false>;
  hipLaunchKernelGGL(kern, grid, block, 0, (hipStream_t)stream, C > 0 ? color : nullptr, depth, mask, boxes, zn, zf,
                     C > 0 ? color_out : nullptr, depth_out, mask_out, stack, stack_row_stride, stack_depth, C, H, W, T, tiles,
                     items, stages);
  return lf_launch_status();
}
