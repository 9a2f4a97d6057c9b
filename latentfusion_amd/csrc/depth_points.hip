// Evaluation point clouds from depth maps (gfx950): back-projection of the viewport lattice, segmentation by re-projection into
// the mask and ORDERED compaction of the kept points (reference observation.py:292-316 Observation.pointcloud over
// pointcloud.py:57-79 project_pointcloud / compute_point_mask).  The per-pixel arithmetic is the chain include/lf_hip.h writes
// out, every step one correctly rounded fp32 operation (explicit fmaf where the chain fuses, fp contraction off for the rest
// of the file -- the pragma below), in ONE device function that both launches inline, so the counting launch and the writing
// launch decide every pixel alike.
//   launch 1  one workgroup per chunk of DP_CHUNK consecutive pixels of one view: the number of kept pixels into scratch[chunk]
//   launch 2  the same grid: a workgroup adds up the counts of the chunks before its own (integers: any order gives the same sum;
//             the order is fixed all the same), then walks its chunk in DP_ROUNDS rounds of 256 consecutive pixels, ranks the kept
//             ones by a wave ballot and the four wave totals, and writes the rows.  The first chunk of a view also adds up its
//             view's counts into counts[b].
// No atomics: a row's place is a function of the keep decisions before it alone.  segment = 0 is one launch that writes every
// pixel at its own index.
#include <math.h>
#include "lf_common.h"

#pragma clang fp contract(off)      // to the end of the file: only the fmaf calls are fused

namespace {

constexpr int DP_ROUNDS = 4;
constexpr int DP_CHUNK = 256 * DP_ROUNDS;       // pixels of one workgroup
constexpr int DP_CAM = LF_DEPTH_CAM_FLOATS;

struct DpPoint {
  float x, y, z;
  bool keep;
};

__device__ __forceinline__ float dp_row(const float* __restrict__ t, float x, float y, float z) {
  return fmaf(t[0], x, fmaf(t[1], y, fmaf(t[2], z, t[3])));
}

// lattice coordinate of sample j of n: v0 + vw * (j / (n - 1)); v0 for n = 1
__device__ __forceinline__ float dp_lattice(float v0, float vw, int j, int n) {
  return n > 1 ? fmaf(vw, (float)j / (float)(n - 1), v0) : v0;
}

// one pixel (view b, row yy, column xx) of depth z: the point and, with SEGMENT, whether it is kept
template <bool SEGMENT>
__device__ __forceinline__ DpPoint dp_pixel(const float* __restrict__ cam, const void* __restrict__ mask, int mask_u8, float z,
                                            int b, int yy, int xx, int H, int W, int frame_w, int frame_h, int to_object) {
  DpPoint p;
  const float u = dp_lattice(cam[0], cam[2], xx, W), v = dp_lattice(cam[1], cam[3], yy, H);
  float x = (u - cam[6]) / cam[4] * z;
  float y = (v - cam[7]) / cam[5] * z;
  float zz = z;
  if (to_object) {
    const float a = dp_row(cam + 8, x, y, zz), bb = dp_row(cam + 12, x, y, zz), c = dp_row(cam + 16, x, y, zz);
    x = a;
    y = bb;
    zz = c;
  }
  p.x = x;
  p.y = y;
  p.z = zz;
  p.keep = true;
  if constexpr (SEGMENT) {
    const float h0 = dp_row(cam + 20, x, y, zz), h1 = dp_row(cam + 24, x, y, zz), h2 = dp_row(cam + 28, x, y, zz);
    const float pu = h0 / h2, pv = h1 / h2;
    // trunc(pu) in [0, frame_w)  <=>  -1 < pu < frame_w (the comparisons are false for NaN; +-inf fails one of them)
    bool keep = z != 0.f && pu > -1.f && pu < (float)frame_w && pv > -1.f && pv < (float)frame_h;
    if (keep) {
      const long at = ((long)b * frame_h + (int)pv) * frame_w + (int)pu;      // (frame_h, frame_w) == (H, W): inside the mask
      keep = mask_u8 ? ((const unsigned char*)mask)[at] != 0 : ((const float*)mask)[at] != 0.f;
    }
    p.keep = keep;
  }
  return p;
}

// workgroup (b, c): pixels c * DP_CHUNK + r * 256 + thread, r < DP_ROUNDS, of view b
__global__ void __launch_bounds__(256) dp_count_kernel(const float* __restrict__ depth, const void* __restrict__ mask, int mask_u8,
                                                      const float* __restrict__ cams, int* __restrict__ chunk_count, int H, int W,
                                                      int cpv, int frame_w, int frame_h, int to_object) {
  __shared__ int wtot[4];
  const int b = blockIdx.x / cpv, c = blockIdx.x - b * cpv, tid = threadIdx.x;
  const int HW = H * W;
  const float* cam = cams + (long)b * DP_CAM;
  int n = 0;
#pragma unroll
  for (int r = 0; r < DP_ROUNDS; ++r) {
    const int i = c * DP_CHUNK + r * 256 + tid;
    if (i < HW) {
      const int yy = i / W, xx = i - yy * W;
      n += dp_pixel<true>(cam, mask, mask_u8, depth[(long)b * HW + i], b, yy, xx, H, W, frame_w, frame_h, to_object).keep ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((tid & 63) == 0) wtot[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) chunk_count[blockIdx.x] = wtot[0] + wtot[1] + wtot[2] + wtot[3];
}

__global__ void __launch_bounds__(256) dp_write_kernel(const float* __restrict__ depth, const void* __restrict__ mask, int mask_u8,
                                                      const float* __restrict__ color, const float* __restrict__ cams,
                                                      const int* __restrict__ chunk_count, float* __restrict__ points,
                                                      float* __restrict__ colors, int* __restrict__ index, int* __restrict__ counts,
                                                      int H, int W, int cpv, int frame_w, int frame_h, int to_object, long cap) {
  __shared__ int wsum[4], wview[4], wtot[DP_ROUNDS][4];
  const int b = blockIdx.x / cpv, c = blockIdx.x - b * cpv, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W;
  const float* cam = cams + (long)b * DP_CAM;

  // rows before this chunk: the counts of chunks [0, blockIdx.x), thread t taking t, t + 256, ..; chunk 0 of a view: its total too
  int before = 0, view = 0;
  for (int j = tid; j < (int)blockIdx.x; j += 256) before += chunk_count[j];
  if (c == 0)
    for (int j = tid; j < cpv; j += 256) view += chunk_count[blockIdx.x + j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    before += __shfl_xor(before, o, 64);
    view += __shfl_xor(view, o, 64);
  }
  if (lane == 0) {
    wsum[wave] = before;
    wview[wave] = view;
  }

  DpPoint p[DP_ROUNDS];
  int rank[DP_ROUNDS];
#pragma unroll
  for (int r = 0; r < DP_ROUNDS; ++r) {
    const int i = c * DP_CHUNK + r * 256 + tid;
    p[r].keep = false;
    if (i < HW) {
      const int yy = i / W, xx = i - yy * W;
      p[r] = dp_pixel<true>(cam, mask, mask_u8, depth[(long)b * HW + i], b, yy, xx, H, W, frame_w, frame_h, to_object);
    }
    const unsigned long long bal = __ballot(p[r].keep);
    rank[r] = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[r][wave] = __popcll(bal);
  }
  __syncthreads();
  long row = (long)wsum[0] + wsum[1] + wsum[2] + wsum[3];
  if (c == 0 && tid == 0) counts[b] = wview[0] + wview[1] + wview[2] + wview[3];
#pragma unroll
  for (int r = 0; r < DP_ROUNDS; ++r) {
    long at = row + rank[r];
    for (int w = 0; w < wave; ++w) at += wtot[r][w];
    if (p[r].keep && at < cap) {               // (at < cap always: the two launches decide alike; the test costs nothing)
      const int i = c * DP_CHUNK + r * 256 + tid;
      points[at * 3] = p[r].x;
      points[at * 3 + 1] = p[r].y;
      points[at * 3 + 2] = p[r].z;
      if (index != nullptr) index[at] = b * HW + i;
      if (colors != nullptr) {
        const float* cb = color + (long)b * 3 * HW + i;
        colors[at * 3] = cb[0];
        colors[at * 3 + 1] = cb[HW];
        colors[at * 3 + 2] = cb[2 * (long)HW];
      }
    }
    row += wtot[r][0] + wtot[r][1] + wtot[r][2] + wtot[r][3];
  }
}

// segment = 0: every pixel at its own index
__global__ void __launch_bounds__(256) dp_all_kernel(const float* __restrict__ depth, const float* __restrict__ color,
                                                    const float* __restrict__ cams, float* __restrict__ points,
                                                    float* __restrict__ colors, int* __restrict__ index, int* __restrict__ counts, int H,
                                                    int W, int cpv, int to_object) {
  const int b = blockIdx.x / cpv, c = blockIdx.x - b * cpv, tid = threadIdx.x;
  const int HW = H * W;
  const float* cam = cams + (long)b * DP_CAM;
  if (c == 0 && tid == 0) counts[b] = HW;
#pragma unroll
  for (int r = 0; r < DP_ROUNDS; ++r) {
    const int i = c * DP_CHUNK + r * 256 + tid;
    if (i >= HW) continue;
    const int yy = i / W, xx = i - yy * W;
    const long at = (long)b * HW + i;
    const DpPoint p = dp_pixel<false>(cam, nullptr, 0, depth[at], b, yy, xx, H, W, 0, 0, to_object);
    points[at * 3] = p.x;
    points[at * 3 + 1] = p.y;
    points[at * 3 + 2] = p.z;
    if (index != nullptr) index[at] = (int)at;
    if (colors != nullptr) {
      const float* cb = color + (long)b * 3 * HW + i;
      colors[at * 3] = cb[0];
      colors[at * 3 + 1] = cb[HW];
      colors[at * 3 + 2] = cb[2 * (long)HW];
    }
  }
}

inline bool dp_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }
inline long dp_chunks(int H, int W) { return ((long)H * W + DP_CHUNK - 1) / DP_CHUNK; }
inline bool dp_domain(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long)B * H * W <= 0x7fffffffL; }

}  // namespace

extern "C" size_t lf_depth_points_scratch_bytes(int B, int H, int W) {
  if (!dp_domain(B, H, W)) return 0;
  return (size_t)B * (size_t)dp_chunks(H, W) * sizeof(int);
}

extern "C" int lf_depth_points(const float* depth, const void* mask, int mask_u8, const float* color, const float* cams,
                               float* points, float* colors, int* index, int* counts, void* scratch, size_t scratch_bytes, int B,
                               int H, int W, int frame_w, int frame_h, int to_object, int segment, void* stream) {
  lf_clear_error();
  if (depth == nullptr || cams == nullptr || points == nullptr || counts == nullptr || !dp_domain(B, H, W)) return LF_EINVAL;
  if ((mask_u8 != 0 && mask_u8 != 1) || (to_object != 0 && to_object != 1) || (segment != 0 && segment != 1)) return LF_EINVAL;
  if ((color == nullptr) != (colors == nullptr)) return LF_EINVAL;
  if (segment && (mask == nullptr || frame_w != W || frame_h != H)) return LF_EINVAL;
  if (!dp_aligned4(depth) || !dp_aligned4(mask) || !dp_aligned4(color) || !dp_aligned4(cams) || !dp_aligned4(points) ||
      !dp_aligned4(colors) || !dp_aligned4(index) || !dp_aligned4(counts) || !dp_aligned4(scratch))
    return LF_EALIGN;
  const int cpv = (int)dp_chunks(H, W);
  const size_t need = (size_t)B * (size_t)cpv * sizeof(int);
  if (segment && (scratch == nullptr || scratch_bytes < need)) return LF_ENOSPC;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((long)B * cpv));
  if (!segment) {
    hipLaunchKernelGGL(dp_all_kernel, grid, dim3(256), 0, s, depth, color, cams, points, colors, index, counts, H, W, cpv, to_object);
    return lf_launch_status();
  }
  int* chunk_count = (int*)scratch;
  hipLaunchKernelGGL(dp_count_kernel, grid, dim3(256), 0, s, depth, mask, mask_u8, cams, chunk_count, H, W, cpv, frame_w, frame_h,
                     to_object);
  const int st = lf_launch_status();
  if (st) return st;
  hipLaunchKernelGGL(dp_write_kernel, grid, dim3(256), 0, s, depth, mask, mask_u8, color, cams, (const int*)chunk_count, points,
                     colors, index, counts, H, W, cpv, frame_w, frame_h, to_object, (long)B * H * W);
  return lf_launch_status();
}
