// Initial pose from a target's depth and mask (gfx950), batched over B frames: the centre of the mask's bounding box and the
// mid-range of the MAD-filtered masked depth (reference pose/initialization.py:8-86: _masks_to_viewports, _erode_mask,
// _reject_outliers_mad, _estimate_camera_dist, estimate_translation).  Every output is an order statistic, a minimum or maximum,
// an integer count or one correctly rounded fp32 operation on those, so the results are held bit for bit to the host functions
// and do not depend on the order in which the atomics below arrive.  No float atomics, no waiting between workgroups.
//   di_compact_kernel  one pass over the pixels: the bounding box and pixel count of the foreground (reduced per workgroup, then
//                      integer atomicMax / atomicAdd on the image's header) and the valid depths (foreground, inside the eroded
//                      mask when a radius is given, depth > 0) appended to the image's row of scratch -- one atomicAdd per
//                      workgroup reserves its range, the places inside come from __ballot prefixes.
//   di_select_kernel   one workgroup per image over its compacted values: an 8-bit-digit radix select, most significant digit
//                      first, on the raw bit patterns (positive floats, +inf included, order like their bits) finds the lower
//                      median, the same select over the bits of |d - median| the MAD, one more pass the kept minimum, maximum
//                      and count; then the translation.  The LDS histogram takes one add per wave where the wave's active lanes
//                      agree on the digit (the high digits of depths that lie close together), one per lane otherwise.
// The header of image b is DI_HDR ints (one 128-byte line, so that the images' atomics do not share a line):
//   [0] n_valid  [1] n_mask  [2] W - xmin  [3] H - ymin  [4] xmax + 1  [5] ymax + 1     (0 = no foreground; all by atomicMax / Add
//   from zero, so one hipMemsetAsync prepares them)
#include <math.h>
#include "lf_common.h"

namespace {

constexpr int DI_HDR = 32;            // ints per image header
constexpr int DI_CT = 256;            // threads of the compact kernel
constexpr int DI_PPT = 4;             // pixels per thread of the compact kernel
constexpr int DI_ST = 1024;           // threads of the select kernel
constexpr int DI_UNR = 4;             // values per thread in flight in the select kernel's passes (they are bound by load latency)
constexpr int DI_MAX_R = 8;
constexpr long DI_MAX_GRID = 1L << 20;  // workgroups per launch at most; beyond it the kernels walk their items / images with a grid stride
//                                        (more than 2^20 tiles or images: reachable inside B * H * W < 2^31, not exercised by the tests)

__device__ __forceinline__ int di_lane_prefix(unsigned long long m) {           // set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

template <bool U8>
__device__ __forceinline__ bool di_fg(const void* __restrict__ mask, long i) {
  if constexpr (U8) return ((const unsigned char*)mask)[i] != 0;
  else return ((const float*)mask)[i] != 0.f;                                    // (NaN != 0: foreground, as under .bool())
}

// work item (b, tile): pixels tile * 1024 + k * 256 + thread, k < 4, of image b; the items are walked with a grid stride
template <bool U8>
__global__ void __launch_bounds__(DI_CT) di_compact_kernel(const float* __restrict__ depth, const void* __restrict__ mask, int r,
                                                         int* __restrict__ hdr, float* __restrict__ vals, int H, int W,
                                                         int tiles, long items) {
  __shared__ int s_box[5];            // n_mask, W - xmin, H - ymin, xmax + 1, ymax + 1 of this workgroup
  __shared__ int s_wave[DI_CT / 64];
  __shared__ int s_base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int HW = H * W;
  for (long item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = (int)(item / tiles), tile = (int)(item - (long)b * tiles);
    const float* dep = depth + (long)b * HW;
    const long moff = (long)b * HW;
    if (tid < 5) s_box[tid] = 0;
    __syncthreads();

    bool valid[DI_PPT];
    float d[DI_PPT];
    int n_fg = 0, bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
#pragma unroll
    for (int k = 0; k < DI_PPT; ++k) {
      const long p = ((long)tile * DI_PPT + k) * DI_CT + tid;
      valid[k] = false;
      d[k] = 0.f;
      if (p < HW) {
        const int y = (int)(p / W), x = (int)(p - (long)y * W);
        if (di_fg<U8>(mask, moff + p)) {
          ++n_fg;
          bx0 = max(bx0, W - x);
          by0 = max(by0, H - y);
          bx1 = max(bx1, x + 1);
          by1 = max(by1, y + 1);
          d[k] = dep[p];
          bool ok = d[k] > 0.f;                                                  // drops NaN, 0 and negatives, keeps +inf
          if (ok && r > 0) {                                                     // the disk: taps outside the frame are foreground
            const int r2 = r * r;
            for (int dy = -r; dy <= r && ok; ++dy) {
              const int yy = y + dy;
              if (yy < 0 || yy >= H) continue;
              for (int dx = -r; dx <= r; ++dx) {
                const int xx = x + dx;
                if (dx * dx + dy * dy > r2 || xx < 0 || xx >= W) continue;
                if (!di_fg<U8>(mask, moff + (long)yy * W + xx)) {
                  ok = false;
                  break;
                }
              }
            }
          }
          valid[k] = ok;
        }
      }
    }

    // bounding box: butterfly over the wave, one LDS atomic per wave and value, then one global atomic per workgroup and value
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      n_fg += __shfl_xor(n_fg, o, 64);
      bx0 = max(bx0, __shfl_xor(bx0, o, 64));
      by0 = max(by0, __shfl_xor(by0, o, 64));
      bx1 = max(bx1, __shfl_xor(bx1, o, 64));
      by1 = max(by1, __shfl_xor(by1, o, 64));
    }
    if (lane == 0 && n_fg > 0) {
      atomicAdd(&s_box[0], n_fg);
      atomicMax(&s_box[1], bx0);
      atomicMax(&s_box[2], by0);
      atomicMax(&s_box[3], bx1);
      atomicMax(&s_box[4], by1);
    }

    // compaction: places inside the wave from the ballots, the waves' ranges from LDS, the workgroup's from one atomicAdd
    unsigned long long bal[DI_PPT];
    int n_wave = 0;
#pragma unroll
    for (int k = 0; k < DI_PPT; ++k) {
      bal[k] = __ballot(valid[k]);
      n_wave += __popcll(bal[k]);
    }
    if (lane == 0) s_wave[wave] = n_wave;
    __syncthreads();
    int* h = hdr + (long)b * DI_HDR;
    if (tid == 0) {
      int total = 0;
#pragma unroll
      for (int w = 0; w < DI_CT / 64; ++w) total += s_wave[w];
      s_base = total > 0 ? atomicAdd(&h[0], total) : 0;
      if (s_box[0] > 0) {
        atomicAdd(&h[1], s_box[0]);
        atomicMax(&h[2], s_box[1]);
        atomicMax(&h[3], s_box[2]);
        atomicMax(&h[4], s_box[3]);
        atomicMax(&h[5], s_box[4]);
      }
    }
    __syncthreads();
    int at = s_base;
    for (int w = 0; w < wave; ++w) at += s_wave[w];
    float* out = vals + (long)b * HW;
#pragma unroll
    for (int k = 0; k < DI_PPT; ++k) {
      const int slot = at + di_lane_prefix(bal[k]);
      if (valid[k] && slot < HW) out[slot] = d[k];                              // (slot < HW always: at most HW pixels are valid)
      at += __popcll(bal[k]);
    }
    __syncthreads();                                                             // s_box / s_wave / s_base are reused by the next item
  }
}

// key of value i: the bits of d (MAD = false) or of |d - med| (MAD = true); both are non-negative floats, which order like their bits
template <bool MAD>
__device__ __forceinline__ unsigned di_key(float d, float med) {
  if constexpr (MAD) return __float_as_uint(fabsf(d - med));
  else return __float_as_uint(d);
}

// The element of rank `rank` (0-based, < n) among the n keys, by all DI_ST threads of the workgroup.  s_hist: 256 ints, s_sel: 2.
template <bool MAD>
__device__ unsigned di_radix_select(const float* __restrict__ v, int n, int rank, float med, int* s_hist, int* s_sel) {
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned prefix = 0;
  constexpr int step = DI_ST * DI_UNR;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (long base = 0; base < n; base += step) {                               // (uniform: whole workgroups walk it, the ballots see every lane)
      float dv[DI_UNR];
#pragma unroll
      for (int u = 0; u < DI_UNR; ++u) {
        const long i = base + u * DI_ST + tid;
        dv[u] = i < n ? v[i] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < DI_UNR; ++u) {
        const unsigned key = di_key<MAD>(dv[u], med);
        const bool act = base + u * DI_ST + tid < n && (pass == 0 || (key >> (shift + 8)) == prefix);
        const unsigned digit = (key >> shift) & 255u;
        const unsigned long long am = __ballot(act);
        if (am != 0) {
          const int first = __ffsll((long long)am) - 1;
          const unsigned d0 = (unsigned)__shfl((int)digit, first, 64);
          const unsigned long long same = __ballot(act && digit == d0);
          if (same == am) {
            if (lane == first) atomicAdd(&s_hist[d0], __popcll(am));
          } else if (act) {
            atomicAdd(&s_hist[digit], 1);
          }
        }
      }
    }
    __syncthreads();
    if (tid < 64) {                                                              // the bucket that holds `rank`: lane l scans bins 4l .. 4l + 3
      const int c0 = s_hist[4 * lane], c1 = s_hist[4 * lane + 1], c2 = s_hist[4 * lane + 2], c3 = s_hist[4 * lane + 3];
      const int sum = c0 + c1 + c2 + c3;
      int incl = sum;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      const int excl = incl - sum;
      if (rank >= excl && rank < incl) {                                         // exactly one lane (0 <= rank < the pass's total)
        int rem = rank - excl, bin = 4 * lane;
        if (rem >= c0) {
          rem -= c0;
          ++bin;
          if (rem >= c1) {
            rem -= c1;
            ++bin;
            if (rem >= c2) {
              rem -= c2;
              ++bin;
            }
          }
        }
        s_sel[0] = bin;
        s_sel[1] = rem;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | (unsigned)s_sel[0];
    rank = s_sel[1];
    __syncthreads();                                                             // s_sel and s_hist are rewritten by the next pass
  }
  return prefix;
}

__global__ void __launch_bounds__(DI_ST) di_select_kernel(const int* __restrict__ hdr, const float* __restrict__ vals,
                                                         const float* __restrict__ intr, int intr_n, float m,
                                                         float* __restrict__ trans, float* __restrict__ stats,
                                                         int* __restrict__ counts, int B, int H, int W) {
  __shared__ int s_hist[256];
  __shared__ int s_sel[2];
  __shared__ unsigned s_kept[3];      // count, min bits, max bits
  const int tid = threadIdx.x, lane = tid & 63;
  const int HW = H * W;
  const float fnan = __int_as_float(0x7fc00000);
  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    const int* h = hdr + (long)b * DI_HDR;
    const float* v = vals + (long)b * HW;
    const int n = min(max(h[0], 0), HW);                                         // (never more than the row holds)
    const int n_mask = h[1];
    float med = fnan, mad = fnan;
    if (n > 0) {
      med = __uint_as_float(di_radix_select<false>(v, n, (n - 1) / 2, 0.f, s_hist, s_sel));
      // median +inf: inf - inf = NaN is among |d - median|, and the host's median propagates it
      if (med < INFINITY) mad = __uint_as_float(di_radix_select<true>(v, n, (n - 1) / 2, med, s_hist, s_sel));
    }
    if (tid == 0) {
      s_kept[0] = 0u;
      s_kept[1] = 0xffffffffu;
      s_kept[2] = 0u;
    }
    __syncthreads();
    if (n > 0 && mad == mad) {
      int cnt = 0;
      unsigned lo = 0xffffffffu, hi = 0u;
      for (long base = 0; base < n; base += DI_ST * DI_UNR) {
        float dv[DI_UNR];
#pragma unroll
        for (int u = 0; u < DI_UNR; ++u) {
          const long i = base + u * DI_ST + tid;
          dv[u] = i < n ? v[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < DI_UNR; ++u) {
          const float d = dv[u];
          if (base + u * DI_ST + tid < n && fabsf(d - med) / mad < m) {                  // one division, one compare: 0/0 and x/0 keep nothing
            ++cnt;
            lo = min(lo, __float_as_uint(d));
            hi = max(hi, __float_as_uint(d));
          }
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o, 64));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
      }
      if (lane == 0 && cnt > 0) {
        atomicAdd(&s_kept[0], (unsigned)cnt);
        atomicMin(&s_kept[1], lo);
        atomicMax(&s_kept[2], hi);
      }
    }
    __syncthreads();
    if (tid == 0) {
      const int n_kept = (int)s_kept[0];
      const float kmin = n_kept > 0 ? __uint_as_float(s_kept[1]) : fnan;
      const float kmax = n_kept > 0 ? __uint_as_float(s_kept[2]) : fnan;
      const float z = n_kept > 0 ? (kmin + kmax) / 2.0f : fnan;
      int xmin = -1, ymin = -1, xmax = -1, ymax = -1;
      float cu = fnan, cv = fnan;
      if (n_mask > 0) {
        xmin = W - h[2];
        ymin = H - h[3];
        xmax = h[4] - 1;
        ymax = h[5] - 1;
        cu = ((float)xmax + (float)xmin) / 2.0f;
        cv = ((float)ymax + (float)ymin) / 2.0f;
      }
      float* st = stats + (long)b * 8;
      st[0] = z;
      st[1] = med;
      st[2] = mad;
      st[3] = kmin;
      st[4] = kmax;
      st[5] = cu;
      st[6] = cv;
      st[7] = 0.f;
      int* ct = counts + (long)b * 8;
      ct[0] = n_mask;
      ct[1] = n;
      ct[2] = n_kept;
      ct[3] = xmin;
      ct[4] = ymin;
      ct[5] = xmax;
      ct[6] = ymax;
      ct[7] = 0;
      if (trans != nullptr) {
        const float* k = intr + (intr_n == 1 ? 0L : (long)b * 4);
        const float fu = k[0], fv = k[1], u0 = k[2], v0 = k[3];
        float* t = trans + (long)b * 3;
        if (n_kept > 0) {
          const float qx = (cu - u0) / fu, qy = (cv - v0) / fv;                  // a division, then a multiplication
          t[0] = __fmul_rn(qx, z);
          t[1] = __fmul_rn(qy, z);
          t[2] = z;
        } else {
          t[0] = t[1] = t[2] = fnan;
        }
      }
    }
    __syncthreads();                                                             // s_kept is reset by the next image
  }
}

inline bool di_aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

}  // namespace

extern "C" size_t lf_depth_init_scratch_bytes(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || (long)B * H * W > 0x7fffffffL) return 0;
  return (size_t)B * DI_HDR * sizeof(int) + (size_t)B * (size_t)H * (size_t)W * sizeof(float);
}

extern "C" int lf_depth_init(const float* depth, const void* mask, int mask_u8, const float* intr, int intr_n, float m,
                             int erode_radius, float* trans, float* stats, int* counts, void* scratch, size_t scratch_bytes,
                             int B, int H, int W, void* stream) {
  lf_clear_error();
  if (depth == nullptr || mask == nullptr || stats == nullptr || counts == nullptr || scratch == nullptr) return LF_EINVAL;
  if (B < 1 || H < 1 || W < 1 || (long)B * H * W > 0x7fffffffL) return LF_EINVAL;
  if (mask_u8 != 0 && mask_u8 != 1) return LF_EINVAL;
  if (erode_radius < 0 || erode_radius > DI_MAX_R || !(m > 0.f)) return LF_EINVAL;
  if ((intr == nullptr) != (trans == nullptr)) return LF_EINVAL;
  if (intr != nullptr && intr_n != 1 && intr_n != B) return LF_EINVAL;
  if (!di_aligned4(depth) || !di_aligned4(mask) || !di_aligned4(intr) || !di_aligned4(trans) || !di_aligned4(stats) ||
      !di_aligned4(counts) || (((uintptr_t)scratch) & 7u) != 0)
    return LF_EALIGN;
  if (scratch_bytes < lf_depth_init_scratch_bytes(B, H, W)) return LF_ENOSPC;
  hipStream_t s = (hipStream_t)stream;
  int* hdr = (int*)scratch;
  float* vals = (float*)(hdr + (size_t)B * DI_HDR);
  const hipError_t e = hipMemsetAsync(hdr, 0, (size_t)B * DI_HDR * sizeof(int), s);
  if (e != hipSuccess) return (int)e;
  const int HW = H * W;
  const int tiles = (int)(((long)HW + DI_CT * DI_PPT - 1) / (DI_CT * DI_PPT));
  const long items = (long)B * tiles;
  const unsigned grid1 = (unsigned)(items < DI_MAX_GRID ? items : DI_MAX_GRID);
  const auto kern = mask_u8 ? di_compact_kernel<true> : di_compact_kernel<false>;
  hipLaunchKernelGGL(kern, dim3(grid1), dim3(DI_CT), 0, s, depth, mask, erode_radius, hdr, vals, H, W, tiles, items);
  const int st = lf_launch_status();
  if (st) return st;
  const unsigned grid2 = (unsigned)((long)B < DI_MAX_GRID ? (long)B : DI_MAX_GRID);
  hipLaunchKernelGGL(di_select_kernel, dim3(grid2), dim3(DI_ST), 0, s, (const int*)hdr, (const float*)vals, intr, intr_n, m,
                     trans, stats, counts, B, H, W);
  return lf_launch_status();
}
