// What the resampler (resample.hip) and the deterministic splat (splat.hip) share: the lattice steps of a volume and the
// launch of a kernel template by map kind.  Everything sits in the unnamed namespace, as the kernels of both files do.
#pragma once
#include "lf_common.h"

namespace {

typedef __bf16 bf16x4r __attribute__((ext_vector_type(4)));

struct Steps { float w, h, d; };                              // 1/(W-1), 1/(H-1), 1/(D-1) (0 for size 1)

Steps make_steps(int D, int H, int W) {
  Steps st;
  st.w = W > 1 ? 1.0f / (float)(W - 1) : 0.f;
  st.h = H > 1 ? 1.0f / (float)(H - 1) : 0.f;
  st.d = D > 1 ? 1.0f / (float)(D - 1) : 0.f;
  return st;
}

}  // namespace

// KERNEL<LF_MAP_O2C> or KERNEL<LF_MAP_C2O> by `kind`, 256 threads, on stream s
#define LAUNCH_BY_KIND(KERNEL, GRID, ...)                                                                   \
  do {                                                                                                      \
    if (kind == LF_MAP_O2C) hipLaunchKernelGGL((KERNEL<LF_MAP_O2C>), GRID, dim3(256), 0, s, __VA_ARGS__);   \
    else                    hipLaunchKernelGGL((KERNEL<LF_MAP_C2O>), GRID, dim3(256), 0, s, __VA_ARGS__);   \
  } while (0)
