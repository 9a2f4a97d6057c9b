// The tile walk of the ring convolutions -- conv3d_c16_f16x3_kernel (conv_split.hip: the f16 hi / lo split and the bf16 form) and
// ring_multi_kernel (conv_gru.hip: NG output groups over one staged halo) -- written once and included by both, in eight
// sections (conv_split.hip's header describes the organisation):
//
//     template <...> __global__ void kernel(...) {
//       extern __shared__ ... smem[];  constexpr IN16, IN_SH, LDS_B (bytes of LDS to clear), NT (threads), NPW (halo pieces per wave)
//       tid, lane, wv, pz, ry, n, kg;  D, H, W, ntiles, tiles_x, tiles_y, tiles_z (kernel arguments, or references to them)
//     #define RING_WALK_SETUP
//     #include "ring_walk.inc"       // LDS zero fill, XCD-aware tile range [t_begin, t_end) (returns when empty), OOB, nvox, sample_bytes
//       ... weights; plane_bytes, in_plane_bytes, in_sample_bytes; the file's halo staging: foff[NPW], f_x, fetch_column(bx, by, bn),
//       stg[NPW] ...
//     #define RING_WALK_HALO
//     #include "ring_walk.inc"       // fetch_plane(z, on): NPW buffer loads of one z plane into stg[]
//       ... commit_plane(slot): the file's conversion of stg[] into ring slot `slot` ...
//     #define RING_WALK_PRIME
//     #include "ring_walk.inc"       // first tile (cx, cy, cz, cn); ring state rot; halo planes 0..3 of the first tile staged
//       ... lane_b; the file's epilogue: eoff[RYs], epi_column(bx, by, bn), struct Epi, epi_tile(E, bz, valid),
//       epi_part(E, acc, IC<row>, IC<part>) ...
//     #define RING_WALK_HEAD
//     #include "ring_walk.inc"       // accP = 0 (the previous tile's sums); (px_, py_, pz_, pn_)
//       for (int t = t_begin; t < t_end; ++t) {
//     #define RING_WALK_NEXT
//     #include "ring_walk.inc"       // tile t + 1 = (nx, ny, nz, nn), on, slide; per-column addressing when the previous / the next
//                                    // tile starts a column; Epi E and the previous tile's epilogue loads
//         fetch_plane(nz * TZs - 1 + (slide ? 2 : 0) + pz, on);  __builtin_amdgcn_sched_barrier(0);
//     #define RING_WALK_OPERANDS
//     #include "ring_walk.inc"       // operand base addresses aP / aQ / aR from rot
//         ... commit target; acc = 0; the file's product step with the parts of the previous tile's epilogue between its MFMAs;
//         commit of the incoming planes; lds_barrier_s() ...
//     #define RING_WALK_TURN
//     #include "ring_walk.inc"       // new column: rot + 4, planes 2, 3 fetched and committed, barrier; else rot + 2; accP = acc;
//                                    // step to tile t + 1
//       }
//     #define RING_WALK_LAST
//     #include "ring_walk.inc"       // the last tile's epilogue
//     }
//
// A section un-defines its own selector.  The lines between the sections stay with the kernels: they differ (staging, product
// step, epilogue), carry the f16x3 kernel's instrumentation (the SPLIT_ABL guard of the fetch, TS cycle stamps on both sides of
// the fetch and of the tile barrier), or sit between two shared parts in one kernel only -- and the ORDER of the statements is
// part of what is shared: moving lane_b in front of conv_split's bias load (64 changed lines over its 14 kernels) or acc = 0 in
// front of the commit target (987; 2,992 over conv_gru's 20) moved device code, so those lines stay where each kernel had them.
//
// The sharing is textual for the reason wino_ring.inc gives.  Tried as __forceinline__ functions over references and measured
// with tools/resample_isa_diff.py: the tile range, the operand bases and the eoff[] column offsets changed up to 2,700 lines
// in a kernel, the frame of the product loop (static_for over read / MFMA / epilogue-part hooks) 68 - 1,041.  What is shared
// as C++ (ring_tile.h) left every symbol of both files identical: the operand -> (row, pair) table op_row / op_pair, the
// whole-epilogue loop ring_epilogue, and the host side RingPlan.  conv_gru.hip names its argument struct's tile counts through
// references, which load at the point of use like conv_split's kernel arguments; copies into locals moved the loads.
// As text, all 35 symbols equal the two hand-written copies this file replaced (profiles/ring_shared_isa.txt).

#if defined(RING_WALK_SETUP)
#undef RING_WALK_SETUP
  // zero-weight K slots and the rows an operand reads past its wave's share meet whatever is in LDS: 0 * garbage
  // could be NaN, so everything starts as zeros (the planes hold finite values from then on)
  for (int i = tid; i < LDS_B / 16; i += NT) ((u32x4s*)smem)[i] = (u32x4s){0u, 0u, 0u, 0u};
  __syncthreads();

  // workgroups b, b+8, b+16, ... run on the same XCD (one L2 each): give them consecutive tile ranges so that the
  // halo columns shared by neighbouring ranges are fetched from HBM once
  const int nb = gridDim.x;
  const int lb = (nb % 8 == 0) ? (blockIdx.x % 8) * (nb / 8) + blockIdx.x / 8 : blockIdx.x;
  const int per = (ntiles + nb - 1) / nb;
  const int t_begin = lb * per;
  const int t_end = min(t_begin + per, ntiles);
  if (t_begin >= t_end) return;

  constexpr int OOB = (int)0x80000000;                    // per-lane offset of a voxel outside the volume: loads return 0, stores are dropped
  const long nvox = (long)D * H * W;
  const unsigned sample_bytes = (unsigned)(nvox * 64);

#elif defined(RING_WALK_HALO)
#undef RING_WALK_HALO
  // the plane itself is the instruction's SCALAR offset, and a plane outside [0, D) -- wave-uniform, every wave fetches one
  // plane -- gets a zero-sized descriptor
  auto fetch_plane = [&](int z, bool on) {
    const bool v = on && (unsigned)z < (unsigned)D;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)f_x, 0, v ? in_sample_bytes : 0u, 0x00020000);
    const int soff = v ? z * in_plane_bytes : 0;
#pragma unroll
    for (int k = 0; k < NPW; ++k) {
      if constexpr (IN16) {
        const u32x2s h = __builtin_amdgcn_raw_buffer_load_b64(rs, foff[k], soff, 0);
        stg[k] = (u32x4s){h[0], h[1], 0u, 0u};
      } else {
        stg[k] = __builtin_amdgcn_raw_buffer_load_b128(rs, foff[k], soff, 0);
      }
    }
  };

#elif defined(RING_WALK_PRIME)
#undef RING_WALK_PRIME
  // tile coordinates are stepped, not divided: (cx, cy, cz, cn) = tile t, (nx, ny, nz, nn) = tile t + 1
  int cx, cy, cz, cn;
  {
    int tt = t_begin;                                            // z fastest: a workgroup walks up columns of tiles
    cz = tt % tiles_z; tt /= tiles_z;
    cx = tt % tiles_x; tt /= tiles_x;
    cy = tt % tiles_y; cn = tt / tiles_y;
  }
  // ring state: halo plane hp (0..3) of the current tile sits in slot (rot + hp) % 6
  int rot = 0;
  fetch_column(cx, cy, cn);
  fetch_plane(cz * TZs - 1 + pz, true);
  commit_plane(pz);
  fetch_plane(cz * TZs + 1 + pz, true);
  commit_plane(2 + pz);
  lds_barrier_s();

#elif defined(RING_WALK_HEAD)
#undef RING_WALK_HEAD
  f32x4 accP[RYs];                                                // the previous tile's sums, finished under this tile's MFMAs
#pragma unroll
  for (int r = 0; r < RYs; ++r) accP[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int px_ = cx, py_ = cy, pz_ = cz, pn_ = cn;

#elif defined(RING_WALK_NEXT)
#undef RING_WALK_NEXT
    int nx = cx, ny = cy, nz = cz + 1, nn = cn;
    if (nz == tiles_z) { nz = 0; ++nx; }
    if (nx == tiles_x) { nx = 0; ++ny; }
    if (ny == tiles_y) { ny = 0; ++nn; }
    const bool on = t + 1 < t_end;
    const bool slide = on && nz != 0;
    // per-column addressing, recomputed when the previous tile (epilogue) / the next tile (halo) starts a column
    if (t == t_begin + 1 || (t > t_begin && pz_ == 0)) epi_column(px_, py_, pn_);
    if (on && nz == 0) fetch_column(nx, ny, nn);
    Epi E;
    epi_tile(E, pz_, t > t_begin);                     // (the previous tile's epilogue loads, requested first)

#elif defined(RING_WALK_OPERANDS)
#undef RING_WALK_OPERANDS
    // ---- operand base addresses of this wave: planes pz, pz+1 (pairs along z) and pz+2 ----
    const int s0 = mod6(rot + pz), s1 = mod6(s0 + 1), s2 = mod6(s1 + 1);
    const int aP = ((kg >> 1) ? s1 : s0) * PLANE_B + lane_b;
    const int aQ = s2 * PLANE_B + lane_b + (kg >> 1) * 32;
    const int aR = s2 * PLANE_B + lane_b + 2 * 32 + (kg >> 1) * (HXs * 32);

#elif defined(RING_WALK_TURN)
#undef RING_WALK_TURN
    if (on && !slide) {
      // bottom of a new column: what was fetched are its planes 0, 1 (now in slots rot+4, rot+5); planes 2, 3 go to
      // the slots this tile has just released (exposed once per column)
      rot = mod6(rot + 4);
      fetch_plane(nz * TZs + 1 + pz, true);
      commit_plane(mod6(rot + 2 + pz));
      lds_barrier_s();
    } else {
      rot = mod6(rot + 2);
    }
#pragma unroll
    for (int r = 0; r < RYs; ++r) accP[r] = acc[r];
    px_ = cx; py_ = cy; pz_ = cz; pn_ = cn;
    cx = nx; cy = ny; cz = nz; cn = nn;

#elif defined(RING_WALK_LAST)
#undef RING_WALK_LAST
  {
    if (t_end - t_begin == 1 || pz_ == 0) epi_column(px_, py_, pn_);
    Epi E;
    epi_tile(E, pz_, true);
    ring_epilogue(epi_part, E, accP);
  }

#else
#error "ring_walk.inc: define RING_WALK_SETUP, _HALO, _PRIME, _HEAD, _NEXT, _OPERANDS, _TURN or _LAST"
#endif
