/*
 * lf_hip.h -- C ABI of liblf_hip.so: the MI355X (gfx950) kernels behind the LatentFusion
 * reconstruct-and-render hot path.
 *
 * The reference (NVlabs/latentfusion) has no FFI layer: its hot path is a chain of ATen calls
 * issued from nn.Module.forward.  Each entry point below replaces one such chain; the
 * reference call sites are cited per function as latentfusion/<file>:<lines>.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data unless stated otherwise;
 *   - activations are channels-last: volumes [N][D][H][W][C], images [N][H][W][C]
 *     (the Python host mirror converts from/to the reference's NCDHW at its API boundary);
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, never synchronised;
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *     LF_E* code for rejected arguments (nothing is launched in that case);
 *   - no function keeps a pointer past its return; no hidden allocations: scratch space is
 *     passed in explicitly (see lf_*_scratch_bytes).
 */
#ifndef LF_HIP_H
#define LF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LF_ABI_VERSION 1

#define LF_EINVAL   (-1)   /* bad size / flag combination            */
#define LF_EALIGN   (-2)   /* pointer or channel count not aligned   */
#define LF_ENOSPC   (-3)   /* scratch buffer too small               */

/* epilogue flags of the conv entry points */
#define LF_EPI_LRELU     1u   /* y = max(y, slope*y)                                         */
#define LF_EPI_PIXELNORM 2u   /* y = y / sqrt(mean_c(y^2) + eps); also writes the norm       */
#define LF_EPI_ADD       4u   /* (prev_flags of lf_conv3d_c16_wino only) prev_y is an addend  */
#define LF_EPI_DOT       8u   /* (prev_flags of lf_conv1x1_bwd_data only, alone) gx is stored as it is; prev_norm is an OUTPUT:
                                 prev_norm[record] = sum_c gx[record][c] * prev_y[record][c] per 16-channel record            */

/* grid-map kinds of the 3-D resampler */
#define LF_MAP_O2C 0   /* bilinear polynomial map (ObjectToCameraTransform)                  */
#define LF_MAP_C2O 1   /* projective map (CameraToObjectTransform)                           */
#define LF_MAP_COEFS 20 /* floats per sample in the coefficient block of either kind         */

int lf_abi_version(void);

/* Name of the device the library is running on (for logs); returns 0 / hip error. */
int lf_device_name(char* buf, int buflen);

/* ------------------------------------------------------------------------------------------
 * 3-D resampling: out[n,z,y,x,:] = trilinear(vol[n or 0], g(n; x,y,z)), padding=border,
 * align_corners=False, i.e. F.grid_sample as used by
 *   ObjectToCameraTransform.forward   modules/geometry.py:669-690  (+ camera_coords :515-531)
 *   CameraToObjectTransform.forward   modules/geometry.py:625-657
 * The sampling grid is never materialised; it is evaluated per voxel from `coef`:
 *   LF_MAP_O2C: g = c0 + c1*a + c2*b + c3*k + c4*a*k + c5*b*k, (a,b,k) = (x/(W-1), y/(H-1),
 *               z/(D-1)) -- torch.linspace(0, 1, size), 0 on an axis of size 1 --,
 *               c_j = coef[n][3*j .. 3*j+2] (x,y,z components)                  -> 18 floats
 *   LF_MAP_C2O: l = (lx,ly,lz,1) with lx = -1 + 2x/(W-1) (lattice in [-1,1]),
 *               gx = (A0.l)/(A3.l), gy = (A1.l)/(A3.l), gz = A2.l, A_r = coef[n][4*r..] -> 16 floats
 * vol_n == 1 broadcasts one volume to all N samples (Photographer.decode, recon/models.py:489-494).
 * Output spatial size == input spatial size (D,H,W), channels C.
 */
int lf_resample3d_fwd(const float* vol, int vol_n, const float* coef, int kind,
                      float* out, int N, int D, int H, int W, int C, void* stream);

/* d(loss)/d(coef) for LF_MAP_O2C given gout = d(loss)/d(out): gcoef[n][18] (fixed-order,
 * deterministic two-stage reduction).  Replaces grid_sampler_3d_backward (grid part) plus the
 * autograd chain grid -> camera of modules/geometry.py:469-531,669-686.
 * scratch must hold lf_resample3d_bwd_coef_scratch_bytes(N,D,H,W) bytes. */
size_t lf_resample3d_bwd_coef_scratch_bytes(int N, int D, int H, int W);
int lf_resample3d_bwd_coef(const float* gout, const float* vol, int vol_n, const float* coef,
                           float* gcoef, void* scratch, size_t scratch_bytes,
                           int N, int D, int H, int W, int C, void* stream);
/* The same over N samples whose per-block voxel partition is the one a launch of part_n samples uses: every sample's 18
 * sums are bit-identical to lf_resample3d_bwd_coef called with N = part_n on a group containing it, whatever N is (the
 * multi-target pose loop launches T targets x part_n hypotheses and reproduces T single-target loops).  part_n >= 1;
 * NULL pointers -> LF_EINVAL.  scratch: lf_resample3d_bwd_coef_part_scratch_bytes(N, part_n, D, H, W) bytes. */
size_t lf_resample3d_bwd_coef_part_scratch_bytes(int N, int part_n, int D, int H, int W);
int lf_resample3d_bwd_coef_part(const float* gout, const float* vol, int vol_n, const float* coef,
                                float* gcoef, void* scratch, size_t scratch_bytes,
                                int N, int D, int H, int W, int C, int part_n, void* stream);

/* Several source volumes behind one launch: `vol` holds vol_n >= 1 channels-last volumes [vol_n][D][H][W][C] back to back and
 * `vol_idx` is a DEVICE array of N int32; sample i reads volume vol_idx[i].  The reference renders one object per call --
 * Photographer.decode expands its single volume over the N cameras, recon/models.py:489-494 -- so the hypotheses of several
 * objects (pose refinement of a whole scene, pose/estimation.py:52-143 once per object) take one decode each; this is the
 * form that expansion needs when row i of the batch belongs to object vol_idx[i].
 * Everything else is lf_resample3d_fwd / lf_resample3d_bwd_coef_part: per sample the same operations in the same order, so
 * sample i's output is bit-identical to lf_resample3d_fwd(vol + vol_idx[i]*D*H*W*C, vol_n = 1, ...) on that sample, and its
 * 18 sums to lf_resample3d_bwd_coef called with N = part_n on that volume.  The lf_set_tuning forms without an indexed kernel
 * (key 1 = 4, 5; key 2 other than 10) run the default form.
 * Checked before anything is launched: NULL pointers, vol_n < 1, part_n < 1 -> LF_EINVAL; vol_idx not 4-byte aligned ->
 * LF_EALIGN; a volume or output pointer that is not 16-byte aligned takes the scalar kernels, as above; scratch below
 * lf_resample3d_bwd_coef_indexed_scratch_bytes(N, part_n, D, H, W) -> LF_ENOSPC.  The TABLE's contents live on the device and
 * are not inspected by the host: the kernels clamp every entry into [0, vol_n), so a bad entry reads another volume, never
 * outside the buffer (the Python wrapper ops.volume_table rejects one with ValueError when it builds the table). */
int lf_resample3d_fwd_indexed(const float* vol, int vol_n, const int32_t* vol_idx, const float* coef, int kind,
                              float* out, int N, int D, int H, int W, int C, void* stream);
size_t lf_resample3d_bwd_coef_indexed_scratch_bytes(int N, int part_n, int D, int H, int W);
int lf_resample3d_bwd_coef_indexed(const float* gout, const float* vol, int vol_n, const int32_t* vol_idx, const float* coef,
                                   float* gcoef, void* scratch, size_t scratch_bytes,
                                   int N, int D, int H, int W, int C, int part_n, void* stream);

/* d(loss)/d(vol) (trilinear splat, fp32 atomics; training / encoder backward only).
 * gvol must be zero-initialised by the caller; with vol_n == 1 all samples accumulate into one
 * volume. */

/* The same gradient, DETERMINISTIC: contributions are accumulated as round(value * 2^K) with 64-bit integer atomics
 * (integer addition is associative, so the result does not depend on the order the hardware retires them) and
 * converted back in a second pass; K follows max|gout| (found by an order-independent atomic max) so that 2^24
 * contributions to one voxel cannot overflow -- the quantum is 2^-38 of the largest gradient.  gvol is overwritten.
 * scratch: lf_resample3d_bwd_vol_det_scratch_bytes(vol_n, D, H, W, C) bytes, 8-byte aligned. */
size_t lf_resample3d_bwd_vol_det_scratch_bytes(int vol_n, int D, int H, int W, int C);
int lf_resample3d_bwd_vol_det(const float* gout, const float* coef, int kind, float* gvol, int vol_n, void* scratch,
                              size_t scratch_bytes, int N, int D, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------------
 * He-equalised 3x3(x3) convolution with fused epilogue, stride 1, zero padding 1:
 *   y = conv(x, W) * he + bias ; [LeakyReLU(slope)] ; [PixelNorm over channels (eps)]
 * = Equalized.forward + nn.LeakyReLU + PixelNorm of one half of Block.forward
 *   modules/equalized.py:57-64, modules/blocks.py:152-158, modules/__init__.py:14-15.
 * dims = 3: x [N][D][H][W][Cin];  dims = 2: D must be 1.
 * wpack: weights re-laid-out by the host as [tap][CoutP][CinP], tap = (kz*3+ky)*3+kx (dims=2:
 *        ky*3+kx), CinP = Cin rounded up to 16, CoutP = lf_conv3x3_cout_padded(Cout), zero padded.
 * bias: [Cout] or NULL.  norm_out: [N*D*H*W] receives sqrt(mean_c(y^2)+eps) when
 * LF_EPI_PIXELNORM is set (needed by the backward), may be NULL otherwise.
 * LF_EPI_PIXELNORM requires Cout <= 64 here; wider layers use lf_pixelnorm_fwd afterwards.
 */
/* Padded cout count the host packer must use for wpack (multiple of the cout-tile group). */
int lf_conv3x3_cout_padded(int Cout);
int lf_conv1x1_cout_padded(int Cout);

int lf_conv3x3_fwd(const float* x, const float* wpack, const float* bias, float* y, float* norm_out,
                   int dims, int N, int D, int H, int W, int Cin, int Cout,
                   float he, unsigned flags, float slope, float eps, void* stream);

/* Pointwise (1x1 / 1x1x1) He-equalised convolution with the same epilogue, i.e. a GEMM over
 * pixels.  Used for InputBlock/OutputBlock (modules/blocks.py:78-133), FactorProjection2d3d
 * and FactorProjection3d2d (modules/geometry.py:711-749).
 * Input addressing is generalised so that the depth axis of a channels-last volume can be
 * folded into K without a copy: K = ksl * Cin; element (pixel p, k = s*Cin + c) is read from
 * x[n*x_batch_stride + s*x_slice_stride + p*Cin + c].  wpack: [CoutP][Kp] (K ordered s-major,
 * Kp = K rounded up to 16, CoutP = lf_conv1x1_cout_padded(Cout), zero padded).
 * Output addressing is generalised the same way: channel co of pixel p of sample n is written to
 *   y[n*y_batch_stride + (co / y_slice_channels)*y_slice_stride + p*y_row_stride + co % y_slice_channels]
 * (y_slice_channels >= Cout: plain channels-last rows; y_slice_channels = C: the output is
 * unfolded into Cout/C depth slices of a channels-last volume -- used by the projection backward).
 * LF_EPI_PIXELNORM requires Cout <= 128 here. */
int lf_conv1x1_fwd(const float* x, const float* wpack, const float* bias, float* y, float* norm_out,
                   int N, int P, int Cin, int ksl, long x_batch_stride, long x_slice_stride,
                   int Cout, long y_batch_stride, int y_row_stride, int y_slice_channels,
                   long y_slice_stride,
                   float he, unsigned flags, float slope, float eps, void* stream);
/* The same with every input slice scaled by a per-pixel factor first: element (p, k = s*Cin + c) is
 * x[...] * xscale[(n*ksl + s)*P + p], the product rounded to fp32 as a separate scaling pass would round it (Cin % 4 == 0).
 * Replaces `z = z * depth_weights_resized` ahead of the factor projection (reference recon/models.py:427-430 -> modules/
 * geometry.py:744-749) without the scaled volume (round 6; was lf_column_scale_fwd + lf_conv1x1_fwd). */
int lf_conv1x1_fwd_scaled(const float* x, const float* xscale, const float* wpack, const float* bias, float* y, float* norm_out,
                          int N, int P, int Cin, int ksl, long x_batch_stride, long x_slice_stride,
                          int Cout, long y_batch_stride, int y_row_stride, int y_slice_channels,
                          long y_slice_stride,
                          float he, unsigned flags, float slope, float eps, void* stream);

/* Data gradients of the two convolutions: gx = conv^T(gy) * he with the host-packed transposed
 * weights (taps flipped / in-out swapped).  When prev_y != NULL the epilogue backward of the layer
 * that PRODUCED this convolution's input (whose saved output is prev_y, norm prev_norm, epilogue
 * prev_flags) is folded into the store, i.e. the result is already dL/d(pre-activation) of that
 * layer and no separate lf_epilogue_bwd pass over the volume is needed.
 *   3x3: Cout (the producer's channel count) in {16, 32, 64}; a voxel's whole row of Cout channels lies in one workgroup's
 *        tiles, PixelNorm' takes its mean over all Cout channels and prev_norm is indexed by voxel, prev_norm[N*D*H*W].
 *   1x1: 16-channel records, y_slice_channels == y_row_stride == 16, Cout and the two y strides multiples of 16; PixelNorm'
 *        takes its mean over the record and prev_norm is indexed by record, prev_norm[offset of the record in gx / 16].
 * prev_norm is required with LF_EPI_PIXELNORM in prev_flags; prev_y must be 16-byte aligned. */
int lf_conv3x3_bwd_data(const float* gy, const float* wpack_t, float* gx, int dims, int N, int D, int H, int W,
                        int Cin, int Cout, float he, const float* prev_y, const float* prev_norm,
                        unsigned prev_flags, float slope, void* stream);
int lf_conv1x1_bwd_data(const float* gy, const float* wpack_t, float* gx, int N, int P, int Cin, int Cout,
                        long y_batch_stride, int y_row_stride, int y_slice_channels, long y_slice_stride,
                        float he, const float* prev_y, const float* prev_norm, unsigned prev_flags,
                        float slope, float* amax_out, void* stream);
/* (amax_out, optional: zero-initialised LF_AMAX_FLOATS-float buffer that receives max|gx| when prev_y != NULL;
 *  consumed by lf_conv3d_c16_split as amax_in.) */

/* Split-precision ("f16x3") variant of the fused conv3d 16->16 block and of its data gradient:
 * every fp32 operand is split on-chip into f16 hi + lo (22 mantissa bits) and the product is formed
 * from three f16 MFMAs accumulating in fp32 (a_hi*b_hi + a_hi*b_lo + a_lo*b_hi; dropped term <= 2^-22).
 * Same semantics / epilogue / fused previous-layer backward as lf_conv3x3_fwd / lf_conv3x3_bwd_data
 * for dims = 3, Cin = Cout = 16.  wsplit: [14 tap pairs][hi,lo][16 cout][32 = 2 taps x 16 cin] f16 (pairing from
 * lf_conv3d_c16_split_pairs),
 * lf_conv3d_c16_split_wpack_halfs() elements (host-packed).  amax_in (device scalar, may be NULL):
 * max-abs of x, used to pre-scale tiny gradient tensors by a power of two (undone exactly);
 * amax_out (may be NULL, zero-initialised by the caller): receives max-abs of the output.
 * Both are LF_AMAX_FLOATS-float buffers of partial maxima (one slot per 128-byte line; the maximum over the
 * buffer is the value): producers spread their atomic maxima over the slots, consumers reduce them. */
#define LF_AMAX_FLOATS 2048
size_t lf_conv3d_c16_split_wpack_halfs(void);
void lf_conv3d_c16_split_pairs(int* taps28);   /* tap indices (kz*9+ky*3+kx; -1 = zero) of the 14 K-slot pairs */
int lf_conv3d_c16_split(const float* x, const void* wsplit, const float* bias, float* y, float* norm_out,
                        int N, int D, int H, int W, float he, unsigned flags, float slope, float eps,
                        const float* prev_y, const float* prev_norm, unsigned prev_flags,
                        const float* amax_in, float* amax_out, void* stream);

/* Winograd F(2x2x2, 3x3x3) variant of the same fused 16 -> 16 conv3d step, all-fp32 arithmetic
 * (v_mfma_f32_16x16x4_f32 on G-transformed weights, B/A transforms on the fp32 VALU): 64 instead of
 * 216 multiplies per 2x2x2 outputs.  Same semantics / epilogue / fused previous-layer backward as
 * lf_conv3x3_fwd / lf_conv3x3_bwd_data for dims = 3, Cin = Cout = 16 (modules/blocks.py:152-158).
 * upack: lf_conv3d_c16_wino_upack_floats() floats, [4 z-freq a][16 (y,x)-freq b*4+c][4 k-chunks i][64 lanes l]
 *        = U[a][b][c][cout = l & 15][cin = (l >> 4) * 4 + i],  U = (G (x) G (x) G) w  with
 *        G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]  (host-packed, once per weight update).
 * amax_out (may be NULL, zero-initialised by the caller): receives max-abs of the output.
 * prev_flags == LF_EPI_ADD: forward form with an addend, y = epilogue(conv(x) * he + bias + prev_y), prev_y in
 * y's layout -- a convolution over concatenated inputs evaluated as a sum of 16-channel pieces (the ConvGRU
 * gates, modules/gru.py:37-42). */
size_t lf_conv3d_c16_wino_upack_floats(void);
int lf_conv3d_c16_wino(const float* x, const float* upack, const float* bias, float* y, float* norm_out,
                       int N, int D, int H, int W, float he, unsigned flags, float slope, float eps,
                       const float* prev_y, const float* prev_norm, unsigned prev_flags,
                       float* amax_out, void* stream);

/* The renderer's factor projection fused into the Winograd kernel of the LAST camera block (round 4).
 * Reference: Photographer.decode runs camera_blocks then FactorProjection3d2d (recon/models.py:417-437,
 * modules/geometry.py:731-749: view (N, C*D, H, W) -> 1x1 conv -> LeakyReLU -> PixelNorm); a workgroup of
 * lf_conv3d_c16_wino walks exactly the axis that projection contracts.
 *
 * lf_conv3d_c16_wino_projfwd = lf_conv3d_c16_wino (forward form, prev_y = NULL) followed by
 *   lf_conv1x1_fwd(y as (N, H*W, K = D*16), ..., Cout = 16, proj_he, proj_flags)  ->  zp (N, H, W, 16), pnorm (N*H*W or NULL)
 * in ONE launch: same operands, same accumulation order, bit-identical zp; y / norm_out are still written (the backward
 * pass needs them).  proj_wA: lf_conv3d_c16_wino_proj_pack_floats(D) floats, [D][64 lanes l][4 i]
 *   = Wp[cout = l & 15][k = d*16 + (l >> 4)*4 + i]   (Wp = the (16, D*16) matrix lf_conv1x1_fwd takes, depth-major K).
 */
size_t lf_conv3d_c16_wino_proj_pack_floats(int D);
int lf_conv3d_c16_wino_projfwd(const float* x, const float* upack, const float* bias, float* y, float* norm_out,
                               int N, int D, int H, int W, float he, unsigned flags, float slope, float eps,
                               const float* proj_wA, const float* proj_bias, float* zp, float* pnorm,
                               float proj_he, unsigned proj_flags, void* stream);

/* bf16 autocast policy of the training step (BASELINE cfg 5; the reference wraps Sculptor / Photographer.forward in
 * `autocast(enabled=self.training)`, recon/models.py:199,405).
 * lf_round_bf16: y = bf16(x) kept in fp32 containers (the autocast cast of an operand of the fp32-MFMA kernels: bf16 x bf16
 * products are exact in fp32, so those kernels then compute what a bf16 MFMA would). */
int lf_round_bf16(const float* x, float* y, long n, void* stream);
/* The fused 16 -> 16 conv3d block step under that policy: operands rounded to bf16 (RNE) while the halo is staged, products on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation, DIRECT convolution (a Winograd transform of bf16 data is not bf16-exact),
 * on the ring organisation of lf_conv3d_c16_split (column walk over 2 x 8 x 16 tiles, six z-plane slots
 * of bf16 halo in LDS, tap pairs per MFMA, the epilogue under the next tile's MFMAs).  round_out: 0 = fp32 epilogue on the
 * accumulator, 1 = y = epilogue(bf16(bf16(acc) * he) + bias) -- autocast's convolution returns a half tensor and `* he` stays in
 * half, the fp32 bias promotes the rest (modules/equalized.py:57-64); with flags = 0 and bias = NULL also its data gradient.  addend != NULL (bias = NULL, flags = 0,
 * round_out = 0): y = conv(x) * he + addend, the running sum of the ConvGRU gates evaluated without the channel
 * concatenation (modules/gru.py:31-40).
 * wpack: lf_conv3d_c16_ring_bf16_wpack_elems() bf16 values, [14 pairs][16 cout][32 = 2 taps x 16 cin], the tap pairs of
 * lf_conv3d_c16_split_pairs (a missing second tap = zeros). */
size_t lf_conv3d_c16_ring_bf16_wpack_elems(void);
int lf_conv3d_c16_ring_bf16(const float* x, const void* wpack, const float* bias, float* y, float* norm_out,
                            int N, int D, int H, int W, float he, unsigned flags, float slope, float eps,
                            const float* addend, int round_out, void* stream);
/* The same launch with the STORAGE type of its three volumes selectable (round 5: the training step keeps the 16-channel
 * tensors that only half-precision convolutions produce and consume as bf16 channels-last records, 32 B per voxel --
 * half the HBM bytes of the same arithmetic: the staging rounds an fp32 input to bf16 anyway).  io = OR of LF_IO_*:
 * LF_IO_IN_BF16: x is bf16; LF_IO_OUT_BF16: y is written as bf16 (RNE of the fp32 epilogue result);
 * LF_IO_ADDEND_BF16: addend is bf16 (needs addend != NULL).  norm_out stays fp32.  io = 0 is lf_conv3d_c16_ring_bf16. */
#define LF_IO_IN_BF16 1
#define LF_IO_OUT_BF16 2
#define LF_IO_ADDEND_BF16 4
int lf_conv3d_c16_ring_bf16_io(const void* x, const void* wpack, const float* bias, void* y, float* norm_out,
                               int N, int D, int H, int W, float he, unsigned flags, float slope, float eps,
                               const void* addend, int round_out, int io, void* stream);

/* MULTI-OUTPUT form of the bf16 ring convolution for the ConvGRU recurrence of the training step (round 6; reference
 * modules/gru.py:30-43 under recon/fusion.py:188-197, autograd of the same lines): ONE staged input volume x (bf16 records,
 * or fp32 with x_bf16 = 0) is convolved with `ngroups` (1 or 2) weight packs (wpack = the packs of
 * lf_conv3d_c16_ring_bf16 back to back) into `ngroups` outputs; per group g the epilogue is
 *     y_g = fma(conv_g, he, add_g)                       add_g fp32 or (LF_RING_ADD_BF16) bf16, NULL = no addend
 *     y_g = bf16(bf16(conv_g) * he)                      LF_RING_ROUND: what autocast's half-precision convolution returns
 * stored as fp32 or (LF_RING_OUT_BF16) bf16 records; addend_per_sample = 0: one addend volume for all N samples.
 * `extra` folds an element-wise stage of the recurrence into the epilogue of the convolution that owns the same voxels:
 *   LF_RING_EX_RH    (x = h: fp32, or its bf16 copy with e0 = the fp32 h; the LAST group = reset gate stored as bf16):
 *                    o2 = bf16(h * sigmoid(y_last as stored))
 *   LF_RING_EX_BLEND (ngroups 1, y_0 = candidate stored as bf16; e0 = h fp32, e1 = update pre-activation bf16):
 *                    o2 (fp32) = h (1 - u) + y_0 u,  u = sigmoid(e1)
 *   LF_RING_EX_ABWD  (group 0 = LF_RING_ROUND | LF_RING_ADD_BF16 with add_0 = reset pre-activation, NOT added;
 *                    e0 = h fp32, e1 = gh1 fp32): g = group 0's result is not stored; y_0 (bf16) = g h r (1 - r),
 *                    o2 (fp32) = e1 + g r,  r = sigmoid(add_0).  y_0 may alias add_0.
 *   LF_RING_EX_BLOCK (ngroups 1, flags LF_RING_ROUND | LF_RING_OUT_BF16; e0 = bias[16] fp32 or NULL, o2 = norms fp32 per voxel):
 *                    y_0 = PixelNorm(LeakyReLU(bf16(bf16(conv) * he) + bias)), slope 0.2, eps 1e-8: the Block step of
 *                    lf_conv3d_c16_ring_bf16_io (flags LRELU | PIXELNORM, round_out 1) with its epilogue at compile time.
 *   LF_RING_EX_PREV  (ngroups 1, bf16 x, flags LF_RING_ROUND | LF_RING_OUT_BF16: the data gradient of a 16 -> 16 layer) e0 = the
 *                    bf16 activation of the layer that PRODUCED this layer's input, e1 = its PixelNorm norms (fp32 per voxel):
 *                    y_0 = LeakyReLU'(PixelNorm'(g; e0, e1)) of the rounded result g, slope 0.2 -- that producer's pre-activation
 *                    gradient; o2 = fp32 scratch of 16 * (1 + 2 * #CUs) floats, zero-filled by the caller: o2[0..15] receives the
 *                    producer's bias gradient (sums of the un-rounded y_0, fixed order).  Autograd of modules/blocks.py:152-158.
 * In-place addends (y_g == add_g) are allowed.  Only the combinations the recurrence launches are instantiated (LF_EINVAL
 * otherwise): no extra with (bf16 x, 1 or 2 groups) or (fp32 x, 1 group); EX_RH and EX_ABWD with 1 or 2 groups; EX_BLEND with 1.
 * D*H*W*64 < 2^31. */
#define LF_RING_ADD_BF16 1u
#define LF_RING_OUT_BF16 2u
#define LF_RING_ROUND 4u
#define LF_RING_EX_NONE 0
#define LF_RING_EX_RH 1
#define LF_RING_EX_BLEND 2
#define LF_RING_EX_ABWD 3
#define LF_RING_EX_BLOCK 4
#define LF_RING_EX_PREV 5
int lf_conv3d_c16_ring_multi(const void* x, int x_bf16, const void* wpack, int ngroups,
                             void* y0, const void* add0, unsigned flags0, void* y1, const void* add1, unsigned flags1,
                             int extra, const void* e0, const void* e1, void* o2,
                             int N, int D, int H, int W, float he, int addend_per_sample, void* stream);
/* The LF_RING_EX_BLEND launch spelled out, with an optional second output: cand (bf16, may alias `addend`) = conv(rh) * he +
 * addend (bf16); h_new (fp32) = h (1 - u) + cand u, u = sigmoid(upre as stored, bf16); h_new_bf16 (or NULL) = the same state
 * rounded to bf16 -- what the next step's gate convolutions and the weight gradients stage, at half the bytes. */
int lf_conv3d_c16_ring_blend(const void* rh, const void* wpack, void* cand, const void* addend, const float* h, const void* upre,
                             float* h_new, void* h_new_bf16, int N, int D, int H, int W, float he, void* stream);

/* Winograd F(2x2x2,3x3x3) for wide (>= 64-channel) 3-D convolutions, stage 1: the input transform.  x channels-last;
 * V [64][T][Cin], T = lf_wino3d_tiles(N, D, H, W), frequency f = (a*4 + b)*4 + c (z, y, x).  Cin a multiple of 4.
 * Stages 2 + 3: lf_wino_fused_gemm below. */
long lf_wino3d_tiles(int N, int D, int H, int W);
int lf_wino3d_input_transform(const float* x, float* V, int N, int D, int H, int W, int C, void* stream);

/* Stages 2 + 3 of the wide Winograd convolution in ONE launch, on this library's own fp32-MFMA GEMM (no library GEMM on
 * the hot path): for every frequency f the product V[f] (T x Cin) . U2[f]^T is accumulated on v_mfma_f32_16x16x4_f32 and
 * folded straight into the 2^dims outputs of each tile (output transform A^T M A), then He scale, bias and LeakyReLU are
 * applied in the store -- M (8x / 4x the output) never reaches memory.  dims = 3: V [64][T][Cin] from
 * lf_wino3d_input_transform; dims = 2 (D = 1): V [16][T][Cin] from lf_wino2d_input_transform.
 * U2: [F][CoutP][Cin], CoutP = lf_wino_fused_cout_padded(Cout) (zero padded), U2[f][co][ci] = ((G (x) ..) w)[co][ci][f]
 * -- output-channel major so that both GEMM operands stream along the contraction axis.  Cin, Cout multiples of 4.
 * flags: LF_EPI_LRELU only; for PixelNorm run lf_pixelnorm_fwd on y afterwards (y is 1/8 resp. 1/4 of V);
 * | LF_OUT_DEPTH_INNER (dims = 3): y is written as [N][H][W][D][Cout] instead of [N][D][H][W][Cout] -- a pixel's depth column
 * of the last camera block becomes ONE contiguous row of D*Cout floats, so the factor projection 3-D -> 2-D that follows
 * (modules/geometry.py:744-749; K = D*Cout = 4096 in the released model) is a plain row-major GEMM.
 * Also the data gradient of the same convolution (transposed / flipped U2, flags = 0, bias = NULL).
 * Replaces Equalized.forward + LeakyReLU of modules/equalized.py:57-64, blocks.py:152-158 for >= 64-channel layers.
 * Problems with few tile / channel blocks are split over the frequencies (more workgroups): each part writes its raw
 * partial outputs to `scratch` (lf_wino_fused_scratch_bytes(...) bytes, 0 when no split is used) and a second launch
 * adds them in a fixed order and applies the epilogue -- deterministic, no atomics. */
#define LF_OUT_DEPTH_INNER 0x100u
int lf_wino_fused_cout_padded(int Cout);
size_t lf_wino_fused_scratch_bytes(int dims, int N, int D, int H, int W, int Cout);
int lf_wino_fused_gemm(const float* V, const float* U2, const float* bias, float* y, void* scratch, size_t scratch_bytes,
                       int dims, int N, int D, int H, int W, int Cin, int Cout, float he, unsigned flags, float slope,
                       void* stream);

/* The same over N samples taken as N / part_n parts of part_n consecutive samples, with the frequency split that a launch of
 * ONE part chooses (lf_resample3d_bwd_coef_part is the precedent): every output value is formed by exactly the operations,
 * in exactly the order, of lf_wino_fused_gemm called on its part alone with N = part_n and the same other arguments, whatever
 * N is -- so the multi-target pose loop's T x part_n rows reproduce T single-target loops bit for bit.  The frequency split
 * is the only thing lf_wino_fused_gemm takes from the batch that changes a bit (it groups the F frequency contributions into
 * the partial sums the finish launch adds); the workgroup shape, which does not, still follows the whole batch, and so do the
 * grid, the scratch and the finish: one GEMM launch plus at most one finish launch.  A shape forced with lf_set_tuning(3, v)
 * counts for the part as for the batch.  part_n = N issues exactly the launches of lf_wino_fused_gemm.
 * Returns LF_EINVAL for part_n <= 0 or N % part_n != 0, otherwise as lf_wino_fused_gemm, with
 * scratch: lf_wino_fused_scratch_bytes_part(...) bytes (>= lf_wino_fused_scratch_bytes, equal at part_n = N; 0 for bad
 * arguments); nothing is launched on an error. */
size_t lf_wino_fused_scratch_bytes_part(int dims, int N, int D, int H, int W, int Cout, int part_n);
int lf_wino_fused_gemm_part(const float* V, const float* U2, const float* bias, float* y, void* scratch, size_t scratch_bytes,
                            int dims, int N, int D, int H, int W, int Cin, int Cout, float he, unsigned flags, float slope,
                            int part_n, void* stream);

/* Row-major GEMM with the Block epilogue in the store, on the same fp32 MFMA (no library GEMM on the hot path):
 *   y[m][co] = epilogue( he * sum_k x[m][k] * W[co][k] + bias[co] )        m < M, co < Cout, k < K
 *   epilogue = [LeakyReLU(slope)] ; [PixelNorm over co (eps), norm_out[m] = sqrt(mean_co(y^2) + eps)]
 * Replaces FactorProjection3d2d.forward (view -> 1x1 conv -> LeakyReLU -> PixelNorm) of modules/geometry.py:744-749 with
 * Equalized.forward modules/equalized.py:57-64 and PixelNorm modules/__init__.py:14-15 on the ranking path, where it was a
 * library GEMM + ATen leaky_relu_ + lf_pixelnorm_fwd: one launch, PixelNorm over ALL output channels (lf_conv1x1_fwd stops
 * at 128, lf_wino_fused_gemm has none).
 * x: [M][K], row stride K -- the depth-innermost rows LF_OUT_DEPTH_INNER makes the last camera block write (K = D*C,
 * k = d*C + c).  y: [M][Cout].  bias: [Cout] or NULL.  norm_out: [M], or NULL (ignored without LF_EPI_PIXELNORM).
 * wpack: [CoutP][K] row-major, wpack[co][k] = W[co][k], rows Cout .. CoutP-1 zero, CoutP = lf_rows_gemm_cout_padded(Cout)
 * (16, 32, 64, 128, 192 or 256; 0 for a Cout outside the domain).
 * flags: LF_EPI_LRELU | LF_EPI_PIXELNORM as for lf_conv1x1_fwd.
 * One workgroup owns 128 rows and all Cout columns of them; the contraction of an output element runs over k in ONE order
 * that depends on K alone (no split over K, no atomics), so a row's result is bit-identical whatever M it is computed in
 * and the kernel is run-to-run identical.  Rows >= M are neither read nor written.
 * Domain: K >= 4, K % 4 == 0; 16 <= Cout <= 256, Cout % 4 == 0; 1 <= M <= 128 * (2^31 - 1) (the workgroup count is 32-bit,
 * addresses are 64-bit); x, wpack, y 16-byte aligned.  Returns LF_EINVAL for a NULL x / wpack / y, a size or flag outside
 * that, LF_EALIGN for a misaligned buffer; nothing is launched then. */
int lf_rows_gemm_cout_padded(int Cout);
int lf_rows_gemm_epi(const float* x, const float* wpack, const float* bias, float* y, float* norm_out,
                     long M, int K, int Cout, float he, unsigned flags, float slope, float eps, void* stream);

/* Split-precision ("f16x3") form of the 3-D wide Winograd convolution: the per-frequency products on
 * v_mfma_f32_16x16x32_f16, each fp32 product formed from three f16 products of hi / lo halves
 * (a*b ~= a_lo*b_hi + a_hi*b_lo + a_hi*b_hi, fp32 accumulation); otherwise the contract of lf_wino_fused_gemm for dims = 3.
 * Replaces Equalized.forward + LeakyReLU of modules/equalized.py:57-64, blocks.py:152-158 for >= 64-channel 3-D layers.
 * Split operands are stored as records of 32 channels, [32 hi halfs][32 lo halfs] (128 B), CinP = lf_wino_f16x3_cin_padded(Cin)
 * channels per row (zero padded).
 *   lf_wino3d_input_transform_f16x3: x channels-last [N][D][H][W][C] -> V [64][T][CinP/32][2][32] halfs (T = lf_wino3d_tiles),
 *     the fp32 transform of lf_wino3d_input_transform scaled by 2^eV, then split.  eV: 8 * amax * 2^eV in [2^11, 2^12) with
 *     amax = the maximum over the slots of amax_in (an LF_AMAX_FLOATS buffer holding a bound of max|x|, read on the device);
 *     amax_in = NULL: eV = 0.
 *   lf_wino_fused_f16x3_gemm: U2 [64][CoutP][CinP/32][2][32] halfs = the Winograd weights times 2^eU, split (host-packed,
 *     CoutP = lf_wino_fused_cout_padded(Cout)); amax_in: the buffer the transform read.  y = epilogue(he 2^-(eU+eV) M) with
 *     flags LF_EPI_LRELU | LF_OUT_DEPTH_INNER as for lf_wino_fused_gemm; data gradient with transposed / flipped packs,
 *     flags = 0, bias = NULL.  amax_out (may be NULL, zero-initialised by the caller): receives max|y|.  Small problems are
 *     split over the frequencies into `scratch` (lf_wino_fused_f16x3_scratch_bytes(...) bytes, 0 = no split) and summed in a
 *     fixed order.  Returns LF_EINVAL for a NULL operand, Cin / Cout not multiples of 4 or bad flags, LF_ENOSPC for missing
 *     or short scratch; nothing is launched then. */
int lf_wino_f16x3_cin_padded(int Cin);
int lf_wino3d_input_transform_f16x3(const float* x, const float* amax_in, void* V, int N, int D, int H, int W, int C, void* stream);
size_t lf_wino_fused_f16x3_scratch_bytes(int N, int D, int H, int W, int Cout);
int lf_wino_fused_f16x3_gemm(const void* V, const void* U2, int eU, const float* amax_in, const float* bias, float* y,
                             float* amax_out, void* scratch, size_t scratch_bytes, int N, int D, int H, int W, int Cin, int Cout,
                             float he, unsigned flags, float slope, void* stream);

/* 2-D counterpart, F(2x2,3x3): V [16][T][Cin], T = lf_wino2d_tiles(N, H, W), f = b*4 + c (y, x). */
long lf_wino2d_tiles(int N, int H, int W);
int lf_wino2d_input_transform(const float* x, float* V, int N, int H, int W, int C, void* stream);

/* Split-precision ("f16x3") form of the 2-D wide Winograd convolution, F(2x2,3x3): the 2-D decoder's >= 64-channel layers
 * (Equalized.forward + LeakyReLU of modules/equalized.py:57-64, blocks.py:152-158, 2-D).  Products and records as for
 * lf_wino_fused_f16x3_gemm; the input scale is chosen PER TILE by the transform, not from a bound held on the device.
 *   lf_wino2d_input_transform_f16x3: x channels-last [N][H][W][C] -> V [16][T][CinP/32][2][32] halfs (T = lf_wino2d_tiles,
 *     CinP = lf_wino_f16x3_cin_padded(C), zero padded) and eV [T] ints: the fp32 transform of lf_wino2d_input_transform times
 *     2^eV[t], eV[t] such that the tile's largest finite |V| times 2^eV[t] lies in [2^11, 2^12) (0 for an all-zero tile).
 *     Non-finite inputs stay non-finite in exactly the frequencies they reach.  x, V 16-byte, eV 4-byte aligned.
 *   lf_wino_fused2d_f16x3_gemm: U2 [16][CoutP][CinP/32][2][32] halfs = the Winograd weights times 2^eU, split (host-packed,
 *     CoutP = lf_wino_fused_cout_padded(Cout)); V, eV from the transform.  y [N][H][W][Cout] = epilogue(2^-eV[t] he 2^-eU M)
 *     with flags 0 or LF_EPI_LRELU (PixelNorm: lf_pixelnorm_fwd afterwards); data gradient with transposed / flipped packs,
 *     flags = 0, bias = NULL.  Small problems are split over the frequencies into `scratch`
 *     (lf_wino_fused2d_f16x3_scratch_bytes(...) bytes, 0 = no split) and summed in a fixed order.
 *   Both return LF_EINVAL for a NULL operand, a size < 1, Cin / Cout not multiples of 4 or bad flags, LF_EALIGN for a
 *   misaligned buffer, LF_ENOSPC for missing or short scratch; nothing is launched then. */
int lf_wino2d_input_transform_f16x3(const float* x, void* V, int* eV, int N, int H, int W, int C, void* stream);
size_t lf_wino_fused2d_f16x3_scratch_bytes(int N, int H, int W, int Cout);
int lf_wino_fused2d_f16x3_gemm(const void* V, const int* eV, const void* U2, int eU, const float* bias, float* y, void* scratch,
                               size_t scratch_bytes, int N, int H, int W, int Cin, int Cout, float he, unsigned flags, float slope,
                               void* stream);

/* Gate arithmetic of the convolutional GRU fuser, inference path (modules/gru.py:30-43; no tanh on the
 * candidate).  `rec` is the channels-last record [x | state] (rec_stride floats per voxel, state at
 * rec_off) that the gate convolutions read; upre / rpre = update / reset pre-activations, pre_stride floats
 * per voxel (one merged [update | reset] convolution: rpre = upre + Ch, pre_stride = 2*Ch; two 16-channel
 * Winograd convolutions: separate tensors, pre_stride = Ch).
 *   stage A: u = sigmoid(upre);  rec.state = h * sigmoid(rpre)
 *   stage B: h_out = h * (1 - u) + cand * u;  rec.state = h_out (rec may be NULL) */
int lf_gru_stage_a(const float* upre, const float* rpre, int pre_stride, const float* h, float* u, float* rec,
                   long nvox, int Ch, int rec_stride, int rec_off, void* stream);
int lf_gru_stage_b(const float* h, const float* u, const float* cand, float* h_out, float* rec, long nvox, int Ch,
                   int rec_stride, int rec_off, void* stream);
/* Backward of the two stages for the training path (autograd of modules/gru.py:37-43), plain arrays of n floats
 * (n % 4 == 0, 16-byte aligned):
 *   stage B: gh = g (1 - u), gu = g (cand - h), gc = g u
 *   stage A: gupre = gu u (1 - u), grpre = grh h r (1 - r), gh = grh r,  r = sigmoid(rpre) */
int lf_gru_stage_b_bwd(const float* g, const float* h, const float* u, const float* cand, float* gh, float* gu, float* gc,
                       long n, void* stream);
int lf_gru_stage_a_bwd(const float* gu, const float* grh, const float* u, const float* rpre, const float* h, float* gupre,
                       float* grpre, float* gh, long n, void* stream);
/* The ConvGRU recurrence of the TRAINING step sequenced explicitly (ops._GruFuse; autograd of recon/fusion.py:188-197 over
 * modules/gru.py:30-43): plain arrays of n values (n % 4 == 0, 16-byte aligned).  The state h, the gradient chain g / gh1 /
 * gh12 and the accumulators are fp32; rpre, upre, cand, rh and the gate gradients are fp32 (bf16 = 0) or bf16 (bf16 = 1).
 *   stage_a     rh = h sigmoid(rpre)
 *   stage_b     h_out = h (1 - u) + cand u,  u = sigmoid(upre)
 *   stage_b_bwd gh1 = g (1 - u); gupre = g (cand - h) u (1 - u); gc = g u; acc_u += gupre; acc_o += gc   (acc_* may be NULL)
 *   stage_a_bwd grpre = grh h r (1 - r); gh12 = gh1 + grh r, r = sigmoid(rpre); acc_r += grpre            (acc_r may be NULL) */
int lf_gru_train_stage_a(const void* rpre, const float* h, void* rh, long n, int bf16, void* stream);
int lf_gru_train_stage_b(const float* h, const void* upre, const void* cand, float* h_out, long n, int bf16, void* stream);
int lf_gru_train_stage_b_bwd(const float* g, const float* h, const void* upre, const void* cand, float* gh1, void* gupre,
                             void* gc, float* acc_u, float* acc_o, long n, int bf16, void* stream);
int lf_gru_train_stage_a_bwd(const void* grh, const void* rpre, const float* h, const float* gh1, void* grpre, float* gh12,
                             float* acc_r, long n, int bf16, void* stream);
/* dst[i] (+= if accumulate) sum over `views` bf16 arrays of n elements each (src = the arrays back to back), in order:
 * the sum over the recurrence's steps of a stored gate gradient (bias / coordinate-channel weight gradients). n % 4 == 0. */
int lf_sum_views_bf16(const void* src, float* dst, long n, int views, int accumulate, void* stream);

/* Storage-type variants of the 16-channel resampler for the training step (io bit 0: the source, bit 1: the destination is a
 * bf16 channels-last volume; same fp32 interpolation / same fixed-point sums as lf_resample3d_fwd / lf_resample3d_bwd_vol_det
 * with C = 16).  The splat runs in BINNED form: the output voxels are first listed under the source tiles their corners touch
 * (count / scan / fill, <= 8 entries per voxel), then one workgroup per tile adds exactly its lists into 64-bit LDS accumulators
 * -- same integers, bit-identical to the tile / atomic forms of lf_resample3d_bwd_vol_det (3.7 -> 2.5 ms at 8 x 128^3).  A volume
 * per sample (vol_n == N) is processed in passes of as many samples as 512 MB of lists hold; one shared volume (vol_n == 1)
 * needs all samples in one pass and otherwise takes the tile form.  scratch: lf_resample3d_bwd_vol_det_io_scratch_bytes. */
int lf_resample3d_fwd_io(const void* vol, int vol_n, const float* coef, int kind, void* out, int N, int D, int H, int W,
                         int io, void* stream);
size_t lf_resample3d_bwd_vol_det_io_scratch_bytes(int vol_n, int N, int D, int H, int W);
int lf_resample3d_bwd_vol_det_io(const void* gout, const float* coef, int kind, void* gvol, int vol_n, void* scratch,
                                 size_t scratch_bytes, int N, int D, int H, int W, int io, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depth-column composites of the renderer (channels-last volumes [N][D][H][W][C], P = H*W pixels).
 * A depth column is strided by P*C floats: lanes run along the contiguous (pixel, channel) axis, the depth axis is
 * split over the waves of a workgroup (and over 16-lane groups combined with wave shuffles for the single-channel
 * softmax), partials meet in LDS in a fixed order -> deterministic, no atomics.
 *   lf_column_reduce_sum_fwd   y[n][p][c] = sum_d x[n][d][p][c]        Photographer 'sum' projection,
 *                                                                       recon/models.py:436-437
 *   lf_column_reduce_sum_bwd   gx[n][d][p][c] = gy[n][p][c]
 *   lf_column_softmax_fwd      w = softmax_d(logits[n][d][p]) ; zdepth[n][p] = sum_d w * linspace(-1,1,D)[d]
 *                              (_compute_depth_weights + _depth_from_weight, recon/models.py:378-395);
 *                              weights or zdepth may be NULL
 *   lf_column_softmax_bwd      glogits = w * (t - sum_d w t),  t = gweights + gzdepth * linspace(-1,1,D)
 *                              (either gradient may be NULL)
 *   lf_column_scale_fwd/bwd    out[row][:] = z[row][:] * w[row]  (z * depth_weights_resized, models.py:427-430);
 *                              bwd: gz = gout * w, gw[row] = sum_c gout * z  (gz or gw may be NULL); C % 4 == 0 */
/* The 17th channel of the OCCLUSION module for the render-loop engine (recon/models.py:378-395 over modules/unet.py's input
 * block, blocks.py:78-91, and the U-Net's first 3x3x3 convolution, blocks.py:152-158), 16 latent channels: the 17-channel tensors
 * cat(z, depth coordinate) / input-block output are never built.
 *   lf_occ_input_fwd   t = LeakyReLU(W1 [z; d] + b1) for the 17 outputs, d = linspace(-1, 1, D)[plane]: ta (outputs 0..15,
 *                      channels-last [rows][16]) and t16 (output 16, [rows]).
 *                      w: [17][20] = W1 * he (row = output; 16 latent inputs, depth input at [16]), b: [20]
 *   lf_occ_conv17_fwd  pre[v][co] = sum_taps w27[tap][co] * t16[v + tap - 1], zero padding; w27: [kz*9 + ky*3 + kx][16] =
 *                      W2[co][16][kz][ky][kx] * he.  The addend (LF_EPI_ADD) of the lf_conv3d_c16_wino launch over ta.
 *   lf_occ_conv17_bwd  gp16[u] = LeakyReLU'(t16[u]) * sum_taps sum_co w27[tap][co] * g[u - (tap - 1)][co]
 *                      (both on v_mfma_f32_16x16x4_f32: the forward as a 16 x 27 by 27 x voxels product, the backward as
 *                      h[tap][voxel] = W g per z plane into LDS followed by the shifted sums)
 *   lf_occ_input_bwd   gz = g_zs * wocc[row] + W1[:16]^T (gta * LeakyReLU'(ta)) + W1[16] * gp16   (ta == NULL: gta already carries
 *                      LeakyReLU'(ta) -- the data gradient that produced it applied it, prev_y = ta; g_zs / wocc: the direct term of
 *                      the occlusion scaling z * wocc, both NULL to leave it out); prev_y != NULL: followed by the epilogue
 *                      backward of the layer that produced z (saved output prev_y, norm prev_norm, prev_flags), as in
 *                      lf_conv3x3_bwd_data */
int lf_occ_input_fwd(const float* z, const float* w, const float* b, float* ta, float* t16, int N, int D, long P, float slope,
                     void* stream);
int lf_occ_input_bwd(const float* gta, const float* ta, const float* gp16, const float* w, const float* g_zs, const float* wocc,
                     float* gz, long rows, float slope, const float* prev_y, const float* prev_norm, unsigned prev_flags,
                     void* stream);
/* lf_occ_input_bwd with the factor projection's data gradient recomputed instead of read (round 6): the direct term of the scaling is
 * ((Wp_d^T gp2d[n][pixel]) * he_p) * wocc[voxel] with wpack_t = the transposed projection pack lf_conv1x1_bwd_data takes
 * ([D * 16 rows (d, c)][16 cout]) and gp2d the (N, H*W, 16) gradient of the projection's pre-activation; gta must already carry
 * LeakyReLU'(ta) (the data gradient that produced it ran with prev_y = ta).  P % 16 == 0, N*D*P < 2^31. */
int lf_occ_input_bwd_proj(const float* gta, const float* gp16, const float* w, const float* gp2d, const float* wpack_t, float he_p,
                          const float* wocc, float* gz, int N, int D, long P, float slope,
                          const float* prev_y, const float* prev_norm, unsigned prev_flags, void* stream);
/* Gradient of the occlusion weights through `z * w` -> factor projection: gw[n][d][p] = sum_c z[n][d][p][c] * g_zs[n][d][p][c],
 * g_zs = (Wp_d^T gp2d[n][p]) * he_p recomputed on the matrix pipe (wpack_t, gp2d as for lf_occ_input_bwd_proj); one read of z. */
int lf_occ_weight_grad(const float* z, const float* gp2d, const float* wpack_t, float he_p, float* gw, int N, int D, long P, void* stream);
/* lf_occ_weight_grad followed by the depth softmax's backward in one launch: glogits[d] = w[d] * (gw[d] - sum_e w[e] gw[e]) per pixel
 * column (weights = the softmax output lf_column_softmax(_head)_fwd stored); no gw volume.  D <= 256, P % 16 == 0. */
int lf_occ_weight_grad_softmax_bwd(const float* z, const float* gp2d, const float* wpack_t, float he_p, const float* weights,
                                   float* glogits, int N, int D, long P, void* stream);
/* Data gradient of the occlusion module's 16 -> 1 output block (no activation) onto the 16-channel activation y that fed it, with
 * the LeakyReLU' / PixelNorm' of the layer that produced y (its norm, flags) applied in the store:
 *   g[v][c] = epilogue'( (gl[v] * w16[c]) * he )          (rows voxels; what lf_conv1x1_bwd_data(Cin = 1, prev_y = y) computes) */
int lf_occ_head_bwd(const float* gl, const float* w16, float he, const float* y, const float* norm, unsigned flags, float slope,
                    float* g, long rows, void* stream);
int lf_occ_conv17_fwd(const float* t16, const float* w27, float* pre, int N, int D, int H, int W, void* stream);
int lf_occ_conv17_bwd(const float* g, const float* t16, const float* w27, float* gp16, int N, int D, int H, int W, float slope,
                      void* stream);
int lf_column_reduce_sum_fwd(const float* x, float* y, int N, int D, long P, int C, void* stream);
int lf_column_reduce_sum_bwd(const float* gy, float* gx, int N, int D, long P, int C, void* stream);
int lf_column_softmax_fwd(const float* logits, float* weights, float* zdepth, int N, int D, long P, void* stream);
/* The same with the logits formed on the way in: logit[n][d][p] = (sum_c y[n][d][p][c] * w16[c]) * he + bias[0] over a channels-last
 * 16-channel volume y (the occlusion module's 16 -> 1 output block without activation, reference recon/models.py:378-388 over
 * modules/unet.py / blocks.py OutputBlock); the logits volume is not written.  D <= 256; y and w16 16-byte aligned. */
int lf_column_softmax_head_fwd(const float* y, const float* w16, const float* bias, float he, float* weights, float* zdepth,
                               int N, int D, long P, void* stream);
int lf_column_softmax_bwd(const float* weights, const float* gweights, const float* gzdepth, float* glogits,
                          int N, int D, long P, void* stream);
int lf_column_scale_fwd(const float* z, const float* w, float* out, long rows, int C, void* stream);
int lf_column_scale_bwd(const float* gout, const float* z, const float* w, float* gz, float* gw, long rows, int C,
                        void* stream);

/* View reductions of the fusers: z holds V per-view volumes of n floats each, `view_stride` floats apart (any
 * element order -- the output uses the same one).
 *   lf_fuse_views_fwd  kind = LF_FUSE_MEAN | MAX | ABSMAX (signed value of largest magnitude) | MEDIAN (lower median,
 *                      torch.median; V <= 64): PoolFuser / pool_tensor, recon/fusion.py:45-57, functional.py:47-49.
 *                      idx (may be NULL; unused for MEAN) receives the selected view per element.  A NaN in any view is
 *                      the result of every kind, as in torch (selections pick the first NaN view).
 *   lf_fuse_views_bwd  gz[v][i] = g[i] / V (MEAN) or g[i] * (v == idx[i]).
 *   lf_fuse_blend_fwd  BlendFuser.forward, recon/fusion.py:139-148: weights[v][row] = softmax_v(logits[v][row]),
 *                      out[row][:] = sum_v z[v][row][:] * weights[v][row]  (rows voxels, C % 4 == 0 channels-last;
 *                      logits / weights views `logit_view_stride` floats apart); weights may be NULL.
 *   lf_fuse_blend_bwd  gz[v] = g * w_v ; glogits_v = w_v (a_v - sum_u w_u a_u), a_v = sum_c g z_v (either may be NULL). */
#define LF_FUSE_MEAN   0
#define LF_FUSE_MAX    1
#define LF_FUSE_ABSMAX 2
#define LF_FUSE_MEDIAN 3
int lf_fuse_views_fwd(const float* z, float* out, int* idx, int kind, int V, long n, long view_stride, void* stream);
int lf_fuse_views_bwd(const float* g, const int* idx, float* gz, int kind, int V, long n, long view_stride, void* stream);
int lf_fuse_blend_fwd(const float* z, const float* logits, float* weights, float* out, int V, long rows, int C,
                      long z_view_stride, long logit_view_stride, void* stream);
int lf_fuse_blend_bwd(const float* g, const float* z, const float* weights, float* gz, float* glogits, int V, long rows,
                      int C, long z_view_stride, long logit_view_stride, void* stream);

/* Cell arithmetic of the convolutional LSTM fuser (modules/lstm.py:41-56): cc = conv([x, h]) holds the gate
 * pre-activations of a voxel as channel blocks [i | f | o | g] (channels-last record of 4*Ch floats);
 *   c' = sigmoid(f) c + sigmoid(i) tanh(g);  h' = sigmoid(o) tanh(c').
 * bwd: given gh = dL/dh' and gcn = dL/dc' (either may be NULL) -> gcc [nvox][4*Ch] and gc = dL/dc. */
int lf_lstm_cell_fwd(const float* cc, const float* c_cur, float* h_next, float* c_next, long nvox, int Ch, void* stream);
int lf_lstm_cell_bwd(const float* cc, const float* c_cur, const float* gh, const float* gcn, float* gcc, float* gc,
                     long nvox, int Ch, void* stream);

/* 2-D grid sampling of planar images, F.grid_sample(align_corners=False) semantics: the crop / zoom
 * (geometry.py:20-44,287-354; zeros padding), Camera.uncrop (geometry.py:261-285; border padding) and the
 * image-based-rendering warps (ibr.py:52-93).  img [N][C][H][W], grid [N][Ho][Wo][2] = (x, y) in [-1,1],
 * out / gout [N][C][Ho][Wo]; bilinear = 1 | 0 (nearest, round-half-even); border = 1 (replicate) | 0 (zeros).
 * bwd: gimg (zero-initialised by the caller, accumulated with float atomics) and/or ggrid may be NULL. */
int lf_grid_sample2d_fwd(const float* img, const float* grid, float* out, int N, int C, int H, int W, int Ho, int Wo,
                         int bilinear, int border, void* stream);
int lf_grid_sample2d_bwd(const float* img, const float* grid, const float* gout, float* gimg, float* ggrid,
                         int N, int C, int H, int W, int Ho, int Wo, int bilinear, int border, void* stream);

/* Fused depth-based reprojection of image-based rendering (ibr.py:11-93: depth_to_warp_field + reproject_views) for B
 * objects, Vo output and Vi input views, all planar fp32:
 *   image_in [B][Vi][C][H][W], depth_in [B][Vi][H][W] (metric z, used as it stands), depth_out [B][Vo][H][W] (normalised,
 *   denormalised with the output camera's znear - 0.01 / zfar + 0.01), mask_out [B][Vo][H][W] or NULL;
 *   image_re[b][o][i][c] at image_re + ((b*Vo + o)*Vi + i) * image_row_stride + c*H*W, depth_re[b][o][i] at depth_re + (same
 *   row) * depth_row_stride: C*H*W and H*W for packed outputs, (C+2)*H*W each with depth_re = image_re + C*H*W to land in the
 *   (B*Vo, Vi, C+2, H, W) input of the IBR generator (the plane after the depth is not touched).
 * Per (b, o, i, pixel): the output pixel of the linspace(0,1) viewport lattice is unprojected with its depth, carried to
 * object space and projected into input view i; image_in[b][i] is sampled there (bilinear, align_corners=False, zeros padding,
 * the taps of lf_grid_sample2d_fwd, also for a non-finite coordinate), and so is the transformed input depth, whose value at
 * each tap is formed from depth_in at that tap: unprojected, carried into output camera o, its z normalised with the OUTPUT
 * camera's bounds, clamped to [0,1] (NaN kept), *2-1.  With mask_out the stores are image_re * m and (depth_re + 1) * m - 1,
 * every operation rounded on its own.  No grid, point set or expanded image is materialised.  The coordinate chain runs in
 * fp64 on the fp32 records and is split into floor + offset before the fp32 sampling (at the zero-padded frame edge the value
 * changes by |image| per pixel; an fp32 chain would move that edge by several 1e-6 pixels at W = 32 already).
 * Records (floats, formed in fp64 on the host; ops.pack_ibr_cameras), vp = viewport (x0, y0, x1, y1).  The entries of the
 * coordinate chain are kept as TWO floats, v ~ rec[k] + rec[k + LF_IBR_*_SPLIT] (the fp32 rounding of v and the fp32 rounding of
 * the remainder), because a relative error e of that chain moves the sample by e*W pixels; the others are rounded once.
 *   pair_rec [B][Vo][Vi][LF_IBR_PAIR_FLOATS]: [0,12) rows N0, N1, N2 (4 floats each) of the 3x4 map  K_i E_i E_o^-1  (output
 *     camera -> object -> input image) with N0 := (N0 - vp_i.x0 N2) / (vp_i.x1 - vp_i.x0), N1 likewise in y, so that for the
 *     camera point P = (x, y, z, 1):  sample x = W * (N0.P)/(N2.P) - 0.5,  y = H * (N1.P)/(N2.P) - 0.5;  [16,28) their second
 *     floats;  [12,16) the z row of E_o E_i^-1 (input camera -> object -> output camera) as D = (row - (0,0,0,zn_o)) /
 *     (zf_o - zn_o): normalised depth before the clamp = D.P for the input-camera point P.  zn = znear - 0.01, zf = zfar + 0.01.
 *   in_rec [B][Vi][LF_IBR_VIEW_FLOATS], out_rec [B][Vo][LF_IBR_VIEW_FLOATS]: [0] ax = (vp.x1 - vp.x0)/fu, [1] bx = (vp.x0 - u0)/fu,
 *     [2] ay, [3] by likewise (camera x / z = ax * lattice + bx); out_rec also [4] = (zf - zn)/2, [5] = (zf + zn)/2
 *     (z = d*[4] + [5]) and at [8,14) the second floats of [0,6).  The rest is padding.
 * bwd: g_image_re [B][Vo][Vi][C][H][W] and g_depth_re [B][Vo][Vi][H][W], packed, either may be NULL (not both); with mask_out
 * they are the gradients of the masked outputs.  g_image_in and g_depth_in are accumulated with float atomics into buffers the
 * caller zeroed -- NOT run-to-run identical in the last bits; g_depth_out (through the sampling coordinate of both samples) is
 * summed over i and c in a fixed order inside one thread, without atomics -- run-to-run identical.  Any of the three may be
 * NULL.  Cameras are constants (no gradient); a tap whose normalised depth is outside [0,1] passes no gradient to depth_in.
 * LF_EINVAL and nothing launched: a NULL required pointer, a size below 1, a row stride below the packed row, H*W or the
 * number of 256-pixel blocks >= 2^31 - 1.  One 4-byte store per lane and plane: no alignment demands. */
#define LF_IBR_PAIR_FLOATS 32
#define LF_IBR_PAIR_SPLIT 16
#define LF_IBR_VIEW_FLOATS 16
#define LF_IBR_VIEW_SPLIT 8
int lf_ibr_reproject_fwd(const float* image_in, const float* depth_in, const float* depth_out, const float* mask_out,
                         const float* pair_rec, const float* in_rec, const float* out_rec, float* image_re, float* depth_re,
                         int B, int Vo, int Vi, int C, int H, int W, long image_row_stride, long depth_row_stride, void* stream);
int lf_ibr_reproject_bwd(const float* image_in, const float* depth_in, const float* depth_out, const float* mask_out,
                         const float* pair_rec, const float* in_rec, const float* out_rec, const float* g_image_re,
                         const float* g_depth_re, float* g_image_in, float* g_depth_in, float* g_depth_out,
                         int B, int Vo, int Vi, int C, int H, int W, void* stream);

/* Weight gradient of the He-equalised conv (training step; autograd of equalized.py:57-64):
 *   gw[tap][co][ci] = scale * sum_v gpre[v][co] * x[v + tap][ci],   tap = (kz*3 + ky)*3 + kx, zero padding,
 * dims = 3 (27 taps), 2 (9 taps, D = 1) or 0 (pointwise: one tap, rows = N*D*H*W).  x, gpre channels-last
 * [N][D][H][W][C]; gpre is the gradient w.r.t. the pre-activation (after lf_epilogue_bwd); scale = he.
 * x == NULL: all-ones single-channel input, i.e. gw[0][co][0] = sum_v gpre[v][co] (bias gradient, scale 1).
 * Deterministic: per-block partials in `scratch`, fixed-order fp64 sum.  Scratch: lf_conv_bwd_weight_scratch_bytes of the
 * same arguments (Cin = 0 for x == NULL), LF_ENOSPC and nothing launched below it.  A buffer of that size also serves
 * lf_conv_bwd_weight_bf16(_io) on the same shape (it is the larger of the two needs where both kernels apply). */
size_t lf_conv_bwd_weight_scratch_bytes(int dims, int N, int D, int H, int W, int Cin, int Cout);
int lf_conv_bwd_weight(const float* x, const float* gpre, float* gw, void* scratch, size_t scratch_bytes,
                       int dims, int N, int D, int H, int W, int Cin, int Cout, float scale, void* stream);
/* The same weight gradient on the bf16 MFMA (autocast policy of the training step; recon/models.py:199,405): x and gpre
 * are rounded to bf16 (RNE) as they are staged -- the identity on operands the policy has already rounded -- products
 * are exact, accumulation fp32, partials summed in a fixed order in fp64 like lf_conv_bwd_weight.
 * Domain: dims = 3, Cin = Cout = 16, N*D*H*W >= 8192, D*H*W*64 < 2^31 - 1 and (D+3)*H*W*64 < 2^32.
 * lf_conv_bwd_weight_bf16_scratch_bytes returns the scratch the entries below demand (LF_ENOSPC below it) inside the domain
 * and 0 outside it, where they return LF_EINVAL (the caller keeps lf_conv_bwd_weight for the rest); it asks nothing of the
 * device outside the domain. */
size_t lf_conv_bwd_weight_bf16_scratch_bytes(int dims, int N, int D, int H, int W, int Cin, int Cout);
int lf_conv_bwd_weight_bf16(const float* x, const float* gpre, float* gw, void* scratch, size_t scratch_bytes,
                            int dims, int N, int D, int H, int W, int Cin, int Cout, float scale, void* stream);
/* ... with x (io & 1) and / or gpre (io & 2) stored as bf16 channels-last records (see lf_conv3d_c16_ring_bf16_io). */
int lf_conv_bwd_weight_bf16_io(const void* x, const void* gpre, float* gw, void* scratch, size_t scratch_bytes,
                               int dims, int N, int D, int H, int W, int Cin, int Cout, float scale, int io, void* stream);
/* The same weight gradient (lf_conv_bwd_weight's math, layouts and output; autograd of equalized.py:57-64 /
 * modules/blocks.py:152-158 in train_reconstruct.py:421-535) for WIDE layers: any Cin, Cout >= 16 (ragged allowed), dims
 * 0 / 2 / 3, x != NULL (the bias gradient stays on lf_conv_bwd_weight).  LDS-staged fp32 MFMA over 64 x 64 channel tiles;
 * fp32 products are exact, so it also serves bf16-valued (autocast) operands.  Deterministic: per-run partials in
 * `scratch` (lf_conv_bwd_weight_wide_scratch_bytes; 0 for an unsupported shape), fixed-order fp64 sum.  Returns LF_EINVAL
 * for a NULL operand or an unsupported shape, LF_EALIGN for x / gpre / gw / scratch not 16-byte aligned, LF_ENOSPC for a
 * short scratch; nothing is launched and gw is not written then. */
size_t lf_conv_bwd_weight_wide_scratch_bytes(int dims, int N, int D, int H, int W, int Cin, int Cout);
int lf_conv_bwd_weight_wide(const float* x, const float* gpre, float* gw, void* scratch, size_t scratch_bytes,
                            int dims, int N, int D, int H, int W, int Cin, int Cout, float scale, void* stream);

/* Epilogue backward of a 16-CHANNEL layer for the training step: gp = LeakyReLU'(y) PixelNorm'(gy; y, norm) (flags says
 * which; flags = 0: gp = gy) with the bias gradient gbias[16] = column sums of the un-rounded gp folded into the same pass
 * (gbias = NULL: no sums; else scratch of lf_epilogue_bwd_c16_scratch_bytes(rows) bytes), fixed-order reduction.
 * io: bit 0 -- gy, bit 1 -- y, bit 2 -- gp are bf16 [rows][16] arrays instead of fp32 (see lf_conv3d_c16_ring_bf16_io).
 * Autograd of modules/blocks.py:152-158 + equalized.py:57-64. */
size_t lf_epilogue_bwd_c16_scratch_bytes(long rows);
int lf_epilogue_bwd_c16(const void* gy, const void* y, const float* norm, void* gp, float* gbias, void* scratch,
                        size_t scratch_bytes, long rows, unsigned flags, float slope, int io, void* stream);

/* The 2-D -> 3-D lift of the training step for 16 image channels and C0 = 16 volume channels as ONE kernel each way (round 6;
 * reference modules/geometry.py:711-731 FactorProjection2d3d + autograd, bf16 autocast policy): rows x [R = V*P][16] fp32
 * (bf16 values) -> pointwise conv to 16*S channels (channel = c*S + d), He scale, bias, LeakyReLU, PixelNorm over all 16*S
 * channels -> bf16 channels-last volume records (v, d, p) of 16 channels + norm[R]; the 16*S-channel row is never stored.
 * wtab: bf16 [S][16 c][16 cin] = W[c*S + d][cin]; btab: fp32 [S][16 c] or NULL.  R % 16 == 0, P % 16 == 0, R % P == 0.
 * Backward: gvol / yvol = gradient and saved volume (bf16 records), wtab_t: bf16 [S][16 cin][16 c]; gx [R][16] fp32 (rounded to
 * bf16 values if round_gx), gw [16*S][16] (scaled by he), gb [16*S]; S in {16, 32, 64, 128}; scratch of
 * lf_lift16_bwd_scratch_bytes(S) bytes (per-workgroup partials, summed in a fixed order: deterministic). */
int lf_lift16_fwd(const float* x, const void* wtab, const float* btab, void* vol, float* norm, long R, long P, int S,
                  float he, float slope, float eps, void* stream);
size_t lf_lift16_bwd_scratch_bytes(int S);
int lf_lift16_bwd(const void* gvol, const void* yvol, const float* norm, const float* x, const void* wtab_t, float* gx, float* gw,
                  float* gb, void* scratch, size_t scratch_bytes, long R, long P, int S, float he, float slope, int round_gx,
                  void* stream);

/* The 3-D -> 2-D factor projection of the training step's renderer for 16 volume channels and 16 output channels on the same
 * idea (reference modules/geometry.py:731-749 FactorProjection3d2d + autograd): vol = bf16 records (v, d, p); y fp32 rows
 * [R][16] = PixelNorm(LeakyReLU(he * sum_{c,d} W[o][c*S + d] vol + b)), norm [R].  wtab: bf16 [S][16 o][16 c].
 * Backward from gp (fp32 rows [R][16], rounded to bf16 inside): gxvol = bf16 records of he * W^T gp; gw [16][16*S] (scaled by
 * he); wtab_t: bf16 [S][16 c][16 o]; S in {16, 32, 64, 128}; deterministic (per-workgroup partials, fixed order). */
int lf_proj16_fwd(const void* vol, const void* wtab, const float* bias, float* y, float* norm, long R, long P, int S, float he,
                  float slope, float eps, void* stream);
size_t lf_proj16_bwd_scratch_bytes(int S);
int lf_proj16_bwd(const float* gp, const void* vol, const void* wtab_t, void* gxvol, float* gw, void* scratch, size_t scratch_bytes,
                  long R, long P, int S, float he, void* stream);

/* ---- pointwise 16 -> 16 layers of the training step (round 6; csrc/pw16.hip) ------------------------------------------------------------
 * 1x1x1 convolutions under the bf16 autocast + storage policy (the sculptor's output block, reference recon/models.py:143,222 over
 * modules/blocks.py:108-119): one v_mfma_f32_16x16x16_bf16 per 16 voxels instead of the 3x3x3 ring kernels with the weights on the
 * centre tap.  rows = N*D*H*W voxels, channels-last 16-channel records.
 *   lf_pw16_fwd   y = act( bf16(bf16(W x) * he) + bias ) stored as bf16; x in bf16 (x_bf16 = 1) or fp32 storage (rounded on load);
 *                 w_bf16 = bf16 [cout][cin]; flags: 0 or LF_EPI_LRELU
 *   lf_pw16_bwd   gx = bf16(bf16(W^T gy) * he) stored as bf16 (gx_bf16 = 1) or fp32; wt_bf16 = bf16 [cin][cout]; gy in bf16 storage;
 *                 gbias != NULL: also gbias[c] = sum over the voxels of gy[.][c] (per-workgroup partial sums in `scratch`, reduced in
 *                 a fixed order: deterministic) */
int lf_pw16_fwd(const void* x, int x_bf16, const void* w_bf16, const float* bias, float he, unsigned flags, float slope, void* y,
                long rows, void* stream);
size_t lf_pw16_bwd_scratch_bytes(long rows);
int lf_pw16_bwd(const void* gy_bf16, const void* wt_bf16, float he, void* gx, int gx_bf16, float* gbias, void* scratch,
                size_t scratch_bytes, long rows, void* stream);

/* Standalone PixelNorm over the last (channel) axis of [rows][C], in place allowed.
 * norm_out[rows] receives sqrt(mean+eps).  modules/__init__.py:14-15. */
int lf_pixelnorm_fwd(const float* x, float* y, float* norm_out, long rows, int C, float eps, void* stream);

/* Backward of the fused epilogue: given gy = dL/dy, the saved output y and norm, produce
 * dL/d(conv*he + bias) (the caller then runs the transposed convolution and applies he):
 *   flags = LRELU|PIXELNORM: gp = lrelu'(y) * (gy - y * mean_c(gy*y)) / norm
 *   flags = LRELU           : gp = lrelu'(y) * gy
 *   flags = PIXELNORM       : gp = (gy - y*mean_c(gy*y)) / norm
 * rows x C, channels-last; in place (gp == gy) allowed. */
int lf_epilogue_bwd(const float* gy, const float* y, const float* norm, float* gp,
                    long rows, int C, unsigned flags, float slope, void* stream);
/* The same, also publishing max|gp| into amax_out (zero-initialised LF_AMAX_FLOATS buffer; order-independent atomic max):
 * the input bound of a lf_wino3d_input_transform_f16x3 data-gradient launch.  y, gy, gp, amax_out must not be NULL. */
int lf_epilogue_bwd_amax(const float* gy, const float* y, const float* norm, float* gp,
                         long rows, int C, unsigned flags, float slope, float* amax_out, void* stream);

/* ---- latent loss term of the pose loop (csrc/latent.hip) ---------------------------------------------------------------------
 * Cosine distance between the projected latent zp [N][P][C] (channels-last, P = h*w) and the target's latent code zt, per
 * hypothesis (reference pose/estimation.py:111-114 over distances.py:5-9 = 1 - torch.cosine_similarity(.., eps = 1e-8)):
 *   dist = 1 - dot / (max(|zp|, eps) * max(|zt|, eps)),  dot = sum zp*zt over the row's P*C values.
 * zt is read through ELEMENT STRIDES (the form chosen of the two the kernel could take; no host-side conversion): value
 * (n, p, c) lives at zt[n*zt_sn + p*zt_sp + c*zt_sc], so an (N, C, h, w) tensor is passed as it is, NCHW-contiguous
 * (zt_sp = 1, zt_sc = P) or channels-last (zt_sp = C, zt_sc = 1; f32x4 loads when 16-byte aligned).  zt_n = 1 broadcasts one
 * code to all rows (zt_sn is then ignored), else zt_n = N.  Strides are >= 0.
 *   lf_latent_cosine_fwd   sums[N][4] = (dot, |zp|^2, |zt|^2, dist).  losses [N][8] (lf_pose_loss_fwd's layout) may be NULL; else
 *                          losses[n][5] = dist and losses[n][4] += w_latent * dist.  Two launches: per-workgroup partial sums
 *                          into `scratch` (lf_latent_cosine_scratch_bytes(N, P, C) bytes), then a fixed-order fp64 finish per
 *                          row; no float atomics.  A row's split into partial sums depends on (P, C) only: row i of a batch is
 *                          bit-identical to a call on that row alone.
 *   lf_latent_cosine_bwd_epi  gp = Epi'(g_in + gscale * d(dist)/d(zp); zp, norm, flags) in one launch: the addend of the latent
 *                          term joins the decoder's gradient g_in (NULL: the addend alone) at the projection's OUTPUT zp, then
 *                          the epilogue backward of lf_epilogue_bwd in its three forms, or flags = 0: the plain sum.
 *                          d(dist)/d(zp) = -( zt/(a b) - dot zp/(a^2 b |zp|) ), a = max(|zp|, eps), b = max(|zt|, eps): as
 *                          autograd of torch.cosine_similarity, whose clamp acts on the value only (|zp| = 0: no zp term).
 *                          `sums` is the forward's output; norm[N*P] is required with LF_EPI_PIXELNORM; gp == g_in allowed.
 * Domain: C % 4 == 0 (else LF_EALIGN), 4 <= C <= 256, P >= 1, N >= 1, N * slices < 2^31 (else LF_EINVAL); zp, g_in, gp, sums and
 * scratch 16-byte aligned (LF_EALIGN); a short scratch buffer is LF_ENOSPC.  Nothing is written in any of these cases. */
size_t lf_latent_cosine_scratch_bytes(int N, long P, int C);
int lf_latent_cosine_fwd(const float* zp, const float* zt, int zt_n, long zt_sn, long zt_sp, long zt_sc, float* sums,
                         float* losses, float w_latent, void* scratch, size_t scratch_bytes, int N, long P, int C,
                         void* stream);
int lf_latent_cosine_bwd_epi(const float* g_in, const float* zp, const float* norm, const float* zt, int zt_n, long zt_sn,
                             long zt_sp, long zt_sc, const float* sums, float gscale, float* gp, int N, long P, int C,
                             unsigned flags, float slope, void* stream);

/* ---- pose metrics on model point clouds (csrc/points.hip) ------------------------------------------------------------------
 * ADD-S's nearest-point search and the point-pair means of ADD / ADD-sym / proj2d, batched over camera pairs (reference
 * pose/metrics.py:79-109: compute_point_add, compute_point_add_s over best_distance, compute_point_proj2d).  Points are packed
 * xyz fp32 rows; strides are in floats and >= 0, and a stride of 0 shares one cloud between all batches / rows (one model
 * cloud, B camera pairs).
 *   lf_nn_dist   dist[b][i] = min_j |T1_b x1[b][i] - T2_b x2[b][j]|, i < M, j < Q, idx[b][i] = the smallest such j (int32),
 *                mean[b] = mean_i dist[b][i].  T1 / T2: NULL or [B][12] row-major 3x4 affine maps, applied in fp32 as
 *                fmaf(t0, x, fmaf(t1, y, fmaf(t2, z, t3))) per row.  dist, idx and mean may each be NULL, not all three.
 *                Distances are coordinate differences, squared and summed (one multiply, two fmaf), the minimum taken over
 *                d^2 and one root per query: not the Gram form |a|^2 + |b|^2 - 2ab of torch.cdist, which loses 3e-3 .. 1.4e-2
 *                of a nearest distance on a model cloud in fp32.  A query's dist and idx bits depend on that query and its
 *                batch's candidates only (not on B, M, its place in the batch or the run); an exact tie returns the smallest
 *                j.  mean: one fp64 partial sum per 64 consecutive queries into `scratch` (lf_nn_dist_scratch_bytes(B, M, Q) bytes,
 *                needed only with mean), then a fixed-order fp64 finish per batch, no atomics; mean[b] does not depend on B.
 *                NaN: a query with a NaN coordinate gets dist = NaN and idx = -1, the other queries are untouched; a NaN among
 *                a batch's candidates makes every query of that batch NaN / -1 (as torch.min would), the other batches are
 *                untouched.  INFINITE coordinates, and finite ones whose squared differences overflow, are outside the
 *                contract (no fault; dist is then inf or NaN and idx may be -1).
 *   lf_points_pair_dist   mean[r] = mean_p |dehom(A_r (x_p, 1)) - dehom(Bm_r (x_p, 1))|, r < R, p < P; A, Bm: [R][rows][4]
 *                row-major.  rows = 4 divides by the fourth component and compares 3-D points (ADD with obj_to_cam), rows = 3
 *                divides by the third and compares 2-D points (proj2d with the 3x4 obj_to_image).  One launch plus the same
 *                fixed-order finish; scratch: lf_points_pair_dist_scratch_bytes(R, P) bytes; a row's mean does not depend on R.
 * Domain: B, M, Q, R, P >= 1, B * M < 2^31, R <= 65535, rows in {3, 4}, required pointers not NULL (else LF_EINVAL); every
 * pointer 4-byte aligned and scratch 8-byte aligned (LF_EALIGN; the kernels read the packed rows with 4-byte loads and keep
 * fp64 partial sums in scratch); a short scratch buffer is LF_ENOSPC.
 * Nothing is launched or written in any of these cases. */
size_t lf_nn_dist_scratch_bytes(int B, int M, int Q);
int lf_nn_dist(const float* x1, long x1_sb, const float* T1, const float* x2, long x2_sb, const float* T2, float* dist, int* idx,
               float* mean, void* scratch, size_t scratch_bytes, int B, int M, int Q, void* stream);
size_t lf_points_pair_dist_scratch_bytes(int R, int P);
int lf_points_pair_dist(const float* pts, long pts_sr, const float* A, const float* Bm, int rows, float* mean, void* scratch,
                        size_t scratch_bytes, int R, int P, void* stream);

/* ---- initial pose from depth and mask (csrc/depth_init.hip) -------------------------------------------------------------------
 * The translation the estimators start from, for B frames in one call (reference pose/initialization.py:8-86:
 * _masks_to_viewports, _erode_mask, _reject_outliers_mad, _estimate_camera_dist, estimate_translation): the centre of the mask's
 * bounding box and the mid-range of the MAD-filtered masked depth.
 *   depth [B][H][W] fp32; mask [B][H][W], fp32 (mask_u8 = 0) or bytes (mask_u8 = 1), foreground iff != 0 (a NaN is foreground,
 *   as under .bool()); intr [intr_n][4] = (fu, fv, u0, v0), intr_n = 1 (shared) or B; intr and trans are both given or both
 *   NULL (intr_n is then ignored).
 * Per image b, all in fp32:
 *   1. (xmin, ymin, xmax, ymax) = bounding box of the foreground of the UN-eroded mask, n_mask its pixel count,
 *      cu = (xmax + xmin) / 2, cv = (ymax + ymin) / 2.
 *   2. a pixel is valid iff it is foreground and depth > 0 (drops NaN, 0 and negatives, keeps +inf) and, with
 *      erode_radius = r > 0, every tap (dx, dy), dx^2 + dy^2 <= r^2, that lies inside the frame is foreground (taps outside
 *      count as foreground): the erosion the reference computes and, by its guard, discards -- r = 0 reproduces the reference.
 *   3. median = the valid depth of rank (n_valid - 1) / 2 (the lower median, as torch.median).
 *   4. mad = the value of the same rank among |d - median|; NaN when median is +inf (inf - inf is then among them).
 *   5. d is kept iff |d - median| / mad < m: one division, one compare, so 0/0 and x/0 keep nothing.
 *   6. z = (min_kept + max_kept) / 2.
 *   7. trans[b] = ((cu - u0) / fu * z, (cv - v0) / fv * z, z): a division, then a multiplication.
 *   stats[b][8]  = (z, median, mad, min_kept, max_kept, cu, cv, 0)
 *   counts[b][8] = (n_mask, n_valid, n_kept, xmin, ymin, xmax, ymax, 0)
 * Degenerate images are reported, never a fault: n_mask = 0 gives the box (-1, -1, -1, -1) and cu = cv = NaN; n_valid = 0
 * gives median = mad = NaN; n_kept = 0 gives z = min_kept = max_kept = trans[b] = NaN.  Subnormal depths are outside the
 * contract.  A memset and two launches whatever B is: a compaction pass (bounding box and valid depths into scratch, integer
 * atomics only) and one workgroup per image that finds both medians by an 8-bit-digit radix select on the bit patterns.  Every
 * output is an order statistic, a minimum / maximum, a count or one correctly rounded operation on those: the bits depend on
 * the image alone, not on B, the run or the order in which the atomics arrive.
 * Domain: B, H, W >= 1, B * H * W < 2^31, 0 <= erode_radius <= 8, m > 0 (a NaN m is refused), mask_u8 in {0, 1}, intr_n in
 * {1, B}, required pointers not NULL (else LF_EINVAL); every pointer 4-byte aligned and scratch 8-byte aligned (LF_EALIGN);
 * fewer than lf_depth_init_scratch_bytes(B, H, W) bytes of scratch is LF_ENOSPC (the query returns 0 outside the domain).
 * Nothing is launched or written in any of these cases. */
size_t lf_depth_init_scratch_bytes(int B, int H, int W);
int lf_depth_init(const float* depth, const void* mask, int mask_u8, const float* intr, int intr_n, float m, int erode_radius,
                  float* trans, float* stats, int* counts, void* scratch, size_t scratch_bytes, int B, int H, int W,
                  void* stream);

/* ---- evaluation point clouds from depth maps (csrc/depth_points.hip) ------------------------------------------------------------
 * Observation.pointcloud (reference observation.py:292-316 over pointcloud.py:57-79 project_pointcloud / compute_point_mask):
 * back-projection of the viewport lattice, segmentation by re-projection into the mask, ordered compaction.
 *   depth [B][H][W] fp32; mask [B][H][W], fp32 (mask_u8 = 0) or bytes (mask_u8 = 1), foreground iff != 0, NULL allowed with
 *   segment = 0; color [B][3][H][W] fp32 or NULL (colors is then NULL too); cams [B][LF_DEPTH_CAM_FLOATS], one record per view,
 *   formed by the caller in fp64 from the camera and rounded once:
 *     [0] vx, [1] vy (viewport xmin, ymin), [2] vw, [3] vh (viewport width, height), [4] fu, [5] fv, [6] u0, [7] v0,
 *     [8..19] cam_to_obj, [20..31] obj_to_image, both 3x4 row-major.
 *   points [cap][3], colors [cap][3] or NULL, index [cap] int32 or NULL, counts [B] int32; cap = B * H * W.
 * Per pixel (b, y, x) with z = depth[b][y][x], every step ONE correctly rounded fp32 operation in this order:
 *   1. u = fmaf(vw, x / (W - 1), vx), and u = vx for W = 1; v = fmaf(vh, y / (H - 1), vy), v = vy for H = 1.
 *   2. px = ((u - u0) / fu) * z, py = ((v - v0) / fv) * z, pz = z: a subtraction, a division, a multiplication.
 *   3. to_object = 1: (px, py, pz) <- rows of cam_to_obj, each fmaf(t0, px, fmaf(t1, py, fmaf(t2, pz, t3))); to_object = 0 keeps
 *      the camera-frame point.
 *   4. segment = 1: (h0, h1, h2) = rows of obj_to_image applied to the point of step 3 by the same chain -- whatever to_object
 *      is, as the reference does -- and u' = h0 / h2, v' = h1 / h2.  The pixel is kept iff z != 0, both quotients are finite,
 *      trunc(u') in [0, frame_w), trunc(v') in [0, frame_h) and mask[b][trunc(v')][trunc(u')] != 0 (trunc: toward zero, so
 *      -1 < u' < 0 reads column 0, as .long() does).
 * ZERO DEPTH: a pixel whose depth is exactly 0 is never kept under segment.  This is the one departure from the reference,
 * where such a pixel back-projects to the camera centre and its re-projection is 0/0 in exact arithmetic: rounding noise in
 * fp32 (finite garbage of a few pixels), so the reference keeps or drops it by accident.
 * Output: the kept pixels' points in the order of their source index b * H * W + y * W + x (view-major, then row-major), packed
 * from row 0; index[row] = that source index, colors[row] = color[b][0..2][y][x]; counts[b] = kept pixels of view b.  Rows from
 * sum(counts) on are not written.  segment = 0: every pixel is written at its own index, counts[b] = H * W, one launch.
 * Compaction without atomics: launch 1 writes the kept count of every chunk of 1024 consecutive pixels of a view into scratch;
 * launch 2 adds up the counts of the chunks before its own in a fixed order, ranks its kept pixels by a wave ballot and writes
 * the rows.  points, colors, index and counts are bit-identical from run to run, and a view's rows depend on that view alone
 * (the other views only shift them).
 * Domain: B, H, W >= 1, B * H * W < 2^31, mask_u8, to_object, segment in {0, 1}, color and colors both given or both NULL,
 * required pointers (depth, cams, points, counts; mask with segment) not NULL, and with segment (frame_h, frame_w) == (H, W) --
 * the reference indexes the H x W mask with frame pixels and raises IndexError otherwise (else LF_EINVAL); every pointer
 * 4-byte aligned (LF_EALIGN); with segment, fewer than lf_depth_points_scratch_bytes(B, H, W) bytes of scratch is LF_ENOSPC (the
 * query returns 0 outside the domain).  Nothing is launched or written in any of these cases. */
#define LF_DEPTH_CAM_FLOATS 32
size_t lf_depth_points_scratch_bytes(int B, int H, int W);
int lf_depth_points(const float* depth, const void* mask, int mask_u8, const float* color, const float* cams, float* points,
                    float* colors, int* index, int* counts, void* scratch, size_t scratch_bytes, int B, int H, int W, int frame_w,
                    int frame_h, int to_object, int segment, void* stream);

/* ---- farthest-point sampling (csrc/fps.hip) -------------------------------------------------------------------------------------
 * Greedy farthest-point sampling of B clouds (reference three/utils.py:4-49 farthest_points with F.pairwise_distance, as
 * tools/dataset/moped_eval_pointclouds.py and the BOP / RealSense readers call it).  x: packed xyz fp32 rows [B][N][3], x_sb the
 * batch stride in floats, 0 shares one cloud (as lf_nn_dist).  centers [B][K] int32, owner [B][N] int32, nearest [B][N] fp32;
 * each may be NULL, not all three.
 * Arithmetic, every operation one correctly rounded fp32 operation, never contracted:
 *   d^2(i, c) = (dx * dx + dy * dy) + dz * dz, dx = x_i - x_c (direct differences, as lf_nn_dist; NOT F.pairwise_distance,
 *   which adds 1e-6 to every coordinate difference: the two agree except at near-ties).
 *   min_i starts at 1e14f (the reference's 1e7, squared) and is held on d^2.
 *   pick k = the SMALLEST index among the maxima of min before update k (so pick 0 is row 0); centers[b][k] = pick k.
 *   update k: owner[i] = k whenever d^2(i, pick k) <= min_i (the last centre that attains the minimum wins, as
 *   clusters[distances == new_distances] = i does), then min_i = min(min_i, d^2).
 *   nearest[i] = sqrt(min_i) after the K updates, one correctly rounded root.
 * The maximum is exact and ties go to the smallest index, so no reduction order shows: the two forms give the same bits.
 *   form 1, resident: one workgroup per cloud, the coordinates and running minima in LDS (16 bytes per point) for all K picks of
 *     ONE launch, one workgroup barrier per pick.  N <= LF_FPS_RESIDENT_MAX = (160 KiB - 256 bytes of reduction slots) / 16;
 *     above that form 1 is LF_EINVAL.  No scratch.
 *   form 2, streamed: any N.  One launch per pick over ceil(N / 1024) workgroups per cloud; each first reduces the previous
 *     launch's per-workgroup partial maxima from scratch in a fixed order (so all derive the same pick), updates its slice of
 *     the running minima (in scratch) and writes its own partial.  K launches, and one more that takes the roots when nearest
 *     is asked for, queued back to back.
 *   form 0: resident iff N <= LF_FPS_RESIDENT_MAX -- by N alone, so a cloud's result and path do not depend on B.
 * No kernel waits for another workgroup.  NaN / infinite coordinates and differences beyond 1e7 are outside the contract: no
 * fault, result unspecified.
 * Domain: B >= 1, 1 <= K <= N, B * N < 2^31, x_sb >= 0, form in {0, 1, 2} (else LF_EINVAL); every pointer 4-byte aligned
 * (LF_EALIGN); the streamed form with fewer than lf_farthest_points_scratch_bytes(B, N, K, form) bytes of scratch is LF_ENOSPC
 * (the query returns 0 for the resident form and outside the domain).  Nothing is launched or written in any of these cases. */
#define LF_FPS_RESIDENT_MAX 10224
size_t lf_farthest_points_scratch_bytes(int B, int N, int K, int form);
int lf_farthest_points(const float* x, long x_sb, int* centers, int* owner, float* nearest, void* scratch, size_t scratch_bytes,
                       int B, int N, int K, int form, void* stream);

/* ---- training losses (csrc/train_loss.hip) --------------------------------------------------------------------------------------
 * The loss tail of the generator's training step in three launches forward and one backward, no device-to-host copy, no float
 * atomics (reference losses.py:33-57 HardPixelLoss, losses.py:94-99 beta_prior_loss, train_reconstruct.py:491-521 the terms).
 * Two parts; either may be absent, not both.
 * Hard-pixel part (absent when x = NULL; B, C, H, W, base, k and the part's other pointers are then ignored):
 *   x, y [B][C][H][W] fp32; base 0 = L1, 1 = smooth-L1 with beta 1; l[b][p] = mean_c base(x, y), every operation rounded on
 *   its own (no FMA contraction): L1 |x - y|; smooth-L1 d = |x - y|, d < 1 ? 0.5f * d * d : d - 0.5f.  For C = 1 these are the
 *   bits of F.l1_loss / F.smooth_l1_loss(reduction='none'); for C > 1 the channels are added in the order 0 .. C-1 and divided
 *   by C.  A NaN loss counts as the positive quiet NaN, above +inf.
 *   k = 0: no mining, the term is the mean over all B*C*H*W elements.  1 <= k <= H*W: per image the k largest l[b][.] are
 *   kept and the term is their mean over B*k.  One radix select per image on the bit patterns gives thresh[b] = t_b, the k-th
 *   largest value, sel[b][2] = (n_gt = the count above it, n_tie = k - n_gt); of the pixels equal to t_b the n_tie of lowest
 *   pixel index are kept.  img_sum[b] = the kept sum of image b.  (k = 0: thresh = 0, sel = (H*W, 0).)  An image's sum is split
 *   by (H, W) alone and finished in fp64: image b of a batch has the bits of a call on that image alone.
 * Mask part (absent when mlogit = NULL; Mn, alpha, beta, log_beta are then ignored): mlogit = z, mtarget = t [Mn] fp32.
 *   mask_recon = mean of max(z, 0) - z * t + log1p(exp(-|z|)).
 *   mask_beta  = mean of clamp(-((alpha - 1) * log(clamp(m, 1e-4)) + (beta - 1) * log(clamp(1 - m, 1e-4)) - log_beta), min 0),
 *   m = sigmoid(z) rounded to fp32 and 1 - m formed from that value; log_beta = lgamma(alpha) + lgamma(beta) -
 *   lgamma(alpha + beta) comes from the host.  Elements in fp32, sums in fp64 in an order that follows Mn alone.
 * terms[4] = (recon, mask_recon, mask_beta, 0) on the device, 0 for an absent part.
 * lf_recon_loss_bwd reads g_terms[3] = d/d(terms) FROM DEVICE MEMORY and the forward's thresh and sel and writes
 *   gx [B][C][H][W]: exactly 0 outside the selection, inside g_terms[0] / (B*k*C) * base' (B*H*W*C for k = 0), base' =
 *   sign(x - y) for L1 and for smooth-L1 at d >= 1, (x - y) otherwise;
 *   gmlogit [Mn] = g_terms[1] * (m - t) / Mn + g_terms[2] * dbeta/dm * m * (1 - m) / Mn, dbeta/dm zero where the outer clamp is
 *   active and, per factor, where its inner clamp is.
 *   One workgroup per image walks the pixels in index order (the tied pixels are ranked by a ballot prefix count), so two
 *   calls give the same bits.
 * Scratch: lf_recon_loss_scratch_bytes(B, C, H, W, Mn) bytes; B = C = H = W = 0 there stands for an absent hard-pixel part,
 * Mn = 0 for an absent mask part.  It returns 0 outside the domain and never touches the device.
 * Domain (else LF_EINVAL): terms, scratch (fwd), g_terms (bwd) and the pointers of every present part not NULL; a part
 * present; B, C, H, W >= 1, C <= 4, H*W < 2^31 - 1, 0 <= k <= H*W, base in {0, 1}; 1 <= Mn <= 2^40; ceil(B*H*W / 256) +
 * ceil(Mn / 2048) and B + ceil(Mn / 4096) workgroups at most 2^31 - 1.  Every pointer 4-byte aligned, scratch 8-byte aligned
 * (LF_EALIGN).  Less scratch than the query says is LF_ENOSPC.  Nothing is launched or written in any of these cases. */
size_t lf_recon_loss_scratch_bytes(int B, int C, int H, int W, long Mn);
int lf_recon_loss_fwd(const float* x, const float* y, int base, int k, const float* mlogit, const float* mtarget, float alpha,
                      float beta, float log_beta, float* thresh, int* sel, float* img_sum, float* terms, void* scratch,
                      size_t scratch_bytes, int B, int C, int H, int W, long Mn, void* stream);
int lf_recon_loss_bwd(const float* g_terms, const float* x, const float* y, int base, int k, const float* thresh, const int* sel,
                      const float* mlogit, const float* mtarget, float alpha, float beta, float log_beta, float* gx,
                      float* gmlogit, int B, int C, int H, int W, long Mn, void* stream);

/* ---- observation preprocessing (csrc/obs_prepare.hip) ---------------------------------------------------------------------------
 * Observation.zoom -> prepare -> normalize for B frames in ONE launch, whatever B is; no scratch, no atomics (reference
 * modules/geometry.py:20-44,287-354 crop_to_viewport / Camera.zoom, observation.py:225-282 zoom / prepare / normalize,
 * recon/models.py Sculptor.encode for the stacked form).
 *   color [B][C][H][W] fp32 (C >= 0; color and color_out are ignored and may be NULL when C = 0); depth [B][H][W] fp32;
 *   mask [B][H][W], fp32 (mask_u8 = 0) or bytes (mask_u8 = 1; a byte counts as its value converted to float); boxes [B][4] =
 *   (x0, y0, x1, y1) in frame pixels, fp32 ON THE DEVICE, the un-truncated viewport of Camera.zoom_viewport; zn, zf [B]: the
 *   camera's znear - 0.01 and zfar + 0.01 (required with LF_OBS_NORMALIZE, otherwise ignored); T: the target size.
 *   stages: LF_OBS_PREPARE | LF_OBS_NORMALIZE, any combination; the crop always runs.
 * Lattice of frame b, per axis (x: corners x0, x1, size W, index i = output column; y: y0, y1, H, output row), every
 * operation rounded on its own in fp32 unless it says fp64:
 *   1. c0 = truncf(x0), c1 = truncf(x1)                           (quirk Q15: toward zero; equals the host's fp64 trunc)
 *   2. start = (float)((double)c0 / (double)W), end = (float)((double)c1 / (double)W)      (one fp64 division each)
 *   3. T = 1: l = start.  T > 1: step = (end - start) / (float)(T - 1)                     (a subtraction, an IEEE division);
 *      i <  T / 2 (integer division):  l = start + step * (float)i                         (a multiplication, an addition)
 *      i >= T / 2:                     l = end - step * (float)(T - 1 - i)                 (a multiplication, a subtraction)
 *      so point 0 is exactly start and point T - 1 exactly end whenever step is finite, as in every linspace; the bits in
 *      between are this form's own, NOT those of ATen's linspace.
 *   4. g = l * 2, then g - 1                                        (the grid value of F.grid_sample, align_corners=False)
 * Per output pixel (row oy, column ox) the pixel coordinate is lf_unnorm2d(g) and the taps, their validity under zeros
 * padding and the bilinear weights come from csrc/sample2d_taps.h exactly as in lf_grid_sample2d_fwd: colour is bilinear,
 * depth and mask are nearest (round-half-even).  A non-finite coordinate takes whatever that header yields; nothing is ever
 * read outside the frame, and each frame is read only where its box lies.  Then, with m the CROPPED mask value, every
 * operation rounded separately:
 *   LF_OBS_PREPARE    colour: c * 2, - 1, * m, + 1, / 2, clamp [0, 1]         (gan_denormalize(gan_normalize(c) * m))
 *                     depth:  d * m
 *   LF_OBS_NORMALIZE  colour: c * 2, - 1                                        (gan_normalize)
 *                     depth:  d - zn, / (zf - zn) (one subtraction per frame, one IEEE division), clamp [0, 1], * 2, - 1
 *   clamp is torch.clamp: a NaN stays NaN.  The mask output is the cropped mask under every stage.
 * Outputs: color_out [B][C][T][T], depth_out [B][T][T], mask_out [B][T][T].  stack (optional, NULL = none): the encoder input
 * written directly, row b at stack + b * stack_row_stride (in floats, >= the planes written) holds the planes
 * [colour (C) | depth if stack_depth = 1 | mask * 2 - 1] of T * T floats each, with the values of the three outputs; floats of
 * a row beyond those planes are not touched.
 * Domain: B, H, W, T >= 1, C >= 0, mask_u8 and stack_depth in {0, 1}, no stage bit beyond the two, zn and zf given with
 * LF_OBS_NORMALIZE, required pointers not NULL, B * max(C, 1) * H * W < 2^31 and B * (C + 2) * T^2 < 2^31 (else LF_EINVAL);
 * every pointer 4-byte aligned (LF_EALIGN).  Nothing is launched or written in any of these cases. */
#define LF_OBS_PREPARE   1
#define LF_OBS_NORMALIZE 2
int lf_obs_prepare(const float* color, const float* depth, const void* mask, int mask_u8, const float* boxes, const float* zn,
                   const float* zf, float* color_out, float* depth_out, float* mask_out, float* stack, long stack_row_stride,
                   int stack_depth, int B, int C, int H, int W, int T, int stages, void* stream);

/* Block-end rescale by exactly x2 (up = 1) or x0.5 (up = 0): nearest (linear = 0) or bi-/tri-linear
 * with align_corners=False (linear = 1) = Interpolate / F.interpolate(scale_factor=...) of
 * modules/__init__.py:18-36, blocks.py:160-162.  x: [N][D][H][W][C] (D = 1 for dims = 2); the output
 * extent is 2*in or floor(in/2) per spatial axis.  lf_resize_bwd is the exact adjoint (gather form). */
int lf_resize_fwd(const float* x, float* y, int dims, int N, int D, int H, int W, int C, int linear, int up,
                  void* stream);
int lf_resize_bwd(const float* gy, float* gx, int dims, int N, int D, int H, int W, int C, int linear, int up,
                  void* stream);

/* ------------------------------------------------------------------------------------------
 * Camera -> coefficient blocks, with Jacobian (fp64 forward-mode duals inside).
 * Replaces the chain of tiny ops log_quaternion -> qexp -> normalize -> quat_to_mat -> cam_to_obj ->
 * camera_coords (three/quaternion.py:39-93,287-311; modules/geometry.py:106-153,207-213,469-531)
 * plus the viewport / depth-range algebra of Camera.uncrop and denormalize_depth (:261-285,555-558).
 *   params     [N][10] = (log_quaternion 3, translation 3, viewport xmin,ymin,xmax,ymax)
 *   intrinsics [N][4]  = (fu, fv, u0, v0)
 *   coefs      [N][24] : [0..17] LF_MAP_O2C block; [18..21] (ax,bx,ay,by): crop sample position of
 *                         frame pixel (x,y) is (ax*x+bx, ay*y+by); [22..23] (a,b): depth = d*a + b
 *   jac        [N][24][10] = d coefs / d params
 * lf_camera_coefs_bwd: gparams[N][10] = sum_j gcoefs[N][j] * jac[N][j][:]. */
#define LF_CAM_PARAMS 10
#define LF_CAM_COEFS  24
int lf_camera_coefs(const float* params, const float* intrinsics, float cube_size, float z_span,
                    int crop_h, int crop_w, float* coefs, float* jac, int N, void* stream);
int lf_camera_coefs_bwd(const float* gcoefs, const float* jac, float* gparams, int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused pose loss = default_pose_loss (pose/estimation.py:70-118, pose/utils.py:81-117) over
 * Photographer.interpret_logits(apply_mask=True) (recon/models.py:455-484), Camera.uncrop
 * (nearest for depth, bilinear for mask logits, border padding) and denormalize_depth.
 *   logits  [N][h*w][2]  head outputs (depth_logit, mask_logit), channels-last
 *   coefs   [N][24]      from lf_camera_coefs (entries 18..23 are used)
 *   target_depth/mask [H*W] of the (single) target frame; weights[4] = (depth, ov_depth, iou, mask)
 *   sums    [N][8]  S0..S6 (sum l1, sum l1*sig*mt, sum sig*mt, sum sig, intersection, sum mt*valid, sum bce)
 *   losses  [N][8]  (depth, ov_depth, iou, mask, weighted total, 0,0,0)
 *   gsums   [N][8]  d(mean_n total)/d(sums), consumed by lf_pose_loss_bwd
 * lf_pose_loss_bwd writes glogits [N][h*w][2] and gcoefs[N][24] entries 18..23 (0..17 untouched).
 * All reductions are fixed-order (no float atomics).  scratch: lf_pose_loss_scratch_bytes.
 * One argument check serves the eight entry points below, and nothing is launched on a rejected call: a NULL pointer,
 * N < 1, h <= 1, w <= 1, H <= 0 or W <= 0 -> LF_EINVAL; scratch_bytes below lf_pose_loss_scratch_bytes -> LF_ENOSPC. */
size_t lf_pose_loss_scratch_bytes(int N, int h, int w, int H, int W);
int lf_pose_loss_fwd(const float* logits, const float* coefs, const float* target_depth,
                     const float* target_mask, const float* weights, float* sums, float* losses,
                     float* gsums, void* scratch, size_t scratch_bytes,
                     int N, int h, int w, int H, int W, void* stream);
int lf_pose_loss_bwd(const float* logits, const float* coefs, const float* target_depth,
                     const float* target_mask, const float* gsums, float* glogits, float* gcoefs,
                     void* scratch, size_t scratch_bytes, int N, int h, int w, int H, int W, void* stream);
/* The loss as the cross-entropy and Metropolis estimators evaluate it (PoseEstimator._render_observation,
 * pose/estimation.py:207-216): the de-normalised crop depth is multiplied by the crop's own sigmoid mask before it is
 * uncropped, z_depth = denormalize(depth) * mask; everything else as lf_pose_loss_fwd.  Forward only (those estimators
 * rank hypotheses, they do not differentiate); same scratch size. */
int lf_pose_loss_fwd_masked(const float* logits, const float* coefs, const float* target_depth,
                            const float* target_mask, const float* weights, float* sums, float* losses,
                            void* scratch, size_t scratch_bytes, int N, int h, int w, int H, int W, void* stream);
/* The loss as the MODULE path evaluates it (default_pose_loss handed the predicted metric depth crop and the mask-logit
 * crop, pose/estimation.py:70-118 called from :703-713 with the caller's own de-normalisation): channel 0 of
 * depth_and_logits [N][h*w][2] is the depth itself (no tanh / apply_mask / denormalize_depth inside), channel 1 the mask
 * logit; coefs entries 18..21 (the uncrop map) are used.  lf_pose_loss_bwd_depth writes d/d(depth crop, logit crop) and
 * gcoefs entries 18..21 (22, 23 = 0).  Same sums / losses / gsums / scratch as lf_pose_loss_fwd / _bwd. */
int lf_pose_loss_fwd_depth(const float* depth_and_logits, const float* coefs, const float* target_depth,
                           const float* target_mask, const float* weights, float* sums, float* losses,
                           float* gsums, void* scratch, size_t scratch_bytes,
                           int N, int h, int w, int H, int W, void* stream);
int lf_pose_loss_bwd_depth(const float* depth_and_logits, const float* coefs, const float* target_depth,
                           const float* target_mask, const float* gsums, float* gcrop, float* gcoefs,
                           void* scratch, size_t scratch_bytes, int N, int h, int w, int H, int W, void* stream);
/* Several target frames in one launch: N = T * n samples grouped by target, sample i scored against frame i / n of
 * target_depth / target_mask [T][H*W]; gsums is d(mean over the n samples OF THE SAME TARGET)/d(sums).  Otherwise as
 * lf_pose_loss_fwd / _fwd_masked / _bwd, and per target the outputs (sums, losses, gsums, glogits, gcoefs 18..23) are
 * bit-identical to the single-target entry point called on that target's n rows alone: those are this launch plan with
 * T = 1, n = N.  Scratch: lf_pose_loss_scratch_bytes(N, h, w, H, W).  Beyond the check above, T < 1, n < 1 or
 * N != T * n -> LF_EINVAL. */
int lf_pose_loss_fwd_mt(const float* logits, const float* coefs, const float* target_depth,
                        const float* target_mask, const float* weights, float* sums, float* losses,
                        float* gsums, void* scratch, size_t scratch_bytes,
                        int N, int T, int n, int h, int w, int H, int W, void* stream);
int lf_pose_loss_fwd_masked_mt(const float* logits, const float* coefs, const float* target_depth,
                               const float* target_mask, const float* weights, float* sums, float* losses,
                               void* scratch, size_t scratch_bytes, int N, int T, int n, int h, int w, int H, int W,
                               void* stream);
int lf_pose_loss_bwd_mt(const float* logits, const float* coefs, const float* target_depth,
                        const float* target_mask, const float* gsums, float* glogits, float* gcoefs,
                        void* scratch, size_t scratch_bytes, int N, int T, int n, int h, int w, int H, int W,
                        void* stream);

/* Batched Adam / AdamW step over N independent rows of P parameters (pose/estimation.py:579-594,
 * 664-666).  step_size[n] = lr[n] / (1 - beta1^t) and bias_correction2_sqrt = sqrt(1 - beta2^t)
 * are formed on the host in double like torch.optim does. */
int lf_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                 const float* step_size, const float* lr, float bias_correction2_sqrt,
                 float beta1, float beta2, float eps, float weight_decay, int N, int P, void* stream);

/* ------------------------------------------------------------------------------------------
 * Layout helpers (the reference is NCDHW; kernels are channels-last). */
int lf_nchw_to_nhwc(const float* src, float* dst, int N, int C, long P, void* stream);
int lf_nhwc_to_nchw(const float* src, float* dst, int N, int C, long P, void* stream);
/* FactorProjection2d3d.view (geometry.py:728): src [N][P][C0*S] with channel = c*S + d
 * -> dst [N][S][P][C0], optionally scaling row (n,p) by 1/norm[n*P+p] (deferred PixelNorm). */
int lf_lift_unfold(const float* src, const float* norm_or_null, float* dst,
                   int N, long P, int C0, int S, void* stream);
/* The same permutation for the training step, either way (autograd of the .view above and of
 * FactorProjection3d2d's reshape, geometry.py:745): fold = 0: src [N][P][C0*S] -> dst [N][S][P][C0];
 * fold = 1: src [N][S][P][C0] -> dst [N][P][C0*S].  4 * C0 * (S + 1) * 4 bytes of LDS must fit 64 KB (LF_EINVAL). */
int lf_lift_permute(const float* src, float* dst, int N, long P, int C0, int S, int fold, void* stream);
/* FactorProjection2d3d of the TRAINING step in two passes instead of four (modules/geometry.py:711-728 and its autograd):
 * lf_lift_norm_unfold: src [N][P][C0*S] = LeakyReLU(conv * he + b) rows (channel = c*S + d) -> PixelNorm over the C0*S channels
 *   of every pixel, written as the (N,C0,S,H,W) channels-last volume dst [N][S][P][C0] (fp32, or bf16 with out_bf16) and
 *   norm_out [N*P] = sqrt(mean + eps);
 * lf_lift_bwd: gradient volume + saved volume (io bit 0 / bit 1: stored as bf16) + norm -> gp [N][P][C0*S], the gradient
 *   w.r.t. the convolution's pre-activation (PixelNorm' then LeakyReLU'), as rows for the weight / data gradient products;
 *   round_bf16: written as bf16 values in the fp32 container (the autocast policy's operand rounding).
 * C0 % 4 == 0, S % 4 == 0, 2 * 4 * C0 * (S + 1) floats of LDS (<= 150 KB). */
int lf_lift_norm_unfold(const float* src, void* dst, float* norm_out, int N, long P, int C0, int S, float eps, int out_bf16,
                        void* stream);
int lf_lift_bwd(const void* gvol, const void* yvol, const float* norm, float* gp, int N, long P, int C0, int S, float slope,
                int round_bf16, int io, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LF_HIP_H */
