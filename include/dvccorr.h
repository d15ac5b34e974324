/*
 * dvccorr.h -- C ABI of the MI355X (gfx950) correlation hot path for RAFT-DVC.
 *
 * This is the drop-in boundary: plain pointers, sizes and an opaque stream,
 * no torch types.  Every entry point is stream-ordered on the caller's HIP
 * stream, never allocates device memory, never synchronises, and returns a
 * dvc_status (0 = OK); dvc_last_error() returns a thread-local message.
 * All device buffers are allocated by the caller (PyTorch in the Python host
 * layer, raft-dvc_amd/dvccorr).
 *
 * Reference interface each entry point replaces (zachtong/RAFT-DVC):
 *   dvc_layout_init        -- pyramid geometry of CorrBlock.__init__          src/core/corr.py:125-139
 *   dvc_pack_queries       -- fmap1.reshape(B,C,N).transpose(1,2)             src/core/corr.py:155-161
 *   dvc_pack_targets       -- fmap2 (+ its avg_pool3d pyramid, as in the
 *                             on-the-fly block)                               src/core/corr.py:158-161,
 *                                                                             src/core/corr_otf.py:83-86
 *   dvc_corr_build         -- torch.matmul(...) / sqrt(C) [+ pyramid levels]  src/core/corr.py:141-167
 *   dvc_corr_pool          -- F.avg_pool3d(corr, 2, stride=2)                 src/core/corr.py:136-139
 *   dvc_corr_lookup        -- CorrBlock.__call__                              src/core/corr.py:169-208
 *   dvc_corr_lookup_fused  -- CorrBlockOnTheFly.__call__ (any convention)     src/core/corr_otf.py:96-138,
 *                             / the CUDA OTF forward_one_level* launchers     src/core/cuda/corr_otf_cuda.cu:448-488
 *   dvc_corr_backward      -- autograd backward of CorrBlock (matmul,        src/core/corr.py:141-208;
 *                             avg_pool3d, grid_sample) / the CUDA OTF         src/core/cuda/corr_otf_cuda.cu:247-441,
 *                             backward launcher                               :491-530
 *   dvc_sample3d           -- bilinear_sampler_3d                             src/core/corr.py:17-68
 *   dvc_proj_pack,         -- CorrBlock.__call__ followed by the motion       src/core/corr.py:169-208 +
 *   dvc_corr_lookup_proj      encoder's F.relu(self.convc1(corr))            src/core/update.py:219-222, 246
 *   dvc_corr_lookup_fused_proj -- CorrBlockOnTheFly.__call__ + the same       src/core/corr_otf.py:96-237 +
 *                             convc1                                         src/core/update.py:219-222, 246
 *   dvc_coords_grid        -- coords_grid_3d                                 src/core/corr.py:71-99
 *   dvc_upflow             -- upflow_3d(flow, target_shape)                  src/core/corr.py:211-253
 *   dvc_flow_step          -- coords1 + delta_flow; upflow_3d(coords1 - coords0)  src/core/raft_dvc.py:482-485
 *
 * Layouts (row-major, element counts):
 *   fmap           (B, C, H, W, D) float32, channels-first, contiguous   (reference layout)
 *   coords         (B, 3, Nq) float32, channel order (h, w, d)           (corr.py:169-173)
 *   lookup out     (B, L*(2r+1)^3, Nq) float32; channel l*n^3+a*n^2+b*n+e (corr.py:188-208)
 *   packed queries [B][Nq][c_pad]         dtype (f32, bf16 or f16), zero channel padding; c_pad = 32, 64
 *                                         or 128 for C up to 128, else C rounded up to a multiple of 128
 *   packed targets [B][row_stride][c_pad] dtype; rows = level-concatenated target voxels
 *   corr pyramid   [B][Nq][row_stride]    store dtype; row q holds every level of query q:
 *                  level l voxel (y,x,z) at offset[l] + (y*W_l + x)*Dp_l + z, Dp_l = ceil8(D_l),
 *                  padding columns are 0; DVC_CORR_GUARD_BYTES of zeros before and after.
 *                  With DVC_BRICKED (below) the bricked levels hold the same values in
 *                  (1, 8, 8) bricks: offset[l] + ((y*W_l/8 + x/8)*Dp_l/8 + z/8)*64 + (x%8)*8 + z%8.
 * Nq is the number of query voxels per batch element; Nq == H*W*D for the
 * reference CorrBlock, Nq < H*W*D for one rank's query slab (sharded path).
 */
#ifndef DVCCORR_H
#define DVCCORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DVC_MAX_LEVELS 8
/* 2 (round 4): c_pad rounds to 32 / 64 / 128 then multiples of 128 (was ceil32), DVC_F16, and
 * dvc_corr_backward_mfma */
/* 3 (round 6): dvc_corr_lookup_proj on a DVC_F32 pyramid reads dvc_proj_pack_exact's hi + lo weight blocks
 * (2 x dvc_proj_packed_bytes; under version 2 an fp32 pyramid took dvc_proj_pack's single fp16 block) */
#define DVC_ABI_VERSION 3
/* The corr pyramid buffer must be allocated with DVC_CORR_GUARD_BYTES of extra
 * space before its first row and after its last row.  dvc_corr_build zeroes
 * them; dvc_corr_lookup's walk kernels load each window run from a clamped
 * address without branching and cancel out-of-range elements with zero
 * weights, so they may touch up to 2r+2 elements outside a row. */
#define DVC_CORR_GUARD_BYTES 256

typedef enum {
    DVC_OK = 0,
    DVC_ERR_INVALID = 1,      /* bad argument (shape, pointer, range) -- maps to ValueError/RuntimeError */
    DVC_ERR_UNSUPPORTED = 2,  /* valid but not implemented on this build */
    DVC_ERR_LAUNCH = 3,       /* hipGetLastError after a launch */
    DVC_ERR_RUNTIME = 4       /* other HIP runtime failure */
} dvc_status;

/* DVC_F16: the reference's AMP pyramid (torch.amp.autocast('cuda') in its Trainer, trainer.py:249-252,
 * makes CorrBlock's matmul and pyramid float16, corr.py:155-167): pack, build (v_mfma_f32_32x32x16_f16),
 * pool, lookup (also convc1-fused) and backward; the on-the-fly entry points (dvc_corr_lookup_fused,
 * dvc_corr_lookup_fused_proj) take it too (round 4): the reference's CorrBlockOnTheFly einsum runs in fp16 under
 * the same autocast (corr_otf.py:198-237), and the window dots are rounded to fp16 like the fp16 pyramid.
 * DVC_F32 on dvc_corr_lookup_fused_proj (round 7): the reference's fp32 evaluation of CorrBlockOnTheFly
 * (raft_dvc.py:403-412) with convc1 fused -- fp32 window dots on the matrix cores, the exact split consumer. */
typedef enum { DVC_F32 = 0, DVC_BF16 = 1, DVC_F16 = 2 } dvc_dtype;

/* Layout flag ORed into the dtype of dvc_pack_targets and the store_dtype of dvc_corr_lookup /
 * dvc_corr_lookup_proj (dvc_corr_build is layout-blind: it writes the columns in packed-target
 * order, so bricked targets give a bricked pyramid).  The levels dvc_bricked_levels() names
 * (Dp_l >= 32 and W_l % 8 == 0: a z-row of at least 64 bytes) are stored in (1, 8, 8) bricks of
 * one 128-byte line (bf16), so a lookup window's plane strip touches lines of 8 columns x 8 z
 * instead of 2 columns x 32 z -- fewer HBM lines per query (the lookup is bound by its bytes).
 * Only the tile lookup kernels read it: radius 1..6, no legacy W != D bricked level, and
 * num_levels <= 4 for the pack; other uses return DVC_ERR_UNSUPPORTED (dvc_corr_pool, the
 * on-the-fly and backward paths and dvc_corr_build take the plain dtype).
 * A bricked buffer carries no tag of its own: the CALLER keeps track of it and passes it, with the
 * DVC_BRICKED flag, only to dvc_corr_lookup / dvc_corr_lookup_proj.  Passed with the plain dtype to
 * any entry point (dvc_corr_lookup_fused, dvc_corr_backward, dvc_corr_pool, a walk lookup) it would
 * be read as the linear layout -- wrong values, no error.  (dvccorr's Python layer records the flag
 * next to every packed buffer and checks it, dvccorr/ops.py.) */
#define DVC_BRICKED 0x100

/* corr_sampler_version 2 = fixed, 1 = legacy W<->D swap (raft_dvc.py:71-77, corr.py:49-52). */
typedef enum { DVC_FIXED = 0, DVC_LEGACY = 1 } dvc_convention;

typedef struct {
    int32_t num_levels;
    int32_t channels;                 /* C */
    int32_t c_pad;                    /* packed-row length: 32, 64, 128, then multiples of 128 */
    int32_t H[DVC_MAX_LEVELS];
    int32_t W[DVC_MAX_LEVELS];
    int32_t D[DVC_MAX_LEVELS];
    int32_t Dp[DVC_MAX_LEVELS];       /* D rounded up to 8 */
    int32_t zero_level[DVC_MAX_LEVELS]; /* a size-1 axis: the reference samples all zeros (corr.py:41-44) */
    int64_t offset[DVC_MAX_LEVELS];   /* element offset of level l inside a row */
    int64_t level_elems[DVC_MAX_LEVELS];
    int64_t row_elems;                /* sum of padded level sizes */
    int64_t row_stride;               /* row_elems rounded up to 128 */
} dvc_layout;

/* Pure host function (no GPU).  Fails (DVC_ERR_INVALID) exactly where the
 * reference constructor raises: pooling an axis of size < 2. */
int dvc_layout_init(int H, int W, int D, int num_levels, int C, dvc_layout *out);

/* Bit mask of the levels DVC_BRICKED stores in bricks (pure host function). */
int dvc_bricked_levels(const dvc_layout *lay);

/* How many trailing levels the dvc_corr_lookup call with these arguments stages whole in LDS (the tile kernel's
 * coarse path, tuning "lookup_coarse") under the current tuning; 0 = none, -1 = bad arguments.  Pure host function,
 * the rule the launch itself applies: for tests and tools. */
int dvc_lookup_coarse_levels(int B, int64_t Nq, int H, int W, int D, int num_levels, int radius, int convention,
                             int store_dtype);

/* Bytes of float32 workspace dvc_pack_targets needs (pooled fmap2 levels 1..L-1; 0 for
 * num_levels <= 4, whose levels are pooled in LDS by one single-pass kernel). */
size_t dvc_pack_workspace_bytes(int B, int C, int H, int W, int D, int num_levels);

/* fmap1 query slab (B, C, Nq) float32 -> packed queries [B][Nq][c_pad] (dtype). */
int dvc_pack_queries(const float *fmap1, void *packed, int B, int C, int64_t Nq, int dtype, void *stream);

/* fmap2 (B, C, H, W, D) float32 -> packed targets [B][row_stride][c_pad] (dtype),
 * level l = l-fold 2x2x2 mean of fmap2 (floor), computed in float32. */
int dvc_pack_targets(const float *fmap2, void *packed, float *workspace, int B, int C, int H, int W, int D,
                     int num_levels, int dtype, void *stream);

/* dvc_pack_targets straight from an H-slab all-gather's receive buffer (the multi-GPU path,
 * dvccorr/sharded.py): gathered = world slabs of (B, C, maxh, W, D) float32, maxh = ceil(H / world),
 * slab r holding fmap2's planes [h0(r), h0(r + 1)) of the balanced split (h0(r) = r (H / world) +
 * min(r, H % world)) in its first planes.  Same packed output, bit for bit, as dvc_pack_targets of the
 * assembled fmap2, without assembling it (a copy of fmap2 per forward).  1 <= world <= H; the
 * single-pass pack only (num_levels <= 4, DVC_ERR_UNSUPPORTED otherwise); no workspace. */
int dvc_pack_targets_gathered(const float *gathered, int world, void *packed, int B, int C, int H, int W, int D,
                              int num_levels, int dtype, void *stream);

/* corr[b][q][col] = (sum_c q[b][q][c] * t[b][col][c]) * (1/sqrt(C)) for col in
 * [col_begin, col_end), stored as store_dtype.  in_dtype selects the MFMA path:
 * DVC_BF16 -> v_mfma_f32_32x32x16_bf16, DVC_F32 -> v_mfma_f32_32x32x2_f32.
 * col range [0, row_stride) builds every level from the pooled targets (by
 * linearity equal to pooling the correlation); [0, level_elems[0]) builds
 * level 0 only, for dvc_corr_pool to finish (the reference's op order). */
int dvc_corr_build(const void *packed_q, const void *packed_t, void *corr, int B, int64_t Nq, int C, int H, int W,
                   int D, int num_levels, int in_dtype, int store_dtype, int64_t col_begin, int64_t col_end,
                   void *stream);

/* Level src_level+1 of every row from level src_level: 2x2x2 mean, floor (avg_pool3d). */
int dvc_corr_pool(void *corr, int B, int64_t Nq, int H, int W, int D, int num_levels, int src_level,
                  int store_dtype, void *stream);

/* Radius-r trilinear lookup of every level (CorrBlock.__call__). */
int dvc_corr_lookup(const void *corr, const float *coords, float *out, int B, int64_t Nq, int H, int W, int D,
                    int num_levels, int radius, int convention, int store_dtype, void *stream);

/* Fused on-the-fly lookup: no correlation volume.  Dots of each query's
 * packed feature row with the packed target rows of its (2r+2)^3 integer
 * window, scattered by the trilinear weights.  workspace: see
 * dvc_lookup_fused_workspace_bytes. */
size_t dvc_lookup_fused_workspace_bytes(int B, int64_t Nq, int num_levels, int radius);
int dvc_corr_lookup_fused(const void *packed_q, const void *packed_t, const float *coords, float *out,
                          void *workspace, int B, int64_t Nq, int C, int H, int W, int D, int num_levels,
                          int radius, int convention, int dtype, void *stream);

/* Backward of dvc_corr_lookup / dvc_corr_lookup_fused w.r.t. both feature maps
 * (autograd through corr.py:141-208; coords get no gradient, raft_dvc.py:441):
 *   grad_out   (B, L*(2r+1)^3, Nq) float32   gradient of the lookup output
 *   grad_fmap1 (B, C, Nq) float32            overwritten
 *   grad_fmap2 (B, C, H, W, D) float32       overwritten (these Nq queries' contribution)
 * packed_q / packed_t are the forward's packed operands (dtype).  No atomics: every
 * sum runs in a fixed order, so results are bitwise reproducible.  Supported:
 * radius 1..6, any C (the gradient sums run per 128-channel group), Nq a multiple of W*D
 * (DVC_ERR_UNSUPPORTED otherwise);
 * both conventions on every level shape (legacy levels with W != D use a stretched
 * window box).  The workspace size covers either convention.  The call may fork part of its
 * work onto a library-owned high-priority stream (fork / join events, joined before it returns
 * to the caller's stream) except while the caller's stream is being captured into a HIP graph:
 * then every launch stays on that stream and the captured graph replays bitwise equal to the
 * eager call (its workspace clears are kernels, not memset nodes). */
size_t dvc_corr_backward_workspace_bytes(int B, int64_t Nq, int C, int H, int W, int D, int num_levels, int radius);
/* The workspace of dvc_corr_backward for one packed dtype: bf16 / fp16 operands need no lo tiles, so
 * their workspace is smaller than the dtype-less query's (~88 MB less at config #3); 0 for a bad dtype.  Either
 * query's size is enough for a call with that dtype. */
size_t dvc_corr_backward_workspace_bytes_dtype(int B, int64_t Nq, int C, int H, int W, int D, int num_levels,
                                               int radius, int dtype);
int dvc_corr_backward(const void *packed_q, const void *packed_t, const float *coords, const float *grad_out,
                      float *grad_fmap1, float *grad_fmap2, void *workspace, int B, int64_t Nq, int C, int H, int W,
                      int D, int num_levels, int radius, int convention, int dtype, void *stream);
/* Pure host function: 1 when dvc_corr_backward runs this shape's gradient sums on the matrix cores
 * (bf16 operands on v_mfma_f32_32x32x16_bf16, fp16 on _f16, fp32 operands split into bf16 hi/lo
 * tiles and multiplied twice, ~2^-16 relative per operand; the window gradients enter as one
 * 16-bit value each for bf16 / fp16 and as bf16 hi/lo pairs for fp32), 0 when it takes the VALU kernels (a volume whose MFMA-kernel buffer offsets would exceed
 * 31 bits: level-0 fmaps of about 154^3 and up).  The answer also follows the CALLING THREAD's
 * dvc_set_tuning("bwd_mfma", v) knob (0: VALU kernels for every dtype).  Same results either way
 * within the dtype's tolerance. */
int dvc_corr_backward_mfma(int B, int64_t Nq, int C, int H, int W, int D, int num_levels, int radius, int convention,
                           int dtype);
/* Pure host function: 1 when the window-gradient pass of dvc_corr_backward reads grad_out through
 * 64-bit addresses because one output row of (2r+1)^2 channels spans more than 2^31 - 1 bytes
 * ((2r+1)^2 * 4 * Nq; Nq > ~6.6 M at r = 4), 0 when it uses 32-bit buffer offsets.  Same values. */
int dvc_corr_backward_gout64(int64_t Nq, int radius);

/* Lookup with the motion encoder's convc1 (1x1x1 Conv3d L*(2r+1)^3 -> 96, + ReLU,
 * update.py:222, 246) fused into its epilogue: the L*(2r+1)^3-channel lookup output
 * never reaches HBM.
 *   dvc_proj_pack: convc1.weight viewed (96, L*(2r+1)^3) float32 -> packed fp16
 *     weights (dvc_proj_packed_bytes) in the kernel's MFMA operand order for one
 *     (num_levels, radius, convention); pack once per weight update.
 *   dvc_proj_pack_exact: the same weights as bf16 hi + lo blocks (2 x dvc_proj_packed_bytes:
 *     hi = bf16(w), then lo = bf16(w - hi)) for DVC_F32 pyramids.
 *   dvc_corr_lookup_proj: out (B, 96, Nq) float32 = relu(W . lookup(coords) + bias),
 *     bias (96) float32.  bf16 / f16 pyramids (dvc_proj_pack weights): the lookup values and
 *     the weights enter fp16 MFMA with float32 accumulation (tolerance 1e-2 max-normalised
 *     against the float32 reference).  DVC_F32 pyramids (dvc_proj_pack_exact weights, round 5):
 *     both operands split into bf16 hi + lo, three MFMAs per step (x_hi w_hi + x_lo w_hi +
 *     x_hi w_lo, float32 accumulation): the fp32 tolerance 1e-5 (the reference's fp32
 *     evaluation, evaluate_phase1.py:115-131).  A DVC_F32 call reads 2 x dvc_proj_packed_bytes
 *     of packed_w: passing dvc_proj_pack's single block there reads past it (ABI 3; the
 *     Python wrapper refuses a short buffer).  Supported: radius 1..4, tile-kernel row widths,
 *     and for the legacy convention W == D at every non-zero level (DVC_ERR_UNSUPPORTED otherwise). */
#define DVC_PROJ_COUT 96
#define DVC_PROJ_MAX_RADIUS 4
size_t dvc_proj_packed_bytes(int num_levels, int radius);
int dvc_proj_pack(const float *weight, void *packed, int cout, int num_levels, int radius, int convention,
                  void *stream);
int dvc_proj_pack_exact(const float *weight, void *packed, int cout, int num_levels, int radius, int convention,
                        void *stream);
int dvc_corr_lookup_proj(const void *corr, const float *coords, const void *packed_w, const float *bias, float *out,
                         int B, int64_t Nq, int H, int W, int D, int num_levels, int radius, int convention,
                         int store_dtype, void *stream);

/* The same composition on the on-the-fly path (CorrBlockOnTheFly.__call__ followed by
 * F.relu(self.convc1(corr)), src/core/corr_otf.py:96-237 + src/core/update.py:246):
 * packed_q / packed_t as for dvc_corr_lookup_fused (bf16, f16 or f32), packed_w from dvc_proj_pack
 * (for DVC_F32 from dvc_proj_pack_exact, 2 x dvc_proj_packed_bytes: the bf16 hi block then the lo block, as for
 * dvc_corr_lookup_proj on an fp32 pyramid), out (B, 96, Nq) float32.  Queries are processed in order of their level-0 window
 * origin (a radix sort per call), so each workgroup's union of windows is small; the
 * per-query 96-channel rows are transposed to (B, 96, Nq) at the end.  Workspace:
 * dvc_lookup_fused_proj_workspace_bytes (sort keys + the [B][Nq][96] rows).
 * DVC_F32 (k_fused_proj_f32): the window dots are those of dvc_corr_lookup_fused in fp32 (operands split into
 * three bf16 pieces, fp32 values), convc1 runs on bf16 hi/lo splits of both operands; fp32 tolerance 1e-5.
 * Supported: bf16 / f16 / f32, radius 1..4, C_pad in {32, 64, 128}, and for the legacy convention
 * W == D at every non-zero level (DVC_ERR_UNSUPPORTED otherwise). */
size_t dvc_lookup_fused_proj_workspace_bytes(int B, int64_t Nq);
int dvc_corr_lookup_fused_proj(const void *packed_q, const void *packed_t, const float *coords, const void *packed_w,
                               const float *bias, float *out, void *workspace, int B, int64_t Nq, int C, int H, int W,
                               int D, int num_levels, int radius, int convention, int dtype, void *stream);

/* bilinear_sampler_3d: vol (B, C, Hv, Wv, Dv), pts (B, Nq, 3) in (h, w, d) -> out (B, C, Nq). */
int dvc_sample3d(const float *vol, const float *pts, float *out, int B, int C, int Hv, int Wv, int Dv, int64_t Nq,
                 int convention, void *stream);

/* Per-iteration flow bookkeeping of RAFTDVC.forward, float32:
 *   dvc_coords_grid  coords (B, 3, H, W, D) = identity grid          src/core/corr.py:71-99
 *   dvc_upflow       flow_up (B, C, H, W, D) = upflow_3d(flow (B, C, h, w, d),
 *                    target_shape=(H, W, D)); C >= 3, channels 0..2 scaled by H/h, W/w, D/d
 *                                                                     src/core/corr.py:211-253
 *   dvc_flow_step    coords1_out = coords1 + delta_flow (delta_flow nullable: + 0) and
 *                    flow_up = upflow_3d(coords1_out - coords0, (H, W, D)), coords0 the
 *                    identity grid, in one pass                      src/core/raft_dvc.py:482-485
 *                    (coords1_out nullable; outputs must not alias inputs). */
int dvc_coords_grid(float *coords, int B, int H, int W, int D, void *stream);
int dvc_upflow(const float *flow, float *flow_up, int B, int C, int h, int w, int d, int H, int W, int D,
               void *stream);
int dvc_flow_step(const float *coords1, const float *delta_flow, float *coords1_out, float *flow_up, int B, int h,
                  int w, int d, int H, int W, int D, void *stream);

/* SepConvGRU3D forward, one fused launch per axis pass (src/core/update.py:139-199; the update block's default
 * GRU, hidden 96 and input 147 at update.py:283-297).  Per axis a in (h, w, d), conv_*_a a 5-tap 1-D convolution
 * zero-padded by 2 along a:  z = sigmoid(conv_z(cat[h, x])), r = sigmoid(conv_r(cat[h, x])),
 * q = tanh(conv_q(cat[r h, x])), h_out = (1 - z) h + z q.  Tensors are (B, C, H, W, D) float32, contiguous.
 *   dvc_gru_packed_bytes  bytes of one axis's packed weights and biases (0 for an unsupported shape or dtype)
 *   dvc_gru_pack          packs one axis: wz, wr, wq the (hidden, hidden + input, 5) float32 weights of the
 *                         axis's three convolutions (their contiguous storage), bz, br, bq the (hidden) biases,
 *                         into the MFMA operand order [gate][tap][c_in] padded.  dtype DVC_BF16 / DVC_F16:
 *                         one 16-bit block; DVC_F32: bf16 hi and lo pieces (three products per step, fp32
 *                         tolerance 1e-5; the 16-bit dtypes 1e-2).  A packed buffer is used with the dtype
 *                         it was packed for.
 *   dvc_sep_gru_pass      one axis pass (axis 0 = h, 1 = w, 2 = d) with that axis's packed buffer; h_out must
 *                         not overlap h or x (a pass reads its neighbours).  No atomics, no allocation, no
 *                         host synchronisation: capturable in a graph.  Workgroups own DVC_GRU_SEG output
 *                         positions along the axis.
 * Errors, before any GPU call: a null pointer, B / H / W / D < 1, axis outside 0..2, a bad dtype or overlapping
 * buffers are DVC_ERR_INVALID; hidden != DVC_GRU_HIDDEN, input outside 1..DVC_GRU_MAX_INPUT or a volume of
 * 2^31 voxels or more are DVC_ERR_UNSUPPORTED. */
#define DVC_GRU_HIDDEN 96
#define DVC_GRU_MAX_INPUT 160
#define DVC_GRU_SEG 8
size_t dvc_gru_packed_bytes(int hidden, int input, int dtype);
int dvc_gru_pack(const float *wz, const float *wr, const float *wq, const float *bz, const float *br,
                 const float *bq, void *packed, int hidden, int input, int dtype, void *stream);
int dvc_sep_gru_pass(const float *h, const float *x, const void *packed, float *h_out, int B, int hidden, int input,
                     int H, int W, int D, int axis, int dtype, void *stream);

/* The update block's plain convolutions on the matrix cores (src/core/update.py:205-348: BasicMotionEncoder's
 * convf1 / convf2 / conv and the flow and uncertainty heads).  Tensors are (B, C, H, W, D) float32, contiguous.
 *   dvc_conv3   3 x 3 x 3, zero padding 1, stride 1, + bias, + ReLU when relu != 0.  The input is the channel
 *               concatenation of src0 (c0 channels) and src1 (c1 channels; src1 may be NULL, c1 is then ignored);
 *               the output is the channel slice [dst_offset, dst_offset + cout) of dst, a tensor with dst_channels
 *               channels.  dst must not overlap a source.  Workgroups own boxes of
 *               DVC_CONV3_TH x DVC_CONV3_TW x DVC_CONV3_TD output voxels.
 *   dvc_conv3_pack / dvc_conv3_packed_bytes   w the (cout, cin, 3, 3, 3) float32 weight, bias (cout), into 1 KB MFMA
 *               A-operand fragments [32-channel chunk][tap][16-channel tile] (x 2 pieces, bf16 hi and lo, for
 *               DVC_F32), then 16 float32 biases per tile.  The tile count is cout / 16 rounded up to 1, 2, 4, 5 or
 *               8 (zero rows; padded outputs are never stored).
 *   dvc_conv7_flow (+ _pack, _packed_bytes)   encoder.convf1: 3 -> DVC_CONV7_COUT channels, 7 x 7 x 7, zero padding
 *               3, + bias + ReLU; w (64, 3, 7, 7, 7), fragments [kh][kw][tile] with k = 8 ci + kd.
 * dtype as the GRU: DVC_BF16 / DVC_F16 round the operands once (tolerance 1e-2), DVC_F32 uses bf16 hi + lo pieces
 * (1e-5); accumulation and output are float32.  No atomics, no allocation, no host synchronisation.
 * Errors, before any GPU call: a null pointer, B / H / W / D < 1, a bad dtype, c0 / c1 / cout < 1,
 * dst_offset < 0 or dst_offset + cout > dst_channels, or dst overlapping a source are DVC_ERR_INVALID; c0 + c1 >
 * DVC_CONV3_MAX_CIN, cout > DVC_CONV3_MAX_COUT or 2^31 voxels or more are DVC_ERR_UNSUPPORTED
 * (dvc_conv3_packed_bytes returns 0 for both). */
#define DVC_CONV3_TH 4
#define DVC_CONV3_TW 4
#define DVC_CONV3_TD 16
#define DVC_CONV3_MAX_CIN 128
#define DVC_CONV3_MAX_COUT 128
#define DVC_CONV7_TH 4
#define DVC_CONV7_TW 4
#define DVC_CONV7_TD 16
#define DVC_CONV7_COUT 64
size_t dvc_conv3_packed_bytes(int cin, int cout, int dtype);
int dvc_conv3_pack(const float *w, const float *bias, void *packed, int cin, int cout, int dtype, void *stream);
int dvc_conv3(const float *src0, int c0, const float *src1, int c1, const void *packed, float *dst, int dst_channels,
              int dst_offset, int cout, int relu, int B, int H, int W, int D, int dtype, void *stream);
size_t dvc_conv7_flow_packed_bytes(int dtype);
int dvc_conv7_flow_pack(const float *w, const float *bias, void *packed, int dtype, void *stream);
int dvc_conv7_flow(const float *flow, const void *packed, float *dst, int B, int H, int W, int D, int dtype,
                   void *stream);

/* The feature and context encoders' forward (csrc/encoder.hip; src/core/extractor.py:79-301, input_dim = 1, norms
 * 'instance' and 'none').  Tensors are (B, C, H, W, D) float32, contiguous.  A convolution stores its raw output
 * (+ bias) once; its InstanceNorm3d and ReLU are applied by the kernel that reads it, from a (B, C, 2) float32
 * scale_shift = (1 / sqrt(var + eps), -mean scale) table.  An output extent is (n - 1) / stride + 1.
 *   dvc_enc_stem   conv1: 1 -> DVC_ENC_STEM_COUT channels, 7 x 7 x 7, zero padding 3, stride 1 or 2, + bias; w
 *               (32, 1, 7, 7, 7).
 *   dvc_enc_conv   taps = 27 (3 x 3 x 3, zero padding 1) or 1 (1 x 1 x 1), stride 1 or 2, + bias.  prologue applied
 *               to the input on load: DVC_ENC_IDENTITY, DVC_ENC_RELU, or DVC_ENC_NORM_RELU = relu(x scale + shift)
 *               with scale_shift (B, cin, 2) (NULL: scale 1, shift 0); the zero padding belongs to the activated
 *               tensor.  split < 0: y (B, cout, ..) gets the raw output.  0 < split < cout (the context encoder's
 *               conv2): y (B, split, ..) gets tanh of channels [0, split), y2 (B, cout - split, ..) the ReLU of the
 *               rest.
 *   partials    where not NULL, the kernel writes dvc_enc_partials_bytes(taps, stride, cout, B, OH, OW, OD) bytes of
 *               per-workgroup double sums of its output and its square ((taps, stride) = (343, stride) for the stem);
 *               dvc_enc_stats reduces them in a fixed order (no atomics: bit-identical from run to run) into
 *               scale_shift (B, cout, 2), biased variance.
 *   dvc_enc_residual   out = relu(c3 scale3 + shift3 + r) over (B, C, H, W, D), r = shortcut (DVC_ENC_SC_PLAIN),
 *               shortcut scale4 + shift4 (DVC_ENC_SC_NORM) or relu(shortcut scale4 + shift4) (DVC_ENC_SC_NORM_RELU);
 *               a NULL table is scale 1, shift 0.  out must not overlap c3 or the shortcut.
 * dtype: DVC_BF16 / DVC_F16 round the operands once, as dvc_conv3; DVC_F32 splits every operand into three bf16
 * pieces (hi + mid + lo, the float32 value exactly) and takes six products per step, so only the float32
 * accumulation rounds -- two pieces per operand, as dvc_conv3 uses, compound to 1e-4 over an encoder's twenty
 * normalised layers.  The packed weights hold three pieces per fragment for DVC_F32.  No atomics, no allocation, no
 * host synchronisation.
 * Errors, before any GPU call: a null pointer, B / H / W / D < 1, a bad dtype, taps, stride, prologue, mode or
 * split, or an output overlapping an input are DVC_ERR_INVALID; cin outside 8..DVC_ENC_MAX_CIN or no multiple of 8,
 * cout outside 1..DVC_ENC_MAX_COUT, B * C > 65535 planes or 2^31 voxels or more are DVC_ERR_UNSUPPORTED (the size
 * functions return 0 for all of these). */
#define DVC_ENC_TH 4
#define DVC_ENC_TW 4
#define DVC_ENC_TD 16
#define DVC_ENC_STEM_COUT 32
#define DVC_ENC_MAX_CIN 128
#define DVC_ENC_MAX_COUT 160
#define DVC_ENC_IDENTITY 0
#define DVC_ENC_RELU 1
#define DVC_ENC_NORM_RELU 2
#define DVC_ENC_SC_PLAIN 0
#define DVC_ENC_SC_NORM 1
#define DVC_ENC_SC_NORM_RELU 2
size_t dvc_enc_stem_packed_bytes(int dtype);
int dvc_enc_stem_pack(const float *w, const float *bias, void *packed, int dtype, void *stream);
int dvc_enc_stem(const float *x, const void *packed, float *y, void *partials_or_null, int B, int H, int W, int D,
                 int stride, int dtype, void *stream);
size_t dvc_enc_conv_packed_bytes(int taps, int cin, int cout, int dtype);
int dvc_enc_conv_pack(const float *w, const float *bias, void *packed, int taps, int cin, int cout, int dtype,
                      void *stream);
int dvc_enc_conv(const float *x, const float *scale_shift_or_null, int prologue, const void *packed, float *y,
                 float *y2_or_null, int split, void *partials_or_null, int taps, int stride, int cin, int cout, int B,
                 int H, int W, int D, int dtype, void *stream);
size_t dvc_enc_partials_bytes(int taps, int stride, int cout, int B, int OH, int OW, int OD);
int dvc_enc_stats(const void *partials, float *scale_shift, int taps, int stride, int cout, int B, int OH, int OW,
                  int OD, float eps, void *stream);
int dvc_enc_residual(const float *c3, const float *scale_shift3_or_null, const float *shortcut,
                     const float *scale_shift4_or_null, int mode, float *out, int C, int B, int H, int W, int D,
                     void *stream);

/* The backward of the encoders' forward (csrc/encoder_grad.hip): what dvccorr.encoder_ad needs.  For a layer
 * y = conv(act(x)) + bias with cin -> cout channels, taps 27 or 1 (or 343: the stem, cin = 1, no prologue), stride 1 or
 * 2, input volume (H, W, D), output volume (OH, OW, OD), and g_x = dL/dy (B, cout, OH, OW, OD):
 *   dvc_enc_norm_grad   g_x from the gradient g with respect to the normalised value n = fma(x, scale, shift) of a raw
 *               output x (B, C, H, W, D): gn = g [n > 0] (mask = 1) or g (mask = 0), g_x = scale (gn - mean(gn) -
 *               n mean(gn n)), the means per (b, c) from per-workgroup double partials summed in index order.  With
 *               scale_shift NULL (no norm) g_x = gn, the mask being [x > 0].  db (C), where not NULL, gets the sums
 *               of g_x over (b, v), in a fixed order; gx may be NULL (db only).  partials: a work buffer of
 *               dvc_enc_grad_partials_bytes(C, B, H, W, D) = B C ceil(H W D / DVC_ENC_GRAD_CHUNK) 3 doubles.
 *   dvc_enc_grad_add    dst = (a + b) [m > 0] over n values; b and m may be NULL (dst may be a).
 *   dvc_enc_split_grad  the gradient of the context encoder's conv2 output from its two halves: g (B, cout, ..) =
 *               g_net (1 - net^2) on channels [0, split), g_ctx [ctx > 0] on the rest; a NULL gradient is zero.
 *   dvc_enc_conv_pack_dgrad   the weights of the input gradient, W'[ci][o][t'] = w[o][ci][taps - 1 - t'], in
 *               dvc_enc_conv_pack's layout (dvc_enc_dgrad_packed_bytes bytes); used with the dtype it was packed for.
 *   dvc_enc_dgrad       dx (B, cin, H, W, D) = the transposed convolution of g_x: dvc_enc_conv's kernel at stride 1
 *               on the packed dgrad weights; for stride 2 the source is read with zeros between its voxels.  cout
 *               (the kernel's K) is a multiple of 8 up to DVC_ENC_MAX_COUT here, cin up to DVC_ENC_MAX_COUT.
 *   dvc_enc_wgrad       dw[o][ci][t] = sum over (b, v) of g_x[b, o, v] act(x)[b, ci, v stride + delta(t)], the
 *               (cout, cin, taps) float32 weight gradient as a split-K GEMM over the output voxels on the matrix
 *               cores; the prologue as dvc_enc_conv (the zero padding belongs to the activated tensor).  A K step is
 *               32 output voxels; the nk = B ceil(OH OW OD / 32) steps are cut into slabs of per = ceil(nk /
 *               min(ceil(nk / 4), ceil(DVC_ENC_WGRAD_TARGET / groups))) steps, groups = ceil(ceil(taps cin / 16) /
 *               (taps == 1 ? 2 : 7)) * ceil(cout / 32); each slab writes its partial to the workspace
 *               (dvc_enc_wgrad_workspace_bytes = slabs * cout * cin * taps * 4) and the slabs are summed in index
 *               order (bit-identical from run to run).
 *   dvc_enc_stem_wgrad  the same for conv1: x (B, 1, H, W, D), dw (32, 1, 7, 7, 7).
 * dtype as the forward; for DVC_F16 the gradient operands are rounded to fp16 too (scale the loss as under AMP).
 * No atomics, no allocation, no host synchronisation.  Errors as dvc_enc_conv; channel counts outside the above are
 * DVC_ERR_UNSUPPORTED (the _bytes functions return 0). */
#define DVC_ENC_GRAD_CHUNK 4096
#define DVC_ENC_WGRAD_TARGET 1024
size_t dvc_enc_grad_partials_bytes(int C, int B, int H, int W, int D);
int dvc_enc_norm_grad(const float *g, const float *x, const float *scale_shift_or_null, int mask, float *gx_or_null,
                      float *db_or_null, void *partials, int C, int B, int H, int W, int D, void *stream);
int dvc_enc_grad_add(const float *a, const float *b_or_null, const float *m_or_null, float *dst, long long n,
                     void *stream);
int dvc_enc_split_grad(const float *g_net_or_null, const float *g_ctx_or_null, const float *net, const float *ctx,
                       float *g, int split, int cout, int B, int H, int W, int D, void *stream);
size_t dvc_enc_dgrad_packed_bytes(int taps, int cin, int cout, int dtype);
int dvc_enc_conv_pack_dgrad(const float *w, void *packed, int taps, int cin, int cout, int dtype, void *stream);
int dvc_enc_dgrad(const float *g, const void *packed, float *dx, int taps, int stride, int cin, int cout, int B, int H,
                  int W, int D, int dtype, void *stream);
size_t dvc_enc_wgrad_workspace_bytes(int taps, int stride, int cin, int cout, int B, int H, int W, int D);
int dvc_enc_wgrad(const float *x, const float *scale_shift_or_null, int prologue, const float *g, float *dw,
                  void *workspace, int taps, int stride, int cin, int cout, int B, int H, int W, int D, int dtype,
                  void *stream);
size_t dvc_enc_stem_wgrad_workspace_bytes(int stride, int B, int H, int W, int D);
int dvc_enc_stem_wgrad(const float *x, const float *g, float *dw, void *workspace, int stride, int B, int H, int W,
                       int D, int dtype, void *stream);

/* The backward of dvc_conv3 (csrc/conv3_grad.hip).  With y = conv(cat[src0, src1], w) + bias (+ ReLU) and
 * g = dL/dy (times [y > 0] under ReLU), all (B, C, H, W, D) float32, contiguous:
 *   dvc_conv3_grad_prep   g = grad_y [y > 0] and db[o] = sum over (b, v) of g[b, o, v].  With ReLU pass y (the
 *               layer's own output) and g; without, pass both NULL: g is grad_y itself and only db is written.
 *               partial is a work buffer of cout * B * ceil(H W D / DVC_CONV3_PREP_CHUNK) floats; the sums have a
 *               fixed order, so db is bit-identical from run to run.  g must not overlap grad_y or y.
 *   dvc_conv3_pack_dgrad  the weights of the input gradient: the fragments of the layer W'[ci][o][t'] =
 *               w[o][ci][26 - t'] (cin and cout swapped, all three axes flipped, zero biases) in dvc_conv3_pack's
 *               layout, dvc_conv3_packed_bytes(cout, cin, dtype) bytes, so that
 *               dvc_conv3(g, cout, NULL, 0, packed, dx, cin, 0, cin, 0, ...) is d loss / d cat[src0, src1].
 *   dvc_conv3_wgrad       dw[o][ci][t] = sum over (b, v) of g[b, o, v] cat[src0, src1][b, ci, v + delta(t)], the
 *               (cout, c0 + c1, 3, 3, 3) float32 weight gradient, as a GEMM over the voxels on the matrix cores.  A
 *               K-block is a box of DVC_CONV3_WGRAD_KH x KW x KD voxels; the nbox = B ceil(H / KH) ceil(W / KW)
 *               ceil(D / KD) blocks are cut into slabs of per = ceil(nbox / min(nbox, ceil(DVC_CONV3_WGRAD_TARGET /
 *               (ceil(cin / 16) * groups)))) consecutive blocks, groups = ceil(cout / 32) (1 for cout <= 16).  Each
 *               of the ceil(nbox / per) slabs writes its partial dw to the workspace and the slabs are summed in index
 *               order (no slab is empty; bit-identical from run to run).  dw and the workspace must not overlap an
 *               input.  dtype as dvc_conv3; for DVC_F16 the gradient operand g is rounded to fp16 too (scale the
 *               loss as under AMP).
 *   dvc_conv3_wgrad_workspace_bytes   slabs * cout * cin * 27 * 4 (0 for an unsupported shape).
 * No atomics, no allocation, no host synchronisation.  Errors as dvc_conv3: a null pointer, B / H / W / D < 1, a bad
 * dtype, channel counts < 1 or overlapping buffers are DVC_ERR_INVALID; cin or cout above 128 or 2^31 voxels or more
 * are DVC_ERR_UNSUPPORTED. */
#define DVC_CONV3_WGRAD_KH 4
#define DVC_CONV3_WGRAD_KW 4
#define DVC_CONV3_WGRAD_KD 16
#define DVC_CONV3_WGRAD_TARGET 512
#define DVC_CONV3_PREP_CHUNK 4096
int dvc_conv3_pack_dgrad(const float *w, void *packed, int cin, int cout, int dtype, void *stream);
int dvc_conv3_grad_prep(const float *grad_y, const float *y_or_null, float *g_or_null, float *db, float *partial,
                        int cout, int B, int H, int W, int D, void *stream);
size_t dvc_conv3_wgrad_workspace_bytes(int cin, int cout, int B, int H, int W, int D);
int dvc_conv3_wgrad(const float *src0, int c0, const float *src1, int c1, const float *g, int cout, float *dw,
                    void *workspace, int B, int H, int W, int D, int dtype, void *stream);

/* The weight gradient of dvc_conv7_flow (csrc/conv7_grad.hip): encoder.convf1 trains.  flow (B, 3, H, W, D) and g
 * (B, DVC_CONV7_COUT, H, W, D) float32, contiguous; g = dL/dy [y > 0] and the bias gradient come from
 * dvc_conv3_grad_prep with cout = DVC_CONV7_COUT.  The layer's input is the flow, which the model detaches at every
 * iteration (raft_dvc.py:441): there is no input gradient.
 *   dvc_conv7_wgrad       dw[o][ci][kh][kw][kd] = sum over (b, h, w, d) of g[b, o, h, w, d] flow[b, ci, h + kh - 3,
 *               w + kw - 3, d + kd - 3] (out-of-volume flow is zero), the (64, 3, 7, 7, 7) float32 weight gradient,
 *               as a GEMM over the voxels on the matrix cores.  The 3 * 343 = 1029 weights of an output channel are
 *               the GEMM's columns, in 65 tiles of 16; a workgroup owns DVC_CONV7_WGRAD_TILES of them, so there are
 *               groups = ceil(65 / TILES) workgroups per slab.  A K-block is a box of DVC_CONV7_WGRAD_KH x KW x KD
 *               voxels; the nbox = B ceil(H / KH) ceil(W / KW) ceil(D / KD) blocks are cut into slabs of per =
 *               ceil(nbox / min(nbox, ceil(DVC_CONV7_WGRAD_TARGET / groups))) consecutive blocks.  Each of the
 *               ceil(nbox / per) slabs writes its partial dw to the workspace and the slabs are summed in index order
 *               (no slab is empty; bit-identical from run to run).  dtype as dvc_conv7_flow; for DVC_F16 the
 *               gradient operand g is rounded to fp16 too (scale the loss as under AMP).
 *   dvc_conv7_wgrad_workspace_bytes   slabs * 64 * 1029 * 4 (0 for an empty or unsupported volume).
 * No atomics, no allocation, no host synchronisation.  Errors, before any GPU call: a null pointer, B / H / W / D < 1,
 * a bad dtype, or dw or the workspace overlapping an input or each other are DVC_ERR_INVALID; 2^31 voxels or more are
 * DVC_ERR_UNSUPPORTED. */
#define DVC_CONV7_WGRAD_KH 4
#define DVC_CONV7_WGRAD_KW 4
#define DVC_CONV7_WGRAD_KD 16
#define DVC_CONV7_WGRAD_TILES 5
#define DVC_CONV7_WGRAD_TARGET 256
size_t dvc_conv7_wgrad_workspace_bytes(int B, int H, int W, int D);
int dvc_conv7_wgrad(const float *flow, const float *g, float *dw, void *workspace, int B, int H, int W, int D,
                    int dtype, void *stream);

/* The backward of dvc_sep_gru_pass (csrc/gru_grad.hip).  All tensors (B, C, H, W, D) float32, contiguous; hidden is
 * DVC_GRU_HIDDEN, input 1..DVC_GRU_MAX_INPUT.  With G = dL/dh_out of one axis pass:
 *   dvc_sep_gru_pass_save   dvc_sep_gru_pass that also stores the pass's z, r and q (after tanh) into save, three
 *               (B, hidden, H, W, D) tensors in a row.  h_out is bit-identical to dvc_sep_gru_pass's.  A GRU call keeps
 *               z, r, q of its three passes and two intermediate hidden states: 11 * hidden * B H W D floats (138 MB at
 *               32^3).
 *   dvc_gru_pack_dgrad      the weights of the input gradient, W'[ci][o][t'] = w[o][ci][4 - t'] of (wq) and of (wz; wr),
 *               dvc_gru_dgrad_packed_bytes bytes; used with the dtype it was packed for.
 *   dvc_gru_grad_prep       a_q = G z (1 - q^2), a_z = G (q - h) z (1 - z), dh = G (1 - z), db_q and db_z (the sums of
 *               a_q and a_z over (b, v), in a fixed order).  partial is a work buffer of 2 * hidden * B *
 *               ceil(H W D / DVC_CONV3_PREP_CHUNK) floats.
 *   dvc_sep_gru_dgrad       with D = wq^T *T a_q and E = (wz; wr)^T *T (a_z; a_r), *T the transposed 5-tap convolution
 *               along the axis: writes a_r = D[:hidden] h r (1 - r), adds D[:hidden] r + E[:hidden] to dh (as left by
 *               dvc_gru_grad_prep: dh is then dL/dh of the pass) and D[hidden:] + E[hidden:] to dx (dx_add != 0) or
 *               stores it (dx_add == 0); dx may be NULL (no input gradient).  db_r is the sum of a_r; partial is
 *               hidden * B * ceil(H W D / DVC_CONV3_PREP_CHUNK) floats.
 *   dvc_gru_wgrad           dw[gate z, r, q][o][ci][t] = sum over (b, v) of a_gate[b, o, v] in_gate[b, ci, v + (t - 2) e],
 *               in_z = in_r = cat[h, x], in_q = cat[r h, x]: the three (hidden, hidden + input, 5) weight gradients in
 *               a row, as a GEMM over the voxels on the matrix cores.  A K-block is DVC_GRU_WGRAD_LINES lines x
 *               DVC_GRU_WGRAD_POS positions; the nkb = ceil(lines / LINES) * ceil(len / POS) blocks are cut into slabs
 *               of per = ceil(nkb / min(nkb, ceil(DVC_GRU_WGRAD_TARGET / (3 * ceil((hidden + input) / 16)))))
 *               consecutive blocks; each of the ceil(nkb / per) slabs writes its partial to the workspace
 *               (dvc_gru_wgrad_workspace_bytes = slabs * 3 * hidden * (hidden + input) * 5 * 4) and the slabs are summed
 *               in index order (no slab is empty; bit-identical from run to run).
 * dtype as the forward; for DVC_F16 the gradient operands are rounded to fp16 too (scale the loss as under AMP).
 * No atomics, no allocation, no host synchronisation.  Errors as dvc_conv3_wgrad: a null pointer (dx excepted),
 * B / H / W / D < 1, axis outside 0..2, a bad dtype or an output or workspace overlapping another buffer are
 * DVC_ERR_INVALID; hidden != DVC_GRU_HIDDEN, input outside 1..DVC_GRU_MAX_INPUT or 2^31 voxels or more are
 * DVC_ERR_UNSUPPORTED (the _bytes functions return 0). */
#define DVC_GRU_WGRAD_LINES 32
#define DVC_GRU_WGRAD_POS 4
#define DVC_GRU_WGRAD_TARGET 512
int dvc_sep_gru_pass_save(const float *h, const float *x, const void *packed, float *h_out, float *save, int B,
                          int hidden, int input, int H, int W, int D, int axis, int dtype, void *stream);
size_t dvc_gru_dgrad_packed_bytes(int hidden, int input, int dtype);
int dvc_gru_pack_dgrad(const float *wz, const float *wr, const float *wq, void *packed, int hidden, int input,
                       int dtype, void *stream);
int dvc_gru_grad_prep(const float *g, const float *z, const float *q, const float *h, float *a_q, float *a_z,
                      float *dh, float *db_q, float *db_z, float *partial, int B, int hidden, int H, int W, int D,
                      void *stream);
int dvc_sep_gru_dgrad(const float *a_q, const float *a_z, const float *h, const float *r, const void *packed,
                      float *a_r, float *dh, float *dx_or_null, float *db_r, float *partial, int B, int hidden,
                      int input, int H, int W, int D, int axis, int dx_add, int dtype, void *stream);
size_t dvc_gru_wgrad_workspace_bytes(int hidden, int input, int B, int H, int W, int D, int axis);
int dvc_gru_wgrad(const float *h, const float *x, const float *r, const float *a_z, const float *a_r,
                  const float *a_q, float *dw, void *workspace, int B, int hidden, int input, int H, int W, int D,
                  int axis, int dtype, void *stream);

/* Diagnostics hook for A/B timing.  The product kernel selection is a fixed table;
 * an override set here is PROCESS-GLOBAL (round 6; it was thread-local, which a
 * backward run on the autograd engine's worker thread never saw): it changes every
 * later launch of every host thread, on any stream, until set back.
 *   "lookup_variant" 2 = LDS-staged tile kernel (default), 0 = walk with unaligned
 *                    16-byte run loads, 1 = walk with aligned chunks + v_perm shifter;
 *   "lookup_coarse"  the tile kernel's coarse levels (small enough to stage whole in LDS): 1 = staged
 *                    whole, one unit per tile, dispatched first (default); 2 / 3 / 4 = the A/B
 *                    variants (one unit per level and / or dispatched last); 0 = every level on
 *                    the plane pipeline (bit-identical results for every value);
 *   "lookup_stretch" 1 = legacy W != D levels on k_lookup_stretch (LDS-staged stretched
 *                    boxes; the on-the-fly path on window-dot boxes), 0 = per-output
 *                    generic kernels (bit-identical results either way);
 *   "bwd_stretch"    1 = legacy W != D window gradients in LDS planes, 0 = global boxes
 *                    (bit-identical);
 *   "upflow_staged"  1 = k_upflow through an LDS-staged low-res box (default), 0 = direct;
 *   "fused_variant", "build_variant", "upflow_rows", "bwd_*", ... see capi.hip;
 *   "*_ablate"       diagnostics only, invalidates outputs. */
int dvc_set_tuning(const char *key, int value);

const char *dvc_last_error(void);
const char *dvc_version(void);
int dvc_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* DVCCORR_H */
