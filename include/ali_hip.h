/*
 * ali_hip.h -- C ABI of libali_hip.so: the MI355X (gfx950) kernels behind the
 * ALI/BiGAN training path of wtaylor17/ImageCFGen-Pytorch (image_scms package).
 *
 * The reference has no FFI of its own: all of its arithmetic is dispatched by
 * torch.nn modules.  Each entry point below names the reference call site
 * (file:line, relative to the reference checkout) whose ATen op it replaces.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all tensors fp32 in HBM.
 *   - activations are NHWC ([B,H,W,C], C contiguous); an op that reads an
 *     activation with float4 loads needs its channel stride % 4 == 0 (the
 *     callers pad 5->8 and 771->772 channels with zeros).
 *   - every function is stream ordered, never allocates, never synchronises,
 *     and returns 0 or a negative AliStatus; ali_last_error() gives the text.
 *   - `ws` is caller-provided scratch (>= the matching *_workspace_bytes());
 *     it may be reused by the next call on the same stream, not by concurrent
 *     streams.  Its first ALI_WS_RESERVED bytes are the split-K arrival
 *     counters of the GEMM kernels: zero-fill a new workspace once
 *     (hipMemset); every launch leaves them at zero again.
 */
#ifndef ALI_HIP_H
#define ALI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* ali_stream_t; /* hipStream_t */
#define ALI_WS_RESERVED 4096

typedef enum {
  ALI_OK = 0,
  ALI_ERR_BAD_ARG = -1,
  ALI_ERR_WORKSPACE = -2,
  ALI_ERR_LAUNCH = -3
} AliStatus;

typedef enum { ALI_ACT_NONE = 0, ALI_ACT_LEAKY = 1, ALI_ACT_TANH = 2 } AliAct;

/* Geometry of one Conv2d (cross-correlation) y = conv(x, W):
 *   x [B,H,W,C] (channel stride C, may include zero padding channels)
 *   y [B,P,Q,K] (channel stride K)
 *   W [K][C][R][S] logically; one stride and one padding for both axes.
 * Maps and kernels may be rectangular: H != W, P != Q and R != S are supported by ali_conv_fwd, ali_conv_bwd_data
 * and ali_conv_bwd_weight on every route (R, S <= 5; tests/test_gpu_conv_geometry.py), 1 x n and n x 1 maps included.
 * The special first-layer kernels behind them (8 -> 32 channels, stride 1; 4 / 8 -> 64 channels, stride 2) take 3x3 /
 * 5x5 kernels on rectangular maps; any other kernel shape runs on the general GEMM kernel.  ali_conv_fwd takes any
 * stride, ali_conv_bwd_data strides 1 and 2 (ALI_ERR_BAD_ARG otherwise, dx untouched).  Of the direct one-channel
 * entry points ali_tconv1_fwd needs a square kernel (R == S) and ali_tconv1_dgrad R*S in {1, 4, 9, 16, 25}.
 * A ConvTranspose2d (mnist.py:64-72, audio_mnist.py:216-242) is described by
 * the Conv2d it is the data-gradient of: x := its output, y := its input. */
typedef struct {
  int32_t B, H, W, C;
  int32_t P, Q, K;
  int32_t R, S, stride, pad;
} AliConvGeom;

/* Optional fused epilogue, applied in this order to v = acc:
 *   v += bias[n]; v = act(v); v *= mask[img*mask_ld + n]; v *= act'(dact_y)
 * dact_y has the layout of the output; act' is evaluated on the *activated*
 * value saved in forward (leaky: y>0 ? 1 : slope, tanh: 1-y*y).
 *
 * Fused BatchNorm2d reductions (mnist.py:111,114,118,122; bn_mode != 0): the launch also leaves, per M-tile of its
 * grid ("slot"; ali_conv_mtiles tells how many), the column sums over the tile's rows that nn.BatchNorm2d needs, so no
 * separate pass over the tensor is made:
 *   bn_mode 1 (the conv in front of a BatchNorm, forward): s0 = sum v~, s1 = sum v~^2 with v~ = v * bn_stat_mask[img,n]
 *             (a Dropout2d between the conv and the BatchNorm; NULL: v~ = v, the stored value);
 *   bn_mode 2 (the data-gradient GEMM behind a BatchNorm, backward): s0 = sum g~ * xhat, s1 = sum g~ with
 *             g~ = v * bn_mask_pre[img,n], xhat = (bn_x * bn_mask_in[img,n] - bn_mean[n]) * bn_invstd[n]; bn_x has the
 *             layout of the output.
 * bn_part[(s*N + n) * slots + slot(tile)], slots = number of M-tiles.  bn_groups > 1 (mode 1): the batch is that many
 * passes back to back (B/groups images each, B/groups a multiple of the tile height: ali_conv_mtiles reports it);
 * the slots of pass g are the contiguous range [g*slots/groups, (g+1)*slots/groups).  Consumed by
 * ali_bn_stats_from_partials / ali_bn_bwd_from_partials. */
typedef struct {
  const float* bias;   /* [N] or NULL */
  int32_t act;         /* AliAct */
  float slope;
  const float* mask;   /* per (image, channel) Dropout2d mask or NULL */
  int32_t mask_ld;
  const float* dact_y; /* or NULL */
  int32_t dact;        /* AliAct of the producer of dact_y */
  float dslope;
  float* bn_part;      /* or NULL */
  int32_t bn_mode, bn_groups;
  const float* bn_stat_mask;   /* mode 1, or NULL; row stride bn_mask_ld */
  int32_t bn_mask_ld;
  const float* bn_x;           /* mode 2 */
  const float* bn_mean;
  const float* bn_invstd;
  const float* bn_mask_in;     /* mode 2, or NULL; row stride bn_mask_ld */
  const float* bn_mask_pre;    /* mode 2, or NULL; row stride bn_mask_ld */
  /* Arithmetic of the contraction: 0 = fp32 operands on v_mfma_f32_32x32x2_f32 (exact fp32 fma chain); 1 = operands
   * rounded to fp16 on their way into LDS, v_mfma_f32_32x32x16_f16 with fp32 accumulation (BASELINE config 5,
   * esrf_acoustic.py:134-260) where the layer takes the uniform-tap path (input channel stride % 32 == 0, more
   * than 32 output channels); other layers keep fp32.  Tensors in HBM are fp32 either way. */
  int32_t mfma_f16;
  /* fp16 twins (mfma_f16 launches only; all optional): in16 / w16 = the gathered operand and the packed weights as
   * fp16 arrays of the same shapes -- when both are given and the input channel stride % 64 == 0 the kernel reads them
   * instead of x / w (half the bytes, no conversion); out16 = where to leave the fp16 twin of the output for the next
   * layer.  A launch that cannot run on fp16 MFMA (ali_conv_uses_f16 = 0) ignores in16 / w16 and keeps fp32
   * arithmetic, but still leaves out16, so that the layer behind it reads fp16 operands (ali_conv_writes_out16). */
  const void* in16;
  const void* w16;
  void* out16;
  /* Dispatch order of the launch's M-tiles (device int32[tile_order_n], from ali_conv_tile_order; NULL = natural
   * order).  Ignored unless tile_order_n equals the launch's M-tile count and every block owns a whole k-loop. */
  const int32_t* tile_order;
  int32_t tile_order_n;
  /* Operands that are column ranges of wider row-major buffers (the Discriminator's joint [dx | dz] rows,
   * mnist.py:152-154): in_ld = floats between consecutive pixels of the gathered operand (its fp16 twin alike),
   * out_ld = the same for the output (and dact_y, out16).  0 = dense.  Not with the fused BatchNorm modes. */
  int32_t in_ld;
  int32_t out_ld;
  /* Forward convs: the number of leading input channels that carry data when the channel stride is padded (a first
   * layer's 5 planes in an 8-channel NHWC tensor, mnist.py:108); the others must be zero in x or in w_kxc.  A hint:
   * 0 = unknown; kernels that can skip the padding do. */
  int32_t in_ch_live;
  /* Capacity check of bn_part: the number of slots the caller sized it for (what ali_conv_mtiles told it); a launch
   * whose M-tile count differs (tuning reloaded in between, other precision) fails with ALI_ERR_BAD_ARG instead of
   * writing out of bounds.  0 = unchecked. */
  int32_t bn_slots;
  /* mfma_f16 launches: the fp16 twin of dact_y (same layout), or NULL.  When given, act' is evaluated on it instead of
   * on dact_y -- the sign / value of the previous layer's output as the next layer's GEMM saw it -- and the launch reads
   * 2 instead of 4 bytes per output element (the data gradients of the first layers are bound by exactly these bytes).
   * dact_y must still be passed (it selects the epilogue). */
  const void* dact_y16;
} AliEpilogue;

/* A weight-gradient launch that splits the pixel range writes S partial results ("slabs") into its workspace and
 * sums them in a second launch.  With `fold` given, ali_conv_bwd_weight skips that second launch and describes it here
 * instead (S > 0; S == 0: nothing was deferred, dst is final): the caller gives every such launch of a backward pass its
 * own workspace region (ws_used bytes from the start of the ws it passed stay live) and folds them all with ONE
 * ali_wgrad_fold_multi in front of the optimiser step. */
typedef struct AliWgradFold {
  const float* ws;
  float* dst;
  const float* dbws;
  float* db;
  int64_t slab, s_dc, s_gc, s_tap;
  int32_t S, Mtot, Cg, Cd, Cg_log, Cd_log, T, reserved;
  uint64_t ws_used;
} AliWgradFold;

/* With `job` given (together with `fold`), ali_conv_bwd_weight does not launch its GEMM either when the launch is of
 * the common kind (fp32, 64x64 tiles, pixel table): it records it here (opaque[0] = 1; 0 = it was launched as usual) and
 * the caller issues all recorded launches of a backward pass with ONE ali_wgrad_launch_multi -- in front of
 * ali_wgrad_fold_multi, after the last of their operands has been produced. */
typedef struct AliWgradJob {
  uint64_t opaque[40];
} AliWgradJob;

/* ---- implicit-GEMM convolutions (fp32 MFMA v_mfma_f32_32x32x2_f32) -------
 * ali_conv_fwd       : nn.Conv2d forward  (mnist.py:31-39,100-135; c2d(...) in
 *                      audio_mnist.py:186-198 etc.) and ConvTranspose2d dgrad.
 *                      w_kxc = packed [K][R*S][C]  (ali_pack_weights).
 * ali_conv_bwd_data  : Conv2d data gradient and nn.ConvTranspose2d forward
 *                      (mnist.py:64-72; ct2d(...) audio_mnist.py:228-242) and
 *                      nn.Linear+Unflatten (audio_mnist.py:226-227) as a 4x4
 *                      transposed conv on a 1x1 map. stride 2 is decomposed
 *                      into sub-pixel phases (no zero insertion).
 *                      w_cxk = packed [C][R*S][K].
 * ali_conv_bwd_weight: weight gradient of either; dst[dc*s_dc+gc*s_gc+t*s_tap]
 *                      with gc = channel of x (logical count Cg_log), dc =
 *                      channel of dy (logical count Cd_log), t = r*S+s.     */
size_t ali_conv_workspace_bytes(const AliConvGeom* g, int32_t which /*0 fwd,1 bwd_data,2 bwd_weight*/);
/* Number of M-tiles (= bn_part slots) ali_conv_fwd (which = 0) / ali_conv_bwd_data (which = 1) will launch for this
 * geometry with AliEpilogue.mfma_f16 = mfma_f16, and the tile height in *tile_rows; 0 for a bad geometry.  Rows are ordered (pixel, image) when
 * *pixel_major != 0 (then bn_groups needs B/groups % tile_rows == 0), (image, pixel) otherwise (then it needs
 * B/groups * P*Q % tile_rows == 0). */
int32_t ali_conv_mtiles(const AliConvGeom* g, int32_t which, int32_t mfma_f16, int32_t* tile_rows,
                        int32_t* pixel_major);
/* Host-side: the M-tile ids of the launch ali_conv_fwd (which = 0) / ali_conv_bwd_data (which = 1) makes for g, sorted
 * by k-loop length, longest first (edge tiles of padded / strided-transposed convolutions skip the taps that fall
 * outside the input).  The workgroup dispatcher deals blocks round-robin over the CUs, so dispatching in this order
 * gives every CU the same mix of long and short tiles.  Writes at most cap ids to order (host memory) and returns their
 * number; 0 when all tiles cost the same or the launch cannot use an order.  Upload once per geometry and pass as
 * AliEpilogue.tile_order. */
int32_t ali_conv_tile_order(const AliConvGeom* g, int32_t which, int32_t mfma_f16, int32_t* order, int32_t cap);
/* 1 if the launch ali_conv_fwd (which = 0) / ali_conv_bwd_data (which = 1) makes for g with mfma_f16 = 1 writes
 * AliEpilogue.out16 (every valid geometry does). */
int32_t ali_conv_writes_out16(const AliConvGeom* g, int32_t which);
/* 1 if that launch, given ep (mfma_f16 = 1), multiplies fp16-rounded operands: the uniform-tap GEMM loop (gathered
 * channel count % 32 == 0) and the first Conv2d of the spectrogram stacks (4 / 8 -> 64 channels, 5x5, stride 2,
 * audio_mnist.py:186); every other launch keeps fp32 arithmetic.  What a checker has to know to emulate the launch. */
int32_t ali_conv_uses_f16(const AliConvGeom* g, int32_t which, const AliEpilogue* ep);
/* The launch plan: everything the host decides for one ali_conv_fwd / ali_conv_bwd_data call (DESIGN.md 3.1.1 has the
 * order of the decisions).  The four queries above are views of it. */
typedef struct {
  int32_t route;        /* 0: implicit-GEMM kernel; 1: per-image first conv (8 -> 32 channels, stride 1); 2: row-walking
                           first conv (4 / 8 -> 64 channels, 5x5, stride 2).  Routes 1 and 2 fill route, threads, grid_*
                           (1: also ntile_m = images = bn_part slots, tile_rows = P*Q; 2: f16), the rest is 0 */
  int32_t bm, bn;       /* tile */
  int32_t mode;         /* gather loop: 0 scalar, 1 16-byte gathers, 2 uniform-tap loop, 3 channel stride 4 / 8 / 16 */
  int32_t f16;          /* 0 fp32 MFMA; fp16 MFMA: 1 operands converted in flight, 2 fp16 twins read, 3 LDS-DMA kernel */
  int32_t uni;          /* uniform-tile kernel instance */
  int32_t threads;      /* 256 or 512 */
  int32_t ntile_m, ntile_n, tile_rows, pixel_major;   /* as ali_conv_mtiles, which plans without twins */
  int32_t splitk, kt_per_split;                       /* grid-wide split along K, k-tiles per share */
  int32_t tail_split, tail_u0;    /* the blocks from tail_u0 on are cut tail_split ways along K (1: none) */
  int32_t lin1d, xcd_chunk;       /* 1-D grid (tail split, dispatch order, XCD chunks); blocks per XCD chunk or 0 */
  int32_t ordered;                /* AliEpilogue.tile_order is followed */
  int32_t grid_x, grid_y, grid_z;
  int32_t job_variant;  /* -1: launched at once; 0 / 1: recorded in the AliGemmJob (64x64 / 128x32 multi-job kernel) */
  int32_t empty;        /* nothing to launch */
} AliConvPlan;
/* Host side only (no GPU needed, nothing launched, no operand touched): what ali_conv_fwd (which = 0) /
 * ali_conv_bwd_data (which = 1) would do for g and ep (NULL = no epilogue; pointers are only compared with NULL) given
 * a workspace of ws_bytes (has_ws = 0: a NULL workspace) -- as_job != 0: what ali_conv_fwd_job / ali_conv_bwd_data_job
 * would.  Returns the status and leaves the error text the launch would. */
int32_t ali_conv_plan(const AliConvGeom* g, int32_t which, const AliEpilogue* ep, size_t ws_bytes, int32_t has_ws,
                      int32_t as_job, AliConvPlan* out);
int ali_conv_fwd(const AliConvGeom* g, const float* x, const float* w_kxc, float* y,
                 const AliEpilogue* ep, void* ws, size_t ws_bytes, ali_stream_t stream);
int ali_conv_bwd_data(const AliConvGeom* g, const float* dy, const float* w_cxk, float* dx,
                      const AliEpilogue* ep, void* ws, size_t ws_bytes, ali_stream_t stream);
int ali_conv_bwd_weight(const AliConvGeom* g, const float* x, const float* dy, float* dst,
                        int32_t Cg_log, int32_t Cd_log, int64_t s_dc, int64_t s_gc, int64_t s_tap,
                        float* db /* optional: db[dc] = sum over pixels of dy (Conv2d bias gradient) */,
                        const int32_t* pixtab /* optional: ali_wgrad_pixtab of the same geometry; NULL = the kernel
                                                 computes its gather addresses itself, same result bit for bit */,
                        int32_t mfma_f16 /* as AliEpilogue.mfma_f16 (needs pixtab); accumulation and slabs stay fp32 */,
                        const void* x16, const void* dy16 /* optional fp16 twins of x / dy (AliEpilogue.out16 of the
                                                             launches that produced them): read instead of x / dy */,
                        int32_t dy_ld /* floats between consecutive pixels of dy; 0 = K (dense).  > K: dy is a column
                                         range of wider rows (AliEpilogue.in_ld / out_ld); twins are then not read */,
                        AliWgradFold* fold /* optional: defer the slab reduction, see AliWgradFold */,
                        AliWgradJob* job /* optional (needs fold): defer the launch itself, see AliWgradJob */,
                        int32_t split_target /* with job: blocks this GEMM should have inside the combined launch
                                                (clamped to 256..1024; 0 = 1024, the stand-alone rule) */,
                        void* ws, size_t ws_bytes, ali_stream_t stream);
/* Independent forward / data-gradient GEMMs in ONE launch.  ali_conv_fwd_job / ali_conv_bwd_data_job take the arguments
 * of ali_conv_fwd / ali_conv_bwd_data and, when the launch is of a kind a multi-job kernel exists for (fp32, uniform-tap
 * loop, 64x64 or 128x32 tiles), record it in *job (opaque[0] = 1) instead of launching; any other launch is issued on
 * `stream` right away (opaque[0] = 0), exactly as the plain entry point would.  ali_gemm_launch_multi then issues the
 * recorded jobs: up to 4 of the same kernel variant per launch, longest k-loops first.  The jobs of one call must be
 * mutually independent (no job reads what another writes), each must have been given a workspace of its own (split-K
 * slabs and arrival counters live there), and every operand named at record time must still be alive and unchanged.
 * mnist.py:224-248: E(x) and G(z), the two branches of the E+G backward pass, D.dx and D.dz are such chains. */
typedef struct AliGemmJob {
  uint64_t opaque[112];
} AliGemmJob;
int ali_conv_fwd_job(const AliConvGeom* g, const float* x, const float* w_kxc, float* y, const AliEpilogue* ep,
                     void* ws, size_t ws_bytes, AliGemmJob* job, ali_stream_t stream);
int ali_conv_bwd_data_job(const AliConvGeom* g, const float* dy, const float* w_cxk, float* dx, const AliEpilogue* ep,
                          void* ws, size_t ws_bytes, AliGemmJob* job, ali_stream_t stream);
int ali_gemm_launch_multi(int32_t n, const AliGemmJob* jobs, ali_stream_t stream);

/* Launches deferred weight-gradient GEMMs (jobs[i].opaque[0] == 1 each) together, 12 per launch, longest blocks first.
 * Every operand and workspace region named at ali_conv_bwd_weight time must still be alive and unchanged. */
int ali_wgrad_launch_multi(int32_t n, const AliWgradJob* jobs, ali_stream_t stream);
/* 1 if ali_conv_bwd_weight would defer the launch for this geometry when given a job (pixel table present): lets the
 * caller count a pass's jobs -- and so choose split_target -- before the first launch. */
int32_t ali_wgrad_deferrable(const AliConvGeom* g, int32_t mfma_f16);
/* Folds the slabs of up to any number of deferred weight-gradient launches (jobs[i].S > 0 each) in as few launches as
 * possible (12 jobs per launch), writing every dst / db. */
int ali_wgrad_fold_multi(int32_t n, const AliWgradFold* jobs, ali_stream_t stream);
/* Per-geometry table for ali_conv_bwd_weight: entry i (2 x int32) of output pixel i = (b,p,q) holds the byte offset of
 * x[b, p*stride, q*stride, 0] and the packed pair (p*stride, q*stride); the kernel adds its tap's (r-pad, s-pad).  With it the kernel's gather
 * addresses cost a table read instead of two integer divisions per 16 bytes (fp32 MFMA shares the vector issue
 * path: that arithmetic is 12-27 % of the kernel's issue slots).  Depends on g only; build once, keep, pass along.
 * `out` holds 2 * B*P*Q int32. */
int ali_wgrad_pixtab(const AliConvGeom* g, int32_t* out, ali_stream_t stream);

/* ---- direct kernels for the one-channel ends of the stacks (VALU + LDS, HBM bound) ----------
 * Stride-1 correlations between a K-channel NHWC map `big` [B,P,Q,K] and a 1-channel map `small`
 * [B,H,W] (H = P+R-1-2*pad), used for ConvTranspose2d(64->1,k4)+Tanh (mnist.py:72-73) and for the single
 * consumed input plane / per-input-channel weight gradient of a first Conv2d (mnist.py:108):
 *   fwd   : out[b,h,w]    = act(bias + sum_{r,s,k} big[b,h+pad-r,w+pad-s,k] * w_tk[r*S+s][k])
 *   dgrad : gbig[b,p,q,k] = act'(y[b,p,q,k]) * sum_{r,s} small[b,p+r-pad,q+s-pad] * w_tk[r*S+s][k]
 *   wgrad : dw[c*s_c + k*s_k + (r*S+s)*s_tap] = sum_{b,p,q} big[b,p,q,k] * small[b,p+r-pad,q+s-pad][c]
 *           for the first nc (<= 8) channels c of `small` (element stride sstride between pixels)
 * `sstride` / `ostride`: element stride of the 1-channel map when it is one plane of an NHWC tensor. */
int ali_tconv1_fwd(const float* big, const float* w_tk, const float* bias, float* out, int32_t B, int32_t P,
                   int32_t Q, int32_t K, int32_t R, int32_t S, int32_t pad, int32_t ostride, int32_t act,
                   float slope, const float* rowscale /* optional: out[b,..] *= rowscale[b * rowscale_ld] (the column of
                   a Dropout2d mask when `out` is one plane of a masked input's gradient) */, int32_t rowscale_ld,
                   ali_stream_t stream);
int ali_tconv1_dgrad(const float* small, int32_t sstride, const float* w_tk, const float* dact_y, int32_t dact,
                     float dslope, float* gbig, int32_t B, int32_t P, int32_t Q, int32_t K, int32_t R, int32_t S,
                     int32_t pad, ali_stream_t stream);
int ali_tconv1_wgrad(const float* big, const float* small, int32_t sstride, int32_t nc, float* dw, int64_t s_k,
                     int64_t s_tap, int64_t s_c, int32_t B, int32_t P, int32_t Q, int32_t K, int32_t R, int32_t S,
                     int32_t pad, void* ws, size_t ws_bytes, ali_stream_t stream);
/* Which kernel the three entry points above launch for a shape: the launch and this query read one plan.  `op` is an
 * ALI_T1_OP_*; `nc` and `ws_bytes` (the whole workspace, reserved head included) matter to the weight gradient only.
 * Returns an ALI_T1_* family plus the template arguments of the instantiation, or the negative error code with which
 * the launch would refuse the shape (ali_last_error says why).  Host arithmetic only: works without a GPU.  It reads
 * ALI_NO_T1_MFMA like the launches do. */
#define ALI_T1_OP_FWD 0
#define ALI_T1_OP_DGRAD 1
#define ALI_T1_OP_WGRAD 2
#define ALI_T1_FWD_MFMA 1000   /* + 10 NT + KC : tconv1_fwd_mfma_kernel<NT, KC, 8>, NT tap tiles, KC = K / 16 */
#define ALI_T1_FWD 2000        /* + S          : tconv1_fwd_kernel<S * S, S> */
#define ALI_T1_DGRAD_BAND 3000 /* + R * S      : tconv1_dgrad_band_kernel<R * S> */
#define ALI_T1_DGRAD 4000      /* + R * S      : tconv1_dgrad_kernel<R * S> */
#define ALI_T1_WGRAD_MFMA 5000 /* + NT         : tconv1_wgrad_mfma_kernel<NT, 8> */
#define ALI_T1_WGRAD_RB 6000   /* + 10 nc + S  : tconv1_wgrad_rb_kernel<nc, S> */
#define ALI_T1_WGRAD 7000      /* + nc         : tconv1_wgrad_kernel<nc> */
int32_t ali_tconv1_route(int32_t op, int32_t B, int32_t P, int32_t Q, int32_t K, int32_t R, int32_t S, int32_t pad,
                         int32_t nc, size_t ws_bytes);

/* dst[(n*T+t)*Cpad + c] = c < C ? src[n*s_n + t*s_tap + c*s_c] : 0.
 * Re-lays reference-layout parameters ([Cout,Cin,kh,kw] Conv2d, [Cin,Cout,kh,kw]
 * ConvTranspose2d, [out,in] Linear) into the kernel layouts.   */
int ali_pack_weights(const float* src, float* dst, int32_t N, int32_t T, int32_t C, int32_t Cpad,
                     int64_t s_n, int64_t s_tap, int64_t s_c, ali_stream_t stream);

/* the same for up to 40 parameters in one launch (all packs of a parameter group after its Adam step):
 * dims[4*i..] = {N, T, C, Cpad}, strides[3*i..] = {s_n, s_tap, s_c} of job i (host arrays). */
int ali_pack_weights_multi(int32_t n_jobs, const float* const* src, float* const* dst,
                           void* const* dst16 /* optional (array and entries): fp16 twin of dst[i], written alongside */,
                           const int32_t* dims, const int64_t* strides, ali_stream_t stream);

/* ---- pointwise / reduction kernels (HBM bound) --------------------------- */
/* gpre = gy * act'(y)  (backward of nn.LeakyReLU / nn.Tanh, mnist.py:32-73) */
int ali_act_bwd(const float* gy, const float* y, float* gpre, int64_t n, int32_t act, float slope,
                ali_stream_t stream);
/* out[c] = sum_rows x[row*ld + c]  (bias gradients). ws >= 2048*C floats.  */
int ali_colsum(const float* x, int64_t rows, int32_t C, int32_t ld, float* out, void* ws, size_t ws_bytes,
               ali_stream_t stream);
/* out = x * mask[img, c]   (nn.Dropout2d forward and backward, mnist.py:99-134) */
int ali_rowmask_mul(const float* x, const float* mask, float* out, int32_t B, int32_t rows_per_img, int32_t C,
                    ali_stream_t stream);
/* counter-based Bernoulli(1-p)/(1-p) masks for production runs: draw i uses the key
 * (seed, *dev_counter, offset + i).  dev_counter (device int64, may be NULL) lets a captured
 * HIP graph produce fresh masks on every replay (the stepper bumps it once per iteration). */
int ali_dropout_mask(uint64_t seed, uint64_t offset, const int64_t* dev_counter, float p, float* out, int64_t n,
                     ali_stream_t stream);

/* All masks of one iteration in one launch: segment j is a [rows][seg_cpad[j]] mask stored at elements
 * [seg_end[j-1], seg_end[j]) with drop probability seg_p[j] (host arrays, n_seg <= 64).  Its first seg_clog[j] columns
 * take, row-major, the draws ali_dropout_mask gives with offset = number of draws of the earlier segments; the
 * remaining (channel padding) columns are 1. */
int ali_dropout_mask_multi(uint64_t seed, const int64_t* dev_counter, const int64_t* seg_end, const float* seg_p,
                           const int32_t* seg_clog, const int32_t* seg_cpad, int32_t n_seg, float* out,
                           ali_stream_t stream);

/* nn.BatchNorm2d in training / eval mode (mnist.py:111,114,118,122).
 * stats: per-channel batch mean / biased var of (mask ? x*mask : x), running
 * stats updated with `momentum` and the unbiased variance when `training`;
 * writes sc = gamma*invstd, sh = beta - mean*sc and mean/invstd for backward.
 * apply: out = (x*sc + sh) * (mask_post ? mask_post[img,c] : 1).
 * bwd_reduce: dgamma = sum g~ * xhat, dbeta = sum g~, g~ = g*(mask_pre?mask_pre:1),
 *   xhat computed from x~ = x*(mask_in?mask_in:1).
 * bwd_apply: gx = gamma*invstd*(g~ - dbeta/N - xhat*dgamma/N)   [batch stats]
 *            gx = gamma*invstd*g~                               [eval]
 *            then gx *= mask_in (if given) and *= leaky'(x) (slope >= 0 given). */
/* groups > 1 (stats, apply): the batch holds that many independent forward passes back to back (B/groups images each);
 * statistics, running-stat updates (in group order) and scale/shift are per pass; group g's mean/invstd/sc/sh live at
 * [g*stat_stride + c]. */
int ali_bn_stats(const float* x, const float* mask, int32_t B, int32_t rows_per_img, int32_t C,
                 const float* gamma, const float* beta, float* running_mean, float* running_var,
                 float momentum, float eps, int32_t training,
                 float* mean, float* invstd, float* sc, float* sh, int32_t groups, int64_t stat_stride,
                 void* ws, size_t ws_bytes, ali_stream_t stream);
int ali_bn_apply(const float* x, const float* sc, const float* sh, const float* mask_in, const float* mask_post,
                 float* out, int32_t B, int32_t rows_per_img, int32_t C, int32_t groups, int64_t stat_stride,
                 ali_stream_t stream);
int ali_bn_bwd(const float* x, const float* g, const float* mask_in, const float* mask_pre,
               const float* mean, const float* invstd, const float* gamma,
               int32_t B, int32_t rows_per_img, int32_t C, int32_t batch_stats, float lrelu_slope,
               float* dgamma, float* dbeta, float* gx, void* ws, size_t ws_bytes, ali_stream_t stream);

/* The same two ops fed by the per-tile partial sums a convolution launch left in `part` (AliEpilogue.bn_part, slots =
 * M-tiles of that launch): no reduction pass over the tensor.  stats: training mode only, `count` = rows per pass
 * (B/groups * H*W).  bwd: dgamma / dbeta from the partials, then the elementwise gx pass of ali_bn_bwd. */
int ali_bn_stats_from_partials(const float* part, int32_t slots, int32_t groups, int32_t C, int64_t count,
                               const float* gamma, const float* beta, float* running_mean, float* running_var,
                               float momentum, float eps, float* mean, float* invstd, float* sc, float* sh,
                               int64_t stat_stride, ali_stream_t stream);
int ali_bn_bwd_from_partials(const float* part, int32_t slots, const float* x, const float* g, const float* mask_in,
                             const float* mask_pre, const float* mean, const float* invstd, const float* gamma,
                             int32_t B, int32_t rows_per_img, int32_t C, int32_t batch_stats, float lrelu_slope,
                             float* dgamma, float* dbeta, float* gx, ali_stream_t stream);
/* Which kernels ali_bn_stats, ali_bn_apply, ali_bn_bwd, ali_bn_bwd_from_partials, ali_colsum and ali_act_bwd launch for
 * a shape: the launches and this query read one plan.  `op` is an ALI_EW_OP_*; `rows_per_group` = B/groups *
 * rows_per_img (ali_colsum: rows, ali_act_bwd: n with C = 1); `ld` the row stride of ali_colsum (the others: C);
 * `groups` > 1 for stats and apply only; `aligned` = every tensor operand the entry names is 16-byte aligned.  Returns 1
 * (float4 kernels), 0 (scalar kernels; with groups > 1 one launch per group) with out_blocks (may be NULL) = {reduction
 * blocks per group, 0 without a reduction pass; blocks of the element-wise pass, 0 without one}, or the negative error
 * code with which the launch would refuse the shape.  ali_bn_stats_from_partials has no route to choose (one
 * 256-thread block per channel).  Host arithmetic only: works without a GPU. */
#define ALI_EW_OP_BN_STATS 0
#define ALI_EW_OP_BN_APPLY 1
#define ALI_EW_OP_BN_BWD 2
#define ALI_EW_OP_BN_BWD_FROM_PARTIALS 3
#define ALI_EW_OP_COLSUM 4
#define ALI_EW_OP_ACT_BWD 5
int32_t ali_ew_plan(int32_t op, int64_t rows_per_group, int32_t rows_per_img, int32_t C, int32_t ld, int32_t groups,
                    int32_t aligned, int32_t* out_blocks);

/* nn.BCEWithLogitsLoss (mean) against a constant target, forward + gradient,
 * and the diagnostic sigmoid().mean() (mnist.py:181,228-248).
 * out[0] = loss, out[1] = mean(sigmoid(logit)); glogit[i] = gscale*(sigmoid-t)/B. */
int ali_bce_logits(const float* logit, int32_t B, float target, float gscale, float* out2, float* glogit,
                   ali_stream_t stream);

/* nn.CrossEntropyLoss() (mean) against probability targets, its gradient, the arg-max prediction and the hit count of
 * the classifier loops (classifiers/mnist.py:48-56, audiomnist_generator_score.py:90-98) in one launch; csrc/xent.hip.
 * logit, target: contiguous [B][C] fp32, 1 <= C <= 4096 (ALI_ERR_BAD_ARG before any launch otherwise).  Per row b, with
 * lse_b the max-shifted logsumexp (no overflow for |logit| <= 1e4):
 *   loss_b = -sum_j t_bj (z_bj - lse_b);   out2[0] = mean_b loss_b;
 *   glogit[b][j] = gscale * (softmax_bj * sum_k t_bk - t_bj) / B     (soft targets need not sum to 1);   NULL: skipped
 *   pred[b] = first maximum of the logit row (torch.argmax);   NULL: skipped
 *   out2[1] = number of rows whose pred equals the first maximum of the target row, as a float;
 *   *hits_accum += that number (device int64; NULL: skipped) -- a scoring loop needs no host read per batch.
 * ws: >= ALI_WS_RESERVED + 16 * min(ceil(B / 4), 1024) bytes; the arrival counter is the last int of the reserved head
 * and is left at zero.  No float atomics: bit-identical from run to run.  A NaN logit never becomes the prediction
 * (torch.argmax would pick it) and makes its row's loss and gradient, hence out2[0], NaN. */
int ali_softmax_xent(const float* logit, const float* target, int32_t B, int32_t C, float gscale, float* out2,
                     float* glogit, int32_t* pred, int64_t* hits_accum, void* ws, size_t ws_bytes, ali_stream_t stream);

/* The DeepSCM conditional VAE between its conv stacks (deepscm_vae/mnist.py:121-133 and the audio / whale copies);
 * csrc/vae.hip.  S draws of the latent for B samples are S*B rows (s-major: row = s*B + b) of ONE decoder pass.
 *
 * ali_vae_latent_fwd: out[row][0..L) = mean[b] + eps[row] * exp(k * log_var[b])  (k = 0.5: elbo; k = 1: encoder.sample,
 *   which multiplies by exp(log_var), mnist.py:58-61).  mean / log_var: [B][L] views, rows head_ld floats apart (one
 *   [B][2L] head output serves both).  eps [S*B][L] is read, or, when NULL, drawn from the latent stream of
 *   ali_normal_fill -- element offset + row*L + l under (seed, *dev_counter) -- and stored to eps_out (optional).
 *   write_cond: columns [L, ld) of every row become [onehot_j[b] @ tables[j] (256 each, j < n_emb <= 8) | cont[b] | 0],
 *   the row of ali_g_input; otherwise they are left as they are.  kl_out (optional): kl_out[0] = sum_b dkl_b,
 *   dkl_b = 0.5 sum_l (e^lv + mean^2 - 1 - lv); needs ws >= ALI_WS_RESERVED + 8*B bytes.
 * ali_vae_loglik: x [B][P], xhat [S*B][P], the decoder's scalar log_var (reference: -5):
 *   out3[0] = lp = mean_b (1/S) sum_s ( -0.5 sum_p (x - xhat)^2 e^-log_var - P log_var / 2 - P/2 log 2pi )
 *   out3[2] = kl_sum[0] / B (0 when kl_sum is NULL);   out3[1] = -(lp - kl_weight * out3[2]), the training loss
 *   gxhat (optional) = gscale * (xhat - x) * e^-log_var / (S*B), the loss gradient; 16-byte accesses when P % 4 == 0.
 *   ws >= ALI_WS_RESERVED + 8 * min(S*B, 1024) bytes.
 * ali_vae_latent_bwd: gin [S*B][ld] is the decoder input gradient.  For l < L, with gz = gin[s*B + b][l]:
 *   gmean[b][l]    = sum_s gz + kl_weight * c * mean / B
 *   glog_var[b][l] = sum_s gz * eps * k * e^(k lv) + kl_weight * c * 0.5 (e^lv - 1) / B
 *   (rows gld floats apart; c = kl_scale[0], a device scalar, or 1 when NULL: autograd's incoming gradient).
 *   gcond [B][ncond] (optional) = sum_s gin[s*B + b][L .. L + ncond), what ali_g_input_table_grad takes per table.
 * Every reduction runs in a fixed order in fp64, without float atomics: bit-identical from run to run.  The arrival
 * counter is the last int of the workspace's reserved head and is left at zero. */
int ali_vae_latent_fwd(const float* mean, const float* log_var, int32_t head_ld, const float* eps, float* eps_out,
                       uint64_t seed, const int64_t* dev_counter, uint64_t offset, int32_t S, int32_t B, int32_t L,
                       float k, const void* const* onehot, const int32_t* n_classes, const int32_t* onehot_is_int,
                       const float* const* tables, int32_t n_emb, const float* cont, int32_t n_cont, int32_t write_cond,
                       int32_t ld, float* out, float* kl_out, void* ws, size_t ws_bytes, ali_stream_t stream);
int ali_vae_loglik(const float* x, const float* xhat, int32_t B, int32_t S, int32_t P, float log_var,
                   const float* kl_sum, float kl_weight, float gscale, float* out3, float* gxhat, void* ws,
                   size_t ws_bytes, ali_stream_t stream);
int ali_vae_latent_bwd(const float* gin, int32_t ld, const float* eps, const float* mean, const float* log_var,
                       int32_t head_ld, int32_t S, int32_t B, int32_t L, float k, float kl_weight, const float* kl_scale,
                       float* gmean, float* glog_var, int32_t gld, int32_t ncond, float* gcond, ali_stream_t stream);

/* The counterfactual explainers (explain/cf_example.py); csrc/explain.hip.  Row arithmetic in fp64, fixed reduction
 * order, no float atomics (bit-identical from run to run), no host reads and no allocation: every launch can be recorded
 * into a HIP graph.  Arguments are checked before the launch (ALI_ERR_BAD_ARG, message in ali_last_error).
 *
 * ali_row_dist: out[s] = mean_n |y[s][n] - x[s or 0][n]| (ALI_DIST_L1) or the mean of the squares (ALI_DIST_L2);
 *   x: [xB][N] with xB in {1, S} (1: the one row is compared with every row of y), y: [S][N], 1 <= S <= 65535.  A row is
 *   split over min(ceil(N / 4096), 64) blocks; ws >= ALI_WS_RESERVED + 8 * S * that many bytes; the arrival counter is
 *   the last int of the reserved head and is left at zero.  The `mse` metric of the sweep and the
 *   `(x - x_).abs().mean()` term of the hinge loop (cf_example.py:14,121).
 * ali_cf_hinge: the per-row loss of HingeLossCFExplainer (cf_example.py:111-122); logit [B][C], 2 <= C <= 4096,
 *   target [B] int32, m [B], out3 [B][3] = (c * h + m, h, m), glogit [B][C] (optional) = d (c * h) / d logit.
 *   target[b] >= 0: h = max_{i != t} logit[i] - logit[t]; the maximum is the FIRST one (the strict `>` of
 *   max_excluding); glogit = +c there, -c at t, 0 elsewhere.  target[b] < 0: h = mean_i (logit[i] - orig_pred[b][i])^2,
 *   glogit = 2 c (logit - orig_pred) / C (orig_pred: the softmax row the reference compares the logits with).  Rows are
 *   independent explanations: nothing is averaged over B.  A target >= C, or target < 0 with orig_pred NULL, gives
 *   h = NaN and a zero gradient row.
 * ali_cf_join: gy[b][n] = gx_clf[b][n][0] + sign(x_cf[b][n] - x[b or 0][n]) / N -- plane 0 of the classifier's
 *   NHWC input gradient ([B][N][cpad]) plus the gradient of mean |x - x_cf| (sign(0) = 0, 1 / N as an fp32 division:
 *   exactly torch's fp32 statement); 1 <= N < 2^24, xB in {1, B}.
 * ali_cf_input_fwd: raw optimisation variables -> the generator's input rows (the layout of ali_g_input) and the
 *   transformed attribute rows, one launch, one block per row.  A segment table describes the row: segment q takes
 *   `width` values at column src_off of raw (ALI_CF_TANH, ALI_CF_SOFTMAX: trained) or of given (ALI_CF_COPY: an ignored
 *   feature, or the encoder's codes), transforms them (tanh / softmax over the segment / nothing), stores them at
 *   column attr_off of attrs_out (attr_off < 0: not stored) and writes them to columns dst_off.. of the row (table < 0)
 *   or their product with tables[table] ([width][256], summed over the classes in ascending order) to the 256 columns
 *   at dst_off.  Columns [n_log, ld) become 0.  At most ALI_CF_MAX_SEGMENTS segments; softmax / table segments are at
 *   most 1024 wide and need attr_off >= 0 when they go through a table.
 * ali_cf_input_step: the backward of that map and torch.optim.Adam's update of the trained variables (bias corrected,
 *   eps outside the square root, no decay) in one launch, one block per row.  g_rows [B][ld]: the gradient of the input
 *   rows; rows / attrs: what ali_cf_input_fwd left.  Gradient of the transformed values: g_rows[dst_off + i], or
 *   <g_rows[dst_off .. dst_off + 256), tables[table][k]>; then g * (1 - t^2) (tanh) or the softmax Jacobian
 *   p_k (g_k - sum_j p_j g_j).  raw, m, v: [B][raw_ld]; step [B] int32 counts COMPLETED steps per row: the row's block
 *   reads it, runs step + 1 and stores that back.  graw (optional, [B][raw_ld]): the gradient of the trained columns.
 *   lr, beta1, beta2, eps are doubles, as torch.optim.Adam holds them.
 * ali_cf_select: the tail of DeepCounterfactualExplainer's sweep (cf_example.py:53,64-69): pred[s] = first maximum of
 *   logit[s] ([S][C], S <= 1024, C <= 4096), hit = pred[s] == *target (device int32), order = the hit rows by ascending
 *   metric (ties: ascending row; NaN behind every number, torch.argsort's stable order) followed by the other rows in
 *   row order, *n_hit = the number of hit rows.  One block, rank by counting.  A NaN logit never becomes the prediction
 *   (torch.argmax would pick it). */
#define ALI_DIST_L1 0
#define ALI_DIST_L2 1
#define ALI_CF_COPY 0
#define ALI_CF_TANH 1
#define ALI_CF_SOFTMAX 2
#define ALI_CF_MAX_SEGMENTS 16
#define ALI_CF_EMB 256
typedef struct {
  int32_t kind;      /* ALI_CF_COPY / ALI_CF_TANH / ALI_CF_SOFTMAX */
  int32_t width;
  int32_t src_off;   /* column of raw (trained) or of given (ALI_CF_COPY) */
  int32_t dst_off;   /* column of the generator's input row */
  int32_t table;     /* >= 0: through tables[table] into ALI_CF_EMB columns; < 0: width columns, directly */
  int32_t attr_off;  /* column of the attribute rows; < 0: not kept (z) */
} AliCfSegment;
int ali_row_dist(const float* x, int32_t xB, const float* y, int32_t S, int64_t N, int32_t mode, float* out, void* ws,
                 size_t ws_bytes, ali_stream_t stream);
int ali_cf_hinge(const float* logit, const int32_t* target, const float* orig_pred, const float* m, float c, int32_t B,
                 int32_t C, float* out3, float* glogit, ali_stream_t stream);
int ali_cf_join(const float* gx_clf, int32_t cpad, const float* x_cf, const float* x, int32_t xB, int32_t B, int64_t N,
                float* gy, ali_stream_t stream);
int ali_cf_input_fwd(const float* raw, int32_t raw_ld, const float* given, int32_t given_ld, const AliCfSegment* segs,
                     int32_t n_seg, const float* const* tables, int32_t n_tables, int32_t B, int32_t n_log, int32_t ld,
                     float* rows, float* attrs_out, int32_t attrs_ld, ali_stream_t stream);
int ali_cf_input_step(const float* g_rows, int32_t ld, const float* rows, const float* attrs, int32_t attrs_ld,
                      const AliCfSegment* segs, int32_t n_seg, const float* const* tables, int32_t n_tables, int32_t B,
                      float* raw, float* m, float* v, int32_t raw_ld, int32_t given_ld, int32_t* step, double lr,
                      double beta1, double beta2, double eps, float* graw, ali_stream_t stream);
int ali_cf_select(const float* logit, const float* metric, const int32_t* target, int32_t S, int32_t C, int32_t* pred,
                  int32_t* order, int32_t* n_hit, ali_stream_t stream);

/* Expected gradients (Erion et al.) around the two conv chains: what shap.GradientExplainer(...).shap_values(a) does
 * to f(a) = mean_z softmax(clf(decoder(z, a))) in morphomnist_attribute_shap.py (csrc/attrib.hip).  R explained rows
 * x [R][A], background bg [Nb][A], S interpolated samples per row, n_draws latents per sample, C classes:
 *   a[r,k] = t[r,k] x[r] + (1 - t[r,k]) bg[idx[r,k]],   delta[r,k] = x[r] - bg[idx[r,k]]
 *   phi[r,c,:] = sum_k delta[r,k] * d/da[r,k] ( scale * sum_s softmax(clf(decoder(z[r,k,s], a[r,k])))_c ),
 *   scale = 1 / (S * n_draws).
 * ali_eg_input: (x, bg, idx, t, z) -> the generator's input rows and delta, one launch, one block per (r, k)
 *   (morphomnist_attribute_shap.py:74-79,113-114: the repeat of the attribute columns, randn, and shap's interpolation).
 *   rows [R*S*n_draws][ld] = [z | mixed categorical @ table | mixed continuous | 0], row ((r*S + k)*n_draws + s);
 *   delta [R][S][A] = x - bg[idx], one fp32 subtraction.  The mix is the fp32 rounding of the fp64 expression above;
 *   t == 0 gives bg[idx] and t == 1 gives x, bit for bit.  The segments are AliCfSegment entries (kind ALI_CF_COPY):
 *   `width` attribute columns at src_off go to the row's columns dst_off.. (table < 0) or, times tables[table]
 *   ([width][256], summed over the classes in ascending order), to its 256 columns at dst_off; attr_off is not read.
 *   They must lie in [latent, n_log) and fill it.  A <= 1024.  idx [R][S] int32 (values are clamped into [0, Nb)),
 *   t [R][S] and z [R][S][n_draws][latent] may each be NULL and are then drawn from the counter RNG under (seed,
 *   *dev_counter), `offset` counting the explained rows in front of row 0 (so a call split into row ranges draws what
 *   the whole call draws): idx = (hi24 * Nb) >> 24 and t = lo24 / 2^24 of hash (offset + r) * S + k under the "eg" key
 *   (csrc/ali_rng.h), z element (((offset + r) * S + k) * n_draws + s) * latent + l of ali_normal_fill's stream.
 *   idx_out / t_out (optional, [R][S]) receive the values used.
 * ali_eg_seed: logits [N][K] and a class c -> glogit[n][k] = scale * p_c * ((k == c) - p_k), p the max-subtracted
 *   softmax of the row, evaluated in fp64 and rounded once (the gradient of scale * softmax(.)_c that autograd seeds
 *   through `.softmax(1)` and the mean, :81); p_out [N][K] (optional) receives p.  One thread per row: 1 <= K <= 1024.
 * ali_eg_reduce: g_rows [R*S*n_draws][ld] (the gradient of the generator's input rows at class c) and delta ->
 *   phi[r][c][:] ([R][C][A]; the other classes are not touched): the mean of (x - b) * grad over the samples behind
 *   `vae_explainer.shap_values(a_expl)` (:124,126).  Attribute gradient of a row: g_rows[dst_off + i], or
 *   <g_rows[dst_off .. dst_off + 256), tables[table][i]>; times delta[r][k][i], summed over (k, s) in fp64 in a fixed
 *   order: rows of a 64-row chunk by wave (w, w + 4, ...), waves 0..3, chunks in order by the block that arrives last.
 *   No float atomics: the same inputs give the same bits.  A <= 256; ws >= ALI_WS_RESERVED + 8 * R * A *
 *   ceil(S * n_draws / 64) bytes; the arrival counter is the last int of the reserved head and is left at zero. */
int ali_eg_input(const float* x, const float* bg, const int32_t* idx, const float* t, const float* z, uint64_t seed,
                 const int64_t* dev_counter, uint64_t offset, const AliCfSegment* segs, int32_t n_seg,
                 const float* const* tables, int32_t n_tables, int32_t R, int32_t S, int32_t n_draws, int32_t Nb,
                 int32_t A, int32_t latent, int32_t n_log, int32_t ld, float* rows, float* delta, int32_t* idx_out,
                 float* t_out, ali_stream_t stream);
int ali_eg_seed(const float* logit, int64_t N, int32_t K, int32_t c, double scale, float* glogit, float* p_out,
                ali_stream_t stream);
int ali_eg_reduce(const float* g_rows, int32_t ld, const float* delta, const AliCfSegment* segs, int32_t n_seg,
                  const float* const* tables, int32_t n_tables, int32_t R, int32_t S, int32_t n_draws, int32_t A,
                  int32_t C, int32_t c, float* phi, void* ws, size_t ws_bytes, ali_stream_t stream);

/* The contrastive family (csrc/contrast.hip): the pertinent-negative search of the contrastive explanation method
 * (Dhurandhar et al. 2018) and the counterfactual search of Wachter et al. 2017, B rows as B independent searches around
 * the classifier's chain (DESIGN 3.19 has the statement).  Per row b: the image x0 [N], its label t0, the bounds lo / hi,
 * the iterate v (and the slack y, or Adam's m / v2), the search constants c / c_lo / c_hi, the counters it (iteration
 * of the round, 0..K) and rnd, the best so far.  Everything a launch branches on is read from device memory, so one
 * recorded graph serves every iteration of every round; all four write with ordinary vector stores, reduce in a fixed
 * order in fp64 (no float atomics: the same inputs give the same bits) and need no workspace.
 * ali_ct_attack: logit [R][C], 2 <= C <= 1024, one thread per search row b < B.  Row eval_off + b is evaluated:
 *   pred[b] = its first arg-max (ties to the first index, as ali_softmax_xent), succ[b] = pred[b] != t0[b].  Row
 *   grad_off + b is attacked: own = s[t0], other = the largest s[j], j != t0 (first on ties), A[b] = max(0, own - other
 *   + kappa) and seed[b][:] = c[b] * (e_t0 - e_other) where own - other + kappa > 0 (evaluated in fp64), else 0;
 *   the columns [C, seed_ld) are 0: the gradient of the last stage's output as chain_backward takes it.
 *   t0 == NULL: only pred is written (the labels of x0 themselves).
 * ali_ct_book: one block per row, k = it[b].  k >= 1 and succ[b]: the round has a success; with dist[b] < best_dist[b]
 *   the row v[b] is copied into best[b] (otherwise best is not written), best_dist / best_label (= pred[b]) follow and
 *   found[b] = 1; copied[b] says whether that happened in this launch.  k == K closes the round: after a success
 *   c_hi = min(c_hi, c), c = (c_lo + c_hi) / 2; otherwise c_lo = max(c_lo, c) and c = (c_lo + c_hi) / 2 if c_hi < 1e9
 *   else 10 c; round_succ[b] = 0.  it is not written: the update that follows in the stream sees the same k.
 * ali_ct_cem_update: one block per row.  k == K: v = y = x0, it = 0, rnd += 1, the distances 0.  k < K, with gx the
 *   classifier's input gradient at y (element i of row b at gx[(b * N + i) * gx_stride]):
 *     g = gx + 2 (y - x0);  norm = |g|_2 -> gnorm;  g *= clip / norm if norm > clip;  u = y - lr sqrt(1 - k / K) g
 *     w = min(u - beta, hi) if u - x0 > beta, max(u + beta, lo) if u - x0 < -beta, else x0;  v' = w if w > x0 else x0
 *     y' = v' + k / (k + 3) (v' - v), then x0 where y' <= x0;  l1 = |v' - x0|_1, l2 = |v' - x0|_2^2 of v' as stored,
 *     dist = l2 + beta l1;  it = k + 1.  Pixels that fall back to x0, lo or hi receive those floats themselves.
 * ali_ct_ce_update: one block per row.  k == K: v = x0, m = v2 = 0, it = 0, rnd += 1, l1 = 0.  k < K:
 *     g = gx + gamma sign(v - x0) (sign(0) = 0), the same clip, Adam (torch.optim.Adam's formula) at step k + 1,
 *     v' clamped to [lo, hi], l1 = |v' - x0|_1 of v' as stored, it = k + 1.
 *   Rows of N % 4 == 0 floats in 16-byte aligned buffers move as 16-byte accesses.  N < 2^31, gx_stride in [1, 64]. */
int ali_ct_attack(const float* logit, int32_t R, int32_t C, int32_t B, int32_t eval_off, int32_t grad_off,
                  const int32_t* t0, const float* c, double kappa, float* seed, int32_t seed_ld, float* A, int32_t* pred,
                  int32_t* succ, ali_stream_t stream);
int ali_ct_book(const float* v, const float* dist, const int32_t* succ, const int32_t* pred, const int32_t* it,
                int32_t K, int32_t B, int64_t N, float* best, float* best_dist, int32_t* best_label, int32_t* found,
                int32_t* round_succ, float* c, float* c_lo, float* c_hi, int32_t* copied, ali_stream_t stream);
int ali_ct_cem_update(const float* gx, int32_t gx_stride, float* v, float* y, const float* x0, const float* lo,
                      const float* hi, int32_t* it, int32_t* rnd, int32_t K, double lr, double beta, double clip,
                      int32_t B, int64_t N, float* l1, float* l2, float* dist, float* gnorm, ali_stream_t stream);
int ali_ct_ce_update(const float* gx, int32_t gx_stride, float* v, const float* x0, const float* lo, const float* hi,
                     float* m, float* v2, int32_t* it, int32_t* rnd, int32_t K, double lr, double gamma, double clip,
                     double beta1, double beta2, double eps, int32_t B, int64_t N, float* l1, float* gnorm,
                     ali_stream_t stream);
/* The pertinent-positive search ("Pertinent positives"): the background b (an fp32 "no information" pixel
 * value) replaces x0 as the centre, the box of pixel i is [min(b, x0_i), max(b, x0_i)].  ali_ct_book serves it as is.
 * ali_ct_pp_attack: ali_ct_attack's arguments with t0 required and the hinge turned round: succ[b] = pred[b] == t0[b];
 *   A[b] = max(0, other - own + kappa) and seed[b][:] = c[b] * (e_other - e_t0) where other - own + kappa > 0, else 0;
 *   the columns [C, seed_ld) are 0.
 * ali_ct_pp_update: one block per row.  k == K: v = y = b, it = 0, rnd += 1, the distances 0.  k < K, with gx the
 *   classifier's input gradient at y:
 *     g = gx + 2 (y - b);  norm = |g|_2 -> gnorm;  g *= clip / norm if norm > clip;  u = y - lr sqrt(1 - k / K) g
 *     w = u - beta if u - b > beta, u + beta if u - b < -beta, else b;  v' = w clamped to the box
 *     y' = v' + k / (k + 3) (v' - v) clamped to the box;  l1 = |v' - b|_1, l2 = |v' - b|_2^2 of v' as stored,
 *     dist = l2 + beta l1;  it = k + 1.  Pixels that fall back to b or x0 receive those floats themselves.
 *   Rows and gx as ali_ct_cem_update. */
int ali_ct_pp_attack(const float* logit, int32_t R, int32_t C, int32_t B, int32_t eval_off, int32_t grad_off,
                     const int32_t* t0, const float* c, double kappa, float* seed, int32_t seed_ld, float* A,
                     int32_t* pred, int32_t* succ, ali_stream_t stream);
int ali_ct_pp_update(const float* gx, int32_t gx_stride, float* v, float* y, const float* x0, float background,
                     int32_t* it, int32_t* rnd, int32_t K, double lr, double beta, double clip, int32_t B, int64_t N,
                     float* l1, float* l2, float* dist, float* gnorm, ali_stream_t stream);

/* torch.optim.Adam step (mnist.py:176-179,230,236,241), no amsgrad / decay.
 * One launch over a flat parameter segment.  The 1-based step count is `step`, or *dev_step when
 * dev_step != NULL (graph replays); the gradient is read as grad_scale * g (1/world for DP).
 * With `arrive` (a zeroed device int32 the launch leaves at zero; needs dev_step): *dev_step is the number of COMPLETED
 * steps -- the launch runs step *dev_step + 1 and its last block stores that value back, so a captured graph's step
 * count advances without a launch of its own.  p16 (optional, n halves): also leave (_Float16)p -- the fp16 twin of
 * master weights that already live in a GEMM's layout (AliEpilogue.w16), so that no re-pack launch has to produce it. */
int ali_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
             float eps, int32_t step, int32_t* dev_step, int32_t* arrive, float grad_scale, void* p16,
             ali_stream_t stream);
/* counters[i][0] += incs[i] for n device int64 counters in one launch (nn.BatchNorm2d.num_batches_tracked of every
 * layer, mnist.py:111-123 forward in train mode; the stepper's iteration counter).  A counter may be named more than
 * once: it receives every increment. */
int ali_add_i64_multi(int32_t n, int64_t* const* counters, const int64_t* incs, ali_stream_t stream);

/* BCEWithLogitsLoss of two passes batched along the rows, rows [0,B) against target_a and [B,2B) against target_b
 * (mnist.py:228: (bce(D_valid, 0) + bce(D_fake, 1)) / 2; :245-248: the two sigmoid().mean() scores):
 * out3 = {(loss_a + loss_b)/2, mean sigmoid(a), mean sigmoid(b)}; glogit[i] = gscale*(sigmoid - target)/B or NULL. */
int ali_bce_logits_pair(const float* logit, int32_t B, float target_a, float target_b, float gscale, float* out3,
                        float* glogit, ali_stream_t stream);

/* Between the conv stacks of a WGAN-GP critic step (gans/audio_mnist.py: wgan_loss_it, compute_gradient_penalty);
 * csrc/gan.hip.  x_real, x_fake, xhat, g0, v: contiguous [B][P] fp32, 1 <= B <= 65535; 16-byte accesses when P % 4 == 0
 * and the pointers are 16-byte aligned, one element at a time otherwise.
 *
 * ali_gp_mix: xhat[b][p] = eps[b] * x_real[b][p] + (1 - eps[b]) * x_fake[b][p], the products and the sum rounded one by
 *   one (torch's fp32 statement bit for bit).  eps [B] is read, or, when NULL, drawn per image, uniform in [0, 1) (24
 *   bits), from the counter RNG of ali_normal_fill under a key of its own: image b is element offset + b of the stream
 *   keyed by (seed, *dev_counter; dev_counter may be NULL) -- a captured graph advances with the device counter.  The
 *   eps used is stored to eps_out [B] (optional).
 * ali_gp_penalty: g0 is the gradient of sum_b D(xhat_b) with respect to xhat.  n_b = ||g0_b||_2;
 *   out2[0] = mean_b (n_b - 1)^2;  out2[1] = mean_b n_b;
 *   v[b][p] = lambda * (2 / B) * (1 - 1 / n_b) * g0[b][p]  (NULL: skipped; v_b = 0 where n_b == 0, as torch's norm
 *   backward) -- the gradient of lambda * out2[0] with respect to g0.  v may be g0 itself.  One launch, one block per
 *   image; ws >= ALI_WS_RESERVED + 16 * B bytes; the arrival counter is the last int of the reserved head and is left
 *   at zero.  fp64 sums in a fixed order, no float atomics: bit-identical from run to run.
 * ali_wgan_critic: logits d_fake [B], d_real [B] (either may be NULL, its mean is then 0):
 *   out3[0] = mean(d_fake) - mean(d_real);  out3[1] = mean(d_fake);  out3[2] = mean(d_real);
 *   g_fake[b] = gscale / B;  g_real[b] = -gscale / B  (each optional; needs its logits).  The generator's loss
 *   -mean D(G(z)) is the call with d_real = NULL, gscale = -1: out3[0] is then its negative. */
int ali_gp_mix(const float* x_real, const float* x_fake, const float* eps, uint64_t seed, const int64_t* dev_counter,
               uint64_t offset, int32_t B, int64_t P, float* xhat, float* eps_out, ali_stream_t stream);
int ali_gp_penalty(const float* g0, int32_t B, int64_t P, float lambda, float* out2, float* v, void* ws,
                   size_t ws_bytes, ali_stream_t stream);
int ali_wgan_critic(const float* d_fake, const float* d_real, int32_t B, float gscale, float* out3, float* g_fake,
                    float* g_real, ali_stream_t stream);

/* The MorphoMNIST attribute SCM (attribute_scms/mnist.py, attribute_scms/_flows.py: the statement) and the Gumbel-max
 * posterior of the conditional categoricals (attribute_scms/causal_module.py); csrc/flow.hip.
 *
 * theta: the trainable state, ALI_FLOW_THETA = 75 floats
 *   gamma, beta | W1[10] b1[10] W2[2][10] b2[2] | uw[8] uh[8] ud[7] ul[8]
 *   (BatchNorm of log thickness | Linear(1,10) -> ReLU -> Linear(10,2) = (mean, log_scale) of the intensity's affine
 *   flow given the raw thickness | raw widths, heights, knot derivatives, lambdas of the slant's rational-linear spline,
 *   8 bins on [-3, 3]^2).  cst: 4 floats {i_min, i_max - i_min, s_min, s_max - s_min}.  stats: 2 device floats {mean,
 *   variance} of log thickness, a batch's (ali_flow_stats) or the moving buffers.  eps = 1e-5; g = relu(gamma) + 1e-6.
 *   Rows are evaluated in fp64 and rounded once; all sums are fp64 in a fixed order (threads strided over rows, lanes,
 *   waves, blocks ascending in the block that arrives last), no float atomics: the same inputs give the same bits.
 *   ws >= ALI_WS_RESERVED + 8 * 103 * 64 bytes serves every entry; the arrival counter (last int of the reserved head)
 *   is left at zero.
 *
 * ali_flow_stats: out2 = {mean, unbiased variance} of log t[n * stride], n < N.  moving (optional, 2 floats {mean,
 *   variance}): moving <- (1 - momentum) * moving + momentum * out2 in the same launch; N < 2 is then ALI_ERR_BAD_ARG
 *   before any launch (torch yields NaN statistics there and poisons the buffers).  Without moving, N == 1 gives a NaN
 *   variance as torch does.
 *
 * ali_flow_nll: the three log-densities of rows (t, i, s) -- columns with row strides st, si, ss (in floats):
 *   thickness  x1 = log t; u = (x1 - m) rsqrt(v + eps) g + beta;  lp = N(u) - x1 + log g - log(v + eps) / 2
 *   intensity  p = clamp((i - i_min) / i_rng, FLT_MIN, 1 - FLT_EPSILON); w = log p - log1p(-p);
 *              h = relu(W1 t + b1); (mean, a) = W2 h + b2; ls = clamp(a, -5, 3); u = (w - mean) exp(-ls);
 *              lp = N(u) - ls + softplus(-w) + softplus(w) - log i_rng
 *   slant      q = (s - s_min) / s_rng; u = spline^-1(q);  lp = N(u) + log(du/dq) - log s_rng
 *   with N(u) = -u^2 / 2 - log(2 pi) / 2.  lp [N][3] (optional); out4 (optional) = {-mean_n(lp_t + lp_i + lp_s),
 *   mean lp_t, mean lp_i, mean lp_s}; gtheta [75] (optional) = sum_n sum_j wgt[n][j] * d lp[n][j] / d theta, wgt a
 *   [N][3] device array or, when NULL, the constant gscale / N.  The statistics depend on data alone and carry no
 *   gradient; gamma and the hidden units are gated by their ReLU; the clamp of a passes the gradient straight through.
 *
 * ali_flow_map: the mechanisms elementwise on rows in [N][3] -> out [N][3] (thickness, intensity, slant).  Per column
 *   ALI_FLOW_SKIP (copied through), ALI_FLOW_FORWARD (noise -> value) or ALI_FLOW_INVERSE (value -> noise); the
 *   intensity's context is the thickness VALUE of the row: the column's output when it runs forward, its input
 *   otherwise.  Inverse BatchNorm reads stats_inv, forward BatchNorm stats_fwd (the moving buffers).  The spline is
 *   the identity outside [-3, 3]; sigmoid's output is clamped like p above.
 *   cf != 0 (the modes are ignored): in = observed rows; columns named in cf_mask (bit 0 thickness, 1 intensity, 2
 *   slant) take val [N][3], every other column is forward(inverse(observed | observed parents) | counterfactual
 *   parents), thickness before intensity; the abducted noise goes to noise_out [N][3] (optional).  val may be NULL
 *   when cf_mask == 0.  out may be in.
 *
 * ali_gumbel_posterior: logits [N][C], y [N] (int64, in [0, C)), 1 <= C <= 4096, one wave per row:
 *   noise[n][y] = g_y + lse(logits_n) - logit_y  (lse max-shifted, fp64)
 *   noise[n][l] = -log(exp(-g_l - logit_l) + exp(-g_y - logit_y)) - logit_l
 *   so that argmax_l(logits + noise) = y.  g [N][C] ~ Gumbel(0, 1) is read, or, when NULL, drawn from the counter RNG
 *   of ali_normal_fill under a key of its own: g = -log(-log u), u = (k + 0.5) / 2^24 strictly inside (0, 1), k the
 *   top 24 bits of the hash of element offset + n * C + l of the stream keyed by (seed, *dev_counter; may be NULL).
 *   The g used is stored to g_out (optional).  ali_hip.source.gumbel_reference is the recipe in fp64.  A y outside
 *   [0, C) is not checked (it is device data): such a row gets NaN and no out-of-bounds access is made. */
#define ALI_FLOW_THETA 75
typedef enum { ALI_FLOW_SKIP = 0, ALI_FLOW_FORWARD = 1, ALI_FLOW_INVERSE = 2 } AliFlowMode;
int ali_flow_stats(const float* t, int64_t stride, int64_t N, float* out2, float* moving, float momentum, void* ws,
                   size_t ws_bytes, ali_stream_t stream);
int ali_flow_nll(const float* t, int64_t st, const float* i, int64_t si, const float* s, int64_t ss, int64_t N,
                 const float* theta, const float* cst, const float* stats, const float* wgt, float gscale, float* lp,
                 float* out4, float* gtheta, void* ws, size_t ws_bytes, ali_stream_t stream);
int ali_flow_map(const float* in, const float* val, float* out, float* noise_out, int64_t N, int32_t mode_t,
                 int32_t mode_i, int32_t mode_s, int32_t cf, int32_t cf_mask, const float* theta, const float* cst,
                 const float* stats_inv, const float* stats_fwd, ali_stream_t stream);
int ali_gumbel_posterior(const float* logits, const int64_t* y, const float* g, uint64_t seed,
                         const int64_t* dev_counter, uint64_t offset, int32_t N, int32_t C, float* noise, float* g_out,
                         ali_stream_t stream);

/* The AudioMNIST attribute SCM (attribute_scms/audio_mnist.py: the statement); csrc/cat.hip.
 *   native_speaker  logits = W4 relu(W3 relu(W2 relu(W1 c + b1) + b2) + b3) + b4, c the country row, 128 wide
 *   accent          logits = V2 relu(V1 [tower_c(c) | tower_n(n)] + c1) + c2, n the native_speaker row, each tower
 *                   Linear(C, 64) ReLU Linear(64, 64) ReLU Linear(64, 64) ReLU Linear(64, 64), frozen
 * Cc, Cn, Ca (classes of country_of_origin, native_speaker, accent) lie in [1, 64], N in [1, 2^24): anything else is
 * ALI_ERR_BAD_ARG before any launch.  Weights are torch Linear's [out][in], row-major.
 *   theta  (trained, ali_cat_theta_size(Cc, Cn, Ca, 0) floats):
 *          W1[128][Cc] b1[128] W2[128][128] b2[128] W3[128][128] b3[128] W4[Cn][128] b4[Cn] | V1[64][128] c1[64]
 *          V2[Ca][64] c2[Ca]
 *   towers (frozen, ali_cat_theta_size(Cc, Cn, Ca, 1) floats): tower_c then tower_n, each
 *          A1[64][C] a1[64] A2[64][64] a2[64] A3[64][64] a3[64] A4[64][64] a4[64]
 * Context and target rows are fp32 rows at a row stride (in floats, >= the width, <= 2^16), read as dense rows.  The
 * matrix products run on the fp64 MFMA (fp32 operands are exact in it, activations stay fp64 between layers) and every
 * result is rounded to fp32 once.  Sums over rows have fixed orders, no float atomics: the same inputs give the same bits.
 *
 * ali_cat_plan (host only): how entry (AliCatEntry) runs N rows -- a grid of `grid` blocks of `threads` threads, block b
 *   taking the row tiles t = b, b + grid, ... < tiles (at most tiles_per_block of them), tile t being rows
 *   [t * tile_rows, min(N, (t + 1) * tile_rows)); grid2 x threads2: the weight-gradient launch of ALI_CAT_ENTRY_GRAD;
 *   ws_bytes: the workspace the entry needs (0 for ali_cat_map).  The launches use the same function.
 *
 * ali_cat_nll: row n reads source row index[n] (int64, optional; src_rows = rows of the tables, ignored without index)
 *   of country, native and accent; a row's class is the first maximum of its target row.  An index outside
 *   [0, src_rows) is not checked (device data): such a row reads nothing, its lp is NaN.
 *   lp [N][2] (optional) = log softmax(logits)[class] of native_speaker and accent, the log-softmax max-shifted in fp64;
 *   out3 (optional) = {-mean(lp_n + lp_a), mean lp_n, mean lp_a};
 *   gtheta (optional, theta's layout; the second launch) = gscale * sum_n (wgt[n][0] d lp_n + wgt[n][1] d lp_a) / d theta,
 *   wgt [N][2] or, NULL, 1 / N each.  A ReLU passes the gradient where its pre-activation is > 0.  The towers get none.
 *   The arrival counter (last int of the reserved head) is left at zero.
 *
 * ali_cat_map: one launch, row-wise, mode (AliCatMode) over AliCatMapArgs.  Every decision is the first maximum of the
 *   fp64 sums of stored fp32 values: the logits rounded to fp32 (logits_out [N][Cn + Ca], native_speaker's columns
 *   first; ALI_CAT_CF: [2][N][Cn + Ca], observed then counterfactual parents) plus the draws g (g_out) or the noise
 *   (noise_out [N][Cn + Ca]).  Draws are ali_gumbel_posterior's: g = gumbel(element e) of the stream keyed by (seed,
 *   *dev_counter); a call uses the elements from `offset` on as stated per mode.  Classes are int64; a class outside
 *   its range is not checked (device data): as a parent it is a zero row, as an observation its noise is NaN.
 *   ALI_CAT_LOGITS  logits_out for country and native_rows (dense, optional) or the one-hot of y[0]
 *   ALI_CAT_SAMPLE  native_speaker then accent, each held (y[node] given) or drawn: out[node] = argmax(logits + g), g at
 *                   e = offset + n (Cn + Ca) + col, col the node's column in logits_out; g_out [N][Cn + Ca]
 *   ALI_CAT_DIFFER  like SAMPLE, but node `node` is drawn up to ALI_CAT_TRIES times, try t at e = offset + (t N + n) C +
 *                   class (C the node's classes), keeping the first try whose class is not v[node][n]; status[n] = 1
 *                   when none is (out holds the last try).  g_out [ALI_CAT_TRIES][N][C] (optional) makes it draw and
 *                   store every try.  The other node's draws lie behind the tries: offset + ALI_CAT_TRIES N C + the
 *                   SAMPLE element.
 *   ALI_CAT_ABDUCT  noise_out = the Gumbel posterior (ali_gumbel_posterior's formulas on the fp32 logits) of the observed
 *                   y[0] under country and of y[1] under (country, y[0]); g as in SAMPLE
 *   ALI_CAT_CF      abduction as above, then native_speaker before accent under country_cf (NULL: country): a node in
 *                   cf_mask (bit 0 native_speaker, bit 1 accent) takes v[node], another argmax(logits(counterfactual
 *                   parents) + noise) -> out[node] */
#define ALI_CAT_TRIES 64
typedef enum { ALI_CAT_LOGITS = 0, ALI_CAT_SAMPLE = 1, ALI_CAT_DIFFER = 2, ALI_CAT_ABDUCT = 3, ALI_CAT_CF = 4 } AliCatMode;
typedef enum { ALI_CAT_ENTRY_NLL = 0, ALI_CAT_ENTRY_GRAD = 1, ALI_CAT_ENTRY_MAP = 2 } AliCatEntry;
typedef struct AliCatPlan {
  int32_t grid, threads, tile_rows, tiles, tiles_per_block, grid2, threads2, lds_bytes;
  uint64_t ws_bytes;
} AliCatPlan;
typedef struct AliCatMapArgs {
  const float* country;     int64_t country_ld;
  const float* country_cf;  int64_t country_cf_ld;
  const float* native_rows; int64_t native_ld;
  const int64_t* y[2];      /* classes of native_speaker, accent: held (SAMPLE, DIFFER; NULL = drawn) or observed */
  const int64_t* v[2];      /* CF: the values of the nodes in cf_mask; DIFFER: v[node] = the forbidden classes */
  int32_t node, cf_mask;
  int64_t* out[2];
  int32_t* status;
  float* logits_out;
  float* g_out;
  float* noise_out;
} AliCatMapArgs;
int ali_cat_plan(int64_t N, int32_t Cc, int32_t Cn, int32_t Ca, int32_t entry, AliCatPlan* plan);
int32_t ali_cat_theta_size(int32_t Cc, int32_t Cn, int32_t Ca, int32_t towers); /* 0: a class count out of range */
int ali_cat_nll(const float* theta, const float* towers, int32_t Cc, int32_t Cn, int32_t Ca, const float* country,
                int64_t sc, const float* native, int64_t sn, const float* accent, int64_t sa, const int64_t* index,
                int64_t src_rows, int64_t N, const float* wgt, float gscale, float* lp, float* out3, float* gtheta,
                void* ws, size_t ws_bytes, ali_stream_t stream);
int ali_cat_map(int32_t mode, const float* theta, const float* towers, int32_t Cc, int32_t Cn, int32_t Ca, int64_t N,
                const AliCatMapArgs* args, uint64_t seed, const int64_t* dev_counter, uint64_t offset,
                ali_stream_t stream);

/* The counterfactual metrics family (train_morphomnist_ae.py, morphomnist_cf_metrics.py, mnist_oracle_scores.py);
 * csrc/cfmetrics.hip.  fp32 in and out, fp64 sums in a fixed order, no float atomics: bit-identical from run to run.
 *
 * ali_mse: loss[0] = mean_i (y_i - x_i)^2 over n elements;  grad[i] (optional) = 2 * gscale * (y_i - x_i) / n, times
 *   1 - y_i^2 when tanh_out != 0 (y is then the output of a tanh and grad the gradient of its pre-activation).  One
 *   launch of min(ceil(n / 1024), 1024) blocks with 16-byte accesses when y, x and grad are 16-byte aligned, of
 *   min(ceil(n / 256), 1024) blocks element by element otherwise.  ws >= ALI_WS_RESERVED + 8 * min(ceil(n / 256),
 *   1024) bytes serves both; the arrival counter is the last int of the reserved head and is left at zero.
 * ali_cf_recon: x [B][N] contiguous; recon [A][B][N], element (a, b, j) at a * ld_plane + b * ld_row + j; orig,
 *   target [B] int32 device labels; out [B][4] (16-byte aligned) =
 *     { sum_j |x|,  sum_j (x - recon[orig])^2,  sum_j (x - recon[target])^2,  sum_j (recon[target] - recon[A-1])^2 }
 *   (plane A - 1: the autoencoder of all classes).  A label outside [0, A - 1) indexes nothing: the columns that
 *   depend on it are NaN.  One wave per row, no workspace.
 * ali_oracle_scores: pred [B] int32; ox, ocf [J][B][C] logits of J oracles on the original and on the counterfactual,
 *   element (j, b, c) of either at j * ld_j + b * C + c, C >= 1.  os[b][j] = (pred[b] == first arg-max of
 *   ocf[j][b][:]);  lvs[b][j] = the Jensen-Shannon divergence 0.5 * (KL(p, m) + KL(q, m)), p = softmax(ox[j][b]),
 *   q = softmax(ocf[j][b]) (max-shifted, fp64), m = (p + q) / 2, KL(a, m) = sum_c a_c * (log(a_c + 1e-6) -
 *   log(m_c + 1e-6)).  One wave per (b, j).
 * Non-finite inputs (what falls out, untested): comparisons with NaN are false, so a NaN logit never becomes the
 *   arg-max -- torch.argmax would pick it -- and a row of NaN alone gives os = 0; its lvs is NaN.  NaN or infinite
 *   images give NaN sums. */
int ali_mse(const float* y, const float* x, int64_t n, float gscale, int32_t tanh_out, float* loss, float* grad,
            void* ws, size_t ws_bytes, ali_stream_t stream);
int ali_cf_recon(const float* x, const float* recon, int64_t ld_row, int64_t ld_plane, const int32_t* orig,
                 const int32_t* target, int32_t A, int32_t B, int32_t N, float* out, ali_stream_t stream);
int ali_oracle_scores(const int32_t* pred, const float* ox, const float* ocf, int64_t ld_j, int32_t J, int32_t B,
                      int32_t C, int32_t* os, float* lvs, ali_stream_t stream);

/* The counterfactual identity metrics (audiomnist_cf_eval.py:93-131: the mean squared distance of a counterfactual to
 * the real recordings of its own subject and target class over the one to every other subject's); csrc/cfeval.hip.
 * For a cell (owner, class) of n bank rows b_j with column sums S and column sums of squares Q,
 *   sum_j ||a - b_j||^2 = sum_k (n a_k^2 - 2 a_k S_k + Q_k),
 * so the bank is read once (ali_group_moments) and a counterfactual row costs one pass over its own D columns
 * (ali_manifold_err).  Moments are fp64: the products of fp32 values are exact there, and the cancellation inside a
 * column keeps 1e-16 of n a^2.  fp64 sums in a fixed order, no float atomics (bit-identical from run to run), no host
 * reads, no allocation: every launch can be recorded into a HIP graph.  Arguments are checked before the launch
 * (ALI_ERR_BAD_ARG, message in ali_last_error); 1 <= O * C <= 65535; cell = owner * C + class.
 *
 * ali_group_moments: rows [N][D] fp32, row r at r * ld (ld >= D); order [n_order] int32 (n_order <= N): the indices of
 *   the rows that belong to a cell, sorted by cell, stable (ascending row inside a cell); start [O * C + 1] int32: the
 *   cell's rows are order[start[cell] .. start[cell + 1]).  S, Q [O * C][D] double: the column sums and column sums of
 *   squares of each cell, its rows added in ascending row order from 0; an empty cell gives +0.  TS, TQ [C][D] double:
 *   the fold of that class's cells in ascending owner order from 0, so that a class held by one owner has TS - S == 0
 *   exactly.  Two launches (column chunks x cells, column chunks x classes), no workspace; 16-byte loads and stores
 *   when D % 4 == 0, ld % 4 == 0 and rows, S, Q are 16-byte aligned, one element at a time otherwise -- the same bits
 *   either way.  order and start are device data: an index outside [0, N) adds nothing, offsets are clamped to
 *   [0, n_order].
 * ali_manifold_err: cf [M][D] fp32, row m at m * ld (ld >= D), 1 <= M <= 65535; owner, cls [M] DEVICE int32 (one graph
 *   serves every batch); the four moment arrays; cnt [O * C], tcnt [C] int32: the rows per cell and per class.
 *   out3 [M][3] = (same, other, ratio): with n = cnt[cell],
 *     same  = sum_k (n a_k^2 - 2 a_k S_k + Q_k) / n
 *     other = the same expression on (TS - S, TQ - Q, tcnt[class] - n)
 *     ratio = same / other
 *   evaluated in double per column, accumulated in double, each rounded to fp32 once (ratio from the unrounded two).
 *   The reference's 0 / 0 is written out, not left to the arithmetic: n == 0 gives same = NaN; tcnt - n == 0 gives
 *   other = NaN; an owner outside [0, O) with a valid class -- a subject the bank has never seen -- gives same = NaN
 *   and other over the whole class; a class outside [0, C) gives three NaNs; ratio is NaN when either part is.  A row
 *   equal to the only row of its cell gives same == 0 exactly.  A row is split over min(ceil(D / 4096), 64) blocks;
 *   ws >= ALI_WS_RESERVED + 16 * M * that many bytes (two fp64 partials per row and block); the block that arrives
 *   last folds each row's partials in block order; the arrival counter is the last int of the reserved head and is
 *   left at zero.  16-byte loads when D % 4 == 0, ld % 4 == 0 and cf and the moment arrays are 16-byte aligned.
 * Non-finite inputs (what falls out, untested): a NaN or infinite element makes the sums of its row (cf) or of its
 *   cell and class (bank) NaN. */
int ali_group_moments(const float* rows, int64_t ld, int32_t N, int32_t D, const int32_t* order, int32_t n_order,
                      const int32_t* start, int32_t O, int32_t C, double* S, double* Q, double* TS, double* TQ,
                      ali_stream_t stream);
int ali_manifold_err(const float* cf, int64_t ld, int32_t M, int32_t D, const int32_t* owner, const int32_t* cls,
                     const double* S, const double* Q, const double* TS, const double* TQ, const int32_t* cnt,
                     const int32_t* tcnt, int32_t O, int32_t C, float* out3, void* ws, size_t ws_bytes,
                     ali_stream_t stream);

/* The morphomnist family (morphomnist/morpho.py: ImageMorphology, ImageMoments, and extract_observed_attributes of
 * mnist_gan_measured_cf.py / mnist_vae_measured_cf.py) for a batch; csrc/morpho.hip.  One workgroup per image in every
 * kernel; integers and fixed-order fp64 sums: the same inputs give the same bits on every run.  No allocation, no host
 * read, no synchronisation.  Limit: H * scale <= 512 and W * scale <= 512 (ALI_ERR_BAD_ARG above it).  Bitmaps are
 * [B][H * scale][wpr] uint32 words, wpr = ceil(W * scale / 32), pixel x of a row at bit x & 31 of word x >> 5; the bits
 * of a row's last word beyond the image are written as 0 and ignored when read.  Every workspace is the caller's: the
 * scratch lies behind the ALI_WS_RESERVED head, which these kernels neither read nor write.
 *
 * ali_morpho_binarise: x [B] images of H x W fp32, image b at b * ld (ld >= H * W), rows contiguous.  scale > 1:
 *   hires = 255 * AH x AWt with AH [H * scale][H], AW [W * scale][W] fp32 DEVICE row-major (the 1-D expand operator of
 *   the statement, rounded from fp64 by the caller), all products in fp32 with fmaf, taken of x less its minimum (the
 *   minimum's plate, 255 * min, is added back to min, max and the sums in fp64: the operators' rows sum to 1);
 *   scale == 1: hires = x and AH, AW are not read.  hires is never stored.  hstats [B][8] double = { min, max, sum v, sum x v, sum y v, sum x^2 v,
 *   sum x y v, sum y^2 v } of hires (x the column, y the row; fp64 sums of the fp32 pixels); bin = hires >= min +
 *   (max - min) * threshold (fp32), and all ones for a constant x (whose hires is constant but for rounding); fg [B] =
 *   the number of set pixels.  ws >= ALI_WS_RESERVED + 4 * B * H * W * scale
 *   bytes when scale > 1.
 * ali_morpho_edt: d2 [B][Hh][Wh] int32 = the exact squared Euclidean distance of every pixel to the nearest 0 pixel of
 *   its image (0 on the background; the border is not background: scipy.ndimage.distance_transform_edt).  status [B]
 *   = 0, or 1 for an image without a 0 pixel, whose d2 is left unwritten.  ws >= ALI_WS_RESERVED + 2 * B * Hh * Wh.
 * ali_morpho_thin: the ordered thinning of the statement.  Every set pixel has the key (d2, corner, tiebreak, linear
 *   index y * Wh + x), corner = 9 - the number of set pixels of its 3 x 3 neighbourhood in bin (zero padded), tiebreak =
 *   hi24 of hash (linear index) under the "thin" key of seed (csrc/ali_rng.h; no counter); the pixels are visited in
 *   ascending key order and each is set to bit (its current neighbourhood) of keep16, a HOST table of 512 bits (bit
 *   3 * r + c of the index is the pixel at row r, column c of the neighbourhood, the centre is bit 4).  The kernel
 *   decides a pixel as soon as all its neighbours with smaller keys are decided, which gives the sequential result
 *   exactly.  fg [B]: the set pixels of bin, the cap of the round loop; an image whose loop ends with undecided pixels
 *   gets status 2 (it cannot happen with consistent inputs).  Images with status != 0 on entry get an empty skeleton.
 *   skel: a bitmap like bin.  ws >= ALI_WS_RESERVED + B * Hh * Wh bytes.  LDS: 8 * Hh * wpr bytes (at most 64 KB).
 * ali_morpho_measure: counts [B][4] int32 = { fg, skeleton pixels, straight pairs (right, below), diagonal pairs
 *   (below-left, below-right) }; values [B][5] fp32 = { area = fg / scale^2, length = (straight + sqrt 2 * diagonal) /
 *   scale, thickness = 2 * mean of sqrt(d2) over the skeleton / scale, intensity, shear }; slant_hires [B] =
 *   atan(shear of hires).  intensity = the median (the mean of the two middle values for an even count, formed in
 *   fp64) of the pixels of x that are >= min + (max - min) / 2 (compared in fp64), in the units of x; shear =
 *   -u11 / u02 of the central moments of (image - its minimum), which a positive affine map of the pixel values leaves
 *   unchanged and which is the moment ratio of the image itself when its background is 0; the minimum's plate is taken
 *   out of the raw fp64 sums in closed form.  Each is evaluated in fp64 and rounded once.  status != 0 gives NaN
 *   for area, length and thickness, an empty skeleton NaN for thickness, a constant image NaN for both shears. */
int ali_morpho_binarise(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t scale, const float* AH,
                        const float* AW, float threshold, uint32_t* bin, int32_t* fg, double* hstats, void* ws,
                        size_t ws_bytes, ali_stream_t stream);
int ali_morpho_edt(const uint32_t* bin, int32_t B, int32_t Hh, int32_t Wh, int32_t* d2, int32_t* status, void* ws,
                   size_t ws_bytes, ali_stream_t stream);
int ali_morpho_thin(const uint32_t* bin, const int32_t* d2, const int32_t* fg, int32_t B, int32_t Hh, int32_t Wh,
                    uint64_t seed, const uint32_t* keep16, uint32_t* skel, int32_t* status, void* ws, size_t ws_bytes,
                    ali_stream_t stream);
int ali_morpho_measure(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t scale, const uint32_t* skel,
                       const int32_t* d2, const int32_t* fg, const double* hstats, const int32_t* status,
                       int32_t* counts, float* values, float* slant_hires, ali_stream_t stream);

/* The perturbation half of the family (morphomnist/perturb.py: SetThickness, SetSlant, ImageMorphology.downscale,
 * SetIntensity -- the ground-truth counterfactual image of mnist_vae_measured_cf.py and the data-set builders), on the
 * bitmaps and measures the four kernels above leave on the device.  Same layout, limits and workspace convention; one
 * workgroup per image, integers and fixed-order fp64 sums, no atomics: the same inputs give the same bits on every run.
 * Status values: 0; 1 and 2 as above; 3: the radius exceeds max_radius; 4: nothing left to work with (NaN thickness,
 * no pixel left, every pixel in one row so that u02 == 0, or a quantised image that is 0 everywhere).  An image with a
 * status != 0 passes through every later kernel as zeros, and keeps its status.
 *
 * ali_morpho_reshape: thickness: the measured thickness of image b at thickness[b * thickness_ld] (fp32, as
 *   ali_morpho_measure wrote it: values + 2 with thickness_ld = 5); target [B] fp32 or NULL (radius 0).  delta =
 *   (double)target - (double)thickness; radius = (int)min(scale * |delta| / 2, 2^30) in fp64, formed on the device;
 *   radius[b] carries the sign of delta (written as 0 unless the status is 0 or 3).  half: DEVICE int16
 *   [max_radius + 1][2 * max_radius + 1], row r = the half widths of the 2 r + 1 rows of the footprint of radius r
 *   (every row one centred run of 2 h + 1 pixels); max_radius <= 64.  delta >= 0: out(y, x) = any pixel of bin within
 *   the footprint around (y, x), outside the image being background; delta < 0: the same of the complement inside the
 *   image, complemented (outside the image does not constrain the erosion).  Exact: the distance along the row to the
 *   nearest set pixel goes to the workspace as uint16 and out(y, x) = any_dy hd(y + dy, x) <= half[dy].  sums [B][6]
 *   int64 = { count, sum x, sum y, sum x^2, sum x y, sum y^2 } of out.  status_out = status_in, else 4 / 3 as above
 *   (out and sums are then 0).  ws >= ALI_WS_RESERVED + 2 * B * Hh * Wh bytes.  LDS: 4 * 512 * 16 bytes.
 * ali_morpho_shear_reduce: shear = u11 / u02 and cy = sum y / count from sums, in fp64 with every operation rounded on
 *   its own; delta = target_shear[b] - shear (target_shear [B] fp64 = -tan(slant), or NULL: delta = 0); row y of bin is
 *   read at column x + shift(y), shift(y) = floor(0.5 - delta * (y - cy)) held to -Wh .. Wh, 0 outside the image (the
 *   shifts equal numpy's fp64 bit for bit).  T = warped RWt (fp64 sums over a row's set pixels in ascending x) goes to
 *   the workspace, raw = 255 * RH T (fp64 sums in ascending y, rounded to fp32 once), q = floor(clip(raw, 0, 255) +
 *   2^-7) in fp32.  RH [H][H * scale], RW [W][W * scale] DOUBLE, DEVICE row-major: the 1-D reduce operator of the
 *   statement as it is (its rows have lobes of both signs; rounded to fp32 they would leave, where the lobes cancel,
 *   the whole error of an fp32 product); scale == 1: they are not read and raw = 255 * warped.  q [B][H][W]; raw
 *   [B][H][W] and shifts [B][H * scale] int32 are written when non-NULL; shear [B] fp64 (NaN with a status).  ws >=
 *   ALI_WS_RESERVED + 8 * B * H * scale * W bytes when scale > 1.  LDS: 4 * 512 * 16 + 4 * 512 bytes.
 * ali_morpho_set_intensity (a third launch: it is testable alone and takes any image, not only shear_reduce's): q [B][N]
 *   fp32; median [B] = the median of the pixels of q that are >= min + (max - min) / 2, as ali_morpho_measure forms it;
 *   out = clip(q * (target[b] / median), 0, 255), factor and product in fp32; target NULL: out = q.  An image whose
 *   maximum is not above 0 gets status 4; with a status out is 0 and median NaN.  out must not overlap q (the median
 *   is selected from q while other threads write out), nor may any output of the three overlap one of its inputs. */
int ali_morpho_reshape(const uint32_t* bin, const float* thickness, int64_t thickness_ld, const float* target,
                       const int32_t* status_in, const int16_t* half, int32_t max_radius, int32_t B, int32_t Hh,
                       int32_t Wh, int32_t scale, uint32_t* out, int32_t* radius, int64_t* sums, int32_t* status_out,
                       void* ws, size_t ws_bytes, ali_stream_t stream);
int ali_morpho_shear_reduce(const uint32_t* bin, const int64_t* sums, const double* target_shear, const int32_t* status,
                            int32_t B, int32_t H, int32_t W, int32_t scale, const double* RH, const double* RW,
                            float* q, float* raw, int32_t* shifts, double* shear, void* ws, size_t ws_bytes,
                            ali_stream_t stream);
int ali_morpho_set_intensity(const float* q, const float* target, const int32_t* status_in, int32_t B, int32_t N,
                             float* out, float* median, int32_t* status_out, ali_stream_t stream);

/* The Morpho-MNIST local perturbations (morphomnist/skeleton.py: LocationSampler, direction; morphomnist/perturb.py:
 * Thinning, Thickening, Swelling, Fracture, local_image -- the plain / thin / thick / swelling / fractures data sets),
 * on the bitmaps, distance maps and skeletons of the measurement kernels.  Same layout and limits; one workgroup per
 * image; integers, integer LDS atomics (atomicAnd: order-free) and fp64 with every operation rounded on its own: the
 * same inputs give the same bits on every run, and the integers are the statement's.  kind [B] int32: 0 plain, 1 thin,
 * 2 thick, 3 swell, 4 fracture; another value gives status 4.  An image with a status != 0 passes through as zeros.
 *
 * ali_morpho_locate: skel and d2 as ali_morpho_thin / ali_morpho_edt wrote them.  Kinds 0 .. 2 and images with a status
 *   draw nothing (n_candidates 0).  Kind 3 draws 1 location from the whole skeleton.  Kind 4 draws `num` (1 .. 8)
 *   from the skeleton less the disks of radius r_tips around its pixels with exactly 1 neighbour (8-connected, zero
 *   padded), then less the disks of radius r_forks around the pixels with exactly 3 neighbours of what is left (a
 *   radius < 0: that erase is skipped; |p - q|^2 <= r^2, radius 0 clears the seeds alone); if nothing is left the
 *   whole skeleton is used and fallback[b] = 1.  n_candidates[b]: the pixels drawn from.  Draw k is the ((hi24 *
 *   n_candidates) >> 24)-th of them in row-major order, hi24 of hash (offset + b) * 8 + k under the "locate" key of
 *   (seed, *dev_counter) (csrc/ali_rng.h); `offset` counts the images in front of image 0, so a call split into row
 *   ranges draws what the whole call draws.  centres [B][8][2] int32 = (row, column), -1 where unused.  For kind 4,
 *   endpoints [B][8][4] = (r0, c0, r1, c1), 0 where unused: with (n, sx, sy, sxx, sxy, syy) the integer sums of the
 *   skeleton inside the (4 scale + 1)^2 window around the centre (window coordinates, outside the image 0), a = n sxx -
 *   sx^2 - (n syy - sy^2), b = 2 (n sxy - sx sy), h = sqrt(a a + b b), cos = sqrt((1 + a / h) / 2), sin =
 *   copysign(sqrt((1 - a / h) / 2), b) ((1, 0) when h == 0), L = sqrt(d2[centre]) + scale / 2, p0 = trunc(centre +
 *   L (cos, -sin)), p1 = trunc(centre - L (cos, -sin)).  LDS: 8 * Hh * ceil(Wh / 32) + 2.2 KB.
 * ali_morpho_local: thickness as ali_morpho_reshape takes it.  By kind: 0 the bitmap; 1 d2 > r^2, r = (int)min(thin_amount
 *   * scale * thickness / 2, 2^15) in fp64; 2 !(d2c > r^2) with thick_amount, d2c the distance map of the complement
 *   bitmap (ali_morpho_edt of ~bin with pad bits 0; NULL says no image is of kind 2: one that is gets status 4); 3 the
 *   radial warp around centre 0: output (y, x) reads row floor(cy + w dy + 0.5) and column floor(cx + w dx + 0.5), w =
 *   (dd / R^2) ** ((swell_strength - 1) / 2) where dd = dx^2 + dy^2 <= R^2 (no pow when the exponent is 1) and 1
 *   beyond, R = (swell_radius * sqrt(thickness) / 2) * scale, 0 outside the image; 4 the bitmap less every pixel within
 *   frac_radius of a pixel t = 0 .. m of the lines p0 -> p1 of the first num_frac end points, m = max(|dr|, |dc|), the
 *   major coordinate moving by t and the minor by (2 t |dminor| + m) / (2 m) in integers; line pixels outside the image
 *   count.  radius[b]: r, min(R, 2^15) truncated, or frac_radius.  Status 4: NaN thickness (kinds 1 .. 3), no candidate
 *   (kinds 3, 4), or an empty result.  out has pad bits 0; sums [B][6] int64 are its moment sums (count, x, y, xx, xy,
 *   yy), what ali_morpho_shear_reduce with target_shear NULL takes to form the low-resolution image.  frac_radius <=
 *   1024.  LDS: 32 KB. */
int ali_morpho_locate(const uint32_t* skel, const int32_t* d2, const int32_t* status, const int32_t* kind, int32_t B,
                      int32_t Hh, int32_t Wh, int32_t scale, int32_t r_tips, int32_t r_forks, int32_t num, uint64_t seed,
                      const int64_t* dev_counter, uint64_t offset, int32_t* n_candidates, int32_t* fallback,
                      int32_t* centres, int32_t* endpoints, ali_stream_t stream);
int ali_morpho_local(const uint32_t* bin, const int32_t* d2, const int32_t* d2c, const float* thickness,
                     int64_t thickness_ld, const int32_t* status_in, const int32_t* kind, const int32_t* n_candidates,
                     const int32_t* centres, const int32_t* endpoints, double thin_amount, double thick_amount,
                     double swell_strength, double swell_radius, int32_t frac_radius, int32_t num_frac, int32_t B,
                     int32_t Hh, int32_t Wh, int32_t scale, uint32_t* out, int32_t* radius, int64_t* sums,
                     int32_t* status_out, ali_stream_t stream);

/* The bounding parallelogram of Morpho-MNIST's measure_image (morphomnist/morpho.py: bounds_of, quantile_loc): x, ld, B,
 * H, W, scale, AH, AW as ali_morpho_binarise takes them; hires = expand(x - min x), formed as ali_morpho_binarise forms it
 * (fp32 fmaf, never stored).  bounds [B][6] fp64 = left, right, top, bottom, shear, middle in up-sampled pixels: shear =
 * u11 / u02 and middle = m01 of hires in fp64 (every operation rounded on its own); hcdf[t] = sum over rows y of the fp64
 * prefix of row y up to #{x : x + .5 < t + shear * (y - middle)}, over m00; vcdf[t] = the rows above t over m00; left /
 * top = the first crossing of bound_frac / 2, right / bottom = the last crossing of 1 - bound_frac / 2, interpolated with
 * np.interp's formula (0 below the first entry, n - 1 at or above the last).  The four locations are NaN when m00 <= 0
 * or the shear is not finite.  hcdf [B][W * scale] and vcdf [B][H * scale] fp64 are written when non-NULL.  0 <
 * bound_frac < 1.  ws >= ALI_WS_RESERVED + 4 * B * H * W * scale bytes when scale > 1 and H * W * scale > 28 * 448 (T
 * is kept in LDS up to that size), else none.  LDS: 58.5 KB.  One workgroup per image, no atomics, fixed-order sums. */
int ali_morpho_bounds(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t scale, const float* AH,
                      const float* AW, double bound_frac, double* bounds, double* hcdf, double* vcdf, void* ws,
                      size_t ws_bytes, ali_stream_t stream);

/* SetWidth of Morpho-MNIST (morphomnist/perturb.py: width_stage, width_columns, affine_stage): the width of the bounding
 * parallelogram measured on the grey up-sampled image under the BITMAP's shear and centroid row, then the horizontal
 * scaling about the bitmap's centroid that brings that width to the target and keeps the shear, then downscale.  One
 * workgroup per image, no atomics, integers and fixed-order fp64 sums, every fp64 operation of the statement rounded on
 * its own: the same inputs give the same bits on every run.  Status values: 0; 1: the bitmap has no background (fg[b] ==
 * Hh * Wh); 5: target[b] is NaN, infinite or <= 0; 4: the bitmap is empty or every set pixel lies in one row, the grey
 * mass is <= 0, the width is not finite or <= 0, or the quantised image is 0 everywhere -- decided in this order.  An
 * image with a status != 0 passes through as zeros.
 *
 * ali_morpho_width: x, ld, B, H, W, scale, AH, AW as ali_morpho_binarise takes them; bin, fg: what it wrote for the same
 *   x.  sums [B][6] int64 = { count, sum x, sum y, sum x^2, sum x y, sum y^2 } of bin.  wb [B][6] fp64 = left, right,
 *   shear, cx, cy, factor: shear = u11 / u02, cx = sum x / count, cy = sum y / count of the sums, as
 *   ali_morpho_shear_reduce forms them; left, right = the first crossing of bound_frac / 2 and the last crossing of 1 -
 *   bound_frac / 2 of hcdf[t] = sum over rows y of the fp64 prefix of row y of hires up to #{x : x + .5 < t + shear * (y -
 *   cy)}, over m00 -- pass 2 of ali_morpho_bounds (the same fp32 fmaf chains for hires = expand(x - min x), the same
 *   prefixes, comparison and interpolation) under the bitmap's moments; m00 = the rows' totals added in ascending y;
 *   factor = ((right - left) / scale) / target[b].  target [B] fp64.  With a status sums are 0 and wb NaN.  hcdf [B][W *
 *   scale] fp64 is written when non-NULL (0 with a status).  0 < bound_frac < 1.  ws as ali_morpho_bounds: >=
 *   ALI_WS_RESERVED + 4 * B * H * W * scale bytes when scale > 1 and H * W * scale > 28 * 448, else none.  LDS: 54.4 KB.
 * ali_morpho_affine_reduce: bin, sums, wb, status as ali_morpho_width left them: shear, cx and cy are formed from sums
 *   again (the same bits as wb's), factor is wb[b][5].  Output pixel (y, x) of the warped bitmap reads bit c of row y of bin, c =
 *   floor(((cx + factor * (x - cx)) + (shear * (1 - factor)) * (y - cy)) + 0.5) held to -1 .. Wh in fp64 (a NaN: -1),
 *   each operation rounded on its own in the order morphomnist/perturb.py: width_columns fixes; 0 outside the image: the
 *   columns equal numpy's bit for bit.  Then T, raw and q exactly as ali_morpho_shear_reduce forms them (RH, RW, ws and
 *   the scale == 1 short cut as there).  q [B][H][W]; raw [B][H][W] and warped [B][H * scale][ceil(W * scale / 32)] (pad
 *   bits 0) are written when non-NULL.  status_out [B] = status, or 4 when q is 0 everywhere.  LDS: 4 * 512 * 16 bytes. */
int ali_morpho_width(const float* x, int64_t ld, int32_t B, int32_t H, int32_t W, int32_t scale, const float* AH,
                     const float* AW, const uint32_t* bin, const int32_t* fg, double bound_frac, const double* target,
                     int64_t* sums, double* wb, int32_t* status, double* hcdf, void* ws, size_t ws_bytes,
                     ali_stream_t stream);
int ali_morpho_affine_reduce(const uint32_t* bin, const int64_t* sums, const double* wb, const int32_t* status, int32_t B,
                             int32_t H, int32_t W, int32_t scale, const double* RH, const double* RW, float* q,
                             float* raw, uint32_t* warped, int32_t* status_out, void* ws, size_t ws_bytes,
                             ali_stream_t stream);

/* Attribute plumbing of one batch (mnist.py:47-55, audio_mnist.py:203-210, whalecalls.py:455): idx[b*n_cat + j] =
 * argmax of categorical attribute j (one-hot rows of n_classes[j] floats, or int32 when cat_is_int[j]; first maximum
 * like torch.argmax); cont[b*n_cont + j] = cont_in[j][b]. */
int ali_attr_pack(const void* const* cat, const int32_t* n_classes, const int32_t* cat_is_int, int32_t n_cat,
                  const float* const* cont_in, int32_t n_cont, int32_t B, int32_t* idx, float* cont, ali_stream_t stream);

/* Device-side input pipeline (opt-in: mnist.train(input_pipeline="device"), train_on_stream(z_source="device")).
 *
 * ali_normal_fill: out[i] ~ N(0,1), i < n, from the counter RNG of ali_dropout_mask under a key of its own (seed,
 * *dev_counter and a latent-stream constant; dev_counter may be NULL).  Element g = offset + i is the cosine (g even)
 * or sine (g odd) half of the Box-Muller pair of hash g >> 1, u1 in (0,1] and u2 in [0,1) being disjoint 24-bit
 * fields of that hash: a value depends on (seed, counter, g) alone, so a buffer filled by one launch equals the same
 * buffer filled piecewise, whatever the split or the alignment of out (4-byte aligned; 16-byte stores inside).
 * ali_hip.source.normal_reference is the recipe in fp64.
 *
 * ali_batch_gather: one training batch from a data set resident in device memory, rows index[b] (device int64) of
 * images [N][HW] (uint8 if images_u8, else fp32) and attrs [N][attr_ld] fp32 = [one-hot (n_cls) | continuous (n_cont)]:
 *   out_images[b][:]  = 2*x/255 - 1 (mnist.py:204; the division as torch's device kernel performs it: times the fp32
 *                       reciprocal of the scalar)
 *   out_onehot[b][:]  = the one-hot row;  out_idx[b] = its first maximum (torch.argmax)
 *   out_cont[b][j]    = 2*(a - lo[j])/(hi[j] - lo[j]) - 1 (mnist.py:206, IEEE division, nothing contracted)
 * -- bit for bit what image_scms.mnist._scale_batch + MnistFamily.conditioning hand the stepper.  An index outside
 * [0, N) reads nothing and yields NaN. */
int ali_normal_fill(uint64_t seed, const int64_t* dev_counter, uint64_t offset, float* out, int64_t n,
                    ali_stream_t stream);
int ali_batch_gather(const void* images, int32_t images_u8, const float* attrs, int32_t attr_ld, const int64_t* index,
                     const float* lo, const float* hi, int64_t N, int32_t HW, int32_t n_cls, int32_t n_cont, int32_t B,
                     float* out_images, float* out_onehot, int32_t* out_idx, float* out_cont, ali_stream_t stream);

/* Generator input (mnist.py:76-85; audio_mnist.py:250-256): out[b*ld + :] = [ z[b, :zdim] | onehot_j[b] @ tables[j]
 * ([n_classes[j]][256]) for j < n_emb | cont[b, :n_cont] | zeros ] -- a true sum over classes (soft attributes), the
 * zero padding brings the row to the GEMM's channel stride.  ali_g_input_table_grad: the gradient of one table,
 * out[n][k] = sum_b onehot[b][n] * g[b*ld + off + k] (samples in order, no atomics). */
int ali_g_input(const float* z, int32_t zdim, const void* const* onehot, const int32_t* n_classes,
                const int32_t* onehot_is_int, const float* const* tables, int32_t n_emb, const float* cont, int32_t n_cont,
                int32_t B, int32_t ld, float* out, ali_stream_t stream);
int ali_g_input_table_grad(const void* onehot, int32_t onehot_is_int, int32_t n_classes, const float* g, int32_t ld,
                           int32_t off, int32_t B, float* out, ali_stream_t stream);

/* Conditioning-plane assembly (mnist.py:24-29,46-55; audio_mnist.py:178-209):
 * out[b,h,w,0] = X[b,h,w]; out[..,1+j] = tanh(emb_j[idx_j[b]][src(h,w)]) for the
 * n_emb categorical planes (16x16 tables, nearest up-sampling, src = floor(dst*16/H));
 * then n_cont broadcast scalars cont[b,j]; remaining channels up to Cpad = 0. */
int ali_assemble_planes(const float* X, const int32_t* idx, const float* const* emb_tables, int32_t n_emb,
                        const float* cont, int32_t n_cont, float* out, int32_t B, int32_t H, int32_t W,
                        int32_t Cpad, const float* mask /* optional [B][mask_ld]: out[b,..,c] *= mask[b][c], the
                        Dropout2d in front of the consuming conv (mnist.py:118) */, int32_t mask_ld, ali_stream_t stream);

/* Backward of ali_assemble_planes for one embedding table (mnist.py:17-18,46-55 and copies: Embedding -> 16x16 ->
 * nearest Upsample -> Tanh):  out[n][cell] = sum over samples b with idx[b*idx_ld + idx_col] == n and over the pixels
 * (h,w) that the up-sampling maps to cell (floor(h*16/H)*16 + floor(w*16/W)) of
 *   g[((b*H+h)*W+w)*g_ld + g_ch] * (1 - x[((b*H+h)*W+w)*x_ld + x_ch]^2)        (tanh' from the stored plane).
 * Fixed summation order (no atomics).  out is [n_rows][256]. */
int ali_plane_table_grad(const float* g, int32_t g_ld, int32_t g_ch, const float* x, int32_t x_ld, int32_t x_ch,
                         const int32_t* idx, int32_t idx_ld, int32_t idx_col, int32_t B, int32_t H, int32_t W,
                         int32_t n_rows, float* out,
                         const float* table /* optional [n_rows][256]: take the plane value tanh(table[n][cell]) from
                         the table instead of x (x may then be NULL): the stored planes may carry a Dropout2d mask */,
                         ali_stream_t stream);

/* Gather half of a strided transposed convolution in scatter form (ConvTranspose2d forward with one or two output
 * channels -- audio_mnist.py:281, whalecalls.py / esrf_acoustic.py Generator tails -- and the few input planes of a
 * first Conv2d's data gradient that are consumed, audio_mnist.py:203-210): a 1x1 GEMM (ali_conv_fwd) first produces,
 * for every pixel (b,h,w) of the H x W map, the contribution contrib[(b,h,w)*ldc + (r*S+s)*NC + c] of that pixel to
 * output channel c through tap (r,s); this sums, per output pixel, the taps whose source position exists:
 *   out[((b*Hout+oy)*Wout+ox)*ostride + c] = act(bias[c] + sum_{r,s} contrib[b,(oy+pad-r)/stride,(ox+pad-s)/stride,c,r,s])
 * over the (r,s) for which both quotients are exact and inside the map.  NC <= 8. */
int ali_col2im(const float* contrib, int32_t ldc, const float* bias, float* out, int32_t B, int32_t H, int32_t W,
               int32_t Hout, int32_t Wout, int32_t NC, int32_t ostride, int32_t R, int32_t S, int32_t stride,
               int32_t pad, int32_t act, float slope, ali_stream_t stream);
/* The two halves above in ONE launch, for 64-channel maps and at most two output channels (what the spectrogram stacks
 * have at their one-channel ends): x [B,H,W,64] times the tap matrix w_nc [NC*R*S][64] (row (r*S+s)*NC + c, the layout
 * the 1x1 GEMM takes) on the matrix cores in exact fp32, contributions kept in LDS per output tile, then the sum and
 * epilogue of ali_col2im -- the [pixels][taps] tensor is never written.  ali_tconv_scatter_ok tells whether a shape is
 * served (otherwise: ali_conv_fwd + ali_col2im). */
int32_t ali_tconv_scatter_ok(int32_t C, int32_t NC, int32_t R, int32_t S, int32_t stride);
int ali_tconv_scatter(const float* x, const float* w_nc, const float* bias, float* out, int32_t B, int32_t H, int32_t W,
                      int32_t C, int32_t Hout, int32_t Wout, int32_t NC, int32_t ostride, int32_t R, int32_t S,
                      int32_t stride, int32_t pad, int32_t act, float slope, ali_stream_t stream);

/* Weight gradient of that transposed convolution for ONE output channel: dw[k*s_k + (r*S+s)*s_tap] = sum_{b,p,q}
 * big[b,p,q,k] * small[(b, p*stride - pad + r, q*stride - pad + s) * sstride], big = its 64-channel input [B,P,Q,64], small
 * = the gradient of its [B,H,W] output (element stride sstride).  One launch + a slab fold; ali_tconv_scatter_wgrad_ws
 * returns the workspace bytes it needs, 0 when the shape is not served (then: ali_conv_bwd_weight). */
int64_t ali_tconv_scatter_wgrad_ws(int32_t B, int32_t P, int32_t Q, int32_t K, int32_t R, int32_t S, int32_t stride);
int ali_tconv_scatter_wgrad(const float* big, const float* small, int32_t sstride, float* dw, int64_t s_k, int64_t s_tap,
                            int32_t B, int32_t P, int32_t Q, int32_t K, int32_t H, int32_t W, int32_t R, int32_t S,
                            int32_t stride, int32_t pad, void* ws, size_t ws_bytes, ali_stream_t stream);
/* The launch plan of the two entry points above for a shape: the launch, ali_tconv_scatter_wgrad_ws and this query read
 * one plan each.  `op` is an ALI_TS_OP_*; the arguments are those of ali_tconv_scatter -- for ALI_TS_OP_WGRAD: B, H, W, C
 * = the 64-channel map (the launch's B, P, Q, K), Hout x Wout = the one-channel map, NC = 1, ostride = its sstride.
 * Fills plan[0..5] and returns ALI_OK, or returns the error code with which the launch would refuse the shape
 * (ali_last_error says why; a workspace that is too small is the launch's own refusal: compare plan[5]):
 *   ALI_TS_OP_FWD   : NT (tconv_scatter_kernel<NT>), OBH, OBW (output tile of a block), LDS bytes, blocks, 0
 *   ALI_TS_OP_WGRAD : NT (tconvs_wgrad_mfma_kernel<NT, 4>), RB (rows of a band), bands per image, LDS bytes, blocks,
 *                     workspace bytes (= ali_tconv_scatter_wgrad_ws)
 * Host arithmetic only: works without a GPU.  It reads ALI_NO_T1_MFMA like the launches do.  Every plan a shape can
 * reach -- 19 forward, 8 weight-gradient -- and every template of ali_col2im is held to an fp64 reference by
 * tests/test_gpu_scatter_routes.py. */
#define ALI_TS_OP_FWD 0
#define ALI_TS_OP_WGRAD 1
int32_t ali_tconv_scatter_plan(int32_t op, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Hout, int32_t Wout,
                               int32_t NC, int32_t ostride, int32_t R, int32_t S, int32_t stride, int32_t pad,
                               int64_t* plan);

/* Tail of the spectrogram front-end (the step in front of the path): torchaudio.transforms.Spectrogram
 * (power 2) + (. + 1e-6).log() and, optionally, spect_to_img (audio_mnist.py:116,347-363 and copies).  `y` holds, per
 * frame (b,t), the windowed DFT as produced by a 1x1 ali_conv_fwd with the [2F x win] cos|sin matrix: re[f] = y[f],
 * im[f] = y[F+f].  out[b,f,t] = log(re^2 + im^2 + 1e-6); with mean/std (per last-dim index t, as the reference
 * computes them): clip((. - mean[t]) / (std[t] + 1e-6), -k, k) / k. */
int ali_spect_post(const float* y, int32_t B, int32_t T, int32_t F, const float* mean, const float* std, float clip_k,
                   float* out, ali_stream_t stream);

/* SSIM of image pairs and its gradient (the --metric ssim loss of the encoder fine-tuning scripts,
 * finetune_mnist_bigan.py:75-76; definition: pytorch_msssim.ssim).  X, Y are `planes` = B*C contiguous H x W planes,
 * `win` the win_size taps g of the 1-D window on the device (win_size odd, <= ALI_SSIM_MAX_WIN, <= H, W).  With F the
 * separable valid correlation with g along H and W (map Hm x Wm = (H-win_size+1) x (W-win_size+1)):
 *   mu1 = F(X), mu2 = F(Y), s1 = F(X*X) - mu1^2, s2 = F(Y*Y) - mu2^2, s12 = F(X*Y) - mu1*mu2,
 *   cs = (2*s12 + C2) / (s1 + s2 + C2),  S = (2*mu1*mu2 + C1) / (mu1^2 + mu2^2 + C1) * cs,
 *   ssim_pc[plane] = mean over the map of S.
 * mA/mB/mC (all three or none), each [planes][Hm][Wm], receive A = dS/dF(Y), Bq = dS/dF(Y*Y), Cq = dS/dF(X*Y).
 * Planes larger than one 32x32 map tile put planes*tiles partial sums into the workspace (fixed-order fold). */
#define ALI_SSIM_MAX_WIN 25
int ali_ssim_fwd(const float* X, const float* Y, int64_t planes, int32_t H, int32_t W, const float* win,
                 int32_t win_size, float C1, float C2, float* ssim_pc, float* mA, float* mB, float* mC, void* ws,
                 size_t ws_bytes, ali_stream_t stream);
/* dY[plane][p] = gpc[plane] / (Hm*Wm) * (Ft(A)[p] + 2*Y[p]*Ft(Bq)[p] + X[p]*Ft(Cq)[p]), Ft the transposed (full)
 * filter and gpc[planes] the incoming gradient of ssim_pc on the device.  The metric is symmetric: the gradient
 * w.r.t. X is the same pair of calls with X and Y exchanged. */
int ali_ssim_bwd(const float* X, const float* Y, const float* mA, const float* mB, const float* mC, const float* gpc,
                 int64_t planes, int32_t H, int32_t W, const float* win, int32_t win_size, float* dY,
                 ali_stream_t stream);

/* Griffin-Lim phase reconstruction: torchaudio.transforms.GriffinLim as the reference builds it next to every
 * Spectrogram (image_scms/audio_mnist.py:62-64,117; whalecalls.py:56-59; esrf_acoustic.py:40-43) and calls it on
 * img_to_spect(G(...)).exp() (audio_mnist_reconstruction.py:64-67, audiomnist_generate.py:94).  F = n_fft/2 + 1 bins,
 * T frames, left = (n_fft - win)/2, start = n_fft/2.  One iteration is
 *   X [B*T][2F] --inverse DFT GEMM (ali_conv_fwd 1x1, [win x 2F] matrix)--> fr [B][T][win] --ali_gl_ola--> frames
 *   [B][T][win] --forward DFT GEMM ([2F x win] matrix of the spectrogram front-end)--> Y [B*T][2F] --ali_gl_phase--> X.
 *
 * ali_gl_init: src [B][F][T] -> mag [B*T][F] and X [B*T][2F] = (re | im) of angles * mag.  mode says what src is:
 *   ALI_GL_SRC_IMAGE  mag = exp((src * stds_kept * (std[t] + 1e-6) + mean[t]) / power)   (img_to_spect, audio_mnist.py:365-366,
 *                     .exp() and ** (1/power) in one pass; mean / std per last index t)
 *   ALI_GL_SRC_LOG    mag = exp(src / power)        ALI_GL_SRC_SPEC   mag = src ** (1/power)
 * angles = a0_re + i*a0_im ([B][F][T] planes, both or none); else, with rand_init, re and im uniform in [0,1): the two
 * disjoint 24-bit fields (bits 40..63 / 16..39) of hash offset + e, e = (b*F + f)*T + t, of the counter RNG of
 * ali_dropout_mask under a key of its own (seed, *dev_counter -- may be NULL -- and a phase-stream constant): a draw
 * depends on (seed, counter, offset + e) alone (ali_hip.griffinlim.uniform_reference is the host recipe); else 1 + 0i.
 *
 * ali_gl_ola: y[p] = (sum over the frames t that reach p, ascending, of fr[b][t][p - t*hop - left]) * renv[p], renv the
 * reciprocal window envelope 1 / sum_t w^2 over the un-cut signal (n_renv entries, p >= n_renv reads 0): gather form,
 * no atomics, bit-reproducible.  final_wave == 0: out [B][T][win] = the next transform's frames,
 * out[b][t][j] = y[start + reflect(t*hop + left + j - start)], reflect the centre=True / pad_mode="reflect" map of a
 * signal of `length` samples (which must have T frames); final_wave != 0: out [B][length] = y[start + i], zero behind
 * the signal's end (torch.istft(length=)), and *advance (optional device counter) += 1.  A block owns frames_per_block
 * consecutive frames of one clip (0: chosen so that its staged rows fit 48 KiB of LDS).
 *
 * ali_gl_phase: per bin of the `rows` x F spectra Y / tprev / X ([rows][2F], re | im) and mag ([rows][F]):
 *   a = Y - m*tprev (tprev NULL or m == 0: a = Y), X = a * (1 / (|a| + 1e-16)) * mag; a == 0 gives 0, nothing gives NaN.
 *
 * ali_gl_check (host only): 1 when the window envelope exceeds 1e-11 over the kept range [start, start + length)
 * (length <= 0: to the signal's end less start) -- the condition torch.istft checks --, 0 when it does not, ALI_ERR_BAD_ARG
 * unless 0 < hop <= win <= n_fft. */
typedef enum { ALI_GL_SRC_IMAGE = 0, ALI_GL_SRC_LOG = 1, ALI_GL_SRC_SPEC = 2 } AliGlSource;
int ali_gl_init(const float* src, int32_t B, int32_t F, int32_t T, int32_t mode, const float* mean, const float* std,
                float stds_kept, float power, const float* a0_re, const float* a0_im, int32_t rand_init, uint64_t seed,
                const int64_t* dev_counter, uint64_t offset, float* mag, float* X, ali_stream_t stream);
int ali_gl_ola(const float* fr, const float* renv, int32_t n_renv, int32_t B, int32_t T, int32_t n_fft, int32_t win,
               int32_t hop, int64_t length, int32_t final_wave, float* out, int32_t frames_per_block, int64_t* advance,
               ali_stream_t stream);
int ali_gl_phase(const float* Y, const float* tprev, const float* mag, float m, int64_t rows, int32_t F, float* X,
                 ali_stream_t stream);
int32_t ali_gl_check(int32_t n_fft, int32_t win, int32_t hop, int32_t T, int64_t length);

const char* ali_last_error(void);
/* The Discriminator's one-output head, Conv2d(C, 1, 1) on a 1x1 map (mnist.py:127), as a GEMV:
 *   ali_head_fwd  : y[b] = bias[0] + sum_c x[b][c] * w[c]            (x rows ld floats apart, C % 4 == 0)
 *   ali_head_wgrad: dw[c] = sum_b g[b] * x[b][c],  db[0] = sum_b g[b] (db optional)                          */
int ali_head_fwd(const float* x, int32_t ld, const float* w, const float* bias, float* y, int32_t B, int32_t C,
                 ali_stream_t stream);
int ali_head_wgrad(const float* x, int32_t ld, const float* g, float* dw, float* db, int32_t B, int32_t C,
                   ali_stream_t stream);
/* The head's backward pass in one launch, bit for bit what ali_conv_bwd_data (one gathered channel, mask and act'
 * epilogue) followed by ali_head_wgrad leave:
 *   g[b][c] = ((gl[b] * w[c]) * mask[b][c]) * act'(y_prev[b][c])      g, y_prev dense [B][C]; mask rows mask_ld apart
 *   dw[c]   = sum_b gl[b] * x[b][c],  db[0] = sum_b gl[b]             x rows ld floats apart
 * mask may be NULL; y_prev is read only when dact != ALI_ACT_NONE; dw == NULL: data gradient only (x, ld, db, ws unused).
 * With dw the row lanes of ali_head_wgrad's sum run as blocks of their own and meet in ws (zero-filled once; 32 C + 32
 * bytes behind the reserved head, whose first ceil(C / 32) counters the launch uses and leaves at 0): the block that
 * arrives last adds them in ali_head_wgrad's order. */
int ali_head_bwd(const float* gl, const float* w, const float* y_prev, int32_t dact, float dslope, const float* mask,
                 int32_t mask_ld, float* g, const float* x, int32_t ld, float* dw, float* db, int32_t B, int32_t C,
                 void* ws, size_t ws_bytes, ali_stream_t stream);
/* n device-to-device copies (dst[i] <- src[i], bytes[i] each; pointers and sizes multiples of 4) in one launch per 8:
 * the per-step refresh of the input buffers a captured HIP graph reads. */
int ali_copy_multi(int32_t n, const void* const* src, void* const* dst, const int64_t* bytes, ali_stream_t stream);
int ali_version(void);
/* Re-read the developer tuning variables (ALI_SPLITK, ALI_NO_ORDER, ...: csrc/ali_common.h) from the environment;
 * they are otherwise read once per process.  Tests and sweeps only. */
void ali_reload_tuning(void);

#ifdef __cplusplus
}
#endif
#endif /* ALI_HIP_H */
