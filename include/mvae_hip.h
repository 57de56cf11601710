/*
 * mvae_hip.h -- C ABI of libmvae_hip.so: the MVAE train-step kernels for MI355X (gfx950).
 *
 * The reference (mhw32/multimodal-vae-public) has no FFI: its hot path is a chain of
 * PyTorch ATen ops dispatched from model.py / train.py.  Each entry point below
 * replaces the ATen op(s) at the cited reference call sites (paths relative to the
 * reference repository root; SURVEY.md section 2.2 is the op inventory K1..K15).
 *
 * Conventions
 *   - every tensor is fp32, contiguous unless a leading dimension is given, NCHW for images;
 *     class labels are int64;
 *   - all pointers are DEVICE pointers borrowed for the duration of the enqueue; the
 *     library never allocates, frees or retains device memory; scratch is passed in
 *     (`ws`, `ws_bytes`; size it with the matching *_ws_bytes query);
 *   - `stream` is a hipStream_t passed as void*; kernels are asynchronous, no host sync;
 *   - return 0 on success, <0 on error (MVAE_ERR_*); no C++ exception crosses the ABI;
 *   - re-entrant: no global mutable state (launch plans are pure functions of the shapes).  The
 *     tuning overrides at the end of this header exist only in the separate -DMVAE_TUNING build
 *     (libmvae_hip_tuning.so, used by tools/gemm_bench.py); libmvae_hip.so does not export them;
 *   - the data-parallel gradient exchange (RCCL over xGMI) is part of the ABI: mvae_comm_* at the end of this
 *     header; RCCL is bound at run time, so the library has no link-time dependency on it.
 */
#ifndef MVAE_HIP_H
#define MVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVAE_OK          0
#define MVAE_ERR_ARG    (-1)   /* bad shape / null pointer / unsupported stride */
#define MVAE_ERR_LAUNCH (-2)   /* hipLaunchKernel reported an error */
#define MVAE_ERR_WS     (-3)   /* workspace too small */
#define MVAE_ERR_COMM   (-4)   /* RCCL not loadable / an RCCL or HIP runtime call of mvae_comm_* failed (mvae_comm_last_error) */

/* flags */
#define MVAE_ACT_SWISH   1     /* fwd: also write swish(out); bwd: multiply by swish'(preact) */
#define MVAE_ACCUMULATE  2     /* add into the destination instead of overwriting it */

#define MVAE_POE_VARIANT_A 0   /* mnist/model.py:156-163, fashionmnist/model.py:175-182 */
#define MVAE_POE_VARIANT_B 1   /* celeba/model.py:200-207, celeba19/model.py:219-226 */
#define MVAE_POE_NO_PRIOR  4   /* OR-ed into `variant`: no built-in N(0,1) prior -- the caller's stack carries every expert,
                                  as when ProductOfExperts.forward is called on a [M,B,D] stack whose row 0 is what
                                  prior_expert returned (mnist/model.py:50-63,156-163,172-185).  REQUIREMENT: every
                                  term's mask must then select at least one of the E experts -- an empty product has
                                  no precision (0/0: NaN mu, inf logvar) and the launch cannot see a device mask; the
                                  Python binding checks host-built masks (kernels._check_no_prior_masks) */
#define MVAE_MAX_EXPERTS  32

typedef void *mvae_stream_t;   /* hipStream_t */

int mvae_abi_version(void);
/* bytes of scratch a GEMM-shaped call below may need for an output of rows_out x cols_out reduced
 * over reduce_len (split reductions, or the repacked weights of a transposed conv: pass
 * rows_out = Cin, cols_out = Cout*16 of the mirrored conv) */
size_t mvae_gemm_ws_bytes(int rows_out, int cols_out, int reduce_len);
/* ------------------------------------------------------------------------------------
 * K1  Linear (nn.Linear forward / backward): mnist/model.py:75-78,95-98,117-119,136-139;
 *     fashionmnist/model.py:84-86,107-109,135-137,155-161; celeba/model.py:89-92,114,
 *     148-154,175-184; celeba19/model.py:115-118,140,176-178,199-205.
 * K5  Swish (x*sigmoid(x), mnist/model.py:166-169) and K7 Dropout(0.1) (celeba/model.py:91)
 *     are fused into the epilogues.
 *
 * fwd : pre[M,N] = x[M,K] . w[N,K]^T + bias[N]         (pre may be NULL when act given)
 *       act[M,N] = swish(pre) * (mask ? mask*mask_scale : 1)   (if act != NULL)
 * dgrad: dx[M,K] (+)= (dy[M,N] . w[N,K]) * (mask ? mask*mask_scale : 1) * swish'(pre_in)
 *        (pre_in = pre-activation that produced this layer's INPUT, NULL for none)
 * wgrad: dw[N,K] (+)= dy^T . x ;  db[N] (+)= sum_m dy   (db may be NULL)
 * ws (mvae_gemm_ws_bytes): scratch for split reductions; NULL disables splitting.
 * ---------------------------------------------------------------------------------- */
int mvae_linear_fwd(const float *x, int ldx, const float *w, const float *bias,
                    float *pre, float *act, int ldy,
                    const float *mask, float mask_scale,
                    int M, int N, int K, void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_linear_dgrad(const float *dy, int lddy, const float *w,
                      float *dx, int lddx,
                      const float *pre_in, const float *mask, float mask_scale,
                      int M, int N, int K, int flags, void *ws, size_t ws_bytes,
                      mvae_stream_t stream);
int mvae_linear_wgrad(const float *dy, int lddy, const float *x, int ldx,
                      float *dw, float *db, int M, int N, int K, int flags,
                      void *ws, size_t ws_bytes, mvae_stream_t stream);

/* Several Linear weight gradients of DIFFERENT shapes in one launch: dw_q[N_q][K_q] (+)= dy_q^T x_q and, where
 * db_q != NULL, db_q[N_q] (+)= column sums of dy_q -- the loss.backward() work of up to
 * MVAE_WGRAD_BATCH_MAX nn.Linear layers (mnist/model.py:75-78,95-104,137-145) that nothing but the optimizer
 * waits for.  Each item: N*K <= 2048 tiles of 32x32, M <= 4096, operands below 4 GiB; distinct dw / db per
 * item (MVAE_ERR_ARG otherwise -- use mvae_linear_wgrad for those).  Same arithmetic as mvae_linear_wgrad's
 * direct path: per output the batch rows are summed in a fixed order (deterministic). */
#define MVAE_WGRAD_BATCH_MAX 16
typedef struct {
    const float *dy; int lddy;      /* [M, N] upstream gradient, row stride lddy */
    const float *x; int ldx;        /* [M, K] layer input, row stride ldx */
    float *dw;                      /* [N, K] contiguous */
    float *db;                      /* [N] or NULL */
    int M, N, K;
    int flags;                      /* MVAE_ACCUMULATE: add to dw / db */
} mvae_wgrad_item;
int mvae_linear_wgrad_batched(const mvae_wgrad_item *items, int n_items, mvae_stream_t stream);

/* The same launch, which also runs optimizer.step() (torch.optim.Adam defaults, mnist/train.py:168,219) on the
 * parameters whose gradients it has just produced: the weight gradients are the last thing loss.backward() computes
 * for a layer and nothing but the optimizer reads them, so the update rides the gradient's epilogue instead of
 * waiting for one arena-wide launch behind the whole backward pass (15 us + a join at the very end of a 296-us
 * MNIST step).  The gradient is still written.  The four arenas are laid out alike: the parameter / moment element
 * of gradient address g is at the same offset from its base as g is from grad_base.  coef2: the step's two
 * bias-correction factors, left there by mvae_adam_prepare earlier on a stream this one is ordered behind.
 * MVAE_ACCUMULATE is refused (the update needs the step's whole gradient; the CALLER guarantees that no other
 * launch of the step adds to these gradients or reads these parameters afterwards).  An item with dy == x == NULL
 * is a finished gradient of K elements at dw (written earlier on this stream, e.g. an Embedding's): it only takes
 * the update.  Same arithmetic, bit for bit, as mvae_linear_wgrad_batched followed by mvae_adam_apply_at. */
typedef struct {
    const float *grad_base;         /* gradient arena */
    float *param_base;              /* parameter arena */
    float *exp_avg_base;            /* first / second moment arenas */
    float *exp_avg_sq_base;
    const float *coef2;             /* device: { lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) } (mvae_adam_prepare) */
    double beta1, beta2, eps;
    float grad_scale;               /* gradients are multiplied by this first (1 / world size; 1 here) */
} mvae_adam_fuse;
int mvae_linear_wgrad_batched_adam(const mvae_wgrad_item *items, int n_items, const mvae_adam_fuse *adam,
                                   mvae_stream_t stream);

/* Grouped forms: G independent Linear problems of ONE shape in one launch.  celeba19 builds 18
 * identical attribute encoders / decoders (celeba19/model.py:29-30, 173-196) and the reference runs
 * them one after another (celeba19/model.py:78-81, 53-54); here operand g of every array is at
 * base + g * <name>_gs floats (the expert's slice of the parameter arena / of a [G, rows, width]
 * activation buffer; any two same-shaped problems qualify: the stride is the pointer difference,
 * modulo 2^64).  No dropout mask.  ws (NULL = never split): G * mvae_gemm_ws_bytes of the single
 * problem is always enough.  Same maths as the single forms. */
int mvae_linear_fwd_grouped(const float *x, int ldx, size_t x_gs, const float *w, size_t w_gs,
                            const float *bias, size_t bias_gs, float *pre, float *act, int ldy,
                            size_t y_gs, int G, int M, int N, int K, void *ws, size_t ws_bytes,
                            mvae_stream_t stream);
int mvae_linear_dgrad_grouped(const float *dy, int lddy, size_t dy_gs, const float *w, size_t w_gs,
                              float *dx, int lddx, size_t dx_gs, const float *pre_in, size_t pre_gs,
                              int G, int M, int N, int K, int flags, void *ws, size_t ws_bytes,
                              mvae_stream_t stream);
int mvae_linear_wgrad_grouped(const float *dy, int lddy, size_t dy_gs, const float *x, int ldx,
                              size_t x_gs, float *dw, size_t dw_gs, float *db, size_t db_gs, int G,
                              int M, int N, int K, int flags, void *ws, size_t ws_bytes,
                              mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K2  Conv2d 4x4, bias=False, (stride,pad) in {(2,1),(1,0)}: fashionmnist/model.py:79,81;
 *     celeba/model.py:77,79,82,85; celeba19/model.py:103,105,108,111.
 *     Implicit im2col GEMM on fp32 MFMA; x[B,Cin,H,W], w[Cout,Cin,4,4], y[B,Cout,OH,OW].
 *     fwd  : pre = conv(x,w) ; act = swish(pre) (either may be NULL)
 *     dgrad: dx (+)= conv^T(dy,w) * swish'(pre_in)   (pre_in NULL for none)
 *     wgrad: dw (+)= correlate(x, dy)
 * K3  ConvTranspose2d 4x4, bias=False: fashionmnist/model.py:112,114; celeba/model.py:117,
 *     120,123,126; celeba19/model.py:143,146,149,152.  w[Cin,Cout,4,4].  Forward of the
 *     transpose is the dgrad of the mirrored conv and vice versa.
 * ---------------------------------------------------------------------------------- */
int mvae_conv2d_k4_fwd(const float *x, const float *w, float *pre, float *act,
                       int B, int Cin, int H, int W, int Cout, int stride, int pad,
                       mvae_stream_t stream);
int mvae_conv2d_k4_dgrad(const float *dy, const float *w, float *dx, const float *pre_in,
                         int B, int Cin, int H, int W, int Cout, int stride, int pad,
                         void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_conv2d_k4_wgrad(const float *dy, const float *x, float *dw,
                         int B, int Cin, int H, int W, int Cout, int stride, int pad,
                         int flags, void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_convT2d_k4_fwd(const float *x, const float *w, float *pre, float *act,
                        int B, int Cin, int H, int W, int Cout, int stride, int pad,
                        void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_convT2d_k4_dgrad(const float *dy, const float *w, float *dx, const float *pre_in,
                          int B, int Cin, int H, int W, int Cout, int stride, int pad,
                          mvae_stream_t stream);
int mvae_convT2d_k4_wgrad(const float *dy, const float *x, float *dw,
                          int B, int Cin, int H, int W, int Cout, int stride, int pad,
                          int flags, void *ws, size_t ws_bytes, mvae_stream_t stream);

/* The two dgrad-form launches -- mvae_conv2d_k4_dgrad and mvae_convT2d_k4_fwd -- read the weights from a
 * repacked copy (parity-class major, input channel contiguous) in `ws`.  With `w` given they make that copy
 * themselves, a small launch in front of every call.  A caller that runs many steps can make the copies of all
 * its layers in ONE launch per step instead (the weights only change in the optimizer) and pass w = NULL with
 * ws = the layer's copy:
 *   mvae_conv_k4_repack_floats   floats of the copy this launch would read, or 0 if it reads `w` directly (the
 *                                <= 4-channel and stride-1 5x5 shapes have their own kernels) -- then w = NULL is
 *                                MVAE_ERR_ARG.  transposed: 0 = Conv2d data gradient, 1 = ConvTranspose2d forward;
 *                                B, Cin, H, W, Cout, stride, pad exactly as in that call.
 *   mvae_conv_k4_repack_batched  up to 16 copies in one launch (Cin, Cout: the module's own). */
typedef struct {
    const float *w; float *wr;
    int transposed, Cin, Cout, stride, pad;
} mvae_repack_item;
size_t mvae_conv_k4_repack_floats(int transposed, const float *w, int B, int Cin, int H, int W, int Cout,
                                  int stride, int pad);
int mvae_conv_k4_repack_batched(const mvae_repack_item *items, int n_items, mvae_stream_t stream);

/* Statistics-only ConvTranspose2d forward: the transposed conv in FRONT OF THE LAST BatchNorm of a decoder pass whose
 * output the reference never reads -- celeba19/train.py:278-283 runs the image decoder for the 18 attribute-only terms
 * too (celeba19/model.py:52-61), celeba/train.py:195 for the attribute-only term; the only effect is the BatchNorm
 * running-statistics update (reproduced by default).  The launch computes the layer but STORES
 * NOTHING: each block leaves one (mean, M2) record per output channel over MVAE_STATS_TILE_ELEMS elements,
 *     part[tile][Cout][2],   tiles of one image -- hence of one batch group -- contiguous,
 * and mvae_bn_stats_merge turns the records of each group into that BatchNorm's saved + running statistics exactly
 * as mvae_bn_train_fwd(y = NULL) would from the activations (equal-count merge: mean = avg(mean_i),
 * M2 = sum(M2_i) + n * sum((mean_i - mean)^2); groups in order, n_updates times each).
 *   mvae_convT2d_k4_stats_tiles  number of records the launch writes, or 0 if the shape is not covered (covered:
 *                                stride 2, pad 1, <= 32 output channels, B*H*W a multiple of 128) -- the caller then
 *                                uses mvae_convT2d_k4_fwd + mvae_bn_train_fwd(y = NULL).
 *   w / ws                       as in mvae_convT2d_k4_fwd (w = NULL: ws holds the repacked copy). */
#define MVAE_STATS_TILE_ELEMS 512
size_t mvae_convT2d_k4_stats_tiles(int B, int Cin, int H, int W, int Cout, int stride, int pad);
int mvae_convT2d_k4_fwd_stats(const float *x, const float *w, float *part, size_t part_floats,
                              int B, int Cin, int H, int W, int Cout, int stride, int pad,
                              void *ws, size_t ws_bytes, mvae_stream_t stream);

/* Which kernel a 4x4 conv launch takes.  The library picks one of the kernels / template forms below by shape, batch
 * size and scratch size; this query runs the SAME decision function the launch switches on, launches nothing and
 * touches no device (like mvae_conv_k4_repack_floats, mvae_convT2d_k4_stats_tiles and mvae_gemm_ws_bytes).
 *   op        the launch (MVAE_OP_*); B, Cin, H, W, Cout, stride, pad mean exactly what they mean to that launch
 *   ws_bytes  the scratch that launch would be given (ignored by the launches without one)
 *   splits    (may be NULL) the number of reduction partials a finish launch sums, 1 where there is none
 *   returns   a MVAE_ROUTE_* code, or what the launch itself would return for these arguments without launching:
 *             MVAE_ERR_ARG (bad op / shape, a statistics-only shape that is not covered), MVAE_ERR_WS (scratch too small).
 * The query ASSUMES 16-BYTE-ALIGNED OPERANDS (with those, which of pre / act / pre_in a call passes does not change the
 * route); several kernels are only taken for aligned operands, so a launch on a less aligned view may take the
 * implicit-GEMM launch where the query names another.  MVAE_ROUTE_IGEMM covers the vector- and scalar-weight-load forms
 * and the tile plans of igemm_kernel: those differ in speed, not in the code path a shape test has to reach. */
#define MVAE_OP_CONV_FWD        0   /* mvae_conv2d_k4_fwd */
#define MVAE_OP_CONV_DGRAD      1   /* mvae_conv2d_k4_dgrad */
#define MVAE_OP_CONV_WGRAD      2   /* mvae_conv2d_k4_wgrad */
#define MVAE_OP_CONVT_FWD       3   /* mvae_convT2d_k4_fwd */
#define MVAE_OP_CONVT_FWD_STATS 4   /* mvae_convT2d_k4_fwd_stats */
#define MVAE_OP_CONVT_DGRAD     5   /* mvae_convT2d_k4_dgrad */
#define MVAE_OP_CONVT_WGRAD     6   /* mvae_convT2d_k4_wgrad */

#define MVAE_ROUTE_IGEMM            1   /* igemm_kernel on gathered operands (+ split finish for weight gradients) */
#define MVAE_ROUTE_IGEMM_PAIR       2   /* ... stride-2 dgrad form storing the two column classes of a row as pairs */
#define MVAE_ROUTE_GEMM2            3   /* gemm2_kernel (forward form; tuning builds only by default) */
#define MVAE_ROUTE_CONV_PATCH       4   /* retired (the forward-form LDS-patch kernel, removed): never returned; the number stays reserved */
#define MVAE_ROUTE_SMALL_FWD16      5   /* conv_small_fwd_kernel<Cin, 16>: <= 4 input channels, < 1024 blocks of 32 */
#define MVAE_ROUTE_SMALL_FWD32      6   /* conv_small_fwd_kernel<Cin, 32> */
#define MVAE_ROUTE_DGRAD_SMALL3D    7   /* convT_small3d_kernel: <= 4 output channels, rows through LDS by DMA */
#define MVAE_ROUTE_DGRAD_SMALL3     8   /* convT_small3_kernel: ... register-staged */
#define MVAE_ROUTE_DGRAD_SMALL2     9   /* convT_small2_kernel: ... straight from memory, two quads per thread */
#define MVAE_ROUTE_DGRAD_SMALL     10   /* convT_small_kernel: the plain form */
#define MVAE_ROUTE_S1              11   /* convT_s1_kernel<1>: stride 1, dense GEMM + col2im */
#define MVAE_ROUTE_S1_WIDE         12   /* convT_s1_kernel<2>: 128-column blocks */
#define MVAE_ROUTE_PATCH8          13   /* convT_patch2_kernel on the 8 x 8 lattice */
#define MVAE_ROUTE_PATCH7          14   /* ... 7 x 7 */
#define MVAE_ROUTE_PATCH16         15   /* ... 16 x 16 */
#define MVAE_ROUTE_PATCH_STATS     16   /* ... 16 x 16, statistics-only records */
#define MVAE_ROUTE_WGRAD_SMALLCIN  17   /* wgrad_smallcin_kernel<MT, NT> (+ finish) */
#define MVAE_ROUTE_WGRAD_SMALLCIN2 18   /* wgrad_smallcin2_kernel (+ finish) */
#define MVAE_ROUTE_WGRAD_PATCH     19   /* wgrad_patch_kernel (+ finish: few <= 16 < normal <= 64 < wide) */
int mvae_conv_k4_route(int op, int B, int Cin, int H, int W, int Cout, int stride, int pad,
                       size_t ws_bytes, int *splits /* may be NULL */);

/* Which kernel a Linear launch takes.  mvae_linear_fwd / _bce_fwd / _ce_fwd / _dgrad / _wgrad and their grouped forms pick
 * one of the kernel instantiations below by tile counts, reduction length, operand alignment, output form and scratch
 * size; this query runs the SAME route function the launch switches on, launches nothing, allocates nothing and touches
 * no device.
 *   op         the launch (MVAE_LOP_*); G = 1 for the single entry points (the fused losses have no grouped form)
 *   M, N, K    as that launch's own arguments (rows, output features, input features)
 *   ld_a, ld_b its two leading dimensions in the order of its argument list: (ldx, ldy) for the forwards, (lddy, lddx) for
 *              the data gradient, (lddy, ldx) for the weight gradient
 *   gs_a, gs_b the group strides of its two INPUT operands: (x, w), (dy, w), (dy, x); ignored for G = 1
 *   aligned    non-zero: both input operands are 16-byte aligned (the scratch is taken to be: allocators align it)
 *   fwd_form   MVAE_LOP_FWD only (MVAE_LFORM_*): which outputs the call stores
 *   want_db    MVAE_LOP_WGRAD only: a bias gradient is asked for
 *   ws_bytes   the scratch the launch would be given; 0 = none, i.e. ws = NULL: no split reduction
 *   splits     (may be NULL) the number of reduction partials a finish launch sums, 1 where there is none
 *   finish     (may be NULL) the launch that sums them (MVAE_LFINISH_*)
 *   returns    a MVAE_LROUTE_* code, or what the launch itself would return for these arguments without launching:
 *              MVAE_ERR_ARG (bad op / shape / leading dimension), MVAE_ERR_WS (scratch too small for the split plan).
 * Forward and data gradient share the gemm2s ids (the kernel's Q_RK parameter follows the op), the fused losses and the
 * weight gradient share the small igemm ids (the epilogue follows the op). */
#define MVAE_LOP_FWD      0   /* mvae_linear_fwd, mvae_linear_fwd_grouped */
#define MVAE_LOP_BCE_FWD  1   /* mvae_linear_bce_fwd */
#define MVAE_LOP_CE_FWD   2   /* mvae_linear_ce_fwd */
#define MVAE_LOP_DGRAD    3   /* mvae_linear_dgrad, mvae_linear_dgrad_grouped */
#define MVAE_LOP_WGRAD    4   /* mvae_linear_wgrad, mvae_linear_wgrad_grouped */

#define MVAE_LFORM_OTHER    0   /* pre alone, or act alone with a dropout mask */
#define MVAE_LFORM_PRE_ACT  1   /* pre and act */
#define MVAE_LFORM_ACT_ONLY 2   /* act alone, no mask */

#define MVAE_LFINISH_NONE     0
#define MVAE_LFINISH_FINISH   1   /* finish_kernel: more than 16 partials */
#define MVAE_LFINISH_FEW      2   /* finish_few_kernel */
#define MVAE_LFINISH_FEW_VEC  3   /* finish_few_vec_kernel: float4 partial loads */
#define MVAE_LFINISH_G2       4   /* g2_finish_kernel (the persistent gemm2 modes: tuning builds only) */

#define MVAE_LROUTE_GEMM2            1   /* gemm2_kernel, one 64 x 64 tile per block */
#define MVAE_LROUTE_G2S_32x64_K4     2   /* gemm2s_kernel: tile 32 x 64, 4 k-groups of waves */
#define MVAE_LROUTE_G2S_64x32_K4     3
#define MVAE_LROUTE_G2S_32x64_K2     4
#define MVAE_LROUTE_G2S_64x32_K2     5
#define MVAE_LROUTE_G2S_32x32_K8     6
#define MVAE_LROUTE_G2S_32x32_K4     7
#define MVAE_LROUTE_IGS_64x32_K4     8   /* igemm_kernel, small layouts (BK = 64, float4 loaders) */
#define MVAE_LROUTE_IGS_64x32_K2     9
#define MVAE_LROUTE_IGS_32x64_K4    10
#define MVAE_LROUTE_IGS_32x64_K2    11
#define MVAE_LROUTE_IGS_32x32_K8    12
#define MVAE_LROUTE_IGS_32x32_K4    13
#define MVAE_LROUTE_IG_32x128       14   /* igemm_kernel, large layouts (BK = 32), float4 loaders: the narrow plan */
#define MVAE_LROUTE_IG_128x128      15   /* the 128-row tiles: conv plans; a Linear launch takes them only when a tuning build forces the tile */
#define MVAE_LROUTE_IG_128x64       16
#define MVAE_LROUTE_IG_64x128       17
#define MVAE_LROUTE_IG_64x64_K4     18
#define MVAE_LROUTE_IG_64x64_K2     19
#define MVAE_LROUTE_IG_64x64        20
#define MVAE_LROUTE_IG_32x128_S     30   /* ... scalar loaders (an operand that float4 loads cannot take) */
#define MVAE_LROUTE_IG_128x128_S    31
#define MVAE_LROUTE_IG_128x64_S     32
#define MVAE_LROUTE_IG_64x128_S     33
#define MVAE_LROUTE_IG_64x64_K4_S   34
#define MVAE_LROUTE_IG_64x64_K2_S   35
#define MVAE_LROUTE_IG_64x64_S      36
#define MVAE_LROUTE_DGRAD_SMALLN    40   /* dgrad_smalln_kernel: N <= 16 */
#define MVAE_LROUTE_WGRAD_DIRECT_4  41   /* wgrad_direct_kernel, 4 waves per 32 x 32 tile */
#define MVAE_LROUTE_WGRAD_DIRECT_8  42
#define MVAE_LROUTE_WGRAD_DIRECT_16 43
#define MVAE_LROUTE_WGRAD_BATCHED2      50   /* wgrad_batched2_kernel */
#define MVAE_LROUTE_WGRAD_BATCHED       51   /* wgrad_batched_kernel */
#define MVAE_LROUTE_WGRAD_BATCHED_ADAM  52   /* wgrad_batched_adam_kernel */
int mvae_linear_route(int op, int G, int M, int N, int K, int ld_a, int ld_b, size_t gs_a, size_t gs_b, int aligned,
                      int fwd_form, int want_db, size_t ws_bytes, int *splits /* may be NULL */,
                      int *finish /* may be NULL */);
/* The same for mvae_linear_wgrad_batched (adam = 0) / mvae_linear_wgrad_batched_adam (adam != 0) on an item table: the
 * items' pointers are only compared with NULL and with one another, never dereferenced.
 *   tile_rows, tile_cols, waves  (each may be NULL) the output tile a block computes and the waves that share it
 *   returns    MVAE_LROUTE_WGRAD_BATCHED2 / _BATCHED / _BATCHED_ADAM, or MVAE_ERR_ARG where the launch refuses the table
 *              (the Adam form's checks of its mvae_adam_fuse argument are not part of the table and not repeated here). */
int mvae_linear_wgrad_batched_route(const mvae_wgrad_item *items, int n_items, int adam, int *tile_rows /* may be NULL */,
                                    int *tile_cols /* may be NULL */, int *waves /* may be NULL */);

/* ------------------------------------------------------------------------------------
 * K17 General stride-2 conv family (csrc/conv_gen.hip): Conv2d / ConvTranspose2d with a square kernel
 *     ks in {4, 5}, stride 2, pad in {0, 1}, bias=False, ANY map size (odd, non-square) with
 *     H + 2 pad >= ks and W + 2 pad >= ks (Conv2d) or H, W >= 1 (ConvTranspose2d, output_padding 0):
 *     the image stacks of multimnist/model.py:78-84 (Conv2d(32,64,4,2,1) on 25 x 25, Conv2d(128,256,4,2,0))
 *     and :120-128 (ConvTranspose2d(256,128,4,2,0), ConvTranspose2d(64,32,5,2,1)).
 *     Same contracts as the k4 launches above, argument for argument, with `ks` next to stride and pad:
 *     forward writes pre and / or act = swish(pre); the data gradients multiply by swish'(pre_in) when given;
 *     the weight gradients overwrite or (MVAE_ACCUMULATE) add.  Exact fp32 MFMA, no atomics, deterministic.
 *     Anything outside the domain -- other ks / stride / pad, a tensor of 2^28 elements or more (32-bit byte
 *     offsets) -- is MVAE_ERR_ARG.  Geometries the k4 family covers are accepted too, but the Python layers
 *     never send those here.  The two launches that take `ws` without being weight gradients (Conv2d data gradient,
 *     ConvTranspose2d forward) make a class-major copy of the weights there (MVAE_ERR_WS if it does not fit).
 *   mvae_conv_gen_ws_bytes   scratch the launch `op` (MVAE_OP_*, B, Cin, H, W, Cout as that launch's own
 *                            arguments) needs: the partial slabs of a split weight gradient, the weight copy of the
 *                            two launches above (Cin * Cout * ks * ks floats), 0 for the others.
 *   mvae_conv_gen_supported  1 / 0: the predicate the launches apply (transposed: 0 Conv2d, 1 ConvTranspose2d).
 *   Both are host only.
 * ---------------------------------------------------------------------------------- */
int mvae_conv2d_gen_fwd(const float *x, const float *w, float *pre, float *act,
                        int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad,
                        mvae_stream_t stream);
int mvae_conv2d_gen_dgrad(const float *dy, const float *w, float *dx, const float *pre_in,
                          int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad,
                          void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_conv2d_gen_wgrad(const float *dy, const float *x, float *dw,
                          int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad,
                          int flags, void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_convT2d_gen_fwd(const float *x, const float *w, float *pre, float *act,
                         int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad,
                         void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_convT2d_gen_dgrad(const float *dy, const float *w, float *dx, const float *pre_in,
                           int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad,
                           mvae_stream_t stream);
int mvae_convT2d_gen_wgrad(const float *dy, const float *x, float *dw,
                           int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad,
                           int flags, void *ws, size_t ws_bytes, mvae_stream_t stream);
size_t mvae_conv_gen_ws_bytes(int op, int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad);
int mvae_conv_gen_supported(int transposed, int B, int Cin, int H, int W, int Cout, int ks, int stride, int pad);

/* ------------------------------------------------------------------------------------
 * K4  BatchNorm2d / BatchNorm1d (training mode, eps 1e-5, momentum 0.1) + fused Swish:
 *     celeba/model.py:80,83,86,118,121,124,149,152,176,179,182; celeba19/model.py:106,109,
 *     112,144,147,150.  x is [G*B, C, HW] (HW = 1 for BatchNorm1d): G independent groups
 *     of B samples, each normalised with its own batch statistics -- G > 1 lets one launch
 *     serve the G model() calls of a train step that the reference issues separately.
 *     Running statistics are updated sequentially for g = 0..G-1, each `n_updates` times
 *     (unbiased variance for the running estimate, biased for normalisation).
 *     save_mean / save_invstd are [G, C].  ws: mvae_bn_ws_bytes(G, C, B*HW).
 *     y == NULL: statistics only (saved + running), for decoder passes the reference runs but
 *     whose output it never reads (celeba19/train.py:277-283 -- SURVEY Appendix B-4).
 *     eval: y = swish?((x - running_mean) / sqrt(running_var + eps) * gamma + beta).
 * ---------------------------------------------------------------------------------- */
size_t mvae_bn_ws_bytes(int G, int C, int n_per_group);
int mvae_bn_train_fwd(const float *x, const float *gamma, const float *beta, float *y,
                      float *save_mean, float *save_invstd,
                      float *running_mean, float *running_var,
                      int G, int B, int C, int HW, float eps, float momentum,
                      int n_updates, const int *n_updates_dev /* nullable: overrides n_updates */,
                      int flags, void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_bn_train_bwd(const float *dy, const float *x, const float *gamma, const float *beta,
                      const float *save_mean, const float *save_invstd,
                      float *dx, float *dgamma, float *dbeta,
                      int G, int B, int C, int HW, int flags,
                      void *ws, size_t ws_bytes, mvae_stream_t stream);
/* Which kernel mvae_bn_train_fwd (bwd = 0) / mvae_bn_train_bwd (bwd != 0) takes for a shape -- the route function the
 * launches themselves switch on (csrc/norm.hip bn_shape + bn_route).  Host only: launches nothing, allocates nothing,
 * touches no device, holds no state.
 *   aligned    x, y / dy and dx are all 16-byte aligned (an operand that is not takes every HW onto the scalar kernels)
 *   slices     (may be NULL) S, the batch slices per (group, channel) of the two-launch routes; 1 for the others
 *   launches   (may be NULL) kernel launches of the call: 2 for the two-launch routes, 1 for the fused and BatchNorm1d
 *              routes; MVAE_BNROUTE_SLICE reports 2, the call WITH running statistics (its second launch advances them and
 *              is skipped when running_mean == NULL)
 *   returns    a MVAE_BNROUTE_* code, or the MVAE_ERR_ARG the launch would return for this shape (a non-positive
 *              dimension, B * HW >= 2^31, G * B * C * HW >= 2^40).  Null pointers and the workspace size (MVAE_ERR_WS) are
 *              the launch's own checks and not repeated here. */
#define MVAE_BNROUTE_TWO_VEC_ROWS     1   /* bn_partial_stats / bn_fwd_apply / bn_bwd_partial / bn_bwd_apply, float4 sweep, a row per HW/4 lanes */
#define MVAE_BNROUTE_TWO_VEC_COLS     2   /* ... float4 sweep, lanes walk the columns of a row (HW/4 no power of two, or HW > 1024) */
#define MVAE_BNROUTE_TWO_SCALAR       3   /* ... one element per lane (HW % 4 != 0, or an unaligned operand) */
#define MVAE_BNROUTE_FUSED_VEC_G1     4   /* bn_fused_{fwd,bwd}_kernel<true, 1, 4>: all groups in one block, float4 units */
#define MVAE_BNROUTE_FUSED_VEC_G2     5   /* <true, 2, 4> */
#define MVAE_BNROUTE_FUSED_VEC_G3     6   /* <true, 3, 4>: forward only */
#define MVAE_BNROUTE_FUSED_SCALAR_G1  7   /* <false, 1, 16>: 16 one-element units per thread */
#define MVAE_BNROUTE_FUSED_SCALAR_GN  8   /* <false, 3 (forward) / 2 (backward), 8>: 8 units per thread and group */
#define MVAE_BNROUTE_BN1D_G1          9   /* bn1d_fused_{fwd,bwd}_kernel<1>: HW = 1, 16 columns per block */
#define MVAE_BNROUTE_BN1D_GN         10   /* bn1d_fused_{fwd,bwd}_kernel<3> */
#define MVAE_BNROUTE_SLICE           11   /* bn_slice_fwd_kernel (+ bn_running_kernel): forward only */
int mvae_bn_route(int bwd, int G, int B, int C, int HW, int aligned, int *slices /* may be NULL */,
                  int *launches /* may be NULL */);
/* saved + running statistics of G groups from the records of mvae_convT2d_k4_fwd_stats (`tiles` records of
 * `elems_per_tile` elements per channel; tiles % G == 0, a group's tiles contiguous).  save_* may be NULL. */
int mvae_bn_stats_merge(const float *part, int tiles, int elems_per_tile, int G, int C,
                        float *save_mean, float *save_invstd, float *running_mean, float *running_var,
                        float eps, float momentum, int n_updates, const int *n_updates_dev, mvae_stream_t stream);
int mvae_bn_eval_fwd(const float *x, const float *gamma, const float *beta, float *y,
                     const float *running_mean, const float *running_var,
                     int N, int C, int HW, float eps, int flags, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K5  stand-alone Swish (only where no producer epilogue can host it).
 * K6  Embedding lookup + Swish and its scatter-add backward: mnist/model.py:116,123;
 *     fashionmnist/model.py:133; celeba19/model.py:174,183.
 *     fwd: act[r,:] = swish(w[idx[r],:]) ; bwd: dw[c,:] (+)= sum_{r: idx[r]==c} dact[r,:]*swish'(w[c,:])
 *     idx is int64 (labels) or, with idx_is_float, the {0,1} floats celeba19 casts by .long().
 * ---------------------------------------------------------------------------------- */
int mvae_swish_fwd(const float *x, float *y, size_t n, mvae_stream_t stream);
int mvae_swish_bwd(const float *dy, const float *x, float *dx, size_t n, mvae_stream_t stream);
/* sample.py (mnist/sample.py:100-112, celeba/sample.py): std = exp(logvar/2) comes from mvae_reparam_fwd with
 * mu = 0, eps = 1; z = eps * std + mu for n_samples draws of ONE posterior row is the periodic affine map
 * below (period = n_latents; 1 for the prior N(0,1)); F.sigmoid on the image decoder's logits. */
int mvae_sigmoid_fwd(const float *x, float *y, size_t n, mvae_stream_t stream);
int mvae_affine_fwd(const float *x, const float *scale, const float *shift, float *y, size_t n, size_t period,
                    mvae_stream_t stream);
int mvae_embedding_swish_fwd(const void *idx, int idx_is_float, const float *w, float *act,
                             int R, int n_classes, int width, mvae_stream_t stream);
int mvae_embedding_swish_bwd(const void *idx, int idx_is_float, const float *w,
                             const float *dact, float *dw,
                             int R, int n_classes, int width, int flags, mvae_stream_t stream);
/* grouped: table / output / index g at base + g * <name>_gs elements (celeba19: idx = attrs[B,18],
 * idx_is_float = 18 (row stride), idx_gs = 1 (column g)); dw shares w's group stride. */
int mvae_embedding_swish_fwd_grouped(const void *idx, int idx_is_float, size_t idx_gs, const float *w,
                                     size_t w_gs, float *act, size_t act_gs, int G, int R,
                                     int n_classes, int width, mvae_stream_t stream);
int mvae_embedding_swish_bwd_grouped(const void *idx, int idx_is_float, size_t idx_gs, const float *w,
                                     size_t w_gs, const float *dact, size_t dact_gs, float *dw, int G,
                                     int R, int n_classes, int width, int flags, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K8-K10, K12  prior expert + product of experts + reparameterise + analytic KL, fused:
 *     mnist/model.py:29-35,46-64,156-163,172-185; celeba/model.py:200-207;
 *     celeba19/model.py:63-89,219-226; KL: mnist/train.py:56, celeba/train.py:62,
 *     celeba19/train.py:58.
 *     E experts (the N(0,1) prior is implicit and always present) given as mu_e/logvar_e
 *     pointers with a common row stride `ld`; T terms, term t fuses the experts whose bit
 *     is set in masks[t] (DEVICE uint32[T], so a captured graph can be replayed with new
 *     subsets).  noise is [T,B,D] or NULL (eval: z = mu).
 *     fwd outputs mu/logvar/z [T,B,D] and kl[T,B] = -0.5*sum_d(1+lv-mu^2-exp(lv)).
 *     bwd inputs: dz, dmu, dlogvar [T,B,D] and dkl [T,B] = d loss / d kl (any may be NULL);
 *     outputs the per-expert gradients, summed over the terms that contain the expert.
 * ---------------------------------------------------------------------------------- */
typedef struct {
    const float *mu[MVAE_MAX_EXPERTS];
    const float *logvar[MVAE_MAX_EXPERTS];
} mvae_experts_t;
typedef struct {
    float *dmu[MVAE_MAX_EXPERTS];
    float *dlogvar[MVAE_MAX_EXPERTS];
} mvae_expert_grads_t;

int mvae_poe_fwd(const mvae_experts_t *experts, int ld, int E,
                 const uint32_t *masks_dev, int T,
                 const float *noise, float *mu, float *logvar, float *z, float *kl,
                 int B, int D, int variant, mvae_stream_t stream);
/* mvae_poe_fwd that draws its own reparameterisation noise (mnist/model.py:32: eps = std.data.new(size).normal_()):
 * eps[T,B,D] = exactly the standard normals mvae_philox_fill(seed, *counter_dev + counter_offset) would write,
 * generated inside the launch and stored to noise_out for the backward.  The counter is not advanced. */
int mvae_poe_fwd_draw(const mvae_experts_t *experts, int ld, int E,
                      const uint32_t *masks_dev, int T,
                      float *noise_out, uint64_t seed, const uint64_t *counter_dev, uint64_t counter_offset,
                      float *mu, float *logvar, float *z, float *kl,
                      int B, int D, int variant, mvae_stream_t stream);
int mvae_poe_bwd(const mvae_experts_t *experts, int ld, int E,
                 const uint32_t *masks_dev, int T,
                 const float *noise, const float *mu, const float *logvar,
                 const float *dz, const float *dmu, const float *dlogvar,
                 const float *dkl, int dkl_per_term /* dkl is [T] (beta/B per term) instead of [T,B] */,
                 const mvae_expert_grads_t *grads, int ldg,
                 int B, int D, int variant, mvae_stream_t stream);

/* mvae_poe_bwd with the latent gradient in TWO buffers: dz of term t = dz_a[slot_a[t]] + dz_b[slot_b[t]], each
 * buffer [n_slots, B, D] holding only the terms its decoder saw (slot -1: the term is not in that buffer;
 * slot_* are HOST arrays of T ints).  The fused step's two decoders run on two streams; with one buffer each,
 * neither their first layers' data gradients nor a cleared shared dz sit on the joined chain.  The sum is taken
 * a-then-b: same bits as accumulating b onto a. */
int mvae_poe_bwd_split(const mvae_experts_t *experts, int ld, int E,
                       const uint32_t *masks_dev, int T,
                       const float *noise, const float *mu, const float *logvar,
                       const float *dz_a, const int *slot_a, const float *dz_b, const int *slot_b,
                       const float *dkl, int dkl_per_term,
                       const mvae_expert_grads_t *grads, int ldg,
                       int B, int D, int variant, mvae_stream_t stream);

/* stand-alone reparameterised draw for the public MVAE.reparametrize (mnist/model.py:29-35):
 * z = eps * exp(0.5 * logvar) + mu */
int mvae_reparam_fwd(const float *mu, const float *logvar, const float *eps, float *z, size_t n,
                     mvae_stream_t stream);
int mvae_reparam_bwd(const float *dz, const float *logvar, const float *eps,
                     float *dmu, float *dlogvar, size_t n, mvae_stream_t stream);

/* stand-alone KL rows for the reference-surface elbo_loss(mu, logvar) (mnist/train.py:56) */
int mvae_kl_rows_fwd(const float *mu, const float *logvar, float *kl, int B, int D,
                     mvae_stream_t stream);
int mvae_kl_rows_bwd(const float *mu, const float *logvar, const float *dkl,
                     float *dmu, float *dlogvar, int B, int D, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K11 BCE-with-logits row sums: mnist/train.py:47-49,62-74; celeba/train.py:50-58,68-80;
 *     celeba19/train.py:52-57,63-75.  logits/target [R,P];
 *     rowsum[r] = sum_p colw[(r / rows_per_group), p] * bce(logits[r,p], target[r % target_rows, p])
 *     (colw NULL -> 1).  target row of logits row r is (r / target_div) % target_rows, its element p
 *     lives at row * target_row_stride + p * target_col_stride (contiguous: div 1, strides P and 1;
 *     celeba19 reads column i of attrs[B,18] for decoder i with strides 1 and 18).
 *     bwd: dlogits[r,p] = drow[r / rows_per_group] * colw * dbce/dx  (drow is a DEVICE array;
 *     d loss / d rowsum is the constant lambda/B, so the fwd entry can emit it in the same pass).
 * K13 categorical CE: mnist/train.py:52,77-94.  row[r] = -log_softmax(logits[r,:]+1e-6)[label[r % label_rows]]
 * K14 ELBO combine: total = sum_r coef[r / rows_per_group] * rows[r]  (mnist/train.py:57-58,214)
 * ---------------------------------------------------------------------------------- */
int mvae_bce_rowsum_fwd(const float *logits, const float *target, const float *colw,
                        float *rowsum, const float *drow_dev, float *dlogits /* nullable: fused bwd */,
                        int R, int P, int rows_per_group, int target_rows,
                        int target_div, int target_row_stride, int target_col_stride,
                        mvae_stream_t stream);
int mvae_bce_rowsum_bwd(const float *logits, const float *target, const float *colw,
                        const float *drow_dev, float *dlogits,
                        int R, int P, int rows_per_group, int target_rows,
                        int target_div, int target_row_stride, int target_col_stride,
                        mvae_stream_t stream);
/* Which kernel mvae_bce_rowsum_fwd / _bwd take for a row of P logits, and how the block kernel walks it -- the functions
 * the launch and the kernel themselves switch on (csrc/loss.hip bce_block_row + bce_row_vec).  Host only: launches nothing,
 * allocates nothing, touches no device, holds no state.
 *   aligned        the row's logits, target, column weights and dlogits pointers are all 16-byte aligned (the kernel decides
 *                  per row: a target row stride that is no multiple of 4 floats takes some rows off the float4 path)
 *   has_colw       colw != NULL: weighted rows stay off the batched loop
 *   batched_trips  (may be NULL) the four-group trips thread 0 of the block makes (no thread makes more); 0 off the float4 path
 *   tail           (may be NULL) 1 if any thread makes a single-group trip; 0 off the float4 path
 *   returns        a MVAE_BCEROUTE_* code, or the MVAE_ERR_ARG the launch would return (P <= 0, target_col_stride <= 0;
 *                  the out-pointers are then left alone).  The launch's other checks are not repeated here. */
#define MVAE_BCE_BLOCK_MIN_P 512            /* rows of at least this many logits take a block each, shorter ones a wave */
#define MVAE_BCEROUTE_WAVE               1  /* bce_row_wave_kernel: a wave per row, one element per lane and trip */
#define MVAE_BCEROUTE_BLOCK_SCALAR       2  /* bce_row_block_kernel, one element per thread and trip (P % 4 != 0, a column
                                               stride, or an unaligned operand) */
#define MVAE_BCEROUTE_BLOCK_VEC          3  /* ... float4, single-group trips only */
#define MVAE_BCEROUTE_BLOCK_VEC_BATCHED  4  /* ... float4, thread 0 makes at least one four-group trip */
int mvae_bce_route(int P, int target_col_stride, int aligned, int has_colw, int *batched_trips /* may be NULL */,
                   int *tail /* may be NULL */);
int mvae_ce_fwd(const float *logits, const int64_t *label, float *row,
                const float *drow_dev, float *dlogits /* nullable: fused bwd */,
                int R, int K, int rows_per_group, int label_rows, mvae_stream_t stream);
int mvae_ce_bwd(const float *logits, const int64_t *label, const float *drow_dev,
                float *dlogits, int R, int K, int rows_per_group, int label_rows,
                mvae_stream_t stream);
/* K1 + K12 / K13 in one launch: a decoder's LAST Linear whose only consumer is its reconstruction term
 * (mnist/model.py:104 -> mnist/train.py:47-49,62-74; mnist/model.py:146 -> mnist/train.py:52,77-94).  The logits
 * stay in the GEMM's accumulators: the epilogue writes d loss / d logits (what the backward consumes) and the loss.
 *   bce: dlogits[m][n] = drow[m / rows_per_group] * dBCE(logit, target[(m % target_rows) * target_row_stride + n]),
 *        partial[m][n / 32] = sum of the 32 columns' terms  (partial is [M, ceil(N / 32)] floats; a row's term is
 *        the sum of its partials -- mvae_elbo_reduce with rows_per_group = B * ceil(N / 32) adds them up);
 *   ce : N <= 32 classes; row[m] and dlogits as mvae_ce_fwd defines them, label[m % label_rows].
 * `logits` (nullable): also store the logits (tests).  The reduction is never split. */
int mvae_linear_bce_fwd(const float *x, int ldx, const float *w, const float *bias, const float *target,
                        int target_rows, int target_row_stride, const float *drow_dev, int rows_per_group,
                        float *dlogits, int ldy, float *logits, float *partial, int M, int N, int K,
                        mvae_stream_t stream);
int mvae_linear_ce_fwd(const float *x, int ldx, const float *w, const float *bias, const int64_t *label,
                       int label_rows, const float *drow_dev, int rows_per_group, float *dlogits, int ldy,
                       float *logits, float *row, int M, int N, int K, mvae_stream_t stream);
/* The ELBO of a whole fused step in one launch (mnist/train.py:57-58 batch mean per term, :214 sum of terms;
 * celeba19/train.py:59,265-302).  Each part is a vector of loss rows in `groups` groups of `rows_per_group`;
 * group g feeds term `term_of[g]` (device table) or `first_term + g`:
 *     elbo[t] = sum over parts and groups of term t of  coef[g] * sum(rows of g),   elbo[T] = sum over everything,
 * accumulated part by part, group by group (fixed order).  Optionally clears `zero[0..zero_n)` (the latent
 * gradient the decoders' first layers accumulate into) and advances a Philox launch counter by `counter_inc`
 * -- the step's bookkeeping that would otherwise be 5-6 single-purpose launches.  At most 1024 groups over all
 * parts; a part of more than one row per group has at most MVAE_ELBO_MAX_TERMS groups. */
#define MVAE_ELBO_MAX_PARTS 4
#define MVAE_ELBO_MAX_TERMS 40
#define MVAE_ELBO_LONG_GROUP 2048   /* a group of more rows than this is summed by all 16 waves of the block, not by one */
typedef struct {
    const float *rows;      /* [groups * rows_per_group] */
    const float *coef;      /* per group, device; NULL = 1 */
    const int *term_of;     /* per group, device; NULL = first_term + group */
    int first_term, groups, rows_per_group;
} mvae_elbo_part;
int mvae_elbo_reduce(const mvae_elbo_part *parts, int n_parts, float *elbo, int T, float *zero, size_t zero_n,
                     uint64_t *counter_dev, uint64_t counter_inc, mvae_stream_t stream);
/* mvae_elbo_reduce whose launch also does what mvae_adam_prepare does: *step_dev += delta, then coef2[0..1] = the two
 * bias-correction factors at the new counter value (the same double-precision expressions).  For a fused step in
 * which nothing reads coef2 before the update at the end of the chain: the bookkeeping launch is ordered before that
 * update anyway, so the optimizer's counter launch leaves the encoder branch it used to end. */
int mvae_elbo_reduce_prepare(const mvae_elbo_part *parts, int n_parts, float *elbo, int T, float *zero,
                             size_t zero_n, uint64_t *counter_dev, uint64_t counter_inc, int64_t *step_dev,
                             int64_t delta, double lr, double beta1, double beta2, float *coef2,
                             mvae_stream_t stream);
/* out[g] (+)= coef[g] * sum_{r in group g} rows[r] for g < G; *total_out (+)= sum_g of those
 * (either destination may be NULL) */
int mvae_group_sums(const float *rows, const float *coef_dev, float *out, float *total_out,
                    int G, int rows_per_group, int flags, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K10 noise: counter-based Philox4x32-10 on device (perf mode; parity mode passes the
 *     host-drawn noise of the reference's CPU generator instead).  `counter_dev` is a
 *     device uint64 advanced by the kernel itself, so a captured hipGraph replays fresh noise.
 * K15 Adam (torch.optim.Adam defaults, mnist/train.py:168,219), one launch over the flat
 *     parameter arena; `step_dev` is a device int64 incremented by the kernel.
 * ---------------------------------------------------------------------------------- */
int mvae_randn(float *out, size_t n, uint64_t seed, uint64_t *counter_dev, mvae_stream_t stream);
int mvae_bernoulli(float *out, size_t n, float keep_prob, uint64_t seed, uint64_t *counter_dev,
                   mvae_stream_t stream);
/* the same draws at launch index *counter_dev + counter_offset WITHOUT advancing the counter (a fused step
 * advances it once, in mvae_elbo_reduce) */
int mvae_philox_fill(float *out, size_t n, int bernoulli, float keep_prob, uint64_t seed,
                     const uint64_t *counter_dev, uint64_t counter_offset, mvae_stream_t stream);
int mvae_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                   size_t n, double lr, double beta1, double beta2, double eps, float grad_scale,
                   int64_t *step_dev, mvae_stream_t stream);
/* Adam over a range of the arena WITHOUT advancing `step_dev` (t = *step_dev + 1): data-parallel replicas
 * update each gradient bucket as its all-reduce lands and advance the counter once per step with
 * mvae_counter_add (mnist/train.py:219 is ONE optimizer.step(); the ranges partition it). */
int mvae_adam_apply(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                    size_t n, double lr, double beta1, double beta2, double eps, float grad_scale,
                    const int64_t *step_dev, mvae_stream_t stream);
/* mvae_adam_apply at step t = *step_dev + step_add (step_add = 0: the caller advanced the counter earlier in
 * the step, off the critical chain, and needs no counter launch behind the update) */
int mvae_adam_apply_at(float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                       size_t n, double lr, double beta1, double beta2, double eps, float grad_scale,
                       const int64_t *step_dev, int64_t step_add, mvae_stream_t stream);
/* *step_dev += delta, then coef2[0..1] = { lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) } at t = the new counter value:
 * the counter launch of a step whose weight-gradient launches apply Adam themselves
 * (mvae_linear_wgrad_batched_adam); a later mvae_adam_apply_at(..., step_add = 0) on the rest of the arena computes
 * the same two factors from the counter. */
int mvae_adam_prepare(int64_t *step_dev, int64_t delta, double lr, double beta1, double beta2, float *coef2,
                      mvae_stream_t stream);
int mvae_counter_add(int64_t *counter_dev, int64_t delta, mvae_stream_t stream);
/* mvae_adam_apply_at(..., step_add = 0) with the step's two bias-correction factors READ from coef2 instead of recomputed
 * from the counter (ABI 6): the fused step's counter launch is mvae_adam_prepare -- early in the step, off the critical
 * chain -- and the update at the end of the chain (mnist/train.py:219) starts streaming at once: the two double-precision
 * pow() behind the factors were ~300 fp64 instructions in front of every wavefront of the 72-MB MNIST update.  Same
 * arithmetic as mvae_adam_apply_at, bit for bit. */
int mvae_adam_apply_coef(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                         const float *coef2, double beta1, double beta2, double eps, float grad_scale,
                         mvae_stream_t stream);

/* Measurement aid (no reference counterpart): an EMPTY kernel on `stream`.  A profiling host launches one in front of
 * every call of a single-stream step; in the rocprofv3 kernel trace the k-th marker dispatch then separates the kernels
 * of call k - 1 from those of call k (tools/step_by_shape.py -> profiles/r04_*_by_shape.txt, the per-(call, shape)
 * table bench.py's roofline.rocprof_avg_us is read from).  `tag` is not interpreted. */
int mvae_trace_marker(int tag, mvae_stream_t stream);
int mvae_fill(float *out, size_t n, float value, mvae_stream_t stream);
/* One launch that puts a step's inputs where a captured graph reads them -- what `image.cuda()`, `text.cuda()`
 * (mnist/train.py:188-190) and the per-step scalars (annealing factor :180-186) amount to for a replayed step:
 * image_dst <- image_src (device, 16-byte aligned, a multiple of 4 floats), label_dst <- label_src (device, a multiple
 * of 4 bytes), table_dst <- table_src_host: PINNED HOST memory (hipHostMalloc / torch pin_memory) read by the kernel
 * itself.  Any of the three may be empty (size 0). */
int mvae_ingest(const float *image_src, float *image_dst, size_t image_floats,
                const void *label_src, void *label_dst, size_t label_bytes,
                const void *table_src_host, void *table_dst, size_t table_bytes, mvae_stream_t stream);

/* CelebA-19 term plumbing (celeba19/train.py:264-302, celeba19/model.py:56-60): gather the z blocks
 * a decoder needs, scatter-add the gradients back per term, and sum ELBO pieces by term table.
 *   block_gather      : dst[j] = src[idx[j]]                     (blocks of block_elems floats)
 *   block_scatter_add : dst[t] += sum_{j: idx[j]==t} src[j]      (j ascending: deterministic)
 *   scatter_sums      : out[idx[j]] += coef[j]*vals[j]; *total (+)= sum_j coef[j]*vals[j]
 * idx tables are DEVICE int32 so a captured graph follows each step's sampled subsets. */
int mvae_block_gather(const float *src, const int *idx_dev, float *dst, int n_dst, size_t block_elems,
                      mvae_stream_t stream);
int mvae_block_scatter_add(const float *src, const int *idx_dev, float *dst, int n_src, int n_dst,
                           size_t block_elems, mvae_stream_t stream);
int mvae_scatter_sums(const float *vals, const float *coef_dev, const int *idx_dev, float *out,
                      float *total_out, int n, int flags, mvae_stream_t stream);

/* K7 Dropout fan-out (celeba/model.py:89-92 runs twice per step on the same batch; only the
 *    Bernoulli draw differs): out[g,b,:] = h[b,:] * masks[g,b,:] * scale, and its backward
 *    dh[b,:] = sum_g dout[g,b,:] * masks[g,b,:] * scale. */
int mvae_dropout_fanout_fwd(const float *h, const float *masks, float *out, float scale,
                            int G, int B, int N, mvae_stream_t stream);
int mvae_dropout_fanin_bwd(const float *dout, const float *masks, float *dh, float scale,
                           int G, int B, int N, mvae_stream_t stream);
/* elementwise BCE-with-logits, the reference helper's own shape (mnist/train.py:62-74) */
int mvae_bce_elem_fwd(const float *logits, const float *target, float *out, size_t n,
                      mvae_stream_t stream);
int mvae_bce_elem_bwd(const float *logits, const float *target, const float *g,
                      float *dlogits, float *dtarget, size_t n, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Input pipeline: what the reference's DataLoader workers do per image on
 * the CPU, on a batch of raw uint8 images resident in HBM.
 *   mvae_u8_to_f32            : ToTensor (mnist/train.py:160,164): dst = (float)src / 255
 *   mvae_resize_crop_u8_to_f32: Compose([Resize(S), CenterCrop(S), ToTensor()]) (celeba/train.py:
 *       146-148, celeba19/train.py:200-202) on src[B,H,W,3] -> dst[B,3,S,S].  Resize is Pillow's
 *       8-bit separable BILINEAR resample (torchvision delegates to it), byte-exact: the caller
 *       builds the fixed-point coefficient tables of both axes once per image size with the HOST
 *       function mvae_resample_coeffs (kk[out, ksize], bounds[out, 2] = first tap, taps; ksize =
 *       mvae_resample_ksize) and uploads them; out_h/out_w = the resized size, (crop_top,
 *       crop_left) the crop origin in it, [y0, y1) the source rows the cropped rows depend on
 *       (min/max over their bounds).  One block per image, (y1-y0)*S*3 bytes of LDS <= 150 KiB.
 * ---------------------------------------------------------------------------------- */
int mvae_resample_ksize(int in_size, int out_size);
int mvae_resample_coeffs(int in_size, int out_size, int *kk_host, int *bounds_host);
int mvae_resize_crop_u8_to_f32(const uint8_t *src, float *dst, int B, int H, int W, int out_h,
                               int out_w, int S, int crop_top, int crop_left, const int *kx_dev,
                               const int *bx_dev, int ksx, const int *ky_dev, const int *by_dev,
                               int ksy, int y0, int y1, mvae_stream_t stream);
int mvae_u8_to_f32(const uint8_t *src, float *dst, size_t n, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K16  The recurrent text stacks of the MultiMNIST MVAE: multimnist/model.py:145-235 --
 *      TextEncoder: nn.Embedding(12, 200) -> nn.GRU(200, 200, 1, bidirectional) -> x[-1], directions summed ->
 *      nn.Linear(200, 2D) (:162-179); TextDecoder: nn.Linear(D, 200) -> 4 steps of
 *      swish(nn.Embedding) | z -> nn.GRU(200 + D, 200, 2, dropout=0.1) -> | z -> nn.Linear(200 + D, 12), greedy
 *      arg-max feedback (:196-228).  The matrix products are mvae_linear_* launches with leading dimensions (the
 *      torch.cat's of :222,226 are column ranges of one buffer); these are the remaining element kernels.
 *   gru_cell_fwd  torch's gate order r | z | n in gi = x.W_ih^T + b_ih and gh = h.W_hh^T + b_hh ([B, 3H] each):
 *                 r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h' = (1 - z) n + z h;
 *                 gates [B, 4H] (r | z | n | gh_n, nullable) is what the backward needs.
 *   gru_cell_bwd  dh' = dh_new (+ dh_extra, nullable) -> dgi, dgh [B, 3H] contiguous and dh_prev [B, H] = dh' * z
 *                 (the caller adds dgh.W_hh with an accumulating mvae_linear_dgrad).
 *   embedding_fwd / _bwd   nn.Embedding with an index stride (column t of text[B, 4]: stride 4) and an output
 *                 leading dimension; flags: MVAE_ACT_SWISH (swish(embed(c)), :220), bwd also MVAE_ACCUMULATE.
 *                 The backward adds the rows of a class in row order: deterministic.
 *   copy2d        dst[r, :cols] (+)= src[r, :cols] (* mask[r, :cols] * scale): column ranges of the cat buffers, the
 *                 inter-layer Dropout of nn.GRU (mask in {0,1}, scale 1 / 0.9) and its backward, the direction sum.
 *   argmax_rows   first maximum per row (torch.max(F.log_softmax(c_out, dim=1), dim=1)[1], :211).
 * ------------------------------------------------------------------------------------ */
int mvae_gru_cell_fwd(const float *gi, int ldgi, const float *gh, int ldgh, const float *h_prev, int ldh,
                      float *h_new, int ldo, float *gates /* nullable */, int B, int H, mvae_stream_t stream);
int mvae_gru_cell_bwd(const float *dh_new, int lddh, const float *dh_extra /* nullable */, int ldde,
                      const float *gates, const float *h_prev, int ldh, float *dgi, float *dgh, float *dh_prev,
                      int B, int H, mvae_stream_t stream);
int mvae_embedding_fwd(const int64_t *idx, int idx_stride, const float *w, float *out, int ldo, int R,
                       int n_classes, int width, int flags, mvae_stream_t stream);
int mvae_embedding_bwd(const int64_t *idx, int idx_stride, const float *w, const float *dout, int ldd, float *dw,
                       int R, int n_classes, int width, int flags, mvae_stream_t stream);
int mvae_copy2d(const float *src, int lds, float *dst, int ldd, const float *mask /* nullable */, int ldm,
                float scale, int rows, int cols, int flags, mvae_stream_t stream);
int mvae_argmax_rows(const float *x, int ldx, int64_t *out, int R, int K, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K18  The whole greedy TextDecoder after z2h in one launch per direction (csrc/gru_seq.hip).  A workgroup owns 16
 *      batch rows for all L steps of both GRU layers, the h2o Linear and the arg-max feedback; workgroups never
 *      communicate (no grid barrier, flag or atomic).  All buffers are contiguous fp32 (fed: int64), weights in
 *      nn.GRU / nn.Linear layout: w_ih0 [3H, H+D], w_hh0 / w_ih1 / w_hh1 [3H, H], w_h2o [n_chars, H+D].
 *   gru_dec_seq_supported  host-only: 1 where the kernels' LDS plan holds (both fit the CU's 160 KiB; n_chars <= 16;
 *                 H, D, L <= 4096; B * 4H and B * (H+D) below 2^31), else 0.  H and D need no alignment.
 *   gru_dec_seq_fwd  z [B, D], hz = z2h(z) [B, H] -> words [B, L, n_chars]; masks (nullable) [L, B, H] in {0, 1}, the
 *                 layer-0 output is multiplied by mask * mask_scale.  The tape (all seven pointers, or none of them)
 *                 is time-major: xcat_all, ocat_all [L, B, H+D]; h0_all, h1_all [L+1, B, H] (slot 0 = hz);
 *                 d0_all [L, B, H]; gates0, gates1 [L, B, 4H] (r | z | n | gh_n).  fed (nullable) [L, B]: the
 *                 characters fed in, fed[0] = sos.  Character indices are clamped to [0, n_chars).
 *   gru_dec_seq_bwd  dwords [B, L, n_chars] and the tape -> dgi0/dgh0/dgi1/dgh1_all [L, B, 3H], demb_all [L, B, H]
 *                 (gradient of swish(embed)), dlog_all [L, B, n_chars] (dwords time-major), dhz [B, H], dz [B, D]
 *                 (the direct paths only; the caller adds dhz . W_z2h).  No weight gradients: those are Linear
 *                 weight-gradient launches on the [L * B, .] views.
 *   Both return MVAE_ERR_ARG before any launch on a null pointer, B <= 0 or an unsupported geometry.
 * ------------------------------------------------------------------------------------ */
int mvae_gru_dec_seq_supported(int B, int H, int D, int n_chars, int L);
int mvae_gru_dec_seq_fwd(const float *z, const float *hz, const float *w_emb, const float *w_ih0, const float *w_hh0,
                         const float *b_ih0, const float *b_hh0, const float *w_ih1, const float *w_hh1,
                         const float *b_ih1, const float *b_hh1, const float *w_h2o, const float *b_h2o,
                         const float *masks /* nullable */, float mask_scale, float *words, float *xcat_all,
                         float *h0_all, float *h1_all, float *d0_all, float *ocat_all, float *gates0, float *gates1,
                         int64_t *fed /* nullable */, int B, int H, int D, int n_chars, int L, int sos,
                         mvae_stream_t stream);
int mvae_gru_dec_seq_bwd(const float *dwords, const float *w_ih0, const float *w_hh0, const float *w_ih1,
                         const float *w_hh1, const float *w_h2o, const float *masks /* nullable */, float mask_scale,
                         const float *h0_all, const float *h1_all, const float *gates0, const float *gates1,
                         float *dgi0_all, float *dgh0_all, float *dgi1_all, float *dgh1_all, float *demb_all,
                         float *dlog_all, float *dhz, float *dz, int B, int H, int D, int n_chars, int L,
                         mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K19  The whole TextEncoder in one launch per direction (csrc/gru_enc_seq.hip): the embedding gathers, the L cells of
 *      the forward-direction GRU, the ONE cell of the reverse direction that x[-1] uses (on position L-1, from h = 0),
 *      s = h_L + h_b and out = s . W_h2p^T + b_h2p.  Ownership as K18: a workgroup owns 16 batch rows for the whole
 *      sequence; workgroups never communicate (no grid barrier, flag or atomic).  All buffers are contiguous fp32
 *      (x, idx_all: int64), weights in nn.GRU / nn.Linear layout: w_ih, w_hh (and the reverse pair) [3H, H],
 *      w_h2p [P, H] with P = 2 * n_latents, w_emb [n_chars, H].
 *   gru_enc_seq_supported  host-only: 1 where both kernels' LDS plans fit the CU's 160 KiB, H, P, L <= 4096,
 *                 B * 4H < 2^31 and bidirectional is 0 or 1; else 0 (any size <= 0 included).  No alignment needed.
 *   gru_enc_seq_fwd  x [B, L] -> out [B, P].  Characters are clamped to [0, n_chars) before any address is formed.
 *                 Unidirectional: the four reverse parameters are null (all four or none).  The tape (all five of
 *                 e_all, h_all, gates, s, idx_all, plus gates_r exactly when bidirectional; or none of them) is
 *                 time-major: e_all [L, B, H]; h_all [L+1, B, H] (slot 0 zeros, slot t+1 the state after position t);
 *                 gates [L, B, 4H] and gates_r [B, 4H] (r | z | n | gh_n); s [B, H]; idx_all [L, B] the clamped
 *                 characters.  Without a tape nothing but out is written.
 *   gru_enc_seq_bwd  dout [B, P] and the tape -> dgi_all, dgh_all [L, B, 3H], de_all [L, B, H] (gradient of the
 *                 gathered embeddings; position L-1 includes the reverse cell's part) and, bidirectional (w_ih_r,
 *                 gates_r, dgi_r, dgh_r: all four or none), dgi_r, dgh_r [B, 3H].  No weight gradients: those are
 *                 Linear weight-gradient launches on the [L * B, .] views and one embedding backward on idx_all.
 *   Both return MVAE_ERR_ARG before any launch on a null required pointer, a partial tape or reverse set, gates_r
 *   without reverse parameters, or an unsupported geometry.
 * ------------------------------------------------------------------------------------ */
int mvae_gru_enc_seq_supported(int B, int H, int P, int n_chars, int L, int bidirectional);
int mvae_gru_enc_seq_fwd(const int64_t *x, const float *w_emb, const float *w_ih, const float *w_hh, const float *b_ih,
                         const float *b_hh, const float *w_ih_r /* nullable */, const float *w_hh_r /* nullable */,
                         const float *b_ih_r /* nullable */, const float *b_hh_r /* nullable */, const float *w_h2p,
                         const float *b_h2p, float *out, float *e_all, float *h_all, float *gates,
                         float *gates_r /* nullable */, float *s, int64_t *idx_all, int B, int H, int P, int n_chars,
                         int L, mvae_stream_t stream);
int mvae_gru_enc_seq_bwd(const float *dout, const float *w_h2p, const float *w_ih, const float *w_hh,
                         const float *w_ih_r /* nullable */, const float *h_all, const float *gates,
                         const float *gates_r /* nullable */, float *dgi_all, float *dgh_all,
                         float *dgi_r /* nullable */, float *dgh_r /* nullable */, float *de_all, int B, int H, int P,
                         int n_chars, int L, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K20  Importance-weighted marginal log-likelihood (csrc/loglike.hip): the element work of the `loglike.py` the
 *      reference's README names in every experiment folder ("to compute the marginal log likelihood log p(x) using
 *      q(z|x,y) as the inference network", README.md) but never published.  With K samples per
 *      datum the decoders and the loss-row kernels (K11, K13) run on the K * B rows between these two launches.
 *   iw_draw        mu, logvar [B, D] with row stride ld (column ranges of a heads buffer) -> z [Kc, B, D] contiguous,
 *                  sample-major (row r = k * B + b belongs to datum r % B: the addressing mvae_ce_fwd's label_rows and
 *                  mvae_bce_rowsum_fwd's target_rows already use, so the decoders take z as a plain batch of Kc * B rows)
 *                  and lw [Kc, B]:   z = mu + exp(0.5 logvar) * eps,
 *                  lw[k, b] = sum_d 0.5 eps^2 - 0.5 z^2 + 0.5 logvar  (= log p(z) - log q(z | x); the 2 pi terms cancel).
 *                  eps [Kc, B, D] given: used as is (parity runs).  eps NULL: generated in the launch -- exactly the
 *                  standard normals mvae_philox_fill(seed, *counter_dev + counter_offset) would write for a [Kc, B, D]
 *                  array (the contract of mvae_poe_fwd_draw); the counter is not advanced.  eps_out (nullable) receives
 *                  the noise used.  One wave per row, lanes along d, fixed reduction order: a row's lw does not depend
 *                  on Kc or B.  MVAE_ERR_ARG on a non-positive size, ld < D, a null pointer, Kc * B >= 2^31.
 *   iw_accumulate  folds a chunk of log-weights  logw[k, b] = lw[k, b] - sum_j rec_a[(k * B + b) * rows_a + j]
 *                  - sum_j rec_b[(k * B + b) * rows_b + j]  (rec_*: nullable loss rows, i.e. -log p, in the same
 *                  sample-major order; rows_* rows per sample: 1, or 4 for the [Kc, B, 4] text rows) into
 *                  state [B, 2] = (running maximum, running sum of exp(logw - maximum)) by the online log-sum-exp merge.
 *                  The caller initialises state to (-inf, 0); the maximum is subtracted before every exp and a -inf
 *                  maximum is never subtracted from itself.  finish_k > 0 (the TOTAL number of samples folded so far,
 *                  this chunk included) also writes out[b] = maximum + log(sum) - log(finish_k).  One wave per datum,
 *                  lanes along k, wave maximum then wave sum: no atomics, deterministic.
 * ------------------------------------------------------------------------------------ */
int mvae_iw_draw(const float *mu, const float *logvar, int ld, const float *eps /* nullable */, uint64_t seed,
                 const uint64_t *counter_dev /* nullable with eps */, uint64_t counter_offset,
                 float *eps_out /* nullable */, float *z, float *lw, int Kc, int B, int D, mvae_stream_t stream);
int mvae_iw_accumulate(const float *lw, const float *rec_a /* nullable */, int rows_a,
                       const float *rec_b /* nullable */, int rows_b, float *state, float *out /* nullable */,
                       int Kc, int B, int finish_k, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K21  MultiMNIST dataset builder (csrc/multimnist_data.hip): the compose step of multimnist/datasets.py:107-146 --
 *      0-4 MNIST digits, each resized to w x w (scipy.misc.imresize = Pillow's 8-bit BILINEAR), padded to its place
 *      on a 50 x 50 canvas, summed; "crude check for overlapping digits": np.max(canvas) > 255 -- for M canvases in
 *      ONE launch over a digit bank resident in HBM.
 *   bank   uint8 [n_bank, 28, 28], 4-byte aligned.
 *   plan   int32 [M, MVAE_MM_PLAN_STRIDE] on the device: n (0..4), then four records (bank index, w, top, left);
 *          records past n are not read.  The digit lands on rows top..top+w, columns left..left+w (np.pad's first
 *          pair pads rows).  The caller validates: 0 <= index < n_bank, MVAE_MM_WMIN <= w <= MVAE_MM_WMAX,
 *          0 <= top, top + w <= 50, the same for left.  A canvas whose plan breaks one of these is not composed:
 *          it comes out all zero with flag -1.
 *   kk     int32 [44, 50, MVAE_MM_KSIZE], bounds int32 [44, 50, 2] on the device: for every width w, slice
 *          w - MVAE_MM_WMIN holds the host tables of mvae_resample_coeffs(28, w) (rows of ksize(28, w) <= 9
 *          coefficients, zero-padded to 9; rows past w unused).  One table serves both passes.
 *   canvas uint8 [M, 50, 50], 4-byte aligned: min(sum, 255) -- exact wherever flags is 0.
 *   flags  int32 [M]: 1 if any pixel sum exceeds 255 (a sum of exactly 255 is not flagged), else 0.
 *   Horizontal pass first, uint8 intermediate, then the vertical pass, like mvae_resize_crop_u8_to_f32; w = 28 is
 *   the identity.  One 256-thread block per canvas; integer sums, no atomics, deterministic.
 *   Null pointers, M <= 0, n_bank <= 0 or a misaligned bank / canvas: MVAE_ERR_ARG before any launch.
 * ------------------------------------------------------------------------------------ */
#define MVAE_MM_DIGIT 28
#define MVAE_MM_CANVAS 50
#define MVAE_MM_MAX_DIGITS 4
#define MVAE_MM_PLAN_STRIDE 17
#define MVAE_MM_WMIN 7
#define MVAE_MM_WMAX 50
#define MVAE_MM_KSIZE 9
int mvae_multimnist_compose(const uint8_t *bank, int n_bank, const int *plan_dev, int M, const int *kk_dev,
                            const int *bounds_dev, uint8_t *canvas, int *flags, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K22  Segmented BCE-with-logits row sums (csrc/loss_multi.hip): the reconstruction terms of SEVERAL image
 *      modalities in one launch -- vision/train.py:20-58,61-73 sums six image BCEs per ELBO term and :183-288
 *      evaluates seven terms per step.  For up to MVAE_BCE_MULTI_MAX segments (logits matrices of R rows each):
 *        rowsum[r] = sum_s weight_s * sum_p bce(logits_s[r, p], target_s[r % target_rows, p])
 *        dlogits_s[r, p] = drow[r / rows_per_group] * weight_s * dbce/dx        (drow is a DEVICE array)
 *      with the bce of K11.  A row's elements are cut into chunks of 4096 across blocks (the grid follows the bytes,
 *      not R); each block leaves one weighted partial in `ws`, and a second small launch adds a row's partials in
 *      index order: no atomics, the same inputs give the same bits.  float4 loads where P % 4 == 0 and the segment's
 *      pointers are 16-byte aligned, scalar loads otherwise (decided per segment).
 *   fwd   writes rowsum (nullable) and, for every segment with dlogits where drow_dev is given, the gradient in the
 *         same pass.  ws: mvae_bce_multi_ws_bytes(segs, n_segs, R) bytes (R * chunks-per-row floats), read and
 *         written only when rowsum is given.
 *   bwd   the gradient alone, the same arithmetic (bit-equal to the fused one); segments without dlogits are skipped.
 *   mvae_bce_multi_ws_bytes is a host-only function of the P's and R (pointers are only compared with NULL); 0 for
 *         a table the launches refuse.
 *   Refused on the host before any launch: a null table, a null logits / target, n_segs outside 1..8, P <= 0,
 *   R <= 0, rows_per_group <= 0 or R % rows_per_group != 0, target_rows <= 0, nothing to write (no rowsum and no
 *   gradient), R * chunks-per-row >= 2^31 -- MVAE_ERR_ARG; scratch too small -- MVAE_ERR_WS.
 * ------------------------------------------------------------------------------------ */
#define MVAE_BCE_MULTI_MAX 8
typedef struct {
    const float *logits;   /* [R, P] contiguous */
    const float *target;   /* [target_rows, P] contiguous; row of logits row r is r % target_rows */
    float *dlogits;        /* [R, P] or NULL: no gradient for this segment */
    int P;
    float weight;
} mvae_bce_seg;
size_t mvae_bce_multi_ws_bytes(const mvae_bce_seg *segs, int n_segs, int R);
int mvae_bce_multi_fwd(const mvae_bce_seg *segs, int n_segs, float *rowsum /* nullable */,
                       const float *drow_dev /* nullable */, int R, int rows_per_group, int target_rows,
                       void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_bce_multi_bwd(const mvae_bce_seg *segs, int n_segs, const float *drow_dev, int R, int rows_per_group,
                       int target_rows, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K23  The vision experiment's input pipeline (csrc/vision_data.hip): what vision/datasets.py:54-91 does per item on
 *      the CPU, for a batch of raw uint8 sources resident in HBM, in ONE launch -- six float32 NCHW batches.
 *   rgb [B, H, W, 3], edge / mask [B, H, W], gray [B, H, W] or NULL (then gray is the luma of rgb, Pillow's
 *   convert('L'): (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16), mark [H, W, 4]: the RGBA watermark already resized
 *   to H x W, one for the batch.  All uint8, contiguous; no alignment is required of any of them.
 *   image_out / obscured_out / watermark_out [B, 3, S, S], gray_out / edge_out / mask_out [B, 1, S, S].
 *     obscured  = rgb where x <= W / 2, else 0                                          (vision/datasets.py:108-109)
 *     watermark = Pillow's paste(mark, (0, 0), mark) on rgb: per channel t = dst * (255 - a) + src * a + 128,
 *                 ((t >> 8) + t) >> 8 with a the mark's alpha                                         (:125-128)
 *   Then every plane takes Resize + CenterCrop + ToTensor exactly as mvae_resize_crop_u8_to_f32 (same tables, same
 *   meaning of out_h / out_w, crop_top / crop_left, [y0, y1)); mask_out holds 1.0f - u8 / 255.0f (:87).
 *   Grid (B, 4): a block owns three planes (image | obscured | watermark | gray, edge, mask) and reads each source
 *   byte once; (y1 - y0) * S * 3 bytes of LDS plus 32 KiB of staged rows, <= 150 KiB.  No atomics, no scratch.
 *   Refused on the host before any launch (MVAE_ERR_ARG): a null pointer other than gray, a non-positive size, a crop
 *   outside the resized image, [y0, y1) outside the image or empty, an LDS need above 150 KiB.
 * ------------------------------------------------------------------------------------ */
int mvae_vision_compose(const uint8_t *rgb, const uint8_t *edge, const uint8_t *mask, const uint8_t *gray /* nullable */,
                        const uint8_t *mark, float *image_out, float *gray_out, float *edge_out, float *mask_out,
                        float *obscured_out, float *watermark_out, int B, int H, int W, int out_h, int out_w, int S,
                        int crop_top, int crop_left, const int *kx_dev, const int *bx_dev, int ksx, const int *ky_dev,
                        const int *by_dev, int ksy, int y0, int y1, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K24  Importance-weighted estimates of several image modalities from one decoder pass (csrc/loglike_multi.hip): the
 *      vision experiment's evaluation wants the six marginals log p(x_m) and the joint log p(x_1..x_6) of a datum from
 *      the same K draws.  K20's accumulate folds ONE state from at most two reconstruction rows and K22 returns only
 *      the weighted sum over its segments; here up to MVAE_BCE_MULTI_MAX segments (mvae_bce_seg: logits [R, P_s] on the
 *      R = Kc * B sample-major rows of mvae_iw_draw, target [B, P_s], row r reads target row r % B; dlogits and weight
 *      are ignored) give S + 1 states in two launches:
 *        rec_s[k, b]  = sum_p bce(logits_s[k * B + b, p], target_s[b, p])                 (the bce of K11)
 *        logw_s[k, b] = lw[k, b] - rec_s[k, b]                       s = 0 .. S-1         (the marginals)
 *        logw_S[k, b] = lw[k, b] - (rec_0 + rec_1 + ... + rec_{S-1})[k, b], added in segment order    (the joint)
 *        state[j, b]  = (running maximum, running sum of exp(logw_j - maximum)) over k,   state [S + 1, B, 2]
 *        out[j, b]    = maximum + log(sum) - log(finish_k)           when finish_k > 0,   out [S + 1, B]
 *   score   K22's plan: a row's elements are cut into chunks of 4096, one block per (row, chunk), one unweighted
 *           partial per block in `ws`; float4 loads where P % 4 == 0 and the segment's pointers are 16-byte aligned,
 *           scalar loads otherwise (decided per segment).
 *   fold    one wave per (state, datum), lanes along k: a lane adds its sample's partials per segment in index order
 *           (the per-segment row sums never exist as an array), forms its log-weight, and the wave merges it into the
 *           state by K20's rules: the caller initialises state to (-inf, 0), the maximum is subtracted before every
 *           exp, a -inf maximum is never subtracted from itself, wave maximum then wave sum.  finish_k as in
 *           mvae_iw_accumulate: the TOTAL number of samples folded so far, this chunk included.
 *   No atomics: the same inputs give the same bits.  With S = 1 state 0 and state 1 hold the same bits.
 *   mvae_iw_score_multi_ws_bytes is a host-only function of the P's and R = Kc * B (R * chunks-per-row floats); 0 for
 *   a table the launch refuses.
 *   Refused on the host before any launch: a null table, a null logits / target / lw / state, n_segs outside 1..8,
 *   P <= 0, Kc <= 0, B <= 0, finish_k < 0, finish_k > 0 without out, Kc * B or R * chunks-per-row >= 2^31 --
 *   MVAE_ERR_ARG; scratch too small -- MVAE_ERR_WS.
 * ------------------------------------------------------------------------------------ */
size_t mvae_iw_score_multi_ws_bytes(const mvae_bce_seg *segs, int n_segs, int R);
int mvae_iw_score_multi(const mvae_bce_seg *segs, int n_segs, const float *lw, float *state, float *out /* nullable */,
                        int Kc, int B, int finish_k, void *ws, size_t ws_bytes, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K25  Importance-weighted estimates of many one-logit modalities from one decoder pass (csrc/loglike_heads.hip): the
 *      CelebA-19 evaluation wants the image marginal, the 18 attribute marginals log p(a_i) and the joint of a datum from
 *      the same K draws.  The 18 attribute decoders end in Linear(512, 1): K24 stops at MVAE_BCE_MULTI_MAX segments and
 *      wants a logits matrix per segment, K20's accumulate folds one state per launch.  Two entry points:
 *   heads_bce_rows  the last layer of G one-logit heads fused with its Bernoulli term, on the R = Kc * B sample-major rows
 *                   of mvae_iw_draw:
 *                     logit[g, r] = sum_j h[g * h_gs + r * ldh + j] * w[g * w_gs + j] + bias[g * b_gs]        j < H
 *                     rec[g * rec_gs + r] = bce(logit[g, r], target[(r % target_rows) * ldt + g])     (the bce of K11)
 *                     logits_out[g * logits_gs + r] = logit[g, r]                                (nullable: parity runs)
 *                   h: the post-Swish output of the third grouped Linear, [G, R, H] with unit column stride and any
 *                   ldh >= H.  w, bias: (pointer of group 0, group stride in floats), like the grouped Linear entry
 *                   points.  target: float {0, 1} [target_rows, >= G] with row stride ldt; group g reads column g (a
 *                   column range of the [B, 18] attribute matrix is passed as it is).  Grid (row blocks, G): lanes along
 *                   H, a wave owns a row at a time, the group's weight row stays in registers across the rows of a
 *                   block, the wave reduces in a fixed shuffle order.  float4 loads where H % 4 == 0, ldh % 4 == 0, h_gs
 *                   and w_gs are multiples of 4 and h and w are 16-byte aligned; scalar loads otherwise (decided once per
 *                   launch).  Every activation is read once: HBM-bound.  No atomics, no scratch: the same inputs give
 *                   the same bits, and a row's value depends neither on R nor on the grid.
 *                   Refused on the host before any launch (MVAE_ERR_ARG): a null h / w / bias / target / rec, G outside
 *                   1..4096, R, H or target_rows <= 0, ldh < H, ldt < G, G * R >= 2^31.
 *   iw_fold_rows    K24's fold for row sums that already exist, up to MVAE_IW_FOLD_MAX states besides the joint:
 *                     logw_j[k, b] = lw[k, b] - rec[sel[j] * rec_ss + k * B + b]                      j = 0 .. S-1
 *                     logw_S[k, b] = lw[k, b] - (rec[sel[0]..] + ... + rec[sel[S-1]..])[k, b]   added in j order
 *                     state [S + 1, B, 2], out [S + 1, B], finish_k as in mvae_iw_accumulate
 *                   sel: a HOST array of S row indices, passed to the kernel by value; NULL means 0 .. S-1 (a subset of
 *                   the rows is scored without a copy; the caller answers for sel[j] * rec_ss + Kc * B lying inside rec).
 *                   One wave per (state, datum), lanes along k, K20's rules: the caller initialises state to (-inf, 0),
 *                   the maximum is subtracted before every exp, a -inf maximum is never subtracted from itself, wave
 *                   maximum then wave sum, no atomics.  With S = 1 state 0 and state 1 hold the same bits.
 *                   Refused on the host before any launch (MVAE_ERR_ARG): a null rec / lw / state, S outside 1..64, a
 *                   negative sel entry, Kc or B <= 0, rec_ss < Kc * B, finish_k < 0, finish_k > 0 without out,
 *                   Kc * B >= 2^31.
 * ------------------------------------------------------------------------------------ */
#define MVAE_IW_FOLD_MAX 64
int mvae_heads_bce_rows(const float *h, int ldh, size_t h_gs, const float *w, size_t w_gs, const float *bias, size_t b_gs,
                        const float *target, int target_rows, int ldt, float *rec, size_t rec_gs,
                        float *logits_out /* nullable */, size_t logits_gs, int G, int R, int H, mvae_stream_t stream);
int mvae_iw_fold_rows(const float *rec, size_t rec_ss, const int *sel /* host, nullable */, int S, const float *lw,
                      float *state, float *out /* nullable */, int Kc, int B, int finish_k, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K26  Canny edge detection for a batch of uint8 images in HBM (csrc/vision_setup.hip): the edge step of the reference's
 *      vision/setup.py:55-75, which calls scikit-image's feature.canny(image / 255., sigma) per file.  What is computed is
 *      that function's documented algorithm on a float image in [0, 1] with its default thresholds and no mask:
 *   1 luma      g = u8 / 255; with channels == 3 first L = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 (Pillow's
 *               convert('L'), the luma of K23).
 *   2 blur      taps w[k] = exp(-k^2 / 2 sigma^2), |k| <= r = int(4 sigma + 0.5), normalised to sum 1 (built on the host
 *               in double, used as fp32); separable, down the columns then along the rows, zeros outside the image; divided by the same blur
 *               of an all-ones image, by[y] * bx[x].
 *   3 gradient  isobel along rows, jsobel along columns: the unnormalised 3 x 3 Sobel (1-2-1 across, -1 0 +1 along) of the
 *               blurred image with its border sample duplicated; mag = sqrt(isobel^2 + jsobel^2).
 *   4 maxima    candidates: pixels not on the image border with mag > 0.  With ai = |isobel|, aj = |jsobel| and
 *               (c1, c2, w) =   same sign (both >= 0 or both <= 0), ai >= aj:  (+1, 0)  (+1, +1)  aj / ai
 *                               same sign, ai <= aj:                           (0, +1)  (+1, +1)  ai / aj
 *                               opposite sign, ai <= aj:                       (0, +1)  (-1, +1)  ai / aj
 *                               opposite sign, ai >= aj:                       (-1, 0)  (-1, +1)  aj / ai
 *               ((dy, dx) offsets; the cases are applied in this order, a later one overwrites an earlier one), a
 *               candidate is a local maximum when mag[c2] * w + mag[c1] * (1 - w) <= mag with these offsets and with
 *               them negated.
 *   5 classes   2 (strong): a local maximum with mag >= high; 1 (weak): one with low <= mag < high; 0: the rest.
 *   6 edges     255 where the 8-connected component of non-zero classes a pixel lies in holds a strong pixel, else 0.
 *   src [B, H, W] (channels 1) or [B, H, W, 3] (channels 3), edges / cls [B, H, W] uint8, mag [B, H, W] float; cls and mag
 *   may be NULL.  The uint8 pointers may have any byte alignment (mag: a float's).  Two launches: a tiled float stage
 *   (32 x 32 pixels per block, steps 1-5, one class byte per pixel into cls or, when cls is NULL, into ws) and the
 *   hysteresis (one block per image, the class plane in LDS).  mvae_canny_hysteresis is step 6 alone on a caller's class
 *   plane (a value above 2 counts as strong).  No atomics: the same inputs give the same bits.
 *   mvae_canny_supported: 1 when H, W >= 3, 0 < sigma and r <= 16 (sigma < 4.125), and (H + 2) * ((W + 11) & ~3) <= 144 KiB
 *   (the padded class plane of one image in one block's LDS; 218 x 178 is 41.4 KB); else 0.  Host-only.
 *   mvae_canny_ws_bytes: B * H * W, or 0 for a shape the launch refuses.  Host-only.  ws is not read when cls is given.
 *   Refused on the host before any launch: a null src / edges (mvae_canny_hysteresis: cls / edges), channels other than
 *   1 or 3, B <= 0, a shape or sigma mvae_canny_supported refuses, low < 0, high < low, a NaN or infinite threshold --
 *   MVAE_ERR_ARG; cls NULL and ws NULL or smaller than mvae_canny_ws_bytes -- MVAE_ERR_WS.
 * ------------------------------------------------------------------------------------ */
int mvae_canny_supported(int H, int W, float sigma);
size_t mvae_canny_ws_bytes(int B, int H, int W);
int mvae_canny(const uint8_t *src, int channels /* 1: gray [B,H,W]; 3: RGB [B,H,W,3] */, int B, int H, int W,
               float sigma, float low, float high,
               uint8_t *edges /* [B,H,W], 0 or 255 */, uint8_t *cls /* nullable [B,H,W]: 0 none, 1 weak, 2 strong */,
               float *mag /* nullable [B,H,W] */, void *ws, size_t ws_bytes, mvae_stream_t stream);
int mvae_canny_hysteresis(const uint8_t *cls, uint8_t *edges, int B, int H, int W, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K27  Product of experts of condition rows that each select their own experts, with n draws per row
 *      (csrc/poe_table.hip).  MVAE.infer (celeba19/model.py:63-89) takes None per modality for the whole batch; a batch
 *      whose rows condition on different subsets (a sweep over every attribute value, imputing missing attributes) has no
 *      launch there.  A celeba19 AttributeEncoder reads its {0, 1} input through Embedding(2, 512): in eval mode the 2 * A
 *      heads of a model are a fixed table, and a row's posterior is a product over a per-row selection from it.
 *   table     float [A, 2, 2D] contiguous: row (a, v) = expert a's head for input value v, mu in the first D columns,
 *             logvar in the last D.
 *   state     int8 [C, A] on the device: -1 attribute absent, 0 / 1 selects table row (a, state).  The caller validates
 *             (any other value selects nothing: the launch never reads outside the table).
 *   img_heads float [img_rows, 2D] with row stride ld_img >= 2D, or NULL; img_row int32 [C] on the device: the row of
 *             img_heads condition c uses, -1 for none; several conditions may name one row.  The caller validates
 *             -1 <= img_row < img_rows (a value >= img_rows is treated as -1).  With img_heads NULL img_row is not read.
 *   mu, logvar [C, D], z [n, C, D] contiguous.  PoE variant B as K8-K10 compute it for celeba19: T_e = 1 / (exp(logvar_e) + 1e-8),
 *             the N(0, 1) prior always an expert, experts added in the order infer stacks them (prior, image, attributes
 *             ascending), mu = sum mu_e T_e / sum T_e, logvar = log(1 / sum T_e), z = mu + exp(0.5 logvar) * eps.
 *             n = 0 is legal: mu and logvar only (eval-mode reparametrize: z = mu), z / eps / the counter are not touched.
 *   eps       [n, C, D] given: used as is.  NULL: generated in the launch -- exactly the standard normals
 *             mvae_philox_fill(seed, *counter_dev + counter_offset) would write for an [n, C, D] array (the contract of
 *             mvae_iw_draw and mvae_poe_fwd_draw); the counter is not advanced.  eps_out (nullable) receives the noise used.
 *   One wave per (condition, slice of 8 draws), lanes along d (D need not be a multiple of 64); the image row and every
 *   selected table row of a condition are requested before the first is reduced; every slice recomputes the posterior in
 *   the same fixed order and slice 0 stores it.  No atomics, no scratch: the same inputs give the same bits, and a row's
 *   values depend neither on C nor on n.
 *   Refused on the host before any launch (MVAE_ERR_ARG): a null table / state / mu / logvar, A outside
 *   1..MVAE_POE_TABLE_MAX_A, C or D <= 0, n < 0, n > 8 * 65535, img_heads with a null img_row, img_rows <= 0 or
 *   ld_img < 2D, n > 0 with a null z or with neither eps nor counter_dev.
 * ------------------------------------------------------------------------------------ */
#define MVAE_POE_TABLE_MAX_A 32
int mvae_poe_table_draw(const float *table, int A, const int8_t *state, const float *img_heads /* nullable */, int ld_img,
                        int img_rows, const int32_t *img_row /* nullable with img_heads */,
                        const float *eps /* nullable */, uint64_t seed,
                        const uint64_t *counter_dev /* nullable with eps or n = 0 */, uint64_t counter_offset,
                        float *eps_out /* nullable */, float *mu, float *logvar, float *z /* nullable with n = 0 */,
                        int n, int C, int D, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K28  Label prediction from a trained model (csrc/predict.hip): the Monte-Carlo posterior predictive of the label
 *      modality, E_{q(z | x)} p(y | z) in the log domain, and its scoring against labels -- the classification accuracy the
 *      MVAE paper reports beside its log-likelihoods (predict.py).  K20 folds one state per datum; a prediction needs one
 *      per (datum, class).  Two entry points:
 *   predict_fold   logits: the label decoder's output on the R = Kc * B sample-major rows of mvae_iw_draw (row r belongs to
 *                  datum r % B), C logits per row, element (r, c) at logits[r * row_stride + c * col_stride] ([R, C]
 *                  row-major: (C, 1); the [G, R] block of grouped one-logit heads: (1, R)).
 *                    MVAE_PREDICT_CATEGORICAL   v[k, b, c] = logits[r, c] - logsumexp_c' logits[r, c']      r = k * B + b
 *                                               state [B, C, 2], out [B, C]
 *                    MVAE_PREDICT_BERNOULLI     v[k, b, c, 0] = -softplus(-logits[r, c])   (class 1 first)
 *                                               v[k, b, c, 1] = -softplus(+logits[r, c])
 *                                               state [B, C, 2, 2], out [B, C, 2]
 *                  A state entry is (running maximum, running sum of exp(v - maximum)) over the samples folded so far,
 *                  merged by K20's rules: the caller initialises it to (-inf, 0), the maximum is subtracted before every
 *                  exp, a -inf maximum is never subtracted from itself, lanes along k, wave maximum then wave sum.
 *                  finish_k > 0 (the total number of samples folded, this chunk included) also writes
 *                  out = maximum + log(sum / finish_k) (the merge's carry and this line are formed in double and
 *                  rounded once).  A row's log-normaliser is computed once per row with the
 *                  row's own maximum subtracted (a tile of 256 rows of a datum at a time, kept in LDS); a -inf logit gives
 *                  v = -inf.  Kc = 1 on a fresh state with finish_k = 1 returns v itself: plain log_softmax /
 *                  -softplus (the no-sampling path, z = mu, uses the same launch).  Categorical: one block per datum;
 *                  Bernoulli: one wave per (datum, head).  No atomics, no scratch: the same inputs give the same bits,
 *                  and a datum's value does not depend on B or, beyond rounding, on how K is cut into chunks.
 *                  Refused on the host before any launch (MVAE_ERR_ARG): a null logits / state, an unknown mode, R, B or
 *                  C <= 0, R % B != 0, C > MVAE_PREDICT_MAX_C, a stride <= 0, strides under which two elements alias
 *                  (neither row_stride > (C - 1) * col_stride nor col_stride > (R - 1) * row_stride), finish_k < 0,
 *                  finish_k > 0 without out, R * C >= 2^31.
 *   predict_score  logp: predict_fold's out.  targets: categorical int64 [B]; Bernoulli float {0, 1} [B, C] with row
 *                  stride target_stride >= C (not read in categorical mode).
 *                    categorical   pred[b] = argmax_c logp[b, c] (the lowest index on a tie), nll[b] = -logp[b, y_b],
 *                                  correct[b] = (pred[b] == y_b), confusion [C, C] (truth, prediction) += the counts
 *                    Bernoulli     pred[b, c] = logp[b, c, 0] > logp[b, c, 1], nll[b, c] = -logp[b, c, 1 - y],
 *                                  correct[b, c] = (pred == y), confusion [C, 2, 2] (head, truth, prediction) += the counts
 *                  pred int64, nll float, correct uint8; confusion int64, nullable: the caller zeroes it once and passes
 *                  it call after call (stream order serialises the calls).  A target outside 0 .. C - 1 (Bernoulli:
 *                  other than 0 or 1) is counted nowhere, gives nll = +inf and correct = 0, and never indexes the table.
 *                  targets NULL: predictions only -- nll, correct and confusion must be NULL too.  One block: threads
 *                  loop over the rows, the counts go to an integer histogram in LDS, then the same block adds it to the
 *                  table with plain loads and stores.  No global atomics; integer counts: the same bits every run.
 *                  Refused on the host before any launch (MVAE_ERR_ARG): a null logp / pred, an unknown mode, B or
 *                  C <= 0, C > MVAE_PREDICT_MAX_C, B * C >= 2^31, targets without nll or correct, nll / correct /
 *                  confusion without targets, Bernoulli targets with target_stride < C.
 * ------------------------------------------------------------------------------------ */
#define MVAE_PREDICT_MAX_C 64
#define MVAE_PREDICT_CATEGORICAL 0
#define MVAE_PREDICT_BERNOULLI 1
int mvae_predict_fold(const float *logits, long long row_stride, long long col_stride, int R, int B, int C, int mode,
                      float *state, float *out /* nullable */, int finish_k, mvae_stream_t stream);
int mvae_predict_score(const float *logp, int mode, const void *targets /* nullable */, int target_stride, int B, int C,
                       int64_t *pred, float *nll /* nullable with targets */, uint8_t *correct /* nullable with targets */,
                       int64_t *confusion /* nullable */, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K29 Ragged product of experts: the PoE of K8-K10 for a batch whose rows observe different modalities (weak
 *     supervision; csrc/poe_ragged.hip).  The reference has no counterpart: its loop runs every term on every row
 *     (mnist/train.py:197-218; the `is_paired` of multimnist/train.py:189 is a comment without code).
 *   slot_dev   int32 [T, B]: the row of the COMPACT outputs that (term t, batch row b) owns, or -1 where the term is
 *              not evaluated on the row.  mu / logvar / z are [R, D], kl is [R]; rows >= R are never written, and a
 *              slot outside 0..R-1 counts as -1.  An inactive (t, b) costs nothing; a wave whose row has no active
 *              term exits.
 *   experts    expert e's head is compact as well: [n_rows[e], ld] (n_rows: HOST array of E ints; pointers of an
 *              expert with no row may be NULL), and erow_dev int32 [E, B] gives batch row b's row in it, or -1.  erow
 *              maps the rows that have expert e one-to-one onto 0..n_rows[e]-1; an entry outside counts as -1.  An
 *              expert of masks[t] that a row lacks drops out of that row's product; an absent row is never read.
 *   noise      dense [T, B, D], read at (t, b) (NULL: z = mu).  With draw != 0 it is WRITTEN instead: eps of (t, b, d)
 *              is element (t * B + b) * D + d of the stream mvae_philox_fill(seed, *counter_dev + counter_offset) would
 *              write -- the dense index, so a draw does not depend on which other rows are present and equals
 *              mvae_poe_fwd_draw's at full presence.  The counter is not advanced.
 *   bwd        dz / dmu / dlogvar [R, D] and dkl [R] (any may be NULL) -> the experts' compact gradient buffers
 *              [n_rows[e], ldg].  EVERY element is written: zero where no active term contains the expert on that
 *              row.  Fixed summation order, no atomics: the same bits every run.
 *   Refused (MVAE_ERR_ARG): E outside 1..MVAE_MAX_EXPERTS, T outside 1..40, B or D <= 0, ld or ldg < D, R < 0,
 *   n_rows[e] outside 0..B, a NULL table, a NULL head or gradient of an expert that has rows, draw without noise / z /
 *   counter.  R == 0 (forward) and no expert row at all (backward) launch nothing.
 * ------------------------------------------------------------------------------------ */
int mvae_poe_ragged_fwd(const mvae_experts_t *experts, int ld, int E, const int *n_rows, const int *erow_dev,
                        const uint32_t *masks_dev, int T, const int *slot_dev, int R,
                        float *noise /* nullable */, int draw, uint64_t seed, const uint64_t *counter_dev,
                        uint64_t counter_offset, float *mu, float *logvar, float *z /* nullable */,
                        float *kl /* nullable */, int B, int D, int variant, mvae_stream_t stream);
int mvae_poe_ragged_bwd(const mvae_experts_t *experts, int ld, int E, const int *n_rows, const int *erow_dev,
                        const uint32_t *masks_dev, int T, const int *slot_dev, int R,
                        const float *noise, const float *mu, const float *logvar,
                        const float *dz, const float *dmu, const float *dlogvar, const float *dkl,
                        const mvae_expert_grads_t *grads, int ldg, int B, int D, int variant, mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * K30 The reconstruction row sums of K11 / K13 for compact logits rows that find their target through an index
 *     (csrc/loss_ragged.hip): logits [R, P] (BCE) or [R, K] (CE), targets in batch order -- float [B, P] or int64 [B] --
 *     and rowmap_dev int32 [R], the batch row of each logits row.
 *       row[r] = coef[r] * loss(logits[r, :], target[rowmap[r]])   (coef_dev [R], NULL: 1)
 *       dlogits[r, :] = coef[r] * d loss / d logits                (fwd: optional, in the same pass; bwd: drow_dev as coef)
 *     No gathered copy of the targets is made and a target row no logits row maps to is never read.  A rowmap entry
 *     outside 0..B-1, or a label outside 0..K-1, makes its row NaN and indexes nothing.  K <= 1024.
 * ------------------------------------------------------------------------------------ */
int mvae_bce_rows_indexed_fwd(const float *logits, const float *target, const int *rowmap_dev,
                              const float *coef_dev /* nullable */, float *rowsum, float *dlogits /* nullable */,
                              int R, int P, int B, mvae_stream_t stream);
int mvae_bce_rows_indexed_bwd(const float *logits, const float *target, const int *rowmap_dev,
                              const float *drow_dev /* nullable */, float *dlogits, int R, int P, int B,
                              mvae_stream_t stream);
int mvae_ce_rows_indexed_fwd(const float *logits, const int64_t *label, const int *rowmap_dev,
                             const float *coef_dev /* nullable */, float *row, float *dlogits /* nullable */,
                             int R, int K, int B, mvae_stream_t stream);
int mvae_ce_rows_indexed_bwd(const float *logits, const int64_t *label, const int *rowmap_dev,
                             const float *drow_dev /* nullable */, float *dlogits, int R, int K, int B,
                             mvae_stream_t stream);

/* ------------------------------------------------------------------------------------
 * C1  Gradient exchange of data-parallel replicas -- RCCL over xGMI.
 *     The reference has NO counterpart: it is single-process, single-device (no DataParallel, no
 *     torch.distributed anywhere; README.md:47 `CUDA_VISIBLE_DEVICES=0`).  What this replaces is what N
 *     independent copies of mnist/train.py:197-219 would have to add between `backward()` (:218) and
 *     `optimizer.step()` (:219): the average of every parameter's gradient over the replicas.
 *
 *   One process per GPU, one communicator per process.  Start-up: rank 0 calls mvae_comm_unique_id and hands the
 *   128 bytes to its peers over any host transport (a file, a socket, MPI, torch.distributed's store); every rank
 *   calls mvae_comm_init (collective: returns when all `world` ranks joined); mvae_comm_broadcast makes parameters
 *   and buffers equal.  Per step: after the last weight-gradient launch of a bucket (a contiguous fp32 range of the
 *   gradient arena) was enqueued on `stream`, mvae_comm_allreduce_async sums that range over the ranks IN PLACE on
 *   the communicator's own stream -- ordered after `stream`'s work so far, concurrent with what `stream` gets next --
 *   and returns a ticket; mvae_comm_wait(ticket, stream) makes `stream` wait for it (then: mvae_adam_apply on the
 *   range with grad_scale = 1 / world).  Enqueue-only, no host sync, and capturable: issued between
 *   hipStreamBeginCapture / EndCapture on `stream` the collectives become nodes of the step's hipGraph (the
 *   communicator's stream forks from and joins back into the capturing stream -- every ticket must be waited on
 *   before EndCapture).  RCCL is dlopen-ed on first use: mvae_comm_use_library(path) > $MVAE_RCCL_LIB >
 *   "librccl.so.1" on the loader path.  At most 16 tickets may be outstanding; tickets are per communicator.
 *   Returns MVAE_OK / MVAE_ERR_ARG / MVAE_ERR_COMM (text: mvae_comm_last_error).
 * ------------------------------------------------------------------------------------ */
#define MVAE_COMM_ID_BYTES 128
typedef struct mvae_comm mvae_comm_t;
int mvae_comm_use_library(const char *librccl_path);         /* before first use; MVAE_ERR_ARG once another one is bound */
int mvae_comm_rccl_version(void);                            /* RCCL's version code (e.g. 22606), or MVAE_ERR_COMM */
int mvae_comm_unique_id(void *id_out, size_t id_bytes);      /* id_bytes >= MVAE_COMM_ID_BYTES */
int mvae_comm_init(mvae_comm_t **comm, const void *id, size_t id_bytes, int rank, int world, int device);
int mvae_comm_rank(const mvae_comm_t *comm);
int mvae_comm_world(const mvae_comm_t *comm);
const char *mvae_comm_last_error(const mvae_comm_t *comm);
int mvae_comm_broadcast(mvae_comm_t *comm, void *buf, size_t bytes, int root, mvae_stream_t stream);
int mvae_comm_allreduce_async(mvae_comm_t *comm, float *buf, size_t count, mvae_stream_t stream, int *ticket);
int mvae_comm_wait(mvae_comm_t *comm, int ticket /* < 0: everything issued so far */, mvae_stream_t stream);
/* Failure detection (ABI 5).  mvae_comm_async_error: MVAE_ERR_COMM once a collective of this communicator has failed
 * asynchronously (ncclCommGetAsyncError; MVAE_OK when the bound library has no such entry).  mvae_comm_synchronize is
 * the watchdog a host puts where it would otherwise call hipStreamSynchronize: it blocks until everything enqueued
 * on `stream` so far -- after mvae_comm_wait that includes the collectives -- has finished, for at most timeout_ms,
 * polling the asynchronous error state meanwhile; MVAE_ERR_COMM = a peer failed or the budget ran out (the
 * collective of a dead peer never completes), after which the communicator must be abandoned.  Not capturable. */
int mvae_comm_async_error(mvae_comm_t *comm);
int mvae_comm_synchronize(mvae_comm_t *comm, mvae_stream_t stream, int timeout_ms);
int mvae_comm_destroy(mvae_comm_t *comm);

#ifdef MVAE_TUNING
/* ------------------------------------------------------------------------------------
 * Tuning overrides -- libmvae_hip_tuning.so only (the same sources built with -DMVAE_TUNING).
 * Process-global, not thread-safe, not part of the product ABI.
 * ---------------------------------------------------------------------------------- */
/* force the per-wave tile (wm, wn in {1,2}: 64/128 rows/cols per block) and the number of reduction
 * splits of every subsequent GEMM-shaped launch; 0 = automatic; splits < 0: forward forms never split */
void mvae_debug_set_tiling(int wm, int wn, int splits);
/* force the number of k-wave groups (1, 2, 4) of 64x64-tile launches; 0 = automatic */
void mvae_debug_set_kwaves(int kw);
/* off != 0: never use the small (64x32 / 32x64 / 32x32, BK = 64) Linear layouts; waves in {4, 8}: force
 * their block size; 0 = automatic */
void mvae_debug_set_small(int off, int waves);
/* blocks a split reduction aims for; 0 = automatic */
void mvae_debug_set_split_target(long blocks);
/* knock-out study of the direct Linear weight-gradient kernel: 1 = loads without MFMAs, 2 = MFMAs without
 * loads (results are then meaningless); 0 = normal */
void mvae_debug_set_knockout(int mode);
#endif

#ifdef __cplusplus
}
#endif
#endif /* MVAE_HIP_H */
