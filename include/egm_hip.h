/*
 * egm_hip.h — C ABI of libegm_hip.so, the MI355X (gfx950) implementation of the
 * EGM-UNet segmentation training hot path.
 *
 * The reference (feiyeha/EGM-Unet) is pure PyTorch Python and has no FFI of its
 * own: the drop-in boundary is the nn.Module forward()/state_dict() surface
 * (src/unet.py:61-96, src/EGM-UNet.py:1503-1541) and the train_utils entry
 * points (train_utils/train_and_eval.py:7-100).  The host-side mirror of that
 * surface lives in egm_unet_amd/ (Python, like the reference); every arithmetic
 * step it performs goes through the entry points declared here.  Each entry
 * point cites the reference computation it replaces.
 *
 * Conventions
 *  - plain C: caller-owned DEVICE pointers, sizes as int / long long, an explicit
 *    hipStream_t (passed as void*).  No allocation, no synchronisation inside.
 *  - return 0 on success, negative egm_status otherwise; egm_last_error() gives
 *    the message (thread-local).
 *  - activations are NHWC ("pixel-major"): element (n,y,x,c) of a tensor with
 *    pixel stride `ld` (in elements, >= C, multiple of 8) lives at
 *    base[((n*H + y)*W + x)*ld + c].  A channel slice of a wider buffer is the
 *    same thing with an offset base pointer, so concatenations are never copied.
 *  - `dtype` selects the activation storage type: EGM_F32 (parity path) or
 *    EGM_BF16 (throughput path).  All accumulation is fp32.  Parameters,
 *    statistics, gradients of parameters and optimizer state are always fp32.
 *  - channel counts of activation tensors are multiples of 8 (callers pad with
 *    zero channels; packers zero the matching weights).
 */
#ifndef EGM_HIP_H
#define EGM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* egm_stream_t; /* hipStream_t */

enum egm_status { EGM_OK = 0, EGM_ERR_ARG = -1, EGM_ERR_LAUNCH = -2, EGM_ERR_UNSUPPORTED = -3 };
enum egm_dtype { EGM_F32 = 0, EGM_BF16 = 1 };
enum egm_act { EGM_ACT_NONE = 0, EGM_ACT_RELU = 1, EGM_ACT_SIGMOID = 2, EGM_ACT_SILU = 3 /* x*sigmoid(x): Conv, src/EGM-UNet.py:25-43 */ };

int egm_version(void);
const char* egm_last_error(void);
/* 1 when the current HIP device is gfx950; 0 otherwise (message set). */
int egm_device_ok(void);

/* ---- layout conversion at the module boundary ------------------------------------------------
 * image  [N,C,H,W] fp32 -> NHWC dtype with ld channels (channels C..ld-1 zero-filled);
 * logits NHWC dtype -> [N,C,H,W] fp32.  (model(image)["out"], train_and_eval.py:58) */
int egm_nchw_to_nhwc(int dtype, const void* src_f32, void* dst, int ld, int N, int C, int H, int W, egm_stream_t s);
int egm_nhwc_to_nchw(int dtype, const void* src, int ld, void* dst_f32, int N, int C, int H, int W, egm_stream_t s);

/* ---- convolution (nn.Conv2d stride 1, 'same' padding = dil*(k-1)/2; src/EGM-UNet.py:49,893,964,1210-1218) ---- */
/* Pack fp32 OIHW weights [Cout][Cin/groups][KH][KW] into the two dense operand layouts the kernels read:
 *   wf [KH*KW][CoutP][CinP]  (forward;  CoutP/CinP = Cout/Cin rounded up to 8, block-diagonal for groups>1)
 *   wd [KH*KW][CinP][CoutP]  (data gradient: taps flipped, in/out swapped).  Either output may be NULL.
 * bf16 3x3 images whose CoutP and CinP are multiples of 16 are stored chunk-major instead, [tap][CinP/16][CoutP][16] (wd:
 * [tap][CoutP/16][CinP][16]): same size, the 16-channel weight slab of a cout tile is contiguous per tap, which is what the LDS-DMA
 * staging of the 3x3 kernel reads.  The layout is a function of (dtype, KH, KW, CinP, CoutP) alone; egm_conv_fwd derives it from its
 * own arguments, callers never see it. */
int egm_conv_pack(int dtype, const void* w_oihw_f32, void* wf, void* wd, int Cout, int Cin, int KH, int KW, int groups,
                  egm_stream_t s);
/* Every conv weight of a model in one launch.  table_dev: device array of 120-byte entries
 * {const float* w; void* wf; void* wd; const float* w5, *w3, *b7, *b5, *b3; float* out; float* bout;
 *  int Cout, Cin, CoutP, CinP, KH, KW, groups, chunk0, kind, pad;}; an entry takes
 * ceil(KH*KW*CoutP*CinP / egm_conv_pack_chunk()) workgroups ("chunks"), chunk0 = the sum of the chunk counts of the entries before
 * it (the kernels of all *_multi entry points find their entry by binary search on chunk0), total_chunks = the sum over all.
 * kind 0: egm_conv_pack of the parameter w (the other pointers unused).  The derived FusionConv weights, built from their real
 * parameters by the same launch, bit for bit what egm_fold2_pack / egm_merge357_pack write:
 * kind 1 (fold2, KH = KW = groups = 1): w = the real [Cout][2*Cin] weight, out = fp32 [Cout][Cin];
 * kind 2 (merge357, KH = KW = 7, groups = 1): w / w5 / w3 = the 7x7 / 5x5 / 3x3 weights, b7 / b5 / b3 their biases, out = fp32
 * [Cout][Cin][7][7], bout = fp32 [Cout]. */
int egm_conv_pack_chunk(void);
int egm_conv_pack_multi(int dtype, const void* table_dev, int n, long long total_chunks, egm_stream_t s);
/* Launch groups: between egm_group_begin() and egm_group_end(s) the egm_conv_fwd* calls of THIS host thread are recorded instead of
 * launched; egm_group_end launches them, merging those that run the same kernel instantiation into one launch (up to 4 members; the
 * parallel branches of EdgeEnhancedGRFB, src/EGM-UNet.py:1256-1278).  The recorded convolutions must be independent of each other
 * and their outputs must not be used before egm_group_end.  Convolutions taking a kernel without a merged form are launched at once.
 * egm_group_abort() drops an open group (error paths). */
int egm_group_begin(void);
int egm_group_end(egm_stream_t s);
int egm_group_abort(void);
/* 3x3 kernel selection, a bit mask (default 5; env EGM_CONV_TILE): 1 = the 8-wave LDS-DMA tile kernel wherever its >= 64-cout tiles
 * fill the chip, 2 = its 32-cout tiles too (measured slower than the 4-wave kernel: parity tests and A/B runs only), 4 = the
 * weights-in-registers kernel for the 32 -> 32 layers; 0 = the 4-wave register-staged kernel everywhere; -1 = query only.
 * Returns the previous mode (A/B timing and parity tests). */
int egm_conv_tile_mode(int mode);
/* Diagnostics only (tools/conv_tile_diag.py): phase-elimination switches of the tile kernel, OR of 1 = no LDS-DMA, 2 = no MFMA phase,
 * 4 = no epilogue; outputs are wrong while any is set.  -1 = query.  Returns the previous value; 0 in production. */
int egm_conv_tile_debug(int dbg);
/* 7x7 kernel selection for 16 -> 16 channels (FusionConv's merged 3x3+5x5+7x7 conv at the 64-channel level, src/EGM-UNet.py:1210-1228):
 * 1 = the weights-in-registers v_mfma_f32_16x16x32_bf16 kernel (csrc/conv7x7_c16.hip; default, env EGM_CONV_C7), 0 = the generic
 * pipelined kernel, -1 = query only.  Returns the previous mode (A/B timing and parity tests). */
int egm_conv_c7_mode(int mode);
/* egm_conv_fwd with the output channels written to TWO tensors: couts [0, csplit) to y (pixel stride ldy), [csplit, Cout) to y2
 * (pixel stride ldy2).  The data gradient of the conv behind a channel concatenation (Up, src/EGM-UNet.py:947-949) written as the
 * gradients of the two concatenated tensors, each dense, instead of one interleaved tensor whose halves the consumers read as half
 * cache lines.  No bias, no statistics.  Supported where egm_conv_split_ok() says so (the 8-wave 3x3 kernel, csplit % 8 == 0). */
int egm_conv_split_ok(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, int csplit);
int egm_conv_fwd_split(int dtype, const void* x, int ldx, const void* wf, void* y, int ldy, void* y2, int ldy2, int csplit, int N,
                       int H, int W, int Cin, int Cout, int KH, int KW, int dil, egm_stream_t s);
/* Name of the kernel egm_conv_fwd launches for a shape, spelled like the rows of a rocprofv3 kernel trace (e.g.
 * "conv_igemm_pipe_kernel<2, 3, 3, 2>"); returns its length, copies at most buflen-1 characters into buf (may be NULL). */
int egm_conv_kernel_name(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, char* buf, int buflen);
/* y = conv(x, wf) (+bias).  Cin/Cout are the PADDED counts of wf.  bias (fp32, bias_n <= Cout valid entries; the rest count as 0) may be NULL.
 * stats, when non-NULL, receives per-pixel-tile partial sums [ntiles][2][Cout] of y and y*y
 * (consumed by egm_bn_finalize); egm_conv_stats_tiles() gives ntiles for the same dtype/shape/kernel.
 * The data gradient is the same call on dy with wd (Cin/Cout swapped). */
int egm_conv_fwd(int dtype, const void* x, int ldx, const void* wf, const void* bias_f32, int bias_n, void* y, int ldy,
                 float* stats, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, egm_stream_t s);
int egm_conv_stats_tiles(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil);
/* egm_conv_fwd without statistics, with act (enum egm_act) applied in the epilogue after the bias, before the one rounding to `dtype`:
 * y = act(conv(x, wf) + bias).  The eval-mode conv -> BatchNorm -> activation of egm_unet_amd/infer.py, with wf / bias from
 * egm_conv_fold_pack_multi.  Same plan, kernel family, launch groups and ldy (concat slots) as egm_conv_fwd; act = NONE is
 * egm_conv_fwd with stats = NULL. */
int egm_conv_fwd_act(int dtype, const void* x, int ldx, const void* wf, const void* bias_f32, int bias_n, void* y, int ldy, int N, int H,
                     int W, int Cin, int Cout, int KH, int KW, int dil, int act, egm_stream_t s);
/* BatchNorm folded into the conv in front of it, every conv -> BatchNorm pair of a model in one launch (csrc/infer.hip).  table_dev:
 * device array of 104-byte entries {const float* w, *b, *gamma, *beta, *running_mean, *running_var; void* wf; float* bias; float eps;
 * int Cout, Cin, CoutP, CinP, KH, KW, groups, chunk0, pad;}; b, gamma, beta may be NULL (0, 1, 0).  With s = gamma / sqrt(running_var
 * + eps): wf = egm_conv_pack's forward pack of w*s (fp32 product, one rounding to `dtype`), bias [CoutP] fp32 = (b - running_mean)*s
 * + beta, padded channels 0.  Chunks of egm_conv_fold_chunk() elements per workgroup; chunk0 / total_chunks as for egm_conv_pack_multi. */
int egm_conv_fold_chunk(void);
int egm_conv_fold_pack_multi(int dtype, const void* table_dev, int n, long long total_chunks, egm_stream_t s);
/* out[n][h][w] = lut[argmax_c logits[n][c][h][w]] (lut NULL: the index itself); logits fp32 NCHW, C <= 256, ties to the lowest index as
 * torch.argmax (predict.py's mask and its color_map). */
int egm_argmax_u8(const float* logits, const unsigned char* lut, unsigned char* out, int N, int C, int H, int W, egm_stream_t s);
/* Weight gradient: dw_oihw_f32 [CoutR][CinR/groups][KH][KW] (+)= sum_pixels dy (x) x.
 * Cin/Cout are padded counts of the activation buffers, CinR/CoutR the real (unpadded) ones.
 * workspace: egm_conv_wgrad_workspace() bytes.  accumulate != 0 adds to dw. */
long long egm_conv_wgrad_workspace(int N, int H, int W, int Cin, int Cout, int KH, int KW);
int egm_conv_wgrad(int dtype, const void* x, int ldx, const void* dy, int lddy, float* dw_oihw_f32, void* workspace,
                   int N, int H, int W, int Cin, int Cout, int CinR, int CoutR, int KH, int KW, int dil, int groups,
                   int accumulate, egm_stream_t s);
/* Deferred form: egm_conv_wgrad with dw == NULL writes only the partial slabs (egm_conv_wgrad_slabs() of them) into the
 * workspace; egm_wgrad_reduce_multi() then finishes MANY convolutions in one launch.  table_dev: device array of 72-byte
 * entries {const float* slab; float* dw; float* dw2; float* dw3; int nslab, taps, CoutP, CinP, CoutR, CinR, groups, accumulate,
 * chunk0, mode;}; chunks per entry = ceil(taps*CoutP*CinP / egm_wgrad_reduce_chunk()), chunk0 / total_chunks as for
 * egm_conv_pack_multi.  mode & 3 = where a reduced element goes:
 *   0  dw, the fp32 OIHW gradient (dw2, dw3 unused);
 *   1  fold2: the reduced [CoutR][CinR] 1x1 gradient belongs to a weight derived as W[:, :K] + W[:, K:]; dw is the gradient of the
 *      real [CoutR][2*CinR] parameter and receives every element twice, at [co][ci] and [co][CinR + ci] (egm_fold2_bwd's result);
 *   2  merge357: the reduced 7x7 gradient (taps = 49, groups = 1) goes to dw (the 7x7 parameter's gradient) and, where the tap lies in
 *      the centre 5x5 / 3x3 window, to dw2 / dw3 (the 5x5 / 3x3 parameters', egm_merge357_bwd's result); a NULL destination is skipped.
 * accumulate applies to mode 0 only.  mode & 4: the entry is summed in the order of egm_wgrad_reduce's kernel for many slabs of a
 * small gradient (egm_wgrad_reduce_is_wide() tells when egm_wgrad_reduce takes it) and takes chunks of egm_wgrad_reduce_chunk_wide()
 * elements; without the bit the order is that of egm_wgrad_reduce's other kernel.  Each slab element is read once either way. */
int egm_conv_wgrad_kernel_name(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil, char* buf, int buflen);   /* as egm_conv_kernel_name */
/* egm_conv_wgrad's slab-only form (dw == NULL) for 1..EGM_WGRAD_MULTI_MAX independent convolutions in one call: members that take the
 * same kernel instantiation (egm_conv_wgrad_kernel_name) run as ONE launch.  Arguments per member as egm_conv_wgrad's; slabs =
 * its workspace.  (The reference has no counterpart: torch.autograd launches cudnn's weight-gradient kernel per conv, train_utils'
 * loss.backward(); here the slabs of a backward pass have no reader before egm_wgrad_reduce_multi, so their launches can wait.) */
#define EGM_WGRAD_MULTI_MAX 4
typedef struct egm_conv_wgrad_desc {
    const void* x; const void* dy; void* slabs;
    int ldx, lddy, N, H, W, Cin, Cout, Cin_real, Cout_real, KH, KW, dil, groups, pad_;
} egm_conv_wgrad_desc;
int egm_conv_wgrad_multi(int dtype, const egm_conv_wgrad_desc* descs, int n, egm_stream_t stream);
int egm_conv_wgrad_slabs(int dtype, int N, int H, int W, int Cin, int Cout, int KH, int KW, int dil);
/* The reduction of ONE convolution's slabs, at once (what egm_conv_wgrad with dw != NULL runs behind its slab kernel). */
int egm_wgrad_reduce(const float* slabs, float* dw_oihw_f32, int nslab, int taps, int CoutP, int CinP, int CoutR, int CinR, int groups,
                     int accumulate, egm_stream_t s);
int egm_wgrad_reduce_chunk(void);   /* packed elements reduced by one workgroup of egm_wgrad_reduce_multi */
int egm_wgrad_reduce_chunk_wide(void);   /* ... of an entry with mode & 4 */
int egm_wgrad_reduce_is_wide(int nslab, int taps, int CoutP, int CinP);   /* 1 when egm_wgrad_reduce sums these slabs with its many-slab kernel */
int egm_wgrad_reduce_multi(const void* table_dev, int n, long long total_chunks, egm_stream_t s);
/* Depthwise 3x3 (RecursiveGatedAttention.dwconv, src/EGM-UNet.py:507-509): y = (dw3x3(x, w) + b) * scale.
 * w fp32 [C][1][3][3], b fp32 [C], scale fp32 [1] (device). */
int egm_dwconv3_fwd(int dtype, const void* x, int ldx, const float* w, const float* b, const float* scale, void* y, int ldy,
                    int N, int H, int W, int C, egm_stream_t s);
/* dx, dw, db, dscale of the above.  partial: fp32 scratch >= egm_dwconv3_bwd_workspace() bytes. */
long long egm_dwconv3_bwd_workspace(int N, int H, int W, int C);
int egm_dwconv3_bwd(int dtype, const void* x, int ldx, const void* dy, int lddy, const float* w, const float* b,
                    const float* scale, void* dx, int lddx, float* dw, float* db, float* dscale, void* workspace,
                    int N, int H, int W, int C, egm_stream_t s);

/* ---- per-channel reductions ------------------------------------------------------------------
 * Two-stage, deterministic: stage 1 writes per-block partial "tiles" [nblk][2][C] (sum, sum of squares) with
 * nblk = egm_channel_partials_blocks(npix, C); egm_reduce_tiles() (or egm_bn_finalize) sums tiles in fixed order
 * in double.  Used for bias gradients and for BN statistics of tensors not produced by egm_conv_fwd. */
int egm_channel_partials_blocks(long long npix, int C);
int egm_channel_sums(int dtype, const void* x, int ld, long long npix, int C, float* partials, egm_stream_t s);
int egm_reduce_tiles(const float* tiles, int ntiles, int C, float* out_2xC, egm_stream_t s);
/* batch independent reductions: tiles [batch][ntiles][2][C] -> out [batch][2][C] */
int egm_reduce_tiles_batched(const float* tiles, int batch, int ntiles, int C, float* out, egm_stream_t s);
/* The bias gradients (db[c] = sum over pixels of dy[., c]) of up to a whole backward pass in two launches; bit-identical, per tensor, to
 * egm_channel_sums + egm_reduce_tiles (same blocks, same order).  Replaces the per-layer bias reduction autograd performs for the
 * nn.Conv2d(bias=True) layers of src/EGM-UNet.py:1256-1313, 1362-1390, 1499 (torch: grad_bias = dy.sum((0, 2, 3))).
 * table_dev: device array of 2n egm_bsum_entry; [0, n): chunk0 = index of the tensor's first partial-sum block (nblk =
 * egm_channel_partials_blocks(npix, C) blocks each, blocks1 in all); [n, 2n): the same tensors with chunk0 = index of the first
 * reduction block (C / 8 each, blocks2 in all).  part = nblk * 2 * C floats of workspace, out = Cout floats (c < Cout <= C written). */
typedef struct { const void* x; float* part; float* out; long long npix; int ld, C, Cout, nblk, chunk0, pad; } egm_bsum_entry;
int egm_bias_grad_multi(int dtype, const void* table_dev, int n, long long blocks1, long long blocks2, egm_stream_t s);

/* ---- BatchNorm2d (train-mode batch statistics / eval-mode running statistics) + activation -----
 * (nn.BatchNorm2d + ReLU/Sigmoid: src/EGM-UNet.py:50-51,878-879,966-973) */
/* stats tiles [ntiles][2][C] -> mean/var; writes scale=gamma*rstd, shift=beta-mean*scale, save_mean, save_rstd (fp32 [C]);
 * when running_mean != NULL updates running stats with `momentum` (unbiased variance, as torch).
 * gamma/beta/running_* hold C_real entries; channels C_real..C-1 (zero padding) get scale = shift = 0. */
int egm_bn_finalize(const float* stats, int ntiles, long long count, const float* gamma, const float* beta, float eps,
                    float momentum, float* running_mean, float* running_var, float* scale, float* shift,
                    float* save_mean, float* save_rstd, int C, int C_real, egm_stream_t s);
/* eval mode: scale/shift (and save_mean/save_rstd when non-NULL) from running statistics. */
int egm_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float eps, float* scale, float* shift, float* save_mean, float* save_rstd, int C, int C_real,
                       egm_stream_t s);
/* z = act(y*scale + shift) */
int egm_bn_act_fwd(int dtype, const void* y, int ldy, const float* scale, const float* shift, int act, void* z, int ldz,
                   long long npix, int C, egm_stream_t s);
/* Backward of z = act(BN(y)), dzp = dz*act'(y*scale+shift), xhat = (y-mean)*rstd:
 *   reduce: partial tiles [nblk][2][C] of (sum dzp, sum dzp*xhat)  -> egm_reduce_tiles -> sums [2][C]
 *           (sums[0] is dbeta, sums[1] is dgamma)
 *   apply : train != 0: dy = scale*(dzp - sums[0]/npix - xhat*sums[1]/npix);  train == 0: dy = scale*dzp */
int egm_bn_act_bwd_reduce(int dtype, const void* dz, int lddz, const void* y, int ldy, const float* scale,
                          const float* shift, const float* save_mean, const float* save_rstd, int act, float* partials,
                          long long npix, int C, egm_stream_t s);
int egm_bn_act_bwd_apply(int dtype, const void* dz, int lddz, const void* y, int ldy, const float* scale,
                         const float* shift, const float* save_mean, const float* save_rstd, int act, int train,
                         const float* sums, void* dy, int lddy, long long npix, int C, egm_stream_t s);
/* BatchNorm backward with dz computed on the fly from its producer (csrc/bn_dz_fused.hip), the two passes of egm_bn_act_bwd_reduce /
 * egm_bn_act_bwd_apply (same partials geometry: egm_channel_partials_blocks(npix, C) blocks; C/8 must divide 256):
 *   _cls_: dz[p][c] = sum_{k < nc} dlogits[p][k]*w_cls[k*ldw + c] -- the data gradient of the 1x1 classifier behind the last
 *          BatchNorm+ReLU (OutConv, src/EGM-UNet.py:952-956): its conv launch and the tensor it wrote do not exist.  nc <= 8; w_cls is the
 *          fp32 OIHW weight [nc][ldw] (rounded to `dtype` inside, like the conv's operand pack); dlogits has >= 8 channels per pixel.
 *   _mca_: dz = dxo*(g_h + g_w + g_c)*inv + (A + B*x) -- the MCALayer's last backward step (egm_mca_bwd_dx) behind DoubleConv1's first
 *          BatchNorm+ReLU (src/EGM-UNet.py:893-896), x being this BatchNorm's own output, recomputed from y. */
/* Forward twin of _cls_: z = act(y*scale + shift) written to z AND the classifier applied in the same pass,
 * logits_nchw[n][k][h][w] (fp32, the module's output layout) = sum_c z[c]*w_cls[k*ldw + c] + bias[k], rounded to `dtype` like the conv
 * kernel's output (egm_bn_act_fwd + the 1x1 conv launch + egm_nhwc_to_nchw as one pass).  nc <= 8, C/8 a power of two <= 64. */
int egm_bn_act_cls_fwd(int dtype, const void* y, int ldy, const float* scale, const float* shift, int act, void* z, int ldz,
                       const float* w_cls, int nc, int ldw, const float* bias, float* logits_nchw, int N, int H, int W, int C,
                       egm_stream_t s);
int egm_bn_cls_bwd_reduce(int dtype, const void* dlogits, int lddl, const float* w_cls, int nc, int ldw, const void* y, int ldy,
                          const float* scale, const float* shift, const float* save_mean, const float* save_rstd, int act,
                          float* partials, long long npix, int C, egm_stream_t s);
int egm_bn_cls_bwd_apply(int dtype, const void* dlogits, int lddl, const float* w_cls, int nc, int ldw, const void* y, int ldy,
                         const float* scale, const float* shift, const float* save_mean, const float* save_rstd, int act, int train,
                         const float* sums, void* dy, int lddy, long long npix, int C, egm_stream_t s);
int egm_bn_mca_bwd_reduce(int dtype, const void* dxo, int ldd, const float* gates, const float* coef, int no_spatial, const void* y,
                          int ldy, const float* scale, const float* shift, const float* save_mean, const float* save_rstd, int act,
                          float* partials, int N, int H, int W, int C, egm_stream_t s);
int egm_bn_mca_bwd_apply(int dtype, const void* dxo, int ldd, const float* gates, const float* coef, int no_spatial, const void* y,
                         int ldy, const float* scale, const float* shift, const float* save_mean, const float* save_rstd, int act,
                         int train, const float* sums, void* dy, int lddy, int N, int H, int W, int C, egm_stream_t s);
/* Second stage of the BatchNorm backward: partial tiles of egm_bn_act_bwd_reduce -> sums [2][C] (dbeta | dgamma) and
 * cf [4][C] = scale | shift | cb | cc with dy = scale*dzp + cb + cc*y (what the fused apply passes read). */
int egm_bn_bwd_coefs(const float* partials, int ntiles, long long count, const float* scale, const float* shift,
                     const float* save_mean, const float* save_rstd, int train, float* sums_2xC, float* cf_4xC, int C,
                     egm_stream_t s);

/* Multi-tensor forms: the BatchNorm passes of up to EGM_BN_MULTI_MAX INDEPENDENT layers in one launch each (the parallel branches of
 * EdgeEnhancedGRFB, src/EGM-UNet.py:1256-1278, work on 8-32 channel tensors whose passes are launch-latency bound).  `descs` is a HOST
 * array (it is copied into the kernel argument); every pass reads the fields it needs and ignores the others; coef = [4][C] rows
 * scale | shift | save_mean | save_rstd.  Same arithmetic and block decomposition per tensor as the single-tensor entry points. */
#define EGM_BN_MULTI_MAX 4
enum egm_bn_multi_pass { EGM_BN_MULTI_FINALIZE = 0, EGM_BN_MULTI_FWD = 1, EGM_BN_MULTI_BWD_REDUCE = 2, EGM_BN_MULTI_BWD_COEFS = 3,
                         EGM_BN_MULTI_BWD_APPLY = 4 };
typedef struct egm_bn_desc {
    const void* y;  void* z;  const void* dz;  void* dy;        /* BatchNorm input, output, gradient of the output, of the input */
    float* coef;                                                  /* [4][C] */
    const float* stats;                                           /* finalize: conv partial tiles [ntiles][2][C] */
    const float* gamma;  const float* beta;  float* running_mean;  float* running_var;
    float* partials;  float* sums;  float* cf4;                   /* backward: [nblocks][2][C], [2][C], [4][C] */
    long long npix;
    int ldy, ldz, lddz, lddy, ntiles, nblocks, C, C_real, act, train;
    float eps, momentum;
} egm_bn_desc;
int egm_bn_multi(int dtype, int pass, const egm_bn_desc* descs, int n, egm_stream_t s);

/* BatchNorm(+act) fused with the element-wise op behind it (z and dz never reach memory; same rounding points as the unfused
 * chain, so results agree bit for bit):
 *   EGM_EW_GATE  out = p*(1 + z)          EdgeAwareFeatureEnhancer, src/EGM-UNet.py:884-886 (z = sigmoid(BN(y)))
 *   EGM_EW_SAR   out = relu(alpha*p + z)  EdgeEnhancedGRFB residual tail, :1315-1317 (z = BN(y) of the shortcut, p = fusion output)
 * fwd: reads y, p, writes out.  bwd_reduce: partial tiles [egm_channel_partials_blocks][2][C] of the BatchNorm backward sums, from
 * g (= dL/dout), q (GATE: p; SAR: out, for the ReLU mask) and y.  bwd_apply (cf from egm_bn_bwd_coefs): writes dy (gradient of the
 * BatchNorm input) and dp. */
enum egm_ew_mode { EGM_EW_GATE = 0, EGM_EW_SAR = 1 };
int egm_bn_ew_fwd(int dtype, int mode, const void* y, int ldy, const float* scale, const float* shift, int act, const void* p,
                  int ldp, float alpha, void* out, int ldo, long long npix, int C, egm_stream_t s);
int egm_bn_ew_bwd_reduce(int dtype, int mode, const void* g, int ldg, const void* q, int ldq, const void* y, int ldy,
                         const float* scale, const float* shift, const float* save_mean, const float* save_rstd, int act,
                         float alpha, float* partials, long long npix, int C, egm_stream_t s);
int egm_bn_ew_bwd_apply(int dtype, int mode, const void* g, int ldg, const void* q, int ldq, const void* y, int ldy,
                        const float* cf_4xC, int act, float alpha, void* dy, int lddy, void* dp, int lddp, long long npix, int C,
                        egm_stream_t s);

/* Backward of a 1x1 convolution (groups 1) in ONE pass over dy and x (csrc/conv1x1_bwd.hip): dx = dy . W (data gradient, may be NULL) and
 * the weight-gradient slabs [egm_conv1x1_bwd_slabs(npix)][CoutP][CinP] fp32, laid out like egm_conv_wgrad's workspace (taps = 1) so that
 * egm_wgrad_reduce_multi / egm_conv_wgrad's own reduction sum them.  wd = egm_conv_pack's wd [CinP][CoutP] in `dtype`; Cin, Cout are the
 * PADDED channel counts (<= 128).  Replaces the egm_conv_fwd(dy, wd) + egm_conv_wgrad pair of BasicConv(k = 1) and friends
 * (src/EGM-UNet.py:958-975, 1210-1218).  Up to 4 convolutions per call (one launch). */
typedef struct egm_conv1x1_bwd_desc {
    const void* x;  const void* dy;  const void* wd;  void* dx;  float* slabs;
    long long npix;
    int ldx, lddy, lddx, Cin, Cout, pad_;
} egm_conv1x1_bwd_desc;
int egm_conv1x1_bwd_supported(int dtype, int Cin, int Cout);
int egm_conv1x1_bwd_slabs(long long npix);
int egm_conv1x1_bwd(int dtype, const egm_conv1x1_bwd_desc* descs, int n, egm_stream_t s);

/* ---- pooling / resampling --------------------------------------------------------------------- */
/* nn.MaxPool2d(2,2) (src/EGM-UNet.py:908); H, W are the INPUT sizes (even). */
int egm_maxpool2_fwd(int dtype, const void* x, int ldx, void* y, int ldy, int N, int H, int W, int C, egm_stream_t s);
int egm_maxpool2_bwd(int dtype, const void* x, int ldx, const void* dy, int lddy, void* dx, int lddx, int N, int H, int W,
                     int C, egm_stream_t s);
/* egm_maxpool2_bwd with a second gradient of x summed in the same pass: dx = scatter(dy) + add (even H, W). */
int egm_maxpool2_bwd_add(int dtype, const void* x, int ldx, const void* dy, int lddy, const void* add, int ldadd, void* dx, int lddx,
                         int N, int H, int W, int C, egm_stream_t s);
/* The max pool at an encoder skip connection fused into its neighbours (csrc/pool_fused.hip; src/EGM-UNet.py:908 behind :44-55 at the
 * top level and behind the EdgeEnhancedGRFB target gate :1319-1321 below it).  H, W = the full-resolution sizes, both even.
 *   egm_bn_act_fwd_pool   : z = act(y*scale + shift) AND pooled = maxpool2(z)                      (egm_bn_act_fwd + egm_maxpool2_fwd)
 *   egm_bn_pool_bwd_reduce: egm_bn_act_bwd_reduce with dz = gskip + scatter(gpool) computed on the fly (egm_maxpool2_bwd_add never runs);
 *                           partials [egm_bn_pool_bwd_blocks()][2][C]
 *   egm_bn_pool_bwd_apply : egm_bn_act_bwd_apply with the same on-the-fly dz
 *   egm_gate3_fwd_pool    : out = x*(1 + mean_k sigmoid(t[k])) AND pooled = maxpool2(out)           (egm_gate3_fwd + egm_maxpool2_fwd)
 *   egm_gate3_pool_bwd    : egm_gate3_bwd with g = gskip + scatter(gpool) computed on the fly */
int egm_bn_act_fwd_pool(int dtype, const void* y, int ldy, const float* scale, const float* shift, int act, void* z, int ldz,
                        void* pooled, int ldp, int N, int H, int W, int C, egm_stream_t s);
int egm_bn_pool_bwd_blocks(int N, int H, int W, int C);
int egm_bn_pool_bwd_reduce(int dtype, const void* gskip, int ldgs, const void* gpool, int ldgp, const void* y, int ldy,
                           const float* scale, const float* shift, const float* save_mean, const float* save_rstd, int act,
                           float* partials, int N, int H, int W, int C, egm_stream_t s);
int egm_bn_pool_bwd_apply(int dtype, const void* gskip, int ldgs, const void* gpool, int ldgp, const void* y, int ldy,
                          const float* scale, const float* shift, const float* save_mean, const float* save_rstd, int act, int train,
                          const float* sums, void* dy, int lddy, int N, int H, int W, int C, egm_stream_t s);
int egm_gate3_fwd_pool(int dtype, const void* x, int ldx, const void* t, int ldt, void* out, int ldo, void* pooled, int ldp, int N,
                       int H, int W, int C, egm_stream_t s);
int egm_gate3_pool_bwd(int dtype, const void* gskip, int ldgs, const void* gpool, int ldgp, const void* x, int ldx, const void* t,
                       int ldt, void* dx, int lddx, void* dt, int lddt, int N, int H, int W, int C, egm_stream_t s);
/* Up.forward front half (src/EGM-UNet.py:937-947): out = cat([skip, pad(bilinear_x2_align_corners(low))], C).
 * Writes BOTH halves of `out` (ld = ldo >= Cs + Cl): skip [N,Hs,Ws,Cs], low [N,Hl,Wl,Cl].
 * skip == NULL: the skip channels were produced straight into out[..., :Cs] by their own kernel; only the Cl upsampled channels are written. */
int egm_upcat_fwd(int dtype, const void* skip, int lds, const void* low, int ldl, void* out, int ldo, int N, int Hs, int Ws,
                  int Cs, int Hl, int Wl, int Cl, egm_stream_t s);
/* BatchNorm apply fused into the stencil behind it (csrc/bn_stencil_fused.hip; bf16 only, anything else is EGM_ERR_ARG: callers keep
 * the two-kernel path).  Bit-identical to the pairs they replace.
 *   egm_bn_act_hp_fwd   : z = act(y*scale + shift) written to z (ld = ldz >= C: may be a channel slot of a wider buffer) AND
 *                         edge = z - avgpool3x3(z) (zero pad, divisor 9)                             (egm_bn_act_fwd + egm_highpass3)
 *   egm_bn_act_upcat_fwd: egm_upcat_fwd of low = act(y_low*scale + shift), which is never written   (egm_bn_act_fwd + egm_upcat_fwd);
 *                         scale, shift, act belong to `low`; skip == NULL as for egm_upcat_fwd */
int egm_bn_act_hp_fwd(int dtype, const void* y, int ldy, const float* scale, const float* shift, int act, void* z, int ldz,
                      void* edge, int lde, int N, int H, int W, int C, egm_stream_t s);
int egm_bn_act_upcat_fwd(int dtype, const void* skip, int lds, const void* low, int ldl, const float* scale, const float* shift,
                         int act, void* out, int ldo, int N, int Hs, int Ws, int Cs, int Hl, int Wl, int Cl, egm_stream_t s);
/* dlow = transposed bilinear of dout[..., Cs:Cs+Cl]; (dskip is dout[..., :Cs], a view). */
int egm_upcat_bwd_low(int dtype, const void* dout, int ldo, void* dlow, int ldl, int N, int Hs, int Ws, int Cs, int Hl,
                      int Wl, int Cl, egm_stream_t s);

/* ---- generic fused elementwise helpers -------------------------------------------------------- */
/* out = alpha*a + beta*b (b may be NULL) */
int egm_axpby(int dtype, const void* a, int lda, float alpha, const void* b, int ldb, float beta, void* out, int ldo,
              long long npix, int C, egm_stream_t s);
/* out = a + b + c (+ d when non-NULL): gradient fan-in of a tensor with 3-4 consumers in one pass */
int egm_sum4(int dtype, const void* a, int lda, const void* b, int ldb, const void* c, int ldc, const void* d, int ldd, void* out,
             int ldo, long long npix, int C, egm_stream_t s);
/* out = highpass3(a) + b (+ c) (+ d) in one pass (c, d may be NULL): gradient fan-in when one consumer of the tensor was egm_highpass3
 * (the stencil is self-adjoint); highpass3(a) is rounded to the storage type before the sum, like the separate pass. */
int egm_sum4_hp(int dtype, const void* a, int lda, const void* b, int ldb, const void* c, int ldc, const void* d, int ldd, void* out,
                int ldo, int N, int H, int W, int C, egm_stream_t s);
/* fp32 vector add: y[i] += x[i] (parameter-gradient accumulation) */
int egm_vec_add_f32(float* y, const float* x, long long n, egm_stream_t s);
int egm_fill_f32(float* y, float v, long long n, egm_stream_t s);
/* fp32 matrix column block copy: dst[r][col0_dst + c] = src[r][col0_src + c], c < ncols (weight re-layout for inputs padded per tensor) */
int egm_copy_cols_f32(const float* src, int ld_src, int col0_src, float* dst, int ld_dst, int col0_dst, int rows, int ncols,
                      egm_stream_t s);

/* ---- EdgeAwareFeatureEnhancer pieces (src/EGM-UNet.py:872-886) -------------------------------------------------- */
/* out = x - avgpool3x3(x) (zero pad, divisor 9).  Self-adjoint: the same call is its own backward. */
int egm_highpass3(int dtype, const void* x, int ldx, void* out, int ldo, int N, int H, int W, int C, egm_stream_t s);
/* out = x*(1+w);  backward: dx = g*(1+w), dw = g*x */
int egm_gate_mul_fwd(int dtype, const void* x, int ldx, const void* w, int ldw, void* out, int ldo, long long npix, int C,
                     egm_stream_t s);
int egm_gate_mul_bwd(int dtype, const void* g, int ldg, const void* x, int ldx, const void* w, int ldw, void* dx, int lddx,
                     void* dw, int lddw, long long npix, int C, egm_stream_t s);

/* ---- EdgeEnhancedGRFB tail (src/EGM-UNet.py:1315-1321) ----------------------------------------------------------- */
/* out = relu(alpha*a + b);  backward (mask = out > 0): da = alpha*g*mask, db = g*mask */
int egm_scale_add_relu_fwd(int dtype, const void* a, int lda, float alpha, const void* b, int ldb, void* out, int ldo,
                           long long npix, int C, egm_stream_t s);
int egm_scale_add_relu_bwd(int dtype, const void* g, int ldg, const void* out, int ldo, float alpha, void* da, int ldda,
                           void* db, int lddb, long long npix, int C, egm_stream_t s);
/* out = x*(1 + mean_k sigmoid(t[..,k])), k<3 (t: 8-channel map, 3 real);  backward writes dx and dt (8 channels) */
int egm_gate3_fwd(int dtype, const void* x, int ldx, const void* t, int ldt, void* out, int ldo, long long npix, int C,
                  egm_stream_t s);
int egm_gate3_bwd(int dtype, const void* g, int ldg, const void* x, int ldx, const void* t, int ldt, void* dx, int lddx,
                  void* dt, int lddt, long long npix, int C, egm_stream_t s);

/* ---- RecursiveGatedAttention pieces (src/EGM-UNet.py:531-544) ---------------------------------------------------- */
/* out = a * sigmoid(gl[..,0]) (gl: 8-channel map, 1 real);  backward writes da and dgl (8 channels) */
int egm_bcast_gate_fwd(int dtype, const void* a, int lda, const void* gl, int ldgl, void* out, int ldo, long long npix, int C,
                       egm_stream_t s);
int egm_bcast_gate_bwd(int dtype, const void* g, int ldg, const void* a, int lda, const void* gl, int ldgl, void* da, int ldda,
                       void* dgl, int lddgl, long long npix, int C, egm_stream_t s);
/* nn.GELU (erf form) */
int egm_gelu_fwd(int dtype, const void* x, int ldx, void* out, int ldo, long long npix, int C, egm_stream_t s);
int egm_gelu_bwd(int dtype, const void* g, int ldg, const void* x, int ldx, void* dx, int lddx, long long npix, int C,
                 egm_stream_t s);

/* ---- FusionConv pieces (src/EGM-UNet.py:1171-1236) ---------------------------------------------------------------- */
/* SpatialAttentionModule input: out[..,0] = mean_c x, out[..,1] = max_c x over the C_real real channels (8-channel map) */
int egm_chan_meanmax_fwd(int dtype, const void* x, int ldx, void* out, int ldo, long long npix, int C, int C_real,
                         egm_stream_t s);
int egm_chan_meanmax_bwd(int dtype, const void* g, int ldg, const void* x, int ldx, void* dx, int lddx, long long npix, int C,
                         int C_real, egm_stream_t s);
/* SpatialAttentionModule.conv1 (7x7, 2 -> 1, no bias, w fp32 [1][2][7][7]) as a direct stencil on the 8-channel (mean, max)
 * map; out/dx are 8-channel maps (ch0 / ch0-1 real).  bwd: dx, dw; workspace egm_sa_conv7_bwd_workspace() bytes. */
int egm_sa_conv7_fwd(int dtype, const void* x, int ldx, const float* w, void* y, int ldy, int N, int H, int W, egm_stream_t s);
long long egm_sa_conv7_bwd_workspace(int N, int H, int W);
int egm_sa_conv7_bwd(int dtype, const void* x, int ldx, const void* dy, int lddy, const float* w, void* dx, int lddx, float* dw,
                     void* workspace, int N, int H, int W, egm_stream_t s);
/* ChannelAttentionModule pools: out [2N][C] (rows 0..N-1 = global average, N..2N-1 = global max), argidx int32 [N][C] =
 * first position of the maximum; workspace egm_global_pool_workspace() bytes. */
long long egm_global_pool_workspace(int N, long long HW, int C);
int egm_global_avgmax_fwd(int dtype, const void* x, int ldx, void* out, int* argidx, void* workspace, int N, long long HW,
                          int C, egm_stream_t s);
int egm_global_avgmax_bwd(int dtype, const void* gout, const int* argidx, void* dx, int lddx, int N, long long HW, int C,
                          egm_stream_t s);
/* dst[n][c] = dst[N+n][c] = red[n][0][c] (red fp32 [N][2][C]): the channel-attention gradient of egm_fusion_combine_bwd, reduced by
 * egm_reduce_tiles_batched, as the [2N][C] rows the attention's backward takes. */
int egm_rows_dup(int dtype, const float* red, void* dst, int ldd, int N, int C, egm_stream_t s);
/* ChannelAttentionModule.fc (src/EGM-UNet.py:1171-1190) on the R = 2N pooled rows: logits = W2 . relu(W0 . pooled).  w0 fp32 [Cr][C],
 * w2 fp32 [C][Cr] (the 1x1 conv weights as stored), h fp32 [R][Cr] = the hidden activation kept for backward.  One workgroup each;
 * the rows, the hidden activations and both weight matrices must fit 64 KB of LDS (C = 128, Cr = 32, R = 16: 46 KB backward).  Backward OVERWRITES dw0 / dw2. */
int egm_ca_mlp_fwd(int dtype, const void* pooled, int ldp, const float* w0, const float* w2, float* h, void* logits, int ldo, int R,
                   int C, int Cr, egm_stream_t s);
int egm_ca_mlp_bwd(int dtype, const void* dlogits, int ldd, const void* pooled, int ldp, const float* h, const float* w0,
                   const float* w2, float* dw0, float* dw2, void* dpooled, int lddp, int R, int C, int Cr, egm_stream_t s);
/* out = f + s*sigmoid(sa[..,0])*sigmoid(ca[n][c] + ca[N+n][c])   (x_out = up(res + x_fused_s * x_fused_c), :1232-1235).
 * backward: ds, dsa (8-channel map) and per-image partial tiles [N][nblk][2][C] of dca (row 0; reduce with
 * egm_reduce_tiles per image); nblk = egm_fusion_combine_blocks(HW, C).  df is g itself. */
int egm_fusion_combine_fwd(int dtype, const void* f, int ldf, const void* sv, int lds, const void* sa, int ldsa, const void* ca,
                           void* out, int ldo, int N, long long HW, int C, egm_stream_t s);
int egm_fusion_combine_blocks(long long HW, int C);
int egm_fusion_combine_bwd(int dtype, const void* g, int ldg, const void* sv, int lds, const void* sa, int ldsa, const void* ca,
                           void* ds, int ldds, void* dsa, int lddsa, float* partials, int N, long long HW, int C, egm_stream_t s);
/* Algebraic folds of FusionConv parameters (fp32, tiny): down(cat[x,x]) == conv with W[:, :K] + W[:, K:];
 * conv3(f)+conv5(f)+conv7(f) == one 7x7 conv with the zero-padded kernels (and biases) summed. */
int egm_fold2_fwd(const float* w, float* out, int rows, int K, egm_stream_t s);
int egm_fold2_bwd(const float* g, float* dw, int rows, int K, egm_stream_t s);
int egm_merge357_fwd(const float* w3, const float* w5, const float* w7, const float* b3, const float* b5, const float* b7,
                     float* w, float* b, int Co, int Ci, egm_stream_t s);
int egm_merge357_bwd(const float* gw, float* d3, float* d5, float* d7, const float* gb, float* gb3, int Co, int Ci, egm_stream_t s);
/* egm_fold2_fwd / egm_merge357_fwd that ALSO write the operand packs (egm_conv_pack layouts, groups = 1) of the derived weight:
 * wf [taps][CoutP][CinP], wd [taps flipped][CinP][CoutP] in `dtype`, CoutP/CinP = the counts rounded up to 8. */
int egm_fold2_pack(int dtype, const float* w, float* out, void* wf, void* wd, int rows, int K, egm_stream_t s);
int egm_merge357_pack(int dtype, const float* w3, const float* w5, const float* w7, const float* b3, const float* b5, const float* b7,
                      float* w, float* b, void* wf, void* wd, int Co, int Ci, egm_stream_t s);

/* ---- MCALayer (src/EGM-UNet.py:686-791, MCAGate :836-869, StdPool :827-834) ---------------------------------------- */
/* Three-axis sums in one pass: sums fp32 [N][H+W+C][2] laid out per image as [H rows | W columns | C channels];
 * mode 0: (sum a, sum a^2); mode 1: (sum a*b, -).  workspace egm_mca_reduce_workspace() bytes. C: power of two <= 512. */
long long egm_mca_reduce_workspace(int N, int H, int W, int C);
int egm_mca_reduce(int dtype, int mode, const void* a, int lda, const void* b, int ldb, float* sums, void* workspace, int N,
                   int H, int W, int C, egm_stream_t s);
/* egm_mca_reduce mode 0 over z = act(y*scale + shift), the BatchNorm(+ReLU) output of the conv in front of the MCALayer
 * (src/EGM-UNet.py:893-896), which is WRITTEN to z on the way: egm_bn_act_fwd and the statistics pass over its result as one pass. */
int egm_mca_reduce_bn(int dtype, const void* y, int ldy, const float* scale, const float* shift, int act, void* z, int ldz,
                      float* sums, void* workspace, int N, int H, int W, int C, egm_stream_t s);
/* sums -> stats [N][L][2] (mean, unbiased std), o [N][L] (pre-conv gate input), gates [N][L] (sigmoid outputs); L=H+W+C.
 * w_*: MCAGate.weight (2 floats); k_*: the 1 x ks conv kernel of each gate (h_cw, w_hc, c_hw).
 * ks_c == 0 is MCALayer(no_spatial=True) (src/EGM-UNet.py:700-703,766-771): there is no c_hw gate, w_c / k_c may be NULL, the channel
 * rows of `gates` are written as zeros (so x*(g_h+g_w+g_c) is x*(g_h+g_w)) and, in the backward, their coef / dwts / dks rows are zeros. */
int egm_mca_gates_fwd(const float* sums, const float* w_h, const float* k_h, int ks_h, const float* w_w, const float* k_w,
                      int ks_w, const float* w_c, const float* k_c, int ks_c, float* stats, float* o, float* gates, int N, int H,
                      int W, int C, egm_stream_t s);
/* dG [N][L][2] (slot 0 = sum over each slice of dx_out*x) -> coef [N][L][2] (A, B with dx += A + B*x along each axis),
 * dwts [3][2] (gradients of the three MCAGate.weight), dks [3][8] (gradients of the conv kernels). */
int egm_mca_gates_bwd(const float* dG, const float* stats, const float* o, const float* gates, const float* w_h, const float* k_h,
                      int ks_h, const float* w_w, const float* k_w, int ks_w, const float* w_c, const float* k_c, int ks_c,
                      float* dz_scratch, float* coef, float* dwts, float* dks, int N, int H, int W, int C, egm_stream_t s);
/* x_out = x*(g_h+g_w+g_c)/3; no_spatial != 0: x*(g_h+g_w)/2 (gates from egm_mca_gates_fwd with ks_c == 0) */
int egm_mca_xout(int dtype, const void* x, int ldx, const float* gates, void* xo, int ldo, int N, int H, int W, int C,
                 int no_spatial, egm_stream_t s);
/* r1 = 0.51*xo + 0.2*(max3-min3)(xo) + 0.1*shuffle4(xo); u2 = (xo - avg3 xo)^2; codes (optional, N*H*W*C bytes) = window
 * positions of the first max / first min, for the backward.  Then out = r1 + 0.2*avg3(u2) via egm_add_avg3. */
int egm_mca_stencil1(int dtype, const void* xo, int ld, void* r1, int ldr, void* u2, int ldu, unsigned char* codes, int N, int H,
                     int W, int C, egm_stream_t s);
int egm_add_avg3(int dtype, const void* a, int lda, const void* b, int ldb, float scale, void* out, int ldo, int N, int H, int W,
                 int C, egm_stream_t s);
/* The three calls above in ONE pass (x read once with a 2-pixel halo; out / codes / optionally x_out written once): 16 x 16 pixel tiles
 * of 32-channel chunks staged through LDS.  xo may be NULL (the backward recomputes x_out = x * gate).  Same arithmetic, rounding points
 * and summation order as egm_mca_xout + egm_mca_stencil1 + egm_add_avg3. */
int egm_mca_fused_fwd(int dtype, const void* x, int ldx, const float* gates, void* xo, int ldxo, void* out, int ldo, unsigned char* codes,
                      int N, int H, int W, int C, int no_spatial, egm_stream_t s);
/* backward chain: du = 0.4*(xo - avg3 xo)*avg3(g); dxo = 0.51 g + 0.1 unshuffle(g) + du - avg3(du) + 0.2*range_bwd(codes, g);
 * dx = dxo*(g_h+g_w+g_c)/3 + sum_axes(A + B*x)   (no_spatial != 0: /2, as in the forward) */
int egm_mca_bwd_du(int dtype, const void* xo, int ld, const void* g, int ldg, void* du, int ldd, int N, int H, int W, int C,
                   egm_stream_t s);
int egm_mca_bwd_dxo(int dtype, const unsigned char* codes, const void* g, int ldg, const void* du, int ldd, void* dxo, int ldo,
                    int N, int H, int W, int C, egm_stream_t s);
/* egm_mca_bwd_du + egm_mca_bwd_dxo as ONE tiled pass, bf16 only (x_out, g and the codes staged with their halo in LDS, du kept there):
 * same operand order in every sum as the pair.  Replaces the du / dxo steps of MCALayer's autograd backward (src/EGM-UNet.py:729-772). */
int egm_mca_bwd_dudxo(int dtype, const unsigned char* codes, const void* xo, int ldxo, const void* g, int ldg, void* dxo, int ldo,
                      int N, int H, int W, int C, egm_stream_t s);
int egm_mca_bwd_dx(int dtype, const void* dxo, int ldd, const void* x, int ldx, const float* gates, const float* coef, void* dx,
                   int ldo, int N, int H, int W, int C, int no_spatial, egm_stream_t s);

/* ---- CLIP ViT / CLIPSeg inference path (clip/model.py:159-206,487-501; models/clipseg.py:79-133,188-256,436-496) --------
 * Activations are row-major [rows, D] token matrices (batch-first), bf16 or fp32; scores and statistics are fp32. */
/* Batched GEMM with fused epilogue: C[b] = act(alpha * A[b](M x K) * op(B[b]) + bias) + R[b].
 * transB != 0: B[b] is [N][K] (nn.Linear weight, K of q k^T); else [K][N] (V of P V, `x @ proj`).  Two batch levels
 * (nb1 x nb2, e.g. images x heads) with element strides s?1 / s?2.  act: 0 none, 1 ReLU, 2 QuickGELU.
 * c_is_f32 != 0 stores C as fp32 (attention scores).  bias fp32 [N] or NULL; R (dtype, ldr) or NULL. */
int egm_gemm(int dtype, const void* A, int lda, const void* B, int ldb, int transB, void* C, int ldc, int c_is_f32,
             const float* bias, int act, const void* R, int ldr, float alpha, int M, int N, int K, int nb1, int nb2,
             long long sA1, long long sA2, long long sB1, long long sB2, long long sC1, long long sC2, long long sR1,
             long long sR2, egm_stream_t s);
/* Name of the kernel egm_gemm launches for a product, spelled like the rows of a kernel trace; returns its length, copies at most
 * buflen-1 characters into buf (may be NULL).  Host only, needs no device (as egm_conv_kernel_name).  ldr = 0: no residual; batch =
 * nb1 * nb2; every pointer counts as 16-byte aligned; honours egm_gemm_dma_mode.  One of
 *   gemm_kernel<bf16_t, true>  gemm_kernel<bf16_t, false>  gemm_kernel<float, true>  gemm_kernel<float, false>
 *   gemm_nt128_kernel<2, 2>  gemm_nt128_kernel<2, 4>
 *   gemm_dma_kernel<NT, NW>   NT 1..4 with NW 8; NT 3, 4 with NW 4 under mode 2.  The two middle template arguments of the trace
 *                             (<NT, HAS_R, ACT, NW>: residual and activation, which do not move the plan) are left out of the name. */
int egm_gemm_kernel_name(int dtype, int transB, int c_is_f32, int M, int N, int K, int lda, int ldb, int ldc, int ldr, int batch,
                         char* buf, int buflen);
/* Large bf16 A * B^T products (M >= 512, N >= 256, K a multiple of 64, one batch, >= 128 tiles of 256 x 256) run on the 8-wave LDS-DMA
 * kernel (csrc/gemm_dma.hip), bit-identical to the register-staged one.  mode 1 / 0: on / off, 2: its 4-wave form (128-row wave tiles),
 * 3: on without the 256 x 128 tile rule, 4: 256-wide tiles whatever N (both for A/B runs, profiles/r04_ab_runs.md), -1: query; returns the
 * previous mode (default: env EGM_GEMM_DMA, else 1). */
int egm_gemm_dma_mode(int mode);
/* P[r][:] (dtype) = softmax(S[r][:L]) (S fp32); causal != 0 keeps columns j <= r % L (text encoder mask,
 * clip/model.py:462-468); accumulate != 0 adds to P (CSA: softmax(q q^T) + softmax(k k^T), models/clipseg.py:96-102).
 * Columns L..ldp-1 of P are written as 0. */
/* Fused multi-head self attention on packed qkv [B][L][3*H*64] (bf16, head dimension 64): out [B][L][H*64].
 * mode 0: softmax(q k^T / 8) v; 1: causal (clip/model.py:462-468); 2: CSA (softmax(q q^T / 8) + softmax(k k^T / 8)) v
 * (models/clipseg.py:96-102).  Online softmax, fp32 statistics; scores and probabilities never reach HBM. */
int egm_attention_fused(int dtype, const void* qkv, int ld, int B, int L, int H, int head_dim, int mode, void* out, int ldo,
                        egm_stream_t s);
int egm_softmax_rows(int dtype, const float* S, int lds, void* P, int ldp, long long rows, int L, int causal, int accumulate,
                     egm_stream_t s);
/* LayerNorm over the last dimension with fp32 statistics (clip/model.py:159-165). */
int egm_layernorm(int dtype, const void* x, int ldx, const float* gamma, const float* beta, float eps, void* y, int ldy,
                  long long rows, int D, egm_stream_t s);
/* VisionTransformer.conv1 front half: fp32 NCHW image -> patch rows [B*(H/P)*(W/P)][C*P*P] (then egm_gemm with conv1.weight). */
int egm_patchify(int dtype, const float* img_nchw, void* out, int B, int C, int H, int W, int P, egm_stream_t s);
/* x[b][0] = class_embedding + pos[0]; x[b][1+t] = tok[b][t] + pos[1+t]  (models/clipseg.py:205-213) */
int egm_vit_assemble(int dtype, const void* tok, const float* cls, const float* pos, void* x, int B, int Ltok, int D, egm_stream_t s);
/* x[n][t] = token_embedding[tokens[n][t]] + (t < split ? pos[t] : pos_res[t])  (clip/model.py:428-431,488-490; split = 20) */
int egm_text_embed(int dtype, const int* tokens, const float* emb, const float* pos, const float* pos_res, int split, void* x,
                   int n, int L, int D, egm_stream_t s);
/* FiLM: a[b][t][:] = a[b][t][:] * mul[b][:] + add[b][:]  (models/clipseg.py:467-471) */
int egm_film(int dtype, void* a, const void* mul, const void* add, int B, int L, int D, egm_stream_t s);
/* out[n][:] = x[n][idx[n]][:]  (EOT token / class token selection) */
int egm_gather_rows(int dtype, const void* x, const int* idx, void* out, int n, int L, int D, egm_stream_t s);
/* ConvTranspose2d(D -> 1, kernel P, stride P) back half: y[b*Ltot + tok_off + ty*g + tx][i*P + j] (+ bias) ->
 * out fp32 [B][1][g*P][g*P]  (models/clipseg.py:478-484) */
int egm_pixel_shuffle(int dtype, const void* y, int ldy, int tok_off, int Ltot, const float* bias, float* out, int B, int g,
                      int P, egm_stream_t s);
/* fp32 -> dtype copy of a weight matrix */
int egm_cast_f32(int dtype, const float* src, void* dst, long long n, egm_stream_t s);

/* ---- criterion, metrics, optimizer --------------------------------------------------------------
 * criterion(): train_utils/train_and_eval.py:7-19 + dice_coefficient_loss.py:7-108 (five terms; reference quirks kept:
 * stencils on raw logit channel 0 against the label map of sample 0).  logits/dlogits fp32 NCHW, target int64 [N,H,W].
 * loss6 = {total, ce, dice, laplace, lap, sobel} (device).  workspace: egm_loss_workspace() bytes, kept for the
 * backward; signs: N*H*W bytes (stencil sign codes), needed when dice != 0. */
long long egm_loss_workspace(int N, int C);
int egm_loss_fwd(const float* logits, const long long* target, const float* class_weight, int N, int C, int H, int W,
                 long long ignore_index, int dice, float* loss6, float* workspace, unsigned char* signs, egm_stream_t s);
int egm_loss_bwd(const float* logits, const long long* target, const float* class_weight, int N, int C, int H, int W,
                 long long ignore_index, int dice, const float* workspace, const unsigned char* signs, const float* grad_out,
                 float* dlogits, egm_stream_t s);
/* ConfusionMatrix.update + DiceCoefficient.update (train_utils/distributed_utils.py:81-91,135-144):
 * hist[C*C] += bincount(C*t + argmax); counts[N][C][3] += (inter, pred, tgt) one-hot counts over t != dice_ignore_index;
 * pred (int64 [N,H,W]) optional.  hist/counts are zeroed by the caller. */
int egm_argmax_hist(const float* logits, const long long* target, int N, int C, int H, int W, long long dice_ignore_index,
                    unsigned long long* hist, unsigned long long* counts, long long* pred, egm_stream_t s);
/* out[2+2C] = {dice (classes 1.., mean over images), acc_global, acc[C], iu[C]} (distributed_utils.py:97-105,147-151) */
int egm_metrics_finalize(const unsigned long long* hist, const unsigned long long* counts, int N, int C, float* out,
                         egm_stream_t s);
/* CLIPSeg (+) UNet ensemble tail (predict_CLIPseg.py:501-525): fused = bilinear(clip_logits -> HxW, align_corners=False) +
 * alpha*unet_logits; pred (int64 [N,H,W], optional) = argmax_c fused; fused (fp32 [N,C,H,W], optional). */
int egm_ensemble_fuse(const float* clip_logits, const float* unet_logits, float alpha, int N, int C, int hc, int wc, int H, int W,
                      long long* pred, float* fused, egm_stream_t s);
/* Alpha grid search (eval_CLIPseg.py:656-723): one pass accumulates a confusion matrix for EVERY alpha of the grid
 * (hist: zeroed uint64 [na][C][C], accumulates across calls); egm_ensemble_miou gives mean IoU per alpha. na<=128, C<=4. */
int egm_ensemble_alpha_hist(const float* clip_logits, const float* unet_logits, const long long* target, const float* alphas, int na,
                            int N, int C, int hc, int wc, int H, int W, unsigned long long* hist, egm_stream_t s);
int egm_ensemble_miou(const unsigned long long* hist, int na, int C, float* miou, egm_stream_t s);
/* torch.optim.SGD(momentum, weight_decay) (train.py:115-118) over a device table of 40-byte {float* p; const float* g; float* buf;
 * long long n; long long chunk0;} entries (chunk0 as for egm_conv_pack_multi): g' = g*grad_scale + wd*p;
 * v = first_step ? g' : mu*v + g'; p -= lr*v.
 * lr_dev (device scalar) overrides lr when non-NULL. */
int egm_sgd_chunk(void);   /* elements per workgroup; total_chunks = sum over tensors of ceil(n / egm_sgd_chunk()) */
int egm_sgd_multi(const void* table_dev, int ntensors, long long total_chunks, const float* lr_dev, float lr, float momentum,
                  float weight_decay, float grad_scale, int first_step, egm_stream_t s);
/* table of {float* dst; const float* src; long long n;}: gradient bucket gather/scatter for the RCCL all-reduce. */
int egm_copy_multi(const void* table_dev, int ntensors, egm_stream_t s);

/* ---- Up(bilinear=False): nn.ConvTranspose2d(Cin, Cout, 2, stride 2) (src/unet.py:36, src/EGM-UNet.py:941) ------------------
 * Run as a 1x1 convolution with 4*CoutP output channels ordered (i, j, co) -- egm_convT2x2_pack rearranges the [Cin][Cout][2][2]
 * parameter into that OIHW matrix (to_packed = 1) or scatters a gradient back (to_packed = 0) -- followed by the 2x2 pixel shuffle,
 * which adds the bias and writes at offset (oy, ox) inside a zero-filled [Ho][Wo] frame (F.pad of Up.forward). */
int egm_convT2x2_pack(float* w_iohw, float* w4, int Cin, int Cout, int CoutP, int to_packed, egm_stream_t s);
int egm_shuffle2x2_fwd(int dtype, const void* y4, int ld4, const float* bias, int bias_n, void* out, int ldo, int N, int H, int W, int C,
                       int Ho, int Wo, int oy, int ox, egm_stream_t s);
int egm_shuffle2x2_bwd(int dtype, const void* g, int ldg, void* d4, int ld4, int N, int H, int W, int C, int Ho, int Wo, int oy, int ox,
                       egm_stream_t s);

/* ---- ELA, Efficient Local Attention (src/EGM-UNet.py:56-79; an unused ablation block of the reference) -----------
 * strip means mh [N][H][C] (over W) and mw [N][W][C] (over H), fp32 -> shared depthwise Conv1d(ks, no bias, conv_w [C][ks]) ->
 * GroupNorm(groups, C) -> sigmoid gates gh, gw -> out = x * gh[n,h,c] * gw[n,w,c].  yh/yw (conv outputs) and stats
 * [N][2][groups][2] (mean, rstd) are kept for egm_ela_bwd, which returns dx and the parameter gradients. */
int egm_ela_strip_means(int dtype, const void* x, int ldx, float* mh, float* mw, int N, int H, int W, int C, egm_stream_t s);
int egm_ela_gates_fwd(const float* mh, const float* mw, const float* conv_w, int ks, const float* gamma, const float* beta, float eps,
                      float* yh, float* yw, float* gh, float* gw, float* stats, int N, int H, int W, int C, int groups, egm_stream_t s);
int egm_ela_apply(int dtype, const void* x, int ldx, const float* gh, const float* gw, void* out, int ldo, int N, int H, int W, int C,
                  egm_stream_t s);
long long egm_ela_bwd_workspace(int N, int H, int W, int C, int ks);
int egm_ela_bwd(int dtype, const void* g, int ldg, const void* x, int ldx, const float* mh, const float* mw, const float* yh, const float* yw,
                const float* gh, const float* gw, const float* stats, const float* conv_w, int ks, const float* gamma, void* dx, int lddx,
                float* dconv_w, float* dgamma, float* dbeta, float* workspace, int N, int H, int W, int C, int groups, egm_stream_t s);

/* ---- HEGDC (src/EGM-UNet.py:210-340; an unused ablation block of the reference) ---------------------------------------
 * egm_hegdc_edge_features: the block's no_grad branch: channel mean -> fixed Scharr/16 + Sobel/4 stencils -> magnitudes ->
 * min-max over the WHOLE batch -> sqrt (gamma 0.5) -> blend a*scharr + (1-a)*sobel, a = sigmoid(mean difference); feats
 * [N][H][W][8] in the activation dtype holds (scharr_x, scharr_y, sobel_x, sobel_y, blend, 0, 0, 0).
 * egm_scale_sigmoid_*: W * sigmoid(den) ("density" scaling of conv1's weight) and its gradients.
 * egm_mul2_scalar_*: a * b * alpha with a learnable device scalar alpha and its gradients (db may be NULL). */
long long egm_hegdc_edge_workspace(int N, int H, int W);
int egm_hegdc_edge_features(int dtype, const void* x, int ldx, int C_real, void* feats, float* workspace, int N, int H, int W,
                            egm_stream_t s);
int egm_scale_sigmoid_fwd(const float* w, const float* den, float* out, long long n, egm_stream_t s);
int egm_scale_sigmoid_bwd(const float* g, const float* w, const float* den, float* dw, float* dden, float* partials, long long n,
                          egm_stream_t s);
int egm_mul2_scalar_fwd(int dtype, const void* a, int lda, const void* b, int ldb, const float* alpha, void* out, int ldo, long long npix,
                        int C, egm_stream_t s);
int egm_mul2_scalar_bwd(int dtype, const void* g, int ldg, const void* a, int lda, const void* b, int ldb, const float* alpha, void* da,
                        int ldda, void* db, int lddb, float* dalpha, float* partials, long long npix, int C, egm_stream_t s);

/* ---- device-side data path (transforms.py, my_dataset.py:118-132) ----------------------------------------------
 * Decoded uint8 images [H][W][C] already in device memory.
 * egm_resample_u8: one separable pass of Pillow's antialiased resize (F.resize -> Image.resize(BILINEAR), transforms.py:39):
 *   axis 1: dst [H][out_size][C], axis 0: dst [out_size][W][C];  out = clip8((2^21 + sum_j src[b0+j] * coefs[o][j]) >> 22)
 *   with bounds [out_size][2] = (b0, n) and coefs [out_size][ksize] int32 (22-bit fixed point) computed by the caller.
 * egm_gather_u8: dst[y][x][c] = src[yidx[y]][xidx[x]][c]  (NEAREST resize of the mask, transforms.py:40).
 * egm_augment_u8: hflip/vflip -> pad_if_smaller with zeros -> crop(top, left, crop_h, crop_w) -> to_tensor (/255) ->
 *   normalize(mean, std) (transforms.py:46-107), written into an [out_h][out_w] collate slot: outside the crop the image is
 *   0.0 and the target 255 (collate_fn).  out_img_chw fp32 [3][out_h][out_w], out_target int64 [out_h][out_w] (may be NULL with
 *   mask_hw NULL).  mean3/std3 are HOST pointers (3 floats each). */
int egm_resample_u8(const void* src, int H, int W, int C, void* dst, int axis, int out_size, const int* bounds, const int* coefs,
                    int ksize, egm_stream_t s);
int egm_gather_u8(const void* src, int H, int W, int C, void* dst, int Ho, int Wo, const int* yidx, const int* xidx, egm_stream_t s);
int egm_augment_u8(const void* img_hwc3, const void* mask_hw, int H, int W, int hflip, int vflip, int top, int left, int crop_h,
                   int crop_w, const float* mean3_host, const float* std3_host, float* out_img_chw, long long* out_target,
                   int out_h, int out_w, egm_stream_t s);

/* ---- per-image ensemble pipeline: the two ends around the models (predict_CLIPseg.py:447-451, :525-534) ------------------
 * egm_clip_preprocess_u8: ToTensor -> Normalize(mean, std) -> Resize((Sh, Sw)) of the float tensor, i.e.
 *   F.interpolate(x, (Sh, Sw), mode="bilinear", align_corners=False, antialias=A), from the decoded uint8 photo [H][W][3] to fp32
 *   [3][Sh][Sw].  The separable filter comes from the caller as for egm_resample_u8, with fp32 weights: per output index
 *   bounds [out][2] = (b0, n) int32 and weights [out][ksize] fp32 summing to one (x tables over W -> Sw, y tables over H -> Sh; the
 *   antialiased triangle rule or the two taps of plain bilinear, one kernel serves both).
 *   out = ((sum_i wy[i] * sum_j wx[j] * img[b0y+i][b0x+j]) / 255 - mean) / std: the filter runs on the bytes and the result is
 *   normalised, which differs from normalising first by rounding only.  Two launches: horizontal into tmp_chw (fp32 [3][H][Sw],
 *   supplied by the caller), then vertical.  mean3/std3 are HOST pointers (3 floats each).  ksize <= 64 per
 *   axis and a horizontal reduction whose staging fits 64 KiB of LDS, otherwise EGM_ERR_ARG.
 * egm_ensemble_mask_u8: out[n][y][x] = lut[argmax_c fused[n][c][yidx[y]][xidx[x]]] (lut: 256 bytes, NULL = the class id), uint8
 *   [N][H0][W0], with fused = bilinear(clip_logits -> HxW, align_corners=False) + alpha * unet_logits evaluated by the expression of
 *   egm_ensemble_fuse (csrc/ensemble_fuse.h), ties to the lowest class: bit-identical to egm_ensemble_fuse followed by a gather.
 *   yidx [H0] / xidx [W0] int32: the nearest-neighbour tables of cv2.resize(pred, (W0, H0), INTER_NEAREST).  alpha_dev is a DEVICE
 *   scalar, so a captured graph follows a new alpha. */
int egm_clip_preprocess_u8(const void* img_hwc3, int H, int W, float* out_chw, int Sh, int Sw, const int* xbounds, const float* xweights,
                           int xksize, const int* ybounds, const float* yweights, int yksize, const float* mean3_host,
                           const float* std3_host, float* tmp_chw, egm_stream_t s);
int egm_ensemble_mask_u8(const float* clip_logits, const float* unet_logits, const float* alpha_dev, int N, int C, int hc, int wc, int H,
                         int W, const int* yidx, const int* xidx, const unsigned char* lut, unsigned char* out, int H0, int W0,
                         egm_stream_t s);

/* ---- batched ensemble pipeline: the same two ends for B photos of one size, contiguous uint8 [B][H][W][3] (image b starts b*H*W*3
 * bytes in, at whatever alignment that is; nothing outside the buffer is read).  Every launch covers the whole batch, so the launch
 * count does not depend on B.  The tail needs no batched form: egm_ensemble_mask_u8 takes N.
 * egm_unet_preprocess_batch_u8: egm_resample_u8 along axis 1 (W -> ow), then along axis 0 (H -> oh), then egm_augment_u8 without
 *   flips and with the full crop, for every image: fp32 [B][3][oh][ow], per element the same expressions, so image b equals the
 *   per-image chain bit for bit.  Tables as for egm_resample_u8 (bounds [out][2], coefs [out][ksize] int32, 22-bit fixed point).
 *   A pass whose bounds and coefs are NULL is the identity and is skipped (then ow == W, or oh == H).  tmp_bhwc3: uint8
 *   [B][H][ow][3] from the caller, used by the horizontal pass only (may be NULL without one).  The vertical pass writes the
 *   normalised floats directly: two launches, or one without a horizontal pass.  mean3/std3 are HOST pointers.
 * egm_clip_preprocess_batch_u8: egm_clip_preprocess_u8 for every image, fp32 [B][3][Sh][Sw], bit-identical per image (the same
 *   horizontal kernel over the B*H rows, the same taps and expressions in the vertical pass).  tmp_cbhw: fp32 [3][B][H][Sw] from the
 *   caller.  The same limits: ksize <= 64 per axis and the LDS bound, otherwise EGM_ERR_ARG; B*H*W*3 < 2^31.  Two launches. */
int egm_unet_preprocess_batch_u8(const void* imgs_bhwc3, int B, int H, int W, float* out_bchw, int oh, int ow, const int* xbounds,
                                 const int* xcoefs, int xksize, const int* ybounds, const int* ycoefs, int yksize,
                                 const float* mean3_host, const float* std3_host, void* tmp_bhwc3, egm_stream_t s);
int egm_clip_preprocess_batch_u8(const void* imgs_bhwc3, int B, int H, int W, float* out_bchw, int Sh, int Sw, const int* xbounds,
                                 const float* xweights, int xksize, const int* ybounds, const float* yweights, int yksize,
                                 const float* mean3_host, const float* std3_host, float* tmp_cbhw, egm_stream_t s);

/* ---- ensemble scoring at the ground truth's size (evaluating_indicator.py:347-417, eval_CLIPseg.py:682-711) ---------------------
 * Both accumulate exact integer counts into caller-zeroed uint64 matrices (hist[label class][predicted class], across calls), in one
 * launch each, and are capturable.  C <= 4; na <= 128.  A class table is 256 bytes of DEVICE memory, byte value -> class; a value
 * >= C drops the pixel.
 * egm_mask_confusion_u8: hist[label_cls[label[i]]][pred_cls[pred[i]]] += 1 for the npix pixels of two uint8 images (a batch
 *   [N][H0][W0] is npix = N*H0*W0).  One streaming pass with 16-byte loads in the body; any base alignment of either image and any
 *   npix >= 1.  Partial counts are 32 bits per lane and summed in 64 bits per workgroup, then at most C*C 64-bit atomics per
 *   workgroup; a lane counts fewer than 2^22 pixels at any admitted size, and npix > 2^40 is refused (EGM_ERR_ARG).
 * egm_ensemble_alpha_hist_u8: the alpha grid search scored at the label's size.  hist [na][C][C] (the layout egm_ensemble_miou
 *   reads): hist[a][t][p] = number of label pixels (n, Y, X) of class t = label_cls[labels[n][Y][X]] whose source pixel
 *   (yidx[Y], xidx[X]) has fused argmax p under alphas[a], where yidx / xidx are the nearest-neighbour tables of
 *   cv2.resize(pred, (Wl, Hl), INTER_NEAREST) from H x W.  The tables come in as their spans: ybeg [H+1] / xbeg [W+1] int32,
 *   non-decreasing, beg[i] = the first label index whose source is >= i and beg[H] = Hl, so source pixel (y, x) owns the label
 *   rectangle [ybeg[y], ybeg[y+1]) x [xbeg[x], xbeg[x+1]) (empty for some pixels when the label is the smaller one).  The
 *   rectangle's classes are counted once and the na argmaxes run once per SOURCE pixel: one read of the labels plus N*H*W*na
 *   argmaxes whatever the label's size (one lane per source pixel counts and stages, then one lane per alpha accumulates).
 *   Fused value and argmax are those of egm_ensemble_mask_u8 (csrc/ensemble_fuse.h, ties to the lowest class): bit-identical to
 *   running it once per alpha with lut = NULL and counting.  labels: uint8 [N][Hl][Wl]; logits as for egm_ensemble_fuse.
 *   Partial counts are 32 bits per lane, then per workgroup; either is at most the call's label pixels, so N*Hl*Wl >= 2^32 is
 *   refused (EGM_ERR_ARG): split such a batch. */
int egm_mask_confusion_u8(const unsigned char* pred, const unsigned char* label, long long npix, const unsigned char* pred_cls,
                          const unsigned char* label_cls, int C, unsigned long long* hist, egm_stream_t s);
int egm_ensemble_alpha_hist_u8(const float* clip_logits, const float* unet_logits, const unsigned char* labels,
                               const unsigned char* label_cls, const float* alphas, int na, int N, int C, int hc, int wc, int H, int W,
                               int Hl, int Wl, const int* ybeg, const int* xbeg, unsigned long long* hist, egm_stream_t s);

/* ---- threshold-swept scores of binary logits (csrc/sweep.hip) ---------------------------------------------------------
 * scores: fp32.  C == 1: one map per sample, [N][HW] (c_pos, c_neg ignored).  C >= 2: an NCHW tensor [N][C][HW]; a pixel's score is
 * the fp32 difference x[n][c_pos] - x[n][c_neg] (0 <= c_pos != c_neg < C).  Samples are independent and may start at any 4-byte offset
 * (odd HW); 1 <= N <= 65535 (the grid's y), 1 <= HW <= 2^40, otherwise EGM_ERR_ARG.
 * egm_sweep_hist: hist[n][g][b] += 1 for every kept pixel, b = #{i : score > cuts[i]} by fp32 comparison alone (NaN: bin 0), g its truth.
 *   cuts: T floats, strictly ascending, no NaN, the last one +inf (so b <= T - 1), 2 <= T <= 256.  They are given twice: cuts_host in
 *   HOST memory is what the launcher checks before the launch, cuts_dev in DEVICE memory holds the same T floats and is what the kernel
 *   reads (once per workgroup, into LDS), so a captured launch carries no table in its arguments.
 *   target: target_f32 == 0: uint8 [N][HW] through target_cls (256 bytes of DEVICE memory: 0 = negative, 1 = positive, anything else
 *   drops the pixel); target_f32 != 0: fp32 [N][HW], > 0.5 is positive, anything else (NaN included) negative, target_cls may be NULL.
 *   hist: uint64 [N][2][T], caller-zeroed, accumulated across calls.  One launch, one workgroup per egm_sweep_chunk() pixels of a
 *   sample; 32-bit partial counts on chip are bounded by that chunk, so no size can wrap them; at most one 64-bit atomic per non-zero
 *   cell and workgroup.  Integer adds: the result does not depend on scheduling.
 * egm_score_mask_u8: out[n][i] = score > cut ? v_fg : v_bg (uint8 [N][HW], any alignment); cut may be +-inf, not NaN; v_* in 0..255.
 * Both launch on s, allocate nothing, wait for nothing (capturable), and check their arguments before the launch. */
long long egm_sweep_chunk(void);
int egm_sweep_hist(const float* scores, int N, int C, int c_pos, int c_neg, long long HW, const void* target, int target_f32,
                   const unsigned char* target_cls, const float* cuts_host, const float* cuts_dev, int T, unsigned long long* hist,
                   egm_stream_t s);
int egm_score_mask_u8(const float* scores, int N, int C, int c_pos, int c_neg, long long HW, float cut, int v_bg, int v_fg,
                      unsigned char* out, egm_stream_t s);

/* ---- connected components of uint8 class maps and the mask clean-up on them (csrc/ccl.hip) -------------------------
 * cls: uint8 [N][H][W], 0 = background; images are independent.  Two pixels are joined when they hold the same byte and are neighbours:
 * `connectivity` (8 or 4) for foreground bytes, the dual (4 or 8) for background.  Any H, W >= 1 and any alignment; H*W <= 2^30,
 * otherwise EGM_ERR_ARG.  Launch count and grids depend on the shapes only, every launch covers the batch, nothing waits for the
 * device or for another workgroup, and every device loop has a trip bound derived from H*W.
 * workspace: egm_ccl_workspace(N, H, W) bytes of device memory owned by the caller (egm_ccl_label_u8 touches only its first 256 bytes).
 *   Its first int32 is a status word: a loop that ran into its bound ORs a bit in (1 find, 2 union) and leaves.  It is never cleared
 *   by these calls: the caller zeroes it once and reads it whenever it likes; 0 = every call since then ran to completion.
 * egm_ccl_label_u8: labels int32 [N][H][W] = raster index y*W + x of the first pixel, in raster order, of the pixel's component
 *   (background components included); areas int32 [N][H][W] (may be NULL) = the pixel count at a component's first pixel, 0 elsewhere.
 *   Three launches.
 * egm_mask_clean_u8: params_dev = int32 {min_area, keep_largest, max_hole} in DEVICE memory (a captured graph follows new values).
 *   Stage 1 (max_hole > 0): a background component that touches no image border and has at most max_hole pixels takes the byte of
 *   the pixel left of its first pixel.  Stage 2 (min_area > 1 or keep_largest), on the relabelled result: a foreground component
 *   smaller than min_area becomes 0; with keep_largest only the largest component of each byte value stays (ties: the smaller first
 *   index), if it passes min_area.  Results: out_cls uint8 [N][H][W] (may be NULL), the cleaned map, and, when out != NULL,
 *   out [N][H0][W0] = lut[cleaned[yidx[y]][xidx[x]]] written by the last pass itself (tables and lut as for egm_ensemble_mask_u8;
 *   any alignment of out).  out_cls and out may not both be NULL.  Nine launches whatever the parameters. */
long long egm_ccl_workspace(int N, int H, int W);
int egm_ccl_label_u8(const unsigned char* cls, int N, int H, int W, int connectivity, int* labels, int* areas, void* workspace,
                     egm_stream_t s);
int egm_mask_clean_u8(const unsigned char* cls, int N, int H, int W, int connectivity, const int* params_dev, void* workspace,
                      unsigned char* out_cls, const int* yidx, const int* xidx, const unsigned char* lut, unsigned char* out, int H0,
                      int W0, egm_stream_t s);

/* ---- Boundary IoU counts of uint8 masks at their own size (csrc/boundary.hip) ----------------------------------------
 * pred, label: uint8 [N][H][W]; images are independent.  Class tables as for egm_mask_confusion_u8 (256 bytes of DEVICE memory, a
 * value >= C puts the pixel in no class); 1 <= C <= 4.  With M_k = "the pixel's class is k", the eroded mask is E_k(y, x) = 1 iff
 * M_k = 1 at every (y + dy, x + dx), |dy|, |dx| <= radius, all of them inside the image (outside counts as 0), and the band is
 * B_k = M_k and not E_k: mask_to_boundary of the Boundary IoU paper (Cheng et al., CVPR 2021) with dilation radius `radius` pixels.
 * A window larger than the image leaves E_k empty, so the band is the whole mask.
 * counts [N][C][3] uint64, caller-zeroed and accumulated across calls (may be NULL): {|Bpred_k and Blabel_k|, |Bpred_k|, |Blabel_k|}
 *   of image n.  band_pred / band_label uint8 [N][H][W] (may be NULL): bit k = B_k of that side.  label == NULL is the one-sided
 *   form and needs counts == NULL and band_label == NULL.  At least one output must be given.
 * workspace: egm_boundary_workspace(N, H, W) bytes of device memory owned by the caller (two bytes per pixel of a padded row).
 * Two launches whatever the content, each covering the batch (rows, then columns); nothing waits for the device or for another
 * workgroup; every device loop has a trip count derived from H, W and radius; capturable on one stream.  Any H, W >= 1 with
 * H*W <= 2^30 and N*H <= 2^31, any radius >= 1, any base alignment of the images and of the band outputs; otherwise EGM_ERR_ARG.
 * Counts are exact: a lane counts at most 512 pixels in 32 bits, a wave's sum goes to counts with one 64-bit atomic per cell. */
long long egm_boundary_workspace(int N, int H, int W);
int egm_mask_boundary_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W, int radius,
                         const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                         unsigned long long* counts, unsigned char* band_pred, unsigned char* band_label, egm_stream_t s);

/* ---- Contour scores of uint8 masks at their own size (csrc/contour.hip) --------------------------------------------------
 * Images, class tables, C and the independence of a batch's images as for egm_mask_boundary_u8; every distance is a squared integer
 * distance compared with radius^2.
 * egm_mask_boundary_euclid_u8: egm_mask_boundary_u8 with a Euclidean band.  BE_k = the pixels of class k with some q in Z^2,
 *   |p - q|^2 <= radius^2, that is outside the image or not of class k (a pixel in no class is in no band and is "not k" for every k).
 *   Arguments, outputs ({|BEpred_k and BElabel_k|, |BEpred_k|, |BElabel_k|}, bit k = BE_k) and the one-sided form as there.  BE_k is a
 *   subset of the box band of the same radius; a disc larger than the image makes the band the whole mask.
 * egm_mask_contour_f_u8: the counts of the boundary F-measure.  The contour K_k = the pixels of class k with a 4-neighbour INSIDE THE
 *   IMAGE whose class is not k (the image frame makes no contour, unlike the band).  counts [N][C][4] uint64, caller-zeroed and
 *   accumulated across calls (may be NULL): {mp, |Kpred_k|, mg, |Klabel_k|} of image n, mp = the pixels of Kpred_k with a pixel of
 *   Klabel_k within `radius` (the tolerance), mg the mirror image.  contour_pred / contour_label uint8 [N][H][W] (may be NULL): bit k =
 *   K_k of that side.  label == NULL needs counts == NULL and contour_label == NULL.  At least one output must be given.
 * workspace: egm_contour_workspace(N, H, W, C) bytes of device memory owned by the caller, good for both calls (max(3, 2 C + 1) bytes
 *   per pixel of a padded row).
 * Two launches per call whatever the content, N, C and radius (rows, then columns); nothing waits for the device or for another
 * workgroup; capturable on one stream.  1 <= radius <= 254 (a row distance is kept in a byte, 255 = none), H*W <= 2^30, N*H <= 2^31,
 * any base alignment of the images and of the outputs; otherwise EGM_ERR_ARG.  Counts are exact: a lane counts at most 64 pixels in
 * 32 bits, a wave's sum goes to counts with one 64-bit atomic per non-zero cell. */
long long egm_contour_workspace(int N, int H, int W, int C);
int egm_mask_boundary_euclid_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W, int radius,
                                const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                                unsigned long long* counts, unsigned char* band_pred, unsigned char* band_label, egm_stream_t s);
int egm_mask_contour_f_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W, int radius,
                          const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                          unsigned long long* counts, unsigned char* contour_pred, unsigned char* contour_label, egm_stream_t s);

/* ---- Surface distances of uint8 masks at their own size (csrc/surface.hip) ---------------------------------------------
 * Images, class tables, C, the independence of a batch's images and the contour K_k of a side (4-neighbours inside the image, the
 * frame makes none, a dropped byte is "not k") as for egm_mask_contour_f_u8.  For a pixel p of Kpred_k, d2(p) = the minimum over q in
 * Klabel_k of |p - q|^2 in the same image, an exact integer, never truncated: direction 0 is pred -> label, direction 1 label -> pred.
 * counts [N][C][2][260] uint64, caller-zeroed and accumulated across calls (may be NULL), per image, class and direction:
 *   [0] n = |K| of the asking side; [1] the sum of q = isqrt(d2 * 2^16) = floor(256 d); [2] the sum of d2; [3] the largest d2 (combined
 *   with max, not add); [4 + t], t = 0..255: the pixels with ceil(sqrt(d2)) = t in integers, bin 255 = "255 or more".  Where the other
 *   side's contour of the class is empty in the image the direction has no distances: n is counted, the rest stays as it was.  The
 *   sum of bins 0..r of direction 0 is egm_mask_contour_f_u8's mp at radius r (r <= 254), of direction 1 its mg.
 * d2_pred / d2_label int32 [N][H][W] (may be NULL): d2 at the side's contour pixels (for the pixel's own class), -1 everywhere else
 *   and where the other contour is empty.  Both images are required; at least one of the three outputs must be given.
 * workspace: egm_surface_workspace(N, H, W, C) bytes of device memory owned by the caller (1 + 4 C bytes per pixel of a padded row:
 *   the contour byte and a 16-bit row distance per side and class, 0xFFFF = none).
 * Two launches per call whatever the content, N, C and the distances (rows, then columns); nothing waits for the device, for another
 * workgroup or for another wave; every device loop has a trip count of at most max(H, the chunks of a row); capturable on one
 * stream.  H, W <= 32767 (d2 < 2^31, a row distance fits 16 bits), H*W <= 2^30, N*H <= 2^31, any base alignment of the images, the
 * natural alignment of counts and of the maps; otherwise EGM_ERR_ARG.  Every cell is exact and independent of the order of the adds. */
long long egm_surface_workspace(int N, int H, int W, int C);
int egm_mask_surface_dist_u8(const unsigned char* pred, const unsigned char* label, int N, int H, int W,
                             const unsigned char* pred_cls, const unsigned char* label_cls, int C, void* workspace,
                             unsigned long long* counts, int* d2_pred, int* d2_label, egm_stream_t s);

/* ---- Sliding-window inference: overlapping tiles cut and blended on the device (csrc/tiles.hip) -------------------------
 * A plan cuts every image of an fp32 NCHW batch into ny x nx tiles of h x w pixels: tile t = (n * ny + i) * nx + j covers rows ys[i] ..
 * ys[i] + h - 1 and columns xs[j] .. xs[j] + w - 1 of image n, T = N * ny * nx tiles.  ys_dev [ny] / xs_dev [nx]: int32 DEVICE tables,
 * ascending, every tile inside its image, every pixel covered at least once (egm_unet_amd.tiled.TilePlan makes them).
 * egm_tile_gather_f32: dst fp32 [count][C][h][w], dst[k] = tile min(t0 + k, T - 1) of src: the clamp fills the last chunk of a batched
 *   loop with copies of the last tile.  0 <= t0 < T, count > 0.  ONE launch whatever count is.
 * egm_tile_blend_f32: tiles fp32 [T][C][h][w] -> logits_out fp32 NCHW and / or mask_out uint8 [N][H][W] (either may be NULL, not both).
 *   wy_dev [h] / wx_dev [w]: fp32 DEVICE tables, the two profiles of the separable weight (> 0), made on the host.  A gather: each output
 *   pixel (y, x) visits the tiles that cover it in ascending t, no atomics, so the result does not depend on scheduling.  The arithmetic
 *   is fixed so that a float32 restatement gives the same bits: per covering tile wt = wy[y - y0] * wx[x - x0] (one fp32 rounding),
 *   p = wt * v (one rounding), acc = acc + p and wsum = wsum + wt (one rounding each, never contracted into an FMA), from acc = wsum =
 *   0; then out = acc / wsum, correctly rounded.  mask = lut[argmax_c out], ties to the lowest class as egm_argmax_u8; lut NULL: the
 *   index itself.  ONE launch whatever T is; T*C*h*w*4 bytes read, N*C*H*W*4 (+ N*H*W) written.  Offsets into tiles are 64-bit.
 * Limits: H, W <= 32767, h <= H, w <= W, ny * h >= H and nx * w >= W (fewer tiles cannot cover the image: a stride above the window),
 *   T < 2^31, C <= 256 when a mask is asked for; any alignment of every buffer (16-byte stores where W % 4 == 0, resp. w % 4 == 0, and
 *   the output's base is aligned).  Bad scalars and null pointers return EGM_ERR_ARG with a message before any launch.  Nothing waits
 *   for the device; capturable on one stream. */
int egm_tile_gather_f32(const float* src, int N, int C, int H, int W, const int* ys_dev, int ny, const int* xs_dev, int nx, int h, int w,
                        int t0, int count, float* dst, egm_stream_t s);
int egm_tile_blend_f32(const float* tiles, int N, int C, int H, int W, const int* ys_dev, int ny, const int* xs_dev, int nx, int h, int w,
                       const float* wy_dev, const float* wx_dev, const unsigned char* lut, float* logits_out, unsigned char* mask_out,
                       egm_stream_t s);

/* ---- Test-time augmentation: flip and multi-scale views made and merged on the device (csrc/tta.hip) -------------------
 * An axis resized from n_in to n_out pixels (bilinear, align_corners=False, no antialias) is two DEVICE tables made on the host in
 * integers (egm_unet_amd.tta.resize_axis): idx int32 [n_out][2] = the two source pixels (i0, i1) of output pixel d, and l1 fp32 [n_out],
 * the weight of i1; the weight of i0 is l0 = 1 - l1 (one fp32 subtraction on the device).  The device never computes a coordinate.
 * With a = A[r(iy0)][c(ix0)], b = A[r(iy0)][c(ix1)], c = A[r(iy1)][c(ix0)], d = A[r(iy1)][c(ix1)] the sample is
 *     top = lx0 * a + lx1 * b,  bot = lx0 * c + lx1 * d,  val = ly0 * top + ly1 * bot,
 * every multiply, add and subtract one fp32 rounding, none contracted into an FMA, so a float32 restatement gives the same bits.
 * A flip code's bit 0 mirrors the columns, bit 1 the rows.
 * egm_tta_views_f32: src fp32 [N][C][H][W] -> dst fp32 [F*N][C][h][w], the F flipped views of ONE scale; view f of image n at batch
 *   index f*N + n.  dst[f*N + n][c][y][x] = the sample of src[n][c] at row ry = (flips[f] & 2 ? h-1-y : y) of yi_dev [h][2] / yl_dev [h]
 *   and column cx = (flips[f] & 1 ? w-1-x : x) of xi_dev [w][2] / xl_dev [w] (here r and c are the identity: the mirror is in which
 *   table row a pixel reads).  flips_dev: int32 [F].  ONE launch whatever N and F are; the taps are gathers (dword loads).
 * egm_tta_merge_f32: views_dev: DEVICE table of V egm_tta_view, each a view's fp32 [N][C][h][w] tensor, its size, its flip code and the
 *   four tables from (h, w) to (H, W): yi [H][2], yl [H], xi [W][2], xl [W]; r(k) = h-1-k for a rows flip, c(k) = w-1-k for a columns
 *   flip.  -> logits_out fp32 [N][C][H][W] and / or mask_out uint8 [N][H][W] (either may be NULL, not both).
 *   mode 0 (mean): acc = 0; acc = acc + sample_v for v ascending; out = acc / (float)V, correctly rounded.  Bit-reproducible.
 *   mode 1 (prob): per view and pixel m = max_c sample_c, e_c = expf(sample_c - m) (the accurate expf), z = the sum of e_c in ascending
 *     c, acc_c = acc_c + e_c / z; out_c = acc_c / (float)V.  The samples of every class stay in registers: C <= 8.
 *   mask = lut[argmax_c out], ties to the lowest class as egm_argmax_u8; lut NULL: the index itself.  ONE launch whatever N and V are,
 *   no atomics; the mask needs no merged tensor in memory.
 * Every index read from a table is clamped into its tensor before it addresses memory, and a flip code is read & 3, so a wrong table
 *   gives wrong pixels, never an access outside [N][C][h][w] as the call (the descriptor) states it.
 * Limits: H, W, h, w <= 32767, V <= 4096, C <= 256 when a mask is asked for, C <= 8 in mode 1; any alignment of every buffer (16-byte
 *   stores where the row length is a multiple of 4 and the output's base is aligned; tables int32 / fp32 aligned).  Bad scalars and
 *   null pointers return EGM_ERR_ARG with a message before any launch.  Nothing waits for the device; capturable on one stream. */
typedef struct egm_tta_view {
    const float* logits;        /* fp32 [N][C][h][w] */
    const int* yi;              /* int32 [H][2] */
    const float* yl;            /* fp32 [H] */
    const int* xi;              /* int32 [W][2] */
    const float* xl;            /* fp32 [W] */
    int h, w, flip, pad;
} egm_tta_view;                 /* 56 bytes */
int egm_tta_views_f32(const float* src, int N, int C, int H, int W, int h, int w, const int* yi_dev, const float* yl_dev,
                      const int* xi_dev, const float* xl_dev, const int* flips_dev, int F, float* dst, egm_stream_t s);
int egm_tta_merge_f32(const egm_tta_view* views_dev, int V, int N, int C, int H, int W, int mode, const unsigned char* lut,
                      float* logits_out, unsigned char* mask_out, egm_stream_t s);

/* ---- batched training data path: B ragged photos with masks -> the batch a train step reads (train.py:14-33, my_dataset.py:118-132)
 * egm_train_batch_u8: for every image b what egm_resample_u8 (axis 1, then axis 0), egm_gather_u8 and egm_augment_u8 compute one
 *   after the other, written into slot b of out_img_bchw fp32 [B][3][slot_h][slot_w] and out_target_bhw int64 [B][slot_h][slot_w]: per
 *   element the same expressions, so slot b equals the per-image chain bit for bit (image 0.0 / target 255 outside the crop, bytes 0 /
 *   target 0 where the crop window reaches past the resized photo).  Two launches whatever B; one when max_hpass_pixels is 0.
 * table_dev: DEVICE memory, B rows of egm_train_desc followed by the int32 tables the rows point to; every *_off of a row counts
 *   int32 elements from table_dev itself (one blob, one upload).  With sy = y + top, sx = x + left, yy = vflip ? oh-1-sy : sy and
 *   xx = hflip ? ow-1-sx : sx over the crop, the visible resized rows are [y0, y0 + ny) and the visible resized columns [c0, c0 + nc);
 *   all tables are cut to those windows:
 *     xb_off  int32 [nc][2]       (first tap, tap count) of resized column c0 + i over the W source columns   (xksize > 0 only)
 *     xc_off  int32 [nc][xksize]  its 22-bit fixed-point coefficients                                          (xksize > 0 only)
 *     yb_off  int32 [ny][2], yc_off int32 [ny][yksize]: the same for resized row y0 + i over the H source rows  (yksize > 0 only)
 *     xnn_off int32 [nc], ynn_off int32 [ny]: source column / row of the mask for resized column c0 + i / row y0 + i (NEAREST)
 *   xksize == 0 (ow == W) or yksize == 0 (oh == H) flags that pass as the identity.  [r0, r0 + nr) are the source rows the vertical
 *   taps of the visible rows touch (the visible rows themselves without a vertical pass).  The horizontal pass writes uint8
 *   [nr][nc][3] at workspace + ws_off; an image without one uses no workspace.
 * slot_h >= max_crop_h, slot_w >= max_crop_w (the largest crop of the batch).  workspace: uint8 [workspace_bytes], may be NULL when
 *   max_hpass_pixels (the largest nr * nc among the images with a horizontal pass) is 0.  mean3/std3 are HOST pointers.
 *   B * 3 * slot_h * slot_w < 2^31 and workspace_bytes < 2^31, otherwise EGM_ERR_ARG.  Rows are built by egm_unet_amd.data.plan_train_batch;
 *   the kernels clamp every table value into its window, so a wrong row gives wrong pixels, never an access outside the buffers it names. */
typedef struct egm_train_desc {
    const void* img;            /* uint8 [H][W][3] */
    const void* mask;           /* uint8 [H][W] */
    int H, W, oh, ow;           /* source size, resized size */
    int hflip, vflip, top, left;
    int crop_h, crop_w, r0, nr;
    int c0, nc, y0, ny;
    int xksize, yksize;
    long long ws_off;           /* bytes into the workspace */
    int xb_off, xc_off, yb_off, yc_off, xnn_off, ynn_off;
} egm_train_desc;               /* 120 bytes */
int egm_train_batch_u8(const egm_train_desc* table_dev, int B, int slot_h, int slot_w, int max_crop_h, int max_crop_w,
                       float* out_img_bchw, long long* out_target_bhw, const float* mean3_host, const float* std3_host,
                       void* workspace, long long workspace_bytes, long long max_hpass_pixels, egm_stream_t s);

/* ---- CLIPSeg decoder training (models/clipseg.py:380-420,452-496; experiments/phrasecut.yaml:1-47) ------------------
 * The backward matrix products run on egm_gemm over transposed copies (egm_transpose: dst[b][c][r] = src[b][r][c]).
 * egm_relu_bwd: dst = g where out > 0.  egm_softmax_bwd_rows: dS = P*(dP - sum_j dP_j P_j)*alpha per row (P storage type,
 * dP fp32).  egm_layernorm_bwd: dx and per-block partials [egm_layernorm_bwd_blocks(rows)][2][D] of (dbeta, dgamma) for
 * egm_reduce_tiles.  egm_film_fwd/bwd: out = mul[b,:]*a + add[b,:] and its gradients.  egm_pixel_unshuffle: gradient of
 * egm_pixel_shuffle (rows of the tok_off leading tokens are zero).  egm_bce_logits_*: nn.BCEWithLogitsLoss(mean).
 * egm_adamw_multi: torch.optim.AdamW step over a device table of 48-byte {p, g, m, v, n, chunk0} entries. */
int egm_transpose(int dtype, const void* src, int rows, int cols, int ld_src, long long batch_stride_src, void* dst, int ld_dst,
                  long long batch_stride_dst, int batch, egm_stream_t s);
int egm_relu_bwd(int dtype, const void* g, const void* out, void* dst, long long n, egm_stream_t s);
int egm_softmax_bwd_rows(int dtype, const void* P, int ldp, const float* dP, int lddp, void* dS, int ldds, long long rows, int L,
                         float alpha, egm_stream_t s);
int egm_layernorm_bwd_blocks(long long rows);
int egm_layernorm_bwd(int dtype, const void* x, int ldx, const void* g, int ldg, const float* gamma, float eps, void* dx, int lddx,
                      float* partials, long long rows, int D, egm_stream_t s);
int egm_film_fwd(int dtype, const void* a, const void* mul, const void* add, void* out, int B, int L, int D, egm_stream_t s);
int egm_film_bwd(int dtype, const void* g, const void* a, const void* mul, void* da, void* dmul, void* dadd, int B, int L, int D,
                 egm_stream_t s);
int egm_pixel_unshuffle(int dtype, const float* dout, void* dy, int B, int g, int P, int tok_off, int Ltot, egm_stream_t s);
int egm_sum_f32(const float* x, long long n, float scale, float* partials, float* out, egm_stream_t s);
int egm_bce_logits_fwd(const float* x, const float* t, long long n, float* partials, float* loss, egm_stream_t s);
int egm_bce_logits_bwd(const float* x, const float* t, const float* grad_out, long long n, float* dx, egm_stream_t s);
int egm_adamw_chunk(void);
int egm_adamw_multi(const void* table_dev, int ntensors, long long total_chunks, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int step, egm_stream_t s);

/* ---- CLIPSeg decoder training: dropout, visual-prompt mask ---------------------------------------------------------------------
 * nn.TransformerEncoderLayer(dropout=0.1) in train mode (models/clipseg.py:421-422): out = residual + keep*x/(1-p), keep regenerated
 * from (seed, element index) by a counter-based hash, so the backward is the same call on the gradient (residual = NULL).
 * x/out may be fp32 (dtype EGM_F32) or bf16. */
int egm_dropout(int dtype, const void* x, const void* residual, void* out, long long n, float p, unsigned long long seed,
                egm_stream_t s);
/* CLIPDensePredTMasked (models/clipseg.py:500-525; forward_multihead_attention :111-117): the class token's attention row of every
 * (batch, head) is multiplied by a [nmask][ntok] mask, head bh taking mask row bh % nmask (the reference's repeat() pairing). */
int egm_attn_mask_cls(int dtype, void* probs, int ldp, long long head_stride, const float* mask, int nmask, int nbh, int ntok,
                      egm_stream_t s);

/* ---- CLIPSeg refined head, complex_trans_conv=True (models/clipseg.py:401-414; experiments/phrasecut.yaml:74 rd64-uni-refined) --------
 * Conv2d(rd, rd, 3, pad 1) -> ReLU -> ConvTranspose2d(rd, rd/2, 4, stride 4) -> ReLU -> ConvTranspose2d(rd/2, 1, 4, stride 4) on the g x g
 * token grid of a [B][Ltot][rd] (rows tok_off .. tok_off + g*g - 1; the leading class token is skipped), out fp32 [B][1][16g][16g].
 * Supported: patch 16 (ViT-B/16), rd 64 or 128, 1 <= g <= 32; anything else returns EGM_ERR_UNSUPPORTED.
 * egm_refine_pack: the fp32 parameters w0 [rd][rd][3][3], w1 [rd][rd/2][4][4], w2 [rd/2][1][4][4] -> packed, egm_refine_packed_elems(rd,
 *   patch) elements in `dtype` (operand layouts of the forward and backward products; rerun after every optimizer step).
 * egm_refine_fwd: ONE launch.  h (dtype [B][g*g][rd], the first ReLU's output, for the backward) may be NULL.
 * egm_refine_bwd: three launches from dout fp32 [B][1][16g][16g], the forward's a and h: da (dtype, shape of a, rows outside the grid 0)
 *   and the parameter gradients (fp32, parameter shapes; overwritten).  Weight gradients are per-slice slabs in the workspace
 *   (egm_refine_bwd_workspace() bytes) summed in fixed order: bitwise reproducible. */
long long egm_refine_packed_elems(int rd, int patch);
long long egm_refine_bwd_workspace(int B, int g, int rd, int patch);
int egm_refine_pack(int dtype, const float* w0, const float* w1, const float* w2, void* packed, int rd, int patch, egm_stream_t s);
int egm_refine_fwd(int dtype, const void* a, int tok_off, int Ltot, const void* packed, const float* b0, const float* b1,
                   const float* b2, void* h, float* out, int B, int g, int rd, int patch, egm_stream_t s);
int egm_refine_bwd(int dtype, const float* dout, const void* a, int tok_off, int Ltot, const void* h, const void* packed,
                   const float* b1, void* da, float* dw0, float* db0, float* dw1, float* db1, float* dw2, float* db2,
                   void* workspace, int B, int g, int rd, int patch, egm_stream_t s);

/* ---- CLIPSeg baseline head, CLIPDenseBaseline (models/clipseg.py:529-590) -------------------------------------------------------------
 * Per token of the activation x [B][Ltot][768] (rows tok_off .. tok_off + g*g - 1; the class token is skipped):
 *   u = x W_red^T + b_red;  f = mul[b] * u + add[b];  h = relu(f W1^T + b1);  a3 = h W2^T + b2;  out = ConvTranspose2d(rd -> 1, 16, 16)(a3)
 * with W_red [rd][768], W1 [rd2][rd], W2 [rd][rd2], Wt [rd][1][16][16] (fp32 parameters), mul / add [B][rd] in `dtype`, out fp32
 * [B][1][16g][16g].  Supported (egm_baseline_supported() == 1): patch 16, rd and rd2 multiples of 16 in 16 .. 128; dtype bf16 only.
 * Anything else returns EGM_ERR_UNSUPPORTED.
 * egm_baseline_pack: the four weights -> egm_baseline_packed_elems() bf16 elements (MFMA operand layouts; rerun after every optimizer step).
 * egm_baseline_fwd: ONE launch.  u ([B][g*g][rd]) and h ([B][g*g][rd2]) in `dtype` receive the saved tensors of the backward, or are both NULL.
 * egm_baseline_bwd: two launches from dout fp32 [B][1][16g][16g] and the forward's u, h (requires Ltot == tok_off + g*g): du (`dtype`,
 *   [B][Ltot][rd], the gradient of u; class-token rows 0), dmul / dadd (`dtype`, [B][rd]) and the fp32 gradients of Wt, bt, W2, b2, W1, b1
 *   (parameter shapes; overwritten).  Per-workgroup slabs in the workspace (egm_baseline_bwd_workspace() bytes) are summed in fixed
 *   order: bitwise reproducible.  The gradient of W_red / b_red (du^T x) is left to the caller. */
int egm_baseline_supported(int rd, int rd2, int patch);
long long egm_baseline_packed_elems(int rd, int rd2, int patch);
long long egm_baseline_bwd_workspace(int B, int g, int rd, int rd2, int patch);
int egm_baseline_pack(int dtype, const float* w_red, const float* w1, const float* w2, const float* wt, void* packed, int rd, int rd2,
                      int patch, egm_stream_t s);
int egm_baseline_fwd(int dtype, const void* x, int tok_off, int Ltot, const void* mul, const void* add, const void* packed,
                     const float* b_red, const float* b1, const float* b2, const float* bt, void* u, void* h, float* out, int B, int g,
                     int rd, int rd2, int patch, egm_stream_t s);
int egm_baseline_bwd(int dtype, const float* dout, const void* u, const void* h, const void* mul, const void* add, const void* packed,
                     const float* b2, void* du, int tok_off, int Ltot, float* dwt, float* dbt, float* dw2, float* db2, float* dw1,
                     float* db1, void* dmul, void* dadd, void* workspace, int B, int g, int rd, int rd2, int patch, egm_stream_t s);
/* egm_baseline_fwd_multi: the same head for K prompts on each of B activations, ONE launch (CLIPDenseBase.forward_multi).  mul / add are
 * [K][rd]; out is fp32 [B*K][1][16g][16g] with sequence b*K + k (= [B][K][16g][16g]).  Per token tile u = x W_red^T + b_red is computed
 * once per prompt group and every prompt of the group runs FiLM .. Wt on it; each prompt's output equals egm_baseline_fwd's with that
 * prompt's mul / add bit for bit.  prompts_per_group <= 0: chosen so that the grid covers the device (B = 1: one prompt per group).
 * Same support and dtype rules as egm_baseline_fwd. */
int egm_baseline_fwd_multi(int dtype, const void* x, int tok_off, int Ltot, const void* mul, const void* add, const void* packed,
                           const float* b_red, const float* b1, const float* b2, const float* bt, float* out, int B, int K, int g, int rd,
                           int rd2, int patch, int prompts_per_group, egm_stream_t s);

/* ---- CLIPSeg multi-prompt decoder (CLIPDenseBase.forward_multi, CLIPSegMultiLabel; csrc/clipseg_multi.hip) ----------------------------
 * B images, K prompts; decoder sequences are b-major (s = b*K + k), rows [L][D] per sequence, D a multiple of 4, 16-byte aligned buffers.
 * egm_film_fanout: out[b*K + k][t][:] = mul[k][:] * r[b][t][:] + add[k][:]  (the FiLM at cond_layer, B -> B*K sequences; same rounding
 *   as egm_film).  r [B][L][D], mul / add [K][D], out [B*K][L][D], all in `dtype`.
 * egm_bcast_add: a[b*K + k][t][:] += r[b][t][:]  (reduce_i(act_i) of the layers behind cond_layer, a GEMM over B*L rows only).
 * egm_sigmoid_affine: x[n][c][:] = offset + scale[c] * sigmoid(x[n][c][:]) in place; x fp32 [N][C][HW] (HW a multiple of 4), scale fp32 [C]
 *   (CLIPSegMultiLabel: offset -10, scale 3 for background, else 1). */
int egm_film_fanout(int dtype, const void* r, const void* mul, const void* add, void* out, int B, int K, int L, int D, egm_stream_t s);
int egm_bcast_add(int dtype, void* a, const void* r, int B, int K, int L, int D, egm_stream_t s);
int egm_sigmoid_affine(float* x, const float* scale, float offset, int N, int C, long long HW, egm_stream_t s);
/* Decoder training on K prompts (CLIPDenseBase.forward_multi_train).  fp32 accumulation, one rounding per output, no allocation, no
 * synchronisation, no atomics: results are bitwise reproducible.
 * egm_bcast_add_out: out[b*K + k][t][:] = a[b*K + k][t][:] + r[b][t][:], egm_bcast_add out of place (same expression and rounding).
 * egm_group_sum: out[b][t][:] = sum_k g[b*K + k][t][:] (k ascending), the gradient of egm_bcast_add's r.
 * egm_film_fanout_bwd: from g [B*K][L][D] (the gradient of egm_film_fanout's out), r and mul:
 *   dr[b][t][:] = sum_k g[b*K + k][t][:] * mul[k][:] (k ascending),  dmul[k][:] = sum_{b,t} g[b*K + k][t][:] * r[b][t][:],
 *   dadd[k][:] = sum_{b,t} g[b*K + k][t][:];  dr [B][L][D], dmul / dadd [K][D], all in `dtype`.  One workgroup per (image, token tile)
 *   writes fp32 partials [block][2][K][D] into ws (egm_film_fanout_bwd_workspace() bytes), a second launch adds them in block order. */
int egm_bcast_add_out(int dtype, const void* a, const void* r, void* out, int B, int K, int L, int D, egm_stream_t s);
int egm_group_sum(int dtype, const void* g, void* out, int B, int K, int L, int D, egm_stream_t s);
long long egm_film_fanout_bwd_workspace(int dtype, int B, int K, int L, int D);
int egm_film_fanout_bwd(int dtype, const void* g, const void* r, const void* mul, void* dr, void* dmul, void* dadd, void* ws, int B, int K,
                        int L, int D, egm_stream_t s);

/* ---- CLIPSeg visual prompts (csrc/vprompt.hip, egm_unet_amd/prompts.py) ------------------------------------------------
 * The support image of a one-shot query from a decoded photo and its mask.  fp32, a fixed evaluation order with one rounding per
 * operation (tests/vprompt_oracle.py restates it); no allocation, no synchronisation with the host; K images per launch; S in 8 .. 8192.
 * egm_vprompt_mask_f32: uint8 masks [K][H][W] -> coverage m [K][S][S] in [0, 1], the separable filter of data.float_filter_tables
 *   (bounds int32 [S][2], weights fp32 [S][ksize] per axis, at most 64 taps) on the 0/1 indicator, columns first; value v is object when
 *   bit v of the 256-bit set lut8_host (8 words, host memory) is set.  tmp_khs: fp32 [K][H][S].  Two launches; the second also resets the
 *   K box records box_k4 (int32 [K][4] = y0, y1, x0, x1 with exclusive ends) to the empty box {S, 0, S, 0}.
 * egm_vprompt_blend_f32: x [K][3][S][S], m -> out [K][3][S][S] by mode 0 overlay, 1 highlight, 2 highlight2, 3 shape, 4 image_only,
 *   5 image_black, 6 x*m + bg_fac * blur(x) * (1 - m) - sub; blur: the separable 15-tap filter taps15_host (host memory), rows first,
 *   reflect-101 borders (blur == 0: blur(x) = x).  The same launch grows box_k4[k] to the extents of m > 0 with vector atomics, so
 *   egm_vprompt_mask_f32 has to run before it on the stream.  One launch.
 * egm_vprompt_crop_f32: the square window around box_k4[k] widened by cnum / 1024 of its side per side (the whole image for an empty
 *   box), resampled to S x S bilinearly from integer taps; pixels outside the image read 0.  Not in place.  One launch.
 * egm_cond_mix_f32: out[g][:] = w * text[g][:] + (1 - w) * mean(vis[group_off[g] .. group_off[g + 1]][:]), the mean a left-to-right sum
 *   divided once; text_gd == NULL: the mean alone.  vis [K][D], group_off int32 [G + 1] on the device, ascending from 0 to K. */
int egm_vprompt_mask_f32(const void* masks_khw, int K, int H, int W, float* m_kss, int S, const int* xbounds, const float* xweights,
                         int xksize, const int* ybounds, const float* yweights, int yksize, const unsigned int* lut8_host, float* tmp_khs,
                         int* box_k4, egm_stream_t s);
int egm_vprompt_blend_f32(const float* x_k3ss, const float* m_kss, float* out_k3ss, int* box_k4, int K, int S, int mode,
                          const float* taps15_host, int blur, float bg_fac, float sub, egm_stream_t s);
int egm_vprompt_crop_f32(const float* src_k3ss, const int* box_k4, float* out_k3ss, int K, int S, int cnum, egm_stream_t s);
int egm_cond_mix_f32(float* out_gd, const float* vis_kd, const int* group_off, const float* text_gd, float w, int G, int K, int D,
                     egm_stream_t s);

/* ---- Guided upsampling: photo-guided mask edges at photo size (csrc/guided.hip, egm_unet_amd/refine.py) ----------------
 * The fast guided filter (He, Sun, Tang: "Guided Image Filtering" 2013, "Fast Guided Filter" 2015) with a three-colour guide.  fp32, a
 * fixed evaluation order with one rounding per multiply, add, subtract and divide and no FMA (tests/guided_oracle.py restates it).
 * Box mean of a channel X at (y, x) with radius r, the window clipped to the image: t[y'][x] = X[y'][xlo], t = t + X[y'][k] for k
 * ascending to xhi; u = t[ylo][x], u = u + t[k][x] for k ascending to yhi; mean = u / (float)(rows * columns of the window).
 * egm_guided_coefs_f32: guide fp32 [N][3][h][w] (the low-resolution photo in the caller's units) and EXACTLY ONE of scores fp32
 *   [N][C][h][w] and cls uint8 [N][h][w] (read as the one-hot scores S_c = cls == c ? 1 : 0) -> A_out fp32 [N][h][w][4C], per pixel and
 *   class (a0, a1, a2, b).  With m(.) the box mean: s_ij = m(G_i G_j) - m(G_i) m(G_j), + eps_i on the diagonal; v_i = m(G_i S_c) -
 *   m(G_i) m(S_c); the cofactors c00 = s11 s22 - s12 s12, c01 = s02 s12 - s01 s22, c02 = s01 s12 - s02 s11, c11 = s00 s22 - s02 s02,
 *   c12 = s01 s02 - s00 s12, c22 = s00 s11 - s01 s01; det = (s00 c00 + s01 c01) + s02 c02; a0 = ((c00 v0 + c01 v1) + c02 v2) / det, a1
 *   from the row (c01, c11, c12), a2 from (c02, c12, c22); b = ((m(S_c) - a0 m(G_0)) - a1 m(G_1)) - a2 m(G_2).  A = the box mean, same
 *   r, of those 4C channels.  workspace: egm_guided_workspace(N, C, h, w) bytes of device memory (the unsmoothed coefficients).
 *   TWO launches whatever N and C: a workgroup owns a 16 x 16 tile of one image with an r-pixel halo in LDS (at most 111 KiB).
 * egm_guided_apply_u8: imgs uint8 [N][H0][W0][3] contiguous (image n starts n*H0*W0*3 bytes in, at whatever alignment that is) ->
 *   mask_out uint8 [N][H0][W0] and, when q_out != NULL, q_out fp32 [N][C][H0][W0].  Per photo pixel I_i = (float)byte_i * scale_i +
 *   offset_i; each of the 4C channels of A is sampled with the expression and the tables of egm_tta_views_f32 (yi [H0][2], yl [H0], xi
 *   [W0][2], xl [W0] from (h, w) to (H0, W0), any ratio); q_c = ((a0 I_0 + a1 I_1) + a2 I_2) + b; mask = lut[argmax_c q_c], ties to the
 *   lowest class, lut 256 bytes or NULL = the class id.  ONE launch, no atomics; the photo is read as dwords where a row's address
 *   allows it, the mask leaves in non-temporal dwords (bytes on ragged ends and unaligned rows); the part of A behind a strip of
 *   4 x 256 photo pixels is staged in LDS where it is at most 32 KiB, else gathered; table indices are clamped.  h*w*C < 2^29.
 * Limits: 1 <= r <= 16, 1 <= C <= 8, N <= 65535, every side <= 32767, eps_i finite and > 0; A and the workspace 16-byte aligned.  Bad
 *   scalars, null pointers and both or neither of scores and cls return EGM_ERR_ARG with a message before any launch.  Nothing waits
 *   for the device; capturable on one stream.
 * egm_ensemble_fuse_dev_f32: egm_ensemble_fuse's `fused` (fp32 [N][C][H][W], the same expression, bit for bit) with alpha read from
 *   DEVICE memory, so a captured graph follows its value.  One launch. */
long long egm_guided_workspace(int N, int C, int h, int w);
int egm_guided_coefs_f32(const float* guide, const float* scores, const unsigned char* cls, int N, int C, int h, int w, int r, float eps0,
                         float eps1, float eps2, float* A_out, void* workspace, egm_stream_t s);
int egm_guided_apply_u8(const unsigned char* imgs, int N, int H0, int W0, const float* A, int C, int h, int w, const int* yi_dev,
                        const float* yl_dev, const int* xi_dev, const float* xl_dev, float scale0, float scale1, float scale2,
                        float offset0, float offset1, float offset2, const unsigned char* lut, unsigned char* mask_out, float* q_out,
                        egm_stream_t s);
int egm_ensemble_fuse_dev_f32(const float* clip_logits, const float* unet_logits, const float* alpha_dev, int N, int C, int hc, int wc,
                              int H, int W, float* fused, egm_stream_t s);

/* ---- Boundary loss: signed distance maps of the target made on the device (csrc/sdf.hip, train_utils/boundary_loss.py)
 * Kervadec et al., "Boundary loss for highly unbalanced segmentation" (MIDL 2019; Medical Image Analysis 2021).
 * egm_target_sdf_i64: target int64 [N][H][W], valid(p) = target(p) != ignore_index; classes = a HOST array of K distinct class ids >= 0,
 *   1 <= K <= 4.  s_out int32 [N][K][H][W], every cell written, exact: for p of class k, s = -min |p - q|^2 over the valid q of the
 *   same image that are not of class k; for p valid and not of class k, s = +min |p - q|^2 over the q of class k; s = 0 for an ignored
 *   p and wherever the minimum runs over nothing, which makes the whole plane of (n, k) zero when image n has no pixel of class k or
 *   no valid pixel outside it.  Every defined distance is >= 1.
 *   workspace: egm_sdf_workspace(N, H, W, K) bytes of device memory owned by the caller (1 + 4 K bytes per pixel of a row padded to 16:
 *   a byte of "is of class k" / "is valid and not of class k" bits and a 16-bit row distance per bit, 0xFFFF = none).
 *   Two launches per call whatever the content (rows, then columns); nothing waits for the device, for another workgroup or for
 *   another wave; no atomics; every device loop has a trip count of at most max(H, the chunks of a row); capturable on one stream.
 *   H, W <= 32767, H*W <= 2^30, N*H <= 2^31; otherwise, and for a null pointer, K outside 1..4, a negative or a repeated class id:
 *   EGM_ERR_ARG with a message before any launch.
 * egm_sdf_phi_f32: phi of n cells of s as an fp32 tensor, for inspection and tests (the loss passes make it on the fly).
 * egm_bloss_fwd: logits fp32 [N][C][H][W], sdf = s_out above for the same classes (ids in [0, C), C <= 16), target and ignore_index as
 *   above (read for the count of valid pixels only).  phi_k = sqrt((float)s) for s > 0, -(sqrt((float)-s) - 1) for s < 0, 0 for s = 0
 *   (the official one_hot2dist, correctly rounded fp32, never stored).  L_B = (1/D) sum_n sum_k sum_p phi_k(p) softmax(x[n,:,p])[class k],
 *   D = K * max(1, valid pixels of the batch), the count an integer.  out2 = {w L_B, L_B} with w = w_dev[0] read on the DEVICE, so a
 *   captured graph follows a new weight.  workspace: egm_bloss_workspace(N, C, H, W) bytes, 4-byte aligned, kept for the backward (per
 *   workgroup partial sums written with plain stores and summed in a fixed order in double, the counts, 1 / D).  Two launches.
 * egm_bloss_bwd: dlogits[n][j][p] = grad_out[0] (1 when NULL) * w / D * p_j ([j in classes] phi_j - sum_k phi_k p_k), exactly 0 at an
 *   ignored pixel; every element written (non-temporal stores).  One launch.  N <= 65535.  Four pixels per lane where H*W is a multiple
 *   of 4 and logits, sdf and dlogits are 16-byte aligned, one otherwise, in both passes: the same dlogits either way (the forward
 *   groups its partial sums differently, so L_B agrees within rounding). */
long long egm_sdf_workspace(int N, int H, int W, int K);
int egm_target_sdf_i64(const long long* target, int N, int H, int W, const int* classes, int K, long long ignore_index, void* workspace,
                       int* s_out, egm_stream_t s);
int egm_sdf_phi_f32(const int* sdf, long long n, float* phi, egm_stream_t s);
long long egm_bloss_workspace(int N, int C, int H, int W);
int egm_bloss_fwd(const float* logits, const int* sdf, const long long* target, const int* classes, int K, int N, int C, int H, int W,
                  long long ignore_index, const float* w_dev, void* workspace, float* out2, egm_stream_t s);
int egm_bloss_bwd(const float* logits, const int* sdf, const int* classes, int K, int N, int C, int H, int W, const void* workspace,
                  const float* grad_out, const float* w_dev, float* dlogits, egm_stream_t s);

/* ---- Distillation against a frozen teacher (csrc/distill.hip, train_utils/distill_loss.py)
 * Hinton, Vinyals, Dean, "Distilling the knowledge in a neural network" (2015).
 * Student logits x fp32 [N][C][H][W], teacher logits z of teacher_dtype (EGM_F32 or EGM_BF16) in the same shape, C <= 16; target int64
 * [N][H][W] or NULL.  A pixel is valid when (target == NULL or has_ignore == 0 or target != ignore_index) and
 * (tau == 0 or max_c softmax(z)_c >= tau, at temperature 1), tau = tau_dev[0] read on the DEVICE.  With q = softmax(x / T),
 * p = softmax(z / T), V = the valid pixels of the batch (an integer count):
 *   L_KD = T^2 / max(1, V) * sum over the valid pixels of sum_c p_c (log p_c - log q_c),  log-softmax in the max-subtracted form
 * egm_distill_fwd: out2 = {w L_KD, L_KD} with w = w_dev[0] read on the device, valid_out[0] = V (NULL: not written); no valid pixel
 *   gives 0.  workspace: egm_distill_workspace(N, C, H, W) bytes, 4-byte aligned, kept for the backward (per workgroup partial sums
 *   written with plain stores and summed in a fixed order in double, the counts, 1 / max(1, V)).  Two launches, no atomics.
 * egm_distill_bwd: dlogits[n][c][p] = grad_out[0] (1 when NULL) * w * T / max(1, V) * (q_c - p_c) at a valid pixel, exactly 0
 *   elsewhere; both softmaxes are recomputed, every element is written.  One launch.
 *   Four pixels per lane where C <= 4, H*W is a multiple of 4 and every plane starts at a boundary of its four-pixel load (16 bytes of
 *   fp32, 8 of bf16), one otherwise: the same dlogits either way.  egm_distill_blocks() = the workgroups per image of both passes.
 * egm_pseudo_target_i64: out int64 [N][H][W] = argmax_c z (ties to the lowest class, as egm_argmax_u8) where the confidence
 *   max_c softmax(z)_c >= tau and existing (int64 [N][H][W] or NULL) is not ignore_index there; ignore_index elsewhere.  One launch.
 * A null pointer, C > 16, T <= 0, N > 65535 or another teacher_dtype: EGM_ERR_ARG with a message before any launch. */
int egm_distill_blocks(void);
long long egm_distill_workspace(int N, int C, int H, int W);
int egm_distill_fwd(const float* logits, const void* teacher, int teacher_dtype, const long long* target, int N, int C, int H, int W,
                    int has_ignore, long long ignore_index, float temperature, const float* w_dev, const float* tau_dev, void* workspace,
                    float* out2, long long* valid_out, egm_stream_t s);
int egm_distill_bwd(const float* logits, const void* teacher, int teacher_dtype, const long long* target, int N, int C, int H, int W,
                    int has_ignore, long long ignore_index, float temperature, const float* w_dev, const float* tau_dev,
                    const void* workspace, const float* grad_out, float* dlogits, egm_stream_t s);
int egm_pseudo_target_i64(const void* teacher, int teacher_dtype, const long long* existing, int N, int C, int H, int W,
                          long long ignore_index, const float* tau_dev, long long* out, egm_stream_t s);
/* egm_renorm_resize_f32: x fp32 [N][3][H][W] normalised with one (mean, std) -> out fp32 [N][3][Sh][Sw] =
 *   F.interpolate(x * a_c + b_c, (Sh, Sw), mode="bilinear", align_corners=False, antialias=...) with the tables of
 *   data.float_filter_tables (egm_clip_preprocess_u8's contract); a3_host, b3_host: HOST arrays of the per-channel affine map.
 *   tmp[n][c][y][xo] = sum_j wx[xo][j] * fmaf(x[n][c][y][x0 + j], a_c, b_c), then out[n][c][yo][xo] = sum_j wy[yo][j] * tmp[n][c][y0 + j][xo];
 *   both sums start at 0 and take their taps in table order, each step one fmaf(weight, value, sum).  tmp: N * 3 * H * Sw floats.
 *   Two launches whatever N.  More than 64 taps on an axis: EGM_ERR_ARG with egm_clip_preprocess_batch_u8's message. */
int egm_renorm_resize_f32(const float* x_nchw, int N, int H, int W, float* out_nchw, int Sh, int Sw, const int* xbounds,
                          const float* xweights, int xksize, const int* ybounds, const float* yweights, int yksize, const float* a3_host,
                          const float* b3_host, float* tmp_nchw, egm_stream_t s);

/* ---- Stable radix sort of (key, value) pairs (csrc/sort.hip)
 * egm_sort_pairs_u32: keys, vals uint32 [S][L] -> keys_out, vals_out [S][L]: each of the S segments sorted ascending on the key bits
 *   [begin_bit, end_bit), 0 <= begin_bit < end_bit <= 32 (the other bits travel with the key and are not looked at); elements with equal
 *   bits keep their input order (stable), so np.argsort(kind="stable") of the masked keys restates the permutation exactly and two calls
 *   give the same bits.  An LSD sort of 8 bits per pass over tiles of 2048 elements: ceil((end_bit - begin_bit) / 8) passes of three
 *   launches (tile histograms, an exclusive scan of the [segment][digit][tile] table, a scatter whose in-tile rank comes from 64-bit
 *   __ballot matches and per-wave LDS counters), all segments of a pass in one launch.  No workgroup waits for another, every loop is
 *   bounded by the arguments, no atomics on global memory; capturable on one stream.
 *   workspace: egm_sort_pairs_workspace(S, L) bytes of device memory owned by the caller, 4-byte aligned (two ping-pong planes and
 *   the table).  The outputs must not be the inputs (the inputs are left as they were).  1 <= S <= 65535, 1 <= L < 2^31; otherwise,
 *   and for a null pointer or an empty bit range: EGM_ERR_ARG with a message before any launch. */
long long egm_sort_pairs_workspace(int S, long long L);
int egm_sort_pairs_u32(const unsigned int* keys, const unsigned int* vals, int S, long long L, int begin_bit, int end_bit, void* workspace,
                       unsigned int* keys_out, unsigned int* vals_out, egm_stream_t s);

/* ---- Lovasz-Softmax loss (csrc/lovasz.hip, train_utils/lovasz_loss.py)
 * Berman, Triki, Blaschko, "The Lovasz-Softmax loss" (CVPR 2018): the convex extension of the Jaccard loss.
 * logits fp32 [N][C][H][W], C <= 16; target int64 [N][H][W], valid(p) = target(p) != ignore_index; classes = a HOST array of K distinct
 * ids in [0, C), 1 <= K <= 16.  per_image = 0: one segment, the batch (S = 1, L = N H W); else S = N segments of L = H W.  N H W < 2^31.
 * egm_lovasz_errors: per class k and pixel p, fg = [target(p) == id_k], e = |fg - softmax(x)[id_k]| in fp32 (0 at an ignored pixel);
 *   keys [K][N][H][W] = (~bits(e) & 0x3FFFFFFF) | fg << 30 | valid << 31, vals = the pixel's flat index (n, h, w) within its segment,
 *   e_out (may be NULL) the fp32 e plane [K][N][H][W].  One launch.
 * egm_lovasz_coefs: the errors, their stable sort over key bits [0, 30) (descending e, ties by ascending pixel index), and along the
 *   sorted order of each (class, segment) the inclusive counts F_j of valid foreground and V_j of valid elements (exact uint32), G = the
 *   segment's foreground.  J(F, V) = 1 - (G - F) / (G + V - F); for a valid element g_j = J(F_j, V_j) - J(F_j - fg_j, V_j - 1), the
 *   second term 0 when V_j == 1, in double, rounded once to fp32; g = 0 for an ignored element.  coef [K][N][H][W] fp32, every element
 *   written at the pixel's own place: sign(p_c - fg) g (0 where e == 0).  4 * 3 + 4 launches whatever N, K, the content and per_image.
 * egm_lovasz_fwd: the same, then L_{s,k} = sum_j e_j g_j (one double partial per workgroup, summed in a fixed order in double),
 *   L_s = (1 / P_s) sum over the counted classes (present != 0: those with G_{s,k} > 0, decided on the device; else all K), 0 when
 *   P_s = 0, L = (1 / S) sum_s L_s.  out2 = {w L, L} with w = w_dev[0] read on the DEVICE.  4 * 3 + 5 launches.
 *   workspace: egm_lovasz_workspace(N, C, H, W, K, per_image) bytes, 16-byte aligned, kept for the backward (it holds, per class and
 *   segment, 1 / (S P_s) where the class is counted and 0 where it is not).
 * egm_lovasz_bwd: dlogits[n][j][p] = grad_out[0] (1 when NULL) * w * sum_k scale_{k,s} coef_k(p) p_{id_k} ([id_k == j] - p_j), exactly
 *   0 at an ignored pixel; every element written (non-temporal stores).  One launch.
 * Nothing waits for the device or for another workgroup; no atomics on global memory; capturable on one stream.  A null pointer,
 * C > 16, K outside 1..16, an id outside [0, C), a repeated id, N H W >= 2^31, N > 65535 or a misaligned workspace: EGM_ERR_ARG with a
 * message before any launch. */
long long egm_lovasz_workspace(int N, int C, int H, int W, int K, int per_image);
int egm_lovasz_errors(const float* logits, const long long* target, const int* classes, int K, int N, int C, int H, int W,
                      long long ignore_index, int per_image, unsigned int* keys, unsigned int* vals, float* e_out, egm_stream_t s);
int egm_lovasz_coefs(const float* logits, const long long* target, const int* classes, int K, int N, int C, int H, int W,
                     long long ignore_index, int per_image, void* workspace, float* e_out, float* coef, egm_stream_t s);
int egm_lovasz_fwd(const float* logits, const long long* target, const int* classes, int K, int N, int C, int H, int W,
                   long long ignore_index, int per_image, int present, const float* w_dev, void* workspace, float* coef, float* out2,
                   egm_stream_t s);
int egm_lovasz_bwd(const float* logits, const float* coef, const int* classes, int K, int N, int C, int H, int W, int per_image,
                   const void* workspace, const float* grad_out, const float* w_dev, float* dlogits, egm_stream_t s);

/* ---- Lovasz hinge loss (csrc/lovasz_hinge.hip, train_utils/lovasz_loss.py)
 * The same paper's lovasz_hinge: the convex extension of the Jaccard loss of one binary score map per image.
 * Scores as for egm_sweep_hist.  C == 1: logits fp32 [N][H][W], s = x[n][p] (c_pos, c_neg ignored; a [N][K][H][W] tensor is N K
 * images).  C >= 2: logits fp32 [N][C][H][W], s = x[n][c_pos][p] - x[n][c_neg][p], one fp32 subtraction, 0 <= c_pos != c_neg < C.
 * target, of the score's shape [N][H][W]: target_f32 != 0: fp32, ignored iff t == (float)ignore_index (tested first), else positive
 * iff t > 0.5; target_f32 == 0: int64, ignored iff t == ignore_index, positive iff t == positive, every other value negative.
 * use_ignore == 0: nothing is ignored.  per_image = 0: one segment of all images (S = 1, L = N H W); else S = N segments of L = H W.
 * N H W < 2^31, N <= 65535.
 * egm_lovasz_hinge_errors: sigma = +1 at a positive pixel, -1 otherwise; e = 1 - s sigma in fp32 (one rounding); r = e where the pixel
 *   is valid and e > 0, else +0; keys [N][H][W] = (~bits(r) & 0x7FFFFFFF) | fg << 31 with fg = valid and positive, vals = the pixel's
 *   flat index within its segment, e_out (may be NULL) the fp32 plane of e, of every pixel, ignored ones included.  One launch.
 * egm_lovasz_hinge_coefs: the errors, their stable sort over key bits [0, 31) (descending r, ties by ascending pixel index), and along
 *   the sorted order of each segment F_j, the inclusive count of fg; G = the segment's fg; J(F, V) = 1 - (G - F) / (G + V - F);
 *   g_j = J(F_j, j) - J(F_j - fg_j, j - 1), the second term 0 at j = 1, in double, rounded once to fp32.  coef [N][H][W] fp32, every
 *   element written at the pixel's own place: -sigma g where r > 0, else 0.  4 * 3 + 4 launches whatever N, the content and per_image.
 * egm_lovasz_hinge_fwd: the same, then L_s = sum_j r_j g_j (one double partial per workgroup, summed in a fixed order in double; 0 for
 *   a segment with no valid pixel, which still counts), L = (1 / S) sum_s L_s.  out2 = {w L, L} with w = w_dev[0] read on the DEVICE.
 *   4 * 3 + 5 launches.  workspace: egm_lovasz_hinge_workspace(N, H, W, per_image) bytes, 16-byte aligned; the backward does not need it.
 * egm_lovasz_hinge_bwd: m = (grad_out[0] (1 when NULL) * w) * (1.0f / S), fp32 products in this order.  C == 1: dlogits[n][p] =
 *   m coef[n][p]; C >= 2: dlogits[n][c_pos] = m coef, dlogits[n][c_neg] = -(m coef), every other channel +0.  Every element written
 *   (non-temporal stores); no additions.  One launch.
 * Nothing waits for the device or for another workgroup; no atomics on global memory; capturable on one stream.  A null pointer, a bad
 * shape, N H W >= 2^31, N > 65535, equal or out-of-range channels (C >= 2) or a misaligned workspace: EGM_ERR_ARG with a message before
 * any launch. */
long long egm_lovasz_hinge_workspace(int N, int H, int W, int per_image);
int egm_lovasz_hinge_errors(const float* logits, const void* target, int target_f32, int N, int C, int c_pos, int c_neg, int H, int W,
                            long long positive, long long ignore_index, int use_ignore, int per_image, unsigned int* keys,
                            unsigned int* vals, float* e_out, egm_stream_t s);
int egm_lovasz_hinge_coefs(const float* logits, const void* target, int target_f32, int N, int C, int c_pos, int c_neg, int H, int W,
                           long long positive, long long ignore_index, int use_ignore, int per_image, void* workspace, float* e_out,
                           float* coef, egm_stream_t s);
int egm_lovasz_hinge_fwd(const float* logits, const void* target, int target_f32, int N, int C, int c_pos, int c_neg, int H, int W,
                         long long positive, long long ignore_index, int use_ignore, int per_image, const float* w_dev, void* workspace,
                         float* coef, float* out2, egm_stream_t s);
int egm_lovasz_hinge_bwd(const float* coef, int N, int C, int c_pos, int c_neg, int H, int W, int per_image, const float* grad_out,
                         const float* w_dev, float* dlogits, egm_stream_t s);

/* ---- Exact ranking scores of binary logits (csrc/rank.hip, egm_unet_amd/rank.py)
 * Step-wise average precision with one threshold per distinct score, the exact AUROC numerator and the best foreground IoU over every
 * distinct score, of S segments (an evaluation set, or one image each) of L elements.
 * egm_rank_keys: scores, target, target_f32 and target_cls exactly as for egm_sweep_hist (C == 1 or the fp32 difference of two
 *   channels; uint8 through target_cls or fp32 cut at 0.5; odd HW, samples at any 4-byte offset); 1 <= N <= 65535, 1 <= HW < 2^31.
 *   With s' = the score, NaN replaced by -inf and -0 by +0, and b its bits: key = b where s' is negative, ~b & 0x7FFFFFFF otherwise
 *   (the complement of the order-preserving map), so ascending keys are descending scores, equal keys are scores that compare equal in
 *   fp32, and every kept key is <= 0xFF800000; a dropped pixel gets key 0xFFFFFFFF.  val = positive | kept << 1.  keys, vals: uint32,
 *   element (n, i) written at [offset + n HW + i] (offset >= 0: a batch's place in a larger plane).  One launch.
 * egm_rank_scores: keys, vals uint32 [S][L] as egm_rank_keys makes them (a kept element's key below every dropped one's).  Their
 *   stable sort over all 32 key bits; along the sorted order of a segment F_j = the inclusive count of positives, V_j = j + 1 (kept
 *   elements come first); an element is a group end when it is kept and its successor is missing, not kept or has another key.  Over
 *   the group ends g = 1..Gd in order, with TP_g = F, FP_g = V - F there and TP_0 = FP_0 = 0, P and Nn the kept positives / negatives:
 *     ap_sum = sum_g (TP_g - TP_{g-1}) TP_g / (TP_g + FP_g) in double (one partial per workgroup, summed in a fixed order);
 *     auc2 = sum_g (FP_g - FP_{g-1}) (TP_{g-1} + TP_g), exact uint64 (AUROC = auc2 / (2 P Nn));
 *     best = the g maximising TP_g / (P + FP_g), compared exactly by uint64 cross-multiplication, the first (highest score) on a tie.
 *   out_u64 [S][8] = {P, Nn, Gd, auc2, best_tp, best_fp, best_key, 0} (best_* all 0 when P == 0), out_f64 [S] = ap_sum / P (0 when
 *   P == 0).  A segment with nothing kept gives zeros.  skeys_out, tp_out: uint32 [S][L] or NULL: the sorted keys and F_j of every
 *   element (stage outputs for tests).  workspace: egm_rank_workspace(S, L) bytes, 16-byte aligned (about 16 bytes per element).
 *   4 * 3 + 4 launches whatever S, L and the content: the sort, then tile counts, a scan per segment, apply, finalize.
 * Nothing waits for the device or for another workgroup; no atomics on global memory; capturable on one stream.  1 <= S <= 65535,
 * 1 <= L < 2^31.  A null pointer (other than skeys_out, tp_out), a bad shape, equal or out-of-range channels (C >= 2), a negative offset
 * or a misaligned workspace: EGM_ERR_ARG with a message before any launch. */
int egm_rank_keys(const float* scores, int N, int C, int c_pos, int c_neg, long long HW, const void* target, int target_f32,
                  const unsigned char* target_cls, unsigned int* keys, unsigned int* vals, long long offset, egm_stream_t s);
long long egm_rank_workspace(int S, long long L);
int egm_rank_scores(const unsigned int* keys, const unsigned int* vals, int S, long long L, void* workspace, unsigned long long* out_u64,
                    double* out_f64, unsigned int* skeys_out, unsigned int* tp_out, egm_stream_t s);

/* ---- CLIPSeg training batches: object crop, resize, jitter (csrc/clipseg_batch.hip, egm_unet_amd/clipseg_data.py)
 * B ragged uint8 photos [H_b][W_b][3] with masks [H_b][W_b] (nonzero = object) -> img fp32 [B][3][S][S], seg fp32 [B][1][S][S] of 0 / 1
 * and choice int32 [B][3] = (off_y, off_x, exceed), the sample recipe of datasets/phrasecut.py:66-111, 263-311.  Each entry point below
 * is ONE launch whatever B (egm_color_jitter_f32 with stages == 3: two), none waits for the device, none uses atomics.
 * table_dev: DEVICE memory, B rows of egm_clipseg_batch_desc followed by the int32 / fp32 tables the rows point to; every *_off of a
 *   row counts 4-byte elements from table_dev itself (one blob, one upload), except prof_off, which counts int32 elements of profile_dev.
 *   The crop window is win_h x win_w: m x m with m = min(H, W) sliding along axis 1 (x) when W > H, else along axis 0 (y); axis -1:
 *   no object crop, the window is the photo (win_h = H, win_w = W) and the choice is (0, 0, 0).  With L the photo's side along the axis:
 *     cand_off  int32 [ncand]   the candidate offsets along the axis, in the order they were drawn
 *     prof_off  int32 [L] line counts, then [L + 1] their exclusive prefix sums (written by egm_clipseg_choose)
 *     yi_off int32 [S][2], yl_off fp32 [S]: per output row the two source rows (i0, i1) RELATIVE TO THE WINDOW'S ORIGIN and the weight l1
 *       of i1 (align_corners=True: scale = (float)(win - 1) / (float)(S - 1), src = scale * dst, i0 = (int)src, i1 = min(i0 + 1, win - 1),
 *       l1 = src - i0, all fp32); xi_off, xl_off: the same for the columns
 *     ynn_off, xnn_off int32 [S]: the mask's nearest source row / column, min((int)floor(dst * ((float)win / (float)S)), win - 1)
 * egm_mask_profile_u8: profile_dev[prof_off + i] = the number of nonzero mask bytes of line i of the axis (column i over all rows for
 *   axis 1, row i over all columns for axis 0); rows with axis -1 are skipped.  max_units: the largest of ceil(W / 256) (axis 1) and
 *   ceil(H / 4) (axis 0) over the batch, the work items of one image.
 * egm_clipseg_choose: window sum of candidate c = prefix[o_c + m] - prefix[o_c] with o_c clamped into [0, L - m]; the first c with
 *   sum > thresh is taken (exceed 0); if there is none, the c with the largest sum, the earliest on a tie (exceed 1).  choice_b3[b] =
 *   (o, 0, exceed) for axis 0, (0, o, exceed) for axis 1, (0, 0, 0) for axis -1 or ncand <= 0 (profile_dev may then be NULL).
 * egm_clipseg_batch_u8: choice_b3 is read on the DEVICE and clamped into [0, L - m].  Per output pixel and channel, from the four bytes
 *   a, b (row i0; columns i0, i1), c, d (row i1) as floats: l0 = 1 - l1, top = lx0 a + lx1 b, bot = lx0 c + lx1 d, v = (ly0 top + ly1 bot)
 *   / 255, one fp32 rounding per operation, no FMA.  seg = 1 where the mask byte at the nearest indices is nonzero and negative == 0, else 0.
 *   order_dev == NULL (then factors_dev == NULL too): img = (v - mean_c) / std_c, finished.  Otherwise order_dev int32 [B][4] is a
 *   permutation of the operations 0 brightness, 1 contrast, 2 saturation, 3 hue and factors_dev fp32 [B][8] = (r_0 .. r_3, q_0 .. q_3)
 *   with r = (float)f, q = (float)(1.0 - f) (r_3 = the hue shift): the operations in front of the contrast are applied, img receives the
 *   values UN-normalised and partials[b][t] (double [B][egm_color_jitter_tiles(S, S)]) the gray sum of tile t of 1024 consecutive pixels;
 *   egm_color_jitter_f32 with stages == 2 finishes the batch.  mean3 / std3 are HOST pointers.
 * egm_color_jitter_f32: torchvision's ColorJitter on fp32 [B][3][H][W] in [0, 1], tensor formulas, one fp32 rounding per operation:
 *   gray g = (0.2989 R + 0.587 G) + 0.114 B; brightness clamp(r x, 0, 1); saturation clamp(r x + q g, 0, 1); contrast clamp(r x + q mean,
 *   0, 1), mean = the image's mean of g at that point of the chain: per tile ((g0 + g1) + g2) + g3 per lane of 4 consecutive pixels in
 *   double, the xor butterfly 32, 16 .. 1 over the 64 lanes, the 4 waves in ascending order; the tiles in ascending order; divided by
 *   H W in double and rounded once; hue: _rgb2hsv, h = remainder(h + r_3, 1), _hsv2rgb (tests/clipseg_batch_oracle.py restates all of it).
 *   stages & 1: x -> out through the operations in front of the contrast, and the partials (x == out allowed); stages & 2: the contrast
 *   and what follows in place on out, then (x - mean_c) / std_c when mean3_host / std3_host (HOST pointers, both or neither) are given.
 * Limits: B <= 65535; H W 3 < 2^31 per photo (the host plan checks it); B 3 S S < 2^31; 2 <= S <= 32767; any number of lines and
 *   candidates that fits the tables (a slide axis of 8192 lines with 1000 candidates is tested).  Bad scalars and null pointers return
 *   EGM_ERR_ARG with a message before any launch.  The kernels clamp the device-chosen offset, every candidate, every tap and nearest
 *   index into its window and the window into the photo, and read an operation id & 3: a wrong row gives wrong pixels, never an access
 *   outside the buffers it names. */
typedef struct egm_clipseg_batch_desc {
    const void* img;            /* uint8 [H][W][3] */
    const void* mask;           /* uint8 [H][W] */
    int H, W, win_h, win_w;
    int axis, ncand, thresh, negative;
    int cand_off, prof_off;
    int yi_off, yl_off, xi_off, xl_off, ynn_off, xnn_off;
} egm_clipseg_batch_desc;       /* 80 bytes */
int egm_color_jitter_tiles(int H, int W);
int egm_mask_profile_u8(const egm_clipseg_batch_desc* table_dev, int B, int max_units, int* profile_dev, egm_stream_t s);
int egm_clipseg_choose(const egm_clipseg_batch_desc* table_dev, int B, int* profile_dev, int* choice_b3, egm_stream_t s);
int egm_clipseg_batch_u8(const egm_clipseg_batch_desc* table_dev, int B, int S, const int* choice_b3, const int* order_dev,
                         const float* factors_dev, float* out_img_b3ss, float* out_seg_b1ss, double* partials,
                         const float* mean3_host, const float* std3_host, egm_stream_t s);
int egm_color_jitter_f32(const float* x_b3hw, float* out_b3hw, int B, int H, int W, const int* order_dev, const float* factors_dev,
                         double* partials, const float* mean3_host, const float* std3_host, int stages, egm_stream_t s);

#ifdef __cplusplus
}
#endif
#endif /* EGM_HIP_H */
