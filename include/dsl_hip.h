/* dsl_hip.h — C ABI of libdsl_hip.so: the MI355X (gfx950) kernels behind the FCOS R50-FPN
 * teacher–student training step of chenbinghui1/DSL.
 *
 * Nothing like this exists in the reference (it is pure Python over torch/cuDNN/mmcv ops); each
 * entry point below names the reference call it replaces (paths relative to /root/reference).
 *
 * Conventions:
 *   - every function returns 0 on success, <0 on error; dsl_last_error() gives a thread-local text
 *   - the caller owns every buffer; the library never allocates device memory (workspace and table
 *     sizes are queried: dsl_*_workspace_bytes, dsl_wgrad_pixtab_bytes).  What the library DOES own, per
 *     device and for the life of the process: the HIP streams it schedules its op lists on (12 candidates
 *     created at first use, dsl_streams_init), the named events of dsl_run_ops / dsl_stream_*_slot and the
 *     event pairs of dsl_prof_*; tests/test_abi_gpu.py holds hipMemGetInfo still over multi-scale steps
 *   - kernels are enqueued on the given hipStream_t (passed as void*), no implicit device sync
 *   - activations are NHWC bf16; tensors that span the 5 FPN levels are stored level-major:
 *     [level][image][y][x][channel] ("segments"), which is exactly the flattened location order
 *     of mmdet/models/dense_heads/fcos_head.py:239-258
 *   - weights: fp32 master in KRSC = [Cout][kh][kw][Cin]; bf16 packed copies in the same order
 *     ("fwd pack", rows padded to 64) and in CRSK = [Cin][kh][kw][CoutPad] ("dgrad pack")
 */
#ifndef DSL_HIP_H
#define DSL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSL_MAX_SEG 5
#define DSL_MAX_GROUP 8   /* convolutions per grouped weight-gradient launch */

int dsl_version(void);
const char* dsl_last_error(void);
/* Library options - the library reads no environment variable.  Names: "wgrad_slots" (default 128: workgroup budget of a
 * weight-gradient launch whose descriptor leaves `slots` 0), "stream_probe" (1; 0 = the library takes its streams as the runtime deals
 * them instead of probing for hardware queues of their own, dsl_streams_init), "debug_sync" (0; 1 = dsl_run_ops drains the device after every op and
 * names it on stderr), "skip_kinds" (0; timing-only ablation: bit mask of op kinds dsl_run_ops skips), "comm_queue" (1; which of the four
 * hardware queues the communication stream is placed on, see dsl_comm_stream_queue; set it before the streams exist).  Unknown name: -1. */
int dsl_set_option(const char* name, int value);
int dsl_get_option(const char* name, int* value);

/* ------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on MFMA (forward, data-gradient) — replaces F.conv2d / cuDNN in
 * mmdet/models/backbones/resnet.py:262-301,598-645, necks/fpn.py:150-202,
 * dense_heads/anchor_free_head.py:197-217, fcos_head.py:154-156 and their autograd backward.
 * One "compute grid" pixel (seg, n, y, x) gathers, per tap (r, s), a contiguous channel vector of
 * the source:   mode 0 (forward):   (sy, sx) = (y*stride + r - pad, x*stride + s - pad)
 *               mode 1 (transposed): (sy, sx) = ((y + pad - r)/stride, (x + pad - s)/stride) if divisible
 * and writes to destination pixel (y*os, x*os).
 * Epilogue: v = acc*scale[c] + bias[c]; [mask_first: v *= (mask>0)]; v += addend (same index, or
 * nearest-upsampled from (ah, aw) when DSL_CONV_ADD_UPSAMPLE); [mask_last: v *= (mask>0)];
 * [relu]; store bf16 or fp32.
 * ---------------------------------------------------------------------------------------- */
enum {
  DSL_CONV_RELU_OUT = 1,      /* ReLU in the epilogue */
  DSL_CONV_RELU_IN = 2,       /* ReLU applied to the gathered source (FPN P7 = conv(relu(P6))) */
  DSL_CONV_OUT_F32 = 4,       /* destination is fp32 (head logits) instead of bf16 */
  DSL_CONV_MASK_FIRST = 8,    /* v = acc*(mask>0) + addend */
  DSL_CONV_MASK_LAST = 16,    /* v = (acc + addend)*(mask>0) */
  DSL_CONV_ADD_UPSAMPLE = 32, /* addend is nearest-upsampled (fpn.py:163-172) */
  DSL_CONV_SMALL_C = 64,      /* source has 8 channels (stem, image packed NHWC8) */
  DSL_CONV_FP8 = 128,         /* src and wgt are OCP fp8 e4m3 (dsl_quant_fp8 / dsl_quant_fp8_weights; forward mode, cs % 128 == 0,
                               * cs / lds count bytes): MX-scaled fp8 MFMA, `scale` carries 1 / (weight scale x activation scale) */
  /* bits 8-11: tile configuration, bits 12-15: split-K factor (test hooks; 0 = the library's own choice) */
  DSL_CONV_EPI_STAGED = 1 << 16   /* test hook: the general staged fp32 epilogue even where an in-register one applies (same bits) */
};

typedef struct dsl_conv_desc {
  int32_t nseg, n;                                   /* level segments, images */
  int32_t gh[DSL_MAX_SEG], gw[DSL_MAX_SEG];          /* compute grid per segment */
  int32_t sh[DSL_MAX_SEG], sw[DSL_MAX_SEG];          /* source spatial size */
  int32_t dh[DSL_MAX_SEG], dw[DSL_MAX_SEG];          /* destination spatial size */
  int32_t ah[DSL_MAX_SEG], aw[DSL_MAX_SEG];          /* addend spatial size (ADD_UPSAMPLE) */
  int32_t cs;                                        /* source channels (GEMM-K per tap) */
  int32_t cd;                                        /* real destination channels */
  int32_t cd_pad;                                    /* weight rows (multiple of 64) */
  int32_t ldd, lda, ldm;                             /* row strides (elements) of dst/addend/mask */
  int32_t kh, kw, stride, pad, mode, os, flags;
  const void* src;                                   /* bf16 */
  const void* wgt;                                   /* bf16 [cd_pad][kh*kw*cs] (SMALL_C: rows of round_up(kh*kw*8, 64); FP8: e4m3).
                                                      * Mode 1 reads the dgrad pack with the same tap order: no flip */
  void* dst;                                         /* bf16 or fp32 */
  const float* scale;                                /* [cd] or NULL (=1) */
  const float* bias;                                 /* [cd] or NULL (=0) */
  const void* addend;                                /* bf16 or NULL; may equal dst (in-place accumulation: each element is read
                                                      * before it is written) */
  const void* mask;                                  /* bf16 or NULL */
  void* workspace;                                   /* optional fp32 scratch for split-K (small-M, large-K convs) */
  size_t workspace_bytes;                            /* NULL/0: never split */
  int32_t cs_real;                                   /* 0 = cs; else the source's real channel count when cs is padded (the
                                                      * C- / 5-channel predictor gradients stored round_up(C, 64) / 64 wide,
                                                      * 1 <= C <= 128): only the
                                                      * algorithmic FLOP / byte counts of dsl_prof_* use it */
  int32_t lds;                                       /* 0 = cs; else the source's pixel stride in elements (>= cs, multiple of
                                                      * 8): the source is a channel slice [0, cs) of wider rows */
  void* gn_ws;                                       /* NULL, or the `workspace` of the dsl_gn_desc that normalises this output
                                                      * (8 channels per group, conv_stats = 1): the epilogue leaves the per-tile
                                                      * statistics records there and dsl_groupnorm_relu_fwd skips its own
                                                      * statistics pass (ConvModule conv -> GN -> ReLU, anchor_free_head.py:104-133);
                                                      * legal only where dsl_conv2d_gn_fusable() says 1 */
  const void* gn_x;                                  /* NULL: gn_ws takes the forward records (sum, sum of squares).  Else this launch is
                                                      * the data gradient that produces dY of that GroupNorm + ReLU, gn_x its bf16 input
                                                      * of the forward pass (same rows as dst, ldd == cd): gn_ws takes the BACKWARD
                                                      * records and dsl_groupnorm_relu_bwd (conv_stats = 1) skips its reduction pass */
  const float* gn_gamma;                             /* with gn_x: the norm's weight, bias and the forward statistics (dsl_gn_desc.stats) */
  const float* gn_beta;
  const float* gn_stats;
} dsl_conv_desc;

/* 1 if a launch of `d` can write GroupNorm records (pipelined kernel, bf16 output on its own pixel grid, no split-K) */
int dsl_conv2d_gn_fusable(const dsl_conv_desc* d);

/* bytes of split-K scratch this conv would like (0 if it will not split); any smaller buffer is legal */
size_t dsl_conv2d_workspace_bytes(const dsl_conv_desc* d);
int dsl_conv2d(const dsl_conv_desc* d, void* stream);

/* What dsl_conv2d(d) would launch, from the function the launch itself takes its numbers from.  Host only: no HIP call, works
 * without a device (tools, tests/test_conv_plan_cpu.py).  Returns what dsl_conv2d would return for a descriptor it refuses. */
typedef struct dsl_conv_plan {
  int32_t kernel;        /* 0 v1 gemm, 1 glds, 2 pipe, 3 pipe + backward GN records, 4 pipe SMALL_C, 5 fp8 */
  int32_t cfg;           /* tile table row, -1 for the v1 kernel */
  int32_t bco, bpx, threads, splits;
  int32_t grid[3];       /* as passed to the launch */
  int32_t ident, addfast;
  size_t lds_bytes, workspace_bytes;
} dsl_conv_plan;
int dsl_conv2d_plan(const dsl_conv_desc* d, dsl_conv_plan* out);

/* Weight gradient: dW[co][r][s][ci] = scale[co] * sum_p dY[p][co] * X[p@(r,s)][ci]  (fp32, KRSC).
 * Split-K over pixels into a caller-owned workspace, then a reduce pass.  Optionally also
 * db[co] = sum_p dY[p][co].  Replaces the autograd backward of the same F.conv2d calls. */
typedef struct dsl_wgrad_desc {
  int32_t nseg, n;
  int32_t gh[DSL_MAX_SEG], gw[DSL_MAX_SEG];          /* dY spatial size (conv output grid) */
  int32_t sh[DSL_MAX_SEG], sw[DSL_MAX_SEG];          /* X spatial size (conv input) */
  int32_t cs;                                        /* X channels (Cin) */
  int32_t cy;                                        /* dY channels = row stride (multiple of 64) */
  int32_t cd;                                        /* real Cout (rows of dW written) */
  int32_t kh, kw, stride, pad;
  int32_t splits;                                    /* from dsl_wgrad_splits() */
  const void* dy;                                    /* bf16 */
  const void* x;                                     /* bf16 */
  const float* scale;                                /* [cd] or NULL */
  float* dw;                                         /* fp32 [cd][kh*kw*cs] */
  float* db;                                         /* fp32 [cd] or NULL */
  void* workspace;
  size_t workspace_bytes;
  int32_t ldx;                                       /* 0 = cs; else X's pixel stride in elements (X is a channel slice of wider rows) */
  int32_t shared;                                    /* group launches: 1 = the members are applications of ONE convolution (same dw):
                                                      * their gradients are summed into dw (RLA's recurrent / conv_out layers) */
  int32_t slots;                                     /* 0 = default (option "wgrad_slots", 128); else the workgroup budget the split factor
                                                      * is chosen for: launches that run beside the caller's stream leave it CUs, the
                                                      * ones at the very end of a pass can take the chip (group launches: descs[0]'s) */
  int32_t pad_;
  const void* pixtab;                                /* the geometry's pixel descriptor table: caller-owned device memory of
                                                      * >= dsl_wgrad_pixtab_bytes(d), written ONCE per geometry by dsl_wgrad_pixtab_fill
                                                      * (any descriptor of the same nseg / n / grid / source sizes / kh / kw / stride /
                                                      * pad may share it).  May be NULL when dsl_wgrad_pixtab_bytes(d) is 0 */
  size_t pixtab_bytes;
} dsl_wgrad_desc;

int dsl_wgrad_splits(const dsl_wgrad_desc* d);
size_t dsl_wgrad_workspace_bytes(const dsl_wgrad_desc* d);
/* The pipelined weight-gradient kernels read their gather addresses (source pixel of tap (0, 0), tap validity bits) from a table of
 * 8 bytes per output pixel.  It is the CALLER's memory like every other buffer: query the size (0 = this geometry's kernel needs
 * none), fill it with one small kernel on `stream`, hand it over in dsl_wgrad_desc.pixtab.  The library keeps no device allocation
 * of its own (until round 6 it cached these tables in hipMalloc'd memory for the life of the process). */
size_t dsl_wgrad_pixtab_bytes(const dsl_wgrad_desc* d);
int dsl_wgrad_pixtab_fill(const dsl_wgrad_desc* d, void* table, size_t bytes, void* stream);
int dsl_conv2d_wgrad(const dsl_wgrad_desc* d, void* stream);
/* The weight gradients of `count` (<= DSL_MAX_GROUP) convolutions that share one geometry - every descriptor
 * field except dy, x, scale, dw, db - as ONE launch: the workgroups that fill the chip come from `count` times
 * more output tiles, so `count` times fewer pixel splits and fp32 partial tiles are needed (ResNet blocks of
 * one stage, the FCOS tower layers).  Uses descs[0].workspace (>= dsl_wgrad_group_workspace_bytes); the
 * members' `splits` fields are ignored. */
size_t dsl_wgrad_group_workspace_bytes(const dsl_wgrad_desc* descs, int count);
int dsl_conv2d_wgrad_group(const dsl_wgrad_desc* descs, int count, void* stream);

/* Multi launch: the weight gradients of up to DSL_MAX_MULTI sub-launches (sub-launch s = counts[s] consecutive descriptors
 * of one geometry, as in dsl_conv2d_wgrad_group) that share one tile configuration (dsl_wgrad_multi_config: 1..4; 0 = has
 * no multi form) as ONE grid and ONE reduce grid: the backward pass of a whole FPN or ResNet stage instead of one launch
 * pair per layer.  Split factors are chosen for the launch as a whole (every workgroup gets about 1/wgrad_slots of its
 * K iterations), sub-launches that end up with one split write dW directly and have no partial tiles or reduce pass.
 * The launch plan is a table the caller owns: dsl_wgrad_multi_build fills `table_host` (dsl_wgrad_multi_table_bytes()
 * bytes of host memory), the caller copies those bytes to device memory once and passes both to
 * dsl_conv2d_wgrad_multi.  The table holds the descriptors' pointers and `workspace`
 * (>= dsl_wgrad_multi_workspace_bytes): rebuild it when they change.  Results are bit-identical to the same sub-launches
 * run through dsl_conv2d_wgrad_group with the same split factors; with different split factors they differ by fp32
 * summation order only. */
#define DSL_MAX_MULTI 16
int dsl_wgrad_multi_config(const dsl_wgrad_desc* d);
size_t dsl_wgrad_multi_table_bytes(void);
size_t dsl_wgrad_multi_workspace_bytes(const dsl_wgrad_desc* descs, const int* counts, int nsub);
int dsl_wgrad_multi_build(const dsl_wgrad_desc* descs, const int* counts, int nsub, void* workspace, size_t workspace_bytes,
                          void* table_host, size_t table_bytes);
int dsl_conv2d_wgrad_multi(const void* table_host, const void* table_dev, void* stream);
int dsl_wgrad_multi_info(const void* table_host, double* flops, double* bytes, int* blocks, int* red_blocks, int* nsub);
/* The launch planner behind dsl_wgrad_multi_build, callable without a device (tests, tools): sub-launch s has stages[s] K stages
 * (32 pixels each), tiles[s] output tiles over all its members and tile_elems[s] fp32 elements per split (may be NULL);
 * cfg = tile configuration 1..3, cap = workgroups of the persistent grid (a multiple of 8).  The planner picks the split
 * factors by simulating the grid: items go longest first to the least loaded workgroup of their XCD class, cost = the longest
 * workgroup's stages (+ a fixed cost per item) + the reduce pass the partial tiles need.  splits_out[nsub]; info[5] =
 * {grid, makespan in stages, work items, makespan of round 3's rule (one target length, stride walk), its work items}. */
int dsl_wgrad_plan_probe(const int* stages, const int* tiles, const long long* tile_elems, int nsub, int cfg, int cap,
                         int* splits_out, int* info);

/* fp8 forward path (BASELINE.json configs[4], first slice; the reference trains in fp32 and has no such path).
 * dsl_quant_fp8: y[r][c] = e4m3(clamp(x[r][c] * scale, +-448)) for a bf16 [rows][ld_x] tensor -> fp8 [rows][c] (c % 16 == 0).
 * dsl_quant_fp8_weights: per output channel co < cout: s = 448 / max|w[co][:]| (1 if the row is zero), w8[co][k] = e4m3(w * s),
 * comb[co] = inv_act_scale / s  - the `scale` vector of the fp8 convolution's epilogue (x BatchNorm scale if bn_scale != NULL);
 * rows cout .. cout_pad are zero-filled with comb 0. */
int dsl_quant_fp8(const void* x_bf16, void* y_fp8, long rows, int c, int ld_x, float scale, void* stream);
/* Dynamic per-tensor activation scale (what the engine uses): dsl_absmax writes n_partials block maxima of |x|; dsl_quant_fp8_dyn
 * quantises with scale = 448 / max(partials) (the tensor's own maximum: nothing saturates); dsl_fp8_comb makes the convolution's
 * epilogue scale comb[i] = winv[i] * max(partials) / 448 from the weights' inverse scales (dsl_quant_fp8_weights with
 * inv_act_scale = 1).  No atomics, nothing to clear between steps. */
int dsl_absmax(const void* x_bf16, long rows, int c, int ld_x, float* partials, int n_partials, void* stream);
int dsl_quant_fp8_dyn(const void* x_bf16, void* y_fp8, long rows, int c, int ld_x, const float* partials, int n_partials, void* stream);
int dsl_fp8_comb(const float* winv, float* comb, int n, const float* partials, int n_partials, void* stream);
int dsl_quant_fp8_weights(const float* w, void* w8, float* comb, const float* bn_scale, int cout, int cout_pad, int k,
                          float inv_act_scale, void* stream);
/* Delayed scaling (round 6; what the engine uses for the towers' fp8 forward): an activation is quantised by its PRODUCER's pass with
 * the scale of the previous step's maximum, and leaves this step's block maxima for the next one - no pass of its own.
 * dsl_fp8_prep, one launch per step for n_items convolutions that share cout_pad and k: per item and output channel co < cout the
 *   weight row is quantised as dsl_quant_fp8_weights does (s_w = 448 / max|w[co][:]|); a = margin * max(amax[0 .. n_amax)) is the
 *   input tensor's expected maximum; scale[0] = 448 / a (1 when a == 0: nothing recorded yet - run the forward pass once to record)
 *   is what the input's producer multiplies by, comb[co] = a / 448 / s_w[co] the convolution's epilogue scale; rows co >= cout are 0.
 * dsl_quant_fp8_delayed: y = e4m3(clamp(x * scale[0], +-448)) for a tensor nobody's epilogue can quantise (the FPN outputs),
 *   partials[b] = block b's max|x| (n_partials blocks, every one written). */
typedef struct dsl_fp8_prep_item {
  const float* w;       /* fp32 [cout][k] */
  void* w8;             /* e4m3 [cout_pad][k] */
  float* comb;          /* [cout_pad] */
  const float* amax;    /* block maxima of the convolution's input, left by the previous step */
  float* scale;         /* [1] */
  int32_t n_amax, cout;
} dsl_fp8_prep_item;
int dsl_fp8_prep(const dsl_fp8_prep_item* items_dev, int n_items, int cout_pad, int k, float margin, void* stream);
int dsl_quant_fp8_delayed(const void* x_bf16, void* y_fp8, long rows, int c, int ld_x, const float* scale_dev, float* partials,
                          int n_partials, void* stream);

/* A whole trained bottleneck's forward pass as ONE launch (csrc/bneck.hip; mmdet/models/backbones/resnet.py:262-301 Bottleneck.forward,
 * caffe style: stride on conv1; eval-mode BatchNorms folded to (scale, bias)):
 *   a1 = relu(bn1(conv1_1x1/stride(x))), a2 = relu(bn2(conv2_3x3(a1))), out = relu(bn3(conv3_1x1(a2)) + identity)
 * x [n][hin][win] rows of ldx elements (cin read), a1 / a2 [n][h][w][planes] (written: the weight gradients read them), identity and out
 * [n][h][w] rows of ldi / ldo elements (4 planes channels); weights bf16 in the forward layout of dsl_conv2d: w1 [planes][cin],
 * w2 [planes][3][3][planes], w3 [4 planes][planes].  planes = 128 or 256 (ResNet-50's layer2 / layer3), stride 1 or 2.  Bit-identical to
 * the three dsl_conv2d launches it replaces (same K order, same rounding points). */
typedef struct dsl_bneck_desc {
  const void* x; const void* w1; const void* w2; const void* w3; const void* idt;
  const float* s1; const float* b1; const float* s2; const float* b2; const float* s3; const float* b3;
  void* a1; void* a2; void* out;
  int32_t n, hin, win, h, w;
  int32_t planes, cin, ldx, stride, ldi, ldo;
} dsl_bneck_desc;
int dsl_bottleneck_fwd_supported(const dsl_bneck_desc* d);      /* 1 if dsl_bottleneck_fwd takes this shape */
int dsl_bottleneck_fwd(const dsl_bneck_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * GPU data path
 * ---------------------------------------------------------------------------------------- */
/* One image of a batch: decoded uint8 HWC (BGR, as mmcv.imread yields) on the device and the parameters the reference's CPU
 * pipeline draws per sample - Resize(keep_ratio) target size, PatchShuffle mode / split, RandomFlip, Normalize
 * (mmdet/datasets/pipelines/transforms.py:218-247, 2143-2248, 334-470, 652-690). */
typedef struct dsl_image_prep_item {
  const unsigned char* src;      /* [src_h][src_w][3] */
  int32_t src_h, src_w;
  int32_t new_h, new_w;          /* size after Resize (= src size: no resampling) */
  int32_t flip;                  /* bit 0: horizontal, bit 1: vertical (3: diagonal); 1 is RandomFlip's */
  int32_t ps_mode, ps_crop;      /* PatchShuffle: 0 none, 1 'flip' (columns [crop, w) first), 2 'flop' (rows [crop, h) first) */
  int32_t to_rgb;
  float mean[3], inv_std[3];     /* in output channel order */
} dsl_image_prep_item;
/* dst[n][3][hc][wc] fp32 <- resize (OpenCV's 8-bit fixed-point bilinear) -> PatchShuffle -> flip -> normalise, zero padded to the
 * canvas (Pad(size_divisor) and the loader's merge/pad, datasets/builder.py:236-267).  items_dev: device array of n items. */
int dsl_image_prep(const dsl_image_prep_item* items_dev, int n, float* dst, int hc, int wc, void* stream);
/* The same up to (not including) Normalize: the uint8 BGR images [n][hc][wc][3] (zero outside an image's new_h x new_w) that the
 * unlabeled stream's augmentations work on. */
int dsl_image_prep_u8(const dsl_image_prep_item* items_dev, int n, unsigned char* dst_u8, int hc, int wc, void* stream);

/* One augmentation pass over a batch of uint8 canvases (src -> dst, different buffers): per image `kind` selects the pass.
 * RandomAugmentBBox_Fast(aug_type='affine') (mmdet/datasets/pipelines/semi_aug.py:344-531: imgaug Affine, whole image or inside
 * one box) and UBAug (transforms.py:2098-2140: torchvision ColorJitter in its random order, RandomGrayscale, GaussianBlur,
 * three RandomErasing).  The host draws the parameters and transforms the boxes.  The colour, grayscale and blur passes are
 * Pillow's 8-bit arithmetic (ImageEnhance / Blend.c, Convert.c, BoxBlur.c) bit for bit - pinned against Pillow's own outputs
 * (tests/golden/ubaug_pil.npz); the stored channel order plays Pillow's (R, G, B), as the reference hands mmcv's BGR array to
 * ToPILImage unchanged.  imgaug is not available to this build: AFFINE follows its documented convention, parity UNPINNED.
 * ERASE writes its own N(0, 1) stream through torchvision's value mapping (mul(255).byte(): truncate, wrap). */
enum { DSL_AUG_COPY = 0, DSL_AUG_AFFINE = 1, DSL_AUG_BRIGHTNESS = 2, DSL_AUG_CONTRAST = 3, DSL_AUG_SATURATION = 4, DSL_AUG_HUE = 5,
       DSL_AUG_GRAY = 6, DSL_AUG_BLUR_H = 7, DSL_AUG_BLUR_V = 8, DSL_AUG_ERASE = 9,
       /* RandAug's ops on an image without boxes (mmdet/datasets/pipelines/autoaug_fast.py:219-224, 244-250, 371-372, 407, reached from
        * semi_aug.py:494-497): Pillow's ImageOps.autocontrast / equalize / solarize / posterize and ImageEnhance.Sharpness bit for
        * bit, pinned against Pillow's own outputs (tests/golden/randaug_pil.npz) */
       DSL_AUG_AUTOCONTRAST = 10, DSL_AUG_EQUALIZE = 11, DSL_AUG_SOLARIZE = 12, DSL_AUG_POSTERIZE = 13, DSL_AUG_SHARPNESS = 14 };
typedef struct dsl_aug_item {
  int32_t h, w;                  /* the image inside its canvas */
  int32_t kind;
  int32_t order;                 /* AFFINE: 0 nearest, 1 bilinear */
  float m[6];                    /* AFFINE: output pixel (x, y) relative to roi's corner -> source position x_s = m0 x + m1 y + m2,
                                  * y_s = m3 x + m4 y + m5 inside the roi (the inverse of the drawn transform) */
  int32_t roi[4];                /* AFFINE: x0, y0, x1, y1 - the region replaced and sampled (whole image, or one box) */
  int32_t cval;                  /* AFFINE: fill value (125) */
  float f[3];                    /* f[0]: BRIGHTNESS / CONTRAST / SATURATION / SHARPNESS the enhancement factor; HUE int(factor * 255), the
                                  * 8-bit shift; BLUR_H / BLUR_V the fractional box radius of GaussianBlur(sigma) (BoxBlur.c); SOLARIZE the
                                  * threshold (0 .. 256); POSTERIZE the bits kept (1 .. 8) */
  int32_t rect[3][4];            /* ERASE: up to three rectangles x0, y0, x1, y1 (x1 <= x0: unused) */
  uint32_t seed;                 /* ERASE: noise stream */
} dsl_aug_item;
/* scratch: dsl_image_aug_scratch_bytes(n) bytes, 8-byte aligned (per image: the luma sum, the three 256-bin band histograms and
 * the tables derived from them); need_stats: bit 0 set when some item is a CONTRAST pass, bit 1 when some item is an AUTOCONTRAST or
 * EQUALIZE pass (0: scratch may be NULL). */
size_t dsl_image_aug_scratch_bytes(int n);
int dsl_image_aug(const dsl_aug_item* items_dev, int n, const unsigned char* src, unsigned char* dst, int hc, int wc,
                  void* scratch, int need_stats, void* stream);
/* Normalize + Pad of a uint8 canvas batch (the tail of dsl_image_prep): dst[n][3][hc][wc] fp32. */
int dsl_image_normalize(const unsigned char* src_u8, const dsl_image_prep_item* items_dev, int n, float* dst, int hc, int wc,
                        void* stream);

/* Integer (non-resampling) geometric steps on uint8 BGR images, one launch per batch: the image work of the reference's RandomCrop,
 * MinIoURandomCrop, Expand, RandomShift and CutOut (mmdet/datasets/pipelines/transforms.py:693-873, 1113-1249, 1021-1109, 491-577,
 * 1850-1920).  The host draws the parameters and moves the boxes; an image's ordered step list maps (src_h, src_w) to (out_h, out_w):
 *   CROP    a = x0, y0, cw, ch          -> ch x cw: img[y0 : y0 + ch, x0 : x0 + cw]
 *   EXPAND  a = left, top, W, H; fill   -> H x W: fill everywhere, the input at (top, left)
 *   SHIFT   a = dx, dy                  -> unchanged: out[y, x] = in[y - dy, x - dx], zero where that falls outside (|dx| < w, |dy| < h)
 *   CUTOUT  a = x1, y1, x2, y2; fill    -> unchanged: the rectangle [y1, y2) x [x1, x2), already clipped to the image, set to fill
 * in_h / in_w: the size of the image the step receives (the kernel walks the list backwards from each output pixel and has no other
 * way to know it).  Every pixel of the dst_h x dst_w rectangle is written once: zero outside out_h x out_w. */
enum { DSL_GEO_CROP = 1, DSL_GEO_EXPAND = 2, DSL_GEO_SHIFT = 3, DSL_GEO_CUTOUT = 4 };
#define DSL_GEO_MAX_STEPS 32
typedef struct dsl_geo_step {
  int32_t kind;
  int32_t a[4];
  int32_t in_h, in_w;
  uint8_t fill[4];               /* EXPAND / CUTOUT: B, G, R (fill[3] unused) */
} dsl_geo_step;
typedef struct dsl_geo_item {
  const unsigned char* src;      /* [src_h] rows of src_ld pixels, src_w of them the image */
  int32_t src_h, src_w, src_ld;
  int32_t out_h, out_w;          /* size of the image after the last step (= src size for an empty list: a copy) */
  unsigned char* dst;            /* [dst_h] rows of dst_ld pixels; dst != src */
  int32_t dst_h, dst_w, dst_ld;  /* rectangle written, >= out_h x out_w */
  int32_t nsteps;                /* 0 .. DSL_GEO_MAX_STEPS; a longer list is split over launches by the caller */
  dsl_geo_step steps[DSL_GEO_MAX_STEPS];
} dsl_geo_item;
/* items: the n items in HOST memory - every list is checked here before anything runs (pointers, sizes, each step inside the image it
 * receives, the sizes chaining up to out_h x out_w, dst_h <= max_dst_h, dst_w <= max_dst_w); items_dev: the same n items on the
 * device, which the kernel reads.  The library allocates nothing and does not copy the table. */
int dsl_image_geo(const dsl_geo_item* items, const dsl_geo_item* items_dev, int n, int max_dst_h, int max_dst_w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Memory-bound fused layers
 * ---------------------------------------------------------------------------------------- */
/* NCHW fp32 image -> NHWC8 bf16 (channels 3..7 zero).  Replaces the implicit layout of
 * SingleStageDetector.extract_feat's input (detectors/single_stage.py:40-45). */
int dsl_pack_image(const float* img_nchw, void* out_nhwc8, int n, int h, int w, void* stream);

/* The frozen stem as one kernel: fp32 NCHW image -> conv1 7x7 / 2 (3 -> 64) + eval-mode BatchNorm (scale, bias) + ReLU + MaxPool
 * 3x3 / 2 -> NHWC bf16 [n][ph][pw] rows of ld_out elements (resnet.py:598-645 _make_stem_layer, :634-638).  w_groups: conv1's
 * weight as [22][64][8] bf16 - group g holds, for every cout, the values 8 (g % 3) .. + 8 of the 21 (kx, c) values of tap row
 * g / 3, zero beyond (ParamStore.stem_groups16).  Same arithmetic as dsl_pack_image + dsl_conv2d + dsl_maxpool3x3s2 up to the
 * fp32 summation order of the 147 products. */
int dsl_stem_pool(const float* img_nchw, const void* w_groups, const float* scale, const float* bias, void* out, int ld_out,
                  int n, int h, int w, void* stream);
/* The same with half_last = 1: img_nchw holds n - 1 images; image n - 1 is SemiEpochBasedRunner's scale-invariant copy of the
 * last one (semi_epoch_based_runner.py:186-204: F.interpolate(img[-1:], size = (h / 2, w / 2), mode = 'bilinear') pasted at the
 * top-left of a zero canvas), sampled from its source while the patch is loaded - no interpolate / zeros / cat passes, no
 * second copy of the batch; bit-identical to them (h, w even). */
int dsl_stem_pool_half(const float* img_nchw, const void* w_groups, const float* scale, const float* bias, void* out, int ld_out,
                       int n, int h, int w, int half_last, void* stream);

/* 3x3 stride-2 pad-1 max pool, NHWC bf16 (resnet.py:610,638). */
int dsl_maxpool3x3s2(const void* x, void* y, int n, int h, int w, int c, void* stream);
int dsl_maxpool3x3s2_ld(const void* x, void* y, int n, int h, int w, int c, int ldy, void* stream);   /* output row stride ldy >= c */

/* GroupNorm(32 groups, eps) + ReLU over level-major NHWC bf16 (mmcv ConvModule norm+act as used at
 * anchor_free_head.py:104-133).  stats = [nseg*n*groups][2] fp32 (mean, rstd), written by fwd.
 * Both directions are two passes with two-level, fixed-order reductions through `workspace` (block records,
 * no atomics, nothing to pre-zero): results are bit-identical from run to run. */
typedef struct dsl_gn_desc {
  int32_t nseg, n, c, groups;
  int32_t h[DSL_MAX_SEG], w[DSL_MAX_SEG];
  float eps;
  const void* x;          /* bf16 pre-norm conv output */
  void* y;                /* bf16 relu(gn(x)) */
  const float* gamma;
  const float* beta;
  float* stats;
  /* backward only */
  const void* dy;         /* bf16 grad wrt y */
  void* dx;               /* bf16 grad wrt x */
  float* dgamma;          /* fp32 [c], overwritten */
  float* dbeta;           /* fp32 [c], overwritten */
  float* dbias;           /* fp32 [c] or NULL: sum over pixels of dx = gradient of the bias of the conv that made x */
  void* workspace;        /* >= dsl_groupnorm_workspace_bytes(d); private to this call until it completes */
  size_t workspace_bytes;
  int32_t conv_stats;     /* 1 = a convolution already left this call's block records in `workspace` (dsl_conv_desc.gn_ws ==
                           * workspace): forward, the one that produced x; backward, the data gradient that produced dy (its
                           * gn_x = x).  One pass instead of two; needs c / groups == 8 */
  int32_t pad_;
  /* forward only, optional (all NULL: off) - the fp8 copy of y that an fp8 convolution reads next (DSL_CONV_FP8), written in the
   * same pass with a DELAYED scale: y8 = e4m3(clamp(bf16(y) * y8_scale[0], +-448)) [pixel][c]; y8_amax[(segment * n + image) * nblk +
   * block] = max of this call's bf16(y) over the block's pixels (nblk = ceil(max hw / 128); blocks outside a level never write:
   * clear the buffer once) - the maxima dsl_fp8_prep turns into the NEXT step's scale */
  void* y8;
  const float* y8_scale;
  float* y8_amax;
} dsl_gn_desc;
size_t dsl_groupnorm_workspace_bytes(const dsl_gn_desc* d);
int dsl_groupnorm_relu_fwd(const dsl_gn_desc* d, void* stream);
int dsl_groupnorm_relu_bwd(const dsl_gn_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * RLA_ResNet layers (mmdet/models/backbones/resnet_rla.py:71-137,289-327): explicit row strides (ld, elements) because the
 * block input cat(x, h) is ONE buffer [pixel][C + 128] = [x | h (32) | zeros]
 * ---------------------------------------------------------------------------------------- */
/* nn.AvgPool2d((2, 2), stride=(2, 2)) on h at a stage transition (:98-100,129-130) and its backward */
int dsl_avgpool2x2(const void* x, int ldx, void* y, int ldy, int n, int h, int w, int c, void* stream);
int dsl_avgpool2x2_bwd(const void* gy, int ldgy, void* gx, int ldgx, int n, int h, int w, int c, void* stream);
/* t = tanh(bn(u)), BN in eval mode folded to (scale, bias) (:318-320), and its backward: g_u, dgamma, dbeta (overwritten;
 * block records in `workspace`, fixed-order sums).  dgamma = dbeta = NULL: the records [ceil(rows / 256)][2 c] are left
 * in `workspace` and dsl_rec_sum_multi sums them - several row ranges of one tensor (image-split backward chains on
 * two streams) write their records side by side and are summed by one launch behind both. */
int dsl_bn_tanh_fwd(const void* u, int ldu, const float* scale, const float* bias, void* t, int ldt, long rows, int c,
                    void* stream);
size_t dsl_bn_tanh_bwd_workspace_bytes(long rows, int c);
int dsl_bn_tanh_bwd(const void* gt, int ldgt, const void* t, int ldt, const void* u, int ldu, const float* scale,
                    const float* mean, const float* var, float eps, void* gu, int ldgu, float* dgamma, float* dbeta,
                    void* workspace, long rows, int c, void* stream);
typedef struct dsl_rec_sum_item {
  const float* rec; float* out_a; float* out_b;      /* out_a[ch] = sum_r rec[r][ch], out_b[ch] = sum_r rec[r][c + ch] */
  int32_t nrec, pad_;
} dsl_rec_sum_item;
int dsl_rec_sum_multi(const dsl_rec_sum_item* items_dev, int n, int c, void* stream);      /* items: DEVICE array, one workgroup each */
/* eval-mode BatchNorm with TRAINABLE affine parameters (norm_eval freezes the statistics only, :380-388): per-step fold
 * scale = gamma / sqrt(var + eps), bias = beta - mean * scale over n channels */
int dsl_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* scale,
                float* bias, int n, void* stream);
/* (gamma, beta) gradients of conv -> BN(eval) pairs from the UNSCALED weight gradient dWu (dsl_conv2d_wgrad with scale =
 * NULL, db = dbeta): dgamma[c] = (<W[c], dWu[c]> - mean[c] dbeta[c]) / sqrt(var[c] + eps), then dWu[c] *= gamma[c] /
 * sqrt(var[c] + eps) in place.  `items` is a DEVICE array; one workgroup per weight row (row_start = prefix sum of rows). */
typedef struct dsl_bn_post_item {
  const float* w; float* dw; float* dgamma; const float* dbeta; const float* gamma; const float* mean; const float* var;
  int32_t rows, k, row_start, pad_;
} dsl_bn_post_item;
int dsl_bn_wgrad_post(const dsl_bn_post_item* items_dev, int n, int total_rows, float eps, void* stream);
/* The recurrent path of one RLA block as ONE launch (resnet_rla.py:125-136): u = h_in + conv_out(x) (1x1, c4 -> 32; w_conv_out rows of c4
 * elements, 32 used), t = tanh(u * bn_scale + bn_bias), h_out = recurrent_conv(t) (3x3, pad 1; w_recurrent [>= 32][3][3][tw], the first
 * 32 of every tw input columns used).  x [n*h*w][ldx], h_in [..][ldh], u [..][32], t [..][tw] (first 32 written), h_out [..][ldo] (32 written);
 * bf16.  Same rounding points as dsl_conv2d (addend h_in) -> dsl_bn_tanh_fwd -> dsl_conv2d, which it replaces. */
int dsl_rla_tail_fwd(const void* x, int ldx, const void* h_in, int ldh, const void* w_conv_out, int c4, const float* bn_scale,
                     const float* bn_bias, const void* w_recurrent, int tw, void* u, void* t, void* h_out, int ldo, int n, int h, int w,
                     void* stream);
/* ... and its backward tail as ONE launch: g_t = recurrent_conv^T(g_h) (the 3x3 data gradient; wT_recurrent = the data-gradient pack
 * [>= 32 ci][3][3][ldw co], 32 co used; g_h [n*h*w][ldgh], 32 used) followed by dsl_bn_tanh_bwd's arithmetic on it (t [..][ldt], u [..][32],
 * g_u [..][ldgu], 32 written; dgamma / dbeta fp32 [32] overwritten, or NULL: the tile records [tiles][64] stay in `workspace` for
 * dsl_rec_sum_multi).  workspace >= dsl_rla_tail_bwd_workspace_bytes(n, h, w).  g_t is never stored.  Replaces dsl_conv2d (mode 1) ->
 * dsl_bn_tanh_bwd; g_u equals theirs bit for bit, dgamma / dbeta differ by the summation order of their records only. */
size_t dsl_rla_tail_bwd_workspace_bytes(int n, int h, int w);
int dsl_rla_tail_bwd(const void* g_h, int ldgh, const void* wT_recurrent, int ldw, const void* t, int ldt, const void* u,
                     const float* scale, const float* mean, const float* var, float eps, void* g_u, int ldgu, float* dgamma, float* dbeta,
                     void* workspace, int n, int h, int w, void* stream);
/* one of the above as an op-list entry (DSL_OP_RLA): kind selects the call, the arguments are taken in declaration order
 * from p[] (pointers), i[] (ints: strides / sizes), f[] (eps), rows */
enum { DSL_RLA_AVGPOOL = 2, DSL_RLA_AVGPOOL_BWD = 3, DSL_RLA_BN_TANH = 4, DSL_RLA_BN_TANH_BWD = 5,
       DSL_RLA_BN_FOLD = 6, DSL_RLA_BN_POST = 7, DSL_RLA_REC_SUM = 8 /* p[0] = items, i[0] = n, i[1] = c */,
       DSL_RLA_TAIL_FWD = 9 /* p[] = x, h_in, w_conv_out, bn_scale, bn_bias, w_recurrent, u, t, h_out; i[] = ldx, ldh, c4, tw, ldo, n, h, w */,
       DSL_RLA_TAIL_BWD = 10 /* p[] = g_h, wT_recurrent, t, u, scale, mean, var, g_u, dgamma, dbeta, workspace; i[] = ldgh, ldw, ldt, ldgu, n, h, w;
                              * f[0] = eps */ };
typedef struct dsl_rla_desc {
  int32_t kind;
  int32_t i[8];
  float f[2];
  int64_t rows;
  void* p[12];
} dsl_rla_desc;
int dsl_rla_op(const dsl_rla_desc* d, void* stream);

/* out[n][y][x][c] = sum over the children of (y,x) in g (backward of the FPN nearest upsample,
 * fpn.py:163-172).  out is (h, w), g is (ch, cw) (normally 2h x 2w); bf16. */
int dsl_sum2x2(const void* g, void* out, int n, int h, int w, int ch, int cw, int c, void* stream);

/* per-channel column sum of a bf16 [rows][ld] matrix -> fp32 [c]  (conv bias gradient) */
int dsl_colsum(const void* x, float* out, long rows, int c, int ld, void* stream);

/* ------------------------------------------------------------------------------------------
 * FCOS targets and losses (fcos_head.py:170-338,550-726; losses/focal_loss.py:11-56;
 * losses/iou_loss.py:14-36,85-219; losses/cross_entropy_loss.py:73-112)
 * ---------------------------------------------------------------------------------------- */
struct dsl_atss_desc;
typedef struct dsl_fcos_desc {
  int32_t nlvl, n;                     /* levels, images */
  int32_t h[DSL_MAX_SEG], w[DSL_MAX_SEG], stride[DSL_MAX_SEG];
  float range_lo[DSL_MAX_SEG], range_hi[DSL_MAX_SEG];
  float radius;                        /* center_sample_radius (1.5) */
  int32_t num_classes;                 /* C >= 1 (the host uses 1..128); ld_cls % 4 == 0, ld_cls >= C, ld_gcls >= ld_cls */
  /* ground truth, concatenated over images; gt_off[n+1] prefix offsets (device int32) */
  const float* gt_boxes;               /* [G][4] xyxy */
  const int64_t* gt_labels;            /* [G] */
  const int32_t* gt_off;               /* [n+1] */
  const float* ig_boxes;               /* ignore boxes or NULL */
  const int32_t* ig_off;               /* [n+1] or NULL */
  /* outputs of assign, level-major [lvl][img][y][x] */
  int64_t* labels;                     /* [M] in [0, num_classes] */
  float* bbox_targets;                 /* [M][4], already / stride (norm_on_bbox) */
  int32_t* assign_idx;                 /* [M] argmin gt index within the image, -1 = background */
  float* cls_weight;                   /* [M] ignore weight * stream weight */
  float* pos_weight;                   /* [M] stream weight (bbox / centerness) */
  float* stats;                        /* [8]: 0 num_pos, 1 sum ctr targets (this rank) ... */
  float loss_weight;                   /* unlabeled-stream weight (DSL) ; 1.0 = off */
  /* head outputs */
  const float* cls_logits;             /* [M][ld_cls] fp32 */
  const float* regctr;                 /* [M][ld_rc] fp32: raw conv_reg (4) + centerness logit (1) */
  int32_t ld_cls, ld_rc;
  const float* scales;                 /* [nlvl] Scale parameters */
  /* [0] = sum over ranks of num_pos, [1] = sum over ranks of sum(ctr targets); the kernel applies
   * max(x*inv_world, 1) and max(x*inv_world, 1e-6)  (reduce_mean, fcos_head.py:264-274) */
  const float* norm;
  /* gradients (bf16, padded rows) and loss sums */
  void* g_cls;  int32_t ld_gcls;       /* bf16 [M][ld_gcls] */
  void* g_rc;   int32_t ld_grc;        /* bf16 [M][ld_grc] */
  float* g_scales;                     /* fp32 [DSL_MAX_SEG], overwritten */
  float* losses;                       /* fp32 [4]: cls, bbox, centerness, sisoft (overwritten) */
  float soft_weight;                   /* effective sisoft weight (0 = off) */
  float grad_scale;                    /* d(total)/d(each loss), normally 1 */
  float inv_world;                     /* 1/world_size: norm[] holds the SUM over ranks of stats[0:2] */
  void* workspace;                     /* >= dsl_fcos_workspace_bytes(d): block records of the loss / num_pos sums, which */
  size_t workspace_bytes;              /* are added up in a fixed order (bit-identical results from run to run) */
  float* logvec;                       /* NULL, or fp32 [5]: cls, bbox, centerness, [sisoft if soft_weight != 0,] their sum - the log
                                        * vector of BaseDetector._parse_losses (detectors/base.py:175-208) without a framework op */
  /* Head options; all zero = the fcos_semi "tricks" head (center_sampling, norm_on_bbox, centerness_on_reg, GIoULoss) */
  int32_t head_flags;                  /* DSL_HEAD_* below */
  int32_t ld_ctr;                      /* row stride of ctr (floats) */
  const float* ctr;                    /* NULL: the centerness logit is regctr[m][4].  Else ctr[m * ld_ctr] - centerness_on_reg=False
                                        * (fcos_head.py:155-158): conv_centerness reads the classification tower, its logit is a column
                                        * of the classification predictor's output; regctr then needs 4 columns only */
  void* g_ctr;                         /* bf16, with ctr: the centerness gradient goes to g_ctr[m * ld_gctr], column 4 of g_rc gets 0 */
  int32_t ld_gctr;                     /* row stride of g_ctr (bf16 elements); read only when g_ctr is set */
  /* Loss family, read only with DSL_HEAD_LOSS_EXT in head_flags (then every field counts as written: a weight of 0 is 0).  Without
   * the bit - a zero-filled tail included - the terms are the default head's: GIoU or, with DSL_HEAD_IOU_LOSS, the IoU log loss;
   * focal gamma 2, alpha 0.25; weights 1.  With the bit and exactly those values the same kernel runs (bit-identical outputs). */
  int32_t box_kind;                    /* DSL_BOX_* below: loss_bbox (it replaces DSL_HEAD_IOU_LOSS) */
  float box_eps;                       /* eps of DIoULoss / CIoULoss (losses/iou_loss.py:107,162; the classes' default 1e-6); the other
                                        * kinds use 1e-6 */
  float focal_gamma, focal_alpha;      /* FocalLoss gamma >= 0, 0 <= alpha <= 1 (losses/focal_loss.py:11-56) */
  float w_cls, w_bbox, w_ctr;          /* loss_weight of loss_cls / loss_bbox / loss_centerness: scale losses[0..2], logvec and the
                                        * term's gradients (g_cls; g_rc[:, :4] and g_scales; the centerness gradient).  The sisoft term
                                        * and the stream weight `loss_weight` above are independent of them */
  const struct dsl_atss_desc* atss;    /* read only with DSL_HEAD_ATSS: anchor_scale and delta_stds of the ATSS head (below) */
} dsl_fcos_desc;
#define DSL_HEAD_INSIDE_BOX 1   /* center_sampling=False: inside = min(l, t, r, b) > 0, radius unused (fcos_head.py:676-678) */
#define DSL_HEAD_RAW_TARGETS 2  /* norm_on_bbox=False, assignment: bbox_targets stay in pixels (fcos_head.py:618) */
#define DSL_HEAD_EXP_DECODE 4   /* norm_on_bbox=False, loss and detection: distances = exp(scale * x), no stride multiply
                                 * (fcos_head.py:162-167); the gradient goes through exp into g_rc and g_scales */
#define DSL_HEAD_IOU_LOSS 8     /* loss_bbox = IoULoss(linear=False, eps=1e-6): -log(clamp(iou, eps)) (losses/iou_loss.py:14-36) */
#define DSL_HEAD_LOSS_EXT 16    /* dsl_fcos_desc: box_kind .. w_ctr are set (loss family); not a dsl_det_desc flag */
#define DSL_HEAD_ATSS 32        /* ATSSHead (below): anchor-delta decode, the stored ground-truth box as target, ATSS normalisers */
/* dsl_fcos_desc.box_kind.  Linear IoU: 1 - clamp(iou, 1e-6), no gradient where the clamp is active (losses/iou_loss.py:31-33).
 * DIoU / CIoU restate losses/iou_loss.py:105-219 (union = a1 + a2 - overlap + eps, c2 = cw^2 + ch^2 + eps, CIoU's h = y2 - y1 + eps)
 * with two deviations from the reference's fp32 results: CIoU's penalty v^2 / (1 - iou + v) and its gradient are 0 where v == 0
 * (the reference: 0/0 = NaN when prediction and target coincide; 0 is the fp64 value), and the focal gradient for gamma < 1 is the
 * finite limit where the sigmoid saturates to exactly 0 or 1 (the reference: NaN). */
#define DSL_BOX_GIOU 0
#define DSL_BOX_IOU_LOG 1
#define DSL_BOX_IOU_LINEAR 2
#define DSL_BOX_DIOU 3
#define DSL_BOX_CIOU 4
size_t dsl_fcos_workspace_bytes(const dsl_fcos_desc* d);   /* with DSL_HEAD_ATSS: also what dsl_atss_assign needs; with DSL_HEAD_PAA: what
                                                            * the dsl_paa_* passes need (reads d->atss->max_gt) */

/* ------------------------------------------------------------------------------------------
 * ATSS: adaptive training sample selection (mmdet/core/bbox/assigners/atss_assigner.py:66-178,
 * mmdet/models/dense_heads/atss_head.py:142-309,420-495,569-684, mmdet/core/anchor/anchor_generator.py:99-143,287-352,
 * mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:144-266, iou_calculators/iou2d_calculator.py:212-260), fp32, contraction off.
 *
 * Anchors: location (x, y) of a level with stride s has ONE square anchor [x s - a/2, y s - a/2, x s + a/2, y s + a/2],
 * a = anchor_scale * s (AnchorGenerator(ratios=[1.0], scales_per_octave=1, octave_base_scale=anchor_scale), center_offset 0):
 * its centre is (x s, y s), without FCOS's + s / 2.
 * Valid anchors of image i (valid_flags with allowed_border = -1): x < min(ceil(pad_w_i / s), w_l), y < min(ceil(pad_h_i / s), h_l).
 * An invalid anchor takes no part in the selection: label = num_classes, cls_weight = 0, assign_idx = -1.
 *
 * dsl_atss_assign: per ground-truth box and level the min(topk, valid anchors of the level) valid anchors with the smallest
 * sqrt(dx^2 + dy^2) between anchor centre and box centre ((x1 + x2) / 2, (y1 + y2) / 2) - every valid anchor of the level is
 * scanned.  TIE RULE: equal distances go to the lower anchor index (y * w_l + x); torch.topk leaves the order of ties unspecified.
 * Threshold = mean + unbiased std (n - 1; NaN, i.e. no positive, for a single candidate) of the candidates' IoUs with the box,
 * summed in ascending (level, rank) order; IoU as BboxOverlaps2D (union clamped at 1e-6).  A candidate is positive iff IoU >=
 * threshold and min(cx - x1, cy - y1, x2 - cx, y2 - cy) > 0.01.  An anchor positive for several boxes takes the one with the highest
 * IoU, equal IoUs the lower ground-truth index.  Every other valid anchor is background with cls_weight 1; an image without
 * ground truth is all background.  ig_boxes / ig_off are not read (ignore_iof_thr = -1).
 * Outputs are dsl_fcos_assign's; bbox_targets holds the assigned ground-truth box in pixels (x1, y1, x2, y2; zeros elsewhere),
 * stats[0] = sum_i max(npos_i, 1) (atss_head.py:554), stats[1] = the sum of the centerness targets (block records added in
 * block order), npos[i] = positives of image i.  No float atomics: conflicts are resolved by a 64-bit integer maximum of
 * (IoU bits << 32 | ~ground-truth index) per anchor, the counts by integer adds - a second run is bit-identical.
 *
 * DSL_HEAD_ATSS in dsl_fcos_desc.head_flags (dsl_fcos_loss, `atss` set) and in dsl_det_desc.head_flags (dsl_fcos_detect, _collect;
 * the descriptor is then a dsl_det_atss_desc): the box is delta2bbox of d = scale_l * x * delta_stds against the anchor - cx = acx + a dx, w = a exp(dw), dw / dh
 * clamped to +-|log(16 / 1000)| (no gradient through an active clamp), corners at +- 0.5 w; detection clips to img_shapes.
 * Loss: the target is the stored ground-truth box, the centerness target comes from the anchor centre and that box; loss_cls and
 * loss_centerness are divided by max(norm[0] * inv_world, 1), loss_bbox - weighted by the centerness target - by
 * max(norm[1] * inv_world, 1) (atss_head.py:268-287; FCOS clamps the latter at 1e-6).  The loss family applies unchanged.
 * ---------------------------------------------------------------------------------------- */
typedef struct dsl_atss_desc {
  int32_t topk;                        /* 1..16 (ATSSAssigner's 9) */
  int32_t max_gt;                      /* capacity of gt_boxes: one workgroup per possible box is launched, >= gt_off[n] */
  float anchor_scale;                  /* octave_base_scale (8), > 0 */
  float delta_stds[4];                 /* DeltaXYWHBBoxCoder target_stds (0.1, 0.1, 0.2, 0.2), > 0; the means are 0 */
  const int32_t* pad_shapes;           /* device [n][2]: (pad_h, pad_w) of every image (img_meta['pad_shape']) */
  int32_t* npos;                       /* device [n], output of dsl_atss_assign: positives per image */
} dsl_atss_desc;
#define DSL_ATSS_MAX_TOPK 16
/* `d` as for dsl_fcos_assign, with DSL_HEAD_ATSS in head_flags and a workspace of dsl_fcos_workspace_bytes(d) */
int dsl_atss_assign(const dsl_fcos_desc* d, const dsl_atss_desc* a, void* stream);

int dsl_fcos_points(const dsl_fcos_desc* d, float* points /* [P][2] */, void* stream);
int dsl_fcos_assign(const dsl_fcos_desc* d, void* stream);
int dsl_fcos_loss(const dsl_fcos_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * GFL: GFLHead's Quality Focal Loss, Distribution Focal Loss and integral box decode (mmdet/models/dense_heads/gfl_head.py:15-48
 * Integral, :210-296 loss_single, :348-370 the avg_factor exchange, :416-443 detection; mmdet/models/losses/gfocal_loss.py:11-78;
 * mmdet/core/bbox/transforms.py:165-186 bbox2distance), fp32, contraction off.
 *
 * A dsl_gfl_desc wraps a dsl_fcos_desc with DSL_HEAD_ATSS | DSL_HEAD_GFL | DSL_HEAD_LOSS_EXT in head_flags: targets come from
 * dsl_atss_assign (bbox_targets = the assigned ground-truth box in pixels).  R = reg_max + 1.  fcos.regctr holds the box predictor's
 * fp32 output [M][ld_rc], ld_rc >= 4R, side k's R logits at columns k R .. k R + R - 1; there is no centerness (ctr, g_ctr NULL, w_ctr,
 * focal_gamma, focal_alpha not read).  A location's point is its anchor's centre (x s, y s).
 *
 * Per positive (label < num_classes), in units of the stride s: z = scale_l * logits, d_k = sum_j j softmax(z_k)_j (Integral),
 * prediction (x - d0, y - d1, x + d2, y + d3), target = bbox_targets / s.
 *
 * dsl_gfl_quality (behind the predictors, in front of the exchange of stats[0:2] between ranks): score[m] = IoU(prediction, target),
 * bbox_overlaps aligned with max(union, 1e-6); weight[m] = max_c sigmoid(cls[m][c]); 0 for every other location.
 * fcos.stats[1] = sum_m weight[m], block records added in block order (bit-identical from run to run); stats[0] stays
 * dsl_atss_assign's sum_i max(npos_i, 1).
 *
 * dsl_gfl_loss (forward and backward in one launch + the fixed-order sum of its block records), with
 * num = max(norm[0] * inv_world, 1), avg = max(norm[1] * inv_world, 1):
 *   losses[0] = w_cls / num * sum_m cls_weight[m] sum_c qfl(m, c), qfl = BCE(x, 0) sigmoid(x)^beta, at a positive's label column
 *               BCE(x, score[m]) |score[m] - sigmoid(x)|^beta (score is a constant for the gradient; beta == 2 multiplies, other
 *               beta >= 0 use powf; at |score - sigmoid| == 0 the gradient is taken as 0, also for beta < 1 where it diverges)
 *   losses[1] = w_bbox / avg * sum_pos weight[m] box_loss(prediction, target), box_kind any DSL_BOX_*
 *   losses[2] = w_dfl / (4 avg) * sum_pos weight[m] sum_k [CE(z_k, l) (l + 1 - t) + CE(z_k, l + 1) (t - l)],
 *               t = clamp(target side distance in stride units, 0, reg_max - 0.1), l = floor(t)
 *   losses[3] = 0; logvec = [cls, bbox, dfl, their sum].
 * g_cls as dsl_fcos_loss.  g_rc[m][0 .. 4R) = scale_l * dL/dz (bf16) for a positive - the box loss chained through the softmax
 * expectation's Jacobian p_j (j - d_k), plus DFL's p_j - [j == l] (l + 1 - t) - [j == l + 1] (t - l) - and the whole row of ld_grc
 * elements zero for every other location; columns 4R .. ld_grc of a positive's row are written zero too: every launch rewrites
 * the whole buffer.  g_scales[l] = sum over the level's positives of dL/dz * logit.  weight is a constant for the gradient.
 * ld_grc: a power of two in 8..512, >= 4R.  Workspace: dsl_fcos_workspace_bytes(&g->fcos).
 *
 * Each wavefront walks 64 locations: the rows of its non-positives are zeroed with 16-byte stores by the whole wavefront, and each
 * positive is processed by the whole wavefront (16 lanes per side, two bins per lane), so no lane runs the 4R-wide row alone.
 * ---------------------------------------------------------------------------------------- */
#define DSL_HEAD_GFL 64         /* GFLHead: dsl_fcos_desc inside a dsl_gfl_desc; dsl_det_desc inside a dsl_det_gfl_desc */
#define DSL_GFL_MAX_REG 16
typedef struct dsl_gfl_desc {
  dsl_fcos_desc fcos;
  int32_t reg_max;                     /* 1..16 */
  float qfl_beta;                      /* QualityFocalLoss beta >= 0 (2) */
  float w_dfl;                         /* DistributionFocalLoss loss_weight >= 0 (0.25) */
  float* score;                        /* [M] out of dsl_gfl_quality, in of dsl_gfl_loss */
  float* weight;                       /* [M] likewise */
} dsl_gfl_desc;
int dsl_gfl_quality(const dsl_gfl_desc* g, void* stream);
int dsl_gfl_loss(const dsl_gfl_desc* g, void* stream);

/* ------------------------------------------------------------------------------------------
 * LD: LDHead's Localization Distillation term on top of GFL (mmdet/models/dense_heads/ld_head.py:99-126 loss_single, :253-261 the
 * reduction of the level lists; mmdet/models/losses/kd_loss.py:27-35 knowledge_distillation_kl_div_loss), fp32, contraction off.
 *
 * A dsl_ld_desc wraps a dsl_gfl_desc whose fcos.head_flags carry DSL_HEAD_LD beside DSL_HEAD_GFL | DSL_HEAD_ATSS | DSL_HEAD_LOSS_EXT;
 * dsl_gfl_desc keeps its size and offsets, and dsl_gfl_quality(&l->gfl) is the quality pass.  soft holds a frozen teacher's box
 * predictor output for the same locations, laid out as fcos.regctr with row stride ld_soft; soft_scales its five Scale values.
 *
 * dsl_ld_loss = everything dsl_gfl_loss does (the same kernel, the LD code behind a template argument), plus for each positive m
 * and side k, with R = reg_max + 1, z = scales[l] * student logits, s = soft_scales[l] * teacher logits, p = softmax(z / T),
 * t = softmax(s / T):
 *   kd(m, k)  = T^2 / R * sum_j t_j (log t_j - log p_j), a term with t_j == 0 counting as 0 (F.kl_div)
 *   losses[3] = w_ld / 4 * sum_pos weight[m] sum_k kd(m, k)
 * losses[3] is NOT divided by avg: the reference divides only loss_bbox and loss_dfl by the exchanged weight sum and leaves loss_ld
 * as weighted_loss(avg_factor=4.0) returned it.  It therefore needs no value from other ranks.  weight[m] is the quality pass's
 * value, a constant for the gradient; the teacher receives no gradient.
 * Gradient: dL/dz_j += w_ld * weight[m] / 4 * T / R * (p_j - t_j) * grad_scale, added to the row's box and DFL gradient in front of
 * the one bf16 rounding of g_rc and chained into g_scales[l] like them (a term that is exactly zero leaves the row's bits as
 * dsl_gfl_loss writes them).  logvec = [cls, bbox, dfl, ld, their sum].
 * Refused: DSL_HEAD_LD without DSL_HEAD_GFL (or a descriptor without DSL_HEAD_LD), soft or soft_scales NULL, ld_soft < 4R,
 * T not finite or < 1, w_ld < 0 or not finite, and whatever dsl_gfl_loss refuses.
 * One soft row load per positive and two more max / sum reductions per side inside the 16-lane groups; no LDS, launch or pass
 * over non-positive rows beyond dsl_gfl_loss's.
 * ---------------------------------------------------------------------------------------- */
#define DSL_HEAD_LD 128         /* LDHead: dsl_gfl_desc inside a dsl_ld_desc */
typedef struct dsl_ld_desc {
  dsl_gfl_desc gfl;
  const float* soft;                   /* teacher's box predictor output, fp32 [M][ld_soft], laid out as fcos.regctr */
  int32_t ld_soft;                     /* >= 4R */
  const float* soft_scales;            /* teacher's 5 Scale values (device) */
  float T;                             /* temperature, finite, >= 1 (kd_loss.py:50) */
  float w_ld;                          /* loss_ld.loss_weight >= 0 */
} dsl_ld_desc;
int dsl_ld_loss(const dsl_ld_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * PAA: probabilistic anchor assignment (mmdet/models/dense_heads/paa_head.py:86-399 loss, get_pos_loss, paa_reassign,
 * gmm_separation_scheme; mmdet/core/bbox/assigners/max_iou_assigner.py:127-212 assign_wrt_overlaps; sklearn.mixture.GaussianMixture
 * as paa_head.py:326-347 sets it up), fp32 with contraction off, the mixture fit in fp64.
 *
 * A dsl_paa_desc wraps a dsl_fcos_desc with DSL_HEAD_ATSS | DSL_HEAD_PAA | DSL_HEAD_LOSS_EXT in head_flags.  PAAHead is an ATSSHead: the
 * anchors, the valid flags, the delta2bbox decode and the gradient layout are DSL_HEAD_ATSS's; fcos.atss supplies anchor_scale,
 * delta_stds, pad_shapes, npos, max_gt and topk - here PAA's per-level top-k, 1..16.  The centerness column of regctr / g_rc carries the
 * IoU-prediction logit and its gradient.  Order of a step: dsl_paa_assign (reads no prediction), the predictors, dsl_paa_pos_loss,
 * dsl_paa_reassign, dsl_paa_loss; DSL_OP_PAA_REFINE is the middle pair.  No call synchronises with the host or allocates.
 *
 * dsl_paa_assign = MaxIoUAssigner(pos_iou_thr = neg_iou_thr, min_pos_iou = 0, ignore_iof_thr = -1, gt_max_assign_all) on the valid
 * anchors, IoU as BboxOverlaps2D (union clamped at 1e-6): an anchor is a candidate of its argmax box if that IoU >= pos_iou_thr, equal
 * maxima go to the lower box index.  Then the low-quality pass: for every box i in ascending order, every valid anchor whose IoU with
 * i equals i's maximum over the image's valid anchors is given to i - even at IoU 0, even if a better box had it; a later box
 * overwrites an earlier one (max_iou_assigner.py:190-198).  Both sides of that comparison are the same fp32 expression, so equal IoUs
 * are equal bits.  Outputs: cand_gt (= assign_idx), labels (the box's label, or num_classes), bbox_targets (the box in pixels, zeros
 * elsewhere), cls_weight (1 valid, 0 invalid anchor), pos_weight 1; stats and npos are cleared.  ig_boxes are not read.  No atomics:
 * a second run is bit-identical.
 *
 * dsl_paa_pos_loss (behind the predictors): for every candidate pos_loss[m] = w_cls * sum_c focal(m, c) + w_bbox * box_loss(decode(m),
 * target) with the head's focal gamma / alpha and box_kind - the reference's reduction_override='none', where avg_factor is not
 * applied (paa_head.py:201-255) - and 0 elsewhere.  It also leaves the aligned IoU of the same two boxes (union clamped at 1e-6) in
 * iou_target[m] for every candidate, 0 elsewhere.
 * dsl_paa_pos_loss and dsl_paa_reassign are an ORDERED PAIR: dsl_paa_reassign keeps iou_target where an anchor stays positive and
 * clears it where it does not, and neither it nor dsl_paa_assign restores a cleared value.  So dsl_paa_reassign is right only
 * directly behind a dsl_paa_pos_loss of the same assignment and head outputs (pos_loss itself may be rewritten in between);
 * DSL_OP_PAA_REFINE is that pair.  Run again without dsl_paa_pos_loss on unchanged inputs it repeats its result bit for bit.
 *
 * dsl_paa_reassign, one workgroup per ground-truth box (max_gt launched): per level the min(topk, count) candidates of the box with
 * the smallest pos_loss, concatenated in level order and sorted ascending.  TIE RULE in both places: equal losses go to the lower
 * location index (torch.topk / sort leave it unspecified).  Fewer than two samples: the box keeps none (gmm_flags 1).  Else
 * GaussianMixture(2, covariance_type='diag', weights (0.5, 0.5), means (min, max), precisions (1, 1), tol 1e-3, reg_covar 1e-6,
 * max_iter 100) is fitted by the workgroup's first wavefront (at most 80 samples, two per lane, fixed-order butterfly sums): the lower
 * bound is the mean of the E-step's log-normaliser, starting from -inf, the loop stops when |change| < tol, the parameters are those
 * of the last M-step: nk = sum resp + 10 eps(fp64), mean = resp . x / nk, variance = resp . (x * x) / nk - mean^2 + reg_covar, weights
 * nk / sum nk.  The arithmetic is fp64 on the fp32 losses.  What sklearn 1.7.2 does with float32 input was read from its source and
 * confirmed on the fixtures (scores within 3e-10 of sklearn's on every fitted box): the samples stay float32, so x * x (M-step),
 * x**2 (E-step) and the initial means**2 are float32 products widened afterwards, log(2 pi) is rounded to float32, everything else is
 * float64.  predict = argmax of the weighted log-probabilities (component 0 = the low-loss one, ties to 0), score_samples = their
 * logsumexp.  With fgs = the samples of component 0, the positives are the first j + 1 of them in sorted order, j the position within
 * fgs of the highest score (equal scores: the first; paa_head.py:392-399).  Nothing is ignored.
 * DEVIATION: where a variance comes out <= 0 sklearn raises ("ill-defined empirical covariance") and the reference's training step
 * dies; here the box keeps no positive, gmm_flags = 2, and the step goes on.
 * Every candidate that is not kept gets label = num_classes, assign_idx = -1, pos_weight = 0, iou_target = 0; cls_weight stays 1.  The
 * kept ones keep dsl_paa_pos_loss's iou_target, a constant for the gradient.  gmm_iters[g] = EM iterations (sklearn's n_iter_; 0 = not
 * fitted), gmm_flags[g] = 0 fitted | 1 fewer than two candidates | 2 ill-defined covariance.  npos[i] = positives of image i,
 * stats[0] = sum_i npos_i (not clamped per image), stats[1] = sum_m iou_target[m], from the boxes' records added in box order.
 *
 * dsl_paa_loss = the DSL_HEAD_ATSS loss kernel behind the flag (forward and backward in one launch, paa_head.py:169-199):
 *   losses[0] = w_cls / max(norm[0], n) * sum focal          losses[2] = w_ctr / norm[0] * sum_pos BCE(iou logit, iou_target)
 *   losses[1] = w_bbox / norm[1] * sum_pos max(iou_target, 1e-12) * box_loss
 * both box terms and their gradients are 0 without a positive.  norm is this rank's own stats: the reference does not reduce_mean
 * here, so the host passes inv_world = 1 and exchanges nothing.  norm[1] == 0 with positives present (every IoU exactly 0) is the
 * reference's own division by zero; the kernel divides by 1 instead.  logvec = [cls, bbox, iou, sum]; the gradient buffers use the
 * ATSS layout, the IoU logit's gradient where the centerness gradient goes.
 * Refused, with dsl_last_error naming the field: head_flags other than the three above (or with DSL_HEAD_GFL / DSL_HEAD_LD),
 * atss.topk, atss.max_gt, atss.pad_shapes, atss.npos, pos_iou_thr outside (0, 1), a null pos_loss / iou_target / cand_gt / gmm_iters /
 * gmm_flags, a workspace below dsl_fcos_workspace_bytes(&q->fcos), and what DSL_HEAD_ATSS refuses.
 * ---------------------------------------------------------------------------------------- */
#define DSL_HEAD_PAA 256        /* PAAHead: dsl_fcos_desc inside a dsl_paa_desc; dsl_det_desc inside a dsl_det_paa_desc */
typedef struct dsl_paa_desc {
  dsl_fcos_desc fcos;
  float pos_iou_thr;                   /* MaxIoUAssigner pos_iou_thr == neg_iou_thr, in (0, 1) (0.1) */
  float* pos_loss;                     /* [M] out of dsl_paa_pos_loss, in of dsl_paa_reassign */
  float* iou_target;                   /* [M] out of dsl_paa_pos_loss / dsl_paa_reassign, in of dsl_paa_loss */
  int32_t* cand_gt;                    /* [M] the first assignment's box index within the image, -1 if none */
  int32_t* gmm_iters;                  /* [max_gt] EM iterations per box, 0 if not fitted */
  int32_t* gmm_flags;                  /* [max_gt] 0 fitted, 1 fewer than two candidates, 2 ill-defined covariance */
} dsl_paa_desc;
int dsl_paa_assign(const dsl_paa_desc* q, void* stream);
int dsl_paa_pos_loss(const dsl_paa_desc* q, void* stream);
int dsl_paa_reassign(const dsl_paa_desc* q, void* stream);
int dsl_paa_loss(const dsl_paa_desc* q, void* stream);

/* ------------------------------------------------------------------------------------------
 * FoveaBox: FoveaHead's painted-rectangle targets, focal + SmoothL1 loss and base_len * exp decode
 * (mmdet/models/dense_heads/fovea_head.py:130-132 points, :134-182 loss, :206-265 targets, :298-348 detection;
 * mmdet/models/losses/smooth_l1_loss.py:11-29; losses/focal_loss.py:11-56), fp32, contraction off.
 *
 * A dsl_fovea_desc wraps a dsl_fcos_desc with DSL_HEAD_FOVEA | DSL_HEAD_LOSS_EXT in head_flags and no other head or option flag.
 * The point of location (x, y) of a level with stride s is (s (x + 0.5), s (y + 0.5)).  fcos.regctr holds conv_reg's four raw
 * outputs (ld_rc >= 4): there is no Scale, no centerness (scales, g_scales, ctr, g_ctr are not read or written), no ignore boxes
 * (ig_boxes must be NULL), no stream weight (loss_weight == 1) and no sisoft term (soft_weight == 0).  fcos.range_lo / range_hi /
 * radius are not read: the levels' ranges are lo / hi below.
 *
 * dsl_fovea_assign, one thread per location, the image's boxes staged through LDS in chunks (no cap but the capacity of gt_boxes):
 * area = sqrtf((x2 - x1) * (y2 - y1)); a box hits level l iff lo[l] <= area <= hi[l].  With b = box / s (four divisions; when every
 * stride is a power of two, four products with the exact 1 / s, which are the same bits for every coordinate that is not subnormal),
 * half_w = 0.5 (b.x2 - b.x1):  left = clamp(ceil((b.x1 + (1 - sigma) half_w) - 0.5), 0, w_l - 1),
 * right = clamp(floor((b.x1 + (1 + sigma) half_w) - 0.5), 0, w_l - 1), top / down likewise; 1 - sigma and 1 + sigma are formed in
 * fp64 from the descriptor's float and rounded once (the reference multiplies by the Python float).  The box covers the location
 * iff left <= x <= right and top <= y <= down - both ranges tested after the clamp, so a fovea wholly beyond an edge still covers
 * the border cell and one between two cell centres covers nothing.  Every sum and product above is a separate fp32 operation in
 * the order written (the file is compiled without contraction), which is the reference's torch arithmetic.  Among the covering
 * hits the one of smallest area wins (the reference paints in order of decreasing area).  EQUAL areas: the higher box index wins -
 * what a stable sort gives; the reference's torch.sort is not stable there, so this order is unpinned.
 * Outputs: labels (the box's label, else num_classes), assign_idx (box index within the image, -1 = none), bbox_targets =
 * log(clamp(((px - x1) / base_len, (py - y1) / base_len, (x2 - px) / base_len, (y2 - py) / base_len), 1/16, 16)) from the undivided
 * box, and exactly 0 where nothing was painted (the reference leaves uninitialised memory there and never reads it); cls_weight =
 * pos_weight = 1.  stats[0] = num_pos + n (loss_cls's avg_factor, fovea_head.py:165-166), stats[1] = max(num_pos, 1), stats[2..7] =
 * 0: per-workgroup counts added in workgroup order - no atomics on floats, a second run is bit-identical.
 *
 * dsl_fovea_loss (forward and backward in one launch + the fixed-order sum of its block records), num = max(norm[0] * inv_world,
 * 1), avg = max(norm[1] * inv_world, 1) - the host passes its own stats and inv_world = 1, the reference does not reduce_mean:
 *   losses[0] = w_cls / num * sum_m cls_weight[m] sum_c focal(m, c), gamma >= 0 and 0 <= alpha <= 1 as the loss family's; for gamma
 *               != 2 the modulating factor is formed as exp(-gamma * softplus), not by powf (gamma = 1.5 in configs/foveabox)
 *   losses[1] = w_bbox / avg * sum_pos sum_k sl1(regctr[m][k] - bbox_targets[m][k]),
 *               sl1(d) = 0.5 d^2 / beta where |d| < beta, else |d| - 0.5 beta;  exactly 0 without a positive
 *   losses[2] = losses[3] = 0; logvec = [cls, bbox, their sum].
 * g_cls as dsl_fcos_loss (columns from C on stay zero).  g_rc[m][0..3] = w_bbox / avg * grad_scale * (d / beta or sign(d)), bf16, for
 * a positive; columns 0..7 of every row are rewritten by every launch (zero for a non-positive and in columns 4..7).  A wavefront
 * walks 64 locations.  Workspace: dsl_fcos_workspace_bytes(&f->fcos).
 * Refused, with dsl_last_error naming the field: head_flags other than DSL_HEAD_FOVEA | DSL_HEAD_LOSS_EXT, fcos.ig_boxes,
 * fcos.soft_weight != 0, fcos.loss_weight != 1, fcos.ctr / g_ctr, sigma outside (0, 1], base_len <= 0, lo > hi, smooth_l1_beta <= 0,
 * a workspace below dsl_fcos_workspace_bytes.
 *
 * Detection (DSL_HEAD_FOVEA in dsl_det_desc.head_flags, the descriptor being a dsl_det_fovea_desc): the pair score is the class
 * sigmoid alone, x1 = clamp(px - base_len exp(p0), 0, img_w - 1) and so on (fovea_head.py:326-333: the clamp is to img_shape - 1);
 * scales and ctr are not read.  dsl_fcos_detect_collect refuses the flag: FoveaHead.get_bboxes has no with_nms argument.
 * ---------------------------------------------------------------------------------------- */
#define DSL_HEAD_FOVEA 512      /* FoveaHead: dsl_fcos_desc inside a dsl_fovea_desc; dsl_det_desc inside a dsl_det_fovea_desc */
typedef struct dsl_fovea_desc {
  dsl_fcos_desc fcos;
  float sigma;                         /* the fovea's share of the box, in (0, 1] (0.4) */
  float base_len[DSL_MAX_SEG];         /* base_edge_list: the unit of a level's log distances, > 0 (16, 32, 64, 128, 256) */
  float lo[DSL_MAX_SEG], hi[DSL_MAX_SEG];   /* scale_ranges: sqrt(area) bounds of a level, lo <= hi */
  float smooth_l1_beta;                /* SmoothL1Loss beta > 0 (0.11 in the reference's configs) */
} dsl_fovea_desc;
int dsl_fovea_assign(const dsl_fovea_desc* f, void* stream);
int dsl_fovea_loss(const dsl_fovea_desc* f, void* stream);

/* ------------------------------------------------------------------------------------------
 * AutoAssign: AutoAssignHead's differentiable label assignment - no hard assigner - and its three losses
 * (mmdet/models/dense_heads/autoassign_head.py:81-119 centre prior, :173-187 points, :204-212 forward, :238-256 positive loss,
 * :282-310 negative loss, :384-437 IoU / normalisers / centre loss / the batch without boxes, :492-509 inside mask;
 * bbox_overlaps and GIoULoss as the other heads'), fp32, contraction off.
 *
 * A dsl_aa_desc wraps a dsl_fcos_desc with DSL_HEAD_AUTOASSIGN | DSL_HEAD_LOSS_EXT in head_flags and no other head or option flag.
 * The point of location (x, y) of a level with stride s is (x s, y s): no half-stride offset.  fcos.regctr holds conv_reg's four raw
 * outputs and the objectness logit (conv_centerness on the regression tower) in column 4 (ld_rc >= 8); the box prediction is
 * relu(scales[l] x) s, decoded as (px - d0, py - d1, px + d2, py + d3).  No ignore boxes (ig_boxes must be NULL), no stream weight
 * (loss_weight == 1), no sisoft term (soft_weight == 0), fcos.ctr / g_ctr NULL; fcos.range_lo / range_hi / radius, the focal
 * settings, w_cls and w_ctr are not read, box_kind must be DSL_BOX_GIOU.  labels, bbox_targets, assign_idx, cls_weight and
 * pos_weight are neither read nor written: there is no per-location target.
 * A pair (point i, box g of its image) is INSIDE iff min(px - x1, py - y1, x2 - px, y2 - py) > 0 in fp32.  For inside pairs
 *   c(i, g) = prod_{d = x, y} exp(-(((p_d - centre_d(g)) / s - mean[label_g][d])^2) / (2 sigma[label_g][d]^2)),  else 0,
 * mean / sigma fp32 [C][2] (the trained parameters center_prior.mean / .sigma).  A box whose label is outside [0, C) has no row in
 * the prior; the host refuses such labels where it sees them (FcosLossPlan.set_targets, labels on the host).  Arriving on the
 * device, the box is never dereferenced by its label and: counts in stats[0] and in its image's n_boxes of the centre loss (both are
 * gt_off differences); adds nothing to stats[1], to sum c of its image, to the positive loss (its term is 0, not 100), to any
 * gradient or negative weight; and still takes part in iou(i), which is over all boxes of the image.
 *
 * dsl_aa_assign - what depends on the boxes and the prior alone, so that the ranks' sums can be exchanged while the forward
 * pass runs: stats[0] = the boxes of the batch (gt_off[n]), stats[1] = sum over all pairs of c, stats[2..7] = 0.  One wavefront per
 * box walks the box's footprint on every level; lane partial sums in footprint order, an xor butterfly, then the boxes' records
 * in box order.
 *
 * dsl_aa_loss (forward and backward), with N_pos = max(norm[0] * inv_world, 1), N_neg = max(norm[1] * inv_world, 1) - norm holds
 * the sum over ranks of stats[0:2] (reduce_mean, :407-408, :414-416):
 *   iou(i)   = max over ALL boxes of image(i) of the plain IoU (union clamped at 1e-6) of the decoded box - not only the boxes that
 *              hold i; written to `iou`; no gradient
 *   reg(i,g) = w_bbox * (1 - giou(decoded box, box g)),  p_pos = sigmoid(cls[i][label_g]) sigmoid(obj[i]) exp(-reg),
 *   w = exp(3 p_pos) c,  R_g = sum_i p_pos w / max(sum_i w, 1e-12)
 *   losses[0] = w_pos / N_pos * sum_g -max(log R_g, -100)      (a box that holds no point: R = 0, its term is 100)
 *   t(i) = 1 / max(1 - iou(i), 1e-12), per box over its inside points t_norm = (t - min + 1e-12) / (max - min + 1e-12);
 *   p_neg_weight[i][label_g] = 1 - t_norm, 1 elsewhere; where several boxes of one class hold a point, the HIGHEST box index wins
 *   (the reference's index assignment on the CPU; pinned by the fixtures)
 *   q = sigmoid(cls) sigmoid(obj) p_neg_weight,  losses[1] = w_neg / N_neg * sum_{i, c} q^2 * -max(log(1 - q), -100)
 *   losses[2] = w_center / n * sum_images [ n_boxes / max(sum c, 1e-12) if the image has an inside pair, else 0 ]  (this rank's)
 *   a batch without boxes: losses[0] = losses[2] = 0 and no gradient for the prior; losses[1] with weights 1.  losses[3] = 0;
 *   logvec = [pos, neg, center, their sum].
 * Gradients, all times grad_scale: g_cls [M][ld_gcls] bf16 (columns below C written), g_rc [M][ld_grc] bf16 - columns 0..3 through
 * the stride, the ReLU and the Scale, column 4 the objectness, 5..7 zero - g_scales [nlvl], g_mean / g_sigma fp32 [C][2]
 * (overwritten).  The gradient flows through exp(3 p_pos) and through c (into R and into the centre loss); the BCE derivatives
 * are torch's, (x - target) / max((1 - x) x, 1e-12).  N_pos and N_neg carry none.
 * Launches: a per-point pass (boxes staged through LDS in chunks of 64) for iou; a per-box pass (one wavefront per box over its
 * footprint) for sum c, sum w, sum p w, min / max t; a per-image pass; a per-point pass, one wavefront per location - a lane per box
 * for the positive terms, the boxes that hold the point then taken in ascending index by the lane that owns their class, a lane per
 * class for the negative loss; a per-box pass for one d mean / d sigma record per box; one workgroup that adds the block records,
 * the boxes' terms and, per class, the boxes' records in box order.  No float atomics; a second run is bit-identical.
 * Workspace: dsl_fcos_workspace_bytes(&f->fcos) (it reads max_gt).
 * Refused, with dsl_last_error naming the field: head_flags other than DSL_HEAD_AUTOASSIGN | DSL_HEAD_LOSS_EXT, fcos.ig_boxes,
 * fcos.soft_weight != 0, fcos.loss_weight != 1, fcos.ctr / g_ctr, num_classes outside 1..128, max_gt outside 1..2^20, a negative
 * or non-finite weight, box_kind other than DSL_BOX_GIOU, ld_rc < 8, null mean / sigma / g_mean / g_sigma / iou, a workspace
 * below dsl_fcos_workspace_bytes.  dsl_fcos_assign / dsl_fcos_loss refuse the flag.
 * ---------------------------------------------------------------------------------------- */
#define DSL_HEAD_AUTOASSIGN 1024   /* AutoAssignHead: dsl_fcos_desc inside a dsl_aa_desc */
typedef struct dsl_aa_desc {
  dsl_fcos_desc fcos;
  float w_pos, w_neg, w_center;        /* pos_loss_weight, neg_loss_weight, center_loss_weight (0.25, 0.75, 0.75) */
  int32_t max_gt;                      /* capacity of fcos.gt_boxes / gt_labels in boxes: sizes the per-box launches and records */
  const float* mean;                   /* [C][2] center_prior.mean */
  const float* sigma;                  /* [C][2] center_prior.sigma (!= 0) */
  float* g_mean;                       /* [C][2], overwritten by dsl_aa_loss */
  float* g_sigma;                      /* [C][2], overwritten by dsl_aa_loss */
  float* iou;                          /* [M], written by dsl_aa_loss */
} dsl_aa_desc;
int dsl_aa_assign(const dsl_aa_desc* f, void* stream);
int dsl_aa_loss(const dsl_aa_desc* f, void* stream);

/* One dispatch for every head, on head_flags.  The contract the flags state: with DSL_HEAD_GFL `d` is the first member of a
 * dsl_gfl_desc, with DSL_HEAD_LD of a dsl_ld_desc (whose first member is that dsl_gfl_desc), so the three share one address.
 * With DSL_HEAD_PAA `d` is the first member of a dsl_paa_desc, with DSL_HEAD_FOVEA of a dsl_fovea_desc, with DSL_HEAD_AUTOASSIGN of a
 * dsl_aa_desc.
 * dsl_head_assign: DSL_HEAD_AUTOASSIGN -> dsl_aa_assign, else DSL_HEAD_FOVEA -> dsl_fovea_assign, else DSL_HEAD_PAA -> dsl_paa_assign, else DSL_HEAD_ATSS ->
 * dsl_atss_assign(d, d->atss), else dsl_fcos_assign.
 * dsl_head_loss: DSL_HEAD_AUTOASSIGN -> dsl_aa_loss, else DSL_HEAD_FOVEA -> dsl_fovea_loss, else DSL_HEAD_PAA -> dsl_paa_loss, else DSL_HEAD_LD -> dsl_ld_loss (which refuses
 * the flag without DSL_HEAD_GFL), else
 * DSL_HEAD_GFL -> dsl_gfl_loss, else dsl_fcos_loss.  DSL_OP_ASSIGN / DSL_OP_LOSS of an op list are these two calls on the op's desc. */
int dsl_head_assign(const dsl_fcos_desc* d, void* stream);
int dsl_head_loss(const dsl_fcos_desc* d, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer / EMA over flat fp32 buffers (mmcv OptimizerHook + torch SGD, wired at
 * apis/train.py:111,157-166; EMA at runner/hooks/semi_epoch_based_runner.py:368-409)
 * ---------------------------------------------------------------------------------------- */
int dsl_sumsq(const float* x, long n, float* out /* [1], accumulated */, void* stream);
/* the same sum, overwritten (not accumulated), summed in a fixed order: workspace >= 1024 floats */
int dsl_sumsq_det(const float* x, long n, float* out /* [1] */, float* workspace, void* stream);
/* p -= lr*lr_mult[i] * (m = mom*m + (g*clip + wd*wd_mult[i]*p)); also writes bf16(p) to p16.
 * clip = min(max_norm/(sqrt(*gnorm_sq)+1e-6), 1) when gnorm_sq != NULL.  group[i] in {0,1}:
 * 1 = bias group (lr*bias_lr_mult, wd*bias_decay_mult). */
int dsl_sgd_step(float* p, const float* g, float* m, void* p16, const uint8_t* group, long n,
                 float lr, float momentum, float wd, float bias_lr_mult, float bias_decay_mult,
                 const float* gnorm_sq, float max_norm, int first_step, void* stream);
/* The optimizer family: what mmdet/apis/train.py:111 `build_optimizer(model, cfg.optimizer)` builds beyond plain momentum SGD -
 * torch.optim.SGD(nesterov=True), Adam, AdamW - with mmcv DefaultOptimizerConstructor's paramwise_cfg as a table of up to
 * DSL_OPT_MAX_GROUPS (lr, wd) pairs; group[i] is element i's row.  One pass like dsl_sgd_step: clip, update, bf16(p) to p16.
 * With d0 = g * clip, clip = min(max_norm / (sqrt(*gnorm_sq) + 1e-6), 1) when gnorm_sq != NULL (else 1), k = group[i]:
 *   SGD    d = d0 + wd[k] p;  m = d (first_step) or momentum m + d;  p -= lr[k] (nesterov ? d + momentum m : m)
 *   ADAM   d = d0 + wd[k] p;  m = beta1 m + (1 - beta1) d;  v = beta2 v + (1 - beta2) d d;
 *          p -= lr[k] step_scale * m / (sqrt(v) rsqrt_bc2 + eps)
 *   ADAMW  p *= 1 - lr[k] wd[k], then ADAM's update with d = d0
 * (torch's single-tensor formulas).  The bias corrections come from the host, computed in double for step t = 1, 2, ..:
 * step_scale = 1 / (1 - beta1^t), rsqrt_bc2 = 1 / sqrt(1 - beta2^t); there is no device step counter.  The descriptor is copied
 * into the launch's kernel arguments: nothing is allocated and no device table has to stay alive.  Refused before anything is
 * launched: a null d / p / g / m / group, v == NULL for an Adam kind, n <= 0 or n % 4 != 0, p / g / m / v not 16-byte aligned
 * (p16: 8, group: 4), kind or n_groups out of range, nesterov with momentum == 0.  v may be NULL for SGD, p16 may be NULL. */
#define DSL_OPT_SGD   0
#define DSL_OPT_ADAM  1
#define DSL_OPT_ADAMW 2
#define DSL_OPT_MAX_GROUPS 16
typedef struct dsl_optim_desc {
  int32_t kind, n_groups;
  float lr[DSL_OPT_MAX_GROUPS], wd[DSL_OPT_MAX_GROUPS];      /* absolute, per group */
  float momentum; int32_t nesterov, first_step;              /* SGD */
  float beta1, beta2, eps, step_scale, rsqrt_bc2;            /* Adam kinds */
  float max_norm;
} dsl_optim_desc;
int dsl_optim_step(const dsl_optim_desc* d, float* p, const float* g, float* m, float* v /* NULL for SGD */, void* p16 /* may be NULL */,
                   const uint8_t* group, long n, const float* gnorm_sq /* NULL: no clip */, void* stream);
/* Gradient accumulation over flat fp32 buffers (mmcv GradientCumulativeOptimizerHook): the gradient of one micro-step joins the
 * window's running sum.  Plain fp32 adds in micro-step order - one rounding per element and call, no atomics, denormals kept - i.e.
 * the bits of torch's `p.grad += g`.  n > 0, n % 4 == 0, both pointers 16-byte aligned (checked before anything is launched). */
#define DSL_ACC_SET  0   /* acc[i]  = g[i]           first micro-step of a window (acc is not read) */
#define DSL_ACC_ADD  1   /* acc[i] += g[i]           */
#define DSL_ACC_FOLD 2   /* g[i]    = acc[i] + g[i]  closing micro-step: g then holds the window's sum; acc is left as is */
int dsl_grad_accumulate(float* acc, float* g, long n, int mode, void* stream);
int dsl_ema_lerp(float* teacher, const float* student, long n, float keep, void* stream);
/* the same, and the teacher's bf16 forward copy written in the same pass (what dsl_cast_bf16 would re-read the result for) */
int dsl_ema_lerp_bf16(float* teacher, const float* student, void* teacher_bf16, long n, float keep, void* stream);
int dsl_cast_bf16(const float* x, void* y, long n, void* stream);
/* bf16 -> fp32 (n % 4 == 0): the way back of a gradient bucket that crossed xGMI as bf16 (dsl_allreduce_bucket_bf16). */
int dsl_cast_f32(const void* x_bf16, float* y, long n, void* stream);
/* The clipping norm in pieces, for data parallel with grad_clip (every DSL config: mmcv OptimizerHook's clip_grad_norm_,
 * mmdet/apis/train.py:157-166): one dsl_sumsq_partial per gradient bucket as its all-reduce completes (DSL_SUMSQ_PARTS block
 * sums of x[0..n) -> partials), one dsl_sumsq_fold over all of them (index order) behind the last bucket.  No atomics. */
#define DSL_SUMSQ_PARTS 256
int dsl_sumsq_partial(const float* x, long n, float* partials /* [DSL_SUMSQ_PARTS] */, void* stream);
int dsl_sumsq_fold(const float* partials, int n_partials, float* out /* [1] */, void* stream);
/* KRSC fp32 -> CRSK bf16 ("dgrad pack"), optional per-cout scale fold. */
int dsl_pack_dgrad(const float* w, const float* scale, void* out, int cout, int cout_pad, int taps,
                   int cin, void* stream);
/* the same for many convs in ONE launch: `items` is a DEVICE array of n entries */
typedef struct dsl_pack_item {
  const float* w; const float* scale; void* out;
  int32_t cout, cout_pad, taps, cin;
  int32_t block_start, tiles_ci, tiles_co;             /* 64x64 (cout x cin) tiles; block_start: prefix sum of tiles_ci*tiles_co*taps */
  int32_t tapmap;   /* 0: out tap t = source tap t of `taps`.  Else a tap SELECTION (the parity-class packs of a stride-2 3x3 data
                     * gradient): bits 16-23 = taps of the source weight (9), nibble t (bits 4t..4t+3) = source tap of out tap t,
                     * 0xF = a zero tap; `taps` (<= 4) counts the OUT taps */
} dsl_pack_item;
int dsl_pack_dgrad_batched(const dsl_pack_item* items_dev, int n, int total_blocks, void* stream);

/* ------------------------------------------------------------------------------------------
 * Teacher sweep post-processing (fcos_head.py:406-548, core/post_processing/bbox_nms.py:7-94)
 * ---------------------------------------------------------------------------------------- */
typedef struct dsl_det_desc {
  int32_t nlvl, n;
  int32_t h[DSL_MAX_SEG], w[DSL_MAX_SEG], stride[DSL_MAX_SEG];
  int32_t num_classes, nms_pre, max_per_img;
  float score_thr, iou_thr;
  const float* cls_logits; int32_t ld_cls;
  const float* regctr; int32_t ld_rc;        /* raw conv_reg; scale, relu, *stride applied here */
  const float* scales;
  const float* img_shapes;                   /* [n][2] (h, w) clip bounds */
  const float* scale_factors;                /* [n][4] */
  float* dets;                               /* [n][max_per_img][5] */
  int64_t* det_labels;                       /* [n][max_per_img] */
  int32_t* det_count;                        /* [n] */
  void* workspace; size_t workspace_bytes;
  int32_t head_flags;                        /* DSL_HEAD_EXP_DECODE: exp(scale x) without the stride (fcos_head.py:162-167); 0 = relu * stride */
  int32_t ld_ctr;                            /* row stride of ctr (floats); read only when ctr is set */
  const float* ctr;                          /* NULL: centerness logit = regctr[m][4]; else ctr[m * ld_ctr] (fcos_head.py:155-158) */
  int32_t nms_method;                        /* DSL_NMS_*; 0 = the hard NMS, and soft_sigma / soft_min_score are not read */
  float soft_sigma;                          /* DSL_NMS_GAUSSIAN: w = exp(-iou^2 / soft_sigma), > 0 (mmcv: 0.5) */
  float soft_min_score;                      /* Soft-NMS: a candidate whose decayed score is < soft_min_score is dropped, >= 0 (mmcv: 1e-3) */
} dsl_det_desc;
/* An ATSS head's detection descriptor: with DSL_HEAD_ATSS in det.head_flags the dsl_det_desc handed to dsl_fcos_detect /
 * dsl_fcos_detect_collect is the first member of one of these (dsl_det_desc itself keeps its layout), and `atss` supplies
 * anchor_scale and delta_stds (atss_head.py:420-495). */
typedef struct dsl_det_atss_desc {
  dsl_det_desc det;
  const struct dsl_atss_desc* atss;
} dsl_det_atss_desc;
/* A GFL head's detection descriptor (DSL_HEAD_GFL in det.head_flags, no other decode flag; gfl_head.py:416-443): regctr holds
 * [M][ld_rc >= 4 (reg_max + 1)] distribution logits, distances = Integral(scale_l * logits) * stride from the anchor centre (x s, y s),
 * boxes clipped to img_shapes; the candidate score is the class sigmoid alone (no centerness factor: ctr is not read), nms_pre ranks
 * by the location's maximum class score.  Everything behind candidate collection is shared. */
typedef struct dsl_det_gfl_desc {
  dsl_det_desc det;
  int32_t reg_max;                           /* 1..16 */
} dsl_det_gfl_desc;
/* A PAA head's detection descriptor (DSL_HEAD_ATSS | DSL_HEAD_PAA in det.head_flags; PAAHead._get_bboxes and score_voting,
 * mmdet/models/dense_heads/paa_head.py:519-673): ATSS's decode.  The pair score is sqrt(sigmoid(cls) * sigmoid(iou)), the IoU logit
 * where ATSS has its centerness logit: nms_pre ranks by its per-location maximum, score_thr applies to it, and it is the final score -
 * there is no centerness factor.  With score_voting one more launch runs behind the (hard) NMS, one wavefront per kept detection:
 * over the image's pre-NMS pairs of the same class with score > score_thr and IoU > 0.01 with the kept box (bbox_overlaps, union
 * clamped at 1e-6), p = exp(-(1 - iou)^2 / 0.025) * score; the box becomes sum p * box / sum p (fp64 sums of a fixed order), the score
 * stays; the output is ordered class ascending, then by the NMS's order (det_count is the NMS's).  Boxes are in the frame the
 * reference votes in: divided by scale_factors when those are given (rescale).  The voting pool is the set of pairs dsl_fcos_detect
 * keeps for the NMS - its best 16 384 per image: the existing deviation of this library, carried over.  Test-time augmentation is
 * refused for this head, as in the reference (paa_head.py:536-538: with_nms=False is not supported): dsl_fcos_detect_collect refuses
 * the flag.  score_voting with a Soft-NMS method is refused. */
typedef struct dsl_det_paa_desc {
  dsl_det_atss_desc atss;
  int32_t score_voting;                      /* 0 = the NMS output as it is */
} dsl_det_paa_desc;
/* A Fovea head's detection descriptor (DSL_HEAD_FOVEA in det.head_flags, no other flag; FoveaHead._get_bboxes,
 * mmdet/models/dense_heads/fovea_head.py:298-348): regctr holds conv_reg's four raw outputs, the box is (px - base_len exp(p0),
 * py - base_len exp(p1), px + base_len exp(p2), py + base_len exp(p3)) from the point (s (x + 0.5), s (y + 0.5)), clamped to
 * [0, img_w - 1] x [0, img_h - 1]; the candidate score is the class sigmoid alone (scales and ctr are not read).  Test-time
 * augmentation is refused for this head, as in the reference (FoveaHead.get_bboxes has no with_nms argument,
 * dense_test_mixins.py:62-70): dsl_fcos_detect_collect refuses the flag. */
typedef struct dsl_det_fovea_desc {
  dsl_det_desc det;
  float base_len[DSL_MAX_SEG];               /* base_edge_list, > 0 */
} dsl_det_fovea_desc;
/* An AutoAssign head's detection (DSL_HEAD_AUTOASSIGN in a plain dsl_det_desc's head_flags, no other flag, ctr NULL;
 * autoassign_head.py:173-187,204-212 with FCOSHead._get_bboxes, fcos_head.py:419-516): FCOS's decode relu(scales[l] x) s and candidate
 * score sigmoid(cls) * sigmoid(regctr[m][4]) from the point (x s, y s) - no half-stride offset - clipped to img_shape.
 * get_bboxes has with_nms, so dsl_fcos_detect_collect / _finish serve the head as they serve FCOS's. */
/* dsl_det_desc.nms_method.  Soft-NMS is mmcv's batched_nms with nms=dict(type='soft_nms', method=...) (stated by
 * mmdet/ops/nms/src/soft_nms_cpu.pyx:22-127), per image and class over the candidates the hard NMS would get: pick the highest current score
 * (equal scores: the candidate that comes first in (level, slot, class) order - with views, (view, level, slot, class)), emit it
 * with that score, multiply every other remaining score of the class by w, drop those that fall below soft_min_score, repeat;
 * then the emitted detections of all classes by rescored score, the first max_per_img.  dets[..][4] is the RESCORED score.
 * w with iou = IoU(pick, other), the hard NMS's expression on the class-offset boxes:
 *   LINEAR 1 - iou if iou > iou_thr, else 1;  GAUSSIAN exp(-iou^2 / soft_sigma);  NAIVE 0 if iou > iou_thr, else 1.
 * The workspace / pool sizes grow by 16 384 floats per image when nms_method != 0: query them with the field set. */
#define DSL_NMS_HARD 0
#define DSL_NMS_LINEAR 1
#define DSL_NMS_GAUSSIAN 2
#define DSL_NMS_NAIVE 3
size_t dsl_detect_workspace_bytes(const dsl_det_desc* d);
int dsl_fcos_detect(const dsl_det_desc* d, void* stream);

/* Test-time augmentation: BBoxTestMixin.aug_test_bboxes (mmdet/models/dense_heads/dense_test_mixins.py:38-108) over the views
 * MultiScaleFlipAug made of ONE image.  dsl_fcos_detect split where the reference's with_nms=False returns; the candidates of
 * all views meet in a caller-owned pool, and one sort + NMS runs over it.  At most DSL_MAX_AUG views.
 *
 * Pool (dsl_detect_aug_workspace_bytes; reads d->nlvl, nms_pre, num_classes, d->n == 1): a record per view (the nlvl, nms_pre and
 * num_classes it was collected with), valid rows per (view, level), every view's scale factor, then nviews * nlvl * nms_pre candidate rows of 5 + num_classes floats - mapped-back box, sigmoid
 * centerness, sigmoid class scores - view v's level l at row (v * nlvl + l) * nms_pre, and behind them the scratch of finish.
 * The views may differ in their level sizes; nlvl, nms_pre and num_classes are the pool's and the same for all.  Returns 0
 * (and sets dsl_last_error) for a descriptor or view count it refuses. */
#define DSL_MAX_AUG 16
#define DSL_FLIP_NONE 0
#define DSL_FLIP_HORIZONTAL 1
#define DSL_FLIP_VERTICAL 2
#define DSL_FLIP_DIAGONAL 3   /* both */
size_t dsl_detect_aug_workspace_bytes(const dsl_det_desc* d, int nviews);

/* One view (replaces FCOSHead.get_bboxes(..., rescale=False, with_nms=False), fcos_head.py:340-548, and this view's turn of
 * merge_aug_bboxes, dense_test_mixins.py:173-200): per level the nms_pre top-k by max_c(sigmoid(cls) * sigmoid(ctr)), the decode
 * and the clip to img_shapes[0] (the view's img_shape), then bbox_mapping_back (core/bbox/transforms.py:46-55) in fp32 in the
 * reference's order - bbox_flip against img_shape (:5-31) for `flip` = DSL_FLIP_*, then the division by scale_factors[0..3] -
 * and the rows stored at view `view` of the pool.  `d` is the view's dsl_fcos_detect descriptor (n == 1; img_shapes and
 * scale_factors are required; workspace as dsl_detect_workspace_bytes(d) says; dets / det_labels / det_count are not used).
 * `pool_desc` is the descriptor the pool was sized with (the one finish takes): a view whose nlvl, nms_pre or num_classes differ
 * from it is refused here, with the view's index in the message, before anything is written. */
int dsl_fcos_detect_collect(const dsl_det_desc* d, const dsl_det_desc* pool_desc, int view, int nviews, int flip, void* pool,
                            size_t pool_bytes, void* stream);

/* After every view 0 .. nviews-1 was collected on the same stream (replaces multiclass_nms(merged_bboxes, merged_scores,
 * score_thr, nms, max_per_img, score_factors), dense_test_mixins.py:88-104, core/post_processing/bbox_nms.py:7-94): pairs with
 * score > score_thr, final score = score * centerness, candidates in (view, level, slot, class) order - when more than 16 384
 * are valid the best 16 384 by final score, as dsl_fcos_detect keeps them per image - sort, class-offset NMS, max_per_img
 * (1..1024, checked here).  finish checks every view's record against its own nlvl / nms_pre / num_classes and consumes it:
 * det_count[0] = -1 (and no detection) says that a view was not collected since the last finish, or with other values - a reused
 * pool cannot pass the previous image's rows on.  In that case only det_count is meaningful: dets is zeroed, det_labels holds
 * whatever the NMS wrote.
 * rescale == 0: the kept boxes are multiplied by view 0's scale factor (:99-104).  Reads d->nlvl, num_classes, nms_pre,
 * max_per_img, score_thr, iou_thr, nms_method, soft_sigma, soft_min_score (Soft-NMS: one pass over the pooled views); writes d->dets [1][max_per_img][5], det_labels, det_count. */
int dsl_fcos_detect_finish(const dsl_det_desc* d, int nviews, int rescale, void* pool, size_t pool_bytes, void* stream);

/* The label-file step of the pseudo-label refresh (runner/hooks/unlabel_pred_hook.py:20-57,84-171 with
 * fuse_history=False) on the detections of dsl_fcos_detect, per image: keep score >= parse_thr, int()-truncate the
 * coordinates, round the score to 6 decimals, then per class 0..num_classes-1 mmcv.ops.nms(iou_thr, score_threshold =
 * nms_thr) on the truncated boxes.  Outputs are ordered class-ascending, score-descending:
 * out_boxes [n][max_per_img][4], out_scores [n][max_per_img], out_labels [n][max_per_img], out_count [n]. */
int dsl_pseudo_label_fuse(const float* dets, const int64_t* labels, const int32_t* count, int n, int max_per_img,
                          int num_classes, float parse_thr, float iou_thr, float nms_thr, float* out_boxes,
                          float* out_scores, int64_t* out_labels, int32_t* out_count, void* stream);

/* The same step with fuse_history=True (unlabel_pred_hook.py:131-141): the image's previous labels - old_boxes
 * [n][max_old][4], old_scores [n][max_old], old_labels [n][max_old] (class indices), old_count [n], taken as the label
 * file held them (no truncation, no parse_thr) - precede the new detections in each class's candidate list.
 * max_per_img + max_old <= 1024; the outputs have max_out >= max_per_img + max_old slots per image.  max_old = 0 (old
 * pointers may be NULL) is dsl_pseudo_label_fuse. */
int dsl_pseudo_label_fuse_history(const float* dets, const int64_t* labels, const int32_t* count, int n, int max_per_img,
                                  const float* old_boxes, const float* old_scores, const int64_t* old_labels,
                                  const int32_t* old_count, int max_old, int num_classes, float parse_thr, float iou_thr,
                                  float nms_thr, float* out_boxes, float* out_scores, int64_t* out_labels,
                                  int32_t* out_count, int max_out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation on the device (dsl_amd/evaluation.py: coco_bbox_eval = the bbox protocol of COCOeval; tpfp_default of
 * mmdet/core/evaluation/mean_ap.py).  The kernels restate the host path's fp64 / fp32 operation order and are compared with it
 * bit for bit; they are compiled with floating-point contraction off.
 *
 * Cells: (category c, image i) -> cell c * num_imgs + i.  Detections are ordered by (category, image, rank within the cell:
 * descending score, ties in array order) and already cut to max_dets per cell: det_boxes [num_det][4] fp32 xyxy.  Ground truth
 * is ordered by (category, image, annotation order): gt_boxes [num_gt][4] fp64 - COCO: x, y, w, h; VOC: x1, y1, x2, y2 holding
 * float32 values, regular boxes before ignore boxes - gt_area [num_gt] fp64, gt_crowd / gt_ignore [num_gt] bytes (VOC reads
 * gt_ignore only).  det_off / gt_off [num_cats * num_imgs + 1] int32 delimit the cells.  iou_thrs [num_thrs] fp64, area_ranges
 * [num_ranges][2] fp64 (lo, hi) are DEVICE arrays too; num_ranges * num_thrs <= 64 (one lane each).
 *
 *   DSL_EVAL_COCO  out_a = matched [num_ranges][num_thrs][num_det] bytes, out_b = ignored (same shape), npos [num_cats][num_ranges]
 *                  int32 (zeroed here) = non-ignored ground truth (not crowd, not gt_ignore, area in [lo, hi]).
 *   DSL_EVAL_VOC   num_ranges == 1 and num_thrs == 1 (else an error): out_a = tp [num_det] bytes, out_b = fp [num_det]; npos is
 *                  not used.  The comparison is (double)max_iou >= iou_thrs[0].
 * A cell with more ground truth than the LDS state holds (128) keeps its matched state in `workspace`
 * (dsl_eval_match_workspace_bytes: 0 when max_gt_per_cell fits); max_gt_per_cell is the largest gt_off difference. */
#define DSL_EVAL_COCO 0
#define DSL_EVAL_VOC 1
#define DSL_EVAL_MAX_THRS 16
#define DSL_EVAL_MAX_RANGES 4
size_t dsl_eval_match_workspace_bytes(int num_gt, int max_gt_per_cell);
int dsl_eval_match(int mode, int num_cats, int num_imgs, int num_det, int num_gt, int max_gt_per_cell, const float* det_boxes,
                   const int32_t* det_off, const double* gt_boxes, const double* gt_area, const uint8_t* gt_crowd,
                   const uint8_t* gt_ignore, const int32_t* gt_off, const double* iou_thrs, int num_thrs, const double* area_ranges,
                   int num_ranges, uint8_t* out_a, uint8_t* out_b, int32_t* npos, void* workspace, size_t workspace_bytes,
                   void* stream);
/* COCO accumulation per (category, range, threshold): `perm` [num_det] lists each category's detections (indices into the
 * detection arrays, category c at det_off[c * num_imgs] .. det_off[(c + 1) * num_imgs]) by descending score, ties by (image,
 * rank).  rec_thrs [num_rec <= 128] fp64 ascending, a device array filled by the host (np.linspace(0, 1, 101)).
 * prec [num_ranges][num_thrs][num_rec][num_cats] fp64: the precision envelope at the first detection whose recall reaches
 * rec_thrs[k], 0 past the last recall, -1 everywhere when npos == 0. */
int dsl_eval_accumulate(int num_cats, int num_imgs, int num_det, int num_ranges, int num_thrs, int num_rec, const uint8_t* matched,
                        const uint8_t* ignored, const int32_t* npos, const int32_t* det_off, const int32_t* perm,
                        const double* rec_thrs, double* prec, void* stream);

/* ------------------------------------------------------------------------------------------
 * Data-parallel exchange (one process per GPU, RCCL over xGMI).  Stands where the reference has
 * MMDistributedDataParallel's gradient buckets (mmdet/apis/train.py:92-96) and reduce_mean
 * (mmdet/core/utils/dist_utils.py:63-69).  librccl.so.1 is bound at the first call (dlopen), not at
 * load time.  `comm` is an rcclComm_t (= ncclComm_t) passed as void*: one made here, or the caller's own.
 *   dsl_comm_unique_id   rank 0 fills 128 bytes (ncclGetUniqueId) and hands them to every rank by its own means
 *   dsl_comm_init_rank   ncclCommInitRank on the calling thread's current device (collective over the ranks)
 *   dsl_comm_size        number of ranks of the communicator
 *   dsl_allreduce_bucket in-place fp32 sum of buf[0..count) over the ranks, queued on `stream`; the 1 / world
 *                        averaging of the gradients is folded into the loss kernel's gradient scale
 *   dsl_allreduce_buckets  n ranges in one RCCL group call (one launch for several small buckets)
 * ---------------------------------------------------------------------------------------- */
int dsl_comm_unique_id(void* id128);
int dsl_comm_init_rank(void** comm, int nranks, const void* id128, int rank);
int dsl_comm_size(void* comm);
int dsl_comm_destroy(void* comm);
int dsl_allreduce_bucket(void* comm, float* buf, size_t count, void* stream);
int dsl_allreduce_buckets(void* comm, float* const* bufs, const size_t* counts, int n, void* stream);
/* The same exchange on a bf16 copy of the bucket (half the bytes over xGMI; north_star allows bf16 gradients on the wire): in-place
 * bf16 sum of buf[0..count).  The caller casts fp32 -> bf16 before (dsl_cast_bf16) and back after (dsl_cast_f32); the master gradient,
 * the clipping norm and the optimizer stay fp32. */
int dsl_allreduce_bucket_bf16(void* comm, void* buf_bf16, size_t count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Op-list executor: run a prebuilt sequence of the ops above with one call (keeps the per-step
 * host cost of ~400 launches out of Python).
 * ---------------------------------------------------------------------------------------- */
enum { DSL_OP_CONV = 1, DSL_OP_WGRAD = 2, DSL_OP_GN_FWD = 3, DSL_OP_GN_BWD = 4, DSL_OP_MAXPOOL = 5,
       DSL_OP_SUM2X2 = 6, DSL_OP_COLSUM = 7, DSL_OP_MEMSET = 8, DSL_OP_PACK_IMAGE = 9,
       DSL_OP_ASSIGN = 10, DSL_OP_LOSS = 11,   /* desc = dsl_fcos_desc -> dsl_head_assign, dsl_head_loss.  MAXPOOL: i[4] = output row stride (0 = c) */
       DSL_OP_GFL_QUALITY = 29,  /* desc = dsl_gfl_desc -> dsl_gfl_quality */
       DSL_OP_PAA_REFINE = 30,   /* desc = dsl_paa_desc -> dsl_paa_pos_loss, then dsl_paa_reassign */
       DSL_OP_FORK = 12,   /* side stream i[0] (default 1) waits for everything queued so far on stream i[1] (default 0 = caller's) */
       DSL_OP_JOIN = 13,   /* stream i[1] (default 0 = caller's) waits for everything queued so far on side stream i[0] (default 1) */
       DSL_OP_WGRAD_GROUP = 14,  /* desc = dsl_wgrad_desc[i[0]] -> dsl_conv2d_wgrad_group */
       DSL_OP_RLA = 17,    /* desc = dsl_rla_desc -> dsl_rla_op */
       DSL_OP_RECORD = 15, /* mark "everything queued so far on stream i[0]" in named event slot i[1] (0..15); survives the call */
       DSL_OP_WAIT = 16,   /* stream i[0] waits for named event slot i[1] (no-op if the slot was never recorded) */
       DSL_OP_PACK_DGRAD = 18, /* dsl_pack_dgrad_batched(p[0] = item table, i[0] = items, i[1] = blocks) */
       DSL_OP_WGRAD_MULTI = 19, /* dsl_conv2d_wgrad_multi(p[0] = table_host, p[1] = table_dev) */
       DSL_OP_QUANT_FP8 = 22,  /* p[2] == NULL: dsl_quant_fp8(p[0] = x, p[1] = y, l[0] = rows, i[0] = c, i[1] = ld_x, scale = the float whose bits are
                                * l[1]); else dsl_absmax(.., p[2] = partials, i[2] = n_partials) + dsl_quant_fp8_dyn(..) */
       DSL_OP_FP8_PREP = 27,   /* dsl_fp8_prep(p[0] = items_dev, i[0] = n_items, i[1] = cout_pad, i[2] = k, margin = the float whose bits are l[1]) */
       DSL_OP_QUANT_FP8_DELAYED = 28, /* dsl_quant_fp8_delayed(p[0] = x, p[1] = y, p[2] = partials, p[3] = scale_dev, l[0] = rows, i[0] = c, i[1] = ld_x,
                                       * i[2] = n_partials) */
       DSL_OP_FP8_COMB = 24,   /* dsl_fp8_comb(p[0] = winv, p[1] = comb, i[0] = n, p[2] = partials, i[2] = n_partials) */
       DSL_OP_QUANT_FP8_W = 23, /* dsl_quant_fp8_weights(p[0] = w, p[1] = w8, p[2] = comb, p[3] = bn_scale, i[0] = cout, i[1] = cout_pad, i[2] = k,
                                * inv_act_scale = the float whose bits are l[1]) */
       DSL_OP_BNECK = 26,      /* desc = dsl_bneck_desc -> dsl_bottleneck_fwd */
       DSL_OP_STEM_POOL = 25,  /* dsl_stem_pool(p[0] = img, p[1] = w_groups, l[0] / l[1] = scale / bias pointers, p[2] = out, i[0] = ld_out,
                                * i[1..3] = n, h, w, i[4] = half_last: dsl_stem_pool_half) */
       DSL_OP_PROF = 21 };     /* phase mark (dsl_prof_enable(3) only, else a no-op): i[0] = class >= 4, i[1] = 0 begin | 1 end, l[0] / l[1] =
                                * algorithmic FLOPs / bytes of the phase as IEEE doubles' bit patterns (begin only) */
typedef struct dsl_op {
  int32_t kind;
  int32_t i[7];            /* small integer arguments for the simple ops; i[6] = s > 0: run this op on the library's
                            * side stream s (1..3; independent work, e.g. weight gradients, overlapping the main chain) */
  const void* desc;        /* pointer to the op's descriptor (host memory, must stay alive) */
  void* p[4];              /* device pointers for the simple ops */
  int64_t l[2];
} dsl_op;
int dsl_run_ops(const dsl_op* ops, int n_ops, void* stream);
/* `stream` waits for named event slot `slot` (a DSL_OP_RECORD of an earlier dsl_run_ops): lets a communication stream
 * start a gradient bucket's all-reduce when the side stream has finished that bucket's weight gradients, whatever the
 * caller's compute stream is doing.  Returns 1 (and does nothing) if the slot was never recorded. */
int dsl_stream_wait_slot(int slot, void* stream);
/* Record named event slot `slot` (0..15) on `stream`: the counterpart of dsl_stream_wait_slot / DSL_OP_WAIT for a stream
 * the caller owns (the optimizer's stream marks "bucket updated"; the next forward list waits for it where it first reads
 * that bucket's weights). */
int dsl_stream_record_slot(int slot, void* stream);
/* The library's side stream `id` (1..3: 1 carries the weight gradients) of the current device as a hipStream_t, for work the
 * caller must queue in order with it (the optimizer step of a bucket whose last weight gradients run there). */
int dsl_side_stream(int id, void** stream_out);
/* Create the library's streams of the current device now and pick them so that the three that carry concurrent work (weight gradients,
 * second chain, frozen prefix) sit on hardware queues of their own, none of them `caller_stream`'s - measured with a 300 us spin kernel,
 * whatever other streams the process has created (api.hip side_init).  Optional (the first dsl_run_ops does it).  *distinct_out: how
 * many of the three were found (3 = all, -1 = option "stream_probe" is 0). */
int dsl_streams_init(void* caller_stream, int* distinct_out);
/* Which hardware queue the communication stream (dsl_side_stream(5)) shares - it is PLACED, not dealt (option "comm_queue", default 1):
 * 1 = the weight-gradient stream's, 2 = the second chain's, 3 = the frozen prefix's, 4 = the caller's; 0 = not placed (probe off or no
 * candidate found), -1 = the streams do not exist yet.  Side ids 2 and 3 are ONE stream (they only add ordering). */
int dsl_comm_stream_queue(void);
/* Device-side stand-in for a ring all-reduce of buf[0, n) (fp32, 16-byte aligned) on `stream`: `wgs` workgroups (RCCL: one per
 * channel) make `passes` value-preserving read-modify-write passes over the bucket - the HBM traffic and the CUs the collective's
 * kernels hold beside the backward pass, on a box with one GPU (bench.py extra.comm_proxy: mmdet/apis/train.py:92-96's DDP
 * all-reduce priced without a peer).  Not a collective: no data leaves the device. */
int dsl_comm_proxy(float* buf, long long n, int wgs, int passes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Live kernel timing with HIP events (bench.py roofline): when enabled, each launch of the MFMA
 * conv kernels is bracketed by a hipEvent pair on the launch stream.  Classes: 0 = conv_pipe_kernel
 * <128,128,2,4,2> (forward + data gradient; the kernel with the largest share of the step), 1 = conv_pipe_kernel
 * <256,192,4,2,2> (the head / FPN tile), 2 = every other forward/dgrad conv kernel instance, 3 = the
 * weight-gradient kernels.
 * dsl_prof_enable(1) brackets only class 0 (cheap enough for a timed region), dsl_prof_enable(2) every class
 * (event pairs on concurrently running streams perturb the overlap).
 * dsl_prof_enable(3) brackets no kernel, only PHASES: DSL_OP_PROF ops in an op list mark begin / end of a stretch of the caller's
 * stream (classes 4.. : 4 = head forward - both towers, their GroupNorms and predictors, on two streams -, 5 = head backward data
 * path); with two streams running the same kernel class side by side, a launch's own duration says little about the rate the
 * phase achieves.
 * dsl_prof_read synchronises the events and returns per class: launches, total ms, algorithmic FLOPs.
 * ---------------------------------------------------------------------------------------- */
#define DSL_PROF_CLASSES 8
int dsl_prof_enable(int on);
int dsl_prof_reset(void);
int dsl_prof_read(int64_t* launches, double* ms, double* flops);
/* the same plus the algorithmic HBM bytes of the bracketed launches (tensors read + written once, real channels) */
int dsl_prof_read2(int64_t* launches, double* ms, double* flops, double* bytes);

/* hardware probes used by the tests */
int dsl_probe_tr16(const uint16_t* lds_image /* 4096 u16 */, const int32_t* lane_off /* 64 u16-offsets */,
                   uint16_t* out /* [64][4] */, void* stream);
/* xcc_of_block[b] = HW_REG_XCC_ID of workgroup b; every workgroup adds 1.0 to acc[xcc][0..255] (8 x 256 floats,
 * zeroed by the caller) with workgroup-scope atomics */
int dsl_probe_xcc(int32_t* xcc_of_block, float* acc, int nblocks, void* stream);
/* Runs nblocks one-per-CU workgroups on a temporary stream created with the given CU mask (NULL: unrestricted) and
 * returns per workgroup out[2b] = XCC id, out[2b+1] = HW_ID register (SE/SH/CU fields); synchronous. */
int dsl_probe_cu_mask(const uint32_t* mask, int nwords, int32_t* out /* [nblocks][2] */, int nblocks);

#ifdef __cplusplus
}
#endif
#endif
