/*
 * cvmi355.h -- C ABI of libcvmi355.so: the MI355X (gfx950) kernels behind CircuitVision's
 * dense-vision hot path (YOLO11 detector + SAM 2.1 forward).
 *
 * The reference (JKc66/CircuitVision) is pure Python: its boundary for this path is Python duck
 * typing (`YOLO(path).predict(img)`, `get_modified_sam2(...)(x)`), and the
 * arithmetic lives in torch / torchvision / ultralytics / sam2 wheels.  The entry points below are
 * what a maintainer binds (ctypes) to replace those wheels' operators.  Each
 * one cites the reference call site whose arithmetic it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - plain C: device pointers + sizes; no torch types.  All device buffers are owned by the
 *     caller; kernels never allocate.  `stream` is a hipStream_t passed as void*.
 *   - every function returns 0 on success, non-zero on error; cvmi_last_error() returns a
 *     thread-local message.  Nothing aborts the process (circuit_analyzer.py:255-263, :381-386
 *     catch ordinary exceptions).
 *   - activations are NHWC ("pixels x channels", channel contiguous); a tensor view is
 *     (ptr, ld) where ld = elements between consecutive pixels, so channel slices of a wider
 *     buffer (zero-copy concat / split) are first-class.
 *   - dtype: CVMI_F16 (fp16 storage, fp32 accumulate), CVMI_F32 (exact-f32 MFMA, parity mode) or -- on the SAM 2 path's entry points
 *     (conv2d, attention, layernorm, cast, maxpool2x2, space_to_depth4, nchw_to_nhwc, prompt_tokens, hyper_masks, sam2_transform,
 *     hiera_mlp, tok_linear) -- CVMI_BF16 (bf16 storage / MFMA operands, fp32 accumulate; BASELINE configs[4]).
 */
#ifndef CVMI355_H
#define CVMI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVMI_VERSION 129

typedef void* cvmi_stream_t; /* hipStream_t */

enum { CVMI_F16 = 0, CVMI_F32 = 1, CVMI_BF16 = 2 };   /* BF16: bf16 storage / operands, fp32 accumulate (SAM 2 path entry points) */
enum { CVMI_ACT_NONE = 0, CVMI_ACT_SILU = 1, CVMI_ACT_RELU = 2, CVMI_ACT_GELU = 3, CVMI_ACT_SIGMOID = 4 };

/* ---- library -------------------------------------------------------------------------------- */
int cvmi_version(void);
const char* cvmi_last_error(void);
/* Diagnostic: the kernel (template instance) the calling thread's most recent cvmi_conv2d / cvmi_attention / cvmi_tok_linear /
 * cvmi_hiera_mlp / cvmi_c3k2 / cvmi_stem2 / cvmi_dwpw / cvmi_layernorm* / cvmi_sppf_pool / cvmi_upsample_refine call dispatched to, as rocprofv3 names it up to the spelling of the 16-bit type (e.g. "gemm256x192_kernel<float>").  Read-and-clear: "" when no such
 * call happened since the last read. */
const char* cvmi_last_kernel(void);
/* fills: [0] CU count, [1] wave size, [2] LDS bytes per CU-workgroup, [3] gfx arch number (950) */
int cvmi_device_info(int device, int* out4);
/* ABI guard for the descriptor structs below: sizeof(struct) as THIS library was compiled, for kind = CVMI_DESC_CONV / _C3K2 / _DWPW /
 * _ATTN / _TOK / _MLP (0 for an unknown kind).  A binding compares it with the size of its own mirror of the struct once, at load, and refuses to
 * continue on a mismatch (circuitvision_amd/_lib.py does; INTEGRATION.md shows the check): a struct that is short by a trailing field
 * would otherwise be read past its end. */
enum { CVMI_DESC_CONV = 0, CVMI_DESC_C3K2 = 1, CVMI_DESC_DWPW = 2, CVMI_DESC_ATTN = 3, CVMI_DESC_TOK = 4, CVMI_DESC_MLP = 5 };
size_t cvmi_desc_size(int kind);

/* ---- HIP graph capture of a launch sequence (replaces per-op Python dispatch) ---------------- */
int cvmi_graph_begin(cvmi_stream_t stream);
int cvmi_graph_end(cvmi_stream_t stream, void** graph_exec_out);
int cvmi_graph_launch(void* graph_exec, cvmi_stream_t stream);
int cvmi_graph_destroy(void* graph_exec);

/* ---- fused convolution / linear layer as implicit GEMM on MFMA -------------------------------
 * y[m, n] = act( sum_k A[m, k] * w[n, k] + bias[n] ) (+ res[m, n])
 * A is gathered on the fly (im2col) from up to two NHWC sources that are concatenated along the
 * channel axis (source 0 first), each optionally nearest-2x upsampled (up = 1).
 * k = (ky*KW + kx)*(c0+c1) + c.  m = (b*OH + oy)*OW + ox.
 * Replaces: ultralytics Conv(+BN folded)+SiLU, Concat, Upsample inside YOLO.predict
 * (circuit_analyzer.py:268); nn.Linear / 1x1 Conv2d of Hiera, FpnNeck, mask decoder inside
 * SAM2ImageWrapper.forward (sam2_infer.py:226-260).
 * w: [Npad][Kpad] (dtype), zero padded, Npad % 128 == 0, Kpad % 32 == 0.  bias: [Npad] f32.
 * c0, c1 must be multiples of 16/sizeof(dtype) unless scalar_gather = 1 (e.g. 3-channel stems).
 */
typedef struct cvmi_conv_desc {
  const void* x0; const void* x1;   /* sources (x1 may be NULL when c1 == 0) */
  const void* w; const float* bias;
  const void* res;                  /* optional residual, added after the activation */
  void* y;
  int x0_ld, x1_ld, res_ld, y_ld;   /* elements between consecutive pixels */
  int c0, c1;                       /* channels taken from each source */
  int up0, up1;                     /* 1: source is at half resolution (nearest 2x upsample) */
  int B, H, W;                      /* logical input size (after upsampling) */
  int OH, OW;
  int KH, KW, stride, pad;
  int N;                            /* output channels */
  int Kpad;                         /* padded K (row length of w) */
  int act;                          /* CVMI_ACT_* */
  int dtype;                        /* CVMI_F16 / CVMI_F32: type of x, w */
  int out_f32;                      /* 1: y and res are f32 even when dtype is F16 */
  int scalar_gather;                /* 1: per-element gather (channel count not vectorizable) */
  int res_mod;                      /* > 0: residual row = m % res_mod (batch-broadcast constants) */
  int act_after_res;                /* 1: y = act(conv + bias + res) instead of act(conv + bias) + res */
  int shuffle_cout;                 /* > 0: ConvTranspose2d(k=2,s=2) as GEMM: N = 4*shuffle_cout, column
                                       n = (dy*2+dx)*shuffle_cout + co is stored at output pixel
                                       (2*oy+dy, 2*ox+dx), channel co of a [B,2*OH,2*OW,*] tensor (y, res) */
  int res_rep;                      /* > 1 (with shuffle_cout, or with res_mod == OH * OW): the residual has B / res_rep images, image b
                                       reads residual image b / res_rep (tensors shared by the prompts of an image) */
  float* row_stats;                 /* optional (f32 output + residual, plain 16-bit GEMM with N % 192 == 0 and K >= 1024, i.e. the Hiera stage-3
                                       fc2 shape): float[rows][N / 96][2] = (mean, sum of squared deviations from that mean) of the values
                                       written to each row's 96-column slices -- the statistics of the NEXT LayerNorm over these rows, free of
                                       the E[x^2] - E[x]^2 cancellation (cvmi_tok_linear with ln_stats_in_parts = N / 96 combines the
                                       slices); NULL = off */
  const int* res_map;               /* optional DEVICE table of B ints (128; needs a residual, res_rep <= 1, and shuffle_cout > 0 or res_mod == OH * OW): batch
                                       entry e reads residual image res_map[e] -- res_rep's sharing with the image of every entry stated instead of
                                       derived as e / res_rep ((image, prompt) pairs with a different number of prompts per image).  The CALLER
                                       guarantees 0 <= res_map[e] < number of residual images: the kernels do not check it.  NULL = off */
} cvmi_conv_desc;
int cvmi_conv2d(const cvmi_conv_desc* d, cvmi_stream_t stream);

/* ---- fused C3k2 block (ultralytics C3k2.forward with c3k = False, n = 1; YOLO11 model.2 / .4 / .16 at scale n):
 *   [a|b] = SiLU(cv1 x) (1x1, c1 -> 2c; only when fuse_cv1, else x IS the [a|b] tensor of 2c channels),
 *   t = SiLU(m.cv1 (*) b) (3x3, c -> h), m = b + SiLU(m.cv2 (*) t) (3x3, h -> c; `shortcut`), y = SiLU(cv2 [a|b|m]) (1x1, 3c -> c2).
 * One launch, intermediates in LDS.  Weights / biases are cvmi_conv2d-packed ([Npad >= 128][kpad], BN folded).
 * cvmi_c3k2_supported() tells which (c1, c, h, c2) configurations are built (fp16 only). */
typedef struct {
  const void* x; void* y;
  const void *w0, *w1, *w2, *w3;
  const float *b0, *b1, *b2, *b3;
  int x_ld, y_ld, kpad0, kpad1, kpad2, kpad3;
  int B, H, W, c1, c, h, c2;
  int fuse_cv1, shortcut, dtype;
} cvmi_c3k2_desc;
int cvmi_c3k2_supported(int c1, int c, int h, int c2, int fuse_cv1, int dtype);
int cvmi_c3k2(const cvmi_c3k2_desc* d, cvmi_stream_t stream);

/* ---- fused YOLO11 stem: model.0 (Conv 3x3 s2, 3 -> c0) + model.1 (Conv 3x3 s2, c0 -> c1), SiLU each -------
 * Replaces the first two layers of ultralytics' DetectionModel inside YOLO.predict (circuit_analyzer.py:268) in one
 * launch: the c0-channel half-resolution map never reaches HBM.  x: the space-to-depth(2) image cvmi_letterbox(s2d=1)
 * writes, [B, H2, W2, x_ld >= 16] (12 real channels); w0 / b0: model.0 as the equivalent 2x2 / stride-1 conv over the
 * 16 s2d channels, taps at block offsets (-1, 0), cvmi_conv2d-packed (k = (ty*2 + tx)*16 + c); w1 / b1: model.1,
 * cvmi_conv2d-packed; y: [B, ceil(H2/2), ceil(W2/2), y_ld >= c1].  fp16, (c0, c1) = (16, 32) (YOLO11-n) is built. */
int cvmi_stem2_supported(int c0, int c1, int dtype);
int cvmi_stem2(const void* x, int x_ld, const void* w0, const float* b0, int kpad0, const void* w1, const float* b1, int kpad1,
               void* y, int y_ld, int B, int H2, int W2, int c0, int c1, int dtype, cvmi_stream_t stream);

/* ---- fused depthwise 3x3 + pointwise 1x1 (+ chained 1x1): YOLO11 Detect class branch ---------
 * Replaces, inside YOLO.predict (circuit_analyzer.py:268), the ultralytics Detect.cv3[i] sub-chains
 *   N2 == 0:  y = SiLU(pw1 * SiLU(dw (*) x))                       [DWConv(C, C, 3), Conv(C, N1, 1)]
 *   N2 >  0:  y = w2 * SiLU(pw1 * SiLU(dw (*) x)) + b2             [... , Conv2d(N1, N2, 1)] (class logits, no activation)
 * in one launch each (intermediates stay in LDS).  wd / bd: cvmi_dwconv3x3 layout ([9][C] tap-major, bias [C]);
 * w1 / b1, w2 / b2: cvmi_conv2d-packed ([Npad >= 128][kpad], zero padded, BN folded).  Only the first N2 (or N1)
 * channels of a y pixel are written.  cvmi_dwpw_supported() tells which (C, N1, N2) are built (fp16 only). */
typedef struct {
  const void* x; void* y;
  const void* wd; const float* bd;
  const void* w1; const float* b1;
  const void* w2; const float* b2;
  int x_ld, y_ld, kpad1, kpad2;
  int B, H, W, C, N1, N2;
  int dtype;
} cvmi_dwpw_desc;
int cvmi_dwpw_supported(int C, int N1, int N2, int dtype);
int cvmi_dwpw(const cvmi_dwpw_desc* d, cvmi_stream_t stream);

/* ---- depthwise 3x3 stride-1 conv + bias + act (YOLO Detect cls branch, C2PSA pe) -------------
 * w: [9][C] (tap-major), bias [C] f32.  Replaces ultralytics DWConv inside YOLO.predict. */
int cvmi_dwconv3x3(const void* x, int x_ld, const void* w, const float* bias, const void* res,
                   int res_ld, void* y, int y_ld, int B, int H, int W, int C, int act, int dtype,
                   cvmi_stream_t stream);

/* ---- SPPF pooling: y1 = mp5(y0), y2 = mp5(y1), y3 = mp5(y2) (k=5,s=1,p=2) in one pass ---------
 * buf is the [B,H,W,ld] concat buffer; channels [0,C) hold y0; writes [C,2C), [2C,3C), [3C,4C). */
int cvmi_sppf_pool(void* buf, int ld, int B, int H, int W, int C, int dtype, cvmi_stream_t stream);

/* ---- scaled-dot-product attention, softmax over keys, one launch for all (batch, head) --------
 * Element (b, h, t, d) of q lives at q + b*q_sb + h*q_sh + t*q_st + d (elements); same for k, v, o.
 * Replaces: ultralytics Attention in C2PSA (YOLO.predict); Hiera MultiScaleAttention and the
 * mask decoder's Attention (sam2_infer.py:226, :252).
 * Window mode (win > 0): tokens of batch entry b are the win x win pixels of window
 *   (b / (gw*gh*...)) of a [img][gh*win][gw*win] grid laid out NHWC with pixel stride *_st;
 *   q_pool = 1 takes q as the 2x2 max-pool of the window's q tokens (Hiera q-pooling). */
typedef struct cvmi_attn_desc {
  const void* q; const void* k; const void* v; void* o;
  long long q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st;
  int B, heads, Nq, Nk, dqk, dv;
  float scale;
  int dtype;
  int win, grid_h, grid_w;   /* window mode (0 = off): window side, image grid size in pixels */
  int q_pool;                /* 1: q window is max-pooled 2x2 (Nq = (win/2)^2) */
  int q_bdiv, kv_bdiv;       /* > 1 (fp16, no window, head dims <= 64): q rows of batch entry b are read from entry b / q_bdiv,
                                k / v rows from entry b / kv_bdiv -- the prompts of one image sharing its image-side tensors
                                (SAM 2 MaskDecoder with repeat_image, first two-way layer); 0 / 1 = off */
  int av_fp8;                /* 1 (16-bit dtype, head_dim 72; BASELINE configs[4] "fp8 MFMA attention"): the softmax(QK^T) V contraction runs on the
                                block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4): P as e4m3 of p * 2^8 (block scale 2^-8), V as e4m3,
                                fp32 accumulation, fp32 softmax statistics.  Honoured by the 256-key window kernel and the long-sequence
                                kernel (Hiera stage-3 windows / global blocks); shapes served by other kernels ignore it.  0 = off (default) */
  int q_log2;                /* 1: q was produced already multiplied by scale * log2(e) (e.g. folded into the rows of the projection that makes it):
                                softmax(q k^T) is then exp2 of the products as they stand and `scale` is ignored.  Same result as 0 with the
                                unscaled q; the long-sequence head_dim-72 kernel uses it to carry the running maximum through the matrix pipe. */
  /* Optional projection source (126).  proj_x != NULL: q, k and v are not read; the launch computes them itself as the rows of
     LayerNorm(proj_x[token]) W^T + b and attends inside the windows, so the qkv tensor is never written (Hiera stage 1:
     `attn(window_partition(qkv(norm1(x))))`, behind sam2_infer.py:226).  Built for a 16-bit dtype, win = 8, head_dim 72, proj_K = 144, an even number
     of windows, and 2 heads (plain) or 4 heads with q_pool (the 144 -> 288 transition); every other combination is refused.  The result is
     bit for bit that of cvmi_tok_linear into a [tokens, 3 * heads * 72] buffer followed by cvmi_attention on it.
     Also built (Hiera stage 2): win = 4, head_dim 72, proj_K = 288, a multiple of 8 windows, 4 heads (plain) or 8 heads with q_pool (the
     288 -> 576 transition), no av_fp8.  Its q, k, v are bit for bit cvmi_tok_linear's; the window attention runs on the matrix pipe with a
     16-bit P, so the result is that of the two launches within the 16-bit window kernels' error bound, not bit for bit. */
  const void* proj_x;        /* f32 [img][grid_h][grid_w] token rows of proj_K values, row stride proj_ld elements */
  const void* proj_w;        /* the qkv weight [3 * heads * 72, proj_K] + bias in cvmi_tok_linear's packed format, rows permuted and zero-padded
                                head by head (circuitvision_amd.engine.PackedQkvAttn states the order) */
  const float* proj_gamma;   /* LayerNorm weight / bias [proj_K] */
  const float* proj_beta;
  const float* proj_stats;   /* optional: (mean, rstd) per token as cvmi_tok_linear / cvmi_hiera_mlp write them to ln_stats_out; NULL = computed here */
  int proj_ld, proj_K;
  float proj_eps;
  /* Batch sharing by table (128): DEVICE arrays of B ints; q rows of batch entry b are read from entry q_bmap[b], k / v rows from entry
     kv_bmap[b] -- what q_bdiv / kv_bdiv derive as b / divisor, stated per entry.  Each excludes its divisor being > 1 and carries the
     divisors' restrictions (16-bit dtype, no window, head dims <= 64, no proj_x).  The CALLER guarantees that every value indexes an
     existing batch entry of the shared tensor: the kernels do not check it.  NULL = off */
  const int* q_bmap;
  const int* kv_bmap;
} cvmi_attn_desc;
int cvmi_attention(const cvmi_attn_desc* d, cvmi_stream_t stream);

/* ---- YOLO Detect decode: DFL expectation + dist2bbox + stride scale + class sigmoid -----------
 * box[l]: [B,Hl,Wl,64] (ld box_ld), cls[l]: [B,Hl,Wl,>=roundup(nc,16B)] (ld cls_ld) for l = 0..2.
 * pred: f32 [B, 4+nc, A], A = sum Hl*Wl (ultralytics layout: xywh rows, then class-score rows).
 * best_score f32 [B*A] / best_cls i32 [B*A] (optional, both or neither): per-anchor best class
 * (first maximum) for cvmi_yolo_nms_best.  write_cls = 0 skips the class-score rows of pred. */
int cvmi_detect_decode(const void* const* box, const int* box_ld, const void* const* cls,
                       const int* cls_ld, const int* hs, const int* ws, const float* strides,
                       int nlevels, int B, int nc, int dtype, float* pred, float* best_score,
                       int* best_cls, int write_cls, cvmi_stream_t stream);

/* ---- ultralytics-semantics NMS on the decoded predictions -------------------------------------
 * pred f32 [B, 4+nc, A].  Candidates: max class score > conf_thres; sorted by score desc (ties:
 * lower anchor index first); only the first NMS_MAX_NMS = 30000 of them go on (ultralytics' max_nms);
 * per-class via +cls*max_wh; greedy suppress IoU > iou_thres; first max_det kept (max_det <= 4096).
 * out_det f32 [B, max_det, 6] (x1,y1,x2,y2,conf,cls), out_idx i32 [B, max_det]
 * (anchor index), out_count i32 [B].  workspace: >= cvmi_yolo_nms_workspace(B, A) bytes.
 * Replaces ultralytics ops.non_max_suppression + torchvision.ops.nms (circuit_analyzer.py:268). */
size_t cvmi_yolo_nms_workspace(int B, int A);
int cvmi_yolo_nms(const float* pred, int B, int nc, int A, float conf_thres, float iou_thres,
                  int max_det, float max_wh, float* out_det, int* out_idx, int* out_count,
                  void* workspace, cvmi_stream_t stream);
/* same, with the per-anchor best class supplied by cvmi_detect_decode (only the 4 box rows of pred are read) */
int cvmi_yolo_nms_best(const float* pred, const float* best_score, const int* best_cls, int B, int nc,
                       int A, float conf_thres, float iou_thres, int max_det, float max_wh,
                       float* out_det, int* out_idx, int* out_count, void* workspace,
                       cvmi_stream_t stream);

/* ---- letterbox pre-processing (ultralytics LetterBox + BGR flip + /255) -----------------------
 * src u8 [H,W,3] -> one letterboxed image at dst: the resized region new_w x new_h is placed at
 * (left, top) of an out_h x out_w canvas, pad value 114; 8-bit fixed-point bilinear as OpenCV.
 * s2d = 0: dst is NHWC [out_h, out_w, 3].  s2d = 1: dst is space-to-depth(2) [out_h/2, out_w/2, 16],
 * channel ((y&1)*2 + (x&1))*3 + c, channels 12..15 zero -- the layout the YOLO stem conv reads. */
int cvmi_letterbox(const uint8_t* src, int H, int W, void* dst, int out_h, int out_w, int new_h,
                   int new_w, int top, int left, int dtype, int s2d, cvmi_stream_t stream);
/* The same for B equally sized sources in ONE launch: src u8 [B,H,W,3] contiguous (e.g. one pinned staging buffer copied by one
 * hipMemcpyAsync), image b written at dst + b * dst_image_stride elements (the detector's batched `predict([img, ...])`). */
int cvmi_letterbox_batch(const uint8_t* src, int B, int H, int W, void* dst, long long dst_image_stride, int out_h, int out_w,
                         int new_h, int new_w, int top, int left, int dtype, int s2d, cvmi_stream_t stream);
/* The same for B sources of DIFFERENT sizes onto ONE out_h x out_w canvas shape (a mixed list handed to `predict`: ultralytics letterboxes
 * such a list with auto = False, every image to the full imgsz x imgsz square, and runs it as one batch).  All sources live in one u8 device
 * buffer of src_bytes bytes (one pinned staging buffer, one H2D copy); image b is the H x W x 3 image at src + rows[b].src_byte_offset -- ANY
 * byte offset, the taps are read byte by byte -- resized to new_w x new_h at (left, top) of canvas b, written at dst + b * dst_image_stride
 * elements.  rows is a HOST array, read during the call; it travels in the kernel arguments, 64 images per launch.  Every row is checked as
 * cvmi_letterbox_batch checks its one geometry, and against src_bytes, BEFORE the first launch; cvmi_last_error names the failing row.
 * s2d = 1 writes 16-byte stores: dst and dst_image_stride * sizeof(element) must be 16-byte aligned.
 * Bit-identical to cvmi_letterbox on the same image and geometry (one coefficient function for both kernels). */
typedef struct cvmi_letterbox_row {
  long long src_byte_offset;
  int H, W, new_h, new_w, top, left;
} cvmi_letterbox_row;
int cvmi_letterbox_ragged(const uint8_t* src, long long src_bytes, const cvmi_letterbox_row* rows, int B, void* dst,
                          long long dst_image_stride, int out_h, int out_w, int dtype, int s2d, cvmi_stream_t stream);

/* ---- dtype conversion / layout helpers -------------------------------------------------------- */
/* NCHW (f32 or f16) -> NHWC dtype */
int cvmi_nchw_to_nhwc(const void* src, int src_dtype, void* dst, int dst_dtype, int dst_ld, int B,
                      int C, int H, int W, cvmi_stream_t stream);
/* NHWC dtype -> NCHW f32 */
int cvmi_nhwc_to_nchw_f32(const void* src, int src_dtype, int src_ld, float* dst, int B, int C,
                          int H, int W, cvmi_stream_t stream);

/* ==== SAM 2.1 path (sam2_infer.py:220-275 and the un-vendored sam2 package behind it) ========= */

/* LayerNorm over the channel axis of rows x C (nn.LayerNorm in Hiera / TwoWayTransformer, LayerNorm2d
 * in the mask decoder's upscaling); optional activation after the affine.  x / y dtypes independent
 * (fp16 mode keeps the residual stream in f32 and feeds fp16 to the GEMMs). gamma, beta: f32 [C]. */
/* pad_w > 0: the rows are the pixels of [*, pad_h, pad_w] images and are written into a zero-padded
 * [*, pad_hp, pad_wp] grid (Hiera pads the NORMALISED tokens up to a window multiple; padding stays 0). */
int cvmi_layernorm(const void* x, int x_ld, int x_dtype, const float* gamma, const float* beta,
                   void* y, int y_ld, int y_dtype, long long rows, int C, float eps, int act,
                   int pad_h, int pad_w, int pad_hp, int pad_wp, cvmi_stream_t stream);
/* Same over an f32 stream, writing the f32 result to y AND a 16-bit (y2_dtype) copy to y2 (the GEMM-operand copy the next layer
 * reads: saves a cast pass over the stream; SAM 2 two-way transformer norm4, sam2_infer.py:252). */
int cvmi_layernorm_dual(const void* x, int x_ld, const float* gamma, const float* beta, void* y, int y_ld, void* y2, int y2_ld,
                        int y2_dtype /* CVMI_F16 | CVMI_BF16 */, long long rows, int C, float eps, cvmi_stream_t stream);

/* Fused MLP half of a Hiera block, in place on the f32 residual stream (sam2 hieradet MultiScaleBlock: `x = x + mlp(norm2(x))`,
 * behind sam2_infer.py:226):   x[r, :] += fc2( GELU( fc1( LayerNorm(x[r, :]; gamma, beta, eps) ) ) )   for r < rows, hidden = 4 C,
 * fp16 operands / fp32 accumulation; the normalised copy and the hidden activation never reach HBM.  C in {144, 288} are built
 * (cvmi_hiera_mlp_supported); stages with wider rows keep the separate LayerNorm + two cvmi_conv2d launches.
 * w_packed: both weight matrices in MFMA-fragment order, hidden chunk by hidden chunk (32 hidden units each), every fragment 64 lanes
 * x 8 fp16 = 1 KiB (lane l: r = l & 31, h = l >> 5):
 *   chunk j = [ F1(j, s) for s = 0 .. C/16 ]  ++  [ F2(j, t, s2) for t = 0 .. ceil(C/32) - 1, s2 = 0, 1 ]
 *   F1(j, s)[l][e]     = W1x[32 j + r][16 s + 8 h + e],  W1x = [ fc1.weight | fp16(b1) | fp16(b1 - fp16(b1)) | 0 ... ] (C + 16 columns:
 *                        the fc1 bias rides on two constant-1 input columns as a hi + lo fp16 pair)
 *   F2(j, t, s2)[l][e] = fc2.weight[32 t + r][32 j + 16 s2 + 8 (e >> 2) + 4 h + (e & 3)]   (0 for output rows >= C): the k order in
 *                        which a 32x32 MFMA accumulator, converted in place, serves as the next MFMA's B operand.
 * cvmi_hiera_mlp_packed_bytes(C) = (4 C / 32) * (C/16 + 1 + 2 ceil(C/32)) * 1024.  b2: fc2 bias, f32 [C]. */
int cvmi_hiera_mlp_supported(int C);
size_t cvmi_hiera_mlp_packed_bytes(int C);
/* proj form (127; ao / bp set): the block's attention projection in the same launch.  With x1 = x + ao . Wp^T + bp the launch stores
 * x1 + fc2(GELU(fc1(LayerNorm(x1)))) + b2; x1 itself is never written (sam2 hieradet MultiScaleBlock: `x = shortcut + proj(attn)` then the
 * MLP half).  ao = bp = NULL: the launch described above, bit for bit.  Built for C in {144, 288} and a 16-bit dtype; refused before any
 * launch: another C or dtype, a NULL or not 16-byte aligned ao / w_packed / bp, ao_ld < C or no multiple of 8.  Equal to cvmi_tok_linear(residual)
 * followed by the plain form to within f32 rounding ahead of the same 16-bit roundings (the f32 sums associate as x + (ao . Wp^T + (bp + b2) + ..),
 * fc1 sums its k in the permuted order below), not bit for bit; a repeated launch on the same input is bit-identical.
 * w_packed of the proj form, cvmi_hiera_mlp_proj_packed_bytes(C) = ceil(C/32) * (C/16) * 1024 + cvmi_hiera_mlp_packed_bytes(C) bytes:
 *   [ P(t, s) for t = 0 .. ceil(C/32) - 1, s = 0 .. C/16 - 1 ]  ++  the chunks of the plain form with F1's k permuted
 *   P(t, s)[l][e]  = Wp[32 t + r][16 s + 8 h + e]   (attn.proj.weight; 0 for output rows >= C); the kernel moves ring-slot sized runs of whole
 *                    tiles: floor((C/16 + 1 + 2 ceil(C/32)) / (C/16)) = 2 tiles per piece
 *   F1(j, s)[l][e] = W1[32 j + r][16 s + pi(8 h + e)] for s < C/16,  pi(k) = 8 ((k & 7) >> 2) + 4 (k >> 3) + (k & 3)  (bits 2 and 3 of k
 *                    swapped): the k order in which the accumulator of the proj product (lane = token, register 4 g + e of tile t <-> channel
 *                    32 t + 8 g + 4 h + e), normalised in place, serves as fc1's B operand.  The bias step s = C/16 and F2 are unchanged. */
size_t cvmi_hiera_mlp_proj_packed_bytes(int C);
typedef struct cvmi_mlp_desc {
  void* x;                   /* the f32 residual stream [rows][C], row stride x_ld elements; updated in place */
  const float* gamma;        /* LayerNorm weight / bias, f32 [C] */
  const float* beta;
  const void* w_packed;      /* the stream the selected form reads: the plain form's chunks, or (ao / bp set) the proj form's stream above */
  const float* b2;           /* fc2 bias, f32 [C] */
  float* ln_stats_out;       /* optional: float[2 * rows], per updated row (mean, 1 / sqrt(var + ln_stats_eps)) -- the statistics of the NEXT
                                LayerNorm over these rows (the next block's norm1), consumed through cvmi_tok_desc.ln_stats_in; NULL = off */
  const void* ao;            /* proj form: attention output, 16-bit [rows][C], row stride ao_ld elements; read only.  NULL (with bp) = plain form */
  const float* bp;           /* proj form: attn.proj.bias, f32 [C] */
  long long rows;
  int x_ld;
  int C;
  int dtype;                 /* CVMI_F16 | CVMI_BF16: type of w_packed (and of ao) */
  int ao_ld;
  float eps;                 /* of the LayerNorm inside the launch */
  float ln_stats_eps;        /* of the statistics written to ln_stats_out */
} cvmi_mlp_desc;
int cvmi_hiera_mlp(const cvmi_mlp_desc* d, cvmi_stream_t stream);

/* Token-stationary linear layer for Hiera's short-K GEMMs (sam2 hieradet MultiScaleBlock: qkv(norm1(x)), x = shortcut + proj(attn),
 * mlp.layers[0](norm2(x)) + GELU; behind sam2_infer.py:226):
 *   y[r, n] = act( sum_k in[r, k] * W[n, k] + b[n] ),   r < rows (a multiple of 256), n < N, K in {144, 288, 576}
 * w_packed: ceil(N/32) chunks of (K/16 + 1) MFMA fragments of 1 KiB, fragment (j, s), lane l (r = l & 31, h = l >> 5), element e:
 *   Wx[32 j + r][16 s + 8 h + e],  Wx = [ W | fp16(b) | fp16(b - fp16(b)) | 0 ... ]  (K + 16 columns, rows >= N zero).
 * The chunk count is padded to even (the added chunk is zero): cvmi_tok_linear_packed_bytes(K, N) = 2 ceil(ceil(N/32) / 2) * (K/16 + 1) * 1024
 * for this format; the 16x16x32 format below is not padded: ceil(N/32) * (K/16 + 1) * 1024. */
int cvmi_tok_linear_supported(int K);
size_t cvmi_tok_linear_packed_bytes(int K, int N);
/* Packed-weight format the library expects for this K: 32 = the layout above (32x32x16 MFMA fragments, bias on an extra k-step);
 * 16 (K = 576) = fragments of the 16x16x32 MFMA shape: ceil(N/32) chunks of 2 K/32 + 1 pieces of 1 KiB, piece (j, 2 s + hh), lane l
 * (r16 = l & 15, g = l >> 4), element e:  W[32 j + 16 hh + r16][32 s + 8 g + e]  (rows >= N zero);  the chunk's last piece holds its 32 bias
 * values as f32 in its first 128 bytes (rest zero).  cvmi_tok_linear_packed_bytes follows the format. */
int cvmi_tok_linear_format(int K);
/* The layout of ln_stats_out for a residual-form launch of this shape.  0: float[rows][2] of (mean, rstd).  P > 0: the launch has
 * fewer 256-row blocks than the chip has CUs (the per-rank batch of an 8-GPU job: SAM 2.1-L at 8 images), so P workgroups share a row block,
 * each writing its output-channel slice, and ln_stats_out is float[rows][P][2] of per-slice (mean, sum of squared deviations) -- exactly what
 * the consumer takes with ln_stats_in_parts = P.  Depends on (rows, K, N) only; K = 576 (the 16x16x32 format) is the only K that splits.
 * The caller states the layout it allocated in cvmi_tok_desc.ln_stats_out_parts; a launch that would write another one is refused.
 * Requirements of that format beyond the ones above: 16-bit output needs N % 8 == 0 and out_ld % 8 == 0; in_f32_layernorm = 2 is not built. */
int cvmi_tok_linear_stats_parts(long long rows, int K, int N);
typedef struct cvmi_tok_desc {
  const void* in;            /* [rows][K], row stride in_ld elements; its type is chosen by in_f32_layernorm */
  const float* gamma;        /* LayerNorm weight / bias, f32 [K] (in_f32_layernorm = 1) */
  const float* beta;
  const void* w_packed;
  void* out;                 /* [rows][N] (pool form: [rows / 4][N]), row stride out_ld elements; its type is chosen by out_f32_residual */
  const float* ln_stats_in;  /* optional (in_f32_layernorm = 1): float[2 * rows] of per row (mean, rstd) handed over by the launch that wrote the
                                f32 residual stream (sam2 hieradet MultiScaleBlock: x = shortcut + proj(attn), then mlp.layers[0](norm2(x)));
                                the LayerNorm prologue then reads every row once instead of twice.  NULL = computed here */
  float* ln_stats_out;       /* optional (out_f32_residual = 1): per row (mean, 1 / sqrt(var + ln_stats_eps)) over the N updated values, in the
                                layout ln_stats_out_parts states.  NULL = off */
  long long rows;            /* a multiple of 256 */
  int in_ld;
  int in_f32_layernorm;      /* 1: in is the f32 residual stream, normalised on the fly with gamma / beta / eps (the separate LayerNorm pass
                                and its fp16 copy disappear); 0: in is an fp16 matrix; 2: in is an f32 matrix converted as it is (K = 144, 288;
                                16-bit output, no activation: the neck's lateral convs read the f32 stage outputs, FpnNeck behind sam2_infer.py:226) */
  int out_ld;
  int out_f32_residual;      /* 1: out is the f32 residual stream, updated in place (out[r, n] += y[r, n], act must be NONE); 0: out is fp16
                                (act NONE or GELU).  With in_f32_layernorm = 1 on a launch that shares row blocks (K = 576, fewer than 256 of
                                them) in and out must not overlap: sibling workgroups would read rows the others update; refused */
  int K;
  int N;
  int act;                   /* CVMI_ACT_NONE | CVMI_ACT_GELU */
  int dtype;                 /* CVMI_F16 | CVMI_BF16: type of w_packed and of the 16-bit input / output */
  int ln_stats_in_parts;     /* P > 0: ln_stats_in is float[rows][P][2] of per-slice (mean, sum of squared deviations) instead, P equal column
                                slices of the row (cvmi_conv_desc.row_stats, or a ln_stats_out with ln_stats_out_parts = P) */
  int ln_stats_out_parts;    /* the P the caller allocated ln_stats_out for: 0 = float[rows][2]; P > 0 = float[rows][P][2].  Must equal
                                cvmi_tok_linear_stats_parts(rows, K, N) when ln_stats_out is set: refused otherwise, before any launch */
  int pool_h;                /* pool_h, pool_w > 0 select the pool form, the shortcut path of a Hiera q-pooling block in ONE launch: the rows are the */
  int pool_w;                /* tokens of [rows / (pool_h pool_w)][pool_h][pool_w] grids and out[b, y, x, :] = max over the 2 x 2 token block of
                                ( LayerNorm(in[b, 2y + dy, 2x + dx, :]) W^T + bias ) = `do_pool(self.proj(norm1(x)))` of sam2 hieradet
                                MultiScaleBlock.forward (behind /root/reference/src/sam2_infer.py:226); out is f32 [rows / 4][N], written not
                                added.  pool_h, pool_w even; in_f32_layernorm = 1, out_f32_residual = 0, act NONE, no ln_stats_out, pairs
                                (ln_stats_in_parts = 0) as ln_stats_in.  0, 0 = off */
  float eps;                 /* of the LayerNorm prologue */
  float ln_stats_eps;        /* of the statistics written to ln_stats_out */
} cvmi_tok_desc;
int cvmi_tok_linear(const cvmi_tok_desc* d, cvmi_stream_t stream);

/* 2x2 / stride 2 max-pool, NHWC (Hiera shortcut path of the q-pooling blocks: do_pool(proj(x))). */
int cvmi_maxpool2x2(const void* x, int x_ld, void* y, int y_ld, int B, int H, int W, int C, int dtype,
                    cvmi_stream_t stream);

/* Space-to-depth(4) of a 3-channel NHWC image: [B,H,W,3] -> [B,H/4,W/4,48], channel (sy*4 + sx)*3 + c.  With it Hiera's
 * PatchEmbed (Conv2d 3 -> E, 7x7, stride 4, pad 3; sam2 hieradet.py) is a 2x2 / stride-1 conv over 48 channels
 * (block taps -1, 0), i.e. a vectorised cvmi_conv2d instead of a per-element gather. */
int cvmi_space_to_depth4(const void* x, void* y, int B, int H, int W, int dtype, cvmi_stream_t stream);

/* rows x C copy with dtype conversion (f32 <-> f16). */
int cvmi_cast(const void* x, int x_ld, int x_dtype, void* y, int y_ld, int y_dtype, long long rows, int C,
              cvmi_stream_t stream);

/* Prompt tokens of the SAM 2 mask decoder for n prompts of K labelled points each (upstream PromptEncoder
 * `_embed_points` + MaskDecoder token concat; box = corners labelled 2 / 3 + one padding point labelled -1):
 *   tokens[i, 0:T0]   = out_tokens (obj-score, iou, 4 mask tokens)
 *   tokens[i, T0 + j] = label -1 ? table[0] : [sin, cos](2*pi * ((2*(coords[i,j] + 0.5)/image_size - 1) @ gauss)) + table[1 + label]
 * coords f32 [n,K,2] (x, y in input pixels), labels i32 [n,K] in {-1,0,1,2,3}, gauss f32 [2,128],
 * out_tokens f32 [T0,256], table f32 [5,256] (not_a_point, point_embeddings 0..3).
 * Writes tokens_f32 [n, T0+K, 256] and (optional) the same values in `dtype` to tokens_lp. */
int cvmi_prompt_tokens(const float* coords, const int* labels, const float* gauss, const float* out_tokens,
                       const float* table, float image_size, float* tokens_f32, void* tokens_lp, int dtype,
                       int n, int K, int T0, cvmi_stream_t stream);

/* dst[b*rep + r] = src[b] for r < rep: image-major broadcast of per-image tensors to the prompts of each image
 * (upstream MaskDecoder repeat_image=True).  bytes_per_image must be a multiple of 16. */
int cvmi_repeat_images(const void* src, void* dst, long long bytes_per_image, int B, int rep, cvmi_stream_t stream);

/* dst[n] = src[pair_image[n]] for n < n_pairs: per-image tensors gathered to (image, prompt) pairs whose images a DEVICE table names -- cvmi_repeat_images
 * for pairs with a different number of prompts per image, in any order.  bytes_per_image must be a multiple of 16, src / dst 16-byte aligned,
 * n_pairs <= 65535.  dst_lp (optional, 8-byte aligned; src is then f32): the same values rounded once (nearest even) to lp_dtype = CVMI_F16 or
 * CVMI_BF16, same shape -- in a 16-bit plan the first cvmi_cast of the gathered tensor; NULL: lp_dtype is ignored.
 * The CALLER guarantees 0 <= pair_image[n] < number of images in src: the kernel reads the table as it is (the host side of
 * circuitvision_amd checks every value before it uploads the table). */
int cvmi_gather_images(const void* src, void* dst, void* dst_lp, int lp_dtype, long long bytes_per_image, const int* pair_image, int n_pairs,
                       cvmi_stream_t stream);

/* Mask decoder tail: masks[b,i,p] = sum_c hyper[b,i,c] * up[b,p,c] for the 4 mask tokens (c = 32),
 * plus the stability counters of token 0 (area over +delta / -delta) for
 * dynamic_multimask_via_stability.  hyper f32 [B,4,hyper_ld], up dtype [B,P,up_ld], masks f32 [B,4,P],
 * areas i32 [B,2] (zeroed by this call). */
int cvmi_hyper_masks(const float* hyper, int hyper_ld, const void* up, int up_ld, int up_dtype, int C,
                     float* masks, int* areas, int B, int P, float delta, cvmi_stream_t stream);
/* Select per image: token 0 when dynamic == 0 or stability >= thresh, else 1 + argmax(iou[1:4]).
 * iou f32 [B, iou_ld] (4 values used).  Writes low_res f32 [B,P], iou_out f32 [B], sel i32 [B]. */
int cvmi_select_mask(const float* masks, const int* areas, const float* iou, int iou_ld, int dynamic,
                     float thresh, float* low_res, float* iou_out, int* sel, int B, int P,
                     cvmi_stream_t stream);

/* The multimask tail (upstream MaskDecoder.forward with multimask_output=True): tokens 1..3 of masks f32 [n,4,P] and of iou f32 [n, iou_ld]
 * (4 values used) as contiguous low_res3 f32 [n,3,P] and iou3 f32 [n,3], in token order; no stability fallback.  A plain copy: candidate k
 * is bit-identical to what cvmi_select_mask writes when it selects token 1 + k. */
int cvmi_multimask_out(const float* masks, const float* iou, int iou_ld, float* low_res3, float* iou3, int n, int P,
                       cvmi_stream_t stream);

/* Mask feedback between two decoder passes (upstream's recipe for ambiguous prompts: multimask_output=True, then the best candidate's logits as
 * mask_input of a single-mask pass on the same prompts): mask_out[i] = low_res[i, argmax(iou[i, :])] for the n pairs, in one launch.
 *   low_res  f32 [n, NM, P] and iou f32 [n, NM], NM = 1 or 3 (what a single-mask / multimask plan leaves in low_res / iou)
 *   mask_out f32 [n, P] (the next plan's mask_in);  sel_out i32 [n] the selected candidate, or NULL
 * The selection is torch.argmax's: the lowest index among equal maxima, and a NaN counts as greater than every number (the first NaN wins).
 * NM = 1 always selects candidate 0: the call is a copy.  Only the selected plane is read: n * P * 4 bytes in, as many out, 16 bytes per access.
 * P must be a multiple of 4, low_res / iou / mask_out 16-byte aligned (sel_out 4-byte), n <= 65535; n == 0 returns 0 without a launch. */
int cvmi_best_candidate(const float* low_res, const float* iou, int NM, float* mask_out, int* sel_out, int n, int P, cvmi_stream_t stream);

/* The mask-to-mask pass of upstream's SAM2AutomaticMaskGenerator (use_m2m: refine_with_m2m): EVERY candidate of a decoder pass becomes one
 * prompt of a second, single-mask pass -- its own low-res logits, clamped as SAM2ImagePredictor._predict returns them, as the mask prompt and
 * the prompt it came from beside them.  One launch prepares the second plan's inputs from the first plan's outputs for the n real pairs:
 *   low_res  f32 [n, NM, P], NM = 1 or 3 (what a single-mask / multimask plan leaves in low_res)
 *   mask_out f32 [n*NM, P]:        mask_out[i*NM + k] = clamp(low_res[i, k], -clamp, clamp) -- candidate-major inside the pair, so the planes
 *                                  are one contiguous array in the order of low_res
 *   coords f32 [n, K, 2], labels i32 [n, K], pair_image i32 [n] (or NULL) -> coords_out f32 [n*NM, K, 2], labels_out i32 [n*NM, K],
 *   pair_image_out i32 [n*NM] (NULL exactly when pair_image is: the uniform prompts=P plans): row i written NM times, at rows i*NM .. i*NM+NM-1
 * The clamp is torch.clamp's bit for bit: a NaN stays a NaN, -0.0 stays -0.0, +-inf become +-clamp (upstream's bound is 32; clamp >= 0).
 * P must be a multiple of 4 (at most 2^28), low_res / mask_out 16-byte aligned (16-byte accesses; the tables 4-byte), K in 1 .. 65536,
 * n <= 65535 (the pair is the grid's second dimension); n == 0 returns 0 without a launch.  No atomics: the result does not depend on the
 * launch.  n * NM * P * 4 bytes in, as many out. */
int cvmi_m2m_fanout(const float* low_res, int NM, float clamp, float* mask_out, const float* coords, const int* labels, const int* pair_image,
                    float* coords_out, int* labels_out, int* pair_image_out, int n, int P, int K, cvmi_stream_t stream);

/* Mask prompts (upstream PromptEncoder._embed_masks + SAM2ImagePredictor._predict with mask_input): the decoder's image stream of the
 * B * rep (image, prompt) pairs, image-major (pair i belongs to image i / rep), in one launch --
 *   keys[i] = emb[i / rep] + mask_downscaling(mask[i]) - no_mask_embed
 * with mask_downscaling = Conv2d(1,4,k=2,s=2) -> LayerNorm2d(4) -> GELU -> Conv2d(4,16,k=2,s=2) -> LayerNorm2d(16) -> GELU -> Conv2d(16,256,k=1)
 * (LayerNorm2d: per pixel over the channels, biased variance, eps 1e-6; GELU: the exact erf form), all in f32.
 *   mask    f32 [B*rep, 4*fs, 4*fs] logits (the size of low_res)
 *   emb     f32 [B, fs*fs, 256]: the embed GEMM's output, whose bias already holds no_mem_embed + no_mask_embed
 *   params  f32 [CVMI_MASK_PROMPT_PARAMS], packed in this order: w1[4][2][2] b1[4] g1[4] be1[4]  w2[16][4][2][2] b2[16] g2[16] be2[16]
 *           w3[256][16]  b3'[256] with b3' = b3 - no_mask_embed (g / be: the LayerNorm2d weight / bias)
 *   keys    f32 [B*rep, fs*fs, 256]
 *   keys_lp optional: the same values rounded once (nearest even) to lp_dtype = CVMI_F16 or CVMI_BF16, same shape; NULL: lp_dtype is ignored
 * All pointers 16-byte aligned (keys_lp 8-byte); B, rep, fs > 0; B * rep * fs * fs < 2^31.  fs * fs need not be a multiple of anything.
 * No atomics: the result does not depend on the launch.  Replaces cvmi_repeat_images and, in a 16-bit plan, the first cvmi_cast of keys. */
#define CVMI_MASK_PROMPT_PARAMS 4684
int cvmi_mask_prompt_embed(const float* mask, const float* emb, const float* params, float* keys, void* keys_lp, int lp_dtype,
                           int B, int rep, int fs, cvmi_stream_t stream);

/* cvmi_mask_prompt_embed for n_pairs pairs whose images a DEVICE table names (same kernel, the image index read instead of derived):
 *   keys[i] = emb[pair_image[i]] + mask_downscaling(mask[i]) - no_mask_embed,   mask f32 [n_pairs, 4*fs, 4*fs], keys f32 [n_pairs, fs*fs, 256].
 * The CALLER guarantees 0 <= pair_image[i] < number of images in emb.  Everything else as above. */
int cvmi_mask_prompt_embed_pairs(const float* mask, const float* emb, const float* params, float* keys, void* keys_lp, int lp_dtype, int n_pairs,
                                 const int* pair_image, int fs, cvmi_stream_t stream);

/* F.interpolate(bilinear, align_corners=False) of f32 planes [N,h,w] -> [N,H,W] (sam2_infer.py:263-268,
 * postprocess_masks :127).  mask_u8 (optional): also writes (value > thresh) ? 255 : 0.
 * This call, cvmi_mask_postprocess, cvmi_mask_postprocess_sizes and cvmi_mask_postprocess_rects_dev are one kernel body with the roundings of
 * the sampled value written out (csrc/bilinear.hpp: bil_mix): the four forms resample a plane to the same bits, so a mask is (map > thresh)
 * of the map this call writes, pixel for pixel, whichever of them produced it. */
int cvmi_bilinear_f32(const float* x, int N, int h, int w, float* y, int H, int W, uint8_t* mask_u8,
                      float thresh, cvmi_stream_t stream);   /* y may be NULL when mask_u8 is given */

/* The reference's whole mask post-processing in one pass (circuit_analyzer.py:354-370): postprocess_masks' bilinear resize
 * (sam2_infer.py:127) -> `> thresh` -> u8 {0, 255} (:356-357) -> bounding rectangle of the non-zero pixels (:364-370,
 * cv2.findContours + boundingRect), WITHOUT materialising the f32 [N,H,W] map: only the u8 mask and four ints per plane
 * are written.  extent[n] = {min x, min y, max x, max y} or {W, H, -1, -1} for an empty mask. */
int cvmi_mask_postprocess(const float* x, int N, int h, int w, int H, int W, float thresh, uint8_t* mask_u8,
                          int* extent, cvmi_stream_t stream);
/* The same for planes that return to DIFFERENT sizes (each image's own crop window): sizes is a HOST array of N x {H_n, W_n}; plane n is
 * written at mask_u8 + sum over m < n of H_m * W_m (planes packed back to back); extent[n] as above in plane n's own coordinates. */
int cvmi_mask_postprocess_sizes(const float* x, int N, int h, int w, const int* sizes, float thresh, uint8_t* mask_u8, int* extent,
                                cvmi_stream_t stream);
/* The same with the sizes on the DEVICE: plane n is resized to the {w, h} of rects_dev[n] = {x0, y0, w, h} (a window of cvmi_stage2_crop) and
 * written at mask_u8 + n * plane_stride BYTES -- fixed stride, the caller allocates plane_stride = H0 * W0 of the uncropped image, so no
 * offset depends on a window; a plane is clipped to its stride.  The grid is sized for plane_stride pixels.  extent[n] as above. */
int cvmi_mask_postprocess_rects_dev(const float* x, int N, int h, int w, const int* rects_dev, long long plane_stride, float thresh,
                                    uint8_t* mask_u8, int* extent, cvmi_stream_t stream);

/* ---- automatic mask generation (upstream SAM2AutomaticMaskGenerator at its defaults: one crop, multimask, no mask-to-mask pass): what
 * follows the decoder for the candidate planes of a chunk of grid points, without the f32 map at the image's size.
 *
 * cvmi_amg_score: M planes low f32 [M,h,w] are resized to H x W exactly as cvmi_bilinear_f32 resizes them -- the same taps, weights and
 * scale factors (float)h / (float)H, (float)w / (float)W, the same f32 value v per pixel (csrc/bilinear.hpp) -- and only counted:
 *   stats i32 [M,8] = {n_hi, n_lo, area, x0, y0, x1, y1, 0}: n_hi = #(v > hi), n_lo = #(v > lo), area = #(v > mid), and the inclusive
 *   {min x, min y, max x, max y} of v > mid, {0, 0, 0, 0} for an empty mask (upstream's batched_mask_to_box).
 * The caller passes the levels as f32 (upstream: mid = mask_threshold, lo / hi = mid -+ stability_score_offset, computed in double and rounded
 * once); lo <= mid <= hi is not required.  stats is defined by this call alone (three launches: initialise, score, close the empty boxes) and
 * needs no preparation; all reductions are integer sums and extrema, so the result does not depend on the launch.
 * mask_u8 (optional) u8 [M,H,W]: the same kernel also writes (v > mid) ? 255 : 0; stats is identical with and without it, so the area and
 * box agree with the written mask by construction.
 * A workgroup stages the source rows and columns of a band of output rows in LDS; the call refuses (before any launch) an M above 65535,
 * a plane of 2^31 pixels or more, and a resize whose single output row needs more than 12288 staged floats (w > 6144 of a down-scale beyond
 * 6x in x). */
int cvmi_amg_score(const float* low, int M, int h, int w, int H, int W, float lo, float mid, float hi, int* stats, uint8_t* mask_u8,
                   cvmi_stream_t stream);

/* cvmi_amg_select: ONE image's filter and ordered append of a chunk's candidates, in one launch.
 *   stats i32 [n,8] (cvmi_amg_score), iou f32 [n] (the decoder's predicted IoUs) and low f32 [n,P] for the chunk's n candidate planes in
 *   candidate order (point-major: plane i belongs to point point_base + i / ncand, candidate token i % ncand; ncand = 3 multimask, else 1);
 *   only the first n_valid <= n take part (the rest are the pairs a short last chunk was padded with: never selected, whatever they score).
 * Keep rule: iou > iou_thresh and stability >= stab_thresh with stability = (float)n_hi / (float)n_lo in f32 (0 / 0 = NaN fails, as in torch).
 * Every kept candidate is appended, in candidate order (a prefix sum over the keep flags, not a slot grab), at the image's running count:
 *   counter i32 [2] (DEVICE) = {candidates kept so far, 0}: the caller zeroes both once per image; every call adds its kept count to counter[0]
 *   (counter[1] is the call's own ticket and is 0 again afterwards).  The count goes on past cap; nothing is written at or past slot cap.
 *   records [cap]: cvmi_amg_record of slot s;  pool f32 [cap,P]: its low plane;
 *   nms_block f32 [5,cap]: column s = (cx, cy, w, h, score) of the inclusive box as floats -- the layout cvmi_yolo_nms reads with nc = 1,
 *   A = cap; cx - w / 2 gives the integer corner back exactly.  The caller fills row 4 (score) with -inf once per image, so that the
 *   unused columns never pass its conf_thres; this call does not touch them.
 * P a multiple of 4; low and pool 16-byte aligned.  n_valid == 0 returns 0 without a launch. */
typedef struct cvmi_amg_record {
  float score, stability;      /* predicted IoU, stability score */
  int area, x0, y0, x1, y1;    /* stats[2..6] */
  int point, token;            /* grid point index, candidate token */
  int reserved;                /* 0 */
} cvmi_amg_record;
int cvmi_amg_select(const int* stats, const float* iou, const float* low, int n, int n_valid, int ncand, int point_base, float iou_thresh,
                    float stab_thresh, int P, int cap, int* counter, cvmi_amg_record* records, float* pool, float* nms_block,
                    cvmi_stream_t stream);

/* Crop layers (upstream's crop_n_layers > 0): the planes of a call belong to ONE crop of the image, the rectangle [cx0, cx1) x [cy0, cy1) of
 * a W x H image, and stats / records / nms_block are in the crop's own coordinates (the IoU of the per-crop NMS is translation-invariant and
 * the integers are exact in f32; the caller adds the offsets).
 *
 * cvmi_amg_select_crop: cvmi_amg_select -- the same kernel -- whose keep rule also holds upstream's ~is_box_near_crop_edge, in integers.
 * With b = (x0 + cx0, y0 + cy0, x1 + cx0, y1 + cy0) from the stats (the inclusive maxima and the empty mask's {0, 0, 0, 0} taken as they
 * are), crop = (cx0, cy0, cx1, cy1) and orig = (0, 0, W, H), a candidate is dropped iff for some side k
 *   |b_k - crop_k| <= edge_tol  and not  |b_k - orig_k| <= edge_tol        (upstream: edge_tol = 20; a distance of exactly edge_tol drops).
 * The filter enters both the "kept before me" prefix and the total: slots stay dense and in candidate order.  cvmi_amg_select is this call
 * with crop = image, for which the filter is identically false.  Refused: an empty crop, one that leaves the image, W or H of 2^24 or more. */
int cvmi_amg_select_crop(const int* stats, const float* iou, const float* low, int n, int n_valid, int ncand, int point_base, float iou_thresh,
                         float stab_thresh, int P, int cap, int* counter, cvmi_amg_record* records, float* pool, float* nms_block, int cx0,
                         int cy0, int cx1, int cy1, int W, int H, int edge_tol, cvmi_stream_t stream);

/* cvmi_amg_score_window: cvmi_amg_score's mask mode for a crop of size (H, W) whose masks belong in full-image planes: mask_u8 is
 * u8 [M,PH,PW] and the H x W mask sits at (wx0, wy0) in each plane.  stats are cvmi_amg_score's for the same planes (crop coordinates);
 * inside the window the bytes are the ones its mask mode writes, outside they are 0, and EVERY byte of every plane is written by this one
 * call (no memset before it, no crop-sized temporary, no copy).  The same kernel: its units tile the plane, so a thread stores aligned
 * words of it (PW % 4 == 0, aligned base; bytes otherwise) wherever the window starts; only units that meet the window stage and sample.
 * Window = plane is cvmi_amg_score bit for bit.  Refused before any launch: a null mask_u8, a window that leaves the plane, a plane of 2^31
 * pixels or more, and what cvmi_amg_score refuses. */
int cvmi_amg_score_window(const float* low, int M, int h, int w, int H, int W, float lo, float mid, float hi, int* stats, uint8_t* mask_u8,
                          int PH, int PW, int wx0, int wy0, cvmi_stream_t stream);

/* Hole and sprinkle removal of postprocess_masks (sam2_infer.py:88-128) and the labelling under it, on f32 planes x [N,h,w] with a
 * threshold t.  Foreground is x > t, background x <= t; components are 8-connected in BOTH phases and never cross a plane; h and w need
 * not be even.  The label of a pixel is 1 + (y * w + x) of the raster-first pixel of its component, its area the component's pixel count.
 * workspace: DEVICE, at least cvmi_mask_cc_workspace(N, h, w) bytes (0: the sizes are not positive or N * h * w >= 2^31, which the two
 * calls refuse before they launch anything).  CVMI_MASK_CC_TILE: the edge of the tiles that are labelled in LDS.
 *   cvmi_mask_components: labels / areas i32 [N,h,w], for the pixels of both phases.
 *   cvmi_mask_fill_small: y [N,h,w] (must not overlap x) = t + 10 where x is background, max_hole_area > 0 and area <= max_hole_area;
 *   t - 10 where x is foreground, max_sprinkle_area > 0 and area <= max_sprinkle_area; x elsewhere.  Both tests are made on x, the two
 *   constants are f32 sums, and the limits are floats compared with <= (2.5 fills areas 1 and 2). */
#define CVMI_MASK_CC_TILE 64
size_t cvmi_mask_cc_workspace(int N, int h, int w);
int cvmi_mask_components(const float* x, int N, int h, int w, float thresh, int* labels, int* areas, void* workspace,
                         cvmi_stream_t stream);
int cvmi_mask_fill_small(const float* x, int N, int h, int w, float thresh, float max_hole_area, float max_sprinkle_area, float* y,
                         void* workspace, cvmi_stream_t stream);

/* upstream's remove_small_regions (sam2/utils/amg.py) on N binary u8 planes mask [N,H,W], IN PLACE; foreground is a non-zero byte, components
 * are 8-connected in both phases and never cross a plane (the same tile / seam / flatten kernels, reading bytes).  phases: 1 holes, 2 islands,
 * 3 both, in upstream's order:
 *   holes    every background component of area < min_area (strict; the plane-wide background is a component like any other) is written as 255;
 *   islands  on the RESULT of the holes phase, labelled again (a filled hole can join foreground components): every foreground component of
 *            area < min_area is written as 0 -- but where EVERY foreground component of the plane is that small, the largest one stays, the
 *            one whose raster-first pixel comes first among equals ([UP]: cv2's label order).
 * Bytes that are neither filled nor removed keep their value (a foreground 1 stays 1).
 * info i32 [N,8] = {changed (0 / 1: a pixel of the plane was filled or removed), area and inclusive x0, y0, x1, y1 of the FINAL plane
 * ({0,0,0,0} for an empty one: batched_mask_to_box), pixels filled, pixels removed}.  All reductions are integer sums and extrema, the kept
 * component a 64-bit maximum of (area << 32 | ~root index): results do not depend on the launch.
 * workspace: DEVICE, 8-byte aligned, at least cvmi_mask_remove_small_workspace(N, H, W) bytes = two ints per pixel + 8 per plane (0: sizes
 * not positive or N * H * W >= 2^31).  Refused before any launch: such sizes, min_area <= 0, phases outside 1..3, null pointers. */
size_t cvmi_mask_remove_small_workspace(int N, int H, int W);
int cvmi_mask_remove_small(uint8_t* mask, int N, int H, int W, int min_area, int phases, int* info, void* workspace, cvmi_stream_t stream);

/* upstream's mask_to_rle_pytorch `counts` of N binary u8 planes mask [N,H,W] (row-major; foreground is a non-zero byte): plane n is read in
 * COLUMN-major order (y fastest); its runs alternate, starting with a run of zeros (0 when pixel (0, 0) is set); a run goes on across a
 * column end; the runs sum to H * W (an all-zero plane is {H * W}, an all-set one {0, H * W}).
 *   offsets i32 [N+1]: offsets[n] = index of plane n's first run in counts, offsets[N] = the total.  Always written in full.
 *   counts i32 [cap_runs]: nothing is written at or past counts[cap_runs]; when offsets[N] > cap_runs the caller repeats the call with a
 *   larger capacity (cvmi_external_contours' convention).  cap_runs = 0 with counts = NULL is a pure count.
 * Every position comes from a prefix sum, never a slot grab: replays are bit-identical.  The mask bytes are read once.
 * workspace: DEVICE, 8-byte aligned, workspace_bytes >= cvmi_mask_rle_workspace(N, H, W) (1 bit per pixel rounded up to 64 rows per column,
 * + 8 bytes per 256 such words; 0: sizes not positive, or N * H * W + N >= 2^31 -- positions and the total are int32 and a plane has up to
 * H * W + 1 runs).  Refused before any launch: such sizes, null pointers (counts only with cap_runs > 0), a workspace that is too small. */
size_t cvmi_mask_rle_workspace(int N, int H, int W);
int cvmi_mask_rle(const uint8_t* mask, int N, int H, int W, int cap_runs, int* offsets, int* counts, void* workspace, size_t workspace_bytes,
                  cvmi_stream_t stream);

/* Extent of N binary u8 planes [N,H,W]: extent[n] = {min x, min y, max x, max y} over the non-zero pixels, or
 * {W, H, -1, -1} for an empty plane.  Replaces cv2.findContours(RETR_EXTERNAL) + cv2.boundingRect on the SAM 2 mask
 * (circuit_analyzer.py:364-370): sam_extent_bbox = (min x, min y, max x + 1, max y + 1). */
int cvmi_mask_extent(const uint8_t* mask, int N, int H, int W, int* extent, cvmi_stream_t stream);

/* Fused 'bilinear upsample to HxW' + MultiKernelRefinement (sam2_infer.py:130-189, :263-272):
 * nk parallel convs (1 -> ic channels, odd kernels ks[], zero 'same' padding) + exact GELU + 1x1
 * combiner.  The ic*nk x H x W intermediate never leaves LDS/registers.
 * params f32: for each branch j: w[ic][ks_j][ks_j] then b[ic]; then combiner w[nk*ic], b[1]. */
int cvmi_upsample_refine(const float* low, int N, int h, int w, float* high, int H, int W,
                         const float* params, const int* ks, int nk, int ic, cvmi_stream_t stream);

/* SAM2Transforms.__call__ (sam2_infer.py:49-51): u8 HWC -> /255 -> antialiased bilinear resize to
 * R x R -> ImageNet normalise; written NHWC with 3 channels in dst_dtype. */
int cvmi_sam2_transform(const uint8_t* src, int H, int W, void* dst, int R, int dst_dtype,
                        cvmi_stream_t stream);
/* The same for B equally sized sources in ONE launch (SAM2Transforms.forward_batch, sam2_infer.py:53-56): src u8 [B,H,W,3] contiguous,
 * dst [B,R,R,3].  swap_rb = 1 reads the source channels reversed: circuit_analyzer.py:343 applies cv2.COLOR_BGR2RGB to the image it
 * is handed, which on the device is an index, not a pass over the image. */
int cvmi_sam2_transform_batch(const uint8_t* src, int B, int H, int W, void* dst, int R, int dst_dtype, int swap_rb,
                              cvmi_stream_t stream);
/* The same on a WINDOW of each source image: the crop the reference takes between the detector and the segmenter
 * (CircuitAnalyzer.crop_image_and_adjust_bboxes, circuit_analyzer.py:937-1284, called with padding = 80 at analysis_pipeline.py:177; the
 * cropped image is what segment_with_sam2 :206 then resizes), WITHOUT a cropped copy: image b is the window rects[b] = {x0, y0, w, h} of the
 * u8 [H, W, 3] image at src + b * src_image_stride BYTES (0: every window comes from one image), and exactly the pixels of the window take
 * part in the antialiased resize -- bit-identical to cvmi_sam2_transform on a contiguous copy of the window (every form of the transform is
 * one kernel body that is handed its window; the equal-size batch hands it the whole image).  rects is a HOST array
 * (B x 4 ints, read during the call; it travels in the kernel arguments).  The source may be the buffer the detector's letterbox read. */
int cvmi_sam2_transform_rects(const uint8_t* src, long long src_image_stride, int H, int W, const int* rects, int B, void* dst, int R,
                              int dst_dtype, int swap_rb, cvmi_stream_t stream);
/* cvmi_sam2_transform_rects with rects as a DEVICE array (B x {x0, y0, w, h}, e.g. cvmi_stage2_crop's `window`), read by the kernel: nothing
 * of the call depends on a value the host has not seen.  The host checks the tap bound for the whole H x W image, which bounds every window
 * inside it; the kernel clips a window to the image (cvmi_stage2_crop guarantees 0 <= x0, x0 + w <= W, w, h >= 1 -- and the same in y).
 * Bit-identical to cvmi_sam2_transform_rects on the same windows. */
int cvmi_sam2_transform_rects_dev(const uint8_t* src, long long src_image_stride, int H, int W, const int* rects_dev, int B, void* dst, int R,
                                  int dst_dtype, int swap_rb, cvmi_stream_t stream);
/* cvmi_sam2_transform_rects for sources of DIFFERENT sizes in one packed u8 device buffer of src_bytes bytes (the block the ragged letterbox
 * read): image b is the window {x0, y0, w, h} of the H x W x 3 image at src + rows[b].src_byte_offset (any byte offset).  rows is a HOST
 * array in the kernel arguments, 64 images per launch; every row -- the image inside the buffer, the window inside the image, the tap bound
 * of the window -- is checked before the first launch.  dst_dtype F16, BF16 or F32.  Bit-identical to cvmi_sam2_transform_rects on each
 * image alone. */
typedef struct cvmi_sam2_src_row {
  long long src_byte_offset;
  int H, W;
  int x0, y0, w, h;
} cvmi_sam2_src_row;
int cvmi_sam2_transform_srcs(const uint8_t* src, long long src_bytes, const cvmi_sam2_src_row* rows, int B, void* dst, int R, int dst_dtype,
                             int swap_rb, cvmi_stream_t stream);

/* ---- the glue between the detector and the segmenter, on the device (analysis_pipeline.py:97-115 -> :177): ultralytics' scale_boxes + clip
 * in f32 (subtract the pad, DIVIDE by the gain, clamp), results_to_bboxes' np.rint of the f64 copy, the stage-2 NMS of utils.py:346-361
 * (stable descending confidence, a box survives iff its f64 IoU with every kept box is < stage2_iou; stage2_iou < 0: no pass, list order),
 * CircuitAnalyzer.crop_image_and_adjust_bboxes' window decision (circuit_analyzer.py:937-1284, f64) and its box shift -- one launch, one
 * workgroup per image.  det f32 [B, max_det, 6] {x1, y1, x2, y2, conf, cls} in letterboxed coordinates and count i32 [B] are the detector
 * plan's own outputs; H0, W0 the original image; gain, pad_x, pad_y as detector.scale_boxes computes them; class_flags DEVICE u8 [n_flags]
 * by class id: CVMI_GLUE_CLASS_* bits.  max_det <= CVMI_GLUE_MAX_DET.  Outputs (DEVICE, fixed stride; rows past a count are not written):
 *   kept_idx i32 [B, max_det]: index into the detector's list, in kept order;  kept_count i32 [B];
 *   boxes i32 [B, max_det, 4]: every detector box rounded, in original pixels (detector order);
 *   adj_boxes i32 [B, max_det, 4]: the kept boxes in the window's coordinates, clipped to it (kept order);
 *   window i32 [B, 4] {x0, y0, w, h}: the crop window, the whole image when no crop applies (0 <= x0, x0 + w <= W0, w >= 1; same in y);
 *   info i32 [B, CVMI_GLUE_INFO_HEAD + max_det]: the words named below (what crop_debug_info reports), then one word per KEPT box:
 *   CVMI_GLUE_BOX_EXPANDED = this text box grew the window, CVMI_GLUE_BOX_DROPPED = no positive area left inside the window. */
#define CVMI_GLUE_MAX_DET 320
#define CVMI_GLUE_INFO_HEAD 40
#define CVMI_GLUE_CLASS_NOT_CLUSTERED 1   /* text, explanatory, circuit, vss, crossover (:982) */
#define CVMI_GLUE_CLASS_JUNCTION 2
#define CVMI_GLUE_CLASS_TEXT 4
#define CVMI_GLUE_CLASS_NON_COMPONENT 8   /* circuit_analyzer.py:51 */
#define CVMI_GLUE_BOX_EXPANDED 1
#define CVMI_GLUE_BOX_DROPPED 2
enum {
  CVMI_GLUE_REASON = 0,         /* reason_for_no_crop: CVMI_GLUE_REASON_* */
  CVMI_GLUE_DECISION = 1,       /* crop_decision_source: CVMI_GLUE_DECISION_* */
  CVMI_GLUE_APPLIED = 2,
  CVMI_GLUE_LINK = 3,           /* clustering_proximity_threshold, -1 = None */
  CVMI_GLUE_CLUSTERS = 4,       /* num_clusters_found, -1 = None */
  CVMI_GLUE_MAIN_SIZE = 5,      /* main cluster: elements, text associations, ordinal, first member (position in the kept list, -1 = none) */
  CVMI_GLUE_MAIN_TEXT = 6,
  CVMI_GLUE_MAIN_ID = 7,
  CVMI_GLUE_MAIN_FIRST = 8,
  CVMI_GLUE_TOTAL = 9,          /* boxes the crop saw, component-type boxes, text boxes */
  CVMI_GLUE_COMPONENT_TYPE = 10,
  CVMI_GLUE_TEXT_TYPE = 11,
  CVMI_GLUE_PADDING = 12,
  CVMI_GLUE_BASIS_SET = 13,     /* 1: words BASIS .. BASIS + 7 hold crop_basis_bbox_before_padding as four f64 (low word first) */
  CVMI_GLUE_PADDED_SET = 14,    /* 1: words PADDED .. + 3 hold window_after_main_padding */
  CVMI_GLUE_FINAL_SET = 15,     /* 1: words FINAL .. + 3 hold final_crop_window_abs {x0, y0, x1, y1} */
  CVMI_GLUE_BASIS = 16,
  CVMI_GLUE_PADDED = 24,
  CVMI_GLUE_FINAL = 28          /* 32 .. 39: reserved, zero */
};
enum { CVMI_GLUE_REASON_NONE = 0, CVMI_GLUE_REASON_NO_ELEMENTS = 1, CVMI_GLUE_REASON_TOO_LARGE = 2, CVMI_GLUE_REASON_INVALID = 3 };
enum { CVMI_GLUE_DECISION_UNKNOWN = 0, CVMI_GLUE_DECISION_NO_ELEMENTS = 1, CVMI_GLUE_DECISION_SCORED = 2, CVMI_GLUE_DECISION_FALLBACK = 3 };
int cvmi_stage2_crop(const float* det, const int* count, int B, int max_det, int H0, int W0, float gain, int pad_x, int pad_y,
                     double stage2_iou, int padding, const uint8_t* class_flags, int n_flags, int* kept_idx, int* kept_count, int* boxes,
                     int* adj_boxes, int* window, int* info, cvmi_stream_t stream);

/* ---- node analysis (CircuitAnalyzer.get_node_connections, circuit_analyzer.py:1286-1370): N u8 planes of different sizes, packed back to
 * back (plane n at sum over m < n of its predecessors' pixels), sizes in HOST arrays read during the call. */

/* Mask preparation (:1327-1345 + resize_image_keep_aspect :787-809): src -> emptied (the boxes zeroed) -> resized (cv2.resize INTER_LINEAR,
 * 8-bit fixed point, the letterbox's coefficient tables).  sizes: HOST N x {H, W, new_h, new_w}; resized is packed by {new_h, new_w}.
 * boxes: DEVICE i32 [box_start[N], 4] {xmin, ymin, xmax, ymax} = int() of the reference's values, only the boxes it empties (classes
 * other than crossover / junction / circuit / vss); plane n owns boxes [box_start[n], box_start[n + 1]) (HOST, N + 1 ints). */
int cvmi_node_prepare(const uint8_t* src, int N, const int* sizes, const int* boxes, const int* box_start, uint8_t* emptied,
                      uint8_t* resized, cvmi_stream_t stream);

/* enhance_lines (:289-311) fused: cv2.GaussianBlur((5,5), 1) (bit-exact 8-bit path, BORDER_REFLECT_101) -> cv2.dilate(ones(3,3), 2) ->
 * cv2.erode(ones(3,3), 2) (5 x 5 max / min, border replicated).  sizes: HOST N x {H, W}; dst packed like src (no aliasing).
 * sums: DEVICE u64 [N], each plane's exact pixel sum of dst (get_contours' cv2.mean(img)[0] > 127 is sum > 127 * H * W). */
int cvmi_enhance_lines(const uint8_t* src, int N, const int* sizes, uint8_t* dst, unsigned long long* sums, cvmi_stream_t stream);

/* get_contours' cv2.findContours(img, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) (:388-405) on N packed u8 planes (sizes: HOST N x {H, W}).
 * Foreground = non-zero, or != 255 where sums (DEVICE u64 [N], from cvmi_enhance_lines; NULL = never) says the plane inverts (:398).
 * binarize = 1 writes the reference's img[img == 255] = 1 (:401) into planes that do not invert.  workspace: DEVICE, at least
 * cvmi_contours_workspace(N, sizes) bytes.  Outputs (DEVICE):
 *   counts i32 [N + 3]: contours per plane, then the total contours, the total points, the longest traced border (steps);
 *   per contour c < min(total, cap_contours), plane by plane, each plane's contours in REVERSE raster order of their start pixels (cv2's
 *   list order): info i32 [cap_contours, 8] {plane, npts, first point, x, y, w, h, steps} (x .. h = cv2.boundingRect of the points) and
 *   area2 i64 [cap_contours] = twice the signed shoelace area of the points; points i32 [cap_points, 2] (x, y), plane-relative.
 * Nothing is truncated silently: when the totals exceed the capacities, the outputs past them are not written and the caller repeats
 * the call with capacities of at least the totals. */
size_t cvmi_contours_workspace(int N, const int* sizes);
int cvmi_external_contours(uint8_t* planes, const unsigned long long* sums, int N, const int* sizes, int binarize, void* workspace,
                           size_t workspace_bytes, int cap_contours, int cap_points, int* counts, int* info, long long* area2,
                           int* points, cvmi_stream_t stream);

/* The contour x component-box loop of get_node_connections (:1380-1446) and the contour moments of its ground choice, on the outputs of
 * cvmi_external_contours while they are on the device.  info i32 [C, 8] / points i32 [P, 2]: as cvmi_external_contours wrote them (C, P =
 * its totals).  boxes: DEVICE i32 [box_start[N], 5] {xmin, ymin, xmax, ymax, threshold}: resize_bboxes' ints (:461-477) of the boxes the loop
 * visits (class not in non_components, :51), threshold = 20 / 8 / 6 by class (:1407-1415), chosen by the host.  box_start: HOST N + 1 ints,
 * plane n owns boxes [box_start[n], box_start[n + 1]); pair_start: HOST C + 1 ints, contour c owns first[pair_start[c] .. pair_start[c + 1]),
 * one slot per box of its plane.  workspace: DEVICE, at least cvmi_node_connect_workspace(N, C) bytes.  Outputs (DEVICE):
 *   first i32 [pair_start[C]]: the index within the contour of the FIRST point, in contour order, that passes is_point_near_bbox (:811-846:
 *   inside the closed box, or within threshold of one of its four edge LINES), -1 when there is none or when the broad phase skips the pair
 *   (:1399-1401: the box against the contour's rectangle {x, y, x + w, y + h}, without threshold);
 *   moments i64 [C, 3] {a00, a10, a01}: cv::contourMoments' sums over the closed polygon, dxy = x_prev y - x y_prev, a00 += dxy,
 *   a10 += dxy (x_prev + x), a01 += dxy (y_prev + y), exact in int64 (equal to OpenCV's double accumulators while they stay below 2^53).
 * One workgroup per 1024 points of a contour; the host arrays are read during the call. */
size_t cvmi_node_connect_workspace(int N, int C);
int cvmi_node_connect(const int* info, const int* points, int C, int P, const int* boxes, int N, const int* box_start, const int* pair_start,
                      void* workspace, size_t workspace_bytes, int* first, long long* moments, cvmi_stream_t stream);

/* ---- terminal reclassification (CircuitAnalyzer.reclassify_terminals_based_on_connectivity, circuit_analyzer.py:2217-2311), the step
 * between the segmenter and node analysis (run_terminal_reclassification, analysis_pipeline.py:117-137). */

/* segment_circuit (:313-319) and the box emptying (:2244-2249) on N windows of u8 [., ., 3] images in ONE buffer, in one launch per 32
 * planes: cv2.cvtColor(RGB2GRAY) = (R 9798 + G 19235 + B 3735 + 16384) >> 15 with R read from channel red_channel (0 or 2) and B from
 * 2 - red_channel; cv2.adaptiveThreshold(255, ADAPTIVE_THRESH_MEAN_C, THRESH_BINARY_INV, 31, 21): mean = the normalised 31 x 31 box filter,
 * u8, rounded half to even (no ties: 961 is odd), border REPLICATED AT THE WINDOW's edge (no pixel outside the window is read);
 * dst = 255 where grey - mean <= -21, else 0; then 0 inside every rectangle of the plane.
 *   src: DEVICE, src_bytes long (every window is checked against it).  planes: HOST i64 [N, 4] {byte offset of the window's first pixel, row
 *   pitch in BYTES (>= 3 W, any alignment), H, W}, H W < 2^31.  rects: DEVICE i32 [box_start[N], 4] {x0, y0, x1, y1}, half-open, in window
 *   pixels (the host resolves the reference's numpy slices, negative stops included, and drops the empty ones); plane n owns rectangles
 *   [box_start[n], box_start[n + 1]) (HOST, N + 1 ints).  The host arrays are read during the call.
 *   dst: DEVICE u8, the N planes packed back to back (plane n at the sum of its predecessors' H W), must not overlap src.
 *   sums: DEVICE u64 [N], zeroed by this call, each plane's exact pixel sum of dst (what cvmi_external_contours' inversion test reads). */
int cvmi_segment_circuit(const uint8_t* src, size_t src_bytes, int N, const long long* planes, int red_channel, const int* rects,
                         const int* box_start, uint8_t* dst, unsigned long long* sums, cvmi_stream_t stream);

/* The contour x terminal-box loop of :2272-2286 on the outputs of cvmi_external_contours: cvmi_node_connect WITHOUT its broad phase (every
 * contour is tested against every box of its plane, so a contour far from a box but within threshold of one of its edge lines counts) and
 * without the moments.  Arguments and layout as cvmi_node_connect: boxes DEVICE i32 [box_start[N], 5] {xmin, ymin, xmax, ymax, threshold}
 * (the reference's threshold here is 10), box_start / pair_start HOST, workspace DEVICE of at least cvmi_contour_hits_workspace(N, C)
 * bytes.  Output first i32 [pair_start[C]] (DEVICE, written entirely by this call): the index of the first point of the contour that passes
 * is_point_near_bbox, or -1.  Nothing is launched when there is no contour or no pair. */
size_t cvmi_contour_hits_workspace(int N, int C);
int cvmi_contour_hits(const int* info, const int* points, int C, int P, const int* boxes, int N, const int* box_start, const int* pair_start,
                      void* workspace, size_t workspace_bytes, int* first, cvmi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CVMI355_H */
