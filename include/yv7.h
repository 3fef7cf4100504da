/* yv7.h — C ABI of the MI355X-native YOLOv7 inference path (libyv7.so, gfx950).
 *
 * Plain C types only: every tensor crosses the boundary as a device pointer plus sizes; streams
 * cross as hipStream_t passed as void*.  Every call returns 0 on success, a positive hipError_t
 * on a HIP failure, or a negative yv7_status on an argument / shape error; the message is in the
 * thread-local yv7_last_error().  Nothing throws or aborts across the ABI.  The caller owns every
 * input, output and workspace buffer; a plan owns only its packed weights and small tables.
 *
 * What each entry point replaces in the reference (qbxlvnf11/yolo-series):
 *   yv7_plan_create   attempt_load() -> Model.fuse() product   models/experimental.py:247-270,
 *                     models/yolo.py:693-710 (the fused, deploy-form network: weights folded on the
 *                     host by the Python mirror, packed NHWC/KRSC and handed over here once)
 *   yv7_forward       Model.forward / forward_once            models/yolo.py:581-631, including every
 *                     layer forward (Conv.fuseforward common.py:110-111, RepConv common.py:498-500,
 *                     SPPCSPC common.py:276-280, MP/SP common.py:30-45, ReOrg common.py:48-53,
 *                     Concat common.py:56-62, Shortcut common.py:80-86, DownC common.py:181-192, nn.Upsample)
 *                     and Detect/IDetect decode yolo.py:42-63,140-160
 *   yv7_nms           non_max_suppression()                   utils/general.py:628-720 incl. the
 *                     torchvision.ops.nms call at general.py:704
 *   yv7_end2end       TRT EfficientNMS_TRT plugin contract    models/experimental.py:111-156,
 *                     utils/add_nms.py:94-138 (fixed-shape num_dets/boxes/scores/classes)
 *   yv7_letterbox     letterbox() + the detect.py input         utils/datasets.py:1277-1307,
 *                     conversion                                detect.py:100-104, datasets.py:199
 *   yv7_letterbox_ragged  the same for frames of different    models/common.py:899-918 (autoShape's
 *                     sizes on one canvas                       letterbox loop, np.stack, transpose, / 255)
 *   yv7_letterbox_c, yv7_letterbox_ragged_c  both for frames of 1..16 channels (no counterpart: the
 *                     original's loaders are 3-channel)
 *   yv7_scale_boxes   scale_coords() + clip_coords(),           utils/general.py:340-361, detect.py:183,
 *                     .round(), the Detections views            models/common.py:940-948
 *   yv7_match         the per-image, per-class matching of      test.py:123,131,179-213
 *                     predictions to labels for mAP
 *   yv7_confusion     ConfusionMatrix.process_batch over a      utils/metrics.py:121-159 as called from
 *                     batch, into a matrix kept on the device   test.py:137-140,181-189
 *   yv7_coco_match    pycocotools' COCOeval.evaluateImg (bbox)  test.py:256-278: ev.evaluate() of the
 *                     over a batch, on the JSON rows' values    third-party library the reference calls
 *   yv7_draw_boxes    plot_one_box() over a batch               utils/plots.py:57-68, detect.py:204-238
 *   yv7_mosaic        plot_images(): the picture grid of a      utils/plots.py:114-190 as called from
 *                     batch with its labels or predictions      test.py:215-220
 */
#ifndef YV7_H
#define YV7_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YV7_ABI_VERSION 5

/* Activation tensors in the forward workspace are NHWC with a YV7_BORDER-pixel zero frame around
 * every image: [B][h + 2*YV7_BORDER][w + 2*YV7_BORDER][C].  Kernels write only interiors; the frame
 * serves every 3x3 / pad-1 window's out-of-image taps.  yv7_forward clears a workspace the first
 * time it sees it with a given layout (pointer, size and batch geometry B, H, W) and trusts the frame
 * on later calls with that layout.  So between calls the workspace memory belongs to the plan: a
 * caller that frees it, reuses it for anything else or writes into it calls yv7_workspace_forget
 * first (the Python binding does so whenever it drops a workspace). */
#define YV7_BORDER 1

typedef enum {
  YV7_OK = 0,
  YV7_E_ARG = -1,       /* bad argument (null pointer, bad enum) */
  YV7_E_SHAPE = -2,     /* shape not supported by the plan (e.g. H/W not a multiple of max stride) */
  YV7_E_WORKSPACE = -3, /* workspace too small */
  YV7_E_ABI = -4,       /* descriptor abi_version mismatch */
  YV7_E_DEVICE = -5     /* no gfx950 device / wrong device */
} yv7_status;

typedef enum { YV7_DT_F32 = 0, YV7_DT_F16 = 1 } yv7_dtype;
typedef enum { YV7_ACT_NONE = 0, YV7_ACT_SILU = 1, YV7_ACT_LEAKY = 2 } yv7_act;
/* Weight / arithmetic format of one CONV op.  FP8 (fp16 plans, 1x1 stride-1 convs only; BASELINE
 * configs[4]): weights OCP e4m3 [cout_pad32][cin padded to 128] at w_off with fp32 per-output-channel
 * scales [cout] at s_off; the fp16 input is quantized per tensor, x8 = e4m3(clamp(x / xscale, +-448)),
 * and the GEMM runs on the block-scaled fp8 MFMA; y = act(acc * xscale * wscale[c] + bias[c]). */
typedef enum { YV7_WFMT_PLAN = 0, YV7_WFMT_FP8 = 1 } yv7_wfmt;

typedef enum {
  YV7_OP_INPUT = 0,    /* NCHW image batch -> NHWC tensor; k=2 means fused ReOrg space-to-depth; cout = the
                          image's channels C (k=2: 4 C), 1 .. the tensor's channels (0: the 3-channel image) */
  YV7_OP_CONV = 1,     /* k x k conv, stride s, pad, + fp32 bias + act; NHWC channel slices in/out */
  YV7_OP_MAXPOOL = 2,  /* max pool k, stride s, pad (implicit -inf padding) */
  YV7_OP_UPSAMPLE = 3, /* nearest-neighbour x2 */
  YV7_OP_COPY = 4,     /* channel-slice copy (concat input that could not be written in place) */
  YV7_OP_DETECT = 5,   /* 1x1 conv + bias + sigmoid + grid/anchor decode -> z rows, raw logits */
  YV7_OP_STEM = 6,     /* fp16: image -> conv A (cin->32, 3x3, stride s) -> conv B (32->64, 3x3, s2), A kept in LDS;
                          cin = the image's channels, 1..4 (weights K = tap*cin + ci);
                          cin 12: the yolov7-w6 front end, image -> ReOrg (common.py:48-53) -> conv A (12->64,
                          3x3, s1; weights K = tap*16 + ci) -> conv B (64->128, 3x3, s2) */
  YV7_OP_ADD = 7       /* dst = src + src2 over cout channels (Shortcut, common.py:80-86): three channel slices with
                          their own tensors, offsets and pitches; fp16 adds in fp32 and rounds once */
} yv7_op_kind;

/* One NHWC activation tensor of the plan: [B, H >> shift, W >> shift, channels]. Tensor 0 is the
 * packed network input written by YV7_OP_INPUT. */
typedef struct {
  int32_t channels; /* channel count == row pitch in elements (multiple of 8) */
  int32_t shift;    /* log2 spatial downsampling relative to the network input */
} yv7_tensor_desc;

typedef struct {
  int32_t kind;                /* yv7_op_kind */
  int32_t src, src_coff, cin;  /* input tensor, channel offset, channels read */
  int32_t dst, dst_coff, cout; /* output tensor, channel offset, channels written */
  int32_t k, s, pad, act;      /* window / stride / padding / yv7_act */
  int32_t level;               /* DETECT: head level */
  int64_t w_off;               /* CONV/DETECT: byte offset of weights [cout_pad32][k][k][cin], K padded to 64 */
  int64_t b_off;               /* CONV/DETECT: byte offset of fp32 bias [cout_pad] */
  int32_t cout2, act2;         /* STEM: second conv's output channels / activation */
  int64_t w2_off, b2_off;      /* STEM: second conv's weights / bias */
  int32_t wfmt;                /* CONV: yv7_wfmt */
  float xscale;                /* CONV, wfmt FP8: per-tensor input scale (a power of two) */
  int64_t s_off;               /* CONV, wfmt FP8: byte offset of fp32 weight scales [cout] */
  int32_t pool;                /* CONV (fp16 plans, 1x1): 2 = the input is first max-pooled 2x2 / stride 2 (an MP
                                  layer, common.py:30-36, folded into the conv's operand loads); then s = 2 */
  int32_t reserved;
  int32_t src2, src2_coff;     /* ADD: the second operand's tensor and channel offset (cout channels).  CONV (fp16
                                  plans, wfmt PLAN, pool 0): a residual of the output's resolution, cout channels at
                                  src2_coff, added after bias and activation in fp32 and rounded once (a Shortcut
                                  folded into its producer); -1 = none.  Every other kind: -1 */
} yv7_op_desc;

typedef struct {
  int32_t abi_version;   /* YV7_ABI_VERSION */
  int32_t dtype;         /* yv7_dtype of activations and packed weights */
  int32_t n_tensors;
  const yv7_tensor_desc* tensors;
  int32_t n_ops;
  const yv7_op_desc* ops;
  int32_t nl, na, no;    /* detection levels, anchors per level, outputs per anchor (nc + 5) */
  const float* stride;   /* [nl] */
  const float* anchor_grid; /* [nl][na][2] anchor sizes in pixels (Detect.anchor_grid) */
  int32_t max_shift;     /* input H and W must be multiples of 1 << max_shift */
} yv7_net_desc;

typedef struct yv7_plan yv7_plan;

int32_t yv7_abi_version(void);
const char* yv7_last_error(void);

/* weights: host or device pointer to the packed blob (copied into plan-owned device memory). */
int yv7_plan_create(const yv7_net_desc* desc, const void* weights, size_t nbytes, int device,
                    yv7_plan** out);
void yv7_plan_destroy(yv7_plan* plan);

/* Bytes of caller-provided workspace yv7_forward needs for a [B,C,H,W] batch. */
size_t yv7_workspace_bytes(const yv7_plan* plan, int B, int H, int W);
/* Hand workspace memory [ws, ws + bytes) back to the caller: the next yv7_forward on any part of it
 * clears it again. */
int yv7_workspace_forget(yv7_plan* plan, const void* ws, size_t bytes);
/* Rows of z per image: sum over levels of na * (H >> s_l) * (W >> s_l). */
int64_t yv7_num_rows(const yv7_plan* plan, int H, int W);

/* Per-row detection score record (16 bytes), one per row of z: the objectness z[..., 4], the
 * single-label NMS score max_c z[..., 5 + c] * z[..., 4] with its first-max class (general.py:669-684,
 * computed from the very floats written to z).  yv7_nms / yv7_end2end accept it instead of
 * re-reading every row of z for the candidate filter. */
typedef struct {
  float obj;
  float conf;
  int32_t cls;
  int32_t reserved;
} yv7_row_best;

/* x: [B,C,H,W] (x_dtype f32 or f16, values in [0,1]) on the plan's device; C is fixed by the plan (its
 * INPUT op's cout, or its STEM op's cin; 3 for the ReOrg stem) and is not passed: the caller checks it.
 * z_out: [B, N, no] fp32 decoded boxes (Detect z).  raw_out (nullable): per level l the raw head
 * logits [B, na, ny_l, nx_l, no] fp32, levels concatenated.  rowbest_out (nullable): [B, N]
 * yv7_row_best (fp16 plans write it from the head's epilogue).  Asynchronous on `stream`. */
int yv7_forward(yv7_plan* plan, const void* x, int x_dtype, int B, int H, int W, float* z_out,
                float* raw_out, yv7_row_best* rowbest_out, void* workspace, size_t ws_bytes, void* stream);

/* The kernels the dispatch launches for every op of a [B,C,H,W] forward, without running it (a dry
 * run of yv7_forward's op loop): one line per op, "op<TAB>kernel[|kernel...]", kernel = the demangled
 * symbol rocprofv3's kernel trace reports.  Lets a caller attribute per-op timings (yv7_profile_read)
 * to kernel families.  x_dtype: the image dtype the forward would get (the INPUT / STEM kernels depend on
 * it).  An op that would launch more than 4 kernels is an error.  Needs the plan's device to be current;
 * buf receives a NUL-terminated string. */
int yv7_op_kernels(yv7_plan* plan, int B, int H, int W, int x_dtype, char* buf, size_t bytes);

/* Force the kernel configuration of one CONV / DETECT op (0 = the tuned dispatch, the default).  A CONV that
 * carries a residual takes only the variants of the families with the residual epilogue (1, 4, 6 and the ring's
 * 100 + 10 * configuration + K splits); any other is an error.  For
 * parity tests of every kernel variant and A/B timing; the accepted values are the real kernel
 * configurations of the fp16 dispatch (the `abi` rows of csrc/conv_f16.hip's forced-variant table),
 * never its microbenchmark hooks.  A split-K
 * variant changes yv7_workspace_bytes. */
int yv7_set_op_variant(yv7_plan* plan, int op, int variant);

/* Live per-op timing: with max_forwards > 0 every following yv7_forward (up to max_forwards of
 * them) launches each op's kernels with a (start, stop) HIP event pair (hipExtLaunchKernel: the
 * first kernel's dispatch begin, the last kernel's end — the interval rocprofv3's kernel trace
 * reports); an op that launches nothing records both events back to back.  0 turns it off and frees
 * the events.  yv7_profile_read synchronizes on the recorded events and returns, per op, the elapsed
 * milliseconds summed over the recorded forwards (op_ms: [n_ops]). */
int yv7_profile_enable(yv7_plan* plan, int max_forwards);
int yv7_profile_read(yv7_plan* plan, int* n_forwards, float* op_ms);

/* Byte offset of activation tensor `tensor_id` inside the forward workspace and its bordered NHWC dims
 * (B, h + 2*YV7_BORDER, w + 2*YV7_BORDER, C); the image interior starts at [YV7_BORDER][YV7_BORDER].
 * Lets a caller read any intermediate layer for per-layer parity checks. */
int yv7_tensor_info(const yv7_plan* plan, int tensor_id, int B, int H, int W, int64_t* offset,
                    int64_t* dims4);

/* Byte range of the fp8 staging buffer inside the forward workspace (the dense e4m3 copy of an FP8
 * op's input; after a forward it holds the last FP8 op's quantized input).  bytes = 0 when the plan
 * has no FP8 op.  For parity tests of the quantization. */
int yv7_f8_scratch_info(const yv7_plan* plan, int B, int H, int W, int64_t* offset, int64_t* bytes);

/* Batched NMS over z [B,N,no] fp32, the semantics of utils/general.py:628-720.
 * det: [B,max_det,6] (x1,y1,x2,y2,conf,cls), src_row: [B,max_det] int64 anchor row of each kept
 * box, count: [B] int32.  classes: nullable [ncls] int32 class filter.  rowbest (nullable): the
 * yv7_row_best records of z from yv7_forward; used for the single-label, unfiltered case. */
size_t yv7_nms_workspace_bytes(int B, int N, int no, int multi_label, int max_nms);
int yv7_nms(const float* z, const yv7_row_best* rowbest, int B, int N, int no, float conf_thres,
            float iou_thres, int multi_label, int agnostic, const int32_t* classes, int ncls, int max_det,
            int max_nms, float* det, int64_t* src_row, int32_t* count, void* workspace, size_t ws_bytes,
            void* stream);

/* EfficientNMS_TRT-shaped output (End2End, experimental.py:226-241): num_dets int32 [B,1],
 * det_boxes [B,topk,4], det_scores [B,topk], det_classes int32 [B,topk]; zero-padded. */
size_t yv7_end2end_workspace_bytes(int B, int N, int no, int topk);
int yv7_end2end(const float* z, int B, int N, int no, float conf_thres, float iou_thres, int topk,
                int32_t* num_dets, float* det_boxes, float* det_scores, int32_t* det_classes,
                void* workspace, size_t ws_bytes, void* stream);

/* Frame pre-processing (replaces utils/datasets.py:1277-1307 letterbox() with its cv2.resize
 * INTER_LINEAR + cv2.copyMakeBorder, and detect.py:100-104's BGR->RGB / HWC->CHW / half / 255):
 * src: B uint8 frames [B][H][W][3] BGR on the device; the host computes the letterbox geometry
 * (new_h x new_w resized image placed at (top, left) of an out_h x out_w canvas of colour
 * (pad_b, pad_g, pad_r)), exactly as letterbox() does.  out_kind: 0 = uint8 [B][out_h][out_w][3]
 * BGR (the letterboxed frame), 1 = fp16 [B][3][out_h][out_w] RGB / 255, 2 = fp32 likewise (the model
 * input).  The workspace holds the resize tables (yv7_letterbox_workspace_bytes).  Asynchronous. */
size_t yv7_letterbox_workspace_bytes(int new_h, int new_w);
int yv7_letterbox(const void* src, int B, int H, int W, int new_h, int new_w, int top, int left, int out_h,
                  int out_w, int pad_b, int pad_g, int pad_r, int out_kind, void* dst, void* workspace,
                  size_t ws_bytes, void* stream);

/* Ragged letterbox (replaces models/common.py:899-918, autoShape's per-image letterbox() loop with np.stack,
 * transpose((0, 3, 1, 2)) and / 255; and a detect.py loop that batches files of different sizes): B frames,
 * each with its own size and host-computed geometry, onto one out_h x out_w canvas in one call.  Per frame the
 * arithmetic is yv7_letterbox's (identity, bilinear or exact-2x area, chosen per frame), bit for bit.
 * frames is a host array the caller may free on return: the descriptors travel to the kernel by value,
 * 64 per launch, and the call is asynchronous on `stream` without any device synchronisation.
 * (pad0, pad1, pad2) is the canvas colour in the input's channel order.  out_kind as yv7_letterbox; the float
 * kinds write planes in the input's channel order (swap_rb = 0: RGB frames, autoShape) or reversed (swap_rb = 1:
 * BGR frames -> RGB planes, detect.py).  The coefficients are computed inline, so the workspace size is 0
 * and workspace may be null. */
typedef struct {
  const void* data;                /* device pointer, uint8 [h][w][3] ([h][w][channels] for the _c form), packed */
  int32_t h, w;                    /* source size */
  int32_t new_h, new_w, top, left; /* resized size and its place on the canvas */
} yv7_frame_desc;

size_t yv7_letterbox_ragged_workspace_bytes(const yv7_frame_desc* frames, int B);
int yv7_letterbox_ragged(const yv7_frame_desc* frames, int B, int out_h, int out_w, int pad0, int pad1, int pad2,
                         int swap_rb, int out_kind, void* dst, void* workspace, size_t ws_bytes, void* stream);

/* Both letterboxes for frames of `channels` interleaved channels, 1..YV7_LETTERBOX_MAX_CH (grayscale, thermal,
 * RGBA, RGB+IR ...): src is uint8 [B][H][W][channels], yv7_frame_desc::data uint8 [h][w][channels], packed.  Per
 * frame the arithmetic is yv7_letterbox's with cn = channels: the same identity, exact-2x area and bilinear modes
 * and coefficients; in the bilinear vertical pass value (x, c) rounds in two steps iff
 * x * channels + c < new_w * channels / 16 * 16 (the SIMD pass runs over the interleaved row; this is
 * oracle/letterbox_ref.py resize_linear_u8 on an [h][w][channels] array).  Outside the resized frame channel c
 * takes pad[c]; pad is a host array of `channels` bytes, read before the call returns.  out_kind 0 writes uint8
 * [B][out_h][out_w][channels] (dst aligned to one pixel for 2 and 4 channels, which store a pixel at once); 1 and
 * 2 write fp16 / fp32 [B][channels][out_h][out_w], each value (float)v / 255.0f rounded once, planes in the
 * input's order.  swap_rb = 1 reverses the float planes and is legal with channels == 3 only; the uint8 kind
 * ignores it.  With channels == 3, yv7_letterbox_ragged_c equals yv7_letterbox_ragged and
 * yv7_letterbox_c(swap_rb = 1) equals yv7_letterbox bit for bit (they launch the same kernels).  Workspaces are
 * the 3-channel functions'.  Asynchronous, no device synchronisation; the ragged form makes no copy either.
 * YV7_E_ARG: channels out of range, swap_rb with channels != 3, null pad, a misaligned 2- / 4-channel uint8 dst. */
#define YV7_LETTERBOX_MAX_CH 16
int yv7_letterbox_c(const void* src, int B, int H, int W, int channels, int new_h, int new_w, int top, int left,
                    int out_h, int out_w, const uint8_t* pad, int swap_rb, int out_kind, void* dst, void* workspace,
                    size_t ws_bytes, void* stream);
int yv7_letterbox_ragged_c(const yv7_frame_desc* frames, int B, int channels, int out_h, int out_w,
                           const uint8_t* pad, int swap_rb, int out_kind, void* dst, void* workspace,
                           size_t ws_bytes, void* stream);

/* Boxes back to image pixels (replaces utils/general.py:340-361 scale_coords(ratio_pad=None) + clip_coords,
 * detect.py:183's .round() and the derived views of Detections.__init__, models/common.py:940-948) on yv7_nms's
 * fixed-shape output, without a host sync.  Per row < count[b] of det [B,max_det,6], in place: columns 0, 2
 * = (x - pad_w) / gain clamped to [0, w0], columns 1, 3 = (y - pad_h) / gain clamped to [0, h0] (IEEE fp32
 * division), then rounded half to even if round_boxes.  The host computes gain = min(h1 / h0, w1 / w0),
 * pad_w = (w1 - w0 * gain) / 2 and pad_h = (h1 - h0 * gain) / 2 in double and narrows them once.
 * xywh (centre, size), xyxyn and xywhn (the two divided by (w0, h0, w0, h0, 1, 1)): nullable [B,max_det,6];
 * their rows >= count[b] are zeroed, det's are left alone.  images is a host array, passed on by value. */
typedef struct {
  int32_t h0, w0; /* the image's own size */
  float gain, pad_w, pad_h;
} yv7_scale_desc;

int yv7_scale_boxes(float* det, const int32_t* count, int B, int max_det, const yv7_scale_desc* images,
                    int round_boxes, float* xywh, float* xyxyn, float* xywhn, void* stream);

/* Predictions matched to labels for mAP (replaces test.py:179-213, the per-image, per-class loop with .item()
 * inside, together with the labels' way to native pixels, test.py:123,131,186-187), for the whole batch in one
 * launch per 64 images and without a host sync.
 * det, count: yv7_nms's output AFTER yv7_scale_boxes, i.e. boxes in each image's own pixels.  targets: device
 * [L,6] rows (image, class, x, y, w, h) normalised to the canvas_h x canvas_w canvas, sorted by image;
 * label_off: device [B+1] with image b's labels in rows label_off[b] .. label_off[b+1] (0 first, L last).
 * images: host array, passed on by value, of the descriptors of scale_coords(ratio_pad): (h0, w0, gain, pad_w,
 * pad_h).  iouv: host array of niou <= 16 ascending IoU thresholds (torch.linspace(0.5, 0.95, 10) as fp32).
 * A label becomes native pixels in fp32 in the reference's order: (x, y, w, h) * (canvas_w, canvas_h, canvas_w,
 * canvas_h), x -+ w / 2, minus the pad, IEEE division by gain, clamp to [0, w0] / [0, h0].  Each row
 * r < count[b] takes the label of its class (float equality with det[r,5]) of highest box_iou, the first one
 * on ties (torch.max); a NaN among them gives none.  A row whose best IoU exceeds iouv[0] claims its label; a
 * label goes to the lowest such row and every other row that chose it gets nothing (test.py:202-210).
 * correct [B,max_det,niou] uint8: best > iouv[:] for the winners, 0 elsewhere (rows >= count[b] included);
 * claimed_by [L] int32: the winning row of each label, or -1.  Both are written in full. */
int yv7_match(const float* det, const int32_t* count, int B, int max_det, const float* targets,
              const int32_t* label_off, int L, const yv7_scale_desc* images, int canvas_h, int canvas_w,
              const float* iouv, int niou, uint8_t* correct, int32_t* claimed_by, void* stream);

/* The evaluation's confusion matrix (replaces ConfusionMatrix.process_batch, utils/metrics.py:121-159, as test.py
 * calls it per image at :188-189 with its two skips at :137-140 and :181), for a whole batch in one launch per 64
 * images and without a host sync.  det, count, targets, label_off, images, canvas_h, canvas_w: exactly yv7_match's,
 * and a label becomes native pixels by the same arithmetic.  All inputs are read-only; count and label_off are
 * clamped on the device.
 * matrix: device int32, (nc + 1) * (nc + 1) + 1 entries, row-major [row][col], 1 <= nc <= 1024.  The call ADDS
 * into it and never zeroes it: the caller zeroes it once per evaluation.  The last entry counts dropped increments.
 * ws: device scratch of at least yv7_confusion_ws_bytes(B, max_det, L) bytes, 8-byte aligned (per-label bids and
 * per-row choices: neither max_det nor the labels per image are limited).
 * Per image b: nothing is added if count[b] == 0 or the image has no labels.  Rows r < count[b] with
 * det[r,4] > conf (strict, fp32) are live.  box_iou in fp32 between every label and every live row, classes
 * playing no part; a pair is a candidate iff iou > iou_thres (strict; a NaN never is).  Each live row keeps its
 * candidate label of highest IoU; each label keeps, among the rows that chose it, the row of highest IoU: those
 * pairs are the matches, and a row whose label went to another row is unmatched (it takes no second choice).
 * With gc the label's class and dc the row's: a matched label adds 1 at [gc][dc], an unmatched label at [nc][gc];
 * if the image has at least one match every unmatched live row adds 1 at [dc][nc], otherwise the rows add nothing
 * (the reference's `if n:`).  A class is its float truncated toward zero; outside [0, nc) or NaN, that increment
 * is dropped and the last entry is incremented instead.
 * Ties, which the reference leaves to an unstable argsort: a row takes the first maximum in label order, a label
 * takes the lowest row index.  The sums are integers: identical from run to run. */
size_t yv7_confusion_ws_bytes(int B, int max_det, int L);
int yv7_confusion(const float* det, const int32_t* count, int B, int max_det, const float* targets,
                  const int32_t* label_off, int L, const yv7_scale_desc* images, int canvas_h, int canvas_w,
                  float conf, float iou_thres, int nc, int32_t* matrix, void* ws, size_t ws_bytes, void* stream);

/* COCO bbox matching (restates pycocotools' COCOeval.evaluateImg, which test.py:256-278 reaches through
 * ev.evaluate(); the library itself is not used), for a whole batch in one launch per 64 images and without a host
 * sync.  All inputs are read-only; count and gt_off are clamped on the device.  All arithmetic is IEEE double
 * without contraction unless said otherwise; the integer outputs are identical from run to run.
 * det, count: yv7_nms's output after yv7_scale_boxes (native pixels), B images of max_det rows.
 * gts: device [G,7] double rows (class index, x, y, w, h, area, iscrowd) sorted by image, in annotation order
 * within an image; gt_off: device [B+1], image b's gts are rows gt_off[b] .. gt_off[b+1].  A gt belongs to the
 * class of a row r iff (double)det[r,5] == gts[g,0].
 * Values: the evaluation runs on what the predictions JSON holds.  In fp32, in xyxy2xywh's order, w = x2 - x1,
 * h = y2 - y1, x = (x1 + x2) / 2 - w / 2, y = (y1 + y2) / 2 - h / 2; each becomes rint((double)v * 1000.0) / 1000.0
 * and the score rint((double)s * 100000.0) / 100000.0 (the products are exact, so this is Python's round(v, 3) and
 * round(s, 5)).  A detection's area is w * h of the rounded values; a gt's area is its own field and is used
 * only for the area ranges.
 * IoU(d, g): w = min(d.x + d.w, g.x + g.w) - max(d.x, g.x), h likewise; 0 if w <= 0 or h <= 0; else i = w * h and
 * i / (d.w * d.h) for a crowd gt, i / (d.w * d.h + g.w * g.h - i) otherwise.
 * Per image and class: the rows r < count[b] of the class in (rounded score descending, row ascending) order;
 * a row's position is its rank, and rows at position >= 100 take no part.  For each of the area ranges
 * a = [0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10] a gt is ignored iff it is a crowd or its area lies outside
 * the range (area < lo or area > hi), and the gts are ordered not-ignored first, annotation order within each
 * group.  For each threshold t of np.linspace(0.5, 0.95, 10) and each detection in rank order:
 *     iou = min(t, 1 - 1e-10); m = -1
 *     for g in gts: if matched[g] and not crowd[g]: continue
 *                   if m > -1 and not ignored[m] and ignored[g]: break
 *                   if IoU(d, g) < iou: continue
 *                   iou = IoU(d, g); m = g
 *     if m > -1: the detection is matched, ignored iff ignored[m]; matched[m] = 1
 * so that among equal IoUs the last gt wins and an IoU equal to the threshold matches.  An unmatched detection is
 * ignored iff its own area lies outside the range.
 * rank [B,max_det] int32: the position within (image, class), -1 for rows >= count[b] or at position >= 100.
 * flags [B,max_det,4] uint32, one word per area range: bit t = matched at threshold t, bit 10 + t = ignored at
 * threshold t; 0 where rank is -1.  Both are written in full.
 * ws: device scratch of at least yv7_coco_match_ws_bytes(B, max_det, G) bytes, 8-byte aligned (the sorted rows and
 * the per-gt match state: neither max_det, nor the rows per class, nor the gts per image or class are limited).
 * A NaN score or class gives that image meaningless flags; nothing is read or written out of bounds. */
size_t yv7_coco_match_ws_bytes(int B, int max_det, int G);
int yv7_coco_match(const float* det, const int32_t* count, int B, int max_det, const double* gts,
                   const int32_t* gt_off, int G, uint32_t* flags, int32_t* rank, void* ws, size_t ws_bytes,
                   void* stream);

/* Boxes and labels drawn onto the frames (replaces utils/plots.py:57-68 plot_one_box as detect.py:204-238 and
 * Detections.display, models/common.py:953-991, call it per box on the host), for a whole batch in two launches
 * per 64 images and without a host sync.  The drawing is integer-only and defined here, not by cv2: corners are
 * square, edges are not anti-aliased, and the text comes from the caller's glyph atlas.
 * images: host array, passed on by value; each frame is drawn in place.  det, count: yv7_nms's output after
 * yv7_scale_boxes, read-only; count is clamped to [0, max_det] on the device.  palette: device uint8 [npal][3] in
 * the frames' channel order, class c takes palette[c % npal].  names (nullable: boxes without labels): device
 * bytes, class c's name is names[name_off[c] .. name_off[c + 1]), name_off device int32 [nc + 1]; a class >= nc
 * gets a box and no label.  atlases: host array of n_atlas <= YV7_DRAW_MAX_ATLAS records, passed on by value.
 * reverse: draw rows count-1 .. 0 (detect.py:209) instead of 0 .. count-1 (Detections.display).
 * ws: device scratch of yv7_draw_ws_bytes(B, max_det) bytes, 16-byte aligned.
 *
 * Per row r < count[b], in draw order, later primitives over earlier ones, everything clipped to the image:
 *   a row with a non-finite value or a negative class draws nothing.
 *   corners: the four coordinates truncated toward zero (after a clamp to +-2^28), xa = min(x1, x2),
 *     xb = max(x1, x2), ya, yb likewise; class = the float truncated.
 *   outline, with t the image's thickness and lo = t / 2: the pixels with x in [xa - lo, xb - lo + t - 1] and
 *     y in [ya - lo, yb - lo + t - 1] for which x is in [xa - lo, xa - lo + t - 1] or [xb - lo, xb - lo + t - 1],
 *     or y is in the same bands of ya, yb; they take the class colour.
 *   label "name d.dd": the digits are n = rint((double)conf * 100) clamped to [0, 100] (round half to even, what
 *     f'{conf:.2f}' prints), written n / 100, '.', n / 10 % 10, n % 10.  tw = the sum of the advances,
 *     th = cell_h.  Background: the class colour on x in [xa, xa + tw], y in [ya - th - 3, ya].  Glyph cells: rows
 *     ya - 1 - th .. ya - 2, character k starting at xa + the advances before it; a cell pixel of coverage a is,
 *     per channel, (a * text + (255 - a) * colour + 127) / 255 with text = (225, 255, 255).
 * A pixel that no primitive covers is not written. */
#define YV7_DRAW_MAX_ATLAS 8
#define YV7_DRAW_TILE_W 64 /* the pixel kernel's tile, for tests that want shapes around it */
#define YV7_DRAW_TILE_H 32

typedef struct {
  void* data;        /* device pointer, uint8 [h][w][3], packed rows */
  int32_t h, w;
  int32_t thickness; /* line thickness t >= 1 */
  int32_t atlas;     /* which glyph atlas the image's labels use (ignored without names) */
} yv7_draw_image;

/* One text height.  metrics: device int32 [95][2], for ASCII 32 .. 126 the glyph's first column in cover and its
 * advance width; a glyph is exactly as wide as its advance.  cover: device uint8 [cell_h][total_w] coverage.
 * Any other byte draws as '?'. */
typedef struct {
  const int32_t* metrics;
  const uint8_t* cover;
  int32_t cell_h, total_w;
} yv7_glyph_atlas;

size_t yv7_draw_ws_bytes(int B, int max_det);
int yv7_draw_boxes(const yv7_draw_image* images, int B, const float* det, const int32_t* count, int max_det,
                   const uint8_t* palette, int npal, const char* names, const int32_t* name_off, int nc,
                   const yv7_glyph_atlas* atlases, int n_atlas, int reverse, void* ws, size_t ws_bytes, void* stream);

/* The picture grid of a batch (replaces utils/plots.py:105-190 plot_images as test.py:215-220 calls it for the
 * first three batches, on the host, on arrays it first copies back): up to ns * ns images pasted as tiles into one
 * picture, predictions or labels drawn on it, a caption and a border per tile, and the whole downscaled, in four
 * launches (two when there are no rows to draw) whatever B, the counts and the number of tiles, and without a host
 * sync.  Integer-only like yv7_draw_boxes, and defined here, not by cv2.  The host computes the geometry
 * (plots.py:128-145, 186-187): n <= ns * ns tiles of tile_h x tile_w, tile i at block_x = tile_w * (i / ns),
 * block_y = tile_h * (i % ns) (column by column); the mosaic is Hs x Ws = ns * tile_h x ns * tile_w.
 * The paint order, later steps over earlier ones, each step over all tiles in turn:
 * a. Canvas: uint8 [Hs][Ws][3], every byte 255.
 * b. Tiles: image i < n of images [B][3][H][W] (planes; in_kind YV7_MOSAIC_U8 as is, _F16 / _F32 in [0, 1] become
 *    clamp(trunc((float)x * 255.0f), 0, 255) with NaN -> 0, the product rounded to fp32) read as an HWC pixel and
 *    pasted at its block: as is when (tile_h, tile_w) == (H, W), else resized by the letterbox's rule bit for bit
 *    (yv7_letterbox's resize: cv2's 8-bit INTER_LINEAR with its exact-2x INTER_AREA fast path and the SIMD
 *    vertical pass's rounding split at tile_w * 3 / 16 * 16).
 * c. Rows, in the order tile 0 .. n - 1 and within a tile row 0 .. last, each drawn exactly as yv7_draw_boxes draws
 *    a row (outline, label background, glyph cells, truncation toward zero, a non-finite value or a negative class
 *    draws nothing, a class >= nc or names == NULL draws a box without a label) with thickness 3, the one atlas,
 *    and clipped to the whole mosaic, not to the tile.  The row's corners are computed in fp32, every product and
 *    sum rounded on its own (no FMA); scaled means sf < 1, and (float)sf is the factor.
 *    Predictions (det != NULL): det [B][max_det][6], count [B] in canvas pixels (before yv7_scale_boxes).  Row
 *      r < clamp(count[i], 0, max_det) of image i < n is drawn iff conf > 0.25f.  Each corner is v * (float)sf if
 *      scaled, then + (float)block_x (x1, x2) or + (float)block_y (y1, y2).  Label "name d.d": the digits are
 *      n = rint((double)conf * 10) clamped to [0, 10], written n / 10, '.', n % 10.
 *    Labels (label_off != NULL): targets [L][6] rows (image, class, x, y, w, h), label_off [B + 1]; image i's rows
 *      are label_off[i] .. label_off[i + 1], clamped to [0, L]; label_off must not decrease (a row that two tiles
 *      claim goes to the first) and column 0 is not read.  Corners x - w / 2, x + w / 2, y - h / 2, y + h / 2;
 *      with normalized != 0 times (float)tile_w (x) or (float)tile_h (y), else times (float)sf if scaled; then the
 *      block offset.  Label "name".  The row's confidence counts as 1.
 *    det and label_off both NULL: no rows.
 * d. Captions (captions and cap_off may both be NULL): tile i's bytes are captions[cap_off[i] .. cap_off[i + 1]),
 *    offsets clamped to [0, cap_bytes].  Glyph cells from pen x = block_x + 5 on rows block_y + 5 ..
 *    block_y + 5 + cell_h - 1, each cell as wide as its advance; a cell pixel of coverage a becomes, per channel,
 *    (a * 220 + (255 - a) * dst + 127) / 255 over whatever is there.  No background; clipped to the mosaic; tiles
 *    in order, so a caption that runs into a later tile's caption is blended first.
 * e. Borders: for every tile, with X0 = block_x, X1 = block_x + tile_w, Y0 = block_y, Y1 = block_y + tile_h, a
 *    pixel becomes (255, 255, 255) when (|x - X0| <= 1 or |x - X1| <= 1) and Y0 - 1 <= y <= Y1 + 1, or when
 *    (|y - Y0| <= 1 or |y - Y1| <= 1) and X0 - 1 <= x <= X1 + 1.  Clipped to the mosaic.
 * f. Output: out uint8 [out_h][out_w][3], Hs / YV7_MOSAIC_MAX_RATIO <= out_h <= Hs and likewise out_w (one thread
 *    sums an output pixel's whole footprint, so the ratio is bounded: a smaller output is refused; plot_images'
 *    own ratio is at most ns).  Equal sizes: a copy.  Otherwise the
 *    exact box filter, with Ws, Hs the mosaic's and Wd, Hd the output's size:
 *      wx(X, x) = max(0, min((X + 1) * Ws, (x + 1) * Wd) - max(X * Ws, x * Wd)), wy(Y, y) likewise,
 *      out[Y][X][c] = (sum_y sum_x wy * wx * S[y][x][c] + Ws * Hs / 2) / (Ws * Hs) in integers
 *    (an exact 2x is (a + b + c + d + 2) >> 2; 3:2 has the weights (2, 1) / (1, 2)).  The sum is bounded by
 *    255 * Ws * Hs + Ws * Hs / 2: with both sides at most YV7_MOSAIC_MAX_SIDE = 16384 a row's inner sum fits
 *    32 bits and the whole 64; larger mosaics are refused.
 * All device inputs are read-only.  ws: device scratch of at least yv7_mosaic_ws_bytes(desc) bytes, 16-byte
 * aligned: the row records (48 bytes each: n * max_det of them, or L), then the canvas.  One thread decides each
 * stored pixel of every step, so nothing depends on execution order. */
#define YV7_MOSAIC_U8 0
#define YV7_MOSAIC_F16 1
#define YV7_MOSAIC_F32 2
#define YV7_MOSAIC_MAX_SIDE 16384
#define YV7_MOSAIC_THICKNESS 3
#define YV7_MOSAIC_MAX_RATIO 8 /* mosaic side : output side, at most */

typedef struct {
  const void* images;      /* device [B][3][H][W] of in_kind */
  int32_t in_kind, B, H, W;
  int32_t n, ns, tile_h, tile_w;
  double sf;               /* max_size / max(H, W); the rows are scaled by (float)sf iff sf < 1 */
  const float* det;        /* predictions: device [B][max_det][6], or NULL */
  const int32_t* count;    /* device [B] */
  int32_t max_det;
  int32_t L;               /* labels: rows of targets */
  const float* targets;    /* device [L][6]; may be NULL when L == 0 */
  const int32_t* label_off; /* device [B + 1], or NULL */
  int32_t normalized;
  int32_t npal;
  const uint8_t* palette;  /* device uint8 [npal][3], as yv7_draw_boxes' */
  const char* names;       /* device bytes, nullable: boxes without labels */
  const int32_t* name_off; /* device [nc + 1] */
  int32_t nc;
  int32_t cap_bytes;       /* the size of captions */
  const char* captions;    /* device bytes, nullable */
  const int32_t* cap_off;  /* device [n + 1], nullable with captions */
  yv7_glyph_atlas atlas;   /* read only with names or captions */
  int32_t out_h, out_w;
} yv7_mosaic_desc;

size_t yv7_mosaic_ws_bytes(const yv7_mosaic_desc* desc);
int yv7_mosaic(const yv7_mosaic_desc* desc, void* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* YV7_H */
