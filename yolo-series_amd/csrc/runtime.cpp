// libyv7 runtime: the C ABI of include/yv7.h outside the plan — version and error reporting, NMS, the
// End2End output mode, the letterbox (one size or ragged), the boxes' way back to image pixels, the
// matching of predictions to labels and the drawing of boxes onto the frames.
// (Plans: plan_create.cpp, plan_layout.cpp, forward.cpp.)
#include <cmath>

#include "plan.h"

using namespace yv7rt;

namespace {
thread_local std::string g_err;
}  // namespace

int yv7rt::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int yv7rt::hip_fail(hipError_t e, const char* where) {
  g_err = std::string(where) + ": " + hipGetErrorString(e);
  return (int)e;
}

extern "C" {

int32_t yv7_abi_version(void) { return YV7_ABI_VERSION; }

const char* yv7_last_error(void) { return g_err.c_str(); }

size_t yv7_nms_workspace_bytes(int B, int N, int no, int multi_label, int max_nms) {
  if (B <= 0 || N <= 0 || no < 6 || max_nms <= 0) return 0;
  return yv7::nms_workspace_bytes(B, N, no, multi_label, max_nms);
}

static int nms_check(const float* z, int B, int N, int no, int max_det, int max_nms, void* ws, size_t ws_bytes,
                     int multi) {
  if (!z || !ws) return fail(YV7_E_ARG, "yv7_nms: null argument");
  if (B <= 0 || N <= 0 || no < 6 || no - 5 > 128) return fail(YV7_E_SHAPE, "yv7_nms: bad z shape (nc <= 128)");
  if (max_det <= 0 || max_nms <= 0 || max_nms > 65536) return fail(YV7_E_ARG, "yv7_nms: max_det/max_nms out of range");
  if (ws_bytes < yv7::nms_workspace_bytes(B, N, no, multi, max_nms)) return fail(YV7_E_WORKSPACE, "yv7_nms: workspace too small");
  return 0;
}

int yv7_nms(const float* z, const yv7_row_best* rowbest, int B, int N, int no, float conf_thres, float iou_thres,
            int multi_label, int agnostic, const int32_t* classes, int ncls, int max_det, int max_nms, float* det,
            int64_t* src_row, int32_t* count, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = nms_check(z, B, N, no, max_det, max_nms, ws, ws_bytes, multi_label)) return rc;
  if (!det || !src_row || !count || (ncls > 0 && !classes)) return fail(YV7_E_ARG, "yv7_nms: null output");
  hipError_t e = yv7::launch_nms(z, rowbest, B, N, no, conf_thres, iou_thres, multi_label, agnostic, 0,
                                 ncls > 0 ? classes : nullptr, ncls, max_det, max_nms, det, src_row, count, ws,
                                 reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_nms");
  return 0;
}

static const int E2E_MAX_NMS = 65536;

static size_t e2e_layout(int B, int N, int no, int topk, size_t* det_off, size_t* src_off, size_t* cnt_off) {
  const size_t need = yv7::nms_workspace_bytes(B, N, no, 1, E2E_MAX_NMS);
  *det_off = align256(need);
  *src_off = align256(*det_off + sizeof(float) * 6 * (size_t)B * topk);
  *cnt_off = align256(*src_off + sizeof(int64_t) * (size_t)B * topk);
  return align256(*cnt_off + sizeof(int32_t) * (size_t)B);
}

size_t yv7_end2end_workspace_bytes(int B, int N, int no, int topk) {
  if (B <= 0 || N <= 0 || no < 6 || topk <= 0) return 0;
  size_t a, b, c;
  return e2e_layout(B, N, no, topk, &a, &b, &c);
}

int yv7_end2end(const float* z, int B, int N, int no, float conf_thres, float iou_thres, int topk, int32_t* num_dets,
                float* det_boxes, float* det_scores, int32_t* det_classes, void* ws, size_t ws_bytes, void* stream) {
  // multi-label candidates, class-aware IoU on raw boxes (EfficientNMS), top-k by score
  const int max_nms = E2E_MAX_NMS;
  if (topk <= 0) return fail(YV7_E_ARG, "yv7_end2end: topk must be positive");
  if (B <= 0 || N <= 0 || no < 6 || no - 5 > 128) return fail(YV7_E_SHAPE, "yv7_end2end: bad z shape");
  size_t det_off, src_off, cnt_off;
  const size_t total = e2e_layout(B, N, no, topk, &det_off, &src_off, &cnt_off);
  if (!z || !ws || !num_dets || !det_boxes || !det_scores || !det_classes) return fail(YV7_E_ARG, "yv7_end2end: null");
  if (ws_bytes < total) return fail(YV7_E_WORKSPACE, "yv7_end2end: workspace too small (need " + std::to_string(total) + ")");
  unsigned char* w = reinterpret_cast<unsigned char*>(ws);
  float* det = reinterpret_cast<float*>(w + det_off);
  int64_t* src = reinterpret_cast<int64_t*>(w + src_off);
  int32_t* cnt = reinterpret_cast<int32_t*>(w + cnt_off);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = yv7::launch_nms(z, nullptr, B, N, no, conf_thres, iou_thres, 1, 0, 1, nullptr, 0, topk, max_nms,
                                 det, src, cnt, ws, st);
  if (e != hipSuccess) return hip_fail(e, "yv7_end2end nms");
  e = yv7::launch_end2end_pack(det, cnt, B, topk, topk, num_dets, det_boxes, det_scores, det_classes, st);
  if (e != hipSuccess) return hip_fail(e, "yv7_end2end pack");
  return 0;
}

size_t yv7_letterbox_workspace_bytes(int new_h, int new_w) {
  if (new_h <= 0 || new_w <= 0) return 0;
  return yv7::letterbox_workspace_bytes(new_h, new_w);
}

int yv7_letterbox(const void* src, int B, int H, int W, int new_h, int new_w, int top, int left, int out_h,
                  int out_w, int pad_b, int pad_g, int pad_r, int out_kind, void* dst, void* workspace,
                  size_t ws_bytes, void* stream) {
  if (!src || !dst || !workspace) return fail(YV7_E_ARG, "yv7_letterbox: null argument");
  if (out_kind < 0 || out_kind > 2) return fail(YV7_E_ARG, "yv7_letterbox: out_kind must be 0, 1 or 2");
  if (B <= 0 || H <= 0 || W <= 0 || new_h <= 0 || new_w <= 0 || top < 0 || left < 0 || top + new_h > out_h ||
      left + new_w > out_w)
    return fail(YV7_E_SHAPE, "yv7_letterbox: the resized image must lie inside the output canvas");
  if ((size_t)B * H * W * 3 >= ((size_t)1 << 40)) return fail(YV7_E_SHAPE, "yv7_letterbox: input too large");
  for (int v : {pad_b, pad_g, pad_r})
    if (v < 0 || v > 255) return fail(YV7_E_ARG, "yv7_letterbox: pad colour outside 0..255");
  if (ws_bytes < yv7::letterbox_workspace_bytes(new_h, new_w)) return fail(YV7_E_WORKSPACE, "yv7_letterbox: workspace too small");
  const uint8_t pad[3] = {(uint8_t)pad_b, (uint8_t)pad_g, (uint8_t)pad_r};
  hipError_t e = yv7::launch_letterbox(reinterpret_cast<const uint8_t*>(src), B, H, W, new_h, new_w, top, left, out_h,
                                       out_w, pad, out_kind, dst, workspace, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_letterbox launch");
  return 0;
}

static_assert(sizeof(yv7_frame_desc) == sizeof(yv7::RaggedFrame) && sizeof(yv7_scale_desc) == sizeof(yv7::ScaleImage),
              "the kernels' records mirror the ABI descriptors");

size_t yv7_letterbox_ragged_workspace_bytes(const yv7_frame_desc* frames, int B) {
  (void)frames;
  (void)B;
  return 0;   // the resize coefficients are computed inline: no tables to hold
}

int yv7_letterbox_ragged(const yv7_frame_desc* frames, int B, int out_h, int out_w, int pad0, int pad1, int pad2,
                         int swap_rb, int out_kind, void* dst, void* workspace, size_t ws_bytes, void* stream) {
  if (!frames || !dst) return fail(YV7_E_ARG, "yv7_letterbox_ragged: null argument");
  if (B <= 0) return fail(YV7_E_ARG, "yv7_letterbox_ragged: B must be positive");
  if (out_kind < 0 || out_kind > 2) return fail(YV7_E_ARG, "yv7_letterbox_ragged: out_kind must be 0, 1 or 2");
  if (out_h <= 0 || out_w <= 0 || out_h > 65535)
    return fail(YV7_E_SHAPE, "yv7_letterbox_ragged: canvas must be positive and at most 65535 rows");
  for (int v : {pad0, pad1, pad2})
    if (v < 0 || v > 255) return fail(YV7_E_ARG, "yv7_letterbox_ragged: pad colour outside 0..255");
  for (int i = 0; i < B; ++i) {
    const yv7_frame_desc& f = frames[i];
    const std::string who = "yv7_letterbox_ragged: frame " + std::to_string(i);
    if (!f.data) return fail(YV7_E_ARG, who + " has null data");
    if (f.h <= 0 || f.w <= 0 || f.new_h <= 0 || f.new_w <= 0) return fail(YV7_E_SHAPE, who + " has a non-positive size");
    if (f.top < 0 || f.left < 0 || (int64_t)f.top + f.new_h > out_h || (int64_t)f.left + f.new_w > out_w)
      return fail(YV7_E_SHAPE, who + ": the resized image must lie inside the output canvas");
    if ((size_t)f.h * f.w * 3 >= ((size_t)1 << 40)) return fail(YV7_E_SHAPE, who + " is too large");
  }
  if (ws_bytes < yv7_letterbox_ragged_workspace_bytes(frames, B) || (ws_bytes > 0 && !workspace))
    return fail(YV7_E_WORKSPACE, "yv7_letterbox_ragged: workspace null or too small");
  const uint8_t pad[3] = {(uint8_t)pad0, (uint8_t)pad1, (uint8_t)pad2};
  hipError_t e = yv7::launch_letterbox_ragged(reinterpret_cast<const yv7::RaggedFrame*>(frames), B, out_h, out_w, pad,
                                              swap_rb != 0, out_kind, dst, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_letterbox_ragged launch");
  return 0;
}

static_assert(YV7_LETTERBOX_MAX_CH == yv7::LETTERBOX_MAX_CH, "the ABI's channel limit is the kernels'");

// the checks the two channel-count entry points share; dst_align: the uint8 output's packed stores
static int letterbox_c_args(const std::string& who, int channels, const uint8_t* pad, int swap_rb, int out_kind,
                            const void* dst) {
  if (channels < 1 || channels > YV7_LETTERBOX_MAX_CH)
    return fail(YV7_E_ARG, who + ": channels must be 1.." + std::to_string(YV7_LETTERBOX_MAX_CH));
  if (swap_rb && channels != 3) return fail(YV7_E_ARG, who + ": swap_rb needs channels == 3");
  if (!pad) return fail(YV7_E_ARG, who + ": null pad");
  if (out_kind < 0 || out_kind > 2) return fail(YV7_E_ARG, who + ": out_kind must be 0, 1 or 2");
  if (out_kind == 0 && (channels == 2 || channels == 4) && reinterpret_cast<uintptr_t>(dst) % channels)
    return fail(YV7_E_ARG, who + ": a uint8 dst of 2 / 4 channels must be aligned to one pixel");
  return 0;
}

int yv7_letterbox_c(const void* src, int B, int H, int W, int channels, int new_h, int new_w, int top, int left,
                    int out_h, int out_w, const uint8_t* pad, int swap_rb, int out_kind, void* dst, void* workspace,
                    size_t ws_bytes, void* stream) {
  if (!src || !dst || !workspace) return fail(YV7_E_ARG, "yv7_letterbox_c: null argument");
  if (int rc = letterbox_c_args("yv7_letterbox_c", channels, pad, swap_rb, out_kind, dst)) return rc;
  if (B <= 0 || H <= 0 || W <= 0 || new_h <= 0 || new_w <= 0 || top < 0 || left < 0 || top + new_h > out_h ||
      left + new_w > out_w)
    return fail(YV7_E_SHAPE, "yv7_letterbox_c: the resized image must lie inside the output canvas");
  if (out_h > 65535 || B > 65535) return fail(YV7_E_SHAPE, "yv7_letterbox_c: at most 65535 rows and frames");
  if ((size_t)B * H * W * channels >= ((size_t)1 << 40)) return fail(YV7_E_SHAPE, "yv7_letterbox_c: input too large");
  if (ws_bytes < yv7::letterbox_workspace_bytes(new_h, new_w))
    return fail(YV7_E_WORKSPACE, "yv7_letterbox_c: workspace too small");
  hipError_t e = yv7::launch_letterbox_cn(reinterpret_cast<const uint8_t*>(src), B, H, W, channels, new_h, new_w, top,
                                          left, out_h, out_w, pad, swap_rb != 0, out_kind, dst, workspace,
                                          reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_letterbox_c launch");
  return 0;
}

int yv7_letterbox_ragged_c(const yv7_frame_desc* frames, int B, int channels, int out_h, int out_w, const uint8_t* pad,
                           int swap_rb, int out_kind, void* dst, void* workspace, size_t ws_bytes, void* stream) {
  if (!frames || !dst) return fail(YV7_E_ARG, "yv7_letterbox_ragged_c: null argument");
  if (B <= 0) return fail(YV7_E_ARG, "yv7_letterbox_ragged_c: B must be positive");
  if (int rc = letterbox_c_args("yv7_letterbox_ragged_c", channels, pad, swap_rb, out_kind, dst)) return rc;
  if (out_h <= 0 || out_w <= 0 || out_h > 65535)
    return fail(YV7_E_SHAPE, "yv7_letterbox_ragged_c: canvas must be positive and at most 65535 rows");
  for (int i = 0; i < B; ++i) {
    const yv7_frame_desc& f = frames[i];
    const std::string who = "yv7_letterbox_ragged_c: frame " + std::to_string(i);
    if (!f.data) return fail(YV7_E_ARG, who + " has null data");
    if (f.h <= 0 || f.w <= 0 || f.new_h <= 0 || f.new_w <= 0) return fail(YV7_E_SHAPE, who + " has a non-positive size");
    if (f.top < 0 || f.left < 0 || (int64_t)f.top + f.new_h > out_h || (int64_t)f.left + f.new_w > out_w)
      return fail(YV7_E_SHAPE, who + ": the resized image must lie inside the output canvas");
    if ((size_t)f.h * f.w * channels >= ((size_t)1 << 40)) return fail(YV7_E_SHAPE, who + " is too large");
  }
  if (ws_bytes < yv7_letterbox_ragged_workspace_bytes(frames, B) || (ws_bytes > 0 && !workspace))
    return fail(YV7_E_WORKSPACE, "yv7_letterbox_ragged_c: workspace null or too small");
  hipError_t e = yv7::launch_letterbox_ragged_cn(reinterpret_cast<const yv7::RaggedFrame*>(frames), B, channels, out_h,
                                                 out_w, pad, swap_rb != 0, out_kind, dst,
                                                 reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_letterbox_ragged_c launch");
  return 0;
}

int yv7_scale_boxes(float* det, const int32_t* count, int B, int max_det, const yv7_scale_desc* images,
                    int round_boxes, float* xywh, float* xyxyn, float* xywhn, void* stream) {
  if (!det || !count || !images) return fail(YV7_E_ARG, "yv7_scale_boxes: null argument");
  if (B <= 0) return fail(YV7_E_ARG, "yv7_scale_boxes: B must be positive");
  if (max_det <= 0) return fail(YV7_E_ARG, "yv7_scale_boxes: max_det must be positive");
  for (int i = 0; i < B; ++i) {
    const std::string who = "yv7_scale_boxes: image " + std::to_string(i);
    if (images[i].h0 <= 0 || images[i].w0 <= 0) return fail(YV7_E_SHAPE, who + " has a non-positive size");
    if (!(images[i].gain > 0.f) || !std::isfinite(images[i].gain))
      return fail(YV7_E_ARG, who + ": gain must be positive and finite");
  }
  hipError_t e = yv7::launch_scale_boxes(det, count, B, max_det, reinterpret_cast<const yv7::ScaleImage*>(images),
                                         round_boxes != 0, xywh, xyxyn, xywhn, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_scale_boxes launch");
  return 0;
}

int yv7_match(const float* det, const int32_t* count, int B, int max_det, const float* targets,
              const int32_t* label_off, int L, const yv7_scale_desc* images, int canvas_h, int canvas_w,
              const float* iouv, int niou, uint8_t* correct, int32_t* claimed_by, void* stream) {
  if (B <= 0) return fail(YV7_E_ARG, "yv7_match: B must be positive");
  if (max_det <= 0) return fail(YV7_E_ARG, "yv7_match: max_det must be positive");
  if (niou < 1 || niou > yv7::MATCH_MAX_IOU) return fail(YV7_E_ARG, "yv7_match: niou must be in 1..16");
  if (L < 0) return fail(YV7_E_ARG, "yv7_match: L must not be negative");
  if (L > 0 && !targets) return fail(YV7_E_ARG, "yv7_match: null targets with L > 0");
  if (!det || !count || !label_off || !images || !iouv || !correct || (L > 0 && !claimed_by))
    return fail(YV7_E_ARG, "yv7_match: null argument");
  if (canvas_h <= 0 || canvas_w <= 0) return fail(YV7_E_ARG, "yv7_match: canvas must be positive");
  for (int i = 0; i < B; ++i) {
    const std::string who = "yv7_match: image " + std::to_string(i);
    if (images[i].h0 <= 0 || images[i].w0 <= 0) return fail(YV7_E_ARG, who + " has a non-positive size");
    if (!(images[i].gain > 0.f) || !std::isfinite(images[i].gain))
      return fail(YV7_E_ARG, who + ": gain must be positive and finite");
  }
  yv7::MatchIou th;
  for (int k = 0; k < yv7::MATCH_MAX_IOU; ++k) th.v[k] = iouv[std::min(k, niou - 1)];
  hipError_t e = yv7::launch_match(det, count, B, max_det, targets, label_off, L,
                                   reinterpret_cast<const yv7::ScaleImage*>(images), canvas_h, canvas_w, th, niou,
                                   correct, claimed_by, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_match launch");
  return 0;
}

size_t yv7_confusion_ws_bytes(int B, int max_det, int L) { return yv7::confusion_ws_bytes(B, max_det, L); }

int yv7_confusion(const float* det, const int32_t* count, int B, int max_det, const float* targets,
                  const int32_t* label_off, int L, const yv7_scale_desc* images, int canvas_h, int canvas_w,
                  float conf, float iou_thres, int nc, int32_t* matrix, void* ws, size_t ws_bytes, void* stream) {
  if (B <= 0) return fail(YV7_E_ARG, "yv7_confusion: B must be positive");
  if (max_det <= 0) return fail(YV7_E_ARG, "yv7_confusion: max_det must be positive");
  if (nc < 1 || nc > yv7::CONFUSION_MAX_NC) return fail(YV7_E_ARG, "yv7_confusion: nc must be in 1..1024");
  if (L < 0) return fail(YV7_E_ARG, "yv7_confusion: L must not be negative");
  if (L > 0 && !targets) return fail(YV7_E_ARG, "yv7_confusion: null targets with L > 0");
  if (ws_bytes < yv7::confusion_ws_bytes(B, max_det, L)) return fail(YV7_E_ARG, "yv7_confusion: ws_bytes too small");
  if (!det || !count || !label_off || !images || !matrix || !ws) return fail(YV7_E_ARG, "yv7_confusion: null argument");
  if (reinterpret_cast<uintptr_t>(ws) % 8 != 0) return fail(YV7_E_ARG, "yv7_confusion: ws must be 8-byte aligned");
  if (canvas_h <= 0 || canvas_w <= 0) return fail(YV7_E_ARG, "yv7_confusion: canvas must be positive");
  for (int i = 0; i < B; ++i) {
    const std::string who = "yv7_confusion: image " + std::to_string(i);
    if (images[i].h0 <= 0 || images[i].w0 <= 0) return fail(YV7_E_ARG, who + " has a non-positive size");
    if (!(images[i].gain > 0.f) || !std::isfinite(images[i].gain))
      return fail(YV7_E_ARG, who + ": gain must be positive and finite");
  }
  hipError_t e = yv7::launch_confusion(det, count, B, max_det, targets, label_off, L,
                                       reinterpret_cast<const yv7::ScaleImage*>(images), canvas_h, canvas_w, conf,
                                       iou_thres, nc, matrix, ws, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_confusion launch");
  return 0;
}

size_t yv7_coco_match_ws_bytes(int B, int max_det, int G) { return yv7::coco_match_ws_bytes(B, max_det, G); }

int yv7_coco_match(const float* det, const int32_t* count, int B, int max_det, const double* gts,
                   const int32_t* gt_off, int G, uint32_t* flags, int32_t* rank, void* ws, size_t ws_bytes,
                   void* stream) {
  if (B <= 0) return fail(YV7_E_ARG, "yv7_coco_match: B must be positive");
  if (max_det <= 0) return fail(YV7_E_ARG, "yv7_coco_match: max_det must be positive");
  if (G < 0) return fail(YV7_E_ARG, "yv7_coco_match: G must not be negative");
  if (G > 0 && !gts) return fail(YV7_E_ARG, "yv7_coco_match: null gts with G > 0");
  if (ws_bytes < yv7::coco_match_ws_bytes(B, max_det, G))
    return fail(YV7_E_WORKSPACE, "yv7_coco_match: ws_bytes too small");
  if (!det || !count || !gt_off || !flags || !rank || !ws) return fail(YV7_E_ARG, "yv7_coco_match: null argument");
  if (reinterpret_cast<uintptr_t>(ws) % 8 != 0) return fail(YV7_E_ARG, "yv7_coco_match: ws must be 8-byte aligned");
  hipError_t e = yv7::launch_coco_match(det, count, B, max_det, gts, gt_off, G, flags, rank, ws,
                                        reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_coco_match launch");
  return 0;
}

static_assert(sizeof(yv7_draw_image) == sizeof(yv7::DrawImage) && sizeof(yv7_glyph_atlas) == sizeof(yv7::DrawAtlas) &&
                  YV7_DRAW_MAX_ATLAS == yv7::DRAW_MAX_ATLAS && YV7_DRAW_TILE_W == yv7::DRAW_TILE_W &&
                  YV7_DRAW_TILE_H == yv7::DRAW_TILE_H,
              "the drawing kernels' records mirror the ABI descriptors");

size_t yv7_draw_ws_bytes(int B, int max_det) {
  if (B <= 0 || max_det <= 0) return 0;
  return yv7::draw_ws_bytes(B, max_det);
}

int yv7_draw_boxes(const yv7_draw_image* images, int B, const float* det, const int32_t* count, int max_det,
                   const uint8_t* palette, int npal, const char* names, const int32_t* name_off, int nc,
                   const yv7_glyph_atlas* atlases, int n_atlas, int reverse, void* ws, size_t ws_bytes, void* stream) {
  if (B <= 0) return fail(YV7_E_ARG, "yv7_draw_boxes: B must be positive");
  if (max_det <= 0) return fail(YV7_E_ARG, "yv7_draw_boxes: max_det must be positive");
  if (npal < 1) return fail(YV7_E_ARG, "yv7_draw_boxes: npal must be at least 1");
  if (!images || !det || !count || !palette || !ws) return fail(YV7_E_ARG, "yv7_draw_boxes: null argument");
  if (ws_bytes < yv7::draw_ws_bytes(B, max_det)) return fail(YV7_E_WORKSPACE, "yv7_draw_boxes: workspace too small");
  if (reinterpret_cast<uintptr_t>(ws) % 16 != 0) return fail(YV7_E_ARG, "yv7_draw_boxes: ws must be 16-byte aligned");
  if (names) {
    if (!name_off || !atlases) return fail(YV7_E_ARG, "yv7_draw_boxes: names without name_off or atlases");
    if (nc < 1) return fail(YV7_E_ARG, "yv7_draw_boxes: nc must be at least 1 with names");
    if (n_atlas < 1 || n_atlas > YV7_DRAW_MAX_ATLAS)
      return fail(YV7_E_ARG, "yv7_draw_boxes: n_atlas must be in 1..8 with names");
    for (int i = 0; i < n_atlas; ++i) {
      const std::string who = "yv7_draw_boxes: atlas " + std::to_string(i);
      if (!atlases[i].metrics || !atlases[i].cover) return fail(YV7_E_ARG, who + " has a null pointer");
      if (atlases[i].cell_h <= 0 || atlases[i].total_w <= 0 || atlases[i].cell_h > 4096)
        return fail(YV7_E_SHAPE, who + " has a non-positive size or more than 4096 rows");
    }
  }
  for (int i = 0; i < B; ++i) {
    const yv7_draw_image& im = images[i];
    const std::string who = "yv7_draw_boxes: image " + std::to_string(i);
    if (!im.data) return fail(YV7_E_ARG, who + " has null data");
    if (im.h <= 0 || im.w <= 0) return fail(YV7_E_SHAPE, who + " has a non-positive size");
    if (im.h > (1 << 20) || im.w > (1 << 20)) return fail(YV7_E_SHAPE, who + " is too large (a side above 2^20)");
    if (im.thickness < 1 || im.thickness > 4096) return fail(YV7_E_ARG, who + ": thickness must be in 1..4096");
    if (names && (im.atlas < 0 || im.atlas >= n_atlas)) return fail(YV7_E_ARG, who + ": atlas index out of range");
  }
  hipError_t e = yv7::launch_draw_boxes(reinterpret_cast<const yv7::DrawImage*>(images), B, det, count, max_det,
                                        palette, npal, reinterpret_cast<const uint8_t*>(names), name_off, nc,
                                        reinterpret_cast<const yv7::DrawAtlas*>(atlases), n_atlas, reverse != 0, ws,
                                        reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_draw_boxes launch");
  return 0;
}

static_assert(YV7_MOSAIC_MAX_SIDE == yv7::MOSAIC_MAX_SIDE && YV7_MOSAIC_THICKNESS == yv7::MOSAIC_THICKNESS,
              "the mosaic kernels' constants mirror the header's");

// the descriptor's checks that need no workspace; fills a
static int mosaic_check(const yv7_mosaic_desc* d, yv7::MosaicArgs* a) {
  if (!d) return fail(YV7_E_ARG, "yv7_mosaic: null argument");
  if (!d->images) return fail(YV7_E_ARG, "yv7_mosaic: null images");
  if (d->in_kind < YV7_MOSAIC_U8 || d->in_kind > YV7_MOSAIC_F32)
    return fail(YV7_E_ARG, "yv7_mosaic: in_kind must be YV7_MOSAIC_U8, _F16 or _F32");
  if (d->B <= 0 || d->H <= 0 || d->W <= 0) return fail(YV7_E_SHAPE, "yv7_mosaic: B, H and W must be positive");
  if (d->H > (1 << 20) || d->W > (1 << 20)) return fail(YV7_E_SHAPE, "yv7_mosaic: an image side above 2^20");
  if (d->n <= 0 || d->ns <= 0 || d->tile_h <= 0 || d->tile_w <= 0)
    return fail(YV7_E_SHAPE, "yv7_mosaic: n, ns, tile_h and tile_w must be positive");
  if (d->n > d->B) return fail(YV7_E_SHAPE, "yv7_mosaic: n exceeds B");
  if ((int64_t)d->ns * d->tile_h > YV7_MOSAIC_MAX_SIDE || (int64_t)d->ns * d->tile_w > YV7_MOSAIC_MAX_SIDE)
    return fail(YV7_E_SHAPE, "yv7_mosaic: the mosaic is too large (a side above 16384)");
  if ((int64_t)d->n > (int64_t)d->ns * d->ns) return fail(YV7_E_SHAPE, "yv7_mosaic: n exceeds ns * ns");
  if (!(d->sf > 0.0)) return fail(YV7_E_ARG, "yv7_mosaic: sf must be positive");
  if (d->out_h <= 0 || d->out_w <= 0) return fail(YV7_E_SHAPE, "yv7_mosaic: out_h and out_w must be positive");
  if (d->out_h > d->ns * d->tile_h || d->out_w > d->ns * d->tile_w)
    return fail(YV7_E_SHAPE, "yv7_mosaic: the output is larger than the mosaic");
  // one thread sums an output pixel's whole footprint: keep it to (ratio + 1)^2 canvas pixels
  if ((int64_t)d->ns * d->tile_h > (int64_t)YV7_MOSAIC_MAX_RATIO * d->out_h ||
      (int64_t)d->ns * d->tile_w > (int64_t)YV7_MOSAIC_MAX_RATIO * d->out_w)
    return fail(YV7_E_SHAPE, "yv7_mosaic: the output is more than 8 times smaller than the mosaic");
  const bool pred = d->det != nullptr, lab = d->label_off != nullptr;
  if (pred && (lab || d->targets)) return fail(YV7_E_ARG, "yv7_mosaic: predictions and labels both given");
  if (pred) {
    if (!d->count) return fail(YV7_E_ARG, "yv7_mosaic: det without count");
    if (d->max_det <= 0) return fail(YV7_E_ARG, "yv7_mosaic: max_det must be positive");
    if ((int64_t)d->n * d->max_det > (1 << 24)) return fail(YV7_E_SHAPE, "yv7_mosaic: more than 2^24 rows");
  } else if (lab) {
    if (d->L < 0 || d->L > (1 << 24)) return fail(YV7_E_SHAPE, "yv7_mosaic: L must be in 0..2^24");
    if (d->L > 0 && !d->targets) return fail(YV7_E_ARG, "yv7_mosaic: label_off without targets");
  } else if (d->targets) {
    return fail(YV7_E_ARG, "yv7_mosaic: targets without label_off");
  }
  if (pred || (lab && d->L > 0)) {
    if (!d->palette) return fail(YV7_E_ARG, "yv7_mosaic: rows without a palette");
    if (d->npal < 1) return fail(YV7_E_ARG, "yv7_mosaic: npal must be at least 1");
    if (d->names && !d->name_off) return fail(YV7_E_ARG, "yv7_mosaic: names without name_off");
    if (d->names && d->nc < 1) return fail(YV7_E_ARG, "yv7_mosaic: nc must be at least 1 with names");
  }
  if ((d->captions != nullptr) != (d->cap_off != nullptr))
    return fail(YV7_E_ARG, "yv7_mosaic: captions and cap_off go together");
  if (d->captions && d->cap_bytes < 0) return fail(YV7_E_ARG, "yv7_mosaic: cap_bytes must not be negative");
  if (d->names || d->captions) {
    if (!d->atlas.metrics || !d->atlas.cover) return fail(YV7_E_ARG, "yv7_mosaic: the atlas has a null pointer");
    if (d->atlas.cell_h <= 0 || d->atlas.total_w <= 0 || d->atlas.cell_h > 4096)
      return fail(YV7_E_SHAPE, "yv7_mosaic: the atlas has a non-positive size or more than 4096 rows");
  }
  a->g = {d->n, d->ns, d->tile_h, d->tile_w};
  a->images = d->images;
  a->in_kind = d->in_kind; a->B = d->B; a->H = d->H; a->W = d->W;
  a->sf = d->sf;
  a->det = d->det; a->count = d->count; a->max_det = d->max_det;
  a->targets = d->targets; a->label_off = d->label_off; a->L = d->L; a->normalized = d->normalized != 0;
  a->palette = d->palette; a->npal = d->npal;
  a->names = reinterpret_cast<const uint8_t*>(d->names); a->name_off = d->name_off; a->nc = d->nc;
  a->captions = reinterpret_cast<const uint8_t*>(d->captions); a->cap_off = d->cap_off; a->cap_bytes = d->cap_bytes;
  a->atlas = {d->atlas.metrics, d->atlas.cover, d->atlas.cell_h, d->atlas.total_w};
  a->out_h = d->out_h; a->out_w = d->out_w;
  return 0;
}

size_t yv7_mosaic_ws_bytes(const yv7_mosaic_desc* desc) {
  yv7::MosaicArgs a;
  if (mosaic_check(desc, &a)) return 0;
  return yv7::mosaic_ws_bytes(a);
}

int yv7_mosaic(const yv7_mosaic_desc* desc, void* out, void* ws, size_t ws_bytes, void* stream) {
  yv7::MosaicArgs a;
  if (int rc = mosaic_check(desc, &a)) return rc;
  if (!out || !ws) return fail(YV7_E_ARG, "yv7_mosaic: null argument");
  if (ws_bytes < yv7::mosaic_ws_bytes(a)) return fail(YV7_E_WORKSPACE, "yv7_mosaic: workspace too small");
  if (reinterpret_cast<uintptr_t>(ws) % 16 != 0) return fail(YV7_E_ARG, "yv7_mosaic: ws must be 16-byte aligned");
  hipError_t e = yv7::launch_mosaic(a, reinterpret_cast<uint8_t*>(out), ws, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "yv7_mosaic launch");
  return 0;
}

}  // extern "C"
