// Predictions matched to labels for mAP evaluation (gfx950): test.py:123,131,179-213 for a whole batch in one
// launch, on yv7_nms's fixed-shape output after yv7_scale_boxes, with no host sync.
//
// The reference walks the images in Python: labels to canvas pixels (test.py:123), xywh2xyxy and scale_coords
// to the image's own pixels (test.py:186-187), then per class box_iou(...).max(1) and a loop in which the first
// prediction (in NMS order) to choose a label keeps it (test.py:192-210).  Here one workgroup takes one image.
//
// Bit-exact against that chain on the CPU: every step is the reference's fp32 operation in the reference's order
// (IEEE division, no contraction: the file is built with -ffp-contract=off and without fast-math like the rest
// of the library), and the label's way to native pixels is scale_boxes_kernel's arithmetic (postprocess.hip).
//
// Per image: rows are taken MATCH_THREADS at a time, a thread per row.  The image's labels pass through LDS in
// chunks of MATCH_THREADS as (class, native box, area); each row keeps its best same-class IoU with torch.max's
// rule (first maximum in label order; a NaN, once met, stays).  A row whose best IoU exceeds iouv[0] claims its
// label with an unsigned atomic min of its row index on claimed_by, in global memory, so labels per image are
// unbounded.  -1 is the largest unsigned value: "unclaimed" needs no second pass.  After a barrier a row has
// won iff its label still holds its index: rows of later batches are larger and cannot take a label back.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "yv7_kernels.h"

namespace yv7 {

namespace {

constexpr int MATCH_THREADS = 256;

struct MatchChunk {
  ScaleImage im[RAGGED_CHUNK];
};

// torch.min / torch.max of two floats: a NaN operand gives NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float tmin(float a, float b) { return (a != a || b != b) ? a + b : fminf(a, b); }
__device__ __forceinline__ float tmax(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }
// Tensor.clamp(0)
__device__ __forceinline__ float clamp0(float a) { return a != a ? a : fmaxf(a, 0.f); }

__global__ __launch_bounds__(MATCH_THREADS) void match_kernel(
    MatchChunk ch, int b0, const float* __restrict__ det, const int32_t* __restrict__ count, int max_det,
    const float* __restrict__ targets, const int32_t* __restrict__ label_off, int L, float canvas_h, float canvas_w,
    MatchIou iouv, int niou, uint8_t* __restrict__ correct, int32_t* claimed_by) {
  __shared__ float s_cls[MATCH_THREADS], s_x1[MATCH_THREADS], s_y1[MATCH_THREADS], s_x2[MATCH_THREADS],
      s_y2[MATCH_THREADS], s_area[MATCH_THREADS];
  const int tid = threadIdx.x;
  const ScaleImage im = ch.im[blockIdx.x];
  const int b = b0 + blockIdx.x;
  const int cnt = min(max(count[b], 0), max_det);
  const int lo = min(max(label_off[b], 0), L);
  const int hi = min(max(label_off[b + 1], lo), L);
  unsigned* claim = reinterpret_cast<unsigned*>(claimed_by);

  for (int l = lo + tid; l < hi; l += MATCH_THREADS)
    __hip_atomic_store(claim + l, 0xffffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  __syncthreads();

  const float w0 = (float)im.w0, h0 = (float)im.h0;
  for (int r0 = 0; r0 < max_det; r0 += MATCH_THREADS) {
    const int row = r0 + tid;
    uint8_t* out = correct + ((size_t)b * max_det + row) * niou;
    if (r0 >= cnt) {   // the whole batch lies beyond count[b] (uniform over the workgroup)
      if (row < max_det)
        for (int k = 0; k < niou; ++k) out[k] = 0;
      continue;
    }
    const bool live = row < cnt;
    float px1 = 0.f, py1 = 0.f, px2 = 0.f, py2 = 0.f, pcls = 0.f, parea = 0.f;
    if (live) {
      const float* p = det + ((size_t)b * max_det + row) * 6;
      px1 = p[0]; py1 = p[1]; px2 = p[2]; py2 = p[3]; pcls = p[5];
      parea = (px2 - px1) * (py2 - py1);
    }
    bool found = false;
    float best = 0.f;
    int best_l = 0;
    for (int c0 = lo; c0 < hi; c0 += MATCH_THREADS) {
      __syncthreads();   // the previous chunk has been read
      if (c0 + tid < hi) {
        const float* t = targets + (size_t)(c0 + tid) * 6;
        // test.py:123 (to canvas pixels), xywh2xyxy, then scale_coords(ratio_pad) + clip_coords
        const float x = t[2] * canvas_w, y = t[3] * canvas_h, w = t[4] * canvas_w, h = t[5] * canvas_h;
        const float x1 = fminf(fmaxf(((x - w / 2.f) - im.pad_w) / im.gain, 0.f), w0);
        const float y1 = fminf(fmaxf(((y - h / 2.f) - im.pad_h) / im.gain, 0.f), h0);
        const float x2 = fminf(fmaxf(((x + w / 2.f) - im.pad_w) / im.gain, 0.f), w0);
        const float y2 = fminf(fmaxf(((y + h / 2.f) - im.pad_h) / im.gain, 0.f), h0);
        s_cls[tid] = t[1]; s_x1[tid] = x1; s_y1[tid] = y1; s_x2[tid] = x2; s_y2[tid] = y2;
        s_area[tid] = (x2 - x1) * (y2 - y1);
      }
      __syncthreads();
      if (live) {
        const int n = min(MATCH_THREADS, hi - c0);
        for (int j = 0; j < n; ++j) {
          if (s_cls[j] != pcls) continue;
          // box_iou, utils/general.py:464-486
          const float iw = clamp0(tmin(px2, s_x2[j]) - tmax(px1, s_x1[j]));
          const float ih = clamp0(tmin(py2, s_y2[j]) - tmax(py1, s_y1[j]));
          const float inter = iw * ih;
          const float iou = inter / ((parea + s_area[j]) - inter);
          // torch.max over the class's labels: the first maximum; a NaN wins and stays
          if (!found || (best == best && (iou != iou || iou > best))) {
            found = true;
            best = iou;
            best_l = c0 + j;
          }
        }
      }
    }
    const bool valid = live && found && best > iouv.v[0];
    if (valid) atomicMin(claim + best_l, (unsigned)row);
    __threadfence();
    __syncthreads();
    bool win = false;
    if (valid) win = __hip_atomic_load(claim + best_l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)row;
    if (row < max_det)
      for (int k = 0; k < niou; ++k) out[k] = (win && best > iouv.v[k]) ? 1 : 0;
  }
}

}  // namespace

hipError_t launch_match(const float* det, const int32_t* count, int B, int max_det, const float* targets,
                        const int32_t* label_off, int L, const ScaleImage* images, int canvas_h, int canvas_w,
                        const MatchIou& iouv, int niou, uint8_t* correct, int32_t* claimed_by, hipStream_t st) {
  for (int b0 = 0; b0 < B; b0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - b0);
    MatchChunk ch;
    for (int i = 0; i < RAGGED_CHUNK; ++i) ch.im[i] = images[b0 + std::min(i, n - 1)];   // unused: the last one
    hipLaunchKernelGGL(match_kernel, dim3(n), dim3(MATCH_THREADS), 0, st, ch, b0, det, count, max_det, targets,
                       label_off, L, (float)canvas_h, (float)canvas_w, iouv, niou, correct, claimed_by);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace yv7
