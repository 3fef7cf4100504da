// Detections back in each image's own pixels (gfx950): scale_coords + clip_coords on yv7_nms's fixed-shape
// output, and the derived views of Detections.
//
// Replaces utils/general.py:340-361 (scale_coords with ratio_pad=None, clip_coords), detect.py:183's .round()
// and models/common.py:940-948 (xywh = xyxy2xywh, xyxyn / xywhn = the two divided by (w, h, w, h, 1, 1)).
// The reference runs these per image on variable-length tensors; here one launch covers the batch's
// [B][max_det][6] rows with no host sync, reading count[b] on the device.
//
// Bit-exact against the CPU reference: the host computes gain and the pads in double as the Python does and
// narrows them to fp32 once (what torch does with a Python scalar operand); the kernel subtracts, divides
// (IEEE fp32 division, not a reciprocal multiply), clamps and optionally rounds half to even in fp32.  This
// file is compiled without fast-math and with -ffp-contract=off like the rest of the library.
//
// One thread per (image, row).  Rows at or beyond count[b] leave det untouched and are zero in the views.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "yv7_kernels.h"

namespace yv7 {

namespace {

struct ScaleChunk {
  ScaleImage im[RAGGED_CHUNK];
};

__device__ __forceinline__ void store6(float* p, float a, float b, float c, float d, float e, float f) {
  p[0] = a; p[1] = b; p[2] = c; p[3] = d; p[4] = e; p[5] = f;
}

__global__ void scale_boxes_kernel(ScaleChunk ch, int b0, float* __restrict__ det, const int32_t* __restrict__ count,
                                   int max_det, int round_boxes, float* __restrict__ xywh,
                                   float* __restrict__ xyxyn, float* __restrict__ xywhn) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= max_det) return;
  const ScaleImage& im = ch.im[blockIdx.y];
  const int b = b0 + blockIdx.y;
  const size_t o = ((size_t)b * max_det + row) * 6;
  if (row >= count[b]) {
    if (xywh) store6(xywh + o, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
    if (xyxyn) store6(xyxyn + o, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
    if (xywhn) store6(xywhn + o, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float w0 = (float)im.w0, h0 = (float)im.h0;
  float x1 = fminf(fmaxf((det[o + 0] - im.pad_w) / im.gain, 0.f), w0);
  float y1 = fminf(fmaxf((det[o + 1] - im.pad_h) / im.gain, 0.f), h0);
  float x2 = fminf(fmaxf((det[o + 2] - im.pad_w) / im.gain, 0.f), w0);
  float y2 = fminf(fmaxf((det[o + 3] - im.pad_h) / im.gain, 0.f), h0);
  if (round_boxes) { x1 = rintf(x1); y1 = rintf(y1); x2 = rintf(x2); y2 = rintf(y2); }
  const float conf = det[o + 4], cls = det[o + 5];
  det[o + 0] = x1; det[o + 1] = y1; det[o + 2] = x2; det[o + 3] = y2;
  const float cx = (x1 + x2) / 2.f, cy = (y1 + y2) / 2.f, bw = x2 - x1, bh = y2 - y1;
  if (xywh) store6(xywh + o, cx, cy, bw, bh, conf, cls);
  if (xyxyn) store6(xyxyn + o, x1 / w0, y1 / h0, x2 / w0, y2 / h0, conf, cls);
  if (xywhn) store6(xywhn + o, cx / w0, cy / h0, bw / w0, bh / h0, conf, cls);
}

}  // namespace

hipError_t launch_scale_boxes(float* det, const int32_t* count, int B, int max_det, const ScaleImage* images,
                              int round_boxes, float* xywh, float* xyxyn, float* xywhn, hipStream_t st) {
  for (int b0 = 0; b0 < B; b0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - b0);
    ScaleChunk ch;
    for (int i = 0; i < RAGGED_CHUNK; ++i) ch.im[i] = images[b0 + std::min(i, n - 1)];   // unused: the last one
    hipLaunchKernelGGL(scale_boxes_kernel, dim3((max_det + 127) / 128, n), dim3(128), 0, st, ch, b0, det, count,
                       max_det, round_boxes, xywh, xyxyn, xywhn);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace yv7
