// Boxes and labels drawn onto the frames on the device (gfx950): plot_one_box for a whole batch.
//
// Replaces utils/plots.py:57-68 (plot_one_box: cv2.rectangle + cv2.getTextSize + filled rectangle + cv2.putText)
// as detect.py:204-238 and Detections.display (models/common.py:953-991) call it once per box, per image, on the
// host.  Here the batch's frames, already on the device for the ragged letterbox, are annotated from yv7_nms's
// fixed-shape output after yv7_scale_boxes in two launches per 64 images, reading count[b] on the device.
//
// The drawing is integer arithmetic only and defined by the contract in include/yv7.h, not by
// cv2: square corners, no anti-aliased edges, and the text comes from a glyph atlas the caller supplies.
//
//   draw_prep_kernel   one thread per (image, row < count): the row becomes a record in the workspace.
//   draw_pixels_kernel one block per tile of one image: each thread decides its pixels from the records.
// Both bodies live in draw_device.h, which the mosaic (mosaic.hip) shares.
//
// One thread decides each pixel, so the result cannot depend on the order in which threads run, and overlapping
// boxes need no atomics.  Rows are packed and w may be odd: bytes are stored one by one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "draw_device.h"
#include "yv7_kernels.h"

namespace yv7 {

namespace {

using namespace drawdev;

struct DrawChunk {
  DrawImage im[RAGGED_CHUNK];
};

struct DrawAtlases {
  DrawAtlas a[DRAW_MAX_ATLAS];
};

__global__ void draw_prep_kernel(DrawChunk ch, DrawAtlases at, int b0, const float* __restrict__ det,
                                 const int32_t* __restrict__ count, int max_det, const uint8_t* __restrict__ palette,
                                 int npal, const uint8_t* __restrict__ names, const int32_t* __restrict__ name_off,
                                 int nc, int32_t* __restrict__ ws) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = b0 + blockIdx.y;
  const int cnt = min(max(count[b], 0), max_det);
  if (row >= cnt) return;   // never read
  const DrawImage& im = ch.im[blockIdx.y];
  draw_make_record<LABEL_CONF2>(det + ((size_t)b * max_det + row) * 6, im.t, at.a[im.atlas], palette, npal, names,
                                name_off, nc, ws + ((size_t)b * max_det + row) * REC);
}

__global__ __launch_bounds__(THREADS) void draw_pixels_kernel(
    DrawChunk ch, DrawAtlases at, int b0, const int32_t* __restrict__ count, int max_det,
    const uint8_t* __restrict__ names, const int32_t* __restrict__ name_off, int reverse,
    const int32_t* __restrict__ ws) {
  const DrawImage& im = ch.im[blockIdx.z];
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
  if (tx0 >= im.w || ty0 >= im.h) return;   // the grid is the chunk's largest image
  const int b = b0 + blockIdx.z;
  const int cnt = min(max(count[b], 0), max_det);
  draw_tile_pixels<LABEL_CONF2>(im.data, im.h, im.w, im.t, at.a[im.atlas], tx0, ty0, cnt,
                                ws + (size_t)b * max_det * REC, reverse, names, name_off);
}

}  // namespace

size_t draw_ws_bytes(int B, int max_det) { return (size_t)B * max_det * REC * sizeof(int32_t); }

hipError_t launch_draw_boxes(const DrawImage* images, int B, const float* det, const int32_t* count, int max_det,
                             const uint8_t* palette, int npal, const uint8_t* names, const int32_t* name_off, int nc,
                             const DrawAtlas* atlases, int n_atlas, int reverse, void* ws, hipStream_t st) {
  DrawAtlases at = {};   // without names no atlas is read
  if (names)
    for (int i = 0; i < DRAW_MAX_ATLAS; ++i) at.a[i] = atlases[std::min(i, n_atlas - 1)];   // unused: the last one
  for (int b0 = 0; b0 < B; b0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - b0);
    DrawChunk ch;
    int gw = 0, gh = 0;
    for (int i = 0; i < RAGGED_CHUNK; ++i) {
      ch.im[i] = images[b0 + std::min(i, n - 1)];   // unused: the last one
      if (!names) ch.im[i].atlas = 0;
      gw = std::max(gw, (ch.im[i].w + TW - 1) / TW);
      gh = std::max(gh, (ch.im[i].h + TH - 1) / TH);
    }
    hipLaunchKernelGGL(draw_prep_kernel, dim3((max_det + 127) / 128, n), dim3(128), 0, st, ch, at, b0, det, count,
                       max_det, palette, npal, names, name_off, nc, reinterpret_cast<int32_t*>(ws));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(draw_pixels_kernel, dim3(gw, gh, n), dim3(THREADS), 0, st, ch, at, b0, count, max_det, names,
                       name_off, reverse, reinterpret_cast<const int32_t*>(ws));
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace yv7
