// The picture grid of a batch on the device (gfx950): plot_images for test_batch*_labels.jpg / _pred.jpg.
//
// Replaces utils/plots.py:105-190 (plot_images: per image a cv2.resize, a paste, plot_one_box per row, cv2.putText
// and cv2.rectangle, then one cv2.resize INTER_AREA of the whole) as test.py:215-220 runs it in threads on arrays
// copied back to the host.  Here the batch, nms_batched's det / count and the label rows are already on the device,
// and the picture is built from them in four launches without reading count on the host.  The contract is in
// include/yv7.h; steps a-f there map to the kernels as follows.
//
//   mosaic_tiles_kernel   a + b: one thread per canvas pixel; inside a tile i < n it takes the image's pixel
//                         (resize_u8.h: the letterbox's resize, reading planes of u8 / fp16 / fp32), else 255.
//   mosaic_rows_kernel    c: one thread per candidate row (tile, r < max_det) or label row; the corners go to mosaic
//                         coordinates in fp32 and become a draw record (draw_device.h).  A row that is not drawn gets
//                         an empty record, so the record count is fixed and count is only read here.
//   mosaic_pixels_kernel  c: draw_device.h's tile walk over the canvas as one image with all the records.
//   mosaic_output_kernel  d + e + f: one thread per output pixel; each canvas pixel it reads goes through the
//                         captions' blends and the borders first, then into the box filter's integer sum.
//
// One thread decides each stored pixel in every kernel: no atomics, no dependence on execution order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "draw_device.h"
#include "resize_u8.h"
#include "yv7_kernels.h"

namespace yv7 {

namespace {

using namespace drawdev;

__device__ __forceinline__ int unit_to_u8(float x) {   // clamp(trunc(x * 255), 0, 255), NaN -> 0
  const float f = __fmul_rn(x, 255.0f);
  return f >= 255.0f ? 255 : (f > 0.0f ? (int)f : 0);
}

template <int KIND>
__device__ __forceinline__ int plane_value(const void* __restrict__ p, size_t i) {
  if constexpr (KIND == 0) return reinterpret_cast<const uint8_t*>(p)[i];
  else if constexpr (KIND == 1) return unit_to_u8((float)reinterpret_cast<const _Float16*>(p)[i]);
  else return unit_to_u8(reinterpret_cast<const float*>(p)[i]);
}

template <int KIND>
__global__ void mosaic_tiles_kernel(MosaicGeom g, const void* __restrict__ images, int H, int W, int mode, double sx,
                                    double sy, uint8_t* __restrict__ canvas) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  const int Ws = g.ns * g.tile_w;
  if (x >= Ws) return;
  const int col = x / g.tile_w, row = y / g.tile_h;
  const int i = col * g.ns + row;
  int v[3] = {255, 255, 255};
  if (i < g.n) {
    const size_t plane = (size_t)H * W, base = (size_t)i * 3 * plane;
    resize_px([=](int yy, int xx, int c) -> int {
                return plane_value<KIND>(images, base + c * plane + (size_t)yy * W + xx);
              }, mode, H, W, g.tile_w, sx, sy, x - col * g.tile_w, y - row * g.tile_h, v);
  }
  uint8_t* d = canvas + ((size_t)y * Ws + x) * 3;
  d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
}

struct MosaicRows {
  const float* det;
  const int32_t* count;
  const float* targets;
  const int32_t* label_off;
  int max_det, L, normalized, scaled;
  float sf;
};

// PRED: thread j is row j % max_det of tile j / max_det; else label row j of the tile whose label_off range holds it
template <bool PRED>
__global__ void mosaic_rows_kernel(MosaicGeom g, MosaicRows r, DrawAtlas atlas, const uint8_t* __restrict__ palette,
                                   int npal, const uint8_t* __restrict__ names,
                                   const int32_t* __restrict__ name_off, int nc, int nrec,
                                   int32_t* __restrict__ recs) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nrec) return;
  int32_t* rec = recs + (size_t)j * REC;
  float d[6];
  int tile = -1;
  float mx = 1.0f, my = 1.0f;   // applied when mul
  bool mul = r.scaled;
  if (PRED) {
    const int i = j / r.max_det, row = j - i * r.max_det;
    const float* s = r.det + ((size_t)i * r.max_det + row) * 6;
    if (row < min(max(r.count[i], 0), r.max_det) && s[4] > 0.25f) {
      tile = i;
      for (int k = 0; k < 6; ++k) d[k] = s[k];
      mx = my = r.sf;
    }
  } else {
    for (int i = 0; i < g.n && tile < 0; ++i) {
      const int lo = min(max(r.label_off[i], 0), r.L), hi = min(max(r.label_off[i + 1], 0), r.L);
      if (j >= lo && j < hi) tile = i;
    }
    if (tile >= 0) {
      const float* s = r.targets + (size_t)j * 6;
      const float hw = __fmul_rn(s[4], 0.5f), hh = __fmul_rn(s[5], 0.5f);   // w / 2, h / 2
      d[0] = __fsub_rn(s[2], hw); d[1] = __fsub_rn(s[3], hh);
      d[2] = __fadd_rn(s[2], hw); d[3] = __fadd_rn(s[3], hh);
      d[4] = 1.0f; d[5] = s[1];
      if (r.normalized) {
        mul = true; mx = (float)g.tile_w; my = (float)g.tile_h;
      } else {
        mx = my = r.sf;
      }
    }
  }
  if (tile < 0) {
    draw_empty_record(rec);
    return;
  }
  const float bx = (float)(g.tile_w * (tile / g.ns)), by = (float)(g.tile_h * (tile % g.ns));
  if (mul) {
    d[0] = __fmul_rn(d[0], mx); d[1] = __fmul_rn(d[1], my);
    d[2] = __fmul_rn(d[2], mx); d[3] = __fmul_rn(d[3], my);
  }
  d[0] = __fadd_rn(d[0], bx); d[1] = __fadd_rn(d[1], by);
  d[2] = __fadd_rn(d[2], bx); d[3] = __fadd_rn(d[3], by);
  draw_make_record<PRED ? LABEL_CONF1 : LABEL_NAME>(d, MOSAIC_THICKNESS, atlas, palette, npal, names, name_off, nc,
                                                    rec);
}

template <bool PRED>
__global__ __launch_bounds__(THREADS) void mosaic_pixels_kernel(MosaicGeom g, DrawAtlas atlas, int nrec,
                                                                const int32_t* __restrict__ recs,
                                                                const uint8_t* __restrict__ names,
                                                                const int32_t* __restrict__ name_off,
                                                                uint8_t* __restrict__ canvas) {
  draw_tile_pixels<PRED ? LABEL_CONF1 : LABEL_NAME>(canvas, g.ns * g.tile_h, g.ns * g.tile_w, MOSAIC_THICKNESS, atlas,
                                                    blockIdx.x * TW, blockIdx.y * TH, nrec, recs, 0, names, name_off);
}

struct MosaicCaptions {
  const uint8_t* bytes;     // null: no captions
  const int32_t* off;
  int nbytes;
};

// canvas pixel (x, y) after the captions (d) and the borders (e)
__device__ __forceinline__ void finished_pixel(const MosaicGeom& g, const MosaicCaptions& cap, const DrawAtlas& a,
                                               const uint8_t* __restrict__ canvas, int Ws, int x, int y, int v[3]) {
  const uint8_t* p = canvas + ((size_t)y * Ws + x) * 3;
  v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
  bool white = false;
  for (int i = 0; i < g.n; ++i) {
    const int X0 = g.tile_w * (i / g.ns), Y0 = g.tile_h * (i % g.ns), X1 = X0 + g.tile_w, Y1 = Y0 + g.tile_h;
    const bool on_x = abs(x - X0) <= 1 || abs(x - X1) <= 1, on_y = abs(y - Y0) <= 1 || abs(y - Y1) <= 1;
    white = white || (on_x && y >= Y0 - 1 && y <= Y1 + 1) || (on_y && x >= X0 - 1 && x <= X1 + 1);
    const int gy = y - (Y0 + 5);
    int dx = x - (X0 + 5);
    if (white || !cap.bytes || gy < 0 || gy >= a.cell_h || dx < 0) continue;
    const int lo = min(max(cap.off[i], 0), cap.nbytes), hi = min(max(cap.off[i + 1], 0), cap.nbytes);
    for (int k = lo; k < hi; ++k) {
      const int gl = glyph_index(cap.bytes[k]);
      const int adv = max(a.metrics[2 * gl + 1], 0);
      if (dx < adv) {
        const int col = min(max(a.metrics[2 * gl] + dx, 0), a.total_w - 1);
        const int cov = a.cover[(size_t)gy * a.total_w + col];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (cov * 220 + (255 - cov) * v[c] + 127) / 255;
        break;
      }
      dx -= adv;
    }
  }
  if (white) v[0] = v[1] = v[2] = 255;
}

__global__ void mosaic_output_kernel(MosaicGeom g, MosaicCaptions cap, DrawAtlas atlas,
                                     const uint8_t* __restrict__ canvas, int Hd, int Wd, uint8_t* __restrict__ out) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x, Y = blockIdx.y;
  if (X >= Wd) return;
  const int Ws = g.ns * g.tile_w, Hs = g.ns * g.tile_h;
  uint8_t* o = out + ((size_t)Y * Wd + X) * 3;
  int v[3];
  if (Ws == Wd && Hs == Hd) {
    finished_pixel(g, cap, atlas, canvas, Ws, X, Y, v);
    o[0] = (uint8_t)v[0]; o[1] = (uint8_t)v[1]; o[2] = (uint8_t)v[2];
    return;
  }
  // sides <= MOSAIC_MAX_SIDE = 2^14: X * Ws < 2^28, a row's sum <= 255 * Ws < 2^22, the whole <= 255 * 2^28
  const int xl = X * Ws, xr = xl + Ws, yl = Y * Hs, yr = yl + Hs;   // the output pixel's span, in units of 1 / Wd
  uint64_t acc[3] = {0, 0, 0};
  for (int y = yl / Hd; y * Hd < yr; ++y) {
    const int wy = min(yr, (y + 1) * Hd) - max(yl, y * Hd);
    uint32_t row[3] = {0, 0, 0};
    for (int x = xl / Wd; x * Wd < xr; ++x) {
      const int wx = min(xr, (x + 1) * Wd) - max(xl, x * Wd);
      finished_pixel(g, cap, atlas, canvas, Ws, x, y, v);
#pragma unroll
      for (int c = 0; c < 3; ++c) row[c] += (uint32_t)(wx * v[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += (uint64_t)wy * row[c];
  }
  const uint64_t area = (uint64_t)Ws * Hs;
#pragma unroll
  for (int c = 0; c < 3; ++c) o[c] = (uint8_t)((acc[c] + area / 2) / area);
}

size_t records_bytes(int nrec) { return ((size_t)nrec * REC * sizeof(int32_t) + 15) / 16 * 16; }

}  // namespace

int mosaic_records(const MosaicArgs& a) { return a.det ? a.g.n * a.max_det : a.label_off ? a.L : 0; }

size_t mosaic_ws_bytes(const MosaicArgs& a) {
  return records_bytes(mosaic_records(a)) + (size_t)a.g.ns * a.g.tile_h * a.g.ns * a.g.tile_w * 3;
}

hipError_t launch_mosaic(const MosaicArgs& a, uint8_t* out, void* ws, hipStream_t st) {
  const MosaicGeom& g = a.g;
  const int Ws = g.ns * g.tile_w, Hs = g.ns * g.tile_h;
  const int nrec = mosaic_records(a);
  int32_t* recs = reinterpret_cast<int32_t*>(ws);
  uint8_t* canvas = reinterpret_cast<uint8_t*>(ws) + records_bytes(nrec);
  DrawAtlas atlas = a.atlas;

  const int mode = resize_mode(a.H, a.W, g.tile_h, g.tile_w);
  const double sx = resize_scale(a.W, g.tile_w), sy = resize_scale(a.H, g.tile_h);
  const dim3 tgrid((Ws + 127) / 128, Hs);
  if (a.in_kind == 0)
    hipLaunchKernelGGL(mosaic_tiles_kernel<0>, tgrid, dim3(128), 0, st, g, a.images, a.H, a.W, mode, sx, sy, canvas);
  else if (a.in_kind == 1)
    hipLaunchKernelGGL(mosaic_tiles_kernel<1>, tgrid, dim3(128), 0, st, g, a.images, a.H, a.W, mode, sx, sy, canvas);
  else
    hipLaunchKernelGGL(mosaic_tiles_kernel<2>, tgrid, dim3(128), 0, st, g, a.images, a.H, a.W, mode, sx, sy, canvas);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;

  if (nrec > 0) {
    const MosaicRows r{a.det, a.count, a.targets, a.label_off, a.max_det, a.L, a.normalized, a.sf < 1.0, (float)a.sf};
    const dim3 rgrid((nrec + 127) / 128), pgrid((Ws + TW - 1) / TW, (Hs + TH - 1) / TH);
    if (a.det) {
      hipLaunchKernelGGL(mosaic_rows_kernel<true>, rgrid, dim3(128), 0, st, g, r, atlas, a.palette, a.npal, a.names,
                         a.name_off, a.nc, nrec, recs);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      hipLaunchKernelGGL(mosaic_pixels_kernel<true>, pgrid, dim3(THREADS), 0, st, g, atlas, nrec, recs, a.names,
                         a.name_off, canvas);
    } else {
      hipLaunchKernelGGL(mosaic_rows_kernel<false>, rgrid, dim3(128), 0, st, g, r, atlas, a.palette, a.npal, a.names,
                         a.name_off, a.nc, nrec, recs);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      hipLaunchKernelGGL(mosaic_pixels_kernel<false>, pgrid, dim3(THREADS), 0, st, g, atlas, nrec, recs, a.names,
                         a.name_off, canvas);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }

  const MosaicCaptions cap{a.captions, a.cap_off, a.cap_bytes};
  hipLaunchKernelGGL(mosaic_output_kernel, dim3((a.out_w + 127) / 128, a.out_h), dim3(128), 0, st, g, cap, atlas, canvas,
                     a.out_h, a.out_w, out);
  return hipGetLastError();
}

}  // namespace yv7
