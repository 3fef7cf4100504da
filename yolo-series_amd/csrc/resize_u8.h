// The 8-bit resize of the letterbox (cv2.resize INTER_LINEAR restated bit for bit, oracle/letterbox_ref.py
// resize_linear_u8), as device functions: preprocess.hip's kernels and the mosaic's tiles (mosaic.hip) share them.
// Fixed-point coefficients with 11 fractional bits from the same float/double arithmetic as resize.cpp, an
// exact-int32 horizontal pass and the SIMD vertical pass's rounding; an exact 2x downscale takes cv2's INTER_AREA
// fast path (rounded 2 x 2 mean).  The source is reached through fetch(row, column, channel) -> 0..255, so it
// may be packed HWC bytes or planes of another type.
#ifndef YV7_RESIZE_U8_H
#define YV7_RESIZE_U8_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace yv7 {

constexpr int RESIZE_COEF = 2048;   // INTER_RESIZE_COEF_SCALE
constexpr int RESIZE_SIMD_LANES = 16;

enum { RESIZE_IDENTITY = 0, RESIZE_LINEAR = 1, RESIZE_AREA2X = 2 };

__host__ __device__ inline int resize_mode(int H, int W, int nh, int nw) {
  if (nh == H && nw == W) return RESIZE_IDENTITY;
  if (W == 2 * nw && H == 2 * nh) return RESIZE_AREA2X;
  return RESIZE_LINEAR;
}

__host__ __device__ inline double resize_scale(int src, int dst) { return 1.0 / ((double)dst / src); }

__device__ __forceinline__ int cv_round(float v) { return (int)rintf(v); }   // cvRound: half to even

struct ResizeTap {
  int i0, i1;   // the two source indices, clamped
  int c0, c1;   // their coefficients
};

// columns: (sx, fx) reset at the borders (resize.cpp, resizeGeneric_ setup)
__device__ __forceinline__ ResizeTap resize_col_tap(int x, double scale, int W) {
  float f = (float)((x + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { s = 0; f = 0.f; }
  if (s >= W - 1) { s = W - 1; f = 0.f; }
  return {s, min(s + 1, W - 1), cv_round((1.f - f) * (float)RESIZE_COEF), cv_round(f * (float)RESIZE_COEF)};
}

// rows: fy kept, fetched rows clamped
__device__ __forceinline__ ResizeTap resize_row_tap(int y, double scale, int H) {
  float f = (float)((y + 0.5) * scale - 0.5);
  const int s = (int)floorf(f);
  f -= (float)s;
  return {min(max(s, 0), H - 1), min(max(s + 1, 0), H - 1), cv_round((1.f - f) * (float)RESIZE_COEF),
          cv_round(f * (float)RESIZE_COEF)};
}

// the vertical pass on two horizontal sums; pos: the value's position in its destination row (x * 3 + c), nw: the
// destination width.  The positions the SIMD vertical pass covers round in two steps, the row's tail in one.
__device__ __forceinline__ int resize_vertical(int d0, int d1, int b0, int b1, int pos, int nw) {
  const int nv = nw * 3 / RESIZE_SIMD_LANES * RESIZE_SIMD_LANES;
  int o;
  if (pos < nv) o = ((((d0 >> 4) * b0) >> 16) + (((d1 >> 4) * b1) >> 16) + 2) >> 2;
  else o = (d0 * b0 + d1 * b1 + (1 << 21)) >> 22;
  return min(max(o, 0), 255);
}

// ---- cn interleaved channels (preprocess.hip's channel-count kernels).  The SIMD pass runs over the interleaved
// destination row of nw * cn values, so the split is at resize_split(nw, cn) of pos = x * cn + c: neither the
// 3-channel split nor a per-plane one (nw / 16 * 16) holds for another count.
__host__ __device__ inline int resize_split(int nw, int cn) { return nw * cn / RESIZE_SIMD_LANES * RESIZE_SIMD_LANES; }

__device__ __forceinline__ int resize_vertical_at(int d0, int d1, int b0, int b1, int pos, int nv) {
  int o;
  if (pos < nv) o = ((((d0 >> 4) * b0) >> 16) + (((d1 >> 4) * b1) >> 16) + 2) >> 2;
  else o = (d0 * b0 + d1 * b1 + (1 << 21)) >> 22;
  return min(max(o, 0), 255);
}

// channel c of destination pixel (x, y) of an H x W x cn packed source: one value, so a caller's channel loop
// holds the fetches, the vertical pass and the store of one channel at a time.  The taps are the pixel's and are
// read in the bilinear mode only.
__device__ __forceinline__ int resize_value_cn(const uint8_t* __restrict__ img, int W, int cn, int mode,
                                               const ResizeTap& cx, const ResizeTap& cy, int x, int y, int c, int nv) {
  const auto fetch = [img, W, cn, c](int yy, int xx) -> int { return img[((size_t)yy * W + xx) * cn + c]; };
  if (mode == RESIZE_IDENTITY) return fetch(y, x);
  if (mode == RESIZE_AREA2X)
    return (fetch(2 * y, 2 * x) + fetch(2 * y, 2 * x + 1) + fetch(2 * y + 1, 2 * x) + fetch(2 * y + 1, 2 * x + 1) + 2) >> 2;
  const int d0 = fetch(cy.i0, cx.i0) * cx.c0 + fetch(cy.i0, cx.i1) * cx.c1;
  const int d1 = fetch(cy.i1, cx.i0) * cx.c0 + fetch(cy.i1, cx.i1) * cx.c1;
  return resize_vertical_at(d0, d1, cy.c0, cy.c1, x * cn + c, nv);
}

// destination pixel (x, y) of a bilinear resize with the taps cx, cy
template <class Fetch>
__device__ __forceinline__ void resize_linear_px(Fetch fetch, const ResizeTap& cx, const ResizeTap& cy, int x, int nw,
                                                 int v[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int d0 = fetch(cy.i0, cx.i0, c) * cx.c0 + fetch(cy.i0, cx.i1, c) * cx.c1;
    const int d1 = fetch(cy.i1, cx.i0, c) * cx.c0 + fetch(cy.i1, cx.i1, c) * cx.c1;
    v[c] = resize_vertical(d0, d1, cy.c0, cy.c1, x * 3 + c, nw);
  }
}

// destination pixel (x, y) of an exact 2x downscale
template <class Fetch>
__device__ __forceinline__ void resize_area2x_px(Fetch fetch, int x, int y, int v[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)
    v[c] = (fetch(2 * y, 2 * x, c) + fetch(2 * y, 2 * x + 1, c) + fetch(2 * y + 1, 2 * x, c) +
            fetch(2 * y + 1, 2 * x + 1, c) + 2) >> 2;
}

// destination pixel (x, y) of an H x W source resized to nh x nw by mode (resize_mode), scales from resize_scale
template <class Fetch>
__device__ __forceinline__ void resize_px(Fetch fetch, int mode, int H, int W, int nw, double sx, double sy, int x,
                                          int y, int v[3]) {
  if (mode == RESIZE_IDENTITY) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = fetch(y, x, c);
  } else if (mode == RESIZE_AREA2X) {
    resize_area2x_px(fetch, x, y, v);
  } else {
    resize_linear_px(fetch, resize_col_tap(x, sx, W), resize_row_tap(y, sy, H), x, nw, v);
  }
}

}  // namespace yv7

#endif  // YV7_RESIZE_U8_H
