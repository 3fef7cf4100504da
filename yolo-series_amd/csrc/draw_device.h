// The record and pixel code of the drawing contract (include/yv7.h), shared by draw.hip (yv7_draw_boxes: one image
// per row list) and mosaic.hip (yv7_mosaic: every tile's rows on one picture).
//
//   draw_make_record  one det row (x1, y1, x2, y2, conf, class) becomes a 12-int record: the bounding rectangle of
//                     everything it paints, the sorted corners, the label's width, the colour, the class and the
//                     confidence's digits.  A skipped row gets an empty bounding rectangle.
//   draw_tile_pixels  one block per TW x TH tile of one image.  The block tests the image's records against its
//                     tile 256 at a time, from the last drawn to the first, and keeps the hits in LDS in that
//                     order (wave ballots, so the order does not depend on timing); with no hit it goes on to the
//                     next 256 or leaves.  Each thread owns TH / 4 pixels of one column and walks the hits until
//                     one covers the pixel: within a row text is over the background over the outline, so the
//                     first cover found is the colour painter's order leaves.  Only covered pixels are stored.
//
// The label's text is a compile-time mode: "name d.dd" (yv7_draw_boxes), "name d.d" and "name" (the mosaic's
// predictions and labels).
#ifndef YV7_DRAW_DEVICE_H
#define YV7_DRAW_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yv7_kernels.h"

namespace yv7 {
namespace drawdev {

constexpr int TW = DRAW_TILE_W, TH = DRAW_TILE_H;
constexpr int THREADS = 256;
constexpr int ROWS_PER_THREAD = TH / (THREADS / TW);
constexpr int REC = 12;             // int32 per record
constexpr int LIM = 1 << 28;        // coordinates are clamped here: far outside any image, far from overflow
static_assert(TW == 64 && THREADS % TW == 0 && TH % (THREADS / TW) == 0, "one wave per tile row");

enum { R_BX0, R_BY0, R_BX1, R_BY1, R_XA, R_YA, R_XB, R_YB, R_TW, R_COLOUR, R_CLS, R_N };
enum { LABEL_CONF2 = 0, LABEL_CONF1 = 1, LABEL_NAME = 2 };   // "name d.dd", "name d.d", "name"

__device__ __forceinline__ int trunc_clamped(float v) {   // Python's int() on a finite float, clamped to +-LIM
  return (int)fminf(fmaxf(v, -(float)LIM), (float)LIM);
}

__device__ __forceinline__ int glyph_index(int byte) {    // ASCII 32..126 -> 0..94, anything else draws as '?'
  return (byte >= 32 && byte <= 126) ? byte - 32 : '?' - 32;
}

template <int MODE>
__device__ __forceinline__ int label_extra() {   // the bytes after the name
  return MODE == LABEL_CONF2 ? 5 : MODE == LABEL_CONF1 ? 4 : 0;
}

// the confidence's digits: f'{conf:.2f}' / '%.1f' % conf; an fp32 times 100 (10) is exact in double, rint is
// round-half-even
template <int MODE>
__device__ __forceinline__ int label_digits(float conf) {
  if (MODE == LABEL_CONF2) return (int)fmin(fmax(rint((double)conf * 100.0), 0.0), 100.0);
  if (MODE == LABEL_CONF1) return (int)fmin(fmax(rint((double)conf * 10.0), 0.0), 10.0);
  return 0;
}

// byte k of the label; k in [0, len + label_extra<MODE>())
template <int MODE>
__device__ __forceinline__ int label_byte(const uint8_t* __restrict__ name, int len, int n, int k) {
  if (k < len) return name[k];
  if (MODE == LABEL_CONF2) {
    switch (k - len) {
      case 0: return ' ';
      case 1: return '0' + n / 100;
      case 2: return '.';
      case 3: return '0' + (n / 10) % 10;
      default: return '0' + n % 10;
    }
  }
  switch (k - len) {   // LABEL_CONF1; LABEL_NAME never gets here
    case 0: return ' ';
    case 1: return '0' + n / 10;
    case 2: return '.';
    default: return '0' + n % 10;
  }
}

__device__ __forceinline__ void draw_empty_record(int32_t* __restrict__ rec) {
  rec[R_BX0] = 1; rec[R_BY0] = 1; rec[R_BX1] = 0; rec[R_BY1] = 0;
}

// d: the row's six values; t: the line thickness; a: the atlas of the image's labels (read only with names).
template <int MODE>
__device__ __forceinline__ void draw_make_record(const float* __restrict__ d, int t, const DrawAtlas& a,
                                                 const uint8_t* __restrict__ palette, int npal,
                                                 const uint8_t* __restrict__ names,
                                                 const int32_t* __restrict__ name_off, int nc,
                                                 int32_t* __restrict__ rec) {
  bool ok = true;
  for (int k = 0; k < 6; ++k) ok = ok && isfinite(d[k]);
  if (!ok || d[5] < 0.f) {
    draw_empty_record(rec);
    return;
  }
  const int x1 = trunc_clamped(d[0]), y1 = trunc_clamped(d[1]), x2 = trunc_clamped(d[2]), y2 = trunc_clamped(d[3]);
  const int xa = min(x1, x2), xb = max(x1, x2), ya = min(y1, y2), yb = max(y1, y2);
  const int cls = trunc_clamped(d[5]);
  const int lo = t / 2;
  int bx0 = xa - lo, by0 = ya - lo, bx1 = xb - lo + t - 1, by1 = yb - lo + t - 1;
  int tw = -1;   // no label
  int n = 0;
  if (names && cls < nc) {
    n = label_digits<MODE>(d[4]);
    const int o0 = name_off[cls], len = max(name_off[cls + 1] - o0, 0);
    tw = 0;
    for (int k = 0; k < len + label_extra<MODE>(); ++k) {
      const int adv = a.metrics[2 * glyph_index(label_byte<MODE>(names + o0, len, n, k)) + 1];
      tw = min(tw + max(adv, 0), LIM);
    }
    bx0 = min(bx0, xa); bx1 = max(bx1, xa + tw);
    by0 = min(by0, ya - a.cell_h - 3); by1 = max(by1, ya);
  }
  const uint8_t* c = palette + 3 * (cls % npal);
  rec[R_BX0] = bx0; rec[R_BY0] = by0; rec[R_BX1] = bx1; rec[R_BY1] = by1;
  rec[R_XA] = xa; rec[R_YA] = ya; rec[R_XB] = xb; rec[R_YB] = yb;
  rec[R_TW] = tw; rec[R_COLOUR] = c[0] | (c[1] << 8) | (c[2] << 16); rec[R_CLS] = cls; rec[R_N] = n;
}

// The block's tile starts at (tx0, ty0) of the image data [h][w][3]; recs holds cnt records in row order, drawn
// 0 .. cnt - 1 (reverse: cnt - 1 .. 0).  Every thread of the block must call it (block-wide barriers); cnt is
// uniform.
template <int MODE>
__device__ __forceinline__ void draw_tile_pixels(uint8_t* __restrict__ data, int h, int w, int t, const DrawAtlas& a,
                                                 int tx0, int ty0, int cnt, const int32_t* __restrict__ recs,
                                                 int reverse, const uint8_t* __restrict__ names,
                                                 const int32_t* __restrict__ name_off) {
  const int tx1 = min(tx0 + TW, w) - 1, ty1 = min(ty0 + TH, h) - 1;   // inclusive

  __shared__ int32_t s_rec[THREADS][REC];
  __shared__ int s_wave[THREADS / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = tx0 + lane;
  const int lo = t / 2;
  const int th = a.cell_h;
  uint32_t todo = 0;   // bit j: pixel (x, ty0 + wave + 4 j) is inside the image and not yet decided
  for (int j = 0; j < ROWS_PER_THREAD; ++j)
    if (x <= tx1 && ty0 + wave + (THREADS / TW) * j <= ty1) todo |= 1u << j;

  for (int base = 0; base < cnt; base += THREADS) {
    // draw index, from the last drawn down; thread i of this round tests draw index cnt - 1 - (base + i)
    const int di = cnt - 1 - (base + tid);
    const int row = reverse ? cnt - 1 - di : di;
    bool hit = false;
    if (di >= 0) {
      const int4 bb = *reinterpret_cast<const int4*>(recs + (size_t)row * REC);
      hit = bb.x <= tx1 && bb.z >= tx0 && bb.y <= ty1 && bb.w >= ty0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int k = 0; k < THREADS / 64; ++k) {
      if (k < wave) before += s_wave[k];
      total += s_wave[k];
    }
    if (total == 0) {       // uniform: most tiles
      __syncthreads();      // s_wave is rewritten in the next round
      continue;
    }
    if (hit) {
      const int slot = before + __popcll(m & ((1ull << lane) - 1ull));
      const int32_t* r = recs + (size_t)row * REC;
      for (int k = 0; k < REC; ++k) s_rec[slot][k] = r[k];
    }
    __syncthreads();

    for (int j = 0; j < ROWS_PER_THREAD; ++j) {
      if (!(todo >> j & 1u)) continue;
      const int y = ty0 + wave + (THREADS / TW) * j;
      for (int i = 0; i < total; ++i) {
        const int32_t* r = s_rec[i];
        if (x < r[R_BX0] || x > r[R_BX1] || y < r[R_BY0] || y > r[R_BY1]) continue;
        const int xa = r[R_XA], ya = r[R_YA], xb = r[R_XB], yb = r[R_YB], tw = r[R_TW];
        const uint32_t colour = (uint32_t)r[R_COLOUR];
        int c0 = colour & 255, c1 = colour >> 8 & 255, c2 = colour >> 16 & 255;
        bool covered = false;
        if (tw >= 0 && x >= xa && x <= xa + tw && y >= ya - th - 3 && y <= ya) {
          covered = true;   // the label's background, and inside it the glyph cells
          int dx = x - xa;
          const int gy = y - (ya - 1 - th);
          if (dx < tw && gy >= 0 && gy < th) {
            const int o0 = name_off[r[R_CLS]], len = max(name_off[r[R_CLS] + 1] - o0, 0);
            for (int k = 0; k < len + label_extra<MODE>(); ++k) {
              const int g = glyph_index(label_byte<MODE>(names + o0, len, r[R_N], k));
              const int adv = max(a.metrics[2 * g + 1], 0);
              if (dx < adv) {
                const int col = min(max(a.metrics[2 * g] + dx, 0), a.total_w - 1);
                const int cov = a.cover[(size_t)gy * a.total_w + col];
                c0 = (cov * 225 + (255 - cov) * c0 + 127) / 255;
                c1 = (cov * 255 + (255 - cov) * c1 + 127) / 255;
                c2 = (cov * 255 + (255 - cov) * c2 + 127) / 255;
                break;
              }
              dx -= adv;
            }
          }
        } else if (x >= xa - lo && x <= xb - lo + t - 1 && y >= ya - lo && y <= yb - lo + t - 1) {
          const bool on_x = (x >= xa - lo && x <= xa - lo + t - 1) || (x >= xb - lo && x <= xb - lo + t - 1);
          const bool on_y = (y >= ya - lo && y <= ya - lo + t - 1) || (y >= yb - lo && y <= yb - lo + t - 1);
          covered = on_x || on_y;
        }
        if (covered) {
          uint8_t* p = data + ((size_t)y * w + x) * 3;
          p[0] = (uint8_t)c0; p[1] = (uint8_t)c1; p[2] = (uint8_t)c2;
          todo &= ~(1u << j);
          break;
        }
      }
    }
    __syncthreads();   // s_rec and s_wave are rewritten in the next round
  }
}

}  // namespace drawdev
}  // namespace yv7

#endif  // YV7_DRAW_DEVICE_H
