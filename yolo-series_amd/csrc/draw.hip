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
//   draw_prep_kernel   one thread per (image, row < count): the row becomes a 12-int record in the workspace:
//                      the bounding rectangle of everything it paints, the sorted corners, the label's width,
//                      the colour, the class and the confidence's three digits.  A skipped row gets an empty
//                      bounding rectangle.
//   draw_pixels_kernel one block per TW x TH tile of one image.  The block tests the image's records against
//                      its tile 256 at a time, from the last drawn to the first, and keeps the hits in LDS in that
//                      order (wave ballots, so the order does not depend on timing); with no hit it goes on to the
//                      next 256 or leaves.  Each thread owns TH / 4 pixels of one column and walks the hits until
//                      one covers the pixel: within a row text is over the background over the outline, so the
//                      first cover found is the colour painter's order leaves.  Only covered pixels are stored.
//
// One thread decides each pixel, so the result cannot depend on the order in which threads run, and overlapping
// boxes need no atomics.  Rows are packed and w may be odd: bytes are stored one by one.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "yv7_kernels.h"

namespace yv7 {

namespace {

constexpr int TW = DRAW_TILE_W, TH = DRAW_TILE_H;
constexpr int THREADS = 256;
constexpr int ROWS_PER_THREAD = TH / (THREADS / TW);
constexpr int REC = 12;             // int32 per record
constexpr int LIM = 1 << 28;        // coordinates are clamped here: far outside any image, far from overflow
static_assert(TW == 64 && THREADS % TW == 0 && TH % (THREADS / TW) == 0, "one wave per tile row");

enum { R_BX0, R_BY0, R_BX1, R_BY1, R_XA, R_YA, R_XB, R_YB, R_TW, R_COLOUR, R_CLS, R_N };

struct DrawChunk {
  DrawImage im[RAGGED_CHUNK];
};

struct DrawAtlases {
  DrawAtlas a[DRAW_MAX_ATLAS];
};

__device__ __forceinline__ int trunc_clamped(float v) {   // Python's int() on a finite float, clamped to +-LIM
  return (int)fminf(fmaxf(v, -(float)LIM), (float)LIM);
}

__device__ __forceinline__ int glyph_index(int byte) {    // ASCII 32..126 -> 0..94, anything else draws as '?'
  return (byte >= 32 && byte <= 126) ? byte - 32 : '?' - 32;
}

// byte k of the label "name + ' ' + d.dd"; k in [0, len + 5)
__device__ __forceinline__ int label_byte(const uint8_t* __restrict__ name, int len, int n, int k) {
  if (k < len) return name[k];
  switch (k - len) {
    case 0: return ' ';
    case 1: return '0' + n / 100;
    case 2: return '.';
    case 3: return '0' + (n / 10) % 10;
    default: return '0' + n % 10;
  }
}

__global__ void draw_prep_kernel(DrawChunk ch, DrawAtlases at, int b0, const float* __restrict__ det,
                                 const int32_t* __restrict__ count, int max_det, const uint8_t* __restrict__ palette,
                                 int npal, const uint8_t* __restrict__ names, const int32_t* __restrict__ name_off,
                                 int nc, int32_t* __restrict__ ws) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = b0 + blockIdx.y;
  const int cnt = min(max(count[b], 0), max_det);
  if (row >= cnt) return;   // never read
  const DrawImage& im = ch.im[blockIdx.y];
  const float* d = det + ((size_t)b * max_det + row) * 6;
  int32_t* rec = ws + ((size_t)b * max_det + row) * REC;
  bool ok = true;
  for (int k = 0; k < 6; ++k) ok = ok && isfinite(d[k]);
  if (!ok || d[5] < 0.f) {
    rec[R_BX0] = 1; rec[R_BY0] = 1; rec[R_BX1] = 0; rec[R_BY1] = 0;
    return;
  }
  const int x1 = trunc_clamped(d[0]), y1 = trunc_clamped(d[1]), x2 = trunc_clamped(d[2]), y2 = trunc_clamped(d[3]);
  const int xa = min(x1, x2), xb = max(x1, x2), ya = min(y1, y2), yb = max(y1, y2);
  const int cls = trunc_clamped(d[5]);
  const int t = im.t, lo = t / 2;
  int bx0 = xa - lo, by0 = ya - lo, bx1 = xb - lo + t - 1, by1 = yb - lo + t - 1;
  int tw = -1;   // no label
  int n = 0;
  if (names && cls < nc) {
    // f'{conf:.2f}': an fp32 times 100 is exact in double, rint is round-half-even
    n = (int)fmin(fmax(rint((double)d[4] * 100.0), 0.0), 100.0);
    const DrawAtlas& a = at.a[im.atlas];
    const int o0 = name_off[cls], len = max(name_off[cls + 1] - o0, 0);
    tw = 0;
    for (int k = 0; k < len + 5; ++k) {
      const int adv = a.metrics[2 * glyph_index(label_byte(names + o0, len, n, k)) + 1];
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

__global__ __launch_bounds__(THREADS) void draw_pixels_kernel(
    DrawChunk ch, DrawAtlases at, int b0, const int32_t* __restrict__ count, int max_det,
    const uint8_t* __restrict__ names, const int32_t* __restrict__ name_off, int reverse,
    const int32_t* __restrict__ ws) {
  const DrawImage& im = ch.im[blockIdx.z];
  const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
  if (tx0 >= im.w || ty0 >= im.h) return;   // the grid is the chunk's largest image
  const int b = b0 + blockIdx.z;
  const int cnt = min(max(count[b], 0), max_det);
  const int tx1 = min(tx0 + TW, im.w) - 1, ty1 = min(ty0 + TH, im.h) - 1;   // inclusive
  const int32_t* recs = ws + (size_t)b * max_det * REC;

  __shared__ int32_t s_rec[THREADS][REC];
  __shared__ int s_wave[THREADS / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = tx0 + lane;
  const int t = im.t, lo = t / 2;
  const DrawAtlas& a = at.a[im.atlas];
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
            for (int k = 0; k < len + 5; ++k) {
              const int g = glyph_index(label_byte(names + o0, len, r[R_N], k));
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
          uint8_t* p = im.data + ((size_t)y * im.w + x) * 3;
          p[0] = (uint8_t)c0; p[1] = (uint8_t)c1; p[2] = (uint8_t)c2;
          todo &= ~(1u << j);
          break;
        }
      }
    }
    __syncthreads();   // s_rec and s_wave are rewritten in the next round
  }
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
