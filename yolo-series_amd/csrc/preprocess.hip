// Frame pre-processing on the GPU (gfx950): letterbox = cv2.resize(INTER_LINEAR) + constant border,
// optionally fused with detect.py's input conversion (BGR -> RGB, HWC -> CHW, /255, half/float).
//
// Replaces utils/datasets.py:1277-1307 (letterbox; cv2.resize at :1302, cv2.copyMakeBorder at :1305)
// and detect.py:100-104 / datasets.py:199 (img[:, :, ::-1].transpose(2, 0, 1), .half()/.float(),
// /= 255).  The resize restates OpenCV's generic 8-bit bilinear path bit for bit (see
// oracle/letterbox_ref.py for the algorithm and its parity status): fixed-point coefficient tables
// (11 fractional bits) computed once per shape by a small kernel with the same float/double
// arithmetic as resize.cpp, an exact-int32 horizontal pass and the SIMD vertical pass's rounding;
// an exact 2x downscale takes cv2's INTER_AREA fast path (rounded 2 x 2 mean), as cv2 does.
//
// One thread per output pixel (3 channels); a batch of B frames of one size in one launch.  Input:
// uint8 [B][H][W][3] BGR (packed rows).  Outputs: uint8 [B][oh][ow][3] BGR (the letterboxed frame,
// letterbox()'s return), or fp16 / fp32 [B][3][oh][ow] RGB in [0, 1] (the model input).
// letterbox_ragged_kernel does the same for B frames of B different sizes, each with its own geometry.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "resize_u8.h"
#include "yv7_kernels.h"

namespace yv7 {

namespace {

// tables: per destination column / row, the two source indices (clamped) and two coefficients
struct LbTab {
  int* x0;
  int* x1;
  int* ca0;
  int* ca1;
  int* y0;
  int* y1;
  int* cb0;
  int* cb1;
};

__global__ void lb_tables_kernel(LbTab t, int H, int W, int nh, int nw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nw) {
    const ResizeTap c = resize_col_tap(i, resize_scale(W, nw), W);
    t.x0[i] = c.i0; t.x1[i] = c.i1; t.ca0[i] = c.c0; t.ca1[i] = c.c1;
  } else if (i < nw + nh) {
    const int r = i - nw;
    const ResizeTap c = resize_row_tap(r, resize_scale(H, nh), H);
    t.y0[r] = c.i0; t.y1[r] = c.i1; t.cb0[r] = c.c0; t.cb1[r] = c.c1;
  }
}

// mode: resize_mode(); the bilinear one reads the tables
template <int OUT>
__global__ void letterbox_kernel(const uint8_t* __restrict__ src, int H, int W, int nh, int nw, int top, int left,
                                 int oh, int ow, uint8_t pb, uint8_t pg, uint8_t pr, int mode, LbTab t,
                                 void* __restrict__ dst) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x;
  const int oy = blockIdx.y;
  const int b = blockIdx.z;
  if (ox >= ow) return;
  const int y = oy - top, x = ox - left;
  int v[3];
  if ((unsigned)y < (unsigned)nh && (unsigned)x < (unsigned)nw) {
    const uint8_t* img = src + (size_t)b * H * W * 3;
    const auto fetch = [img, W](int yy, int xx, int c) -> int { return img[((size_t)yy * W + xx) * 3 + c]; };
    if (mode == RESIZE_IDENTITY) {
      v[0] = fetch(y, x, 0); v[1] = fetch(y, x, 1); v[2] = fetch(y, x, 2);
    } else if (mode == RESIZE_AREA2X) {
      resize_area2x_px(fetch, x, y, v);
    } else {   // the taps from lb_tables_kernel
      resize_linear_px(fetch, ResizeTap{t.x0[x], t.x1[x], t.ca0[x], t.ca1[x]},
                       ResizeTap{t.y0[y], t.y1[y], t.cb0[y], t.cb1[y]}, x, nw, v);
    }
  } else {
    v[0] = pb; v[1] = pg; v[2] = pr;
  }
  if constexpr (OUT == 0) {
    uint8_t* d = reinterpret_cast<uint8_t*>(dst) + (((size_t)b * oh + oy) * ow + ox) * 3;
    d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
  } else {
    // RGB planes = BGR reversed; x / 255 in float (fp16: rounded once, as torch's half division)
    const size_t plane = (size_t)oh * ow, o = (size_t)b * 3 * plane + (size_t)oy * ow + ox;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float f = (float)v[2 - c] / 255.0f;
      if constexpr (OUT == 1) reinterpret_cast<_Float16*>(dst)[o + c * plane] = (_Float16)f;
      else reinterpret_cast<float*>(dst)[o + c * plane] = f;
    }
  }
}

// ---- ragged batch: every frame its own size, geometry and resize mode (autoShape, common.py:899-918; a
// detect.py loop over a directory).  Up to RAGGED_CHUNK frame records travel by value as one kernel argument,
// so the call needs no host-to-device copy and no workspace; blockIdx.z picks the record, which makes the
// mode branch uniform per block.  The two coefficient pairs lb_tables_kernel would store are computed inline
// with the same expressions (the row pair is the same for a whole block); the host supplies each axis'
// scale = 1.0 / ((double)dst / src) as a double.
struct LbFrame {
  const uint8_t* src;
  double sx, sy;   // column / row scale
  int H, W, nh, nw, top, left, mode, reserved;
};
static_assert(sizeof(LbFrame) == 56, "LbFrame is sized for 64 records in one kernel argument");

struct LbChunk {
  LbFrame f[RAGGED_CHUNK];
};

template <int OUT>
__global__ void letterbox_ragged_kernel(LbChunk ch, int b0, int oh, int ow, uint8_t p0, uint8_t p1, uint8_t p2,
                                        int swap_rb, void* __restrict__ dst) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x;
  const int oy = blockIdx.y;
  const LbFrame& f = ch.f[blockIdx.z];
  const int b = b0 + blockIdx.z;
  if (ox >= ow) return;
  const int H = f.H, W = f.W, nw = f.nw;
  const int y = oy - f.top, x = ox - f.left;
  int v[3];
  if ((unsigned)y < (unsigned)f.nh && (unsigned)x < (unsigned)nw) {
    const uint8_t* img = f.src;
    // the taps lb_tables_kernel would store, computed inline (the row pair is the same for a whole block)
    resize_px([img, W](int yy, int xx, int c) -> int { return img[((size_t)yy * W + xx) * 3 + c]; }, f.mode, H, W,
              nw, f.sx, f.sy, x, y, v);
  } else {
    v[0] = p0; v[1] = p1; v[2] = p2;
  }
  if constexpr (OUT == 0) {
    uint8_t* d = reinterpret_cast<uint8_t*>(dst) + (((size_t)b * oh + oy) * ow + ox) * 3;
    d[0] = (uint8_t)v[0]; d[1] = (uint8_t)v[1]; d[2] = (uint8_t)v[2];
  } else {
    // planes in the input's channel order, or reversed (BGR frames -> RGB planes) with swap_rb
    const size_t plane = (size_t)oh * ow, o = (size_t)b * 3 * plane + (size_t)oy * ow + ox;
    const float f0 = (float)v[0] / 255.0f, f1 = (float)v[1] / 255.0f, f2 = (float)v[2] / 255.0f;
    const float lo = swap_rb ? f2 : f0, hi = swap_rb ? f0 : f2;
    if constexpr (OUT == 1) {
      _Float16* d = reinterpret_cast<_Float16*>(dst);
      d[o] = (_Float16)lo; d[o + plane] = (_Float16)f1; d[o + 2 * plane] = (_Float16)hi;
    } else {
      float* d = reinterpret_cast<float*>(dst);
      d[o] = lo; d[o + plane] = f1; d[o + 2 * plane] = hi;
    }
  }
}

// ---- any channel count 1..LETTERBOX_MAX_CH (grayscale, thermal, RGBA, RGB+IR frames): packed [H][W][cn] in,
// uint8 [oh][ow][cn] or float planes [cn][oh][ow] out.  CN is the count at compile time (1..4) or 0 for a
// run-time count (5..16).  One thread per output pixel as above; the pixel's taps are computed once and every
// channel's fetches, vertical pass and store sit inside the channel loop, so no per-thread array is indexed by
// a run-time value.  The pad bytes travel by value in two words, picked by shifts.
struct LbPad {
  uint64_t lo, hi;   // channels 0..7 and 8..15, channel c at bits 8 * (c & 7)
};

__device__ __forceinline__ int lb_pad(const LbPad& p, int c) {
  return (int)(((c < 8 ? p.lo : p.hi) >> ((c & 7) * 8)) & 255);
}

// pix: the pixel's index in the uint8 output, o: its offset in plane 0 of its float frame
template <int OUT, int CN>
__device__ __forceinline__ void lb_pixel_cn(bool inside, const uint8_t* __restrict__ img, int W, int cn_rt, int mode,
                                            const ResizeTap& cx, const ResizeTap& cy, int x, int y, int nw,
                                            const LbPad& pad, void* __restrict__ dst, size_t pix, size_t plane,
                                            size_t o) {
  const int cn = CN ? CN : cn_rt;
  const int nv = resize_split(nw, cn);
  uint32_t packed = 0;
#pragma clang loop unroll_count(CN ? CN : 1)
  for (int c = 0; c < cn; ++c) {
    const int v = inside ? resize_value_cn(img, W, cn, mode, cx, cy, x, y, c, nv) : lb_pad(pad, c);
    if constexpr (OUT == 0) {
      if constexpr (CN == 2 || CN == 4) packed |= (uint32_t)v << (8 * c);
      else reinterpret_cast<uint8_t*>(dst)[pix * cn + c] = (uint8_t)v;
    } else {
      // planes in the input's channel order; x / 255 in float (fp16: rounded once)
      const float f = (float)v / 255.0f;
      const size_t at = o + (size_t)c * plane;
      if constexpr (OUT == 1) reinterpret_cast<_Float16*>(dst)[at] = (_Float16)f;
      else reinterpret_cast<float*>(dst)[at] = f;
    }
  }
  if constexpr (OUT == 0 && CN == 4) reinterpret_cast<uint32_t*>(dst)[pix] = packed;
  if constexpr (OUT == 0 && CN == 2) reinterpret_cast<uint16_t*>(dst)[pix] = (uint16_t)packed;
}

template <int OUT, int CN>
__global__ void letterbox_cn_kernel(const uint8_t* __restrict__ src, int H, int W, int cn_rt, int nh, int nw, int top,
                                    int left, int oh, int ow, LbPad pad, int mode, LbTab t,
                                    void* __restrict__ dst) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x;
  const int oy = blockIdx.y;
  const int b = blockIdx.z;
  if (ox >= ow) return;
  const int cn = CN ? CN : cn_rt;
  const int y = oy - top, x = ox - left;
  const bool inside = (unsigned)y < (unsigned)nh && (unsigned)x < (unsigned)nw;
  ResizeTap cx{0, 0, 0, 0}, cy{0, 0, 0, 0};
  if (inside && mode == RESIZE_LINEAR) {   // the taps from lb_tables_kernel
    cx = ResizeTap{t.x0[x], t.x1[x], t.ca0[x], t.ca1[x]};
    cy = ResizeTap{t.y0[y], t.y1[y], t.cb0[y], t.cb1[y]};
  }
  const size_t plane = (size_t)oh * ow;
  lb_pixel_cn<OUT, CN>(inside, src + (size_t)b * H * W * cn, W, cn, mode, cx, cy, x, y, nw, pad, dst,
                       ((size_t)b * oh + oy) * ow + ox, plane, (size_t)b * cn * plane + (size_t)oy * ow + ox);
}

template <int OUT, int CN>
__global__ void letterbox_ragged_cn_kernel(LbChunk ch, int b0, int cn_rt, int oh, int ow, LbPad pad,
                                           void* __restrict__ dst) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x;
  const int oy = blockIdx.y;
  const LbFrame& f = ch.f[blockIdx.z];
  const int b = b0 + blockIdx.z;
  if (ox >= ow) return;
  const int cn = CN ? CN : cn_rt;
  const int y = oy - f.top, x = ox - f.left;
  const bool inside = (unsigned)y < (unsigned)f.nh && (unsigned)x < (unsigned)f.nw;
  ResizeTap cx{0, 0, 0, 0}, cy{0, 0, 0, 0};
  if (inside && f.mode == RESIZE_LINEAR) {   // computed inline; the row pair is the same for a whole block
    cx = resize_col_tap(x, f.sx, f.W);
    cy = resize_row_tap(y, f.sy, f.H);
  }
  const size_t plane = (size_t)oh * ow;
  lb_pixel_cn<OUT, CN>(inside, f.src, f.W, cn, f.mode, cx, cy, x, y, f.nw, pad, dst,
                       ((size_t)b * oh + oy) * ow + ox, plane, (size_t)b * cn * plane + (size_t)oy * ow + ox);
}

template <int V>
struct IntC {
  static constexpr int value = V;
};

// call(out kind, channel count) with both as compile-time constants; counts above 4 share the run-time one
template <class Call>
void lb_dispatch_cn(int out_kind, int cn, Call call) {
  const auto by_count = [&](auto out) {
    switch (cn) {
      case 1: call(out, IntC<1>{}); break;
      case 2: call(out, IntC<2>{}); break;
      case 3: call(out, IntC<3>{}); break;
      case 4: call(out, IntC<4>{}); break;
      default: call(out, IntC<0>{}); break;
    }
  };
  if (out_kind == 0) by_count(IntC<0>{});
  else if (out_kind == 1) by_count(IntC<1>{});
  else by_count(IntC<2>{});
}

LbPad lb_pack_pad(const uint8_t* pad, int cn) {
  LbPad p{0, 0};
  for (int c = 0; c < cn; ++c) (c < 8 ? p.lo : p.hi) |= (uint64_t)pad[c] << ((c & 7) * 8);
  return p;
}

LbChunk lb_chunk(const RaggedFrame* frames, int n) {
  LbChunk ch;
  for (int i = 0; i < RAGGED_CHUNK; ++i) {
    const RaggedFrame& r = frames[std::min(i, n - 1)];   // unused records repeat the last one
    LbFrame& f = ch.f[i];
    f.src = r.src;
    f.H = r.H; f.W = r.W; f.nh = r.nh; f.nw = r.nw; f.top = r.top; f.left = r.left;
    f.sx = resize_scale(r.W, r.nw);
    f.sy = resize_scale(r.H, r.nh);
    f.mode = resize_mode(r.H, r.W, r.nh, r.nw);
    f.reserved = 0;
  }
  return ch;
}

}  // namespace

hipError_t launch_letterbox_ragged_cn(const RaggedFrame* frames, int B, int cn, int oh, int ow, const uint8_t* pad,
                                      int swap_rb, int out_kind, void* dst, hipStream_t st) {
  if (cn == 3) return launch_letterbox_ragged(frames, B, oh, ow, pad, swap_rb, out_kind, dst, st);
  const LbPad p = lb_pack_pad(pad, cn);
  for (int b0 = 0; b0 < B; b0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - b0);
    const LbChunk ch = lb_chunk(frames + b0, n);
    const dim3 grid((ow + 127) / 128, oh, n);
    lb_dispatch_cn(out_kind, cn, [&](auto out, auto count) {
      hipLaunchKernelGGL((letterbox_ragged_cn_kernel<decltype(out)::value, decltype(count)::value>), grid, dim3(128),
                         0, st, ch, b0, cn, oh, ow, p, dst);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_letterbox_ragged(const RaggedFrame* frames, int B, int oh, int ow, const uint8_t pad[3],
                                   int swap_rb, int out_kind, void* dst, hipStream_t st) {
  for (int b0 = 0; b0 < B; b0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - b0);
    const LbChunk ch = lb_chunk(frames + b0, n);
    const dim3 grid((ow + 127) / 128, oh, n);
    if (out_kind == 0)
      hipLaunchKernelGGL(letterbox_ragged_kernel<0>, grid, dim3(128), 0, st, ch, b0, oh, ow, pad[0], pad[1], pad[2],
                         swap_rb, dst);
    else if (out_kind == 1)
      hipLaunchKernelGGL(letterbox_ragged_kernel<1>, grid, dim3(128), 0, st, ch, b0, oh, ow, pad[0], pad[1], pad[2],
                         swap_rb, dst);
    else
      hipLaunchKernelGGL(letterbox_ragged_kernel<2>, grid, dim3(128), 0, st, ch, b0, oh, ow, pad[0], pad[1], pad[2],
                         swap_rb, dst);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

size_t letterbox_workspace_bytes(int nh, int nw) { return (size_t)(4 * nw + 4 * nh) * sizeof(int) + 256; }

hipError_t launch_letterbox(const uint8_t* src, int B, int H, int W, int nh, int nw, int top, int left, int oh,
                            int ow, const uint8_t pad[3], int out_kind, void* dst, void* ws, hipStream_t st) {
  int* w = reinterpret_cast<int*>(ws);
  LbTab t{w, w + nw, w + 2 * nw, w + 3 * nw, w + 4 * nw, w + 4 * nw + nh, w + 4 * nw + 2 * nh, w + 4 * nw + 3 * nh};
  const int mode = resize_mode(H, W, nh, nw);
  if (mode == RESIZE_LINEAR) {
    const int n = nw + nh;
    hipLaunchKernelGGL(lb_tables_kernel, dim3((n + 255) / 256), dim3(256), 0, st, t, H, W, nh, nw);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const dim3 grid((ow + 127) / 128, oh, B);
  if (out_kind == 0)
    hipLaunchKernelGGL(letterbox_kernel<0>, grid, dim3(128), 0, st, src, H, W, nh, nw, top, left, oh, ow, pad[0],
                       pad[1], pad[2], mode, t, dst);
  else if (out_kind == 1)
    hipLaunchKernelGGL(letterbox_kernel<1>, grid, dim3(128), 0, st, src, H, W, nh, nw, top, left, oh, ow, pad[0],
                       pad[1], pad[2], mode, t, dst);
  else
    hipLaunchKernelGGL(letterbox_kernel<2>, grid, dim3(128), 0, st, src, H, W, nh, nw, top, left, oh, ow, pad[0],
                       pad[1], pad[2], mode, t, dst);
  return hipGetLastError();
}

// Three channels written as launch_letterbox writes them (uint8, or float planes reversed) take its kernels.
hipError_t launch_letterbox_cn(const uint8_t* src, int B, int H, int W, int cn, int nh, int nw, int top, int left,
                               int oh, int ow, const uint8_t* pad, int swap_rb, int out_kind, void* dst, void* ws,
                               hipStream_t st) {
  if (cn == 3 && (out_kind == 0 || swap_rb))
    return launch_letterbox(src, B, H, W, nh, nw, top, left, oh, ow, pad, out_kind, dst, ws, st);
  int* w = reinterpret_cast<int*>(ws);
  LbTab t{w, w + nw, w + 2 * nw, w + 3 * nw, w + 4 * nw, w + 4 * nw + nh, w + 4 * nw + 2 * nh, w + 4 * nw + 3 * nh};
  const int mode = resize_mode(H, W, nh, nw);
  if (mode == RESIZE_LINEAR) {
    const int n = nw + nh;
    hipLaunchKernelGGL(lb_tables_kernel, dim3((n + 255) / 256), dim3(256), 0, st, t, H, W, nh, nw);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const LbPad p = lb_pack_pad(pad, cn);
  const dim3 grid((ow + 127) / 128, oh, B);
  lb_dispatch_cn(out_kind, cn, [&](auto out, auto count) {
    hipLaunchKernelGGL((letterbox_cn_kernel<decltype(out)::value, decltype(count)::value>), grid, dim3(128), 0, st,
                       src, H, W, cn, nh, nw, top, left, oh, ow, p, mode, t, dst);
  });
  return hipGetLastError();
}

}  // namespace yv7
