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
//
// confusion_kernel (below match_kernel) builds the evaluation's confusion matrix, utils/metrics.py:121-159 as
// test.py:137-140,181-189 calls it, for a whole batch in one launch behind match_kernel's, adding into a matrix
// that stays on the device for the whole run.  It shares native_label() with match_kernel.
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

// One label row (image, class, x, y, w, h normalised to the canvas) as its box in the image's own pixels:
// test.py:123 (to canvas pixels), xywh2xyxy, then scale_coords(ratio_pad) + clip_coords
struct NativeBox {
  float x1, y1, x2, y2;
};
__device__ __forceinline__ NativeBox native_label(const float* __restrict__ t, float canvas_w, float canvas_h,
                                                  const ScaleImage& im, float w0, float h0) {
  const float x = t[2] * canvas_w, y = t[3] * canvas_h, w = t[4] * canvas_w, h = t[5] * canvas_h;
  NativeBox n;
  n.x1 = fminf(fmaxf(((x - w / 2.f) - im.pad_w) / im.gain, 0.f), w0);
  n.y1 = fminf(fmaxf(((y - h / 2.f) - im.pad_h) / im.gain, 0.f), h0);
  n.x2 = fminf(fmaxf(((x + w / 2.f) - im.pad_w) / im.gain, 0.f), w0);
  n.y2 = fminf(fmaxf(((y + h / 2.f) - im.pad_h) / im.gain, 0.f), h0);
  return n;
}

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
        const NativeBox n = native_label(t, canvas_w, canvas_h, im, w0, h0);
        s_cls[tid] = t[1]; s_x1[tid] = n.x1; s_y1[tid] = n.y1; s_x2[tid] = n.x2; s_y2[tid] = n.y2;
        s_area[tid] = (n.x2 - n.x1) * (n.y2 - n.y1);
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

// ------------------------------------------------------------------------------------------ confusion matrix
// Per image (one workgroup), the reference's steps with its quirks: rows with conf > conf are live; every
// (label, live row) pair of box_iou > iou_thres is a candidate, whatever the classes; a row keeps its candidate
// label of highest IoU (the first maximum in label order), a label keeps among the rows that chose it the one of
// highest IoU (the lowest row on ties), and a row that lost its label is unmatched: it takes no second choice.
//
// A row bids for its label with a 64-bit atomic max on key[label] = (IoU as an order-preserving unsigned word,
// ~row): the higher IoU wins, then the lower row; 0 is "no bid" (no real IoU maps to a zero high word).  The
// keys and each row's chosen label live in the workspace, so neither max_det nor the labels per image are bounded
// by LDS.  After a barrier the labels add their cells (matched: [gc][dc], unmatched: [nc][gc]) and, if the image
// has a match at all, the unmatched live rows add [dc][nc].  Cells are added with integer atomics, so the sums
// do not depend on their order.
__device__ __forceinline__ unsigned ordered_bits(float v) {
  const unsigned u = __float_as_uint(v + 0.f);   // -0 becomes +0: equal floats, equal words
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// .int() of a class value as a matrix index, or -1 when it lies outside [0, nc) or is a NaN
__device__ __forceinline__ int class_index(float c, int nc) {
  return (c > -1.f && c < (float)nc) ? (int)c : -1;
}

// One increment at [r][c]; an index of -1 drops it and counts the drop in the entry behind the matrix
__device__ __forceinline__ void add_cell(int32_t* matrix, int nc, int r, int c) {
  const int n1 = nc + 1;
  atomicAdd(matrix + ((r < 0 || c < 0) ? n1 * n1 : r * n1 + c), 1);
}

__global__ __launch_bounds__(MATCH_THREADS) void confusion_kernel(
    MatchChunk ch, int b0, const float* __restrict__ det, const int32_t* __restrict__ count, int max_det,
    const float* __restrict__ targets, const int32_t* __restrict__ label_off, int L, float canvas_h, float canvas_w,
    float conf, float iou_thres, int nc, int32_t* matrix, unsigned long long* key, int32_t* chosen) {
  __shared__ float s_x1[MATCH_THREADS], s_y1[MATCH_THREADS], s_x2[MATCH_THREADS], s_y2[MATCH_THREADS],
      s_area[MATCH_THREADS];
  __shared__ int s_any;
  const int tid = threadIdx.x;
  const ScaleImage im = ch.im[blockIdx.x];
  const int b = b0 + blockIdx.x;
  const int cnt = min(max(count[b], 0), max_det);
  const int lo = min(max(label_off[b], 0), L);
  const int hi = min(max(label_off[b + 1], lo), L);
  if (cnt == 0 || hi == lo) return;   // test.py:137-140 and `if nl` (uniform over the workgroup)

  if (tid == 0) s_any = 0;
  for (int l = lo + tid; l < hi; l += MATCH_THREADS)
    __hip_atomic_store(key + l, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  __syncthreads();

  const float w0 = (float)im.w0, h0 = (float)im.h0;
  const float* dimg = det + (size_t)b * max_det * 6;
  int32_t* cimg = chosen + (size_t)b * max_det;
  for (int r0 = 0; r0 < cnt; r0 += MATCH_THREADS) {
    const int row = r0 + tid;
    bool live = false;
    float px1 = 0.f, py1 = 0.f, px2 = 0.f, py2 = 0.f, parea = 0.f;
    if (row < cnt) {
      const float* p = dimg + (size_t)row * 6;
      live = p[4] > conf;
      px1 = p[0]; py1 = p[1]; px2 = p[2]; py2 = p[3];
      parea = (px2 - px1) * (py2 - py1);
    }
    bool found = false;
    float best = 0.f;
    int best_l = 0;
    for (int c0 = lo; c0 < hi; c0 += MATCH_THREADS) {
      __syncthreads();   // the previous chunk has been read
      if (c0 + tid < hi) {
        const NativeBox n = native_label(targets + (size_t)(c0 + tid) * 6, canvas_w, canvas_h, im, w0, h0);
        s_x1[tid] = n.x1; s_y1[tid] = n.y1; s_x2[tid] = n.x2; s_y2[tid] = n.y2;
        s_area[tid] = (n.x2 - n.x1) * (n.y2 - n.y1);
      }
      __syncthreads();
      if (live) {
        const int n = min(MATCH_THREADS, hi - c0);
        for (int j = 0; j < n; ++j) {
          // box_iou, utils/general.py:464-486
          const float iw = clamp0(tmin(px2, s_x2[j]) - tmax(px1, s_x1[j]));
          const float ih = clamp0(tmin(py2, s_y2[j]) - tmax(py1, s_y1[j]));
          const float inter = iw * ih;
          const float iou = inter / ((parea + s_area[j]) - inter);
          if (iou > iou_thres && (!found || iou > best)) {   // a NaN is never a candidate
            found = true;
            best = iou;
            best_l = c0 + j;
          }
        }
      }
    }
    if (row < cnt) cimg[row] = found ? best_l : -1;
    if (found)
      atomicMax(key + best_l, ((unsigned long long)ordered_bits(best) << 32) | (0xffffffffu - (unsigned)row));
  }
  __threadfence();
  __syncthreads();

  bool any = false;
  for (int l = lo + tid; l < hi; l += MATCH_THREADS) {
    const unsigned long long k = __hip_atomic_load(key + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int gc = class_index(targets[(size_t)l * 6 + 1], nc);
    if (k != 0ull) {
      // the winner's row; a foreign key (label ranges that overlap through a bad label_off) stays in bounds
      const unsigned row = min(0xffffffffu - (unsigned)k, (unsigned)(max_det - 1));
      add_cell(matrix, nc, gc, class_index(dimg[(size_t)row * 6 + 5], nc));
      any = true;
    } else {
      add_cell(matrix, nc, nc, gc);
    }
  }
  if (any) s_any = 1;
  __syncthreads();
  if (!s_any) return;   // the reference's `if n:`: without a match the rows add nothing
  for (int row = tid; row < cnt; row += MATCH_THREADS) {
    const float* p = dimg + (size_t)row * 6;
    if (!(p[4] > conf)) continue;
    const int l = cimg[row];   // written by this very thread
    unsigned winner = 0;   // ~row of the label's winner; no row's ~row is 0
    if (l >= 0) winner = (unsigned)__hip_atomic_load(key + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool won = winner == 0xffffffffu - (unsigned)row;
    if (!won) add_cell(matrix, nc, class_index(p[5], nc), nc);
  }
}

// ------------------------------------------------------------------------------------------ COCO matching
// pycocotools' bbox COCOeval.evaluateImg for a whole batch (the contract is in include/yv7.h), in IEEE double on
// the values that test.py's _predictions.json holds.  One workgroup takes one image, in two phases.
//
// Phase 1, a thread per row: the row's box as the JSON's rounded (x, y, w, h) and, by counting over the image's
// rows (staged through LDS, COCO_THREADS at a time), the number of rows of a lower class and the number of rows
// of its own class that precede it in (rounded score descending, row) order.  Their sum is the row's place in
// the image's rows sorted by (class, score, row); the second count is its rank.  The box goes to that place in
// the workspace, and a row of rank 0 registers its class as a job.  The image's gts get the same treatment:
// gperm lists them by class, in annotation order within a class.
//
// Phase 2, a wave per class: lane a * 10 + t runs the greedy matching of area range a at threshold t (lanes 40
// and up shadow lane 39 and are dropped), so the walk over detections and gts and every IoU are uniform over the
// wave and only the bookkeeping differs per lane.  Detections and gts are loaded 64 at a time, one per lane, and
// handed round with v_readlane.  The contract's gt order (not ignored first) needs no sort: until a detection has
// a match among the gts its range does not ignore, the scan keeps the two groups' best candidates apart, and
// the first group's wins.  Which gts a lane has matched is a 64-bit mask in a register; a class with more than 64
// gts in the image keeps one mask per 64 gts and lane in the workspace.
constexpr int COCO_THREADS = 256, COCO_WAVE = 64, COCO_LANES = 40, COCO_MAX_DETS = 100, COCO_T = 10;

struct CocoThr {
  double t[COCO_T];   // np.linspace(0.5, 0.95, 10)
};

// round(float(v), 3) and round(float(s), 5) of the JSON rows: the products are exact in double
__device__ __forceinline__ double round3(float v) { return rint((double)v * 1000.0) / 1000.0; }
__device__ __forceinline__ double round5(float v) { return rint((double)v * 100000.0) / 100000.0; }

__device__ __forceinline__ int lane_int(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ double lane_double(double v, int lane) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                          __builtin_amdgcn_readlane(__double2loint(v), lane));
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = COCO_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, COCO_WAVE);
  return v;
}

__global__ __launch_bounds__(COCO_THREADS) void coco_match_kernel(
    int b0, const float* __restrict__ det, const int32_t* __restrict__ count, int max_det,
    const double* __restrict__ gts, const int32_t* __restrict__ gt_off, int G, CocoThr thr,
    uint32_t* __restrict__ flags, int32_t* __restrict__ rank, double* dbox, unsigned long long* mws, int32_t* drow,
    int32_t* heads, int32_t* gperm) {
  __shared__ double s_score[COCO_THREADS];
  __shared__ float s_cls[COCO_THREADS];
  __shared__ int s_nheads;
  const int tid = threadIdx.x;
  const int b = b0 + blockIdx.x;
  const int cnt = min(max(count[b], 0), max_det);
  const int glo = min(max(gt_off[b], 0), G);
  const int ghi = min(max(gt_off[b + 1], glo), G);
  const size_t img = (size_t)b * max_det;
  if (tid == 0) s_nheads = 0;
  __syncthreads();

  // ---- phase 1: rows
  for (int r0 = 0; r0 < max_det; r0 += COCO_THREADS) {
    const int row = r0 + tid;
    const bool live = row < cnt;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, cls = 0.f;
    double sc = 0.0;
    if (live) {
      const float* p = det + (img + row) * 6;
      x1 = p[0]; y1 = p[1]; x2 = p[2]; y2 = p[3]; cls = p[5];
      sc = round5(p[4]);
    }
    int below = 0, ahead = 0, same = 0;
    if (r0 < cnt) {   // uniform over the workgroup
      for (int c0 = 0; c0 < cnt; c0 += COCO_THREADS) {
        __syncthreads();   // the previous chunk has been read
        if (c0 + tid < cnt) {
          const float* q = det + (img + c0 + tid) * 6;
          s_score[tid] = round5(q[4]);
          s_cls[tid] = q[5];
        }
        __syncthreads();
        if (live) {
          const int n = min(COCO_THREADS, cnt - c0);
          for (int j = 0; j < n; ++j) {
            const float c2 = s_cls[j];
            if (c2 < cls) {
              ++below;
            } else if (c2 == cls) {
              ++same;
              const double s2 = s_score[j];
              if (s2 > sc || (s2 == sc && c0 + j < row)) ++ahead;
            }
          }
        }
      }
    }
    if (row >= max_det) continue;
    const int rk = (live && ahead < COCO_MAX_DETS) ? ahead : -1;
    rank[img + row] = rk;
    if (rk < 0)
      for (int a = 0; a < 4; ++a) flags[(img + row) * 4 + a] = 0u;
    if (!live) continue;
    const int pos = min(below + ahead, cnt - 1);
    // xyxy2xywh in fp32, then the corner (test.py:168-177)
    const float w = x2 - x1, h = y2 - y1;
    const float cx = (x1 + x2) / 2.f, cy = (y1 + y2) / 2.f;
    double* o = dbox + (img + pos) * 4;
    o[0] = round3(cx - w / 2.f);
    o[1] = round3(cy - h / 2.f);
    o[2] = round3(w);
    o[3] = round3(h);
    drow[img + pos] = row;
    if (ahead == 0) {
      const int i = min(atomicAdd(&s_nheads, 1), cnt - 1);
      heads[(img + i) * 2] = pos;
      heads[(img + i) * 2 + 1] = same;
    }
  }
  // ---- phase 1: gts by class, annotation order kept
  for (int g = glo + tid; g < ghi; g += COCO_THREADS) {
    const double c = gts[(size_t)g * 7];
    int before = 0;
    for (int g2 = glo; g2 < ghi; ++g2) {
      const double c2 = gts[(size_t)g2 * 7];
      if (c2 < c || (c2 == c && g2 < g)) ++before;
    }
    gperm[min(glo + before, ghi - 1)] = g;
  }
  __threadfence();
  __syncthreads();

  // ---- phase 2: a wave per class
  const int wave = __builtin_amdgcn_readfirstlane(tid / COCO_WAVE);
  const int lane = tid % COCO_WAVE;
  const int at = min(lane, COCO_LANES - 1);
  const int ar = at / COCO_T;
  const double a_lo = ar == 2 ? 1024.0 : ar == 3 ? 9216.0 : 0.0;
  const double a_hi = ar == 1 ? 1024.0 : ar == 2 ? 9216.0 : 1e10;
  const double t0 = thr.t[at % COCO_T] < 1.0 - 1e-10 ? thr.t[at % COCO_T] : 1.0 - 1e-10;
  const int nheads = min(s_nheads, cnt);
  for (int hd = wave; hd < nheads; hd += COCO_THREADS / COCO_WAVE) {
    const int pos0 = __builtin_amdgcn_readfirstlane(min(max(heads[(img + hd) * 2], 0), cnt - 1));
    const int nd = __builtin_amdgcn_readfirstlane(
        min(min(max(heads[(img + hd) * 2 + 1], 0), COCO_MAX_DETS), cnt - pos0));
    const int hrow = min(max(drow[img + pos0], 0), cnt - 1);
    const double cls = (double)det[(img + hrow) * 6 + 5];
    // the class's gts are gperm[gs .. gs + ng)
    int nb = 0, ne = 0;
    for (int g = glo + lane; g < ghi; g += COCO_WAVE) {
      const double c2 = gts[(size_t)g * 7];
      nb += c2 < cls;
      ne += c2 == cls;
    }
    nb = wave_sum(nb);
    ne = wave_sum(ne);
    const int gs = __builtin_amdgcn_readfirstlane(min(glo + nb, ghi));
    const int ng = __builtin_amdgcn_readfirstlane(min(ne, ghi - gs));
    const int nchunk = (ng + COCO_WAVE - 1) / COCO_WAVE;
    const bool multi = nchunk > 1;
    if (multi && lane < COCO_LANES)
      for (int k = 0; k < nchunk; ++k) mws[(size_t)(gs + k * COCO_WAVE) * COCO_LANES + lane] = 0ull;

    double gx = 0.0, gy = 0.0, gw = 0.0, gh = 0.0, garea = 0.0;
    int gcrowd = 0;
    unsigned long long mask = 0ull;
    auto load_gts = [&](int k) {
      const int gi = k * COCO_WAVE + lane;
      if (gi < ng) {
        const int g = min(max(gperm[gs + gi], glo), ghi - 1);
        const double* q = gts + (size_t)g * 7;
        gx = q[1]; gy = q[2]; gw = q[3]; gh = q[4]; garea = q[5];
        gcrowd = q[6] != 0.0;
      }
    };
    if (!multi && ng > 0) load_gts(0);

    for (int d0 = 0; d0 < nd; d0 += COCO_WAVE) {
      double dx = 0.0, dy = 0.0, dw = 0.0, dh = 0.0;
      int dr = 0;
      if (d0 + lane < nd) {
        const double* q = dbox + (img + pos0 + d0 + lane) * 4;
        dx = q[0]; dy = q[1]; dw = q[2]; dh = q[3];
        dr = min(max(drow[img + pos0 + d0 + lane], 0), cnt - 1);
      }
      const int ndc = min(COCO_WAVE, nd - d0);
      for (int dj = 0; dj < ndc; ++dj) {
        const double x = lane_double(dx, dj), y = lane_double(dy, dj), w = lane_double(dw, dj),
                     h = lane_double(dh, dj);
        const int row = lane_int(dr, dj);
        const double da = w * h;
        double iou_n = t0, iou_i = t0;   // the running bar among the gts not ignored / ignored
        int m_n = -1, m_i = -1;
        for (int k = 0; k < nchunk; ++k) {
          if (multi) {
            load_gts(k);
            mask = lane < COCO_LANES ? mws[(size_t)(gs + k * COCO_WAVE) * COCO_LANES + lane] : 0ull;
          }
          const int n = min(COCO_WAVE, ng - k * COCO_WAVE);
          for (int j = 0; j < n; ++j) {
            const double X = lane_double(gx, j), Y = lane_double(gy, j), W = lane_double(gw, j),
                         H = lane_double(gh, j), A = lane_double(garea, j);
            const bool crowd = lane_int(gcrowd, j) != 0;
            const double xe = x + w < X + W ? x + w : X + W, xs = x > X ? x : X;
            const double ye = y + h < Y + H ? y + h : Y + H, ys = y > Y ? y : Y;
            const double iw = xe - xs, ih = ye - ys;
            double iou = 0.0;
            if (iw > 0.0 && ih > 0.0) {
              const double inter = iw * ih;
              const double ga = W * H;
              const double uni = crowd ? da : da + ga - inter;
              iou = inter / uni;
            }
            if (((mask >> j) & 1ull) && !crowd) continue;
            const bool ig = crowd || A < a_lo || A > a_hi;
            if (!ig) {
              if (!(iou < iou_n)) { iou_n = iou; m_n = k * COCO_WAVE + j; }
            } else {
              if (!(iou < iou_i)) { iou_i = iou; m_i = k * COCO_WAVE + j; }
            }
          }
        }
        const int m = m_n >= 0 ? m_n : m_i;
        const bool matched = m >= 0;
        const bool ignored = matched ? m_n < 0 : (da < a_lo || da > a_hi);
        if (matched) {
          if (!multi) {
            mask |= 1ull << m;
          } else if (lane < COCO_LANES) {
            mws[(size_t)(gs + (m / COCO_WAVE) * COCO_WAVE) * COCO_LANES + lane] |= 1ull << (m % COCO_WAVE);
          }
        }
        const unsigned long long bm = __ballot(matched), bi = __ballot(ignored);
        if (lane < 4)
          flags[(img + row) * 4 + lane] = (uint32_t)((bm >> (lane * COCO_T)) & 0x3ffull) |
                                          ((uint32_t)((bi >> (lane * COCO_T)) & 0x3ffull) << COCO_T);
      }
    }
  }
}

}  // namespace

size_t coco_match_ws_bytes(int B, int max_det, int G) {
  if (B <= 0 || max_det <= 0 || G < 0) return 0;
  const size_t rows = (size_t)B * max_det;
  // dbox [rows][4] double, mws [G][40] u64, drow [rows] i32, heads [rows][2] i32, gperm [G] i32
  return rows * (4 * sizeof(double) + 3 * sizeof(int32_t)) +
         (size_t)G * (COCO_LANES * sizeof(unsigned long long) + sizeof(int32_t));
}

hipError_t launch_coco_match(const float* det, const int32_t* count, int B, int max_det, const double* gts,
                             const int32_t* gt_off, int G, uint32_t* flags, int32_t* rank, void* ws, hipStream_t st) {
  const size_t rows = (size_t)B * max_det;
  double* dbox = reinterpret_cast<double*>(ws);
  unsigned long long* mws = reinterpret_cast<unsigned long long*>(dbox + rows * 4);
  int32_t* drow = reinterpret_cast<int32_t*>(mws + (size_t)G * COCO_LANES);
  int32_t* heads = drow + rows;
  int32_t* gperm = heads + rows * 2;
  CocoThr thr;   // np.linspace(0.5, 0.95, 10): arange(10) * step + start, the last one set to stop
  const double step = (0.95 - 0.5) / 9.0;
  for (int i = 0; i < COCO_T; ++i) thr.t[i] = (double)i * step + 0.5;
  thr.t[COCO_T - 1] = 0.95;
  for (int b0 = 0; b0 < B; b0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - b0);
    hipLaunchKernelGGL(coco_match_kernel, dim3(n), dim3(COCO_THREADS), 0, st, b0, det, count, max_det, gts, gt_off, G,
                       thr, flags, rank, dbox, mws, drow, heads, gperm);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

size_t confusion_ws_bytes(int B, int max_det, int L) {
  if (B <= 0 || max_det <= 0 || L < 0) return 0;
  return (size_t)L * sizeof(unsigned long long) + (size_t)B * max_det * sizeof(int32_t);
}

hipError_t launch_confusion(const float* det, const int32_t* count, int B, int max_det, const float* targets,
                            const int32_t* label_off, int L, const ScaleImage* images, int canvas_h, int canvas_w,
                            float conf, float iou_thres, int nc, int32_t* matrix, void* ws, hipStream_t st) {
  unsigned long long* key = reinterpret_cast<unsigned long long*>(ws);   // [L], then chosen [B, max_det]
  int32_t* chosen = reinterpret_cast<int32_t*>(key + L);
  for (int b0 = 0; b0 < B; b0 += RAGGED_CHUNK) {
    const int n = std::min(RAGGED_CHUNK, B - b0);
    MatchChunk ch;
    for (int i = 0; i < RAGGED_CHUNK; ++i) ch.im[i] = images[b0 + std::min(i, n - 1)];   // unused: the last one
    hipLaunchKernelGGL(confusion_kernel, dim3(n), dim3(MATCH_THREADS), 0, st, ch, b0, det, count, max_det, targets,
                       label_off, L, (float)canvas_h, (float)canvas_w, conf, iou_thres, nc, matrix, key, chosen);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

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
