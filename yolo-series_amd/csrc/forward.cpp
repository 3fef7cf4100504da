// libyv7 forward: the per-batch launch sequence of the fused network.
//
// yv7_forward walks the plan's op list once per batch, launching one kernel per op (or per fused group of ops)
// on the caller's stream (forward_once's per-layer loop, models/yolo.py:603-627, without the Python
// dispatch); no allocation, no host sync, so callers can capture it in a graph.
#include <cxxabi.h>

#include <cstdlib>
#include <cstring>

#include "plan.h"

using namespace yv7rt;

namespace {

// One forward's arguments and layout, as the per-kind op functions see them.
struct Fwd {
  const yv7_plan* p;
  const Layout& l;
  const void* x;
  int x_dtype;
  float* z;
  float* raw;
  float* best;   // row records the fp16 head's epilogue writes, or null
  unsigned char* wsb;
  hipStream_t st;
  unsigned char* at(int tensor) const { return wsb + l.off[tensor]; }
};

int launched(hipError_t e) { return e == hipSuccess ? 0 : hip_fail(e, "yv7_forward launch"); }

// The MP block's two readers of one tensor (cfg/deploy/yolov7.yaml: `MP -> 1x1` and `1x1`, adjacent ops
// i, i + 1: the pooled one is the fp16 plan's pool = 2 op) as ONE register-streamed launch that reads the
// tensor once (conv_rs.hip); the second op records no time of its own.  Both ops on the default dispatch
// only; YV7_DUAL=0: off.  Fills the full-resolution conv *cf and its pooled partner *q; returns 2, or 0.
int find_pair(const yv7_plan* p, size_t i, const Layout& l, unsigned char* wsb, yv7::ConvParams* cf,
              yv7::Conv1x1Pooled* q) {
  static const int dual = yv7::env_int("YV7_DUAL", 1);
  if (!dual || p->dtype != YV7_DT_F16 || i + 1 >= p->ops.size() || p->op_variant[i] || p->op_variant[i + 1]) return 0;
  const auto& o = p->ops[i];
  const auto& o1 = p->ops[i + 1];
  // one launch reads the shared slice while it writes both outputs: neither output may overlap the input
  // slice or the other output (in order, op i + 1 would see op i's writes) — the hazards graph.py's
  // _merge_siblings checks before its fusions
  if (o1.kind != YV7_OP_CONV || is_f8(o1) || o.src2 >= 0 || o1.src2 >= 0 || o1.src != o.src || o1.src_coff != o.src_coff || o1.cin != o.cin ||
      o1.k != 1 || o.k != 1 || (o.pool == 2) == (o1.pool == 2) || o1.w_off == o.w_off ||
      overlap(o.dst, o.dst_coff, o.cout, o.src, o.src_coff, o.cin) ||
      overlap(o1.dst, o1.dst_coff, o1.cout, o.src, o.src_coff, o.cin) ||
      overlap(o.dst, o.dst_coff, o.cout, o1.dst, o1.dst_coff, o1.cout))
    return 0;
  const size_t fi = o.pool == 2 ? i + 1 : i, pi = o.pool == 2 ? i : i + 1;
  yv7::ConvParams cp;
  if (!bind_conv(p, fi, l, wsb, cf)) return 0;
  bind_conv(p, pi, l, wsb, &cp);   // (its output shape: the shift test below)
  q->w = cp.w;
  q->bias = cp.bias;
  q->y = cp.y;
  q->yc = cp.yc;
  q->yoff = cp.yoff;
  q->cout = cp.cout;
  q->act = cp.act;
  if (p->tensors[p->ops[pi].dst].shift != p->tensors[p->ops[fi].dst].shift + 1) return 0;
  return yv7::conv1x1_rs_supported(*cf, q) ? 2 : 0;
}

// SPPCSPC's cascade (graph.py: pool5 three times, each reading the previous slice of one concat tensor) as
// one fused launch; the two later ops record no time of their own.
struct PoolCascade {
  void* x;
  int H, W, xc, coff, C;
};
int find_cascade(const yv7_plan* p, size_t i, const Layout& l, unsigned char* wsb, PoolCascade* c) {
  if (i + 2 >= p->ops.size()) return 0;
  const auto &o = p->ops[i], &o1 = p->ops[i + 1], &o2 = p->ops[i + 2];
  const auto& ti = p->tensors[o.src];
  auto pool5 = [](const yv7_op_desc& q) { return q.kind == YV7_OP_MAXPOOL && q.k == 5 && q.s == 1 && q.pad == 2; };
  *c = PoolCascade{wsb + l.off[o.src], l.H >> ti.shift, l.W >> ti.shift, ti.channels, o.src_coff, o.cout};
  const bool cascade = pool5(o) && pool5(o1) && pool5(o2) && o.src == o.dst && o1.src == o.dst && o1.dst == o.dst &&
                       o2.src == o.dst && o2.dst == o.dst && o.dst_coff == o.src_coff + o.cout &&
                       o1.src_coff == o.dst_coff && o1.dst_coff == o1.src_coff + o.cout && o2.src_coff == o1.dst_coff &&
                       o2.dst_coff == o2.src_coff + o.cout && o1.cout == o.cout && o2.cout == o.cout &&
                       yv7::spp_cascade_supported(p->dtype, c->H, c->W, o.cout);
  return cascade ? 3 : 0;
}

int op_input(const Fwd& f, const yv7_op_desc& o) {
  return launched(yv7::launch_input(f.p->dtype, f.x, f.x_dtype, f.at(o.dst), f.l.B, input_channels(o), f.l.H, f.l.W,
                                    f.p->tensors[o.dst].channels, o.k == 2, f.st));
}

// 82: the fp8 GEMM quantizes the fp16 input slice on its way into LDS (no staging pass, but every N tile
// of a row block converts it again: VALU work ~2x the block's MFMA time per K step); 81: a separate
// quantize pass into the dense e4m3 staging buffer, then the GEMM reads e4m3 by LDS-DMA.  Default (measured
// per layer on MI355X, bs32 640, profiles/r2_fp8_ab_*.txt): fused up to 2 N tiles (cout <= 256), staged beyond.
int op_conv_f8(const Fwd& f, size_t i, const yv7::ConvParams& c) {
  const yv7_op_desc& o = f.p->ops[i];
  yv7::F8ConvParams q;
  std::memset(&q, 0, sizeof(q));
  const int v = f.p->op_variant[i];
  if (v == 81 || (v == 0 && o.cout > 256)) {
    unsigned char* x8 = f.wsb + f.l.f8_off;
    hipError_t e = yv7::launch_quant_f8(c.x, c.B, c.H, c.W, c.xc, c.xoff, o.cin, c.kpad, 1.0f / o.xscale, x8, f.st);
    if (e != hipSuccess) return hip_fail(e, "yv7_forward fp8 quantize");
    q.x8 = x8;
  } else {
    const size_t xb = yv7::bordered_pixels(c.B, c.H, c.W) * c.xc * 2;
    if (xb >= ((size_t)1 << 31))
      return fail(YV7_E_SHAPE, "yv7_forward: fp8 op " + std::to_string(i) + " input exceeds 2 GiB");
    q.x16 = c.x;
    q.xbytes = (uint32_t)xb;
    q.xc = c.xc;
    q.xoff = c.xoff;
    q.cin = o.cin;
    q.qscale = 1.0f / o.xscale;
  }
  q.y = c.y;
  q.w8 = c.w;
  q.bias = c.bias;
  q.wscale = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(f.p->weights) + o.s_off);
  q.xscale = o.xscale;
  q.wbytes = (uint32_t)((size_t)((o.cout + 31) / 32 * 32) * c.kpad);
  q.M = c.M;
  q.kp = c.kpad;
  q.cout = o.cout;
  q.H = c.Ho;
  q.W = c.Wo;
  q.yc = c.yc;
  q.yoff = c.yoff;
  q.act = o.act;
  return launched(yv7::launch_conv_f8(q, f.st));
}

// A CONV op: the fp8 GEMM, else the 3x3 chain or the dual 1x1 pair starting here (*n: the ops the launch
// covers), else its own kernel.
int op_conv(const Fwd& f, size_t i, size_t* n) {
  yv7::ConvParams c, cf;
  if (!bind_conv(f.p, i, f.l, f.wsb, &c))
    return fail(YV7_E_SHAPE, "yv7_forward: op " + std::to_string(i) + " output shape mismatch");
  if (is_f8(f.p->ops[i])) return op_conv_f8(f, i, c);
  yv7::ChainParams ch;
  if (const int k = find_chain(f.p, i, f.l, f.wsb, &ch)) {
    *n = k;
    return launched(yv7::launch_conv_chain(ch, f.st));
  }
  yv7::Conv1x1Pooled q;
  if (const int k = find_pair(f.p, i, f.l, f.wsb, &cf, &q)) {
    *n = k;
    return launched(yv7::launch_conv1x1_rs(cf, &q, f.st));
  }
  return launched(yv7::launch_conv(f.p->dtype, c, false, f.st));
}

int op_detect(const Fwd& f, size_t i) {
  const yv7_plan* p = f.p;
  const yv7_op_desc& o = p->ops[i];
  yv7::ConvParams c;
  bind_conv(p, i, f.l, f.wsb, &c);
  c.z = f.z;
  c.raw = f.raw ? f.raw + f.l.raw_off[o.level] : nullptr;
  c.nrows = f.l.nrows;
  c.row_off = f.l.row_off[o.level];
  c.na = p->na;
  c.no = p->no;
  c.stride = p->stride[o.level];
  for (int a = 0; a < p->na * 2; ++a) c.anchor[a] = p->anchor_grid[o.level * p->na * 2 + a];
  c.best = f.best;
  return launched(yv7::launch_conv(p->dtype, c, true, f.st));
}

int op_stem(const Fwd& f, const yv7_op_desc& o) {
  const int H = f.l.H, W = f.l.W;
  const auto& to = f.p->tensors[o.dst];
  const unsigned char* wb = reinterpret_cast<const unsigned char*>(f.p->weights);
  const int reorg = o.cin == 12;   // conv A runs on the 2x space-to-depth image
  if ((H >> to.shift) != H / (reorg + 1) / o.s / 2 || (W >> to.shift) != W / (reorg + 1) / o.s / 2 ||
      (reorg && (H % 4 || W % 4)))
    return fail(YV7_E_SHAPE, "yv7_forward: stem output shape mismatch");
  // the kernels address the image through 32-bit byte offsets, bit 31 marking a pixel outside it
  if ((size_t)f.l.B * input_channels(o) * H * W * (f.x_dtype == YV7_DT_F16 ? 2 : 4) >= ((size_t)1 << 31))
    return fail(YV7_E_SHAPE, "yv7_forward: stem input exceeds 2 GiB");
  yv7::StemParams sp;
  sp.variant = 0;
  sp.x = f.x;
  sp.y = f.at(o.dst);
  sp.wa = wb + o.w_off;
  sp.ba = reinterpret_cast<const float*>(wb + o.b_off);
  sp.wb = wb + o.w2_off;
  sp.bb = reinterpret_cast<const float*>(wb + o.b2_off);
  sp.B = f.l.B;
  sp.H = H;
  sp.W = W;
  sp.yc = to.channels;
  sp.yoff = o.dst_coff;
  sp.reorg = reorg;
  sp.cin = o.cin;
  sp.kpad_a = ((reorg ? 9 * 16 : 9 * o.cin) + 63) / 64 * 64;
  sp.kpad_b = (9 * o.cout + 63) / 64 * 64;
  sp.act_a = o.act;
  sp.act_b = o.act2;
  sp.sa = o.s;
  return launched(yv7::launch_stem(sp, f.x_dtype, f.st));
}

int op_maxpool(const Fwd& f, size_t i, size_t* n) {
  const yv7_op_desc& o = f.p->ops[i];
  const auto& ti = f.p->tensors[o.src];
  const auto& to = f.p->tensors[o.dst];
  PoolCascade c;
  if (const int k = find_cascade(f.p, i, f.l, f.wsb, &c)) {
    *n = k;
    return launched(yv7::launch_spp_cascade(f.p->dtype, c.x, f.l.B, c.H, c.W, c.xc, c.coff, c.C, f.st));
  }
  const int Hi = f.l.H >> ti.shift, Wi = f.l.W >> ti.shift;
  const int Ho = (Hi + 2 * o.pad - o.k) / o.s + 1, Wo = (Wi + 2 * o.pad - o.k) / o.s + 1;
  if (Ho != (f.l.H >> to.shift) || Wo != (f.l.W >> to.shift))
    return fail(YV7_E_SHAPE, "yv7_forward: maxpool op " + std::to_string(i) + " shape mismatch");
  return launched(yv7::launch_maxpool(f.p->dtype, f.at(o.src), f.l.B, Hi, Wi, ti.channels, o.src_coff, f.at(o.dst), Ho,
                                      Wo, to.channels, o.dst_coff, o.cout, o.k, o.s, o.pad, f.st));
}

int op_upsample(const Fwd& f, const yv7_op_desc& o) {
  const auto& ti = f.p->tensors[o.src];
  const auto& to = f.p->tensors[o.dst];
  if (to.shift + 1 != ti.shift) return fail(YV7_E_SHAPE, "yv7_forward: upsample shift mismatch");
  return launched(yv7::launch_upsample2x(f.p->dtype, f.at(o.src), f.l.B, f.l.H >> ti.shift, f.l.W >> ti.shift,
                                         ti.channels, o.src_coff, f.at(o.dst), to.channels, o.dst_coff, o.cout, f.st));
}

int op_copy(const Fwd& f, const yv7_op_desc& o) {
  const auto& ti = f.p->tensors[o.src];
  const auto& to = f.p->tensors[o.dst];
  if (to.shift != ti.shift) return fail(YV7_E_SHAPE, "yv7_forward: copy shift mismatch");
  return launched(yv7::launch_copy(f.p->dtype, f.at(o.src), f.l.B, f.l.H >> ti.shift, f.l.W >> ti.shift, ti.channels,
                                   o.src_coff, f.at(o.dst), to.channels, o.dst_coff, o.cout, f.st));
}

int op_add(const Fwd& f, const yv7_op_desc& o) {
  const auto& ta = f.p->tensors[o.src];
  const auto& tb = f.p->tensors[o.src2];
  const auto& to = f.p->tensors[o.dst];
  return launched(yv7::launch_add(f.p->dtype, f.at(o.src), ta.channels, o.src_coff, f.at(o.src2), tb.channels,
                                  o.src2_coff, f.at(o.dst), to.channels, o.dst_coff, f.l.B, f.l.H >> to.shift,
                                  f.l.W >> to.shift, o.cout, f.st));
}

// Launches op i, or the fused group that starts at it: *n ops (1 unless a recogniser found a group).
int run_op(const Fwd& f, size_t i, size_t* n) {
  const yv7_op_desc& o = f.p->ops[i];
  switch (o.kind) {
    case YV7_OP_INPUT: return op_input(f, o);
    case YV7_OP_CONV: return op_conv(f, i, n);
    case YV7_OP_DETECT: return op_detect(f, i);
    case YV7_OP_STEM: return op_stem(f, o);
    case YV7_OP_MAXPOOL: return op_maxpool(f, i, n);
    case YV7_OP_UPSAMPLE: return op_upsample(f, o);
    case YV7_OP_COPY: return op_copy(f, o);
    case YV7_OP_ADD: return op_add(f, o);
    default: return fail(YV7_E_ARG, "yv7_forward: unknown op kind");
  }
}

// Kernels write only tensor interiors, so the zero frames survive from one forward to the next:
// a workspace is cleared the first time it is seen with this layout (pointer, size AND the batch
// geometry: (B, H, W) and (B, W, H) have equal sizes but different frames) and never again, until
// the caller hands the memory back with yv7_workspace_forget (include/yv7.h).
int clear_on_first_use(yv7_plan* p, void* ws, const Layout& l, hipStream_t st) {
  for (const auto& w : p->ws_ready)
    if (w.ptr == ws && w.bytes == l.end && w.B == l.B && w.H == l.H && w.W == l.W) return 0;
  hipError_t e = hipMemsetAsync(ws, 0, l.end, st);
  if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync(workspace)");
  // a workspace overlapping this one (another layout of the same memory) is no longer intact
  forget_workspaces(p, ws, l.end);
  p->ws_ready.push_back({ws, l.end, l.B, l.H, l.W});
  if (p->ws_ready.size() > 8) p->ws_ready.erase(p->ws_ready.begin());
  return 0;
}

// The forward's op loop.  dry: launch nothing (yv7_kernels.h LaunchRec), record per op the host stubs
// of the kernels the dispatch picks into *kernels (yv7_op_kernels); no workspace clearing, no events.
int forward_impl(yv7_plan* p, const void* x, int x_dtype, int B, int H, int W, float* z, float* raw,
                 yv7_row_best* rowbest, void* ws, size_t ws_bytes, void* stream,
                 std::vector<std::vector<const void*>>* kernels) {
  const bool dry = kernels != nullptr;
  if (!p || !x || !z || !ws) return fail(YV7_E_ARG, "yv7_forward: null argument");
  if (x_dtype != YV7_DT_F32 && x_dtype != YV7_DT_F16) return fail(YV7_E_ARG, "yv7_forward: bad x_dtype");
  Layout l;
  if (int rc = plan_layout(p, B, H, W, &l)) return rc;
  if (!dry && ws_bytes < l.end) return fail(YV7_E_WORKSPACE, "yv7_forward: workspace too small (need " +
                                                                 std::to_string(l.end) + " bytes)");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!dry)
    if (int rc = clear_on_first_use(p, ws, l, st)) return rc;
  // fp16 plans score the rows in the head's epilogue; other paths derive the records from z after the
  // last op
  const bool rowbest_fused = rowbest && yv7::det_writes_rowbest(p->dtype);
  const Fwd f{p, l, x, x_dtype, z, raw, rowbest_fused ? reinterpret_cast<float*>(rowbest) : nullptr,
              reinterpret_cast<unsigned char*>(ws), st};
  hipEvent_t* ev = nullptr;
  // the forward's event slot is claimed only once every op has launched (below): a forward that fails
  // part-way leaves the slot to the next one instead of a pair that was never recorded
  if (!dry && p->prof_used < p->prof_max) ev = &p->events[(size_t)p->prof_used * 2 * p->ops.size()];
  // the op's (start, stop) pair rides on its kernel launches (yv7_kernels.h YV7_LAUNCH); cleared on
  // every way out of this function
  struct EventScope {
    ~EventScope() {
      yv7::op_events() = yv7::OpEvents{};
      yv7::launch_rec() = yv7::LaunchRec{};
    }
  } event_scope;
  if (dry) kernels->assign(p->ops.size(), {});
  hipError_t e = hipSuccess;
  size_t fused_until = 0;   // ops [.., fused_until) were launched as part of a fused group
  for (size_t i = 0; i < p->ops.size(); ++i) {
    if (ev) yv7::op_events() = yv7::OpEvents{ev[2 * i], ev[2 * i + 1], 0};
    if (dry) {
      yv7::launch_rec() = yv7::LaunchRec{};
      yv7::launch_rec().dry = true;
    }
    if (i >= fused_until) {   // else: launched with a predecessor — no kernel, an empty event pair
      size_t n = 1;
      if (int rc = run_op(f, i, &n)) return rc;
      fused_until = i + n;
    }
    if (dry) {
      const auto& r = yv7::launch_rec();
      if (r.n > 4) return fail(YV7_E_ARG, "yv7_op_kernels: op " + std::to_string(i) + " launches more than 4 kernels");
      for (int k = 0; k < r.n; ++k) (*kernels)[i].push_back(r.fn[k]);
    }
    if (ev && yv7::op_events().launches == 0) {   // no kernel of its own (a later op of a fused group)
      if ((e = hipEventRecord(ev[2 * i], st)) != hipSuccess || (e = hipEventRecord(ev[2 * i + 1], st)) != hipSuccess)
        return hip_fail(e, "hipEventRecord");
    }
  }
  yv7::op_events() = yv7::OpEvents{};
  if (dry) return 0;
  if (ev) p->prof_used++;
  if (rowbest && !rowbest_fused &&
      (e = yv7::launch_row_best(z, B, l.nrows, p->no, rowbest, st)) != hipSuccess)
    return hip_fail(e, "yv7_forward row scores");
  return 0;
}

}  // namespace

// A chain of 3x3 stride-1 fp16 convs starting at op i that the runtime launches as ONE kernel
// (conv_lr.hip conv3x3_chain_kernel: an ELAN block's 3x3 stack): ops i .. i + n - 1, each reading the
// previous one's output slice, all of a shape the low-resolution kernel takes.  NOT in the default dispatch:
// measured slower than the per-layer launches on every yolov7 bs 32 stack it applies to (round 6,
// profiles/r6_chain/: 20^2 256 x 4 116.8 vs 89.4 us, 40^2 128 x 4 130.0 vs 105.0; bench 7679 / 7710 vs 7847 /
// 7868 img/s) — each layer's 640 tiles are one round of the chip, so the next layer's tiles find nothing to
// overlap with, and the queue's dequeues plus the polls cost more than the three kernel boundaries they
// remove.  Forced per chain with variant 305 on its first op (yv7_set_op_variant; the later ops on 0);
// YV7_CHAIN=1 chains every eligible stack.  Fills *c (pointers from workspace base wsb, null for a layout
// query) and returns n (0: no chain here); the later ops of the chain record no time of their own.
int yv7rt::find_chain(const yv7_plan* p, size_t i, const Layout& l, unsigned char* wsb, yv7::ChainParams* c) {
  static const int all = yv7::env_int("YV7_CHAIN", 0);
  static const long max_tasks = yv7::env_int("YV7_CHAIN_TASKS", 1280);
  if (p->dtype != YV7_DT_F16 || i >= p->ops.size()) return 0;
  const bool forced = p->op_variant[i] == 305;
  if (!forced && !all) return 0;
  auto eligible = [&](size_t j) {
    const auto& o = p->ops[j];
    return o.kind == YV7_OP_CONV && !is_f8(o) && o.k == 3 && o.s == 1 && o.pad == 1 && !o.pool && o.src2 < 0 &&
           p->op_variant[j] == (j == i && forced ? 305 : 0) && o.act == p->ops[i].act;
  };
  if (!eligible(i)) return 0;
  size_t n = 1;
  while (n < (size_t)yv7::CHAIN_MAX && i + n < p->ops.size() && eligible(i + n)) {
    const auto& a = p->ops[i + n - 1];
    const auto& b = p->ops[i + n];
    if (b.src != a.dst || b.src_coff != a.dst_coff || b.cin != a.cout) break;
    ++n;
  }
  for (; n >= 2; --n) {
    // no layer's output may overlap the chain's input slice or another layer's output
    bool ok = true;
    for (size_t j = 0; j < n && ok; ++j) {
      const auto& oj = p->ops[i + j];
      if (overlap(oj.dst, oj.dst_coff, oj.cout, p->ops[i].src, p->ops[i].src_coff, p->ops[i].cin)) ok = false;
      for (size_t k = 0; k < j && ok; ++k) {
        const auto& ok_ = p->ops[i + k];
        if (overlap(oj.dst, oj.dst_coff, oj.cout, ok_.dst, ok_.dst_coff, ok_.cout)) ok = false;
      }
    }
    if (!ok) continue;
    std::memset(c, 0, sizeof(*c));
    c->nl = (int)n;
    for (size_t j = 0; j < n && ok; ++j) {
      yv7::ConvParams& q = c->p[j];
      ok = bind_conv(p, i + j, l, wsb, &q);
      q.variant = 0;
      int cfg = yv7::lr_default_cfg(q);
      if (cfg == 0 || cfg == 2) ++cfg;   // 128-channel tiles -> 64-channel (conv_lr.hip chain_forms)
      if (cfg == 5 || cfg == 6) cfg = 1;  // 160-pixel tiles (H % 10 == 0) -> the 80-pixel 64-channel form
      if (cfg < 0 || (j > 1 && cfg != c->cfg1)) ok = false;
      if (j == 0) c->cfg0 = cfg;
      if (j == 1) c->cfg1 = cfg;
    }
    if (!ok || !yv7::chain_supported(*c)) continue;
    // (YV7_CHAIN=1: only where a layer has few tiles, its ramp and tail dominating)
    if (!forced && yv7::chain_tasks(*c) > max_tasks * (long)n) return 0;
    c->ctr = reinterpret_cast<int*>(wsb + l.chain_off);
    return (int)n;
  }
  return 0;
}

extern "C" {

int yv7_forward(yv7_plan* p, const void* x, int x_dtype, int B, int H, int W, float* z, float* raw,
                yv7_row_best* rowbest, void* ws, size_t ws_bytes, void* stream) {
  return forward_impl(p, x, x_dtype, B, H, W, z, raw, rowbest, ws, ws_bytes, stream, nullptr);
}

int yv7_op_kernels(yv7_plan* p, int B, int H, int W, int x_dtype, char* buf, size_t bytes) {
  if (!p || !buf || bytes == 0) return fail(YV7_E_ARG, "yv7_op_kernels: null argument");
  std::vector<std::vector<const void*>> ks;
  // dry run: the op loop with placeholder pointers (nothing is launched or dereferenced on the host)
  static const float dummy[4] = {0, 0, 0, 0};
  void* ph = const_cast<float*>(dummy);
  if (int rc = forward_impl(p, ph, x_dtype, B, H, W, static_cast<float*>(ph), nullptr, nullptr, ph, 0, nullptr, &ks))
    return rc;
  std::string out;
  for (size_t i = 0; i < ks.size(); ++i) {
    out += std::to_string(i);
    for (size_t k = 0; k < ks[i].size(); ++k) {
      const char* mangled = hipKernelNameRefByPtr(ks[i][k], nullptr);
      std::string name = mangled ? mangled : "?";
      int st = 0;
      char* dem = mangled ? abi::__cxa_demangle(mangled, nullptr, nullptr, &st) : nullptr;
      if (dem && st == 0) name = dem;
      std::free(dem);
      out += (k ? "|" : "\t") + name;
    }
    out += "\n";
  }
  if (out.size() + 1 > bytes) return fail(YV7_E_ARG, "yv7_op_kernels: buffer too small (need " + std::to_string(out.size() + 1) + ")");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return 0;
}

}  // extern "C"
