// libyv7 workspace layout: where a batch's tensors and scratch lie (one function, computed per call), the conv
// operand binder that reads it, and the ABI's layout queries.
#include <algorithm>
#include <cstring>

#include "plan.h"

using namespace yv7rt;

namespace {

size_t tensor_bytes(const yv7_plan* p, const yv7_tensor_desc& t, int B, int H, int W) {
  return yv7::bordered_pixels(B, H >> t.shift, W >> t.shift) * t.channels * elem_size(p->dtype);
}

int check_hw(const yv7_plan* p, int B, int H, int W) {
  const int m = (1 << p->max_shift) - 1;
  if (B <= 0 || H <= 0 || W <= 0 || (H & m) || (W & m))
    return fail(YV7_E_SHAPE, "input H and W must be positive multiples of " + std::to_string(1 << p->max_shift) +
                                 " (got B=" + std::to_string(B) + " H=" + std::to_string(H) + " W=" +
                                 std::to_string(W) + ")");
  // kernels address a tensor with 32-bit byte offsets (buffer loads)
  for (const auto& t : p->tensors)
    if (tensor_bytes(p, t, B, H, W) >= (size_t(1) << 31))
      return fail(YV7_E_SHAPE, "batch too large: an activation tensor would exceed 2 GiB (split the batch)");
  return 0;
}

// Geometry / operand fields of a CONV or DETECT op's kernel parameters (bind_conv adds the pointers).
yv7::ConvParams conv_params(const yv7_plan* p, size_t op, int B, int H, int W) {
  const yv7_op_desc& o = p->ops[op];
  const auto& ti = p->tensors[o.src];
  const size_t es = elem_size(p->dtype);
  yv7::ConvParams c;
  std::memset(&c, 0, sizeof(c));
  c.B = B;
  c.H = H >> ti.shift;
  c.W = W >> ti.shift;
  c.xc = ti.channels;
  c.xoff = o.src_coff;
  c.cin = o.cin;
  c.Ho = (c.H + 2 * o.pad - o.k) / o.s + 1;
  c.Wo = (c.W + 2 * o.pad - o.k) / o.s + 1;
  c.cout = o.cout;
  c.k = o.k;
  c.s = o.s;
  c.pad = o.pad;
  c.act = o.act;
  c.pool = o.kind == YV7_OP_CONV ? o.pool : 0;
  c.kpad = kpad_of(o);
  c.K = o.k * o.k * o.cin;
  c.M = B * c.Ho * c.Wo;
  c.xbytes = (uint32_t)tensor_bytes(p, ti, B, H, W);
  c.wbytes = (uint32_t)((size_t)((o.cout + 31) / 32 * 32) * c.kpad * es);
  c.variant = p->op_variant[op] == 305 ? 0 : p->op_variant[op];   // 305: a chain start (find_chain)
  if (p->wfrag && p->wf_off[op] >= 0) {
    c.wf = reinterpret_cast<const unsigned char*>(p->wfrag) + p->wf_off[op];
    c.wfbytes = (uint32_t)yv7::frag_bytes(o.cin, o.cout, o.k * o.k);
  }
  return c;
}

// The scratch block behind the tensors (l->off, B, H, W are set; tensors_end: where the tensors stop).
void layout_scratch(const yv7_plan* p, size_t tensors_end, Layout* l) {
  const bool f16 = p->dtype == YV7_DT_F16;
  for (size_t i = 0; f16 && i < p->ops.size(); ++i) {
    const auto& o = p->ops[i];
    if (is_f8(o)) {
      const int sh = p->tensors[o.src].shift;
      l->f8_bytes = std::max(l->f8_bytes, (size_t)l->B * (l->H >> sh) * (l->W >> sh) * kpad_of(o));
    } else if (o.kind == YV7_OP_CONV) {
      const yv7::ConvParams c = conv_params(p, i, l->B, l->H, l->W);
      l->part_bytes = std::max(l->part_bytes, yv7::conv_splitk_part_bytes(c));
      l->cnt_n = std::max(l->cnt_n, yv7::conv_splitk_tiles(c));
    }
  }
  l->part_off = tensors_end;
  l->cnt_off = align256(l->part_off + l->part_bytes);
  l->f8_off = align256(l->cnt_off + (size_t)l->cnt_n * 4);
  l->chain_off = align256(l->f8_off + l->f8_bytes);
  yv7::ChainParams c;
  for (size_t i = 0; f16 && i < p->ops.size(); ++i)
    if (find_chain(p, i, *l, nullptr, &c)) l->chain_bytes = std::max(l->chain_bytes, yv7::chain_counter_bytes(c));
  l->end = align256(l->chain_off + l->chain_bytes);
}

}  // namespace

int yv7rt::plan_layout(const yv7_plan* p, int B, int H, int W, Layout* l) {
  if (int rc = check_hw(p, B, H, W)) return rc;
  *l = Layout{};
  l->B = B;
  l->H = H;
  l->W = W;
  l->off.resize(p->tensors.size());
  size_t o = 0;
  for (size_t i = 0; i < p->tensors.size(); ++i) {
    l->off[i] = o;
    o = align256(o + tensor_bytes(p, p->tensors[i], B, H, W));
  }
  layout_scratch(p, o, l);
  l->nrows = (int)yv7_num_rows(p, H, W);
  std::vector<int> lvl_rows(p->nl, 0);
  for (const auto& op : p->ops)
    if (op.kind == YV7_OP_DETECT) {
      const int s = p->tensors[op.src].shift;
      lvl_rows[op.level] = p->na * (H >> s) * (W >> s);
    }
  int acc = 0;
  size_t racc = 0;
  l->row_off.resize(p->nl);
  l->raw_off.resize(p->nl);
  for (int lv = 0; lv < p->nl; ++lv) {
    l->row_off[lv] = acc;
    l->raw_off[lv] = racc;
    acc += lvl_rows[lv];
    racc += (size_t)B * lvl_rows[lv] * p->no;
  }
  return 0;
}

bool yv7rt::bind_conv(const yv7_plan* p, size_t i, const Layout& l, unsigned char* wsb, yv7::ConvParams* c) {
  const yv7_op_desc& o = p->ops[i];
  const unsigned char* wb = reinterpret_cast<const unsigned char*>(p->weights);
  *c = conv_params(p, i, l.B, l.H, l.W);
  c->x = wsb + l.off[o.src];
  c->w = wb + o.w_off;
  c->bias = reinterpret_cast<const float*>(wb + o.b_off);
  c->zero = p->zero;
  c->part = reinterpret_cast<float*>(wsb + l.part_off);
  c->part_bytes = l.part_bytes;
  c->cnt = reinterpret_cast<int*>(wsb + l.cnt_off);
  c->cnt_n = l.cnt_n;
  if (o.kind != YV7_OP_CONV) return true;
  const auto& to = p->tensors[o.dst];
  c->y = wsb + l.off[o.dst];
  c->yc = to.channels;
  c->yoff = o.dst_coff;
  if (o.src2 >= 0) {   // the residual (validate_net: fp16 plan, the output's resolution)
    const auto& tr = p->tensors[o.src2];
    c->res = wsb + l.off[o.src2];
    c->rbytes = (uint32_t)tensor_bytes(p, tr, l.B, l.H, l.W);
    c->rc = tr.channels;
    c->roff = o.src2_coff;
  }
  return c->Ho == (l.H >> to.shift) && c->Wo == (l.W >> to.shift);
}

void yv7rt::forget_workspaces(yv7_plan* p, const void* ws, size_t bytes) {
  const char* lo = reinterpret_cast<const char*>(ws);
  std::vector<yv7_plan::WsKey> keep;
  for (const auto& w : p->ws_ready) {
    const char* wl = reinterpret_cast<const char*>(w.ptr);
    if (wl + w.bytes <= lo || lo + bytes <= wl) keep.push_back(w);
  }
  p->ws_ready = keep;
}

extern "C" {

size_t yv7_workspace_bytes(const yv7_plan* p, int B, int H, int W) {
  Layout l;
  return !p || plan_layout(p, B, H, W, &l) ? 0 : l.end;
}

int yv7_workspace_forget(yv7_plan* p, const void* ws, size_t bytes) {
  if (!p || !ws) return fail(YV7_E_ARG, "yv7_workspace_forget: null argument");
  forget_workspaces(p, ws, bytes ? bytes : 1);
  return 0;
}

int64_t yv7_num_rows(const yv7_plan* p, int H, int W) {
  if (!p) return -1;
  int64_t n = 0;
  for (const auto& o : p->ops)
    if (o.kind == YV7_OP_DETECT) {
      const int s = p->tensors[o.src].shift;
      n += (int64_t)p->na * (H >> s) * (W >> s);
    }
  return n;
}

int yv7_tensor_info(const yv7_plan* p, int id, int B, int H, int W, int64_t* offset, int64_t* dims4) {
  if (!p || id < 0 || id >= (int)p->tensors.size() || !offset || !dims4) return fail(YV7_E_ARG, "yv7_tensor_info");
  Layout l;
  if (int rc = plan_layout(p, B, H, W, &l)) return rc;
  *offset = (int64_t)l.off[id];
  const auto& t = p->tensors[id];
  dims4[0] = B;
  dims4[1] = (H >> t.shift) + 2 * YV7_BORDER;
  dims4[2] = (W >> t.shift) + 2 * YV7_BORDER;
  dims4[3] = t.channels;
  return 0;
}

int yv7_f8_scratch_info(const yv7_plan* p, int B, int H, int W, int64_t* offset, int64_t* bytes) {
  if (!p || !offset || !bytes) return fail(YV7_E_ARG, "yv7_f8_scratch_info");
  Layout l;
  if (int rc = plan_layout(p, B, H, W, &l)) return rc;
  *offset = (int64_t)l.f8_off;
  *bytes = (int64_t)l.f8_bytes;
  return 0;
}

}  // extern "C"
