// libyv7 plans: descriptor validation, creation (packed weights to HBM) and destruction, the live-profiling
// events and the per-op kernel variant override.
//
// A plan is the deploy-form network (attempt_load -> Model.fuse, models/experimental.py:247-270)
// as a flat list of ops over NHWC tensors.
#include <cstdlib>
#include <cstring>

#include "plan.h"

using namespace yv7rt;

namespace {

// The rejections of one op of the descriptor (validate_net).
int validate_op(const yv7_net_desc* d, int i, size_t nbytes) {
  const auto& o = d->ops[i];
  const int vec = d->dtype == YV7_DT_F16 ? 8 : 4;
  const std::string op = "yv7_plan_create: op " + std::to_string(i);
  const bool src_ok = o.kind == YV7_OP_INPUT || o.kind == YV7_OP_STEM || (o.src >= 0 && o.src < d->n_tensors);
  const bool dst_ok = o.kind == YV7_OP_DETECT || (o.dst >= 0 && o.dst < d->n_tensors);
  if (!src_ok || !dst_ok) return fail(YV7_E_ARG, op + " bad tensor id");
  if (o.kind < YV7_OP_INPUT || o.kind > YV7_OP_ADD) return fail(YV7_E_ARG, op + " unknown op kind");
  if (o.kind == YV7_OP_ADD) {
    if (o.src2 < 0 || o.src2 >= d->n_tensors) return fail(YV7_E_ARG, op + " bad second-operand tensor id");
    if (o.cout <= 0 || o.cout % vec) return fail(YV7_E_ARG, op + " add channels not a multiple of the vector");
    if (o.src2_coff < 0 || o.src2_coff % vec || o.src2_coff + o.cout > d->tensors[o.src2].channels)
      return fail(YV7_E_ARG, op + " second-operand channel slice out of range");
    if (d->tensors[o.src].shift != d->tensors[o.dst].shift || d->tensors[o.src2].shift != d->tensors[o.dst].shift)
      return fail(YV7_E_ARG, op + " add operands and result differ in resolution");
    // (conservative: an exactly in-place add would be safe — a lane reads its vectors before it writes them —
    // but no graph produces one, and a partial overlap never is)
    if (overlap(o.dst, o.dst_coff, o.cout, o.src, o.src_coff, o.cout) ||
        overlap(o.dst, o.dst_coff, o.cout, o.src2, o.src2_coff, o.cout))
      return fail(YV7_E_ARG, op + " add result overlaps an operand");
  } else if (o.kind == YV7_OP_CONV && o.src2 != -1) {
    // the residual of a conv: added at the output's (pixel, channel) in the epilogue of the fp16 tile / ring kernels
    if (d->dtype != YV7_DT_F16 || o.wfmt != YV7_WFMT_PLAN || o.pool != 0)
      return fail(YV7_E_ARG, op + " residual needs an fp16 plan, plan-format weights and no pool");
    if (o.src2 < 0 || o.src2 >= d->n_tensors) return fail(YV7_E_ARG, op + " bad residual tensor id");
    if (o.cout <= 0 || o.cout % vec) return fail(YV7_E_ARG, op + " residual channels not a multiple of the vector");
    if (o.src2_coff < 0 || o.src2_coff % vec || o.src2_coff + o.cout > d->tensors[o.src2].channels)
      return fail(YV7_E_ARG, op + " residual channel slice out of range");
    if (d->tensors[o.src2].shift != d->tensors[o.dst].shift)
      return fail(YV7_E_ARG, op + " residual and result differ in resolution");
    if (overlap(o.dst, o.dst_coff, o.cout, o.src2, o.src2_coff, o.cout))
      return fail(YV7_E_ARG, op + " residual overlaps the result");
  } else if (o.src2 != -1) {
    return fail(YV7_E_ARG, op + " takes no second operand (src2 must be -1)");
  }
  if (o.kind == YV7_OP_CONV || o.kind == YV7_OP_DETECT) {
    if (o.cin % vec || (o.kind == YV7_OP_CONV && o.cout % vec))
      return fail(YV7_E_ARG, op + " channels not a multiple of the vector");
    if (o.kind == YV7_OP_CONV && o.pool != 0 &&
        (o.pool != 2 || d->dtype != YV7_DT_F16 || o.k != 1 || o.s != 2 || o.pad != 0 || o.wfmt != YV7_WFMT_PLAN))
      return fail(YV7_E_ARG, op + " bad pooled conv (fp16 plans, pool 2 with k 1, s 2, pad 0)");
    if (o.kind == YV7_OP_CONV && o.wfmt != YV7_WFMT_PLAN &&
        (o.wfmt != YV7_WFMT_FP8 || d->dtype != YV7_DT_F16 || o.k != 1 || o.s != 1 || o.pad != 0 || o.cout > 1024 ||
         !(o.xscale > 0.0f) || o.xscale > 1e30f || o.s_off < 0 || (size_t)o.s_off + sizeof(float) * o.cout > nbytes))
      return fail(YV7_E_ARG, op + " bad fp8 conv (fp16 plans, 1x1 stride 1, cout <= 1024, xscale > 0, scales in blob)");
    const size_t wb = (size_t)((o.cout + 31) / 32 * 32) * kpad_of(o) * (is_f8(o) ? 1 : elem_size(d->dtype));
    if (o.w_off < 0 || o.b_off < 0 || (size_t)o.w_off + wb > nbytes ||
        (size_t)o.b_off + sizeof(float) * o.cout > nbytes)
      return fail(YV7_E_ARG, op + " weight range outside blob");
    if (o.k < 1 || o.s < 1 || o.pad < 0 || o.pad > YV7_BORDER || o.k - 1 - o.pad > YV7_BORDER)
      return fail(YV7_E_ARG, op + " window reaches past the tensors' zero frame (needs pad <= 1, k - 1 - pad <= 1)");
    if (o.kind == YV7_OP_DETECT && (o.level < 0 || o.level >= d->nl || o.cout != d->na * d->no || o.k != 1))
      return fail(YV7_E_ARG, "yv7_plan_create: bad detect op");
  }
  if (o.kind == YV7_OP_INPUT) {
    // cout: the channels the op packs (plan.h input_packed)
    const int c = input_packed(o);
    if (c < 1 || c > d->tensors[o.dst].channels)
      return fail(YV7_E_ARG, op + " input channels outside 1 .. the destination tensor's channels");
    if (o.k == 2 && c % 4)
      return fail(YV7_E_ARG, op + " reorganised input channels not a multiple of 4");
  }
  if (o.kind == YV7_OP_STEM) {
    if (d->dtype != YV7_DT_F16 || !yv7::stem_supported(o.cin, o.cout, o.cout2, o.s) || o.k != 3 || o.act != o.act2 ||
        o.dst_coff % vec || o.dst_coff + o.cout2 > d->tensors[o.dst].channels)
      return fail(YV7_E_ARG, "yv7_plan_create: unsupported stem op");
    // cin 12: the w6 front end (ReOrg fused), conv A's K = tap * 16 + ci; else K = tap * cin + ci, cin 1 .. 4
    const int ka = o.cin == 12 ? 9 * 16 : 9 * o.cin;
    const size_t wa = (size_t)o.cout * ((ka + 63) / 64 * 64) * 2, wb = (size_t)o.cout2 * ((9 * o.cout + 63) / 64 * 64) * 2;
    if (o.w_off < 0 || o.w2_off < 0 || (size_t)o.w_off + wa > nbytes || (size_t)o.w2_off + wb > nbytes ||
        (size_t)o.b_off + 4 * o.cout > nbytes || (size_t)o.b2_off + 4 * o.cout2 > nbytes)
      return fail(YV7_E_ARG, "yv7_plan_create: stem weight range outside blob");
  } else if (o.kind != YV7_OP_INPUT && o.kind != YV7_OP_DETECT) {
    const int src_c = d->tensors[o.src].channels, dst_c = d->tensors[o.dst].channels;
    const int cin = o.kind == YV7_OP_CONV ? o.cin : o.cout;
    if (o.src_coff < 0 || o.src_coff + cin > src_c || o.dst_coff < 0 || o.dst_coff + o.cout > dst_c ||
        o.src_coff % vec || o.dst_coff % vec)
      return fail(YV7_E_ARG, op + " channel slice out of range");
  }
  return 0;
}

// 3x3 / stride-1 or 2 / pad-1 fp16 convs of a shape the fragment kernels accept (conv_lr.hip lr_supported:
// cin / 32 in {2, 4, 6, 8, 12, 16, 24}, cout % 16 == 0, cout <= 1024; conv_s2.hip: cin 64 / 128) get a
// fragment-packed weight copy, and so do 1x1 stride-1 convs with 128 / 256 / 512 inputs (conv_w1.hip) —
// none at all with YV7_FRAG=0 (every fragment kernel then stays off: conv_lr, the register-weight 3x3 / 1x1
// kernels and the register-weight Detect head; the forced variants 270-288 / 290-295 / 302-303 fall back to
// the tuned kernel).  YV7_LR=0 only takes conv_lr out of the dispatch (it used to switch the
// packing, i.e. four kernel families, off at once).  Per fp16 plan: yolov7 54.0 MB (3x3 49.8 + 1x1 4.1) beside its 73.9 MB
// blob, yolov7-w6 112.4 MB, yolov7-tiny 10.3 MB.
bool wants_frag(int dtype, const yv7_op_desc& o) {
  static const int lr = yv7::env_int("YV7_FRAG", 1);
  const int nch = o.cin / 32;
  // the Detect head conv with K = 256 / 512 (conv_det_rw_kernel: the weights resident in VGPRs)
  if (dtype == YV7_DT_F16 && o.kind == YV7_OP_DETECT)
    return lr && o.k == 1 && (o.cin == 256 || o.cin == 512) && o.cout <= 256;
  if (!lr || dtype != YV7_DT_F16 || o.kind != YV7_OP_CONV || is_f8(o) || o.pool || o.cout % 16 || o.cout > 1024 ||
      o.src2 >= 0)   // (a conv with a residual runs the tile / ring kernels only)
    return false;
  if (o.k == 1)   // conv_w1.hip: 1x1 stride 1 with 128 / 256 / 512 inputs
    return o.s == 1 && o.pad == 0 && (o.cin == 128 || o.cin == 256 || o.cin == 512);
  return o.k == 3 && (o.s == 1 || o.s == 2) && o.pad == 1 && o.cin % 32 == 0 &&
         (nch == 2 || nch == 4 || nch == 6 || nch == 8 || nch == 12 || nch == 16 || nch == 24);
}

// The plan's device memory: the weight blob, the zero page and the fragment-packed copies of the 3x3 / 1x1
// weights (conv_lr.hip), packed on the device from the plan's own copy.  On failure *where names the step;
// the caller destroys the plan, which frees whatever was allocated.
hipError_t upload(yv7_plan* p, const void* weights, const char** where) {
  hipError_t e = hipSuccess;
  *where = "hipMalloc(weights)";
  if (p->wbytes && (e = hipMalloc(&p->weights, p->wbytes)) != hipSuccess) return e;
  *where = "hipMemcpy(weights)";
  if (p->wbytes && (e = hipMemcpy(p->weights, weights, p->wbytes, hipMemcpyDefault)) != hipSuccess) return e;
  *where = "hipMalloc(zero page)";
  if ((e = hipMalloc(&p->zero, 4096)) != hipSuccess || (e = hipMemset(p->zero, 0, 4096)) != hipSuccess) return e;
  *where = "yv7_plan_create: fragment packing";
  p->wf_off.assign(p->ops.size(), -1);
  size_t wf_total = 0;
  for (size_t i = 0; i < p->ops.size(); ++i)
    if (wants_frag(p->dtype, p->ops[i])) {
      p->wf_off[i] = (int64_t)wf_total;
      wf_total = align256(wf_total + yv7::frag_bytes(p->ops[i].cin, p->ops[i].cout, p->ops[i].k * p->ops[i].k));
    }
  if (!wf_total) return hipSuccess;
  // packed on a private stream and waited for on that stream only (a device-wide sync here
  // made plan creation wait for other plans' forwards on their own streams).  A blocking stream: its
  // work is ordered after the null stream's weight copy above.
  hipStream_t ps = nullptr;
  e = hipMalloc(&p->wfrag, wf_total);
  if (e == hipSuccess) e = hipStreamCreate(&ps);
  for (size_t i = 0; e == hipSuccess && i < p->ops.size(); ++i)
    if (p->wf_off[i] >= 0)
      e = yv7::pack_frag(reinterpret_cast<const unsigned char*>(p->weights) + p->ops[i].w_off, kpad_of(p->ops[i]),
                         p->ops[i].cin, p->ops[i].cout, p->ops[i].k * p->ops[i].k,
                         reinterpret_cast<unsigned char*>(p->wfrag) + p->wf_off[i], ps);
  if (e == hipSuccess) e = hipStreamSynchronize(ps);
  if (ps) (void)hipStreamDestroy(ps);
  return e;
}

void free_events(yv7_plan* p) {
  for (auto e : p->events) (void)hipEventDestroy(e);
  p->events.clear();
  p->prof_max = p->prof_used = 0;
}

// Kernel variants a caller may force per op: every real kernel configuration of the fp16 dispatch
// (conv_f16.hip: the `abi` rows of its forced-variant table), never the microbenchmark hooks (90-99, 298;
// ws64's 12-14 and 16), which skip work on purpose.
bool variant_allowed(const yv7_op_desc& o, int v) {
  if (v == 0) return true;
  const int kind = o.kind;
  if (is_f8(o)) return v == 81 || v == 82;   // fp8 1x1: staged quantize pass / fused quantization
  if (kind == YV7_OP_DETECT) return v == 89 || v == 92 || v == 94 || v == 97 || v == 99;   // 89: conv_det_nc.hip
  if (v == 305) return o.k == 3 && o.s == 1;   // the chained launch of the 3x3 stack starting here (find_chain)
  return yv7::conv_f16_variant_is_config(v);
}

}  // namespace

int yv7rt::validate_net(const yv7_net_desc* d, size_t nbytes) {
  if (d->abi_version != YV7_ABI_VERSION) return fail(YV7_E_ABI, "yv7_plan_create: abi_version mismatch");
  if (d->dtype != YV7_DT_F32 && d->dtype != YV7_DT_F16) return fail(YV7_E_ARG, "yv7_plan_create: bad dtype");
  if (d->n_tensors <= 0 || d->n_ops <= 0 || !d->tensors || !d->ops)
    return fail(YV7_E_ARG, "yv7_plan_create: empty network");
  if (d->nl <= 0 || d->nl > 8 || d->na <= 0 || d->na > 4 || d->no < 6 || d->no - 5 > 128)
    return fail(YV7_E_ARG, "yv7_plan_create: unsupported head geometry (nl<=8, na<=4, nc<=128)");
  const int vec = d->dtype == YV7_DT_F16 ? 8 : 4;
  for (int i = 0; i < d->n_tensors; ++i)
    if (d->tensors[i].channels <= 0 || d->tensors[i].channels % vec || d->tensors[i].shift < 0 ||
        d->tensors[i].shift > d->max_shift)
      return fail(YV7_E_ARG, "yv7_plan_create: tensor " + std::to_string(i) + " has bad channels/shift");
  for (int i = 0; i < d->n_ops; ++i)
    if (int rc = validate_op(d, i, nbytes)) return rc;
  return 0;
}

extern "C" {

int yv7_plan_create(const yv7_net_desc* d, const void* weights, size_t nbytes, int device, yv7_plan** out) {
  if (!d || !out || (!weights && nbytes)) return fail(YV7_E_ARG, "yv7_plan_create: null argument");
  *out = nullptr;
  if (int rc = validate_net(d, nbytes)) return rc;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(YV7_E_DEVICE, std::string("libyv7 is built for gfx950; device is ") + prop.gcnArchName);

  yv7_plan* p = new yv7_plan();
  p->device = device;
  p->dtype = d->dtype;
  p->tensors.assign(d->tensors, d->tensors + d->n_tensors);
  p->ops.assign(d->ops, d->ops + d->n_ops);
  p->op_variant.assign(p->ops.size(), 0);
  p->nl = d->nl;
  p->na = d->na;
  p->no = d->no;
  p->max_shift = d->max_shift;
  p->stride.assign(d->stride, d->stride + d->nl);
  p->anchor_grid.assign(d->anchor_grid, d->anchor_grid + d->nl * d->na * 2);
  p->wbytes = nbytes;
  const char* where = nullptr;
  if ((e = upload(p, weights, &where)) != hipSuccess) {
    yv7_plan_destroy(p);
    return hip_fail(e, where);
  }
  *out = p;
  return 0;
}

void yv7_plan_destroy(yv7_plan* p) {
  if (!p) return;
  free_events(p);
  if (p->weights) (void)hipFree(p->weights);
  if (p->zero) (void)hipFree(p->zero);
  if (p->wfrag) (void)hipFree(p->wfrag);
  delete p;
}

int yv7_profile_enable(yv7_plan* p, int max_forwards) {
  if (!p || max_forwards < 0) return fail(YV7_E_ARG, "yv7_profile_enable");
  free_events(p);
  if (max_forwards == 0) return 0;
  const size_t n = (size_t)max_forwards * 2 * p->ops.size();
  p->events.resize(n);
  for (size_t i = 0; i < n; ++i) {
    hipError_t e = hipEventCreate(&p->events[i]);
    if (e != hipSuccess) {
      p->events.resize(i);
      free_events(p);
      return hip_fail(e, "hipEventCreate");
    }
  }
  p->prof_max = max_forwards;
  return 0;
}

int yv7_profile_read(yv7_plan* p, int* n_forwards, float* op_ms) {
  if (!p || !n_forwards || !op_ms) return fail(YV7_E_ARG, "yv7_profile_read");
  const size_t nops = p->ops.size();
  for (size_t i = 0; i < nops; ++i) op_ms[i] = 0.f;
  *n_forwards = p->prof_used;
  for (int f = 0; f < p->prof_used; ++f) {
    hipEvent_t* ev = &p->events[(size_t)f * 2 * nops];
    hipError_t e = hipEventSynchronize(ev[2 * nops - 1]);
    if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize");
    for (size_t i = 0; i < nops; ++i) {
      float ms = 0.f;
      if ((e = hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1])) != hipSuccess) return hip_fail(e, "hipEventElapsedTime");
      op_ms[i] += ms;
    }
  }
  return 0;
}

int yv7_set_op_variant(yv7_plan* p, int op, int variant) {
  if (!p || op < 0 || op >= (int)p->ops.size()) return fail(YV7_E_ARG, "yv7_set_op_variant: bad op index");
  const auto& o = p->ops[op];
  if (o.kind != YV7_OP_CONV && o.kind != YV7_OP_DETECT)
    return fail(YV7_E_ARG, "yv7_set_op_variant: op " + std::to_string(op) + " is not a CONV / DETECT op");
  if (!variant_allowed(o, variant))
    return fail(YV7_E_ARG, "yv7_set_op_variant: variant " + std::to_string(variant) + " is not a kernel configuration");
  if (o.kind == YV7_OP_DETECT && o.cout > 256 && (variant == 92 || variant == 97 || variant == 99))
    return fail(YV7_E_ARG, "yv7_set_op_variant: variant " + std::to_string(variant) + " is a 256-channel Detect form; op " +
                               std::to_string(op) + " has na * no = " + std::to_string(o.cout) + " > 256");
  if (o.kind == YV7_OP_CONV && o.src2 >= 0 && variant != 0 && !yv7::conv_f16_variant_has_residual(variant))
    return fail(YV7_E_ARG, "yv7_set_op_variant: op " + std::to_string(op) + " carries a residual; variant " +
                               std::to_string(variant) + " is of a kernel family without the residual epilogue");
  p->op_variant[op] = variant;
  return 0;
}

}  // extern "C"
