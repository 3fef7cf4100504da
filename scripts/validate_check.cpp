// Host-only check of validate_net (csrc/plan_create.cpp) for a sanitizer build: the descriptors of
// tests/test_plan_validate.py, each mutation's code and message.  No device is touched.  From the repository
// root, after the library is built:
//   hipcc -std=c++17 -x hip --offload-host-only -Xarch_host -fsanitize=address,undefined -g scripts/validate_check.cpp \
//     yolo-series_amd/csrc/plan_create.cpp yolo-series_amd/csrc/runtime.cpp -x none yolo-series_amd/yv7/libyv7.so \
//     -Wl,-rpath,$PWD/yolo-series_amd/yv7 -o validate_check && ./validate_check
#include <cstdio>
#include <cstring>
#include <functional>

#include "../yolo-series_amd/csrc/plan.h"

struct Net {
  yv7_net_desc d;
  std::vector<yv7_tensor_desc> t;
  std::vector<yv7_op_desc> ops;
  size_t nbytes = 12544;
  float stride[1] = {8.f}, anchors[8] = {10, 10, 10, 10, 10, 10, 10, 10};
};

static yv7_op_desc op(int kind) {
  yv7_op_desc o;
  std::memset(&o, 0, sizeof(o));
  o.kind = kind;
  o.k = o.s = 1;
  o.src2 = -1;   // no second operand
  return o;
}

static yv7_op_desc stem() {
  yv7_op_desc o = op(YV7_OP_STEM);
  o.cin = 3, o.cout = 32, o.cout2 = 64, o.k = 3, o.dst = 1;
  return o;
}

static int check(const char* want, const std::function<void(Net&)>& mutate) {
  Net n;
  std::memset(&n.d, 0, sizeof(n.d));
  n.t = {{8, 0}, {16, 0}};
  yv7_op_desc in = op(YV7_OP_INPUT), conv = op(YV7_OP_CONV), det = op(YV7_OP_DETECT);
  conv.cin = 8, conv.dst = 1, conv.cout = 16, conv.k = 3, conv.pad = 1, conv.b_off = 8192;
  det.src = 1, det.cin = 16, det.cout = 6, det.w_off = 8256, det.b_off = 12352;
  n.ops = {in, conv, det};
  n.d.abi_version = YV7_ABI_VERSION, n.d.dtype = YV7_DT_F16, n.d.nl = n.d.na = 1, n.d.no = 6;
  n.d.n_ops = -1;
  mutate(n);
  n.d.n_tensors = (int)n.t.size(), n.d.tensors = n.t.data(), n.d.ops = n.ops.data();
  if (n.d.n_ops < 0) n.d.n_ops = (int)n.ops.size();
  n.d.stride = n.stride, n.d.anchor_grid = n.anchors;
  const int rc = yv7rt::validate_net(&n.d, n.nbytes);
  const bool ok = want ? rc == YV7_E_ARG && std::strstr(yv7_last_error(), want) : rc == 0;
  std::printf("%s  rc %d  %s\n", ok ? "ok  " : "FAIL", rc, rc ? yv7_last_error() : "(valid)");
  return ok ? 0 : 1;
}

int main() {
  int bad = check(nullptr, [](Net&) {});
  bad += check("bad dtype", [](Net& n) { n.d.dtype = 2; });
  bad += check("empty network", [](Net& n) { n.d.n_ops = 0; });
  bad += check("unsupported head geometry", [](Net& n) { n.d.na = 5; });
  bad += check("tensor 1 has bad channels/shift", [](Net& n) { n.t[1].channels = 12; });
  bad += check("op 1 bad tensor id", [](Net& n) { n.ops[1].src = 7; });
  bad += check("not a multiple of the vector", [](Net& n) { n.ops[1].cin = 4; });
  bad += check("bad pooled conv", [](Net& n) { n.ops[1].pool = 2; });
  bad += check("bad fp8 conv", [](Net& n) { n.ops[1].wfmt = YV7_WFMT_FP8, n.ops[1].xscale = 1.f; });
  bad += check("op 2 weight range outside blob", [](Net& n) { n.nbytes = 12352; });
  bad += check("window reaches past", [](Net& n) { n.ops[1].pad = 2; });
  bad += check("bad detect op", [](Net& n) { n.ops[2].cout = 12; });
  bad += check("unsupported stem op", [](Net& n) { n.ops.insert(n.ops.begin() + 1, stem()); });
  bad += check("stem weight range outside blob", [](Net& n) {
    n.t[1].channels = 64;
    yv7_op_desc s = stem();
    s.w2_off = 1 << 20;
    n.ops.insert(n.ops.begin() + 1, s);
  });
  bad += check("op 1 channel slice out of range", [](Net& n) { n.ops[1].dst_coff = 8; });
  bad += check("op 2 channel slice out of range", [](Net& n) {
    yv7_op_desc m = op(YV7_OP_MAXPOOL);
    m.src = m.dst = 1, m.dst_coff = 8, m.cout = 16;
    n.ops.insert(n.ops.begin() + 2, m);
  });
  // ADD (t1 + t2 -> t3, 16 channels each) and the second-operand field of the other kinds
  auto with_add = [](Net& n) {
    n.t = {{8, 0}, {16, 0}, {16, 0}, {16, 0}};
    yv7_op_desc a = op(YV7_OP_ADD);
    a.src = 1, a.src2 = 2, a.dst = 3, a.cout = 16;
    n.ops.insert(n.ops.begin() + 2, a);
  };
  bad += check(nullptr, with_add);
  bad += check("op 2 bad second-operand tensor id", [&](Net& n) { with_add(n), n.ops[2].src2 = 9; });
  bad += check("op 2 add channels not a multiple of the vector", [&](Net& n) { with_add(n), n.ops[2].cout = 12; });
  bad += check("op 2 second-operand channel slice out of range", [&](Net& n) { with_add(n), n.ops[2].src2_coff = 8; });
  bad += check("op 2 add operands and result differ in resolution", [&](Net& n) {
    with_add(n), n.t[2].shift = 1, n.d.max_shift = 1;
  });
  bad += check("op 2 add result overlaps an operand", [&](Net& n) { with_add(n), n.ops[2].dst = 2; });
  // a residual on the conv (op 1: t0 -> t1, 16 channels), from a third tensor t2
  auto with_res = [](Net& n) {
    n.t = {{8, 0}, {16, 0}, {16, 0}};
    n.ops[1].src2 = 2;
  };
  bad += check(nullptr, with_res);
  bad += check("op 1 residual overlaps the result", [](Net& n) { n.ops[1].src2 = 1; });
  bad += check("op 1 residual needs an fp16 plan", [&](Net& n) { with_res(n), n.ops[1].pool = 2; });
  bad += check("op 1 residual needs an fp16 plan", [&](Net& n) { with_res(n), n.ops[1].wfmt = YV7_WFMT_FP8, n.ops[1].xscale = 1.f; });
  bad += check("op 1 residual needs an fp16 plan", [&](Net& n) { with_res(n), n.d.dtype = YV7_DT_F32; });
  bad += check("op 1 bad residual tensor id", [&](Net& n) { with_res(n), n.ops[1].src2 = 9; });
  bad += check("op 1 residual channel slice out of range", [&](Net& n) { with_res(n), n.ops[1].src2_coff = 8; });
  bad += check("op 1 residual and result differ in resolution", [&](Net& n) { with_res(n), n.t[2].shift = 1, n.d.max_shift = 1; });
  bad += check("op 2 takes no second operand", [](Net& n) { n.ops[2].src2 = 0; });
  std::printf("%d failed\n", bad);
  return bad ? 1 : 0;
}
