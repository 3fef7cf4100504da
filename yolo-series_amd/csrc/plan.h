// Shared by the runtime's translation units: the plan, error reporting, the small helpers and the per-call
// workspace layout.  plan_create.cpp builds and destroys a plan, plan_layout.cpp places its tensors and scratch
// in a workspace and binds a conv's operands, forward.cpp walks the ops, runtime.cpp holds the rest of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/yv7.h"
#include "conv_f16_launch.h"
#include "yv7_kernels.h"

struct yv7_plan {
  int device = 0;
  int dtype = 0;
  std::vector<yv7_tensor_desc> tensors;
  std::vector<yv7_op_desc> ops;
  int nl = 0, na = 0, no = 0, max_shift = 0;
  std::vector<float> stride, anchor_grid;
  void* weights = nullptr;
  size_t wbytes = 0;
  void* zero = nullptr;  // 4 KiB of zeros
  // fp16 plans: every 3x3 stride-1/2 conv's weights again, fragment-packed for conv_lr.hip (pack_frag);
  // wf_off[op] = byte offset into wfrag, -1 when the op has none
  void* wfrag = nullptr;
  std::vector<int64_t> wf_off;
  // the workspaces whose zero frames are known to be intact for one layout (see yv7_forward); several,
  // so that batches in flight can run concurrently on their own streams and workspaces
  struct WsKey {
    const void* ptr;
    size_t bytes;
    int B, H, W;
  };
  std::vector<WsKey> ws_ready;
  // per-op kernel variant override (0 = tuned dispatch; yv7_set_op_variant)
  std::vector<int> op_variant;
  // live profiling: events[f * 2 * n_ops + 2 * i + {0: start, 1: stop}] of op i in profiled forward f
  std::vector<hipEvent_t> events;
  int prof_max = 0, prof_used = 0;
};

namespace yv7rt {
#pragma GCC visibility push(hidden)

// set yv7_last_error()'s message and return the code (runtime.cpp)
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* where);

inline size_t elem_size(int dtype) { return dtype == YV7_DT_F16 ? 2 : 4; }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool is_f8(const yv7_op_desc& o) { return o.kind == YV7_OP_CONV && o.wfmt == YV7_WFMT_FP8; }
// K padding of a conv's packed weights: 64 in the plan dtype, 128 for fp8 (one MFMA K step)
inline int kpad_of(const yv7_op_desc& o) {
  if (is_f8(o)) return (o.cin + 127) / 128 * 128;
  return (o.k * o.k * o.cin + 63) / 64 * 64;
}
// Channels an INPUT op packs (cout; k == 2: after the space-to-depth, four per image plane); 0, from a descriptor
// written before the field was read, stands for the three-plane image
inline int input_packed(const yv7_op_desc& o) { return o.cout ? o.cout : (o.k == 2 ? 12 : 3); }
// Planes C of the [B,C,H,W] image an INPUT or STEM op reads (the ReOrg stem, cin 12: three)
inline int input_channels(const yv7_op_desc& o) {
  if (o.kind == YV7_OP_STEM) return o.cin == 12 ? 3 : o.cin;
  return o.k == 2 ? input_packed(o) / 4 : input_packed(o);
}
// channel slices [ca, ca + na) of tensor ta and [cb, cb + nb) of tensor tb share a channel
inline bool overlap(int ta, int ca, int na, int tb, int cb, int nb) { return ta == tb && ca < cb + nb && cb < ca + na; }

// Where a [B,C,H,W] batch's data lies in the workspace (computed per call, plan_layout.cpp).  Tensors: bordered
// NHWC [B][h + 2*YV7_BORDER][w + 2*YV7_BORDER][C] each, 256-byte aligned.  Behind them the scratch: split-K
// fp32 partial tiles (the largest any conv of the plan needs; convs run one at a time) and the per-tile arrival
// counters (zeroed with the workspace, re-armed by the kernels), the dense e4m3 copy of an FP8 op's input (the
// largest one) and the ready counters of a chained 3x3 launch (the largest chain).
struct Layout {
  int B = 0, H = 0, W = 0;
  std::vector<size_t> off;   // byte offset of every tensor
  size_t part_off = 0, part_bytes = 0, cnt_off = 0;
  int cnt_n = 0;
  size_t f8_off = 0, f8_bytes = 0;
  size_t chain_off = 0, chain_bytes = 0;
  size_t end = 0;   // the workspace's size
  int nrows = 0;    // yv7_num_rows
  std::vector<int> row_off;     // z row offset of each Detect level
  std::vector<size_t> raw_off;  // raw-logit element offset of each Detect level
};
// Fills *l after checking (B, H, W) against the plan; the check's error code otherwise.
int plan_layout(const yv7_plan* p, int B, int H, int W, Layout* l);
// The kernel parameters of CONV / DETECT op i: geometry, weights and the operand pointers into the workspace at
// wsb (null for a layout query).  False when a CONV's output shape is not its destination tensor's.
bool bind_conv(const yv7_plan* p, size_t i, const Layout& l, unsigned char* wsb, yv7::ConvParams* c);
// Drops every remembered workspace that overlaps [ws, ws + bytes).
void forget_workspaces(yv7_plan* p, const void* ws, size_t bytes);
// The chained 3x3 launch starting at op i (forward.cpp): fills *c, returns the ops it covers (0: none).
int find_chain(const yv7_plan* p, size_t i, const Layout& l, unsigned char* wsb, yv7::ChainParams* c);
// Every rejection of a network descriptor; no HIP call.  0, or the code fail() was given (plan_create.cpp).
int validate_net(const yv7_net_desc* d, size_t nbytes);

#pragma GCC visibility pop
}  // namespace yv7rt
