"""Dev tool: the default dispatch (yv7_op_kernels: the kernel every op launches, a dry run) of the three
single-GPU bench plans — yolov7 640 bs32, yolov7-tiny 640 bs32, yolov7-w6 1280 bs8 (fp16) — one line
per op and one `workspace` line per plan (yv7_workspace_bytes), for diffing two builds of libyv7
(pruning must not change the dispatch).  tests/test_dispatch_pin.py compares
dispatch_lines() with tests/golden/dispatch_fp16.txt; a pull request that changes the dispatch on
purpose regenerates that file with this tool.

layout_lines(): the workspace layout (every tensor's yv7_tensor_info, yv7_workspace_bytes,
yv7_f8_scratch_info, yv7_num_rows) and the dispatch of plans that take the runtime's other paths — forced
chains, a dissolved dual pair, split-K scratch, an fp8 plan, an fp32 plan, the reorg stem — all dry runs;
tests/test_runtime_layout.py compares it with tests/golden/runtime_layout.txt.
usage: python scripts/dump_dispatch.py OUT.txt [--layout]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'yolo-series_amd'), ROOT]
import torch  # noqa: E402

from models.yolo import Model  # noqa: E402
from yv7 import _lib as L  # noqa: E402
from yv7.runtime import Plan, kernel_key  # noqa: E402
from yv7.synthetic import synthetic_state_dict  # noqa: E402

PLANS = (('yolov7', 32, 640), ('yolov7-tiny', 32, 640), ('yolov7-w6', 8, 1280))


def _model(name):
    m = Model(name)
    synthetic_state_dict(m, seed=0)
    return m.float().fuse().eval()


def dispatch_lines():
    lines = []
    for name, B, img in PLANS:
        plan = Plan.from_model(_model(name), 'cuda:0', torch.float16)
        for i, ks in enumerate(plan.op_kernels(B, img, img, torch.float16)):
            lines.append(f'{name}\t{i}\t' + '|'.join(kernel_key(k) for k in ks))
        lines.append(f'{name}\tworkspace\t{L.lib().yv7_workspace_bytes(plan._h, B, img, img)}')
    return lines


def _case_lines(tag, plan, B, H, W, x_dtype=torch.float16):
    lib, lines = L.lib(), []
    off, dims, n = ctypes.c_int64(), (ctypes.c_int64 * 4)(), ctypes.c_int64()
    for t in range(len(plan.graph.tensors)):
        L.check(lib.yv7_tensor_info(plan._h, t, B, H, W, ctypes.byref(off), dims), 'yv7_tensor_info')
        lines.append(f'{tag}\ttensor {t}\t{off.value}\t' + ' '.join(str(d) for d in dims))
    lines.append(f'{tag}\tworkspace\t{lib.yv7_workspace_bytes(plan._h, B, H, W)}')
    L.check(lib.yv7_f8_scratch_info(plan._h, B, H, W, ctypes.byref(off), ctypes.byref(n)), 'yv7_f8_scratch_info')
    lines.append(f'{tag}\tf8_scratch\t{off.value}\t{n.value}')
    lines.append(f'{tag}\tnum_rows\t{plan.num_rows(H, W)}')
    for i, ks in enumerate(plan.op_kernels(B, H, W, x_dtype)):
        lines.append(f'{tag}\top {i}\t' + '|'.join(kernel_key(k) for k in ks))
    return lines


def layout_lines():
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_chain import stacks
    from test_dual import _pairs
    from yv7.graph import FP8_MIN_COUT, compile_model, fp8_candidates
    lines = []
    m = _model('yolov7')

    def f16():
        return Plan.from_model(m, 'cuda:0', torch.float16)
    plan = f16()
    lines += _case_lines('yolov7 f16 B2 256x320 x16', plan, 2, 256, 320)
    lines += _case_lines('yolov7 f16 B2 256x320 x32', plan, 2, 256, 320, torch.float32)
    plan = f16()   # variant 305 on every 3x3 stack: chain kernels, empty followers, chain-counter scratch
    for i in stacks(plan):
        plan.set_op_variant(i, 305)
    lines += _case_lines('yolov7 f16 B32 640x640 chains', plan, 32, 640, 640)
    plan = f16()   # a forced variant on the pooled op of the first MP pair: the pair runs as two launches
    plan.set_op_variant(_pairs(plan.graph)[0][0], 1)
    lines += _case_lines('yolov7 f16 B2 256x256 pair dissolved', plan, 2, 256, 256)
    plan = f16()   # 128 x 128 ring, two K splits: partial-tile scratch in the workspace
    ops = plan.graph.ops
    plan.set_op_variant(next(i for i, o in enumerate(ops) if o['kind'] == L.OP_CONV and o.get('k', 1) == 3 and
                             o.get('s', 1) == 1 and o['cin'] == 256 and o['cout'] == 256), 132)
    lines += _case_lines('yolov7 f16 B8 640x640 splitk', plan, 8, 640, 640)
    g = compile_model(m, L.DT_F16, fp8={i: 1.0 for i in fp8_candidates(plan.graph, FP8_MIN_COUT)})
    lines += _case_lines('yolov7 fp8 B2 256x256', Plan(g, 'cuda:0', g.weight_blob().to('cuda:0')), 2, 256, 256)
    lines += _case_lines('yolov7-tiny f32 B1 64x96', Plan.from_model(_model('yolov7-tiny'), 'cuda:0', torch.float32),
                         1, 64, 96, torch.float32)
    lines += _case_lines('yolov7-w6 f16 B1 256x384', Plan.from_model(_model('yolov7-w6'), 'cuda:0', torch.float16),
                         1, 256, 384)
    return lines


if __name__ == '__main__':
    lines = layout_lines() if '--layout' in sys.argv[2:] else dispatch_lines()
    open(sys.argv[1], 'w').write('\n'.join(lines) + '\n')
    print(len(lines), 'lines')
