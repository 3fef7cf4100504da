"""Dev tool: the default dispatch (yv7_op_kernels: the kernel every op launches, a dry run) of the three
single-GPU bench plans — yolov7 640 bs32, yolov7-tiny 640 bs32, yolov7-w6 1280 bs8 (fp16) — one line
per op and one `workspace` line per plan (yv7_workspace_bytes), for diffing two builds of libyv7
(pruning must not change the dispatch).  tests/test_dispatch_pin.py compares
dispatch_lines() with tests/golden/dispatch_fp16.txt; a pull request that changes the dispatch on
purpose regenerates that file with this tool.
usage: python scripts/dump_dispatch.py OUT.txt"""
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


def dispatch_lines():
    lines = []
    for name, B, img in PLANS:
        m = Model(name)
        synthetic_state_dict(m, seed=0)
        plan = Plan.from_model(m.float().fuse().eval(), 'cuda:0', torch.float16)
        for i, ks in enumerate(plan.op_kernels(B, img, img, torch.float16)):
            lines.append(f'{name}\t{i}\t' + '|'.join(kernel_key(k) for k in ks))
        lines.append(f'{name}\tworkspace\t{L.lib().yv7_workspace_bytes(plan._h, B, img, img)}')
    return lines


if __name__ == '__main__':
    lines = dispatch_lines()
    open(sys.argv[1], 'w').write('\n'.join(lines) + '\n')
    print(len(lines), 'lines')
