"""Dev tool: per-op event timing of the Detect heads of a custom-nc model (the live profiling events of
yv7_profile_enable, as scripts/op_profile.py), row records on.

The net is head-only: three stride-2 convs to stride 8, then per level a 1x1 conv to the head's input width —
by default yolov7's three head inputs, 256 @80^2, 512 @40^2, 1024 @20^2 at 640^2.  Per (nc, level): the kernel
the dispatch picks, its time, and the ratio to the z-write floor B * rows * no * 4 bytes / 8 TB/s.

--lib runs another build of libyv7.so (an A/B against the parent commit's library in one job);
--variant forces a DETECT variant (89: conv_det_nc_kernel, 99: the 64 x 256 ring) on every level.
A head with na * no > 256 is only ever launched on conv_det_nc_kernel: anything else is refused here, on the
host, before the first launch (the 256-wide forms decode one N tile only).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'yolo-series_amd'), ROOT]
ap = argparse.ArgumentParser()
ap.add_argument('--nc', default='1,20,79')
ap.add_argument('--na', type=int, default=3)
ap.add_argument('--b', type=int, default=32)
ap.add_argument('--img', type=int, default=640)
ap.add_argument('--widths', default='256,512,1024')
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--variant', type=int, default=0)
ap.add_argument('--lib', default='')
ap.add_argument('--label', default='')
a = ap.parse_args()

from yv7 import _lib as L  # noqa: E402
if a.lib:
    L.LIB_PATH = os.path.abspath(a.lib)
import torch  # noqa: E402
from models.yolo import Model  # noqa: E402
from yv7.runtime import kernel_key  # noqa: E402
from yv7.synthetic import synthetic_state_dict  # noqa: E402

ANCHORS = [[12, 16, 19, 36, 40, 28, 30, 32], [36, 75, 76, 55, 72, 146, 74, 100], [142, 110, 192, 243, 459, 401, 325, 322]]


def conv(f, c, k=1, s=1):
    return [f, 1, 'Conv', [c, k, s]]


def net(nc, na, w):
    return {'nc': nc, 'depth_multiple': 1.0, 'width_multiple': 1.0, 'anchors': [l[:2 * na] for l in ANCHORS],
            'backbone': [conv(-1, 32, 3, 2), conv(-1, 64, 3, 2), conv(-1, 64, 3, 2), conv(2, w[0]),
                         conv(2, 64, 3, 2), conv(4, w[1]), conv(4, 64, 3, 2), conv(6, w[2])],
            'head': [[[3, 5, 7], 1, 'Detect', ['nc', 'anchors']]]}


widths = [int(v) for v in a.widths.split(',')]
B, H = a.b, a.img
for nc in (int(v) for v in a.nc.split(',')):
    m = Model(net(nc, a.na, widths))
    m.load_state_dict(synthetic_state_dict(m, seed=3, calib_hw=256))
    plan = m.float().eval().fuse().to('cuda:0').half().plan()
    dets = sorted(((i, o) for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_DETECT), key=lambda t: t[1]['level'])
    for i, _ in dets if a.variant else []:
        plan.set_op_variant(i, a.variant)
    ks = plan.op_kernels(B, H, H)
    keys = [kernel_key(ks[i][0]) for i, _ in dets]
    if a.na * (nc + 5) > 256 and not all(k.startswith('conv_det_nc_kernel') for k in keys):
        sys.exit(f'nc {nc}: na * no = {a.na * (nc + 5)} > 256 on {keys}: not launched')
    x = torch.rand(B, 3, H, H, device='cuda:0').half()
    N = plan.num_rows(H, H)
    z = torch.empty(B, N, plan.no, device='cuda:0')
    rb = torch.empty(B, N, 4, device='cuda:0')
    for _ in range(3):
        plan.forward_into(x, z, rowbest=rb)
    torch.cuda.synchronize()
    plan.profile_enable(a.iters)
    for _ in range(a.iters):
        plan.forward_into(x, z, rowbest=rb)
    torch.cuda.synchronize()
    n, ms = plan.profile_read()
    for (i, o), key in zip(dets, keys):
        s = int(plan.graph.stride[o['level']])
        rows = a.na * (H // s) ** 2
        us = ms[i] / n * 1e3
        floor = B * rows * plan.no * 4 / 8e12 * 1e6
        print(f'{a.label:8s} nc {nc:3d} na {a.na} DET {o["cin"]:5d}->{o["cout"]:4d} @{H // s:<3d} bs {B}: {us:7.1f} us  '
              f'z floor {floor:5.1f} us  x{us / floor:5.2f}  {key}', flush=True)
    del plan, m
