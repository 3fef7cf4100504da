"""The stepped addressing of the register-weight kernels (conv_w1.hip, conv_s2.hip) at the shapes where a step can
go wrong, op by op against fp32 torch (tests/opcheck.py, the tolerance of tests/test_variants.py); conv_lr.hip's
configurations, whose addressing is per block, run through the same shapes.

Each kernel's configurations are forced with the variant API on a small net whose 1x1 / 3x3 layers have the
kernels' input widths (cin 64 / 128 / 256, and 512 for the 1x1) and ragged outputs: cout 80 and 240 (cout % 32 ==
16: the last channel pair of a store is half masked; 240 is the 255-channel head rounded to the kernels' 16-channel
granularity) and 192 (the last 128- / 256-channel N slice partly outside the layer).  The frames put the stride-8
level at 20 x 20, 40 x 24 and 16 x 160 (stride 4: 40 x 40, 80 x 48, 32 x 320): rows narrower than a 1x1 tile's
pixels (the per-lane decomposition conv_w1.hip keeps there), tiles that span three rows and two images (20- and
24-pixel rows under 32-pixel tiles, 40 and 48 under 64), M not a multiple of the tile (B = 1, 5 at 20 x 20), and
B = 1, 5 leave the trailing 4-image group of conv_s2.hip / conv_lr.hip partial.

Reference: models/common.py:110-111 (Conv.fuseforward).

The second test compares two `bench.py --dump-outputs` folders (the parent build's and this build's, same
arguments: inputs and weights are seeded) byte for byte; it runs when both are named in the environment.
"""
import copy
import glob
import os

import pytest
import torch

from helpers import frames
from opcheck import check_ops, kernel_summary
from yv7 import _lib as L

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

NET = {'nc': 3, 'depth_multiple': 1.0, 'width_multiple': 1.0,
       'anchors': [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]],
       'backbone': [[-1, 1, 'Conv', [32, 3, 1]],    # 0  @1
                    [-1, 1, 'Conv', [64, 3, 2]],    # 1  @2
                    [-1, 1, 'Conv', [80, 3, 1]],    # 2  3x3 s1, cin 64 -> 80
                    [-1, 1, 'Conv', [64, 1, 1]],    # 3
                    [-1, 1, 'Conv', [192, 3, 2]],   # 4  @4: 3x3 s2, cin 64 -> 192
                    [-1, 1, 'Conv', [128, 1, 1]],   # 5
                    [-1, 1, 'Conv', [240, 1, 1]],   # 6  1x1, cin 128 -> 240
                    [-1, 1, 'Conv', [256, 1, 1]],   # 7
                    [-1, 1, 'Conv', [80, 1, 1]],    # 8  1x1, cin 256 -> 80
                    [-1, 1, 'Conv', [128, 1, 1]],   # 9
                    [-1, 1, 'Conv', [240, 3, 1]],   # 10 3x3 s1, cin 128 -> 240
                    [-1, 1, 'Conv', [128, 1, 1]],   # 11
                    [-1, 1, 'Conv', [80, 3, 2]],    # 12 @8: 3x3 s2, cin 128 -> 80
                    [-1, 1, 'Conv', [512, 1, 1]],   # 13
                    [-1, 1, 'Conv', [192, 1, 1]],   # 14 1x1, cin 512 -> 192
                    [-1, 1, 'Conv', [128, 1, 1]],   # 15
                    [-1, 1, 'Conv', [80, 1, 1]],    # 16 1x1, cin 128 -> 80
                    [-1, 1, 'Conv', [256, 1, 1]],   # 17
                    [-1, 1, 'Conv', [240, 1, 1]],   # 18 1x1, cin 256 -> 240
                    [-1, 1, 'Conv', [256, 1, 1]],   # 19
                    [-1, 1, 'Conv', [192, 3, 1]],   # 20 3x3 s1, cin 256 -> 192 (P3)
                    [-1, 1, 'Conv', [64, 1, 1]],    # 21
                    [-1, 1, 'Conv', [80, 3, 2]],    # 22 @16: 3x3 s2, cin 64 (P4)
                    [-1, 1, 'Conv', [128, 1, 1]],   # 23
                    [-1, 1, 'Conv', [96, 3, 2]]],   # 24 @32: 3x3 s2, cin 128 (P5)
       'head': [[[20, 22, 24], 1, 'Detect', ['nc', 'anchors']]]}

LR = [270, 271, 272, 273, 274, 275, 276, 277, 278, 279]          # conv_lr.hip lr_rows
S2 = [280, 281, 282, 283, 284, 285, 286, 287, 288]               # conv_s2.hip s2_rows
W1_CIN = {290: 128, 291: 256, 292: 512, 293: 256, 294: 128, 295: 512, 302: 256, 303: 256}   # conv_w1.hip w1_rows
FAMILY = {'conv3x3_lr_kernel': LR, 'conv3x3s2_rw_kernel': S2, 'conv1x1_rw_kernel': list(W1_CIN)}


@pytest.fixture(scope='module', autouse=True)
def _no_miopen():
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = prev


@pytest.fixture(scope='module')
def plan():
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    m = Model(copy.deepcopy(NET))
    m.load_state_dict(synthetic_state_dict(m, seed=5, calib_hw=160))
    return m.float().eval().fuse().to(DEV).half().plan()


@pytest.mark.parametrize('B', [1, 5, 8])
@pytest.mark.parametrize('H,W', [(160, 160), (320, 192), (128, 1280)])   # stride 8: 20 x 20, 40 x 24, 16 x 160
def test_stepped_addressing(plan, B, H, W):
    x = frames(B, H, W, seed=11).to(DEV).half()
    ops = plan.graph.ops
    convs = [i for i, o in enumerate(ops) if o['kind'] == L.OP_CONV]
    launched = {k: set() for k in FAMILY}
    lines = []
    for v in [0] + LR + S2 + list(W1_CIN):
        for i in convs:
            plan.set_op_variant(i, v)
        ks = plan.op_kernels(B, H, W)
        for fam, vs in FAMILY.items():
            if v in vs:
                launched[fam] |= {i for i in convs if any(fam in k for k in ks[i])}
        if v in W1_CIN:   # the 1x1 kernel takes every size: each layer of its input width must launch it
            want = [i for i in convs if ops[i].get('k', 1) == 1 and ops[i]['cin'] == W1_CIN[v]]
            assert want, (v, W1_CIN[v])
            for i in want:
                assert any('conv1x1_rw_kernel' in k for k in ks[i]), (v, i, ks[i])
        z, xs = plan.forward(x)
        torch.cuda.synchronize()
        out = check_ops(plan, x, B, H, W, raw=xs, z=z)
        for i in convs:
            got = plan.tensor_view(ops[i]['dst'], B, H, W)[..., ops[i]['dst_coff']:ops[i]['dst_coff'] + ops[i]['cout']]
            assert torch.isfinite(got).all(), f'variant {v}: op {i} output not finite'
        assert torch.isfinite(z).all(), f'variant {v}: z not finite'
        lines.append(f'variant {v}: ' + kernel_summary(out))
        for i in convs:
            plan.set_op_variant(i, 0)
    print('\n' + '\n'.join(lines))
    ragged = lambda i: ops[i]['cout'] in (80, 192, 240)   # noqa: E731
    for fam, got in launched.items():
        assert any(ragged(i) for i in got), f'{fam} launched on no ragged layer at B {B}, {H} x {W}: ops {sorted(got)}'
    # the 3x3 kernels at stride 1 and stride 2, on both of their input widths
    for fam in ('conv3x3_lr_kernel', 'conv3x3s2_rw_kernel'):
        seen = {(ops[i]['s'], ops[i]['cin']) for i in launched[fam]}
        assert {(1, 64), (1, 128), (2, 64), (2, 128)} <= seen, (fam, sorted(seen))
    assert any(ops[i]['cin'] == 256 for i in launched['conv3x3_lr_kernel'])


def test_bench_outputs_equal_parent():
    """Every .npy of two `bench.py --steps 2 --warmup 1 --dump-outputs DIR` runs, the parent build's and this one's,
    byte for byte (YV7_DUMP_PARENT, YV7_DUMP_NEW)."""
    a, b = os.environ.get('YV7_DUMP_PARENT'), os.environ.get('YV7_DUMP_NEW')
    if not (a and b):
        pytest.skip('YV7_DUMP_PARENT and YV7_DUMP_NEW name no pair of bench.py --dump-outputs folders')
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(a, '*.npy')))
    assert names and names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(b, '*.npy'))), names
    for n in names:
        with open(os.path.join(a, n), 'rb') as fa, open(os.path.join(b, n), 'rb') as fb:
            assert fa.read() == fb.read(), f'{n} differs between {a} and {b}'
