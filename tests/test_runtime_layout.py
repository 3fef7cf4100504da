"""The runtime's workspace layout and fused-group dispatch, pinned: every tensor's yv7_tensor_info,
yv7_workspace_bytes, yv7_f8_scratch_info, yv7_num_rows and the kernels of every op (dry runs: nothing
executes) of plans that take each path of the op loop — a non-square frame with fp16 and fp32 input,
forced 3x3 chains (chain kernels, empty followers, the chain-counter scratch), a dual 1x1 pair dissolved
by a forced variant, split-K partial-tile scratch, an fp8 plan (staging buffer, quantize + GEMM pairs),
an fp32 plan and the reorg stem — equal tests/golden/runtime_layout.txt line for line.

The text is scripts/dump_dispatch.py layout_lines()'s, dumped on an MI355X (the dispatch rules read the CU
count).  A change that moves the layout or the dispatch on purpose regenerates the file with that tool.
"""
import ctypes
import importlib.util
import os

import pytest
import torch

from helpers import fresh_model
from yv7 import _lib as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_matches_golden():
    spec = importlib.util.spec_from_file_location('dump_dispatch', os.path.join(ROOT, 'scripts', 'dump_dispatch.py'))
    dump = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dump)
    want = open(os.path.join(ROOT, 'tests', 'golden', 'runtime_layout.txt')).read().splitlines()
    got = dump.layout_lines()
    moved = [f'{g!r} (golden: {w!r})' for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not moved, f'{len(got)} lines vs {len(want)}; ' + '; '.join(moved[:8])


def test_layout_errors():
    """A frame that is no multiple of the plan's largest stride: no workspace size, YV7_E_SHAPE from
    yv7_tensor_info; a workspace one byte short: YV7_E_WORKSPACE naming yv7_workspace_bytes' count."""
    lib = L.lib()
    plan = fresh_model('yolov7-tiny').to('cuda:0').half().plan()
    B = 2
    assert lib.yv7_workspace_bytes(plan._h, B, 250, 256) == 0
    off, dims = ctypes.c_int64(), (ctypes.c_int64 * 4)()
    rc = lib.yv7_tensor_info(plan._h, 0, B, 250, 256, ctypes.byref(off), dims)
    assert rc == -2 and lib.yv7_last_error().decode() == \
        'input H and W must be positive multiples of 32 (got B=2 H=250 W=256)'
    need = lib.yv7_workspace_bytes(plan._h, B, 256, 256)
    assert need > 0
    x = torch.zeros(B, 3, 256, 256, dtype=torch.float16, device='cuda:0')
    z = torch.empty(B, plan.num_rows(256, 256), plan.no, device='cuda:0')
    ws = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    rc = lib.yv7_forward(plan._h, x.data_ptr(), L.DT_F16, B, 256, 256, z.data_ptr(), None, None, ws.data_ptr(),
                         need - 1, None)
    assert rc == -3 and lib.yv7_last_error().decode() == f'yv7_forward: workspace too small (need {need} bytes)'
