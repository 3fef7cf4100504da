"""The default fp16 dispatch, pinned: the kernel every op launches (Plan.op_kernels through kernel_key, a dry
run: nothing executes) and the workspace size (yv7_workspace_bytes) of the three single-GPU bench plans —
yolov7 640 bs 32, yolov7-tiny 640 bs 32, yolov7-w6 1280 bs 8, fp16, synthetic weights — equal
tests/golden/dispatch_fp16.txt line for line.

The text is scripts/dump_dispatch.py's (one line per op, one `workspace` line per plan).  A change that
moves the dispatch on purpose regenerates the file with that tool on an MI355X (the rules read the CU
count); the file's diff is then the dispatch change in reviewable form.
"""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_matches_golden():
    spec = importlib.util.spec_from_file_location('dump_dispatch', os.path.join(ROOT, 'scripts', 'dump_dispatch.py'))
    dump = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dump)
    want = open(os.path.join(ROOT, 'tests', 'golden', 'dispatch_fp16.txt')).read().splitlines()
    got = dump.dispatch_lines()
    moved = [f'{g!r} (golden: {w!r})' for g, w in zip(got, want) if g != w]
    assert len(got) == len(want) and not moved, f'{len(got)} lines vs {len(want)}; ' + '; '.join(moved[:8])
