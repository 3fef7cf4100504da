"""Ragged letterbox (yv7_letterbox_ragged): B frames of B sizes on one canvas in one call.

CPU: autoshape_geometry (models/common.py:909-915 restated in utils/datasets.py) on hand-derived cases and
against the oracle's letterbox_geometry; the C layout of the two new descriptors; every host-side validation
message of the entry point (no device is touched before they return).
GPU: every frame's slice of the output bit-exact against oracle/letterbox_ref.py, for all three output kinds and
both channel orders, and byte-equal to yv7_letterbox on a same-size batch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import letterbox_ref as R
from utils import datasets as D
from yv7 import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# canvas 64 x 64: three identity frames (two with borders on different axes), one exact-2x frame and two
# bilinear ones (one up-scaling) with odd borders (11/12 and 21/22)
BATCH_A = [(48, 64), (64, 48), (33, 51), (128, 128), (64, 64), (20, 61)]
# canvas 96 x 96: the second frame resizes to 36 columns, 36 * 3 % 16 != 0 -> the row tail takes the scalar cast
BATCH_B = [(333, 517), (100, 37)]


# ------------------------------------------------------------------------------------------ CPU
def test_autoshape_geometry_hand_derived():
    # 720 x 1280 at 640: gain 0.5 -> 360 x 640 -> rows rounded up to 384; exact 2x downscale, 12 px above and below
    shape1, geoms, descs = D.autoshape_geometry([(720, 1280)], 640, 32)
    assert shape1 == [384, 640]
    assert geoms[0][0] == (640, 360) and geoms[0][3] == (12, 12, 0, 0)
    assert 1280 == 2 * geoms[0][0][0] and 720 == 2 * geoms[0][0][1]            # the exact-2x area mode
    assert descs[0] == (720, 1280, 0.5, 0.0, 12.0)
    # bus.jpg and zidane.jpg together: a square canvas, one padded left/right, one above/below
    shape1, geoms, _ = D.autoshape_geometry([(1080, 810), (720, 1280)], 640, 32)
    assert shape1 == [640, 640]
    assert geoms[0][3] == (0, 0, 80, 80) and geoms[1][3] == (140, 140, 0, 0)
    # three COCO-like frames: the tallest (480 x 640) sets the canvas; 427 -> 53 px split 26 / 27
    shape1, geoms, _ = D.autoshape_geometry([(427, 640), (480, 640), (375, 500)], 640, 32)
    assert shape1 == [480, 640] and geoms[0][3] == (26, 27, 0, 0)
    # 147 * (640 / 147) = 640.0000000000001 in Python floats: the reference rounds it up a whole stride
    assert 147 * (640 / 147) > 640
    shape1, geoms, _ = D.autoshape_geometry([(147, 100)], 640, 32)
    assert shape1 == [672, 448]


@pytest.mark.parametrize('shapes,size', [(BATCH_A, 64), (BATCH_B, 96), ([(1080, 810), (720, 1280), (147, 100)], 640)])
def test_autoshape_geometry_matches_oracle(shapes, size):
    shape1, geoms, descs = D.autoshape_geometry(shapes, size, 32)
    for s, g, d in zip(shapes, geoms, descs):
        assert g == R.letterbox_geometry(s, shape1, auto=False)
        (nw, nh), _, _, (top, bottom, left, right) = g
        assert [nh + top + bottom, nw + left + right] == shape1
        gain = min(shape1[0] / s[0], shape1[1] / s[1])                     # general.py:342-343
        assert d == (s[0], s[1], gain, (shape1[1] - s[1] * gain) / 2, (shape1[0] - s[0] * gain) / 2)


def test_batches_cover_what_they_claim():
    def mode(s, g):
        (nw, nh) = g[0]
        return 0 if (nh, nw) == s else 2 if s == (2 * nh, 2 * nw) else 1
    shape1, geoms, _ = D.autoshape_geometry(BATCH_A, 64, 32)
    assert shape1 == [64, 64]
    assert [mode(s, g) for s, g in zip(BATCH_A, geoms)] == [0, 0, 1, 2, 0, 1]
    assert geoms[0][3] == (8, 8, 0, 0) and geoms[1][3] == (0, 0, 8, 8)
    assert geoms[2][3] == (11, 12, 0, 0) and geoms[5][3] == (21, 22, 0, 0)
    shape1, geoms, _ = D.autoshape_geometry(BATCH_B, 96, 32)
    assert shape1 == [96, 96] and geoms[1][0][0] == 36 and 36 * 3 % 16 != 0


def test_descriptor_layout_matches_c(tmp_path):
    """ctypes mirrors of yv7_frame_desc / yv7_scale_desc have the C sizes and offsets."""
    prog = tmp_path / 'layout.c'
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv7.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(yv7_frame_desc), '
                    'offsetof(yv7_frame_desc, h), offsetof(yv7_frame_desc, new_h), offsetof(yv7_frame_desc, left), '
                    'sizeof(yv7_scale_desc), offsetof(yv7_scale_desc, w0), offsetof(yv7_scale_desc, gain), '
                    'offsetof(yv7_scale_desc, pad_h));return 0;}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(prog), '-o', str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    F, S = _lib.FrameDesc, _lib.ScaleDesc
    assert got == [ctypes.sizeof(F), F.h.offset, F.new_h.offset, F.left.offset,
                   ctypes.sizeof(S), S.w0.offset, S.gain.offset, S.pad_h.offset]
    assert got[0] == 32 and got[4] == 20


def _frame(**kw):
    f = dict(data=0x1000, h=10, w=10, new_h=10, new_w=10, top=0, left=0)   # the pointer is never followed
    f.update(kw)
    return _lib.FrameDesc(**f)


def test_ragged_validation_messages():
    L = _lib.lib()
    dst = ctypes.c_void_p(0x2000)

    def call(frames, B=None, oh=16, ow=16, pad=(114, 114, 114), kind=0, dst=dst, ws=None, ws_bytes=0):
        arr = (_lib.FrameDesc * max(len(frames), 1))(*frames)
        rc = L.yv7_letterbox_ragged(arr if frames else None, len(frames) if B is None else B, oh, ow, *pad, 0, kind,
                                    dst, ws, ws_bytes, None)
        return rc, L.yv7_last_error().decode()

    assert L.yv7_letterbox_ragged_workspace_bytes(None, 4) == 0
    for args, code, text in [
        (dict(frames=[]), -1, 'null argument'),
        (dict(frames=[_frame()], dst=None), -1, 'null argument'),
        (dict(frames=[_frame()], B=0), -1, 'B must be positive'),
        (dict(frames=[_frame()], kind=3), -1, 'out_kind must be 0, 1 or 2'),
        (dict(frames=[_frame()], oh=0), -2, 'canvas'),
        (dict(frames=[_frame()], pad=(114, 256, 114)), -1, 'pad colour outside 0..255'),
        (dict(frames=[_frame(), _frame(data=None)]), -1, 'frame 1 has null data'),
        (dict(frames=[_frame(), _frame(), _frame(w=0)]), -2, 'frame 2 has a non-positive size'),
        (dict(frames=[_frame(new_h=0)]), -2, 'frame 0 has a non-positive size'),
        (dict(frames=[_frame(), _frame(top=7)]), -2, 'frame 1: the resized image must lie inside the output canvas'),
        (dict(frames=[_frame(left=-1)]), -2, 'frame 0: the resized image must lie inside the output canvas'),
        (dict(frames=[_frame()], ws=None, ws_bytes=64), -3, 'workspace'),
    ]:
        rc, msg = call(**args)
        assert rc == code and text in msg, (args, rc, msg)


# ------------------------------------------------------------------------------------------ GPU
def _random_frames(shapes, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in shapes]


def _expected(frame, canvas, color, swap_rb, out_kind):
    lb, _, _ = R.letterbox(frame, canvas, color=color, auto=False)
    if out_kind == D.OUT_U8_HWC:
        return torch.from_numpy(lb)
    # to_input reverses the channels itself: hand it the frame pre-reversed to keep the order
    return R.to_input(lb if swap_rb else lb[:, :, ::-1], half=out_kind == D.OUT_F16_CHW)


@pytest.mark.gpu
@pytest.mark.parametrize('shapes,size,seed', [(BATCH_A, 64, 3), (BATCH_B, 96, 4)])
@pytest.mark.parametrize('out_kind', [D.OUT_U8_HWC, D.OUT_F16_CHW, D.OUT_F32_CHW])
@pytest.mark.parametrize('swap_rb', [False, True])
def test_gpu_ragged_bit_exact(shapes, size, seed, out_kind, swap_rb):
    frames = _random_frames(shapes, seed)
    shape1, geoms, _ = D.autoshape_geometry(shapes, size, 32)
    out = D.letterbox_ragged(frames, geoms, shape1, swap_rb=swap_rb, out_kind=out_kind).cpu()
    assert out.shape[0] == len(frames)
    for i, f in enumerate(frames):
        want = _expected(f, shape1, (114, 114, 114), swap_rb, out_kind)
        assert out[i].dtype == want.dtype and torch.equal(out[i], want), \
            f'frame {i} {shapes[i]}: {int((out[i] != want).sum())} values differ'


@pytest.mark.gpu
@pytest.mark.parametrize('swap_rb', [False, True])
def test_gpu_ragged_pad_colour_and_tensor_frames(swap_rb):
    """A non-grey pad colour, given in the frames' channel order; half of the frames already on the device."""
    frames = _random_frames(BATCH_A, 5)
    shape1, geoms, _ = D.autoshape_geometry(BATCH_A, 64, 32)
    mixed = [torch.from_numpy(f).cuda() if i % 2 else f for i, f in enumerate(frames)]
    color = (0, 50, 200)
    for kind in (D.OUT_U8_HWC, D.OUT_F32_CHW):
        out = D.letterbox_ragged(mixed, geoms, shape1, color=color, swap_rb=swap_rb, out_kind=kind).cpu()
        for i, f in enumerate(frames):
            assert torch.equal(out[i], _expected(f, shape1, color, swap_rb, kind)), (kind, i)


@pytest.mark.gpu
@pytest.mark.parametrize('half', [True, False])
def test_gpu_ragged_equals_letterbox_on_one_size(half):
    """A same-size batch: the ragged call's output is yv7_letterbox's, byte for byte (bilinear, odd borders)."""
    shape = (333, 517)
    frames = _random_frames([shape] * 3, 6)
    geom = D.letterbox_geometry(shape, 96, auto=False)
    stacked = torch.from_numpy(np.stack(frames)).cuda()
    for kind in (D.OUT_U8_HWC, D.OUT_F16_CHW if half else D.OUT_F32_CHW):
        old = D._run(stacked, geom, (114, 114, 114), kind)
        new = D.letterbox_ragged(frames, [geom] * 3, (96, 96), swap_rb=True, out_kind=kind)
        assert old.dtype == new.dtype and torch.equal(old.cpu().view(torch.uint8), new.cpu().view(torch.uint8))


@pytest.mark.gpu
def test_gpu_ragged_more_frames_than_one_launch_holds():
    """70 frames: the descriptors travel 64 per launch, so this takes two."""
    shapes = [BATCH_A[i % len(BATCH_A)] for i in range(70)]
    frames = _random_frames(shapes, 7)
    shape1, geoms, _ = D.autoshape_geometry(shapes, 64, 32)
    out = D.letterbox_ragged(frames, geoms, shape1, out_kind=D.OUT_U8_HWC).cpu()
    for i in (0, 63, 64, 65, 69):
        assert torch.equal(out[i], _expected(frames[i], shape1, (114, 114, 114), False, D.OUT_U8_HWC)), i
