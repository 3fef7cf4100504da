"""Boxes back to image pixels (yv7_scale_boxes): scale_coords + clip_coords on yv7_nms's fixed-shape output and
the derived views of Detections (models/common.py:940-948), bit-exact against CPU torch.

CPU: every host-side validation message.  GPU: four images of four sizes on a 640 x 640 canvas, counts
0 / 1 / 17 / 300 of 300 rows, coordinates that leave the canvas on both sides.  The scalars are scale_desc's,
the function autoshape_geometry fills its descriptors with; autoshape_geometry itself puts these four sizes
on a 672 x 640 canvas (147 * (640 / 147) > 640), which runs as a second case."""
import ctypes

import pytest
import torch

from oracle import nms_ref
from utils import general as G
from utils.datasets import autoshape_geometry
from yv7 import _lib

SHAPES = [(1080, 810), (720, 1280), (33, 51), (147, 100)]
CANVAS = (640, 640)
COUNTS = [0, 1, 17, 300]
MAX_DET = 300
SENTINEL = -12345.5


def test_scale_desc_is_scale_coords_scalars():
    # bus.jpg on 640 x 640: gain 640/1080, 80 px left and right
    assert G.scale_desc((640, 640), (1080, 810, 3)) == (1080, 810, 640 / 1080, (640 - 810 * (640 / 1080)) / 2, 0.0)


def test_scale_boxes_validation_messages():
    L = _lib.lib()
    det, cnt = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)   # never followed

    def call(descs, det=det, cnt=cnt, B=None, max_det=300):
        arr = (_lib.ScaleDesc * max(len(descs), 1))(*[_lib.ScaleDesc(*d) for d in descs])
        rc = L.yv7_scale_boxes(det, cnt, len(descs) if B is None else B, max_det, arr if descs else None, 0,
                               None, None, None, None)
        return rc, L.yv7_last_error().decode()

    ok = (480, 640, 1.0, 0.0, 0.0)
    for args, code, text in [
        (dict(descs=[ok], det=None), -1, 'null argument'),
        (dict(descs=[ok], cnt=None), -1, 'null argument'),
        (dict(descs=[]), -1, 'null argument'),
        (dict(descs=[ok], B=0), -1, 'B must be positive'),
        (dict(descs=[ok], max_det=0), -1, 'max_det must be positive'),
        (dict(descs=[ok, (0, 640, 1.0, 0.0, 0.0)]), -2, 'image 1 has a non-positive size'),
        (dict(descs=[(480, -1, 1.0, 0.0, 0.0)]), -2, 'image 0 has a non-positive size'),
        (dict(descs=[ok, ok, (480, 640, 0.0, 0.0, 0.0)]), -1, 'image 2: gain must be positive and finite'),
        (dict(descs=[(480, 640, float('inf'), 0.0, 0.0)]), -1, 'image 0: gain must be positive and finite'),
        (dict(descs=[(480, 640, float('nan'), 0.0, 0.0)]), -1, 'image 0: gain must be positive and finite'),
    ]:
        rc, msg = call(**args)
        assert rc == code and text in msg, (args, rc, msg)


def _case():
    g = torch.Generator().manual_seed(11)
    det = torch.empty(len(SHAPES), MAX_DET, 6)
    det[..., :4] = torch.rand(len(SHAPES), MAX_DET, 4, generator=g) * 680 - 20     # uniform in [-20, 660]
    det[..., 4] = torch.rand(len(SHAPES), MAX_DET, generator=g)
    det[..., 5] = torch.randint(0, 80, (len(SHAPES), MAX_DET), generator=g).float()
    for b, n in enumerate(COUNTS):
        det[b, n:] = SENTINEL
    return det


def _views(x, shape):
    """Detections.__init__ (common.py:940-948) on the CPU."""
    gn = torch.tensor([shape[1], shape[0], shape[1], shape[0], 1., 1.])
    xywh = x.clone()
    xywh[:, 0] = (x[:, 0] + x[:, 2]) / 2
    xywh[:, 1] = (x[:, 1] + x[:, 3]) / 2
    xywh[:, 2] = x[:, 2] - x[:, 0]
    xywh[:, 3] = x[:, 3] - x[:, 1]
    return xywh, x / gn, xywh / gn


def _descs(canvas):
    if canvas == CANVAS:
        return [G.scale_desc(canvas, s) for s in SHAPES]
    shape1, _, descs = autoshape_geometry(SHAPES, 640, 32)
    assert tuple(shape1) == canvas
    return descs


@pytest.mark.gpu
@pytest.mark.parametrize('round_boxes', [False, True])
@pytest.mark.parametrize('canvas', [CANVAS, (672, 640)])
def test_gpu_scale_boxes_bit_exact(round_boxes, canvas):
    det0 = _case()
    descs = _descs(canvas)
    det = det0.cuda()
    cnt = torch.tensor(COUNTS, dtype=torch.int32).cuda()
    xywh, xyxyn, xywhn = (v.cpu() for v in G.scale_boxes(det, cnt, descs, round_boxes=round_boxes, views=True))
    det = det.cpu()
    low = high = 0
    for b, (shape, n) in enumerate(zip(SHAPES, COUNTS)):
        want = det0[b, :n].clone()
        want[:, :4] = nms_ref.scale_coords(canvas, want[:, :4], shape)
        if round_boxes:
            want[:, :4] = want[:, :4].round()
        low += int((want[:, [0, 2]] == 0).sum())
        high += int((want[:, [0, 2]] == shape[1]).sum())
        w_xywh, w_xyxyn, w_xywhn = _views(want, shape)
        assert torch.equal(det[b, :n], want), f'image {b}: xyxy'
        assert torch.equal(xywh[b, :n], w_xywh), f'image {b}: xywh'
        assert torch.equal(xyxyn[b, :n], w_xyxyn), f'image {b}: xyxyn'
        assert torch.equal(xywhn[b, :n], w_xywhn), f'image {b}: xywhn'
        # beyond count: det bit-unchanged, the views zero
        assert torch.equal(det[b, n:], det0[b, n:]) and (det[b, n:] == SENTINEL).all()
        for v in (xywh, xyxyn, xywhn):
            assert not v[b, n:].any()
    assert low > 0 and high > 0   # the clamp acted on both sides


@pytest.mark.gpu
def test_gpu_scale_boxes_without_views():
    det0 = _case()
    descs = _descs(CANVAS)
    det = det0.cuda()
    assert G.scale_boxes(det, torch.tensor(COUNTS, dtype=torch.int32).cuda(), descs, views=False) is None
    for b, (shape, n) in enumerate(zip(SHAPES, COUNTS)):
        assert torch.equal(det[b, :n, :4].cpu(), nms_ref.scale_coords(CANVAS, det0[b, :n, :4], shape))
        assert torch.equal(det[b, :, 4:].cpu(), det0[b, :, 4:])
