"""models.common.autoShape / Detections / NMS, Model.autoshape() and detect.py --batch-size.

CPU: Detections assembled from given tensors (len, tolist, pandas, print).
GPU (yolov7-tiny, synthetic weights, size 64): autoShape on six RGB frames of six sizes against the chain it
replaces — oracle letterbox -> model(x) -> non_max_suppression -> the oracle's scale_coords on the CPU — with
torch.equal: the pre- and post-processing kernels are bit-exact and the forward sees the same input at the same
batch size.  At 64 x 64 the head has 252 rows, so no image can reach the 300-detection cut; CONF below is the
class default, at which the synthetic head keeps detections in every one of these frames (asserted)."""
import os

import numpy as np
import pytest
import torch

from helpers import fresh_model
from models.common import NMS, Detections, autoShape

BUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bus.jpg')
BATCH_A = [(48, 64), (64, 48), (33, 51), (128, 128), (64, 64), (20, 61)]
CONF = 0.25   # autoShape.conf's default


# ------------------------------------------------------------------------------------------ CPU
def _hand_made():
    imgs = [np.zeros((100, 200, 3), np.uint8), np.zeros((50, 40, 3), np.uint8)]
    pred = [torch.tensor([[20., 10., 60., 50., 0.875, 0.], [0., 0., 200., 100., 0.75, 2.], [10., 20., 30., 40., 0.5, 0.]]),
            torch.zeros((0, 6))]
    return Detections(imgs, pred, ['a.jpg', 'b.jpg'], times=[0.0, 0.002, 0.006, 0.012],
                      names=['person', 'bicycle', 'car'], shape=(2, 3, 64, 128))


def test_class_attributes_are_the_reference_defaults():
    for cls in (autoShape, NMS):
        assert (cls.conf, cls.iou, cls.classes) == (0.25, 0.45, None)


def test_detections_from_cpu_tensors(capsys):
    d = _hand_made()
    assert len(d) == 2 and d.n == 2 and d.s == (2, 3, 64, 128)
    assert d.t == pytest.approx((1.0, 2.0, 3.0))                   # ms per image
    assert d.xyxy is d.pred
    assert d.xywh[0][0].tolist() == [40., 30., 40., 40., 0.875, 0.]
    assert d.xyxyn[0][1].tolist() == [0., 0., 1., 1., 0.75, 2.]
    assert d.xywhn[0][0].tolist() == pytest.approx([0.2, 0.3, 0.2, 0.4, 0.875, 0.])
    assert d.xywh[1].shape == (0, 6)
    d.print()
    out = capsys.readouterr().out.splitlines()
    assert out[0] == 'image 1/2: 100x200 2 persons, 1 car'
    assert out[1] == 'image 2/2: 50x40'
    assert out[2] == 'Speed: 1.0ms pre-process, 2.0ms inference, 3.0ms NMS per image at shape (2, 3, 64, 128)'
    for method in (d.show, d.save, d.render):
        with pytest.raises(NotImplementedError):
            method()


def test_detections_tolist_and_pandas():
    d = _hand_made()
    parts = d.tolist()
    assert len(parts) == 2 and all(isinstance(p, Detections) and len(p) == 1 for p in parts)
    for i, p in enumerate(parts):
        assert p.imgs is d.imgs[i] and p.files == [d.files[i]] and p.names == d.names and p.s == d.s
        for k in ('pred', 'xyxy', 'xywh', 'xyxyn', 'xywhn'):
            assert torch.equal(getattr(p, k), getattr(d, k)[i])
    pd = d.pandas()
    assert list(pd.xyxy[0].columns) == ['xmin', 'ymin', 'xmax', 'ymax', 'confidence', 'class', 'name']
    assert list(pd.xyxyn[0].columns) == list(pd.xyxy[0].columns)
    assert list(pd.xywh[0].columns) == ['xcenter', 'ycenter', 'width', 'height', 'confidence', 'class', 'name']
    assert list(pd.xywhn[0].columns) == list(pd.xywh[0].columns)
    assert pd.xyxy[0]['name'].tolist() == ['person', 'car', 'person'] and pd.xyxy[0]['class'].tolist() == [0, 2, 0]
    assert len(pd.xyxy[1]) == 0
    assert isinstance(d.xyxy[0], torch.Tensor)                      # the original is untouched


def test_autoshape_rejects_what_it_cannot_take():
    from models.common import _as_hwc3
    with pytest.raises(ValueError, match='uint8'):
        _as_hwc3(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError, match='uint8'):
        _as_hwc3(torch.zeros(8, 8, 3))
    assert _as_hwc3(np.zeros((3, 8, 9), np.uint8)).shape == (8, 9, 3)      # CHW
    assert _as_hwc3(np.zeros((8, 9, 4), np.uint8)).shape == (8, 9, 3)      # alpha dropped
    assert _as_hwc3(np.zeros((8, 9), np.uint8)).shape == (8, 9, 3)         # grey tiled


# ------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope='module')
def tiny():
    return fresh_model('yolov7-tiny').cuda()


def _frames(shapes, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in shapes]


def _cpu_views(x, shape):
    gn = torch.tensor([shape[1], shape[0], shape[1], shape[0], 1., 1.])
    xywh = x.clone()
    xywh[:, 0] = (x[:, 0] + x[:, 2]) / 2
    xywh[:, 1] = (x[:, 1] + x[:, 3]) / 2
    xywh[:, 2] = x[:, 2] - x[:, 0]
    xywh[:, 3] = x[:, 3] - x[:, 1]
    return xywh, x / gn, xywh / gn


def _chain(model, frames, canvas, conf, bgr=False, round_boxes=False):
    """The reference's steps on the same model: oracle letterbox (auto=False) -> model -> NMS -> CPU scale_coords."""
    from oracle import letterbox_ref as R, nms_ref
    from utils.general import non_max_suppression
    x = torch.stack([R.to_input(lb if bgr else lb[:, :, ::-1]) for lb in
                     (R.letterbox(f, canvas, auto=False)[0] for f in frames)])
    with torch.no_grad():
        y = model(x.cuda())[0]
    out = []
    for f, det in zip(frames, non_max_suppression(y, conf, 0.45)):
        det = det.cpu().clone()
        det[:, :4] = nms_ref.scale_coords(canvas, det[:, :4], f.shape)
        if round_boxes:
            det[:, :4] = det[:, :4].round()
        out.append(det)
    return out


@pytest.mark.gpu
def test_gpu_autoshape_equals_the_reference_chain(tiny):
    frames = _frames(BATCH_A, 21)
    a = tiny.autoshape()
    assert isinstance(a, autoShape) and a.names == tiny.names and a.stride is tiny.stride and a.yaml is tiny.yaml
    assert a.autoshape() is a
    a.conf = CONF
    res = a([f.copy() for f in frames], size=64)
    assert isinstance(res, Detections) and len(res) == 6 and tuple(res.s) == (6, 3, 64, 64)
    assert res.files == [f'image{i}.jpg' for i in range(6)]
    want = _chain(tiny, frames, (64, 64), CONF)
    counts = [len(p) for p in res.pred]
    print(f'\nautoShape conf {CONF}: detections per image {counts}')
    assert max(counts) > 0 and max(counts) < 300
    for i, (p, w) in enumerate(zip(res.pred, want)):
        assert torch.equal(p.cpu(), w), f'image {i}: pred'
        for got, ref, k in zip((res.xywh[i], res.xyxyn[i], res.xywhn[i]), _cpu_views(w, BATCH_A[i]),
                               ('xywh', 'xyxyn', 'xywhn')):
            assert torch.equal(got.cpu(), ref), f'image {i}: {k}'
    # one image, not in a list; a float tensor goes straight to the model
    one = a(frames[2].copy(), size=64)
    assert len(one) == 1 and one.files == ['image0.jpg'] and tuple(one.s)[0] == 1
    z = a(torch.zeros(1, 3, 64, 64))
    assert z[0].shape == (1, 252, 85)


@pytest.mark.gpu
def test_gpu_autoshape_fp16():
    m = fresh_model('yolov7-tiny').half().cuda()
    res = m.autoshape()(_frames(BATCH_A, 22), size=64)
    assert tuple(res.s) == (6, 3, 64, 64)
    for (h, w), p in zip(BATCH_A, res.pred):
        p = p.cpu()
        assert p.dtype == torch.float32 and torch.isfinite(p).all()
        assert (p[:, [0, 2]] >= 0).all() and (p[:, [0, 2]] <= w).all()
        assert (p[:, [1, 3]] >= 0).all() and (p[:, [1, 3]] <= h).all()


@pytest.mark.gpu
def test_gpu_autoshape_filename_and_pil(tiny):
    from PIL import Image
    pil = Image.fromarray(_frames([(40, 56)], 23)[0])
    res = tiny.autoshape()([BUS, pil], size=64)
    assert res.files == ['bus.jpg', 'image1.jpg']
    assert res.imgs[0].shape == (1080, 810, 3) and res.imgs[1].shape == (40, 56, 3)
    assert tuple(res.s) == (2, 3, 64, 64) and len(res.pred) == 2
    with pytest.raises(ValueError, match='uint8'):
        tiny.autoshape()([np.zeros((8, 8, 3), np.float32)], size=64)


@pytest.mark.gpu
def test_gpu_autoshape_hip_tensor_frames(tiny):
    """uint8 HWC tensors already on the device are read in place: same results as the numpy frames."""
    frames = _frames(BATCH_A[:3], 25)
    a = tiny.autoshape()
    host = a([f.copy() for f in frames], size=64)
    mixed = a([torch.from_numpy(frames[0]).cuda(), frames[1].copy(), torch.from_numpy(frames[2]).cuda()], size=64)
    assert sum(len(p) for p in host.pred) > 0
    for p, q in zip(host.pred, mixed.pred):
        assert torch.equal(p, q)
    assert isinstance(mixed.imgs[0], torch.Tensor) and isinstance(mixed.imgs[1], np.ndarray)


@pytest.fixture
def png_dir(tmp_path):
    from PIL import Image
    for name, f in zip('abc', _frames([(48, 64), (33, 51), (128, 128)], 24)):
        Image.fromarray(f).save(tmp_path / f'{name}.png')
    return tmp_path


def _run_detect(png_dir, batch):
    import detect
    return detect.detect(detect.parse_opt(['--cfg', 'yolov7-tiny', '--fp32', '--source', str(png_dir), '--img-size', '64',
                                           '--batch-size', str(batch), '--quiet']))


@pytest.mark.gpu
def test_gpu_detect_batch_size_3(png_dir, tiny, monkeypatch):
    import detect
    from utils.datasets import imread, letterbox_ragged
    calls = []
    monkeypatch.setattr(detect, 'letterbox_ragged',
                        lambda *a, **k: calls.append(len(a[0])) or letterbox_ragged(*a, **k))
    got = _run_detect(png_dir, 3)
    assert calls == [3]
    paths = sorted(str(p) for p in png_dir.iterdir())
    assert [p for p, _ in got] == paths
    want = _chain(tiny, [imread(p) for p in paths], (64, 64), 0.25, bgr=True, round_boxes=True)
    assert sum(len(w) for w in want) > 0
    for (p, d), w in zip(got, want):
        assert not d.is_cuda and torch.equal(d, w), p
    # a short last group: 3 files at --batch-size 2
    calls.clear()
    got2 = _run_detect(png_dir, 2)
    assert calls == [2, 1] and [p for p, _ in got2] == paths


@pytest.mark.gpu
def test_gpu_detect_batch_size_1_takes_the_old_loop(png_dir, monkeypatch):
    import detect
    from utils import datasets
    ragged, single = [], []
    monkeypatch.setattr(detect, 'letterbox_ragged', lambda *a, **k: ragged.append(1))
    real = datasets.letterbox
    monkeypatch.setattr(datasets, 'letterbox', lambda *a, **k: single.append(1) or real(*a, **k))
    got = _run_detect(png_dir, 1)
    assert len(got) == 3 and len(single) == 3 and not ragged
