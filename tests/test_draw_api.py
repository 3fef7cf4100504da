"""Detections.render / save and detect.py --save-img (yolov7-tiny, synthetic weights, size 64): the annotated images
equal the numpy restatement of the drawing contract (tests/draw_ref.py) applied to the original frames and the
detections the same call returns."""
import os

import numpy as np
import pytest
import torch

import draw_ref as R
from helpers import fresh_model
from utils import plots

pytestmark = pytest.mark.gpu

BUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bus.jpg')
BATCH_A = [(48, 64), (64, 48), (33, 51), (128, 128), (64, 64), (20, 61)]     # tests/test_autoshape.py's sizes


@pytest.fixture(scope='module')
def tiny():
    return fresh_model('yolov7-tiny').cuda()


def _frames(shapes, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in shapes]


def _want(frame, pred, names, palette, t, reverse=False):
    return R.draw(frame, pred.cpu().numpy(), palette, t, names=[n.encode() for n in names],
                  atlas=plots.glyph_atlas_host(plots.text_height(t)), reverse=reverse)


def test_gpu_render_equals_the_restatement(tiny):
    frames = _frames(BATCH_A, 21)
    given = [f.copy() for f in frames]
    given[1] = torch.from_numpy(frames[1]).cuda()          # a HIP-tensor image is drawn in place
    res = tiny.autoshape()(list(given), size=64)
    counts = [len(p) for p in res.pred]
    print(f'\ndetections per image {counts}')
    assert min(counts) > 0
    pred = [p.clone() for p in res.pred]
    out = res.render()
    assert out is res.imgs and len(out) == 6
    for i, (f, p) in enumerate(zip(frames, pred)):
        want = _want(f, p, tiny.names, plots.color_list(), plots.line_thickness(f.shape))
        assert (want != f).any()
        got = out[i]
        if i == 1:
            assert isinstance(got, torch.Tensor) and got.data_ptr() == given[1].data_ptr()
            got = got.cpu().numpy()
        else:
            assert isinstance(got, np.ndarray) and np.array_equal(given[i], f)      # the caller's array is left alone
        assert np.array_equal(got, want), f'image {i}'
        assert torch.equal(res.pred[i], p)
    # results assembled by hand from device tensors take the same path
    from models.common import Detections
    by_hand = Detections([f.copy() for f in frames], pred, res.files, names=tiny.names)
    for i, (got, f, p) in enumerate(zip(by_hand.render(), frames, pred)):
        assert np.array_equal(got, _want(f, p, tiny.names, plots.color_list(), plots.line_thickness(f.shape))), i


def test_gpu_save_writes_what_pil_writes(tiny, tmp_path, capsys):
    from PIL import Image
    frames = _frames(BATCH_A[:3], 22)
    res = tiny.autoshape()([f.copy() for f in frames], size=64)
    res.files = ['a.png', 'b.jpg', 'c.png']
    out = tmp_path / 'run'
    res.save(str(out))
    assert sorted(p.name for p in out.iterdir()) == res.files
    assert 'Saved a.png, b.jpg, c.png to' in capsys.readouterr().out
    for im, f, orig, p in zip(res.imgs, res.files, frames, res.pred):
        assert np.array_equal(im, _want(orig, p, tiny.names, plots.color_list(), plots.line_thickness(orig.shape)))
        Image.fromarray(im).save(tmp_path / f)
        assert (out / f).read_bytes() == (tmp_path / f).read_bytes()
    # the default directory increments (common.py:984), a named one is reused
    res.save(str(out))
    assert len(list(out.iterdir())) == 3


@pytest.fixture
def crops(tmp_path):
    from PIL import Image
    src = tmp_path / 'src'
    src.mkdir()
    bus = Image.open(BUS).convert('RGB')
    for name, (l, t, w, h) in zip('ab', [(0, 300, 405, 540), (200, 100, 333, 251)]):
        bus.crop((l, t, l + w, t + h)).save(src / f'{name}.png')
    return src


@pytest.mark.parametrize('batch', [2, 1])
def test_gpu_detect_save_img(crops, tmp_path, batch):
    import detect
    from PIL import Image
    from utils.datasets import imread
    args = ['--cfg', 'yolov7-tiny', '--fp32', '--source', str(crops), '--img-size', '64', '--batch-size', str(batch),
            '--quiet', '--project', str(tmp_path / 'runs')]
    plain = detect.detect(detect.parse_opt(args + ['--name', 'plain']))
    assert not (tmp_path / 'runs').exists()                                  # without the flag nothing is written
    got = detect.detect(detect.parse_opt(args + ['--name', 'drawn', '--save-img']))
    assert sorted(p.name for p in (tmp_path / 'runs' / 'drawn').iterdir()) == ['a.png', 'b.png']
    names = fresh_model('yolov7-tiny').names
    bgr = [c[::-1] for c in plots.color_list()]
    assert sum(len(d) for _, d in got) > 0
    for (path, d), (path0, d0) in zip(got, plain):
        assert path == path0 and torch.equal(d, d0) and not d.is_cuda       # the results are unchanged
        want = _want(imread(path), d, names, bgr, 1, reverse=True)
        saved = np.asarray(Image.open(tmp_path / 'runs' / 'drawn' / os.path.basename(path)).convert('RGB'))
        assert np.array_equal(saved[:, :, ::-1], want), path
