"""plot_images and test.py's test_batch*_labels.jpg / _pred.jpg on the GPU: the device pictures equal the numpy
restatement of the contract (tests/mosaic_ref.py) with the PIL atlas, plot_images enqueues without a host
synchronisation, and test() writes exactly the reference's six pictures, byte for byte the JPEG of the restatement's
picture, without changing its statistics.

The evaluation fixture is tests/test_evaluate.py's (crops of tests/golden/bus.jpg, labelled), run in batches of 3:
four rectangular batches, the last one a single image."""
import io
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

import mosaic_ref as M
from test_evaluate import CONF, IMGSZ, IOU, ForeignLoader, world  # noqa: F401  (world: the module-scoped fixture)
from test_evaluate import run as run_batches_of_four
from utils import datasets as D
from utils import plots

pytestmark = pytest.mark.gpu

BATCH = 3
PNGS = {'confusion_matrix.png', 'PR_curve.png', 'F1_curve.png', 'P_curve.png', 'R_curve.png'}
JPGS = {f'test_batch{k}_{kind}.jpg' for k in range(3) for kind in ('labels', 'pred')}


def _atlas():
    return plots.glyph_atlas_host(plots.text_height(3))


def _reference(images, names, paths, max_size=640, max_out=1280, **rows):
    g = plots.mosaic_geometry(*images.shape[0:1], *images.shape[2:], max_size=max_size, max_out=max_out)
    raw = [n if isinstance(n, bytes) else str(n).encode() for n in names]
    captions = [Path(paths[i]).name[:40].encode() for i in range(g['n'])] if paths else None
    return M.mosaic(images, g['n'], g['ns'], *g['tile'], g['sf'], *g['out'], palette=plots.color_list(), names=raw,
                    atlas=_atlas(), captions=captions, **rows)


def _require_sync_debug_mode():
    """The probe-and-skip guard of tests/test_evaluate.py."""
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            with pytest.raises(RuntimeError):
                torch.ones(1, device='cuda').item()     # the mode must see a real sync, or it shows nothing
        finally:
            torch.cuda.set_sync_debug_mode('default')
    except (pytest.fail.Exception, AttributeError):
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag a .item() on this ROCm build')


def _batch(rs, B, H, W, max_det, nc):
    images = (rs.rand(B, 3, H, W) * 1.02 - 0.01).astype(np.float16)
    det = np.zeros((B, max_det, 6), np.float32)
    # a quarter-pixel grid, so that xyxy -> xywh -> xyxy is exact in fp32
    x1 = rs.randint(-40, 4 * W - 80, (B, max_det)) / 4
    y1 = rs.randint(-40, 4 * H - 80, (B, max_det)) / 4
    det[:, :, 0], det[:, :, 1] = x1, y1
    det[:, :, 2] = x1 + rs.randint(8, 4 * W // 2, (B, max_det)) / 2
    det[:, :, 3] = y1 + rs.randint(8, 4 * H // 2, (B, max_det)) / 2
    det[:, :, 4] = rs.rand(B, max_det)
    det[:, :, 5] = rs.randint(0, nc + 1, (B, max_det))
    count = rs.randint(0, max_det + 1, B).astype(np.int32)
    count[0], count[-1] = max_det, 0
    return images, det, count


def _plot_images_case():
    rs = np.random.RandomState(21)
    B, H, W, max_det = 5, 72, 104, 7
    names = ['person', 'bus', 'tie']
    paths = [f'/data/images/some_image_{i:04d}.jpg' for i in range(B)]
    images, det, count = _batch(rs, B, H, W, max_det, len(names))
    kw = dict(max_size=64, max_out=100)          # sf < 1: bilinear tiles 45 x 64, a 3 x 3 grid, and a downscale
    dev = dict(images=torch.from_numpy(images).cuda(), det=torch.from_numpy(det).cuda(),
               count=torch.from_numpy(count).cuda())
    per = [3, 0, 4, 2, 1]
    t = np.zeros((sum(per), 6), np.float32)
    t[:, 0] = np.repeat(np.arange(B), per)
    t[:, 1] = rs.randint(0, len(names), len(t))
    t[:, 2:4] = rs.rand(len(t), 2)
    t[:, 4:6] = rs.rand(len(t), 2) * 0.5
    off = np.concatenate(([0], np.cumsum(per))).astype(np.int32)
    t_dev, off_dev = torch.from_numpy(t).cuda(), torch.from_numpy(off).cuda()

    def both():
        return (plots.plot_images(dev['images'], (dev['det'], dev['count']), paths, None, names, **kw),
                plots.plot_images(dev['images'], t_dev, paths, None, names, label_off=off_dev, **kw))

    return locals()


def test_plot_images_does_not_synchronise():
    _require_sync_debug_mode()
    both = _plot_images_case()['both']
    first = both()                 # fills the atlas / names / palette caches, which upload once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        pred, lab = both()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(pred, first[0]) and torch.equal(lab, first[1])


def test_plot_images_equals_the_restatement():
    c = _plot_images_case()
    images, det, count, t, off, names, paths, kw, dev, t_dev, per = (
        c[k] for k in ('images', 'det', 'count', 't', 'off', 'names', 'paths', 'kw', 'dev', 't_dev', 'per'))
    pred, lab = c['both']()
    want = _reference(images, names, paths, det=det, count=count, **kw)
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == want.shape and want.shape[1] == 100
    assert np.array_equal(pred.cpu().numpy(), want)
    want = _reference(images, names, paths, targets=t, label_off=off, normalized=True, **kw)
    assert np.array_equal(lab.cpu().numpy(), want)
    # label_off counted on the device, and the same rows from the host in any order
    assert torch.equal(plots.plot_images(dev['images'], t_dev, paths, None, names, **kw), lab)
    mixed = t[np.argsort(-t[:, 0], kind='stable')]      # images descending, each image's rows in their order
    assert torch.equal(plots.plot_images(dev['images'], mixed, paths, None, names, **kw), lab)
    # the reference's [n, 7] host rows give the picture of the equivalent (det, count)
    host = plots.output_to_target((dev['det'], dev['count']))
    assert host.shape == (int(count.sum()), 7)
    assert torch.equal(plots.plot_images(dev['images'], host, paths, None, names, **kw), pred)
    # names=None: the class index in decimal; no targets: tiles, captions and borders
    got = plots.plot_images(dev['images'], (dev['det'], dev['count']), None, None, None, **kw)
    want = _reference(images, [str(i) for i in range(1024)], None, det=det, count=count, **kw)
    assert np.array_equal(got.cpu().numpy(), want)
    got = plots.plot_images(dev['images'].float(), None, paths, None, names, **kw)
    assert np.array_equal(got.cpu().numpy(), _reference(images.astype(np.float32), names, paths, **kw))


def test_plot_images_saves_with_pil(tmp_path):
    rs = np.random.RandomState(22)
    images = torch.from_numpy(rs.randint(0, 256, (2, 3, 40, 56)).astype(np.uint8)).cuda()
    f = tmp_path / 'images.jpg'
    out = plots.plot_images(images, None, ['a.jpg', 'b.jpg'], str(f))
    buf = io.BytesIO()
    Image.fromarray(out.cpu().numpy()).save(buf, 'JPEG')
    assert f.read_bytes() == buf.getvalue() and tuple(out.shape) == (80, 112, 3)


def _loader(path):
    return D.create_dataloader('Test', path, IMGSZ, BATCH, 32, pad=0.5, rect=True)[0]


def _run(w, **kw):
    import contextlib
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        return w['T'].test(w['data'], batch_size=BATCH, imgsz=IMGSZ, conf_thres=CONF, iou_thres=IOU, model=w['model'],
                           dataloader=_loader(w['path']), **kw)


def test_test_writes_the_six_pictures_and_keeps_its_statistics(world, tmp_path, monkeypatch):  # noqa: F811
    w, calls = world, []
    real = w['T'].plot_images

    def spy(images, targets, paths, fname, names, **kw):
        if isinstance(targets, tuple):
            rows = dict(det=targets[0].cpu().numpy().copy(), count=targets[1].cpu().numpy().copy())
        else:
            rows = dict(targets=targets.cpu().numpy().copy(), label_off=kw['label_off'].cpu().numpy().copy(),
                        normalized=kw['normalized'])
        calls.append((images.cpu().numpy().copy(), list(names), list(paths), rows))
        assert fname is None
        return real(images, targets, paths, fname, names, **kw)
    monkeypatch.setattr(w['T'], 'plot_images', spy)
    res = _run(w, plots=True, save_dir=tmp_path)
    assert {p.name for p in tmp_path.iterdir()} == PNGS | JPGS        # and none for batch 3
    assert len(calls) == 6
    for k in range(3):
        for j, kind in enumerate(('labels', 'pred')):
            images, names, paths, rows = calls[2 * k + j]
            assert ('det' in rows) == (kind == 'pred') and images.shape[0] == BATCH
            buf = io.BytesIO()
            Image.fromarray(_reference(images, names, paths, **rows)).save(buf, 'JPEG')
            assert (tmp_path / f'test_batch{k}_{kind}.jpg').read_bytes() == buf.getvalue(), (k, kind)
    # the labels are drawn: the picture with them differs from the one without
    images, names, paths, rows = calls[0]
    assert len(rows['targets']) and not np.array_equal(_reference(images, names, paths, **rows),
                                                       _reference(images, names, paths))
    monkeypatch.setattr(w['T'], 'plot_images', real)
    off = _run(w, plots=False, save_dir=tmp_path / 'off')
    assert res[0] == off[0] and np.array_equal(res[1], off[1]) and res[0][2] > 0


def test_no_pictures_with_plots_off_or_the_default_save_dir(world, tmp_path, monkeypatch):  # noqa: F811
    w = world

    def never(*a, **k):
        raise AssertionError('plot_images must not run')
    monkeypatch.setattr(w['T'], 'plot_images', never)
    monkeypatch.chdir(tmp_path)
    (tmp_path / 'out').mkdir()
    _run(w, plots=False, save_dir=tmp_path / 'out')
    _run(w, plots=True)                                   # a model and the default save_dir
    assert list((tmp_path / 'out').iterdir()) == [] and [p.name for p in tmp_path.iterdir()] == ['out']


def test_enqueue_with_the_pictures_does_not_synchronise(world, tmp_path):  # noqa: F811
    """A uint8 dataloader, plots on and a real save_dir: the step that enqueues batch 1 with its two pictures and
    consumes batch 0 (writing its two files) runs under sync-debug mode 'error'."""
    _require_sync_debug_mode()
    w = world
    res, _ = run_batches_of_four(w, w['data'], model=w['model'], dataloader=ForeignLoader(w['path'], probe=True),
                                 plots=True, save_dir=tmp_path)
    assert {p.name for p in tmp_path.iterdir()} == PNGS | JPGS         # 3 batches of 4, 4 and 2: all get pictures
    assert res[0][:4] == w['ref']['result'][:4]
