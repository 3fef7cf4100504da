"""The image entry points on models of another channel count, with the frame mode stated: autoShape,
Detections.render, detect.py --frames and test.py --frames / test(frames=).

Every result is compared with == / torch.equal against a reference chain the test runs itself: the CPU letterbox of
tests/letterbox_channels_ref.py -> the same model on that tensor -> nms_batched (or the per-image NMS list) ->
scale_boxes.  yolov7-tiny with seeded synthetic weights at 64 pixels; frames are a few dozen pixels."""
import contextlib
import io
import os
import random
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import letterbox_channels_ref as H
from models.yolo import Model
from test_evaluate_cpu import load_test_entry
from utils import datasets as D
from utils import general as G
from utils import plots
from yv7.arch import get_cfg
from yv7.synthetic import synthetic_frames, synthetic_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZE = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WEIGHTS = {}


def weights(C):
    if C not in _WEIGHTS:
        _WEIGHTS[C] = synthetic_state_dict(Model('yolov7-tiny', ch=C), seed=0, calib_hw=128)
    return _WEIGHTS[C]


def fresh(C, half):
    m = Model('yolov7-tiny', ch=C)
    m.load_state_dict(weights(C))
    m = m.float().fuse().eval().to(DEV)
    return m.half() if half else m


def frame(h, w, C, seed):
    """A uint8 [h, w, C] frame with the structure the weights were calibrated on."""
    x = synthetic_frames(1, h, w, seed=seed, ch=C)[0]
    return np.ascontiguousarray((x * 255).round().clamp(0, 255).byte().permute(1, 2, 0).numpy())


def reference_autoshape(model, frames, conf, iou):
    """frames: uint8 [h, w, C] arrays -> (det, count, (xywh, xyxyn, xywhn)) on the device, and the batch tensor."""
    half = next(model.parameters()).dtype == torch.float16
    C = frames[0].shape[2]
    shape1, geoms, descs = D.autoshape_geometry([f.shape[:2] for f in frames], SIZE, int(model.stride.max()))
    x = torch.stack([H.to_planes(H.place(f, g[0], g[3], [114] * C), half) for f, g in zip(frames, geoms)]).to(DEV)
    assert list(x.shape[2:]) == shape1
    with torch.no_grad():
        y = model(x)[0]
    det, _, cnt = G.nms_batched(y, conf_thres=conf, iou_thres=iou, classes=None)
    views = G.scale_boxes(det, cnt, descs, round_boxes=False, views=True)
    return det, cnt, views, x


def assert_detections_equal(res, det, cnt, views):
    counts = cnt.tolist()
    assert sum(counts) > 0, 'the fixture must produce detections'
    for i, c in enumerate(counts):
        assert torch.equal(res.pred[i], det[i, :c]) and res.pred[i].shape == (c, 6)
        for got, want in zip((res.xywh, res.xyxyn, res.xywhn), views):
            assert torch.equal(got[i], want[i, :c])


SHAPES = [(48, 64), (40, 30), (70, 50)]


@pytest.mark.parametrize('half', [True, False], ids=['fp16', 'fp32'])
def test_autoshape_gray_files_images_and_arrays(half, tmp_path):
    frames = [frame(h, w, 1, 3 + i) for i, (h, w) in enumerate(SHAPES)]
    Image.fromarray(frames[0][:, :, 0], 'L').save(tmp_path / 'a.png')
    model = fresh(1, half)
    a = model.autoshape(frames='L')
    a.conf = 0.1
    inputs = [str(tmp_path / 'a.png'), Image.fromarray(frames[1][:, :, 0], 'L'), frames[2][:, :, 0]]   # file, PIL, HW
    res = a(inputs, size=SIZE)
    det, cnt, views, x = reference_autoshape(model, frames, 0.1, a.iou)
    assert tuple(res.s) == tuple(x.shape) and res.files == ['a.jpg', 'image1.jpg', 'image2.jpg']
    assert_detections_equal(res, det, cnt, views)
    # render(): the boxes on the 3-channel display copies
    want = plots.plot_boxes([np.repeat(f, 3, axis=2) for f in frames], det.clone(), cnt, names=a.names,
                            colors=plots.color_list(), reverse=False)
    out = res.render()
    assert len(out) == 3
    drawn = 0
    for f, o, w in zip(frames, out, want):
        assert isinstance(o, np.ndarray) and o.shape == f.shape[:2] + (3,) and np.array_equal(o, w.cpu().numpy())
        drawn += int((o != np.repeat(f, 3, axis=2)).sum())
    assert drawn > 0


@pytest.mark.parametrize('half', [True, False], ids=['fp16', 'fp32'])
def test_autoshape_rgba(half, tmp_path):
    frames = [frame(h, w, 4, 13 + i) for i, (h, w) in enumerate(SHAPES)]
    Image.fromarray(frames[0], 'RGBA').save(tmp_path / 'a.png')
    model = fresh(4, half)
    a = model.autoshape(frames='RGBA')
    a.conf = 0.1
    chw = np.ascontiguousarray(frames[2].transpose(2, 0, 1))
    res = a([tmp_path / 'a.png', Image.fromarray(frames[1], 'RGBA'), chw], size=SIZE)
    assert_detections_equal(res, *reference_autoshape(model, frames, 0.1, a.iou)[:3])
    with pytest.raises(ValueError, match=r'expected an image of 4 channels .* got shape \(48, 64, 3\)'):
        a([frames[0][:, :, :3]], size=SIZE)


@pytest.mark.parametrize('half', [True, False], ids=['fp16', 'fp32'])
def test_autoshape_raw_five_channels_from_npy_and_tensors(half, tmp_path):
    frames = [frame(h, w, 5, 23 + i) for i, (h, w) in enumerate(SHAPES)]
    for i, f in enumerate(frames):
        np.save(tmp_path / f'{i}.npy', f)
    model = fresh(5, half)
    a = model.autoshape(frames='raw')
    a.conf = 0.1
    det, cnt, views, _ = reference_autoshape(model, frames, 0.1, a.iou)
    assert_detections_equal(a([str(tmp_path / f'{i}.npy') for i in range(3)], size=SIZE), det, cnt, views)
    res = a([torch.from_numpy(f).to(DEV) for f in frames], size=SIZE)
    assert_detections_equal(res, det, cnt, views)
    out = res.render()          # HIP tensors in: display copies on the device out, the frames themselves untouched
    assert all(isinstance(o, torch.Tensor) and o.shape == f.shape[:2] + (3,) for o, f in zip(out, frames))
    with pytest.raises(ValueError, match=r'0\.npy: a \.npy array is read'):
        fresh(1, half).autoshape(frames='L')([str(tmp_path / '0.npy')], size=SIZE)


# ------------------------------------------------------------------------------------------ detect.py
@pytest.fixture(scope='module')
def gray(tmp_path_factory):
    """A 1-channel checkpoint with its cfg, and a folder of pictures: gray PNGs and one RGB JPEG."""
    root = tmp_path_factory.mktemp('gray')
    ckpt, cfgp = root / 'gray.pt', root / 'gray.yaml'
    torch.save({'model': weights(1)}, ckpt)
    cfg = get_cfg('yolov7-tiny')
    cfg['ch'] = 1
    cfgp.write_text(yaml.safe_dump(cfg))
    src = root / 'source'
    src.mkdir()
    Image.fromarray(frame(48, 64, 1, 31)[:, :, 0], 'L').save(src / 'gray.png')
    Image.fromarray(frame(50, 40, 3, 32), 'RGB').save(src / 'rgb.jpg', quality=95)
    return dict(root=root, ckpt=str(ckpt), cfg=str(cfgp), source=src)


def txt_lines(det, shape):
    """detect.py's --save-txt --save-conf lines for one image's rows."""
    gn = torch.tensor(shape)[[1, 0, 1, 0]]
    out = []
    for *xyxy, conf, cls in reversed(det):
        xywh = (G.xyxy2xywh(torch.tensor(xyxy).view(1, 4)) / gn).view(-1).tolist()
        line = (cls, *xywh, conf)
        out.append(('%g ' * len(line)).rstrip() % line)
    return out


@pytest.mark.parametrize('batch,fp32', [(2, False), (1, True)], ids=['batch2-fp16', 'one-by-one-fp32'])
def test_detect_frames_l(gray, batch, fp32, tmp_path):
    import detect
    argv = ['--weights', gray['ckpt'], '--cfg', gray['cfg'], '--source', str(gray['source']), '--img-size', str(SIZE),
            '--frames', 'L', '--save-txt', '--save-conf', '--save-img', '--batch-size', str(batch), '--conf-thres',
            '0.1', '--project', str(tmp_path), '--name', 'out', '--quiet'] + (['--fp32'] if fp32 else [])
    opt = detect.parse_opt(argv)
    results = detect.detect(opt)
    model = detect.load_model(opt, torch.device(DEV))
    model = model.float() if fp32 else model.half()
    paths = sorted(str(p) for p in gray['source'].iterdir())
    assert [p for p, _ in results] == paths
    total = 0
    for (path, got) in results:
        im0 = D.imread(path, 'L')
        assert im0.shape[2] == 1
        lb, _, _ = H.letterbox(im0, (SIZE, SIZE), [114])
        if batch > 1:   # the ragged letterbox converts: (float)v / 255.0f, rounded once
            x = H.to_planes(lb, half=not fp32)[None].to(DEV)
        else:           # the reference's own loop converts the uint8 frame with torch on the device (detect.py:
            #             100-104, unchanged here), whose division by a host scalar is not the exact quotient in
            #             every last bit (tests/test_detect.py bounds that path instead of comparing it bit for bit)
            x = torch.from_numpy(np.ascontiguousarray(lb.transpose(2, 0, 1))).to(DEV)
            x = x.float() if fp32 else x.half()
            x /= 255.0
            x = x[None]
        with torch.no_grad():
            y = model(x)[0]
        if batch > 1:
            det, _, cnt = G.nms_batched(y, 0.1, 0.45, classes=None, agnostic=False)
            G.scale_boxes(det, cnt, [G.scale_desc((SIZE, SIZE), im0.shape)], round_boxes=True, views=False)
        else:   # the reference's own loop: the per-image list, scale_coords().round()
            d = G.non_max_suppression(y, 0.1, 0.45, classes=None, agnostic=False)[0]
            d[:, :4] = G.scale_coords(x.shape[2:], d[:, :4], im0.shape).round()
            det, cnt = d[None].float().contiguous(), torch.tensor([len(d)], dtype=torch.int32, device=DEV)
        n = int(cnt[0])
        total += n
        assert torch.equal(got, det[0, :n].cpu())
        txt = tmp_path / 'out' / 'labels' / (Path(path).stem + '.txt')
        if n:
            assert txt.read_text().splitlines() == txt_lines(det[0, :n].cpu(), im0.shape)
        else:
            assert not txt.exists()
        saved = tmp_path / 'out' / Path(path).name
        assert saved.is_file()
        if saved.suffix == '.png':   # lossless: the display copy with the boxes drawn
            want = plots.plot_boxes([np.repeat(im0, 3, axis=2)], det, cnt, names=model.names,
                                    colors=plots.color_list(), line_thickness=1, reverse=True)[0]
            with Image.open(saved) as im:
                assert im.mode == 'RGB' and np.array_equal(np.asarray(im), want.cpu().numpy())
            assert n and (want.cpu().numpy() != np.repeat(im0, 3, axis=2)).any()
    assert total > 0


def test_detect_refuses_a_file_of_another_channel_count(gray, tmp_path):
    import detect
    opt = detect.parse_opt(['--weights', gray['ckpt'], '--cfg', gray['cfg'], '--source', str(gray['source']),
                            '--img-size', str(SIZE), '--frames', 'raw', '--batch-size', '2', '--quiet'])
    with pytest.raises(ValueError, match=r'rgb\.jpg: holds 3-channel frames, the model takes 1'):
        detect.detect(opt)


# ------------------------------------------------------------------------------------------ test.py
CONF, IOU = 0.001, 0.6
CROPS = [(100, 300, 120, 90), (300, 200, 90, 120), (50, 500, 64, 64), (200, 400, 128, 96)]   # left, top, w, h


class HelperLoader:
    """Batches built on the CPU by the helper from PIL's 'L' conversion of each file: [nb, 1, h, w] half planes in
    pinned memory, with the package's own targets, paths and shapes.  With probe, the step that handles the second
    batch runs under sync debug mode 'error' (tests/test_evaluate.py ForeignLoader)."""

    def __init__(self, path, batch, probe=False):
        self.probe, self.batches = probe, []
        loader, ds = D.create_dataloader('Test', path, SIZE, batch, 32, pad=0.5, rect=True, frames='L', channels=1)
        self.dataset = ds
        for k, (img, targets, paths, shapes) in enumerate(loader):
            idx = range(k * batch, min((k + 1) * batch, len(ds)))
            planes = []
            for i in idx:
                with Image.open(ds.img_files[i]) as im:
                    f = np.asarray(im.convert('L'))[:, :, None]
                (nw_nh, _, _, border) = ds.geometry(i)[2]
                planes.append(H.to_planes(H.place(f, nw_nh, border, [114]), half=True))
            mine = torch.stack(planes)
            assert tuple(mine.shape[2:]) == ds.canvas(idx[0]) and torch.equal(mine, img.cpu())   # the loader's batch
            self.batches.append((mine.pin_memory(), targets.pin_memory(), paths, shapes))

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        for k, b in enumerate(self.batches):
            if self.probe and k == 1:
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode('error')
            try:
                yield b
            finally:
                if self.probe and k == 1:
                    torch.cuda.set_sync_debug_mode('default')


@pytest.fixture(scope='module')
def grayset(gray):
    """Four crops of the golden picture, three stored gray and one RGB, with labels from the model's own
    detections mixed with random boxes."""
    root = gray['root'] / 'set'
    (root / 'images').mkdir(parents=True)
    (root / 'labels').mkdir()
    bus = Image.open(os.path.join(ROOT, 'tests', 'golden', 'bus.jpg')).convert('RGB')
    for i, (l, t, w, h) in enumerate(CROPS):
        crop = bus.crop((l, t, l + w, t + h))
        (crop if i == 1 else crop.convert('L')).save(root / 'images' / f'{i:06d}.png')
    path = str(root / 'images')
    T = load_test_entry()
    T.opt.cfg = gray['cfg']
    model = T.load_model([gray['ckpt']], torch.device(DEV)).half()
    rng = random.Random(5)
    with torch.no_grad():
        for img, _, paths, shapes in HelperLoader(path, 2):
            out = G.non_max_suppression(model(img.to(DEV))[0], 0.25, 0.45)
            for si, det in enumerate(out):
                (h0, w0), ratio_pad = shapes[si]
                det = det.cpu().clone()
                G.scale_coords(img.shape[2:], det[:, :4], (h0, w0), ratio_pad)
                rows = [(int(c), (x1 + x2) / 2 / w0, (y1 + y2) / 2 / h0, (x2 - x1) / w0, (y2 - y1) / h0)
                        for x1, y1, x2, y2, _, c in det[:6].tolist() if x2 > x1 and y2 > y1]
                rows += [(rng.randrange(80), rng.uniform(.2, .8), rng.uniform(.2, .8), rng.uniform(.05, .3),
                          rng.uniform(.05, .3)) for _ in range(2)]
                (root / 'labels' / (Path(paths[si]).stem + '.txt')).write_text(
                    ''.join('%d %.6f %.6f %.6f %.6f\n' % r for r in rows))
    data = root / 'gray.yaml'
    data.write_text(f'nc: 80\nval: {path}\nnames: {[str(i) for i in range(80)]}\n')
    return dict(path=path, data=str(data), T=T, model=model, ckpt=gray['ckpt'])


def sync_debug_mode_flags_a_sync():
    """Whether torch's sync debug mode 'error' raises on a .item() in this build: without that it shows nothing."""
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            torch.ones(1, device='cuda').item()
        except RuntimeError:
            return True
        finally:
            torch.cuda.set_sync_debug_mode('default')
    except AttributeError:
        pass
    return False


def run_test(T, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return T.test(*args, imgsz=SIZE, conf_thres=CONF, iou_thres=IOU, **kw)


@pytest.mark.parametrize('batch', [1, 2])
def test_test_frames_l_equals_the_helper_built_batches(grayset, batch, tmp_path):
    probe = sync_debug_mode_flags_a_sync()
    w = grayset
    T = w['T']
    pictures = {f'test_batch{k}_{kind}.jpg' for k in range(min(3, 4 // batch)) for kind in ('labels', 'pred')}
    (tmp_path / 'ref').mkdir()
    # the explicit dataloader, its second step under sync debug mode, pictures on
    ref = run_test(T, w['data'], batch_size=batch, model=w['model'], save_dir=tmp_path / 'ref', plots=True,
                   dataloader=HelperLoader(w['path'], batch, probe=probe), frames='L')
    assert pictures <= {p.name for p in (tmp_path / 'ref').iterdir()}
    # test.py's own loader from the files
    T.opt.project, T.opt.name, T.opt.exist_ok = str(tmp_path), 'own', False
    got = run_test(T, w['data'], weights=[w['ckpt']], batch_size=batch, frames='L', plots=True, save_json=False,
                   save_txt=True)
    assert got[0][:4] == ref[0][:4] and np.array_equal(got[1], ref[1])
    assert 0 < got[0][2] < 1, 'the fixture must produce matches and misses'
    names = {p.name for p in (tmp_path / 'own').iterdir()}
    assert pictures <= names and (len(pictures) == 6 or batch == 2)
    for name in pictures:   # the same pictures from both runs
        assert (tmp_path / 'own' / name).read_bytes() == (tmp_path / 'ref' / name).read_bytes()
    assert len(list((tmp_path / 'own' / 'labels').iterdir())) == 4


def test_test_without_frames_still_refuses_the_gray_model(grayset, tmp_path):
    T = grayset['T']
    T.opt.project, T.opt.name = str(tmp_path), 'refused'
    with pytest.raises(RuntimeError, match='this entry point loads 3-channel images'):
        run_test(T, grayset['data'], weights=[grayset['ckpt']], batch_size=2)
