"""test.py end to end on the GPU: the batched evaluation equals the reference's per-image chain exactly.

Fixture: ten lossless crops of tests/golden/bus.jpg (aspect ratios on both sides of 1, two of them exactly twice
their target size so the 2x area resize runs), labels that mix yolov7-tiny's own conf-0.25 detections with random
boxes (one image has no label file), imgsz 160 and batches of 4: three rectangular batches, the last one ragged.

Reference, computed once from the same loader's batches: non_max_suppression(multi_label=True) lists, CPU
scale_coords(ratio_pad), oracle.metrics_ref.match_image and oracle.metrics_ref.ap_per_class, arranged as
test.py:130-227 arranges them.  Every stage of the batched path is bit-exact by construction, so the numbers are
compared with ==."""
import contextlib
import io
import json
import os
import random
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import metrics_ref
from test_evaluate_cpu import load_test_entry
from utils import datasets as D
from utils import general as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMGSZ, BATCH, CONF, IOU = 160, 4, 0.001, 0.6
# (left, top, width, height) of each crop of the 810 x 1080 picture
CROPS = [(100, 300, 320, 240), (300, 200, 240, 320), (50, 500, 200, 200), (200, 400, 400, 300), (400, 100, 333, 500),
         (0, 0, 810, 1080), (350, 600, 160, 120), (150, 450, 500, 211), (600, 300, 97, 160), (100, 250, 640, 360)]
NO_LABEL_FILE = 4


def fresh_model():
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    m = Model('yolov7-tiny')
    sd = synthetic_state_dict(m, seed=0)       # head biases raised so that detections exist
    return m, sd


def make_loader(path):
    return D.create_dataloader('Test', path, IMGSZ, BATCH, 32, pad=0.5, rect=True)[0]


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    root = tmp_path_factory.mktemp('evalset')
    (root / 'images').mkdir()
    (root / 'labels').mkdir()
    bus = Image.open(os.path.join(ROOT, 'tests', 'golden', 'bus.jpg')).convert('RGB')
    for i, (l, t, w, h) in enumerate(CROPS):
        bus.crop((l, t, l + w, t + h)).save(root / 'images' / f'{i:06d}.png')
    path = str(root / 'images')
    m, sd = fresh_model()
    ckpt = root / 'tiny.pt'
    torch.save({'model': sd, 'cfg': 'yolov7-tiny'}, ckpt)
    model = m.float().fuse().eval().to('cuda:0')

    # labels: the model's own detections at conf 0.25 (native pixels -> normalised xywh) and random boxes
    rng = random.Random(7)
    model.half()
    with torch.no_grad():
        for img, _, paths, shapes in make_loader(path):
            out = G.non_max_suppression(model(img)[0], 0.25, 0.45)
            for si, det in enumerate(out):
                stem = Path(paths[si]).stem
                if int(stem) == NO_LABEL_FILE:
                    continue
                (h0, w0), ratio_pad = shapes[si]
                det = det.cpu().clone()
                G.scale_coords(img.shape[2:], det[:, :4], (h0, w0), ratio_pad)
                rows = [(int(c), (x1 + x2) / 2 / w0, (y1 + y2) / 2 / h0, (x2 - x1) / w0, (y2 - y1) / h0)
                        for x1, y1, x2, y2, _, c in det[:8].tolist() if x2 > x1 and y2 > y1]
                rows += [(rng.randrange(80), rng.uniform(.2, .8), rng.uniform(.2, .8), rng.uniform(.05, .3),
                          rng.uniform(.05, .3)) for _ in range(3)]
                rng.shuffle(rows)
                (root / 'labels' / f'{stem}.txt').write_text(''.join('%d %.6f %.6f %.6f %.6f\n' % r for r in rows))
    model.float()

    data = {'nc': 80, 'val': path, 'names': [str(i) for i in range(80)]}
    yaml_path = root / 'bus.yaml'
    yaml_path.write_text(f'nc: 80\nval: {path}\nnames: {[str(i) for i in range(80)]}\n')
    w = dict(root=root, path=path, ckpt=str(ckpt), model=model, data=data, yaml=str(yaml_path), T=load_test_entry())
    w['ref'] = reference_chain(model, path)
    return w


def reference_chain(model, path):
    """test.py:105-227 image by image on the CPU (after the package's forward and NMS lists)."""
    iouv = metrics_ref.IOUV
    stats, seen, per_image = [], 0, {}
    model.half()
    with torch.no_grad():
        for img, targets, paths, shapes in make_loader(path):
            nb, _, height, width = img.shape
            out = G.non_max_suppression(model(img)[0], conf_thres=CONF, iou_thres=IOU, multi_label=True)
            targets = targets.clone()
            targets[:, 2:] *= torch.Tensor([width, height, width, height])
            for si, pred in enumerate(out):
                pred = pred.cpu()
                labels = targets[targets[:, 0] == si, 1:]
                nl = len(labels)
                tcls = labels[:, 0].tolist() if nl else []
                seen += 1
                if len(pred) == 0:
                    if nl:
                        stats.append((torch.zeros(0, len(iouv), dtype=torch.bool), torch.Tensor(), torch.Tensor(), tcls))
                    continue
                predn = pred.clone()
                G.scale_coords(img[si].shape[1:], predn[:, :4], shapes[si][0], shapes[si][1])
                per_image[paths[si]] = (pred, predn, shapes[si])
                correct = torch.zeros(pred.shape[0], len(iouv), dtype=torch.bool)
                if nl:
                    tbox = G.xywh2xyxy(labels[:, 1:5])
                    G.scale_coords(img[si].shape[1:], tbox, shapes[si][0], shapes[si][1])
                    correct = metrics_ref.match_image(predn, torch.cat((labels[:, 0:1], tbox), 1), iouv)
                stats.append((correct, pred[:, 4], pred[:, 5], tcls))
    model.float()
    stats = [np.concatenate(x, 0) for x in zip(*stats)]
    assert stats[0].any() and not stats[0].all(), 'the fixture must produce matches and misses'
    p, r, ap, f1, ap_class = metrics_ref.ap_per_class(*stats)
    ap50, apm = ap[:, 0], ap.mean(1)
    maps = np.zeros(80) + apm.mean()
    for i, c in enumerate(ap_class):
        maps[c] = apm[i]
    return dict(result=(p.mean(), r.mean(), ap50.mean(), apm.mean(), 0.0, 0.0, 0.0), maps=maps, stats=stats, seen=seen,
                per_image=per_image, nt=len(stats[3]))


def run(w, *args, **kw):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = w['T'].test(*args, batch_size=BATCH, imgsz=IMGSZ, conf_thres=CONF, iou_thres=IOU, **kw)
    return res, buf.getvalue()


def assert_equals_reference(w, res, text):
    ref = w['ref']
    (mp, mr, map50, map_, *loss), maps, t = res
    assert (mp, mr, map50, map_) == ref['result'][:4], ((mp, mr, map50, map_), ref['result'][:4])
    assert loss == [0.0, 0.0, 0.0]
    assert np.array_equal(maps, ref['maps'])
    assert t[3:] == (IMGSZ, IMGSZ, BATCH) and all(v > 0 for v in t[:3])
    line = [ln for ln in text.splitlines() if ln.split()[:1] == ['all']][0].split()
    assert int(line[1]) == ref['seen'] == 10 and int(line[2]) == ref['nt']


def test_model_and_weights_entries_equal_the_per_image_chain(world, tmp_path):
    w = world
    res_m, text_m = run(w, w['data'], model=w['model'], dataloader=make_loader(w['path']))
    assert_equals_reference(w, res_m, text_m)
    w['T'].opt.project, w['T'].opt.name = str(tmp_path), 'exp'
    res_w, text_w = run(w, w['yaml'], weights=w['ckpt'])
    assert_equals_reference(w, res_w, text_w)
    assert 'Speed:' in text_w and (tmp_path / 'exp').is_dir()
    assert res_w[0] == res_m[0] and np.array_equal(res_w[1], res_m[1])


def test_statistics_are_the_reference_stats_list(world, monkeypatch):
    """tp, conf, pred_cls and target_cls reach ap_per_class exactly as the per-image chain concatenates them."""
    w, got = world, {}
    real = w['T'].ap_per_class

    def spy(tp, conf, pred_cls, target_cls, **kw):
        got.update(tp=tp, conf=conf, pred_cls=pred_cls, target_cls=target_cls)
        return real(tp, conf, pred_cls, target_cls, **kw)
    monkeypatch.setattr(w['T'], 'ap_per_class', spy)
    run(w, w['data'], model=w['model'], dataloader=make_loader(w['path']))
    for k, want in zip(('tp', 'conf', 'pred_cls', 'target_cls'), w['ref']['stats']):
        assert got[k].dtype == want.dtype and np.array_equal(got[k], want), k


def test_save_txt_and_save_json(world, tmp_path):
    w = world
    run(w, w['data'], model=w['model'], dataloader=make_loader(w['path']), save_dir=tmp_path, save_txt=True,
        save_conf=True, save_json=True)
    jwant = []
    for path, (pred, predn, shapes) in w['ref']['per_image'].items():
        stem = Path(path).stem
        # test.py:147-153
        gn = torch.tensor(shapes[0])[[1, 0, 1, 0]]
        want = ''
        for *xyxy, conf, cls in predn.tolist():
            xywh = (G.xyxy2xywh(torch.tensor(xyxy).view(1, 4)) / gn).view(-1).tolist()
            line = (cls, *xywh, conf)
            want += ('%g ' * len(line)).rstrip() % line + '\n'
        assert (tmp_path / 'labels' / f'{stem}.txt').read_text() == want, stem
        # and the text parses back to the native-space detections (to %g's six digits)
        back = np.array([[float(v) for v in ln.split()] for ln in want.splitlines()])
        xyxy = G.xywh2xyxy(torch.from_numpy(back[:, 1:5] * gn.numpy()))
        assert np.allclose(xyxy.numpy(), predn[:, :4].numpy(), rtol=0, atol=1e-5 * max(shapes[0]) * 2)
        # test.py:168-177
        box = G.xyxy2xywh(predn[:, :4])
        box[:, :2] -= box[:, 2:] / 2
        for p, b in zip(pred.tolist(), box.tolist()):
            jwant.append({'image_id': int(stem), 'category_id': int(p[5]), 'bbox': [round(x, 3) for x in b],
                          'score': round(p[4], 5)})
    assert len(list((tmp_path / 'labels').glob('*.txt'))) == len(w['ref']['per_image'])
    assert json.loads((tmp_path / '_predictions.json').read_text()) == jwant


class ForeignLoader:
    """What the reference's own DataLoader yields: uint8 CHW RGB letterboxed batches and targets on the host.
    With `probe`, the step that handles the second batch (enqueue it, then read the first batch's results) runs
    under torch's sync debug mode 'error', in which any implicit host-device synchronisation raises."""

    def __init__(self, path, probe=False):
        self.batches, self.probe = [], probe
        ds = make_loader(path).dataset
        own = make_loader(path)
        for k, (_, targets, paths, shapes) in enumerate(own):
            idx = range(k * BATCH, min((k + 1) * BATCH, len(ds)))
            u8 = D.letterbox_ragged([ds.frame(i) for i in idx], [ds.geometry(i)[2] for i in idx], ds.canvas(idx[0]),
                                    out_kind=D.OUT_U8_HWC)
            img = u8.cpu().flip(3).permute(0, 3, 1, 2).contiguous().pin_memory()      # BGR HWC -> RGB CHW
            self.batches.append((img, targets.pin_memory(), paths, shapes))

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


def test_foreign_uint8_dataloader_gives_the_same_result(world):
    w = world
    res, text = run(w, w['data'], model=w['model'], dataloader=ForeignLoader(w['path']))
    assert_equals_reference(w, res, text)


def test_steady_state_batch_step_has_no_host_sync(world):
    w = world
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            with pytest.raises(RuntimeError):
                torch.ones(1, device='cuda').item()     # the mode must see a real sync, or it shows nothing
        finally:
            torch.cuda.set_sync_debug_mode('default')
    except (pytest.fail.Exception, AttributeError):
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag a .item() on this ROCm build')
    res, text = run(w, w['data'], model=w['model'], dataloader=ForeignLoader(w['path'], probe=True))
    assert_equals_reference(w, res, text)
