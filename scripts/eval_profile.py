"""Measurements for the batched mAP evaluation, one process, one box:

  (a) per batch of 32, yolov7 640, synthetic weights, conf 0.001, iou 0.65: device time (event pairs) of the eval
      NMS (multi_label), scale_boxes, yv7_match and yv7_confusion (ConfusionMatrix.process_batches);
  (b) host time from the NMS output to that batch's appended statistics: the per-image way (non_max_suppression's
      list, then per image scale_coords + metrics.match_predictions + .cpu()) against the batched step
      (scale_boxes + match_batch + pinned copies + one event wait + slicing), old and new alternating;
  (c) test() images/s on an in-memory dataset of pre-decoded frames, plots=True (the confusion launch in every
      batch step) and plots=False alternating, against forward + eval NMS alone on the same batches; and the
      seconds the five plot files take after the loop (ap_per_class(plot=True) beyond plot=False, and
      ConfusionMatrix.plot with its one read of the device matrix).

    python scripts/eval_profile.py --out profiles/evaluate
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'yolo-series_amd')
sys.path[:0] = [PKG, ROOT]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def spread(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'n': len(xs)}


def load_entry():
    spec = importlib.util.spec_from_file_location('yv7_test_entry', os.path.join(PKG, 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_model(name, dev):
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    with contextlib.redirect_stdout(sys.stderr):
        m = Model(name)
        synthetic_state_dict(m, seed=0)
        m = m.float().fuse().eval().to(dev).half()
    return m


def labels_for(det, cnt, shape, per_image, gen):
    """Labels in test.py's form from a batch's own detections: the first `per_image` boxes of each image (matches
    exist) and as many random ones; rows (image, cls, x, y, w, h) normalised to the canvas, sorted by image."""
    h, w = shape
    rows = []
    for b in range(det.shape[0]):
        d = det[b, :min(int(cnt[b]), per_image)]
        xywh = torch.stack(((d[:, 0] + d[:, 2]) / 2 / w, (d[:, 1] + d[:, 3]) / 2 / h, (d[:, 2] - d[:, 0]) / w,
                            (d[:, 3] - d[:, 1]) / h), 1).clamp(0, 1)
        own = torch.cat((torch.full((len(d), 1), float(b)), d[:, 5:6], xywh), 1)
        rnd = torch.cat((torch.full((per_image, 1), float(b)),
                         torch.randint(0, 80, (per_image, 1), generator=gen).float(),
                         torch.rand(per_image, 2, generator=gen) * 0.6 + 0.2,
                         torch.rand(per_image, 2, generator=gen) * 0.25 + 0.05), 1)
        rows += [own, rnd]
    return torch.cat(rows)


def measure_ab(model, dev, a):
    from utils import general as G
    from utils import metrics as M
    from yv7.synthetic import synthetic_frames
    T = load_entry()
    B, S = a.batch, a.img
    x = synthetic_frames(B, S, S, seed=1).to(dev).half()
    iouv = M.iou_thresholds()
    with torch.no_grad():
        z = model(x)[0]
        det0, _, cnt0 = G.nms_batched(z, 0.25, 0.45)
        torch.cuda.synchronize()
        targets = labels_for(det0.cpu(), cnt0.cpu(), (S, S), 10, torch.Generator().manual_seed(2))
    t_dev = targets.to(dev)
    counts = torch.bincount(targets[:, 0].long(), minlength=B).tolist()
    descs = [(S, S, 1.0, 0.0, 0.0)] * B
    shapes = [((S, S), ((1.0, 1.0), (0.0, 0.0)))] * B

    # (a) device times
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    dev_ms = {'nms': [], 'scale_boxes': [], 'match': [], 'confusion': []}
    cm = M.ConfusionMatrix(nc=80)
    for it in range(a.warmup + a.reps):
        off = T.label_offsets(t_dev, B, counts)
        ev[0].record()
        det, _, cnt = G.nms_batched(z, a.conf, a.iou, multi_label=True)
        ev[1].record()
        G.scale_boxes(det, cnt, descs, views=False)
        ev[2].record()
        M.match_batch(det, cnt, t_dev, off, descs, (S, S), iouv)
        ev[3].record()
        cm.process_batches(det, cnt, t_dev, off, descs, (S, S))
        ev[4].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            for k, name in enumerate(dev_ms):
                dev_ms[name].append(ev[k].elapsed_time(ev[k + 1]))
    kept = cnt.tolist()

    # (b) host time from the NMS output to the batch's statistics, old and new alternating
    def old_way():
        out = G.non_max_suppression(z, a.conf, a.iou, multi_label=True)   # includes the NMS, subtracted below
        torch.cuda.synchronize()
        t = time.perf_counter()
        tg = t_dev.clone()
        tg[:, 2:] *= torch.tensor([S, S, S, S], device=dev)
        stats = []
        for si, pred in enumerate(out):
            labels = tg[tg[:, 0] == si, 1:]
            tcls = labels[:, 0].tolist()
            if len(pred) == 0:
                continue
            predn = pred.clone()
            G.scale_coords((S, S), predn[:, :4], shapes[si][0], shapes[si][1])
            tbox = G.xywh2xyxy(labels[:, 1:5])
            G.scale_coords((S, S), tbox, shapes[si][0], shapes[si][1])
            c = M.match_predictions(predn, torch.cat((labels[:, 0:1], tbox), 1), iouv)
            stats.append((c.cpu().numpy(), pred[:, 4].cpu().numpy(), pred[:, 5].cpu().numpy(), tcls))
        return time.perf_counter() - t, stats

    slot = T._Slot(B, G.MAX_DET, iouv.numel())

    def new_way():
        det, _, cnt = G.nms_batched(z, a.conf, a.iou, multi_label=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        G.scale_boxes(det, cnt, descs, views=False)
        correct, _ = M.match_batch(det, cnt, t_dev, T.label_offsets(t_dev, B, counts), descs, (S, S), iouv)
        slot.count.copy_(cnt, non_blocking=True)
        slot.det.copy_(det, non_blocking=True)
        slot.correct.copy_(correct, non_blocking=True)
        slot.event.record()
        t_enq = time.perf_counter() - t
        slot.event.synchronize()
        stats = []
        for si, n in enumerate(slot.count.tolist()):
            tcls = targets[targets[:, 0] == si, 1].tolist()
            if n == 0:
                continue
            predn = slot.det[si, :n].clone()
            stats.append((slot.correct[si, :n].numpy().astype(bool), predn[:, 4].numpy(), predn[:, 5].numpy(), tcls))
        return time.perf_counter() - t, t_enq, stats

    old_s, new_s, enq_s = [], [], []
    for it in range(a.warmup // 2 + a.reps // 2):
        to, so = old_way()
        tn, te, sn = new_way()
        if it >= a.warmup // 2:
            old_s.append(to * 1e3)
            new_s.append(tn * 1e3)
            enq_s.append(te * 1e3)
    same = all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
               for x, y in zip(so, sn)) and len(so) == len(sn)
    live = int((torch.arange(det.shape[1], device=dev)[None] < cnt[:, None]).logical_and(det[..., 4] > cm.conf).sum())
    matrix = cm.matrix
    return {'batch': B, 'img': S, 'conf': a.conf, 'iou': a.iou, 'labels': int(targets.shape[0]),
            'detections_kept': int(sum(kept)), 'device_ms': {k: spread(v) for k, v in dev_ms.items()},
            'confusion': {'conf': cm.conf, 'iou_thres': cm.iou_thres, 'live_rows_per_batch': live,
                          'increments_per_batch': float(matrix.sum()) / (a.warmup + a.reps),
                          'matched_per_batch': float(matrix[:80, :80].sum()) / (a.warmup + a.reps)},
            'host_ms_per_batch': {'per_image': spread(old_s), 'batched': spread(new_s),
                                  'batched_enqueue_only': spread(enq_s)},
            'per_image_and_batched_statistics_equal': bool(same)}


def measure_c(model, dev, a):
    from PIL import Image
    from utils import datasets as D
    from utils import general as G
    T = load_entry()
    gen = torch.Generator().manual_seed(3)
    bus = Image.open(os.path.join(ROOT, 'tests', 'golden', 'bus.jpg')).convert('RGB').resize((640, 853))
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'images'))
        os.makedirs(os.path.join(tmp, 'labels'))
        names = []
        for i in range(a.files):   # 640 x 480 crops at different offsets
            top = (i * 37) % (853 - 480)
            bus.crop((0, top, 640, top + 480)).save(os.path.join(tmp, 'images', f'{i:04d}.png'))
            lab = torch.cat((torch.randint(0, 80, (8, 1), generator=gen).float(),
                             torch.rand(8, 2, generator=gen) * 0.6 + 0.2, torch.rand(8, 2, generator=gen) * 0.25 + 0.05), 1)
            with open(os.path.join(tmp, 'labels', f'{i:04d}.txt'), 'w') as f:
                f.write(''.join('%d %.6f %.6f %.6f %.6f\n' % tuple(r) for r in lab.tolist()))
            names.append(os.path.join(tmp, 'images', f'{i:04d}.png'))
        lst = os.path.join(tmp, 'val.txt')
        with open(lst, 'w') as f:
            f.write('\n'.join(names * a.repeat) + '\n')
        loader, ds = D.create_dataloader('Test', lst, a.img, a.batch, 32, pad=0.5, rect=True, cache=True)
        for _ in loader:   # decode every frame once: the timed passes read them from memory
            pass
        torch.cuda.synchronize()
        data = {'nc': 80, 'val': tmp}

        def full(plots, **kw):
            # with a model and the default save_dir no file is written: plots=True times the loop with the
            # confusion launch in it, the plotting is timed on its own below
            with contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t = time.perf_counter()
                T.test(data, model=model, dataloader=loader, batch_size=a.batch, imgsz=a.img, conf_thres=a.conf,
                       iou_thres=a.iou, plots=plots, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
            model.half()   # test() leaves the model in fp32 like the reference
            return len(ds) / dt

        def plotting_seconds():
            """One run that writes confusion_matrix.png, timed where test() makes the call (the device matrix is
            read there); and the four curve files on seeded statistics of this set's size (its labels are random,
            so its own statistics hold no true positive and test() skips ap_per_class, as the reference does)."""
            from utils import metrics as M
            spent = {}
            real_cm = T.ConfusionMatrix

            class TimedMatrix(real_cm):
                def plot(self, *args, **kw):
                    t = time.perf_counter()
                    super().plot(*args, **kw)
                    spent['confusion_matrix_plot'] = time.perf_counter() - t
            T.ConfusionMatrix = TimedMatrix
            try:
                with tempfile.TemporaryDirectory() as out:
                    full(True, save_dir=out)
                    rng = np.random.default_rng(4)
                    n = len(ds) * G.MAX_DET
                    conf = rng.random(n).astype(np.float32)
                    stats = (rng.random((n, 10)) < conf[:, None] * np.linspace(1.0, 0.3, 10), conf,
                             rng.integers(0, 80, n).astype(np.float32),
                             rng.integers(0, 80, len(ds) * 8).astype(np.float32))
                    names = {i: str(i) for i in range(80)}
                    for key, plot in (('ap_per_class_no_plot', False), ('ap_per_class_plot', True)):
                        t = time.perf_counter()
                        M.ap_per_class(*stats, plot=plot, save_dir=out, names=names)
                        spent[key] = time.perf_counter() - t
                    spent['files'] = sorted(os.listdir(out))
            finally:
                T.ConfusionMatrix = real_cm
            return spent

        def forward_nms():
            torch.cuda.synchronize()
            t = time.perf_counter()
            with torch.no_grad():
                for img, _, _, _ in loader:
                    G.nms_batched(model(img)[0], a.conf, a.iou, multi_label=True)
            torch.cuda.synchronize()
            return len(ds) / (time.perf_counter() - t)

        def loader_only():
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in loader:
                pass
            torch.cuda.synchronize()
            return len(ds) / (time.perf_counter() - t)

        full(True), full(False), forward_nms()
        ev, ev_off, fw, lo = [], [], [], []
        for _ in range(a.passes):
            fw.append(forward_nms())
            ev.append(full(True))
            ev_off.append(full(False))
            lo.append(loader_only())
        plotting = plotting_seconds()
    return {'images': len(ds), 'frame': [480, 640], 'canvas': [int(v) for v in ds.batch_shapes[0]], 'batch': a.batch,
            'conf': a.conf, 'iou': a.iou, 'test_images_per_s': spread(ev),
            'test_plots_false_images_per_s': spread(ev_off),
            'ratio_plots_true_over_false': statistics.median(ev) / statistics.median(ev_off),
            'plotting_seconds': plotting, 'forward_nms_images_per_s': spread(fw),
            'loader_alone_images_per_s': spread(lo),
            'ratio_test_over_forward_nms': statistics.median(ev) / statistics.median(fw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='yolov7')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--img', type=int, default=640)
    ap.add_argument('--conf', type=float, default=0.001)
    ap.add_argument('--iou', type=float, default=0.65)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--files', type=int, default=64)
    ap.add_argument('--repeat', type=int, default=8)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'evaluate'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('eval_profile.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    os.makedirs(a.out, exist_ok=True)
    model = build_model(a.model, dev)
    res = {'model': a.model, 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__}
    res['batch_step'] = measure_ab(model, dev, a)
    with open(os.path.join(a.out, 'evaluate.json'), 'w') as f:   # kept if the next part fails
        json.dump(res, f, indent=1)
    res['throughput'] = measure_c(model, dev, a)
    with open(os.path.join(a.out, 'evaluate.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
