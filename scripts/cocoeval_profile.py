"""Measurements for the COCO evaluation without pycocotools, one process, one box:

  (a) per batch of 32, yolov7 640, synthetic weights, conf 0.001: device time (event pairs) of CocoEvaluator.add_batch
      (the gts' upload and the yv7_coco_match launch) beside yv7_match on the same rows, and the host time of
      CocoEvaluator.update on that batch's pinned copies;
  (b) test(save_json=True) images/s on an in-memory dataset with the annotation file at hand (the evaluator in
      every batch step) and without it (the code path of the commit before), alternating;
  (c) accumulate + summarize seconds on 5000 images' worth of such batches.

The annotation file is synthetic, of COCO-like density: per image the boxes of its first detections (matches exist)
and as many random ones, about seven gts, one in ten a crowd.

    python scripts/cocoeval_profile.py --out profiles/cocoeval
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'yolo-series_amd')
sys.path[:0] = [PKG, ROOT, os.path.join(ROOT, 'scripts')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from eval_profile import build_model, labels_for, load_entry, spread  # noqa: E402


def annotations(det, cnt, ids, own, gen):
    """{images, annotations, categories} for the batch's images: `own` boxes from each image's first detections,
    `own - 1` random ones, every tenth a crowd; category = class index (80 categories)."""
    anns = []
    for b, i in enumerate(ids):
        d = det[b, :min(int(cnt[b]), own)]
        rows = [(int(r[5]), float(r[0]), float(r[1]), float(r[2] - r[0]), float(r[3] - r[1])) for r in d.tolist()]
        for _ in range(own - 1):
            w, h = (torch.rand(2, generator=gen) * 150 + 10).tolist()
            x, y = (torch.rand(2, generator=gen) * 400).tolist()
            rows.append((int(torch.randint(0, 80, (1,), generator=gen)), x, y, w, h))
        for c, x, y, w, h in rows:
            anns.append({'id': len(anns) + 1, 'image_id': i, 'category_id': c, 'bbox': [x, y, w, h],
                         'area': w * h * 0.7, 'iscrowd': int(len(anns) % 10 == 9)})
    return {'images': [{'id': i} for i in ids], 'annotations': anns, 'categories': [{'id': c} for c in range(80)]}


def measure_batch(model, dev, a):
    from utils import cocoeval as C
    from utils import general as G
    from utils import metrics as M
    from yv7.synthetic import synthetic_frames
    T = load_entry()
    B, S = a.batch, a.img
    x = synthetic_frames(B, S, S, seed=1).to(dev).half()
    descs = [(S, S, 1.0, 0.0, 0.0)] * B
    with torch.no_grad():
        z = model(x)[0]
        det, _, cnt = G.nms_batched(z, a.conf, a.iou, multi_label=True)
        G.scale_boxes(det, cnt, descs, views=False)
        torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(2)
    n_img = a.images
    ids = list(range(n_img))
    reps_ids = [ids[k:k + B] for k in range(0, n_img - B + 1, B)]
    one = annotations(det.cpu(), cnt.cpu(), ids[:B], 4, gen)
    anno = {'images': [{'id': i} for i in ids], 'categories': one['categories'], 'annotations': []}
    for k, chunk in enumerate(reps_ids):   # the same gts under every batch's image ids
        for an in one['annotations']:
            anno['annotations'].append(dict(an, id=len(anno['annotations']) + 1, image_id=an['image_id'] + k * B))
    ev = C.CocoEvaluator(C.CocoGt(anno), False, dev)
    targets = labels_for(det.cpu(), cnt.cpu(), (S, S), 4, torch.Generator().manual_seed(3))
    t_dev = targets.to(dev)
    counts = torch.bincount(targets[:, 0].long(), minlength=B).tolist()
    iouv = M.iou_thresholds()

    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    dev_ms = {'match': [], 'coco_add_batch': []}
    for it in range(a.warmup + a.reps):
        off = T.label_offsets(t_dev, B, counts)
        e[0].record()
        M.match_batch(det, cnt, t_dev, off, descs, (S, S), iouv)
        e[1].record()
        e[2].record()
        flags, rank = ev.add_batch(det, cnt, reps_ids[0])
        e[3].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            dev_ms['match'].append(e[0].elapsed_time(e[1]))
            dev_ms['coco_add_batch'].append(e[2].elapsed_time(e[3]))
    # the launch alone: the gts already on the device (add_batch's uploads left out)
    from yv7 import _lib
    rows = [ev.gt_rows(i) for i in reps_ids[0]]
    goff = torch.from_numpy(np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)).to(dev)
    gts = torch.from_numpy(np.concatenate(rows)).to(dev)
    nbytes = _lib.lib().yv7_coco_match_ws_bytes(B, det.shape[1], len(gts))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    launch_ms = []
    for it in range(a.warmup + a.reps):
        e[0].record()
        rc = _lib.lib().yv7_coco_match(det.data_ptr(), cnt.data_ptr(), B, det.shape[1], gts.data_ptr(), goff.data_ptr(),
                                       len(gts), flags.data_ptr(), rank.data_ptr(), ws.data_ptr(), nbytes,
                                       torch.cuda.current_stream().cuda_stream)
        e[1].record()
        _lib.check(rc, 'yv7_coco_match')
        torch.cuda.synchronize()
        if it >= a.warmup:
            launch_ms.append(e[0].elapsed_time(e[1]))
    dev_ms['coco_match_launch'] = launch_ms

    det_h, cnt_h = det.cpu().numpy(), cnt.cpu().tolist()
    flags_h, rank_h = flags.cpu().numpy(), rank.cpu().numpy()
    upd = []
    for chunk in reps_ids:
        t = time.perf_counter()
        ev.update(chunk, det_h, cnt_h, flags_h, rank_h)
        upd.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter()
    ev.accumulate()
    t_acc = time.perf_counter() - t
    t = time.perf_counter()
    stats = ev.summarize(print_fn=lambda s: None)
    t_sum = time.perf_counter() - t
    return {'batch': B, 'img': S, 'conf': a.conf, 'iou': a.iou, 'detections_kept': int(sum(cnt_h)),
            'ranked_rows': int((rank_h >= 0).sum()), 'gts_per_batch': int(len(gts)),
            'device_ms': {k: spread(v) for k, v in dev_ms.items()}, 'update_host_ms_per_batch': spread(upd),
            'images_accumulated': len(reps_ids) * B, 'accumulate_s': t_acc, 'summarize_s': t_sum,
            'stats': [float(v) for v in stats]}


def measure_loop(model, dev, a):
    from PIL import Image
    from utils import datasets as D
    from utils import general as G
    T = load_entry()
    gen = torch.Generator().manual_seed(3)
    bus = Image.open(os.path.join(ROOT, 'tests', 'golden', 'bus.jpg')).convert('RGB').resize((640, 853))
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'images'))
        os.makedirs(os.path.join(tmp, 'labels'))
        anns = []
        for i in range(a.files):
            top = (i * 37) % (853 - 480)
            bus.crop((0, top, 640, top + 480)).save(os.path.join(tmp, 'images', f'{i:04d}.png'))
            lab = torch.cat((torch.randint(0, 80, (7, 1), generator=gen).float(),
                             torch.rand(7, 2, generator=gen) * 0.6 + 0.2, torch.rand(7, 2, generator=gen) * 0.25 + 0.05), 1)
            with open(os.path.join(tmp, 'labels', f'{i:04d}.txt'), 'w') as f:
                f.write(''.join('%d %.6f %.6f %.6f %.6f\n' % tuple(r) for r in lab.tolist()))
            for c, cx, cy, w, h in lab.tolist():
                anns.append({'id': len(anns) + 1, 'image_id': i, 'category_id': int(c),
                             'bbox': [(cx - w / 2) * 640, (cy - h / 2) * 480, w * 640, h * 480],
                             'area': w * 640 * h * 480, 'iscrowd': int(len(anns) % 10 == 9)})
        anno_path = os.path.join(tmp, 'instances.json')
        with open(anno_path, 'w') as f:
            json.dump({'images': [{'id': i} for i in range(a.files)], 'annotations': anns,
                       'categories': [{'id': c} for c in range(80)]}, f)
        lst = os.path.join(tmp, 'val.txt')
        with open(lst, 'w') as f:
            f.write('\n'.join(os.path.join(tmp, 'images', f'{i:04d}.png') for i in range(a.files)) + '\n')
        loader, ds = D.create_dataloader('Test', lst, a.img, a.batch, 32, pad=0.5, rect=True, cache=True)
        for _ in loader:
            pass
        torch.cuda.synchronize()
        data = {'nc': 80, 'val': tmp}

        def full(anno):
            T.opt.anno_json = anno
            out = tempfile.mkdtemp(dir=tmp)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                torch.cuda.synchronize()
                t = time.perf_counter()
                T.test(data, model=model, dataloader=loader, batch_size=a.batch, imgsz=a.img, conf_thres=a.conf,
                       iou_thres=a.iou, plots=False, save_json=True, save_dir=out)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
            model.half()
            assert ('Average Precision' in buf.getvalue()) == os.path.isfile(anno)
            return len(ds) / dt
        missing = os.path.join(tmp, 'missing.json')
        full(anno_path), full(missing)
        on, off = [], []
        for _ in range(a.passes):
            on.append(full(anno_path))
            off.append(full(missing))
    return {'images': len(ds), 'batch': a.batch, 'with_evaluator_images_per_s': spread(on),
            'without_annotation_file_images_per_s': spread(off),
            'ratio_with_over_without': statistics.median(on) / statistics.median(off)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', default='yolov7')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--img', type=int, default=640)
    ap.add_argument('--conf', type=float, default=0.001)
    ap.add_argument('--iou', type=float, default=0.65)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--images', type=int, default=4992)
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cocoeval'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('cocoeval_profile.py measures on the GPU: no device found')
    dev = torch.device('cuda:0')
    os.makedirs(a.out, exist_ok=True)
    model = build_model(a.model, dev)
    res = {'model': a.model, 'device': torch.cuda.get_device_name(0), 'torch': torch.__version__}
    res['batch_step'] = measure_batch(model, dev, a)
    with open(os.path.join(a.out, 'cocoeval.json'), 'w') as f:   # kept if the next part fails
        json.dump(res, f, indent=1)
    res['loop'] = measure_loop(model, dev, a)
    with open(os.path.join(a.out, 'cocoeval.json'), 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
