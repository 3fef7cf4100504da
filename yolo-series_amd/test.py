"""test.py — the reference's mAP evaluation (test.py:21-288) on the MI355X path, with its call sites unchanged
(test.py:58 attempt_load, :115 model(img, augment), :126 non_max_suppression's arguments) and its signature and
return value: ((mp, mr, map50, map, 0.0, 0.0, 0.0), maps, t).

The reference's loop reads every batch back and matches predictions to labels per image and per class in
Python (test.py:130-213).  Here each batch is enqueued on the stream as forward -> nms_batched(multi_label)
-> scale_boxes(ratio_pad) -> match_batch (one yv7_match launch for the whole batch) -> with `plots`,
ConfusionMatrix.process_batches (one yv7_confusion launch, adding into a matrix that stays on the device) -> copies
of count, det and correct into pinned host buffers behind an event, and the host turns a batch's buffers into
statistics, --save-txt lines and --save-json rows only after the NEXT batch has been enqueued (the last one after
the loop).  The statistics are the reference's `stats` list, so ap_per_class gives its numbers.

With `save_json` and the annotation file (`opt.anno_json` / --anno-json) at hand the reference's COCO numbers
(test.py:256-278) replace `map` and `map50`.  Where pycocotools can be imported it runs exactly as in the
reference.  Where it cannot, its bbox COCOeval is restated here (utils/cocoeval.py): each batch gains one
yv7_coco_match launch behind the matching, whose flag words travel in the same pinned slot, and the host folds them
into the 12-line summary after the loop.

With `plots` (the default; --task speed turns it off) the run directory receives the reference's
confusion_matrix.png, PR_curve.png, F1_curve.png, P_curve.png and R_curve.png after the loop; the confusion matrix
is read from the device once, there.  One deliberate deviation: called with a `model` and `save_dir` left at its
default, test() writes no files (the reference would drop the five PNGs into the working directory); the matrix
is still accumulated.

With `plots` the first three batches also give the reference's test_batch{0,1,2}_labels.jpg and _pred.jpg
(test.py:215-220): plot_images builds both picture grids on the stream (one yv7_mosaic call each, from the batch,
the label rows and nms_batched's det / count before scale_boxes rewrites them), they travel in pinned buffers
behind the slot's event, and the host only encodes the JPEGs when it consumes the batch.  The pictures follow the
contract in include/yv7.h, not cv2's rendering.

Not here: W&B logging (`wandb_logger`, `trace` are accepted and ignored), `save_hybrid` and `compute_loss`
(NotImplementedError), --task study, dataset download, COCO segmentation and keypoint evaluation (the restated
COCOeval is the bbox one).  Without checkpoints at hand `--cfg NAME --synthetic-seed S` builds seeded synthetic
weights like detect.py.  There is no CPU path.

    python test.py --data data.yaml --cfg yolov7-tiny --img-size 640 --batch-size 32
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.experimental import attempt_load  # noqa: E402
from utils.datasets import FRAME_MODES, ValLoader, create_dataloader, entry_channels  # noqa: E402
from utils.general import (check_dataset, check_file, check_img_size, coco80_to_coco91_class,  # noqa: E402
                           increment_path, nms_batched, scale_boxes, xyxy2xywh)
from utils.metrics import ConfusionMatrix, ap_per_class, match_batch  # noqa: E402
from utils.plots import display_copy, mosaic_tables, plot_images  # noqa: E402
from utils.torch_utils import select_device  # noqa: E402

# what the reference reads from its global `opt` when called directly (test.py:51, 54, 90); the CLI replaces it
opt = argparse.Namespace(device='', project='runs/test', name='exp', exist_ok=False, task='val', single_cls=False,
                         cfg=None, synthetic_seed=0, anno_json='./coco/annotations/instances_val2017.json')


# test()'s default save_dir, by identity: with a model and this very object no plot files are written
_NO_SAVE_DIR = Path('')


class _Slot:
    """Pinned host buffers for one batch in flight, and the event behind which they are valid."""

    def __init__(self, nb, max_det, niou, coco=False):
        self.count = torch.empty((nb,), dtype=torch.int32, pin_memory=True)
        self.det = torch.empty((nb, max_det, 6), dtype=torch.float32, pin_memory=True)
        self.correct = torch.empty((nb, max_det, niou), dtype=torch.uint8, pin_memory=True)
        self.flags = torch.empty((nb, max_det, 4), dtype=torch.int32, pin_memory=True) if coco else None
        self.rank = torch.empty((nb, max_det), dtype=torch.int32, pin_memory=True) if coco else None
        self.event = torch.cuda.Event()
        self.targets = self.paths = self.shapes = None
        self.mosaics = None   # (batch index, labels picture, predictions picture) in pinned memory, batches 0..2

    def fits(self, nb):
        return self.count.numel() >= nb


def label_offsets(targets, nb, counts=None):
    """int32 [nb + 1] on targets' device: image b's rows of targets are label_off[b]:label_off[b + 1].  From the
    loader's per-image counts when it gives them; else counted on the device (a comparison and a cumsum:
    torch.bincount would size its output on the host and wait for the device)."""
    dev = targets.device
    if counts is not None:
        off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
        return torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)
    per = (targets[:, 0:1] == torch.arange(nb, device=dev, dtype=targets.dtype)).sum(0, dtype=torch.int32)
    return torch.cat((torch.zeros(1, dtype=torch.int32, device=dev), per.cumsum(0, dtype=torch.int32)))


def load_model(weights, device):
    if weights:
        return attempt_load(weights, map_location=device, cfg=opt.cfg)   # load FP32 model (test.py:58)
    if not opt.cfg:
        raise ValueError('test.py: pass --weights, or --cfg NAME for seeded synthetic weights')
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    m = Model(opt.cfg)
    synthetic_state_dict(m, seed=opt.synthetic_seed)
    return attempt_load(m, map_location=device)


def test(data,
         weights=None,
         batch_size=32,
         imgsz=640,
         conf_thres=0.001,
         iou_thres=0.6,  # for NMS
         save_json=False,
         single_cls=False,
         augment=False,
         verbose=False,
         model=None,
         dataloader=None,
         save_dir=_NO_SAVE_DIR,
         save_txt=False,
         save_hybrid=False,
         save_conf=False,
         plots=True,
         wandb_logger=None,
         compute_loss=None,
         half_precision=True,
         trace=False,
         is_coco=False,
         v5_metric=False,
         frames=None):
    if save_hybrid:
        raise NotImplementedError('save_hybrid (autolabelling through NMS labels=) is not part of the MI355X path')
    if compute_loss is not None:
        raise NotImplementedError('compute_loss: training is not part of the MI355X inference path')
    training = model is not None
    write_plots = bool(plots) and not (training and save_dir is _NO_SAVE_DIR)
    if training:   # called with a model (train.py's use)
        device = next(model.parameters()).device
    else:          # called directly
        device = select_device(opt.device, batch_size=batch_size)
    if device.type == 'cpu':
        raise RuntimeError('test.py runs on a ROCm (MI355X) device via libyv7; move the model to cuda (the CPU '
                           'reference lives in oracle/ and is test-only)')
    if not training:
        save_dir = Path(increment_path(Path(opt.project) / opt.name, exist_ok=opt.exist_ok))
        (save_dir / 'labels' if save_txt else save_dir).mkdir(parents=True, exist_ok=True)
        model = load_model(weights, device)
        ch = entry_channels(model, frames)   # (the loader below is this function's own)
        gs = max(int(model.stride.max()), 32)
        imgsz = check_img_size(imgsz, s=gs)
    elif save_txt:
        (Path(save_dir) / 'labels').mkdir(parents=True, exist_ok=True)
    save_dir = Path(save_dir)

    half = bool(half_precision)   # there is no CPU path (test.py:66)
    if half:
        model.half()
    model.eval()
    dtype = next(model.parameters()).dtype
    if isinstance(data, str):
        import yaml
        is_coco = data.endswith('coco.yaml')
        with open(data) as f:
            data = yaml.load(f, Loader=yaml.SafeLoader)
    check_dataset(data)
    nc = 1 if single_cls else int(data['nc'])
    iouv = torch.linspace(0.5, 0.95, 10)   # iou vector for mAP@0.5:0.95 (test.py:78); travels by value
    niou = iouv.numel()

    if not training:
        model(torch.zeros(1, ch, imgsz, imgsz).to(device).type_as(next(model.parameters())))  # run once
        task = opt.task if opt.task in ('train', 'val', 'test') else 'val'
        dataloader = create_dataloader('Test', data[task], imgsz, batch_size, gs, opt, pad=0.5, rect=True,
                                       prefix=f'{task}: ', data_dict=data, half=half, device=device, frames=frames,
                                       channels=ch)[0]
    if v5_metric:
        print('Testing with YOLOv5 AP metric...')

    seen = 0
    confusion_matrix = ConfusionMatrix(nc=nc) if plots else None
    names = {k: v for k, v in enumerate(model.names if hasattr(model, 'names') else model.module.names)}
    plot_names = [names[k] for k in sorted(names)]
    if write_plots:
        mosaic_tables(plot_names, device)   # the pictures' atlas, names and palette: uploaded here, not in enqueue()
    coco91class = coco80_to_coco91_class()
    s = ('%20s' + '%12s' * 6) % ('Class', 'Images', 'Labels', 'P', 'R', 'mAP@.5', 'mAP@.5:.95')
    p, r, mp, mr, map50, map, ap, ap_class = 0., 0., 0., 0., 0., 0., [], []
    jdict, stats, timers = [], [], []
    slots = [None, None]

    # COCO numbers without pycocotools (test.py:256-278): annotations are read before the loop
    anno_json = getattr(opt, 'anno_json', None) or './coco/annotations/instances_val2017.json'
    evaluator = None
    if save_json and os.path.isfile(anno_json):
        try:
            import pycocotools  # noqa: F401
        except ImportError:
            from utils.cocoeval import CocoEvaluator, CocoGt
            ids = [int(Path(x).stem) for x in dataloader.dataset.img_files] if is_coco else None
            evaluator = CocoEvaluator(CocoGt(anno_json), is_coco, device, img_ids=ids)

    def image_id(path):
        stem = Path(path).stem
        return int(stem) if stem.isnumeric() else stem

    def enqueue(k, img, targets, paths, shapes, counts):
        """Batch k onto the stream; returns its slot.  Nothing here waits for the device."""
        img = img.to(device, non_blocking=True)
        img_plot = img   # the uint8 batch where the loader supplied one
        if write_plots and k < 3 and img.shape[1] != 3:
            img_plot = display_copy(img, 1)   # the picture grid is 3-channel
        if not img.is_floating_point():
            img = (img.half() if half else img.float()) / 255.0   # uint8 to fp16/32, 0 - 255 to 0.0 - 1.0
        elif img.dtype != dtype:
            img = img.to(dtype)
        nb, _, height, width = img.shape
        t_host = None if targets.is_cuda else targets
        t_dev = targets if targets.is_cuda else targets.pin_memory().to(device, non_blocking=True)
        t_dev = t_dev.float().contiguous()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        with torch.no_grad():
            ev[0].record()
            out = model(img, augment=augment)[0]   # inference output (test.py:115)
            ev[1].record()
            det, _, cnt = nms_batched(out, conf_thres=conf_thres, iou_thres=iou_thres, multi_label=True)
            ev[2].record()
        timers.append(ev)
        # ratio_pad: gain = ratio[0] and the pads as they stand (general.py:345-346)
        descs = [(int(h0), int(w0), rp[0][0], rp[1][0], rp[1][1]) for (h0, w0), rp in shapes]
        off = label_offsets(t_dev, nb, counts)
        mosaics = None
        if write_plots and k < 3:   # test.py:215-220, on the stream; det is still in canvas pixels here
            pics = (plot_images(img_plot, t_dev, paths, None, plot_names, label_off=off, normalized=True),
                    plot_images(img_plot, (det, cnt), paths, None, plot_names))
            mosaics = (k, *(torch.empty(p.shape, dtype=torch.uint8, pin_memory=True) for p in pics))
            for host, p in zip(mosaics[1:], pics):
                host.copy_(p, non_blocking=True)
        scale_boxes(det, cnt, descs, views=False)   # native-space pred (test.py:144)
        correct, _ = match_batch(det, cnt, t_dev, off, descs, (height, width), iouv)
        if plots:   # test.py:188-189 for the whole batch, behind the matching launch
            confusion_matrix.process_batches(det, cnt, t_dev, off, descs, (height, width))
        if evaluator is not None:   # COCOeval.evaluateImg for the whole batch, behind the same launches
            flags, rank = evaluator.add_batch(det, cnt, [image_id(p) for p in paths])
        slot = slots[k % 2]
        if slot is None or not slot.fits(nb) or slot.det.shape[1] != det.shape[1]:
            slot = slots[k % 2] = _Slot(max(nb, batch_size), det.shape[1], niou, coco=evaluator is not None)
        slot.count[:nb].copy_(cnt, non_blocking=True)
        slot.det[:nb].copy_(det, non_blocking=True)
        slot.correct[:nb].copy_(correct, non_blocking=True)
        if evaluator is not None:
            slot.flags[:nb].copy_(flags, non_blocking=True)
            slot.rank[:nb].copy_(rank, non_blocking=True)
        if t_host is None:
            t_host = torch.empty(t_dev.shape, dtype=torch.float32, pin_memory=True)
            t_host.copy_(t_dev, non_blocking=True)
        slot.event.record()
        slot.targets, slot.paths, slot.shapes, slot.nb = t_host, paths, shapes, nb
        slot.mosaics = mosaics
        return slot

    def consume(slot):
        """A finished batch's pinned copies -> the reference's per-image statistics and side outputs."""
        nonlocal seen
        slot.event.synchronize()
        if slot.mosaics is not None:
            from PIL import Image
            k, labels_pic, pred_pic = slot.mosaics
            Image.fromarray(labels_pic.numpy()).save(save_dir / f'test_batch{k}_labels.jpg')
            Image.fromarray(pred_pic.numpy()).save(save_dir / f'test_batch{k}_pred.jpg')
            slot.mosaics = None
        counts = slot.count[:slot.nb].tolist()
        tcol, tclass = slot.targets[:, 0], slot.targets[:, 1]
        if evaluator is not None:
            evaluator.update([image_id(p) for p in slot.paths[:slot.nb]], slot.det[:slot.nb].numpy(), counts,
                             slot.flags[:slot.nb].numpy(), slot.rank[:slot.nb].numpy())
        for si, n in enumerate(counts):
            tcls = tclass[tcol == si].tolist()
            path = Path(slot.paths[si])
            seen += 1
            if n == 0:
                if len(tcls):
                    stats.append((np.zeros((0, niou), dtype=bool), np.zeros(0, np.float32), np.zeros(0, np.float32),
                                  tcls))
                continue
            predn = slot.det[si, :n].clone()
            if save_txt:   # test.py:147-153
                gn = torch.tensor(slot.shapes[si][0])[[1, 0, 1, 0]]   # normalization gain whwh
                rows = torch.cat((predn[:, 5:6], xyxy2xywh(predn[:, :4]) / gn, predn[:, 4:5]), 1).tolist()
                with open(save_dir / 'labels' / (path.stem + '.txt'), 'a') as f:
                    for row in rows:
                        line = tuple(row) if save_conf else tuple(row[:5])
                        f.write(('%g ' * len(line)).rstrip() % line + '\n')
            if save_json:   # test.py:168-177
                box = xyxy2xywh(predn[:, :4])
                box[:, :2] -= box[:, 2:] / 2   # xy center to top-left corner
                for pr, b in zip(predn.tolist(), box.tolist()):
                    jdict.append({'image_id': image_id(path),
                                  'category_id': coco91class[int(pr[5])] if is_coco else int(pr[5]),
                                  'bbox': [round(x, 3) for x in b],
                                  'score': round(pr[4], 5)})
            stats.append((slot.correct[si, :n].numpy().astype(bool), predn[:, 4].numpy(), predn[:, 5].numpy(), tcls))

    print(s)
    own = isinstance(dataloader, ValLoader)
    pending = None
    for k, batch in enumerate(dataloader.batches() if own else dataloader):
        slot = enqueue(k, *batch, *(() if own else (None,)))
        if pending is not None:
            consume(pending)   # batch k - 1, while batch k runs
        pending = slot
    if pending is not None:
        consume(pending)

    # Compute statistics (test.py:223-230)
    stats = [np.concatenate(x, 0) for x in zip(*stats)]
    if len(stats) and stats[0].any():
        p, r, ap, f1, ap_class = ap_per_class(*stats, plot=write_plots, v5_metric=v5_metric, save_dir=save_dir,
                                              names=names)
        ap50, ap = ap[:, 0], ap.mean(1)   # AP@0.5, AP@0.5:0.95
        mp, mr, map50, map = p.mean(), r.mean(), ap50.mean(), ap.mean()
        nt = np.bincount(stats[3].astype(np.int64), minlength=nc)   # number of targets per class
    else:
        nt = np.zeros(1)

    pf = '%20s' + '%12i' * 2 + '%12.3g' * 4
    print(pf % ('all', seen, nt.sum(), mp, mr, map50, map))
    if (verbose or (nc < 50 and not training)) and nc > 1 and len(stats):
        for i, c in enumerate(ap_class):
            print(pf % (names[c], seen, nt[c], p[i], r[i], ap50[i], ap[i]))

    # Speeds from the event pairs, read now that everything has finished (the reference: time_synchronized())
    torch.cuda.synchronize(device)
    t0 = sum(e[0].elapsed_time(e[1]) for e in timers)   # ms
    t1 = sum(e[1].elapsed_time(e[2]) for e in timers)
    t = tuple(x / max(seen, 1) for x in (t0, t1, t0 + t1)) + (imgsz, imgsz, batch_size)
    if not training:
        print('Speed: %.1f/%.1f/%.1f ms inference/NMS/total per %gx%g image at batch-size %g' % t)

    if write_plots:   # test.py:247-248; the one read of the device matrix
        confusion_matrix.plot(save_dir=save_dir, names=list(names.values()))

    if save_json and len(jdict):   # test.py:256-278
        w = Path(weights[0] if isinstance(weights, list) else weights).stem if weights is not None else ''
        pred_json = str(save_dir / f'{w}_predictions.json')
        print('\nEvaluating pycocotools mAP... saving %s...' % pred_json)
        with open(pred_json, 'w') as f:
            json.dump(jdict, f)
        if evaluator is not None:   # pycocotools cannot be imported: its bbox COCOeval, restated
            evaluator.accumulate()
            map, map50 = evaluator.summarize()[:2]   # update results (mAP@0.5:0.95, mAP@0.5)
        else:
            try:
                from pycocotools.coco import COCO
                from pycocotools.cocoeval import COCOeval
                anno = COCO(anno_json)
                pred = anno.loadRes(pred_json)
                ev = COCOeval(anno, pred, 'bbox')
                if is_coco:
                    ev.params.imgIds = [int(Path(x).stem) for x in dataloader.dataset.img_files]
                ev.evaluate()
                ev.accumulate()
                ev.summarize()
                map, map50 = ev.stats[:2]   # update results (mAP@0.5:0.95, mAP@0.5)
            except Exception as e:
                print(f'pycocotools unable to run: {e}')

    model.float()   # for training
    if not training:
        note = f"\n{len(list(save_dir.glob('labels/*.txt')))} labels saved to {save_dir / 'labels'}" if save_txt else ''
        print(f'Results saved to {save_dir}{note}')
    maps = np.zeros(nc) + map
    for i, c in enumerate(ap_class):
        maps[c] = ap[i]
    return (mp, mr, map50, map, 0.0, 0.0, 0.0), maps, t


def parse_opt(argv=None):
    parser = argparse.ArgumentParser(prog='test.py')
    parser.add_argument('--weights', nargs='+', type=str, default=None, help='model.pt path(s)')
    parser.add_argument('--cfg', type=str, default=None, help='architecture for state_dict checkpoints or '
                        'synthetic weights')
    parser.add_argument('--synthetic-seed', type=int, default=0, help='seeded synthetic weights when --weights is absent')
    parser.add_argument('--data', type=str, default='data/coco.yaml', help='*.data path')
    parser.add_argument('--batch-size', type=int, default=32, help='size of each image batch')
    parser.add_argument('--img-size', type=int, default=640, help='inference size (pixels)')
    parser.add_argument('--conf-thres', type=float, default=0.001, help='object confidence threshold')
    parser.add_argument('--iou-thres', type=float, default=0.65, help='IOU threshold for NMS')
    parser.add_argument('--task', default='val', help='val, test or speed')
    parser.add_argument('--device', default='', help='cuda device, i.e. 0 or 0,1,2,3')
    parser.add_argument('--single-cls', action='store_true', help='treat as single-class dataset')
    parser.add_argument('--augment', action='store_true', help='augmented inference')
    parser.add_argument('--verbose', action='store_true', help='report mAP by class')
    parser.add_argument('--save-txt', action='store_true', help='save results to *.txt')
    parser.add_argument('--save-hybrid', action='store_true', help='unsupported: label+prediction hybrid results')
    parser.add_argument('--save-conf', action='store_true', help='save confidences in --save-txt labels')
    parser.add_argument('--save-json', action='store_true', help='save a cocoapi-compatible JSON results file and, '
                        'with the annotation file at hand, report the COCO bbox mAP (pycocotools if importable, '
                        'else the built-in restatement on the device)')
    parser.add_argument('--anno-json', type=str, default='./coco/annotations/instances_val2017.json',
                        help='COCO annotation file for --save-json')
    parser.add_argument('--project', default='runs/test', help='save to project/name')
    parser.add_argument('--name', default='exp', help='save to project/name')
    parser.add_argument('--exist-ok', action='store_true', help='existing project/name ok, do not increment')
    parser.add_argument('--no-trace', action='store_true', help='accepted and ignored: nothing is traced here')
    parser.add_argument('--frames', choices=FRAME_MODES, default=None, help='how files become the frames of a model '
                        'of another channel count: a PIL mode, or raw for 8-bit bands / .npy arrays')
    parser.add_argument('--v5-metric', action='store_true', help='assume maximum recall as 1.0 in AP calculation')
    o = parser.parse_args(argv)
    o.save_json |= o.data.endswith('coco.yaml')
    o.data = check_file(o.data)
    return o


def main(argv=None):
    global opt
    opt = parse_opt(argv)
    print(opt)
    if opt.task in ('train', 'val', 'test'):   # run normally
        return test(opt.data, opt.weights, opt.batch_size, opt.img_size, opt.conf_thres, opt.iou_thres,
                    opt.save_json, opt.single_cls, opt.augment, opt.verbose, save_txt=opt.save_txt | opt.save_hybrid,
                    save_hybrid=opt.save_hybrid, save_conf=opt.save_conf, trace=not opt.no_trace,
                    v5_metric=opt.v5_metric, frames=opt.frames)
    if opt.task == 'speed':   # speed benchmarks
        return [test(opt.data, w, opt.batch_size, opt.img_size, 0.25, 0.45, save_json=False, plots=False,
                     v5_metric=opt.v5_metric, frames=opt.frames) for w in (opt.weights or [None])]
    raise NotImplementedError(f'--task {opt.task}: only val, test and speed are part of the MI355X path')


if __name__ == '__main__':
    main()
