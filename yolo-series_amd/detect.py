"""detect.py — the reference's PyTorch inference loop (detect.py:25-230, its `else` branch: no ONNX/TRT)
on the MI355X path: attempt_load -> LoadImages (GPU letterbox) -> model(img)[0] -> non_max_suppression
-> scale_coords().round(), with the reference's call sites unchanged (detect.py:41, 144, 152, 183).

Differences, all forced by the environment: frames are decoded by PIL (cv2 is absent; decode parity
unpinned), there are no checkpoints offline so `--cfg NAME --synthetic-seed S` builds seeded synthetic
weights instead of `--weights`, and annotated images (detect.py:204-238) are opt-in: `--save-img` draws the
boxes on the device (utils/plots.py plot_boxes, one yv7_draw_boxes call per group of files) and saves them with
PIL; `--save-txt` writes the reference's label format.  There is no CPU execution path.

`--batch-size N` (N > 1) runs groups of up to N files, of whatever sizes, per forward: one ragged letterbox
launch (yv7_letterbox_ragged), one forward, one batched NMS, one box-scaling launch (yv7_scale_boxes with the
.round()); the default, 1, is the reference's loop above.

    python detect.py --cfg yolov7-tiny --source ../tests/golden/bus.jpg --img-size 640
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from models.experimental import attempt_load  # noqa: E402
from utils.datasets import (FRAME_MODES, OUT_F16_CHW, OUT_F32_CHW, LoadImages, entry_channels,  # noqa: E402
                            letterbox_geometry, letterbox_ragged, read_frame)
from utils.general import (check_img_size, nms_batched, non_max_suppression, scale_boxes, scale_coords,  # noqa: E402
                           scale_desc, xyxy2xywh)
from utils.plots import color_list, display_frames, plot_boxes  # noqa: E402
from utils.torch_utils import select_device, time_synchronized  # noqa: E402


def bgr_colors():
    """color_list() in the frames' channel order: they are BGR until they are saved."""
    return [c[::-1] for c in color_list()]


def save_images(frames, paths, save_dir, bgr=True):
    """Annotated frames on the device (BGR, or display copies in RGB order) -> save_dir / name, RGB, with PIL: one
    download for the group."""
    from PIL import Image
    flat = torch.cat([f.reshape(-1) for f in frames]).cpu().numpy()
    off = 0
    for f, path in zip(frames, paths):
        im = flat[off:off + f.numel()].reshape(tuple(f.shape))
        off += f.numel()
        Image.fromarray(im[:, :, ::-1] if bgr else im).save(save_dir / Path(path).with_suffix(
            '.png' if Path(path).suffix.lower() == '.npy' else Path(path).suffix).name)


def load_model(opt, device):
    if opt.weights:
        return attempt_load(opt.weights, map_location=device, cfg=opt.cfg)   # load FP32 model (detect.py:41)
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    m = Model(opt.cfg or 'yolov7')
    synthetic_state_dict(m, seed=opt.synthetic_seed)
    return attempt_load(m, map_location=device)


def draw(im0s, det, cnt, names, bgr, device):
    """detect.py:216-218: name + conf, thickness 1, the last row first.  BGR frames are drawn in place; frames of
    a stated mode (--frames) on their 3-channel display copies, which are in RGB order."""
    if bgr:
        return plot_boxes(im0s, det, cnt, names=names, colors=bgr_colors(), line_thickness=1, reverse=True)
    return plot_boxes(display_frames(im0s, device), det, cnt, names=names, colors=color_list(), line_thickness=1,
                      reverse=True)


def detect_batched(opt, model, dataset, imgsz, half, names, save_dir):
    """The loop of detect() over groups of up to opt.batch_size files, each group one forward."""
    device = next(model.parameters()).device
    bgr = dataset.frames in (None, 'RGB')
    results = []
    files = dataset.files
    for g0 in range(0, len(files), opt.batch_size):
        paths = files[g0:g0 + opt.batch_size]
        im0s = [read_frame(p, dataset.frames, dataset.channels) for p in paths]   # BGR / frame order, sizes differ
        geoms = [letterbox_geometry(im0.shape[:2], (imgsz, imgsz), auto=False) for im0 in im0s]   # datasets.py:196
        if opt.save_img:   # one upload: the letterbox and the drawing take the same tensors
            packed = torch.from_numpy(np.concatenate([im0.reshape(-1) for im0 in im0s])).to(device)
            sizes = [im0.size for im0 in im0s]
            im0s = [p.view(im0.shape) for p, im0 in zip(packed.split(sizes), im0s)]
        t1 = time_synchronized()
        img = letterbox_ragged(im0s, geoms, (imgsz, imgsz), swap_rb=bgr, device=device,
                               out_kind=OUT_F16_CHW if half else OUT_F32_CHW)
        with torch.no_grad():
            pred = model(img, augment=opt.augment)[0]
        t2 = time_synchronized()
        det, _, cnt = nms_batched(pred, opt.conf_thres, opt.iou_thres, classes=opt.classes, agnostic=opt.agnostic_nms)
        scale_boxes(det, cnt, [scale_desc(img.shape[2:], im0.shape) for im0 in im0s], round_boxes=True, views=False)
        counts = cnt.tolist()
        t3 = time_synchronized()
        if opt.save_img:
            save_images(draw(im0s, det, cnt, names, bgr, device), paths, save_dir, bgr)
        for i, (path, im0) in enumerate(zip(paths, im0s)):
            d, s = det[i, :counts[i]].cpu(), ''
            gn = torch.tensor(im0.shape)[[1, 0, 1, 0]]      # normalization gain whwh
            for c in d[:, -1].unique():
                n = (d[:, -1] == c).sum()
                s += f"{n} {names[int(c)]}{'s' * (n > 1)}, "
            if opt.save_txt and len(d):
                with open(save_dir / 'labels' / (Path(path).stem + '.txt'), 'a') as f:
                    for *xyxy, conf, cls in reversed(d):
                        xywh = (xyxy2xywh(torch.tensor(xyxy).view(1, 4)) / gn).view(-1).tolist()
                        line = (cls, *xywh, conf) if opt.save_conf else (cls, *xywh)
                        f.write(('%g ' * len(line)).rstrip() % line + '\n')
            if not opt.quiet:
                print(f'{s}Done. ({(1E3 * (t2 - t1) / len(paths)):.1f}ms) Inference, '
                      f'({(1E3 * (t3 - t2) / len(paths)):.1f}ms) NMS')
            results.append((path, d))
    return results


def detect(opt):
    """Returns [(path, det)] with det [n, 6] (x1, y1, x2, y2, conf, cls) in original-image pixels (CPU)."""
    device = select_device(opt.device)
    if device.type == 'cpu':
        raise RuntimeError('detect.py: the MI355X path has no CPU execution (oracle/ holds the CPU reference)')
    half = not opt.fp32                                   # detect.py:38 (half on every GPU device)
    model = load_model(opt, device)
    frames = getattr(opt, 'frames', None)
    ch = entry_channels(model, frames)
    bgr = frames in (None, 'RGB')
    stride = int(model.stride.max())
    imgsz = check_img_size(opt.img_size, s=stride)
    if half:
        model.half()
    dataset = LoadImages(opt.source, img_size=imgsz, stride=stride, frames=frames, channels=ch)
    names = model.module.names if hasattr(model, 'module') else model.names
    model(torch.zeros(1, ch, imgsz, imgsz).to(device).type_as(next(model.parameters())))  # run once
    save_dir = Path(opt.project) / opt.name
    if opt.save_txt:
        (save_dir / 'labels').mkdir(parents=True, exist_ok=True)
    if opt.save_img:
        save_dir.mkdir(parents=True, exist_ok=True)
    results = []
    t0 = time.time()
    if opt.batch_size > 1:
        results = detect_batched(opt, model, dataset, imgsz, half, names, save_dir)
        if not opt.quiet:
            print(f'Done. ({time.time() - t0:.3f}s)')
        return results
    for path, img, im0s, vid_cap, ratio, dwdh in dataset:
        img = torch.from_numpy(img).to(device)
        img = img.half() if half else img.float()          # uint8 to fp16/32
        img /= 255.0                                       # 0 - 255 to 0.0 - 1.0
        if img.ndimension() == 3:
            img = img.unsqueeze(0)
        t1 = time_synchronized()
        with torch.no_grad():
            pred = model(img, augment=opt.augment)[0]
        t2 = time_synchronized()
        pred = non_max_suppression(pred, opt.conf_thres, opt.iou_thres, classes=opt.classes, agnostic=opt.agnostic_nms)
        t3 = time_synchronized()
        for i, det in enumerate(pred):
            p, s, im0 = Path(path), '', im0s
            gn = torch.tensor(im0.shape)[[1, 0, 1, 0]]      # normalization gain whwh
            if len(det):
                det[:, :4] = scale_coords(img.shape[2:], det[:, :4], im0.shape).round()
                for c in det[:, -1].unique():
                    n = (det[:, -1] == c).sum()
                    s += f"{n} {names[int(c)]}{'s' * (n > 1)}, "
                if opt.save_txt:
                    with open(save_dir / 'labels' / (p.stem + '.txt'), 'a') as f:
                        for *xyxy, conf, cls in reversed(det.cpu()):
                            xywh = (xyxy2xywh(torch.tensor(xyxy).view(1, 4)) / gn).view(-1).tolist()
                            line = (cls, *xywh, conf) if opt.save_conf else (cls, *xywh)
                            f.write(('%g ' * len(line)).rstrip() % line + '\n')
            if opt.save_img:   # detect.py:216-218 through the batch's drawing path, a batch of one
                cnt = torch.tensor([len(det)], dtype=torch.int32, device=device)
                box = det[None].float().contiguous() if len(det) else torch.zeros((1, 1, 6), device=device)
                save_images(draw([im0], box, cnt, names, bgr, device), [path], save_dir, bgr)
            if not opt.quiet:
                print(f'{s}Done. ({(1E3 * (t2 - t1)):.1f}ms) Inference, ({(1E3 * (t3 - t2)):.1f}ms) NMS')
            results.append((path, det.cpu()))
    if not opt.quiet:
        print(f'Done. ({time.time() - t0:.3f}s)')
    return results


def parse_opt(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--weights', nargs='+', type=str, default=None, help='model.pt path(s)')
    ap.add_argument('--cfg', type=str, default=None, help='architecture (yolov7, yolov7-tiny, yolov7-w6, ...) for '
                    'state_dict checkpoints or synthetic weights')
    ap.add_argument('--synthetic-seed', type=int, default=0, help='seeded synthetic weights when --weights is absent')
    ap.add_argument('--source', type=str, default='inference/images', help='file/folder')
    ap.add_argument('--img-size', type=int, default=640, help='inference size (pixels)')
    ap.add_argument('--conf-thres', type=float, default=0.25, help='object confidence threshold')
    ap.add_argument('--iou-thres', type=float, default=0.45, help='IOU threshold for NMS')
    ap.add_argument('--device', default='', help='cuda device, i.e. 0 or 0,1,2,3')
    ap.add_argument('--save-txt', action='store_true', help='save results to *.txt')
    ap.add_argument('--save-conf', action='store_true', help='save confidences in --save-txt labels')
    ap.add_argument('--save-img', action='store_true', help='save the images with boxes and labels drawn')
    ap.add_argument('--classes', nargs='+', type=int, help='filter by class: --class 0, or --class 0 2 3')
    ap.add_argument('--agnostic-nms', action='store_true', help='class-agnostic NMS')
    ap.add_argument('--augment', action='store_true', help='augmented inference')
    ap.add_argument('--project', default='runs/detect', help='save results to project/name')
    ap.add_argument('--name', default='exp', help='save results to project/name')
    ap.add_argument('--fp32', action='store_true', help='run the fp32 plan instead of half()')
    ap.add_argument('--batch-size', type=int, default=1, help='files per forward (sizes may differ); 1 = one by one')
    ap.add_argument('--frames', choices=FRAME_MODES, default=None, help='how files become the frames of a model of '
                    'another channel count: a PIL mode, or raw for the file\'s own 8-bit bands / .npy arrays')
    ap.add_argument('--quiet', action='store_true')
    return ap.parse_args(argv)


if __name__ == '__main__':
    detect(parse_opt())
