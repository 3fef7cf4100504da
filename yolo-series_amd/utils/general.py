"""Post-processing API — mirror of the reference's utils/general.py subset on the inference path.

non_max_suppression keeps the reference signature and return type (utils/general.py:628-720) but
runs the whole batch as HIP kernels (libyv7 yv7_nms: candidate filter, conf product, argmax or
multi-label expansion, class filter, class-offset boxes, stable score sort, greedy IoU
suppression, max_det) in one stream-ordered call; the only host sync is reading the per-image
counts to build the returned list, exactly where the reference's semantics need it.
The small box helpers below are plain tensor math on the caller's device; check_dataset, check_file,
increment_path and coco80_to_coco91_class are test.py's host-side helpers.
"""
from __future__ import annotations

import glob
import math
import re
from pathlib import Path

import torch

from yv7 import _lib

MAX_WH = 4096      # general.py:640
MAX_DET = 300      # general.py:641
MAX_NMS = 30000    # general.py:642


def make_divisible(x, divisor):  # general.py:177-179
    return math.ceil(x / divisor) * divisor


def check_img_size(img_size, s=32):  # general.py:124-129
    new_size = make_divisible(img_size, int(s))
    if new_size != img_size:
        print('WARNING: --img-size %g must be multiple of max stride %g, updating to %g' % (img_size, s, new_size))
    return new_size


def check_three_channels(model):
    """For the entry points that load images themselves (autoShape, detect.py, test.py's loader), which produce
    3-channel frames as the reference's loaders do: a model built with another channel count (Model(cfg, ch=C),
    a single model or an Ensemble) is refused here, before any forward."""
    for m in (model if isinstance(model, torch.nn.ModuleList) else [model]):
        if getattr(m, 'yaml', {}).get('ch', 3) != 3:
            raise RuntimeError('this entry point loads 3-channel images; call the model on a [B,C,H,W] tensor')


def input_channels(model):
    """The input channel count of a model, or the one all members of an Ensemble share."""
    chs = {getattr(m, 'yaml', {}).get('ch', 3) for m in (model if isinstance(model, torch.nn.ModuleList) else [model])}
    if len(chs) != 1:
        raise ValueError(f'the ensemble mixes input channel counts {sorted(chs)}')
    return chs.pop()


def check_file(file):  # general.py:146-154
    if file == '' or Path(file).is_file():
        return file
    found = glob.glob('./**/' + file, recursive=True)
    assert len(found), f'File Not Found: {file}'
    assert len(found) == 1, f"Multiple files match '{file}', specify exact path: {found}"
    return found[0]


def check_dataset(data):  # general.py:157-174, local paths only: a missing dataset is an error, never a download
    val = data.get('val')
    if val and len(val):
        missing = [str(p) for p in (Path(x).resolve() for x in (val if isinstance(val, list) else [val]))
                   if not p.exists()]
        if missing:
            raise Exception(f'Dataset not found, nonexistent paths: {missing} (this package does not download)')


def increment_path(path, exist_ok=True, sep=''):  # general.py:902-912: runs/exp -> runs/exp2, runs/exp3, ...
    path = Path(path)
    if not path.exists() or exist_ok:
        return str(path)
    taken = [re.search(rf'{re.escape(path.stem)}{sep}(\d+)', d) for d in glob.glob(f'{path}{sep}*')]
    taken = [int(m.group(1)) for m in taken if m]
    return f'{path}{sep}{max(taken) + 1 if taken else 2}'


def coco80_to_coco91_class():  # general.py:244-253: the 80 contiguous class indices as COCO's paper ids
    return [i for i in range(1, 91) if i not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)]


def xyxy2xywh(x):  # general.py:256-263
    y = x.clone()
    y[:, 0] = (x[:, 0] + x[:, 2]) / 2
    y[:, 1] = (x[:, 1] + x[:, 3]) / 2
    y[:, 2] = x[:, 2] - x[:, 0]
    y[:, 3] = x[:, 3] - x[:, 1]
    return y


def xywh2xyxy(x):  # general.py:275-282
    y = x.clone()
    y[:, 0] = x[:, 0] - x[:, 2] / 2
    y[:, 1] = x[:, 1] - x[:, 3] / 2
    y[:, 2] = x[:, 0] + x[:, 2] / 2
    y[:, 3] = x[:, 1] + x[:, 3] / 2
    return y


def clip_coords(boxes, img_shape):  # general.py:356-361
    boxes[:, 0].clamp_(0, img_shape[1])
    boxes[:, 1].clamp_(0, img_shape[0])
    boxes[:, 2].clamp_(0, img_shape[1])
    boxes[:, 3].clamp_(0, img_shape[0])


def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None):  # general.py:340-353
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad = (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    else:
        gain = ratio_pad[0][0]
        pad = ratio_pad[1]
    coords[:, [0, 2]] -= pad[0]
    coords[:, [1, 3]] -= pad[1]
    coords[:, :4] /= gain
    clip_coords(coords, img0_shape)
    return coords


def scale_desc(img1_shape, img0_shape):
    """The scalars of scale_coords(img1_shape, ., img0_shape) (general.py:342-343) as yv7_scale_desc
    values (h0, w0, gain, pad_w, pad_h): Python floats here, narrowed to fp32 once at the C boundary."""
    h0, w0 = int(img0_shape[0]), int(img0_shape[1])
    gain = min(img1_shape[0] / h0, img1_shape[1] / w0)
    return h0, w0, gain, (img1_shape[1] - w0 * gain) / 2, (img1_shape[0] - h0 * gain) / 2


def scale_boxes(det, count, descs, round_boxes=False, views=True):
    """scale_coords + clip_coords (general.py:340-361) on nms_batched's outputs, in place and stream-ordered
    (libyv7 yv7_scale_boxes): det [B,max_det,6], count [B] int32, descs one scale_desc per image.
    round_boxes adds detect.py:183's .round().  With views, also returns Detections' (xywh, xyxyn, xywhn)
    (common.py:946-948), each [B,max_det,6] with rows beyond count[b] zero; otherwise None."""
    if not det.is_cuda:
        raise RuntimeError('scale_boxes runs on a ROCm device (libyv7); got a CPU tensor')
    B, max_det, six = det.shape
    if det.dtype != torch.float32 or six != 6 or not det.is_contiguous() or len(descs) != B:
        raise ValueError(f'scale_boxes: expected contiguous fp32 det [B, max_det, 6] and {B} descriptors')
    if count.dtype != torch.int32 or count.numel() != B:
        raise ValueError('scale_boxes: count must be int32 [B]')
    arr = (_lib.ScaleDesc * B)(*[_lib.ScaleDesc(*d) for d in descs])
    out = tuple(torch.empty_like(det) for _ in range(3)) if views else None
    ptrs = [t.data_ptr() for t in out] if views else [None] * 3
    dev = det.device
    with torch.cuda.device(dev):
        rc = _lib.lib().yv7_scale_boxes(det.data_ptr(), count.data_ptr(), B, max_det, arr, int(bool(round_boxes)),
                                        *ptrs, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, 'yv7_scale_boxes')
    return out


def box_iou(box1, box2):  # general.py:464-486
    def box_area(box):
        return (box[2] - box[0]) * (box[3] - box[1])

    area1 = box_area(box1.T)
    area2 = box_area(box2.T)
    inter = (torch.min(box1[:, None, 2:], box2[:, 2:]) - torch.max(box1[:, None, :2], box2[:, :2])).clamp(0).prod(2)
    return inter / (area1[:, None] + area2 - inter)


class _NmsWorkspace:
    """Device scratch for yv7_nms, grown on demand and reused across calls — one buffer per (device,
    stream): calls on one stream are ordered, calls on different streams (several batches in flight)
    may run concurrently and must not share scratch."""

    def __init__(self):
        self.buf = {}

    def get(self, device, nbytes, stream=0):
        key = (device, stream)
        t = self.buf.get(key)
        if t is None or t.numel() < nbytes:
            t = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
            self.buf[key] = t
        return t


_WS = _NmsWorkspace()


def nms_batched(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False,
                max_det=MAX_DET, max_nms=MAX_NMS, out=None, rowbest=None):
    """Stream-ordered batched NMS: returns device tensors (det [B,max_det,6], src_row [B,max_det], count [B]).

    rowbest: the forward's per-row score records (Plan.forward_into(..., rowbest=)); found automatically
    for a z returned by Model.forward / Plan.forward that has not been modified since."""
    if not prediction.is_cuda:
        raise RuntimeError('non_max_suppression runs on a ROCm device (libyv7); got a CPU tensor')
    if rowbest is None:
        from yv7.runtime import row_scores
        rowbest = row_scores.lookup(prediction)
    z = prediction.detach()
    if z.dtype != torch.float32:
        z = z.float()
    z = z.contiguous()
    B, N, no = z.shape
    dev = z.device
    if out is None:
        det = torch.empty((B, max_det, 6), dtype=torch.float32, device=dev)
        src = torch.empty((B, max_det), dtype=torch.int64, device=dev)
        cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    else:
        det, src, cnt = out
    cls_t = None
    ncls = 0
    if classes is not None:
        cls_t = torch.tensor(list(classes), dtype=torch.int32, device=dev)
        ncls = cls_t.numel()
    L = _lib.lib()
    multi = int(bool(multi_label))
    nbytes = L.yv7_nms_workspace_bytes(B, N, no, multi, max_nms)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _WS.get(dev, nbytes, stream)
    with torch.cuda.device(dev):
        rc = L.yv7_nms(z.data_ptr(), rowbest.data_ptr() if rowbest is not None else None, B, N, no,
                       float(conf_thres), float(iou_thres), multi, int(bool(agnostic)),
                       cls_t.data_ptr() if cls_t is not None else None, ncls, max_det, max_nms, det.data_ptr(),
                       src.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    _lib.check(rc, 'yv7_nms')
    return det, src, cnt


def non_max_suppression(prediction, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False,
                        labels=(), return_rows=False):
    """Runs NMS on inference results.  Returns a list of [n_i, 6] tensors (xyxy, conf, cls) per image;
    with return_rows=True also the anchor-row index of every kept box."""
    if labels and any(len(l) for l in labels):
        raise NotImplementedError('autolabelling (labels=...) is not part of the MI355X inference path')
    det, src, cnt = nms_batched(prediction, conf_thres, iou_thres, classes, agnostic, multi_label)
    counts = cnt.tolist()  # the one host sync: variable-length outputs
    out = [det[i, :n] for i, n in enumerate(counts)]
    if return_rows:
        return out, [src[i, :n] for i, n in enumerate(counts)]
    return out


def end2end(prediction, conf_thres=0.25, iou_thres=0.45, topk=100):
    """EfficientNMS_TRT-shaped outputs (models/experimental.py:111-156, End2End 226-241):
    (num_dets int32 [B,1], det_boxes [B,topk,4], det_scores [B,topk], det_classes int32 [B,topk])."""
    if not prediction.is_cuda:
        raise RuntimeError('end2end runs on a ROCm device (libyv7); got a CPU tensor')
    z = prediction.detach().float().contiguous()
    B, N, no = z.shape
    dev = z.device
    num = torch.empty((B, 1), dtype=torch.int32, device=dev)
    boxes = torch.empty((B, topk, 4), dtype=torch.float32, device=dev)
    scores = torch.empty((B, topk), dtype=torch.float32, device=dev)
    cls = torch.empty((B, topk), dtype=torch.int32, device=dev)
    L = _lib.lib()
    nbytes = L.yv7_end2end_workspace_bytes(B, N, no, topk)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ws = _WS.get(dev, nbytes, stream)
    with torch.cuda.device(dev):
        rc = L.yv7_end2end(z.data_ptr(), B, N, no, float(conf_thres), float(iou_thres), topk, num.data_ptr(),
                           boxes.data_ptr(), scores.data_ptr(), cls.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    _lib.check(rc, 'yv7_end2end')
    return num, boxes, scores, cls
