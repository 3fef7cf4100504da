"""mAP evaluation — the "mAP@0.5 parity" half of the metric.

Mirrors the reference's test.py statistics and utils/metrics.py:
  match_predictions  test.py:181-208: per image, per class, every prediction (in the NMS output's
                     descending-confidence order) takes its best-IoU target; a target already taken by
                     an earlier prediction is not taken again; correct at 10 IoU thresholds 0.5:0.95.
                     Vectorised on the device: the first claimant of a target (lowest prediction index
                     among those with IoU > 0.5) is the one the reference's sequential loop accepts.
  ap_per_class       utils/metrics.py:18-78   (host numpy, as the reference)
  compute_ap         utils/metrics.py:81-110  (101-point interpolation, v5_metric=False sentinel)
  map_from_lists     test.py:218-227          mAP@0.5 and mAP@0.5:0.95 over a set of images
  match_batch        test.py:123,131,179-213  the matching for a whole batch in one launch (libyv7 yv7_match),
                     stream-ordered, on nms_batched's output after scale_boxes: what test.py's loop runs
  ConfusionMatrix    utils/metrics.py:113-185 the evaluation's confusion matrix: process_batches is one yv7_confusion
                     launch per batch into a matrix kept on the device, process_batch the per-image call on the host
  plot_pr_curve,     utils/metrics.py:190-227 the PR, F1, P and R curve files ap_per_class(plot=True) writes, drawn
  plot_mc_curve      on matplotlib's Agg canvas without pyplot
"""
from __future__ import annotations

import ctypes
from pathlib import Path

import numpy as np
import torch

_trapz = getattr(np, 'trapezoid', None) or np.trapz


def iou_thresholds(device=None):
    return torch.linspace(0.5, 0.95, 10, device=device)   # test.py:92


def box_iou(box1, box2):
    """utils/general.py:464-486: pairwise IoU of xyxy boxes [N,4] x [M,4] -> [N,M]."""
    def area(b):
        return (b[2] - b[0]) * (b[3] - b[1])
    a1, a2 = area(box1.T), area(box2.T)
    inter = (torch.min(box1[:, None, 2:], box2[:, 2:]) - torch.max(box1[:, None, :2], box2[:, :2])).clamp(0).prod(2)
    return inter / (a1[:, None] + a2 - inter)


def match_predictions(pred, labels, iouv=None):
    """pred [n,6] (xyxy, conf, cls) in NMS order, labels [m,5] (cls, xyxy) -> correct [n, 10] bool."""
    dev = pred.device
    iouv = iou_thresholds(dev) if iouv is None else iouv.to(dev)
    n, m = pred.shape[0], labels.shape[0]
    correct = torch.zeros(n, iouv.numel(), dtype=torch.bool, device=dev)
    if n == 0 or m == 0:
        return correct
    labels = labels.to(dev)
    iou = box_iou(pred[:, :4], labels[:, 1:5])
    iou = torch.where(pred[:, 5:6] == labels[None, :, 0], iou, torch.full_like(iou, -1.0))  # same class only
    best, tgt = iou.max(1)            # each prediction's best target (first maximum, as torch .max)
    valid = best > iouv[0]
    # the first valid claimant of every target wins (test.py:197-204 'detected' bookkeeping)
    idx = torch.arange(n, device=dev)
    first = torch.full((m,), n, dtype=torch.long, device=dev)
    first.scatter_reduce_(0, tgt[valid], idx[valid], reduce='amin')
    win = valid & (first[tgt] == idx)
    correct[win] = best[win, None] > iouv
    return correct


def _check_batch(who, det, count, targets, label_off, descs):
    """The argument checks match_batch and ConfusionMatrix.process_batches share."""
    if not det.is_cuda:
        raise RuntimeError(f'{who} runs on a ROCm device (libyv7); got a CPU tensor')
    dev = det.device
    if det.dim() != 3 or det.dtype != torch.float32 or det.shape[2] != 6 or not det.is_contiguous() \
            or len(descs) != det.shape[0]:
        raise ValueError(f'{who}: expected contiguous fp32 det [B, max_det, 6] and {det.shape[0]} descriptors')
    B = det.shape[0]
    if count.dtype != torch.int32 or count.numel() != B or count.device != dev or not count.is_contiguous():
        raise ValueError(f'{who}: count must be contiguous int32 [B] on det\'s device')
    if (targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[1] != 6 or not targets.is_contiguous()
            or targets.device != dev):
        raise ValueError(f'{who}: targets must be contiguous fp32 [L, 6] on det\'s device')
    if (label_off.dtype != torch.int32 or label_off.numel() != B + 1 or label_off.device != dev
            or not label_off.is_contiguous()):
        raise ValueError(f'{who}: label_off must be contiguous int32 [B + 1] on det\'s device')


def match_batch(det, count, targets, label_off, descs, canvas_hw, iouv=None):
    """test.py:123,131,179-213 for a batch, stream-ordered (libyv7 yv7_match): det [B,max_det,6] and count [B]
    int32 as nms_batched returns them AFTER scale_boxes (native pixels); targets [L,6] fp32 on the device, rows
    (image, cls, x, y, w, h) normalised to the canvas and sorted by image; label_off [B+1] int32 on the device,
    image b's rows being label_off[b]:label_off[b+1]; descs one scale_desc per image (for ratio_pad:
    (h0, w0, ratio[0], pad_w, pad_h)); canvas_hw the model input's (h, w).
    Returns (correct [B,max_det,niou] uint8, zero in rows >= count[b]; claimed_by [L] int32, the row that
    took each label or -1)."""
    from yv7 import _lib
    _check_batch('match_batch', det, count, targets, label_off, descs)
    B, max_det, _ = det.shape
    dev = det.device
    iouv = iou_thresholds() if iouv is None else iouv
    th = [float(v) for v in iouv.detach().float().cpu().tolist()]
    n_l, niou = targets.shape[0], len(th)
    arr = (_lib.ScaleDesc * B)(*[_lib.ScaleDesc(*d) for d in descs])
    correct = torch.empty((B, max_det, niou), dtype=torch.uint8, device=dev)
    claimed_by = torch.empty((n_l,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().yv7_match(det.data_ptr(), count.data_ptr(), B, max_det, targets.data_ptr() if n_l else None,
                                  label_off.data_ptr(), n_l, arr, int(canvas_hw[0]), int(canvas_hw[1]),
                                  (ctypes.c_float * niou)(*th), niou, correct.data_ptr(),
                                  claimed_by.data_ptr() if n_l else None, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, 'yv7_match')
    return correct, claimed_by


def compute_ap(recall, precision, v5_metric=False):
    """utils/metrics.py:81-110."""
    mrec = np.concatenate(([0.], recall, [1.0] if v5_metric else [recall[-1] + 0.01]))
    mpre = np.concatenate(([1.], precision, [0.]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    return _trapz(np.interp(x, mrec, mpre), x), mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, v5_metric=False, plot=False, save_dir='.', names=()):
    """utils/metrics.py:18-78: (p, r, ap [nc, 10], f1, classes).  With plot, PR_curve.png, F1_curve.png, P_curve.png
    and R_curve.png are written into save_dir (metrics.py:41,66-75); the return value is the same either way."""
    i = np.argsort(-conf)
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes = np.unique(target_cls)
    nc = unique_classes.shape[0]
    px, py = np.linspace(0, 1, 1000), []   # for plotting
    ap, p, r = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l = (target_cls == c).sum()
        n_p = i.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + 1e-16)
        r[ci] = np.interp(-px, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p[ci] = np.interp(-px, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j], mpre, mrec = compute_ap(recall[:, j], precision[:, j], v5_metric=v5_metric)
            if plot and j == 0:
                py.append(np.interp(px, mrec, mpre))   # precision at mAP@0.5
    f1 = 2 * p * r / (p + r + 1e-16)
    if plot:
        plot_pr_curve(px, py, ap, Path(save_dir) / 'PR_curve.png', names)
        plot_mc_curve(px, f1, Path(save_dir) / 'F1_curve.png', names, ylabel='F1')
        plot_mc_curve(px, p, Path(save_dir) / 'P_curve.png', names, ylabel='Precision')
        plot_mc_curve(px, r, Path(save_dir) / 'R_curve.png', names, ylabel='Recall')
    i = f1.mean(0).argmax()
    return p[:, i], r[:, i], ap, f1[:, i], unique_classes.astype('int32')


# Plots (utils/metrics.py:164-227).  Every figure is a matplotlib.figure.Figure on its own Agg canvas: pyplot is not
# imported, so neither the process's backend nor pyplot's list of figures changes, and nothing stays open.
def _figure(figsize):
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    fig = Figure(figsize=figsize, tight_layout=True)
    FigureCanvasAgg(fig)
    return fig, fig.add_subplot(1, 1, 1)


def _finish_curve(fig, ax, xlabel, ylabel, path):
    ax.set_xlabel(xlabel)
    ax.set_ylabel(ylabel)
    ax.set_xlim(0, 1)
    ax.set_ylim(0, 1)
    ax.legend(bbox_to_anchor=(1.04, 1), loc='upper left')
    fig.savefig(Path(path), dpi=250)


def plot_pr_curve(px, py, ap, save_dir='pr_curve.png', names=()):
    """utils/metrics.py:190-207: the precision-recall curve; names[i] labels the i-th curve as the reference does."""
    fig, ax = _figure((9, 6))
    py = np.stack(py, axis=1)
    if 0 < len(names) < 21:   # display per-class legend if < 21 classes
        for i, y in enumerate(py.T):
            ax.plot(px, y, linewidth=1, label=f'{names[i]} {ap[i, 0]:.3f}')   # plot(recall, precision)
    else:
        ax.plot(px, py, linewidth=1, color='grey')
    ax.plot(px, py.mean(1), linewidth=3, color='blue', label='all classes %.3f mAP@0.5' % ap[:, 0].mean())
    _finish_curve(fig, ax, 'Recall', 'Precision', save_dir)


def plot_mc_curve(px, py, save_dir='mc_curve.png', names=(), xlabel='Confidence', ylabel='Metric'):
    """utils/metrics.py:210-227: a metric against confidence, one line per class and their mean."""
    fig, ax = _figure((9, 6))
    if 0 < len(names) < 21:   # display per-class legend if < 21 classes
        for i, y in enumerate(py):
            ax.plot(px, y, linewidth=1, label=f'{names[i]}')   # plot(confidence, metric)
    else:
        ax.plot(px, py.T, linewidth=1, color='grey')
    y = py.mean(0)
    ax.plot(px, y, linewidth=3, color='blue', label=f'all classes {y.max():.2f} at {px[y.argmax()]:.3f}')
    _finish_curve(fig, ax, xlabel, ylabel, save_dir)


class ConfusionMatrix:
    """utils/metrics.py:113-185 with the reference's interface and cell roles (rows: the label's class for a match,
    nc for an unmatched label; columns: the prediction's class for a match, nc for an unmatched prediction).

    process_batches is the evaluation's path: one yv7_confusion launch per batch on the current stream, adding
    into an int32 matrix that stays on the device; nothing is read back.  process_batch is the reference's
    per-image call on the host, the slow and compatible path.  `.matrix` is the sum of both as float64
    [nc + 1, nc + 1]; reading it is the one synchronisation.

    Where two IoUs are equal the reference's unstable argsort defines nothing.  Here a prediction takes the first
    maximum in label order and a label takes the lowest prediction index, on both paths.  A class outside [0, nc)
    (or a NaN) drops that increment and counts it; `.matrix` then raises ValueError naming the count."""

    def __init__(self, nc, conf=0.25, iou_thres=0.45):
        if not 1 <= int(nc) <= 1024:
            raise ValueError(f'ConfusionMatrix: nc must be in 1..1024, got {nc}')
        self.nc = int(nc)   # number of classes
        self.conf = conf
        self.iou_thres = iou_thres
        self.host_matrix = np.zeros((self.nc + 1, self.nc + 1), dtype=np.int64)
        self.host_dropped = 0
        self._device = None   # int32 [(nc + 1)^2 + 1] on the evaluation's device, created on first use

    def _add(self, r, c):
        if r < 0 or c < 0:
            self.host_dropped += 1
        else:
            self.host_matrix[r, c] += 1

    def _class_index(self, values):
        """.int() of class values as matrix indices; -1 outside [0, nc) and for a NaN."""
        v = np.asarray(values, dtype=np.float32)
        ok = (v > -1) & (v < self.nc)
        return np.where(ok, np.trunc(np.where(ok, v, 0)), -1).astype(np.int64)

    def process_batch(self, detections, labels):
        """One image on the host: detections [N,6] (x1, y1, x2, y2, conf, class), labels [M,5] (class, x1, y1,
        x2, y2), in the same pixels.  utils/metrics.py:121-159, every step in fp32."""
        detections = torch.as_tensor(detections).detach().float().cpu()
        labels = torch.as_tensor(labels).detach().float().cpu()
        detections = detections[detections[:, 4] > torch.tensor(self.conf, dtype=torch.float32)]
        gt = self._class_index(labels[:, 0].numpy())
        dc = self._class_index(detections[:, 5].numpy())
        n_l, n_d = labels.shape[0], detections.shape[0]
        label_of = np.full(n_d, -1, dtype=np.int64)    # each prediction's candidate label of highest IoU
        det_of = np.full(n_l, -1, dtype=np.int64)      # the matches: each label's prediction
        if n_l and n_d:
            iou = box_iou(labels[:, 1:], detections[:, :4]).numpy()
            with np.errstate(invalid='ignore'):
                cand = np.where(iou > np.float32(self.iou_thres), iou, -np.inf)   # a NaN is no candidate
            has = (cand > -np.inf).any(0)
            label_of = np.where(has, cand.argmax(0), -1)   # argmax: the first maximum in label order
            for d in range(n_d):                            # ascending: the lowest index keeps a tie
                l = label_of[d]
                if l >= 0 and (det_of[l] < 0 or cand[l, d] > cand[l, det_of[l]]):
                    det_of[l] = d
        any_match = bool((det_of >= 0).any())
        for l in range(n_l):
            if det_of[l] >= 0:
                self._add(gt[l], dc[det_of[l]])   # a match
            else:
                self._add(self.nc, gt[l])         # an unmatched label
        if any_match:
            for d in range(n_d):
                if label_of[d] < 0 or det_of[label_of[d]] != d:
                    self._add(dc[d], self.nc)     # an unmatched prediction

    def process_batches(self, det, count, targets, label_off, descs, canvas_hw):
        """A whole batch in one yv7_confusion launch on the current stream; match_batch's arguments (det and count
        after scale_boxes, targets [L,6] normalised to the canvas and sorted by image, label_off [B+1], one
        scale_desc per image, the canvas's (h, w)).  Reads nothing back."""
        from yv7 import _lib
        _check_batch('ConfusionMatrix.process_batches', det, count, targets, label_off, descs)
        B, max_det, _ = det.shape
        dev = det.device
        if self._device is None:
            self._device = torch.zeros(((self.nc + 1) ** 2 + 1,), dtype=torch.int32, device=dev)
        elif self._device.device != dev:
            raise ValueError('ConfusionMatrix.process_batches: the matrix lives on another device')
        n_l = targets.shape[0]
        arr = (_lib.ScaleDesc * B)(*[_lib.ScaleDesc(*d) for d in descs])
        nbytes = _lib.lib().yv7_confusion_ws_bytes(B, max_det, n_l)
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().yv7_confusion(det.data_ptr(), count.data_ptr(), B, max_det,
                                          targets.data_ptr() if n_l else None, label_off.data_ptr(), n_l, arr,
                                          int(canvas_hw[0]), int(canvas_hw[1]), float(self.conf),
                                          float(self.iou_thres), self.nc, self._device.data_ptr(), ws.data_ptr(),
                                          ws.numel() * 8, torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, 'yv7_confusion')

    @property
    def matrix(self):
        """float64 [nc + 1, nc + 1]: the host's part plus the device's.  Waits for the device."""
        total, dropped = self.host_matrix.copy(), self.host_dropped
        if self._device is not None:
            dev = self._device.cpu().numpy().astype(np.int64)
            total += dev[:-1].reshape(self.nc + 1, self.nc + 1)
            dropped += int(dev[-1])
        if dropped:
            raise ValueError(f'ConfusionMatrix: {dropped} increments dropped: a class index outside [0, {self.nc})')
        return total.astype(np.float64)

    def plot(self, save_dir='', names=()):
        """confusion_matrix.png as utils/metrics.py:164-181 draws it (seaborn's heatmap restated on matplotlib):
        columns normalised by their sums + 1e-6, cells < 0.005 blank, 'Blues', annotations when nc < 30."""
        matrix = self.matrix
        array = matrix / (matrix.sum(0).reshape(1, self.nc + 1) + 1E-6)   # normalize
        array[array < 0.005] = np.nan   # don't annotate (would appear as 0.00)
        fig, ax = _figure((12, 9))
        from matplotlib import colormaps
        n = self.nc + 1
        size = 10.0 if self.nc < 50 else 8.0   # sn.set(font_scale=...) for label size
        shown = np.isfinite(array)
        vmin, vmax = (float(array[shown].min()), float(array[shown].max())) if shown.any() else (0.0, 1.0)
        cmap = colormaps['Blues']
        mesh = ax.pcolormesh(np.ma.masked_invalid(array), cmap=cmap, vmin=vmin, vmax=vmax)
        ax.set_xlim(0, n)
        ax.set_ylim(n, 0)   # row 0 on top
        ax.set_aspect('equal')
        ax.set_facecolor((1, 1, 1))
        fig.colorbar(mesh, ax=ax)
        if self.nc < 30:   # annot
            span = (vmax - vmin) or 1.0
            for r, c in zip(*np.nonzero(shown)):
                rgb = np.asarray(cmap((array[r, c] - vmin) / span)[:3])
                rgb = np.where(rgb <= 0.03928, rgb / 12.92, ((rgb + 0.055) / 1.055) ** 2.4)
                dark = rgb @ np.array([0.2126, 0.7152, 0.0722]) <= 0.408   # the cell's relative luminance
                ax.text(c + 0.5, r + 0.5, '%.2f' % array[r, c], ha='center', va='center', fontsize=8,
                        color='w' if dark else '.15')
        names = list(names)
        if (0 < len(names) < 99) and len(names) == self.nc:   # apply names to ticklabels
            ticks = np.arange(n) + 0.5
            ax.set_xticks(ticks)
            ax.set_xticklabels(names + ['background FP'], rotation=90, fontsize=size)
            ax.set_yticks(ticks)
            ax.set_yticklabels(names + ['background FN'], rotation=0, fontsize=size)
        else:
            ax.tick_params(labelsize=size)
        ax.set_xlabel('True', fontsize=size)
        ax.set_ylabel('Predicted', fontsize=size)
        fig.savefig(Path(save_dir) / 'confusion_matrix.png', dpi=250)

    def print(self):
        matrix = self.matrix
        for i in range(self.nc + 1):
            print(' '.join(map(str, matrix[i])))


def map_from_lists(preds, labels):
    """preds: per image [n,6] (xyxy, conf, cls); labels: per image [m,5] (cls, xyxy) ->
    (mAP@0.5, mAP@0.5:0.95) as test.py:218-227 computes them."""
    stats = []
    for pred, lab in zip(preds, labels):
        tcls = lab[:, 0].tolist()
        if pred.shape[0] == 0:
            if len(tcls):
                stats.append((np.zeros((0, 10), bool), np.zeros(0), np.zeros(0), tcls))
            continue
        c = match_predictions(pred.float(), lab.float())
        stats.append((c.cpu().numpy(), pred[:, 4].float().cpu().numpy(), pred[:, 5].float().cpu().numpy(), tcls))
    stats = [np.concatenate(x, 0) for x in zip(*stats)]
    if len(stats) and stats[0].any():
        _, _, ap, _, _ = ap_per_class(*stats)
        return float(ap[:, 0].mean()), float(ap.mean(1).mean())
    return 0.0, 0.0


def dets_as_labels(dets):
    """Detections [n,6] (xyxy, conf, cls) of a reference run -> labels [n,5] (cls, xyxy), the parity
    check's ground truth."""
    return torch.cat((dets[:, 5:6], dets[:, :4]), 1)
