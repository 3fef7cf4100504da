"""COCO bbox mAP without pycocotools — what test.py:256-278 gets from COCO / loadRes / COCOeval(anno, pred, 'bbox')
.evaluate() / .accumulate() / .summarize(), restated (the contract is in include/yv7.h at yv7_coco_match and in
DESIGN §4.22).

  CocoGt              the annotation file's images, annotations and categories
  CocoEvaluator       add_batch: the per-(image, category) greedy matching of a whole batch in one yv7_coco_match
                      launch on the current stream, on nms_batched's output after scale_boxes (no host read);
                      update / accumulate / summarize: COCOeval.accumulate and .summarize in numpy on the host
  evaluate_json       a saved predictions file through the same kernel, 64 images at a time

The evaluation runs on the values the predictions JSON holds: round(v, 3) of the fp32 xywh and round(s, 5) of the
fp32 score.  For an fp32 v the products v * 1000 and s * 100000 are exact in double, so rint(v * 1000) / 1000 is
Python's round(v, 3) bit for bit; the kernel and this file both use that form."""
from __future__ import annotations

import json

import numpy as np
import torch

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0.0, 1.0, 101)
AREA_RANGES = ((0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10))
AREA_NAMES = ('all', 'small', 'medium', 'large')
MAX_DETS = (1, 10, 100)
CHUNK = 64   # images per yv7_coco_match launch


def round_score(s):
    """round(float(s), 5) of fp32 scores, as float64."""
    return np.rint(np.asarray(s, dtype=np.float32).astype(np.float64) * 100000.0) / 100000.0


def round_coord(v):
    """round(float(v), 3) of fp32 coordinates, as float64."""
    return np.rint(np.asarray(v, dtype=np.float32).astype(np.float64) * 1000.0) / 1000.0


def _coco91_to_class():
    from utils.general import coco80_to_coco91_class
    return {c: i for i, c in enumerate(coco80_to_coco91_class())}


class CocoGt:
    """The annotation file: image ids, sorted category ids, and each image's annotations in file order as
    (category_id, x, y, w, h, area, iscrowd)."""

    def __init__(self, anno_json):
        if isinstance(anno_json, dict):
            d = anno_json
        else:
            with open(anno_json) as f:
                d = json.load(f)
        self.img_ids = [im['id'] for im in d['images']]
        self.cat_ids = sorted(c['id'] for c in d['categories'])
        self.anns = {i: [] for i in self.img_ids}
        for a in d['annotations']:
            x, y, w, h = a['bbox']
            row = (a['category_id'], float(x), float(y), float(w), float(h), float(a['area']),
                   1.0 if a.get('iscrowd', 0) else 0.0)
            self.anns.setdefault(a['image_id'], []).append(row)


class CocoEvaluator:
    """COCOeval(anno, pred, 'bbox') with params.imgIds = img_ids (default: the file's images)."""

    def __init__(self, gt, is_coco, device, img_ids=None):
        self.gt, self.device = gt, torch.device(device) if device is not None else None
        self.cat_ids = list(gt.cat_ids)
        to_class = _coco91_to_class() if is_coco else None
        # category id -> the class index a detection of it carries; -1: no detection can have it
        self.class_of = {c: (to_class.get(c, -1) if is_coco else c) for c in self.cat_ids}
        self.k_of_class = {v: k for k, c in enumerate(self.cat_ids) for v in [self.class_of[c]] if v != -1}
        known = set(gt.img_ids)
        self.known = known
        self.eval_ids = sorted(set(gt.img_ids if img_ids is None else img_ids))
        self.seq = {i: n for n, i in enumerate(self.eval_ids)}
        k_of_cat = {c: k for k, c in enumerate(self.cat_ids)}
        self._rows = {}
        self.npig = np.zeros((len(self.cat_ids), len(AREA_RANGES)), dtype=np.int64)
        for i, anns in gt.anns.items():
            rows = np.array([(float(self.class_of.get(a[0], -1)),) + a[1:] for a in anns],
                            dtype=np.float64).reshape(-1, 7)
            self._rows[i] = rows
            if i not in self.seq:
                continue
            for a in anns:   # gts count from the file alone, whether or not a detection ever meets them
                if a[0] in k_of_cat and not a[6]:
                    for ai, (lo, hi) in enumerate(AREA_RANGES):
                        self.npig[k_of_cat[a[0]], ai] += not (a[5] < lo or a[5] > hi)
        self._empty = np.zeros((0, 7), dtype=np.float64)
        self._acc = []
        self.precision = self.recall = self.stats = None

    def gt_rows(self, image_id):
        if image_id not in self.known:
            raise ValueError(f'prediction for image {image_id!r}, which the annotation file does not list')
        return self._rows.get(image_id, self._empty)

    def add_batch(self, det, count, image_ids):
        """det [B,max_det,6] fp32 and count [B] int32 on the device (native pixels), image_ids the B ids.
        Enqueues the gts' upload and one yv7_coco_match launch on the current stream; returns (flags
        [B,max_det,4] int32 holding the uint32 words, rank [B,max_det] int32) on the device."""
        from yv7 import _lib
        if not det.is_cuda:
            raise RuntimeError('CocoEvaluator.add_batch runs on a ROCm device (libyv7); got a CPU tensor')
        dev = det.device
        if det.dim() != 3 or det.dtype != torch.float32 or det.shape[2] != 6 or not det.is_contiguous() \
                or len(image_ids) != det.shape[0]:
            raise ValueError(f'add_batch: expected contiguous fp32 det [B, max_det, 6] and {det.shape[0]} image ids')
        B, max_det, _ = det.shape
        if count.dtype != torch.int32 or count.numel() != B or count.device != dev or not count.is_contiguous():
            raise ValueError('add_batch: count must be contiguous int32 [B] on det\'s device')
        rows = [self.gt_rows(i) for i in image_ids]
        off = np.zeros(B + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(r) for r in rows])
        G = int(off[-1])
        off_dev = torch.from_numpy(off).pin_memory().to(dev, non_blocking=True)
        gts_dev = torch.from_numpy(np.concatenate(rows)).pin_memory().to(dev, non_blocking=True) if G else None
        flags = torch.empty((B, max_det, 4), dtype=torch.int32, device=dev)
        rank = torch.empty((B, max_det), dtype=torch.int32, device=dev)
        nbytes = _lib.lib().yv7_coco_match_ws_bytes(B, max_det, G)
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().yv7_coco_match(det.data_ptr(), count.data_ptr(), B, max_det,
                                           gts_dev.data_ptr() if G else None, off_dev.data_ptr(), G,
                                           flags.data_ptr(), rank.data_ptr(), ws.data_ptr(), nbytes,
                                           torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, 'yv7_coco_match')
        return flags, rank

    def update(self, image_ids, det_host, count, flags, rank):
        """A finished batch's host copies: keeps, per evaluated image, the ranked rows' class, rounded score, rank
        and flag words."""
        det = np.asarray(det_host, dtype=np.float32)
        rank = np.asarray(rank, dtype=np.int32)
        flags = np.asarray(flags).view(np.uint32).reshape(rank.shape + (4,))
        count = np.asarray(count).reshape(-1)
        B = len(image_ids)
        seq = np.array([self.seq.get(i, -1) for i in image_ids], dtype=np.int64)
        valid = (rank[:B] >= 0) & (np.arange(rank.shape[1])[None, :] < count[:B, None]) & (seq[:, None] >= 0)
        bi, ri = np.nonzero(valid)
        if len(bi):
            self._acc.append((seq[bi], det[bi, ri, 5].astype(np.float64), round_score(det[bi, ri, 4]),
                              rank[bi, ri].astype(np.int64), flags[bi, ri]))

    def accumulate(self):
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(AREA_RANGES), len(MAX_DETS)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        if self._acc:
            seq, cls, score, rank, flags = (np.concatenate(x) for x in zip(*self._acc))
        else:
            seq = rank = np.zeros(0, np.int64)
            cls = score = np.zeros(0, np.float64)
            flags = np.zeros((0, 4), np.uint32)
        kk = np.full(len(cls), -1, dtype=np.int64)
        for c in np.unique(cls):
            if np.isfinite(c) and c == int(c):
                kk[cls == c] = self.k_of_class.get(int(c), -1)
        order = np.lexsort((rank, seq))   # image by image, each image's rows in rank order
        tbits = np.arange(T, dtype=np.uint32)[:, None]
        for k in range(K):
            if not self.npig[k].any():
                continue
            sel = order[kk[order] == k]
            sel = sel[np.argsort(-score[sel], kind='mergesort')]
            for m, max_det in enumerate(MAX_DETS):
                sm = sel[rank[sel] < max_det]
                nd = len(sm)
                for a in range(A):
                    npig = int(self.npig[k, a])
                    if npig == 0:
                        continue
                    f = flags[sm, a][None, :]
                    dtm = ((f >> tbits) & 1).astype(bool)
                    dtig = ((f >> (tbits + np.uint32(T))) & 1).astype(bool)
                    tp_sum = np.cumsum(dtm & ~dtig, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(~dtm & ~dtig, axis=1).astype(dtype=float)
                    for t in range(T):
                        tp, fp = tp_sum[t], fp_sum[t]
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = np.maximum.accumulate(pr[::-1])[::-1]   # non-increasing from the right
                        inds = np.searchsorted(rc, REC_THRS, side='left')
                        q = np.zeros(R)
                        ok = inds < nd
                        q[ok] = pr[inds[ok]]
                        precision[t, :, k, a, m] = q
        self.precision, self.recall = precision, recall
        return precision, recall

    def summarize(self, print_fn=print):
        if self.precision is None:
            self.accumulate()

        def one(ap, t=None, a=0, m=2):
            s = self.precision[:, :, :, a, m] if ap else self.recall[:, :, a, m]
            if t is not None:
                s = s[t:t + 1]
            v = float(np.mean(s[s > -1])) if (s > -1).any() else -1.0
            iou = '0.50:0.95' if t is None else '{:0.2f}'.format(IOU_THRS[t])
            print_fn(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
                'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou, AREA_NAMES[a],
                MAX_DETS[m], v))
            return v
        self.stats = np.array([one(1), one(1, t=0), one(1, t=5), one(1, a=1), one(1, a=2), one(1, a=3),
                               one(0, m=0), one(0, m=1), one(0, m=2), one(0, a=1), one(0, a=2), one(0, a=3)])
        return self.stats


def evaluate_json(anno_json, pred_json, is_coco=False, device='cuda:0'):
    """The 12 COCO bbox stats of a saved predictions file (test.py's _predictions.json rows: image_id,
    category_id, bbox xywh, score) against an annotation file, through yv7_coco_match.  The rows go to the device
    as fp32 xyxy; a file whose numbers do not come back from that form unchanged (they do for round(v, 3) of
    fp32 boxes within a few thousand pixels) is refused."""
    gt = CocoGt(anno_json)
    with open(pred_json) as f:
        preds = json.load(f)
    ev = CocoEvaluator(gt, is_coco, device)
    to_class = _coco91_to_class() if is_coco else None
    per_image = {}
    for p in preds:
        ev.gt_rows(p['image_id'])   # an unknown image raises before anything is launched
        c = to_class.get(p['category_id'], -1) if is_coco else p['category_id']
        per_image.setdefault(p['image_id'], []).append(tuple(p['bbox']) + (p['score'], c))
    ids = list(per_image)
    dev = torch.device(device)
    for i0 in range(0, len(ids), CHUNK):
        chunk = ids[i0:i0 + CHUNK]
        count = np.array([len(per_image[i]) for i in chunk], dtype=np.int32)
        det = np.zeros((len(chunk), max(int(count.max()), 1), 6), dtype=np.float32)
        for b, i in enumerate(chunk):
            r = np.array(per_image[i], dtype=np.float64).reshape(-1, 6)
            x1, y1 = r[:, 0].astype(np.float32), r[:, 1].astype(np.float32)
            x2, y2 = (r[:, 0] + r[:, 2]).astype(np.float32), (r[:, 1] + r[:, 3]).astype(np.float32)
            d = np.stack((x1, y1, x2, y2, r[:, 4].astype(np.float32), r[:, 5].astype(np.float32)), 1)
            w, h = x2 - x1, y2 - y1
            back = np.stack((round_coord((x1 + x2) / np.float32(2) - w / np.float32(2)),
                             round_coord((y1 + y2) / np.float32(2) - h / np.float32(2)),
                             round_coord(w), round_coord(h), round_score(d[:, 4]), d[:, 5].astype(np.float64)), 1)
            if not np.array_equal(back, r):
                raise ValueError(f'evaluate_json: image {i!r} has rows that fp32 xyxy boxes do not reproduce')
            det[b, :len(r)] = d
        d_det = torch.from_numpy(det).pin_memory().to(dev, non_blocking=True)
        d_cnt = torch.from_numpy(count).pin_memory().to(dev, non_blocking=True)
        with torch.cuda.device(dev):
            flags, rank = ev.add_batch(d_det, d_cnt, chunk)
        ev.update(chunk, det, count, flags.cpu().numpy(), rank.cpu().numpy())
    ev.accumulate()
    return ev.summarize()
