"""The COCO bbox evaluation contract (include/yv7.h at yv7_coco_match) in plain Python and numpy,
written from the contract's text: values as the predictions JSON holds them, IoU, the per-(image, category)
greedy matching, accumulate and summarize.  Sequential and slow on purpose; the tests compare the kernel's flag
words and the package's statistics with what this file gives."""
import json

import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, 10)
REC_THRS = np.linspace(0, 1, 101)
AREA_RANGES = [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]
MAX_DETS = [1, 10, 100]
FORMAT = ' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'


def json_row(x1, y1, x2, y2, score):
    """One fp32 xyxy row as test.py writes it: xyxy2xywh in fp32, centre to corner, round(v, 3), round(s, 5)."""
    f = np.float32
    x1, y1, x2, y2 = f(x1), f(y1), f(x2), f(y2)
    w, h = x2 - x1, y2 - y1
    x, y = (x1 + x2) / f(2) - w / f(2), (y1 + y2) / f(2) - h / f(2)
    return [round(float(v), 3) for v in (x, y, w, h)], round(float(f(score)), 5)


def iou(d, g, crowd):
    """d, g: (x, y, w, h)."""
    da, ga = d[2] * d[3], g[2] * g[3]
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if w <= 0 or h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def evaluate_img(dts, gts):
    """dts: [(bbox, score)] in jdict order; gts: [(bbox, area, crowd)] in annotation order, one (image, category).
    Returns rank [len(dts)] (-1 past the first 100) and, per area range, dtm and dtIg as [T][len(dts)] lists
    (0 for unranked rows) and the number of gts the range does not ignore."""
    order = sorted(range(len(dts)), key=lambda i: -dts[i][1])[:100]   # stable
    rank = [-1] * len(dts)
    for pos, i in enumerate(order):
        rank[i] = pos
    ious = [[iou(dts[i][0], g[0], g[2]) for g in gts] for i in order]
    out = []
    for lo, hi in AREA_RANGES:
        ign = [bool(g[2]) or g[1] < lo or g[1] > hi for g in gts]
        gorder = sorted(range(len(gts)), key=lambda j: ign[j])   # stable: not ignored first
        T = len(IOU_THRS)
        dtm = [[0] * len(dts) for _ in range(T)]
        dtig = [[0] * len(dts) for _ in range(T)]
        for ti, t in enumerate(IOU_THRS):
            matched = [False] * len(gts)
            for pos, i in enumerate(order):
                best = min(t, 1 - 1e-10)
                m = -1
                for j in gorder:
                    if matched[j] and not gts[j][2]:
                        continue
                    if m > -1 and not ign[m] and ign[j]:
                        break
                    if ious[pos][j] < best:
                        continue
                    best = ious[pos][j]
                    m = j
                if m > -1:
                    dtig[ti][i] = int(ign[m])
                    dtm[ti][i] = 1
                    matched[m] = True
                else:
                    a = dts[i][0][2] * dts[i][0][3]
                    dtig[ti][i] = int(a < lo or a > hi)
        out.append((dtm, dtig, sum(not x for x in ign)))
    return rank, out


def flag_words(dtm, dtig, i):
    """The kernel's word for detection i of one area range: bit t matched, bit 10 + t ignored."""
    return sum(dtm[t][i] << t for t in range(10)) | sum(dtig[t][i] << (10 + t) for t in range(10))


def match_rows(det, count, gts, gt_off):
    """yv7_coco_match's outputs for det [B,max_det,6] fp32, count [B], gts [G,7] float64, gt_off [B+1]:
    (flags [B,max_det,4] uint32, rank [B,max_det] int32)."""
    B, max_det, _ = det.shape
    flags = np.zeros((B, max_det, 4), dtype=np.uint32)
    rank = -np.ones((B, max_det), dtype=np.int32)
    for b in range(B):
        n = int(count[b])
        rows = [json_row(*det[b, r, :5]) for r in range(n)]
        g_img = gts[gt_off[b]:gt_off[b + 1]]
        for c in sorted(set(float(v) for v in det[b, :n, 5])):
            idx = [r for r in range(n) if float(det[b, r, 5]) == c]
            g_c = [(tuple(g[1:5]), g[5], g[6] != 0) for g in g_img if g[0] == c]
            rk, per_range = evaluate_img([rows[r] for r in idx], g_c)
            for k, r in enumerate(idx):
                rank[b, r] = rk[k]
                if rk[k] >= 0:
                    for a, (dtm, dtig, _) in enumerate(per_range):
                        flags[b, r, a] = flag_words(dtm, dtig, k)
    return flags, rank


def _load(x):
    if isinstance(x, (str, bytes)) or hasattr(x, '__fspath__'):
        with open(x) as f:
            return json.load(f)
    return x


def evaluate(pred_json, anno_json, class_of_category=None, img_ids=None):
    """pred_json / anno_json: paths or the loaded objects.  class_of_category: category id -> the category_id the
    predictions use for it (identity by default).  Returns a dict: precision [T,R,K,A,M], recall [T,K,A,M],
    stats [12], lines (the printed table) and three fixture diagnostics."""
    preds, anno = _load(pred_json), _load(anno_json)
    file_ids = [im['id'] for im in anno['images']]
    known = set(file_ids)
    for p in preds:
        if p['image_id'] not in known:
            raise ValueError(f"prediction for unknown image {p['image_id']!r}")
    images = sorted(set(file_ids if img_ids is None else img_ids))
    cats = sorted(c['id'] for c in anno['categories'])
    pred_cat = (lambda c: c) if class_of_category is None else (lambda c: class_of_category[c])
    gt_of, dt_of = {}, {}
    for a in anno['annotations']:
        gt_of.setdefault((a['image_id'], a['category_id']), []).append(
            (tuple(float(v) for v in a['bbox']), float(a['area']), bool(a.get('iscrowd', 0))))
    for p in preds:
        dt_of.setdefault((p['image_id'], p['category_id']), []).append((tuple(p['bbox']), p['score']))

    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cats), len(AREA_RANGES), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    diag = dict(crowd_matches=0, ignored_by_range=0, max_gts_per_image_class=0)
    for k, cat in enumerate(cats):
        per_image = []
        for im in images:
            gts, dts = gt_of.get((im, cat), []), dt_of.get((im, pred_cat(cat)), [])
            if not gts and not dts:
                continue
            diag['max_gts_per_image_class'] = max(diag['max_gts_per_image_class'], len(gts))
            rank, per_range = evaluate_img(dts, gts)
            per_image.append((dts, rank, per_range))
            dtm, dtig, _ = per_range[0]
            if any(g[2] for g in gts):
                # a detection matched and ignored at t = 0.5 in `all` met a crowd (nothing else is ignored there)
                diag['crowd_matches'] += sum(1 for i in range(len(dts)) if dtm[0][i] and dtig[0][i])
            for a in (1, 2, 3):
                dm, di, _ = per_range[a]
                diag['ignored_by_range'] += sum(1 for i in range(len(dts)) if rank[i] >= 0 and not dm[0][i] and di[0][i])
        if not per_image:
            continue
        for a in range(A):
            npig = sum(pr[a][2] for _, _, pr in per_image)
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                scores, dtm, dtig = [], [[] for _ in range(T)], [[] for _ in range(T)]
                for dts, rank, pr in per_image:
                    keep = sorted((i for i in range(len(dts)) if 0 <= rank[i] < max_det), key=lambda i: rank[i])
                    scores += [dts[i][1] for i in keep]
                    for t in range(T):
                        dtm[t] += [pr[a][0][t][i] for i in keep]
                        dtig[t] += [pr[a][1][t][i] for i in keep]
                inds = np.argsort(-np.array(scores, dtype=np.float64), kind='mergesort')
                nd = len(inds)
                for t in range(T):
                    mt = np.array(dtm[t], dtype=bool)[inds]
                    ig = np.array(dtig[t], dtype=bool)[inds]
                    tp = np.cumsum(mt & ~ig).astype(dtype=float)
                    fp = np.cumsum(~mt & ~ig).astype(dtype=float)
                    rc = tp / npig
                    pr_ = tp / (fp + tp + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr_ = pr_.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr_[i] > pr_[i - 1]:
                            pr_[i - 1] = pr_[i]
                    q = np.zeros(R)
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side='left')):
                        if pi < nd:
                            q[ri] = pr_[pi]
                    precision[t, :, k, a, m] = q
    stats, lines = summarize(precision, recall)
    return dict(precision=precision, recall=recall, stats=stats, lines=lines, **diag)


def summarize(precision, recall):
    names = ['all', 'small', 'medium', 'large']
    stats, lines = [], []

    def one(ap, t=None, a=0, m=2):
        s = precision[:, :, :, a, m] if ap else recall[:, :, a, m]
        if t is not None:
            s = s[t:t + 1]
        s = s[s > -1]
        v = float(np.mean(s)) if len(s) else -1.0
        stats.append(v)
        lines.append(FORMAT.format('Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)',
                                   '0.50:0.95' if t is None else '{:0.2f}'.format(IOU_THRS[t]), names[a],
                                   MAX_DETS[m], v))
    one(1)
    one(1, t=0)
    one(1, t=5)
    for a in (1, 2, 3):
        one(1, a=a)
    for m in (0, 1, 2):
        one(0, m=m)
    for a in (1, 2, 3):
        one(0, a=a)
    return np.array(stats), lines
