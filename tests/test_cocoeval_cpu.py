"""The COCO bbox evaluation on the host (no GPU): hand-worked answers of the contract's restatement
(tests/cocoeval_ref.py) and of utils.cocoeval's host half (update / accumulate / summarize) fed with flag words
and ranks built by the restatement, yv7_coco_match's argument checks, and the CLI flag.

Every scenario is evaluated twice, by cocoeval_ref.evaluate on the JSON rows and by CocoEvaluator on fp32 rows,
and the two must agree exactly before the hand-worked value is checked."""
import json
import random

import numpy as np
import pytest

import cocoeval_ref as R
from test_evaluate_cpu import load_test_entry
from utils import cocoeval as C
from yv7 import _lib

# precision with true positives only is tp / (tp + spacing(1)): one in all but the last bit or two
ONE = pytest.approx(1.0, abs=1e-12)


def make_anno(gts, cats=(0,), extra_images=()):
    """gts: {image: [(cat, x, y, w, h[, area[, crowd]])]} -> annotation dict (area defaults to w * h)."""
    anns = []
    for im, rows in gts.items():
        for r in rows:
            cat, x, y, w, h = r[:5]
            area = r[5] if len(r) > 5 and r[5] is not None else w * h
            anns.append({'id': len(anns) + 1, 'image_id': im, 'category_id': cat, 'bbox': [x, y, w, h],
                         'area': area, 'iscrowd': int(r[6]) if len(r) > 6 else 0})
    images = [{'id': i} for i in list(gts) + list(extra_images)]
    return {'images': images, 'annotations': anns, 'categories': [{'id': c} for c in cats]}


def make_preds(dets):
    """dets: {image: [(cls, x1, y1, x2, y2, score)]} -> the rows test.py would write."""
    out = []
    for im, rows in dets.items():
        for cls, x1, y1, x2, y2, s in rows:
            bbox, score = R.json_row(x1, y1, x2, y2, s)
            out.append({'image_id': im, 'category_id': cls, 'bbox': bbox, 'score': score})
    return out


def host_eval(anno, dets, is_coco=False):
    """utils.cocoeval's host half, with the restatement standing in for the kernel."""
    ev = C.CocoEvaluator(C.CocoGt(anno), is_coco, None)
    ids = list(dets)
    if ids:
        max_det = max(1, max(len(v) for v in dets.values()))
        det = np.zeros((len(ids), max_det, 6), dtype=np.float32)
        count = np.zeros(len(ids), dtype=np.int32)
        for b, i in enumerate(ids):
            for r, (cls, x1, y1, x2, y2, s) in enumerate(dets[i]):
                det[b, r] = (x1, y1, x2, y2, s, cls)
            count[b] = len(dets[i])
        rows = [ev.gt_rows(i) for i in ids]
        off = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
        flags, rank = R.match_rows(det, count, np.concatenate(rows), off)
        ev.update(ids, det, count, flags.view(np.int32), rank)
    ev.accumulate()
    lines = []
    stats = ev.summarize(print_fn=lines.append)
    return ev, stats, lines


def both(anno, dets, **kw):
    ref = R.evaluate(make_preds(dets), anno, **kw)
    ev, stats, lines = host_eval(anno, dets)
    assert np.array_equal(ev.precision, ref['precision']) and np.array_equal(ev.recall, ref['recall'])
    assert np.array_equal(stats, ref['stats']) and lines == ref['lines']
    return ref


def box(x, y, w, h):
    return (x, y, x + w, y + h)


def test_one_gt_one_exact_detection():
    ref = both(make_anno({1: [(0, 10, 10, 20, 20)]}), {1: [(0, *box(10, 10, 20, 20), 0.9)]})
    # area 400 is small: medium and large are empty
    assert ref['stats'].tolist() == [ONE, ONE, ONE, ONE, -1, -1, 1.0, 1.0, 1.0, 1.0, -1, -1]
    assert ref['lines'][0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000'
    assert ref['lines'][1] == ' Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 1.000'
    assert ref['lines'][6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 1.000'
    assert ref['lines'][10] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000'
    assert len(ref['lines']) == 12


def test_tp_fp_tp_gives_the_101_point_value():
    anno = make_anno({1: [(0, 10, 10, 20, 20), (0, 100, 100, 20, 20)]})
    dets = {1: [(0, *box(10, 10, 20, 20), 0.9), (0, *box(200, 200, 20, 20), 0.8), (0, *box(100, 100, 20, 20), 0.7)]}
    ref = both(anno, dets)
    # rc = .5 .5 1, pr = 1 .5 2/3 -> 1 2/3 2/3: 51 recall points at 1, 50 at 2/3
    assert ref['stats'][1] == pytest.approx((51 + 50 * 2 / 3) / 101, rel=1e-12)
    assert ref['stats'][8] == 1.0


def test_crowd_matched_twice_ignores_both_and_counts_no_fp():
    anno = make_anno({1: [(0, 10, 10, 20, 20), (0, 100, 100, 60, 60, None, 1)]})
    dets = {1: [(0, *box(100, 100, 20, 20), 0.9), (0, *box(130, 130, 20, 20), 0.8), (0, *box(10, 10, 20, 20), 0.7)]}
    ref = both(anno, dets)
    rank, per = R.evaluate_img([R.json_row(*d[1:]) for d in dets[1]],
                               [((10., 10., 20., 20.), 400., False), ((100., 100., 60., 60.), 3600., True)])
    dtm, dtig, npig = per[0]
    assert npig == 1 and [dtm[0][i] for i in range(3)] == [1, 1, 1] and [dtig[0][i] for i in range(3)] == [1, 1, 0]
    assert ref['stats'][1] == ONE and ref['crowd_matches'] == 2   # as false positives they would halve the AP


def test_unmatched_detection_outside_the_range_is_ignored_there_and_a_fp_in_all():
    anno = make_anno({1: [(0, 10, 10, 20, 20)]})
    dets = {1: [(0, *box(200, 200, 100, 100), 0.9), (0, *box(10, 10, 20, 20), 0.5)]}
    ref = both(anno, dets)
    assert ref['stats'][1] == pytest.approx(0.5, rel=1e-12)    # all: FP then TP
    assert ref['stats'][3] == ONE                              # small: the 100 x 100 box is ignored
    assert ref['ignored_by_range'] >= 1


@pytest.mark.parametrize('side,ranges', [(32, (1, 2)), (96, (2, 3))])
def test_boundary_areas_belong_to_both_neighbouring_ranges(side, ranges):
    ref = both(make_anno({1: [(0, 8, 8, side, side)]}), {1: [(0, *box(8, 8, side, side), 0.9)]})
    for a in (1, 2, 3):
        assert ref['stats'][2 + a] == (ONE if a in ranges else -1), a
        assert ref['stats'][8 + a] == (1.0 if a in ranges else -1), a


def test_iou_equal_to_the_threshold_matches():
    d, g = (0.0, 0.0, 10.0, 10.0), (0.0, 0.0, 10.0, 20.0)
    assert R.iou(d, g, False) == 0.5
    rank, per = R.evaluate_img([(d, 0.9)], [(g, 200.0, False)])
    assert [per[0][0][t][0] for t in range(10)] == [1] + [0] * 9
    ref = both(make_anno({1: [(0, *g)]}), {1: [(0, 0, 0, 10, 10, 0.9)]})
    assert ref['stats'][1] == ONE and ref['stats'][2] == 0.0


def test_equal_ious_take_the_last_gt():
    g0, g1 = (10.0, 0.0, 20.0, 10.0), (14.0, 0.0, 20.0, 10.0)
    d, e = (12.0, 0.0, 20.0, 10.0), (4.0, 0.0, 20.0, 10.0)
    assert R.iou(d, g0, False) == R.iou(d, g1, False) > 0.5
    assert R.iou(e, g0, False) > 0.5 > R.iou(e, g1, False)
    rank, per = R.evaluate_img([(d, 0.9), (e, 0.8)], [(g0, 200.0, False), (g1, 200.0, False)])
    assert per[0][0][0] == [1, 1]   # d took g1, so g0 was left for e
    ref = both(make_anno({1: [(0, *g0), (0, *g1)]}), {1: [(0, *box(*d), 0.9), (0, *box(*e), 0.8)]})
    assert ref['stats'][1] == ONE


def test_a_match_that_is_not_ignored_is_not_replaced_by_a_better_ignored_gt():
    g0, crowd, d = (0.0, 0.0, 10.0, 10.0), (0.0, 0.0, 40.0, 40.0), (0.0, 0.0, 10.0, 16.0)
    assert R.iou(d, g0, False) == 0.625 and R.iou(d, crowd, True) == 1.0
    rank, per = R.evaluate_img([(d, 0.9)], [(crowd, 1600.0, True), (g0, 100.0, False)])
    dtm, dtig, _ = per[0]
    assert [dtm[t][0] for t in range(10)] == [1] * 10
    assert [dtig[t][0] for t in range(10)] == [0, 0, 0] + [1] * 7    # past 0.625 only the crowd is left
    both(make_anno({1: [(0, *crowd, None, 1), (0, *g0)]}), {1: [(0, *box(*d), 0.9)]})


def test_the_101st_detection_of_a_class_counts_nowhere():
    anno = make_anno({1: [(0, 10, 10, 20, 20)]})
    miss = [(0, *box(200 + i, 200, 20, 20), 0.9 - i * 0.001) for i in range(100)]
    ref = both(anno, {1: miss + [(0, *box(10, 10, 20, 20), 0.5)]})
    assert ref['stats'][8] == 0.0 and ref['stats'][0] == 0.0
    ref = both(anno, {1: miss[:99] + [(0, *box(10, 10, 20, 20), 0.5)]})
    assert ref['stats'][8] == 1.0


def test_max_dets_apply_per_image():
    anno = make_anno({1: [(0, 10, 10, 20, 20)], 2: [(0, 10, 10, 20, 20)]})
    dets = {1: [(0, *box(10, 10, 20, 20), 0.5)],
            2: [(0, *box(200, 200, 20, 20), 0.9), (0, *box(10, 10, 20, 20), 0.8)]}
    ref = both(anno, dets)
    # per image the first row of each is kept: one TP of two gts; a global top-1 would keep the FP alone
    assert ref['stats'][6:9].tolist() == [0.5, 1.0, 1.0]


def test_category_with_detections_and_no_gt_stays_minus_one():
    anno = make_anno({1: [(0, 10, 10, 20, 20)]}, cats=(0, 1))
    ref = both(anno, {1: [(0, *box(10, 10, 20, 20), 0.9), (1, *box(50, 50, 20, 20), 0.8)]})
    assert (ref['precision'][:, :, 1] == -1).all() and (ref['recall'][:, 1] == -1).all()
    assert ref['stats'][0] == ONE


def test_image_with_gts_and_no_predictions_lowers_recall():
    anno = make_anno({1: [(0, 10, 10, 20, 20)], 2: [(0, 10, 10, 20, 20)]})
    ref = both(anno, {1: [(0, *box(10, 10, 20, 20), 0.9)]})
    assert ref['stats'][8] == 0.5
    ref = both(anno, {})
    assert ref['stats'][8] == 0.0 and ref['stats'][0] == 0.0


def test_img_ids_limit_the_evaluated_images():
    anno = make_anno({1: [(0, 10, 10, 20, 20)], 2: [(0, 10, 10, 20, 20)]})
    dets = {1: [(0, *box(10, 10, 20, 20), 0.9)]}
    ref = R.evaluate(make_preds(dets), anno, img_ids=[1])
    assert ref['stats'][8] == 1.0
    ev = C.CocoEvaluator(C.CocoGt(anno), False, None, img_ids=[1])
    assert ev.npig[0].tolist() == [1, 1, 0, 0]


def test_is_coco_maps_category_ids_to_class_indices():
    anno = make_anno({1: [(13, 10, 10, 20, 20)]}, cats=(1, 13))
    ev = C.CocoEvaluator(C.CocoGt(anno), True, None)
    assert ev.class_of == {1: 0, 13: 11} and ev.gt_rows(1)[0, 0] == 11.0


def test_prediction_for_an_unknown_image_raises(tmp_path):
    anno = make_anno({1: [(0, 10, 10, 20, 20)]})
    preds = make_preds({7: [(0, *box(10, 10, 20, 20), 0.9)]})
    with pytest.raises(ValueError):
        R.evaluate(preds, anno)
    ev = C.CocoEvaluator(C.CocoGt(anno), False, None)
    with pytest.raises(ValueError, match='7'):
        ev.gt_rows(7)
    (tmp_path / 'a.json').write_text(json.dumps(anno))
    (tmp_path / 'p.json').write_text(json.dumps(preds))
    with pytest.raises(ValueError, match='7'):   # before anything touches a device
        C.evaluate_json(str(tmp_path / 'a.json'), str(tmp_path / 'p.json'))


def test_rounding_identity_on_random_and_tie_values():
    rng = np.random.default_rng(0)
    v = np.concatenate(((rng.random(200000) * 2000 - 100).astype(np.float32),
                        (np.arange(1, 20001, 2) / 16).astype(np.float32)))       # odd / 16: exact ties at 1e-3
    assert ((v[-10000:].astype(np.float64) * 1000) % 1 == 0.5).all()
    assert C.round_coord(v).tolist() == [round(float(x), 3) for x in v]
    s = np.concatenate((rng.random(200000).astype(np.float32), (np.arange(1, 64, 2) / 64).astype(np.float32)))
    assert ((s[-32:].astype(np.float64) * 100000) % 1 == 0.5).all()
    assert C.round_score(s).tolist() == [round(float(x), 5) for x in s]
    assert json.loads(json.dumps(C.round_coord(v[:1000]).tolist())) == C.round_coord(v[:1000]).tolist()


def test_random_scenes_agree_between_the_restatement_and_the_host_half():
    rng = random.Random(3)
    gts, dets = {}, {}
    for im in range(1, 7):
        gts[im] = [(rng.randrange(3), rng.uniform(0, 200), rng.uniform(0, 200), rng.uniform(5, 120), rng.uniform(5, 120),
                    None, rng.random() < 0.2) for _ in range(rng.randrange(0, 9))]
        rows = []
        for g in gts[im]:
            if rng.random() < 0.7:
                j = [rng.uniform(-6, 6) for _ in range(4)]
                rows.append((g[0], g[1] + j[0], g[2] + j[1], g[1] + g[3] + j[2], g[2] + g[4] + j[3],
                             round(rng.random(), 2)))
        rows += [(rng.randrange(4), *box(rng.uniform(0, 200), rng.uniform(0, 200), rng.uniform(5, 120),
                                         rng.uniform(5, 120)), round(rng.random(), 2)) for _ in range(rng.randrange(0, 6))]
        rng.shuffle(rows)
        if rows:
            dets[im] = rows
    ref = both(make_anno(gts, cats=(0, 1, 2)), dets)
    assert 0 < ref['stats'][0] < 1


def test_coco_match_argument_errors_are_host_only():
    lib = _lib.lib()
    assert lib.yv7_coco_match_ws_bytes(0, 300, 10) == 0 and lib.yv7_coco_match_ws_bytes(1, 0, 10) == 0
    assert lib.yv7_coco_match_ws_bytes(1, 300, -1) == 0
    assert lib.yv7_coco_match_ws_bytes(2, 300, 10) > lib.yv7_coco_match_ws_bytes(2, 300, 0) > 0

    def call(B=1, max_det=300, G=0, ws_bytes=1 << 30):
        rc = lib.yv7_coco_match(None, None, B, max_det, None, None, G, None, None, None, ws_bytes, None)
        return rc, lib.yv7_last_error().decode()
    for kw, rc_want, text in (({'B': 0}, -1, 'B must be positive'), ({'max_det': 0}, -1, 'max_det must be positive'),
                              ({'G': -1}, -1, 'G must not be negative'), ({'G': 3}, -1, 'null gts with G > 0'),
                              ({'ws_bytes': 8}, -3, 'ws_bytes too small'), ({}, -1, 'null argument')):
        rc, msg = call(**kw)
        assert rc == rc_want and msg == 'yv7_coco_match: ' + text, (kw, rc, msg)


def test_cli_knows_anno_json(tmp_path):
    T = load_test_entry()
    y = tmp_path / 'd.yaml'
    y.write_text('nc: 2\nval: .\n')
    assert T.parse_opt(['--data', str(y)]).anno_json == './coco/annotations/instances_val2017.json'
    assert T.parse_opt(['--data', str(y), '--anno-json', 'x.json']).anno_json == 'x.json'
    assert T.opt.anno_json == './coco/annotations/instances_val2017.json'
