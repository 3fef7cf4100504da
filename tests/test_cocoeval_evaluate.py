"""test.py --save-json end to end on the GPU without pycocotools: the COCO numbers equal the contract's restatement
(tests/cocoeval_ref.py) on the _predictions.json the same run wrote.

Fixture: tests/test_evaluate.py's ten crops, model and labels, with an annotation file written from the label files
in native pixels: every third gt a crowd, a category (80) with gts and no detections, and an extra image (99) with
gts only.  The statistics are doubles computed by the same numpy operations on identical integers, so == holds."""
import contextlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import cocoeval_ref as R
from test_evaluate import (BATCH, CONF, CROPS, IMGSZ, IOU, ForeignLoader, assert_equals_reference,  # noqa: F401
                           make_loader, world)
from utils import cocoeval as C
from utils import general as G

pytestmark = pytest.mark.gpu


def write_annotations(root):
    anns = []
    for i, (_, _, w0, h0) in enumerate(CROPS):
        f = root / 'labels' / f'{i:06d}.txt'
        if not f.exists():
            continue
        for line in f.read_text().splitlines():
            c, cx, cy, w, h = line.split()
            w, h = float(w) * w0, float(h) * h0
            x, y = float(cx) * w0 - w / 2, float(cy) * h0 - h / 2
            anns.append({'id': len(anns) + 1, 'image_id': i, 'category_id': int(c), 'bbox': [x, y, w, h],
                         'area': w * h, 'iscrowd': int(len(anns) % 3 == 2)})
    for im in (3, 99):   # a category without detections; an image without predictions
        anns.append({'id': len(anns) + 1, 'image_id': im, 'category_id': 80, 'bbox': [10.0, 10.0, 50.0, 40.0],
                     'area': 2000.0, 'iscrowd': 0})
    anns.append({'id': len(anns) + 1, 'image_id': 99, 'category_id': 0, 'bbox': [5.0, 5.0, 30.0, 30.0], 'area': 900.0,
                 'iscrowd': 0})
    anno = {'images': [{'id': i} for i in list(range(len(CROPS))) + [99]], 'annotations': anns,
            'categories': [{'id': c, 'name': str(c)} for c in range(81)]}
    path = root / 'instances.json'
    path.write_text(json.dumps(anno))
    return str(path)


def run_test(w, save_dir, anno_json, loader=None, **kw):
    """test(save_json=True) with opt.anno_json set and pycocotools made unimportable -> (result, text, stats)."""
    T, seen = w['T'], {}
    real = C.CocoEvaluator.summarize

    def spy(self, *a, **k):
        seen['stats'] = real(self, *a, **k)
        return seen['stats']
    buf = io.StringIO()
    with pytest.MonkeyPatch.context() as mp, contextlib.redirect_stdout(buf):
        mp.setitem(sys.modules, 'pycocotools', None)     # `import pycocotools` raises ImportError
        mp.setattr(C.CocoEvaluator, 'summarize', spy)
        mp.setattr(T.opt, 'anno_json', anno_json, raising=False)
        res = T.test(w['data'], batch_size=BATCH, imgsz=IMGSZ, conf_thres=CONF, iou_thres=IOU, model=w['model'],
                     dataloader=loader if loader is not None else make_loader(w['path']), save_dir=save_dir,
                     save_json=True, plots=False, **kw)
    return res, buf.getvalue(), seen.get('stats')


@pytest.fixture(scope='module')
def coco(world, tmp_path_factory):
    out = tmp_path_factory.mktemp('cocoeval')
    anno = write_annotations(world['root'])
    res, text, stats = run_test(world, out, anno)
    pred = str(out / '_predictions.json')
    return dict(anno=anno, pred=pred, res=res, text=text, stats=stats, ref=R.evaluate(pred, anno), out=out)


def pinned_predictions(w):
    """_predictions.json as tests/test_evaluate.py pins it (test.py:168-177 on the per-image chain)."""
    jwant = []
    for path, (pred, predn, shapes) in w['ref']['per_image'].items():
        b = G.xyxy2xywh(predn[:, :4])
        b[:, :2] -= b[:, 2:] / 2
        for p, bb in zip(pred.tolist(), b.tolist()):
            jwant.append({'image_id': int(Path(path).stem), 'category_id': int(p[5]), 'bbox': [round(x, 3) for x in bb],
                          'score': round(p[4], 5)})
    return jwant


def test_the_fixture_is_not_vacuous(coco):
    ref = coco['ref']
    assert 0 < ref['stats'][0] < 1, ref['stats']
    assert ref['crowd_matches'] >= 1 and ref['ignored_by_range'] >= 1 and ref['max_gts_per_image_class'] > 1, \
        {k: ref[k] for k in ('crowd_matches', 'ignored_by_range', 'max_gts_per_image_class')}
    areas = [a['area'] for a in json.load(open(coco['anno']))['annotations']]
    assert min(areas) < 1024 and max(areas) > 9216 and any(1024 < a < 9216 for a in areas)
    # category 80: gts and no detections
    assert (ref['precision'][:, :, 80, 0, 2] == 0).all() and (ref['recall'][:, 80, 0, 2] == 0).all()


def test_map_and_the_twelve_stats_equal_the_restatement(coco):
    (mp, mr, map50, map_, *_), maps, t = coco['res']
    ref = coco['ref']
    print(coco['stats'], ref['stats'])
    assert (map_, map50) == (ref['stats'][0], ref['stats'][1])
    assert np.array_equal(coco['stats'], ref['stats'])
    for line in ref['lines']:
        assert line in coco['text'].splitlines(), line
    assert 'pycocotools unable to run' not in coco['text']


def test_predictions_json_is_unchanged(world, coco):
    assert json.loads(Path(coco['pred']).read_text()) == pinned_predictions(world)


def test_evaluate_json_gives_the_same_stats(coco):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        stats = C.evaluate_json(coco['anno'], coco['pred'])
    assert np.array_equal(stats, coco['ref']['stats'])
    assert buf.getvalue().splitlines() == coco['ref']['lines']


def test_without_the_annotation_file_nothing_changes(world, coco, tmp_path):
    res, text, stats = run_test(world, tmp_path, str(tmp_path / 'missing.json'))
    assert stats is None and 'pycocotools unable to run' in text
    assert_equals_reference(world, res, text)
    assert (tmp_path / '_predictions.json').read_text() == Path(coco['pred']).read_text()
    assert json.loads((tmp_path / '_predictions.json').read_text()) == pinned_predictions(world)


def test_next_batch_is_enqueued_before_results_are_read(world, coco, tmp_path):
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            with pytest.raises(RuntimeError):
                torch.ones(1, device='cuda').item()     # the mode must see a real sync, or it shows nothing
        finally:
            torch.cuda.set_sync_debug_mode('default')
    except (pytest.fail.Exception, AttributeError):
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag a .item() on this ROCm build')
    res, text, stats = run_test(world, tmp_path, coco['anno'], loader=ForeignLoader(world['path'], probe=True))
    assert np.array_equal(stats, coco['ref']['stats'])
    assert (res[0][3], res[0][2]) == (coco['ref']['stats'][0], coco['ref']['stats'][1])


def test_unknown_image_raises(world, tmp_path):
    anno = json.load(open(write_annotations(world['root'])))
    anno['images'] = [im for im in anno['images'] if im['id'] != 2]
    anno['annotations'] = [a for a in anno['annotations'] if a['image_id'] != 2]
    (tmp_path / 'a.json').write_text(json.dumps(anno))
    with pytest.raises(ValueError, match='2'):
        run_test(world, tmp_path, str(tmp_path / 'a.json'))
