"""test.py with plots: the confusion matrix accumulated on the device equals the reference's per-image chain, and the
five plot files appear where the reference writes them.

On tests/test_evaluate.py's ten-image set.  The chain: ConfusionMatrix.process_batch on each image's native-space
predictions and native labels, skipping an image without predictions (test.py:137-140) or without labels (`if nl`),
as test.py:181-189 does."""
import numpy as np
import pytest
import torch

from test_evaluate import make_loader, run, world  # noqa: F401  (world is the module's fixture)
from utils import general as G
from utils.metrics import ConfusionMatrix

pytestmark = pytest.mark.gpu

FILES = ('confusion_matrix.png', 'PR_curve.png', 'F1_curve.png', 'P_curve.png', 'R_curve.png')
NC = 80


@pytest.fixture(scope='module')
def chain_matrix(world):
    cm = ConfusionMatrix(nc=NC)
    used = 0
    for img, targets, paths, shapes in make_loader(world['path']):
        height, width = img.shape[2:]
        targets = targets.cpu().clone()
        targets[:, 2:] *= torch.Tensor([width, height, width, height])
        for si, path in enumerate(paths):
            labels = targets[targets[:, 0] == si, 1:]
            if path not in world['ref']['per_image'] or not len(labels):
                continue
            predn = world['ref']['per_image'][path][1]
            tbox = G.xywh2xyxy(labels[:, 1:5])
            G.scale_coords((height, width), tbox, shapes[si][0], shapes[si][1])
            cm.process_batch(predn, torch.cat((labels[:, 0:1], tbox), 1))
            used += 1
    assert used >= 8
    return cm.matrix


@pytest.fixture
def spy(world, monkeypatch):
    made = []

    class Spy(ConfusionMatrix):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(world['T'], 'ConfusionMatrix', Spy)
    return made


def test_matrix_equals_the_per_image_chain_and_the_files_are_written(world, chain_matrix, spy, tmp_path):
    w = world
    res, _ = run(w, w['data'], model=w['model'], dataloader=make_loader(w['path']), save_dir=tmp_path, plots=True)
    assert len(spy) == 1 and (spy[0].nc, spy[0].conf, spy[0].iou_thres) == (NC, 0.25, 0.45)
    got = spy[0].matrix
    assert got.dtype == np.float64 and np.array_equal(got, chain_matrix)
    assert spy[0].host_matrix.sum() == 0, 'the evaluation accumulates on the device only'
    assert got.sum() > 0 and got[:NC, :NC].sum() > 0 and got[NC].sum() + got[:, NC].sum() > 0
    for f in FILES:
        assert (tmp_path / f).stat().st_size > 0, f
    # plots=False: nothing is built or written, and the results are the same
    off = tmp_path / 'off'
    off.mkdir()
    res_off, _ = run(w, w['data'], model=w['model'], dataloader=make_loader(w['path']), save_dir=off, plots=False)
    assert len(spy) == 1 and not list(off.iterdir())
    assert res_off[0] == res[0] and np.array_equal(res_off[1], res[1])


def test_weights_entry_writes_the_files_into_its_run_directory(world, chain_matrix, spy, tmp_path):
    w = world
    w['T'].opt.project, w['T'].opt.name = str(tmp_path), 'exp'
    run(w, w['yaml'], weights=w['ckpt'])
    for f in FILES:
        assert (tmp_path / 'exp' / f).stat().st_size > 0, f
    assert np.array_equal(spy[0].matrix, chain_matrix)


def test_model_with_the_default_save_dir_writes_no_file(world, chain_matrix, spy, tmp_path, monkeypatch):
    w = world
    monkeypatch.chdir(tmp_path)
    run(w, w['data'], model=w['model'], dataloader=make_loader(w['path']))
    assert not list(tmp_path.iterdir())
    assert np.array_equal(spy[0].matrix, chain_matrix), 'the matrix is accumulated all the same'
