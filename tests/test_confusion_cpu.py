"""utils.metrics.ConfusionMatrix on the host, yv7_confusion's argument checks and the plot files (no GPU).

process_batch is checked against answers worked by hand from the reference's rules (utils/metrics.py:121-159) and
against an independent restatement of its steps written here: sort the candidate pairs by IoU, descending, keep the
first per detection, sort again, keep the first per label.  The restatement sorts stably, so where no two candidate
IoUs of one detection or one label are equal it is the reference whatever its argsort does; the random images are
seeded so that this holds, and the test says so before it compares."""
import matplotlib
import numpy as np
import pytest
import torch

from utils.metrics import ConfusionMatrix, ap_per_class, box_iou
from yv7 import _lib


def cells(cm):
    """The non-zero cells of the matrix as {(row, col): count}."""
    m = cm.matrix
    assert m.dtype == np.float64 and m.shape == (cm.nc + 1, cm.nc + 1)
    return {(int(r), int(c)): int(m[r, c]) for r, c in zip(*np.nonzero(m))}


def run(dets, labels, nc=3, **kw):
    cm = ConfusionMatrix(nc, **kw)
    cm.process_batch(torch.tensor(dets, dtype=torch.float32).reshape(-1, 6),
                     torch.tensor(labels, dtype=torch.float32).reshape(-1, 5))
    return cells(cm)


# ------------------------------------------------------------------------------------------ hand-worked answers
def test_plain_match():
    assert run([[0, 0, 10, 10, 0.9, 2]], [[2, 0, 0, 10, 10]]) == {(2, 2): 1}


def test_wrong_class_match_lands_at_label_class_row_and_prediction_class_column():
    assert run([[0, 0, 10, 10, 0.9, 2]], [[1, 0, 0, 10, 10]]) == {(1, 2): 1}


def test_two_rows_choose_one_label_the_loser_takes_no_second_choice():
    # row 0: IoU 1 with label 0, 0.6 with label 1; row 1: 0.9 with label 0, 60 / 90 with label 1.  Both choose
    # label 0, row 0 keeps it; row 1 is unmatched although label 1 would be a candidate, and label 1 stays unmatched
    got = run([[0, 0, 10, 10, 0.9, 0], [0, 0, 10, 9, 0.8, 1]], [[0, 0, 0, 10, 10], [2, 0, 0, 10, 6]])
    assert got == {(0, 0): 1, (1, 3): 1, (3, 2): 1}


def test_live_rows_without_a_candidate_pair_count_the_labels_only():
    got = run([[40, 40, 50, 50, 0.9, 0], [60, 60, 70, 70, 0.8, 1]], [[2, 0, 0, 10, 10], [2, 20, 20, 30, 30]])
    assert got == {(3, 2): 2}


def test_rows_at_exactly_conf_are_not_live():
    got = run([[0, 0, 10, 10, 0.25, 1], [20, 20, 30, 30, 0.25, 1]], [[1, 0, 0, 10, 10], [0, 20, 20, 30, 30]])
    assert got == {(3, 1): 1, (3, 0): 1}


def test_iou_exactly_at_the_threshold_is_excluded():
    assert run([[0, 0, 2, 1, 0.9, 0]], [[0, 0, 0, 1, 1]], iou_thres=0.5) == {(3, 0): 1}
    assert run([[0, 0, 2, 1, 0.9, 0]], [[0, 0, 0, 1, 1]], iou_thres=0.45) == {(0, 0): 1}


def test_tie_a_row_takes_the_first_maximum_in_label_order():
    assert run([[0, 0, 10, 10, 0.9, 2]], [[0, 0, 0, 10, 10], [1, 0, 0, 10, 10]]) == {(0, 2): 1, (3, 1): 1}
    assert run([[0, 0, 10, 10, 0.9, 2]], [[1, 0, 0, 10, 10], [0, 0, 0, 10, 10]]) == {(1, 2): 1, (3, 0): 1}


def test_tie_a_label_takes_the_lowest_row():
    assert run([[0, 0, 10, 10, 0.9, 1], [0, 0, 10, 10, 0.8, 2]], [[0, 0, 0, 10, 10]]) == {(0, 1): 1, (2, 3): 1}
    assert run([[0, 0, 10, 10, 0.9, 2], [0, 0, 10, 10, 0.8, 1]], [[0, 0, 0, 10, 10]]) == {(0, 2): 1, (1, 3): 1}


def test_empty_sides():
    assert run([], [[1, 0, 0, 10, 10]]) == {(3, 1): 1}
    assert run([[0, 0, 10, 10, 0.9, 1]], []) == {}


def test_out_of_range_class_is_dropped_counted_and_reported():
    cm = ConfusionMatrix(3)
    cm.process_batch(torch.tensor([[0, 0, 10, 10, 0.9, 3.0]]), torch.tensor([[1.0, 0, 0, 10, 10]]))
    cm.process_batch(torch.zeros(0, 6), torch.tensor([[float('nan'), 0, 0, 10, 10], [-0.5, 0, 0, 10, 10]]))
    assert cm.host_dropped == 2 and cm.host_matrix.sum() == 1 and cm.host_matrix[3, 0] == 1   # -0.5 truncates to 0
    with pytest.raises(ValueError, match='2 increments dropped'):
        cm.matrix
    with pytest.raises(ValueError, match='1..1024'):
        ConfusionMatrix(0)


def test_print_writes_the_rows(capsys):
    cm = ConfusionMatrix(1)
    cm.process_batch(torch.tensor([[0, 0, 10, 10, 0.9, 0.0]]), torch.tensor([[0.0, 0, 0, 10, 10]]))
    cm.print()
    assert capsys.readouterr().out == '1.0 0.0\n0.0 0.0\n'


# ------------------------------------------------------------------------------------------ the restatement
def restated(dets, labels, nc, conf=0.25, iou_thres=0.45):
    """The reference's steps with stable sorts -> (matrix [nc + 1, nc + 1] int64, whether an IoU tie was met)."""
    out = np.zeros((nc + 1, nc + 1), dtype=np.int64)
    dets = dets[dets[:, 4] > conf]
    iou = box_iou(labels[:, 1:], dets[:, :4])
    pairs = [(float(iou[l, d]), l, d) for l in range(labels.shape[0]) for d in range(dets.shape[0])
             if bool(iou[l, d] > iou_thres)]
    tie = False
    for axis in (2, 1):
        for k in {p[axis] for p in pairs}:
            v = [p[0] for p in pairs if p[axis] == k]
            tie |= len(set(v)) != len(v)
    pairs.sort(key=lambda p: -p[0])            # by IoU, descending
    per_det = {}
    for p in pairs:
        per_det.setdefault(p[2], p)            # the first of every detection
    pairs = sorted(per_det.values(), key=lambda p: -p[0])
    per_label = {}
    for p in pairs:
        per_label.setdefault(p[1], p)          # the first of every label
    matched_dets = {p[2] for p in per_label.values()}
    for l in range(labels.shape[0]):
        if l in per_label:
            out[int(labels[l, 0]), int(dets[per_label[l][2], 5])] += 1
        else:
            out[nc, int(labels[l, 0])] += 1
    if per_label:
        for d in range(dets.shape[0]):
            if d not in matched_dets:
                out[int(dets[d, 5]), nc] += 1
    return out, tie


def random_image(seed, nc, n_labels, n_dets):
    """Labels in a 640 x 640 image and detections that are mostly jittered copies of them, so that detections
    compete for labels and labels for detections."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n_labels, 2, generator=g) * 500 + 20
    wh = torch.rand(n_labels, 2, generator=g) * 100 + 20
    labels = torch.cat((torch.randint(0, nc, (n_labels, 1), generator=g).float(), xy, xy + wh), 1)
    pick = torch.randint(0, n_labels, (n_dets,), generator=g)
    box = labels[pick, 1:] + (torch.rand(n_dets, 4, generator=g) - 0.5) * 30
    cls = torch.where(torch.rand(n_dets, generator=g) < 0.2, torch.randint(0, nc, (n_dets,), generator=g).float(),
                      labels[pick, 0])
    conf = torch.rand(n_dets, generator=g)
    return torch.cat((box, conf[:, None], cls[:, None]), 1), labels


@pytest.mark.parametrize('seed,nc,n_labels,n_dets', [(1, 3, 8, 30), (2, 5, 20, 60), (3, 80, 40, 200), (4, 1, 5, 40),
                                                     (5, 4, 60, 20)])
def test_process_batch_agrees_with_the_restatement(seed, nc, n_labels, n_dets):
    dets, labels = random_image(seed, nc, n_labels, n_dets)
    want, tie = restated(dets, labels, nc)
    assert not tie, 'the seed must give no two equal candidate IoUs in one row or one label'
    cm = ConfusionMatrix(nc)
    cm.process_batch(dets, labels)
    got = cm.matrix
    assert np.array_equal(got, want.astype(np.float64))
    assert want[:nc, :nc].sum() > 0 and want[:, nc].sum() > 0, 'the image must have matches and unmatched rows'


# ------------------------------------------------------------------------------------------ host-only checks
def call_confusion(B=1, max_det=300, L=0, nc=80, ws_bytes=1 << 20, images=None):
    lib = _lib.lib()
    rc = lib.yv7_confusion(None, None, B, max_det, None, None, L, images, 640, 640, 0.25, 0.45, nc, None, None,
                           ws_bytes, None)
    return rc, lib.yv7_last_error().decode()


def test_confusion_argument_errors_are_host_only():
    """Every refusal comes back as -1 with its own text, before any device is touched (null pointers throughout)."""
    seen = set()
    for kw, text in (({'B': 0}, 'B must be positive'), ({'B': -3}, 'B must be positive'),
                     ({'max_det': 0}, 'max_det must be positive'), ({'max_det': -1}, 'max_det must be positive'),
                     ({'nc': 0}, 'nc must be in 1..1024'), ({'nc': -2}, 'nc must be in 1..1024'),
                     ({'nc': 1025}, 'nc must be in 1..1024'), ({'L': -1}, 'L must not be negative'),
                     ({'L': 4}, 'null targets with L > 0'), ({'ws_bytes': 1199}, 'ws_bytes too small'),
                     ({}, 'null argument')):
        rc, msg = call_confusion(**kw)
        assert rc == -1 and msg == 'yv7_confusion: ' + text, (kw, rc, msg)
        seen.add(msg)
    assert len(seen) == 7
    images = (_lib.ScaleDesc * 1)(_lib.ScaleDesc(480, 640, 1.0, 0.0, 0.0))
    rc, msg = call_confusion(images=images)
    assert rc == -1 and msg == 'yv7_confusion: null argument'


def test_confusion_ws_bytes():
    f = _lib.lib().yv7_confusion_ws_bytes
    assert f(1, 300, 0) == 1200 and f(2, 300, 10) == 2 * 300 * 4 + 10 * 8
    assert f(0, 300, 10) == 0 and f(1, 0, 10) == 0 and f(1, 300, -1) == 0


def test_process_batches_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match='ROCm'):
        ConfusionMatrix(80).process_batches(torch.zeros(1, 300, 6), torch.zeros(1, dtype=torch.int32),
                                            torch.zeros(0, 6), torch.zeros(2, dtype=torch.int32),
                                            [(480, 640, 1.0, 0.0, 0.0)], (640, 640))


# ------------------------------------------------------------------------------------------ plot files
PNG = b'\x89PNG\r\n\x1a\n'
CURVES = ('PR_curve.png', 'F1_curve.png', 'P_curve.png', 'R_curve.png')


def pyplot_state():
    import matplotlib.pyplot as plt
    return matplotlib.get_backend(), len(plt.get_fignums())


def stats(seed=0, n=400, ncls=3):
    rng = np.random.default_rng(seed)
    conf = rng.random(n).astype(np.float32)
    tp = rng.random((n, 10)) < conf[:, None] * np.linspace(1.0, 0.3, 10)
    return tp, conf, rng.integers(0, ncls, n).astype(np.float32), rng.integers(0, ncls, 150).astype(np.float32)


@pytest.mark.parametrize('names', [{0: 'a', 1: 'b', 2: 'c'}, ()])
def test_ap_per_class_plot_writes_four_curves_and_returns_the_same(tmp_path, names):
    before = pyplot_state()
    want = ap_per_class(*stats())
    assert not list(tmp_path.iterdir())
    got = ap_per_class(*stats(), plot=True, save_dir=tmp_path, names=names)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    for f in CURVES:
        assert (tmp_path / f).read_bytes()[:8] == PNG, f
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(CURVES)
    assert pyplot_state() == before


@pytest.mark.parametrize('nc,named', [(3, True), (3, False), (40, True)])
def test_confusion_matrix_plot_writes_its_file(tmp_path, nc, named):
    before = pyplot_state()
    cm = ConfusionMatrix(nc)
    dets, labels = random_image(9, nc, 12, 40)
    cm.process_batch(dets, labels)
    cm.plot(save_dir=tmp_path, names=[f'class{i}' for i in range(nc)] if named else ())
    assert (tmp_path / 'confusion_matrix.png').read_bytes()[:8] == PNG
    assert [p.name for p in tmp_path.iterdir()] == ['confusion_matrix.png']
    assert pyplot_state() == before


def test_an_empty_matrix_still_plots_and_a_plot_error_propagates(tmp_path):
    ConfusionMatrix(2).plot(save_dir=tmp_path)
    assert (tmp_path / 'confusion_matrix.png').read_bytes()[:8] == PNG
    with pytest.raises(OSError):
        ConfusionMatrix(2).plot(save_dir=tmp_path / 'missing')
