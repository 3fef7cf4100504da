"""yv7_confusion: the evaluation's confusion matrix for a whole batch in one launch, against
ConfusionMatrix.process_batch (the host's per-image restatement of utils/metrics.py:121-159) summed image by image
over natively scaled labels, with the reference's two skips (test.py:137-140 and `if nl`).

The C ABI runs on guarded buffers: a guard word on either side of the matrix and of the scratch, the scratch filled
with junk, and a check that no input changed.  Every comparison is torch.equal on the int32 matrix, the dropped
counter included."""
import pytest
import torch

from test_match import GUARD32, IDENT, RAGGED_CHUNK, S, jittered_predictions, label, native_labels, random_targets
from utils.metrics import ConfusionMatrix
from yv7 import _lib

pytestmark = pytest.mark.gpu

GUARD64 = 0x7f7f7f7f7f7f7f7f


def reference(det, count, targets, off, descs, canvas, nc, conf=0.25, iou_thres=0.45):
    """int32 [(nc + 1)^2 + 1]: process_batch per image, the dropped increments in the last entry."""
    cm = ConfusionMatrix(nc, conf, iou_thres)
    for b in range(det.shape[0]):
        n = int(count[b])
        if n == 0 or off[b + 1] == off[b]:
            continue
        cm.process_batch(det[b, :n], native_labels(targets[off[b]:off[b + 1], 1:], descs[b], canvas))
    return torch.cat((torch.from_numpy(cm.host_matrix).flatten(), torch.tensor([cm.host_dropped]))).to(torch.int32)


def run(det, count, targets, off, descs, canvas, nc, conf=0.25, iou_thres=0.45, calls=1):
    """`calls` yv7_confusion calls into one zeroed, guarded matrix -> int32 [(nc + 1)^2 + 1] on the host."""
    B, max_det, _ = det.shape
    L = targets.shape[0]
    d_det, d_cnt, d_tgt = det.cuda(), count.cuda(), targets.cuda()
    d_off = torch.tensor(off, dtype=torch.int32).cuda()
    keep = [t.clone() for t in (d_det, d_cnt, d_tgt, d_off)]
    n = (nc + 1) ** 2 + 1
    mat = torch.full((n + 2,), GUARD32, dtype=torch.int32).cuda()
    mat[1:-1] = 0
    nbytes = _lib.lib().yv7_confusion_ws_bytes(B, max_det, L)
    assert nbytes == L * 8 + B * max_det * 4
    words = (nbytes + 7) // 8
    ws = torch.full((words + 2,), GUARD64, dtype=torch.int64).cuda()      # junk inside, guards outside
    arr = (_lib.ScaleDesc * B)(*[_lib.ScaleDesc(*d) for d in descs])
    for _ in range(calls):
        rc = _lib.lib().yv7_confusion(d_det.data_ptr(), d_cnt.data_ptr(), B, max_det, d_tgt.data_ptr() if L else None,
                                      d_off.data_ptr(), L, arr, canvas[0], canvas[1], conf, iou_thres, nc,
                                      mat[1:].data_ptr(), ws[1:].data_ptr(), nbytes,
                                      torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, 'yv7_confusion')
    torch.cuda.synchronize()
    mat, ws = mat.cpu(), ws.cpu()
    assert int(mat[0]) == GUARD32 and int(mat[-1]) == GUARD32, 'written outside the matrix'
    assert int(ws[0]) == GUARD64 and int(ws[-1]) == GUARD64, 'written outside the scratch'
    if nbytes % 8:
        assert int(ws[-2]) >> 32 == GUARD64 >> 32, 'written past ws_bytes'
    for now, before in zip((d_det, d_cnt, d_tgt, d_off), keep):
        assert torch.equal(now.view(torch.uint8), before.view(torch.uint8)), 'an input changed'
    return mat[1:-1]


def check(det, count, targets, off, descs, canvas, nc, **kw):
    want = reference(det, count, targets, off, descs, canvas, nc, **kw)
    got = run(det, count, targets, off, descs, canvas, nc, **kw)
    assert torch.equal(got, want), (got.nonzero().flatten().tolist(), want.nonzero().flatten().tolist())
    return got


def cells(flat, nc):
    m = flat[:-1].reshape(nc + 1, nc + 1)
    return {(int(r), int(c)): int(m[r, c]) for r, c in m.nonzero().tolist()}, int(flat[-1])


# ------------------------------------------------------------------------------------------ hand cases
def one_image(rows, labels, nc=3, max_det=8, **kw):
    """rows: (x1, y1, x2, y2, conf, cls); labels: (cls, x1, y1, x2, y2) on the 64 x 64 identity canvas."""
    det = torch.full((1, max_det, 6), 7.0)
    det[0, :, 4] = 0.99                                   # rows >= count are junk that would be live
    for r, row in enumerate(rows):
        det[0, r] = torch.tensor(row, dtype=torch.float32)
    targets = torch.tensor([label(*lab) for lab in labels], dtype=torch.float32).reshape(-1, 6)
    flat = check(det, torch.tensor([len(rows)], dtype=torch.int32), targets, [0, len(labels)], [IDENT], (S, S), nc,
                 **kw)
    return cells(flat, nc)


HAND = {
    'plain match': ([(0, 0, 10, 10, 0.9, 2)], [(2, 0, 0, 10, 10)], {}, {(2, 2): 1}),
    'wrong class': ([(0, 0, 10, 10, 0.9, 2)], [(1, 0, 0, 10, 10)], {}, {(1, 2): 1}),
    'two rows, one label': ([(0, 0, 10, 10, 0.9, 0), (0, 0, 10, 9, 0.8, 1)], [(0, 0, 0, 10, 10), (2, 0, 0, 10, 6)], {},
                            {(0, 0): 1, (1, 3): 1, (3, 2): 1}),
    'no candidate pair': ([(40, 40, 50, 50, 0.9, 0), (52, 52, 62, 62, 0.8, 1)],
                          [(2, 0, 0, 10, 10), (2, 20, 20, 30, 30)], {}, {(3, 2): 2}),
    'rows at conf': ([(0, 0, 10, 10, 0.25, 1), (20, 20, 30, 30, 0.25, 1)], [(1, 0, 0, 10, 10), (0, 20, 20, 30, 30)], {},
                     {(3, 1): 1, (3, 0): 1}),
    'iou at the threshold': ([(0, 0, 2, 1, 0.9, 0)], [(0, 0, 0, 1, 1)], {'iou_thres': 0.5}, {(3, 0): 1}),
    'iou above the threshold': ([(0, 0, 2, 1, 0.9, 0)], [(0, 0, 0, 1, 1)], {}, {(0, 0): 1}),
    'row tie: first label': ([(0, 0, 10, 10, 0.9, 2)], [(1, 0, 0, 10, 10), (0, 0, 0, 10, 10)], {},
                             {(1, 2): 1, (3, 0): 1}),
    'label tie: lowest row': ([(0, 0, 10, 10, 0.9, 2), (0, 0, 10, 10, 0.8, 1)], [(0, 0, 0, 10, 10)], {},
                              {(0, 2): 1, (1, 3): 1}),
}


@pytest.mark.parametrize('name', list(HAND))
def test_hand_cases(name):
    rows, labels, kw, want = HAND[name]
    assert one_image(rows, labels, **kw) == (want, 0)


def test_bad_classes_and_a_nan_box_are_dropped_and_counted():
    nan = float('nan')
    # row 0: class 3 == nc, matched -> dropped.  row 1: NaN box, never a candidate, unmatched and live -> [1][nc].
    # row 2: NaN class, unmatched -> dropped.  label 1: class -1, unmatched -> dropped.  label 2: class 2.9 -> 2
    got = one_image([(0, 0, 10, 10, 0.9, 3), (nan, 0, 10, 10, 0.9, 1), (40, 40, 50, 50, 0.9, nan)],
                    [(0, 0, 0, 10, 10), (-1, 20, 20, 30, 30), (2.9, 30, 30, 40, 40)])
    assert got == ({(1, 3): 1, (3, 2): 1}, 3)


# ------------------------------------------------------------------------------------------ generated cases
def image(g, n_rows, n_labels, nc, desc, canvas, index, max_det):
    """(det [max_det,6], targets [n_labels,6]): jittered copies of the labels, classes inside [0, nc)."""
    rows = random_targets(g, max(n_labels, 1), nc, float(index))
    det = torch.rand(max_det, 6, generator=g) * 100.0            # junk wherever no prediction is placed
    det[:, 4] = 0.99
    det[:, 5] = 0.0
    if n_rows:
        p = jittered_predictions(g, n_rows, rows, desc, canvas)
        p[:, 5] = p[:, 5] % nc
        det[:n_rows] = p
    return det, rows[:n_labels]


def batch(seed, sizes, nc, descs, canvas, max_det):
    g = torch.Generator().manual_seed(seed)
    parts = [image(g, n, m, nc, descs[b], canvas, b, max_det) for b, (n, m) in enumerate(sizes)]
    off = [0]
    for _, m in sizes:
        off.append(off[-1] + m)
    count = torch.tensor([n for n, _ in sizes], dtype=torch.int32)
    return torch.stack([p[0] for p in parts]), count, torch.cat([p[1] for p in parts]), off


def test_edge_counts_and_label_counts_with_a_non_identity_descriptor():
    """count 0, 1, 255, 256, 257, 300 at max_det 300 against 5, 1, 256, 257, 600, 0 and 40 labels: images skipped for
    either reason, rows past one workgroup's 256 and labels past one staging chunk; gain 0.5 with pads (16, 76)."""
    canvas, desc = (512, 672), (720, 1280, 0.5, 16.0, 76.0)
    sizes = [(0, 5), (1, 1), (255, 256), (256, 257), (257, 600), (300, 0), (300, 40)]
    det, count, targets, off = batch(21, sizes, 3, [desc] * len(sizes), canvas, 300)
    flat = check(det, count, targets, off, [desc] * len(sizes), canvas, 3)
    got, dropped = cells(flat, 3)
    assert dropped == 0 and sum(v for (r, c), v in got.items() if r < 3 and c < 3) > 100
    assert any(r == 3 for r, _ in got) and any(c == 3 for _, c in got), 'unmatched labels and rows must occur'


def test_600_rows_and_600_labels_at_max_det_600():
    canvas, descs = (640, 640), [(480, 640, 1.0, 0.0, 80.0)]
    det, count, targets, off = batch(22, [(600, 600)], 80, descs, canvas, 600)
    flat = check(det, count, targets, off, descs, canvas, 80)
    assert int(flat[:-1].sum()) >= 600 and int(flat[-1]) == 0


@pytest.mark.parametrize('B,nc', [(1, 1), (RAGGED_CHUNK - 1, 3), (RAGGED_CHUNK, 128), (RAGGED_CHUNK + 1, 80)])
def test_batch_sizes_around_the_descriptor_chunk_with_skipped_images(B, nc):
    """Every third image has no rows and every fifth no labels; past 64 images a second launch takes the rest."""
    descs = [(S - (b % 5), S - (b % 3), 1.0, 0.0, 0.0) for b in range(B)]
    sizes = [(0 if b % 3 == 2 else 4, 0 if b % 5 == 2 else 3) for b in range(B)]
    det, count, targets, off = batch(23 + B, sizes, nc, descs, (S, S), 6)
    flat = check(det, count, targets, off, descs, (S, S), nc)
    contributing = [m for n, m in sizes if n and m]
    assert int(flat[-1]) == 0 and int(flat[:-1].sum()) >= sum(contributing)       # every label lands in some cell
    if B > RAGGED_CHUNK:
        last = reference(det[-1:], count[-1:], targets[off[-2]:], [0, off[-1] - off[-2]], descs[-1:], (S, S), nc)
        assert int(last.sum()) > 0, 'the image behind the chunk boundary must contribute'


def test_calls_add_up_and_repeat_exactly_and_the_wrapper_gives_the_same():
    canvas, descs = (640, 640), [(480, 640, 1.0, 0.0, 80.0), (1080, 810, 640 / 1080, 80.0, 0.0)]
    args = batch(24, [(300, 200), (280, 150)], 5, descs, canvas, 300)
    once = check(*args, descs, canvas, 5)
    assert torch.equal(run(*args, descs, canvas, 5), once), 'the same call on a fresh matrix'
    assert torch.equal(run(*args, descs, canvas, 5, calls=2), once * 2), 'the kernel adds and never zeroes'
    cm = ConfusionMatrix(5)
    d = [t.cuda() for t in args[:3]] + [torch.tensor(args[3], dtype=torch.int32).cuda()]
    cm.process_batches(*d, descs, canvas)
    cm.process_batches(*d, descs, canvas)
    cm.process_batch(args[0][0, :300], native_labels(args[2][:200, 1:], descs[0], canvas))    # and a host part
    host = reference(args[0][:1], args[1][:1], args[2][:200], [0, 200], descs[:1], canvas, 5)
    want = (once * 2 + host)[:-1].reshape(6, 6).double().numpy()
    assert (cm.matrix == want).all()
