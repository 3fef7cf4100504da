"""yv7_match: predictions matched to labels for a whole batch in one launch, against the reference's per-image
chain on the CPU, bit for bit.

Reference per image: labels to canvas pixels (test.py:123), xywh2xyxy + scale_coords(ratio_pad) (test.py:186-187)
with the CPU helpers of utils.general, then oracle.metrics_ref.match_image (test.py:181-208).  claimed_by is
derived here by the same loop: per class in torch.unique order, the first prediction above iouv[0] to choose a
label keeps it.  Every comparison is torch.equal on the integer outputs."""
import ctypes

import pytest
import torch

from oracle import metrics_ref
from utils import general as G
from utils.metrics import match_batch
from yv7 import _lib

pytestmark = pytest.mark.gpu

IOUV = metrics_ref.IOUV
NIOU = len(IOUV)
RAGGED_CHUNK = 64          # descriptors per launch (include/yv7.h)
GUARD32 = 0x7f7f7f7f


def native_labels(rows, desc, canvas):
    """rows [m,5] (cls, x, y, w, h normalised to the canvas) -> [m,5] (cls, xyxy in the image's pixels)."""
    h0, w0, gain, pw, ph = desc
    lab = rows.clone()
    lab[:, 1:] *= torch.Tensor([canvas[1], canvas[0], canvas[1], canvas[0]])       # test.py:123
    tbox = G.xywh2xyxy(lab[:, 1:5])
    G.scale_coords(canvas, tbox, (h0, w0), ((gain, gain), (pw, ph)))               # test.py:187
    return torch.cat((lab[:, 0:1], tbox), 1)


def claims(pred, lab):
    """The winning prediction row of every label, or -1: test.py:192-210's bookkeeping."""
    out = torch.full((lab.shape[0],), -1, dtype=torch.int32)
    if not (lab.shape[0] and pred.shape[0]):
        return out
    tcls, tbox = lab[:, 0], lab[:, 1:5]
    for cls in torch.unique(tcls):
        ti = (cls == tcls).nonzero(as_tuple=False).view(-1)
        pi = (cls == pred[:, 5]).nonzero(as_tuple=False).view(-1)
        if pi.shape[0]:
            ious, i = metrics_ref.box_iou(pred[pi, :4], tbox[ti]).max(1)
            for j in (ious > IOUV[0]).nonzero(as_tuple=False):
                d = int(ti[i[j]])
                if out[d] < 0:
                    out[d] = int(pi[j])
    return out


def reference(det, count, targets, off, descs, canvas):
    B, max_det, _ = det.shape
    correct = torch.zeros((B, max_det, NIOU), dtype=torch.uint8)
    claimed = torch.full((targets.shape[0],), -1, dtype=torch.int32)
    for b in range(B):
        n = int(count[b])
        pred = det[b, :n]
        lab = native_labels(targets[off[b]:off[b + 1], 1:], descs[b], canvas)
        correct[b, :n] = metrics_ref.match_image(pred, lab).to(torch.uint8)
        claimed[off[b]:off[b + 1]] = claims(pred, lab)
    return correct, claimed


def run(det, count, targets, off, descs, canvas):
    """The C ABI on guarded outputs; checks the guards, the zero rows and that no input changed."""
    B, max_det, _ = det.shape
    L = targets.shape[0]
    d_det, d_cnt, d_tgt = det.cuda(), count.cuda(), targets.cuda()
    d_off = torch.tensor(off, dtype=torch.int32).cuda()
    keep = [t.clone() for t in (d_det, d_cnt, d_tgt, d_off)]
    buf = torch.full((B + 2, max_det, NIOU), 0xFF, dtype=torch.uint8).cuda()    # one image of 0xFF on either side
    cl = torch.full((L + 2,), GUARD32, dtype=torch.int32).cuda()
    arr = (_lib.ScaleDesc * B)(*[_lib.ScaleDesc(*d) for d in descs])
    iouv = (ctypes.c_float * NIOU)(*IOUV.tolist())
    rc = _lib.lib().yv7_match(d_det.data_ptr(), d_cnt.data_ptr(), B, max_det, d_tgt.data_ptr() if L else None,
                              d_off.data_ptr(), L, arr, canvas[0], canvas[1], iouv, NIOU, buf[1].data_ptr(),
                              cl[1:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'yv7_match')
    torch.cuda.synchronize()
    buf, cl = buf.cpu(), cl.cpu()
    assert bool((buf[0] == 0xFF).all()) and bool((buf[-1] == 0xFF).all()), 'correct written outside [B,max_det,niou]'
    assert int(cl[0]) == GUARD32 and int(cl[-1]) == GUARD32, 'claimed_by written outside [L]'
    for now, before in zip((d_det, d_cnt, d_tgt, d_off), keep):
        assert torch.equal(now.view(torch.uint8), before.view(torch.uint8)), 'an input changed'
    correct = buf[1:-1]
    for b in range(B):
        assert not correct[b, int(count[b]):].any(), 'rows >= count[b] must be zero'
    # the wrapper gives the same
    w_correct, w_claimed = match_batch(d_det, d_cnt, d_tgt, d_off, descs, canvas, IOUV)
    assert torch.equal(w_correct.cpu(), correct) and torch.equal(w_claimed.cpu(), cl[1:-1])
    return correct, cl[1:-1]


def check(det, count, targets, off, descs, canvas):
    want = reference(det, count, targets, off, descs, canvas)
    got = run(det, count, targets, off, descs, canvas)
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1])
    return got


# ------------------------------------------------------------------------------------------ hand cases
S = 64                      # canvas: a power of two keeps the hand-made normalised labels exact
IDENT = (S, S, 1.0, 0.0, 0.0)


def label(cls, x1, y1, x2, y2):
    return [0.0, float(cls), (x1 + x2) / 2 / S, (y1 + y2) / 2 / S, (x2 - x1) / S, (y2 - y1) / S]


def one_image(preds, labels, desc=IDENT, max_det=8):
    det = torch.full((1, max_det, 6), 7.0)              # rows >= count hold junk of a matching class
    for r, (box, cls) in enumerate(preds):
        det[0, r] = torch.tensor([*box, 0.9 - 0.1 * r, cls])
    targets = torch.tensor(labels, dtype=torch.float32).reshape(-1, 6)
    return check(det, torch.tensor([len(preds)], dtype=torch.int32), targets, [0, len(labels)], [desc], (S, S))


def test_class_mismatch_at_iou_one():
    correct, claimed = one_image([((10, 10, 20, 20), 1)], [label(2, 10, 10, 20, 20)])
    assert not correct.any() and claimed.tolist() == [-1]


def test_exact_match_is_correct_at_every_threshold():
    correct, claimed = one_image([((10, 10, 20, 20), 2)], [label(2, 10, 10, 20, 20)])
    assert correct[0, 0].tolist() == [1] * NIOU and claimed.tolist() == [0]


def test_iou_exactly_half_is_not_a_match():
    correct, claimed = one_image([((0, 0, 2, 1), 0)], [label(0, 0, 0, 1, 1)])
    assert not correct.any() and claimed.tolist() == [-1]


def test_two_identical_labels_first_index_wins():
    correct, claimed = one_image([((10, 10, 20, 20), 3)], [label(3, 10, 10, 20, 20), label(3, 10, 10, 20, 20)])
    assert correct[0, 0].all() and claimed.tolist() == [0, -1]


def test_two_predictions_one_label_lower_row_wins_loser_gets_nothing():
    # row 1 prefers label 0 (IoU 0.9) to label 1 (IoU 60/90) and loses it to row 0; label 1 stays unclaimed
    correct, claimed = one_image([((0, 0, 10, 10), 1), ((0, 0, 10, 9), 1)],
                                 [label(1, 0, 0, 10, 10), label(1, 0, 0, 10, 6)])
    assert correct[0, 0].all() and not correct[0, 1].any() and claimed.tolist() == [0, -1]


def test_nan_best_iou_claims_nothing():
    # row 0 has no area; against the zero-area label of its class its IoU is 0 / 0, and torch.max keeps the NaN
    # whether it comes before or after the good label.  Row 1 takes the good label as usual.
    for labels in ([label(4, 20, 20, 30, 30), label(4, 5, 5, 5, 5)], [label(4, 5, 5, 5, 5), label(4, 20, 20, 30, 30)]):
        correct, claimed = one_image([((5, 5, 5, 5), 4), ((20, 20, 30, 30), 4)], labels)
        good = 0 if labels[0][4] > 0 else 1
        assert not correct[0, 0].any() and correct[0, 1].all()
        assert claimed.tolist() == [1 if i == good else -1 for i in range(2)]


def test_label_clamped_by_scale_coords():
    # the image is 40 wide and 48 high on a 64 x 64 canvas: the label's box [30,30,60,60] clamps to [30,30,40,48]
    correct, claimed = one_image([((30, 30, 40, 48), 0)], [label(0, 30, 30, 60, 60)], desc=(48, 40, 1.0, 0.0, 0.0))
    assert correct[0, 0].all() and claimed.tolist() == [0]


# ------------------------------------------------------------------------------------------ generated cases
def random_targets(g, n, ncls, image=0.0):
    xy = torch.rand(n, 2, generator=g) * 0.8 + 0.1
    wh = torch.rand(n, 2, generator=g) * 0.18 + 0.02
    cls = torch.randint(0, ncls, (n, 1), generator=g).float()
    return torch.cat((torch.full((n, 1), image), cls, xy, wh), 1)


def jittered_predictions(g, n, rows, desc, canvas, wrong_class=0.1):
    """n predictions, each a label's native box moved by up to a few pixels, mostly of that label's class."""
    lab = native_labels(rows[:, 1:], desc, canvas)
    pick = torch.randint(0, lab.shape[0], (n,), generator=g)
    box = lab[pick, 1:5] + (torch.rand(n, 4, generator=g) - 0.5) * 12.0
    cls = lab[pick, 0].clone()
    flip = torch.rand(n, generator=g) < wrong_class
    cls[flip] = (cls[flip] + 1) % 5
    conf = torch.sort(torch.rand(n, generator=g), descending=True).values
    return torch.cat((box, conf[:, None], cls[:, None]), 1)


def test_edge_sizes_and_non_identity_descriptors():
    """Counts (0, 1, 300) and labels (5, 0, 700): labels without predictions, a prediction without labels, more
    rows than a workgroup has threads and more labels than one staging chunk; gain 0.5 with pads (16, 76)."""
    g = torch.Generator().manual_seed(11)
    canvas, desc = (512, 672), (720, 1280, 0.5, 16.0, 76.0)
    t0, t2 = random_targets(g, 5, 3, 0.0), random_targets(g, 700, 3, 2.0)
    targets = torch.cat((t0, t2))
    det = torch.rand(3, 300, 6, generator=g) * 100.0         # junk wherever no prediction is placed
    det[..., 5] = 1.0
    det[1, 0] = torch.tensor([100.0, 100.0, 300.0, 300.0, 0.8, 1.0])
    det[2] = jittered_predictions(g, 300, t2, desc, canvas)
    count = torch.tensor([0, 1, 300], dtype=torch.int32)
    correct, claimed = check(det, count, targets, [0, 5, 5, 705], [desc] * 3, canvas)
    assert correct[2].any() and (claimed[5:] >= 256).any(), 'the case must exercise rows past the first 256'
    assert (claimed[:5] == -1).all()


def test_dense_random():
    g = torch.Generator().manual_seed(5)
    canvas, descs = (640, 640), [(480, 640, 1.0, 0.0, 80.0), (1080, 810, 640 / 1080, 80.0, 0.0)]
    rows = [random_targets(g, 200, 5, float(b)) for b in range(2)]
    det = torch.stack([jittered_predictions(g, 300, rows[b], descs[b], canvas) for b in range(2)])
    count = torch.tensor([300, 300], dtype=torch.int32)
    correct, claimed = check(det, count, torch.cat(rows), [0, 200, 400], descs, canvas)
    won = correct[..., 0].sum(1)
    assert (won > 20).all() and (won < 300).all(), 'the case must have winners and losers'
    assert int((claimed >= 0).sum()) == int(won.sum())


def test_descriptor_chunk_boundary():
    """One more image than a launch carries descriptors: the last image takes the second launch."""
    B = RAGGED_CHUNK + 1
    g = torch.Generator().manual_seed(3)
    canvas = (S, S)
    descs = [(S - (b % 5), S - (b % 3), 1.0, 0.0, 0.0) for b in range(B)]
    targets = random_targets(g, B, 2)
    targets[:, 0] = torch.arange(B).float()
    det = torch.zeros(B, 4, 6)
    for b in range(B):
        lab = native_labels(targets[b:b + 1, 1:], descs[b], canvas)
        shift = 0.0 if b % 2 == 0 else 40.0      # odd images miss
        det[b, 0] = torch.tensor([*(lab[0, 1:5] + shift).tolist(), 0.5, float(lab[0, 0])])
    count = torch.ones(B, dtype=torch.int32)
    correct, claimed = check(det, count, targets, list(range(B + 1)), descs, canvas)
    assert claimed.tolist() == [0 if b % 2 == 0 else -1 for b in range(B)]
    assert correct[-1, 0].all()


def test_no_labels_at_all():
    det = torch.rand(2, 5, 6)
    correct, claimed = check(det, torch.tensor([5, 2], dtype=torch.int32), torch.zeros(0, 6), [0, 0, 0],
                             [IDENT] * 2, (S, S))
    assert not correct.any() and claimed.numel() == 0
