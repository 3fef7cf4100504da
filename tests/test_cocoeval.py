"""yv7_coco_match: the COCO bbox matching of a whole batch in one launch, against the contract's restatement
(tests/cocoeval_ref.py).  The outputs are integers, so they are compared with torch.equal.

Every cell calls the C ABI on buffers the test builds: rows >= count[b] of det are NaN, the outputs and the
workspace start as 0xFF bytes, and flags and rank sit between guard images that must stay 0xFF."""
import random

import numpy as np
import pytest
import torch

import cocoeval_ref as R
from yv7 import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def box(x, y, w, h):
    return (x, y, x + w, y + h)


# ---- images: (dets [(x1, y1, x2, y2, score, cls)], gts [(cls, x, y, w, h, area, crowd)])
def hand_worked():
    f = np.float32
    up = float(np.nextafter(f(0.5), f(1)))    # rounds to 0.5 at five decimals like 0.5 itself
    return [
        # one exact detection
        ([(*box(10, 10, 20, 20), 0.9, 0)], [(0, 10, 10, 20, 20, 400, 0)]),
        # TP FP TP
        ([(*box(10, 10, 20, 20), 0.9, 0), (*box(200, 200, 20, 20), 0.8, 0), (*box(100, 100, 20, 20), 0.7, 0)],
         [(0, 10, 10, 20, 20, 400, 0), (0, 100, 100, 20, 20, 400, 0)]),
        # a crowd matched twice; an unmatched detection outside the small range
        ([(*box(100, 100, 20, 20), 0.9, 0), (*box(130, 130, 20, 20), 0.8, 0), (*box(10, 10, 20, 20), 0.7, 0),
          (*box(300, 300, 100, 100), 0.6, 0)],
         [(0, 10, 10, 20, 20, 400, 0), (0, 100, 100, 60, 60, 3600, 1)]),
        # areas exactly 1024 and 9216, in two classes
        ([(*box(8, 8, 32, 32), 0.9, 1), (*box(8, 8, 96, 96), 0.9, 2)],
         [(1, 8, 8, 32, 32, 1024, 0), (2, 8, 8, 96, 96, 9216, 0)]),
        # IoU exactly 0.5; and 3-decimal rounding that moves an IoU onto 0.5 (9.9996 -> 10.0) or off it (9.9994)
        ([(0, 0, 10, 10, 0.9, 0), (100, 0, 109.9996, 10, 0.9, 1), (200, 0, 209.9994, 10, 0.9, 2)],
         [(0, 0, 0, 10, 20, 200, 0), (1, 100, 0, 10, 20, 200, 0), (2, 200, 0, 10, 20, 200, 0)]),
        # equal IoUs take the last gt
        ([(*box(12, 0, 20, 10), 0.9, 0), (*box(4, 0, 20, 10), 0.8, 0)],
         [(0, 10, 0, 20, 10, 200, 0), (0, 14, 0, 20, 10, 200, 0)]),
        # the break rule, crowd first
        ([(*box(0, 0, 10, 16), 0.9, 0)], [(0, 0, 0, 40, 40, 1600, 1), (0, 0, 0, 10, 10, 100, 0)]),
        # scores equal after rounding that differ before it: the row decides, not the raw score
        ([(*box(200, 200, 20, 20), 0.5, 0), (*box(10, 10, 20, 20), up, 0), (*box(10, 10, 20, 21), 0.5, 0)],
         [(0, 10, 10, 20, 20, 400, 0)]),
        # degenerate boxes on both sides
        ([(10, 10, 10, 30, 0.9, 0), (10, 10, 30, 10, 0.8, 0), (*box(10, 10, 20, 20), 0.7, 0)],
         [(0, 10, 10, 0, 20, 0, 0), (0, 10, 10, 20, 0, 0, 0), (0, 10, 10, 20, 20, 400, 0)]),
        # classes only among the gts (3) or only among the detections (5)
        ([(*box(10, 10, 20, 20), 0.9, 5), (*box(50, 50, 20, 20), 0.8, 0)],
         [(3, 10, 10, 20, 20, 400, 0), (0, 50, 50, 20, 20, 400, 0)]),
        # no rows; no gts
        ([], [(0, 10, 10, 20, 20, 400, 0), (1, 10, 10, 20, 20, 400, 1)]),
        ([(*box(10, 10, 20, 20), 0.9, 0), (*box(10, 10, 20, 20), 0.9, 7)], []),
        ([], []),
    ]


def rand_image(rng, n_det_per_class, n_gt_per_class, crowds='mixed'):
    """Per class c, n_det_per_class[c] rows and n_gt_per_class[c] gts; rows are jittered gts and stray boxes."""
    dets, gts = [], []
    for c, (nd, ng) in enumerate(zip(n_det_per_class, n_gt_per_class)):
        mine = []
        for j in range(ng):
            w, h = rng.uniform(8, 130), rng.uniform(8, 130)
            crowd = {'first': j < ng // 4, 'last': j >= ng - ng // 4, 'mixed': j % 3 == 1, 'none': False}[crowds]
            area = w * h * rng.choice((0.5, 1.0, 1.0))    # a segmentation area, smaller than the box
            mine.append((c, rng.uniform(0, 500), rng.uniform(0, 400), w, h, area, int(crowd)))
        gts += mine
        for j in range(nd):
            if mine and rng.random() < 0.8:
                g = mine[rng.randrange(len(mine))]
                j4 = [rng.uniform(-0.12, 0.12) * s for s in (g[3], g[4], g[3], g[4])]
                b = (g[1] + j4[0], g[2] + j4[1], g[1] + g[3] + j4[2], g[2] + g[4] + j4[3])
            else:
                b = box(rng.uniform(0, 500), rng.uniform(0, 400), rng.uniform(8, 130), rng.uniform(8, 130))
            score = rng.choice((round(rng.random(), 2), rng.random()))    # some ties
            dets.append((*b, score, c))
    rng.shuffle(dets)
    rng.shuffle(gts)
    return dets, gts


def heavy(rng):
    """The per-class row counts 0, 1, 100, 101, 130 and gt counts 0, 1, 64, 65, 130, crowds first, last, mixed."""
    return [rand_image(rng, (100, 1, 0, 3), (64, 1, 2, 0), 'first'),
            rand_image(rng, (101, 2, 0), (65, 0, 1), 'last'),
            rand_image(rng, (130, 5), (130, 3), 'mixed')]


def assemble(images, max_det):
    B = len(images)
    det = np.full((B, max_det, 6), np.nan, dtype=np.float32)
    count = np.zeros(B, dtype=np.int32)
    rows, off = [], [0]
    for b, (d, g) in enumerate(images):
        assert len(d) <= max_det
        if d:
            det[b, :len(d)] = np.array(d, dtype=np.float64)
        count[b] = len(d)
        rows += [tuple(float(v) for v in r) for r in g]
        off.append(len(rows))
    gts = np.array(rows, dtype=np.float64).reshape(-1, 7)
    return det, count, gts, np.array(off, dtype=np.int32)


def launch(det, count, gts, gt_off, rank_fill=-1):
    """-> (flags [B,max_det,4] uint32, rank [B,max_det] int32) on the host; checks guards and inputs."""
    B, max_det, _ = det.shape
    G = len(gts)
    d_det, d_cnt = torch.from_numpy(det).to(DEV), torch.from_numpy(count).to(DEV)
    d_gts, d_off = torch.from_numpy(gts).to(DEV), torch.from_numpy(gt_off).to(DEV)
    flags = torch.full((B + 2, max_det, 4), -1, dtype=torch.int32, device=DEV)
    # -1 is 0xFF in every byte; it is also a value the kernel writes, so the repeat launch fills with -2
    rank = torch.full((B + 2, max_det), rank_fill, dtype=torch.int32, device=DEV)
    lib = _lib.lib()
    nbytes = lib.yv7_coco_match_ws_bytes(B, max_det, G)
    ws = torch.full((nbytes + 16,), 0xFF, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 8 == 0
    rc = lib.yv7_coco_match(d_det.data_ptr(), d_cnt.data_ptr(), B, max_det, d_gts.data_ptr() if G else None,
                            d_off.data_ptr(), G, flags[1].data_ptr(), rank[1].data_ptr(), ws.data_ptr(), nbytes,
                            torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'yv7_coco_match')
    torch.cuda.synchronize()
    assert (flags[0] == -1).all() and (flags[-1] == -1).all() and (rank[0] == rank_fill).all() and (rank[-1] == rank_fill).all()
    assert (ws[nbytes:] == 0xFF).all()
    assert torch.equal(d_det.cpu().view(torch.int32), torch.from_numpy(det).view(torch.int32))
    assert torch.equal(d_gts.cpu(), torch.from_numpy(gts)) and torch.equal(d_cnt.cpu(), torch.from_numpy(count))
    return flags[1:-1].cpu(), rank[1:-1].cpu()


def check(images, max_det):
    det, count, gts, off = assemble(images, max_det)
    want_flags, want_rank = R.match_rows(det, count, gts, off)
    flags, rank = launch(det, count, gts, off)
    assert torch.equal(rank, torch.from_numpy(want_rank))
    assert torch.equal(flags, torch.from_numpy(want_flags.view(np.int32)))
    again_flags, again_rank = launch(det, count, gts, off, rank_fill=-2)
    assert torch.equal(again_flags, flags) and torch.equal(again_rank, rank)
    return flags, rank


def test_single_row():
    flags, rank = check(hand_worked()[:1], 1)
    assert rank.tolist() == [[0]]
    # matched at every threshold in every range; in medium and large the gt (area 400) is ignored, and so is its match
    assert [v & 0xFFFFFFFF for v in flags[0, 0].tolist()] == [0x3FF, 0x3FF, 0xFFFFF, 0xFFFFF]


def test_hand_worked_cases_three_images_at_a_time():
    cases = hand_worked()
    for i in range(0, len(cases) - 2, 3):
        check(cases[i:i + 3], 300)
    flags, rank = check(cases[4:7], 300)
    f = [[v & 0xFFFFFFFF for v in row] for row in flags[0, :3].tolist()]
    assert f[0][0] == 0x001 and f[1][0] == 0x001 and f[2][0] == 0x000    # IoU on 0.5, rounded onto it, rounded off it
    assert (flags[1, :2, 0] & 1).tolist() == [1, 1]                      # equal IoUs: the last gt, so both match
    assert flags[2, 0, 0].item() & 0xFFFFF == 0x3FF | (0x3F8 << 10)      # the break rule
    flags, rank = check(cases[7:8], 300)
    assert rank[0, :3].tolist() == [0, 1, 2] and (flags[0, :3, 0] & 1).tolist() == [0, 1, 0]


def test_descriptor_chunk_64_images_300_rows():
    rng = random.Random(11)
    images = hand_worked() + heavy(rng)
    images.append(rand_image(rng, (60, 70, 90, 80), (5, 0, 9, 3)))    # 300 rows: two passes of the row loop
    while len(images) < 64:
        images.append(rand_image(rng, [rng.randrange(0, 7) for _ in range(4)], [rng.randrange(0, 5) for _ in range(4)]))
    assert len(images) == 64 and len(images[16][0]) == 300
    flags, rank = check(images, 300)
    assert (rank >= 0).any() and (flags & 1).any() and ((flags >> 10) & 1).any()


def test_second_launch_65_images_450_rows():
    rng = random.Random(12)
    images = [rand_image(rng, [rng.randrange(0, 6) for _ in range(3)], [rng.randrange(0, 4) for _ in range(3)])
              for _ in range(62)]
    images.insert(5, ([], []))
    images.append(rand_image(rng, (120, 110, 100, 70, 50), (6, 2, 0, 70, 1), 'mixed'))   # 450 rows
    images.append(hand_worked()[2])                                     # image 64: the second launch's only one
    assert len(images) == 65 and len(images[63][0]) == 450
    flags, rank = check(images, 450)
    assert (rank[64, :4] >= 0).all() and (rank[63] == -1).sum() == 20 + 10    # rows past 100 in two classes


def test_counts_and_offsets_are_clamped():
    """A count beyond max_det or below 0 and offsets beyond G are clamped, as yv7_match does."""
    images = hand_worked()[:3]
    det, count, gts, off = assemble(images, 4)
    det[np.isnan(det)] = 0
    want_f, want_r = R.match_rows(det, np.array([1, 3, 4], np.int32), gts, off)
    count2 = np.array([1, 3, 900], dtype=np.int32)
    off2 = off.copy()
    off2[-1] = 1 << 20
    flags, rank = launch(det, count2, gts, off2)
    assert torch.equal(rank, torch.from_numpy(want_r)) and torch.equal(flags, torch.from_numpy(want_f.view(np.int32)))
    flags, rank = launch(det, np.array([-5, 3, 4], np.int32), gts, off)
    assert (rank[0] == -1).all() and (flags[0] == 0).all()


def test_argument_errors_return_negative_codes_and_launch_nothing():
    lib = _lib.lib()
    buf = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = buf.data_ptr()

    def call(B=1, max_det=1, G=0, det=p, count=p, gts=None, off=p, flags=p, rank=p, ws=p, ws_bytes=512):
        rc = lib.yv7_coco_match(det, count, B, max_det, gts, off, G, flags, rank, ws, ws_bytes, None)
        return rc, lib.yv7_last_error().decode()
    for kw, code in (({'B': 0}, -1), ({'max_det': -1}, -1), ({'G': -1}, -1), ({'G': 2}, -1), ({'det': None}, -1),
                     ({'count': None}, -1), ({'off': None}, -1), ({'flags': None}, -1), ({'rank': None}, -1),
                     ({'ws': None}, -1), ({'ws': p + 4}, -1), ({'ws_bytes': 8}, -3)):
        rc, msg = call(**kw)
        assert rc == code and msg.startswith('yv7_coco_match: '), (kw, rc, msg)
    torch.cuda.synchronize()
    assert (buf == 0).all()
