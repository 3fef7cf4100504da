"""Device time of the two picture grids of one batch (yolov7 640^2, bs 32: 16 tiles, up to 4800 rows) against the
numpy restatement's wall time on the host (profiles/mosaic/mosaic_device.json).

    python scripts/mosaic_timing.py [OUT.json]
"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'yolo-series_amd'), ROOT, os.path.join(ROOT, 'tests')]
import numpy as np
import torch
from utils import plots
import mosaic_ref as M

rs = np.random.RandomState(0)
B, H, W, max_det, nc = 32, 640, 640, 300, 80
names = [f'class{i:02d}' for i in range(nc)]
images = rs.rand(B, 3, H, W).astype(np.float16)
det = np.zeros((B, max_det, 6), np.float32)
x1 = rs.rand(B, max_det) * (W - 40); y1 = rs.rand(B, max_det) * (H - 40)
det[..., 0], det[..., 1] = x1, y1
det[..., 2] = x1 + 10 + rs.rand(B, max_det) * 200
det[..., 3] = y1 + 10 + rs.rand(B, max_det) * 200
det[..., 4] = rs.rand(B, max_det)            # conf 0.001 output: most rows are below 0.25
det[..., 5] = rs.randint(0, nc, (B, max_det))
det_all = det.copy(); det_all[..., 4] = 0.26 + 0.7 * det[..., 4]   # worst case: all 4800 rows drawn
count = np.full(B, max_det, np.int32)
per = rs.randint(3, 12, B)
t = np.zeros((per.sum(), 6), np.float32)
t[:, 0] = np.repeat(np.arange(B), per); t[:, 1] = rs.randint(0, nc, len(t))
t[:, 2:4] = rs.rand(len(t), 2); t[:, 4:6] = rs.rand(len(t), 2) * 0.4
off = np.concatenate(([0], np.cumsum(per))).astype(np.int32)
paths = [f'/data/coco/images/val2017/{i:012d}.jpg' for i in range(B)]

d_img = torch.from_numpy(images).cuda()
d_u8 = (d_img.float() * 255).to(torch.uint8)
d_det, d_all, d_cnt = torch.from_numpy(det).cuda(), torch.from_numpy(det_all).cuda(), torch.from_numpy(count).cuda()
d_t, d_off = torch.from_numpy(t).cuda(), torch.from_numpy(off).cuda()

def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        out.append(a.elapsed_time(b) * 1000)
    out.sort()
    return dict(median_us=round(out[len(out) // 2], 1), min_us=round(out[0], 1), max_us=round(out[-1], 1))

class _R(dict):
    def __setitem__(self, k, v):
        print(k, v, flush=True); dict.__setitem__(self, k, v)
res = _R()
res['tiles_only_fp16'] = timed(lambda: plots.plot_images(d_img, None, None, None, names))
res['tiles_captions_fp16'] = timed(lambda: plots.plot_images(d_img, None, paths, None, names))
res['labels_fp16'] = timed(lambda: plots.plot_images(d_img, d_t, paths, None, names, label_off=d_off))
res['pred_conf_uniform_fp16'] = timed(lambda: plots.plot_images(d_img, (d_det, d_cnt), paths, None, names))
res['pred_all_4800_drawn_fp16'] = timed(lambda: plots.plot_images(d_img, (d_all, d_cnt), paths, None, names))
res['pred_all_4800_drawn_u8'] = timed(lambda: plots.plot_images(d_u8, (d_all, d_cnt), paths, None, names))
both = lambda: (plots.plot_images(d_img, d_t, paths, None, names, label_off=d_off),
                plots.plot_images(d_img, (d_det, d_cnt), paths, None, names))
res['both_pictures_fp16'] = timed(both)
both_all = lambda: (plots.plot_images(d_img, d_t, paths, None, names, label_off=d_off),
                    plots.plot_images(d_img, (d_all, d_cnt), paths, None, names))
res['both_pictures_all_drawn_fp16'] = timed(both_all)
# the call's host side (no sync inside): wall time of enqueueing both
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(20):
    both()
res['both_pictures_host_enqueue_ms'] = round((time.perf_counter() - t0) / 20 * 1000, 3); torch.cuda.synchronize()
# pinned copies of both 1280 x 1280 pictures
pics = both(); hosts = [torch.empty(p.shape, dtype=torch.uint8, pin_memory=True) for p in pics]
res['two_pinned_copies'] = timed(lambda: [h.copy_(p, non_blocking=True) for h, p in zip(hosts, pics)])

# the restatement on the host, same two pictures
g = plots.mosaic_geometry(B, H, W)
atlas = plots.glyph_atlas_host(plots.text_height(3)); raw = [n.encode() for n in names]
caps = [os.path.basename(p)[:40].encode() for p in paths[:g['n']]]
def host(det_, **kw):
    return M.mosaic(images, g['n'], g['ns'], *g['tile'], g['sf'], *g['out'], palette=plots.color_list(), names=raw,
                    atlas=atlas, captions=caps, **kw)
t0 = time.perf_counter(); lab = host(None, targets=t, label_off=off, normalized=True); t1 = time.perf_counter()
pred = host(None, det=det, count=count); t2 = time.perf_counter()
pred_all = host(None, det=det_all, count=count); t3 = time.perf_counter()
res['host_restatement_s'] = dict(labels=round(t1 - t0, 3), pred=round(t2 - t1, 3), pred_all_drawn=round(t3 - t2, 3))
res['equal_to_restatement'] = bool(np.array_equal(pics[0].cpu().numpy(), lab) and np.array_equal(pics[1].cpu().numpy(), pred)
                                   and np.array_equal(plots.plot_images(d_img, (d_all, d_cnt), paths, None, names).cpu().numpy(), pred_all))
res['rows_drawn'] = dict(pred=int(len(M.pred_rows(det, count, 16, 4, 640, 640, 1.0))), labels=int(off[16]))
from PIL import Image; import io
t0 = time.perf_counter(); buf = io.BytesIO(); Image.fromarray(pred).save(buf, 'JPEG'); res['jpeg_encode_ms'] = round((time.perf_counter() - t0) * 1000, 1)
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        json.dump(res, f, indent=1)
print(json.dumps(res, indent=1))
