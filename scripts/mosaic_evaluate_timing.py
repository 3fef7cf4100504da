"""test() per-batch host time on one checkout of this repository (profiles/mosaic/evaluate_*.json): 8 batches of 32
noise images at 640^2, yolov7 with synthetic weights, conf 0.001, plots on, a real save_dir; three runs in the
process, the first one warms up.  Run it on two checkouts in turn to compare them.

    python scripts/mosaic_evaluate_timing.py TREE TAG [OUT.json]
"""
import contextlib, io, json, os, sys, tempfile, time
TREE, TAG = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path[:0] = [os.path.join(TREE, 'yolo-series_amd'), TREE]
import numpy as np
import torch
import test as T
from models.yolo import Model
from yv7.synthetic import synthetic_state_dict

m = Model('yolov7'); synthetic_state_dict(m, seed=0)
model = m.float().fuse().eval().to('cuda:0')
rs = np.random.RandomState(0)
NB, B = 8, 32
batches = []
for k in range(NB):
    img = torch.from_numpy(rs.randint(0, 256, (B, 3, 640, 640)).astype(np.uint8)).pin_memory()
    per = rs.randint(3, 12, B)
    t = np.zeros((per.sum(), 6), np.float32)
    t[:, 0] = np.repeat(np.arange(B), per); t[:, 1] = rs.randint(0, 80, len(t))
    t[:, 2:4] = rs.rand(len(t), 2) * 0.6 + 0.2; t[:, 4:6] = rs.rand(len(t), 2) * 0.3 + 0.05
    paths = [f'/data/images/{k * B + i:012d}.jpg' for i in range(B)]
    shapes = [((640, 640), ((1.0, 1.0), (0.0, 0.0)))] * B
    batches.append((img, torch.from_numpy(t).pin_memory(), paths, shapes))

class Loader:
    def __init__(self): self.t = []
    def __len__(self): return NB
    def __iter__(self):
        for b in batches:
            self.t.append(time.perf_counter()); yield b
        self.t.append(time.perf_counter())

data = {'nc': 80, 'val': '/nonexistent', 'names': [str(i) for i in range(80)]}
T.check_dataset = lambda d: None
out = {'tag': TAG, 'runs': []}
for rep in range(3):
    with tempfile.TemporaryDirectory() as d:
        ld = Loader(); torch.cuda.synchronize(); t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            res = T.test(data, batch_size=B, imgsz=640, conf_thres=0.001, iou_thres=0.6, model=model, dataloader=ld,
                         save_dir=d, plots=True)
        total = time.perf_counter() - t0
        steps = [round((b - a) * 1000, 2) for a, b in zip(ld.t, ld.t[1:])]
        out['runs'].append(dict(total_s=round(total, 3), step_ms=steps, files=sorted(os.listdir(d)), map50=float(res[0][2])))
print(json.dumps(out))
if len(sys.argv) > 3:
    with open(sys.argv[3], 'w') as f:
        json.dump(out, f)
