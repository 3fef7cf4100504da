"""Draw time, device against host (profiles/draw/README.md).

The device side is plot_boxes (yv7_draw_boxes: two launches per 64 images) on frames already on the device, timed with
device events around the call, warmed, the median of --iters runs.  The host alternative is what drawing on the CPU
would need from the same state: count.tolist() + det.cpu() + a PIL ImageDraw loop (rectangle, filled rectangle, text),
timed with a host clock on frames already on the host.  Both draw the same seeded boxes with name + conf labels.

    python scripts/draw_timing.py --iters 20
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'yolo-series_amd'))

from utils import plots  # noqa: E402


def boxes(rs, B, n, h, w):
    det = np.zeros((B, n, 6), np.float32)
    cx, cy = rs.rand(B, n) * w, rs.rand(B, n) * h
    bw, bh = rs.rand(B, n) * w * 0.4 + 8, rs.rand(B, n) * h * 0.4 + 8
    det[..., 0], det[..., 1] = np.clip(cx - bw / 2, 0, w), np.clip(cy - bh / 2, 0, h)
    det[..., 2], det[..., 3] = np.clip(cx + bw / 2, 0, w), np.clip(cy + bh / 2, 0, h)
    det[..., 4] = rs.rand(B, n)
    det[..., 5] = rs.randint(0, 80, (B, n))
    return det


def host_draw(frames, det, cnt, names, colors, t):
    from PIL import Image, ImageDraw, ImageFont
    counts, d = cnt.tolist(), det.cpu()
    font = ImageFont.load_default(plots.text_height(t) * 22 // 28)
    out = []
    for f, rows, c in zip(frames, d, counts):
        im = Image.fromarray(f)
        draw = ImageDraw.Draw(im)
        for x1, y1, x2, y2, conf, cls in rows[:c].tolist():
            col = colors[int(cls) % len(colors)]
            draw.rectangle([int(x1), int(y1), int(x2), int(y2)], outline=col, width=t)
            label = f'{names[int(cls)]} {conf:.2f}'
            tw = int(draw.textlength(label, font=font))
            draw.rectangle([int(x1), int(y1) - plots.text_height(t) - 3, int(x1) + tw, int(y1)], fill=col)
            draw.text((int(x1), int(y1) - plots.text_height(t) - 1), label, fill=(225, 255, 255), font=font)
        out.append(np.asarray(im))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32)
    opt = ap.parse_args()
    names = [f'class{i}' for i in range(80)]
    colors = plots.color_list()
    rs = np.random.RandomState(0)
    for h, w in ((1080, 810), (1920, 1080)):
        base = rs.randint(0, 256, (opt.batch, h, w, 3)).astype(np.uint8)
        t = plots.line_thickness((h, w))
        for n in (20, 300):
            det = torch.from_numpy(boxes(rs, opt.batch, n, h, w)).cuda()
            cnt = torch.full((opt.batch,), n, dtype=torch.int32).cuda()
            dev = torch.from_numpy(base).cuda()
            frames = list(dev.unbind(0))
            ms = []
            for it in range(opt.iters + 3):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                plots.plot_boxes(frames, det, cnt, names=names, colors=colors, line_thickness=t)
                b.record()
                b.synchronize()
                if it >= 3:
                    ms.append(a.elapsed_time(b))
            host_frames = [f for f in base]
            hs = []
            for it in range(3):
                t0 = time.perf_counter()
                host_draw(host_frames, det, cnt, names, colors, t)
                hs.append((time.perf_counter() - t0) * 1e3)
            painted = float((dev.cpu().numpy() != base).any(axis=3).mean())
            print(json.dumps({'frames': opt.batch, 'h': h, 'w': w, 'boxes': n, 't': t,
                              'device_ms_median': round(float(np.median(ms)), 4),
                              'device_ms_min': round(min(ms), 4), 'device_ms_max': round(max(ms), 4),
                              'host_ms_median': round(float(np.median(hs)), 1), 'painted_fraction': round(painted, 4)}),
                  flush=True)


if __name__ == '__main__':
    main()
