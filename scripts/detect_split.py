"""Where detect.py --batch-size 32 --save-img spends its wall time: decode, device work, encode + write
(profiles/draw/README.md).  32 copies of tests/golden/bus.jpg, yolov7 at 640, synthetic weights; the second of two
runs is reported.  decode = imread, encode = save_images past its one download (PIL's PNG/JPEG encoder and the file
write); loop = detect_batched; device = the rest of the loop (upload, letterbox, forward, NMS, scaling, drawing),
closed by a synchronize; total also holds building the model.

    python scripts/detect_split.py
"""
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'yolo-series_amd'))

import torch  # noqa: E402

import detect  # noqa: E402


def main():
    tmp = tempfile.mkdtemp()
    for ext in ('jpg', 'png'):
        src = os.path.join(tmp, f'src_{ext}')
        os.makedirs(src)
        from PIL import Image
        with Image.open(os.path.join(ROOT, 'tests', 'golden', 'bus.jpg')) as im:
            for i in range(32):
                im.save(os.path.join(src, f'{i:02d}.{ext}'))
        spent = {'decode': 0.0, 'encode': 0.0, 'download': 0.0, 'loop': 0.0}
        imread, cat = detect.imread, torch.cat

        def timed_imread(p):
            t0 = time.perf_counter()
            out = imread(p)
            spent['decode'] += time.perf_counter() - t0
            return out

        def timed_save(frames, paths, save_dir):
            t0 = time.perf_counter()
            flat = cat([f.reshape(-1) for f in frames]).cpu()
            t1 = time.perf_counter()
            spent['download'] += t1 - t0
            from pathlib import Path
            off = 0
            for f, path in zip(frames, paths):
                a = flat[off:off + f.numel()].numpy().reshape(tuple(f.shape))
                off += f.numel()
                Image.fromarray(a[:, :, ::-1]).save(save_dir / Path(path).name)
            spent['encode'] += time.perf_counter() - t1

        batched = detect.detect_batched

        def timed_loop(*a, **k):
            t0 = time.perf_counter()
            out = batched(*a, **k)
            torch.cuda.synchronize()
            spent['loop'] = time.perf_counter() - t0
            return out

        detect.imread, detect.save_images, detect.detect_batched = timed_imread, timed_save, timed_loop
        for run in range(2):
            for k in spent:
                spent[k] = 0.0
            opt = detect.parse_opt(['--cfg', 'yolov7', '--source', src, '--img-size', '640', '--batch-size', '32',
                                    '--save-img', '--quiet', '--project', tmp, '--name', f'out_{ext}_{run}'])
            t0 = time.perf_counter()
            res = detect.detect(opt)
            torch.cuda.synchronize()
            total = time.perf_counter() - t0
        detect.imread, detect.detect_batched = imread, batched
        boxes = sum(len(d) for _, d in res)
        device = spent['loop'] - spent['decode'] - spent['encode'] - spent['download']
        print(json.dumps({'format': ext, 'files': 32, 'boxes': boxes, 'total_s': round(total, 3),
                          'loop_s': round(spent['loop'], 3), 'decode_s': round(spent['decode'], 3),
                          'device_s': round(device, 3), 'download_s': round(spent['download'], 3),
                          'encode_write_s': round(spent['encode'], 3)}), flush=True)
    shutil.rmtree(tmp)


if __name__ == '__main__':
    main()
