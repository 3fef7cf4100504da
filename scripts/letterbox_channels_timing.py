"""Time the ragged letterbox per channel count on the device.

usage: python scripts/letterbox_channels_timing.py [--lib PATH/libyv7.so] [--label NAME]

Workload: 32 frames of 1080 x 810 onto a 640 x 640 canvas (autoShape's geometry: 480 x 640 resized, 80 columns of
border on each side), fp16 planes out.  One HIP event pair around each call; the figure is the median of 30 calls
after 10 warm-up calls, all in this process.  C = 1, 3, 4, 8 go through yv7_letterbox_ragged_c and C = 3 also
through yv7_letterbox_ragged; a library without the _c entry point (an older build given with --lib) reports the
latter alone.  Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, H, W, NH, NW, TOP, LEFT, S = 32, 1080, 810, 640, 480, 0, 80, 640
WARMUP, CALLS = 10, 30


class FrameDesc(ctypes.Structure):   # yv7_frame_desc
    _fields_ = [('data', ctypes.c_void_p), ('h', ctypes.c_int32), ('w', ctypes.c_int32), ('new_h', ctypes.c_int32),
                ('new_w', ctypes.c_int32), ('top', ctypes.c_int32), ('left', ctypes.c_int32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=os.path.join(ROOT, 'yolo-series_amd', 'yv7', 'libyv7.so'))
    ap.add_argument('--label', default='this')
    opt = ap.parse_args()
    lib = ctypes.CDLL(opt.lib)
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib.yv7_letterbox_ragged.argtypes = [ctypes.POINTER(FrameDesc), i, i, i, i, i, i, i, i, vp, vp, sz, vp]
    has_c = hasattr(lib, 'yv7_letterbox_ragged_c')
    if has_c:
        lib.yv7_letterbox_ragged_c.argtypes = [ctypes.POINTER(FrameDesc), i, i, i, i, ctypes.POINTER(ctypes.c_uint8), i,
                                               i, vp, vp, sz, vp]
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(0)

    def measure(C, old):
        src = torch.randint(0, 256, (B, H, W, C), dtype=torch.uint8, generator=gen).cuda()
        dst = torch.empty((B, C, S, S), dtype=torch.float16, device='cuda')
        descs = (FrameDesc * B)()
        for b, d in enumerate(descs):
            d.data, d.h, d.w, d.new_h, d.new_w, d.top, d.left = src[b].data_ptr(), H, W, NH, NW, TOP, LEFT
        pad = (ctypes.c_uint8 * C)(*([114] * C))

        def call():
            if old:
                rc = lib.yv7_letterbox_ragged(descs, B, S, S, 114, 114, 114, 0, 1, dst.data_ptr(), None, 0, stream)
            else:
                rc = lib.yv7_letterbox_ragged_c(descs, B, C, S, S, pad, 0, 1, dst.data_ptr(), None, 0, stream)
            assert rc == 0, rc
        for _ in range(WARMUP):
            call()
        torch.cuda.synchronize()
        times = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        return round(statistics.median(times), 2)

    out = {'label': opt.label, 'unit': 'us', 'frames': B, 'c3_ragged': measure(3, True)}
    if has_c:
        for C in (1, 3, 4, 8):
            out[f'c{C}_ragged_c'] = measure(C, False)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
