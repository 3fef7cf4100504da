"""TEST INFRASTRUCTURE ONLY — the letterbox of a C-channel frame on the CPU.

oracle/letterbox_ref.py's resize_linear_u8 is written for cn interleaved channels (its rounding split is
new_w * cn // 16 * 16 over the interleaved row) and its letterbox_geometry knows no channels; only its letterbox()
allocates a 3-channel canvas.  This helper joins the two with a per-channel canvas colour, and restates the float
conversion of the model input ((u8.float() / 255), and .half() of that: one rounding) without reordering channels.
"""
import numpy as np
import torch

from oracle import letterbox_ref as R


def place(img, new_wh, border, pad):
    """img [H, W, C] uint8 resized to new_wh = (w, h) (identity when it has that size) inside `border` =
    (top, bottom, left, right) of colour pad[c] -> uint8 [h + top + bottom, w + left + right, C]."""
    C = img.shape[2]
    pad = np.asarray(pad, np.uint8)
    assert pad.shape == (C,)
    if img.shape[1::-1] != tuple(new_wh):
        img = R.resize_linear_u8(img, new_wh[0], new_wh[1])
    top, bottom, left, right = border
    out = np.empty((img.shape[0] + top + bottom, img.shape[1] + left + right, C), np.uint8)
    out[...] = pad
    out[top:top + img.shape[0], left:left + img.shape[1]] = img
    return out


def letterbox(img, new_shape, pad, auto=False, scaleFill=False, scaleup=True, stride=32):
    """oracle.letterbox_ref.letterbox for [H, W, C] frames and a per-channel pad: (img, ratio, (dw, dh))."""
    new_unpad, ratio, dwdh, border = R.letterbox_geometry(img.shape[:2], new_shape, auto, scaleFill, scaleup, stride)
    return place(img, new_unpad, border, pad), ratio, dwdh


def to_planes(img_hwc, half=False):
    """uint8 [H, W, C] -> [C, H, W] float in [0, 1], channels in the frame's order; half: rounded once."""
    x = torch.from_numpy(np.ascontiguousarray(img_hwc.transpose(2, 0, 1))).float() / 255
    return x.half() if half else x


def output(img_hwc, out_kind):
    """What the library writes for out_kind 0 (uint8 HWC), 1 (fp16 planes), 2 (fp32 planes)."""
    return torch.from_numpy(img_hwc) if out_kind == 0 else to_planes(img_hwc, half=out_kind == 1)


def random_frame(h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)


def pads(c):
    """Distinct per channel, none 114."""
    return [(37 * k + 11) % 251 for k in range(c)]
