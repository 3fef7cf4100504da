"""Frame pre-processing on the GPU — the reference's letterbox() and detect.py's input conversion.

`letterbox(img, new_shape, color, auto, scaleFill, scaleup, stride)` keeps the signature and return
value of utils/datasets.py:1277-1307 ((img, ratio, (dw, dh)); img HWC BGR uint8) with the resize and
border done by libyv7 (yv7_letterbox: cv2.resize INTER_LINEAR restated bit for bit in fixed point,
see csrc/preprocess.hip).  `letterbox_batch(frames, img_size, half, ...)` fuses it with detect.py's
conversion (img[:, :, ::-1].transpose(2, 0, 1), .half()/.float(), /= 255, detect.py:100-104) and
writes the [B, 3, S, S] model input in one launch; `letterbox_ragged(frames, geoms, canvas, ...)` does
so for frames of different sizes (yv7_letterbox_ragged), with `autoshape_geometry` supplying autoShape's
inference shape and per-frame geometry (models/common.py:909-915).  There is no CPU path: inputs go to the current
HIP device and the library must be built (the ctypes binding raises otherwise).

`create_dataloader` / `LoadImagesAndLabels` restate the non-augmented path of the reference's validation loader
(utils/datasets.py:68-96, 352-490, 826-929, 959-971) for the plain images/ + labels/*.txt layout: the image
list, label files, rectangular batch shapes, per-image geometry, label transform and `shapes` are the
reference's; the pixels are decoded on the host and written onto the batch's canvas by one letterbox_ragged call.
"""
from __future__ import annotations

import ctypes
import glob
import os
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from utils.general import check_three_channels, input_channels, make_divisible, scale_desc
from yv7 import _lib as L

OUT_U8_HWC, OUT_F16_CHW, OUT_F32_CHW = 0, 1, 2
MAX_CHANNELS = 16   # YV7_LETTERBOX_MAX_CH


def letterbox_geometry(shape, new_shape=(640, 640), auto=True, scaleFill=False, scaleup=True, stride=32):
    """datasets.py:1279-1305 for a frame of `shape` (h, w): new_unpad (w, h), ratio, (dw, dh) and the
    integer border (top, bottom, left, right) cv2.copyMakeBorder receives."""
    if isinstance(new_shape, int):
        new_shape = (new_shape, new_shape)
    r = min(new_shape[0] / shape[0], new_shape[1] / shape[1])
    if not scaleup:   # only scale down (better test mAP)
        r = min(r, 1.0)
    ratio = r, r
    new_unpad = int(round(shape[1] * r)), int(round(shape[0] * r))
    dw, dh = new_shape[1] - new_unpad[0], new_shape[0] - new_unpad[1]
    if auto:   # minimum rectangle
        dw, dh = np.mod(dw, stride), np.mod(dh, stride)
    elif scaleFill:   # stretch
        dw, dh = 0.0, 0.0
        new_unpad = (new_shape[1], new_shape[0])
        ratio = new_shape[1] / shape[1], new_shape[0] / shape[0]
    dw /= 2
    dh /= 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return new_unpad, ratio, (dw, dh), (top, bottom, left, right)


def pad_colour(color, C):
    """The canvas colour of a C-channel frame as C ints: a scalar, a length-C sequence, or the 3-tuple default
    (114, 114, 114), which means 114 in every channel."""
    c = [int(color)] * C if np.isscalar(color) else [int(v) for v in color]
    if len(c) != C and c == [114, 114, 114]:
        c = [114] * C
    if len(c) != C or any(v < 0 or v > 255 for v in c):
        raise ValueError(f'letterbox: color must be a scalar or {C} values in 0..255, got {color}')
    return c


def _pad_bytes(c):
    return (ctypes.c_uint8 * len(c))(*c)


def _run(frames: torch.Tensor, geom, color, out_kind):
    """frames: uint8 [B, H, W, C] on a HIP device -> letterboxed output of `out_kind`.  Three channels are BGR and
    their float planes come out RGB (yv7_letterbox); any other count keeps its order (yv7_letterbox_c)."""
    if not frames.is_cuda:
        raise RuntimeError('letterbox: frames must be on a HIP device (there is no CPU path)')
    if frames.dtype != torch.uint8 or frames.dim() != 4 or not 1 <= frames.shape[-1] <= MAX_CHANNELS:
        raise ValueError(f'letterbox: expected uint8 [B, H, W, C] frames of 1..{MAX_CHANNELS} channels (3: BGR), '
                         f'got {frames.dtype} {tuple(frames.shape)}')
    if frames.shape[-1] != 3:
        return _run_c(frames.contiguous(), geom, pad_colour(color, frames.shape[-1]), out_kind)
    frames = frames.contiguous()
    B, H, W, _ = frames.shape
    (nw, nh), _, _, (top, bottom, left, right) = geom
    oh, ow = nh + top + bottom, nw + left + right
    dev = frames.device
    if out_kind == OUT_U8_HWC:
        out = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=dev)
    else:
        out = torch.empty((B, 3, oh, ow), dtype=torch.float16 if out_kind == OUT_F16_CHW else torch.float32,
                          device=dev)
    lib = L.lib()
    ws = torch.empty(int(lib.yv7_letterbox_workspace_bytes(nh, nw)), dtype=torch.uint8, device=dev)
    c = [int(v) for v in color]
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.yv7_letterbox(frames.data_ptr(), B, H, W, nh, nw, top, left, oh, ow, c[0], c[1], c[2], out_kind,
                                  out.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'yv7_letterbox')
    return out


def _run_c(frames, geom, c, out_kind):
    B, H, W, C = frames.shape
    (nw, nh), _, _, (top, bottom, left, right) = geom
    oh, ow = nh + top + bottom, nw + left + right
    dev = frames.device
    if out_kind == OUT_U8_HWC:
        out = torch.empty((B, oh, ow, C), dtype=torch.uint8, device=dev)
    else:
        out = torch.empty((B, C, oh, ow), dtype=torch.float16 if out_kind == OUT_F16_CHW else torch.float32,
                          device=dev)
    lib = L.lib()
    ws = torch.empty(int(lib.yv7_letterbox_workspace_bytes(nh, nw)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(lib.yv7_letterbox_c(frames.data_ptr(), B, H, W, C, nh, nw, top, left, oh, ow, _pad_bytes(c), 0,
                                    out_kind, out.data_ptr(), ws.data_ptr(), ws.numel(), stream), 'yv7_letterbox_c')
    return out


def letterbox(img, new_shape=(640, 640), color=(114, 114, 114), auto=True, scaleFill=False, scaleup=True, stride=32):
    """utils/datasets.py:1277-1307: resize and pad an HWC uint8 frame (numpy array or HIP tensor) of 1..16 channels
    (3: BGR).  color: a scalar or one value per channel; the default is 114 in every channel.
    Returns (img, ratio, (dw, dh)); img has the input's type (numpy in -> numpy out)."""
    as_numpy = isinstance(img, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(img)).to(f'cuda:{torch.cuda.current_device()}') if as_numpy else img
    if t.dim() != 3:
        raise ValueError(f'letterbox: expected an HWC frame, got shape {tuple(t.shape)}')
    geom = letterbox_geometry(tuple(t.shape[:2]), new_shape, auto, scaleFill, scaleup, stride)
    out = _run(t[None], geom, color, OUT_U8_HWC)[0]
    return (out.cpu().numpy() if as_numpy else out), geom[1], geom[2]


def letterbox_batch(frames, img_size=640, half=True, color=(114, 114, 114), auto=False, scaleFill=False,
                    scaleup=True, stride=32):
    """LoadImages (datasets.py:196-200) + detect.py:100-104 for a batch of same-size frames:
    uint8 [B, H, W, 3] BGR (HIP tensor) -> ([B, 3, S, S] half/float RGB in [0, 1], ratio, (dw, dh)).
    detect.py's loader letterboxes with auto=False (datasets.py:196), the default here.
    [B, H, W, C] frames of another channel count give [B, C, S, S] in the frames' channel order."""
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames)).to(f'cuda:{torch.cuda.current_device()}')
    if frames.dim() == 3:
        frames = frames[None]
    geom = letterbox_geometry(tuple(frames.shape[1:3]), img_size, auto, scaleFill, scaleup, stride)
    x = _run(frames, geom, color, OUT_F16_CHW if half else OUT_F32_CHW)
    return x, geom[1], geom[2]


def autoshape_geometry(shapes, size=640, stride=32):
    """autoShape's shapes (common.py:909-915) for frames of `shapes` [(h, w), ...]: the common inference
    shape shape1 = [h1, w1] (every frame scaled so its longer side is `size`, the per-axis maximum rounded
    up to `stride` — in Python floats, whose rounding is part of the result: 147 * (640 / 147) > 640), each
    frame's letterbox_geometry(shape, shape1, auto=False) and each frame's scale_desc(shape1, shape)."""
    shape1 = [[y * (size / max(s)) for y in s] for s in shapes]
    shape1 = [make_divisible(max(s[k] for s in shape1), int(stride)) for k in (0, 1)]
    geoms = [letterbox_geometry(tuple(s), shape1, auto=False) for s in shapes]
    return shape1, geoms, [scale_desc(shape1, s) for s in shapes]


def _hip_device(device):
    device = torch.device(device)
    return torch.device('cuda', torch.cuda.current_device()) if device.index is None else device


def pack_frames(frames, device):
    """A list of uint8 HWC frames (numpy arrays or HIP tensors) -> (device pointers, the tensors behind
    them).  Host frames travel in one packed buffer, one host-to-device copy; HIP tensors are used in place."""
    host = [(i, np.ascontiguousarray(f)) for i, f in enumerate(frames) if isinstance(f, np.ndarray)]
    ptrs, keep = [None] * len(frames), []
    if host:
        packed = torch.from_numpy(np.concatenate([f.reshape(-1) for _, f in host])).to(device)
        keep.append(packed)
        off = 0
        for i, f in host:
            ptrs[i] = packed.data_ptr() + off
            off += f.size
    for i, f in enumerate(frames):
        if isinstance(f, torch.Tensor):
            if f.device != device:
                raise RuntimeError(f'letterbox_ragged: tensor frames must be on {device}, got {f.device}')
            f = f.contiguous()
            keep.append(f)
            ptrs[i] = f.data_ptr()
    return ptrs, keep


def letterbox_ragged(frames, geoms, canvas, color=(114, 114, 114), swap_rb=False, out_kind=OUT_F32_CHW,
                     device=None):
    """One yv7_letterbox_ragged call: frames (uint8 HWC numpy arrays or HIP tensors, any sizes) with their
    letterbox_geometry results onto a canvas (h, w) -> [B, h, w, C] uint8 or [B, C, h, w] half / float in
    [0, 1], C = the frames' channel count, 1..16.  color is in the frames' channel order (a scalar, C values, or
    the default: 114 everywhere); swap_rb reverses the channel order of the float outputs of 3-channel frames and
    is ignored for other counts.  Three channels go through yv7_letterbox_ragged, others through its _c form."""
    device = _hip_device(device if device is not None else 'cuda')
    C = frames[0].shape[2] if len(frames) and frames[0].ndim == 3 else 3
    for f in frames:
        u8 = f.dtype == (torch.uint8 if isinstance(f, torch.Tensor) else np.uint8)
        if not u8 or f.ndim != 3 or f.shape[2] != C or not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f'letterbox_ragged: expected uint8 [H, W, {C}] frames of 1..{MAX_CHANNELS} channels, '
                             f'got {f.dtype} {tuple(f.shape)}')
    B, (oh, ow) = len(frames), canvas
    ptrs, keep = pack_frames(frames, device)   # `keep` lives until the launch below is enqueued on the stream
    descs = (L.FrameDesc * B)()
    for d, p, f, ((nw, nh), _, _, (top, _, left, _)) in zip(descs, ptrs, frames, geoms):
        d.data, d.h, d.w, d.new_h, d.new_w, d.top, d.left = p, f.shape[0], f.shape[1], nh, nw, top, left
    if out_kind == OUT_U8_HWC:
        out = torch.empty((B, oh, ow, C), dtype=torch.uint8, device=device)
    else:
        out = torch.empty((B, C, oh, ow), dtype=torch.float16 if out_kind == OUT_F16_CHW else torch.float32,
                          device=device)
    c = [int(v) for v in color] if C == 3 else pad_colour(color, C)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        if C == 3:
            L.check(L.lib().yv7_letterbox_ragged(descs, B, oh, ow, c[0], c[1], c[2], int(bool(swap_rb)), out_kind,
                                                 out.data_ptr(), None, 0, stream), 'yv7_letterbox_ragged')
        else:
            L.check(L.lib().yv7_letterbox_ragged_c(descs, B, C, oh, ow, _pad_bytes(c), 0, out_kind, out.data_ptr(),
                                                   None, 0, stream), 'yv7_letterbox_ragged_c')
    return out


# ------------------------------------------------------------------------------------------ images
IMG_FORMATS = ('bmp', 'jpg', 'jpeg', 'png', 'tif', 'tiff', 'webp', 'mpo')


# How a file or an array becomes a C-channel frame, stated by the caller (a loader cannot know whether a 1-channel
# model wants PIL's luma of an RGB JPEG or the raw band of a thermal PNG): a PIL convert() target, or 'raw' for the
# file's own 8-bit bands / a .npy uint8 array.  None everywhere means today's 3-channel behaviour.
FRAME_MODES = ('L', 'LA', 'RGB', 'RGBA', 'raw')
_RAW_PIL_MODES = ('L', 'LA', 'RGB', 'RGBA', 'CMYK', 'YCbCr')   # PIL modes whose bands are 8-bit samples


def frame_channels(mode):
    """Bands of a PIL frame mode; None for 'raw' (the file decides)."""
    if mode not in FRAME_MODES:
        raise ValueError(f'frames must be one of {FRAME_MODES}, got {mode!r}')
    return {'L': 1, 'LA': 2, 'RGB': 3, 'RGBA': 4, 'raw': None}[mode]


def check_frame_mode(mode, ch):
    """A frame mode against a model's input channels: ValueError on a mismatch."""
    n = frame_channels(mode)
    if (n is not None and n != ch) or not 1 <= ch <= MAX_CHANNELS:
        raise ValueError(f"frames={mode!r} gives {n if n is not None else f'1..{MAX_CHANNELS}'}-channel frames, "
                         f'the model takes {ch}')


def entry_channels(model, frames):
    """The channel count an image entry point (autoShape, detect.py, test.py's loader) feeds `model` with.  With no
    frame mode stated it loads 3-channel images and refuses any other model, as ever; with one, the mode's band
    count must be the model's (ValueError otherwise)."""
    if frames is None:
        check_three_channels(model)
        return 3
    ch = input_channels(model)
    check_frame_mode(frames, ch)
    return ch


def _is_npy(path):
    return str(path).lower().endswith('.npy')


def imread(path, mode=None):
    """cv2.imread(path) (BGR uint8 HWC) substitute: cv2 is absent from this image, frames are decoded by
    PIL.  JPEG decoders may differ from cv2's libjpeg by +-1 per channel (decode parity unpinned);
    everything after the decode (letterbox, model, NMS) is the path under test.
    mode (FRAME_MODES): a PIL mode returns im.convert(mode)'s bands in PIL's order as [H, W, C]; 'raw' returns the
    file's own 8-bit bands unconverted, or a .npy file's uint8 [H, W, C] / [H, W] array.  Anything else (16-bit,
    palette, float data) raises ValueError naming the file and what it holds."""
    from PIL import Image
    if mode is None:
        with Image.open(path) as im:
            rgb = np.asarray(im.convert('RGB'))
        return np.ascontiguousarray(rgb[:, :, ::-1])
    frame_channels(mode)
    if _is_npy(path):
        if mode != 'raw':
            raise ValueError(f"{path}: a .npy array is read with frames='raw' only, not {mode!r}")
        a = np.load(path, allow_pickle=False)
        if a.dtype != np.uint8 or a.ndim not in (2, 3):
            raise ValueError(f'{path}: holds a {a.dtype} array of shape {a.shape}; expected uint8 [H, W, C] or [H, W]')
    else:
        with Image.open(path) as im:
            if mode == 'raw' and im.mode not in _RAW_PIL_MODES:
                raise ValueError(f"{path}: holds mode {im.mode!r} data; frames='raw' reads 8-bit bands "
                                 f'{_RAW_PIL_MODES} only')
            a = np.asarray(im if mode == 'raw' else im.convert(mode))
    return np.array(a, dtype=np.uint8).reshape(a.shape[0], a.shape[1], -1)   # an own, writable copy


def read_frame(path, frames, channels):
    """imread for a loader: the BGR frame for frames None / 'RGB', else imread(path, frames) checked against the
    model's channel count."""
    if frames in (None, 'RGB'):
        return imread(path)
    img = imread(path, frames)
    if channels is not None and img.shape[2] != channels:
        raise ValueError(f'{path}: holds {img.shape[2]}-channel frames, the model takes {channels}')
    return img


def _formats(frames):
    return IMG_FORMATS + ('npy',) if frames == 'raw' else IMG_FORMATS


class LoadImages:
    """utils/datasets.py:133-202 for image files (a file, a directory or a glob): yields
    (path, img CHW RGB uint8 letterboxed, img0 HWC BGR, None, ratio, (dw, dh)) like the reference, with
    the letterbox done on the current HIP device (auto=False, as datasets.py:196).
    frames (FRAME_MODES) other than None / 'RGB': img is [C, S, S] and img0 [H, W, C], both in the frame's own
    channel order; channels is the model's count, checked per file; 'raw' also lists .npy files."""

    def __init__(self, path, img_size=640, stride=32, frames=None, channels=None):
        import glob
        import os
        p = str(os.path.abspath(path))
        if '*' in p:
            files = sorted(glob.glob(p, recursive=True))
        elif os.path.isdir(p):
            files = sorted(glob.glob(os.path.join(p, '*.*')))
        elif os.path.isfile(p):
            files = [p]
        else:
            raise Exception(f'ERROR: {p} does not exist')
        if frames is not None:
            frame_channels(frames)
        self.frames, self.channels = frames, channels
        self.files = [x for x in files if x.split('.')[-1].lower() in _formats(frames)]
        self.img_size, self.stride, self.mode, self.cap = img_size, stride, 'image', None
        self.nf = len(self.files)
        assert self.nf > 0, f'No images found in {p}. Supported formats are: {IMG_FORMATS}'

    def __iter__(self):
        self.count = 0
        return self

    def __next__(self):
        if self.count == self.nf:
            raise StopIteration
        path = self.files[self.count]
        self.count += 1
        img0 = read_frame(path, self.frames, self.channels)
        img, ratio, dwdh = letterbox(img0, new_shape=(self.img_size, self.img_size), auto=False)
        if self.frames in (None, 'RGB'):
            img = img[:, :, ::-1]   # BGR to RGB
        img = np.ascontiguousarray(img.transpose(2, 0, 1))   # C x S x S
        return path, img, img0, self.cap, ratio, dwdh

    def __len__(self):
        return self.nf


# ------------------------------------------------------------------------------------------ validation set
LOADER_WORKERS = 8     # host decode threads: a fixed default, never sized from the machine's CPU count


def img2label_paths(img_paths):
    """datasets.py:352-355: .../images/x.jpg -> .../labels/x.txt (the first /images/ and the last extension)."""
    sa, sb = os.sep + 'images' + os.sep, os.sep + 'labels' + os.sep
    out = []
    for p in img_paths:
        q = p.replace(sa, sb, 1)
        out.append('txt'.join(q.rsplit(q.split('.')[-1], 1)))
    return out


def read_label_file(path):
    """datasets.py:612-631 for one label file: fp32 [n, 5] rows (cls, x, y, w, h), normalised.  A missing or
    empty file is an empty label set; a malformed row raises ValueError naming the file (the reference drops the
    image with a warning); duplicate rows are dropped, the first of each staying in file order."""
    if not os.path.isfile(path):
        return np.zeros((0, 5), dtype=np.float32)
    with open(path) as f:
        rows = [ln.split() for ln in f.read().strip().splitlines()]
    if not rows:
        return np.zeros((0, 5), dtype=np.float32)
    if any(len(r) != 5 for r in rows):
        raise ValueError(f'{path}: labels require 5 columns each')
    try:
        l = np.array(rows, dtype=np.float32)
    except ValueError as e:
        raise ValueError(f'{path}: {e}') from None
    if not (l >= 0).all():       # a NaN fails this too
        raise ValueError(f'{path}: negative labels')
    if not (l[:, 1:] <= 1).all():
        raise ValueError(f'{path}: non-normalized or out of bounds coordinate labels')
    _, first = np.unique(l, axis=0, return_index=True)
    return l[np.sort(first)]


def list_images(path, prefix='', formats=IMG_FORMATS):
    """datasets.py:383-398: the sorted image files under a directory (recursively), or named by a .txt list whose
    './' entries are relative to the list; several of either as a list."""
    f = []
    for p in path if isinstance(path, (list, tuple)) else [path]:
        p = Path(p)
        if p.is_dir():
            f += glob.glob(str(p / '**' / '*.*'), recursive=True)
        elif p.is_file():
            parent = str(p.parent) + os.sep
            with open(p) as t:
                f += [parent + x[2:] if x.startswith('./') else x for x in t.read().strip().splitlines()]
        else:
            raise Exception(f'{prefix}Error loading data from {path}: {p} does not exist')
    files = sorted(x.replace('/', os.sep) for x in f if x.split('.')[-1].lower() in formats)
    assert files, f'{prefix}No images found in {path}'
    return files


def image_size(path):
    """(w, h) from the file's header, without decoding: the size imread() returns (EXIF orientation is not applied
    by either).  A .npy file's comes from its header too; the array is not loaded."""
    if _is_npy(path):
        with open(path, 'rb') as f:
            major, _ = np.lib.format.read_magic(f)
            read = np.lib.format.read_array_header_1_0 if major == 1 else np.lib.format.read_array_header_2_0
            shape = read(f)[0]
        if len(shape) not in (2, 3):
            raise ValueError(f'{path}: holds an array of shape {shape}; expected [H, W, C] or [H, W]')
        return shape[1], shape[0]
    from PIL import Image
    with Image.open(path) as im:
        return im.size


class LoadImagesAndLabels:
    """The reference's LoadImagesAndLabels (datasets.py:358-958) without augmentation, mosaic, label cache,
    segments or its CrowdHuman / SHEL modes.  Holds, per image in evaluation order: img_files, label_files,
    labels (fp32 [n, 5], normalised to the image) and shapes ((w, h), float64); with rect, batch_shapes (h, w).
    frames (FRAME_MODES) / channels: how files become frames and the model's channel count, as LoadImages."""

    def __init__(self, path, img_size=640, batch_size=16, augment=False, hyp=None, rect=False, cache_images=False,
                 single_cls=False, stride=32, pad=0.0, prefix='', frames=None, channels=None):
        if augment:
            raise NotImplementedError('augmented loading (training) is not part of the MI355X inference path')
        if frames is not None:
            frame_channels(frames)
        self.frames, self.channels = frames, channels
        self.img_size, self.augment, self.hyp, self.rect, self.stride, self.path = img_size, False, hyp, rect, stride, path
        self.img_files = list_images(path, prefix, _formats(frames))
        self.label_files = img2label_paths(self.img_files)
        self.labels = [read_label_file(f) for f in self.label_files]
        self.shapes = np.array([image_size(f) for f in self.img_files], dtype=np.float64)   # wh
        if single_cls:       # datasets.py:452-454
            for x in self.labels:
                x[:, 0] = 0
        n = len(self.img_files)
        bi = np.floor(np.arange(n) / batch_size).astype(int)     # batch index of image, datasets.py:460-464
        nb = bi[-1] + 1
        self.batch, self.n, self.indices, self.batch_size = bi, n, range(n), batch_size
        if rect:             # datasets.py:467-490
            ar = self.shapes[:, 1] / self.shapes[:, 0]           # h / w
            irect = ar.argsort()
            self.img_files = [self.img_files[i] for i in irect]
            self.label_files = [self.label_files[i] for i in irect]
            self.labels = [self.labels[i] for i in irect]
            self.shapes = self.shapes[irect]
            ar = ar[irect]
            shapes = [[1, 1]] * nb
            for i in range(nb):
                ari = ar[bi == i]
                mini, maxi = ari.min(), ari.max()
                if maxi < 1:
                    shapes[i] = [maxi, 1]
                elif mini > 1:
                    shapes[i] = [1, 1 / mini]
            self.batch_shapes = np.ceil(np.array(shapes) * img_size / stride + pad).astype(int) * stride
        self.imgs = [None] * n   # decoded frames stay here when cache_images
        self.cache_images = bool(cache_images)

    def __len__(self):
        return self.n

    def canvas(self, index):
        """(h, w) of the letterboxed batch image `index` lands in (datasets.py:854)."""
        if self.rect:
            return tuple(int(v) for v in self.batch_shapes[self.batch[index]])
        return (self.img_size, self.img_size)

    def geometry(self, index):
        """load_image's sizes (datasets.py:966-971) followed by letterbox(auto=False, scaleup=False)
        (datasets.py:855, 1277-1307): ((h0, w0), (h, w), letterbox_geometry of (h, w) on the canvas)."""
        w0, h0 = (int(v) for v in self.shapes[index])
        r = self.img_size / max(h0, w0)
        h, w = (int(h0 * r), int(w0 * r)) if r != 1 else (h0, w0)
        return (h0, w0), (h, w), letterbox_geometry((h, w), self.canvas(index), auto=False, scaleup=False)

    def item_shapes(self, index):
        """The reference's `shapes` entry (datasets.py:856): ((h0, w0), ((h / h0, w / w0), (dw, dh)))."""
        (h0, w0), (h, w), (_, _, pad, _) = self.geometry(index)
        return (h0, w0), ((h / h0, w / w0), pad)

    def item_labels(self, index):
        """The image's labels on its canvas (datasets.py:858-860, 894-899): fp32 [n, 5] (cls, x, y, w, h)
        normalised by the canvas, in the reference's numpy fp32 arithmetic."""
        _, (h, w), (_, ratio, (padw, padh), _) = self.geometry(index)
        ch, cw = self.canvas(index)
        x = self.labels[index]
        l = x.copy()
        if l.size:
            sw, sh = ratio[0] * w, ratio[1] * h
            x1 = sw * (x[:, 1] - x[:, 3] / 2) + padw    # xywhn2xyxy, general.py:295-302
            y1 = sh * (x[:, 2] - x[:, 4] / 2) + padh
            x2 = sw * (x[:, 1] + x[:, 3] / 2) + padw
            y2 = sh * (x[:, 2] + x[:, 4] / 2) + padh
            l[:, 1], l[:, 2], l[:, 3], l[:, 4] = (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1   # xyxy2xywh
            l[:, [2, 4]] /= ch
            l[:, [1, 3]] /= cw
        return l

    def frame(self, index):
        """The decoded image: HWC uint8 at its own size, BGR or in the frame mode's channel order."""
        img = self.imgs[index]
        if img is None:
            img = read_frame(self.img_files[index], self.frames, self.channels)
            if self.cache_images:
                self.imgs[index] = img
        return img


class ValLoader:
    """Batches of a LoadImagesAndLabels in order, as the reference's DataLoader + collate_fn yield them
    (datasets.py:925-929): (img, targets, paths, shapes), with img the letterboxed batch already on the device
    as [nb, 3, h, w] half (or float) RGB in [0, 1] and targets fp32 [n, 6] (index in batch, cls, x, y, w, h) on
    the host.  Frames are decoded by a thread pool one batch ahead, uploaded through pinned memory and written
    onto the canvas (colour 114) by one letterbox_ragged call on the current stream.  frames / channels default to
    the dataset's; with a frame mode other than None / 'RGB' img is [nb, C, h, w] in the frames' channel order."""

    def __init__(self, dataset, batch_size, half=True, device=None, workers=LOADER_WORKERS, frames=None,
                 channels=None):
        self.dataset, self.batch_size, self.half, self.device = dataset, batch_size, half, device
        if frames is not None or channels is not None:
            dataset.frames, dataset.channels = frames, channels
        self.workers = max(1, int(workers))

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for img, targets, paths, shapes, _ in self.batches():
            yield img, targets, paths, shapes

    def _upload(self, frames, device):
        sizes = [f.size for f in frames]
        host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
        view, off = host.numpy(), 0
        for f, n in zip(frames, sizes):
            view[off:off + n] = f.reshape(-1)
            off += n
        dev = host.to(device, non_blocking=True)
        out, off = [], 0
        for f, n in zip(frames, sizes):
            out.append(dev[off:off + n].view(f.shape))
            off += n
        return out

    def batches(self):
        """As __iter__, with each batch's per-image label counts as a fifth entry."""
        ds = self.dataset
        device = _hip_device(self.device if self.device is not None else 'cuda')
        groups = [range(i, min(i + self.batch_size, len(ds))) for i in range(0, len(ds), self.batch_size)]
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            ahead = [pool.submit(ds.frame, i) for i in groups[0]] if groups else []
            for g, idx in enumerate(groups):
                frames = [f.result() for f in ahead]
                ahead = [pool.submit(ds.frame, i) for i in groups[g + 1]] if g + 1 < len(groups) else []
                geoms = [ds.geometry(i)[2] for i in idx]
                bgr = getattr(ds, 'frames', None) in (None, 'RGB')   # BGR frames -> RGB planes; others keep order
                img = letterbox_ragged(self._upload(frames, device), geoms, ds.canvas(idx[0]), swap_rb=bgr,
                                       out_kind=OUT_F16_CHW if self.half else OUT_F32_CHW, device=device)
                labels = [ds.item_labels(i) for i in idx]
                targets = torch.zeros((sum(len(l) for l in labels), 6))
                off = 0
                for j, l in enumerate(labels):
                    targets[off:off + len(l), 0] = j
                    targets[off:off + len(l), 1:] = torch.from_numpy(l)
                    off += len(l)
                yield (img, targets, tuple(ds.img_files[i] for i in idx), tuple(ds.item_shapes(i) for i in idx),
                       [len(l) for l in labels])


def create_dataloader(mode, path, imgsz, batch_size, stride, opt=None, hyp=None, augment=False, cache=False, pad=0.0,
                      rect=False, rank=-1, world_size=1, workers=LOADER_WORKERS, image_weights=False, quad=False,
                      prefix='', dataset_name='COCO2017', data_dict=None, half=True, device=None, frames=None,
                      channels=None):
    """datasets.py:68-96 for evaluation: (loader, dataset); both support len().  mode, rank, world_size,
    image_weights, quad, dataset_name and data_dict are accepted for the reference's call sites and unused."""
    if augment:
        raise NotImplementedError('augmented loading (training) is not part of the MI355X inference path')
    dataset = LoadImagesAndLabels(path, imgsz, batch_size, augment=False, hyp=hyp, rect=rect, cache_images=cache,
                                  single_cls=bool(getattr(opt, 'single_cls', False)), stride=int(stride), pad=pad,
                                  prefix=prefix, frames=frames, channels=channels)
    return ValLoader(dataset, min(batch_size, len(dataset)), half=half, device=device, workers=workers), dataset
