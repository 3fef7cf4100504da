"""yv7_letterbox_c / yv7_letterbox_ragged_c: the letterbox for frames of 1..16 interleaved channels.

Both entry points through ctypes, torch.equal against tests/letterbox_channels_ref.py (oracle.letterbox_ref's
resize_linear_u8 on an [h][w][C] array, a per-channel pad) for every output kind, into guarded buffers whose
canary bytes before and after dst must survive.  The 24 x 40 -> 19 x 31 case is the one whose seeded inputs tell
the interleaved rounding split from the 3-channel and the per-plane ones (tests/test_letterbox_channels_cpu.py
asserts that); the others are one per resize mode and edge: exact 2x, identity, an up-scale, one-column and
one-row sources, and a row wider than one 128-thread block.
"""
import ctypes

import numpy as np
import pytest
import torch

import letterbox_channels_ref as H
from utils import datasets as D
from yv7 import _lib

CHANNELS = [1, 2, 3, 4, 5, 8, 16]
KINDS = [0, 1, 2]
DTYPES = {0: torch.uint8, 1: torch.float16, 2: torch.float32}
GUARD = 256   # bytes of canary on each side of dst; a multiple of every store's alignment

# (source h, w), (resized h, w), (top, left), (canvas h, w)
CASES = {
    'bilinear': ((24, 40), (19, 31), (5, 1), (32, 32)),
    'area2x': ((48, 64), (24, 32), (3, 5), (32, 40)),
    'identity': ((32, 32), (32, 32), (4, 9), (40, 48)),
    'upscale': ((7, 9), (23, 30), (2, 1), (32, 32)),
    'one_column': ((9, 1), (12, 5), (7, 11), (32, 32)),
    'one_row': ((1, 9), (4, 13), (0, 0), (32, 32)),
    'two_blocks': ((3, 70), (6, 140), (1, 7), (8, 150)),
}
RAGGED_CANVAS = (40, 150)   # holds every case above at its (top, left)


def _border(case, canvas=None):
    _, (nh, nw), (top, left), (oh, ow) = case
    oh, ow = canvas or (oh, ow)
    return (top, oh - top - nh, left, ow - left - nw)


_REF = {}


def reference(name, C, seed, canvas=None):
    """The letterboxed uint8 [oh, ow, C] frame of a case, and its source; computed once per key."""
    key = (name, C, seed, canvas)
    if key not in _REF:
        (h, w), (nh, nw), _, _ = CASES[name]
        src = H.random_frame(h, w, C, seed)
        _REF[key] = (src, H.place(src, (nw, nh), _border(CASES[name], canvas), H.pads(C)))
    return _REF[key]


class Guarded:
    """A device buffer with canaries around the part the library may write."""

    def __init__(self, shape, kind):
        self.shape, self.dtype = shape, DTYPES[kind]
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=self.dtype).element_size()
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
        self.ptr = self.buf.data_ptr() + GUARD

    def result(self):
        host = self.buf.cpu()
        assert bool((host[:GUARD] == 0xA5).all()) and bool((host[GUARD + self.nbytes:] == 0xA5).all()), \
            'canary bytes around dst were overwritten'
        return host[GUARD:GUARD + self.nbytes].clone().view(self.dtype).reshape(self.shape)


def _pad(C):
    return (ctypes.c_uint8 * C)(*H.pads(C))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out_shape(B, C, oh, ow, kind):
    return (B, oh, ow, C) if kind == 0 else (B, C, oh, ow)


def call_c(srcs, case, C, kind, swap_rb=0):
    """yv7_letterbox_c on a batch of same-size frames."""
    (h, w), (nh, nw), (top, left), (oh, ow) = case
    L = _lib.lib()
    src = torch.from_numpy(np.stack(srcs)).cuda()
    out = Guarded(_out_shape(len(srcs), C, oh, ow, kind), kind)
    ws = torch.empty(int(L.yv7_letterbox_workspace_bytes(nh, nw)), dtype=torch.uint8, device='cuda')
    rc = L.yv7_letterbox_c(src.data_ptr(), len(srcs), h, w, C, nh, nw, top, left, oh, ow, _pad(C), swap_rb, kind,
                           out.ptr, ws.data_ptr(), ws.numel(), _stream())
    assert rc == 0, L.yv7_last_error().decode()
    return out.result()


def call_ragged_c(srcs, cases, canvas, C, kind, swap_rb=0):
    """yv7_letterbox_ragged_c on frames of their own sizes."""
    L = _lib.lib()
    dev = [torch.from_numpy(s).cuda() for s in srcs]
    descs = (_lib.FrameDesc * len(srcs))()
    for d, t, ((h, w), (nh, nw), (top, left), _) in zip(descs, dev, cases):
        d.data, d.h, d.w, d.new_h, d.new_w, d.top, d.left = t.data_ptr(), h, w, nh, nw, top, left
    out = Guarded(_out_shape(len(srcs), C, *canvas, kind), kind)
    rc = L.yv7_letterbox_ragged_c(descs, len(srcs), C, canvas[0], canvas[1], _pad(C), swap_rb, kind, out.ptr, None, 0,
                                  _stream())
    assert rc == 0, L.yv7_last_error().decode()
    return out.result()


def _assert_equal(got, want_u8, kind, what):
    want = H.output(want_u8, kind)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert torch.equal(got, want), f'{what}: {int((got != want).sum())} of {want.numel()} values differ'


@pytest.mark.gpu
@pytest.mark.parametrize('C', CHANNELS)
def test_letterbox_c_equals_reference(C):
    """Two frames per call, so the batch stride is exercised too."""
    for name, case in CASES.items():
        refs = [reference(name, C, seed) for seed in (11, 12)]
        for kind in KINDS:
            got = call_c([r[0] for r in refs], case, C, kind)
            for b, (_, want) in enumerate(refs):
                _assert_equal(got[b], want, kind, f'C={C} {name} kind {kind} frame {b}')


@pytest.mark.gpu
@pytest.mark.parametrize('C', CHANNELS)
def test_letterbox_ragged_c_equals_reference(C):
    """Every case as one frame of a single call: seven sizes, all three resize modes, one canvas."""
    names = list(CASES)
    refs = [reference(n, C, 21 + i, RAGGED_CANVAS) for i, n in enumerate(names)]
    for kind in KINDS:
        got = call_ragged_c([r[0] for r in refs], [CASES[n] for n in names], RAGGED_CANVAS, C, kind)
        for b, (n, (_, want)) in enumerate(zip(names, refs)):
            _assert_equal(got[b], want, kind, f'C={C} {n} kind {kind}')


@pytest.mark.gpu
@pytest.mark.parametrize('C', [1, 4, 5])
def test_ragged_c_two_chunks_of_the_argument(C):
    """65 frames of 8 x 8 resized to 6 x 6: the records travel 64 per launch, so this takes two."""
    case = ((8, 8), (6, 6), (1, 1), (8, 8))
    srcs = [H.random_frame(8, 8, C, 100 + i) for i in range(65)]
    for kind in (0, 1):
        got = call_ragged_c(srcs, [case] * 65, (8, 8), C, kind)
        for b in (0, 1, 62, 63, 64):
            _assert_equal(got[b], H.place(srcs[b], (6, 6), (1, 1, 1, 1), H.pads(C)), kind, f'C={C} frame {b}')


def _old_pads():
    return H.pads(3)


@pytest.mark.gpu
@pytest.mark.parametrize('swap_rb', [0, 1])
def test_three_channels_equal_the_existing_ragged_entry_point(swap_rb):
    L = _lib.lib()
    names = list(CASES)
    srcs = [reference(n, 3, 31 + i, RAGGED_CANVAS)[0] for i, n in enumerate(names)]
    dev = [torch.from_numpy(s).cuda() for s in srcs]
    descs = (_lib.FrameDesc * len(srcs))()
    for d, t, n in zip(descs, dev, names):
        (h, w), (nh, nw), (top, left), _ = CASES[n]
        d.data, d.h, d.w, d.new_h, d.new_w, d.top, d.left = t.data_ptr(), h, w, nh, nw, top, left
    for kind in KINDS:
        new = call_ragged_c(srcs, [CASES[n] for n in names], RAGGED_CANVAS, 3, kind, swap_rb)
        old = Guarded(_out_shape(len(srcs), 3, *RAGGED_CANVAS, kind), kind)
        rc = L.yv7_letterbox_ragged(descs, len(srcs), *RAGGED_CANVAS, *_old_pads(), swap_rb, kind, old.ptr, None, 0,
                                    _stream())
        assert rc == 0, L.yv7_last_error().decode()
        assert torch.equal(new.view(torch.uint8), old.result().view(torch.uint8)), (kind, swap_rb)


@pytest.mark.gpu
def test_three_channels_swapped_equal_yv7_letterbox():
    """yv7_letterbox's float planes are the frame's reversed: yv7_letterbox_c(channels = 3, swap_rb = 1); its uint8
    kind ignores swap_rb."""
    L = _lib.lib()
    for name in ('bilinear', 'area2x', 'identity'):
        case = CASES[name]
        (h, w), (nh, nw), (top, left), (oh, ow) = case
        srcs = [reference(name, 3, seed)[0] for seed in (41, 42)]
        src = torch.from_numpy(np.stack(srcs)).cuda()
        ws = torch.empty(int(L.yv7_letterbox_workspace_bytes(nh, nw)), dtype=torch.uint8, device='cuda')
        for kind, swaps in ((0, (0, 1)), (1, (1,)), (2, (1,))):
            old = Guarded(_out_shape(2, 3, oh, ow, kind), kind)
            rc = L.yv7_letterbox(src.data_ptr(), 2, h, w, nh, nw, top, left, oh, ow, *_old_pads(), kind, old.ptr,
                                 ws.data_ptr(), ws.numel(), _stream())
            assert rc == 0, L.yv7_last_error().decode()
            want = old.result().view(torch.uint8)
            for swap_rb in swaps:
                assert torch.equal(call_c(srcs, case, 3, kind, swap_rb).view(torch.uint8), want), (name, kind, swap_rb)


def test_argument_errors():
    """Each returns YV7_E_ARG with a message naming the function before anything is launched (no device is
    touched: the pointers are never followed)."""
    L = _lib.lib()
    desc = (_lib.FrameDesc * 1)(_lib.FrameDesc(data=0x1000, h=10, w=10, new_h=10, new_w=10, top=0, left=0))
    pad = (ctypes.c_uint8 * 16)(*range(16))
    src, dst, ws = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)

    def plain(C=4, pad=pad, swap_rb=0, kind=0, dst=dst, new_w=10, ws_bytes=1 << 20):
        return L.yv7_letterbox_c(src, 1, 10, 10, C, 10, new_w, 0, 0, 16, 16, pad, swap_rb, kind, dst, ws, ws_bytes,
                                 None)

    def ragged(C=4, pad=pad, swap_rb=0, kind=0, dst=dst, B=1, oh=16):
        return L.yv7_letterbox_ragged_c(desc, B, C, oh, 16, pad, swap_rb, kind, dst, None, 0, None)

    for fn, name in ((plain, 'yv7_letterbox_c'), (ragged, 'yv7_letterbox_ragged_c')):
        for kw, code, text in [
            (dict(C=0), -1, 'channels must be 1..16'),
            (dict(C=17), -1, 'channels must be 1..16'),
            (dict(C=-3), -1, 'channels must be 1..16'),
            (dict(C=4, swap_rb=1), -1, 'swap_rb needs channels == 3'),
            (dict(C=1, swap_rb=1), -1, 'swap_rb needs channels == 3'),
            (dict(pad=None), -1, 'null pad'),
            (dict(dst=None), -1, 'null argument'),
            (dict(kind=3), -1, 'out_kind must be 0, 1 or 2'),
            (dict(C=4, dst=ctypes.c_void_p(0x2002)), -1, 'aligned'),
        ]:
            rc = fn(**kw)
            msg = L.yv7_last_error().decode()
            assert rc == code and text in msg and msg.startswith(name + ':'), (name, kw, rc, msg)
    # the existing functions' size and geometry checks
    assert plain(new_w=17) == -2 and 'yv7_letterbox_c: the resized image must lie inside' in L.yv7_last_error().decode()
    assert plain(ws_bytes=8) == -3 and 'yv7_letterbox_c: workspace too small' in L.yv7_last_error().decode()
    assert ragged(B=0) == -1 and 'yv7_letterbox_ragged_c: B must be positive' in L.yv7_last_error().decode()
    assert ragged(oh=8) == -2 and 'yv7_letterbox_ragged_c: frame 0: the resized image must lie inside' in \
        L.yv7_last_error().decode()


@pytest.mark.gpu
def test_python_wrappers_take_channel_frames():
    """letterbox / letterbox_batch / letterbox_ragged on [.., C] frames: the default colour is 114 everywhere, a
    scalar or C values are taken as given, a wrong count raises."""
    C = 4
    src = H.random_frame(24, 40, C, 51)
    want, ratio, dwdh = H.letterbox(src, (32, 32), [114] * C)
    got, r, d = D.letterbox(src, (32, 32), auto=False)
    assert isinstance(got, np.ndarray) and np.array_equal(got, want) and r == ratio and d == dwdh
    x, _, _ = D.letterbox_batch(np.stack([src, src]), 32, half=True, color=7)
    assert torch.equal(x[1].cpu(), H.to_planes(H.letterbox(src, (32, 32), [7] * C)[0], half=True))
    geom = D.letterbox_geometry((24, 40), (32, 32), auto=False)
    out = D.letterbox_ragged([src], [geom], (32, 32), color=H.pads(C), swap_rb=True, out_kind=D.OUT_F32_CHW)
    assert torch.equal(out[0].cpu(), H.to_planes(H.letterbox(src, (32, 32), H.pads(C))[0]))
    with pytest.raises(ValueError, match='color'):
        D.letterbox_ragged([src], [geom], (32, 32), color=(1, 2, 3))
    with pytest.raises(ValueError, match='frames'):
        D.letterbox_ragged([src, src[:, :, :3]], [geom, geom], (32, 32))


@pytest.mark.gpu
def test_ragged_wrapper_enqueues_without_a_host_sync():
    try:
        torch.cuda.set_sync_debug_mode('error')
        try:
            with pytest.raises(RuntimeError):
                torch.ones(1, device='cuda').item()     # the mode must see a real sync, or it shows nothing
        finally:
            torch.cuda.set_sync_debug_mode('default')
    except (pytest.fail.Exception, AttributeError):
        pytest.skip('torch.cuda.set_sync_debug_mode("error") does not flag a .item() on this ROCm build')
    C = 4
    srcs = [H.random_frame(h, w, C, 61 + i) for i, (h, w) in enumerate([(24, 40), (48, 64), (32, 32)])]
    geoms = [D.letterbox_geometry(s.shape[:2], (32, 32), auto=False) for s in srcs]
    dev = [torch.from_numpy(s).cuda() for s in srcs]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = D.letterbox_ragged(dev, geoms, (32, 32), out_kind=D.OUT_F16_CHW)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for b, s in enumerate(srcs):
        assert torch.equal(out[b].cpu(), H.to_planes(H.letterbox(s, (32, 32), [114] * C)[0], half=True)), b
