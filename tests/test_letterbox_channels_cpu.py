"""The C-channel image entry points on the host: the reference helper the GPU tests compare against, the proof that
their inputs separate the right rounding rule from the two wrong ones, the frame modes and readers, the channel
checks of autoShape, and the ctypes signatures of the two new C functions."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import letterbox_channels_ref as H
from oracle import letterbox_ref as R
from test_letterbox_channels import CASES, reference
from utils import datasets as D
from yv7 import _lib


# ------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize('shape,canvas', [((24, 40), (32, 32)), ((48, 64), (32, 32)), ((32, 32), (40, 48)),
                                          ((7, 9), (32, 32))])
def test_helper_equals_the_oracle_at_three_channels(shape, canvas):
    img = H.random_frame(*shape, 3, 1)
    want, ratio, dwdh = R.letterbox(img, canvas, color=(9, 80, 200), auto=False)
    got, r, d = H.letterbox(img, canvas, (9, 80, 200))
    assert np.array_equal(got, want) and r == ratio and d == dwdh
    assert torch.equal(H.to_planes(got[:, :, ::-1], half=True), R.to_input(got, half=True))
    assert torch.equal(H.to_planes(got[:, :, ::-1]), R.to_input(got))


def resize_with_split(img, new_w, new_h, two_step):
    """resize_linear_u8's bilinear path with the vertical pass's rounding chosen by two_step[x, c] (bool)."""
    h, w, cn = img.shape
    src = img.astype(np.int64)
    xs0, xs1, a0, a1 = R.linear_tables(w, new_w, True)
    ys0, ys1, b0, b1 = R.linear_tables(h, new_h, False)
    d = src[:, xs0, :] * a0[None, :, None] + src[:, xs1, :] * a1[None, :, None]
    d0, d1 = d[ys0], d[ys1]
    bb0, bb1 = b0[:, None, None], b1[:, None, None]
    vec = ((((d0 >> 4) * bb0) >> 16) + (((d1 >> 4) * bb1) >> 16) + 2) >> 2
    sca = (d0 * bb0 + d1 * bb1 + (1 << 21)) >> 22
    return np.clip(np.where(two_step[None], vec, sca), 0, 255).astype(np.uint8)


def splits(new_w, cn):
    pos = np.arange(new_w)[:, None] * cn + np.arange(cn)[None, :]
    x = np.broadcast_to(np.arange(new_w)[:, None], (new_w, cn))
    return {'interleaved': pos < new_w * cn // 16 * 16, 'times3': pos < new_w * 3 // 16 * 16,
            'per_plane': x < new_w // 16 * 16}


@pytest.mark.parametrize('C', [1, 2, 3, 4, 5, 8, 16])
def test_gpu_inputs_tell_the_rounding_rules_apart(C):
    """On the 24 x 40 -> 19 x 31 sources the GPU tests use, a kernel that kept the 3-channel split (C != 3) or split
    per plane (C >= 2) would give other bytes than the reference."""
    (h, w), (nh, nw), _, _ = CASES['bilinear']
    for seed, canvas in ((11, None), (12, None), (21, (40, 150))):
        src = reference('bilinear', C, seed, canvas)[0]
        want = R.resize_linear_u8(src, nw, nh)
        s = splits(nw, C)
        assert np.array_equal(resize_with_split(src, nw, nh, s['interleaved']), want)
        if C != 3:
            assert (resize_with_split(src, nw, nh, s['times3']) != want).any(), (C, seed)
        if C >= 2:
            assert (resize_with_split(src, nw, nh, s['per_plane']) != want).any(), (C, seed)


# ------------------------------------------------------------------------------------------ modes and readers
def test_frame_modes():
    assert D.FRAME_MODES == ('L', 'LA', 'RGB', 'RGBA', 'raw')
    assert [D.frame_channels(m) for m in D.FRAME_MODES] == [1, 2, 3, 4, None]
    for m in D.FRAME_MODES[:4]:
        assert len(Image.new(m, (2, 2)).getbands()) == D.frame_channels(m)
    with pytest.raises(ValueError, match='frames must be one of'):
        D.frame_channels('CMYK')
    assert D.pad_colour((114, 114, 114), 5) == [114] * 5 and D.pad_colour(3, 2) == [3, 3]
    assert D.pad_colour([1, 2, 3, 4], 4) == [1, 2, 3, 4]
    for bad in ((1, 2, 3), (1, 2, 3, 4, 5), (0, 0, 0, 256)):
        with pytest.raises(ValueError, match='color'):
            D.pad_colour(bad, 4)


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('frames')
    arr = H.random_frame(10, 14, 4, 3)
    out = {'arr': arr}
    for mode, a in (('L', arr[:, :, 0]), ('LA', arr[:, :, :2]), ('RGB', arr[:, :, :3]), ('RGBA', arr)):
        out[mode] = str(d / f'{mode}.png')
        Image.fromarray(a, mode).save(out[mode])
    out['jpg'] = str(d / 'rgb.jpg')
    Image.fromarray(arr[:, :, :3], 'RGB').save(out['jpg'])
    out['npy5'], out['npy2d'], out['npyf'] = str(d / 'five.npy'), str(d / 'flat.npy'), str(d / 'float.npy')
    out['five'] = H.random_frame(10, 14, 5, 4)
    np.save(out['npy5'], out['five'])
    np.save(out['npy2d'], arr[:, :, 0])
    np.save(out['npyf'], arr.astype(np.float32))
    out['u16'], out['pal'] = str(d / 'deep.png'), str(d / 'palette.png')
    Image.fromarray((arr[:, :, 0].astype(np.uint16) << 8)).save(out['u16'])
    Image.fromarray(arr[:, :, 0], 'L').convert('P').save(out['pal'])
    return out


def test_imread_modes(files):
    arr = files['arr']
    own = {'L': arr[:, :, :1], 'LA': arr[:, :, :2], 'RGB': arr[:, :, :3], 'RGBA': arr}
    for name, a in own.items():
        raw = D.imread(files[name], 'raw')
        assert raw.dtype == np.uint8 and raw.flags['C_CONTIGUOUS'] and np.array_equal(raw, a), name
        assert np.array_equal(D.imread(files[name], name), a)          # a file in its own mode converts to itself
        for mode in D.FRAME_MODES[:4]:                                    # every conversion is PIL's
            with Image.open(files[name]) as im:
                want = np.asarray(im.convert(mode))
            got = D.imread(files[name], mode)
            assert got.shape == (10, 14, D.frame_channels(mode)) and np.array_equal(got, want.reshape(got.shape))
    # mode None is today's BGR reader
    assert np.array_equal(D.imread(files['RGB']), arr[:, :, 2::-1])
    with Image.open(files['jpg']) as im:
        rgb, luma = np.asarray(im.convert('RGB')), np.asarray(im.convert('L'))
    assert np.array_equal(D.imread(files['jpg']), rgb[:, :, ::-1])
    assert np.array_equal(D.imread(files['jpg'], 'raw'), rgb) and np.array_equal(D.imread(files['jpg'], 'L')[:, :, 0], luma)
    # .npy: HWC and HW, 'raw' only
    assert np.array_equal(D.imread(files['npy5'], 'raw'), files['five'])
    assert np.array_equal(D.imread(files['npy2d'], 'raw'), arr[:, :, :1])
    assert D.image_size(files['npy5']) == (14, 10) and D.image_size(files['npy2d']) == (14, 10)
    assert D.image_size(files['RGBA']) == (14, 10)


def test_imread_refusals(files):
    for key, what in (('u16', r"deep\.png: holds mode 'I;16"), ('pal', r"palette\.png: holds mode 'P'"),
                      ('npyf', r'float\.npy: holds a float32 array of shape \(10, 14, 4\)')):
        with pytest.raises(ValueError, match=what):
            D.imread(files[key], 'raw')
    with pytest.raises(ValueError, match=r"five\.npy: a \.npy array is read with frames='raw' only"):
        D.imread(files['npy5'], 'L')
    with pytest.raises(ValueError, match='frames must be one of'):
        D.imread(files['L'], 'bgr')


def test_read_frame_names_file_and_both_counts(files):
    with pytest.raises(ValueError, match=r'RGBA\.png: holds 4-channel frames, the model takes 1'):
        D.read_frame(files['RGBA'], 'raw', 1)
    assert D.read_frame(files['RGBA'], 'L', 1).shape == (10, 14, 1)
    assert np.array_equal(D.read_frame(files['RGB'], None, None), D.imread(files['RGB']))


# ------------------------------------------------------------------------------------------ autoShape's checks
def test_as_hwc():
    from models.common import _as_hwc
    a = H.random_frame(6, 9, 5, 1)
    assert _as_hwc(a, 5) is a
    assert np.array_equal(_as_hwc(np.ascontiguousarray(a.transpose(2, 0, 1)), 5), a)      # CHW
    g = a[:, :, 0]
    assert _as_hwc(g, 1).shape == (6, 9, 1) and np.array_equal(_as_hwc(g, 1)[:, :, 0], g)
    sq = H.random_frame(4, 7, 4, 2)                # [4, 7, 4]: both ends could be the channels -> taken as HWC
    assert _as_hwc(sq, 4) is sq
    for bad, C in ((a, 4), (g, 2), (a[None], 5), (a[:, :, :3], 1)):
        with pytest.raises(ValueError, match=rf'expected an image of {C} channels .* got shape'):
            _as_hwc(bad, C)
    with pytest.raises(ValueError, match='must be uint8'):
        _as_hwc(a.astype(np.float32), 5)
    with pytest.raises(ValueError, match='HIP device'):
        _as_hwc(torch.from_numpy(a), 5)


def _model(ch):
    from models.yolo import Model
    return Model('yolov7-tiny', ch=ch)


def test_mode_and_model_channels_must_agree():
    from models.common import autoShape
    m1, m4 = _model(1), _model(4)
    for m, frames in ((m1, 'RGB'), (m1, 'LA'), (m4, 'L'), (m4, 'RGB')):
        with pytest.raises(ValueError, match='-channel frames, the model takes'):
            m.autoshape(frames=frames)
        with pytest.raises(ValueError, match='-channel frames, the model takes'):
            autoShape(m, frames=frames)
    with pytest.raises(ValueError, match='frames must be one of'):
        m1.autoshape(frames='gray')
    for m, frames, ch in ((m1, 'L', 1), (m4, 'RGBA', 4), (m4, 'raw', 4), (m1, 'raw', 1), (_model(3), 'RGB', 3)):
        a = m.autoshape(frames=frames)
        assert (a.frames, a.ch) == (frames, ch) and a.stride is m.stride
    with pytest.raises(ValueError, match='-channel frames, the model takes 5'):
        D.check_frame_mode('RGBA', 5)
    D.check_frame_mode('raw', 16)
    with pytest.raises(ValueError, match='the model takes 17'):
        D.check_frame_mode('raw', 17)


def test_without_frames_a_gray_model_is_still_refused():
    from models.common import autoShape
    m = _model(1)
    for call in (m.autoshape, lambda: autoShape(m), lambda: m.autoshape(frames=None)):
        with pytest.raises(RuntimeError, match='this entry point loads 3-channel images'):
            call()


def test_display_channels():
    from utils.plots import display_channels, display_copy
    assert [display_channels(c) for c in (1, 2, 3, 4, 16)] == [(0, 0, 0), (0, 1, 1), (0, 1, 2), (0, 1, 2), (0, 1, 2)]
    x = torch.arange(2 * 5 * 3 * 4, dtype=torch.uint8).reshape(2, 5, 3, 4)
    assert torch.equal(display_copy(x, 1), x[:, [0, 1, 2]]) and display_copy(x, 1).is_contiguous()
    assert torch.equal(display_copy(x[:, :2], 1), x[:, [0, 1, 1]])
    assert torch.equal(display_copy(x[0, :1].permute(1, 2, 0), 2), x[0, [0, 0, 0]].permute(1, 2, 0))


# ------------------------------------------------------------------------------------------ the C ABI
def test_ctypes_signatures():
    L = _lib.lib()
    i, vp, sz, pu8 = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint8)
    assert L.yv7_letterbox_c.restype is i and L.yv7_letterbox_ragged_c.restype is i
    assert L.yv7_letterbox_c.argtypes == [vp, i, i, i, i, i, i, i, i, i, i, pu8, i, i, vp, vp, sz, vp]
    assert L.yv7_letterbox_ragged_c.argtypes == [ctypes.POINTER(_lib.FrameDesc), i, i, i, i, pu8, i, i, vp, vp, sz, vp]
    assert D.MAX_CHANNELS == 16
