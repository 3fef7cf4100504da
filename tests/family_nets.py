"""Small cfg dicts with DownC and Shortcut for the e6 / d6 / e6e tests, and their seeded synthetic weights."""
from __future__ import annotations

import copy
import functools

from models.yolo import Model
from yv7.synthetic import synthetic_state_dict


def _c(f, c, k=1, s=1):
    return [f, 1, 'Conv', [c, k, s]]


def _half(c, out, first):
    """A short E-ELAN half: 2 x 1x1 split (read `first` layers back), 2 x 3x3, 4-way concat, 1x1."""
    return [_c(first[0], c), _c(first[1], c), _c(-1, c, 3), _c(-1, c, 3), [[-1, -2, -3, -4], 1, 'Concat', [1]],
            _c(-1, out)]


def _twice(c, out):
    """yolov7-e6e's doubled block (cfg/deploy/yolov7-e6e.yaml:20-40), shortened: two halves on one input, joined
    by a residual Shortcut."""
    return _half(c, out, (-1, -2)) + _half(c, out, (-7, -8)) + [[[-1, -7], 1, 'Shortcut', [1]]]


# ReOrg, Conv 80, DownC 160, a doubled block (Shortcut at layer 15, stride 4), DownC 320, a doubled block
# (Shortcut at layer 29, stride 8), a 2-level Detect
MINI_E6E = {'nc': 3, 'depth_multiple': 1.0, 'width_multiple': 1.0,
            'anchors': [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119]],
            'backbone': [[-1, 1, 'ReOrg', []], _c(-1, 80, 3), [-1, 1, 'DownC', [160]]] + _twice(64, 160) +
                        [[-1, 1, 'DownC', [320]]] + _twice(128, 320),
            'head': [[[15, 29], 1, 'Detect', ['nc', 'anchors']]]}


def add_net(c):
    """A net whose Shortcut (layer 8) adds two `c`-channel 1x1 conv outputs that both lie at non-zero channel
    offsets of wider concat tensors (layers 6, 7) and whose sum lands at a non-zero offset of a third (layer
    10), the three of different widths; one Detect level at stride 8."""
    return {'nc': 3, 'depth_multiple': 1.0, 'width_multiple': 1.0, 'anchors': [[30, 61, 62, 45, 59, 119]],
            'backbone': [_c(-1, 32, 3, 2), _c(-1, 64, 3, 2), _c(-1, 64, 3, 2),      # 0-2: stride 8
                         _c(2, c), _c(2, c), _c(2, c, 3),                            # 3-5 (5 is 3x3: no sibling of 3, 4)
                         [[3, 4], 1, 'Concat', [1]],                                 # 6: layer 4 at offset c of 2c
                         [[2, 5], 1, 'Concat', [1]],                                 # 7: layer 5 at offset 64 of 64 + c
                         [[4, 5], 1, 'Shortcut', [1]],                               # 8
                         _c(6, 2 * c, 3),                                            # 9
                         [[9, 8], 1, 'Concat', [1]],                                 # 10: the sum at offset 2c of 3c
                         _c(6, 32), _c(7, 32), _c(10, 32),                           # 11-13
                         [[-1, -2, -3], 1, 'Concat', [1]], _c(-1, 64, 3)],           # 14, 15
            'head': [[[15], 1, 'Detect', ['nc', 'anchors']]]}


def res_net(kin):
    """A net whose Shortcut (layer 8) folds into the 1x1 conv of layer 7 (K = kin -> 160 channels: the last 128-wide
    N tile is masked): the residual (layer 4) lies at offset 160 of a 320-channel concat, the sum at offset 32 of
    a 192-channel one; one Detect level at stride 8."""
    return {'nc': 3, 'depth_multiple': 1.0, 'width_multiple': 1.0, 'anchors': [[30, 61, 62, 45, 59, 119]],
            'backbone': [_c(-1, 32, 3, 2), _c(-1, 64, 3, 2), _c(-1, 64, 3, 2),      # 0-2: stride 8
                         _c(2, 160), _c(2, 160), _c(2, kin, 3),                      # 3-5 (5 is 3x3: no sibling)
                         [[3, 4], 1, 'Concat', [1]],                                 # 6: layer 4 at offset 160 of 320
                         _c(5, 160),                                                 # 7: the conv that takes the residual
                         [[7, 4], 1, 'Shortcut', [1]],                               # 8
                         _c(6, 32, 3),                                               # 9
                         [[9, 8], 1, 'Concat', [1]],                                 # 10: the sum at offset 32 of 192
                         _c(6, 32), _c(10, 32),                                      # 11, 12
                         [[-1, -2], 1, 'Concat', [1]], _c(-1, 64, 3)],               # 13, 14
            'head': [[[14], 1, 'Detect', ['nc', 'anchors']]]}


@functools.lru_cache(maxsize=None)
def _weights(key, calib_hw, seed):
    cfg = key if isinstance(key, str) else (MINI_E6E if key == ('mini',) else
                                            (res_net if key[0] == 'res' else add_net)(key[1]))
    m = Model(copy.deepcopy(cfg))
    return m.yaml, synthetic_state_dict(m, seed=seed, calib_hw=calib_hw)


def fresh(key, calib_hw=128, seed=0, fuse=True):
    """A new fp32 eval Model with cached synthetic weights.  key: a registered name, ('mini',) for MINI_E6E or
    ('add', c) for add_net(c), ('res', kin) for res_net(kin)."""
    cfg, sd = _weights(key, calib_hw, seed)
    m = Model(copy.deepcopy(cfg))
    m.load_state_dict(sd)
    m = m.float().eval()
    return m.fuse() if fuse else m
