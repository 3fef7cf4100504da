"""The fp16 implicit-GEMM families — the register-staged tile kernel and the 8-wave ring with split-K
(csrc/conv_f16_ring.hip), the persistent rings and their weight-stationary forms (conv_f16_pring.hip), the 8-phase
rings (conv_f16_p8.hip) — and the spatial 3x3 kernels (conv_halo / conv_ws / conv_hring.hip) at ragged M, N and K
and on tile walks of more than one tile per block, op by op against fp32 torch (tests/opcheck.py, its own bar: one
fp16 ulp + 1e-4 rms for the convs, its STEM rule for the fused stem).  tests/test_addr_trim.py does the same for the
fragment families (270-279, 280-288, 290-295, 302-303), which are left out here.

The net (edge_net) is flat: all three Detect levels at stride 8, so a frame only needs H, W % 8 == 0.  Its stem is
yolov7's (3x3 strides 1, 2: stem2_kernel, the levels below at strides 2 / 4 / 8) or yolov7-tiny's (2, 2:
stem_kernel, levels at 4 / 8 / 8).  Level 1 has the 64 -> 64 3x3 of the weight-stationary spatial kernel, a 1x1
64 -> 120 (the only row with 256-pixel tiles and at most 128 outputs, 235, needs that many pixels to walk tiles)
and the inputs of the two stride-2 3x3 layers.  The wide level holds the layers of LAYERS: every one of them reads a
slice at a non-zero channel offset of one concat tensor and writes a slice at a non-zero offset of another (pitches
424 / 744 / 808 / 1720 / 1216; offsets such as 8, 16, 24, 40, 104, 232: 8-aligned, not 64-aligned), chained
through 1x1 "feeder" convs that give the next layer its input width.  The graph compiler's sibling merges are off
(YV7_NO_MERGE), so each layer stays one GEMM of its own width.  Four small 1x1 convs on the 24-channel layer put
something at offset 0 of each concat, and one 1x1 per concat reads it whole (K = 424 ... 1720) so that it is live.

Frames: B 8, 232 x 312 and B 3, 40 x 56 (ragged: with the (1, 2) stem M = 144 768 / 36 192 / 9 048 and
1 680 / 420 / 105 at strides 2 / 4 / 8; no level is a whole number of 128- or 256-pixel tiles, 105 is less than one
tile and 105 % 16 = 9; the stem's own 8 x 16 output tiles are partial too), and for the spatial kernels, whose maps
must be divisible by 16, B 5, 256 x 384 (480 tiles of the 64 -> 64 kernel; 360 of the halo ring, two per block) and
B 7, 192 x 320 (420; 315 of the halo ring, whose balanced grid of 158 blocks then ends on a block with one tile).

Every non-fragment entry of tests/test_variants.py's CONV_VARIANTS is forced on every conv, family by family
(FAMILIES), and per forward
  * check_ops passes, every conv output slice and z are finite,
  * the zero frame of every tensor of the plan is still zero (check_ops pads its reference itself),
and test_launch_accounting, from dry runs of the same plans (Plan.op_kernels), asserts per variant that its own
kernel launched (own_forms restates csrc/conv_f16.hip forced_rows with the rows of conv_f16_launch.h), on partial M
tiles and masked N tiles, that the persistent kernels walked more tiles than they have blocks (walk restates the
launchers' grid rules), the K-step counts 1, 2, 3, 5, 9 and both parities / residues of the 8-phase rings' buffer
rotation, and that the 2- and 4-way K splits really split (the split-K scratch shows in yv7_workspace_bytes).
profiles/gemm_edges/cases.txt is this module's -s output on an MI355X.

Reference: models/common.py:110-111 (Conv.fuseforward), models/yolo.py:46-57 (Detect).
"""
import copy
import functools
import re
import time

import pytest
import torch

from helpers import bordered, frames
from opcheck import check_ops, kernel_summary
from test_variants import CONV_VARIANTS
from yv7 import _lib as L
from yv7.runtime import kernel_key

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ANCHORS = [[10, 13, 16, 30, 33, 23], [30, 61, 62, 45, 59, 119], [116, 90, 156, 198, 373, 326]]

FRAGMENT = set(range(270, 280)) | set(range(280, 289)) | set(range(290, 296)) | {302, 303}   # test_addr_trim.py
VARIANTS = [v for v in CONV_VARIANTS if v not in FRAGMENT]
FAMILIES = {'tile': [1, 2, 8], 'ring': [4, 5, 6, 7],
            'ring-cfg01': [100, 102, 104, 110, 112, 114], 'ring-cfg23': [120, 122, 124, 130, 132, 134],
            'ring-cfg45': [140, 142, 144, 150, 152, 154],
            'pring': [201, 202, 203, 204, 205, 206], 'p8': [231, 232], 'ws1x1': [234, 235, 236, 239],
            'spatial': [10, 11, 15, 17, 262]}
SPATIAL = FAMILIES['spatial']
PERSISTENT = [201, 202, 203, 204, 205, 206, 231, 232, 234, 235, 236, 239, 11, 15, 17, 262]
RAGGED_FRAMES = [(8, 232, 312), (3, 40, 56)]
SQUARE_FRAMES = [(5, 256, 384), (7, 192, 320)]
STEMS = [(1, 2), (2, 2)]


@pytest.fixture(scope='module', autouse=True)
def _no_miopen():
    prev = torch.backends.cudnn.enabled
    torch.backends.cudnn.enabled = False
    yield
    torch.backends.cudnn.enabled = prev


def _c(f, c, k=1, s=1):
    return [f, 1, 'Conv', [c, k, s]]


def _cat(*f):
    return [list(f), 1, 'Concat', [1]]


# The wide level's layers under test: net layer -> (cin, cout, k, s).  19-35 at stride 1 from the wide level's own
# concats, 10 / 11 the stride-2 3x3 layers from level 1.
LAYERS = {19: (64, 520, 1, 1),    # nk 1
          20: (128, 264, 1, 1),   # nk 2
          22: (192, 264, 1, 1),   # nk 3; K <= 256 and 128 < cout <= 512: the N-split weight-stationary row's domain
          24: (320, 520, 1, 1),   # nk 5
          26: (448, 136, 1, 1),   # nk 7
          29: (96, 72, 1, 1),     # K tail: kpad 128, cout % 16 == 8
          30: (128, 120, 1, 1),   # a weight-stationary row with cout <= 128
          31: (256, 136, 1, 1),   # the weight-stationary row with 256-channel tiles
          32: (64, 264, 3, 1),    # nk 9
          33: (128, 136, 3, 1),   # nk 18
          34: (96, 72, 3, 1),     # kpad 896: a K step straddles two taps (the 8-phase rings refuse it)
          35: (128, 384, 3, 1),   # the column-group halo ring's layer (cout % 128 == 0)
          10: (64, 136, 3, 2),
          11: (128, 264, 3, 2)}
# ... and the 1x1 "feeders" between them: net layer -> (cin, cout)
FEEDERS = {17: (136, 64), 18: (264, 128), 21: (520, 192), 23: (264, 320), 25: (264, 448), 27: (520, 96), 28: (136, 256)}


def edge_net(sa):
    """sa: the stride of the stem's first conv (1: yolov7, 2: yolov7-tiny)."""
    last = 2 if sa == 1 else 1   # both forms reach stride 8 at the Detect level
    return {'nc': 3, 'depth_multiple': 1.0, 'width_multiple': 1.0, 'anchors': ANCHORS,
            'backbone': [_c(-1, 32, 3, sa), _c(-1, 64, 3, 2),               # 0-1: the fused stem -> level 1
                         _c(1, 64, 3), _c(1, 64), _c(1, 120),                # 2 (64 -> 64 3x3), 3, 4 (64 -> 120)
                         _cat(2, 3, 4),                                      # 5: 248 = [2 | 3 @64 | 4 @128]
                         _c(1, 40), _c(5, 128),                              # 6; 7: 248 -> 128
                         _cat(6, 7),                                         # 8: 168 = [6 | 7 @40]
                         _c(8, 24, 3, 2), _c(3, 136, 3, 2), _c(7, 264, 3, 2),   # 9 (cout <= 32), 10, 11 -> wide level
                         _cat(9, 10, 11),                                    # 12: A 424 = [9 | 10 @24 | 11 @160]
                         _c(9, 40), _c(9, 8), _c(9, 16), _c(9, 32),          # 13-16: offset 0 of B, C, D, E
                         _c(10, 64), _c(11, 128),                            # 17, 18: feeders 64 @B 40, 128 @B 104
                         _c(17, 520), _c(18, 264),                           # 19 @D 16, 20 @D 536
                         _c(19, 192), _c(21, 264),                           # 21 @B 232, 22 @D 800
                         _c(20, 320), _c(23, 520),                           # 23 @B 424, 24 @D 1064
                         _c(22, 448), _c(25, 136),                           # 25 @C 104, 26 @D 1584
                         _c(24, 96), _c(26, 256),                            # 27 @C 8, 28 @C 552
                         _c(27, 72), _c(18, 120), _c(28, 136),               # 29 @E 32, 30 @E 104, 31 @E 224
                         _c(17, 264, 3), _c(18, 136, 3), _c(27, 72, 3), _c(18, 384, 3),   # 32 @E 360, 33 @624, 34 @760, 35 @832
                         _cat(13, 17, 18, 21, 23),                           # 36: B 744
                         _cat(14, 27, 25, 28),                               # 37: C 808
                         _cat(15, 19, 20, 22, 24, 26),                       # 38: D 1720
                         _cat(16, 29, 30, 31, 32, 33, 34, 35),               # 39: E 1216
                         _c(12, 64), _c(36, 64), _c(37, 64), _c(38, 64), _c(39, 64),   # 40-44: each concat read whole
                         _cat(40, 41, 42, 43, 44),                           # 45: 320
                         _c(45, 64, 3, last),                                # 46 -> stride 8
                         _c(46, 64), _c(46, 128), _c(46, 128, 3)],           # 47-49: the Detect levels' inputs
            'head': [[[47, 48, 49], 1, 'Detect', ['nc', 'anchors']]]}


# where the layers under test and the feeders must lie: net layer -> (source tensor's channels, source offset,
# destination tensor's channels, destination offset)
CA, CB, CC, CD, CE = 424, 744, 808, 1720, 1216   # the wide level's concats
PLACES = {10: (248, 64, CA, 24), 11: (168, 40, CA, 160),
          17: (CA, 24, CB, 40), 18: (CA, 160, CB, 104), 19: (CB, 40, CD, 16), 20: (CB, 104, CD, 536),
          21: (CD, 16, CB, 232), 22: (CB, 232, CD, 800), 23: (CD, 536, CB, 424), 24: (CB, 424, CD, 1064),
          25: (CD, 800, CC, 104), 26: (CC, 104, CD, 1584), 27: (CD, 1064, CC, 8), 28: (CD, 1584, CC, 552),
          29: (CC, 8, CE, 32), 30: (CB, 104, CE, 104), 31: (CC, 552, CE, 224), 32: (CB, 40, CE, 360),
          33: (CB, 104, CE, 624), 34: (CC, 8, CE, 760), 35: (CB, 104, CE, 832)}


@functools.lru_cache(maxsize=None)
def edge_plan(sa):
    from models.yolo import Model
    from yv7.synthetic import synthetic_state_dict
    m = Model(copy.deepcopy(edge_net(sa)))
    m.load_state_dict(synthetic_state_dict(m, seed=7, calib_hw=128))
    m = m.float().eval().fuse().to(DEV).half()
    with pytest.MonkeyPatch.context() as mp:   # no sibling merges: every layer stays a GEMM of its own width
        mp.setenv('YV7_NO_MERGE', '1')
        mp.setenv('YV7_NO_TMERGE', '1')
        plan = m.plan()
    g = plan.graph
    assert g.stride == [8.0, 8.0, 8.0] and g.ops[0]['kind'] == L.OP_STEM and g.ops[0]['s'] == sa
    convs = {o['layers'][0][0]: o for o in g.ops if o['kind'] == L.OP_CONV}
    assert all(len(o['layers']) == 1 for o in convs.values()) and len(convs) == 40, sorted(convs)
    assert not any(o['kind'] in (L.OP_COPY, L.OP_ADD, L.OP_MAXPOOL) for o in g.ops)
    shape = lambda o: (o['cin'], o['cout'], o['k'], o['s'])   # noqa: E731
    for lay, want in LAYERS.items():
        assert shape(convs[lay]) == want, (lay, shape(convs[lay]), want)
    for lay, (cin, cout) in FEEDERS.items():
        assert shape(convs[lay]) == (cin, cout, 1, 1), (lay, shape(convs[lay]))
    for lay, want in PLACES.items():
        o = convs[lay]
        got = (g.tensors[o['src']][0], o['src_coff'], g.tensors[o['dst']][0], o['dst_coff'])
        assert got == want, (lay, got, want)
        assert o['src_coff'] > 0 and o['dst_coff'] > 0 and g.tensors[o['src']][0] != g.tensors[o['dst']][0]
    assert shape(convs[2]) == (64, 64, 3, 1) and shape(convs[4]) == (64, 120, 1, 1) and convs[9]['cout'] == 24
    assert any(o['dst_coff'] % 64 for o in convs.values()) and all(o['dst_coff'] % 8 == 0 for o in convs.values())
    # level 1 / wide / Detect levels at shifts 1, 2, 3 behind the (1, 2) stem and 2, 3, 3 behind the (2, 2) stem
    shifts = [g.tensors[convs[lay]['dst']][1] for lay in (2, 19, 46)]
    assert shifts == ([1, 2, 3] if sa == 1 else [2, 3, 3]), shifts
    return plan


# ---- what a forced variant must launch: csrc/conv_f16.hip forced_rows, with the rows of csrc/conv_f16_launch.h

# tile_rows: (BM, BN, WM, PF); conv_f16_kernel<BM, BN, WM, ONE, DET, PF, POOL>
T128x32, T128x64, T128x128, T256x32, T256x64 = (128, 32, 4, 1), (128, 64, 2, 1), (128, 128, 2, 1), (256, 32, 4, 1), (256, 64, 4, 1)
T128x64pf2, T128x128pf2 = (128, 64, 2, 2), (128, 128, 2, 2)
# ring_rows: (BM, BN, WM, WN, STAGES); conv_f16_ring_kernel<BM, BN, WM, WN, STAGES, ONE, DET>.  The first six are
# the configurations of the variants 100 + 10 * configuration + K splits.
RING_CFG = [(256, 256, 2, 4, 2), (256, 128, 4, 2, 3), (128, 128, 2, 2, 3), (128, 128, 2, 2, 2), (128, 64, 2, 2, 3),
            (256, 64, 4, 2, 3)]
R256x256, R256x128, R128x128s3, R128x128s2, R128x64, R256x64 = RING_CFG
R512x64, R256x128s2, R128x64s4 = (512, 64, 8, 1, 2), (256, 128, 4, 2, 2), (128, 64, 2, 2, 4)
# pring_rows: (BM, BN, WM, WN, STAGES, WS, occ); conv_f16_pring_kernel<BM, BN, WM, WN, STAGES, ONE, ACT, 64, WS, HOOK>
PRING = {201: (256, 256, 2, 4, 2, 0, 1), 202: (256, 128, 4, 2, 3, 0, 1), 203: (128, 128, 2, 2, 3, 0, 1),
         204: (128, 128, 2, 2, 2, 0, 2), 205: (256, 128, 4, 2, 2, 0, 1), 206: (128, 256, 2, 4, 2, 0, 1),
         234: (128, 256, 2, 4, 2, 4, 1), 235: (256, 128, 4, 2, 2, 4, 1), 236: (128, 128, 2, 4, 2, 8, 1),
         239: (256, 128, 4, 2, 3, 4, 1)}
TF = r'(true|false)'


def _tile(r):
    return 'tile', re.compile(rf'conv_f16_kernel<{r[0]}, {r[1]}, {r[2]}, {TF}, false, {r[3]}, false>$'), r[0], r[1]


def _ring(r):
    return 'ring', re.compile(rf'conv_f16_ring_kernel<{r[0]}, {r[1]}, {r[2]}, {r[3]}, {r[4]}, {TF}, false>$'), r[0], r[1]


def _pring(r):
    return ('pring', re.compile(rf'conv_f16_pring_kernel<{r[0]}, {r[1]}, {r[2]}, {r[3]}, {r[4]}, {TF}, \d, 64, {r[5]}, 0>$'),
            r[0], r[1])


def own_forms(v):
    """The kernels variant v launches where its form applies: [(family, key pattern, BM, BN)], the row of wide
    layers first, then forced_rows' rows for layers of at most 128 / 64 / 32 outputs."""
    if v == 1:   # csrc/conv.hip launch_conv: without a residual, variant 1 is that file's generic kernel
        return [('tile', re.compile(rf'(conv_kernel<_Float16, 128, {bn}, {TF}, false>$|.*conv_kernelIDF16_Li128ELi{bn}ELb[01]ELb0EE)'),
                 128, bn) for bn in (128, 64, 32)]
    if v in (2, 8):
        return [_tile(r) for r in {2: (T128x128, T256x64, T256x32), 8: (T128x128pf2, T128x64pf2, T128x32)}[v]]
    if v in (4, 5, 6, 7):
        return [_ring(r) for r in {4: (R256x128, R256x64), 5: (R256x256, R256x128s2, R512x64), 6: (R128x128s2, R128x64),
                                   7: (R128x128s3, R128x64s4)}[v]]
    if 100 <= v < 160:
        return [_ring(RING_CFG[(v - 100) // 10])]
    if v in PRING:
        return [_pring(PRING[v])]
    if v == 231:
        return [('p8', re.compile(rf'conv_f16_p8_kernel<{TF}, \d, 256, 256>$'), 256, 256)]
    if v == 232:
        return [('p8', re.compile(rf'conv_f16_p8n_kernel<{TF}, \d>$'), 256, 128)]
    return [('spatial', re.compile({10: r'conv3x3_halo_kernel<', 11: r'conv3x3_ws64_kernel<\d, 0, 4>$',
                                    15: r'conv3x3_ws64r_kernel<', 17: r'conv3x3_ws64_kernel<\d, 0, 8>$',
                                    262: r'conv3x3_hring2_kernel<'}[v]), 16, 128 if v == 262 else 64)]


def walk(v, M, cout, B, Ho, Wo, cus):
    """(T, walkers) of a persistent variant's launch: T tiles shared by `walkers` blocks that step through them.
    Restates the grid rules of csrc/conv_f16_pring.hip launch_pring (its PR_PLAIN, PR_WS and PR_WSN branches: grid =
    min(T, CUs * occ); min(M tiles, CUs); per N tile min(CUs / nN rounded down to 8, M tiles rounded up to 8), at
    least 8, blocks walking the M tiles), csrc/conv_f16_p8.hip launch_p8 (min(T, CUs)), csrc/conv_ws.hip
    launch_conv_ws64 (min(B * H/16 * W/16, CUs)) and csrc/conv_hring.hip launch_conv_hring (T = B * H/16 * W/16 *
    ceil(cout / 128), per = ceil(T / CUs) tiles per block, ceil(T / per) blocks)."""
    up = lambda a, b: (a + b - 1) // b   # noqa: E731
    if v in PRING:
        bm, bn, _, _, _, ws, occ = PRING[v]
        if v == 239:
            nN, T = up(cout, bn), up(M, bm)
            return T, max(8, min(cus // nN // 8 * 8, up(T, 8) * 8))
        if ws:
            return up(M, bm), min(up(M, bm), cus)
        T = up(M, bm) * up(cout, bn)
        return T, min(T, cus * occ)
    if v in (231, 232):
        T = up(M, 256) * up(cout, 256 if v == 231 else 128)
        return T, min(T, cus)
    if v in (11, 15, 17):
        T = B * (Ho // 16) * (Wo // 16)
        return T, min(T, cus)
    assert v == 262, v
    T = B * (Ho // 16) * (Wo // 16) * up(cout, 128)
    return T, up(T, up(T, cus))


def conv_ops(plan):
    return [i for i, o in enumerate(plan.graph.ops) if o['kind'] == L.OP_CONV]


def force(plan, v):
    for i in conv_ops(plan):
        plan.set_op_variant(i, v)


def launches(plan, sa, v, B, H, W, cus):
    """One record per conv op of the dry run of variant v on every conv: the kernel key, whether it is one of the
    variant's own forms, and the layer's GEMM sizes with the tile counts of that form."""
    g = plan.graph
    ks = plan.op_kernels(B, H, W)
    out = []
    for i in conv_ops(plan):
        o = g.ops[i]
        assert v == 0 or len(ks[i]) == 1, (v, i, ks[i])
        key = '|'.join(kernel_key(k) for k in ks[i])
        sh = g.tensors[o['dst']][1]
        Ho, Wo = H >> sh, W >> sh
        M = B * Ho * Wo
        r = dict(stem=sa, frame=(B, H, W), v=v, op=i, layer=o['layers'][0][0], key=key, cin=o['cin'], cout=o['cout'],
                 k=o['k'], s=o['s'], M=M, nk=(o['k'] * o['k'] * o['cin'] + 63) // 64, own=None)
        for fam, pat, bm, bn in own_forms(v) if v else []:
            if pat.match(key):
                r.update(own=fam, bm=bm, bn=bn)
                if v in PERSISTENT:
                    r['T'], r['walkers'] = walk(v, M, o['cout'], B, Ho, Wo, cus)
        out.append(r)
    return out


def describe(r):
    return (f'{r["cin"]}->{r["cout"]}' + (' 3x3' if r['k'] == 3 else '') + (' s2' if r['s'] == 2 else '') + f' nk {r["nk"]}' +
            (f' T {r["T"]}/{r["walkers"]}' if 'T' in r else ''))


def summary(recs):
    """Per variant: the kernels its own forms launched and the layers they launched on, grouped by M (T / grid: the
    tiles of a persistent launch over the blocks that walk them)."""
    lines = []
    for v in sorted({r['v'] for r in recs}):
        own = [r for r in recs if r['v'] == v and r['own']]
        lines.append(f'  variant {v}: own kernel on {len(own)} of {sum(r["v"] == v for r in recs)} convs')
        for key in sorted({r['key'] for r in own}):
            on = [r for r in own if r['key'] == key]
            lines.append(f'    {key}: ' + '; '.join(f'M {M}: ' + ', '.join(describe(r) for r in on if r['M'] == M)
                                                   for M in sorted({r['M'] for r in on}, reverse=True)))
    return lines


def check_zero_frames(plan, B, H, W, what):
    for t in range(len(plan.graph.tensors)):
        x = bordered(plan, t, B, H, W)
        assert not (x[:, 0].any() or x[:, -1].any() or x[:, :, 0].any() or x[:, :, -1].any()), \
            f'{what}: the zero frame of tensor {t} {tuple(x.shape)} was written'


def run_family(sa, fam, B, H, W):
    """Each variant of the family forced on every conv: the forward, check_ops, finite outputs, intact zero frames."""
    plan = edge_plan(sa)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    x = frames(B, H, W, seed=23).to(DEV).half()
    ops = plan.graph.ops
    recs, lines = [], []
    t0 = time.perf_counter()
    try:
        for v in FAMILIES[fam] if fam != 'tuned' else [0]:
            force(plan, v)
            recs += launches(plan, sa, v, B, H, W, cus)
            z, xs = plan.forward(x)
            torch.cuda.synchronize()
            out = check_ops(plan, x, B, H, W, raw=xs, z=z)
            assert ops[0]['kind'] == L.OP_STEM and 0 in out
            for i in conv_ops(plan):
                got = plan.tensor_view(ops[i]['dst'], B, H, W)[..., ops[i]['dst_coff']:ops[i]['dst_coff'] + ops[i]['cout']]
                assert torch.isfinite(got).all(), f'variant {v}: op {i} output not finite'
            assert torch.isfinite(z).all(), f'variant {v}: z not finite'
            check_zero_frames(plan, B, H, W, f'variant {v}')
            lines.append(f'  variant {v}: ' + kernel_summary(out))
    finally:
        force(plan, 0)
    wall = time.perf_counter() - t0
    print(f'\nstem {sa} {fam} B {B} {H}x{W}: {wall:.2f} s\n' + '\n'.join(lines + (summary(recs) if fam != 'tuned' else [])))
    return recs


GEMM_FAMILIES = [f for f in FAMILIES if f != 'spatial']


@pytest.mark.parametrize('B,H,W', RAGGED_FRAMES)
@pytest.mark.parametrize('fam', GEMM_FAMILIES)
@pytest.mark.parametrize('stem', STEMS)
def test_gemm_family_ragged(stem, fam, B, H, W):
    recs = run_family(stem[0], fam, B, H, W)
    assert any(r['own'] for r in recs)


@pytest.mark.parametrize('B,H,W', SQUARE_FRAMES)
@pytest.mark.parametrize('stem', STEMS)
def test_spatial_family(stem, B, H, W):
    recs = run_family(stem[0], 'spatial', B, H, W)
    assert any(r['own'] for r in recs)


@pytest.mark.parametrize('B,H,W', RAGGED_FRAMES + SQUARE_FRAMES)
@pytest.mark.parametrize('stem', STEMS)
def test_tuned_dispatch(stem, B, H, W):
    run_family(stem[0], 'tuned', B, H, W)


def test_stem_kernels():
    """The (1, 2) stem launches stem2_kernel, the (2, 2) stem stem_kernel; at B 8, 232 x 312 both have partial 8 x 16
    output tiles, and the (1, 2) form more of them than csrc/stem.hip stem_t has blocks (2 per CU)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B, H, W = RAGGED_FRAMES[0]
    for sa, name in ((1, 'stem2_kernel'), (2, 'stem_kernel')):
        ks = edge_plan(sa).op_kernels(B, H, W)[0]
        assert len(ks) == 1 and name in ks[0], (sa, ks)
        hb, wb = H // sa // 2, W // sa // 2
        assert hb % 8 and wb % 16, (sa, hb, wb)
    tiles = B * ((H // 2 + 7) // 8) * ((W // 2 + 15) // 16)
    assert tiles > 2 * cus and tiles % (2 * cus), f'{tiles} stem tiles on {cus} CUs: no block walks a second tile'


def split_grows_workspace(plan, i, v, B, H, W):
    """Variant v (two or four K splits) on op i alone needs split-K scratch that its one-split form does not."""
    lib = L.lib()
    try:
        plan.set_op_variant(i, v - v % 10)
        base = lib.yv7_workspace_bytes(plan._h, B, H, W)
        plan.set_op_variant(i, v)
        return lib.yv7_workspace_bytes(plan._h, B, H, W) > base
    finally:
        plan.set_op_variant(i, 0)


def test_launch_accounting():
    """Assertions 3-7 of the module's docstring, from dry runs of every variant on every frame and both stems."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert sorted(v for f in FAMILIES.values() for v in f) == sorted(VARIANTS), 'FAMILIES misses a CONV_VARIANTS entry'
    recs = []
    for sa, _ in STEMS:
        plan = edge_plan(sa)
        try:
            for v in VARIANTS:
                force(plan, v)
                for B, H, W in RAGGED_FRAMES + SQUARE_FRAMES:
                    recs += launches(plan, sa, v, B, H, W, cus)
        finally:
            force(plan, 0)
    ragged = [r for r in recs if r['frame'] in RAGGED_FRAMES]
    part_m = lambda r: r['M'] % r['bm'] != 0      # noqa: E731
    mask_n = lambda r: r['cout'] % r['bn'] != 0   # noqa: E731
    multi = lambda r: r['T'] > r['walkers'] and r['T'] % r['walkers'] != 0   # noqa: E731
    for v in VARIANTS:
        own = [r for r in recs if r['v'] == v and r['own']]
        print(f'variant {v}: own kernel on {len(own)} of {sum(r["v"] == v for r in recs)} launches' +
              (', walks ' + ', '.join(sorted({f'{r["T"]}/{r["walkers"]}' for r in own if multi(r)})) if v in PERSISTENT else ''))
        # 3. every form of the variant launched somewhere
        for fam, pat, bm, bn in own_forms(v):
            assert any(pat.match(r['key']) for r in own), f'variant {v}: {pat.pattern} launched on no layer'
        if v in SPATIAL:
            assert all(r['k'] == 3 and r['s'] == 1 for r in own), v
        else:
            # 4. partial M tiles and masked N tiles, at the ragged frames
            rg = [r for r in ragged if r['v'] == v and r['own']]
            assert any(part_m(r) for r in rg), f'variant {v}: no launch with a partial M tile'
            assert any(mask_n(r) for r in rg), f'variant {v}: no launch with a masked N tile'
            if own[0]['own'] != 'tile':
                assert any(part_m(r) and mask_n(r) for r in rg), f'variant {v}: no launch with both'
        # 5. more tiles than blocks, and no whole number of rounds
        if v in PERSISTENT:
            walked = [r for r in own if multi(r)]
            assert walked, f'variant {v}: no block walks a second tile on {cus} CUs: ' + \
                ', '.join(sorted({f'T {r["T"]} / {r["walkers"]}' for r in own}))
            if v == 231:
                assert any(r['k'] == 1 and r['nk'] % 2 == 0 for r in walked), '231: no walk on a 1x1 with even nk'
                assert any(r['k'] == 3 and r['nk'] % 2 == 0 for r in walked), '231: no walk on a 3x3 with even nk'
                assert any(r['nk'] % 2 == 1 for r in walked), '231: no walk with odd nk'
            if v == 232:
                assert any(r['nk'] % 3 == 0 for r in walked), '232: no walk with nk % 3 == 0'
                assert any(r['nk'] % 3 != 0 for r in walked), '232: no walk with nk % 3 != 0'
            if v in (202, 203, 239):
                assert any(r['nk'] % 3 != 0 for r in walked), f'{v}: no walk with nk % 3 != 0'
        # 6. K steps
        if v in (231, 232, 204, 6):
            assert {1, 2, 3, 5, 9} <= {r['nk'] for r in own}, (v, sorted({r['nk'] for r in own}))
            on34 = [r for r in recs if r['v'] == v and r['layer'] == 34]
            assert on34 and all((r['own'] is None and r['key'].startswith('conv_f16_kernel<')) == (v in (231, 232))
                                for r in on34), (v, [r['key'] for r in on34])
        # 7. the K splits split, on a partial M tile and a masked N tile
        if 100 <= v < 160 and v % 10 > 1:
            cand = [r for r in ragged if r['v'] == v and r['own'] and part_m(r) and mask_n(r) and r['nk'] >= v % 10]
            assert cand, f'variant {v}: no ragged layer with {v % 10} K steps'
            r = max(cand, key=lambda r: r['M'] * r['cout'])
            assert split_grows_workspace(edge_plan(r['stem']), r['op'], v, *r['frame']), \
                f'variant {v}: no split-K scratch for op {r["op"]} at {r["frame"]}'
