"""The stepped pixel index of the register-weight conv kernels, restated in numpy and checked against the
closed form (no GPU).

conv_w1.hip decomposes only a tile's first pixel m0 (Div24 multiply-highs, yv7_kernels.h) and derives every
lane's bordered index from per-tile scalars by compares (tile_base / step_pix); conv_s2.hip decomposes a tile
index into (column group, row group, image group) with the same multiply-highs, indexes the lane's pixel of the
tile's first row from a per-tile scalar plus a launch-invariant lane part, and steps rows by the bordered row
pitch.  An off-by-one in a wrap threshold shows here: every pixel of every tile for H, W in 4 .. 160 step 4,
B in 1 .. 9 and every tile size the kernels' configuration tables hold.

Closed form (conv_w1.hip header): pixel m of a [B][H][W] tensor sits at bordered index
m + 2 r + (2 b + 1)(W + 2) + 1 with r = m // W, b = r // H.
"""
import numpy as np
import pytest

NWR = 2                              # conv_w1.hip: row wraps inside a tile the stepped index covers
W1_TPX = (32, 64, 128, 256)          # PG * TPF * 16 over w1_rows
SIZES = range(4, 161, 4)
BATCHES = range(1, 10)


def make_div24(d):
    s = 0
    while (1 << s) < d:
        s += 1
    return ((1 << (24 + s)) + d - 1) // d, s


def div24(n, mul, sh):
    n = np.asarray(n, dtype=np.uint64)
    hi = (((n << np.uint64(8)) & np.uint64(0xffffffff)) * np.uint64(mul)) >> np.uint64(32)
    return (hi >> np.uint64(sh)).astype(np.int64)


def closed_form(m, H, W):
    r = m // W
    b = r // H
    return m + 2 * r + (2 * b + 1) * (W + 2) + 1


def _div24_exact(d, top):
    # the quotient is monotone in n, so it is exact on [0, top) iff it is exact on both sides of every multiple
    mul, sh = make_div24(d)
    assert mul < (1 << 32) and sh < 32
    k = np.arange(0, top // d + 1, dtype=np.int64) * d
    n = np.concatenate([k, k[1:] - 1, np.array([top - 1])])
    n = n[n < top]
    assert np.array_equal(div24(n, mul, sh), n // d), d


def test_div24_exact():
    for d in range(1, 321):              # every divisor the tests' shapes use, over more than their pixel counts
        _div24_exact(d, 1 << 19)
    for d in (1, 3, 4, 7, 20, 40, 80, 96, 160, 1000, 4095, 4096, 4097, 65535, 65536, (1 << 24) - 1, 1 << 24):
        _div24_exact(d, 1 << 24)         # the kernels' whole range (M < 2^24)


def stepped_w1(H, W, M, TPX):
    """Bordered index of every pixel m < ceil(M / TPX) * TPX as conv_w1.hip computes it (-1: past the tensor)."""
    T = (M + TPX - 1) // TPX
    m0 = np.arange(T, dtype=np.int64) * TPX
    R0 = div24(m0, *make_div24(W))
    c0 = m0 - R0 * W
    b0 = div24(R0, *make_div24(H))
    h0 = R0 - b0 * H
    idx = m0 + 2 * R0 + (2 * b0 + 1) * (W + 2) + 1
    t1 = W - c0
    tb = (H - h0) * W - c0
    rem = M - m0
    rep = lambda a: np.repeat(a, TPX)
    off = np.tile(np.arange(TPX, dtype=np.int64), T)
    s = rep(idx) + off
    for w in range(NWR):
        s += 2 * (off >= rep(t1) + w * W)
    s += 2 * (W + 2) * (off >= rep(tb))
    return np.where(off < rep(rem), s, -1)


@pytest.mark.parametrize('TPX', W1_TPX)
def test_w1_stepped_index_matches_closed_form(TPX):
    checked = 0
    for W in SIZES:
        if not TPX - 2 < NWR * W:       # the kernel keeps the per-lane decomposition there
            continue
        for H in SIZES:
            assert H >= NWR
            # the index of a pixel does not depend on B; B only moves the tensor's end (rem), so check the
            # whole 9-image tensor once and every smaller batch's last tile and end
            M9 = 9 * H * W
            got = stepped_w1(H, W, M9, TPX)
            m = np.arange(len(got), dtype=np.int64)
            want = np.where(m < M9, closed_form(m, H, W), -1)
            assert np.array_equal(got, want), (H, W, TPX)
            for B in BATCHES:
                M = B * H * W
                t0 = (M - 1) // TPX * TPX
                tail = stepped_w1(H, W, M, TPX)[t0:]
                mt = np.arange(t0, t0 + TPX, dtype=np.int64)
                assert np.array_equal(tail, np.where(mt < M, closed_form(mt, H, W), -1)), (B, H, W, TPX)
            checked += 1
    assert checked


def test_w1_dma_swizzle_term_is_launch_invariant():
    # piece k = wave + 8 mm covers pixels 8 (k % PPC) + lane / 8; the source swizzle (px >> 1) & 7 equals
    # 4 (wave & 1) | lane / 16 for every piece because PPC = TPX / 8 is even
    for TPX in W1_TPX:
        PPC = TPX // 8
        assert PPC % 2 == 0
        for IC in (1, 2, 4, 8):
            for mm in range(max(IC * TPX // 64, 1)):
                for wave in range(8):
                    for lane in range(64):
                        k = wave + 8 * mm
                        px = (k % PPC) * 8 + (lane >> 3)
                        assert (px >> 1) & 7 == (4 * (wave & 1)) | (lane >> 4)
                        assert (lane & 7) ^ ((px >> 1) & 7) == (lane & 7) ^ (lane >> 4) ^ (4 * (wave & 1))


def pix_index(b, h, w, H, W):
    return (b * (H + 2) + h + 1) * (W + 2) + w + 1


S2_TILES = [(2, 2), (4, 2), (4, 1), (2, 1), (8, 1), (2, 4), (4, 4)]   # (TM, PG) over conv_s2.hip s2_rows


@pytest.mark.parametrize('TM,PG', S2_TILES)
def test_s2_stepped_store_index_matches_closed_form(TM, PG):
    """conv_s2.hip's epilogue: tile t -> (cg, y0, b0) by two Div24 divisions; the lane (image img, column
    4 pg + c of the tile) stores row i at ybase(tile) + y_lane + i (W + 2), dead when img >= B - b0.  Every output
    pixel of the tensor must be written exactly once, at its closed-form index."""
    checked = 0
    for W in range(8, 161, 8):          # (a row step has no wrap to get wrong: a coarser grid than the 1x1's)
        if W % (4 * PG):
            continue
        for H in range(8, 161, 8):
            if H % TM:
                continue
            ncg, nrg = W // (4 * PG), H // TM
            t = np.arange(3 * nrg * ncg, dtype=np.int64)            # B = 9: three image groups
            tq = div24(t, *make_div24(ncg))
            ig = div24(tq, *make_div24(nrg))
            assert np.array_equal(tq, t // ncg) and np.array_equal(ig, t // ncg // nrg)
            cg, y0, b0 = t - tq * ncg, (tq - ig * nrg) * TM, ig * 4
            ybase = pix_index(b0, y0, cg * 4 * PG, H, W)[:, None, None, None]
            img = np.arange(4, dtype=np.int64)[None, :, None, None]
            xl = np.arange(4 * PG, dtype=np.int64)[None, None, :, None]
            i = np.arange(TM, dtype=np.int64)[None, None, None, :]
            got = ybase + (img * (H + 2) * (W + 2) + xl) + i * (W + 2)
            m = ((b0[:, None, None, None] + img) * H + y0[:, None, None, None] + i) * W + cg[:, None, None, None] * 4 * PG + xl
            assert np.array_equal(got, closed_form(m, H, W)), (H, W)
            for B in BATCHES:
                live = np.broadcast_to(img < B - b0[:, None, None, None], got.shape)
                assert np.array_equal(np.bincount(m[live], minlength=B * H * W), np.ones(B * H * W, dtype=np.int64)), (B, H, W)
            checked += 1
    assert checked
