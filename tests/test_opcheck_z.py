"""tests/opcheck.py's raw-free z check (check_z_level) on a synthetic Detect level, no GPU: na 3, no 85, a
6 x 10 grid, B = 3.  It must accept what the project's logit tolerance allows (reference logits moved by a
uniform +-dl) and reject every way a head can misplace or miss rows: two adjacent rows swapped, two anchors
exchanged, a shift by one grid cell, one NaN, one image's rows never written.  Also _ulp_check's treatment of
non-finite values.  Reference computation: models/yolo.py:52-57 (Detect's decode).
"""
import pytest
import torch

from opcheck import _ulp_check, check_z_level, decode_ref

B, NY, NX, NA, NO = 3, 6, 10, 3, 85
STRIDE = 16.0
ANCHORS = torch.tensor([[36., 75.], [76., 55.], [72., 146.]], dtype=torch.float64)


@pytest.fixture(scope='module')
def level():
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(B, NY, NX, NA * NO, generator=g, dtype=torch.float64) * 2.0
    dl = 1e-4 * max(1.0, logits.abs().max().item())
    noise = (torch.rand(logits.shape, generator=g, dtype=torch.float64) * 2 - 1) * dl
    z = decode_ref(logits + noise, STRIDE, ANCHORS).float()
    return logits, z


def check(z, logits):
    return check_z_level(z, logits, STRIDE, ANCHORS, 'synthetic level')


def test_logits_within_dl_pass(level):
    logits, z = level
    assert z.shape == (B, NA * NY * NX, NO)
    worst = check(z, logits)
    print(f'\nlogits moved by a uniform +-dl: worst ratio to the bound {worst:.3g}')
    assert 0.05 < worst <= 1.0   # the bound is neither missed nor far from what +-dl uses of it
    assert check(decode_ref(logits, STRIDE, ANCHORS).float(), logits) < 0.05   # fp32 rounding of z alone


def test_swapped_rows_fail(level):
    logits, z = level
    bad = z.clone()
    bad[1, [77, 78]] = z[1, [78, 77]]
    with pytest.raises(AssertionError, match='beyond the bound'):
        check(bad, logits)


def test_exchanged_anchors_fail(level):
    logits, z = level
    hw = NY * NX
    bad = z.clone()
    bad[:, :hw], bad[:, hw:2 * hw] = z[:, hw:2 * hw], z[:, :hw]
    with pytest.raises(AssertionError, match='beyond the bound'):
        check(bad, logits)


def test_shift_by_one_cell_fails(level):
    logits, z = level
    with pytest.raises(AssertionError, match='beyond the bound'):
        check(torch.roll(z, 1, 1), logits)
    # the right values in the right rows with the grid of the neighbouring cell: x is off by one stride
    bad = z.clone()
    bad[..., 0] += STRIDE
    with pytest.raises(AssertionError, match='beyond the bound'):
        check(bad, logits)


def test_one_nan_fails(level):
    logits, z = level
    bad = z.clone()
    bad[2, 100, 40] = float('nan')
    with pytest.raises(AssertionError, match='1 of .* not finite'):
        check(bad, logits)


@pytest.mark.parametrize('sentinel', [float('nan'), -1.0e30, 0.0])
def test_unwritten_image_fails(level, sentinel):
    logits, z = level
    bad = z.clone()
    bad[1] = sentinel
    with pytest.raises(AssertionError):
        check(bad, logits)


def test_ulp_check_non_finite():
    ref = torch.linspace(-2, 2, 64)
    assert _ulp_check(ref.half(), ref, 'op', True) < 1e-3
    got = ref.half().clone()
    got[5] = float('nan')
    with pytest.raises(AssertionError, match='1 of 64 elements off .1 not finite'):
        _ulp_check(got, ref, 'op', True)
    got[5] = float('inf')
    with pytest.raises(AssertionError, match='1 not finite'):
        _ulp_check(got, ref, 'op', False)
    bad_ref = ref.clone()
    bad_ref[7] = float('nan')
    with pytest.raises(AssertionError, match='reference values not finite; its input: max .x. 3, finite True'):
        _ulp_check(ref.half(), bad_ref, 'op', True, xin=torch.full((4,), 3.0))
    with pytest.raises(AssertionError, match='reference values not finite'):
        _ulp_check(ref.half(), bad_ref, 'op', True)
