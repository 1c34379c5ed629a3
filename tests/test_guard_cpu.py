"""The guard-band harness (tests/guard.py) must be able to FAIL: fake "kernels" written in torch on CPU tensors - one
correct, the others each with one planted overrun or stray read - and the checks of tests/test_gpu_guard_bands.py
(`assert_intact` after the call; bit equality of the results with the outside poisoned "zero" / "nan" / "huge") accept
the first and reject each of the others at the right place.  Without this file the GPU tests could be vacuous."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guard import GUARD_ROWS, KINDS, Guarded, assert_same_bits, bits  # noqa: E402

M, N, LD = 5, 8, 16
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def _flat(g):
    """(flat buffer, offset of the window) - what a kernel gets as a raw pointer."""
    return g.buf, g.base


def k_correct(x, y):
    xb, xo = _flat(x)
    yb, yo = _flat(y)
    for r in range(M):
        yb[yo + r * y.ld: yo + r * y.ld + N] = xb[xo + r * x.ld: xo + r * x.ld + N] * 2


def k_past_last_row(x, y):
    k_correct(x, y)
    yb, yo = _flat(y)
    yb[yo + M * y.ld] = 1.0                       # row M, column 0


def k_column_n(x, y):
    k_correct(x, y)
    yb, yo = _flat(y)
    yb[yo + 2 * y.ld + N] = 1.0                   # row 2, the first guard column


def k_in_front(x, y):
    k_correct(x, y)
    yb, yo = _flat(y)
    yb[yo - 1] = 1.0


def k_other_nan(x, y):
    """writes a NaN - the sentinel's own float value - with another payload, one element past the window"""
    k_correct(x, y)
    yb, yo = _flat(y)
    last = yo + (M - 1) * y.ld + N
    b = bits(yb)
    b[last] = b[last] ^ 0x2                       # still a quiet NaN, payload changed


def k_reads_past_input(x, y):
    """the last row's sum runs one element too far: a stray read that only the poisoned runs can show"""
    k_correct(x, y)
    xb, xo = _flat(x)
    yb, yo = _flat(y)
    r = M - 1
    stray = xb[xo + r * x.ld + N].float().abs()
    y.view[r, 0] = torch.fmax(y.view[r, 0].float(), stray).to(y.dtype)        # fmax: a NaN operand is ignored


def _pair(dtype, ld_in=LD, ld_out=LD, **kw):
    g = torch.Generator().manual_seed(1)
    x = Guarded((M, N), dtype, "cpu", ld=ld_in, **kw)
    x.load(torch.randn(M, N, generator=g))
    y = Guarded((M, N), dtype, "cpu", ld=ld_out, **kw)
    return x, y


def _sweep(kernel, x, y):
    """What every GPU case does: three runs, guards checked after each, the three results compared bit for bit."""
    outs = {}
    for kind in KINDS:
        x.poison(kind)
        y.poison(kind).blank()
        kernel(x, y)
        x.assert_intact(f"input [{kind}]")
        y.assert_intact(f"output [{kind}]")
        outs[kind] = y.view.clone()
    assert_same_bits(outs["zero"], outs["nan"], "zero vs nan")
    assert_same_bits(outs["huge"], outs["nan"], "huge vs nan")
    assert torch.isfinite(outs["nan"].float()).all()
    return outs["nan"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_correct_kernel_passes(dtype):
    x, y = _pair(dtype)
    out = _sweep(k_correct, x, y)
    assert torch.equal(out.float(), (x.view * 2).float())
    # the guards are at least the persistent kernel's 256-row tile on both ends, and really hold the sentinel
    assert x.lead >= GUARD_ROWS * LD and x.trail >= GUARD_ROWS * LD
    assert int(x.outside.sum()) == x.buf.numel() - M * N


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel,row,col", [(k_past_last_row, M, 0), (k_column_n, 2, N), (k_in_front, -1, LD - 1),
                                            (k_other_nan, M - 1, N)])
def test_planted_overruns_are_caught_where_they_happen(dtype, kernel, row, col):
    x, y = _pair(dtype)
    kernel(x, y)
    x.assert_intact("input")
    with pytest.raises(AssertionError) as e:
        y.assert_intact("planted")
    m = re.search(r"planted: (\d+) element\(s\).*first at \(row (-?\d+), column (\d+)\)", str(e.value))
    assert m, str(e.value)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (1, row, col), str(e.value)
    # and in the three-run form, whatever the outside holds (a write of 1.0 is a change against zeros too)
    with pytest.raises(AssertionError):
        _sweep(kernel, *_pair(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_stray_read_is_caught_by_the_poisoned_runs(dtype):
    x, y = _pair(dtype)
    k_reads_past_input(x, y)                      # one run with the NaN sentinel alone: the max() swallows the stray value
    x.assert_intact("input")
    y.assert_intact("output")
    with pytest.raises(AssertionError, match="(zero|huge) vs nan"):
        _sweep(k_reads_past_input, *_pair(dtype))


def test_dense_rows_contiguous_window_and_one_dimension():
    x = Guarded((3, 4, N), torch.float32, "cpu")          # ld = None: contiguous
    assert x.view.is_contiguous() and x.view.shape == (3, 4, N) and x.rows == 12
    x.load(torch.arange(3 * 4 * N).float())
    x.assert_intact("contiguous")
    x.buf[x.base + 12 * N] = 0.0
    with pytest.raises(AssertionError, match=r"row 12, column 0"):
        x.assert_intact("contiguous")
    v = Guarded((10,), torch.int32, "cpu")
    v.load(torch.arange(10, dtype=torch.int32))
    v.assert_intact("vector")
    v.buf[v.base - 1] = 7
    with pytest.raises(AssertionError, match=r"row -1, column 9"):
        v.assert_intact("vector")
    s = Guarded((2, 3, N), torch.bfloat16, "cpu", ld=LD)  # leading axes packed on top of the row stride
    assert s.view.stride() == (3 * LD, LD, 1)


def test_integer_buffers_and_poison_kinds():
    for dtype in (torch.uint8, torch.int32):
        g = Guarded((M, N), dtype, "cpu", ld=LD)
        g.load(torch.ones(M, N, dtype=dtype))
        for kind in KINDS:
            g.poison(kind)
            g.assert_intact(kind)
            assert (g.view == 1).all()
        g.buf[g.base + N] += 2
        with pytest.raises(AssertionError, match=rf"row 0, column {N}"):
            g.assert_intact("int")
    f = Guarded((M, N), torch.float16, "cpu", ld=LD).poison("huge")
    out = f.buf[f.outside]
    assert torch.isfinite(out).all() and out.abs().min() == 65504 and (out > 0).any() and (out < 0).any()
    z = Guarded((M, N), torch.bfloat16, "cpu", ld=LD).poison("zero")
    assert (bits(z.buf)[z.outside] == 0).all()
    n = Guarded((M, N), torch.float32, "cpu", ld=LD)
    assert torch.isnan(n.buf).all() and int(bits(n.buf)[0]) == 0x7FC00123


def test_base_offset_leaves_only_the_promised_alignment():
    for dtype, off in ((torch.bfloat16, 16), (torch.float32, 16), (torch.uint8, 16), (torch.bfloat16, 2)):
        g = Guarded((M, N), dtype, "cpu", ld=LD, base_offset_bytes=off)
        rel = g.view.data_ptr() - g.buf.data_ptr()
        assert rel % 256 == off
        g.assert_intact("offset")
    with pytest.raises(ValueError):
        Guarded((M, N), torch.float32, "cpu", base_offset_bytes=2)


def test_assert_same_bits_tells_nan_payloads_and_signed_zeros_apart():
    a = torch.tensor([1.0, float("nan"), 0.0])
    b = a.clone()
    assert_same_bits(a, b, "same")
    c = a.clone()
    bits(c)[1] ^= 1
    with pytest.raises(AssertionError, match=r"first at \(1,\)"):
        assert_same_bits(a, c, "nan payload")
    d = a.clone()
    d[2] = -0.0
    with pytest.raises(AssertionError, match=r"first at \(2,\)"):
        assert_same_bits(a, d, "signed zero")
