"""The one-launch blocks on a real MI355X against answers that are known exactly (tests/block_cases.py), both libraries.

vx_ff_fused, vx_tblock_fused (+ vx_tblock_pack) and vx_audio_xattn (+ vx_audio_xattn_pack) run every step of a default clip; the
Gaussian tests of tests/test_gpu_kernels.py hold them to 2^-7 .. 2^-4 of the largest value on tensors that the residual
dominates.  Here every case has an answer that does not depend on the arithmetic (tests/test_block_cases_cpu.py shows on the CPU
that each mutant of the references below is caught and what the old bounds let through):

  block   case                      bound      what it pins
  ff      signs                     bit-equal  packing of W1 and W2, the value / gate interleave, colsum and bias order, residual, in place
  ff      rounding (output)         bit-equal  ONE rounding of the output (>= 1/4 ties, >= 1/4 other roundings)
  ff      rounding (h)              bit-equal  ONE rounding of h = value * gelu(gate) before W2 (>= 1/2 of the nonzero h rounded)
  ff      folded                    bit-equal  rstd (acc - mean colsum) + bias1 on both halves
  tblock  counted                   bit-equal  who is in the row sum (q = 0); f = 24: the 8 padded key rows weigh exactly 0
  tblock  routing (v from x)        bit-equal  which frame, head, pixel, item of V; pe row of the frame; pe added BEFORE the rounding
  tblock  routing (q, k from x)     bit-equal  which pixel, item, head of q and k
  tblock  tilted                    one ulp    the softmax scale (two logit levels ~4 bits apart)
  tblock  dense v / out-projection  bit-equal  every packed column of blocks 5-7 and of the three out-projection parts, bias_o
  tblock  dense q #v, dense k #v    bit-equal  every packed column of blocks 0-4, the shared M block included: 3 unit-vector tables at
                                               f = 16, 2 at f = 24 put every channel of a head under some frame's unit (<= 5 % of
                                               the (row, head) pairs have tied top keys or a winning logit >= 2^12 and are left out)
  tblock  own statistics            bit-equal  ln_stats == NULL: the kernel's two-pass statistics (rows with exact mean and variance)
  audio   counted                   bit-equal  5 tokens in the row sum, none of the padding slots; colsum of the ROUNDED Kq
  audio   routing                   bit-equal  which token, head, frame; alpha, bias_o inside alpha, ONE rounding
  audio   tilted                    one ulp    the scale log2(e) / sqrt(d)
  audio   dense out-projection      bit-equal  every packed VO column
  ("bit-equal": equal values of the element type; where the expected value is exactly 0, up to block_cases.LEAK_TOL = 2^-20 - a
  winner that leads by 40 bits leaves 2^-40 of the other rows, and gelu_f is 2^-30 instead of 0 under a gate of -128.)
stats_out / row_stats_out are held to float64 statistics of the rows the launch STORED under block_cases.stats_of: the two-part
sums under gemm_cases' rule for row_stats_out (equal where float32-exact, else N 2^-24 of the mass), (mean, rstd) under
norm_cases' rule for vx_row_stats (mean 2^-23, rstd 2^-16 relative; wider only where that rule's own derivation exceeds 2^-16 - rows that
are almost constant around their mean, as `counted` stores them - or a row's float32 sums are not exact; the widest used is printed:
7.6e-5 for the temporal block, 5.7e-4 for the audio block's constant `counted` rows, on both libraries).

Deviation |out - expected| that the CPU emulations of legitimate designs leave (float32 accumulation forwards, backwards, in two
halves; the row sum from the rounded P; the scaled row maximum rounded on its own; P normalised by a float32 reciprocal one ulp
off either way; the two-part statistics finished in float32; own statistics at either end of the row-statistics bound) - tests/test_block_cases_cpu.py prints them: 0 on every case of both element types, the two
`tilted` cases (one unit allowed) included.

Shapes, the smallest at which each kernel can still go wrong (vx_last_kernel() is asserted after every fused launch):
  ff_fused      m = 128 (one tile) and m = 128 (2 CUs + 3): a workgroup takes several tiles, the weight stream wraps, the tile
                count is uneven over the XCDs.  ff_fused_kernel<2>.
  tblock_fused  f = 16 (tblock_kernel<16>): (b, hw) = (1, 8), (2, 64), (3, 8 k);  f = 24 (tblock_kernel<24>): (1, 4), (2, 64), (3, 4 k),
                k the smallest odd number with 3 k tiles above the CU count (and no multiple of it; hw % 8 != 0 at f = 24).
  audio_xattn   C in {320, 640, 1280} x rows_per_frame in {16, 48, 256}, 3 frames: axattn_split_kernel; C = 320 with
                rows_per_frame = 4096, 3 frames: axattn_kernel<2>.  Statistics in as [rows, 2] (C = 320, 1280) and the two-part
                [rows, 4] (C = 640, every case); out of place with [rows, 2] out and in place with the two-part [rows, 4] out; a launch over
                the last two frames gives the bits of those rows.
  axattn_kernel<1> is reachable only through the VX_AX_FORM knob, which the library reads once per process: untested here.
x and out are column slices of wider buffers filled with a sentinel (row stride above the width, base 16 bytes into a row).
"""
import ctypes as C

import pytest
import torch

import block_cases as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 777.0


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from v_express_amd import lib as L, ops as o
    return L, o


@pytest.fixture(params=B.ELEMS, ids=lambda e: B.EL_NAME[e])
def ops_el(mods, request):
    """(lib, ops, element type): every test runs on the bfloat16 and on the float16 library."""
    L, o = mods
    with L.element_type(request.param):
        yield L, o, request.param


def last_kernel(ops):
    return ops._lib.vx_last_kernel().decode()


def cu_count(ops):
    info = (C.c_int32 * 4)()
    assert ops._lib.vx_device_info(torch.cuda.current_device(), info) == 0
    return int(info[0])


def column_slice(t):
    """t [rows, C] as columns 8 .. 8 + C of a [rows, C + 24] buffer full of FILL: (view, buffer)."""
    wide = torch.full((t.shape[0], t.shape[1] + 24), FILL, dtype=t.dtype, device=DEV)
    view = wide[:, 8:8 + t.shape[1]]
    view.copy_(t)
    return view, wide


def untouched(wide, width):
    return bool((wide[:, :8] == FILL).all()) and bool((wide[:, 8 + width:] == FILL).all())


WIDEST = {}         # test id -> the widest relative rstd tolerance block_cases.stats_of handed out (printed: 2^-16 is norm_cases' constant)


def check_stats(case, got_rows, st, parts, eps, what):
    want, tol = B.stats_of(got_rows.double(), parts, eps)
    if parts == 0:
        WIDEST[case.block] = max(WIDEST.get(case.block, 0.0), float((tol[:, 1] / want[:, 1]).max()))
    bad = ~((st.double() - want).abs() <= tol)
    if bool(bad.any()):
        r, j = (int(v) for v in bad.nonzero()[0])
        name = (("sum", "sum of squares") * 2)[j] + f" of half {j // 2}" if parts == 2 else ("mean", "rstd")[j]
        return (f"{case.block} {case.name} {case.shape} {what}: {int(bad.sum())} statistics wrong, first the {name} of {case.where(r, 0)}: "
                f"got {float(st[r, j])!r}, the stored row has {float(want[r, j])!r} (+- {float(tol[r, j]):.3g})")
    return None


# ----------------------------------------------------------------------------------------------------- ff
@pytest.mark.parametrize("tiles", ["one", "2 CUs + 3"])
def test_ff_fused(ops_el, tiles):
    _, ops, el = ops_el
    m = 128 if tiles == "one" else 128 * (2 * cu_count(ops) + 3)
    assert ops.ff_fused_applies(m, B.FF_C, B.FF_H)
    failures = []
    for case in B.ff_cases(el, m, DEV):
        k = B.ff_kernel_operands(case)
        x, wide = column_slice(k["x"])
        got = ops.ff_fused(x, k["w1"], k["b1"], k["colsum"], k["stats"], k["w2"], k["b2"])
        assert last_kernel(ops) == "ff_fused_kernel<2>", last_kernel(ops)
        assert got.data_ptr() == x.data_ptr() and untouched(wide, B.FF_C), f"ff {case.name}: not in place, or the sentinel columns changed"
        msg = case.first_wrong(got)
        if msg:
            failures.append(msg)
    assert not failures, f"{len(failures)} cases fail:\n" + "\n".join(failures)


# ----------------------------------------------------------------------------------------------------- tblock
def tb_shapes(f, cus):
    pix = 8 if f == 16 else 4
    k = cus // 3 + 1
    while k % 2 == 0 or (3 * k) % cus == 0:
        k += 1
    return {"one tile": (1, pix), "two items": (2, 64), "more tiles than CUs": (3, pix * k)}


@pytest.mark.parametrize("shape", ["one tile", "two items", "more tiles than CUs"])
@pytest.mark.parametrize("f", [16, 24])
def test_tblock_fused(ops_el, f, shape):
    _, ops, el = ops_el
    cus = cu_count(ops)
    b, hw = tb_shapes(f, cus)[shape]
    if shape == "more tiles than CUs":
        tiles = b * hw // (8 if f == 16 else 4)
        assert tiles > cus and tiles % cus and (f == 16 or hw % 8)
    assert ops.tblock_fused_applies(B.TB_C, B.HEADS, f, hw)
    failures = []
    for case in B.tb_cases(el, b, f, hw, DEV):
        k = B.tb_kernel_operands(case)
        x, wide = column_slice(k["x"])
        m = x.shape[0]
        given = k["stats"] is not None
        so = k["stats"].clone() if given else torch.full((m, 2), float("nan"), device=DEV)      # given: in place, as the model does
        got = ops.tblock_fused(x, k["wqkv"], k["bqkv"], k["colsum"], k["pe"], k["wo"], k["bo"], b=b, f=f, hw=hw,
                               heads=B.HEADS, stats=so if given else None, stats_out=so, eps=k["eps"])
        assert last_kernel(ops) == f"tblock_kernel<{f}>", last_kernel(ops)
        assert got.data_ptr() == x.data_ptr() and untouched(wide, B.TB_C), f"tblock {case.name}: not in place, or the sentinel columns changed"
        for msg in (case.first_wrong(got), check_stats(case, got, so, 0, k["eps"], "stats_out")):
            if msg:
                failures.append(msg)
    print(f"widest relative rstd tolerance so far: {WIDEST}")
    assert not failures, f"{len(failures)} checks fail:\n" + "\n".join(failures)


# ----------------------------------------------------------------------------------------------------- audio cross-attention
AX_SHAPES = [(c, rpf, "axattn_split_kernel") for c in (320, 640, 1280) for rpf in (16, 48, 256)] + [(320, 4096, "axattn_kernel<2>")]


@pytest.mark.parametrize("c,rpf,kernel", AX_SHAPES)
def test_audio_xattn(ops_el, c, rpf, kernel):
    _, ops, el = ops_el
    frames, m = 3, 3 * rpf
    assert ops.audio_xattn_applies(c, B.HEADS, B.TOKENS, rpf)
    failures = []
    for case in B.ax_cases(el, c, frames, rpf, DEV, fmt=4 if c == 640 else 2):
        k = B.ax_kernel_operands(case)
        fold = ops.audio_xattn_pack(k["kv"], k["wq"], k["bq"], k["wo"], frames=frames, n_ctx=B.TOKENS, heads=B.HEADS)
        x, xwide = column_slice(k["x"])
        out, owide = column_slice(torch.zeros_like(k["x"]))
        so2 = torch.full((m, 2), float("nan"), device=DEV)
        ops.audio_xattn(x, k["stats"], fold, k["bo"], k["alpha"], rows_per_frame=rpf, stats_out=so2, out=out)
        assert last_kernel(ops) == kernel, last_kernel(ops)
        assert torch.equal(x, k["x"]) and untouched(xwide, c) and untouched(owide, c), f"audio {case.name}: x or the sentinel columns changed"
        # in place, the two-part statistics out (over the ones read where those are two-part)
        so4 = k["stats"].clone() if k["stats"].shape[1] == 4 else torch.full((m, 4), float("nan"), device=DEV)
        got = ops.audio_xattn(x, so4 if k["stats"].shape[1] == 4 else k["stats"], fold, k["bo"], k["alpha"], rows_per_frame=rpf, stats_out=so4)
        assert got.data_ptr() == x.data_ptr() and untouched(xwide, c)
        if not torch.equal(got, out):
            failures.append(f"audio {case.name} {case.shape}: the in-place launch differs from the out-of-place one")
        # the last two frames alone: the bits of those rows
        sub = ops.audio_xattn_pack(k["kv"][B.TOKENS:], k["wq"], k["bq"], k["wo"], frames=frames - 1, n_ctx=B.TOKENS, heads=B.HEADS)
        o2 = torch.empty((m - rpf, c), dtype=el, device=DEV)
        ops.audio_xattn(k["x"][rpf:], k["stats"][rpf:].contiguous(), sub, k["bo"], k["alpha"], rows_per_frame=rpf, out=o2)
        if not torch.equal(o2, out[rpf:]):
            failures.append(f"audio {case.name} {case.shape}: a launch over the last two frames differs from those rows of the full launch")
        for msg in (case.first_wrong(out), check_stats(case, out, so2, 0, 1e-5, "row_stats_out [rows, 2]"),
                    check_stats(case, out, so4, 2, 1e-5, "row_stats_out [rows, 4]")):
            if msg:
                failures.append(msg)
    print(f"widest relative rstd tolerance so far: {WIDEST}")
    assert not failures, f"{len(failures)} checks fail:\n" + "\n".join(failures)
