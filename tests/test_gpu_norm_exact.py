"""The kernels of csrc/vx_norm.hip on a real MI355X against answers that are known exactly (tests/norm_cases.py), both libraries.

The Gaussian tests accept max|err| <= 2^-6 max|ref| and relative L2 <= 8e-3 (LayerNorm 2^-7 / 6e-3): a wrong eps, the unbiased
variance, a truncating store, and at 4096 x 320 a whole group normalised with its neighbour's statistics stay inside
(tests/test_norm_cases_cpu.py measures it).  Here every (frame, group) / row holds one quarter m - 1.5 s and three quarters
m + 0.5 s at hashed positions: mean = m, var + eps = s^2 and every float32 sum are exact in any order.

  case           bound                                                       what it pins
  counted        workspace totals per (frame, group) equal; two-part sums    every pixel, channel, frame, slice tail, source and
                 equal; vx_row_stats / _finalize: mean 2^-23, rstd 2^-16     group index of the statistics
                 relative (float32 1/c, one product, 1-ulp rsqrt, the
                 cancellation of E[x^2] - mean^2 at |m| <= 6)
  affine         equal                                                       mean, rstd, eps, the population variance, the group /
                                                                             row of the statistics, gamma / beta / table indexing,
                                                                             the padded destination
  rounding       equal (>= 1/4 ties, >= 1/4 other roundings)                 round-to-nearest-even and ONE rounding
  activated      equal at argument 0 and from 32 on; |out| <= 2^-40 |arg|    that the activation runs, which one, on which
                 from -32 down; else one of the two neighbours of the        channels, after the affine
                 float64 answer
  any partition  equal to affine                                             gn_group_stats on 1, 3, 8, 9, 64, 67 hand-made partial sums
  folded         w_out, bias_out equal (n = 40, (2, 256, 320) and (2, 1024,  the one rounding of the scaled weight, the mean of the
                 320)); gemm on the folded weights == groupnorm + gemm ==    right group per channel, n no multiple of 32, frames > 1
                 the exact answer at (2, 1024, 320), n = 3840 only: grouped
                 weights need 192 tiles of the persistent kernel
  producer chain equal                                                       the apply-only route on a producer's sums; stale sums
                                                                             dropped when the tensor is overwritten
  quantised      bytes equal, scale 2^-22 relative, K padding zero           the per-row scale, the zero fill, the table on this path

"Equal" is torch.equal on the raw bits.  Strided operands (the LayerNorm family's ldx / ldo) are column slices of wider buffers
filled with 777 at a base 16 bytes into a row; GroupNorm's contiguous tensors sit between two guard frames of 777.  The
references are norm_cases' float64 restatements evaluated with torch on the device (their builders assert their conditions there).
"""
import pytest
import torch

import gemm_cases as G
import norm_cases as N

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 777.0
ACT = {"none": 0, "silu": 1, "gelu": 2}


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from v_express_amd import lib as L, ops as o
    return L, o


@pytest.fixture(params=N.ELEMS, ids=lambda e: N.EL_NAME[e])
def ops_el(mods, request):
    """(lib module, ops, element type): every test runs on the bfloat16 and on the float16 library."""
    L, o = mods
    with L.element_type(request.param):
        yield L, o, request.param


def to_el(x, el):
    return x.to(torch.float32).to(el)


def column_slice(t, dtype=None):
    """t [rows, C] as columns 8 .. 8 + C of a [rows, C + 24] buffer of FILL (a shape: an output): a row stride above the width
    and a base 16 bytes into a row - the alignment the ABI promises, no more."""
    rows, c = t.shape if isinstance(t, torch.Tensor) else t
    wide = torch.full((rows, c + 24), FILL, dtype=dtype or t.dtype, device=DEV)
    view = wide[:, 8:8 + c]
    if isinstance(t, torch.Tensor):
        view.copy_(t)
    return view, wide


def fill_intact(wide, c):
    return bool((wide[:, :8] == FILL).all()) and bool((wide[:, 8 + c:] == FILL).all())


def guarded(frames, hw, c, el, src=None):
    """[frames, hw, c] between two guard frames of FILL -> (view, whole buffer)."""
    buf = torch.full((frames + 2, hw, c), FILL, dtype=el, device=DEV)
    if src is not None:
        buf[1:-1].copy_(src)
    return buf[1:-1], buf


def guards_intact(buf):
    return bool((buf[0] == FILL).all()) and bool((buf[-1] == FILL).all())


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def gn_operands(case):
    g, el = case.geo, case.el
    x = to_el(case.x(), el)
    x1, b1 = guarded(g.frames, g.hw, g.c1, el, x[..., :g.c1])
    x2, b2 = guarded(g.frames, g.hw, g.c2, el, x[..., g.c1:]) if g.c2 else (None, None)
    return x1, x2, [b for b in (b1, b2) if b is not None], case.gamma.float(), case.beta.float()


def run_gn(ops, case):
    """One case on its kernel -> (name -> output, failure text or None for the guards and the padded form)."""
    g, el = case.geo, case.el
    x1, x2, bufs, gamma, beta = gn_operands(case)
    kw = dict(frames=g.frames, hw=g.hw, groups=g.groups)
    got, note = {}, None
    if case.name == "counted":
        ws, slices = ops.groupnorm_stats(x1, x2=x2, **kw)
        tot = ws.view(g.frames, slices, g.groups, 2).double().sum(dim=1)
        got["sums"], got["squares"] = tot[..., 0], tot[..., 1]
    else:
        out, obuf = guarded(g.frames, g.hw, g.c, el)
        ops.groupnorm(x1, gamma, beta, eps=case.eps, silu=ACT[case.act], x2=x2, out=out, **kw)
        got["out"] = out
        bufs.append(obuf)
        if g.pad:
            H, W = g.pad
            for _ in range(2):                          # twice: the persistent image is reused
                img = ops.groupnorm(x1, gamma, beta, eps=case.eps, silu=ACT[case.act], x2=x2, pad_hw=g.pad, **kw)
            img = img.view(g.frames, H + 2, W + 2, g.c)
            if not bits_equal(img[:, 1:-1, 1:-1], out.view(g.frames, H, W, g.c)):
                note = "the interior of the padded image differs from the unpadded call"
            if not (bool((img[:, 0] == 0).all()) and bool((img[:, -1] == 0).all()) and bool((img[:, :, 0] == 0).all())
                    and bool((img[:, :, -1] == 0).all())):
                note = "the border of the padded image is not zero"
    torch.cuda.synchronize()
    if not all(guards_intact(b) for b in bufs):
        note = "a guard frame was written"
    return got, note


@pytest.mark.parametrize("geo", N.GN_GEOS, ids=lambda g: g.text())
def test_groupnorm(ops_el, geo):
    L, ops, el = ops_el
    failures = []
    for s in N.SCALES:
        for case in N.gn_cases(geo, el, s, DEV):
            got, note = run_gn(ops, case)
            msg = case.first_wrong(got, case.wants()) or (note and f"{case.title()}: {note}")
            if msg:
                failures.append(msg)
    assert not failures, f"{len(failures)} (kernel, shape, case) triples fail:\n" + "\n".join(failures)


def _apply(L, ops, case, x, ws, stat_slices, out):
    g = case.geo
    gamma, beta = case.gamma.float(), case.beta.float()       # (named: they must outlive the call that takes their addresses)
    L.check(ops._lib.vx_groupnorm_apply(ops._ptr(x), g.c, None, 0, g.frames, g.hw, g.groups, float(case.eps), ops._ptr(gamma),
                                        ops._ptr(beta), 0, ops._ptr(out), ops._ptr(ws), stat_slices, ops._gn_slices(g.hw), g.hw, 0,
                                        ops._stream()), "vx_groupnorm_apply")
    torch.cuda.synchronize()


def fold_operands(case, n):
    """Integer weights in [-3, 3] and biases; gamma = +-2^k s on seven channels of eight (w gamma rstd an integer) and
    (1 + 2^-(p-1)) s on the eighth, where w = +-3 is a tie of the element type: the ONE rounding.  Every term of the bias dot is a
    multiple of 2^-(p-1) and their absolute sum stays below 2^(25-p): exact in float32 in any order."""
    g, el, dev = case.geo, case.el, case.dev
    p = N.SIG_BITS[el]
    ch = N._ar(g.c, dev)
    h = N._hash(51, ch)
    gamma = torch.where(h % 8 == 0, 1.0 + 2.0 ** -(p - 1), N._pm(h) * torch.exp2((h >> 4) % 2).double()) * case.s
    w = (N._hash(52, N._ar(n, dev)[:, None], ch[None, :]) % 7 - 3).double()
    bb = (N._hash(53, N._ar(n, dev)) % 17 - 8).double()
    mean = N.group_mean(N._ar(g.frames, dev)[:, None], (ch // g.cg)[None, :])              # [frames, C]
    w_out = N.round_el(w[None] * (gamma / case.s)[None, None, :], el).expand(g.frames, n, g.c).contiguous()   # rstd = 1 / s, every frame
    terms = w_out * mean[:, None, :]
    assert float(terms.abs().sum(-1).max()) < 2.0 ** (25 - p) and bool((terms * 2.0 ** (p - 1) == torch.round(terms * 2.0 ** (p - 1))).all())
    ties, _ = N.tie_shares(w[None] * (gamma / case.s)[None, None, :], el)
    assert ties > 0.02, ties
    return gamma, w, bb, w_out, bb[None] - terms.sum(-1)


@pytest.mark.parametrize("geo", N.CHAIN_GEOS + [N.Gn(3, 100, 320)], ids=lambda g: g.text())
def test_any_partition_and_fold(ops_el, geo):
    """vx_groupnorm_apply and vx_groupnorm_fold_linear on the exact totals handed over as 1, 3, 8, 9, 64 and 67 hand-made partial
    sums per frame (fewer than, exactly and no multiple of the GN_SUBS = 8 strided re-reduction; the apply pass's own slices differ
    from them): the apply output equals `affine` / `rounding`, the folded weights and biases equal their exact values."""
    L, ops, el = ops_el
    failures = []
    n = 40                                              # 32 rows per block: a second, ragged block
    for s in N.SCALES:
        for build in (N.affine, N.rounding):
            case = build(geo, el, s, DEV)
            tot = N.counted(geo, el, s, DEV).values()
            x = to_el(case.x(), el)
            want = case.wants()
            gamma, w, bb, w_want, b_want = fold_operands(case, n)
            for parts in N.PARTITIONS:
                ws = N.partitions(tot["sums"], tot["squares"], parts, DEV)
                out, obuf = guarded(geo.frames, geo.hw, geo.c, el)
                _apply(L, ops, case, x, ws, parts, out)
                torch.cuda.synchronize()
                msg = case.first_wrong({"out": out}, want) or (None if guards_intact(obuf) else f"{case.title()}: a guard frame was written")
                if msg:
                    failures.append(f"vx_groupnorm_apply on {parts} partial sums: {msg}")
                if build is N.affine:
                    w_f, b_f = ops.groupnorm_fold_linear(ws, gamma.float(), to_el(w, el), bb.float(), frames=geo.frames, hw=geo.hw,
                                                         groups=geo.groups, eps=case.eps, slices=parts)
                    if not bits_equal(w_f, to_el(w_want, el)):
                        bad = (w_f.view(torch.int16) != to_el(w_want, el).view(torch.int16)).nonzero()
                        i = tuple(bad[0].tolist())
                        failures.append(f"vx_groupnorm_fold_linear on {parts} partial sums, {case.title()}: w_out wrong, "
                                        f"{len(bad)} elements, first at {i}: got {float(w_f[i])!r}, want {float(w_want[i])!r} "
                                        f"(w {float(w[i[1:]])!r}, gamma {float(gamma[i[2]])!r})")
                    if not torch.equal(b_f.double(), b_want):
                        bad = (b_f.double() != b_want).nonzero()
                        failures.append(f"vx_groupnorm_fold_linear on {parts} partial sums, {case.title()}: bias_out wrong, "
                                        f"{len(bad)} elements, first at {tuple(bad[0].tolist())}: got {float(b_f[tuple(bad[0])])}, "
                                        f"want {float(b_want[tuple(bad[0])])}")
    assert not failures, f"{len(failures)} fail:\n" + "\n".join(failures)


def test_folded_end_to_end(ops_el):
    """The second half of `folded`: gemm(x, w_f, rowbias=b_f, w_group_rows=hw) on the fold kernel's own output equals groupnorm +
    gemm, and both equal the exact answer bit for bit.  Grouped weights need the persistent 256 x 320 kernel, which takes a launch
    from 192 tiles of the nominal two-item launch on (ops.RING_MIN_TILES): inside frame_rows(1024, items=1), 2 x 1024 rows x
    n = 3840 are 16 x 12 of them, so this half runs at (2, 1024, 320) only - (2, 256, 320) would need n = 15360 - and the route is
    asserted.  Integer weights in [-3, 3], gamma rstd = +-1 / +-2, beta and bias integers: GroupNorm's output (multiples of 1/2 up
    to 14) is representable, every term of either GEMM is a multiple of 1/2 and every partial sum stays below 2^15 - exact in
    float32 in any order, rounded once."""
    L, ops, el = ops_el
    geo, n = N.CHAIN_GEOS[1], 3840
    dev, hw, m = DEV, geo.hw, geo.frames * geo.hw
    ch = N._ar(geo.c, dev)
    h = N._hash(54, ch)
    w = (N._hash(52, N._ar(n, dev)[:, None], ch[None, :]) % 7 - 3).double()
    bias = (N._hash(53, N._ar(n, dev)) % 17 - 8).double()
    beta = ((h >> 8) % 5 - 2).double()
    for s in N.SCALES:
        gamma = N._pm(h) * torch.exp2((h >> 4) % 2).double() * s
        x64 = N.gn_input(geo, s, dev)
        ref = N.gn_forward(geo, x64, gamma, beta, geo.eps(s), el)
        gn64 = ref["arg"].view(m, geo.c)
        assert N._representable(gn64, el) and float((gn64.abs() @ w.abs().t()).max()) < 2.0 ** 15
        want = to_el(N.round_el(gn64 @ w.t() + bias, el), el)
        x = to_el(x64, el)
        with ops.frame_rows(hw, items=1):
            ws, sl = ops.groupnorm_stats(x, frames=geo.frames, hw=hw, groups=geo.groups)
            w_f, b_f = ops.groupnorm_fold_linear(ws, gamma.float(), to_el(w, el), (bias + w @ beta).float(), frames=geo.frames, hw=hw,
                                                 groups=geo.groups, eps=geo.eps(s), slices=sl)
            with ops.GemmProfile() as prof:
                folded = ops.gemm(x.view(m, geo.c), w_f, None, rowbias=b_f, rows_per_group=hw, w_group_rows=hw)
            gemms = [r for r in prof.records if len(r) == 7 and isinstance(r[4], tuple)]
            assert len(gemms) == 1 and gemms[0][3] == G.RING, f"route moved: {[r[3] for r in gemms]}"
            normed = ops.groupnorm(x, gamma.float(), beta.float(), frames=geo.frames, hw=hw, groups=geo.groups, eps=geo.eps(s), silu=0)
            assert bits_equal(normed.view(m, geo.c), to_el(gn64, el)), "groupnorm() misses the exact answer"
            unfused = ops.gemm(normed.view(m, geo.c), to_el(w, el), bias.float())
        for name, got in (("gemm on the folded weights", folded), ("groupnorm + gemm", unfused)):
            bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
            assert len(bad) == 0, (f"s={s:g} [{N.EL_NAME[el]}] {name}: {len(bad)} of {got.numel()} wrong, first at {tuple(bad[0].tolist())}: "
                                   f"got {float(got[tuple(bad[0])])!r}, want {float(want[tuple(bad[0])])!r}")


@pytest.mark.parametrize("geo", N.CHAIN_GEOS, ids=lambda g: g.text())
def test_producer_chain(ops_el, geo):
    """x -> gemm(identity weight, gn=(32, hw)) leaves GroupNorm sums on its output (the 64 x 160 tile at these sizes: asserted):
    groupnorm() then runs the apply pass only and must equal the exact answer and the call that takes its own statistics.  The
    same out= tensor overwritten by a launch that leaves no sums must lose them: the next groupnorm() answers for the NEW contents."""
    L, ops, el = ops_el
    kw = dict(frames=geo.frames, hw=geo.hw, groups=geo.groups)
    eye = torch.eye(geo.c, device=DEV, dtype=el)
    for s in N.SCALES:
        for build in (N.affine, N.rounding):
            case = build(geo, el, s, DEV)
            gamma, beta = case.gamma.float(), case.beta.float()
            x = to_el(case.x(), el).view(-1, geo.c)
            o = torch.empty_like(x)
            with ops.GemmProfile() as prof:
                ops.gemm(x, eye, None, gn=(geo.groups, geo.hw), out=o)
            gemms = [r for r in prof.records if len(r) == 7 and isinstance(r[4], tuple)]
            assert len(gemms) == 1 and gemms[0][3] == G._k(G.T64), f"route moved: {[r[3] for r in gemms]}"
            st = ops.gn_of(o)
            assert st is not None and st.fits(geo.frames, geo.hw, geo.groups, geo.c), "the launch left no GroupNorm sums"
            assert bits_equal(o, x)
            with ops.OpProfile() as oprof:
                fused = ops.groupnorm(o, gamma, beta, eps=case.eps, silu=0, **kw)
            assert [r[0] for r in oprof.records] == ["groupnorm_apply"], oprof.records
            plain = ops.groupnorm(o.clone(), gamma, beta, eps=case.eps, silu=0, **kw)
            want = case.wants()
            for name, t in (("apply-only", fused), ("own statistics", plain)):
                msg = case.first_wrong({"out": t}, want)
                assert msg is None, f"{name}: {msg}"
            assert bits_equal(fused, plain)
            # new contents (the next frames of the same hash), no statistics from this launch
            x2 = to_el(N.gn_input(geo, s, DEV, frame0=geo.frames), el).view(-1, geo.c)
            ops.gemm(x2, eye, None, out=o)
            assert ops.gn_of(o) is None, "stale GroupNorm sums survived the overwrite"
            again = ops.groupnorm(o, gamma, beta, eps=case.eps, silu=0, **kw)
            ref = N.gn_forward(geo, x2.double().view(geo.frames, geo.hw, geo.c), case.gamma, case.beta, case.eps, el)["out"]
            assert bits_equal(again, to_el(ref, el)), "groupnorm() after the overwrite does not answer for the new contents"


def test_groupnorm_lds_limit_is_refused_before_any_launch(ops_el):
    """gn_apply needs 144 B of LDS per channel with one channel per group: C = groups = 2048 asks for 294,912 B, above the 160 KB
    of a gfx950 workgroup.  vx_groupnorm and vx_groupnorm_apply return VX_ERR_INVALID from a host-side check: neither the
    statistics workspace nor the output is touched."""
    L, ops, el = ops_el
    c, hw = 2048, 4
    x = torch.zeros(1, hw, c, dtype=el, device=DEV)
    gamma = torch.ones(c, device=DEV)
    out = torch.full((1, hw, c), FILL, dtype=el, device=DEV)
    ws = torch.full((2 * c,), FILL, device=DEV)
    lib = ops._lib
    rc = lib.vx_groupnorm(ops._ptr(x), c, None, 0, 1, hw, c, 1e-5, ops._ptr(gamma), ops._ptr(gamma), 0, ops._ptr(out), ops._ptr(ws),
                          1, hw, 0, ops._stream())
    assert rc == -1 and "apply LDS" in lib.vx_last_error_string().decode()
    rc = lib.vx_groupnorm_apply(ops._ptr(x), c, None, 0, 1, hw, c, 1e-5, ops._ptr(gamma), ops._ptr(gamma), 0, ops._ptr(out),
                                ops._ptr(ws), 1, 1, hw, 0, ops._stream())
    assert rc == -1 and "apply LDS" in lib.vx_last_error_string().decode()
    with pytest.raises(L.VxError):
        ops.groupnorm(x, gamma, gamma, frames=1, hw=hw, groups=c, eps=1e-5, silu=0, out=out)
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((ws == FILL).all())


# ----------------------------------------------------------------------------------------------------- LayerNorm family
def run_ln(L, ops, case):
    l, el = case.geo, case.el
    xv, xw = column_slice(to_el(case.x(), el))
    got, wides = {}, [(xw, l.c)]
    if case.name == "counted":
        st = ops.row_stats(xv, eps=case.eps)
        got["mean"], got["rstd"] = st[:, 0], st[:, 1]
        if "parts" in case.outputs:
            got["parts"] = ops.row_stats(xv, out=torch.full((l.rows, 4), float("nan"), device=DEV))
            parts = case.values()["parts"].float().contiguous()             # the exact two-part sums, not the kernel's
            fin = torch.full((l.rows, 2), float("nan"), device=DEV)
            L.check(ops._lib.vx_row_stats_finalize(ops._ptr(parts), l.rows, l.c, float(case.eps), ops._ptr(fin), ops._stream()),
                    "vx_row_stats_finalize")
            got["fin_mean"], got["fin_rstd"] = fin[:, 0], fin[:, 1]
    else:
        ov, ow = column_slice((l.rows, l.c), el)
        ops.layernorm(xv, case.gamma.float(), case.beta.float(), case.eps, add=None if case.add is None else case.add.float().contiguous(),
                      add_rows_per_entry=case.rpe, add_entries=case.entries, out=ov)
        got["out"] = ov
        wides.append((ow, l.c))
    torch.cuda.synchronize()
    note = None if all(fill_intact(w, c) for w, c in wides) else "the launch wrote beside its columns"
    return got, note


@pytest.mark.parametrize("l", N.LN_GEOS, ids=lambda l: l.text())
def test_layernorm_and_row_statistics(ops_el, l):
    L, ops, el = ops_el
    failures = []
    for s in N.SCALES:
        for case in N.ln_cases(l, el, s, DEV):
            got, note = run_ln(L, ops, case)
            msg = case.first_wrong(got, case.wants()) or (note and f"{case.title()}: {note}")
            if msg:
                failures.append(msg)
    assert not failures, f"{len(failures)} (kernel, shape, case) triples fail:\n" + "\n".join(failures)


def test_rows_wider_than_2048_are_reported_unsupported(ops_el):
    L, ops, el = ops_el
    x = torch.zeros(4, 2056, dtype=el, device=DEV)
    g = torch.ones(2056, device=DEV)
    out = torch.full((4, 2056), FILL, dtype=el, device=DEV)
    st = torch.full((4, 2), FILL, device=DEV)
    for call in (lambda: ops.layernorm(x, g, g, out=out), lambda: ops.row_stats(x, out=st)):
        with pytest.raises(L.VxError, match=r"rc=-2.*exceeds 2048"):
            call()
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((st == FILL).all())


@pytest.mark.parametrize("l", N.FP8_GEOS, ids=lambda l: l.text())
@pytest.mark.parametrize("norm", [True, False], ids=["normalised", "plain"])
def test_quantised(ops_el, l, norm):
    """vx_layernorm_fp8: the bytes equal, scale within 2^-22 relative (max * the float32 1/448: two roundings of 2^-24, then
    rounded again), the K padding [c, ldo8) zero."""
    L, ops, el = ops_el
    c = N.fp8_case(l, el, norm, DEV)
    xv, xw = column_slice(to_el(c.x, el))
    if norm:
        r = ops.layernorm_fp8(xv, c.gamma.float(), c.beta.float(), c.eps, add=c.add.float().contiguous(), add_rows_per_entry=c.rpe,
                              add_entries=c.entries)
    else:
        r = ops.quantize_fp8(xv)
    torch.cuda.synchronize()
    kp = (l.c + 127) // 128 * 128
    assert r.q.shape == (l.rows, kp) and fill_intact(xw, l.c)
    assert bool((r.q[:, l.c:] == 0).all()), "the K padding must be zero bytes"
    bad = (r.q[:, :l.c] != c.q).nonzero()
    assert len(bad) == 0, (f"{len(bad)} bytes wrong, first at {tuple(bad[0].tolist())}: got {int(r.q[tuple(bad[0])])}, "
                           f"want {int(c.q[tuple(bad[0])])}")
    rel = ((r.scale.double() - c.scale) / c.scale).abs().max().item()
    assert rel <= 2.0 ** -22, rel
