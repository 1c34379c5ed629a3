"""tests/fp8_gemm_cases.py on the CPU: the exact-answer fp8 GEMM cases are right, and they catch what the aggregate bounds miss.

For every geometry of fp8_gemm_cases.ROUTES (the launches tests/test_gpu_fp8_gemm_exact.py makes; here with `reduced` row
counts, n and K unchanged), `products`, and both element types:
  (a) consistency: the encoded bytes decode back to gemm_cases' integers times the scales, the expected outputs computed from the
      BYTES are gemm_cases' own, every expected value is the float64 value rounded once, and the decode table from the format's
      formula is torch.float8_e4m3fn's;
  (b) the `rounding` shares of gemm_cases still hold (the builders assert them), and the left-out shares of `products` and `scales`
      stay under their caps (printed);
  (c) every design of fp8_gemm_cases.EMULATIONS (float32; K tiles of 128 forwards, backwards, in two halves; the three orders of
      the two scale multiplications) gives deviation 0 on the power-of-two cases and `products` and stays inside `scales`' bound;
  (d) every mutant of the reference (fp8_gemm_cases.MUTANTS) violates at least one case on at least one route shape - which case
      and which shape is printed; the dropped half K tile is missed at logical K = 320 and caught at K = 128, 256 and 640; the
      scale product rounded to the element type is caught by `scales` only;
  (e) for the record, on Gaussian data: which mutants the bound of test_gpu_kernels.py::test_gemm_fp8_store_and_split accepts;
  (f) the GPU file's own path on the host: tests/fp8_gemm_harness.py - the operands' layout, the expected outputs, the judging and
      the fill checks of tests/test_gpu_fp8_gemm_exact.py, everything but the library call - with a float32 stand-in for the
      kernel, every launch of up to 1024 rows at its FULL shape (the rest `reduced`): an index that leaves its table is an
      IndexError here before it can reach a GPU (a rowbias group that is not whole is refused where the case is built), and
      stand-ins built from MUTANTS fail through the same harness, one per judged kind.

Measured here (bfloat16, test_gemm_fp8_store_and_split's operand recipe - Gaussian a, Gaussian w K^-1/2, scale = row amax / 448,
bias, residual, alpha = 0.95, plus a two-group rowbias for the rowbias mutant - at 128 x 320; max|err| / allowed and relL2 /
allowed under max|err| <= 2^-7 max|ref| + 1e-5 and relL2 <= 6e-3; a defect PASSES while both are <= 1):
  K                                                                  320                 640                1280
  correct                                                          0.39 /   0.28      0.25 /   0.28      0.46 /   0.28   passes at every K
  subnormals flushed on A                                          0.39 /   0.28      0.25 /   0.28      0.46 /   0.28   passes at every K
  subnormals flushed on W                                          0.39 /   0.28      0.25 /   0.28      0.46 /   0.28   passes at every K
  0x80 decoded as NaN                                              0.39 /   0.28      0.25 /   0.28      0.46 /   0.28   passes at every K
  decode with exponent bias 8                                     42.51 /  61.17     55.79 /  61.52     47.17 /  61.08   caught at every K
  upper 64 bytes of the last K tile dropped                        0.39 /   0.28     21.36 /  25.98     15.08 /  18.25   passes at K = 320
  a_scale of the neighbouring row on the last row                  0.46 /   0.29      7.82 /   1.12      4.32 /   0.73   passes at K = 320
  w_scale[n - 4 .. n - 1] for the four columns before them        11.36 /   1.39      7.94 /   1.15      5.69 /   0.86   caught at every K
  bias added before the scales                                    49.88 /  82.98     45.43 /  85.11     41.58 /  83.20   caught at every K
  scale product rounded to the element type                        0.39 /   0.31      0.35 /   0.32      0.46 /   0.30   passes at every K
  truncating store                                                 0.45 /   0.55      0.50 /   0.55      0.51 /   0.55   passes at every K
  round-half-away store                                            0.39 /   0.28      0.25 /   0.28      0.46 /   0.28   passes at every K
  dequantised accumulator rounded before bias and residual         0.51 /   0.31      0.35 /   0.31      0.46 /   0.31   passes at every K
  alpha applied to the residual                                    2.93 /   4.35      3.37 /   4.32      3.32 /   4.27   caught at every K
  rowbias of the neighbouring group                               56.34 / 113.80     60.20 / 121.45     74.99 / 116.93   caught at every K
  V^T tokens t and t + 1 exchanged at a sequence's end            95.13 /  28.68    114.48 /  31.42     94.96 /  30.77   caught at every K
The old bound accepts, at every K: both subnormal flushes, the NaN decode of 0x80 (the producers never write that byte), a scale
product rounded to the element type, the truncating and the round-half-away store and the early rounding of the dequantised
accumulator.  The dropped half K tile passes at K = 320, the K of most fp8 launches of the model, and only there.  A wrong
a_scale on one row passes at K = 320 and is caught at 640 and 1280 - by the maximum alone, on the one row it touches; the size
of that row's amax decides, not K.  Caught wherever they bite: the exponent bias, the bias in front of the scales, alpha on the
residual, the neighbouring rowbias group, the exchanged V^T tokens - and the shifted w_scale vector: the Gaussian bound WOULD
catch it, but no Gaussian test has a column tail (n % 160 != 0), a rowbias, or a sequence that ends inside a tile, so these
code paths were never run at kernel level rather than run and under-checked.
test_old_bound_figures re-measures and prints the table and asserts what the sentences above say of every K.
"""
import pytest
import torch

import fp8_gemm_cases as P
import fp8_gemm_harness as H
import gemm_cases as G

ROUTE_NAMES = sorted(P.ROUTES)
OLD_KS = (320, 640, 1280)


def geometries(route):
    seen, out = set(), []
    for l in P.ROUTES[route]:
        g = P.reduced(l.geo)
        if g not in seen:
            seen.add(g)
            out.append(g)
    return out


def all_cases(g, el):
    return P.cases(g, el) + ([P.in_place(g, el)] if g.epi == "store" else [])


@pytest.fixture(autouse=True)
def _fresh_cache():
    G.clear_cache()
    yield
    G.clear_cache()


def values(want):
    return {k: v[0] for k, v in want.items()}


def test_decode_table():
    t = P.decode_table()
    ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    assert torch.equal(torch.isnan(t), torch.isnan(ref)) and int(torch.isnan(t).sum()) == 2
    fin = ~torch.isnan(t)
    assert torch.equal(t[fin], ref[fin]) and len(P.FINITE) == 254
    assert float(t[0x7E]) == 448.0 and float(t[0x01]) == 2.0 ** -9 and float(t[0x08]) == 2.0 ** -6
    assert float(t[0x80]) == 0.0 and bool(torch.signbit(t[0x80]))
    exact, top = P.product_is_exact()
    assert exact and top == 448.0 * 448.0 / 4 == 50176.0


@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_consistency_conditions_and_emulations(route, capsys):
    lines = []
    for g in geometries(route):
        for el in G.ELEMS:
            for case in all_cases(g, el):
                q, w8 = case.bytes_("cpu")
                sa, sw = case.scales("cpu")
                t = P.decode_table()
                assert q.shape == (g.m, case.kp) and w8.shape == (g.n, case.kp) and case.kp % 128 == 0
                assert bool((q[:, g.k:] == 0).all()) and bool((w8[:, g.k:] == 0).all()), "the K padding is zero bytes"
                a = G.gather(g, case.base.dens, torch.arange(g.m))
                if case.kind == "pow2":                    # the bytes are gemm_cases' integers over the scales, all normal
                    assert torch.equal(t[q[:, :g.k].long()] * sa.double()[:, None], a)
                    assert torch.equal(t[w8[:, :g.k].long()] * sw.double()[:, None], G.weight(g, "cpu"))
                    assert bool(((((q >> 3) & 15) != 0) | ((q & 0x7F) == 0)).all()) and bool((((w8[:, :g.k] >> 3) & 15) != 0).all())
                    zeros = q[:, :g.k][a == 0]
                    if zeros.numel() >= 64:
                        share = float((zeros == 0x80).double().mean())
                        assert 0.3 < share < 0.7, f"{share} of A's zeros are -0"
                    own = case.base.expected()             # gemm_cases' own expected outputs, from the integers
                else:
                    assert torch.equal(t[q[:, :g.k].long()], a) and torch.equal(t[w8[:, :g.k].long()], G.weight(g, "cpu"))
                    own = None
                want = case.expected()
                if own is not None:
                    for name, (w, tol) in own.items():
                        assert torch.equal(want[name][0], w), f"{case.name}: from the bytes != gemm_cases' own ({name})"
                if g.epi == "store":                       # the float64 value rounded once
                    x, _ = case.base.exact("cpu", acc=case.dequantised())
                    assert torch.equal(want["out"][0], G.round_el(x, el))
                msg = case.first_wrong(values(want), want)
                assert msg is None, "the reference misses its own case: " + msg
                worst = 0.0
                for emu in P.EMULATIONS:
                    got = case.expected(emu=emu)
                    dev = max(float((got[n][0] - w).abs().max()) for n, (w, _) in want.items())
                    worst = max(worst, dev)
                    msg = case.first_wrong(values(got), want)
                    assert msg is None, f"emulation '{emu}' leaves the case, the case list is refused: " + msg
                    if case.kind == "pow2":
                        assert dev == 0.0, (emu, dev)
                lines.append(f"    {g.text():50s} [{G.EL_NAME[el]}] {case.name:22s} emulations: deviation {worst:g}; "
                             + "; ".join(case.base.conditions + case.conditions))
    with capsys.disabled():
        print(f"\nroute {route}: builder conditions and the largest deviation of the emulated designs")
        print("\n".join(lines))


def test_products(capsys):
    lines = []
    for el in G.ELEMS:
        case = P.products(el)
        q, w8 = case.bytes_("cpu")
        assert sorted(set(int(b) for b in q.amax(dim=1))) == P.FINITE and int((q != 0).sum()) == 253
        assert sorted(set(int(b) for b in w8[:, 0])) == P.FINITE and bool((w8 == w8[:, :1]).all())
        want = case.expected()
        t = P.decode_table()
        hot = t[q.long()].sum(dim=1)               # (one nonzero byte per row; byte 0x00 / 0x80 rows: 0)
        x = hot[:, None] * t[w8[:, 0].long()][None, :] * 0.25
        assert torch.equal(want["out"][0], G.round_el(x, el)) and float(x.abs().max()) == 50176.0
        left = float(case.left_out().double().mean())
        assert (left == 0.0) if el is torch.bfloat16 else (0.0 < left <= P.PRODUCTS_CAP)
        worst = 0.0
        for emu in P.EMULATIONS:
            got = case.expected(emu=emu)
            worst = max(worst, float((got["out"][0] - want["out"][0]).abs().max()))
            assert case.first_wrong(values(got), want) is None, emu
        assert worst == 0.0
        lines.append(f"    products [{G.EL_NAME[el]}] emulations: deviation {worst:g}; " + "; ".join(case.conditions))
    with capsys.disabled():
        print("\nproducts: conditions and the largest deviation of the emulated designs")
        print("\n".join(lines))


def catches(case, mut):
    """Whether the case tells the mutant from the reference."""
    want = case.expected()
    try:
        got = case.expected(mut=mut)
    except AssertionError:                  # (the mutant moves a SiLU argument out of the saturated range, or makes it NaN)
        return True
    return any(bool(b.any()) for b in case.wrong(values(got), want).values())


def test_every_mutant_is_caught(capsys):
    caught = {m: [] for m in P.MUTANTS}
    for route in ROUTE_NAMES:
        for g in geometries(route):
            for el in G.ELEMS:
                for case in all_cases(g, el):
                    for mut, applies in P.MUTANTS.items():
                        if applies(case) and catches(case, mut):
                            caught[mut].append(f"{case.name} [{G.EL_NAME[el]}] at {route}: {g.text()}")
            G.clear_cache()
    for el in G.ELEMS:
        case = P.products(el)
        for mut, applies in P.MUTANTS.items():
            if applies(case) and catches(case, mut):
                caught[mut].append(f"products [{G.EL_NAME[el]}] at 128x160 store: {case.geo.text()}")
    with capsys.disabled():
        print("\nwhich case catches which mutant (the first (case, shape) and how many (case, shape, element type) in all)")
        for mut, hits in caught.items():
            names = sorted({h.split(" [")[0] for h in hits})
            print(f"    {mut:60s} {len(hits):4d}: {hits[0] if hits else 'NOT CAUGHT'}   (cases: {', '.join(names)})")
    assert len(P.MUTANTS) == 15
    missed = [m for m, hits in caught.items() if not hits]
    assert not missed, "no case catches " + "; ".join(missed)
    only = {h.split(" [")[0] for h in caught["scale product rounded to the element type"]}
    assert only == {"scales"}, only
    for m in ("subnormals flushed on A", "subnormals flushed on W"):
        assert {h.split(" [")[0] for h in caught[m]} == {"products"}


def test_scale_product_in_the_element_type_is_invisible_to_the_other_cases():
    """Power-of-two scales: their product is a value of the element type, so only `scales` can see this defect."""
    for g in (P.reduced(P.ROUTES["128x160 store"][3].geo), P.PRODUCTS_GEO):
        for el in G.ELEMS:
            cl = [P.products(el)] if g is P.PRODUCTS_GEO else [c for c in all_cases(g, el) if c.kind == "pow2"]
            for case in cl:
                sa, sw = (t.double() for t in case.scales("cpu"))
                s = sa[:, None] * sw[None, :]
                assert torch.equal(G.round_el(s, el), s)


@pytest.mark.parametrize("k,seen", [(128, True), (256, True), (320, False), (640, True)])
def test_dropped_half_k_tile(k, seen):
    """Logical K = 320 is padded to 384 with zero bytes: a kernel that drops bytes 64 .. 127 of the last K tile gets every such
    launch right; K = 128, 256 and 640 end on a full tile."""
    mut = "upper 64 bytes of the last K tile dropped"
    for el in G.ELEMS:
        g = G.linear(40, 320, k)
        hits = []
        for case in all_cases(g, el):
            want, got = case.expected(), case.expected(mut=mut)
            hits.append(any(bool(b.any()) for b in case.wrong(values(got), want).values()))
            assert P.MUTANTS[mut](case) == seen
        assert any(hits) == seen and (all(hits) or not seen), (k, hits)


def test_old_bound_figures(capsys):
    """The reason for this file: what the Gaussian fp8 tests' bound lets through (bfloat16; the table of the module docstring)."""
    rows = {}
    passes = {}
    for k in OLD_KS:
        fig = P.old_bound_figures(k)
        assert max(fig["correct"]) <= 1, f"K={k}: the rounded reference itself misses the old bound {fig['correct']}"
        for name, (mx, l2) in fig.items():
            rows.setdefault(name, []).append(f"{mx:8.2f} / {l2:6.2f}" if mx != float("inf") else "     NaN /    NaN")
            passes.setdefault(name, []).append(max(mx, l2) <= 1)
    with capsys.disabled():
        print("\nGaussian data under the aggregate bound [bf16, 128 x 320], max|err| / allowed and relL2 / allowed, K = "
              + ", ".join(str(k) for k in OLD_KS))
        for name, r in rows.items():
            verdict = "passes at every K" if all(passes[name]) else "caught at every K" if not any(passes[name]) else \
                "passes at K = " + ", ".join(str(k) for k, p in zip(OLD_KS, passes[name]) if p)
            print(f"    {name:60s} " + "  ".join(r) + f"   {verdict}")
    # what the module docstring says of the figures
    for name in ("subnormals flushed on A", "subnormals flushed on W", "0x80 decoded as NaN", "truncating store",
                 "round-half-away store", "scale product rounded to the element type",
                 "dequantised accumulator rounded before bias and residual"):
        assert all(passes[name]), f"'{name}' no longer passes the old bound: this record is out of date"
    for name in ("decode with exponent bias 8", "bias added before the scales", "alpha applied to the residual",
                 "rowbias of the neighbouring group", "V^T tokens t and t + 1 exchanged at a sequence's end",
                 "w_scale[n - 4 .. n - 1] for the four columns before them"):
        assert not any(passes[name]), f"'{name}' passes the old bound somewhere: this record is out of date"
    assert passes["upper 64 bytes of the last K tile dropped"] == [True, False, False]


# ----------------------------------------------------------------------------------------------------- the GPU file's path, on the host
def host_shape(g):
    """Full shape up to 1024 rows - the launches whose m `reduced` changes, the odd tails among them - and `reduced` beyond."""
    return g if g.m <= 1024 else P.reduced(g)


def test_partial_rowbias_group_is_refused_where_the_case_is_built():
    """m = 130 in groups of 16: row 128 would read row 8 of a rowbias table of 8 rows."""
    g = G.linear(130, 160, 128, rows_per_group=16)
    with pytest.raises(AssertionError, match=r"m=130 is no multiple of rows_per_group=16"):
        G.signs(g, torch.bfloat16, "cpu", residual=True)
    with pytest.raises(AssertionError, match=r"m=130 is no multiple of rows_per_group=16"):
        P.Fp8Case("pow2", G.Case("signs", g, torch.bfloat16, 1.0))
    for routes in (G.ROUTES, P.ROUTES):                    # no launch of either file's routes has one, at its full shape
        for name, launches in routes.items():
            for l in launches:
                assert not l.geo.rows_per_group or l.geo.m % l.geo.rows_per_group == 0, (name, l.geo.text())


@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_harness_with_a_host_stand_in(route):
    """tests/fp8_gemm_harness.py - all that tests/test_gpu_fp8_gemm_exact.py does but the library call - with a stand-in for
    the kernel: an index that leaves its table fails here.  Every launch of the route at `host_shape`, both element types; the
    stand-in is the 'K tiles forwards' design of EMULATIONS (float32), and a second time float32 arithmetic on the tensors of
    the call themselves, which shows that the laid-out operands are the problem the expected outputs belong to."""
    for el in G.ELEMS:
        for stand_in in (H.reference_stand_in("cpu", emu="K tiles forwards"), H.operand_stand_in):
            failures, made = H.run_route(route, el, stand_in, "cpu", shape=host_shape)
            assert made >= 2 * len(P.ROUTES[route])
            assert not failures, f"{len(failures)} (route, shape, case) triples fail:\n" + "\n".join(failures)


def test_harness_products_and_chained_with_a_host_stand_in():
    for el in G.ELEMS:
        for geo in (P.PRODUCTS_GEO, P.PRODUCTS_RING_GEO):
            for stand_in in (H.reference_stand_in("cpu", emu="K tiles backwards"), H.operand_stand_in):
                assert H.run_case(P.products(el, geo=geo), "products", stand_in, "cpu") is None
        for m, n, k in P.CHAINED:
            def produce(x, w):                             # amax / 448 scales and exact quotients, as the producers make them
                sa, sw = x.double().abs().amax(dim=1) / 448.0, w.double().abs().amax(dim=1) / 448.0
                qa, qw = x.double() / sa[:, None], w.double() / sw[:, None]
                assert torch.equal(qa.float().to(torch.float8_e4m3fn).double(), qa)
                return ((qa @ qw.t()) * sa[:, None] * sw[None, :]).float().to(el), sa.float(), sw.float()
            assert H.judge_chained(m, n, k, el, "cpu", produce) is None


def test_harness_fails_on_a_wrong_stand_in():
    """That the GPU file checks anything: stand-ins built from MUTANTS fail through the same harness, one per judged kind,
    with a message naming route, shape, case and the first wrong element."""
    el = torch.bfloat16
    # pow2 (==): every case of the route's launches that the mutant can touch fails
    failures, made = H.run_route("128x160 store", el, H.reference_stand_in("cpu", mut="truncating store"), "cpu", shape=P.reduced)
    assert len(failures) >= len(P.ROUTES["128x160 store"]) and made > len(failures)
    msg = [f for f in failures if "rounding + residual" in f and "K=1280" in f][0]
    for part in ("128x160 store (gemm_kernel<128x160x128,4w,STORE,fast,fp8>)", "rounding + residual [bf16]", "-> 1280 [m=40 K=1280 store]",
                 "out:", "first at (", "got ", "expected "):
        assert part in msg, (part, msg)
    # scales (the band): the one case that sees a scale product formed in the element type
    failures, _ = H.run_route("128x160 store", el, H.reference_stand_in("cpu", mut="scale product rounded to the element type"),
                              "cpu", shape=P.reduced)
    assert failures and all(": scales [bf16]" in f for f in failures), failures
    # products (==, float16 with its left-out pairs): a flushed subnormal and a dropped half K tile
    for e in G.ELEMS:
        for mut in ("subnormals flushed on W", "upper 64 bytes of the last K tile dropped"):
            msg = H.run_case(P.products(e), "products", H.reference_stand_in("cpu", mut=mut), "cpu")
            assert msg is not None and msg.startswith(f"products [{G.EL_NAME[e]}]") and "first at (" in msg, (mut, msg)
    # ... and a stand-in that writes beside its output, into the residual, or reads a wrong rowbias group
    case = P.in_place(G.linear(48, 160, 128), el)

    def beside(call):
        H.operand_stand_in(call)
        call.guards[-1][1][5, 3] = 0.0
    assert "the fill beside residual was written" in H.run_case(case, "k", beside, "cpu", in_place=True)

    def shifted_group(call):
        call.rows_per_group += 1
        H.operand_stand_in(call)
    assert "in place: signs + residual [bf16]" in H.run_case(case, "k", shifted_group, "cpu", in_place=True)
    store = P.cases(G.linear(48, 160, 128), el)[1]

    def into_residual(call):
        H.operand_stand_in(call)
        call.residual[7, 7] += 2
    assert "the operand residual was written" in H.run_case(store, "k", into_residual, "cpu")


def test_failure_message_names_the_element():
    g = G.linear(40, 160, 128)
    case = [c for c in P.cases(g, torch.bfloat16) if c.name == "rounding + residual"][0]
    want = case.expected()
    got = case.expected(mut="truncating store")
    msg = case.first_wrong(values(got), want)
    assert msg is not None and "rounding + residual [bf16]" in msg and "out:" in msg and "first at (" in msg and "Kp=128" in msg, msg
