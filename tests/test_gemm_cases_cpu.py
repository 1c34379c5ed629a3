"""tests/gemm_cases.py on the CPU: the exact-answer GEMM cases are right, and they catch what the aggregate bounds miss.

For every geometry tests/test_gpu_gemm_exact.py launches (gemm_cases.ROUTES, with `reduced` row counts: n, K and the
convolution as on the GPU) and both element types:
  (a) every builder's stated condition holds and is printed: the share of large values (`signs`), the tie shares (`rounding`),
      the saturated range (`saturated`), exactness (`folded`), the sum bounds (`statistics`);
  (b) float32 accumulation in every legitimate order (gemm_cases.EMULATIONS: 64-wide chunks forwards and backwards, taps
      innermost and outermost, 2 to 8 K slices summed afterwards) meets every case with deviation 0;
  (c) every mutant of the reference (gemm_cases.MUTANTS) violates at least one case at every geometry where it can differ from
      the reference at all (a structural fact per mutant: a 3x3 kernel, two frames and padding, a second source, ...);
      which case catches which mutant is printed per route;
  (d) for the record, on Gaussian data: every mutant's fraction of the bounds of the aggregate tests per K.

Measured here (bfloat16, one Gaussian draw per K, m x n = 512 x 320, residual added; max|err| / allowed and relL2 / allowed
under max|err| <= 2^-7 max|ref| + 1e-5 and relL2 <= 6e-3; a defect PASSES while both are <= 1):
  K                                               64            320          1280         2560         2880         5120         11520
  correct                                         0.27 / 0.28   0.27 / 0.28  0.22 / 0.28  0.28 / 0.28  0.27 / 0.28  0.24 / 0.28  0.25 / 0.28
  truncating store                                0.54 / 0.55   0.55 / 0.55  0.44 / 0.55  0.71 / 0.55  0.53 / 0.55  0.70 / 0.55  0.50 / 0.55
  round-half-away store                           0.27 / 0.28   0.27 / 0.28  0.22 / 0.28  0.28 / 0.28  0.27 / 0.28  0.24 / 0.28  0.25 / 0.28
  double rounding before the residual             0.53 / 0.37   0.54 / 0.37  0.44 / 0.37  0.49 / 0.37  0.53 / 0.37  0.47 / 0.37  0.49 / 0.37
  last K-term dropped in a 16-row band            13.50 / 2.21  7.08 / 1.11  1.89 / 0.55  2.00 / 0.39  2.05 / 0.43  1.86 / 0.39  1.15 / 0.32
  one K-term dropped for one pixel of one frame   0.94 / 0.28   0.65 / 0.28  0.34 / 0.28  1.33 / 0.30  0.83 / 0.28  0.77 / 0.29  0.55 / 0.28
  one K-term at the split boundary counted twice  9.96 / 1.96   8.64 / 1.17  3.37 / 0.70  1.97 / 0.41  1.58 / 0.36  0.88 / 0.33  0.86 / 0.31
The three store defects pass at every K.  A wrong term confined to ONE output row (mutant 5: one term of one row, as the draw
gives it) passes from the smallest K of the GPU shapes, 64, on - at six of the seven K; it is the size of that one term that
decides, not K.  A wrong term in 16 rows x 320 columns is caught up to K = 2880 - by the maximum, the L2 share is inside from
K = 1280 - and the double-counted term passes from K = 5120, where the cooperative split and split-K live.
test_old_bound_figures re-measures and prints the table and asserts what the sentences above say.
"""
import pytest
import torch

import gemm_cases as G

ROUTE_NAMES = sorted(G.ROUTES)
OLD_KS = (64, 320, 1280, 2560, 2880, 5120, 11520)        # the K of the GPU shapes (23040: the two-source cooperative convolution)


def launches(route):
    """The route's launches with reduced row counts, duplicates (shapes that differ in their rows only) dropped."""
    seen, out = set(), []
    for l in G.ROUTES[route]:
        g = G.reduced(l.geo)
        if (g, l.skip) not in seen:
            seen.add((g, l.skip))
            out.append((g, l.skip))
    return out


@pytest.fixture(autouse=True)
def _fresh_cache():
    G.clear_cache()
    yield
    G.clear_cache()


@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_builder_conditions_and_emulations(route, capsys):
    lines = []
    for g, skip in launches(route):
        for el in G.ELEMS:
            for case in G.cases(g, el, skip=skip):
                want = case.expected()
                msg = case.first_wrong({k: v[0] for k, v in want.items()}, want)
                assert msg is None, "the reference misses its own case: " + msg
                worst = 0.0
                # the long-K convolutions: one order of each kind (a gather of 512 x 23040 per order otherwise)
                orders = G.EMULATIONS if g.m * g.k <= 1 << 21 else G.EMULATIONS[1:3] + G.EMULATIONS[-1:]
                for order in orders:
                    got = case.expected(acc=G.emulate(case, order))
                    for name, (w, _) in want.items():
                        worst = max(worst, float((got[name][0] - w).abs().max()))
                    msg = case.first_wrong({k: v[0] for k, v in got.items()}, want)
                    assert msg is None, f"emulation '{order}' leaves the case, the case list is refused: " + msg
                lines.append(f"    {g.text():60s} [{G.EL_NAME[el]}] {case.name:28s} emulations: deviation {worst:g}; "
                             + "; ".join(case.conditions))
    with capsys.disabled():
        print(f"\nroute {route}: builder conditions and the largest deviation of the emulated accumulation orders")
        print("\n".join(lines))


@pytest.mark.parametrize("route", ROUTE_NAMES)
def test_every_mutant_is_caught(route, capsys):
    lines, missed = [], []
    for g, skip in launches(route):
        for el in G.ELEMS:
            cl = G.cases(g, el, skip=skip)
            wants = [c.expected() for c in cl]
            found = []
            for mname, applies in G.MUTANTS.items():
                if not applies(g):
                    continue
                catchers = []
                for c, want in zip(cl, wants):
                    got = c.expected(mut=mname)
                    if any(bool(b.any()) for b in c.wrong({k: v[0] for k, v in got.items()}, want).values()):
                        catchers.append(c.name)
                found.append(f"{mname}: {', '.join(catchers) if catchers else 'NOT CAUGHT'}")
                if not catchers:
                    missed.append(f"{g.text()} [{G.EL_NAME[el]}]: {mname}")
            lines.append(f"    {g.text()} [{G.EL_NAME[el]}]\n" + "\n".join("        " + f for f in found))
    with capsys.disabled():
        print(f"\nroute {route}: which case catches which mutant (mutants that cannot differ at a geometry are left out)")
        print("\n".join(lines))
    assert not missed, f"route {route}: no case catches " + "; ".join(missed)


def test_every_mutant_applies_somewhere():
    geos = [G.reduced(l.geo) for ls in G.ROUTES.values() for l in ls]
    idle = [m for m, applies in G.MUTANTS.items() if not any(applies(g) for g in geos)]
    assert not idle and len(G.MUTANTS) == 19, idle


def test_operands_are_functions_of_their_coordinates():
    """A value does not move when the shape changes: the first rows / frames of a larger problem are the smaller problem."""
    small, big = G.linear(40, 160, 64), G.linear(300, 320, 64)
    assert torch.equal(G.image(small, 1.0, "cpu"), G.image(big, 1.0, "cpu")[:, :40])
    assert torch.equal(G.weight(small, "cpu"), G.weight(big, "cpu")[:160])
    a, b = G.conv(2, 8, 6, 64, 160, pad=1), G.conv(3, 8, 6, 64, 160, bordered=True)
    assert torch.equal(G.accumulate(a, 1.0, "cpu"), G.accumulate(b, 1.0, "cpu")[:a.m])      # pad-1 == the pre-bordered pad-0 form
    two = G.conv(2, 8, 6, 128, 160, c2=64, pad=1)
    one = G.conv(2, 8, 6, 192, 160, pad=1)
    assert torch.equal(G.accumulate(two, 1.0, "cpu"), G.accumulate(one, 1.0, "cpu"))        # two sources == their concatenation
    # the im2col of the reference against torch's own convolution
    import torch.nn.functional as F
    for g in (G.conv(2, 9, 7, 64, 64, pad=1, stride=2), G.conv(2, 8, 6, 64, 160, pad=1, ups=1), G.conv(2, 7, 9, 64, 160, pad=1),
              G.conv(2, 8, 6, 64, 64, stride=2, pad_end=1)):
        x = G.image(g, 1.0, "cpu").permute(0, 3, 1, 2)
        if g.ups:
            x = F.interpolate(x, scale_factor=2.0, mode="nearest")
        if g.pad_end:
            x = F.pad(x, (0, 1, 0, 1))
        w = G.weight(g, "cpu").reshape(g.n, 3, 3, g.cin).permute(0, 3, 1, 2)
        y = F.conv2d(x, w, stride=g.stride, padding=g.pad).permute(0, 2, 3, 1).reshape(g.m, g.n)
        assert torch.equal(y, G.accumulate(g, 1.0, "cpu")), g.text()
    win = G.conv(2, 10, 8, 64, 160, window=(1, 2, 6, 4))
    full = G.accumulate(G.conv(2, 10, 8, 64, 160), 1.0, "cpu").reshape(2, 8, 6, 160)
    assert torch.equal(G.accumulate(win, 1.0, "cpu").reshape(2, 6, 4, 160), full[:, 1:7, 2:6])


def test_old_bound_figures(capsys):
    """The reason for this file: what the Gaussian tests' bound lets through (bfloat16; the table of the module docstring)."""
    rows = {name: [] for name in G.OLD_MUTANTS}
    first_pass = None
    for k in OLD_KS:
        fig = G.old_bound_figures(k)
        for name, (mx, l2) in fig.items():
            rows[name].append(f"{mx:.2f} / {l2:.2f}")
        assert max(fig["correct"]) <= 1, f"K={k}: the rounded reference itself misses the old bound {fig['correct']}"
        for name in ("truncating store", "round-half-away store", "double rounding before the residual"):
            assert max(fig[name]) <= 1, f"K={k}: '{name}' no longer passes the old bound {fig[name]}: this record is out of date"
        if first_pass is None and max(fig["one K-term dropped for one pixel of one frame"]) <= 1:
            first_pass = k
        if k >= 5120:
            assert max(fig["one K-term at the split boundary counted twice"]) <= 1, (k, fig)
    with capsys.disabled():
        print("\nGaussian data under the aggregate bound [bf16, 512 x 320], max|err| / allowed and relL2 / allowed, K = "
              + ", ".join(str(k) for k in OLD_KS))
        for name, r in rows.items():
            print(f"    {name:50s} " + "  ".join(r))
        print(f"    'one K-term dropped for one pixel of one frame' first passes at K = {first_pass}")
    assert first_pass is not None, "the one-pixel defect is caught by the old bound at every K: this record is out of date"


def test_failure_message_names_the_element():
    g = G.linear(40, 160, 64)
    case = G.rounding(g, torch.bfloat16, residual=True)
    want = case.expected()
    got = case.expected(mut="truncating store")
    msg = case.first_wrong({k: v[0] for k, v in got.items()}, want)
    assert msg is not None and "rounding + residual [bf16]" in msg and "out:" in msg and "first at (" in msg, msg
