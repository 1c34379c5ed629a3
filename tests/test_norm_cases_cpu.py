"""tests/norm_cases.py on the CPU: the exact-answer normalisation cases are right, and they catch what the aggregate bounds miss.

For every geometry tests/test_gpu_norm_exact.py launches (norm_cases.GN_GEOS, CHAIN_GEOS, LN_GEOS, FP8_GEOS; `reduced`: fewer
rows / frames where they only repeat the pattern), both element types and both scales s:
  (a) every builder's stated condition holds and is printed;
  (b) every float32 emulation (norm_cases.EMULATIONS) meets every case, with deviation 0 on every output that is demanded equal;
  (c) every mutant of the reference (norm_cases.MUTANTS) violates at least one case at every geometry where it can differ from
      the reference at all; which case catches which mutant is printed;
  (d) on Gaussian data, every defect's fraction of the aggregate bounds of test_groupnorm / test_layernorm.

Measured here (bfloat16, one Gaussian draw per shape by the recipes of tests/test_gpu_kernels.py; max|err| / allowed and
relL2 / allowed; a defect PASSES while both are <= 1).  GroupNorm under 2^-6 max|ref| + 1e-5 and relL2 <= 8e-3:
  defect                                                 4x64x320 SiLU  3x256x64     2x1024x128 SiLU  5x16x2560 SiLU  2x4096x320
  correct                                                0.18 / 0.21    0.21 / 0.21  0.19 / 0.21      0.19 / 0.21     0.18 / 0.21
  eps left out                                           0.18 / 0.21    0.21 / 0.21  0.19 / 0.21      0.19 / 0.21     0.18 / 0.21
  eps x 100                                              0.18 / 0.21    0.22 / 0.21  0.20 / 0.21      0.19 / 0.21     0.19 / 0.21
  variance divided by n - 1                              0.18 / 0.24    0.24 / 0.24  0.20 / 0.21      0.24 / 0.22     0.18 / 0.21
  truncating store                                       0.42 / 0.42    0.39 / 0.42  0.38 / 0.41      0.41 / 0.42     0.37 / 0.41
  rounding before the activation as well                 0.24 / 0.33    0.21 / 0.21  0.27 / 0.33      0.35 / 0.34     0.18 / 0.21
  last pixel of every frame missing from the sums        1.77 / 1.80    0.57 / 0.54  0.20 / 0.25      3.06 / 7.14     0.19 / 0.21
  last statistics slice counted twice                    8.49 / 22.2    2.47 / 4.29  0.77 / 1.66      21.7 / 62.2     0.69 / 1.11
  last group normalised with its neighbour's statistics  1.17 / 1.16    4.14 / 1.50  1.79 / 0.74      1.69 / 1.28     0.66 / 0.28
A wrong or missing eps, the unbiased variance, a truncating store and a double rounding pass at every shape; a dropped pixel
passes from hw = 256 on; a whole group normalised with the wrong group's statistics passes at 4096 x 320, the 64 x 64 level.
LayerNorm under 2^-7 max|ref| + 1e-5 and relL2 <= 6e-3:
  defect                                                 100x64         257x320      64x640           33x1280
  correct                                                0.25 / 0.28    0.44 / 0.28  0.39 / 0.28      0.29 / 0.28
  eps left out                                           0.25 / 0.28    0.44 / 0.28  0.39 / 0.28      0.29 / 0.28
  variance divided by c - 1                              1.19 / 1.33    0.49 / 0.38  0.39 / 0.31      0.29 / 0.29
  last 8-channel chunk missing from the statistics       20.6 / 16.4    4.49 / 2.92  2.55 / 1.65      0.78 / 0.69
Eps left out passes at all four, the unbiased variance from c = 320 on, the last 8-channel chunk missing from the statistics at
c = 1280.
test_old_bound_figures re-measures and prints both tables and asserts these sentences.
"""
import pytest
import torch

import norm_cases as N

GEOS = N.GN_GEOS + N.CHAIN_GEOS + N.LN_GEOS
IDS = [g.text() for g in GEOS]


def all_cases(geo, el, s):
    g = N.reduced(geo)
    return N.gn_cases(g, el, s) if g.kind == "gn" else N.ln_cases(g, el, s)


def emulations(geo):
    emus = N.EMULATIONS[geo.kind]
    if geo.kind == "gn" and geo.hw > 256:            # (a slice of one pixel is 4096 steps here: the slices of 16 pixels and more)
        emus = [e for e in emus if e["slice"] >= 15]
    return emus


@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_builder_conditions_and_emulations(geo, capsys):
    lines = []
    for el in N.ELEMS:
        for s in N.SCALES:
            for case in all_cases(geo, el, s):
                want = case.wants()
                msg = case.first_wrong(case.values(), want)
                assert msg is None, "the reference misses its own case: " + msg
                worst = 0.0
                for emu in emulations(case.geo):
                    got = case.values(emu=emu)
                    msg = case.first_wrong(got, want)
                    assert msg is None, f"emulation '{N.emu_name(emu)}' leaves the case, the case is refused: " + msg
                    for k, w in want.items():
                        if w.bits:
                            worst = max(worst, float((got[k] - w.lo).abs().max()))
                assert worst == 0.0
                lines.append(f"    {case.title():58s} emulations: deviation {worst:g}; " + "; ".join(case.conditions))
    with capsys.disabled():
        print(f"\n{geo.text()}: builder conditions and the largest deviation of the float32 emulations on the outputs demanded equal")
        print("\n".join(lines))


@pytest.mark.parametrize("geo", GEOS, ids=IDS)
def test_every_mutant_is_caught(geo, capsys):
    lines, missed = [], []
    for el, s in ((el, s) for el in N.ELEMS for s in N.SCALES):
        cl = all_cases(geo, el, s)
        wants = [c.wants() for c in cl]
        found = []
        for mname, applies in N.MUTANTS.items():
            if not any(applies(c) for c in cl):
                continue
            catchers = []
            for c, want in zip(cl, wants):
                if applies(c) and any(bool(b.any()) for b in c.wrong(c.values(mut=mname), want).values()):
                    catchers.append(c.name)
            found.append(f"{mname}: {', '.join(catchers) if catchers else 'NOT CAUGHT'}")
            if not catchers:
                missed.append(f"[{N.EL_NAME[el]}] {mname}")
        lines.append(f"    [{N.EL_NAME[el]}, s = {s:g}]\n" + "\n".join("        " + f for f in found))
    with capsys.disabled():
        print(f"\n{geo.text()}: which case catches which mutant (mutants that cannot differ at this geometry are left out)")
        print("\n".join(lines))
    assert not missed, f"{geo.text()}: no case catches " + "; ".join(missed)


def test_every_mutant_applies_somewhere():
    cl = [c for geo in GEOS for c in all_cases(geo, torch.bfloat16, 1.0)]
    idle = [m for m, applies in N.MUTANTS.items() if not any(applies(c) for c in cl)]
    assert not idle and len(N.MUTANTS) == 19, idle


def test_operands_are_functions_of_their_coordinates():
    """Values do not move with the split of the concat; hand-made partial sums keep their totals."""
    a, b = N.Gn(2, 64, 1280, 640), N.Gn(2, 64, 1920)
    assert torch.equal(N.gn_input(a, 1.0), N.gn_input(b, 1.0))
    assert torch.equal(N.gn_input(N.Gn(1, 64, 320), 4.0, frame0=1)[0], N.gn_input(N.Gn(2, 64, 320), 4.0)[1])
    assert torch.equal(N.add_table(4, 64, "cpu"), N.add_table(9, 64, "cpu")[:4])
    c = N.counted(N.Gn(2, 256, 320), torch.bfloat16, 1.0)
    v = c.values()
    for parts in N.PARTITIONS:
        ws = N.partitions(v["sums"], v["squares"], parts, "cpu")
        assert ws.shape == (2, parts, 32, 2) and torch.equal(ws.double().sum(1), torch.stack([v["sums"], v["squares"]], -1))


@pytest.mark.parametrize("l", N.FP8_GEOS, ids=lambda l: l.text())
def test_quantised_rows_are_exact(l, capsys):
    lines = []
    for el in N.ELEMS:
        for norm in (True, False):
            c = N.fp8_case(l, el, norm)
            back = c.q.view(torch.float8_e4m3fn).double() * c.scale[:, None]
            assert torch.equal(back, c.y) and len(set(c.scale.tolist())) > 1, "the rows must differ in their scale"
            lines.append(f"    {l.text()} [{N.EL_NAME[el]}] norm={norm}: " + "; ".join(c.conditions))
    with capsys.disabled():
        print("\n" + "\n".join(lines))


def test_old_bound_figures(capsys):
    """The reason for this file: what the Gaussian tests' bounds let through (bfloat16; the tables of the module docstring)."""
    gn = {s: N.old_gn_figures(*s) for s in N.OLD_GN_SHAPES}
    ln = {s: N.old_ln_figures(*s) for s in N.OLD_LN_SHAPES}
    with capsys.disabled():
        print("\nGaussian data under the aggregate bounds [bf16]: max|err| / allowed and relL2 / allowed")
        print("    GroupNorm (2^-6, 8e-3) at " + ", ".join("x".join(str(v) for v in s[:3]) + (" " + s[3] if s[3] != "none" else "")
                                                          for s in N.OLD_GN_SHAPES))
        for m in N.OLD_GN_MUTANTS:
            print(f"    {m:56s} " + "  ".join(f"{gn[s][m][0]:.2f} / {gn[s][m][1]:.2f}" for s in N.OLD_GN_SHAPES))
        print("    LayerNorm (2^-7, 6e-3) at " + ", ".join(f"{r}x{c}" for r, c in N.OLD_LN_SHAPES))
        for m in N.OLD_LN_MUTANTS:
            print(f"    {m:56s} " + "  ".join(f"{ln[s][m][0]:.2f} / {ln[s][m][1]:.2f}" for s in N.OLD_LN_SHAPES))

    def passes(fig, m):
        return max(fig[m]) <= 1
    for s, fig in gn.items():
        assert passes(fig, "correct"), (s, fig["correct"])
        for m in ("eps left out", "eps x 100", "variance divided by n - 1", "truncating store", "rounding before the activation as well"):
            assert passes(fig, m), f"{s}: '{m}' no longer passes the old bound {fig[m]}: this record is out of date"
        # a dropped pixel passes from hw = 256 on
        assert passes(fig, "last pixel of every frame missing from the sums") == (s[1] >= 256), (s, fig)
    assert passes(gn[(2, 4096, 320, "none")], "last group normalised with its neighbour's statistics")
    for s, fig in ln.items():
        assert passes(fig, "correct") and passes(fig, "eps left out"), (s, fig)
        assert passes(fig, "variance divided by c - 1") == (s[1] >= 320), (s, fig)
    assert passes(ln[(33, 1280)], "last 8-channel chunk missing from the statistics")


def test_failure_message_names_the_element():
    case = N.rounding(N.Gn(2, 64, 320), torch.bfloat16, 1.0)
    msg = case.first_wrong(case.values(mut="truncating store"), case.wants())
    assert msg is not None and "rounding [bf16]" in msg and "out:" in msg and "first at (" in msg, msg


def test_groupnorm_lds_limit_is_refused_on_the_host():
    """gn_apply's LDS request (144 B per channel with one channel per group) above the 160 KB of a gfx950 workgroup: VX_ERR_INVALID
    from the host-side check of vx_groupnorm / vx_groupnorm_apply, in front of every device call (this machine has no device)."""
    import ctypes
    from v_express_amd import lib as L
    f32p = ctypes.cast(0x1000, ctypes.POINTER(ctypes.c_float))
    c = 2048                                            # 294,912 B; the wav2vec2 call (C = groups = 512: 73,728 B) is inside
    assert L.lib.vx_groupnorm(0x1000, c, None, 0, 1, 4, c, 1e-5, f32p, f32p, 0, 0x1000, f32p, 1, 4, 0, None) == -1
    assert "apply LDS 294912" in L.lib.vx_last_error_string().decode()
    assert L.lib.vx_groupnorm_apply(0x1000, c, None, 0, 1, 4, c, 1e-5, f32p, f32p, 0, 0x1000, f32p, 1, 1, 4, 0, None) == -1
    assert "apply LDS 294912" in L.lib.vx_last_error_string().decode()
