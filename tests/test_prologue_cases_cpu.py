"""tests/prologue_cases.py on the CPU: the exact-answer cases of the prologue's kernel routes are right, and what they catch.

For every case tests/test_gpu_prologue_exact.py runs (and the small-channel convolutions / the d = 64 short-key attention that
gemm_cases.ROUTES["small conv"] and attention_cases.small_kv_geoms(64) add to the older exact suites), both element types:
  (a) the reference equals an independently written float64 F.conv1d / F.conv2d / grouped F.conv1d(padding=kp // 2)[..., :-1]
      formulation, and meets its own case;
  (b) float32 accumulation in three orders (tap by tap forwards / backwards or in halves, 64-wide K chunks forwards / backwards)
      deviates by 0; gelu_f's polynomial and the erf form, both in float32, stay inside `middle`;
  (c) every mutant (prologue_cases.MUTANTS) violates every case where it structurally can differ from the reference; the two
      convolution mutants live in gemm_cases.MUTANTS and the V-offset mutant in attention_cases.MUTANTS, whose CPU files hold
      them to the same rule;
  (d) the route keys the case lists state are the ones vx_gemm_config_name gives the launches (host code, no GPU);
  (e) for the record, what the per-kernel Gaussian tests of tests/test_gpu_prologue.py let through.

(e) measured here, bfloat16, relL2 / allowed and max|err| / allowed (a defect PASSES while both are <= 1):
  vx_wave_conv1d, 4000 samples x 32 channels, rel 4e-3, max 2^-8       correct 0.41 / 0.51; every mutant >= 65 / 82
  windows + GELU, T = 799, C = n = 32, k = 3, s = 2, rel 6e-3, max 2^-7  correct 0.28 / 0.33
      tanh-form GELU 0.28 / 0.33 PASSES; sigmoid-form GELU 1.61 / 0.59; GELU before the bias 13.6 / 7.8; every addressing
      mutant (stride, late window, dropped or reversed taps) >= 99 / 67
  positional conv, T = 18, H = 768, 16 groups, kp = 128, same bound     correct 0.28 / 0.38
      tanh-form GELU 0.28 / 0.38 PASSES; sigmoid-form GELU 0.57 / 0.38 PASSES; last tap dropped 0.28 / 0.38 PASSES (at 18
      tokens the last tap reads only padding: it IS the reference there, and only the 249-token Gaussian case can see it);
      group g with group g+1's bias slice 13.3 / 13.2; GELU before the bias 9.2 / 9.9; every other mutant >= 46 / 38
So the per-kernel Gaussian tests do catch a mis-addressed window, tap, group or stride; what they cannot see is the FORM of
the activation (tanh everywhere, the sigmoid form behind the positional conv), and - like every aggregate bound - a store
that truncates or rounds twice (tests/test_gemm_cases_cpu.py).  The end-to-end bounds (3e-2 behind 12 LayerNormed layers) are
five times wider still.  test_old_bound_figures re-measures the table and asserts exactly the PASSES above.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import attention_cases as A
import gemm_cases as G
import prologue_cases as P

F64 = torch.float64
EL_IDS = dict(params=P.ELEMS, ids=lambda e: P.EL_NAME[e])


@pytest.fixture(**EL_IDS)
def el(request):
    return request.param


def all_cases(el):
    return P.wave_cases(el) + P.window_cases(el) + P.gelu_cases(el) + P.positional_cases(el)


# ----------------------------------------------------------------------------------------------------- (a)
def restated(c):
    """The case's exact output from torch's own convolutions (float64)."""
    if isinstance(c, P.Wave):
        return F.conv1d(c.wave("cpu")[None, None], c.weight("cpu").t()[:, None, :], stride=c.stride)[0].t()
    if isinstance(c, P.Win):
        y = F.conv1d(c.x("cpu").t()[None], c.weight("cpu").permute(0, 2, 1), c.bias("cpu"), stride=c.s)[0].t()
        y = c.alpha * (F.gelu(y) if c.act == "gelu" else y)
        return y if not c.residual else y + c.residual_t("cpu")
    x = c.x("cpu")
    y = F.conv1d(x.t()[None], c.weight("cpu").permute(0, 2, 1), c.bias("cpu"), padding=c.kp // 2, groups=c.G)[0, :, :-1].t()
    return x + F.gelu(y)


def test_references_equal_torch_convolutions(el, capsys):
    lines = []
    for c in all_cases(el):
        want, ex = restated(c), c.exact()
        assert want.shape == ex.shape, c.text()
        # integers are equal; behind a GELU the two float64 spellings (erfc here, erf in torch) may differ in the last bits
        tol = 0.0 if getattr(c, "act", "none") != "gelu" else 1e-13
        assert float((want - ex).abs().max()) <= tol * max(1.0, float(ex.abs().max())), c.text()
        assert c.first_wrong(c.stored()) is None, "the reference misses its own case"
        lines.append(f"    {c.text():100s} {'; '.join(c.conditions)}")
    # the small-channel convolutions: gemm_cases' gather against F.conv2d
    for lch in G.ROUTES["small conv"]:
        g = lch.geo
        x = G.image(g, 1.0, "cpu").permute(0, 3, 1, 2)
        w = G.weight(g, "cpu").reshape(g.n, 3, 3, g.cin).permute(0, 3, 1, 2)
        y = F.conv2d(x, w, stride=g.stride, padding=g.pad).permute(0, 2, 3, 1).reshape(g.m, g.n)
        assert torch.equal(y, G.accumulate(g, 1.0, "cpu")), g.text()
    G.clear_cache()
    with capsys.disabled():
        print(f"\nprologue cases [{P.EL_NAME[el]}]: builder conditions")
        print("\n".join(lines))


# ----------------------------------------------------------------------------------------------------- (b)
def test_float32_emulations_deviate_by_zero(el):
    for c in all_cases(el):
        want = c.want()
        if isinstance(c, P.Wave):
            outs = {o: P.emulate_wave(c, o) for o in P.WAVE_ORDERS}
        elif isinstance(c, P.Pos):
            outs = {o: P.emulate_pos(c, o) for o in P.POS_ORDERS}
        else:
            outs = {o: c.stored(acc=P.emulate_win(c, o)) for o in P.WIN_ORDERS}
        for order, out in outs.items():
            assert not bool(want.wrong(out).any()), f"emulation '{order}' leaves the case: {c.text()}"
            if getattr(c, "kind", "") != "middle":
                assert float((out - c.stored()).abs().max()) == 0.0, (order, c.text())


def test_float32_gelu_designs_stay_inside_middle(el, capsys):
    worst = {}
    for c in P.window_cases(el) + P.gelu_cases(el):
        if c.kind != "middle":
            continue
        ex, arg = c.exact(with_arg=True)
        for name, fn in P.GELU_DESIGNS.items():
            y = fn(arg)
            out = y if c.out_f32 else P.round_el(y, c.el)
            assert not bool(c.want().wrong(out).any()), f"'{name}' leaves the case: {c.text()}"
            worst[name] = max(worst.get(name, 0.0), float((y - ex).abs().max()))
    with capsys.disabled():
        tanh, sig = P.tanh_form_distance()
        print(f"\n[{P.EL_NAME[el]}] largest |float32 design - float64| over the integer arguments in [-8, 8] (bound {P.GELU_ABS:g}): "
              + "; ".join(f"{k}: {v:.3g}" for k, v in worst.items()))
        print(f"    smallest distance of the tanh form on 1 <= |x| <= 4: {tanh:.3g}; of the sigmoid form: {sig:.3g}")
    assert max(worst.values()) <= P.GELU_ABS and tanh > 16 * 2 * P.GELU_ABS


# ----------------------------------------------------------------------------------------------------- (c)
def test_every_mutant_is_caught(el, capsys):
    cases = all_cases(el)
    lines, missed = [], []
    for mname, applies in P.MUTANTS.items():
        hit = [c for c in cases if applies(c)]
        assert hit, f"'{mname}' applies to no case"
        miss = [c.text() for c in hit if not P.caught(c, mname)]
        missed += [f"{mname}: {t}" for t in miss]
        kinds = sorted({type(c).__name__ + " " + c.kind for c in hit})
        lines.append(f"    {mname:45s} caught at {len(hit) - len(miss)} of the {len(hit)} cases it can touch ({', '.join(kinds)})")
    with capsys.disabled():
        print(f"\nprologue cases [{P.EL_NAME[el]}]: mutants")
        print("\n".join(lines))
    assert not missed, "no catch: " + "; ".join(missed)
    assert len(P.MUTANTS) == 17


def test_convolution_and_v_offset_mutants_are_caught(el):
    """The three mutants that live with the older suites, at the shapes this work adds."""
    for lch in G.ROUTES["small conv"]:
        g = G.reduced(lch.geo)
        cl = G.cases(g, el)
        wants = [c.expected() for c in cl]
        for mname in ("straddling K tile reads its second tap one pixel to the right", "no zero fill right of the last column"):
            if not G.MUTANTS[mname](g):
                assert mname.startswith("straddling") and g.cin % 64 == 0, (mname, g.text())
                continue
            assert any(any(bool(b.any()) for b in c.wrong({k: v[0] for k, v in c.expected(mut=mname).items()}, w).values())
                       for c, w in zip(cl, wants)), f"{g.text()}: '{mname}' not caught"
        G.clear_cache()
    assert any(G.straddling_tile(l.geo) > 0 for l in G.ROUTES["small conv"]), "no K tile straddles a tap boundary (cin 96)"
    geoms = A.small_kv_geoms(64)
    assert sorted({g.n_kv * 2 * g.heads * g.d * 2 for g in geoms}) == [61440, 65536]      # bytes of LDS, of 65536 admitted
    for g in geoms:
        mutant = A.MUTANTS["V read at v_off = 0: the K columns"]
        catchers = [c.name for c in A.cases(g, el) if bool(c.first_queries(5).wrong(c.first_queries(5).run(mutant)).any())]
        assert {"counted", "routing", "tilted"} <= set(catchers), (g, catchers)


# ----------------------------------------------------------------------------------------------------- (d)
def library_key(m, n, k, lda, act, residual, out_f32=False, splitk=1, conv=None):
    """vx_gemm_config_name for a STORE launch as ops.gemm sets it up (pointers are dummies: nothing is dereferenced)."""
    from v_express_amd import lib as L
    p, ptr = L.GemmParams(), C.c_void_p(256)
    p.m, p.n, p.k, p.epi, p.alpha, p.splitk, p.act = m, n, k, L.VX_EPI_STORE, 1.0, splitk, act
    p.a = p.w = p.out = ptr
    p.ldc, p.lda1, p.out_f32 = n, lda, int(out_f32)
    if conv is None:
        p.c1, p.kh, p.kw, p.stride, p.nb, p.h_in, p.w_in, p.h_out, p.w_out = k, 1, 1, 1, 1, m, 1, m, 1
    else:
        g = conv
        p.c1, p.kh, p.kw, p.stride, p.pad, p.nb, p.h_in, p.w_in = g.c1, 3, 3, g.stride, g.pad, g.nb, g.h, g.w
        p.h_out, p.w_out = g.out_hw
    if splitk > 1:
        p.splitk_ws, p.ring_hint = ptr, -1
    if residual:
        p.residual, p.ldr = ptr, n
    return L.lib.vx_gemm_config_name(C.byref(p)).decode()


def test_stated_routes_are_the_librarys():
    from v_express_amd import lib as L
    el = torch.bfloat16
    for c in P.window_cases(el) + P.gelu_cases(el):
        sk = 8 if "splitk8" in c.key else 1
        got = library_key(c.t_out, c.n, c.K, c.s * c.C if c.k > 1 else c.C + 24, L.VX_ACT_GELU if c.act == "gelu" else L.VX_ACT_NONE,
                          c.residual, c.out_f32, sk)
        assert got == c.key, (c.text(), got)
    for c in P.positional_cases(el):
        assert library_key(c.T, c.cg, c.K, c.cg, L.VX_ACT_GELU, True) == c.key, c.text()
    for lch in G.ROUTES["small conv"]:
        g = lch.geo
        assert library_key(g.m, g.n, g.k, g.c1 + 24, L.VX_ACT_NONE, False, conv=g) == lch.key, g.text()


# ----------------------------------------------------------------------------------------------------- (e)
PASSES = {"windows": {"tanh-form GELU"}, "positional": {"tanh-form GELU", "sigmoid-form GELU", "last tap dropped"}, "wave": set()}


def test_old_bound_figures(capsys):
    """The reason for this file: what the per-kernel Gaussian tests of the prologue let through (the module docstring)."""
    lines = []
    for which in ("wave", "windows", "positional"):
        fig = P.old_bound_figures(which)
        rel, mx = P.OLD_BOUNDS[which]
        lines.append(f"  {which} (relL2 <= {rel:g}, max|err| <= {mx:g} max|ref|): relL2 / allowed, max|err| / allowed")
        for name, (l2, m) in fig.items():
            inside = l2 <= 1 and m <= 1
            lines.append(f"    {name:45s} {l2:8.3g} / {m:8.3g}   {'PASSES' if inside else 'caught'}")
            if name == "correct":
                assert inside, f"{which}: the rounded reference itself misses the old bound"
            else:
                assert inside == (name in PASSES[which]), f"{which}: '{name}' {'passes' if inside else 'is caught'}: the record is out of date"
    with capsys.disabled():
        print("\nGaussian operands under the bounds of tests/test_gpu_prologue.py [bf16]")
        print("\n".join(lines))
