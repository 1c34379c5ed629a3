"""Guidance reuse on the MI355X: `vx_combine_units_keep` against `vx_combine_units` / `vx_combine_units3` bit for bit and
against the float32 subtraction, `vx_combine_reused` on inputs whose answer is exact, against the float32 torch expression
in its stated order bit for bit and against float64 under the derived bound, their argument errors and guard bands (both
element libraries; the code is float32 in both), and VExpressPipeline with `guidance_refresh` against the restated loop
over the oracle UNet (tests/guidance_reuse_restated.py)."""
import pytest
import torch

import guidance_reuse_restated as GR
from guard import assert_same_bits
from loop_worker import call_small, dev, oracle_on_cpu, rel_l2, scheduler, small  # noqa: F401
from test_gpu_apg import layout, predictions

pytestmark = pytest.mark.gpu

ELEMS = [torch.bfloat16, torch.float16]
# 480 threads: a partial last block; c = 3 (no channel pairs left over evenly); one window
SHAPES = [(2, 4, 4, 60), (2, 3, 2, 300), (1, 4, 4, 80)]
S, S_A = 3.5, 6.0


def keep(ops, dev, rows, granules, seed, s=S, s_a=S_A):
    """One ops.combine_units_keep call on the rows (2 or 3 tensors [nW, c, f, hw]) scattered by `layout`: (preds, diffs,
    the device buffers gathered / unit_index)."""
    nW, c, f, hw = rows[0].shape
    gathered, uidx = layout(rows, granules, seed)
    gathered, uidx = gathered.to(dev), uidx.to(dev)
    preds = torch.full((nW, c, f, hw), float("nan"), device=dev)
    diffs = torch.full((len(rows) - 1, nW, c, f, hw), float("nan"), device=dev)
    ops.combine_units_keep(gathered, uidx, c, f, hw, s, s_a, diffs, preds)
    torch.cuda.synchronize()
    return preds.cpu(), diffs.cpu(), gathered, uidx


def reused(ops, dev, cnd, last, prev, coef, granules=1, seed=0):
    """One ops.combine_reused call on the conditional row cnd [nW, c, f, hw] and the slots last / prev [n, nW, c, f, hw]."""
    nW, c, f, hw = cnd.shape
    gathered, uidx = layout((cnd,), granules, seed)
    preds = torch.full((nW, c, f, hw), float("nan"), device=dev)
    ops.combine_reused(gathered.to(dev), uidx.to(dev), c, f, hw, last.to(dev), None if prev is None else prev.to(dev),
                       *coef, preds)
    torch.cuda.synchronize()
    return preds.cpu()


# ------------------------------------------------------------------------------------------------ vx_combine_units_keep
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("granules", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_keep_is_the_plain_combine_and_the_float32_differences(dev, elem, shape, granules):
    from v_express_amd import lib as L, ops
    u, m, c = predictions(*shape, 3.0, seed=shape[3] + granules)
    with L.element_type(elem):
        for rows in ((u, c), (u, m, c)):
            preds, diffs, gathered, uidx = keep(ops, dev, rows, granules, seed=len(rows))
            base = torch.full(shape, float("nan"), device=dev)
            if len(rows) == 2:
                ops.combine_units(gathered, uidx, shape[1], shape[2], shape[3], S, base)
            else:
                ops.combine_units3(gathered, uidx, shape[1], shape[2], shape[3], S, S_A, base)
            torch.cuda.synchronize()
            assert torch.isfinite(preds).all()
            assert_same_bits(preds, base.cpu(), f"vx_combine_units_keep rows={len(rows)} {shape} granules={granules}: preds")
            for k in range(len(rows) - 1):
                assert_same_bits(diffs[k], rows[k + 1] - rows[k], f"vx_combine_units_keep rows={len(rows)} {shape}: diffs[{k}]")


# ------------------------------------------------------------------------------------------------ vx_combine_reused
def halves(shape, seed):
    """Multiples of 1 / 2 in [-4, 4]: with the dyadic coefficients below every product and every sum is exact."""
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float() / 2


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_reused_exact_answers(dev, elem, shape):
    """s = 3.5, w = 1: a = 5, b = -2.5; s_a = 6: a = 10, b = -5; hold (w = 0): a = 2.5 and 5."""
    from v_express_amd import lib as L, ops, sampling
    assert sampling.reuse_coefficients((S, S_A), 1.0) == [(5.0, -2.5), (10.0, -5.0)]
    assert sampling.reuse_coefficients((S, S_A), 0.0) == [(2.5, 0.0), (5.0, 0.0)]
    cnd, l1, p1, l2, p2 = (halves(shape, seed) for seed in range(5))
    last, prev = torch.stack([l1, l2]), torch.stack([p1, p2])
    with L.element_type(elem):
        for granules in (1, 2):
            got = reused(ops, dev, cnd, last, prev, (5.0, -2.5, 10.0, -5.0), granules, seed=granules)
            assert_same_bits(got, (cnd.double() + 5 * l1.double() - 2.5 * p1.double() + 10 * l2.double()
                                   - 5 * p2.double()).float(), f"two differences, linear {shape}")
            got = reused(ops, dev, cnd, last[:1], prev[:1], (5.0, -2.5, 0.0, 0.0), granules, seed=granules)
            assert_same_bits(got, cnd + 5 * l1 - 2.5 * p1, f"one difference, linear {shape}")
            got = reused(ops, dev, cnd, last, None, (2.5, 0.0, 5.0, 0.0), granules, seed=granules)
            assert_same_bits(got, cnd + 2.5 * l1 + 5 * l2, f"two differences, hold {shape}")
            got = reused(ops, dev, cnd, last[:1], None, (2.5, 0.0, 0.0, 0.0), granules, seed=granules)
            assert_same_bits(got, cnd + 2.5 * l1, f"one difference, hold {shape}")


COEFS = [(2.5, 0.0, 0.0, 0.0), (3.75, -1.25, 0.0, 0.0), (2.5, 0.0, 5.0, 0.0), (3.75, -1.25, 7.5, -2.5),
         (0.3 * (1 + 1 / 3), -0.1, 1.7 * (1 + 1 / 3), -1.7 / 3)]


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_reused_vs_the_float32_expression_and_float64(dev, elem, shape):
    """On Gaussian rows the output holds the bits of the float32 torch expression in the stated order (nothing is
    contracted), and against float64 |err| <= (T + 2) 2^-24 (|c| + sum |a_k L_k| + sum |b_k P_k|), T the number of terms:
    each of the T sums is rounded once, at most 2^-24 of a partial sum that the magnitude bounds, and the T products
    together err by at most 2^-24 of the magnitude (each by 2^-24 of its own term): T + 1, and one more for the second
    order.  The coefficients are float32 values on both sides.  Measured on the MI355X, both libraries: the largest
    |err| is 0.46 (c = 4) / 0.46 (c = 3) of the bound."""
    from v_express_amd import lib as L, ops
    u, m, c = predictions(*shape, 3.0, seed=shape[3])
    _, m2, c2 = predictions(*shape, 3.0, seed=shape[3] + 1)
    last, prev = torch.stack([m - u, c - m]), torch.stack([m2 - u, c2 - m2])

    def f32(v):
        return float(torch.tensor(v, dtype=torch.float32))
    worst = 0.0
    with L.element_type(elem):
        for coef in COEFS:
            coef = tuple(f32(v) for v in coef)
            n = 2 if coef[2] != 0.0 else 1
            pv = prev[:n] if coef[1] != 0.0 else None
            for granules in (1, 2):
                got = reused(ops, dev, c, last[:n], pv, coef, granules, seed=granules)
                assert_same_bits(got, GR.reused_f32(c, last[:n], pv, *coef), f"vx_combine_reused {shape} {coef}")
            ref, mag, terms = c.double(), c.double().abs(), 0
            for k in range(n):
                for coefficient, slot in ((coef[2 * k], last), (coef[2 * k + 1], pv)):
                    if slot is not None and coefficient != 0.0:
                        ref = ref + coefficient * slot[k].double()
                        mag = mag + (coefficient * slot[k].double()).abs()
                        terms += 1
            ratio = ((got.double() - ref).abs() / (2.0 ** -24 * mag)).max().item()
            worst = max(worst, ratio / (terms + 2))
            assert ratio <= terms + 2, (coef, ratio)
    print(f"[vx_combine_reused {elem}, {shape}] largest |err| / ((T + 2) 2^-24 magnitude) = {worst:.3g}")


@pytest.mark.parametrize("elem", ELEMS)
def test_reused_without_prev_is_the_two_slot_call_with_b_zero(dev, elem):
    """prev = NULL (every b is 0) runs the kernel without the P terms.  The entry point refuses prev together with b = 0
    everywhere, so the two-slot kernel's b = 0 is reached with b1 = 1 on a P1 of zeros (it adds +0) and, with two
    differences, b2 = 0 on a finite P2: the same bits as without prev."""
    from v_express_amd import lib as L, ops
    shape = (2, 4, 4, 60)
    u, m, c = predictions(*shape, 3.0, seed=11)
    last, prev = torch.stack([m - u, c - m]), torch.stack([torch.zeros_like(u), u - m])
    with L.element_type(elem):
        for n, a2 in ((1, 0.0), (2, 5.0)):
            alone = reused(ops, dev, c, last[:n], None, (2.5, 0.0, a2, 0.0))
            both = reused(ops, dev, c, last[:n], prev[:n], (2.5, 1.0, a2, 0.0))
            assert_same_bits(alone, both, f"prev = NULL against the two-slot kernel, n_diffs = {n}")
            assert_same_bits(alone, GR.reused_f32(c, last[:n], None, 2.5, 0.0, a2, 0.0), f"prev = NULL, n_diffs = {n}")


# ------------------------------------------------------------------------------------------------ errors, guard bands
@pytest.mark.parametrize("elem", ELEMS)
def test_kernel_argument_errors(dev, elem):
    from v_express_amd import lib as L, ops
    u, _, c = predictions(1, 4, 4, 16, 0.0, seed=1)
    gathered, uidx = layout((u, c), 1, 0)
    gathered, uidx = gathered.to(dev), uidx.to(dev)
    preds = torch.zeros(1, 4, 4, 16, device=dev)
    diffs, last, prev = (torch.zeros(1, 1, 4, 4, 16, device=dev) for _ in range(3))
    with L.element_type(elem):
        GR.check_argument_errors(L.current(), gathered.data_ptr(), uidx.data_ptr(), diffs.data_ptr(), last.data_ptr(),
                                 prev.data_ptr(), preds.data_ptr())
        one = uidx[:, 1:].contiguous()
        with pytest.raises(ValueError, match="prev"):
            ops.combine_reused(gathered, one, 4, 4, 16, last, None, 2.5, -1.25, 0.0, 0.0, preds)
        with pytest.raises(ValueError, match="prev"):
            ops.combine_reused(gathered, one, 4, 4, 16, last, prev, 2.5, 0.0, 0.0, 0.0, preds)
    torch.cuda.synchronize()
    assert not preds.any() and not diffs.any()                     # nothing was launched


@pytest.mark.parametrize("hw", [80, 1040])
@pytest.mark.parametrize("c", [4, 3])
def test_guard_bands(dev, hw, c):
    """tests/test_gpu_guard_bands.py's sweep on both launches, two rows and three: nothing is written outside preds and
    diffs, nothing outside gathered / unit_index / last / prev is depended on (three runs with the outside zero / NaN /
    huge, bit-equal), and the inputs keep their bits."""
    from test_gpu_guard_bands import F32, G, O, sweep
    from v_express_amd import lib as L, ops
    nW, f, gran = 2, 4, 2
    rows3 = predictions(nW, c, f, hw, 3.0, seed=hw + c)
    with L.element_type(torch.bfloat16):
        for rows in ((rows3[0], rows3[2]), rows3):
            n = len(rows) - 1
            gathered, uidx = layout(rows, gran, seed=len(rows))
            gathered = torch.nan_to_num(gathered)
            gg, gi = G(gathered, F32), G(uidx, torch.int32)
            preds, diffs = O((nW, c, f, hw), F32), O((n, nW, c, f, hw), F32)
            got, kept = sweep(f"combine_units_keep rows={len(rows)}", [gg, gi], [preds, diffs],
                              lambda: ops.combine_units_keep(gg.view, gi.view, c, f, hw, S, S_A, diffs.view, preds.view))
            for k in range(n):
                assert_same_bits(kept[k].cpu(), rows[k + 1] - rows[k], f"guarded diffs[{k}]")
            assert_same_bits(gg.view.cpu(), gathered, "gathered")
            assert_same_bits(gi.view.cpu(), uidx, "unit_index")
            # the reuse step on the slots the refresh wrote, and on a second pair
            cg, ci = layout((rows[-1],), gran, seed=7)
            cg, ci = G(torch.nan_to_num(cg), F32), G(ci, torch.int32)
            last_t, prev_t = kept.cpu(), (0.5 * kept).cpu()
            last, prev = G(last_t, F32), G(prev_t, F32)
            coef = (3.75, -1.25, 7.5, -2.5) if n == 2 else (3.75, -1.25, 0.0, 0.0)
            out, = sweep(f"combine_reused n_diffs={n}", [cg, ci, last, prev], [preds],
                         lambda: ops.combine_reused(cg.view, ci.view, c, f, hw, last.view, prev.view, *coef, preds.view))
            assert_same_bits(out.cpu(), GR.reused_f32(rows[-1], last_t, prev_t, *coef), "guarded combine_reused")
            assert_same_bits(last.view.cpu(), last_t, "last")
            assert_same_bits(prev.view.cpu(), prev_t, "prev")
            hold = (coef[0], 0.0, coef[2], 0.0)
            out, = sweep(f"combine_reused n_diffs={n}, prev NULL", [cg, ci, last], [preds],
                         lambda: ops.combine_reused(cg.view, ci.view, c, f, hw, last.view, None, *hold, preds.view))
            assert_same_bits(out.cpu(), GR.reused_f32(rows[-1], last_t, None, *hold), "guarded combine_reused, hold")


# ------------------------------------------------------------------------------------------------ the pipeline
STEPS, K = 6, 2                    # refreshes at steps 0, 2, 4, 5; reuse at 1 and 3 ("linear": w = 1 / 2 at step 3)


def _windows(small):
    from oracle import loop as OL
    return OL.uniform_windows(small["F"], small["cf"], small["co"])


@pytest.mark.parametrize("mode", GR.MODES)
@pytest.mark.parametrize("s_a", [None, S_A], ids=["two_rows", "three_rows"])
def test_pipeline_vs_restated_oracle_loop(small, s_a, mode):
    """reflected_F11_c4o2, 6 DDIM steps, k = 2, against the restated float64 loop with reuse over the oracle UNet, within
    the siblings' bound 5e-2 max(1, S); S (guidance_reuse_restated.l1_ratio) is the largest ratio, over the steps, of the
    L1 weight on UNet outputs in the step's guided prediction to plain CFG's |1 - s| + |s| = 6: two rows 1 (hold) and
    11 / 6 (linear), three rows 16 / 6 (hold) and 31 / 6 (linear).  Measured on the MI355X: two rows relL2 9.80e-3 (hold)
    and 1.05e-2 (linear), three rows 1.48e-2 and 1.55e-2; the plain clip lies at 2.7e-2 to 4.4e-2 of those loops."""
    inp = small["inp"]
    audio = {} if s_a is None else dict(audio_guidance_scale=s_a)
    plain = call_small(small, scheduler("ddim"), STEPS, **audio)
    assert "refresh" not in small["pipe"].last_guidance
    same = call_small(small, scheduler("ddim"), STEPS, guidance_refresh=1, guidance_reuse=mode, **audio)
    assert torch.equal(plain, same)
    got = call_small(small, scheduler("ddim"), STEPS, guidance_refresh=K, guidance_reuse=mode, **audio)
    lg = small["pipe"].last_guidance
    assert lg["refresh"] == K and lg["reuse"] == mode and lg["refresh_steps"] == [0, 2, 4, 5]
    assert lg["unguided_schedule"] is not None
    with oracle_on_cpu():
        ref, state = GR.restated_loop(small["oracle"], inp["latents"], _windows(small), S, inp["kps_features"],
                                      inp["audio_embeddings"], STEPS, "ddim", s_a=s_a, k=K, mode=mode)
    assert state.log == ["refresh", "reuse", "refresh", "reuse", "refresh", "refresh"]
    s_ratio = GR.l1_ratio(("u", "c") if s_a is None else ("u", "m", "c"), S, s_a, [True] * STEPS, K, mode)
    r = rel_l2(got, ref)
    print(f"[DDIM, guidance_refresh {K} {mode}, audio_guidance_scale {s_a}, SMALL, reflected_F11_c4o2, {STEPS} steps] "
          f"relL2={r:.4g} vs the restated loop with reuse (S = {s_ratio:.4g}, bound {5e-2 * max(1.0, s_ratio):.4g}); the "
          f"plain clip vs that loop: relL2={rel_l2(plain, ref):.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2 * max(1.0, s_ratio), (r, s_ratio)
    assert rel_l2(got, plain) > 1e-4


def test_pipeline_dpm_multistep_history_is_unaffected(small):
    """One DPM++ 2M run with k = 2 ("hold", two rows: S = 1) within the same bound: the multistep history takes the
    prediction of a reuse step like any other.  Measured on the MI355X: relL2 9.28e-3."""
    inp = small["inp"]
    got = call_small(small, scheduler("dpm"), STEPS, guidance_refresh=K)
    assert small["pipe"].last_guidance["refresh_steps"] == [0, 2, 4, 5]
    with oracle_on_cpu():
        ref, _ = GR.restated_loop(small["oracle"], inp["latents"], _windows(small), S, inp["kps_features"],
                                  inp["audio_embeddings"], STEPS, "dpm", k=K, mode="hold")
    r = rel_l2(got, ref)
    print(f"[DPM++ 2M, guidance_refresh {K} hold, SMALL, reflected_F11_c4o2, {STEPS} steps] relL2={r:.4g} vs the restated "
          f"loop with reuse (bound 5e-2)")
    assert torch.isfinite(got).all() and r <= 5e-2 * max(1.0, GR.l1_ratio(("u", "c"), S, None, [True] * STEPS, K, "hold"))
