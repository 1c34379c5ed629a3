"""UniPC sampling on the MI355X: `vx_overlap_unipc_step` (both libraries) on the exact-answer cases of tests/unipc_cases.py
inside guard bands, against float64 under its per-update rounding bound over the scheduler's real coefficient sequence,
VExpressPipeline with the scheduler against the per-frame restated loop over the oracle UNet, and merged UNet calls."""
import numpy as np
import pytest
import torch

import cases
import guard
import unipc_cases as UC
import unipc_restated as U
import unipc_worker as UW
from loop_restated import restated_loop
from loop_worker import call_pipeline, call_small as _call, cosine, dev, inputs, oracle_on_cpu, rel_l2, small  # noqa: F401

pytestmark = pytest.mark.gpu

make = UW.scheduler
EPS = 2.0 ** -24                                 # unit roundoff of float32
CASES = UC.cases()


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_exact_answer_cases(dev, elem, case):
    """Every buffer inside guard bands: the kernel leaves the bits of the float64 reference (every intermediate is exact in
    float32, contracted or not), the bits of everything it must not write - frames outside frame_ids, history slots other
    than h_write, preds - and nothing outside the buffers."""
    from v_express_amd import lib as L, ops
    from v_express_amd.scheduler import UniPCStep
    with L.element_type(elem):
        bufs = {k: guard.Guarded(case[k].shape, torch.float32, dev).load(torch.from_numpy(case[k]))
                for k in ("latents", "preds", "history", "saved")}
        ops.overlap_unipc_step(bufs["latents"].view, bufs["preds"].view, torch.from_numpy(case["terms"]).to(dev),
                               torch.from_numpy(case["frame_ids"]).to(dev), torch.from_numpy(case["counts"]).to(dev),
                               bufs["history"].view, bufs["saved"].view, UniPCStep(*case["coef"]))
        torch.cuda.synchronize()
    for k, want in zip(("latents", "history", "saved"), UC.reference(case)):
        bufs[k].assert_intact(f"{case['name']}: {k}")
        guard.assert_same_bits(bufs[k].view.cpu(), torch.from_numpy(want.astype(np.float32)), f"{case['name']}: {k}")
    bufs["preds"].assert_intact(f"{case['name']}: preds")
    guard.assert_same_bits(bufs["preds"].view.cpu(), torch.from_numpy(case["preds"]), f"{case['name']}: preds")


@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
def test_unipc_kernel_vs_float64(dev, elem, solver_type):
    """The real coefficient sequence of a third-order run of 6 steps (predictor orders 1, 2, 3, 3, 2, 1; the corrector at
    orders 1, 2, 3, 3 and skipped before the step to sigma = 0) over the reflected-window plan of F = 11, f = 4 on 8 x 8
    latents (704 quads: the grid has a tail), history and saved starting as NaN (what is not named must not be read).
    Each update against float64 on the device's own previous state, elementwise, with T = max_terms and the magnitudes
    |.| the sums of the absolute values of the terms of the expanded expressions (include/vexpress_hip_solvers.h):
        |m - ref|   <= (T + 2)  2^-24 |m|      |xc - ref| <= (T + 7) 2^-24 |xc|      |out - ref| <= (T + 11) 2^-24 |out|
    Two frames outside frame_ids keep their bits in every buffer; the step to sigma = 0 leaves m."""
    from oracle import loop as OL
    from v_express_amd import lib as L, ops
    from v_express_amd.context import overlap_plan
    F_, f, h, w, C, extra, n = 11, 4, 8, 8, 4, 2, 6
    hw = h * w
    windows = OL.uniform_windows(F_, f, 2)
    plan = overlap_plan(windows, F_)
    sf, T = plan["step_frames"], plan["max_terms"]
    assert sorted(sf) == list(range(F_)) and len(sf) * C * hw // 4 == 704 and T >= 2
    terms = torch.full((len(sf), T, 2), -1, dtype=torch.int32)
    for i, fr in enumerate(sf):
        for j, (wi, li) in enumerate(plan["terms"][fr]):
            terms[i, j, 0], terms[i, j, 1] = wi, li
    counts = [float(plan["counts"][fr]) for fr in sf]
    s = make(solver_order=3, solver_type=solver_type)
    s.set_timesteps(n)
    _, coefs = s.loop_steps(s.timesteps.tolist(), 0)
    assert [s.solver_order_at(i) for i in range(n)] == [1, 2, 3, 3, 2, 1]
    assert [c.use_c for c in coefs] == [0, 1, 1, 1, 1, 0] and coefs[3].h3 == coefs[3].h_write
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(1, C, F_ + extra, h, w, generator=g)
    worst = dict(m=0.0, xc=0.0, out=0.0)
    with L.element_type(elem):
        lat_d = lat.to(dev)
        hist = torch.full((3, C, F_ + extra, h, w), float("nan"), device=dev)
        saved = torch.full_like(lat_d, float("nan"))
        args = (terms.to(dev), torch.tensor(sf, dtype=torch.int32, device=dev), torch.tensor(counts, device=dev))
        for i, cf in enumerate(coefs):
            preds = torch.randn(len(windows), C, f, hw, generator=g)
            x_all, h_all, s_all = lat_d.double().cpu()[0], hist.double().cpu(), saved.double().cpu()[0]
            ops.overlap_unipc_step(lat_d, preds.to(dev), *args, hist, saved, cf)
            got, got_h, got_s = lat_d.double().cpu()[0], hist.double().cpu(), saved.double().cpu()[0]
            a_i, s_i, q_s, q_m, q_1, q_2, q_3, k_x, k_m, k_1, k_2 = (float(np.float32(v)) for v in cf[5:])  # as the kernel receives them
            for k, fr in enumerate(sf):
                ps = [preds[wi, :, li].double().view(C, h, w) / counts[k] for wi, li in plan["terms"][fr]]
                v, vabs = sum(ps), sum(p.abs() for p in ps)
                x = x_all[:, fr]
                m_ref, m_mag = a_i * x - s_i * v, (a_i * x).abs() + abs(s_i) * vabs
                xc_ref, xc_mag = x, x.abs()
                if cf.use_c:
                    sv = s_all[:, fr]
                    xc_ref, xc_mag = q_s * sv + q_m * m_ref, (q_s * sv).abs() + abs(q_m) * m_mag
                    for slot, q in ((cf.h1, q_1), (cf.h2, q_2), (cf.h3, q_3)):
                        if slot >= 0:
                            xc_ref, xc_mag = xc_ref + q * h_all[slot, :, fr], xc_mag + (q * h_all[slot, :, fr]).abs()
                ref, mag = k_x * xc_ref + k_m * m_ref, abs(k_x) * xc_mag + abs(k_m) * m_mag
                for slot, kk in ((cf.h1, k_1), (cf.h2, k_2)):
                    if slot >= 0:
                        ref, mag = ref + kk * h_all[slot, :, fr], mag + (kk * h_all[slot, :, fr]).abs()
                assert torch.isfinite(ref).all() and torch.isfinite(got[:, fr]).all(), (i, fr)
                assert torch.isfinite(got_s[:, fr]).all() and torch.isfinite(got_h[cf.h_write, :, fr]).all(), (i, fr)
                worst["out"] = max(worst["out"], ((got[:, fr] - ref).abs() / ((T + 11) * EPS * mag)).max().item())
                worst["m"] = max(worst["m"], ((got_h[cf.h_write, :, fr] - m_ref).abs() / ((T + 2) * EPS * m_mag)).max().item())
                if cf.use_c:
                    worst["xc"] = max(worst["xc"], ((got_s[:, fr] - xc_ref).abs() / ((T + 7) * EPS * xc_mag)).max().item())
                else:
                    assert torch.equal(got_s[:, fr], x), (i, fr)
                if i == n - 1:                                   # the step to sigma = 0: m itself
                    assert torch.equal(got[:, fr], got_h[cf.h_write, :, fr]), (i, fr)
            # nothing else moved: the frames outside frame_ids and the slots the update does not write
            assert torch.equal(got[:, F_:], lat[0, :, F_:].double())
            assert got_h[:, :, F_:].isnan().all() and got_s[:, F_:].isnan().all()
            for slot in range(3):
                if slot != cf.h_write:
                    assert torch.equal(got_h[slot].nan_to_num(7.0), h_all[slot].nan_to_num(7.0)), (i, slot)
        torch.cuda.synchronize()
    print(f"[overlap_unipc_step, order 3 {solver_type}, {n} updates, {elem}, T = {T}] max |err| / bound: m {worst['m']:.3g} "
          f"(K = T + 2), xc {worst['xc']:.3g} (K = T + 7), out {worst['out']:.3g} (K = T + 11)")
    assert max(worst.values()) <= 1.0


# ------------------------------------------------------------------------------------------------ the pipeline
STEPS = 6
_REF = {}


def _restated(small, kind, rounded=False):
    """The float64 per-frame loop over the oracle UNet (its outputs rounded to bfloat16 or not), computed once; kind:
    "ddim" or UniPC's solver order."""
    from oracle import loop as OL
    key = (kind, rounded)
    if key not in _REF:
        inp = small["inp"]
        unet = U.bf16_outputs(small["oracle"]) if rounded else small["oracle"]
        windows = OL.uniform_windows(small["F"], small["cf"], small["co"])
        args = (unet, inp["latents"], windows, cases.GUIDANCE, inp["kps_features"], inp["audio_embeddings"], STEPS)
        with oracle_on_cpu():
            _REF[key] = restated_loop(*args, "ddim") if kind == "ddim" else U.restated_unipc_loop(*args, solver_order=kind)
    return _REF[key]


def _amplification(small, order):
    """S: how much more than DDIM (at as many UNet evaluations) the sampler amplifies element-type rounding - the
    relative L2 between the restated loop with the oracle's outputs rounded to bfloat16 and without, over DDIM's.  From
    the restated loops alone, never from the code under test."""
    own = rel_l2(_restated(small, order, True), _restated(small, order))
    ddim = rel_l2(_restated(small, "ddim", True), _restated(small, "ddim"))
    return own / ddim, own, ddim


@pytest.mark.parametrize("order", [2, 3])
def test_pipeline_vs_restated_oracle_loop(small, order):
    """reflected_F11_c4o2: relative L2 <= 5e-2 max(1, S) and cosine >= 0.998 - the project's bound for this clip
    (tests/test_gpu_linear_multistep.py), widened only by the sampler's own amplification S of element-type rounding."""
    got = _call(small, make(solver_order=order), STEPS)
    ref = _restated(small, order)
    S, own, ddim = _amplification(small, order)
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[unipc order {order}, SMALL, reflected_F11_c4o2, {STEPS} steps] relL2={r:.4g} cosine={c:.6f} vs the restated "
          f"loop; S = {S:.3g} (bf16-rounded outputs move the restated loop by {own:.3g}, DDIM's by {ddim:.3g})")
    assert torch.isfinite(got).all() and r <= 5e-2 * max(1.0, S) and c >= 0.998, (r, c, S)


def test_merged_unet_calls_are_bit_identical(small):
    """F = 6 in windows of 4 with overlap 2 (two windows): one UNet call per window (units_per_call 2) against both in one
    call (4), UniPC of order 3 at 5 steps (third order and its corrector reached)."""
    pipe, clips = small["pipe"], {}
    upc = pipe.units_per_call
    try:
        for n in (2, 4):
            pipe.units_per_call = n
            clips[n] = call_pipeline(pipe, make(solver_order=3), inputs(6), 6, 5, small["cf"], small["co"]).cpu()
    finally:
        pipe.units_per_call = upc
    assert pipe.last_overlap["windows"] == 2
    assert torch.isfinite(clips[2]).all() and torch.equal(clips[2], clips[4])
