"""Euler, LMS and PNDM sampling on the MI355X: `vx_overlap_linear_step` (both libraries) against float64 under its
per-update rounding bound over each sampler's real coefficient sequence, VExpressPipeline with each scheduler against the
per-frame restated loop over the oracle UNet, Euler against first-order DPM-Solver++, and merged UNet calls with LMS."""
import numpy as np
import pytest
import torch

import cases
import dpm_restated as D
import linear_multistep_restated as LM
import linear_multistep_worker as LW
from loop_restated import restated_loop
from loop_worker import call_pipeline, call_small as _call, cosine, dev, inputs, oracle_on_cpu, rel_l2, small  # noqa: F401

pytestmark = pytest.mark.gpu

make = LW.scheduler
U = 2.0 ** -24                                   # unit roundoff of float32


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("kind,n", [("euler", 4), ("lms", 6), ("pndm", 5)])
def test_linear_kernel_vs_float64(dev, elem, kind, n):
    """The real coefficient sequence of each sampler - Euler 4 steps; LMS 6 steps (orders 1, 2, 3, 4, 4, 4); PNDM N = 5
    (six entries, every row of its table) - over the reflected-window plan of F = 11, f = 4 on 8 x 8 latents (704 quads: the
    grid has a tail), history and saved starting as NaN (a slot that is not named must not be read).  Each update against
    float64 on the device's own previous state, elementwise, T = max_terms:
        |out - ref| <= (T + 5) 2^-24 (|k_x b| + |k_v| sum_t |p_t / count| + sum_j |c_j h_j|)
        |m - ref|   <= (T + 2) 2^-24 (|p_x x| + |p_v| sum_t |p_t / count|)
    (each product and each sum is one rounding, a contraction only lowers the error).  Two frames outside frame_ids keep
    their bits in every buffer; an Euler step to sigma = 0 leaves x0."""
    from oracle import loop as OL
    from v_express_amd import lib as L, ops
    from v_express_amd.context import overlap_plan
    F_, f, h, w, C, extra = 11, 4, 8, 8, 4, 2
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
    s = make(kind)
    s.set_timesteps(n)
    coefs = [s.linear_coefficients(i) for i in range(len(s.timesteps))]
    if kind == "lms":
        assert [s.order_at(i) for i in range(n)] == [1, 2, 3, 4, 4, 4]
    if kind == "pndm":
        assert len(coefs) == 6 and [c.saved_mode for c in coefs] == [1, 2, 0, 0, 0, 0]
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(1, C, F_ + extra, h, w, generator=g)
    worst_out = worst_m = 0.0
    with L.element_type(elem):
        lat_d = lat.to(dev)
        hist = torch.full((3, C, F_ + extra, h, w), float("nan"), device=dev)
        saved = torch.full_like(lat_d, float("nan"))
        args = (terms.to(dev), torch.tensor(sf, dtype=torch.int32, device=dev), torch.tensor(counts, device=dev))
        for i, cf in enumerate(coefs):
            preds = torch.randn(len(windows), C, f, hw, generator=g)
            x_all, h_all, s_all = lat_d.double().cpu()[0], hist.double().cpu(), saved.double().cpu()[0]
            ops.overlap_linear_step(lat_d, preds.to(dev), *args, hist, saved, cf)
            got, got_h, got_s = lat_d.double().cpu()[0], hist.double().cpu(), saved.double().cpu()[0]
            k_x, k_v, c_1, c_2, c_3, p_x, p_v = (float(np.float32(v)) for v in cf[5:])     # as the kernel receives them
            for k, fr in enumerate(sf):
                ps = [preds[wi, :, li].double().view(C, h, w) / counts[k] for wi, li in plan["terms"][fr]]
                v, vabs = sum(ps), sum(p.abs() for p in ps)
                x = x_all[:, fr]
                b = s_all[:, fr] if cf.saved_mode == 2 else x
                ref, mag = k_x * b + k_v * v, (k_x * b).abs() + abs(k_v) * vabs
                for slot, cj in ((cf.h1, c_1), (cf.h2, c_2), (cf.h3, c_3)):
                    if slot >= 0:
                        ref, mag = ref + cj * h_all[slot, :, fr], mag + (cj * h_all[slot, :, fr]).abs()
                assert torch.isfinite(ref).all() and torch.isfinite(got[:, fr]).all(), (kind, i, fr)
                worst_out = max(worst_out, ((got[:, fr] - ref).abs() / ((T + 5) * U * mag)).max().item())
                if cf.h_write >= 0:
                    m_ref, m_mag = p_x * x + p_v * v, (p_x * x).abs() + abs(p_v) * vabs
                    worst_m = max(worst_m, ((got_h[cf.h_write, :, fr] - m_ref).abs() / ((T + 2) * U * m_mag)).max().item())
                if cf.saved_mode == 1:
                    assert torch.equal(got_s[:, fr], x), (kind, i, fr)
                if kind == "euler" and i == n - 1:
                    a_s, s_s = s.noise_coefficients(i)
                    assert (cf.k_x, cf.k_v) == pytest.approx((a_s, -s_s), rel=1e-15)      # x0 = a x - s v
            # nothing else moved: the frames outside frame_ids, the slots and the saved sample the update does not write
            assert torch.equal(got[:, F_:], lat[0, :, F_:].double())
            assert got_h[:, :, F_:].isnan().all() and got_s[:, F_:].isnan().all()
            for slot in range(3):
                if slot != cf.h_write:
                    assert torch.equal(got_h[slot].nan_to_num(7.0), h_all[slot].nan_to_num(7.0)), (kind, i, slot)
            if cf.saved_mode != 1:
                assert torch.equal(got_s.nan_to_num(7.0), s_all.nan_to_num(7.0)), (kind, i)
        torch.cuda.synchronize()
    print(f"[overlap_linear_step, {kind}, {len(coefs)} updates, {elem}] max |err| / bound: out {worst_out:.3g}, "
          f"history {worst_m:.3g}")
    assert worst_out <= 1.0 and worst_m <= 1.0


# ------------------------------------------------------------------------------------------------ the pipeline
STEPS = {"euler": 6, "lms": 6, "pndm": 5}
_REF = {}


def _restated(small, kind, steps, rounded=False):
    """The float64 per-frame loop over the oracle UNet (its outputs rounded to bfloat16 or not), computed once."""
    from oracle import loop as OL
    key = (kind, steps, rounded)
    if key not in _REF:
        inp = small["inp"]
        unet = LM.bf16_outputs(small["oracle"]) if rounded else small["oracle"]
        windows = OL.uniform_windows(small["F"], small["cf"], small["co"])
        args = (unet, inp["latents"], windows, cases.GUIDANCE, inp["kps_features"], inp["audio_embeddings"], steps)
        with oracle_on_cpu():
            _REF[key] = restated_loop(*args, "ddim") if kind == "ddim" else LM.restated_linear_loop(*args, kind)
    return _REF[key]


def _amplification(small, kind, steps):
    """S: how much more than DDIM (at as many UNet evaluations) the sampler amplifies element-type rounding - the
    relative L2 between the restated loop with the oracle's outputs rounded to bfloat16 and without, over DDIM's."""
    evals = steps + (1 if kind == "pndm" else 0)
    own = rel_l2(_restated(small, kind, steps, True), _restated(small, kind, steps))
    ddim = rel_l2(_restated(small, "ddim", evals, True), _restated(small, "ddim", evals))
    return own / ddim, own, ddim


@pytest.mark.parametrize("kind", LM.SAMPLERS)
def test_pipeline_vs_restated_oracle_loop(small, kind):
    """reflected_F11_c4o2: relative L2 <= 5e-2 max(1, S) and cosine >= 0.998 - the project's bound for this clip
    (tests/test_gpu_dpm_solver.py), widened only by the sampler's own amplification S of element-type rounding."""
    steps = STEPS[kind]
    got = _call(small, make(kind), steps)
    ref = _restated(small, kind, steps)
    S, own, ddim = _amplification(small, kind, steps)
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[{kind}, SMALL, reflected_F11_c4o2, {steps} steps] relL2={r:.4g} cosine={c:.6f} vs the restated loop; "
          f"S = {S:.3g} (bf16-rounded outputs move the restated loop by {own:.3g}, DDIM's by {ddim:.3g})")
    assert torch.isfinite(got).all() and r <= 5e-2 * max(1.0, S) and c >= 0.998, (r, c, S)


def test_euler_matches_first_order_dpm_solver(small):
    """Euler is first-order DPM-Solver++'s update on the same sigmas (tests/test_linear_multistep_cpu.py compares the
    coefficients); the two clips differ by the rounding of the two kernels' different operation order, as first-order
    DPM++ and DDIM do (test_first_order_dpm_solver_matches_the_ddim_pipeline: the bf16 rounding of the UNet inputs)."""
    from v_express_amd import DPMSolverMultistepScheduler
    euler = _call(small, make("euler"), 10)
    dpm1 = _call(small, DPMSolverMultistepScheduler(**{**D.KWARGS, "solver_order": 1}), 10)
    r = rel_l2(euler, dpm1)
    print(f"[10 steps, SMALL, reflected_F11_c4o2] Euler vs first-order DPM++ relL2={r:.4g}")
    assert torch.isfinite(euler).all() and r <= 1e-2


def test_merged_unet_calls_are_bit_identical_with_lms(small):
    """F = 6 in windows of 4 with overlap 2 (two windows): one UNet call per window (units_per_call 2) against both in one
    call (4), LMS at 5 steps (fourth order reached)."""
    pipe, clips = small["pipe"], {}
    upc = pipe.units_per_call
    try:
        for n in (2, 4):
            pipe.units_per_call = n
            clips[n] = call_pipeline(pipe, make("lms"), inputs(6), 6, 5, small["cf"], small["co"]).cpu()
    finally:
        pipe.units_per_call = upc
    assert pipe.last_overlap["windows"] == 2
    assert torch.isfinite(clips[2]).all() and torch.equal(clips[2], clips[4])
