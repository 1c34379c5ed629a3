"""DPM-Solver++ multistep sampling on the host: v_express_amd.DPMSolverMultistepScheduler's tables, order rule and update
coefficients against float64 restatements (tests/dpm_restated.py), the stateful `step()` inside the oracle's
mean-overlap loop, convergence on an analytic model against DDIM, and VExpressPipeline.__call__ with the DPM-Solver++
update under emulated kernels (one process and two gloo ranks)."""
import math

import numpy as np
import pytest
import torch

import cases
import dpm_restated as D
from loop_restated import restated_loop
from loop_worker import call_pipeline, emulated, inputs, oracle_unet, rel_l2, spawn_gloo  # noqa: F401


def make(**kw):
    from v_express_amd import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**{**D.KWARGS, **kw})


# ------------------------------------------------------------------------------------------------ (a) tables
@pytest.mark.parametrize("n", [5, 12, 15, 25])
def test_timesteps_and_sigma_table(n):
    s = make()
    s.set_timesteps(n)
    assert s.timesteps.tolist() == D.timesteps(n)
    assert s.timesteps.tolist() == [int(t) for t in np.round(np.arange(1000, 0, -1000 / n)).astype(np.int64) - 1]
    assert s.sigmas.dtype == torch.float32 and len(s.sigmas) == n + 1
    ref = D.sigmas(n)
    # float32 tables (cumulative product, zero-SNR rescale) against float64
    assert max(abs(float(a) / b - 1) for a, b in zip(s.sigmas[:n], ref[:n])) <= 2e-4
    # the 2^-24 clamp: abar[999] = 2^-24 exactly, sigma(999) = sqrt(2^24 - 1)
    assert float(s.alphas_cumprod[-1]) == 2.0 ** -24 and s.timesteps[0] == 999
    assert float(s.sigmas[0]) == pytest.approx(math.sqrt(2.0 ** 24 - 1), rel=1e-7)
    assert float(s.sigmas[-1]) == 0.0
    m = make(final_sigmas_type="sigma_min")
    m.set_timesteps(n)
    assert torch.equal(m.sigmas[:n], s.sigmas[:n])
    # sigma(0): 1 - abar_0 = 8.5e-4 in float32 keeps about four digits
    assert float(m.sigmas[-1]) == pytest.approx(D.sigmas(n, "sigma_min")[-1], rel=1e-4) and float(m.sigmas[-1]) > 0


@pytest.mark.parametrize("n", [5, 12, 15, 25])
@pytest.mark.parametrize("opts", [dict(), dict(solver_order=1), dict(final="sigma_min"),
                                  dict(final="sigma_min", lower_order_final=False),
                                  dict(final="sigma_min", euler_at_final=True, lower_order_final=False)])
def test_order_schedule(n, opts):
    kw = dict(solver_order=opts.get("solver_order", 2), lower_order_final=opts.get("lower_order_final", True),
              euler_at_final=opts.get("euler_at_final", False), final_sigmas_type=opts.get("final", "zero"))
    s = make(**kw)
    s.set_timesteps(n)
    want = D.orders(n, kw["solver_order"], kw["lower_order_final"], kw["euler_at_final"], kw["final_sigmas_type"])
    assert [s.solver_order_at(i) for i in range(n)] == want
    # the rules spelled out: first order at i = 0; the last step is first order below 15 steps (lower_order_final) or
    # when it ends at sigma = 0; i = n - 2 stays second order (diffusers' lower_order_second only lowers third order)
    assert want[0] == 1
    if kw["solver_order"] == 2:
        last_first = kw["final_sigmas_type"] == "zero" or kw["euler_at_final"] or (kw["lower_order_final"] and n < 15)
        assert want[-1] == (1 if last_first else 2)
        assert want[1:-1] == [2] * (n - 2)
    else:
        assert want == [1] * n
    # a run that starts later (strength < 1) starts at first order
    assert s.solver_order_at(2, begin_index=2) == 1


@pytest.mark.parametrize("n,final", [(5, "zero"), (12, "sigma_min"), (15, "zero"), (25, "sigma_min")])
def test_coefficients_vs_float64_restatement(n, final):
    s = make(final_sigmas_type=final)
    s.set_timesteps(n)
    sg = [float(v) for v in s.sigmas]                  # the float32 table, restated arithmetic in float64
    for i in range(n):
        got = s.multistep_coefficients(i)
        ref = D.coefficients(sg, i, s.solver_order_at(i))
        assert all(isinstance(v, float) and math.isfinite(v) for v in got)
        for a, b in zip(got, ref):
            assert a == pytest.approx(b, rel=1e-12, abs=1e-15), (i, got, ref)
    # the collapsed coefficients reproduce diffusers' update form on tensors
    g = torch.Generator().manual_seed(0)
    x, v, xp = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(3))
    for i in range(n):
        a, sd, cx, c0, c1 = s.multistep_coefficients(i)
        x0 = a * x - sd * v
        ref, _ = D.update(sg, i, s.solver_order_at(i), x, v, xp)
        assert rel_l2(cx * x - c0 * x0 + c1 * xp, ref) <= 1e-12


def test_step_ending_at_sigma_zero_returns_x0_exactly():
    s = make()
    s.set_timesteps(5)
    assert s.multistep_coefficients(4) == (*s.multistep_coefficients(4)[:2], 0.0, -1.0, 0.0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 4, 3, 8, 8, generator=g)
    for t in s.timesteps.tolist():
        v = torch.randn(x.shape, generator=g)
        out = s.step(v, t, x)
        x = out.prev_sample
    assert torch.equal(x, out.pred_original_sample)


def test_options_and_construction():
    from v_express_amd import DDIMScheduler, DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(**D.KWARGS)           # inference_v2.yaml's noise_scheduler_kwargs, unchanged
    assert (s.config.solver_order, s.config.final_sigmas_type, s.init_noise_sigma, s.order) == (2, "zero", 1.0, 1)
    ddim = DDIMScheduler(**D.KWARGS)
    assert torch.equal(DDIMScheduler.from_config(ddim.config).alphas_cumprod, ddim.alphas_cumprod)
    for src in (ddim.config, dict(D.KWARGS)):
        f = DPMSolverMultistepScheduler.from_config(src)
        f.set_timesteps(15)
        s.set_timesteps(15)
        assert torch.equal(f.sigmas, s.sigmas) and torch.equal(f.alphas_cumprod, s.alphas_cumprod)
    # the betas are DDIM's; only the last cumulative product differs (the clamp)
    assert torch.equal(s.betas, ddim.betas) and torch.equal(s.alphas_cumprod[:-1], ddim.alphas_cumprod[:-1])
    assert float(ddim.alphas_cumprod[-1]) == 0.0
    for k, v in D.KWARGS.items():
        assert getattr(ddim.config, k) == v
    x = torch.randn(3)
    assert s.scale_model_input(x, 999) is x
    for bad in (dict(solver_order=3), dict(algorithm_type="dpmsolver"), dict(solver_type="heun"),
                dict(prediction_type="epsilon"), dict(timestep_spacing="leading"), dict(use_karras_sigmas=True),
                dict(final_sigmas_type="denoise_to_zero"), dict(thresholding=True), dict(algorithm_type="sde-dpmsolver++")):
        name = next(iter(bad))
        with pytest.raises(NotImplementedError, match=name):
            make(**bad)


def test_set_timesteps_resets_the_state():
    s = make()
    s.set_timesteps(6)
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(16, generator=g)
    vs = [torch.randn(16, generator=g) for _ in range(6)]

    def run():
        x = x0.clone()
        for t, v in zip(s.timesteps.tolist(), vs):
            x = s.step(v, t, x).prev_sample
        return x
    a = run()
    s.set_timesteps(6)
    assert s.step_index is None and torch.equal(run(), a)


# ------------------------------------------------------------------------------------------------ (b) oracle loop
def test_stateful_step_in_the_oracle_single_window_loop():
    """oracle.loop.mean_overlap on one window calls `step` once per timestep for every frame: the stateful scheduler
    there against the float64 per-frame restatement."""
    from oracle import loop as OL
    F_, cf, co, _ = cases.PIPELINE_CASES["single_F8_c8o2"]
    n = 6
    windows = OL.uniform_windows(F_, cf, co)
    assert len(windows) == 1
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(1, 4, F_, 8, 8, generator=g)
    wts = torch.randn(2, 4, 1, 8, 8, generator=g) * 0.3

    def unet_fn(x, t, e, k):                    # a smooth, input-dependent stand-in for the UNet
        return torch.tanh(x) * (0.5 + t / 2000.0) + wts
    s = make()
    s.set_timesteps(n)

    class Stepper:
        def step(self, v, t, x):
            return s.step(v, t, x).prev_sample
    got = OL.mean_overlap(unet_fn, lat, s.timesteps.tolist(), Stepper(), windows, cases.GUIDANCE,
                          torch.zeros(2, 1, F_, 8, 8), torch.zeros(2, F_, 1, 8))
    ref = restated_loop(lambda x, t, e, k, rows: unet_fn(x, t, e, k), lat, windows, cases.GUIDANCE,
                        torch.zeros(2, 1, F_, 8, 8), torch.zeros(2, F_, 1, 8), n, "dpm")
    r = rel_l2(got, ref)
    print(f"[stateful step, single window, {n} steps] relL2 vs float64 = {r:.3g}")
    assert torch.isfinite(got).all() and r <= 1e-5


# ------------------------------------------------------------------------------------------------ (c) convergence
def _analytic_runs(n, xT, sampler, solver_order=2):
    """Data N(0, 0.6^2) per element: the ideal v-prediction is linear in x and the probability-flow ODE maps x_T to
    0.6 x_T.  Returns the sampler's final latents (float64)."""
    from v_express_amd import DDIMScheduler
    abar = D.alphas_cumprod(clamp=False)
    s2 = 0.36

    def vhat(x, t):
        a, sg = math.sqrt(abar[t]), math.sqrt(1.0 - abar[t])
        return a * sg * (1.0 - s2) / (a * a * s2 + sg * sg) * x
    x = xT.clone()
    if sampler == "ddim":
        d = DDIMScheduler(**D.KWARGS)
        d.set_timesteps(n)
        for t in d.timesteps.tolist():
            x = d.step(vhat(x, t), t, x).prev_sample
    else:
        p = make(solver_order=solver_order)
        p.set_timesteps(n)
        for t in p.timesteps.tolist():
            x = p.step(vhat(x, t), t, x).prev_sample
    return x


def test_convergence_on_the_analytic_model():
    xT = torch.from_numpy(np.random.default_rng(0).standard_normal(10000))
    finals = {n: (_analytic_runs(n, xT, "ddim"), _analytic_runs(n, xT, "dpm", 1), _analytic_runs(n, xT, "dpm", 2))
              for n in (8, 10, 12, 15, 20, 25)}
    res = {n: tuple(rel_l2(x, 0.6 * xT) for x in xs) for n, xs in finals.items()}
    for n, (dd, d1, d2) in res.items():
        print(f"[analytic model] {n:2d} steps: DDIM {dd:.4f}  DPM++ 1st order {d1:.4f}  DPM++ 2M {d2:.4f}")
    assert res[15][2] <= res[25][0]                                 # 2M at 15 steps ends as close as DDIM at 25
    for n in (8, 10, 12, 20, 25):
        assert res[n][2] < res[n][0]
    # 1000 % n == 0: first order is DDIM's update but for the 2^-24 clamp, which leaves alpha = 2.4e-4 in the first x0
    # (DDIM: 0); times c_0 = 0.034 that is 8e-6 of the first update (measured 1.3e-5 / 6.0e-6 / 4.5e-6 in the end)
    for n in (10, 20, 25):
        d = rel_l2(finals[n][1], finals[n][0])
        print(f"[analytic model] {n:2d} steps: first-order DPM++ vs DDIM relL2 {d:.3g}")
        assert d <= 2e-5


# ------------------------------------------------------------------------------------------------ (d) __call__
def _call(scheduler, inp, F_, steps, cf, co):
    """On a pipeline of its own."""
    import loop_worker
    return call_pipeline(loop_worker.build_pipeline("cpu"), scheduler, inp, F_, steps, cf, co)


def test_pipeline_call_with_dpm_solver_vs_restated_oracle_loop(emulated):
    """__call__ with DPM++ 2M (5 steps, reflected last window [8, 9, 10, 9]) under emulated kernels against the per-frame
    restated loop over the oracle UNet; the DDIM clip of the same inputs differs from it (the update really changed)."""
    from oracle import loop as OL
    F_, cf, co, _ = cases.PIPELINE_CASES["reflected_F11_c4o2"]
    steps = 5
    inp = inputs(F_)
    calls = []
    orig = emulated.overlap_multistep_step

    def counted(*a):
        calls.append(a[-1])
        return orig(*a)
    emulated.overlap_multistep_step = counted
    got = _call(make(), inp, F_, steps, cf, co)
    assert len(calls) == steps and calls[-1][2:] == (0.0, -1.0, 0.0)
    with torch.no_grad():
        ref = restated_loop(oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), cases.GUIDANCE,
                            inp["kps_features"], inp["audio_embeddings"], steps, "dpm")
    from v_express_amd import DDIMScheduler
    ddim = _call(DDIMScheduler(**D.KWARGS), inp, F_, steps, cf, co)
    r, rd = rel_l2(got, ref), rel_l2(ddim, ref)
    print(f"[__call__ DPM++ 2M, emulated kernels, reflected_F11_c4o2, {steps} steps] relL2 vs restated oracle loop "
          f"{r:.4g} (the DDIM clip: {rd:.4g})")
    assert torch.isfinite(got).all() and r <= 5e-2 and rd > 4 * r


def test_unsupported_scheduler_fails_before_any_kernel(emulated, monkeypatch):
    import loop_worker

    class Other:
        init_noise_sigma = 1.0

        def set_timesteps(self, n):
            self.timesteps = torch.arange(999, 0, -100)

    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "overlap_ddim_step", "overlap_multistep_step", "ncfhw_to_nhwc",
                 "groupnorm", "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)
    pipe = loop_worker.build_pipeline("cpu")
    inp = inputs(4)
    with pytest.raises(TypeError, match="DDIMScheduler or .*DPMSolverMultistepScheduler"):
        call_pipeline(pipe, Other(), inp, 4, 2, 4, 2)
    with pytest.raises(TypeError, match="DPMSolverMultistepScheduler"):
        pipe.denoise(inp["latents"].clone(), None, None, [999], [[0, 1, 2, 3]], cases.GUIDANCE)


def test_two_gloo_ranks_with_dpm_solver_are_bit_identical_to_one_process(emulated):
    """Every rank applies the update to the same gathered predictions and keeps the same x0 history: the clip of two gloo
    ranks (the windows of F = 14, 8 / 2 split over them) is bit-identical to one process, on both ranks."""
    import dpm_worker
    ref = dpm_worker.run()
    for rank, lat in enumerate(spawn_gloo(dpm_worker.main, 2, timeout=600)):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))
