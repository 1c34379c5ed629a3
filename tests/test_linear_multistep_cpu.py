"""Euler, LMS and PNDM sampling on the host: the three schedulers' collapsed coefficients (the one update form of
`vx_overlap_linear_step`) against the float64 restatements of diffusers' own update forms
(tests/linear_multistep_restated.py), convergence on the analytic model, every option that is not built, VExpressPipeline
with each scheduler under emulated kernels (one process and two gloo ranks), the third C ABI header
(include/vexpress_hip_samplers.h) with its binding, and the argument checks of ops.overlap_linear_step."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cases
import dpm_restated as D
import linear_multistep_restated as LM
import linear_multistep_worker as LW
from loop_worker import call_pipeline, inputs, oracle_unet, rel_l2, small_pipe, spawn_gloo  # noqa: F401

make = LW.scheduler


@pytest.fixture()
def emulated(monkeypatch):
    return LW.emulate(monkeypatch)


def apply(cf, x, v, H, saved):
    """One update in the kernel's form on float64 tensors: (out, saved'), H (three slots) updated in place."""
    b = saved if cf.saved_mode == 2 else x
    out = cf.k_x * b + cf.k_v * v
    for slot, c in ((cf.h1, cf.c_1), (cf.h2, cf.c_2), (cf.h3, cf.c_3)):
        if slot >= 0:
            out = out + c * H[slot]
    if cf.saved_mode == 1:
        saved = x
    if cf.h_write >= 0:
        H[cf.h_write] = cf.p_x * x + cf.p_v * v
    return out, saved


def alpha(sig):
    return 1.0 / math.sqrt(1.0 + sig * sig)


# ------------------------------------------------------------------------------------------------ (a) coefficients
@pytest.mark.parametrize("n", [10, 25])
@pytest.mark.parametrize("kind,lms_order", [("euler", None), ("lms", 4), ("lms", 2)])
def test_sigma_schedulers_collapse_to_the_restated_ve_update(kind, lms_order, n):
    """k_x x + k_v v + sum c_j H_j == a' X' with X' diffusers' update in the VE frame, x = a X, through a whole run on the
    float32 sigma table (sigma_0 = 4096 included); the history entry written is the derivative eps."""
    s = make(kind, **({} if lms_order is None else dict(lms_order=lms_order)))
    s.set_timesteps(n)
    assert s.timesteps.tolist() == [float(t) for t in D.timesteps(n)] and len(s.sigmas) == n + 1
    assert float(s.alphas_cumprod[-1]) == 2.0 ** -24 and float(s.sigmas[-1]) == 0.0
    assert float(s.init_noise_sigma) == float(s.sigmas[0]) == pytest.approx(math.sqrt(2.0 ** 24 - 1), rel=1e-7)
    sg = [float(v) for v in s.sigmas]
    g = torch.Generator().manual_seed(0)
    X = torch.randn(64, generator=g, dtype=torch.float64) * sg[0]
    ds, H, worst = [], [None] * 3, 0.0
    for i in range(n):
        v = torch.randn(64, generator=g, dtype=torch.float64)
        cf = s.linear_coefficients(i)
        assert all(isinstance(c, float) and math.isfinite(c) for c in cf[5:]) and cf.saved_mode == 0
        if kind == "euler":
            ref, d = LM.euler_update_ve(sg, i, X, v), None
            assert cf[:4] == (-1, -1, -1, -1)
        else:
            ref, d = LM.lms_update_ve(sg, i, lms_order, X, v, ds)
            ds = (ds + [d])[-lms_order:]
            assert s.order_at(i) == LM.lms_order_at(i, 0, lms_order) == 1 + sum(h >= 0 for h in cf[:3])
        got, _ = apply(cf, alpha(sg[i]) * X, v, H, None)
        worst = max(worst, rel_l2(got, alpha(sg[i + 1]) * ref))
        if d is not None:
            worst = max(worst, rel_l2(H[cf.h_write], d))
        X = ref
    print(f"[{kind} order {lms_order}, {n} steps] collapsed coefficients vs the restated VE update: relL2 {worst:.3g}")
    assert worst <= 1e-12
    last = s.linear_coefficients(n - 1)
    if kind == "euler":                                          # a step to sigma = 0 returns x0 = a x - s v
        a = alpha(sg[n - 1])
        assert last.k_x == pytest.approx(a, rel=1e-15) and last.k_v == pytest.approx(-sg[n - 1] * a, rel=1e-15)


@pytest.mark.parametrize("n", [10, 25])
@pytest.mark.parametrize("zero_snr", [True, False])
def test_pndm_collapses_to_the_restated_plms_update(n, zero_snr):
    """Every entry of the N + 1 list against step_plms / _get_prev_sample on the scheduler's own float32 table (the plain
    table, where diffusers' form is defined everywhere, and the zero-SNR one, where the restatement takes its limit at
    a = 0)."""
    s = make("pndm", rescale_betas_zero_snr=zero_snr)
    s.set_timesteps(n)
    assert s.timesteps.tolist() == LM.pndm_timesteps(n) and len(s.timesteps) == n + 1
    abar = [float(v) for v in s.alphas_cumprod]
    assert (abar[-1] == 0.0) == zero_snr and float(s.final_alpha_cumprod) == abar[0] and s.init_noise_sigma == 1.0
    g = torch.Generator().manual_seed(1)
    x = torch.randn(64, generator=g, dtype=torch.float64)
    ets, saved_ref, H, saved, worst = [], None, [None] * 3, None, 0.0
    for k, t in enumerate(s.timesteps.tolist()):
        v = torch.randn(64, generator=g, dtype=torch.float64)
        cf = s.linear_coefficients(k)
        assert cf.saved_mode == {0: 1, 1: 2}.get(k, 0) and (cf.p_x, cf.p_v) == (0.0, 1.0)
        assert sum(h >= 0 for h in cf[:3]) == {0: 0, 1: 1, 2: 1, 3: 2}.get(k, 3) and (cf.h_write == -1) == (k == 1)
        ref, ets, saved_ref = LM.pndm_update(abar, abar[0], n, k, t, x, v, ets, saved_ref)
        got, saved = apply(cf, x, v, H, saved)
        worst = max(worst, rel_l2(got, ref))
        x = ref
    print(f"[pndm, N = {n}, zero SNR {zero_snr}] collapsed coefficients vs step_plms: relL2 {worst:.3g}")
    assert worst <= 1e-12


def test_pndm_transfer_equals_the_diffusers_form_near_zero_alpha():
    """The rotation (al' al + s' s) b + (s' al - al' s) vc against _get_prev_sample at a = 2^-24 and over the table."""
    s = make("pndm")
    s.set_timesteps(25)
    g = torch.Generator().manual_seed(2)
    b, vc = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(2))
    abar = [float(v) for v in s.alphas_cumprod]
    for a, ap in [(2.0 ** -24, abar[959]), (abar[959], abar[919]), (abar[39], abar[0]), (abar[500], abar[460])]:
        al, sa, al1, s1 = math.sqrt(a), math.sqrt(1 - a), math.sqrt(ap), math.sqrt(1 - ap)
        assert rel_l2((al1 * al + s1 * sa) * b + (s1 * al - al1 * sa) * vc, LM.pndm_prev_sample(a, ap, b, vc)) <= 1e-11


@pytest.mark.parametrize("n", [5, 25])
def test_pndm_timestep_list(n):
    s = make("pndm")
    s.set_timesteps(n)
    tr = D.timesteps(n)
    assert s.timesteps.tolist() == [tr[0], tr[1]] + tr[1:] and len(s.timesteps) == n + 1
    if n == 5:
        assert s.timesteps.tolist() == [999, 799, 799, 599, 399, 199]
    # the level of every entry: noise_coefficients(j) is timesteps[j]'s, the last one abar[0]'s
    for j, t in enumerate(s.timesteps.tolist()):
        a, sd = s.noise_coefficients(j)
        assert a == pytest.approx(math.sqrt(float(s.alphas_cumprod[t])), rel=1e-15) and a * a + sd * sd == pytest.approx(1)
    assert s.noise_coefficients(n + 1)[0] == pytest.approx(math.sqrt(float(s.alphas_cumprod[0])), rel=1e-15)


def test_pndm_first_entries_are_finite_on_the_zero_snr_table():
    s = make("pndm")
    s.set_timesteps(10)
    assert float(s.alphas_cumprod[999]) == 0.0                    # no clamp
    for k in (0, 1):
        cf = s.linear_coefficients(k)
        assert all(math.isfinite(c) for c in cf[5:])
    a1 = float(s.alphas_cumprod[899])
    cf = s.linear_coefficients(0)                                 # from pure noise: x' = s' x - al' v
    assert cf.k_x == pytest.approx(math.sqrt(1 - a1), rel=1e-15) and cf.k_v == pytest.approx(-math.sqrt(a1), rel=1e-15)


@pytest.mark.parametrize("n", [10, 25])
def test_lms_integrals_vs_quad(n):
    from scipy.integrate import quad
    s = make("lms")
    s.set_timesteps(n)
    sg = [float(v) for v in s.sigmas]
    worst = 0.0
    for i in range(n):
        o = s.order_at(i)
        L = s.lms_coefficients(i)
        assert len(L) == o
        assert sum(L) == pytest.approx(sg[i + 1] - sg[i], rel=1e-12)         # the basis polynomials sum to 1
        for j in range(o):
            def basis(tau):
                prod = 1.0
                for k in range(o):
                    if k != j:
                        prod *= (tau - sg[i - k]) / (sg[i - j] - sg[i - k])
                return prod
            ref = quad(basis, sg[i], sg[i + 1], epsrel=1e-12, epsabs=0.0)[0]
            worst = max(worst, abs(L[j] - ref) / max(abs(ref), abs(sg[i + 1] - sg[i])))
            assert L[j] == pytest.approx(LM.lms_weights(sg, i, o)[j], rel=1e-10, abs=1e-12 * abs(sg[i + 1] - sg[i]))
    print(f"[lms integrals, {n} steps] max |L_j - quad| relative to the step: {worst:.3g}")
    assert worst <= 1e-9
    # a run that starts later (strength < 1) starts at first order, its history empty
    assert s.order_at(3, begin_index=3) == 1 and s.order_at(5, begin_index=3) == 3
    cf = s.linear_coefficients(4, begin_index=3)
    assert (cf.h1, cf.h2, cf.h3, cf.h_write) == (0, -1, -1, 1)


@pytest.mark.parametrize("n", [10, 25])
def test_first_order_lms_is_euler_is_first_order_dpm_solver(n):
    from v_express_amd import DPMSolverMultistepScheduler
    e, l1 = make("euler"), make("lms", lms_order=1)
    dpm = DPMSolverMultistepScheduler(**{**D.KWARGS, "solver_order": 1})
    for s in (e, l1, dpm):
        s.set_timesteps(n)
    assert torch.equal(e.sigmas, dpm.sigmas) and torch.equal(e.sigmas, l1.sigmas)
    for i in range(n):
        ce, cl = e.linear_coefficients(i), l1.linear_coefficients(i)
        assert cl[:5] == (-1, -1, -1, -1, 0) and cl.c_1 == cl.c_2 == cl.c_3 == 0.0
        assert cl.k_x == pytest.approx(ce.k_x, rel=1e-12, abs=1e-15) and cl.k_v == pytest.approx(ce.k_v, rel=1e-12)
        # DPM-Solver++ first order: x' = c_x x - c_0 (a x - s v) = (c_x - c_0 a) x + c_0 s v; c_x - c_0 a cancels at the
        # first step (a = 2.4e-4 against c_x ~ 1e-3), hence the absolute term
        a, sd, c_x, c_0, c_1 = dpm.multistep_coefficients(i)
        assert c_1 == 0.0
        assert ce.k_x == pytest.approx(c_x - c_0 * a, rel=1e-10, abs=1e-13)
        assert ce.k_v == pytest.approx(c_0 * sd, rel=1e-10, abs=1e-13)


# ------------------------------------------------------------------------------------------------ (b) step()
@pytest.mark.parametrize("kind", LM.SAMPLERS)
def test_stateful_step_matches_the_coefficients_and_resets(kind):
    """`step()` (the scheduler's own frame) against the kernel-form coefficients through a 6-step run; set_timesteps
    resets the state."""
    s = make(kind)
    s.set_timesteps(6)
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(32, generator=g, dtype=torch.float64)
    vs = [torch.randn(32, generator=g, dtype=torch.float64) for _ in range(len(s.timesteps))]

    def run():
        x = x0 * float(s.init_noise_sigma)
        for t, v in zip(s.timesteps.tolist(), vs):
            s.scale_model_input(x, t)                            # (as a pipeline calls it before the UNet)
            x = s.step(v, t, x).prev_sample
        return x
    a = run()
    s.set_timesteps(6)
    assert torch.equal(run(), a)
    x, H, saved = x0.clone(), [None] * 3, None                   # the VP frame: x0 * sigma_0 / sqrt(1 + sigma_0^2)
    if kind != "pndm":
        x = x * float(s.init_noise_sigma) / s.frame_scale(0)
    for i, v in enumerate(vs):
        x, saved = apply(s.linear_coefficients(i), x, v, H, saved)
    assert rel_l2(x, a) <= 1e-11                                 # (the final sigma is 0: both frames agree there)


# ------------------------------------------------------------------------------------------------ (c) convergence
def _analytic_final_std(kind, n, xT):
    """Data N(0, 0.6^2) per element with the exact v-prediction (tests/test_dpm_solver_cpu.py's model): the std of the
    sampler's final latents."""
    from v_express_amd import DDIMScheduler
    abar = D.alphas_cumprod(clamp=False)
    s2 = 0.36

    def vhat(x, t):
        a, sg = math.sqrt(abar[t]), math.sqrt(1.0 - abar[t])
        return a * sg * (1.0 - s2) / (a * a * s2 + sg * sg) * x
    s = DDIMScheduler(**D.KWARGS) if kind == "ddim" else make(kind)
    s.set_timesteps(n)
    x = xT.clone() * float(s.init_noise_sigma)
    for t in s.timesteps.tolist():
        x = s.step(vhat(s.scale_model_input(x, t), int(t)), t, x).prev_sample
    return float(x.std())


def test_convergence_on_the_analytic_model():
    """The probability-flow answer is a final std of 0.6 at level 1 (Euler, LMS, DDIM) and sqrt(0.36 abar_0 + 1 - abar_0)
    = 0.60045 at PNDM's own end level abar[0].  Inequalities only."""
    xT = torch.from_numpy(np.random.default_rng(0).standard_normal(10000))
    a0 = D.alphas_cumprod(clamp=False)[0]
    exact = dict(euler=0.6, lms=0.6, ddim=0.6, pndm=math.sqrt(0.36 * a0 + 1.0 - a0))
    err = {}
    for n in (10, 20, 25, 50):
        std = {k: _analytic_final_std(k, n, xT) for k in ("ddim",) + LM.SAMPLERS}
        err[n] = {k: abs(v - exact[k]) for k, v in std.items()}
        print(f"[analytic model] {n:2d} steps: final std DDIM {std['ddim']:.4f}  Euler {std['euler']:.4f}  "
              f"LMS(4) {std['lms']:.4f}  PNDM {std['pndm']:.4f} (exact 0.6; PNDM {exact['pndm']:.5f})")
        assert err[n]["lms"] < err[n]["euler"] and err[n]["pndm"] < err[n]["euler"]
        assert std["euler"] == pytest.approx(std["ddim"], abs=1e-4)          # Euler is DDIM up to the 2^-24 clamp
    assert err[10]["lms"] < err[50]["euler"]


# ------------------------------------------------------------------------------------------------ (d) options
def test_options_and_construction():
    from v_express_amd import DDIMScheduler, EulerDiscreteScheduler, LMSDiscreteScheduler, PNDMScheduler
    ddim = DDIMScheduler(**D.KWARGS)
    for kind, cls in (("euler", EulerDiscreteScheduler), ("lms", LMSDiscreteScheduler), ("pndm", PNDMScheduler)):
        extra = dict(skip_prk_steps=True) if kind == "pndm" else {}
        s = cls(**D.KWARGS, **extra)                             # inference_v2.yaml's noise_scheduler_kwargs, unchanged
        assert s.order == 1
        for src in (ddim.config, dict(D.KWARGS)):                # clip_sample, set_alpha_to_one, ... of DDIM: ignored
            f = cls.from_config(src, **extra)
            f.set_timesteps(15)
            s.set_timesteps(15)
            assert torch.equal(f.timesteps, s.timesteps) and torch.equal(f.alphas_cumprod, s.alphas_cumprod)
        assert torch.equal(s.betas, ddim.betas)
        x, z = torch.randn(2, 3), torch.randn(2, 3)
        t = s.timesteps[3]
        if kind == "pndm":
            assert s.scale_model_input(x, t) is x
            assert torch.allclose(s.add_noise(x, z, t), ddim.add_noise(x, z, t))
        else:
            assert torch.allclose(s.add_noise(x, z, t), x + float(s.sigmas[3]) * z)
            a, sd = s.noise_coefficients(3)
            assert sd / a == pytest.approx(float(s.sigmas[3]), rel=1e-12) and s.frame_scale(3) == pytest.approx(1 / a)
            assert s.noise_coefficients(15) == (1.0, 0.0)
    assert LMSDiscreteScheduler(**D.KWARGS).config.lms_order == 4
    assert float(PNDMScheduler(**D.KWARGS, skip_prk_steps=True, set_alpha_to_one=True).final_alpha_cumprod) == 1.0
    common = [dict(prediction_type="epsilon"), dict(timestep_spacing="leading"), dict(trained_betas=[0.1, 0.2]),
              dict(beta_schedule="squaredcos_cap_v2")]
    bad = {"euler": common + [dict(interpolation_type="log_linear"), dict(use_karras_sigmas=True),
                              dict(timestep_type="continuous"), dict(final_sigmas_type="sigma_min"), dict(sigma_min=0.1),
                              dict(sigma_max=10.0)],
           "lms": common + [dict(use_karras_sigmas=True), dict(lms_order=5), dict(lms_order=0)],
           "pndm": common + [dict(skip_prk_steps=False)]}
    for kind, opts in bad.items():
        for opt in opts:
            with pytest.raises(NotImplementedError, match=next(iter(opt))):
                make(kind, **opt)
    with pytest.raises(NotImplementedError, match="skip_prk_steps"):
        PNDMScheduler(**D.KWARGS)                                # diffusers' default: the Runge-Kutta warm-up
    e = make("euler")
    e.set_timesteps(4)
    with pytest.raises(NotImplementedError, match="s_churn"):
        e.step(torch.zeros(2), e.timesteps[0], torch.zeros(2), s_churn=0.5)
    p = make("pndm")
    p.set_timesteps(4)
    with pytest.raises(NotImplementedError, match="begin_index"):
        p.linear_coefficients(2, begin_index=1)


def test_unbuilt_pipeline_routes_fail_before_any_kernel(emulated, small_pipe, monkeypatch):
    """PNDM with strength < 1 or an init clip (`known`), and eta != 0 with any of the three."""
    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "known_blend", "overlap_ddim_step", "overlap_linear_step",
                 "ncfhw_to_nhwc", "groupnorm", "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)
    inp = inputs(4)
    for kind in LM.SAMPLERS:
        with pytest.raises(NotImplementedError, match="eta"):
            call_pipeline(small_pipe, make(kind), inp, 4, 2, 4, 2, eta=0.5)
    init = torch.randn(1, 4, 4, 8, 8)
    with pytest.raises(NotImplementedError, match="strength"):
        call_pipeline(small_pipe, make("pndm"), inp, 4, 4, 4, 2, strength=0.5)
    with pytest.raises(NotImplementedError, match="init"):
        call_pipeline(small_pipe, make("pndm"), inp, 4, 4, 4, 2, init_latents=init)
    p = make("pndm")
    p.set_timesteps(4)
    small_pipe.scheduler = p
    lat = inp["latents"].clone()
    with pytest.raises(NotImplementedError, match="begin_index"):
        small_pipe.denoise(lat, None, None, p.timesteps.tolist()[2:], [[0, 1, 2, 3]], cases.GUIDANCE)
    with pytest.raises(NotImplementedError, match="known"):
        small_pipe.denoise(lat, None, None, p.timesteps.tolist(), [[0, 1, 2, 3]], cases.GUIDANCE,
                           known=(init, torch.randn_like(init), None))


def test_unsupported_scheduler_message_lists_the_new_classes(small_pipe):
    class Other:
        pass
    small_pipe.scheduler = Other()
    with pytest.raises(TypeError, match="DDIMScheduler or .*DPMSolverMultistepScheduler.*EulerDiscreteScheduler, "
                                        "LMSDiscreteScheduler or PNDMScheduler, not Other"):
        small_pipe._sampler()


# ------------------------------------------------------------------------------------------------ (e) __call__
def _call(scheduler, inp, F_, steps, cf, co, **kw):
    """On a pipeline of its own."""
    import loop_worker
    return call_pipeline(loop_worker.build_pipeline("cpu"), scheduler, inp, F_, steps, cf, co, **kw)


@pytest.mark.parametrize("kind", LM.SAMPLERS)
def test_pipeline_call_vs_restated_oracle_loop(emulated, kind):
    """__call__ with each scheduler (5 steps, reflected last window [8, 9, 10, 9]) under emulated kernels against the
    per-frame restated loop over the oracle UNet; one overlap_linear_step per entry of the timestep list; the DDIM clip of
    the same inputs differs from LMS's and PNDM's (the update really changed).  The tolerance is the DPM-Solver++ test's."""
    from oracle import loop as OL
    F_, cf, co, _ = cases.PIPELINE_CASES["reflected_F11_c4o2"]
    steps = 5
    inp = inputs(F_)
    calls = []
    orig = emulated.overlap_linear_step

    def counted(*a):
        calls.append(a[-1])
        return orig(*a)
    emulated.overlap_linear_step = counted
    seen = []
    got = _call(make(kind), inp, F_, steps, cf, co, callback=lambda i, t, lat: seen.append((i, t)))
    entries = steps + (1 if kind == "pndm" else 0)
    assert len(calls) == entries and [i for i, _ in seen] == list(range(entries))
    with torch.no_grad():
        ref = LM.restated_linear_loop(oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), cases.GUIDANCE,
                                      inp["kps_features"], inp["audio_embeddings"], steps, kind)
    r = rel_l2(got, ref)
    print(f"[__call__ {kind}, emulated kernels, reflected_F11_c4o2, {steps} steps] relL2 vs restated oracle loop {r:.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2
    if kind != "euler":
        from v_express_amd import DDIMScheduler
        rd = rel_l2(_call(DDIMScheduler(**D.KWARGS), inp, F_, steps, cf, co), ref)
        print(f"    the DDIM clip: {rd:.4g}")
        assert rd > 4 * r


@pytest.mark.parametrize("kind", ["euler", "lms"])
def test_init_video_sampling_with_the_sigma_schedulers(emulated, kind):
    """strength < 1 with an init clip: the run starts at begin_index with an empty history (first order there) and ends
    finite; LMS's first update of the run names no history slot."""
    F_, cf, co, _ = cases.PIPELINE_CASES["reflected_F11_c4o2"]
    inp = inputs(F_)
    calls = []
    orig = emulated.overlap_linear_step

    def counted(*a):
        calls.append(a[-1])
        return orig(*a)
    emulated.overlap_linear_step = counted
    init = torch.randn(1, 4, F_, 8, 8, generator=torch.Generator().manual_seed(9)) * 0.5
    got = _call(make(kind), inp, F_, 6, cf, co, strength=0.5, init_latents=init)
    assert len(calls) == 3 and calls[0][:3] == (-1, -1, -1) and torch.isfinite(got).all()
    if kind == "lms":
        assert [sum(h >= 0 for h in c[:3]) for c in calls] == [0, 1, 2]


@pytest.mark.parametrize("kind", LM.SAMPLERS)
def test_two_gloo_ranks_are_bit_identical_to_one_process(emulated, kind):
    """Every rank applies the update to the same gathered predictions and keeps the same history: the clip of two gloo
    ranks (the windows of F = 14, 8 / 2 split over them) is bit-identical to one process, on both ranks."""
    ref = LW.run(kind)
    for rank, lat in enumerate(spawn_gloo(LW.main, 2, kind, timeout=600)):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))


# ------------------------------------------------------------------------------------------------ (f) the third header
def test_third_header_parses_and_is_disjoint_from_the_others():
    from v_express_amd import abi
    s = abi.samplers_header()
    assert s is abi.samplers_header() and s.version == 1 and not s.enums and not s.structs
    assert list(s.functions) == ["vx_samplers_abi_version", "vx_overlap_linear_step"]
    assert not set(s.functions) & (set(abi.header().functions) | set(abi.guidance_header().functions))
    i32, vp, fl = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float
    assert s.functions["vx_samplers_abi_version"] == (i32, [])
    restype, params = s.functions["vx_overlap_linear_step"]
    assert restype is i32
    assert [t for _, t in params] == [vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, i32, vp] + [i32] * 4 + [vp, i32] + \
        [fl] * 7 + [vp]
    assert [n for n, _ in params][11:18] == ["history", "h1", "h2", "h3", "h_write", "saved", "saved_mode"]
    text = open(abi.SAMPLERS_HEADER).read()
    with pytest.raises(ImportError, match="VX_ABI_VERSION"):
        abi.parse(text, "samplers.h")
    assert abi.parse(text, "samplers.h", "VX_SAMPLERS_ABI_VERSION").functions == s.functions


def test_third_header_is_bound_on_both_libraries_and_stamped():
    import os
    import subprocess
    import sys
    from v_express_amd import abi, lib
    functions = abi.samplers_header().functions
    assert not set(functions) & set(lib.declared_symbols())          # declared_symbols keeps meaning the first header
    for so in (lib.lib, lib.lib_f16()):
        for n, (restype, params) in functions.items():
            fn = so.__dict__[n]                                      # __dict__: the function objects _load touched
            assert fn.restype is restype and list(fn.argtypes) == [t for _, t in params], n
        assert so.vx_samplers_abi_version() == abi.samplers_header().version == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "lib_id.py")], capture_output=True, text=True)
    assert out.stdout.strip() == lib.source_id()
    assert "vexpress_hip_samplers.h" in open(os.path.join(root, "tools", "lib_id.py")).read()
    mk = open(os.path.join(lib.CSRC, "Makefile")).read()
    assert "vexpress_hip_samplers.h" in mk and "vx_sampler.hip" in mk


# ------------------------------------------------------------------------------------------------ (g) argument checks
def test_overlap_linear_step_argument_checks(monkeypatch):
    """Every check of the wrapper fails before the library is asked (its entry point is replaced by one that fails)."""
    from v_express_amd import lib, ops
    from v_express_amd.scheduler import LinearStep

    def no_launch(*a):
        raise AssertionError("the library was called")
    for so in (lib.lib, lib.lib_f16()):
        monkeypatch.setattr(so, "vx_overlap_linear_step", no_launch)
    monkeypatch.setattr(ops, "_stream", lambda: None)                # (no device in this suite to ask for its stream)
    C, F_, h, w, nW, f, T = 4, 6, 4, 4, 2, 4, 2
    good = dict(latents=torch.zeros(1, C, F_, h, w), preds=torch.zeros(nW, C, f, h * w),
                terms=torch.zeros(3, T, 2, dtype=torch.int32), frame_ids=torch.arange(3, dtype=torch.int32),
                counts=torch.ones(3), history=torch.zeros(3, C, F_, h, w), saved=torch.zeros(1, C, F_, h, w),
                coef=LinearStep(0, 1, -1, 2, 1, 1.0, 0.5, 0.1, 0.2, 0.0, 0.3, 0.4))

    def call(**kw):
        a = {**good, **kw}
        ops.overlap_linear_step(*(a[k] for k in ("latents", "preds", "terms", "frame_ids", "counts", "history", "saved",
                                                 "coef")))
    with pytest.raises(AssertionError, match="the library was called"):
        call()                                                       # the good arguments reach the library
    cf = good["coef"]
    for err, match, kw in [
            (TypeError, "latents", dict(latents=good["latents"].double())),
            (TypeError, "preds", dict(preds=good["preds"].transpose(2, 3))),
            (TypeError, "terms", dict(terms=good["terms"].long())),
            (TypeError, "frame_ids", dict(frame_ids=good["frame_ids"].long())),
            (TypeError, "counts", dict(counts=good["counts"].double())),
            (ValueError, "latents must be", dict(latents=torch.zeros(C, F_, h, w))),
            (ValueError, "latents must be", dict(preds=torch.zeros(nW, C + 1, f, h * w))),
            (ValueError, "multiple of 4", dict(preds=torch.zeros(nW, C, f, h * w + 1))),
            (ValueError, "multiple of 4", dict(latents=torch.zeros(1, C, F_, 3, 3), preds=torch.zeros(nW, C, f, 9),
                                               history=None, saved=None,
                                               coef=cf._replace(h1=-1, h2=-1, h_write=-1, saved_mode=0))),
            (ValueError, "terms must be", dict(terms=torch.zeros(2, T, 2, dtype=torch.int32))),
            (ValueError, "terms must be", dict(counts=torch.ones(4))),
            (ValueError, "h2", dict(coef=cf._replace(h2=3))),
            (ValueError, "h_write", dict(coef=cf._replace(h_write=-2))),
            (ValueError, "h1", dict(coef=cf._replace(h1=1.0))),
            (ValueError, "saved_mode", dict(coef=cf._replace(saved_mode=3))),
            (ValueError, "history is None", dict(history=None)),
            (ValueError, "saved is None", dict(saved=None)),
            (TypeError, "history", dict(history=torch.zeros(2, C, F_, h, w))),
            (TypeError, "history", dict(history=good["history"].double())),
            (TypeError, "saved", dict(saved=torch.zeros(1, C, F_ + 1, h, w))),
            (ValueError, "finite", dict(coef=cf._replace(c_1=float("nan")))),
            (ValueError, "finite", dict(coef=cf._replace(k_x=float("inf"))))]:
        with pytest.raises(err, match=match):
            call(**kw)
    # buffers the coefficients do not name may be absent
    with pytest.raises(AssertionError, match="the library was called"):
        call(history=None, saved=None, coef=cf._replace(h1=-1, h2=-1, h_write=-1, saved_mode=0))
