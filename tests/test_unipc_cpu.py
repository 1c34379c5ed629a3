"""UniPC sampling on the host: v_express_amd.UniPCMultistepScheduler's folded coefficients (the update form of
`vx_overlap_unipc_step`) against the float64 restatement of diffusers' own form (tests/unipc_restated.py), polynomial
exactness of the predictor and the corrector on an uneven grid, the corrector-off identity with DPM-Solver++, the analytic
model, every option that is not built, VExpressPipeline with the scheduler under emulated kernels (one process, init-video
sampling, two gloo ranks), the fourth C ABI header (include/vexpress_hip_solvers.h) with its binding, and the argument
checks of ops.overlap_unipc_step."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cases
import dpm_restated as D
import init_video_restated as R
import unipc_restated as U
import unipc_worker as UW
from loop_worker import call_pipeline, inputs, oracle_unet, rel_l2, small_pipe, spawn_gloo  # noqa: F401

make = UW.scheduler


@pytest.fixture()
def emulated(monkeypatch):
    return UW.emulate(monkeypatch)


def apply(cf, x, v, H, saved):
    """One update in the kernel's form on float64 tensors: (out, xc, m); H (three slots) is not changed."""
    m = cf.a_i * x - cf.s_i * v
    xc = x
    if cf.use_c:
        xc = cf.q_s * saved + cf.q_m * m
        for slot, q in ((cf.h1, cf.q_1), (cf.h2, cf.q_2), (cf.h3, cf.q_3)):
            if slot >= 0:
                xc = xc + q * H[slot]
    out = cf.k_x * xc + cf.k_m * m
    for slot, k in ((cf.h1, cf.k_1), (cf.h2, cf.k_2)):
        if slot >= 0:
            out = out + k * H[slot]
    return out, xc, m


# ------------------------------------------------------------------------------------------------ (a) coefficients
@pytest.mark.parametrize("final", ["zero", "sigma_min"])
@pytest.mark.parametrize("begin", [0, 2])
@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
@pytest.mark.parametrize("solver_order", [1, 2, 3])
@pytest.mark.parametrize("n", [5, 10, 25])
def test_folded_coefficients_equal_the_restated_step(n, solver_order, solver_type, begin, final):
    """The folded coefficients applied in float64 through a whole run on the float32 sigma table (sigma_0 = 4096 included)
    against the restated step with its D1 list and linear solve: the same arithmetic in another association, 1e-10
    relative.  disable_corrector = [0, 3]: the correctors of steps 0 and 3 (at indices 1 and 4) do not run."""
    off = [0, 3]
    s = make(solver_order=solver_order, solver_type=solver_type, final_sigmas_type=final, disable_corrector=off)
    s.set_timesteps(n)
    assert s.timesteps.tolist() == D.timesteps(n) and len(s.sigmas) == n + 1 and s.sigmas.dtype == torch.float32
    sg = [float(v) for v in s.sigmas]
    g = torch.Generator().manual_seed(n)
    x = torch.randn(64, generator=g, dtype=torch.float64)
    xr, st = x.clone(), U.State()
    H, saved, worst = [None] * 3, None, 0.0
    coefs = s.loop_steps(s.timesteps.tolist()[begin:], begin)
    assert coefs[0] == "unipc" and len(coefs[1]) == n - begin
    for i, cf in zip(range(begin, n), coefs[1]):
        v = torch.randn(64, generator=g, dtype=torch.float64)
        assert cf == s.unipc_coefficients(i, begin) and type(cf).__name__ == "UniPCStep"
        assert all(isinstance(c, float) and math.isfinite(c) for c in cf[5:]) and all(isinstance(c, int) for c in cf[:5])
        p = s.solver_order_at(i, begin)
        assert p == U.order_at(n, i, begin, solver_order) == min(solver_order, n - i, i - begin + 1)
        ends_at_zero = sg[i + 1] == 0.0
        assert cf.use_c == int(i > begin and (i - 1) not in off and not ends_at_zero)
        pc = s.solver_order_at(i - 1, begin) if cf.use_c else 0
        reads = max(pc, p - 1)
        r = i - begin
        assert (cf.h1, cf.h2) == tuple((r - j) % 3 if j <= reads else -1 for j in (1, 2))
        assert cf.h3 == ((r - 3) % 3 if pc == 3 else -1) and cf.h_write == r % 3
        if ends_at_zero:                                         # m itself, whatever xc is
            assert cf[:5] == (-1, -1, -1, r % 3, 0) and cf[7:] == (0.0,) * 5 + (0.0, 1.0, 0.0, 0.0)
        out, xc, m = apply(cf, x, v, H, saved)
        xr = U.step(sg, n, i, xr, v, st, solver_order, solver_type, off)
        worst = max(worst, rel_l2(out, xr), rel_l2(m, st.ms[0]))
        if not ends_at_zero:                                     # (there the restated corrector still runs: no output reads it)
            worst = max(worst, rel_l2(xc, st.last_sample))
        H[cf.h_write], saved, x = m, xc, out
    print(f"[unipc order {solver_order} {solver_type}, {n} steps from {begin}, final {final}] folded coefficients vs the "
          f"restated step: relL2 {worst:.3g}")
    assert worst <= 1e-10


def test_begin_index_starts_with_an_empty_history():
    s = make(solver_order=3)
    s.set_timesteps(10)
    first = s.unipc_coefficients(4, begin_index=4)
    assert first[:5] == (-1, -1, -1, 0, 0) and s.solver_order_at(4, 4) == 1 and s.solver_order_at(6, 4) == 3
    assert s.unipc_coefficients(5, begin_index=4)[:5] == (0, -1, -1, 1, 1)
    assert s.unipc_coefficients(7, begin_index=4)[:5] == (2, 1, 0, 0, 1)          # the slot written is the oldest one read
    with pytest.raises(IndexError):
        s.unipc_coefficients(3, begin_index=4)
    with pytest.raises(IndexError):
        s.unipc_coefficients(10)
    with pytest.raises(RuntimeError, match="set_timesteps"):
        make().unipc_coefficients(0)


# ------------------------------------------------------------------------------------------------ (b) exactness
GRID = [3.0, 1.9, 1.4, 0.6, 0.45, 0.2, 0.11]                     # uneven in lambda = -log sigma; six steps, none to 0


def _exact_run(poly):
    """x0(lambda) = poly and the exact samples x_j of the data-prediction ODE on GRID:
    x_b = (s_b / s_a) x_a + s_b int_a^b e^lambda x0(lambda) dlambda (s = sigma alpha), by scipy.integrate.quad."""
    from scipy.integrate import quad
    lams = [-math.log(sg) for sg in GRID]

    def x0(lm):
        return sum(c * lm ** k for k, c in enumerate(poly))
    xs = [0.7]
    for a in range(len(GRID) - 1):
        sa, sb = U.alpha_sigma(GRID[a])[1], U.alpha_sigma(GRID[a + 1])[1]
        integral, err = quad(lambda lm: math.exp(lm) * x0(lm), lams[a], lams[a + 1], epsabs=0.0, epsrel=2e-14)
        assert err <= 1e-13 * max(abs(integral), 1.0)
        xs.append(sb / sa * xs[-1] + sb * integral)
    return [x0(lm) for lm in lams], xs


def _errors(poly, solver_type):
    """Per step index i of a third-order run on GRID fed the exact samples and predictions: (|xc - x_i|, |out - x_{i+1}|),
    the corrector's and the predictor's error."""
    s = make(solver_order=3, solver_type=solver_type, final_sigmas_type="sigma_min")
    s.set_timesteps(len(GRID) - 1)
    s.sigmas = torch.tensor(GRID, dtype=torch.float64)
    ms, xs = _exact_run(poly)
    errs, H = [], [None] * 3
    for i in range(len(GRID) - 1):
        cf = s.unipc_coefficients(i)
        a_i, s_i = U.alpha_sigma(GRID[i])
        x = torch.tensor([xs[i]], dtype=torch.float64)
        v = (a_i * x - ms[i]) / s_i                              # the model output whose data prediction is x0(lambda_i)
        out, xc, m = apply(cf, x, v, H, None if i == 0 else torch.tensor([xs[i - 1]], dtype=torch.float64))
        assert abs(float(m) - ms[i]) <= 1e-14
        errs.append((abs(float(xc) - xs[i]), abs(float(out) - xs[i + 1])))
        H[cf.h_write] = m
    return s, errs


@pytest.mark.parametrize("solver_type", ["bh1", "bh2"])
def test_polynomial_exactness_on_an_uneven_grid(solver_type):
    """Orders on the six-step grid: predictor 1, 2, 3, 3, 2, 1; the corrector at index i has the order of step i - 1.  The
    order-3 predictor reproduces a quadratic x0(lambda), the order-2 corrector a quadratic, the order-3 corrector a cubic,
    to 1e-12 (samples of magnitude 1); the order-2 predictor with its rho = 0.5 shortcut is NOT exact for a linear x0."""
    s, quad_err = _errors([0.3, -0.8, 0.25], solver_type)
    assert [s.solver_order_at(i) for i in range(6)] == [1, 2, 3, 3, 2, 1]
    _, cubic_err = _errors([0.3, -0.8, 0.25, -0.1], solver_type)
    _, lin_err = _errors([0.3, -0.8], solver_type)
    print(f"[unipc {solver_type}, uneven grid] quadratic x0: predictor order 3 {quad_err[2][1]:.2g} {quad_err[3][1]:.2g}, "
          f"corrector order 2 {quad_err[2][0]:.2g} {quad_err[5][0]:.2g}, order 3 {quad_err[3][0]:.2g} {quad_err[4][0]:.2g}; "
          f"cubic x0: corrector order 3 {cubic_err[3][0]:.2g} {cubic_err[4][0]:.2g}; linear x0: predictor order 2 "
          f"{lin_err[1][1]:.2g}, corrector order 1 {lin_err[1][0]:.2g}")
    assert max(quad_err[2][1], quad_err[3][1]) <= 1e-12                      # predictor, order 3
    assert max(quad_err[2][0], quad_err[5][0]) <= 1e-12                      # corrector, order 2 (of steps 1 and 4)
    assert max(quad_err[3][0], quad_err[4][0]) <= 1e-12                      # corrector, order 3: degree <= 3
    assert max(cubic_err[3][0], cubic_err[4][0]) <= 1e-12
    assert cubic_err[2][1] > 1e-6 and cubic_err[2][0] > 1e-6                 # one degree too many for either
    assert lin_err[1][1] > 1e-4 and lin_err[4][1] > 1e-4                     # the published shortcut, not the solve
    assert max(lin_err[2][1], lin_err[3][1], lin_err[2][0], lin_err[3][0]) <= 1e-12


# ------------------------------------------------------------------------------------------------ (c) corrector off
@pytest.mark.parametrize("n", [6, 10, 20])
def test_corrector_off_is_dpm_solver(n):
    """With the corrector disabled at every step, order 2 / bh2 is this project's DPM-Solver++ 2M `step()` and order 1
    its first-order one, in float64."""
    from v_express_amd import DPMSolverMultistepScheduler
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(64, generator=g, dtype=torch.float64)
    vs = [torch.randn(64, generator=g, dtype=torch.float64) for _ in range(n)]
    for order in (2, 1):
        u = make(solver_order=order, disable_corrector=list(range(n)))
        d = DPMSolverMultistepScheduler(**{**D.KWARGS, "solver_order": order})
        for s in (u, d):
            s.set_timesteps(n)
        assert torch.equal(u.sigmas, d.sigmas) and torch.equal(u.timesteps, d.timesteps)
        xu, xd = x0.clone(), x0.clone()
        for t, v in zip(u.timesteps.tolist(), vs):
            ou, od = u.step(v, t, xu), d.step(v, t, xd)
            xu, xd = ou.prev_sample, od.prev_sample
            assert rel_l2(xu, xd) <= 1e-10 and rel_l2(ou.pred_original_sample, od.pred_original_sample) <= 1e-10
        assert torch.equal(xu, ou.pred_original_sample)          # the step to sigma = 0 returns m exactly
        assert [c.use_c for c in u.loop_steps(u.timesteps.tolist(), 0)[1]] == [0] * n


def test_stateful_step_matches_the_restated_step_and_resets():
    s = make(solver_order=3)
    s.set_timesteps(7)
    sg = [float(v) for v in s.sigmas]
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(32, generator=g, dtype=torch.float64)
    vs = [torch.randn(32, generator=g, dtype=torch.float64) for _ in range(7)]

    def run(ts, vs_):
        x = x0.clone()
        for t, v in zip(ts, vs_):
            x = s.step(v, t, x).prev_sample
        return x
    a = run(s.timesteps.tolist(), vs)
    s.set_timesteps(7)
    assert s.step_index is None and torch.equal(run(s.timesteps.tolist(), vs), a)
    xr, st = x0.clone(), U.State()
    for i, v in enumerate(vs):
        xr = U.step(sg, 7, i, xr, v, st, 3)
    assert rel_l2(a, xr) <= 1e-10
    # a run that starts inside the schedule (strength < 1): first order and no corrector at its first step
    s.set_timesteps(7)
    b = run(s.timesteps.tolist()[3:], vs[3:])
    xr, st = x0.clone(), U.State()
    for i in range(3, 7):
        xr = U.step(sg, 7, i, xr, vs[i], st, 3)
    assert rel_l2(b, xr) <= 1e-10 and rel_l2(b, a) > 1e-3
    s.set_timesteps(7)
    (prev,) = s.step(vs[0], s.timesteps[0], x0, return_dict=False)
    assert prev.shape == x0.shape and s.step_index == 1


# ------------------------------------------------------------------------------------------------ (d) analytic model
def _analytic_error(s, n, xT):
    """tests/test_dpm_solver_cpu.py's model - data N(0, 0.6^2) per element, the exact v-prediction, the zero-SNR schedule:
    the probability-flow ODE maps x_T to 0.6 x_T.  The error of the final std."""
    abar = D.alphas_cumprod(clamp=False)
    s2 = 0.36

    def vhat(x, t):
        a, sg = math.sqrt(abar[t]), math.sqrt(1.0 - abar[t])
        return a * sg * (1.0 - s2) / (a * a * s2 + sg * sg) * x
    s.set_timesteps(n)
    x = xT.clone()
    for t in s.timesteps.tolist():
        x = s.step(vhat(x, int(t)), t, x).prev_sample
    return abs(float(x.std()) - 0.6 * float(xT.std()))


def test_analytic_model_corrector_lowers_the_error():
    from v_express_amd import DPMSolverMultistepScheduler
    xT = torch.from_numpy(np.random.default_rng(0).standard_normal(10000))
    print("[analytic model] steps: |final std - 0.6 std(x_T)|  UniPC 2 bh2 / the same, corrector off / DPM++ 2M / UniPC 2 bh1")
    for n in (5, 8, 10, 15, 25):
        uni = _analytic_error(make(), n, xT)
        off = _analytic_error(make(disable_corrector=list(range(n))), n, xT)
        dpm = _analytic_error(DPMSolverMultistepScheduler(**D.KWARGS), n, xT)
        bh1 = _analytic_error(make(solver_type="bh1"), n, xT)
        print(f"    {n:2d}: {uni:.4f} / {off:.4f} / {dpm:.4f} / {bh1:.4f}")
        if n < 25:                                               # (at 25 steps corrector on and off tie)
            assert uni < dpm and uni < off


# ------------------------------------------------------------------------------------------------ (e) options
def test_options_and_construction():
    from v_express_amd import DDIMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler
    from v_express_amd.scheduler import _Scheduler
    s = UniPCMultistepScheduler(**D.KWARGS)                      # inference_v2.yaml's noise_scheduler_kwargs, unchanged
    assert isinstance(s, _Scheduler) and s.order == 1 and s.init_noise_sigma == 1.0
    assert (s.config.solver_order, s.config.solver_type, s.config.final_sigmas_type, s.config.disable_corrector,
            s.config.predict_x0, s.config.lower_order_final) == (2, "bh2", "zero", [], True, True)
    ddim, dpm = DDIMScheduler(**D.KWARGS), DPMSolverMultistepScheduler(**D.KWARGS)
    for src in (ddim.config, dict(D.KWARGS)):                    # clip_sample, set_alpha_to_one, ... of DDIM: ignored
        f = UniPCMultistepScheduler.from_config(src, solver_order=3)
        assert f.config.solver_order == 3
        for sch in (f, s, dpm):
            sch.set_timesteps(15)
        assert torch.equal(f.sigmas, s.sigmas) and torch.equal(f.alphas_cumprod, s.alphas_cumprod)
    # the tables, the levels and add_noise are DPM-Solver++'s, the 2^-24 clamp included
    assert torch.equal(s.sigmas, dpm.sigmas) and torch.equal(s.timesteps, dpm.timesteps)
    assert torch.equal(s.alphas_cumprod, dpm.alphas_cumprod) and float(s.alphas_cumprod[-1]) == 2.0 ** -24
    assert [s.noise_coefficients(j) for j in range(16)] == [dpm.noise_coefficients(j) for j in range(16)]
    assert s.noise_coefficients(15) == (1.0, 0.0)
    x, z = torch.randn(2, 3), torch.randn(2, 3)
    assert torch.equal(s.add_noise(x, z, s.timesteps[3]), dpm.add_noise(x, z, dpm.timesteps[3]))
    assert s.scale_model_input(x, 999) is x
    m = make(final_sigmas_type="sigma_min")
    m.set_timesteps(15)
    assert torch.equal(m.sigmas[:15], s.sigmas[:15]) and float(m.sigmas[-1]) > 0
    for zero_snr in (True, False):
        make(rescale_betas_zero_snr=zero_snr).set_timesteps(5)
    for bad in (dict(solver_order=4), dict(solver_order=0), dict(prediction_type="epsilon"), dict(predict_x0=False),
                dict(solver_type="midpoint"), dict(lower_order_final=False), dict(disable_corrector=[0.5]),
                dict(solver_p=object()), dict(use_karras_sigmas=True), dict(thresholding=True),
                dict(timestep_spacing="leading"), dict(final_sigmas_type="denoise_to_zero"), dict(trained_betas=[0.1, 0.2])):
        name = next(iter(bad))
        with pytest.raises(NotImplementedError, match=f"UniPCMultistepScheduler: {name}"):
            make(**bad)
    with pytest.raises(NotImplementedError, match="eta"):
        s.loop_steps(s.timesteps.tolist(), 0, eta=0.5)


def test_unbuilt_routes_fail_before_any_kernel(emulated, small_pipe, monkeypatch):
    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "known_blend", "overlap_ddim_step", "overlap_unipc_step",
                 "ncfhw_to_nhwc", "groupnorm", "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)
    with pytest.raises(NotImplementedError, match="eta"):
        call_pipeline(small_pipe, make(), inputs(4), 4, 2, 4, 2, eta=0.5)


def test_unsupported_scheduler_message_names_the_class(small_pipe):
    class Other:
        pass
    small_pipe.scheduler = Other()
    with pytest.raises(TypeError, match="DPMSolverMultistepScheduler or v_express_amd.UniPCMultistepScheduler or .*"
                                        "EulerDiscreteScheduler, LMSDiscreteScheduler or PNDMScheduler, not Other"):
        small_pipe._sampler()
    small_pipe.scheduler = make()
    assert small_pipe._sampler() == "unipc"


# ------------------------------------------------------------------------------------------------ (f) __call__
def _call(scheduler, inp, F_, steps, cf, co, **kw):
    """On a pipeline of its own."""
    import loop_worker
    return call_pipeline(loop_worker.build_pipeline("cpu"), scheduler, inp, F_, steps, cf, co, **kw)


def _counted(emulated):
    calls = []
    orig = emulated.overlap_unipc_step

    def counted(*a):
        calls.append((a[-1], a[5], a[6]))
        return orig(*a)
    emulated.overlap_unipc_step = counted
    return calls


@pytest.mark.parametrize("solver_order", [2, 3])
def test_pipeline_call_vs_restated_oracle_loop(emulated, solver_order):
    """__call__ with UniPC (5 steps, reflected last window [8, 9, 10, 9]) under emulated kernels against the per-frame
    restated loop over the oracle UNet: one overlap_unipc_step per timestep, the history and the saved sample the same
    buffers throughout; the DPM++ 2M clip of the same inputs differs (the corrector really ran).  The tolerance is the
    DPM-Solver++ test's."""
    from oracle import loop as OL
    from v_express_amd import DPMSolverMultistepScheduler
    F_, cf, co, _ = cases.PIPELINE_CASES["reflected_F11_c4o2"]
    steps = 5
    inp = inputs(F_)
    calls = _counted(emulated)
    seen = []
    got = _call(make(solver_order=solver_order), inp, F_, steps, cf, co, callback=lambda i, t, lat: seen.append(i))
    assert len(calls) == steps and seen == list(range(steps))
    assert [c.use_c for c, _, _ in calls] == [0, 1, 1, 1, 0] and calls[0][0][:4] == (-1, -1, -1, 0)
    assert len({id(h) for _, h, _ in calls}) == 1 and len({id(s) for _, _, s in calls}) == 1
    assert tuple(calls[0][1].shape) == (3, 4, F_, 8, 8) and calls[0][2].shape == inp["latents"].shape
    with torch.no_grad():
        ref = U.restated_unipc_loop(oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), cases.GUIDANCE,
                                    inp["kps_features"], inp["audio_embeddings"], steps, solver_order=solver_order)
    r = rel_l2(got, ref)
    rd = rel_l2(_call(DPMSolverMultistepScheduler(**D.KWARGS), inp, F_, steps, cf, co), ref)
    print(f"[__call__ UniPC order {solver_order}, emulated kernels, reflected_F11_c4o2, {steps} steps] relL2 vs restated "
          f"oracle loop {r:.4g} (the DPM++ 2M clip: {rd:.4g})")
    assert torch.isfinite(got).all() and r <= 5e-2 and rd > 2 * r


def test_init_video_sampling_and_strength(emulated):
    """strength 0.6 of 5 steps with init latents and a soft mask: the run starts at begin_index 2 with an empty history
    (first order, no corrector), the known blend moves the latents only, and the clip matches the restated loop; strength
    alone (no init clip) starts the same way."""
    from oracle import loop as OL
    F_, cf, co, _ = cases.PIPELINE_CASES["reflected_F11_c4o2"]
    steps, strength = 5, 0.6
    inp = inputs(F_)
    init = 0.5 * torch.randn(1, 4, F_, 8, 8, generator=torch.Generator().manual_seed(5))
    mask = torch.ones(F_, 1, 64, 64)
    mask[:2] = 0.0
    mask[:, :, :28] = 0.0
    m = R.box_mean(mask[:, 0])
    assert sorted(m.unique().tolist()) == [0.0, 0.5, 1.0]
    calls = _counted(emulated)
    got = _call(make(solver_order=3), inp, F_, steps, cf, co, strength=strength, init_latents=init, mask=mask)
    # (the last step ends at sigma = 0: it returns m, reads nothing and skips its corrector)
    assert [c[:5] for c, _, _ in calls] == [(-1, -1, -1, 0, 0), (0, -1, -1, 1, 1), (-1, -1, -1, 2, 0)]
    with torch.no_grad():
        ref = U.restated_unipc_loop(oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), cases.GUIDANCE,
                                    inp["kps_features"], inp["audio_embeddings"], steps, solver_order=3,
                                    known=(init, inp["latents"], m, strength))
    r = rel_l2(got, ref)
    print(f"[__call__ UniPC order 3, init_latents + soft mask, strength {strength}, {steps} steps] relL2 vs restated loop "
          f"{r:.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2
    keep = (m == 0).reshape(1, 1, F_, 8, 8).expand_as(got)
    assert torch.equal(got[keep], init[keep])
    del calls[:]
    plain = _call(make(solver_order=3), inp, F_, steps, cf, co, strength=strength)
    assert len(calls) == 3 and calls[0][0][:5] == (-1, -1, -1, 0, 0) and torch.isfinite(plain).all()


def test_two_gloo_ranks_are_bit_identical_to_one_process(emulated):
    """Every rank applies the update to the same gathered predictions and keeps the same history and saved sample: the
    clip of two gloo ranks (the windows of F = 14, 8 / 2 split over them) is bit-identical to one process, on both."""
    ref = UW.run()
    for rank, lat in enumerate(spawn_gloo(UW.main, 2, timeout=600)):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))


# ------------------------------------------------------------------------------------------------ (g) the fourth header
def test_fourth_header_parses_and_is_disjoint_from_the_others():
    from v_express_amd import abi
    s = abi.solvers_header()
    assert s is abi.solvers_header() and s.version == 1 and not s.enums and not s.structs
    assert list(s.functions) == ["vx_solvers_abi_version", "vx_overlap_unipc_step"]
    assert not set(s.functions) & (set(abi.header().functions) | set(abi.guidance_header().functions) |
                                   set(abi.samplers_header().functions))
    assert abi.header().version == 15 and abi.samplers_header().version == 1
    assert list(abi.samplers_header().functions) == ["vx_samplers_abi_version", "vx_overlap_linear_step"]
    i32, vp, fl = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float
    assert s.functions["vx_solvers_abi_version"] == (i32, [])
    restype, params = s.functions["vx_overlap_unipc_step"]
    assert restype is i32
    assert [t for _, t in params] == [vp, i32, i32, i32, vp, i32, vp, i32, vp, vp, i32, vp] + [i32] * 4 + [vp, i32] + \
        [fl] * 11 + [vp]
    from v_express_amd.scheduler import UniPCStep
    assert tuple(n for n, _ in params[12:16]) + tuple(n for n, _ in params[17:29]) == UniPCStep._fields
    assert [n for n, _ in params][:12] == [n for n, _ in abi.samplers_header().functions["vx_overlap_linear_step"][1]][:12]
    text = open(abi.SOLVERS_HEADER).read()
    assert "K = T + 11" in text
    with pytest.raises(ImportError, match="VX_ABI_VERSION"):
        abi.parse(text, "solvers.h")
    assert abi.parse(text, "solvers.h", "VX_SOLVERS_ABI_VERSION").functions == s.functions


def test_fourth_header_is_bound_on_both_libraries_and_stamped():
    import os
    import subprocess
    import sys
    from v_express_amd import abi, lib
    functions = abi.solvers_header().functions
    assert not set(functions) & set(lib.declared_symbols())          # declared_symbols keeps meaning the first header
    for so in (lib.lib, lib.lib_f16()):
        for n, (restype, params) in functions.items():
            fn = so.__dict__[n]                                      # __dict__: the function objects _load touched
            assert fn.restype is restype and list(fn.argtypes) == [t for _, t in params], n
        assert so.vx_solvers_abi_version() == abi.solvers_header().version == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "lib_id.py")], capture_output=True, text=True)
    assert out.stdout.strip() == lib.source_id()
    assert "vexpress_hip_solvers.h" in open(os.path.join(root, "tools", "lib_id.py")).read()
    mk = open(os.path.join(lib.CSRC, "Makefile")).read()
    assert "vexpress_hip_solvers.h" in mk and "vx_unipc.hip" in mk


# ------------------------------------------------------------------------------------------------ (h) argument checks
def test_overlap_unipc_step_argument_checks(monkeypatch):
    """Every check of the wrapper fails before the library is asked (its entry point is replaced by one that fails)."""
    from v_express_amd import lib, ops
    from v_express_amd.scheduler import UniPCStep

    def no_launch(*a):
        raise AssertionError("the library was called")
    for so in (lib.lib, lib.lib_f16()):
        monkeypatch.setattr(so, "vx_overlap_unipc_step", no_launch)
    monkeypatch.setattr(ops, "_stream", lambda: None)                # (no device in this suite to ask for its stream)
    C, F_, h, w, nW, f, T = 4, 6, 4, 4, 2, 4, 2
    good = dict(latents=torch.zeros(1, C, F_, h, w), preds=torch.zeros(nW, C, f, h * w),
                terms=torch.zeros(3, T, 2, dtype=torch.int32), frame_ids=torch.arange(3, dtype=torch.int32),
                counts=torch.ones(3), history=torch.zeros(3, C, F_, h, w), saved=torch.zeros(1, C, F_, h, w),
                coef=UniPCStep(0, 1, -1, 2, 1, 0.5, 0.25, 1.0, 0.5, 0.1, 0.2, 0.0, 0.3, 0.4, 0.6, 0.7))

    def call(**kw):
        a = {**good, **kw}
        ops.overlap_unipc_step(*(a[k] for k in ("latents", "preds", "terms", "frame_ids", "counts", "history", "saved",
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
                                               history=None, saved=torch.zeros(1, C, F_, 3, 3),
                                               coef=cf._replace(h1=-1, h2=-1, h_write=-1))),
            (ValueError, "terms must be", dict(terms=torch.zeros(2, T, 2, dtype=torch.int32))),
            (ValueError, "terms must be", dict(counts=torch.ones(4))),
            (ValueError, "h2", dict(coef=cf._replace(h2=3))),
            (ValueError, "h_write", dict(coef=cf._replace(h_write=-2))),
            (ValueError, "h1", dict(coef=cf._replace(h1=1.0))),
            (ValueError, "use_c", dict(coef=cf._replace(use_c=2))),
            (ValueError, "history is None", dict(history=None)),
            (ValueError, "saved is None", dict(saved=None)),
            (ValueError, "saved is None", dict(saved=None, coef=cf._replace(use_c=0))),
            (TypeError, "history", dict(history=torch.zeros(2, C, F_, h, w))),
            (TypeError, "history", dict(history=good["history"].double())),
            (TypeError, "saved", dict(saved=torch.zeros(1, C, F_ + 1, h, w))),
            (ValueError, "finite", dict(coef=cf._replace(q_1=float("nan")))),
            (ValueError, "finite", dict(coef=cf._replace(k_x=float("inf"))))]:
        with pytest.raises(err, match=match):
            call(**kw)
    # the history may be absent when the coefficients name no slot
    with pytest.raises(AssertionError, match="the library was called"):
        call(history=None, coef=cf._replace(h1=-1, h2=-1, h_write=-1))
