"""Ancestral sampling on the host: the counter-based noise restated (Philox4x32-10 known answers), the update
coefficients of DDIMScheduler.ancestral_coefficients (eta > 0) and EulerAncestralDiscreteScheduler against diffusers'
textbook updates in float64, Euler ancestral against DDIM eta = 1, the analytic model, the options, and
VExpressPipeline.__call__ with the ancestral update under emulated kernels (one process and two gloo ranks)."""
import math

import numpy as np
import pytest
import torch

import ancestral_restated as A
import cases
import dpm_restated as D
from loop_restated import restated_loop
from loop_worker import (SEED, call_pipeline as _call, emulated, inputs, oracle_unet, rel_l2,  # noqa: F401
                         small_pipe, spawn_gloo)


def ddim(**kw):
    from v_express_amd import DDIMScheduler
    return DDIMScheduler(**{**A.KWARGS, **kw})


def euler(**kw):
    from v_express_amd import EulerAncestralDiscreteScheduler
    return EulerAncestralDiscreteScheduler(**{**A.KWARGS, **kw})


def apply(coef, x, v, z):
    a, s, cx, c0, cz = coef
    return cx * x - c0 * (a * x - s * v) + cz * z


# ------------------------------------------------------------------------------------------------ (1) noise
def test_philox_known_answers_and_the_noise_mapping():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in A.philox4x32_10(ctr, key)) == want
    # the mapping: key = (seed lo, seed hi), counter = (quad, channel, frame, step), Box-Muller on (r0, r1) / (r2, r3)
    seed, step, frame, ch, q = (0xA4093822 << 32) | 0x1234, 7, 5, 2, 3
    r = [int(v) for v in A.philox4x32_10((q, ch, frame, step), (0x1234, 0xA4093822))]
    z = A.normals(seed, step, [frame], 4, 64)[ch, 0, 4 * q:4 * q + 4]
    for (a, b), (za, zb) in zip(((r[0], r[1]), (r[2], r[3])), (z[:2], z[2:])):
        u1, u2 = ((a >> 8) + 1) * 2.0 ** -24, (b >> 8) * 2.0 ** -24
        rho = math.sqrt(-2.0 * math.log(u1))
        assert za == pytest.approx(rho * math.cos(2 * math.pi * u2), abs=1e-15)
        assert zb == pytest.approx(rho * math.sin(2 * math.pi * u2), abs=1e-15)
    # u1 never reaches 0: the largest magnitude a word pair can give is sqrt(2 * 24 ln 2)
    assert np.abs(A.normals(1, 0, range(4), 4, 4096)).max() <= math.sqrt(48 * math.log(2))


# ------------------------------------------------------------------------------------------------ (2) coefficients
@pytest.mark.parametrize("n", [8, 10, 15, 25, 50])
def test_ddim_eta_coefficients_vs_textbook(n):
    s = ddim()
    s.set_timesteps(n)
    g = torch.Generator().manual_seed(n)
    x, v, z = (torch.randn(256, generator=g, dtype=torch.float64) for _ in range(3))
    for eta in (0.3, 1.0, 0.0):
        for t in s.timesteps.tolist():
            a, ap = (float(u) for u in s._alphas(t))              # the float32 table, float64 arithmetic
            coef = s.ancestral_coefficients(t, eta)
            assert all(isinstance(c, float) and math.isfinite(c) for c in coef)
            ref = A.ddim_eta_update(a, ap, eta, x, v, z)
            assert rel_l2(apply(coef, x, v, z), ref) <= 1e-12, (eta, t)
            if eta == 0.0:
                # eta = 0 draws nothing and is today's DDIM update (step_coefficients: fp32-rounded scalars)
                assert coef[4] == 0.0
                sa, s1a, sap, s1ap = s.step_coefficients(t)
                today = sap * (sa * x - s1a * v) + s1ap * (sa * v + s1a * x)
                assert rel_l2(apply(coef, x, v, z), today) <= 1e-6
    # a last step that ends below t = 0 (alpha_prev = 1) returns x0 exactly (n = 15 ends at t = 66 - 66 = 0)
    if int(s.timesteps[-1]) - 1000 // n < 0:
        assert s.ancestral_coefficients(s.timesteps[-1], 1.0)[2:] == (0.0, -1.0, 0.0)


@pytest.mark.parametrize("n", [8, 10, 15, 25, 50])
def test_euler_ancestral_coefficients_vs_textbook_ve_frame(n):
    s = euler()
    s.set_timesteps(n)
    sg = [float(u) for u in s.sigmas]
    g = torch.Generator().manual_seed(100 + n)
    x_ve, v, z = (torch.randn(256, generator=g, dtype=torch.float64) for _ in range(3))
    x_ve = x_ve * 3.0
    for i in range(n):
        coef = s.ancestral_coefficients(i)
        ref_vp = A.euler_a_update_ve(sg[i], sg[i + 1], x_ve, v, z) / math.sqrt(1.0 + sg[i + 1] ** 2)
        got = apply(coef, x_ve / math.sqrt(1.0 + sg[i] ** 2), v, z)
        assert rel_l2(got, ref_vp) <= 1e-12, i
        assert coef[0] == pytest.approx(1.0 / math.sqrt(1.0 + sg[i] ** 2), rel=1e-15)
        assert s.frame_scale(i) == pytest.approx(math.sqrt(1.0 + sg[i] ** 2), rel=1e-15)
    assert s.ancestral_coefficients(n - 1)[2:] == (0.0, -1.0, 0.0) and s.frame_scale(n) == 1.0
    # a later start (strength < 1, begin_index b > 0): the VP run from step b is the VE run from step b
    b = n // 3
    x_vp = x_ve / s.frame_scale(b)
    xr = x_ve.clone()
    for i in range(b, n):
        zi = torch.randn(256, generator=g, dtype=torch.float64)
        vi = 0.3 * (s.ancestral_coefficients(i)[0] * x_vp) + 0.1 * zi
        x_vp = apply(s.ancestral_coefficients(i), x_vp, vi, zi)
        xr = A.euler_a_update_ve(sg[i], sg[i + 1], xr, vi, zi)
    assert rel_l2(x_vp, xr) <= 1e-12


def test_euler_ancestral_stateful_step_matches_the_coefficients():
    """The diffusers-style tensor step (VE frame, float32, noise from the generator) against the VP coefficients."""
    s = euler()
    s.set_timesteps(10)
    g = torch.Generator().manual_seed(3)
    x_ve = torch.randn(1, 4, 2, 8, 8, generator=g) * float(s.init_noise_sigma)
    for i, t in enumerate(s.timesteps.tolist()):
        v = torch.randn(x_ve.shape, generator=g)
        gs = torch.Generator().manual_seed(1000 + i)
        z = torch.randn(x_ve.shape, generator=torch.Generator().manual_seed(1000 + i))
        want = apply(s.ancestral_coefficients(i), x_ve.double() / s.frame_scale(i), v.double(), z.double())
        assert s.step_index in (None, i)
        x_ve = s.step(v, t, x_ve, generator=gs).prev_sample
        assert rel_l2(x_ve / s.frame_scale(i + 1), want) <= 1e-5, i
    assert s.step_index == 10


# ------------------------------------------------------------------------------------------------ (3) Euler a == DDIM 1
def _gaussian_runs(n, sampler, x, zs, abar):
    s2 = 0.36

    def vhat(x, a, s):
        return a * s * (1.0 - s2) / (a * a * s2 + s * s) * x
    if sampler == "ddim":
        for i, (a, ap) in enumerate(A.ddim_table(n, abar)):
            x = A.ddim_eta_update(a, ap, 1.0, x, vhat(x, math.sqrt(a), math.sqrt(1 - a)), zs[i])
        return x
    sg = [math.sqrt((1.0 - abar[t]) / abar[t]) for t in D.timesteps(n)] + [0.0]
    x = x * math.sqrt(1.0 + sg[0] ** 2)
    for i in range(n):
        r = math.sqrt(1.0 + sg[i] ** 2)
        x = A.euler_a_update_ve(sg[i], sg[i + 1], x, vhat(x / r, 1.0 / r, sg[i] / r), zs[i])
    return x


def test_euler_ancestral_is_ddim_eta_one_when_the_steps_are_even():
    """On the clamped table, float64, shared noise, exact Gaussian model: the two samplers are one when n divides 1000
    (DDIM's previous timestep is the next trailing timestep); at n = 15 the trailing timesteps are not evenly spaced."""
    abar = D.alphas_cumprod(clamp=True)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.standard_normal(4096))
    zs = [torch.from_numpy(rng.standard_normal(4096)) for _ in range(40)]
    for n in (8, 10, 25, 40):
        d = (_gaussian_runs(n, "ddim", x, zs, abar) - _gaussian_runs(n, "euler", x, zs, abar)).abs().max().item()
        print(f"[Euler a vs DDIM eta=1, {n} steps] max |diff| = {d:.3g}")
        assert d <= 1e-13, n
    d15 = (_gaussian_runs(15, "ddim", x, zs, abar) - _gaussian_runs(15, "euler", x, zs, abar)).abs().max().item()
    print(f"[Euler a vs DDIM eta=1, 15 steps] max |diff| = {d15:.3g}")
    assert 0.05 <= d15 <= 0.15


# ------------------------------------------------------------------------------------------------ (4) analytic model
def _analytic_std(n, sampler, N=400_000):
    """Data N(0, 0.6^2), exact v-prediction, this project's coefficient methods, noise from numpy seed 0."""
    rng = np.random.default_rng(0)
    x = rng.standard_normal(N)
    if sampler == "euler-a":
        s = euler()
        s.set_timesteps(n)
        coefs = [s.ancestral_coefficients(i) for i in range(n)]
        x = x * float(s.init_noise_sigma) / s.frame_scale(0)
    else:
        s = ddim()
        s.set_timesteps(n)
        coefs = [s.ancestral_coefficients(t, 0.0 if sampler == "ddim" else 1.0) for t in s.timesteps.tolist()]
    for a, sd, cx, c0, cz in coefs:
        v = a * sd * (1.0 - 0.36) / (a * a * 0.36 + sd * sd) * x
        x = cx * x - c0 * (a * x - sd * v) + (cz * rng.standard_normal(N) if cz else 0.0)
    return float(x.std())


def test_analytic_model_final_std():
    """The data std is 0.6.  On this schedule every sampler ends below it and closes in with more steps; the ancestral
    samplers (DDIM eta = 1, Euler a) end further below it than deterministic DDIM at the same step count: they need
    more steps for the same spread."""
    want = {10: (0.477, 0.442, 0.443), 15: (0.526, 0.483, 0.479), 25: (0.543, 0.513, 0.515),
            50: (0.568, 0.548, 0.548)}
    got = {n: tuple(_analytic_std(n, smp) for smp in ("ddim", "ddim-eta", "euler-a")) for n in want}
    for n, row in got.items():
        print(f"[analytic model] {n:2d} steps: DDIM eta=0 {row[0]:.4f}  DDIM eta=1 {row[1]:.4f}  Euler a {row[2]:.4f}")
        for g_, w_ in zip(row, want[n]):
            assert abs(g_ - w_) <= 0.005, (n, row)
        assert row[1] < row[0] and row[2] < row[0]
    for k in range(3):
        col = [got[n][k] for n in sorted(got)]
        assert col == sorted(col) and len(set(col)) == len(col)


# ------------------------------------------------------------------------------------------------ (5) options
def test_euler_ancestral_options_and_construction():
    from v_express_amd import DDIMScheduler, EulerAncestralDiscreteScheduler
    import v_express_amd
    assert "EulerAncestralDiscreteScheduler" in v_express_amd.__all__
    s = EulerAncestralDiscreteScheduler(**A.KWARGS)          # inference_v2.yaml's noise_scheduler_kwargs, unchanged
    for src in (DDIMScheduler(**A.KWARGS).config, dict(A.KWARGS)):
        f = EulerAncestralDiscreteScheduler.from_config(src)
        f.set_timesteps(15)
        s.set_timesteps(15)
        assert torch.equal(f.sigmas, s.sigmas) and torch.equal(f.timesteps, s.timesteps)
    for n in (8, 15, 25):
        s.set_timesteps(n)
        assert s.timesteps.dtype == torch.float32 and s.timesteps.tolist() == [float(t) for t in D.timesteps(n)]
        assert s.sigmas.dtype == torch.float32 and len(s.sigmas) == n + 1 and float(s.sigmas[-1]) == 0.0
        ref = D.sigmas(n)
        assert max(abs(float(a) / b - 1) for a, b in zip(s.sigmas[:n], ref[:n])) <= 2e-4
        # the 2^-24 clamp: sigma_max = sqrt(2^24 - 1), init_noise_sigma = sigma_max ("trailing")
        assert float(s.alphas_cumprod[-1]) == 2.0 ** -24
        assert float(s.init_noise_sigma) == float(s.sigmas.max()) == pytest.approx(math.sqrt(2.0 ** 24 - 1), rel=1e-7)
    x = torch.randn(4)
    s.set_timesteps(10)
    assert torch.equal(s.scale_model_input(x, 999), x / ((s.sigmas[0] ** 2 + 1) ** 0.5))
    for bad in (dict(prediction_type="epsilon"), dict(timestep_spacing="leading"), dict(beta_schedule="linear"),
                dict(trained_betas=[0.1] * 1000)):
        name = next(iter(bad))
        with pytest.raises(NotImplementedError, match=name):
            euler(**bad)


def test_eta_limits():
    s = ddim()
    s.set_timesteps(25)
    with pytest.raises(ValueError, match="eta"):
        [s.ancestral_coefficients(t, 1.5) for t in s.timesteps.tolist()]
    with pytest.raises(ValueError, match="eta"):
        s.ancestral_coefficients(999, -0.1)
    # eta = 1 is fine at every step, including t = 999 where 1 - a' - sigma^2 is 0 exactly
    assert all(math.isfinite(c) for t in s.timesteps.tolist() for c in s.ancestral_coefficients(t, 1.0))


# ------------------------------------------------------------------------------------------------ (6) __call__
@pytest.mark.parametrize("sampler", ["ddim-0.5", "ddim-1", "euler-a"])
def test_pipeline_call_ancestral_vs_restated_oracle_loop(emulated, small_pipe, sampler):
    """__call__ (reflected last window [8, 9, 10, 9], 5 steps) under emulated kernels against the per-frame restated loop
    over the oracle UNet with the restated noise; units_per_call 2 and 4 give the same bits."""
    from oracle import loop as OL
    F_, cf, co, _ = cases.PIPELINE_CASES["reflected_F11_c4o2"]
    steps = 5
    inp = inputs(F_)
    eta = {"ddim-0.5": 0.5, "ddim-1": 1.0, "euler-a": 0.0}[sampler]
    sched = euler() if sampler == "euler-a" else ddim()
    calls = []
    orig = emulated.overlap_ancestral_step

    def counted(*a):
        calls.append(a[-1])
        return orig(*a)
    emulated.overlap_ancestral_step = counted
    seen = []
    runs = {}
    try:
        for upc in (2, 4):
            small_pipe.units_per_call = upc
            runs[upc] = _call(small_pipe, sched, inp, F_, steps, cf, co, eta=eta, noise_seed=SEED,
                              callback=lambda i, t, x: seen.append((i, x.clone())))
    finally:
        small_pipe.units_per_call = 2
    got = runs[2]
    assert calls == list(range(steps)) * 2 and torch.equal(runs[2], runs[4])
    with torch.no_grad():
        ref = restated_loop(oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), cases.GUIDANCE,
                            inp["kps_features"], inp["audio_embeddings"], steps,
                            "euler-a" if sampler == "euler-a" else "ddim-eta", seed=SEED, eta=eta)
    r = rel_l2(got, ref)
    print(f"[__call__ {sampler}, emulated kernels, reflected_F11_c4o2, {steps} steps] relL2 vs restated loop {r:.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2
    # the callback sees the scheduler's frame: Euler a's first latents are at sigma(t_1) scale, the last are x0
    assert [i for i, _ in seen[:steps]] == list(range(steps)) and torch.equal(seen[steps - 1][1], got)
    if sampler == "euler-a":
        sched.set_timesteps(steps)
        assert seen[0][1].std().item() > 0.5 * float(sched.sigmas[1])
    # a different seed gives a different clip
    other = _call(small_pipe, sched, inp, F_, steps, cf, co, eta=eta, noise_seed=SEED + 1)
    assert rel_l2(other, got) > 1e-2


def test_pipeline_seed_from_the_generator(emulated, small_pipe):
    """noise_seed=None: one draw from the generator after the initial latents (which stay what they were); the same
    generator seed gives the same clip; noise_seed overrides the generator."""
    from v_express_amd import synth
    F_, cf, co = 6, 4, 2
    inp = synth.synthetic_inputs(cases.unet_cfg(cases.SMALL), F_, 8, 8)
    seeds = []
    orig = emulated.overlap_ancestral_step

    def spy(*a):
        seeds.append(a[-2])
        return orig(*a)
    emulated.overlap_ancestral_step = spy

    def run(gseed, **kw):
        g = torch.Generator().manual_seed(gseed)
        out = _call(small_pipe, euler(), inp, F_, 2, cf, co, latents=None, generator=g, **kw)
        return out, g
    a, ga = run(11)
    b, gb = run(11)
    assert torch.equal(a, b) and seeds[0] == seeds[2]
    # what the generator was asked for: the latents, then one 63-bit seed
    g = torch.Generator().manual_seed(11)
    torch.randn((1, 4, F_, 8, 8), generator=g)
    assert seeds[0] == int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g))
    assert torch.equal(ga.get_state(), g.get_state())
    c, _ = run(12)
    assert rel_l2(c, a) > 1e-2
    d, _ = run(12, noise_seed=seeds[0])
    e, _ = run(13, noise_seed=seeds[0])
    assert seeds[-1] == seeds[0] and not torch.equal(d, a)     # d: the latents of 12, the noise of 11
    assert rel_l2(d, e) > 1e-2                                 # different latents, same noise


def test_pipeline_ddim_eta_zero_is_unchanged(emulated, small_pipe, monkeypatch):
    """DDIM at eta = 0: the ancestral op is never called, the generator gives only the latents, and the clip is that of
    the DDIM update on those latents."""
    from v_express_amd import synth
    F_, cf, co = 6, 4, 2
    inp = synth.synthetic_inputs(cases.unet_cfg(cases.SMALL), F_, 8, 8)

    def boom(*a, **k):
        raise AssertionError("the ancestral update ran")
    monkeypatch.setattr(emulated, "overlap_ancestral_step", boom)
    g = torch.Generator().manual_seed(5)
    got = _call(small_pipe, ddim(), inp, F_, 3, cf, co, latents=None, generator=g)
    g2 = torch.Generator().manual_seed(5)
    lat = torch.randn((1, 4, F_, 8, 8), generator=g2)
    assert torch.equal(g.get_state(), g2.get_state())
    ref = _call(small_pipe, ddim(), inp, F_, 3, cf, co, latents=lat, eta=0.0)
    assert torch.equal(got, ref)


def test_eta_with_other_schedulers_and_bad_eta_fail_before_any_kernel(emulated, small_pipe, monkeypatch):
    from v_express_amd import DPMSolverMultistepScheduler, synth

    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "overlap_ddim_step", "overlap_multistep_step",
                 "overlap_ancestral_step", "ncfhw_to_nhwc", "groupnorm", "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)
    inp = synth.synthetic_inputs(cases.unet_cfg(cases.SMALL), 4, 8, 8)
    for sched in (DPMSolverMultistepScheduler(**A.KWARGS), euler()):
        with pytest.raises(NotImplementedError, match="eta"):
            _call(small_pipe, sched, inp, 4, 2, 4, 2, eta=0.5)
    with pytest.raises(ValueError, match="eta"):
        _call(small_pipe, ddim(), inp, 4, 25, 4, 2, eta=1.5)
    with pytest.raises(ValueError, match="noise_seed"):
        small_pipe.scheduler = euler()
        small_pipe.scheduler.set_timesteps(2)
        small_pipe.denoise(inp["latents"].clone(), None, None, small_pipe.scheduler.timesteps.tolist(),
                           [[0, 1, 2, 3]], cases.GUIDANCE)


def test_two_gloo_ranks_with_euler_ancestral_are_bit_identical_to_one_process(emulated):
    """The noise depends on (seed, step, frame, channel, pixel) only: the clip of two gloo ranks (the windows of F = 14,
    8 / 2 split over them) is bit-identical to one process, on both ranks."""
    import ancestral_worker
    ref = ancestral_worker.run()
    for rank, lat in enumerate(spawn_gloo(ancestral_worker.main, 2, timeout=600)):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))
