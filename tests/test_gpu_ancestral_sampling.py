"""Ancestral sampling on the MI355X: `vx_overlap_ancestral_step` (both libraries) - its noise against the host restatement
of the counter-based generator, four consecutive updates of each sampler against float64, the noise statistics at the
configs[1] shape - VExpressPipeline with DDIM eta = 1 and Euler ancestral against the per-frame restated loop over the
oracle UNet, and a two-window Euler ancestral clip at the SD-1.5 widths."""
import math

import pytest
import torch

import ancestral_restated as A
import cases
from loop_restated import restated_loop
from loop_worker import call_small as _call, cosine, dev, oracle_on_cpu, rel_l2, small  # noqa: F401

pytestmark = pytest.mark.gpu

SEEDS = (0, 12345, (0xDEADBEEF << 32) | 0x01234567)


def check(got, ref, what, rel, mx):
    """tests/test_gpu_kernels.py's bound: max |err| <= mx * max|ref| + 1e-5 and relative L2 <= rel."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err = (got - ref).abs()
    r = rel_l2(got, ref)
    assert err.max().item() <= mx * ref.abs().max().item() + 1e-5 and r <= rel, \
        f"{what}: max|err|={err.max().item():.4g}, relL2={r:.3g}"


def plan_args(windows, F_, dev):
    from v_express_amd.context import overlap_plan
    plan = overlap_plan(windows, F_)
    sf = plan["step_frames"]
    terms = torch.full((len(sf), plan["max_terms"], 2), -1, dtype=torch.int32)
    for i, fr in enumerate(sf):
        for j, (wi, li) in enumerate(plan["terms"][fr]):
            terms[i, j, 0], terms[i, j, 1] = wi, li
    counts = [float(plan["counts"][fr]) for fr in sf]
    return plan, sf, counts, (terms.to(dev), torch.tensor(sf, dtype=torch.int32, device=dev),
                              torch.tensor(counts, device=dev))


# ------------------------------------------------------------------------------------------------ (1) kernel noise
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
def test_kernel_noise_vs_host_restatement(dev, elem):
    """(c_x, c_0, c_z) = (0, 0, 1) writes z itself: every step frame of the reflected F = 11 plan, several steps and
    seeds (one with the high 32 bits set)."""
    from oracle import loop as OL
    from v_express_amd import lib as L, ops
    F_, f, h, w = 11, 4, 8, 8
    windows = OL.uniform_windows(F_, f, 2)
    _, sf, _, args = plan_args(windows, F_, dev)
    worst = 0.0
    with L.element_type(elem):
        preds = torch.randn(len(windows), 4, f, h * w, device=dev)
        for seed in SEEDS:
            for step in (0, 1, 17, 999):
                lat = torch.randn(1, 4, F_, h, w, device=dev) * 1e3       # (0 x, 0 x0: only z remains)
                ops.overlap_ancestral_step(lat, preds, *args, (0.0, 0.0, 0.0, 0.0, 1.0), seed, step)
                ref = torch.from_numpy(A.normals(seed, step, sf, 4, h * w)).view(4, len(sf), h, w)
                got = lat[0, :, sf].cpu()
                err = (got.double() - ref).abs().max().item()
                worst = max(worst, err)
                assert torch.isfinite(got).all() and err <= 4e-6, (seed, step, err)
                # frames outside the plan's step frames are untouched (all eleven are step frames here)
                assert sorted(sf) == list(range(F_))
    print(f"[vx_overlap_ancestral_step noise, {elem}] max |z - restated z| = {worst:.3g}")


# ------------------------------------------------------------------------------------------------ (2) kernel update
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("sampler", ["ddim-eta", "euler-a"])
def test_ancestral_kernel_four_updates_vs_float64(dev, elem, sampler):
    from oracle import loop as OL
    from v_express_amd import DDIMScheduler, EulerAncestralDiscreteScheduler, lib as L, ops
    F_, f, h, w = 11, 4, 8, 8
    hw = h * w
    windows = OL.uniform_windows(F_, f, 2)
    plan, sf, counts, args = plan_args(windows, F_, dev)
    if sampler == "euler-a":
        s = EulerAncestralDiscreteScheduler(**A.KWARGS)
        s.set_timesteps(4)
        coefs = [s.ancestral_coefficients(i) for i in range(4)]
    else:
        s = DDIMScheduler(**A.KWARGS)
        s.set_timesteps(4)
        coefs = [s.ancestral_coefficients(t, 0.7) for t in s.timesteps.tolist()]
    assert coefs[-1][2:] == (0.0, -1.0, 0.0) and all(c[4] > 0 for c in coefs[:-1])
    seed = SEEDS[2]
    g = torch.Generator().manual_seed(9)
    lat = torch.randn(1, 4, F_, h, w, generator=g)
    ref = lat.double().clone()
    with L.element_type(elem):
        lat_d = lat.to(dev)
        for i in range(4):
            preds = torch.randn(len(windows), 4, f, hw, generator=g)
            ops.overlap_ancestral_step(lat_d, preds.to(dev), *args, coefs[i], seed, i)
            a, sd, cx, c0, cz = coefs[i]
            z = torch.from_numpy(A.normals(seed, i, sf, 4, hw))
            for k, fr in enumerate(sf):
                v = sum(preds[wi, :, li].double() / counts[k] for wi, li in plan["terms"][fr]).view(4, h, w)
                x = ref[0, :, fr].clone()
                ref[0, :, fr] = cx * x - c0 * (a * x - sd * v) + cz * z[:, k].view(4, h, w)
            check(lat_d, ref, f"overlap_ancestral_step {sampler} update {i} ({elem})", 1e-5, 1e-5)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (3) statistics
def test_noise_statistics_at_the_configs1_shape(dev):
    """16 frames x 4 x 64 x 64 = 262 144 normals per call: mean, variance and the correlation between neighbouring
    pixels, channels, frames, steps and seeds within 5 standard errors (deterministic for these seeds)."""
    from v_express_amd import ops
    F_, h = 16, 64
    _, _, _, args = plan_args([list(range(F_))], F_, dev)
    preds = torch.zeros(1, 4, F_, h * h, device=dev)

    def draw(seed, step):
        lat = torch.zeros(1, 4, F_, h, h, device=dev)          # (finite: 0 x and 0 x0 must be 0)
        ops.overlap_ancestral_step(lat, preds, *args, (0.0, 0.0, 0.0, 0.0, 1.0), seed, step)
        return lat[0].double().cpu()
    z = draw(SEEDS[2], 3)
    N = z.numel()
    assert N == 262144
    se = 1.0 / math.sqrt(N)

    def corr(a, b):
        a, b = a.flatten() - a.mean(), b.flatten() - b.mean()
        return (a @ b / (a.norm() * b.norm())).item()
    stats = dict(mean=z.mean().item(), var_minus_1=z.var().item() - 1.0,
                 pixel=corr(z[..., :-1], z[..., 1:]), row=corr(z[:, :, :-1], z[:, :, 1:]),
                 quad=corr(z.view(4, F_, -1, 4)[..., 1], z.view(4, F_, -1, 4)[..., 2]),
                 channel=corr(z[:-1], z[1:]), frame=corr(z[:, :-1], z[:, 1:]),
                 step=corr(z, draw(SEEDS[2], 4)), seed=corr(z, draw(SEEDS[2] + 1, 3)),
                 seed_hi=corr(z, draw(SEEDS[2] ^ (1 << 32), 3)))
    print("[noise statistics, 262144 normals] " + ", ".join(f"{k} {v:.2e}" for k, v in stats.items()))
    assert abs(stats["mean"]) <= 5 * se
    assert abs(stats["var_minus_1"]) <= 5 * math.sqrt(2.0 / N)
    for k in ("pixel", "row", "quad", "channel", "frame", "step", "seed", "seed_hi"):
        assert abs(stats[k]) <= 5 * se, k
    assert torch.equal(z, draw(SEEDS[2], 3))


# ------------------------------------------------------------------------------------------------ (4) pipeline
def _sched(sampler):
    from v_express_amd import DDIMScheduler, EulerAncestralDiscreteScheduler
    return (EulerAncestralDiscreteScheduler if sampler == "euler-a" else DDIMScheduler)(**A.KWARGS)


@pytest.mark.parametrize("sampler", ["ddim-eta", "euler-a"])
def test_pipeline_ancestral_vs_restated_oracle_loop(small, sampler):
    from oracle import loop as OL
    steps, seed = 6, SEEDS[2]
    eta = 1.0 if sampler == "ddim-eta" else 0.0
    got = _call(small, _sched(sampler), steps, eta=eta, noise_seed=seed)
    again = _call(small, _sched(sampler), steps, eta=eta, noise_seed=seed)
    other = _call(small, _sched(sampler), steps, eta=eta, noise_seed=seed + 1)
    assert torch.equal(got, again) and rel_l2(other, got) > 1e-2
    inp = small["inp"]
    with oracle_on_cpu():
        ref = restated_loop(small["oracle"], inp["latents"], OL.uniform_windows(small["F"], small["cf"], small["co"]),
                            cases.GUIDANCE, inp["kps_features"], inp["audio_embeddings"], steps, sampler, seed=seed,
                            eta=eta)
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[{sampler}, SMALL, reflected_F11_c4o2, {steps} steps] relL2={r:.4g} cosine={c:.6f} vs the restated loop")
    assert torch.isfinite(got).all() and r <= 5e-2 and c >= 0.998, (r, c)


def test_pipeline_ddim_eta_zero_does_not_touch_the_ancestral_kernel(small, monkeypatch):
    from v_express_amd import ops
    before = _call(small, _sched("ddim"), 4)

    def boom(*a, **k):
        raise AssertionError("the ancestral update ran")
    monkeypatch.setattr(ops, "overlap_ancestral_step", boom)
    after = _call(small, _sched("ddim"), 4, eta=0.0)
    assert torch.equal(before, after)


# ------------------------------------------------------------------------------------------------ (5) SD-1.5 widths
def test_fullsize_two_windows_euler_ancestral_25_steps_with_decode(dev):
    """512x512, F = 28 (windows [0..15] and [12..27]), Euler ancestral at 25 steps, decoded: finite frames in [0, 1],
    one UNet call per window (units_per_call 2) bit-identical to both windows in one call (4), and a video other than
    the DDIM one."""
    from v_express_amd import AutoencoderKLDecoder, UNet2DConditionModel, UNet3DConditionModel, VExpressPipeline, synth
    cfg, vcfg = cases.unet_cfg(cases.FULL), synth.VaeConfig()
    unet = UNet3DConditionModel(cfg).to(dev)
    refnet = UNet2DConditionModel(cfg).to(dev)
    vae = AutoencoderKLDecoder(vcfg).to(dev)
    unet.load_state_dict(synth.unet3d_state_dict(cfg, seed=42, device=dev, draw_on_device=True))
    unet.release_raw_weights()
    refnet.load_state_dict(synth.refnet_state_dict(cfg, seed=43, device=dev, draw_on_device=True))
    refnet.release_raw_weights()
    vae.load_state_dict(synth.vae_decoder_state_dict(vcfg, seed=44, device=dev, draw_on_device=True))
    pipe = VExpressPipeline(vae=vae, reference_net=refnet, denoising_unet=unet, scheduler=_sched("euler-a"))
    F_, cf, co, _ = cases.FULLSIZE_F28_CASE
    inp = synth.synthetic_inputs(cfg, F_, 64, 64, seed=42, device=dev)

    def run(sched, **kw):
        pipe.scheduler = sched
        return pipe(None, None, None, 512, 512, F_, 25, cases.GUIDANCE, context_frames=cf, context_overlap=co,
                    reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD,
                    reference_latents=inp["ref_latents"], kps_features=inp["kps_features"],
                    audio_embeddings=inp["audio_embeddings"], latents=inp["latents"], output_device=None, **kw)
    videos = {}
    for upc in (2, 4):
        pipe.units_per_call = upc
        videos[upc] = run(_sched("euler-a"), noise_seed=SEEDS[1])
    v = videos[4]
    ddim = run(_sched("ddim"))
    d = rel_l2(v, ddim)
    print(f"[SD-1.5 widths, 512x512, F=28, Euler a 25 steps] video mean {v.mean().item():.4f} "
          f"std {v.std().item():.4f}; relL2 to the DDIM video {d:.4g}")
    assert v.shape == (1, 3, F_, 512, 512) and torch.isfinite(v).all()
    assert v.min().item() >= 0.0 and v.max().item() <= 1.0 and v.std().item() > 0
    assert torch.equal(videos[2], videos[4])
    assert d > 1e-3
