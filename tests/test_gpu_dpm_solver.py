"""DPM-Solver++ multistep sampling on the MI355X: `vx_overlap_multistep_step` (both libraries) against float64 over four
consecutive updates, VExpressPipeline with v_express_amd.DPMSolverMultistepScheduler against the per-frame restated loop
over the oracle UNet, first-order DPM++ against the DDIM pipeline, and a two-window clip at the SD-1.5 widths."""
import pytest
import torch

import cases
import dpm_restated as D
from loop_restated import restated_loop
from loop_worker import call_small as _call, cosine, dev, oracle_on_cpu, rel_l2, small  # noqa: F401

pytestmark = pytest.mark.gpu


def check(got, ref, what, rel, mx):
    """tests/test_gpu_kernels.py's bound: max |err| <= mx * max|ref| + 1e-5 and relative L2 <= rel."""
    got, ref = got.double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err = (got - ref).abs()
    r = rel_l2(got, ref)
    assert err.max().item() <= mx * ref.abs().max().item() + 1e-5 and r <= rel, \
        f"{what}: max|err|={err.max().item():.4g}, relL2={r:.3g}"


def make(**kw):
    from v_express_amd import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**{**D.KWARGS, **kw})


# ------------------------------------------------------------------------------------------------ (e) kernel
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
def test_multistep_kernel_four_updates_vs_float64(dev, elem):
    """Orders 1, 2, 2 and the final sigma = 0 step (4 steps) over the reflected-window plan of F = 11 (last window
    [8, 9, 10, 9]), the x0 history carried on the device between them."""
    from oracle import loop as OL
    from v_express_amd import lib as L, ops
    from v_express_amd.context import overlap_plan
    F_, f, h, w = 11, 4, 8, 8
    hw = h * w
    windows = OL.uniform_windows(F_, f, 2)
    plan = overlap_plan(windows, F_)
    sf = plan["step_frames"]
    terms = torch.full((len(sf), plan["max_terms"], 2), -1, dtype=torch.int32)
    for i, fr in enumerate(sf):
        for j, (wi, li) in enumerate(plan["terms"][fr]):
            terms[i, j, 0], terms[i, j, 1] = wi, li
    counts = [float(plan["counts"][fr]) for fr in sf]
    s = make()
    s.set_timesteps(4)
    assert [s.solver_order_at(i) for i in range(4)] == [1, 2, 2, 1] and float(s.sigmas[-1]) == 0.0
    g = torch.Generator().manual_seed(7)
    lat = torch.randn(1, 4, F_, h, w, generator=g)
    ref, hist_ref = lat.double().clone(), torch.zeros_like(lat, dtype=torch.float64)
    with L.element_type(elem):
        lat_d = lat.to(dev)
        hist = torch.full_like(lat_d, float("nan"))          # the first update must not read it
        args = (terms.to(dev), torch.tensor(sf, dtype=torch.int32, device=dev), torch.tensor(counts, device=dev))
        for i in range(4):
            preds = torch.randn(len(windows), 4, f, hw, generator=g)
            coef = s.multistep_coefficients(i)
            ops.overlap_multistep_step(lat_d, preds.to(dev), *args, hist, coef)
            a, sd, cx, c0, c1 = coef
            for k, fr in enumerate(sf):
                v = sum(preds[wi, :, li].double() / counts[k] for wi, li in plan["terms"][fr]).view(4, h, w)
                x = ref[0, :, fr].clone()
                x0 = a * x - sd * v
                ref[0, :, fr] = cx * x - c0 * x0 + c1 * hist_ref[0, :, fr]
                hist_ref[0, :, fr] = x0
            check(lat_d, ref, f"overlap_multistep_step update {i} (order {s.solver_order_at(i)}, {elem})", 1e-5, 1e-5)
            check(hist, hist_ref, f"x0 history after update {i} ({elem})", 1e-5, 1e-5)
        torch.cuda.synchronize()
    assert torch.equal(lat_d, hist)                          # the sigma = 0 step stores x0 itself


# ------------------------------------------------------------------------------------------------ (f), (g) pipeline
def test_pipeline_dpm_solver_vs_restated_oracle_loop(small):
    from oracle import loop as OL
    steps = 6
    got = _call(small, make(), steps)
    inp = small["inp"]
    with oracle_on_cpu():
        ref = restated_loop(small["oracle"], inp["latents"], OL.uniform_windows(small["F"], small["cf"], small["co"]),
                            cases.GUIDANCE, inp["kps_features"], inp["audio_embeddings"], steps, "dpm")
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[DPM++ 2M, SMALL, reflected_F11_c4o2, {steps} steps] relL2={r:.4g} cosine={c:.6f} vs the restated loop")
    assert torch.isfinite(got).all() and r <= 5e-2 and c >= 0.998, (r, c)


def test_first_order_dpm_solver_matches_the_ddim_pipeline(small):
    """1000 % 10 == 0: first-order DPM++ is DDIM's update (up to the 2^-24 clamp of the first sigma); the two clips differ
    by the bf16 rounding of the UNet inputs."""
    from v_express_amd import DDIMScheduler
    dpm1 = _call(small, make(solver_order=1), 10)
    ddim = _call(small, DDIMScheduler(**D.KWARGS), 10)
    r = rel_l2(dpm1, ddim)
    print(f"[10 steps, SMALL, reflected_F11_c4o2] first-order DPM++ vs DDIM relL2={r:.4g}")
    assert torch.isfinite(dpm1).all() and r <= 1e-2


# ------------------------------------------------------------------------------------------------ (h) SD-1.5 widths
def test_fullsize_two_windows_dpm_solver_15_steps_with_decode(dev):
    """512x512, F = 28 (windows [0..15] and [12..27]), DPM++ 2M at 15 steps, decoded: finite frames in [0, 1], and one
    UNet call per window (units_per_call 2) bit-identical to both windows in one call (4)."""
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
    pipe = VExpressPipeline(vae=vae, reference_net=refnet, denoising_unet=unet, scheduler=make())
    F_, cf, co, _ = cases.FULLSIZE_F28_CASE
    inp = synth.synthetic_inputs(cfg, F_, 64, 64, seed=42, device=dev)
    videos = {}
    for upc in (2, 4):
        pipe.units_per_call = upc
        videos[upc] = pipe(None, None, None, 512, 512, F_, 15, cases.GUIDANCE, context_frames=cf, context_overlap=co,
                           reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD,
                           reference_latents=inp["ref_latents"], kps_features=inp["kps_features"],
                           audio_embeddings=inp["audio_embeddings"], latents=inp["latents"], output_device=None)
    v = videos[4]
    print(f"[SD-1.5 widths, 512x512, F=28, DPM++ 2M 15 steps] video mean {v.mean().item():.4f} "
          f"std {v.std().item():.4f}")
    assert v.shape == (1, 3, F_, 512, 512) and torch.isfinite(v).all()
    assert v.min().item() >= 0.0 and v.max().item() <= 1.0 and v.std().item() > 0
    assert torch.equal(videos[2], videos[4])
