"""Weighted window blending on the MI355X: `vx_overlap_blend` (both libraries) bit for bit against the float32 torch
restatement and within its bound of float64, its argument errors, VExpressPipeline with `context_schedule="uniform_fit"`
and `overlap_blend="linear"` against the restated loop over the oracle UNet (DDIM, DPM++ 2M), the identities with the mean
route, and one full-size clip."""
import pytest
import torch

import cases
import dpm_restated as D
import window_blend_restated as WB
from loop_restated import restated_loop
from loop_worker import (SEED, call_pipeline, cosine, dev, inputs, oracle_on_cpu, rel_l2,  # noqa: F401
                         scheduler, small)

pytestmark = pytest.mark.gpu


def _windows(name, F_, f, o):
    from v_express_amd.context import get_context_scheduler
    return list(get_context_scheduler(name)(step=0, num_frames=F_, context_size=f, context_stride=1, context_overlap=o,
                                            closed_loop=False))


# ------------------------------------------------------------------------------------------------ the kernel
# (c, hw, F, f, o, blend): one quad per row and blocks with idle threads; three terms, padded -1 terms and a tail block;
# every frame with another term count; the production plan
SHAPES = [(4, 4, 5, 3, 1, "linear"), (4, 36, 11, 4, 2, "linear"), (3, 64, 7, 4, 3, "pyramid"), (4, 4096, 44, 24, 4, "linear")]


@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("c,hw,F_,f,o,blend", SHAPES)
def test_blend_kernel_vs_float32_restatement_and_float64(dev, elem, c, hw, F_, f, o, blend):
    from v_express_amd import lib as L, ops
    from v_express_amd.context import blend_weights, weighted_overlap_plan
    ws = _windows("uniform_fit", F_, f, o)
    plan = weighted_overlap_plan(ws, F_, blend_weights(ws, blend))
    terms, wts = WB.tables(plan)
    if (F_, f, o) == (7, 4, 3):
        assert sorted(set(len(t) for t in plan["terms"].values())) == [1, 2, 3, 4]
    if plan["max_terms"] > 1:
        # a skipped first term: the first frame of two or more terms leads with -1, its second term initialises the sum
        i = next(i for i in range(F_) if len(plan["terms"][i]) >= 2)
        terms[i, 0] = -1
    assert int(terms[..., 0].max()) < len(ws) and int(terms[..., 1].max()) < f and tuple(terms.shape) == (F_, plan["max_terms"], 2)
    g = torch.Generator().manual_seed(13)
    # a different constant per (slot, channel, position) plus noise: a wrong index cannot cancel
    base = torch.arange(len(ws) * c * f, dtype=torch.float32).view(len(ws), c, f, 1) * 0.37 - 3.0
    preds = base + torch.randn(len(ws), c, f, hw, generator=g)
    want = torch.empty(c, F_, hw)
    WB.overlap_blend(preds, terms, wts, want)
    ref, bound = WB.overlap_blend64(preds, terms, wts)
    with L.element_type(elem):
        out = torch.full((c, F_, hw), float("nan"), device=dev)
        ops.overlap_blend(preds.to(dev), terms.to(dev), wts.to(dev), out)
        torch.cuda.synchronize()
    got = out.cpu()
    ratio = ((got.double() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"[vx_overlap_blend {elem}, c {c}, hw {hw}, F {F_}, f {f}, o {o}, {blend}] max |err| / bound vs float64 = "
          f"{ratio:.4f}")
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert ((got.double() - ref).abs() <= bound).all()


def test_blend_argument_errors_before_any_launch(dev):
    from v_express_amd import lib as L, ops
    terms = torch.tensor([[[0, 0]], [[0, 1]]], dtype=torch.int32, device=dev)
    wts = torch.ones(2, 1, device=dev)
    with pytest.raises(L.VxError, match="hw % 4 == 0"):
        ops.overlap_blend(torch.zeros(1, 2, 2, 6, device=dev), terms, wts, torch.zeros(2, 2, 6, device=dev))
    flat = torch.zeros(1 * 2 * 2 * 8 + 1, device=dev)
    off = flat[1:].view(1, 2, 2, 8)                           # 4 bytes past a 16-byte boundary
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(L.VxError, match="16-byte aligned"):
        ops.overlap_blend(off, terms, wts, torch.zeros(2, 2, 8, device=dev))
    with pytest.raises(L.VxError, match="16-byte aligned"):
        ops.overlap_blend(torch.zeros(1, 2, 2, 8, device=dev), terms, wts, flat[1:].view(2, 2, 8))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the device loop
def _call(S, sched, steps, F_=None, **kw):
    F_ = F_ or S["F"]
    return call_pipeline(S["pipe"], sched, inputs(F_), F_, steps, S["cf"], S["co"], **kw).cpu()


@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_pipeline_uniform_fit_linear_vs_restated_oracle_loop(small, kind):
    """SMALL, F 11 in even-fit windows of 4 with overlap 2, 6 steps: rel-L2 <= 5e-2 and cosine >= 0.998 against the
    float64-weighted restated loop (tests/test_gpu_dpm_solver.py's bound for this pipeline); the mean route's pair from
    the same run is printed next to it."""
    steps = 6
    F_, cf, co = small["F"], small["cf"], small["co"]
    assert (F_, cf, co) == (11, 4, 2)
    windows = WB.fit_windows(F_, cf, co)
    fit = dict(context_schedule="uniform_fit")
    got = _call(small, scheduler(kind), steps, overlap_blend="linear", **fit)
    assert small["pipe"].last_overlap == dict(schedule="uniform_fit", blend="linear", windows=5, max_terms=3,
                                              blend_launches=steps)
    mean = _call(small, scheduler(kind), steps, **fit)
    inp = small["inp"]
    with oracle_on_cpu():
        ref, ref_mean = (restated_loop(small["oracle"], inp["latents"], windows, cases.GUIDANCE, inp["kps_features"],
                                       inp["audio_embeddings"], steps, kind, raw=raw)
                         for raw in (WB.raw_weights(windows, "linear"), None))
    r, c = rel_l2(got, ref), cosine(got, ref)
    rm, cm = rel_l2(mean, ref_mean), cosine(mean, ref_mean)
    print(f"[{kind}, SMALL, uniform_fit F11 c4 o2, {steps} steps] linear: relL2={r:.4g} cosine={c:.6f}; mean: "
          f"relL2={rm:.4g} cosine={cm:.6f} vs the restated loops")
    assert torch.isfinite(got).all() and not torch.equal(got, mean)
    assert r <= 5e-2 and c >= 0.998, (r, c)


def test_device_identities(small):
    from v_express_amd import DDIMScheduler
    steps = 3
    # two windows (F 6: counts 1 and 2): the ones profile is the mean route, bit for bit
    mean6 = _call(small, scheduler("ddim"), steps, F_=6)
    ones6 = _call(small, scheduler("ddim"), steps, F_=6, overlap_blend=[1.0] * 4)
    assert small["pipe"].last_overlap["blend_launches"] == steps
    assert torch.isfinite(mean6).all() and torch.equal(mean6, ones6)
    # overlap_blend="mean" is no keyword at all
    base = _call(small, scheduler("ddim"), steps)
    same = _call(small, scheduler("ddim"), steps, overlap_blend="mean")
    assert torch.equal(base, same) and small["pipe"].last_overlap["blend_launches"] == 0
    # DDIM eta = 1 with "linear": one UNet call per window against merged calls
    pipe, clips = small["pipe"], {}
    upc = pipe.units_per_call
    try:
        for n in (1, 4):
            pipe.units_per_call = n
            clips[n] = _call(small, DDIMScheduler(**D.KWARGS), steps, eta=1.0, noise_seed=SEED,
                             context_schedule="uniform_fit", overlap_blend="linear")
    finally:
        pipe.units_per_call = upc
    assert torch.isfinite(clips[1]).all() and torch.equal(clips[1], clips[4]) and not torch.equal(clips[1], base)


# ------------------------------------------------------------------------------------------------ full size
def test_fullsize_F44_linear_two_dpm_steps_with_decode(dev):
    """512x512, F = 44 in windows of 24 with overlap 4 (the production plan), 2 DPM++ steps with "linear", decoded."""
    from v_express_amd import (AutoencoderKLDecoder, DPMSolverMultistepScheduler, UNet2DConditionModel,
                               UNet3DConditionModel, VExpressPipeline, synth)
    cfg, vcfg = cases.unet_cfg(cases.FULL), synth.VaeConfig()
    unet = UNet3DConditionModel(cfg).to(dev)
    refnet = UNet2DConditionModel(cfg).to(dev)
    vae = AutoencoderKLDecoder(vcfg).to(dev)
    unet.load_state_dict(synth.unet3d_state_dict(cfg, seed=42, device=dev, draw_on_device=True))
    unet.release_raw_weights()
    refnet.load_state_dict(synth.refnet_state_dict(cfg, seed=43, device=dev, draw_on_device=True))
    refnet.release_raw_weights()
    vae.load_state_dict(synth.vae_decoder_state_dict(vcfg, seed=44, device=dev, draw_on_device=True))
    pipe = VExpressPipeline(vae=vae, reference_net=refnet, denoising_unet=unet,
                            scheduler=DPMSolverMultistepScheduler(**D.KWARGS))
    F_ = 44
    inp = synth.synthetic_inputs(cfg, F_, 64, 64, seed=42, device=dev)
    v = pipe(None, None, None, 512, 512, F_, 2, cases.GUIDANCE, context_frames=24, context_overlap=4,
             context_schedule="uniform_fit", overlap_blend="linear", reference_attention_weight=cases.W_REF,
             audio_attention_weight=cases.W_AUD, reference_latents=inp["ref_latents"], kps_features=inp["kps_features"],
             audio_embeddings=inp["audio_embeddings"], latents=inp["latents"], output_device=None)
    assert pipe.last_overlap == dict(schedule="uniform_fit", blend="linear", windows=2, max_terms=2, blend_launches=2)
    print(f"[SD-1.5 widths, 512x512, F=44, uniform_fit + linear, DPM++ 2M 2 steps] video mean {v.mean().item():.4f} "
          f"std {v.std().item():.4f}")
    assert v.shape == (1, 3, F_, 512, 512) and torch.isfinite(v).all()
    assert v.min().item() >= 0.0 and v.max().item() <= 1.0 and v.std().item() > 0
