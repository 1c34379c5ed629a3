"""Launch census of the benchmarked clip on a real MI355X: BASELINE configs[1] built as bench.py builds it (SD-1.5 widths,
512x512 = 64x64 latents, one window, CFG 3.5, bf16, synthetic weights and inputs drawn on the device with bench.py's
seeds), recorded by tests/census.py: every distinct launch of the ReferenceNet + bank pass, of each DDIM step and of the
decode is checked against its float64 restatement (tests/fake_ops.py) on the arguments it really got, at the bound of
that op's own test; every kernel instantiation the clip launched must have been checked; and the recorded run must be
bit-identical to an unrecorded one (the census disturbs nothing).

    python -m pytest tests/test_gpu_census.py -m gpu -q -s        (prints one table row per checked signature)
"""
import time

import pytest
import torch

import census

pytestmark = pytest.mark.gpu

# GEMM variants the benchmarked configuration launches (profiles/r06zh_gemm_by_shape.txt) and the attention kernel of the
# 64x64 level: the census must have seen - and checked - each of them
MUST_SEE = ("coop2", "splitk4", "gather", "SPLIT")


@pytest.fixture(scope="module")
def models():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import v_express_amd as vx
    from v_express_amd import synth
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    elem = torch.bfloat16
    cfg, vcfg = synth.UNetConfig(), synth.VaeConfig()
    unet = vx.UNet3DConditionModel(cfg).to(dev).to(elem)
    refnet = vx.UNet2DConditionModel(cfg).to(dev).to(elem)
    vae = vx.AutoencoderKLDecoder(vcfg).to(dev).to(elem)
    unet.load_state_dict(synth.unet3d_state_dict(cfg, seed=42, device=dev, dtype=elem, draw_on_device=True))
    unet.release_raw_weights()
    refnet.load_state_dict(synth.refnet_state_dict(cfg, seed=43, device=dev, dtype=elem, draw_on_device=True))
    refnet.release_raw_weights()
    vae.load_state_dict(synth.vae_decoder_state_dict(vcfg, seed=44, device=dev, dtype=elem, draw_on_device=True))
    vae._prepared()
    sched = vx.DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                             steps_offset=1, prediction_type="v_prediction", rescale_betas_zero_snr=True,
                             timestep_spacing="trailing")
    pipe = vx.VExpressPipeline(vae=vae, reference_net=refnet, denoising_unet=unet, scheduler=sched)
    return dict(cfg=cfg, unet=unet, refnet=refnet, pipe=pipe, sched=sched, dev=dev)


def _clip(m, F, steps, decode, cen=None):
    """The phases of one clip: ReferenceNet write pass + reader.update, `steps` DDIM steps of 25 (each its own phase:
    the step boundary comes through denoise's callback), the decode.  -> (latents, video or None)."""
    import v_express_amd as vx
    from v_express_amd import ops, synth
    from v_express_amd.context import uniform
    cfg, unet, refnet, pipe, sched, dev = (m[k] for k in ("cfg", "unet", "refnet", "pipe", "sched", "dev"))
    h = w = 64

    def phase(name):
        if cen is not None:
            cen.phase = name
    phase("refnet+bank")                 # (with the per-clip input layouts: the kps tokens' ncfhw_to_nhwc)
    unet._temb_cache.clear()
    inp = synth.synthetic_inputs(cfg, F, h, w, seed=42, device=dev)
    writer = vx.ReferenceAttentionControl(refnet, do_classifier_free_guidance=True, mode="write", fusion_blocks="full")
    reader = vx.ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", fusion_blocks="full",
                                          reference_attention_weight=0.95, audio_attention_weight=3.0)
    sched.set_timesteps(25)
    timesteps = sched.timesteps.tolist()[:steps]
    windows = list(uniform(step=0, num_frames=F, context_size=F, context_stride=1, context_overlap=4, closed_loop=False))
    assert len(windows) == 1
    c0 = cfg.block_out_channels[0]
    kps_tokens = ops.ncfhw_to_nhwc(inp["kps_features"], c0).view(2, F, h * w, c0)
    audio = inp["audio_embeddings"].to(torch.bfloat16).contiguous()
    lat = inp["latents"].clone()
    torch.cuda.synchronize()

    def next_step(i, t, latents):
        phase(f"DDIM step {i + 2}")
    refnet(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768, device=dev), return_dict=False)
    reader.update(writer, True)
    phase("DDIM step 1")
    pipe.denoise(lat, kps_tokens, audio, timesteps, windows, 3.5, callback=next_step)
    phase("decode")
    video = pipe.decode_latents(lat) if decode else None
    torch.cuda.synchronize()
    return lat, video


@pytest.mark.parametrize("F,steps,decode", [(16, 2, True), (24, 1, False)], ids=["bench_f16", "ctx24"])
def test_every_launch_of_the_clip_matches_its_float64_restatement(models, monkeypatch, F, steps, decode):
    from v_express_amd import ops
    t0 = time.time()
    cen = census.Census(ops)
    with monkeypatch.context() as mp:
        cen.install(mp)
        with cen.recording():
            lat, video = _clip(models, F, steps, decode, cen)
    t_rec = time.time() - t0
    print(f"\n[census F={F}, {steps} DDIM step(s){', decode' if decode else ''}]\n{cen.report()}")
    t1 = time.time()
    lat0, video0 = _clip(models, F, steps, decode)
    print(f"recorded + checked run {t_rec:.1f} s, plain run {time.time() - t1:.1f} s")
    # (a) every checked launch within its bound, (b) coverage
    cen.assert_clean()
    syms = cen.symbols()
    gemm_syms = [s for s in syms if s.startswith("gemm")]
    if F == 16:
        for v in MUST_SEE:
            assert any(v in s for s in gemm_syms), f"no {v} GEMM launched: {sorted(gemm_syms)}"
        assert any(s.startswith("attn3_kernel") for s in syms), sorted(syms)
    # the one-launch temporal block of the window's length
    assert f"tblock_kernel<{F}>" in syms, sorted(syms)
    phases = {r.phase for r in cen.rows.values()}
    assert phases == {"refnet+bank"} | {f"DDIM step {i + 1}" for i in range(steps)} | ({"decode"} if decode else set())
    # (c) the census disturbs nothing
    assert torch.equal(lat, lat0), (lat - lat0).abs().max().item()
    if decode:
        assert torch.equal(video, video0), (video - video0).abs().max().item()
