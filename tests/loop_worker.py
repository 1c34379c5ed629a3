"""What the test workers share (TEST INFRASTRUCTURE): the small-config pipeline, the kernel emulation of the CPU suite and
one way to drive the denoising loop on it."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cases  # noqa: E402


class _Setattr:
    setattr = staticmethod(setattr)


def emulate_kernels(patch=_Setattr):
    """CPU suite only: tests/fake_ops.py stands in for the HIP wrappers and the device guards are lifted, so the whole
    host side (models, loop, sharding) runs in a process without a GPU.  `patch`: anything with a pytest monkeypatch's
    setattr; by default the replacements stay for the life of the process (a spawned worker)."""
    import fake_ops
    from v_express_amd import ops, unet_3d, vae
    fake_ops.install(patch, ops)
    patch.setattr(unet_3d._UNetBase, "_need_gpu", lambda self: None)
    patch.setattr(vae.AutoencoderKLDecoder, "_need_gpu", lambda self: None)
    if os.environ.get("VX_TEST_FORCE_ROUND4") == "1":
        force_round4_paths(ops, patch.setattr)
    return ops


def force_round4_paths(ops, patch=setattr):
    """The round-4 host paths at the small widths of the CPU models, where the routing rules would not pick them: every
    temporal attention block as ONE `ops.tblock_fused` call (also in the pixel-shard layout of a frame-sharded unit), row
    statistics as two-part sums ([rows, 4] buffers) at every width."""
    patch(ops, "tblock_fused_applies", lambda c, heads, f, hw: True)
    patch(ops, "STATS_PARTS_WIDTHS", set(range(8, 4096, 8)))


def build_pipeline(device):
    """The small-config pipeline (UNet3D + ReferenceNet + VAE decoder, seeded synthetic weights)."""
    from v_express_amd import (AutoencoderKLDecoder, DDIMScheduler, UNet2DConditionModel, UNet3DConditionModel,
                               VExpressPipeline, synth)
    cfg = cases.unet_cfg(cases.SMALL)
    vcfg = synth.VaeConfig(**cases.SMALL_VAE)
    unet = UNet3DConditionModel(cfg).to(device)
    refnet = UNet2DConditionModel(cfg).to(device)
    unet.load_state_dict(synth.unet3d_state_dict(cfg), strict=True)
    refnet.load_state_dict(synth.refnet_state_dict(cfg), strict=True)
    vae = AutoencoderKLDecoder(vcfg).to(device)
    vae.load_state_dict(synth.vae_decoder_state_dict(vcfg))
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                          steps_offset=1, prediction_type="v_prediction", rescale_betas_zero_snr=True,
                          timestep_spacing="trailing")
    return VExpressPipeline(vae=vae, reference_net=refnet, denoising_unet=unet, scheduler=sched)


def run_loop(pipe, F, context, overlap, steps, *, schedule="uniform", latent, device, **loop_kwargs):
    """The denoising loop of `pipe` (its scheduler, `steps` timesteps) on the seeded synthetic clip of F frames of
    latent x latent, windows of `context` frames: the pieces of VExpressPipeline.__call__ in its order, then
    `pipe.denoise(..., **loop_kwargs)` on the windows themselves, so that a worker can reach every keyword of the loop
    (last_overlap's schedule stays None).  Returns the final latents on the CPU."""
    from v_express_amd import ReferenceAttentionControl, ops, synth
    from v_express_amd.context import get_context_scheduler
    cfg = cases.unet_cfg(cases.SMALL)
    unet, refnet, sched = pipe.denoising_unet, pipe.reference_net, pipe.scheduler
    inp = synth.synthetic_inputs(cfg, F, latent, latent, device=device)
    writer = ReferenceAttentionControl(refnet, do_classifier_free_guidance=True, mode="write", fusion_blocks="full")
    reader = ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", fusion_blocks="full",
                                       reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD)
    refnet(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768, device=device),
           return_dict=False)
    reader.update(writer, True, dtype=unet.dtype)
    sched.set_timesteps(steps)
    windows = list(get_context_scheduler(schedule)(step=0, num_frames=F, context_size=context, context_stride=1,
                                                   context_overlap=overlap, closed_loop=False))
    c0 = cfg.block_out_channels[0]
    kps = ops.ncfhw_to_nhwc(inp["kps_features"], c0).view(2, F, latent * latent, c0)
    audio = inp["audio_embeddings"].to(torch.bfloat16).contiguous()
    lat = inp["latents"].clone().float() * sched.init_noise_sigma        # (1 but for Euler ancestral)
    pipe.denoise(lat, kps, audio, sched.timesteps.tolist(), windows, cases.GUIDANCE, **loop_kwargs)
    return lat.cpu()
