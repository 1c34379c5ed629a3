"""One rank of tests/test_guidance_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop
(DDIM) with guidance_rescale and a guidance interval under emulated kernels (tests/fake_ops.py +
guidance_restated.guidance_rescale)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import dist_gpu_worker as W  # noqa: E402
import guidance_restated as G  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, four CFG units), 5 DDIM steps of which 3 are guided
F, CF, CO, STEPS, PHI, END = 14, 8, 2, 5, 0.7, 0.6


def run(frame_shards=None, latent=8):
    from v_express_amd import DDIMScheduler, ReferenceAttentionControl, ops, synth
    from v_express_amd.context import get_context_scheduler
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = sched = DDIMScheduler(**G.KWARGS)
    pipe.frame_shards = frame_shards
    unet, refnet = pipe.denoising_unet, pipe.reference_net
    cfg = cases.unet_cfg(cases.SMALL)
    inp = synth.synthetic_inputs(cfg, F, latent, latent)
    # the pieces of VExpressPipeline.__call__ in its order (as dist_gpu_worker._run on CPU tensors)
    writer = ReferenceAttentionControl(refnet, do_classifier_free_guidance=True, mode="write", fusion_blocks="full")
    reader = ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", fusion_blocks="full",
                                       reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD)
    refnet(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768), return_dict=False)
    reader.update(writer, True)
    sched.set_timesteps(STEPS)
    windows = list(get_context_scheduler("uniform")(step=0, num_frames=F, context_size=CF, context_stride=1,
                                                    context_overlap=CO, closed_loop=False))
    c0 = cfg.block_out_channels[0]
    kps = ops.ncfhw_to_nhwc(inp["kps_features"], c0).view(2, F, latent * latent, c0)
    audio = inp["audio_embeddings"].to(torch.bfloat16).contiguous()
    lat = inp["latents"].clone().float()
    pipe.denoise(lat, kps, audio, sched.timesteps.tolist(), windows, cases.GUIDANCE, guidance_rescale=PHI,
                 guidance_end=END)
    assert pipe.last_guidance["guided_steps"] == 3 and pipe.last_guidance["unguided_schedule"] is not None
    return lat, dict(pipe.last_schedule), dict(pipe.last_guidance)


def main(frame_shards=None, latent=8):
    """Under RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT: this rank's final latents and its two schedules."""
    import torch.distributed as dist
    from v_express_amd import ops
    torch.set_num_threads(2)
    dist.init_process_group("gloo")
    W.emulate_kernels()
    ops.guidance_rescale = G.guidance_rescale
    out = run(frame_shards, latent)
    dist.barrier()
    dist.destroy_process_group()
    return out
