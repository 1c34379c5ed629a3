"""One rank of the two-rank run of tests/test_window_blend_cpu.py (gloo, emulated kernels) (TEST INFRASTRUCTURE): the
small-config denoising loop (DDIM) over the even-fit windows of F = 7 (windows of 4, overlap 2: starts 0, 1, 3, so frame 3
lies in three windows) with the "linear" blend."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import dist_gpu_worker as W  # noqa: E402
import guidance_restated as G  # noqa: E402

F, CF, CO, STEPS, BLEND = 7, 4, 2, 2, "linear"


def run(latent=8, device="cpu", blend=BLEND):
    from v_express_amd import DDIMScheduler, ReferenceAttentionControl, ops, synth
    from v_express_amd.context import get_context_scheduler
    pipe = W.build_pipeline(device)
    pipe.scheduler = sched = DDIMScheduler(**G.KWARGS)
    pipe.frame_shards = 1
    unet, refnet = pipe.denoising_unet, pipe.reference_net
    cfg = cases.unet_cfg(cases.SMALL)
    inp = synth.synthetic_inputs(cfg, F, latent, latent, device=device)
    # the pieces of VExpressPipeline.__call__ in its order (as dist_gpu_worker._run on CPU tensors)
    writer = ReferenceAttentionControl(refnet, do_classifier_free_guidance=True, mode="write", fusion_blocks="full")
    reader = ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", fusion_blocks="full",
                                       reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD)
    refnet(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768, device=device),
           return_dict=False)
    reader.update(writer, True, dtype=unet.dtype)
    sched.set_timesteps(STEPS)
    windows = list(get_context_scheduler("uniform_fit")(step=0, num_frames=F, context_size=CF, context_stride=1,
                                                        context_overlap=CO, closed_loop=False))
    assert [w[0] for w in windows] == [0, 1, 3]
    c0 = cfg.block_out_channels[0]
    kps = ops.ncfhw_to_nhwc(inp["kps_features"], c0).view(2, F, latent * latent, c0)
    audio = inp["audio_embeddings"].to(torch.bfloat16).contiguous()
    lat = inp["latents"].clone().float()
    pipe.denoise(lat, kps, audio, sched.timesteps.tolist(), windows, cases.GUIDANCE, overlap_blend=blend)
    return lat.cpu(), dict(pipe.last_schedule), dict(pipe.last_overlap)


def main(latent=8):
    """CPU, under RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT: this rank's final latents and its two reports."""
    import torch.distributed as dist
    import window_blend_restated as WB
    from v_express_amd import ops
    torch.set_num_threads(2)
    dist.init_process_group("gloo")
    W.emulate_kernels()
    ops.overlap_blend = WB.overlap_blend
    out = run(latent)
    dist.barrier()
    dist.destroy_process_group()
    return out
