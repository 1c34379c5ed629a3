"""One rank of tests/test_ancestral_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop
with Euler ancestral sampling under emulated kernels (tests/fake_ops.py + ancestral_restated.overlap_ancestral_step)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ancestral_restated as A  # noqa: E402
import cases  # noqa: E402
import dist_gpu_worker as W  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, four CFG units), 3 Euler ancestral steps, 8x8 latents
F, CF, CO, STEPS, LATENT, SEED = 14, 8, 2, 3, 8, (7 << 40) | 12345


def run():
    from v_express_amd import EulerAncestralDiscreteScheduler, ReferenceAttentionControl, ops, synth
    from v_express_amd.context import get_context_scheduler
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = sched = EulerAncestralDiscreteScheduler(**A.KWARGS)
    unet, refnet = pipe.denoising_unet, pipe.reference_net
    cfg = cases.unet_cfg(cases.SMALL)
    inp = synth.synthetic_inputs(cfg, F, LATENT, LATENT)
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
    kps = ops.ncfhw_to_nhwc(inp["kps_features"], c0).view(2, F, LATENT * LATENT, c0)
    audio = inp["audio_embeddings"].to(torch.bfloat16).contiguous()
    lat = inp["latents"].clone().float() * sched.init_noise_sigma
    pipe.denoise(lat, kps, audio, sched.timesteps.tolist(), windows, cases.GUIDANCE, noise_seed=SEED)
    return lat


def main():
    """Under RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT: this rank's final latents."""
    import torch.distributed as dist
    from v_express_amd import ops
    torch.set_num_threads(2)
    dist.init_process_group("gloo")
    W.emulate_kernels()
    ops.overlap_ancestral_step = A.overlap_ancestral_step
    lat = run()
    dist.barrier()
    dist.destroy_process_group()
    return lat
