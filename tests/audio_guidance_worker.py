"""One rank of the two-rank runs of tests/test_audio_guidance_cpu.py (gloo, emulated kernels) and
tests/test_gpu_audio_guidance.py (ranks folded onto one GPU, real kernels) (TEST INFRASTRUCTURE): the small-config
denoising loop (DDIM) with three rows per window (audio_guidance_scale), the rescale and a guidance interval.
usage (GPU, under torch.distributed.run): audio_guidance_worker.py OUT.pt GEOMETRY"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import guidance_restated as G  # noqa: E402

# name -> (F, context frames, overlap): one window = 3 units (on two ranks (u, m) | (c): the c row runs alone), two
# windows = 6 units
GEOMETRY = {"one_window": (8, 8, 2), "two_windows": (14, 8, 2)}
# 3 DDIM steps of which the first 2 are guided (1 / 3 <= 0.67 and 2 / 3 <= 0.67; 3 / 3 is not)
S_AUDIO, STEPS, PHI, END = 6.0, 3, 0.7, 0.67


def run(geometry, latent=8, device="cpu", frame_shards=1):
    """frame_shards = 1: whole units only, so that three units on two ranks leave one row alone on a rank."""
    from v_express_amd import DDIMScheduler
    pipe = W.build_pipeline(device)
    pipe.scheduler = DDIMScheduler(**G.KWARGS)
    pipe.frame_shards = frame_shards
    lat = W.run_loop(pipe, *GEOMETRY[geometry], STEPS, latent=latent, device=device, guidance_rescale=PHI,
                     guidance_end=END, audio_guidance_scale=S_AUDIO)
    assert pipe.last_guidance["guided_steps"] == 2 and pipe.last_guidance["rows"] == ("u", "m", "c")
    return lat, dict(pipe.last_schedule), dict(pipe.last_guidance)


def main(rank, geometry, latent=8):
    """CPU, one rank of loop_worker.spawn_gloo: this rank's final latents and its two schedules."""
    torch.set_num_threads(2)
    W.emulate_kernels()
    return run(geometry, latent)


if __name__ == "__main__":
    import torch.distributed as dist
    out_path, geometry = sys.argv[1], sys.argv[2]
    dist.init_process_group(os.environ.get("VX_DIST_BACKEND", "gloo"))
    torch.cuda.set_device(0)
    lat, sched, guid = run(geometry, device="cuda")
    if dist.get_rank() == 0:
        torch.save(dict(latents=lat, schedule=sched), out_path)
    dist.barrier()
    dist.destroy_process_group()
