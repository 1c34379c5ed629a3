"""One rank of tests/test_guidance_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop
(DDIM) with guidance_rescale and a guidance interval under emulated kernels (loop_worker.emulate_kernels)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import guidance_restated as G  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, four CFG units), 5 DDIM steps of which 3 are guided
F, CF, CO, STEPS, PHI, END = 14, 8, 2, 5, 0.7, 0.6


def run(frame_shards=None, latent=8):
    from v_express_amd import DDIMScheduler
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = DDIMScheduler(**G.KWARGS)
    pipe.frame_shards = frame_shards
    lat = W.run_loop(pipe, F, CF, CO, STEPS, latent=latent, device="cpu", guidance_rescale=PHI, guidance_end=END)
    assert pipe.last_guidance["guided_steps"] == 3 and pipe.last_guidance["unguided_schedule"] is not None
    return lat, dict(pipe.last_schedule), dict(pipe.last_guidance)


def main(rank, frame_shards=None, latent=8):
    """One rank of loop_worker.spawn_gloo: this rank's final latents and its two schedules."""
    torch.set_num_threads(2)
    W.emulate_kernels()
    return run(frame_shards, latent)
