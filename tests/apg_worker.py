"""One rank of tests/test_apg_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop (DDIM)
with adaptive projected guidance, three rows per window and a guidance interval, under emulated kernels
(loop_worker.emulate_kernels + apg_restated.guidance_apg)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import apg_restated as AP  # noqa: E402
import guidance_restated as G  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, six units), 5 DDIM steps of which 3 are guided
F, CF, CO, STEPS, END, S_AUDIO = 14, 8, 2, 5, 0.6, 6.0
APG = (0.0, 1.0, -0.5)


def emulate(patch=W._Setattr):
    """loop_worker.emulate_kernels plus the stand-in for ops.guidance_apg."""
    ops = W.emulate_kernels(patch)
    patch.setattr(ops, "guidance_apg", AP.guidance_apg)
    return ops


def run(frame_shards=None, latent=8):
    from v_express_amd import DDIMScheduler
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = DDIMScheduler(**G.KWARGS)
    pipe.frame_shards = frame_shards
    lat = W.run_loop(pipe, F, CF, CO, STEPS, latent=latent, device="cpu", guidance_end=END, audio_guidance_scale=S_AUDIO,
                     apg=APG)
    assert pipe.last_guidance["guided_steps"] == 3 and pipe.last_guidance["rows"] == ("u", "m", "c")
    return lat, dict(pipe.last_schedule), dict(pipe.last_guidance)


def main(rank, frame_shards=None, latent=8):
    """One rank of loop_worker.spawn_gloo: this rank's final latents and its two schedules."""
    torch.set_num_threads(2)
    emulate()
    return run(frame_shards, latent)
