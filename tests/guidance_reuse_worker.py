"""One rank of tests/test_guidance_reuse_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop
(DDIM) with guidance reuse under emulated kernels (loop_worker.emulate_kernels + the stand-ins of
guidance_reuse_restated.py for ops.combine_units_keep / ops.combine_reused)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import guidance_reuse_restated as GR  # noqa: E402
import guidance_restated as G  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows), 5 DDIM steps, refresh period 2: refreshes at steps 0, 2, 4
F, CF, CO, STEPS, K, S_AUDIO = 14, 8, 2, 5, 2, 6.0
NEW_OPS = ("combine_units_keep", "combine_reused")


def emulate(patch=W._Setattr):
    """loop_worker.emulate_kernels plus the stand-ins for the two guidance-reuse ops."""
    ops = W.emulate_kernels(patch)
    patch.setattr(ops, "combine_units_keep", GR.combine_units_keep)
    patch.setattr(ops, "combine_reused", GR.combine_reused)
    return ops


def run(frame_shards=None, latent=8, s_a=None, mode="linear", pipe=None, **kw):
    from v_express_amd import DDIMScheduler
    pipe = pipe or W.build_pipeline("cpu")
    pipe.scheduler = DDIMScheduler(**G.KWARGS)
    pipe.frame_shards = frame_shards
    audio = {} if s_a is None else dict(audio_guidance_scale=s_a)
    kw.setdefault("guidance_refresh", K)
    lat = W.run_loop(pipe, F, CF, CO, STEPS, latent=latent, device="cpu", guidance_reuse=mode, **audio, **kw)
    return lat, dict(pipe.last_schedule), dict(pipe.last_guidance)


def main(rank, frame_shards=None, latent=8, s_a=S_AUDIO):
    """One rank of loop_worker.spawn_gloo: this rank's final latents and its two reports."""
    torch.set_num_threads(2)
    emulate()
    return run(frame_shards, latent, s_a)
