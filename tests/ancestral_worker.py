"""One rank of tests/test_ancestral_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop
with Euler ancestral sampling under emulated kernels (loop_worker.emulate_kernels)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import ancestral_restated as A  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, four CFG units), 3 Euler ancestral steps, 8x8 latents
F, CF, CO, STEPS, LATENT, SEED = 14, 8, 2, 3, 8, (7 << 40) | 12345


def run():
    from v_express_amd import EulerAncestralDiscreteScheduler
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = EulerAncestralDiscreteScheduler(**A.KWARGS)
    return W.run_loop(pipe, F, CF, CO, STEPS, latent=LATENT, device="cpu", noise_seed=SEED)


def main(rank):
    """One rank of loop_worker.spawn_gloo: this rank's final latents."""
    torch.set_num_threads(2)
    W.emulate_kernels()
    return run()
