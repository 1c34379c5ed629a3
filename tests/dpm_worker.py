"""One rank of tests/test_dpm_solver_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop
with a DPM-Solver++ scheduler under emulated kernels (loop_worker.emulate_kernels)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import dpm_restated as D  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, four CFG units), 3 DPM++ 2M steps (orders 1, 2, 1), 8x8 latents
F, CF, CO, STEPS, LATENT = 14, 8, 2, 3, 8


def run():
    from v_express_amd import DPMSolverMultistepScheduler
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = DPMSolverMultistepScheduler(**D.KWARGS)
    return W.run_loop(pipe, F, CF, CO, STEPS, latent=LATENT, device="cpu")


def main(rank):
    """One rank of loop_worker.spawn_gloo: this rank's final latents."""
    torch.set_num_threads(2)
    W.emulate_kernels()
    return run()
