"""One rank of tests/test_ancestral_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop
with Euler ancestral sampling under emulated kernels (tests/fake_ops.py + ancestral_restated.overlap_ancestral_step)."""
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
