"""One rank of tests/test_linear_multistep_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising
loop with one of the linear multistep schedulers (Euler, LMS, PNDM) under emulated kernels (loop_worker.emulate_kernels +
linear_multistep_restated.overlap_linear_step)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import linear_multistep_restated as LM  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, four CFG units), 5 steps (LMS orders 1..4, 4; PNDM: six entries, every
# row of its table), 8x8 latents
F, CF, CO, STEPS, LATENT = 14, 8, 2, 5, 8


def scheduler(kind, **kw):
    from v_express_amd import EulerDiscreteScheduler, LMSDiscreteScheduler, PNDMScheduler
    extra = dict(skip_prk_steps=True) if kind == "pndm" else {}
    cls = {"euler": EulerDiscreteScheduler, "lms": LMSDiscreteScheduler, "pndm": PNDMScheduler}[kind]
    return cls(**{**LM.KWARGS, **extra, **kw})


def emulate(patch=W._Setattr):
    """loop_worker.emulate_kernels plus the stand-in for ops.overlap_linear_step."""
    ops = W.emulate_kernels(patch)
    patch.setattr(ops, "overlap_linear_step", LM.overlap_linear_step)
    return ops


def run(kind):
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = scheduler(kind)
    return W.run_loop(pipe, F, CF, CO, STEPS, latent=LATENT, device="cpu")


def main(rank, kind):
    """One rank of loop_worker.spawn_gloo: this rank's final latents."""
    torch.set_num_threads(2)
    emulate()
    return run(kind)
