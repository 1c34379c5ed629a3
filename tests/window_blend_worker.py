"""One rank of the two-rank run of tests/test_window_blend_cpu.py (gloo, emulated kernels) (TEST INFRASTRUCTURE): the
small-config denoising loop (DDIM) over the even-fit windows of F = 7 (windows of 4, overlap 2: starts 0, 1, 3, so frame 3
lies in three windows) with the "linear" blend."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import guidance_restated as G  # noqa: E402

F, CF, CO, STEPS, BLEND = 7, 4, 2, 2, "linear"


def run(latent=8, device="cpu", blend=BLEND):
    from v_express_amd import DDIMScheduler
    from v_express_amd.context import get_context_scheduler
    assert [w[0] for w in get_context_scheduler("uniform_fit")(step=0, num_frames=F, context_size=CF, context_stride=1,
                                                               context_overlap=CO, closed_loop=False)] == [0, 1, 3]
    pipe = W.build_pipeline(device)
    pipe.scheduler = DDIMScheduler(**G.KWARGS)
    pipe.frame_shards = 1
    lat = W.run_loop(pipe, F, CF, CO, STEPS, schedule="uniform_fit", latent=latent, device=device, overlap_blend=blend)
    return lat, dict(pipe.last_schedule), dict(pipe.last_overlap)


def main(rank, latent=8):
    """CPU, one rank of loop_worker.spawn_gloo: this rank's final latents and its two reports."""
    torch.set_num_threads(2)
    W.emulate_kernels()
    return run(latent)
