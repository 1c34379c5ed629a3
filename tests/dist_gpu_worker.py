"""torch.distributed.run worker for tests/test_gpu_models.py: the small-config denoising loop with the ranks folded onto
ONE GPU (VX_DIST_BACKEND=gloo: collectives staged through the host) - exercises the real process groups, the
frame-shard all-to-alls inside the motion modules and the unit gather.  Rank 0 saves the final latents.
usage: dist_gpu_worker.py OUT.pt F CONTEXT OVERLAP STEPS FRAME_SHARDS(0 = automatic)"""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from loop_worker import build_pipeline, emulate_kernels, force_round4_paths, run_loop  # noqa: E402,F401


def run(F, cf, co, steps, frame_shards, latent=16, device="cuda"):
    pipe = build_pipeline(device)
    return _run(pipe, pipe.denoising_unet, pipe.reference_net, pipe.scheduler, None, F, cf, co, steps, frame_shards,
                latent, device)


def _run(pipe, unet, refnet, sched, cfg, F, cf, co, steps, frame_shards, latent, device):
    """(unet, refnet, sched and cfg are the pipeline's own: kept for the callers that pass them)"""
    pipe.frame_shards = frame_shards or None
    return run_loop(pipe, F, cf, co, steps, latent=latent, device=device)


def main():
    out, F, cf, co, steps, S = sys.argv[1], *map(int, sys.argv[2:7])
    dist.init_process_group(os.environ.get("VX_DIST_BACKEND", "gloo"))
    torch.cuda.set_device(0)
    lat = run(F, cf, co, steps, S)
    if dist.get_rank() == 0:
        torch.save(lat, out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
