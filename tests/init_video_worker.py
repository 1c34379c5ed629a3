"""One rank of tests/test_init_video_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): VExpressPipeline.__call__ on the
small configuration with init latents, a mask and strength < 1 under emulated kernels (loop_worker.emulate_kernels).
No generator and no `latents` are passed: every rank draws its own noise from a differently seeded global generator, so
the result is one process's only if rank 0's noise reaches every rank."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import cases  # noqa: E402
import init_video_restated as R  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, four CFG units), the last 3 of 5 DDIM steps
F, CF, CO, STEPS, STRENGTH, SEED0 = 14, 8, 2, 5, 0.6, 4321


def inputs(latent):
    """(synthetic inputs, init latents, pixel mask [F, 1, H, W]): frames 0-1 kept whole, the upper part of the others
    kept, with a pixel edge inside a latent row (a soft latent edge)."""
    from v_express_amd import synth
    inp = synth.synthetic_inputs(cases.unet_cfg(cases.SMALL), F, latent, latent)
    g = torch.Generator().manual_seed(77)
    init = 0.5 * torch.randn(1, 4, F, latent, latent, generator=g)
    mask = torch.ones(F, 1, 8 * latent, 8 * latent)
    mask[:2] = 0.0
    mask[:, :, :4 * latent - 4] = 0.0
    return inp, init, mask


def run(frame_shards=None, latent=8, rank=0):
    from v_express_amd import DDIMScheduler
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = DDIMScheduler(**R.KWARGS)
    pipe.frame_shards = frame_shards
    inp, init, mask = inputs(latent)
    torch.manual_seed(SEED0 + rank)                     # the noise is drawn from the global generator
    lat = pipe(None, None, None, 8 * latent, 8 * latent, F, STEPS, cases.GUIDANCE, strength=STRENGTH,
               context_frames=CF, context_overlap=CO, reference_attention_weight=cases.W_REF,
               audio_attention_weight=cases.W_AUD, reference_latents=inp["ref_latents"],
               kps_features=inp["kps_features"], audio_embeddings=inp["audio_embeddings"], decode=False,
               init_latents=init, mask=mask)
    assert pipe.last_init == dict(begin_index=2, masked=True, blend_launches=4)
    return lat, dict(pipe.last_schedule), dict(pipe.last_init)


def main(rank, frame_shards=None, latent=8):
    """One rank of loop_worker.spawn_gloo: this rank's final latents, its schedule and last_init."""
    torch.set_num_threads(2)
    W.emulate_kernels()
    return run(frame_shards, latent, rank)
