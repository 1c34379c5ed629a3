"""What the hi-res tests share and one rank of tests/test_hires_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE):
loop_worker.emulate_kernels plus the float32 stand-in of tests/resize_cases.py for ops.latent_resize, and
VExpressPipeline.__call__ with `hires_size` on the small configuration."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import cases  # noqa: E402
import hires_restated as H  # noqa: E402
import resize_cases as RC  # noqa: E402

SEED0 = 977


def emulate(patch=W._Setattr):
    """loop_worker.emulate_kernels plus the stand-in for the latent resize."""
    ops = W.emulate_kernels(patch)
    patch.setattr(ops, "latent_resize", RC.latent_resize)
    return ops


def call_hires(pipe, sched, inp1, inp2, F_=H.F, steps=H.STEPS, cf=H.CF, co=H.CO, **kw):
    """`pipe.__call__` from the first size's inputs to the second's: features for both sizes, inp1's latents and inp2's
    latents as the two N(0,1) tensors unless the caller passes its own (None: drawn), the hi-res defaults of
    hires_restated.  Returns what the pipeline returns (decode=False unless asked)."""
    px, px2 = 8 * inp1["latents"].shape[-1], 8 * inp2["latents"].shape[-1]
    pipe.scheduler = sched
    kw.setdefault("latents", inp1["latents"])
    kw.setdefault("hires_noise", inp2["latents"])
    kw.setdefault("decode", False)
    kw.setdefault("hires_size", (px2, px2))
    kw.setdefault("hires_steps", H.HIRES_STEPS)
    kw.setdefault("hires_strength", H.STRENGTH)
    kw.setdefault("audio_embeddings", inp1["audio_embeddings"])
    return pipe(None, None, None, px, px, F_, steps, cases.GUIDANCE, context_frames=cf, context_overlap=co,
                reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD,
                reference_latents=inp1["ref_latents"], kps_features=inp1["kps_features"],
                hires_reference_latents=inp2["ref_latents"], hires_kps_features=inp2["kps_features"], **kw)


def run(rank=0):
    """The hi-res clip of one rank: 2 steps, then the last of 2 at strength 0.5; no generator and no noise tensors are
    passed, so every rank draws both N(0,1) tensors from its own, differently seeded global generator."""
    from v_express_amd import DDIMScheduler
    import init_video_restated as R
    pipe = W.build_pipeline("cpu")
    inp1, inp2 = H.inputs()
    torch.manual_seed(SEED0 + rank)
    lat = call_hires(pipe, DDIMScheduler(**R.KWARGS), inp1, inp2, steps=2, hires_steps=2, hires_strength=0.5,
                     latents=None, hires_noise=None)
    last = {k: v for k, v in pipe.last_hires.items() if k not in ("base_latents", "events")}
    return lat, pipe.last_hires["base_latents"], dict(pipe.last_schedule), last


def main(rank):
    """One rank of loop_worker.spawn_gloo."""
    torch.set_num_threads(2)
    emulate()
    return run(rank)
