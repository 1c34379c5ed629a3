"""Launch-trace recorder of the denoising loop (TEST INFRASTRUCTURE): runs `VExpressPipeline.__call__` on the small
configuration under emulated kernels (loop_worker.emulate_kernels) and writes down, in order, every
loop launch it issues - the `ops` wrappers of OPS, `unet.forward_tokens` and `dist.all_gather_units` - with the shape and
dtype of every tensor argument, every int / bool / str / None / float argument, small int32 tensors (terms, frame ids,
unit index) by value, and the four `last_*` reports of the call.  tests/test_loop_trace_cpu.py compares a fresh record
with tests/golden/denoise_launch_trace.json, which this file wrote at the commit before the loop was split into its
stitch / guidance / sampler / known parts:
    python tests/loop_trace.py tests/golden/denoise_launch_trace.json"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cases  # noqa: E402
import loop_worker  # noqa: E402

OPS = ("gather_latents", "pack_rows", "combine_units", "combine_units3", "guidance_rescale", "guidance_rescale3",
       "overlap_blend", "overlap_ddim_step", "overlap_multistep_step", "overlap_ancestral_step", "known_blend")

# latent 8 x 8, F = 7 in windows of 4 with overlap 2 under uniform_fit (starts 0, 1, 3: frame 3 lies in three windows),
# 3 steps, one rank
LATENT, F, CF, CO, STEPS, SEED = 8, 7, 4, 2, 3, 12345

# name -> (sampler, guidance_scale, audio_guidance_scale, guidance_rescale, guidance_end, overlap_blend, init);
# init: None, "mask" (init_latents + mask) or "strength" (init_latents, strength 0.67, no mask)
CASES = {
    "ddim": ("ddim", 3.5, None, 0.0, 1.0, "mean", None),
    "ddim_one_row": ("ddim", 1.0, None, 0.0, 1.0, "mean", None),
    "ddim_rescale_interval": ("ddim", 3.5, None, 0.7, 0.67, "mean", None),
    "ddim_never_guided": ("ddim", 3.5, None, 0.0, 0.0, "mean", None),
    "ddim_three_rows": ("ddim", 3.5, 6.0, 0.0, 1.0, "mean", None),
    "ddim_three_rows_rescale_interval_linear": ("ddim", 3.5, 6.0, 0.7, 0.67, "linear", None),
    "ddim_silent_and_full_rows_rescale": ("ddim", 1.0, 6.0, 0.7, 1.0, "mean", None),
    "ddim_eta": ("ddim-eta", 3.5, None, 0.0, 1.0, "mean", None),
    "euler_a_rescale_interval_pyramid_masked": ("euler-a", 3.5, None, 0.7, 0.67, "pyramid", "mask"),
    "dpm": ("dpm", 3.5, None, 0.0, 1.0, "mean", None),
    "dpm_three_rows_rescale_interval_linear_masked": ("dpm", 3.5, 6.0, 0.7, 0.67, "linear", "mask"),
    "ddim_init_strength": ("ddim", 3.5, None, 0.0, 1.0, "mean", "strength"),
    "ddim_init_masked": ("ddim", 3.5, None, 0.0, 1.0, "mean", "mask"),
}


def describe(v):
    """One argument as JSON data."""
    if isinstance(v, torch.Tensor):
        d = dict(shape=list(v.shape), dtype=str(v.dtype))
        if v.dtype == torch.int32 and v.numel() <= 512:
            d["values"] = v.reshape(-1).tolist()
        return d
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return dict(float=v)
    if isinstance(v, (list, tuple)):
        return [describe(x) for x in v]
    if isinstance(v, dict):
        return {str(k): describe(x) for k, x in v.items()}
    return dict(object=type(v).__name__)


def record_case(pipe, patch, name):
    """The launches of one case of CASES, in order, and the reports it leaves; `patch.setattr` installs the wrappers (and,
    for a monkeypatch, takes them off again)."""
    from v_express_amd import ops, synth
    sampler, s, s_a, phi, end, blend, init = CASES[name]
    calls, wrapped = [], []

    def wrap(obj, attr, label):
        orig = getattr(obj, attr)

        def traced(*a, **k):
            calls.append(dict(op=label, args=describe(a), kwargs=describe(dict(sorted(k.items())))))
            return orig(*a, **k)
        wrapped.append((obj, attr, orig))
        patch.setattr(obj, attr, traced)
    for op in OPS:
        wrap(ops, op, op)
    wrap(pipe.denoising_unet, "forward_tokens", "unet.forward_tokens")
    wrap(pipe.dist, "all_gather_units", "dist.all_gather_units")
    pipe.scheduler = loop_worker.scheduler(sampler)
    inp = synth.synthetic_inputs(cases.unet_cfg(cases.SMALL), F, LATENT, LATENT)
    rows = slice(0, 2) if s > 1.0 or (s_a is not None and s_a > 1.0) else slice(1, 2)    # one conditioning row
    kw = {}
    if init is not None:
        kw["init_latents"] = 0.5 * torch.randn(1, 4, F, LATENT, LATENT, generator=torch.Generator().manual_seed(77))
        if init == "mask":
            mask = torch.ones(F, 1, 8 * LATENT, 8 * LATENT)
            mask[:2] = 0.0
            mask[:, :, :4 * LATENT - 4] = 0.0
            kw["mask"] = mask
        else:
            kw["strength"] = 0.67
    if sampler == "ddim-eta":
        kw["eta"] = 1.0
    if s_a is not None:
        kw["audio_guidance_scale"] = s_a
    try:
        pipe(None, None, None, 8 * LATENT, 8 * LATENT, F, STEPS, s, context_schedule="uniform_fit", context_frames=CF,
             context_overlap=CO, reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD,
             reference_latents=inp["ref_latents"], kps_features=inp["kps_features"][rows],
             audio_embeddings=inp["audio_embeddings"][rows], latents=inp["latents"], noise_seed=SEED, decode=False,
             guidance_rescale=phi, guidance_end=end, overlap_blend=blend, **kw)
    finally:
        for obj, attr, orig in wrapped:
            patch.setattr(obj, attr, orig)
    last = dict(schedule=pipe.last_schedule, guidance=pipe.last_guidance, init=pipe.last_init,
                overlap=pipe.last_overlap)
    return dict(calls=calls, last=describe(last))


def record(patch, pipe=None, names=None):
    """name -> record_case of every case, as it comes back from a JSON file (tuples are lists there)."""
    pipe = pipe or loop_worker.build_pipeline("cpu")
    loop_worker.emulate_kernels(patch)
    out = {name: record_case(pipe, patch, name) for name in names or CASES}
    return json.loads(json.dumps(out))


if __name__ == "__main__":
    torch.set_num_threads(4)
    trace = record(loop_worker._Setattr)
    with open(sys.argv[1], "w") as fh:
        json.dump(trace, fh, separators=(",", ":"))
        fh.write("\n")
    print({k: len(v["calls"]) for k, v in trace.items()})
