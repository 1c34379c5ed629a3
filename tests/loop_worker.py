"""What the loop tests and their workers share (TEST INFRASTRUCTURE): the kernel emulation of the CPU suite, the
small-config pipeline and the ways to drive it, the oracle UNet of tests/loop_restated.py, the gloo spawn of the
multi-rank tests and the fixtures of both suites.  Test files import the fixtures by name
(`from loop_worker import emulated, small_pipe  # noqa: F401`)."""
import os
import socket
import sys
from contextlib import contextmanager

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import cases  # noqa: E402

SEED = (0x9E3779B9 << 32) | 0x7F4A7C15
UPDATES = ("overlap_ddim_step", "overlap_multistep_step", "overlap_ancestral_step")
LOOP_OPS = ("gather_latents", "pack_rows", "combine_units", "guidance_rescale", "combine_units3", "guidance_rescale3",
            "overlap_blend", "known_blend") + UPDATES


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def cosine(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-300)).item()


# ------------------------------------------------------------------------------------------------ the emulation
class _Setattr:
    setattr = staticmethod(setattr)


def emulate_kernels(patch=_Setattr):
    """CPU suite only, and its only way in: tests/fake_ops.py stands in for the HIP wrappers, the *_restated.py stand-ins
    for the loop kernels fake_ops does not have, and the device guards are lifted, so the whole host side (models, loop,
    sharding) runs in a process without a GPU.  `patch`: anything with a pytest monkeypatch's setattr; by default the
    replacements stay for the life of the process (a spawned worker)."""
    import ancestral_restated as A
    import audio_guidance_restated as AG
    import dpm_restated as D
    import fake_ops
    import guidance_restated as G
    import init_video_restated as R
    import window_blend_restated as WB
    from v_express_amd import ops, prologue, unet_3d, vae
    fake_ops.install(patch, ops)
    for name, fn in (("overlap_ancestral_step", A.overlap_ancestral_step), ("guidance_rescale", G.guidance_rescale),
                     ("overlap_multistep_step", D.overlap_multistep_step), ("known_blend", R.known_blend),
                     ("combine_units3", AG.combine_units3), ("guidance_rescale3", AG.guidance_rescale3),
                     ("overlap_blend", WB.overlap_blend), ("_PADDED", {})):
        patch.setattr(ops, name, fn)
    for cls in (unet_3d._UNetBase, vae.AutoencoderKLDecoder, prologue._Module):
        patch.setattr(cls, "_need_gpu", lambda self: None)
    if os.environ.get("VX_TEST_FORCE_ROUND4") == "1":
        force_round4_paths(ops, patch.setattr)
    return ops


@pytest.fixture()
def emulated(monkeypatch):
    return emulate_kernels(monkeypatch)


def force_round4_paths(ops, patch=setattr):
    """The round-4 host paths at the small widths of the CPU models, where the routing rules would not pick them: every
    temporal attention block as ONE `ops.tblock_fused` call (also in the pixel-shard layout of a frame-sharded unit), row
    statistics as two-part sums ([rows, 4] buffers) at every width."""
    patch(ops, "tblock_fused_applies", lambda c, heads, f, hw: True)
    patch(ops, "STATS_PARTS_WIDTHS", set(range(8, 4096, 8)))


def build_pipeline(device):
    """The small-config pipeline (UNet3D + ReferenceNet + VAE decoder, seeded synthetic weights)."""
    from v_express_amd import (AutoencoderKLDecoder, DDIMScheduler, UNet2DConditionModel, UNet3DConditionModel,
                               VExpressPipeline, synth)
    cfg = cases.unet_cfg(cases.SMALL)
    vcfg = synth.VaeConfig(**cases.SMALL_VAE)
    unet = UNet3DConditionModel(cfg).to(device)
    refnet = UNet2DConditionModel(cfg).to(device)
    unet.load_state_dict(synth.unet3d_state_dict(cfg), strict=True)
    refnet.load_state_dict(synth.refnet_state_dict(cfg), strict=True)
    vae = AutoencoderKLDecoder(vcfg).to(device)
    vae.load_state_dict(synth.vae_decoder_state_dict(vcfg))
    sched = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False,
                          steps_offset=1, prediction_type="v_prediction", rescale_betas_zero_snr=True,
                          timestep_spacing="trailing")
    return VExpressPipeline(vae=vae, reference_net=refnet, denoising_unet=unet, scheduler=sched)


def run_loop(pipe, F, context, overlap, steps, *, schedule="uniform", latent, device, **loop_kwargs):
    """The denoising loop of `pipe` (its scheduler, `steps` timesteps) on the seeded synthetic clip of F frames of
    latent x latent, windows of `context` frames: the pieces of VExpressPipeline.__call__ in its order, then
    `pipe.denoise(..., **loop_kwargs)` on the windows themselves, so that a worker can reach every keyword of the loop
    (last_overlap's schedule stays None).  Returns the final latents on the CPU."""
    from v_express_amd import ReferenceAttentionControl, ops, synth
    from v_express_amd.context import get_context_scheduler
    cfg = cases.unet_cfg(cases.SMALL)
    unet, refnet, sched = pipe.denoising_unet, pipe.reference_net, pipe.scheduler
    inp = synth.synthetic_inputs(cfg, F, latent, latent, device=device)
    writer = ReferenceAttentionControl(refnet, do_classifier_free_guidance=True, mode="write", fusion_blocks="full")
    reader = ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", fusion_blocks="full",
                                       reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD)
    refnet(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768, device=device),
           return_dict=False)
    reader.update(writer, True, dtype=unet.dtype)
    sched.set_timesteps(steps)
    windows = list(get_context_scheduler(schedule)(step=0, num_frames=F, context_size=context, context_stride=1,
                                                   context_overlap=overlap, closed_loop=False))
    c0 = cfg.block_out_channels[0]
    kps = ops.ncfhw_to_nhwc(inp["kps_features"], c0).view(2, F, latent * latent, c0)
    audio = inp["audio_embeddings"].to(torch.bfloat16).contiguous()
    lat = inp["latents"].clone().float() * sched.init_noise_sigma        # (1 but for Euler ancestral)
    pipe.denoise(lat, kps, audio, sched.timesteps.tolist(), windows, cases.GUIDANCE, **loop_kwargs)
    return lat.cpu()


# ------------------------------------------------------------------------------------------------ __call__
@pytest.fixture(scope="module")
def small_pipe():
    return build_pipeline("cpu")


def scheduler(kind):
    from dpm_restated import KWARGS
    from v_express_amd import DDIMScheduler, DPMSolverMultistepScheduler, EulerAncestralDiscreteScheduler
    return {"ddim": DDIMScheduler, "ddim-eta": DDIMScheduler, "dpm": DPMSolverMultistepScheduler,
            "euler-a": EulerAncestralDiscreteScheduler}[kind](**KWARGS)


def sampler_kw(kind, eta=1.0):
    kw = dict(eta=eta if kind == "ddim-eta" else 0.0)
    if kind in ("ddim-eta", "euler-a"):
        kw["noise_seed"] = SEED
    return kw


def call_pipeline(pipe, sched, inp, F_, steps, cf, co, guidance=cases.GUIDANCE, **kw):
    """`pipe.__call__` with `sched` on the synthetic inputs `inp` (64 x 64 pixels, latents 8 x 8): the final latents."""
    pipe.scheduler = sched
    kw.setdefault("latents", inp["latents"])
    kw.setdefault("decode", False)
    return pipe(None, None, None, 64, 64, F_, steps, guidance, context_frames=cf, context_overlap=co,
                reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD,
                reference_latents=inp["ref_latents"], kps_features=inp["kps_features"],
                audio_embeddings=inp["audio_embeddings"], **kw)


_INPUTS = {}


def inputs(F_):
    """synth.synthetic_inputs of the small configuration, F_ frames of 8 x 8 latents (CPU; drawn once per length)."""
    from v_express_amd import synth
    if F_ not in _INPUTS:
        _INPUTS[F_] = synth.synthetic_inputs(cases.unet_cfg(cases.SMALL), F_, 8, 8)
    return _INPUTS[F_]


def oracle_unet(inp):
    """The `unet_fn` of loop_restated.restated_loop over the small configuration's weights and inp's reference latents."""
    from loop_restated import oracle_rows_unet
    from v_express_amd import synth
    cfg, ocfg = cases.unet_cfg(cases.SMALL), cases.oracle_cfg(cases.SMALL)
    return oracle_rows_unet(synth.unet3d_state_dict(cfg), synth.refnet_state_dict(cfg), ocfg, inp["ref_latents"],
                            cases.W_REF, cases.W_AUD)


def trace_ops(monkeypatch, ops, names=LOOP_OPS):
    """Records the names of the loop's ops as they are called."""
    trace = []
    for name in names:
        def wrap(*a, _fn=getattr(ops, name), _name=name, **k):
            trace.append(_name)
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, wrap)
    return trace


# ------------------------------------------------------------------------------------------------ gloo ranks
def _by_value(v, to_numpy):
    """Tensors <-> numpy arrays through tuples.  Results cross the queue BY VALUE (numpy arrays are pickled into it): a
    torch tensor travels as a file descriptor that the parent must fetch from the child while it is still alive - on a
    busy machine the child was gone first (EOFError in q.get)."""
    if isinstance(v, tuple):
        return tuple(_by_value(x, to_numpy) for x in v)
    if to_numpy and isinstance(v, torch.Tensor):
        return v.numpy().copy()
    if not to_numpy and type(v).__module__ == "numpy":
        return torch.from_numpy(v)
    return v


def _gloo_rank(rank, world, port, q, target, args):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, _by_value(target(rank, *args), True)))
    dist.barrier()
    dist.destroy_process_group()


def spawn_gloo(target, world, *args, timeout=600, join=120):
    """`target(rank, *args)` in `world` spawned processes with a gloo process group up: what each returned (tensors,
    possibly in tuples, with anything picklable), ordered by rank.  Every exit code must be 0."""
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_gloo_rank, args=(r, world, port, q, target, args)) for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=timeout) for _ in procs)
    for p in procs:
        p.join(timeout=join)
        assert p.exitcode == 0
    assert sorted(results) == list(range(world))
    return [_by_value(results[r], False) for r in range(world)]


# ------------------------------------------------------------------------------------------------ the GPU suite
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)
    return "cuda"


def build_small(dev, case="reflected_F11_c4o2"):
    """The small pipeline on the device with the geometry and CPU inputs of cases.PIPELINE_CASES[case], the state dicts
    and oracle config, and the oracle UNet of loop_restated over them."""
    from v_express_amd import synth
    F_, cf, co, _ = cases.PIPELINE_CASES[case]
    cfg = cases.unet_cfg(cases.SMALL)
    return dict(pipe=build_pipeline(dev), inp=inputs(F_), F=F_, cf=cf, co=co, cfg=cfg,
                ocfg=cases.oracle_cfg(cases.SMALL), sd3=synth.unet3d_state_dict(cfg), sd2=synth.refnet_state_dict(cfg),
                oracle=oracle_unet(inputs(F_)))


@pytest.fixture(scope="module")
def small(dev):
    return build_small(dev)


def call_small(S, sched, steps, inp=None, guidance=cases.GUIDANCE, **kw):
    """call_pipeline on build_small's pipeline and geometry (`inp`: other inputs of the same length), on the CPU."""
    return call_pipeline(S["pipe"], sched, inp or S["inp"], S["F"], steps, S["cf"], S["co"], guidance, **kw).cpu()


@contextmanager
def oracle_on_cpu():
    """The float64 reference of a GPU test: no autograd, at most 16 threads."""
    nthreads = torch.get_num_threads()
    torch.set_num_threads(min(16, nthreads))
    try:
        with torch.no_grad():
            yield
    finally:
        torch.set_num_threads(nthreads)
