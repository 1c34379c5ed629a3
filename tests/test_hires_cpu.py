"""Two-pass (hi-res) sampling on the host: `hires_size` and its companions on VExpressPipeline.__call__ under emulated
kernels (loop_worker.emulate_kernels + the float32 stand-in of tests/resize_cases.py for ops.latent_resize) against the
restated chain of tests/hires_restated.py, the draw order and the seed rule, the audio prologue shared by the passes, the
untouched default path, the argument errors and two gloo ranks against one process."""
import pytest
import torch

import cases
import hires_restated as H
import hires_worker as HW
import loop_worker
from loop_worker import (SEED, call_pipeline, rel_l2, sampler_kw, scheduler, small_pipe, spawn_gloo,  # noqa: F401
                         trace_ops)


@pytest.fixture()
def emulated(monkeypatch):
    return HW.emulate(monkeypatch)


def _windows():
    from oracle import loop as OL
    return OL.uniform_windows(H.F, H.CF, H.CO)


def _spy_denoise(pipe, monkeypatch):
    """Records, per denoise call, (noise_seed, the N(0,1) tensor the pass started from, its number of timesteps)."""
    seen, orig = [], pipe.denoise

    def denoise(lat, kps, audio, timesteps, *a, **k):
        known = k.get("known")
        seen.append((k.get("noise_seed"), (lat if known is None else known[1]).clone(), len(timesteps)))
        return orig(lat, kps, audio, timesteps, *a, **k)
    monkeypatch.setattr(pipe, "denoise", denoise)
    return seen


# ------------------------------------------------------------------------------------------------ (1) the feature
@pytest.mark.parametrize("kind,mode", [("ddim", "bilinear"), ("ddim", "bicubic"), ("dpm", "bilinear"),
                                       ("euler-a", "bilinear")])
def test_pipeline_vs_the_restated_chain(emulated, small_pipe, kind, mode):
    """SMALL, F = 6, windows 4 / 2, 64 -> 128 pixels, 3 steps, then the last 3 of 5 at strength 0.6: the second pass's
    latents against restated loop -> float64 resize -> restated loop, by the bound of test_init_video_cpu.py's pipeline
    test (relL2 <= 5e-2); the first pass's latents are those of the plain call, bit for bit; Euler ancestral runs its
    second pass on noise_seed + 1.  Fails on a pipeline without the feature."""
    inp1, inp2 = H.inputs()
    kw = sampler_kw(kind)
    got = HW.call_hires(small_pipe, scheduler(kind), inp1, inp2, hires_mode=mode, **kw)
    last = small_pipe.last_hires
    assert got.shape == (1, 4, H.F, 16, 16) and torch.isfinite(got).all()
    assert {k: last[k] for k in ("base", "size", "mode", "steps", "begin_index")} == dict(
        base=(64, 64), size=(128, 128), mode=mode, steps=5, begin_index=2)
    assert last["events"] is None and small_pipe.last_init == dict(begin_index=2, masked=False, blend_launches=1)
    plain = call_pipeline(small_pipe, scheduler(kind), inp1, H.F, H.STEPS, H.CF, H.CO, **kw)
    assert small_pipe.last_hires is None and torch.equal(last["base_latents"], plain)
    with torch.no_grad():
        base, ref = H.chain(inp1, inp2, _windows(), cases.GUIDANCE, H.STEPS, H.HIRES_STEPS, H.STRENGTH, mode, kind,
                            seed=SEED if kind == "euler-a" else None)
    r_base, r = rel_l2(plain, base), rel_l2(got, ref)
    print(f"[__call__ hires {kind} {mode}, 64 -> 128 px, 3 + 3 of 5 steps, emulated kernels] relL2 vs the restated chain "
          f"{r:.4g} (first pass {r_base:.4g})")
    assert r_base <= 5e-2 and r <= 5e-2
    # the other resize mode gives another clip: the mode reaches the kernel
    if kind == "ddim" and mode == "bicubic":
        other = HW.call_hires(small_pipe, scheduler(kind), inp1, inp2)
        assert rel_l2(other, got) > 1e-4


def test_decode_returns_the_video_of_the_second_size(emulated, small_pipe):
    inp1, inp2 = H.inputs()
    video = HW.call_hires(small_pipe, scheduler("ddim"), inp1, inp2, steps=1, hires_steps=2, hires_strength=0.5,
                          decode=True, output_device=None)
    assert video.shape == (1, 3, H.F, 128, 128) and torch.isfinite(video).all()


# ------------------------------------------------------------------------------------------------ (2) draws and seeds
def test_draw_order_from_the_generator(emulated, small_pipe, monkeypatch):
    """DDIM with eta > 0 (ancestral, init_noise_sigma = 1) and nothing but a generator: pass-1 latents, pass-1 seed,
    pass-2 noise, pass-2 seed, in that order."""
    inp1, inp2 = H.inputs()
    seen = _spy_denoise(small_pipe, monkeypatch)
    HW.call_hires(small_pipe, scheduler("ddim-eta"), inp1, inp2, steps=1, hires_steps=2, hires_strength=0.5, eta=0.5,
                  latents=None, hires_noise=None, generator=torch.Generator().manual_seed(31))
    g = torch.Generator().manual_seed(31)
    lat1 = torch.randn(1, 4, H.F, 8, 8, generator=g)
    seed1 = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g))
    noise2 = torch.randn(1, 4, H.F, 16, 16, generator=g)
    seed2 = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=g))
    assert [(s, n) for s, _, n in seen] == [(seed1, 1), (seed2, 1)]
    assert torch.equal(seen[0][1], lat1) and torch.equal(seen[1][1], noise2)


def test_explicit_noise_seed_gives_the_second_pass_the_next_one(emulated, small_pipe, monkeypatch):
    inp1, inp2 = H.inputs()
    seen = _spy_denoise(small_pipe, monkeypatch)
    HW.call_hires(small_pipe, scheduler("euler-a"), inp1, inp2, steps=1, hires_steps=2, hires_strength=0.5,
                  noise_seed=SEED)
    assert [s for s, _, _ in seen] == [SEED, SEED + 1]
    assert torch.equal(seen[1][1], inp2["latents"])


def test_callback_index_runs_on_through_both_passes(emulated, small_pipe):
    inp1, inp2 = H.inputs()
    seen = []
    HW.call_hires(small_pipe, scheduler("ddim"), inp1, inp2, steps=2, hires_steps=4, hires_strength=0.5,
                  callback=lambda i, t, x: seen.append((i, tuple(x.shape[-2:]))), callback_steps=1)
    assert seen == [(0, (8, 8)), (1, (8, 8)), (2, (16, 16)), (3, (16, 16))]
    seen.clear()
    HW.call_hires(small_pipe, scheduler("ddim"), inp1, inp2, steps=2, hires_steps=4, hires_strength=0.5,
                  callback=lambda i, t, x: seen.append(i), callback_steps=3)
    assert seen == [0, 3]


# ------------------------------------------------------------------------------------------------ (3) the prologue
def test_audio_prologue_runs_once(emulated, small_pipe, monkeypatch):
    inp1, inp2 = H.inputs()
    calls = []

    def audio(waveform, video_length, pad, do_cfg):
        calls.append((waveform, video_length, pad, do_cfg))
        return inp1["audio_embeddings"]
    monkeypatch.setattr(small_pipe, "prepare_audio_embeddings", audio)
    got = HW.call_hires(small_pipe, scheduler("ddim"), inp1, inp2, steps=1, hires_steps=2, hires_strength=0.5,
                        audio_embeddings=None)
    assert calls == [(None, H.F, 2, True)]
    given = HW.call_hires(small_pipe, scheduler("ddim"), inp1, inp2, steps=1, hires_steps=2, hires_strength=0.5)
    assert len(calls) == 1 and torch.equal(got, given)


# ------------------------------------------------------------------------------------------------ (4) defaults
def test_without_hires_size_nothing_changes(emulated, small_pipe, monkeypatch):
    """hires_size=None: no resize launch, the launch list and the bits of a call without the keywords, last_hires None."""
    inp1, _ = H.inputs()
    trace = trace_ops(monkeypatch, emulated, loop_worker.LOOP_OPS + ("latent_resize",))
    plain = call_pipeline(small_pipe, scheduler("ddim"), inp1, H.F, 3, H.CF, H.CO)
    want, n = list(trace), len(trace)
    off = call_pipeline(small_pipe, scheduler("ddim"), inp1, H.F, 3, H.CF, H.CO, hires_size=None, hires_steps=7,
                        hires_strength=0.3, hires_mode="bicubic")
    assert small_pipe.last_hires is None
    assert trace[n:] == want and "latent_resize" not in trace and torch.equal(off, plain)
    del trace[:]
    HW.call_hires(small_pipe, scheduler("ddim"), *H.inputs(), steps=1, hires_steps=2, hires_strength=0.5)
    assert trace.count("latent_resize") == 1 and trace.count("known_blend") == 1
    assert trace.index("latent_resize") < trace.index("known_blend")
    assert small_pipe.last_hires is not None


# ------------------------------------------------------------------------------------------------ (5) errors
def test_bad_hires_arguments_fail_before_any_model_runs(emulated, small_pipe, monkeypatch):
    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "known_blend", "latent_resize", "overlap_ddim_step", "ncfhw_to_nhwc",
                 "groupnorm", "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)
    monkeypatch.setattr(small_pipe, "prepare_audio_embeddings", no_kernels)
    inp1, inp2 = H.inputs()
    init = torch.zeros(1, 4, H.F, 8, 8)
    bad = [
        dict(hires_size=(128, 100)),                                      # not a size width / height admit
        dict(hires_size=(0, 128)),
        dict(hires_size=(-128, 128)),
        dict(hires_size=128),
        dict(hires_size=(128.0, 128.0)),
        dict(hires_size=(128, 128, 128)),
        dict(hires_strength=0.0),
        dict(hires_strength=1.5),
        dict(hires_strength=-0.1),
        dict(hires_strength=float("nan")),
        dict(hires_steps=3, hires_strength=0.3),                          # int(3 * 0.3) == 0
        dict(hires_steps=0),
        dict(hires_steps=2.5),
        dict(init_latents=init),
        dict(init_latents=init, mask=torch.ones(1, 64, 64)),
        dict(init_video=torch.zeros(1, 3, H.F, 64, 64)),
        dict(hires_mode="nearest"),
        dict(hires_mode=None),
        dict(hires_noise=inp1["latents"]),                                # the first size's shape
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="hires|init|mask"):
            HW.call_hires(small_pipe, scheduler("ddim"), inp1, inp2, **kw)
    # features for the first size without their counterparts for the second
    common = dict(context_frames=H.CF, context_overlap=H.CO, audio_embeddings=inp1["audio_embeddings"],
                  latents=inp1["latents"], decode=False, hires_size=(128, 128))
    small_pipe.scheduler = scheduler("ddim")
    with pytest.raises(ValueError, match="hires_reference_latents"):
        small_pipe(None, None, None, 64, 64, H.F, 3, cases.GUIDANCE, reference_latents=inp1["ref_latents"],
                   kps_features=inp1["kps_features"], hires_kps_features=inp2["kps_features"], **common)
    with pytest.raises(ValueError, match="hires_kps_features"):
        small_pipe(None, None, None, 64, 64, H.F, 3, cases.GUIDANCE, reference_latents=inp1["ref_latents"],
                   kps_features=inp1["kps_features"], hires_reference_latents=inp2["ref_latents"], **common)
    # the hires_* tensors without hires_size
    for name, v in (("hires_noise", inp2["latents"]), ("hires_reference_latents", inp2["ref_latents"]),
                    ("hires_kps_features", inp2["kps_features"])):
        with pytest.raises(ValueError, match=name):
            call_pipeline(small_pipe, scheduler("ddim"), inp1, H.F, 3, H.CF, H.CO, **{name: v})


def test_pndm_cannot_start_inside_its_schedule(emulated, small_pipe, monkeypatch):
    import linear_multistep_worker as LMW

    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "ncfhw_to_nhwc", "groupnorm", "gemm", "latent_resize"):
        monkeypatch.setattr(emulated, name, no_kernels)
    inp1, inp2 = H.inputs()
    with pytest.raises(NotImplementedError):
        HW.call_hires(small_pipe, LMW.scheduler("pndm"), inp1, inp2)


def test_check_hires_reports_the_second_pass():
    from v_express_amd.pipeline import check_hires
    assert check_hires(None, None, 0.5, "bilinear", 25, 8) is None
    assert check_hires((768, 512), None, 0.5, "bicubic", 25, 8) == dict(size=(768, 512), steps=25, begin_index=13,
                                                                        mode="bicubic")
    assert check_hires((768, 768), 15, 1.0, "bilinear", 25, 8) == dict(size=(768, 768), steps=15, begin_index=0,
                                                                       mode="bilinear")


# ------------------------------------------------------------------------------------------------ (6) two ranks
def test_two_gloo_ranks_reach_one_result(emulated):
    """No generator, no noise tensors: each rank draws its own two N(0,1) tensors, rank 0's win in both passes and every
    rank resizes for itself, so two gloo ranks give the bits of one process seeded as rank 0."""
    ref, base, _, last = HW.run(rank=0)
    other, _, _, _ = HW.run(rank=1)
    assert not torch.equal(ref, other)                          # rank 1's own draws would give another clip
    results = spawn_gloo(HW.main, 2, timeout=900)
    for rank, (lat, base_r, sched, last_r) in enumerate(results):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))
        assert torch.equal(base_r, base) and last_r == last and sched["world"] == 2
