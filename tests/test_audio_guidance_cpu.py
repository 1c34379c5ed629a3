"""A separate audio guidance scale on the host: `audio_guidance_scale` of VExpressPipeline under emulated kernels
(tests/fake_ops.py + guidance_restated.guidance_rescale + audio_guidance_restated.combine_units3 / guidance_rescale3)
against float64 restatements over the oracle UNet: three rows per window (u, m, c), the (m, c) route of
guidance_scale <= 1, the defaults bit for bit, an all-zero audio row, every sampler with the rescale and a guidance
interval, init-video sampling, the argument errors (the C entry points' included), the unit schedules for three rows and
two gloo ranks against one process."""
import ctypes
import pytest
import torch

import audio_guidance_restated as AG
import cases
from loop_restated import restated_loop
from loop_worker import (SEED, call_pipeline as _call, emulated, inputs as _inputs,  # noqa: F401
                         oracle_unet as _oracle_unet, rel_l2, scheduler, small_pipe, spawn_gloo, trace_ops as _trace)

PHI, S, S_A = 0.7, cases.GUIDANCE, 6.0
BOUND = 5e-2        # the relative-L2 bound tests/test_guidance_cpu.py applies to the two-row loop at these geometries


# ------------------------------------------------------------------------------------------------ (1) three rows
def test_audio_scale_changes_the_clip_and_matches_the_restatement(emulated, small_pipe, monkeypatch):
    """Two windows (F = 6, windows of 4 with overlap 2), 3 DDIM steps, s = 3.5, s_a = 6: the latents differ from the
    s_a = None call, lie within the two-row loop's bound of the float64-combined three-row loop over the oracle UNet, and
    are strictly closer to it than the two-row clip.  Fails on a pipeline that ignores audio_guidance_scale."""
    from oracle import loop as OL
    F_, cf, co, steps = 6, 4, 2, 3
    inp = _inputs(F_)
    windows = OL.uniform_windows(F_, cf, co)
    assert len(windows) == 2
    plain = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co)
    assert "rows" not in small_pipe.last_guidance
    unet = small_pipe.denoising_unet
    calls = []
    orig = unet.forward_tokens

    def spy(x_in, t, *a, **k):
        calls.append((k["b"], list(k["batch_rows"]), list(k["audio_zero"])))
        return orig(x_in, t, *a, **k)
    monkeypatch.setattr(unet, "forward_tokens", spy)
    trace = _trace(monkeypatch, emulated)
    got = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, audio_guidance_scale=S_A)
    lg = small_pipe.last_guidance
    assert lg["rows"] == ("u", "m", "c") and lg["audio_scale"] == S_A and lg["guided_steps"] == steps
    assert small_pipe.last_schedule == dict(kind="whole units", frame_shards=1, mixed_shards=1, units=6, world=1)
    # one call per window (3 rows; a second window would make 6 > units_per_call = 4): bank rows (zero, ref, ref), audio
    # (zero, zero, real)
    assert calls == [(3, [0, 1, 1], [True, True, False])] * (2 * steps)
    assert trace.count("combine_units3") == steps and "combine_units" not in trace and "guidance_rescale3" not in trace
    assert torch.isfinite(got).all() and rel_l2(got, plain) > 1e-3
    with torch.no_grad():
        ref = restated_loop(_oracle_unet(inp), inp["latents"], windows, S, inp["kps_features"], inp["audio_embeddings"],
                            steps, "ddim", s_a=S_A)
    r, r2 = rel_l2(got, ref), rel_l2(plain, ref)
    print(f"[__call__ audio_guidance_scale={S_A}, guidance_scale={S}, emulated kernels, {steps} steps] relL2 vs restated "
          f"three-row loop {r:.4g}; the two-row clip {r2:.4g}")
    assert r <= BOUND and r < r2


# ------------------------------------------------------------------------------------------------ (2) defaults
def test_defaults_take_the_two_row_route_bit_for_bit(emulated, small_pipe, monkeypatch):
    F_, cf, co, steps = 6, 4, 2, 2
    inp = _inputs(F_)

    def boom(*a, **k):
        raise AssertionError("a three-row op ran")
    monkeypatch.setattr(emulated, "combine_units3", boom)
    monkeypatch.setattr(emulated, "guidance_rescale3", boom)
    plans = []
    orig = type(small_pipe)._unit_plan

    def counting(self, *a, **k):
        plans.append(a[-1])
        return orig(self, *a, **k)
    monkeypatch.setattr(type(small_pipe), "_unit_plan", counting)
    trace = _trace(monkeypatch, emulated)
    base = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co)
    base_trace = list(trace)
    assert plans == [[0, 1]] and base_trace.count("combine_units") == steps
    assert small_pipe.last_guidance == dict(guided_steps=steps, steps=steps, rescale=0.0, unguided_schedule=None)
    for kw, want in ((dict(audio_guidance_scale=None), {}), (dict(audio_guidance_scale=S), dict(rows=("u", "c"),
                                                                                                 audio_scale=S))):
        del trace[:], plans[:]
        same = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, **kw)
        assert plans == [[0, 1]] and trace == base_trace and torch.equal(base, same)
        assert small_pipe.last_guidance == dict(guided_steps=steps, steps=steps, rescale=0.0, unguided_schedule=None,
                                                **want)
    # with the rescale and an interval as well
    ctl = dict(guidance_rescale=PHI, guidance_end=0.5)
    del trace[:], plans[:]
    a = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, **ctl)
    a_trace, a_plans = list(trace), list(plans)
    del trace[:], plans[:]
    b = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, audio_guidance_scale=S, **ctl)
    assert a_plans == [[0, 1], [1]] == plans and trace == a_trace and torch.equal(a, b)
    # neither scale above 1: today's no-CFG route, one row of conditioning
    nocfg = cases.cond_only(inp)
    del plans[:]
    c = _call(small_pipe, scheduler("ddim"), nocfg, F_, steps, cf, co, guidance=1.0)
    d = _call(small_pipe, scheduler("ddim"), nocfg, F_, steps, cf, co, guidance=1.0, audio_guidance_scale=0.5)
    assert plans == [[0], [0]] and torch.equal(c, d) and small_pipe.last_guidance["rows"] == ("c",)


def test_row_table():
    from v_express_amd.pipeline import GUIDANCE_ROWS, guidance_rows
    assert GUIDANCE_ROWS == AG.ROWS
    for s in (0.0, 1.0, 1.5, 3.5):
        for s_a in (None, 0.0, 0.5, 1.0, 1.5, 3.5, 6.0):
            assert guidance_rows(s, s_a) == AG.rows_for(s, s_a), (s, s_a)
    assert guidance_rows(3.5, 6) == ("u", "m", "c") and guidance_rows(3.5, 0) == ("u", "m", "c")
    assert guidance_rows(1.0, 3.5) == ("m", "c") and guidance_rows(3.5, 3.5) == ("u", "c")
    assert guidance_rows(1.0, 1.0) == ("c",) and guidance_rows(0.5, 1.0) == ("c",)


# ------------------------------------------------------------------------------------------------ (3) rows (m, c)
def test_audio_scale_alone_runs_the_rows_m_c_through_the_two_row_ops(emulated, small_pipe, monkeypatch):
    """guidance_scale = 1, audio_guidance_scale = 3.5: g = m + s_a (c - m) through combine_units with guidance == s_a, the
    conditioning in the CFG layout (the prologue hooks asked for it); against the restated (m, c) loop."""
    from oracle import loop as OL
    F_, cf, co, steps = 6, 4, 2, 3
    inp = _inputs(F_)
    seen = []
    orig = emulated.combine_units

    def spy(gathered, uidx, c, f, hw, guidance, preds):
        seen.append((tuple(uidx.shape), guidance))
        return orig(gathered, uidx, c, f, hw, guidance, preds)
    monkeypatch.setattr(emulated, "combine_units", spy)
    trace = _trace(monkeypatch, emulated)
    unet = small_pipe.denoising_unet
    calls = []
    orig_ft = unet.forward_tokens

    def spy_ft(x_in, t, *a, **k):
        calls.append((list(k["batch_rows"]), list(k["audio_zero"])))
        return orig_ft(x_in, t, *a, **k)
    monkeypatch.setattr(unet, "forward_tokens", spy_ft)
    got = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, guidance=1.0, audio_guidance_scale=3.5)
    lg = small_pipe.last_guidance
    assert lg["rows"] == ("m", "c") and lg["audio_scale"] == 3.5 and lg["guided_steps"] == steps
    assert seen == [((2, 2, 1), 3.5)] * steps
    assert not {"combine_units3", "guidance_rescale3", "guidance_rescale"} & set(trace)
    # both windows in one call of 4 rows: every row reads the reference bank, the m rows carry zero audio
    assert calls == [([1, 1, 1, 1], [True, False, True, False])] * steps
    with torch.no_grad():
        ref = restated_loop(_oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), 1.0, inp["kps_features"],
                            inp["audio_embeddings"], steps, "ddim", s_a=3.5)
    nocfg = _call(small_pipe, scheduler("ddim"), cases.cond_only(inp), F_, steps, cf, co, guidance=1.0)
    r, r2 = rel_l2(got, ref), rel_l2(nocfg, ref)
    print(f"[__call__ guidance_scale=1, audio_guidance_scale=3.5, {steps} steps] relL2 vs restated (m, c) loop {r:.4g}; "
          f"the unguided clip {r2:.4g}")
    assert torch.isfinite(got).all() and r <= BOUND and r < r2
    # the silent row needs the zero-audio row of the CFG layout
    with pytest.raises(ValueError, match="audio_guidance_scale.*2 batch row"):
        _call(small_pipe, scheduler("ddim"), cases.cond_only(inp), F_, steps, cf, co, guidance=1.0,
              audio_guidance_scale=3.5)
    with pytest.raises(ValueError, match="audio_guidance_scale.*2 batch row"):
        _call(small_pipe, scheduler("ddim"), cases.cond_only(inp), F_, steps, cf, co, audio_guidance_scale=S_A)


def test_prologue_hooks_get_the_cfg_layout_when_either_scale_exceeds_one(emulated, small_pipe, monkeypatch):
    inp = _inputs(4)
    flags = []

    def kps_hook(kps_images, height, width, do_cfg):
        flags.append(("kps", do_cfg))
        return inp["kps_features"] if do_cfg else inp["kps_features"][1:]

    def audio_hook(audio_waveform, video_length, num_pad_audio_frames, do_cfg):
        flags.append(("audio", do_cfg))
        return inp["audio_embeddings"] if do_cfg else inp["audio_embeddings"][1:]
    monkeypatch.setattr(small_pipe, "prepare_kps_feature", kps_hook)
    monkeypatch.setattr(small_pipe, "prepare_audio_embeddings", audio_hook)
    small_pipe.scheduler = scheduler("ddim")
    for s, s_a, want in ((1.0, 3.5, True), (3.5, 6.0, True), (1.0, None, False), (1.0, 0.5, False), (0.5, 1.0, False)):
        del flags[:]
        small_pipe(None, None, None, 64, 64, 4, 1, s, context_frames=4, context_overlap=2,
                   reference_latents=inp["ref_latents"], latents=inp["latents"], decode=False, audio_guidance_scale=s_a)
        assert flags == [("kps", want), ("audio", want)], (s, s_a)


# ------------------------------------------------------------------------------------------------ (4) silent audio
@pytest.mark.parametrize("s_a", [0.0, 1.0, 6.0])
def test_all_zero_audio_makes_the_three_row_clip_the_two_row_clip(emulated, small_pipe, s_a):
    """With all-zero audio in the conditional row the silent row IS the conditional row (same bank, same keypoints, same
    route through the read transformer), c - m is +0 everywhere and the three-row clip equals the two-row clip at the same
    guidance_scale bit for bit, whatever the audio scale."""
    F_, cf, co, steps = 6, 4, 2, 2
    inp = _inputs(F_)
    inp = dict(inp, audio_embeddings=torch.zeros_like(inp["audio_embeddings"]))
    two = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co)
    three = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, audio_guidance_scale=s_a)
    assert small_pipe.last_guidance["rows"] == ("u", "m", "c")
    assert torch.isfinite(two).all() and torch.equal(two, three)
    a = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, guidance_rescale=PHI)
    b = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, guidance_rescale=PHI, audio_guidance_scale=s_a)
    assert torch.equal(a, b) and not torch.equal(a, two)


# ------------------------------------------------------------------------------------------------ (5) interplay
@pytest.mark.parametrize("kind", ["ddim", "ddim-eta", "dpm", "euler-a"])
def test_every_sampler_with_rescale_and_interval_vs_restated_loop(emulated, small_pipe, monkeypatch, kind):
    """Reflected last window [8, 9, 10, 9], 5 steps, s_a = 6, phi = 0.7, guidance_end = 0.6 (3 guided + 2 unguided steps):
    against the restated three-row loop; the unguided steps issue the ops of the ("c",) plan."""
    from oracle import loop as OL
    F_, cf, co, _ = cases.PIPELINE_CASES["reflected_F11_c4o2"]
    steps = 5
    inp = _inputs(F_)
    eta = 0.5 if kind == "ddim-eta" else 0.0
    kw = dict(noise_seed=SEED) if kind in ("ddim-eta", "euler-a") else {}
    unet = small_pipe.denoising_unet
    orig_ft = unet.forward_tokens
    trace = _trace(monkeypatch, emulated)

    def spy_ft(x_in, t, *a, **k):
        trace.append(("unet", tuple(k["batch_rows"]), tuple(k["audio_zero"])))
        return orig_ft(x_in, t, *a, **k)
    monkeypatch.setattr(unet, "forward_tokens", spy_ft)
    got = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, eta=eta, guidance_rescale=PHI, guidance_end=0.6,
                audio_guidance_scale=S_A, **kw)
    lg = small_pipe.last_guidance
    assert lg["guided_steps"] == 3 and lg["steps"] == 5 and lg["rows"] == ("u", "m", "c")
    nW = len(OL.uniform_windows(F_, cf, co))
    assert lg["unguided_schedule"]["units"] == nW and small_pipe.last_schedule["units"] == 3 * nW
    full = list(trace)
    # the ops of steps 3-4 are those of a two-row clip's unguided steps (the ("c",) plan)
    del trace[:]
    _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, eta=eta, guidance_rescale=PHI, guidance_end=0.6, **kw)
    two = list(trace)
    update = {"ddim": "overlap_ddim_step", "dpm": "overlap_multistep_step"}.get(kind, "overlap_ancestral_step")
    cut3, cut2 = [[i for i, n in enumerate(t) if n == update][2] + 1 for t in (full, two)]
    assert full[cut3:] == two[cut2:] and full[cut3:].count("combine_units") == 2
    assert ("unet", (1, 1, 1, 1), (False,) * 4) in full[cut3:] and ("unet", (1,), (False,)) in full[cut3:]
    assert full[:cut3].count("guidance_rescale3") == 3 and "combine_units" not in full[:cut3]
    with torch.no_grad():
        ref = restated_loop(_oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), S, inp["kps_features"],
                            inp["audio_embeddings"], steps, kind, s_a=S_A, phi=PHI, end=0.6, seed=SEED, eta=eta)
    r = rel_l2(got, ref)
    print(f"[__call__ {kind}, audio scale {S_A}, rescale {PHI}, guidance_end 0.6, reflected_F11_c4o2, {steps} steps] "
          f"relL2 vs restated loop {r:.4g}")
    assert torch.isfinite(got).all() and r <= BOUND


def test_emulated_rescale3_vs_float64(emulated):
    """The stand-in of the CPU suite holds the kernel's bound (4 x the float32 torch.std evaluation's error) and its two
    exact properties: phi = 0 is combine_units3, equal c and m rows give the two-row op."""
    g = torch.Generator().manual_seed(3)
    u = torch.randn(2, 4, 6, 80, generator=g) + 3.0
    m = u + 0.3 * torch.randn(2, 4, 6, 80, generator=g)
    c = m + 0.3 * torch.randn(2, 4, 6, 80, generator=g)
    gathered = torch.stack([x[w].permute(1, 2, 0).reshape(6 * 80, 4) for w in range(2) for x in (u, m, c)])
    uidx = torch.arange(6, dtype=torch.int32).view(2, 3, 1)
    ws = torch.full((2 * 6 * 6,), float("nan"))
    got, plain, zero = torch.empty(2, 4, 6, 80), torch.empty(2, 4, 6, 80), torch.empty(2, 4, 6, 80)
    AG.guidance_rescale3(gathered, uidx, 4, 6, 80, S, S_A, PHI, ws, got)
    base = AG.float32_baseline_error3(u, m, c, S, S_A, PHI)
    assert (got.double() - AG.combine3_rescaled(u, m, c, S, S_A, PHI)).abs().max().item() <= 4 * base
    AG.combine_units3(gathered, uidx, 4, 6, 80, S, S_A, plain)
    AG.guidance_rescale3(gathered, uidx, 4, 6, 80, S, S_A, 0.0, ws, zero)
    assert torch.equal(plain, zero)
    same = torch.stack([x[w].permute(1, 2, 0).reshape(6 * 80, 4) for w in range(2) for x in (u, m, m)])
    two = torch.empty(2, 4, 6, 80)
    AG.combine_units3(same, uidx, 4, 6, 80, S, S_A, plain)
    emulated.combine_units(same, uidx[:, :2].contiguous(), 4, 6, 80, S, two)
    assert torch.equal(plain, two)


def test_init_latents_and_mask_keep_their_region_exactly(emulated, small_pipe):
    F_, cf, co, steps = 6, 4, 2, 4
    inp = _inputs(F_)
    init = torch.randn(1, 4, F_, 8, 8, generator=torch.Generator().manual_seed(7)) * 0.18215
    mask = torch.ones(F_, 1, 64, 64)
    mask[..., :32] = 0.0                                        # latent columns 0..3 are kept
    got = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, strength=0.5, init_latents=init, mask=mask,
                audio_guidance_scale=S_A)
    two = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, strength=0.5, init_latents=init, mask=mask)
    assert small_pipe.last_init["masked"] and torch.isfinite(got).all()
    assert torch.equal(got[..., :4], init[..., :4]) and torch.equal(two[..., :4], init[..., :4])
    assert rel_l2(got[..., 4:], two[..., 4:]) > 1e-3


# ------------------------------------------------------------------------------------------------ (6) errors
def test_bad_audio_scale_fails_before_any_prologue_hook(emulated, small_pipe, monkeypatch):
    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "combine_units3", "guidance_rescale3", "overlap_ddim_step",
                 "ncfhw_to_nhwc", "groupnorm", "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)

    def no_hook(*a, **k):
        raise AssertionError("a prologue hook ran")
    for name in ("prepare_reference_latent", "prepare_kps_feature", "prepare_kps_tokens", "prepare_audio_embeddings"):
        monkeypatch.setattr(small_pipe, name, no_hook)
    small_pipe.scheduler = scheduler("ddim")
    inp = _inputs(4)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="audio_guidance_scale"):
            small_pipe(None, None, None, 64, 64, 4, 2, S, context_frames=4, context_overlap=2,
                       audio_guidance_scale=bad)
        with pytest.raises(ValueError, match="audio_guidance_scale"):
            small_pipe.denoise(inp["latents"].clone(), None, None, [999, 499], [[0, 1, 2, 3]], S,
                               audio_guidance_scale=bad)


def test_ops_wrappers_check_their_arguments():
    from v_express_amd import ops
    gathered = torch.zeros(3, 4 * 16, 4)
    uidx = torch.tensor([[[0], [1], [2]]], dtype=torch.int32)
    ws, preds = torch.zeros(ops.guidance_rescale_ws_floats(1, 4, 16)), torch.zeros(1, 4, 4, 16)
    for op, tail in ((ops.combine_units3, (preds,)), (ops.guidance_rescale3, (0.7, ws, preds))):
        with pytest.raises(ValueError, match="u, m, c"):
            op(gathered, uidx[:, :2].contiguous(), 4, 4, 16, 3.5, 6.0, *tail)
        with pytest.raises(TypeError):
            op(gathered, uidx.long(), 4, 4, 16, 3.5, 6.0, *tail)
        with pytest.raises(ValueError, match="sizes"):
            op(gathered, uidx, 4, 4, 16, 3.5, 6.0, *tail[:-1], preds[:, :3].contiguous())
    with pytest.raises(ValueError, match="phi"):
        ops.guidance_rescale3(gathered, uidx, 4, 4, 16, 3.5, 6.0, 1.5, ws, preds)
    with pytest.raises(ValueError, match="workspace"):
        ops.guidance_rescale3(gathered, uidx, 4, 4, 16, 3.5, 6.0, 0.7, ws[:5], preds)


def test_c_entry_points_validate_before_any_launch():
    """(12) Null pointers, shards not dividing f and a short workspace return < 0 with a message; the checks run before
    any launch, so this needs no GPU (the pointers are never read)."""
    from v_express_amd import lib as L
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for so in (L.lib, L.lib_f16()):
        err = so.vx_last_error_string
        for args in ((None, p, 1, 1, 4, 4, 16, 3.5, 6.0, p, None), (p, None, 1, 1, 4, 4, 16, 3.5, 6.0, p, None),
                     (p, p, 1, 1, 4, 4, 16, 3.5, 6.0, None, None), (p, p, 1, 3, 4, 4, 16, 3.5, 6.0, p, None),
                     (p, p, 0, 1, 4, 4, 16, 3.5, 6.0, p, None)):
            assert so.vx_combine_units3(*args) < 0 and b"vx_combine_units3: bad arguments" in err()
        need = so.vx_guidance_rescale_ws_floats(1, 4, 16)
        for args, msg in (((None, p, 1, 1, 4, 4, 16, 3.5, 6.0, 0.7, p, need, p, None), b"bad arguments"),
                          ((p, p, 1, 1, 4, 4, 16, 3.5, 6.0, 0.7, None, need, p, None), b"bad arguments"),
                          ((p, p, 1, 1, 4, 4, 16, 3.5, 6.0, 0.7, p, need, None, None), b"bad arguments"),
                          ((p, p, 1, 3, 4, 4, 16, 3.5, 6.0, 0.7, p, need, p, None), b"bad arguments"),
                          ((p, p, 1, 1, 4, 4, 16, 3.5, 6.0, 1.5, p, need, p, None), b"phi"),
                          ((p, p, 1, 1, 1, 1, 1, 3.5, 6.0, 0.7, p, need, p, None), b"two values"),
                          ((p, p, 1, 1, 4, 4, 16, 3.5, 6.0, 0.7, p, need - 1, p, None), b"workspace too small")):
            assert so.vx_guidance_rescale3(*args) < 0
            assert err().startswith(b"vx_guidance_rescale3: ") and msg in err(), err()


# ------------------------------------------------------------------------------------------------ (7) schedules, ranks
@pytest.mark.parametrize("world", [2, 4, 8])
def test_unit_schedules_for_three_rows(world):
    """halves = 3: every (window, row) unit exactly once, loads differing by at most one (whole units) or equal (mixed),
    no two units in one slot."""
    from v_express_amd.distributed import MixedUnitSchedule, UnitSchedule, choose_mixed_shards, partition_units
    for nW in range(1, 12):
        units = [(w, h) for w in range(nW) for h in range(3)]
        parts = partition_units(nW, world, 3)
        assert sorted(u for p in parts for u in p) == units
        assert max(map(len, parts)) - min(map(len, parts)) <= 1
        for S in (1, 2):
            if world % S:
                continue
            sched = UnitSchedule(nW, world, S, 3)
            assert sorted(sched.slot) == units and len(set(sched.slot.values())) == len(units)
            sizes = [len(a) for a in sched.assign]
            assert max(sizes) - min(sizes) <= 1 and sched.max_units == max(sizes)
            seen = set()
            for u in units:
                ranks, slot = sched.unit_ranks(u)
                assert len(ranks) == S and 0 <= slot < sched.max_units
                seen |= {(r, slot) for r in ranks}
            assert len(seen) == len(units) * S
            for r in range(world):
                assert [(w, h) for w, hs in sched.calls(r) for h in hs] == sched.assign[r // S]
        Sm = choose_mixed_shards(len(units), world, 8, 64)
        if Sm > 1:
            mixed = MixedUnitSchedule(nW, world, Sm, 3)
            assert sorted(mixed.slots) == units
            places = [p for u in units for p in mixed.slots[u]]
            assert len(places) == len(set(places)) == len(units) * Sm
            assert all(0 <= slot < mixed.max_slots and 0 <= r < world for r, slot in places)
            whole = [len(w) for w in mixed.whole]
            assert max(whole) == min(whole) and sorted(sum(mixed.whole, []) + mixed.split) == units


@pytest.mark.parametrize("geometry,units", [("one_window", 3), ("two_windows", 6)])
def test_two_gloo_ranks_are_bit_identical_to_one_process(emulated, geometry, units):
    """Three rows per window, the rescale and an interval on two gloo ranks (whole units): one window = 3 units, ranks
    (u, m) | (c), so the c row runs alone on its rank; two windows = 6 units.  The bits of one process, on both ranks."""
    import audio_guidance_worker
    ref, _, _ = audio_guidance_worker.run(geometry)
    results = spawn_gloo(audio_guidance_worker.main, 2, geometry, timeout=900)
    for rank, (lat, sched, guid) in enumerate(results):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))
        assert sched == dict(kind="whole units", frame_shards=1, mixed_shards=1, units=units, world=2)
        assert guid["unguided_schedule"]["units"] == units // 3 and guid["guided_steps"] == 2
