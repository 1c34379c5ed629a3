"""Weighted window blending and the even-fit context schedule on the host: `context.uniform_fit`, `blend_weights`,
`weighted_overlap_plan`, and `overlap_blend` / `context_schedule="uniform_fit"` of VExpressPipeline under emulated kernels
(tests/fake_ops.py + the restated ops of the earlier features + window_blend_restated.overlap_blend) against float64
restatements over the oracle UNet: the schedule's properties over a grid, the weights, the seam property, the restated
kernel's bound, every sampler, the defaults and the ones profile bit for bit, the composition with the guidance controls
and init-video sampling, two gloo ranks against one process, the symbol and the C entry point's argument checks."""
import ctypes
import random

import numpy as np
import pytest
import torch

import cases
import init_video_restated as R
import window_blend_restated as WB
from loop_restated import restated_loop
from loop_worker import (SEED, UPDATES, call_pipeline as _call, emulated, inputs as _inputs,  # noqa: F401
                         oracle_unet as _oracle_unet, rel_l2, sampler_kw as _sampler_kw, scheduler, small_pipe,
                         spawn_gloo, trace_ops as _trace)

S = cases.GUIDANCE
BOUND = 5e-2        # the relative-L2 bound tests/test_audio_guidance_cpu.py applies to the same loop at these geometries
F11 = (11, 4, 2)    # F, context frames, overlap: even-fit starts 0, 1, 3, 5, 7 - frame 3 lies in three windows


def sched_windows(name, F_, f, o):
    from v_express_amd.context import get_context_scheduler
    return list(get_context_scheduler(name)(step=0, num_frames=F_, context_size=f, context_stride=1, context_overlap=o,
                                            closed_loop=False))


# ------------------------------------------------------------------------------------------------ (1) the schedule
def _grid():
    """Every (f, o) of 2 <= f <= 32, 0 <= o < f (o = 0 and o = f - 1 among them); per pair the lengths F = 1, f - 1, f,
    f + 1, every aligned length f + k (f - o) below 130, and every third of the others."""
    for f in range(2, 33):
        for o in range(f):
            hop = f - o
            for F_ in range(1, 130):
                aligned = F_ <= f or (F_ - f) % hop == 0
                if aligned or F_ in (1, f - 1, f + 1, 129) or (F_ + f + o) % 3 == 0:
                    yield f, o, F_, aligned


def test_uniform_fit_properties_over_the_grid():
    from v_express_amd.context import uniform, uniform_fit
    sets = same = 0
    for f, o, F_, aligned in _grid():
        ws = list(uniform_fit(step=5, num_frames=F_, context_size=f, context_stride=3, context_overlap=o,
                              closed_loop=True))            # the three ignored arguments, at values `uniform` would heed
        sets += 1
        if F_ <= f:
            assert ws == [list(range(F_))]
        else:
            starts = [w[0] for w in ws]
            assert starts == WB.fit_starts(F_, f, o)
            assert all(w == list(range(w[0], w[0] + f)) and w[0] >= 0 and w[-1] < F_ for w in ws)    # f distinct, in range
            assert all(b > a for a, b in zip(starts[:-1], starts[1:]))
            assert all(f - (b - a) >= o for a, b in zip(starts[:-1], starts[1:]))
            assert sorted(set(i for w in ws for i in w)) == list(range(F_))                          # covered
        assert len(ws) == WB.uniform_count(F_, f, o)
        if aligned:
            same += 1
            assert ws == list(uniform(step=0, num_frames=F_, context_size=f, context_stride=1, context_overlap=o,
                                      closed_loop=False)), (f, o, F_)
    assert sets > 30000 and same >= 22352                   # all aligned sets of the full grid are in


def test_uniform_fit_examples_and_registration():
    from v_express_amd.context import get_context_scheduler, uniform, uniform_fit
    assert get_context_scheduler("uniform_fit") is uniform_fit and get_context_scheduler("uniform") is uniform
    with pytest.raises(ValueError, match="Unknown context_overlap policy"):
        get_context_scheduler("pyramid")
    for F_, want in ((45, [0, 10, 21]), (50, [0, 13, 26]), (200, [0, 19, 39, 58, 78, 97, 117, 136, 156, 176]),
                     (44, [0, 20]), (24, [0]), (7, [0])):
        assert [w[0] for w in sched_windows("uniform_fit", F_, 24, 4)] == want
    assert [w[0] for w in sched_windows("uniform_fit", *F11)] == [0, 1, 3, 5, 7]
    assert "ignored" in uniform_fit.__doc__
    # the count of the reference module's own single level
    assert len(sched_windows("uniform", 50, 24, 4)) == 3 and sched_windows("uniform", 50, 24, 4)[-1][-1] != 49


# ------------------------------------------------------------------------------------------------ (2) the weights
def test_linear_weights_cross_fade_and_normalised_rows():
    from v_express_amd.context import blend_weights, weighted_overlap_plan
    for F_, f, o in ((44, 24, 4), (45, 24, 4), (50, 24, 4), (200, 24, 4), F11, (7, 4, 3), (30, 16, 4), (9, 4, 0)):
        ws = sched_windows("uniform_fit", F_, f, o)
        raw = blend_weights(ws, "linear")
        assert raw.dtype == np.float64 and raw.shape == (len(ws), f)
        assert np.array_equal(raw, np.array(WB.linear([w[0] for w in ws], f)))
        terms = WB.frame_terms(ws, F_)
        for fi, tt in terms.items():
            if len(tt) == 2:                                 # a true cross-fade where exactly two windows overlap
                assert abs(sum(raw[wi, li] for wi, li in tt) - 1.0) <= 1e-15, (F_, fi)
        for blend in ("linear", "pyramid", [0.5 + (j % 3) for j in range(f)]):
            plan = weighted_overlap_plan(ws, F_, blend_weights(ws, blend))
            wts, tab = plan["weights"], plan["term_table"]
            assert wts.dtype == np.float32 and wts.shape == (F_, plan["max_terms"]) and tab.dtype == np.int32
            assert plan["step_frames"] == list(range(F_)) and plan["terms"] == terms
            assert plan["max_terms"] == max(len(tt) for tt in terms.values())
            norm = WB.normalised(ws, F_, WB.raw_weights(ws, blend))
            for fi, tt in terms.items():
                n = len(tt)
                assert abs(float(wts[fi].astype(np.float64).sum()) - 1.0) <= 2.0 ** -23 * n
                assert [tuple(r) for r in tab[fi, :n]] == tt and (tab[fi, n:] == -1).all() and (wts[fi, n:] == 0).all()
                assert [float(x) for x in wts[fi, :n]] == [float(np.float32(w)) for _, _, w in norm[fi]]   # rounded once
                if n == 1:
                    assert wts[fi, 0] == np.float32(1.0)
    ws = sched_windows("uniform_fit", 44, 24, 4)
    assert blend_weights(ws, "linear")[0, 19:].tolist() == [1.0, 0.8, 0.6, 0.4, 0.2]
    assert blend_weights(ws, "linear")[1, :5].tolist() == [0.2, 0.4, 0.6, 0.8, 1.0]


def test_pyramid_and_profile_weights():
    from v_express_amd.context import blend_weights
    for f in (2, 3, 4, 7, 24):
        ws = [list(range(f)), list(range(1, f + 1))]
        assert blend_weights(ws, "pyramid").tolist() == [[float(min(j + 1, f - j)) for j in range(f)]] * 2
        prof = [1.0 + 0.25 * j for j in range(f)]
        for p in (prof, tuple(prof), np.array(prof), torch.tensor(prof, dtype=torch.float64)):
            assert blend_weights(ws, p).tolist() == [prof] * 2
    # a weighted blend without "linear" takes any duplicate-free windows, in any order
    assert blend_weights([[3, 2, 1, 0], [5, 3, 4, 2]], "pyramid").shape == (2, 4)


def test_rejections_name_uniform_fit():
    from v_express_amd.context import blend_weights, check_blend, weighted_overlap_plan
    reflected = sched_windows("uniform", *F11)
    assert reflected[-1] == [8, 9, 10, 9]                   # a non-aligned `uniform` clip: the reflected last window
    for blend in ("linear", "pyramid", [1.0, 2.0, 2.0, 1.0]):
        with pytest.raises(ValueError, match='context_schedule="uniform_fit"'):
            blend_weights(reflected, blend)
    with pytest.raises(ValueError, match='context_schedule="uniform_fit"'):
        weighted_overlap_plan(reflected, 11, np.ones((len(reflected), 4)))
    for ws in ([[0, 1, 2, 3], [2, 3, 5, 4]],                # not ascending
               [[0, 1, 2, 3], [2, 3, 4, 6]],                # not contiguous
               [[2, 3, 4, 5], [0, 1, 2, 3]],                # not by increasing start
               [[0, 1, 2, 3], [0, 1, 2, 3]]):               # starts do not increase
        with pytest.raises(ValueError, match='context_schedule="uniform_fit"'):
            blend_weights(ws, "linear")
    ok = [[0, 1, 2, 3], [2, 3, 4, 5]]
    for bad, what in (("gaussian", "unknown overlap_blend"), ([1.0, 1.0, 1.0], "4 expected, got 3"),
                      ([1.0] * 5, "4 expected, got 5"), ([1.0, 0.0, 1.0, 1.0], "finite positive"),
                      ([1.0, -1.0, 1.0, 1.0], "finite positive"), ([1.0, float("nan"), 1.0, 1.0], "finite positive"),
                      ([1.0, float("inf"), 1.0, 1.0], "finite positive"), ([1.0, "x", 1.0, 1.0], "sequence of numbers"),
                      (3.0, "sequence of numbers")):
        with pytest.raises(ValueError, match=what):
            blend_weights(ok, bad)
        with pytest.raises(ValueError, match=what):
            check_blend(bad, 4)
    assert [check_blend(b, 4) for b in (None, "mean", "linear", "pyramid", [1, 2, 2, 1])] == \
        ["mean", "mean", "linear", "pyramid", "profile"]
    with pytest.raises(ValueError, match="never completed"):
        weighted_overlap_plan([[0, 1, 2, 3]], 6, np.ones((1, 4)))


# ------------------------------------------------------------------------------------------------ (3) the seam
def test_seam_jump_is_a_half_under_the_mean_and_a_fifth_under_linear():
    from v_express_amd.context import blend_weights, weighted_overlap_plan
    ws = sched_windows("uniform_fit", 44, 24, 4)
    assert ws == sched_windows("uniform", 44, 24, 4) and [w[0] for w in ws] == [0, 20]
    assert WB.max_jump(WB.blend_constants(ws, 44, None, [0.0, 1.0])) == 0.5
    # through the product's own plan: float32 weights k / 5 against constants 0 and 1
    plan = weighted_overlap_plan(ws, 44, blend_weights(ws, "linear"))
    v = [sum(float(plan["weights"][i, t]) * float(wi) for t, (wi, _) in enumerate(plan["terms"][i])) for i in range(44)]
    assert abs(WB.max_jump(v) - 1 / 5) <= 2.0 ** -24          # two weights <= 1, each rounded once to float32
    assert WB.max_jump(WB.blend_constants(ws, 44, WB.linear([0, 20], 24), [0.0, 1.0])) == pytest.approx(1 / 5, abs=1e-15)


def test_linear_seams_on_random_offsets_F200():
    from v_express_amd.context import blend_weights
    F_, f, o = 200, 24, 4
    ws = sched_windows("uniform_fit", F_, f, o)
    raw = blend_weights(ws, "linear").tolist()
    rng = random.Random(5)
    for _ in range(20):
        off = [rng.gauss(0.0, 1.0) for _ in ws]
        spread = max(off) - min(off)                         # the largest pairwise disagreement
        lin, mean = WB.max_jump(WB.blend_constants(ws, F_, raw, off)), WB.max_jump(WB.blend_constants(ws, F_, None, off))
        assert lin <= 2.0 / (o + 1) * spread and lin < mean, (lin, mean, spread)


# ------------------------------------------------------------------------------------------------ (4) the restated op
@pytest.mark.parametrize("mean", [0.0, 30.0])
def test_restated_kernel_within_its_bound_of_float64(mean):
    from v_express_amd.context import blend_weights, weighted_overlap_plan
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for (F_, f, o), blend, c, hw in ((F11, "linear", 4, 36), ((7, 4, 3), "pyramid", 3, 64), ((44, 24, 4), "linear", 4, 64)):
        ws = sched_windows("uniform_fit", F_, f, o)
        plan = weighted_overlap_plan(ws, F_, blend_weights(ws, blend))
        terms, wts = WB.tables(plan)
        preds = torch.randn(len(ws), c, f, hw, generator=g) + mean
        out = torch.full((c, F_, hw), float("nan"))
        WB.overlap_blend(preds, terms, wts, out)
        ref, bound = WB.overlap_blend64(preds, terms, wts)
        assert torch.isfinite(out).all() and ((out.double() - ref).abs() <= bound).all()
        worst = max(worst, ((out.double() - ref).abs() / bound).max().item())
        # against the float64 weights of the definition: the one rounding of each weight more
        norm = WB.normalised(ws, F_, WB.raw_weights(ws, blend))
        for fi in (0, F_ // 2, F_ - 1):
            exact = sum(w * preds[wi, :, li].double() for wi, li, w in norm[fi])
            mag = sum(w * preds[wi, :, li].double().abs() for wi, li, w in norm[fi])
            assert ((out[:, fi].double() - exact).abs() <= (2 * plan["max_terms"] + 1) * WB.U * mag).all()
    print(f"[restated overlap_blend, predictions of mean {mean}] largest |err| / bound {worst:.3f}")
    # the first valid term initialises the sum: a -1 in the first column, and a row of one term times 1.0 is a copy
    preds = torch.randn(2, 2, 3, 4, generator=g)
    terms = torch.tensor([[[-1, -1], [1, 2]], [[0, 0], [-1, -1]], [[0, 1], [1, 0]]], dtype=torch.int32)
    wts = torch.tensor([[0.25, 1.0], [1.0, 0.0], [0.75, 0.25]])
    out = torch.full((2, 3, 4), float("nan"))
    WB.overlap_blend(preds, terms, wts, out)
    assert torch.equal(out[:, 0], preds[1, :, 2]) and torch.equal(out[:, 1], preds[0, :, 0])
    assert torch.equal(out[:, 2], 0.75 * preds[0, :, 1] + 0.25 * preds[1, :, 0])


# ------------------------------------------------------------------------------------------------ the emulated pipeline
@pytest.mark.parametrize("kind", ["ddim", "dpm", "ddim-eta", "euler-a"])
def test_weighted_clips_match_the_restated_loop(emulated, small_pipe, monkeypatch, kind):
    """F 11 in even-fit windows of 4 with overlap 2 (starts 0, 1, 3, 5, 7), 3 steps of DDIM, DPM++ 2M, DDIM eta = 1 and
    Euler ancestral: the "linear" and "pyramid" clips lie within the loop's bound of the float64-weighted restated loop
    over the oracle UNet, differ from the mean clip, and run exactly one overlap_blend per timestep, before the update.
    Fails on a pipeline without the keyword."""
    F_, cf, co = F11
    steps = 3
    inp = _inputs(F_)
    windows = WB.fit_windows(F_, cf, co)
    assert [w[0] for w in windows] == [0, 1, 3, 5, 7] and len(WB.frame_terms(windows, F_)[3]) == 3
    skw = _sampler_kw(kind)
    mean = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, context_schedule="uniform_fit", **skw)
    assert small_pipe.last_overlap == dict(schedule="uniform_fit", blend="mean", windows=5, max_terms=3, blend_launches=0)
    update = {"ddim": "overlap_ddim_step", "dpm": "overlap_multistep_step"}.get(kind, "overlap_ancestral_step")
    trace = _trace(monkeypatch, emulated)
    unet = _oracle_unet(inp)
    for blend in ("linear", "pyramid"):
        del trace[:]
        got = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, context_schedule="uniform_fit",
                    overlap_blend=blend, **skw)
        assert small_pipe.last_overlap == dict(schedule="uniform_fit", blend=blend, windows=5, max_terms=3,
                                               blend_launches=steps)
        tail = [n for n in trace if n in ("combine_units", "overlap_blend") + UPDATES]
        assert tail == ["combine_units", "overlap_blend", update] * steps
        assert torch.isfinite(got).all() and rel_l2(got, mean) > 1e-3
        with torch.no_grad():
            ref = restated_loop(unet, inp["latents"], windows, S, inp["kps_features"], inp["audio_embeddings"], steps,
                                kind, seed=SEED, eta=skw["eta"], raw=WB.raw_weights(windows, blend))
        r = rel_l2(got, ref)
        print(f"[__call__ {kind}, uniform_fit F11 c4 o2, overlap_blend={blend}, {steps} steps, emulated kernels] relL2 vs "
              f"the restated weighted loop {r:.4g}; the mean clip {rel_l2(mean, ref):.4g}")
        assert r <= BOUND


def test_a_profile_runs_as_given(emulated, small_pipe):
    """A per-position profile equal to the pyramid gives the pyramid clip's bits; a lopsided one another clip."""
    F_, cf, co = 7, 4, 2
    inp = _inputs(F_)
    kw = dict(context_schedule="uniform_fit")
    pyr = _call(small_pipe, scheduler("ddim"), inp, F_, 2, cf, co, overlap_blend="pyramid", **kw)
    prof = _call(small_pipe, scheduler("ddim"), inp, F_, 2, cf, co, overlap_blend=(1, 2, 2, 1), **kw)
    assert small_pipe.last_overlap == dict(schedule="uniform_fit", blend="profile", windows=3, max_terms=3,
                                           blend_launches=2)
    lop = _call(small_pipe, scheduler("ddim"), inp, F_, 2, cf, co, overlap_blend=torch.tensor([8.0, 4.0, 2.0, 1.0]), **kw)
    assert torch.equal(pyr, prof) and not torch.equal(pyr, lop) and torch.isfinite(lop).all()
    # one short window (F < context_frames): every weight normalises to 1 - the mean clip's bits
    short = _inputs(4)
    a = _call(small_pipe, scheduler("ddim"), short, 4, 2, 6, 2)
    b = _call(small_pipe, scheduler("ddim"), short, 4, 2, 6, 2, overlap_blend=[1, 2, 3, 3, 2, 1], **kw)
    assert torch.equal(a, b) and small_pipe.last_overlap["blend_launches"] == 2


# ------------------------------------------------------------------------------------------------ defaults
def test_defaults_take_the_mean_route_bit_for_bit(emulated, small_pipe, monkeypatch):
    F_, cf, co, steps = 6, 4, 2, 2                            # an aligned length: 4 + (4 - 2)
    inp = _inputs(F_)

    def boom(*a, **k):
        raise AssertionError("overlap_blend ran on the mean route")
    monkeypatch.setattr(emulated, "overlap_blend", boom)
    plans = []
    from v_express_amd import pipeline as P
    monkeypatch.setattr(P, "weighted_overlap_plan", lambda *a, **k: plans.append(a) or boom())
    trace = _trace(monkeypatch, emulated)
    base = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co)
    base_trace = list(trace)
    assert "overlap_blend" not in base_trace and base_trace.count("overlap_ddim_step") == steps
    want = dict(schedule="uniform", blend="mean", windows=2, max_terms=2, blend_launches=0)
    assert small_pipe.last_overlap == want
    for kw in (dict(overlap_blend="mean"), dict(overlap_blend=None), dict(context_schedule="uniform_fit"),
               dict(context_schedule="uniform_fit", overlap_blend="mean")):
        del trace[:]
        same = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, **kw)
        assert trace == base_trace and torch.equal(base, same) and not plans
        assert small_pipe.last_overlap == dict(want, schedule=kw.get("context_schedule", "uniform"))
    # the other last_* reports are what they were
    assert small_pipe.last_guidance == dict(guided_steps=steps, steps=steps, rescale=0.0, unguided_schedule=None)
    assert small_pipe.last_init == dict(begin_index=0, masked=False, blend_launches=0)
    # uniform_fit with the mean on a length `uniform` reflects: the existing mean route, no duplicates, every frame once
    del trace[:]
    fit = _call(small_pipe, scheduler("ddim"), _inputs(7), 7, steps, cf, co, context_schedule="uniform_fit")
    assert "overlap_blend" not in trace and torch.isfinite(fit).all()
    assert small_pipe.last_overlap == dict(schedule="uniform_fit", blend="mean", windows=3, max_terms=3, blend_launches=0)


@pytest.mark.parametrize("kind", ["ddim", "dpm", "ddim-eta", "euler-a"])
def test_ones_profile_on_two_windows_is_the_mean_route_bit_for_bit(emulated, small_pipe, monkeypatch, kind):
    """Counts 1 and 2 only: weights 1 and 0.5, and x * 0.5 == x / 2, x * 1 == x / 1 in float32."""
    F_, cf, co, steps = 6, 4, 2, 2
    inp = _inputs(F_)
    skw = _sampler_kw(kind)
    mean = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, **skw)
    trace = _trace(monkeypatch, emulated)
    ones = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, overlap_blend=[1.0] * cf, **skw)
    assert trace.count("overlap_blend") == steps and small_pipe.last_overlap["blend"] == "profile"
    assert torch.isfinite(ones).all() and torch.equal(mean, ones)
    lin = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, overlap_blend="linear", **skw)
    assert not torch.equal(mean, lin)


# ------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("case", ["rescale", "interval", "audio-scale", "init-mask"])
def test_linear_composes_with_the_other_controls(emulated, small_pipe, monkeypatch, case):
    """F 7 in even-fit windows of 4 with overlap 2 (starts 0, 1, 3), DDIM, "linear", with guidance_rescale = 0.7, with
    guidance_end = 0.6, with audio_guidance_scale = 6 and with an init clip + mask at strength 0.6: one short run each
    against the restated loop."""
    F_, cf, co = 7, 4, 2
    inp = _inputs(F_)
    windows = WB.fit_windows(F_, cf, co)
    raw = WB.raw_weights(windows, "linear")
    steps = {"interval": 5, "init-mask": 5}.get(case, 3)
    kw, rkw = {}, {}
    if case == "rescale":
        kw, rkw = dict(guidance_rescale=0.7), dict(phi=0.7)
    elif case == "interval":
        kw, rkw = dict(guidance_end=0.6), dict(end=0.6)
    elif case == "audio-scale":
        kw, rkw = dict(audio_guidance_scale=6.0), dict(s_a=6.0)
    else:
        init = torch.randn(1, 4, F_, 8, 8, generator=torch.Generator().manual_seed(7)) * 0.18215
        mask = torch.ones(F_, 1, 64, 64)
        mask[:2] = 0.0
        mask[2:, :, :32] = 0.0                               # frames 0-1 kept whole, the upper half of the others
        kw = dict(strength=0.6, init_latents=init, mask=mask)
        rkw = dict(known=(init, inp["latents"], R.box_mean(mask[:, 0]), 0.6))
    trace = _trace(monkeypatch, emulated)
    got = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, context_schedule="uniform_fit",
                overlap_blend="linear", **kw)
    ran = small_pipe.last_overlap["blend_launches"]
    assert trace.count("overlap_blend") == ran == (3 if case == "init-mask" else steps)
    before = {"rescale": "guidance_rescale", "audio-scale": "combine_units3"}.get(case, "combine_units")
    assert all(trace[i - 1] == before and trace[i + 1] == "overlap_ddim_step"
               for i, n in enumerate(trace) if n == "overlap_blend")
    if case == "interval":
        assert small_pipe.last_guidance["guided_steps"] == 3
    if case == "init-mask":
        assert small_pipe.last_init == dict(begin_index=2, masked=True, blend_launches=4)
        assert torch.equal(got[:, :, :2], init[:, :, :2]) and torch.equal(got[..., :4, :], init[..., :4, :])
    with torch.no_grad():
        ref = restated_loop(_oracle_unet(inp), inp["latents"], windows, S, inp["kps_features"], inp["audio_embeddings"],
                            steps, "ddim", raw=raw, **rkw)
    r = rel_l2(got, ref)
    print(f"[__call__ ddim, uniform_fit F7 c4 o2, linear + {case}, {steps} steps, emulated kernels] relL2 vs the restated "
          f"loop {r:.4g}")
    assert torch.isfinite(got).all() and r <= BOUND


# ------------------------------------------------------------------------------------------------ errors
def test_bad_blends_fail_before_any_prologue_hook(emulated, small_pipe, monkeypatch):
    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "overlap_blend", "overlap_ddim_step", "ncfhw_to_nhwc", "groupnorm",
                 "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)

    def no_hook(*a, **k):
        raise AssertionError("a prologue hook ran")
    for name in ("prepare_reference_latent", "prepare_kps_feature", "prepare_kps_tokens", "prepare_audio_embeddings"):
        monkeypatch.setattr(small_pipe, name, no_hook)
    small_pipe.scheduler = scheduler("ddim")
    lat = _inputs(11)["latents"]
    fit, reflected = WB.fit_windows(*F11), sched_windows("uniform", *F11)
    for bad, what in (("gaussian", "unknown overlap_blend"), ([1.0] * 3, "4 expected, got 3"),
                      ([1.0, 0.0, 1.0, 1.0], "finite positive"), ([1.0, float("inf"), 1.0, 1.0], "finite positive"),
                      ([1.0, -2.0, 1.0, 1.0], "finite positive")):
        with pytest.raises(ValueError, match=what):
            small_pipe(None, None, None, 64, 64, 11, 2, S, context_frames=4, context_overlap=2,
                       context_schedule="uniform_fit", overlap_blend=bad)
        with pytest.raises(ValueError, match=what):
            small_pipe.denoise(lat.clone(), None, None, [999, 499], fit, S, overlap_blend=bad)
    # a schedule the blend rejects: the reflected last window of a non-aligned `uniform` clip
    for blend in ("linear", "pyramid", [1.0, 2.0, 2.0, 1.0]):
        with pytest.raises(ValueError, match='context_schedule="uniform_fit"'):
            small_pipe(None, None, None, 64, 64, 11, 2, S, context_frames=4, context_overlap=2, overlap_blend=blend)
        with pytest.raises(ValueError, match='context_schedule="uniform_fit"'):
            small_pipe.denoise(lat.clone(), None, None, [999, 499], reflected, S, overlap_blend=blend)
    with pytest.raises(ValueError, match="Unknown context_overlap policy"):
        small_pipe(None, None, None, 64, 64, 11, 2, S, context_frames=4, context_overlap=2, context_schedule="fit",
                   overlap_blend="linear")


def test_ops_wrapper_checks_its_arguments():
    from v_express_amd import ops
    preds, out = torch.zeros(2, 4, 3, 8), torch.zeros(4, 5, 8)
    terms, wts = torch.full((5, 2, 2), -1, dtype=torch.int32), torch.zeros(5, 2)
    for args in ((preds.double(), terms, wts, out), (preds, terms, wts.double(), out), (preds, terms, wts, out.double()),
                 (preds, terms.long(), wts, out), (preds.transpose(2, 3), terms, wts, out),
                 (preds, terms, wts, out.transpose(0, 1)), (preds, terms.transpose(0, 1), wts, out)):
        with pytest.raises(TypeError, match="overlap_blend"):
            ops.overlap_blend(*args)
    for args in ((preds[0], terms, wts, out), (preds, terms[..., :1].contiguous(), wts, out),
                 (preds, terms, wts[:, :1].contiguous(), out), (preds, terms, wts[:4].contiguous(), out),
                 (preds, terms, wts, out[:, :4].contiguous()), (preds, terms, wts, torch.zeros(1, 4, 4, 2, 4))):
        with pytest.raises(ValueError, match="overlap_blend"):
            ops.overlap_blend(*args)


# ------------------------------------------------------------------------------------------------ the C entry point
def test_symbol_is_declared_bound_and_exported_by_both_libraries():
    from v_express_amd import lib as L
    assert "vx_overlap_blend" in L.declared_symbols()
    with open(L.HEADER) as f:
        header = f.read()
    assert "int vx_overlap_blend(const float* preds, int c, int f_window, int hw, const int32_t* terms" in header
    assert ":552-572" in header.split("int vx_overlap_blend(")[0].rsplit("/*", 1)[1]
    for so, path in ((L.lib, L.LIB_PATH), (L.lib_f16(), L.LIB16_PATH)):
        assert hasattr(ctypes.CDLL(path), "vx_overlap_blend")
        assert len(so.vx_overlap_blend.argtypes) == 10 and so.vx_overlap_blend.restype is ctypes.c_int32
        assert so.vx_abi_version() == 15


def test_c_entry_point_validates_before_any_launch():
    """Null pointers, sizes < 1, hw % 4 != 0 and a pointer off the 16-byte grid return < 0 with a message; the checks run
    before any launch, so this needs no GPU (the pointers are never read)."""
    from v_express_amd import lib as L
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    for elem, so in ((torch.bfloat16, L.lib), (torch.float16, L.lib_f16())):
        err = so.vx_last_error_string
        for args in ((None, 4, 3, 8, p, p, 2, 5, p, None), (p, 4, 3, 8, None, p, 2, 5, p, None),
                     (p, 4, 3, 8, p, None, 2, 5, p, None), (p, 4, 3, 8, p, p, 2, 5, None, None),
                     (p, 0, 3, 8, p, p, 2, 5, p, None), (p, 4, 0, 8, p, p, 2, 5, p, None),
                     (p, 4, 3, 8, p, p, 0, 5, p, None), (p, 4, 3, 8, p, p, 2, 0, p, None),
                     (p, 4, 3, 6, p, p, 2, 5, p, None), (p, 4, 3, 0, p, p, 2, 5, p, None),
                     (p + 4, 4, 3, 8, p, p, 2, 5, p, None), (p, 4, 3, 8, p, p, 2, 5, p + 8, None)):
            rc = so.vx_overlap_blend(*args)
            assert rc < 0 and err().startswith(b"vx_overlap_blend: bad arguments"), (args, err())
            with L.element_type(elem), pytest.raises(L.VxError, match="hw % 4 == 0 and 16-byte aligned"):
                L.check(rc, "vx_overlap_blend")


# ------------------------------------------------------------------------------------------------ two ranks
def test_two_gloo_ranks_are_bit_identical_to_one_process(emulated):
    """Three windows x two CFG halves on two gloo ranks with the "linear" blend (the blend, like the update, runs
    redundantly on every rank): the bits of one process, on both ranks."""
    import window_blend_worker
    ref, _, over = window_blend_worker.run()
    assert over == dict(schedule=None, blend="linear", windows=3, max_terms=3, blend_launches=window_blend_worker.STEPS)
    mean, _, _ = window_blend_worker.run(blend="mean")
    assert not torch.equal(ref, mean)
    results = spawn_gloo(window_blend_worker.main, 2, timeout=900)
    for rank, (lat, sched, got_over) in enumerate(results):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))
        assert sched == dict(kind="whole units", frame_shards=1, mixed_shards=1, units=6, world=2)
        assert got_over == over
