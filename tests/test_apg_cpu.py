"""Adaptive projected guidance on the host: `apg_eta` / `apg_norm_threshold` / `apg_momentum` of VExpressPipeline under
emulated kernels (tests/fake_ops.py + apg_restated.guidance_apg) against the restated loop, the defaults bit for bit, the
argument errors, the momentum buffers over an interval, two gloo ranks against one process, the stand-in against float64
under the kernel's bound, and the second C ABI header (include/vexpress_hip_guidance.h) with its binding."""
import ctypes

import pytest
import torch

import apg_restated as AP
import apg_worker
import cases
from loop_restated import restated_loop
from loop_worker import (LOOP_OPS, call_pipeline as _call, inputs as _inputs, oracle_unet as _oracle_unet,  # noqa: F401
                         rel_l2, scheduler, small_pipe, spawn_gloo, trace_ops as _trace)

S, S_A, R_CAP, BETA = cases.GUIDANCE, 6.0, 1.0, -0.5
BOUND = 5e-2        # the relative-L2 bound tests/test_guidance_cpu.py applies to the loop at these geometries
APG_KW = dict(apg_eta=0.0, apg_norm_threshold=R_CAP, apg_momentum=BETA)
GEO = (6, 3, 4, 2)  # F, steps, context frames, overlap: two windows


@pytest.fixture()
def emulated(monkeypatch):
    return apg_worker.emulate(monkeypatch)


def _run(pipe, inp, **kw):
    F_, steps, cf, co = GEO
    return _call(pipe, scheduler("ddim"), inp, F_, steps, cf, co, **kw)


# ------------------------------------------------------------------------------------------------ (1) the clip
@pytest.mark.parametrize("s_a", [None, S_A], ids=["two_rows", "three_rows"])
def test_apg_clip_matches_the_restated_loop(emulated, small_pipe, monkeypatch, s_a):
    """Two windows, 3 DDIM steps of which 2 are guided (guidance_end 0.67), eta 0, r 1 (it bites on some frames and not
    on others), beta -0.5: within 2 e_plain of the APG restated loop (e_plain: the plain clip against the plain loop),
    within the loop bound, and closer to it than the plain clip.  Fails on a pipeline that ignores apg_eta."""
    from oracle import loop as OL
    F_, steps, cf, co = GEO
    inp = _inputs(F_)
    windows = OL.uniform_windows(F_, cf, co)
    audio = {} if s_a is None else dict(audio_guidance_scale=s_a)
    plain = _run(small_pipe, inp, guidance_end=0.67, **audio)
    assert "apg" not in small_pipe.last_guidance
    trace = _trace(monkeypatch, emulated, LOOP_OPS + ("guidance_apg",))
    got = _run(small_pipe, inp, guidance_end=0.67, **audio, **APG_KW)
    lg = small_pipe.last_guidance
    assert lg["apg"] == dict(eta=0.0, norm_threshold=R_CAP, momentum=BETA) and lg["guided_steps"] == 2
    assert trace.count("guidance_apg") == 2 and trace.count("combine_units") == 1            # the unguided step
    assert "combine_units3" not in trace and "guidance_rescale" not in trace and "guidance_rescale3" not in trace
    assert torch.isfinite(got).all() and rel_l2(got, plain) > 1e-3
    with torch.no_grad():
        oracle = _oracle_unet(inp)
        ref_plain = restated_loop(oracle, inp["latents"], windows, S, inp["kps_features"], inp["audio_embeddings"], steps,
                                  "ddim", s_a=s_a, end=0.67)
        ref, state = AP.restated_loop(oracle, inp["latents"], windows, S, inp["kps_features"], inp["audio_embeddings"],
                                      steps, "ddim", s_a=s_a, end=0.67, eta=0.0, r=R_CAP, beta=BETA)
    bites = torch.cat([c for call in state.capped for c in call])
    assert bool(bites.any()) and not bool(bites.all())
    e_plain, r = rel_l2(plain, ref_plain), rel_l2(got, ref)
    print(f"[__call__ APG eta 0 r {R_CAP} beta {BETA}, audio_guidance_scale {s_a}, emulated kernels, {steps} steps] relL2 "
          f"vs the APG restated loop {r:.4g}; e_plain {e_plain:.4g}; the plain clip vs the APG loop "
          f"{rel_l2(plain, ref):.4g}; the cap bit on {int(bites.sum())} of {bites.numel()} frame differences")
    assert r <= 2 * e_plain and r <= BOUND and r < rel_l2(plain, ref)


def test_rows_m_c_are_guided_by_the_audio_scale(emulated, small_pipe, monkeypatch):
    inp = _inputs(GEO[0])
    seen = []
    orig = emulated.guidance_apg

    def spy(gathered, uidx, c, f, hw, guidance, audio_guidance, *rest):
        seen.append((tuple(uidx.shape), guidance))
        return orig(gathered, uidx, c, f, hw, guidance, audio_guidance, *rest)
    monkeypatch.setattr(emulated, "guidance_apg", spy)
    got = _run(small_pipe, inp, guidance=1.0, audio_guidance_scale=3.5, **APG_KW)
    assert small_pipe.last_guidance["rows"] == ("m", "c") and seen == [((2, 2, 1), 3.5)] * GEO[1]
    assert not torch.equal(got, _run(small_pipe, inp, guidance=1.0, audio_guidance_scale=3.5))


# ------------------------------------------------------------------------------------------------ (2) defaults
def test_defaults_are_bit_identical_and_never_call_the_op(emulated, small_pipe, monkeypatch):
    inp = _inputs(GEO[0])
    trace = _trace(monkeypatch, emulated, LOOP_OPS + ("guidance_apg", "guidance_apg_ws_floats"))
    base = _run(small_pipe, inp)
    base_trace, base_report = list(trace), dict(small_pipe.last_guidance)
    assert "apg" not in base_report
    del trace[:]
    same = _run(small_pipe, inp, apg_eta=None, apg_norm_threshold=0.0, apg_momentum=0.0)
    assert torch.equal(base, same) and trace == base_trace and small_pipe.last_guidance == base_report
    assert "guidance_apg" not in trace and "guidance_apg_ws_floats" not in trace
    # apg_eta = None switches everything off, whatever the other two say
    del trace[:]
    assert torch.equal(base, _run(small_pipe, inp, apg_norm_threshold=2.0, apg_momentum=-0.5)) and trace == base_trace
    # without classifier-free guidance the keywords are ignored
    nocfg = cases.cond_only(inp)
    a = _run(small_pipe, nocfg, guidance=1.0)
    del trace[:]
    b = _run(small_pipe, nocfg, guidance=1.0, **APG_KW)
    assert torch.equal(a, b) and "guidance_apg" not in trace and small_pipe.last_guidance["apg"] is None


def test_guidance_end_zero_is_the_no_cfg_route_bit_for_bit(emulated, small_pipe, monkeypatch):
    inp = _inputs(GEO[0])
    trace = _trace(monkeypatch, emulated, ("guidance_apg",))
    off = _run(small_pipe, inp, guidance_end=0.0, **APG_KW)
    assert small_pipe.last_guidance["guided_steps"] == 0 and not trace
    assert torch.equal(off, _run(small_pipe, cases.cond_only(inp), guidance=1.0))


# ------------------------------------------------------------------------------------------------ (3) errors
def test_bad_arguments_fail_before_any_kernel(emulated, small_pipe, monkeypatch):
    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "guidance_apg", "overlap_ddim_step", "ncfhw_to_nhwc", "groupnorm",
                 "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)
    inp = _inputs(4)
    for bad, word in ((dict(apg_eta=-0.1), "apg_eta"), (dict(apg_eta=1.5), "apg_eta"),
                      (dict(apg_eta=0.0, apg_norm_threshold=-1.0), "apg_norm_threshold"),
                      (dict(apg_eta=0.0, apg_norm_threshold=float("inf")), "apg_norm_threshold"),
                      (dict(apg_eta=0.0, apg_momentum=1.0), "apg_momentum"),
                      (dict(apg_eta=0.0, apg_momentum=-1.5), "apg_momentum"),
                      (dict(apg_eta=0.5, guidance_rescale=0.7), "same defect.*not built")):
        with pytest.raises(ValueError, match=word):
            _call(small_pipe, scheduler("ddim"), inp, 4, 2, 4, 2, **bad)
        apg = (bad["apg_eta"], bad.get("apg_norm_threshold", 0.0), bad.get("apg_momentum", 0.0))
        with pytest.raises(ValueError, match=word):
            small_pipe.denoise(inp["latents"].clone(), None, None, [999, 499], [[0, 1, 2, 3]], S, apg=apg,
                               guidance_rescale=bad.get("guidance_rescale", 0.0))


def test_ops_wrapper_checks_its_arguments():
    from v_express_amd import ops
    gathered = torch.zeros(3, 4 * 16, 4)
    uidx = torch.tensor([[[0], [1], [2]]], dtype=torch.int32)
    two = uidx[:, :2].contiguous()
    ws, preds, buf = torch.zeros(ops.guidance_apg_ws_floats(1, 3, 4, 16)), torch.zeros(1, 4, 4, 16), torch.zeros(2, 1, 4, 4, 16)
    assert ws.numel() == 1 * 4 * 1 * 5 and ops.guidance_apg_ws_floats(2, 2, 16, 4096) == 2 * 16 * 16 * 3
    tail = (ws, preds)
    for args, err, word in (((gathered, uidx[:, :1].contiguous(), 4, 4, 16, S, S_A, 0.0, 0.0, 0.0, None) + tail, ValueError, "unit_index"),
                            ((gathered, two, 4, 4, 16, S, S_A, 1.5, 0.0, 0.0, None) + tail, ValueError, "eta"),
                            ((gathered, two, 4, 4, 16, S, S_A, 0.0, -1.0, 0.0, None) + tail, ValueError, "norm_threshold"),
                            ((gathered, two, 4, 4, 16, S, S_A, 0.0, 0.0, 1.0, buf[:1]) + tail, ValueError, "momentum"),
                            ((gathered, two, 4, 4, 16, S, S_A, 0.0, 0.0, -0.5, None) + tail, ValueError, "momentum_buf"),
                            ((gathered, two, 4, 4, 16, S, S_A, 0.0, 0.0, 0.0, buf[:1]) + tail, ValueError, "momentum_buf"),
                            ((gathered, uidx, 4, 4, 16, S, S_A, 0.0, 0.0, -0.5, buf[:1]) + tail, ValueError, "momentum_buf"),
                            ((gathered, uidx, 4, 4, 16, S, S_A, 0.0, 0.0, 0.0, None, ws[:-1], preds), ValueError, "workspace"),
                            ((gathered, two, 4, 4, 16, S, S_A, 0.0, 0.0, 0.0, None, ws, preds[:, :3].contiguous()), ValueError, "sizes"),
                            ((gathered, two.long(), 4, 4, 16, S, S_A, 0.0, 0.0, 0.0, None) + tail, TypeError, "int32")):
        with pytest.raises(err, match=word):
            ops.guidance_apg(*args)


def test_library_argument_errors_name_the_argument():
    """vx_guidance_apg validates before any launch, so both libraries answer without a GPU (the pointers are never
    followed)."""
    from v_express_amd import lib
    keep = [torch.zeros(64) for _ in range(5)]
    for so in (lib.lib, lib.lib_f16()):
        AP.check_argument_errors(so, *(t.data_ptr() for t in keep))


# ------------------------------------------------------------------------------------------------ (4) the momentum
def test_unguided_steps_leave_the_momentum_alone(emulated, small_pipe, monkeypatch):
    """5 DDIM steps, guidance_start 0.2, guidance_end 0.8: steps 1-3 are guided.  The buffers are zeros until step 1 and
    keep their bits through step 4; every guided step reads what the one before it stored."""
    from v_express_amd import sampling
    inp = _inputs(GEO[0])
    made, log = [], []
    orig_init = sampling.Guidance.__init__

    def init(self, *a, **k):
        orig_init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(sampling.Guidance, "__init__", init)
    orig = emulated.guidance_apg

    def spy(*a):
        before = a[10].clone()
        orig(*a)
        log.append((before, a[10].clone()))
    monkeypatch.setattr(emulated, "guidance_apg", spy)
    snaps = []
    _call(small_pipe, scheduler("ddim"), inp, GEO[0], 5, GEO[2], GEO[3], guidance_start=0.2, guidance_end=0.8,
          callback=lambda i, t, x: snaps.append(made[-1].momentum.clone()), **APG_KW)
    assert small_pipe.last_guidance["guided_steps"] == 3 and len(log) == 3 and len(snaps) == 5
    assert made[-1].momentum.shape == (1, 2, 4, GEO[2], 64) and not snaps[0].any() and not log[0][0].any()
    assert log[0][1].any() and torch.equal(snaps[1], log[0][1])
    assert torch.equal(log[1][0], log[0][1]) and torch.equal(log[2][0], log[1][1])
    assert torch.equal(snaps[3], log[2][1]) and torch.equal(snaps[4], snaps[3])              # step 4: unguided


def test_no_momentum_means_no_buffer(emulated, small_pipe, monkeypatch):
    inp = _inputs(GEO[0])
    seen = []
    orig = emulated.guidance_apg

    def spy(*a):
        seen.append(a[10])
        orig(*a)
    monkeypatch.setattr(emulated, "guidance_apg", spy)
    _run(small_pipe, inp, apg_eta=0.5, apg_norm_threshold=R_CAP)
    assert seen == [None] * GEO[1]


# ------------------------------------------------------------------------------------------------ (5) two ranks
@pytest.mark.parametrize("frame_shards,latent", [(None, 8), (2, 16)])
def test_two_gloo_ranks_are_bit_identical_to_one_process(emulated, frame_shards, latent):
    """F = 14, windows 8 / 2, three rows, APG with momentum, guidance_end = 0.6: the combine is redundant on every rank
    and does not see which rank or granule a frame came from, so two gloo ranks (whole units, and every unit
    frame-sharded two ways) give the bits of one process, on both ranks."""
    ref, _, _ = apg_worker.run(None, latent)
    results = spawn_gloo(apg_worker.main, 2, frame_shards, latent, timeout=900)
    for rank, (lat, sched, guid) in enumerate(results):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))
        assert sched["frame_shards"] == (frame_shards or 1) and sched["units"] == 6 and sched["world"] == 2
        assert guid["apg"] == dict(eta=0.0, norm_threshold=1.0, momentum=-0.5)


# ------------------------------------------------------------------------------------------------ (6) numerics
def test_eta_one_without_cap_and_momentum_is_cfg_up_to_rounding(emulated, small_pipe, monkeypatch):
    """eta = 1, r = 0, beta = 0 after one step: c + (s - 1)(c - u) against u + s (c - u), both within the kernel bound
    of the float64 value, so the latents differ by no more than twice the bound pushed through the DDIM update."""
    inp = _inputs(GEO[0])
    seen = []
    orig = emulated.guidance_apg

    def spy(*a):
        orig(*a)
        seen.append((AP.unit_rows(*a[:5]), a[12].clone()))
    monkeypatch.setattr(emulated, "guidance_apg", spy)
    F_, _, cf, co = GEO
    cfg = _call(small_pipe, scheduler("ddim"), inp, F_, 1, cf, co)
    apg = _call(small_pipe, scheduler("ddim"), inp, F_, 1, cf, co, apg_eta=1.0)
    (rows, preds), = seen
    u, c = rows[0].double(), rows[1].double()
    ref = u + S * (c - u)
    _, dbars, ratios = AP.project(rows, (S,), 1.0, 0.0, 0.0, None, (1, 3))
    bound = AP.bound(rows, (S,), 0.0, None, dbars, ratios)
    assert bool(((preds.double() - ref).abs() <= bound).all())
    # one v-prediction DDIM step is linear in the prediction with a coefficient below 1 in magnitude
    assert (apg.double() - cfg.double()).abs().max().item() <= 2 * bound.max().item()
    assert torch.isfinite(apg).all()


@pytest.mark.parametrize("mean", [0.0, 3.0, 30.0])
@pytest.mark.parametrize("shape", [(1, 4, 16, 4096), (2, 4, 6, 80), (1, 4, 3, 1040)])
def test_stand_in_holds_the_kernel_bound(mean, shape):
    """apg_restated.guidance_apg against the float64 formula under tests/test_gpu_apg.py's bound, its inputs and
    parameter sets."""
    g = torch.Generator().manual_seed(int(mean) + shape[2])
    u = torch.randn(shape, generator=g) + mean
    m = u + 0.3 * torch.randn(shape, generator=g)
    rows3 = (u, m, m + 0.3 * torch.randn(shape, generator=g))
    prev = 0.3 * torch.randn((2,) + shape, generator=torch.Generator().manual_seed(7))
    nW, c, f, hw = shape
    worst = 0.0
    for kw in (dict(s=3.5, eta=0.0), dict(s=7.5, eta=0.0, r=5.0, beta=-0.5), dict(s=12.0, eta=0.0, r=2.5, beta=-0.75),
               dict(s=3.5, eta=0.6, r=40.0, beta=0.25)):
        for rows in ((rows3[0], rows3[2]), rows3):
            beta, r, scales = kw.get("beta", 0.0), kw.get("r", 0.0), (kw["s"], S_A)[:len(rows) - 1]
            p = None if beta == 0.0 else list(prev[:len(rows) - 1])
            ref, dbars, ratios = AP.project(rows, scales, kw["eta"], r, beta, p, (1, 3))
            gathered = torch.stack([x.permute(0, 2, 3, 1).reshape(nW, f * hw, c) for x in rows], 1).reshape(-1, f * hw, c)
            uidx = torch.arange(nW * len(rows), dtype=torch.int32).view(nW, len(rows), 1)
            buf = None if p is None else torch.stack(p).clone()
            got = torch.empty(shape)
            AP.guidance_apg(gathered, uidx, c, f, hw, kw["s"], S_A, kw["eta"], r, beta, buf,
                            torch.empty(nW * f * -(-hw // AP.CHUNK) * (2 * len(rows) - 1)), got)
            ratio = ((got.double() - ref).abs() / AP.bound(rows, scales, beta, p, dbars, ratios)).max().item() * AP.K
            worst = max(worst, ratio)
    print(f"[guidance_apg stand-in, {shape}, mean {mean}] max |err| / (2^-24 magnitude) = {worst:.3g} (bound {AP.K})")
    assert worst <= AP.K


# ------------------------------------------------------------------------------------------------ (7) the second header
def test_second_header_parses_and_is_disjoint_from_the_first():
    from v_express_amd import abi
    g, h = abi.guidance_header(), abi.header()
    assert g is abi.guidance_header() and g.version == 1 and not g.enums and not g.structs
    assert list(g.functions) == ["vx_guidance_abi_version", "vx_guidance_apg_ws_floats", "vx_guidance_apg"]
    assert not set(g.functions) & set(h.functions)
    i32, vp, fl = ctypes.c_int32, ctypes.c_void_p, ctypes.c_float
    assert g.functions["vx_guidance_abi_version"] == (i32, [])
    assert g.functions["vx_guidance_apg_ws_floats"] == (ctypes.c_int64, [(n, i32) for n in ("n_windows", "rows", "f", "hw")])
    restype, params = g.functions["vx_guidance_apg"]
    assert restype is i32 and [t for _, t in params] == [vp, vp] + [i32] * 6 + [fl] * 5 + [vp, vp, ctypes.c_int64, vp, vp]
    # the version macro is an argument of the reader; its default is the first header's
    text = open(abi.GUIDANCE_HEADER).read()
    with pytest.raises(ImportError, match="VX_ABI_VERSION"):
        abi.parse(text, "guidance.h")
    assert abi.parse(text, "guidance.h", "VX_GUIDANCE_ABI_VERSION").functions == g.functions
    assert abi.parse(open(abi.HEADER).read()).version == h.version


def test_second_header_is_bound_on_both_libraries():
    from v_express_amd import abi, lib
    functions = abi.guidance_header().functions
    assert not set(functions) & set(lib.declared_symbols())          # declared_symbols keeps meaning the first header
    for so in (lib.lib, lib.lib_f16()):
        for n, (restype, params) in functions.items():
            fn = so.__dict__[n]                                      # __dict__: the function objects _load touched
            assert fn.restype is restype and list(fn.argtypes) == [t for _, t in params], n
        assert so.vx_guidance_abi_version() == abi.guidance_header().version == 1


def test_build_stamp_covers_the_second_header(tmp_path):
    import os
    import subprocess
    import sys
    from v_express_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "lib_id.py")], capture_output=True, text=True)
    assert out.stdout.strip() == lib.source_id()
    assert "vexpress_hip_guidance.h" in open(os.path.join(root, "tools", "lib_id.py")).read()
    mk = open(os.path.join(lib.CSRC, "Makefile")).read()
    assert "vexpress_hip_guidance.h" in mk and "vx_guide.hip" in mk
