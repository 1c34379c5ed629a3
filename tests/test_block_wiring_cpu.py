"""The wiring of v_express_amd/blocks.py on the CPU emulation (tests/fake_ops.py under the real blocks.py / weights.py).

1. Freshness of LayerNorm row statistics (tests/stats_spy.py): the unmutated blocks are clean with every wrapped entry
   point consuming statistics at least once, and for every producer of row statistics in blocks.py a mutant of the CALL
   SEQUENCE that makes that one producer skip `stats_out` is flagged at >= 100 x the bound (census.STAT_BOUNDS).  A
   statistics buffer nobody wrote reads (mean 0, rstd 1) - the most benign content an unwritten buffer can have - so the
   ratio is a property of the inputs, not of the allocator.
2. The wiring mutants of the float64 reference (tests/block_wiring_cases.py) lie beyond twice the route bound
   3 x e_emul of tests/test_gpu_block_wiring.py, at the emulation's geometries: a kernel route that made one of these
   mistakes could not pass its GPU case.
"""
import sys

import pytest
import torch

import block_wiring_cases as BC
import stats_spy
from loop_worker import emulated  # noqa: F401

EL = torch.bfloat16


# ------------------------------------------------------------------------------------------------ 1. freshness
def _unwritten(ops, mp):
    """ops.stats_buffer with defined content: (mean 0, rstd 1) / zero sums instead of uninitialised memory."""
    real = ops.stats_buffer

    def buffer(rows, c, device):
        st = real(rows, c, device).zero_()
        if st.shape[1] == 2:
            st[:, 1] = 1.0
        return st
    mp.setattr(ops, "stats_buffer", buffer)


def _skip_producer(ops, mp, op, caller, pred=lambda k: True, nth=None):
    """Mutant of the call sequence: `ops.<op>` called from blocks.<caller> with pred(kwargs) (nth: only the nth such call)
    loses its `stats_out` (a row_stats refresh is not made at all).  Installed OUTSIDE the spy, which therefore sees the
    mutated call.  -> hits."""
    inner = getattr(ops, op)
    hits, seen = [], [0]

    def call(*a, **k):
        if sys._getframe(1).f_code.co_name == caller and pred(k) and (op == "row_stats" or k.get("stats_out") is not None):
            seen[0] += 1
            if nth is not None and seen[0] - 1 != nth:
                return inner(*a, **k)
            hits.append(1)
            if op == "row_stats":
                return k["out"] if k.get("out") is not None else ops.stats_buffer(a[0].shape[0], a[0].shape[-1], a[0].device)
            k = dict(k, stats_out=None)
        return inner(*a, **k)
    mp.setattr(ops, op, call)
    return hits


def _spied(ops, monkeypatch, cs, P, mutant=None, **switches):
    """run(cs) under the spy (and one producer mutant) -> (spy, hits)."""
    with monkeypatch.context() as mp:
        for name, v in switches.items():
            mp.setattr(ops, name, v)
        _unwritten(ops, mp)
        spy = stats_spy.StatsSpy(ops).install(mp)
        hits = _skip_producer(ops, mp, *mutant) if mutant else None
        BC.run(cs, P)
    return spy, hits


@pytest.fixture(scope="module")
def read_cases():
    """The spatial read block at C = 320, f = 4, 8 x 8 pixels: the product's own rules pick the one-launch FF (rows % 128)
    and the one-launch audio block (hw % 16) there; the three audio / bank combinations."""
    out = {}
    for combo in "ABN":
        cs = BC.make_case("read", c=320, f=4, H=8, W=8, device="cpu", elem=EL, combo=combo)
        out[combo] = (cs, BC.prepare(cs))
    return out


@pytest.fixture(scope="module")
def motion_case():
    """The motion module at C = 320, f = 16, 2 x 4 pixels: `tblock_fused_applies` (hw % 8) and `ff_fused_applies`."""
    cs = BC.make_case("motion", c=320, f=16, H=2, W=4, device="cpu", elem=EL)
    return cs, BC.prepare(cs)


W_REF, W_AUD = BC.W_REF, BC.W_AUD
# (block, combo, switches, (op, calling function of blocks.py, predicate on the keywords)) per producer of row statistics
PRODUCERS = {
    "proj_in": ("read", "A", {}, ("gemm", "_norm_proj_in")),
    "attn1_out": ("read", "A", {}, ("gemm", "_self_attention")),
    "attn1_5_out_banked": ("read", "A", {}, ("gemm", "_spatial_transformer_read", lambda k: k.get("alpha") == W_REF)),
    "audio_xattn_item": ("read", "A", {}, ("audio_xattn", "_spatial_transformer_read")),
    "audio_xattn_batched": ("read", "N", {}, ("audio_xattn", "_spatial_transformer_read")),
    "audio_out_item": ("read", "A", {"AX_FUSED": [False]}, ("gemm", "_spatial_transformer_read",
                                                            lambda k: k.get("alpha") == W_AUD)),
    "audio_out_batched": ("read", "N", {"AX_FUSED": [False]}, ("gemm", "_spatial_transformer_read",
                                                               lambda k: k.get("alpha") == W_AUD)),
    "row_stats_refresh": ("read", "B", {}, ("row_stats", "_spatial_transformer_read")),
    "row_stats_refresh_unfolded": ("read", "A", {"FOLD_ZERO_AUDIO": [False]}, ("row_stats", "_spatial_transformer_read")),
    "motion_proj_in": ("motion", None, {}, ("gemm", "_norm_proj_in")),
    "motion_tblock_fused_0": ("motion", None, {}, ("tblock_fused", "_motion_module", lambda k: True, 0)),
    "motion_tblock_fused_1": ("motion", None, {}, ("tblock_fused", "_motion_module", lambda k: True, 1)),
    "motion_attn_out_three_launch_0": ("motion", None, {"TB_FUSED": [False]}, ("gemm", "_motion_module", lambda k: True, 0)),
    "motion_attn_out_three_launch_1": ("motion", None, {"TB_FUSED": [False]}, ("gemm", "_motion_module", lambda k: True, 1)),
}


def _pick(block, combo, read_cases, motion_case):
    return motion_case if block == "motion" else read_cases[combo]


def test_unmutated_blocks_consume_only_fresh_statistics(emulated, monkeypatch, read_cases, motion_case):
    ops = emulated
    seen = {}
    runs = [("read", c, sw) for c in "ABN" for sw in ({}, {"AX_FUSED": [False]}, {"FF_FUSED": [False]},
                                                      {"FOLD_ZERO_AUDIO": [False]})]
    runs += [("motion", None, sw) for sw in ({}, {"TB_FUSED": [False]}, {"FF_FUSED": [False], "FF_PROJ_FOLD_MM": [False]})]
    for block, combo, sw in runs:
        cs, P = _pick(block, combo, read_cases, motion_case)
        spy, _ = _spied(ops, monkeypatch, cs, P, **sw)
        assert spy.consumptions(), (block, combo, sw)
        spy.assert_fresh()
        for r in spy.consumptions():
            seen[r.op] = seen.get(r.op, 0) + 1
    print("consumptions per wrapped entry point:", seen)
    assert set(seen) == set(stats_spy.WRAPPED), seen


@pytest.mark.parametrize("name", sorted(PRODUCERS))
def test_a_producer_that_skips_stats_out_is_flagged(emulated, monkeypatch, read_cases, motion_case, name):
    ops = emulated
    block, combo, sw, mutant = PRODUCERS[name]
    cs, P = _pick(block, combo, read_cases, motion_case)
    spy, hits = _spied(ops, monkeypatch, cs, P, mutant=mutant, **sw)
    assert hits, f"{name}: the mutated producer was never called"
    stale = spy.stale()
    print(f"[{name}] {len(hits)} producer call(s) mutated, {len(stale)} stale of {len(spy.records)} checks, worst "
          f"{spy.worst():.3g} x bound\n{spy.report()}")
    assert stale and all(r.kind == "consumed" for r in stale)
    # the condition on the INPUTS: a stale statistic is no near miss (synth's weights: ~1000 x)
    assert spy.worst() >= 100.0


def test_the_census_flags_a_stale_consumption(emulated, monkeypatch, read_cases):
    """tests/census.py runs the same check on every checked call: clean on the unmutated block, and with the attn1
    out-projection's `stats_out` skipped the next consumers' rows fail with the detail "fresh:..." - and nothing else does
    (each restatement applies the statistics it is handed, so without the check this census is clean)."""
    import census
    ops = emulated
    cs, P = read_cases["A"]

    def recorded(mutant):
        with monkeypatch.context() as mp:
            _unwritten(ops, mp)
            cen = census.Census(ops)
            cen.install(mp)
            hits = _skip_producer(ops, mp, *mutant) if mutant else None
            with cen.recording():
                BC.run(cs, P)
        return cen, hits
    cen, _ = recorded(None)
    assert not cen.failures(), cen.report()
    assert any(r.op in stats_spy.WRAPPED for r in cen.rows.values())
    cen, hits = recorded(("gemm", "_self_attention"))
    bad = cen.failures()
    print(cen.report())
    assert hits and bad and all(r.detail.startswith("fresh:") and r.ratio >= 100.0 for r in bad), [(r.op, r.detail) for r in bad]


@pytest.fixture(scope="module")
def slab_case():
    """_feed_forward under slabs needs m % (2 * 65536) == 0 rows at C = 64: the FF of a motion module's weights on
    131072 rows (the slab loop is per row: nothing but the row count matters)."""
    cs = BC.make_case("motion", c=64, f=2, H=2, W=2, device="cpu", elem=EL)
    g = torch.Generator().manual_seed(5)
    h = (torch.randn(131072, 64, generator=g) * torch.rand(131072, 1, generator=g).add(0.5) +
         torch.randn(131072, 1, generator=g)).to(EL)
    return cs, BC.prepare(cs), h


def test_feed_forward_slabs_slice_fresh_statistics_and_keep_the_bits(emulated, monkeypatch, slab_case):
    """`_feed_forward`: "Rows are independent: same bits" - and each slab must be handed ITS rows' statistics."""
    from v_express_amd import blocks as B
    ops = emulated
    cs, P, h0 = slab_case

    def ff(slab_bytes, mutate=None, stats=True):
        h = h0.clone()
        with monkeypatch.context() as mp:
            mp.setattr(ops, "FF_SLAB_BYTES", [slab_bytes])
            _unwritten(ops, mp)
            spy = stats_spy.StatsSpy(ops).install(mp)
            hits = mutate(mp) if mutate else None
            calls = []
            inner = ops.geglu
            mp.setattr(ops, "geglu", lambda *a, **k: (calls.append(a[0].shape[0]), inner(*a, **k))[1])
            assert B._feed_forward(P, h, ops.row_stats(h) if stats else None) is None
        return h, spy, calls, hits
    whole, spy, calls, _ = ff(0)
    assert calls == [131072]
    spy.assert_fresh()
    slabbed, spy, calls, _ = ff(131072 * 256 * 2 // 2)             # half the GEGLU result per slab
    assert calls == [65536, 65536], calls
    spy.assert_fresh()
    assert torch.equal(slabbed, whole)

    # mutant 1: every slab is handed the first slab's statistics (the slice forgotten)
    def first_slab(mp):
        inner = ops.geglu
        hits = []

        def call(a, w, bias, out=None, ln=None):
            if ln is not None and a.data_ptr() != h_ptr[0]:
                hits.append(1)
                ln = (first[0], ln[1])
            elif ln is not None:
                first[0] = ln[0]
            return inner(a, w, bias, out=out, ln=ln)
        mp.setattr(ops, "geglu", call)
        return hits
    first, h_ptr = [None], [None]

    def ff_first_slab():
        h = h0.clone()
        h_ptr[0] = h.data_ptr()
        with monkeypatch.context() as mp:
            mp.setattr(ops, "FF_SLAB_BYTES", [131072 * 256 * 2 // 2])
            spy = stats_spy.StatsSpy(ops).install(mp)
            hits = first_slab(mp)
            B._feed_forward(P, h, ops.row_stats(h))
        return spy, hits
    spy, hits = ff_first_slab()
    assert hits and spy.stale() and spy.worst() >= 100.0, spy.report()
    # mutant 2: the statistics pass of _feed_forward itself (no producer handed any) is not made
    _, spy, calls, hits = ff(131072 * 256 * 2 // 2, mutate=lambda mp: _skip_producer(ops, mp, "row_stats", "_feed_forward"),
                             stats=False)
    print(f"[_feed_forward under slabs] skipped row_stats: worst {spy.worst():.3g} x bound")
    assert hits and calls == [65536, 65536] and spy.stale() and spy.worst() >= 100.0, spy.report()


def test_small_unet_forward_consumes_only_fresh_statistics(emulated, monkeypatch):
    """The whole `small_f4_8x8` forward with the forced-fusion switches of
    test_round3_fused_paths_host_composition_vs_reference_golden: every one of its 143 consumptions fresh."""
    import cases
    import v_express_amd as vx
    from v_express_amd import synth
    ops = emulated
    kw, F_, h, w, t = cases.FORWARD_CASES["small_f4_8x8"]
    cfg = cases.unet_cfg(kw)
    unet, refnet = vx.UNet3DConditionModel(cfg).to("cpu"), vx.UNet2DConditionModel(cfg).to("cpu")
    unet.load_state_dict(synth.unet3d_state_dict(cfg), strict=True)
    refnet.load_state_dict(synth.refnet_state_dict(cfg), strict=True)
    inp = synth.synthetic_inputs(cfg, F_, h, w)
    writer = vx.ReferenceAttentionControl(refnet, do_classifier_free_guidance=True, mode="write", fusion_blocks="full")
    reader = vx.ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", fusion_blocks="full",
                                          reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD)
    refnet(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768), return_dict=False)
    reader.update(writer, True)
    monkeypatch.setattr(ops, "gn_fold_applies", lambda m, hw, c, n: True)
    monkeypatch.setattr(ops, "qk_on_ring", lambda m, c: True)
    monkeypatch.setattr(ops, "tblock_fused_applies", lambda c, heads, f, hw: True)
    spy = stats_spy.StatsSpy(ops).install(monkeypatch)
    unet(inp["latents"].repeat(2, 1, 1, 1, 1), t, encoder_hidden_states=inp["audio_embeddings"].reshape(-1, 5, 768),
         kps_features=inp["kps_features"], return_dict=False)
    print(f"{len(spy.consumptions())} consumptions, worst {spy.worst():.3g} x bound\n{spy.report()}")
    assert len(spy.consumptions()) == 143
    spy.assert_fresh()


# ------------------------------------------------------------------------------------------------ 2. wiring mutants
# the emulation's geometries: the smallest at which every term of the block exists (8 heads, 32 groups -> C = 64)
WIRING = {
    "read_A": dict(kind="read", c=128, f=2, H=4, W=4, combo="A"),
    "read_B": dict(kind="read", c=128, f=2, H=4, W=4, combo="B"),
    "motion": dict(kind="motion", c=64, f=4, H=2, W=2),
    "resnet_skip": dict(kind="resnet", c=64, skip=64, cout=64, f=2, H=4, W=4),
    "upsample_phases": dict(kind="upsample", c=64, f=2, H=16, W=16),
}
_MEMO = {}


def _wiring(name, ops, monkeypatch):
    """(case, reference, e_emul) - computed once and shared (the emulation is deterministic)."""
    if name not in _MEMO:
        cs = BC.make_case(device="cpu", elem=EL, **WIRING[name])
        ref = BC.reference(cs)
        out = BC.emulated(cs, BC.prepare(cs), monkeypatch.context)
        _MEMO[name] = (cs, ref, BC.errors(out, ref))
    return _MEMO[name]


@pytest.mark.parametrize("name,mut", [(n, m) for n, v in WIRING.items() for m in BC.MUTANTS[v["kind"]]])
def test_wiring_mutant_of_the_reference_lies_beyond_twice_the_route_bound(emulated, monkeypatch, name, mut):
    cs, ref, e_emul = _wiring(name, emulated, monkeypatch)
    err = BC.errors(BC.reference(cs, mut), ref)
    print(f"[{name}] e_emul relL2 {e_emul[0]:.3g} max {e_emul[1]:.3g}; mutant {mut}: relL2 {err[0]:.3g} "
          f"({err[0] / e_emul[0]:.1f} x) max {err[1]:.3g} ({err[1] / e_emul[1]:.1f} x)")
    assert e_emul[0] > 0 and e_emul[1] > 0
    assert not BC.within(err, e_emul, 2 * 3.0), "the route bound 3 x e_emul would accept this wiring error"


# float32 products of K <= 4C = 256 terms (weights.fold_*): sqrt(K) 2^-24 ~ 1e-6 expected, K 2^-24 = 1.5e-5 at worst
FOLD_BIAS_REL = 1e-5


@pytest.mark.parametrize("kind", ["read", "motion"])
def test_load_time_folds_match_their_float64_statement_and_their_mutants_do_not(kind):
    """weights.fold_layernorm / fold_ff_proj / fold_groupnorm / the key fold, tensor by tensor: the folded weights to one
    rounding of the element type, the float32 biases to float32 accumulation, colsum = the sum of the ROUNDED weights.
    The fold mutants no block-level bound can see (block_wiring_cases.FOLD_MUTANTS) miss this bound by >= 100 x."""
    cs = BC.make_case(kind, c=64, f=2, H=4, W=4, device="cpu", elem=EL)
    got, want = BC.fold_tensors(BC.prepare(cs)), BC.fold_statements(cs)
    ulp = torch.finfo(EL).eps                    # spacing of the element type at 1: one rounding errs by half of it
    for name, ref in want.items():
        g = got[name].double()
        assert g.shape == ref.shape, name
        if name.endswith(".w"):
            # one rounding errs by at most half an ulp of each element: relative L2 <= ulp / 2; elementwise one ulp of the
            # largest element (fold_ff_proj rounds a float32 product Wp W2 whose small elements carry float32 cancellation)
            e = BC.errors(g, ref)
            assert e[0] <= ulp / 2 and e[1] <= ulp, (name, e)
            if name[:-2] + ".s" in got:
                s = got[name[:-2] + ".s"].double()
                assert ((s - g.sum(1)).abs() <= FOLD_BIAS_REL * g.abs().sum(1)).all(), name
        else:
            assert BC.errors(g, ref)[0] <= FOLD_BIAS_REL, (name, BC.errors(g, ref))
    for mut in BC.FOLD_MUTANTS[kind]:
        m = BC.fold_statements(cs, mut)
        worst = max(BC.errors(m[n], want[n])[0] for n in want)
        print(f"[{kind}] fold mutant {mut}: relL2 {worst:.3g} = {worst / FOLD_BIAS_REL:.0f} x the bound")
        assert worst >= 100 * FOLD_BIAS_REL, mut


def test_the_restated_upsample_phases_are_the_oracles_upsample(emulated, monkeypatch):
    cs, ref, _ = _wiring("upsample_phases", emulated, monkeypatch)
    got = BC.to_tokens(BC.upsample_phases_ref(BC.sd64(cs), BC.P_, BC.to_nchw(cs.x, cs.H, cs.W)))
    assert BC.errors(got, ref)[1] <= 1e-13


@pytest.mark.parametrize("name", ["resnet_skip", "resnet_shortcut", "resnet_plain", "downsample", "downsample_nogn", "upsample_3x3",
                                  "write", "bank_kv"])
def test_emulated_block_matches_the_float64_reference(emulated, monkeypatch, name):
    """The blocks without a mutant list of their own: the case module's reference and the emulated block agree to the
    rounding of the element type (a wrong layout in the CASES themselves would show here, on the CPU)."""
    geo = {"resnet_skip": WIRING["resnet_skip"], "resnet_shortcut": dict(kind="resnet", c=64, cout=128, f=2, H=4, W=4),
           "resnet_plain": dict(kind="resnet", c=64, f=2, H=4, W=4), "downsample": dict(kind="downsample", c=64, f=2, H=4, W=4),
           "downsample_nogn": dict(kind="downsample", c=64, f=2, H=4, W=4, gn_groups=0),
           "upsample_3x3": dict(kind="upsample", c=64, f=2, H=4, W=4), "write": dict(kind="write", c=64, f=2, H=4, W=4),
           "bank_kv": dict(kind="bank_kv", c=64, f=1, H=4, W=4)}[name]
    cs = BC.make_case(device="cpu", elem=EL, **geo)
    ref = BC.reference(cs)
    out = BC.emulated(cs, BC.prepare(cs), monkeypatch.context)
    # 2^-7: a few bf16 roundings (2^-9 each) on top of one another - far below any layout error (relative error ~1)
    if name == "bank_kv":
        e, ekmax = BC.bank_kv_errors(cs, out, ref)
        assert e[0] <= 2 ** -7 and ekmax <= 2 ** -7, (e, ekmax)
    elif name == "write":
        assert BC.errors(out[0], ref[0])[0] <= 2 ** -7 and BC.errors(out[1], ref[1])[0] <= 2 ** -7
    else:
        assert BC.errors(out, ref)[0] <= 2 ** -7, BC.errors(out, ref)
