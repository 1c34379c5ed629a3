"""The launch census (tests/census.py) has teeth, shown on the CPU: the small emulated forward of
test_host_emulated.py recorded with tests/fake_ops.py standing in for the kernels.  Clean, every launch matches its
restatement exactly and coverage is complete; with ONE signature's output perturbed (the last 64 rows of every launch of
one GEMM signature scaled by 1 + 2^-4) the census flags exactly that signature, while the forward still passes the
model-level golden bound of test_unet_forward_host_composition_vs_reference_golden (relative L2 <= 3e-2)."""
import os

import torch

import cases
import census
from loop_worker import emulated  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel_l2(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _forward(cen):
    import v_express_amd as vx
    from v_express_amd import synth
    kw, F, h, w, t = cases.FORWARD_CASES["small_f4_8x8"]
    cfg = cases.unet_cfg(kw)
    unet, refnet = vx.UNet3DConditionModel(cfg).to("cpu"), vx.UNet2DConditionModel(cfg).to("cpu")
    unet.load_state_dict(synth.unet3d_state_dict(cfg), strict=True)
    refnet.load_state_dict(synth.refnet_state_dict(cfg), strict=True)
    inp = synth.synthetic_inputs(cfg, F, h, w)
    writer = vx.ReferenceAttentionControl(refnet, do_classifier_free_guidance=True, mode="write", fusion_blocks="full")
    reader = vx.ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", fusion_blocks="full",
                                          reference_attention_weight=cases.W_REF, audio_attention_weight=cases.W_AUD)
    with cen.recording():
        cen.phase = "refnet+bank"
        refnet(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768), return_dict=False)
        reader.update(writer, True)
        cen.phase = "forward"
        x = inp["latents"].repeat(2, 1, 1, 1, 1)
        ehs = inp["audio_embeddings"].reshape(-1, 5, 768)
        return unet(x, t, encoder_hidden_states=ehs, kps_features=inp["kps_features"], return_dict=False)[0]


def test_census_passes_a_clean_run_and_flags_exactly_one_perturbed_signature(emulated, monkeypatch):
    ops = emulated
    gold = torch.load(os.path.join(GOLD, "forward_small_f4_8x8.pt"), weights_only=False)["pred"]
    with monkeypatch.context() as mp:
        cen = census.Census(ops)
        cen.install(mp)
        got = _forward(cen)
        print(cen.report())
    cen.assert_clean()
    # the restatement against itself: no error beyond float64 BLAS noise surfacing in a float32 output (ratio ~1e-10)
    assert max(r.ratio for r in cen.rows.values()) < 1e-6
    assert {r.phase for r in cen.rows.values()} == {"refnet+bank", "forward"}
    assert rel_l2(got, gold) <= 3e-2

    # the target: a GEMM signature of the forward that adds a residual, returns a fresh [m, n] tensor, has rows to spare
    # and leaves no GroupNorm statistics (scaling rows behind them would be caught as stale statistics instead)
    cands = [r.sig for r in cen.rows.values() if r.op == "gemm" and r.phase == "forward" and
             "residual" in dict(r.sig[2]) and "out" not in dict(r.sig[2]) and dict(r.sig[2]).get("gn") is None and
             r.sig[1][0][1][0] >= 256]
    assert cands
    target = cands[len(cands) // 2]
    real_gemm = ops.gemm
    hits = []

    def perturbed_gemm(*a, **k):
        y = real_gemm(*a, **k)
        if census.signature("gemm", a, k, ops) == target:
            hits.append(1)
            y[-64:] *= 1 + 2 ** -4
        return y
    monkeypatch.setattr(ops, "gemm", perturbed_gemm)
    cen2 = census.Census(ops)
    cen2.install(monkeypatch)
    got2 = _forward(cen2)
    print(cen2.report())
    flagged = {r.sig for r in cen2.failures()}
    worst = max(r.ratio for r in cen2.failures())
    r2 = rel_l2(got2, gold)
    print(f"perturbed {len(hits)} launches of {target[:2]}: census err/bound {worst:.3g}; forward relL2 vs golden "
          f"{r2:.4g} (clean {rel_l2(got, gold):.4g})")
    assert hits and flagged == {target}, flagged
    assert not cen2.coverage_errors()
    assert r2 <= 3e-2 and not torch.equal(got2, got)
