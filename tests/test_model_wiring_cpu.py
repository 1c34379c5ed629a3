"""The wiring of v_express_amd/vae.py, wav2vec2.py and prologue.py on the CPU emulation (tests/fake_ops.py under the real
model files, blocks.py and weights.py), stage by stage against float64 (tests/model_wiring_cases.py).

1. The tapped call sequence and the scalar arguments of every model and geometry EQUAL the stage table.
2. Every stage's emulated output against its float64 reference ON THE PRODUCT'S OWN STAGE INPUT gives e_emul = (relative
   L2, max|err| / max|ref|); every wiring mutant of the reference lies beyond 2 x 3 x e_emul of its stage in at least one
   of the two (3 = the route bound of tests/test_gpu_model_wiring.py, 2 = the margin over it).  A stage of pure data
   movement has e_emul = 0: there any difference is beyond the bound.
3. The same mutants through the whole float64 model (`chain`) against the OLD end-to-end bound of the suite: which of them
   it lets through is printed.  Measured (small / full geometry, relative L2 movement of the model's output):
       VAE decode (bound 3e-2)   mid-attention to_q bias dropped 5.3e-3 / 2.1e-3
       VAE encode (2e-2)         mid-attention to_q bias dropped 1.1e-3 / 5.6e-4
       wav2vec2 (3e-2)           q_proj bias dropped 2.6e-3 / 5.8e-4; query scaled before its bias 7.6e-3 / 4.1e-3;
                                 positional-conv bias dropped 2.0e-2 / 1.9e-2 (passes at the small config only)
       VKpsGuider (2e-2)         blocks.2 bias dropped 7.5e-3 / 1.6e-2; conv_in bias dropped 5.6e-4 / 1.1e-3
       AudioProjection (2e-2)    none of the listed edits (they move the output by 0.18 ... 0.60)
   and every scalar-argument error (an eps of 1e-5 for 1e-6 moves the VAE by 1e-4), which no output bound sees at all.
4. The recorder is transparent, and an in-place call's recorded input is the value before the call.
5. The fused QKV biases (which carry the key bias no stage can see: the softmax cancels it) equal their float64 statement.

    python -m pytest tests/test_model_wiring_cpu.py -q -s        (prints e_emul per stage and the ratio of every mutant)
"""
import pytest
import torch

import model_wiring_cases as MC
import stage_tap
from loop_worker import emulated  # noqa: F401

EL = torch.bfloat16
CASES = [(m, g) for m, geos in MC.GEOMETRIES.items() for g in geos]
_MEMO = {}


def _case(model, geo, monkeypatch):
    """(case, recorded calls of the emulated model, its output, {stage: (got, ref, state)}) - once per geometry, shared and
    left unchanged (the emulation is deterministic)."""
    key = (model, geo)
    if key not in _MEMO:
        cs = MC.make_case(model, geo, device="cpu", elem=EL)
        calls, out = MC.emulated(cs, monkeypatch.context, stage_tap.StageTap)
        _MEMO[key] = (cs, calls, out)
    return _MEMO[key]


def _results(model, geo, monkeypatch):
    key = (model, geo, "results")
    if key not in _MEMO:
        cs, calls, _ = _case(model, geo, monkeypatch)
        MC.check_sequence(cs, calls)
        _MEMO[key] = MC.stage_results(cs, calls)
    return _MEMO[key]


@pytest.mark.parametrize("model,geo", CASES)
def test_call_sequence_and_scalar_arguments_equal_the_stage_table(emulated, monkeypatch, model, geo):
    cs, calls, _ = _case(model, geo, monkeypatch)
    MC.check_sequence(cs, calls)
    assert sum(len(st.calls) for st in cs.stages) == len(calls)


@pytest.mark.parametrize("model,geo", CASES)
def test_every_stage_has_a_measured_bound_and_every_mutant_lies_beyond_twice_it(emulated, monkeypatch, model, geo):
    cs, _, _ = _case(model, geo, monkeypatch)
    res = _results(model, geo, monkeypatch)
    e_emul = {}
    for st in cs.stages:
        got, ref, _ = res[st.name]
        e = e_emul[st.name] = MC.errors(got, ref)
        print(f"[{model}/{geo}] {st.name:<40} e_emul relL2 {e[0]:.3g} max {e[1]:.3g}")
        assert got.shape.numel() == ref.shape.numel() and torch.isfinite(got.float()).all()
        # a few roundings of the element type on top of one another - far below any layout error (relative error ~ 1)
        assert e[0] <= 2 ** -6, (st.name, e)
        assert st.exact or (e[0] > 0 and e[1] > 0), f"{st.name}: a stage without a rounding has no bound"
    weak = []
    for name, mut in MC.mutants(cs):
        st = next(s for s in cs.stages if s.name == name)
        _, ref, state = res[name]
        with torch.no_grad():
            err = MC.errors(st.ref(state, cs.w64, mut), ref)
        e = e_emul[name]
        ratio = tuple(a / b if b > 0 else float("inf") if a > 0 else 0.0 for a, b in zip(err, e))
        pinned = (name, mut) in MC.PINNED.get(model, {})
        print(f"[{model}/{geo}] mutant {name}:{mut}: relL2 {err[0]:.3g} ({ratio[0]:.1f} x) max {err[1]:.3g} ({ratio[1]:.1f} x)"
              + (f"   PINNED DIRECTLY: {MC.PINNED[model][(name, mut)]}" if pinned else ""))
        assert err[0] > 0
        if MC.within(err, e, 2 * 3.0) and not pinned:
            weak.append(f"{name}:{mut} {ratio[0]:.1f} x / {ratio[1]:.1f} x")
    assert not weak, f"the stage bound 3 x e_emul (with its margin of 2) would accept these wiring errors: {weak}"


@pytest.mark.parametrize("model,geo", [c for c in CASES if c[0] != "vae_decode_video"])
def test_mutants_against_the_old_end_to_end_bound(emulated, monkeypatch, model, geo):
    """What the suite's end-to-end bound alone lets through: the mutants through the WHOLE float64 model."""
    cs, _, out = _case(model, geo, monkeypatch)
    bound = MC.OLD_BOUND[model]
    clean = MC.chain(cs)
    e2e = MC.errors(out, clean)[0]
    print(f"[{model}/{geo}] emulated model against the chained float64 stages: relL2 {e2e:.3g} (the suite's bound: {bound})")
    assert e2e <= bound                                        # the chain IS the model the old tests compare with
    through = []
    for name, mut in MC.model_level_mutants(cs):
        moved = MC.errors(MC.chain(cs, (name, mut)), clean)[0]
        passes = moved + e2e <= bound
        print(f"[{model}/{geo}] {name}:{mut}: the output moves by {moved:.3g} -> {'PASSES' if passes else 'fails'} the old bound")
        if passes:
            through.append(f"{name}:{mut}")
    print(f"[{model}/{geo}] let through by {bound}: {through}")
    # (AudioProjection: every listed edit moves its output by 0.18 ... 0.60, past 2e-2; what its end-to-end bound hides is
    # the scalar arguments and the depth of the comparison, not one of these edits.  The other models each hide some.)
    assert through or model == "audio_projection", "the end-to-end bound catches every mutant here"


@pytest.mark.parametrize("model,geo", [("vae_decode", "small"), ("wav2vec2", "small"), ("audio_projection", "small")])
def test_the_recorder_is_transparent_and_keeps_inputs_from_before_the_call(emulated, monkeypatch, model, geo):
    cs, calls, out = _case(model, geo, monkeypatch)
    bare = MC.emulated(cs, monkeypatch.context)
    assert torch.equal(bare, out)
    inplace = [c for c in calls if c.after]
    assert inplace, "no in-place call in this model"
    for c in inplace:
        for k, v in c.after.items():
            assert not torch.equal(v, c.inputs[k]) or not torch.isfinite(c.inputs[k].float()).all()
    if model == "vae_decode":                                  # _self_attention(A, ln, h): h = a copy of the GroupNorm's INPUT
        i = next(i for i, c in enumerate(calls) if c.name == "blocks._self_attention")
        assert torch.equal(calls[i].inputs["h"].reshape(-1), calls[i - 1].inputs["x1"].reshape(-1))
        assert "h" in calls[i].after and "ln" not in calls[i].after
    if model == "audio_projection":                            # ops.gemm(a, wo, residual=lat, out=lat): lat before the add
        c = next(c for c in calls if c.name == "ops.gemm" and "residual" in c.inputs)
        assert torch.equal(c.inputs["residual"], c.inputs["out"]) and torch.equal(c.after["out"], c.out)


@pytest.mark.parametrize("model,geo", [("vae_decode", "small"), ("vae_decode", "full"), ("wav2vec2", "small"), ("wav2vec2", "base")])
def test_fused_qkv_biases_equal_their_float64_statement(emulated, monkeypatch, model, geo):
    """The key bias is invisible in every stage output (model_wiring_cases: equivalent by construction); the prepared
    tensor is where it shows.  float32 copies of float32 biases: 1e-5 (block wiring: FOLD_BIAS_REL) is generous."""
    cs, _, _ = _case(model, geo, monkeypatch)
    pins = MC.bqkv_statement(cs)
    assert pins
    for name, (got, want) in pins.items():
        assert got.dtype == torch.float32 and got.shape == want.shape, name
        assert MC.errors(got, want)[0] <= 1e-5, (name, MC.errors(got, want))
        c = want.shape[0] // 3
        dropped = want.clone()
        dropped[c:2 * c] = 0                                   # the equivalent edit: visible here
        assert MC.errors(dropped, want)[0] >= 100 * 1e-5, name
    # the mutants of the query bias that no stage bound can see (model_wiring_cases.PINNED) miss THIS bound by >= 100 x
    for (stage_name, mut), _ in MC.PINNED[model].items():
        e = min(MC.errors(bad, pins[name][1])[0] for name, (_, bad) in MC.bqkv_statement(cs, mut).items())
        print(f"[{model}/{geo}] pinned mutant {stage_name}:{mut}: bqkv moves by relL2 >= {e:.3g} = {e / 1e-5:.0f} x the bound")
        assert e >= 100 * 1e-5, mut
