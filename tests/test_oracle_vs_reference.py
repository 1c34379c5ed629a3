"""Tier A == Tier B: the reference's own modules (imported unmodified) against oracle/, through what
tests/make_golden.py live recorded from them in tests/golden/reference_live.pt (outputs on seeded inputs, the
`state_dict()` key / shape schemas, the context scheduler's windows over a parameter grid).  Also pins the synthetic
state_dict schema to the reference's own keys / shapes."""
import os

import torch

import cases
from oracle import unet as OU
from v_express_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _live():
    return torch.load(os.path.join(GOLD, "reference_live.pt"), weights_only=False)


def _same_schema(schema, sd):
    """What a strict `load_state_dict` of `sd` into the recorded module checks: the same keys, the same shapes."""
    return set(schema) == set(sd) and all(tuple(schema[k]) == tuple(sd[k].shape) for k in sd)


def test_schema_and_forward_against_live_reference():
    g = _live()
    kw = cases.SMALL
    cfg, ocfg = cases.unet_cfg(kw), cases.oracle_cfg(kw)
    sd3, sd2 = synth.unet3d_state_dict(cfg, seed=7), synth.refnet_state_dict(cfg, seed=8)
    assert _same_schema(g["unet3d_schema"], sd3) and _same_schema(g["refnet_schema"], sd2)
    assert len(sd3) == 1386 and len(sd2) == 684
    inp = synth.synthetic_inputs(cfg, 6, 8, 16, seed=9)
    frames = [1, 2, 3, 5]
    pred, banks = g["forward_pred"], g["forward_banks"]
    ob = OU.refnet_banks(sd2, ocfg, inp["ref_latents"])
    assert set(ob) == set(banks)
    assert max((ob[k] - banks[k]).abs().max().item() for k in ob) < 5e-5
    x = inp["latents"][:, :, frames].repeat(2, 1, 1, 1, 1)
    ehs = inp["audio_embeddings"][:, frames].reshape(-1, 5, 768)
    o = OU.unet3d_forward(sd3, ocfg, x, 519, ehs, inp["kps_features"][:, :, frames], OU.reader_banks(ob), 0.9, 2.0)
    assert (o - pred).abs().max().item() < 2e-5


def test_uncond_reference_attention_is_out_bias():
    """attention against an all-zero bank returns exactly to_out.bias."""
    from oracle import leaf as L
    g = torch.Generator().manual_seed(0)
    w = {"a.to_q.weight": torch.randn(64, 64, generator=g), "a.to_k.weight": torch.randn(64, 64, generator=g),
         "a.to_v.weight": torch.randn(64, 64, generator=g), "a.to_out.0.weight": torch.randn(64, 64, generator=g),
         "a.to_out.0.bias": torch.randn(64, generator=g)}
    x = torch.randn(2, 16, 64, generator=g)
    o = L.attention(w, "a", x, torch.zeros(2, 16, 64), 8)
    assert torch.allclose(o, w["a.to_out.0.bias"].expand_as(o), atol=1e-6)


def test_prologue_models_against_live_reference():
    """VKpsGuider / AudioProjection (reference modules, unmodified) and AutoencoderKL.encode (diffusers stand-in) vs
    oracle/prologue.py on the same synthetic weights (reference outputs: tests/golden/prologue.pt); the recorded
    `state_dict()` schemas pin the key schema as a strict load would."""
    import oracle
    from oracle import prologue as OP
    g, gp = _live(), torch.load(os.path.join(GOLD, "prologue.pt"), weights_only=False)
    inp = cases.prologue_inputs()
    # --- VKpsGuider
    for tag, kw in (("small", cases.KPS_SMALL), ("full", {})):
        kcfg = synth.KpsGuiderConfig(**kw)
        sd = synth.kps_guider_state_dict(kcfg)
        assert _same_schema(g[f"kps_schema_{tag}"], sd)
        want = gp[f"kps_{tag}"]                                                    # [1, C, f, h/8, w/8]
        b, c, f, H, W = inp["kps_images"].shape
        got = OP.kps_guider(sd, inp["kps_images"].permute(0, 2, 1, 3, 4).reshape(b * f, c, H, W))
        got = got.reshape(b, f, -1, H // 8, W // 8).permute(0, 2, 1, 3, 4)
        assert (got - want).abs().max().item() < 1e-5
    # --- AudioProjection
    for tag, kw, key in (("small", cases.AUDIO_SMALL, "audio_windows_small"), ("full", {}, "audio_windows_full")):
        acfg = synth.AudioProjectionConfig(**kw)
        sd = synth.audio_projection_state_dict(acfg)
        assert _same_schema(g[f"audio_schema_{tag}"], sd)
        want = gp[f"audio_{tag}"]
        got = OP.audio_projection(sd, inp[key], acfg.depth, acfg.heads)
        assert (got - want).abs().max().item() < 2e-5
    # --- VAE encode (mean): the encoder half of the full AutoencoderKL schema
    vcfg = synth.VaeConfig(**cases.SMALL_VAE)
    sdv = synth.vae_encoder_state_dict(vcfg)
    schema = g["vae_schema"]
    missing = set(schema) - set(sdv)
    assert all(k.startswith(("decoder.", "post_quant_conv.")) for k in missing) and set(sdv) <= set(schema)
    assert all(tuple(schema[k]) == tuple(v.shape) for k, v in sdv.items())
    want = gp["vae_mean"]
    got = OP.vae_encode_mean(sdv, oracle.VaeConfig(**cases.SMALL_VAE), inp["ref_image"])
    assert (got - want).abs().max().item() < 2e-5


def test_audio_windows_and_median_against_live_reference():
    """The audio-window construction of prepare_audio_embeddings (executed from the reference pipeline's own source
    lines) and pipelines/utils.py:median_filter_3d vs the oracle restatements: bit-exact (reference outputs:
    tests/golden/prologue.pt)."""
    from oracle import prologue as OP
    gp = torch.load(os.path.join(GOLD, "prologue.pt"), weights_only=False)
    inp = cases.prologue_inputs()
    got = OP.median_filter_3d(inp["video"], 3)
    assert torch.equal(got, gp["median"])
    F_, pad = 7, 2
    got = OP.audio_windows(inp["wav2vec_states"], F_, pad)
    assert torch.equal(got, gp["audio_windows_F7"])


def test_context_scheduler_own_formulation_equals_the_reference_for_all_parameters():
    """v_express_amd.context.uniform (round 3: an own formulation - dilation levels, radical-inverse offset, reflection -
    instead of a transcription) against the reference's pipelines/context.py:22-60 (its windows recorded as digests in
    tests/golden/reference_live.pt) for every combination of clip length, window size, overlap, stride, closed_loop and
    step on a grid that covers one-window clips, exact multiples, reflected last windows and the multi-level
    (context_stride > 1) schedules the pipeline itself never asks for."""
    from v_express_amd import context as C
    g = _live()
    grid = list(cases.context_grid())
    assert g["context_grid"].tolist() == [[F, size, ov, stride, int(closed), step]
                                          for F, size, ov, stride, closed, step in grid]
    n = 0
    for (F, size, ov, stride, closed, step), want in zip(grid, g["context_digests"].tolist()):
        b = list(C.uniform(step, F, size, stride, ov, closed))
        assert cases.window_digest(b) == want, (F, size, ov, stride, closed, step)
        n += 1
    assert n > 10000
    for v, want in g["ordered_halving"].items():
        assert C.radical_inverse_base2(v) == want
