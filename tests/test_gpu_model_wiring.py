"""v_express_amd/vae.py, wav2vec2.py and prologue.py on a real MI355X, stage by stage against float64.

Each case runs one model through its own entry point on both element libraries under tests/stage_tap.py and
tests/stats_spy.py (tests/model_wiring_cases.py holds the stage tables, the float64 references and the geometries).  Per case:

* the tapped call sequence and its scalar arguments EQUAL the stage table (a dropped, added or reordered call, a wrong eps,
  head count, activation code, stride or padding fails by stage name);
* every stage is within 3 x e_emul of its float64 reference ON ITS OWN RECORDED INPUT, in relative L2 and in max|err| /
  max|ref|; e_emul is measured in the same run: the same model through tests/fake_ops.py (float64 arithmetic, element-type
  rounding at every kernel boundary) on the same seeds, each emulated stage against float64 on ITS recorded input.  A
  stage of pure data movement has e_emul = 0 and must be bit-equal; tests/test_model_wiring_cpu.py shows that every wiring
  mutant of a reference lies beyond 2 x 3 x e_emul (or pins the tensor it corrupts);
* the routes, asserted: which upsampler ran as four 2x2 phases and which with the upsampling in its gather
  (`ops.block_paths()`), the attention kernel of the VAE's one head (d = 512 at the sd-vae-ft-mse widths), the G per-group
  positional GEMMs of wav2vec2, `vx_small_kv_attention` over 15 keys, no launch on the persistent kernel (no width here is
  a multiple of its 320-column tile) and no split-K launch (`ops._splitk` takes frames of at most 64 rows; the smallest
  frame here has 96);
* freshness: no stale LayerNorm row statistics (stats_spy), and wherever a GroupNorm is handed partial sums that a producer
  left on its input (`ops.keep_gn`: a resnet's conv2 for the next resnet's norm1 / the mid attention's group_norm) they are
  the sums of the values it normalises (census.STAT_BOUNDS["gn_sums"]);
* the identities the code claims, bit for bit: decode_video / encode_video in chunks of 1, 2 and all frames, each frame
  decoded / encoded / guided alone = its rows of the batched call, AudioProjection on one frame = its row of the batch.

    python -m pytest tests/test_gpu_model_wiring.py -m gpu -q -s      (prints e_emul and the kernels' error per stage)

Measured on an MI355X (also LABNOTES.md 19), 234 stages per element type, 30 tests in 10 s.  Per model and geometry: the range
of e_emul over its stages (relative L2; the stages of pure data movement, e_emul = 0 and bit-equal, left out; 2.6e-08 is
vx_vae_postprocess in float32) and the worst ratio kernels / e_emul in either measure with the stage that has it - every stage
sits at no more than 1.07 x in relative L2 and 1.96 x in the max measure, so nothing had to be added to the emulation:

    model / geometry           stages   bf16: e_emul relL2 (min ... max)   worst ratio relL2 / max (stage)          f16: e_emul relL2 (min ... max)   worst ratio relL2 / max (stage)
    vae_decode/small              22   0.00166 ... 0.00405   1.00 / 1.51 (up.0.resnets.2)                            0.000208 ... 0.000504   1.01 / 1.15 (up.3.resnets.2)
    vae_decode/full               22   0.00166 ... 0.00386   1.01 / 1.23 (up.2.resnets.0)                            0.000208 ... 0.000487   1.00 / 1.17 (up.3.resnets.1)
    vae_decode_video/small        44   2.57e-08 ... 0.00403  1.01 / 1.37 (chunk2.up.3.resnets.1)                     2.56e-08 ... 0.000504   1.01 / 1.42 (chunk2.mid.resnets.1)
    vae_encode/small              18   0.00154 ... 0.00398   1.02 / 1.17 (down.3.resnets.0)                          0.000193 ... 0.000498   1.01 / 1.55 (conv_norm_out+conv_out+quant_conv)
    vae_encode/full               18   0.00154 ... 0.004     1.00 / 1.22 (down.2.resnets.1)                          0.000193 ... 0.000499   1.05 / 1.10 (down.2.resnets.0)
    wav2vec2/small                18   0.00165 ... 0.00278   1.02 / 1.08 (conv4)                                     0.000195 ... 0.000342   1.07 / 1.66 (conv4)
    wav2vec2/base                 58   0.00163 ... 0.00285   1.01 / 1.28 (layers.8.layer_norm)                       0.000203 ... 0.00036    1.02 / 1.96 (layers.0.final_layer_norm)
    audio_projection/small         6   0.00232 ... 0.0034    1.00 / 1.00 (pos_emb+proj_in)                           0.000289 ... 0.000433   1.03 / 1.21 (proj_out+norm_out)
    audio_projection/full         10   0.00198 ... 0.00388   1.01 / 1.11 (layers.2.feed_forward)                     0.000247 ... 0.000487   1.01 / 1.06 (layers.2.attention)
    kps_guider/small               9   0.00148 ... 0.00227   1.00 / 1.00 (layout_in)                                 0.000184 ... 0.000278   1.00 / 1.06 (conv_out)
    kps_guider/full                9   0.00148 ... 0.00227   1.00 / 1.00 (layout_in)                                 0.000184 ... 0.000278   1.00 / 1.01 (blocks.5)
"""
import pytest
import torch

import census
import model_wiring_cases as MC
import stage_tap
import stats_spy

pytestmark = pytest.mark.gpu
ELEMS = (torch.bfloat16, torch.float16)
EL_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
FACTOR = 3.0
CASES = [(m, g) for m, geos in MC.GEOMETRIES.items() for g in geos]


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from v_express_amd import blocks as b, lib as L, ops as o
    torch.cuda.set_device(0)
    return L, o, b


@pytest.fixture(params=ELEMS, ids=lambda e: EL_NAME[e])
def ops_el(mods, request):
    L, o, b = mods
    with L.element_type(request.param):
        yield o, b, request.param
    o.clear_caches()


_CASE = {}


def case_of(model, geo, el, **kw):
    """The case (model on the GPU in `el`, inputs, stage table, float64 weights) - built once and left unchanged."""
    key = (model, geo, el, tuple(sorted(kw.items())))
    if key not in _CASE:
        _CASE[key] = MC.make_case(model, geo, device="cuda", elem=el, **kw)
    return _CASE[key]


class GnSpy:
    """Every `ops.groupnorm` call (nested ones too): where the input carries a producer's partial sums, their distance from
    the sums of the values about to be normalised, in units of census.STAT_BOUNDS["gn_sums"]."""

    def __init__(self, ops):
        self.ops, self.calls, self.ratios = ops, 0, []

    def install(self, mp):
        real = self.ops.groupnorm

        def call(x1, *a, **k):
            self.calls += 1
            st = self.ops.gn_of(x1) if k.get("x2") is None else None
            if st is not None:
                assert st.fits(k["frames"], k["hw"], k["groups"], x1.shape[-1]), "GroupNorm sums of another geometry"
                x = x1.double().view(st.frames, st.hw, st.groups, -1)
                want = torch.stack([x.sum(dim=(1, 3)), (x * x).sum(dim=(1, 3))], dim=-1)
                self.ratios.append(census._stat_ratio(census._gn_sums(st.ws, st.frames, st.groups, st.hw, st.c), want,
                                                      census.STAT_BOUNDS["gn_sums"])[0])
            return real(x1, *a, **k)
        call.__wrapped__ = real
        mp.setattr(self.ops, "groupnorm", call)
        return self


def run_kernels(ops, blocks, mp, cs):
    """-> (tapped calls, output, stats spy, GroupNorm spy, block paths, GEMM launches as text, other kernels as (name, symbol))."""
    with mp.context() as m:
        spy = stats_spy.StatsSpy(ops).install(m)
        gn = GnSpy(ops).install(m)
        tap = stage_tap.StageTap(ops, blocks).install(m)
        ops.BLOCK_PATHS.clear()
        with ops.GemmProfile() as gp, ops.OpProfile() as op:
            calls, out = MC.record(cs, tap)
        torch.cuda.synchronize()
    gemms = [(tuple(r[4]), f"{r[4][0]}x{r[4][1]}x{r[4][2]} {r[3]} = {r[5]}") for r in gp.records]
    return calls, out, spy, gn, ops.block_paths(), gemms, [(r[0], r[5]) for r in op.records]


def check_routes(cs, calls, paths, gemms, others):
    name = f"{cs.model}/{cs.geo}"
    texts = [t for _, t in gemms]
    assert not [t for t in texts if "gemm_ring" in t], f"{name}: a launch on the persistent kernel: {sorted(set(texts))}"
    assert not [t for t in texts if "splitk" in t], f"{name}: a split-K launch: {sorted(set(texts))}"
    kernels = {n for n, _ in others}
    if cs.model in ("vae_decode", "vae_decode_video"):
        ups = {k.split("hw_in=")[1].split()[0]: v for k, v in paths.items() if k.startswith("upsample_conv ")}
        lat = MC.LAT_H * MC.LAT_W
        assert ops_min_hw() == 256 and set(ups) == {str(lat), str(4 * lat), str(16 * lat)}, ups
        assert ups[str(lat)].startswith("one 3x3"), ups          # 96 pixels: below ops.UPSAMPLE_PHASES_MIN_HW
        assert ups[str(4 * lat)].startswith("four 2x2") and ups[str(16 * lat)].startswith("four 2x2"), ups
        phases = [t for sh, t in gemms if sh[2] == 4 * sh[1]]                  # 2x2 convolutions C -> C: K = 4 C
        assert phases and len(phases) % 8 == 0, f"{name}: {len(phases)} phase launches (two upsamplers x four phases per call)"
    if cs.model.startswith("vae"):
        # vae.py calls resnet_block WITHOUT `items`: the library picks the tile itself, and at these widths (32 ... 512, none
        # a multiple of 160) that is the 128 x 128 tile for every launch wider than 32 columns and the 256 x 32 tile below -
        # whatever the row count.  Those tiles write no GroupNorm partial sums (vx_gemm_gn_slabs), so every GroupNorm of the
        # VAE makes its own statistics pass and none is handed a producer's sums (the emulation, which emits them whenever
        # asked, checks their freshness on the CPU: fake_ops.groupnorm).
        for sh, t in gemms:
            want = "gemm_kernel<256x32x64,4w," if sh[1] <= 32 else "gemm_kernel<128x128x64,4w,"
            assert f" {want}" in t, f"{name}: {t}"
        assert "groupnorm_stats+apply" in kernels and "groupnorm_apply" not in kernels, kernels
        d = cs.cfg.block_out_channels[-1]
        want = {512: "attn_kernel<16, 32, 1, false, 1>", 128: "attn_kernel<4, 8, 2, true, 2>"}[d]
        got = sorted({s for n, s in others if n == "attention"})
        assert got == [want], f"{name}: the one-head attention (d = {d}) ran {got}, not {want}"
    if cs.model == "wav2vec2":
        cfg = cs.cfg
        G, cg = cfg.num_conv_pos_embedding_groups, cfg.hidden_size // cfg.num_conv_pos_embedding_groups
        pos = [t for sh, t in gemms if sh[1] == cg and sh[2] == cfg.num_conv_pos_embeddings * cg]
        assert len(pos) == G, f"{name}: {len(pos)} positional launches of N = {cg}, K = {cfg.num_conv_pos_embeddings * cg}; {G} groups"
        outs = [c for c in calls if c.name == "ops.gemm" and "residual" in c.inputs and c.inputs["out"].shape[1] == cg]
        assert len(outs) == G and all(c.out.shape == (c.inputs["a"].shape[0], cg) for c in outs)      # column slices of y
    if cs.model == "audio_projection":
        kv = [c for c in calls if c.name == "ops.small_kv_attention"]
        assert len(kv) == cs.cfg.depth and all(c.scalars["n_kv"] == 15 for c in kv)
        assert "small_kv_attention" in kernels, kernels


def ops_min_hw():
    from v_express_amd import ops
    return ops.UPSAMPLE_PHASES_MIN_HW[0]


@pytest.mark.parametrize("model,geo", CASES)
def test_every_stage_on_its_own_input_against_float64(ops_el, monkeypatch, model, geo):
    ops, blocks, el = ops_el
    cs = case_of(model, geo, el)
    calls_e, _ = MC.emulated(cs, monkeypatch.context, stage_tap.StageTap)
    calls, out, spy, gn, paths, gemms, others = run_kernels(ops, blocks, monkeypatch, cs)
    assert torch.isfinite(out.float()).all()
    MC.check_sequence(cs, calls)
    MC.check_sequence(cs, calls_e)
    for _, t in sorted(set(gemms)):
        print(f"    [{model}/{geo} {EL_NAME[el]}] gemm {t}")
    print(f"    [{model}/{geo} {EL_NAME[el]}] other kernels {sorted(set(others))}")
    print(f"    [{model}/{geo} {EL_NAME[el]}] paths {paths}")
    check_routes(cs, calls, paths, gemms, others)
    spy.assert_fresh()
    print(f"    [{model}/{geo} {EL_NAME[el]}] {gn.calls} GroupNorm calls, {len(gn.ratios)} handed a producer's sums, worst "
          f"{max(gn.ratios, default=0.0):.3g} x their bound")
    assert all(r <= 1.0 for r in gn.ratios), f"stale GroupNorm partial sums: {gn.ratios}"
    res, res_e = MC.stage_results(cs, calls), MC.stage_results(cs, calls_e)
    bad = []
    for st in cs.stages:
        (got, ref, _), (got_e, ref_e, _) = res[st.name], res_e[st.name]
        err, e_emul = MC.errors(got, ref), MC.errors(got_e, ref_e)
        r = tuple(a / b if b > 0 else (0.0 if a == 0 else float("inf")) for a, b in zip(err, e_emul))
        print(f"[{model}/{geo} {st.name} {EL_NAME[el]}] e_emul {e_emul[0]:.3g} / {e_emul[1]:.3g}   kernels {err[0]:.3g} / "
              f"{err[1]:.3g}  ({r[0]:.2f} x / {r[1]:.2f} x)")
        # the emulation runs the PRODUCT's host code: a wiring error there inflates e_emul itself.  A stage is a few roundings
        # of the element type (measured: up to 0.5 eps); at 2 eps the emulation itself is wired wrongly (a layout error: ~ 1)
        if e_emul[0] > 2 * torch.finfo(el).eps:
            bad.append(f"{st.name}: the EMULATED stage is {e_emul} from float64: the host code is wired wrongly")
        if not MC.within(err, e_emul, FACTOR):
            bad.append(f"{st.name}: kernels {err} beyond {FACTOR} x e_emul {e_emul}")
    assert not bad, f"{model}/{geo}: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------ identities, bit for bit
def test_decode_video_in_chunks_and_frame_by_frame(ops_el):
    """decode_video with chunk 1, 2 and all frames, and each frame decoded alone = its rows of the batched `decode`."""
    ops, _, el = ops_el
    cs = case_of("vae_decode_video", "small", el)
    lat = cs.inputs["latents"]
    whole = cs.net.decode_video(lat, chunk=MC.VIDEO_FRAMES)
    for chunk in (1, 2):
        assert torch.equal(cs.net.decode_video(lat, chunk=chunk), whole), f"decode_video: chunk {chunk} differs from one call"
    cd = case_of("vae_decode", "small", el)
    z = cd.inputs["x"]
    batched = cd.net.decode(z).sample
    for i in range(z.shape[0]):
        assert torch.equal(cd.net.decode(z[i:i + 1]).sample, batched[i:i + 1]), f"decode: frame {i} alone differs from its rows"


def test_encode_video_in_chunks_and_frame_by_frame(ops_el):
    """encode_video: "the chunk size does not change a bit"; it is the posterior mean of 2 x - 1 times the scaling factor."""
    ops, _, el = ops_el
    cs = case_of("vae_encode", "small", el)
    x = cs.inputs["x"]                                                         # [n, 3, H, W] in [-1, 1]
    video = ((x + 1.0) / 2.0).permute(1, 0, 2, 3)[None].contiguous()           # [1, 3, F, H, W] in [0, 1]
    whole = cs.net.encode_video(video, chunk=x.shape[0])
    assert torch.equal(cs.net.encode_video(video, chunk=1), whole)
    frames = video[0].permute(1, 0, 2, 3)
    mean = cs.net.encode(2.0 * frames - 1.0).latent_dist.mean
    assert torch.equal(whole, (mean * cs.cfg.scaling_factor).permute(1, 0, 2, 3)[None])
    for i in range(x.shape[0]):
        assert torch.equal(cs.net.encode(x[i:i + 1]).latent_dist.mean, cs.net.encode(x).latent_dist.mean[i:i + 1]), \
            f"encode: frame {i} alone differs from its rows"


@pytest.mark.parametrize("geo", ["small", "full"])
def test_guider_and_audio_projection_one_frame_alone(ops_el, geo):
    ops, _, el = ops_el
    cs = case_of("kps_guider", geo, el)
    x = cs.inputs["x"]
    batched = cs.net.forward_tokens(x)[0]
    for i in range(x.shape[2]):
        assert torch.equal(cs.net.forward_tokens(x[:, :, i:i + 1])[0], batched[i:i + 1]), f"guider: frame {i} alone differs"
    ca = case_of("audio_projection", geo, el)
    a = ca.inputs["x"]
    batched = ca.net(a)
    for i in range(a.shape[0]):
        assert torch.equal(ca.net(a[i:i + 1]), batched[i:i + 1]), f"AudioProjection: frame {i} alone differs from its row"
