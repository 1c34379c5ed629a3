"""Init-video sampling on the host: `init_video` / `init_latents` / `mask` / `composite` of VExpressPipeline.__call__ and
`known=` of denoise under emulated kernels (tests/fake_ops.py + init_video_restated.known_blend /
vae_postprocess_composite) against float64 restatements of diffusers' img2img start and inpaint loop, for every sampler;
the exact identities of the blend, the untouched default path, the schedulers' noise_coefficients / add_noise, the
argument errors, and two gloo ranks against one process."""
import pytest
import torch

import cases
import dpm_restated as D
import init_video_restated as R
import loop_worker
from loop_restated import restated_loop
from loop_worker import (SEED, call_pipeline as _call, inputs as _inputs, oracle_unet as _oracle_unet,  # noqa: F401
                         rel_l2, sampler_kw, scheduler, small_pipe, spawn_gloo)

KINDS = ["ddim", "ddim-eta", "dpm", "euler-a"]


@pytest.fixture()
def emulated(monkeypatch):
    """The shared emulation plus the stand-in of the one kernel of this feature that is no loop op."""
    ops = loop_worker.emulate_kernels(monkeypatch)
    monkeypatch.setattr(ops, "vae_postprocess_composite", R.vae_postprocess_composite)
    return ops


def _init(F_, seed=5):
    return 0.5 * torch.randn(1, 4, F_, 8, 8, generator=torch.Generator().manual_seed(seed))


def _mask(F_, edge=32):
    """Pixel mask [F, 1, 64, 64]: frames 0-1 kept whole, rows above `edge` of the others kept (1 = regenerate)."""
    m = torch.ones(F_, 1, 64, 64)
    m[:2] = 0.0
    m[:, :, :edge] = 0.0
    return m


# ------------------------------------------------------------------------------------------------ (1) the feature
def test_init_latents_and_mask_change_the_clip_and_match_the_restatement(emulated, small_pipe):
    """F = 6 in windows of 4 with overlap 2, 5 DDIM steps, strength 0.6 (the loop starts at step index 2), random init
    latents, a mask that keeps frames 0-1 whole and the upper half of the others: the clip differs from the call without
    an init clip, matches the float64 restated loop over the oracle UNet (start, blend after every step, init itself
    after the last) and is closer to it than the no-init clip is.  Fails on a pipeline without the feature."""
    from oracle import loop as OL
    F_, cf, co, steps, strength = 6, 4, 2, 5, 0.6
    inp, init, mask = _inputs(F_), _init(F_), _mask(F_)
    plain = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, strength=strength)
    assert small_pipe.last_init == dict(begin_index=2, masked=False, blend_launches=0)
    got = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, strength=strength, init_latents=init, mask=mask)
    assert small_pipe.last_init == dict(begin_index=2, masked=True, blend_launches=4)
    assert torch.isfinite(got).all() and rel_l2(got, plain) > 1e-2
    m = R.box_mean(mask[:, 0])
    assert set(m.unique().tolist()) == {0.0, 1.0} and m[:2].sum() == 0 and m[2:, :32].sum() == 0 and m[2:, 32:].all()
    with torch.no_grad():
        ref = restated_loop(_oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), cases.GUIDANCE,
                            inp["kps_features"], inp["audio_embeddings"], steps, known=(init, inp["latents"], m, strength))
    r, r_plain = rel_l2(got, ref), rel_l2(plain, ref)
    print(f"[__call__ init_latents + mask, strength {strength}, emulated kernels, {steps} DDIM steps] relL2 vs restated "
          f"loop {r:.4g}; the clip without init: {r_plain:.4g}")
    assert r <= 5e-2 and r < r_plain
    # the kept cells are the init latents themselves
    keep = (m == 0).reshape(1, 1, F_, 8, 8).expand_as(got)
    assert torch.equal(got[keep], init[keep])


# ------------------------------------------------------------------------------------------------ (2) every sampler
@pytest.mark.parametrize("kind", KINDS)
def test_every_sampler_vs_restated_loop_and_kept_cells_after_every_step(emulated, small_pipe, kind):
    """reflected_F11_c4o2 (last window [8, 9, 10, 9]), 5 steps, strength 0.6, a mask whose pixel edge lies inside a latent
    row (latent mask values 0, 0.5, 1): against the restated loop, and after every step the cells with m == 0 equal
    a_{i+1} init + s_{i+1} noise in float64 (init after the last step) to the bound of vx_known_blend; Euler ancestral
    in the scheduler's own frame, where that is init + sigma_{i+1} noise."""
    from oracle import loop as OL
    F_, cf, co, _ = cases.PIPELINE_CASES["reflected_F11_c4o2"]
    steps, strength, b = 5, 0.6, 2
    inp, init, mask = _inputs(F_), _init(F_), _mask(F_, edge=28)
    noise = inp["latents"]
    m = R.box_mean(mask[:, 0])
    assert sorted(m.unique().tolist()) == [0.0, 0.5, 1.0]
    sched = scheduler(kind)
    keep = (m == 0).reshape(1, 1, F_, 8, 8).expand(1, 4, F_, 8, 8)
    seen = []

    def check(i, t, x):
        j = b + i + 1
        a, s = (1.0, 0.0) if j == steps else sched.noise_coefficients(j)
        scale = sched.frame_scale(j) if kind == "euler-a" else 1.0          # VP -> the scheduler's own frame
        want = R.blend(x, init, noise, None, a * scale, s * scale)
        bound = R.blend_bound(x, init, noise, None, a * scale, s * scale)
        err = (x.double() - want).abs()
        seen.append(i)
        assert (err[keep] <= bound[keep]).all(), (kind, i, (err[keep] - bound[keep]).max().item())
    got = _call(small_pipe, sched, inp, F_, steps, cf, co, strength=strength, init_latents=init, mask=mask,
                callback=check, **sampler_kw(kind, 0.5))
    assert seen == [0, 1, 2] and small_pipe.last_init == dict(begin_index=b, masked=True, blend_launches=4)
    with torch.no_grad():
        ref = restated_loop(_oracle_unet(inp), noise, OL.uniform_windows(F_, cf, co), cases.GUIDANCE,
                            inp["kps_features"], inp["audio_embeddings"], steps, kind, seed=SEED,
                            eta=0.5 if kind == "ddim-eta" else 0.0, known=(init, noise, m, strength))
    r = rel_l2(got, ref)
    print(f"[__call__ {kind}, init_latents + soft mask, strength {strength}, reflected_F11_c4o2, {steps} steps] relL2 vs "
          f"restated loop {r:.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2


# ------------------------------------------------------------------------------------------------ (3) exact identities
@pytest.mark.parametrize("kind", ["ddim", "dpm"])
def test_mask_of_ones_and_img2img_identities(emulated, small_pipe, kind):
    """m = 1 everywhere gives the bits of the maskless img2img call; img2img gives the bits of the call without an init
    clip that is handed the start latents as `latents` with the same strength (init_noise_sigma == 1)."""
    F_, cf, co, steps, strength = 6, 4, 2, 5, 0.6
    inp, init = _inputs(F_), _init(F_)
    img2img = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, strength=strength, init_latents=init)
    assert small_pipe.last_init == dict(begin_index=2, masked=False, blend_launches=1)
    ones = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, strength=strength, init_latents=init,
                 mask=torch.ones(1, 64, 64))
    assert small_pipe.last_init["blend_launches"] == 4 and torch.equal(ones, img2img)
    sched = scheduler(kind)
    sched.set_timesteps(steps)
    assert float(sched.init_noise_sigma) == 1.0
    start = torch.empty_like(init)
    emulated.known_blend(start, init, inp["latents"], None, *sched.noise_coefficients(2))
    today = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, strength=strength, latents=start)
    assert torch.equal(img2img, today)
    assert not torch.equal(img2img, _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, strength=strength))


@pytest.mark.parametrize("kind", KINDS)
def test_mask_of_zeros_returns_the_init_latents_exactly(emulated, small_pipe, kind):
    """At (a, s) = (1, 0), 0 * x + 1 * (1 * init + 0 * noise) is exact for finite x: a mask that keeps everything returns
    the init latents bit for bit, whatever the sampler did in between."""
    F_, cf, co, steps = 6, 4, 2, 3
    inp, init = _inputs(F_), _init(F_, seed=9)
    got = _call(small_pipe, scheduler(kind), inp, F_, steps, cf, co, strength=0.7, init_latents=init,
                mask=torch.zeros(F_, 1, 64, 64, dtype=torch.bool), **sampler_kw(kind, 0.5))
    assert small_pipe.last_init == dict(begin_index=1, masked=True, blend_launches=3)
    assert torch.equal(got, init)


def test_composite_through_decode(emulated, small_pipe, monkeypatch):
    """decode=True with init_video, a mask and composite: where M == 0 the video is init_video bit for bit, where M == 1
    the plain decode of the same latents; composite=False and init_latents alone decode plainly.  (The encoder is
    replaced by a function of the video here: the decoder-only VAE of the small pipeline has none.)"""
    F_, cf, co, steps = 4, 4, 2, 2
    inp = _inputs(F_)
    g = torch.Generator().manual_seed(3)
    video, init = torch.rand(1, 3, F_, 64, 64, generator=g), _init(F_)
    mask = torch.zeros(F_, 64, 64)
    mask[:, 40:] = 1.0
    monkeypatch.setattr(small_pipe.vae, "encode_video", lambda v, chunk=8: init.clone(), raising=False)
    kw = dict(strength=0.5, decode=True, output_device=None)
    lat = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, strength=0.5, init_latents=init, mask=mask)
    plain = small_pipe.decode_latents(lat)
    comp = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, init_video=video, mask=mask, **kw)
    M = mask[None, None].expand_as(comp) > 0
    assert torch.equal(comp[~M], video[~M]) and torch.equal(comp[M], plain[M]) and not torch.equal(comp, plain)
    off = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, init_video=video, mask=mask, composite=False,
                **kw)
    only_latents = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, init_latents=init, mask=mask, **kw)
    assert torch.equal(off, plain) and torch.equal(only_latents, plain)


# ------------------------------------------------------------------------------------------------ (4) defaults
@pytest.mark.parametrize("strength", [1.0, 0.4])
def test_defaults_launch_nothing_new(emulated, small_pipe, monkeypatch, strength):
    """Without an init clip the two new ops never run and the clip is the parent commit's path bit for bit: the same
    launches in the same order as prepare_latents + the plain loop, also for strength < 1 (the low-noise steps started
    from pure noise: vestigial, and unchanged)."""
    F_, cf, co, steps = 6, 4, 2, 5
    inp = _inputs(F_)

    def boom(*a, **k):
        raise AssertionError("a kernel of init-video sampling ran")
    monkeypatch.setattr(emulated, "known_blend", boom)
    monkeypatch.setattr(emulated, "vae_postprocess_composite", boom)
    trace = []
    for name in ("combine_units", "overlap_ddim_step", "vae_postprocess"):
        def spy(*a, _orig=getattr(emulated, name), _name=name, **k):
            trace.append(_name)
            return _orig(*a, **k)
        monkeypatch.setattr(emulated, name, spy)
    got = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, strength=strength, decode=True,
                output_device=None)
    n = min(int(steps * strength), steps)
    assert trace == ["combine_units", "overlap_ddim_step"] * n + ["vae_postprocess"]
    assert small_pipe.last_init == dict(begin_index=steps - n, masked=False, blend_launches=0)
    assert torch.isfinite(got).all() and got.shape == (1, 3, F_, 64, 64)

def test_default_clip_equals_the_loop_without_known(emulated, small_pipe, monkeypatch):
    """The same, on the latents, for the vestigial strength < 1 without an init clip: __call__ == the parent's pieces by
    hand - the caller's latents times init_noise_sigma, then the loop over the last int(N * strength) timesteps."""
    monkeypatch.setattr(emulated, "known_blend", None)
    from oracle import loop as OL
    from v_express_amd import ReferenceAttentionControl
    F_, cf, co, steps, strength = 6, 4, 2, 5, 0.4
    inp = _inputs(F_)
    got = _call(small_pipe, scheduler("ddim"), inp, F_, steps, cf, co, strength=strength)
    sched = scheduler("ddim")
    small_pipe.scheduler = sched
    writer = ReferenceAttentionControl(small_pipe.reference_net, do_classifier_free_guidance=True, mode="write",
                                       fusion_blocks="full")
    reader = ReferenceAttentionControl(small_pipe.denoising_unet, do_classifier_free_guidance=True, mode="read",
                                       fusion_blocks="full", reference_attention_weight=cases.W_REF,
                                       audio_attention_weight=cases.W_AUD)
    sched.set_timesteps(steps)
    small_pipe.reference_net(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768),
                             return_dict=False)
    reader.update(writer, True, dtype=small_pipe.dtype)
    lat = inp["latents"].clone()
    kps = emulated.ncfhw_to_nhwc(inp["kps_features"], 64).view(2, F_, 64, 64)
    audio = inp["audio_embeddings"].to(torch.bfloat16).contiguous()
    small_pipe.denoise(lat, kps, audio, sched.timesteps[3:].tolist(),
                       [list(w) for w in OL.uniform_windows(F_, cf, co)], cases.GUIDANCE, begin_index=3)
    reader.clear()
    writer.clear()
    assert torch.equal(got, lat)


# ------------------------------------------------------------------------------------------------ (5) coefficients
@pytest.mark.parametrize("n", [10, 25])
@pytest.mark.parametrize("kind", ["ddim", "dpm", "euler-a"])
def test_noise_coefficients_and_add_noise(kind, n):
    """(a_j, s_j) for j = 0 .. N against the float64 formulas on the float64 table.  The schedulers keep diffusers'
    float32 tables (a cumulative product of 1000 float32 factors: up to 1000 * 2^-24 = 6e-5 relative on abar, 3e-5 on its
    root, and the same absolute error after the zero-SNR shift), so the bound is 1e-4 absolute on numbers in [0, 1];
    a_j^2 + s_j^2 = 1 to 1e-6; add_noise is a_j x + s_j z (Euler ancestral, in its own frame: x + sigma_j z)."""
    sched = scheduler(kind)
    sched.set_timesteps(n)
    want = R.coefficients(kind, n)
    assert len(want) == n + 1
    for j in range(n + 1):
        a, s = sched.noise_coefficients(j)
        assert abs(a - want[j][0]) <= 1e-4 and abs(s - want[j][1]) <= 1e-4, (j, a, s, want[j])
        assert abs(a * a + s * s - 1.0) <= 1e-6 and a >= 0.0 and s >= 0.0
    assert sched.noise_coefficients(n) == (1.0, 0.0)
    if kind == "ddim":
        assert sched.noise_coefficients(0) == (0.0, 1.0)              # zero terminal SNR: strength 1 is pure noise
    else:
        assert 0.0 < sched.noise_coefficients(0)[0] < 1e-3            # the clamped table: sigma_0 = 4096
    with pytest.raises(IndexError):
        sched.noise_coefficients(n + 1)
    g = torch.Generator().manual_seed(n)
    x, z = torch.randn(2, 4, 3, 8, 8, generator=g), torch.randn(2, 4, 3, 8, 8, generator=g)
    for j in (0, 1, n // 2, n - 1):
        t = sched.timesteps[j]
        a, s = sched.noise_coefficients(j)
        got = sched.add_noise(x, z, t)
        if kind == "euler-a":
            sig = D.sigmas(n)[j]
            want_x = x.double() + sig * z.double()
            assert abs(s / a - sig) <= 1e-4 * sig
        else:
            want_x = a * x.double() + s * z.double()
        assert got.dtype == torch.float32 and got.shape == x.shape
        assert rel_l2(got, want_x) <= 1e-4
        # one timestep per sample of the batch
        pair = sched.add_noise(x, z, torch.stack([sched.timesteps[j], sched.timesteps[n - 1]]))
        assert torch.equal(pair[0], got[0]) and torch.equal(pair[1], sched.add_noise(x, z, sched.timesteps[n - 1])[1])


# ------------------------------------------------------------------------------------------------ (6) errors
def test_bad_init_arguments_fail_before_any_kernel(emulated, small_pipe, monkeypatch):
    def no_kernels(*a, **k):
        raise AssertionError("a kernel ran")
    for name in ("gather_latents", "combine_units", "known_blend", "vae_postprocess_composite", "overlap_ddim_step",
                 "ncfhw_to_nhwc", "groupnorm", "gemm"):
        monkeypatch.setattr(emulated, name, no_kernels)
    F_ = 4
    inp = _inputs(F_)
    init, video, mask = _init(F_), torch.rand(1, 3, F_, 64, 64), torch.ones(F_, 1, 64, 64)
    bad = [
        dict(mask=mask),                                                      # a mask without an init clip
        dict(init_video=video, init_latents=init),                            # both
        dict(init_latents=_init(F_ + 1)),                                     # frame count
        dict(init_latents=init[..., :7]),                                     # latent size
        dict(init_latents=init[0]),
        dict(init_video=video[:, :, :3]),                                     # frame count
        dict(init_video=video[..., :56]),                                     # width
        dict(init_video=video[:, :, :, :32]),                                 # height
        dict(init_latents=init, mask=torch.ones(F_ - 1, 1, 64, 64)),          # neither F nor 1 frames
        dict(init_latents=init, mask=torch.ones(F_, 64, 56)),
        dict(init_latents=init, mask=torch.ones(F_, 2, 64, 64)),
        dict(init_latents=init, mask=torch.ones(64, 64)),
        dict(init_latents=init, mask=torch.ones(F_, 1, 64, 64, dtype=torch.int64)),
        dict(init_latents=init, mask=mask * 1.5),                             # values outside [0, 1]
        dict(init_latents=init, mask=mask - 1.25),
        dict(init_latents=init, mask=mask * float("nan")),
        dict(init_video=video * 1.5),
        dict(init_video=video - 0.5),
    ]
    for kw in bad:
        with pytest.raises(ValueError, match="init|mask"):
            _call(small_pipe, scheduler("ddim"), inp, F_, 2, 4, 2, **kw)
    # denoise(known=...): shapes are checked before anything runs
    lat, noise = inp["latents"].clone(), inp["latents"]
    for known in ((init[:, :, :3], noise, None), (init, noise[..., :4], None), (init, noise, torch.ones(F_, 63)),
                  (init, noise, torch.ones(F_ + 1, 64))):
        with pytest.raises(ValueError, match="known"):
            small_pipe.denoise(lat, None, None, [999, 499], [[0, 1, 2, 3]], cases.GUIDANCE, known=known)
    # a valid init_video needs the encoder half: an error as well, not a silent plain run
    with pytest.raises(NotImplementedError, match="encoder"):
        _call(small_pipe, scheduler("ddim"), inp, F_, 2, 4, 2, init_video=video)
    # composite=True with init_latents alone is not an error (nothing to composite onto): checked in
    # test_composite_through_decode


def test_ops_wrappers_check_their_arguments():
    from v_express_amd import ops
    x, init, noise = torch.zeros(1, 4, 3, 2, 4), torch.zeros(1, 4, 3, 2, 4), torch.zeros(1, 4, 3, 2, 4)
    m = torch.ones(3, 8)
    with pytest.raises(TypeError, match="float32"):
        ops.known_blend(x, init.double(), noise, m, 1.0, 0.0)
    with pytest.raises(TypeError, match="contiguous"):
        ops.known_blend(x, init, noise.transpose(3, 4).contiguous().transpose(3, 4), m, 1.0, 0.0)
    with pytest.raises(TypeError, match="mask"):
        ops.known_blend(x, init, noise, m.bool(), 1.0, 0.0)
    with pytest.raises(ValueError, match="shape"):
        ops.known_blend(x, init[:, :, :2].contiguous(), noise, m, 1.0, 0.0)
    with pytest.raises(ValueError, match="mask"):
        ops.known_blend(x, init, noise, torch.ones(3, 4), 1.0, 0.0)
    with pytest.raises(ValueError, match="% 4"):
        ops.known_blend(x[..., :3].contiguous(), init[..., :3].contiguous(), noise[..., :3].contiguous(), None, 1.0, 0.0)
    for a, s in ((-0.1, 1.0), (1.0, -1e-3), (float("nan"), 0.0)):
        with pytest.raises(ValueError, match="negative"):
            ops.known_blend(x, init, noise, m, a, s)
    rows, video, M = torch.zeros(2 * 16, 8), torch.zeros(1, 3, 5, 4, 4), torch.ones(5, 16)
    with pytest.raises(TypeError, match="rows"):
        ops.vae_postprocess_composite(rows[:31], 2, 3, 4, 4, video, M)
    with pytest.raises(TypeError, match="init video"):
        ops.vae_postprocess_composite(rows, 2, 3, 4, 4, video.double(), M)
    with pytest.raises(ValueError, match="init video"):
        ops.vae_postprocess_composite(rows, 2, 3, 4, 4, video[..., :3].contiguous(), M)
    with pytest.raises(ValueError, match="mask"):
        ops.vae_postprocess_composite(rows, 2, 3, 4, 4, video, M[:2].contiguous())
    for frame0 in (-1, 4):
        with pytest.raises(ValueError, match="frames"):
            ops.vae_postprocess_composite(rows, 2, 3, 4, 4, video, M, frame0)


def test_mask_forms_and_the_latent_box_mean():
    from v_express_amd.pipeline import check_init, latent_mask
    init = torch.zeros(1, 4, 3, 8, 8)
    hard = torch.zeros(3, 64, 64, dtype=torch.bool)
    hard[:, 28:] = True
    for mask in (hard, hard[:, None], hard.half(), hard[:1].float(), hard[:1, None].double()):
        pm = check_init(None, init, mask, 3, 64, 64, 8)
        assert pm.dtype == torch.float32 and pm.shape == (mask.shape[0], 64, 64)
        lm = latent_mask(pm, 3, 8)
        assert lm.dtype == torch.float32 and lm.is_contiguous() and lm.shape == (3, 64)
        assert torch.equal(lm.double(), R.box_mean(hard.float()))
        assert sorted(lm.unique().tolist()) == [0.0, 0.5, 1.0]
    assert check_init(None, init, None, 3, 64, 64, 8) is None and check_init(None, None, None, 3, 64, 64, 8) is None


# ------------------------------------------------------------------------------------------------ (7) two ranks
@pytest.mark.parametrize("frame_shards,latent", [(None, 8), (2, 16)])
def test_two_gloo_ranks_are_bit_identical_to_one_process(emulated, frame_shards, latent):
    """F = 14, windows 8 / 2, init latents + mask, strength 0.6 (3 of 5 DDIM steps), no generator: each rank draws its
    own noise, rank 0's is broadcast as N(0,1) and the start latents and every blend are formed on every rank, so two
    gloo ranks (whole units, and every unit frame-sharded two ways) give the bits of one process, on both ranks."""
    import init_video_worker
    ref, _, _ = init_video_worker.run(None, latent, rank=0)
    if latent == 8:
        other, _, _ = init_video_worker.run(None, latent, rank=1)
        assert not torch.equal(ref, other)                       # rank 1's own draw would give another clip
    results = spawn_gloo(init_video_worker.main, 2, frame_shards, latent, timeout=900)
    for rank, (lat, sched, last) in enumerate(results):
        assert torch.isfinite(lat).all() and torch.equal(lat, ref), (rank, rel_l2(lat, ref))
        assert sched["frame_shards"] == (frame_shards or 1) and sched["units"] == 4 and sched["world"] == 2
        assert last == dict(begin_index=2, masked=True, blend_launches=4)
