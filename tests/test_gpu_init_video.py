"""Init-video sampling on the MI355X: `vx_known_blend` and `vx_vae_postprocess_composite` (both element libraries)
against float64 and their exact identities, `AutoencoderKL.encode_video` against the oracle encoder, and
VExpressPipeline with init latents / an init video, a mask and the pixel composite against the restated loop over the
oracle UNet and the bit-exact identities of the blend."""
import pytest
import torch

import cases
import init_video_restated as R
from loop_restated import restated_loop
from loop_worker import (build_small, call_pipeline, cosine, dev, inputs, oracle_on_cpu,  # noqa: F401
                         oracle_unet, rel_l2, scheduler)

pytestmark = pytest.mark.gpu

ELEMS = [torch.bfloat16, torch.float16]


def table25():
    """(a, s) of a real 25-step DDIM schedule: every level, with (0, 1) at j = 0 and (1, 0) at j = 25."""
    from v_express_amd import DDIMScheduler
    sched = DDIMScheduler(**R.KWARGS)
    sched.set_timesteps(25)
    tab = [sched.noise_coefficients(j) for j in range(26)]
    assert tab[0] == (0.0, 1.0) and tab[25] == (1.0, 0.0)
    return tab


def latent_mask(kind, F_, hw, g):
    if kind == "none":
        return None
    m = torch.rand(F_, hw, generator=g)
    if kind == "hard":
        m = (m > 0.5).float()
    else:
        m[:, ::5], m[:, 1::7] = 0.0, 1.0                # a soft mask still has cells that are exactly kept / free
    return m.contiguous()


# ------------------------------------------------------------------------------------------------ (8) vx_known_blend
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("kind", ["hard", "soft", "none"])
@pytest.mark.parametrize("shape", [(4, 16, 4096), (4, 6, 80)])
def test_known_blend_vs_float64(dev, elem, kind, shape):
    """|err| <= 6 * 2^-24 * (|m x| + (1 - m)(|a init| + |s noise|)) elementwise: at most six float32 roundings reach a
    term of the expression (init_video_restated.blend_bound) - derived, not measured.  (a, s) from a 25-step table,
    (0, 1) and (1, 0) included.  The CPU stand-in holds the same bound on the same inputs."""
    from v_express_amd import lib as L, ops
    c, F_, hw = shape
    g = torch.Generator().manual_seed(F_ + hw)
    x, init, noise = (torch.randn(1, c, F_, hw // 8, 8, generator=g) * sc for sc in (1.0, 0.5, 1.0))
    m = latent_mask(kind, F_, hw, g)
    tab = table25()
    worst = 0.0
    with L.element_type(elem):
        for j in (0, 1, 7, 13, 24, 25):
            a, s = tab[j]
            got = x.to(dev).clone() if m is not None else torch.full(x.shape, float("nan"), device=dev)
            ops.known_blend(got, init.to(dev), noise.to(dev), None if m is None else m.to(dev), a, s)
            torch.cuda.synchronize()
            want, bound = R.blend(x, init, noise, m, a, s), R.blend_bound(x, init, noise, m, a, s)
            err = (got.cpu().double() - want).abs()
            ratio = (err / bound.clamp_min(1e-300)).max().item()
            worst = max(worst, ratio)
            print(f"[vx_known_blend {elem}, {shape}, mask {kind}, j = {j}: (a, s) = ({a:.6f}, {s:.6f})] max |err| "
                  f"{err.max().item():.3g}, max err / (2^-24 * magnitude) {6 * ratio:.3g} (bound 6)")
            assert torch.isfinite(got).all() and (err <= bound).all()
            emu = x.clone()
            R.known_blend(emu, init, noise, m, a, s)
            assert ((emu.double() - want).abs() <= bound).all()
    assert worst <= 1.0


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", [(4, 16, 4096), (4, 6, 80)])
def test_known_blend_identities(dev, elem, shape):
    """m = 1 everywhere keeps the bits of the latents at any (a, s); (m, a, s) = (0, 1, 0) and the maskless launch at
    (1, 0) write the bits of init; a hard mask moves exactly the cells it names."""
    from v_express_amd import lib as L, ops
    c, F_, hw = shape
    g = torch.Generator().manual_seed(11)
    x, init, noise = (torch.randn(1, c, F_, hw // 8, 8, generator=g).to(dev) for _ in range(3))
    a, s = table25()[9]
    with L.element_type(elem):
        got = x.clone()
        ops.known_blend(got, init, noise, torch.ones(F_, hw, device=dev), a, s)
        assert torch.equal(got, x)
        got = x.clone()
        ops.known_blend(got, init, noise, torch.zeros(F_, hw, device=dev), 1.0, 0.0)
        assert torch.equal(got, init)
        got = torch.full_like(x, float("nan"))
        ops.known_blend(got, init, noise, None, 1.0, 0.0)
        assert torch.equal(got, init)
        hard = (torch.rand(F_, hw, generator=g) > 0.5).float().to(dev)
        got = x.clone()
        ops.known_blend(got, init, noise, hard, 1.0, 0.0)
        sel = (hard > 0).reshape(1, 1, F_, hw // 8, 8).expand_as(x)
        assert torch.equal(got[sel], x[sel]) and torch.equal(got[~sel], init[~sel])


# ------------------------------------------------------------------------------------------------ (9) the composite
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("ld", [3, 8])
def test_postprocess_composite(dev, elem, ld):
    """M = 1: the bits of vx_vae_postprocess; M = 0: the init frames bit for bit; random soft M: |err| <= 4 * 2^-24
    against float64 (operands in [0, 1]: the post-process, M v, 1 - M, its product and the sum round by at most 2^-25
    each); a row stride ld > c, a frame offset and a one-frame mask."""
    from v_express_amd import lib as L, ops
    n, c, h, w, F_, f0 = 3, 3, 24, 20, 7, 2
    g = torch.Generator().manual_seed(ld)
    rows = (torch.randn(n * h * w, ld, generator=g) * 1.5).to(dev)          # values beyond [-1, 1]: the clamp works
    video = torch.rand(1, c, F_, h, w, generator=g).to(dev)
    with L.element_type(elem):
        plain = ops.vae_postprocess(rows, n, c, h, w)
        ones, zeros = torch.ones(F_, h * w, device=dev), torch.zeros(1, h * w, device=dev)
        assert torch.equal(ops.vae_postprocess_composite(rows, n, c, h, w, video, ones, f0), plain)
        kept = ops.vae_postprocess_composite(rows, n, c, h, w, video, zeros, f0)
        assert torch.equal(kept, video[0, :, f0:f0 + n].permute(1, 0, 2, 3))
        for frames in (F_, 1):
            M = torch.rand(frames, h * w, generator=g)
            got = ops.vae_postprocess_composite(rows, n, c, h, w, video, M.to(dev), f0).cpu()
            v = (rows[:, :c].cpu().double().reshape(n, h, w, c).permute(0, 3, 1, 2) / 2 + 0.5).clamp(0, 1)
            Mk = M.reshape(frames, h, w)
            Mk = Mk if frames == 1 else Mk[f0:f0 + n]
            want = R.composite(v, video[0, :, f0:f0 + n].permute(1, 0, 2, 3).cpu(), Mk)
            err = (got.double() - want).abs().max().item()
            print(f"[vx_vae_postprocess_composite {elem}, ld {ld}, mask frames {frames}] max |err| {err:.3g} "
                  f"= {err / R.U:.3g} * 2^-24 (bound 4)")
            assert err <= 4 * R.U
            emu = R.vae_postprocess_composite(rows.cpu(), n, c, h, w, video.cpu(), M, f0)
            assert (emu.double() - want).abs().max().item() <= 4 * R.U


# ------------------------------------------------------------------------------------------------ (12) C entry points
def test_kernel_argument_errors(dev):
    from v_express_amd import lib as L
    x, init, noise = (torch.zeros(1, 4, 2, 2, 4, device=dev) for _ in range(3))
    m = torch.ones(2, 8, device=dev)
    lib = L.lib
    rc = lib.vx_known_blend(x.data_ptr(), init.data_ptr(), noise.data_ptr(), m.data_ptr(), 4, 2, 6, 1.0, 0.0, None)
    assert rc < 0 and b"hw % 4" in lib.vx_last_error_string()
    rc = lib.vx_known_blend(x.data_ptr(), init.data_ptr() + 4, noise.data_ptr(), m.data_ptr(), 4, 2, 8, 1.0, 0.0, None)
    assert rc < 0 and b"aligned" in lib.vx_last_error_string()
    rc = lib.vx_known_blend(x.data_ptr(), init.data_ptr(), noise.data_ptr(), m.data_ptr(), 4, 2, 8, -0.5, 0.0, None)
    assert rc < 0 and b"negative" in lib.vx_last_error_string()
    rc = lib.vx_known_blend(x.data_ptr(), None, noise.data_ptr(), m.data_ptr(), 4, 2, 8, 1.0, 0.0, None)
    assert rc < 0 and b"vx_known_blend" in lib.vx_last_error_string()
    rows, video, out = torch.zeros(2 * 16, 8, device=dev), torch.zeros(3, 5, 16, device=dev), torch.zeros(2, 3, 16,
                                                                                                       device=dev)
    M = torch.ones(5, 16, device=dev)
    args = (rows.data_ptr(), 8, 2, 3, 16, video.data_ptr())
    rc = lib.vx_vae_postprocess_composite(*args, 5, 4, M.data_ptr(), 5, out.data_ptr(), None)
    assert rc < 0 and b"inside the init video" in lib.vx_last_error_string()
    rc = lib.vx_vae_postprocess_composite(*args, 5, 0, M.data_ptr(), 2, out.data_ptr(), None)
    assert rc < 0 and b"mask" in lib.vx_last_error_string()
    rc = lib.vx_vae_postprocess_composite(*args, 5, 0, None, 5, out.data_ptr(), None)
    assert rc < 0 and b"bad arguments" in lib.vx_last_error_string()
    rc = lib.vx_vae_postprocess_composite(rows.data_ptr(), 2, 2, 3, 16, video.data_ptr(), 5, 0, M.data_ptr(), 5,
                                          out.data_ptr(), None)
    assert rc < 0 and b"bad arguments" in lib.vx_last_error_string()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (10) encode_video
def test_encode_video_chunks_and_oracle(dev):
    """F = 5: chunk = 1, 3 and 8 give identical bits (batch-invariant kernels), and every frame matches
    oracle.prologue.vae_encode_mean of 2 x - 1 times the scaling factor to relative 3e-2, the bound
    test_gpu_prologue.py::test_vae_encode_vs_oracle_and_reference_golden applies to the reference image."""
    import oracle
    from oracle import prologue as OP
    from v_express_amd import AutoencoderKL, synth
    vcfg = synth.VaeConfig(**cases.SMALL_VAE)
    sd = synth.vae_encoder_state_dict(vcfg)
    vae = AutoencoderKL(vcfg).to(dev)
    vae.load_state_dict(sd)
    video = torch.rand(1, 3, 5, 64, 48, generator=torch.Generator().manual_seed(21))
    got = {ch: vae.encode_video(video, chunk=ch) for ch in (1, 3, 8)}
    assert got[1].shape == (1, 4, 5, 8, 6) and got[1].dtype == torch.float32 and got[1].is_contiguous()
    assert torch.equal(got[1], got[3]) and torch.equal(got[1], got[8])
    ocfg = oracle.VaeConfig(**cases.SMALL_VAE)
    for fr in range(5):
        ref = OP.vae_encode_mean(sd, ocfg, 2.0 * video[:, :, fr] - 1.0) * vcfg.scaling_factor
        r = rel_l2(got[8][:, :, fr].cpu(), ref)
        print(f"[encode_video frame {fr}] relL2 vs oracle {r:.4g}")
        assert r <= 3e-2
    with pytest.raises(ValueError, match="encode_video"):
        vae.encode_video(video[0])


# ------------------------------------------------------------------------------------------------ (11) the pipeline
@pytest.fixture(scope="module")
def small(dev):
    """The small pipeline with BOTH halves of the VAE (seeded synthetic encoder + decoder weights)."""
    from v_express_amd import AutoencoderKL, synth
    S = build_small(dev)
    vcfg = synth.VaeConfig(**cases.SMALL_VAE)
    vae = AutoencoderKL(vcfg).to(dev)
    vae.load_state_dict(dict(synth.vae_decoder_state_dict(vcfg), **synth.vae_encoder_state_dict(vcfg)))
    S["pipe"].vae = vae
    return S


def _call(S, inp, F_, steps, cf, co, **kw):
    return call_pipeline(S["pipe"], scheduler("ddim"), inp, F_, steps, cf, co, **kw).cpu()


def _mask(F_):
    m = torch.ones(F_, 1, 64, 64)
    m[:2] = 0.0
    m[:, :, :32] = 0.0
    return m


def test_pipeline_init_latents_and_mask_vs_restated_oracle_loop(small):
    """The CPU suite's first case on the device: F = 6, windows 4 / 2, 5 DDIM steps, strength 0.6, random init latents,
    frames 0-1 and the upper half of the others kept - the bounds of test_gpu_guidance.py's pipeline test."""
    from oracle import loop as OL
    F_, cf, co, steps, strength = 6, 4, 2, 5, 0.6
    inp = inputs(F_)
    init = 0.5 * torch.randn(1, 4, F_, 8, 8, generator=torch.Generator().manual_seed(5))
    mask = _mask(F_)
    got = _call(small, inp, F_, steps, cf, co, strength=strength, init_latents=init, mask=mask)
    assert small["pipe"].last_init == dict(begin_index=2, masked=True, blend_launches=4)
    plain = _call(small, inp, F_, steps, cf, co, strength=strength)
    with oracle_on_cpu():
        ref = restated_loop(oracle_unet(inp), inp["latents"], OL.uniform_windows(F_, cf, co), cases.GUIDANCE,
                            inp["kps_features"], inp["audio_embeddings"], steps,
                            known=(init, inp["latents"], R.box_mean(mask[:, 0]), strength))
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[DDIM, init_latents + mask, strength {strength}, SMALL, F = 6, {steps} steps] relL2={r:.4g} cosine={c:.6f} "
          f"vs the restated loop; the clip without init: relL2={rel_l2(plain, ref):.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2 and c >= 0.998, (r, c)
    assert r < rel_l2(plain, ref)


def test_pipeline_init_video_identities_through_decode(small):
    """decode=True with init_video: a mask of zeros returns the init video exactly (latents and pixels are the caller's
    own); a mask of ones returns the plain decode of the same latents; a half mask returns each on its side."""
    from v_express_amd import synth
    F_, cf, co, steps = 6, 4, 2, 3
    inp = synth.synthetic_inputs(small["cfg"], F_, 8, 8)
    video = torch.rand(1, 3, F_, 64, 64, generator=torch.Generator().manual_seed(8))
    kw = dict(strength=0.7, init_video=video, decode=True)
    kept = _call(small, inp, F_, steps, cf, co, mask=torch.zeros(1, 64, 64), **kw)
    assert small["pipe"].last_init == dict(begin_index=1, masked=True, blend_launches=3)
    assert torch.equal(kept, video)
    ones = torch.ones(F_, 1, 64, 64)
    lat = _call(small, inp, F_, steps, cf, co, strength=0.7, init_video=video, mask=ones)
    img2img = _call(small, inp, F_, steps, cf, co, strength=0.7, init_video=video)
    assert torch.equal(lat, img2img)                     # m = 1 everywhere: the bits of the maskless call
    plain = small["pipe"].decode_latents(lat.cuda()).cpu()
    free = _call(small, inp, F_, steps, cf, co, mask=ones, **kw)
    assert torch.equal(free, plain)
    half = _mask(F_)
    lat_h = _call(small, inp, F_, steps, cf, co, strength=0.7, init_video=video, mask=half)
    plain_h = small["pipe"].decode_latents(lat_h.cuda()).cpu()
    comp = _call(small, inp, F_, steps, cf, co, mask=half, **kw)
    M = half[None, :, 0].expand(1, 3, F_, 64, 64) > 0
    assert torch.equal(comp[~M], video[~M]) and torch.equal(comp[M], plain_h[M])
    assert torch.equal(_call(small, inp, F_, steps, cf, co, mask=half, composite=False, **kw), plain_h)
    # the kept latent cells are the encoded init video itself
    init = small["pipe"].vae.encode_video(video).cpu()
    keep = (R.box_mean(half[:, 0]) == 0).reshape(1, 1, F_, 8, 8).expand_as(init)
    assert torch.equal(lat_h[keep], init[keep])
