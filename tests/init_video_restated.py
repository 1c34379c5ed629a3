"""float64 restatements of init-video sampling (TEST INFRASTRUCTURE) for tests/test_init_video_cpu.py and
tests/test_gpu_init_video.py: the signal / noise pair (a_j, s_j) of every sampler's schedule level, the known-region blend
of diffusers' StableDiffusionInpaintPipeline loop (`(1 - mask) * add_noise(init, noise, t_{i+1}) + mask * latents`, init
itself after the last step) and the img2img start `add_noise(init, noise, t_b)`, the pixel composite, and emulated
`ops.known_blend` / `ops.vae_postprocess_composite` in the style of tests/fake_ops.py.  The loop that uses them is
tests/loop_restated.py."""
import math

import torch

import dpm_restated as D

KWARGS = D.KWARGS
U = 2.0 ** -24                    # unit roundoff of float32


def begin_index(n, strength):
    """diffusers' get_timesteps: the loop runs the last min(int(n * strength), n) steps."""
    return max(n - min(int(n * strength), n), 0)


def coefficients(kind, n):
    """[(a_j, s_j)] for j = 0 .. n, float64: the level the latents have at step index j (j = n: after the last step).
    DDIM: sqrt(abar), sqrt(1 - abar) of timesteps[j] on the zero-SNR table, (1, 0) at the end; DPM-Solver++ and Euler
    ancestral: (1, sigma_j) / sqrt(1 + sigma_j^2) on the clamped table, the final sigma 0."""
    if kind in ("ddim", "ddim-eta"):
        abar = D.alphas_cumprod(clamp=False)
        return [(math.sqrt(abar[t]), math.sqrt(1.0 - abar[t])) for t in D.timesteps(n)] + [(1.0, 0.0)]
    return [(1.0 / math.sqrt(1.0 + s * s), s / math.sqrt(1.0 + s * s)) for s in D.sigmas(n)]


def box_mean(mask, scale=8):
    """Pixel mask [F, H, W] -> latent mask float64 [F, (H / scale) * (W / scale)]: the scale x scale box mean."""
    F_, H, W = mask.shape
    m = mask.double().reshape(F_, H // scale, scale, W // scale, scale).mean((2, 4))
    return m.reshape(F_, -1)


def blend(x, init, noise, m, a, s):
    """m x + (1 - m)(a init + s noise) in float64; x, init, noise [1, c, F, h, w], m [F, h * w] or None (the start)."""
    known = a * init.double() + s * noise.double()
    if m is None:
        return known
    mm = m.double().reshape(1, 1, x.shape[2], x.shape[3], x.shape[4])
    return mm * x.double() + (1.0 - mm) * known


def blend_bound(x, init, noise, m, a, s, roundings=6):
    """The elementwise bound of vx_known_blend: roundings * 2^-24 * (|m x| + (1 - m)(|a init| + |s noise|)).  Six float32
    roundings at most reach one term of the expression: the conversion of the coefficient, its product, the inner sum,
    1 - m, the product with it and the outer sum."""
    known = abs(a) * init.double().abs() + abs(s) * noise.double().abs()
    if m is None:
        return roundings * U * known
    mm = m.double().reshape(1, 1, x.shape[2], x.shape[3], x.shape[4])
    return roundings * U * (mm * x.double().abs() + (1.0 - mm) * known)


def known_blend(latents, init, noise, mask, a, s):
    """Emulated ops.known_blend: the kernel's expression in float64, float32 store, in place.  m = 1 keeps the bits of
    latents, (m, a, s) = (0, 1, 0) writes the bits of init, as the kernel does."""
    assert latents.dtype == init.dtype == noise.dtype == torch.float32 and init.shape == noise.shape == latents.shape
    assert a >= 0.0 and s >= 0.0 and (latents.shape[3] * latents.shape[4]) % 4 == 0
    assert mask is None or (mask.dtype == torch.float32 and tuple(mask.shape) == (latents.shape[2],
                                                                                 latents.shape[3] * latents.shape[4]))
    latents.copy_(blend(latents, init, noise, mask, float(a), float(s)).float())


def composite(decoded, init_video, mask):
    """M decoded + (1 - M) init_video in float64; decoded / init_video [n, 3, H, W], mask [n or 1, H, W]."""
    mm = mask.double()[:, None]
    return mm * decoded.double() + (1.0 - mm) * init_video.double()


def vae_postprocess_composite(x, n, c, h, w, init_video, mask, frame0=0):
    """Emulated ops.vae_postprocess_composite: fake_ops.vae_postprocess, then the composite in float64, float32 store."""
    import fake_ops
    v = fake_ops.vae_postprocess(x, n, c, h, w)
    F_ = init_video.shape[2]
    assert tuple(init_video.shape) == (1, c, F_, h, w) and mask.shape[0] in (1, F_) and mask.shape[1] == h * w
    assert 0 <= frame0 and frame0 + n <= F_
    keep = init_video[0, :, frame0:frame0 + n].permute(1, 0, 2, 3)
    mk = mask.reshape(-1, h, w)
    mk = mk if mk.shape[0] == 1 else mk[frame0:frame0 + n]
    return composite(v, keep, mk).float().contiguous()
