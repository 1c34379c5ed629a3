"""Two-pass (hi-res) sampling restated (TEST INFRASTRUCTURE): the restated loop at the first size, the float64 latent
resize of tests/resize_cases.py, and the restated loop at the second size started as diffusers' img2img pipelines start
(known = (resized, noise, None, strength)).  The two oracle UNets stand over synth.synthetic_inputs at the two sizes (the
reference latents and keypoint features of each size) with the same synthetic weights; the audio embeddings are the first
size's in both passes, as the pipeline computes them once."""
import loop_worker as W
import resize_cases as RC
from loop_restated import restated_loop

# the small configuration's hi-res case: F = 6 in windows of 4 with overlap 2, 64 -> 128 pixels (latents 8 -> 16), 3 steps
# at the first size, the last int(5 * 0.6) = 3 of 5 at the second
F, CF, CO, STEPS, HIRES_STEPS, STRENGTH, LATENT, LATENT2 = 6, 4, 2, 3, 5, 0.6, 8, 16
_INPUTS = {}


def inputs(F_=F, latent=LATENT, latent2=LATENT2):
    """(synthetic inputs at the first size, at the second): CPU, drawn once per geometry."""
    from v_express_amd import synth
    import cases
    key = (F_, latent, latent2)
    if key not in _INPUTS:
        cfg = cases.unet_cfg(cases.SMALL)
        _INPUTS[key] = (synth.synthetic_inputs(cfg, F_, latent, latent),
                        synth.synthetic_inputs(cfg, F_, latent2, latent2))
    return _INPUTS[key]


def resize64(latents, size, mode):
    """The float64 resize of [1, C, F, h, w] latents (any float dtype)."""
    _, c, F_, h, w = latents.shape
    return RC.reference(latents.reshape(c * F_, h, w), size[0], size[1], mode).reshape(1, c, F_, *size)


def first_pass(inp1, windows, s, steps, sampler="ddim", seed=None, **kw):
    """The restated loop at the first size: its final latents (float64)."""
    return restated_loop(W.oracle_unet(inp1), inp1["latents"], windows, s, inp1["kps_features"],
                         inp1["audio_embeddings"], steps, sampler, seed=seed, **kw)


def second_pass(base, inp1, inp2, windows, s, steps, strength, mode="bilinear", sampler="ddim", seed=None, **kw):
    """The restated second pass from the first pass's latents `base` (restated, or a device's own): resized in float64,
    noised with inp2's latents to the level of `strength`, the last int(steps * strength) of `steps` timesteps over the
    oracle UNet of the second size; the ancestral seed is the first pass's + 1."""
    resized = resize64(base, tuple(inp2["latents"].shape[-2:]), mode)
    return restated_loop(W.oracle_unet(inp2), inp2["latents"], windows, s, inp2["kps_features"],
                         inp1["audio_embeddings"], steps, sampler, seed=None if seed is None else seed + 1,
                         known=(resized, inp2["latents"], None, strength), **kw)


def chain(inp1, inp2, windows, s, steps, hires_steps, strength, mode="bilinear", sampler="ddim", seed=None, **kw):
    """(first pass's latents, second pass's latents), float64."""
    base = first_pass(inp1, windows, s, steps, sampler, seed, **kw)
    return base, second_pass(base, inp1, inp2, windows, s, hires_steps, strength, mode, sampler, seed, **kw)
