"""float64 restatements of the three linear multistep samplers (TEST INFRASTRUCTURE) for
tests/test_linear_multistep_cpu.py and tests/test_gpu_linear_multistep.py, written from the published behaviour of
diffusers==0.29.2 and independent of v-express_amd/scheduler.py: `EulerDiscreteScheduler` and `LMSDiscreteScheduler` in
their own (VE) frame, `PNDMScheduler` with skip_prk_steps (step_plms / _get_prev_sample) on cumulative alphas; the per-frame
restated loop over the oracle UNet; and an emulated `ops.overlap_linear_step` in the style of tests/fake_ops.py."""
import math

import numpy as np
import torch

import dpm_restated as D
import guidance_restated as G
from loop_restated import guided_prediction, stitch_mean

KWARGS = D.KWARGS
SAMPLERS = ("euler", "lms", "pndm")


# ------------------------------------------------------------------------------------------------ Euler, LMS (VE frame)
def derivative(sig, X, v):
    """diffusers' v-prediction arithmetic at sigma: x0 = v (-sigma / sqrt(sigma^2 + 1)) + X / (sigma^2 + 1) and the
    derivative d = (X - x0) / sigma."""
    x0 = v * (-sig / math.sqrt(sig * sig + 1.0)) + X / (sig * sig + 1.0)
    return x0, (X - x0) / sig


def euler_update_ve(sg, i, X, v):
    """EulerDiscreteScheduler.step (gamma = 0): X' = X + d (sigma_{i+1} - sigma_i)."""
    _, d = derivative(sg[i], X, v)
    return X + d * (sg[i + 1] - sg[i])


def lms_weights(sg, i, order):
    """LMSDiscreteScheduler.get_lms_coefficient(order, i, j) for j < order: the integral of the Lagrange basis polynomial
    over [sigma_i, sigma_{i+1}].  The integrand has degree order - 1 <= 3: four Gauss-Legendre nodes integrate it exactly
    (diffusers: scipy.integrate.quad, epsrel = 1e-4)."""
    nodes, wts = np.polynomial.legendre.leggauss(4)
    lo, hi = sg[i], sg[i + 1]
    taus = 0.5 * (hi - lo) * nodes + 0.5 * (hi + lo)
    out = []
    for j in range(order):
        total = 0.0
        for tau, wt in zip(taus, wts):
            prod = 1.0
            for k in range(order):
                if k != j:
                    prod *= (tau - sg[i - k]) / (sg[i - j] - sg[i - k])
            total += wt * prod
        out.append(0.5 * (hi - lo) * total)
    return out


def lms_order_at(i, begin, lms_order):
    return min(i - begin + 1, lms_order)


def lms_update_ve(sg, i, order, X, v, ds):
    """LMSDiscreteScheduler.step: X' = X + sum_j L_j d_{i-j}; ds = the earlier derivatives, newest last.  Returns
    (X', d_i)."""
    _, d = derivative(sg[i], X, v)
    hist = (list(ds) + [d])[-order:]
    L = lms_weights(sg, i, len(hist))
    return X + sum(lj * dj for lj, dj in zip(L, reversed(hist))), d


# ------------------------------------------------------------------------------------------------ PNDM (VP frame)
def pndm_timesteps(n, T=1000):
    """plms_timesteps under skip_prk_steps: reverse(t[:-1] + t[-2:-1] + t[-1:]) of the ascending trailing list t."""
    t = D.timesteps(n, T)[::-1]
    return (t[:-1] + t[-2:-1] + t[-1:])[::-1]


def pndm_prev_sample(a, ap, b, vc):
    """PNDMScheduler._get_prev_sample for v-prediction on the cumulative alphas a (from) and ap (to): the model output is
    first turned into eps = sqrt(a) vc + sqrt(1 - a) b, then
        x' = sqrt(ap / a) b - (ap - a) eps / (a sqrt(1 - ap) + sqrt(a (1 - a) ap)).
    At a = 0 (the unclamped zero-SNR table's last entry) this is 0 / 0; its limit a -> 0 is sqrt(1 - ap) b - sqrt(ap) vc,
    which is what is returned there."""
    if a == 0.0:
        return math.sqrt(1.0 - ap) * b - math.sqrt(ap) * vc
    eps = math.sqrt(a) * vc + math.sqrt(1.0 - a) * b
    return math.sqrt(ap / a) * b - (ap - a) * eps / (a * math.sqrt(1.0 - ap) + math.sqrt(a * (1.0 - a) * ap))


def pndm_from_to(n_steps, counter, t, T=1000):
    """(from, to) timesteps of entry `counter` at list timestep t: t -> t - T // N, entry 1: t + T // N -> t."""
    r = T // n_steps
    return (t + r, t) if counter == 1 else (t, t - r)


def pndm_update(abar, final, n_steps, counter, t, x, v, ets, saved):
    """PNDMScheduler.step_plms: (x', ets', saved') for entry `counter` at list timestep t; `ets` the stored outputs (newest
    last), `saved` the sample entry 0 kept."""
    frm, to = pndm_from_to(n_steps, counter, t)
    if counter != 1:
        ets = list(ets[-3:]) + [v]
    b = x
    if len(ets) == 1 and counter == 0:
        vc, saved = v, x
    elif len(ets) == 1 and counter == 1:
        vc, b, saved = (v + ets[-1]) / 2, saved, None
    elif len(ets) == 2:
        vc = (3 * ets[-1] - ets[-2]) / 2
    elif len(ets) == 3:
        vc = (23 * ets[-1] - 16 * ets[-2] + 5 * ets[-3]) / 12
    else:
        vc = (1 / 24) * (55 * ets[-1] - 59 * ets[-2] + 37 * ets[-3] - 9 * ets[-4])
    ap = abar[to] if to >= 0 else final
    return pndm_prev_sample(abar[frm], ap, b, vc), ets, saved


# ------------------------------------------------------------------------------------------------ the restated loop
def restated_linear_loop(unet_fn, latents, windows, s, kps_feature, audio_embeddings, n, sampler, *, lms_order=4,
                         start=0.0, end=1.0):
    """The final latents (float64) of the per-frame loop: every frame gets one update per entry of the timestep list from
    the mean of its windows' guided predictions (loop_restated's), with its own history.  "euler" / "lms": the VE frame -
    latents x sigma_0, the UNet fed x / sqrt(1 + sigma^2), n entries; "pndm": n + 1 entries on the unclamped table, final
    level abar[0]; "ddim": loop_restated's own update, for comparisons."""
    F_ = latents.shape[2]
    if sampler == "pndm":
        abar = D.alphas_cumprod(clamp=False)
        ts = pndm_timesteps(n)
        lat = latents.double().clone()
        state = {fi: ([], None) for fi in range(F_)}
    else:
        sg = D.sigmas(n)
        ts = D.timesteps(n)
        lat = latents.double() * sg[0]
        state = {fi: [] for fi in range(F_)}
    guided = G.guided_steps(len(ts), start, end)
    for i, t in enumerate(ts):
        scale = 1.0 if sampler == "pndm" else 1.0 / math.sqrt(1.0 + sg[i] ** 2)
        names = ("u", "c") if guided[i] else ("c",)
        preds = [guided_prediction(unet_fn, lat[:, :, ctx] * scale, t, ctx, names, guided[i], s, None, 0.0, kps_feature,
                                   audio_embeddings) for ctx in windows]
        v = stitch_mean(preds, windows, F_)
        x = lat.clone()
        for fi, vf in v.items():
            if sampler == "euler":
                lat[:, :, fi] = euler_update_ve(sg, i, x[:, :, fi], vf)
            elif sampler == "lms":
                lat[:, :, fi], d = lms_update_ve(sg, i, lms_order, x[:, :, fi], vf, state[fi])
                state[fi] = (state[fi] + [d])[-lms_order:]
            else:
                ets, saved = state[fi]
                lat[:, :, fi], ets, saved = pndm_update(abar, abar[0], n, i, t, x[:, :, fi], vf, ets, saved)
                state[fi] = (ets, saved)
    return lat


def bf16_outputs(unet_fn):
    """`unet_fn` with its outputs rounded to bfloat16: the element-type rounding a sampler amplifies."""
    def fn(*a):
        return unet_fn(*a).bfloat16().float()
    return fn


# ------------------------------------------------------------------------------------------------ the kernel stand-in
def overlap_linear_step(latents, preds, terms, frame_ids, counts, history, saved, coef):
    """Emulated ops.overlap_linear_step (fake_ops style: the kernel's sum order for v, float64 update, float32 stores)."""
    h1, h2, h3, h_write, saved_mode = (int(v) for v in coef[:5])
    k_x, k_v, c_1, c_2, c_3, p_x, p_v = (float(v) for v in coef[5:])
    _, c, _, h, w = latents.shape
    fr = frame_ids.long()

    def frames(buf):
        return buf.index_select(1, fr).transpose(0, 1).reshape(-1, c, h * w).double()

    def store(buf, val):
        buf.index_copy_(1, fr, val.float().reshape(-1, c, h, w).transpose(0, 1))
    v = None
    for j in range(terms.shape[1]):
        slot, li = terms[:, j, 0].long(), terms[:, j, 1].long()
        term = preds[slot.clamp_min(0), :, li.clamp_min(0)] / counts[:, None, None]
        term = torch.where((slot >= 0)[:, None, None], term, torch.zeros_like(term))
        v = term if v is None else v + term
    v = v.double()
    x = frames(latents[0])
    b = frames(saved[0]) if saved_mode == 2 else x
    out = k_x * b + k_v * v
    for slot, cj in ((h1, c_1), (h2, c_2), (h3, c_3)):
        if slot >= 0:
            out = out + cj * frames(history[slot])
    if saved_mode == 1:
        store(saved[0], x)
    if h_write >= 0:
        store(history[h_write], p_x * x + p_v * v)
    store(latents[0], out)
