"""float64 restatement of UniPC sampling (TEST INFRASTRUCTURE) for tests/test_unipc_cpu.py and tests/test_gpu_unipc.py,
written from the published behaviour of diffusers==0.29.2 `UniPCMultistepScheduler` (predict_x0, v-prediction, solver types
"bh1" / "bh2") and independent of v-express_amd/scheduler.py: the update in diffusers' own form - the D1 differences
(m_k - m0) / r_k kept as a list, the weights rho from a linear solve of R rho = b - the order of events of its `step()`,
and the per-frame restated loop over the oracle UNet.  The schedule tables are dpm_restated's."""
import math

import numpy as np
import torch

import dpm_restated as D
import guidance_restated as G
import init_video_restated as R
from loop_restated import guided_prediction, known_blend, known_level, stitch_mean

KWARGS = D.KWARGS


def alpha_sigma(sig):
    """diffusers' _sigma_to_alpha_sigma_t: alpha = 1 / sqrt(1 + sigma^2), sigma_t = sigma alpha."""
    a = 1.0 / math.sqrt(sig * sig + 1.0)
    return a, sig * a


def lam(sig):
    a, s = alpha_sigma(sig)
    return math.log(a) - math.log(s)


def order_at(n, i, begin, solver_order):
    """this_order of step(): min(solver_order, n - i) under lower_order_final, capped by lower_order_nums + 1, the number
    of steps the run has taken plus one."""
    return min(solver_order, n - i, i - begin + 1)


def bh_update(sg, a, order, x, ms, solver_type="bh2", m_t=None):
    """multistep_uni_p_bh_update (m_t None) or multistep_uni_c_bh_update (m_t: the data prediction at the end point) from
    point a to point a + 1 of the sigmas sg: x the base sample at a, ms the data predictions at points a, a - 1, ...
    (newest first).  A predictor step that ends at sigma = 0 (h = inf, expm1(-h) = -1, sigma_t = 0) is m0."""
    m0 = ms[0]
    if sg[a + 1] == 0.0:
        assert order == 1 and m_t is None
        return m0.clone()
    (a_t, s_t), (_, s_s) = alpha_sigma(sg[a + 1]), alpha_sigma(sg[a])
    h = lam(sg[a + 1]) - lam(sg[a])
    rks, D1s = [], []
    for i in range(1, order):
        rk = (lam(sg[a - i]) - lam(sg[a])) / h
        rks.append(rk)
        D1s.append((ms[i] - m0) / rk)
    rks.append(1.0)
    hh = -h
    h_phi_1 = math.expm1(hh)
    h_phi_k = h_phi_1 / hh - 1.0
    factorial_i = 1
    B_h = hh if solver_type == "bh1" else math.expm1(hh)
    Rm, b = [], []
    for i in range(1, order + 1):
        Rm.append([rk ** (i - 1) for rk in rks])
        b.append(h_phi_k * factorial_i / B_h)
        factorial_i *= i + 1
        h_phi_k = h_phi_k / hh - 1.0 / factorial_i
    Rm, b = np.array(Rm, dtype=np.float64), np.array(b, dtype=np.float64)
    x_t_ = s_t / s_s * x - a_t * h_phi_1 * m0
    if m_t is None:
        if order == 2:
            rhos = [0.5]
        else:
            rhos = np.linalg.solve(Rm[:-1, :-1], b[:-1]).tolist() if D1s else []
        res = sum(r * d for r, d in zip(rhos, D1s)) if D1s else 0.0
        return x_t_ - a_t * B_h * res
    rhos = [0.5] if order == 1 else np.linalg.solve(Rm, b).tolist()
    res = sum(r * d for r, d in zip(rhos[:-1], D1s)) if D1s else 0.0
    return x_t_ - a_t * B_h * (res + rhos[-1] * (m_t - m0))


class State:
    """What diffusers' scheduler keeps between steps: model_outputs (here newest first), last_sample, this_order."""

    def __init__(self):
        self.ms, self.last_sample, self.this_order, self.taken = [], None, 0, 0


def step(sg, n, i, x, v, st, solver_order=2, solver_type="bh2", disable=()):
    """UniPCMultistepScheduler.step at step index i on float64 tensors: the data prediction from the sample the model saw,
    the corrector of the previous step (not at the first step of a run, nor when i - 1 is disabled), then the predictor
    from the corrected sample.  Returns the next sample; `st` is advanced."""
    a, s = alpha_sigma(sg[i])
    m_t = a * x - s * v
    if st.taken > 0 and (i - 1) not in disable and st.last_sample is not None:
        x = bh_update(sg, i - 1, st.this_order, st.last_sample, st.ms, solver_type, m_t=m_t)
    st.ms = ([m_t] + st.ms)[:solver_order]
    st.this_order = min(solver_order, n - i, st.taken + 1)
    st.last_sample = x
    st.taken += 1
    return bh_update(sg, i, st.this_order, x, st.ms, solver_type)


# ------------------------------------------------------------------------------------------------ the restated loop
def restated_unipc_loop(unet_fn, latents, windows, s, kps_feature, audio_embeddings, n, *, solver_order=2,
                        solver_type="bh2", disable=(), known=None):
    """The final latents (float64) of the per-frame loop: every frame gets one UniPC step per timestep from the mean of
    its windows' guided predictions (loop_restated's), with its own State.  known = (init, noise, m, strength): started as
    diffusers' img2img pipelines start (`latents` is then not read) and, with m [F, h * w] (1 = regenerate), blended after
    every step - the latents only, never a frame's saved sample."""
    F_ = latents.shape[2]
    sg, ts = D.sigmas(n), D.timesteps(n)
    b = 0 if known is None else R.begin_index(n, known[3])
    lat = latents.double().clone() if known is None else known_level(known, "dpm", n, sg, b)
    guided = G.guided_steps(n - b, 0.0, 1.0)
    state = {fi: State() for fi in range(F_)}
    for i in range(b, n):
        names = ("u", "c") if guided[i - b] else ("c",)
        preds = [guided_prediction(unet_fn, lat[:, :, ctx], ts[i], ctx, names, guided[i - b], s, None, 0.0, kps_feature,
                                   audio_embeddings) for ctx in windows]
        v = stitch_mean(preds, windows, F_)
        x = lat.clone()
        for fi, vf in v.items():
            lat[:, :, fi] = step(sg, n, i, x[:, :, fi], vf, state[fi], solver_order, solver_type, disable)
        lat = known_blend(lat, known, "dpm", n, sg, i + 1)
    return lat


def bf16_outputs(unet_fn):
    """`unet_fn` with its outputs rounded to bfloat16: the element-type rounding a sampler amplifies."""
    def fn(*a):
        return unet_fn(*a).bfloat16().float()
    return fn
