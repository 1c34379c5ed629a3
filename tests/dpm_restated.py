"""float64 restatements of DPM-Solver++ multistep sampling (TEST INFRASTRUCTURE) for tests/test_dpm_solver_cpu.py and
tests/test_gpu_dpm_solver.py: the schedule tables, diffusers' order rule and update (DPMSolverMultistepScheduler of
diffusers==0.29.2, algorithm_type "dpmsolver++", solver_type "midpoint", v-prediction) and an emulated
`ops.overlap_multistep_step` in the style of tests/fake_ops.py.  The loop that uses them is tests/loop_restated.py."""
import math

import numpy as np
import torch

# inference_v2.yaml noise_scheduler_kwargs (the reference's own configuration)
KWARGS = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, steps_offset=1,
              prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")


def alphas_cumprod(T=1000, beta_start=0.00085, beta_end=0.012, clamp=True):
    """Scaled-linear betas rescaled to zero terminal SNR, cumulative product; `clamp`: abar[-1] = 2^-24 (DPM-Solver)."""
    betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=np.float64) ** 2
    s = np.sqrt(np.cumprod(1.0 - betas))
    s = (s - s[-1]) * (s[0] / (s[0] - s[-1]))
    abar = s ** 2
    if clamp:
        abar = abar.copy()
        abar[-1] = 2.0 ** -24
    return abar


def timesteps(n, T=1000):
    """Trailing spacing: round(arange(T, 0, -T/n)) - 1."""
    return [int(round(T - k * T / n)) - 1 for k in range(n)]


def sigmas(n, final="zero", abar=None):
    """[sigma(t_0) ... sigma(t_{n-1}), sigma_last], sigma(t) = sqrt((1 - abar_t) / abar_t)."""
    abar = alphas_cumprod() if abar is None else abar
    sig = [math.sqrt((1.0 - abar[t]) / abar[t]) for t in timesteps(n)]
    return sig + [0.0 if final == "zero" else math.sqrt((1.0 - abar[0]) / abar[0])]


def orders(n, solver_order=2, lower_order_final=True, euler_at_final=False, final="zero", begin=0):
    """diffusers DPMSolverMultistepScheduler.step: first order at the first step of a run, at solver_order 1, and at the
    last step when the final sigma is 0, with euler_at_final, or with lower_order_final below 15 steps.  Its second
    small-n rule (`lower_order_second`, i = n - 2) only lowers third order to second: no change at solver_order <= 2."""
    out = []
    for i in range(begin, n):
        last = i == n - 1 and (euler_at_final or (lower_order_final and n < 15) or final == "zero")
        out.append(1 if (solver_order == 1 or i == begin or last) else 2)
    return out


def _alpha_sigma(s):
    a = 1.0 / math.sqrt(s * s + 1.0)
    return a, s * a


def update(sg, i, order, x, v, x0_prev):
    """One update at step index i on float64 tensors: (x', x0), in diffusers' own form (lambda = log alpha - log sigma,
    D1 = (m0 - m1) / r0).  A step that ends at sigma = 0 (h = inf) is x0."""
    a_s, s_s = _alpha_sigma(sg[i])
    x0 = a_s * x - s_s * v
    if sg[i + 1] == 0.0:
        return x0.clone(), x0
    a_t, s_t = _alpha_sigma(sg[i + 1])
    lam_t, lam_s = math.log(a_t) - math.log(s_t), math.log(a_s) - math.log(s_s)
    h = lam_t - lam_s
    out = (s_t / s_s) * x - a_t * (math.exp(-h) - 1.0) * x0
    if order == 2:
        a_p, s_p = _alpha_sigma(sg[i - 1])
        r0 = (lam_s - (math.log(a_p) - math.log(s_p))) / h
        out = out - 0.5 * a_t * (math.exp(-h) - 1.0) * (x0 - x0_prev) / r0
    return out, x0


def coefficients(sg, i, order):
    """(alpha_i, sigma_i, c_x, c_0, c_1) of x' = c_x x - c_0 x0 + c_1 x0_prev, from the update above."""
    a_s, s_s = _alpha_sigma(sg[i])
    if sg[i + 1] == 0.0:
        return a_s, s_s, 0.0, -1.0, 0.0
    a_t, s_t = _alpha_sigma(sg[i + 1])
    lam = [math.log(a) - math.log(s) for a, s in (_alpha_sigma(sg[i + 1]), (a_s, s_s))]
    h = lam[0] - lam[1]
    A = a_t * (math.exp(-h) - 1.0)
    B = 0.0
    if order == 2:
        a_p, s_p = _alpha_sigma(sg[i - 1])
        B = 0.5 * A / ((lam[1] - (math.log(a_p) - math.log(s_p))) / h)
    return a_s, s_s, s_t / s_s, A + B, B


def overlap_multistep_step(latents, preds, terms, frame_ids, counts, x0_history, coef):
    """Emulated ops.overlap_multistep_step (fake_ops style: the kernel's sum order, float64 update, float32 stores)."""
    a, s, cx, c0, c1 = (float(v) for v in coef)
    _, c, _, h, w = latents.shape
    fr = frame_ids.long()
    v = None
    for j in range(terms.shape[1]):
        slot, li = terms[:, j, 0].long(), terms[:, j, 1].long()
        term = preds[slot.clamp_min(0), :, li.clamp_min(0)] / counts[:, None, None]
        term = torch.where((slot >= 0)[:, None, None], term, torch.zeros_like(term))
        v = term if v is None else v + term
    x = latents[0].index_select(1, fr).transpose(0, 1).reshape(-1, c, h * w).double()
    x0 = a * x - s * v.double()
    new = cx * x - c0 * x0
    if c1 != 0.0:
        new = new + c1 * x0_history[0].index_select(1, fr).transpose(0, 1).reshape(-1, c, h * w).double()
    x0_history[0].index_copy_(1, fr, x0.float().reshape(-1, c, h, w).transpose(0, 1))
    latents[0].index_copy_(1, fr, new.float().reshape(-1, c, h, w).transpose(0, 1))
