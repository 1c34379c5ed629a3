"""DDIM and DPM-Solver++ schedulers.  DDIM has the configuration the reference builds (inference.py:132-136 from
inference_v2.yaml:24-35): scaled-linear betas rescaled to zero terminal SNR, trailing timestep spacing,
v-prediction, eta = 0.  The arithmetic is diffusers==0.29.2 `DDIMScheduler` (absent third-party dependency;
restated from its published behaviour — SURVEY.md Appendix A).

Host side only: the per-step update itself runs in the fused `vx_overlap_ddim_step` kernel, fed by
`step_coefficients(t)`; `step()` is kept as the reference-compatible tensor API.  DPMSolverMultistepScheduler (the
second-order multistep sampler of the reference's scheduler list, pipelines/v_express_pipeline.py:83-90) feeds
`vx_overlap_multistep_step` the same way through `multistep_coefficients(i)`.  The ancestral samplers (DDIM with
eta > 0 through `DDIMScheduler.ancestral_coefficients(t, eta)`, EulerAncestralDiscreteScheduler through
`ancestral_coefficients(i)`) feed `vx_overlap_ancestral_step`, which draws its noise on the device.  The rest of the
reference's list - EulerDiscreteScheduler, LMSDiscreteScheduler, PNDMScheduler - are linear multistep updates in the loop's
frame and feed `vx_overlap_linear_step` through `linear_coefficients(i, begin_index)`.  UniPCMultistepScheduler - not on
the reference's list: a predictor-corrector, one order higher than DPM-Solver++ at the same UNet evaluations - feeds
`vx_overlap_unipc_step` through `unipc_coefficients(i, begin_index)`.

What the classes share is stated once: `_Scheduler` (all seven) holds `from_config`, the refusal of options that are not
built, the beta / alphas_cumprod / sigma tables, the timestep -> step index lookup and the index checks, and the
contract with the denoising loop, `loop_steps(timesteps, begin_index, eta, init)` -> (update, coefs): which of the five
fused updates ("ddim", "multistep", "ancestral", "linear", "unipc") the scheduler runs, the per-step coefficients that
update takes, and every rule about eta or the start of a run that depends on the class.  `_AlphaScheduler` (DDIM, PNDM)
adds the noise levels read from alphas_cumprod, `_LambdaScheduler` (DPM-Solver++, UniPC) the sigmas of the run in the
variance-preserving frame, `_SigmaScheduler` (Euler ancestral, Euler, LMS) the sigma (VE) parametrisation.
"""
from types import SimpleNamespace

import collections
import math

import numpy as np
import torch


def _betas(num_train_timesteps, beta_start, beta_end, beta_schedule, rescale_betas_zero_snr):
    """float32 beta table of diffusers' schedulers: linear or scaled-linear, optionally rescaled to zero terminal SNR."""
    if beta_schedule == "linear":
        betas = torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
    elif beta_schedule == "scaled_linear":
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    else:
        raise NotImplementedError(beta_schedule)
    if rescale_betas_zero_snr:
        abar_sqrt = torch.cumprod(1.0 - betas, 0).sqrt()
        a0, aT = abar_sqrt[0].clone(), abar_sqrt[-1].clone()
        abar_sqrt = (abar_sqrt - aT) * (a0 / (a0 - aT))
        abar = abar_sqrt ** 2
        betas = 1 - torch.cat([abar[0:1], abar[1:] / abar[:-1]])
    return betas


def _per_sample(v, sample):
    """A per-timestep coefficient list as a tensor of `sample`'s dtype that broadcasts over its batch axis."""
    t = torch.tensor(v, dtype=torch.float64).to(device=sample.device, dtype=sample.dtype).flatten()
    return t.reshape((-1,) + (1,) * (sample.dim() - 1)) if t.numel() > 1 else t.reshape(())


def _timestep_list(timesteps):
    if isinstance(timesteps, torch.Tensor):
        return [float(t) for t in timesteps.flatten().tolist()]
    if isinstance(timesteps, (list, tuple)):
        return [float(t) for t in timesteps]
    return [float(timesteps)]


def _trailing(num_train_timesteps, n, dtype):
    """diffusers' "trailing" timestep spacing: n timesteps from num_train_timesteps - 1 down, as a numpy array."""
    return np.round(np.arange(num_train_timesteps, 0, -num_train_timesteps / n)).astype(dtype) - 1


def _vp(sigma):
    """(a, s) = (1, sigma) / sqrt(1 + sigma^2) in float64: the variance-preserving pair of a sigma."""
    a = 1.0 / math.sqrt(sigma * sigma + 1.0)
    return a, sigma * a


class _Scheduler:
    """What all seven schedulers share; a subclass sets `config` and then calls `_tables`."""
    order = 1
    init_noise_sigma = 1.0

    @classmethod
    def from_config(cls, cfg, **overrides):
        """From a dict or another scheduler's `config` (e.g. `DDIMScheduler(...).config`)."""
        cfg = dict(cfg) if isinstance(cfg, dict) else dict(vars(cfg))
        cfg.update(overrides)
        return cls(**cfg)

    def _check_options(self, *options):
        """`options`: (name, value, accepted) triples of the class's own table."""
        for name, value, ok in options:
            if not ok:
                raise NotImplementedError(f"{type(self).__name__}: {name}={value!r} is not built")

    def _tables(self, sigma):
        """betas and alphas_cumprod of `config`, float32; with `sigma` the sigma table too, else final_alpha_cumprod."""
        cfg = self.config
        self.betas = _betas(cfg.num_train_timesteps, cfg.beta_start, cfg.beta_end, cfg.beta_schedule,
                            cfg.rescale_betas_zero_snr)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, 0)
        self.num_inference_steps = None
        if not sigma:
            self.final_alpha_cumprod = torch.tensor(1.0) if cfg.set_alpha_to_one else self.alphas_cumprod[0]
            return
        if cfg.rescale_betas_zero_snr:
            # the zero-SNR table ends at alphas_cumprod = 0: diffusers clamps it so that the first sigma is finite (4096)
            self.alphas_cumprod[-1] = 2 ** -24
        # sigma(t) = sqrt((1 - abar_t) / abar_t) in float32, as diffusers computes it
        self.sigma_table = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5

    def scale_model_input(self, sample, timestep=None):
        return sample

    def _index_of(self, timestep, repeated=False):
        """Step index of a schedule timestep: the first match (diffusers' index_for_timestep) or, with `repeated`, the
        second one of a timestep the list holds twice (diffusers' _init_step_index)."""
        t = float(timestep)
        hits = [i for i, own in enumerate(self.timesteps.tolist()) if float(own) == t]
        if not hits:
            raise ValueError(f"timestep {t} is not in this schedule")
        return hits[1 if repeated and len(hits) > 1 else 0]

    def _check_index(self, i, begin_index=0, closed=False, n=None):
        if self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps() first")
        n = self.num_inference_steps if n is None else n
        if not begin_index <= i < n + (1 if closed else 0):
            raise IndexError(f"step index {i} outside [{begin_index}, {n}{']' if closed else ')'}")

    def loop_steps(self, timesteps, begin_index, eta=0.0, init=False):
        """What the denoising loop runs for `timesteps`, the scheduler's own from step index `begin_index` on:
        (update, coefs) - the fused update, one of "ddim", "multistep", "ancestral", "linear", "unipc"
        (ops.overlap_<update>_step),
        and the list of per-step coefficients that update takes.  `init`: the run starts from a noised clip.  Everything
        the class does not build fails here: eta is DDIM's option, NotImplementedError from every other class."""
        raise NotImplementedError

    def _no_eta(self, eta):
        if eta != 0.0:
            raise NotImplementedError(f"eta != 0 is a DDIM option; {type(self).__name__} does not take it")


class _AlphaScheduler(_Scheduler):
    """DDIM and PNDM: the noise level of a timestep is read from alphas_cumprod (unclamped: both updates are finite at
    abar = 0), and of the state after the last step from final_alpha_cumprod."""

    def noise_coefficients(self, j):
        """(a_j, s_j) = (sqrt(abar), sqrt(1 - abar)) of timesteps[j], the level the latents have at step index j;
        j = len(timesteps): the level after the last step (final_alpha_cumprod).  Float64 arithmetic on the float32
        table: x_j = a_j x0 + s_j noise is `add_noise(x0, noise, timesteps[j])`."""
        n = len(self.timesteps)
        if not 0 <= j <= n:
            raise IndexError(f"step index {j} outside [0, {n}]")
        abar = float(self.alphas_cumprod[int(self.timesteps[j])]) if j < n else float(self.final_alpha_cumprod)
        return math.sqrt(abar), math.sqrt(1.0 - abar)

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' add_noise: sqrt(abar_t) x0 + sqrt(1 - abar_t) noise, t one timestep or one per sample of the
        batch (host torch arithmetic; the loop forms its start latents with vx_known_blend)."""
        abar = [float(self.alphas_cumprod[int(t)]) for t in _timestep_list(timesteps)]
        a = _per_sample([math.sqrt(v) for v in abar], original_samples)
        s = _per_sample([math.sqrt(1.0 - v) for v in abar], original_samples)
        return a * original_samples + s * noise


class DDIMScheduler(_AlphaScheduler):
    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon",
                 timestep_spacing="leading", rescale_betas_zero_snr=False, **unused):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, clip_sample=clip_sample,
                                      steps_offset=steps_offset, prediction_type=prediction_type,
                                      timestep_spacing=timestep_spacing, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, set_alpha_to_one=set_alpha_to_one,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._tables(sigma=False)
        if clip_sample:
            raise NotImplementedError("clip_sample=True is not used by V-Express (inference_v2.yaml:28)")
        if prediction_type != "v_prediction":
            raise NotImplementedError("only v_prediction (inference_v2.yaml:31) is built")
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)

    def set_timesteps(self, num_inference_steps, device=None):
        T, sp = self.config.num_train_timesteps, self.config.timestep_spacing
        self.num_inference_steps = num_inference_steps
        if sp == "trailing":
            ts = _trailing(T, num_inference_steps, np.int64)
        elif sp == "leading":
            ts = (np.arange(0, num_inference_steps) * (T // num_inference_steps)).round()[::-1].astype(np.int64)
            ts = ts + self.config.steps_offset
        elif sp == "linspace":
            ts = np.linspace(0, T - 1, num_inference_steps).round()[::-1].astype(np.int64)
        else:
            raise ValueError(sp)
        self.timesteps = torch.from_numpy(ts.copy())

    def _alphas(self, t):
        t = int(t)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        return a, a_prev

    def step_coefficients(self, t):
        """(sqrt(a_t), sqrt(1-a_t), sqrt(a_prev), sqrt(1-a_prev)) as fp32-rounded Python floats: exactly the
        four scalars of DDIMScheduler.step for v-prediction, eta=0."""
        a, a_prev = self._alphas(t)
        return (float(a ** 0.5), float((1 - a) ** 0.5), float(a_prev ** 0.5), float((1 - a_prev) ** 0.5))

    def ancestral_coefficients(self, t, eta):
        """(alpha_s, sigma_s, c_x, c_0, c_z) of DDIM with `eta` at timestep t: x0 = alpha_s x - sigma_s v,
        x' = c_x x - c_0 x0 + c_z z - diffusers' sqrt(a') x0 + k eps + sigma_eta z with eps written through x and x0
        (k = sqrt(1 - a' - sigma_eta^2)).  Float64 arithmetic on the float32 table; the last step (a' = 1) returns x0
        exactly.  ValueError for eta < 0 or when 1 - a' - sigma_eta^2 < 0 (diffusers would compute NaN; eta > 1 can)."""
        eta = float(eta)
        if not eta >= 0.0:
            raise ValueError(f"eta must be >= 0, got {eta}")
        a, ap = (float(v) for v in self._alphas(t))
        var = (1.0 - ap) / (1.0 - a) * (1.0 - a / ap)
        kk = 1.0 - ap - eta * eta * var                # eta = 1 at a = 0: exactly 0
        if kk < -1e-12:
            raise ValueError(f"eta={eta}: 1 - alpha_prev - sigma_eta^2 = {kk:.3g} < 0 at timestep {int(t)}")
        sig, k = eta * math.sqrt(var), math.sqrt(max(kk, 0.0))
        sa, s1a = math.sqrt(a), math.sqrt(1.0 - a)
        return sa, s1a, k / s1a, -(math.sqrt(ap) - k * sa / s1a), sig

    def loop_steps(self, timesteps, begin_index, eta=0.0, init=False):
        """ "ddim" with `step_coefficients` for eta = 0, "ancestral" with `ancestral_coefficients` for eta > 0 (ValueError
        for eta < 0 or too large); both read the timesteps themselves, `begin_index` only numbers the noise draws."""
        if eta < 0:
            raise ValueError(f"eta must be >= 0, got {eta}")
        if eta == 0.0:
            return "ddim", [self.step_coefficients(int(t)) for t in timesteps]
        return "ancestral", [self.ancestral_coefficients(t, eta) for t in timesteps]

    def step(self, model_output, timestep, sample, eta=0.0, **unused):
        if eta != 0.0:
            raise NotImplementedError("eta != 0 is not used by V-Express")
        sa, s1a, sap, s1ap = self.step_coefficients(timestep)
        x0 = sa * sample - s1a * model_output
        eps = sa * model_output + s1a * sample
        return SimpleNamespace(prev_sample=sap * x0 + s1ap * eps, pred_original_sample=x0)


class _LambdaScheduler(_Scheduler):
    """DPM-Solver++ and UniPC: exponential integrators on lambda = -log sigma over the clamped sigma table, in the
    variance-preserving frame - sigmas = table[timesteps] + [the final sigma], the noise level of a step index read from
    them.  A subclass has `_reset` (the state of its `step()`)."""

    def set_timesteps(self, num_inference_steps, device=None):
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(_trailing(T, num_inference_steps, np.int64))
        sig = self.sigma_table[self.timesteps]
        last = torch.zeros(1) if self.config.final_sigmas_type == "zero" else self.sigma_table[:1]
        self.sigmas = torch.cat([sig, last]).to(torch.float32)
        self._reset()

    def noise_coefficients(self, j):
        """(a_j, s_j) = (alpha_t, sigma_t) of sigmas[j], the level the latents have at step index j (j = number of
        steps: the final sigma).  Float64 arithmetic on the float32 sigmas."""
        self._check_index(j, closed=True)
        return _vp(float(self.sigmas[j]))

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' DPMSolverMultistepScheduler.add_noise (UniPCMultistepScheduler's is the same): alpha_t x0 + sigma_t
        noise at the schedule's own timesteps (one, or one per sample of the batch)."""
        pairs = [self.noise_coefficients(self._index_of(t)) for t in _timestep_list(timesteps)]
        a = _per_sample([p[0] for p in pairs], original_samples)
        s = _per_sample([p[1] for p in pairs], original_samples)
        return a * original_samples + s * noise


class DPMSolverMultistepScheduler(_LambdaScheduler):
    """DPM-Solver++ (multistep, data prediction, midpoint) for the zero-terminal-SNR v-prediction schedule: the arithmetic
    of diffusers==0.29.2 `DPMSolverMultistepScheduler` restated for the options listed in `__init__` (any other value
    raises NotImplementedError naming the option).

    The loop runs the update in the fused `vx_overlap_multistep_step` kernel, fed by `multistep_coefficients(i)`:
        x0 = alpha_i x - sigma_i v ;   x' = c_x x - c_0 x0 + c_1 x0_prev
    with the previous step's x0 kept on the device.  `step()` is the stateful diffusers-style tensor API.
    """

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                 dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++",
                 solver_type="midpoint", lower_order_final=True, euler_at_final=False, use_karras_sigmas=False,
                 use_lu_lambdas=False, final_sigmas_type="zero", lambda_min_clipped=-float("inf"),
                 variance_type=None, timestep_spacing="linspace", steps_offset=0, rescale_betas_zero_snr=False,
                 **unused):
        # (clip_sample, set_alpha_to_one, ... of a DDIM configuration are not parameters of this solver: ignored, as
        # diffusers' from_config does)
        self._check_options(("trained_betas", trained_betas, trained_betas is None),
                            ("solver_order", solver_order, solver_order in (1, 2)),
                            ("prediction_type", prediction_type, prediction_type == "v_prediction"),
                            ("thresholding", thresholding, not thresholding),
                            ("algorithm_type", algorithm_type, algorithm_type == "dpmsolver++"),
                            ("solver_type", solver_type, solver_type == "midpoint"),
                            ("use_karras_sigmas", use_karras_sigmas, not use_karras_sigmas),
                            ("use_lu_lambdas", use_lu_lambdas, not use_lu_lambdas),
                            ("final_sigmas_type", final_sigmas_type, final_sigmas_type in ("zero", "sigma_min")),
                            ("lambda_min_clipped", lambda_min_clipped, lambda_min_clipped == -float("inf")),
                            ("variance_type", variance_type, variance_type is None),
                            ("timestep_spacing", timestep_spacing, timestep_spacing == "trailing"))
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, solver_order=solver_order,
                                      prediction_type=prediction_type, algorithm_type=algorithm_type,
                                      solver_type=solver_type, lower_order_final=lower_order_final,
                                      euler_at_final=euler_at_final, final_sigmas_type=final_sigmas_type,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._tables(sigma=True)
        self.timesteps = None
        self.sigmas = None
        self._reset()

    def _reset(self):
        self.step_index = None
        self._x0_prev = None
        self._taken = 0

    def solver_order_at(self, i, begin_index=0):
        """Order of the update at step index i of a run that started at `begin_index` (diffusers' step(): first order
        at the first step of a run, at solver_order 1, and at the last step under final_sigmas_type "zero",
        euler_at_final, or lower_order_final below 15 steps).  diffusers' other small-n rule, `lower_order_second` at
        i = n - 2, caps the order at 2 and so changes nothing for solver_order <= 2."""
        self._check_index(i, begin_index)
        cfg, n = self.config, self.num_inference_steps
        last = i == n - 1 and (cfg.euler_at_final or (cfg.lower_order_final and n < 15)
                               or cfg.final_sigmas_type == "zero")
        return 1 if (cfg.solver_order == 1 or i == begin_index or last) else 2

    def multistep_coefficients(self, i, begin_index=0):
        """(alpha_i, sigma_i, c_x, c_0, c_1) of step index i: x0 = alpha_i x - sigma_i v, x' = c_x x - c_0 x0 + c_1 x0_prev.
        Float64 arithmetic on the float32 sigma table; a step that ends at sigma = 0 returns x0 exactly (c_x = 0,
        c_0 = -1, c_1 = 0), so no inf or NaN reaches the kernel."""
        order = self.solver_order_at(i, begin_index)
        sg = [float(s) for s in self.sigmas]
        s0, s1 = sg[i], sg[i + 1]
        (a_i, sd_i), (a_1, sd_1) = _vp(s0), _vp(s1)
        if s1 == 0.0:
            return a_i, sd_i, 0.0, -1.0, 0.0
        h = math.log(s0) - math.log(s1)                                    # lambda = -log sigma
        A = a_1 * math.expm1(-h)
        c_x = sd_1 / sd_i
        B = 0.0
        if order == 2:
            r = (math.log(sg[i - 1]) - math.log(s0)) / h
            B = 0.5 * A / r
        return a_i, sd_i, c_x, A + B, B

    def loop_steps(self, timesteps, begin_index, eta=0.0, init=False):
        self._no_eta(eta)
        return "multistep", [self.multistep_coefficients(begin_index + i, begin_index) for i in range(len(timesteps))]

    def step(self, model_output, timestep, sample, return_dict=True, **unused):
        """One update on tensors (v-prediction `model_output`), keeping the step index and the last x0 like diffusers."""
        if self.step_index is None:
            self.step_index = self._index_of(int(timestep))
        i = self.step_index
        a_i, sd_i, c_x, c_0, c_1 = self.multistep_coefficients(i, begin_index=i - self._taken)
        x0 = a_i * sample - sd_i * model_output
        prev = c_x * sample - c_0 * x0
        if c_1 != 0.0:
            prev = prev + c_1 * self._x0_prev
        self._x0_prev = x0
        self.step_index += 1
        self._taken += 1
        out = SimpleNamespace(prev_sample=prev, pred_original_sample=x0)
        return out if return_dict else (prev,)


# ---------------------------------------------------------------------------------------------------------------------
# UniPC: per frame and timestep the corrector of the step that ended at the sample the UNet just saw, then the predictor
# from the corrected sample, both linear in the data predictions m:
#     m = a_i x - s_i v;   xc = q_s saved + q_m m + q_1 H[h1] + q_2 H[h2] + q_3 H[h3] if use_c else x
#     out = k_x xc + k_m m + k_1 H[h1] + k_2 H[h2];   saved <- xc;   H[h_write] <- m
# over the latents x, the window-averaged model output v, three per-frame history tensors H (a ring of three slots holding
# the earlier m, newest in h1) and the saved corrected sample.  The fused `vx_overlap_unipc_step` kernel runs it, fed by
# `UniPCMultistepScheduler.unipc_coefficients(i, begin_index)`.
UniPCStep = collections.namedtuple("UniPCStep", "h1 h2 h3 h_write use_c a_i s_i q_s q_m q_1 q_2 q_3 k_x k_m k_1 k_2")
UniPCStep.__doc__ = """Coefficients of one UniPC update: history slots read (h1..h3: the data predictions of the previous
three steps, newest first) and written (h_write), each 0..2 or -1 (none); use_c 1 (the corrector runs from the saved
sample) or 0 (xc = x); m = a_i x - s_i v; xc = q_s saved + q_m m + sum_j q_j H[h_j]; out = k_x xc + k_m m + k_1 H[h1] +
k_2 H[h2]; the sample saved is xc, the history entry written is m."""


class UniPCMultistepScheduler(_LambdaScheduler):
    """UniPC (unified predictor-corrector, Zhao et al. 2023; multistep, data prediction) for the zero-terminal-SNR
    v-prediction schedule: the arithmetic of diffusers==0.29.2 `UniPCMultistepScheduler` restated for the options listed in
    `__init__` (any other value raises NotImplementedError naming the option).  Timesteps, sigmas and noise levels are
    DPMSolverMultistepScheduler's (the 2^-24 clamp included); the loop's frame is variance-preserving.

    With lambda = -log sigma, a step of order p from point a to point b (h = lambda_b - lambda_a, hh = -h) over the base
    sample x_a, the data prediction m0 at a and older ones m_k at r_k = (lambda_k - lambda_a) / h is
        x_b = (s_b / s_a) x_a - alpha_b phi1 m0 - alpha_b B (sum_k rho_k (m_k - m0) / r_k [+ rho_p (m_t - m0)])
    with phi1 = expm1(hh), B = hh ("bh1") or phi1 ("bh2"), and rho the solution of R rho = b (R[i][k] = r_k^(i-1), r_p = 1,
    b_i = g_i i! / B) - the whole system for the corrector, whose last unknown weighs the prediction m_t at b itself; its
    leading (p-1) x (p-1) block for the predictor; the published shortcut rho = [0.5] for the second-order predictor and
    the first-order corrector.  After every UNet evaluation the step that ended there is corrected with the new m_t (no
    further evaluation), then the predictor runs from the corrected sample - `unipc_coefficients(i)` folds both into the
    coefficients of the fused `vx_overlap_unipc_step` kernel.  `step()` is the stateful diffusers-style tensor API."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                 dynamic_thresholding_ratio=0.995, sample_max_value=1.0, predict_x0=True, solver_type="bh2",
                 lower_order_final=True, disable_corrector=(), solver_p=None, use_karras_sigmas=False,
                 timestep_spacing="linspace", steps_offset=0, final_sigmas_type="zero", rescale_betas_zero_snr=False,
                 **unused):
        # (clip_sample, set_alpha_to_one, ... of a DDIM configuration are not parameters of this solver: ignored, as
        # diffusers' from_config does)
        disable_corrector = [] if disable_corrector is None else list(disable_corrector)
        self._check_options(("trained_betas", trained_betas, trained_betas is None),
                            ("solver_order", solver_order, solver_order in (1, 2, 3)),
                            ("prediction_type", prediction_type, prediction_type == "v_prediction"),
                            ("thresholding", thresholding, not thresholding),
                            ("predict_x0", predict_x0, predict_x0 is True),
                            ("solver_type", solver_type, solver_type in ("bh1", "bh2")),
                            ("lower_order_final", lower_order_final, lower_order_final is True),
                            ("disable_corrector", disable_corrector,
                             all(isinstance(k, int) and not isinstance(k, bool) for k in disable_corrector)),
                            ("solver_p", solver_p, solver_p is None),
                            ("use_karras_sigmas", use_karras_sigmas, not use_karras_sigmas),
                            ("final_sigmas_type", final_sigmas_type, final_sigmas_type in ("zero", "sigma_min")),
                            ("timestep_spacing", timestep_spacing, timestep_spacing == "trailing"))
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, solver_order=solver_order,
                                      prediction_type=prediction_type, predict_x0=predict_x0, solver_type=solver_type,
                                      lower_order_final=lower_order_final, disable_corrector=disable_corrector,
                                      solver_p=solver_p, final_sigmas_type=final_sigmas_type,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._tables(sigma=True)
        self.timesteps = None
        self.sigmas = None
        self._reset()

    def _reset(self):
        self.step_index = None
        self._ring = [None] * 3
        self._saved = None
        self._taken = 0

    def solver_order_at(self, i, begin_index=0):
        """p_i = min(solver_order, n - i, i - begin_index + 1): the order of the predictor of step index i in a run that
        started at `begin_index` - and of the corrector that redoes that step at index i + 1 (diffusers' this_order under
        lower_order_final; the history starts empty at begin_index)."""
        self._check_index(i, begin_index)
        return min(self.config.solver_order, self.num_inference_steps - i, i - begin_index + 1)

    def _bh_weights(self, a, order, corrector):
        """(c_x, c_0, [c_1 .. c_{order-1}], c_t) of the step from point a to point a + 1 written
        x_b = c_x x_a + c_0 m0 + sum_k c_k m_k + c_t m_t, m_k the data prediction at point a - k (c_t = 0 for the
        predictor): the (m_k - m0) / r_k differences folded into the coefficients.  Float64 arithmetic on the float32
        sigmas; a predictor step that ends at sigma = 0 (first order by solver_order_at) is m0 itself."""
        sg = self.sigmas
        s_a, s_b = float(sg[a]), float(sg[a + 1])
        if s_b == 0.0:
            return 0.0, 1.0, [], 0.0
        (al_b, sd_b), (_, sd_a) = _vp(s_b), _vp(s_a)
        lam_a = -math.log(s_a)
        h = -math.log(s_b) - lam_a
        hh = -h
        rks = [(-math.log(float(sg[a - k])) - lam_a) / h for k in range(1, order)] + [1.0]
        phi1 = math.expm1(hh)
        B = hh if self.config.solver_type == "bh1" else phi1
        g, fact, b = phi1 / hh - 1.0, 1, []
        for i in range(1, order + 1):
            b.append(g * fact / B)
            fact *= i + 1
            g = g / hh - 1.0 / fact
        R = [[rk ** (i - 1) for rk in rks] for i in range(1, order + 1)]
        if corrector:
            rho = [0.5] if order == 1 else np.linalg.solve(np.array(R), np.array(b)).tolist()
        elif order <= 2:
            rho = [0.5] * (order - 1)
        else:
            rho = np.linalg.solve(np.array(R)[:-1, :-1], np.array(b)[:-1]).tolist()
        older = [-al_b * B * rho[k] / rks[k] for k in range(order - 1)]
        rho_t = rho[order - 1] if corrector else 0.0
        c_0 = -al_b * phi1 + al_b * B * (sum(rho[k] / rks[k] for k in range(order - 1)) + rho_t)
        return sd_b / sd_a, c_0, older, -al_b * B * rho_t

    def unipc_coefficients(self, i, begin_index=0):
        """UniPCStep of step index i of a run that started at `begin_index`: the corrector from point i - 1 to i (order
        p_{i-1}, base the saved sample; not at the first step of a run, nor when i - 1 is in disable_corrector, nor before
        a predictor that ends at sigma = 0 and returns m whatever xc is) and the predictor from i to i + 1 (order p_i).
        The data prediction of point j lives in ring slot (j - begin_index) % 3; this step's goes to the slot of point
        i - 3, which a third-order corrector reads in the same update."""
        p = self.solver_order_at(i, begin_index)
        a_i, s_i = _vp(float(self.sigmas[i]))
        k_x, k_m, k_old, _ = self._bh_weights(i, p, corrector=False)
        r = i - begin_index
        use_c = r > 0 and (i - 1) not in self.config.disable_corrector and float(self.sigmas[i + 1]) != 0.0
        q_s = q_m = 0.0
        q_old, pc = [], 0
        if use_c:
            pc = self.solver_order_at(i - 1, begin_index)
            q_s, q_0, older, q_m = self._bh_weights(i - 1, pc, corrector=True)
            q_old = [q_0] + older                      # m_{i-1} is the corrector's m0
        reads = max(pc, len(k_old))
        slots = [(r - j) % 3 if j <= reads else -1 for j in (1, 2)] + [(r - 3) % 3 if pc == 3 else -1]
        q_old = q_old + [0.0] * (3 - len(q_old))
        k_old = k_old + [0.0] * (2 - len(k_old))
        return UniPCStep(*slots, r % 3, int(use_c), a_i, s_i, float(q_s), float(q_m), *map(float, q_old), float(k_x),
                         float(k_m), *map(float, k_old))

    def loop_steps(self, timesteps, begin_index, eta=0.0, init=False):
        self._no_eta(eta)
        return "unipc", [self.unipc_coefficients(begin_index + i, begin_index) for i in range(len(timesteps))]

    def step(self, model_output, timestep, sample, return_dict=True, **unused):
        """One update on tensors (v-prediction `model_output`), keeping the step index, the last data predictions and the
        corrected sample like diffusers."""
        if self.step_index is None:
            self.step_index = self._index_of(int(timestep))
        i = self.step_index
        cf = self.unipc_coefficients(i, begin_index=i - self._taken)
        H = self._ring
        m = cf.a_i * sample - cf.s_i * model_output
        xc = sample
        if cf.use_c:
            xc = cf.q_s * self._saved + cf.q_m * m
            for slot, q in ((cf.h1, cf.q_1), (cf.h2, cf.q_2), (cf.h3, cf.q_3)):
                if slot >= 0:
                    xc = xc + q * H[slot]
        prev = cf.k_x * xc + cf.k_m * m
        for slot, k in ((cf.h1, cf.k_1), (cf.h2, cf.k_2)):
            if slot >= 0:
                prev = prev + k * H[slot]
        self._saved, H[cf.h_write] = xc, m
        self.step_index += 1
        self._taken += 1
        out = SimpleNamespace(prev_sample=prev, pred_original_sample=m)
        return out if return_dict else (prev,)


class _SigmaScheduler(_Scheduler):
    """What the three samplers of the sigma (VE) parametrisation - Euler ancestral, Euler, LMS - share: the clamped
    zero-SNR table, sigmas = table[timesteps] + [0], init_noise_sigma = the largest sigma, the UNet input
    x / sqrt(1 + sigma^2), and the VP pair and frame scale the loop asks for.  A class that has `frame_scale` hands its
    latents over in the VE frame; the loop runs in the VP frame."""

    def _sigma_tables(self):
        self._tables(sigma=True)
        T = self.config.num_train_timesteps
        self.sigmas = torch.cat([self.sigma_table.flip(0), torch.zeros(1)]).to(torch.float32)
        self.timesteps = torch.linspace(0, T - 1, T, dtype=torch.float64).flip(0).to(torch.float32)
        self._reset()

    def _reset(self):
        self._step_index = None
        self._begin_index = None
        self._derivatives = []

    @property
    def init_noise_sigma(self):
        """diffusers: the largest sigma under "linspace" / "trailing" spacing (a float32 tensor)."""
        return self.sigmas.max()

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index=0):
        self._begin_index = begin_index

    def set_timesteps(self, num_inference_steps, device=None):
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(_trailing(T, num_inference_steps, np.float32))
        sig = self.sigma_table[self.timesteps.long()]
        self.sigmas = torch.cat([sig, torch.zeros(1)]).to(torch.float32)
        self._reset()

    def _init_step_index(self, timestep):
        if self._begin_index is None:
            self._step_index = self._index_of(timestep, repeated=True)
        else:
            self._step_index = self._begin_index

    def scale_model_input(self, sample, timestep=None):
        """x_ve -> x_vp = x_ve / sqrt(1 + sigma^2) at the current step (diffusers' scaling of the UNet input)."""
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma = self.sigmas[self._step_index]
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def _vp_at(self, j):
        return _vp(float(self.sigmas[j]))

    def loop_steps(self, timesteps, begin_index, eta=0.0, init=False):
        """The two deterministic samplers (Euler ancestral has its own)."""
        self._no_eta(eta)
        return "linear", [self.linear_coefficients(begin_index + i, begin_index) for i in range(len(timesteps))]

    def noise_coefficients(self, j):
        """(a_j, s_j) = (1, sigma_j) / sqrt(1 + sigma_j^2) of sigmas[j]: the variance-preserving pair of the frame the
        loop runs in (x_vp = x_ve / sqrt(1 + sigma^2)); j = number of steps: the final sigma = 0, (1, 0)."""
        self._check_index(j, closed=True)
        return self._vp_at(j)

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' add_noise in the scheduler's own (VE) frame: x0 + sigma noise at the schedule's own timesteps (one,
        or one per sample of the batch)."""
        sig = [float(self.sigmas[self._index_of(t)]) for t in _timestep_list(timesteps)]
        return original_samples + _per_sample(sig, original_samples) * noise

    def frame_scale(self, i):
        """sqrt(1 + sigmas[i]^2): x_ve = frame_scale(i) x_vp at step index i (1 at the final sigma = 0)."""
        s = float(self.sigmas[i])
        return math.sqrt(1.0 + s * s)

    def _derivative(self, model_output, sample, i):
        """diffusers' v-prediction arithmetic in the VE frame: (x0, d = (x - x0) / sigma = eps), float64 scalars."""
        sigma = float(self.sigmas[i])
        x0 = model_output * (-sigma / math.sqrt(sigma * sigma + 1.0)) + sample / (sigma * sigma + 1.0)
        return x0, (sample - x0) / sigma


class EulerAncestralDiscreteScheduler(_SigmaScheduler):
    """Euler ancestral sampling for the zero-terminal-SNR v-prediction schedule: the arithmetic of diffusers==0.29.2
    `EulerAncestralDiscreteScheduler` restated for the options listed in `__init__` (any other value raises
    NotImplementedError naming the option).

    diffusers works in the VE frame (x_ve = x0 + sigma eps, `scale_model_input` divides by sqrt(1 + sigma^2)).  The loop
    runs in the VP frame x_vp = x_ve / sqrt(1 + sigma^2) - exactly the UNet input - with the update of the fused
    `vx_overlap_ancestral_step` kernel, fed by `ancestral_coefficients(i)`:
        x0 = alpha_s x - sigma_s v ;   x' = c_x x - c_0 x0 + c_z z
    `step()` is the stateful diffusers-style tensor API in the VE frame.
    """

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0,
                 rescale_betas_zero_snr=False, **unused):
        # (clip_sample, set_alpha_to_one, ... of a DDIM configuration are not parameters of this sampler: ignored, as
        # diffusers' from_config does)
        self._check_options(("trained_betas", trained_betas, trained_betas is None),
                            ("beta_schedule", beta_schedule, beta_schedule == "scaled_linear"),
                            ("prediction_type", prediction_type, prediction_type == "v_prediction"),
                            ("timestep_spacing", timestep_spacing, timestep_spacing == "trailing"))
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, prediction_type=prediction_type,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._sigma_tables()

    def ancestral_coefficients(self, i):
        """(alpha_s, sigma_s, c_x, c_0, c_z) of step index i in the VP frame: x0 = alpha_s x - sigma_s v,
        x' = c_x x - c_0 x0 + c_z z with x, x' = x_ve / sqrt(1 + sigma^2) at sigmas[i], sigmas[i + 1].  Float64
        arithmetic on the float32 sigmas; a step that ends at sigma = 0 returns x0 exactly (c_x = 0, c_0 = -1, c_z = 0)."""
        self._check_index(i)
        s, s1 = float(self.sigmas[i]), float(self.sigmas[i + 1])
        r = math.sqrt(1.0 + s * s)
        alpha_s, sigma_s = 1.0 / r, s / r
        if s1 == 0.0:
            return alpha_s, sigma_s, 0.0, -1.0, 0.0
        s_up = math.sqrt(s1 * s1 * (s * s - s1 * s1) / (s * s))
        s_down = math.sqrt(s1 * s1 - s_up * s_up)
        r1 = math.sqrt(1.0 + s1 * s1)
        return alpha_s, sigma_s, r * s_down / (s * r1), -(1.0 - s_down / s) / r1, s_up / r1

    def loop_steps(self, timesteps, begin_index, eta=0.0, init=False):
        self._no_eta(eta)
        return "ancestral", [self.ancestral_coefficients(begin_index + i) for i in range(len(timesteps))]

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, **unused):
        """One update on tensors in the VE frame (v-prediction `model_output`, diffusers' arithmetic in float32), noise
        drawn with torch.randn on `generator`, keeping the step index like diffusers."""
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        sigma = self.sigmas[i]
        sample = sample.to(torch.float32)
        x0 = model_output * (-sigma / (sigma ** 2 + 1) ** 0.5) + (sample / (sigma ** 2 + 1))
        sigma_from, sigma_to = self.sigmas[i], self.sigmas[i + 1]
        sigma_up = (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5
        sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
        prev = sample + (sample - x0) / sigma * (sigma_down - sigma)
        gen_dev = generator.device if generator is not None else model_output.device
        noise = torch.randn(model_output.shape, generator=generator, dtype=model_output.dtype, device=gen_dev)
        prev = (prev + noise.to(model_output.device) * sigma_up).to(model_output.dtype)
        self._step_index += 1
        out = SimpleNamespace(prev_sample=prev, pred_original_sample=x0)
        return out if return_dict else (prev,)


# ---------------------------------------------------------------------------------------------------------------------
# Linear multistep samplers (Euler discrete, LMS discrete, PNDM): one update form in the loop's variance-preserving frame,
#     b = saved if saved_mode == 2 else x;   out = k_x b + k_v v + c_1 H[h1] + c_2 H[h2] + c_3 H[h3]
# over the latents x, the window-averaged model output v, up to three per-frame history tensors H (a ring of three slots;
# the entry a step writes is p_x x + p_v v) and, for PNDM's warm-up pair, one saved sample.  The fused
# `vx_overlap_linear_step` kernel runs it, fed by each class's `linear_coefficients(i, begin_index)`.
LinearStep = collections.namedtuple("LinearStep", "h1 h2 h3 h_write saved_mode k_x k_v c_1 c_2 c_3 p_x p_v")
LinearStep.__doc__ = """Coefficients of one linear multistep update: history slots read (h1..h3) and written (h_write), each
0..2 or -1 (none); saved_mode 0 (no saved sample), 1 (store x) or 2 (the saved sample is the base b);
out = k_x b + k_v v + sum_j c_j H[h_j]; the history entry written is p_x x + p_v v."""


def _linear_step(k_x, k_v, reads=(), h_write=-1, saved_mode=0, p=(0.0, 0.0)):
    """LinearStep from (slot, coefficient) pairs of the history terms, in the order they are added."""
    slots = [sl for sl, _ in reads] + [-1] * (3 - len(reads))
    cs = [float(cj) for _, cj in reads] + [0.0] * (3 - len(reads))
    return LinearStep(*slots, h_write, saved_mode, float(k_x), float(k_v), *cs, float(p[0]), float(p[1]))


def lms_integrals(sg, i, order):
    """[L_0 .. L_{order-1}] of step index i: L_j = integral from sg[i] to sg[i + 1] of the Lagrange basis polynomial
    prod_{k != j, k < order} (tau - sg[i - k]) / (sg[i - j] - sg[i - k]) - the weights of diffusers'
    LMSDiscreteScheduler.get_lms_coefficient, integrated here as an exact polynomial in float64 (diffusers:
    scipy.integrate.quad with epsrel = 1e-4).  In the variable u = tau - sg[i] the lower limit is 0, so the antiderivative
    is evaluated once, at u = sg[i + 1] - sg[i]."""
    nodes = [float(sg[i - k]) - float(sg[i]) for k in range(order)]
    upper = float(sg[i + 1]) - float(sg[i])
    out = []
    for j in range(order):
        coef = [1.0]                                             # the basis polynomial in u, ascending powers
        for k in range(order):
            if k != j:
                d, nxt = nodes[j] - nodes[k], [0.0] * (len(coef) + 1)
                for p, cp in enumerate(coef):                    # times (u - nodes[k]) / d
                    nxt[p + 1] += cp / d
                    nxt[p] -= cp * nodes[k] / d
                coef = nxt
        out.append(sum(cp * upper ** (p + 1) / (p + 1) for p, cp in enumerate(coef)))
    return out


class EulerDiscreteScheduler(_SigmaScheduler):
    """Euler sampling for the zero-terminal-SNR v-prediction schedule: the arithmetic of diffusers==0.29.2
    `EulerDiscreteScheduler` restated for the options listed in `__init__` (any other value raises NotImplementedError
    naming the option; `step(..., s_churn != 0)` too).

    diffusers works in the VE frame (x_ve = x0 + sigma eps, `scale_model_input` divides by sqrt(1 + sigma^2)); the loop runs
    in the VP frame x_vp = x_ve / sqrt(1 + sigma^2) - exactly the UNet input - with `vx_overlap_linear_step`, fed by
    `linear_coefficients(i)`.  With a = 1 / sqrt(1 + sigma_i^2), s = sigma_i a and primes for i + 1:
        x0 = a x - s v,  eps = s x + a v,  x' = a' x0 + s' eps = (a' a + s' s) x + (s' a - a' s) v
    (the deterministic DDIM update between the two sigmas).  `step()` is the stateful diffusers-style tensor API in the VE
    frame."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, prediction_type="epsilon", interpolation_type="linear", use_karras_sigmas=False,
                 sigma_min=None, sigma_max=None, timestep_spacing="linspace", timestep_type="discrete", steps_offset=0,
                 rescale_betas_zero_snr=False, final_sigmas_type="zero", **unused):
        # (clip_sample, set_alpha_to_one, ... of a DDIM configuration are not parameters of this sampler: ignored, as
        # diffusers' from_config does)
        self._check_options(("trained_betas", trained_betas, trained_betas is None),
                            ("beta_schedule", beta_schedule, beta_schedule in ("linear", "scaled_linear")),
                            ("prediction_type", prediction_type, prediction_type == "v_prediction"),
                            ("interpolation_type", interpolation_type, interpolation_type == "linear"),
                            ("use_karras_sigmas", use_karras_sigmas, not use_karras_sigmas),
                            ("sigma_min", sigma_min, sigma_min is None),
                            ("sigma_max", sigma_max, sigma_max is None),
                            ("timestep_spacing", timestep_spacing, timestep_spacing == "trailing"),
                            ("timestep_type", timestep_type, timestep_type == "discrete"),
                            ("final_sigmas_type", final_sigmas_type, final_sigmas_type == "zero"))
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, prediction_type=prediction_type,
                                      interpolation_type=interpolation_type, use_karras_sigmas=use_karras_sigmas,
                                      timestep_spacing=timestep_spacing, timestep_type=timestep_type,
                                      steps_offset=steps_offset, rescale_betas_zero_snr=rescale_betas_zero_snr,
                                      final_sigmas_type=final_sigmas_type)
        self._sigma_tables()

    def linear_coefficients(self, i, begin_index=0):
        """LinearStep of step index i: k_x = a' a + s' s, k_v = s' a - a' s, no history.  Float64 arithmetic on the
        float32 sigmas; a step that ends at sigma = 0 is x0 itself, (k_x, k_v) = (a, -s)."""
        self._check_index(i, begin_index)
        (a, s), (a1, s1) = self._vp_at(i), self._vp_at(i + 1)
        return _linear_step(a1 * a + s1 * s, s1 * a - a1 * s)

    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0,
             generator=None, return_dict=True, **unused):
        """One update on tensors in the VE frame (v-prediction `model_output`): x + d (sigma' - sigma), keeping the step
        index like diffusers."""
        self._check_options(("s_churn", s_churn, s_churn == 0.0))
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        x0, d = self._derivative(model_output, sample, i)
        prev = sample + d * (float(self.sigmas[i + 1]) - float(self.sigmas[i]))
        self._step_index += 1
        out = SimpleNamespace(prev_sample=prev, pred_original_sample=x0)
        return out if return_dict else (prev,)


class LMSDiscreteScheduler(_SigmaScheduler):
    """Linear multistep (Adams-Bashforth on the sigma grid) sampling for the zero-terminal-SNR v-prediction schedule: the
    arithmetic of diffusers==0.29.2 `LMSDiscreteScheduler` restated for the options listed in `__init__` (any other value
    raises NotImplementedError naming the option).  `lms_order` (1..4, default 4: the `order=4` default of diffusers'
    `step`) is this project's keyword - the loop cannot pass `order` to a step; the class attribute `order` stays 1 (the
    reference reads it, pipelines/v_express_pipeline.py:582).  `rescale_betas_zero_snr` is this project's too (diffusers'
    class has no such keyword): the reference's noise_scheduler_kwargs pass unchanged.

    diffusers: X' = X + sum_j L_j d_{i-j} in the VE frame, d = eps, L_j = `lms_integrals` (here exact; diffusers
    integrates numerically to 1e-4).  In the VP frame of the loop, with E = sigma_i + L_0 formed as
    sigma_{i+1} - sum_{j>=1} L_j:
        x' = a' (a + E s) x + a' (E a - s) v + sum_{j>=1} a' L_j eps_{i-j},   eps_i = s x + a v
    with eps kept per frame in a ring of three slots - `linear_coefficients(i, begin_index)` for `vx_overlap_linear_step`.
    `step()` is the stateful diffusers-style tensor API in the VE frame."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, use_karras_sigmas=False, prediction_type="epsilon", timestep_spacing="linspace",
                 steps_offset=0, rescale_betas_zero_snr=False, lms_order=4, **unused):
        self._check_options(("trained_betas", trained_betas, trained_betas is None),
                            ("beta_schedule", beta_schedule, beta_schedule in ("linear", "scaled_linear")),
                            ("use_karras_sigmas", use_karras_sigmas, not use_karras_sigmas),
                            ("prediction_type", prediction_type, prediction_type == "v_prediction"),
                            ("timestep_spacing", timestep_spacing, timestep_spacing == "trailing"),
                            ("lms_order", lms_order, lms_order in (1, 2, 3, 4)))
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, use_karras_sigmas=use_karras_sigmas,
                                      prediction_type=prediction_type, timestep_spacing=timestep_spacing,
                                      steps_offset=steps_offset, rescale_betas_zero_snr=rescale_betas_zero_snr,
                                      lms_order=lms_order)
        self._sigma_tables()

    def order_at(self, i, begin_index=0):
        """min(i - begin_index + 1, lms_order): the number of derivatives the update of step index i combines in a run
        that started at `begin_index` (the history starts empty there)."""
        self._check_index(i, begin_index)
        return min(i - begin_index + 1, self.config.lms_order)

    def lms_coefficients(self, i, begin_index=0):
        """[L_0 .. L_{o-1}] of step index i, o = order_at(i, begin_index)."""
        return lms_integrals(self.sigmas.tolist(), i, self.order_at(i, begin_index))

    def linear_coefficients(self, i, begin_index=0):
        """LinearStep of step index i of a run that started at `begin_index`.  eps_{i-j} is read from ring slot
        (i - begin_index - j) % 3 and eps_i written to slot (i - begin_index) % 3 - at fourth order the slot of
        eps_{i-3}, read by the same update.  lms_order 1 keeps no history."""
        L = self.lms_coefficients(i, begin_index)
        (a, s), (a1, _) = self._vp_at(i), self._vp_at(i + 1)
        E = float(self.sigmas[i + 1]) - sum(L[1:])                 # sigma_i + L_0
        r = i - begin_index
        reads = [((r - j) % 3, a1 * L[j]) for j in range(1, len(L))]
        return _linear_step(a1 * (a + E * s), a1 * (E * a - s), reads,
                            h_write=r % 3 if self.config.lms_order > 1 else -1, p=(s, a))

    def step(self, model_output, timestep, sample, order=None, return_dict=True, **unused):
        """One update on tensors in the VE frame (v-prediction `model_output`), keeping the step index and the last
        derivatives like diffusers; `order` defaults to lms_order."""
        if self._step_index is None:
            self._init_step_index(timestep)
        i = self._step_index
        order = self.config.lms_order if order is None else int(order)
        x0, d = self._derivative(model_output, sample, i)
        self._derivatives = (self._derivatives + [d])[-order:]
        L = lms_integrals(self.sigmas.tolist(), i, min(len(self._derivatives), order))
        prev = sample + sum(lj * dj for lj, dj in zip(L, reversed(self._derivatives)))
        self._step_index += 1
        out = SimpleNamespace(prev_sample=prev, pred_original_sample=x0)
        return out if return_dict else (prev,)


# the Adams-Bashforth weights of diffusers' PNDMScheduler.step_plms by the number of stored outputs (newest first)
_PLMS = {1: (1.0,), 2: (3 / 2, -1 / 2), 3: (23 / 12, -16 / 12, 5 / 12), 4: (55 / 24, -59 / 24, 37 / 24, -9 / 24)}


class PNDMScheduler(_AlphaScheduler):
    """PNDM's linear multistep part (PLMS) for the zero-terminal-SNR v-prediction schedule: the arithmetic of
    diffusers==0.29.2 `PNDMScheduler` with `skip_prk_steps=True`, restated for the options listed in `__init__` (any other
    value raises NotImplementedError naming the option - diffusers' default skip_prk_steps=False, the Runge-Kutta warm-up,
    among them).  `rescale_betas_zero_snr` is this project's keyword (diffusers' class has none): the reference's
    noise_scheduler_kwargs pass unchanged; the table needs no clamp, see `_transfer`.

    `set_timesteps(N)` gives N + 1 entries, the second timestep twice: entry 0 is an Euler step whose sample is saved,
    entry 1 redoes it from the saved sample with the mean of the two outputs, entries 2, 3, >= 4 are Adams-Bashforth of
    order 2, 3, 4 over the stored outputs.  The loop runs it with `vx_overlap_linear_step`, fed by
    `linear_coefficients(n)`; `step()` is the stateful diffusers-style tensor API."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, skip_prk_steps=False, set_alpha_to_one=False, prediction_type="epsilon",
                 timestep_spacing="leading", steps_offset=0, rescale_betas_zero_snr=False, **unused):
        self._check_options(("trained_betas", trained_betas, trained_betas is None),
                            ("beta_schedule", beta_schedule, beta_schedule in ("linear", "scaled_linear")),
                            ("skip_prk_steps", skip_prk_steps, bool(skip_prk_steps)),
                            ("prediction_type", prediction_type, prediction_type == "v_prediction"),
                            ("timestep_spacing", timestep_spacing, timestep_spacing == "trailing"))
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, skip_prk_steps=skip_prk_steps,
                                      set_alpha_to_one=set_alpha_to_one, prediction_type=prediction_type,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        self._tables(sigma=False)
        self.pndm_order = 4
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)
        self._reset()

    def _reset(self):
        self.counter = 0
        self.ets = []
        self.cur_sample = None

    def set_timesteps(self, num_inference_steps, device=None):
        """diffusers' plms_timesteps under skip_prk_steps: with t the ascending trailing list,
        reverse(t[:-1] + t[-2:-1] + t[-1:]) - N + 1 entries for N >= 2, the second one repeated."""
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        t = _trailing(T, num_inference_steps, np.int64)[::-1]
        ts = np.concatenate([t[:-1], t[-2:-1], t[-1:]])[::-1].copy()
        self.timesteps = torch.from_numpy(ts)
        self._reset()

    def _abar(self, t):
        return float(self.alphas_cumprod[t]) if t >= 0 else float(self.final_alpha_cumprod)

    def _transfer(self, t_from, t_to):
        """(k_x, g) of diffusers' _get_prev_sample between two timesteps, x' = k_x b + g vc.  diffusers writes it
        sqrt(ap / a) b - (ap - a)(sqrt(a) vc + sqrt(1 - a) b) / (a sqrt(1 - ap) + sqrt(a (1 - a) ap)) on the cumulative
        alphas a (from) and ap (to), 0 / 0 at a = 0; the same map is the rotation used here,
        k_x = al' al + s' s, g = s' al - al' s with al = sqrt(a), s = sqrt(1 - a), finite on the unclamped zero-SNR table."""
        a, ap = self._abar(t_from), self._abar(t_to)
        al, s, al1, s1 = math.sqrt(a), math.sqrt(1.0 - a), math.sqrt(ap), math.sqrt(1.0 - ap)
        return al1 * al + s1 * s, s1 * al - al1 * s

    def _entry(self, n):
        self._check_index(n, n=len(self.timesteps))
        t, r = int(self.timesteps[n]), self.config.num_train_timesteps // self.num_inference_steps
        return (t + r, t) if n == 1 else (t, t - r)

    def linear_coefficients(self, n, begin_index=0):
        """LinearStep of entry n (diffusers' `counter`) of the timestep list.  The history holds the averaged model
        output itself, (p_x, p_v) = (0, 1); the k-th output stored (entry 0, then entries 2, 3, ...) goes to ring slot
        k % 3 - at fourth order the slot of the oldest one, read by the same update."""
        self._check_start(begin_index)
        k_x, g = self._transfer(*self._entry(n))
        if n == 0:
            return _linear_step(k_x, g, h_write=0, saved_mode=1, p=(0.0, 1.0))
        if n == 1:
            return _linear_step(k_x, 0.5 * g, [(0, 0.5 * g)], saved_mode=2, p=(0.0, 1.0))
        k = n - 1                                      # this entry's output is the k-th one stored
        w = _PLMS[min(k + 1, 4)]
        reads = [((k - j) % 3, g * w[j]) for j in range(1, len(w))]
        return _linear_step(k_x, g * w[0], reads, h_write=k % 3, p=(0.0, 1.0))

    def _check_start(self, begin_index, init=False):
        """The first two entries are a pair (an Euler step, redone from the saved sample): a run that starts inside the
        schedule has none.  NotImplementedError for begin_index != 0 (strength < 1) or an init clip."""
        if begin_index != 0:
            raise NotImplementedError("PNDMScheduler: begin_index != 0 (strength < 1) is not built: the warm-up pair of "
                                      "entries is not defined for a run that starts inside the schedule")
        if init:
            raise NotImplementedError("PNDMScheduler: init-video sampling (known / init_video / init_latents) is not built: "
                                      "the warm-up pair of entries is not defined for a run that starts from a noised clip")

    def loop_steps(self, timesteps, begin_index, eta=0.0, init=False):
        self._no_eta(eta)
        self._check_start(begin_index, init)
        return "linear", [self.linear_coefficients(i) for i in range(len(timesteps))]

    def step(self, model_output, timestep, sample, return_dict=True, **unused):
        """diffusers' step_plms on tensors (v-prediction `model_output`), keeping `counter`, `ets` and `cur_sample`."""
        n = self.counter
        k_x, g = self._transfer(*self._entry(n))
        if n != 1:
            self.ets = self.ets[-3:] + [model_output]
        if n == 0:
            combined, self.cur_sample = model_output, sample
        elif n == 1:
            combined, sample, self.cur_sample = (model_output + self.ets[-1]) / 2, self.cur_sample, None
        else:
            w = _PLMS[len(self.ets)]
            combined = sum(wj * e for wj, e in zip(w, reversed(self.ets)))
        prev = k_x * sample + g * combined
        self.counter += 1
        return SimpleNamespace(prev_sample=prev) if return_dict else (prev,)
