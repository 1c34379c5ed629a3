"""DDIM and DPM-Solver++ schedulers.  DDIM has the configuration the reference builds (inference.py:132-136 from
inference_v2.yaml:24-35): scaled-linear betas rescaled to zero terminal SNR, trailing timestep spacing,
v-prediction, eta = 0.  The arithmetic is diffusers==0.29.2 `DDIMScheduler` (absent third-party dependency;
restated from its published behaviour — SURVEY.md Appendix A).

Host side only: the per-step update itself runs in the fused `vx_overlap_ddim_step` kernel, fed by
`step_coefficients(t)`; `step()` is kept as the reference-compatible tensor API.  DPMSolverMultistepScheduler (the
second-order multistep sampler of the reference's scheduler list, pipelines/v_express_pipeline.py:83-90) feeds
`vx_overlap_multistep_step` the same way through `multistep_coefficients(i)`.  The ancestral samplers (DDIM with
eta > 0 through `DDIMScheduler.ancestral_coefficients(t, eta)`, EulerAncestralDiscreteScheduler through
`ancestral_coefficients(i)`) feed `vx_overlap_ancestral_step`, which draws its noise on the device.
"""
from types import SimpleNamespace

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


class DDIMScheduler:
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type="epsilon",
                 timestep_spacing="leading", rescale_betas_zero_snr=False, **unused):
        betas = _betas(num_train_timesteps, beta_start, beta_end, beta_schedule, rescale_betas_zero_snr)
        self.betas = betas
        self.alphas_cumprod = torch.cumprod(1.0 - betas, 0)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, clip_sample=clip_sample,
                                      steps_offset=steps_offset, prediction_type=prediction_type,
                                      timestep_spacing=timestep_spacing, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, set_alpha_to_one=set_alpha_to_one,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        if clip_sample:
            raise NotImplementedError("clip_sample=True is not used by V-Express (inference_v2.yaml:28)")
        if prediction_type != "v_prediction":
            raise NotImplementedError("only v_prediction (inference_v2.yaml:31) is built")
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.arange(num_train_timesteps - 1, -1, -1)

    def set_timesteps(self, num_inference_steps, device=None):
        T, sp = self.config.num_train_timesteps, self.config.timestep_spacing
        self.num_inference_steps = num_inference_steps
        if sp == "trailing":
            ts = np.round(np.arange(T, 0, -T / num_inference_steps)).astype(np.int64) - 1
        elif sp == "leading":
            ts = (np.arange(0, num_inference_steps) * (T // num_inference_steps)).round()[::-1].astype(np.int64)
            ts = ts + self.config.steps_offset
        elif sp == "linspace":
            ts = np.linspace(0, T - 1, num_inference_steps).round()[::-1].astype(np.int64)
        else:
            raise ValueError(sp)
        self.timesteps = torch.from_numpy(ts.copy())

    def scale_model_input(self, sample, timestep=None):
        return sample

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
        """diffusers' DDIMScheduler.add_noise: sqrt(abar_t) x0 + sqrt(1 - abar_t) noise, t one timestep or one per
        sample of the batch (host torch arithmetic; the loop forms its start latents with vx_known_blend)."""
        abar = [float(self.alphas_cumprod[int(t)]) for t in _timestep_list(timesteps)]
        a = _per_sample([math.sqrt(v) for v in abar], original_samples)
        s = _per_sample([math.sqrt(1.0 - v) for v in abar], original_samples)
        return a * original_samples + s * noise

    def step(self, model_output, timestep, sample, eta=0.0, **unused):
        if eta != 0.0:
            raise NotImplementedError("eta != 0 is not used by V-Express")
        sa, s1a, sap, s1ap = self.step_coefficients(timestep)
        x0 = sa * sample - s1a * model_output
        eps = sa * model_output + s1a * sample
        return SimpleNamespace(prev_sample=sap * x0 + s1ap * eps, pred_original_sample=x0)


class DPMSolverMultistepScheduler:
    """DPM-Solver++ (multistep, data prediction, midpoint) for the zero-terminal-SNR v-prediction schedule: the arithmetic
    of diffusers==0.29.2 `DPMSolverMultistepScheduler` restated for the options listed in `__init__` (any other value
    raises NotImplementedError naming the option).

    The loop runs the update in the fused `vx_overlap_multistep_step` kernel, fed by `multistep_coefficients(i)`:
        x0 = alpha_i x - sigma_i v ;   x' = c_x x - c_0 x0 + c_1 x0_prev
    with the previous step's x0 kept on the device.  `step()` is the stateful diffusers-style tensor API.
    """
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, solver_order=2, prediction_type="epsilon", thresholding=False,
                 dynamic_thresholding_ratio=0.995, sample_max_value=1.0, algorithm_type="dpmsolver++",
                 solver_type="midpoint", lower_order_final=True, euler_at_final=False, use_karras_sigmas=False,
                 use_lu_lambdas=False, final_sigmas_type="zero", lambda_min_clipped=-float("inf"),
                 variance_type=None, timestep_spacing="linspace", steps_offset=0, rescale_betas_zero_snr=False,
                 **unused):
        # (clip_sample, set_alpha_to_one, ... of a DDIM configuration are not parameters of this solver: ignored, as
        # diffusers' from_config does)
        for name, value, ok in (("trained_betas", trained_betas, trained_betas is None),
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
                                ("timestep_spacing", timestep_spacing, timestep_spacing == "trailing")):
            if not ok:
                raise NotImplementedError(f"DPMSolverMultistepScheduler: {name}={value!r} is not built")
        self.betas = _betas(num_train_timesteps, beta_start, beta_end, beta_schedule, rescale_betas_zero_snr)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, 0)
        if rescale_betas_zero_snr:
            # the zero-SNR table ends at alphas_cumprod = 0: diffusers clamps it so that the first sigma is finite
            self.alphas_cumprod[-1] = 2 ** -24
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, solver_order=solver_order,
                                      prediction_type=prediction_type, algorithm_type=algorithm_type,
                                      solver_type=solver_type, lower_order_final=lower_order_final,
                                      euler_at_final=euler_at_final, final_sigmas_type=final_sigmas_type,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        # sigma(t) = sqrt((1 - abar_t) / abar_t) in float32, as diffusers computes it
        self.sigma_table = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = None
        self.sigmas = None
        self._reset()

    @classmethod
    def from_config(cls, cfg, **overrides):
        """From a dict or another scheduler's `config` (e.g. `DDIMScheduler(...).config`)."""
        cfg = dict(cfg) if isinstance(cfg, dict) else dict(vars(cfg))
        cfg.update(overrides)
        return cls(**cfg)

    def _reset(self):
        self.step_index = None
        self._x0_prev = None
        self._taken = 0

    def set_timesteps(self, num_inference_steps, device=None):
        T = self.config.num_train_timesteps
        self.num_inference_steps = num_inference_steps
        ts = np.round(np.arange(T, 0, -T / num_inference_steps)).astype(np.int64) - 1
        self.timesteps = torch.from_numpy(ts.copy())
        sig = self.sigma_table[self.timesteps]
        last = torch.zeros(1) if self.config.final_sigmas_type == "zero" else self.sigma_table[:1]
        self.sigmas = torch.cat([sig, last]).to(torch.float32)
        self._reset()

    def scale_model_input(self, sample, timestep=None):
        return sample

    def solver_order_at(self, i, begin_index=0):
        """Order of the update at step index i of a run that started at `begin_index` (diffusers' step(): first order
        at the first step of a run, at solver_order 1, and at the last step under final_sigmas_type "zero",
        euler_at_final, or lower_order_final below 15 steps).  diffusers' other small-n rule, `lower_order_second` at
        i = n - 2, caps the order at 2 and so changes nothing for solver_order <= 2."""
        cfg, n = self.config, self.num_inference_steps
        if n is None:
            raise RuntimeError("call set_timesteps() first")
        if not begin_index <= i < n:
            raise IndexError(f"step index {i} outside [{begin_index}, {n})")
        last = i == n - 1 and (cfg.euler_at_final or (cfg.lower_order_final and n < 15)
                               or cfg.final_sigmas_type == "zero")
        return 1 if (cfg.solver_order == 1 or i == begin_index or last) else 2

    def multistep_coefficients(self, i, begin_index=0):
        """(alpha_i, sigma_i, c_x, c_0, c_1) of step index i: x0 = alpha_i x - sigma_i v, x' = c_x x - c_0 x0 + c_1 x0_prev.
        Float64 arithmetic on the float32 sigma table; a step that ends at sigma = 0 returns x0 exactly (c_x = 0,
        c_0 = -1, c_1 = 0), so no inf or NaN reaches the kernel."""
        order = self.solver_order_at(i, begin_index)
        sg = [float(s) for s in self.sigmas]

        def alpha(s):
            return 1.0 / math.sqrt(s * s + 1.0)
        s0, s1 = sg[i], sg[i + 1]
        a_i, sd_i = alpha(s0), s0 * alpha(s0)
        if s1 == 0.0:
            return a_i, sd_i, 0.0, -1.0, 0.0
        h = math.log(s0) - math.log(s1)                                    # lambda = -log sigma
        A = alpha(s1) * math.expm1(-h)
        c_x = (s1 * alpha(s1)) / sd_i
        B = 0.0
        if order == 2:
            r = (math.log(sg[i - 1]) - math.log(s0)) / h
            B = 0.5 * A / r
        return a_i, sd_i, c_x, A + B, B

    def _indices_of(self, timesteps):
        """Step indices of schedule timesteps (diffusers' index_for_timestep: the first match)."""
        own = [float(t) for t in self.timesteps.tolist()]
        out = []
        for t in _timestep_list(timesteps):
            if t not in own:
                raise ValueError(f"timestep {t} is not in this schedule")
            out.append(own.index(t))
        return out

    def noise_coefficients(self, j):
        """(a_j, s_j) = (alpha_t, sigma_t) of sigmas[j], the level the latents have at step index j (j = number of
        steps: the final sigma).  Float64 arithmetic on the float32 sigmas."""
        if self.sigmas is None or self.num_inference_steps is None:
            raise RuntimeError("call set_timesteps() first")
        if not 0 <= j <= self.num_inference_steps:
            raise IndexError(f"step index {j} outside [0, {self.num_inference_steps}]")
        sg = float(self.sigmas[j])
        a = 1.0 / math.sqrt(sg * sg + 1.0)
        return a, sg * a

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' DPMSolverMultistepScheduler.add_noise: alpha_t x0 + sigma_t noise at the schedule's own timesteps
        (one, or one per sample of the batch)."""
        pairs = [self.noise_coefficients(i) for i in self._indices_of(timesteps)]
        a = _per_sample([p[0] for p in pairs], original_samples)
        s = _per_sample([p[1] for p in pairs], original_samples)
        return a * original_samples + s * noise

    def step(self, model_output, timestep, sample, return_dict=True, **unused):
        """One update on tensors (v-prediction `model_output`), keeping the step index and the last x0 like diffusers."""
        if self.step_index is None:
            hits = (self.timesteps == int(timestep)).nonzero()
            if len(hits) == 0:
                raise ValueError(f"timestep {int(timestep)} is not in this schedule")
            self.step_index = int(hits[0])
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


class EulerAncestralDiscreteScheduler:
    """Euler ancestral sampling for the zero-terminal-SNR v-prediction schedule: the arithmetic of diffusers==0.29.2
    `EulerAncestralDiscreteScheduler` restated for the options listed in `__init__` (any other value raises
    NotImplementedError naming the option).

    diffusers works in the VE frame (x_ve = x0 + sigma eps, `scale_model_input` divides by sqrt(1 + sigma^2)).  The loop
    runs in the VP frame x_vp = x_ve / sqrt(1 + sigma^2) - exactly the UNet input - with the update of the fused
    `vx_overlap_ancestral_step` kernel, fed by `ancestral_coefficients(i)`:
        x0 = alpha_s x - sigma_s v ;   x' = c_x x - c_0 x0 + c_z z
    `step()` is the stateful diffusers-style tensor API in the VE frame.
    """
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                 trained_betas=None, prediction_type="epsilon", timestep_spacing="linspace", steps_offset=0,
                 rescale_betas_zero_snr=False, **unused):
        # (clip_sample, set_alpha_to_one, ... of a DDIM configuration are not parameters of this sampler: ignored, as
        # diffusers' from_config does)
        for name, value, ok in (("trained_betas", trained_betas, trained_betas is None),
                                ("beta_schedule", beta_schedule, beta_schedule == "scaled_linear"),
                                ("prediction_type", prediction_type, prediction_type == "v_prediction"),
                                ("timestep_spacing", timestep_spacing, timestep_spacing == "trailing")):
            if not ok:
                raise NotImplementedError(f"EulerAncestralDiscreteScheduler: {name}={value!r} is not built")
        self.betas = _betas(num_train_timesteps, beta_start, beta_end, beta_schedule, rescale_betas_zero_snr)
        self.alphas_cumprod = torch.cumprod(1.0 - self.betas, 0)
        if rescale_betas_zero_snr:
            # the zero-SNR table ends at alphas_cumprod = 0: diffusers clamps it so that the first sigma is finite
            self.alphas_cumprod[-1] = 2 ** -24
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, prediction_type=prediction_type,
                                      timestep_spacing=timestep_spacing, steps_offset=steps_offset,
                                      rescale_betas_zero_snr=rescale_betas_zero_snr)
        # sigma(t) = sqrt((1 - abar_t) / abar_t) in float32, as diffusers computes it
        self.sigma_table = ((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5
        self.sigmas = torch.cat([self.sigma_table.flip(0), torch.zeros(1)]).to(torch.float32)
        self.timesteps = torch.linspace(0, num_train_timesteps - 1, num_train_timesteps,
                                        dtype=torch.float64).flip(0).to(torch.float32)
        self.num_inference_steps = None
        self._step_index = None
        self._begin_index = None

    @classmethod
    def from_config(cls, cfg, **overrides):
        """From a dict or another scheduler's `config` (e.g. `DDIMScheduler(...).config`)."""
        cfg = dict(cfg) if isinstance(cfg, dict) else dict(vars(cfg))
        cfg.update(overrides)
        return cls(**cfg)

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
        ts = np.arange(T, 0, -T / num_inference_steps).round().astype(np.float32) - 1
        self.timesteps = torch.from_numpy(ts.copy())
        sig = self.sigma_table[self.timesteps.long()]
        self.sigmas = torch.cat([sig, torch.zeros(1)]).to(torch.float32)
        self._step_index = None
        self._begin_index = None

    def _init_step_index(self, timestep):
        if self._begin_index is not None:
            self._step_index = self._begin_index
            return
        hits = (self.timesteps == float(timestep)).nonzero()
        if len(hits) == 0:
            raise ValueError(f"timestep {float(timestep)} is not in this schedule")
        self._step_index = int(hits[1 if len(hits) > 1 else 0])

    def scale_model_input(self, sample, timestep=None):
        """x_ve -> x_vp = x_ve / sqrt(1 + sigma^2) at the current step (diffusers' scaling of the UNet input)."""
        if self._step_index is None:
            self._init_step_index(timestep)
        sigma = self.sigmas[self._step_index]
        return sample / ((sigma ** 2 + 1) ** 0.5)

    def ancestral_coefficients(self, i):
        """(alpha_s, sigma_s, c_x, c_0, c_z) of step index i in the VP frame: x0 = alpha_s x - sigma_s v,
        x' = c_x x - c_0 x0 + c_z z with x, x' = x_ve / sqrt(1 + sigma^2) at sigmas[i], sigmas[i + 1].  Float64
        arithmetic on the float32 sigmas; a step that ends at sigma = 0 returns x0 exactly (c_x = 0, c_0 = -1, c_z = 0)."""
        n = self.num_inference_steps
        if n is None:
            raise RuntimeError("call set_timesteps() first")
        if not 0 <= i < n:
            raise IndexError(f"step index {i} outside [0, {n})")
        s, s1 = float(self.sigmas[i]), float(self.sigmas[i + 1])
        r = math.sqrt(1.0 + s * s)
        alpha_s, sigma_s = 1.0 / r, s / r
        if s1 == 0.0:
            return alpha_s, sigma_s, 0.0, -1.0, 0.0
        s_up = math.sqrt(s1 * s1 * (s * s - s1 * s1) / (s * s))
        s_down = math.sqrt(s1 * s1 - s_up * s_up)
        r1 = math.sqrt(1.0 + s1 * s1)
        return alpha_s, sigma_s, r * s_down / (s * r1), -(1.0 - s_down / s) / r1, s_up / r1

    def noise_coefficients(self, j):
        """(a_j, s_j) = (1, sigma_j) / sqrt(1 + sigma_j^2) of sigmas[j]: the variance-preserving pair of the frame the
        loop runs in (x_vp = x_ve / sqrt(1 + sigma^2)); j = number of steps: the final sigma = 0, (1, 0)."""
        n = self.num_inference_steps
        if n is None:
            raise RuntimeError("call set_timesteps() first")
        if not 0 <= j <= n:
            raise IndexError(f"step index {j} outside [0, {n}]")
        sg = float(self.sigmas[j])
        a = 1.0 / math.sqrt(sg * sg + 1.0)
        return a, sg * a

    def add_noise(self, original_samples, noise, timesteps):
        """diffusers' EulerAncestralDiscreteScheduler.add_noise, in the scheduler's own (VE) frame: x0 + sigma noise at
        the schedule's own timesteps (one, or one per sample of the batch)."""
        own = [float(t) for t in self.timesteps.tolist()]
        sig = []
        for t in _timestep_list(timesteps):
            if t not in own:
                raise ValueError(f"timestep {t} is not in this schedule")
            sig.append(float(self.sigmas[own.index(t)]))
        return original_samples + _per_sample(sig, original_samples) * noise

    def frame_scale(self, i):
        """sqrt(1 + sigmas[i]^2): x_ve = frame_scale(i) x_vp at step index i (1 at the final sigma = 0)."""
        s = float(self.sigmas[i])
        return math.sqrt(1.0 + s * s)

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
