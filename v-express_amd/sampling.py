"""The four parts of `VExpressPipeline.denoise`, each resolved once before the loop into an object that holds its own
buffers and host-side coefficients, so that a timestep reads straight down:
    UNet calls of guidance.plan(i) -> all_gather_units -> guidance.combine -> stitch.reduce -> sampler.update -> known.after
  Stitch    how the window predictions of a step become one prediction per frame: the mean plan, or the weighted pre-pass;
  Guidance  which rows a step runs per window and the one launch that combines them (rescaled or not);
  Sampler   the update and the per-step coefficients the scheduler in use names (scheduler.loop_steps), that update's
            buffers and, for a scheduler that has `frame_scale` - the sigma (VE) ones: Euler ancestral, Euler, LMS - the
            VE <-> VP frame;
  Known     the known region of init-video sampling: the start latents and the blend after every step.
A choice that does not depend on the timestep is made in a constructor (a method bound there), never in the loop.  Every
kernel wrapper is looked up as `ops.<name>` when it is called: tests and tools replace them there."""
import struct
from typing import Any, List, NamedTuple

import torch

from . import ops

# The batch rows a window can run, as (bank row, keypoint row, audio row) of the CFG-layout conditioning (row 0 zeros,
# row 1 real): "u" drops everything, "m" ("silent") keeps the reference bank and the keypoints and drops the audio, "c"
# keeps everything.
GUIDANCE_ROWS = {"u": (0, 0, 0), "m": (1, 1, 0), "c": (1, 1, 1)}


REUSE_MODES = ("hold", "linear")


def refresh_roles(guided, refresh):
    """The role of every step under guidance reuse with the period `refresh`: None for an unguided step, "refresh" for a
    guided step that runs all its rows - the first and the last guided step, and every guided step that `refresh` - 1
    reuse steps precede since the last refresh - and "reuse" for the guided steps between, which run the conditional row
    alone.  Unguided steps do not count towards the period."""
    idx = [i for i, g in enumerate(guided) if g]
    roles, since = [None] * len(guided), 0
    for n, i in enumerate(idx):
        if n == 0 or n == len(idx) - 1 or since == refresh - 1:
            roles[i], since = "refresh", 0
        else:
            roles[i], since = "reuse", since + 1
    return roles


def reuse_coefficients(scales, w):
    """(a_k, b_k) of a reuse step per guidance difference with the scale s_k: u + s (m - u) + s_a (c - m) rewritten around
    c, c + sum (s_k - 1) d_k, with d_k extrapolated from the last two refreshes, d_k = (1 + w) L_k - w P_k: a_k =
    (s_k - 1)(1 + w), b_k = -(s_k - 1) w.  Formed in double, each rounded to float32 once."""
    def f32(v):
        return struct.unpack("f", struct.pack("f", v))[0]
    return [(f32((s - 1.0) * (1.0 + w)), f32(-(s - 1.0) * w) if w else 0.0) for s in scales]


class UnitCall(NamedTuple):
    """One UNet call of a step plan (VExpressPipeline._unit_plan): the reference-bank row of every batch row; (frame ids
    int32 [f_loc], repeats) of every window; the keypoint and audio tokens of the rows, the step-invariant audio K | V
    (unet.precompute_audio_kv) and which rows carry all-zero audio; the frames of a window this rank computes and their
    frame-shard group; the first send slot of the call and how many it fills."""
    bank_rows: List[int]
    gathers: list
    kps: torch.Tensor
    ehs: torch.Tensor
    audio_kv: Any
    audio_zero: List[bool]
    f_loc: int
    shard: Any
    s0: int
    n_slots: int


class Stitch:
    """Mean of the overlapping predictions (the reference's 1 / count, summed inside the update) or, for a weighted blend,
    one vx_overlap_blend launch per step into `blended`, one "window" of F frames that the update reads through the
    trivial plan (one term, count 1).  Identical on every rank, like the update.  `report` is last_overlap."""

    def __init__(self, plan, weighted, blend_kind, nW, C, F, hw, steps, dev):
        # plan: context.overlap_plan, or context.weighted_overlap_plan for a weighted blend
        if not weighted:
            sf = plan["step_frames"]
            terms = torch.full((len(sf), plan["max_terms"], 2), -1, dtype=torch.int32)
            for i, fr in enumerate(sf):
                for j, (wi, li) in enumerate(plan["terms"][fr]):
                    terms[i, j, 0], terms[i, j, 1] = wi, li
            self.terms = terms.to(dev)
            self.frame_ids = torch.tensor(sf, dtype=torch.int32, device=dev)
            self.counts = torch.tensor([float(plan["counts"][fr]) for fr in sf], dtype=torch.float32, device=dev)
            self.blended, self._reduce = None, self._window_preds
        else:
            self.blend_terms = torch.from_numpy(plan["term_table"]).to(dev)
            self.blend_w = torch.from_numpy(plan["weights"]).to(dev)
            self.blended = torch.empty((1, C, F, hw), device=dev, dtype=torch.float32)
            self.frame_ids = torch.arange(F, dtype=torch.int32, device=dev)
            self.terms = torch.stack([torch.zeros_like(self.frame_ids), self.frame_ids], dim=1).view(F, 1, 2).contiguous()
            self.counts = torch.ones(F, dtype=torch.float32, device=dev)
            self._reduce = self._blend
        self.report = dict(schedule=None, blend=blend_kind, windows=nW, max_terms=plan["max_terms"],
                           blend_launches=0 if self.blended is None else steps)

    def reduce(self, preds):
        """The buffer the update reads: `preds` itself on the mean route, `blended` after one vx_overlap_blend."""
        return self._reduce(preds)

    def _window_preds(self, preds):
        return preds

    def _blend(self, preds):
        ops.overlap_blend(preds, self.blend_terms, self.blend_w, self.blended)
        return self.blended


class Guidance:
    """The rows of a guided step (`row_names`: guidance_rows), the plan of the guided steps and - only when some step runs
    without guidance - the plan of the conditional row alone, and the one launch that turns a step's gathered units into
    window predictions: vx_combine_units, vx_combine_units3, vx_guidance_rescale, vx_guidance_rescale3 or - with
    `apg` = (eta, norm_threshold, momentum) - vx_guidance_apg, whose workspace and zero-initialised momentum buffers
    (`momentum`: one per guidance difference, advanced by the guided steps only) live here.
    Guidance reuse, `reuse` = (refresh period k > 1, "hold" | "linear"): the guided steps take the roles of refresh_roles;
    a refresh step runs the guided plan and vx_combine_units_keep, which also stores the differences of consecutive rows
    in `slots` (float32 [1 or 2][rows - 1, nW, C, f, hw]; refresh number j writes slot j % 2 in the "linear" mode, the
    one slot in the "hold" mode); a reuse step runs the conditional-only plan of an unguided step and vx_combine_reused
    on the slots, with the coefficients of reuse_coefficients.  Unguided steps neither read nor advance the slots, which
    are identical on every rank, like the momentum buffers.
    `unit_plan(half_rows)` builds a plan (VExpressPipeline._unit_plan, given the all-zero audio rows): collective, so both
    plans are built here, on every rank, before the loop.  `report` is last_guidance, `schedule` last_schedule."""

    def __init__(self, row_names, guidance_scale, audio_guidance_scale, rescale, guided, kps_tokens, audio, unit_plan,
                 nW, C, f, hw, dev, apg=None, reuse=None):
        steps = len(guided)
        do_cfg = len(row_names) > 1                   # a guided step combines rows
        cond_rows = 2 if do_cfg else 1
        if kps_tokens.shape[0] != cond_rows or audio.shape[0] != cond_rows:
            what = f"guidance_scale={guidance_scale}"
            if row_names in (("m", "c"), ("u", "m", "c")):
                what += f" with audio_guidance_scale={audio_guidance_scale} (the silent row takes the zero-audio row 0)"
            raise ValueError(f"{what} needs {cond_rows} batch row(s) of kps features / audio embeddings, got "
                             f"{kps_tokens.shape[0]} / {audio.shape[0]}")
        if not do_cfg:                                # nothing to rescale, nothing to switch off
            rescale, guided = 0.0, [True] * steps
        # which CFG halves carry all-zero audio tokens (the unconditional half, :403-405): one device reduction per clip
        audio_is_zero = [bool((audio[hh] == 0).all().item()) for hh in range(audio.shape[0])]
        # (the one-scale routes name their rows by index, as they always have; a silent row needs the triple)
        half_rows = [GUIDANCE_ROWS[r] for r in row_names] if "m" in row_names else list(range(cond_rows))
        self.plan_g = unit_plan(audio_is_zero, half_rows)
        # (a reuse step issues exactly an unguided step's UNet calls: the same plan object)
        roles = refresh_roles(guided, reuse[0]) if reuse is not None and do_cfg else None
        reusing = roles is not None and "reuse" in roles
        self.plan_c = None if all(guided) and not reusing else unit_plan(audio_is_zero, [1])
        self.schedule = self.plan_g["schedule"]
        self.report = dict(guided_steps=sum(guided) if do_cfg else 0, steps=steps, rescale=rescale,
                           unguided_schedule=None if self.plan_c is None else self.plan_c["schedule"])
        if audio_guidance_scale is not None:
            self.report.update(rows=row_names, audio_scale=float(audio_guidance_scale))
        # the one scale of a two-row combine: (m, c) is guided by the audio scale; one row: u + 1 (u - u)
        scale2 = (float(audio_guidance_scale) if row_names == ("m", "c") else guidance_scale) if do_cfg else 1.0
        if apg is not None:                           # (like the rescale: nothing to project without guidance)
            self.report.update(apg=dict(zip(("eta", "norm_threshold", "momentum"), apg)) if do_cfg else None)
            apg = apg if do_cfg and any(guided) else None
        ws = self.momentum = None
        if rescale > 0.0 and any(guided):
            ws = torch.empty(ops.guidance_rescale_ws_floats(nW, f, hw), device=dev, dtype=torch.float32)
        if apg is not None:
            eta, r, beta = apg
            ws = torch.empty(ops.guidance_apg_ws_floats(nW, len(row_names), f, hw), device=dev, dtype=torch.float32)
            if beta != 0.0:
                self.momentum = torch.zeros((len(row_names) - 1, nW, C, f, hw), device=dev, dtype=torch.float32)
        geo, s, s_a, self.workspace = (C, f, hw), guidance_scale, audio_guidance_scale, ws

        # the launch of a guided step - u + s (m - u) + s_a (c - m) or the CFG combine (:548-550), each window rescaled
        # towards its conditional row's spread or not - and of an unguided one: the conditional prediction itself
        def rescale3(g, u, p): ops.guidance_rescale3(g, u, *geo, s, s_a, rescale, ws, p)
        def combine3(g, u, p): ops.combine_units3(g, u, *geo, s, s_a, p)
        def rescale2(g, u, p): ops.guidance_rescale(g, u, *geo, scale2, rescale, ws, p)
        def combine2(g, u, p): ops.combine_units(g, u, *geo, scale2, p)
        def conditional(g, u, p): ops.combine_units(g, u, *geo, 1.0, p)
        # adaptive projected guidance: every difference of the rows projected on c, capped and run through its momentum
        def apg3(g, u, p): ops.guidance_apg(g, u, *geo, s, s_a, eta, r, beta, self.momentum, ws, p)
        def apg2(g, u, p): ops.guidance_apg(g, u, *geo, scale2, 0.0, eta, r, beta, self.momentum, ws, p)
        if apg is not None:
            guided_op = apg3 if len(row_names) == 3 else apg2
        elif len(row_names) == 3:
            guided_op = combine3 if ws is None else rescale3
        else:
            guided_op = combine2 if ws is None else rescale2
        self.plans = [self.plan_g if g else self.plan_c for g in guided]
        self.combines = [guided_op if g else conditional for g in guided]
        self.slots = None
        if reuse is not None:
            self.report.update(refresh=reuse[0], reuse=reuse[1],
                               refresh_steps=[i for i, r in enumerate(roles or []) if r == "refresh"])
        if reusing:
            scales = (s, s_a) if len(row_names) == 3 else (scale2,)
            self._reuse(roles, reuse[1], scales, geo, (nW, C, f, hw), dev)

    def _reuse(self, roles, mode, scales, geo, shape, dev):
        """The plans and launches of the refresh and reuse steps (some step reuses): allocates the slots."""
        nd = len(scales)
        self.slots = torch.empty((2 if mode == "linear" else 1, nd) + shape, device=dev, dtype=torch.float32)
        s, s_a = (scales + (0.0,))[:2]

        def keep(slot):
            def op(g, u, p): ops.combine_units_keep(g, u, *geo, s, s_a, slot, p)
            return op

        def reused(last, prev, coef):
            (a1, b1), (a2, b2) = (coef + [(0.0, 0.0)])[:2]
            prev = prev if b1 != 0.0 or b2 != 0.0 else None

            def op(g, u, p): ops.combine_reused(g, u, *geo, last, prev, a1, b1, a2, b2, p)
            return op
        done = []                                     # the step indices of the refreshes so far
        for i, role in enumerate(roles):
            if role == "refresh":
                self.combines[i] = keep(self.slots[len(done) % len(self.slots)])
                done.append(i)
            elif role == "reuse":
                last = self.slots[(len(done) - 1) % len(self.slots)]
                w = 0.0
                if mode == "linear" and len(done) > 1:
                    w = (i - done[-1]) / (done[-1] - done[-2])
                self.plans[i] = self.plan_c
                self.combines[i] = reused(last, self.slots[len(done) % len(self.slots)], reuse_coefficients(scales, w))

    def plan(self, i):
        return self.plans[i]

    def combine(self, i, gathered, uidx, preds):
        self.combines[i](gathered, uidx, preds)


class Sampler:
    """The update of one frame set per timestep, `update` and `coefs` as the scheduler's loop_steps returned them: "ddim"
    (vx_overlap_ddim_step), "multistep" (vx_overlap_multistep_step, with the previous step's x0 of every frame in
    `x0_hist`: identical on every rank, like the latents), "ancestral" (vx_overlap_ancestral_step, noise keyed by
    `noise_seed` and the step index) or "linear" (vx_overlap_linear_step, with `history`, three per-frame slots, and
    `saved`, PNDM's saved sample: allocated only when some step names them, never read before they are written, identical
    on every rank) or "unipc" (vx_overlap_unipc_step, with `history`, the data predictions of the last three steps of every
    frame, and `saved`, the corrected sample the next corrector starts from: identical on every rank, never read before
    they are written, and not touched by the known blend, like the DPM++ history).  A scheduler that has `frame_scale`
    (Euler ancestral, Euler, LMS): the latents come and go in its (VE) frame and the loop runs in the VP frame
    x / sqrt(1 + sigma^2); None for the others."""

    def __init__(self, scheduler, update, coefs, latents, begin_index, noise_seed):
        self.begin_index, self.steps, self.coefs = begin_index, len(coefs), coefs
        self.frame_scale = getattr(scheduler, "frame_scale", None) if coefs else None
        if update == "multistep":
            self.x0_hist = torch.empty_like(latents)
        elif update == "ancestral":
            self.noise_seed = int(noise_seed)
        elif update == "linear":
            slots = any(max(cf[:4]) >= 0 for cf in coefs)
            self.history = torch.empty((3,) + tuple(latents.shape[1:]), device=latents.device,
                                       dtype=torch.float32) if slots else None
            self.saved = torch.empty_like(latents) if any(cf.saved_mode for cf in coefs) else None
        elif update == "unipc":                       # (every update writes a history slot and the saved sample)
            self.history = torch.empty((3,) + tuple(latents.shape[1:]), device=latents.device, dtype=torch.float32)
            self.saved = torch.empty_like(latents)
        self._update = {"ddim": self._ddim, "multistep": self._multistep, "ancestral": self._ancestral,
                        "linear": self._linear, "unipc": self._unipc}[update]

    def start(self, latents):
        if self.frame_scale is not None:
            latents.mul_(1.0 / self.frame_scale(self.begin_index))               # VE -> VP, once

    def update(self, i, t, latents, step_preds, stitch):
        """The update of step i (timestep t) on the frames of the stitch's plan."""
        self._update(i, latents, step_preds, stitch)

    def _ddim(self, i, latents, step_preds, stitch):
        ops.overlap_ddim_step(latents, step_preds, stitch.terms, stitch.frame_ids, stitch.counts, self.coefs[i])

    def _multistep(self, i, latents, step_preds, stitch):
        ops.overlap_multistep_step(latents, step_preds, stitch.terms, stitch.frame_ids, stitch.counts, self.x0_hist,
                                   self.coefs[i])

    def _ancestral(self, i, latents, step_preds, stitch):
        ops.overlap_ancestral_step(latents, step_preds, stitch.terms, stitch.frame_ids, stitch.counts, self.coefs[i],
                                   self.noise_seed, self.begin_index + i)

    def _linear(self, i, latents, step_preds, stitch):
        ops.overlap_linear_step(latents, step_preds, stitch.terms, stitch.frame_ids, stitch.counts, self.history,
                                self.saved, self.coefs[i])

    def _unipc(self, i, latents, step_preds, stitch):
        ops.overlap_unipc_step(latents, step_preds, stitch.terms, stitch.frame_ids, stitch.counts, self.history,
                               self.saved, self.coefs[i])

    def callback_view(self, i, latents):
        """What a callback sees after step i: the scheduler's own (VE) frame for the sigma schedulers, as the reference's."""
        if self.frame_scale is None:
            return latents
        return latents * self.frame_scale(self.begin_index + i + 1)

    def finish(self, latents):
        if self.frame_scale is not None:
            scale = self.frame_scale(self.begin_index + self.steps)
            if scale != 1.0:                                                     # a run that stops before sigma = 0
                latents.mul_(scale)


def check_known(known, latents):
    """Validates the `known` argument of denoise against the latents; returns (init, noise, mask), all None without it."""
    if known is None:
        return None, None, None
    init, noise, kmask = known
    for t, name in ((init, "init"), (noise, "noise")):
        if tuple(t.shape) != tuple(latents.shape):
            raise ValueError(f"known: {name} must be shaped like the latents {tuple(latents.shape)}, got "
                             f"{tuple(t.shape)}")
    want = (latents.shape[2], latents.shape[3] * latents.shape[4])
    if kmask is not None and tuple(kmask.shape) != want:
        raise ValueError(f"known: the latent mask must be [F, h * w] = {list(want)}, got {tuple(kmask.shape)}")
    return init, noise, kmask


class Known:
    """Init-video sampling: (init, noise, mask) of check_known and the scheduler's (a, s) of the start and of the blend
    after every step, resolved on the host.  `start` forms the start latents a_b init + s_b noise in the frame the loop
    runs in (the sigma schedulers: the VP frame, (init + sigma noise) / sqrt(1 + sigma^2)); `after` puts the kept part back at
    the level the latents have after step i (init itself after the last step) - with a mask only.  `report` is last_init."""

    def __init__(self, scheduler, init, noise, mask, steps, begin_index):
        self.init, self.noise, self.mask, self._after = init, noise, mask, self._nothing
        self.active = init is not None
        self.scheduler, self.begin_index = scheduler, begin_index
        if mask is not None:
            self.blend = [(1.0, 0.0) if i == steps - 1 else scheduler.noise_coefficients(begin_index + i + 1)
                          for i in range(steps)]
            self._after = self._blend
        self.report = dict(begin_index=begin_index, masked=mask is not None,
                           blend_launches=(1 + (steps if mask is not None else 0)) if self.active else 0)

    def start(self, latents):
        ops.known_blend(latents, self.init, self.noise, None, *self.scheduler.noise_coefficients(self.begin_index))

    def after(self, i, latents):
        self._after(i, latents)

    def _nothing(self, i, latents):
        """No mask (plain img2img, or no init clip at all): nothing after the start."""

    def _blend(self, i, latents):
        ops.known_blend(latents, self.init, self.noise, self.mask, *self.blend[i])
