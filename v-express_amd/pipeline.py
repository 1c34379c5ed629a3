"""Drop-in for the reference `VExpressPipeline` (pipelines/v_express_pipeline.py:71-646) with the hot loop on
libvexpress_hip kernels and everything resident in HBM.

Same constructor kwargs and `__call__` signature/defaults as the reference (SURVEY.md §8b surface #1); returns
a float32 `[1, 3, F, H, W]` tensor in [0, 1] (on the CPU like the reference unless `output_device` is given).

Differences that change memory/time but not results: latents, kps features and
predictions never visit the host (the reference keeps latents and kps features on the CPU and copies a window
up/down every step: :363,:521,:531,:538,:572); the per-frame Python bookkeeping of :552-572 is replayed once on
the host into a static plan (context.overlap_plan) and executed by two small kernels; CFG + 1/count + sum + DDIM
step are fused; the VAE decodes frames in batches.  With `torch.distributed` initialised the (window, CFG-half)
units of a timestep are sharded over the ranks (distributed.py) — the reference's
`do_multi_devices_inference` flag is accepted and, as in the reference, changes nothing by itself.

Once-per-clip prologue: VKpsGuider, AudioProjection and the VAE encoder run on the HIP
kernels when the v_express_amd classes are passed (prologue.py, vae.AutoencoderKL); wav2vec2 stays a user-provided
transformers module.  The benchmark and the loop parity tests pass the prologue outputs in directly
(`reference_latents=`, `kps_features=`, `audio_embeddings=`, `latents=` keyword arguments).
"""
from types import SimpleNamespace
from typing import Callable, List, Optional, Union

import math
import numbers
import os

import torch

from . import lib as L
from . import ops
from .context import blend_weights, check_blend, get_context_scheduler, overlap_plan, weighted_overlap_plan
from .distributed import (DistContext, MixedUnitSchedule, UnitSchedule, choose_frame_shards, choose_mixed_shards,
                          split_frames)
from .mutual_self_attention import ReferenceAttentionControl
from .sampling import GUIDANCE_ROWS, REUSE_MODES, Guidance, Known, Sampler, Stitch, UnitCall, check_known
from .scheduler import _Scheduler


def _in_unet_element_type(fn):
    """Pipeline entry points launch kernels themselves (gather / combine / DDIM, layout changes): they run under the
    denoising UNet's 16-bit element type (lib.element_type: bfloat16, or IEEE half for a float16 model)."""
    import functools

    @functools.wraps(fn)
    def run(self, *args, **kwargs):
        with L.element_type(_pipeline_element(self)):
            return fn(self, *args, **kwargs)
    return run


def _pipeline_element(pipe):
    """The denoising UNet's element type; a partial pipeline (the prologue helpers are callable on any object that
    carries the components they use) falls back to the first component that has one, then to the type in force."""
    for name in ("denoising_unet", "reference_net", "vae", "audio_projection", "audio_encoder", "v_kps_guider"):
        elem = getattr(getattr(pipe, name, None), "_elem", None)
        if elem is not None:
            return elem
    return L.ELEM[0]


def guided_steps(n, guidance_start=0.0, guidance_end=1.0):
    """Which of n timesteps run with classifier-free guidance: step i iff i / n >= start and (i + 1) / n <= end
    (diffusers' control_guidance_start / _end rule, in Python floats)."""
    return [i / n >= guidance_start and (i + 1) / n <= guidance_end for i in range(n)]


def check_guidance(guidance_rescale, guidance_start, guidance_end, n):
    """Validates the guidance controls; returns (phi as float, guided_steps(n, start, end))."""
    phi, start, end = float(guidance_rescale), float(guidance_start), float(guidance_end)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"guidance_rescale must lie in [0, 1], got {guidance_rescale}")
    if not (0.0 <= start <= 1.0 and 0.0 <= end <= 1.0):
        raise ValueError(f"guidance_start / guidance_end must lie in [0, 1], got {guidance_start} / {guidance_end}")
    if start > end:
        raise ValueError(f"guidance_start ({guidance_start}) must not exceed guidance_end ({guidance_end})")
    return phi, guided_steps(n, start, end)


def check_apg(apg, guidance_rescale=0.0):
    """Validates the adaptive-projected-guidance controls `apg` = None (off) or (eta, norm_threshold, momentum); returns
    None or the three as floats."""
    if apg is None or apg[0] is None:
        return None
    eta, r, beta = (float(v) for v in apg)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"apg_eta must lie in [0, 1], got {apg[0]}")
    if not (math.isfinite(r) and r >= 0.0):
        raise ValueError(f"apg_norm_threshold must be a finite number >= 0 (0: no cap), got {apg[1]}")
    if not abs(beta) < 1.0:
        raise ValueError(f"apg_momentum must satisfy |apg_momentum| < 1, got {apg[2]}")
    if float(guidance_rescale) > 0.0:
        raise ValueError("apg_eta together with guidance_rescale > 0: both fight the same defect (the over-driven guided "
                         "prediction), and the combination is not built; pass one of them")
    return eta, r, beta


def check_reuse(guidance_refresh, guidance_reuse, guidance_rescale=0.0, apg=None):
    """Validates the guidance-reuse controls; returns None for the period 1 (every guided step runs its rows, as without
    the keywords) or (period, mode)."""
    k = guidance_refresh
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or k < 1:
        raise ValueError(f"guidance_refresh must be an integer >= 1, got {guidance_refresh!r}")
    if guidance_reuse not in REUSE_MODES:
        raise ValueError(f"guidance_reuse must be one of {REUSE_MODES}, got {guidance_reuse!r}")
    if k == 1:
        return None
    if float(guidance_rescale) > 0.0:
        raise ValueError("guidance_refresh > 1 together with guidance_rescale > 0: the rescale needs the row statistics of "
                         "a full step, which a reuse step does not run, and the combination is not built; pass one of them")
    if apg is not None and apg[0] is not None:
        raise ValueError("guidance_refresh > 1 together with apg_eta: the projection needs the row statistics of a full "
                         "step, which a reuse step does not run, and the combination is not built; pass one of them")
    return int(k), guidance_reuse


def check_audio_guidance(audio_guidance_scale):
    """Validates `audio_guidance_scale`; returns it as a float, or None."""
    if audio_guidance_scale is None:
        return None
    s_a = float(audio_guidance_scale)
    if not (math.isfinite(s_a) and s_a >= 0.0):
        raise ValueError(f"audio_guidance_scale must be a finite number >= 0, got {audio_guidance_scale}")
    return s_a


def guidance_rows(guidance_scale, audio_guidance_scale=None):
    """The rows a guided step runs per window for the scales s = guidance_scale and s_a = audio_guidance_scale, whose
    guided prediction is u + s (m - u) + s_a (c - m):
      s_a None or == s  -> ("u", "c") for s > 1, else ("c",): the formula is u + s (c - u), the one-scale route;
      s > 1, s_a != s   -> ("u", "m", "c");
      s <= 1, s_a > 1   -> ("m", "c"): m + s_a (c - m), audio guidance at the cost of one-scale CFG;
      s <= 1, s_a <= 1  -> ("c",): no guidance."""
    s_a = check_audio_guidance(audio_guidance_scale)
    if s_a is None or s_a == guidance_scale:
        return ("u", "c") if guidance_scale > 1.0 else ("c",)
    if guidance_scale > 1.0:
        return ("u", "m", "c")
    return ("m", "c") if s_a > 1.0 else ("c",)


def check_init(init_video, init_latents, mask, video_length, height, width, scale, channels=4):
    """Validates the init-video arguments of __call__ against the clip's geometry (ValueError); returns the mask at pixel
    resolution as float32 [F or 1, H, W] on its own device, or None."""
    if init_video is not None and init_latents is not None:
        raise ValueError("init_video and init_latents are two forms of one input: pass one of them")
    if mask is not None and init_video is None and init_latents is None:
        raise ValueError("mask says which part of an init clip to keep: pass init_video or init_latents with it")
    F, H, W = int(video_length), int(height), int(width)
    if init_video is not None:
        if not isinstance(init_video, torch.Tensor) or tuple(init_video.shape) != (1, 3, F, H, W):
            raise ValueError(f"init_video must be a [1, 3, {F}, {H}, {W}] tensor (video_length, height, width), got "
                             f"{tuple(getattr(init_video, 'shape', ()))}")
        lo, hi = float(init_video.min()), float(init_video.max())
        if not (lo >= 0.0 and hi <= 1.0):
            raise ValueError(f"init_video values must lie in [0, 1], got [{lo}, {hi}]")
    if init_latents is not None:
        want = (1, channels, F, H // scale, W // scale)
        if not isinstance(init_latents, torch.Tensor) or tuple(init_latents.shape) != want:
            raise ValueError(f"init_latents must be a {list(want)} tensor (video_length, height / {scale}, width / "
                             f"{scale}), got {tuple(getattr(init_latents, 'shape', ()))}")
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dim() not in (3, 4) or (mask.dim() == 4 and mask.shape[1] != 1):
        raise ValueError(f"mask must be [F or 1, 1, H, W] or [F or 1, H, W], got {tuple(getattr(mask, 'shape', ()))}")
    m = mask[:, 0] if mask.dim() == 4 else mask
    if m.shape[0] not in (1, F) or tuple(m.shape[1:]) != (H, W):
        raise ValueError(f"mask must have {F} frames or 1, of {H} x {W} pixels (video_length, height, width), got "
                         f"{tuple(mask.shape)}")
    if not (m.dtype == torch.bool or m.is_floating_point()):
        raise ValueError(f"mask must be a float or bool tensor, got {m.dtype}")
    m = m.to(torch.float32)
    lo, hi = float(m.min()), float(m.max())
    if not (lo >= 0.0 and hi <= 1.0):
        raise ValueError(f"mask values must lie in [0, 1], got [{lo}, {hi}]")
    return m


def check_hires(hires_size, hires_steps, hires_strength, hires_mode, num_inference_steps, scale, init_given=False,
                features=(None, None), hires_features=(None, None), hires_noise=None, video_length=None, channels=4):
    """Validates the two-pass (hi-res) arguments of __call__ (ValueError); returns None without `hires_size`, else
    dict(size=(width2, height2), steps, begin_index, mode).  `scale`: the VAE's; `features` / `hires_features`: the
    caller's (reference_latents, kps_features) of the two sizes."""
    names = ("hires_reference_latents", "hires_kps_features")
    if hires_size is None:
        for name, v in zip(names + ("hires_noise",), tuple(hires_features) + (hires_noise,)):
            if v is not None:
                raise ValueError(f"{name} belongs to the second pass of hi-res sampling: pass hires_size with it")
        return None
    try:
        width2, height2 = hires_size
        ok = all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in (width2, height2))
    except (TypeError, ValueError):
        ok = False
    # the UNet's own rule for width / height: three 2x resampling stages under the VAE's factor
    if not ok or min(width2, height2) < 1 or width2 % (8 * scale) or height2 % (8 * scale):
        raise ValueError(f"hires_size must be (width2, height2), positive multiples of {8 * scale} as width and height "
                         f"are, got {hires_size!r}")
    if init_given:
        raise ValueError("hires_size together with init_video / init_latents / mask: the second pass starts from the "
                         "first one's clip, the first from noise; pass one of them")
    if hires_mode not in ops.RESIZE_MODES:
        raise ValueError(f"hires_mode must be one of {ops.RESIZE_MODES}, got {hires_mode!r}")
    steps = num_inference_steps if hires_steps is None else hires_steps
    if isinstance(steps, bool) or not isinstance(steps, numbers.Integral) or steps < 1:
        raise ValueError(f"hires_steps must be a positive integer, got {hires_steps!r}")
    if not isinstance(hires_strength, numbers.Real) or not 0.0 < float(hires_strength) <= 1.0:
        raise ValueError(f"hires_strength must lie in (0, 1], got {hires_strength!r}")
    run = int(steps * hires_strength)
    if run == 0:
        raise ValueError(f"hires_steps = {steps} at hires_strength = {hires_strength} leaves the second pass no step to "
                         f"run (int(hires_steps * hires_strength) == 0)")
    for name, first, second in zip(names, features, hires_features):
        if first is not None and second is None:
            raise ValueError(f"{name[6:]} was given for the first size: the second pass needs {name} at "
                             f"{width2} x {height2} (or pass images for both)")
    if hires_noise is not None:
        want = (1, channels, int(video_length), height2 // scale, width2 // scale)
        if not isinstance(hires_noise, torch.Tensor) or tuple(hires_noise.shape) != want:
            raise ValueError(f"hires_noise must be a {list(want)} tensor, got {tuple(getattr(hires_noise, 'shape', ()))}")
    return dict(size=(int(width2), int(height2)), steps=int(steps), begin_index=int(steps) - run, mode=hires_mode)


def latent_mask(pixel_mask, video_length, scale):
    """The latent mask of a pixel mask (float32 [F or 1, H, W]): the scale x scale box mean, one row per frame,
    float32 [F, (H / scale) * (W / scale)].  A hard pixel edge inside a latent cell becomes a soft latent edge."""
    m = torch.nn.functional.avg_pool2d(pixel_mask[:, None].cpu(), scale)[:, 0]
    return m.expand(video_length, -1, -1).reshape(video_length, -1).contiguous()


class VExpressPipeline:
    def __init__(self, vae, reference_net, denoising_unet, v_kps_guider=None, audio_processor=None,
                 audio_encoder=None, audio_projection=None, scheduler=None, image_proj_model=None, tokenizer=None,
                 text_encoder=None):
        self.vae = vae
        self.reference_net = reference_net
        self.denoising_unet = denoising_unet
        self.v_kps_guider = v_kps_guider
        self.audio_processor = audio_processor
        self.audio_encoder = audio_encoder
        self.audio_projection = audio_projection
        self.scheduler = scheduler
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1)
        self.dist = DistContext.from_env()
        # ranks per (window, CFG-half) unit, each holding 1/S of the window's frames; None = automatic (S > 1 only
        # when the clip has fewer units than ranks, distributed.choose_frame_shards)
        self.frame_shards = None
        # uneven clips (units % world != 0): frame-shard only the left-over units so that every rank carries the same
        # load (distributed.MixedUnitSchedule); None = automatic, 1 = never (whole units only, round-2 behaviour).  An
        # explicit frame_shards = 1 ("no frame sharding") also means whole units only unless mixed_shards is set as well.
        self.mixed_shards = None
        # the schedule the last denoise() call chose (for logs / bench.py): dict(kind, frame_shards, mixed_shards, ...)
        self.last_schedule = {}
        # the guidance controls of the last denoise() call: dict(guided_steps, steps, rescale, unguided_schedule), the
        # last one the last_schedule-style dict of the conditional-only plan of its unguided steps, or None.  A call that
        # passes audio_guidance_scale also finds `rows` (guidance_rows: ("u", "c"), ("u", "m", "c"), ("m", "c") or
        # ("c",)) and `audio_scale` in it; without the keyword the dict is what it was before the keyword existed.  A call
        # that passes apg (apg_eta) finds `apg` = dict(eta, norm_threshold, momentum), or None where it was ignored.  A
        # call with guidance_refresh > 1 finds `refresh` (the period), `reuse` ("hold" or "linear") and `refresh_steps`
        # (the indices of the guided steps that ran all their rows; empty where the keywords were ignored)
        self.last_guidance = {}
        # init-video sampling of the last denoise() call: dict(begin_index, masked, blend_launches) - the step index the
        # loop started at, whether a latent mask was blended in after every step, and the vx_known_blend launches of the
        # call (the one that forms the start latents included; 0 without an init clip)
        self.last_init = {}
        # the window stitch of the last denoise() call: dict(schedule, blend, windows, max_terms, blend_launches) - the
        # context_schedule name (None when denoise was called directly: it takes the windows themselves), the blend
        # ("mean", "linear", "pyramid" or "profile"), the number of windows, the most predictions summed into one frame
        # and the vx_overlap_blend launches of the call (one per timestep of a weighted blend; 0 on the mean route)
        self.last_overlap = {}
        # two-pass (hi-res) sampling of the last __call__: None without hires_size, else dict(base = (width, height),
        # size = (width2, height2), mode, steps, begin_index (of the second pass), base_latents (the first pass's result,
        # on the device), events (six HIP events, None off the GPU: hires_timings_ms reads them))
        self.last_hires = None
        # batch rows per UNet call: 2 = the two CFG halves of one window; 4 (default), 6, ... also merge consecutive
        # windows of this rank into one call.  Every kernel is batch-invariant, so the rows come out bit-identical;
        # merged calls measure 4-5 % faster (profiles/r02e_host_overhead.json: b = 3 74.0 ms vs 49.2 + 28.2 ms,
        # b = 4 94.1 vs 2 x 49.2 ms at 512x512, f = 16), which is what the 3-unit ranks of the 8-GPU config-4 run and
        # the multi-window single-GPU clips execute
        self.units_per_call = int(os.environ.get("VX_UNITS_PER_CALL", "4"))
        self.last_timing = {}

    # ------------------------------------------------------------------ plumbing
    @property
    def device(self):
        return self.denoising_unet.device

    @property
    def dtype(self):
        return self.denoising_unet.dtype

    def to(self, *args, **kwargs):
        for m in (self.vae, self.reference_net, self.denoising_unet):
            m.to(*args, **kwargs)
        return self

    # ------------------------------------------------------------------ once-per-clip prologue (reference hooks)
    @staticmethod
    def _preprocess_image(image, height, width, normalize):
        """diffusers VaeImageProcessor.preprocess as configured at pipelines/v_express_pipeline.py:112-119
        (do_convert_rgb, resize with LANCZOS, [0,1]; `normalize`: 2x-1 for the reference image only)."""
        import numpy as np
        from PIL import Image
        if isinstance(image, torch.Tensor):
            t = image if image.ndim == 4 else image[None]
        else:
            arr = np.asarray(image.convert("RGB").resize((width, height), resample=Image.LANCZOS), dtype=np.float32)
            t = torch.from_numpy(arr / 255.0).permute(2, 0, 1)[None]
        return 2.0 * t - 1.0 if normalize else t

    @_in_unet_element_type
    def prepare_reference_latent(self, reference_image, height, width):
        """pipelines/v_express_pipeline.py:343-348: VAE-encode the reference image (posterior mean) * 0.18215.  Runs on
        the HIP VAE encoder when `vae` is a v_express_amd.AutoencoderKL (encoder weights loaded)."""
        if not hasattr(self.vae, "encode"):
            raise NotImplementedError("this VAE has no encoder half (AutoencoderKLDecoder): construct "
                                      "v_express_amd.AutoencoderKL and load encoder.* / quant_conv.*, or pass "
                                      "reference_latents=[1,4,h/8,w/8] (already scaled by 0.18215)")
        x = self._preprocess_image(reference_image, height, width, normalize=True)
        return self.vae.encode(x).latent_dist.mean * 0.18215

    @_in_unet_element_type
    def prepare_kps_tokens(self, kps_images, height, width, do_classifier_free_guidance):
        """prepare_kps_feature (:350-372) on the device, returning the token layout the loop consumes:
        bf16 `[2, F, hw, C0]` (row 0 = the all-zero unconditional half).  Needs a v_express_amd.VKpsGuider."""
        frames = [self._preprocess_image(img, height, width, normalize=False).unsqueeze(2) for img in kps_images]
        x = torch.cat(frames, dim=2)                                          # [1, 3, F, H, W]
        toks = []
        for i in range(0, x.shape[2], 16):                                    # :359-366 (chunks of 16 frames)
            t, h, w = self.v_kps_guider.forward_tokens(x[:, :, i:i + 16])
            toks.append(t)
        tok = torch.cat(toks, dim=0).view(1, x.shape[2], h * w, -1)
        if do_classifier_free_guidance:
            tok = torch.cat([torch.zeros_like(tok), tok], dim=0)
        return tok

    @_in_unet_element_type
    def prepare_kps_feature(self, kps_images, height, width, do_classifier_free_guidance):
        """pipelines/v_express_pipeline.py:350-372 with the reference's return layout `[2, C, F, h, w]` float32."""
        if self.v_kps_guider is None:
            raise NotImplementedError("no v_kps_guider given; pass kps_features=[2,320,F,h/8,w/8]")
        if hasattr(self.v_kps_guider, "forward_tokens"):
            tok = self.prepare_kps_tokens(kps_images, height, width, do_classifier_free_guidance)
            b2, F_, hw, c = tok.shape
            h = height // self.vae_scale_factor
            return tok.float().view(b2, F_, h, hw // h, c).permute(0, 4, 1, 2, 3).contiguous()
        frames = [self._preprocess_image(img, height, width, normalize=False).unsqueeze(2) for img in kps_images]
        x = torch.cat(frames, dim=2).to(self.device)                          # a user-provided torch module
        feats = [self.v_kps_guider(x[:, :, i:i + 16].to(next(self.v_kps_guider.parameters()).dtype)).float()
                 for i in range(0, x.shape[2], 16)]
        feat = torch.cat(feats, dim=2)
        if do_classifier_free_guidance:
            feat = torch.cat([torch.zeros_like(feat), feat], dim=0)
        return feat

    @_in_unet_element_type
    def prepare_audio_embeddings(self, audio_waveform, video_length, num_pad_audio_frames,
                                 do_classifier_free_guidance):
        """pipelines/v_express_pipeline.py:374-407.  `audio_processor` / `audio_encoder` are v_express_amd's
        WaveformProcessor / Wav2Vec2Model (HIP kernels) or the transformers objects the reference uses - anything with
        the same call signature; the window construction and the AudioProjection run here."""
        if self.audio_encoder is None or self.audio_projection is None or self.audio_processor is None:
            raise NotImplementedError("no audio modules given; pass audio_embeddings=[2,F,5,768]")
        from .prologue import audio_windows
        wav = self.audio_processor(audio_waveform, return_tensors="pt", sampling_rate=16000)["input_values"]
        if getattr(self.audio_encoder, "wants_fp32_input", False):
            enc_dtype = torch.float32            # the HIP encoder reads the raw waveform in float32
        else:
            enc_dtype = next(self.audio_encoder.parameters()).dtype
        emb = self.audio_encoder(wav.to(self.device, enc_dtype)).last_hidden_state
        per_frame = audio_windows(emb, video_length, num_pad_audio_frames).to(enc_dtype)
        out = self.audio_projection(per_frame).unsqueeze(0)
        if do_classifier_free_guidance:
            out = torch.cat([torch.zeros_like(out), out], dim=0)
        return out

    def prepare_latents(self, batch_size, num_channels_latents, width, height, video_length, dtype, device,
                        generator, latents=None):
        """pipelines/v_express_pipeline.py:189-224: N(0,1) drawn on the CPU generator, times init_noise_sigma.
        Drawn in fp32 so the draw does not depend on the compute dtype (SURVEY.md §8c RNG note)."""
        shape = (batch_size, num_channels_latents, video_length, height // self.vae_scale_factor,
                 width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(
                f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        return self._initial_noise(shape, device, generator, latents) * self.scheduler.init_noise_sigma

    @staticmethod
    def _initial_noise(shape, device, generator, latents=None):
        """The N(0,1) draw of prepare_latents (or the caller's `latents`) before init_noise_sigma: float32 on `device`."""
        if latents is None:
            latents = torch.randn(shape, generator=generator, device="cpu", dtype=torch.float32)
        return latents.to(device=device, dtype=torch.float32)

    # ------------------------------------------------------------------ the hot loop
    def _sampler(self, eta=0.0):
        """The fused update the loop runs with this scheduler and eta - "ddim", "multistep", "ancestral", "linear" or "unipc", the
        scheduler's own answer (scheduler.loop_steps, here for a run of no steps; the caller asks again with its
        timesteps for the coefficients).  Any scheduler that is not one of the project's raises TypeError before anything
        runs: the fused updates are the only ones the loop has.  eta is honoured by DDIM only: the others raise
        NotImplementedError."""
        if not isinstance(self.scheduler, _Scheduler):
            raise TypeError(f"the denoising loop drives v_express_amd.DDIMScheduler or "
                            f"v_express_amd.DPMSolverMultistepScheduler or v_express_amd.UniPCMultistepScheduler or "
                            f"v_express_amd.EulerAncestralDiscreteScheduler or "
                            f"v_express_amd.EulerDiscreteScheduler, LMSDiscreteScheduler or PNDMScheduler, "
                            f"not {type(self.scheduler).__name__}")
        return self.scheduler.loop_steps((), 0, eta)[0]

    def _unit_plan(self, latents, kps_tokens, audio, audio_is_zero, windows, win_ids, half_rows):
        """The static plan of one kind of timestep: which (window, half) units this rank computes, in which UNet calls,
        and where they land in the exchange buffer.  `half_rows`: the row of the kps / audio tensors and of the reference
        banks that each half of the plan uses - [0, 1] under classifier-free guidance, [0] without, [1] for the
        conditional half alone of a CFG clip (an unguided step).  An entry may also name the three separately, as
        (bank row, keypoint row, audio row): GUIDANCE_ROWS["m"] = (1, 1, 0) is the silent row of three-row guidance (an
        int r stands for (r, r, r)).  Collective (`dc.frame_shard`): every rank builds it.
        Returns dict(calls, local, uidx, max_slots, schedule), calls a list of sampling.UnitCall."""
        unet, dc, dev = self.denoising_unet, self.dist, latents.device
        _, C, F, H, W = latents.shape
        hw = H * W
        f = len(windows[0])
        nW = len(windows)
        halves_n = len(half_rows)
        row_of = [r if isinstance(r, tuple) else (r, r, r) for r in half_rows]      # (bank, kps, audio) of each half
        win_ids_long = win_ids.long()
        min_hw = (H // 8) * (W // 8)
        S = self.frame_shards or choose_frame_shards(nW, dc.world_size, f, min_hw, halves_n)
        if S < 1 or dc.world_size % S or f % S or min_hw % S:
            raise ValueError(f"frame_shards={S} must divide the world size ({dc.world_size}), the window length ({f}) "
                             f"and the {H // 8}x{W // 8} tokens of the coarsest UNet level")
        # Three schedules, one exchange format.  G = frame granules per unit in the exchange buffer:
        #   uniform, S = 1: every unit whole on one rank (G = 1);  uniform, S > 1: every unit on S ranks (G = S);
        #   mixed: floor(units / world) whole units per rank + the left-over units sharded Sm ways (G = Sm): every rank
        #   then carries the same load (the 20 units of the config-4 clip on 8 GPUs: 2 + 1/2 per rank instead of 3 | 2).
        Sm = 1
        whole_units_only = self.mixed_shards == 1 or (self.frame_shards == 1 and self.mixed_shards is None)
        if S == 1 and dc.enabled and not whole_units_only:
            Sm = self.mixed_shards or choose_mixed_shards(nW * halves_n, dc.world_size, f, min_hw)
        schedule = dict(kind="mixed" if Sm > 1 else ("frame-sharded" if S > 1 else "whole units"),
                        frame_shards=S, mixed_shards=Sm, units=nW * halves_n, world=dc.world_size)
        if Sm > 1:
            sched_m = MixedUnitSchedule(nW, dc.world_size, Sm, halves_n)
            G, max_slots, unit_slots = Sm, sched_m.max_slots, sched_m.slots
            # (call groups, frame shards of these calls): this rank's whole units, then its share of one sharded unit
            su = sched_m.split_unit(dc.rank)
            plan_calls = [(sched_m.whole_calls(dc.rank), 1), ([(su[0], [su[1]])], Sm)]
        else:
            sched_u = UnitSchedule(nW, dc.world_size, S, halves_n)
            G, max_slots = S, sched_u.max_units
            unit_slots = {}
            for u in sched_u.slot:
                ranks, slot = sched_u.unit_ranks(u)
                unit_slots[u] = [(r, slot) for r in ranks]
            plan_calls = [(sched_u.calls(dc.rank), S)]
        g_frames = f // G                              # frames per exchange granule
        # per-timestep exchange: only conv_out's C real channels travel (the GEMM pads them to 8); unit_index tells the
        # combine kernel which gathered slot holds frame granule j of (window, CFG half)
        local = torch.zeros((max_slots, g_frames * hw, C), device=dev, dtype=torch.float32)
        uidx = torch.empty((nW, halves_n, G), dtype=torch.int32)
        for wi in range(nW):
            for hlf in range(halves_n):
                for j, (r, slot) in enumerate(unit_slots[(wi, hlf)]):
                    uidx[wi, hlf, j] = r * max_slots + slot
        uidx = uidx.to(dev)
        # per-call constants (window ids, conditioning slices) do not depend on the timestep: build them once so
        # the timestep loop issues kernels only (no host->device copies, no syncs)
        # UNet calls of this rank: the units of one window always share a call; `units_per_call` > 2 also merges
        # consecutive windows into one batch (every kernel is batch-invariant, so the rows come out identical - only
        # the launches get fatter, which helps the 16x16 / 8x8 levels of multi-window clips)
        limit = int(self.units_per_call)
        calls = []
        for my_calls, Sc in plan_calls:
            shard = dc.frame_shard(Sc)                 # collective when it creates the groups: every rank gets here
            f_loc = f // Sc
            lo = (dc.rank % Sc) * f_loc                # this rank's frames of the windows of these calls: [lo, lo+f_loc)
            merged, cur = [], []
            for wi, halves in my_calls:
                if cur and (limit <= 2 or sum(len(h) for _, h in cur) + len(halves) > limit):
                    merged.append(cur)
                    cur = []
                cur.append((wi, halves))
            if cur:
                merged.append(cur)
            for group in merged:
                rows = [(wi, hlf) for wi, halves in group for hlf in halves]      # batch rows of the call, in order
                kps_l, ehs_l = [], []
                for wi, halves in group:
                    ksel = torch.tensor([row_of[hlf][1] for hlf in halves], device=dev)
                    asel = torch.tensor([row_of[hlf][2] for hlf in halves], device=dev)
                    ids_long = win_ids_long[wi][lo:lo + f_loc]
                    kps_l.append(kps_tokens.index_select(0, ksel).index_select(1, ids_long)
                                 .reshape(len(halves) * f_loc, hw, -1))
                    e = audio.index_select(0, asel).index_select(1, ids_long)
                    ehs_l.append(e.reshape(-1, e.shape[-1]))
                kps = torch.cat(kps_l, dim=0).contiguous()
                ehs = torch.cat(ehs_l, dim=0).contiguous()
                gathers = [(win_ids[wi][lo:lo + f_loc].contiguous(), len(halves)) for wi, halves in group]
                # send slots of the call: its units occupy consecutive slots in row order (a whole unit of a mixed
                # schedule = G consecutive granules, a sharded unit this rank's one granule)
                s0 = min(slot for (r, slot) in unit_slots[rows[0]] if r == dc.rank)
                n_slots = len(rows) * (G // Sc)
                # the audio K | V of all 16 transformer blocks is step-invariant: once per clip and call
                bank_rows = [row_of[hlf][0] for _, hlf in rows]
                calls.append(UnitCall(bank_rows, gathers, kps, ehs, unet.precompute_audio_kv(ehs),
                                      [audio_is_zero[row_of[hlf][2]] for _, hlf in rows], f_loc, shard, s0, n_slots))
        return dict(calls=calls, local=local, uidx=uidx, max_slots=max_slots, schedule=schedule)

    @_in_unet_element_type
    def denoise(self, latents, kps_tokens, audio, timesteps, windows, guidance_scale, callback=None,
                callback_steps=1, *, begin_index=None, eta=0.0, noise_seed=None, guidance_rescale=0.0,
                guidance_start=0.0, guidance_end=1.0, known=None, audio_guidance_scale=None, overlap_blend="mean",
                apg=None, guidance_refresh=1, guidance_reuse="hold"):
        """pipelines/v_express_pipeline.py:526-583.  latents fp32 [1,4,F,h,w] (device, updated in place);
        kps_tokens bf16 [b, F, hw, C0]; audio bf16 [b, F, n_ctx, 768] with b = 2 (uncond, cond) under classifier-free
        guidance (guidance_scale > 1, :443) and b = 1 (the conditional row only) without.
        DPM-Solver++ and the ancestral samplers: `timesteps` are the scheduler's from step index `begin_index` on
        (default: its last len(timesteps)); each frame gets exactly one update per timestep, so the multistep history is
        per frame.  Ancestral samplers (DDIM with eta > 0, Euler ancestral) draw the noise of step index i on the device
        from `noise_seed` (64 bits, required), keyed by (step index, frame, channel, pixel) only.  Euler ancestral: the
        latents come and go in the scheduler's (VE) frame; the loop runs in the VP frame x / sqrt(1 + sigma^2).
        Euler, LMS and PNDM run one vx_overlap_linear_step per timestep (Euler and LMS in the VE frame like Euler
        ancestral; LMS keeps eps of the last three steps per frame, PNDM the last model outputs and, for its warm-up
        pair, one saved sample).  PNDM's timestep list has one entry more than num_inference_steps - the second timestep
        twice - and every entry is one timestep of the loop (the guidance interval counts them); it cannot start inside
        the schedule: begin_index != 0 or `known` raise NotImplementedError.
        UniPC runs one vx_overlap_unipc_step per timestep: the corrector of the step that ended at the sample the UNet just
        saw, then the predictor from the corrected sample; it keeps the data predictions of the last three steps per frame
        and the corrected sample, and starts a run (begin_index) at first order without a corrector.
        Guidance controls (classifier-free guidance only; every sampler): step i of the N timesteps is guided iff
        i / N >= guidance_start and (i + 1) / N <= guidance_end, any other step computes the conditional rows only and
        takes them as the prediction; guidance_rescale = phi > 0 scales each window's guided prediction g by
        1 + phi (std(cond) / std(g) - 1) before the overlap sum (diffusers' rescale_noise_cfg, vx_guidance_rescale).
        A separate audio scale: audio_guidance_scale = s_a (None = guidance_scale) guides on the audio apart from the
        reference image and the keypoints, g = u + s (m - u) + s_a (c - m) with m the row that keeps bank and keypoints
        and drops the audio; the rows a guided step runs are guidance_rows(s, s_a) - three per window for s > 1 and
        s_a != s (vx_combine_units3 / vx_guidance_rescale3), (m, c) with guidance s_a for s <= 1 < s_a; both need the
        b = 2 conditioning.  The rescale is towards std(c); an unguided step runs c alone, and neither scale applies.
        Adaptive projected guidance: apg = (eta, norm_threshold, momentum) (None: off) replaces the combine of a guided
        step by vx_guidance_apg - per window and per frame, each guidance difference (c - u; m - u and c - m with three
        rows; c - m for the rows (m, c)) runs through a momentum buffer the loop owns (zeros before the first guided
        step), is capped at the norm norm_threshold (0: no cap) and has its part parallel to the conditional prediction
        scaled by eta (Sadat et al., diffusers' AdaptiveProjectedGuidance, on the model output).  Not together with
        guidance_rescale; an unguided step neither reads nor advances the buffers; ignored without guidance.
        Guidance reuse: guidance_refresh = k > 1 runs all rows of a guided step only on the refresh steps - the first
        and the last guided step and every k-th between (sampling.refresh_roles) - where vx_combine_units_keep forms the
        prediction of the plain combine, bit for bit, and stores the differences of consecutive rows; the guided steps
        between run the conditional row alone, on the unit plan of an unguided step, and vx_combine_reused adds the stored
        differences: c + sum (s_k - 1) L_k with guidance_reuse = "hold", and with "linear" the differences of the last two
        refreshes extrapolated in the step index (hold until there are two).  Everything after the prediction is
        unchanged.  Not together with guidance_rescale or apg; ignored without guidance; k = 1 is the loop without it.
        Init-video sampling (every sampler): known = (init, noise, m) - the clip's clean latents and the N(0,1) tensor,
        fp32 shaped like `latents`, and the latent mask fp32 [F, h*w] in [0, 1] (1 = regenerate, 0 = keep) or None.  The
        loop then starts from a_b init + s_b noise, b = begin_index (what `latents` held is not read), with (a_j, s_j)
        the scheduler's noise_coefficients(j); with a mask, after the update of step index i the kept part is put back
        at the level the latents now have, x = m x + (1 - m)(a_{i+1} init + s_{i+1} noise), and after the last of
        `timesteps` it is init itself, (a, s) = (1, 0), as in diffusers' inpaint loop (vx_known_blend; the same noise
        at every step; the multistep history and the ancestral noise are left alone; a callback sees the blended
        latents).  m = None is plain img2img: no launch after the start.
        A weighted window blend (every sampler): overlap_blend = "linear", "pyramid" or a sequence of f positive weights
        (context.blend_weights) replaces the 1 / count of the mean ("mean" or None: the reference's, :552-572) by
        per-window, per-position weights normalised per frame.  One vx_overlap_blend launch per timestep, after the
        combine / rescale launch (the rescale still acts per window), forms every frame's prediction; the sampler's
        update then runs on that buffer with the trivial plan (one term, count 1), so x0 history, noise stream and the
        known-region blend are what they are on the mean route.  The windows must not hold a frame twice ("linear":
        contiguous runs by increasing start), which context_schedule="uniform_fit" gives for any clip length."""
        update = self._sampler(eta)
        blend_kind = check_blend(overlap_blend, len(windows[0]))
        raw_weights = None if blend_kind == "mean" else blend_weights(windows, overlap_blend)
        guidance_rescale, guided = check_guidance(guidance_rescale, guidance_start, guidance_end, len(timesteps))
        row_names = guidance_rows(guidance_scale, audio_guidance_scale)
        apg = check_apg(apg, guidance_rescale)
        reuse = check_reuse(guidance_refresh, guidance_reuse, guidance_rescale, apg)
        init, noise, kmask = check_known(known, latents)
        if update != "ddim" or known is not None:
            all_ts = [int(t) for t in self.scheduler.timesteps.tolist()]
            if begin_index is None:
                begin_index = len(all_ts) - len(timesteps)
            if [int(t) for t in timesteps] != all_ts[begin_index:begin_index + len(timesteps)]:
                raise ValueError(f"{type(self.scheduler).__name__}: timesteps must be the scheduler's own, from step "
                                 f"index begin_index on")
        if update == "ancestral" and noise_seed is None:
            raise ValueError(f"{type(self.scheduler).__name__}: an ancestral sampler draws noise on the device: pass "
                             f"noise_seed")
        _, coefs = self.scheduler.loop_steps(timesteps, begin_index, eta, init=known is not None)
        unet, dc, dev = self.denoising_unet, self.dist, latents.device
        _, C, F, H, W = latents.shape
        hw = H * W
        f = len(windows[0])
        if any(len(w) != f for w in windows):
            raise ValueError("all context windows must have the same length")
        nW = len(windows)
        win_ids = torch.tensor(windows, dtype=torch.int32, device=dev)
        # the four parts (sampling.py), each resolved here: host coefficients, plans and buffers.  Everything that can
        # fail has failed before the first kernel
        plan = overlap_plan(windows, F) if raw_weights is None else weighted_overlap_plan(windows, F, raw_weights)
        stitch = Stitch(plan, raw_weights is not None, blend_kind, nW, C, F, hw, len(timesteps), dev)
        self.last_overlap = stitch.report
        guidance = Guidance(row_names, guidance_scale, audio_guidance_scale, guidance_rescale, guided, kps_tokens, audio,
                            lambda audio_is_zero, half_rows: self._unit_plan(latents, kps_tokens, audio, audio_is_zero,
                                                                             windows, win_ids, half_rows),
                            nW, C, f, hw, dev, apg=apg, reuse=reuse)
        self.last_schedule, self.last_guidance = guidance.schedule, guidance.report
        preds = torch.empty((nW, C, f, hw), device=dev, dtype=torch.float32)
        sampler = Sampler(self.scheduler, update, coefs, latents, begin_index, noise_seed)
        known = Known(self.scheduler, init, noise, kmask, len(timesteps), begin_index)
        self.last_init = known.report
        if known.active:
            known.start(latents)                      # (already in the frame the loop runs in)
        else:
            sampler.start(latents)
        for i, t in enumerate(timesteps):
            t = int(t)
            step_plan = guidance.plan(i)
            local, max_slots, uidx = step_plan["local"], step_plan["max_slots"], step_plan["uidx"]
            for call in step_plan["calls"]:
                parts = [ops.gather_latents(latents, ids, reps=reps) for ids, reps in call.gathers]
                x_in = parts[0] if len(parts) == 1 else torch.cat(parts, dim=0)
                out = unet.forward_tokens(x_in, t, call.ehs, call.kps, b=len(call.bank_rows), f=call.f_loc, H=H, W=W,
                                          batch_rows=call.bank_rows, audio_kv=call.audio_kv,
                                          audio_zero=call.audio_zero, frame_shard=call.shard)
                # a call's units occupy consecutive send slots, in row order: one strided pack per call
                ops.pack_rows(out, C, local[call.s0:call.s0 + call.n_slots])
            gathered = dc.all_gather_units(local, max_slots)          # [world, max_slots, (f/G)*hw, C]
            guidance.combine(i, gathered, uidx, preds)
            sampler.update(i, t, latents, stitch.reduce(preds), stitch)
            known.after(i, latents)
            if callback is not None and i % callback_steps == 0:
                callback(i, t, sampler.callback_view(i, latents))
        sampler.finish(latents)
        return latents

    @torch.no_grad()
    @_in_unet_element_type
    def decode_latents(self, latents, chunk=8, composite=None):
        """pipelines/v_express_pipeline.py:152-166; frames are split evenly over the ranks when distributed.
        composite = (init_video fp32 [1, 3, F, H, W], pixel mask fp32 [F or 1, H * W]), both on the device: the video is
        mask * decoded + (1 - mask) * init_video, formed inside the post-process launch."""
        dc = self.dist
        F = latents.shape[2]
        comp = {} if composite is None else dict(init_video=composite[0], mask=composite[1])
        if not dc.enabled:
            return self.vae.decode_video(latents, chunk=chunk, **comp)
        spans = split_frames(F, dc.world_size)
        lo, hi = spans[dc.rank]
        per = spans[0][1] - spans[0][0]
        if comp:
            comp["frame0"] = lo
        part = self.vae.decode_video(latents[:, :, lo:hi].contiguous(), chunk=chunk, **comp) if hi > lo else None
        Hh, Ww = latents.shape[-2] * self.vae_scale_factor, latents.shape[-1] * self.vae_scale_factor
        buf = torch.zeros((per, 3, Hh, Ww), device=latents.device, dtype=torch.float32)
        if part is not None:
            buf[:hi - lo].copy_(part[0].permute(1, 0, 2, 3))
        allf = dc.all_gather_frames(buf).reshape(-1, 3, Hh, Ww)[:F]
        return allf.permute(1, 0, 2, 3).unsqueeze(0)

    # ------------------------------------------------------------------ reference call surface
    @torch.no_grad()
    @_in_unet_element_type
    def __call__(self, reference_image, kps_images, audio_waveform, width, height, video_length,
                 num_inference_steps, guidance_scale, strength=1., num_images_per_prompt=1, eta: float = 0.0,
                 generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
                 output_type: Optional[str] = "tensor", return_dict: bool = True,
                 callback: Optional[Callable[[int, int, torch.FloatTensor], None]] = None,
                 callback_steps: Optional[int] = 1, context_schedule="uniform", context_frames=24,
                 context_overlap=4, reference_attention_weight=1., audio_attention_weight=1.,
                 num_pad_audio_frames=2, do_multi_devices_inference=False, save_gpu_memory=False,
                 reference_latents=None, kps_features=None, audio_embeddings=None, latents=None,
                 noise_seed: Optional[int] = None, output_device="cpu", decode=True, guidance_rescale: float = 0.0,
                 guidance_start: float = 0.0, guidance_end: float = 1.0, init_video=None, init_latents=None,
                 mask=None, composite=True, audio_guidance_scale: Optional[float] = None, overlap_blend="mean",
                 apg_eta: Optional[float] = None, apg_norm_threshold: float = 0.0, apg_momentum: float = 0.0,
                 guidance_refresh: int = 1, guidance_reuse: str = "hold", hires_size=None,
                 hires_steps: Optional[int] = None, hires_strength: float = 0.5, hires_mode: str = "bilinear",
                 hires_noise=None, hires_reference_latents=None, hires_kps_features=None, **kwargs):
        """Window stitch: `context_schedule` = "uniform" (the reference's; a clip length that is not f + k (f - o) ends in
        a reflected window with duplicate frames) or "uniform_fit" (the same number of windows spread evenly over any
        length); `overlap_blend` = "mean" (default, also None: the reference's 1 / count) or a weighted blend of the
        overlapping predictions - "linear" (a cross-fade over each actual overlap), "pyramid" or a sequence of
        `context_frames` positive weights.  A weighted blend needs windows without duplicate frames: use "uniform_fit".
        A separate audio scale: `audio_guidance_scale` = s_a (default None: the one scale of `guidance_scale` = s)
        guides on the audio apart from the reference image and the keypoints: u + s (m - u) + s_a (c - m), m the
        prediction with bank and keypoints but silent audio (three rows per window for s > 1 and s_a != s; the rows
        (m, c) for s <= 1 < s_a).  The prologue runs in the CFG layout whenever either scale exceeds 1.
        Adaptive projected guidance: `apg_eta` in [0, 1] (default None: off) switches it on for the guided steps - the
        part of each guidance difference parallel to the conditional prediction is scaled by apg_eta (0 removes it, the
        published remedy for the saturation of a large scale), the difference is capped at the norm
        `apg_norm_threshold` per frame (0: no cap) and averaged with `apg_momentum` (|.| < 1, usually negative) over the
        guided steps.  It acts on the model output per window and frame, with every row route and sampler; it cannot be
        combined with `guidance_rescale`, and without guidance it is ignored.
        Guidance reuse (CFG-cache): `guidance_refresh` = k > 1 computes the guidance differences only on every k-th guided
        step (and on the first and the last one); the guided steps between run the conditional row alone - the cost of an
        unguided step - and add the stored differences, held (`guidance_reuse` = "hold", the default) or extrapolated
        linearly from the last two refreshes ("linear").  It cannot be combined with `guidance_rescale` or `apg_eta`;
        without guidance it is ignored; the effect on visual quality with real weights is not measured.
        Init-video sampling (diffusers' img2img / inpaint semantics for a 4-channel UNet): `init_video` fp32
        [1, 3, F, H, W] in [0, 1] (VAE-encoded here; needs v_express_amd.AutoencoderKL) or `init_latents`
        [1, 4, F, h, w] (clean, already scaled) makes the loop start from the clip noised to the level of `strength`
        instead of from pure noise; `mask` ([F or 1, 1, H, W] or [F or 1, H, W], float or bool in [0, 1]; 1 =
        regenerate, 0 = keep) restricts the change to a region (its 8 x 8 box mean is the latent mask), and with
        `init_video` and `composite` the kept pixels of the output are the caller's own, not their VAE round trip.
        `latents` / `generator` give the N(0,1) noise, as without an init clip.
        Two-pass (hi-res) sampling: `hires_size` = (width2, height2) (default None: off) samples the clip at
        (width, height) as without it, resizes the latents on the device (`ops.latent_resize`, `hires_mode` "bilinear" or
        "bicubic"), noises them to the level of `hires_strength` and runs the last int(hires_steps * hires_strength) of
        `hires_steps` timesteps (default: num_inference_steps) at the new size - the init-latents route above, with
        ReferenceNet banks and keypoint tokens built at the new size from the images (or from
        `hires_reference_latents` / `hires_kps_features` when the first pass was given features) and the audio embeddings
        of the first pass.  `hires_noise` is the N(0,1) tensor of the second pass, as `latents` is of the first;
        `generator` is drawn from in the order pass-1 latents, pass-1 ancestral seed, pass-2 noise, pass-2 ancestral
        seed, and an explicit `noise_seed` gives the second pass noise_seed + 1.  The callback's step index runs on
        through both passes.  decode=False returns the second pass's latents; `last_hires` reports the run.  Not
        together with init_video / init_latents / mask; PNDM cannot start inside its schedule (NotImplementedError).
        The effect on visual quality with real weights is not measured."""
        # an unsupported scheduler, eta with one other than DDIM, guidance controls out of range or init-video arguments
        # that do not fit the clip fail here, before the prologue
        ancestral = self._sampler(eta) == "ancestral"
        check_guidance(guidance_rescale, guidance_start, guidance_end, max(int(num_inference_steps), 1))
        audio_guidance_scale = check_audio_guidance(audio_guidance_scale)
        apg = check_apg((apg_eta, apg_norm_threshold, apg_momentum), guidance_rescale)
        check_reuse(guidance_refresh, guidance_reuse, guidance_rescale, apg)
        hires = check_hires(hires_size, hires_steps, hires_strength, hires_mode, num_inference_steps,
                            self.vae_scale_factor, not (init_video is None and init_latents is None and mask is None),
                            (reference_latents, kps_features), (hires_reference_latents, hires_kps_features),
                            hires_noise, video_length, self.denoising_unet.in_channels)

        def clip_windows():
            return list(get_context_scheduler(context_schedule)(
                step=0, num_frames=video_length, context_size=context_frames, context_stride=1,
                context_overlap=context_overlap, closed_loop=False))
        windows = None
        if check_blend(overlap_blend, int(context_frames)) != "mean":
            # a blend the schedule's windows cannot carry fails here too; the mean's windows come after the prologue, as
            # they always have (an unknown schedule fails there)
            windows = clip_windows()
            if not isinstance(overlap_blend, str):
                overlap_blend = [float(v) for v in overlap_blend][:len(windows[0])]   # (one short window: F < f)
            blend_weights(windows, overlap_blend)
        pixel_mask = check_init(init_video, init_latents, mask, video_length, height, width, self.vae_scale_factor,
                                self.denoising_unet.in_channels)
        if init_video is not None and not hasattr(self.vae, "encode_video"):
            raise NotImplementedError("this VAE has no encoder half (AutoencoderKLDecoder): construct "
                                      "v_express_amd.AutoencoderKL and load encoder.* / quant_conv.*, or pass "
                                      "init_latents=[1,4,F,h/8,w/8] (already scaled by 0.18215)")
        # the arguments both passes of a hi-res call share; `audio_embeddings` and `windows` are filled in by the first
        # pass, where they have always been computed, and found there by the second
        c = SimpleNamespace(
            reference_image=reference_image, kps_images=kps_images, audio_waveform=audio_waveform,
            video_length=video_length, guidance_scale=guidance_scale, eta=eta, generator=generator,
            num_images_per_prompt=num_images_per_prompt, context_schedule=context_schedule, clip_windows=clip_windows,
            windows=windows, reference_attention_weight=reference_attention_weight,
            audio_attention_weight=audio_attention_weight, num_pad_audio_frames=num_pad_audio_frames,
            audio_embeddings=audio_embeddings, ancestral=ancestral, guidance_rescale=guidance_rescale,
            guidance_start=guidance_start, guidance_end=guidance_end, audio_guidance_scale=audio_guidance_scale,
            overlap_blend=overlap_blend, apg=apg, guidance_refresh=guidance_refresh, guidance_reuse=guidance_reuse,
            # the CFG layout of banks and conditioning (row 0 zeros, row 1 real): whenever a guided step combines rows
            do_cfg=len(guidance_rows(guidance_scale, audio_guidance_scale)) > 1)
        dev = self.device
        self.last_hires = None
        if hires is None:
            lat, video_dev, ev, _ = self._sample_pass(c, width, height, num_inference_steps, strength, reference_latents,
                                                      kps_features, latents, init_video, init_latents, pixel_mask,
                                                      noise_seed, callback, callback_steps or 1)
        else:
            # the second pass's start is checked before the first one's prologue (PNDM: NotImplementedError)
            self.scheduler.set_timesteps(hires["steps"])
            self.scheduler.loop_steps(self.scheduler.timesteps[hires["begin_index"]:].tolist(), hires["begin_index"], eta,
                                      init=True)
            width2, height2 = hires["size"]
            base, _, ev1, n1 = self._sample_pass(c, width, height, num_inference_steps, strength, reference_latents,
                                                 kps_features, latents, None, None, None, noise_seed, callback,
                                                 callback_steps or 1)
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if ev1 else None
            if marks:
                marks[0].record()
            resized = ops.latent_resize(base, (height2 // self.vae_scale_factor, width2 // self.vae_scale_factor),
                                        hires["mode"])
            if marks:
                marks[1].record()
            every, cb2 = callback_steps or 1, None
            if callback is not None:
                def cb2(i, t, x):                        # the step index runs on through both passes
                    if (n1 + i) % every == 0:
                        callback(n1 + i, t, x)
            lat, video_dev, ev, _ = self._sample_pass(c, width2, height2, hires["steps"], hires_strength,
                                                      hires_reference_latents, hires_kps_features, hires_noise, None,
                                                      resized, None, None if noise_seed is None else noise_seed + 1,
                                                      cb2, 1)
            self.last_hires = dict(hires, base=(int(width), int(height)), base_latents=base,
                                   events=None if marks is None else (ev1[0], ev1[1], marks[0], marks[1], ev[0], ev[1]))
        if not decode:
            return lat
        comp = None
        if composite and video_dev is not None and pixel_mask is not None:
            # the kept pixels are the caller's own: a VAE round trip must not degrade them
            comp = (video_dev, pixel_mask.reshape(pixel_mask.shape[0], -1).to(dev).contiguous())
        video = self.decode_latents(lat, composite=comp)
        if ev:
            ev[2].record()
        self._events = ev
        if output_device is not None:
            video = video.to(output_device)
        return video

    def _sample_pass(self, c, width, height, num_inference_steps, strength, reference_latents, kps_features, latents,
                     init_video, init_latents, pixel_mask, noise_seed, callback, callback_steps):
        """One sampling pass of __call__ at (width, height): timesteps, ReferenceNet banks, keypoint tokens, the start
        latents and the loop.  `c`: the arguments of the call that do not depend on the size (a namespace; this pass
        fills in `audio_embeddings` and `windows` if they are still missing).  Returns (latents, the init video on the
        device or None, the three timing events or None, the number of timesteps run)."""
        dev = self.device
        do_cfg, video_length, generator, eta = c.do_cfg, c.video_length, c.generator, c.eta
        # timesteps (retrieve_timesteps + get_timesteps, :448-449)
        self.scheduler.set_timesteps(num_inference_steps)
        init_t = min(int(num_inference_steps * strength), num_inference_steps)
        begin_index = max(num_inference_steps - init_t, 0)
        timesteps = self.scheduler.timesteps[begin_index:].tolist()
        # a start the scheduler does not build, coefficients it cannot form (e.g. eta too large: ValueError) fail here
        self.scheduler.loop_steps(timesteps, begin_index, eta, init=init_video is not None or init_latents is not None)
        writer = ReferenceAttentionControl(self.reference_net, do_classifier_free_guidance=do_cfg, mode="write",
                                           batch_size=1, fusion_blocks="full")
        reader = ReferenceAttentionControl(self.denoising_unet, do_classifier_free_guidance=do_cfg, mode="read",
                                           batch_size=1, fusion_blocks="full",
                                           reference_attention_weight=c.reference_attention_weight,
                                           audio_attention_weight=c.audio_attention_weight)
        if reference_latents is None:
            reference_latents = self.prepare_reference_latent(c.reference_image, height, width)
        kps_tokens = None
        if kps_features is None:
            if hasattr(self.v_kps_guider, "forward_tokens"):
                kps_tokens = self.prepare_kps_tokens(c.kps_images, height, width, do_cfg)   # stays in the token layout
            else:
                kps_features = self.prepare_kps_feature(c.kps_images, height, width, do_cfg)
        if c.audio_embeddings is None:
            c.audio_embeddings = self.prepare_audio_embeddings(c.audio_waveform, video_length, c.num_pad_audio_frames,
                                                               do_cfg)
        if c.windows is None:
            c.windows = c.clip_windows()
        # ReferenceNet once per clip (:502-509)
        ehs0 = torch.zeros((1, 1, self.denoising_unet.cfg.cross_attention_dim), dtype=torch.float32, device=dev)
        self.reference_net(reference_latents.to(dev), timestep=0, encoder_hidden_states=ehs0, return_dict=False)
        reader.update(writer, do_cfg, dtype=self.dtype)
        known = video_dev = None
        if init_video is None and init_latents is None:
            lat = self.prepare_latents(c.num_images_per_prompt, self.denoising_unet.in_channels, width, height,
                                       video_length, self.dtype, dev, generator, latents)
            if self.dist.enabled and latents is None:
                # every rank drew from its own CPU generator; the loop needs identical step-start latents on all ranks
                # (each rank's UNet inputs are gathered from them and every rank applies the DDIM update): rank 0's
                # draw wins
                lat = self.dist.broadcast(lat.contiguous(), src=0)
        else:
            # the same draw, kept as N(0,1): the loop forms the start latents from it and reuses it at every blend.
            # Rank 0's noise wins as its latents do; every rank encodes the init video itself (batch-invariant kernels)
            h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
            noise = self._initial_noise((1, self.denoising_unet.in_channels, video_length, h, w), dev, generator,
                                        latents).contiguous()
            if self.dist.enabled and latents is None:
                noise = self.dist.broadcast(noise, src=0)
            if init_video is not None:
                video_dev = init_video.to(device=dev, dtype=torch.float32).contiguous()
                init = self.vae.encode_video(video_dev)
            else:
                init = init_latents.to(device=dev, dtype=torch.float32).contiguous()
            m = None if pixel_mask is None else latent_mask(pixel_mask, video_length, self.vae_scale_factor).to(dev)
            known = (init, noise, m)
            lat = torch.empty_like(noise)
        if c.ancestral and noise_seed is None:
            # the ancestral noise is drawn on the device from one 64-bit seed, taken from the generator AFTER the
            # initial latents (which so stay what they are for a given generator); rank 0's seed wins, like its latents
            g = generator[0] if isinstance(generator, list) else generator
            seed = torch.randint(0, 2 ** 63 - 1, (1,), generator=g)
            if self.dist.enabled:
                seed = self.dist.broadcast(seed.to(lat.device), src=0).cpu()
            noise_seed = int(seed)
        if kps_tokens is None:
            b2, c0, F, h, w = kps_features.shape
            kps_tokens = ops.ncfhw_to_nhwc(kps_features.to(dev), c0).view(b2, F, h * w, c0)
        audio = c.audio_embeddings.to(device=dev, dtype=ops.BF16).contiguous()
        timed = lat.is_cuda          # (host-logic tests run this method on CPU tensors over emulated kernels)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if timed else None
        if timed:
            ev[0].record()
        self.denoise(lat, kps_tokens, audio, timesteps, c.windows, c.guidance_scale, callback, callback_steps,
                     begin_index=begin_index, eta=eta, noise_seed=noise_seed, guidance_rescale=c.guidance_rescale,
                     guidance_start=c.guidance_start, guidance_end=c.guidance_end, known=known,
                     audio_guidance_scale=c.audio_guidance_scale, overlap_blend=c.overlap_blend, apg=c.apg,
                     guidance_refresh=c.guidance_refresh, guidance_reuse=c.guidance_reuse)
        self.last_overlap["schedule"] = c.context_schedule
        if timed:
            ev[1].record()
        reader.clear()
        writer.clear()
        return lat, video_dev, ev, len(timesteps)

    def timings_ms(self):
        """(denoise loop, decode) GPU milliseconds of the last call (a hi-res call: the loop of its second pass)."""
        e = self._events
        e[2].synchronize()
        return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])

    def hires_timings_ms(self):
        """(first pass's loop, latent resize, second pass's loop) GPU milliseconds of the last hi-res call."""
        e = self.last_hires["events"]
        e[5].synchronize()
        return e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3]), e[4].elapsed_time(e[5])
