"""Time one BASELINE configs[1] clip (512x512, F = 16 in one window, CFG 3.5, synthetic weights, the set-up of bench.py)
with a chosen sampler and step count (GPU box):
    python tools/sampler_bench.py --scheduler ddim --steps 25
    python tools/sampler_bench.py --scheduler dpm --steps 15 [--order 2]
    python tools/sampler_bench.py --scheduler euler-a --steps 25
    python tools/sampler_bench.py --scheduler euler|lms|pndm --steps 25 [--lms-order 4]
    python tools/sampler_bench.py --scheduler unipc --steps 10 [--solver-order 2] [--solver-type bh2]
    python tools/sampler_bench.py --scheduler ddim-eta --eta 1.0 --steps 25
    python tools/sampler_bench.py --scheduler ddim --steps 25 --guidance-rescale 0.7 --guidance-end 0.6
    python tools/sampler_bench.py --scheduler ddim --steps 25 --init-video --strength 0.6 --mask lower-half
    python tools/sampler_bench.py --scheduler ddim --steps 25 --audio-guidance-scale 6 [--guidance-scale 1]
    python tools/sampler_bench.py --scheduler ddim --steps 25 --apg-eta 0 --apg-norm-threshold 20 --apg-momentum -0.5
    python tools/sampler_bench.py --scheduler ddim --steps 25 --guidance-refresh 2 [--guidance-reuse linear]
    python tools/sampler_bench.py --scheduler ddim --steps 25 --size 768
    python tools/sampler_bench.py --scheduler ddim --steps 25 --hires-size 768 [--hires-steps 15] [--hires-strength 0.5]
Prints one JSON line: ms per clip (host clock around whole clips, ending in a device synchronise), the denoise and decode
milliseconds of the same clips (HIP events), and the average microseconds of the per-step update launch (HIP events
around each `ops.overlap_ddim_step` / `ops.overlap_multistep_step` / `ops.overlap_ancestral_step` /
`ops.overlap_linear_step` (Euler, LMS, PNDM - whose list has steps + 1 entries) / `ops.overlap_unipc_step` of one further, instrumented clip; for the ancestral samplers also `ddim_update_us`, the DDIM update of the same clip timed the same way,
for comparison).  The guidance controls (--guidance-rescale, --guidance-start, --guidance-end) are passed to the loop; the
line then also carries them, the number of guided steps, `rescale_us` (the `ops.guidance_rescale` launches of a step,
timed the same way; it stands in for the one `vx_combine_units` launch of a step without the rescale, `combine_us`) and
the smallest and largest clip of the timed ones (`clip_ms_min`, `clip_ms_max`: HIP events, denoise + decode).
--init-video starts every clip from a synthetic 16-frame video (VAE-encoded inside the clip: `encode_ms`, part of
`denoise_ms` and of the clip) noised to the level of --strength, which also cuts the timesteps to the last
int(steps * strength); --mask lower-half keeps the upper half of every frame (a `vx_known_blend` launch after every step,
`blend_us`, and the composite post-process at the decode).  `postprocess_us` is the post-process launch of a decoded
chunk (`postprocess`: which of the two ran), timed like the update launch.
--audio-guidance-scale s_a (with --guidance-scale s, default 3.5) runs the rows of a separate audio scale (`rows`: three per
window for s > 1, the rows (m, c) for s <= 1 < s_a); `combine3_us` / `rescale3_us` are then the `ops.combine_units3` /
`ops.guidance_rescale3` launches of a guided step, timed like their two-row siblings.
--apg-eta ETA [--apg-norm-threshold R] [--apg-momentum BETA] switches adaptive projected guidance on (with any of the row
routes above; not with --guidance-rescale): `apg_us` is then the two launches of one `ops.guidance_apg` call, a guided
step's, timed like the update launch, and `apg_combine_us` the plain combine of the same rows (`ops.combine_units` /
`ops.combine_units3` into a scratch buffer, right after every APG call of the same instrumented clip), for comparison.
--guidance-refresh K [--guidance-reuse hold|linear] switches guidance reuse on (K > 1; with any row route, not with
--guidance-rescale or --apg-eta): the line then carries `refresh_steps`, and from one instrumented clip `keep_us` (the
`ops.combine_units_keep` launch of a refresh step), `reused_us` (the `ops.combine_reused` launch of a reuse step) and
`keep_combine_us` (the plain combine of the same rows into a scratch buffer right after every keep launch of that clip:
`ops.combine_units` / `ops.combine_units3`), each timed like the update launch.
--frames F --context-frames f --context-overlap o --context-schedule uniform|uniform_fit choose the clip length and its
windows (defaults: 16 frames in one window of 16, overlap 4, `uniform`); --overlap-blend mean|linear|pyramid the stitch of
overlapping windows - a weighted blend adds one `ops.overlap_blend` launch per step (`overlap_blend_us`, timed like the
update launch, whose own time is then that of the trivial one-term plan).
--size S samples an S x S clip instead of 512 x 512 (a multiple of 64).
--hires-size S2 [--hires-steps N2] [--hires-strength T] [--hires-mode bilinear|bicubic] times two-pass (hi-res) clips: S x S
with --steps, the latents resized to S2 x S2 and the last int(N2 * T) of N2 timesteps there, decoded at S2 x S2.  These
clips run through `VExpressPipeline.__call__` on features (the public route of the feature), so a clip also holds what
the other clips of this tool keep outside the timed region: the ReferenceNet run and the keypoint-token layout of each
pass.  The line carries `pass1_ms`, `resize_us` (the one `vx_latent_resize` launch) and `pass2_ms` (HIP events of
`pipe.hires_timings_ms()`: the two loops and the launch between them), `decode_ms`, and `other_ms`, the rest of the clip.
The loop controls above are passed on; the per-launch columns are not collected in this mode."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scheduler", choices=("ddim", "dpm", "ddim-eta", "euler-a", "euler", "lms", "pndm", "unipc"),
                    default="ddim")
    ap.add_argument("--eta", type=float, default=1.0, help="DDIM eta of --scheduler ddim-eta")
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--order", type=int, choices=(1, 2), default=2, help="DPM-Solver++ solver_order")
    ap.add_argument("--lms-order", type=int, choices=(1, 2, 3, 4), default=4, help="LMSDiscreteScheduler lms_order")
    ap.add_argument("--solver-order", type=int, choices=(1, 2, 3), default=2, help="UniPCMultistepScheduler solver_order")
    ap.add_argument("--solver-type", choices=("bh1", "bh2"), default="bh2", help="UniPCMultistepScheduler solver_type")
    ap.add_argument("--guidance-rescale", type=float, default=0.0, help="phi of the CFG rescale")
    ap.add_argument("--guidance-start", type=float, default=0.0)
    ap.add_argument("--guidance-end", type=float, default=1.0)
    ap.add_argument("--guidance-scale", type=float, default=3.5)
    ap.add_argument("--audio-guidance-scale", type=float, default=None,
                    help="a separate scale for the audio (three rows per window for --guidance-scale > 1)")
    ap.add_argument("--apg-eta", type=float, default=None,
                    help="adaptive projected guidance: the scale of the part parallel to the conditional prediction")
    ap.add_argument("--apg-norm-threshold", type=float, default=0.0, help="cap of a guidance difference's norm per frame")
    ap.add_argument("--apg-momentum", type=float, default=0.0)
    ap.add_argument("--guidance-refresh", type=int, default=1,
                    help="guidance reuse: compute the guidance differences on every K-th guided step only")
    ap.add_argument("--guidance-reuse", choices=("hold", "linear"), default="hold")
    ap.add_argument("--init-video", action="store_true", help="start from a synthetic init video (img2img)")
    ap.add_argument("--strength", type=float, default=1.0, help="run the last int(steps * strength) timesteps")
    ap.add_argument("--mask", choices=("none", "lower-half"), default="none",
                    help="with --init-video: regenerate the lower half of every frame, keep the upper half")
    ap.add_argument("--frames", type=int, default=16, help="clip length")
    ap.add_argument("--context-frames", type=int, default=16)
    ap.add_argument("--context-overlap", type=int, default=4)
    ap.add_argument("--context-schedule", choices=("uniform", "uniform_fit"), default="uniform")
    ap.add_argument("--overlap-blend", choices=("mean", "linear", "pyramid"), default="mean")
    ap.add_argument("--size", type=int, default=512, help="pixel size of the (square) clip, a multiple of 64")
    ap.add_argument("--hires-size", type=int, default=None,
                    help="two-pass sampling: the pixel size of the second pass (through VExpressPipeline.__call__)")
    ap.add_argument("--hires-steps", type=int, default=None, help="timesteps of the second pass's schedule (default: --steps)")
    ap.add_argument("--hires-strength", type=float, default=0.5)
    ap.add_argument("--hires-mode", choices=("bilinear", "bicubic"), default="bilinear")
    ap.add_argument("--clips", type=int, default=5, help="timed clips")
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.steps < 1 or args.clips < 1:
        ap.error("--steps and --clips must be >= 1")
    if args.mask != "none" and not args.init_video:
        ap.error("--mask needs --init-video")
    if not 0.0 <= args.strength <= 1.0:
        ap.error("--strength must lie in [0, 1]")
    if args.size < 64 or args.size % 64 or (args.hires_size is not None and (args.hires_size < 64 or args.hires_size % 64)):
        ap.error("--size and --hires-size must be positive multiples of 64")
    if args.hires_size is not None and (args.init_video or args.strength != 1.0):
        ap.error("--hires-size starts its first pass from noise: no --init-video, no --strength")
    if not torch.cuda.is_available():
        raise SystemExit("sampler_bench.py measures on the GPU: no device visible")
    import v_express_amd as vx
    from v_express_amd import ops, synth
    from v_express_amd.context import get_context_scheduler
    from v_express_amd.pipeline import latent_mask
    dev, elem = torch.device("cuda", 0), torch.bfloat16
    torch.cuda.set_device(dev)
    cfg, vcfg = synth.UNetConfig(), synth.VaeConfig()
    F, h = args.frames, args.size // 8
    unet = vx.UNet3DConditionModel(cfg).to(dev).to(elem)
    refnet = vx.UNet2DConditionModel(cfg).to(dev).to(elem)
    vae = (vx.AutoencoderKL if args.init_video else vx.AutoencoderKLDecoder)(vcfg).to(dev).to(elem)
    unet.load_state_dict(synth.unet3d_state_dict(cfg, seed=42, device=dev, dtype=elem, draw_on_device=True))
    unet.release_raw_weights()
    refnet.load_state_dict(synth.refnet_state_dict(cfg, seed=43, device=dev, dtype=elem, draw_on_device=True))
    refnet.release_raw_weights()
    vae.load_state_dict(synth.vae_decoder_state_dict(vcfg, seed=44, device=dev, dtype=elem, draw_on_device=True))
    if args.init_video:
        vae.load_state_dict(synth.vae_encoder_state_dict(vcfg, seed=47, device=dev, dtype=elem))
        vae._prepared_encoder()
    vae._prepared()
    kw = dict(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", clip_sample=False, steps_offset=1,
              prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")
    eta = args.eta if args.scheduler == "ddim-eta" else 0.0
    if args.scheduler in ("ddim", "ddim-eta"):
        sched = vx.DDIMScheduler(**kw)
        update = "overlap_ddim_step" if args.scheduler == "ddim" else "overlap_ancestral_step"
    elif args.scheduler == "euler-a":
        sched, update = vx.EulerAncestralDiscreteScheduler(**kw), "overlap_ancestral_step"
    elif args.scheduler == "euler":
        sched, update = vx.EulerDiscreteScheduler(**kw), "overlap_linear_step"
    elif args.scheduler == "lms":
        sched, update = vx.LMSDiscreteScheduler(**kw, lms_order=args.lms_order), "overlap_linear_step"
    elif args.scheduler == "pndm":
        sched, update = vx.PNDMScheduler(**kw, skip_prk_steps=True), "overlap_linear_step"
    elif args.scheduler == "unipc":
        sched = vx.UniPCMultistepScheduler(**kw, solver_order=args.solver_order, solver_type=args.solver_type)
        update = "overlap_unipc_step"
    else:
        sched, update = vx.DPMSolverMultistepScheduler(**kw, solver_order=args.order), "overlap_multistep_step"
    pipe = vx.VExpressPipeline(vae=vae, reference_net=refnet, denoising_unet=unet, scheduler=sched)
    inp = synth.synthetic_inputs(cfg, F, h, h, seed=42, device=dev)
    if args.hires_size is not None:
        return hires_bench(args, vx, pipe, cfg, inp, eta)
    writer = vx.ReferenceAttentionControl(refnet, do_classifier_free_guidance=True, mode="write", fusion_blocks="full")
    reader = vx.ReferenceAttentionControl(unet, do_classifier_free_guidance=True, mode="read", fusion_blocks="full",
                                          reference_attention_weight=0.95, audio_attention_weight=3.0)
    refnet(inp["ref_latents"], timestep=0, encoder_hidden_states=torch.zeros(1, 1, 768, device=dev), return_dict=False)
    reader.update(writer, True)
    sched.set_timesteps(args.steps)
    begin = max(args.steps - min(int(args.steps * args.strength), args.steps), 0)
    if args.scheduler == "pndm" and (begin or args.init_video):
        ap.error("--scheduler pndm runs the whole schedule from noise: no --strength < 1, no --init-video")
    timesteps = sched.timesteps[begin:].tolist()
    if not timesteps:
        ap.error("--strength leaves no timestep to run")
    windows = list(get_context_scheduler(args.context_schedule)(
        step=0, num_frames=F, context_size=args.context_frames, context_stride=1, context_overlap=args.context_overlap,
        closed_loop=False))
    c0 = cfg.block_out_channels[0]
    kps_tokens = ops.ncfhw_to_nhwc(inp["kps_features"], c0).view(2, F, h * h, c0)
    audio = inp["audio_embeddings"].to(elem).contiguous()

    init_video = latent_m = composite = None
    if args.init_video:
        init_video = torch.rand(1, 3, F, 8 * h, 8 * h, generator=torch.Generator().manual_seed(7)).to(dev)
        if args.mask == "lower-half":
            pixel_m = torch.zeros(F, 8 * h, 8 * h)
            pixel_m[:, 4 * h:] = 1.0
            latent_m = latent_mask(pixel_m, F, 8).to(dev)
            composite = (init_video, pixel_m.reshape(F, -1).to(dev).contiguous())
    # with the defaults the calls below are the ones this tool has always made (no begin_index, no known)
    extra = dict(begin_index=begin) if begin or args.init_video else {}
    if args.audio_guidance_scale is not None:
        extra["audio_guidance_scale"] = args.audio_guidance_scale
    if args.overlap_blend != "mean":
        extra["overlap_blend"] = args.overlap_blend
    if args.apg_eta is not None:
        extra["apg"] = (args.apg_eta, args.apg_norm_threshold, args.apg_momentum)
    if args.guidance_refresh != 1:
        extra.update(guidance_refresh=args.guidance_refresh, guidance_reuse=args.guidance_reuse)

    def one_clip(ev=None):
        if ev:
            ev[0].record()
        if args.init_video:
            init = vae.encode_video(init_video)
            if ev:
                ev[3].record()
            lat = torch.empty_like(init)
            extra["known"] = (init, inp["latents"], latent_m)
        else:
            lat = inp["latents"] * pipe.scheduler.init_noise_sigma     # (1 but for the sigma schedulers)
        pipe.denoise(lat, kps_tokens, audio, timesteps, windows, args.guidance_scale, eta=eta, noise_seed=12345,
                     guidance_rescale=args.guidance_rescale, guidance_start=args.guidance_start,
                     guidance_end=args.guidance_end, **extra)
        if ev:
            ev[1].record()
        video = pipe.decode_latents(lat, composite=composite) if composite else pipe.decode_latents(lat)
        if ev:
            ev[2].record()
        return video

    for _ in range(args.warmup):
        one_clip()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.clips)]
    t0 = time.perf_counter()
    for ev in evs:
        video = one_clip(ev)
    torch.cuda.synchronize()
    clip_ms = 1e3 * (time.perf_counter() - t0) / args.clips
    denoise_ms = sum(e[0].elapsed_time(e[1]) for e in evs) / args.clips
    decode_ms = sum(e[1].elapsed_time(e[2]) for e in evs) / args.clips
    per_clip = [e[0].elapsed_time(e[2]) for e in evs]
    encode_ms = round(sum(e[0].elapsed_time(e[3]) for e in evs) / args.clips, 2) if args.init_video else None
    assert video.shape == (1, 3, F, args.size, args.size) and torch.isfinite(video).all()
    # one more clip with events around every update launch (kept out of the timed clips above)
    def update_launch_us(name):
        orig, marks = getattr(ops, name), []

        def marked(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = orig(*a, **k)
            e.record()
            marks.append((s, e))
            return out
        setattr(ops, name, marked)
        try:
            one_clip()
        finally:
            setattr(ops, name, orig)
        torch.cuda.synchronize()
        return len(marks), 1e3 * sum(s.elapsed_time(e) for s, e in marks) / max(len(marks), 1)

    def apg_launch_us():
        """(the ops.guidance_apg call, the plain combine of the same rows) of a guided step, microseconds: one instrumented
        clip in which every APG call is followed by the combine into a scratch buffer."""
        orig, marks = ops.guidance_apg, []

        def timed(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            return s, e

        def marked(gathered, uidx, c, f, hw, guidance, audio_guidance, *rest):
            a = timed(lambda: orig(gathered, uidx, c, f, hw, guidance, audio_guidance, *rest))
            scratch = torch.empty_like(rest[-1])
            if uidx.shape[1] == 3:
                b = timed(lambda: ops.combine_units3(gathered, uidx, c, f, hw, guidance, audio_guidance, scratch))
            else:
                b = timed(lambda: ops.combine_units(gathered, uidx, c, f, hw, guidance, scratch))
            marks.append((a, b))
        ops.guidance_apg = marked
        try:
            one_clip()
        finally:
            ops.guidance_apg = orig
        torch.cuda.synchronize()
        return [1e3 * sum(m[i][0].elapsed_time(m[i][1]) for m in marks) / max(len(marks), 1) for i in (0, 1)]

    def reuse_launch_us():
        """(the ops.combine_units_keep launch, the plain combine of the same rows, the ops.combine_reused launch),
        microseconds: one instrumented clip in which every keep launch is followed by the combine into a scratch buffer."""
        orig_keep, orig_reused, keeps, plains, reuseds = ops.combine_units_keep, ops.combine_reused, [], [], []

        def timed(fn, marks):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            marks.append((s, e))

        def keep(gathered, uidx, c, f, hw, guidance, audio_guidance, diffs, preds):
            timed(lambda: orig_keep(gathered, uidx, c, f, hw, guidance, audio_guidance, diffs, preds), keeps)
            scratch = torch.empty_like(preds)
            if uidx.shape[1] == 3:
                timed(lambda: ops.combine_units3(gathered, uidx, c, f, hw, guidance, audio_guidance, scratch), plains)
            else:
                timed(lambda: ops.combine_units(gathered, uidx, c, f, hw, guidance, scratch), plains)

        def reused(*a):
            timed(lambda: orig_reused(*a), reuseds)
        ops.combine_units_keep, ops.combine_reused = keep, reused
        try:
            one_clip()
        finally:
            ops.combine_units_keep, ops.combine_reused = orig_keep, orig_reused
        torch.cuda.synchronize()
        return [round(1e3 * sum(s.elapsed_time(e) for s, e in m) / len(m), 2) if m else None
                for m in (keeps, plains, reuseds)]
    n_updates, update_us = update_launch_us(update)
    blend_launches, blend_us = update_launch_us("known_blend") if args.init_video else (0, None)
    wblend_launches, wblend_us = update_launch_us("overlap_blend") if args.overlap_blend != "mean" else (0, None)
    post = "vae_postprocess_composite" if composite else "vae_postprocess"
    postprocess_us = round(update_launch_us(post)[1], 2)
    guided = pipe.last_guidance["guided_steps"]
    rows = pipe.last_guidance.get("rows")
    three = rows == ("u", "m", "c")
    reusing = args.guidance_refresh != 1 and len(pipe.last_guidance.get("refresh_steps", ())) < guided
    rescaled = args.guidance_rescale > 0 and guided
    rescale_us = round(update_launch_us("guidance_rescale")[1], 2) if rescaled and not three else None
    rescale3_us = round(update_launch_us("guidance_rescale3")[1], 2) if rescaled and three else None
    combine3_us = round(update_launch_us("combine_units3")[1], 2) if three and guided and not rescaled and args.apg_eta is None and not reusing else None
    apg_us = apg_combine_us = None
    if args.apg_eta is not None and guided:
        apg_us, apg_combine_us = (round(v, 2) for v in apg_launch_us())
    keep_us = keep_combine_us = reused_us = None
    if reusing:
        keep_us, keep_combine_us, reused_us = reuse_launch_us()
    combine_us = None
    if (rescale_us is None and rescale3_us is None and combine3_us is None and apg_us is None and not reusing) \
            or guided < args.steps:
        combine_us = round(update_launch_us("combine_units")[1], 2)
    ddim_us = None
    if update == "overlap_ancestral_step":
        # the DDIM update of the same clip, timed the same way (eta = 0 on a DDIM scheduler of the same steps)
        sched_a, eta_a = pipe.scheduler, eta
        pipe.scheduler, eta = vx.DDIMScheduler(**kw), 0.0
        pipe.scheduler.set_timesteps(args.steps)
        try:
            ddim_us = round(update_launch_us("overlap_ddim_step")[1], 2)
        finally:
            pipe.scheduler, eta = sched_a, eta_a
    print(json.dumps(dict(
        scheduler=args.scheduler,
        order={"dpm": args.order, "lms": args.lms_order, "unipc": args.solver_order}.get(args.scheduler),
        eta=eta if args.scheduler == "ddim-eta" else None, steps=args.steps,
        config=f"{args.size}x{args.size}, {F} frames ({'one window' if len(windows) == 1 else f'{len(windows)} windows'}), "
               f"CFG {args.guidance_scale:g}, synthetic weights, bf16",
        clips=args.clips,
        ms_per_clip=round(clip_ms, 2), denoise_ms=round(denoise_ms, 2), decode_ms=round(decode_ms, 2),
        frames_per_s=round(F * 1e3 / clip_ms, 3), update_launches=n_updates, update_us=round(update_us, 2),
        ddim_update_us=ddim_us, guidance_rescale=args.guidance_rescale, guidance_start=args.guidance_start,
        guidance_end=args.guidance_end, guided_steps=guided, rescale_us=rescale_us, combine_us=combine_us,
        audio_guidance_scale=args.audio_guidance_scale, rows=rows, combine3_us=combine3_us, rescale3_us=rescale3_us,
        apg=pipe.last_guidance.get("apg"), apg_us=apg_us, apg_combine_us=apg_combine_us,
        guidance_refresh=args.guidance_refresh, guidance_reuse=args.guidance_reuse if args.guidance_refresh != 1 else None,
        refresh_steps=pipe.last_guidance.get("refresh_steps"), keep_us=keep_us, keep_combine_us=keep_combine_us,
        reused_us=reused_us,
        clip_ms_min=round(min(per_clip), 2), clip_ms_max=round(max(per_clip), 2), init_video=args.init_video,
        strength=args.strength, mask=args.mask, begin_index=begin, steps_run=len(timesteps), encode_ms=encode_ms,
        blend_launches=blend_launches, blend_us=None if blend_us is None else round(blend_us, 2), postprocess=post,
        postprocess_us=postprocess_us, frames=F, context_frames=args.context_frames,
        context_overlap=args.context_overlap, context_schedule=args.context_schedule, windows=len(windows),
        overlap_blend=args.overlap_blend, overlap_blend_launches=wblend_launches,
        overlap_blend_us=None if wblend_us is None else round(wblend_us, 2), build=vx.lib.lib.vx_build_id().decode())))


def hires_bench(args, vx, pipe, cfg, inp, eta):
    """--hires-size: timed two-pass clips through VExpressPipeline.__call__ on features; prints the JSON line."""
    from v_express_amd import synth
    F, size2 = args.frames, args.hires_size
    inp2 = synth.synthetic_inputs(cfg, F, size2 // 8, size2 // 8, seed=42, device=inp["latents"].device)
    kw = dict(context_schedule=args.context_schedule, context_frames=args.context_frames,
              context_overlap=args.context_overlap, reference_attention_weight=0.95, audio_attention_weight=3.0,
              reference_latents=inp["ref_latents"], kps_features=inp["kps_features"],
              audio_embeddings=inp["audio_embeddings"], latents=inp["latents"], eta=eta, noise_seed=12345,
              guidance_rescale=args.guidance_rescale, guidance_start=args.guidance_start, guidance_end=args.guidance_end,
              audio_guidance_scale=args.audio_guidance_scale, overlap_blend=args.overlap_blend,
              guidance_refresh=args.guidance_refresh, guidance_reuse=args.guidance_reuse, output_device=None,
              hires_size=(size2, size2), hires_steps=args.hires_steps, hires_strength=args.hires_strength,
              hires_mode=args.hires_mode, hires_noise=inp2["latents"], hires_reference_latents=inp2["ref_latents"],
              hires_kps_features=inp2["kps_features"])
    if args.apg_eta is not None:
        kw.update(apg_eta=args.apg_eta, apg_norm_threshold=args.apg_norm_threshold, apg_momentum=args.apg_momentum)

    def one_clip():
        return pipe(None, None, None, args.size, args.size, F, args.steps, args.guidance_scale, **kw)
    for _ in range(args.warmup):
        one_clip()
    torch.cuda.synchronize()
    parts, per_clip = [], []
    t0 = time.perf_counter()
    for _ in range(args.clips):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        video = one_clip()
        e.record()
        parts.append((pipe.last_hires["events"], pipe._events))
        per_clip.append((s, e))
    torch.cuda.synchronize()
    clip_ms = 1e3 * (time.perf_counter() - t0) / args.clips
    assert video.shape == (1, 3, F, size2, size2) and torch.isfinite(video).all()
    per_clip = [s.elapsed_time(e) for s, e in per_clip]
    pass1 = sum(h[0].elapsed_time(h[1]) for h, _ in parts) / args.clips
    resize = sum(h[2].elapsed_time(h[3]) for h, _ in parts) / args.clips
    pass2 = sum(h[4].elapsed_time(h[5]) for h, _ in parts) / args.clips
    decode = sum(d[1].elapsed_time(d[2]) for _, d in parts) / args.clips
    last = pipe.last_hires
    print(json.dumps(dict(
        scheduler=args.scheduler, steps=args.steps,
        config=f"{args.size}x{args.size} -> {size2}x{size2}, {F} frames, CFG {args.guidance_scale:g}, synthetic weights, "
               f"bf16, through __call__ on features",
        clips=args.clips, ms_per_clip=round(clip_ms, 2), frames_per_s=round(F * 1e3 / clip_ms, 3),
        clip_ms_min=round(min(per_clip), 2), clip_ms_max=round(max(per_clip), 2), pass1_ms=round(pass1, 2),
        resize_us=round(1e3 * resize, 2), pass2_ms=round(pass2, 2), decode_ms=round(decode, 2),
        other_ms=round(sum(per_clip) / args.clips - pass1 - resize - pass2 - decode, 2), hires_size=size2,
        hires_steps=last["steps"], hires_strength=args.hires_strength, hires_mode=last["mode"],
        hires_begin_index=last["begin_index"], hires_steps_run=last["steps"] - last["begin_index"], frames=F,
        windows=pipe.last_overlap["windows"], build=vx.lib.lib.vx_build_id().decode())))


if __name__ == "__main__":
    main()
