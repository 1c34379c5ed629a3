"""The one restated denoising loop (TEST INFRASTRUCTURE): pipelines/v_express_pipeline.py:526-583 in float64 over the
oracle UNet with every extension the project has made to it, laid out as v-express_amd/sampling.py is - the guided
prediction of one window, the stitch (the reference's mean, or per-frame normalised weights), one update per frame per
timestep, the known blend - so that a new loop feature is one edit here.  The arithmetic itself is imported: the
schedule tables and updates of dpm_restated / ancestral_restated, the step rule and rescale of guidance_restated, the row
rule of audio_guidance_restated, the levels of init_video_restated and the weights of window_blend_restated."""
import math

import torch

import ancestral_restated as A
import audio_guidance_restated as AG
import dpm_restated as D
import guidance_restated as G
import init_video_restated as R
import window_blend_restated as WB

DPM = dict(solver_order=2, lower_order_final=True, euler_at_final=False, final="zero")


def oracle_rows_unet(sd3, sd2, ocfg, ref_latents, w_ref, w_aud):
    """The oracle UNet with a bank per batch row: fn(x [b, 4, f, h, w], t, audio [b * f, n_ctx, 768], kps [b, C0, f, h,
    w], bank_rows) with bank_rows[i] = 1 for the reference bank and 0 for the all-zero one (what
    ReferenceAttentionControl's cat([zeros, v]) gives rows 0 / 1; the oracle takes banks as plain [b, hw, C] tensors)."""
    from oracle import unet as OU
    ref = OU.refnet_banks(sd2, ocfg, ref_latents)

    def fn(x, t, audio, kps, bank_rows):
        banks = {k: torch.cat([v if r else torch.zeros_like(v) for r in bank_rows]) for k, v in ref.items()}
        return OU.unet3d_forward(sd3, ocfg, x, t, audio, kps, banks, w_ref, w_aud)
    return fn


def guided_prediction(unet_fn, x, t, ctx, names, guided, s, s_a, phi, kps_feature, audio_embeddings):
    """The prediction of window `ctx` from latents x [1, c, f, h, w] (:540-550): one UNet call over the rows `names` of
    AG.ROWS, combined as u + s (m - u) + s_a (c - m) (three rows), m + s_a (c - m) (rows m, c) or u + s (c - u) (rows u,
    c) and rescaled towards std(c) for phi > 0; the c row as it is when it is the only one or the step is not guided."""
    trip = [AG.ROWS[r] for r in names]
    aud = torch.cat([audio_embeddings[a][ctx] for _, _, a in trip])
    kps = torch.stack([kps_feature[k][:, ctx] for _, k, _ in trip])
    out = unet_fn(x.float().repeat(len(trip), 1, 1, 1, 1), t, aud, kps, [b for b, _, _ in trip]).double()
    p = {r: out[j:j + 1] for j, r in enumerate(names)}
    if not guided or names == ("c",):
        return p["c"]
    if names == ("u", "m", "c"):
        pred = p["u"] + s * (p["m"] - p["u"]) + s_a * (p["c"] - p["m"])
    elif names == ("m", "c"):
        pred = p["m"] + s_a * (p["c"] - p["m"])
    else:
        pred = p["u"] + s * (p["c"] - p["u"])
    return G.rescale(pred, p["c"], phi) if phi > 0.0 else pred


def stitch_mean(preds, windows, F_):
    """{frame: prediction} as :552-572 writes it: pred / count, accumulated in window order until a frame's count is
    reached (a frame that completes twice in one window, e.g. 9 of [8, 9, 10, 9], keeps the last)."""
    count = torch.zeros(F_, dtype=torch.long)
    for ctx in windows:
        count[ctx] += 1
    counter = torch.zeros(F_, dtype=torch.long)
    pending, final = [None] * F_, {}
    for ctx, pred in zip(windows, preds):
        counter[ctx] += 1
        pred = pred / count[ctx][None, None, :, None, None].double()
        for li, fi in enumerate(ctx):
            pending[fi] = pred[:, :, li].clone() if pending[fi] is None else pending[fi] + pred[:, :, li]
            if counter[fi] == count[fi]:
                final[fi] = pending[fi]
                pending[fi] = None
    return final


def stitch_weighted(preds, windows, F_, raw):
    """{frame: prediction}: the weighted sum of the windows that hold the frame, float64 weights raw / sum(raw of the
    frame) (raw [nW][f])."""
    norm = WB.normalised(windows, F_, raw)
    return {fi: sum(wt * preds[wi][:, :, li] for wi, li, wt in norm[fi]) for fi in range(F_)}


def frame_update(sampler, i, fi, x, v, hist, sg, order, tab, seed, eta):
    """One update of frame fi [1, c, h, w] at step index i: (x', the frame's x0 history), the textbook updates of
    dpm_restated / ancestral_restated with the counter-based noise."""
    if sampler == "dpm":
        return D.update(sg, i, order, x, v, hist)
    _, c, h, w = x.shape
    if sampler == "euler-a":
        return A.euler_a_update_ve(sg[i], sg[i + 1], x, v, A.noise_like(seed, i, fi, c, h, w)[None]), hist
    z = A.noise_like(seed, i, fi, c, h, w)[None] if sampler == "ddim-eta" else 0.0
    a, ap = tab[i]
    return A.ddim_eta_update(a, ap, eta if sampler == "ddim-eta" else 0.0, x, v, z), hist


def known_level(known, sampler, n, sg, j):
    """add_noise(init, noise, t_j) at step index j, init itself at j = n; Euler ancestral in its own (VE) frame."""
    init, noise = known[0].double(), known[1].double()
    if j == n:
        return init.clone()
    if sampler == "euler-a":
        return init + sg[j] * noise
    a, s = R.coefficients(sampler, n)[j]
    return a * init + s * noise


def known_blend(lat, known, sampler, n, sg, j):
    """diffusers' inpaint blend after a step: m lat + (1 - m) known_level(j); lat itself without a mask."""
    if known is None or known[2] is None:
        return lat
    mm = known[2].double().reshape(1, 1, *lat.shape[2:])
    return mm * lat + (1.0 - mm) * known_level(known, sampler, n, sg, j)


def restated_loop(unet_fn, latents, windows, s, kps_feature, audio_embeddings, n, sampler="ddim", *, s_a=None, phi=0.0,
                  start=0.0, end=1.0, unguided=("c",), seed=None, eta=0.0, sched_kw=None, raw=None, known=None):
    """The final latents (float64) of n steps over `windows`; the defaults are the reference's own loop (DDIM, one scale,
    the mean).  `unet_fn` of oracle_rows_unet; kps_feature / audio_embeddings in the CFG layout (row 0 zeros).
    s, s_a: the scales, rows by AG.rows_for; phi: the CFG rescale; start / end: the guidance interval, counted over the
    steps that run (an unguided step takes the c row as it is, from a UNet call over the rows `unguided`: c alone as the
    product calls it; ("u", "c") is the call of the two-row tests - the rows are independent, but the float32 oracle
    rounds a row of a batch of two differently in the last place).  sampler "ddim", "ddim-eta" (eta, seed), "dpm" (sched_kw:
    the keys of DPM) or "euler-a" (seed; VE frame: latents x sigma_0, the UNet fed x / sqrt(1 + sigma^2)).  raw: None for
    the reference's mean, else [nW][f] weights.  known = (init, noise, m, strength): started as diffusers' img2img
    pipelines start (`latents` is then not read) and, with m [F, h * w] (1 = regenerate), blended after every step."""
    kw = dict(DPM, **(sched_kw or {}))
    rows = AG.rows_for(s, s_a)
    F_ = latents.shape[2]
    sg = D.sigmas(n, kw["final"])
    b = 0 if known is None else R.begin_index(n, known[3])
    if known is not None:
        lat = known_level(known, sampler, n, sg, b)
    else:
        lat = latents.double() * (sg[0] if sampler == "euler-a" else 1.0)
    scale = [1.0 / math.sqrt(1.0 + x ** 2) if sampler == "euler-a" else 1.0 for x in sg]
    guided = G.guided_steps(n - b, start, end)
    ords = D.orders(n, kw["solver_order"], kw["lower_order_final"], kw["euler_at_final"], kw["final"], begin=b)
    tab, ts = A.ddim_table(n), D.timesteps(n)
    hist = torch.zeros_like(lat)
    for i in range(b, n):
        names = rows if guided[i - b] else unguided
        preds = [guided_prediction(unet_fn, lat[:, :, ctx] * scale[i], ts[i], ctx, names, guided[i - b], s, s_a, phi,
                                   kps_feature, audio_embeddings) for ctx in windows]
        v = stitch_mean(preds, windows, F_) if raw is None else stitch_weighted(preds, windows, F_, raw)
        x = lat.clone()
        for fi, vf in v.items():
            lat[:, :, fi], hist[:, :, fi] = frame_update(sampler, i, fi, x[:, :, fi], vf, hist[:, :, fi], sg, ords[i - b],
                                                         tab, seed, eta)
        lat = known_blend(lat, known, sampler, n, sg, i + 1)
    return lat
