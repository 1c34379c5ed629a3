"""Restatements of adaptive projected guidance (TEST INFRASTRUCTURE) for tests/test_apg_cpu.py and tests/test_gpu_apg.py:
Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models" (ICLR 2025)
as include/vexpress_hip_guidance.h states it - per window and per frame, each guidance difference d runs through a
momentum (dbar = d + beta * previous dbar), is capped at the norm r and has its part parallel to the conditional row c
scaled by eta.  `project` is the float64 formula, `bound` the elementwise error bound of the float32 kernel against it,
`guidance_apg` a float32 CPU stand-in with `ops.guidance_apg`'s signature in the style of guidance_restated.py, and
`restated_loop` tests/loop_restated.py's loop with the projected prediction and the per-window momentum in place of its
`guided_prediction`."""
import torch

import audio_guidance_restated as AG
import loop_restated as LR

CHUNK = 256                       # pixels per partial of vx_guidance_apg
K = 64                            # the roundings the bound allows for (`bound`)


def project(rows, scales, eta, r, beta, prev, dims):
    """float64 APG of the rows (u, c), (m, c) or (u, m, c) (tensors of one shape) with one scale per difference
    rows[j + 1] - rows[j]; the statistics run over `dims`.  prev: the previous dbar of every difference, or None for
    zeros.  Returns (g, [dbar per difference], [sqrt(S_dd / S_cc) per difference])."""
    rows = [x.double() for x in rows]
    cnd = rows[-1]
    scc = (cnd * cnd).sum(dims, keepdim=True)
    one, zero = torch.ones_like(scc), torch.zeros_like(scc)
    g, dbars, ratios = cnd.clone(), [], []
    for j, s in enumerate(scales):
        dbar = rows[j + 1] - rows[j]
        if prev is not None:
            dbar = dbar + beta * prev[j].double()
        sdd = (dbar * dbar).sum(dims, keepdim=True)
        sdc = (dbar * cnd).sum(dims, keepdim=True)
        capped = (sdd > 0) & (r > 0)
        phi = torch.where(capped, torch.minimum(one, r / torch.sqrt(torch.where(capped, sdd, one))), one)
        k = torch.where(scc > 0, sdc / torch.where(scc > 0, scc, one), zero)
        g = g + (s - 1.0) * phi * (dbar - (1.0 - eta) * k * cnd)
        dbars.append(dbar)
        ratios.append(torch.sqrt(sdd / scc))
    return g, dbars, ratios


def bound(rows, scales, beta, prev, dbars, ratios):
    """K 2^-24 (|c| + sum over the differences of |s - 1| (|d| + |beta dbar_prev| + |dbar| + sqrt(S_dd / S_cc) |c|)),
    elementwise in float64.  K = 64: a sum of the kernel is at most 16 sequential adds per thread (4 at c = 4: one pixel
    per thread), 6 shuffle levels, 3 cross-wave adds and one product rounding - 26 roundings -, then the quotient, the
    two coefficients and the four roundings of g."""
    rows = [x.double() for x in rows]
    cnd = rows[-1].abs()
    mag = cnd.clone()
    for j, s in enumerate(scales):
        p = torch.zeros_like(cnd) if prev is None else (beta * prev[j].double()).abs()
        mag = mag + abs(s - 1.0) * ((rows[j + 1] - rows[j]).abs() + p + dbars[j].abs() + ratios[j] * cnd)
    return K * 2.0 ** -24 * mag


def unit_rows(gathered, unit_index, c, f, hw):
    """The all-gathered buffer seen through unit_index: the rows, float32 [nW, c, f, hw] each."""
    nW, rows, S = unit_index.shape
    g = gathered.reshape(-1, (f // S) * hw, c)
    h = g.index_select(0, unit_index.reshape(-1).long()).view(nW, rows, f, hw, c).permute(1, 0, 4, 2, 3)
    return [h[r] for r in range(rows)]


def guidance_apg(gathered, unit_index, c, f, hw, guidance, audio_guidance, eta, norm_threshold, momentum, momentum_buf,
                 workspace, preds):
    """Emulated ops.guidance_apg: float32 differences, momentum, products and g as the kernel forms them (every operation
    rounded on its own), the sums of a frame in float64, A and B in float64 rounded once."""
    nW, rows, _ = unit_index.shape
    assert rows in (2, 3) and 0.0 <= eta <= 1.0 and norm_threshold >= 0.0 and abs(momentum) < 1.0
    assert (momentum != 0.0) == (momentum_buf is not None)
    assert workspace.numel() >= nW * f * ((hw + CHUNK - 1) // CHUNK) * (2 * (rows - 1) + 1)
    f32 = torch.float32
    xs = [x.contiguous() for x in unit_rows(gathered, unit_index, c, f, hw)]
    cnd = xs[-1]
    scc = (cnd * cnd).double().sum((1, 3), keepdim=True)
    one = torch.ones_like(scc)
    g = cnd.clone()
    for j, s in enumerate((guidance, audio_guidance)[:rows - 1]):
        d = xs[j + 1] - xs[j]
        if momentum != 0.0:
            buf = momentum_buf.view(rows - 1, nW, c, f, hw)[j]
            d = d + torch.tensor(momentum, dtype=f32) * buf
            buf.copy_(d)
        sdd = (d * d).double().sum((1, 3), keepdim=True)
        sdc = (d * cnd).double().sum((1, 3), keepdim=True)
        capped = (sdd > 0) & (norm_threshold > 0.0)
        r = float(torch.tensor(norm_threshold, dtype=f32))
        phi = torch.where(capped, torch.minimum(one, r / torch.sqrt(torch.where(capped, sdd, one))), one)
        k = torch.where(scc > 0, sdc / torch.where(scc > 0, scc, one), torch.zeros_like(scc))
        a = (float(torch.tensor(s, dtype=f32)) - 1.0) * phi
        b = a * (1.0 - float(torch.tensor(eta, dtype=f32))) * k
        g = (g + a.float() * d) - b.float() * cnd
    preds.copy_(g.view_as(preds))


class ProjectedPrediction:
    """A stateful stand-in for loop_restated.guided_prediction: the float64 projection of every window's rows per frame,
    with the momentum of every window (windows are visited in order, `n_windows` per step) carried between the guided
    steps; an unguided step is loop_restated's own and leaves the momentum alone."""

    def __init__(self, n_windows, eta, r, beta):
        self.n, self.eta, self.r, self.beta = n_windows, eta, r, beta
        self.prev, self.calls = [None] * n_windows, 0
        self.capped = []                               # per guided (step, window): which frames the cap bit on

    def __call__(self, unet_fn, x, t, ctx, names, guided, s, s_a, phi, kps_feature, audio_embeddings):
        w = self.calls % self.n
        self.calls += 1
        if not guided or names == ("c",):
            return _PLAIN(unet_fn, x, t, ctx, names, guided, s, s_a, phi, kps_feature, audio_embeddings)
        assert phi == 0.0
        trip = [AG.ROWS[r] for r in names]
        aud = torch.cat([audio_embeddings[a][ctx] for _, _, a in trip])
        kps = torch.stack([kps_feature[k][:, ctx] for _, k, _ in trip])
        out = unet_fn(x.float().repeat(len(trip), 1, 1, 1, 1), t, aud, kps, [b for b, _, _ in trip]).double()
        rows = [out[j:j + 1] for j in range(len(names))]
        scales = {("u", "c"): (s,), ("m", "c"): (s_a,), ("u", "m", "c"): (s, s_a)}[names]
        g, dbars, _ = project(rows, scales, self.eta, self.r, self.beta, self.prev[w], (1, 3, 4))
        self.prev[w] = dbars
        if self.r > 0:
            self.capped.append([(d * d).sum((1, 3, 4)).flatten().sqrt() > self.r for d in dbars])
        return g


_PLAIN = LR.guided_prediction


def restated_loop(unet_fn, latents, windows, s, kps_feature, audio_embeddings, n, sampler="ddim", *, eta, r, beta, **kw):
    """loop_restated.restated_loop with APG (eta, r, beta) on its guided steps: (final latents float64, the
    ProjectedPrediction that ran).  loop_restated looks `guided_prediction` up as a module global: it is replaced for
    the duration of the call."""
    state = ProjectedPrediction(len(windows), eta, r, beta)
    LR.guided_prediction = state
    try:
        return LR.restated_loop(unet_fn, latents, windows, s, kps_feature, audio_embeddings, n, sampler, **kw), state
    finally:
        LR.guided_prediction = _PLAIN


def check_argument_errors(so, gathered, unit_index, momentum_buf, workspace, preds):
    """Every argument vx_guidance_apg of the library `so` must refuse - before any launch, rc < 0, the argument named
    in the message - on device pointers (integers) of one window of 4 channels, 4 frames and 16 pixels, two rows."""
    inf, nan = float("inf"), float("nan")
    need = so.vx_guidance_apg_ws_floats(1, 2, 4, 16)
    assert need == 1 * 4 * 1 * 3 and so.vx_guidance_apg_ws_floats(2, 3, 16, 4096) == 2 * 16 * 16 * 5
    good = dict(rows=2, eta=0.0, r=0.0, beta=0.0, buf=None, ws_floats=need)
    for change, word in ((dict(rows=1), b"rows"), (dict(rows=4), b"rows"), (dict(eta=1.5), b"eta"),
                         (dict(eta=-0.25), b"eta"), (dict(eta=nan), b"eta"), (dict(r=-1.0), b"norm_threshold"),
                         (dict(r=inf), b"norm_threshold"), (dict(r=nan), b"norm_threshold"),
                         (dict(beta=1.0), b"momentum"), (dict(beta=-1.5), b"momentum"), (dict(beta=nan), b"momentum"),
                         (dict(ws_floats=need - 1), b"workspace"), (dict(beta=-0.5), b"momentum_buf"),
                         (dict(buf=momentum_buf), b"momentum_buf")):
        a = dict(good, **change)
        rc = so.vx_guidance_apg(gathered, unit_index, 1, a["rows"], 1, 4, 4, 16, 3.5, 6.0, a["eta"], a["r"], a["beta"],
                                a["buf"], workspace, a["ws_floats"], preds, None)
        msg = so.vx_last_error_string()
        assert rc < 0 and b"vx_guidance_apg" in msg and word in msg, (change, rc, msg)
