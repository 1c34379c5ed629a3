"""Restatements of guidance reuse (TEST INFRASTRUCTURE) for tests/test_guidance_reuse_cpu.py and
tests/test_gpu_guidance_reuse.py: the step-role rule (a guided step refreshes if it is the first or the last guided step
or k - 1 reuse steps have passed since the last refresh), the prediction of a reuse step
    g = c + sum_k [a_k L_k + b_k P_k],   a_k = (s_k - 1)(1 + w),   b_k = -(s_k - 1) w
(L_k / P_k: difference k of the rows at the last refresh / at the one before it; w = 0 for "hold" and, for "linear",
(i - i_last) / (i_last - i_prev) once two refreshes exist), float32 CPU stand-ins with the signatures of
`ops.combine_units_keep` / `ops.combine_reused`, tests/loop_restated.py's loop with reuse in place of its
`guided_prediction`, the L1 weight of a step's prediction on UNet outputs, and the scalar Gaussian model of the issue."""
import math

import torch

import ancestral_restated as A
import audio_guidance_restated as AG
import fake_ops
import guidance_restated as G
import loop_restated as LR

MODES = ("hold", "linear")


def roles(guided, k):
    """None (unguided), "refresh" or "reuse" per step, restated from the issue's three conditions."""
    guided_idx = [i for i, g in enumerate(guided) if g]
    out = [None] * len(guided)
    reuse_run = 0
    for i in guided_idx:
        if i == guided_idx[0] or i == guided_idx[-1] or reuse_run == k - 1:
            out[i] = "refresh"
            reuse_run = 0
        else:
            out[i] = "reuse"
            reuse_run += 1
    return out


def weight(mode, i, refreshes):
    """w of a reuse step at loop index i after the refreshes at the indices `refreshes` (ascending)."""
    if mode == "hold" or len(refreshes) < 2:
        return 0.0
    return (i - refreshes[-1]) / (refreshes[-1] - refreshes[-2])


def coefficients(scales, w):
    """[(a_k, b_k)] in double."""
    return [((s - 1.0) * (1.0 + w), -(s - 1.0) * w) for s in scales]


def scales_for(names, s, s_a):
    return {("u", "c"): (s,), ("m", "c"): (s_a,), ("u", "m", "c"): (s, s_a)}[names]


def l1_ratio(names, s, s_a, guided, k, mode):
    """S of the loop bound 5e-2 max(1, S): the largest ratio, over the steps, of the L1 weight on UNet outputs in the
    step's guided prediction to plain CFG's |1 - s| + |s|.  A refresh step of two rows weighs |1 - s| + |s|, of three
    rows |1 - s| + |s - s_a| + |s_a|; a reuse step c + sum a_k L_k + b_k P_k weighs 1 + 2 sum (|a_k| + |b_k|) (every
    stored difference is a difference of two outputs); an unguided step weighs 1."""
    scales = scales_for(names, s, s_a)
    plain = abs(1.0 - s) + abs(s)
    if len(scales) == 2:
        full = abs(1.0 - s) + abs(s - s_a) + abs(s_a)
    else:
        full = abs(1.0 - scales[0]) + abs(scales[0])
    worst, done = 0.0, []
    for i, role in enumerate(roles(guided, k)):
        if role == "refresh":
            wt = full
            done.append(i)
        elif role == "reuse":
            wt = 1.0 + 2.0 * sum(abs(a) + abs(b) for a, b in coefficients(scales, weight(mode, i, done)))
        else:
            wt = 1.0
        worst = max(worst, wt / plain)
    return worst


# ------------------------------------------------------------------------------------------------ the stand-ins
def combine_units_keep(gathered, unit_index, c, f, hw, guidance, audio_guidance, diffs, preds):
    """Emulated ops.combine_units_keep: preds by the emulated combine of the same rows (fake_ops.combine_units /
    audio_guidance_restated.combine_units3: the same bits), diffs the float32 subtractions."""
    nW, rows, S = unit_index.shape
    assert rows in (2, 3) and diffs.numel() == (rows - 1) * preds.numel()
    if rows == 2:
        fake_ops.combine_units(gathered, unit_index, c, f, hw, guidance, preds)
    else:
        AG.combine_units3(gathered, unit_index, c, f, hw, guidance, audio_guidance, preds)
    g = gathered.reshape(-1, (f // S) * hw, c)
    h = g.index_select(0, unit_index.reshape(-1).long()).view(nW, rows, f, hw, c).permute(1, 0, 4, 2, 3)
    d = diffs.view(rows - 1, nW, c, f, hw)
    for k in range(rows - 1):
        d[k].copy_(h[k + 1].float() - h[k].float())


def reused_f32(cnd, last, prev, a1, b1, a2, b2):
    """The float32 torch expression of vx_combine_reused in its stated order: every product and sum rounded on its own.
    cnd [nW, c, f, hw]; last / prev [n, nW, c, f, hw] (prev None: the b terms are left out)."""
    f32 = torch.float32
    t = [torch.tensor(v, dtype=f32) for v in (a1, b1, a2, b2)]
    p = cnd + t[0] * last[0]
    if prev is not None:
        p = p + t[1] * prev[0]
    if last.shape[0] == 2:
        p = p + t[2] * last[1]
        if prev is not None:
            p = p + t[3] * prev[1]
    return p


def combine_reused(gathered, unit_index, c, f, hw, last, prev, a1, b1, a2, b2, preds):
    """Emulated ops.combine_reused."""
    nW, rows, S = unit_index.shape
    assert rows == 1 and last.numel() in (preds.numel(), 2 * preds.numel())
    assert (b1 != 0.0 or b2 != 0.0) == (prev is not None)
    n = last.numel() // preds.numel()
    assert n == 2 or (a2 == 0.0 and b2 == 0.0)
    g = gathered.reshape(-1, (f // S) * hw, c)
    cnd = g.index_select(0, unit_index.reshape(-1).long()).view(nW, f, hw, c).permute(0, 3, 1, 2).float()
    shape = (n, nW, c, f, hw)
    preds.copy_(reused_f32(cnd, last.view(shape), None if prev is None else prev.view(shape), a1, b1, a2, b2)
                .view_as(preds))


def check_argument_errors(so, gathered, unit_index, diffs, last, prev, preds):
    """Every argument vx_combine_units_keep / vx_combine_reused of the library `so` must refuse - before any launch,
    rc < 0, the argument named in the message - on device pointers (integers) of one window of 4 channels, 4 frames and
    16 pixels."""
    for rows in (1, 4):
        rc = so.vx_combine_units_keep(gathered, unit_index, 1, rows, 1, 4, 4, 16, 3.5, 6.0, diffs, preds, None)
        msg = so.vx_last_error_string()
        assert rc < 0 and b"vx_combine_units_keep" in msg and b"rows" in msg, (rows, rc, msg)
    rc = so.vx_combine_units_keep(gathered, unit_index, 1, 2, 1, 4, 4, 16, 3.5, 6.0, None, preds, None)
    assert rc < 0 and b"diffs" in so.vx_last_error_string()
    rc = so.vx_combine_units_keep(gathered, unit_index, 1, 2, 3, 4, 4, 16, 3.5, 6.0, diffs, preds, None)
    assert rc < 0 and b"shards" in so.vx_last_error_string()
    good = dict(n=1, last=last, prev=None, a1=2.5, b1=0.0, a2=0.0, b2=0.0)
    for change, word in ((dict(n=0), b"n_diffs"), (dict(n=3), b"n_diffs"), (dict(b1=-2.5), b"prev"),
                         (dict(prev=prev), b"prev"), (dict(n=2, b2=-5.0), b"prev"), (dict(last=None), b"last"),
                         (dict(a2=5.0), b"a2"), (dict(a1=float("nan")), b"a1"), (dict(b1=float("inf"), prev=prev), b"b1")):
        a = dict(good, **change)
        rc = so.vx_combine_reused(gathered, unit_index, 1, a["n"], 1, 4, 4, 16, a["last"], a["prev"], a["a1"], a["b1"],
                                  a["a2"], a["b2"], preds, None)
        msg = so.vx_last_error_string()
        assert rc < 0 and b"vx_combine_reused" in msg and word in msg, (change, rc, msg)


# ------------------------------------------------------------------------------------------------ the loop
class ReusedPrediction:
    """A stateful stand-in for loop_restated.guided_prediction (windows are visited in order, `n_windows` per step, the
    loop starting at step index 0): a refresh step is loop_restated's own guided prediction and keeps the float64
    differences of the window's rows; a reuse step runs the conditional row alone (the UNet call of an unguided step)
    and adds the kept differences; an unguided step is loop_restated's own."""

    def __init__(self, n_windows, role_list, mode):
        self.n, self.roles, self.mode = n_windows, role_list, mode
        self.kept = [[] for _ in range(n_windows)]       # per window: [(step index, [d_k])] of its refreshes
        self.calls, self.log = 0, []

    def __call__(self, unet_fn, x, t, ctx, names, guided, s, s_a, phi, kps_feature, audio_embeddings):
        w, i = self.calls % self.n, self.calls // self.n
        self.calls += 1
        role = self.roles[i]
        if w == 0:
            self.log.append(role)
        if role is None or names == ("c",):
            return _PLAIN(unet_fn, x, t, ctx, names, guided, s, s_a, phi, kps_feature, audio_embeddings)
        assert phi == 0.0 and guided
        if role == "reuse":
            cnd = _PLAIN(unet_fn, x, t, ctx, ("c",), False, s, s_a, phi, kps_feature, audio_embeddings)
            done = [j for j, _ in self.kept[w]]
            g = cnd.clone()
            for k, (a, b) in enumerate(coefficients(scales_for(names, s, s_a), weight(self.mode, i, done))):
                g = g + a * self.kept[w][-1][1][k]
                if b != 0.0:
                    g = g + b * self.kept[w][-2][1][k]
            return g
        trip = [AG.ROWS[r] for r in names]
        aud = torch.cat([audio_embeddings[a][ctx] for _, _, a in trip])
        kps = torch.stack([kps_feature[k][:, ctx] for _, k, _ in trip])
        out = unet_fn(x.float().repeat(len(trip), 1, 1, 1, 1), t, aud, kps, [b for b, _, _ in trip]).double()
        rows = [out[j:j + 1] for j in range(len(names))]
        self.kept[w].append((i, [rows[j + 1] - rows[j] for j in range(len(rows) - 1)]))
        if names == ("u", "m", "c"):
            return rows[0] + s * (rows[1] - rows[0]) + s_a * (rows[2] - rows[1])
        return rows[0] + scales_for(names, s, s_a)[0] * (rows[1] - rows[0])


_PLAIN = LR.guided_prediction


def restated_loop(unet_fn, latents, windows, s, kps_feature, audio_embeddings, n, sampler="ddim", *, k, mode, **kw):
    """loop_restated.restated_loop with guidance reuse (period k, mode): (final latents float64, the ReusedPrediction
    that ran).  loop_restated looks `guided_prediction` up as a module global: it is replaced for the call."""
    assert mode in MODES and "known" not in kw
    guided = G.guided_steps(n, kw.get("start", 0.0), kw.get("end", 1.0))
    state = ReusedPrediction(len(windows), roles(guided, k), mode)
    LR.guided_prediction = state
    try:
        return LR.restated_loop(unet_fn, latents, windows, s, kps_feature, audio_embeddings, n, sampler, **kw), state
    finally:
        LR.guided_prediction = _PLAIN


# ------------------------------------------------------------------------------------------------ the scalar model
def gaussian_final_mean(n, s, k, mode, mu=1.0, sd=0.6):
    """Exact DDIM sampling of N(mu, sd^2) by its exact v-prediction on this project's schedule, guided from the
    unconditional model N(0, sd^2) with the scale s and the reuse period k: (final mean, final std) started from N(0, 1).
    With a = sqrt(abar_t), sg = sqrt(1 - abar_t), D = a^2 sd^2 + sg^2: v(x | mu) = (x - a mu) a sg (1 - sd^2) / D - sg mu,
    so c - u = -mu sg / D does not depend on x; mean and std evolve exactly, the std without any effect of reuse."""
    tab = A.ddim_table(n)
    role_list = roles([True] * n, k)
    mean, std, kept = 0.0, 1.0, []
    for i, (abar, abar_prev) in enumerate(tab):
        a, sg = math.sqrt(abar), math.sqrt(1.0 - abar)
        ap, sp = math.sqrt(abar_prev), math.sqrt(1.0 - abar_prev)
        dd = a * a * sd * sd + sg * sg
        slope = a * sg * (1.0 - sd * sd) / dd
        v_c = (mean - a * mu) * slope - sg * mu
        d = -mu * sg / dd
        if role_list[i] == "refresh":
            v = v_c + (s - 1.0) * d
            kept.append((i, d))
        else:
            (aa, bb), = coefficients((s,), weight(mode, i, [j for j, _ in kept]))
            v = v_c + aa * kept[-1][1] + (bb * kept[-2][1] if bb != 0.0 else 0.0)
        # x' = ap (a x - sg v) + sp (sg x + a v)
        mean = (ap * a + sp * sg) * mean + (sp * a - ap * sg) * v
        std = abs((ap * a + sp * sg) + (sp * a - ap * sg) * slope) * std
    return mean, std
