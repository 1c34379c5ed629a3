"""Restatements of the weighted window blend (TEST INFRASTRUCTURE) for tests/test_window_blend_cpu.py and
tests/test_gpu_window_blend.py: the even-fit window starts and the raw weights ("linear", "pyramid") written out from
their definitions, the per-frame plan with its normalised weights, and `ops.overlap_blend` in float32 torch arithmetic
(the kernel's bits: one rounding per product and per sum, the first valid term initialises) and in float64 with its bound.
The loop that uses them is tests/loop_restated.py."""
import math

import torch


U = 2.0 ** -24                    # unit roundoff of float32


# ------------------------------------------------------------------------------------------------ schedule and weights
def fit_starts(F_, f, o):
    """Window starts of the even-fit schedule: ceil((F - o) / (f - o)) windows, start k at floor(k (F - f) / (n - 1))."""
    if F_ <= f:
        return [0]
    n = math.ceil((F_ - o) / (f - o))
    return [(k * (F_ - f)) // (n - 1) for k in range(n)]


def fit_windows(F_, f, o):
    return [list(range(s, s + min(f, F_))) for s in fit_starts(F_, f, o)]


def uniform_count(F_, f, o):
    """Windows of the reference's single-level schedule: starts 0, f - o, ... while start < F - o."""
    return 1 if F_ <= f else len(range(0, F_ - o, f - o))


def pyramid(f):
    return [float(min(j + 1, f - j)) for j in range(f)]


def linear(starts, f):
    """float64 [nW][f]: 1 inside, a ramp j + 1 over L + 1 across the L frames shared with the window before and f - j over
    R + 1 across the R frames shared with the one after."""
    out = []
    for k, s in enumerate(starts):
        left = f - (s - starts[k - 1]) if k else 0
        right = f - (starts[k + 1] - s) if k + 1 < len(starts) else 0
        row = []
        for j in range(f):
            w = 1.0
            if left > 0:
                w = min(w, (j + 1) / (left + 1))
            if right > 0:
                w = min(w, (f - j) / (right + 1))
            row.append(w)
        out.append(row)
    return out


def raw_weights(windows, blend):
    f = len(windows[0])
    if blend == "linear":
        return linear([w[0] for w in windows], f)
    row = pyramid(f) if blend == "pyramid" else [float(v) for v in blend]
    return [list(row) for _ in windows]


def frame_terms(windows, F_):
    """{frame: [(window, position), ...]} in ascending window order."""
    terms = {i: [] for i in range(F_)}
    for wi, w in enumerate(windows):
        for li, fi in enumerate(w):
            terms[fi].append((wi, li))
    return terms


def normalised(windows, F_, raw):
    """{frame: [(window, position, float64 weight), ...]}, the weights of a frame summing to 1."""
    out = {}
    for fi, tt in frame_terms(windows, F_).items():
        tot = sum(raw[wi][li] for wi, li in tt)
        out[fi] = [(wi, li, raw[wi][li] / tot) for wi, li in tt]
    return out


def max_jump(per_frame):
    """Largest |v[i + 1] - v[i]| of a per-frame sequence of numbers."""
    return max(abs(b - a) for a, b in zip(per_frame[:-1], per_frame[1:]))


def blend_constants(windows, F_, raw, offsets):
    """The blended prediction of every frame when window k predicts the constant offsets[k] (float64); raw None = mean."""
    if raw is None:
        raw = [[1.0] * len(w) for w in windows]
    norm = normalised(windows, F_, raw)
    return [sum(w * offsets[wi] for wi, _, w in norm[i]) for i in range(F_)]


# ------------------------------------------------------------------------------------------------ the op
def tables(plan, device="cpu"):
    """(terms int32 [F, T, 2], weights float32 [F, T]) of a context.weighted_overlap_plan, as the op takes them."""
    return torch.from_numpy(plan["term_table"]).to(device), torch.from_numpy(plan["weights"]).to(device)


def overlap_blend(preds, terms, weights, out):
    """`ops.overlap_blend` restated in float32 torch arithmetic (any device): out[ch, i, px] = sum over t, in ascending
    t, of weights[i][t] * preds[slot, ch, li, px]; every product and sum is one float32 operation of its own and the
    first valid term (slot >= 0) initialises the sum - the kernel's bits."""
    assert preds.dtype == weights.dtype == out.dtype == torch.float32 and terms.dtype == torch.int32
    _, c, _, hw = preds.shape
    n, T = weights.shape
    assert tuple(terms.shape) == (n, T, 2) and out.numel() == c * n * hw and hw % 4 == 0
    v = torch.zeros((n, c, hw), dtype=torch.float32, device=preds.device)
    started = torch.zeros(n, dtype=torch.bool, device=preds.device)
    for t in range(T):
        slot, li = terms[:, t, 0].long(), terms[:, t, 1].long()
        valid = slot >= 0
        term = weights[:, t, None, None] * preds[slot.clamp_min(0), :, li.clamp_min(0)]       # [F, c, hw]
        new = torch.where(started[:, None, None], v + term, term)
        v = torch.where(valid[:, None, None], new, v)
        started = started | valid
    out.view(c, n, hw).copy_(v.permute(1, 0, 2))


def overlap_blend64(preds, terms, weights):
    """float64 (value [c, F, hw], bound): the same sum without rounding, and 2 T 2^-24 sum_t |w_t p_t| with T the term
    columns of the table (one rounding per product and per add, each acting on a partial sum no larger than sum |w p|)."""
    _, c, _, hw = preds.shape
    n, T = weights.shape
    v = torch.zeros((n, c, hw), dtype=torch.float64)
    mag = torch.zeros_like(v)
    for t in range(T):
        slot, li = terms[:, t, 0].long(), terms[:, t, 1].long()
        term = weights[:, t, None, None].double() * preds[slot.clamp_min(0), :, li.clamp_min(0)].double()
        term = torch.where((slot >= 0)[:, None, None], term, torch.zeros_like(term))
        v, mag = v + term, mag + term.abs()
    return v.permute(1, 0, 2), (2 * T * U * mag).permute(1, 0, 2)
