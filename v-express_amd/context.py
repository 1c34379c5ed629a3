"""Sliding-window context scheduler + the host-side plan of the mean-overlap loop.

`uniform` reproduces the window lists of pipelines/context.py:22-60 (the AnimateDiff "uniform" schedule) - they are part
of the numerical contract, bit for bit - in its own formulation (round 3; rounds 1-2 carried a transcription): the
schedule is a set of dilation levels d = 1, 2, 4, ...; on each level windows of `context_size` frames spaced d apart
start every `context_size * d - context_overlap` frames from an offset given by the base-2 radical inverse of `step`,
and a frame index that runs past the clip is reflected to `F - 2 - (e mod F)`.  The pipeline only ever asks for
step = 0, context_stride = 1, closed_loop = False (pipelines/v_express_pipeline.py:471-481): one level, starts
0, s, 2s, ... with s = context_size - context_overlap while start < F - context_overlap.  Asserted identical to the
reference module for a grid of parameters (tests/golden/windows.pt, tests/test_oracle_vs_reference.py).
`overlap_plan` turns the per-window bookkeeping of pipelines/v_express_pipeline.py:498-500,552-572
into a static table the device kernels consume: for every frame, which (window, position) predictions make up
its averaged noise prediction and by what count they are divided - including the reference's behaviour for a
reflected last window with duplicate frame ids: the count is incremented once, the
duplicated frame is stepped twice and the LAST write wins.
"""
from typing import Callable, List

import numpy as np


def radical_inverse_base2(val: int) -> float:
    """The 64-bit bit-reversal of `val` as a fraction in [0, 1) (van der Corput sequence): 0, 1/2, 1/4, 3/4, ..."""
    rev = 0
    for _ in range(64):
        rev = (rev << 1) | (val & 1)
        val >>= 1
    return rev / float(1 << 64)


ordered_halving = radical_inverse_base2          # the reference's name for it (pipelines/context.py:14-19)


def uniform(step: int = ..., num_frames: int = ..., context_size: int = None, context_stride: int = 3,
            context_overlap: int = 4, closed_loop: bool = True):
    """Generator of frame-index lists, one per context window (see the module docstring)."""
    F = num_frames
    if F <= context_size:
        yield list(range(F))
        return
    phase = radical_inverse_base2(step)
    shift = int(round(F * phase))
    levels = min(context_stride, int(np.ceil(np.log2(F / context_size))) + 1)
    last_start = F + shift - (0 if closed_loop else context_overlap)       # exclusive bound of the window starts
    for level in range(levels):
        d = 1 << level
        first = int(phase * d) + shift
        hop = context_size * d - context_overlap
        for start in range(first, last_start, hop):
            frames = start + d * np.arange(context_size)
            frames = np.where(frames >= F, F - 2 - frames % F, frames)     # reflection past the end of the clip
            yield [int(e) for e in frames]


def uniform_fit(step: int = ..., num_frames: int = ..., context_size: int = None, context_stride: int = 3,
                context_overlap: int = 4, closed_loop: bool = True):
    """Generator of frame-index lists like `uniform`, for any clip length: as many windows as `uniform`'s single level,
    every one `context_size` consecutive in-range frames, their starts spread evenly over the clip,
    s_k = (k * (F - f)) // (n - 1) with n = ceil((F - o) / (f - o)) - no reflected window, no duplicate frame, and
    consecutive windows overlap by at least `context_overlap`.  For F <= f or (F - f) % (f - o) == 0 the list is
    `uniform(step=0, context_stride=1, closed_loop=False)`'s.  `step`, `context_stride` and `closed_loop` are accepted
    for the shared signature and ignored: the windows do not move with the timestep, have one level and are not closed.
    The reference has no counterpart: inference.py cuts the clip to an aligned length instead (aligned_video_length)."""
    F, f, o = num_frames, context_size, context_overlap
    if F <= f:
        yield list(range(F))
        return
    hop = f - o
    n = -((o - F) // hop)                                                  # ceil((F - o) / hop) >= 2
    for k in range(n):
        start = (k * (F - f)) // (n - 1)
        yield list(range(start, start + f))


def get_context_scheduler(name: str) -> Callable:
    if name == "uniform":
        return uniform
    if name == "uniform_fit":
        return uniform_fit
    raise ValueError(f"Unknown context_overlap policy {name}")


def compute_num_context(init_video_length, context_size, context_overlap):
    """pipelines/context.py:7-11."""
    return (init_video_length - context_size) // (context_size - context_overlap) + 1


def aligned_video_length(init_video_length, context_size, context_overlap):
    """inference.py:255-264: the clip length inference.py actually requests (whole windows only)."""
    n = compute_num_context(init_video_length, context_size, context_overlap)
    return (n - 1) * (context_size - context_overlap) + context_size


def overlap_plan(windows: List[List[int]], num_frames: int):
    """Static plan of one timestep of the mean-overlap loop.

    Returns dict(counts[F], terms: {frame: [(window, latent_idx), ...]}, step_frames: ordered frame list,
    max_terms).  `terms[frame]` are the predictions summed (each divided by counts[frame]) into the value the
    frame's DDIM step finally keeps, replaying v_express_pipeline.py:552-572 symbolically."""
    counts = np.zeros(num_frames, dtype=np.int64)
    for w in windows:
        counts[np.unique(np.asarray(w))] += 1          # tensor index_put: duplicates count once (:498-500)
    counter = np.zeros(num_frames, dtype=np.int64)
    pending = [None] * num_frames
    final = {}
    for wi, w in enumerate(windows):
        counter[np.unique(np.asarray(w))] += 1         # :552
        for li, fi in enumerate(w):                     # :556-564
            if pending[fi] is None:
                pending[fi] = [(wi, li)]
            else:
                pending[fi] = pending[fi] + [(wi, li)]
            if counter[fi] == counts[fi]:
                final[fi] = pending[fi]                 # stepped now; a later duplicate overwrites (:572)
                pending[fi] = None
    leftover = [i for i in range(num_frames) if i not in final]
    if leftover:
        raise ValueError(f"frames {leftover[:8]} are never completed by the window schedule")
    step_frames = sorted(final)
    return dict(counts=counts, terms=final, step_frames=step_frames,
                max_terms=max(len(v) for v in final.values()))


BLEND_NAMES = ("mean", "linear", "pyramid")
_FIT_HINT = 'context_schedule="uniform_fit" gives such windows for any clip length'


def check_blend(blend, window_length=None):
    """Validates `overlap_blend` (ValueError); returns its kind: "mean" (also for None), "linear", "pyramid" or "profile"
    (a sequence of `window_length` finite positive numbers, one weight per window position)."""
    if blend is None:
        return "mean"
    if isinstance(blend, str):
        if blend not in BLEND_NAMES:
            raise ValueError(f"unknown overlap_blend {blend!r}: one of {BLEND_NAMES} or a per-position weight profile")
        return blend
    try:
        prof = np.asarray([float(v) for v in blend], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"overlap_blend must be one of {BLEND_NAMES} or a sequence of numbers, got {blend!r}") from None
    if window_length is not None and prof.shape[0] != window_length:
        raise ValueError(f"an overlap_blend profile has one weight per window position: {window_length} expected, got "
                         f"{prof.shape[0]}")
    if prof.shape[0] == 0 or not (np.isfinite(prof).all() and (prof > 0).all()):
        raise ValueError("an overlap_blend profile must hold finite positive numbers only")
    return "profile"


def blend_weights(windows: List[List[int]], blend):
    """Raw (not yet normalised) weights of a weighted window blend, float64 [windows, f]: weight[k][j] is what window k's
    prediction of its j-th frame counts for.  blend = "pyramid": min(j + 1, f - j) (AnimateDiff front ends' name);
    a sequence of f finite positive numbers: that profile for every window; "linear": a cross-fade over the actual
    overlap with each neighbour - with L_k = f - (s_k - s_{k-1}) frames shared with the window before (0 for the first)
    and R_k = f - (s_{k+1} - s_k) with the one after (0 for the last), min(1, (j + 1) / (L_k + 1), (f - j) / (R_k + 1)),
    so that where exactly two windows overlap their weights sum to 1.  Every weighted blend needs windows without a
    duplicate frame, "linear" ascending contiguous runs listed by increasing start: a reflected last window of `uniform`
     is given no weighted meaning."""
    kind = check_blend(blend, len(windows[0]))
    if kind == "mean":
        raise ValueError('blend_weights: "mean" is the unweighted route (overlap_plan)')
    f = len(windows[0])
    if any(len(w) != f for w in windows):
        raise ValueError("all context windows must have the same length")
    for k, w in enumerate(windows):
        if len(set(w)) != f:
            raise ValueError(f"overlap_blend={kind!r} needs windows without duplicate frames, window {k} is {list(w)} "
                             f"(a reflected last window); {_FIT_HINT}")
    if kind == "pyramid":
        row = np.minimum(np.arange(f) + 1, f - np.arange(f)).astype(np.float64)
        return np.tile(row, (len(windows), 1))
    if kind == "profile":
        return np.tile(np.asarray([float(v) for v in blend], dtype=np.float64), (len(windows), 1))
    starts = [w[0] for w in windows]
    for k, w in enumerate(windows):
        if list(w) != list(range(w[0], w[0] + f)) or (k and starts[k] <= starts[k - 1]):
            raise ValueError(f'overlap_blend="linear" needs every window to be an ascending contiguous run, listed by '
                             f"increasing start; window {k} is {list(w)}; {_FIT_HINT}")
    j = np.arange(f, dtype=np.float64)
    raw = np.ones((len(windows), f), dtype=np.float64)
    for k in range(len(windows)):
        left = max(f - (starts[k] - starts[k - 1]), 0) if k else 0
        right = max(f - (starts[k + 1] - starts[k]), 0) if k + 1 < len(windows) else 0
        if left:
            raw[k] = np.minimum(raw[k], (j + 1) / (left + 1))
        if right:
            raw[k] = np.minimum(raw[k], (f - j) / (right + 1))
    return raw


def weighted_overlap_plan(windows: List[List[int]], num_frames: int, raw):
    """Static plan of the weighted blend of one timestep (vx_overlap_blend): every frame's prediction is the sum over the
    windows that hold it, in ascending window order, of weight * prediction, the weights of a frame normalised to sum 1.

    Returns dict(step_frames: all frames, ascending; terms: {frame: [(window, latent_idx), ...]}; max_terms;
    weights: float32 [F, max_terms] = raw / sum(raw of the frame), formed in float64 and rounded once - a frame of one
    term gets exactly 1; term_table: int32 [F, max_terms, 2], the terms in order, padded with -1 (weight 0))."""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.shape != (len(windows), len(windows[0])):
        raise ValueError(f"raw weights must be [windows, f] = {[len(windows), len(windows[0])]}, got {list(raw.shape)}")
    terms = {i: [] for i in range(num_frames)}
    for wi, w in enumerate(windows):
        if len(set(w)) != len(w):
            raise ValueError(f"a weighted blend needs windows without duplicate frames, window {wi} is {list(w)}; "
                             f"{_FIT_HINT}")
        for li, fi in enumerate(w):
            terms[fi].append((wi, li))
    leftover = [i for i in range(num_frames) if not terms[i]]
    if leftover:
        raise ValueError(f"frames {leftover[:8]} are never completed by the window schedule")
    max_terms = max(len(v) for v in terms.values())
    weights = np.zeros((num_frames, max_terms), dtype=np.float32)
    table = np.full((num_frames, max_terms, 2), -1, dtype=np.int32)
    for i in range(num_frames):
        r = np.array([raw[wi, li] for wi, li in terms[i]], dtype=np.float64)
        weights[i, :len(r)] = (r / r.sum()).astype(np.float32)
        table[i, :len(r)] = terms[i]
    return dict(step_frames=list(range(num_frames)), terms=terms, max_terms=max_terms, weights=weights,
                term_table=table)
