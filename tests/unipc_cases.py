"""Exact-answer cases for `vx_overlap_unipc_step` (TEST INFRASTRUCTURE) for tests/test_unipc_cases_cpu.py and
tests/test_gpu_unipc.py: small-integer inputs and dyadic coefficients, so that every intermediate of the kernel's
expression is a small multiple of 2^-9 - exact in float32 whatever the order of the sums and whether or not a product and
a sum are contracted - and the float64 `reference` is the float32 answer bit for bit.  `MUTANTS` are the ways the kernel
can go wrong that the cases exist to catch; each must change the answer of at least one case.

A case holds numpy arrays: latents [1, C, F, h, w], preds [nW, C, f, hw], terms int32 [n, T, 2], frame_ids int32 [n],
counts [n], history [3, C, F, h, w], saved [1, C, F, h, w] (float32) and `coef`, the sixteen fields of
v_express_amd.scheduler.UniPCStep.  History slots and saved samples that the update must not read hold NaN."""
import numpy as np

FIELDS = "h1 h2 h3 h_write use_c a_i s_i q_s q_m q_1 q_2 q_3 k_x k_m k_1 k_2".split()
# dyadic, all different, none 0 or 1: a swapped pair or a skipped term changes the answer
SCALARS = dict(a_i=0.5, s_i=0.25, q_s=1.5, q_m=-0.25, q_1=0.75, q_2=-0.5, q_3=1.25, k_x=-0.75, k_m=1.75, k_1=0.5, k_2=-1.5)

MUTANTS = ("m_from_xc", "saved_is_x", "saved_is_out", "corrector_skipped", "predictor_from_x", "write_before_read",
           "h1_h2_swapped", "minus_one_slot_read", "count_ignored", "frame_ids_ignored")


def _coef(h1, h2, h3, h_write, use_c):
    return tuple([h1, h2, h3, h_write, use_c] + [SCALARS[k] for k in FIELDS[5:]])


def _plan_two_windows():
    """frame_ids [1, 3, 4] of F = 5 over two windows of f = 3, max_terms 2: frame 1 has one term and a -1 pad after it,
    frame 3 two terms (count 2), frame 4 a -1 pad BEFORE its one term (the first valid term starts the sum)."""
    terms = np.array([[[0, 1], [-1, -1]], [[0, 2], [1, 0]], [[-1, -1], [1, 1]]], dtype=np.int32)
    return dict(F=5, f=3, nW=2, frame_ids=np.array([1, 3, 4], dtype=np.int32), terms=terms,
                counts=np.array([1.0, 2.0, 1.0], dtype=np.float32))


def _plan_trivial(F, frame_ids):
    """One "window" that holds every frame (the plan of the weighted blend): one term, count 1."""
    ids = np.array(frame_ids, dtype=np.int32)
    terms = np.stack([np.zeros_like(ids), ids], axis=1).reshape(-1, 1, 2).astype(np.int32)
    return dict(F=F, f=F, nW=1, frame_ids=ids, terms=terms, counts=np.ones(len(ids), dtype=np.float32))


def _case(name, plan, C, h, w, coef, seed):
    rng = np.random.default_rng(seed)
    F_ = plan["F"]

    def ints(*shape, lo=-3, hi=4):
        return rng.integers(lo, hi, size=shape).astype(np.float32)
    h1, h2, h3, h_write, use_c = coef[:5]
    history = ints(3, C, F_, h, w)
    for slot in range(3):
        if slot not in (h1, h2, h3 if use_c else -1):
            history[slot] = np.nan                      # never written, or only written by this update: not to be read
    saved = ints(1, C, F_, h, w) if use_c else np.full((1, C, F_, h, w), np.nan, dtype=np.float32)
    return dict(name=name, C=C, F=F_, h=h, w=w, coef=coef, latents=ints(1, C, F_, h, w),
                preds=2.0 * ints(plan["nW"], C, plan["f"], h * w), terms=plan["terms"], frame_ids=plan["frame_ids"],
                counts=plan["counts"], history=history, saved=saved)


def cases():
    """The first update of a run (no corrector, no history read, coefficients on the absent slots all the same), second
    order (one slot), third order (three slots, the written one read by the same update), third-order predictor with the
    corrector disabled; hw = 4 and 12 over the two-window plan, and 320 threads (5 frames x 4 channels x hw 64: two blocks,
    the second one with a tail) over the trivial plan."""
    two = _plan_two_windows()
    out = []
    for hw_name, (h, w) in (("hw4", (2, 2)), ("hw12", (2, 6))):
        out += [_case(f"first_{hw_name}", two, 4, h, w, _coef(-1, -1, -1, 0, 0), 1),
                _case(f"order2_{hw_name}", two, 4, h, w, _coef(0, -1, -1, 1, 1), 2),
                _case(f"order3_{hw_name}", two, 4, h, w, _coef(2, 1, 0, 0, 1), 3),
                _case(f"predictor3_no_corrector_{hw_name}", two, 4, h, w, _coef(1, 0, -1, 2, 0), 4)]
    out.append(_case("order3_320_threads", _plan_trivial(7, [0, 2, 3, 5, 6]), 4, 8, 8, _coef(0, 2, 1, 1, 1), 5))
    return out


def reference(case, mutant=None):
    """(latents, history, saved) after the update, float64 arithmetic in the kernel's form; with `mutant` one of MUTANTS,
    what a kernel with that fault would leave."""
    assert mutant is None or mutant in MUTANTS
    h1, h2, h3, h_write, use_c = case["coef"][:5]
    a_i, s_i, q_s, q_m, q_1, q_2, q_3, k_x, k_m, k_1, k_2 = case["coef"][5:]
    lat, hist, saved = (case[k].astype(np.float64) for k in ("latents", "history", "saved"))
    preds, C = case["preds"].astype(np.float64), case["C"]
    hw = case["h"] * case["w"]
    if mutant == "h1_h2_swapped":
        h1, h2 = h2, h1
    if mutant == "corrector_skipped":
        use_c = 0

    def slot_of(s):
        return max(s, 0) if mutant == "minus_one_slot_read" else s
    new_lat, new_hist, new_saved = lat.copy(), hist.copy(), saved.copy()
    for k, fr in enumerate(case["frame_ids"].tolist()):
        if mutant == "frame_ids_ignored":
            fr = k
        v = None
        for slot, li in case["terms"][k].tolist():
            if slot < 0:
                continue
            term = preds[slot, :, li].reshape(C, case["h"], case["w"])
            if mutant != "count_ignored":
                term = term / float(case["counts"][k])
            v = term if v is None else v + term
        assert v is not None and v.size == C * hw
        x = lat[0, :, fr]
        H = hist[:, :, fr]
        if mutant == "write_before_read" and h_write >= 0:
            H = H.copy()
            H[h_write] = a_i * x - s_i * v
        m = a_i * x - s_i * v
        xc = x
        if use_c:
            xc = q_s * saved[0, :, fr] + q_m * m
            for s, q in ((h1, q_1), (h2, q_2), (h3, q_3)):
                if slot_of(s) >= 0:
                    xc = xc + q * H[slot_of(s)]
            if mutant == "m_from_xc":
                m = a_i * xc - s_i * v
        out = k_x * (x if mutant == "predictor_from_x" else xc) + k_m * m
        for s, kk in ((h1, k_1), (h2, k_2)):
            if slot_of(s) >= 0:
                out = out + kk * H[slot_of(s)]
        new_saved[0, :, fr] = {"saved_is_x": x, "saved_is_out": out}.get(mutant, xc)
        if h_write >= 0:
            new_hist[h_write, :, fr] = m
        new_lat[0, :, fr] = out
    return new_lat, new_hist, new_saved


def same_bits(a, b):
    """Two arrays hold the same float32 bits (NaNs compare by payload; +0 and -0 differ)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())
