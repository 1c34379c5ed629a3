"""tests/block_cases.py on the CPU: every construction claim, every mutant caught, every emulation inside its bound.

The builders assert their own claims while they build (representable operands, every sum exact in float32, saturated gates,
tie shares, 40-bit margins, closed forms such as out == x + perm(v0 + 1) + bias_o, no more than 5 % of the (row, head) pairs
left out); this file builds every case on both element types, runs every mutant of the block's reference against every case
and every emulation of a legitimate design, and prints what the emulations leave.

No bound was chosen in advance: "bits" cases compare values of the element type for equality (block_cases.LEAK_TOL only where the
expected value is exactly 0), the two `tilted` cases allow one unit in the last place of the expected value.  The emulations
(float32 accumulation forwards, backwards and in two halves; the row sum from the rounded P; the scaled row maximum rounded on
its own; P normalised by a float32 reciprocal one ulp off either way; the two-part statistics finished in float32; the
block's own statistics at either end of the row-statistics bound) leave deviation 0 on
EVERY case of both element types, `tilted` included - the printed table; tests/test_gpu_blocks_exact.py quotes it.

Control (`old_bound_figures`, Gaussian problems of tests/test_gpu_kernels.py, (max|err|, relative L2) as fractions of the old
bounds; below 1 = let through):
                                                  bfloat16        float16
  audio  colsum of unrounded Kq                   0.33  0.17      0.04  0.02    (increment: 0.10 0.07 / 0.01 0.01)
  audio  output rounded twice                     0.33  0.33      0.04  0.04    (increment: 0.10 0.13 / 0.01 0.02)
  tblock pe added after the rounding of q/k/v     0.13  1.11      0.02  0.14
  tblock a padded key frame unmasked (f = 24)     1.46  18.4      1.45  18.3    - a Gaussian problem does catch this one:
  audio  a padded token slot counted              8.00  12.8      7.72  12.8      a 25th key / sixth token carries 4 % / 17 %
The old bounds let the rounding-class defects through on both element types and catch a whole extra key; what they cannot
do is say WHICH key, frame, head or column was wrong, nor visit the f = 24 tail, the padding slots and the packed columns
with operands that make a one-element mix-up visible.
"""
import pytest
import torch

import block_cases as B

FF_M = 256
TB_SHAPES = ((2, 16, 8), (2, 24, 4))
AX_SHAPES = ((320, 3, 16, 2), (640, 2, 48, 4), (1280, 2, 16, 2))       # (C, frames, rows per frame, statistics format)


def _cases(block, el):
    if block == "ff":
        return B.ff_cases(el, FF_M)
    if block == "tb":
        return [c for s in TB_SHAPES for c in B.tb_cases(el, *s)]
    return [c for (cd, fr, rpf, fmt) in AX_SHAPES for c in B.ax_cases(el, cd, fr, rpf, fmt=fmt)]


@pytest.fixture(scope="module")
def built():
    """(block, element type) -> cases; the builders' assertions run here."""
    return {(blk, el): _cases(blk, el) for blk in ("ff", "tb", "ax") for el in B.ELEMS}


@pytest.mark.parametrize("block", ["ff", "tb", "ax"])
def test_construction_claims(built, block):
    for el in B.ELEMS:
        for c in built[block, el]:
            assert c.conditions, c.name
            e = c.expected()
            assert bool(torch.isfinite(e).all()) and B.representable(e, el)
            assert not bool(c.wrong(e).any())
            print(f"[{block} {B.EL_NAME[el]} {c.shape}] {c.name}: " + "; ".join(c.conditions))


@pytest.mark.parametrize("block", ["ff", "tb", "ax"])
def test_every_mutant_is_caught_on_both_element_types(built, block):
    for el in B.ELEMS:
        caught = {m: [] for m in B.MUTANTS[block]}
        for c in built[block, el]:
            for m in B.MUTANTS[block]:
                n = int(c.wrong(c.forward(mut=m)).sum())
                if n:
                    caught[m].append(f"{c.name} {tuple(c.shape.values())}: {n}")
        for m, by in caught.items():
            print(f"[{block} {B.EL_NAME[el]}] {m}: caught by " + ("; ".join(by) if by else "NOTHING"))
        missed = [m for m, by in caught.items() if not by]
        assert not missed, f"{block} [{B.EL_NAME[el]}]: no case catches {missed}"


def test_what_each_case_pins(built):
    """The mutants a case is THERE for (the table in tests/test_gpu_blocks_exact.py), case by case."""
    must = {("ff", "signs"): ["bias1 in un-interleaved order", "mean * colsum dropped"],
            ("ff", "rounding (output)"): ["output rounded twice (before the residual)"],
            ("ff", "rounding (h)"): ["h not rounded before W2"],
            ("ff", "folded"): ["mean * colsum dropped", "mean * colsum applied with rstd outside"],
            ("tb", "counted"): ["the last frame or token dropped", "a padded key frame unmasked (f = 24)", "the neighbouring pixel's key and value",
                                "the neighbouring head's key and value"],
            ("tb", "routing (v from x)"): ["the neighbouring item's key and value", "the neighbouring pixel's key and value", "pe row of frame + 1",
                                           "pe row of frame - 1", "pe added after the rounding of q / k / v", "heads swapped in the out-projection input"],
            ("tb", "routing (q, k from x)"): ["the neighbouring item's key and value", "the neighbouring pixel's key and value",
                                              "the neighbouring head's key and value"],
            ("tb", "tilted"): ["scale from a head dim padded to 48", "scale from a head dim padded to 64", "a padded key frame unmasked (f = 24)"],
            ("tb", "dense v / out-projection"): ["heads swapped in the out-projection input", "mean * colsum dropped"],
            ("tb", "dense q"): ["mean * colsum dropped", "the neighbouring head's key and value"],
            ("tb", "dense k"): ["mean * colsum dropped", "the neighbouring pixel's key and value"],
            ("tb", "own statistics"): ["mean * colsum dropped", "the neighbouring pixel's key and value"],
            ("ax", "counted"): ["a padded token slot counted", "the last frame or token dropped", "colsum of unrounded Kq", "mean * colsum dropped"],
            ("ax", "routing"): ["the neighbouring item's key and value", "the neighbouring head's key and value", "alpha applied to the residual",
                                "bias_o outside alpha", "output rounded twice (before the residual)"],
            ("ax", "tilted"): ["scale from a head dim padded to 48", "scale from a head dim padded to 64"],
            ("ax", "dense out-projection"): ["heads swapped in the out-projection input", "bias_o outside alpha"]}
    for (blk, el), cases in built.items():
        for c in cases:
            for m in must[blk, c.name.split(" #")[0]]:
                if "(f = 24)" in m and c.shape.get("f") != 24:
                    continue
                assert bool(c.wrong(c.forward(mut=m)).any()), f"{blk} {c.name} {c.shape} [{B.EL_NAME[el]}] does not catch: {m}"


@pytest.mark.parametrize("f", [16, 24])
def test_dense_q_and_k_observe_every_projection_column(f):
    """The unit-vector tables of the dense q / dense k variants cover all 40 channels of every head (3 tables at f = 16, 2 at f
    = 24), and the reference mutant "q / k column n built from its neighbour in the head" - weight row, bias, column sum and
    table column, what a wrong tb_src_col would do - is caught for EVERY n of the 640, on both element types, by the variant
    whose table reads that channel."""
    nv = B.dense_variants(f)
    pos = torch.stack([B.unit_positions(f, v) for v in range(nv)])                  # [variant, frame, head]
    for h in range(B.HEADS):
        assert set(pos[:, :, h].flatten().tolist()) == set(range(B.TB_D)), f"head {h}: a channel is under no unit vector"
    b, hw = 1, 8 if f == 16 else 4
    for el in B.ELEMS:
        for wi, which in enumerate(("q", "k")):
            cases = B.tb_dense_cases(el, b, f, hw, which=(which,))
            for h in range(B.HEADS):
                for ch in range(B.TB_D):
                    v = next(v for v in range(nv) if ch in pos[v, :, h].tolist())
                    n = wi * B.TB_C + h * B.TB_D + ch
                    n2 = wi * B.TB_C + h * B.TB_D + (ch + 1) % B.TB_D
                    c = cases[v]
                    assert bool(c.wrong(c.forward(mut=("column", n, n2))).any()), \
                        f"{c.name} f={f} [{B.EL_NAME[el]}]: {which} column {n} (head {h} channel {ch}) built from column {n2} goes unnoticed"
    print(f"[tb f={f}] every one of the 640 q / k columns is observed: {nv} unit tables, the column mutant caught 640 times per element type")


@pytest.mark.parametrize("block", ["ff", "tb", "ax"])
def test_every_emulation_passes(built, block):
    for el in B.ELEMS:
        worst = {}
        for c in built[block, el]:
            emus = dict(B.EMULATIONS[block])
            if c.name == "own statistics":
                emus.update(B.TB_OWN_EMULATIONS)
            for name, emu in emus.items():
                got = c.forward(emu=emu)
                assert not bool(c.wrong(got).any()), f"{block} {c.name} {c.shape} [{B.EL_NAME[el]}]: the emulation '{name}' fails"
                worst[c.name] = max(worst.get(c.name, 0.0), c.deviation(got))
        print(f"[{block} {B.EL_NAME[el]}] largest |emulation - expected| per case: " +
              ", ".join(f"{k} {v:g}" + (" (of one unit allowed)" if k == "tilted" else "") for k, v in worst.items()))


def test_statistics_of_the_stored_rows(built):
    """block_cases.stats_of: float32 sums of the stored rows, lane order of the kernels or plain, stay inside the rule; the two
    halves swapped do not."""
    widest = {}
    for (blk, el), cases in built.items():
        if blk == "ff":
            continue
        for c in cases:
            st = c.expected()
            w_, t_ = B.stats_of(st, 0, 1e-5)
            widest[blk, B.EL_NAME[el]] = max(widest.get((blk, B.EL_NAME[el]), 0.0), float((t_[:, 1] / w_[:, 1]).max()))
            for parts in (0, 2):
                want, tol = B.stats_of(st, parts, 1e-5)
                s32 = st.to(torch.float32)
                if parts == 2:
                    v = s32.reshape(st.shape[0], 2, -1)
                    got = torch.stack([v.sum(2), (v * v).sum(2)], 2).reshape(-1, 4)
                    swapped, _ = B.stats_of(st, 2, 1e-5, mut=B.STATS_MUTANTS[0])
                    assert bool(((swapped - want).abs() > tol).any()), f"{blk} {c.name}: swapped halves go unnoticed"
                else:
                    inv = torch.tensor(1.0 / st.shape[1], dtype=torch.float32)
                    mean = s32.sum(1) * inv
                    var = ((s32 * s32).sum(1) * inv - mean * mean).clamp_min(0.0)
                    got = torch.stack([mean, 1.0 / torch.sqrt(var + 1e-5)], 1)
                assert bool(((got.double() - want).abs() <= tol).all()), f"{blk} {c.name} parts={parts}: float32 statistics outside the rule"
    print("widest relative rstd tolerance used (2^-16 = 1.53e-05): " + ", ".join(f"{k[0]} {k[1]} {v:.3g}" for k, v in widest.items()))


def test_old_bound_figures():
    """The control: what the Gaussian bounds let through (module docstring)."""
    for el in B.ELEMS:
        fig = B.old_bound_figures(el)
        for k, (mx, l2) in fig.items():
            print(f"[old bounds {B.EL_NAME[el]}] {k}: max|err| {mx:.3f}, relative L2 {l2:.3f} of the allowed")
        through = ["colsum of unrounded Kq", "output rounded twice (before the residual)"]
        through += ["audio increment: " + k for k in through]
        if el is torch.float16:
            through.append("pe added after the rounding of q / k / v")
        for k in through:
            assert max(fig[k]) < 1, (k, fig[k])
        assert fig["pe added after the rounding of q / k / v"][0] < 1 and fig["a padded key frame unmasked (f = 24)"][1] > 1
