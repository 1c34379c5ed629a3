"""Adaptive projected guidance on the MI355X: `vx_guidance_apg` (both element libraries; the code is float32 in both)
on inputs whose answer is exact, against the float64 restatement under the derived elementwise bound, its independence of
the exchange layout, its argument errors and guard bands, and VExpressPipeline with `apg_eta` against the restated loop
over the oracle UNet (tests/apg_restated.py)."""
import pytest
import torch

import apg_restated as AP
import cases
from loop_restated import restated_loop
from loop_worker import call_small, cosine, dev, oracle_on_cpu, rel_l2, scheduler, small  # noqa: F401

pytestmark = pytest.mark.gpu

ELEMS = [torch.bfloat16, torch.float16]
# the real window; two windows of one ragged chunk; a full chunk of 256 pixels plus a tail
SHAPES = [(1, 4, 16, 4096), (2, 4, 6, 80), (1, 4, 3, 1040)]
S, S_A = 3.5, 6.0


def layout(rows, granules, seed, spare=3):
    """tests/test_gpu_audio_guidance.py's `layout`: the rows [nW, c, f, hw] as an all-gathered unit buffer of `granules`
    frame granules per unit, scattered by a seeded permutation, with `spare` unused, NaN-filled slots:
    (gathered [slots, (f/G) hw, c], unit_index int32 [nW, len(rows), G])."""
    nW, c, f, hw = rows[0].shape
    fl = f // granules
    n = nW * len(rows) * granules
    perm = torch.randperm(n + spare, generator=torch.Generator().manual_seed(seed))[:n]
    gathered = torch.full((n + spare, fl * hw, c), float("nan"))
    uidx = torch.empty((nW, len(rows), granules), dtype=torch.int32)
    k = 0
    for w in range(nW):
        for r, x in enumerate(rows):
            for j in range(granules):
                slot = int(perm[k])
                k += 1
                uidx[w, r, j] = slot
                gathered[slot] = x[w, :, j * fl:(j + 1) * fl].permute(1, 2, 0).reshape(fl * hw, c)
    return gathered, uidx


def run(ops, dev, rows, s=S, s_a=S_A, eta=0.0, r=0.0, beta=0.0, prev=None, granules=1, seed=0):
    """One ops.guidance_apg call on the rows (2 or 3 tensors [nW, c, f, hw]) with a NaN-poisoned workspace; prev: the
    momentum buffers' contents [rows - 1, nW, c, f, hw] (zeros by default).  Returns (preds, momentum buffers or None)."""
    nW, c, f, hw = rows[0].shape
    gathered, uidx = layout(rows, granules, seed)
    ws = torch.full((ops.guidance_apg_ws_floats(nW, len(rows), f, hw),), float("nan"), device=dev)
    preds = torch.full((nW, c, f, hw), float("nan"), device=dev)
    buf = None
    if beta != 0.0:
        buf = torch.zeros((len(rows) - 1, nW, c, f, hw), device=dev) if prev is None else prev.to(dev).clone()
    ops.guidance_apg(gathered.to(dev), uidx.to(dev), c, f, hw, s, s_a, eta, r, beta, buf, ws, preds)
    torch.cuda.synchronize()
    return preds.cpu(), None if buf is None else buf.cpu()


def combine(ops, dev, rows, s):
    """vx_combine_units on two rows."""
    nW, c, f, hw = rows[0].shape
    gathered, uidx = layout(rows, 1, 1)
    preds = torch.full((nW, c, f, hw), float("nan"), device=dev)
    ops.combine_units(gathered.to(dev), uidx.to(dev), c, f, hw, s, preds)
    torch.cuda.synchronize()
    return preds.cpu()


def predictions(nW, c, f, hw, mean, seed):
    """u ~ N(mean, 1), m = u + 0.3 N(0, 1), c = m + 0.3 N(0, 1): float32 [nW, c, f, hw] each."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(nW, c, f, hw, generator=g) + mean
    m = u + 0.3 * torch.randn(nW, c, f, hw, generator=g)
    return u, m, m + 0.3 * torch.randn(nW, c, f, hw, generator=g)


def signs(nW, c, f, hw):
    """+1 / -1 alternating by pixel, the same for every channel and frame (hw is even: every frame sums to zero)."""
    assert hw % 2 == 0
    return (1.0 - 2.0 * (torch.arange(hw) % 2)).float().expand(nW, c, f, hw).contiguous()


# ------------------------------------------------------------------------------------------------ exact answers
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_answers(dev, elem, shape):
    """Small integers (and halves), so that every sum, quotient and coefficient is exact and the answer is known to the
    bit."""
    from v_express_amd import lib as L, ops
    with L.element_type(elem):
        # u == c bitwise: no difference, g == c whatever the parameters, and the momentum stays zero
        _, _, c = predictions(*shape, 3.0, seed=1)
        for kw in (dict(s=3.5, eta=0.0), dict(s=7.5, eta=0.3, r=0.5), dict(s=12.0, eta=1.0, r=2.5, beta=-0.75)):
            got, buf = run(ops, dev, (c.clone(), c), **kw)
            assert torch.equal(got, c), kw
            assert buf is None or not buf.any()
        got, _ = run(ops, dev, (c.clone(), c.clone(), c), eta=0.3, r=0.5)
        assert torch.equal(got, c)
        # orthogonal: c = 1, d = +-1 alternating by pixel, so S_dc = 0 and k = 0; nothing to remove, no cap: the CFG bits
        one, d = torch.ones(shape), signs(*shape)
        got, _ = run(ops, dev, (one - d, one), eta=0.0)
        assert torch.equal(got, one + (S - 1.0) * d) and torch.equal(got, combine(ops, dev, (one - d, one), S))
        # parallel: c = +-1, u = -c, so d = 2 c and k = 2: eta = 0 removes all of it, eta = 1 keeps the CFG bits 6 c
        got, _ = run(ops, dev, (-d, d), eta=0.0)
        assert torch.equal(got, d)
        got, _ = run(ops, dev, (-d, d), eta=1.0)
        assert torch.equal(got, 6.0 * d) and torch.equal(got, combine(ops, dev, (-d, d), S))
        # momentum: beta = -0.5 on a buffer that holds d: dbar = d / 2, stored; g = 1 +- 1.25
        got, buf = run(ops, dev, (one - d, one), eta=0.0, beta=-0.5, prev=d[None])
        assert torch.equal(buf[0], 0.5 * d) and torch.equal(got, one + 1.25 * d)


@pytest.mark.parametrize("elem", ELEMS)
def test_exact_cap(dev, elem):
    """The orthogonal case at c * hw = 64, so |d| = 8 per frame: r = 2 gives phi = 1 / 4 and g = 1 +- 0.625 at s = 3.5;
    r = 8 and r = 16 do not bite."""
    from v_express_amd import lib as L, ops
    shape = (2, 4, 3, 16)
    one, d = torch.ones(shape), signs(*shape)
    with L.element_type(elem):
        got, _ = run(ops, dev, (one - d, one), eta=0.0, r=2.0)
        assert torch.equal(got, one + 0.625 * d)
        for r in (8.0, 16.0):
            got, _ = run(ops, dev, (one - d, one), eta=0.0, r=r)
            assert torch.equal(got, one + 2.5 * d), r


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_three_rows_with_two_equal_rows_are_the_two_row_launch(dev, elem, shape):
    from v_express_amd import lib as L, ops
    u, m, c = predictions(*shape, 3.0, seed=2)
    prev = 0.3 * torch.randn((1,) + shape, generator=torch.Generator().manual_seed(3))
    zero = torch.zeros_like(prev)
    kw = dict(eta=0.3, r=5.0, beta=-0.5)
    with L.element_type(elem):
        # m == c: the second difference is zero and stays zero
        three, b3 = run(ops, dev, (u, c.clone(), c), prev=torch.cat([prev, zero]), seed=4, **kw)
        two, b2 = run(ops, dev, (u, c), s=S, prev=prev, seed=5, **kw)
        assert torch.isfinite(two).all() and torch.equal(three, two)
        assert torch.equal(b3[0], b2[0]) and not b3[1].any()
        # u == m: the first difference is zero, the second one guided by s_a
        three, b3 = run(ops, dev, (m.clone(), m, c), prev=torch.cat([zero, prev]), seed=6, **kw)
        two, b2 = run(ops, dev, (m, c), s=S_A, prev=prev, seed=7, **kw)
        assert torch.isfinite(two).all() and torch.equal(three, two)
        assert torch.equal(b3[1], b2[0]) and not b3[0].any()


# ------------------------------------------------------------------------------------------------ against float64
PARAMS = [dict(s=3.5, eta=0.0), dict(s=7.5, eta=0.0, r=5.0, beta=-0.5), dict(s=12.0, eta=0.0, r=2.5, beta=-0.75),
          dict(s=3.5, eta=0.6, r=40.0, beta=0.25)]


def against_float64(apg, rows, kw, prev):
    """max over the elements of |err| / bound * K for one call `apg(rows, prev=..., **kw) -> (preds, buffers)`; also
    checks the stored momentum (two roundings)."""
    kw = dict(kw)
    beta, s_a = kw.get("beta", 0.0), kw.setdefault("s_a", S_A)
    scales = (kw["s"], s_a)[:len(rows) - 1]
    p = None if beta == 0.0 else list(prev[:len(rows) - 1])
    ref, dbars, ratios = AP.project(rows, scales, kw["eta"], kw.get("r", 0.0), beta, p, (1, 3))
    got, buf = apg(rows, prev=None if p is None else torch.stack(p), **kw)
    assert torch.isfinite(got).all()
    if p is not None:
        for j, dbar in enumerate(dbars):
            mag = (rows[j + 1].double() - rows[j].double()).abs() + (beta * p[j].double()).abs() + dbar.abs()
            assert bool(((buf[j].double() - dbar).abs() <= 2.0 ** -23 * mag).all())
    return ((got.double() - ref).abs() / AP.bound(rows, scales, beta, p, dbars, ratios)).max().item() * AP.K


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("mean", [0.0, 3.0, 30.0])
@pytest.mark.parametrize("shape", SHAPES + [(2, 3, 2, 300)])
def test_apg_vs_float64(dev, elem, mean, shape):
    """|err| <= K 2^-24 (|c| + sum |s - 1| (|d| + |beta dbar_prev| + |dbar| + sqrt(S_dd / S_cc) |c|)), K = 64
    (apg_restated.bound), two rows and three; (2, 3, 2, 300) runs the kernel of c != 4."""
    from v_express_amd import lib as L, ops
    rows = predictions(*shape, mean, seed=int(mean) + shape[2])
    prev = 0.3 * torch.randn((2,) + shape, generator=torch.Generator().manual_seed(7))
    worst = 0.0
    with L.element_type(elem):
        for kw in PARAMS:
            for xs in ((rows[0], rows[2]), rows):
                worst = max(worst, against_float64(lambda r_, **k: run(ops, dev, r_, **k), xs, kw, prev))
    print(f"[vx_guidance_apg {elem}, {shape}, mean {mean}] max |err| / (2^-24 magnitude) = {worst:.3g} (bound {AP.K})")
    assert worst <= AP.K


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("shape", [(2, 4, 8, 1040), (2, 4, 4, 80)])
def test_results_do_not_depend_on_the_layout(dev, elem, shape):
    """Granules 1 / 2 / 4 scattered by a seeded permutation (NaN in the spare slots), one launch of two windows against
    two of one; the workspace is NaN-poisoned in every run."""
    from v_express_amd import lib as L, ops
    rows3 = predictions(*shape, 3.0, seed=5)
    prev = 0.3 * torch.randn((2,) + shape, generator=torch.Generator().manual_seed(8))
    kw = dict(eta=0.25, r=5.0, beta=-0.5)
    with L.element_type(elem):
        for rows in ((rows3[0], rows3[2]), rows3):
            p = prev[:len(rows) - 1]
            one, buf = run(ops, dev, rows, prev=p, granules=1, seed=1, **kw)
            assert torch.isfinite(one).all() and torch.isfinite(buf).all()
            for granules in (2, 4):
                got, b = run(ops, dev, rows, prev=p, granules=granules, seed=10 + granules, **kw)
                assert torch.equal(one, got) and torch.equal(buf, b), granules
            for w in range(2):
                got, b = run(ops, dev, tuple(x[w:w + 1] for x in rows), prev=p[:, w:w + 1], granules=2, seed=20 + w, **kw)
                assert torch.equal(got[0], one[w]) and torch.equal(b[:, 0], buf[:, w]), w


# ------------------------------------------------------------------------------------------------ errors, guard bands
@pytest.mark.parametrize("elem", ELEMS)
def test_kernel_argument_errors(dev, elem):
    from v_express_amd import lib as L, ops
    u, _, c = predictions(1, 4, 4, 16, 0.0, seed=1)
    gathered, uidx = layout((u, c), 1, 0)
    gathered, uidx = gathered.to(dev), uidx.to(dev)
    ws = torch.zeros(ops.guidance_apg_ws_floats(1, 2, 4, 16), device=dev)
    preds, buf = torch.zeros(1, 4, 4, 16, device=dev), torch.zeros(1, 1, 4, 4, 16, device=dev)
    with L.element_type(elem):
        AP.check_argument_errors(L.current(), gathered.data_ptr(), uidx.data_ptr(), buf.data_ptr(), ws.data_ptr(),
                                 preds.data_ptr())
        with pytest.raises(ValueError, match="momentum_buf"):
            ops.guidance_apg(gathered, uidx, 4, 4, 16, S, S_A, 0.0, 0.0, -0.5, None, ws, preds)
        with pytest.raises(ValueError, match="workspace"):
            ops.guidance_apg(gathered, uidx, 4, 4, 16, S, S_A, 0.0, 0.0, 0.0, None, ws[:-1], preds)
    torch.cuda.synchronize()
    assert not preds.any() and not buf.any()                       # nothing was launched


@pytest.mark.parametrize("hw", [80, 1040])
@pytest.mark.parametrize("c", [4, 3])
def test_guard_bands(dev, hw, c):
    """tests/test_gpu_guard_bands.py's sweep on vx_guidance_apg, two rows and three: nothing is written outside preds, the
    momentum buffers and the workspace (at exactly vx_guidance_apg_ws_floats), and nothing outside gathered / unit_index
    is depended on (three runs with the outside zero / NaN / huge, bit-equal)."""
    from test_gpu_guard_bands import F32, G, O, Out, sweep
    from v_express_amd import lib as L, ops
    nW, f, gran = 2, 4, 2
    rows3 = predictions(nW, c, f, hw, 3.0, seed=hw + c)
    prev = 0.3 * torch.randn((2, nW, c, f, hw), generator=torch.Generator().manual_seed(9))
    with L.element_type(torch.bfloat16):
        for rows in ((rows3[0], rows3[2]), rows3):
            n_ws = ops.guidance_apg_ws_floats(nW, len(rows), f, hw)
            assert n_ws == nW * f * -(-hw // 256) * (2 * len(rows) - 1)
            gathered, uidx = layout(rows, gran, seed=len(rows))
            gg, gi = G(torch.nan_to_num(gathered), F32), G(uidx, torch.int32)
            preds, ws = O((nW, c, f, hw), F32), O((n_ws,), F32)
            buf, p = O((len(rows) - 1, nW, c, f, hw), F32), prev[:len(rows) - 1]
            got, _, b = sweep(f"guidance_apg rows={len(rows)}", [gg, gi], [preds, Out(ws, finite=False), Out(buf, init=p)],
                              lambda: ops.guidance_apg(gg.view, gi.view, c, f, hw, S, S_A, 0.25, 5.0, -0.5, buf.view,
                                                       ws.view, preds.view))
            scales = (S, S_A)[:len(rows) - 1]
            ref, dbars, ratios = AP.project(rows, scales, 0.25, 5.0, -0.5, list(p), (1, 3))
            assert bool(((got.cpu().double() - ref).abs() <= AP.bound(rows, scales, -0.5, list(p), dbars, ratios)).all())
            assert bool(((b.cpu().double() - torch.stack(dbars)).abs() <= 1e-5).all())


# ------------------------------------------------------------------------------------------------ the pipeline
R_CAP, BETA, END = 1.0, -0.5, 0.6          # r: the norms of the small clip's differences per frame lie on both sides of it
_PLAIN_REF = {}


def _call(S_, steps, **kw):
    return call_small(S_, scheduler("ddim"), steps, **kw)


def _windows(small):
    from oracle import loop as OL
    return OL.uniform_windows(small["F"], small["cf"], small["co"])


def _plain_ref(small, steps, s_a):
    """The restated loop without APG (guidance_end END), computed once per route."""
    if s_a not in _PLAIN_REF:
        inp = small["inp"]
        with oracle_on_cpu():
            _PLAIN_REF[s_a] = restated_loop(small["oracle"], inp["latents"], _windows(small), S, inp["kps_features"],
                                            inp["audio_embeddings"], steps, "ddim", s_a=s_a, end=END)
    return _PLAIN_REF[s_a]


@pytest.mark.parametrize("s_a", [None, S_A], ids=["two_rows", "three_rows"])
def test_pipeline_vs_restated_oracle_loop(small, s_a):
    """reflected_F11_c4o2, 5 DDIM steps of which 3 are guided, eta 0, r = 1 (it bites on some frames and not on others),
    beta -0.5.  e_plain: the plain clip against the plain restated loop.  The APG clip lies within 2 e_plain of the APG
    restated loop (the projection coefficient's error is a second term of the size of the difference's own), within the
    loop bound of tests/test_gpu_guidance.py (relative L2 5e-2, cosine 0.998), and closer to it than the plain clip.
    Measured on the MI355X: two rows relL2 4.89e-3 (e_plain 6.11e-3), three rows 7.01e-3 (e_plain 8.74e-3)."""
    steps, inp = 5, small["inp"]
    audio = {} if s_a is None else dict(audio_guidance_scale=s_a)
    plain = _call(small, steps, guidance_end=END, **audio)
    assert "apg" not in small["pipe"].last_guidance
    got = _call(small, steps, guidance_end=END, apg_eta=0.0, apg_norm_threshold=R_CAP, apg_momentum=BETA, **audio)
    lg = small["pipe"].last_guidance
    assert lg["apg"] == dict(eta=0.0, norm_threshold=R_CAP, momentum=BETA) and lg["guided_steps"] == 3
    with oracle_on_cpu():
        ref, state = AP.restated_loop(small["oracle"], inp["latents"], _windows(small), S, inp["kps_features"],
                                      inp["audio_embeddings"], steps, "ddim", s_a=s_a, end=END, eta=0.0, r=R_CAP, beta=BETA)
    bites = torch.cat([c for call in state.capped for c in call])
    assert bool(bites.any()) and not bool(bites.all())
    e_plain = rel_l2(plain, _plain_ref(small, steps, s_a))
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[DDIM, APG eta 0 r {R_CAP} beta {BETA}, guidance_end {END}, audio_guidance_scale {s_a}, SMALL, "
          f"reflected_F11_c4o2, {steps} steps] relL2={r:.4g} cosine={c:.6f} vs the APG restated loop; e_plain={e_plain:.4g}; "
          f"the plain clip vs the APG loop: relL2={rel_l2(plain, ref):.4g}; the cap bit on {int(bites.sum())} of "
          f"{bites.numel()} frame differences")
    assert torch.isfinite(got).all() and r <= 2 * e_plain, (r, e_plain)
    assert r <= 5e-2 and c >= 0.998, (r, c)
    assert r < rel_l2(plain, ref)


def test_pipeline_without_a_guided_step_is_the_no_cfg_route_bit_for_bit(small):
    steps = 5
    off = _call(small, steps, guidance_end=0.0, apg_eta=0.0, apg_norm_threshold=R_CAP, apg_momentum=BETA)
    assert small["pipe"].last_guidance["guided_steps"] == 0
    assert torch.equal(off, _call(small, steps, inp=cases.cond_only(small["inp"]), guidance=1.0))
