"""Every route of v_express_amd/blocks.py on a real MI355X against float64, with the row statistics checked for freshness.

Each case runs one block through the real `weights.prep_*` and `blocks.*` at the smallest geometry at which the product's
own `*_applies` rule takes the route it means to test (the predicates are never replaced), with the route selected by the
product's own switches, on both element libraries, under tests/stats_spy.py.  Per case:

* the route, including the effect of every switch a case sets: `ops.block_paths()`; the GEMM launches by shape,
  configuration and kernel (`GemmProfile`: Q | K as one [m, 2C] STORE launch on "gemm_ring..." with V^T alone, or one
  3C-wide SPLIT launch; the K = 5C dual-source launch of the proj_out fold or the K = 4C one; "coop2", "splitk"); the other
  kernels by wrapper name (`OpProfile`: the GroupNorm's own statistics pass or its apply-only pass, `row_stats`); calls of
  `row_stats` / `add_row_bias` / `groupnorm_stats`; the entry points, row widths and formats of every consumption of
  statistics - a case that silently ran the fallback, or whose switch went dead, fails;
* freshness: no stale consumption; GroupNorm sums riding on the output = sums of its stored values (STAT_BOUNDS["gn_sums"]);
* against float64 (tests/block_wiring_cases.py, from the raw state_dict): the bound is MEASURED, not fixed - the same block
  through tests/fake_ops.py (float64 arithmetic, element-type rounding at every kernel boundary) on the same inputs gives
  e_emul = (relative L2, max|err| / max|ref|); the kernels must stay within 3 x e_emul in both ("about 3x the rounding
  noise", gemm_cases.py / attention_cases.py).  tests/test_block_wiring_cpu.py shows that every wiring mutant of the
  reference lies beyond 2 x 3 x e_emul;
* the identities the code claims, bit for bit: each batch item computed alone = its rows of the batched call
  (`ops.frame_rows`), FF slabs on = off, FF_FUSED on = off where the one launch claims the bits of the two (from
  hw = 256 on: the 256-row tile).  FOLD_ZERO_AUDIO on / off, TB_FUSED on / off (summation order inside the 16 x 16
  products) and FF_FUSED on / off at 8 x 8 (other GEMM tiles) differ by rounding and meet through float64 only.

    python -m pytest tests/test_gpu_block_wiring.py -m gpu -q -s      (prints e_emul and the kernels' error per case)

Measured on an MI355X (also LABNOTES.md 18); every route sits at 0.86 ... 1.09 x e_emul, so nothing had to be added to the
emulation:

    case                                   bf16: e_emul relL2 / max   kernels relL2 / max  (ratio)      f16: e_emul relL2 / max   kernels relL2 / max  (ratio)
    read 16x16_c640_one_part_stats           0.0037 / 0.00381    0.0037 / 0.00392  (1.00 / 1.03)   0.000463 / 0.000525 0.000463 / 0.000525 (1.00 / 1.00)
    read 16x16_c640_proj_fold               0.00365 / 0.00446   0.00365 / 0.0039   (1.00 / 0.87)   0.000454 / 0.000577 0.000454 / 0.000498 (1.00 / 0.86)
    read 16x16_c640_proj_fold_off           0.00386 / 0.00446   0.00387 / 0.00413  (1.00 / 0.92)   0.000481 / 0.000577 0.000481 / 0.000577 (1.00 / 1.00)
    read 24x32_c640_ring_parts              0.00363 / 0.00409   0.00363 / 0.0044   (1.00 / 1.07)   0.000453 / 0.000533 0.000453 / 0.000533 (1.00 / 1.00)
    read 32x48_gn_fold_off                  0.00366 / 0.00417   0.00366 / 0.00432  (1.00 / 1.04)   0.000456 / 0.000507 0.000456 / 0.000524 (1.00 / 1.03)
    read 32x48_gn_fold_ring                 0.00365 / 0.0043    0.00365 / 0.0042   (1.00 / 0.98)   0.000454 / 0.000524 0.000454 / 0.000524 (1.00 / 1.00)
    read 32x48_qk_ring_off                  0.00373 / 0.00435   0.00373 / 0.00435  (1.00 / 1.00)   0.000467 / 0.000503 0.000467 / 0.000508 (1.00 / 1.01)
    read 32x48_ring_off                     0.00366 / 0.00417   0.00366 / 0.00432  (1.00 / 1.04)   0.000456 / 0.000507 0.000456 / 0.000524 (1.00 / 1.03)
    read 8x8_A                              0.00367 / 0.00393   0.00367 / 0.004    (1.00 / 1.02)   0.000458 / 0.000553 0.000459 / 0.000506 (1.00 / 0.91)
    read 8x8_A_audio_three_launches         0.00364 / 0.00422   0.00364 / 0.00404  (1.00 / 0.96)   0.000455 / 0.00045  0.000455 / 0.000482 (1.00 / 1.07)
    read 8x8_A_ff_two_launches              0.00367 / 0.00393   0.00367 / 0.004    (1.00 / 1.02)   0.000458 / 0.000553 0.000459 / 0.000506 (1.00 / 0.91)
    read 8x8_A_fp8                           0.0106 / 0.0125     0.0106 / 0.012    (1.00 / 0.96)    0.00997 / 0.0113    0.00997 / 0.0114   (1.00 / 1.01)
    read 8x8_A_no_ln_fold                   0.00367 / 0.00364   0.00367 / 0.00398  (1.00 / 1.09)   0.000457 / 0.000542 0.000457 / 0.000542 (1.00 / 1.00)
    read 8x8_A_separate_stats_pass          0.00367 / 0.00393   0.00367 / 0.004    (1.00 / 1.02)   0.000458 / 0.000553 0.000459 / 0.000506 (1.00 / 0.91)
    read 8x8_A_unfolded_zero_audio          0.00376 / 0.00393   0.00376 / 0.004    (1.00 / 1.02)   0.000469 / 0.000553  0.00047 / 0.000506 (1.00 / 0.91)
    read 8x8_B                              0.00376 / 0.00408   0.00377 / 0.004    (1.00 / 0.98)   0.000471 / 0.000541  0.00047 / 0.000563 (1.00 / 1.04)
    read 8x8_N                              0.00385 / 0.00393   0.00386 / 0.004    (1.00 / 1.02)   0.000481 / 0.000553 0.000481 / 0.000506 (1.00 / 0.91)
    read 8x8_N_audio_three_launches         0.00381 / 0.00422   0.00381 / 0.00404  (1.00 / 0.96)   0.000475 / 0.000462 0.000475 / 0.000482 (1.00 / 1.04)
    motion 16x16_c640_proj_fold             0.00346 / 0.00383   0.00347 / 0.00384  (1.00 / 1.00)   0.000433 / 0.000491 0.000435 / 0.000471 (1.00 / 0.96)
    motion 16x16_c640_proj_fold_mm_off      0.00367 / 0.00395   0.00368 / 0.00395  (1.00 / 1.00)   0.000459 / 0.00047   0.00046 / 0.000471 (1.00 / 1.00)
    motion 2x2_f24                          0.00308 / 0.00342   0.00307 / 0.00313  (1.00 / 0.92)   0.000384 / 0.000458 0.000382 / 0.000458 (1.00 / 1.00)
    motion 32x48_gn_fold_ring               0.00309 / 0.00321    0.0031 / 0.00343  (1.00 / 1.07)   0.000386 / 0.000446 0.000387 / 0.00044  (1.00 / 0.99)
    motion 8x8_f16                           0.0031 / 0.00315   0.00311 / 0.00308  (1.00 / 0.98)   0.000387 / 0.000366 0.000388 / 0.000386 (1.00 / 1.06)
    motion 8x8_f16_fp8                       0.0146 / 0.0118     0.0146 / 0.0118   (1.00 / 1.00)     0.0142 / 0.0134     0.0143 / 0.0142   (1.00 / 1.06)
    motion 8x8_f16_no_ln_fold               0.00312 / 0.00297   0.00313 / 0.00308  (1.00 / 1.04)   0.000389 / 0.0004    0.00039 / 0.000385 (1.00 / 0.96)
    motion 8x8_f16_three_launches            0.0031 / 0.00315   0.00311 / 0.00308  (1.00 / 0.98)   0.000387 / 0.000366 0.000388 / 0.000367 (1.00 / 1.00)
    motion 8x8_f8_three_launches            0.00316 / 0.00321   0.00317 / 0.00316  (1.00 / 0.99)   0.000394 / 0.000443 0.000395 / 0.000443 (1.00 / 1.00)
    resnet 16x16_c1280_coop                 0.00315 / 0.00445   0.00315 / 0.00445  (1.00 / 1.00)   0.000394 / 0.000551 0.000394 / 0.000551 (1.00 / 1.00)
    resnet 16x16_c1280_coop_off             0.00315 / 0.00445   0.00315 / 0.00445  (1.00 / 1.00)   0.000394 / 0.000551 0.000394 / 0.000551 (1.00 / 1.00)
    resnet 16x16_no_gn_fused                0.00302 / 0.00521   0.00302 / 0.00521  (1.00 / 1.00)   0.000378 / 0.000654 0.000378 / 0.000654 (1.00 / 1.00)
    resnet 16x16_shortcut                   0.00302 / 0.00521   0.00302 / 0.00521  (1.00 / 1.00)   0.000378 / 0.000654 0.000378 / 0.000654 (1.00 / 1.00)
    resnet 16x16_skip_shortcut              0.00315 / 0.00468   0.00315 / 0.00468  (1.00 / 1.00)   0.000394 / 0.000621 0.000394 / 0.000621 (1.00 / 1.00)
    resnet 8x8_plain                        0.00186 / 0.00223   0.00186 / 0.00223  (1.00 / 1.00)   0.000232 / 0.000376 0.000232 / 0.000376 (1.00 / 1.00)
    sampler downsample_gn                   0.00241 / 0.00362   0.00241 / 0.00362  (1.00 / 1.00)   0.000301 / 0.000393 0.000301 / 0.000393 (1.00 / 1.00)
    sampler downsample_no_gn                0.00241 / 0.00362   0.00241 / 0.00362  (1.00 / 1.00)   0.000301 / 0.000393 0.000301 / 0.000393 (1.00 / 1.00)
    sampler upsample_3x3_below_min_hw       0.00241 / 0.00353   0.00241 / 0.00353  (1.00 / 1.00)     0.0003 / 0.000416   0.0003 / 0.000416 (1.00 / 1.00)
    sampler upsample_phases                 0.00235 / 0.00375   0.00235 / 0.00375  (1.00 / 1.00)   0.000293 / 0.000449 0.000293 / 0.000449 (1.00 / 1.00)
    sampler upsample_phases_off             0.00241 / 0.00346   0.00241 / 0.00346  (1.00 / 1.00)     0.0003 / 0.000448   0.0003 / 0.000448 (1.00 / 1.00)
    write 8x8                               0.00372 / 0.00396   0.00372 / 0.00396  (1.00 / 1.00)   0.000454 / 0.000542 0.000455 / 0.000542 (1.00 / 1.00)
    write 8x8/bank                          0.00364 / 0.00574   0.00365 / 0.00574  (1.00 / 1.00)   0.000455 / 0.000883 0.000455 / 0.000883 (1.00 / 1.00)
    write 16x16_c640                        0.00378 / 0.00407   0.00377 / 0.00407  (1.00 / 1.00)   0.000473 / 0.000552 0.000472 / 0.000552 (1.00 / 1.00)
    write 16x16_c640/bank                   0.00375 / 0.00553   0.00375 / 0.00553  (1.00 / 1.00)   0.000467 / 0.000661 0.000466 / 0.000661 (1.00 / 1.00)
    bank_kv c320                            0.00235 / 0.00292   0.00235 / 0.00292  (1.00 / 1.00)   0.000293 / 0.00044  0.000293 / 0.00044  (1.00 / 1.00)
    bank_kv c640                            0.00242 / 0.00371   0.00242 / 0.00371  (1.00 / 1.00)   0.000302 / 0.000428 0.000302 / 0.000428 (1.00 / 1.00)
"""
import pytest
import torch

import block_wiring_cases as BC
import census
import stats_spy

pytestmark = pytest.mark.gpu
ELEMS = (torch.bfloat16, torch.float16)
EL_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
FACTOR = 3.0


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from v_express_amd import lib as L, ops as o
    torch.cuda.set_device(0)
    return L, o


@pytest.fixture(params=ELEMS, ids=lambda e: EL_NAME[e])
def ops_el(mods, request):
    """(ops, element type): every case runs on the bfloat16 and on the float16 library."""
    L, o = mods
    with L.element_type(request.param):
        yield o, request.param
    o.clear_caches()


_REF = {}


def case_and_reference(el, **geo):
    """(case, prepared weights, float64 reference) - computed once per (geometry, element type) and left unchanged."""
    key = (el, tuple(sorted(geo.items())))
    if key not in _REF:
        cs = BC.make_case(device="cuda", elem=el, **geo)
        _REF[key] = (cs, BC.prepare(cs), BC.reference(cs))
    return _REF[key]


class Switches:
    """The product's own switches for the duration of a run (and `ops.fp8_projections`)."""

    def __init__(self, ops, mp, sw):
        self.ops, self.mp, self.sw = ops, mp, dict(sw)

    def __enter__(self):
        self.fp8 = self.ops.fp8_projections(self.sw.pop("FP8_PROJ", False))
        self.fp8.__enter__()
        self.ctx = self.mp.context()
        m = self.ctx.__enter__()
        for k, v in self.sw.items():
            m.setattr(self.ops, k, v)
        return m

    def __exit__(self, *a):
        self.ctx.__exit__(*a)
        self.fp8.__exit__(*a)


COUNTED = ("row_stats", "add_row_bias", "groupnorm_stats")      # entry points counted per run (no statistics of their own)


class Launches(list):
    """The GEMM launches of a run as "<m>x<n>x<k> <configuration> = <kernel>" strings, with their shapes, the names of the
    other kernels' wrappers (`OpProfile`) and the calls of COUNTED."""

    def __init__(self, gp, op, calls):
        super().__init__(f"{r[4][0]}x{r[4][1]}x{r[4][2]} {r[3]} = {r[5]}" for r in gp.records)
        self.shapes = [tuple(r[4]) for r in gp.records]
        self.ops = [r[0] for r in op.records]
        self.calls = calls

    def at(self, n, k, subs=()):
        """The launches with these N and K whose text carries every substring."""
        return [t for t, sh in zip(self, self.shapes) if sh[1] == n and sh[2] == k and all(x in t for x in subs)]


def run_kernels(ops, mp, cs, P, sw, items=None):
    """-> (output, spy, block paths, Launches)."""
    with Switches(ops, mp, sw) as m:
        spy = stats_spy.StatsSpy(ops).install(m)
        calls = {}
        for name in COUNTED:
            def counted(*a, _fn=getattr(ops, name), _name=name, **k):
                calls[_name] = calls.get(_name, 0) + 1
                return _fn(*a, **k)
            m.setattr(ops, name, counted)
        ops.BLOCK_PATHS.clear()
        with ops.GemmProfile() as gp, ops.OpProfile() as op:
            out = BC.run(cs, P, items)
        torch.cuda.synchronize()
        return out, spy, ops.block_paths(), Launches(gp, op, calls)


def first(out):
    return out[0] if isinstance(out, tuple) else out


def gn_ratio(ops, out):
    st = ops.gn_of(out)
    if st is None:
        return None
    assert st.fits(out.shape[0], out.shape[1], st.groups, out.shape[2])
    x = out.double().view(st.frames, st.hw, st.groups, -1)
    want = torch.stack([x.sum(dim=(1, 3)), (x * x).sum(dim=(1, 3))], dim=-1)
    return census._stat_ratio(census._gn_sums(st.ws, st.frames, st.groups, st.hw, st.c), want,
                              census.STAT_BOUNDS["gn_sums"])[0]


def check_route(name, paths, gemms, spy, route):
    """route: {"paths": {block: text a decision of that block must start with}, "no_paths": {block: text none of its
    decisions may start with}, "gemm": [substrings some launched GEMM configuration / kernel name must carry], "no_gemm": [substrings none may carry], "consumed": [entry points that must have consumed statistics],
    "not_consumed": [...], "parts": True when the statistics must be two-part sums, "consumed_at": [(entry point, row width,
    statistics width) some consumption must have], "gemm_at" / "no_gemm_at": [(N, K, substrings)] a launch of that shape
    carrying all substrings must / must not exist, "ops" / "no_ops": wrapper names of the other kernels (`OpProfile`) that
    must / must not have run, "calls": {entry point of COUNTED: whether it must have been called}, "no_decision": [blocks
    whose `*_applies` rule must not even have been asked], "raw_gn": whether the output object carries sums at all}."""
    for n, k, subs in route.get("gemm_at", ()):
        assert gemms.at(n, k, subs), f"{name}: no N={n} K={k} launch with {subs}: {gemms.at(n, k) or sorted(set(gemms))}"
    for n, k, subs in route.get("no_gemm_at", ()):
        assert not gemms.at(n, k, subs), f"{name}: a N={n} K={k} launch with {subs} ran: {gemms.at(n, k, subs)}"
    for op in route.get("ops", ()):
        assert op in gemms.ops, f"{name}: no {op} kernel ran: {sorted(set(gemms.ops))}"
    for op in route.get("no_ops", ()):
        assert op not in gemms.ops, f"{name}: a {op} kernel ran"
    for op, want in route.get("calls", {}).items():
        assert bool(gemms.calls.get(op)) == want, f"{name}: ops.{op} called {gemms.calls.get(op, 0)} x, wanted {'some' if want else 'none'}"
    for block in route.get("no_decision", ()):
        assert not [k for k in paths if k.startswith(block + " ")], f"{name}: a {block} decision was taken: {paths}"
    for op, c, width in route.get("consumed_at", ()):
        assert any(r.op == op and r.shape[-1] == c and r.width == width for r in spy.consumptions()), \
            f"{name}: no {op} consumed [*, {width}] statistics of {c}-wide rows:\n{spy.report()}"
    for block, text in route.get("paths", {}).items():
        hit = [v for k, v in paths.items() if k.startswith(block + " ")]
        assert any(v.startswith(text) for v in hit), f"{name}: {block} took {hit or 'no decision'}, wanted {text!r}"
    for block, text in route.get("no_paths", {}).items():
        hit = [v for k, v in paths.items() if k.startswith(block + " ")]
        assert hit and not any(v.startswith(text) for v in hit), f"{name}: {block} took {hit or 'no decision'}, not to be {text!r}"
    for sub in route.get("gemm", ()):
        assert any(sub in g for g in gemms), f"{name}: no {sub} GEMM launched: {sorted(set(gemms))}"
    for sub in route.get("no_gemm", ()):
        assert not any(sub in g for g in gemms), f"{name}: a {sub} GEMM was launched: {sorted(set(gemms))}"
    ops_seen = {r.op for r in spy.consumptions()}
    for op in route.get("consumed", ()):
        assert op in ops_seen, f"{name}: {op} consumed no statistics ({sorted(ops_seen)})"
    for op in route.get("not_consumed", ()):
        assert op not in ops_seen, f"{name}: {op} consumed statistics: the route meant to avoid it"
    if "parts" in route:
        widths = {r.width for r in spy.records}
        assert widths == ({4} if route["parts"] else {2}), f"{name}: statistics formats {widths}"


def check(name, ops, el, mp, geo, sw, route, alone=True, factor=FACTOR):
    """One case: route, freshness, the float64 bound measured through the emulation, each item alone.  -> the output."""
    cs, P, ref = case_and_reference(el, **geo)
    with Switches(ops, mp, sw):
        emul = BC.emulated(cs, P, mp.context)
    out, spy, paths, gemms = run_kernels(ops, mp, cs, P, sw)
    check_route(name, paths, gemms, spy, route)
    if "raw_gn" in route:
        assert (getattr(first(out), "_vx_gn", None) is not None) == route["raw_gn"], f"{name}: sums on the output object"
    spy.assert_fresh()
    outs, refs, emuls = (out, ref, emul) if isinstance(out, tuple) and cs.kind == "write" else ((out,), (ref,), (emul,))
    for i, (o, r, e) in enumerate(zip(outs, refs, emuls)):
        e_emul, err = BC.errors(e, r), BC.errors(o, r)
        print(f"[{name}{'/bank' if i else ''} {EL_NAME[el]}] e_emul {e_emul[0]:.3g} / {e_emul[1]:.3g}   kernels {err[0]:.3g} / "
              f"{err[1]:.3g}  ({err[0] / e_emul[0]:.2f} x / {err[1] / e_emul[1]:.2f} x)   stats worst {spy.worst():.3g}")
        assert torch.isfinite(o.float()).all()
        assert BC.within(err, e_emul, factor), f"{name}: kernels {err} beyond {factor} x e_emul {e_emul}"
    g = gn_ratio(ops, first(out)) if first(out).dim() == 3 else None
    if route.get("gn"):
        assert g is not None, f"{name}: no GroupNorm sums ride on the output"
    if g is not None:
        print(f"    GroupNorm sums on the output: {g:.3g} x their bound")
    assert g is None or g <= 1.0, f"{name}: GroupNorm sums on the output are {g:.3g} x their bound off the stored values"
    if alone:
        for bi in range(cs.b):
            one = run_kernels(ops, mp, cs, P, sw, items=[bi])[0]
            for o1, ob in zip(one if isinstance(one, tuple) else (one,), outs):        # (the writer: output AND bank)
                r1 = ob.shape[0] // cs.b
                assert torch.equal(o1, ob[bi * r1:(bi + 1) * r1]), f"{name}: item {bi} alone differs from its rows"
    return out


# ------------------------------------------------------------------------------------------------ the spatial read block
G8 = dict(kind="read", c=320, f=16, H=8, W=8)                    # one-launch FF (rows % 128), one-launch audio block (hw % 16)
ONE_FF = {"feed_forward": "one launch"}
ONE_AX = {"audio_cross_attention": "one launch"}


def QK_RING_ON(c, width):
    """Q | K as ONE LayerNorm-folded [m, C] -> [m, 2C] STORE launch on the persistent kernel, consuming `width`-wide
    statistics, V^T alone through a C-wide SPLIT launch; no fused 3C-wide SPLIT launch."""
    return dict(gemm_at=[(2 * c, c, ["gemm_ring", "STORE"]), (c, c, ["SPLIT"])], no_gemm_at=[(3 * c, c, [])],
                consumed_at=[("gemm", c, width), ("gemm_split", c, width)])


def QK_RING_OFF(c):
    """q, k and V^T from ONE 3C-wide SPLIT launch; no [m, 2C] STORE launch (the bank's K | V projection is a SPLIT one)."""
    return dict(gemm_at=[(3 * c, c, ["SPLIT"])], no_gemm_at=[(2 * c, c, ["STORE"])])


READ = {
    # name: (geometry, switches, route)
    "8x8_A": (dict(G8, combo="A"), {}, dict(paths={**ONE_FF, **ONE_AX, "groupnorm_proj_in": "GroupNorm apply"},
                                            consumed=["gemm_split", "gemm", "audio_xattn", "ff_fused"], no_gemm=["gemm_ring"],
                                            parts=False, calls={"row_stats": False, "add_row_bias": False},
                                            gemm_at=[(960, 320, ["SPLIT"])])),
    # (item 1: banked with zero audio - its constant attn2 term cannot ride on attn1: add_row_bias + a statistics refresh)
    "8x8_B": (dict(G8, combo="B"), {}, dict(paths={**ONE_FF, **ONE_AX}, consumed=["audio_xattn", "ff_fused"],
                                            calls={"row_stats": True, "add_row_bias": True})),
    "8x8_N": (dict(G8, combo="N"), {}, dict(paths={**ONE_FF, **ONE_AX}, consumed=["audio_xattn", "ff_fused"],
                                            calls={"row_stats": False, "add_row_bias": False})),
    "8x8_A_unfolded_zero_audio": (dict(G8, combo="A"), {"FOLD_ZERO_AUDIO": [False]},
                                  dict(paths=ONE_FF, calls={"row_stats": True, "add_row_bias": True})),
    "8x8_A_ff_two_launches": (dict(G8, combo="A"), {"FF_FUSED": [False]},
                              dict(paths={"feed_forward": "two launches"}, consumed=["geglu"], not_consumed=["ff_fused"])),
    "8x8_A_audio_three_launches": (dict(G8, combo="A"), {"AX_FUSED": [False]},
                                   dict(paths={"audio_cross_attention": "three launches"}, not_consumed=["audio_xattn"])),
    "8x8_N_audio_three_launches": (dict(G8, combo="N"), {"AX_FUSED": [False]},
                                   dict(paths={"audio_cross_attention": "three launches"}, not_consumed=["audio_xattn"])),
    "8x8_A_no_ln_fold": (dict(G8, combo="A"), {"LN_FOLD": [False]},
                         dict(not_consumed=["gemm", "geglu", "gemm_split", "ff_fused", "audio_xattn"])),
    "8x8_A_separate_stats_pass": (dict(G8, combo="A"), {"FUSED_STATS": [False]},
                                  dict(paths=ONE_FF, consumed=["ff_fused"], calls={"row_stats": True, "add_row_bias": False},
                                       ops=["row_stats"])),
    "8x8_A_fp8": (dict(G8, combo="A"), {"FP8_PROJ": True}, dict(paths={"feed_forward": "two launches"}, consumed=["geglu"],
                                                                 not_consumed=["gemm", "gemm_split"])),
    # hw >= 256, C = 640: proj_out folded into the FF's second GEMM; two-part statistics ([rows, 4]) finished for
    # consumers that are not on the persistent kernel
    "16x16_c640_proj_fold": (dict(kind="read", c=640, f=4, H=16, W=16, combo="A"), {},
                             dict(paths={"ff_proj_out": "FF output GEMM + proj_out as one"}, consumed=["geglu"], parts=True,
                                  no_gemm=["gemm_ring"], gemm_at=[(640, 3200, [])], no_gemm_at=[(640, 2560, [])])),
    "16x16_c640_proj_fold_off": (dict(kind="read", c=640, f=4, H=16, W=16, combo="A"), {"FF_PROJ_FOLD": [False]},
                                 dict(paths={"ff_proj_out": "two launches"}, consumed=["geglu"],
                                      gemm_at=[(640, 2560, [])], no_gemm_at=[(640, 3200, [])])),
    "16x16_c640_one_part_stats": (dict(kind="read", c=640, f=4, H=16, W=16, combo="B"), {"STATS_PARTS_WIDTHS": set()},
                                  dict(parts=False)),
    # the persistent kernel at N = 320 (2 * 24576 / 256 tiles), with it the GroupNorm fold and Q | K on the ring
    "32x48_gn_fold_ring": (dict(kind="read", c=320, f=16, H=32, W=48, combo="A"), {},
                           dict(paths={"groupnorm_proj_in": "GroupNorm folded", **ONE_FF, **ONE_AX}, **QK_RING_ON(320, 2),
                                calls={"groupnorm_stats": True}, no_ops=["groupnorm_stats+apply", "groupnorm_apply"])),
    "32x48_gn_fold_off": (dict(kind="read", c=320, f=16, H=32, W=48, combo="A"), {"GN_FOLD": [False]},
                          dict(paths={"groupnorm_proj_in": "GroupNorm apply"}, **QK_RING_ON(320, 2),
                               calls={"groupnorm_stats": False}, ops=["groupnorm_stats+apply"])),
    "32x48_ring_off": (dict(kind="read", c=320, f=16, H=32, W=48, combo="A"), {"RING_MODE": [0]},
                       dict(paths={"groupnorm_proj_in": "GroupNorm apply"}, no_gemm=["gemm_ring"], **QK_RING_OFF(320))),
    "32x48_qk_ring_off": (dict(kind="read", c=320, f=16, H=32, W=48, combo="B"), {"QK_RING": [False]},
                          dict(paths={"groupnorm_proj_in": "GroupNorm folded"}, gemm=["gemm_ring"], **QK_RING_OFF(320))),
    # Q | K on the ring at N = 640 and two-part statistics with their ring consumer: rows_item = 16 * 768
    "24x32_c640_ring_parts": (dict(kind="read", c=640, f=16, H=24, W=32, combo="A"), {},
                              dict(paths={"ff_proj_out": "FF output GEMM + proj_out as one"}, parts=True, **QK_RING_ON(640, 4))),
}


@pytest.mark.parametrize("name", sorted(READ))
def test_spatial_transformer_read_routes(ops_el, monkeypatch, name):
    ops, el = ops_el
    geo, sw, route = READ[name]
    # (every read block's proj_out - folded into the FF or not - leaves the next GroupNorm's partial sums on the output)
    check("read " + name, ops, el, monkeypatch, geo, sw, dict(route, gn=True))


def test_read_one_launch_ff_keeps_the_bits_of_the_two_launches(ops_el, monkeypatch):
    """ops.py: "The 64x64-level feed-forward (C = 320) as ONE launch: bit-identical to the two vx_gemm launches" - through
    the whole block, at the smallest geometry at which the two launches run on the 256-row tile the one launch restates
    (hw = 256, rows = 8192).  Below it (8 x 8) the two launches run on the 128 x 128 / 64 x 160 tiles, whose float32 sums
    differ in the last bit on 0.02 % (bf16) / 0.13 % (f16) of the elements: those routes meet through float64 only."""
    ops, el = ops_el
    cs, P, _ = case_and_reference(el, kind="read", c=320, f=16, H=16, W=16, combo="A")
    a, spy, paths, _ = run_kernels(ops, monkeypatch, cs, P, {})
    check_route("read 16x16 FF identity", paths, _, spy, dict(paths=ONE_FF, consumed=["ff_fused"]))
    # (FF_PROJ_FOLD off: from hw = 256 on the two-launch FF would otherwise fold proj_out into its second GEMM - other
    # weights, other roundings; the one-launch arm never takes that fold)
    b, spy, paths, gemms = run_kernels(ops, monkeypatch, cs, P, {"FF_FUSED": [False], "FF_PROJ_FOLD": [False]})
    check_route("read 16x16 FF identity", paths, gemms, spy,
                dict(paths={"feed_forward": "two launches", "ff_proj_out": "two launches"}, consumed=["geglu"], gemm=["GEGLU"]))
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the motion module
M8 = dict(kind="motion", c=320, f=16, H=8, W=8)
ONE_TB = {"temporal_attention": "one launch"}
MOTION = {
    "8x8_f16": (M8, {}, dict(paths={**ONE_TB, **ONE_FF}, consumed=["tblock_fused", "ff_fused"], not_consumed=["gemm"])),
    "2x2_f24": (dict(kind="motion", c=320, f=24, H=2, W=2), {}, dict(paths=ONE_TB, consumed=["tblock_fused"])),
    "8x8_f16_three_launches": (M8, {"TB_FUSED": [False]},
                               dict(paths={"temporal_attention": "three launches"}, consumed=["gemm", "ff_fused"],
                                    not_consumed=["tblock_fused"])),
    "8x8_f8_three_launches": (dict(kind="motion", c=320, f=8, H=8, W=8), {},
                              dict(paths={"temporal_attention": "three launches"}, consumed=["gemm"])),
    "8x8_f16_no_ln_fold": (M8, {"LN_FOLD": [False]}, dict(not_consumed=["gemm", "geglu", "tblock_fused", "ff_fused"])),
    "8x8_f16_fp8": (M8, {"FP8_PROJ": True}, dict(consumed=["geglu"], not_consumed=["gemm", "tblock_fused"])),
    "16x16_c640_proj_fold": (dict(kind="motion", c=640, f=16, H=16, W=16), {},
                             dict(paths={"ff_proj_out": "FF output GEMM + proj_out as one"}, consumed=["gemm", "geglu"],
                                  parts=True, gemm_at=[(640, 3200, [])], no_gemm_at=[(640, 2560, [])])),
    "16x16_c640_proj_fold_mm_off": (dict(kind="motion", c=640, f=16, H=16, W=16), {"FF_PROJ_FOLD_MM": [False]},
                                    dict(consumed=["gemm", "geglu"], no_decision=["ff_proj_out"],
                                         gemm_at=[(640, 2560, [])], no_gemm_at=[(640, 3200, [])])),
    "32x48_gn_fold_ring": (dict(kind="motion", c=320, f=16, H=32, W=48), {},
                           dict(paths={"groupnorm_proj_in": "GroupNorm folded", **ONE_TB, **ONE_FF}, gemm=["gemm_ring"])),
}


@pytest.mark.parametrize("name", sorted(MOTION))
def test_motion_module_routes(ops_el, monkeypatch, name):
    ops, el = ops_el
    geo, sw, route = MOTION[name]
    # (gn_next: the sums ride on the output wherever a frame has whole 8-row slabs - not at 2 x 2 pixels)
    check("motion " + name, ops, el, monkeypatch, geo, sw, dict(route, gn=name != "2x2_f24"))


def test_motion_one_launch_ff_keeps_the_bits_of_the_two_launches(ops_el, monkeypatch):
    """As test_read_one_launch_ff_keeps_the_bits_of_the_two_launches, in the motion module (hw = 256).  The one-launch
    TEMPORAL block claims no bits: it differs from its three launches "by the summation order inside the 16 x 16 products"
    (test_tblock_fused_matches_the_three_launches; measured through this block at 8 x 8: 5 % of the bf16 elements, one ulp),
    so TB_FUSED on and off are both cases of MOTION above and meet through float64."""
    ops, el = ops_el
    cs, P, _ = case_and_reference(el, kind="motion", c=320, f=16, H=16, W=16)
    a = run_kernels(ops, monkeypatch, cs, P, {})[0]
    b, spy, paths, gemms = run_kernels(ops, monkeypatch, cs, P, {"FF_FUSED": [False], "FF_PROJ_FOLD": [False]})
    check_route("motion 16x16 FF identity", paths, gemms, spy,
                dict(paths={"feed_forward": "two launches", "ff_proj_out": "two launches"}, consumed=["geglu"], gemm=["GEGLU"]))
    assert torch.equal(a, b)


def test_feed_forward_slabs_keep_the_bits_and_slice_fresh_statistics(ops_el, monkeypatch):
    """`_feed_forward`: "Rows are independent: same bits".  Slabs need m % (2 * 65536) == 0 rows at C = 320: the 64x64
    level's 2 x 16 x 4096 rows, two-launch FF (the one-launch kernel has no intermediate to slab)."""
    from v_express_amd import blocks as B
    ops, el = ops_el
    cs, P, _ = case_and_reference(el, **M8)
    g = torch.Generator().manual_seed(5)
    h0 = (torch.randn(131072, 320, generator=g) * torch.rand(131072, 1, generator=g).add(0.5) +
          torch.randn(131072, 1, generator=g)).to(el).cuda()

    def ff(slab_bytes):
        h = h0.clone()
        with Switches(ops, monkeypatch, {"FF_FUSED": [False], "FF_SLAB_BYTES": [slab_bytes]}) as m:
            spy = stats_spy.StatsSpy(ops).install(m)
            with ops.frame_rows(4096, items=2):
                assert B._feed_forward(P, h, ops.row_stats(h)) is None
        torch.cuda.synchronize()
        return h, spy
    whole, spy = ff(0)
    assert len(spy.consumptions("geglu")) == 1
    spy.assert_fresh()
    slabbed, spy = ff(131072 * 1280 * 2 // 2)
    assert [r.shape[0] for r in spy.consumptions("geglu")] == [65536, 65536]
    spy.assert_fresh()
    assert torch.equal(slabbed, whole)


# ------------------------------------------------------------------------------------------------ resnet, samplers, writer
RESNET = {
    # 8x8: the long-K 3x3 convolutions take split-K (hw <= 64, K >= 2560)
    "8x8_plain": (dict(kind="resnet", c=320, f=16, H=8, W=8, temb_dim=1280), {}, dict(gemm=["splitk"])),
    "16x16_skip_shortcut": (dict(kind="resnet", c=320, skip=320, cout=320, f=16, H=16, W=16, temb_dim=1280), {}, {}),
    # (norm1 makes its own statistics pass - the input carries no sums -, norm2 applies the sums conv1 left)
    "16x16_shortcut": (dict(kind="resnet", c=320, cout=640, f=4, H=16, W=16, temb_dim=1280), {},
                       dict(ops=["groupnorm_stats+apply", "groupnorm_apply"], raw_gn=True)),
    "16x16_no_gn_fused": (dict(kind="resnet", c=320, cout=640, f=4, H=16, W=16, temb_dim=1280), {"GN_FUSED": [False]},
                          dict(ops=["groupnorm_stats+apply"], no_ops=["groupnorm_apply"], raw_gn=False)),
    # 96 <= tiles < 192, K >= 8192: the cooperative two-way K split on the persistent kernel
    "16x16_c1280_coop": (dict(kind="resnet", c=1280, skip=1280, cout=1280, f=16, H=16, W=16, temb_dim=1280), {},
                         dict(paths={"gemm_too_few_tiles": "persistent kernel, cooperative"}, gemm=["coop2"])),
    "16x16_c1280_coop_off": (dict(kind="resnet", c=1280, skip=1280, cout=1280, f=16, H=16, W=16, temb_dim=1280),
                             {"RING_COOP": [False]}, dict(no_paths={"gemm_too_few_tiles": "persistent kernel"}, no_gemm=["coop2"])),
}


@pytest.mark.parametrize("name", sorted(RESNET))
def test_resnet_block_routes(ops_el, monkeypatch, name):
    ops, el = ops_el
    geo, sw, route = RESNET[name]
    # (conv2's epilogue leaves the sums where it is no split-K launch: the 16 x 16 cases, unless GN_FUSED is off)
    check("resnet " + name, ops, el, monkeypatch, geo, sw, dict(route, gn=name.startswith("16x16") and "GN_FUSED" not in sw))


SAMPLERS = {
    "downsample_gn": (dict(kind="downsample", c=320, f=4, H=16, W=16), {}, {}),
    "downsample_no_gn": (dict(kind="downsample", c=320, f=4, H=16, W=16, gn_groups=0), {}, {}),
    "upsample_phases": (dict(kind="upsample", c=320, f=4, H=16, W=16), {}, dict(paths={"upsample_conv": "four 2x2"})),
    "upsample_phases_off": (dict(kind="upsample", c=320, f=4, H=16, W=16), {"UPSAMPLE_PHASES": [False]},
                            dict(paths={"upsample_conv": "one 3x3"})),
    "upsample_3x3_below_min_hw": (dict(kind="upsample", c=1280, f=4, H=8, W=8), {}, dict(paths={"upsample_conv": "one 3x3"})),
}


@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_sampler_routes(ops_el, monkeypatch, name):
    ops, el = ops_el
    geo, sw, route = SAMPLERS[name]
    out = check("sampler " + name, ops, el, monkeypatch, geo, sw, route)
    if name == "downsample_no_gn":
        assert ops.gn_of(out) is None


@pytest.mark.parametrize("name,geo", [("8x8", dict(kind="write", c=320, f=1, H=8, W=8)),
                                      ("16x16_c640", dict(kind="write", c=640, f=1, H=16, W=16))])
def test_spatial_transformer_write_output_and_bank(ops_el, monkeypatch, name, geo):
    ops, el = ops_el
    check("write " + name, ops, el, monkeypatch, geo, {}, {})


@pytest.mark.parametrize("c,H,W", [(320, 8, 8), (640, 16, 16)])
def test_bank_kv_against_float64(ops_el, monkeypatch, c, H, W):
    ops, el = ops_el
    cs, P, ref = case_and_reference(el, kind="bank_kv", c=c, f=1, H=H, W=W)
    emul = BC.emulated(cs, P, monkeypatch.context)
    got = BC.run(cs, P)
    (e_emul, k_emul), (err, k_err) = BC.bank_kv_errors(cs, emul, ref), BC.bank_kv_errors(cs, got, ref)
    print(f"[bank_kv c={c} {EL_NAME[el]}] e_emul {e_emul[0]:.3g} / {e_emul[1]:.3g} kmax {k_emul:.3g}   kernels {err[0]:.3g} / "
          f"{err[1]:.3g} kmax {k_err:.3g}")
    assert BC.within(err, e_emul, FACTOR)
    # key_norm_max bounds the norms of the STORED keys (census.STAT_BOUNDS["key_norm_max"]); against float64 keys it may
    # sit one element rounding of k away
    want = got[0].double().reshape(-1, BC.HEADS, c // BC.HEADS).norm(dim=-1).amax(dim=0)
    assert census._stat_ratio(got[2], want, census.STAT_BOUNDS["key_norm_max"])[0] <= 1.0
