"""vx_gemm on a real MI355X against answers that are known exactly (tests/gemm_cases.py), both libraries, every route.

The Gaussian GEMM tests accept max|err| <= 2^-7 max|ref| and relative L2 <= 6e-3: a truncating store, a double rounding in front
of the residual or one wrong K-term at the long-K shapes stays inside (tests/test_gemm_cases_cpu.py measures it).  Here the
operands are small integers from a counter hash of their logical coordinates: every partial sum is exact in float32, the
expected output is the exact value rounded once, and every tile, pipeline depth, split and route must give the same bits.

  case        bound                                                  what it pins
  signs       equal                                                  every K-term, tap, channel, frame, row, bias and rowbias index
  rounding    equal (>= 1/4 ties, >= 1/4 other roundings)            round-to-nearest-even, ONE rounding, the residual behind it
  saturated   equal; |out| <= 2^-40 alpha (SiLU) / 2^-30 (GEGLU)     that the activation runs, on which columns, the value / gate
              where the argument is <= -32 and there is no residual  pairing of the 8-row interleave, where alpha and the residual act
  folded      equal                                                  rstd (acc - mean colsum) + bias with hand-made statistics
  statistics  equal (sums of squares past 2^24: N 2^-24 relative)    GroupNorm partial sums per slab and the two-part row sums, of the
                                                                     STORED values

The reference is gemm_cases' float64 restatement evaluated with torch on the device at the full shape (its builders assert
their conditions there).  A, the residual, the output and the SPLIT row parts are column slices of wider buffers filled with
777, and the fill must still be there afterwards.  After every call the route is asserted twice: vx_gemm_config_name's key
(ops.GemmProfile) must be the one gemm_cases.ROUTES states, and vx_last_kernel() must be that key's instantiation - a policy
change then fails loudly instead of moving a case to another kernel.  The routes and their shapes are gemm_cases.ROUTES.
"""
import contextlib
import re

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 777.0


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from v_express_amd import lib as L, ops as o
    return L, o


@pytest.fixture(params=G.ELEMS, ids=lambda e: G.EL_NAME[e])
def ops_el(mods, request):
    """(lib module, ops, element type): every test runs on the bfloat16 and on the float16 library."""
    L, o = mods
    G.clear_cache()
    with L.element_type(request.param):
        yield L, o, request.param
    G.clear_cache()


def column_slice(t, dtype=None):
    """t [rows, C] as columns 8 .. 8 + C of a [rows, C + 24] buffer of FILL (None: an output of that shape): a row stride above
    the width and a base 16 bytes into a row - the alignment the ABI promises, no more."""
    rows, c = t.shape if isinstance(t, torch.Tensor) else t
    wide = torch.full((rows, c + 24), FILL, dtype=dtype or t.dtype, device=DEV)
    view = wide[:, 8:8 + c]
    if isinstance(t, torch.Tensor):
        view.copy_(t)
    return view, wide


def fill_intact(wide, c):
    return bool((wide[:, :8] == FILL).all()) and bool((wide[:, 8 + c:] == FILL).all())


def assert_route(key, sym, want):
    """The key vx_gemm_config_name gave is the stated one, and vx_last_kernel() is that key's instantiation."""
    assert key == want, f"route moved: vx_gemm_config_name says {key}, the case list says {want}"
    fam, bm, bn, epi, addr = re.fullmatch(r"(gemm_ring_kernel|gemm_kernel)<(\d+)x(\d+)x64,\dw,(STORE|GEGLU|SPLIT),(fast|gather).*>",
                                          key).groups()
    name, args = sym[:-1].split("<")
    args = [a.strip() for a in args.split(",")]
    assert name == fam, (key, sym)
    e = str(("STORE", "GEGLU", "SPLIT").index(epi))
    if fam == "gemm_ring_kernel":           # <EPI, RES, F8, STATS, LNF, GNS[, SK]>
        assert args[0] == e and (len(args) > 6) == key.endswith(",coop2>"), (key, sym)
    else:                                   # <BM, BN, WARPS_M, WARPS_N, STAGES, EPI, FAST, F8, LNF, GNS>
        assert args[:2] == [bm, bn] and args[5] == e and args[6] == ("true" if addr == "fast" else "false"), (key, sym)


def run(L, ops, case, lch, monkeypatch):
    """One launch of `case` under the launch's knobs -> (name -> output tensor, slab rows of the GroupNorm sums)."""
    g, el = case.geo, case.el
    t = G.kernel_operands(case, DEV)
    H, W = (g.h + 2, g.w + 2) if g.bordered else (g.h, g.w)
    a1, _ = column_slice(t["a1"].view(-1, g.c1))
    a2 = column_slice(t["a2"].view(-1, g.c2))[0] if g.c2 else None
    plain = g.nb == 1 and g.w == 1 and g.kk == 1
    geom, offset = None, 0
    if not plain:
        if g.window:
            geom = ops.ConvGeom(g.nb, H, W, g.kk, g.kk, g.stride, 0, out_hw=g.window[2:])
            offset = g.window[0] * g.stride * W + g.window[1] * g.stride
        else:
            geom = ops.ConvGeom(g.nb, H, W, g.kk, g.kk, g.stride, g.pad, g.ups, g.pad_end)
        assert (geom.h_out, geom.w_out) == g.out_hw and geom.m == g.m
    if lch.ring_mode is not None:
        monkeypatch.setattr(ops, "RING_MODE", [lch.ring_mode])
    if lch.coop_min_k is not None:
        monkeypatch.setattr(ops, "COOP_MIN_K", [lch.coop_min_k])
    got, slab_rows, fills = {}, 128, []
    res = None
    if t["residual"] is not None:
        res, _ = column_slice(t["residual"])
    with ops.frame_rows(*lch.frame_rows) if lch.frame_rows else contextlib.nullcontext(), ops.GemmProfile() as prof:
        if g.epi == "geglu":
            out, wide = column_slice((g.m, g.n_out), el)
            fills.append((wide, g.n_out))
            ops.geglu(a1, t["w"], t["bias"], out=out, ln=t["ln"])
            got["out"] = out
        elif g.epi == "split":
            pc = g.n // 3
            q, wq = column_slice((g.m, pc), el)
            k, wk = column_slice((g.m, pc), el)
            fills += [(wq, pc), (wk, pc)]
            if g.seq_len:
                d = pc // g.heads
                vt = ops.alloc_vt(g.m // g.seq_len, g.heads, d, g.seq_len, DEV)
                last = ("vt", vt)
            else:
                v, wv = column_slice((g.m, pc), el)
                fills.append((wv, pc))
                last = ("rows", v)
            ops.gemm_split(a1, t["w"], t["bias"], [("rows", q), ("rows", k), last], part_cols=pc, seq_len=g.seq_len,
                           head_dim=pc // g.heads if g.seq_len else 0, ln=t["ln"])
            got["q"], got["k"] = q, k
            if g.seq_len:
                got["vt"] = vt[..., :g.seq_len]
                assert bool((vt[..., g.seq_len:] == 0).all()), "the pitch padding of V^T must stay zero"
            else:
                got["v"] = last[1]
        else:
            out, wide = column_slice((g.m, g.n), torch.float32 if g.out_f32 else el)
            fills.append((wide, g.n))
            w = t["w"].view(g.groups, g.n, g.k) if g.groups > 1 else t["w"]
            rowbias = None
            if t["rowbias"] is not None:                      # a strided view, like the time-embedding slices
                rb3 = torch.full((t["rowbias"].shape[0], 3 * g.n), FILL, dtype=torch.float32, device=DEV)
                rowbias = rb3[:, g.n:2 * g.n]
                rowbias.copy_(t["rowbias"])
            st = torch.full((g.m, 4), float("nan"), device=DEV) if g.stats2 else None
            ops.gemm(a1, w, t["bias"], geom=geom, a2=a2, residual=res, alpha=case.alpha,
                     act=L.VX_ACT_SILU if case.act == "silu" else L.VX_ACT_NONE, rowbias=rowbias, rows_per_group=g.rows_per_group,
                     out=out, out_f32=g.out_f32, ln=t["ln"], stats_out=st, w_group_rows=g.m // g.groups if g.groups > 1 else 0,
                     gn=(32, g.gn_hw) if g.gn_hw else None, a_pixel_offset=offset)
            got["out"] = out
            if g.gn_hw:
                gst = ops.gn_of(out)
                assert gst is not None and gst.fits(g.m // g.gn_hw, g.gn_hw, 32, g.n), "the launch left no GroupNorm sums"
                slab_rows = g.gn_hw // gst.slabs
                got["gn sums"], got["gn squares"] = gst.ws[..., 0], gst.ws[..., 1]
                got["gn total sums"], got["gn total squares"] = gst.ws[..., 0].double().sum(dim=1), gst.ws[..., 1].double().sum(dim=1)
            if g.stats2:
                got["row sums"], got["row squares"] = st[:, 0::2], st[:, 1::2]
    gemms = [r for r in prof.records if len(r) == 7 and isinstance(r[4], tuple)]
    assert len(gemms) == 1, [r[3] for r in prof.records]
    assert_route(gemms[0][3], gemms[0][5], lch.key)
    assert ops._lib.vx_last_kernel().decode() == gemms[0][5] or g.stats2       # (vx_row_stats_parts may follow the GEMM)
    torch.cuda.synchronize()
    for wide, c in fills:
        assert fill_intact(wide, c), f"{case.name} {g.text()}: the launch wrote beside its output columns"
    return got, slab_rows


def run_route(ops_el, monkeypatch, launches, repeat=1):
    """Every applicable case of every launch; all failing (route, shape, case) triples with their first wrong element."""
    L, ops, el = ops_el
    failures = []
    for lch in launches:
        for case in G.cases(lch.geo, el, DEV, skip=lch.skip):
            for _ in range(repeat):
                got, slab_rows = run(L, ops, case, lch, monkeypatch)
                msg = case.first_wrong(got, case.expected(DEV, slab_rows=slab_rows))
                if msg:
                    failures.append(f"{lch.key}: {msg}")
                    break
        G.clear_cache()
    assert not failures, f"{len(failures)} (route, shape, case) triples fail:\n" + "\n".join(failures)


@pytest.mark.parametrize("route", [r for r in sorted(G.ROUTES) if not r.startswith("coop")])
def test_route(ops_el, monkeypatch, route):
    run_route(ops_el, monkeypatch, G.ROUTES[route])


@pytest.mark.parametrize("route", ["coop", "coop conv"])
def test_cooperative_split(ops_el, monkeypatch, route):
    """The two K halves of a tile on two CUs that meet inside the launch: 15 frames (partner pairs on different XCDs), 16 and
    32; every case three times on the same workspace (the rendezvous words carry the launch's epoch)."""
    run_route(ops_el, monkeypatch, G.ROUTES[route], repeat=3)


def test_every_route_gives_the_same_bits(ops_el, monkeypatch):
    """One `signs` and one `rounding` problem (24576 x 640 x 2560, with residual) on the persistent kernel, the classic 128 x 160
    tile, the cooperative split and classic split-K: all four outputs bit-identical (the Gaussian tests compare these routes
    within 2^-6), and equal to the exact answer."""
    L, ops, el = ops_el
    for build in (G.signs, G.rounding):
        case = build(G.CROSS[0].geo, el, DEV, residual=True)
        want = case.expected(DEV)
        outs = []
        for lch in G.CROSS:
            with monkeypatch.context() as mp:
                got, _ = run(L, ops, case, lch, mp)
            outs.append(got["out"].clone())
            msg = case.first_wrong(got, want)
            assert msg is None, f"{lch.key}: {msg}"
        for lch, o in zip(G.CROSS[1:], outs[1:]):
            assert torch.equal(o.view(torch.int16), outs[0].view(torch.int16)), f"{lch.key} and {G.CROSS[0].key} differ in bits"
