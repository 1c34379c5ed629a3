"""vx_gemm with fp8 operands (a_fp8 = 1) on a real MI355X against answers that are known exactly (tests/fp8_gemm_cases.py), both
libraries, every fp8 route.

The Gaussian fp8 tests (test_gpu_kernels.py::test_gemm_fp8_store_and_split, ::test_gemm_fp8_ring_vs_classic_tiles) accept both
subnormal flushes, a truncating or round-half-away store, a scale product formed in the element type, an early rounding of the
dequantised accumulator and, at K = 320, a dropped half K tile (tests/test_fp8_gemm_cases_cpu.py measures it), and never ran a
column tail, a rowbias or a sequence that ends inside a tile.  Here:

  case        bound                                                  what it pins
  pow2        equal (gemm_cases' signs / rounding / saturated as     the decode, the scale indices, the scale placement in front
              e4m3 bytes with power-of-two scales)                   of the bias, the epilogue order, ONE round-to-nearest-even
  scales      the derived interval `band()`: equal wherever the      a scale product formed in float32, not in the element type
              float32 error cannot reach a rounding boundary
  products    equal (float16: less the pairs with a subnormal        the decode of all 254 finite bytes on both operands,
              result, `left_out`)                                    subnormals and both zeros
  chained     equal; every a_scale and w_scale == 2^-6               ops.quantize_fp8 / ops.fp8_weight pad and scale as the GEMM reads

Everything but the library call is tests/fp8_gemm_harness.py, which tests/test_fp8_gemm_cases_cpu.py drives on the host with a
stand-in for the kernel at these shapes: the operands' layout (q 16 bytes into the rows of a wider sentinel-filled buffer;
output, residual and the SPLIT row parts column slices of buffers of 777; the rowbias the middle third of a wider table; the
V^T pitch padding zero), the reference evaluated with torch on the device at the full shape, the judging, the fill checks.  The
function handed to it here makes the call and asserts the route twice: vx_gemm_config_name's key (ops.GemmProfile) must be the
one fp8_gemm_cases.ROUTES states and vx_last_kernel() that key's instantiation (fp8_gemm_cases.KERNELS).
"""
import pytest
import torch

import fp8_gemm_cases as P
import fp8_gemm_harness as H
import gemm_cases as G

pytestmark = pytest.mark.gpu
DEV = "cuda"


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


def library(L, ops):
    """The one function that calls the library: the launch of an fp8_gemm_harness.Call, and the route it took."""
    def launch(call):
        a, w = ops.Fp8Rows(call.q, call.a_scale, call.k), ops.Fp8Weight(call.w8, call.w_scale, call.k)
        with ops.GemmProfile() as prof:
            if call.parts:
                ops.gemm_split(a, w, call.bias, call.parts, part_cols=call.part_cols, seq_len=call.seq_len, head_dim=call.head_dim)
            else:
                ops.gemm(a, w, call.bias, residual=call.residual, alpha=call.alpha,
                         act=L.VX_ACT_SILU if call.silu else L.VX_ACT_NONE, rowbias=call.rowbias,
                         rows_per_group=call.rows_per_group, out=call.out)
        gemms = [r for r in prof.records if len(r) == 7 and isinstance(r[4], tuple)]
        assert len(gemms) == 1, [r[3] for r in prof.records]
        key, sym = gemms[0][3], ops._lib.vx_last_kernel().decode()
        assert key == call.key, f"route moved: vx_gemm_config_name says {key}, the case list says {call.key}"
        assert sym == gemms[0][5] == P.kernel_of(key, call.residual is not None), (key, sym, gemms[0][5])
        torch.cuda.synchronize()
    return launch


class ring_requested:
    """ops.FP8_RING[0] = True (vx_gemm_params.ring_hint = 3) for the routes of fp8_gemm_cases.RING_ROUTES."""

    def __init__(self, ops, on):
        self.ops, self.on = ops, on

    def __enter__(self):
        self.saved = self.ops.FP8_RING[0]
        self.ops.FP8_RING[0] = bool(self.on)

    def __exit__(self, *a):
        self.ops.FP8_RING[0] = self.saved


@pytest.mark.parametrize("route", sorted(P.ROUTES))
def test_route(ops_el, route):
    """Every case of every launch of the route, and `in_place` on STORE; all failing (route, shape, case) triples with their
    first wrong element."""
    L, ops, el = ops_el
    with ring_requested(ops, route in P.RING_ROUTES):
        failures, made = H.run_route(route, el, library(L, ops), DEV)
    assert made >= 2 * len(P.ROUTES[route])
    assert not failures, f"{len(failures)} (route, shape, case) triples fail:\n" + "\n".join(failures)


def test_products(ops_el):
    """All 254 x 256 pairs of finite bytes on the classic 128 x 160 tile.  The persistent kernel takes whole 256 x 320 tiles
    only (vx_gemm_ring_eligible: n % 320 == 0, so not the table's first 256 columns): its variant is 256 x 320, rows and
    columns repeating from the 255th on as the builder repeats them - every pair is there again."""
    L, ops, el = ops_el
    st = P.ROUTES["128x160 store"][0].key
    ring = P.ROUTES["ring store"][0].key
    assert P.kernel_of(st, False).startswith("gemm_kernel<128, 160,") and P.kernel_of(ring, False).startswith("gemm_ring_kernel<")
    for geo, key in ((P.PRODUCTS_GEO, st), (P.PRODUCTS_RING_GEO, ring)):
        with ring_requested(ops, key == ring):
            msg = H.run_case(P.products(el, DEV, geo=geo), key, library(L, ops), DEV)
        assert msg is None, f"{key}: {msg}"


@pytest.mark.parametrize("m,n,k", P.CHAINED)
def test_chained(ops_el, m, n, k):
    """ops.quantize_fp8 and ops.fp8_weight feeding the GEMM at logical K = 40, 320, 640 (K padding 88, 64, 0)."""
    L, ops, el = ops_el

    def produce(x, w):
        a8, w8 = ops.quantize_fp8(x), ops.fp8_weight(w)
        assert a8.q.shape == (m, P.pad128(k)) and w8.w8.shape == (n, P.pad128(k)) and bool((a8.q[:, k:] == 0).all()) \
            and bool((w8.w8[:, k:] == 0).all()), "the K padding is not zero bytes"
        return ops.gemm(a8, w8, None), a8.scale, w8.scale
    ops.clear_caches()                  # (fp8_weight caches by address)
    try:
        msg = H.judge_chained(m, n, k, el, DEV, produce)
    finally:
        ops.clear_caches()
    assert msg is None, msg


def test_refusals(ops_el):
    """n = 4: vx_gemm takes n % 8 == 0 only, whatever the operand type (no fp8 producer of the model has another n), and the
    refused launch writes nothing.  A rowbias table that does not cover the last row's group never reaches the kernel, which
    reads rowbias + (row // rows_per_group) * rowbias_ld unchecked."""
    L, ops, el = ops_el
    z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
    one = lambda n: torch.ones(n, dtype=torch.float32, device=DEV)
    wide = torch.full((8, 32), H.FILL, dtype=el, device=DEV)
    with pytest.raises(L.VxError, match="multiple of 8"):
        ops.gemm(ops.Fp8Rows(z(8, 128), one(8), 128), ops.Fp8Weight(z(4, 128), one(4), 128), None, out=wide[:, 8:12])
    torch.cuda.synchronize()
    assert bool((wide == H.FILL).all()), "a refused launch wrote its output"
    a, w = ops.Fp8Rows(z(130, 128), one(130), 128), ops.Fp8Weight(z(160, 128), one(160), 128)
    out = torch.full((130, 160), H.FILL, dtype=el, device=DEV)
    table = torch.zeros(9, 160, dtype=torch.float32, device=DEV)             # 130 rows in groups of 16: 9 groups
    for rowbias, rpg in ((table[:8], 16), (table, 0), (table, -16), (table[:, :152], 16)):
        with pytest.raises(ValueError, match="rowbias"):
            ops.gemm(a, w, None, rowbias=rowbias, rows_per_group=rpg, out=out)
    torch.cuda.synchronize()
    assert bool((out == H.FILL).all()), "a refused launch wrote its output"
    ops.gemm(a, w, None, rowbias=table, rows_per_group=16, out=out)          # the whole table: accepted
    assert bool((out == 0).all())
