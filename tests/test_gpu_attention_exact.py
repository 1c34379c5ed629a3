"""Attention kernels on a real MI355X against answers that are known exactly (tests/attention_cases.py), both libraries.

The Gaussian attention tests (test_gpu_kernels.py, test_gpu_f16.py, test_gpu_guard_bands.py) accept max|err| <= 2^-6 max|ref|
and relative L2 <= 1e-2.  A kernel that counts one padded key in the row sum of a ragged last key tile stays inside that from
65 keys upwards, and none of them has more than one key batch under q_per_kv > 1 (tests/test_attention_cases_cpu.py shows
both on the CPU).  Here every case has an answer that does not depend on the arithmetic:

  case      bound                                                       what it pins
  counted   bit-equal                                                   who is in the row sum (q = 0: the mean of n_kv integers)
  unity     |out - 1| <= 2^-8 (bfloat16) / 2^-11 (float16)              numerator and denominator see the same keys (V = 1)
  routing   bit-equal to V[pi(query)]                                   which key, which head, which key batch; also scale = 0
  tilted    |out - float64| <= one unit in the last place of expected   the softmax scale (two exact logit levels)

Deviation |out - expected| that the CPU emulations of legitimate designs leave (P rounded to the element type before PV with
the row sum from the unrounded P; the same under a shift 6 bits above the row maximum; the row sum from the rounded P), the
largest over every shape below (tests/test_attention_cases_cpu.py prints them):
  bfloat16  counted 0, unity (qs = 0.25 and 1) 0, routing 0, routing prescaled 0, tilted 0
  float16   counted 0, routing 0, routing prescaled 0; unity 2^-11 (d = 160, qs = 0.25, row sum from the unrounded P: the tie
            below 1.0, the whole bound) and 0 elsewhere; tilted 2^-10 (d = 64: the float64 answer lies next to a rounding
            boundary of [1, 2), so the neighbouring value - one unit, the whole bound - is a correct rounding too) and 0 elsewhere
Routes (the kernel vx_last_kernel() names is asserted after every call), key tile 64 everywhere:
  vx_attention / vx_attention_bounded   n_kv in {1, 7, 63, 64, 65, 100, 129, 200} x n_q in {1, 65, 100}, 8 heads, batch 4 with
      q_per_kv = 2 - TWO key batches; q and k are column slices of wider buffers, as the model passes them.
      d = 8 attn_kernel<1, 2, 4>; d = 40 exact attn2_kernel (ops._BOUNDED_SOFTMAX off); d = 40 bounded attn3_kernel with the key-norm
      table computed inside and passed in, plain and prescaled keys; d = 64, d = 80 (plain and prescaled), d = 160 attn_kernel;
      d = 512 with one head, one batch, n_kv in {65, 100}.
  vx_temporal_attention   f in {1, 2, 15, 16, 17, 24, 31, 32} x d in {8, 40, 80, 160}, hw = 5, b = 2, 8 heads.
  vx_small_kv_attention   n_kv in {1, 5, 15, 16} x d in {8, 40, 160} x n_q in {7, 100}, batch 3 (one kernel: nothing to route,
      and the entry point does not set vx_last_kernel); d = 64 with 16 heads, AudioProjection's shape: n_kv in {15, 16} x n_q
      in {5, 100} - 61,440 and 65,536 of the 65,536 bytes of LDS the entry point admits.
"""
import pytest
import torch

import attention_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 777.0        # what the wider buffers hold beside the q / k columns: a read of the wrong columns shows


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from v_express_amd import lib as L, ops as o
    return L, o


@pytest.fixture(params=A.ELEMS, ids=lambda e: A.EL_NAME[e])
def ops_el(mods, request):
    """(ops, element type): every test runs on the bfloat16 and on the float16 library (tests/test_gpu_guard_bands.py::ops_el)."""
    L, o = mods
    with L.element_type(request.param):
        yield o, request.param


def last_kernel(ops):
    return ops._lib.vx_last_kernel().decode()


def column_slice(t):
    """t [rows, C] on the device as columns 8 .. 8 + C of a [rows, C + 24] buffer: a row stride above the width and a base 16
    bytes into a row - the alignment the ABI promises, no more."""
    wide = torch.full((t.shape[0], t.shape[1] + 24), FILL, dtype=t.dtype, device=DEV)
    view = wide[:, 8:8 + t.shape[1]]
    view.copy_(t)
    return view


def vt_of(ops, case):
    g = case.geom
    vt = ops.alloc_vt(A.kv_batches(g), g.heads, g.d, g.n_kv, DEV)      # (the pitch padding beyond n_kv is zero)
    return A.pack_vt(case.v, g, vt.shape[-1], like=vt)


def run_attention(ops, case, kmax=None):
    g = case.geom
    q, k, vt = column_slice(case.q), column_slice(case.k), vt_of(ops, case)
    out = ops.attention(q, k, vt, batch=g.batch, heads=g.heads, n_q=g.n_q, n_kv=g.n_kv, head_dim=g.d, q_per_kv=g.q_per_kv,
                        kmax=kmax(k) if kmax else None, k_prescaled=case.prescaled)
    return out


def run_cases(geoms, el, call, prescaled=False):
    """Every case of every geometry through `call(case) -> output`; the first wrong element of each failing (shape, case)."""
    failures = []
    for g in geoms:
        for case in A.cases(g, el, prescaled):
            msg = case.first_wrong(call(case))
            if msg:
                failures.append(msg)
    assert not failures, f"{len(failures)} (shape, case) pairs fail:\n" + "\n".join(failures)


ATTN_KERNEL = {8: "attn_kernel<1, 2, 4, true, 2>", 64: "attn_kernel<2, 4, 2, true, 2>", 80: "attn_kernel<3, 5, 2, true, 2>",
               160: "attn_kernel<5, 10, 2, false, 2>", 512: "attn_kernel<16, 32, 1, false, 1>"}


@pytest.mark.parametrize("d,prescaled", [(8, False), (64, False), (80, False), (80, True), (160, False), (512, False)])
def test_plain_kernel(ops_el, d, prescaled):
    """attn_kernel: keys beyond n_kv are ZEROS in its last tile and only the -inf mask keeps them out of the row sum."""
    ops, el = ops_el

    def call(case):
        out = run_attention(ops, case)
        assert last_kernel(ops) == ATTN_KERNEL[d], last_kernel(ops)
        return out
    run_cases(A.attention_geoms(d), el, call, prescaled)


def test_attn2_exact_d40(ops_el):
    """d = 40 with the bounded softmax off: attn2_kernel, online softmax, row sums out of the PV MFMA's ones row."""
    ops, el = ops_el

    def call(case):
        out = run_attention(ops, case)
        assert last_kernel(ops) == "attn2_kernel<2, 3, 2, true, false>", last_kernel(ops)
        return out
    saved = ops._BOUNDED_SOFTMAX[0]
    try:
        ops._BOUNDED_SOFTMAX[0] = False
        run_cases(A.attention_geoms(40), el, call)
    finally:
        ops._BOUNDED_SOFTMAX[0] = saved


@pytest.mark.parametrize("prescaled", [False, True], ids=["plain", "prescaled"])
@pytest.mark.parametrize("table", ["inside", "passed"])
def test_attn3_bounded_d40(ops_el, table, prescaled):
    """d = 40 under the bounded softmax: attn3_kernel (its UNIT variant for prescaled keys), the key-norm table computed
    inside ops.attention or by vx_key_norm_max beforehand and passed in."""
    ops, el = ops_el
    assert ops._BOUNDED_SOFTMAX[0], "the bounded softmax is the default"

    def call(case):
        g = case.geom
        kmax = (lambda k: ops.key_norm_max(k, kv_batches=A.kv_batches(g), heads=g.heads, n_kv=g.n_kv, head_dim=g.d)) \
            if table == "passed" else None
        out = run_attention(ops, case, kmax)
        name = last_kernel(ops)
        assert name.startswith("attn3_kernel<") and name[:-1].split(", ")[2] == ("true" if prescaled else "false"), name
        return out
    run_cases(A.attention_geoms(40), el, call, prescaled)


@pytest.mark.parametrize("d", A.TEMPORAL_HEAD_DIMS)
def test_temporal(ops_el, d):
    """vx_temporal_attention over f frames per (batch, pixel, head): one and two 16-frame tiles, both block widths."""
    ops, el = ops_el
    b, hw, heads = 2, 5, 8
    kk = (d + 31) // 32

    def call(case):
        f = case.geom.n_q
        qkv = column_slice(A.pack_qkv(case, b, f, hw))
        out = ops.temporal_attention(qkv, b=b, f=f, hw=hw, heads=heads, head_dim=d)
        ft = 1 if f <= 16 else 2
        want = f"temporal_attn_kernel<{kk}, {2 * kk}, {ft}, {8 if kk * ft <= 6 else 4}>"
        assert last_kernel(ops) == want, (last_kernel(ops), want)
        # rows (b f) hw -> the builders' (b hw) f
        return out.reshape(b, f, hw, -1).permute(0, 2, 1, 3).reshape(b * hw * f, -1)
    run_cases(A.temporal_geoms(d, b, hw), el, call)


@pytest.mark.parametrize("d", A.SMALL_KV_HEAD_DIMS)
def test_small_kv(ops_el, d):
    """vx_small_kv_attention: one key to its limit of 16, K | V columns of one tensor."""
    ops, el = ops_el

    def call(case):
        g = case.geom
        return ops.small_kv_attention(column_slice(case.q), column_slice(A.pack_kv(case)), batch=g.batch, n_q=g.n_q,
                                      n_kv=g.n_kv, heads=g.heads, head_dim=d)
    run_cases(A.small_kv_geoms(d), el, call)
