"""The prologue's kernel routes on a real MI355X against answers that are known exactly (tests/prologue_cases.py), both libraries.

tests/test_gpu_prologue.py checks wav2vec2, AudioProjection, VKpsGuider and the VAE encoder end to end and kernel by kernel on
Gaussian operands (relative L2 <= 4e-3 .. 3e-2); what that lets through is measured in tests/test_prologue_cases_cpu.py.  Here
the operands are small integers from a counter hash of their logical coordinates and the expected output is the exact value
rounded once:

  test           kernel / route                                             bound
  wave           vx_wave_conv1d, `signs` and `rounding`                     bit-equal
  windows        vx_gemm over OVERLAPPING rows (row stride s C below the     bit-equal (`signs`, `rounding`, also behind a GELU
                 row length k C): 128x128 fast, 128x160 gather               of arguments >= 32); `saturated` and `middle` below
  gelu           VX_ACT_GELU in the STORE epilogue of every classic tile     `saturated`: the argument itself from 32 on,
                 and in splitk_reduce_kernel (K = 2560 at 64 rows per        |out| <= 2^-40 alpha (or out == residual) from -32
                 frame), into the element type and into float32              down; `middle`: 0 at 0, else within 5.1e-7 + 2^-24
                                                                             |ref| of float64 (float32) / the element-type
                                                                             value below or above such a result
  positional     Wav2Vec2Model._positional itself: G launches, each a        bit-equal (`signs`, `rounding`, `saturated`), x
                 column slice of y with bias slice, GELU and residual        unchanged
  small_kv d64   vx_small_kv_attention, 16 heads x 64, 15 and 16 keys        attention_cases' `tilted`: one unit in the last place
                 (61,440 and 65,536 bytes of LDS)                            (the other cases: tests/test_gpu_attention_exact.py)

x of the windows is dense (the windows need ld == C) and lies between guard rows of 777; tokens no window reaches hold 2^20
(2^15 in float16).  Every window case also runs with x ending on the buffer's last element.  Outputs, residuals, the plain
linears' A and the positional conv's x are column slices of 777-filled wider buffers whose fill must survive; after every
vx_gemm call the route is asserted as tests/test_gpu_gemm_exact.py does.  References are evaluated with torch on the device.

Largest deviation of the two toleranced cases, measured on an MI355X (both libraries give the same figures):
  gelu `middle` into float32   max |out - float64| = 1.05e-7 over the integer arguments in [-8, 8], every tile and the split-K
                               reduction alike (bound 5.1e-7 + 2^-24 |ref|; the float32 restatement on the CPU gives the same
                               1.05e-7); into bfloat16 / float16 4.05e-3 / 3.98e-4, rounding alone (gelu(3) = 2.99595 is bfloat16 3)
  small_kv d = 64 `tilted`     0 (bound: one unit in the last place)
"""
import contextlib

import pytest
import torch

import attention_cases as A
import prologue_cases as P
from test_gpu_gemm_exact import assert_route, column_slice, fill_intact

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = P.GUARD
GUARD_ROWS = 3


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from v_express_amd import lib as L, ops as o
    return L, o


@pytest.fixture(params=P.ELEMS, ids=lambda e: P.EL_NAME[e])
def ops_el(mods, request):
    L, o = mods
    with L.element_type(request.param):
        yield L, o, request.param


def guarded_rows(t, tail=True):
    """t [rows, C] dense between GUARD_ROWS rows of FILL in front and (tail) behind -> (the whole buffer, the first row's offset)."""
    rows, c = t.shape
    buf = torch.full((GUARD_ROWS + rows + (GUARD_ROWS if tail else 0), c), FILL, dtype=t.dtype, device=DEV)
    buf[GUARD_ROWS:GUARD_ROWS + rows] = t
    return buf, GUARD_ROWS * c


def run_win(L, ops, c, tail=True):
    """One vx_gemm launch of a Win case -> its output; route, guards and the untouched input are asserted here."""
    el = c.el
    x = c.x(DEV).to(el)
    if c.k > 1:                                 # overlapping rows over a dense buffer
        buf, off = guarded_rows(x if tail else x[:c.used], tail)
        a = torch.as_strided(buf, (c.t_out, c.K), (c.s * c.C, 1), off)
        if not tail:
            assert off + (c.t_out - 1) * c.s * c.C + c.K == buf.numel()          # the last window ends on the last element
    else:
        a, buf = column_slice(x)
    before = buf.clone()
    w = c.weight(DEV).reshape(c.n, c.K).to(el).contiguous()
    bias = c.bias(DEV).to(torch.float32)
    res = c.residual_t(DEV)
    res_w = None
    if res is not None:
        res, res_w = column_slice(res.to(el))
    out, wide = column_slice((c.t_out, c.n), torch.float32 if c.out_f32 else el)
    with ops.frame_rows(*c.frame_rows) if c.frame_rows else contextlib.nullcontext(), ops.GemmProfile() as prof:
        ops.gemm(a, w, bias, act=L.VX_ACT_GELU if c.act == "gelu" else L.VX_ACT_NONE, alpha=c.alpha, residual=res, out=out,
                 out_f32=c.out_f32)
    assert len(prof.records) == 1, [r[3] for r in prof.records]
    assert_route(prof.records[0][3], prof.records[0][5], c.key)
    torch.cuda.synchronize()
    assert fill_intact(wide, c.n), f"{c.text()}: the launch wrote beside its output columns"
    assert torch.equal(buf, before) and (res_w is None or fill_intact(res_w, c.n)), f"{c.text()}: the launch wrote into an input"
    return out


def run_all(cases, call):
    failures = [m for m in (c.first_wrong(call(c), DEV) for c in cases) if m]
    assert not failures, f"{len(failures)} cases fail:\n" + "\n".join(failures)


def test_wave(ops_el):
    """vx_wave_conv1d: one time step, 3904 threads (no multiple of 256), 16 taps at stride 3, 300 steps; trailing samples that
    no window may read hold 2^20."""
    L, ops, el = ops_el

    def call(c):
        buf = torch.full((c.samples + 16,), FILL, dtype=torch.float32, device=DEV)
        wave = buf[8:8 + c.samples]
        wave.copy_(c.wave(DEV))
        wbuf = torch.full((c.taps + 2, c.c), FILL, dtype=torch.float32, device=DEV)
        wt = wbuf[1:1 + c.taps]
        wt.copy_(c.weight(DEV))
        got = ops.wave_conv1d(wave, wt, c.stride)
        assert got.shape == (c.t_out, c.c) and got.dtype == el, (c.text(), got.shape, got.dtype)
        return got
    run_all(P.wave_cases(el, DEV), call)


@pytest.mark.parametrize("tail", [True, False], ids=["guard rows behind", "ends on the last element"])
def test_windows(ops_el, tail):
    """vx_gemm over overlapping A rows (lda1 < c1), as the wav2vec2 feature encoder's layers 1..6 launch it."""
    L, ops, el = ops_el
    run_all(P.window_cases(el, DEV), lambda c: run_win(L, ops, c, tail))


def test_gelu(ops_el, capsys):
    """VX_ACT_GELU in the STORE epilogue of every classic tile and in the split-K reduction."""
    L, ops, el = ops_el
    worst = {}

    def call(c):
        out = run_win(L, ops, c)
        if c.kind == "middle":
            key = "float32" if c.out_f32 else P.EL_NAME[el]
            worst[key] = max(worst.get(key, 0.0), float((out.double() - c.exact(DEV)).abs().max()))
        return out
    try:
        run_all(P.gelu_cases(el, DEV), call)
    finally:
        with capsys.disabled():
            print(f"\n[{P.EL_NAME[el]}] gelu middle: largest |out - float64| " + ", ".join(f"into {k}: {v:.4g}" for k, v in worst.items()))


@pytest.mark.parametrize("shape,key", P.POSITIONAL_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_positional(ops_el, shape, key):
    """Wav2Vec2Model._positional with the case's integers in place of the prepared weights: the group-major padded copy, G
    launches into column slices of y, bias slice + GELU + residual slice fused."""
    L, ops, el = ops_el
    from v_express_amd import synth
    from v_express_amd.wav2vec2 import Wav2Vec2Model
    T, H, Gn, kp = shape
    cfg = synth.Wav2Vec2Config(hidden_size=H, num_hidden_layers=0, num_attention_heads=4, conv_dim=(32,) * 7,
                               num_conv_pos_embeddings=kp, num_conv_pos_embedding_groups=Gn)
    m = Wav2Vec2Model(cfg).to("cuda")
    m.load_state_dict(synth.wav2vec2_state_dict(cfg))
    prepared = m._prepared()
    failures = []
    for c in (c for c in P.positional_cases(el, DEV) if (c.T, c.H, c.G, c.kp) == shape):
        assert c.key == key
        w = c.weight(DEV).to(el)                                                # [H, kp, cg]
        prepared["pos_w"] = [w[g * c.cg:(g + 1) * c.cg].reshape(c.cg, c.K).contiguous() for g in range(Gn)]
        prepared["pos_b"] = c.bias(DEV).to(torch.float32).contiguous()
        x, wide = column_slice(c.x(DEV).to(el))
        before = wide.clone()
        with ops.GemmProfile() as prof:
            got = m._positional(x)
        assert len(prof.records) == Gn, [r[3] for r in prof.records]
        for r in prof.records:
            assert_route(r[3], r[5], c.key)
            assert r[4] == (T, c.cg, c.K), r[4]
        torch.cuda.synchronize()
        assert torch.equal(wide, before), f"{c.text()}: x changed"
        assert got.shape == (T, H) and got.dtype == el
        msg = c.first_wrong(got, DEV)
        if msg:
            failures.append(msg)
    assert not failures, f"{len(failures)} cases fail:\n" + "\n".join(failures)


def test_small_kv_d64_tilted(ops_el, capsys):
    """AudioProjection's shape through vx_small_kv_attention, K and V as column halves of one buffer: the softmax scale (the
    other cases of these shapes run in tests/test_gpu_attention_exact.py); prints the largest deviation."""
    L, ops, el = ops_el
    worst, failures = 0.0, []
    for g in A.small_kv_geoms(64):
        case = [c for c in A.cases(g, el) if c.name == "tilted"][0]
        kv = torch.full((g.batch * g.n_kv, 2 * g.heads * g.d + 24), FILL, dtype=el, device=DEV)
        view = kv[:, 8:8 + 2 * g.heads * g.d]
        view.copy_(A.pack_kv(case))
        q, _ = column_slice(case.q.to(DEV))
        out, wide = column_slice((g.batch * g.n_q, g.heads * g.d), el)
        ops.small_kv_attention(q, view, batch=g.batch, n_q=g.n_q, n_kv=g.n_kv, heads=g.heads, head_dim=g.d, out=out)
        torch.cuda.synchronize()
        assert fill_intact(wide, g.heads * g.d)
        worst = max(worst, case.deviation(out))
        msg = case.first_wrong(out)
        if msg:
            failures.append(msg)
    with capsys.disabled():
        print(f"\n[{P.EL_NAME[el]}] small_kv d = 64 tilted: largest |out - expected| {worst:.4g}")
    assert not failures, "\n".join(failures)
