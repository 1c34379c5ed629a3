"""Everything tests/test_gpu_fp8_gemm_exact.py does except the library call, on any device.

The fp8 cases (tests/fp8_gemm_cases.py) are laid out for a launch - operands in the least alignment the ABI promises, every
destination inside guard columns -, handed to ONE function that is passed in (`launch(call)`: the GPU file's calls ops.gemm /
ops.gemm_split and asserts the route, tests/test_fp8_gemm_cases_cpu.py passes a stand-in that is float32 arithmetic on the
host), judged by the case's own bound and checked for intact fills.  So the whole path of the GPU file but the kernel runs on
the CPU at the full shapes first: an index that leaves its table is an IndexError there, not an aborted indexing kernel on a GPU.

Layout of a launch (`build`):
  q          columns 16 .. 16 + Kp of a uint8 [m, Kp + 48] buffer of SENTINEL bytes (a finite, nonzero e4m3 value: a kernel that
             reads beside its rows gets other sums): row stride above Kp and a multiple of 16, base 16 bytes into a row
  w8         contiguous [n, Kp] (the kernel's weight stride is K itself); a_scale [m], w_scale [n], bias [n] float32 contiguous
  out, residual, the SPLIT row parts
             columns 8 .. 8 + C of [m, C + 24] buffers of FILL (test_gpu_gemm_exact.column_slice)
  rowbias    the middle third of a float32 [groups, 3 n] buffer of FILL
  V^T        [sequences, heads, d, pitch], pitch = seq_len rounded up to 8: the padding zero, and zero afterwards
  in place   (what the out projections pass) out IS the residual view; the expected value is the case's, which is shown to
             be what the residual buffer held before the launch
Afterwards every fill, the q bytes, the scales and - unless in place - the residual must be what they were.
"""
from dataclasses import dataclass, field
from typing import Optional

import torch

import fp8_gemm_cases as P
import gemm_cases as G

FILL = 777.0
SENTINEL = 0x55            # e4m3 13.0


@dataclass
class Call:
    """One launch as the function passed in gets it.  STORE: out[m, n] = residual + alpha * act(q w8^T a_scale w_scale + bias +
    rowbias[row // rows_per_group]); SPLIT: parts = [("rows", q), ("rows", k), ("rows", v) | ("vt", vt)] of part_cols columns."""
    case: P.Fp8Case
    key: str                            # the route key fp8_gemm_cases.ROUTES states for the launch
    q: torch.Tensor
    a_scale: torch.Tensor
    w8: torch.Tensor
    w_scale: torch.Tensor
    k: int                              # the logical K (q and w8 are padded to a multiple of 128)
    bias: Optional[torch.Tensor] = None
    rowbias: Optional[torch.Tensor] = None
    rows_per_group: int = 0
    residual: Optional[torch.Tensor] = None
    alpha: float = 1.0
    silu: bool = False
    out: Optional[torch.Tensor] = None
    parts: list = field(default_factory=list)
    part_cols: int = 0
    seq_len: int = 0
    head_dim: int = 0
    in_place: bool = False
    guards: list = field(default_factory=list)         # (name, wide buffer, first column, columns, fill)
    kept: list = field(default_factory=list)           # (name, tensor, its clone before the launch)


def column_slice(t, dev, dtype=None):
    """t [rows, C] (or its shape: an output) -> (columns 8 .. 8 + C of a [rows, C + 24] buffer of FILL, the buffer)."""
    rows, c = t.shape if isinstance(t, torch.Tensor) else t
    wide = torch.full((rows, c + 24), FILL, dtype=dtype or t.dtype, device=dev)
    view = wide[:, 8:8 + c]
    if isinstance(t, torch.Tensor):
        view.copy_(t)
    return view, wide


def build(case, key, dev, in_place=False):
    """The Call of a case: operands from `kernel_operands` in the layout of the module docstring."""
    g, el = case.geo, case.el
    t = case.kernel_operands(dev)
    m, kp = t["q"].shape
    assert (m, kp) == (g.m, case.kp) and t["w8"].shape == (g.n, kp)
    q_wide = torch.full((m, kp + 48), SENTINEL, dtype=torch.uint8, device=dev)
    q = q_wide[:, 16:16 + kp]
    q.copy_(t["q"])
    assert q.stride(0) % 16 == 0 and q.stride(0) > kp and q.storage_offset() == 16
    call = Call(case, key, q, t["a_scale"].contiguous(), t["w8"].contiguous(), t["w_scale"].contiguous(), g.k,
                bias=t["bias"], alpha=case.base.alpha, silu=case.base.act == "silu", in_place=in_place)
    call.guards.append(("q", q_wide, 16, kp, SENTINEL))
    call.kept += [("q", q, t["q"]), ("a_scale", call.a_scale, call.a_scale.clone()), ("w_scale", call.w_scale, call.w_scale.clone()),
                  ("w8", call.w8, call.w8.clone())]

    def guarded(name, src, dtype=None):
        view, wide = column_slice(src, dev, dtype)
        call.guards.append((name, wide, 8, view.shape[1], FILL))
        return view
    if t["rowbias"] is not None:
        rb = t["rowbias"]
        assert g.rows_per_group > 0 and rb.shape[0] * g.rows_per_group >= g.m, (g.m, g.rows_per_group, tuple(rb.shape))
        rb3 = torch.full((rb.shape[0], 3 * g.n), FILL, dtype=torch.float32, device=dev)
        call.rowbias, call.rows_per_group = rb3[:, g.n:2 * g.n], g.rows_per_group
        call.rowbias.copy_(rb)
        call.guards.append(("rowbias", rb3, g.n, g.n, FILL))
        call.kept.append(("rowbias", call.rowbias, rb))
    if t["residual"] is not None:
        call.residual = guarded("residual", t["residual"])
        # the expected outputs are the case's: they hold for this launch because the buffer holds the case's residual
        assert torch.equal(call.residual.to(G.F64), case.base.residual_t(dev)), "the residual is not exact in the element type"
        if not in_place:
            call.kept.append(("residual", call.residual, t["residual"]))
    if g.epi == "split":
        pc = g.n // 3
        call.part_cols, call.seq_len, call.head_dim = pc, g.seq_len, pc // g.heads if g.seq_len else 0
        call.parts = [("rows", guarded("q part", (m, pc), el)), ("rows", guarded("k part", (m, pc), el))]
        if g.seq_len:
            pitch = (g.seq_len + 7) // 8 * 8
            vt = torch.zeros((m // g.seq_len, g.heads, call.head_dim, pitch), dtype=el, device=dev)
            vt[..., :g.seq_len] = FILL
            call.parts.append(("vt", vt))
        else:
            call.parts.append(("rows", guarded("v part", (m, pc), el)))
    elif in_place:
        assert call.residual is not None and call.rowbias is not None and call.alpha != 1.0
        call.out = call.residual
    else:
        call.out = guarded("out", (m, g.n), el)
    return call


def outputs(call):
    """name -> tensor, under the names of the case's expected outputs."""
    if call.case.geo.epi != "split":
        return {"out": call.out}
    got = {"q": call.parts[0][1], "k": call.parts[1][1]}
    kind, last = call.parts[2]
    if kind == "vt":
        got["vt"] = last[..., :call.seq_len]
    else:
        got["v"] = last
    return got


def deliver(call, values):
    """A stand-in's results (name -> tensor of values of the element type) into the destinations of the launch."""
    for name, dst in outputs(call).items():
        dst.copy_(values[name].to(dst.dtype))


def disturbed(call):
    """What the launch changed beside its outputs: a list of messages."""
    msgs = []
    for name, wide, c0, c, fill in call.guards:
        if not (bool((wide[:, :c0] == fill).all()) and bool((wide[:, c0 + c:] == fill).all())):
            msgs.append(f"the fill beside {name} was written")
    for name, t, before in call.kept:
        if not torch.equal(t, before):
            msgs.append(f"the operand {name} was written")
    if call.seq_len:
        vt = call.parts[2][1]
        if not bool((vt[..., call.seq_len:] == 0).all()):
            msgs.append("the pitch padding of V^T did not stay zero")
    return msgs


def run_case(case, key, launch, dev, in_place=False):
    """One launch of one case -> None or a message naming shape, case and the first wrong element of every output."""
    call = build(case, key, dev, in_place)
    want = case.expected(dev)
    launch(call)
    msgs = [m for m in (case.first_wrong(outputs(call), want, dev),) if m] + disturbed(call)
    if not msgs:
        return None
    head = "" if msgs[0].startswith(case.name) else f"{case.name} [{P.EL_NAME[case.el]}] {case.geo.text()}: "
    return ("in place: " if in_place else "") + head + "; ".join(msgs)


def launch_cases(geo, el, dev):
    """[(case, in place)] of one launch: every case of `cases` and, on STORE, `in_place`."""
    out = [(c, False) for c in P.cases(geo, el, dev)]
    if geo.epi == "store":
        out.append((P.in_place(geo, el, dev), True))
    return out


def run_route(route, el, launch, dev, shape=None):
    """Every case of every launch of a route (shape: geometry -> the geometry to run, e.g. fp8_gemm_cases.reduced) -> (the
    failing triples' messages, the number of launches made)."""
    failures, made = [], 0
    for lch in P.ROUTES[route]:
        geo = shape(lch.geo) if shape else lch.geo
        for case, inp in launch_cases(geo, el, dev):
            msg = run_case(case, lch.key, launch, dev, inp)
            made += 1
            if msg:
                failures.append(f"{route} ({lch.key}): {msg}")
        G.clear_cache()
    return failures, made


# ----------------------------------------------------------------------------------------------------- stand-ins for the kernel
def reference_stand_in(dev, emu=None, mut=None):
    """A launch function that delivers the case's own restatement: a legitimate design (emu, one of EMULATIONS: float32
    arithmetic) or a subtly wrong one (mut, one of MUTANTS)."""
    def launch(call):
        deliver(call, {k: v[0] for k, v in call.case.expected(dev, mut=mut, emu=emu).items()})
    return launch


def operand_stand_in(call):
    """A launch function that computes from the TENSORS of the call, as a kernel must: float32, K tiles of 128 forwards,
    acc * (a_scale * w_scale), the epilogue in float32, one rounding.  It shows that the operands of `build` are the problem the
    expected outputs belong to (slices, strides, the rowbias view and its group size, the in-place residual)."""
    dev = call.q.device
    f32 = torch.float32
    tab = P.decode_table(dev).to(f32)
    a, w = tab[call.q.to(torch.int64)], tab[call.w8.to(torch.int64)]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=f32, device=dev)
    for k0 in range(0, a.shape[1], 128):
        acc = acc + a[:, k0:k0 + 128] @ w[:, k0:k0 + 128].t()
    x = acc * (call.a_scale[:, None] * call.w_scale[None, :])
    if call.bias is not None:
        x = x + call.bias[None, :]
    if call.rowbias is not None:
        x = x + call.rowbias[torch.arange(a.shape[0], device=dev) // call.rows_per_group]
    if call.silu:
        x = x * (1.0 / (1.0 + torch.exp(-x)))
    x = x * call.alpha
    if call.residual is not None:
        x = x + call.residual.to(f32)
    el = call.case.el
    x = x.to(el)
    if call.case.geo.epi != "split":
        call.out.copy_(x)
        return
    pc = call.part_cols
    vals = {"q": x[:, :pc], "k": x[:, pc:2 * pc]}
    if call.seq_len:
        vals["vt"] = x[:, 2 * pc:].reshape(-1, call.seq_len, pc // call.head_dim, call.head_dim).permute(0, 2, 3, 1)
    else:
        vals["v"] = x[:, 2 * pc:]
    deliver(call, vals)


# ----------------------------------------------------------------------------------------------------- chained
def judge_chained(m, n, k, el, dev, produce):
    """produce(x, w) -> (out [m, n], a_scale [m], w_scale [n]): the producers' quantisation feeding the GEMM.  None or a message."""
    x, w, want = P.chained(m, n, k, el, dev)
    out, sa, sw = produce(x, w)
    msgs = []
    for name, s in (("a_scale", sa), ("w_scale", sw)):
        if not bool((s.to(G.F64) == 2.0 ** -6).all()):
            msgs.append(f"{name} is not 2^-6 everywhere (first: {float(s[(s.to(G.F64) != 2.0 ** -6).nonzero()[0, 0]])!r})")
    bad = out.to(G.F64) != want
    if bool(bad.any()):
        idx = tuple(int(v) for v in bad.nonzero()[0])
        msgs.append(f"out: {int(bad.sum())} of {bad.numel()} wrong, first at {idx}: got {float(out[idx])!r}, expected "
                    f"{float(want[idx])!r}")
    return f"chained [{P.EL_NAME[el]}] {m} x {n} x {k}: " + "; ".join(msgs) if msgs else None
