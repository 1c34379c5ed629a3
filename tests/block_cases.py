"""Problems with exactly known answers for the three one-launch blocks (vx_ff_fused, vx_tblock_fused + vx_tblock_pack,
vx_audio_xattn + vx_audio_xattn_pack), float64 references with the kernels' documented rounding points, mutants, emulations.

Host only (torch on any device, no import of v_express_amd): tests/test_block_cases_cpu.py shows that the cases are right and
that they tell a subtly wrong block from a right one; tests/test_gpu_blocks_exact.py feeds them to the kernels.

The Gaussian block tests (tests/test_gpu_kernels.py) accept 2^-7 .. 2^-4 of the largest value and relative L2 2e-3 .. 2.5e-2 on
tensors that the residual dominates: a column sum of unrounded Kq, a double rounding in front of the residual and (float16) a
positional row added after the rounding of q / k / v stay inside; a whole extra key frame or token slot does not
(`old_bound_figures`), but nothing there says which frame, head, pixel or packed column was wrong.  Here every operand is a
counter hash of its LOGICAL coordinates (gemm_cases._hash: x of (row, channel), weights of (output, input), tables of
(frame, column)), small dyadic values throughout, so every product and partial sum is exact in float32 in any order, and the
attention problems are attention_cases' builders (`counted`, `routing`, `tilted`) realised THROUGH the block.

Rounding points of the references (the kernel headers):
  ff      pre = rstd (x W1^T - mean colsum) + b1; h = value gelu(gate) rounded to the element type; out = x + h W2^T + b2
          rounded once.
  tblock  [q | k | v] = rstd (x W^T - mean colsum) + b + pe[frame] rounded; P = 2^(scale log2e (s - max)) rounded, the row sum
          from the unrounded P; O = (P V) / sum rounded; out = x + O Wo^T + bo rounded once.  `scale` is an operand.
  audio   Kq = float32(log2e / sqrt d) * (K to_q) rounded through float32 to the element type (the pack's one float32
          product), colsum = sums of the ROUNDED Kq, sbias = scale (K . bq); S = rstd (x Kq^T - mean colsum) + sbias;
          P = softmax_2 over the 5 tokens, normalised, THEN rounded; VO = to_out_head V^T rounded; out = x + alpha (P VO^T +
          bo) rounded once.

A row has C channels, q | k | v need 3C: a case feeds one or two of them from x through SELECTOR weights (one nonzero
+-2^e per row, at the fixed non-identity permutation (7 c + 3) % C of the channels: a head or column mix-up reads another
value) and the others from the per-frame table (pe_rows / kv).  Two complementary variants make each of q, k, v depend on the
pixel at least once.  LayerNorm statistics are hand-made (gemm_cases "folded": mean an integer in [-2, 2], rstd in {0.5, 1,
2}), biases and tables integers: the fold is exact.

  ff cases     signs, rounding (output), rounding (h), folded                                       - `ff_cases`
  tblock cases counted, routing (v from x | q, k from x), tilted, dense v / out-projection, dense q, dense k,
               own statistics                                                                        - `tb_cases`
  audio cases  counted, routing, tilted, dense out-projection                                        - `ax_cases`
Bounds: "bits" (the stored bit patterns, up to the sign of zero) or "ulp" (one unit in the last place of the expected value:
tilted only, whose P are real numbers).  `MUTANTS` edit the REFERENCE, never a kernel; `EMULATIONS` are legitimate designs.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

import attention_cases as A
from gemm_cases import (ELEMS, EL_NAME, SIG_BITS, F64, I64, _ar, _hash, _ulp, a_value, interleave8,  # noqa: F401
                        round_el, small_ints, tie_shares, w_value)

F32 = torch.float32
LOG2E = A.LOG2E
HEADS = 8
TOKENS = 5                      # audio tokens per frame
FF_C, FF_H = 320, 1280
TB_C, TB_D = 320, 40
# "bits" cases of the attention blocks: a winner that leads by 40 bits leaves 2^-40 of the other rows in O; where the expected
# value is exactly 0 that (or 0) is stored: Case.allowed applies it THERE only, every other element is compared for equality.
LEAK_TOL = 2.0 ** -20


# ----------------------------------------------------------------------------------------------------- helpers
def _mm(a, bt, emu=None):
    """a [m, k] @ bt [k, n] in float64 - or, for an emulation, in float32 over 64-wide K chunks in the order it names."""
    if emu is None:
        return a @ bt
    a32, b32 = a.to(F32), bt.to(F32)
    k = a.shape[1]
    ch = [(k0, min(k0 + 64, k)) for k0 in range(0, k, 64)]
    order = emu.get("order", "forwards")
    if order == "backwards":
        ch = ch[::-1]
    groups = [ch[:len(ch) // 2], ch[len(ch) // 2:]] if order == "two halves" and len(ch) > 1 else [ch]
    parts = []
    for grp in groups:
        acc = torch.zeros(a.shape[0], bt.shape[1], dtype=F32, device=a.device)
        for k0, k1 in grp:
            acc = acc + a32[:, k0:k1] @ b32[k0:k1]
        parts.append(acc)
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    return out.to(F64)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def src_of(n, c=None):
    """The fixed non-identity permutation behind every selector weight: output n reads input (7 n + 3) % c."""
    c = n.numel() if c is None else c
    return (7 * n + 3) % c


def selector(n_out, n_in, salt, dev, exps=(-1, 0, 1)):
    """float64 [n_out, n_in]: row n has ONE nonzero +-2^e at column (7 n + 3) % n_in, sign and e hashed from (salt, n)."""
    n = _ar(n_out, dev)
    h = _hash(salt, n)
    val = (1.0 - 2.0 * ((h >> 9) & 1).to(F64)) * torch.exp2(torch.tensor(exps, dtype=F64, device=dev)[(h >> 3) % len(exps)])
    w = torch.zeros(n_out, n_in, dtype=F64, device=dev)
    w[n, src_of(n, n_in)] = val
    return w


def hand_stats(rows, dev, rstds=(0.5, 1.0, 2.0)):
    """(mean [rows] integers in [-2, 2], rstd [rows]) of gemm_cases "folded"."""
    r = _ar(rows, dev)
    return small_ints(6, 2, dev, r), torch.tensor(rstds, dtype=F64, device=dev)[_hash(7, r) % len(rstds)]


def representable(t, el):
    return bool((round_el(t, el) == t).all())


def exact_in_f32(*masses):
    """True where every |term| sum (given in units of the terms' common granularity) stays below 2^24: any float32
    summation order gives the exact sum."""
    return all(float(m.max()) < 2.0 ** 24 for m in masses)


def _grain(t):
    """The largest power of two (as an exponent) that divides every element of t (dyadic values, exponent >= -40)."""
    for e in range(8, -41, -1):
        s = t * 2.0 ** -e
        if bool((s == torch.round(s)).all()):
            return e
    raise AssertionError("values are not small dyadic numbers")


# ----------------------------------------------------------------------------------------------------- the case
@dataclass
class Case:
    block: str                      # ff | tb | ax
    name: str
    el: torch.dtype
    shape: dict
    o: dict                         # operands, float64 (what the kernel is fed: `kernel_operands`)
    bound: str = "bits"             # bits | ulp
    keep: Optional[torch.Tensor] = None      # bool [rows, C]: the judged elements (dense q / k leave tied rows out)
    zero_tol: float = 0.0           # allowed where the expected value is exactly 0 (ff: |gelu_f| <= 2^-30 under a low gate; LEAK_TOL)
    conditions: list = field(default_factory=list)
    _exp: Optional[torch.Tensor] = None

    def forward(self, mut=None, emu=None):
        """The stored output [rows, C] as float64 values of the element type: reference, a mutant or an emulation."""
        return FORWARD[self.block](self, mut, emu)

    def expected(self):
        if self._exp is None:
            self._exp = self.forward()
        return self._exp

    def allowed(self):
        e = self.expected()
        if self.bound == "ulp":
            return _ulp(e, self.el)
        return torch.where(e == 0, torch.full_like(e, self.zero_tol), torch.zeros_like(e))

    def wrong(self, got):
        """bool [rows, C]: where `got` (any float type, values of the element type) violates the case."""
        e = self.expected()
        g = got.detach().to(e.device).to(F64)
        bad = ~((g == e) | ((g - e).abs() <= self.allowed()))
        return bad if self.keep is None else bad & self.keep

    def deviation(self, got):
        e = self.expected()
        dev = torch.nan_to_num((got.detach().to(e.device).to(F64) - e).abs(), nan=math.inf)
        if self.keep is not None:
            dev = dev * self.keep
        return float(dev.max())

    def where(self, row, col):
        s = self.shape
        if self.block == "ff":
            return f"row {row} (tile {row // 128}) column {col}"
        if self.block == "tb":
            f, hw = s["f"], s["hw"]
            head = int(src_of(torch.tensor(col), TB_C)) // TB_D if self.o.get("wo_selector") else "-"
            return f"item {row // (f * hw)} frame {row // hw % f} pixel {row % hw} head {head} column {col}"
        rpf = s["rows_per_frame"]
        d = s["c"] // HEADS
        head = int(src_of(torch.tensor(col), s["c"])) // d if self.o.get("wo_selector") else "-"
        return f"item (frame) {row // rpf} pixel {row % rpf} head {head} column {col}"

    def first_wrong(self, got):
        """None, or a message naming item, frame, pixel, head and column of the first wrong element."""
        bad = self.wrong(got)
        if not bool(bad.any()):
            return None
        row, col = (int(v) for v in bad.nonzero()[0])
        e = self.expected()
        return (f"{self.block} {self.name} [{EL_NAME[self.el]}] {self.shape}: {int(bad.sum())} of {bad.numel()} wrong, first at "
                f"{self.where(row, col)}: got {float(got[row, col])!r}, expected {float(e[row, col])!r} (bound: {self.bound})")


# ===================================================================================================== ff
def uninterleave8(t):
    """What the kernel makes of a [2 hidden] table handed over in LOGICAL order although it expects the interleaved one."""
    idx = interleave8(torch.arange(t.shape[0], device=t.device))
    out = torch.empty_like(t)
    out[idx] = t
    return out


def ff_forward(c, mut=None, emu=None):
    o, el = c.o, c.el
    x = o["x"]
    acc = _mm(x, o["w1"].t(), emu)
    mean, rstd, cs, b1 = o["mean"][:, None], o["rstd"][:, None], o["colsum"][None, :], o["b1"]
    if mut == "bias1 in un-interleaved order":
        b1 = uninterleave8(b1)
    if mut == "mean * colsum dropped":
        pre = rstd * acc + b1
    elif mut == "mean * colsum applied with rstd outside":
        pre = rstd * acc - mean * cs + b1
    else:
        pre = rstd * (acc - mean * cs) + b1
    val, gate = pre[:, :FF_H], pre[:, FF_H:]
    h = val * gelu64(gate)
    if mut != "h not rounded before W2":
        h = round_el(h, el)
    y = _mm(h, o["w2"].t(), emu)
    if mut == "output rounded twice (before the residual)":
        return round_el(x + round_el(y + o["b2"], el), el)
    return round_el(x + (y + o["b2"]), el)


def _ff_case(name, el, m, dev, x, wv, wg, b1, colsum, mean, rstd, w2, b2, low_gates=False):
    o = dict(x=x, w1=torch.cat([wv, wg], 0), b1=b1, colsum=colsum, mean=mean, rstd=rstd, w2=w2, b2=b2)
    c = Case("ff", name, el, dict(m=m), o, zero_tol=2.0 ** -20 if low_gates else 0.0)
    for k in ("x", "w1", "w2"):
        assert representable(o[k], el), f"ff {name}: {k} is not representable in {el}"
    # ---- the construction claims, on the reference
    pre = rstd[:, None] * (x @ o["w1"].t() - mean[:, None] * colsum[None, :]) + b1
    val, gate = pre[:, :FF_H], pre[:, FF_H:]
    assert bool((gate.abs() >= 32).all()), f"ff {name}: a gate outside the saturated range ({float(gate.abs().min())})"
    assert low_gates or bool((gate >= 32).all()), f"ff {name}: a negative gate"
    hx = val * torch.where(gate > 0, gate, torch.zeros_like(gate))
    assert bool((hx.to(F32).to(F64) == hx).all()), f"ff {name}: value * gate is not exact in float32"
    hr = round_el(hx, el)
    g1 = _grain(x) + _grain(o["w1"])
    g2 = min(_grain(hr) + _grain(w2), _grain(b2), _grain(x))
    assert exact_in_f32((x.abs() @ o["w1"].abs().t()) * 2.0 ** -g1, (hr.abs() @ w2.abs().t() + b2.abs() + x.abs()) * 2.0 ** -g2), \
        f"ff {name}: a sum can leave 2^24 units"
    exact = x + hr @ w2.t() + b2
    c.conditions.append(f"gates saturated ({float((gate < 0).double().mean()):.2f} low), every sum exact in float32, "
                        f"{float((hr != hx).double().mean()):.3f} of h rounded, max |out| {float(exact.abs().max()):g}")
    return c, hx, exact


def _ff_x(m, dev, dens, scale=1.0):
    return scale * a_value(0, _ar(m, dev)[:, None], 0, _ar(FF_C, dev)[None, :], dens)


def _ff_gate_dense(dev):
    return w_value(0, FF_H + _ar(FF_H, dev)[:, None], 0, 0, _ar(FF_C, dev)[None, :])


def ff_signs(el, m, dev="cpu"):
    """Gate bias +128 on even and -128 on odd 8-column blocks; x in {-2, 0, 2}, value = +-x[(7 j + 3) % 320], dense +-1 gate
    weights; W2 has two +-1/4 per row: |out| < 2^8, NO output needs rounding."""
    j = _ar(FF_H, dev)
    x = _ff_x(m, dev, 16 / 320, 2.0)
    wv = selector(FF_H, FF_C, 21, dev, exps=(0,))
    b1 = torch.cat([torch.zeros(FF_H, dtype=F64, device=dev),
                    2 * small_ints(23, 2, dev, j) + torch.where((j // 8) % 2 == 0, 128.0, -128.0).to(F64)])
    colsum = torch.cat([torch.zeros(FF_H, dtype=F64, device=dev), 2 * small_ints(25, 2, dev, j)])
    mean = small_ints(24, 1, dev, _ar(m, dev))
    n = _ar(FF_C, dev)
    j1 = _hash(26, n) % FF_H
    j2 = (j1 + 1 + 2 * (_hash(27, n) % 600)) % FF_H
    w2 = torch.zeros(FF_C, FF_H, dtype=F64, device=dev)
    w2[n, j1] = 0.25 * (1.0 - 2.0 * ((_hash(28, n) >> 4) & 1).to(F64))
    w2[n, j2] = 0.25 * (1.0 - 2.0 * ((_hash(29, n) >> 4) & 1).to(F64))
    c, hx, exact = _ff_case("signs", el, m, dev, x, wv, _ff_gate_dense(dev), b1, colsum, mean, torch.ones(m, dtype=F64, device=dev),
                            w2, small_ints(30, 8, dev, n), low_gates=True)
    assert representable(hx, el) and representable(exact, el) and float(exact.abs().max()) < 2.0 ** 8, \
        f"ff signs: an output needs rounding (max |out| {float(exact.abs().max())})"
    c.conditions.append("h and every output representable: out == x + (value gate) W2^T + b2")
    return c


def ff_rounding_out(el, m, dev="cpu"):
    """All gates positive multiples of 32 in [32, 224] (two +-32 per gate row), value = +-x in {-1, 0, 1}: h = +-gate exact; W2
    dense +-2^-5: h W2^T is an integer of a few tens; b2 carries gemm_cases' rounding offsets (1.5 * 2^SIG on even, 4x on odd
    columns).  Pins the ONE rounding of the output.  (Its own case: a tie needs an exact output with at most SIG + 1 significant
    bits, and a rounded h alone carries SIG of them at its own exponent - the h that needs rounding is `ff_rounding_h`.)"""
    j, ci = _ar(FF_H, dev), _ar(FF_C, dev)
    x = _ff_x(m, dev, 16 / 320)
    wv = selector(FF_H, FF_C, 31, dev, exps=(0,))
    wg = torch.zeros(FF_H, FF_C, dtype=F64, device=dev)
    c1 = _hash(32, j) % FF_C
    c2 = (c1 + 1 + _hash(33, j) % (FF_C - 1)) % FF_C
    wg[j, c1] = 32.0 * (1.0 - 2.0 * ((_hash(34, j) >> 4) & 1).to(F64))
    wg[j, c2] = 32.0 * (1.0 - 2.0 * ((_hash(35, j) >> 4) & 1).to(F64))
    b1 = torch.cat([torch.zeros(FF_H, dtype=F64, device=dev), 128.0 + 32 * small_ints(36, 1, dev, j)])
    w2 = w_value(1, ci[:, None], 0, 0, j[None, :]) * 2.0 ** -5
    b2 = small_ints(37, 8, dev, ci) + 1.5 * 2.0 ** SIG_BITS[el] * torch.where(ci % 2 == 0, 1.0, 4.0).to(F64)
    z = torch.zeros(m, dtype=F64, device=dev)
    c, hx, exact = _ff_case("rounding (output)", el, m, dev, x, wv, wg, b1, torch.zeros(2 * FF_H, dtype=F64, device=dev), z, z + 1, w2, b2)
    assert representable(hx, el), "ff rounding (output): h needs rounding"
    ties, other = tie_shares(exact, el)
    assert ties >= 0.25 and other >= 0.25, f"ff rounding (output): ties {ties:.3f}, other roundings {other:.3f}"
    c.conditions.append(f"exact outputs: ties {ties:.3f}, other roundings {other:.3f} (each >= 0.25)")
    return c


def ff_rounding_h(el, m, dev="cpu"):
    """All gates positive integers around 2^(SIG-1) (dense +-1 gate weights), value = +-(1 + r 2^-(SIG-1)) x with a full
    significand per hidden unit: value * gate needs rounding.  Pins the ONE rounding of h (and, again, of the output)."""
    j, ci = _ar(FF_H, dev), _ar(FF_C, dev)
    p = SIG_BITS[el] - 1
    x = _ff_x(m, dev, 16 / 320)
    wv = selector(FF_H, FF_C, 41, dev, exps=(0,)) * (1.0 + (_hash(42, j) % 2 ** p).to(F64) * 2.0 ** -p)[:, None]
    b1 = torch.cat([torch.zeros(FF_H, dtype=F64, device=dev), 2.0 ** p + small_ints(43, 8, dev, j)])
    w2 = w_value(2, ci[:, None], 0, 0, j[None, :]) * 2.0 ** -3
    z = torch.zeros(m, dtype=F64, device=dev)
    c, hx, exact = _ff_case("rounding (h)", el, m, dev, x, wv, _ff_gate_dense(dev), b1, torch.zeros(2 * FF_H, dtype=F64, device=dev), z, z + 1,
                            w2, small_ints(44, 8, dev, ci))
    nz = hx != 0
    ties, other = tie_shares(hx[nz], el)
    assert ties + other >= 0.5 and ties > 0, f"ff rounding (h): ties {ties:.3f}, other roundings {other:.3f} of the nonzero h"
    c.conditions.append(f"nonzero h: ties {ties:.3f}, other roundings {other:.3f} (together >= 0.5)")
    return c


def ff_folded(el, m, dev="cpu"):
    """Hand-made statistics per row on both halves: value = rstd (+-x - mean colsum) + b, gate = rstd (dense - mean colsum) + b +
    256, all positive; W2 +-1/8 on a quarter of its entries."""
    j, ci = _ar(FF_H, dev), _ar(FF_C, dev)
    x = _ff_x(m, dev, 16 / 320)
    wv = selector(FF_H, FF_C, 51, dev, exps=(0,))
    b1 = torch.cat([small_ints(52, 2, dev, j), 256.0 + small_ints(53, 8, dev, j)])
    colsum = small_ints(8, 2, dev, _ar(2 * FF_H, dev))
    mean, rstd = hand_stats(m, dev)
    w2 = w_value(3, ci[:, None], 0, 0, j[None, :]) * 2.0 ** -3 * (_hash(54, ci[:, None], j[None, :]) % 4 == 0)
    c, hx, exact = _ff_case("folded", el, m, dev, x, wv, _ff_gate_dense(dev), b1, colsum, mean, rstd, w2, small_ints(55, 8, dev, ci))
    return c


def ff_cases(el, m, dev="cpu"):
    return [ff_signs(el, m, dev), ff_rounding_out(el, m, dev), ff_rounding_h(el, m, dev), ff_folded(el, m, dev)]


def ff_kernel_operands(c):
    """What ops.ff_fused takes: x, the interleaved folded W1 / b1 / colsum, statistics [m, 2], W2, b2."""
    o, el = c.o, c.el
    return dict(x=o["x"].to(el), w1=interleave8(o["w1"]).to(el).contiguous(), b1=interleave8(o["b1"]).to(F32).contiguous(),
                colsum=interleave8(o["colsum"]).to(F32).contiguous(),
                stats=torch.stack([o["mean"], o["rstd"]], 1).to(F32).contiguous(), w2=o["w2"].to(el).contiguous(), b2=o["b2"].to(F32))


FF_MUTANTS = ("mean * colsum dropped", "mean * colsum applied with rstd outside", "bias1 in un-interleaved order",
              "h not rounded before W2", "output rounded twice (before the residual)")
FF_EMULATIONS = {"float32, 64-wide chunks forwards": dict(order="forwards"), "float32, 64-wide chunks backwards": dict(order="backwards"),
                 "float32, two halves of K summed afterwards": dict(order="two halves")}


# ===================================================================================================== tblock
def tb_rows(t, b, f, hw):
    """attention_cases' [(b hw) f, C] -> the model's rows [(b f) hw, C] (row = (item * f + frame) * hw + pixel)."""
    return A.temporal_rows(t, b, f, hw)


def tb_forward(c, mut=None, emu=None, parts=False):
    o, el, s = c.o, c.el, c.shape
    b, f, hw = s["b"], s["f"], s["hw"]
    x = o["x"]
    m, dev = x.shape[0], x.device
    emu = emu or {}
    mm_emu = emu if "order" in emu else None
    frame = (_ar(m, dev) // hw) % f
    if o["mean"] is None:                           # ln_stats == NULL: the kernel's own two-pass statistics
        mean = x.mean(1)
        rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + o["eps"])
        if "stat_err" in emu:                       # ... off by the bound norm_cases gives vx_row_stats
            mean, rstd = mean * (1 + emu["stat_err"] * 2.0 ** -23), rstd * (1 + emu["stat_err"] * 2.0 ** -16)
    else:
        mean, rstd = o["mean"], o["rstd"]
    mean, rstd = mean[:, None], rstd[:, None]
    acc = _mm(x, o["wqkv"].t(), mm_emu)
    cs = o["colsum"][None, :]
    if mut == "mean * colsum dropped":
        fold = rstd * acc
    elif mut == "mean * colsum applied with rstd outside":
        fold = rstd * acc - mean * cs
    else:
        fold = rstd * (acc - mean * cs)
    fr = (frame + 1) % f if mut == "pe row of frame + 1" else (frame - 1) % f if mut == "pe row of frame - 1" else frame
    pe = o["pe"][fr]
    if isinstance(mut, tuple) and mut[0] == "column":          # ("column", n, n2): q | k | v column n is built from column n2's
        fold, pe, bq_ = fold.clone(), pe.clone(), o["bqkv"].clone()           # weight row, bias, colsum and table column
        fold[:, mut[1]], pe[:, mut[1]], bq_[mut[1]] = fold[:, mut[2]], pe[:, mut[2]], bq_[mut[2]]
        qkv = round_el(fold + bq_ + pe, el)
    elif mut == "pe added after the rounding of q / k / v":
        qkv = round_el(fold + o["bqkv"], el) + pe
    else:
        qkv = round_el(fold + o["bqkv"] + pe, el)
    t = qkv.reshape(b, f, hw, 3, HEADS, TB_D).permute(3, 0, 2, 4, 1, 5)         # [3, item, pixel, head, frame, d]
    q, k, v = t[0], t[1], t[2]
    if mut == "the last frame or token dropped":
        k, v = k[..., :-1, :], v[..., :-1, :]
    elif mut == "a padded key frame unmasked (f = 24)" and f == 24:             # (the padding rows re-read frame 23)
        k, v = torch.cat([k, k[..., -1:, :]], -2), torch.cat([v, v[..., -1:, :]], -2)
    elif mut in NEIGHBOUR:                                                      # ... in frame 0
        k, v = k.clone(), v.clone()
        k[..., 0, :], v[..., 0, :] = k.roll(-1, NEIGHBOUR[mut])[..., 0, :], v.roll(-1, NEIGHBOUR[mut])[..., 0, :]
    scale = o["scale"]
    if mut in PADDED_SCALE:
        scale = scale * (TB_D / (-(-TB_D // PADDED_SCALE[mut]) * PADDED_SCALE[mut])) ** 0.5
    sl = torch.einsum("bphid,bphjd->bphij", q, k) * (scale * LOG2E)
    mx = sl.amax(-1, keepdim=True)
    if emu.get("max_rounded"):                      # the row maximum scaled on its own and rounded to float32: the winner's P is 2^(+-tiny)
        mx = mx.to(F32).to(F64)
    p = torch.exp2(sl - mx)
    pr = round_el(p, el)
    den = (pr if emu.get("sum_rounded") else p).sum(-1)
    att = round_el(torch.einsum("bphij,bphjd->bphid", pr, v) / den[..., None], el)
    if mut == "heads swapped in the out-projection input":
        att = att[:, :, [1, 0] + list(range(2, HEADS))]
    of = att.permute(0, 3, 1, 2, 4).reshape(m, TB_C)
    out = round_el(x + (_mm(of, o["wo"].t(), mm_emu) + o["bo"]), el)
    if parts:
        return dict(q=q, k=k, v=v, logits=sl, att=att, out=out, pre=fold + o["bqkv"] + pe)
    return out


NEIGHBOUR = {"the neighbouring item's key and value": 0, "the neighbouring pixel's key and value": 1,
             "the neighbouring head's key and value": 2}
PADDED_SCALE = {"scale from a head dim padded to 48": 48, "scale from a head dim padded to 64": 64}


def _tb_stats(m, dev, rstds=(0.5, 1.0, 2.0)):
    return hand_stats(m, dev, rstds)


def _zeros(*shape, dev="cpu"):
    return torch.zeros(*shape, dtype=F64, device=dev)


def _realize(target, sel, cs, mean, rstd, add):
    """x [m, C] with rstd (x sel^T - mean cs) + add == target: x[:, (7 c + 3) % C] = ((target - add) / rstd + mean cs) / sel_c."""
    cdim = target.shape[1]
    n = _ar(cdim, target.device)
    src = src_of(n, cdim)
    val = ((target - add) / rstd[:, None] + mean[:, None] * cs[None, :]) / sel[n, src][None, :]
    x = torch.empty_like(target)
    x[:, src] = val
    return x


def _tb_case(name, el, b, f, hw, dev, x, w, bias, cs, pe, wo, bo, mean, rstd, bound="bits", eps=1e-5, wo_selector=True, keep=None):
    """w / bias / cs / pe: (q, k, v) triples of [320, 320] / [320] / [320] / [f, 320] (None = zeros)."""
    z1, z2, zf = _zeros(TB_C, dev=dev), _zeros(TB_C, TB_C, dev=dev), _zeros(f, TB_C, dev=dev)
    cat = lambda ts, z, d: torch.cat([z if t is None else t for t in ts], d)
    o = dict(x=x, wqkv=cat(w, z2, 0), bqkv=cat(bias, z1, 0), colsum=cat(cs, z1, 0), pe=cat(pe, zf, 1), wo=wo, bo=bo, mean=mean, rstd=rstd,
             scale=TB_D ** -0.5, eps=eps, wo_selector=wo_selector)
    c = Case("tb", name, el, dict(b=b, f=f, hw=hw), o, bound=bound, keep=keep, zero_tol=LEAK_TOL)
    for k_ in ("x", "wqkv", "wo"):
        assert representable(o[k_], el), f"tb {name}: {k_} is not representable in {el}"
    g = min(_grain(x) + _grain(o["wqkv"]), 0)
    assert exact_in_f32((x.abs() @ o["wqkv"].abs().t()) * 2.0 ** -g), f"tb {name}: a projection sum can leave 2^24 units"
    return c


def _margin(logits, pi):
    """(smallest lead of key pi over every other key in bits, largest winning logit); logits [..., i, j], pi [..., i]."""
    top = logits.gather(-1, pi[..., None])
    others = logits.scatter(-1, pi[..., None], -math.inf).amax(-1, keepdim=True)
    return float((top - others).min()), float(top.abs().max())


def _same(a, b):
    """Equal up to what 2^-40 of another row leaves where a value is exactly 0 (Case.zero_tol)."""
    return float((a - b).abs().max()) <= 2.0 ** -30


def _tb_wo(dev, salt, exps=(-1, 0, 1)):
    return selector(TB_C, TB_C, salt, dev, exps), small_ints(salt + 1, 8, dev, _ar(TB_C, dev))


def _tb_table(salt, lim, f, dev):
    return small_ints(salt, lim, dev, _ar(f, dev)[:, None], _ar(TB_C, dev)[None, :])


def _split_table(t, salt, dev):
    """An integer table [f, 320] as bias [320] + pe [f, 320]: the kernel must add both."""
    bias = small_ints(salt, 4, dev, _ar(TB_C, dev))
    return bias, t - bias[None, :]


def tb_counted(el, b, f, hw, dev="cpu"):
    """q = 0 (zero weight, bias and table), V = attention_cases.counted through a selector weight from x: the mean over exactly f
    frames is the integer v0 + 1 per (item, pixel, head)."""
    m = b * f * hw
    ca = A.counted(A.Geom(b * hw, HEADS, f, f, TB_D, 1), el)
    v_t = tb_rows(ca.v.double(), b, f, hw).to(dev)
    mean, rstd = _tb_stats(m, dev)
    sel = selector(TB_C, TB_C, 61, dev, exps=(0, 1))
    cs_v = small_ints(62, 2, dev, _ar(TB_C, dev))
    x = _realize(v_t, sel, cs_v, mean, rstd, _zeros(m, TB_C, dev=dev))
    kb, kpe = _split_table(_tb_table(63, 8, f, dev), 64, dev)
    wo, bo = _tb_wo(dev, 65)
    c = _tb_case("counted", el, b, f, hw, dev, x, (None, None, sel), (None, kb, None), (None, small_ints(66, 2, dev, _ar(TB_C, dev)), cs_v),
                 (None, kpe, None), wo, bo, mean, rstd)
    r = tb_forward(c, parts=True)
    att_t = tb_rows(ca.expected.double(), b, f, hw).to(dev)
    assert bool((r["q"] == 0).all()) and bool((r["pre"][:, 2 * TB_C:] == v_t).all()), "tb counted: q != 0 or V is not the builder's"
    assert torch.equal(r["out"], round_el(x + att_t @ wo.t() + bo, el)), "tb counted: the reference is not x + perm(v0 + 1) + bias_o"
    c.conditions.append("q == 0, V == attention_cases.counted, out == x + perm(v0 + 1) + bias_o")
    return c


def _codes(f, el, dev):
    """attention_cases.routing for ONE sequence of f frames: (q [f, 320], k [f, 320], pi [f, heads])."""
    r = A.routing(A.Geom(1, HEADS, f, f, TB_D, 1), el)
    return r.q.double().to(dev), r.k.double().to(dev), r.pi[0].to(dev)


def tb_routing_v(el, b, f, hw, dev="cpu", own_stats=False):
    """Routing, V from x: q and k are attention_cases.routing's codes per (frame, head) from bias + table, query frame i wins
    key pi(i, head) by >= 40 bits; V = rstd (+-2^e x[perm] - mean colsum) + b + pe[frame] differs per (item, pixel, frame,
    head); its bias carries 3 * 2^(SIG-1), which the table takes back on the even frames: V needs rounding on the odd ones.  own_stats: ln_stats == NULL, rows of
    norm_cases' construction (80 channels at m - 1.5, 240 at m + 0.5, eps = 0.25: mean = m, rstd = 1 exactly)."""
    m = b * f * hw
    qc, kc, pi = _codes(f, el, dev)
    r_, ch = _ar(m, dev)[:, None], _ar(TB_C, dev)[None, :]
    sel = selector(TB_C, TB_C, 71, dev)
    if own_stats:
        mrow = small_ints(72, 6, dev, _ar(m, dev))
        low = torch.argsort(torch.argsort(_hash(73, r_, ch), dim=1), dim=1) < TB_C // 4
        x = mrow[:, None] + torch.where(low, -1.5, 0.5).to(F64)
        mean = rstd = None
        cs_v = sel.sum(1)                           # the TRUE column sums: v = +-2^e (x - mean) rstd
        eps = 0.25
    else:
        x = 2.0 * (_hash(73, r_, ch) % 8).to(F64) - 7.0
        mean, rstd = _tb_stats(m, dev)
        cs_v = small_ints(74, 2, dev, _ar(TB_C, dev))
        eps = 1e-5
    qb, qpe = _split_table(qc, 75, dev)
    kb, kpe = _split_table(kc, 76, dev)
    # in the BIAS; the table takes it back on the even frames: adding pe after a rounding shows.  (Own statistics: none - V stays
    # representable there, so statistics that are off by the row-statistics bound cannot move a tie.)
    big = 0.0 if own_stats else 3.0 * 2.0 ** (SIG_BITS[el] - 1)
    vpe = _tb_table(77, 8, f, dev) - (_ar(f, dev) % 2 == 0).to(F64)[:, None] * big
    wo, bo = _tb_wo(dev, 78)
    c = _tb_case("own statistics" if own_stats else "routing (v from x)", el, b, f, hw, dev, x, (None, None, sel),
                 (qb, kb, small_ints(79, 4, dev, _ar(TB_C, dev)) + big), (None, None, cs_v), (qpe, kpe, vpe), wo, bo, mean, rstd, eps=eps)
    r = tb_forward(c, parts=True)
    pi_b = pi.t()[None, None].expand(b, hw, HEADS, f)
    lead, top = _margin(r["logits"], pi_b)
    assert lead >= 40 and top < 2 ** 10, f"tb routing: margin {lead} bits, winning logit {top}"
    want = r["v"].gather(3, pi_b[..., None].expand(-1, -1, -1, -1, TB_D))
    assert _same(r["att"], want), "tb routing: the attention output is not V[pi]"
    ties, other = tie_shares(r["pre"][:, 2 * TB_C:], el)
    assert ties + other >= 0.2 or own_stats, f"tb routing: only {ties + other:.3f} of V need rounding"
    assert not own_stats or ties + other == 0, "tb own statistics: a V needs rounding"
    c.conditions.append(f"winner leads by {lead:.0f} bits, out == x + perm(V[pi]) + bias_o, {ties + other:.2f} of V rounded")
    return c


def tb_routing_qk(el, b, f, hw, dev="cpu"):
    """Routing, q = k from x: attention_cases.routing's key codes per (item, pixel, frame, head) through one selector weight
    for q and k (every frame attends to itself), V from bias + table."""
    m = b * f * hw
    r0 = A.routing(A.Geom(b * hw, HEADS, f, f, TB_D, 1), el)
    t = tb_rows(r0.k.double(), b, f, hw).to(dev)
    mean, rstd = _tb_stats(m, dev)
    sel = selector(TB_C, TB_C, 81, dev)
    cs = small_ints(82, 2, dev, _ar(TB_C, dev))
    x = _realize(t, sel, cs, mean, rstd, _zeros(m, TB_C, dev=dev))
    vb, vpe = _split_table(_tb_table(83, 8, f, dev), 84, dev)
    wo, bo = _tb_wo(dev, 85)
    c = _tb_case("routing (q, k from x)", el, b, f, hw, dev, x, (sel, sel, None), (None, None, vb), (cs, cs, small_ints(86, 2, dev, _ar(TB_C, dev))),
                 (None, None, vpe), wo, bo, mean, rstd)
    r = tb_forward(c, parts=True)
    pi_b = _ar(f, dev)[None, None, None].expand(b, hw, HEADS, f)
    lead, top = _margin(r["logits"], pi_b)
    assert lead >= 40 and top < 2 ** 10, f"tb routing (q, k): margin {lead} bits, winning logit {top}"
    assert _same(r["att"], r["v"]), "tb routing (q, k): the attention output is not V of the frame itself"
    c.conditions.append(f"q == k == the codes, own frame leads by {lead:.0f} bits")
    return c


def tb_tilted(el, b, f, hw, dev="cpu"):
    """attention_cases.tilted: q = 1 from x (x = 1 / (rstd 2^e) > 0), keys and values from the table: two logit levels ~4 bits
    apart.  Positive selectors and bias_o = 0: out = x + 2^e O has no cancellation, one unit of O is at most one of out."""
    m = b * f * hw
    ti = A.tilted(A.Geom(1, HEADS, f, f, TB_D, 1), el)
    mean, rstd = _tb_stats(m, dev)
    sel = selector(TB_C, TB_C, 91, dev).abs()
    x = _realize(torch.ones(m, TB_C, dtype=F64, device=dev), sel, _zeros(TB_C, dev=dev), mean, rstd, _zeros(m, TB_C, dev=dev))
    kb, kpe = _split_table(ti.k.double().to(dev), 92, dev)
    vb, vpe = _split_table(ti.v.double().to(dev), 93, dev)
    wo = selector(TB_C, TB_C, 94, dev).abs()
    c = _tb_case("tilted", el, b, f, hw, dev, x, (sel, None, None), (None, kb, vb), (None, None, None), (None, kpe, vpe), wo,
                 _zeros(TB_C, dev=dev), mean, rstd, bound="ulp")
    r = tb_forward(c, parts=True)
    assert bool((r["q"] == 1).all())
    lv = torch.unique(torch.round(r["logits"] * 1024) / 1024)
    assert len(lv) == 2 and 3 < float(lv[1] - lv[0]) < 5, f"tb tilted: logit levels {lv}"
    c.conditions.append(f"two logit levels {float(lv[1] - lv[0]):.3f} bits apart")
    return c


def tb_dense_v(el, b, f, hw, dev="cpu"):
    """q = k = per-frame codes from the table (every frame attends to itself: O == v), Wv and Wo dense +-1, x in {-1, 0, 1}: two
    exact GEMMs in a row.  Every packed column of blocks 5-7 and of the three out-projection parts, and bias_o."""
    m = b * f * hw
    _, kc, _ = _codes(f, el, dev)
    ch = _ar(TB_C, dev)
    x = a_value(0, _ar(m, dev)[:, None], 0, ch[None, :], 16 / 320)
    mean, rstd = _tb_stats(m, dev)
    wv = w_value(10, ch[:, None], 0, 0, ch[None, :])
    wo = w_value(11, ch[:, None], 0, 0, ch[None, :])
    qb, qpe = _split_table(kc, 101, dev)
    c = _tb_case("dense v / out-projection", el, b, f, hw, dev, x, (None, None, wv), (qb, qb, small_ints(102, 4, dev, ch)),
                 (None, None, small_ints(103, 2, dev, ch)), (qpe, qpe, _tb_table(104, 8, f, dev)), wo, small_ints(105, 8, dev, ch), mean, rstd,
                 wo_selector=False)
    r = tb_forward(c, parts=True)
    pre_v = r["pre"][:, 2 * TB_C:]
    assert representable(pre_v, el) and _same(r["att"], r["v"]), "tb dense v: V needs rounding or O != v"
    assert exact_in_f32(r["att"].abs().sum((-1, -3)) * 2.0)
    c.conditions.append(f"O == v == the exact projection (max |v| {float(pre_v.abs().max()):g}), out = x + v Wo^T + bias_o rounded once")
    return c


def dense_variants(f):
    """Unit-vector tables that together put EVERY channel of a head under some frame's unit: 3 at f = 16, 2 at f = 24."""
    return -(-TB_D // f)


def unit_positions(f, variant):
    """[f, heads]: the channel of head h that frame j's unit vector occupies: 7 (j + f variant) + 3 h mod 40.  7 is coprime to
    40, so j + f variant = 0 .. 39 visits every channel once: `dense_variants(f)` tables cover all 40 of every head."""
    j, h = torch.arange(f)[:, None], torch.arange(HEADS)[None, :]
    return (7 * (j + f * variant) + 3 * h) % TB_D


def _unit_table(f, dev, variant=0, amp=128.0):
    """[f, 320]: frame j, head h holds amp at channel unit_positions(f, variant)[j, h] of the head, 0 elsewhere."""
    pos = unit_positions(f, variant).to(dev)
    t = _zeros(f, HEADS, TB_D, dev=dev)
    t.scatter_(2, pos[..., None], amp)
    return t.reshape(f, TB_C), pos


DENSE_SHIFT = 176.0             # ~2.2 standard deviations of the dense projection: the LARGEST of f values lands around 0
DENSE_LEAD, DENSE_TOP = 25.0, 2.0 ** 12


def tb_dense_qk(el, b, f, hw, which, dev="cpu", variant=0):
    """which = "q": keys are 128 e_p from the table, p = unit_positions(f, variant)[j, h] (the variants together make every one
    of a head's 40 channels - the shared M block's q32..39 / k32..39 included - the channel some key frame reads), q = x Wq^T - mean colsum - 176 with dense +-1 Wq and odd
    integers x in [-7, 7] (rstd = 1): query frame i picks the key frame j whose channel of q_i is the largest - the arg-max of a
    dense integer projection, one step of which is 29 bits of logit.  which = "k": the queries are the unit vectors and the keys
    the dense projection.  V = odd integers from bias + table (no zeros: 2^-29 of another row never shows).  The shift keeps the
    winning logit small: a kernel may scale the row maximum separately, which costs 2^-24 of the logit's size in the exponent
    (attention_cases keeps winners below 2^10 for the same reason).  (row, head) pairs whose winner leads by less than 25 bits -
    tied top two - or whose winning logit reaches 2^12 are left out, no more than 5 % of them."""
    m = b * f * hw
    ch = _ar(TB_C, dev)
    unit, pos = _unit_table(f, dev, variant)
    x = 2.0 * (_hash(111, _ar(m, dev)[:, None], ch[None, :]) % 8).to(F64) - 7.0
    mean, rstd = _tb_stats(m, dev, rstds=(1.0,))
    wd = w_value(12 if which == "q" else 13, ch[:, None], 0, 0, ch[None, :])
    csd = small_ints(112, 2, dev, ch)
    bd = _zeros(TB_C, dev=dev) - DENSE_SHIFT
    ub, upe = _split_table(unit, 113, dev)
    vb, vpe = _split_table(2.0 * (_hash(114, _ar(f, dev)[:, None], ch[None, :]) % 8).to(F64) - 7.0, 115, dev)
    wo, bo = _tb_wo(dev, 116)
    iq = which == "q"
    c = _tb_case(f"dense {which} #{variant}", el, b, f, hw, dev, x, (wd, None, None) if iq else (None, wd, None), (bd, ub, vb) if iq else (ub, bd, vb),
                 (csd, None, None) if iq else (None, csd, None), (None, upe, vpe) if iq else (upe, None, vpe), wo, bo, mean, rstd)
    r = tb_forward(c, parts=True)
    top2 = r["logits"].topk(2, dim=-1).values
    lead = top2[..., 0] - top2[..., 1]                                     # [item, pixel, head, frame]
    out_ = (lead < DENSE_LEAD) | (top2[..., 0].abs() >= DENSE_TOP)
    share = float(out_.double().mean())
    assert share <= 0.05, f"tb dense {which}: {share:.3f} of the (row, head) pairs have no clear winner"
    assert bool((r["v"] != 0).all())
    win = r["logits"].argmax(-1)
    assert _same(torch.where(out_[..., None], r["v"], r["att"]), torch.where(
        out_[..., None], r["v"], r["v"].gather(3, win[..., None].expand(-1, -1, -1, -1, TB_D)))), f"tb dense {which}: O != V[arg-max]"
    # out column n reads O of head src_of(n) // 40: leave the unclear (row, head) pairs out
    keep_rh = (~out_).permute(0, 3, 1, 2).reshape(m, HEADS)
    c.keep = keep_rh[:, src_of(ch, TB_C) // TB_D]
    c.conditions.append(f"{share:.3f} of the (row, head) pairs left out (<= 0.05), the others lead by >= {float(lead[~out_].min()):.0f} bits with "
                        f"|winning logit| <= {float(top2[..., 0][~out_].abs().max()):.0f}")
    return c


def tb_cases(el, b, f, hw, dev="cpu"):
    return [tb_counted(el, b, f, hw, dev), tb_routing_v(el, b, f, hw, dev), tb_routing_qk(el, b, f, hw, dev), tb_tilted(el, b, f, hw, dev),
            tb_dense_v(el, b, f, hw, dev), *tb_dense_cases(el, b, f, hw, dev), tb_routing_v(el, b, f, hw, dev, own_stats=True)]


def tb_dense_cases(el, b, f, hw, dev="cpu", which=("q", "k")):
    return [tb_dense_qk(el, b, f, hw, w, dev, v) for w in which for v in range(dense_variants(f))]


def tb_kernel_operands(c):
    """What ops.tblock_fused takes (stats None: ln_stats == NULL)."""
    o, el = c.o, c.el
    stats = None if o["mean"] is None else torch.stack([o["mean"], o["rstd"]], 1).to(F32).contiguous()
    return dict(x=o["x"].to(el), wqkv=o["wqkv"].to(el).contiguous(), bqkv=o["bqkv"].to(F32), colsum=o["colsum"].to(F32),
                pe=o["pe"].to(F32).contiguous(), wo=o["wo"].to(el).contiguous(), bo=o["bo"].to(F32), stats=stats, eps=o["eps"])


TB_MUTANTS = ("a padded key frame unmasked (f = 24)", "the last frame or token dropped", *NEIGHBOUR, "heads swapped in the out-projection input",
              "pe row of frame + 1", "pe row of frame - 1", "pe added after the rounding of q / k / v", *PADDED_SCALE,
              "mean * colsum dropped", "mean * colsum applied with rstd outside")
TB_EMULATIONS = {**FF_EMULATIONS, "row sum taken from the rounded P": dict(sum_rounded=True),
                 "float32 backwards, row sum from the rounded P": dict(order="backwards", sum_rounded=True),
                 "scaled row maximum rounded to float32 on its own": dict(max_rounded=True),
                 "the same, row sum from the rounded P": dict(max_rounded=True, sum_rounded=True)}
TB_OWN_EMULATIONS = {"own statistics at the upper row-statistics bound": dict(stat_err=1.0),
                     "own statistics at the lower row-statistics bound": dict(stat_err=-1.0)}


# ===================================================================================================== audio cross-attention
def ax_scale(d):
    """log2(e) / sqrt(d) as the pack computes it: float32 operands, float32 division."""
    return float(torch.tensor(1.4426950408889634, dtype=F32) / torch.sqrt(torch.tensor(float(d), dtype=F32)))


def ax_stats_in(o, f32=False):
    """(mean, rstd) [rows] of the statistics operand: [rows, 2] as given, [rows, 4] finished as the kernel does (eps 1e-5) - in
    float64, or (an emulation) step by step in float32 with the float32 1 / C."""
    st, cdim = o["stats"], o["x"].shape[1]
    if st.shape[1] == 2:
        return st[:, 0], st[:, 1]
    if f32:
        t = st.to(F32)
        inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(cdim), dtype=F32)
        mean = (t[:, 0] + t[:, 2]) * inv
        var = ((t[:, 1] + t[:, 3]) * inv - mean * mean).clamp_min(0.0)
        return mean.to(F64), (1.0 / torch.sqrt(var + torch.tensor(1e-5, dtype=F32))).to(F64)
    mean = (st[:, 0] + st[:, 2]) / cdim
    var = ((st[:, 1] + st[:, 3]) / cdim - mean * mean).clamp_min(0.0)
    return mean, 1.0 / torch.sqrt(var + 1e-5)


def _ax_contract(xf, w, emu):
    """xf [F, R, K], w [F, N, K] -> [F, R, N] (float64, or float32 chunks for an emulation)."""
    if emu is None or "order" not in emu:
        return torch.einsum("frk,fnk->frn", xf, w)
    return torch.stack([_mm(xf[i], w[i].t(), emu) for i in range(xf.shape[0])])


def ax_forward(c, mut=None, emu=None, parts=False):
    o, el, s = c.o, c.el, c.shape
    cdim, frames, rpf = s["c"], s["frames"], s["rows_per_frame"]
    d = cdim // HEADS
    emu = emu or {}
    x, kv, alpha = o["x"], o["kv"], o["alpha"]
    kk = kv[:, :cdim].reshape(frames, TOKENS, HEADS, d)
    vv = kv[:, cdim:].reshape(frames, TOKENS, HEADS, d)
    scale = ax_scale(d)
    if mut in PADDED_SCALE:
        scale = scale * (d / (-(-d // PADDED_SCALE[mut]) * PADDED_SCALE[mut])) ** 0.5
    kq = torch.einsum("fthj,hjc->fhtc", kk, o["wq"].reshape(HEADS, d, cdim)) * scale
    kq_r = round_el(kq, el)
    colsum = (kq if mut == "colsum of unrounded Kq" else kq_r).sum(-1)                         # [F, H, T]
    sbias = torch.einsum("fthj,hj->fht", kk, o["bq"].reshape(HEADS, d)) * scale
    vo = round_el(torch.einsum("fthj,nhj->fhtn", vv, o["wo"].reshape(cdim, HEADS, d)), el)     # [F, H, T, C]
    if mut in NEIGHBOUR and NEIGHBOUR[mut] != 1:                # token 0 of the next frame ("item") / of the next head
        dim = 0 if NEIGHBOUR[mut] == 0 else 1
        kq_r, colsum, sbias, vo = kq_r.clone(), colsum.clone(), sbias.clone(), vo.clone()
        for t_ in (kq_r, colsum, sbias, vo):
            t_[:, :, 0] = t_.roll(-1, dim)[:, :, 0]
    if mut == "heads swapped in the out-projection input":
        vo = vo[:, [1, 0] + list(range(2, HEADS))]
    mean, rstd = ax_stats_in(o, f32=bool(emu.get("stats32")))
    mean, rstd = mean.reshape(frames, rpf, 1, 1), rstd.reshape(frames, rpf, 1, 1)
    acc = _ax_contract(x.reshape(frames, rpf, cdim), kq_r.reshape(frames, HEADS * TOKENS, cdim), emu).reshape(frames, rpf, HEADS, TOKENS)
    cs, sb = colsum[:, None], sbias[:, None]
    if mut == "mean * colsum dropped":
        sl = rstd * acc + sb
    elif mut == "mean * colsum applied with rstd outside":
        sl = rstd * acc - mean * cs + sb
    else:
        sl = rstd * (acc - mean * cs) + sb
    vo_t = vo
    if mut == "the last frame or token dropped":
        sl, vo_t = sl[..., :-1], vo[:, :, :-1]
    elif mut == "a padded token slot counted":                  # zero weights: logit 0, VO 0
        sl = torch.cat([sl, torch.zeros_like(sl[..., :1])], -1)
        vo_t = torch.cat([vo, torch.zeros_like(vo[:, :, :1])], 2)
    p = torch.exp2(sl - sl.amax(-1, keepdim=True))
    den = p.sum(-1, keepdim=True)
    if "rcp" in emu:                                            # the normalisation as a float32 product with a 1-ulp reciprocal
        inv = (1.0 / den).to(F32)
        inv = torch.nextafter(inv, torch.full_like(inv, math.inf * emu["rcp"])) if emu["rcp"] else inv
        pn = (p.to(F32) * inv).to(F64)
    else:
        pn = p / den
    pr = round_el(pn, el)
    y = torch.einsum("frht,fhtn->frn", pr, vo_t).reshape(frames * rpf, cdim)
    bo = o["bo"]
    if mut == "alpha applied to the residual":
        out = round_el(alpha * (x + y + bo), el)
    elif mut == "bias_o outside alpha":
        out = round_el(x + alpha * y + bo, el)
    elif mut == "output rounded twice (before the residual)":
        out = round_el(x + round_el(alpha * (y + bo), el), el)
    else:
        out = round_el(x + alpha * (y + bo), el)
    if parts:
        return dict(logits=sl, p=pr, vo=vo, kq=kq_r, out=out)
    return out


def _ax_stats(m, cdim, dev, fmt, rstds=(0.5, 1.0, 2.0), positive=False):
    """Hand-made statistics as the operand [m, 2] (mean, rstd), or [m, 4] two-part sums (sum, sum of squares per half row) that
    finish to them: float32 values, so rstd comes out within 2^-22 of the nominal one (only cases with margins use these)."""
    mean, rstd = hand_stats(m, dev, rstds)
    if positive:
        mean = mean.abs()
    if fmt == 2:
        return torch.stack([mean, rstd], 1), mean, rstd
    tot, sq = mean * cdim, cdim * (1.0 / rstd ** 2 - 1e-5 + mean ** 2)
    r = _ar(m, dev)
    d1, d2 = small_ints(121, 3, dev, r), small_ints(122, 3, dev, r)       # the halves differ
    st = torch.stack([tot / 2 + d1, sq / 2 + d2, tot / 2 - d1, sq / 2 - d2], 1).to(F32).to(F64)
    return st, mean, rstd


def _ax_case(name, el, cdim, frames, rpf, dev, x, kv, wq, bq, wo, bo, alpha, stats, bound="bits", wo_selector=True):
    o = dict(x=x, kv=kv, wq=wq, bq=bq, wo=wo, bo=bo, alpha=alpha, stats=stats, wo_selector=wo_selector)
    c = Case("ax", name, el, dict(c=cdim, frames=frames, rows_per_frame=rpf), o, bound=bound, zero_tol=LEAK_TOL if bound == "bits" else 0.0)
    for k_ in ("x", "kv", "wq", "wo"):
        assert representable(o[k_], el), f"audio {name}: {k_} is not representable in {el}"
    d = cdim // HEADS
    kk, vv = kv[:, :cdim].reshape(-1, HEADS, d), kv[:, cdim:].reshape(-1, HEADS, d)
    m1 = torch.einsum("thj,hjc->thc", kk.abs(), wq.reshape(HEADS, d, cdim).abs()) * 2.0 ** -min(_grain(kk) + _grain(wq), 0)
    m2 = torch.einsum("thj,nhj->thn", vv.abs(), wo.reshape(cdim, HEADS, d).abs()) * 2.0 ** -min(_grain(vv) + _grain(wo), 0)
    assert exact_in_f32(m1, m2), f"audio {name}: a sum of the pack can leave 2^24 units"
    return c


def _ax_geom(cdim, frames, rpf):
    return A.Geom(frames, HEADS, rpf, TOKENS, cdim // HEADS, 1)


def _ax_wo(cdim, dev, salt):
    return selector(cdim, cdim, salt, dev), small_ints(salt + 1, 8, dev, _ar(cdim, dev))


def ax_counted(el, cdim, frames, rpf, dev="cpu", fmt=2, alpha=1.0):
    """x[r, :] = mean[r] under hand-made statistics: LayerNorm(x) = 0, so S = rstd (x . Kq - mean colsum) = 0 for every token IF
    colsum holds the sums of the rounded Kq the product sees - every P is round(1 / 5).  V = attention_cases.counted (v0, and
    v0 + 5 on the last token): out = x + alpha (round(1 / 5) 5 (v0 + 1) 2^e + bias_o) exactly."""
    m = frames * rpf
    ca = A.counted(_ax_geom(cdim, frames, rpf), el)
    stats, mean, rstd = _ax_stats(m, cdim, dev, fmt)            # (two-part: sum = mean C exactly, so the float64 mean is exact)
    x = mean[:, None].expand(m, cdim).contiguous()
    ch = _ar(cdim, dev)
    kcode = 2.0 - 4.0 * ((_hash(131, _ar(frames * TOKENS, dev)[:, None], ch[None, :]) >> 6) & 1).to(F64)
    wq = selector(cdim, cdim, 132, dev, exps=(0,))
    wo, bo = _ax_wo(cdim, dev, 133)
    c = _ax_case("counted", el, cdim, frames, rpf, dev, x, torch.cat([kcode, ca.v.double().to(dev)], 1), wq, _zeros(cdim, dev=dev), wo, bo,
                 alpha, stats)
    r = ax_forward(c, parts=True)
    fifth = round_el(torch.tensor(0.2, dtype=F64), el)
    assert bool((r["logits"] == 0).all()) and bool((r["p"] == fifth).all()), "audio counted: a logit is not 0"
    att = ca.expected.double().to(dev) * 5 * fifth              # [m, C] of (frame, head): round(1/5) * (4 v0 + v0 + 5)
    assert torch.equal(r["out"], round_el(x + alpha * (att @ wo.t() + bo), el)), "audio counted: the reference is not the closed form"
    c.conditions.append(f"every logit 0, P = round(1/5) = {float(fifth)!r}, out == x + alpha (5 P (v0 + 1) 2^e + bias_o)")
    return c


def _ax_x_for(q, wq, bq, mean, rstd):
    """x with rstd (x - mean) wq^T + bq == q (the block's own column sums make the fold a true LayerNorm of given statistics)."""
    return _realize(q, wq, torch.ones(q.shape[1], dtype=F64, device=q.device) * wq.sum(1), mean, rstd, bq[None, :].expand_as(q))


def ax_routing(el, cdim, frames, rpf, dev="cpu", fmt=2, alpha=1.0):
    """attention_cases.routing with n_kv = 5: the query of row r is the code of token pi(r, head) of the row's frame, from x
    through the selector to_q; out == x + alpha (2^e V[pi] + bias_o), V rows random and distinct."""
    m = frames * rpf
    r0 = A.routing(_ax_geom(cdim, frames, rpf), el)
    stats, mean, rstd = _ax_stats(m, cdim, dev, fmt)
    wq = selector(cdim, cdim, 141, dev)
    bq = small_ints(142, 2, dev, _ar(cdim, dev))
    x = _ax_x_for(r0.q.double().to(dev), wq, bq, mean, rstd)
    wo, bo = _ax_wo(cdim, dev, 143)
    c = _ax_case("routing", el, cdim, frames, rpf, dev, x, torch.cat([r0.k.double(), r0.v.double()], 1).to(dev), wq, bq, wo, bo, alpha, stats)
    r = ax_forward(c, parts=True)
    pi = r0.pi.to(dev)                                                        # [frames, rpf, heads]
    lead, top = _margin(r["logits"], pi)
    assert lead >= 40 and top < 2 ** 10 + 64, f"audio routing: margin {lead} bits, winning logit {top}"
    onehot = torch.zeros_like(r["p"]).scatter_(-1, pi[..., None], 1.0)
    assert torch.equal(r["p"], onehot), "audio routing: P is not one-hot"
    c.conditions.append(f"token pi leads by {lead:.0f} bits, P one-hot, out == x + alpha (2^e V[pi] + bias_o)")
    return c


def ax_tilted(el, cdim, frames, rpf, dev="cpu", fmt=2, alpha=1.0):
    """attention_cases.tilted with 5 tokens (q = 1 from x, two logit levels ~4 bits apart, V = 1 / 5).  Positive selectors, mean
    >= 0 and bias_o = 0: no cancellation in x + alpha 2^e O."""
    m = frames * rpf
    ti = A.tilted(_ax_geom(cdim, frames, rpf), el)
    stats, mean, rstd = _ax_stats(m, cdim, dev, fmt, positive=True)
    wq = selector(cdim, cdim, 151, dev).abs()
    x = _ax_x_for(torch.ones(m, cdim, dtype=F64, device=dev), wq, _zeros(cdim, dev=dev), mean, rstd)
    c = _ax_case("tilted", el, cdim, frames, rpf, dev, x, torch.cat([ti.k.double(), ti.v.double()], 1).to(dev), wq, _zeros(cdim, dev=dev),
                 selector(cdim, cdim, 152, dev).abs(), _zeros(cdim, dev=dev), alpha, stats, bound="ulp")
    r = ax_forward(c, parts=True)
    gap = r["logits"][..., 0] - r["logits"][..., 1]
    assert 3 < float(gap.min()) and float(gap.max()) < 5, f"audio tilted: logit levels {float(gap.min())} .. {float(gap.max())} bits apart"
    c.conditions.append(f"two logit levels {float(gap.min()):.3f} .. {float(gap.max()):.3f} bits apart")
    return c


def ax_dense_vo(el, cdim, frames, rpf, dev="cpu", fmt=2, alpha=1.0):
    """routing's queries and keys (P one-hot), V in {-1, 0, 1} and a dense +-1 to_out: VO is an exact integer product, out == x +
    alpha (sum over heads of VO[(head, pi)] + bias_o).  Every packed VO column."""
    m, d = frames * rpf, cdim // HEADS
    r0 = A.routing(_ax_geom(cdim, frames, rpf), el)
    stats, mean, rstd = _ax_stats(m, cdim, dev, fmt)
    wq = selector(cdim, cdim, 161, dev)
    bq = _zeros(cdim, dev=dev)
    x = _ax_x_for(r0.q.double().to(dev), wq, bq, mean, rstd)
    ch = _ar(cdim, dev)
    v = a_value(1, _ar(frames * TOKENS, dev)[:, None], 0, ch[None, :], min(1.0, 16.0 / d))
    wo = w_value(14, ch[:, None], 0, 0, ch[None, :])
    c = _ax_case("dense out-projection", el, cdim, frames, rpf, dev, x, torch.cat([r0.k.double().to(dev), v], 1), wq, bq, wo,
                 small_ints(162, 8, dev, ch), alpha, stats, wo_selector=False)
    r = ax_forward(c, parts=True)
    exact_vo = torch.einsum("fthj,nhj->fhtn", v.reshape(frames, TOKENS, HEADS, d), wo.reshape(cdim, HEADS, d))
    assert torch.equal(r["vo"], exact_vo), "audio dense out-projection: VO needs rounding"
    c.conditions.append(f"VO exact integers (max {float(exact_vo.abs().max()):g}), P one-hot")
    return c


def ax_cases(el, cdim, frames, rpf, dev="cpu", fmt=2):
    """counted, routing, tilted, dense out-projection with alpha = 1, 0.5, 2, 0.5."""
    return [ax_counted(el, cdim, frames, rpf, dev, fmt, 1.0), ax_routing(el, cdim, frames, rpf, dev, fmt, 0.5),
            ax_tilted(el, cdim, frames, rpf, dev, fmt, 2.0), ax_dense_vo(el, cdim, frames, rpf, dev, fmt, 0.5)]


def ax_kernel_operands(c):
    o, el = c.o, c.el
    return dict(x=o["x"].to(el), kv=o["kv"].to(el).contiguous(), wq=o["wq"].to(el).contiguous(), bq=o["bq"].to(F32), wo=o["wo"].to(el).contiguous(),
                bo=o["bo"].to(F32), alpha=o["alpha"], stats=o["stats"].to(F32).contiguous())


AX_MUTANTS = ("a padded token slot counted", "the last frame or token dropped", "the neighbouring item's key and value",
              "the neighbouring head's key and value", "heads swapped in the out-projection input", *PADDED_SCALE, "colsum of unrounded Kq",
              "mean * colsum dropped", "mean * colsum applied with rstd outside", "output rounded twice (before the residual)",
              "alpha applied to the residual", "bias_o outside alpha")
AX_EMULATIONS = {**FF_EMULATIONS, "P normalised by a float32 reciprocal": dict(rcp=0), "... one ulp above": dict(rcp=1),
                 "... one ulp below": dict(rcp=-1),
                 "two-part statistics finished in float32": dict(stats32=True)}


# ----------------------------------------------------------------------------------------------------- statistics of the stored rows
def _sum_rule(v, power):
    """gemm_cases._sum_tol over the last axis with the values' true granularity (it knows units down to 1/4 only): None where
    every partial sum of v^power is exact in float32, else N 2^-24 of the mass (first-order bound of any float32 summation)."""
    unit = 2.0 ** _grain(v)
    mass = (v.abs() ** power).sum(-1)
    if float(mass.max()) / unit ** power < 2 ** 24:
        return None
    return v.shape[-1] * 2.0 ** -24 * mass


def stats_of(stored, parts, eps, mut=None):
    """What stats_out must hold for the STORED rows (float64 [rows, C]) -> (want [rows, 2 | 4], tolerance [rows, 2 | 4]).
    parts = 2: (sum, sum of squares) per half row under gemm_cases._sum_tol's rule (equal where every partial sum is exact in
    float32, else N 2^-24 of the mass).  parts = 0: (mean, rstd) under norm_cases' rule for vx_row_stats: mean 2^-23 relative
    (float32 1 / c and one product); rstd 2^-16 relative, their constant, wherever their derivation stays below it: the error of
    var = E[x^2] - mean^2 is (E[x^2] + 2 mean^2) 2^-23 = (3 mean^2 + var) 2^-23, relative to var + eps, HALF of it in rstd, plus
    2^-22 for the division and the reciprocal square root.  The rows stored here leave norm_cases' |m| <= 6, s >= 1 construction
    (a row may be almost constant around a large mean), so where that derivation exceeds 2^-16 it is the tolerance; and where
    the float32 sums of a row are not exact (float16 rows of 11-bit values) the sum rule's N 2^-24 of the mass is carried
    through both.  tests/test_gpu_blocks_exact.py prints the widest relative tolerance it used."""
    rows, cdim = stored.shape
    if parts == 2:
        v = stored.reshape(rows, 2, cdim // 2)
        want = torch.stack([v.sum(2), (v * v).sum(2)], 2).reshape(rows, 4)
        t1, t2 = _sum_rule(v, 1), _sum_rule(v, 2)
        z = torch.zeros(rows, 2, dtype=F64, device=stored.device)
        tol = torch.stack([z if t1 is None else t1, z if t2 is None else t2], 2).reshape(rows, 4)
        if mut == "two-part statistics halves swapped":
            want = want[:, [2, 3, 0, 1]]
        return want, tol
    mean = stored.mean(1)
    var = ((stored - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / torch.sqrt(var + eps)
    t1, t2 = _sum_rule(stored, 1), _sum_rule(stored, 2)
    z = torch.zeros(rows, dtype=F64, device=stored.device)
    d_mean = mean.abs() * 2.0 ** -23 + (z if t1 is None else t1) / cdim
    d_var = (var + mean ** 2) * 2.0 ** -23 + (z if t2 is None else t2) / cdim + 2 * mean.abs() * d_mean
    return torch.stack([mean, rstd], 1), torch.stack([d_mean, rstd * torch.clamp(0.5 * d_var / (var + eps) + 2.0 ** -22, min=2.0 ** -16)], 1)


FORWARD = {"ff": ff_forward, "tb": tb_forward, "ax": ax_forward}
MUTANTS = {"ff": FF_MUTANTS, "tb": TB_MUTANTS, "ax": AX_MUTANTS}
EMULATIONS = {"ff": FF_EMULATIONS, "tb": TB_EMULATIONS, "ax": AX_EMULATIONS}
STATS_MUTANTS = ("two-part statistics halves swapped",)


# ----------------------------------------------------------------------------------------------------- the old bounds
OLD_TB_MUTANTS = ("a padded key frame unmasked (f = 24)", "the last frame or token dropped", "pe added after the rounding of q / k / v")
OLD_AX_MUTANTS = ("a padded token slot counted", "colsum of unrounded Kq", "output rounded twice (before the residual)")


def old_bound_figures(el=torch.bfloat16):
    """name -> (max|err| / allowed, relL2 / allowed) of a mutant of the reference on the GAUSSIAN problems of
    tests/test_gpu_kernels.py under their bounds: the temporal block at f = 24 (max|diff| <= 2^-5 max|want|, relL2 <= 2e-3, x
    ~ 1.5 N(0, 1) + 0.3 also the residual) and the audio block at C = 320 (output: 2^-6 / 8e-3; "audio increment ...": out - x
    under 2^-4 / 2.5e-2).  Below 1 = the old test lets the defect through."""
    gen = torch.Generator().manual_seed(44)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F64)
    q_ = lambda t: round_el(t, el)
    fig = {}

    def figures(got, ref, mx, l2):
        err = (got - ref).abs()
        return float(err.max() / (mx * ref.abs().max())), float(err.norm() / ref.norm() / l2)
    b, f, hw, c = 1, 24, 8, TB_C
    m = b * f * hw
    x = q_(rn(m, c) * 1.5 + 0.3)
    wqkv, wo = q_(rn(3 * c, c) * c ** -0.5), q_(rn(c, c) * c ** -0.5)
    o = dict(x=x, wqkv=wqkv, bqkv=rn(3 * c) * 0.2, colsum=wqkv.sum(1), pe=rn(f, 3 * c) * 0.5, wo=wo, bo=rn(c) * 0.2, mean=None, rstd=None,
             scale=TB_D ** -0.5, eps=1e-5)
    case = Case("tb", "gaussian", el, dict(b=b, f=f, hw=hw), o)
    for mut in OLD_TB_MUTANTS:
        fig[mut] = figures(case.forward(mut=mut), case.expected(), 2.0 ** -5, 2e-3)
    frames, rpf = 2, 64
    m = frames * rpf
    x = q_(rn(m, c) * 1.5 + 0.3)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + 1e-5)
    o = dict(x=x, kv=q_(rn(frames * TOKENS, 2 * c) * 1.2), wq=q_(rn(c, c) * c ** -0.5), bq=rn(c) * 0.2, wo=q_(rn(c, c) * c ** -0.5), bo=rn(c) * 0.3,
             alpha=3.0, stats=torch.stack([mean, rstd], 1))
    case = Case("ax", "gaussian", el, dict(c=c, frames=frames, rows_per_frame=rpf), o)
    for mut in OLD_AX_MUTANTS:
        got, ref = case.forward(mut=mut), case.expected()
        fig[mut] = figures(got, ref, 2.0 ** -6, 8e-3)
        fig["audio increment: " + mut] = figures(got - x, ref - x, 2.0 ** -4, 2.5e-2)
    return fig
