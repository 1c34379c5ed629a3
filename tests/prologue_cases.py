"""The once-per-clip prologue's kernel routes as problems whose correct answer is known exactly: a float64 reference, mutants of
that reference and float32 emulations of legitimate designs.

Host only (torch on any device, no import of v_express_amd): tests/test_prologue_cases_cpu.py shows that the cases are right and
which subtly wrong kernel they tell from a right one; tests/test_gpu_prologue_exact.py feeds them to the kernels.

wav2vec2 -> AudioProjection, VKpsGuider and the VAE encoder are otherwise checked end to end on Gaussian operands
(tests/test_gpu_prologue.py: relative L2 <= 2e-2 .. 3e-2 through up to 20 layers, 4e-3 .. 6e-3 per kernel).  They drive vx_gemm
and its neighbours in ways no case of tests/gemm_cases.py reaches: A rows that OVERLAP (row stride below the row length),
VX_ACT_GELU in the STORE epilogue and in the split-K reduction, sixteen launches that each write a 48-column slice of one
output, and the raw-waveform convolution.  (The small-channel convolutions and vx_small_kv_attention at d = 64 are new entries
of gemm_cases.ROUTES and attention_cases.small_kv_geoms.)

As in gemm_cases the operands are small integers from a counter hash (`gemm_cases._hash`) of their LOGICAL coordinates - the
waveform of (sample), x of (token, channel), W of (output channel, tap, input channel) with the group folded into the channel
numbers, the bias of (column), the residual of (row, column) - so every product and partial sum is exact in float32, the answer
does not depend on summation order, tile or route, and the expected output is the exact value rounded ONCE.

  Wave        vx_wave_conv1d, bit-equal.  `signs`: wave in {-1, 0, 1}, weights +-1.  `rounding`: wave = B + r, r in {-1, 0, 1},
              weight +1 on even and +3 on odd channels, B = round(1.25 * 2^p / taps) with p = 8 (bfloat16) / 11 (float16): the
              sums lie around 1.25 * 2^p (unit 2) and 3.75 * 2^p (unit 4), about 3/8 ties and 1/4 other roundings.  The builder
              asserts >= 1/4 and >= 1/6 from 14 time steps on: all channels of ONE time step share one sum of r, so a single
              step gives two distinct outputs and no share.  `samples` leaves stride - 1 unused trailing samples, which hold
              2^20: a miscounted t_out or offset reads them.
  Windows     out[t, n] = act(sum_{j, ci} W[n, j, ci] x[t s + j, ci] + bias[n]) (+ residual): vx_gemm over overlapping rows
              (k = s = 1: a plain linear).  x is DENSE (the windows need ld == C), so it lies between guard rows of 777 and
              unused trailing tokens hold 2^20 (2^15 in float16, whose largest number is 65504).
              `signs`, `rounding`: gemm_cases' constructions, bit-equal; `rounding + gelu`: every argument is >= 32, where
              gelu is the identity in float32, so the same bits.
              `saturated` (GELU): bias +-128 on alternating 8-column blocks, density 32 / K, alpha 2: arguments >= 32 give
              the argument, arguments <= -32 give |gelu| < 2^-40 (out == residual; without one |out| <= 2^-40 alpha).
              `middle` (GELU): x has ONE +-1 per token, so |sum| <= k, and |bias| <= 8 - k: integer arguments in [-8, 8], 0
              among them.  Argument 0 gives 0 exactly.  Into float32: |out - float64| <= GELU_ABS + 2^-24 |float64|, GELU_ABS
              = 5.1e-7 being what csrc/vx_common.h documents for gelu_f.  Into the element type: the value just below or
              above SOME float32 result inside that bound.  From 0.13 upwards a bfloat16 unit exceeds 1e-6 and this is
              norm_cases' `activated` rule, one of the two neighbours of the float64 x Phi(x).  It cannot be that rule on
              the negative tail: gelu(-5) = -1.4e-6 has a bfloat16 unit of 7e-9 and gelu(-8) = -5e-15 one of 3e-17, which
              no float32 evaluation reaches - torch's own float32 erf form returns -0.0 at -8 - and norm_cases puts no
              GELU argument between -32 and -4 for that reason.  The tanh form is 13 bfloat16 units off at x = -3 and 59 at
              x = -4 (4.1e-4 and 5.6e-5 against the 1e-6 the bound adds), so nothing the rule is for is lost.
  Positional  x + gelu(grouped conv1d(x, padding kp // 2)[..., :-1] + bias) as Wav2Vec2Model._positional computes it: G launches
              over a group-major zero-padded copy.  The GELU is always on, so `signs` carries a bias offset of +128 and both
              `signs` and `rounding` density 256 / K (arguments >= 32: the identity); `saturated` as above, alpha 1.  x is
              the residual; where it is 0 behind a low argument the tiny gelu itself is stored, |out| <= 2^-40.

`MUTANTS` edit the REFERENCE (never a kernel); `emulate_*` are legitimate designs.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

import gemm_cases as G
from gemm_cases import EL_NAME, ELEMS, F64, SIG_BITS, _ar, _hash, round_el, small_ints, tie_shares

GUARD = 777.0
GELU_ABS = 5.1e-7               # the absolute error csrc/vx_common.h documents for gelu_f in float32


def unused_fill(el):
    return 2.0 ** 15 if el is torch.float16 else 2.0 ** 20


def gelu64(x):
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_sigmoid64(x):
    return x * torch.sigmoid(1.702 * x)


def _act(x, act, mut):
    if act != "gelu":
        return x
    return gelu_tanh64(x) if mut == "tanh-form GELU" else gelu_sigmoid64(x) if mut == "sigmoid-form GELU" else gelu64(x)


def neighbours(a, el):
    """The element type's values just below / above (or at) the float64 a; below the smallest normal number the spacing is
    that of the subnormals (gelu(-8) = -5e-15 lies between float16's -2^-24 and 0)."""
    u = G._ulp(a, el).clamp_min(2.0 ** -24 if el is torch.float16 else 2.0 ** -133)
    return torch.floor(a / u) * u, torch.ceil(a / u) * u


@dataclass
class Want:
    lo: torch.Tensor
    hi: torch.Tensor

    def wrong(self, got):
        got = got.to(F64).to(self.lo.device)
        return ~((got >= self.lo) & (got <= self.hi))           # (NaN is wrong)


def _first_wrong(label, got, want):
    bad = want.wrong(got)
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    lo, hi = float(want.lo[idx]), float(want.hi[idx])
    return (f"{label}: {int(bad.sum())} of {bad.numel()} wrong, first at {idx}: got {float(got.to(F64)[idx])!r}, expected "
            + (repr(lo) if lo == hi else f"[{lo!r}, {hi!r}]"))


def _epilogue(c, acc, b, res, mut):
    """residual + alpha * act(acc + bias) (float64) and the activation's argument; b [n], res [m, n] or None."""
    b = b[None, :]
    if mut == "GELU before the bias" and c.act == "gelu":
        arg = acc
        y = _act(acc, c.act, mut) + b
    else:
        arg = acc + b
        if mut == "residual inside the activation" and res is not None:
            return c.alpha * _act(arg + res, c.act, mut), arg
        y = _act(arg, c.act, mut)
    return (c.alpha * y if res is None else c.alpha * y + res), arg


def _want(c, dev):
    ex, arg = c.exact(dev, with_arg=True)
    if c.kind == "middle":
        tol = GELU_ABS + 2.0 ** -24 * ex.abs()
        lo, hi = ex - tol, ex + tol
        if not c.out_f32:                   # the float32 result, wherever inside its bound, rounded down or up
            lo, hi = neighbours(lo, c.el)[0], neighbours(hi, c.el)[1]
        zero = arg == 0
        return Want(torch.where(zero, torch.zeros_like(ex), lo), torch.where(zero, torch.zeros_like(ex), hi))
    st = ex if c.out_f32 else round_el(ex, c.el)
    tol = torch.zeros_like(st)
    if c.kind == "saturated":
        # a residual of at least 1 swallows |gelu| < 2^-40; without one, or where it is 0 (the positional conv's x), the tiny
        # value is what is stored
        res = c.residual_t(dev)
        low = (arg <= -32) if res is None else (arg <= -32) & (res == 0)
        tol = low.to(F64) * 2.0 ** -40 * c.alpha
        st = torch.where(low, torch.zeros_like(st), st)
    return Want(st - tol, st + tol)


# ----------------------------------------------------------------------------------------------------- vx_wave_conv1d
@dataclass
class Wave:
    kind: str                       # signs | rounding
    taps: int
    stride: int
    c: int
    t_out: int
    el: torch.dtype
    conditions: list = field(default_factory=list)

    @property
    def name(self):
        return f"wave {self.kind}"

    @property
    def used(self):
        return (self.t_out - 1) * self.stride + self.taps

    @property
    def samples(self):              # (samples - taps) % stride == stride - 1 != 0
        return self.used + self.stride - 1

    @property
    def base(self):
        return float(round(1.25 * 2.0 ** SIG_BITS[self.el] / self.taps)) if self.kind == "rounding" else 0.0

    def text(self):
        return f"{self.name} [{EL_NAME[self.el]}] taps={self.taps} stride={self.stride} c={self.c} t_out={self.t_out} samples={self.samples}"

    def wave(self, dev):
        """float64 [samples]; the unused trailing samples hold 2^20."""
        i = _ar(self.samples, dev)
        w = (_hash(21, i) % 3 - 1).to(F64) + self.base
        return torch.where(i >= self.used, torch.full_like(w, 2.0 ** 20), w)

    def weight(self, dev):
        """float64 [taps, c], the kernel's layout."""
        j, ch = _ar(self.taps, dev)[:, None], _ar(self.c, dev)[None, :]
        if self.kind == "rounding":
            return torch.where(ch % 2 == 0, 1.0, 3.0).to(F64).expand(self.taps, self.c).contiguous()
        return 1.0 - 2.0 * ((_hash(22, j, ch) >> 7) & 1).to(F64)

    def exact(self, dev="cpu", mut=None):
        wave, w = self.wave(dev), self.weight(dev)
        wave = torch.cat([wave, torch.full((self.taps * self.t_out + 1,), GUARD, dtype=F64, device=dev)])   # (a mutant's overrun)
        step = 1 if mut == "stride 1 for s" else self.taps if mut == "row stride taken as row length" else self.stride
        idx = (_ar(self.t_out, dev) * step)[:, None] + _ar(self.taps, dev)[None, :] + (mut == "window one token late")
        if mut == "taps reversed":
            w = w.flip(0)
        elif mut == "last tap dropped":
            w = torch.cat([w[:-1], torch.zeros_like(w[-1:])])
        elif mut == "wave tap j with weight row j+1":
            w = torch.cat([w[1:], w[-1:]])
        out = wave[idx] @ w
        if mut == "t_out one short":
            out[-1] = float("nan")
        return out

    def want(self, dev="cpu"):
        st = round_el(self.exact(dev), self.el)
        return Want(st, st)

    def stored(self, dev="cpu", mut=None):
        return round_el(self.exact(dev, mut), self.el)

    def first_wrong(self, got, dev="cpu"):
        return _first_wrong(self.text(), got, self.want(dev))


WAVE_SHAPES = ((10, 5, 8, 1), (10, 5, 512, 61), (16, 3, 8, 14), (10, 5, 32, 300))     # (taps, stride, c, t_out)


def wave_cases(el, dev="cpu"):
    out = []
    for taps, stride, c, t_out in WAVE_SHAPES:
        for kind in ("signs", "rounding"):
            case = Wave(kind, taps, stride, c, t_out, el)
            assert (case.samples - taps) % stride != 0 and (case.samples - taps) // stride + 1 == t_out
            ex = case.exact(dev)
            if kind == "signs":
                assert float(ex.abs().max()) <= taps
                case.conditions.append(f"max |exact| {float(ex.abs().max()):g} <= taps")
            else:
                p = SIG_BITS[el]
                assert 2.0 ** p <= taps * case.base < 1.5 * 2.0 ** p, (taps, case.base)
                ties, other = tie_shares(ex, el)
                if t_out >= 14:
                    assert ties >= 0.25 and other >= 1 / 6, f"{case.text()}: ties {ties:.3f}, other roundings {other:.3f}"
                case.conditions.append(f"B = {case.base:g}: ties {ties:.3f}, other roundings {other:.3f} (>= 1/4, >= 1/6 from 14 steps on)")
            out.append(case)
    return out


def emulate_wave(case, order, dev="cpu"):
    """float32 accumulation of the taps forwards (the kernel's FMA chain), backwards, or as two halves added afterwards."""
    wave, w = case.wave(dev).to(torch.float32), case.weight(dev).to(torch.float32)
    idx = (_ar(case.t_out, dev) * case.stride)[:, None] + _ar(case.taps, dev)[None, :]
    terms = wave[idx][:, :, None] * w[None]                    # [t_out, taps, c]
    js = list(range(case.taps))
    parts = {"taps forwards": [js], "taps backwards": [js[::-1]], "two halves": [js[:case.taps // 2], js[case.taps // 2:]]}[order]
    sums = []
    for part in parts:
        acc = torch.zeros(case.t_out, case.c, dtype=torch.float32, device=dev)
        for j in part:
            acc = acc + terms[:, j]
        sums.append(acc)
    return round_el(sum(sums[1:], sums[0]).to(F64), case.el)


WAVE_ORDERS = ("taps forwards", "taps backwards", "two halves")


# ----------------------------------------------------------------------------------------------------- overlapping-row vx_gemm
@dataclass
class Win:
    """T tokens of C channels, k-tap windows of stride s into n columns (k = s = 1: a plain linear over T rows)."""
    kind: str                       # signs | rounding | saturated | middle
    T: int
    C: int
    k: int
    s: int
    n: int
    el: torch.dtype
    key: str = ""                   # the route vx_gemm_config_name must give the launch
    act: str = "none"               # none | gelu
    residual: bool = False
    out_f32: bool = False
    alpha: float = 1.0
    frame_rows: Optional[tuple] = None
    conditions: list = field(default_factory=list)

    @property
    def name(self):
        return self.kind + (" + gelu" if self.act == "gelu" and self.kind in ("signs", "rounding") else "") + \
            (" + residual" if self.residual else "") + (" f32" if self.out_f32 else "")

    @property
    def t_out(self):
        return (self.T - self.k) // self.s + 1

    @property
    def K(self):
        return self.k * self.C

    @property
    def used(self):
        return (self.t_out - 1) * self.s + self.k

    @property
    def dens(self):
        return min(1.0, 32.0 / self.K) if self.kind == "saturated" else G.density(self.K)

    def text(self):
        return (f"{self.name} [{EL_NAME[self.el]}] T={self.T} C={self.C} k={self.k} s={self.s} -> {self.n} "
                f"[m={self.t_out} K={self.K} alpha={self.alpha:g}]")

    def x(self, dev):
        """float64 [T, C]; tokens no window reaches hold `unused_fill`."""
        t, ch = _ar(self.T, dev)[:, None], _ar(self.C, dev)[None, :]
        if self.kind == "middle":           # ONE +-1 per token
            h = _hash(31, t)
            v = torch.where(ch == h % self.C, 1.0 - 2.0 * ((h >> 20) & 1).to(F64), torch.zeros((), dtype=F64, device=dev))
        else:
            v = G.a_value(0, t, 0, ch, self.dens)
        return torch.where(t >= self.used, torch.full_like(v, unused_fill(self.el)), v)

    def weight(self, dev):
        """float64 [n, k, C]; the kernel's matrix is its [n, k * C] view."""
        return G.w_value(0, _ar(self.n, dev)[:, None, None], _ar(self.k, dev)[None, :, None], 0, _ar(self.C, dev)[None, None, :])

    def bias(self, dev):
        j = _ar(self.n, dev)
        if self.kind == "middle":
            return small_ints(3, 8 - self.k, dev, j)
        b = small_ints(3, 8, dev, j)
        if self.kind == "rounding":
            b = b + 1.5 * 2.0 ** SIG_BITS[self.el] * torch.where(j % 2 == 0, 1.0, 4.0).to(F64)
        elif self.kind == "saturated":
            b = b + torch.where((j // 8) % 2 == 0, 128.0, -128.0).to(F64)
        return b

    def residual_t(self, dev):
        if not self.residual:
            return None
        return 2.0 * (_hash(5, _ar(self.t_out, dev)[:, None], _ar(self.n, dev)[None, :]) % 16).to(F64) - 15.0

    def windows(self, dev, mut=None):
        """float64 [t_out, k, C]: what the launch's A rows must hold (a mutant that runs past x reads the guard)."""
        x = torch.cat([self.x(dev), torch.full((self.k * self.t_out + 1, self.C), GUARD, dtype=F64, device=dev)])
        step = 1 if mut == "stride 1 for s" else self.k if mut == "row stride taken as row length" else self.s
        idx = (_ar(self.t_out, dev) * step)[:, None] + _ar(self.k, dev)[None, :] + (mut == "window one token late")
        return x[idx]

    def exact(self, dev="cpu", mut=None, acc=None, with_arg=False):
        if acc is None:
            w = self.weight(dev)
            if mut == "taps reversed":
                w = w.flip(1)
            elif mut == "last tap dropped":
                w = torch.cat([w[:, :-1], torch.zeros_like(w[:, -1:])], dim=1)
            acc = self.windows(dev, mut).reshape(self.t_out, self.K) @ w.reshape(self.n, self.K).t()
        out, arg = _epilogue(self, acc, self.bias(dev), self.residual_t(dev), mut)
        if mut == "t_out one short":
            out[-1] = float("nan")
        return (out, arg) if with_arg else out

    def want(self, dev="cpu"):
        return _want(self, dev)

    def stored(self, dev="cpu", mut=None, acc=None):
        ex = self.exact(dev, mut, acc)
        return ex if self.out_f32 else round_el(ex, self.el)

    def first_wrong(self, got, dev="cpu"):
        return _first_wrong(self.text(), got, self.want(dev))


def _check_win(c, dev):
    """The builder's conditions, verified on the reference."""
    ex, arg = c.exact(dev, with_arg=True)
    if c.kind == "signs":
        share = float((ex.abs() >= 2.0 ** SIG_BITS[c.el]).double().mean())
        assert share < 1e-3, f"{c.text()}: {share:.3g} of the exact values reach 2^{SIG_BITS[c.el]}"
        c.conditions.append(f"share of |exact| >= 2^{SIG_BITS[c.el]}: {share:.2g} (< 1e-3)")
    elif c.kind == "rounding":
        ties, other = tie_shares(ex, c.el)
        if c.t_out >= 16 and c.n >= 128:          # (gemm_cases.rounding: shares mean something over many rows AND columns)
            assert ties >= 0.25 and other >= 0.25, f"{c.text()}: ties {ties:.3f}, other roundings {other:.3f}"
        elif ex.numel() >= 32:
            assert ties > 0 and other > 0, f"{c.text()}: ties {ties:.3f}, other roundings {other:.3f}"
        c.conditions.append(f"ties {ties:.3f}, other roundings {other:.3f}")
    elif c.kind == "saturated":
        assert c.act == "gelu" and bool(((arg >= 32) | (arg <= -32)).all()), f"{c.text()}: an argument outside the saturated range"
        c.conditions.append(f"every argument saturated, {float((arg <= -32).double().mean()):.2f} of them low")
    else:
        assert c.act == "gelu" and not c.residual and c.alpha == 1.0 and c.k < 8
        assert bool((arg == torch.round(arg)).all()) and float(arg.abs().max()) <= 8 and (c.t_out * c.n < 64 or bool((arg == 0).any()))
        c.conditions.append(f"integer arguments in [{float(arg.min()):g}, {float(arg.max()):g}], {int((arg == 0).sum())} of them 0")
    if c.act == "gelu" and c.kind in ("signs", "rounding"):
        assert bool((arg >= 32).all()), f"{c.text()}: a GELU argument below 32"
        c.conditions.append("every GELU argument >= 32: the identity")
    return c


def _k(tile, addr="fast", extra=""):
    return f"gemm_kernel<{tile},STORE,{addr}{extra}>"


# (T, C, k, s, n) and the route: m = 131 crosses a 128-row tile; one unused trailing token; K = 120 on the gathering loads;
# stride 1, the heaviest overlap; one output row
WINDOW_SHAPES = (((263, 64, 3, 2, 64), _k(G.T128)), ((9, 512, 2, 2, 512), _k(G.T128)), ((8, 512, 3, 2, 512), _k(G.T128)),
                 ((263, 40, 3, 2, 160), _k(G.T128x160, "gather")), ((70, 64, 3, 1, 64), _k(G.T128)),
                 ((3, 512, 3, 2, 512), _k(G.T128)))


def window_cases(el, dev="cpu"):
    out = []
    for (T, C, k, s, n), key in WINDOW_SHAPES:
        kw = dict(T=T, C=C, k=k, s=s, n=n, el=el, key=key)
        out += [Win("signs", **kw), Win("signs", residual=True, alpha=2.0 if k * C <= 576 else 0.5, **kw), Win("rounding", **kw),
                Win("rounding", residual=True, **kw), Win("rounding", act="gelu", **kw),
                Win("saturated", act="gelu", alpha=2.0, **kw), Win("saturated", act="gelu", alpha=2.0, residual=True, **kw),
                Win("middle", act="gelu", **kw)]
    return [_check_win(c, dev) for c in out]


# VX_ACT_GELU on plain linears (m, n, K), one per classic tile and addressing, and through the split-K reduction (the 8x8 level:
# 64 rows per frame, K = 2560 -> eight slices and splitk_reduce_kernel), also into float32
GELU_LAUNCHES = (((129, 128, 64), False, _k(G.T128), None), ((300, 128, 64), True, _k(G.T128), None),
                 ((129, 136, 72), False, _k(G.T128x160, "gather"), None), ((65, 160, 64), False, _k(G.T64), None),
                 ((257, 32, 72), False, _k(G.T256x32, "gather"), None), ((129, 256, 72), True, _k(G.T128, "gather"), None),
                 ((128, 320, 2560), False, _k(G.T64, extra=",splitk8"), (64, None)),
                 ((128, 320, 2560), True, _k(G.T128x160, extra=",splitk8"), (64, None)))


def gelu_cases(el, dev="cpu"):
    out = []
    for (m, n, k), f32, key, fr in GELU_LAUNCHES:
        kw = dict(T=m, C=k, k=1, s=1, n=n, el=el, key=key, act="gelu", out_f32=f32, frame_rows=fr)
        out.append(Win("middle", **kw))
        if not f32:
            out += [Win("saturated", alpha=2.0, **kw), Win("saturated", alpha=2.0, residual=True, **kw)]
    return [_check_win(c, dev) for c in out]


def emulate_win(case, order, dev="cpu"):
    """float32 accumulation of a Win case's sums: 64-wide K chunks forwards / backwards, or tap by tap -> float64 [t_out, n]."""
    a = case.windows(dev).reshape(case.t_out, case.K).to(torch.float32)
    w = case.weight(dev).reshape(case.n, case.K).to(torch.float32)
    if order == "tap by tap":
        ch = [(j * case.C, (j + 1) * case.C) for j in range(case.k)]
    else:
        ch = [(k0, min(k0 + 64, case.K)) for k0 in range(0, case.K, 64)]
        if order == "64-wide chunks backwards":
            ch = ch[::-1]
    acc = torch.zeros(case.t_out, case.n, dtype=torch.float32, device=dev)
    for k0, k1 in ch:
        acc = acc + a[:, k0:k1] @ w[:, k0:k1].t()
    return acc.to(F64)


WIN_ORDERS = ("64-wide chunks forwards", "64-wide chunks backwards", "tap by tap")


def gelu_poly_f32(x):
    """csrc/vx_common.h's gelu_f restated in float32 torch (separate multiply and add where the kernel fuses them)."""
    x = x.to(torch.float32)
    u = x.abs().clamp(0.0, 8.0)
    q = torch.full_like(u, 3.309281237e-05)
    for c in (-7.692196523e-04, 8.080716245e-03, -5.341210216e-02, -4.587709606e-01, -1.151201725e+00, -9.999930859e-01):
        q = q * u + c
    return (x.clamp_min(0.0) - u * torch.exp2(q)).to(F64)


def gelu_erf_f32(x):
    x = x.to(torch.float32)
    return (0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))).to(F64)


GELU_DESIGNS = {"relu(x) - |x| 2^q(|x|), degree 6": gelu_poly_f32, "0.5 x (1 + erf(x / sqrt 2)) in float32": gelu_erf_f32}


def tanh_form_distance():
    """The smallest |tanh form - erf form| over the integer arguments 1 <= |x| <= 4 (1.5e-4, 9.8e-5, 4.1e-4, 5.6e-5; at |x| = 5
    the two are 1.2e-6 apart and from 6 on both are relu(x) to within 6e-9), and the same for the sigmoid form."""
    x = torch.arange(-8, 9, dtype=F64)
    x = x[(x != 0) & (x.abs() <= 4)]
    return float((gelu_tanh64(x) - gelu64(x)).abs().min()), float((gelu_sigmoid64(x) - gelu64(x)).abs().min())


# ----------------------------------------------------------------------------------------------------- the positional conv
@dataclass
class Pos:
    kind: str                       # signs | rounding | saturated
    T: int
    H: int
    G: int
    kp: int
    el: torch.dtype
    key: str = ""
    act: str = "gelu"
    alpha: float = 1.0
    out_f32: bool = False
    residual: bool = True           # x itself
    conditions: list = field(default_factory=list)

    @property
    def name(self):
        return f"positional {self.kind}"

    @property
    def cg(self):
        return self.H // self.G

    @property
    def K(self):
        return self.kp * self.cg

    @property
    def dens(self):
        return min(1.0, (32.0 if self.kind == "saturated" else 256.0) / self.K)

    def text(self):
        return f"{self.name} [{EL_NAME[self.el]}] T={self.T} H={self.H} groups={self.G} kp={self.kp} [K={self.K} per group]"

    def x(self, dev):
        return G.a_value(0, _ar(self.T, dev)[:, None], 0, _ar(self.H, dev)[None, :], self.dens)

    def weight(self, dev):
        """float64 [H, kp, cg]: output channel g * cg + co, tap, input channel ci OF THE GROUP (hashed as g * cg + ci); group
        g's kernel matrix is rows [g * cg, (g + 1) * cg) viewed as [cg, kp * cg]."""
        co = _ar(self.H, dev)[:, None, None]
        ci = _ar(self.cg, dev)[None, None, :] + (co // self.cg) * self.cg
        return G.w_value(0, co, _ar(self.kp, dev)[None, :, None], 0, ci)

    def bias(self, dev):
        j = _ar(self.H, dev)
        b = small_ints(3, 8, dev, j)
        if self.kind == "saturated":
            return b + torch.where((j // 8) % 2 == 0, 128.0, -128.0).to(F64)
        if self.kind == "rounding":         # (gemm_cases' offsets; they keep every argument >= 32 by themselves)
            return b + 1.5 * 2.0 ** SIG_BITS[self.el] * torch.where(j % 2 == 0, 1.0, 4.0).to(F64)
        return b + 128.0

    def residual_t(self, dev):
        return self.x(dev)

    def exact(self, dev="cpu", mut=None, with_arg=False):
        T, Gn, cg, kp = self.T, self.G, self.cg, self.kp
        x, w = self.x(dev), self.weight(dev).reshape(Gn, cg, kp, cg)
        front = kp // 2 - (mut in ("front padding kp//2 - 1", "first instead of last output dropped"))
        xp = torch.zeros(T + kp + 1, self.H, dtype=F64, device=dev)
        xp[front:front + T] = x
        step = kp if mut == "row stride taken as row length" else 1
        idx = ((_ar(T, dev) * step)[:, None] + _ar(kp, dev)[None, :] + (mut == "window one token late")).clamp_max(T + kp)
        win = xp[idx].reshape(T, kp, Gn, cg)                                     # [t, tap, group, ci]
        nxt = (torch.arange(Gn, device=dev) + 1) % Gn
        if mut == "group g with group g+1's input columns":
            win = win[:, :, nxt]
        elif mut == "group g with group g+1's weight":
            w = w[nxt]
        elif mut == "taps reversed":
            w = w.flip(2)
        elif mut == "last tap dropped":
            w = torch.cat([w[:, :, :-1], torch.zeros_like(w[:, :, -1:])], dim=2)
        acc = torch.einsum("tjgc,gojc->tgo", win, w).reshape(T, self.H)
        b = self.bias(dev)
        if mut == "group g with group g+1's bias slice":
            b = b.reshape(Gn, cg)[nxt].reshape(-1)
        res = x.reshape(T, Gn, cg)[:, nxt].reshape(T, self.H) if mut == "group g with group g+1's residual slice" else x
        out, arg = _epilogue(self, acc, b, res, mut)
        return (out, arg) if with_arg else out

    def want(self, dev="cpu"):
        return _want(self, dev)

    def stored(self, dev="cpu", mut=None):
        return round_el(self.exact(dev, mut), self.el)

    def first_wrong(self, got, dev="cpu"):
        return _first_wrong(self.text(), got, self.want(dev))


# (T, H, G, kp) and the route of each of the G launches: the real widths (48 columns per group, K = 6144), two row tiles of a
# 32-column group, one token
POSITIONAL_SHAPES = (((18, 768, 16, 128), _k(G.T128)), ((131, 128, 4, 16), _k(G.T256x32)), ((1, 64, 4, 16), _k(G.T256x32)))


def positional_cases(el, dev="cpu"):
    out = []
    for (T, H, Gn, kp), key in POSITIONAL_SHAPES:
        for kind in ("signs", "rounding", "saturated"):
            c = Pos(kind, T, H, Gn, kp, el, key)
            ex, arg = c.exact(dev, with_arg=True)
            if kind == "saturated":
                assert bool(((arg >= 32) | (arg <= -32)).all()), f"{c.text()}: an argument outside the saturated range"
                c.conditions.append(f"every argument saturated, {float((arg <= -32).double().mean()):.2f} of them low")
            else:
                assert bool((arg >= 32).all()), f"{c.text()}: a GELU argument below 32"
                if kind == "signs":
                    share = float((ex.abs() >= 2.0 ** SIG_BITS[el]).double().mean())
                    assert share < 1e-3, f"{c.text()}: {share:.3g} of the exact values reach 2^{SIG_BITS[el]}"
                    c.conditions.append(f"arguments >= 32; share of |exact| >= 2^{SIG_BITS[el]}: {share:.2g} (< 1e-3)")
                else:
                    ties, other = tie_shares(ex, el)
                    assert ex.numel() < 32 or (ties > 0 and other > 0)
                    assert T < 16 or H < 128 or (ties >= 0.25 and other >= 0.25), f"{c.text()}: ties {ties:.3f}, other {other:.3f}"
                    c.conditions.append(f"arguments >= 32; ties {ties:.3f}, other roundings {other:.3f}")
            out.append(c)
    return out


def emulate_pos(case, order, dev="cpu"):
    """The positional conv with float32 sums, tap by tap forwards / backwards or in 64-wide K chunks of each group's matrix,
    through the case's own epilogue -> what would be stored, float64 [T, H]."""
    T, Gn, cg, kp = case.T, case.G, case.cg, case.kp
    x, w = case.x(dev), case.weight(dev).reshape(Gn, cg, kp, cg).to(torch.float32)
    xp = torch.zeros(T + kp, case.H, dtype=torch.float32, device=dev)
    xp[kp // 2:kp // 2 + T] = x.to(torch.float32)
    win = xp[_ar(T, dev)[:, None] + _ar(kp, dev)[None, :]].reshape(T, kp, Gn, cg)
    acc = torch.zeros(T, Gn, cg, dtype=torch.float32, device=dev)
    if order.startswith("tap by tap"):
        for j in (range(kp) if order.endswith("forwards") else reversed(range(kp))):
            acc = acc + torch.einsum("tgc,goc->tgo", win[:, j], w[:, :, j])
    else:
        a, wm = win.permute(0, 2, 1, 3).reshape(T, Gn, kp * cg), w.reshape(Gn, cg, kp * cg)
        for k0 in range(0, kp * cg, 64):
            acc = acc + torch.einsum("tgk,gok->tgo", a[:, :, k0:k0 + 64], wm[:, :, k0:k0 + 64])
    out, _ = _epilogue(case, acc.reshape(T, case.H).to(F64), case.bias(dev), x, None)
    return round_el(out, case.el)


POS_ORDERS = ("tap by tap forwards", "tap by tap backwards", "64-wide chunks")


# ----------------------------------------------------------------------------------------------------- mutants
def _is(cls, cond=lambda c: True):
    return lambda c: isinstance(c, cls) and cond(c)


def _any(*fs):
    return lambda c: any(f(c) for f in fs)


# name -> whether the mutant can differ from the reference at a case (a structural fact, never read off the outputs)
MUTANTS = {
    "row stride taken as row length": _any(_is(Wave, lambda c: c.t_out > 1), _is(Win, lambda c: c.t_out > 1 and c.k != c.s),
                                           _is(Pos, lambda c: c.T > 1)),
    "window one token late": lambda c: True,
    # (the positional conv's last tap reads token t + kp - 1 - kp // 2: zero padding for every t unless T is longer than that)
    "last tap dropped": _any(_is(Wave), _is(Win, lambda c: c.k > 1), _is(Pos, lambda c: c.T > c.kp - 1 - c.kp // 2)),
    # (`rounding` on the waveform has the same weight on every tap; a `middle` window of ONE row may hold one tap only)
    "taps reversed": _any(_is(Wave, lambda c: c.kind == "signs"), _is(Win, lambda c: c.k > 1 and c.kind != "middle"), _is(Pos)),
    "stride 1 for s": _any(_is(Wave, lambda c: c.t_out > 1), _is(Win, lambda c: c.t_out > 1 and c.s > 1)),
    "t_out one short": _any(_is(Wave), _is(Win)),
    "wave tap j with weight row j+1": _is(Wave, lambda c: c.kind == "signs"),
    "front padding kp//2 - 1": _is(Pos),
    "first instead of last output dropped": _is(Pos),
    "group g with group g+1's input columns": _is(Pos),
    "group g with group g+1's weight": _is(Pos),
    "group g with group g+1's bias slice": _is(Pos),
    "group g with group g+1's residual slice": _is(Pos),
    # (a saturated argument is where every form of GELU agrees: only `middle` can tell them apart)
    "tanh-form GELU": _is(Win, lambda c: c.kind == "middle"),
    "sigmoid-form GELU": _is(Win, lambda c: c.kind == "middle"),
    "GELU before the bias": _any(_is(Win, lambda c: c.act == "gelu"), _is(Pos)),
    "residual inside the activation": _any(_is(Win, lambda c: c.kind == "saturated" and c.residual), _is(Pos, lambda c: c.kind == "saturated")),
}


def caught(case, mut, dev="cpu"):
    """Whether the mutated reference, stored as the element type would hold it, violates the case."""
    return bool(case.want(dev).wrong(case.stored(dev, mut)).any())


# ----------------------------------------------------------------------------------------------------- the old bounds
OLD_MUTANTS = {
    "wave": ("window one token late", "last tap dropped", "taps reversed", "stride 1 for s", "wave tap j with weight row j+1"),
    "windows": ("row stride taken as row length", "window one token late", "last tap dropped", "taps reversed", "stride 1 for s",
                "tanh-form GELU", "sigmoid-form GELU", "GELU before the bias"),
    "positional": ("window one token late", "last tap dropped", "taps reversed", "front padding kp//2 - 1",
                   "first instead of last output dropped", "group g with group g+1's input columns",
                   "group g with group g+1's weight", "group g with group g+1's bias slice",
                   "group g with group g+1's residual slice", "tanh-form GELU", "sigmoid-form GELU", "GELU before the bias",
                   "residual inside the activation"),
}
OLD_BOUNDS = {"wave": (4e-3, 2.0 ** -8), "windows": (6e-3, 2.0 ** -7), "positional": (6e-3, 2.0 ** -7)}


def old_bound_figures(which):
    """name -> (relL2 / allowed, max|err| / allowed) of every mutant (and of "correct") on the Gaussian problem of the per-kernel
    test of tests/test_gpu_prologue.py and under its bound (relative L2 <= rel, max|err| <= mx max|ref| + 1e-5), bfloat16: the
    float64 result rounded to the element type, and the same with one defect.  A defect PASSES while both are <= 1.
      wave        4000 samples, 32 channels, 10 taps, stride 5; weights ~ N(0, 1 / taps); 4e-3, 2^-8
      windows     T = 799, 32 channels, k = 3, s = 2, n = 32, GELU, weights ~ N(0, 2 / K), a bias ~ N(0, 0.01) added; 6e-3, 2^-7
      positional  T = 18, H = 768, 16 groups, kp = 128; weights ~ N(0, 1 / K), bias ~ N(0, 0.01); 6e-3, 2^-7"""
    import torch.nn.functional as Fn
    el = torch.bfloat16
    gen = torch.Generator().manual_seed({"wave": 1, "windows": 2, "positional": 3}[which])
    rel, mx = OLD_BOUNDS[which]
    if which == "wave":
        taps, stride, c = 10, 5, 32
        wave = torch.randn(4000, generator=gen).double()
        wt = (torch.randn(taps, c, generator=gen) * taps ** -0.5).double()

        def run(mut):
            w = wt.flip(0) if mut == "taps reversed" else torch.cat([wt[:-1], 0 * wt[-1:]]) if mut == "last tap dropped" else \
                torch.cat([wt[1:], wt[-1:]]) if mut == "wave tap j with weight row j+1" else wt
            t_out = (4000 - taps) // stride + 1
            idx = (torch.arange(t_out) * (1 if mut == "stride 1 for s" else stride))[:, None] + torch.arange(taps)[None, :] + \
                (mut == "window one token late")
            return torch.cat([wave, wave[:1]])[idx] @ w
    elif which == "windows":
        T, C, k, s, n = 799, 32, 3, 2, 32
        x = torch.randn(T, C, generator=gen).to(el).double()
        w = (torch.randn(n, k, C, generator=gen) * (2.0 / (C * k)) ** 0.5).to(el).double()
        b = (torch.randn(n, generator=gen) * 0.1).double()
        t_out = (T - k) // s + 1

        def run(mut):
            step = 1 if mut == "stride 1 for s" else k if mut == "row stride taken as row length" else s
            idx = ((torch.arange(t_out) * step)[:, None] + torch.arange(k)[None, :] + (mut == "window one token late")).clamp_max(T - 1)
            ww = w.flip(1) if mut == "taps reversed" else torch.cat([w[:, :-1], 0 * w[:, -1:]], 1) if mut == "last tap dropped" else w
            acc = x[idx].reshape(t_out, -1) @ ww.reshape(n, -1).t()
            return _act(acc, "gelu", mut) + b if mut == "GELU before the bias" else _act(acc + b, "gelu", mut)
    else:
        T, H, Gn, kp = 18, 768, 16, 128
        cg = H // Gn
        x = torch.randn(T, H, generator=gen).to(el).double()
        w = (torch.randn(H, cg, kp, generator=gen) * (kp * cg) ** -0.5).to(el).double()
        b = (torch.randn(H, generator=gen) * 0.1).double()
        nxt = (torch.arange(Gn) + 1) % Gn
        roll = lambda t: t.reshape(*t.shape[:-1], Gn, cg)[..., nxt, :].reshape(t.shape)

        def run(mut):
            xi = roll(x) if mut == "group g with group g+1's input columns" else x
            ww = w.reshape(Gn, cg, cg, kp)[nxt].reshape(w.shape) if mut == "group g with group g+1's weight" else w
            ww = ww.flip(2) if mut == "taps reversed" else torch.cat([ww[..., :-1], 0 * ww[..., -1:]], 2) if mut == "last tap dropped" else ww
            full = Fn.conv1d(xi.t()[None], ww, None, padding=kp // 2, groups=Gn)[0].t()               # [T + 1, H]
            late = mut in ("window one token late", "front padding kp//2 - 1", "first instead of last output dropped")
            acc = full[1:] if late else full[:-1]
            bb = roll(b) if mut == "group g with group g+1's bias slice" else b
            res = roll(x) if mut == "group g with group g+1's residual slice" else x
            if mut == "GELU before the bias":
                return res + _act(acc, "gelu", mut) + bb
            if mut == "residual inside the activation":
                return _act(acc + bb + res, "gelu", mut)
            return res + _act(acc + bb, "gelu", mut)
    ref = run(None)

    def figures(out):
        err = (round_el(out, el) - ref).abs()
        return (float(err.pow(2).sum().sqrt() / ref.pow(2).sum().sqrt() / rel), float(err.max() / (mx * ref.abs().max() + 1e-5)))
    return {name: figures(run(None if name == "correct" else name)) for name in ("correct",) + OLD_MUTANTS[which]}
