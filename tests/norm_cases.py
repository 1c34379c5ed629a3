"""GroupNorm / LayerNorm / row-statistics problems whose correct answer is known exactly, a float64 restatement, float32
emulations and mutants.

Host only (torch on any device, no import of v_express_amd): tests/test_norm_cases_cpu.py shows that the cases are right and that
they tell a subtly wrong normalisation from a right one; tests/test_gpu_norm_exact.py feeds them to the kernels of vx_norm.hip.

The Gaussian tests accept max|err| <= 2^-6 max|ref| and relative L2 <= 8e-3 (GroupNorm; LayerNorm 2^-7 / 6e-3): a defect in a
mean or an rstd spreads thinly over a group or a row, and eps, the unbiased variance, a truncating store or a whole group
normalised with its neighbour's statistics stay inside (`old_gn_figures`, `old_ln_figures`; tests/test_norm_cases_cpu.py).

The construction.  Operands are a counter hash of their LOGICAL coordinates (frame, pixel, channel of the concat; row, column).
Within every (frame, group) - every row for LayerNorm - of n elements exactly n / q are m - (q - 1) u and the others m + u, with
u = s / 2, s a power of two per call, m an integer in [-6, 6] that differs between neighbouring groups, frames and rows, and the
positions of the low values the n / q smallest hash keys.  q = 4 (q = 17 where n is no multiple of 4: the one-channel groups of
799 pixels): mean = m and variance = (q - 1) u^2 exactly, i.e. 0.75 s^2; the call passes eps = 0.25 s^2 (q = 17: 12 s^2), so
var + eps = (r s)^2 and rstd = 1 / (r s) exactly, r = 1 (q = 17: 4).  Every sum is a multiple of u and every sum of squares a
multiple of u^2 below 2^24 of them: any float32 summation order, slice count or slab partition gives the same bits.  gamma,
beta and the add table are signed powers of two / small dyadic values, so every float64 answer is exact in float32, and in the
"equal" cases representable in the element type or deliberately one bit beyond it.

GroupNorm's statistics are finished in float64 (gn_group_stats), so its ties are reproduced bit for bit.  LayerNorm's mean goes
through the float32 1 / c and its rstd through rsqrtf (1 ulp): its outputs are exact values perturbed by a few 2^-23, which a
store to the element type removes wherever the exact value is representable or far from a tie.  LayerNorm's `rounding` case
therefore takes its ties from beta (+ table) on channels with gamma = 0 and its other roundings from values at least a quarter
of a unit from any tie (EMULATIONS include rsqrt one ulp off either way and both variance forms: deviation 0 is required).

Cases: see `gn_cases` / `ln_cases` / `fp8_case`; bounds are `Want` intervals (lo == hi and `bits`: raw bits equal).
`MUTANTS` edit the REFERENCE (never a kernel); `EMULATIONS` are legitimate float32 designs.
"""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch

from gemm_cases import ELEMS, EL_NAME, SIG_BITS, _hash, _ulp, round_el, tie_shares  # noqa: F401

F64, F32, I64 = torch.float64, torch.float32, torch.int64


def _ar(n, dev):
    return torch.arange(n, dtype=I64, device=dev)


# ----------------------------------------------------------------------------------------------------- geometry
@dataclass(frozen=True)
class Gn:
    frames: int
    hw: int
    c1: int
    c2: int = 0
    groups: int = 32
    act: str = "none"               # none | silu | gelu
    pad: Optional[tuple] = None     # (H, W): the output goes to the interior of the zero-bordered (H + 2) x (W + 2) image
    kind = "gn"

    @property
    def c(self):
        return self.c1 + self.c2

    @property
    def cg(self):
        return self.c // self.groups

    @property
    def n(self):
        return self.hw * self.cg

    @property
    def q(self):
        return 4 if self.n % 4 == 0 else 17

    @property
    def r(self):
        return 1 if self.q == 4 else 4

    def eps(self, s):
        return (0.25 if self.q == 4 else 12.0) * s * s

    def text(self):
        return (f"gn {self.frames}x{self.hw}x{self.c1}" + (f"+{self.c2}" if self.c2 else "") + f" g{self.groups} {self.act}"
                + (f" pad{self.pad}" if self.pad else ""))


@dataclass(frozen=True)
class Ln:
    rows: int
    c: int
    kind = "ln"
    q, r = 4, 1

    @property
    def n(self):
        return self.c

    def eps(self, s):
        return 0.25 * s * s

    def text(self):
        return f"ln {self.rows}x{self.c}"


def gn_slices(hw):
    """ops._gn_slices restated (the mutant 'last statistics slice counted twice' needs the slice the kernels use)."""
    return max(1, min(64, hw // 16))


# ----------------------------------------------------------------------------------------------------- operands
def _lows(key, k):
    """key int64 [..., n], unique along the last axis -> bool, True at the k smallest."""
    kth = torch.sort(key, dim=-1).values[..., k - 1:k]
    return key <= kth


def group_mean(f, g):
    return ((3 * g + 5 * f + 2) % 13 - 6).to(F64)


def gn_input(g, s, dev="cpu", frame0=0):
    """float64 [frames, hw, C] of the logical concat (frame0: the hash's first frame, for the guard frames around a tensor)."""
    f = (_ar(g.frames, dev) + frame0)[:, None, None]
    p, ch = _ar(g.hw, dev)[None, :, None], _ar(g.c, dev)[None, None, :]
    key = _hash(11, f, p, ch) * (1 << 22) + p * g.cg + ch % g.cg
    key = key.view(g.frames, g.hw, g.groups, g.cg).permute(0, 2, 1, 3).reshape(g.frames, g.groups, g.n)
    low = _lows(key, g.n // g.q).view(g.frames, g.groups, g.hw, g.cg).permute(0, 2, 1, 3).reshape(g.frames, g.hw, g.c)
    m = group_mean(f, ch // g.cg)
    return m + 0.5 * s * torch.where(low, -(g.q - 1.0), 1.0).to(F64)


def ln_input(l, s, dev="cpu"):
    """float64 [rows, c]."""
    r, j = _ar(l.rows, dev)[:, None], _ar(l.c, dev)[None, :]
    low = _lows(_hash(12, r, j) * (1 << 22) + j, l.c // 4)
    return group_mean(torch.zeros_like(r), r) + 0.5 * s * torch.where(low, -3.0, 1.0).to(F64)


def add_table(entries, c, dev, unit=0.25):
    """float64 [entries, c], multiples of `unit` in [-4 unit, 4 unit]; a function of (entry, column) for ANY entry index."""
    return ((_hash(13, _ar(entries, dev)[:, None], _ar(c, dev)[None, :]) % 9) - 4).to(F64) * unit


# ----------------------------------------------------------------------------------------------------- activations
def act64(y, act):
    if act == "silu":
        return y / (1.0 + torch.exp(-y))
    if act == "gelu":
        return 0.5 * y * torch.erfc(-y / math.sqrt(2.0))
    return y


def _neighbours(a, el):
    """The element type's values just below / above (or at) the float64 a."""
    u = _ulp(a, el)
    return torch.floor(a / u) * u, torch.ceil(a / u) * u


@dataclass
class Want:
    lo: torch.Tensor
    hi: torch.Tensor
    bits: bool = False              # lo == hi and the raw bits of the stored value are compared


def equal(v):
    return Want(v, v, True)


def within(v, rel):
    d = v.abs() * rel
    return Want(v - d, v + d)


# ----------------------------------------------------------------------------------------------------- float64 restatements
def gn_forward(g, x, gamma, beta, eps, el, mut=None, emu=None, act="none"):
    """vx_groupnorm restated: x float64 [frames, hw, C] -> {"sums", "squares" [frames, groups], "arg" (the activation's argument),
    "out" (rounded to el, float64)}.  `mut`: a MUTANT name; `emu`: an EMULATIONS entry (float32 arithmetic in that order)."""
    F, hw, C, G, cg = g.frames, g.hw, g.c, g.groups, g.cg
    xs = x
    if mut == "second source's statistics taken with the first source's pixel stride":
        flat = x[..., g.c1:].reshape(-1)
        idx = (_ar(F, x.device)[:, None, None] * hw * g.c2 + _ar(hw, x.device)[None, :, None] * g.c1
               + _ar(g.c2, x.device)[None, None, :]) % flat.numel()
        xs = torch.cat([x[..., :g.c1], flat[idx]], dim=-1)
    if emu is not None:
        S, Q = _emu_gn_sums(g, xs, emu)
    else:
        px = xs[:, :-1] if mut == "last pixel of every frame missing from the sums" else xs
        S, Q = px.sum(1), (px * px).sum(1)                                    # per channel [F, C]
        if mut == "last statistics slice counted twice":
            sl = gn_slices(hw)
            pix = -(-hw // sl)
            start = (hw - 1) // pix * pix
            S, Q = S + xs[:, start:].sum(1), Q + (xs[:, start:] ** 2).sum(1)
    cnt = torch.full((F, C), float(g.n), dtype=F64, device=x.device)
    chmask = torch.ones(C, dtype=F64, device=x.device)
    if mut == "a channel of a group missing":
        chmask[cg - 1::cg] = 0.0
    part = (_ar(C, x.device) >= g.c1).to(I64) if mut == "the group that straddles the two sources split at the source boundary" \
        else torch.zeros(C, dtype=I64, device=x.device)
    gid = (_ar(C, x.device) // cg) * 2 + part                                # statistics pool of every channel
    pools = torch.unique(gid, return_inverse=True)[1]
    npool = int(pools.max()) + 1
    Sg = torch.zeros(F, npool, dtype=S.dtype, device=x.device).index_add_(1, pools, S * chmask.to(S.dtype))
    Qg = torch.zeros(F, npool, dtype=S.dtype, device=x.device).index_add_(1, pools, Q * chmask.to(S.dtype))
    if part.any():
        cnt = torch.zeros(npool, dtype=F64, device=x.device).index_add_(0, pools, torch.full((C,), float(hw), dtype=F64,
                                                                                          device=x.device))[pools].expand(F, C)
    Sc, Qc = Sg[:, pools].to(F64), Qg[:, pools].to(F64)                      # per channel: its pool's sums [F, C]
    if mut == "last group normalised with its neighbour's statistics":
        Sc, Qc = Sc.clone(), Qc.clone()
        Sc[:, C - cg:], Qc[:, C - cg:] = Sc[:, C - 2 * cg:C - cg], Qc[:, C - 2 * cg:C - cg]
    mean = Sc / cnt
    if mut == "variance divided by n - 1":
        var = (Qc - cnt * mean * mean) / (cnt - 1).clamp_min(1.0)
    elif emu is not None and emu.get("var") == "twopass":
        d32 = xs.to(F32) - mean.to(F32)[:, None, :]                           # float32 deviations and their float32 sum
        var = (d32 * d32).view(F, hw, G, cg).sum(dim=(1, 3)).repeat_interleave(cg, dim=1).to(F64) / cnt
    else:
        var = Qc / cnt - mean * mean
    e = 0.0 if mut == "eps left out" else eps * 100 if mut == "eps x 100" else eps
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + e)
    if emu is not None:
        mean32, rstd32 = mean.to(F32), rstd.to(F32)
        sc = gamma.to(F32) * rstd32
        sh = beta.to(F32) - mean32 * sc
        if emu.get("fma"):
            arg = (x.to(F32).to(F64) * sc.to(F64)[:, None] + sh.to(F64)[:, None]).to(F32).to(F64)
        else:
            arg = (x.to(F32) * sc[:, None] + sh[:, None]).to(F64)
    else:
        arg = (x - mean[:, None]) * rstd[:, None] * gamma + beta
    if mut == "rounding before the activation as well":
        arg = round_el(arg, el)
    out = act64(arg, act)
    out = round_el(out, el, "trunc") if mut == "truncating store" else round_el(out, el)
    # (the totals of a group: its first channel's pool)
    first = pools[::cg]
    return {"sums": Sg[:, first].to(F64), "squares": Qg[:, first].to(F64), "arg": arg, "out": out}


def _emu_gn_sums(g, x, emu):
    """Per-channel float32 sums [F, C]: slices of emu['slice'] pixels, inside a slice emu['lanes'] pixel lanes each summing its
    pixels in ascending order (cumsum), lanes then slices added in float32 / float64 as the kernels do."""
    F, hw, C = x.shape
    x32 = x.to(F32)
    sp, lanes = emu["slice"], emu["lanes"]
    S = torch.zeros(F, C, dtype=F64, device=x.device)
    Q = torch.zeros(F, C, dtype=F64, device=x.device)
    for p0 in range(0, hw, sp):
        blk = x32[:, p0:p0 + sp]
        s32 = torch.zeros(F, C, dtype=F32, device=x.device)
        q32 = torch.zeros(F, C, dtype=F32, device=x.device)
        for l in range(min(lanes, blk.shape[1])):
            mine = blk[:, l::lanes]
            s32 = s32 + torch.cumsum(mine, 1)[:, -1]
            q32 = q32 + torch.cumsum(mine * mine, 1)[:, -1]
        if emu.get("order") == "gc":                                          # groups first, in float32 (kept on the group's first channel)
            for t in (s32, q32):
                tg = t.view(F, g.groups, g.cg)
                tot = tg.sum(-1)
                tg.zero_()
                tg[:, :, 0] = tot
        S, Q = S + s32.to(F64), Q + q32.to(F64)
    return S, Q


def ln_forward(l, x, gamma, beta, eps, el, add=None, rpe=1, entries=1, mut=None, emu=None):
    """vx_layernorm / vx_row_stats / vx_row_stats_parts / vx_row_stats_finalize restated: x float64 [rows, c] ->
    {"mean", "rstd" [rows], "parts" [rows, 4], "fin_mean", "fin_rstd", "out" [rows, c] (rounded to el, float64)}."""
    rows, c = x.shape
    dev = x.device
    xs = x
    if mut == "row statistics of the neighbouring row":
        xs = x[(_ar(rows, dev) ^ 1).clamp_max(rows - 1)]
    live = torch.ones(c, dtype=F64, device=dev)
    if mut in ("last 8-channel chunk missing from the statistics", "last live chunk of the widest MAXC instantiation dropped"):
        live[c - 8:] = 0.0
    h = c // 2
    p = torch.stack([xs[:, :h].sum(1), (xs[:, :h] ** 2).sum(1), xs[:, h:].sum(1), (xs[:, h:] ** 2).sum(1)], dim=1)
    if mut == "two halves of the two-part sums swapped":
        p = p[:, [2, 3, 0, 1]]
    if emu is not None:
        x32 = xs.to(F32)
        if emu["sum"] == "chunks":
            ssum = x32.view(rows, c // 8, 8).sum(-1).sum(-1)
        elif emu["sum"] == "sequential":
            ssum = torch.cumsum(x32, 1)[:, -1]
        else:                                                                  # two 32-lane half-row trees
            ssum = x32[:, :h].sum(1) + x32[:, h:].sum(1)
        mean = ssum / c if emu["invc"] == "div" else ssum * torch.tensor(1.0 / c, dtype=F32)
        if emu["var"] == "twopass":
            var = ((x32 - mean[:, None]) ** 2).sum(1)
            var = var / c if emu["invc"] == "div" else var * torch.tensor(1.0 / c, dtype=F32)
        else:
            sq = (x32 * x32).sum(1)
            var = (sq / c if emu["invc"] == "div" else sq * torch.tensor(1.0 / c, dtype=F32)) - mean * mean
            var = var.clamp_min(0.0)
        rstd = (1.0 / torch.sqrt((var + torch.tensor(eps, dtype=F32)).to(F64))).to(F32)
        if emu["rsqrt"]:
            rstd = torch.nextafter(rstd, torch.full_like(rstd, float("inf") * emu["rsqrt"]))
        g32, b32 = gamma.to(F32), beta.to(F32)
        if emu["fma"]:
            y = (((x.to(F32) - mean[:, None]) * rstd[:, None]).to(F64) * g32.to(F64) + b32.to(F64)).to(F32)
        else:
            y = (x.to(F32) - mean[:, None]) * rstd[:, None] * g32 + b32
        if add is not None:
            y = y + add.to(F32)[(_ar(rows, dev) // rpe) % entries]
        ic = torch.tensor(1.0 / c, dtype=F32)
        p32 = p.to(F32)
        fm32 = (p32[:, 0] + p32[:, 2]) * ic
        fv32 = ((p32[:, 1] + p32[:, 3]) * ic - fm32 * fm32).clamp_min(0.0)
        fin = (fm32.to(F64), (1.0 / torch.sqrt(fv32 + torch.tensor(eps, dtype=F32))).to(F64))
        mean, rstd, y = mean.to(F64), rstd.to(F64), y.to(F64)
    else:
        mean = (xs * live).sum(1) / c
        d = (xs - mean[:, None]) * live
        div = c - 1 if mut == "variance divided by c - 1" else c
        var = (d * d).sum(1) / div
        e = 0.0 if mut == "eps left out" else eps
        rstd = 1.0 / torch.sqrt(var + e)
        y = (x - mean[:, None]) * rstd[:, None] * gamma + beta
        if add is not None:
            y = y + add[(_ar(rows, dev) // rpe) % entries]
    if mut == "rounding before the add table as well" and add is not None:
        e_idx = (_ar(rows, dev) // rpe) % entries
        y = round_el(y - add[e_idx], el) + add[e_idx]
    out = round_el(y, el, "trunc") if mut == "truncating store" else round_el(y, el)
    if mut == "last live chunk of the widest MAXC instantiation dropped":     # not processed at all: never stored either
        out = out.clone()
        out[:, c - 8:] = 0.0
    if mut == "tail row of an LN_R = 4 pass given the clamped row's output" and rows > 1:
        out = out.clone()
        out[rows - 1] = out[rows - 2]
        mean, rstd = mean.clone(), rstd.clone()
        mean[rows - 1], rstd[rows - 1] = mean[rows - 2], rstd[rows - 2]
    fm = (p[:, 0] + p[:, 2]) / c
    fv = ((p[:, 1] + p[:, 3]) / c - fm * fm).clamp_min(0.0)
    fin = fin if emu is not None else (fm, 1.0 / torch.sqrt(fv + eps))
    return {"mean": mean, "rstd": rstd, "parts": p, "fin_mean": fin[0], "fin_rstd": fin[1], "out": out, "arg": y}


# ----------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    geo: object
    el: torch.dtype
    s: float
    gamma: torch.Tensor
    beta: torch.Tensor
    add: Optional[torch.Tensor] = None
    rpe: int = 1
    entries: int = 1
    outputs: tuple = ("out",)
    conditions: list = field(default_factory=list)

    @property
    def eps(self):
        return self.geo.eps(self.s)

    @property
    def dev(self):
        return self.gamma.device

    @property
    def act(self):                  # only `activated` runs the geometry's activation
        return self.geo.act if self.name == "activated" else "none"

    def title(self):
        return f"{self.geo.text()} s={self.s:g} {self.name} [{EL_NAME[self.el]}]"

    def x(self):
        return gn_input(self.geo, self.s, self.dev) if self.geo.kind == "gn" else ln_input(self.geo, self.s, self.dev)

    def forward(self, mut=None, emu=None):
        if self.geo.kind == "gn":
            return gn_forward(self.geo, self.x(), self.gamma, self.beta, self.eps, self.el, mut, emu, self.act)
        add, entries = self.add, self.entries
        if mut == "add-table index without its % add_entries":                 # the table is a function of (entry, column)
            entries = (self.geo.rows - 1) // self.rpe + 1
            add, mut = add_table(entries, self.geo.c, self.dev), None
        return ln_forward(self.geo, self.x(), self.gamma, self.beta, self.eps, self.el, add, self.rpe, entries, mut, emu)

    def values(self, mut=None, emu=None):
        """The case's outputs as concrete float64 tensors (of the reference, a mutant or an emulation)."""
        r = self.forward(mut, emu)
        return {k: r[k] for k in self.outputs}

    def wants(self):
        """name -> Want, from the float64 restatement."""
        r = self.forward()
        w = {}
        for k in self.outputs:
            v = r[k]
            if k in ("mean", "fin_mean"):
                # float32 1 / c (2^-24) and one product (2^-24)
                w[k] = within(v, 2.0 ** -23)
            elif k in ("rstd", "fin_rstd"):
                # rsqrtf within one ulp of a variance that carries the mean's error: E[x^2] - mean^2 cancels to 0.75 s^2 from
                # m^2 + 0.75 s^2, relative error (3 m^2 + 0.75 s^2) / s^2 * 2^-23 <= 109 * 2^-23 < 2^-16 at |m| <= 6, s >= 1; half in rstd
                w[k] = within(v, 2.0 ** -16)
            elif k == "out" and self.name == "activated":
                w[k] = self._activated_want(r["arg"])
            else:
                w[k] = equal(v)
        return w

    def _activated_want(self, arg):
        a = act64(arg, self.act)
        lo, hi = _neighbours(a, self.el)                                        # elsewhere: one of the two neighbours
        ident = (arg >= 32) & (a.to(F32).to(F64) == arg)
        zero = arg == 0
        sat = arg <= -32
        ex = round_el(arg, self.el)
        lo = torch.where(ident, ex, torch.where(zero, torch.zeros_like(a), torch.where(sat, -arg.abs() * 2.0 ** -40, lo)))
        hi = torch.where(ident, ex, torch.where(zero, torch.zeros_like(a), torch.where(sat, arg.abs() * 2.0 ** -40, hi)))
        return Want(lo, hi)

    def wrong(self, got, wants):
        """name -> bool tensor of elements outside their interval (got: name -> tensor of any float type)."""
        return {k: ~((got[k].to(F64) >= w.lo) & (got[k].to(F64) <= w.hi)) for k, w in wants.items()}

    def first_wrong(self, got, wants):
        for k, bad in self.wrong(got, wants).items():
            w = wants[k]
            if w.bits and got[k].dtype in ELEMS and not bool(bad.any()):       # raw bits (the sign of zero included)
                bad = got[k].contiguous().view(torch.int16) != w.lo.to(F32).to(got[k].dtype).view(torch.int16)
            if bool(bad.any()):
                idx = tuple(int(i) for i in bad.nonzero()[0])
                return (f"{self.title()}: {k}: {int(bad.sum())} of {bad.numel()} wrong, first at {idx}: got {float(got[k][idx])!r}, "
                        f"want [{float(w.lo[idx])!r}, {float(w.hi[idx])!r}]")
        return None


def _pm(h):
    return 1.0 - 2.0 * ((h >> 9) & 1).to(F64)


def _representable(v, el):
    return bool((round_el(v, el) == v).all())


def _check_sums(c, x):
    u2 = (0.5 * c.s) ** 2
    n = c.geo.n
    worst = float((x * x).max()) * n / u2
    assert worst < 2 ** 24, f"{c.title()}: a sum of squares may reach {worst:g} units of u^2"
    c.conditions.append(f"sums of squares <= {worst:.3g} u^2 < 2^24")


def _check_construction(c):
    """The builder conditions every case shares: exact mean / variance / rstd, float32-exact answers, bounded sums."""
    g, x = c.geo, c.x()
    assert _representable(x, c.el), f"{c.title()}: an input is not representable"
    _check_sums(c, x)
    r = c.forward()
    if g.kind == "gn":
        xg = x.view(g.frames, g.hw, g.groups, g.cg)
        want_m = group_mean(_ar(g.frames, c.dev)[:, None], _ar(g.groups, c.dev)[None, :])
        mean = xg.sum(dim=(1, 3)) / g.n                                        # (exact sums: no torch.mean / var here)
        var = ((xg - want_m[:, None, :, None]) ** 2).sum(dim=(1, 3)) / g.n
        low = (xg < want_m[:, None, :, None]).double().sum(dim=(1, 3)) / g.n
    else:
        want_m = group_mean(torch.zeros(g.rows, dtype=I64, device=c.dev), _ar(g.rows, c.dev))
        mean, var = x.sum(1) / g.n, ((x - want_m[:, None]) ** 2).sum(1) / g.n
        low = (x < want_m[:, None]).double().sum(1) / g.n
    assert torch.equal(mean, want_m) and bool((var == (g.q - 1) * (0.5 * c.s) ** 2).all()) and bool((low == 1.0 / g.q).all())
    assert bool((var + c.eps == (g.r * c.s) ** 2).all())
    assert bool((r["arg"].to(F32).to(F64) == r["arg"]).all()), f"{c.title()}: an answer is not exact in float32"
    c.conditions.append(f"1/{g.q} low, mean = m, var + eps = ({g.r} s)^2, float32-exact")
    return r


def _gamma_beta(geo, dev, salt):
    ch = _ar(geo.c, dev)
    h = _hash(salt, ch)
    kmin, nk = (-1, 4) if geo.q == 4 else (1, 2)
    gamma = _pm(h) * torch.exp2((kmin + h % nk).to(F64))
    beta = (2 * ((h >> 4) % 8) - 7).to(F64) / 8
    return gamma, beta


def affine(geo, el, s, dev="cpu", add=None):
    """gamma = +-2^k, beta odd multiples of 1/8, the table multiples of 1/4: every answer an odd multiple of 1/8 below 9 -
    representable, never zero (LayerNorm's float32 perturbation of the normalised part stays far inside half a unit)."""
    gamma, beta = _gamma_beta(geo, dev, 21)
    c = Case("affine" + (f" + table{add}" if add else ""), geo, el, s, gamma, beta)
    if add:
        c.rpe, c.entries = add
        c.add = add_table(c.entries, geo.c, dev)
    r = _check_construction(c)
    assert _representable(r["arg"], el) and bool((r["arg"] != 0).all()), f"{c.title()}: an answer is not representable"
    c.conditions.append(f"answers representable, |y| in [{float(r['arg'].abs().min()):g}, {float(r['arg'].abs().max()):g}]")
    return c


def counted(geo, el, s, dev="cpu"):
    gamma, beta = _gamma_beta(geo, dev, 21)
    outs = ("sums", "squares") if geo.kind == "gn" else ("mean", "rstd", "parts", "fin_mean", "fin_rstd")
    if geo.kind == "ln" and geo.c % 16:
        outs = ("mean", "rstd")
    c = Case("counted", geo, el, s, gamma, beta, outputs=outs)
    _check_construction(c)
    return c


def rounding(geo, el, s, dev="cpu", add=None):
    p = SIG_BITS[el]
    ch = _ar(geo.c, dev)
    h = _hash(22, ch)
    a = (h & 1) == 0
    if geo.kind == "gn":
        # A: the high value lands on 1 + 2^-p (or 1 + 3 2^-p: the tie that rounds up); B: +-2^-(p+2) steps, never a tie
        gamma = torch.where(a, 2.0 * geo.r * 2.0 ** -p, _pm(h) * 2.0 * geo.r * 2.0 ** -(p + 2)).to(F64)
        beta = 1.0 + torch.where(a & (((h >> 3) & 1) == 1), 2.0 ** -(p - 1), 0.0).to(F64)
    else:
        # A: gamma = 0, beta itself the tie (both directions); B: {-0.75, +0.25} 2^-p around 1, a quarter unit from any tie
        gamma = torch.where(a, 0.0, _pm(h) * 2.0 ** -(p + 1)).to(F64)
        beta = 1.0 + torch.where(a, torch.where(((h >> 3) & 1) == 1, 3.0, 1.0) * 2.0 ** -p, 0.0).to(F64)
    c = Case("rounding" + (f" + table{add}" if add else ""), geo, el, s, gamma, beta)
    if add:                                                                     # entry 1 moves the A channels off their ties
        c.rpe, c.entries = add
        c.add = torch.zeros(c.entries, geo.c, dtype=F64, device=dev)
        c.add[1 % c.entries] = torch.where(a, 2.0 ** -(p + 2), 0.0).to(F64)
    r = _check_construction(c)
    ties, other = tie_shares(r["arg"], el)
    assert ties >= 0.25 and other >= 0.25, f"{c.title()}: ties {ties:.3f}, other roundings {other:.3f}"
    c.conditions.append(f"ties {ties:.3f}, other roundings {other:.3f}")
    if geo.kind == "ln":                                                        # margin against the float32 perturbation
        y = r["arg"]
        part = (y - beta - (c.add[(_ar(geo.rows, dev) // c.rpe) % c.entries] if add else 0.0)).abs()
        q = y.abs() / _ulp(y, el)
        fr = q - torch.floor(q)
        assert bool(((part == 0) | ((fr - 0.5).abs() * _ulp(y, el) > part * 2.0 ** -16)).all()), f"{c.title()}: a value sits too close to a tie"
        c.conditions.append("every value with a normalised part >= 2^-16 of it from a tie")
    return c


def activated(geo, el, s, dev="cpu"):
    """Five channel classes: the high value's argument 0; arguments around +64 (identity in float32) and around -64 (saturated);
    arguments of magnitude below 4 (one unit in the last place); and arguments 1 + 2^-p / 1 + 3 2^-p, ties of the element type
    (an argument rounded before the activation moves the result by 0.93 units (SiLU) / 1.08 (GELU): out of the two neighbours).
    gelu_f documents |abs err| <= 5.1e-7, which exceeds a unit of the tiny results between -32 and -4: no GELU argument is put
    there."""
    assert geo.act in ("silu", "gelu")
    ch = _ar(geo.c, dev)
    h = _hash(23, ch)
    cls = h % 5
    p = SIG_BITS[el]
    zh = 1.0 / (2 * geo.r)                                                      # the normalised high value
    # class 0: high -> 0 (gamma zh + beta = 0); the low value gives -4 (SiLU), -2 (GELU) or -2.125 (q = 17)
    gam0 = 1.0 if geo.q == 17 or geo.act == "gelu" else 2.0
    bet0 = -gam0 * zh
    gamma = torch.where(cls == 0, gam0, torch.where(cls == 3, _pm(h), _pm(h) * 2.0 * geo.r)).to(F64)
    gamma = torch.where(cls == 4, 2.0 * geo.r * 2.0 ** -p, gamma)
    beta = torch.where(cls == 0, bet0, torch.where(cls == 1, 64.0, torch.where(cls == 2, -64.0, 0.5))).to(F64)
    beta = torch.where(cls == 4, 1.0 + torch.where(((h >> 5) & 1) == 1, 2.0 ** -(p - 1), 0.0), beta)
    c = Case("activated", geo, el, s, gamma, beta)
    r = _check_construction(c)
    arg = r["arg"]
    a = act64(arg, geo.act)
    ident = (arg >= 32) & (a.to(F32).to(F64) == arg)
    assert bool((ident == (arg >= 32)).all()) and _representable(arg[ident], el), "the identity region is not where it is assumed"
    mid = (arg > -32) & (arg < 32) & (arg != 0)
    assert bool((arg[mid].abs() <= (4.0 if geo.act == "silu" else 3.99)).all()), f"{c.title()}: arguments {arg[mid].abs().max()}"
    shares = [float(m.double().mean()) for m in (arg == 0, ident, arg <= -32, mid)]
    assert min(shares) > 0.02, shares
    c.conditions.append("arguments: zero {:.2f}, identity (>= 32) {:.2f}, saturated (<= -32) {:.2f}, |arg| <= 4 {:.2f}".format(*shares))
    return c


def gn_cases(geo, el, s, dev="cpu"):
    cs = [counted(geo, el, s, dev), affine(geo, el, s, dev), rounding(geo, el, s, dev)]
    if geo.act != "none":
        cs.append(activated(geo, el, s, dev))
    return cs


def ln_cases(l, el, s, dev="cpu"):
    cs = [counted(l, el, s, dev), affine(l, el, s, dev), rounding(l, el, s, dev)]
    if l.rows >= 33 and l.rows <= 300:
        cs += [affine(l, el, s, dev, add=(8, 4)), affine(l, el, s, dev, add=(1, 1)), rounding(l, el, s, dev, add=(8, 4))]
    return cs


# ----------------------------------------------------------------------------------------------------- fp8
@dataclass
class Fp8Case:
    l: Ln
    el: torch.dtype
    norm: bool
    x: torch.Tensor                  # float64 [rows, c]
    gamma: Optional[torch.Tensor]
    beta: Optional[torch.Tensor]
    add: Optional[torch.Tensor]
    rpe: int
    entries: int
    eps: float
    y: torch.Tensor                  # the exact values that are quantised
    scale: torch.Tensor              # exact: max|y| / 448 = 2^k per row
    q: torch.Tensor                  # uint8 [rows, c]: the e4m3 bytes of y / scale
    conditions: list = field(default_factory=list)


def fp8_case(l, el, norm, dev="cpu"):
    """Rows whose quantised values are multiples of 1/2 (times the row's power of two) up to 7 = 448 / 64: y / scale is a multiple of
    32 up to 448, a four-bit integer times a power of two - representable in e4m3 (4 significand bits), so the float32 noise of
    scale = max * (1/448.f) and of LayerNorm's statistics cannot move a byte.  With normalisation gamma = +-1, beta and the table
    multiples of 1/2, and gamma = 0 channels carry the row maximum +-7 * 2^(entry % 2) through the TABLE (2 rows per entry, 4
    entries); without it the row itself is v * 2^(row % 3) with v a multiple of 1/2 and +-7 on some column of every row."""
    r, j = _ar(l.rows, dev)[:, None], _ar(l.c, dev)[None, :]
    hc = _hash(31, _ar(l.c, dev))
    top = (hc % 8) == 0                                                         # the columns that carry the maximum
    assert bool(top.any())
    if norm:
        s = 1.0
        x = ln_input(l, s, dev)
        gamma = torch.where(top, 0.0, _pm(hc)).to(F64)
        beta = torch.where(top, 0.0, ((hc >> 4) % 9 - 4).to(F64) * 0.5).to(F64)
        rpe, entries = 2, 4
        e = _ar(entries, dev)[:, None]
        k = (e % 2).to(F64)
        add = torch.where(top[None, :], _pm(_hash(32, e, j)) * 7.0 * torch.exp2(k), add_table(entries, l.c, dev, 0.25) * 2 * torch.exp2(k))
        ref = ln_forward(l, x, gamma, beta, 0.25, el, add, rpe, entries)
        y = ref["arg"]
        eps = 0.25
    else:
        v = ((_hash(33, r, j) % 27) - 13).to(F64) * 0.5
        v = torch.where(top[None, :], _pm(_hash(34, r, j)) * 7.0, v)
        x = v * torch.exp2((r % 3).to(F64))
        gamma = beta = add = None
        rpe = entries = 1
        y, eps = x, 0.0
    assert _representable(x, el)
    amax = y.abs().amax(1)
    scale = amax / 448.0
    assert bool((torch.exp2(torch.round(torch.log2(scale))) == scale).all()), "a row maximum is not 448 * 2^k"
    t = y / scale[:, None]
    q8 = t.to(F32).to(torch.float8_e4m3fn)
    assert bool((q8.to(F64) == t).all()), "a quantised value is not representable in e4m3"
    c = Fp8Case(l, el, norm, x, gamma, beta, add, rpe, entries, eps, y, scale, q8.view(torch.uint8))
    c.conditions.append(f"row maxima 448 * 2^k, k in {sorted(set(torch.log2(scale).long().tolist()))}; every y / scale in e4m3")
    return c


# ----------------------------------------------------------------------------------------------------- emulations, mutants
# GroupNorm: slices of 1 to 64 pixels summed in float32 and merged in float64; inside a slice 1 to 32 pixel lanes, each adding
# its pixels in ascending order (the kernels' 4-deep unroll adds in that same order, so it is this sum and is not modelled
# apart), lanes then channels -> groups ("cg") or groups first ("gc"); the variance from the sums of squares (float64, as
# gn_group_stats has it) or two-pass over float32 deviations; x * sc + sh with one rounding (fma) or two.
# LayerNorm: 8-element chunk sums then the lanes, a sequential sum, or two half-row sums; the float32 1 / c as a product or a
# division; two-pass or sums-of-squares variance; rsqrt correctly rounded or one ulp off either way; the affine with and without fma.
GN_EMULATIONS = [dict(slice=sp, lanes=ln, order=o, var=v, fma=f) for sp, ln, o, v, f in
                 ((1, 1, "cg", "sumsq", False), (15, 6, "cg", "sumsq", True), (17, 32, "gc", "sumsq", False),
                  (64, 4, "cg", "twopass", True), (16, 1, "gc", "twopass", False), (64, 32, "cg", "sumsq", True))]
LN_EMULATIONS = [dict(sum=sm, invc=i, var=v, rsqrt=rs, fma=f) for sm, i, v, rs, f in
                 (("chunks", "mul", "twopass", 0, False), ("chunks", "mul", "twopass", 1, True), ("chunks", "mul", "twopass", -1, False),
                  ("sequential", "div", "twopass", 0, True), ("halves", "mul", "sumsq", 0, False), ("halves", "mul", "sumsq", 1, True),
                  ("halves", "div", "sumsq", -1, False))]
EMULATIONS = {"gn": GN_EMULATIONS, "ln": LN_EMULATIONS}


def emu_name(e):
    return ", ".join(f"{k}={v}" for k, v in e.items())


def _halves_differ(c):
    p = c.values()["parts"]
    return not torch.equal(p[:, :2], p[:, 2:])


def _gn(f):
    return lambda c: c.geo.kind == "gn" and f(c)


def _ln(f):
    return lambda c: c.geo.kind == "ln" and f(c)


# name -> whether the mutant can differ from the reference at all on a case (a structural fact per mutant)
MUTANTS = {
    "eps left out": lambda c: True,
    "eps x 100": _gn(lambda c: True),
    # rstd changes by 1 / (2 n): on the tie 1 + 3 * 2^-p that moves the float32 argument only while 2^-p / (2 n) > 2^-24
    "variance divided by n - 1": _gn(lambda c: c.geo.n < 2 ** (23 - SIG_BITS[c.el])),
    "variance divided by c - 1": _ln(lambda c: True),
    "truncating store": lambda c: "out" in c.outputs,
    "rounding before the activation as well": _gn(lambda c: c.name == "activated"),
    "rounding before the add table as well": _ln(lambda c: c.add is not None and "out" in c.outputs),
    "last pixel of every frame missing from the sums": _gn(lambda c: c.geo.hw > 1),
    "last statistics slice counted twice": _gn(lambda c: True),
    "last group normalised with its neighbour's statistics": _gn(lambda c: True),
    "a channel of a group missing": _gn(lambda c: c.geo.cg > 1),
    "second source's statistics taken with the first source's pixel stride": _gn(lambda c: c.geo.c2 and c.geo.c1 != c.geo.c2
                                                                                  and c.geo.hw > 1),
    "the group that straddles the two sources split at the source boundary": _gn(lambda c: c.geo.c2 and c.geo.c1 % c.geo.cg),
    "row statistics of the neighbouring row": _ln(lambda c: c.geo.rows > 1),
    "add-table index without its % add_entries": _ln(lambda c: c.add is not None and c.geo.rows > c.rpe * c.entries
                                                    and c.name.startswith("affine")),
    "last 8-channel chunk missing from the statistics": _ln(lambda c: c.geo.c > 8),
    "last live chunk of the widest MAXC instantiation dropped": _ln(lambda c: c.geo.c > 1536),
    "tail row of an LN_R = 4 pass given the clamped row's output": _ln(lambda c: c.geo.rows % 4 != 0 and c.geo.rows > 1),
    "two halves of the two-part sums swapped": _ln(lambda c: "parts" in c.outputs and _halves_differ(c)),
}


# ----------------------------------------------------------------------------------------------------- the geometries of the GPU test
GN_GEOS = [Gn(3, 100, 320, act="silu"), Gn(5, 16, 2560, act="silu"), Gn(2, 64, 1280, 640, act="silu"),
           Gn(3, 1, 1280, 1280, act="silu"), Gn(2, 1040, 64), Gn(2, 72, 64, act="silu", pad=(6, 12)),
           Gn(2, 128, 128, 64, act="silu", pad=(16, 8)), Gn(1, 799, 512, groups=512, act="gelu"), Gn(2, 4096, 320)]
CHAIN_GEOS = [Gn(2, 256, 320), Gn(2, 1024, 320)]
LN_GEOS = [Ln(5, 40), Ln(1, 64), Ln(33, 320), Ln(100, 320), Ln(257, 640), Ln(7, 16), Ln(33, 1032), Ln(6, 2048), Ln(65539, 64)]
FP8_GEOS = [Ln(9, 320), Ln(5, 40)]
SCALES = (1.0, 4.0)
PARTITIONS = (1, 3, 8, 9, 64, 67)


def reduced(geo):
    """The same geometry with fewer rows where the rows only repeat the pattern (the CPU file's emulations and mutants)."""
    if geo.kind == "ln" and geo.rows > 300:
        return Ln(19, geo.c)
    if geo.kind == "gn" and geo.hw >= 4096:
        return Gn(1, geo.hw, geo.c1, geo.c2, geo.groups, geo.act, geo.pad)
    return geo


def partitions(sums, squares, parts, dev):
    """[frames, groups] totals -> workspace float32 [frames, parts, groups, 2] of hand-made partial sums with the same totals:
    integer multiples of the totals' unit spread by a hash, the remainder in the last part (some parts negative or zero)."""
    F, G = sums.shape
    out = torch.zeros(F, parts, G, 2, dtype=F64, device=dev)
    for i, tot in enumerate((sums, squares)):
        if parts > 1:
            h = _hash(41 + i, _ar(F, dev)[:, None, None], _ar(parts - 1, dev)[None, :, None], _ar(G, dev)[None, None, :])
            out[:, :-1, :, i] = ((h % 2001) - 1000).to(F64) * 0.25
        out[:, -1, :, i] = tot - out[:, :-1, :, i].sum(1)
    assert bool((out.to(F32).to(F64) == out).all())
    return out.to(F32)


# ----------------------------------------------------------------------------------------------------- the aggregate bounds
def _rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def _fraction(got, ref, mx, rel):
    err = (got - ref).abs()
    return (float(err.max()) / (mx * float(ref.abs().max()) + 1e-5),
            float(err.pow(2).sum().sqrt() / ref.pow(2).sum().sqrt()) / rel)


OLD_GN_SHAPES = [(4, 64, 320, "silu"), (3, 256, 64, "none"), (2, 1024, 128, "silu"), (5, 16, 2560, "silu"), (2, 4096, 320, "none")]
OLD_GN_MUTANTS = ("correct", "eps left out", "eps x 100", "variance divided by n - 1", "truncating store",
                  "rounding before the activation as well", "last pixel of every frame missing from the sums",
                  "last statistics slice counted twice", "last group normalised with its neighbour's statistics")
OLD_LN_SHAPES = [(100, 64), (257, 320), (64, 640), (33, 1280)]
OLD_LN_MUTANTS = ("correct", "eps left out", "variance divided by c - 1", "last 8-channel chunk missing from the statistics")


def old_gn_figures(frames, hw, c, act, el=torch.bfloat16):
    """One Gaussian draw of tests/test_gpu_kernels.py::test_groupnorm's recipe under its bound (2^-6 max|ref|, relL2 8e-3):
    mutant -> (max|err| / allowed, relL2 / allowed); the float64 restatement is the reference."""
    g = Gn(frames, hw, c, act=act)
    x = ((_rnd(frames, hw, c, scale=2.0).to(el) + 0.7).to(el)).to(F64)
    gamma, beta = (_rnd(c, seed=1) * 0.1 + 1).to(F64), (_rnd(c, seed=2) * 0.1).to(F64)
    ref = act64(gn_forward(g, x, gamma, beta, 1e-5, el)["arg"], act)
    return {m: _fraction(gn_forward(g, x, gamma, beta, 1e-5, el, None if m == "correct" else m, act=act)["out"], ref, 2.0 ** -6, 8e-3)
            for m in OLD_GN_MUTANTS}


def old_ln_figures(rows, c, el=torch.bfloat16):
    """The same for test_layernorm's recipe and bound (2^-7 max|ref|, relL2 6e-3)."""
    l = Ln(rows, c)
    x = ((_rnd(rows, c, scale=1.5).to(el) + 0.3).to(el)).to(F64)
    gamma, beta = (_rnd(c, seed=1) * 0.1 + 1).to(F64), (_rnd(c, seed=2) * 0.1).to(F64)
    ref = ln_forward(l, x, gamma, beta, 1e-5, el)["arg"]
    return {m: _fraction(ln_forward(l, x, gamma, beta, 1e-5, el, mut=None if m == "correct" else m)["out"], ref, 2.0 ** -7, 6e-3)
            for m in OLD_LN_MUTANTS}
