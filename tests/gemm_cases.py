"""GEMM and implicit-convolution problems whose correct answer is known exactly, a float64 reference, mutants and emulations.

Host only (torch on any device, no import of v_express_amd): tests/test_gemm_cases_cpu.py shows that the cases are right and that
they tell a subtly wrong GEMM from a right one; tests/test_gpu_gemm_exact.py feeds them to vx_gemm on every route.

The Gaussian GEMM tests accept max|err| <= 2^-7 max|ref| and relative L2 <= 6e-3, about 3x the rounding noise: a store that
truncates, a double rounding in front of the residual, or one wrong K-term at the long-K shapes stays inside
(`old_bound_figures`; the figures are in tests/test_gemm_cases_cpu.py).  Here the operands are small integers, so every product
and every partial sum is exact in float32: the answer does not depend on summation order, tile, pipeline depth, split or route,
and the expected output is the exact value rounded ONCE to the element type.

Operands are a counter hash of their LOGICAL coordinates - A of (frame, y, x, channel), W of (group, cout, ky, kx, cin), bias of
(column), rowbias of (group, column), residual of (row, column) - never a seeded draw over the tensor's shape: a value does
not move when the shape changes, and a mis-addressed tap, channel, frame or row reads a different value.  (A plain linear is
frame 0, y = row, x = 0.)  A is in {-1, 0, +1} with density min(1, 2304 / K), W in {-1, +1}, bias and rowbias integers in
[-8, 8], the residual odd integers in [-15, 15], alpha in {1, 0.5, 2}.

Cases (every output is compared with `==`: bit-equal up to the sign of zero, unless a tolerance is stated):
  signs       acc + bias (+ rowbias), alone and as residual + alpha * (...).  Fewer than 1e-3 of the exact values reach 2^8
              (bfloat16) / 2^11 (float16): below that one +-1 term moves an output bit.
  rounding    the same with a bias offset of 1.5 * 2^8 (1.5 * 2^11) on even columns, where the integers' unit is 2 (half of
              them ties), and four times that on odd columns, where it is 8 (an eighth ties, three quarters other roundings),
              with and without the odd residual: at least a quarter of the exact values are ties between neighbouring
              representable numbers and at least a quarter need rounding without being ties (asserted from 16 rows x 128 columns on).
              Pins round-to-nearest-even and ONE rounding; `signs + residual` (alpha = 2 or 0.5) pins the order
              residual + alpha * act(acc + bias + rowbias).
  saturated   SiLU with bias +128 on even and -128 on odd 8-column blocks: x >= 32 gives x * rcp(1 + exp(-x)) == x in float32,
              x <= -32 gives |silu| < 2^-40 (out == residual; without one |out| <= 2^-40 alpha).  GEGLU with the gate bias
              +-128: gelu_f clamps |x| at 8 and returns relu(x) - 8 * 2^q(8) = x exactly from 32 on, so out = value * gate, an
              exact integer product rounded once; gate <= -32 gives |out| <= 2^-30.  Density 32 / K here, K <= 320.
  folded      LayerNorm fold with hand-made statistics: mean an integer in [-2, 2], rstd in {0.5, 1, 2}, colsum integers in
              [-2, 2]: rstd * (acc - mean * colsum) + bias is exact.
  statistics  GroupNorm partial sums (per slab, and as totals) and the two-part row sums (sum, sum of squares per half row)
              against float64 sums of the STORED values.  Density 16 / K and bias in [-4, 4] keep |out| <= 32, so every sum of
              squares stays below 2^24 and is exact in float32 in any order; with the residual alpha = 0.5 (half-integers, still
              exact).  `rounded`: bias + 2^8 + 40 on every tenth column plus the odd residual - the odd integers in [2^8, 2^9)
              are all ties, so the stored values differ from the accumulators; the sums stay exact, the sums of squares leave
              2^24 there and are held to N * 2^-24 of the sum, N the number of addends (first-order bound of any float32
              summation of non-negative terms; `_sum_tol` decides per output which of the two holds).  The other cases run on
              these launches too, their statistics under the same rule.

`MUTANTS` edit the REFERENCE (never a kernel); `EMULATIONS` are legitimate designs (float32 accumulation in another order).

ROUTES["small conv"] holds the small-channel convolutions of the keypoint guider and the VAE encoder (cin in {8, 16, 32, 96} into
n in {16, 32, 96}, cin 128 into 8, cin 256 into 320; pad 1, stride 1 and 2), where a 64-wide K tile holds several taps or parts
of two; two mutants are theirs: a straddling tile that reads its later tap from the neighbouring pixel, and a last column
without the zero fill.  The prologue's other routes (overlapping rows, GELU, the positional conv) are tests/prologue_cases.py.
"""
from dataclasses import dataclass, field, replace
from typing import Optional

import torch

ELEMS = (torch.bfloat16, torch.float16)
EL_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}          # significand bits, the implicit one included
I64, F64 = torch.int64, torch.float64
M32 = 0xFFFFFFFF


# ----------------------------------------------------------------------------------------------------- geometry
@dataclass(frozen=True)
class Geo:
    """One launch.  The image is LOGICAL: nb frames of h x w pixels with c1 (+ c2) channels; `bordered` stores it inside a zero
    border of one pixel and hands the kernel a pad-0 convolution (the resnet path), `pad` lets the kernel's gather zero-fill.
    A plain linear over m rows is Geo(nb=1, h=m, w=1)."""
    nb: int
    h: int
    w: int
    c1: int
    n: int
    c2: int = 0
    kk: int = 1                     # kernel side (1 or 3)
    stride: int = 1
    pad: int = 0
    pad_end: int = 0
    ups: int = 0
    bordered: bool = False
    window: Optional[tuple] = None  # (oy0, ox0, oh, ow): a sub-window of a pad-0 convolution's outputs (out_hw + a_pixel_offset)
    epi: str = "store"              # store | geglu | split
    groups: int = 1                 # grouped weights: w_group_rows = m // groups
    rows_per_group: int = 0         # rowbias rows
    gn_hw: int = 0                  # GroupNorm partial sums over frames of gn_hw rows, 32 groups
    stats2: bool = False            # two-part row sums (n = 640)
    seq_len: int = 0                # split: the last of the three parts goes to V^T [m / seq_len, heads, d, pitch]
    heads: int = 0
    out_f32: bool = False

    @property
    def lpad(self):                 # the convolution's logical padding
        return 1 if self.bordered else self.pad

    @property
    def cin(self):
        return self.c1 + self.c2

    @property
    def k(self):
        return self.kk * self.kk * self.cin

    @property
    def out_hw(self):
        if self.window:
            return self.window[2], self.window[3]
        he, we = self.h << self.ups, self.w << self.ups
        return ((he + 2 * self.lpad + self.pad_end - self.kk) // self.stride + 1,
                (we + 2 * self.lpad + self.pad_end - self.kk) // self.stride + 1)

    @property
    def m(self):
        return self.nb * self.out_hw[0] * self.out_hw[1]

    @property
    def n_out(self):
        return self.n // 2 if self.epi == "geglu" else self.n

    def text(self):
        s = f"{self.nb}x{self.h}x{self.w} c{self.c1}" + (f"+{self.c2}" if self.c2 else "") + f" -> {self.n}"
        if self.kk > 1 or self.ups:
            s += f" k{self.kk} s{self.stride} p{self.pad}" + (" bordered" if self.bordered else "") + (" ups" if self.ups else "")
        if self.pad_end:
            s += f" pad_end{self.pad_end}"
        if self.window:
            s += f" window{self.window}"
        for name, v in (("groups", self.groups > 1 and self.groups), ("rowbias/", self.rows_per_group), ("gn hw", self.gn_hw),
                        ("two-part row sums", self.stats2), ("seq_len", self.seq_len), ("f32 out", self.out_f32)):
            if v:
                s += f" {name}" + ("" if v is True else f" {v}")
        return s + f" [m={self.m} K={self.k} {self.epi}]"


def linear(m, n, k, **kw):
    return Geo(1, m, 1, k, n, **kw)


def density(k):
    return min(1.0, 2304.0 / k)


_ACC, _COLS = {}, {}           # caches of the exact sums / weights and of the emulations' operands


# ----------------------------------------------------------------------------------------------------- the counter hash
def _hash(salt, *coords):
    """32 well-mixed bits (int64 tensor) of a salt and integer coordinate tensors (broadcast against each other)."""
    h = None
    s = (salt * 0x9E3779B1 + 0x7F4A7C15) & M32
    for c in coords:
        c = torch.as_tensor(c)
        h = (c + s) if h is None else (h ^ (c + 0x165667B1))
        h = (h * 0x85EBCA6B) & M32
        h = h ^ (h >> 13)
        h = (h * 0xC2B2AE35) & M32
        h = h ^ (h >> 16)
    return h


def a_value(f, y, x, ch, dens):
    """A of (frame, y, x, logical channel) -> float64 in {-1, 0, +1}, nonzero with probability dens."""
    h = _hash(1, f, y, x, ch)
    nz = (h & 0xFFFF) < int(dens * 65536)
    return torch.where(nz, 1.0 - 2.0 * ((h >> 16) & 1).to(F64), torch.zeros((), dtype=F64, device=h.device))


def w_value(grp, co, ky, kx, ci):
    return 1.0 - 2.0 * ((_hash(2, grp, co, ky, kx, ci) >> 7) & 1).to(F64)


def _ar(n, dev):
    return torch.arange(n, dtype=I64, device=dev)


def small_ints(salt, lim, dev, *shape_coords):
    """float64 integers in [-lim, lim] of the coordinates."""
    return (_hash(salt, *shape_coords) % (2 * lim + 1) - lim).to(F64)


def weight(g, dev, grp=0):
    """float64 [n, K] of group grp, K ordered (ky, kx, cin) as the kernel's weight matrix (cached: `clear_cache`)."""
    key = ("w", g.n, g.kk, g.cin, grp, str(dev))
    if key not in _ACC:
        co = _ar(g.n, dev)[:, None, None, None]
        ky = _ar(g.kk, dev)[None, :, None, None]
        kx = _ar(g.kk, dev)[None, None, :, None]
        ci = _ar(g.cin, dev)[None, None, None, :]
        _ACC[key] = w_value(grp, co, ky, kx, ci).reshape(g.n, g.k)
    return _ACC[key]


def image(g, dens, dev, second=False):
    """float64 [nb, h, w, c] of the first (second) source: the logical image."""
    c0, c = (g.c1, g.c2) if second else (0, g.c1)
    return a_value(_ar(g.nb, dev)[:, None, None, None], _ar(g.h, dev)[None, :, None, None], _ar(g.w, dev)[None, None, :, None],
                   c0 + _ar(c, dev)[None, None, None, :], dens)


def out_coords(g, rows):
    oh, ow = g.out_hw
    f, r = rows // (oh * ow), rows % (oh * ow)
    oy, ox = r // ow, r % ow
    if g.window:
        oy, ox = oy + g.window[0], ox + g.window[1]
    return f, oy, ox


def centre_tap_on_last_column(g, ox):
    return (ox * g.stride - g.lpad + g.kk // 2) >> g.ups == g.w - 1


def straddling_tile(g):
    """Index of the first 64-wide K tile that holds channels of two taps (-1: none, the taps end on tile boundaries)."""
    if g.kk == 1 or g.cin % 64 == 0:
        return -1
    return next(t for t in range(-(-g.k // 64)) if (t * 64) // g.cin != (min(g.k, t * 64 + 64) - 1) // g.cin)


def right_of_last_column(g, ox):
    """Whether the output column's last tap lies one pixel right of the (upsampled) image."""
    return ox * g.stride - g.lpad + g.kk - 1 >= (g.w << g.ups)


def gather(g, dens, rows, mut=None, ks=None):
    """The im2col rows `rows` (int64 tensor) in float64 [R, K] (or the K indices `ks` of them): what the kernel's addressing
    must read, zero outside the image.  mut: one of the addressing mutants, applied where it bites among these rows."""
    dev = rows.device
    f, oy, ox = out_coords(g, rows)
    ks = _ar(g.k, dev) if ks is None else ks
    tap, ch = ks // g.cin, ks % g.cin
    uy = (oy * g.stride - g.lpad)[:, None] + (tap // g.kk)[None, :]                 # [R, K] in the (upsampled) image
    ux = (ox * g.stride - g.lpad)[:, None] + (tap % g.kk)[None, :]
    he, we = g.h << g.ups, g.w << g.ups
    valid = (uy >= 0) & (uy < he) & (ux >= 0) & (ux < we)
    lin = (f[:, None] * g.h + (uy >> g.ups)) * g.w + (ux >> g.ups)                  # pixel index, unchecked
    centre = (g.kk // 2) * g.kk + g.kk // 2
    if mut == "tap vector from the pixel to the right":
        # the centre tap's last 8 channels, at the outputs of frame 0 whose centre tap is the image's last column
        hit = (f == 0) & centre_tap_on_last_column(g, ox)
        lin = lin + (hit[:, None] & ((tap == centre) & (ch >= g.cin - 8))[None, :]).to(I64)
    elif mut == "corner tap wraps":
        hit = (f == g.nb - 1) & (oy == 0) & (ox == 0)
        valid = valid | (hit[:, None] & (tap == 0)[None, :])
    elif mut == "tap crosses into the next frame":
        oh, ow = g.out_hw
        hit = (f == 0) & (oy == oh - 1) & (ox == ow // 2)
        valid = valid | (hit[:, None] & (tap == (g.kk - 1) * g.kk + g.kk // 2)[None, :])
    elif mut == "second source first":
        ch = torch.where(ch < g.c2, ch + g.c1, ch - g.c2)
    elif mut == "straddling K tile reads its second tap one pixel to the right":
        # the first 64-wide K tile that holds two taps: the channels of its later tap(s) come from the neighbouring pixel
        k0 = straddling_tile(g) * 64
        lin = lin + ((ks >= k0) & (ks < k0 + 64) & (tap != k0 // g.cin))[None, :].to(I64)
    elif mut == "no zero fill right of the last column":
        # frame 0: the taps one pixel right of the image read what lies there in memory, the next row's first pixel
        valid = valid | ((f == 0)[:, None] & (ux == we) & (uy >= 0) & (uy < he))
    lin = lin.clamp(0, g.nb * g.h * g.w - 1)
    ff, rem = lin // (g.h * g.w), lin % (g.h * g.w)
    return a_value(ff, rem // g.w, rem % g.w, ch[None, :], dens) * valid


def clear_cache():
    _ACC.clear()
    _COLS.clear()


def accumulate(g, dens, dev, chunk=1 << 23):
    """The exact sums float64 [m, n] (grouped weights: rows of group i against W[i]); cached per (geometry, density, device)."""
    core = replace(g, epi="store", rows_per_group=0, gn_hw=0, stats2=False, seq_len=0, heads=0, out_f32=False)
    key = (core, dens, str(dev))
    if key not in _ACC:
        acc = torch.empty(g.m, g.n, dtype=F64, device=dev)
        per = g.m // g.groups
        step = max(1, chunk // g.k)
        for gi in range(g.groups):
            wt = weight(g, dev, gi).t().contiguous()
            for r0 in range(gi * per, (gi + 1) * per, step):
                r1 = min(r0 + step, (gi + 1) * per)
                acc[r0:r1] = gather(g, dens, torch.arange(r0, r1, dtype=I64, device=dev)) @ wt
        _ACC[key] = acc
    return _ACC[key]


# ----------------------------------------------------------------------------------------------------- rounding
def _ulp(x, el):
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -60)))
    return torch.exp2(e - (SIG_BITS[el] - 1))


def round_el(x, el, mode="even"):
    """float64 -> the element type's value, in float64.  even: the hardware's rounding; trunc / away: the store mutants."""
    if mode == "even":
        return x.to(torch.float32).to(el).to(F64)          # (every value here is exact in float32: ONE rounding)
    u = _ulp(x, el)
    q = x.abs() / u
    q = torch.floor(q) if mode == "trunc" else torch.floor(q + 0.5)
    return torch.sign(x) * q * u


def tie_shares(x, el):
    """(share of ties between two neighbouring representable values, share that needs rounding and is no tie)."""
    q = x.abs() / _ulp(x, el)
    fr = q - torch.floor(q)
    return float((fr == 0.5).double().mean()), float(((fr != 0) & (fr != 0.5)).double().mean())


def _sum_tol(v, dims, power):
    """Tolerance of a float32 sum of v^power over dims, any order: None (equal) where every partial sum is an integer multiple
    of the values' unit below 2^24 units - exact in float32 - else N 2^-24 sum |v|^power, N the number of addends (the
    first-order bound of any float32 summation)."""
    unit = 1.0 if bool((v == torch.round(v)).all()) else 0.5 if bool((v * 2 == torch.round(v * 2)).all()) else 0.25
    mass = (v.abs() ** power).sum(dim=dims)
    if float(mass.max()) / unit ** power < 2 ** 24:
        return None
    n = v.numel() // mass.numel()
    return n * 2.0 ** -24 * mass


# ----------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    geo: Geo
    el: torch.dtype
    dens: float
    alpha: float = 1.0
    act: str = "none"               # none | silu (STORE); GEGLU's activation is its epilogue
    residual: bool = False
    bias_lim: int = 8
    bias_extra: str = ""            # "" | rounding | saturated | stat-rounding
    folded: bool = False
    conditions: list = field(default_factory=list)        # what the builder verified, for the CPU file's printout

    def __post_init__(self):
        # the rowbias table has m // rows_per_group rows and `exact` reads row m' // rows_per_group of it: the groups must be
        # whole, or the last rows would read one past its end (an IndexError on the CPU, an aborted indexing kernel on a GPU)
        g = self.geo
        assert g.rows_per_group >= 0 and (not g.rows_per_group or g.m % g.rows_per_group == 0), \
            f"{self.name} {g.text()}: m={g.m} is no multiple of rows_per_group={g.rows_per_group}: the last rowbias group is not whole"

    # ---- operands (float64, on dev)
    def bias(self, dev):
        g, j = self.geo, _ar(self.geo.n, dev)
        b = small_ints(3, self.bias_lim, dev, j)
        if self.bias_extra == "rounding":                  # even columns: integers where the unit is 2; odd columns: where it is 8
            b = b + 1.5 * 2.0 ** SIG_BITS[self.el] * torch.where(j % 2 == 0, 1.0, 4.0).to(F64)
        elif self.bias_extra == "saturated":
            jj = j % (g.n // 2) if g.epi == "geglu" else j             # geglu: the GATE columns [n / 2, n), by their own index
            off = torch.where((jj // 8) % 2 == 0, 128.0, -128.0).to(F64)
            b = b + (off * (j >= g.n // 2) if g.epi == "geglu" else off)
        elif self.bias_extra == "stat-rounding":
            b = b + (j % 10 == 3) * (2.0 ** SIG_BITS[self.el] + 40)         # |acc + bias| <= 32: inside [2^SIG, 2^(SIG+1))
        return b

    def rowbias(self, dev):
        g = self.geo
        if not g.rows_per_group:
            return None
        return small_ints(4, 8, dev, _ar(g.m // g.rows_per_group, dev)[:, None], _ar(g.n, dev)[None, :])

    def residual_t(self, dev):
        g = self.geo
        if not self.residual:
            return None
        return 2.0 * (_hash(5, _ar(g.m, dev)[:, None], _ar(g.n_out, dev)[None, :]) % 16).to(F64) - 15.0

    def ln(self, dev):
        """(mean [m], rstd [m], colsum [n]) of the folded LayerNorm, hand-made."""
        g = self.geo
        r = _ar(g.m, dev)
        rstd = torch.tensor([0.5, 1.0, 2.0], dtype=F64, device=dev)[_hash(7, r) % 3]
        return small_ints(6, 2, dev, r), rstd, small_ints(8, 2, dev, _ar(g.n, dev))

    # ---- the reference
    def exact(self, dev="cpu", mut=None, acc=None):
        """The exact pre-rounding output float64 [m, n_out] (and, for GEGLU / SiLU, whether each element is saturated low):
        residual + alpha * act(fold(acc) + bias + rowbias).  acc: another accumulation to run the epilogue on (emulations)."""
        g = self.geo
        if acc is None:
            acc = accumulate(g, self.dens, dev)
        acc = _mutate_acc(self, acc, mut, dev)
        if self.folded:
            mean, rstd, colsum = self.ln(dev)
            acc = rstd[:, None] * (acc - mean[:, None] * colsum[None, :])
        b = self.bias(dev)
        if mut == "bias index shifted in the last column tile":
            c0 = (g.n - 1) // 160 * 160
            b = torch.cat([b[:c0], b[c0 + 1:], b[-1:]])
        x = acc + b[None, :]
        rb = self.rowbias(dev)
        if rb is not None:
            grp = _ar(g.m, dev)
            if mut == "rowbias group boundary off by one row":
                grp = (grp + 1).clamp_max(g.m - 1)
            x = x + rb[grp // g.rows_per_group]
        low = None
        if g.epi == "geglu":
            half = g.n // 2
            val, gate = x[:, :half], x[:, half:]
            if mut == "value and gate swapped in one 8-row block":
                val, gate = val.clone(), gate.clone()
                blk = slice(8, 16) if half >= 16 else slice(0, 8)
                val[:, blk], gate[:, blk] = x[:, half:][:, blk], x[:, :half][:, blk]
            sat = (gate >= 32) | (gate <= -32)
            assert mut is not None or bool(sat.all()), f"{self.name}: a GEGLU gate outside the saturated range"
            low = gate <= -32
            x = torch.where(low, torch.zeros_like(val), val * gate)
            x = torch.where(sat, x, val * torch.nn.functional.gelu(gate))          # (a mutant's unsaturated gate)
        elif self.act == "silu":
            assert bool(((x >= 32) | (x <= -32)).all()), f"{self.name}: a SiLU argument outside the saturated range"
            low = x <= -32
            x = torch.where(low, torch.zeros_like(x), x)
        res = self.residual_t(dev)
        if mut == "residual added before alpha" and res is not None:
            return self.alpha * (x + res), low
        x = self.alpha * x
        if mut == "double rounding before the residual" and res is not None:
            x = round_el(x, self.el)
        return (x if res is None else x + res), low

    def stored(self, dev="cpu", mut=None, acc=None):
        """The [m, n_out] the kernel must store, as float64 (an fp32 output is the exact value itself)."""
        x, _ = self.exact(dev, mut, acc)
        if self.geo.out_f32:
            return x
        mode = {"truncating store": "trunc", "round-half-away store": "away"}.get(mut, "even")
        return round_el(x, self.el, mode)

    def expected(self, dev="cpu", mut=None, acc=None, slab_rows=128):
        """name -> (float64 tensor, tolerance): tolerance None = equal; a tensor = |got - want| <= it, element by element."""
        g = self.geo
        st = self.stored(dev, mut, acc)
        out = {}
        tol = None
        if self.bias_extra == "saturated" and not self.residual:
            _, low = self.exact(dev, mut, acc)
            tol = low.to(F64) * (2.0 ** -30 if g.epi == "geglu" else 2.0 ** -40 * self.alpha)
        if g.epi == "split":
            pc = g.n // 3
            out["q"], out["k"] = (st[:, :pc], None), (st[:, pc:2 * pc], None)
            if g.seq_len:
                d = pc // g.heads
                vt = st[:, 2 * pc:].reshape(g.m // g.seq_len, g.seq_len, g.heads, d).permute(0, 2, 3, 1).contiguous()
                if mut == "last token dropped from V^T":
                    vt[-1, :, :, -1] = 0
                out["vt"] = (vt, None)
            else:
                out["v"] = (st[:, 2 * pc:], None)
        else:
            out["out"] = (st, tol)
        src = self.exact(dev, None, acc)[0] if mut == "statistics of the unrounded accumulators" else st
        if g.gn_hw:
            frames, cg, slab_rows = g.m // g.gn_hw, g.n // 32, min(slab_rows, g.gn_hw)
            v = st.reshape(frames, g.gn_hw // slab_rows, slab_rows, 32, cg)
            u = src.reshape(v.shape)
            out["gn sums"] = (u.sum(dim=(2, 4)), _sum_tol(v, (2, 4), 1))
            out["gn squares"] = ((u * u).sum(dim=(2, 4)), _sum_tol(v, (2, 4), 2))
            # ... and as totals per (frame, group): the slabs' float32 values added in float64
            out["gn total sums"] = (u.sum(dim=(1, 2, 4)), _sum_tol(v, (1, 2, 4), 1) if out["gn sums"][1] is not None else None)
            out["gn total squares"] = ((u * u).sum(dim=(1, 2, 4)), None if out["gn squares"][1] is None else out["gn squares"][1].sum(dim=1))
        if g.stats2:
            v, u = st.reshape(g.m, 2, g.n // 2), src.reshape(g.m, 2, g.n // 2)
            out["row sums"] = (u.sum(dim=2), _sum_tol(v, 2, 1))
            out["row squares"] = ((u * u).sum(dim=2), _sum_tol(v, 2, 2))
        return out

    # ---- judging an output
    def wrong(self, got, want):
        """got, want: name -> tensor / (tensor, tolerance) -> name -> bool tensor of the elements that violate the case."""
        bad = {}
        for name, (w, tol) in want.items():
            gt = got[name].to(F64).to(w.device)
            ok = gt == w
            if tol is not None:
                ok = ok | ((gt - w).abs() <= tol)
            bad[name] = ~ok
        return bad

    def first_wrong(self, got, want):
        """None, or a message naming the first wrong element of every output that has one."""
        msgs = []
        for name, b in self.wrong(got, want).items():
            if bool(b.any()):
                idx = tuple(int(v) for v in b.nonzero()[0])
                msgs.append(f"{name}: {int(b.sum())} of {b.numel()} wrong, first at {idx}: got "
                            f"{float(got[name].to(F64)[idx])!r}, expected {float(want[name][0][idx])!r}")
        if not msgs:
            return None
        return f"{self.name} [{EL_NAME[self.el]}] {self.geo.text()} alpha={self.alpha}: " + "; ".join(msgs)


def _band(g, dev):
    r0 = min(g.m // 2 // 16 * 16, max(0, g.m - 16))
    return torch.arange(r0, min(g.m, r0 + 16), dtype=I64, device=dev)


def _one_term(g, cols, wt, pick):
    """[R, n]: for every row the product of ONE of its nonzero K-terms with the weights - the last one, or the first at or
    after K index `pick` (rows without a nonzero term there: the last before it; all-zero rows: nothing)."""
    kidx = _ar(g.k, cols.device)[None, :].expand_as(cols)
    nz = cols != 0
    if pick is None:
        sel = torch.where(nz, kidx, torch.full_like(kidx, -1)).amax(dim=1)
    else:
        sel = torch.where(nz & (kidx >= pick), kidx, torch.full_like(kidx, g.k)).amin(dim=1)
        sel = torch.where(sel == g.k, torch.where(nz, kidx, torch.full_like(kidx, -1)).amax(dim=1), sel)
    has = sel >= 0
    sel = sel.clamp_min(0)
    return (cols.gather(1, sel[:, None]) * has[:, None]) * wt[:, sel].t()


def _mutate_acc(case, acc, mut, dev):
    """The mutants that change the sums: a few rows are re-gathered, or lose / gain one K-term."""
    g = case.geo
    if mut is None or mut not in ACC_MUTANTS:
        return acc
    acc = acc.clone()
    per = g.m // g.groups
    wt = lambda r: weight(g, dev, int(r) // per)                                   # [n, K] of the row's group
    oh, ow = g.out_hw
    if mut == "last K-term dropped in a 16-row band":          # (each row's last NONZERO term: a zero term is no defect)
        rows = _band(g, dev)
        acc[rows] -= _one_term(g, gather(g, case.dens, rows), wt(rows[0]), None)
    elif mut == "one K-term dropped for one pixel of one frame":
        rows = torch.tensor([(g.nb - 1) * oh * ow + (oh // 2) * ow + ow // 2], dtype=I64, device=dev)
        acc[rows] -= _one_term(g, gather(g, case.dens, rows), wt(rows[0]), g.k // 3)
    elif mut == "one K-term at the split boundary counted twice":
        rows = torch.arange(0, min(16, g.m), dtype=I64, device=dev)
        acc[rows] += _one_term(g, gather(g, case.dens, rows), wt(0), g.k // 64 // 2 * 64)
    elif mut == "grouped weights use group 0":
        rows = torch.arange(per, min(g.m, per + 16), dtype=I64, device=dev)
        acc[rows] = gather(g, case.dens, rows) @ weight(g, dev, 0).t()
    else:                                                                           # the addressing mutants: the rows they touch
        if mut == "tap vector from the pixel to the right":
            rows = torch.arange(0, oh * ow, dtype=I64, device=dev)
            rows = rows[centre_tap_on_last_column(g, out_coords(g, rows)[2])]
        elif mut == "corner tap wraps":
            rows = torch.tensor([(g.nb - 1) * oh * ow], dtype=I64, device=dev)
        elif mut == "tap crosses into the next frame":
            rows = torch.tensor([(oh - 1) * ow + ow // 2], dtype=I64, device=dev)
        elif mut == "no zero fill right of the last column":
            rows = torch.arange(0, oh * ow, dtype=I64, device=dev)
            rows = rows[right_of_last_column(g, out_coords(g, rows)[2])]
        elif mut == "straddling K tile reads its second tap one pixel to the right":
            rows = torch.arange(0, min(oh * ow, 64), dtype=I64, device=dev)
        else:
            rows = torch.arange(0, min(16, g.m), dtype=I64, device=dev)
        for r0 in range(0, len(rows), 256):
            rr = rows[r0:r0 + 256]
            acc[rr] = gather(g, case.dens, rr, mut) @ wt(rr[0]).t()
    return acc


ACC_MUTANTS = ("last K-term dropped in a 16-row band", "tap vector from the pixel to the right", "corner tap wraps",
               "tap crosses into the next frame", "one K-term dropped for one pixel of one frame",
               "one K-term at the split boundary counted twice", "second source first", "grouped weights use group 0",
               "straddling K tile reads its second tap one pixel to the right", "no zero fill right of the last column")

# name -> whether the mutant can differ from the reference at a geometry (a structural fact, never read off the outputs)
MUTANTS = {
    "last K-term dropped in a 16-row band": lambda g: True,
    "tap vector from the pixel to the right": lambda g: g.kk > 1 and bool(
        centre_tap_on_last_column(g, out_coords(g, torch.arange(g.out_hw[0] * g.out_hw[1]))[2]).any()),
    "corner tap wraps": lambda g: g.lpad > 0 and g.nb >= 2,
    "tap crosses into the next frame": lambda g: g.lpad > 0 and g.nb >= 2 and
    (g.out_hw[0] - 1) * g.stride - g.lpad + g.kk - 1 >= (g.h << g.ups),
    "one K-term dropped for one pixel of one frame": lambda g: True,
    "bias index shifted in the last column tile": lambda g: True,
    "rowbias group boundary off by one row": lambda g: g.rows_per_group > 0 and g.m > g.rows_per_group,
    "residual added before alpha": lambda g: g.epi == "store",
    # (the three store defects need an output that is not representable, a tie, a tie that the residual moves: from 64 outputs on)
    "truncating store": lambda g: not g.out_f32 and g.m * g.n >= 64,
    "round-half-away store": lambda g: not g.out_f32 and g.m * g.n >= 64,
    "double rounding before the residual": lambda g: g.epi == "store" and not g.out_f32 and g.m * g.n >= 64,
    "one K-term at the split boundary counted twice": lambda g: g.k >= 128,
    "second source first": lambda g: g.c2 > 0,
    "value and gate swapped in one 8-row block": lambda g: g.epi == "geglu",
    "last token dropped from V^T": lambda g: g.epi == "split" and g.seq_len > 0,
    "statistics of the unrounded accumulators": lambda g: bool(g.gn_hw or g.stats2),
    "grouped weights use group 0": lambda g: g.groups > 1,
    # the small-channel convolutions (cin % 64 != 0: a 64-wide K tile holds several taps or parts of two)
    "straddling K tile reads its second tap one pixel to the right": lambda g: straddling_tile(g) >= 0,
    # the kernel's own zero fill (pad > 0; a bordered image brings its zeros along), where a tap reaches past the last column
    "no zero fill right of the last column": lambda g: g.pad > 0 and g.h > 1 and bool(
        right_of_last_column(g, torch.arange(g.out_hw[1])).any()),
}


# ---- builders: each verifies its stated condition on the reference (on `dev`) and records it
def signs(g, el, dev="cpu", residual=False):
    alpha = 1.0 if not residual else 2.0 if g.k <= 576 else 0.5
    c = Case("signs" + (" + residual" if residual else ""), g, el, density(g.k), alpha=alpha, residual=residual)
    x, _ = c.exact(dev)
    share = float((x.abs() >= 2.0 ** SIG_BITS[el]).double().mean())
    assert share < 1e-3, f"{c.name} {g.text()}: {share:.3g} of the exact values reach 2^{SIG_BITS[el]}"
    c.conditions.append(f"share of |exact| >= 2^{SIG_BITS[el]}: {share:.2g} (< 1e-3)")
    return c


def rounding(g, el, dev="cpu", residual=False):
    c = Case("rounding" + (" + residual" if residual else ""), g, el, density(g.k), residual=residual, bias_extra="rounding")
    if g.out_f32:
        return c
    x, _ = c.exact(dev)
    ties, inexact = tie_shares(x, el)
    # expected 0.31 and 0.37.  The parity of acc is one fact per row (the number of nonzero terms) and that of the bias one per
    # column, so a share means something only over many rows AND columns: a quarter each from 16 rows x 128 columns on
    if g.m >= 16 and g.n >= 128:
        assert ties >= 0.25 and inexact >= 0.25, f"{c.name} {g.text()}: ties {ties:.3f}, other roundings {inexact:.3f}"
    elif x.numel() >= 32:
        assert ties > 0 and inexact > 0, f"{c.name} {g.text()}: ties {ties:.3f}, other roundings {inexact:.3f}"
    c.conditions.append(f"ties {ties:.3f}, other roundings {inexact:.3f} of {x.numel()} values (each >= 0.25 from 16 rows x 128 columns on)")
    return c


def saturated(g, el, dev="cpu", residual=False, folded=False):
    assert g.k <= 320, "saturated: K <= 320"
    c = Case("saturated" + (" folded" if folded else "") + (" + residual" if residual else ""), g, el, min(1.0, 32.0 / g.k),
             alpha=1.0 if g.epi == "geglu" else 2.0, act="none" if g.epi == "geglu" else "silu", residual=residual,
             bias_extra="saturated", folded=folded)
    _, low = c.exact(dev)                                  # (asserts the saturated range)
    c.conditions.append(f"every activation argument saturated, {float(low.double().mean()):.2f} of them low")
    return c


def folded(g, el, dev="cpu", residual=False):
    c = Case("folded" + (" + residual" if residual else ""), g, el, density(g.k), alpha=0.5 if residual else 1.0,
             residual=residual, folded=True)
    x, _ = c.exact(dev)
    assert bool((x * 4 == torch.round(x * 4)).all()) and float(x.abs().max()) < 2 ** 20
    c.conditions.append(f"rstd (acc - mean colsum) + bias exact, max |exact| {float(x.abs().max()):g}")
    return c


def statistics(g, el, dev="cpu", rounded=False, residual=False):
    """Plain: |out| <= 32, every sum and sum of squares exact.  + residual: alpha = 0.5 (half-integers, still exact).  rounded:
    every tenth column holds odd and even integers in [2^SIG, 2^(SIG+1)) plus the odd residual: the stored values differ
    from the accumulators, the sums stay exact, the sums of squares get the summation bound."""
    assert g.gn_hw or g.stats2
    c = Case("statistics" + (" rounded" if rounded else "") + (" + residual" if residual else ""), g, el, min(1.0, 16.0 / g.k),
             alpha=0.5 if residual and not rounded else 1.0, residual=residual or rounded, bias_lim=4,
             bias_extra="stat-rounding" if rounded else "")
    x, _ = c.exact(dev)
    top = float(x.abs().max())
    want = c.expected(dev)
    sums_exact = all(want[k][1] is None for k in want if k.endswith(" sums"))
    squares_exact = all(want[k][1] is None for k in want if k.endswith(" squares"))
    assert sums_exact, f"{c.name} {g.text()}: a sum can leave 2^24"
    if rounded:
        ties, _ = tie_shares(x, el)
        assert ties >= 0.03, f"{c.name}: ties {ties:.3f}"                             # (half of every tenth column)
        c.conditions.append(f"ties {ties:.3f}; max |exact| {top:g}: every SUM exact in float32, squares to N 2^-24")
    else:
        assert top <= 32 and squares_exact, f"{c.name} {g.text()}: |out| reaches {top}"
        c.conditions.append(f"max |out| {top:g}: every sum and sum of squares below 2^24 units, exact in float32")
    return c


def cases(g, el, dev="cpu", skip=()):
    """Every applicable case of a geometry, less those whose name starts with an entry of `skip` (a route that a case's
    operands would leave: a folded LayerNorm excludes split-K)."""
    return [c for c in _cases(g, el, dev) if not c.name.startswith(tuple(skip) or ("\0",))]


def _cases(g, el, dev):
    sat_ok = g.k <= 320 and g.groups == 1
    if g.epi == "geglu":
        return [saturated(g, el, dev)] + ([saturated(g, el, dev, folded=True)] if g.kk == 1 and g.k % 64 == 0 else [])
    if g.epi == "split":
        return [signs(g, el, dev), rounding(g, el, dev)] + ([folded(g, el, dev)] if g.k % 64 == 0 else [])
    out = [signs(g, el, dev), signs(g, el, dev, residual=True), rounding(g, el, dev), rounding(g, el, dev, residual=True)]
    if g.out_f32:
        return out[:2]
    if sat_ok:
        out += [saturated(g, el, dev), saturated(g, el, dev, residual=True)]
    if g.kk == 1 and g.k % 64 == 0 and g.c2 == 0 and not g.ups and not (g.gn_hw or g.stats2 or g.groups > 1):
        # (a folded LayerNorm excludes GroupNorm sums and row statistics on the same launch - vx_gemm_gn_slabs)
        out += [folded(g, el, dev, residual=True)]
    if g.gn_hw or g.stats2:     # (the other cases' sums are held to the summation bound where they leave 2^24)
        out += [statistics(g, el, dev), statistics(g, el, dev, residual=True), statistics(g, el, dev, rounded=True)]
    return out


# ----------------------------------------------------------------------------------------------------- what the kernel is fed
def kernel_operands(case, dev):
    """The tensors of a launch in the element type / float32, contiguous: a1 [nb, H, W, c1] as STORED (inside its zero border
    when geo.bordered), a2, w [groups * n, K] (GEGLU: value / gate rows interleaved in blocks of 8), bias, rowbias, residual,
    ln = (stats [m, 2], colsum)."""
    g, el = case.geo, case.el

    def stored(second):
        img = image(g, case.dens, dev, second)
        if g.bordered:
            big = torch.zeros(g.nb, g.h + 2, g.w + 2, img.shape[-1], dtype=F64, device=dev)
            big[:, 1:-1, 1:-1] = img
            img = big
        return img.to(el).contiguous()
    w = torch.cat([weight(g, dev, i) for i in range(g.groups)], dim=0)
    bias = case.bias(dev)
    if g.epi == "geglu":
        w, bias = interleave8(w), interleave8(bias)
    rb, res = case.rowbias(dev), case.residual_t(dev)
    ops = dict(a1=stored(False), a2=stored(True) if g.c2 else None, w=w.to(el).contiguous(), bias=bias.to(torch.float32),
               rowbias=None if rb is None else rb.to(torch.float32), residual=None if res is None else res.to(el), ln=None)
    if case.folded:
        mean, rstd, colsum = case.ln(dev)
        cs = interleave8(colsum) if g.epi == "geglu" else colsum
        ops["ln"] = (torch.stack([mean, rstd], dim=1).to(torch.float32).contiguous(), cs.to(torch.float32).contiguous())
    return ops


def interleave8(t):
    """[2 half, ...] (value rows then gate rows) -> blocks of 8 value rows followed by their 8 gate rows (the GEGLU layout)."""
    half = t.shape[0] // 2
    v = t[:half].reshape(half // 8, 8, *t.shape[1:])
    gt = t[half:].reshape(half // 8, 8, *t.shape[1:])
    return torch.stack([v, gt], dim=1).reshape(t.shape).contiguous()


# ----------------------------------------------------------------------------------------------------- emulations
def _chunks(g):
    """K index ranges of 64 (the last may be shorter), in storage order (tap-major)."""
    return [(k0, min(k0 + 64, g.k)) for k0 in range(0, g.k, 64)]


def emulate(case, order, dev="cpu"):
    """float32 accumulation of the case's sums in a legitimate order -> float64 [m, n] for Case.expected(acc=...)."""
    g = case.geo
    per = g.m // g.groups
    core = replace(g, epi="store", rows_per_group=0, gn_hw=0, stats2=False, seq_len=0, heads=0, out_f32=False)
    if (core, case.dens, order, str(dev)) in _COLS:
        return _COLS[core, case.dens, order, str(dev)]
    out = torch.empty(g.m, g.n, dtype=torch.float32, device=dev)
    for gi in range(g.groups):
        rows = torch.arange(gi * per, (gi + 1) * per, dtype=I64, device=dev)
        ck = (core, case.dens, gi, str(dev))
        if ck not in _COLS:
            _COLS[ck] = gather(g, case.dens, rows).to(torch.float32)
        a = _COLS[ck]
        wt = weight(g, dev, gi).to(torch.float32)
        ch = _chunks(g)
        if order == "64-wide chunks backwards":
            ch = ch[::-1]
        elif order == "taps innermost":                    # channel chunk outer, tap inner (the persistent kernel's walk)
            ch = [(t * g.cin + c0, t * g.cin + min(c0 + 64, g.cin)) for c0 in range(0, g.cin, 64) for t in range(g.kk * g.kk)]
        elif order.startswith("K slices"):
            s = int(order.split()[2])
            per_s = -(-len(ch) // s)
            parts = []
            for i in range(0, len(ch), per_s):
                p = torch.zeros(per, g.n, dtype=torch.float32, device=dev)
                for k0, k1 in ch[i:i + per_s]:
                    p = p + a[:, k0:k1] @ wt[:, k0:k1].t()
                parts.append(p)
            acc = parts[0]
            for p in parts[1:]:
                acc = acc + p
            out[rows] = acc
            continue
        acc = torch.zeros(per, g.n, dtype=torch.float32, device=dev)
        for k0, k1 in ch:
            acc = acc + a[:, k0:k1] @ wt[:, k0:k1].t()
        out[rows] = acc
    _COLS[core, case.dens, order, str(dev)] = out.to(F64)
    return _COLS[core, case.dens, order, str(dev)]


EMULATIONS = ("64-wide chunks forwards", "64-wide chunks backwards", "taps innermost", "taps outermost") + \
    tuple(f"K slices {s} summed afterwards" for s in range(2, 9))


# ----------------------------------------------------------------------------------------------------- the old bound
OLD_MUTANTS = ("correct", "truncating store", "round-half-away store", "double rounding before the residual",
               "last K-term dropped in a 16-row band", "one K-term dropped for one pixel of one frame",
               "one K-term at the split boundary counted twice")


def old_bound_figures(k, el=torch.bfloat16, m=512, n=320):
    """name -> (max|err| / allowed, relL2 / allowed) on ONE Gaussian problem m x n x k under the bound of the aggregate tests
    (max|err| <= 2^-7 max|ref| + 1e-5, relative L2 <= 6e-3; float16: both 8x tighter): the float64 result residual + (a w^T +
    bias) rounded to the element type, and the same with one defect."""
    gen = torch.Generator().manual_seed(1000 + k)
    a = torch.randn(m, k, generator=gen).to(el).double()
    w = (torch.randn(n, k, generator=gen) * k ** -0.5).to(el).double()
    bias = torch.randn(n, generator=gen).double()
    res = torch.randn(m, n, generator=gen).to(el).double()
    tight = 0.125 if el is torch.float16 else 1.0
    core = a @ w.t() + bias
    ref = core + res

    def figures(out):
        err = (out - ref).abs()
        return (float(err.max() / (2 ** -7 * tight * ref.abs().max() + 1e-5)),
                float(err.pow(2).sum().sqrt() / ref.pow(2).sum().sqrt() / (6e-3 * tight)))
    out = {}
    for name in OLD_MUTANTS:
        c = core.clone()
        if name == "last K-term dropped in a 16-row band":
            c[16:32] -= a[16:32, -1:] * w[None, :, -1]
        elif name == "one K-term dropped for one pixel of one frame":
            c[m - 1] -= a[m - 1, k // 3] * w[:, k // 3]    # (one term of one row, as it comes)
        elif name == "one K-term at the split boundary counted twice":
            c[:16] += a[:16, k // 2:k // 2 + 1] * w[None, :, k // 2]
        if name == "double rounding before the residual":
            x = round_el(round_el(c, el) + res, el)
        else:
            x = round_el(c + res, el, {"truncating store": "trunc", "round-half-away store": "away"}.get(name, "even"))
        out[name] = figures(x)
    return out


# ----------------------------------------------------------------------------------------------------- routes and shapes
@dataclass(frozen=True)
class Launch:
    """A geometry on a route: the name vx_gemm_config_name must give it (derived from plan_of in csrc/vx_gemm.hip,
    vx_gemm_ring_eligible and ops._ring_hint / _splitk / ring_coop_applies), under which knobs, and the cases it cannot take."""
    geo: Geo
    key: str
    frame_rows: Optional[tuple] = None      # (hw, items) of ops.frame_rows
    ring_mode: Optional[int] = None         # ops.RING_MODE
    coop_min_k: Optional[int] = None        # ops.COOP_MIN_K
    skip: tuple = ()


def _k(tile, epi="STORE", addr="fast", extra="", ring=False):
    return f"{'gemm_ring_kernel' if ring else 'gemm_kernel'}<{tile},{epi},{addr}{extra}>"


T256x32, T64, T128x160, T128, T256, TBIG = ("256x32x64,4w", "64x160x64,2w", "128x160x64,4w", "128x128x64,4w", "256x256x64,8w",
                                             "256x320x64,8w")
RING, COOP = _k(TBIG, ring=True), _k(TBIG, extra=",coop2", ring=True)


def conv(nb, h, w, c1, n, **kw):
    return Geo(nb, h, w, c1, n, **{"kk": 3, **kw})


def _routes():
    r = {}
    # n <= 32: the 256 x 32 tile; K = 8 / 72 gather (K % 64), K = 2880 FAST; one row and a tile plus one
    r["256x32"] = [Launch(linear(m, n, k), _k(T256x32, addr="fast" if k % 64 == 0 else "gather"))
                   for n in (8, 32) for m in (1, 257) for k in (8, 72, 2880)]
    # fewer than 256 tiles of 128 x 160 and FAST addressing: the 64 x 160 tile; row tails around one and two tiles
    r["64x160"] = [Launch(linear(m, 160, 64), _k(T64)) for m in (1, 63, 64, 65, 130)] + \
        [Launch(linear(m, n, k), _k(T64)) for m, n, k in ((130, 1280, 1280), (65, 1280, 64), (63, 160, 1280), (65, 136, 64))]
    # K % 64 != 0: the gathering loads, which the 64-row tile does not have; 136 = one 160-wide tile with a column tail
    r["128x160 gather"] = [Launch(linear(m, n, k), _k(T128x160, addr="gather"))
                           for m, n, k in ((127, 160, 72), (128, 320, 200), (129, 136, 72), (257, 320, 72), (257, 160, 200))]
    # 256 tiles of 128 x 160: the 64-row tile does not take over; 64 tiles of 256 x 320: neither ring nor the big tile
    r["128x160 fast"] = [Launch(linear(16384, 320, 64), _k(T128x160))]
    # widths that pad less in 128-column tiles (328 = 2 tiles + 72 columns), also into float32
    r["128x128"] = [Launch(linear(m, n, k), _k(T128, addr="fast" if k % 64 == 0 else "gather"))
                    for m, n, k in ((129, 128, 64), (300, 256, 64), (300, 328, 72), (129, 328, 128))] + \
        [Launch(linear(300, 128, 64, out_f32=True), _k(T128)), Launch(linear(129, 256, 72, out_f32=True), _k(T128, addr="gather"))]
    r["256x256"] = [Launch(linear(65536, 256, 64), _k(T256))]
    # 256 tiles of 256 x 320 off the persistent kernel (gather addressing): a pad-1 convolution and a K = 72 GEGLU
    r["256x320 classic"] = [Launch(conv(16, 64, 64, 8, 320, pad=1), _k(TBIG, addr="gather")),
                            Launch(linear(32768, 640, 72, epi="geglu"), _k(TBIG, "GEGLU", "gather"))]
    r["geglu"] = [Launch(linear(300, 128, 64, epi="geglu"), _k(T128, "GEGLU")),
                  Launch(linear(130, 640, 320, epi="geglu"), _k(T128, "GEGLU")),
                  Launch(linear(129, 160 * 2, 72, epi="geglu"), _k(T128, "GEGLU", "gather"))]
    # SPLIT: 3 x 64 columns prefer 128-wide tiles, 3 x 320 the 160-wide; sequences of 1, 4, 15, 16 and 100 tokens into V^T
    r["split"] = [Launch(linear(s * t, 3 * c, c, epi="split", seq_len=t, heads=8), _k(T128 if c == 64 else T128x160, "SPLIT"))
                  for s, t, c in ((5, 1, 64), (6, 4, 64), (3, 15, 320), (4, 16, 64), (3, 100, 320), (9, 15, 64))] + \
        [Launch(linear(300, 3 * 64, 64, epi="split"), _k(T128, "SPLIT"))]
    # convolutions on the classic tiles: nb >= 2, h != w
    g160, s64 = _k(T128x160, addr="gather"), _k(T128, addr="gather")
    r["conv"] = [Launch(conv(3, 16, 12, 64, 320, pad=1), g160),
                 Launch(conv(2, 9, 7, 64, 64, pad=1, stride=2), s64),
                 Launch(conv(2, 7, 9, 64, 160, pad=1), g160),
                 Launch(conv(2, 8, 6, 128, 160, pad=1, ups=1), g160),
                 Launch(Geo(5, 8, 16, 192, 128), _k(T128)),
                 Launch(conv(2, 8, 6, 128, 160, c2=64, pad=1), g160),
                 Launch(Geo(2, 8, 6, 128, 160, c2=64), _k(T64)),
                 Launch(conv(2, 8, 6, 64, 160, pad=1), g160),
                 Launch(conv(2, 8, 6, 64, 160, bordered=True), _k(T64)),
                 Launch(conv(2, 8, 6, 64, 64, stride=2, pad_end=1), s64),
                 Launch(conv(2, 10, 8, 64, 160, window=(1, 2, 6, 4)), _k(T64))]
    # the small-channel convolutions of the keypoint guider and the VAE encoder, 2 frames of 9 x 7, pad 1 (the gather's own zero
    # fill), stride 1 and 2: a 64-wide K tile holds eight taps (cin 8), four (16), two (32), or two thirds of one and a third
    # of the next (96: tiles 1, 2, 4, 5, ... straddle a tap boundary); n <= 32 on the 256 x 32 tile, n = 96 on 128 x 128
    g32, g128 = _k(T256x32, addr="gather"), _k(T128, addr="gather")
    r["small conv"] = [Launch(conv(2, 9, 7, cin, n, pad=1, stride=s), g32 if n <= 32 else g128)
                       for cin in (8, 16, 32, 96) for n in (16, 32, 96) for s in (1, 2)] + \
        [Launch(conv(2, 9, 7, 128, 8, pad=1, stride=s), g32) for s in (1, 2)] + \
        [Launch(conv(2, 9, 7, 256, 320, pad=1, stride=s), g160) for s in (1, 2)]
    # classic split-K: the 8x8 level from K = 2560 on (ops._splitk: 8 slices); no folded LayerNorm there
    r["split-K"] = [Launch(conv(2, 8, 8, 320, 320, bordered=True), _k(T64, extra=",splitk8"), skip=("folded",)),
                    Launch(linear(128, 320, 2560), _k(T64, extra=",splitk8"), frame_rows=(64, None), skip=("folded",)),
                    Launch(linear(128, 320, 2560, out_f32=True), _k(T128x160, extra=",splitk8"), frame_rows=(64, None),
                           skip=("folded",)),
                    # half the batch: the same operands at the same coordinates, hence the same bits
                    Launch(conv(1, 8, 8, 320, 320, bordered=True), _k(T64, extra=",splitk8"), skip=("folded",)),
                    Launch(linear(64, 320, 2560), _k(T64, extra=",splitk8"), frame_rows=(64, None), skip=("folded",))]
    # GroupNorm partial sums from the classic tiles (64-row slabs) and the two-part row sums off the persistent kernel
    r["classic statistics"] = [Launch(linear(5 * 64, 320, 64, gn_hw=64), _k(T64)),
                               Launch(linear(16384, 320, 64, gn_hw=256), _k(T128x160)),
                               Launch(linear(300, 640, 64, stats2=True), _k(T64), frame_rows=(100, 1))]
    # the persistent ring kernel: 192 tiles of 256 x 320 (ring_hint = 0) ...
    m96 = 256 * 96
    r["ring"] = [Launch(linear(m96, 640, k), RING) for k in (64, 128, 192, 320)] + \
        [Launch(linear(256 * 150, 640, 64), RING),                                          # 300 tiles: two rounds, ragged last
         Launch(linear(6144, 1280, 64), RING, frame_rows=(256, 1)),                         # ring_hint = 1 with 96 tiles
         Launch(linear(m96, 640, 192, rows_per_group=256 * 48), RING),
         Launch(linear(m96, 640, 64, groups=4), RING)]
    r["ring statistics"] = [Launch(linear(24576, 320, 64, gn_hw=1024), RING, frame_rows=(1024, 1)),      # 10 channels per group
                            Launch(linear(12288, 640, 128, gn_hw=1024), RING, frame_rows=(1024, 1)),     # 20
                            Launch(linear(6144, 1280, 64, gn_hw=256), RING, frame_rows=(256, 1)),        # 40
                            Launch(linear(m96, 640, 64, stats2=True), RING, frame_rows=(1024, 1))]
    r["ring geglu"] = [Launch(linear(m96, 640, 64, epi="geglu"), _k(TBIG, "GEGLU", ring=True)),
                       Launch(linear(256 * 48, 1280, 320, epi="geglu"), _k(TBIG, "GEGLU", ring=True))]
    r["ring conv"] = [Launch(conv(12, 32, 32, 64, 640, bordered=True, rows_per_group=6 * 1024), RING, frame_rows=(1024, 1)),
                      Launch(conv(48, 16, 16, 64, 640, bordered=True), RING, frame_rows=(256, 1)),
                      Launch(conv(192, 8, 8, 64, 640, bordered=True), RING, frame_rows=(64, 1)),
                      Launch(conv(12, 32, 32, 64, 640, c2=128, bordered=True), RING, frame_rows=(1024, 1)),
                      Launch(conv(12, 32, 32, 64, 640, bordered=True, gn_hw=1024), RING, frame_rows=(1024, 1))]
    # the cooperative two-way K split: 96 <= tiles of a nominal CFG pair < 192, K >= COOP_MIN_K (lowered to 2560)
    r["coop"] = [Launch(linear(f * 256, 1280, k), COOP, frame_rows=(256, 2 if f == 32 else 1), coop_min_k=2560, skip=("folded",))
                 for f in (15, 16, 32) for k in (2560, 5120)]
    r["coop conv"] = [Launch(conv(16, 16, 16, 1280, 1280, bordered=True, c2=c2, gn_hw=gn), COOP, frame_rows=(256, 1),
                             coop_min_k=2560) for c2, gn in ((0, 0), (1280, 0), (0, 256), (1280, 256))]
    return r


ROUTES = _routes()

# one problem through every route that accepts it (tests/test_gpu_gemm_exact.py: all outputs bit-identical)
CROSS = [Launch(linear(256 * 96, 640, 2560), RING),
         Launch(linear(256 * 96, 640, 2560), _k(T128x160), ring_mode=0),
         Launch(linear(256 * 96, 640, 2560), COOP, frame_rows=(1024, 3), coop_min_k=2560),
         Launch(linear(256 * 96, 640, 2560), _k(T128x160, extra=",splitk8"), frame_rows=(64, None))]


def reduced(g):
    """The geometry with as few rows as keep every coordinate kind alive (two frames, two rowbias / weight groups, two
    GroupNorm frames): what tests/test_gemm_cases_cpu.py can afford.  n, K and the convolution are unchanged."""
    if g.nb == 1 and g.w == 1:
        gn_hw = 128 if g.gn_hw else 0                       # (rows of a linear have no place in an image: one slab per frame)
        need = max(48 if g.rows_per_group else 40, 2 * gn_hw, g.seq_len * 3, 16 * g.groups)
        m = min(g.h, need)
        if g.seq_len:
            m = m // g.seq_len * g.seq_len
        return replace(g, h=m, rows_per_group=16 if g.rows_per_group else 0, gn_hw=gn_hw)
    nb = min(g.nb, 2)
    if g.k > 8192:                                          # the 1280-channel convolutions: 8 x 8 pixels of the frame
        g = replace(g, h=min(g.h, 8), w=min(g.w, 8))
        g = replace(g, gn_hw=g.out_hw[0] * g.out_hw[1] if g.gn_hw else 0)
    oh, ow = g.out_hw
    return replace(g, nb=nb, rows_per_group=oh * ow if g.rows_per_group else 0)
