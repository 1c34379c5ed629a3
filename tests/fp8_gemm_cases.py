"""fp8 projection GEMM problems whose correct answer is known exactly: e4m3 bytes, scales, a float64 reference, mutants, emulations.

Host only (torch on any device, no import of v_express_amd): tests/test_fp8_gemm_cases_cpu.py shows that the cases are right and
that they tell a subtly wrong fp8 GEMM from a right one; tests/test_gpu_fp8_gemm_exact.py feeds them to vx_gemm (a_fp8 = 1) on
every route (`ROUTES`, `kernel_operands`) through tests/fp8_gemm_harness.py, which lays the operands out, judges and checks the
fills on any device - the CPU file drives it with a stand-in for the kernel at the GPU file's shapes.  The counter hash, Geo / linear, round_el, Launch and the signs / rounding / saturated builders are gemm_cases' own.

The main trick: a gemm_cases problem (A in {-1, 0, +1}, W in {-1, +1}, integer bias / rowbias, odd residual, alpha in {1, 0.5, 2})
is handed to the kernel as e4m3 bytes with power-of-two scales hashed from the LOGICAL coordinates:
    a_scale[m] = 2^ea(m), w_scale[n] = 2^ew(n), ea, ew in [-3, 3];  q[m, k] = A[m, k] 2^-ea(m),  w8[n, k] = W[n, k] 2^-ew(n)
- all normal e4m3 values; half of A's zeros are the byte 0x80 (-0), chosen by the hash; the K padding to a multiple of 128 is zero
bytes, as the producers write it.  The true product is unchanged, so the expected outputs are gemm_cases' own, compared with `==`:
they come out right only if the decode, the scale indices, the scale placement (before the bias) and the epilogue order are all
right.  Every product is +-2^j (j in [-6, 6]) and every partial sum an integer times 2^-6 below 2^24 of them: exact in float32 in
any order, with the scales applied in any order.

Cases that only fp8 has:
  products   254 x 256 x 128, one-hot: row m carries the finite byte b1(m) at position k(m), column n the finite byte b2(n) at
             every k (the 254 finite bytes, the last two columns repeat the first two); both scales 2^-1.  Expected is
             decode(b1) decode(b2) 2^-2 rounded once - an e4m3 x e4m3 product has 8 significant bits and is exact in float32
             (`product_is_exact`).  Pins the decode of every finite byte on both operands, subnormals and both zeros included, with
             no accumulation involved.  float16 leaves out the pairs whose exact scaled product is nonzero and below 2^-14 (a
             subnormal result: 1.25 % of the 254 x 256 pairs, cap 2 %); bfloat16 leaves nothing out.  The largest value is 50176.
  scales     the `signs` problem (no residual, no rowbias) with scales that are no powers of two: float32 in [0.5, 1.5) hashed
             from the row / column.  Expected is the float64 value x rounded once.  Two float32 multiplications of the exact
             integer accumulator, in any order, give a relative error <= 2^-23 of d = acc sa sw; adding the bias in float32 rounds
             once more, <= 2^-24 of the sum.  With eps = 2^-23 |d| + 2^-24 |d + bias| - inside 2^-22 relative to the output
             wherever nothing cancels - the output must lie in [round(x - eps), round(x + eps)]: EQUAL to round(x) wherever x lies
             further than eps from a rounding boundary of the element type, else one of the two neighbours (where the bias cancels
             d the interval is wider: one emulated design is 2 units off -0.00019 in float16 there, the float32 error of d ~ 8).
             The share with two candidates is a condition: the builder asserts it below 0.5 %.  (With a rowbias on top the sums
             cancel often enough for 0.61 % in float16 at K = 128: the rowbias launch runs `scales` without it.)  The one case
             that sees a scale product formed in the element type.
  chained    (`chained` supplies x, w and the expected output; fp8_gemm_harness.judge_chained compares) ops.quantize_fp8(x) and ops.fp8_weight(w) feed the GEMM at logical K in {40, 320, 640}: x and w hold
             integers in [-7, 7] with a +-7 in every row, so amax / 448 = 2^-6 exactly, every quotient is an e4m3 value and the
             output is the exact integer product rounded once.  Pins that the producers' padding and scale conventions are the GEMM's.

`MUTANTS` edit the REFERENCE (never a kernel); `EMULATIONS` are legitimate designs (float32, K tiles of 128 in another order, the
two scales multiplied in another order).
"""
from dataclasses import dataclass, field, replace

import torch

import gemm_cases as G
from gemm_cases import F64, I64, Geo, Launch, linear, round_el  # noqa: F401  (re-exported for the two test files)

ELEMS, EL_NAME = G.ELEMS, G.EL_NAME
F32 = torch.float32


def pad128(k):
    return (k + 127) // 128 * 128


# ----------------------------------------------------------------------------------------------------- e4m3
def decode_table(dev="cpu", mut=None):
    """float64 [256]: OCP e4m3 (MI300 'fn' encoding: bias 7, subnormals m / 8 * 2^-6, no infinities, 0x7F / 0xFF NaN) from the
    format's formula.  mut: one of the decode mutants."""
    b = torch.arange(256, dtype=I64, device=dev)
    s, e, m = b >> 7, (b >> 3) & 15, (b & 7).to(F64)
    bias = 8 if mut == "decode with exponent bias 8" else 7
    sub = m / 8.0 * 2.0 ** (1 - bias)
    v = torch.where(e == 0, sub, (1.0 + m / 8.0) * torch.exp2((e - bias).to(F64)))
    if mut in ("subnormals flushed on A", "subnormals flushed on W"):
        v = torch.where(e == 0, torch.zeros_like(v), v)
    v = torch.where(s == 1, -v, v)
    v[0x7F] = v[0xFF] = float("nan")
    if mut == "0x80 decoded as NaN":
        v[0x80] = float("nan")
    return v


FINITE = [b for b in range(256) if b not in (0x7F, 0xFF)]       # the 254 finite bytes


def product_is_exact():
    """Every e4m3 x e4m3 product, scaled by 2^-2, is a float32 value (8 significant bits, exponent in [-20, 16])."""
    t = decode_table()[FINITE]
    p = t[:, None] * t[None, :] * 0.25
    return bool((p.to(F32).to(F64) == p).all()), float(p.abs().max())


# ----------------------------------------------------------------------------------------------------- the cases
@dataclass
class Fp8Case:
    """kind pow2 / scales: `base` is the gemm_cases case whose integers are encoded (its geometry's K is the LOGICAL K; the bytes
    are padded to kp).  kind products: the one-hot byte table (base carries geometry and element type only)."""
    kind: str                       # pow2 | scales | products
    base: G.Case
    conditions: list = field(default_factory=list)

    @property
    def name(self):
        return {"pow2": self.base.name, "scales": "scales", "products": "products"}[self.kind]

    @property
    def geo(self):
        return self.base.geo

    @property
    def el(self):
        return self.base.el

    @property
    def kp(self):
        return pad128(self.geo.k)

    # ---- what the kernel is fed
    def exponents(self, dev):
        """(ea [m], ew [n]) int64 in [-3, 3] (pow2), 0 (scales), 1 (products: both scales 2^-1, exponent of the INVERSE)."""
        g = self.geo
        if self.kind == "pow2":
            return G._hash(11, G._ar(g.m, dev)) % 7 - 3, G._hash(12, G._ar(g.n, dev)) % 7 - 3
        z = torch.zeros((), dtype=I64, device=dev)
        return z.expand(g.m), z.expand(g.n)

    def scales(self, dev):
        """(a_scale [m], w_scale [n]) float32."""
        g = self.geo
        if self.kind == "scales":
            f = lambda salt, n: (0.5 + (G._hash(salt, G._ar(n, dev)) & 0xFFFFFF).to(F64) / 2.0 ** 24).to(F32)
            return f(14, g.m), f(15, g.n)
        if self.kind == "products":
            return torch.full((g.m,), 0.5, dtype=F32, device=dev), torch.full((g.n,), 0.5, dtype=F32, device=dev)
        ea, ew = self.exponents(dev)
        return torch.exp2(ea.to(F64)).to(F32), torch.exp2(ew.to(F64)).to(F32)

    def bytes_(self, dev):
        """(q uint8 [m, kp], w8 uint8 [n, kp]): the e4m3 bytes, K padding zero."""
        g = self.geo
        q = torch.zeros(g.m, self.kp, dtype=torch.uint8, device=dev)
        w8 = torch.zeros(g.n, self.kp, dtype=torch.uint8, device=dev)
        if self.kind == "products":
            fin = torch.tensor(FINITE, dtype=torch.uint8, device=dev)
            rows = G._ar(g.m, dev)
            q[rows, G._hash(16, rows) % g.k] = fin[rows % 254]
            w8[:, :g.k] = fin[G._ar(g.n, dev) % 254][:, None]
            return q, w8
        ea, ew = self.exponents(dev)
        rows = G._ar(g.m, dev)
        a = G.gather(g, self.base.dens, rows)                                                        # [m, K] in {-1, 0, +1}
        enc = ((a < 0).to(I64) << 7) | ((7 - ea)[:, None] << 3)
        neg0 = (G._hash(13, rows[:, None], G._ar(g.k, dev)[None, :]) & 1) << 7                       # half of the zeros: -0
        q[:, :g.k] = torch.where(a != 0, enc, neg0).to(torch.uint8)
        w = G.weight(g, dev)
        w8[:, :g.k] = (((w < 0).to(I64) << 7) | ((7 - ew)[:, None] << 3)).to(torch.uint8)
        return q, w8

    def kernel_operands(self, dev):
        """q, w8 (uint8), a_scale, w_scale, bias, rowbias (float32 or None), residual (element type or None)."""
        q, w8 = self.bytes_(dev)
        sa, sw = self.scales(dev)
        if self.kind == "products":
            return dict(q=q, w8=w8, a_scale=sa, w_scale=sw, bias=None, rowbias=None, residual=None)
        c = self.base
        rb, res = c.rowbias(dev), c.residual_t(dev)
        return dict(q=q, w8=w8, a_scale=sa, w_scale=sw, bias=c.bias(dev).to(F32), rowbias=None if rb is None else rb.to(F32),
                    residual=None if res is None else res.to(c.el))

    # ---- the reference, from the BYTES
    def dequantised(self, dev="cpu", mut=None, emu=None):
        """float64 [m, n] and the scale product used: decode(q) decode(w8)^T a_scale w_scale, with a mutant of the decode, the K
        loop or the scale indices; emu: float32 arithmetic in one of the EMULATIONS' orders."""
        if mut is None and emu is None:
            # the plain reference is a function of the bytes and the scales - of (kind, m, n, K, density) - and read-only to
            # its callers: one float64 product for all the cases of a launch that share them (gemm_cases' cache: G.clear_cache)
            g = self.geo
            key = ("fp8 dequantised", self.kind, g.m, g.n, g.k, self.base.dens, str(dev))
            if key not in G._ACC:
                G._ACC[key] = self._dequantise(dev, None, None)
            return G._ACC[key]
        return self._dequantise(dev, mut, emu)

    def _dequantise(self, dev, mut, emu):
        g = self.geo
        q, w8 = self.bytes_(dev)
        ta = decode_table(dev, mut if mut in ("subnormals flushed on A", "0x80 decoded as NaN", "decode with exponent bias 8") else None)
        tw = decode_table(dev, mut if mut in ("subnormals flushed on W", "decode with exponent bias 8") else None)
        a, w = ta[q.to(I64)], tw[w8.to(I64)]
        if mut == "upper 64 bytes of the last K tile dropped":
            a = a.clone()
            a[:, self.kp - 64:] = 0
        sa, sw = (t.to(F64) for t in self.scales(dev))
        if mut == "a_scale of the neighbouring row on the last row" and g.m >= 2:
            sa = sa.clone()
            sa[-1] = sa[-2]
        if mut == "w_scale[n - 4 .. n - 1] for the four columns before them" and g.n >= 8:
            sw = sw.clone()
            sw[-8:-4] = sw[-4:]
        if emu is None:
            s = sa[:, None] * sw[None, :]
            if mut == "scale product rounded to the element type":
                s = round_el(s, self.el)
            return (a @ w.t()) * s
        tiles = [(k0, k0 + 128) for k0 in range(0, self.kp, 128)]
        if emu == "K tiles backwards":
            tiles = tiles[::-1]
        a32, w32 = a.to(F32), w.to(F32)

        def run(ts):
            acc = torch.zeros(g.m, g.n, dtype=F32, device=dev)
            for k0, k1 in ts:
                acc = acc + a32[:, k0:k1] @ w32[:, k0:k1].t()
            return acc
        if emu == "K tiles in two halves":
            h = (len(tiles) + 1) // 2
            acc = run(tiles[:h]) + run(tiles[h:])
        else:
            acc = run(tiles)
        sa32, sw32 = sa.to(F32)[:, None], sw.to(F32)[None, :]
        if emu == "(acc * sa) * sw":
            d = (acc * sa32) * sw32
        elif emu == "(acc * sw) * sa":
            d = (acc * sw32) * sa32
        else:
            d = acc * (sa32 * sw32)
        if self.kind != "products":                          # the additions of the epilogue in float32 too
            c = self.base
            b, rb = c.bias(dev), self._rowbias_rows(dev)
            x = d + b.to(F32)[None, :]
            if rb is not None:
                x = x + rb.to(F32)
            return x.to(F64) - b[None, :] - (0 if rb is None else rb)      # (G's epilogue adds them back: exact in float64)
        return d.to(F64)

    def _rowbias_rows(self, dev, shift=0):
        g, rb = self.geo, self.base.rowbias(dev)
        if rb is None:
            return None
        grp = G._ar(g.m, dev) // g.rows_per_group
        return rb[(grp + shift) % rb.shape[0]]

    def expected(self, dev="cpu", mut=None, emu=None):
        """name -> (float64 tensor, tolerance) as gemm_cases.Case.expected; `scales` and `products` add name -> mask entries
        through `judge`.  From the BYTES: the CPU file shows that this equals gemm_cases' own expected outputs."""
        assert mut is None or mut in MUTANTS, mut
        d = self.dequantised(dev, mut, emu)
        if self.kind == "products":
            mode = {"truncating store": "trunc", "round-half-away store": "away"}.get(mut, "even")
            return {"out": (round_el(d, self.el, mode), None)}
        c = self.base
        b = c.bias(dev)[None, :]
        if mut == "bias added before the scales":
            sa, sw = (t.to(F64) for t in self.scales(dev))
            d = d + b * (sa[:, None] * sw[None, :]) - b
        elif mut == "dequantised accumulator rounded before bias and residual":
            d = round_el(d, self.el)
        elif mut == "rowbias of the neighbouring group" and self.geo.rows_per_group:
            d = d + self._rowbias_rows(dev, 1) - self._rowbias_rows(dev)
        gm = {"alpha applied to the residual": "residual added before alpha", "truncating store": "truncating store",
              "round-half-away store": "round-half-away store"}.get(mut)
        out = c.expected(dev, gm, acc=d)
        if mut == "V^T tokens t and t + 1 exchanged at a sequence's end" and "vt" in out and self.geo.seq_len >= 2:
            vt = out["vt"][0].clone()
            vt[..., -2], vt[..., -1] = out["vt"][0][..., -1], out["vt"][0][..., -2]
            out["vt"] = (vt, None)
        return out

    # ---- judging an output
    def band(self, dev="cpu"):
        """scales: (lo, hi) float64 [m, n], the element type's values of exact - eps and exact + eps, eps the float32 error bound
        of the module docstring: a right kernel's output lies in [lo, hi], and lo == hi (the output must be EQUAL to the exact
        value rounded once) wherever the exact value lies further than eps from a rounding boundary."""
        c = self.base
        d = self.dequantised(dev)
        x, _ = c.exact(dev, acc=d)
        assert not self.geo.rows_per_group
        eps = (2.0 ** -23 * d.abs() + 2.0 ** -24 * (d + c.bias(dev)[None, :]).abs()) * (1 + 2.0 ** -20)     # (second-order terms)
        return round_el(x - eps, self.el), round_el(x + eps, self.el)

    def left_out(self, dev="cpu"):
        """products, float16: bool [m, n] of the pairs whose exact scaled product is nonzero and below 2^-14."""
        d = self.dequantised(dev)
        if self.el is torch.float16:
            return (d != 0) & (d.abs() < 2.0 ** -14)
        return torch.zeros_like(d, dtype=torch.bool)

    def wrong(self, got, want, dev="cpu"):
        """name -> bool tensor of the elements that violate the case."""
        if self.kind == "pow2":
            return self.base.wrong(got, want)
        gt, w = got["out"].to(F64).to(want["out"][0].device), want["out"][0]
        if self.kind == "products":
            return {"out": (gt != w) & ~self.left_out(dev)}
        lo, hi = self.band(dev)
        return {"out": ~((gt >= lo) & (gt <= hi))}

    def first_wrong(self, got, want, dev="cpu"):
        msgs = []
        for name, b in self.wrong(got, want, dev).items():
            if bool(b.any()):
                idx = tuple(int(v) for v in b.nonzero()[0])
                msgs.append(f"{name}: {int(b.sum())} of {b.numel()} wrong, first at {idx}: got "
                            f"{float(got[name].to(F64)[idx])!r}, expected {float(want[name][0][idx])!r}")
        if not msgs:
            return None
        return f"{self.name} [{EL_NAME[self.el]}] {self.geo.text()} Kp={self.kp} alpha={self.base.alpha}: " + "; ".join(msgs)


# ---- builders
SCALES_CAP, PRODUCTS_CAP = 0.005, 0.02


def scales(g, el, dev="cpu"):
    base = G.Case("scales", g, el, G.density(g.k))
    c = Fp8Case("scales", base)
    lo, hi = c.band(dev)
    share = float((lo != hi).double().mean())
    assert share <= SCALES_CAP, f"scales {g.text()}: the band leaves out {share:.4f} of the outputs"
    c.conditions.append(f"share inside the 2^-22 band of a rounding boundary (one unit allowed): {share:.5f} (<= {SCALES_CAP})")
    return c


PRODUCTS_GEO = linear(254, 256, 128)
PRODUCTS_RING_GEO = linear(256, 320, 128)      # the persistent kernel takes whole 256 x 320 tiles only: rows and columns repeat


def products(el, dev="cpu", geo=PRODUCTS_GEO):
    c = Fp8Case("products", G.Case("products", geo, el, 1.0))
    share = float(c.left_out(dev).double().mean())
    assert share <= PRODUCTS_CAP, f"products: {share:.4f} of the pairs left out"
    c.conditions.append(f"pairs left out (nonzero, below 2^-14): {share:.4f} (<= {PRODUCTS_CAP}); max |exact| "
                        f"{float(c.dequantised(dev).abs().max()):g}")
    return c


def cases(g, el, dev="cpu"):
    """Every case of a geometry: gemm_cases' signs / rounding / saturated (with and without residual on STORE) as e4m3 bytes
    with power-of-two scales, and `scales` on STORE.  folded, statistics and GEGLU do not exist for fp8."""
    out = [Fp8Case("pow2", c) for c in G.cases(g, el, dev, skip=("folded", "statistics"))]
    if g.epi == "store":
        out.append(scales(replace(g, rows_per_group=0), el, dev))
    return out


def in_place(g, el, dev="cpu"):
    """What the out projections pass: rowbias, alpha != 1 and out aliasing the residual (`signs + residual` with a rowbias).
    rows_per_group: the launch's own, else 256 on whole 256-row tiles (the persistent kernel's condition), else the smallest
    divisor of m from 16 on (gemm_cases' rowbias table has m // rows_per_group rows: the groups must be whole)."""
    rpg = g.rows_per_group or (256 if g.m % 256 == 0 else next(d for d in range(min(16, g.m), g.m + 1) if g.m % d == 0))
    assert g.m % rpg == 0
    return Fp8Case("pow2", G.signs(replace(g, rows_per_group=rpg), el, dev, residual=True))


# ----------------------------------------------------------------------------------------------------- chained
CHAINED = [(130, 160, 40), (257, 320, 320), (129, 136, 640)]       # (m, n, logical K)


def chained(m, n, k, el, dev="cpu"):
    """(x [m, k], w [n, k] in the element type, expected float64 [m, n]): integers in [-7, 7], a +-7 in every row."""
    def ints(salt, rows):
        r, c = G._ar(rows, dev)[:, None], G._ar(k, dev)[None, :]
        v = G.small_ints(salt, 7, dev, r, c)
        pin = c == (G._hash(salt + 1, r) % k)
        return torch.where(pin, 7.0 - 14.0 * (G._hash(salt + 2, r) & 1).to(F64), v)
    x, w = ints(21, m), ints(24, n)
    return x.to(el), w.to(el), round_el(x @ w.t(), el)


# ----------------------------------------------------------------------------------------------------- mutants, emulations
# name -> whether the mutant can differ from the reference at a case (a structural fact, never read off the outputs)
def _store(c):
    return c.kind != "products" and c.geo.epi == "store"


MUTANTS = {
    "subnormals flushed on A": lambda c: c.kind == "products",
    "subnormals flushed on W": lambda c: c.kind == "products",
    "0x80 decoded as NaN": lambda c: c.kind == "products" or c.base.dens < 1.0,
    "decode with exponent bias 8": lambda c: True,
    "upper 64 bytes of the last K tile dropped": lambda c: c.kp - c.geo.k < 64,
    "a_scale of the neighbouring row on the last row": lambda c: c.kind != "products" and c.geo.m >= 2,
    "w_scale[n - 4 .. n - 1] for the four columns before them": lambda c: c.kind != "products" and c.geo.n >= 8,
    "bias added before the scales": lambda c: c.kind != "products",
    "scale product rounded to the element type": lambda c: c.kind == "scales",
    "truncating store": lambda c: c.geo.m * c.geo.n >= 64,
    "round-half-away store": lambda c: c.geo.m * c.geo.n >= 64 and c.kind != "scales",
    "dequantised accumulator rounded before bias and residual": lambda c: _store(c) and c.geo.m * c.geo.n >= 64,
    "alpha applied to the residual": lambda c: _store(c) and c.base.residual and c.base.alpha != 1.0,
    "rowbias of the neighbouring group": lambda c: _store(c) and c.geo.rows_per_group > 0 and c.geo.m > c.geo.rows_per_group,
    "V^T tokens t and t + 1 exchanged at a sequence's end": lambda c: c.geo.epi == "split" and c.geo.seq_len >= 2,
}

EMULATIONS = ("K tiles forwards", "K tiles backwards", "K tiles in two halves", "acc * (sa * sw)", "(acc * sa) * sw",
              "(acc * sw) * sa")


# ----------------------------------------------------------------------------------------------------- the old bound
def old_bound_figures(k, el=torch.bfloat16, m=128, n=320):
    """name -> (max|err| / allowed, relL2 / allowed) on test_gemm_fp8_store_and_split's own operand recipe (Gaussian a, Gaussian
    w k^-1/2, scale = row amax / 448, e4m3 round-to-nearest, bias, residual, alpha = 0.95) under its bound (max|err| <= 2^-7
    max|ref| + 1e-5, relative L2 <= 6e-3): the float64 result of the dequantised operands rounded once, and every mutant."""
    gen = torch.Generator().manual_seed(2000 + k)
    kp = pad128(k)

    def quant(t):
        sc = (t.float().abs().amax(dim=1).clamp_min(1e-30) / 448.0)
        q = torch.zeros(t.shape[0], kp, dtype=torch.uint8)
        q[:, :k] = (t.float() / sc[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
        return q, sc.double()
    q, sa = quant(torch.randn(m, k, generator=gen).to(el))
    w8, sw = quant((torch.randn(n, k, generator=gen) * k ** -0.5).to(el))
    bias = torch.randn(n, generator=gen).double()
    rowbias = torch.randn(2, n, generator=gen).double()[torch.arange(m) * 2 // m]
    res = torch.randn(m, n, generator=gen).to(el).double()
    alpha = 0.95
    good = decode_table()

    def result(mut):
        ta = decode_table("cpu", mut if mut in ("subnormals flushed on A", "0x80 decoded as NaN", "decode with exponent bias 8") else None)
        tw = decode_table("cpu", mut if mut in ("subnormals flushed on W", "decode with exponent bias 8") else None)
        a, w = ta[q.long()], tw[w8.long()]
        if mut == "upper 64 bytes of the last K tile dropped":
            a = a.clone()
            a[:, kp - 64:] = 0
        s1, s2 = sa.clone(), sw.clone()
        if mut == "a_scale of the neighbouring row on the last row":
            s1[-1] = s1[-2]
        if mut == "w_scale[n - 4 .. n - 1] for the four columns before them":
            s2[-8:-4] = s2[-4:]
        s = s1[:, None] * s2[None, :]
        if mut == "scale product rounded to the element type":
            s = round_el(s, el)
        acc = a @ w.t()
        d = (acc + bias) * s - bias if mut == "bias added before the scales" else acc * s
        if mut == "dequantised accumulator rounded before bias and residual":
            d = round_el(d, el)
        rb = rowbias.flip(0) if mut == "rowbias of the neighbouring group" else rowbias
        x = d + bias + rb
        x = alpha * (x + res) if mut == "alpha applied to the residual" else res + alpha * x
        x = round_el(x, el, {"truncating store": "trunc", "round-half-away store": "away"}.get(mut, "even"))
        if mut == "V^T tokens t and t + 1 exchanged at a sequence's end":      # (sequences of 64 tokens, as the old test has them)
            x = x.clone()
            x[63::64], x[62::64] = x[62::64].clone(), x[63::64].clone()
        return x
    ref = res + alpha * ((good[q.long()] @ good[w8.long()].t()) * (sa[:, None] * sw[None, :]) + bias + rowbias)
    tight = 0.125 if el is torch.float16 else 1.0

    def figures(out):
        err = (out - ref).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        return (float(err.max() / (2 ** -7 * tight * ref.abs().max() + 1e-5)),
                float(err.pow(2).sum().sqrt() / ref.pow(2).sum().sqrt() / (6e-3 * tight)))
    return {name: figures(result(None if name == "correct" else name)) for name in ("correct",) + tuple(MUTANTS)}


# ----------------------------------------------------------------------------------------------------- routes and shapes
def _key(tile, epi, ring=False):
    return f"{'gemm_ring_kernel' if ring else 'gemm_kernel'}<{tile},{epi},fast,fp8>"


# vx_gemm_config_name's strings (plan_of in csrc/vx_gemm.hip: an fp8 launch takes the 256 x 320 tile from 256 such tiles on with
# n % 320 == 0, else 128 x 160; vx_gemm_ring_eligible: only on ring_hint = 3 - ops.FP8_RING -, STORE, m % 256 == 0, n % 320 == 0)
K128, K256, KRING = "128x160x128,4w", "256x320x128,8w", "256x320x128,8w"
# ... and vx_last_kernel()'s of the same launch (launch_plan: gemm_kernel<BM, BN, WARPS_M, WARPS_N, STAGES, EPI, FAST, F8, LNF,
# GNS>; ring_launch: gemm_ring_kernel<EPI, RES, F8, STATS, LNF, GNS>, RES = the launch has a residual)
KERNELS = {
    _key(K128, "STORE"): "gemm_kernel<128, 160, 2, 2, 2, 0, true, true, false, false>",
    _key(K256, "STORE"): "gemm_kernel<256, 320, 4, 2, 2, 0, true, true, false, false>",
    _key(K128, "SPLIT"): "gemm_kernel<128, 160, 2, 2, 2, 2, true, true, false, false>",
    _key(K256, "SPLIT"): "gemm_kernel<256, 320, 4, 2, 2, 2, true, true, false, false>",
    _key(KRING, "STORE", ring=True): "gemm_ring_kernel<0, {res}, true, false, false, false>",
}


def kernel_of(key, residual):
    return KERNELS[key].format(res="true" if residual else "false")


def _split(s, t, c):
    return linear(s * t, 3 * c, c, epi="split", seq_len=t, heads=8)


def _routes():
    r = {}
    st = _key(K128, "STORE")
    # n = 8 and n = 136: the `n - 4` clamp of the scale / bias / residual loads (at n = 8 the lanes with lq >= 2 clamp to column
    # 4; vx_gemm refuses n % 8 != 0 for every operand type, and no fp8 producer of the model has such an n: n = 4 is a refusal
    # test of the GPU file); 328 = two tiles + 8 columns; 128 x 320 x 256: two K tiles with nothing padded, neither in rows nor
    # in columns
    r["128x160 store"] = [Launch(linear(m, n, k), st) for m, n, k in ((1, 8, 128), (127, 160, 128), (129, 136, 128), (257, 320, 384),
                                                                       (130, 1280, 1280), (300, 328, 640), (128, 320, 256))]
    # 256 tiles, the last with one row; 86 x 3 = 258 tiles
    r["256x320 store"] = [Launch(linear(65281, 320, 128), _key(K256, "STORE")), Launch(linear(256 * 86, 960, 384), _key(K256, "STORE"))]
    # gemm_cases' split shapes (sequences of 1, 4, 15, 16 and 100 tokens into V^T; K = pad128(c)) and a rows-only launch
    r["128x160 split"] = [Launch(_split(s, t, c), _key(K128, "SPLIT"))
                          for s, t, c in ((5, 1, 64), (6, 4, 64), (3, 15, 320), (4, 16, 64), (3, 100, 320), (9, 15, 64))] + \
        [Launch(linear(300, 192, 64, epi="split"), _key(K128, "SPLIT"))]
    # 87 x 3 and 86 x 3 tiles
    r["256x320 split"] = [Launch(_split(221, 100, 320), _key(K256, "SPLIT")), Launch(_split(1451, 15, 320), _key(K256, "SPLIT"))]
    ring = _key(KRING, "STORE", ring=True)
    m96 = 256 * 96
    r["ring store"] = [Launch(linear(256, 320, 128), ring)] + [Launch(linear(m96, 640, k), ring) for k in (128, 256, 384, 1280)] + \
        [Launch(linear(256 * 150, 640, 128), ring),                                           # 300 tiles: two rounds, ragged last
         Launch(linear(m96, 640, 128, rows_per_group=256 * 48), ring),
         Launch(linear(257, 320, 128), st)]                                                   # m % 256 != 0: the classic tile
    return r


ROUTES = _routes()
RING_ROUTES = ("ring store",)               # run under ops.FP8_RING[0] = True


def reduced(g):
    """gemm_cases.reduced: as few rows as keep every coordinate kind alive; n and K unchanged."""
    return G.reduced(g)
