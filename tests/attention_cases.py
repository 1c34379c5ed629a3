"""Attention problems whose correct answer is known exactly, a float64 reference, and mutants of that reference.

Host only (torch on the CPU, no import of v_express_amd): tests/test_attention_cases_cpu.py shows that the cases are right and
that they tell a subtly wrong attention from a right one; tests/test_gpu_attention_exact.py feeds them to the kernels.

The aggregate bounds of the Gaussian attention tests (max|err| <= 2^-6 max|ref|, relative L2 <= 1e-2) sit ~6x above the
rounding noise of the element type; a kernel that counts ONE padded key in the softmax denominator of a ragged last key tile
stays inside them from 65 keys upwards (`old_bound_figures`).  The cases here have answers that do not depend on the
arithmetic, so one wrong key, weight or count moves at least one output bit:

  counted   q = 0: every logit is 0 and every weight 1 / n_kv in any arithmetic.  V = v0 = 1 + 2 ((kv batch + head) % 4) on every
            key but the last, which holds v0 + n_kv: the mean over exactly n_kv keys is the integer v0 + 1.  BIT-EQUAL.
            (v0 steps by 2 between neighbouring heads and kv batches so that a neighbour's key - value v0 +- 2 or v0 -+ 6 - can
            never equal the mean v0 + 1 and hide.)
  unity     Gaussian q * qs (qs = 0.25, 1), Gaussian k, V = 1: numerator and denominator see the same keys under real
            logits.  |out - 1| <= the unit in the last place below 1.0 (2^-8 bfloat16, 2^-11 float16): rounding P to the
            element type moves numerator / denominator by at most half that, which rounds to 1.0 (or, on the tie, one below).
  routing   keys are distinct +-a sign codes per (kv batch, head), query i is the code of key pi(i), V rows are random and
            distinct: the winning base-2 logit beats every other by >= 40 bits, so out == v[pi(i)] BIT FOR BIT, under the
            exact and the bounded softmax alike (all keys share one norm and q || k: the Cauchy-Schwarz shift IS the winning
            logit).  Also with prescaled keys (K d^-1/2 log2 e rounded to the element type: vx_attention scale = 0).
  tilted    none of the three above depends on the softmax SCALE (q = 0, V = 1, a 40-bit winner), so a scale taken from a
            padded head dim would pass them all.  q = (+1 .. +1); even keys = q, odd keys = q with m = round(2 sqrt(d) /
            log2 e) signs flipped: two logit levels ~4 bits apart, exact in any arithmetic; V = 1 on even and 5 on odd keys.
            |out - float64| <= one unit in the last place of the expected value: the odd keys carry < 6 % of the weight, so
            rounding their P to the element type (2^-9 relative, twice when the row sum is taken from rounded P) moves the
            output by < 0.06 * 4 * 2^-8 < 2^-10 - an eighth of the smallest unit in [1, 2) - on top of the final rounding's half.

`MUTANTS` wrap the REFERENCE (never a kernel); `emulations` are legitimate designs (P rounded before PV, another shift).
"""
import math
from collections import namedtuple
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import torch

LOG2E = 1.4426950408889634
ELEMS = (torch.bfloat16, torch.float16)
EL_NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}
SIG_BITS = {torch.bfloat16: 8, torch.float16: 11}          # significand bits, the implicit one included
KEY_TILE = 64

Geom = namedtuple("Geom", "batch heads n_q n_kv d q_per_kv")


def kv_batches(g):
    return g.batch // g.q_per_kv


def q4(t, g):
    """[batch * n_q, heads * d] -> [batch, n_q, heads, d]"""
    return t.reshape(g.batch, g.n_q, g.heads, g.d)


def k4(t, g):
    """[kv_batches * n_kv, heads * d] -> [kv_batches, n_kv, heads, d]"""
    return t.reshape(kv_batches(g), g.n_kv, g.heads, g.d)


# ----------------------------------------------------------------------------------------------------- reference
def _attend(q, kb, vb, *, scale, base2, masked=()):
    """float64 softmax(q kb^T) vb; q [batch, n_q, heads, d], kb / vb [batch, keys, heads, d] (already gathered per query
    batch).  base2: q . k IS the base-2 logit.  An empty or fully masked key set gives NaN."""
    q, kb, vb = q.double(), kb.double(), vb.double()
    if kb.shape[1] == 0:
        return torch.full(q.shape, float("nan"), dtype=torch.float64)
    s = torch.einsum("bqhd,bkhd->bhqk", q, kb)
    if not base2:
        s = s * ((q.shape[-1] ** -0.5 if scale is None else scale) * LOG2E)
    for j in masked:
        s[..., j] = -math.inf
    p = torch.exp2(s - s.amax(dim=-1, keepdim=True))
    return torch.einsum("bhqk,bkhd->bqhd", p, vb) / p.sum(dim=-1).permute(0, 2, 1)[..., None]


def _kv_of(batch, q_per_kv):
    return torch.arange(batch) // q_per_kv


def reference(q, k, v, *, scale=None, q_per_kv=1, base2=False):
    """float64 attention: q [batch, n_q, heads, d], k / v [kv_batches, n_kv, heads, d]; key batch b // q_per_kv serves query
    batch b.  scale None = d^-1/2.  base2: the keys carry scale * log2 e already (vx_attention's scale = 0)."""
    idx = _kv_of(q.shape[0], q_per_kv)
    return _attend(q, k[idx], v[idx], scale=scale, base2=base2)


def _mutant(edit):
    """edit(q, kb, vb, idx, k, v, kw) -> (kb, vb, kw) with kw = dict(scale, base2, masked)."""
    def run(q, k, v, *, scale=None, q_per_kv=1, base2=False):
        idx = _kv_of(q.shape[0], q_per_kv)
        kw = dict(scale=scale, base2=base2, masked=())
        kb, vb, kw = edit(q, k[idx], v[idx], idx, k, v, kw)
        return _attend(q, kb, vb, **kw)
    return run


def _append(kb, vb, k1, v1):
    return torch.cat([kb, k1.to(kb.dtype)], 1), torch.cat([vb, v1.to(vb.dtype)], 1)


def _m_extra_zero_key(q, kb, vb, idx, k, v, kw):
    return (*_append(kb, vb, torch.zeros_like(kb[:, :1]), torch.zeros_like(vb[:, :1])), kw)


def _m_last_key_twice(q, kb, vb, idx, k, v, kw):
    return (*_append(kb, vb, kb[:, -1:], vb[:, -1:]), kw)


def _m_last_key_dropped(q, kb, vb, idx, k, v, kw):
    return kb[:, :-1], vb[:, :-1], kw


def _m_neighbour_head_key(q, kb, vb, idx, k, v, kw):
    return (*_append(kb, vb, kb[:, :1].roll(-1, dims=2), vb[:, :1].roll(-1, dims=2)), kw)


def _m_neighbour_batch_key(q, kb, vb, idx, k, v, kw):
    nb = (idx + 1) % k.shape[0]
    return (*_append(kb, vb, k[nb][:, :1], v[nb][:, :1]), kw)


def _m_kv_batch_modulo(q, kb, vb, idx, k, v, kw):
    nb = torch.arange(q.shape[0]) % k.shape[0]
    return k[nb], v[nb], kw


def _m_scale_padded_16(q, kb, vb, idx, k, v, kw):
    d = q.shape[-1]
    if not kw["base2"]:                         # (prescaled keys: the caller applied the scale, a kernel has none to get wrong)
        kw = dict(kw, scale=(kw["scale"] or d ** -0.5) * (d / ((d + 15) // 16 * 16)) ** 0.5)
    return kb, vb, kw


def _m_tail4_masked(q, kb, vb, idx, k, v, kw):
    n = kb.shape[1]
    return kb, vb, dict(kw, masked=tuple(range(max(0, n - 4), n)))


def _m_v_is_k(q, kb, vb, idx, k, v, kw):
    return kb, kb, kw


MUTANTS = {
    # (vx_small_kv_attention: K and V are column halves of one buffer and V starts v_off columns in)
    "V read at v_off = 0: the K columns": _mutant(_m_v_is_k),
    "extra zero-logit zero-value key": _mutant(_m_extra_zero_key),
    "last key counted twice": _mutant(_m_last_key_twice),
    "last key dropped": _mutant(_m_last_key_dropped),
    "neighbour head's first key appended": _mutant(_m_neighbour_head_key),
    "neighbour kv batch's first key appended": _mutant(_m_neighbour_batch_key),
    "key batch b % kv_batches": _mutant(_m_kv_batch_modulo),
    "scale from head dim padded to 16": _mutant(_m_scale_padded_16),
    "keys n_kv-4 .. n_kv-1 masked": _mutant(_m_tail4_masked),
}


def emulate(q, k, v, el, *, scale=None, q_per_kv=1, base2=False, shift_bits=0.0, sum_rounded=False):
    """A legitimate kernel design in float64: P = 2^(s - rowmax - shift_bits) rounded to the element type before PV, the row
    sum from the unrounded P (attn_kernel, temporal) or from the rounded one (the ones row of attn2 / attn3)."""
    idx = _kv_of(q.shape[0], q_per_kv)
    qd, kb, vb = q.double(), k[idx].double(), v[idx].double()
    s = torch.einsum("bqhd,bkhd->bhqk", qd, kb)
    if not base2:
        s = s * ((q.shape[-1] ** -0.5 if scale is None else scale) * LOG2E)
    p = torch.exp2(s - s.amax(dim=-1, keepdim=True) - shift_bits)
    pr = p.to(el).double()
    den = (pr if sum_rounded else p).sum(dim=-1)
    return torch.einsum("bhqk,bkhd->bqhd", pr, vb) / den.permute(0, 2, 1)[..., None]


EMULATIONS = {
    "P rounded, row sum of unrounded P": dict(shift_bits=0.0, sum_rounded=False),
    "the same, shift 6 bits above the row maximum": dict(shift_bits=6.0, sum_rounded=False),
    "P rounded, row sum of rounded P, shift 6 bits above": dict(shift_bits=6.0, sum_rounded=True),
}


# ----------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    geom: Geom
    el: torch.dtype
    q: torch.Tensor                 # [batch * n_q, heads * d], element type
    k: torch.Tensor                 # [kv_batches * n_kv, heads * d]
    v: torch.Tensor
    expected: torch.Tensor          # [batch * n_q, heads * d], element type
    bound: str                      # "bits" | "unit" | "ulp"
    prescaled: bool = False
    pi: Optional[torch.Tensor] = None   # routing: [batch, n_q, heads] winning key

    def run(self, fn, **kw):
        """fn = reference, a mutant or emulate -> float64 [batch * n_q, heads * d]"""
        g = self.geom
        out = fn(q4(self.q, g), k4(self.k, g), k4(self.v, g), q_per_kv=g.q_per_kv, base2=self.prescaled, **kw)
        return out.reshape(g.batch * g.n_q, g.heads * g.d)

    def first_queries(self, n):
        """The same case with only the first n queries of every batch (queries are independent: a mutant caught here is
        caught by the whole case)."""
        g = self.geom
        if n >= g.n_q:
            return self
        cut = lambda t: q4(t, g)[:, :n].reshape(g.batch * n, g.heads * g.d)
        return Case(self.name, g._replace(n_q=n), self.el, cut(self.q), self.k, self.v, cut(self.expected), self.bound,
                    self.prescaled, None if self.pi is None else self.pi[:, :n])

    def allowed(self):
        """Largest |got - expected| the case accepts, per element (0 for "bits": those compare bit patterns)."""
        if self.bound == "unit":
            return torch.full(self.expected.shape, 2.0 ** -SIG_BITS[self.el], dtype=torch.float64)
        if self.bound == "ulp":
            e = self.expected.double().abs()
            return torch.exp2(torch.floor(torch.log2(e)) - (SIG_BITS[self.el] - 1))
        return torch.zeros(self.expected.shape, dtype=torch.float64)

    def wrong(self, got):
        """bool [batch * n_q, heads * d]: where `got` (element type, or float64 to be rounded to it) violates the case."""
        got = got.detach().cpu().to(self.el)
        if self.bound == "bits":
            return got.view(torch.int16) != self.expected.view(torch.int16)
        return ~((got.double() - self.expected.double()).abs() <= self.allowed())

    def deviation(self, got):
        """max |got - expected| after rounding to the element type (NaN counts as inf)."""
        dev = (got.detach().cpu().to(self.el).double() - self.expected.double()).abs()
        return float(torch.nan_to_num(dev, nan=math.inf).max())

    def first_wrong(self, got):
        """None, or a message naming the batch, head, query and column of the first wrong element."""
        got = got.detach().cpu().to(self.el)
        bad = self.wrong(got)
        if not bad.any():
            return None
        g = self.geom
        row, col = (int(x) for x in bad.nonzero()[0])
        b, i, h, c = row // g.n_q, row % g.n_q, col // g.d, col % g.d
        msg = (f"{self.name} [{EL_NAME[self.el]}] batch={g.batch} q_per_kv={g.q_per_kv} heads={g.heads} n_q={g.n_q} "
               f"n_kv={g.n_kv} d={g.d}: {int(bad.sum())} wrong elements, first at batch {b} head {h} query {i} column {c}: "
               f"got {float(got[row, col])!r}, expected {float(self.expected[row, col])!r} (bound: {self.bound})")
        if self.pi is not None:
            rows = k4(self.v, g).permute(0, 2, 1, 3).reshape(-1, g.d)                 # [(kv batch, head, key), d]
            hit = (rows.view(torch.int16) == got[row, h * g.d:(h + 1) * g.d].view(torch.int16)).all(dim=1).nonzero()
            want = f"key {int(self.pi[b, i, h])} of kv batch {b // g.q_per_kv} head {h}"
            if len(hit):
                j = int(hit[0])
                msg += (f"; the output row equals V of key {j % g.n_kv} of kv batch {j // (g.heads * g.n_kv)} head "
                        f"{j // g.n_kv % g.heads}, wanted {want}")
            else:
                msg += f"; the output row equals no key's V row, wanted {want}"
        return msg


def _seed(g, el, salt):
    s = salt
    for x in (*g, SIG_BITS[el]):
        s = (s * 1000003 + int(x)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _rows(t):
    return t.reshape(-1, t.shape[-2] * t.shape[-1]).contiguous()


def counted(g, el):
    """Who is in the row sum (module docstring)."""
    kvb, n = kv_batches(g), g.n_kv
    gen = _seed(g, el, 1)
    v0 = 1 + 2 * ((torch.arange(kvb)[:, None] + torch.arange(g.heads)[None, :]) % 4)            # [kvb, heads]
    v = v0[:, None, :, None].expand(kvb, n, g.heads, g.d).clone().double()
    v[:, -1] += n
    mean = v.sum(dim=1) / n                                                                     # float64, exact
    assert torch.equal(mean, (v0 + 1)[:, :, None].expand(kvb, g.heads, g.d).double()), "counted: the mean is not v0 + 1"
    for t in (v, mean):
        assert torch.equal(t.to(el).double(), t), f"counted: a value is not representable in {el}"
    q = torch.zeros(g.batch, g.n_q, g.heads, g.d)
    k = torch.randn(kvb, n, g.heads, g.d, generator=gen)
    exp = mean[_kv_of(g.batch, g.q_per_kv)][:, None].expand(g.batch, g.n_q, g.heads, g.d)
    return Case("counted", g, el, _rows(q).to(el), _rows(k).to(el), _rows(v).to(el), _rows(exp).to(el), "bits")


def unity(g, el, qs):
    """Numerator and denominator see the same keys under real logits (module docstring)."""
    kvb = kv_batches(g)
    gen = _seed(g, el, 2 + int(qs * 4))
    q = torch.randn(g.batch, g.n_q, g.heads, g.d, generator=gen) * qs
    k = torch.randn(kvb, g.n_kv, g.heads, g.d, generator=gen)
    v = torch.ones(kvb, g.n_kv, g.heads, g.d)
    exp = torch.ones(g.batch * g.n_q, g.heads * g.d)
    return Case(f"unity qs={qs:g}", g, el, _rows(q).to(el), _rows(k).to(el), _rows(v).to(el), exp.to(el), "unit")


def route_targets(n_kv):
    """Key 0, key n_kv - 1 and the keys on both sides of every 64-key boundary, then every other key."""
    edge = [0, n_kv - 1] + [j for t in range(KEY_TILE, n_kv, KEY_TILE) for j in (t - 1, t)]
    first = list(dict.fromkeys(j for j in edge if 0 <= j < n_kv))
    return first + [j for j in range(n_kv) if j not in first]


def routing(g, el, prescaled=False):
    """Which key, which head, which batch (module docstring)."""
    kvb, n, d = kv_batches(g), g.n_kv, g.d
    assert n <= 200 or d > 8, "routing: d = 8 has 256 codes, n_kv <= 200 there"
    gen = _seed(g, el, 7)
    if d <= 16:                                 # few codes: draw without replacement from all of them
        ids = torch.stack([torch.randperm(2 ** d, generator=gen)[:n] for _ in range(kvb * g.heads)])
        bits = (ids[..., None] >> torch.arange(d)) & 1
    else:
        bits = torch.randint(0, 2, (kvb * g.heads, n, d), generator=gen)
    code = (1.0 - 2.0 * bits.double()).reshape(kvb, g.heads, n, d).permute(0, 2, 1, 3)          # [kvb, n, heads, d] of +-1
    assert len({tuple(r.tolist()) for r in code[0, :, 0]}) == n, "routing: the codes are not distinct"
    seq = torch.tensor(route_targets(n))
    b_, i_, h_ = torch.meshgrid(torch.arange(g.batch), torch.arange(g.n_q), torch.arange(g.heads), indexing="ij")
    pi = seq[(b_ + i_ + h_) % n]                                                                # [batch, n_q, heads]
    c = d ** -0.5 * LOG2E
    chosen = None
    for e in range(6, -3, -1):                  # the largest power of two that keeps the winning base-2 logit below 2^10
        a = 2.0 ** e
        kk = (code * a * c).to(el).double() if prescaled else code * a
        win = float((a * kk.abs().amax()) * d * (1.0 if prescaled else c))
        if win < 2 ** 10:
            chosen = (a, kk)
            break
    assert chosen is not None, "routing: no power of two keeps the winning logit below 2^10"
    a, kk = chosen
    qq = (code * a)[_kv_of(g.batch, g.q_per_kv)[:, None, None], pi, h_]                        # [batch, n_q, heads, d]
    for t in (qq, kk):
        assert torch.equal(t.to(el).double(), t), f"routing: an operand is not representable in {el}"
    s = torch.einsum("bqhd,bkhd->bhqk", qq, kk[_kv_of(g.batch, g.q_per_kv)]) * (1.0 if prescaled else c)
    top = s.gather(-1, pi.permute(0, 2, 1)[..., None])                                          # [batch, heads, n_q, 1]
    others = s.scatter(-1, pi.permute(0, 2, 1)[..., None], -math.inf).amax(dim=-1, keepdim=True)
    assert float(top.max()) < 2 ** 10, f"routing: winning logit {float(top.max())} >= 2^10"
    assert n == 1 or float((top - others).min()) >= 40, f"routing: margin {float((top - others).min())} bits < 40"
    v = torch.randn(kvb, n, g.heads, d, generator=gen)
    v = (v + torch.where(v >= 0, 0.25, -0.25)).to(el)       # away from zero: 2^-40 of another row is far below half a unit of |v| >= 1/4
    assert len({tuple(r.tolist()) for r in v[0, :, 0].float()}) == n, "routing: the V rows are not distinct"
    exp = v[_kv_of(g.batch, g.q_per_kv)[:, None, None], pi, h_]
    return Case("routing prescaled" if prescaled else "routing", g, el, _rows(qq).to(el), _rows(kk).to(el), _rows(v), _rows(exp),
                "bits", prescaled=prescaled, pi=pi)


def tilted(g, el):
    """The softmax scale (module docstring)."""
    kvb, n, d = kv_batches(g), g.n_kv, g.d
    m = round(2 * d ** 0.5 / LOG2E)
    assert 0 < m < d
    q = torch.ones(g.batch, g.n_q, g.heads, d)
    k = torch.ones(kvb, n, g.heads, d)
    k[:, 1::2, :, :m] = -1.0
    v = torch.ones(kvb, n, g.heads, d)
    v[:, 1::2] = 5.0
    exp = reference(q[:, :1], k, v, q_per_kv=g.q_per_kv).expand(g.batch, g.n_q, g.heads, d)     # (every query is the same)
    return Case("tilted", g, el, _rows(q).to(el), _rows(k).to(el), _rows(v).to(el), _rows(exp).to(el), "ulp")


@lru_cache(maxsize=None)
def cases(g, el, prescaled=False):
    """The cases of one geometry: prescaled keys exist for `routing` only."""
    if prescaled:
        return (routing(g, el, prescaled=True),)
    return (counted(g, el), unity(g, el, 0.25), unity(g, el, 1.0), routing(g, el), tilted(g, el))


# ----------------------------------------------------------------------------------------------------- packings
def pack_vt(v, g, pitch, like=None):
    """[kv_batches * n_kv, heads * d] -> V^T [kv_batches, heads, d, pitch], zero beyond n_kv (what ops.alloc_vt hands out)."""
    vt = torch.zeros(kv_batches(g), g.heads, g.d, pitch, dtype=v.dtype) if like is None else like
    vt[..., :g.n_kv] = k4(v, g).permute(0, 2, 3, 1).to(vt.device)
    return vt


def temporal_rows(t, b, f, hw):
    """[(b hw) f, C] (sequence-major, the builders' layout with batch = b * hw, n = f) -> [(b f) hw, C] (the model's rows)."""
    return t.reshape(b, hw, f, -1).permute(0, 2, 1, 3).reshape(b * f * hw, -1).contiguous()


def pack_qkv(case, b, f, hw):
    """vx_temporal_attention's [(b f) hw, 3C] (Q | K | V columns) of a case built with batch = b * hw, n_q = n_kv = f."""
    g = case.geom
    assert g.batch == b * hw and g.n_q == f and g.n_kv == f and g.q_per_kv == 1
    return torch.cat([temporal_rows(t, b, f, hw) for t in (case.q, case.k, case.v)], dim=1)


def pack_kv(case):
    """vx_small_kv_attention's [batch * n_kv, 2C] (K | V columns)."""
    assert case.geom.q_per_kv == 1
    return torch.cat([case.k, case.v], dim=1)


# ----------------------------------------------------------------------------------------------------- the old bound
def old_bound_figures(g, el=torch.bfloat16):
    """(max|err| / allowed, relL2 / allowed) of the reference rounded to `el`, and of the mutant "extra zero-logit key",
    on the Gaussian problem and under the bound of the aggregate tests (max|err| <= 2^-6 max|ref| + 1e-5, relL2 <= 1e-2)."""
    gen = _seed(g, el, 11)
    kvb = kv_batches(g)
    q = torch.randn(g.batch, g.n_q, g.heads, g.d, generator=gen).to(el)
    k = torch.randn(kvb, g.n_kv, g.heads, g.d, generator=gen).to(el)
    v = torch.randn(kvb, g.n_kv, g.heads, g.d, generator=gen).to(el)
    ref = reference(q, k, v, q_per_kv=g.q_per_kv)

    def figures(out):
        err = (out.to(el).double() - ref).abs()
        return (float(err.max() / (2 ** -6 * ref.abs().max() + 1e-5)),
                float(err.pow(2).sum().sqrt() / ref.pow(2).sum().sqrt() / 1e-2))
    return figures(ref), figures(MUTANTS["extra zero-logit zero-value key"](q, k, v, q_per_kv=g.q_per_kv))


def is_noop(name, g, base2=False):
    """True where MUTANTS[name] IS the reference at this geometry (the only key counted twice, b % kv_batches with one query
    batch per key batch, a head dim that is a multiple of 16, ...), decided on a Gaussian float64 problem of three queries."""
    return _is_noop(name, g._replace(n_q=3), base2)


@lru_cache(maxsize=None)
def _is_noop(name, g, base2):
    gen = torch.Generator().manual_seed(5)
    kvb = kv_batches(g)
    q = torch.randn(g.batch, g.n_q, g.heads, g.d, generator=gen, dtype=torch.float64)
    k = torch.randn(kvb, g.n_kv, g.heads, g.d, generator=gen, dtype=torch.float64)
    v = torch.randn(kvb, g.n_kv, g.heads, g.d, generator=gen, dtype=torch.float64)
    a = reference(q, k, v, q_per_kv=g.q_per_kv, base2=base2)
    b = MUTANTS[name](q, k, v, q_per_kv=g.q_per_kv, base2=base2)
    return bool(torch.isfinite(b).all()) and float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())


# ----------------------------------------------------------------------------------------------------- shapes
# The smallest shapes at which each path can still go wrong; the key tile is 64 everywhere (n_tiles = (n_kv + 63) >> 6):
# one key, one ragged tile, a tile less one, a full tile, a tile plus one, two ragged tiles, two tiles plus one, four tiles
# with a ragged last; one query, one query block plus one, a ragged second block.
ATTN_N_KV = (1, 7, 63, 64, 65, 100, 129, 200)
ATTN_N_Q = (1, 65, 100)
ATTN_HEAD_DIMS = (8, 40, 64, 80, 160)           # 8 heads, batch 4, q_per_kv 2: TWO key batches
TEMPORAL_F = (1, 2, 15, 16, 17, 24, 31, 32)
TEMPORAL_HEAD_DIMS = (8, 40, 80, 160)           # hw = 5, b = 2, 8 heads
SMALL_KV_N_KV = (1, 5, 15, 16)
SMALL_KV_HEAD_DIMS = (8, 40, 64, 160)           # (64: its own shapes, `small_kv_geoms`)
SMALL_KV_N_Q = (7, 100)                         # batch 3


def attention_geoms(d):
    if d == 512:                                # one head, one batch: 64 KiB of K and of V^T per key tile
        return [Geom(1, 1, n_q, n_kv, 512, 1) for n_kv in (65, 100) for n_q in ATTN_N_Q]
    return [Geom(4, 8, n_q, n_kv, d, 2) for n_kv in ATTN_N_KV for n_q in ATTN_N_Q]


def temporal_geoms(d, b=2, hw=5):
    """vx_temporal_attention: b * hw sequences of f frames."""
    return [Geom(b * hw, 8, f, f, d, 1) for f in TEMPORAL_F]


def small_kv_heads(d, n_kv):
    """8 heads where the K | V tile of all heads (n_kv * 2 * heads * d elements in LDS) stays under 48 KiB, else 4."""
    return 8 if n_kv * 2 * 8 * d * 2 <= 48 * 1024 else 4


def small_kv_geoms(d):
    if d == 64:     # AudioProjection's shape: 16 heads, 61,440 and 65,536 of the 65,536 bytes of LDS the entry point admits
        return [Geom(3, 16, n_q, n_kv, 64, 1) for n_kv in (15, 16) for n_q in (5, 100)]
    return [Geom(3, small_kv_heads(d, n_kv), n_q, n_kv, d, 1) for n_kv in SMALL_KV_N_KV for n_q in SMALL_KV_N_Q]
