"""Freshness of LayerNorm row statistics (TEST INFRASTRUCTURE).

blocks.py threads the (mean, rstd) of the residual stream by hand: a GEMM that writes rows of h also writes their
statistics (`stats_out=`), the next GEMM that folds a LayerNorm consumes them (`ln=(stats, colsum)`, or `stats=` of the
one-launch blocks).  A consumer trusts what it is handed; a producer that skipped `stats_out`, or rows that changed
after their producer, leave statistics that describe OTHER rows - and the whole UNet moves by less than its end-to-end
bound.  The spy recomputes, at every consumption, the statistics of the rows the consumer is about to normalise
(`fake_ops.row_stats`, float64) and compares them with what it was handed under `census.STAT_BOUNDS` - the project's own
bounds for statistics a kernel writes (mean, rstd; two-part sums), so a fresh statistic passes by construction and a
stale one misses by orders of magnitude.  Statistics written through `stats_out` are compared with the statistics of the
rows the launch stored, as tests/census.py does.

    spy = stats_spy.StatsSpy(ops)
    spy.install(monkeypatch)          # wraps gemm, geglu, gemm_split (ln=), ff_fused, tblock_fused, audio_xattn (stats=)
    ...                               # model / block code
    print(spy.report()); spy.assert_fresh()

`consumed(name, args, fakes)` / `produced(...)` are the checks themselves: tests/census.py runs them on every checked call.
"""
import inspect

import torch

import fake_ops

# entry points that consume row statistics -> (the argument holding them, the rows they describe)
LN_OPS = ("gemm", "geglu", "gemm_split")                       # ln=(stats, colsum), rows = a
STATS_OPS = ("ff_fused", "tblock_fused", "audio_xattn")        # stats=, rows = h
WRAPPED = LN_OPS + STATS_OPS


def _bounds():
    import census
    return census


def stats_ratio(stats, rows, eps=1e-5, fakes=fake_ops):
    """Worst |stats - float64 statistics of `rows`| over its `census.STAT_BOUNDS` bound ([rows, 2] mean / rstd, [rows, 4]
    two-part sums); non-finite statistics -> inf."""
    census = _bounds()
    if not torch.is_tensor(rows) or rows.dtype not in (torch.bfloat16, torch.float16):
        return None                                            # fp8 rows: no LayerNorm fold rides on them
    if stats.dim() != 2 or stats.shape[1] not in (2, 4) or stats.shape[0] != rows.reshape(-1, rows.shape[-1]).shape[0]:
        return float("inf")
    want = fakes.row_stats(rows, eps, out=torch.empty_like(stats))
    return census._stats_ratio(stats, want)[0]


def consumed(name, args, fakes=fake_ops):
    """(what, ratio) of the statistics the call `name(**args)` is about to consume, or None when it consumes none.  Call it
    BEFORE the launch: the one-launch blocks overwrite their rows."""
    if name in LN_OPS:
        ln = args.get("ln")
        if ln is None:
            return None
        r = stats_ratio(ln[0], args["a"], 1e-5, fakes)
        return None if r is None else ("ln", r)
    if name in STATS_OPS:
        st = args.get("stats")
        if st is None:
            return None
        r = stats_ratio(st, args["h"], args.get("eps", 1e-5), fakes)
        return None if r is None else ("stats", r)
    return None


def produced(name, args, result, fakes=fake_ops):
    """(what, ratio) of the statistics the finished call wrote through `stats_out`, against the rows it stored."""
    so = args.get("stats_out")
    if so is None or name not in ("gemm", "tblock_fused", "audio_xattn"):
        return None
    stored = args.get("out") if torch.is_tensor(args.get("out")) else args["h"] if name in STATS_OPS else result
    eps = args.get("stats_eps", args.get("eps", 1e-5))
    r = stats_ratio(so, stored, eps, fakes)
    return None if r is None else ("stats_out", r)


class Consumption:
    __slots__ = ("op", "kind", "what", "shape", "width", "ratio")

    def __init__(self, op, kind, what, shape, width, ratio):
        self.op, self.kind, self.what, self.shape, self.width, self.ratio = op, kind, what, shape, width, ratio

    def __repr__(self):
        return f"{self.kind} {self.op}({self.what}) rows {self.shape} stats [*, {self.width}] err/bound {self.ratio:.3g}"


class StatsSpy:
    def __init__(self, ops, fakes=fake_ops):
        self.ops, self.fakes = ops, fakes
        self.records = []

    def install(self, monkeypatch):
        for name in WRAPPED:
            monkeypatch.setattr(self.ops, name, self._wrap(name, getattr(self.ops, name)))
        return self

    def _wrap(self, name, real):
        params = inspect.signature(real)                       # (follows __wrapped__ through a census wrapper)

        def call(*a, **k):
            args = params.bind(*a, **k).arguments
            rows = args.get("a") if name in LN_OPS else args.get("h")
            hit = consumed(name, args, self.fakes)
            if hit is not None:
                st = args["ln"][0] if name in LN_OPS else args["stats"]
                self.records.append(Consumption(name, "consumed", hit[0], tuple(rows.shape), st.shape[1], hit[1]))
            out = real(*a, **k)
            hit = produced(name, args, out, self.fakes)
            if hit is not None:
                self.records.append(Consumption(name, "produced", hit[0], tuple(rows.shape), args["stats_out"].shape[1],
                                                hit[1]))
            return out
        call.__wrapped__ = real
        return call

    # ---------------------------------------------------------------------------------------------- results
    def consumptions(self, op=None):
        return [r for r in self.records if r.kind == "consumed" and (op is None or r.op == op)]

    def stale(self):
        return [r for r in self.records if not r.ratio <= 1.0]

    def worst(self):
        return max((r.ratio for r in self.records), default=0.0)

    def report(self):
        """One line per (kind, op, shape, format): how often, and the worst ratio to the bound."""
        agg = {}
        for r in self.records:
            e = agg.setdefault((r.kind, r.op, r.what, r.shape, r.width), [0, 0.0])
            e[0] += 1
            e[1] = max(e[1], r.ratio)
        lines = [f"{'kind':<9} {'op':<13} {'arg':<9} {'rows':<16} {'format':>7} {'calls':>5} {'err/bound':>9}"]
        for (kind, op, what, shape, width), (n, ratio) in sorted(agg.items(), key=lambda kv: str(kv[0])):
            lines.append(f"{kind:<9} {op:<13} {what:<9} {str(shape):<16} {'[*, %d]' % width:>7} {n:>5} {ratio:>9.3g}")
        return "\n".join(lines)

    def assert_fresh(self):
        bad = self.stale()
        assert not bad, "stale row statistics:\n" + "\n".join(map(repr, bad))
