"""Launch census (TEST INFRASTRUCTURE): every distinct kernel launch of a recorded region checked against its float64
restatement in tests/fake_ops.py, on the arguments the model really passed.

    cen = census.Census(ops)
    cen.install(monkeypatch)                     # wraps every fake_ops.ALL entry point on the `ops` module
    with cen.recording():
        cen.phase = "step 1"
        ...                                      # model code; it reaches the kernels only through ops.*
    print(cen.report())
    cen.assert_clean()

Only the outermost wrapped call is recorded (a depth counter lets e.g. upsample_conv_phases -> pad_image / gemm /
pixel_shuffle2x through as part of their caller).  The first call of each signature (op, tensor shapes / strides / dtypes,
every non-tensor argument, producer GroupNorm statistics on an input, the ambient frame_rows context, the element type)
in each phase is checked: every tensor argument is cloned (aliasing kept: one clone per storage), the restatement runs on
the clones FIRST - it may write the shared zero-bordered image of `ops.padded_buffer`, which the real kernel must write
last - then the real op runs on the original arguments and its result is returned unchanged.  The real op's return value
and the post-call value of every tensor argument are compared with the restatement's, per op, at the bound of that op's
own test in test_gpu_kernels.py (BOUNDS).  With GemmProfile / OpProfile active the kernel instantiations a call launched
are attributed to it; `coverage_errors()` then lists every instantiation the region launched that no checked call did,
every wrapped op called but never checked, and every `ops` entry point called that has no restatement.
Row statistics a checked call consumes (`ln=`, `stats=`) are compared with float64 statistics of the rows they describe
(tests/stats_spy.py, STAT_BOUNDS): a producer that skipped `stats_out` shows as a stale consumption, detail "fresh:..."."""
import inspect
from contextlib import contextmanager

import torch

import fake_ops
import stats_spy

# ---------------------------------------------------------------------------------------------------------- bounds
# (relative L2, max|err| / max|ref|) per op, each the bound of that op's existing test in test_gpu_kernels.py.  Variants:
# "+ln" a LayerNorm folded into the GEMM (test_gemm_with_folded_layernorm, ..._geglu_and_split_...), "+a2" the dual-source
# GEMM of the proj_out fold (test_ff_proj_fold_dual_source_gemm), "w_f" the per-frame folded weights
# (test_groupnorm_folded_into_linear), "loop" the float32 loop kernels (test_layout_and_loop_kernels), "layout" the bf16
# layout conversions (same test).
BOUNDS = {
    "gemm": (6e-3, 2 ** -7), "gemm+ln": (8e-3, 2 ** -6), "gemm+a2": (8e-3, 2 ** -6),
    "geglu": (6e-3, 2 ** -7), "geglu+ln": (8e-3, 2 ** -6),
    "gemm_split": (6e-3, 2 ** -7), "gemm_split+ln": (8e-3, 2 ** -6),
    "ff_fused": (8e-3, 2 ** -7), "tblock_fused": (8e-3, 2 ** -7),
    "groupnorm": (8e-3, 2 ** -6), "layernorm": (6e-3, 2 ** -7),
    "groupnorm_fold_linear": (6e-3, 2 ** -7), "groupnorm_fold_linear:w_f": (4e-3, 2 ** -8),
    "attention": (1e-2, 2 ** -6), "temporal_attention": (1e-2, 2 ** -6), "small_kv_attention": (1e-2, 2 ** -6),
    "upsample_conv_phases": (8e-3, 2 ** -6), "audio_xattn": (8e-3, 2 ** -6),
    "add_row_bias": (6e-3, 2 ** -7), "add_residual_f32": (6e-3, 2 ** -7), "wave_conv1d": (6e-3, 2 ** -7),
    "layout": (4e-3, 2 ** -8), "loop": (1e-5, 1e-5),
}
LAYOUT_OPS = {"gather_latents", "ncfhw_to_nhwc"}
LOOP_OPS = {"cfg_combine", "pack_rows", "combine_units", "overlap_ddim_step", "nhwc_to_ncfhw", "vae_postprocess"}
# (rtol, atol) of elementwise statistics: key_norm_max (test_key_norm_max); row statistics [rows, 2] = (mean, rstd)
# (test_gemm_row_stats_out: the epilogue's statistics; the separate vx_row_stats pass is tighter, test_row_stats) and
# [rows, 4] two-part sums (test_gemm_row_stats_two_parts); GroupNorm partial sums (_gn_check)
STAT_BOUNDS = {"key_norm_max": (1e-5, 1e-6), "mean": (2e-5, 2e-6), "rstd": (1e-4, 0.0), "parts": (3e-6, 2e-3),
               "gn_sums": (2e-6, 1e-3)}
# launches that add a residual: |got - ref| <= 2^-8 |ref| + 2^-7 max|ref - residual| + 1e-5 elementwise, on top of the
# op's bound (the residual dominates max|ref| on real activations).  The reference is itself rounded once to bf16, so an
# element whose exact value lies next to a rounding midpoint may land on the neighbouring bf16 value: such one-ulp
# flips are tolerated up to RES_FLIP_FRAC of the elements and reported.
RES_REL, RES_INC, RES_ABS = 2 ** -8, 2 ** -7, 1e-5
RES_FLIP_FRAC = 2 ** -10
RESIDUAL_ARG = {"gemm": "residual", "ff_fused": "h", "tblock_fused": "h", "audio_xattn": "h", "add_residual_f32": "x"}
MAIN_OUT = {"ff_fused": "h", "tblock_fused": "h", "add_row_bias": "x"}
# arguments holding row statistics (compared with STAT_BOUNDS, not as activations)
STATS_ARGS = {"stats", "stats_out", "ln"}
# wrapped entry points that compute nothing worth comparing (allocators)
NOT_COMPARED = {"alloc_vt"}
# `ops` functions that launch no kernel of their own: dispatch predicates, allocators, caches, the fp8 routing helpers
# (they call wrapped entry points, which are checked), attribute plumbing.  Any OTHER public `ops` function the model
# calls that has no fake_ops restatement is a coverage error (`coverage_errors`).
NO_KERNEL = {"block_paths", "proj_layernorm", "proj_input", "proj_weight", "pad128", "fp8_weight", "gn_of", "keep_gn",
             "stats_buffer", "clear_caches", "qk_on_ring", "ring_coop_applies", "ff_fused_applies", "tblock_fused_applies",
             "vt_pitch", "padded_buffer", "gn_fold_applies", "upsample_phases_applies", "ff_proj_fold_applies",
             "audio_xattn_applies"}


def _is_t(x):
    return isinstance(x, torch.Tensor)


def _tensors(obj, out):
    """Every tensor inside obj (nested tuples / lists), in order."""
    if _is_t(obj):
        out.append(obj)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors(v, out)
    return out


def _sig(x, ops):
    if _is_t(x):
        return ("T", tuple(x.shape), tuple(x.stride()), str(x.dtype), ops.gn_of(x) is not None)
    if isinstance(x, (list, tuple)):
        return tuple(_sig(v, ops) for v in x)
    if isinstance(x, dict):
        return tuple(sorted((k, _sig(v, ops)) for k, v in x.items()))
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if type(x).__name__ == "ConvGeom":
        return ("geom",) + tuple(sorted(vars(x).items()))
    if type(x).__name__ in ("AudioFold", "_FakeAudioFold"):
        return ("fold", x.frames, x.c, _sig(x.kq, ops))
    if type(x).__name__ == "Fp8Rows":
        return ("fp8", _sig(x.q, ops), x.k)
    return (type(x).__name__,)


def signature(name, a, k, ops):
    """What a launch is keyed by: the op, every argument (tensors by shape / strides / dtype / producer GroupNorm
    statistics), the ambient frame_rows context (it steers the kernel choice) and the element type in force."""
    return (name, _sig(a, ops), _sig(k, ops), ops._FRAME_ROWS[0], ops._ITEMS[0], str(ops.BF16))


def _clone(obj, memo):
    """Deep copy of the tensors in obj; tensors sharing a storage share the copy's storage (in-place aliasing kept)."""
    if _is_t(obj):
        st = obj.untyped_storage()
        key = (st.data_ptr(), str(obj.device))
        if key not in memo:
            memo[key] = torch.empty(0, dtype=torch.uint8, device=obj.device).set_(st).clone()
        base = memo[key]
        return torch.empty(0, dtype=obj.dtype, device=obj.device).set_(base.untyped_storage(), obj.storage_offset(),
                                                                        obj.size(), obj.stride())
    if isinstance(obj, list):
        return [_clone(v, memo) for v in obj]
    if isinstance(obj, tuple):
        return tuple(_clone(v, memo) for v in obj)
    return obj


def _ulp_bf16(x):
    """Spacing of the bf16 values around |x| (float64)."""
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


class Row:
    __slots__ = ("phase", "op", "sig", "syms", "launches", "ratio", "rel", "detail", "flips")

    def __init__(self, phase, op, sig):
        self.phase, self.op, self.sig = phase, op, sig
        self.syms, self.launches, self.ratio, self.rel, self.detail, self.flips = set(), 0, 0.0, 0.0, "", 0


class Census:
    def __init__(self, ops, fakes=fake_ops):
        self.ops, self.fakes = ops, fakes
        self.phase = "-"
        self.depth = 0
        self.active = False
        self.rows = {}                 # (phase, sig) -> Row of the checked call
        self.called = {}               # (op, sig) -> launches over the region
        self.checked_sigs = set()      # (op, sig) checked in at least one phase
        self.launched = {}             # kernel symbol -> launches
        self.checked_syms = set()
        self.unrestated = {}           # ops entry point without a restatement -> calls
        self.folds = {}                # id(real AudioFold) -> (real fold, fake fold, (op, sig) of the pack)
        self._attributed = [0, 0]      # profile records attributed to a wrapped call
        self._outside = {}             # symbol -> launches outside any wrapped call
        self.gp = self.op_prof = None

    # ------------------------------------------------------------------------------------------ installation
    def install(self, monkeypatch):
        ops = self.ops
        for name in self.fakes.ALL:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))
        for name, fn in list(vars(ops).items()):
            if name.startswith("_") or name in self.fakes.ALL or name in NO_KERNEL or not inspect.isfunction(fn) or \
                    fn.__module__ != ops.__name__:
                continue
            monkeypatch.setattr(ops, name, self._sentinel(name, fn))

    def _sentinel(self, name, real):
        def call(*a, **k):
            if self.active and self.depth == 0:
                self.unrestated[name] = self.unrestated.get(name, 0) + 1
            self.depth += 1
            try:
                return real(*a, **k)
            finally:
                self.depth -= 1
        return call

    @contextmanager
    def recording(self):
        ops = self.ops
        self.gp, self.op_prof = ops.GemmProfile(), ops.OpProfile()
        with self.gp, self.op_prof:
            self.active = True
            try:
                yield self
            finally:
                self.active = False
                self._sweep(outside=True)

    def _records(self):
        return (self.gp.records if self.gp else []), (self.op_prof.records if self.op_prof else [])

    def _sweep(self, outside=False):
        """Symbols recorded since the last sweep (outside=True: launched outside any wrapped call)."""
        g, o = self._records()
        # a GEMM launch by its configuration (tile, epilogue, addressing, split: the names of profiles/*_gemm_by_shape.txt)
        # and the kernel instantiation it ran
        syms = [f"{r[3]} = {r[5]}" for r in g[self._attributed[0]:]] + [r[5] for r in o[self._attributed[1]:]]
        self._attributed = [len(g), len(o)]
        for s in syms:
            self.launched[s] = self.launched.get(s, 0) + 1
            if outside:
                self._outside[s] = self._outside.get(s, 0) + 1
        return syms

    # ------------------------------------------------------------------------------------------ the wrapper
    def _wrap(self, name, real):
        fake = getattr(self.fakes, name)
        params = inspect.signature(fake)

        def call(*a, **k):
            if not self.active or self.depth > 0:
                return real(*a, **k)
            self._sweep(outside=True)
            sig = signature(name, a, k, self.ops)
            self.called[(name, sig)] = self.called.get((name, sig), 0) + 1
            row = self.rows.get((self.phase, sig))
            if name == "audio_xattn_pack":
                return self._pack(name, sig, real, fake, a, k)
            if row is not None or name in NOT_COMPARED:
                out = self._run(real, a, k)
                syms = self._sweep() or [name]
                if row is not None:
                    row.launches += 1
                    row.syms.update(syms)
                elif name in NOT_COMPARED:
                    self.checked_syms.update(syms)
                return out
            row = self.rows[(self.phase, sig)] = Row(self.phase, name, sig)
            row.launches = 1
            return self._check(row, name, real, fake, params, a, k)
        call.__wrapped__ = real
        return call

    def _run(self, real, a, k):
        self.depth += 1
        try:
            return real(*a, **k)
        finally:
            self.depth -= 1

    def _pack(self, name, sig, real, fake, a, k):
        # the restatement's fold from the same (cloned) inputs: checked together with its consumer (audio_xattn)
        ref = fake(*_clone(a, {}), **{kk: _clone(v, {}) for kk, v in k.items()})
        out = self._run(real, a, k)
        syms = self._sweep() or [name]
        self.folds[id(out)] = (out, ref, (name, sig), syms)
        return out

    def _check(self, row, name, real, fake, params, a, k):
        ops = self.ops
        memo = {}
        ca = _clone(list(a), memo)
        ck = {kk: _clone(v, memo) for kk, v in k.items()}
        bound_real = params.bind(*a, **k).arguments
        bound_fake = params.bind(*ca, **ck)
        fa = bound_fake.arguments
        res_name = RESIDUAL_ARG.get(name)
        residual = None
        if res_name and _is_t(bound_real.get(res_name)):
            residual = bound_real[res_name].detach().clone()
        # per-op adapters of the restatement's inputs
        if name == "groupnorm_fold_linear":
            fa["ws"] = _gn_mean_var(fa["ws"], fa["frames"], fa["hw"], fa["groups"], fa["w"].shape[1])
        if name == "audio_xattn":
            hit = self.folds.get(id(bound_real["fold"]))
            if hit is None:
                raise AssertionError("audio_xattn: its fold was not packed inside the recorded region")
            fa["fold"] = hit[1]
            self.checked_sigs.add(hit[2])
            self.checked_syms.update(hit[3])
        # row statistics the launch is about to consume: they must describe the rows it normalises AS THEY ARE NOW
        # (tests/stats_spy.py; the restatement below applies whatever statistics it is handed)
        fresh = stats_spy.consumed(name, bound_real, self.fakes)
        ref = fake(*bound_fake.args, **bound_fake.kwargs)
        ref = _clone(ref, {}) if not isinstance(ref, tuple) else tuple(_clone(r, {}) for r in ref)
        got = self._run(real, a, k)
        syms = self._sweep() or [name]
        row.syms.update(syms)
        self.checked_syms.update(syms)
        self.checked_sigs.add((name, row.sig))
        # ---- comparisons
        results = [] if fresh is None else [("fresh:" + fresh[0], (fresh[1], 0.0, 0))]
        arg_out = "out" if _is_t(bound_real.get("out")) else MAIN_OUT.get(name) if name in MAIN_OUT else \
            "h" if name == "audio_xattn" else None
        key = name + ("+ln" if bound_real.get("ln") is not None and name in ("gemm", "geglu", "gemm_split") else "") + \
            ("+a2" if name == "gemm" and bound_real.get("a2") is not None else "")
        key = "layout" if name in LAYOUT_OPS else "loop" if name in LOOP_OPS else key
        if name == "groupnorm_stats":
            results.append(("sums", _stat_ratio(_gn_sums(got[0], fa["frames"], fa["groups"]),
                                                _gn_sums(ref[0], fa["frames"], fa["groups"], fa["hw"],
                                                         fa["x1"].shape[-1] + (0 if fa.get("x2") is None else
                                                                               fa["x2"].shape[-1])),
                                                STAT_BOUNDS["gn_sums"])))
        elif name == "groupnorm_fold_linear":
            # the per-frame weights against the UNROUNDED product w * gamma * rstd, as test_groupnorm_folded_into_linear
            # states their bound (one rounding: against the restatement's own rounding a one-ulp flip could exceed it)
            c = fa["w"].shape[1]
            rstd = torch.rsqrt(fa["ws"][..., 1] + fa["eps"]).repeat_interleave(c // fa["groups"], dim=1)
            exact = fa["w"].double()[None] * (fa["gamma"].double()[None] * rstd)[:, None, :]
            results.append(("w_f", _ratio(got[0], exact, BOUNDS["groupnorm_fold_linear:w_f"])))
            results.append(("b_f", _ratio(got[1], ref[1], BOUNDS[name])))
        elif name == "row_stats" and not any(got is t for t in _tensors(list(bound_real.values()), [])):
            results.append(("stats", _stats_ratio(got, ref)))
        elif name == "key_norm_max":
            results.append(("kmax", _stat_ratio(got, ref, STAT_BOUNDS["key_norm_max"])))
        elif _is_t(got) and not any(got is t for t in _tensors(list(bound_real.values()), [])):
            results.append(("out", self._cmp(name, key, got, ref, residual)))
        written = _tensors(bound_real.get("stats_out"), [])
        for arg, val in bound_real.items():
            if arg == "fold" or (name == "groupnorm_fold_linear" and arg == "ws"):
                continue
            rt, ft = _tensors(val, []), _tensors(fa[arg] if arg in fa else val, [])
            for i, (r_, f_) in enumerate(zip(rt, ft)):
                what = arg if len(rt) == 1 else f"{arg}[{i}]"
                if written and arg in ("stats", "stats_out") and r_.data_ptr() == written[0].data_ptr():
                    # statistics the launch wrote: against float64 statistics of the rows it STORED (the restatement's
                    # rows may sit one bf16 rounding away), as test_gemm_row_stats_out checks them
                    stored = got if arg_out is None else bound_real[arg_out]
                    eps = bound_real.get("stats_eps", bound_real.get("eps", 1e-5))
                    want = self.fakes.row_stats(stored, eps, out=torch.empty_like(r_))
                    results.append((what, _stats_ratio(r_, want)))
                elif arg in STATS_ARGS or (name == "row_stats" and arg == "out"):
                    results.append((what, _stats_ratio(r_, f_)))
                elif r_.dtype == torch.int32 or r_.dtype == torch.int64:
                    results.append((what, (0.0 if torch.equal(r_, f_) else float("inf"), 0.0, 0)))
                else:
                    main = arg == MAIN_OUT.get(name, "out") or (name == "audio_xattn" and arg == "h")
                    results.append((what, self._cmp(name, key, r_, f_, residual if main else None)))
        # GroupNorm partial sums the GEMM attached to its output: against float64 sums of the STORED output
        if name == "gemm" and bound_real.get("gn") is not None and _is_t(got) and ops.gn_of(got) is not None:
            st = ops.gn_of(got)
            x = got.double().view(st.frames, st.hw, st.groups, -1)
            want = torch.stack([x.sum(dim=(1, 3)), (x * x).sum(dim=(1, 3))], dim=-1)
            results.append(("gn_ws", _stat_ratio(_gn_sums(st.ws, st.frames, st.groups, st.hw, st.c), want,
                                                 STAT_BOUNDS["gn_sums"])))
        worst = max(results, key=lambda r: r[1][0]) if results else ("-", (0.0, 0.0, 0))
        row.ratio, row.rel, row.flips = worst[1][0], worst[1][1], sum(r[1][2] for r in results)
        row.detail = worst[0]
        return got

    def _cmp(self, name, key, got, ref, residual):
        # (an op without an activation bound of its own: its inputs, which must come out unchanged, at the GEMM bound)
        rel, mx = BOUNDS.get(key, BOUNDS["gemm"])
        if got.dtype in (torch.uint8,):
            return (0.0 if torch.equal(got, ref) else float("inf"), 0.0, 0)
        r = _ratio(got, ref, (rel, mx))
        if residual is None:
            return r
        g, f = got.double(), ref.double()
        inc = (f - residual.double().reshape(f.shape)).abs().max().item()
        d = (g - f).abs()
        lim = RES_REL * f.abs() + RES_INC * inc + RES_ABS
        over = d > lim
        flips = 0
        if over.any():
            flip = over & (d <= _ulp_bf16(f) * 1.0001)
            flips = int(flip.sum().item())
            hard = over & ~flip
            ratio_e = (d[hard] / lim[hard]).max().item() if hard.any() else 1.0
            if flips > RES_FLIP_FRAC * d.numel():
                ratio_e = max(ratio_e, flips / (RES_FLIP_FRAC * d.numel()))
        else:
            ratio_e = (d / lim).max().item()
        return (max(r[0], ratio_e), r[1], flips)

    # ------------------------------------------------------------------------------------------ results
    def coverage_errors(self):
        errs = []
        for s, n in sorted(self._outside.items()):
            errs.append(f"kernel {s} launched {n}x outside any wrapped ops entry point")
        for s in sorted(set(self.launched) - self.checked_syms):
            errs.append(f"kernel {s} launched {self.launched[s]}x but never by a checked call")
        for (op, sig), n in sorted(self.called.items(), key=lambda kv: kv[0][0]):
            if op not in NOT_COMPARED and (op, sig) not in self.checked_sigs:
                errs.append(f"ops.{op} called {n}x with a signature never checked: {sig}")
        for op, n in sorted(self.unrestated.items()):
            errs.append(f"ops.{op} called {n}x: no fake_ops restatement (add one to tests/fake_ops.py)")
        return errs

    def failures(self):
        return [r for r in self.rows.values() if not r.ratio <= 1.0]

    def symbols(self):
        return set(self.launched)

    def report(self):
        lines = [f"{'phase':<14} {'op':<22} {'launches':>8} {'err/bound':>9} {'relL2':>9} {'flips':>6}  worst  kernel(s) / shapes"]
        for r in sorted(self.rows.values(), key=lambda r: (r.phase, r.op, -r.ratio)):
            shapes = [t[1] for t in _flat_sig(r.sig[1]) if isinstance(t, tuple) and t and t[0] == "T"][:3]
            lines.append(f"{r.phase:<14} {r.op:<22} {r.launches:>8} {r.ratio:>9.3g} {r.rel:>9.3g} {r.flips:>6}  "
                         f"{r.detail:<6} {', '.join(sorted(r.syms))[:150]}  {shapes}")
        fam = {}
        for r in self.rows.values():
            f = fam.setdefault(r.op, [0, 0, 0.0])
            f[0] += 1
            f[1] += r.launches
            f[2] = max(f[2], r.ratio)
        lines.append("per op: " + "; ".join(f"{op} {v[0]} sig / {v[1]} launches, worst {v[2]:.3g}"
                                             for op, v in sorted(fam.items())))
        lines.append(f"{len(self.rows)} checked signatures, {sum(self.launched.values())} kernel launches of "
                     f"{len(self.launched)} instantiations")
        return "\n".join(lines)

    def assert_clean(self):
        bad = self.failures()
        cov = self.coverage_errors()
        msg = "\n".join([f"over bound: {r.phase} {r.op} err/bound={r.ratio:.3g} ({r.detail}) {r.sig}" for r in bad] + cov)
        assert not bad and not cov, msg


def _flat_sig(s):
    out = []
    if isinstance(s, tuple) and s and s[0] == "T":
        return [s]
    if isinstance(s, tuple):
        for v in s:
            out += _flat_sig(v)
    return out


def _ratio(got, ref, bound):
    """max(max|err| / (mx max|ref| + 1e-5), relL2 / rel) as test_gpu_kernels.check states it; non-finite -> inf."""
    rel, mx = bound
    g, f = got.double(), ref.double()
    if g.shape != f.shape:
        return (float("inf"), float("inf"), 0)
    if not torch.isfinite(g).all():
        return (float("inf"), float("inf"), 0)
    if g.numel() == 0:
        return (0.0, 0.0, 0)
    d = (g - f).abs()
    scale = f.abs().max().item()
    rl2 = (d.norm() / (f.norm() + 1e-12)).item()
    return (max(d.max().item() / (mx * scale + 1e-5), rl2 / rel), rl2, 0)


def _stat_ratio(got, ref, bound):
    rtol, atol = bound
    g, f = got.double(), ref.double().reshape(got.shape)
    if not torch.isfinite(g).all():
        return (float("inf"), float("inf"), 0)
    d = (g - f).abs()
    rl2 = (d.norm() / (f.norm() + 1e-12)).item()
    return ((d / (atol + rtol * f.abs()).clamp_min(1e-300)).max().item(), rl2, 0)


def _stats_ratio(got, ref):
    """Row statistics: [rows, 2] (mean, rstd) or [rows, 4] two-part sums; anything else (colsum, ...) must be unchanged."""
    if got.dtype == torch.float32 and got.dim() == 2 and got.shape[1] == 2:
        a = _stat_ratio(got[:, 0], ref[:, 0], STAT_BOUNDS["mean"])
        b = _stat_ratio(got[:, 1], ref[:, 1], STAT_BOUNDS["rstd"])
        return max(a, b)
    if got.dtype == torch.float32 and got.dim() == 2 and got.shape[1] == 4:
        return _stat_ratio(got, ref, STAT_BOUNDS["parts"])
    return (0.0 if torch.equal(got, ref.to(got.dtype)) else float("inf"), 0.0, 0)


def _gn_sums(ws, frames, groups, hw=None, c=None):
    """(sum, sum of squares) per (frame, group), float64 [frames, groups, 2], from the kernel's workspace (float32
    [frames, slabs, groups, 2] partial sums, vx_norm.hip) or the restatement's (float64 [frames, groups, 2] mean,
    variance: needs hw and the channel count)."""
    if ws.dtype == torch.float64:
        cnt = hw * (c // groups)
        mean, var = ws[..., 0], ws[..., 1]
        return torch.stack([mean * cnt, (var + mean * mean) * cnt], dim=-1)
    return ws.double().reshape(frames, -1, groups, 2).sum(dim=1)


def _gn_mean_var(ws, frames, hw, groups, c):
    """Any workspace -> the restatement's per-(frame, group) (mean, variance) as vx_groupnorm_apply reads it."""
    if ws.dtype == torch.float64:
        return ws
    s = _gn_sums(ws, frames, groups)
    cnt = hw * (c // groups)
    mean = s[..., 0] / cnt
    var = (s[..., 1] / cnt - mean * mean).clamp_min(0)
    return torch.stack([mean, var], dim=-1)
