"""A recorder of the calls a model file makes (TEST INFRASTRUCTURE, host only, torch on any device).

vae.py, wav2vec2.py and prologue.py compose `blocks.*` and `ops.*` calls; tests/model_wiring_cases.py checks them stage by
stage, each stage on the input the PRODUCT gave it.  The tap wraps the callables those files reach - through the module
attributes they reach them by - and keeps, for every call made at the model file's own level:

    name      "blocks.resnet_block", "ops.gemm", ...
    inputs    {parameter name: clone of the tensor argument, taken BEFORE the call}
    scalars   {parameter name: value} of every other plain argument after the defaults are applied (int / float / bool /
              None / str / tuples of them); a ConvGeom argument gives "geom.stride", "geom.pad", ... entries
    out       clone of the returned tensor (of the first element of a returned tuple; None when the call returns none)
    after     {parameter name: clone} of the tensor arguments the call CHANGED (`_self_attention` writes h in place,
              `ops.gemm(..., residual=lat, out=lat)` writes lat)

Calls nested inside a tapped call (the GEMMs of a resnet block, the four launches of an upsampler) are not recorded.  The
tap hands every argument through untouched and returns what the callable returned: it does not change what runs.

    tap = stage_tap.StageTap(ops, blocks).install(monkeypatch)
    model.decode(z)
    [c.name for c in tap.calls]
"""
import inspect

import torch

BLOCK_CALLS = ("resnet_block", "_self_attention", "upsample")
OPS_CALLS = ("gemm", "layernorm", "groupnorm", "wave_conv1d", "small_kv_attention", "ncfhw_to_nhwc", "nhwc_to_ncfhw",
             "vae_postprocess")
_GEOM = ("nb", "h_in", "w_in", "kh", "kw", "stride", "pad", "upsample", "h_out", "w_out")
_PLAIN = (int, float, bool, str, type(None))


class Call:
    __slots__ = ("name", "inputs", "scalars", "out", "after")

    def __init__(self, name, inputs, scalars):
        self.name, self.inputs, self.scalars, self.out, self.after = name, inputs, scalars, None, {}

    def __repr__(self):
        return f"{self.name}({', '.join(f'{k}={tuple(v.shape)}' for k, v in self.inputs.items())}; {self.scalars})"


def _scalars(args):
    out = {}
    for k, v in args.items():
        if isinstance(v, _PLAIN) or (isinstance(v, tuple) and all(isinstance(e, _PLAIN) for e in v)):
            out[k] = v
        elif type(v).__name__ == "ConvGeom":
            out.update({f"{k}.{n}": getattr(v, n) for n in _GEOM})
    return out


class StageTap:
    def __init__(self, ops, blocks):
        self.ops, self.blocks = ops, blocks
        self.calls, self._depth = [], 0

    def install(self, monkeypatch):
        for mod, prefix, names in ((self.blocks, "blocks.", BLOCK_CALLS), (self.ops, "ops.", OPS_CALLS)):
            for n in names:
                monkeypatch.setattr(mod, n, self._wrap(prefix + n, getattr(mod, n)))
        return self

    def clear(self):
        self.calls = []
        return self

    def _wrap(self, name, real):
        params = inspect.signature(real)                       # (follows __wrapped__ through a spy's wrapper)

        def call(*a, **k):
            if self._depth:
                return real(*a, **k)
            bound = params.bind(*a, **k)
            bound.apply_defaults()
            args = bound.arguments
            tensors = {n: v for n, v in args.items() if torch.is_tensor(v)}
            rec = Call(name, {n: v.detach().clone() for n, v in tensors.items()}, _scalars(args))
            self._depth += 1
            try:
                out = real(*a, **k)
            finally:
                self._depth -= 1
            first = out[0] if isinstance(out, tuple) else out          # (blocks.upsample returns (tokens, H, W))
            rec.out = first.detach().clone() if torch.is_tensor(first) else None
            for n, v in tensors.items():
                if not torch.equal(v, rec.inputs[n]):
                    rec.after[n] = v.detach().clone()
            self.calls.append(rec)
            return out
        call.__wrapped__ = real
        return call
