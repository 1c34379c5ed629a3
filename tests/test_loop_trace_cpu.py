"""The denoising loop issues the launches it issued before it was split into its stitch / guidance / sampler / known parts:
tests/loop_trace.py records every loop launch of thirteen small clips (samplers x guidance routes x blends x init clips)
under emulated kernels, and the record must equal tests/golden/denoise_launch_trace.json, which the same recorder wrote at
the commit before the split.  The sequence, every shape and dtype, every int / bool / str / None argument and the int32
tables (terms, frame ids, unit index) must be equal exactly; floats to relative 1e-6 - they are float32 by the time they
reach a kernel and a neighbouring step's coefficient is off by orders of magnitude more: the margin only absorbs a
last-place difference between host maths libraries."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_trace as T  # noqa: E402
from loop_worker import small_pipe  # noqa: E402,F401

REL = 1e-6


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "denoise_launch_trace.json")) as fh:
        return json.load(fh)


def differences(got, want, where, out):
    """Appends to `out` where the two JSON values differ: dict(float=v) leaves to relative REL, anything else exactly
    (type included: True is not 1)."""
    if isinstance(want, dict) and set(want) == {"float"}:
        ok = isinstance(got, dict) and set(got) == {"float"} and (
            got["float"] == want["float"] or abs(got["float"] - want["float"]) <= REL * abs(want["float"]))
        if not ok:
            out.append(f"{where}: {got} != {want}")
    elif isinstance(want, dict) and isinstance(got, dict) and set(got) == set(want):
        for k in want:
            differences(got[k], want[k], f"{where}.{k}", out)
    elif isinstance(want, list) and isinstance(got, list) and len(got) == len(want):
        for i, (g, w) in enumerate(zip(got, want)):
            differences(g, w, f"{where}[{i}]", out)
    elif type(got) is not type(want) or got != want:
        out.append(f"{where}: {got} != {want}")


def test_the_comparison_sees_what_it_must():
    want = dict(op="x", args=[dict(float=0.5), 3, True, None, dict(shape=[2], dtype="torch.int32", values=[1, 2])])
    for got in (dict(op="y", args=want["args"]), dict(want, args=want["args"][:4]),
                dict(want, args=[dict(float=0.5 + 1e-6)] + want["args"][1:]),
                dict(want, args=[0.5] + want["args"][1:]), dict(want, args=want["args"][:2] + [1] + want["args"][3:]),
                dict(want, args=want["args"][:4] + [dict(want["args"][4], values=[1, 3])])):
        out = []
        differences(got, want, "case", out)
        assert out, got
    out = []
    differences(dict(want, args=[dict(float=0.5 * (1 + 5e-7))] + want["args"][1:]), want, "case", out)
    assert not out


def test_every_case_of_the_issue_is_in_the_golden_file(golden):
    assert list(golden) == list(T.CASES) and len(T.CASES) == 13
    assert all(case["calls"] for case in golden.values())


@pytest.mark.parametrize("name", list(T.CASES))
def test_the_loop_issues_the_launches_of_the_parent_commit(monkeypatch, small_pipe, golden, name):
    got = T.record(monkeypatch, small_pipe, [name])[name]
    want = golden[name]
    assert [c["op"] for c in got["calls"]] == [c["op"] for c in want["calls"]]
    out = []
    differences(got, want, name, out)
    assert not out, "\n".join(out[:20])
