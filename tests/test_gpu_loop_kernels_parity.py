"""The float32 kernels of the denoising loop give the bits they gave before vx_elem.hip's combine kernels and
mean-of-terms loops were folded into one each: sha256 digests of every output buffer on the seeded inputs of
tests/loop_kernels.py against tests/golden/loop_kernels_parent.json (written on an MI355X with the parent commit's
library by `python tests/make_golden.py loop_kernels`).  No tolerance: the change was a refactor."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import loop_kernels as LK  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(HERE, "golden", "loop_kernels_parent.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("element", sorted(LK.ELEMENTS))
def test_loop_kernels_give_the_parent_builds_bits(parent, element):
    """Every input digest equals the stored one (the generator did not drift), then every output digest does: both
    combine kernels (one row: -0.0 -> +0.0 and inf -> NaN as u + s (u - u) gives them), both rescales at phi 0 and 0.7,
    S = 1 and 2 frame granules, and the three updates (a skipped middle term, the x0 history unread and read, c_z = 0 and
    not).  The float16 library shares these float32 kernels."""
    from v_express_amd import lib as L
    with L.element_type(LK.ELEMENTS[element]):
        got = LK.run("cuda")
    want = parent[element]
    assert got["inputs"] == want["inputs"], "the seeded inputs drifted: the output digests say nothing"
    assert sorted(got["outputs"]) == sorted(want["outputs"])
    differ = [k for k in want["outputs"] if got["outputs"][k] != want["outputs"][k]]
    assert not differ, f"{element}: outputs that differ from the parent build's bits: {differ}"
