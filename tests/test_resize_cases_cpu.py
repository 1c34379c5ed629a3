"""The latent resize on the host: the tap tables of tests/resize_cases.py against torch.nn.functional.interpolate in
float64, their invariants, the float32 stand-in on the exact and the bound cases, the proof that every mutant is caught
by a case, the sixth ABI header and the argument checks of ops.latent_resize."""
import ctypes
import inspect

import pytest
import torch
import torch.nn.functional as F

import loop_worker  # noqa: F401  (puts the repository on sys.path)
import resize_cases as RC

MODES = ("bilinear", "bicubic")


# ------------------------------------------------------------------------------------------------ (1) the tables
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", RC.TABLE_SHAPES)
def test_tables_agree_with_interpolate_in_float64(shape, mode):
    h, w, h2, w2 = shape
    x = torch.randn(3, h, w, generator=torch.Generator().manual_seed(h * w2), dtype=torch.float64)
    want = F.interpolate(x[None], size=(h2, w2), mode=mode, align_corners=False, antialias=False)[0]
    err = (RC.reference(x, h2, w2, mode) - want).abs().max().item()
    print(f"[{mode} {h}x{w} -> {h2}x{w2}] max |tables - F.interpolate| in float64 = {err:.3g}")
    assert err <= 1e-12


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", RC.TABLE_SHAPES + [(64, 64, 96, 96)])
def test_weights_sum_to_one_and_indices_are_in_range(shape, mode):
    from v_express_amd import ops
    h, w, h2, w2 = shape
    for n_in, n_out in ((h, h2), (w, w2)):
        idx, wts = RC.taps(n_in, n_out, mode)
        assert idx.shape == wts.shape == (n_out, RC.TAPS[mode]) and idx.dtype == torch.int64 and wts.dtype == torch.float64
        assert (wts.sum(dim=1) - 1.0).abs().max().item() <= 1e-15
        assert idx.min().item() >= 0 and idx.max().item() <= n_in - 1
        # the product builds the same tables
        idx_p, wts_p = ops.resize_taps(n_in, n_out, mode)
        assert torch.equal(idx_p, idx) and torch.equal(wts_p, wts)


# ------------------------------------------------------------------------------------------------ (2) the stand-in
@pytest.mark.parametrize("case", RC.EXACT_CASES, ids=RC.case_id)
def test_standin_is_exact_on_the_exact_cases(case):
    """Small integers and dyadic weights: the float64 result is a float32 number, the stand-in and torch's own float32
    interpolate give exactly it."""
    p, h, w, h2, w2, mode = case
    x = RC.case_input(case, exact=True)
    ref = RC.reference(x, h2, w2, mode)
    assert torch.equal(ref.float().double(), ref)
    got = RC.standin_planes(x, h2, w2, mode)
    assert got.dtype == torch.float32 and got.shape == (p, h2, w2) and torch.equal(got.double(), ref)
    assert torch.equal(F.interpolate(x[None], size=(h2, w2), mode=mode, align_corners=False)[0].double(), ref)
    if (h, w) == (h2, w2):
        assert torch.equal(got, x)


@pytest.mark.parametrize("case", RC.BOUND_CASES, ids=RC.case_id)
def test_standin_is_inside_the_bound(case):
    p, h, w, h2, w2, mode = case
    x = RC.case_input(case, exact=False)
    err = (RC.standin_planes(x, h2, w2, mode).double() - RC.reference(x, h2, w2, mode)).abs()
    bound = RC.resize_bound(x, h2, w2, mode)
    print(f"[stand-in {RC.case_id(case)}] largest |err| / bound = {(err / bound).max().item():.3g}")
    assert (bound > 0).all() and (err <= bound).all()


def test_latent_resize_standin_has_the_shape_contract_of_the_op():
    x = torch.randn(1, 4, 3, 5, 7, generator=torch.Generator().manual_seed(0))
    keep = x.clone()
    out = RC.latent_resize(x, (8, 11), "bicubic")
    assert out.shape == (1, 4, 3, 8, 11) and out.dtype == torch.float32 and out.is_contiguous() and torch.equal(x, keep)
    assert torch.equal(out[0, 2, 1], RC.standin_planes(x[0, 2, 1:2], 8, 11, "bicubic")[0])


# ------------------------------------------------------------------------------------------------ (3) the mutants
@pytest.mark.parametrize("mutant", sorted(RC.MUTANTS))
def test_every_mutant_is_caught_by_a_case(mutant):
    hits = [RC.case_id(c) for c in RC.EXACT_CASES if RC.caught(mutant, c, True)] + \
           [RC.case_id(c) for c in RC.BOUND_CASES if RC.caught(mutant, c, False)]
    print(f"[{mutant}: {RC.MUTANTS[mutant]}] caught by {len(hits)} case(s): {hits}")
    assert hits


def test_the_true_resize_is_not_caught():
    for c in RC.EXACT_CASES:
        assert not RC.caught(None, c, True)
    for c in RC.BOUND_CASES:
        assert not RC.caught(None, c, False)


# ------------------------------------------------------------------------------------------------ (4) the sixth header
def test_sixth_header_parses_and_is_disjoint_from_the_others():
    from v_express_amd import abi
    r = abi.resize_header()
    assert r is abi.resize_header() and r.version == 1 and not r.enums and not r.structs
    assert list(r.functions) == ["vx_resize_abi_version", "vx_latent_resize"]
    for other in (abi.header(), abi.guidance_header(), abi.samplers_header(), abi.solvers_header(), abi.reuse_header()):
        assert not set(r.functions) & set(other.functions)
    i32, vp = ctypes.c_int32, ctypes.c_void_p
    assert r.functions["vx_resize_abi_version"] == (i32, [])
    restype, params = r.functions["vx_latent_resize"]
    assert restype is i32 and [t for _, t in params] == [vp, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp]
    assert [n for n, _ in params] == ["src", "planes", "h", "w", "dst", "h2", "w2", "iy", "wy", "ix", "wx", "taps",
                                      "stream"]
    text = open(abi.RESIZE_HEADER).read()
    with pytest.raises(ImportError, match="VX_ABI_VERSION"):
        abi.parse(text, "resize.h")
    assert abi.parse(text, "resize.h", "VX_RESIZE_ABI_VERSION").functions == r.functions
    # the other five headers are what they were
    assert (abi.header().version, abi.guidance_header().version, abi.samplers_header().version,
            abi.solvers_header().version, abi.reuse_header().version) == (15, 1, 1, 1, 1)


def test_sixth_header_is_bound_on_both_libraries_and_stamped():
    import os
    import subprocess
    import sys
    from v_express_amd import abi, lib
    functions = abi.resize_header().functions
    assert not set(functions) & set(lib.declared_symbols())
    for so in (lib.lib, lib.lib_f16()):
        for n, (restype, params) in functions.items():
            fn = so.__dict__[n]
            assert fn.restype is restype and list(fn.argtypes) == [t for _, t in params], n
        assert so.vx_resize_abi_version() == abi.resize_header().version == 1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "lib_id.py")], capture_output=True, text=True)
    assert out.stdout.strip() == lib.source_id()
    assert "vexpress_hip_resize.h" in open(os.path.join(root, "tools", "lib_id.py")).read()
    mk = open(os.path.join(lib.CSRC, "Makefile")).read()
    assert "vexpress_hip_resize.h" in mk and "vx_resize.hip" in mk


# ------------------------------------------------------------------------------------------------ (5) ops.latent_resize
def test_ops_latent_resize_matches_the_header_and_checks_its_arguments():
    from v_express_amd import ops
    assert list(inspect.signature(ops.latent_resize).parameters) == ["latents", "size", "mode"]
    assert inspect.signature(ops.latent_resize).parameters["mode"].default == "bilinear"
    assert list(inspect.signature(RC.latent_resize).parameters) == ["latents", "size", "mode"]
    assert ops.RESIZE_MODES == MODES
    x = torch.zeros(1, 4, 3, 8, 8)
    with pytest.raises(TypeError, match="float32"):
        ops.latent_resize(x.double(), (16, 16))
    with pytest.raises(TypeError, match="contiguous"):
        ops.latent_resize(x.transpose(3, 4), (16, 16))
    with pytest.raises(TypeError, match="latents"):
        ops.latent_resize([1.0], (16, 16))
    with pytest.raises(ValueError, match=r"\[1, C, F, h, w\]"):
        ops.latent_resize(x[0], (16, 16))
    with pytest.raises(ValueError, match=r"\[1, C, F, h, w\]"):
        ops.latent_resize(torch.zeros(2, 4, 3, 8, 8), (16, 16))
    with pytest.raises(ValueError, match="mode"):
        ops.latent_resize(x, (16, 16), "nearest")
    for size in (16, (16,), (16, 16, 16), None):
        with pytest.raises(ValueError, match="size"):
            ops.latent_resize(x, size)
    for size in ((0, 16), (16, -1)):
        with pytest.raises(ValueError, match="positive"):
            ops.latent_resize(x, size)
    with pytest.raises(ValueError, match="mode"):
        ops.resize_taps(8, 16, "area")
