"""A separate audio guidance scale on the MI355X: `vx_combine_units3` / `vx_guidance_rescale3` (both element libraries)
against float64, their independence of the exchange layout, their two exact properties (equal c and m rows give the
two-row kernel; phi = 0 gives the combine), and VExpressPipeline with `audio_guidance_scale` against the restated
three-row loop over the oracle UNet, the all-zero-audio identity and lone rows against batched rows bit for bit."""
import os

import pytest
import torch

import audio_guidance_restated as AG
import cases
from loop_restated import restated_loop
from loop_worker import call_small, cosine, dev, oracle_on_cpu, rel_l2, scheduler, small  # noqa: F401

pytestmark = pytest.mark.gpu

S, S_A, PHI = 3.5, 6.0, 0.7


def predictions(nW, c, f, hw, mean, seed):
    """u ~ N(mean, 1), m = u + 0.3 N(0, 1), c = m + 0.3 N(0, 1): float32 [nW, c, f, hw] each."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(nW, c, f, hw, generator=g) + mean
    m = u + 0.3 * torch.randn(nW, c, f, hw, generator=g)
    return u, m, m + 0.3 * torch.randn(nW, c, f, hw, generator=g)


def layout(rows, granules, seed, spare=3):
    """tests/test_gpu_guidance.py's `layout` for any number of rows: the predictions as an all-gathered unit buffer of
    `granules` frame granules per unit, the granules scattered over the buffer by a seeded permutation (with `spare`
    unused, NaN-filled slots): (gathered [slots, (f/G) hw, c], unit_index int32 [nW, len(rows), G])."""
    nW, c, f, hw = rows[0].shape
    fl = f // granules
    n = nW * len(rows) * granules
    perm = torch.randperm(n + spare, generator=torch.Generator().manual_seed(seed))[:n]
    gathered = torch.full((n + spare, fl * hw, c), float("nan"))
    uidx = torch.empty((nW, len(rows), granules), dtype=torch.int32)
    k = 0
    for w in range(nW):
        for r, x in enumerate(rows):
            for j in range(granules):
                slot = int(perm[k])
                k += 1
                uidx[w, r, j] = slot
                gathered[slot] = x[w, :, j * fl:(j + 1) * fl].permute(1, 2, 0).reshape(fl * hw, c)
    return gathered, uidx


def run_combine3(ops, dev, rows, granules, seed=0, s=S, s_a=S_A):
    nW, c, f, hw = rows[0].shape
    gathered, uidx = layout(rows, granules, seed)
    preds = torch.full((nW, c, f, hw), float("nan"), device=dev)
    ops.combine_units3(gathered.to(dev), uidx.to(dev), c, f, hw, s, s_a, preds)
    torch.cuda.synchronize()
    return preds.cpu()


def run_rescale3(ops, dev, rows, granules, phi, seed=0):
    nW, c, f, hw = rows[0].shape
    gathered, uidx = layout(rows, granules, seed)
    ws = torch.full((ops.guidance_rescale_ws_floats(nW, f, hw),), float("nan"), device=dev)     # poisoned
    preds = torch.full((nW, c, f, hw), float("nan"), device=dev)
    ops.guidance_rescale3(gathered.to(dev), uidx.to(dev), c, f, hw, S, S_A, phi, ws, preds)
    torch.cuda.synchronize()
    return preds.cpu()


# ------------------------------------------------------------------------------------------------ (8) the combine
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mean", [0.0, 3.0, 30.0])
@pytest.mark.parametrize("shape", [(1, 4, 16, 4096), (2, 4, 6, 80)])
def test_combine3_vs_float64(dev, elem, mean, shape):
    """(u + s (m - u)) + s_a (c - m) in float32 is six roundings (m - u, its product, the sum, c - m, its product, the
    sum), each of a value no larger than the running magnitude |u| + |s| |m - u| + |s_a| |c - m|:
    |err| <= 6 * 2^-24 * that magnitude, elementwise, the right side in float64.  (A fused multiply-add only removes
    roundings.)"""
    from v_express_amd import lib as L, ops
    u, m, c = predictions(*shape, mean, seed=int(mean) + shape[2])
    ref = AG.combine3(u, m, c, S, S_A)
    mag = u.double().abs() + S * (m.double() - u.double()).abs() + S_A * (c.double() - m.double()).abs()
    with L.element_type(elem):
        got = run_combine3(ops, dev, (u, m, c), 1)
    err = (got.double() - ref).abs()
    print(f"[vx_combine_units3 {elem}, {shape}, mean {mean}] max |err| / (2^-24 magnitude) = "
          f"{(err / (2.0 ** -24 * mag)).max().item():.3g} (bound 6), max |err| {err.max().item():.3g}")
    assert torch.isfinite(got).all() and bool((err <= 6 * 2.0 ** -24 * mag).all())


# ------------------------------------------------------------------------------------------------ (9) the rescale
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mean", [0.0, 3.0, 30.0])
@pytest.mark.parametrize("shape", [(1, 4, 16, 4096), (2, 4, 6, 80)])
def test_rescale3_vs_float64_restatement(dev, elem, mean, shape):
    """The criterion of vx_guidance_rescale (tests/test_gpu_guidance.py): max |err| <= 4 x the error the same formula has
    when float32 torch.std evaluates it on the CPU, on the same inputs; a NaN-poisoned workspace; phi = 0 is
    vx_combine_units3 bit for bit."""
    from v_express_amd import lib as L, ops
    u, m, c = predictions(*shape, mean, seed=int(mean) + shape[2])
    ref = AG.combine3_rescaled(u, m, c, S, S_A, PHI)
    base = AG.float32_baseline_error3(u, m, c, S, S_A, PHI)
    with L.element_type(elem):
        got = run_rescale3(ops, dev, (u, m, c), 1, PHI)
        err = (got.double() - ref).abs().max().item()
        print(f"[vx_guidance_rescale3 {elem}, {shape}, mean {mean}] max |err| {err:.3g}, float32 torch.std baseline "
              f"{base:.3g}, max |out| {ref.abs().max().item():.3g}")
        assert torch.isfinite(got).all() and err <= 4 * base
        assert torch.equal(run_rescale3(ops, dev, (u, m, c), 1, 0.0), run_combine3(ops, dev, (u, m, c), 1))
    # the CPU stand-in of the CPU suite holds the same bound
    gathered, uidx = layout((u, m, c), 1, 0)
    emu = torch.empty(shape)
    AG.guidance_rescale3(gathered, uidx, shape[1], shape[2], shape[3], S, S_A, PHI,
                         torch.empty(shape[0] * shape[2] * ((shape[3] + AG.CHUNK - 1) // AG.CHUNK) * 6), emu)
    assert (emu.double() - ref).abs().max().item() <= 4 * base


# ------------------------------------------------------------------------------------------------ (10) layouts
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(2, 4, 16, 4096), (2, 4, 8, 80)])
def test_results_do_not_depend_on_the_layout(dev, elem, shape):
    from v_express_amd import lib as L, ops
    rows = predictions(*shape, 3.0, seed=5)
    with L.element_type(elem):
        for run in (lambda r, g, seed: run_combine3(ops, dev, r, g, seed),
                    lambda r, g, seed: run_rescale3(ops, dev, r, g, PHI, seed)):
            one = run(rows, 1, 1)
            assert torch.isfinite(one).all()
            for granules in (2, 4):
                assert torch.equal(one, run(rows, granules, 10 + granules)), granules
            # two launches of one window against one launch of two
            for w in range(2):
                single = run(tuple(x[w:w + 1] for x in rows), 2, 20 + w)
                assert torch.equal(single[0], one[w]), w


# ------------------------------------------------------------------------------------------------ (11) equal rows
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("s_a", [0.0, 6.0])
def test_equal_c_and_m_rows_give_the_two_row_kernel(dev, elem, s_a):
    from v_express_amd import lib as L, ops
    u, m, _ = predictions(2, 4, 6, 80, 3.0, seed=9)
    u[0, 0, 0, :8], m[0, 0, 0, :8] = 0.0, 0.0                    # some exact zeros of either sign
    u[0, 1, 0, :8], m[0, 1, 0, :8] = -0.0, -0.0
    with L.element_type(elem):
        three = run_combine3(ops, dev, (u, m, m.clone()), 2, seed=3, s_a=s_a)
        gathered, uidx = layout((u, m), 2, 4)
        two = torch.full((2, 4, 6, 80), float("nan"), device=dev)
        ops.combine_units(gathered.to(dev), uidx.to(dev), 4, 6, 80, S, two)
        torch.cuda.synchronize()
    assert torch.isfinite(three).all() and torch.equal(three, two.cpu())


# ------------------------------------------------------------------------------------------------ (13) the pipeline
def _call(S_, steps, **kw):
    return call_small(S_, scheduler("ddim"), steps, **kw)


def _restated(small, steps, s, s_a, **kw):
    from oracle import loop as OL
    inp = small["inp"]
    with oracle_on_cpu():
        return restated_loop(small["oracle"], inp["latents"], OL.uniform_windows(small["F"], small["cf"], small["co"]), s,
                             inp["kps_features"], inp["audio_embeddings"], steps, "ddim", s_a=s_a, **kw)


def test_pipeline_three_rows_vs_restated_oracle_loop(small):
    """reflected_F11_c4o2, 5 DDIM steps, the bounds of tests/test_gpu_guidance.py's pipeline test at this geometry
    (relative L2 <= 5e-2, cosine >= 0.998), and strictly closer to the three-row loop than the two-row clip is."""
    steps = 5
    got = _call(small, steps, audio_guidance_scale=S_A)
    assert small["pipe"].last_guidance["rows"] == ("u", "m", "c")
    plain = _call(small, steps)
    ref = _restated(small, steps, S, S_A)
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[DDIM, audio_guidance_scale {S_A}, guidance_scale {S}, SMALL, reflected_F11_c4o2, {steps} steps] "
          f"relL2={r:.4g} cosine={c:.6f} vs the restated loop; the two-row clip: relL2={rel_l2(plain, ref):.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2 and c >= 0.998, (r, c)
    assert r < rel_l2(plain, ref) and not torch.equal(got, plain)
    # with the rescale and an interval
    got = _call(small, steps, audio_guidance_scale=S_A, guidance_rescale=PHI, guidance_end=0.6)
    assert small["pipe"].last_guidance["guided_steps"] == 3
    ref = _restated(small, steps, S, S_A, phi=PHI, end=0.6)
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[the same with rescale {PHI}, guidance_end 0.6] relL2={r:.4g} cosine={c:.6f}")
    assert torch.isfinite(got).all() and r <= 5e-2 and c >= 0.998, (r, c)


def test_pipeline_rows_m_c_vs_restated_oracle_loop(small):
    steps = 5
    got = _call(small, steps, guidance=1.0, audio_guidance_scale=3.5)
    assert small["pipe"].last_guidance["rows"] == ("m", "c")
    ref = _restated(small, steps, 1.0, 3.5)
    nocfg = _call(small, steps, inp=cases.cond_only(small["inp"]), guidance=1.0)
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[DDIM, guidance_scale 1, audio_guidance_scale 3.5, SMALL, reflected_F11_c4o2, {steps} steps] relL2={r:.4g} "
          f"cosine={c:.6f} vs the restated (m, c) loop; the unguided clip: relL2={rel_l2(nocfg, ref):.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2 and c >= 0.998, (r, c)
    assert r < rel_l2(nocfg, ref)
    with pytest.raises(ValueError, match="audio_guidance_scale.*2 batch row"):
        _call(small, steps, inp=cases.cond_only(small["inp"]), guidance=1.0, audio_guidance_scale=3.5)


@pytest.mark.parametrize("s_a", [0.0, 6.0])
def test_pipeline_all_zero_audio_is_the_two_row_clip(small, s_a):
    steps = 3
    inp = dict(small["inp"], audio_embeddings=torch.zeros_like(small["inp"]["audio_embeddings"]))
    two = _call(small, steps, inp=inp)
    three = _call(small, steps, inp=inp, audio_guidance_scale=s_a)
    assert small["pipe"].last_guidance["rows"] == ("u", "m", "c")
    assert torch.isfinite(two).all() and torch.equal(two, three)


def test_defaults_on_the_device_are_the_two_row_clip(small):
    steps = 3
    base = _call(small, steps)
    assert torch.equal(base, _call(small, steps, audio_guidance_scale=None))
    assert torch.equal(base, _call(small, steps, audio_guidance_scale=cases.GUIDANCE))


@pytest.mark.parametrize("geometry", ["one_window", "two_windows"])
def test_lone_rows_equal_batched_rows(dev, geometry, tmp_path):
    """Three rows per window with the rescale and an interval: one process (one UNet call of three rows per window)
    against two ranks folded onto this GPU (gloo, whole units), where one window's rows run as (u, m) on one rank and c
    alone on the other.  Bit for bit: the kernels are batch-invariant and the combine does not see the layout."""
    import subprocess
    import sys
    import audio_guidance_worker as W
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "lat.pt")
    env = dict(os.environ, VX_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(29620 + len(geometry)),
           os.path.join(root, "tests", "audio_guidance_worker.py"), out, geometry]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    got = torch.load(out)
    ref, sched, _ = W.run(geometry, device=dev)                      # this process: no process group -> single rank
    assert got["schedule"]["world"] == 2 and got["schedule"]["kind"] == "whole units" and sched["world"] == 1
    print(f"[lone rows, {geometry}] relL2 two ranks vs one process = {rel_l2(got['latents'], ref):.3g}")
    assert torch.isfinite(ref).all() and torch.equal(got["latents"], ref)
