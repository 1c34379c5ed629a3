"""Guidance controls on the MI355X: `vx_guidance_rescale` (both element libraries) against the float64 restatement, its
independence of the exchange layout, and VExpressPipeline with guidance_rescale and a guidance interval against the
restated loop over the oracle UNet and, bit for bit, against the no-CFG route."""
import pytest
import torch

import cases
import guidance_restated as G
from loop_restated import restated_loop
from loop_worker import call_small, cosine, dev, oracle_on_cpu, rel_l2, scheduler, small  # noqa: F401

pytestmark = pytest.mark.gpu

GUIDANCE, PHI = 3.5, 0.7


def predictions(nW, c, f, hw, mean, seed):
    """u ~ N(mean, 1), cond = u + 0.3 N(0, 1): float32 [nW, c, f, hw] each."""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(nW, c, f, hw, generator=g) + mean
    return u, u + 0.3 * torch.randn(nW, c, f, hw, generator=g)


def layout(u, cond, granules, seed, spare=3):
    """The predictions as an all-gathered unit buffer of `granules` frame granules per unit, the granules scattered over
    the buffer by a seeded permutation (with `spare` unused, NaN-filled slots): (gathered [slots, (f/G) hw, c],
    unit_index int32 [nW, 2, G])."""
    nW, c, f, hw = u.shape
    fl = f // granules
    n = nW * 2 * granules
    perm = torch.randperm(n + spare, generator=torch.Generator().manual_seed(seed))[:n]
    gathered = torch.full((n + spare, fl * hw, c), float("nan"))
    uidx = torch.empty((nW, 2, granules), dtype=torch.int32)
    k = 0
    for w in range(nW):
        for hlf, x in enumerate((u, cond)):
            for j in range(granules):
                slot = int(perm[k])
                k += 1
                uidx[w, hlf, j] = slot
                gathered[slot] = x[w, :, j * fl:(j + 1) * fl].permute(1, 2, 0).reshape(fl * hw, c)
    return gathered, uidx


def run_kernel(ops, dev, u, cond, granules, phi, seed=0, poison=True):
    nW, c, f, hw = u.shape
    gathered, uidx = layout(u, cond, granules, seed)
    ws = torch.full((ops.guidance_rescale_ws_floats(nW, f, hw),), float("nan") if poison else 0.0, device=dev)
    preds = torch.full((nW, c, f, hw), float("nan"), device=dev)
    ops.guidance_rescale(gathered.to(dev), uidx.to(dev), c, f, hw, GUIDANCE, phi, ws, preds)
    torch.cuda.synchronize()
    return preds.cpu(), gathered, uidx


# ------------------------------------------------------------------------------------------------ (9) the kernel
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("mean", [0.0, 3.0, 30.0])
@pytest.mark.parametrize("shape", [(1, 4, 16, 4096), (2, 4, 6, 80)])
def test_kernel_vs_float64_restatement(dev, elem, mean, shape):
    """max |err| <= 4 x the error the same formula has when float32 torch.std evaluates it on the CPU (computed here on
    the same inputs): the factor covers a different merge order and the one extra rounding of the scale.  A prediction
    mean of 30 standard deviations is where sum(x^2) / n - mean^2 would lose three digits."""
    from v_express_amd import lib as L, ops
    u, cond = predictions(*shape, mean, seed=int(mean) + shape[2])
    ref = G.combine_rescaled(u, cond, GUIDANCE, PHI)
    base = G.float32_baseline_error(u, cond, GUIDANCE, PHI)
    with L.element_type(elem):
        got, gathered, uidx = run_kernel(ops, dev, u, cond, 1, PHI)
        err = (got.double() - ref).abs().max().item()
        print(f"[vx_guidance_rescale {elem}, {shape}, mean {mean}] max |err| {err:.3g}, float32 torch.std baseline "
              f"{base:.3g}, max |out| {ref.abs().max().item():.3g}")
        assert torch.isfinite(got).all() and err <= 4 * base
        # phi = 0: exactly vx_combine_units, and no statistics are read (the workspace is NaN)
        zero, _, _ = run_kernel(ops, dev, u, cond, 1, 0.0)
        plain = torch.empty(shape, device=dev)
        ops.combine_units(gathered.to(dev), uidx.to(dev), shape[1], shape[2], shape[3], GUIDANCE, plain)
        torch.cuda.synchronize()
        assert torch.equal(zero, plain.cpu())
    # the CPU stand-in of the CPU suite holds the same bound
    emu = torch.empty(shape)
    G.guidance_rescale(gathered, uidx, shape[1], shape[2], shape[3], GUIDANCE, PHI,
                       torch.empty(shape[0] * shape[2] * ((shape[3] + G.CHUNK - 1) // G.CHUNK) * 6), emu)
    assert (emu.double() - ref).abs().max().item() <= 4 * base


# ------------------------------------------------------------------------------------------------ (10) layouts
@pytest.mark.parametrize("elem", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(2, 4, 16, 4096), (2, 4, 8, 80)])
def test_kernel_result_does_not_depend_on_the_layout(dev, elem, shape):
    from v_express_amd import lib as L, ops
    u, cond = predictions(*shape, 3.0, seed=5)
    with L.element_type(elem):
        one, _, _ = run_kernel(ops, dev, u, cond, 1, PHI, seed=1)
        for granules in (2, 4):
            other, _, _ = run_kernel(ops, dev, u, cond, granules, PHI, seed=10 + granules)
            assert torch.equal(one, other), granules
        # two launches of one window against one launch of two
        for w in range(2):
            single, _, _ = run_kernel(ops, dev, u[w:w + 1], cond[w:w + 1], 2, PHI, seed=20 + w)
            assert torch.equal(single[0], one[w]), w


def test_kernel_argument_errors(dev):
    from v_express_amd import lib as L, ops
    u, cond = predictions(1, 4, 4, 16, 0.0, seed=1)
    gathered, uidx = layout(u, cond, 1, 0)
    ws = torch.zeros(ops.guidance_rescale_ws_floats(1, 4, 16), device=dev)
    preds = torch.zeros(1, 4, 4, 16, device=dev)
    rc = L.lib.vx_guidance_rescale(gathered.to(dev).data_ptr(), uidx.to(dev).data_ptr(), 1, 1, 4, 4, 16, 3.5, 0.7,
                                   ws.data_ptr(), 5, preds.data_ptr(), None)
    assert rc < 0 and b"workspace" in L.lib.vx_last_error_string()
    rc = L.lib.vx_guidance_rescale(gathered.to(dev).data_ptr(), uidx.to(dev).data_ptr(), 1, 1, 4, 4, 16, 3.5, 1.5,
                                   ws.data_ptr(), ws.numel(), preds.data_ptr(), None)
    assert rc < 0 and b"phi" in L.lib.vx_last_error_string()


# ------------------------------------------------------------------------------------------------ (11) the pipeline
def _call(S, steps, **kw):
    return call_small(S, scheduler("ddim"), steps, **kw)


def test_pipeline_with_both_features_vs_restated_oracle_loop(small):
    from oracle import loop as OL
    steps = 5
    got = _call(small, steps, guidance_rescale=PHI, guidance_end=0.6)
    assert small["pipe"].last_guidance["guided_steps"] == 3
    plain = _call(small, steps)
    inp = small["inp"]
    with oracle_on_cpu():
        ref = restated_loop(small["oracle"], inp["latents"], OL.uniform_windows(small["F"], small["cf"], small["co"]),
                            cases.GUIDANCE, inp["kps_features"], inp["audio_embeddings"], steps, "ddim", phi=PHI, end=0.6,
                            unguided=("u", "c"))
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[DDIM, rescale {PHI}, guidance_end 0.6, SMALL, reflected_F11_c4o2, {steps} steps] relL2={r:.4g} "
          f"cosine={c:.6f} vs the restated loop; the clip without the controls: relL2={rel_l2(plain, ref):.4g}")
    assert torch.isfinite(got).all() and r <= 5e-2 and c >= 0.998, (r, c)
    assert r < rel_l2(plain, ref)


def test_pipeline_unguided_steps_are_the_no_cfg_route_bit_for_bit(small):
    steps = 5
    cond = cases.cond_only(small["inp"])
    off = _call(small, steps, guidance_end=0.0, guidance_rescale=PHI)
    assert torch.equal(off, _call(small, steps, inp=cond, guidance=1.0))
    got = _call(small, steps, guidance_end=0.6)
    kept = {}
    _call(small, steps, callback=lambda i, t, x: kept.setdefault(i, x.clone()))
    cont = _call(small, steps, inp=cond, guidance=1.0, strength=0.4, latents=kept[2])
    assert torch.equal(got, cont)
    assert not torch.equal(got, off)
