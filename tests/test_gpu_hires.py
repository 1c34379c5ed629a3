"""Two-pass (hi-res) sampling on the MI355X: `vx_latent_resize` (both element libraries; the code is float32 in both) on
the exact cases bit for bit, on the bound cases inside the derived bound, against the float32 stand-in bit for bit, with
guard bands around its output and unchanged inputs, its argument errors, and VExpressPipeline with `hires_size` against
the restated chain of tests/hires_restated.py started from the device's own first pass."""
import ctypes as C

import pytest
import torch

import cases
import hires_restated as H
import hires_worker as HW
import resize_cases as RC
from guard import assert_same_bits
from loop_worker import (build_pipeline, call_pipeline, cosine, dev, oracle_on_cpu, rel_l2,  # noqa: F401
                         scheduler)

pytestmark = pytest.mark.gpu

ELEMS = [torch.bfloat16, torch.float16]


def resize(ops, dev, x, h2, w2, mode):
    """ops.latent_resize on planes x [P, h, w] (CPU) -> [P, h2, w2] (CPU)."""
    out = ops.latent_resize(x[None, :, None].contiguous().to(dev), (h2, w2), mode)
    torch.cuda.synchronize()
    assert out.shape == (1, x.shape[0], 1, h2, w2) and out.dtype == torch.float32 and out.is_contiguous()
    return out[0, :, 0].cpu()


# ------------------------------------------------------------------------------------------------ vx_latent_resize
@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", RC.EXACT_CASES, ids=RC.case_id)
def test_exact_cases_bit_for_bit(dev, elem, case):
    from v_express_amd import lib as L, ops
    p, h, w, h2, w2, mode = case
    x = RC.case_input(case, exact=True)
    with L.element_type(elem):
        got = resize(ops, dev, x, h2, w2, mode)
    assert_same_bits(got, RC.reference(x, h2, w2, mode).float(), f"vx_latent_resize {RC.case_id(case)}")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", RC.BOUND_CASES, ids=RC.case_id)
def test_bound_cases_and_the_bits_of_the_standin(dev, elem, case):
    """Inside resize_bound (K = 2 taps + 2 roundings per term: derived) against float64, and the bits of the float32
    stand-in: contraction is off and the order is fixed, so the kernel and the torch expression round alike."""
    from v_express_amd import lib as L, ops
    p, h, w, h2, w2, mode = case
    x = RC.case_input(case, exact=False)
    with L.element_type(elem):
        got = resize(ops, dev, x, h2, w2, mode)
    err = (got.double() - RC.reference(x, h2, w2, mode)).abs()
    bound = RC.resize_bound(x, h2, w2, mode)
    print(f"[vx_latent_resize {elem} {RC.case_id(case)}] largest |err| / bound = {(err / bound).max().item():.3g}")
    assert torch.isfinite(got).all() and (err <= bound).all()
    assert_same_bits(got, RC.standin_planes(x, h2, w2, mode), f"vx_latent_resize {RC.case_id(case)} vs the stand-in")


@pytest.mark.parametrize("elem", ELEMS)
@pytest.mark.parametrize("case", [c for c in RC.BOUND_CASES if c[0] < 64], ids=RC.case_id)
def test_guard_bands_and_untouched_inputs(dev, elem, case):
    """The C entry point on guarded windows (bases 16 bytes past a 256-byte boundary): nothing is written outside dst,
    nothing outside src and the tables is depended on (three runs, the outside zero / NaN / huge, bit-equal), and src and
    the tables keep their bits."""
    from test_gpu_guard_bands import F32, G, O, stream, sweep
    from v_express_amd import lib as L
    p, h, w, h2, w2, mode = case
    x = RC.case_input(case, exact=False)
    tabs = RC.f32_tables(h, w, h2, w2, mode)
    src, dst = G(x, F32), O((p, h2, w2), F32)
    gt = [G(t, t.dtype) for t in tabs]
    with L.element_type(elem):
        lib = L.current()

        def call():
            L.check(lib.vx_latent_resize(src.view.data_ptr(), p, h, w, dst.view.data_ptr(), h2, w2,
                                         *(g.view.data_ptr() for g in gt), RC.TAPS[mode], stream()), "vx_latent_resize")
        out, = sweep(f"vx_latent_resize {RC.case_id(case)}", [src] + gt, [dst], call)
    assert_same_bits(out.cpu(), RC.standin_planes(x, h2, w2, mode), "guarded vx_latent_resize")
    assert_same_bits(src.view.cpu(), x, "src")
    for g, t, name in zip(gt, tabs, ("iy", "wy", "ix", "wx")):
        assert_same_bits(g.view.cpu(), t, name)


@pytest.mark.parametrize("elem", ELEMS)
def test_kernel_argument_errors(dev, elem):
    from v_express_amd import lib as L
    x = torch.ones(2, 4, 4, device=dev)
    out = torch.zeros(2, 8, 8, device=dev)
    iy, wy, ix, wx = (t.to(dev) for t in RC.f32_tables(4, 4, 8, 8, "bilinear"))
    s, d, t = x.data_ptr(), out.data_ptr(), (iy.data_ptr(), wy.data_ptr(), ix.data_ptr(), wx.data_ptr())
    with L.element_type(elem):
        lib = L.current()
        bad = [((None, 2, 4, 4, d, 8, 8, *t, 2), b"src"), ((s, 2, 4, 4, None, 8, 8, *t, 2), b"dst"),
               ((s, 2, 4, 4, s, 8, 8, *t, 2), b"must not be src"),
               ((s, 2, 4, 4, d, 8, 8, None, *t[1:], 2), b"tables"), ((s, 2, 4, 4, d, 8, 8, t[0], None, *t[2:], 2), b"tables"),
               ((s, 2, 4, 4, d, 8, 8, *t[:2], None, t[3], 2), b"tables"), ((s, 2, 4, 4, d, 8, 8, *t[:3], None, 2), b"tables"),
               ((s, 0, 4, 4, d, 8, 8, *t, 2), b"positive"), ((s, 2, 0, 4, d, 8, 8, *t, 2), b"positive"),
               ((s, 2, 4, -1, d, 8, 8, *t, 2), b"positive"), ((s, 2, 4, 4, d, 0, 8, *t, 2), b"positive"),
               ((s, 2, 4, 4, d, 8, 0, *t, 2), b"positive"), ((s, 2, 4, 4, d, 8, 8, *t, 3), b"taps"),
               ((s, 2, 4, 4, d, 8, 8, *t, 0), b"taps"), ((s, 2, 4, 4, d, 8, 8, *t, 8), b"taps")]
        for args, word in bad:
            rc = lib.vx_latent_resize(*args, None)
            msg = lib.vx_last_error_string()
            assert rc < 0 and b"vx_latent_resize" in msg and word in msg, (args, msg)
    torch.cuda.synchronize()
    assert not out.any()                                           # nothing was launched
    assert C.c_int(lib.vx_resize_abi_version()).value == 1


# ------------------------------------------------------------------------------------------------ the pipeline
@pytest.fixture(scope="module")
def pipe(dev):
    return build_pipeline(dev)


def test_pipeline_vs_the_restated_chain_from_the_device_base(pipe):
    """SMALL, F = 6, windows 4 / 2, 64 -> 128 pixels, 3 DDIM steps, then the last 3 of 5 at strength 0.6.  The first
    pass's latents (last_hires["base_latents"]) are the bits of the plain decode=False call; the second pass is judged
    against the restated second pass started from those latents (float64 resize, restated loop at 16 x 16), so that the
    drift of the first pass is not counted twice - by the bounds of test_gpu_init_video.py's pipeline test, relL2 <= 5e-2
    and cosine >= 0.998.  Measured on the MI355X: relL2 1.11e-2, cosine 0.999938; the plain init_latents route at
    16 x 16 latents (no hi-res code: the same geometry, 3 of 5 DDIM steps from random init latents) against the restated
    loop in the same job: relL2 1.15e-2, cosine 0.999933 - the bound set at 8 x 8 latents holds at 16 x 16 as it is."""
    from oracle import loop as OL
    inp1, inp2 = H.inputs()
    got = HW.call_hires(pipe, scheduler("ddim"), inp1, inp2).cpu()
    last = pipe.last_hires
    assert got.shape == (1, 4, H.F, 16, 16) and torch.isfinite(got).all()
    assert {k: last[k] for k in ("base", "size", "mode", "steps", "begin_index")} == dict(
        base=(64, 64), size=(128, 128), mode="bilinear", steps=5, begin_index=2)
    base = last["base_latents"]
    assert base.is_cuda and base.shape == (1, 4, H.F, 8, 8)
    ms = pipe.hires_timings_ms()
    assert len(ms) == 3 and all(v > 0.0 for v in ms)
    plain = call_pipeline(pipe, scheduler("ddim"), inp1, H.F, H.STEPS, H.CF, H.CO)
    assert pipe.last_hires is None
    assert_same_bits(base.cpu(), plain.cpu(), "the first pass against the plain call")
    with oracle_on_cpu():
        ref = H.second_pass(base.cpu(), inp1, inp2, OL.uniform_windows(H.F, H.CF, H.CO), cases.GUIDANCE, H.HIRES_STEPS,
                            H.STRENGTH)
    r, c = rel_l2(got, ref), cosine(got, ref)
    print(f"[DDIM hires 64 -> 128 px, 3 + 3 of 5 steps, SMALL, F = 6] relL2={r:.4g} cosine={c:.6f} vs the restated second "
          f"pass from the device's base latents (first pass {ms[0]:.2f} ms, resize {ms[1]:.3f} ms, second {ms[2]:.2f} ms)")
    assert r <= 5e-2 and c >= 0.998, (r, c)


def test_pipeline_decodes_at_the_second_size(pipe):
    inp1, inp2 = H.inputs()
    video = HW.call_hires(pipe, scheduler("ddim"), inp1, inp2, steps=1, hires_steps=2, hires_strength=0.5, decode=True)
    assert video.shape == (1, 3, H.F, 128, 128) and torch.isfinite(video).all()
    assert pipe.last_hires["size"] == (128, 128) and len(pipe.timings_ms()) == 2
