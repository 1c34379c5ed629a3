"""Guard bands on a real MI355X: no kernel writes, or depends on, bytes outside its operands' extents.

Every case (a) puts each output and workspace in a tests/guard.py window (a stride larger than the width wherever the
ABI takes one) and checks after the call that nothing outside changed, (b) puts each input in a window too and runs the
call three times with the outside holding zeros, NaNs and +-largest-finite: the three results must be bit-identical and
finite, (c) compares the "nan" run with the fp32 restatement tests/test_gpu_kernels.py uses for the op, under that file's
tolerances (`check` below is its helper; float16 runs take its 8x tighter figures).  Every window starts 16 bytes past a
256-byte boundary - the alignment the ABI promises for a base and no more (BASE_OFFSET below) - so a kernel that rounds an
address down, or assumes a wider alignment, lands in the guard.  tests/test_guard_cpu.py shows that the harness rejects
planted overruns and stray reads.  bfloat16 everywhere; every vx_gemm, GroupNorm and vx_attention case also on the
float16 library (`ops_el`).

Entry points of include/vexpress_hip.h and their case (every `vx_*` of the header):
  vx_gemm                       test_gemm_classic (ragged M / K tail, N = 8, N no tile multiple; strided A, in-place residual,
                                float32 output), test_gemm_split_k, test_conv3x3, test_gemm_persistent_*, test_gemm_coop_split,
                                test_fp8_layernorm_and_gemm, test_gemm_split_rows_and_vt
  vx_gemm_gn_slabs / vx_gemm_splitk_ws_bytes / vx_gemm_ring_coop_ok / vx_gemm_config_name / vx_gemm_last_kernel /
  vx_last_kernel                host-side answers (an int / a string), used by the cases above to size and pin the launch
  vx_ff_pack_weights, vx_ff_fused            test_ff_fused
  vx_tblock_pack, vx_tblock_fused            test_tblock_fused;  vx_tblock_packed_bytes: host-side size
  vx_audio_xattn_pack, vx_audio_xattn        test_audio_xattn;   vx_audio_xattn_packed_bytes / _supported: host-side
  vx_groupnorm                  test_groupnorm (plain, dual source, padded-output form); vx_groupnorm_ws_floats: host-side size
  vx_groupnorm_stats / _apply / _fold_linear  test_groupnorm_stats_apply_fold
  vx_layernorm                  test_layernorm
  vx_row_stats / _parts / _finalize           test_row_stats
  vx_layernorm_fp8              test_fp8_layernorm_and_gemm
  vx_attention                  test_flash_attention
  vx_attention_bounded, vx_key_norm_max       test_bounded_attention_and_key_norm_max
  vx_temporal_attention         test_temporal_attention
  vx_small_kv_attention         test_small_kv_attention
  vx_add_row_bias, vx_add_residual_f32        test_add_row_bias_and_residual_f32
  vx_pad_image, vx_pixel_shuffle2x            test_pad_image_and_pixel_shuffle
  vx_gather_latents, vx_cfg_combine, vx_pack_rows, vx_nhwc_to_ncfhw, vx_ncfhw_to_nhwc   test_layout_kernels
  vx_combine_units, vx_combine_units3, vx_guidance_rescale, vx_guidance_rescale3         test_combine_and_rescale;
                                vx_guidance_rescale_ws_floats: host-side size
  vx_vae_postprocess, vx_vae_postprocess_composite                                       test_vae_postprocess
  vx_median3d                   test_median3d
  vx_wave_conv1d                test_wave_conv1d
  vx_overlap_ddim_step / _multistep_step / _ancestral_step / vx_overlap_blend            test_overlap_updates
  vx_known_blend                test_known_blend
  vx_last_error_string, vx_abi_version, vx_build_id, vx_element_type, vx_device_info     write nothing to device memory
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from guard import KINDS, Guarded, assert_same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from v_express_amd import lib as L, ops as o
    return L, o


@pytest.fixture
def ops(mods):
    L, o = mods
    with L.element_type(torch.bfloat16):
        yield o


@pytest.fixture(params=[torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def ops_el(mods, request):
    """(ops, element type, tolerance factor) - every GEMM, GroupNorm and flash-attention (vx_attention) case runs on both
    libraries."""
    L, o = mods
    with L.element_type(request.param):
        yield o, request.param, (0.125 if request.param is torch.float16 else 1.0)


def check(got, ref, what, rel=6e-3, mx=2 ** -7, tol=1.0):
    """tests/test_gpu_kernels.py::check (tol = that file's TOL: 1 for bfloat16, 0.125 for float16)."""
    if "fp8" not in what:
        rel, mx = rel * tol, mx * tol
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert torch.isfinite(got).all(), f"{what}: non-finite output ({(~torch.isfinite(got)).sum().item()} elements)"
    err = (got - ref).abs()
    scale = ref.abs().max().item() + 1e-12
    rl2 = (err.pow(2).sum().sqrt() / (ref.pow(2).sum().sqrt() + 1e-12)).item()
    msg = f"{what}: max|err|={err.max().item():.4g}, max|ref|={scale:.4g}, relL2={rl2:.3g}"
    assert err.max().item() <= mx * scale + 1e-5 and rl2 <= rel, msg


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


# Every window's base is 16 bytes past a 256-byte boundary: the alignment the ABI promises and no more.  16 bytes is eight
# bfloat16 / float16 elements (the `% 8` row strides), what the header demands of the float32 loop operands ("16-byte
# aligned") and of the fp8 rows (strides % 16), and the widest load or store a lane can issue; the float32 bias, statistics
# and workspace windows get the same 16 - less than eight of THEIR elements - since the header promises nothing more for a
# base.  Production passes such bases (x[:, 320:], the Q | K | V column slices, big[:, k:2k]); a kernel that rounded an
# address down, or assumed a wider alignment, would read or write the guard in front of the window.
BASE_OFFSET = 16


def _window(shape, dtype, ld):
    g = Guarded(shape, dtype, DEV, ld=ld, base_offset_bytes=BASE_OFFSET)
    assert g.view.data_ptr() % 32 == BASE_OFFSET, "a guarded window must not start on a 32-byte boundary"
    return g


def G(data, dtype, ld=None):
    """A guarded INPUT holding `data` (rounded to dtype)."""
    return _window(tuple(data.shape), dtype, ld).load(data.to(DEV))


def O(shape, dtype, ld=None):
    """A guarded OUTPUT window."""
    return _window(shape, dtype, ld)


class Out:
    """An output of a case: its window is blanked (sentinel NaNs) before every run, or reloaded with `init` (in/out
    operands, zero-filled buffers).  finite = every element must have been written with a finite value; same = the three
    runs must agree bit for bit (off only where the contents legitimately depend on timing)."""

    def __init__(self, g, init=None, finite=True, same=True):
        self.g, self.init, self.finite, self.same = g, init, finite, same


def sweep(what, ins, outs, call):
    """Steps (a) and (b): three runs with everything outside the windows zero / NaN / huge, guards checked after each,
    results compared bit for bit.  Returns the output windows of the "nan" run (clones)."""
    outs = [o if isinstance(o, Out) else Out(o) for o in outs]
    res = {}
    for kind in KINDS:
        for g in ins:
            g.poison(kind)
        for o in outs:
            o.g.poison(kind)
            if o.init is None:
                o.g.blank()
            else:
                o.g.load(o.init)
        call()
        torch.cuda.synchronize()
        for i, g in enumerate(ins):
            g.assert_intact(f"{what} [{kind}] input {i}")
        for i, o in enumerate(outs):
            o.g.assert_intact(f"{what} [{kind}] output {i}")
        res[kind] = [o.g.view.clone() for o in outs]
    for i, o in enumerate(outs):
        if o.same:
            assert_same_bits(res["zero"][i], res["nan"][i], f"{what}: output {i}, outside zero vs NaN")
            assert_same_bits(res["huge"][i], res["nan"][i], f"{what}: output {i}, outside huge vs NaN")
        if o.finite and res["nan"][i].is_floating_point():
            for kind in KINDS:
                assert torch.isfinite(res[kind][i].float()).all(), f"{what} [{kind}]: output {i} is not finite everywhere"
    return res["nan"]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch_gemm(ops, p, expect):
    """One vx_gemm launch of raw parameters through the wrappers' own launcher; the kernel the profile names must
    contain `expect`."""
    with ops.GemmProfile() as prof:
        ops._launch_gemm(p, "vx_gemm")
    name = prof.records[0][3]
    assert expect in name, f"expected a {expect} launch, got {name}"
    return name


def store_params(mods, ops, a, w, geom=None, a2=None, **fields):
    L, _ = mods
    p, _ = ops._base_params(a, w, geom, a2)
    p.epi, p.alpha = L.VX_EPI_STORE, 1.0
    for k, v in fields.items():
        setattr(p, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return p


def conv_ref(x_nhwc, w_oihw, bias, stride, pad, upsample):
    x = x_nhwc.float().permute(0, 3, 1, 2)
    if upsample:
        x = F.interpolate(x, scale_factor=2.0, mode="nearest")
    return F.conv2d(x, w_oihw.float(), bias, stride=stride, padding=pad).permute(0, 2, 3, 1)


def w2d_of(wt):
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], -1).contiguous()


# ----------------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("m,n,k", [(131, 72, 72), (2, 8, 64), (257, 328, 128)])
def test_gemm_classic(ops_el, m, n, k):
    """Classic tiles: clamped rows beyond M, the K tail, N = 8 and N that is no tile multiple; A a strided view
    (lda = k + 8), out with ldc = n + 8 and the residual aliasing it; then the float32 output."""
    ops, el, tol = ops_el
    a, w, bias = G(rnd(m, k), el, ld=k + 8), G(rnd(n, k, scale=k ** -0.5, seed=1), el), G(rnd(n, seed=2), F32)
    res = rnd(m, n, seed=3).to(el)
    out = O((m, n), el, ld=n + 8)
    names = []

    def run():
        with ops.GemmProfile() as prof:
            ops.gemm(a.view, w.view, bias.view, residual=out.view, out=out.view)
        names.append(prof.records[0][3])
    got, = sweep(f"gemm {m}x{n}x{k} in place", [a, w, bias], [Out(out, init=res)], run)
    assert len(set(names)) == 1 and names[0].startswith("gemm_kernel<"), names
    ref = a.view.float() @ w.view.float().t() + bias.view
    check(got, res.to(DEV).float() + ref, f"gemm {m}x{n}x{k} in-place residual, strided A", tol=tol)
    out32 = O((m, n), F32, ld=n + 8)
    got, = sweep(f"gemm {m}x{n}x{k} f32", [a, w, bias], [out32],
                 lambda: ops.gemm(a.view, w.view, bias.view, out=out32.view, out_f32=True))
    check(got, ref, f"gemm {m}x{n}x{k} f32-out", rel=1e-4, mx=1e-4, tol=tol)


def test_gemm_split_k(mods, ops_el):
    """The 8x8 shape of tests/test_gpu_kernels.py::test_gemm_split_k, the slices' workspace at exactly
    vx_gemm_splitk_ws_bytes and the factor ops._splitk picks for it (8)."""
    L, _ = mods
    ops, el, tol = ops_el
    nb, H, W, cin, cout, s = 6, 8, 8, 320, 320, 8
    x = rnd(nb, H + 2, W + 2, cin)
    wt = rnd(cout, cin, 3, 3, scale=(9 * cin) ** -0.5, seed=1)
    a, w, bias = G(x.view(-1, cin), el, ld=cin + 8), G(w2d_of(wt), el), G(rnd(cout, seed=2), F32)
    m = nb * H * W
    res = G(rnd(m, cout, seed=3), el, ld=cout + 8)
    nbytes = int(L.current().vx_gemm_splitk_ws_bytes(m, cout, s))
    assert nbytes == s * m * cout * 4
    ws = O((s * m, cout), F32)
    out = O((m, cout), el, ld=cout + 8)
    g = ops.ConvGeom(nb, H + 2, W + 2, 3, 3, 1, 0)
    p = store_params(mods, ops, a.view, w.view, g, bias=bias.view, residual=res.view, ldr=res.ld, out=out.view, ldc=out.ld,
                     alpha=0.9, act=L.VX_ACT_SILU, splitk=s, splitk_ws=ws.view, ring_hint=-1)
    got, _ = sweep("split-K conv", [a, w, bias, res], [out, Out(ws, finite=False)], lambda: launch_gemm(ops, p, "splitk8"))
    ref = F.silu(conv_ref(a.view.reshape(nb, H + 2, W + 2, cin), w.view.reshape(cout, 3, 3, cin).permute(0, 3, 1, 2),
                          bias.view, 1, 0, 0)).reshape(m, cout) * 0.9 + res.view.float()
    check(got, ref, "split-K conv + silu + residual", tol=tol)


@pytest.mark.parametrize("nb,h,w,c1,c2,cout,stride,ups,split", [(2, 7, 9, 64, 0, 64, 1, 0, 0), (2, 16, 12, 320, 0, 64, 2, 0, 8),
                                                                (2, 8, 8, 128, 0, 160, 1, 1, 0), (2, 8, 8, 128, 64, 160, 1, 0, 0)])
def test_conv3x3(mods, ops_el, nb, h, w, c1, c2, cout, stride, ups, split):
    """3x3 convolutions on the gather path (taps outside the image are zero-filled, never read): pad 1 at 7x9, stride 2
    at 16x12, the fused nearest-2x upsampling at 8x8, two channel-concatenated sources.  The launch is the one ops.gemm
    issues (ops._splitk decides the factor): the stride-2 case (48 output pixels per frame, K = 2880) is split eight ways,
    so its slices' workspace - which the wrapper would take from its own cache - is a guarded window of exactly
    vx_gemm_splitk_ws_bytes; the kernel of every case is pinned by name."""
    L, _ = mods
    ops, el, tol = ops_el
    cin = c1 + c2
    x = rnd(nb, h, w, cin)
    wt = rnd(cout, cin, 3, 3, scale=(9 * cin) ** -0.5, seed=1)
    a = G(x[..., :c1].reshape(-1, c1), el, ld=c1 + 8)
    a2 = G(x[..., c1:].reshape(-1, c2), el, ld=c2 + 16) if c2 else None
    wg, bias = G(w2d_of(wt), el), G(rnd(cout, seed=2), F32)
    g = ops.ConvGeom(nb, h, w, 3, 3, stride, 1, ups)
    out = O((g.m, cout), el, ld=cout + 8)
    ins = [a, wg, bias] + ([a2] if c2 else [])
    p = store_params(mods, ops, a.view, wg.view, g, a2.view if c2 else None, bias=bias.view, out=out.view, ldc=out.ld)
    ops._splitk(p, g, a.view.device, False)
    p.ring_hint = ops._ring_hint(p)
    assert p.splitk == split, f"ops._splitk chose {p.splitk}"
    outs, names = [out], []
    if split:
        ws = O((int(L.current().vx_gemm_splitk_ws_bytes(g.m, cout, split)) // (4 * cout), cout), F32)
        assert ws.view.numel() == split * g.m * cout
        p.splitk_ws = ws.view.data_ptr()
        outs.append(Out(ws, finite=False))
    got = sweep(f"conv3x3 s{stride} ups{ups} {c1}+{c2}", ins, outs, lambda: names.append(launch_gemm(ops, p, "gemm_kernel<")))[0]
    assert len(set(names)) == 1 and names[0].endswith(",gather,splitk8>" if split else ",gather>"), names
    xin = torch.cat([a.view, a2.view], -1) if c2 else a.view
    ref = conv_ref(xin.reshape(nb, h, w, cin), wg.view.reshape(cout, 3, 3, cin).permute(0, 3, 1, 2), bias.view, stride, 1, ups)
    check(got.reshape(ref.shape), ref, f"conv k3 s{stride} ups{ups} {cin}->{cout}", tol=tol)


def test_gemm_persistent_store_and_geglu(mods, ops_el):
    """The persistent 256 x 320 kernel at ONE tile (ring_hint = 1; m = 256, n = 320 is the smallest launch the profile
    shows on it): the STORE epilogue in place (16-byte permlane stores into ldc = n + 8) and GEGLU."""
    L, _ = mods
    ops, el, tol = ops_el
    from v_express_amd import weights as Wt
    m, n, k = 256, 320, 128
    a, w, bias = G(rnd(m, k), el, ld=k + 8), G(rnd(n, k, scale=k ** -0.5, seed=1), el), G(rnd(n, seed=2), F32)
    res = rnd(m, n, seed=3).to(el)
    out = O((m, n), el, ld=n + 8)
    p = store_params(mods, ops, a.view, w.view, bias=bias.view, residual=out.view, ldr=out.ld, out=out.view, ldc=out.ld,
                     alpha=0.75, ring_hint=1)
    got, = sweep("persistent STORE in place", [a, w, bias], [Out(out, init=res)], lambda: launch_gemm(ops, p, "gemm_ring"))
    check(got, res.to(DEV).float() + 0.75 * (a.view.float() @ w.view.float().t() + bias.view), "ring gemm in place", tol=tol)
    n2 = 640                                       # value | gate -> 320 output columns
    wv, bv = rnd(n2, k, scale=k ** -0.5, seed=4), rnd(n2, seed=5)
    wi, bi = G(Wt.geglu_interleave(wv), el), G(Wt.geglu_interleave(bv), F32)
    og = O((m, n2 // 2), el, ld=n2 // 2 + 8)
    pg, _ = ops._base_params(a.view, wi.view, None)
    pg.epi, pg.bias, pg.out, pg.ldc, pg.ring_hint = L.VX_EPI_GEGLU, bi.view.data_ptr(), og.view.data_ptr(), og.ld, 1
    got, = sweep("persistent GEGLU", [a, wi, bi], [og], lambda: launch_gemm(ops, pg, "gemm_ring"))
    hg = a.view.float() @ wv.to(el).to(DEV).float().t() + bv.to(DEV)
    hval, gate = hg.chunk(2, dim=-1)
    check(got, hval * F.gelu(gate), "ring geglu", tol=tol)


@pytest.mark.parametrize("cout,parts", [(320, 0), (640, 2)])
def test_gemm_persistent_conv_rowbias_stats(mods, ops_el, cout, parts):
    """The persistent kernel's 3x3 convolution over a zero-bordered image with the time-embedding rows and the row
    statistics of the stored output: [m, 2] from one tile's registers (n = 320), [m, 4] two-part sums (n = 640)."""
    ops, el, tol = ops_el
    nb, hh, ww, cin = 2, 16, 16, 64
    m = nb * hh * ww
    img = torch.zeros(nb, hh + 2, ww + 2, cin)
    img[:, 1:-1, 1:-1] = rnd(nb, hh, ww, cin)
    wt = rnd(cout, cin, 3, 3, scale=(9 * cin) ** -0.5, seed=1)
    a, w, bias = G(img.view(-1, cin), el, ld=cin + 8), G(w2d_of(wt), el), G(rnd(cout, seed=2), F32)
    rowbias = G(rnd(nb, cout, seed=5), F32, ld=cout + 4)
    out, st = O((m, cout), el, ld=cout + 8), O((m, 4 if parts else 2), F32)
    g = ops.ConvGeom(nb, hh + 2, ww + 2, 3, 3, 1, 0)
    p = store_params(mods, ops, a.view, w.view, g, bias=bias.view, rowbias=rowbias.view, rowbias_ld=rowbias.ld,
                     rows_per_group=hh * ww, out=out.view, ldc=out.ld, ring_hint=1, row_stats_out=st.view,
                     row_stats_eps=1e-5, row_stats_parts=parts)
    got, gst = sweep(f"persistent conv + rowbias + stats[{st.n}]", [a, w, bias, rowbias], [out, st],
                     lambda: launch_gemm(ops, p, "gemm_ring"))
    ref = conv_ref(a.view.reshape(nb, hh + 2, ww + 2, cin), w.view.reshape(cout, 3, 3, cin).permute(0, 3, 1, 2), bias.view,
                   1, 0, 0).reshape(m, cout) + rowbias.view.repeat_interleave(hh * ww, 0)
    check(got, ref, f"ring conv {cout}", tol=tol)
    x = got.double()
    if parts:       # tests/test_gpu_kernels.py::test_gemm_row_stats_two_parts
        h = cout // 2
        want = torch.stack([x[:, :h].sum(1), (x[:, :h] ** 2).sum(1), x[:, h:].sum(1), (x[:, h:] ** 2).sum(1)], dim=1)
        assert torch.allclose(gst.double(), want, rtol=3e-6, atol=2e-3), (gst.double() - want).abs().max()
    else:           # tests/test_gpu_kernels.py::test_gemm_row_stats_out
        assert torch.allclose(gst[:, 0].double(), x.mean(dim=1), rtol=2e-5, atol=2e-6)
        assert torch.allclose(gst[:, 1].double(), torch.rsqrt(x.var(dim=1, unbiased=False) + 1e-5), rtol=1e-4)


def test_gemm_persistent_gn_partial_sums(mods, ops_el):
    """GroupNorm partial sums from the persistent kernel's epilogue, gn_ws at exactly frames * slabs * groups * 2."""
    ops, el, tol = ops_el
    frames, hw, n, k, groups = 2, 256, 320, 128, 32
    m = frames * hw
    a, w, bias = G(rnd(m, k), el, ld=k + 8), G(rnd(n, k, scale=k ** -0.5, seed=1), el), G(rnd(n, seed=2) + 0.7, F32)
    out = O((m, n), el, ld=n + 8)
    p = store_params(mods, ops, a.view, w.view, bias=bias.view, out=out.view, ldc=out.ld, ring_hint=1, gn_groups=groups, gn_hw=hw)
    slabs = int(ops._lib.vx_gemm_gn_slabs(C.byref(p)))
    assert slabs == hw // 128
    ws = O((frames, slabs, groups, 2), F32)
    p.gn_ws = ws.view.data_ptr()
    got, gws = sweep("persistent gn_ws", [a, w, bias], [out, ws], lambda: launch_gemm(ops, p, "gemm_ring"))
    check(got, a.view.float() @ w.view.float().t() + bias.view, "ring gemm with gn_ws", tol=tol)
    x = got.double().view(frames, hw, groups, -1)           # tests/test_gpu_kernels.py::_gn_check
    want = torch.stack([x.sum(dim=(1, 3)), (x * x).sum(dim=(1, 3))], dim=-1)
    assert torch.allclose(gws.double().sum(dim=1), want, rtol=2e-6, atol=1e-3)


def test_gemm_coop_split(mods, ops_el):
    """The cooperative two-way K split at the smallest shape vx_gemm_ring_coop_ok accepts (one 256 x 320 tile, two
    64-channel chunks); the workspace is zeroed inside its window before every launch (epoch 1).  Which half parks its
    accumulators there depends on arrival order, so the workspace's contents are not compared between runs."""
    ops, el, tol = ops_el
    m, n, k = 256, 320, 128
    a, w, bias = G(rnd(m, k), el, ld=k + 8), G(rnd(n, k, scale=k ** -0.5, seed=1), el), G(rnd(n, seed=2), F32)
    out = O((m, n), el, ld=n + 8)
    nbytes = int(ops._lib.vx_gemm_splitk_ws_bytes(m, n, 2))
    ws = O((nbytes // (n * 4), n * 4), torch.uint8)
    assert ws.view.numel() == nbytes
    p = store_params(mods, ops, a.view, w.view, bias=bias.view, out=out.view, ldc=out.ld)
    assert ops._lib.vx_gemm_ring_coop_ok(C.byref(p)) == 1
    for mm, kk in ((128, 128), (256, 64)):                  # and nothing smaller is accepted
        q = store_params(mods, ops, a.view[:mm, :kk], w.view[:, :kk].contiguous(), bias=bias.view, out=out.view, ldc=out.ld)
        assert ops._lib.vx_gemm_ring_coop_ok(C.byref(q)) == 0
    p.ring_hint, p.splitk, p.splitk_ws, p.coop_epoch = 2, 2, ws.view.data_ptr(), 1
    got, _ = sweep("cooperative split", [a, w, bias], [out, Out(ws, init=torch.zeros(ws.shape, dtype=torch.uint8), finite=False,
                                                               same=False)], lambda: launch_gemm(ops, p, "coop2"))
    check(got, a.view.float() @ w.view.float().t() + bias.view, "cooperative split", tol=tol)


def _deq(q8, scale):
    return q8.view(torch.float8_e4m3fn).float() * scale[:, None]


def test_fp8_layernorm_and_gemm(ops_el):
    """vx_layernorm_fp8 (bytes, scales, the zero-filled K padding to 128 - inside the window, as it is the GEMM's K) and
    one fp8 GEMM on the classic 128 x 160 tile fed from those windows.  The fp8 tolerances do not depend on the element type
    (tests/test_gpu_kernels.py::check leaves them alone)."""
    ops, el, tol = ops_el
    rows, c, n = 131, 320, 72
    kp = ops.pad128(c)
    x = G(rnd(rows, c, scale=2.0, seed=7), el, ld=c + 8)
    gam, bet, add = G(1 + 0.1 * rnd(c, seed=1), F32), G(0.1 * rnd(c, seed=2), F32), G(rnd(8, c, seed=3), F32)
    q, sc = O((rows, kp), torch.uint8), O((rows,), F32)
    got_q, got_s = sweep("layernorm_fp8", [x, gam, bet, add], [q, sc], lambda: ops.L.check(
        ops._lib.vx_layernorm_fp8(x.view.data_ptr(), x.ld, rows, c, 1e-5, gam.view.data_ptr(), bet.view.data_ptr(),
                                  add.view.data_ptr(), 16, 8, q.view.data_ptr(), kp, sc.view.data_ptr(), stream()),
        "vx_layernorm_fp8"))
    y = F.layer_norm(x.view.float(), (c,), gam.view, bet.view, 1e-5) + add.view[(torch.arange(rows, device=DEV) // 16) % 8]
    assert (got_q[:, c:] == 0).all(), "K padding must be zero bytes"
    amax = y.abs().amax(dim=1)                               # tests/test_gpu_kernels.py::test_layernorm_fp8
    assert torch.allclose(got_s, amax / 448.0, rtol=2e-3)
    deq = _deq(got_q[:, :c].contiguous(), got_s)
    tolm = y.abs() * 2 ** -4 + got_s[:, None] * 2 ** -6 * 1.01 + 2e-3 * amax[:, None]
    assert ((deq - y).abs() <= tolm).all()
    # the GEMM reads the windows the quantiser has just filled (the last run's contents are still in place; the three runs agreed bit for bit)
    wf = rnd(n, c, scale=c ** -0.5, seed=2).to(el).float()
    wsc = wf.abs().amax(dim=1).clamp_min(1e-30) / 448.0
    w8 = torch.zeros(n, kp, dtype=torch.uint8)
    w8[:, :c] = (wf / wsc[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    w8g, wsg, bias = G(w8, torch.uint8), G(wsc, F32), G(rnd(n, seed=3), F32)
    res = G(rnd(rows, n, seed=4), el, ld=n + 8)
    out = O((rows, n), el, ld=n + 8)
    a8, wt8 = ops.Fp8Rows(q.view, sc.view, c), ops.Fp8Weight(w8g.view, wsg.view, c)
    names = []

    def run():
        with ops.GemmProfile() as prof:
            ops.gemm(a8, wt8, bias.view, residual=res.view, alpha=0.95, out=out.view)
        names.append(prof.records[0][3])
    got, = sweep("fp8 gemm", [q, sc, w8g, wsg, bias, res], [out], run)
    assert all(nm == "gemm_kernel<128x160x128,4w,STORE,fast,fp8>" for nm in names), names
    ref = _deq(q.view, sc.view).double() @ _deq(w8g.view, wsg.view).double().t() + bias.view.double()
    check(got, (res.view.double() + 0.95 * ref).float(), "fp8 gemm store", tol=tol)


@pytest.mark.parametrize("n_tok", [4, 1, 100])
def test_gemm_split_rows_and_vt(ops_el, n_tok):
    """The SPLIT epilogue: Q | K as column slices of ONE wide tensor (row stride 2c + 8), V^T into a buffer whose pitch
    pads the key axis - the padding is the caller's zero (ops.alloc_vt), inside the window, and must still be zero."""
    ops, el, tol = ops_el
    seqs, c, heads = 3, 64, 8
    m, d = seqs * n_tok, c // heads
    a, w, bias = G(rnd(m, c), el, ld=c + 8), G(rnd(3 * c, c, scale=c ** -0.5, seed=1), el), G(rnd(3 * c, seed=2), F32)
    wide = O((m, 2 * c), el, ld=2 * c + 8)
    pitch = ops.vt_pitch(n_tok)
    vt = O((seqs, heads, d, pitch), el)
    qk, gvt = sweep(f"gemm_split n_tok={n_tok}", [a, w, bias], [wide, Out(vt, init=torch.zeros(vt.shape))],
                    lambda: ops.gemm_split(a.view, w.view, bias.view, [("rows", wide.view[:, :c]), ("rows", wide.view[:, c:]),
                                                                      ("vt", vt.view)], part_cols=c, seq_len=n_tok, head_dim=d))
    ref = a.view.float() @ w.view.float().t() + bias.view
    check(qk, ref[:, :2 * c], "split Q | K", tol=tol)
    check(gvt[..., :n_tok], ref[:, 2 * c:].view(seqs, n_tok, heads, d).permute(0, 2, 3, 1), f"split V^T seq_len={n_tok}", tol=tol)
    assert (gvt[..., n_tok:].view(torch.int16) == 0).all(), "the V^T pitch padding must stay zero"


# ----------------------------------------------------------------------------------------------------- one-launch blocks
def test_ff_fused(mods, ops):
    """vx_ff_pack_weights + vx_ff_fused at one 128-row tile: residual stream in place (ldx = 328), statistics in, packed
    weights out of the pack launch and into the block."""
    L, _ = mods
    el = torch.bfloat16
    m, c, hidden = 128, 320, 1280
    assert ops.ff_fused_applies(m, c, hidden) and not ops.ff_fused_applies(m - 64, c, hidden)
    x0 = (rnd(m, c) * 1.5 + 0.3).to(el)
    w1, w2 = G(rnd(2 * hidden, c, scale=c ** -0.5, seed=1), el), G(rnd(c, hidden, scale=hidden ** -0.5, seed=2), el)
    b1, b2 = G(rnd(2 * hidden, seed=3) * 0.3, F32), G(rnd(c, seed=4) * 0.3, F32)
    w1t, w2t = O((2 * hidden, c), el), O((c, hidden), el)
    sweep("ff pack", [w1, w2], [Out(w1t, finite=False), Out(w2t, finite=False)], lambda: L.check(ops._lib.vx_ff_pack_weights(
        w1.view.data_ptr(), w2.view.data_ptr(), w1t.view.data_ptr(), w2t.view.data_ptr(), c, hidden, stream()), "vx_ff_pack_weights"))
    colsum = G(w1.view.float().sum(1).cpu(), F32)
    xf = x0.float()
    st = G(torch.stack([xf.mean(1), torch.rsqrt(xf.var(1, unbiased=False) + 1e-5)], 1), F32)
    x = O((m, c), el, ld=c + 8)
    p = L.FfParams()
    p.x, p.ldx, p.m, p.c, p.hidden = x.view.data_ptr(), x.ld, m, c, hidden
    p.w1t, p.w2t, p.bias1, p.bias2 = w1t.view.data_ptr(), w2t.view.data_ptr(), b1.view.data_ptr(), b2.view.data_ptr()
    p.ln_colsum, p.ln_stats = colsum.view.data_ptr(), st.view.data_ptr()
    p.residual, p.ldr, p.out, p.ldo = x.view.data_ptr(), x.ld, x.view.data_ptr(), x.ld
    got, = sweep("ff_fused", [w1t, w2t, b1, b2, colsum, st], [Out(x, init=x0)],
                 lambda: L.check(ops._lib.vx_ff_fused(C.byref(p), stream()), "vx_ff_fused"))
    xf = xf.to(DEV)                                          # tests/test_gpu_kernels.py::test_ff_fused_prototype_...
    ln = (xf - xf.mean(1, keepdim=True)) * torch.rsqrt(xf.var(1, unbiased=False, keepdim=True) + 1e-5)
    pp = (ln @ w1.view.float().t() + b1.view).view(m, 2 * hidden // 16, 2, 8)
    h = (pp[:, :, 0] * F.gelu(pp[:, :, 1])).reshape(m, hidden)
    check(got, xf + h.to(el).float() @ w2.view.float().t() + b2.view, "ff_fused vs float32", rel=8e-3)


@pytest.mark.parametrize("f,hw", [(16, 8), (24, 4)])
def test_tblock_fused(mods, ops, f, hw):
    """vx_tblock_pack + vx_tblock_fused at one tile (8 pixels x 16 frames / 4 pixels x 24 frames): residual stream in
    place, statistics in and out, the packed weights and tables."""
    L, _ = mods
    el = torch.bfloat16
    c, heads, b = 320, 8, 1
    d, m = c // heads, b * f * hw
    assert ops.tblock_fused_applies(c, heads, f, hw) and not ops.tblock_fused_applies(c, heads, f, hw // 2)
    x0 = (rnd(m, c) * 1.5 + 0.3).to(el)
    wqkv, wo = G(rnd(3 * c, c, scale=c ** -0.5, seed=1), el), G(rnd(c, c, scale=c ** -0.5, seed=2), el)
    bq, bo = G(rnd(3 * c, seed=3) * 0.2, F32), G(rnd(c, seed=4) * 0.2, F32)
    pe = G(rnd(f, 3 * c, seed=5) * 0.5, F32, ld=3 * c + 4)
    colsum = G(wqkv.view.float().sum(1).cpu(), F32)
    nb = int(ops._lib.vx_tblock_packed_bytes(f))
    wqkv_t, wo_t, cs = O((32, nb // 64), el), O((c, c), el), O((1024,), F32)
    assert wo_t.view.numel() * 2 == 204800
    sweep("tblock pack", [wqkv, wo, bq, pe, colsum], [Out(wqkv_t, finite=False), Out(wo_t, finite=False), Out(cs, finite=False)], lambda: L.check(ops._lib.vx_tblock_pack(
        wqkv.view.data_ptr(), bq.view.data_ptr(), colsum.view.data_ptr(), pe.view.data_ptr(), pe.ld, wo.view.data_ptr(),
        wqkv_t.view.data_ptr(), wo_t.view.data_ptr(), cs.view.data_ptr(), c, heads, f, stream()), "vx_tblock_pack"))
    xf = x0.float()
    st = G(torch.stack([xf.mean(1), torch.rsqrt(xf.var(1, unbiased=False) + 1e-5)], 1), F32)
    x, so = O((m, c), el, ld=c + 8), O((m, 2), F32)
    p = L.TBlockParams()
    p.x, p.ldx, p.b, p.f, p.hw, p.c, p.heads = x.view.data_ptr(), x.ld, b, f, hw, c, heads
    p.wqkv_t, p.wo_t, p.colsum_p, p.bias_o = wqkv_t.view.data_ptr(), wo_t.view.data_ptr(), cs.view.data_ptr(), bo.view.data_ptr()
    p.ln_stats, p.stats_out, p.ln_eps, p.scale = st.view.data_ptr(), so.view.data_ptr(), 1e-5, d ** -0.5
    got, gso = sweep(f"tblock_fused f={f}", [wqkv_t, wo_t, cs, bo, st], [Out(x, init=x0), so],
                     lambda: L.check(ops._lib.vx_tblock_fused(C.byref(p), stream()), "vx_tblock_fused"))
    xf = xf.to(DEV)                                          # tests/test_gpu_kernels.py::test_tblock_fused_matches_...
    ln = (xf - xf.mean(1, keepdim=True)) * torch.rsqrt(xf.var(1, unbiased=False, keepdim=True) + 1e-5)
    q3 = ln @ wqkv.view.float().t() + bq.view + pe.view.repeat(b, 1).repeat_interleave(hw, dim=0)
    qq, kk, vv = (t.reshape(b, f, hw, heads, d).permute(0, 2, 3, 1, 4) for t in q3.to(el).float().chunk(3, dim=-1))
    o = F.scaled_dot_product_attention(qq, kk, vv).permute(0, 3, 1, 2, 4).reshape(m, c)
    check(got, xf + o.to(el).float() @ wo.view.float().t() + bo.view, f"tblock_fused f={f} vs float32", rel=8e-3)
    g64 = got.double()
    assert torch.allclose(gso[:, 0].double(), g64.mean(dim=1), rtol=2e-5, atol=2e-6)
    assert torch.allclose(gso[:, 1].double(), torch.rsqrt(g64.var(dim=1, unbiased=False) + 1e-5), rtol=1e-4)


def test_audio_xattn(mods, ops):
    """vx_audio_xattn_pack + vx_audio_xattn at two frames of one 16-row wave each: K | V rows with ldkv = 2c + 8, the four
    packed operands, the residual stream read with ldx = c + 8 and written with ldo = c + 16, statistics in and out."""
    L, _ = mods
    from v_express_amd import weights
    el = torch.bfloat16
    frames, hw, c, heads, n_ctx, alpha = 2, 16, 320, 8, 5, 3.0
    d, m = c // heads, frames * hw
    assert ops.audio_xattn_applies(c, heads, n_ctx, hw) and not ops.audio_xattn_applies(c, heads, n_ctx, hw // 2)
    g = torch.Generator().manual_seed(c + hw)
    h0 = (torch.randn(m, c, generator=g) * 1.5 + 0.3).to(el)
    kv = G(torch.randn(frames * n_ctx, 2 * c, generator=g) * 1.2, el, ld=2 * c + 8)
    wq = torch.randn(c, c, generator=g) * c ** -0.5
    wo = G(torch.randn(c, c, generator=g) * c ** -0.5, el)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.2
    bo = G(torch.randn(c, generator=g) * 0.3, F32)
    Fq = weights.fold_layernorm(wq, None, gamma, beta, DEV)
    wqf, bqf = G(Fq.w.cpu(), el), G(Fq.b.cpu(), F32)
    assert int(ops._lib.vx_audio_xattn_packed_bytes(c, frames)) // 2 <= frames * 48 * c * 2      # what each packed operand holds
    kq, vo, cs, sb = O((frames, 48 * c), el), O((frames, 48 * c), el), O((frames, 48), F32), O((frames, 48), F32)
    sweep("audio_xattn pack", [kv, wqf, bqf, wo], [Out(t_, finite=False) for t_ in (kq, vo, cs, sb)], lambda: L.check(ops._lib.vx_audio_xattn_pack(
        kv.view.data_ptr(), kv.ld, wqf.view.data_ptr(), bqf.view.data_ptr(), wo.view.data_ptr(), c, heads, n_ctx, frames,
        kq.view.data_ptr(), cs.view.data_ptr(), sb.view.data_ptr(), vo.view.data_ptr(), stream()), "vx_audio_xattn_pack"))
    hf = h0.float()
    st = G(torch.stack([hf.mean(1), torch.rsqrt(hf.var(1, unbiased=False) + 1e-5)], 1), F32)
    h, out, so = G(h0, el, ld=c + 8), O((m, c), el, ld=c + 16), O((m, 2), F32)
    fold = ops.AudioFold(kq.view, cs.view, sb.view, vo.view, frames, c)
    got, gso = sweep("audio_xattn", [h, st, kq, vo, cs, sb, bo], [out, so], lambda: ops.audio_xattn(
        h.view, st.view, fold, bo.view, alpha, rows_per_frame=hw, stats_out=so.view, out=out.view))
    x = h.view.float()                                       # tests/test_gpu_kernels.py::test_audio_xattn_one_launch
    ln = F.layer_norm(x, (c,), gamma.to(DEV), beta.to(DEV), 1e-5)
    q = (ln @ wq.to(DEV).t()).view(frames, hw, heads, d).transpose(1, 2)
    k = kv.view[:, :c].float().reshape(frames, n_ctx, heads, d).transpose(1, 2)
    v = kv.view[:, c:].float().reshape(frames, n_ctx, heads, d).transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, dim=-1) @ v
    ref = x + alpha * (a.transpose(1, 2).reshape(m, c) @ wo.view.float().t() + bo.view)
    check(got, ref, "audio_xattn", rel=8e-3, mx=2 ** -6)
    check(got.float() - x, ref - x, "audio_xattn increment", rel=2.5e-2, mx=2 ** -4)
    o = got.float()
    assert torch.allclose(gso[:, 0], o.mean(1), rtol=1e-4, atol=1e-4)
    assert torch.allclose(gso[:, 1], (o.var(1, unbiased=False) + 1e-5).rsqrt(), rtol=2e-3)


# ----------------------------------------------------------------------------------------------------- normalisation
def _gn_ref(x, groups, gamma, beta, silu):
    ref = F.group_norm(x.float().permute(0, 2, 1), groups, gamma, beta, 1e-5).permute(0, 2, 1)
    return F.silu(ref) if silu else ref


@pytest.mark.parametrize("frames,hw,c1,c2,groups,pad_hw", [(3, 72, 64, 0, 32, None), (2, 128, 128, 64, 32, None),
                                                           (2, 72, 64, 0, 32, (6, 12))])
def test_groupnorm(ops_el, frames, hw, c1, c2, groups, pad_hw):
    """vx_groupnorm with its workspace at exactly vx_groupnorm_ws_floats: hw = 72 (ragged slices), two sources, and the
    padded-output form at 6 x 12 - the border of the image is the caller's zero: inside the window, zero before and after."""
    ops, el, tol = ops_el
    L = ops.L
    c = c1 + c2
    x1 = G(rnd(frames, hw, c1, scale=2.0) + 0.7, el)
    x2 = G(rnd(frames, hw, c2, seed=5), el) if c2 else None
    gam, bet = G(rnd(c, seed=1) * 0.1 + 1, F32), G(rnd(c, seed=2) * 0.1, F32)
    slices = ops._gn_slices(hw)
    ws = O((int(ops._lib.vx_groupnorm_ws_floats(frames, slices, groups)),), F32)
    H, W = pad_hw or (1, hw)
    out = O((frames, (H + 2) * (W + 2), c), el) if pad_hw else O((frames, hw, c), el)
    width, pad = (W, 1) if pad_hw else (hw, 0)
    ins = [x1, gam, bet] + ([x2] if c2 else [])
    got, _ = sweep(f"groupnorm {frames}x{hw}x{c1}+{c2} pad={pad}", ins,
                   [Out(out, init=torch.zeros(out.shape)) if pad_hw else out, Out(ws, finite=False)],
                   lambda: L.check(ops._lib.vx_groupnorm(x1.view.data_ptr(), c1, x2.view.data_ptr() if c2 else None, c2, frames, hw,
                                                         groups, 1e-5, gam.view.data_ptr(), bet.view.data_ptr(), 1, out.view.data_ptr(),
                                                         ws.view.data_ptr(), slices, width, pad, stream()), "vx_groupnorm"))
    x = torch.cat([x1.view, x2.view], -1) if c2 else x1.view
    ref = _gn_ref(x, groups, gam.view, bet.view, True)
    if pad_hw:
        img = got.view(frames, H + 2, W + 2, c)
        border = img.clone()
        border[:, 1:-1, 1:-1] = 0
        assert (border.view(torch.int16) == 0).all(), "the zero border of the padded image was written"
        got = img[:, 1:-1, 1:-1].reshape(frames, hw, c)
    check(got, ref, f"groupnorm C={c} hw={hw}", rel=8e-3, mx=2 ** -6, tol=tol)


def test_groupnorm_stats_apply_fold(ops_el):
    """vx_groupnorm_stats -> vx_groupnorm_apply (the bits of vx_groupnorm) and -> vx_groupnorm_fold_linear, the workspace
    a guarded output of the first and a guarded input of the other two."""
    ops, el, tol = ops_el
    L = ops.L
    frames, hw, c, groups, n, eps = 3, 72, 64, 32, 72, 1e-5
    x = G(rnd(frames, hw, c, scale=2.0) + 0.7, el)
    gam, bet = G(rnd(c, seed=1) * 0.1 + 1, F32), G(rnd(c, seed=2) * 0.1, F32)
    slices = ops._gn_slices(hw)
    ws = O((int(ops._lib.vx_groupnorm_ws_floats(frames, slices, groups)),), F32)
    sweep("groupnorm_stats", [x], [Out(ws, finite=False)], lambda: L.check(ops._lib.vx_groupnorm_stats(
        x.view.data_ptr(), c, None, 0, frames, hw, groups, ws.view.data_ptr(), slices, stream()), "vx_groupnorm_stats"))
    out = O((frames, hw, c), el)
    got, = sweep("groupnorm_apply", [x, gam, bet, ws], [out], lambda: L.check(ops._lib.vx_groupnorm_apply(
        x.view.data_ptr(), c, None, 0, frames, hw, groups, eps, gam.view.data_ptr(), bet.view.data_ptr(), 1, out.view.data_ptr(),
        ws.view.data_ptr(), slices, slices, hw, 0, stream()), "vx_groupnorm_apply"))
    check(got, _gn_ref(x.view, groups, gam.view, bet.view, True), "groupnorm_apply", rel=8e-3, mx=2 ** -6, tol=tol)
    assert_same_bits(got, ops.groupnorm(x.view, gam.view, bet.view, frames=frames, hw=hw, groups=groups, eps=eps, silu=True),
                     "stats + apply vs vx_groupnorm")
    w, bb = G(rnd(n, c, scale=c ** -0.5, seed=3), el), G(rnd(n, seed=4), F32)
    w_f, b_f = O((frames, n, c), el), O((frames, n), F32)
    gw, gb = sweep("groupnorm_fold_linear", [ws, gam, w, bb], [w_f, b_f], lambda: L.check(ops._lib.vx_groupnorm_fold_linear(
        ws.view.data_ptr(), frames, hw, slices, groups, eps, gam.view.data_ptr(), c, w.view.data_ptr(), bb.view.data_ptr(), n,
        w_f.view.data_ptr(), b_f.view.data_ptr(), stream()), "vx_groupnorm_fold_linear"))
    xf = x.view.float().view(frames, hw, groups, c // groups)
    mean = xf.mean(dim=(1, 3)).repeat_interleave(c // groups, dim=1)
    rstd = torch.rsqrt(xf.var(dim=(1, 3), unbiased=False) + eps).repeat_interleave(c // groups, dim=1)
    # tests/test_gpu_kernels.py::test_groupnorm_folded_into_linear: one rounding of w * gamma * rstd
    check(gw, w.view.float()[None] * (gam.view[None] * rstd)[:, None, :], "per-frame folded weights", rel=4e-3, mx=2 ** -8, tol=tol)
    # the bias row is the header's float32 expression over the STORED weights: c = 64 products summed in float32, each within
    # 2^-24 relative, and a mean taken from float32 partial sums - 1e-5 of the largest magnitude involved covers both
    want = bb.view[None] - (gw.float() * mean[:, None, :]).sum(-1)
    bound = 1e-5 * max(1.0, (gw.float().abs() * mean.abs()[:, None, :]).sum(-1).max().item())
    assert (gb - want).abs().max().item() <= bound, ((gb - want).abs().max().item(), bound)


@pytest.mark.parametrize("rows", [33, 257])
def test_layernorm(ops, rows):
    el = torch.bfloat16
    c, hw, f = 320, 8, 4
    x = G(rnd(rows, c, scale=1.5) + 0.3, el, ld=c + 8)
    gam, bet, pe = G(rnd(c, seed=1) * 0.1 + 1, F32), G(rnd(c, seed=2) * 0.1, F32), G(rnd(f, c, seed=3), F32)
    out = O((rows, c), el, ld=c + 16)
    got, = sweep(f"layernorm rows={rows}", [x, gam, bet, pe], [out], lambda: ops.layernorm(
        x.view, gam.view, bet.view, add=pe.view, add_rows_per_entry=hw, add_entries=f, out=out.view))
    ref = F.layer_norm(x.view.float(), (c,), gam.view, bet.view, 1e-5) + pe.view[(torch.arange(rows, device=DEV) // hw) % f]
    check(got, ref, "layernorm + positional table")


def test_row_stats(ops):
    el = torch.bfloat16
    L = ops.L
    rows, c = 257, 640
    x = G(rnd(rows, c, seed=c) * 1.5 + 0.7, el, ld=c + 8)
    st2, st4, fin = O((rows, 2), F32), O((rows, 4), F32), O((rows, 2), F32)
    g2, = sweep("row_stats", [x], [st2], lambda: ops.row_stats(x.view, 1e-5, out=st2.view))
    g4, = sweep("row_stats_parts", [x], [st4], lambda: ops.row_stats(x.view, 1e-5, out=st4.view))
    xf = x.view.float()                                      # tests/test_gpu_kernels.py::test_row_stats
    assert torch.allclose(g2[:, 0], xf.mean(dim=1), rtol=1e-5, atol=1e-6)
    assert torch.allclose(g2[:, 1], torch.rsqrt(xf.var(dim=1, unbiased=False) + 1e-5), rtol=1e-5)
    x64, h = xf.double(), c // 2                             # ::test_gemm_row_stats_two_parts
    want = torch.stack([x64[:, :h].sum(1), (x64[:, :h] ** 2).sum(1), x64[:, h:].sum(1), (x64[:, h:] ** 2).sum(1)], dim=1)
    assert torch.allclose(g4.double(), want, rtol=3e-6, atol=2e-3)
    gf, = sweep("row_stats_finalize", [st4], [fin], lambda: L.check(ops._lib.vx_row_stats_finalize(
        st4.view.data_ptr(), rows, c, 1e-5, fin.view.data_ptr(), stream()), "vx_row_stats_finalize"))
    # one-pass variance from the two-part sums (header: rstd within 1e-4 of float64 for |mean| / std <= 2.5)
    assert torch.allclose(gf[:, 0].double(), x64.mean(1), rtol=2e-5, atol=2e-6)
    assert torch.allclose(gf[:, 1].double(), torch.rsqrt(x64.var(1, unbiased=False) + 1e-5), rtol=1e-4)


# ----------------------------------------------------------------------------------------------------- attention
def _sdpa(q, k, v):
    return F.scaled_dot_product_attention(q.float(), k.float(), v.float())


def _attn_problem(ops, el, batch, kvb, heads, n_q, n_kv, d):
    c = heads * d
    q, k = G(rnd(batch * n_q, c), el, ld=c + 8), G(rnd(kvb * n_kv, c, seed=1), el, ld=c + 16)
    v = rnd(kvb * n_kv, c, seed=2)
    vt0 = torch.zeros(kvb, heads, d, ops.vt_pitch(n_kv))
    vt0[..., :n_kv] = v.view(kvb, n_kv, heads, d).permute(0, 2, 3, 1)
    vt = G(vt0, el)
    out = O((batch * n_q, c), el, ld=c + 8)
    rep = batch // kvb
    vv = vt.view[..., :n_kv].permute(0, 3, 1, 2).reshape(kvb, n_kv, heads, d)
    ref = _sdpa(q.view.reshape(batch, n_q, heads, d).transpose(1, 2),
                k.view.reshape(kvb, n_kv, heads, d).transpose(1, 2).repeat_interleave(rep, 0),
                vv.transpose(1, 2).repeat_interleave(rep, 0)).transpose(1, 2).reshape(batch * n_q, c)
    return q, k, vt, out, ref


@pytest.mark.parametrize("n_q,n_kv", [(100, 100), (65, 5), (1, 1)])
@pytest.mark.parametrize("d", [8, 16, 40, 80, 160])
def test_flash_attention(ops_el, d, n_q, n_kv):
    """vx_attention: ragged last query / key tiles, one key, q / k / out with row strides above the width, two query
    batches per key batch; the V^T padding between n_kv and the pitch is the caller's zero and part of the window.
    d = 40 with the bounded softmax off (ops._BOUNDED_SOFTMAX): the exact kernel."""
    ops, el, tol = ops_el
    batch, kvb, heads = 2, 1, 8
    q, k, vt, out, ref = _attn_problem(ops, el, batch, kvb, heads, n_q, n_kv, d)
    saved = ops._BOUNDED_SOFTMAX[0]
    try:
        ops._BOUNDED_SOFTMAX[0] = False
        got, = sweep(f"attention d={d} {n_q}x{n_kv}", [q, k, vt], [out], lambda: ops.attention(
            q.view, k.view, vt.view, batch=batch, heads=heads, n_q=n_q, n_kv=n_kv, head_dim=d, q_per_kv=2, out=out.view))
    finally:
        ops._BOUNDED_SOFTMAX[0] = saved
    assert "attn3" not in ops._lib.vx_last_kernel().decode()
    check(got, ref, f"attention d={d} nq={n_q} nkv={n_kv}", rel=1e-2, mx=2 ** -6, tol=tol)
    assert (vt.view[..., n_kv:].view(torch.int16) == 0).all()


@pytest.mark.parametrize("n_q,n_kv", [(1, 1), (100, 100), (65, 5)])
def test_bounded_attention_and_key_norm_max(ops, n_q, n_kv):
    """vx_key_norm_max into a guarded table, then vx_attention_bounded (d = 40: the attn3 kernel) reading it: one query and
    one key - the smallest it takes - and ragged sizes."""
    el = torch.bfloat16
    L = ops.L
    batch, kvb, heads, d = 2, 1, 8, 40
    q, k, vt, out, ref = _attn_problem(ops, el, batch, kvb, heads, n_q, n_kv, d)
    kmax = O((kvb * heads,), F32)
    gk, = sweep(f"key_norm_max n_kv={n_kv}", [k], [kmax], lambda: L.check(ops._lib.vx_key_norm_max(
        k.view.data_ptr(), k.ld, kvb, heads, n_kv, d, kmax.view.data_ptr(), stream()), "vx_key_norm_max"))
    want = k.view.float().reshape(kvb, n_kv, heads, d).norm(dim=-1).amax(dim=1).reshape(-1)
    assert torch.allclose(gk, want, rtol=1e-5, atol=1e-6)    # tests/test_gpu_kernels.py::test_key_norm_max
    assert ops._BOUNDED_SOFTMAX[0]
    got, = sweep(f"bounded attention {n_q}x{n_kv}", [q, k, vt, kmax], [out], lambda: ops.attention(
        q.view, k.view, vt.view, batch=batch, heads=heads, n_q=n_q, n_kv=n_kv, head_dim=d, q_per_kv=2, out=out.view,
        kmax=kmax.view))
    assert ops._lib.vx_last_kernel().decode().startswith("attn3_kernel<"), ops._lib.vx_last_kernel()
    check(got, ref, f"bounded attention nq={n_q} nkv={n_kv}", rel=1e-2, mx=2 ** -6)


@pytest.mark.parametrize("b,f,hw,heads,d", [(1, 3, 5, 8, 8), (1, 24, 4, 8, 40)])
def test_temporal_attention(ops, b, f, hw, heads, d):
    el = torch.bfloat16
    c = heads * d
    qkv = G(rnd(b * f * hw, 3 * c), el, ld=3 * c + 8)
    out = O((b * f * hw, c), el, ld=c + 4)
    got, = sweep(f"temporal attention f={f} d={d}", [qkv], [out], lambda: ops.temporal_attention(
        qkv.view, b=b, f=f, hw=hw, heads=heads, head_dim=d, out=out.view))
    t = qkv.view.reshape(b, f, hw, 3, heads, d).permute(3, 0, 2, 4, 1, 5)
    ref = _sdpa(t[0], t[1], t[2]).permute(0, 3, 1, 2, 4).reshape(b * f * hw, c)
    check(got, ref, f"temporal attention f={f} d={d}", rel=1e-2, mx=2 ** -6)


@pytest.mark.parametrize("n_kv", [1, 5])
def test_small_kv_attention(ops, n_kv):
    el = torch.bfloat16
    batch, n_q, heads, d = 2, 100, 8, 40
    c = heads * d
    q, kv = G(rnd(batch * n_q, c), el, ld=c + 8), G(rnd(batch * n_kv, 2 * c, seed=1), el, ld=2 * c + 8)
    out = O((batch * n_q, c), el, ld=c + 8)
    got, = sweep(f"small-kv attention n_kv={n_kv}", [q, kv], [out], lambda: ops.small_kv_attention(
        q.view, kv.view, batch=batch, n_q=n_q, n_kv=n_kv, heads=heads, head_dim=d, out=out.view))
    k, v = kv.view[:, :c], kv.view[:, c:]
    ref = _sdpa(q.view.reshape(batch, n_q, heads, d).transpose(1, 2), k.reshape(batch, n_kv, heads, d).transpose(1, 2),
                v.reshape(batch, n_kv, heads, d).transpose(1, 2)).transpose(1, 2).reshape(batch * n_q, c)
    check(got, ref, f"small-kv attention n_kv={n_kv}", rel=1e-2, mx=2 ** -6)


# ----------------------------------------------------------------------------------------------------- elementwise, layout
def test_add_row_bias_and_residual_f32(ops):
    el = torch.bfloat16
    x0 = rnd(50, 640).to(el)
    bias = G(rnd(320, seed=1), F32)
    x = O((50, 640), el, ld=648)
    got, = sweep("add_row_bias on a slice", [bias], [Out(x, init=x0)], lambda: ops.add_row_bias(x.view[:, 320:], bias.view, 0.95))
    ref = x0.to(DEV).float()
    assert_same_bits(got[:, :320], x0.to(DEV)[:, :320], "add_row_bias: the columns left of the slice")
    ref[:, 320:] += 0.95 * bias.view
    check(got, ref, "add_row_bias on a strided view")
    rows, c = 37, 72
    xr, y = G(rnd(rows, c), el, ld=c + 8), G(rnd(rows, c, seed=2), F32, ld=c + 4)
    out = O((rows, c), el, ld=c + 16)
    got, = sweep("add_residual_f32", [xr, y], [out], lambda: ops.add_residual_f32(xr.view, y.view, out=out.view))
    assert_same_bits(got, (xr.view.float() + y.view).to(el), "add_residual_f32: one rounding of the float32 sum")


def test_pad_image_and_pixel_shuffle(ops):
    el = torch.bfloat16
    L = ops.L
    frames, H, W, c = 2, 5, 7, 24
    x = G(rnd(frames, H * W, c), el)
    img = O((frames, (H + 2) * (W + 2), c), el)
    got, = sweep("pad_image", [x], [Out(img, init=torch.zeros(img.shape))], lambda: L.check(ops._lib.vx_pad_image(
        x.view.data_ptr(), frames, H, W, c, img.view.data_ptr(), stream()), "vx_pad_image"))
    want = torch.zeros(frames, H + 2, W + 2, c, device=DEV, dtype=el)
    want[:, 1:-1, 1:-1] = x.view.view(frames, H, W, c)
    assert_same_bits(got.view(frames, H + 2, W + 2, c), want, "pad_image: interior copied, border still zero")
    # four phases with a stride larger than one phase: the gap between them belongs to nobody
    n1 = frames * H * W * c
    stride = n1 + 64
    ph = G(rnd(4, stride), el)
    out = O((frames, 4 * H * W, c), el)
    got, = sweep("pixel_shuffle2x", [ph], [out], lambda: L.check(ops._lib.vx_pixel_shuffle2x(
        ph.view.data_ptr(), stride, frames, H, W, c, out.view.data_ptr(), stream()), "vx_pixel_shuffle2x"))
    p4 = ph.view[:, :n1].reshape(2, 2, frames, H, W, c)     # [a, b, f, y, x, c] -> out[f, 2y + a, 2x + b]
    assert_same_bits(got, p4.permute(2, 3, 0, 4, 1, 5).reshape(frames, 4 * H * W, c), "pixel_shuffle2x")


def test_layout_kernels(ops):
    el = torch.bfloat16
    L = ops.L
    c, Ftot, hw, f, reps, c_pad = 4, 11, 33, 4, 2, 8
    lat = G(rnd(c, Ftot, hw), F32)
    ids = G(torch.tensor([8, 9, 10, 9], dtype=torch.int32), torch.int32)
    out = O((reps * f, hw, c_pad), el)
    got, = sweep("gather_latents", [lat, ids], [out], lambda: L.check(ops._lib.vx_gather_latents(
        lat.view.data_ptr(), c, Ftot, hw, ids.view.data_ptr(), f, reps, c_pad, out.view.data_ptr(), stream()), "vx_gather_latents"))
    ref = lat.view[:, ids.view.long()].permute(1, 2, 0)
    check(got[:f, :, :c], ref, "gather_latents", rel=4e-3, mx=2 ** -8)
    assert torch.equal(got[:f], got[f:]) and (got[..., c:].view(torch.int16) == 0).all()
    # cfg_combine / pack_rows / nhwc_to_ncfhw read float32 rows of stride ld > c
    ld = 12
    uo = G(rnd(2 * f * hw, c), F32, ld=ld)
    slot = O((c, f, hw), F32)
    got, = sweep("cfg_combine", [uo], [slot], lambda: ops.cfg_combine(uo.view, c, f, hw, 3.5, slot.view))
    u, cd = uo.view[:f * hw].reshape(f, hw, c).permute(2, 0, 1), uo.view[f * hw:].reshape(f, hw, c).permute(2, 0, 1)
    check(got, u + 3.5 * (cd - u), "cfg_combine", rel=1e-5, mx=1e-5)
    dst = O((2 * f * hw, c), F32)
    got, = sweep("pack_rows", [uo], [dst], lambda: ops.pack_rows(uo.view, c, dst.view))
    assert_same_bits(got, uo.view.contiguous(), "pack_rows")
    b = 2
    back = O((b, c, f // 2, hw), F32)
    got, = sweep("nhwc_to_ncfhw", [uo], [back], lambda: L.check(ops._lib.vx_nhwc_to_ncfhw(
        uo.view.data_ptr(), ld, b, c, f // 2, hw, back.view.data_ptr(), stream()), "vx_nhwc_to_ncfhw"))
    assert_same_bits(got, uo.view[:b * (f // 2) * hw].reshape(b, f // 2, hw, c).permute(0, 3, 1, 2).contiguous(), "nhwc_to_ncfhw")
    t = G(rnd(b, c, 3, hw), F32)
    nh = O((b * 3, hw, c_pad), el)
    got, = sweep("ncfhw_to_nhwc", [t], [nh], lambda: L.check(ops._lib.vx_ncfhw_to_nhwc(
        t.view.data_ptr(), b, c, 3, hw, c_pad, nh.view.data_ptr(), stream()), "vx_ncfhw_to_nhwc"))
    check(got[..., :c], t.view.permute(0, 2, 3, 1).reshape(b * 3, hw, c), "ncfhw_to_nhwc", rel=4e-3, mx=2 ** -8)
    assert (got[..., c:].view(torch.int16) == 0).all()


def _unit_layout(xs, granules, seed, spare=3):
    """tests/test_gpu_guidance.py::layout for any number of rows: the predictions scattered over an all-gathered buffer."""
    nW, c, f, hw = xs[0].shape
    fl, rows = f // granules, len(xs)
    n = nW * rows * granules
    perm = torch.randperm(n + spare, generator=torch.Generator().manual_seed(seed))[:n]
    gathered = torch.zeros((n + spare, fl * hw, c))
    uidx = torch.empty((nW, rows, granules), dtype=torch.int32)
    k = 0
    for w in range(nW):
        for r, x in enumerate(xs):
            for j in range(granules):
                slot = int(perm[k])
                k += 1
                uidx[w, r, j] = slot
                gathered[slot] = x[w, :, j * fl:(j + 1) * fl].permute(1, 2, 0).reshape(fl * hw, c)
    return gathered, uidx


@pytest.mark.parametrize("hw", [80, 1028])
def test_combine_and_rescale(ops, hw):
    """vx_combine_units (one and two halves), vx_combine_units3 and the two rescales with their workspace at exactly
    vx_guidance_rescale_ws_floats; hw = 1028 is two chunks of 1024 pixels, the second one ragged.  Bounds of
    tests/test_gpu_guidance.py / tests/test_gpu_audio_guidance.py: 4 x the error of float32 torch.std on the CPU."""
    import audio_guidance_restated as A
    import guidance_restated as GR
    nW, c, f, S, s, s_a, phi = 2, 4, 4, 2, 3.5, 2.0, 0.7
    g = torch.Generator().manual_seed(hw)
    u = torch.randn(nW, c, f, hw, generator=g) + 3.0
    mid = u + 0.3 * torch.randn(nW, c, f, hw, generator=g)
    cond = mid + 0.2 * torch.randn(nW, c, f, hw, generator=g)
    n_ws = ops.guidance_rescale_ws_floats(nW, f, hw)
    assert n_ws == nW * f * math.ceil(hw / 1024) * 6
    for xs in ((cond,), (u, cond), (u, mid, cond)):
        gathered, uidx = _unit_layout(xs, S, seed=len(xs))
        gg, gi = G(gathered, F32), G(uidx, torch.int32)
        preds, ws = O((nW, c, f, hw), F32), O((n_ws,), F32)
        if len(xs) < 3:
            got, = sweep(f"combine_units halves={len(xs)}", [gg, gi], [preds],
                         lambda: ops.combine_units(gg.view, gi.view, c, f, hw, s, preds.view))
            want = cond if len(xs) == 1 else (u.double() + s * (cond.double() - u.double())).float()
            if len(xs) == 1:
                assert_same_bits(got.cpu(), want, "combine_units, one half: a copy")
                continue
            check(got.cpu(), want, "combine_units", rel=1e-6, mx=1e-6)
            got, _ = sweep("guidance_rescale", [gg, gi], [preds, Out(ws, finite=False)],
                           lambda: ops.guidance_rescale(gg.view, gi.view, c, f, hw, s, phi, ws.view, preds.view))
            err = (got.cpu().double() - GR.combine_rescaled(u, cond, s, phi)).abs().max().item()
            assert err <= 4 * GR.float32_baseline_error(u, cond, s, phi), err
        else:
            got, = sweep("combine_units3", [gg, gi], [preds],
                         lambda: ops.combine_units3(gg.view, gi.view, c, f, hw, s, s_a, preds.view))
            check(got.cpu(), A.combine3(u, mid, cond, s, s_a).float(), "combine_units3", rel=1e-6, mx=1e-6)
            got, _ = sweep("guidance_rescale3", [gg, gi], [preds, Out(ws, finite=False)],
                           lambda: ops.guidance_rescale3(gg.view, gi.view, c, f, hw, s, s_a, phi, ws.view, preds.view))
            err = (got.cpu().double() - A.combine3_rescaled(u, mid, cond, s, s_a, phi)).abs().max().item()
            assert err <= 4 * A.float32_baseline_error3(u, mid, cond, s, s_a, phi), err


def test_vae_postprocess(ops):
    import init_video_restated as IV
    L = ops.L
    n, c, h, w, ld, Ftot, frame0 = 2, 3, 5, 7, 8, 5, 2
    hw = h * w
    x = G(rnd(n * hw, c) * 2, F32, ld=ld)
    out = O((n, c, hw), F32)
    got, = sweep("vae_postprocess", [x], [out], lambda: L.check(ops._lib.vx_vae_postprocess(
        x.view.data_ptr(), ld, n, c, hw, out.view.data_ptr(), stream()), "vx_vae_postprocess"))
    plain = (x.view.reshape(n, hw, c).permute(0, 2, 1) / 2 + 0.5).clamp(0, 1)
    assert torch.allclose(got, plain)                        # tests/test_gpu_kernels.py::test_layout_and_loop_kernels
    g = torch.Generator().manual_seed(5)
    init, mask = G(torch.rand(c, Ftot, hw, generator=g), F32), G(torch.rand(Ftot, hw, generator=g), F32)
    mask.view[frame0, :5] = 1.0
    mask.view[frame0, 5:10] = 0.0
    got2, = sweep("vae_postprocess_composite", [x, init, mask], [out], lambda: L.check(ops._lib.vx_vae_postprocess_composite(
        x.view.data_ptr(), ld, n, c, hw, init.view.data_ptr(), Ftot, frame0, mask.view.data_ptr(), Ftot, out.view.data_ptr(),
        stream()), "vx_vae_postprocess_composite"))
    keep = init.view[:, frame0:frame0 + n].permute(1, 0, 2)
    ref = IV.composite(got.cpu(), keep.cpu(), mask.view[frame0:frame0 + n].cpu())
    # float32 evaluation of M v + (1 - M) init on values in [0, 1]: three roundings of magnitudes <= 1
    assert (got2.cpu().double() - ref).abs().max().item() <= 4 * 2.0 ** -24
    assert_same_bits(got2[0, :, :5], got[0, :, :5], "M = 1: the bits of vx_vae_postprocess")
    assert_same_bits(got2[0, :, 5:10], keep[0, :, 5:10].contiguous(), "M = 0: the bits of init")


@pytest.mark.parametrize("c,f,h,w", [(3, 2, 2, 2), (1, 3, 5, 7)])
def test_median3d(ops, c, f, h, w):
    L = ops.L
    v = G(torch.rand(c, f, h, w, generator=torch.Generator().manual_seed(h)), F32)
    o32, o8 = O((c, f, h, w), F32), O((f, h, w, c), torch.uint8)
    g32, g8 = sweep(f"median3d {c}x{f}x{h}x{w}", [v], [o32, o8], lambda: L.check(ops._lib.vx_median3d(
        v.view.data_ptr(), c, f, h, w, o32.view.data_ptr(), o8.view.data_ptr(), stream()), "vx_median3d"))
    xp = F.pad(v.view[None], (1, 1, 1, 1, 1, 1), mode="reflect")[0]
    win = xp.unfold(1, 3, 1).unfold(2, 3, 1).unfold(3, 3, 1).reshape(c, f, h, w, 27)
    ref = win.sort(dim=-1).values[..., 13]
    assert_same_bits(g32, ref.contiguous(), "median3d: a selection, exact")
    assert_same_bits(g8, (ref * 255).to(torch.uint8).permute(1, 2, 3, 0).contiguous(), "median3d uint8 packing")


def test_wave_conv1d(ops):
    el = torch.bfloat16
    L = ops.L
    samples, taps, stride, c = 1003, 10, 5, 64
    assert (samples - taps) % stride != 0
    t_out = (samples - taps) // stride + 1
    wave, wt = G(rnd(samples), F32), G(rnd(taps, c, scale=taps ** -0.5, seed=1), F32)
    out = O((t_out, c), el)
    got, = sweep("wave_conv1d", [wave, wt], [out], lambda: L.check(ops._lib.vx_wave_conv1d(
        wave.view.data_ptr(), samples, wt.view.data_ptr(), c, taps, stride, out.view.data_ptr(), stream()), "vx_wave_conv1d"))
    ref = wave.view.unfold(0, taps, stride) @ wt.view
    check(got, ref, "wave_conv1d")


def _plan():
    """11 frames, three windows of 4 ([0..3], [2..5], [4..7]); the step updates frames 1..6 only.  Three term columns, the
    middle one skipped (-1) wherever two windows overlap."""
    wins = [[0, 1, 2, 3], [2, 3, 4, 5], [4, 5, 6, 7]]
    sf = [1, 2, 3, 4, 5, 6]
    terms = torch.full((len(sf), 3, 2), -1, dtype=torch.int32)
    counts = torch.zeros(len(sf))
    for i, fr in enumerate(sf):
        hits = [(wi, w.index(fr)) for wi, w in enumerate(wins) if fr in w]
        for (wi, li), col in zip(hits, (0, 2)):
            terms[i, col, 0], terms[i, col, 1] = wi, li
        counts[i] = len(hits)
    return sf, terms, counts


def _mean_v(preds, terms, counts, c, hw):
    """float32 restatement of the kernels' mean_of_terms: each term divided by the count, summed in term order."""
    v = torch.zeros(terms.shape[0], c, hw)
    for i in range(terms.shape[0]):
        first = True
        for t in range(terms.shape[1]):
            slot, li = int(terms[i, t, 0]), int(terms[i, t, 1])
            if slot < 0:
                continue
            term = preds[slot, :, li] / counts[i]
            v[i] = term if first else v[i] + term
            first = False
    return v


@pytest.mark.parametrize("hw", [8, 80])
def test_overlap_updates(ops, hw):
    """The three overlap updates and vx_overlap_blend: the WHOLE latent clip (and x0_history) is the window; frames the
    step does not list keep their bits; a skipped middle term.  Tolerance of tests/test_gpu_kernels.py's loop check
    (1e-5 of the largest value); the blend is bit-exact against its float32 host expression (header)."""
    import ancestral_restated as AN
    import window_blend_restated as WB
    c, Ftot, fw = 4, 11, 4
    sf, terms, counts = _plan()
    g = torch.Generator().manual_seed(hw)
    lat0, hist0 = torch.randn(c, Ftot, hw, generator=g), torch.randn(c, Ftot, hw, generator=g)
    preds = G(torch.randn(3, c, fw, hw, generator=g), F32)
    tg, ig, cg = G(terms, torch.int32), G(torch.tensor(sf, dtype=torch.int32), torch.int32), G(counts, F32)
    lat, hist = O((1, c, Ftot, 1, hw), F32), O((1, c, Ftot, 1, hw), F32)
    other = [i for i in range(Ftot) if i not in sf]
    v = _mean_v(preds.view.cpu(), terms, counts, c, hw).permute(1, 0, 2)           # [c, frames of the step, hw]
    x = lat0[:, sf]

    def untouched(got, src, what):
        assert_same_bits(got.cpu()[0, :, other, 0], src[:, other], f"{what}: frames outside step_frames")

    coef = (0.8, 0.6, 0.9, 0.43589)
    got, = sweep("overlap_ddim_step", [preds, tg, ig, cg], [Out(lat, init=lat0)], lambda: ops.overlap_ddim_step(
        lat.view, preds.view, tg.view, ig.view, cg.view, coef))
    untouched(got, lat0, "ddim")
    ref = coef[2] * (coef[0] * x - coef[1] * v) + coef[3] * (coef[0] * v + coef[1] * x)
    check(got.cpu()[0, :, sf, 0], ref, "overlap_ddim_step", rel=1e-5, mx=1e-5)
    mcoef = (0.8, 0.6, 1.1, 0.7, 0.25)
    got, gh = sweep("overlap_multistep_step", [preds, tg, ig, cg], [Out(lat, init=lat0), Out(hist, init=hist0)],
                    lambda: ops.overlap_multistep_step(lat.view, preds.view, tg.view, ig.view, cg.view, hist.view, mcoef))
    untouched(got, lat0, "multistep")
    untouched(gh, hist0, "multistep x0_history")
    x0 = mcoef[0] * x - mcoef[1] * v
    check(gh.cpu()[0, :, sf, 0], x0, "overlap_multistep_step x0", rel=1e-5, mx=1e-5)
    check(got.cpu()[0, :, sf, 0], mcoef[2] * x - mcoef[3] * x0 + mcoef[4] * hist0[:, sf], "overlap_multistep_step", rel=1e-5, mx=1e-5)
    acoef, seed, step = (0.8, 0.6, 1.1, 0.7, 0.3), 0x1234567887654321, 7
    got, = sweep("overlap_ancestral_step", [preds, tg, ig, cg], [Out(lat, init=lat0)], lambda: ops.overlap_ancestral_step(
        lat.view, preds.view, tg.view, ig.view, cg.view, acoef, seed, step))
    untouched(got, lat0, "ancestral")
    z = torch.from_numpy(AN.normals(seed, step, sf, c, hw)).float()                # [c, frames of the step, hw]
    ref = acoef[2] * x - acoef[3] * (acoef[0] * x - acoef[1] * v) + acoef[4] * z
    check(got.cpu()[0, :, sf, 0], ref, "overlap_ancestral_step", rel=1e-5, mx=1e-5)
    wts = torch.rand(len(sf), 3, generator=g)
    wg = G(wts, F32)
    blend = O((c, len(sf), hw), F32)
    pa = G(preds.view.cpu(), F32)
    got, = sweep("overlap_blend", [pa, tg, wg], [blend], lambda: ops.overlap_blend(pa.view, tg.view, wg.view, blend.view))
    want = torch.empty(c, len(sf), hw)
    WB.overlap_blend(pa.view.cpu(), terms, wts, want)
    assert_same_bits(got.cpu(), want, "overlap_blend vs its float32 host expression")


@pytest.mark.parametrize("masked", [True, False])
def test_known_blend(ops, masked):
    import init_video_restated as IV
    c, Ftot, h, w, a, s = 4, 3, 2, 6, 0.8, 0.6
    g = torch.Generator().manual_seed(9)
    lat0 = torch.randn(1, c, Ftot, h, w, generator=g)
    init, noise = G(torch.randn(1, c, Ftot, h, w, generator=g), F32), G(torch.randn(1, c, Ftot, h, w, generator=g), F32)
    m = torch.rand(Ftot, h * w, generator=g)
    m[0, :4], m[1, :4] = 1.0, 0.0
    mask = G(m, F32)
    lat = O((1, c, Ftot, h, w), F32)
    got, = sweep(f"known_blend masked={masked}", [init, noise] + ([mask] if masked else []), [Out(lat, init=lat0)],
                 lambda: ops.known_blend(lat.view, init.view, noise.view, mask.view if masked else None, a, s))
    mm = m if masked else None
    ref = IV.blend(lat0, init.view.cpu(), noise.view.cpu(), mm, a, s)
    bound = IV.blend_bound(lat0, init.view.cpu(), noise.view.cpu(), mm, a, s)     # tests/test_gpu_init_video.py's bound
    assert ((got.cpu().double() - ref).abs() <= bound + 1e-30).all()
    if masked:
        assert_same_bits(got.cpu()[0, :, 0].reshape(c, -1)[:, :4], lat0[0, :, 0].reshape(c, -1)[:, :4], "m = 1 keeps the latent's bits")
