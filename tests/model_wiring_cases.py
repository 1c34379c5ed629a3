"""Stage-by-stage wiring cases of the models outside the denoising UNet (TEST INFRASTRUCTURE, host only, torch on any
device): v_express_amd/vae.py (decode, encode), wav2vec2.py and prologue.py (AudioProjection, VKpsGuider).

    case  = make_case("vae_decode", "small", device="cpu", elem=torch.bfloat16)
    calls = record(case, tap)                 # the model on ops.* as they are, under tests/stage_tap.py
    check_sequence(case, calls)               # the tapped call sequence and its scalar arguments EQUAL the stage table
    for st, recs, prev in split(case, calls): # per stage: the PRODUCT's own stage input, converted to float64,
        ref = st.ref(st.reads(recs, prev, case), case.w64, None)      # through the float64 reference of that stage
        err = errors(st.got(recs), ref)

A stage is (name, [(tapped call, the scalar arguments it must have received)], float64 reference).  The scalar arguments
are stated here from the reference's definition (oracle/vae.py, oracle/wav2vec2.py, oracle/prologue.py: GroupNorm eps 1e-6
in every VAE norm, 1e-5 in wav2vec2's layer 0 with one group per channel, the config's layer_norm_eps, one attention head
in the VAE, the activation code of every GEMM, strides and paddings), never read from the product.  Every reference is
built from the RAW state_dict through oracle/leaf.py and the arithmetic of oracle/*.py, in the product's token layout, so
that the stage outputs chain: `chain(case, mutant)` is the whole float64 model, with one stage wired wrongly if asked.
Every stage holds at least one rounding to the element type (a float32-output GEMM goes with the call in front of it), so
the emulation's error against float64, e_emul, is the stage's measured bound; pure data movement (layout calls, the
group-major padded copy of the positional convolution, the Perceiver blocks' key / value rows) is bit-equal (`Stage.moves`).

MUTANTS are edits of the REFERENCE of the stage they touch.  A mutant that changes the stage's output SHAPE (stride 2 on
an even guider block) counts as infinitely far: the product's tensor cannot be compared with it at all.  Notes:
  * wav2vec2 has no convolution bias (conv_bias=False is the one variant V-Express loads, and the strict schema refuses
    the key), yet `_prepared` reads one where the state_dict has it.  The small case puts biases on conv layers 1 .. 6
    behind the schema (straight into the model's raw tensors), so "a conv layer's bias dropped" is a mutant of live code.
  * "positional conv dropping its first output instead of its last" and "padding kp/2 - 1 in front" are ONE error at T
    outputs (both shift the window by one row over the same zero padding); both are listed, they measure the same.
  * stride 2 on the even guider blocks: same output shape at MODEL level only; at stage level the shape differs (above),
    and the stage table's `geom.stride` catches it by name.
Two edits are EQUIVALENT by construction and therefore no mutants:
  * a dropped KEY bias: it adds q . b_k to every logit of a query, which the softmax cancels;
  * keys ordered latents-first in the Perceiver attention: the attention is permutation-invariant over its keys.
`k_proj.bias` / `to_k.bias` are pinned where they are visible instead: tests/test_model_wiring_cpu.py compares the
prepared `bqkv` tensors with their float64 statement (float32 biases within 1e-5, the block wiring tests' rule).
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import cases
from oracle import leaf as L

ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2                 # lib.VX_ACT_* as include/vexpress_hip.h states them
OLD_BOUND = {"vae_decode": 3e-2, "vae_encode": 2e-2, "wav2vec2": 3e-2, "audio_projection": 2e-2, "kps_guider": 2e-2}


def pad8(n):
    return (n + 7) // 8 * 8


class Stage(SimpleNamespace):
    """name; calls [(tapped name, {scalar: value})]; ref(state, w, mut) -> float64 output in the product's layout;
    reads(recs, prev, case) -> state {key: float64 tensor} from the product's recorded inputs; got(recs) -> the product's
    output; put: the state key the output is stored under for the next stage; exact: the output is ref rounded once;
    moves(recs, prev, case) -> [(what, got, want)] bit-equal data movement inside the stage."""


def _first_input(recs, prev, case):
    return {"x": next(iter(recs[0].inputs.values())).double()}


def _last_out(recs):
    r = recs[-1]
    return r.out if r.out is not None else r.after["h"]


def stage(name, calls, ref, reads=_first_input, got=_last_out, put="x", exact=False, moves=None):
    return Stage(name=name, calls=calls, ref=ref, reads=reads, got=got, put=put, exact=exact, moves=moves)


# ------------------------------------------------------------------------------------------------ layouts
def nchw(x, n, H, W, c=None):
    x = x.reshape(n, H, W, -1)
    return (x if c is None else x[..., :c]).permute(0, 3, 1, 2)


def tok(y, flat=False):
    """[n, C, H, W] -> tokens [n, HW, pad8(C)] (zero columns behind C, like the product's channel padding)."""
    n, c, h, w = y.shape
    t = y.permute(0, 2, 3, 1).reshape(n, h * w, c)
    if pad8(c) != c:
        t = F.pad(t, (0, pad8(c) - c))
    return t.reshape(n * h * w, -1) if flat else t


def _without(w, *keys):
    w = dict(w)
    for k in keys:
        w[k] = torch.zeros_like(w[k])
    return w


def _conv(w, p, x, n, H, W, stride=1, padding=1, mut=None, pad_end=False):
    cin = w[p + ".weight"].shape[1]
    img = nchw(x, n, H, W, cin)
    if pad_end:
        img = F.pad(img, (0, 1, 0, 1))
    return L.conv2d(_without(w, p + ".bias") if mut == "bias" else w, p, img, stride=stride, padding=padding)


# ------------------------------------------------------------------------------------------------ VAE
def _gemm(act=ACT_NONE, out_f32=False, **geom):
    return ("ops.gemm", dict(act=act, out_f32=out_f32, alpha=1.0, **{f"geom.{k}": v for k, v in geom.items()}))


_C3 = dict(kh=3, kw=3, stride=1, pad=1)                 # a 3x3 convolution over the stored image
_C3P = dict(kh=3, kw=3, stride=1, pad=0)                # ... over the zero-bordered image a GroupNorm wrote


def _vae_attn(w, p, x, n, H, W, g, mut):
    """oracle.vae._vae_attention with its wiring open to edits: GroupNorm(eps 1e-6), ONE head, biased q/k/v/out, + x."""
    img = nchw(x, n, H, W)
    c = img.shape[1]
    h = F.group_norm(img.reshape(n, c, H * W), g, w[p + ".group_norm.weight"], w[p + ".group_norm.bias"], 1e-6).transpose(1, 2)
    if mut in ("to_q_bias", "to_out_bias"):
        w = _without(w, p + (".to_q.bias" if mut == "to_q_bias" else ".to_out.0.bias"))
    o = L.attention(w, p, h, h, heads=8 if mut == "heads8" else 1)
    o = o.transpose(1, 2).reshape(n, c, H, W)
    return tok(o if mut == "no_residual" else o + img)


def _resnet_stage(name, p, n, H, W, g):
    def ref(s, w, mut):
        if mut == "shortcut_bias":
            w = _without(w, p + ".conv_shortcut.bias")
        return tok(L.resnet(w, p, nchw(s["x"], n, H, W), None, g, 1e-6))
    return stage(name, [("blocks.resnet_block", dict(groups=g, eps=1e-6, frames=n, H=H, W=W, items=None, rows_per_group=0))],
                 ref, reads=lambda recs, prev, case: {"x": recs[0].inputs["x"].double()})


def _mid_attn_stage(name, p, n, H, W, g):
    return stage(name, [("ops.groupnorm", dict(groups=g, eps=1e-6, silu=False, frames=n, hw=H * W, pad_hw=None)),
                        ("blocks._self_attention", dict(heads=1, seqs=n, n_tok=H * W, rows_per_item=0))],
                 lambda s, w, mut: _vae_attn(w, p, s["x"], n, H, W, g, mut).reshape(n * H * W, -1),
                 reads=lambda recs, prev, case: {"x": recs[0].inputs["x1"].double()},
                 got=lambda recs: recs[1].after["h"])


def _norm_out_stage(name, norm, convs, n, H, W, g, out_rows=None):
    """GroupNorm(eps 1e-6) + SiLU into the zero-bordered image, conv_out (and, in the encoder, quant_conv 1x1) into float32."""
    def ref(s, w, mut):
        y = F.silu(L.group_norm(w, norm, nchw(s["x"], n, H, W), g, 1e-6))
        y = L.conv2d(w, convs[0], y)
        for p in convs[1:]:
            y = L.conv2d(_without(w, p + ".bias") if mut == "quant_bias" else w, p, y, padding=0)
        return tok(y, flat=True)
    gemms = [_gemm(out_f32=len(convs) == 1, **_C3P)] + [("ops.gemm", dict(act=ACT_NONE, out_f32=True, alpha=1.0))
                                                         for _ in convs[1:]]
    return stage(name, [("ops.groupnorm", dict(groups=g, eps=1e-6, silu=True, frames=n, hw=H * W, pad_hw=(H, W)))] + gemms,
                 ref, reads=lambda recs, prev, case: {"x": recs[0].inputs["x1"].double()})


def _decode_token_stages(cfg, n, h, w_):
    g, H, W = cfg.norm_num_groups, h, w_
    st = [stage("post_quant_conv+conv_in", [("ops.gemm", dict(act=ACT_NONE, out_f32=False, alpha=1.0)), _gemm(**_C3)],
                lambda s, w, mut, H=H, W=W: tok(L.conv2d(w, "decoder.conv_in",
                                                        _conv(w, "post_quant_conv", s["x"], n, H, W, padding=0,
                                                              mut="bias" if mut == "post_quant_bias" else None))),
                reads=lambda recs, prev, case: {"x": recs[0].inputs["a"].double()})]
    st.append(_resnet_stage("mid.resnets.0", "decoder.mid_block.resnets.0", n, H, W, g))
    st.append(_mid_attn_stage("mid.attention", "decoder.mid_block.attentions.0", n, H, W, g))
    st.append(_resnet_stage("mid.resnets.1", "decoder.mid_block.resnets.1", n, H, W, g))
    nb = len(cfg.block_out_channels)
    for i in range(nb):
        for j in range(cfg.layers_per_block + 1):
            st.append(_resnet_stage(f"up.{i}.resnets.{j}", f"decoder.up_blocks.{i}.resnets.{j}", n, H, W, g))
        if i != nb - 1:
            def up(s, w, mut, p=f"decoder.up_blocks.{i}.upsamplers.0", H=H, W=W):
                a, b = (W, H) if mut == "hw_swap" else (H, W)      # the image read with its axes exchanged
                return tok(L.upsample(w, p, nchw(s["x"], n, a, b)))
            st.append(stage(f"up.{i}.upsampler", [("blocks.upsample", dict(frames=n, H=H, W=W, items=n))], up,
                            reads=lambda recs, prev, case: {"x": recs[0].inputs["x"].double()}))
            H, W = 2 * H, 2 * W
    st.append(_norm_out_stage("conv_norm_out+conv_out", "decoder.conv_norm_out", ["decoder.conv_out"], n, H, W, g))
    return st, H, W


def vae_decode_stages(cfg, n, h, w_):
    st, H, W = _decode_token_stages(cfg, n, h, w_)
    c_lat, c_out = cfg.latent_channels, cfg.out_channels
    first = stage("layout_in", [("ops.ncfhw_to_nhwc", dict(c_pad=8))],
                  lambda s, w, mut: tok(s["x"].reshape(n, c_lat, h, w_)), exact=True)
    last = stage("layout_out", [("ops.nhwc_to_ncfhw", dict(b=n, c=c_out, f=1, h=H, w=W))],
                 lambda s, w, mut: nchw(s["x"], n, H, W, c_out)[:, :, None], exact=True)
    return [first] + st + [last]


def vae_decode_video_stages(cfg, F_, h, w_, chunk):
    """decode_video: latents / scaling_factor, `chunk` frames per decode_tokens call, vx_vae_postprocess (x / 2 + 0.5
    clamped to [0, 1]) per chunk.  State "x<f0>": the chunks are independent chains from the case's latents."""
    out = []
    for f0 in range(0, F_, chunk):
        n = min(chunk, F_ - f0)
        st, H, W = _decode_token_stages(cfg, n, h, w_)

        def lay(s, w, mut, f0=f0, n=n):
            lat = s["latents"][0, :, f0:f0 + n].permute(1, 0, 2, 3)
            return tok(lat * cfg.scaling_factor if mut == "times_scaling_factor" else lat / cfg.scaling_factor)
        out.append(stage(f"chunk{f0}.scale+layout_in", [("ops.ncfhw_to_nhwc", dict(c_pad=8))], lay,
                         reads=lambda recs, prev, case: {"latents": case.inputs["latents"].double()}))
        for s_ in st:
            s_.name = f"chunk{f0}." + s_.name
        out += st
        out.append(stage(f"chunk{f0}.postprocess", [("ops.vae_postprocess", dict(n=n, c=cfg.out_channels, h=H, w=W))],
                         lambda s, w, mut, n=n, H=H, W=W: (nchw(s["x"], n, H, W, cfg.out_channels) / 2 + 0.5).clamp(0, 1)))
    return out


def vae_encode_stages(cfg, n, H, W):
    g, c_lat = cfg.norm_num_groups, cfg.latent_channels
    st = [stage("layout_in", [("ops.ncfhw_to_nhwc", dict(c_pad=8))],
                lambda s, w, mut, H=H, W=W: tok(s["x"].reshape(n, cfg.out_channels, H, W)), exact=True),
          stage("conv_in", [_gemm(**_C3)], lambda s, w, mut, H=H, W=W: tok(_conv(w, "encoder.conv_in", s["x"], n, H, W), flat=True))]
    nb = len(cfg.block_out_channels)
    for i in range(nb):
        for j in range(cfg.layers_per_block):
            st.append(_resnet_stage(f"down.{i}.resnets.{j}", f"encoder.down_blocks.{i}.resnets.{j}", n, H, W, g))
        if i != nb - 1:
            def down(s, w, mut, p=f"encoder.down_blocks.{i}.downsamplers.0.conv", H=H, W=W):
                if mut == "pad_symmetric":
                    return tok(_conv(w, p, s["x"], n, H, W, stride=2, padding=1), flat=True)
                return tok(_conv(w, p, s["x"], n, H, W, stride=2, padding=0, pad_end=True), flat=True)
            st.append(stage(f"down.{i}.downsampler", [_gemm(kh=3, kw=3, stride=2, pad=0, h_out=H // 2, w_out=W // 2)], down))
            H, W = H // 2, W // 2
    st.append(_resnet_stage("mid.resnets.0", "encoder.mid_block.resnets.0", n, H, W, g))
    st.append(_mid_attn_stage("mid.attention", "encoder.mid_block.attentions.0", n, H, W, g))
    st.append(_resnet_stage("mid.resnets.1", "encoder.mid_block.resnets.1", n, H, W, g))
    st.append(_norm_out_stage("conv_norm_out+conv_out+quant_conv", "encoder.conv_norm_out", ["encoder.conv_out", "quant_conv"],
                              n, H, W, g))

    def mean(s, w, mut):
        m = s["x"].reshape(n, H, W, -1)
        m = m[..., c_lat:2 * c_lat] if mut == "mean_second_half" else m[..., :c_lat]
        return m.permute(0, 3, 1, 2)[:, :, None]
    st.append(stage("mean+layout_out", [("ops.nhwc_to_ncfhw", dict(b=n, c=c_lat, f=1, h=H, w=W))], mean, exact=True))
    return st


# ------------------------------------------------------------------------------------------------ VKpsGuider
def kps_stages(cfg, n, H, W):
    nblk = 2 * (len(cfg.block_out_channels) - 1)
    st = [stage("layout_in", [("ops.ncfhw_to_nhwc", dict(c_pad=8))],
                lambda s, w, mut: tok(s["x"][0].permute(1, 0, 2, 3)), exact=True),
          stage("conv_in", [_gemm(ACT_SILU, **_C3)],
                lambda s, w, mut, H=H, W=W: tok(F.silu(_conv(w, "conv_in", s["x"], n, H, W, mut=mut)), flat=True))]
    for i in range(nblk):
        stride = 2 if i % 2 else 1                         # modules/v_kps_guider.py: the SECOND conv of each pair strides

        def blk(s, w, mut, i=i, H=H, W=W, stride=stride):
            s_ = (1 if stride == 2 else 2) if mut == "stride_even" else stride
            H, W = s.get("hw", (H, W))                     # (a chained state carries the geometry a stride mutant left)
            y = F.silu(_conv(w, f"blocks.{i}", s["x"], n, H, W, stride=s_, mut=mut))
            s["hw"] = tuple(y.shape[2:])
            return tok(y, flat=True)
        st.append(stage(f"blocks.{i}", [_gemm(ACT_SILU, kh=3, kw=3, stride=stride, pad=1)], blk))
        if stride == 2:
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1

    def out(s, w, mut, H=H, W=W):
        H, W = s.get("hw", (H, W))
        y = _conv(w, "conv_out", s["x"], n, H, W)
        return tok(F.silu(y) if mut == "silu_after" else y, flat=True)
    st.append(stage("conv_out", [_gemm(ACT_NONE, **_C3)], out))
    return st


# ------------------------------------------------------------------------------------------------ AudioProjection
def _perceiver(w, p, x, lat, heads, mut):
    """oracle.prologue._perceiver_attention (modules/audio_projection.py:48-85) in float64, open to edits."""
    n1, n2 = (".norm2", ".norm1") if mut == "norms_swapped" else (".norm1", ".norm2")
    x, lat = L.layer_norm(w, p + n1, x), L.layer_norm(w, p + n2, lat)
    b, l, _ = lat.shape
    q = F.linear(lat, w[p + ".to_q.weight"])
    k, v = F.linear(torch.cat((x, lat), dim=-2), w[p + ".to_kv.weight"]).chunk(2, dim=-1)
    d = q.shape[-1] // heads

    def split(t):
        return t.view(b, t.shape[1], heads, d).transpose(1, 2)
    q, k, v = split(q), split(k), split(v)
    scale = d ** -0.25
    s = (q * scale) @ (k if mut == "scale_once" else k * scale).transpose(-2, -1)
    out = (torch.softmax(s, dim=-1) @ v).permute(0, 2, 1, 3).reshape(b, l, -1)
    return F.linear(out, w[p + ".to_out.weight"])


def audio_stages(cfg, Fn, n):
    nq, dim, heads = cfg.num_queries, cfg.dim, cfg.heads
    ln = ("ops.layernorm", dict(eps=1e-5, add=None))
    lin = ("ops.gemm", dict(act=ACT_NONE, out_f32=False, alpha=1.0))

    def proj_in(s, w, mut):
        pos = w["pos_emb.weight"]
        x = s["x"] + (0 if mut == "pos_emb_dropped" else pos[:n].roll(1, 0) if mut == "pos_emb_shifted" else pos[:n])
        return L.linear(w, "proj_in", x).reshape(Fn * n, dim)
    st = [stage("pos_emb+proj_in", [lin], proj_in, reads=lambda recs, prev, case: {"x": case.inputs["x"].double()},
                put="xt")]
    for i in range(cfg.depth):
        a, f = f"layers.{i}.0", f"layers.{i}.1"

        def attn(s, w, mut, a=a, i=i):
            lat = s["lat"].reshape(Fn, nq, dim)
            src = lat[:1].expand(Fn, nq, dim) if mut == "latents_frame0" else lat
            return (_perceiver(w, a, s["xt"].reshape(Fn, n, dim), src, heads, mut) + lat).reshape(Fn * nq, dim)

        def kv_rows(recs, prev, case, i=i):
            want = torch.cat([recs[0].out.view(Fn, n, dim), recs[1].out.view(Fn, nq, dim)], dim=1).reshape(Fn * (n + nq), dim)
            out = [("kvin = LN1(x) ++ LN2(latents)", recs[3].inputs["a"], want)]
            if i == 0:                                     # the learned queries, rounded once, one copy per frame
                out.append(("latents repeated per frame", recs[1].inputs["x"],
                            case.w64["latents"][0].to(recs[1].inputs["x"].dtype).repeat(Fn, 1)))
            return out
        st.append(stage(f"layers.{i}.attention",
                        [ln, ln, lin, lin, ("ops.small_kv_attention", dict(batch=Fn, n_q=nq, n_kv=n + nq, heads=heads,
                                                                           head_dim=cfg.dim_head)), lin],
                        attn, reads=lambda recs, prev, case: {"xt": recs[0].inputs["x"].double(),
                                                              "lat": recs[1].inputs["x"].double()},
                        put="lat", moves=kv_rows))

        def ff(s, w, mut, f=f):
            lat = s["lat"]
            h = F.linear(F.gelu(F.linear(L.layer_norm(w, f + ".0", lat), w[f + ".1.weight"])), w[f + ".3.weight"])
            return h if mut == "ff_no_residual" else h + lat
        st.append(stage(f"layers.{i}.feed_forward", [ln, ("ops.gemm", dict(act=ACT_GELU, out_f32=False, alpha=1.0)), lin], ff,
                        reads=lambda recs, prev, case: {"lat": recs[0].inputs["x"].double()}, put="lat"))

    def out(s, w, mut):
        if mut == "norm_out_first":
            return L.linear(w, "proj_out", L.layer_norm(w, "norm_out", s["lat"]))
        return L.layer_norm(w, "norm_out", L.linear(w, "proj_out", s["lat"]))
    st.append(stage("proj_out+norm_out", [lin, ln], out, reads=lambda recs, prev, case: {"lat": recs[0].inputs["a"].double()},
                    put="out"))
    return st


# ------------------------------------------------------------------------------------------------ wav2vec2
def _pos_weight(w, mut):
    p = "encoder.pos_conv_embed.conv.parametrizations.weight.original"
    g, v = w[p + "0"], w[p + "1"]
    if mut == "weight_norm_out_channel":                   # weight_norm(dim=0): one norm per OUTPUT channel
        return g * v / v.norm(dim=(1, 2), keepdim=True)
    return g * v / v.norm(dim=(0, 1), keepdim=True)        # weight_norm(dim=2): one norm per tap


def _w2v_layer_attn(w, p, x, heads, mut):
    t, c = x.shape
    d = c // heads
    src = L.layer_norm(w, p + ".layer_norm", x) if mut == "pre_ln" else x
    wq = _without(w, p + ".attention.q_proj.bias") if mut == "q_bias" else w
    q = L.linear(wq, p + ".attention.q_proj", src) * d ** -0.5
    if mut == "q_scaled_before_bias":
        q = F.linear(src, w[p + ".attention.q_proj.weight"]) * d ** -0.5 + w[p + ".attention.q_proj.bias"]
    k, v = L.linear(w, p + ".attention.k_proj", src), L.linear(w, p + ".attention.v_proj", src)
    q, k, v = (y.view(t, heads, d).transpose(0, 1) for y in (q, k, v))
    a = (torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v).transpose(0, 1).reshape(t, c)
    wo = _without(w, p + ".attention.out_proj.bias") if mut == "out_bias" else w
    return x + L.linear(wo, p + ".attention.out_proj", a)


def w2v_stages(cfg, samples):
    c = cfg.conv_dim[0]
    eps, heads = cfg.layer_norm_eps, cfg.num_attention_heads
    G, kp, Hd = cfg.num_conv_pos_embedding_groups, cfg.num_conv_pos_embeddings, cfg.hidden_size
    fe = "feature_extractor.conv_layers."
    T = (samples - cfg.conv_kernel[0]) // cfg.conv_stride[0] + 1

    def conv0(s, w, mut):
        h = F.conv1d(s["x"][None, None], w[fe + "0.conv.weight"], stride=cfg.conv_stride[0])
        h = F.group_norm(h, c, w[fe + "0.layer_norm.weight"], w[fe + "0.layer_norm.bias"], 1e-5)
        return F.gelu(h)[0].t()
    st = [stage("conv0+group_norm+gelu", [("ops.wave_conv1d", dict(stride=cfg.conv_stride[0])),
                                          ("ops.groupnorm", dict(groups=c, eps=1e-5, silu=ACT_GELU, frames=1, hw=T, pad_hw=None))],
                conv0)]
    gelu = ("ops.gemm", dict(act=ACT_GELU, out_f32=False, alpha=1.0))
    lin = ("ops.gemm", dict(act=ACT_NONE, out_f32=False, alpha=1.0))
    ln = ("ops.layernorm", dict(eps=eps, add=None))
    from_prev = lambda recs, prev, case: {"x": prev.out.double().reshape(-1, prev.out.shape[-1])}      # noqa: E731
    for i in range(1, len(cfg.conv_dim)):
        k, s_ = cfg.conv_kernel[i], cfg.conv_stride[i]

        def conv(s, w, mut, i=i, s_=s_):
            p = fe + f"{i}.conv"
            h = F.conv1d(s["x"].t()[None], w[p + ".weight"], None if mut == "conv_bias" else w.get(p + ".bias"), stride=s_)
            if mut == "group_norm_layer1":
                h = F.group_norm(h, c, w[fe + "0.layer_norm.weight"], w[fe + "0.layer_norm.bias"], 1e-5)
            return F.gelu(h)[0].t()

        def windows(recs, prev, case, k=k, s_=s_):
            return [("overlapping rows of the time-major features", recs[0].inputs["a"],
                     prev.out.reshape(-1, c).unfold(0, k, s_).transpose(1, 2).reshape(-1, k * c))]
        st.append(stage(f"conv{i}", [gelu], conv, reads=from_prev, moves=windows))
        T = (T - k) // s_ + 1
    st.append(stage("feature_projection", [ln, lin],
                    lambda s, w, mut: L.linear(w, "feature_projection.projection",
                                               L.layer_norm(w, "feature_projection.layer_norm", s["x"], eps))))
    cg = Hd // G

    def pos(s, w, mut):
        x = s["x"]
        bias = None if mut == "pos_bias" else w["encoder.pos_conv_embed.conv.bias"]
        xt = x.t()[None]
        if mut == "pad_front_less":                        # kp / 2 - 1 zero rows in front, T outputs
            y = F.conv1d(F.pad(xt, (kp // 2 - 1, kp // 2)), _pos_weight(w, mut), bias, groups=G)
        else:
            y = F.conv1d(xt, _pos_weight(w, mut), bias, padding=kp // 2, groups=G)
            y = y[:, :, 1:] if mut == "drop_first" else y[:, :, :-1]          # Wav2Vec2SamePadLayer (kp even)
        return x + F.gelu(y)[0].t()

    def group_major(recs, prev, case, T=T):
        x = prev.out
        xg = torch.zeros((G, T + kp, cg), device=x.device, dtype=x.dtype)
        xg[:, kp // 2:kp // 2 + T] = x.view(T, G, cg).transpose(0, 1)
        return [(f"group {g_}: the padded group-major rows", recs[g_].inputs["a"],
                 xg[g_].unfold(0, kp, 1)[:T].transpose(1, 2).reshape(T, kp * cg)) for g_ in range(G)] + \
               [(f"group {g_}: the residual columns", recs[g_].inputs["residual"], x[:, g_ * cg:(g_ + 1) * cg])
                for g_ in range(G)]
    st.append(stage("positional_conv+residual", [gelu] * G, pos, reads=from_prev, moves=group_major,
                    got=lambda recs: torch.cat([r.out for r in recs], dim=1)))
    st.append(stage("encoder.layer_norm", [ln], lambda s, w, mut: L.layer_norm(w, "encoder.layer_norm", s["x"], eps)))
    for i in range(cfg.num_hidden_layers):
        p = f"encoder.layers.{i}"
        st.append(stage(f"layers.{i}.attention", [("blocks._self_attention", dict(heads=heads, seqs=1, n_tok=T, rows_per_item=0))],
                        lambda s, w, mut, p=p: _w2v_layer_attn(w, p, s["x"], heads, mut),
                        reads=lambda recs, prev, case: {"x": recs[0].inputs["h"].double()}, got=lambda recs: recs[0].after["h"]))
        st.append(stage(f"layers.{i}.layer_norm", [ln], lambda s, w, mut, p=p: L.layer_norm(w, p + ".layer_norm", s["x"], eps)))

        def ff(s, w, mut, p=p):
            x = s["x"]
            f = L.linear(w, p + ".feed_forward.output_dense", F.gelu(L.linear(w, p + ".feed_forward.intermediate_dense", x)))
            return x + (L.layer_norm(w, p + ".final_layer_norm", f, eps) if mut == "final_ln_before_residual" else f)
        st.append(stage(f"layers.{i}.feed_forward", [gelu, lin], ff))
        st.append(stage(f"layers.{i}.final_layer_norm", [ln],
                        lambda s, w, mut, p=p: L.layer_norm(w, p + ".final_layer_norm", s["x"], eps)))
    return st


# ------------------------------------------------------------------------------------------------ mutants
# model -> [(stage the edit touches, mutant of that stage's reference)]
MUTANTS = {
    "vae_decode": [("mid.attention", "to_q_bias"), ("mid.attention", "to_out_bias"), ("mid.attention", "no_residual"),
                   ("mid.attention", "heads8"), ("up.2.resnets.0", "shortcut_bias"), ("post_quant_conv+conv_in", "post_quant_bias"),
                   ("up.0.upsampler", "hw_swap"), ("up.1.upsampler", "hw_swap"), ("up.2.upsampler", "hw_swap")],
    "vae_decode_video": [("chunk0.scale+layout_in", "times_scaling_factor")],
    "vae_encode": [("mid.attention", "to_q_bias"), ("mid.attention", "to_out_bias"), ("mid.attention", "no_residual"),
                   ("mid.attention", "heads8"), ("down.1.resnets.0", "shortcut_bias"), ("down.0.downsampler", "pad_symmetric"),
                   ("down.2.downsampler", "pad_symmetric"), ("mean+layout_out", "mean_second_half"),
                   ("conv_norm_out+conv_out+quant_conv", "quant_bias")],
    "wav2vec2": [("layers.0.attention", "q_bias"), ("layers.0.attention", "q_scaled_before_bias"), ("layers.0.attention", "out_bias"),
                 ("layers.0.attention", "pre_ln"), ("layers.0.feed_forward", "final_ln_before_residual"),
                 ("positional_conv+residual", "drop_first"), ("positional_conv+residual", "pad_front_less"),
                 ("positional_conv+residual", "weight_norm_out_channel"), ("positional_conv+residual", "pos_bias"),
                 ("conv1", "conv_bias"), ("conv1", "group_norm_layer1")],
    "audio_projection": [("pos_emb+proj_in", "pos_emb_dropped"), ("pos_emb+proj_in", "pos_emb_shifted"),
                         ("layers.0.attention", "norms_swapped"), ("layers.0.attention", "scale_once"),
                         ("layers.0.feed_forward", "ff_no_residual"), ("proj_out+norm_out", "norm_out_first"),
                         ("layers.1.attention", "latents_frame0")],
    "kps_guider": [("blocks.0", "stride_even"), ("blocks.1", "stride_even"), ("conv_out", "silu_after"), ("blocks.2", "bias"),
                   ("conv_in", "bias")],
}
# Mutants no stage bound can see, pinned where the tensor they corrupt is visible: {model: {(stage, mutant): where}}
_BQKV = "the prepared bqkv tensor against its float64 statement (test_fused_qkv_biases_equal_their_float64_statement)"
PINNED = {
    "vae_decode": {("mid.attention", "to_q_bias"): _BQKV}, "vae_encode": {("mid.attention", "to_q_bias"): _BQKV},
    "wav2vec2": {("layers.0.attention", "q_bias"): _BQKV, ("layers.0.attention", "q_scaled_before_bias"): _BQKV},
}


def model_level_mutants(case):
    """The mutants as edits of the WHOLE model: the guider's stride pattern exchanged on every block at once."""
    out = []
    for name, mut in mutants(case):
        m = ("blocks.*", mut) if mut == "stride_even" else (name, mut)
        if m not in out:
            out.append(m)
    return out
# ("conv1", "conv_bias") exists only where the case carries convolution biases (the small wav2vec2 case: docstring)

VAE_FULL = dict(block_out_channels=(128, 256, 512, 512))           # sd-vae-ft-mse
GEOMETRIES = {
    "vae_decode": ("small", "full"), "vae_decode_video": ("small",), "vae_encode": ("small", "full"),
    "wav2vec2": ("small", "base"), "audio_projection": ("small", "full"), "kps_guider": ("small", "full"),
}
LAT_H, LAT_W, N_FRAMES = 8, 12, 2                                  # non-square latents, two frames of different content
VIDEO_FRAMES = 3                                                   # decode_video / encode_video: chunks of 2 + 1


def mutants(case):
    out = MUTANTS[case.model]
    if case.model == "wav2vec2" and not case.conv_bias:
        out = [m for m in out if m != ("conv1", "conv_bias")]
    return out


# ------------------------------------------------------------------------------------------------ cases
def _frames(shape, seed, lo=0.0, hi=1.0, scale=None):
    """Frames of different content AND different statistics (frame i shifted and scaled), on the CPU generator."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) if scale is not None else torch.rand(*shape, generator=g) * (hi - lo) + lo
    return x * (scale or 1.0)


def make_case(model, geo, *, device, elem, chunk=None):
    """The model object with seeded synthetic weights on `device` in `elem`, its inputs, its stage table and its raw
    state_dict in float64.  Built once per (model, geometry, device, element type) by the callers and left unchanged."""
    import v_express_amd as vx
    from v_express_amd import synth
    cs = SimpleNamespace(model=model, geo=geo, device=torch.device(device), elem=elem, conv_bias=False)
    if model.startswith("vae"):
        cfg = synth.VaeConfig(**(cases.SMALL_VAE if geo == "small" else VAE_FULL))
        sd = {**synth.vae_decoder_state_dict(cfg), **synth.vae_encoder_state_dict(cfg)}
        m = vx.AutoencoderKL(cfg)
        m.load_state_dict(sd)
        if model == "vae_decode":
            z = _frames((N_FRAMES, 4, LAT_H, LAT_W), 31, scale=1.0) * torch.tensor([1.0, 1.5]).view(-1, 1, 1, 1)
            cs.inputs, cs.stages = {"x": z}, vae_decode_stages(cfg, N_FRAMES, LAT_H, LAT_W)
            cs.call = lambda: m.decode(z.to(device)).sample
        elif model == "vae_decode_video":
            lat = _frames((1, 4, VIDEO_FRAMES, LAT_H, LAT_W), 32, scale=0.18215) * torch.tensor([1.0, 1.5, 0.7]).view(1, 1, -1, 1, 1)
            cs.chunk = chunk or 2
            cs.inputs, cs.stages = {"latents": lat}, vae_decode_video_stages(cfg, VIDEO_FRAMES, LAT_H, LAT_W, cs.chunk)
            cs.call = lambda: m.decode_video(lat.to(device), chunk=cs.chunk)
        else:
            x = _frames((N_FRAMES, 3, 8 * LAT_H, 8 * LAT_W), 33, lo=-1.0, hi=1.0) * torch.tensor([1.0, 0.6]).view(-1, 1, 1, 1)
            cs.inputs, cs.stages = {"x": x}, vae_encode_stages(cfg, N_FRAMES, 8 * LAT_H, 8 * LAT_W)
            cs.call = lambda: m.encode(x.to(device)).latent_dist.mean
    elif model == "wav2vec2":
        kw, samples = cases.W2V_CASES[geo]
        cfg = synth.Wav2Vec2Config(**kw)
        sd = synth.wav2vec2_state_dict(cfg)
        sd.pop("masked_spec_embed", None)
        m = vx.Wav2Vec2Model(cfg)
        m.load_state_dict(sd)
        if geo == "small":                                 # convolution biases behind the strict schema (docstring)
            g = torch.Generator().manual_seed(34)
            bias = {f"feature_extractor.conv_layers.{i}.conv.bias": 0.1 * torch.randn(cfg.conv_dim[i], generator=g)
                    for i in range(1, len(cfg.conv_dim))}
            sd.update(bias)
            m._raw.update(bias)
            m._invalidate()
            cs.conv_bias = True
        wav = cases.waveform(samples)[0]
        cs.inputs, cs.stages = {"x": wav}, w2v_stages(cfg, samples)
        cs.call = lambda: m.encode(wav.to(device))
    elif model == "audio_projection":
        cfg = synth.AudioProjectionConfig(**(cases.AUDIO_SMALL if geo == "small" else {}))
        sd = synth.audio_projection_state_dict(cfg)
        m = vx.AudioProjection(dim=cfg.dim, depth=cfg.depth, dim_head=cfg.dim_head, heads=cfg.heads, num_queries=cfg.num_queries,
                               embedding_dim=cfg.embedding_dim, output_dim=cfg.output_dim, max_seq_len=cfg.max_seq_len)
        m.load_state_dict(sd)
        x = cases.prologue_inputs()["audio_windows_small" if geo == "small" else "audio_windows_full"]
        cs.inputs, cs.stages = {"x": x}, audio_stages(cfg, x.shape[0], x.shape[1])
        cs.call = lambda: m(x.to(device))
    elif model == "kps_guider":
        cfg = synth.KpsGuiderConfig(**(cases.KPS_SMALL if geo == "small" else {}))
        sd = synth.kps_guider_state_dict(cfg)
        m = vx.VKpsGuider(cfg.conditioning_embedding_channels, block_out_channels=cfg.block_out_channels)
        m.load_state_dict(sd)
        x = cases.prologue_inputs()["kps_images"]          # [1, 3, 3, 64, 48]
        cs.inputs, cs.stages = {"x": x}, kps_stages(cfg, x.shape[2], x.shape[3], x.shape[4])
        cs.call = lambda: m.forward_tokens(x.to(device))[0]
    else:
        raise ValueError(model)
    cs.net, cs.cfg = m.to(device).to(elem), cfg
    cs.w64 = {k: v.to(device=device, dtype=torch.float64) for k, v in sd.items()}
    cs.inputs = {k: v.to(device) for k, v in cs.inputs.items()}
    return cs


# ------------------------------------------------------------------------------------------------ running and comparing
def run(case):
    """The model's own entry point on the case's inputs through `ops` as it stands -> its output."""
    with torch.no_grad():
        return case.call()


def record(case, tap):
    tap.clear()
    out = run(case)
    return list(tap.calls), out


def emulated(case, monkeypatch_context, tap_cls=None):
    """record() (or run(), without a tap class) with tests/fake_ops.py standing in for the kernels: float64 arithmetic,
    element-type rounding at every kernel boundary, on the case's device."""
    import fake_ops
    from v_express_amd import blocks, ops
    with monkeypatch_context() as mp:
        fake_ops.install(mp, ops)
        mp.setattr(fake_ops, "BF16", case.elem)
        mp.setattr(ops, "_PADDED", {})
        if tap_cls is None:
            return run(case)
        return record(case, tap_cls(ops, blocks).install(mp))


def check_sequence(case, calls):
    """The tapped call sequence EQUALS the stage table, and every call received the scalar arguments the table states."""
    want = [(st.name, name, sc) for st in case.stages for name, sc in st.calls]
    got, names = [c.name for c in calls], [n for _, n, _ in want]
    at = next((i for i, (a, b) in enumerate(zip(got, names)) if a != b), min(len(got), len(names)))
    where = want[at][0] if at < len(want) else "behind the last stage"
    assert got == names, (f"{case.model}/{case.geo}: the call sequence leaves the stage table at call {at} (stage {where}): "
                          f"{got[at] if at < len(got) else 'no call'} for {names[at] if at < len(names) else 'no call'}; "
                          f"{len(got)} calls, the table has {len(names)}")
    for c, (stage_name, name, scalars) in zip(calls, want):
        for k, v in scalars.items():
            have = c.scalars.get(k, "<absent>")
            same = k in c.scalars and have == v and isinstance(have, bool) == isinstance(v, bool)
            assert same, (f"{case.model}/{case.geo} stage {stage_name}: {name} received {k}={have!r}, the reference has {v!r}")


def split(case, calls):
    """-> [(stage, its records, the record in front of it)]"""
    out, i = [], 0
    for st in case.stages:
        out.append((st, calls[i:i + len(st.calls)], calls[i - 1] if i else None))
        i += len(st.calls)
    return out


def errors(got, ref):
    """(relative L2, max|err| / max|ref|) of got against the float64 reference; another SHAPE is infinitely far."""
    if got.numel() != ref.numel():
        return float("inf"), float("inf")
    g, r = got.double().reshape(ref.shape), ref.double()
    d = g - r
    return (d.norm() / (r.norm() + 1e-300)).item(), (d.abs().max() / (r.abs().max() + 1e-300)).item()


def within(err, e_emul, factor=3.0):
    return err[0] <= factor * e_emul[0] and err[1] <= factor * e_emul[1]


def stage_results(case, calls):
    """{stage name: (product output, float64 reference on the product's own stage input, state the stage read)}; the
    bit-equal data movement of every stage is asserted on the way."""
    out = {}
    with torch.no_grad():
        for st, recs, prev in split(case, calls):
            state = st.reads(recs, prev, case)
            ref, got = st.ref(state, case.w64, None), st.got(recs)
            for what, g, want in (st.moves(recs, prev, case) if st.moves else ()):
                assert g.shape == want.shape and torch.equal(g, want), f"{case.model}/{case.geo} stage {st.name}: {what} moved"
            if st.exact:
                assert torch.equal(got, ref.to(got.dtype).reshape(got.shape)), \
                    f"{case.model}/{case.geo} stage {st.name}: pure data movement is not bit-equal"
            out[st.name] = (got, ref, state)
    return out


def chain(case, mutant=None):
    """The whole model in float64: the stage references chained from the case's inputs (mutant: (stage, edit); a stage
    name ending in "*" edits every stage that starts with it)."""
    state = {k: v.double() for k, v in case.inputs.items()}
    if case.model == "audio_projection":
        state["lat"] = case.w64["latents"][0].repeat(case.inputs["x"].shape[0], 1)
    with torch.no_grad():
        for st in case.stages:
            hit = mutant is not None and (mutant[0] == st.name or (mutant[0].endswith("*") and st.name.startswith(mutant[0][:-1])))
            mut = mutant[1] if hit else None
            state[st.put] = st.ref(state, case.w64, mut)
    return state[case.stages[-1].put]


def bqkv_statement(case, mut=None):
    """{name: (prepared float32 bqkv, its float64 statement q | k | v)} of every fused QKV bias of the case's model.
    mut: the statement with the query bias dropped ("q_bias") or divided by the softmax scale, as a query scaled BEFORE its
    bias is added would need it ("q_scaled_before_bias": (x W s + b) = s (x W + b / s))."""
    out = {}
    w = dict(case.w64)
    for k in [k for k in w if k.endswith(("to_q.bias", "q_proj.bias"))]:
        if mut in ("q_bias", "to_q_bias"):
            w[k] = torch.zeros_like(w[k])
        elif mut == "q_scaled_before_bias":
            w[k] = w[k] * (w[k].shape[0] // case.cfg.num_attention_heads) ** 0.5
    if case.model.startswith("vae"):
        for half, P in (("decoder", case.net._prepared()), ("encoder", case.net._prepared_encoder())):
            p = half + ".mid_block.attentions.0"
            out[p] = (P["mid.attn"].attn.bqkv, torch.cat([w[f"{p}.to_{n}.bias"] for n in "qkv"]))
    elif case.model == "wav2vec2":
        for i, Lyr in enumerate(case.net._prepared().layers):
            p = f"encoder.layers.{i}.attention"
            out[p] = (Lyr.attn.bqkv, torch.cat([w[f"{p}.{n}_proj.bias"] for n in "qkv"]))
    return out
