"""Block wiring cases (TEST INFRASTRUCTURE, host only, torch on any device): the geometries and inputs of the block-level
tests, a float64 reference of every block of v_express_amd/blocks.py computed from the RAW state_dict - unfolded weights,
the reference's own order of operations, through oracle/unet.py and oracle/leaf.py - and wiring mutants of that reference.

    case = make_case("read", c=64, f=4, H=4, W=4, combo="A", device="cpu", elem=torch.bfloat16)
    ref  = reference(case)                    # float64, [b f, hw, C] token layout like the product's
    out  = run(case, prepare(case))           # blocks.* on ops.* as they are (kernels, or tests/fake_ops.py once installed)
    bad  = reference(case, "w_swap")          # the same block wired wrongly

Inputs are chosen so that a wiring error cannot cancel: two batch items of different content, a temb row per item, one item
with a bank and one without, zero / non-zero audio per item (combo "A": item 0 bank-less with zero audio, item 1 banked with
audio; combo "B": item 0 bank-less with audio, item 1 banked with zero audio - together the four combinations), w_ref != w_aud
both != 1, every to_out bias non-zero, norm affine parameters as synth draws them, the sinusoid table distinct per frame.

A mutant is an edit of what the oracle is GIVEN for one batch item (its weights, its inputs), so the arithmetic stays the
oracle's: e.g. "the fold's bias taken from the gamma-scaled weight" (W o gamma) beta = W (gamma o beta) is the oracle with
the norm's beta replaced by gamma o beta.  Only the four-phase upsample has no oracle form: it is restated here
(`upsample_phases_ref`) and pinned to `oracle.leaf.upsample` by the CPU test.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import cases
from oracle import leaf as L
from oracle import unet as OU

HEADS, GROUPS, N_CTX, CTX_DIM = 8, 32, 5, 768
W_REF, W_AUD = cases.W_REF, cases.W_AUD
OCFG = SimpleNamespace(norm_num_groups=GROUPS, heads=HEADS)
P_ = "blk"                                   # key prefix of the block's state_dict
T_ = P_ + ".transformer_blocks.0"
M_ = P_ + ".temporal_transformer.transformer_blocks.0"
_ATTN_SCORES = 1 << 27                       # float64 scores held at once by the reference's spatial attention (1 GB)

X_SCALE = 0.25


def key_fold(c, heads):
    """The factor the product folds into its key weights, stated here on its own (not taken from weights.key_fold, so that
    a wrong factor there misses the folded tensors' bound): the softmax scale d^-1/2 times log2(e) of the base-2 kernels."""
    import math
    return (c // heads) ** -0.5 * math.log2(math.e)


KINDS = ("resnet", "downsample", "upsample", "read", "write", "motion", "bank_kv")
# wiring mutants of the reference that must land outside the route bound, per block kind
MUTANTS = {
    "read": ("item_bias_other", "w_swap", "drop_b15", "drop_b2", "key_fold_twice", "geglu_swap", "proj_out_residual_h",
             "bank_frame0"),
    "motion": ("pe_interleave", "geglu_swap", "proj_out_residual_h"),
    "resnet": ("temb_other", "concat_order"),
    "upsample": ("phase_tap",),
}
# Mutants of the load-time folds that NO block-level bound can see, with the norm affine parameters as synth draws them
# (gamma ~ 1 + 0.1 N, beta ~ 0.1 N) - measured on the CPU emulation, against e_emul of the block output:
#   fold bias from the gamma-scaled weight, (W o gamma) beta for W beta: the error is W (beta o (gamma - 1)), 1 % of the
#     projection's input - 1.2 x e_emul behind norm1, 0.1 x behind norm1_5 / norm2 (softmax averages it), 0.4 x behind norm3;
#   key fold not applied to the key bias: a constant added to every key moves every logit of a query by the same amount,
#     which the softmax cancels - the mutant is EQUIVALENT (1e-16 in float64), whatever the inputs.
# They are pinned where they are visible instead: tests/test_block_wiring_cpu.py compares every folded tensor of
# weights.prep_* with its float64 statement and asserts that these mutants miss THAT bound.
FOLD_MUTANTS = {
    "read": ("fold_bias_gamma:norm1", "fold_bias_gamma:norm1_5", "fold_bias_gamma:norm2", "fold_bias_gamma:norm3",
             "key_fold_bias"),
    "motion": ("fold_bias_gamma:norms.0", "fold_bias_gamma:norms.1", "fold_bias_gamma:ff_norm"),
}


class Case(SimpleNamespace):
    @property
    def frames(self):
        return self.b * self.f

    @property
    def hw(self):
        return self.H * self.W


def _gen(seed):
    from v_express_amd import synth
    return synth._Gen(seed)


def make_case(kind, *, c, f, H, W, device, elem, combo="A", b=2, skip=0, cout=None, temb_dim=64, gn_groups=GROUPS, seed=7):
    """kind: one of KINDS.  c: channels of x; skip: channels of the skip tensor (resnet); cout: resnet output channels
    (default c: no shortcut unless skip)."""
    from v_express_amd import synth
    g = _gen(seed + 1000 * KINDS.index(kind))
    scfg = SimpleNamespace(cross_attention_dim=CTX_DIM, temporal_max_len=32)
    cs = Case(kind=kind, c=c, f=f, H=H, W=W, b=b, combo=combo, device=torch.device(device), elem=elem, skip=skip,
              cout=cout or c, gn_groups=gn_groups, w_ref=W_REF, w_aud=W_AUD)
    if kind == "resnet":
        g.resnet(P_, c + skip, cs.cout, temb_dim)
    elif kind in ("downsample", "upsample"):
        g.conv(P_ + ".conv", c, c, 3)
    elif kind in ("read", "bank_kv"):
        synth._spatial_block_3d(g, P_, c, scfg)
    elif kind == "write":
        synth._spatial_block_2d(g, P_, c, scfg)
    elif kind == "motion":
        synth._motion_module(g, P_, c, scfg)
    cs.sd = g.sd
    rnd = torch.Generator().manual_seed(seed + 17)

    def draw(*shape, scale=1.0):
        return (torch.randn(*shape, generator=rnd) * scale).to(elem).to(cs.device)
    frames, hw = cs.frames, cs.hw
    # item 1 = item 0's distribution shifted and scaled: different content, different statistics per item
    x = torch.randn(b, f, hw, c, generator=rnd)
    x = x * torch.linspace(1.0, 1.6, b)[:, None, None, None] + torch.linspace(0.0, 0.4, b)[:, None, None, None]
    if kind in ("read", "write", "motion"):
        # these blocks end in `+ x` and normalise x on the way in: at unit scale the residual (and the rounding of the
        # output it dominates) hides the block's own term - a quarter of it shows 3 x more of every wiring mutant
        # (measured on the CPU emulation: the sinusoid mutant 5.1 x -> 14.7 x e_emul) and changes nothing inside the block
        x = x * X_SCALE
    cs.x = x.reshape(frames, hw, c).to(elem).to(cs.device)
    if kind == "resnet":
        cs.skip_x = draw(frames, hw, skip) if skip else None
        cs.emb = torch.randn(b, temb_dim, generator=rnd).to(cs.device)                 # float32, one row per item
    if kind in ("read", "write"):
        n_ctx = N_CTX if kind == "read" else 1
        cs.n_ctx = n_ctx
        ehs = torch.randn(b, f * n_ctx, CTX_DIM, generator=rnd)
        cs.has_bank = [False, True][:b] if kind == "read" else []
        # (combo "N": no zero-audio item - the batched audio launches)
        cs.audio_zero = {"A": [True, False], "B": [False, True], "N": [False, False]}[combo][:b] if kind == "read" \
            else [False] * b
        for bi in range(b):
            if cs.audio_zero[bi]:
                ehs[bi] = 0
        cs.ehs = ehs.reshape(frames * n_ctx, CTX_DIM).to(elem).to(cs.device)
        cs.bank_tokens = [draw(hw, c) if hb else None for hb in cs.has_bank]
    if kind == "bank_kv":
        cs.bank_tokens = [draw(hw, c)]
    return cs


def sd64(cs, device=None):
    return {k: v.to(device=device or cs.device, dtype=torch.float64) for k, v in cs.sd.items()}


# ------------------------------------------------------------------------------------------------ layouts
def to_nchw(x, H, W):
    return x.double().reshape(x.shape[0], H, W, -1).permute(0, 3, 1, 2)


def to_tokens(y):
    n, c, h, w = y.shape
    return y.permute(0, 2, 3, 1).reshape(n, h * w, c)


# ------------------------------------------------------------------------------------------------ the product's side
def prepare(cs):
    """The block's weights through the real load-time folds (v_express_amd.weights.prep_*), in the element type in force."""
    from v_express_amd import weights as Wt
    sd, dev = cs.sd, cs.device
    if cs.kind == "resnet":
        return Wt.prep_resnet(sd, P_, dev)
    if cs.kind == "downsample":
        return Wt.prep_conv(sd, P_ + ".conv", dev)
    if cs.kind == "upsample":
        P = Wt.prep_conv(sd, P_ + ".conv", dev)
        P["phases"] = Wt.fold_upsample_phases(sd, P_ + ".conv", dev)
        return P
    if cs.kind in ("read", "bank_kv"):
        return Wt.prep_spatial_read(sd, P_, dev, heads=HEADS)
    if cs.kind == "write":
        return Wt.prep_spatial_write(sd, P_, dev, heads=HEADS)
    return Wt.prep_motion(sd, P_, dev)


def temb_rows(cs):
    """time_emb_proj(silu(emb)) as float32 [b, Cout]: what UNet3DConditionModel._temb hands the block."""
    w, bias = cs.sd[P_ + ".time_emb_proj.weight"].to(cs.device).double(), cs.sd[P_ + ".time_emb_proj.bias"].to(cs.device).double()
    return (F.silu(cs.emb.double()) @ w.t() + bias).float().contiguous()


def run(cs, P, items=None):
    """blocks.<kind> on the case's inputs through `ops` as it stands -> the block's output(s), token layout.
    items: the batch items to run (default all), e.g. [1]: that item ALONE."""
    from v_express_amd import blocks as B
    sel = list(range(cs.b)) if items is None else list(items)
    b, f, H, W, hw = len(sel), cs.f, cs.H, cs.W, cs.hw

    def rows(t, per=1):
        if t is None:
            return None
        t = t.reshape(cs.b, -1, *t.shape[1:])
        return torch.cat([t[i] for i in sel]).contiguous()
    x = rows(cs.x)
    if cs.kind == "resnet":
        return B.resnet_block(P, x, b * f, H, W, groups=GROUPS, eps=1e-5, temb=temb_rows(cs)[sel].contiguous(),
                              rows_per_group=f * hw, skip=rows(cs.skip_x), items=b)
    if cs.kind == "downsample":
        return B.downsample(P, x, b * f, H, W, gn_groups=cs.gn_groups)[0]
    if cs.kind == "upsample":
        return B.upsample(P, x, b * f, H, W, items=b)[0]
    if cs.kind == "read":
        bank = [None if cs.bank_tokens[i] is None else B.bank_kv(P.attn1_5, cs.bank_tokens[i], HEADS) for i in sel]
        return B.spatial_transformer_read(P, x, b=b, f=f, H=H, W=W, heads=HEADS, groups=GROUPS, ehs=rows(cs.ehs),
                                          bank=bank, w_ref=cs.w_ref, w_aud=cs.w_aud,
                                          audio_zero=[cs.audio_zero[i] for i in sel])
    if cs.kind == "write":
        return B.spatial_transformer_write(P, x, frames=b * f, H=H, W=W, heads=HEADS, groups=GROUPS, ehs=rows(cs.ehs))
    if cs.kind == "motion":
        return B.motion_module(P, x, b=b, f=f, H=H, W=W, heads=HEADS, groups=GROUPS, gn_next=True)
    if cs.kind == "bank_kv":
        return B.bank_kv(P.attn1_5, cs.bank_tokens[0], HEADS)
    raise ValueError(cs.kind)


# ------------------------------------------------------------------------------------------------ the float64 reference
def _read_item(w, cs, bi, x, ehs, bank, w_ref, w_aud):
    """oracle.unet._spatial_transformer_read on ONE batch item, in frame chunks (the [heads, hw, hw] float64 scores of one
    frame: 151 MB at 1536 tokens); frames are independent in this block (the bank is shared by an item's frames)."""
    f, hw = cs.f, cs.hw
    step = max(1, min(f, _ATTN_SCORES // (HEADS * hw * max(hw, bank.shape[1]))))
    out = []
    for f0 in range(0, f, step):
        f1 = min(f, f0 + step)
        out.append(OU._spatial_transformer_read(w, P_, x[f0:f1], f1 - f0, ehs[f0:f1], bank, OCFG, w_ref, w_aud))
    return torch.cat(out)


def _gamma_beta(w, norm):
    w[norm + ".bias"] = w[norm + ".weight"] * w[norm + ".bias"]


def _swap_geglu(w, p):
    for k in (".net.0.proj.weight", ".net.0.proj.bias"):
        v, g = w[p + k].chunk(2, dim=0)
        w[p + k] = torch.cat([g, v], dim=0)


def reference(cs, mut=None):
    """The block in float64 from the raw state_dict, on the (element-type) inputs of the case.  mut: a name of MUTANTS."""
    w0 = sd64(cs)
    b, f, H, W, hw, c = cs.b, cs.f, cs.H, cs.W, cs.hw, cs.c
    kind = cs.kind
    with torch.no_grad():
        if kind == "resnet":
            x = to_nchw(cs.x, H, W)
            if cs.skip:
                sk = to_nchw(cs.skip_x, H, W)
                x = torch.cat([sk, x] if mut == "concat_order" else [x, sk], dim=1)
            emb = cs.emb.double()
            if mut == "temb_other":
                emb = emb.flip(0)
            # the product is handed float32 rows of time_emb_proj(silu(emb)): the reference computes them itself
            return to_tokens(L.resnet(w0, P_, x, emb.repeat_interleave(f, dim=0), GROUPS, 1e-5))
        if kind == "downsample":
            return to_tokens(L.downsample(w0, P_, to_nchw(cs.x, H, W)))
        if kind == "upsample":
            if mut == "phase_tap":
                return to_tokens(upsample_phases_ref(w0, P_, to_nchw(cs.x, H, W), misplace=True))
            return to_tokens(L.upsample(w0, P_, to_nchw(cs.x, H, W)))
        if kind == "bank_kv":
            t = cs.bank_tokens[0].double()
            return t @ w0[T_ + ".attn1_5.to_k.weight"].t(), t @ w0[T_ + ".attn1_5.to_v.weight"].t()
        if kind == "write":
            banks = {}
            y = OU._spatial_transformer_write(w0, P_, to_nchw(cs.x, H, W), cs.ehs.double().reshape(b * f, cs.n_ctx, CTX_DIM),
                                              OCFG, banks)
            return to_tokens(y), banks[P_].reshape(b * f * hw, c)
        if kind == "motion":
            outs = []
            for bi in range(b):
                w = dict(w0)
                x = to_nchw(cs.x[bi * f:(bi + 1) * f], H, W)
                if mut == "pe_interleave":
                    # A.pe_rows[:f].repeat_interleave(b): row j of the [b f] table is frame j // b, not j % f
                    idx = (torch.arange(bi * f, (bi + 1) * f, device=x.device) // b)
                    for i in range(2):
                        k = f"{M_}.attention_blocks.{i}.pos_encoder.pe"
                        w[k] = w[k][:, idx]
                elif mut and mut.startswith("fold_bias_gamma:"):
                    _gamma_beta(w, f"{M_}.{mut.split(':')[1]}")
                elif mut == "geglu_swap":
                    _swap_geglu(w, M_ + ".ff")
                y = OU._motion_module(w, P_, x, f, OCFG)
                if mut == "proj_out_residual_h":
                    tp = P_ + ".temporal_transformer"
                    h_in = L.linear(w, tp + ".proj_in", to_tokens(L.group_norm(w, tp + ".norm", x, GROUPS, 1e-6)))
                    y = y - x + to_nchw(h_in, H, W)
                outs.append(to_tokens(y))
            return torch.cat(outs)
        if kind == "read":
            zero_bank = torch.zeros(1, hw, c, dtype=torch.float64, device=cs.device)
            banks = [zero_bank if t is None else t.double()[None] for t in cs.bank_tokens]
            ehs = cs.ehs.double().reshape(b, f, cs.n_ctx, CTX_DIM)
            b15, b2 = T_ + ".attn1_5.to_out.0.bias", T_ + ".attn2.to_out.0.bias"
            outs = []
            for bi in range(b):
                w = dict(w0)
                x = to_nchw(cs.x[bi * f:(bi + 1) * f], H, W)
                w_ref, w_aud, bank = cs.w_ref, cs.w_aud, banks[bi]
                if mut == "item_bias_other":
                    # the constants of the bank-less (and zero-audio) item ride on the OTHER item's attn1 out-projection
                    other = (bi + 1) % b
                    me = (0 if cs.has_bank[bi] else 1, 1 if (not cs.has_bank[bi] and cs.audio_zero[bi]) else 0)
                    ot = (0 if cs.has_bank[other] else 1, 1 if (not cs.has_bank[other] and cs.audio_zero[other]) else 0)
                    extra = ot[0] * w_ref * w0[b15] + ot[1] * w_aud * w0[b2]
                    w[T_ + ".attn1.to_out.0.bias"] = w0[T_ + ".attn1.to_out.0.bias"] + extra
                    if me[0]:
                        w[b15] = torch.zeros_like(w0[b15])
                    if me[1]:
                        w[b2] = torch.zeros_like(w0[b2])
                elif mut == "w_swap":
                    w_ref, w_aud = w_aud, w_ref
                elif mut == "drop_b15" and not cs.has_bank[bi]:
                    w[b15] = torch.zeros_like(w0[b15])
                elif mut == "drop_b2" and cs.audio_zero[bi]:
                    w[b2] = torch.zeros_like(w0[b2])
                elif mut and mut.startswith("fold_bias_gamma:"):
                    _gamma_beta(w, f"{T_}.{mut.split(':')[1]}")
                elif mut in ("key_fold_bias", "key_fold_twice"):
                    kf = key_fold(c, HEADS)
                    wk = w0[T_ + ".attn1.to_k.weight"]
                    if mut == "key_fold_twice":
                        w[T_ + ".attn1.to_k.weight"] = wk * kf
                    else:      # k = kf (W gamma) xhat + W beta  =  kf (k_true + (1 / kf - 1) W beta)
                        w[T_ + ".attn1.to_k.bias"] = (1.0 / kf - 1.0) * (wk @ w0[T_ + ".norm1.bias"])
                elif mut == "geglu_swap":
                    _swap_geglu(w, T_ + ".ff")
                elif mut == "bank_frame0":
                    bank = banks[0]
                y = _read_item(w, cs, bi, x, ehs[bi], bank, w_ref, w_aud)
                if mut == "proj_out_residual_h":
                    h_in = L.conv2d(w, P_ + ".proj_in", L.group_norm(w, P_ + ".norm", x, GROUPS, 1e-6), padding=0)
                    y = y - x + h_in
                outs.append(to_tokens(y))
            return torch.cat(outs)
    raise ValueError(kind)


def upsample_phases_ref(w, p, x, misplace=False):
    """Nearest-2x + conv3x3 as four 2x2 convolutions over the original image, float64: output pixel (2y + a, 2x + b) reads
    input rows {y - 1 + a, y + a} and columns {x - 1 + b, x + b}; 3x3 taps landing on the same input pixel are added.
    misplace: tap (ky, kx) = (1, 1) of phase (0, 0) goes to the neighbouring phase (0, 1) instead (same window slot)."""
    wt, bias = w[p + ".conv.weight"], w[p + ".conv.bias"]
    cout, cin = wt.shape[:2]
    n, _, H, W = x.shape
    rows = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    ph = torch.zeros(2, 2, cout, cin, 2, 2, dtype=wt.dtype, device=wt.device)
    for a in (0, 1):
        for b in (0, 1):
            for dy, kys in enumerate(rows[a]):
                for dx, kxs in enumerate(rows[b]):
                    for ky in kys:
                        for kx in kxs:
                            ta, tb = (0, 1) if (misplace and (a, b, ky, kx) == (0, 0, 1, 1)) else (a, b)
                            ph[ta, tb, :, :, dy, dx] += wt[:, :, ky, kx]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.empty(n, cout, 2 * H, 2 * W, dtype=x.dtype, device=x.device)
    for a in (0, 1):
        for b in (0, 1):
            out[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], ph[a, b], bias)
    return out


# ------------------------------------------------------------------------------------------------ the load-time folds
def _interleave(t):
    half = t.shape[0] // 2
    v, g = t[:half].reshape(half // 8, 8, *t.shape[1:]), t[half:].reshape(half // 8, 8, *t.shape[1:])
    return torch.stack([v, g], dim=1).reshape(t.shape)


def _ln_fold(w, W, bias, norm, mut, interleave=False, k_rows=None, kf=1.0):
    """float64 statement of weights.fold_layernorm: (gamma o W, W beta + bias); k_rows: the rows carrying the key fold."""
    gamma, beta = w[norm + ".weight"], w[norm + ".bias"]
    scale = torch.ones(W.shape[0], dtype=W.dtype, device=W.device)
    if k_rows is not None:
        scale[k_rows] = kf
    Ws = W * scale[:, None]
    mine = mut is not None and mut.split(":")[-1] == norm.rsplit(".transformer_blocks.0.", 1)[-1]
    b = (Ws * gamma[None]) @ beta if (mine and mut.startswith("fold_bias_gamma")) else Ws @ beta
    if mut == "key_fold_bias" and k_rows is not None:
        b = W @ beta                                       # the weight rows scaled, the bias rows not
    if bias is not None:
        b = b + bias
    wf = Ws * gamma[None]
    return (_interleave(wf), _interleave(b)) if interleave else (wf, b)


def fold_statements(cs, mut=None):
    """{name: float64 tensor} of every tensor the load-time folds of weights.prep_spatial_read / prep_motion build, from the
    raw state_dict (weights.fold_layernorm, fold_ff_proj, fold_groupnorm, the key fold, the sinusoid rows)."""
    w, c, out = sd64(cs), cs.c, {}

    def ff_proj(ff, po):
        wp = w[po + ".weight"].reshape(c, c)
        out["ff_proj.w"] = torch.cat([wp, wp @ w[ff + ".net.2.weight"]], dim=1)
        out["ff_proj.b"] = w[po + ".bias"] + wp @ w[ff + ".net.2.bias"]

    def gn(norm, pi):
        out["gn_fold.bb"] = w[pi + ".bias"] + w[pi + ".weight"].reshape(c, c) @ w[norm + ".bias"]
    if cs.kind == "read":
        a1 = T_ + ".attn1"
        W = torch.cat([w[f"{a1}.{n}.weight"] for n in ("to_q", "to_k", "to_v")])
        out["ln_qkv.w"], out["ln_qkv.b"] = _ln_fold(w, W, None, T_ + ".norm1", mut, k_rows=slice(c, 2 * c),
                                                    kf=key_fold(c, HEADS))
        out["ln_q15.w"], out["ln_q15.b"] = _ln_fold(w, w[T_ + ".attn1_5.to_q.weight"], None, T_ + ".norm1_5", mut)
        out["ln_q2.w"], out["ln_q2.b"] = _ln_fold(w, w[T_ + ".attn2.to_q.weight"], None, T_ + ".norm2", mut)
        out["ln_ff.w"], out["ln_ff.b"] = _ln_fold(w, w[T_ + ".ff.net.0.proj.weight"], w[T_ + ".ff.net.0.proj.bias"],
                                                  T_ + ".norm3", mut, interleave=True)
        ff_proj(T_ + ".ff", P_ + ".proj_out")
        gn(P_ + ".norm", P_ + ".proj_in")
    else:
        for i in range(2):
            a = f"{M_}.attention_blocks.{i}"
            W = torch.cat([w[f"{a}.{n}.weight"] for n in ("to_q", "to_k", "to_v")])
            out[f"attn.{i}.ln_qkv.w"], out[f"attn.{i}.ln_qkv.b"] = _ln_fold(w, W, None, f"{M_}.norms.{i}", mut)
        out["ln_ff.w"], out["ln_ff.b"] = _ln_fold(w, w[M_ + ".ff.net.0.proj.weight"], w[M_ + ".ff.net.0.proj.bias"],
                                                  M_ + ".ff_norm", mut, interleave=True)
        ff_proj(M_ + ".ff", P_ + ".temporal_transformer.proj_out")
        gn(P_ + ".temporal_transformer.norm", P_ + ".temporal_transformer.proj_in")
    return out


def fold_tensors(P):
    """The same names from the prepared block."""
    out = {}
    for k in ("ln_qkv", "ln_q15", "ln_q2", "ln_ff"):
        if P.get(k) is not None:
            out[k + ".w"], out[k + ".b"], out[k + ".s"] = P[k].w, P[k].b, P[k].s
    for i, A in enumerate(P.get("attn") or ()):
        out[f"attn.{i}.ln_qkv.w"], out[f"attn.{i}.ln_qkv.b"], out[f"attn.{i}.ln_qkv.s"] = A.ln_qkv.w, A.ln_qkv.b, A.ln_qkv.s
    out["ff_proj.w"], out["ff_proj.b"], out["gn_fold.bb"] = P.ff_proj.w, P.ff_proj.b, P.gn_fold.bb
    return out


# ------------------------------------------------------------------------------------------------ measures
def errors(got, ref):
    """(relative L2, max|err| / max|ref|) of got against the float64 reference."""
    g, r = got.double().reshape(ref.shape), ref.double()
    d = g - r
    return (d.norm() / (r.norm() + 1e-300)).item(), (d.abs().max() / (r.abs().max() + 1e-300)).item()


def bank_kv_errors(cs, got, ref):
    """bank_kv's (k, vt, kmax) against (k, v) of the reference: k carries weights.key_fold, vt is [1, heads, d, pitch]."""
    k, vt, kmax = got
    n, c = ref[0].shape
    d = c // HEADS
    kf = key_fold(c, HEADS)
    v = vt[0, :, :, :n].double().permute(2, 0, 1).reshape(n, c)
    e = max(errors(k.double() / kf, ref[0]), errors(v, ref[1]))
    want = (ref[0] * kf).reshape(n, HEADS, d).norm(dim=-1).amax(dim=0)
    return e, ((kmax.double() - want).abs() / want).max().item()


def within(err, e_emul, factor=3.0):
    """The route bound: both measures within `factor` x the emulation's own error against float64 (never a fixed number)."""
    return err[0] <= factor * e_emul[0] and err[1] <= factor * e_emul[1]


def emulated(cs, P, monkeypatch_context, items=None):
    """run() with tests/fake_ops.py standing in for the kernels (float64 arithmetic, element-type rounding at every kernel
    boundary) - on the case's device, same routes (the `*_applies` rules are the product's own)."""
    import fake_ops
    from v_express_amd import ops
    with monkeypatch_context() as mp:
        fake_ops.install(mp, ops)
        mp.setattr(fake_ops, "BF16", cs.elem)
        mp.setattr(ops, "_PADDED", {})
        return run(cs, P, items)
