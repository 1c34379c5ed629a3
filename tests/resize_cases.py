"""The latent resize restated (TEST INFRASTRUCTURE, shared by the CPU and the GPU suite): the per-axis tap tables of
torch.nn.functional.interpolate(align_corners=False, antialias=False) in float64, a float64 reference over them, a
float32 stand-in that follows the summation order of vx_latent_resize (include/vexpress_hip_resize.h), the derived
error bound, the cases and the mutants every case set must catch."""
import torch

U = 2.0 ** -24
TAPS = {"bilinear": 2, "bicubic": 4}
# the nine shapes (h, w, h2, w2) on which the tables are compared with F.interpolate
TABLE_SHAPES = [(5, 7, 8, 11), (8, 8, 16, 16), (16, 8, 24, 12), (6, 6, 3, 3), (1, 1, 4, 4), (8, 8, 8, 8), (8, 8, 32, 32),
                (3, 2, 7, 9), (8, 8, 12, 12)]
# (planes, h, w, h2, w2, mode): small integers in, every product and sum exact in float32 - bit for bit
EXACT_CASES = [(3, h, w, h2, w2, mode) for mode in ("bilinear", "bicubic")
               for h, w, h2, w2 in ((8, 8, 16, 16), (6, 6, 3, 3), (8, 8, 8, 8), (1, 1, 4, 4))] + \
              [(3, 8, 8, 32, 32, "bilinear")]
# Gaussian planes, judged by resize_bound: a quad tail and a non-square ratio, three awkward small ones, the real shape
BOUND_CASES = [(p, h, w, h2, w2, mode) for mode in ("bilinear", "bicubic")
               for p, h, w, h2, w2 in ((3, 5, 7, 8, 11), (2, 3, 2, 7, 9), (2, 16, 8, 24, 12), (2, 8, 8, 12, 12),
                                       (64, 64, 64, 96, 96))]


def case_id(case):
    p, h, w, h2, w2, mode = case
    return f"{mode}-P{p}-{h}x{w}-to-{h2}x{w2}"


# ------------------------------------------------------------------------------------------------ tables
def cubic_weights(t, A=-0.75):
    """The cubic convolution weights of the taps i - 1, i, i + 1, i + 2 at the fraction t (Keys' kernel, parameter A)."""
    def near(x):                                  # |x| <= 1
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    # the outer taps, A (|x| - 1) (|x| - 2)^2 at |x| = 1 + t and 2 - t, in the factored form: expanded in |x| the terms
    # cancel from 6 down to 0.1 and the four weights miss the sum 1 by up to 1e-15
    return torch.stack([A * t * (1.0 - t) * (1.0 - t), near(t), near(1.0 - t), A * (1.0 - t) * t * t], dim=1)


def taps(n_in, n_out, mode, mutant=None):
    """(indices int64 [n_out, taps], weights float64 [n_out, taps]) of one axis.  bilinear: s = max(scale (d + 0.5) - 0.5,
    0), i0 = min(floor(s), n_in - 1), i1 = min(i0 + 1, n_in - 1), t = s - i0; bicubic: s unclamped, i = floor(s), the taps
    i - 1 .. i + 2 clamped into [0, n_in - 1], the cubic convolution of t = s - i with A = -0.75.
    `mutant`: one of the per-axis MUTANTS (indices may then leave the range: `gather` reads zeros there)."""
    d = torch.arange(n_out, dtype=torch.float64)
    scale = n_in / n_out
    if mutant == "align_corners":
        s = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    elif mutant == "no_half_pixel":
        s = d * scale
    else:
        s = scale * (d + 0.5) - 0.5
    clamp = mutant != "no_border_clamp"
    if mode == "bilinear":
        if mutant == "unclamped_s":
            i0 = s.trunc()                        # a cast to int of a negative s: 0, and t = s < 0 extrapolates
        else:
            s = s.clamp_min(0.0)
            i0 = s.floor()
        if clamp:
            i0 = i0.clamp_max(n_in - 1)
        t = s - i0
        i1 = i0 + 1
        idx, wts = torch.stack([i0, i1.clamp_max(n_in - 1) if clamp else i1], dim=1), torch.stack([1.0 - t, t], dim=1)
    else:
        i = s.floor()
        idx = torch.stack([i - 1, i, i + 1, i + 2], dim=1)
        wts = cubic_weights(s - i, -0.5 if mutant == "A_minus_half" else -0.75)
        if mutant == "renormalised":
            # the taps outside the plane dropped and the others scaled to sum to 1 (what an antialias filter does)
            inside = ((idx >= 0) & (idx <= n_in - 1)).double()
            wts = wts * inside / (wts * inside).sum(dim=1, keepdim=True)
        if clamp:
            idx = idx.clamp(0, n_in - 1)
    return idx.long(), wts


def tables(h, w, h2, w2, mode, mutant=None):
    """(iy, wy, ix, wx) in float64 / int64."""
    if mutant == "swapped_axes":                  # the x table used for the rows and the y table for the columns
        (ix, wx), (iy, wy) = taps(h, h2, mode), taps(w, w2, mode)
        return _fit(iy, h2, h), _fit(wy, h2), _fit(ix, w2, w), _fit(wx, w2)
    return taps(h, h2, mode, mutant) + taps(w, w2, mode, mutant)


def _fit(t, n, limit=None):
    """Rows 0 .. n - 1 of a table of another length (cyclically), indices kept inside the plane."""
    t = t[torch.arange(n) % t.shape[0]]
    return t if limit is None else t.clamp_max(limit - 1)


def f32_tables(h, w, h2, w2, mode):
    """The tables as the kernel receives them: int32 indices, the float64 weights rounded once to float32."""
    iy, wy, ix, wx = tables(h, w, h2, w2, mode)
    return iy.to(torch.int32).contiguous(), wy.float().contiguous(), ix.to(torch.int32).contiguous(), wx.float().contiguous()


# ------------------------------------------------------------------------------------------------ evaluation
def gather(x, iy_a, ix_b):
    """x [P, h, w] at the rows iy_a [h2] and the columns ix_b [w2] -> [P, h2, w2]; zeros outside the plane."""
    _, h, w = x.shape
    ok = ((iy_a >= 0) & (iy_a < h))[:, None] & ((ix_b >= 0) & (ix_b < w))[None, :]
    return x[:, iy_a.clamp(0, h - 1)][:, :, ix_b.clamp(0, w - 1)] * ok.to(x.dtype)


def apply_tables(x, iy, wy, ix, wx):
    """sum_a wy[y, a] sum_b wx[x, b] x[iy[y, a], ix[x, b]] in the dtype of x / the weights: rows outer, columns inner, taps
    ascending, the first term of each sum initialising it - the order of the kernel."""
    out = None
    for a in range(wy.shape[1]):
        r = None
        for b in range(wx.shape[1]):
            term = wx[None, None, :, b] * gather(x, iy[:, a], ix[:, b])
            r = term if r is None else r + term
        term = wy[None, :, a, None] * r
        out = term if out is None else out + term
    return out


def reference(x, h2, w2, mode, mutant=None):
    """The float64 resize of planes x [P, h, w] (any float dtype) -> [P, h2, w2]."""
    x = x.double()
    if mutant == "nearest":
        iy = (torch.arange(h2, dtype=torch.float64) * (x.shape[1] / h2)).floor().long().clamp_max(x.shape[1] - 1)
        ix = (torch.arange(w2, dtype=torch.float64) * (x.shape[2] / w2)).floor().long().clamp_max(x.shape[2] - 1)
        return gather(x, iy, ix)
    out = apply_tables(x, *tables(x.shape[1], x.shape[2], h2, w2, mode, mutant))
    if mutant == "input_plane_stride":
        # plane p stored h * w elements after plane p - 1 instead of h2 * w2: in plane order, what fits the buffer
        flat, step = torch.zeros(out.numel(), dtype=out.dtype), x.shape[1] * x.shape[2]
        for p in range(out.shape[0]):
            n = max(0, min(h2 * w2, flat.numel() - p * step))
            flat[p * step:p * step + n] = out[p].flatten()[:n]
        return flat.view_as(out)
    return out


def standin_planes(x, h2, w2, mode):
    """vx_latent_resize in float32 torch on the CPU: the float32 tables, the kernel's order, one rounding per product and
    per sum (torch's elementwise float32 kernels do not contract) - the bits of the kernel."""
    assert x.dtype == torch.float32
    iy, wy, ix, wx = f32_tables(x.shape[1], x.shape[2], h2, w2, mode)
    return apply_tables(x, iy.long(), wy, ix.long(), wx)


def latent_resize(latents, size, mode="bilinear"):
    """The stand-in with the signature of ops.latent_resize: [1, C, F, h, w] -> a new [1, C, F, h2, w2]."""
    _, c, F, h, w = latents.shape
    h2, w2 = size
    return standin_planes(latents.reshape(c * F, h, w), h2, w2, mode).reshape(1, c, F, h2, w2).contiguous()


def resize_bound(x, h2, w2, mode):
    """|float32 result - float64 reference| <= K u / (1 - K u) * sum_ab |wy_a| |wx_b| |x_ab| per output, u = 2^-24.
    K counts the roundings that reach one term wy_a wx_b x_ab in the kernel's order:
        2   the two weights, each rounded once from float64 to float32
        2   the two products (wx_b * x, then wy_a * row sum)
        taps - 1   the additions of the row sum that the term passes through, at most
        taps - 1   the additions of the column sum
    K = 2 taps + 2 (6 bilinear, 10 bicubic); (1 + u)^K - 1 <= K u / (1 - K u).  Derived, not measured.  (Gaussian data
    and weights of order 1: nothing underflows.)"""
    k = 2 * TAPS[mode] + 2
    iy, wy, ix, wx = tables(x.shape[1], x.shape[2], h2, w2, mode)
    mag = apply_tables(x.double().abs(), iy, wy.abs(), ix, wx.abs())
    return k * U / (1.0 - k * U) * mag


def case_input(case, exact):
    """The planes of a case: small integers in [-8, 8] (exact) or N(0, 1), seeded by the shape."""
    p, h, w, h2, w2, mode = case
    g = torch.Generator().manual_seed(1000 * h + 10 * w2 + p + TAPS[mode])
    if exact:
        return torch.randint(-8, 9, (p, h, w), generator=g).float()
    return torch.randn(p, h, w, generator=g)


# ------------------------------------------------------------------------------------------------ mutants
# wrong resizes a plausible implementation could compute; every one must be caught by at least one case
MUTANTS = {
    "align_corners": "the align_corners=True mapping s = d (n_in - 1) / (n_out - 1)",
    "no_half_pixel": "the half-pixel offset dropped: s = d n_in / n_out",
    "no_border_clamp": "a border clamp missing: a tap outside the plane does not read the border pixel",
    "unclamped_s": "the bilinear s left unclamped: a negative s truncates to 0 and extrapolates with t < 0",
    "A_minus_half": "the bicubic parameter A = -0.5",
    "swapped_axes": "the x and y tables swapped",
    "input_plane_stride": "a plane stride of h * w used for the output",
    "nearest": "nearest neighbour",
    "renormalised": "weights renormalised over the taps inside the plane",
}


def caught(mutant, case, exact):
    """Whether a kernel that computed `mutant` would fail `case`: other bits (exact) or an element outside the bound."""
    p, h, w, h2, w2, mode = case
    x = case_input(case, exact)
    ref, bad = reference(x, h2, w2, mode), reference(x, h2, w2, mode, mutant)
    if exact:
        return not torch.equal(bad.float(), ref.float())
    return bool(((bad.float().double() - ref).abs() > resize_bound(x, h2, w2, mode)).any())
