"""float64 restatements of three-row guidance (TEST INFRASTRUCTURE) for tests/test_audio_guidance_cpu.py and
tests/test_gpu_audio_guidance.py: the guided prediction g = u + s (m - u) + s_a (c - m) of a separate audio scale (u: no
condition; m, "silent": reference bank + keypoints, zero audio; c: everything), its rescale towards std(c) (diffusers'
`rescale_noise_cfg` with the fully conditional row as the target), the row rule, and emulated `ops.combine_units3` /
`ops.guidance_rescale3` in the style of tests/fake_ops.py and guidance_restated.py.  The loop that uses them is
tests/loop_restated.py."""
import math

import torch

import guidance_restated as G

CHUNK = G.CHUNK
ROWS = {"u": (0, 0, 0), "m": (1, 1, 0), "c": (1, 1, 1)}          # (bank row, keypoint row, audio row), row 0 = zeros


def rows_for(s, s_a):
    """The rows of a guided step for the scales (s, s_a), restated from the issue's table."""
    if s_a is None or s_a == s:
        return ("u", "c") if s > 1.0 else ("c",)
    if s > 1.0:
        return ("u", "m", "c")
    return ("m", "c") if s_a > 1.0 else ("c",)


def combine3(u, m, c, s, s_a):
    """float64 u + s (m - u) + s_a (c - m)."""
    u, m, c = u.double(), m.double(), c.double()
    return u + s * (m - u) + s_a * (c - m)


def combine3_rescaled(u, m, c, s, s_a, phi):
    """u, m, c [nW, ...] float32 -> float64 g (1 + phi (std(c) / std(g) - 1)) per window."""
    g = combine3(u, m, c, s, s_a)
    return torch.stack([G.rescale(g[w], c[w], phi) for w in range(g.shape[0])])


def float32_baseline_error3(u, m, c, s, s_a, phi):
    """max |err| of the same formula evaluated by float32 torch.std on the CPU against float64: the yardstick of the
    kernel's bound (as guidance_restated.float32_baseline_error for the two-row op)."""
    g = (u + s * (m - u)) + s_a * (c - m)
    out = torch.stack([g[w] * (1.0 + phi * (c[w].std() / g[w].std() - 1.0)) for w in range(g.shape[0])])
    return (out.double() - combine3_rescaled(u, m, c, s, s_a, phi)).abs().max().item()


def units3(gathered, unit_index, c, f, hw):
    """The all-gathered buffer seen through a three-row unit_index: (u, m, c) float32 [nW, c, f, hw]."""
    nW, rows, S = unit_index.shape
    assert rows == 3
    g = gathered.reshape(-1, (f // S) * hw, c)
    h = g.index_select(0, unit_index.reshape(-1).long()).view(nW, rows, f, hw, c).permute(1, 0, 4, 2, 3)
    return h[0], h[1], h[2]


def combine_units3(gathered, unit_index, c, f, hw, guidance, audio_guidance, preds):
    """Emulated ops.combine_units3: (u + s (m - u)) + s_a (c - m) in float64, one float32 store."""
    u, m, cnd = (x.double() for x in units3(gathered, unit_index, c, f, hw))
    preds.copy_((u + guidance * (m - u)) + audio_guidance * (cnd - m))


def guidance_rescale3(gathered, unit_index, c, f, hw, guidance, audio_guidance, phi, workspace, preds):
    """Emulated ops.guidance_rescale3: the partials and the merge of guidance_restated.guidance_rescale, over the
    fully conditional row and the three-row g."""
    nW = unit_index.shape[0]
    assert unit_index.shape[1] == 3 and 0.0 <= phi <= 1.0
    assert workspace.numel() >= nW * f * ((hw + CHUNK - 1) // CHUNK) * 6
    u, m, cond = units3(gathered, unit_index, c, f, hw)
    g = ((u.double() + guidance * (m.double() - u.double())) + audio_guidance * (cond.double() - m.double())).float()
    out = torch.empty_like(g)
    for w in range(nW):
        factor = 1.0
        if phi != 0.0:
            n, mean, m2 = 0.0, [0.0, 0.0], [0.0, 0.0]
            for li in range(f):
                for p0 in range(0, hw, CHUNK):
                    nb = None
                    for t, x in enumerate((cond, g)):
                        v = x[w, :, li, p0:p0 + CHUNK].double()
                        nb, mb = float(v.numel()), v.mean().item()
                        qb = ((v - mb) ** 2).sum().item()
                        delta = mb - mean[t]
                        mean[t] += delta * (nb / (n + nb))
                        m2[t] += qb + delta * delta * (n * nb / (n + nb))
                    n += nb
            factor = 1.0 + phi * (math.sqrt(m2[0] / m2[1]) - 1.0)
        out[w] = (g[w].double() * factor).float()
    preds.copy_(out)
