"""float64 restatements of the guidance controls (TEST INFRASTRUCTURE) for tests/test_guidance_cpu.py and
tests/test_gpu_guidance.py: the CFG rescale of Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed"
(diffusers' `rescale_noise_cfg`: g * (1 + phi (std(cond) / std(g) - 1)), unbiased std over everything but the batch
axis), the guidance-interval step rule (diffusers' control_guidance_start / _end convention), and an emulated
`ops.guidance_rescale` in the style of tests/fake_ops.py that forms and merges its partials in the kernel's order.  The
loop that uses them is tests/loop_restated.py."""
import math

import torch

import dpm_restated as D

KWARGS = D.KWARGS
CHUNK = 1024                      # pixels per partial of vx_guidance_rescale


def guided_steps(n, start=0.0, end=1.0):
    """Step i of n is guided iff i / n >= start and (i + 1) / n <= end."""
    out = []
    for i in range(n):
        out.append((i / n >= start) and ((i + 1) / n <= end))
    return out


def rescale(g, cond, phi):
    """rescale_noise_cfg on one window's prediction (any shape; the std runs over all of it), float64."""
    g, cond = g.double(), cond.double()
    return g * (1.0 + phi * (cond.std() / g.std() - 1.0))


def combine_rescaled(u, cond, guidance, phi):
    """u, cond [nW, ...] float32 -> float64 g' per window."""
    u, cond = u.double(), cond.double()
    g = u + guidance * (cond - u)
    return torch.stack([rescale(g[w], cond[w], phi) for w in range(g.shape[0])])


def float32_baseline_error(u, cond, guidance, phi):
    """max |err| of the same formula evaluated by float32 torch.std on the CPU against float64: the yardstick of the
    kernel's bound."""
    g = u + guidance * (cond - u)
    out = torch.stack([g[w] * (1.0 + phi * (cond[w].std() / g[w].std() - 1.0)) for w in range(g.shape[0])])
    return (out.double() - combine_rescaled(u, cond, guidance, phi)).abs().max().item()


def units(gathered, unit_index, c, f, hw):
    """The all-gathered buffer seen through unit_index: (u, cond) float32 [nW, c, f, hw]."""
    nW, halves, S = unit_index.shape
    g = gathered.reshape(-1, (f // S) * hw, c)
    h = g.index_select(0, unit_index.reshape(-1).long()).view(nW, halves, f, hw, c).permute(1, 0, 4, 2, 3)
    return h[0], h[-1]


def guidance_rescale(gathered, unit_index, c, f, hw, guidance, phi, workspace, preds):
    """Emulated ops.guidance_rescale: (count, mean, M2) per (window, frame, chunk of CHUNK pixels), each from two passes,
    merged per window in ascending (frame, chunk) order with the pairwise formula; float64 arithmetic, float32 stores."""
    nW = unit_index.shape[0]
    assert unit_index.shape[1] == 2 and 0.0 <= phi <= 1.0
    assert workspace.numel() >= nW * f * ((hw + CHUNK - 1) // CHUNK) * 6
    u, cond = units(gathered, unit_index, c, f, hw)
    g = (u.double() + guidance * (cond.double() - u.double())).float()
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
