"""One rank of tests/test_unipc_cpu.py's two-rank gloo run (TEST INFRASTRUCTURE): the small-config denoising loop with
UniPCMultistepScheduler under emulated kernels (loop_worker.emulate_kernels + `overlap_unipc_step` below, a torch float32
emulation of ops.overlap_unipc_step: the kernel's expression, every product and sum one float32 operation in the kernel's
order)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loop_worker as W  # noqa: E402  (first: it puts the repository on sys.path)
import dpm_restated as D  # noqa: E402

# F = 14 in windows of 8 with overlap 2 (two windows, four CFG units), 5 steps at solver_order 3 (orders 1, 2, 3, 2, 1; the
# corrector at orders 1, 2, 3 and skipped before the last step), 8x8 latents
F, CF, CO, STEPS, LATENT = 14, 8, 2, 5, 8


def scheduler(**kw):
    from v_express_amd import UniPCMultistepScheduler
    return UniPCMultistepScheduler(**{**D.KWARGS, **kw})


def overlap_unipc_step(latents, preds, terms, frame_ids, counts, history, saved, coef):
    """Emulated ops.overlap_unipc_step in float32 (vx_overlap_unipc_step without contraction)."""
    h1, h2, h3, h_write, use_c = (int(v) for v in coef[:5])
    a_i, s_i, q_s, q_m, q_1, q_2, q_3, k_x, k_m, k_1, k_2 = (torch.tensor(float(v), dtype=torch.float32) for v in coef[5:])
    _, c, _, h, w = latents.shape
    fr = frame_ids.long()

    def frames(buf):
        return buf.index_select(1, fr).transpose(0, 1).reshape(-1, c, h * w)

    def store(buf, val):
        buf.index_copy_(1, fr, val.reshape(-1, c, h, w).transpose(0, 1))
    v = None
    for j in range(terms.shape[1]):
        slot, li = terms[:, j, 0].long(), terms[:, j, 1].long()
        term = preds[slot.clamp_min(0), :, li.clamp_min(0)] / counts[:, None, None]
        valid = (slot >= 0)[:, None, None]
        if v is None:
            v, first = torch.where(valid, term, torch.zeros_like(term)), ~valid
        else:                                                     # the first valid term initialises the sum
            v = torch.where(valid, torch.where(first, term, v + term), v)
            first = first & ~valid
    x = frames(latents[0])
    H1 = frames(history[h1]) if h1 >= 0 else None
    H2 = frames(history[h2]) if h2 >= 0 else None
    m = a_i * x - s_i * v
    xc = x
    if use_c:
        xc = q_s * frames(saved[0]) + q_m * m
        if h1 >= 0:
            xc = xc + q_1 * H1
        if h2 >= 0:
            xc = xc + q_2 * H2
        if h3 >= 0:
            xc = xc + q_3 * frames(history[h3])
    out = k_x * xc + k_m * m
    if h1 >= 0:
        out = out + k_1 * H1
    if h2 >= 0:
        out = out + k_2 * H2
    store(saved[0], xc)
    if h_write >= 0:
        store(history[h_write], m)
    store(latents[0], out)


def emulate(patch=W._Setattr):
    """loop_worker.emulate_kernels plus the stand-in for ops.overlap_unipc_step."""
    ops = W.emulate_kernels(patch)
    patch.setattr(ops, "overlap_unipc_step", overlap_unipc_step)
    return ops


def run(**kw):
    pipe = W.build_pipeline("cpu")
    pipe.scheduler = scheduler(solver_order=3, **kw)
    return W.run_loop(pipe, F, CF, CO, STEPS, latent=LATENT, device="cpu")


def main(rank):
    """One rank of loop_worker.spawn_gloo: this rank's final latents."""
    torch.set_num_threads(2)
    emulate()
    return run()
