"""float64 restatements of ancestral sampling (TEST INFRASTRUCTURE) for tests/test_ancestral_cpu.py and
tests/test_gpu_ancestral_sampling.py: the counter-based noise of v-express_amd/csrc/vx_rng.h (Philox4x32-10 of
Random123 + Box-Muller, keyed by (seed, step, frame, channel, pixel)), the textbook updates of diffusers==0.29.2
`DDIMScheduler.step` with eta and `EulerAncestralDiscreteScheduler.step` (v-prediction), and an emulated
`ops.overlap_ancestral_step` in the style of tests/fake_ops.py.  The loop that uses them is tests/loop_restated.py."""
import math

import numpy as np
import torch

import dpm_restated as D

KWARGS = D.KWARGS
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Random123) on arrays: ctr = 4 uint32 arrays (broadcastable), key = 2 ints -> 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = M0 * c[0], M1 * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return [v.astype(np.uint32) for v in c]


def box_muller(a, b):
    """Two uint32 arrays -> two standard normals (float64): u1 = ((a >> 8) + 1) 2^-24, u2 = (b >> 8) 2^-24."""
    u1 = ((a.astype(np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (b.astype(np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rho = np.sqrt(-2.0 * np.log(u1))
    return rho * np.cos(2.0 * np.pi * u2), rho * np.sin(2.0 * np.pi * u2)


def normals(seed, step, frames, c, hw):
    """The noise of schedule step `step` for absolute frames `frames`: float64 [c, len(frames), hw].  Counter (q, ch,
    frame, step), key (seed & 0xffffffff, seed >> 32); pixel quad q -> pixels 4q .. 4q+3."""
    assert hw % 4 == 0
    seed = int(seed)
    q = np.arange(hw // 4, dtype=np.uint64)[None, None, :]
    ch = np.arange(c, dtype=np.uint64)[:, None, None]
    fr = np.asarray(list(frames), dtype=np.uint64)[None, :, None]
    r = philox4x32_10((q, ch, fr, np.uint64(step)), (seed & 0xFFFFFFFF, seed >> 32))
    shape = (c, len(fr.ravel()), hw // 4)
    r = [np.broadcast_to(v, shape) for v in r]
    za, zb = box_muller(r[0], r[1])
    zc, zd = box_muller(r[2], r[3])
    return np.stack([za, zb, zc, zd], axis=-1).reshape(c, -1, hw)


def noise_like(seed, step, frame, c, h, w):
    """normals() of one frame as a float64 tensor [c, h, w]."""
    return torch.from_numpy(normals(seed, step, [frame], c, h * w)[:, 0].reshape(c, h, w).copy())


# ------------------------------------------------------------------------------------------------ textbook updates
def ddim_eta_update(a, ap, eta, x, v, z):
    """diffusers DDIMScheduler.step, v-prediction, with eta: sqrt(a') x0 + sqrt(1 - a' - s^2) eps + s z."""
    x0 = math.sqrt(a) * x - math.sqrt(1.0 - a) * v
    eps = math.sqrt(a) * v + math.sqrt(1.0 - a) * x
    var = (1.0 - ap) / (1.0 - a) * (1.0 - a / ap)
    # (s^2 = eta^2 var, not the square of its root: at eta = 1, abar_t = 0, 1 - a' - s^2 is then 0 exactly)
    return math.sqrt(ap) * x0 + math.sqrt(max(1.0 - ap - eta * eta * var, 0.0)) * eps + eta * math.sqrt(var) * z


def euler_a_update_ve(sig, sig1, x_ve, v, z):
    """diffusers EulerAncestralDiscreteScheduler.step, v-prediction, VE frame."""
    x0 = v * (-sig / math.sqrt(sig * sig + 1.0)) + x_ve / (sig * sig + 1.0)
    up = math.sqrt(sig1 * sig1 * (sig * sig - sig1 * sig1) / (sig * sig))
    down = math.sqrt(sig1 * sig1 - up * up)
    return x_ve + (x_ve - x0) / sig * (down - sig) + z * up


def ddim_table(n, abar=None):
    """[(abar_t, abar_prev)] of DDIM's trailing schedule (prev_t = t - 1000 // n; abar_prev = 1 below 0)."""
    abar = D.alphas_cumprod(clamp=False) if abar is None else abar
    out = []
    for t in D.timesteps(n):
        p = t - 1000 // n
        out.append((float(abar[t]), float(abar[p]) if p >= 0 else 1.0))
    return out


def overlap_ancestral_step(latents, preds, terms, frame_ids, counts, coef, seed, step_index):
    """Emulated ops.overlap_ancestral_step (fake_ops style: the kernel's sum order, float64 update and noise, float32
    stores)."""
    a, s, cx, c0, cz = (float(v) for v in coef)
    _, c, _, h, w = latents.shape
    fr = frame_ids.long()
    v = None
    for j in range(terms.shape[1]):
        slot, li = terms[:, j, 0].long(), terms[:, j, 1].long()
        term = preds[slot.clamp_min(0), :, li.clamp_min(0)] / counts[:, None, None]
        term = torch.where((slot >= 0)[:, None, None], term, torch.zeros_like(term))
        v = term if v is None else v + term
    x = latents[0].index_select(1, fr).transpose(0, 1).reshape(-1, c, h * w).double()
    new = cx * x - c0 * (a * x - s * v.double())
    if cz != 0.0:
        z = normals(seed, step_index, fr.tolist(), c, h * w)                 # [c, frames, hw]
        new = new + cz * torch.from_numpy(np.ascontiguousarray(z.transpose(1, 0, 2))).to(new.device)
    latents[0].index_copy_(1, fr, new.float().reshape(-1, c, h, w).transpose(0, 1))
