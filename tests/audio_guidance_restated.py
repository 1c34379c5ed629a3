"""float64 restatements of three-row guidance (TEST INFRASTRUCTURE) for tests/test_audio_guidance_cpu.py and
tests/test_gpu_audio_guidance.py: the guided prediction g = u + s (m - u) + s_a (c - m) of a separate audio scale (u: no
condition; m, "silent": reference bank + keypoints, zero audio; c: everything), its rescale towards std(c) (diffusers'
`rescale_noise_cfg` with the fully conditional row as the target), the mean-overlap loop of
pipelines/v_express_pipeline.py:526-583 over the oracle UNet with any row set for every sampler, and emulated
`ops.combine_units3` / `ops.guidance_rescale3` in the style of tests/fake_ops.py and guidance_restated.py."""
import math

import torch

import ancestral_restated as A
import dpm_restated as D
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


def oracle_rows_unet(sd3, sd2, ocfg, ref_latents, w_ref, w_aud):
    """The oracle UNet with a bank per batch row: fn(x [b, 4, f, h, w], t, audio [b * f, n_ctx, 768], kps [b, C0, f, h,
    w], bank_rows) with bank_rows[i] = 1 for the reference bank and 0 for the all-zero one (what
    ReferenceAttentionControl's cat([zeros, v]) gives rows 0 / 1; the oracle takes banks as plain [b, hw, C] tensors)."""
    from oracle import unet as OU
    ref = OU.refnet_banks(sd2, ocfg, ref_latents)

    def fn(x, t, audio, kps, bank_rows):
        banks = {k: torch.cat([v if r else torch.zeros_like(v) for r in bank_rows]) for k, v in ref.items()}
        return OU.unet3d_forward(sd3, ocfg, x, t, audio, kps, banks, w_ref, w_aud)
    return fn


def restated_loop(unet_fn, latents, windows, s, s_a, kps_feature, audio_embeddings, n, sampler="ddim", phi=0.0,
                  start=0.0, end=1.0, seed=None, eta=0.0, rows=None):
    """guidance_restated.restated_loop with the rows of `rows_for(s, s_a)` per window (`unet_fn` of oracle_rows_unet;
    kps_feature / audio_embeddings in the CFG layout, row 0 zeros): a guided step combines them in float64 as
    u + s (m - u) + s_a (c - m) (three rows), m + s_a (c - m) (rows m, c) or u + s (c - u) (rows u, c) and rescales the
    result towards std(c) for phi > 0; an unguided step takes the c row as it is."""
    rows = rows_for(s, s_a) if rows is None else rows
    assert len(rows) > 1
    guided = G.guided_steps(n, start, end)
    lat = latents.double().clone()
    _, c, F_, h, w = lat.shape
    sg = D.sigmas(n)
    if sampler == "euler-a":
        lat = lat * sg[0]
    tab = A.ddim_table(n)
    ords = D.orders(n)
    hist = torch.zeros_like(lat)
    count = torch.zeros(F_, dtype=torch.long)
    for ctx in windows:
        count[ctx] += 1
    for i, t in enumerate(D.timesteps(n)):
        scale = 1.0 / math.sqrt(1.0 + sg[i] ** 2) if sampler == "euler-a" else 1.0
        counter = torch.zeros(F_, dtype=torch.long)
        pending, final = [None] * F_, {}
        names = rows if guided[i] else ("c",)
        for ctx in windows:
            trip = [ROWS[r] for r in names]
            aud = torch.cat([audio_embeddings[a][ctx] for _, _, a in trip])
            kps = torch.stack([kps_feature[k][:, ctx] for _, k, _ in trip])
            inp = (lat[:, :, ctx] * scale).float().repeat(len(trip), 1, 1, 1, 1)
            out = unet_fn(inp, t, aud, kps, [b for b, _, _ in trip]).double()
            p = {r: out[j:j + 1] for j, r in enumerate(names)}
            if not guided[i]:
                pred = p["c"]
            else:
                if names == ("u", "m", "c"):
                    pred = p["u"] + s * (p["m"] - p["u"]) + s_a * (p["c"] - p["m"])
                elif names == ("m", "c"):
                    pred = p["m"] + s_a * (p["c"] - p["m"])
                else:
                    pred = p["u"] + s * (p["c"] - p["u"])
                if phi > 0.0:
                    pred = G.rescale(pred, p["c"], phi)
            counter[ctx] += 1
            pred = pred / count[ctx][None, None, :, None, None].double()
            for li, fi in enumerate(ctx):
                pending[fi] = pred[:, :, li].clone() if pending[fi] is None else pending[fi] + pred[:, :, li]
                if counter[fi] == count[fi]:
                    final[fi] = pending[fi]
                    pending[fi] = None
        x = lat.clone()
        for fi, v in final.items():
            if sampler == "dpm":
                lat[:, :, fi], hist[:, :, fi] = D.update(sg, i, ords[i], x[:, :, fi], v, hist[:, :, fi])
            elif sampler == "euler-a":
                z = A.noise_like(seed, i, fi, c, h, w)[None]
                lat[:, :, fi] = A.euler_a_update_ve(sg[i], sg[i + 1], x[:, :, fi], v, z)
            else:
                z = A.noise_like(seed, i, fi, c, h, w)[None] if sampler == "ddim-eta" else 0.0
                a, ap = tab[i]
                lat[:, :, fi] = A.ddim_eta_update(a, ap, eta if sampler == "ddim-eta" else 0.0, x[:, :, fi], v, z)
    return lat
