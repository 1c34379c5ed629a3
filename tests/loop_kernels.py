"""The float32 kernels of the denoising loop on one fixed set of seeded inputs, as sha256 digests (TEST INFRASTRUCTURE):
`combine_units` (one and two rows), `combine_units3`, `guidance_rescale` / `guidance_rescale3` (phi 0 and 0.7) and the
three `overlap_*_step` updates.  tests/test_gpu_loop_kernels_parity.py compares the digests of the current build with
tests/golden/loop_kernels_parent.json, written by `python tests/make_golden.py loop_kernels` on an MI355X with the library
of the commit before vx_elem.hip's combine kernels and mean-of-terms loops were folded into one each.

Shapes, the smallest at which these kernels can still go wrong: nW = 2 windows of f = 4 frames, c = 4, frame granules
S in {1, 2}; hw = 1028 for combine / rescale (two statistics chunks, the second of 4 pixels; no multiple of the 256-thread
block); hw = 20 with max_terms = 3 for the updates, one frame with a skipped (-1) term in the middle."""
import hashlib
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

NW, C, F_WIN, HW_COMBINE, HW_UPDATE, FRAMES = 2, 4, 4, 1028, 20, 6
S_GUIDE, S_AUDIO = 3.5, 6.0
ELEMENTS = {"bfloat16": torch.bfloat16, "float16": torch.float16}


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.int32).numpy().tobytes()).hexdigest()


def _special(t, positions):
    """+0.0, -0.0 and inf at fixed places of a float32 tensor (flat indices)."""
    flat = t.view(-1)
    for pos, v in zip(positions, (0.0, -0.0, float("inf"))):
        flat[pos] = v
    return t


def combine_inputs(S):
    """(gathered [nW * 3 * S, (f / S) * hw, c], unit_index [nW, 3, S]): a permuted index; window 0 holds +0.0 and -0.0 and
    a frame whose rows m and c are bit-equal, window 1 an inf (so that window 0's statistics stay finite)."""
    g = torch.Generator().manual_seed(20 + S)
    f_loc = F_WIN // S
    gathered = torch.randn(NW * 3 * S, f_loc * HW_COMBINE, C, generator=g)
    uidx = torch.randperm(NW * 3 * S, generator=g).to(torch.int32).view(NW, 3, S).contiguous()
    u0, m0, c0 = (int(uidx[0, r, 0]) for r in range(3))
    gathered[m0, :HW_COMBINE] = gathered[c0, :HW_COMBINE]              # frame 0 of window 0: m == c
    gathered[u0].view(-1)[C * HW_COMBINE + 6] = -0.0
    gathered[c0].view(-1)[C * HW_COMBINE + 5] = 0.0                    # (the row every variant reads, one row included)
    gathered[c0].view(-1)[C * HW_COMBINE + 7] = -0.0
    gathered[int(uidx[1, 2, S - 1])].view(-1)[C * 300 + 1] = float("inf")
    return gathered, uidx


def update_inputs():
    """latents [1, c, 6, 4, 5], preds [nW, c, f, hw], the plan (terms, frame_ids, counts) and an x0 history."""
    g = torch.Generator().manual_seed(31)
    latents = _special(torch.randn(1, C, FRAMES, 4, 5, generator=g), (3, 47, 101))
    preds = _special(torch.randn(NW, C, F_WIN, HW_UPDATE, generator=g), (9, 230, 411))
    hist = torch.randn(1, C, FRAMES, 4, 5, generator=g)
    # (window slot, frame of the window) of every term, -1 = skip: frame 2 skips its middle term, frame 5 sums three
    plan = {3: [(0, 3), (1, 1), (-1, -1)], 0: [(0, 0), (-1, -1), (-1, -1)], 5: [(1, 3), (0, 1), (1, 2)],
            2: [(0, 2), (-1, -1), (1, 0)], 1: [(0, 1), (-1, -1), (-1, -1)], 4: [(-1, -1), (1, 2), (-1, -1)]}
    frame_ids = torch.tensor(list(plan), dtype=torch.int32)
    terms = torch.tensor([plan[fr] for fr in plan], dtype=torch.int32)
    counts = torch.tensor([float(sum(s >= 0 for s, _ in plan[fr])) for fr in plan], dtype=torch.float32)
    return latents, preds, terms, frame_ids, counts, hist


def run(dev="cuda"):
    """dict(inputs = name -> digest, outputs = name -> digest) of every call on the library in force."""
    from v_express_amd import ops
    inputs, outputs = {}, {}
    for S in (1, 2):
        gathered, uidx = combine_inputs(S)
        inputs[f"gathered_S{S}"], inputs[f"unit_index_S{S}"] = digest(gathered), digest(uidx)
        gd = gathered.to(dev)
        idx = {rows: uidx[:, 3 - rows:].contiguous().to(dev) for rows in (1, 2, 3)}
        ws = torch.empty(ops.guidance_rescale_ws_floats(NW, F_WIN, HW_COMBINE), device=dev, dtype=torch.float32)

        def preds():
            return torch.full((NW, C, F_WIN, HW_COMBINE), float("nan"), device=dev, dtype=torch.float32)
        for rows in (1, 2):
            out = preds()
            ops.combine_units(gd, idx[rows], C, F_WIN, HW_COMBINE, S_GUIDE, out)
            outputs[f"combine_units_halves{rows}_S{S}"] = digest(out)
        out = preds()
        ops.combine_units3(gd, idx[3], C, F_WIN, HW_COMBINE, S_GUIDE, S_AUDIO, out)
        outputs[f"combine_units3_S{S}"] = digest(out)
        for phi in (0.0, 0.7):
            out = preds()
            ops.guidance_rescale(gd, idx[2], C, F_WIN, HW_COMBINE, S_GUIDE, phi, ws, out)
            outputs[f"guidance_rescale_phi{phi}_S{S}"] = digest(out)
            out = preds()
            ops.guidance_rescale3(gd, idx[3], C, F_WIN, HW_COMBINE, S_GUIDE, S_AUDIO, phi, ws, out)
            outputs[f"guidance_rescale3_phi{phi}_S{S}"] = digest(out)
    latents, preds_u, terms, frame_ids, counts, hist = update_inputs()
    for name, t in (("latents", latents), ("preds", preds_u), ("terms", terms), ("frame_ids", frame_ids),
                    ("counts", counts), ("x0_history", hist)):
        inputs[f"update_{name}"] = digest(t)
    pd, td, fd, cd = preds_u.to(dev), terms.to(dev), frame_ids.to(dev), counts.to(dev)
    lat = latents.to(dev)
    ops.overlap_ddim_step(lat, pd, td, fd, cd, (0.8, 0.6, 0.9, 0.43588989435))
    outputs["overlap_ddim_step"] = digest(lat)
    for c_1 in (0.0, 0.37):                                   # the x0 history unread, then read
        lat, h = latents.to(dev), hist.to(dev)
        ops.overlap_multistep_step(lat, pd, td, fd, cd, h, (0.8, 0.6, 1.1, 0.45, c_1))
        outputs[f"overlap_multistep_step_c1_{c_1}"] = digest(lat)
        outputs[f"overlap_multistep_step_c1_{c_1}_x0_history"] = digest(h)
    for c_z in (0.0, 0.25):                                   # without and with the generator
        lat = latents.to(dev)
        ops.overlap_ancestral_step(lat, pd, td, fd, cd, (0.8, 0.6, 1.1, 0.45, c_z), (7 << 40) | 12345, 3)
        outputs[f"overlap_ancestral_step_cz_{c_z}"] = digest(lat)
    torch.cuda.synchronize()
    return dict(inputs=inputs, outputs=outputs)


def run_all(dev="cuda"):
    """element type name -> run() on that type's library (the kernels are float32 in both), with the library's build id."""
    from v_express_amd import lib as L
    out = {}
    for name, elem in ELEMENTS.items():
        with L.element_type(elem):
            out[name] = dict(run(dev), build=L.current().vx_build_id().decode())
    return out


def write(path):
    with open(path, "w") as fh:
        json.dump(run_all(), fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    write(sys.argv[1])
