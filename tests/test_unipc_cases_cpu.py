"""The exact-answer cases of `vx_overlap_unipc_step` (tests/unipc_cases.py) on the host: the float64 reference is exact in
float32, the torch float32 emulation of the op (tests/unipc_worker.py) reproduces it bit for bit inside guard bands, and
every mutant of the reference fails at least one case.  tests/test_gpu_unipc.py feeds the same cases to the kernel."""
import numpy as np
import pytest
import torch

import guard
import unipc_cases as UC
import unipc_worker as UW

CASES = UC.cases()


def test_the_case_list_covers_what_the_kernel_can_get_wrong():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) == 9
    two = [c for c in CASES if c["name"] != "order3_320_threads"]
    assert {c["h"] * c["w"] for c in two} == {4, 12}
    for c in two:
        assert (c["C"], c["F"], c["frame_ids"].tolist(), c["terms"].shape, c["preds"].shape[:3]) == \
            (4, 5, [1, 3, 4], (3, 2, 2), (2, 4, 3))
        assert c["terms"][0, 1, 0] == -1 and c["terms"][2, 0, 0] == -1 and (c["terms"][1, :, 0] >= 0).all()
        assert c["counts"].tolist() == [1.0, 2.0, 1.0]
    big = CASES[-1]
    assert len(big["frame_ids"]) * big["C"] * big["h"] * big["w"] // 4 == 320 and big["h"] * big["w"] == 64
    assert len(big["frame_ids"]) < big["F"]                            # frames outside frame_ids exist here too
    # a third-order update writes the slot it reads as h3; the first one of a run reads nothing
    assert any(c["coef"][4] == 1 and c["coef"][2] == c["coef"][3] >= 0 for c in CASES)
    assert any(c["coef"][:3] == (-1, -1, -1) and c["coef"][4] == 0 for c in CASES)
    for c in CASES:
        assert len(c["coef"]) == len(UC.FIELDS) == 16
        for v in c["coef"][5:]:                                         # dyadic: k / 4 with a small k
            assert float(v) * 4 == int(float(v) * 4) and v not in (0.0, 1.0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_is_exact_in_float32(case):
    """Every value of the float64 reference is a float32 value, and so is every intermediate: recomputing the update in
    float32 with another association (the emulation of the op) gives the same bits."""
    ref = UC.reference(case)
    for r in ref:
        fin = np.isfinite(r)
        assert (r[fin].astype(np.float32).astype(np.float64) == r[fin]).all()
        assert (np.abs(r[fin]) * 512 == np.round(np.abs(r[fin]) * 512)).all() and np.abs(r[fin]).max() < 64
    lat, hist, saved = ref
    ids = case["frame_ids"].tolist()
    others = [f for f in range(case["F"]) if f not in ids]
    assert others and UC.same_bits(lat[:, :, others], case["latents"][:, :, others])
    assert UC.same_bits(hist[:, :, others], case["history"][:, :, others])
    assert UC.same_bits(saved[:, :, others], case["saved"][:, :, others])
    assert np.isfinite(lat[:, :, ids]).all() and np.isfinite(saved[:, :, ids]).all()
    for slot in range(3):
        if slot != case["coef"][3]:
            assert UC.same_bits(hist[slot], case["history"][slot])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_float32_emulation_reproduces_the_cases_inside_guard_bands(case):
    C, F_, h, w = case["C"], case["F"], case["h"], case["w"]
    bufs = {k: guard.Guarded(case[k].shape, torch.float32, "cpu").load(torch.from_numpy(case[k]))
            for k in ("latents", "preds", "history", "saved")}
    UW.overlap_unipc_step(bufs["latents"].view, bufs["preds"].view, torch.from_numpy(case["terms"]),
                          torch.from_numpy(case["frame_ids"]), torch.from_numpy(case["counts"]), bufs["history"].view,
                          bufs["saved"].view, case["coef"])
    for k, want in zip(("latents", "history", "saved"), UC.reference(case)):
        bufs[k].assert_intact(f"{case['name']}: {k}")
        assert UC.same_bits(bufs[k].view.numpy(), want), (case["name"], k)
    bufs["preds"].assert_intact(f"{case['name']}: preds")
    assert UC.same_bits(bufs["preds"].view.numpy(), case["preds"])


@pytest.mark.parametrize("mutant", UC.MUTANTS)
def test_every_mutant_fails_at_least_one_case(mutant):
    caught = []
    for case in CASES:
        good, bad = UC.reference(case), UC.reference(case, mutant)
        if not all(UC.same_bits(g, b) for g, b in zip(good, bad)):
            caught.append(case["name"])
    print(f"[unipc cases] mutant {mutant}: caught by {caught}")
    assert caught


def test_mutant_list_is_the_one_the_cases_were_written_for():
    assert set(UC.MUTANTS) == {"m_from_xc", "saved_is_x", "saved_is_out", "corrector_skipped", "predictor_from_x",
                               "write_before_read", "h1_h2_swapped", "minus_one_slot_read", "count_ignored",
                               "frame_ids_ignored"}
