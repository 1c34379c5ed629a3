"""tests/attention_cases.py on the CPU: the exact-answer attention cases are right, and they catch what the aggregate bounds miss.

For every shape tests/test_gpu_attention_exact.py runs, and both element types:
  (a) the float64 reference rounded to the element type meets each case's exact expectation, and so do three emulated
      legitimate designs (attention_cases.EMULATIONS: P rounded to the element type before PV with the row sum from the
      unrounded P; the same under a shift 6 bits above the row maximum; the row sum from the rounded P).  The deviation
      each emulation leaves is printed; an emulation outside a case's bound refuses the case list.
  (b) every mutant of the reference (attention_cases.MUTANTS) violates at least one case at that shape - unless the mutant
      IS the reference there (`is_noop`: the only key counted twice, b % kv_batches with one query batch per key batch, a
      head dim that is a multiple of 16 or prescaled keys for the padded scale), which is decided on a Gaussian float64
      problem and printed as "no-op".  Which case catches which mutant is printed per head dim, element type and shape.
  (c) for the record: on Gaussian data the mutant "extra zero-logit key" PASSES the aggregate bound of the older attention
      tests (max|err| <= 2^-6 max|ref|, relative L2 <= 1e-2; bfloat16) at every key count from 65 upwards.
"""
import pytest
import torch

import attention_cases as A

ENTRIES = ([("attention", d) for d in A.ATTN_HEAD_DIMS + (512,)] + [("temporal", d) for d in A.TEMPORAL_HEAD_DIMS]
           + [("small_kv", d) for d in A.SMALL_KV_HEAD_DIMS])
PRESCALED = {("attention", 40), ("attention", 80)}       # the routes that also run with scale = 0


def geoms(entry, d):
    return {"attention": A.attention_geoms, "temporal": A.temporal_geoms, "small_kv": A.small_kv_geoms}[entry](d)


def shape_str(g):
    return f"{g.batch}/{g.q_per_kv}x{g.heads}h {g.n_q}x{g.n_kv}"


def case_list(entry, d, g, el):
    return A.cases(g, el) + (A.cases(g, el, True) if (entry, d) in PRESCALED else ())


@pytest.mark.parametrize("el", A.ELEMS, ids=lambda e: A.EL_NAME[e])
@pytest.mark.parametrize("entry,d", ENTRIES)
def test_reference_and_emulations_meet_every_case(entry, d, el, capsys):
    worst = {}
    for g in geoms(entry, d):
        for case in case_list(entry, d, g, el):
            msg = case.first_wrong(case.run(A.reference))
            assert msg is None, "the float64 reference misses its own case: " + msg
            for name, kw in A.EMULATIONS.items():
                out = case.run(A.emulate, el=el, **kw)
                worst[case.name, name] = max(worst.get((case.name, name), 0.0), case.deviation(out))
                msg = case.first_wrong(out)
                assert msg is None, f"emulation '{name}' leaves the bound, the case list is refused: " + msg
    with capsys.disabled():
        head = f"\n{entry} d={d} [{A.EL_NAME[el]}] largest |out - expected| of the emulated designs over {len(geoms(entry, d))} shapes:"
        if not any(worst.values()):
            print(head + " 0 in every case under every emulation")
        else:
            print(head)
            for (cname, name), dev in worst.items():
                print(f"    {cname:18s} {name:52s} {dev:.3g}")


def caught(case, mutant):
    """Whether the mutant's output violates the case, judged on the first 12 queries of every batch alone (they hold key 0,
    key n_kv - 1 and both sides of every 64-key boundary of `routing`): that can only under-report the catchers."""
    c = case.first_queries(12)
    return bool(c.wrong(c.run(mutant)).any())


@pytest.mark.parametrize("el", A.ELEMS, ids=lambda e: A.EL_NAME[e])
@pytest.mark.parametrize("entry,d", ENTRIES)
def test_every_mutant_is_caught(entry, d, el, capsys):
    lines, missed = {}, []
    for g in geoms(entry, d):
        cl = case_list(entry, d, g, el)
        found = []
        for mname, mutant in A.MUTANTS.items():
            if A.is_noop(mname, g):
                found.append(f"{mname}: no-op")
                continue
            catchers = [c.name for c in cl if not (c.prescaled and A.is_noop(mname, g, base2=True)) and caught(c, mutant)]
            found.append(f"{mname}: {', '.join(catchers) if catchers else 'NOT CAUGHT'}")
            if not catchers:
                missed.append(f"{shape_str(g)}: {mname}")
        lines.setdefault("\n".join("      " + f for f in found), []).append(g)
    with capsys.disabled():
        print(f"\n{entry} d={d} [{A.EL_NAME[el]}] which case catches which mutant:")
        for body, gs in lines.items():
            heads = sorted({f"batch {g.batch} / q_per_kv {g.q_per_kv}, {g.heads} heads" for g in gs})
            print(f"    {'; '.join(heads)}, n_kv in {sorted({g.n_kv for g in gs})}, n_q in {sorted({g.n_q for g in gs})}\n" + body)
    assert not missed, f"{entry} d={d} [{A.EL_NAME[el]}]: no case catches " + "; ".join(missed)


@pytest.mark.parametrize("d", A.ATTN_HEAD_DIMS + (512,))
def test_extra_zero_key_passes_the_old_aggregate_bound(d, capsys):
    """The reason for this file: one padded key in the denominator of a ragged last tile is inside the Gaussian tests' bound."""
    rows = []
    for g in A.attention_geoms(d):
        if g.n_q != max(A.ATTN_N_Q):            # one documented Gaussian problem per key count
            continue
        (rm, rl), (mm, ml) = A.old_bound_figures(g)
        rows.append(f"    {shape_str(g):22s} reference {rm:.2f} / {rl:.2f}   + one zero-logit key {mm:.2f} / {ml:.2f}")
        assert rm <= 1 and rl <= 1, f"d={d} {shape_str(g)}: the rounded reference itself misses the old bound ({rm:.2f} / {rl:.2f})"
        if g.n_kv >= 65:
            assert mm <= 1 and ml <= 1, (f"d={d} {shape_str(g)}: the mutant no longer passes the old bound ({mm:.2f} / {ml:.2f}) - "
                                         "good news, but then this record is out of date")
    with capsys.disabled():
        print(f"\nattention d={d} [bf16] Gaussian data under the aggregate bound, max|err| / allowed and relL2 / allowed:")
        print("\n".join(rows))


@pytest.mark.parametrize("el", A.ELEMS, ids=lambda e: A.EL_NAME[e])
def test_failure_message_names_element_and_key(el):
    """What a failing GPU test prints: the first wrong element's batch, head, query and column, and for `routing` the key
    whose V row came out instead."""
    g = A.Geom(4, 8, 65, 129, 40, 2)
    case = A.cases(g, el)[3]
    assert case.name == "routing"
    msg = case.first_wrong(case.run(A.MUTANTS["key batch b % kv_batches"]))
    # (batch 0 is served by kv batch 0 under both mappings; batch 1 is the first that reads the other key batch)
    assert msg is not None and "first at batch 1 head 0 query 0 column" in msg and "wanted key" in msg, msg
    msg = case.first_wrong(case.run(A.MUTANTS["last key dropped"]))
    assert msg is not None and "the output row equals" in msg and f"wanted key {g.n_kv - 1} of kv batch" in msg, msg
    wrong_rows = case.wrong(case.run(A.MUTANTS["last key dropped"])).any(dim=1).reshape(g.batch, g.n_q)
    pi_last = (case.pi == g.n_kv - 1).any(dim=2)
    assert torch.equal(wrong_rows, pi_last), "exactly the queries that route to the dropped key are wrong"
    counted = A.cases(g, el)[0]
    msg = counted.first_wrong(counted.run(A.MUTANTS["extra zero-logit zero-value key"]))
    assert msg is not None and "first at batch 0 head 0 query 0 column 0" in msg and "(bound: bits)" in msg, msg
