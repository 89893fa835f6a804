"""The committed mutation audit of the call kernel's text (tests/calls_mutants/): audit.json has to cover every mutant of
mutants.json, each noticed by a case set of tests/calls_cases.py unless the list itself says why it computes the same function on
every input within the contract; and a sample is re-run here (build tests/emu_calls against the changed header -- a plain host
build of a stand-alone program -- and run the set recorded as its killer) so that the record cannot go stale silently.  The full
audit: python tests/calls_mutants/run_audit.py."""
import decimal
import importlib.util
import json
import os

import calls_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _run_audit():
    """tests/calls_mutants/run_audit.py under a name of its own (other audits have a run_audit too)"""
    spec = importlib.util.spec_from_file_location("calls_run_audit", os.path.join(HERE, "calls_mutants", "run_audit.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


SAMPLE = ("last_zero_is_gt", "next_lowest_from_254", "cell_stride_3")
# the one-line changes the audit has to hold at the least
REQUIRED = {"cap_le_255", "all_equal_test_dropped", "last_zero_is_gt", "one_zero_gives_gq_0", "next_lowest_from_254", "next_lowest_le", "ambiguous_sat16",
            "alt_words_sat8", "ref_inner_clamp_dropped", "ref_outer_clamp_dropped", "alt_without_ambiguous", "ref_keeps_ambiguous_alt",
            "alt_sum_from_allele_0", "cell_stride_3", "scores_at_allele_off", "cov_at_tri_off", "cov_stride_total_tri", "counters_2_1_3", "x_lt_y",
            "sample_and_hap_swapped", "constant_3_0103"}


def _load():
    mutants = json.load(open(os.path.join(HERE, "calls_mutants", "mutants.json")))
    audit = json.load(open(os.path.join(HERE, "calls_mutants", "audit.json")))
    return mutants, audit


def test_the_audit_covers_the_mutants_and_they_die():
    import calls_cases as cc
    mutants, audit = _load()
    res = {r["id"]: r for r in audit["results"]}
    assert set(res) == {m["id"] for m in mutants} >= REQUIRED and len(res) == len(mutants) >= 40
    assert sorted(audit["cases"]) == sorted(cc.SANITIZED)  # the audit ran what the tests run
    text = open(os.path.join(os.path.dirname(HERE), "graphtyper_amd", "csrc", "score_core.hpp")).read()
    survivors = 0
    for m in mutants:
        assert text.count(m["find"]) == 1, "mutant %s no longer applies" % m["id"]
        assert m["replace"] != m["find"]
        if m.get("expect") == "survives":
            assert res[m["id"]]["status"] == "SURVIVED" and m.get("why"), m["id"]
            survivors += 1
        else:
            assert res[m["id"]]["status"] in ("killed", "does not compile"), "mutant %s is not noticed by any set" % m["id"]
            assert res[m["id"]]["status"] != "killed" or res[m["id"]]["by"] in audit["cases"]
        assert "build" not in m or m.get("why_build"), m["id"]  # a mutant built with a sanitizer says why it needs one
    assert audit["total"] == len(mutants) and audit["killed"] == len(mutants) - survivors and survivors == 5


def test_the_survivors_compute_the_same_function():
    """the reasons mutants.json gives, as far as they are arithmetic: over every delta two uint16 scores can have"""
    c = float("3.01029995663981195213738894724493026768189881462108541")

    def llround(x):
        return int(decimal.Decimal(x).quantize(decimal.Decimal(1), rounding=decimal.ROUND_HALF_UP))

    for delta in range(0x10000):
        score, short = llround(float(delta) * c), llround(float(delta) * 3.0103)
        want = ref.pl_of(delta)
        assert (score if score < 255 else 255) == want == (score if score <= 255 else 255)  # cap_le_255
        assert (score if score < 254 else 255) == want                                       # cap_lt_254
        assert (short if short < 255 else 255) == want                                       # constant_3_0103
    assert llround(0.0 * c) == 0                                                             # all_equal_test_dropped


def test_a_sample_of_the_mutants_is_killed_again():
    run_audit = _run_audit()
    mutants, audit = _load()
    res = {r["id"]: r for r in audit["results"]}
    killers = [res[mid]["by"] for mid in SAMPLE]
    assert len(set(killers)) == len(SAMPLE)  # (three different sets)
    for mid, killer in zip(SAMPLE, killers):
        r = run_audit.run_one(next(x for x in mutants if x["id"] == mid), [killer])  # (only the recorded killer: a few seconds per mutant)
        assert r["status"] == "killed" and r["by"] == killer, (mid, r)
    # ... and the unmodified header, built the same way, passes those very sets
    assert run_audit.unmodified_passes(killers) is None
