"""The committed mutation audit of the discovery events kernel's text (tests/disc_events_mutants/): audit.json has to cover every
mutant of mutants.json, each noticed by a case set or a launch-level case of tests/disc_event_cases.py unless the list itself says
why it must survive; and a sample is re-run here (build tests/emu_disc_events against the changed header -- a plain host build of
a stand-alone program -- and run the case recorded as its killer) so that the record cannot go stale silently.  The full audit:
python tests/disc_events_mutants/run_audit.py."""
import importlib.util
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _run_audit():
    """tests/disc_events_mutants/run_audit.py under a name of its own (other audits have a run_audit too)"""
    spec = importlib.util.spec_from_file_location("disc_events_run_audit", os.path.join(HERE, "disc_events_mutants", "run_audit.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


SAMPLE = ("block_mask_gt_32", "deletion_limit_one_more", "overflow_to_the_event_counter")


def _load():
    mutants = json.load(open(os.path.join(HERE, "disc_events_mutants", "mutants.json")))
    audit = json.load(open(os.path.join(HERE, "disc_events_mutants", "audit.json")))
    return mutants, audit


def test_the_audit_covers_the_mutants_and_they_die():
    import disc_event_cases as dc
    mutants, audit = _load()
    res = {r["id"]: r for r in audit["results"]}
    assert set(res) == {m["id"] for m in mutants} and len(res) == len(mutants) >= 30
    assert sorted(audit["cases"]) == sorted(list(dc.SETS) + list(dc.LAUNCHES))  # the audit ran what the tests run
    text = open(os.path.join(os.path.dirname(HERE), "graphtyper_amd", "csrc", "gtx_disc_events_dev.hpp")).read()
    survivors = 0
    for m in mutants:
        assert text.count(m["find"]) == 1, "mutant %s no longer applies" % m["id"]
        assert m["replace"] != m["find"]
        if m.get("expect") == "survives":
            assert res[m["id"]]["status"] == "SURVIVED" and m.get("why"), m["id"]
            survivors += 1
        else:
            assert res[m["id"]]["status"] in ("killed", "does not compile"), "mutant %s is not noticed by any case" % m["id"]
            assert res[m["id"]]["status"] != "killed" or res[m["id"]]["by"] in audit["cases"]
        assert "build" not in m or m.get("why_build"), m["id"]  # a mutant built with a sanitizer says why it needs one
    assert audit["total"] == len(mutants) and audit["killed"] == len(mutants) - survivors and survivors <= 4


def test_a_sample_of_the_mutants_is_killed_again():
    run_audit = _run_audit()
    mutants, audit = _load()
    res = {r["id"]: r for r in audit["results"]}
    killers = [res[mid]["by"] for mid in SAMPLE]
    assert len(set(killers)) == len(SAMPLE)  # (three different cases)
    for mid, killer in zip(SAMPLE, killers):
        r = run_audit.run_one(next(x for x in mutants if x["id"] == mid), [killer])  # (only the recorded killer: a few seconds per mutant)
        assert r["status"] == "killed" and r["by"] == killer, (mid, r)
    # ... and the unmodified header, built the same way, passes those very cases
    assert run_audit.unmodified_passes(killers) is None
