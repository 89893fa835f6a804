"""The committed mutation audit of the oracle's unpinned half (tests/oracle_mutants/): audit.json has to cover every mutant of
mutants.json, each killed by a ground-truth / hand-worked test unless the list itself says why it is expected to survive; and a
sample of them is re-run here (compile the changed oracle, run the test that is recorded as its killer) so that the record
cannot go stale silently.  The full audit: python tests/oracle_mutants/run_audit.py."""
import os
import sys

import mutation_audit

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "oracle_mutants"))
import run_audit  # noqa: E402

SAMPLE = ("eps_not_overlapping_1", "walk_budget_div_11", "single_longer_than_94")


def test_the_audit_covers_the_mutants_and_they_die():
    mutants, audit = mutation_audit.load(run_audit.HERE)
    res = {r["id"]: r for r in audit["results"]}
    assert set(res) == {m["id"] for m in mutants} and len(mutants) >= 30
    assert audit["kill_suite"] == run_audit.KILL_SUITE  # the audit ran what the tool runs today
    survivors = 0
    for m in mutants:
        # the text a mutant changes must still be in the oracle, once
        text = open(os.path.join(ROOT, "oracle", m["file"])).read()
        assert text.count(m["find"]) == 1, "mutant %s no longer applies" % m["id"]
        if m.get("expect") == "survives":
            assert res[m["id"]]["status"] == "SURVIVED" and m.get("why"), m["id"]
            survivors += 1
        else:
            assert res[m["id"]]["status"] == "killed", "mutant %s is not noticed by the ground-truth suite" % m["id"]
            assert res[m["id"]]["by"][0].split("::")[0] in audit["kill_suite"] or res[m["id"]]["by"][0].split("::")[0] in [k.split("::")[0] for k in audit["kill_suite"]]
    assert audit["total"] == len(mutants) and audit["killed"] == len(mutants) - survivors


def test_a_sample_of_the_mutants_is_killed_again():
    """compile the changed oracle and run only the test recorded as its killer (a few seconds per mutant); the unmodified oracle
    passes those very tests"""
    mutation_audit.check_sample(run_audit.HERE, SAMPLE, run_audit.run_one, run_audit.suite_passes)
