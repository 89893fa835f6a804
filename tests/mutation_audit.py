"""What the mutation audits share (tests/*_mutants/run_audit.py, tests/oracle_mutants/run_auto.py): the one-line change that has to
apply exactly once, the thread pool, the table, the committed record and the options; for the audits of a kernel's text the whole
run (KernelAudit); and the two checks the audits' tests make of a committed record (check_record, check_sample).

An audit of a kernel's text: every entry of its mutants.json is a piece of the header's text that occurs once, and what replaces it.
For each, the header is copied into a temporary directory and changed, the kernel's host emulation (tests/emu_*) is built against
that directory as a plain stand-alone program (CSRC=<tmp> SAN= OPT=-O2; a mutant whose only fault may be an access out of bounds
names the sanitizer it is built with instead, "build"), and the cases are run through it in `order` until the case module's
judge(name, run) says how one differs, or the program dies.  A mutant no case notices SURVIVES: either mutants.json says why it
must ("expect": "survives"), or the cases have a gap.  Results go to audit.json beside mutants.json (committed)."""
import argparse
import functools
import json
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor

import emu_programs

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
DEAD = ("killed", "does not compile")


def changed(text, mutant, where="the header"):
    """`text` with the mutant's one change; a mutant that does not apply exactly once stops the tool"""
    n = text.count(mutant["find"])
    if n != 1:
        raise SystemExit("mutant %s: its text occurs %d times in %s (must be 1)" % (mutant["id"], n, where))
    return text.replace(mutant["find"], mutant["replace"], 1)


def options(jobs):
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=jobs)
    ap.add_argument("--only", nargs="*")
    return ap


def each(run_one, mutants, jobs):
    """run_one over the mutants, `jobs` at a time, in the list's order"""
    with ThreadPoolExecutor(jobs) as pool:
        yield from pool.map(run_one, mutants)


def write_record(path, record):
    with open(path, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


def audit(here, run_one, jobs, only, **head):
    """the mutants of <here>/mutants.json (or those named in `only`) through run_one, the table, and -- of a whole run -- the record
    <here>/audit.json: `head` (what was run), the counts, the results"""
    mutants = json.load(open(os.path.join(here, "mutants.json")))
    if only:
        mutants = [m for m in mutants if m["id"] in only]
    results = list(each(run_one, mutants, jobs))
    for r in results:
        by = r.get("by", r.get("detail", ""))
        print("%-36s %-16s %s" % (r["id"], r["status"], (by if isinstance(by, str) else " ".join(by)) + (" -- " + r["how"] if "how" in r else "")))
    killed = sum(r["status"] in DEAD for r in results)
    print("%d of %d mutants killed" % (killed, len(results)))
    if not only:
        write_record(os.path.join(here, "audit.json"), dict(head, killed=killed, total=len(results), results=results))


class KernelAudit:
    """the audit of one kernel's text.  here: the directory of mutants.json and audit.json; header: the file under
    graphtyper_amd/csrc that is changed; emu: its emulation's directory under tests/; cases: the case module -- judge(name, run)
    -> None or how the case differs, with run(write, read) of emu_programs.run --; order: the cases, the cheap ones first, so that
    a mutant's recorded killer is quick to run again; covers: the names the tests run, every one of which `order` has to hold;
    also: further headers of the emulation that a mutant may name as its "header" (all of them are copied beside the changed one)"""

    def __init__(self, here, header, emu, cases, order, covers, also=()):
        assert sorted(order) == sorted(covers), sorted(set(order) ^ set(covers))
        self.here, self.emu, self.cases, self.order = here, emu, cases, list(order)
        self.header = os.path.join(ROOT, "graphtyper_amd", "csrc", header)
        self.also = [os.path.join(ROOT, "graphtyper_amd", "csrc", h) for h in also]

    def header_of(self, mutant):
        """the file a mutant changes: the audit's header, or the one of `also` it names"""
        path = os.path.join(os.path.dirname(self.header), mutant.get("header", os.path.basename(self.header)))
        assert path in [self.header] + self.also, path
        return path

    def build(self, csrc, out, san=""):
        """the emulation against the header in `csrc`, into the directory `out` -> (program, None), or (None, the compiler's last words)"""
        try:
            return emu_programs.build(self.emu, out, CSRC=csrc, SAN=san, OPT="-O2"), None
        except emu_programs.BuildFailed as e:
            return None, str(e)[-300:]

    def first_difference(self, exe, tmp, names):
        """the first case of `names` the program at `exe` gets wrong, and how -> (name, how) or None"""
        run = functools.partial(emu_programs.run, exe, tmp)
        for name in names:
            try:
                how = self.cases.judge(name, run)
            except emu_programs.Died as e:
                how = e.how
            if how is not None:
                return name, how
        return None

    def run_one(self, mutant, names=None):
        with tempfile.TemporaryDirectory(prefix="gtx_%s_mutant_" % self.emu) as tmp:
            for path in [self.header] + self.also:
                with open(os.path.join(tmp, os.path.basename(path)), "w") as f:
                    f.write(changed(open(path).read(), mutant) if path == self.header_of(mutant) else open(path).read())
            exe, error = self.build(tmp, tmp, mutant.get("build", ""))
            if error is not None:
                return dict(id=mutant["id"], status="does not compile", detail=error)
            found = self.first_difference(exe, tmp, names or self.order)
            if found is None:
                return dict(id=mutant["id"], status="SURVIVED")
            return dict(id=mutant["id"], status="killed", by=found[0], how=found[1])

    def unmodified_passes(self, names):
        """the header as it is, built the same way, over `names` -> None, or what went wrong"""
        with tempfile.TemporaryDirectory(prefix="gtx_%s_plain_" % self.emu) as tmp:
            exe, error = self.build(os.path.dirname(self.header), tmp)
            return error if error is not None else self.first_difference(exe, tmp, names)

    def main(self):
        a = options(8).parse_args()
        wrong = self.unmodified_passes(self.order)  # (and the restatement's results once, before the threads ask for them)
        if wrong is not None:
            raise SystemExit("the unmodified header fails: %s" % (wrong,))
        audit(self.here, self.run_one, a.j, a.only, cases=self.order)


# ---- what the audits' tests ask of a committed record ----------------------------------------------------------------------------
def load(here):
    return json.load(open(os.path.join(here, "mutants.json"))), json.load(open(os.path.join(here, "audit.json")))


def killer(result):
    """a record's "by": the case's name, or a list whose first entry is the test's id"""
    return result["by"] if isinstance(result["by"], str) else result["by"][0]


def check_record(audit, cases, floor, survivors_ok, required=frozenset()):
    """the committed record of a KernelAudit covers the mutants and they die.  cases: what the tests run, which the record has to
    have run; floor: the least number of mutants; survivors_ok(n): how many may survive for a stated reason; required: ids the list
    has to hold at the least"""
    mutants, record = load(audit.here)
    res = {r["id"]: r for r in record["results"]}
    assert set(res) == {m["id"] for m in mutants} >= set(required) and len(res) == len(mutants) >= floor
    assert sorted(record["cases"]) == sorted(cases)  # the audit ran what the tests run
    survivors = 0
    for m in mutants:
        text = open(audit.header_of(m)).read()
        assert text.count(m["find"]) == 1, "mutant %s no longer applies" % m["id"]
        assert m["replace"] != m["find"]
        if m.get("expect") == "survives":
            assert res[m["id"]]["status"] == "SURVIVED" and m.get("why"), m["id"]
            survivors += 1
        else:
            assert res[m["id"]]["status"] in DEAD, "mutant %s is not noticed by any case" % m["id"]
            assert res[m["id"]]["status"] != "killed" or res[m["id"]]["by"] in record["cases"]
        assert "build" not in m or m.get("why_build"), m["id"]  # a mutant built with a sanitizer says why it needs one
    assert record["total"] == len(mutants) and record["killed"] == len(mutants) - survivors and survivors_ok(survivors)


def check_sample(here, sample, run_one, unmodified_passes):
    """a sample is killed again, each by the killer the record names (only that one: a few seconds per mutant), and the unmodified
    text, built the same way, passes those very cases"""
    mutants, audit = load(here)
    res = {r["id"]: r for r in audit["results"]}
    killers = [killer(res[mid]) for mid in sample]
    assert len(set(killers)) == len(sample) == 3  # (three different ones)
    for mid, by in zip(sample, killers):
        r = run_one(next(x for x in mutants if x["id"] == mid), [by])
        assert r["status"] == "killed" and killer(r) == by, (mid, r)
    assert unmodified_passes(killers) is None
