"""The audit runner's own refusals (tests/mutation_audit.py), on a header of three lines: nothing is built."""
import types

import pytest

import mutation_audit

HEADER = "int twice = 1;\nint twice = 1;\nint once = 2;\n"


def test_the_runner_refuses_what_it_cannot_audit(tmp_path):
    (tmp_path / "three_lines.hpp").write_text(HEADER)

    def audit(order):
        return mutation_audit.KernelAudit(str(tmp_path), str(tmp_path / "three_lines.hpp"), "no_emulation", types.SimpleNamespace(), order, covers=("first", "second"))

    assert audit(("second", "first")).header == str(tmp_path / "three_lines.hpp")
    for find, times in (("never", 0), ("int twice = 1;", 2)):
        with pytest.raises(SystemExit) as refusal:
            audit(("first", "second")).run_one(dict(id="m", find=find, replace="int thrice = 3;"))
        assert str(refusal.value) == "mutant m: its text occurs %d times in the header (must be 1)" % times
    assert mutation_audit.changed(HEADER, dict(id="m", find="once = 2", replace="once = 3")) == HEADER.replace("once = 2", "once = 3")
    # an ORDER that omits a case of its module: the descriptor is not made, so the runner's module does not import
    with pytest.raises(AssertionError):
        audit(("first",))
