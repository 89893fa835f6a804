"""The committed mutation audit of the saturation replay's text (tests/replay_mutants/): audit.json has to cover every mutant of
mutants.json -- one-line changes of mark_cells_at_guard and replay_cells (score_replay.hpp) and of the replay branch of apply_recent and
the calls that reach it (score_core.hpp) --, each noticed by an item order of tests/replay_cases.py unless the list itself says why it
computes the same function on every input; and a sample is re-run here (tests/emu_replay built against the changed header -- a plain
host build of a stand-alone program -- over the set recorded as its killer) so that the record cannot go stale silently.  The full
audit: python tests/replay_mutants/run_audit.py."""
import mutation_audit
import replay_cases as rc
from replay_mutants.run_audit import AUDIT

SAMPLE = ("saturation_guard_down", "mask_hi_shift_31", "second_read_order_0")
# the one-line changes the audit has to hold at the least
REQUIRED = {"sort_cell_key_dropped", "sort_item_descending", "sort_order_descending", "sort_order_shift_9", "eps_mask_takes_order", "guard_le", "guard_fffe",
            "one_allele_gets_eps", "both_is_either", "either_is_both", "triangle_x_descending", "saturation_guard_up", "saturation_guard_down",
            "mark_le_guard", "mark_ignores_replayed", "unsupported_from_64", "bitmap_word_shift_6", "bitmap_bit_mask_15", "cell_stride_short",
            "test_word_shift_6", "test_bit_mask_15", "order_shift_9", "mask_lo_shifted", "mask_hi_shift_31", "item_plus_one", "second_read_order_0",
            "first_read_order_1"}


def test_the_audit_covers_the_mutants_and_they_die():
    mutation_audit.check_record(AUDIT, cases=rc.AUDITED, floor=30, survivors_ok=lambda n: n == 1, required=REQUIRED)


def test_the_survivor_computes_the_same_function():
    """sort_cell_descending: replay_cells walks one cell's entries at a time and needs them side by side, nothing more; the cells'
    order shows nowhere.  The restatement over a log whose cells come in descending order gives every cell the same head and row."""
    (case,), ((s, r),) = rc.cases("halves"), rc.expected("halves")
    by_cell = {}
    for e in sorted(r.log, key=lambda e: (-e[1], e[0], e[2])):
        by_cell.setdefault(e[1], []).append(e)
    assert list(by_cell) == sorted(by_cell, reverse=True) and len(by_cell) == len(r.marked) > 1
    for cell, entries in by_cell.items():
        level = 0
        for _, _, _, eps, _ in entries:
            level += eps if level < 0xFFFF - eps else 0
        assert level == r.head[cell]


def test_a_sample_of_the_mutants_is_killed_again():
    mutation_audit.check_sample(AUDIT.here, SAMPLE, AUDIT.run_one, AUDIT.unmodified_passes)
