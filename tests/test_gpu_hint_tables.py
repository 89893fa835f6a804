"""The tables of the position-hinted pass as the DEVICE builds them (gtx_index_dev.hip: k_hint_graph, k_window_cells, the filter and
flag kernels over index_build.hpp) against the restatement over the oracle's index (tests/hint_tables_ref.py), on the hand-made graphs
of tests/hint_tables_cases.py: all seven tables, every word, exactly.  The sets and their facts: test_hint_tables_cases.py."""
import pytest

import hint_tables_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tc.NAMES)
def test_device_hint_tables_equal_the_restatement(name):
    c = tc.built(name).context(0)
    assert tc.compare(name, [c.hint_table(which) for which in range(7)]) is None
