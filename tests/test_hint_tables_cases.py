"""The tables of the position-hinted pass (gtx_ctx_hint_table 0..6: position flags, reference planes, tail entries, the two half-key
filters, the allele windows and their list per site) of a context WITHOUT a device, held word for word to a plain restatement over the
oracle's index (tests/hint_tables_ref.py) on hand-made graphs (tests/hint_tables_cases.py): lone SNPs at every k-mer offset, repeats,
halves at every distance the far codes tell apart, 16-mers shared by 16 / 17 / 64 / 65 keys, neighbour labels adding up to 16 and 17,
merged and neighbouring sites, other letters, reference nodes of 254 / 255 / 256 bases, windows at the region's ends, an SV graph, and
every table length around the plane groups' ends.  A fact test per set shows, from the restatement alone, that the set holds the shape
it is for.  Every comparison is of integers and exact; a difference is reported as table, position and field.  The same sets through
the stand-alone program: test_hint_tables_emu.py; on the device: test_gpu_hint_tables.py."""
import numpy as np
import pytest

import hint_tables_cases as tc
import hint_tables_ref as H
import scenarios
from graphtyper_amd import lib as gtx
from oracle_lib import Oracle


@pytest.mark.parametrize("name", tc.NAMES)
def test_the_set_holds_the_shape_it_is_for(name):
    tc.FACTS[name](tc.built(name))


@pytest.mark.parametrize("name", tc.NAMES)
def test_host_tables_equal_the_restatement(name):
    c = tc.built(name).context(-1)
    assert tc.compare(name, [c.hint_table(which) for which in range(7)]) is None


@pytest.mark.parametrize("kind", ["snp100", "cfg3"])
def test_graphs_nobody_arranged(kind):
    """the restatement on the synthetic graphs of test_hint_near_free.py, 30 000 bases"""
    ref, recs, _, _ = scenarios.synthetic_case(kind, n_ref=30000, n_reads=10, region_begin=1000000)
    aav = kind == "cfg3"
    g = gtx.graph_from_records(ref, recs, region_begin=1000000, add_all_variants=aav)
    o = Oracle(ref, recs, region_begin=1000000, add_all_variants=aav)
    want = H.HintTablesRef(o.index_dump(), o.graph(), g).tables()
    c = gtx.Context(g, device=-1)
    assert H.compare([c.hint_table(which) for which in range(7)], want) is None
    assert (len(want[5]) > 0) == aav


def test_a_difference_is_named_by_table_position_and_field():
    """what the restatement says of a filter that lacks one key's half, and of a tail entry that calls a site of five alleles a SNP"""
    b = tc.built("plain")
    k = b.key_at(20)
    f0, f1, fl = H.filters(b.r.keys, drop=(k, 1))
    assert np.array_equal(f0, b.want[3]) and (f1 != b.want[4]).sum() == 1
    how = H.compare(b.r.tables(filt=(f0, f1, fl)), b.want)
    assert how.startswith("table 4 (filter side 1) word") and "table 0" not in how  # (nobody's neighbour: the flags stay)
    got = [t.copy() for t in b.want]
    got[2][2 * 499] |= H.TAIL_OK
    assert H.compare(got, b.want) == "table 2 (tail_info) position 499 word x: TAIL_OK: 1, expected 0 (1 words differ)"
    got = [t.copy() for t in b.want]
    got[0][2 * 100 + 1] ^= 1 << H.FAR_LEFT_SHIFT
    assert H.compare(got, b.want) == "table 0 (pos_flags) position 100 word y: far_left: 2, expected 3 (1 words differ)"
