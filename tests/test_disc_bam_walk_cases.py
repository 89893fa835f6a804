"""What the streams of tests/disc_bam_walk_cases.py hold -- each set stands for one thing that can go wrong in the record walk, and a
set that lost it would let the tests built on it pass for nothing -- and that the module's definition reads records as the module
that writes them (tests/disc_bam_cases.py) lays them out.  No library code runs here."""
import numpy as np
import pytest

import disc_bam_cases as bc
import disc_bam_walk_cases as wc


@pytest.mark.parametrize("name", sorted(wc.SETS))
def test_the_set_holds_what_it_is_for(name):
    assert set(wc.SETS) == set(wc.FACTS)
    wc.FACTS[name](wc.streams(name))


@pytest.mark.parametrize("name", sorted(wc.SETS))
def test_the_cut_lists_are_lists(name):
    for s in wc.streams(name):
        names = [n for n, _ in s.cut_lists]
        assert names[:3] == ["none", "every record start", "every 777 bytes"] and ("every byte" in names) == (len(s.data) <= wc.SHORT)
        for label, cuts in s.cut_lists:
            assert all(0 < a < len(s.data) for a in cuts) and all(a < b for a, b in zip(cuts, cuts[1:])), (s.label, label)


def test_the_definition_reads_what_the_writer_wrote():
    """the tables of a sound stream are the ones tests/disc_bam_cases.py states for the same records"""
    for f in bc.files("shift") + bc.files("cigars") + bc.files("counts"):
        stream, offsets, reads, n_cigar = f.tables
        got = wc.define(stream.tobytes())
        assert (got["status"], got["n_reads"], got["n_cigar"]) == (wc.OK, len(reads), n_cigar)
        assert np.array_equal(got["offsets"], offsets) and got["reads"].tobytes() == reads.tobytes()
        assert got["max_l_seq"] == max(len(r["codes"]) for r in f.records)


def test_the_judge_sees_a_wrong_walk():
    """a run that is the definition passes; one that adopts a decoy, misses a status or miscounts the segments does not"""
    def ideal(change=None):
        def run(data, lists):
            out = []
            for cuts in lists:
                want = wc.define(data)
                hit, rewalked, _ = wc.segments(data, cuts)
                got = dict(want, segments_hit=hit, segments_rewalked=rewalked)
                for what in ("offsets", "reads"):
                    table = np.ascontiguousarray(want[what]).view(np.uint8).reshape(-1)
                    g = wc.guarded(len(table))
                    g[wc.GUARD:wc.GUARD + len(table)] = table
                    got[what] = g
                if change:
                    change(got, cuts)
                out.append(got)
            return out
        return run

    def more(got, cuts):
        got["n_reads"] += 1

    def status(got, cuts):
        got["status"] = wc.OK

    def entry(got, cuts):
        if got["n_reads"]:
            got["reads"][wc.GUARD + 12] ^= 1  # a cigar_off

    def guard(got, cuts):
        got["offsets"][-1] = 0

    def hits(got, cuts):
        got["segments_hit"], got["segments_rewalked"] = got["segments_hit"] + got["segments_rewalked"], 0

    for name in wc.SETS:
        assert wc.judge(name, ideal()) is None
    assert "n_reads" in wc.judge("decoy", ideal(more)) and "status" in wc.judge("damage", ideal(status)) and "reads" in wc.judge("counts", ideal(entry))
    assert "guard" in wc.judge("align", ideal(guard)) and "segments" in wc.judge("straddle", ideal(hits))
