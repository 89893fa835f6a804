"""tests/realign_ref.py -- the restatement every realignment test compares with -- held to a second, structurally different
statement of include/gtx.h's definition: tests/realign_brute.py writes every alignment down and picks the best by one global
order.  Over every small pair of four families all five fields are equal (integers: no tolerance).  Small pairs are where the
tie-breaks and the maxima at equal score decide; a misreading of the definition that the restatement and the kernel share
(both carry score and origin packed into one integer) shows here."""
import itertools

import pytest

import realign_brute as rb
import realign_ref as rr

A, C, M, G, T, N, EQ = 1, 2, 3, 4, 8, 15, 0


def strings(alphabet, longest):
    return [s for k in range(1, longest + 1) for s in itertools.product(alphabet, repeat=k)]


FAMILIES = {  # name: (the read's codes, longest read, the window's codes, longest window, pairs)
    "ac": ((A, C), 4, (A, C), 5, 30 * 62),
    "acn": ((A, C, N), 3, (A, C, N), 4, 39 * 120),
    "acgt": ((A, C, G, T), 3, (A, C, G, T), 3, 84 * 84),
    "codes_m_eq": ((A, M, EQ), 3, (A, M, EQ, N), 3, 39 * 84),  # a read's code that is neither a base nor N: a match with itself and N only
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_restatement_equals_the_enumeration(family):
    q_codes, m_max, t_codes, n_max, count = FAMILIES[family]
    pairs = [(q, t) for q in strings(q_codes, m_max) for t in strings(t_codes, n_max)]
    assert len(pairs) == count
    wrong = [(q, t, rr.align(q, t), rb.align(q, t)) for q, t in pairs if rr.align(q, t) != rb.align(q, t)]
    assert wrong == [], wrong[:5]


def test_the_enumeration_by_hand():
    """alignments small enough to score on paper"""
    assert rb.shapes(1, 1) == [(((1, 1),), 0)]
    assert len(rb.shapes(2, 2)) == 5  # (1,1) (1,2) (2,1) (2,2) alone, and (1,1)(2,2)
    assert rb.align((A,), (A,)) == (1, 0, 1, 0, 1)
    assert rb.align((A,), (C,)) == (-4, 0, 1, 0, 1)
    assert rb.align((A,), (C, A, A)) == (1, 0, 1, 1, 2)               # the smaller target_end of two equal places
    assert rb.align((A, C), (A, A)) == (-3, 0, 2, 0, 2)               # 1 - 4 pairing both; clipping the C: 1 - 5 = -4
    assert rb.align((N, N), (C, G)) == (2, 0, 2, 0, 2)
    assert rb.align((M,), (M, N)) == (1, 0, 1, 0, 1) and rb.align((M,), (A, N)) == (1, 0, 1, 1, 2)
    # (the enumeration grows fast: these are as long as it stays quick)
    # seven matches around one target base without a partner: 7 - 7 = 0; clipping ACG off instead: 4 - 5
    q = (A, C, G, T, C, A, G)
    assert rb.align(q, q[:3] + (A,) + q[3:]) == (0, 0, 7, 0, 8)
    # around two: 7 - 8 = -1, which clipping ACG off reaches too, with the same two ends: the smaller target_begin wins
    assert rb.align(q, q[:3] + (A, A) + q[3:]) == (-1, 0, 7, 0, 9)
    # one query base without a partner: 6 - 7 = -1 with all of the query used; either clip gives 3 - 5
    assert rb.align((A, C, G, G, T, C, A), (A, C, G, T, C, A)) == (-1, 0, 7, 0, 6)
