"""The alignment of include/gtx.h (gtx_disc_realign_*) stated a second time, by enumeration: every alignment the model allows is
written down as the cells it pairs and the gaps between them, each is scored by adding up its parts, and the best is picked by
one global order.  No recurrence, no table of cell values, no value that carries an origin along -- nothing in common with
tests/realign_ref.py, which test_realign_brute.py holds to this file over every small pair.

An alignment of a query q[1..m] to a target t[1..n]:
  * begins with a pair of bases (i0, j0): clip_begin = i0 - 1 query bases are clipped, target_begin = j0 - 1;
  * goes on with pairs (i + 1, j + 1) and gaps -- L >= 1 query bases without a partner, or L >= 1 target bases without one; a
    gap costs 7 + (L - 1); a gap of one kind may be followed at once by a gap of the other kind, which pays the opening again
    (two gaps of one kind in a row are one longer gap that was paid for twice: never the best, so they are not written down);
  * ends with a pair (i1, j1): clip_end = i1, target_end = j1;
  * pays 5 when clip_begin > 0 and 5 when clip_end < m;
  * a pair scores +1 when the two codes are equal or either is 15 (N), else -4.
Among the alignments of the highest total: the smallest target_end, then the smallest clip_end, then the smallest target_begin,
then the smallest clip_begin.  (The definition breaks ties cell by cell -- the origin with the smaller db, then cb, at every max
-- which amounts to this order, because adding a score never changes an origin.)"""
import functools

MATCH, MISMATCH, GAP_OPEN, GAP_EXTEND, CLIP, N = 1, -4, 7, 1, 5, 15


def pair_score(a, b):
    return MATCH if (a == b or a == N or b == N) else MISMATCH


def _extend(m, n, i, j, cells, gaps, last, out):
    """(i, j): the cell reached last; cells: the pairs so far; gaps: what the gaps so far cost; last: 'P' after a pair, 'Q' after a
    gap in the query, 'T' after a gap in the target.  Every alignment that ends with a pair goes to `out`."""
    if last == "P":
        out.append((tuple(cells), gaps))
    if i < m and j < n:
        cells.append((i + 1, j + 1))
        _extend(m, n, i + 1, j + 1, cells, gaps, "P", out)
        cells.pop()
    # a gap must be followed by something that ends in a pair: room for it has to be left on both sides
    if last != "Q":
        for length in range(1, m - i):
            if j < n:
                _extend(m, n, i + length, j, cells, gaps + GAP_OPEN + (length - 1) * GAP_EXTEND, "Q", out)
    if last != "T":
        for length in range(1, n - j):
            if i < m:
                _extend(m, n, i, j + length, cells, gaps + GAP_OPEN + (length - 1) * GAP_EXTEND, "T", out)


@functools.lru_cache(maxsize=None)
def shapes(m, n):
    """every alignment of an m-base query to an n-base target, whatever the letters: (paired cells, cost of its gaps)"""
    out = []
    for i0 in range(1, m + 1):
        for j0 in range(1, n + 1):
            _extend(m, n, i0, j0, [(i0, j0)], 0, "P", out)
    return out


def align(q, t):
    """q, t: tuples of 4-bit codes -> (score, clip_begin, clip_end, target_begin, target_end)"""
    m, n = len(q), len(t)
    best = None
    for cells, gaps in shapes(m, n):
        (i0, j0), (i1, j1) = cells[0], cells[-1]
        total = sum(pair_score(q[i - 1], t[j - 1]) for i, j in cells) - gaps
        if i0 > 1:
            total -= CLIP
        if i1 < m:
            total -= CLIP
        order = (-total, j1, i1, j0 - 1, i0 - 1)
        if best is None or order < best:
            best = order
    return -best[0], best[4], best[2], best[3], best[1]
