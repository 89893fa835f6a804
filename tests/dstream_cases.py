"""The record stream's decisions on the device (include/gtx.h: gtx_dstream_push; kernel text graphtyper_amd/csrc/gtx_dstream_dev.hpp)
held to their definition, stated here in plain Python over the records and their nibble rows: define().  The definition knows no
wavefronts, no sorts and no scans, and nothing of the library but its record layouts and the plane layout restated in numpy
(lib.planes_reference); tests/test_dstream_cases.py holds it to the host's gtx_stream_push, push by push.

  checks     over all records of the push, in record order, each record's in this order: rg >= n_read_groups ARG, l_qseq >
             max_read_len UNSUPPORTED, (l_qseq + 1) / 2 > seq_stride or l_qseq > 2 plane_stride ARG (in front of them: n > align_cap,
             item_cap or max_batch CAPACITY).
  kept       (flag & sam_flag_filter) == 0.
  duplicate  a kept record that equals the previous kept record in tid, pos, l_qseq and the first (l_qseq + 1) / 2 bytes of its row;
             any other kept record is a head: a task with the next align_index, its plane row and gtx_read_meta.
  rec meta   {align_index of its head, flag | the forward-only bit OF ITS HEAD, mapq, score_diff, pos, isize}.
  pairing    per key (rg, name_id), the occurrences in stream order, a parked mate first: nothing waits and flag & 1 -> it waits;
             nothing waits and unpaired -> an item of one; something waits -> the same flag & 64 is ARG, else an item of the two with
             this record's sample.  Items in the order of the records that emit them; what waits at the end is parked, in stream order;
             more than parked_cap of them: CAPACITY.
  A failing push leaves the state as it was.

Hand-made record sets, each for one thing that can go wrong (FACTS states what a set holds), every one run whole, one record a push,
cut at CUTS and at its own positions, and by the scripts it is made for (a push with a capacity one short, then again with room), and
judge(name, run): None, or how the results of the program behind `run` differ -- shared by the emulation (tests/test_dstream_emu.py)
and the device (tests/test_gpu_dstream.py).  All values are bytes and words; there is no tolerance."""
import collections
import functools
import struct

import numpy as np

from graphtyper_amd import lib as gtx

OK, ERR_ARG, ERR_UNSUPPORTED, ERR_CAPACITY = 0, 1, 4, 5
WHY_RG, WHY_LONG, WHY_ROW, WHY_CLASH, WHY_PARKED = 1, 2, 3, 4, 5  # gtx_dstream_dev.hpp: DSTREAM_FAIL_*
FORWARD_ONLY, INVALID = 0x8000, 0xFFFFFFFF
PAIRED, REVERSED, MATE_REVERSED, FIRST, SECOND = 1, 16, 32, 64, 128
GUARD = 64   # bytes behind each output
FILL = 0xA5  # what the outputs and their guards hold before a push
CUTS = (1, 63, 64, 65)
SINGLES_UP_TO = 700  # a case of more records is pushed one record a push over its first records only (the model: its first 700)


def params(**kw):
    p = dict(sam_flag_filter=3840, force_align_both_orientations=0, max_read_len=0)
    p.update(kw)
    return p


def max_read_len_of(p):
    return p["max_read_len"] or 256


def new_state():
    """prev: None or ((tid, pos, l_qseq, bytes), align_index, forward-only bit) of the previous kept record; parked: [(rg, name_id, rec
    meta, sample)] in stream order"""
    return dict(prev=None, parked=[], next_align=0, n_records=0, n_duplicated=0)


def counts(state):
    return state["n_records"], state["n_duplicated"], len(state["parked"])


# ---- the definition -------------------------------------------------------------------------------------------------------------------
def forward_only(p, r):
    one = not (r["flag"] & PAIRED) or (r["tid"] == r["mtid"] and -1200 < r["isize"] < 1200 and bool(r["flag"] & REVERSED) != bool(r["flag"] & MATE_REVERSED))
    return FORWARD_ONLY if one and not p["force_align_both_orientations"] else 0


def plane_rows(rows, lengths, plane_stride):
    """the plane rows of nibble rows: the whole first (l + 1) / 2 bytes -- the pad nibble of an odd read too --, zeros behind them"""
    codes = np.zeros((len(rows), 2 * plane_stride), np.uint8)
    for k, (row, l) in enumerate(zip(rows, lengths)):
        nb = (l + 1) // 2
        codes[k, 0:2 * nb:2] = row[:nb] >> 4
        codes[k, 1:2 * nb:2] = row[:nb] & 15
    return gtx.planes_reference(codes, plane_stride) if len(rows) else np.zeros((0, plane_stride), np.uint8)


def define(p, n_read_groups, state, recs, rows, plane_stride, align_cap=None, item_cap=None, max_batch=None, parked_cap=None):
    """-> (planes [n_align, plane_stride], meta [READ_META], items [SCORE_ITEM], the next state, status, reason); a failing status comes
    with no outputs and the state it was given.  reason: (why, record, l_qseq, n_parked) -- what decided a failing push: the check (WHY_*),
    for a record's check the record of the push and its length, and the mates that wait: those the stream holds, or for WHY_PARKED those
    that would wait at the end of the push.  A push that succeeds, or that its capacities refuse before a record is looked at: (0, 0,
    0, the mates that wait behind it)"""
    n, seq_stride = len(recs), rows.shape[1]
    nothing = (np.zeros((0, plane_stride), np.uint8), np.zeros(0, gtx.READ_META), np.zeros(0, gtx.SCORE_ITEM))
    waiting_now = len(state["parked"])
    if any(cap is not None and n > cap for cap in (align_cap, item_cap, max_batch)):
        return nothing + (state, ERR_CAPACITY, (0, 0, 0, waiting_now))
    for i, r in enumerate(recs):
        l = int(r["l_qseq"])
        if r["rg"] >= n_read_groups:
            return nothing + (state, ERR_ARG, (WHY_RG, i, l, waiting_now))
        if l > max_read_len_of(p):
            return nothing + (state, ERR_UNSUPPORTED, (WHY_LONG, i, l, waiting_now))
        if (l + 1) // 2 > seq_stride or l > 2 * plane_stride:
            return nothing + (state, ERR_ARG, (WHY_ROW, i, l, waiting_now))
    kept = [i for i in range(n) if (int(recs[i]["flag"]) & p["sam_flag_filter"]) == 0]
    prev, next_align, heads, me, duplicated = state["prev"], state["next_align"], [], {}, 0
    for i in kept:
        r = recs[i]
        l = int(r["l_qseq"])
        mine = (int(r["tid"]), int(r["pos"]), l, rows[i, :(l + 1) // 2].tobytes())
        if prev is not None and prev[0] == mine:
            duplicated += 1
        else:
            prev = (mine, next_align, forward_only(p, r))
            next_align += 1
            heads.append(i)
        prev = (mine, prev[1], prev[2])
        me[i] = (prev[1], int(r["flag"]) | prev[2], int(r["mapq"]), int(r["score_diff"]), int(r["pos"]), int(r["isize"]))
    # the tasks
    meta = np.zeros(len(heads), gtx.READ_META)
    for k, i in enumerate(heads):
        r = recs[i]
        clip = int(r["cigar_front"]) >> 4 if r["n_cigar"] != 0 and (int(r["cigar_front"]) & 15) == 4 else 0
        meta[k] = (r["l_qseq"], int(r["flag"]) | forward_only(p, r), r["tid"], r["mtid"], r["isize"], int(r["pos"]) - clip)
    planes = plane_rows([rows[i] for i in heads], [int(recs[i]["l_qseq"]) for i in heads], plane_stride)
    # pairing: the occurrences of each key in stream order (-len(parked) .. -1: the parked mates, 0 .. n - 1: the records)
    seen = collections.defaultdict(list)
    P = len(state["parked"])
    for k, (rg, name, m, sample) in enumerate(state["parked"]):
        seen[(rg, name)].append((k - P, m, sample))
    for i in kept:
        seen[(int(recs[i]["rg"]), int(recs[i]["name_id"]))].append((i, me[i], int(recs[i]["sample"])))
    emitted, waits = {}, []
    for key, occurrences in seen.items():
        waiting = None
        for at, m, sample in occurrences:
            if waiting is None:
                if m[1] & PAIRED:
                    waiting = (at, m, sample)
                else:
                    emitted[at] = (m, (INVALID, 0, 0, 0, 0, 0), sample, 0)
            else:
                if (waiting[1][1] & FIRST) == (m[1] & FIRST):
                    return nothing + (state, ERR_ARG, (WHY_CLASH, 0, 0, waiting_now))
                emitted[at] = (waiting[1], m, sample, 0)
                waiting = None
        if waiting is not None:
            waits.append((waiting[0], key[0], key[1], waiting[1], waiting[2]))
    waits.sort(key=lambda w: w[0])
    if parked_cap is not None and len(waits) > parked_cap:
        return nothing + (state, ERR_CAPACITY, (WHY_PARKED, 0, 0, len(waits)))
    items = np.zeros(len(emitted), gtx.SCORE_ITEM)
    for k, at in enumerate(sorted(emitted)):
        items[k] = emitted[at]
    after = dict(prev=prev, parked=[w[1:] for w in waits], next_align=next_align, n_records=state["n_records"] + len(kept),
                 n_duplicated=state["n_duplicated"] + duplicated)
    return planes, meta, items, after, OK, (0, 0, 0, len(waits))


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
Push = collections.namedtuple("Push", "lo hi align_cap item_cap")


def push(lo, hi, align_cap=None, item_cap=None):
    """records [lo, hi) in one call; the capacities default to the number of records"""
    return Push(lo, hi, hi - lo if align_cap is None else align_cap, hi - lo if item_cap is None else item_cap)


class Builder:
    """records and their rows, one add() each.  The bytes of a row behind the read hold a pattern no rule may look at, another one for
    every add(): a comparison or a plane row that takes them in shows."""

    def __init__(self, seq_stride=80, plane_stride=80, n_read_groups=1, **p):
        self.seq_stride, self.plane_stride, self.n_read_groups, self.p = seq_stride, plane_stride, n_read_groups, params(**p)
        self.recs, self.rows = [], []

    def __len__(self):
        return len(self.recs)

    def add(self, codes, pad=0, flag=0, tid=0, mtid=0, pos=1000, isize=0, rg=0, sample=0, name=None, mapq=60, score_diff=7, n_cigar=0, cigar_front=0,
            cigar_back=0, l_qseq=None, times=1):
        """codes: the read's 4-bit codes; pad: the low nibble of an odd read's last byte; l_qseq: another length than len(codes) (the
        row keeps the codes' bytes).  -> the first index"""
        codes = np.asarray(codes, np.uint8)
        l = len(codes) if l_qseq is None else l_qseq
        nb = (len(codes) + 1) // 2
        row = np.full(self.seq_stride, (0xE7 + 37 * len(self.recs)) & 0xFF, np.uint8)
        row[:min(nb, self.seq_stride)] = gtx.pack_nibbles(codes[None, :], stride=max(nb, 1))[0, :min(nb, self.seq_stride)]
        if len(codes) % 2 and nb <= self.seq_stride:
            row[nb - 1] |= pad
        first = len(self.recs)
        for _ in range(times):
            r = np.zeros(1, gtx.STREAM_RECORD)[0]
            r["flag"], r["mapq"], r["score_diff"], r["tid"], r["mtid"], r["pos"], r["isize"], r["l_qseq"], r["rg"], r["sample"] = flag, mapq, score_diff, tid, mtid, pos, isize, l, rg, sample
            r["name_id"] = (1 << 40) + len(self.recs) if name is None else name
            r["n_cigar"], r["cigar_front"], r["cigar_back"] = n_cigar, cigar_front, cigar_back
            self.recs.append(r)
            self.rows.append(row.copy())
        return first

    def case(self, label, cuts=(), scripts=(), max_batch=None, parked_cap=None, splits_agree=True):
        return Case(label, self, cuts, scripts, max_batch, parked_cap, splits_agree)


class Case:
    def __init__(self, label, b, cuts, scripts, max_batch, parked_cap, splits_agree):
        self.label, self.p, self.n_read_groups, self.seq_stride, self.plane_stride = label, b.p, b.n_read_groups, b.seq_stride, b.plane_stride
        self.recs = np.array(b.recs, gtx.STREAM_RECORD) if b.recs else np.zeros(0, gtx.STREAM_RECORD)
        self.rows = np.array(b.rows, np.uint8).reshape(len(b.recs), b.seq_stride)
        n = len(self.recs)
        self.max_batch = max(n, 1) if max_batch is None else max_batch
        self.parked_cap = n if parked_cap is None else parked_cap
        self.splits_agree = splits_agree  # the pushes of every script that succeed leave the same bytes one after the other
        at = sorted({c for c in tuple(CUTS) + tuple(cuts) if 0 < c < n})
        bounds = [0] + at + [n]
        self.scripts = [("whole", [push(0, n)]), ("one record a push", [push(i, i + 1) for i in range(min(n, SINGLES_UP_TO))] + ([push(SINGLES_UP_TO, n)] if n > SINGLES_UP_TO else [])),
                        ("cut at %s" % at, [push(lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])])] + list(scripts)
        if max_batch is not None:  # (the scripts that go with a small max_batch are the case's own)
            self.scripts = list(scripts)

    @functools.lru_cache(maxsize=None)
    def want(self, script_name):
        """per push of the script: dict(planes, meta, items, status, counts [after the push], reason)"""
        return self.want_of(dict(self.scripts)[script_name])

    def want_of(self, pushes):
        state, out = new_state(), []
        for q in pushes:
            planes, meta, items, state, status, reason = define(self.p, self.n_read_groups, state, self.recs[q.lo:q.hi], self.rows[q.lo:q.hi], self.plane_stride,
                                                        align_cap=q.align_cap, item_cap=q.item_cap, max_batch=self.max_batch, parked_cap=self.parked_cap)
            out.append(dict(planes=planes, meta=meta, items=items, status=status, counts=counts(state), reason=reason))
        return out

    def rooms(self, script_name):
        """per push the entries its output arrays hold: exactly what the definition leaves; a failing push: what its capacities say"""
        return rooms_of(dict(self.scripts)[script_name], self.want(script_name))

    def total(self, script_name="whole"):
        """the outputs of the script's pushes that succeed, one after the other -> (planes, meta, items) as bytes"""
        ws = [w for w in self.want(script_name) if w["status"] == OK]
        return tuple(b"".join(w[k].tobytes() for w in ws) for k in ("planes", "meta", "items"))


def rooms_of(pushes, wants):
    return [(len(w["meta"]), len(w["items"])) if w["status"] == OK else (q.align_cap, q.item_cap) for q, w in zip(pushes, wants)]


def bases(l, seed):
    return np.array([1, 2, 4, 8], np.uint8)[np.random.default_rng(seed).integers(0, 4, l)]


FILTER_BITS = (256, 512, 1024, 2048)


def _filters():
    out = []
    for flt in (3840, 0):
        b = Builder(sam_flag_filter=flt)
        for k, bit in enumerate(FILTER_BITS):
            b.add(bases(30, k), pos=100 + k)
            b.add(bases(30, 10 + k), pos=100 + k, flag=bit)
            b.add(bases(30, 20 + k), pos=100 + k, flag=bit | 4 | 8)
        b.add(bases(30, 40), pos=200, flag=2 | 4 | 8)
        out.append(b.case("every bit of 3840 on a record, the filter %d" % flt))
    b = Builder()
    for k in range(5):
        b.add(bases(30, k), pos=100, flag=FILTER_BITS[k % 4])
    out.append(b.case("everything dropped"))
    b = Builder()
    for k in range(3):
        b.add(bases(30, k), pos=100 + k)
    out.append(b.case("pushes of no record", scripts=[("with empty pushes", [push(0, 0), push(0, 2), push(2, 2), push(2, 3), push(3, 3)])]))
    # a dropped record between two kept ones that are equal, and dropped records that are equal to kept ones
    b = Builder()
    b.add(bases(40, 1), pos=300)
    b.add(bases(40, 1), pos=300, flag=1024)
    b.add(bases(40, 1), pos=300)
    b.add(bases(40, 2), pos=300, flag=512)
    b.add(bases(40, 1), pos=300)
    out.append(b.case("dropped records among equal ones", cuts=(2, 3)))
    return out


RUNS = (1, 2, 3, 64, 65, 130)


def _dups_runs():
    b = Builder()
    mids = []
    for k, run in enumerate(RUNS):
        at = b.add(bases(50 + k, 100 + k), pos=1000 + 10 * k, times=run, sample=k % 3)
        mids.append(at + run // 2)
    whole = b.case("runs of %s equal records" % (RUNS,), cuts=mids)
    b = Builder()
    seq = bases(41, 7)
    other_first, other_last = seq.copy(), seq.copy()
    other_first[0] ^= 3
    other_last[-1] ^= 3
    other_second = seq.copy()
    other_second[1] ^= 5
    b.add(seq, pos=500)
    b.add(seq, pos=500, tid=1, mtid=1)         # another tid
    b.add(seq, pos=500, tid=1, mtid=1)         # (a duplicate of that)
    b.add(seq, pos=501, tid=1, mtid=1)         # another pos
    b.add(seq, pos=501, tid=1, mtid=1, l_qseq=40)  # another length over the same bytes
    b.add(seq, pos=501, tid=1, mtid=1, l_qseq=39)  # and one whose last byte is not looked at any more
    b.add(seq, pos=501, tid=1, mtid=1)
    b.add(other_first, pos=501, tid=1, mtid=1)  # the high nibble of the first byte
    b.add(other_second, pos=501, tid=1, mtid=1)  # the low nibble of the first byte
    b.add(other_last, pos=501, tid=1, mtid=1)  # the last base of an odd read: the high nibble of the last byte
    b.add(other_last, pos=501, tid=1, mtid=1, pad=9)  # the pad nibble
    b.add(other_last, pos=501, tid=1, mtid=1, pad=9)  # (a duplicate of that)
    b.add(other_last, pos=501, tid=1, mtid=1, pad=9, mapq=3, score_diff=1, sample=2, flag=2)  # other fields decide nothing
    b.add(other_last, pos=501, tid=1, mtid=2, pad=9)  # nor does mtid
    near = b.case("near misses", cuts=(2, 5, 11))
    b = Builder()
    b.add(bases(60, 1), pos=700)
    b.add(bases(60, 2), pos=700, flag=256)
    b.add(bases(60, 1), pos=700)
    b.add(bases(60, 1), pos=700, flag=2048)
    b.add(bases(60, 1), pos=700, flag=2048)
    b.add(bases(60, 1), pos=700)
    return [whole, near, b.case("a dropped record between two equal ones", cuts=(1, 2, 3, 4, 5))]


def _dups_flags():
    b = Builder()
    seq, mate = bases(70, 3), bases(70, 4)
    fr, rf = PAIRED | MATE_REVERSED | FIRST, PAIRED | REVERSED | SECOND
    # a head that aligns forward only and a duplicate whose own isize would not; then the other way round
    b.add(seq, pos=100, flag=fr, isize=300, name=1)
    b.add(seq, pos=100, flag=fr, isize=5000, name=2)
    b.add(seq, pos=100, flag=PAIRED | FIRST, isize=300, name=3)  # (own bits 16 and 32 equal)
    b.add(seq, pos=100, flag=0, name=4, sample=1)
    b.add(bases(70, 5), pos=150, flag=fr, isize=5000, name=5)
    b.add(bases(70, 5), pos=150, flag=fr, isize=300, name=6)
    b.add(bases(70, 5), pos=150, flag=0, name=7)
    for k, name in enumerate((1, 2, 3, 5, 6)):
        b.add(mate, pos=400 + k, flag=rf, isize=-300, name=name)
    heads = b.case("duplicates whose own flags or isize would decide otherwise", cuts=(2, 3, 5, 6))
    b = Builder()
    b.add([], pos=10)
    b.add([], pos=10)
    b.add([], pos=11)
    b.add([4], pos=11)
    b.add([4], pos=11)
    b.add([4], pos=11, pad=1)
    b.add([8], pos=11)
    b.add([4, 2], pos=11)
    return [heads, b.case("reads of no base and of one", cuts=(2, 4, 5))]


ISIZES = (-1200, -1199, 1199, 1200)


def _orient():
    out = []
    for force in (0, 1):
        b = Builder(force_align_both_orientations=force)
        k = 0
        for isize in ISIZES + (0, 300):
            for strand in (0, REVERSED, MATE_REVERSED, REVERSED | MATE_REVERSED):
                b.add(bases(35, k), pos=100 + k, flag=PAIRED | FIRST | strand, isize=isize)
                k += 1
        b.add(bases(35, k), pos=100 + k, flag=PAIRED | FIRST | REVERSED, isize=300, tid=0, mtid=1)
        b.add(bases(35, k + 1), pos=101 + k, flag=0, isize=5000, tid=0, mtid=1)
        b.add(bases(35, k + 2), pos=102 + k, flag=REVERSED | MATE_REVERSED)
        out.append(b.case("isize %s, the strands, another contig, unpaired; force_align_both_orientations %d" % (ISIZES, force)))
    return out


def cigar(op, length):
    return op | (length << 4)


def _hint():
    b = Builder()
    for k, (n_cigar, front, pos) in enumerate(((0, cigar(4, 10), 500), (2, cigar(4, 10), 500), (2, cigar(0, 10), 500), (2, cigar(5, 10), 500), (1, cigar(4, 3), 500),
                                               (3, cigar(4, 10), 5), (2, cigar(4, (1 << 28) - 1), 7), (2, cigar(4, 0), 9))):
        b.add(bases(30, k), pos=pos, n_cigar=n_cigar, cigar_front=front, cigar_back=cigar(4, 5))
    return [b.case("front operations S, M and H, no operation, a clip beyond pos")]


ROWS = ((80, 80, 0, (1, 31, 32, 33, 63, 64, 65, 159, 160)), (128, 128, 0, (161, 256)), (512, 512, 1000, (1000,)), (77, 80, 0, (1, 33, 153, 154)), (80, 96, 0, (159, 160)),
        (136, 64, 0, (127, 128)))


def _rows():
    out = []
    for seq_stride, plane_stride, max_len, lengths in ROWS:
        b = Builder(seq_stride=seq_stride, plane_stride=plane_stride, max_read_len=max_len)
        for k, l in enumerate(lengths):
            seq = (np.arange(l) % 16).astype(np.uint8) if k % 2 == 0 else bases(l, l)
            last = seq.copy()
            last[-1] ^= 6
            b.add(seq, pos=100 + k, pad=5)
            b.add(seq, pos=100 + k, pad=5)
            b.add(last, pos=100 + k, pad=5)
            b.add(last, pos=100 + k, pad=4 if l % 2 else 5)
        out.append(b.case("lengths %s on rows of %d bytes, plane rows of %d" % (lengths, seq_stride, plane_stride), cuts=(2, 6)))
    return out


APART = (1, 2, 63, 64, 65, 300)


def _pairs_apart():
    b = Builder(n_read_groups=2)
    mids = []
    for k, d in enumerate(APART):
        first = b.add(bases(25, k), pos=1000 * k, flag=PAIRED | FIRST | MATE_REVERSED, isize=200, name=500 + k, sample=1)
        for j in range(d - 1):
            b.add(bases(25, 1000 + j), pos=1000 * k + 1 + j, sample=j % 3)
        b.add(bases(25, 50 + k), pos=1000 * k + d, flag=PAIRED | SECOND | REVERSED, isize=-200, name=500 + k, sample=2)
        mids.append(first + (d + 1) // 2)
    # one name in two read groups: no pair; then each finds its own
    b.add(bases(25, 70), pos=9000, flag=PAIRED | FIRST, name=77, rg=0)
    b.add(bases(25, 71), pos=9001, flag=PAIRED | SECOND, name=77, rg=1)
    b.add(bases(25, 72), pos=9002, flag=PAIRED | FIRST, name=77, rg=1, sample=3)
    b.add(bases(25, 73), pos=9003, flag=PAIRED | SECOND, name=77, rg=0, sample=4)
    # an unpaired record meets a waiting one
    b.add(bases(25, 74), pos=9004, flag=PAIRED | FIRST, name=78, sample=1)
    b.add(bases(25, 75), pos=9005, flag=0, name=78, sample=2)
    n = len(b)
    return [b.case("mates %s records apart, one name in two read groups, other samples, an unpaired record that meets a waiting one" % (APART,), cuts=mids + [n - 5, n - 3, n - 1])]


def _pairs_many():
    b = Builder()
    k = 0
    for name, times in ((1, 3), (2, 4), (3, 200)):
        for j in range(times):
            b.add(bases(25, k), pos=100 + k, flag=PAIRED | (FIRST if j % 2 == 0 else SECOND), name=name, sample=j % 3)
            b.add(bases(25, 5000 + k), pos=100 + k, flag=0)
            k += 1
    b.add(bases(25, 9000), pos=9000, flag=PAIRED | FIRST, name=4)  # its mate never comes
    many = b.case("three, four and 200 occurrences of one name; a mate that never comes", cuts=(3, 7, 9, 100, 215))
    # the clash: records 0 .. 5 are fine and leave a mate parked and a record to be equal to; 6 .. 9 hold the clash; 10 .. 13 go on from the state behind 5
    b = Builder()
    b.add(bases(25, 1), pos=100, flag=PAIRED | FIRST, name=1)
    b.add(bases(25, 2), pos=101, flag=PAIRED | FIRST, name=2)
    b.add(bases(25, 3), pos=102, flag=PAIRED | SECOND, name=2)
    b.add(bases(25, 4), pos=103)
    b.add(bases(25, 4), pos=103)
    b.add(bases(25, 5), pos=104, flag=PAIRED | FIRST, name=3)
    b.add(bases(25, 5), pos=104, name=10)
    b.add(bases(25, 6), pos=105, flag=PAIRED | FIRST, name=3)  # the clash with the parked mate
    b.add(bases(25, 7), pos=106, flag=PAIRED | SECOND, name=1)
    b.add(bases(25, 8), pos=107)
    b.add(bases(25, 5), pos=104, name=11)  # equal to record 5, not to 9
    b.add(bases(25, 9), pos=108, flag=PAIRED | SECOND, name=3)
    b.add(bases(25, 10), pos=109, flag=PAIRED | SECOND, name=1)
    b.add(bases(25, 11), pos=110, flag=PAIRED | SECOND | FIRST, name=12)
    clash = b.case("two reads of one name with the same IS_FIRST_IN_PAIR", splits_agree=False,
                   scripts=[("the clash between two pushes that succeed", [push(0, 6), push(6, 10), push(10, 14)]),
                            ("the clash inside one push", [push(0, 5), push(5, 10), push(5, 6), push(10, 14)])])
    return [many, clash]


def _limits():
    out = []
    b = Builder()
    for k in range(6):
        b.add(bases(25, k), pos=100 + k, flag=PAIRED | FIRST if k < 3 else 0, name=k)
    short = [("align_cap one short, then with room", [push(0, 6, align_cap=5), push(0, 6)]), ("item_cap one short, then with room", [push(0, 6, item_cap=5), push(0, 6)]),
             ("both of no entry", [push(0, 6, 0, 0), push(0, 3), push(3, 6, 2, 3), push(3, 6)])]
    out.append(b.case("capacities one short", scripts=short))
    out.append(b.case("max_batch one short", max_batch=5, scripts=[("six records, then five and one", [push(0, 6), push(0, 5), push(5, 6)])]))
    out.append(b.case("parked_cap reached", parked_cap=3))
    out.append(b.case("parked_cap one over", parked_cap=2, splits_agree=False, scripts=[("three wait, then two", [push(0, 3), push(0, 2), push(3, 6), push(2, 3)])]))
    b = Builder(n_read_groups=3)
    b.add(bases(25, 1), pos=100, rg=2)
    b.add(bases(25, 2), pos=101, rg=3, flag=256)  # the filter would drop it
    b.add(bases(25, 3), pos=102, rg=1)
    out.append(b.case("a read group out of range on a record the filter drops", splits_agree=False))
    b = Builder(seq_stride=80, plane_stride=96)
    b.add(bases(160, 1), pos=100)
    b.add(bases(161, 2), pos=101)
    b.add(bases(20, 3), pos=102)
    out.append(b.case("a read one base too long for its nibble row", splits_agree=False))
    b = Builder(seq_stride=96, plane_stride=80)
    b.add(bases(160, 1), pos=100)
    b.add(bases(161, 2), pos=101)
    b.add(bases(20, 3), pos=102)
    out.append(b.case("a read one base too long for its plane row", splits_agree=False))
    b = Builder(seq_stride=144, plane_stride=144, n_read_groups=2)
    b.add(bases(256, 1), pos=100)
    b.add(bases(20, 2), pos=101)
    b.add(bases(257, 3), pos=102, flag=512)
    b.add(bases(20, 4), pos=103)
    b.add(bases(20, 5), pos=104, rg=2)
    out.append(b.case("a read of 257 bases in front of a read group out of range: the first record that fails decides", splits_agree=False, cuts=(4,)))
    return out


def _model():
    """5 000 records shaped like a position-sorted BAM of two read groups and three samples: pairs 300 +- 50 apart, 5 % duplicates, 3 %
    filtered, 2 % unpaired (of the records; the rates below are per template)"""
    rng = np.random.default_rng(2024)
    rows, pos, name = [], 10000, 0
    while len(rows) < 5200:  # (the last 200 are cut off: mates that never come)
        pos += int(rng.integers(0, 4))
        name += 1
        rg = int(rng.integers(0, 2))
        sample = int(rng.integers(0, 3))
        seq = bases(150, 7000 + name)
        if rng.random() < 0.04:
            rows.append((pos, 0, dict(codes=seq, flag=0, name=name, rg=rg, sample=sample)))
        else:
            ins = int(np.clip(rng.normal(300, 50), 160, 600))
            concordant = rng.random() < 0.9
            rows.append((pos, 0, dict(codes=seq, flag=PAIRED | FIRST | (MATE_REVERSED if concordant else 0), isize=ins, name=name, rg=rg, sample=sample,
                                      n_cigar=2, cigar_front=cigar(4, 5) if rng.random() < 0.1 else cigar(0, 150))))
            rows.append((pos + ins - 150, 1, dict(codes=bases(150, 9000 + name), flag=PAIRED | SECOND | REVERSED, isize=-ins, name=name, rg=rg, sample=sample)))
        if rng.random() < 0.1:  # a duplicate right behind its original, of another name
            rows.append((pos, 0, dict(codes=seq, flag=int(rng.choice([0, 1024])) if rng.random() < 0.5 else 0, name=(1 << 33) + name, rg=rg, sample=sample)))
        if rng.random() < 0.06:
            rows.append((pos, 0, dict(codes=bases(150, 11000 + name), flag=256, name=(1 << 34) + name, rg=rg, sample=sample)))
    rows.sort(key=lambda r: (r[0], r[1]))
    b = Builder(n_read_groups=2)
    for p, _, f in rows[:5000]:
        b.add(f.pop("codes"), pos=p, mapq=int(rng.integers(0, 61)), score_diff=int(rng.integers(0, 40)), **f)
    return [b.case("5 000 records like a sorted BAM", cuts=(257, 1000, 2500, 4999))]


DROP_BITS = (256, 1024, 2048)
AROUND = 5  # a template of _dropped_names: dropped, the first mate, dropped, the second mate, dropped


def _dropped_names():
    """records the filter drops that carry the (rg, name_id) of two mates: in front of the first mate, between the two and behind the
    second -- every bit of DROP_BITS, paired and unpaired, with either FIRST bit.  None of them waits, none is anybody's mate"""
    out = []
    for rg in (0, 1):
        b = Builder(n_read_groups=2)
        k = 0
        for bit in DROP_BITS:
            for paired in (PAIRED, 0):
                for which in (FIRST, SECOND):
                    name, at = 100 + k, 1000 + 10 * k
                    drop = dict(flag=bit | paired | which, name=name, rg=rg, sample=3)
                    b.add(bases(20, 5 * k), pos=at, **drop)
                    b.add(bases(20, 5 * k + 1), pos=at + 1, flag=PAIRED | FIRST | MATE_REVERSED, isize=200, name=name, rg=rg, sample=1)
                    b.add(bases(20, 5 * k + 2), pos=at + 2, **drop)
                    b.add(bases(20, 5 * k + 3), pos=at + 3, flag=PAIRED | SECOND | REVERSED, isize=-200, name=name, rg=rg, sample=2)
                    b.add(bases(20, 5 * k + 4), pos=at + 4, **drop)
                    k += 1
        n = len(b)
        out.append(b.case("dropped records with the mates' name in read group %d: before, between and behind them" % rg, cuts=range(1, n, 2),
                          scripts=[("cut at the even records", [push(lo, min(lo + 2, n)) for lo in range(0, n, 2)])]))
    return out


def _zero_first():
    """what the stream carries before its first kept record is all zeros: a first record of tid 0, pos 0 and no base is no duplicate"""
    out = []
    for dropped_in_front in (0, 1, 2):
        b = Builder()
        for k in range(dropped_in_front):
            b.add([], tid=0, pos=0, flag=1024 if k == 0 else 256, name=50 + k)
        b.add([], tid=0, pos=0, name=1)
        b.add([], tid=0, pos=0, name=2)
        b.add([], tid=0, pos=1, name=3)
        out.append(b.case("a first kept record of tid 0, pos 0 and no base behind %d dropped ones, then its duplicate" % dropped_in_front, cuts=(1, 2, 3)))
    return out


# which checks a record fails -> the fields that make it so on rows of 80 bytes with max_read_len 256 and two read groups
FAILS = dict(rg=dict(rg=2), long=dict(l_qseq=257), row=dict(l_qseq=161))
DOUBLE = (("rg", "long", ERR_ARG, WHY_RG), ("rg", "row", ERR_ARG, WHY_RG), ("long", "row", ERR_UNSUPPORTED, WHY_LONG), ("rg", "long", "row", ERR_ARG, WHY_RG))


def _fail_order():
    """a record that fails two checks or all three -- the host's order decides: rg, max_read_len, the rows --, and pushes whose first
    failing record fails a later check than a record behind it"""
    out = []
    for spec in DOUBLE:
        names = spec[:-2]
        # (257 bases fit rows of 144 bytes: `long` alone; on rows of 80 bytes they fail `row` as well)
        wide = "row" not in names
        b = Builder(seq_stride=144 if wide else 80, plane_stride=144 if wide else 80, n_read_groups=2)
        b.add(bases(30, 1), pos=100)
        f = dict(l_qseq=max(FAILS[k].get("l_qseq", 0) for k in names) or None, rg=2 if "rg" in names else 0)
        b.add(bases(30, 2), pos=101, **f)
        b.add(bases(30, 3), pos=102, rg=1)
        out.append(b.case("one record that fails %s" % " and ".join(names), splits_agree=False))
    # record 1 fails the rows, record 2 max_read_len, record 3 the read group: the first failing record decides, not the first check
    b = Builder(n_read_groups=2)
    b.add(bases(30, 1), pos=100)
    b.add(bases(30, 2), pos=101, l_qseq=161)
    b.add(bases(30, 3), pos=102, l_qseq=300, flag=2048)
    b.add(bases(30, 4), pos=103, rg=5)
    b.add(bases(30, 5), pos=104)
    out.append(b.case("a record too long for its row, then one beyond max_read_len, then a read group out of range", splits_agree=False, cuts=(2, 3),
                      scripts=[("from the second failing record", [push(2, 5)]), ("from the third", [push(3, 5)])]))
    # two records beyond max_read_len, the longer behind the shorter: the reason names the first one's length
    b = Builder(seq_stride=160, plane_stride=160)
    b.add(bases(30, 1), pos=100)
    b.add(bases(260, 2), pos=101)
    b.add(bases(300, 3), pos=102)
    out.append(b.case("a read of 300 bases behind a read of 260", splits_agree=False))
    # the steps behind classify load nothing of a failing push: two equal records too long for their rows at the very end (comparing them
    # would read behind the last row), and one at the end whose plane row would be made from bytes behind it
    b = Builder(seq_stride=80, plane_stride=96)
    b.add(bases(30, 1), pos=100)
    b.add(bases(30, 2), pos=101, l_qseq=161, times=2)
    out.append(b.case("two equal records at the end that are too long for their nibble rows", splits_agree=False))
    b = Builder(seq_stride=80, plane_stride=96)
    b.add(bases(30, 1), pos=100)
    b.add(bases(30, 2), pos=101, l_qseq=161)
    out.append(b.case("a record at the end that is too long for its nibble row", splits_agree=False))
    # the clash comes before the parked table's room: a push that has both
    b = Builder()
    for k, name in enumerate((2, 3, 1, 1)):
        b.add(bases(25, k), pos=100 + k, flag=PAIRED | FIRST, name=name)
    out.append(b.case("a clash in a push that leaves two mates for a parked table of one", splits_agree=False, parked_cap=1,
                      scripts=[("the clash alone, then the two mates", [push(2, 4), push(0, 2)])]))
    return out


PIECE_READS = ((64, 0), (1000, 1000))  # (bases, max_read_len)


def _pieces():
    """a read and copies of it that differ in one base, the read in between every two of them: every record is a head, and for every
    32-bit word of a 16-byte piece, for every piece of a 128-byte step and for the steps there is a copy that differs nowhere else"""
    out = []
    for l, max_len in PIECE_READS:
        b = Builder(seq_stride=(l // 2 + 15) // 16 * 16, plane_stride=(l // 2 + 15) // 16 * 16, max_read_len=max_len)
        seq = bases(l, l)
        for byte in piece_bytes(l):
            other = seq.copy()
            other[2 * byte + byte % 2] ^= 3
            b.add(seq, pos=100)
            b.add(other, pos=100)
        b.add(seq, pos=100, times=2)
        out.append(b.case("a read of %d bases and its copies that differ in one base" % l, cuts=(2, 3)))
    return out


def piece_bytes(l):
    """the bytes at which _pieces' copies differ: of 32 bytes every fourth (the words of both pieces); of 500 bytes one in every 16-byte
    piece, at another place in each, and the last"""
    return list(range(0, 32, 4)) if l == 64 else [min(16 * j + (5 * j) % 16, 499) for j in range(32)]


FRONT_OPS = tuple(range(16))


def _front_ops():
    b = Builder()
    for op in FRONT_OPS:
        b.add(bases(30, op), pos=500 + 20 * op, n_cigar=2, cigar_front=cigar(op, 10), cigar_back=cigar(4, 7))
    return [b.case("every front operation 0 .. 15 with n_cigar 2: only S (4) moves the hint")]


GROUPS = ((5, (0, 4)), (65536, (0, 255, 256, 65535)))


def _groups():
    """one name in several read groups whose numbers differ in their highest bits only (0 and 4 of 5; 0, 255, 256 and 65 535 of 65 536),
    the mates interleaved: a sort by read group that looks at too few bits, or a key cut to 8 or 16 bits, pairs mates of two groups"""
    out = []
    for n_read_groups, groups in GROUPS:
        b = Builder(n_read_groups=n_read_groups)
        k = 0
        for name in (9, 3):
            for rg in groups:
                b.add(bases(25, k), pos=100 + k, flag=PAIRED | FIRST | MATE_REVERSED, isize=200, name=name, rg=rg, sample=0)
                k += 1
            b.add(bases(25, k), pos=100 + k, name=name, rg=groups[0])  # (an unpaired record of the name meets the waiting one of its group)
            k += 1
            for rg in groups[:0:-1]:
                b.add(bases(25, k), pos=100 + k, flag=PAIRED | SECOND | REVERSED, isize=-200, name=name, rg=rg, sample=1 + groups.index(rg))
                k += 1
        b.add(bases(25, k), pos=100 + k, flag=PAIRED | FIRST, name=9, rg=n_read_groups - 1)  # waits to the end
        out.append(b.case("one name in the read groups %s of %d" % (groups, n_read_groups), cuts=range(2, len(b), 3)))
    return out


SETS = dict(filters=_filters, dups_runs=_dups_runs, dups_flags=_dups_flags, orient=_orient, hint=_hint, rows=_rows, pairs_apart=_pairs_apart, pairs_many=_pairs_many,
            limits=_limits, dropped_names=_dropped_names, zero_first=_zero_first, fail_order=_fail_order, front_ops=_front_ops, groups=_groups, pieces=_pieces,
            model=_model)


@functools.lru_cache(maxsize=None)
def cases(name):
    return SETS[name]()


# ---- what each set is for -----------------------------------------------------------------------------------------------------------
def whole(c):
    w, = c.want("whole")
    return w


def facts_filters(cs):
    on, off, dropped, empty, among = cs
    assert whole(on)["counts"] == (5, 0, 0) and whole(off)["counts"] == (13, 0, 0) and len(whole(on)["items"]) == 5
    assert {int(r["flag"]) & 3840 for r in on.recs} == {0} | set(FILTER_BITS)
    assert whole(dropped)["counts"] == (0, 0, 0) and whole(dropped)["status"] == OK and len(whole(dropped)["meta"]) == 0
    assert [q.hi - q.lo for q in dict(empty.scripts)["with empty pushes"]].count(0) == 3
    assert whole(among)["counts"] == (3, 2, 0) and len(whole(among)["meta"]) == 1


def facts_dups_runs(cs):
    runs, near, between = cs
    w = whole(runs)
    assert len(w["meta"]) == len(RUNS) and w["counts"] == (sum(RUNS), sum(RUNS) - len(RUNS), 0)
    assert [int((w["items"]["first"]["align_index"] == k).sum()) for k in range(len(RUNS))] == list(RUNS)
    w = whole(near)
    # of the 14 records the third and the last three are duplicates and no other
    assert w["items"]["first"]["align_index"].tolist() == [0, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 9] and w["counts"] == (14, 4, 0)
    w = whole(between)
    assert w["counts"] == (3, 2, 0) and len(w["meta"]) == 1


def facts_dups_flags(cs):
    heads, short = cs
    w = whole(heads)
    assert len(w["meta"]) == 2 + 5 and w["counts"] == (12, 5, 0)
    fo = {int(i["first"]["align_index"]): int(i["first"]["flag"]) & FORWARD_ONLY for i in w["items"]}
    assert fo[0] == FORWARD_ONLY and fo[1] == 0
    first = [i["first"] for i in w["items"]]
    assert all(int(m["flag"]) & FORWARD_ONLY for m in first if m["align_index"] == 0) and sum(1 for m in first if m["align_index"] == 0) == 4
    assert not any(int(m["flag"]) & FORWARD_ONLY for m in first if m["align_index"] == 1) and sum(1 for m in first if m["align_index"] == 1) == 3
    # ... though two of the first group would not align forward only by themselves, and two of the second would
    assert [forward_only(heads.p, r) for r in heads.recs[:7]] == [FORWARD_ONLY, 0, 0, FORWARD_ONLY, 0, FORWARD_ONLY, FORWARD_ONLY]
    w = whole(short)
    assert w["meta"]["l_qseq"].tolist() == [0, 0, 1, 1, 1, 2] and w["counts"] == (8, 2, 0)


def facts_orient(cs):
    plain, forced = cs
    w = whole(plain)
    got = (w["meta"]["flag"] & FORWARD_ONLY != 0).tolist()
    want = []
    for isize in ISIZES + (0, 300):
        want += [False, -1200 < isize < 1200, -1200 < isize < 1200, False]
    assert got == want + [False, True, True] and True in got[4:12] and got[0:4] == [False] * 4 and got[12:16] == [False] * 4
    assert not (whole(forced)["meta"]["flag"] & FORWARD_ONLY).any()


def facts_hint(cs):
    w = whole(cs[0])
    assert w["meta"]["pos"].tolist() == [500, 490, 500, 500, 497, -5, 7 - ((1 << 28) - 1), 9]


def facts_rows(cs):
    assert [(c.seq_stride, c.plane_stride, max_read_len_of(c.p)) for c in cs] == [(80, 80, 256), (128, 128, 256), (512, 512, 1000), (77, 80, 256), (80, 96, 256), (136, 64, 256)]
    for c, (_, _, _, lengths) in zip(cs, ROWS):
        w = whole(c)
        # per length: a head, its duplicate, a head that differs in the last base, and an odd read's other pad nibble is a head too
        assert w["counts"] == (4 * len(lengths), sum(1 + (l % 2 == 0) for l in lengths), 0)
        assert w["meta"]["l_qseq"].tolist() == [l for l in lengths for _ in range(2 + l % 2)]
    r = cs[0].rows[16][:31]  # (63 bases: every nibble code)
    assert set((r >> 4).tolist()) | set((r & 15).tolist()) == set(range(16))


def facts_pairs_apart(cs):
    w = whole(cs[0])
    pairs = [i for i in w["items"] if i["second"]["align_index"] != INVALID]
    assert len(pairs) == len(APART) + 3 and [int(i["sample"]) for i in pairs] == [2] * len(APART) + [3, 4, 2]
    assert [int(i["second"]["align_index"]) - int(i["first"]["align_index"]) for i in pairs[:len(APART)]] == list(APART)
    assert w["counts"][2] == 0


def facts_pairs_many(cs):
    many, clash = cs
    w = whole(many)
    pairs = [i for i in w["items"] if i["second"]["align_index"] != INVALID]
    assert len(pairs) == 1 + 2 + 100 and w["counts"][2] == 2 and len(w["items"]) == 103 + 207
    assert whole(clash)["status"] == ERR_ARG
    a, b = clash.want("the clash between two pushes that succeed"), clash.want("the clash inside one push")
    assert [x["status"] for x in a] == [OK, ERR_ARG, OK] and [x["status"] for x in b] == [OK, ERR_ARG, OK, OK]
    assert a[1]["counts"] == a[0]["counts"] == (6, 1, 2) and a[2]["counts"] == (10, 2, 1)
    # the push behind the failing one: a duplicate of the record carried from the first push, and the mates of two parked there
    assert a[2]["items"]["first"]["align_index"].tolist() == [4, 4, 0] and a[2]["meta"].shape == (3,)
    assert clash.total("the clash between two pushes that succeed") == clash.total("the clash inside one push")


def facts_limits(cs):
    caps, batch, reached, over, rg, nib, plane, first = cs
    for name, _ in caps.scripts[3:]:
        assert caps.want(name)[0]["status"] == ERR_CAPACITY and caps.want(name)[-1]["status"] == OK and caps.total(name) == caps.total()
    assert [w["status"] for w in caps.want("both of no entry")] == [ERR_CAPACITY, OK, ERR_CAPACITY, OK]
    assert [w["status"] for w in batch.want("six records, then five and one")] == [ERR_CAPACITY, OK, OK]
    assert whole(reached)["status"] == OK and whole(reached)["counts"][2] == 3
    assert whole(over)["status"] == ERR_CAPACITY and [w["status"] for w in over.want("three wait, then two")] == [ERR_CAPACITY, OK, OK, ERR_CAPACITY]
    assert whole(rg)["status"] == ERR_ARG and [w["status"] for w in rg.want("one record a push")] == [OK, ERR_ARG, OK]
    assert whole(nib)["status"] == ERR_ARG and whole(plane)["status"] == ERR_ARG and [w["status"] for w in plane.want("one record a push")] == [OK, ERR_ARG, OK]
    assert whole(first)["status"] == ERR_UNSUPPORTED and [w["status"] for w in first.want("one record a push")] == [OK, OK, ERR_UNSUPPORTED, OK, ERR_ARG]


def facts_model(cs):
    c, = cs
    w = whole(c)
    n = len(c.recs)
    records, duplicated, parked = w["counts"]
    assert n == 5000 and 0.02 * n < n - records < 0.08 * n and 0.02 * n < duplicated < 0.08 * n and 0 < parked < 400
    pairs = w["items"][w["items"]["second"]["align_index"] != INVALID]
    apart = pairs["second"]["pos"] - pairs["first"]["pos"]
    assert len(pairs) > 2000 and 100 < np.median(apart) < 200 and set(c.recs["rg"].tolist()) == {0, 1} and set(c.recs["sample"].tolist()) == {0, 1, 2}
    assert sum(1 for r in c.recs if r["n_cigar"] and (int(r["cigar_front"]) & 15) == 4) > 50  # (clipped hints)
    assert (pairs["first"]["flag"] & FORWARD_ONLY != 0).sum() > 1500 and (pairs["first"]["flag"] & FORWARD_ONLY == 0).sum() > 100


def facts_dropped_names(cs):
    for rg, c in enumerate(cs):
        templates = len(c.recs) // AROUND
        assert templates == len(DROP_BITS) * 2 * 2 and len(c.recs) == templates * AROUND
        seen = set()
        for t in range(templates):
            before, first, between, second, behind = c.recs[AROUND * t:AROUND * t + AROUND]
            # the three dropped records carry the mates' key, and the filter drops them for one bit
            assert len({(int(r["rg"]), int(r["name_id"])) for r in (before, first, between, second, behind)}) == 1 and int(first["rg"]) == rg
            assert int(before["flag"]) == int(between["flag"]) == int(behind["flag"]) and (int(first["flag"]) | int(second["flag"])) & c.p["sam_flag_filter"] == 0
            dropped = int(before["flag"])
            assert dropped & c.p["sam_flag_filter"] in DROP_BITS and bool(dropped & FIRST) != bool(dropped & SECOND)
            seen.add((dropped & c.p["sam_flag_filter"], dropped & PAIRED, dropped & FIRST))
        assert len(seen) == templates  # every bit, paired and unpaired, either FIRST bit
        for script, _ in c.scripts:
            ws = [w for w in c.want(script)]
            items = np.concatenate([w["items"] for w in ws])
            # every item is the pair of a template's two mates with the second mate's sample, and nothing waits at the end
            assert all(w["status"] == OK for w in ws) and ws[-1]["counts"] == (2 * templates, 0, 0) and len(items) == templates
            assert (items["second"]["pos"] - items["first"]["pos"] == 2).all() and (items["sample"] == 2).all()
        assert max(q.hi - q.lo for q in dict(c.scripts)["cut at the even records"]) == 2 and "cut at %s" % list(range(1, len(c.recs), 2)) in dict(c.scripts)


def facts_zero_first(cs):
    for k, c in enumerate(cs):
        first = c.recs[k]
        assert (c.recs[:k]["flag"] & c.p["sam_flag_filter"] != 0).all() and (int(first["tid"]), int(first["pos"]), int(first["l_qseq"]), int(first["flag"])) == (0, 0, 0, 0)
        for script, _ in c.scripts:
            ws = c.want(script)
            # the first kept record is a head though every field the comparison looks at is zero, the second its duplicate
            assert ws[-1]["counts"] == (3, 1, 0) and sum(len(w["meta"]) for w in ws) == 2
            assert np.concatenate([w["items"] for w in ws])["first"]["align_index"].tolist() == [0, 0, 1]
        assert [len(w["meta"]) for w in c.want("one record a push")] == [0] * k + [1, 0, 1]


def facts_fail_order(cs):
    doubles, (order, longer, two_at_the_end, one_at_the_end, both) = cs[:len(DOUBLE)], cs[len(DOUBLE):]
    for c, spec in zip(doubles, DOUBLE):
        names, status, why = spec[:-2], spec[-2], spec[-1]
        r, l = c.recs[1], int(c.recs[1]["l_qseq"])
        fails = dict(rg=int(r["rg"]) >= c.n_read_groups, long=l > max_read_len_of(c.p), row=(l + 1) // 2 > c.seq_stride or l > 2 * c.plane_stride)
        assert {k for k, v in fails.items() if v} == set(names) and len(names) >= 2
        w = whole(c)
        assert (w["status"], w["reason"]) == (status, (why, 1, l, 0))
        assert [x["status"] for x in c.want("one record a push")] == [OK, status, OK] and c.want("one record a push")[1]["reason"] == (why, 0, l, 0)
    assert {(s[-2], s[-1]) for s in DOUBLE} == {(ERR_ARG, WHY_RG), (ERR_UNSUPPORTED, WHY_LONG)}
    # the first failing record decides though both records behind it fail an earlier check
    assert (whole(order)["status"], whole(order)["reason"]) == (ERR_ARG, (WHY_ROW, 1, 161, 0))
    assert order.want("from the second failing record")[0]["reason"] == (WHY_LONG, 0, 300, 0) and order.want("from the second failing record")[0]["status"] == ERR_UNSUPPORTED
    assert order.want("from the third")[0]["reason"] == (WHY_RG, 0, 30, 0) and order.want("from the third")[0]["status"] == ERR_ARG
    assert int(order.recs[2]["flag"]) & order.p["sam_flag_filter"]  # (a record the filter drops is checked like any other)
    assert (whole(longer)["status"], whole(longer)["reason"]) == (ERR_UNSUPPORTED, (WHY_LONG, 1, 260, 0)) and longer.recs["l_qseq"].tolist() == [30, 260, 300]
    # what a step behind classify would load of a failing push lies behind the last row: the two last records are equal in all the
    # comparison looks at first, and one byte longer than a row; a last record that would be a head, its plane row longer than its row
    a, b = two_at_the_end.recs[-2:]
    assert (a["tid"], a["pos"], a["l_qseq"]) == (b["tid"], b["pos"], b["l_qseq"]) and (int(a["l_qseq"]) + 1) // 2 == two_at_the_end.seq_stride + 1
    assert whole(two_at_the_end)["reason"] == (WHY_ROW, 1, 161, 0) and whole(one_at_the_end)["reason"] == (WHY_ROW, 1, 161, 0)
    assert one_at_the_end.plane_stride > one_at_the_end.seq_stride and len(one_at_the_end.recs) == 2
    # the clash decides in front of the parked table's room
    assert (whole(both)["status"], whole(both)["reason"]) == (ERR_ARG, (WHY_CLASH, 0, 0, 0)) and both.parked_cap == 1
    alone, mates = both.want("the clash alone, then the two mates")
    assert (alone["status"], alone["reason"]) == (ERR_ARG, (WHY_CLASH, 0, 0, 0)) and (mates["status"], mates["reason"]) == (ERR_CAPACITY, (WHY_PARKED, 0, 0, 2))


def facts_pieces(cs):
    for c, (l, _) in zip(cs, PIECE_READS):
        at = piece_bytes(l)
        n = 2 * len(at) + 2
        w = whole(c)
        # every record but the last is a head: it differs from the one in front of it in one base, and so in one byte of its row
        assert len(c.recs) == n and w["counts"] == (n, 1, 0) and len(w["meta"]) == n - 1 and (c.recs["l_qseq"] == l).all()
        read = c.rows[:, :(l + 1) // 2]  # (behind it every row has bytes of its own)
        for k, byte in enumerate(at):
            assert np.flatnonzero(read[2 * k] != read[2 * k + 1]).tolist() == [byte] and (read[2 * k] == read[0]).all()
        assert (read[n - 1] == read[n - 2]).all() and c.seq_stride % 16 == 0 and c.seq_stride - (l + 1) // 2 < 16
    assert {b % 16 // 4 for b in piece_bytes(64)} == {0, 1, 2, 3} and {b // 16 for b in piece_bytes(64)} == {0, 1}
    long = piece_bytes(1000)
    # one copy per 16-byte piece of the 500 bytes (the last piece is cut by the read's end), so per piece of a 128-byte step and per step
    assert [b // 16 for b in long] == list(range(32)) and long[-1] == 499 and {b // 128 for b in long} == {0, 1, 2, 3} and {b % 128 // 16 for b in long} == set(range(8))


def facts_front_ops(cs):
    c, = cs
    w = whole(c)
    assert [int(f) & 15 for f in c.recs["cigar_front"]] == list(FRONT_OPS) and set(range(10)) | {12} <= set(FRONT_OPS) and (c.recs["n_cigar"] != 0).all()
    assert (c.recs["cigar_front"] >> 4 == 10).all()
    assert (c.recs["pos"] - w["meta"]["pos"]).tolist() == [10 if op == 4 else 0 for op in FRONT_OPS]


def facts_groups(cs):
    assert [c.n_read_groups for c in cs] == [n for n, _ in GROUPS]
    for c, (n_read_groups, groups) in zip(cs, GROUPS):
        assert set(c.recs["rg"].tolist()) == set(groups) and max(groups) == n_read_groups - 1 and len(set(c.recs["name_id"].tolist())) == 2
        for script, _ in c.scripts:
            ws = c.want(script)
            items = np.concatenate([w["items"] for w in ws])
            rg_of = {int(r["pos"]): int(r["rg"]) for r in c.recs}  # (every record has a pos of its own)
            # 2 names x every group: a pair inside the group, never across; the sample says which group's mate closed it
            assert len(items) == 2 * len(groups) and ws[-1]["counts"] == (len(c.recs), 0, 1)
            assert all(rg_of[int(i["first"]["pos"])] == rg_of[int(i["second"]["pos"])] for i in items)
            assert sorted(int(i["sample"]) for i in items) == sorted([0] * 2 + [1 + k for k in range(1, len(groups))] * 2)
    # the groups of one name differ in bit 2 only (of 3 bits), or in bits 8 .. 15: keys cut to 2, 8 or 16 bits confuse them
    assert 4 & 3 == 0 and 256 & 255 == 0 and 65535 & 255 == 255 and len({g & 0xFFFF for g in GROUPS[1][1]}) == 4


FACTS = dict(filters=facts_filters, dups_runs=facts_dups_runs, dups_flags=facts_dups_flags, orient=facts_orient, hint=facts_hint, rows=facts_rows,
             pairs_apart=facts_pairs_apart, pairs_many=facts_pairs_many, limits=facts_limits, dropped_names=facts_dropped_names, zero_first=facts_zero_first,
             fail_order=facts_fail_order, front_ops=facts_front_ops, groups=facts_groups, pieces=facts_pieces, model=facts_model)


# ---- the judge ------------------------------------------------------------------------------------------------------------------------
SIZES = dict(planes=None, meta=gtx.READ_META.itemsize, items=gtx.SCORE_ITEM.itemsize)


def guarded(n_bytes):
    """an output before the push: n_bytes of FILL and a guard behind them"""
    return np.full(n_bytes + GUARD, FILL, np.uint8)


def differs(c, q, room, want, got):
    """got: dict(status, n_align, n_items, counts, planes, meta, items[, reason]) -- reason: the four words of the device's download that
    say why a push failed (the emulation has them; the library turns them into gtx_last_error), the three outputs as uint8 arrays of `room` entries and a guard,
    as guarded() made them and the push left them"""
    if int(got["status"]) != want["status"]:
        return "status %d for %d" % (got["status"], want["status"])
    if tuple(int(x) for x in got["counts"]) != want["counts"]:
        return "counts %s for %s" % (tuple(got["counts"]), want["counts"])
    if "reason" in got and tuple(int(x) for x in got["reason"]) != want["reason"]:
        return "reason (why, record, l_qseq, n_parked) %s for %s" % (tuple(got["reason"]), want["reason"])
    if (int(got["n_align"]), int(got["n_items"])) != (len(want["meta"]), len(want["items"])):
        return "%d tasks and %d items for %d and %d" % (got["n_align"], got["n_items"], len(want["meta"]), len(want["items"]))
    for what, entries in (("planes", room[0]), ("meta", room[0]), ("items", room[1])):
        size = entries * (c.plane_stride if what == "planes" else SIZES[what])
        out = np.asarray(got[what], np.uint8)
        if len(out) != size + GUARD:
            return "%s: %d bytes for %d" % (what, len(out) - GUARD, size)
        if (out[size:] != FILL).any():
            return "%s: a guard byte was written" % what
        if want["status"] != OK:
            continue
        table = np.ascontiguousarray(want[what]).view(np.uint8).reshape(-1)
        wrong = np.flatnonzero(out[:size] != table)
        if len(wrong):
            at = int(wrong[0])
            return "%s: byte %d is %d for %d (%d bytes differ)" % (what, at, out[at], table[at], len(wrong))
    return None


def judge(name, run):
    """None when the program behind `run` -- run(case, pushes, rooms) -> one result per push -- leaves what the definition says for every
    case of the set `name` under every one of its scripts, else what differs"""
    for k, c in enumerate(cases(name)):
        for script, pushes in c.scripts:
            wants, rooms = c.want(script), c.rooms(script)
            gots = run(c, pushes, rooms)
            if len(gots) != len(pushes):
                return "case %d (%s), %s: %d results for %d pushes" % (k, c.label, script, len(gots), len(pushes))
            for j, (q, room, want, got) in enumerate(zip(pushes, rooms, wants, gots)):
                how = differs(c, q, room, want, got)
                if how is not None:
                    return "case %d (%s), %s, push %d [%d, %d): %s" % (k, c.label, script, j, q.lo, q.hi, how)
    return None


# ---- the emulation's files --------------------------------------------------------------------------------------------------------------
def write_case(path, c, pushes, rooms, waves):
    """the input of tests/emu_dstream: 12 uint32 (sam_flag_filter, force_align_both_orientations, max_read_len, n_read_groups, max_batch,
    parked_cap, seq_stride, plane_stride, waves, n_pushes, n_records, 0), the records, their rows, per push 6 uint32 (lo, hi, align_cap,
    item_cap, and the entries its output arrays hold: tasks, items)"""
    with open(path, "wb") as out:
        out.write(struct.pack("<12I", c.p["sam_flag_filter"], c.p["force_align_both_orientations"], c.p["max_read_len"], c.n_read_groups, c.max_batch, c.parked_cap,
                              c.seq_stride, c.plane_stride, waves, len(pushes), len(c.recs), 0))
        out.write(c.recs.tobytes() + c.rows.tobytes())
        for q, room in zip(pushes, rooms):
            out.write(struct.pack("<6I", q.lo, q.hi, q.align_cap, q.item_cap, room[0], room[1]))


def read_result(path, c, rooms):
    """what the program wrote -- per push 8 uint32 (status, n_align, n_items, 0, then the reason: why, record, l_qseq, n_parked), 3 uint64
    (the counts), then its three output arrays of exactly the push's room -- with a guard of this module's making behind each"""
    raw, at, out = np.fromfile(path, np.uint8), 0, []
    for room in rooms:
        status, n_align, n_items, _, why, record, l_qseq, n_parked = struct.unpack_from("<8I", raw, at)
        got = dict(status=status, n_align=n_align, n_items=n_items, counts=struct.unpack_from("<3Q", raw, at + 32), reason=(why, record, l_qseq, n_parked))
        at += 56
        for what, entries in (("planes", room[0]), ("meta", room[0]), ("items", room[1])):
            size = entries * (c.plane_stride if what == "planes" else SIZES[what])
            g = guarded(size)
            g[:size] = raw[at:at + size]
            got[what] = g
            at += size
        out.append(got)
    assert at == len(raw), (at, len(raw))
    return out


def through(run, waves, c, pushes, rooms):
    """run: emu_programs.run bound to a program and a directory"""
    return run(lambda path: write_case(path, c, pushes, rooms, waves), lambda path: read_result(path, c, rooms))
