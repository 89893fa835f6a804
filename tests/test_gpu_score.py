"""gtx_score_batch* on the device over hand-made records and items: every case set of tests/score_cases.py against the plain restatement
(tests/score_ref.py) array by array -- the wavefront groups, the LDS table and its flush, the staging of a record through LDS, the piece
loop, the triage kernel's queue and the second pass run nowhere but here --; all accumulators in ONE device block (what gtx_scores_alloc
makes, and what lets the scoring kernel's table name a counter by its distance from the lowest) with 4 096 bytes of 0xA5 in front of,
between and behind them that stay as they were; items, records, d_compact, the side array and the queue bit-identical afterwards; the
five entry points; three calls in a row into one block on a stream of the caller's; no items; the connection log's capacity.  All
values are integers; there is no tolerance.  The same sets on the host: test_score_emu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import harness
import score_cases as sc
import score_ref as ref
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu
GUARD = 4096  # bytes in front of, between and behind the accumulators, filled with 0xA5
ARRAYS = (("log_score", np.uint32), ("gt_cov", np.uint32), ("hap_u32", np.uint32), ("stat_u64", np.uint64), ("stat_u32", np.uint32),
          ("conn_near", np.uint32), ("conn_log", np.uint32), ("conn_count", np.uint32))


@functools.lru_cache(maxsize=None)
def device_ctx(params=()):
    return gtx.Context(sc.graph(), device=0, **dict(params))


class Block:
    """the accumulators of one case in one device block, guards around each"""

    def __init__(self, case, conn_cap):
        import torch
        sizes = ref.Sums(sc.facts(), case.n_samples).sizes()
        sizes.update(conn_log=conn_cap * 6, conn_count=2)
        if not case.near:
            sizes["conn_near"] = 0
        self.case, self.conn_cap, self.spans, at = case, conn_cap, {}, GUARD
        for name, dtype in ARRAYS:
            n = sizes[name] * np.dtype(dtype).itemsize
            self.spans[name] = (at, n)
            at += (n + 7) // 8 * 8 + GUARD
        host = np.full(at, 0xA5, np.uint8)
        for a, n in self.spans.values():
            host[a:a + n] = 0
        self.clean = host
        self.dev = torch.from_numpy(host.copy()).to("cuda:0")
        p = {name: self.dev.data_ptr() + a for name, (a, n) in self.spans.items()}
        self.buf = gtx.ScoreBuffers(case.n_samples, p["log_score"], p["gt_cov"], p["hap_u32"], p["stat_u64"], p["stat_u32"], p["conn_log"], p["conn_count"],
                                    conn_cap, p["conn_near"] if case.near else None, None, 0)

    def got(self):
        """-> score_cases.Got; every byte outside the accumulators is still a guard byte"""
        host = self.dev.cpu().numpy()
        outside = np.ones(len(host), bool)
        arrays = {}
        for name, dtype in ARRAYS:
            a, n = self.spans[name]
            outside[a:a + n] = False
            arrays[name] = host[a:a + n].view(dtype).copy()
        assert (host[outside] == 0xA5).all(), "a byte outside the accumulators was written"
        arrays["conn_log"] = arrays["conn_log"].reshape(-1, 6)
        if not self.case.near:
            arrays["conn_near"] = None
        return sc.Got(**arrays)


def work_items(case, want):
    """the items the first stage queues: those the restatement does not call trivial"""
    return [i for i, it in enumerate(want.items) if not it["trivial"]]


def device_score(case, want, entry="batch", items=None, conn_cap=None, block=None, stream=None, queue=None, n_items=None):
    """one call of an entry point over the case -> the block it added to.  Checks what every call has to keep: the inputs, the count of
    refused items"""
    import torch
    ctx = device_ctx(case.params)
    items = case.items if items is None else items
    compact = entry in ("compact", "queued") and bool(case.compact_reads)
    block = block or Block(case, sum(want.conn_log.values()) + 16 if conn_cap is None else conn_cap)
    inputs = dict(items=items, records=case.records_beside_compact if compact else case.records, side=case.side, compact=case.compact,
                  words=gtx.item_words(items))
    if entry == "queued":
        q = np.array(work_items(case, want) if queue is None else queue, np.uint32)
        inputs["work"] = np.concatenate([np.array([len(q), 0, 0, 0], np.uint32), q, np.full(len(items) - len(q), 0xFFFFFFFF, np.uint32)])
    dev = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy()).to("cuda:0") for k, v in inputs.items()}
    p = {k: d.data_ptr() for k, d in dev.items()}
    L, st, n, rw, buf = gtx.lib(), None if stream is None else C.c_void_p(stream.cuda_stream), len(items) if n_items is None else n_items, case.rec_words, C.byref(block.buf)
    before = ctx.error_count()
    torch.cuda.synchronize()
    if entry == "batch":
        rc = L.gtx_score_batch(ctx.h, p["items"], n, p["records"], rw, buf, st)
    elif entry == "flags":
        rc = L.gtx_score_batch_flags(ctx.h, p["items"], n, p["records"], rw, p["side"], buf, st)
    elif entry == "words":
        rc = L.gtx_score_batch_words(ctx.h, p["items"], p["words"], n, p["records"], rw, p["side"], buf, st)
    elif entry == "compact":
        rc = L.gtx_score_batch_compact(ctx.h, p["items"], p["words"], n, p["records"], rw, p["compact"], p["side"], buf, st)
    else:
        rc = L.gtx_score_batch_queued(ctx.h, p["items"], n, p["records"], rw, p["compact"] if compact else None, p["side"], p["work"], buf, st)
    gtx.check(rc)
    torch.cuda.synchronize()
    for k, v in inputs.items():
        assert np.array_equal(np.ascontiguousarray(v).view(np.uint8).reshape(-1), dev[k].cpu().numpy()), "the call wrote its input: " + k
    assert ctx.error_count() == before == 0, "an item was refused by both passes"
    return block


@pytest.mark.parametrize("name", sc.SANITIZED)
def test_every_array_equals_the_restatement(name):
    for k, (case, want) in enumerate(zip(sc.cases(name), sc.expected(name))):
        got = device_score(case, want).got()
        assert sc.differences(case, want, got) == [], k
        # the second witness: the oracle over the same paths (the items it can be asked about: the others add nothing on the device)
        acc = harness.Accumulators(sc.host_ctx(case.params), case.n_samples, conn_cap=len(got.conn_log), near=case.near)
        for a, g in zip(acc.arrays(), [got.log_score, got.gt_cov, got.hap_u32, got.stat_u64, got.stat_u32, got.conn_log.reshape(-1), got.conn_count] + ([got.conn_near] if case.near else [])):
            a[:] = g
        oracle = sc.oracle_scores(case, case.items[sc.held_to_the_oracle(case)])
        assert np.array_equal(harness.canonical_scores(sc.host_ctx(case.params), acc), oracle), k


def test_aligned_records_on_the_device():
    """records in the arena and records with wide allele sets (gtx_score_wide_kernel), made by the aligner, under hand-made items"""
    sets = sc.aligned_records(harness.GpuBackend)
    exp = [a.restate() for a in sets]
    sc.facts_aligned_records(sets, exp)  # (the device's own records have to reach what the set is for)
    for a, want in zip(sets, exp):
        got, acc = a.backend_score()
        assert sc.differences(a, want, got, conn_cap=acc.conn_cap) == [], a.name
        assert np.array_equal(harness.canonical_scores(a.ctx, acc), sc.oracle_scores(a, a.items)), a.name  # the oracle over the same words and arena


def test_many_items_take_a_second_piece_and_pass_32_bits():
    (case,), (want,) = sc.cases("many_items"), sc.expected("many_items")
    assert len(case.all_items) == sc.MANY_ITEMS
    assert sc.differences(case, want, device_score(case, want, items=case.all_items).got()) == []


@pytest.mark.parametrize("entry", ["flags", "words", "compact", "queued"])
def test_the_other_entry_points_give_the_same_accumulators(entry):
    for name in sc.SANITIZED:
        for k, (case, want) in enumerate(zip(sc.cases(name), sc.expected(name))):
            assert sc.differences(case, want, device_score(case, want, entry).got()) == [], (name, k)


def test_a_hand_made_queue_in_any_order_and_a_part_of_it():
    for name in sc.SANITIZED:
        for k, (case, want) in enumerate(zip(sc.cases(name), sc.expected(name))):
            work = work_items(case, want)
            assert sc.differences(case, want, device_score(case, want, "queued", queue=work[::-1]).got()) == [], (name, k)
            part = work[1::2]
            mult = [int(i in part) for i in range(len(case.items))]
            want_part = sc.restate(case, case.items, mult)
            assert sc.differences(case, want_part, device_score(case, want_part, "queued", queue=part).got()) == [], (name, k)


def test_three_calls_into_one_block_on_a_stream_of_the_callers():
    """the first and the third need the second pass: the two sets of state words are used in turn, and the sums add up"""
    import torch
    (tables,), (want_tables,) = sc.cases("site_tables"), sc.expected("site_tables")
    middle, want_middle = sc.cases("connections")[0], sc.expected("connections")[0]
    assert sc.second_pass_items(want_tables) and not sc.second_pass_items(want_middle) and tables.n_samples == middle.n_samples and middle.near
    total = ref.Sums(sc.facts(), tables.n_samples)
    for w, times in ((want_tables, 2), (want_middle, 1)):
        for name in ref.Sums.ARRAYS:
            for i, v in getattr(w, name).items():
                getattr(total, name)[i] += times * v
        for e, v in w.conn_log.items():
            total.conn_log[e] += times * v
    stream = torch.cuda.Stream()
    block = Block(tables, sum(total.conn_log.values()) + 16)
    for case, want in ((tables, want_tables), (middle, want_middle), (tables, want_tables)):
        device_score(case, want, block=block, stream=stream)
    assert sc.differences(tables, total, block.got()) == []


def test_no_items_is_ok_and_writes_nothing():
    (case,), (want,) = sc.cases("single"), sc.expected("single")
    block = device_score(case, want, n_items=0)
    assert np.array_equal(block.dev.cpu().numpy(), block.clean)


def test_the_connection_log_at_its_capacity():
    case, want = sc.cases("connections")[1], sc.expected("connections")[1]
    total = sum(want.conn_log.values())
    assert total > 100 and not case.near
    for cap in (total, total - 1, 0):
        assert sc.differences(case, want, device_score(case, want, conn_cap=cap).got(), conn_cap=cap) == [], cap
