"""gtx_scores_replay, _compact, _log and _apply on the device over hand-made item orders (tests/replay_cases.py): every set through
gtx_score_batch and then the replay, against the restatement (score_ref.replay) and the oracle's guarded explain_to_score -- the log as
a sorted list of tuples, the replayed heads and rows, gtx_calls_batch on the replayed block.  All accumulators lie in ONE device block
with 4 096 bytes of 0xA5 around each: after the replay the block is, byte for byte, the block before it with nothing but the head
word and the triangle row of the replayed cells set to the restatement's values.  All values are integers; there is no tolerance.
The same sets on the host: test_replay_emu.py; the two witnesses against each other: test_replay_ref.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import harness
import replay_cases as rc
import score_cases as sc
import score_ref as ref
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu
GUARD_BYTES = 4096
ARRAYS = (("log_score", np.uint32), ("gt_cov", np.uint32), ("hap_u32", np.uint32), ("stat_u64", np.uint64), ("stat_u32", np.uint32),
          ("conn_near", np.uint32), ("conn_log", np.uint32), ("conn_count", np.uint32))
ERR_ARG, ERR_CAPACITY = 1, 5


@functools.lru_cache(maxsize=None)
def device_ctx(params=()):
    return gtx.Context(sc.graph(), device=0, **dict(params))


def ctx_on_device(case):
    return case.ctx if isinstance(case, sc.Aligned) else device_ctx(case.params)


class Block:
    """the accumulators of one case in one device block, guard bytes around each"""

    def __init__(self, case, conn_cap, fill=None):
        import torch
        f = sc.facts_of(case)
        sizes = ref.Sums(f, case.n_samples).sizes()
        sizes.update(conn_log=conn_cap * 6, conn_count=2)
        self.case, self.conn_cap, self.spans, at = case, conn_cap, {}, GUARD_BYTES
        for name, dtype in ARRAYS:
            n = sizes[name] * np.dtype(dtype).itemsize
            self.spans[name] = (at, n)
            at += (n + 7) // 8 * 8 + GUARD_BYTES
        if fill is None:
            fill = np.full(at, 0xA5, np.uint8)
            for a, n in self.spans.values():
                fill[a:a + n] = 0
        self.dev = torch.from_numpy(fill.copy()).to("cuda:0")
        p = {name: self.dev.data_ptr() + a for name, (a, n) in self.spans.items()}
        self.buf = gtx.ScoreBuffers(case.n_samples, p["log_score"], p["gt_cov"], p["hap_u32"], p["stat_u64"], p["stat_u32"], p["conn_log"], p["conn_count"],
                                    conn_cap, p["conn_near"], None, 0)

    def host(self):
        return self.dev.cpu().numpy()

    def view(self, host, name):
        a, n = self.spans[name]
        return host[a:a + n].view(dict(ARRAYS)[name])

    def got(self, host):
        arrays = {name: self.view(host, name).copy() for name, _ in ARRAYS}
        arrays["conn_log"] = arrays["conn_log"].reshape(-1, 6)
        return sc.Got(**arrays)

    def accumulators(self, host, ctx):
        acc = harness.Accumulators(ctx, self.case.n_samples, conn_cap=self.conn_cap)
        for a, name in zip(acc.arrays(), ("log_score", "gt_cov", "hap_u32", "stat_u64", "stat_u32", "conn_log", "conn_count", "conn_near")):
            a[:] = self.view(host, name)
        return acc

    def replayed(self, host, r):
        """`host` with the head word and the row of every replayed cell set to the restatement's: what the block has to be afterwards"""
        f = sc.facts_of(self.case)
        want = host.copy()
        heads, rows = self.view(want, "hap_u32"), self.view(want, "log_score")
        for cell, row in r.rows.items():
            sample, site = divmod(cell, f.n_hap)
            heads[4 * cell] = r.head[cell] | 0x80000000
            base = sample * f.total_tri + f.tri_off[site]
            rows[base:base + len(row)] = row
        return want


class Run:
    """one case on the device: its inputs uploaded, gtx_score_batch done and held to the unguarded sums"""

    def __init__(self, case, s, stream=None, items=None):
        import torch
        self.torch, self.case, self.s = torch, case, s
        self.ctx = ctx_on_device(case)
        self.compact = bool(case.compact_reads)
        self.items = case.all_items if items is None else items
        self.inputs = dict(items=self.items, records=case.records_beside_compact if self.compact else case.records)
        if self.compact:
            self.inputs.update(side=case.side, compact=case.compact)
        self.dev = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).reshape(-1).copy()).to("cuda:0") for k, v in self.inputs.items()}
        self.p = {k: d.data_ptr() for k, d in self.dev.items()}
        self.st = None if stream is None else C.c_void_p(stream.cuda_stream)
        self.block = Block(case, rc.conn_cap_of(s))
        L, p = gtx.lib(), self.p
        torch.cuda.synchronize()
        if self.compact:
            gtx.check(L.gtx_score_batch_compact(self.ctx.h, p["items"], None, len(self.items), p["records"], case.rec_words, p["compact"], p["side"],
                                                C.byref(self.block.buf), self.st))
        else:
            gtx.check(L.gtx_score_batch(self.ctx.h, p["items"], len(self.items), p["records"], case.rec_words, C.byref(self.block.buf), self.st))
        torch.cuda.synchronize()
        self.before = self.block.host()

    def log(self, block=None, first=0, count=None, item_base=0, cap=None, with_compact=None):
        """gtx_scores_replay_log over items [first, first + count) -> (status, entries, n, n_unsupported)"""
        count = len(self.items) - first if count is None else count
        with_compact = self.compact if with_compact is None else with_compact
        out = np.zeros(max(cap if cap is not None else 1 << 21, 1), gtx.REPLAY_ENTRY)
        n, bad = C.c_uint64(), C.c_uint64()
        rc_ = gtx.lib().gtx_scores_replay_log(self.ctx.h, self.p["items"] + 40 * first, count, self.p["records"], self.case.rec_words,
                                              self.p["compact"] if with_compact else None, self.p["side"] if with_compact else None,
                                              C.byref((block or self.block).buf), item_base, self.st,
                                              None if cap == 0 else out.ctypes.data_as(C.c_void_p), len(out) if cap is None else cap, C.byref(n), C.byref(bad))
        return rc_, out[:min(n.value, len(out))].copy(), int(n.value), int(bad.value)

    def replay(self, block=None, items=None):
        """gtx_scores_replay (_compact where the case has compact reads) -> (n_replayed, n_unsupported).  items: other than the run's"""
        n, bad = C.c_uint64(), C.c_uint64()
        L, p, buf = gtx.lib(), dict(self.p), C.byref((block or self.block).buf)
        if items is not None:
            d_items = self.torch.from_numpy(np.ascontiguousarray(items).view(np.uint8).reshape(-1).copy()).to("cuda:0")
            p["items"] = d_items.data_ptr()
        n_items = len(self.items if items is None else items)
        if self.compact:
            gtx.check(L.gtx_scores_replay_compact(self.ctx.h, p["items"], n_items, p["records"], self.case.rec_words, p["compact"], p["side"], buf,
                                                  self.st, C.byref(n), C.byref(bad)))
        else:
            gtx.check(L.gtx_scores_replay(self.ctx.h, p["items"], n_items, p["records"], self.case.rec_words, buf, self.st, C.byref(n), C.byref(bad)))
        self.torch.cuda.synchronize()
        return int(n.value), int(bad.value)

    def apply(self, block, entries):
        n = C.c_uint64()
        entries = np.ascontiguousarray(entries, gtx.REPLAY_ENTRY)
        rc_ = gtx.lib().gtx_scores_replay_apply(self.ctx.h, C.byref(block.buf), entries.ctypes.data_as(C.c_void_p), len(entries), self.st, C.byref(n))
        self.torch.cuda.synchronize()
        return rc_, int(n.value)

    def fresh(self):
        """another block with the bytes this one had after gtx_score_batch"""
        return Block(self.case, self.block.conn_cap, fill=self.before)

    def calls(self, block):
        torch, case = self.torch, self.case
        f = sc.facts_of(case)
        d_phred = torch.zeros(max(case.n_samples * f.total_tri, 1), dtype=torch.uint8, device="cuda:0")
        d_calls = torch.zeros(max(case.n_samples * f.n_hap, 1) * gtx.SAMPLE_CALL.itemsize, dtype=torch.uint8, device="cuda:0")
        gtx.check(gtx.lib().gtx_calls_batch(self.ctx.h, C.byref(block.buf), d_phred.data_ptr(), d_calls.data_ptr(), self.st))
        torch.cuda.synchronize()
        host_ctx = sc.ctx_of(case)
        return harness.canonical_calls(host_ctx, d_phred.cpu().numpy(), d_calls.cpu().numpy().view(gtx.SAMPLE_CALL), case.n_samples)

    def inputs_are_untouched(self):
        for k, v in self.inputs.items():
            assert np.array_equal(np.ascontiguousarray(v).view(np.uint8).reshape(-1), self.dev[k].cpu().numpy()), "a call wrote its input: " + k


def whole_case(case, s, r, oracle, stream=None):
    """score, log, replay, calls of one case, every check the issue lists -> the block's bytes afterwards"""
    run = Run(case, s, stream=stream)
    block = run.block
    assert sc.differences(case, s, block.got(run.before)) == [], "gtx_score_batch: the unguarded sums"
    status, entries, n, bad = run.log()
    assert status == 0 and n == len(r.log) and bad == len(r.unsupported)
    assert rc.log_tuples(entries) == sorted(r.log)
    assert np.array_equal(block.host(), run.before), "gtx_scores_replay_log wrote to the block"
    assert run.replay() == (len(r.marked), len(r.unsupported))
    after = block.host()
    want = block.replayed(run.before, r)
    bad_at = np.nonzero(after != want)[0]
    assert len(bad_at) == 0, "the block differs from the replayed one at bytes %s" % bad_at[:10]
    run.inputs_are_untouched()
    assert run.ctx.error_count() == 0
    if oracle is not None:
        scores, calls = oracle
        got = harness.canonical_scores(sc.ctx_of(case), block.accumulators(after, sc.ctx_of(case)))
        assert len(got) == len(scores) and np.array_equal(got, scores), "the oracle's scores"
        assert np.array_equal(run.calls(block), calls), "the oracle's calls"
    return run, after


@pytest.mark.parametrize("name,k", [ck for ck in rc.CASE_IDS if ck[0] != "halves"])
def test_log_rows_and_calls_equal_both_witnesses(name, k):
    case, (s, r) = rc.cases(name)[k], rc.expected(name)[k]
    whole_case(case, s, r, rc.oracle_of(name, k))


def test_the_log_in_two_halves_and_the_edges_of_the_interface():
    """on a stream of the caller's"""
    import torch
    (case,), ((s, r),) = rc.cases("halves"), rc.expected("halves")
    stream = torch.cuda.Stream()
    run, after = whole_case(case, s, r, rc.oracle_of("halves", 0), stream=stream)
    assert run.replay() == (0, 0) and np.array_equal(run.block.host(), after)  # (a replayed cell is marked and left alone)
    n_items = len(case.all_items)
    want_log = sorted(r.log)
    rng = np.random.default_rng(11)
    for cut in (0, 1, n_items * 2 // 5, n_items):
        block = run.fresh()
        parts = []
        for first, count in ((0, cut), (cut, n_items - cut)):
            status, entries, n, bad = run.log(block, first, count, item_base=first)
            assert status == 0 and bad == 0 and n == len(entries)
            parts.append(entries)
        assert rc.log_tuples(np.concatenate(parts)) == want_log, cut
        for order in (parts, parts[::-1]):
            block = run.fresh()
            entries = np.concatenate(order)
            rng.shuffle(entries)
            assert run.apply(block, entries) == (0, len(r.marked))
            assert np.array_equal(block.host(), after), cut
    block = run.fresh()
    total = len(want_log)
    assert run.log(block, cap=total - 1)[::2] == (ERR_CAPACITY, total)
    assert run.log(block, cap=0)[::2] == (ERR_CAPACITY, total)
    status, entries, n, bad = run.log(block, cap=total)
    assert status == 0 and n == total
    assert np.array_equal(block.host(), run.before)
    beyond = entries[:3].copy()
    beyond["cell"][1] = case.n_samples * sc.facts().n_hap
    assert run.apply(block, beyond) == (ERR_ARG, 0) and np.array_equal(block.host(), run.before)
    assert run.ctx.error_count() == 0


def test_a_marked_cell_that_no_item_touches_keeps_its_sum_and_gets_no_mark():
    """gtx_scores_replay over the items that leave one cell at the guard without a call: n_replayed is one less than the marked cells,
    the block is byte for byte the one before with the OTHER cells replayed -- that cell's head word and row as they were, no mark --,
    gtx_scores_finalize reports 1, and a later replay with all items replays that cell alone"""
    case, s, r, cell, keep, partial = rc.untouched_case()
    run = Run(case, s)
    block = run.block
    ctx = sc.ctx_of(case)
    assert rc.finalize_count(block.accumulators(run.before, ctx)) == len(r.marked)
    assert run.replay(items=case.all_items[keep]) == (len(r.marked) - 1, 0)
    after = block.host()
    assert np.array_equal(after, block.replayed(run.before, partial))
    assert int(block.view(after, "hap_u32")[4 * cell]) == s.hap_u32[4 * cell] >= rc.GUARD
    assert rc.finalize_count(block.accumulators(after, ctx)) == 1
    assert run.replay() == (1, 0)
    last = block.host()
    assert np.array_equal(last, block.replayed(run.before, r)) and rc.finalize_count(block.accumulators(last, ctx)) == 0
    run.inputs_are_untouched()
    assert run.ctx.error_count() == 0


def test_two_runs_on_fresh_buffers_give_identical_bytes():
    (case,), ((s, r),) = rc.cases("order_within_item"), rc.expected("order_within_item")
    first = whole_case(case, s, r, None)[1]
    second = whole_case(case, s, r, None)[1]
    assert np.array_equal(first, second)


def test_the_aligners_records_in_the_arena_and_a_wide_graph():
    """records in the context's arena (rec_words 8); a graph with a 100-allele site, whose replay is the wide kernel's: the SNP's cell
    of sample 0 equals the oracle, the 100-allele site's cell of sample 1 is counted as unsupported, left bit-identical, reported by
    gtx_scores_finalize and refused by gtx_scores_replay_apply.  That cell is the one thing left out of the comparison with the oracle."""
    sets = rc.aligned_replay(harness.GpuBackend)
    exp = rc.expected_aligned(sets)
    rc.facts_aligned(sets, exp)  # (the device's own records have to reach what the set is for)
    for a, (s, r) in zip(sets, exp):
        run, after = whole_case(a, s, r, None)
        acc = run.block.accumulators(after, a.ctx)
        if a.name == "wide":
            assert len(r.unsupported) == 1 and r.unsupported == {a.big_cell}
            nsat = C.c_uint64()
            copy = [x.copy() for x in (acc.log_score, acc.gt_cov, acc.hap_u32)]
            gtx.check(gtx.lib().gtx_scores_finalize(harness._p(copy[0]), len(copy[0]), harness._p(copy[1]), len(copy[1]), harness._p(copy[2]), len(copy[2]) // 4,
                                                    C.byref(nsat)))
            assert nsat.value == 1
            entry = np.zeros(1, gtx.REPLAY_ENTRY)
            entry["cell"], entry["order_eps"], entry["mask_lo"] = a.big_cell, 8, 1
            assert run.apply(run.block, entry) == (ERR_ARG, 0) and np.array_equal(run.block.host(), after)
            rc.reference_arrays_wide(a, acc, r)
        scores, calls = rc.oracle_streams(a, a.all_items)
        got = harness.canonical_scores(a.ctx, acc)
        assert len(got) == len(scores) and np.array_equal(got, scores), a.name
        phred, sample_calls = a.b.calls(acc, a.n_samples)
        assert np.array_equal(harness.canonical_calls(a.ctx, phred, sample_calls, a.n_samples), calls), a.name
