"""The order in which a context gives its device memory back.  The library keeps freed blocks in a cache that hands them out
again at once, so a context may only let go of its blocks when nothing on the device can still use them: destroying a context
waits for the device itself, whatever its caller did or did not wait for.  One process, three steps: a context is destroyed
while its alignment and scoring calls are still queued on a non-default stream; a second context (whose blocks come back from
the cache) runs the same calls and must give the oracle's records, accumulators and calls; a context for reads of up to 1 000
bases, whose scratch owns the largest blocks, runs against the oracle once.  (No assertion on memory sizes: the card is shared.)"""
import ctypes as C

import numpy as np
import pytest

import harness
import scenarios
from graphtyper_amd import lib as gtx
from oracle_lib import Oracle
from test_gpu_pipeline_long_reads import RB, oracle_text, ragged_case, resident, write_bams

pytestmark = pytest.mark.gpu

N_SAMPLES = 2


def queue_calls(torch, backend, stream, a_seq, a_meta, items):
    """one gtx_align_batch and one gtx_score_batch on `stream`, not waited for -> what the calls use and write (device tensors,
    the host accumulators they belong to)"""
    L = gtx.lib()
    acc = harness.Accumulators(backend.ctx, N_SAMPLES)
    with torch.cuda.stream(stream):
        d_seq, d_meta, d_items = backend._dev(a_seq), backend._dev(a_meta), backend._dev(items)
        devs = [backend._dev(a) for a in acc.arrays()]
        d_rec = torch.zeros(len(a_meta) * 2 * harness.REC_WORDS, dtype=torch.int32, device="cuda:0")
    buf = acc.buffers([d.data_ptr() for d in devs])
    s = C.c_void_p(stream.cuda_stream)
    gtx.check(L.gtx_align_batch(backend.ctx.h, d_seq.data_ptr(), a_seq.shape[1], d_meta.data_ptr(), len(a_meta), d_rec.data_ptr(), harness.REC_WORDS, s))
    gtx.check(L.gtx_score_batch(backend.ctx.h, d_items.data_ptr(), len(items), d_rec.data_ptr(), harness.REC_WORDS, C.byref(buf), s))
    return dict(keep=(d_seq, d_meta, d_items, buf), devs=devs, d_rec=d_rec, acc=acc)


def test_a_context_destroyed_behind_queued_calls_and_its_successors(tmp_path):
    import torch
    assert torch.cuda.is_available(), "this test needs the GPU"
    # the smallest scenario with a second pass: dense variation, more sites per read than the main passes' tables hold
    ref, recs, codes, pos = scenarios.synthetic_case("snp7", n_ref=30000, n_reads=500, region_begin=5000)
    order = np.argsort(pos, kind="stable")
    codes, rec = codes[order], scenarios.stream_records(len(codes), pos, sample=np.arange(len(codes)) % N_SAMPLES)[order]
    oracle = Oracle(ref, recs, region_begin=5000)
    og = oracle.genotyper(N_SAMPLES, 1)
    og.push(list(codes), flags=rec["flag"], tid=rec["tid"], mtid=rec["mtid"], pos=rec["pos"], isize=rec["isize"], mapq=rec["mapq"],
            score_diff=rec["score_diff"], name=rec["name_id"], sample=rec["sample"], rg=rec["rg"])
    graph = gtx.graph_from_records(ref, recs, region_begin=5000)
    stream = torch.cuda.Stream()

    first = harness.GpuBackend(graph)
    a_seq, a_meta, items = gtx.Stream(first.ctx.params, 1).push(rec, gtx.pack_nibbles(codes))
    queued = queue_calls(torch, first, stream, a_seq, a_meta, items)
    first.ctx.close()  # (the stream has not been waited for)
    del queued

    second = harness.GpuBackend(graph)
    queued = queue_calls(torch, second, stream, a_seq, a_meta, items)
    stream.synchronize()
    assert second.ctx.error_count() == 0
    records = queued["d_rec"].cpu().numpy().view(np.uint32)
    status = records.reshape(-1, harness.REC_WORDS)[:, 0] >> 16
    assert not (status & gtx.ST_ERROR_MASK).any(), "kernel table overflow"
    _, tasks = second.big_records()
    assert tasks > 0 and (status & gtx.ST_EXTERNAL).any()  # (the second pass ran, and results live in the arena)
    acc = queued["acc"]
    for host, dev in zip(acc.arrays(), queued["devs"]):
        host[...] = dev.cpu().numpy().view(host.dtype)
    want_scores = og.scores()
    got_scores = harness.canonical_scores(second.ctx, acc)
    assert len(got_scores) == len(want_scores) and np.array_equal(got_scores, want_scores), "score streams differ"
    assert want_scores.sum() > 0
    # the records read for read (every read a task, as the parity tests align them), on the same stream
    seq, lens = harness.pack_ragged(list(codes))
    meta = harness.read_meta(lens)
    with torch.cuda.stream(stream):
        d_seq, d_meta = second._dev(seq), second._dev(meta)
        d_rec = torch.zeros(len(meta) * 2 * harness.REC_WORDS, dtype=torch.int32, device="cuda:0")
    gtx.check(gtx.lib().gtx_align_batch(second.ctx.h, d_seq.data_ptr(), seq.shape[1], d_meta.data_ptr(), len(meta), d_rec.data_ptr(), harness.REC_WORDS,
                                        C.c_void_p(stream.cuda_stream)))
    stream.synchronize()
    got = gtx.parse_records(d_rec.cpu().numpy().view(np.uint32), len(meta), harness.REC_WORDS, second.ctx.hap_order, second.big_records()[0])
    want = oracle.align(list(codes))
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        for o in range(2):
            assert a[o]["status"] == 0 and dict(longest=a[o]["longest"], paths=a[o]["paths"]) == b[o], "read %d orientation %d" % (i, o)
    phred, calls = second.calls(acc, N_SAMPLES)
    got_calls, want_calls = harness.canonical_calls(second.ctx, phred, calls, N_SAMPLES), og.calls()
    assert len(got_calls) == len(want_calls) and np.array_equal(got_calls, want_calls), "sample calls differ"
    second.ctx.close()

    # max_read_len = 1 000: the scratch owns the long reads' workspaces and queues, the largest blocks a scratch has
    ref, recs, codes, rec = ragged_case([150, 250, 400, 1000], 300, seed=10)
    paths = write_bams(tmp_path, rec, codes)
    want = oracle_text(ref, recs, paths)
    assert want.count(b"\t0/1:") > 0
    ctx = gtx.Context(gtx.graph_from_records(ref, recs, region_begin=RB), device=0, max_read_len=1000)
    _, text = resident(ctx, paths, 512)
    assert text == want
    assert ctx.long_pass_tasks()[0] > 0
    ctx.close()
