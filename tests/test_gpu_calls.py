"""gtx_calls_batch on the device over hand-made accumulators: every case set of tests/calls_cases.py against the plain restatement
(tests/calls_ref.py) field by field and against the oracle through harness.canonical_calls; d_phred and d_calls inside larger
buffers whose bytes in front and behind stay as they were; the accumulators bit-identical afterwards; two calls in a row, a stream
of the caller's, no samples at all; and once a state in which the reference itself reaches a clamp (the pooled tail).  All values
are integers; there is no tolerance.  The same sets on the host: test_calls_emu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import calls_cases as cc
import harness
from graphtyper_amd import lib as gtx
from test_calls_emu import pooled_tail_case

pytestmark = pytest.mark.gpu
GUARD = 4096  # bytes in front of and behind each output, filled with 0xA5


@functools.lru_cache(maxsize=None)
def device_ctx(key):
    return gtx.Context(cc.graph(key), device=0)


def device_calls(case, n_samples=None, launches=1, stream=None):
    """-> (phred, calls) of gtx_calls_batch over the case's arrays; checks what every call has to keep: the guards, `reserved`, the
    accumulators"""
    import torch
    ctx = device_ctx(case.key)
    n_samples = case.n_samples if n_samples is None else n_samples
    n_phred, n_calls = n_samples * ctx.total_tri, n_samples * ctx.n_hap * gtx.SAMPLE_CALL.itemsize
    host = [case.log_score, case.gt_cov, case.hap_u32]
    devs = [torch.from_numpy(a.view(np.uint8)).to("cuda:0") for a in host]
    d_phred = torch.full((GUARD + n_phred + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_calls = torch.full((GUARD + n_calls + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    buf = gtx.ScoreBuffers(n_samples, *[d.data_ptr() for d in devs], None, None, None, None, 0, None, None, 0)
    torch.cuda.synchronize()
    for _ in range(launches):
        gtx.check(gtx.lib().gtx_calls_batch(ctx.h, C.byref(buf), d_phred.data_ptr() + GUARD, d_calls.data_ptr() + GUARD,
                                            None if stream is None else C.c_void_p(stream.cuda_stream)))
    torch.cuda.synchronize()
    phred, calls = d_phred.cpu().numpy(), d_calls.cpu().numpy()
    for out, n in ((phred, n_phred), (calls, n_calls)):
        assert (out[:GUARD] == 0xA5).all() and (out[GUARD + n:] == 0xA5).all(), "a byte outside the output was written"
    for a, d in zip(host, devs):
        assert np.array_equal(a.view(np.uint8), d.cpu().numpy()), "an accumulator was written"
    calls = calls[GUARD:GUARD + n_calls].view(gtx.SAMPLE_CALL)
    assert not calls["reserved"].any()
    return phred[GUARD:GUARD + n_phred], calls


@pytest.mark.parametrize("name", cc.SETS)
def test_every_field_equals_the_restatement_and_the_oracle(name):
    for k, (case, want) in enumerate(zip(cc.cases(name), cc.expected(name))):
        got = device_calls(case)
        assert cc.differences(case, want, got) == [], k
        if name in cc.SANITIZED:  # (many_cells: the device against the restatement only)
            assert np.array_equal(cc.canonical(case, *got), cc.oracle_calls(case)), k


def test_the_sets_on_the_device_are_the_sets_of_the_host_tests():
    assert "many_cells" in cc.SETS and cc.cases("many_cells")[0].cells() >= 40003 and len(cc.SETS) == 8


def test_two_calls_in_a_row_and_a_stream_of_the_callers_give_one_result():
    import torch
    stream = torch.cuda.Stream()
    for case, want in zip(cc.cases("random") + cc.cases("layout"), cc.expected("random") + cc.expected("layout")):
        for kw in (dict(launches=2), dict(stream=stream), dict(launches=2, stream=stream)):
            assert cc.differences(case, want, device_calls(case, **kw)) == [], kw


def test_no_samples_is_ok_and_writes_nothing():
    (case,) = cc.cases("ties")
    phred, calls = device_calls(case, n_samples=0)  # (GTX_OK, and every byte of both buffers is a guard byte)
    assert len(phred) == 0 and len(calls) == 0


def test_the_pooled_tail_on_the_device():
    pooled_tail_case(harness.GpuBackend)
