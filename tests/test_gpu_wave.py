"""The hardware side of the wave policy (graphtyper_amd/csrc/wave_hip.hpp: WaveHip) held to the policy's contract (graph_dev.hpp: the
table): gtx_wave_probe runs the probe's text (wave_probe.hpp), a wavefront per set and four to a workgroup, and every word must be
the plain statement's of tests/wave_probe_cases.py.  The sequential side, same sets, same statement: test_wave_seq.py."""
import numpy as np
import pytest

import wave_probe_cases as wc
from graphtyper_amd import lib as gtx

pytestmark = pytest.mark.gpu


GTX_OK, GTX_ERR_ARG, GTX_ERR_NO_DEVICE = 0, 1, 2


def probe(device, words, n, out):
    return gtx.lib().gtx_wave_probe(device, gtx._p(words), n, gtx._p(out))


@pytest.mark.parametrize("n", wc.COUNTS)
def test_the_hardware_wave_equals_the_definition(n):
    words, out = wc.case_words(n), np.full(n * wc.OUT["WORDS"], 0xA5A5A5A5, dtype=np.uint32)
    assert probe(0, words, n, out) == GTX_OK, gtx.lib().gtx_last_error()
    assert wc.differences(n, out) == []


def test_the_argument_errors():
    words, out = wc.case_words(1), np.full(wc.OUT["WORDS"], 0xA5A5A5A5, dtype=np.uint32)
    assert probe(0, None, 1, out) == GTX_ERR_ARG and probe(0, words, 1, None) == GTX_ERR_ARG
    assert probe(-1, words, 1, out) == GTX_ERR_NO_DEVICE
    assert probe(0, words, 0, out) == GTX_OK and probe(0, None, 0, None) == GTX_OK
    assert (out == 0xA5A5A5A5).all()
