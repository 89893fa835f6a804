"""The device entry points of discovery's first pass (include/gtx.h: gtx_disc_first_pass_device,
gtx_disc_first_pass_haplotypes_device) as far as a machine without a GPU can hold them: the symbols, their refusal of an object
that was made for the host stages only, their argument checks.  What they compute is held to the oracle in
tests/test_gpu_discovery_device.py; the accumulation step they share with the host stage (csrc/gtx_disc_support.hpp) is held by
the host stage's own tests in tests/test_discovery.py."""
import ctypes as C
import os

import numpy as np

from graphtyper_amd import lib as gtx
from oracle_lib import _p

NAMES = ["gtx_disc_first_pass_device", "gtx_disc_first_pass_haplotypes_device"]


def test_both_symbols_are_exported_and_declared():
    L = gtx.lib()
    header = open(os.path.join(os.path.dirname(os.path.abspath(gtx.__file__)), "..", "include", "gtx.h")).read()
    for name in NAMES:
        assert name in gtx.EXPORTS and hasattr(L, name) and ("int %s(" % name) in header


def test_an_object_without_a_device_is_refused():
    L = gtx.lib()
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGTACGT", 8, 0, -1, C.byref(h)))
    d = np.zeros(64, np.uint32)
    words, n = np.zeros(16, np.uint32), C.c_uint64(7)
    assert L.gtx_disc_first_pass_device(h, _p(d), 16, _p(d), _p(d), _p(d), 1, _p(d), _p(d), 50, _p(words), len(words), C.byref(n), None) == 2  # GTX_ERR_NO_DEVICE
    assert L.gtx_disc_first_pass_haplotypes_device(h, _p(d), 16, _p(d), _p(d), _p(d), 1, _p(d), _p(d), 50, 3, _p(words), len(words), C.byref(n), None) == 2
    assert b"without a device" in L.gtx_last_error()
    # ... and the helper of the binding raises it
    try:
        gtx.disc_first_pass_device(h, _p(d), 16, _p(d), _p(d), _p(d), 1, _p(d), _p(d))
        raise AssertionError("no error")
    except gtx.GtxError as e:
        assert e.status == 2
    L.gtx_disc_destroy(h)


def test_bad_arguments_are_refused_before_anything_is_touched():
    L = gtx.lib()
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGTACGT", 8, 0, -1, C.byref(h)))
    d = np.zeros(64, np.uint32)
    words, n = np.zeros(16, np.uint32), C.c_uint64()
    call = lambda *a: L.gtx_disc_first_pass_device(*a)  # noqa: E731
    good = [h, _p(d), 16, _p(d), _p(d), _p(d), 1, _p(d), _p(d), 50, _p(words), len(words), C.byref(n), None]
    for at, bad in [(0, None), (2, 0), (2, 24), (8, None), (9, 0), (10, None), (12, None), (3, None)]:
        args = list(good)
        args[at] = bad
        assert call(*args) == 1, at  # GTX_ERR_ARG
    L.gtx_disc_destroy(h)


def test_the_events_batch_checks_its_arguments_before_it_asks_for_the_device():
    """gtx_disc_events_batch: GTX_ERR_ARG is decided before the device is asked for, so an object made for device -1 still gets it for a
    plane_stride of 0 or of no whole plane groups, for misaligned planes and for a null array with n_reads > 0; with all arguments
    right and no reads the answer is the no-device status"""
    L = gtx.lib()
    h = C.c_void_p()
    gtx.check(L.gtx_disc_create(b"ACGTACGT", 8, 0, -1, C.byref(h)))
    d = np.zeros(64, np.uint32)
    at = d.ctypes.data
    assert at % 4 == 0
    good = [h, at, 16, at, 32, at, at, 1, at, 4, at, at, None]  # planes, stride, qual, stride, reads, cigar, n_reads, events, cap, counts, read_out, stream
    bad = [(2, 0), (2, 8), (2, 24), (1, at + 1), (1, at + 2), (0, None)] + [(k, None) for k in (1, 3, 5, 6, 8, 10, 11)]
    for k, value in bad:
        args = list(good)
        args[k] = value
        assert L.gtx_disc_events_batch(*args) == 1, (k, value)  # GTX_ERR_ARG
        assert b"gtx_disc_events_batch: bad argument" in L.gtx_last_error()
    for n_reads in (1, 0):
        args = list(good)
        args[7] = n_reads
        assert L.gtx_disc_events_batch(*args) == 2  # GTX_ERR_NO_DEVICE
    none = [h, None, 16, None, 0, None, None, 0, None, 0, None, None, None]  # no reads: no array is needed
    assert L.gtx_disc_events_batch(*none) == 2
    args = list(good)
    args[8], args[9] = None, 0  # no event buffer for an event_cap of 0 is no bad argument
    assert L.gtx_disc_events_batch(*args) == 2
    L.gtx_disc_destroy(h)
