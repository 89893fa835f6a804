"""The C-ABI library loads without a GPU and exports every symbol include/gtx.h declares."""
import os
import re

from graphtyper_amd import lib as gtx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_match_header():
    gtx.build()
    L = gtx.lib()
    header = open(os.path.join(ROOT, "include", "gtx.h")).read()
    declared = set(re.findall(r"\b(gtx_[a-z0-9_]+)\s*\(", header))
    assert declared == set(gtx.EXPORTS), declared ^ set(gtx.EXPORTS)
    for name in declared:
        assert hasattr(L, name), name


def test_strerror():
    L = gtx.lib()
    assert L.gtx_strerror(0) == b"ok"
    assert b"no HIP device" in L.gtx_strerror(2)


def test_binding_declares_argument_types_for_every_entry_point():
    """ctypes passes an undeclared Python int as a 32-bit C int: a device pointer would be truncated"""
    L = gtx.lib()
    missing = [n for n in gtx.EXPORTS if getattr(L, n).argtypes is None and n not in ("gtx_last_error",)]
    assert missing == []


def test_header_is_plain_c(tmp_path):
    """the boundary is a C ABI: include/gtx.h has to compile as C99 (no C++ types in the signatures) and link against
    the library"""
    import subprocess
    src = tmp_path / "use_gtx.c"
    src.write_text('#include "gtx.h"\nint main(void) { gtx_params p; gtx_score_buffers b; (void)p; (void)b; '
                   'return gtx_strerror(0) == 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "use_gtx.o")])


def test_calls_batch_refuses_null_arguments_and_a_context_without_a_device():
    """gtx_calls_batch: each NULL argument and each NULL accumulator pointer is GTX_ERR_ARG, a device=-1 context GTX_ERR_NO_DEVICE --
    all of it decided before anything is launched, so no device is needed to see it"""
    import ctypes as C

    import numpy as np

    import calls_cases as cc
    L = gtx.lib()
    ctx = cc.host_ctx("shapes")
    ls, cov, cu = np.zeros(ctx.total_tri, np.uint32), np.zeros(ctx.total_allele, np.uint32), np.zeros(ctx.n_hap * 4, np.uint32)
    phred, calls = np.zeros(ctx.total_tri, np.uint8), np.zeros(ctx.n_hap, gtx.SAMPLE_CALL)
    ptrs = [a.ctypes.data for a in (ls, cov, cu)]

    def buffers(missing=None):
        return gtx.ScoreBuffers(1, *[None if k == missing else p for k, p in enumerate(ptrs)], None, None, None, None, 0, None, None, 0)

    args = [ctx.h, C.byref(buffers()), phred.ctypes.data, calls.ctypes.data]
    for k in range(4):
        assert L.gtx_calls_batch(*[None if j == k else a for j, a in enumerate(args)], None) == 1  # GTX_ERR_ARG
    for k in range(3):
        assert L.gtx_calls_batch(ctx.h, C.byref(buffers(missing=k)), phred.ctypes.data, calls.ctypes.data, None) == 1
    assert L.gtx_calls_batch(*args, None) == 2  # GTX_ERR_NO_DEVICE
    assert not phred.any() and not calls.view(np.uint8).any()
