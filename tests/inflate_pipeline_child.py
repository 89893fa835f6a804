"""One gtx_pipeline_run in a process of its own, for test_gpu_bgzf_inflate.py (GTX_BGZF_DEVICE is read from the environment
by the library): python inflate_pipeline_child.py out.npz threads n_pairs file.bam ...  The graph is that of
test_gpu_pipeline_long_reads.test_2x250_pairs_on_a_default_context; `inflate` in the output: gtx_reads_inflate_counts of the process."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

import harness  # noqa: E402
import scenarios  # noqa: E402
from graphtyper_amd import lib as gtx  # noqa: E402
from test_gpu_pipeline_long_reads import RB, accumulators  # noqa: E402


def main(out, threads, n_pairs, paths):
    ref, recs, codes, rec = scenarios.paired_case("snp100", n_ref=12000, n_pairs=n_pairs, region_begin=RB, read_len=250, n_samples=2)
    ctx = gtx.Context(gtx.graph_from_records(ref, recs, region_begin=RB), device=0)
    L = gtx.lib()
    buf = gtx.ScoreBuffers()
    gtx.check(L.gtx_scores_alloc(ctx.h, 2, 1 << 22, C.byref(buf), None))
    st = gtx.pipeline_run(ctx, paths, threads, buf, harness.REC_WORDS, len(rec), chunk=4096, region="chr7")
    cov, s64, s32 = accumulators(ctx, buf)
    np.savez(out, counts=np.array([st["records"], st["tasks"], st["items"], st["records_failed"]], np.uint64), cov=cov, s64=s64, s32=s32,
             inflate=np.array(gtx.reads_inflate_counts(), np.uint64))
    L.gtx_scores_free(ctx.h, C.byref(buf))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4:])
