"""ctypes binding of libgtx.so (C ABI in include/gtx.h) + helpers that build the SoA graph view from variant records.

PyTorch is used by callers only for device memory, streams and torch.distributed; everything that touches reads runs
inside libgtx's HIP kernels.  There is no CPU path: without the built library or without a GPU the calls fail loudly.
"""
import ctypes as C
import os
import sys
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.path.join(HERE, os.environ.get("GTX_LIB", "libgtx.so"))  # GTX_LIB=libgtx_prof.so selects the phase-timing build
INVALID_ID = 0xFFFFFFFF
SPECIAL_START = 0xD0000000

ST_LABEL_OVERFLOW, ST_PATH_OVERFLOW, ST_DFS_OVERFLOW, ST_RECORD_OVERFLOW, ST_EXTERNAL = 1, 2, 4, 8, 16
ST_ERROR_MASK = 15

# names every build of libgtx.so must export (checked by tests/test_abi.py against include/gtx.h)
EXPORTS = ["gtx_strerror", "gtx_last_error", "gtx_ctx_create", "gtx_ctx_destroy", "gtx_ctx_special_positions",
           "gtx_ctx_score_layout", "gtx_ctx_haplotypes", "gtx_ctx_near_pairs", "gtx_index_stats", "gtx_index_get", "gtx_index_dump", "gtx_ctx_hint_table",
           "gtx_align_batch", "gtx_score_batch", "gtx_calls_batch", "gtx_ctx_big_records", "gtx_ctx_big_records_rewind", "gtx_ctx_exact_pass_tasks", "gtx_ctx_long_pass_tasks", "gtx_graph_sv_table", "gtx_ctx_pass_times", "gtx_ctx_error_count", "gtx_ctx_profile", "gtx_ctx_profile_log", "gtx_records_failed", "gtx_vcf_sites", "gtx_vcf_records_final", "gtx_align_batch_planes_compact", "gtx_score_batch_compact", "gtx_align_batch_planes_triaged", "gtx_score_batch_queued", "gtx_scores_replay_compact", "gtx_scores_replay_log", "gtx_scores_replay_apply", "gtx_scores_finalize", "gtx_phase_flags", "gtx_stream_create",
           "gtx_stream_destroy", "gtx_stream_push", "gtx_stream_set_coverage", "gtx_stream_finish", "gtx_stream_counts", "gtx_graph_build", "gtx_graph_from_files", "gtx_graph_get_view",
           "gtx_graph_destroy",
           "gtx_scores_alloc", "gtx_scores_zero", "gtx_scores_free", "gtx_scores_reduce", "gtx_comm_unique_id", "gtx_comm_init_rank",
           "gtx_comm_destroy", "gtx_ctx_kernel_times", "gtx_ref_depth_finalize", "gtx_vcf_records", "gtx_scores_replay", "gtx_reads_open", "gtx_reads_info",
           "gtx_reads_sample_name", "gtx_reads_next", "gtx_reads_close", "gtx_align_batch_flags", "gtx_score_batch_flags", "gtx_score_batch_words", "gtx_item_words",
           "gtx_pack_planes", "gtx_reads_to_planes", "gtx_align_batch_planes", "gtx_align_batch_planes_staged", "gtx_stream_set_planes", "gtx_device_cache_release",
           "gtx_disc_create", "gtx_disc_destroy", "gtx_disc_events_batch", "gtx_disc_first_pass", "gtx_vcf_header", "gtx_bgzf_compress",
           "gtx_shrink_params_default", "gtx_bam_shrink", "gtx_inflate_raw", "gtx_tabix_build", "gtx_tabix_start", "gtx_pipeline_run", "gtx_regions_run", "gtx_regions_free", "gtx_bam_shrink_multi", "gtx_disc_first_pass_haplotypes", "gtx_disc_merge",
           "gtx_pack_2bit", "gtx_stream_push_packed", "gtx_packed_to_planes", "gtx_align_batch_packed", "gtx_align_batch_packed_staged",
           "gtx_inflate_create", "gtx_inflate_destroy", "gtx_inflate_batch", "gtx_inflate_bgzf", "gtx_reads_set_inflate_device", "gtx_reads_inflate_counts",
           "gtx_disc_first_pass_device", "gtx_disc_first_pass_haplotypes_device",
           "gtx_disc_realign_batch", "gtx_disc_set_max_read_len", "gtx_disc_realign_wants", "gtx_disc_realign_target", "gtx_disc_realign_decide",
           "gtx_disc_indel_table", "gtx_disc_indel_table_upload", "gtx_disc_second_intake", "gtx_disc_second_plan", "gtx_disc_second_candidates",
           "gtx_disc_second_rounds", "gtx_disc_second_decide",
           "gtx_disc_variants", "gtx_disc_vcf_sites", "gtx_disc_second_file", "gtx_discover_params_default", "gtx_discover_region", "gtx_discover_destroy",
           "gtx_discover_text", "gtx_discover_variants", "gtx_discover_words", "gtx_discover_good", "gtx_discover_stats",
           "gtx_disc_bam_read", "gtx_disc_bam_destroy", "gtx_disc_bam_stream", "gtx_disc_bam_reads", "gtx_disc_bam_info", "gtx_disc_bam_unpack", "gtx_discover_files",
           "gtx_disc_bam_walk", "gtx_discover_files_front", "gtx_discover_front",
           "gtx_wave_probe",
           "gtx_dstream_create", "gtx_dstream_destroy", "gtx_dstream_push", "gtx_dstream_finish", "gtx_dstream_counts"]


class GraphView(C.Structure):
    _fields_ = [("n_ref", C.c_uint32), ("n_var", C.c_uint32),
                ("ref_order", C.c_void_p), ("ref_len", C.c_void_p), ("ref_dna_off", C.c_void_p), ("ref_nvar", C.c_void_p),
                ("ref_first_var", C.c_void_p), ("var_order", C.c_void_p), ("var_len", C.c_void_p),
                ("var_dna_off", C.c_void_p), ("var_out_ref", C.c_void_p), ("dna", C.c_void_p), ("dna_len", C.c_uint64),
                ("event_off", C.c_void_p), ("event_val", C.c_void_p)]


class PipelineStats(C.Structure):
    _fields_ = [("records", C.c_uint64), ("tasks", C.c_uint64), ("items", C.c_uint64), ("decode_s", C.c_double), ("push_s", C.c_double),
                ("enqueue_s", C.c_double), ("slowest_thread_s", C.c_double), ("loop_s", C.c_double), ("wall_s", C.c_double),
                ("n_samples", C.c_uint32), ("n_threads", C.c_uint32), ("records_failed", C.c_uint64), ("score_items_refused", C.c_uint64),
                ("connections_dropped", C.c_uint64)]


class RegionsStats(C.Structure):
    _fields_ = [("graph_build_s", C.c_double), ("ctx_create_s", C.c_double), ("device_s", C.c_double), ("vcf_text_s", C.c_double), ("wall_s", C.c_double),
                ("n_builders", C.c_uint32), ("n_device_threads", C.c_uint32), ("n_text_threads", C.c_uint32), ("reserved", C.c_uint32),
                ("records_failed", C.c_uint64), ("score_items_refused", C.c_uint64), ("connections_dropped", C.c_uint64)]


class ShrinkParams(C.Structure):
    _fields_ = [("max_frag_len", C.c_int32), ("min_num_matching", C.c_int32), ("filter_mapq0", C.c_int32), ("no_filter_on_coverage", C.c_int32),
                ("min_read_len", C.c_int32), ("min_read_len_low_mapq", C.c_int32), ("min_unpaired_read_len", C.c_int32), ("sam_flag_filter", C.c_int32),
                ("as_filter_threshold", C.c_int64), ("avg_cov_by_readlen", C.c_double), ("change_read_names", C.c_int32), ("compress_level", C.c_int32)]


class ShrinkStats(C.Structure):
    _fields_ = [("records_read", C.c_uint64), ("records_written", C.c_uint64), ("pairs_kept", C.c_uint64), ("singles_kept", C.c_uint64),
                ("dropped_by_depth", C.c_uint64)]


class Params(C.Structure):
    _fields_ = [("max_index_labels", C.c_int32), ("is_sv_graph", C.c_int32), ("hq_reads", C.c_int32),
                ("force_align_both_orientations", C.c_int32), ("is_segment_calling", C.c_int32),
                ("sam_flag_filter", C.c_int32), ("no_second_pass", C.c_int32), ("big_record_words", C.c_uint32),
                ("exact_pass_mb", C.c_uint32), ("max_read_len", C.c_uint32)]


class ScoreLayout(C.Structure):
    _fields_ = [("n_hap", C.c_uint32), ("total_tri", C.c_uint64), ("total_allele", C.c_uint64), ("total_near", C.c_uint64),
                ("ref_depth_len", C.c_uint32)]


class ScoreBuffers(C.Structure):
    _fields_ = [("n_samples", C.c_uint32), ("d_log_score", C.c_void_p), ("d_gt_cov", C.c_void_p), ("d_hap_u32", C.c_void_p),
                ("d_stat_u64", C.c_void_p), ("d_stat_u32", C.c_void_p), ("d_conn_log", C.c_void_p),
                ("d_conn_count", C.c_void_p), ("conn_cap", C.c_uint32), ("d_conn_near", C.c_void_p),
                ("d_ref_depth", C.c_void_p), ("ref_depth_len", C.c_uint32)]


READ_META = np.dtype([("l_qseq", np.uint16), ("flag", np.uint16), ("tid", np.int32), ("mtid", np.int32), ("isize", np.int32), ("pos", np.int32)],
                     align=True)
REC_META = np.dtype([("align_index", np.uint32), ("flag", np.uint16), ("mapq", np.uint8), ("score_diff", np.uint8),
                     ("pos", np.int32), ("isize", np.int32)], align=True)
SCORE_ITEM = np.dtype([("first", REC_META), ("second", REC_META), ("sample", np.uint32), ("kind", np.uint32)], align=True)
ITEM_LEFTOVER = 1
FLAG_FORWARD_ONLY = 0x8000
SAMPLE_CALL = np.dtype([("gt_first", np.uint16), ("gt_second", np.uint16), ("ref_total_depth", np.uint16),
                        ("alt_total_depth", np.uint16), ("gq", np.uint8), ("ambiguous_depth", np.uint8),
                        ("alt_proper_pair_depth", np.uint8), ("reserved", np.uint8)], align=True)
PHASE_ENTRY = np.dtype([("hap1", np.uint16), ("allele1", np.uint16), ("hap2", np.uint16), ("allele2", np.uint16),
                        ("flags", np.int8), ("reserved", np.uint8)], align=True)
STREAM_RECORD = np.dtype([("flag", np.uint16), ("mapq", np.uint8), ("score_diff", np.uint8), ("tid", np.int32),
                          ("mtid", np.int32), ("pos", np.int32), ("isize", np.int32), ("l_qseq", np.uint16),
                          ("rg", np.uint16), ("sample", np.uint32), ("name_id", np.uint64), ("mpos", np.int32),
                          ("n_cigar", np.uint32), ("cigar_front", np.uint32), ("cigar_back", np.uint32)], align=True)
DISC_READ = np.dtype([("pos", np.int32), ("flag", np.uint16), ("mapq", np.uint8), ("reserved", np.uint8), ("l_qseq", np.uint16),
                      ("n_cigar", np.uint16), ("cigar_off", np.uint32)], align=True)
DISC_EVENT = np.dtype([("read", np.uint32), ("pos", np.uint32), ("seq", np.uint32), ("len", np.uint16), ("type", np.uint8), ("hq", np.uint8),
                       ("max_distance", np.uint16), ("reserved", np.uint16)], align=True)
DISC_READ_OUT = np.dtype([("first_event", np.uint32), ("n_events", np.uint32), ("pos_end", np.int32), ("state", np.uint32)], align=True)
assert DISC_READ.itemsize == 16 and DISC_EVENT.itemsize == 20 and DISC_READ_OUT.itemsize == 16
LABEL = np.dtype([("start_index", np.uint32), ("end_index", np.uint32), ("variant_id", np.uint32)], align=True)
assert READ_META.itemsize == 20 and REC_META.itemsize == 16 and SCORE_ITEM.itemsize == 40 and STREAM_RECORD.itemsize == 56 \
    and SAMPLE_CALL.itemsize == 12


REALIGN_PAIR = np.dtype([("read", np.uint32), ("target", np.uint32)], align=True)
REALIGN_RESULT = np.dtype([("score", np.int32), ("clip_begin", np.uint16), ("clip_end", np.uint16), ("target_begin", np.uint16),
                           ("target_end", np.uint16), ("status", np.uint32)], align=True)
REALIGN_EVENT = np.dtype([("pos", np.uint32), ("len", np.uint16), ("type", np.uint8), ("reserved", np.uint8), ("seq_off", np.uint32)], align=True)
REALIGN_DECISION = np.dtype([("pos", np.int64), ("pos_end", np.int64), ("outcome", np.uint32), ("num_clipped_begin", np.uint32),
                             ("num_clipped_end", np.uint32), ("num_ins_begin", np.uint32)], align=True)
REALIGN_OK, REALIGN_BAD_PAIR, REALIGN_TOO_LONG = 0, 1, 2
MAX_READ, MAX_READ_LONG = 256, 1000  # GTX_MAX_READ, GTX_MAX_READ_LONG
REALIGN_MAX_TARGET, REALIGN_MAX_TARGET_LONG = 2048, 4095  # the aligner's windows: by default, after disc_set_max_read_len(handle, > 256)
# the second pass up to the aligner (gtx.h: gtx_disc_indel_table .. gtx_disc_second_candidates)
DISC_INDEL = np.dtype([("pos", np.uint32), ("len", np.uint32), ("seq_off", np.uint32), ("span", np.uint16), ("type", np.uint8), ("good", np.uint8),
                       ("file_index", np.int32)], align=True)
DISC_SECOND_READ = np.dtype([("pos", np.int32), ("pos_end", np.int32), ("score", np.int32), ("num_clipped_begin", np.int16), ("num_clipped_end", np.int16),
                             ("num_ins_begin", np.int16), ("flags", np.uint16), ("mapq", np.uint8), ("reserved", np.uint8), ("l_qseq", np.uint16),
                             ("bucket", np.uint32), ("first_event", np.uint32), ("n_events", np.uint32)], align=True)
DISC_SECOND_EVENT = np.dtype([("indel", np.uint32), ("read_pos", np.int32)], align=True)
DISC_SECOND_PAIR = np.dtype([("read", np.uint32), ("entry", np.uint32)], align=True)
assert DISC_INDEL.itemsize == 20 and DISC_SECOND_READ.itemsize == 36 and DISC_SECOND_EVENT.itemsize == 8 and DISC_SECOND_PAIR.itemsize == 8
DISC_NO_BUCKET = 0xFFFFFFFF
# the second pass from the aligner on (gtx.h: gtx_disc_second_rounds, gtx_disc_second_decide)
DISC_SECOND_SUPPORT = np.dtype([("hq_count", np.uint32), ("anti_count", np.uint32), ("multi_count", np.uint32), ("sequence_reversed", np.uint32),
                                ("proper_pairs", np.uint32), ("max_mapq", np.uint32)], align=True)
assert DISC_SECOND_SUPPORT.itemsize == 24


class DiscRoundsStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("pairs_aligned", C.c_uint64), ("pairs_refused", C.c_uint64), ("windows_built", C.c_uint64), ("rounds_done", C.c_uint32),
                ("rounds_skipped", C.c_uint32), ("compactions", C.c_uint32), ("events_wanted", C.c_uint32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}
REALIGN_NO_PADDING, REALIGN_BETTER, REALIGN_SAME_OVERLAPPING, REALIGN_SAME, REALIGN_WORSE = 0, 1, 2, 3, 4
# discovery to its end (gtx.h: gtx_disc_variants .. gtx_discover_region)
DISC_VARIANT = np.dtype([("pos", np.uint32), ("gt_id", np.uint32), ("ref_off", np.uint32), ("ref_len", np.uint32), ("alt_off", np.uint32), ("alt_len", np.uint32),
                         ("hap_off", np.uint32), ("n_hap", np.uint32), ("anti_off", np.uint32), ("n_anti", np.uint32), ("type", np.uint8), ("reserved", np.uint8, 3)],
                        align=True)
assert DISC_VARIANT.itemsize == 44


class DiscFile(C.Structure):
    _fields_ = [("planes", C.c_void_p), ("qual", C.c_void_p), ("reads", C.c_void_p), ("cigar", C.c_void_p), ("plane_stride", C.c_uint32),
                ("qual_stride", C.c_uint32), ("n_reads", C.c_uint32), ("n_cigar", C.c_uint32)]


class DiscoverParams(C.Structure):
    _fields_ = [("device", C.c_int32), ("bucket_size", C.c_uint32), ("max_read_len", C.c_uint32), ("n_threads", C.c_uint32), ("first_event_cap", C.c_uint32),
                ("second_event_cap", C.c_uint32)]


class DiscoverFileStats(C.Structure):
    _fields_ = [("events", C.c_uint64), ("events_passes", C.c_uint32), ("n_list", C.c_uint32), ("rounds", DiscRoundsStats)]


class DiscoverFrontStats(C.Structure):
    _fields_ = [("members", C.c_uint32), ("members_device", C.c_uint32), ("segments_hit", C.c_uint32), ("segments_rewalked", C.c_uint32), ("fell_back", C.c_uint32),
                ("reserved", C.c_uint32)]


class BamWalkOut(C.Structure):
    _fields_ = [("status", C.c_uint32), ("max_l_seq", C.c_uint32), ("bad_at", C.c_uint64), ("n_cigar", C.c_uint64), ("n_reads", C.c_uint32), ("segments_hit", C.c_uint32),
                ("segments_rewalked", C.c_uint32), ("reserved", C.c_uint32)]


BAM_WALK_OK, BAM_WALK_TRUNCATED, BAM_WALK_MALFORMED, BAM_WALK_LONG_READ = 0, 1, 2, 3


def build(force=False):
    """compile libgtx.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)"""
    src_dir = os.path.join(HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir) if not f.startswith("build")] + [os.path.join(ROOT, "include", "gtx.h")]
    if force or not os.path.exists(LIB_PATH) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs):
        subprocess.check_call(["make", "-C", src_dir, "-s", "-j", str(min(8, os.cpu_count() or 1))])
    return LIB_PATH


_lib = None


def lib():
    """the loaded library; raises if it has not been built (never falls back to anything else)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libgtx.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # A process that uses PyTorch as well has to have PyTorch's HIP runtime in it FIRST: libgtx.so names libamdhip64 by its
        # soname, and with torch already loaded that resolves to the runtime torch brought -- one runtime for both.  The other way
        # round the process holds two, and the library's own sees no device ("no HIP device visible").  Whoever binds the library
        # from Python gets the order right here; a C or C++ host has one runtime anyway.  GTX_NO_TORCH=1: a process that will never
        # use PyTorch (and does not want its two seconds of import) loads the library alone.
        if "torch" not in sys.modules and not os.environ.get("GTX_NO_TORCH"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        L.gtx_strerror.restype = C.c_char_p
        L.gtx_strerror.argtypes = [C.c_int]
        L.gtx_last_error.restype = C.c_char_p
        L.gtx_ctx_create.argtypes = [C.POINTER(GraphView), C.POINTER(Params), C.c_int, C.POINTER(C.c_void_p)]
        L.gtx_ctx_destroy.argtypes = [C.c_void_p]
        L.gtx_ctx_special_positions.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_uint32]
        L.gtx_ctx_score_layout.argtypes = [C.c_void_p, C.POINTER(ScoreLayout)]
        L.gtx_ctx_haplotypes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_index_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gtx_index_get.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.gtx_index_dump.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_ctx_hint_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_align_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                      C.c_void_p]
        L.gtx_score_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(ScoreBuffers),
                                      C.c_void_p]
        L.gtx_calls_batch.argtypes = [C.c_void_p, C.POINTER(ScoreBuffers), C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_ctx_big_records.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]
        L.gtx_ctx_big_records_rewind.argtypes = [C.c_void_p, C.c_void_p]
        L.gtx_ctx_exact_pass_tasks.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.gtx_ctx_long_pass_tasks.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.gtx_graph_sv_table.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_ctx_pass_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        L.gtx_ctx_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]
        L.gtx_ctx_error_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.gtx_ctx_profile.argtypes = [C.c_void_p, C.c_void_p]
        L.gtx_align_batch_planes_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_score_batch_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                              C.POINTER(ScoreBuffers), C.c_void_p]
        L.gtx_align_batch_planes_triaged.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_score_batch_queued.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(ScoreBuffers), C.c_void_p]
        L.gtx_scores_replay_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                C.POINTER(ScoreBuffers), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gtx_scores_replay_log.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(ScoreBuffers),
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gtx_scores_replay_apply.argtypes = [C.c_void_p, C.POINTER(ScoreBuffers), C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
        L.gtx_records_failed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
        L.gtx_ctx_profile_log.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_scores_finalize.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                          C.POINTER(C.c_uint64)]
        L.gtx_phase_flags.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64)]
        L.gtx_ctx_near_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_ref_depth_finalize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.gtx_vcf_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_vcf_records_final.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_vcf_sites.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_align_batch_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.gtx_disc_create.argtypes = [C.c_char_p, C.c_uint64, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]
        L.gtx_disc_destroy.argtypes = [C.c_void_p]
        L.gtx_disc_destroy.restype = None
        L.gtx_disc_events_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                            C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_disc_first_pass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                          C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_disc_first_pass_haplotypes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                                     C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_disc_merge.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_disc_first_pass_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        L.gtx_disc_first_pass_haplotypes_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                                            C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
        L.gtx_disc_realign_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                             C.c_uint32, C.c_void_p, C.c_void_p]
        L.gtx_disc_set_max_read_len.argtypes = [C.c_void_p, C.c_uint32]
        L.gtx_disc_realign_wants.argtypes = [C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, C.c_int64, C.c_uint32]
        L.gtx_disc_realign_target.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        L.gtx_disc_realign_decide.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
        L.gtx_disc_indel_table.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_disc_indel_table_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_disc_second_intake.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                             C.c_uint64] + [C.c_void_p] * 8
        L.gtx_disc_second_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.gtx_disc_second_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.gtx_disc_second_rounds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64,
                                             C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DiscRoundsStats), C.c_void_p]
        L.gtx_disc_second_decide.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.gtx_disc_variants.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_disc_vcf_sites.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_uint64,
                                         C.POINTER(C.c_uint64)]
        L.gtx_disc_second_file.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(DiscRoundsStats), C.c_void_p, C.c_void_p,
                                           C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p]
        L.gtx_discover_params_default.argtypes = [C.POINTER(DiscoverParams)]
        L.gtx_discover_params_default.restype = None
        L.gtx_discover_region.argtypes = [C.c_char_p, C.c_uint64, C.c_int64, C.c_char_p, C.POINTER(DiscFile), C.c_uint32, C.POINTER(DiscoverParams),
                                          C.POINTER(C.c_void_p)]
        L.gtx_discover_destroy.argtypes = [C.c_void_p]
        L.gtx_discover_destroy.restype = None
        L.gtx_discover_text.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.gtx_discover_text.restype = C.c_void_p
        L.gtx_discover_variants.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_uint64)]
        L.gtx_discover_variants.restype = C.c_void_p
        L.gtx_discover_words.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.gtx_discover_words.restype = C.c_void_p
        L.gtx_discover_good.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.gtx_discover_good.restype = C.c_void_p
        L.gtx_discover_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.gtx_discover_stats.restype = C.POINTER(DiscoverFileStats)
        if hasattr(L, "gtx_discover_files"):  # (GTX_LIB= a build of an earlier commit has no BAM front end of discovery)
            L.gtx_disc_bam_read.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
            L.gtx_disc_bam_destroy.argtypes = [C.c_void_p]
            L.gtx_disc_bam_destroy.restype = None
            L.gtx_disc_bam_stream.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
            L.gtx_disc_bam_stream.restype = C.c_void_p
            L.gtx_disc_bam_reads.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]
            L.gtx_disc_bam_reads.restype = C.c_void_p
            L.gtx_disc_bam_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
            L.gtx_disc_bam_info.restype = C.c_char_p
            L.gtx_disc_bam_unpack.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_uint32, C.c_void_p]
            L.gtx_discover_files.argtypes = [C.c_char_p, C.c_uint64, C.c_int64, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(DiscoverParams),
                                             C.POINTER(C.c_void_p)]
        if hasattr(L, "gtx_discover_files_front"):  # (GTX_LIB= a build of an earlier commit has no device front)
            L.gtx_disc_bam_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(BamWalkOut),
                                            C.c_void_p]
            L.gtx_discover_files_front.argtypes = [C.c_char_p, C.c_uint64, C.c_int64, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(DiscoverParams),
                                                   C.c_uint32, C.POINTER(C.c_void_p)]
            L.gtx_discover_front.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
            L.gtx_discover_front.restype = C.POINTER(DiscoverFrontStats)
        L.gtx_wave_probe.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p]
        L.gtx_vcf_header.argtypes = [C.POINTER(VcfHeaderRequest), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_bgzf_compress.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.gtx_device_cache_release.argtypes = []
        L.gtx_device_cache_release.restype = None
        L.gtx_pack_planes.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
        L.gtx_reads_to_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]
        L.gtx_score_batch_words.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(ScoreBuffers), C.c_void_p]
        L.gtx_item_words.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.gtx_align_batch_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.gtx_align_batch_planes_staged.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_stream_set_planes.argtypes = [C.c_void_p, C.c_uint32]
        L.gtx_pack_2bit.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                    C.POINTER(C.c_uint32)]
        L.gtx_stream_push_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                             C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32,
                                             C.POINTER(C.c_uint32)]
        L.gtx_packed_to_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                           C.c_void_p]
        L.gtx_align_batch_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                             C.c_uint32, C.c_void_p, C.c_void_p]
        L.gtx_align_batch_packed_staged.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                    C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gtx_score_batch_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(ScoreBuffers), C.c_void_p]
        L.gtx_reads_open.argtypes = [C.POINTER(C.c_char_p), C.c_uint32, C.c_char_p, C.POINTER(C.c_void_p)]
        L.gtx_reads_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.gtx_reads_sample_name.argtypes = [C.c_void_p, C.c_uint32]
        L.gtx_reads_sample_name.restype = C.c_char_p
        L.gtx_reads_next.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
        L.gtx_reads_close.argtypes = [C.c_void_p]
        L.gtx_reads_close.restype = None
        L.gtx_bam_shrink_multi.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(ShrinkParams), C.c_char_p, C.POINTER(ShrinkStats)]
        L.gtx_inflate_raw.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64]
        if hasattr(L, "gtx_inflate_create"):  # (GTX_LIB= a build of an earlier commit, for A/B runs, has no device inflater; build() insists on EXPORTS)
            L.gtx_inflate_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
            L.gtx_inflate_destroy.argtypes = [C.c_void_p]
            L.gtx_inflate_destroy.restype = None
            L.gtx_inflate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
            L.gtx_inflate_bgzf.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int]
            L.gtx_reads_set_inflate_device.argtypes = [C.c_void_p, C.c_int]
            L.gtx_reads_inflate_counts.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gtx_regions_run.argtypes = [C.POINTER(RegionJob), C.c_uint32, C.POINTER(Params), C.c_int, C.c_char_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32,
                                      C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RegionsStats)]
        L.gtx_regions_free.argtypes = [C.POINTER(RegionJob), C.c_uint32]
        L.gtx_regions_free.restype = None
        L.gtx_pipeline_run.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                       C.POINTER(ScoreBuffers), C.POINTER(PipelineStats)]
        L.gtx_tabix_build.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
        L.gtx_tabix_start.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        L.gtx_shrink_params_default.argtypes = [C.POINTER(ShrinkParams)]
        L.gtx_shrink_params_default.restype = None
        L.gtx_bam_shrink.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(ShrinkParams),
                                     C.c_char_p, C.POINTER(ShrinkStats)]
        L.gtx_scores_replay.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gtx_stream_create.argtypes = [C.POINTER(Params), C.c_uint32, C.POINTER(C.c_void_p)]
        L.gtx_stream_destroy.argtypes = [C.c_void_p]
        L.gtx_stream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.gtx_stream_set_coverage.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.gtx_stream_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.gtx_stream_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gtx_dstream_create.argtypes = [C.POINTER(Params), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.gtx_dstream_destroy.argtypes = [C.c_void_p]
        L.gtx_dstream_destroy.restype = None
        L.gtx_dstream_push.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p]
        L.gtx_dstream_finish.argtypes = [C.c_void_p, C.c_void_p]
        L.gtx_dstream_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.gtx_graph_build.argtypes = [C.c_char_p, C.c_uint64, C.c_int64, C.c_int64, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(C.c_void_p)]
        L.gtx_graph_from_files.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.gtx_graph_get_view.argtypes = [C.c_void_p, C.POINTER(GraphView)]
        L.gtx_graph_destroy.argtypes = [C.c_void_p]
        L.gtx_scores_alloc.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(ScoreBuffers), C.POINTER(C.c_uint64)]
        L.gtx_scores_zero.argtypes = [C.c_void_p, C.POINTER(ScoreBuffers), C.c_void_p]
        L.gtx_scores_free.argtypes = [C.c_void_p, C.POINTER(ScoreBuffers)]
        L.gtx_scores_reduce.argtypes = [C.c_void_p, C.POINTER(ScoreBuffers), C.c_void_p, C.c_void_p]
        L.gtx_comm_unique_id.argtypes = [C.c_void_p]
        L.gtx_comm_init_rank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.gtx_comm_destroy.argtypes = [C.c_void_p]
        _lib = L
    return _lib


class GtxError(RuntimeError):
    def __init__(self, status):
        L = lib()
        self.status = status
        super().__init__("%s: %s" % (L.gtx_strerror(status).decode(), L.gtx_last_error().decode()))


def check(status):
    if status != 0:
        raise GtxError(status)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_hip = None


def download(ptr, dtype, count):
    """host copy of `count` elements of `dtype` at the device pointer `ptr` (hipMemcpy, synchronous)"""
    global _hip
    out = np.zeros(int(count), dtype)
    if out.nbytes:
        if _hip is None:
            _hip = C.CDLL("libamdhip64.so")
            _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rc = _hip.hipMemcpy(_p(out), C.c_void_p(int(ptr)), C.c_size_t(out.nbytes), C.c_int(2))  # hipMemcpyDeviceToHost
        if rc != 0:
            raise RuntimeError("hipMemcpy failed (%d)" % rc)
    return out


# ------------------------------------------------------------------------------------------------------------------
# binding of the host graph builder gtx_graph_build (Graph::add_genomic_region, src/graph/graph.cpp:41-339, including the
# record merge rules) -- SURVEY.md 8(f) row 1
# ------------------------------------------------------------------------------------------------------------------
def parse_events(info):
    """GT_ID / GT_ANTI_HAPLOTYPE of a single-alt record (src/graph/constructor.cpp:1540-1588) ->
    (ref_events, alt_events, alt_anti_events)"""
    ref_ev, alt_ev, alt_anti = [], [], []
    if info and info != ".":
        for kv in info.split(";"):
            if "=" not in kv:
                continue
            k, v = kv.split("=", 1)
            if k == "GT_ID":
                ref_ev.append(-int(v))
                alt_ev.append(int(v))
            elif k == "GT_ANTI_HAPLOTYPE":
                alt_anti.extend(int(x) for x in v.split(","))
    return ref_ev, alt_ev, alt_anti


class _Allele(C.Structure):
    _fields_ = [("seq", C.c_char_p), ("len", C.c_uint32), ("events", C.POINTER(C.c_int64)), ("n_events", C.c_uint32),
                ("anti_events", C.POINTER(C.c_int64)), ("n_anti_events", C.c_uint32)]


class _Record(C.Structure):
    _fields_ = [("pos", C.c_uint32), ("n_alleles", C.c_uint32), ("alleles", C.POINTER(_Allele)), ("is_sv", C.c_int32)]


class RegionJob(C.Structure):
    _fields_ = [("reference", C.c_char_p), ("reference_len", C.c_uint64), ("region_begin", C.c_int64), ("region_end", C.c_int64),
                ("records", C.POINTER(_Record)), ("n_records", C.c_uint32), ("add_all_variants", C.c_int32), ("d_planes", C.c_void_p),
                ("plane_stride", C.c_uint32), ("d_meta", C.c_void_p), ("n_reads", C.c_uint64), ("d_items", C.c_void_p), ("n_items", C.c_uint64),
                ("vcf_begin", C.c_uint32), ("vcf_end", C.c_uint32), ("filter_zero_qual", C.c_int32), ("status", C.c_int32),
                ("text", C.c_void_p), ("text_len", C.c_uint64)]


def _explicit_events(info, n_alts):
    """test syntax used by tests/test_graph_vectors.py: RE= / RA= (reference allele events / anti events),
    E<i>= / A<i>= (alt i); comma separated integers"""
    ev = [([], []) for _ in range(n_alts + 1)]
    if info and info != ".":
        for kv in info.split(";"):
            if "=" not in kv:
                continue
            k, v = kv.split("=", 1)
            if k in ("RE", "RA") or (k[0] in "EA" and k[1:].isdigit()):
                vals = [int(x) for x in v.split(",") if x]
                if k == "RE":
                    ev[0][0].extend(vals)
                elif k == "RA":
                    ev[0][1].extend(vals)
                elif int(k[1:]) < n_alts:
                    ev[int(k[1:]) + 1][0 if k[0] == "E" else 1].extend(vals)
    return ev


def records_array(records):
    """[(pos0, ref, [alts], info)] -> (array of gtx_record, what it points into: keep both alive while the array is in use)"""
    keep = []
    recs = (_Record * max(len(records), 1))()
    for i, (pos, ref, alts, info) in enumerate(records):
        ev = _explicit_events(info, len(alts))
        if len(alts) == 1:
            r_ev, a_ev, a_anti = parse_events(info)
            ev[0][0].extend(r_ev)
            ev[1][0].extend(a_ev)
            ev[1][1].extend(a_anti)
        als = (_Allele * (len(alts) + 1))()
        for j, seq in enumerate([ref] + list(alts)):
            b = seq.encode()
            e = (C.c_int64 * max(len(ev[j][0]), 1))(*ev[j][0])
            a = (C.c_int64 * max(len(ev[j][1]), 1))(*ev[j][1])
            keep.extend([b, e, a])
            als[j] = _Allele(b, len(b), e, len(ev[j][0]), a, len(ev[j][1]))
        keep.append(als)
        recs[i] = _Record(pos, len(alts) + 1, als, 0)
    return recs, keep


def graph_from_records(reference, records, region_begin=0, region_end=0xFFFFFFFF, add_all_variants=False,
                       extend_prefix=False, is_sv_graph=False):
    """reference: str of the region; records: [(pos0, ref, [alts], info)] sorted by pos0 (contig coordinates, 0-based).
    Calls gtx_graph_build (C++: filters, record merging, node emission) and returns the node tables as numpy arrays laid
    out as gtx_graph_view expects."""
    L = lib()
    recs, keep = records_array(records)
    h = C.c_void_p()
    refb = reference.encode()
    check(L.gtx_graph_build(refb, len(refb), region_begin, region_end, recs, len(records), int(add_all_variants),
                            int(is_sv_graph), int(extend_prefix), C.byref(h)))
    return _graph_tables(h)


def _graph_tables(h):
    """node tables of a gtx_graph as numpy arrays laid out as gtx_graph_view expects; destroys the handle"""
    L = lib()
    try:
        v = GraphView()
        check(L.gtx_graph_get_view(h, C.byref(v)))

        def arr(ptr, n, dt):
            if not ptr or n == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy()

        R, V = v.n_ref, v.n_var
        g = dict(ref_order=arr(v.ref_order, R, np.uint32), ref_len=arr(v.ref_len, R, np.uint32),
                 ref_dna_off=arr(v.ref_dna_off, R, np.uint32), ref_nvar=arr(v.ref_nvar, R, np.uint32),
                 ref_first_var=arr(v.ref_first_var, R, np.uint32), var_order=arr(v.var_order, V, np.uint32),
                 var_len=arr(v.var_len, V, np.uint32), var_dna_off=arr(v.var_dna_off, V, np.uint32),
                 var_out_ref=arr(v.var_out_ref, V, np.uint32), dna=arr(v.dna, v.dna_len, np.uint8))
        if v.event_off:
            g["event_off"] = arr(v.event_off, 2 * V + 1, np.uint32)
            g["event_val"] = arr(v.event_val, int(g["event_off"][-1]), np.int64)
        else:
            g["event_off"] = np.zeros(2 * V + 1, np.uint32)
            g["event_val"] = np.zeros(0, np.int64)
        return g
    finally:
        L.gtx_graph_destroy(h)


def graph_from_files(fasta, vcf, region, add_all_variants=False, is_sv_graph=False, with_sv_table=False):
    """gtx_graph_from_files (construct_graph, src/graph/constructor.cpp:1597-1777): node tables + (begin, end) of the
    reference span that was read (0-based) [+ Graph::SVs as text: gtx_graph_sv_table]"""
    L = lib()
    h = C.c_void_p()
    b, e = C.c_int64(), C.c_int64()
    check(L.gtx_graph_from_files(str(fasta).encode(), (str(vcf) if vcf else "").encode(), region.encode(), int(add_all_variants),
                                 int(is_sv_graph), C.byref(h), C.byref(b), C.byref(e)))
    table = None
    if with_sv_table:
        n = C.c_uint64()
        check(L.gtx_graph_sv_table(h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(int(n.value) + 1)
        check(L.gtx_graph_sv_table(h, buf, int(n.value), C.byref(n)))
        table = buf.raw[:int(n.value)].decode()
    tables = _graph_tables(h)
    return (tables, (int(b.value), int(e.value)), table) if with_sv_table else (tables, (int(b.value), int(e.value)))


def disc_first_pass_device(handle, d_planes, plane_stride, d_reads, d_cigar, d_read_out, n_reads, d_events, d_counts, bucket_size=50, file_index=None,
                           stream=None, cap=1 << 16):
    """gtx_disc_first_pass_device (file_index None) or gtx_disc_first_pass_haplotypes_device over the device arrays of
    gtx_disc_events_batch (device pointers as integers) -> the result words; the call is repeated once with the size it names when
    `cap` words are too few.  Raises GtxError on any other status."""
    L = lib()
    n_words = C.c_uint64()
    while True:
        words = np.zeros(max(int(cap), 1), np.uint32)
        if file_index is None:
            rc = L.gtx_disc_first_pass_device(handle, d_planes, plane_stride, d_reads, d_cigar, d_read_out, n_reads, d_events, d_counts, bucket_size, _p(words),
                                              int(cap), C.byref(n_words), stream)
        else:
            rc = L.gtx_disc_first_pass_haplotypes_device(handle, d_planes, plane_stride, d_reads, d_cigar, d_read_out, n_reads, d_events, d_counts, bucket_size,
                                                         file_index, _p(words), int(cap), C.byref(n_words), stream)
        if rc == 5 and n_words.value > cap:
            cap = int(n_words.value)
            continue
        check(rc)
        return words[:n_words.value]


def disc_indel_table(words):
    """gtx_disc_indel_table: the words of gtx_disc_merge -> (DISC_INDEL array in table order, the letters as a uint8 array)"""
    L = lib()
    words = np.ascontiguousarray(words, np.uint32)
    n, n_seq = C.c_uint32(), C.c_uint64()
    rc = L.gtx_disc_indel_table(_p(words), len(words), None, 0, C.byref(n), None, 0, C.byref(n_seq))
    if rc not in (0, 5):
        check(rc)
    entries, seq = np.zeros(max(n.value, 1), DISC_INDEL), np.zeros(max(n_seq.value, 1), np.uint8)
    check(L.gtx_disc_indel_table(_p(words), len(words), _p(entries), n.value, C.byref(n), _p(seq), n_seq.value, C.byref(n_seq)))
    return entries[:n.value], seq[:n_seq.value]


def disc_second_buckets(reference_len, bucket_size):
    """the number of buckets of a region (gtx.h)"""
    return (reference_len - 1) // bucket_size + 1


def disc_second_plan(entries, found, file_index):
    """gtx_disc_second_plan: the table, the found-bits of gtx_disc_second_intake (uint32 words) and the file's index -> its list as
    table indices"""
    L = lib()
    entries, found = np.ascontiguousarray(entries, DISC_INDEL), np.ascontiguousarray(found, np.uint32)
    out, n = np.zeros(max(len(entries), 1), np.uint32), C.c_uint32()
    check(L.gtx_disc_second_plan(_p(entries) if len(entries) else None, len(entries), _p(found) if len(entries) else None, file_index, _p(out), len(out),
                                 C.byref(n)))
    return out[:n.value]


def disc_second_rounds(handle, d_planes, plane_stride, d_list, k0, k1, d_table, d_table_seq, n_table, n_table_seq, d_second, n_reads, d_events, event_cap,
                       n_events, bucket_size, d_bucket_max, d_bucket_global_max, d_max_read_size, d_bucket_reads, d_bucket_off, d_support, stream=None):
    """gtx_disc_second_rounds over device pointers (integers) -> (status, the entries in use, the statistics as a dict).  status is 0, or
    5 (GTX_ERR_CAPACITY: the event array is too small for round k0 + rounds_done, which wants events_wanted entries; the state is that
    round's beginning); any other status raises GtxError."""
    L = lib()
    n, stats = C.c_uint32(n_events), DiscRoundsStats()
    rc = L.gtx_disc_second_rounds(handle, d_planes, plane_stride, d_list, k0, k1, d_table, d_table_seq, n_table, n_table_seq, d_second, n_reads, d_events, event_cap,
                                  C.byref(n), bucket_size, d_bucket_max, d_bucket_global_max, d_max_read_size, d_bucket_reads, d_bucket_off, d_support,
                                  C.byref(stats), stream)
    if rc not in (0, 5):
        check(rc)
    return rc, int(n.value), stats.as_dict()


def disc_second_decide(entries, lst, support):
    """gtx_disc_second_decide: the table, a file's list and its downloaded counters -> per table entry, whether the file's rounds gave
    it good support (bool array; an entry that was good already stays False)"""
    L = lib()
    entries, lst, support = np.ascontiguousarray(entries, DISC_INDEL), np.ascontiguousarray(lst, np.uint32), np.ascontiguousarray(support, DISC_SECOND_SUPPORT)
    assert len(support) == len(entries)
    bits = np.zeros(max((len(entries) + 31) // 32, 1), np.uint32)
    check(L.gtx_disc_second_decide(_p(entries) if len(entries) else None, len(entries), _p(lst) if len(lst) else None, len(lst),
                                   _p(support) if len(entries) else None, _p(bits)))
    return np.array([(bits[t >> 5] >> (t & 31)) & 1 for t in range(len(entries))], bool)


def disc_set_max_read_len(handle, n):
    """gtx_disc_set_max_read_len: 0 or 256 for the aligner's default limits (256 bases, 2 048 letters), 257 .. MAX_READ_LONG for reads of
    up to n bases and windows of up to REALIGN_MAX_TARGET_LONG letters; anything else raises GtxError"""
    check(lib().gtx_disc_set_max_read_len(handle, int(n)))


def disc_second_file(handle, reference_len, planes, plane_stride, reads, cigar, words, file_index, bucket_size=50, event_cap=None, stream=None,
                     max_read_len=None):
    """A file's whole second pass up to the good-bits: the table of the merged `words`, the intake of the file's reads (numpy arrays as
    gtx_disc_events_batch takes them: plane rows, DISC_READ, cigar words), its plan, its rounds and the final decision.  handle: a gtx_disc of the region, reference_len: the region's length.  The event
    array starts at `event_cap` entries (default: two per read, at least 1024) and is doubled -- the call continued at the round it
    stopped in front of -- whenever the rounds report that it is too small.  max_read_len: when given, set on `handle` first
    (disc_set_max_read_len; it stays set).
    -> dict(entries, letters, lst, good [bool per table entry], second [DISC_SECOND_READ], lists [per read, [(table index, read_pos)]],
            support [DISC_SECOND_SUPPORT], stats)"""
    import torch
    L = lib()
    if max_read_len is not None:
        disc_set_max_read_len(handle, max_read_len)
    entries, letters = disc_indel_table(words)
    n, nt = len(reads), len(entries)
    dev = lambda x: torch.from_numpy(np.concatenate([np.ascontiguousarray(x).view(np.uint8).reshape(-1), np.zeros(16, np.uint8)])).to("cuda:0")  # noqa: E731
    zeros = lambda nbytes: torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda:0")  # noqa: E731
    d_planes, d_reads, d_cigar = dev(planes), dev(np.ascontiguousarray(reads, DISC_READ)), dev(np.ascontiguousarray(cigar, np.uint32))
    d_table, d_letters = zeros(nt * DISC_INDEL.itemsize), zeros(len(letters))
    check(L.gtx_disc_indel_table_upload(handle, _p(entries) if nt else None, nt, _p(letters) if len(letters) else None, len(letters), d_table.data_ptr(),
                                        d_letters.data_ptr(), stream))
    nb = disc_second_buckets(reference_len, bucket_size)
    d_second, d_bmax, d_gmax, d_mrs = zeros(n * DISC_SECOND_READ.itemsize), zeros(4 * nb), zeros(4 * nb), zeros(4)
    d_breads, d_boff, d_found = zeros(4 * n), zeros(4 * (nb + 1)), zeros(4 * ((nt + 31) // 32))
    torch.cuda.synchronize()
    check(L.gtx_disc_second_intake(handle, d_planes.data_ptr(), plane_stride, d_reads.data_ptr(), d_cigar.data_ptr(), n, bucket_size, d_table.data_ptr(),
                                   d_letters.data_ptr(), nt, len(letters), d_second.data_ptr(), d_bmax.data_ptr(), d_gmax.data_ptr(), d_mrs.data_ptr(),
                                   d_breads.data_ptr(), d_boff.data_ptr(), d_found.data_ptr(), stream))
    torch.cuda.synchronize()
    found = d_found.cpu().numpy()[:4 * ((nt + 31) // 32)].view(np.uint32)
    lst = disc_second_plan(entries, found, file_index)
    d_list = dev(lst)
    cap = int(event_cap) if event_cap is not None else max(2 * n, 1024)
    d_events, d_support = zeros(cap * DISC_SECOND_EVENT.itemsize), zeros(nt * DISC_SECOND_SUPPORT.itemsize)
    k, used, total = 0, 0, None
    while True:
        torch.cuda.synchronize()
        rc, used, stats = disc_second_rounds(handle, d_planes.data_ptr(), plane_stride, d_list.data_ptr(), k, len(lst), d_table.data_ptr(), d_letters.data_ptr(), nt,
                                             len(letters), d_second.data_ptr(), n, d_events.data_ptr(), cap, used, bucket_size, d_bmax.data_ptr(), d_gmax.data_ptr(),
                                             d_mrs.data_ptr(), d_breads.data_ptr(), d_boff.data_ptr(), d_support.data_ptr(), stream)
        torch.cuda.synchronize()
        k += stats["rounds_done"]
        wanted = stats.pop("events_wanted")
        total = stats if total is None else {key: total[key] + stats[key] for key in stats}
        if rc == 0:
            break
        if wanted <= cap:  # (GTX_ERR_CAPACITY for another reason: a round whose windows are too large)
            check(rc)
        cap = max(2 * cap, wanted)
        bigger = zeros(cap * DISC_SECOND_EVENT.itemsize)
        bigger[:used * DISC_SECOND_EVENT.itemsize] = d_events[:used * DISC_SECOND_EVENT.itemsize]
        d_events = bigger
    second = d_second.cpu().numpy()[:n * DISC_SECOND_READ.itemsize].view(DISC_SECOND_READ).copy()
    events = d_events.cpu().numpy()[:used * DISC_SECOND_EVENT.itemsize].view(DISC_SECOND_EVENT)
    support = d_support.cpu().numpy()[:nt * DISC_SECOND_SUPPORT.itemsize].view(DISC_SECOND_SUPPORT).copy()
    lists = [[(int(e["indel"]), int(e["read_pos"])) for e in events[r["first_event"]:r["first_event"] + r["n_events"]]] for r in second]
    return dict(entries=entries, letters=letters, lst=lst, good=disc_second_decide(entries, lst, support), second=second, lists=lists, support=support, stats=total)


def disc_second_file_c(handle, d_planes, plane_stride, d_reads, d_cigar, n_reads, words, file_index, bucket_size=50, event_cap=0, stream=None, state=True):
    """gtx_disc_second_file: a file's whole second pass in one call of the library, over device arrays of the caller's (pointers as
    integers) and the merged `words` -> what disc_second_file returns without entries and letters; state=False leaves second, lists and
    support out (the optional outputs are not asked for)."""
    L = lib()
    words = np.ascontiguousarray(words, np.uint32)
    nt, n_seq = C.c_uint32(), C.c_uint64()
    rc = L.gtx_disc_indel_table(_p(words), len(words), None, 0, C.byref(nt), None, 0, C.byref(n_seq))
    if rc not in (0, 5):
        check(rc)
    nt = nt.value
    bits, lst, n_list, stats = np.zeros(max((nt + 31) // 32, 1), np.uint32), np.zeros(max(nt, 1), np.uint32), C.c_uint32(), DiscRoundsStats()
    second, support = np.zeros(max(n_reads, 1), DISC_SECOND_READ), np.zeros(max(nt, 1), DISC_SECOND_SUPPORT)
    events_cap, n_events = max(4 * n_reads, 1024), C.c_uint32()
    while True:
        events = np.zeros(events_cap, DISC_SECOND_EVENT)
        rc = L.gtx_disc_second_file(handle, d_planes, plane_stride, d_reads, d_cigar, n_reads, _p(words), len(words), file_index, bucket_size, event_cap, _p(bits),
                                    _p(lst), len(lst), C.byref(n_list), C.byref(stats), _p(second) if state else None, _p(events) if state else None,
                                    events_cap if state else 0, C.byref(n_events) if state else None, _p(support) if state else None, stream)
        if rc == 5 and state and n_events.value > events_cap:  # (the lists are an output of unknown size: the run is repeated for them alone)
            events_cap = n_events.value
            continue
        check(rc)
        break
    stats = stats.as_dict()
    stats.pop("events_wanted")
    out = dict(lst=lst[:n_list.value].copy(), good=np.array([(bits[t >> 5] >> (t & 31)) & 1 for t in range(nt)], bool), stats=stats)
    if state:
        second, events = second[:n_reads], events[:n_events.value]
        out.update(second=second, support=support[:nt],
                   lists=[[(int(e["indel"]), int(e["read_pos"])) for e in events[r["first_event"]:r["first_event"] + r["n_events"]]] for r in second])
    return out


def disc_variants(handle, words, good_bits=None):
    """gtx_disc_variants: the merged words and the files' ORed good-bits (uint32 words, or None) -> (DISC_VARIANT array, letters as bytes,
    ids as a uint32 array)"""
    L = lib()
    words = np.ascontiguousarray(words, np.uint32)
    bits = None if good_bits is None else np.ascontiguousarray(good_bits, np.uint32)
    n, n_letters, n_ids = C.c_uint32(), C.c_uint64(), C.c_uint64()
    rc = L.gtx_disc_variants(handle, _p(words), len(words), _p(bits), None, 0, C.byref(n), None, 0, C.byref(n_letters), None, 0, C.byref(n_ids))
    if rc not in (0, 5):
        check(rc)
    recs, letters, ids = np.zeros(max(n.value, 1), DISC_VARIANT), np.zeros(max(n_letters.value, 1), np.uint8), np.zeros(max(n_ids.value, 1), np.uint32)
    check(L.gtx_disc_variants(handle, _p(words), len(words), _p(bits), _p(recs), n.value, C.byref(n), _p(letters), n_letters.value, C.byref(n_letters), _p(ids),
                              n_ids.value, C.byref(n_ids)))
    return recs[:n.value], letters[:n_letters.value].tobytes(), ids[:n_ids.value]


def disc_vcf_sites(recs, letters, ids, contig):
    """gtx_disc_vcf_sites: records as disc_variants returns them and a contig name -> the text of the sites file behind its header (bytes)"""
    L = lib()
    recs, ids = np.ascontiguousarray(recs, DISC_VARIANT), np.ascontiguousarray(ids, np.uint32)
    letters = np.frombuffer(bytes(letters), np.uint8)
    n = C.c_uint64()
    args = (_p(recs) if len(recs) else None, len(recs), _p(letters) if len(letters) else None, len(letters), _p(ids) if len(ids) else None, len(ids), contig.encode())
    rc = L.gtx_disc_vcf_sites(*args, None, 0, C.byref(n))
    if rc not in (0, 5):
        check(rc)
    buf = C.create_string_buffer(int(n.value) + 1)
    check(L.gtx_disc_vcf_sites(*args, buf, int(n.value), C.byref(n)))
    return buf.raw[:int(n.value)]


def discover_region(reference, region_begin, contig, files, device=0, bucket_size=50, max_read_len=0, n_threads=1, first_event_cap=0, second_event_cap=0):
    """gtx_discover_region: a region's discovery from host arrays to the sites file.  reference: the region's letters (str or bytes);
    files: per file a dict(planes, plane_stride, qual, qual_stride, reads [DISC_READ], cigar [uint32]) of numpy arrays as
    gtx_disc_events_batch takes them.
    -> dict(text [bytes], variants [DISC_VARIANT], letters [bytes], ids [uint32], words [uint32], good [bool per table entry],
            stats [per file: dict(events, events_passes, n_list, rounds)])"""
    L = lib()
    refb = reference.encode("latin-1") if isinstance(reference, str) else bytes(reference)
    keep, structs = [], (DiscFile * max(len(files), 1))()
    for i, f in enumerate(files):
        planes, qual = np.ascontiguousarray(f["planes"]).view(np.uint8).reshape(-1), np.ascontiguousarray(f["qual"]).view(np.uint8).reshape(-1)  # (bytes as they lie)
        reads, cigar = np.ascontiguousarray(f["reads"], DISC_READ), np.ascontiguousarray(f["cigar"], np.uint32)
        if planes.size != len(reads) * int(f["plane_stride"]) or qual.size != len(reads) * int(f["qual_stride"]):
            raise ValueError("discover_region: file %d: the rows do not have the strides' sizes" % i)
        keep.append((planes, qual, reads, cigar))
        structs[i] = DiscFile(planes.ctypes.data if planes.size else None, qual.ctypes.data if qual.size else None, reads.ctypes.data if len(reads) else None,
                              cigar.ctypes.data if len(cigar) else None, int(f["plane_stride"]), int(f["qual_stride"]), len(reads), len(cigar))
    params = _discover_params(device, bucket_size, max_read_len, n_threads, first_event_cap, second_event_cap)
    h = C.c_void_p()
    check(L.gtx_discover_region(refb, len(refb), region_begin, contig.encode(), structs, len(files), C.byref(params), C.byref(h)))
    return _discover_result(h)


def _discover_params(device, bucket_size, max_read_len, n_threads, first_event_cap, second_event_cap):
    params = DiscoverParams()
    lib().gtx_discover_params_default(C.byref(params))
    params.device, params.bucket_size, params.max_read_len, params.n_threads = device, bucket_size, max_read_len, n_threads
    params.first_event_cap, params.second_event_cap = first_event_cap, second_event_cap
    return params


def _discover_result(h, front=False):
    """what a gtx_discover_result holds, as discover_region documents it (front: and, as "front", what gtx_discover_front says of each
    file); the handle is destroyed"""
    L = lib()
    try:
        def view(ptr, dtype, count):
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype).copy() if count else np.zeros(0, dtype)
        n64, n32, letters, n_letters, ids, n_ids = C.c_uint64(), C.c_uint32(), C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        ptr = L.gtx_discover_text(h, C.byref(n64))
        out = dict(text=C.string_at(ptr, n64.value) if n64.value else b"")
        ptr = L.gtx_discover_variants(h, C.byref(n32), C.byref(letters), C.byref(n_letters), C.byref(ids), C.byref(n_ids))
        out.update(variants=view(ptr, DISC_VARIANT, n32.value), letters=view(letters.value, np.uint8, n_letters.value).tobytes(),
                   ids=view(ids.value, np.uint32, n_ids.value))
        ptr = L.gtx_discover_words(h, C.byref(n64))
        out["words"] = view(ptr, np.uint32, n64.value)
        ptr = L.gtx_discover_good(h, C.byref(n32))
        out["good"] = view(ptr, np.uint8, n32.value).astype(bool)
        st = L.gtx_discover_stats(h, C.byref(n32))
        out["stats"] = [dict(events=int(st[i].events), events_passes=int(st[i].events_passes), n_list=int(st[i].n_list), rounds=st[i].rounds.as_dict())
                        for i in range(n32.value)]
        if front:
            fr = L.gtx_discover_front(h, C.byref(n32))
            out["front"] = [{name: int(getattr(fr[i], name)) for name, _ in DiscoverFrontStats._fields_ if name != "reserved"} for i in range(n32.value)]
        return out
    finally:
        L.gtx_discover_destroy(h)


FRONTS = {"host": 0, "device": 1}


def discover_files(reference, region_begin, contig, paths, device=0, bucket_size=50, max_read_len=0, n_threads=1, first_event_cap=0, second_event_cap=0, front=None):
    """gtx_discover_files: discover_region from BAM paths (one sample each, read whole and in file order) -> what discover_region returns.
    front: None is gtx_discover_files; "host" (the same front end) and "device" (the files inflated, walked and unpacked on the device)
    go through gtx_discover_files_front and add "front": per file dict(members, members_device, segments_hit, segments_rewalked,
    fell_back)"""
    L = lib()
    refb = reference.encode("latin-1") if isinstance(reference, str) else bytes(reference)
    arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
    params = _discover_params(device, bucket_size, max_read_len, n_threads, first_event_cap, second_event_cap)
    h = C.c_void_p()
    if front is None:
        check(L.gtx_discover_files(refb, len(refb), region_begin, contig.encode(), arr, len(paths), C.byref(params), C.byref(h)))
        return _discover_result(h)
    check(L.gtx_discover_files_front(refb, len(refb), region_begin, contig.encode(), arr, len(paths), C.byref(params), FRONTS[front] if front in FRONTS else int(front),
                                     C.byref(h)))
    return _discover_result(h, front=True)


def disc_bam_read(path):
    """gtx_disc_bam_read: a BAM file of discovery, read whole -> dict(stream [uint8: the records as they lie in the file], slack [bytes
    behind the stream a device block has to have], reads [DISC_READ], offsets [uint32: each record's 32 fixed bytes in the stream],
    max_l_seq, n_cigar, sample [str]) of copies"""
    L = lib()
    h = C.c_void_p()
    check(L.gtx_disc_bam_read(os.fsencode(path), C.byref(h)))
    try:
        def view(ptr, dtype, count):
            return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype).copy() if count else np.zeros(0, dtype)
        n64, slack, n32, offsets, longest, n_cigar = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_void_p(), C.c_uint32(), C.c_uint64()
        ptr = L.gtx_disc_bam_stream(h, C.byref(n64), C.byref(slack))
        out = dict(stream=view(ptr, np.uint8, n64.value), slack=int(slack.value))
        ptr = L.gtx_disc_bam_reads(h, C.byref(n32), C.byref(offsets))
        out.update(reads=view(ptr, DISC_READ, n32.value), offsets=view(offsets.value, np.uint32, n32.value))
        sample = L.gtx_disc_bam_info(h, C.byref(longest), C.byref(n_cigar))
        out.update(max_l_seq=int(longest.value), n_cigar=int(n_cigar.value), sample=sample.decode())
        return out
    finally:
        L.gtx_disc_bam_destroy(h)


def disc_bam_unpack(handle, d_stream, n_bytes, d_offsets, d_reads, n_reads, d_planes, plane_stride, d_qual, qual_stride, d_cigar, n_cigar, stream=None):
    """gtx_disc_bam_unpack over device arrays of the caller's (pointers as integers): the stream, offsets and reads of disc_bam_read,
    uploaded -> the plane rows, quality rows and CIGAR words written; raises GtxError on any status but GTX_OK"""
    check(lib().gtx_disc_bam_unpack(handle, d_stream, n_bytes, d_offsets, d_reads, n_reads, d_planes, plane_stride, d_qual, qual_stride, d_cigar, n_cigar, stream))


def disc_bam_walk(handle, d_stream, n_bytes, cuts, d_offsets=None, d_reads=None, cap=0, stream=None):
    """gtx_disc_bam_walk over a record stream in device memory of the caller's (pointers as integers); cuts: strictly ascending offsets
    in (0, n_bytes), a host list.  d_offsets / d_reads: device tables of `cap` entries, or None and cap 0 for the counts alone.
    -> (status of the call, dict(status, bad_at, n_reads, n_cigar, max_l_seq, segments_hit, segments_rewalked)); the call's status is
    GTX_OK or GTX_ERR_CAPACITY (n_reads > cap: the dict is filled, no table entry written), any other raises GtxError"""
    cuts = np.ascontiguousarray(cuts, np.uint32)
    out = BamWalkOut()
    rc = lib().gtx_disc_bam_walk(handle, d_stream, n_bytes, cuts.ctypes.data if len(cuts) else None, len(cuts), d_offsets, d_reads, cap, C.byref(out), stream)
    if rc not in (0, 5):
        check(rc)
    return rc, {name: int(getattr(out, name)) for name, _ in BamWalkOut._fields_ if name != "reserved"}


def disc_realign_target(handle, max_read_size, events):
    """gtx_disc_realign_target.  events: [(pos, 'I' | 'D', letters)], events[0] the indel being realigned to (a deletion's letters
    count by their number only) -> (the window's letters as bytes, ref_pos int32 array, begin_padded, applied bits)"""
    L = lib()
    ev = np.zeros(len(events), REALIGN_EVENT)
    letters = b""
    for i, (pos, kind, seq) in enumerate(events):
        ev[i] = (pos, len(seq), ord(kind), 0, len(letters))
        letters += seq.encode() if isinstance(seq, str) else bytes(seq)
    cap = 2 * (int(max_read_size) + 100) + len(letters)
    seq, ref_pos = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.int32)
    n, begin, applied = C.c_uint32(), C.c_int64(), C.c_uint64()
    check(L.gtx_disc_realign_target(handle, max_read_size, _p(ev), len(ev), letters, _p(seq), _p(ref_pos), cap, C.byref(n), C.byref(begin), C.byref(applied)))
    return seq[:n.value].tobytes(), ref_pos[:n.value].copy(), int(begin.value), int(applied.value)


def disc_realign_decide(result, read_len, ref_pos, begin_padded, region_begin, old_score, indel_pos):
    """gtx_disc_realign_decide over one REALIGN_RESULT record -> a REALIGN_DECISION record"""
    res = np.array([result], REALIGN_RESULT)
    ref_pos = np.ascontiguousarray(ref_pos, np.int32)
    out = np.zeros(1, REALIGN_DECISION)
    check(lib().gtx_disc_realign_decide(_p(res), read_len, _p(ref_pos), len(ref_pos), begin_padded, region_begin, old_score, indel_pos, _p(out)))
    return out[0]


def disc_realign_batch(handle, planes, plane_stride, lens, n_reads, target_seq, target_off, n_targets, pairs, n_pairs, out=None, stream=None):
    """gtx_disc_realign_batch.  Every array is a device pointer (an integer: the call is then asynchronous on `stream`, `out` must be
    given and is returned as it is) or a numpy array (all of them: they go through torch tensors on cuda:0, the call waits and the
    results come back as a REALIGN_RESULT array)."""
    L = lib()
    arrays = (planes, lens, target_seq, target_off, pairs)
    if not any(isinstance(a, np.ndarray) for a in arrays):
        check(L.gtx_disc_realign_batch(handle, planes, plane_stride, lens, n_reads, target_seq, target_off, n_targets, pairs, n_pairs, out, stream))
        return out
    import torch
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0") if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda:0")
           for a in arrays]
    d_out = torch.zeros(max(n_pairs, 1) * REALIGN_RESULT.itemsize, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    check(L.gtx_disc_realign_batch(handle, dev[0].data_ptr(), plane_stride, dev[1].data_ptr(), n_reads, dev[2].data_ptr(), dev[3].data_ptr(), n_targets,
                                   dev[4].data_ptr(), n_pairs, d_out.data_ptr(), stream))
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(REALIGN_RESULT)[:n_pairs].copy()


def pack_nibbles(codes, stride=None):
    """[n, L] 4-bit codes -> [n, stride] BAM-packed bytes (high nibble first)"""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    nb = (L + 1) // 2
    stride = stride or ((nb + 15) // 16) * 16
    if L % 2:
        codes = np.concatenate([codes, np.zeros((n, 1), np.uint8)], axis=1)
    out = np.zeros((n, stride), np.uint8)
    out[:, :nb] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    return out


def pack_planes(seq, plane_stride=None):
    """gtx_pack_planes: [n, stride] BAM nibble rows -> [n, plane_stride] plane rows (include/gtx.h: reads as bit planes)"""
    seq = np.ascontiguousarray(seq, np.uint8)
    n, stride = seq.shape
    plane_stride = plane_stride or ((stride + 15) // 16) * 16
    out = np.zeros((n, plane_stride), np.uint8)
    check(lib().gtx_pack_planes(_p(seq), stride, n, _p(out), plane_stride))
    return out


def item_words(items):
    """gtx_item_words: the compact form of score items for gtx_score_batch_words (one uint32 per item)"""
    items = np.ascontiguousarray(items, SCORE_ITEM)
    out = np.zeros(len(items), np.uint32)
    check(lib().gtx_item_words(_p(items), len(items), _p(out)))
    return out


def planes_reference(codes, plane_stride):
    """the plane layout restated in numpy (tests): [n, L] codes -> [n, plane_stride] bytes"""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    groups = plane_stride // 16
    padded = np.zeros((n, groups * 32), np.uint8)
    padded[:, :L] = codes
    out = np.zeros((n, groups, 4), np.uint32)
    for b in range(4):
        bits = ((padded >> b) & 1).reshape(n, groups, 32).astype(np.uint32)
        out[:, :, b] = (bits << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    return out.reshape(n, groups * 4).view(np.uint8).reshape(n, plane_stride)


def pack_2bit(seq, l_qseq, packed_stride=None):
    """gtx_pack_2bit: [n, stride] BAM nibble rows of l_qseq[i] bases -> (rows [n, packed_stride] uint8, exc_start [n + 1] uint32,
    exc uint16) (include/gtx.h: packed 2-bit rows with an exception list)"""
    seq = np.ascontiguousarray(seq, np.uint8)
    n, stride = seq.shape
    l_qseq = np.ascontiguousarray(l_qseq, np.uint32)
    assert len(l_qseq) == n
    packed_stride = packed_stride or max(8, (stride // 2 + 7) // 8 * 8)  # (a row for every base of the nibble row)
    rows = np.zeros((n, packed_stride), np.uint8)
    exc_start = np.zeros(n + 1, np.uint32)
    n_exc = C.c_uint32()
    L = lib()
    rc = L.gtx_pack_2bit(_p(seq), stride, _p(l_qseq), n, _p(rows), packed_stride, _p(exc_start), None, 0, C.byref(n_exc))
    if rc not in (0, 5):  # (5: GTX_ERR_CAPACITY -- the first call only counts)
        check(rc)
    exc = np.zeros(max(n_exc.value, 1), np.uint16)
    check(L.gtx_pack_2bit(_p(seq), stride, _p(l_qseq), n, _p(rows), packed_stride, _p(exc_start), _p(exc), len(exc), C.byref(n_exc)))
    return rows, exc_start, exc[:n_exc.value]


def packed_reference(codes, packed_stride, lengths=None):
    """the packed layout restated in numpy (tests): [n, L] codes, read i being codes[i, :lengths[i]] (default: all L) ->
    (rows [n, packed_stride] uint8, exc_start [n + 1] uint32, exc uint16)"""
    codes = np.asarray(codes, np.uint8)
    n, L = codes.shape
    groups = packed_stride // 8
    inside = np.arange(L)[None, :] < (np.full(n, L) if lengths is None else np.asarray(lengths))[:, None]
    two = np.select([codes == 1, codes == 2, codes == 4, codes == 8], [0, 1, 2, 3], default=0).astype(np.uint8) * inside
    is_exc = ~np.isin(codes, (1, 2, 4, 8)) & inside
    padded = np.zeros((n, groups * 32), np.uint8)
    padded[:, :L] = two
    out = np.zeros((n, groups, 2), np.uint32)
    for b in range(2):
        bits = ((padded >> b) & 1).reshape(n, groups, 32).astype(np.uint64)
        out[:, :, b] = (bits << np.arange(32, dtype=np.uint64)).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    r, j = np.nonzero(is_exc)  # (row-major: sorted by read, then by base index)
    exc = (j.astype(np.uint32) | (codes[r, j].astype(np.uint32) << 12)).astype(np.uint16)
    exc_start = np.zeros(n + 1, np.uint32)
    exc_start[1:] = np.cumsum(np.bincount(r, minlength=n))
    return out.reshape(n, groups * 2).view(np.uint8).reshape(n, packed_stride), exc_start, exc


class Reads:
    """gtx_reads: BAM files merged into the record stream gtx_stream_push takes"""

    def __init__(self, paths, region=None):
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        h = C.c_void_p()
        check(lib().gtx_reads_open(arr, len(paths), region.encode() if region else None, C.byref(h)))
        self.h = h
        ns, nrg = C.c_uint32(), C.c_uint32()
        check(lib().gtx_reads_info(self.h, C.byref(ns), C.byref(nrg)))
        self.n_read_groups = int(nrg.value)
        self.samples = [lib().gtx_reads_sample_name(self.h, i).decode() for i in range(ns.value)]

    def next(self, cap, seq_stride=80):
        """(STREAM_RECORD [n], packed bases [n, seq_stride]); n = 0 at the end"""
        recs = np.zeros(cap, STREAM_RECORD)
        seq = np.zeros((cap, seq_stride), np.uint8)
        n = C.c_uint32()
        check(lib().gtx_reads_next(self.h, _p(recs), _p(seq), seq_stride, cap, C.byref(n)))
        return recs[:n.value], seq[:n.value]

    def set_inflate_device(self, device=0):
        """the files' BGZF members are inflated by the device from here on (gtx_reads_set_inflate_device)"""
        check(lib().gtx_reads_set_inflate_device(self.h, device))

    def close(self):
        if getattr(self, "h", None):
            lib().gtx_reads_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class VcfHeaderRequest(C.Structure):
    _fields_ = [("file_date", C.c_char_p), ("version", C.c_char_p), ("dirty", C.c_int32), ("git_branch", C.c_char_p), ("git_sha1", C.c_char_p),
                ("contig_names", C.POINTER(C.c_char_p)), ("contig_lengths", C.POINTER(C.c_uint32)), ("n_contigs", C.c_uint32),
                ("sample_names", C.POINTER(C.c_char_p)), ("n_samples", C.c_uint32), ("drop_genotypes", C.c_int32)]


def vcf_header(file_date, version, contigs, sample_names, dirty=False, git_branch="", git_sha1="", drop_genotypes=False):
    """gtx_vcf_header: contigs = [(name, length)] -> bytes"""
    names = (C.c_char_p * max(1, len(contigs)))(*[c[0].encode() for c in contigs])
    lens = (C.c_uint32 * max(1, len(contigs)))(*[c[1] for c in contigs])
    samples = (C.c_char_p * max(1, len(sample_names)))(*[s_.encode() for s_ in sample_names])
    rq = VcfHeaderRequest(file_date.encode(), version.encode(), int(dirty), git_branch.encode(), git_sha1.encode(), names, lens, len(contigs),
                          samples, len(sample_names), int(drop_genotypes))
    n = C.c_uint64()
    check(lib().gtx_vcf_header(C.byref(rq), None, 0, C.byref(n)))
    buf = C.create_string_buffer(int(n.value) + 1)
    check(lib().gtx_vcf_header(C.byref(rq), buf, n.value, C.byref(n)))
    return buf.raw[:int(n.value)]


def bgzf_compress(data, level=-1, with_eof=True):
    """gtx_bgzf_compress -> bytes"""
    n = C.c_uint64()
    src = C.create_string_buffer(data, len(data))
    check(lib().gtx_bgzf_compress(src, len(data), level, int(with_eof), None, 0, C.byref(n)))
    out = C.create_string_buffer(int(n.value) + 1)
    check(lib().gtx_bgzf_compress(src, len(data), level, int(with_eof), out, n.value, C.byref(n)))
    return out.raw[:int(n.value)]


def inflate_raw(data, out_len):
    """gtx_inflate_raw -> bytes (raises GtxError on a stream that is not valid or not of that size)"""
    out = C.create_string_buffer(max(out_len, 1))
    check(lib().gtx_inflate_raw(data, len(data), out, out_len))
    return out.raw[:out_len]


INFLATE_MEMBER = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("in_len", np.uint32), ("out_len", np.uint32), ("crc32", np.uint32),
                           ("reserved", np.uint32)], align=True)
assert INFLATE_MEMBER.itemsize == 32
INFLATE_OK, INFLATE_BAD_STREAM, INFLATE_SHORT, INFLATE_LONG, INFLATE_CRC, INFLATE_BAD_MEMBER = range(6)


def reads_inflate_counts():
    """(by the device, fell back to the host on a status, by the reader itself): members of readers on the device path, process-wide"""
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib().gtx_reads_inflate_counts(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


class Inflater:
    """DEFLATE on the device (gtx_inflate_*): BGZF members, one wavefront each"""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        check(lib().gtx_inflate_create(device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().gtx_inflate_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def batch(self, d_in, in_size, d_members, n, d_out, out_size, d_status, check_crc=True, stream=None):
        """device pointers (ints); asynchronous on `stream`"""
        check(lib().gtx_inflate_batch(self.h, d_in, in_size, d_members, n, d_out, out_size, d_status, int(check_crc), stream))

    def bgzf(self, data, check_crc=True):
        """the inflated bytes of a BGZF buffer (the inverse of bgzf_compress)"""
        n = C.c_uint64(0)
        check(lib().gtx_inflate_bgzf(self.h, data, len(data), None, 0, C.byref(n), int(check_crc)))
        out = np.zeros(max(1, n.value), np.uint8)
        check(lib().gtx_inflate_bgzf(self.h, data, len(data), _p(out), n.value, C.byref(n), int(check_crc)))
        return out[:n.value].tobytes()


def pipeline_run(ctx, paths, n_threads, buf, rec_words, record_slots_per_thread, chunk=65536, region=None):
    """gtx_pipeline_run over BAM files into the accumulator block `buf` (ScoreBuffers) -> its statistics as a dict"""
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    st = PipelineStats()
    check(lib().gtx_pipeline_run(ctx.h, arr, len(paths), n_threads, region.encode() if region else None, chunk, rec_words, record_slots_per_thread,
                                 C.byref(buf), C.byref(st)))
    return {k: getattr(st, k) for k, _ in PipelineStats._fields_}


class RegionJobs:
    """the job array of gtx_regions_run.  regions: dicts with reference (str), region_begin, records [(pos0, ref, [alts], info)],
    d_planes / d_meta / d_items (device pointers as int), plane_stride, n_reads, n_items and optionally region_end, add_all_variants,
    vcf_begin, vcf_end, filter_zero_qual.  Built once (the conversion of the records is the caller's staging), run any number of times."""

    def __init__(self, regions):
        self.n = len(regions)
        self.jobs = (RegionJob * max(self.n, 1))()
        self.keep = []
        for k, r in enumerate(regions):
            recs, keep = records_array(r["records"])
            refb = r["reference"].encode()
            self.keep.extend([recs, keep, refb])
            j = self.jobs[k]
            j.reference, j.reference_len = refb, len(refb)
            j.region_begin, j.region_end = r["region_begin"], r.get("region_end", 0xFFFFFFFF)
            j.records, j.n_records = recs, len(r["records"])
            j.add_all_variants = int(r.get("add_all_variants", False))
            j.d_planes, j.plane_stride, j.d_meta, j.n_reads = r["d_planes"], r["plane_stride"], r["d_meta"], r["n_reads"]
            j.d_items, j.n_items = r["d_items"], r["n_items"]
            j.vcf_begin, j.vcf_end = r.get("vcf_begin", 0), r.get("vcf_end", 0xFFFFFFFF)
            j.filter_zero_qual = int(r.get("filter_zero_qual", False))

    def run(self, sample_names, contig="chr1", device=0, rec_words=8, conn_cap=1 << 16, builders=0, device_threads=0, text_threads=0, params=None):
        """gtx_regions_run -> ([text of job k as bytes, or None where the job failed], statistics as a dict); raises on the first failing job's status"""
        L = lib()
        names = (C.c_char_p * max(1, len(sample_names)))(*[n.encode() for n in sample_names])
        params = params or Params(75, 0, 0, 0, 0, 3840, 0, 0, 0)
        st = RegionsStats()
        rc = L.gtx_regions_run(self.jobs, self.n, C.byref(params), device, contig.encode(), names, len(sample_names), rec_words, conn_cap, builders,
                               device_threads, text_threads, C.byref(st))
        texts = [C.string_at(self.jobs[k].text, self.jobs[k].text_len) if self.jobs[k].text else None for k in range(self.n)]
        self.status = [int(self.jobs[k].status) for k in range(self.n)]
        self.texts = texts  # (kept for a caller that catches the first failing job's error: the other jobs have theirs)
        L.gtx_regions_free(self.jobs, self.n)
        check(rc)
        return texts, {k: getattr(st, k) for k, _ in RegionsStats._fields_ if k != "reserved"}


def tabix_build(vcf_gz, min_shift=0, index_path=None):
    """gtx_tabix_build: <vcf>.tbi (min_shift 0) or a .csi"""
    check(lib().gtx_tabix_build(vcf_gz.encode(), min_shift, index_path.encode() if index_path else None))


def tabix_start(vcf_gz, chrom, begin, end):
    """gtx_tabix_start -> virtual offset, or None when the index knows of no record there"""
    v, any_ = C.c_uint64(), C.c_int()
    check(lib().gtx_tabix_start(vcf_gz.encode(), chrom.encode(), begin, end, C.byref(v), C.byref(any_)))
    return int(v.value) if any_.value else None


def shrink_params(**kw):
    """gtx_shrink_params with the reference's defaults, fields overridden by keyword"""
    p = ShrinkParams()
    lib().gtx_shrink_params_default(C.byref(p))
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def bam_shrink(bam_in, intervals, bam_out, params=None):
    """gtx_bam_shrink; intervals: [(chrom, begin, end)] 0-based, both inside.  Returns the stats as a dict."""
    n = len(intervals)
    chroms = (C.c_char_p * n)(*[c.encode() for c, _, _ in intervals])
    begins = (C.c_int32 * n)(*[b for _, b, _ in intervals])
    ends = (C.c_int32 * n)(*[e for _, _, e in intervals])
    st = ShrinkStats()
    check(lib().gtx_bam_shrink(bam_in.encode(), chroms, begins, ends, n, C.byref(params) if params is not None else None, bam_out.encode(), C.byref(st)))
    return {k: int(getattr(st, k)) for k, _ in ShrinkStats._fields_}


def bam_shrink_multi(bam_in, interval_file, bam_out, params=None):
    """gtx_bam_shrink_multi: the intervals come from a file of 'contig first last' lines (1-based)"""
    st = ShrinkStats()
    check(lib().gtx_bam_shrink_multi(bam_in.encode(), interval_file.encode(), C.byref(params) if params is not None else None, bam_out.encode(), C.byref(st)))
    return {k: int(getattr(st, k)) for k, _ in ShrinkStats._fields_}


class VcfRequest(C.Structure):
    _fields_ = [("contig", C.c_char_p), ("sample_names", C.POINTER(C.c_char_p)), ("n_samples", C.c_uint32),
                ("region_begin", C.c_uint32), ("region_end", C.c_uint32), ("filter_zero_qual", C.c_int32),
                ("variant_suffix_id", C.c_char_p), ("gt_cov", C.c_void_p), ("stat_u64", C.c_void_p), ("stat_u32", C.c_void_p),
                ("phred", C.c_void_p), ("calls", C.c_void_p), ("sv_table", C.c_char_p), ("ref_depth", C.c_void_p), ("ref_depth_len", C.c_uint32)]


class Context:
    """gtx_ctx: flat graph + index (host) and, for device >= 0, their copies in HBM"""

    def __init__(self, graph, device=0, max_index_labels=75, is_sv_graph=False, hq_reads=False, force_both=False,
                 is_segment_calling=False, sam_flag_filter=3840, no_second_pass=False, big_record_words=0, exact_pass_mb=0,
                 max_read_len=0):
        L = lib()
        self.g = {k: np.ascontiguousarray(v) for k, v in graph.items()}
        g = self.g
        has_ev = len(g.get("event_val", ())) > 0
        self.view = GraphView(len(g["ref_order"]), len(g["var_order"]), _p(g["ref_order"]), _p(g["ref_len"]),
                              _p(g["ref_dna_off"]), _p(g["ref_nvar"]), _p(g["ref_first_var"]), _p(g["var_order"]),
                              _p(g["var_len"]), _p(g["var_dna_off"]), _p(g["var_out_ref"]), _p(g["dna"]), len(g["dna"]),
                              _p(g["event_off"]) if has_ev else None, _p(g["event_val"]) if has_ev else None)
        self.params = Params(max_index_labels, int(is_sv_graph), int(hq_reads), int(force_both), int(is_segment_calling),
                             sam_flag_filter, int(no_second_pass), int(big_record_words), int(exact_pass_mb), int(max_read_len))
        h = C.c_void_p()
        check(L.gtx_ctx_create(C.byref(self.view), C.byref(self.params), device, C.byref(h)))
        self.h = h
        self.device = device
        lay = ScoreLayout()
        check(L.gtx_ctx_score_layout(self.h, C.byref(lay)))
        self.n_hap, self.total_tri, self.total_allele = int(lay.n_hap), int(lay.total_tri), int(lay.total_allele)
        self.total_near = int(lay.total_near)
        self.ref_depth_len = int(lay.ref_depth_len)
        self.hap_order = np.zeros(self.n_hap, np.uint32)
        self.hap_cnum = np.zeros(self.n_hap, np.uint32)
        self.tri_off = np.zeros(self.n_hap, np.uint64)
        self.allele_off = np.zeros(self.n_hap, np.uint64)
        check(L.gtx_ctx_haplotypes(self.h, _p(self.hap_order), _p(self.hap_cnum), _p(self.tri_off), _p(self.allele_off)))
        self.near_last = np.zeros(self.n_hap, np.uint32)  # layout of the near-pair connection counters (d_conn_near)
        self.near_off = np.zeros(self.n_hap, np.uint64)
        check(L.gtx_ctx_near_pairs(self.h, _p(self.near_last), _p(self.near_off)))

    def close(self):
        if getattr(self, "h", None):
            lib().gtx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass

    def special_positions(self):
        L = lib()
        n = C.c_uint32()
        check(L.gtx_ctx_special_positions(self.h, C.byref(n), None, None, 0))
        rr, ap = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint32)
        check(L.gtx_ctx_special_positions(self.h, C.byref(n), _p(rr), _p(ap), n.value))
        return rr, ap

    def index_stats(self):
        nk, nl = C.c_uint64(), C.c_uint64()
        check(lib().gtx_index_stats(self.h, C.byref(nk), C.byref(nl)))
        return int(nk.value), int(nl.value)

    def index_get(self, key):
        out = np.zeros(4096, LABEL)
        n = C.c_uint32()
        check(lib().gtx_index_get(self.h, C.c_uint64(key), _p(out), 4096, C.byref(n)))
        return [tuple(int(x) for x in out[i]) for i in range(n.value)]

    def index_dump(self):
        nk, nl = self.index_stats()
        keys, counts, labels = np.zeros(nk, np.uint64), np.zeros(nk, np.uint32), np.zeros(nl, LABEL)
        check(lib().gtx_index_dump(self.h, _p(keys), _p(counts), _p(labels)))
        lab = np.stack([labels["start_index"], labels["end_index"], labels["variant_id"]], axis=1) if nl else np.zeros((0, 3), np.uint32)
        return keys, counts, lab

    def hint_table(self, which):
        """one table of the position-hinted pass as uint32 words (gtx_ctx_hint_table): 0 position flags, 1 reference planes,
        2 tail sites, 3 / 4 half-key filters, 5 allele windows (8 words each), 6 first window | count << 24 per reference node"""
        n = C.c_uint64()
        check(lib().gtx_ctx_hint_table(self.h, which, None, 0, C.byref(n)))
        out = np.zeros(n.value // 4, np.uint32)
        if n.value:
            check(lib().gtx_ctx_hint_table(self.h, which, _p(out), n.value, C.byref(n)))
        return out

    def profile(self):
        out = np.zeros(32, np.uint64)
        check(lib().gtx_ctx_profile(self.h, _p(out)))
        return out

    def profile_log(self, cap=1 << 16):
        """the general pass' task log of the profiling build: rows of 16 words (include/gtx.h: gtx_ctx_profile_log)"""
        out = np.zeros((cap, 16), np.uint64)
        n = C.c_uint64()
        check(lib().gtx_ctx_profile_log(self.h, _p(out), cap, C.byref(n)))
        return out[:n.value]

    def big_records(self):
        """(used part of the big-record arena as a host array, number of tasks the last align batch sent through the
        second pass)"""
        ptr, cap, used, tasks = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().gtx_ctx_big_records(self.h, C.byref(ptr), C.byref(cap), C.byref(used), C.byref(tasks)))
        return download(ptr.value or 0, np.uint32, int(used.value)), int(tasks.value)

    def exact_pass_tasks(self):
        """(tasks of the last align batch that went through the exact pass with a small part of its slab, again with a large part,
        again with the whole slab, tasks that keep a table-overflow status even so)"""
        out = (C.c_uint64 * 4)()
        check(lib().gtx_ctx_exact_pass_tasks(self.h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def long_pass_tasks(self):
        """(tasks of the last align batch that the long reads' tier 1 took, that went on to tier 2 with a small part of the exact
        pass' slab, again with a large part, again with the whole slab, tasks that keep a table-overflow status even so)"""
        out = (C.c_uint64 * 5)()
        check(lib().gtx_ctx_long_pass_tasks(self.h, out))
        return tuple(int(x) for x in out)

    def pass_times(self):
        """(ms of the express / general / HBM-table pass of the last align batch, tasks handed to the general pass);
        the first call only arms the timing"""
        ms = (C.c_float * 3)()
        q = C.c_uint32()
        check(lib().gtx_ctx_pass_times(self.h, ms, C.byref(q)))
        return [float(x) for x in ms], int(q.value)

    def kernel_times(self):
        """[(kernel, ms, forward tasks completed)] of the four launches of the last timed align batch"""
        ms, tasks = (C.c_float * 4)(), (C.c_uint32 * 4)()
        check(lib().gtx_ctx_kernel_times(self.h, ms, tasks))
        names = ("gtx_align_hinted_kernel", "gtx_align_express4_kernel", "gtx_align_kernel", "gtx_align_big_kernel")
        return [(n, float(m), int(t)) for n, m, t in zip(names, ms, tasks)]

    def rewind_big_records(self):
        check(lib().gtx_ctx_big_records_rewind(self.h, None))

    def vcf_records(self, contig, sample_names, gt_cov, stat_u64, stat_u32, phred, calls, region_begin=0, region_end=0xFFFFFFFF,
                    filter_zero_qual=False, variant_suffix_id=None, sv_table=None, ref_depth=None):
        """gtx_vcf_records: the VCF records (column line first) of the region's variant sites as bytes; all arrays are host copies.
        SV graphs: sv_table = the text of gtx_graph_sv_table, ref_depth = the FINALISED reference-depth rows [n_samples, ref_depth_len + 1]"""
        names = (C.c_char_p * max(1, len(sample_names)))(*[n.encode() for n in sample_names])
        keep = [np.ascontiguousarray(gt_cov, np.uint32), np.ascontiguousarray(stat_u64, np.uint64), np.ascontiguousarray(stat_u32, np.uint32),
                np.ascontiguousarray(phred, np.uint8), np.ascontiguousarray(calls, SAMPLE_CALL)]
        if ref_depth is not None:
            keep.append(np.ascontiguousarray(ref_depth, np.uint32))
            assert keep[-1].size == len(sample_names) * (self.ref_depth_len + 1)
        rq = VcfRequest(contig.encode(), names, len(sample_names), region_begin, region_end, int(filter_zero_qual),
                        variant_suffix_id.encode() if variant_suffix_id else None, *[C.c_void_p(a.ctypes.data) for a in keep[:5]],
                        sv_table.encode() if sv_table is not None else None, C.c_void_p(keep[5].ctypes.data) if ref_depth is not None else None,
                        self.ref_depth_len if ref_depth is not None else 0)
        n = C.c_uint64()
        check(lib().gtx_vcf_records(self.h, C.byref(rq), None, C.c_uint64(0), C.byref(n)))
        buf = C.create_string_buffer(int(n.value) + 1)
        check(lib().gtx_vcf_records(self.h, C.byref(rq), buf, C.c_uint64(n.value), C.byref(n)))
        return buf.raw[:int(n.value)]

    def vcf_records_final(self, contig, sample_names, gt_cov, stat_u64, stat_u32, phred, calls, region_begin=0, region_end=0xFFFFFFFF,
                          filter_zero_qual=False, variant_suffix_id=None, no_variant_overlapping=False, no_filter_bad_alts=False):
        """gtx_vcf_records_final: the records (column line first) of the file genotype() ends with -- vcf_merge_and_break with the
        variants broken down"""
        names = (C.c_char_p * max(1, len(sample_names)))(*[n.encode() for n in sample_names])
        keep = [np.ascontiguousarray(gt_cov, np.uint32), np.ascontiguousarray(stat_u64, np.uint64), np.ascontiguousarray(stat_u32, np.uint32),
                np.ascontiguousarray(phred, np.uint8), np.ascontiguousarray(calls, SAMPLE_CALL)]
        rq = VcfRequest(contig.encode(), names, len(sample_names), region_begin, region_end, int(filter_zero_qual),
                        variant_suffix_id.encode() if variant_suffix_id else None, *[C.c_void_p(a.ctypes.data) for a in keep], None, None, 0)
        n = C.c_uint64()
        args = (self.h, C.byref(rq), int(no_variant_overlapping), int(no_filter_bad_alts))
        check(lib().gtx_vcf_records_final(*args, None, C.c_uint64(0), C.byref(n)))
        buf = C.create_string_buffer(int(n.value) + 1)
        check(lib().gtx_vcf_records_final(*args, buf, C.c_uint64(n.value), C.byref(n)))
        return buf.raw[:int(n.value)]

    def vcf_sites(self, contig, n_samples, gt_cov, stat_u64, stat_u32, phred, calls, ph_rows):
        """gtx_vcf_sites: the sites-only VCF records (column line first) of the alleles the next iteration keeps, with their GT_ID /
        GT_ANTI_HAPLOTYPE / GT_HAPLOTYPE tags; ph_rows = what phase_flags returned"""
        names = (C.c_char_p * max(1, n_samples))(*[b"S%d" % i for i in range(n_samples)])
        keep = [np.ascontiguousarray(gt_cov, np.uint32), np.ascontiguousarray(stat_u64, np.uint64), np.ascontiguousarray(stat_u32, np.uint32),
                np.ascontiguousarray(phred, np.uint8), np.ascontiguousarray(calls, SAMPLE_CALL)]
        rq = VcfRequest(contig.encode(), names, n_samples, 0, 0xFFFFFFFF, 0, None, *[C.c_void_p(a.ctypes.data) for a in keep], None, None, 0)
        ph = np.zeros(len(ph_rows), PHASE_ENTRY)
        for k, f in enumerate(("hap1", "allele1", "hap2", "allele2", "flags")):
            ph[f] = np.asarray(ph_rows)[:, k] if len(ph_rows) else 0
        n = C.c_uint64()
        check(lib().gtx_vcf_sites(self.h, C.byref(rq), _p(ph), C.c_uint64(len(ph)), None, C.c_uint64(0), C.byref(n)))
        buf = C.create_string_buffer(int(n.value) + 1)
        check(lib().gtx_vcf_sites(self.h, C.byref(rq), _p(ph), C.c_uint64(len(ph)), buf, C.c_uint64(n.value), C.byref(n)))
        return buf.raw[:int(n.value)]

    def phase_flags(self, n_samples, gt_cov, conn_log, n_conn, conn_near=None):
        """gtx_phase_flags: rows (hap1, allele1, hap2, allele2, flags) as an int array [n, 5]"""
        gt_cov = np.ascontiguousarray(gt_cov, np.uint32)
        conn_log = np.ascontiguousarray(conn_log, np.uint32)
        if conn_near is not None:
            conn_near = np.ascontiguousarray(conn_near, np.uint32)
            assert len(conn_near) == n_samples * self.total_near
        n = C.c_uint64()
        cap = 1024
        while True:
            out = np.zeros(cap, PHASE_ENTRY)
            rc = lib().gtx_phase_flags(self.h, n_samples, _p(gt_cov), _p(conn_log), C.c_uint64(n_conn),
                                       _p(conn_near) if conn_near is not None else None, _p(out), C.c_uint64(cap), C.byref(n))
            if rc == 5 and n.value > cap:  # GTX_ERR_CAPACITY
                cap = int(n.value)
                continue
            check(rc)
            out = out[:n.value]
            return np.stack([out["hap1"], out["allele1"], out["hap2"], out["allele2"], out["flags"]], axis=1).astype(np.int64)

    def error_count(self):
        n = C.c_uint32()
        check(lib().gtx_ctx_error_count(self.h, C.byref(n)))
        return int(n.value)


class Stream:
    """gtx_stream: which records align, which reuse the previous alignment, which pairs / reads get scored"""

    def __init__(self, params, n_read_groups=1):
        h = C.c_void_p()
        check(lib().gtx_stream_create(C.byref(params), n_read_groups, C.byref(h)))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None):
            lib().gtx_stream_destroy(self.h)
            self.h = None

    def set_planes(self, plane_stride):
        """gtx_stream_set_planes: push() then returns plane rows of that pitch (0: BAM nibble rows again)"""
        check(lib().gtx_stream_set_planes(self.h, plane_stride))
        self.plane_stride = plane_stride

    def push(self, recs, seq):
        """recs: STREAM_RECORD array, seq: [n, stride] packed bases -> (align_seq, align_meta, items)"""
        recs = np.ascontiguousarray(recs, STREAM_RECORD)
        seq = np.ascontiguousarray(seq, np.uint8)
        n, stride = seq.shape
        a_seq = np.zeros((n, getattr(self, "plane_stride", 0) or stride), np.uint8)
        a_meta = np.zeros(n, READ_META)
        items = np.zeros(n, SCORE_ITEM)
        na, ni = C.c_uint32(), C.c_uint32()
        check(lib().gtx_stream_push(self.h, _p(recs), _p(seq), stride, n, _p(a_seq), _p(a_meta), n, C.byref(na), _p(items), n,
                                    C.byref(ni)))
        return a_seq[:na.value], a_meta[:na.value], items[:ni.value]

    def push_packed(self, recs, seq, packed_stride):
        """push() with the tasks' bases as packed rows: recs, seq: [n, stride] packed bases -> (rows, exc_start, exc, align_meta,
        items), exc_start with one entry per row and one behind the last"""
        recs = np.ascontiguousarray(recs, STREAM_RECORD)
        seq = np.ascontiguousarray(seq, np.uint8)
        n, stride = seq.shape
        rows = np.zeros((n, packed_stride), np.uint8)
        exc_start = np.zeros(n + 1, np.uint32)
        exc = np.zeros(max(1, n * min(4 * packed_stride, 2 * stride)), np.uint16)  # (room for every base of every record)
        a_meta = np.zeros(n, READ_META)
        items = np.zeros(n, SCORE_ITEM)
        ne, na, ni = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().gtx_stream_push_packed(self.h, _p(recs), _p(seq), stride, n, _p(rows), packed_stride, _p(exc_start), _p(exc), len(exc),
                                           C.byref(ne), _p(a_meta), n, C.byref(na), _p(items), n, C.byref(ni)))
        return rows[:na.value], exc_start[:na.value + 1], exc[:ne.value], a_meta[:na.value], items[:ni.value]

    def set_coverage(self, avg_cov_by_readlen):
        a = np.ascontiguousarray(avg_cov_by_readlen, np.float64)
        check(lib().gtx_stream_set_coverage(self.h, _p(a), len(a)))

    def finish(self):
        """end of the stream -> leftover items (SV calling), parked reads are forgotten"""
        cap = max(self.counts()["parked"], 1)
        items = np.zeros(cap, SCORE_ITEM)
        ni = C.c_uint32()
        check(lib().gtx_stream_finish(self.h, _p(items), cap, C.byref(ni)))
        return items[:ni.value]

    def counts(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().gtx_stream_counts(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(records=int(a.value), duplicated=int(b.value), parked=int(c.value))


class DeviceStream:
    """gtx_dstream: gtx_stream's decisions for records that are in device memory, the outputs left there (no SV graphs)"""

    def __init__(self, params, n_read_groups=1, device=0, max_batch=1 << 16, parked_cap=1 << 16):
        h = C.c_void_p()
        check(lib().gtx_dstream_create(C.byref(params), n_read_groups, device, max_batch, parked_cap, C.byref(h)))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None):
            lib().gtx_dstream_destroy(self.h)
            self.h = None

    def push_raw(self, d_recs, d_seq, seq_stride, n, d_planes, plane_stride, d_meta, align_cap, d_items, item_cap, stream=None):
        """device pointers in and out -> (status, n_align, n_items); nothing is raised"""
        na, ni = C.c_uint32(), C.c_uint32()
        rc = lib().gtx_dstream_push(self.h, d_recs, d_seq, seq_stride, n, d_planes, plane_stride, d_meta, align_cap, d_items, item_cap, C.byref(na), C.byref(ni), stream)
        return rc, int(na.value), int(ni.value)

    def push(self, recs, seq, plane_stride, stream=None):
        """recs: a uint8 torch tensor on the device holding n STREAM_RECORD, seq: a uint8 tensor [n, seq_stride] of packed bases there ->
        (planes [n_align, plane_stride], meta [n_align * 20 bytes], items [n_items * 40 bytes]) as uint8 tensors on the device"""
        import torch
        n, seq_stride = seq.shape
        assert recs.numel() == n * STREAM_RECORD.itemsize and recs.is_contiguous() and seq.is_contiguous()
        planes = torch.empty((max(n, 1), plane_stride), dtype=torch.uint8, device=seq.device)
        meta = torch.empty(max(n, 1) * READ_META.itemsize, dtype=torch.uint8, device=seq.device)
        items = torch.empty(max(n, 1) * SCORE_ITEM.itemsize, dtype=torch.uint8, device=seq.device)
        if stream is None:
            torch.cuda.current_stream().synchronize()  # (the tensors above and the caller's are made on torch's stream; the push runs on the null stream)
        rc, na, ni = self.push_raw(recs.data_ptr(), seq.data_ptr(), seq_stride, n, planes.data_ptr(), plane_stride, meta.data_ptr(), n, items.data_ptr(), n, stream)
        check(rc)
        return planes[:na], meta[:na * READ_META.itemsize], items[:ni * SCORE_ITEM.itemsize]

    def finish(self, stream=None):
        """end of the stream: the parked mates are forgotten"""
        check(lib().gtx_dstream_finish(self.h, stream))

    def counts(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().gtx_dstream_counts(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(records=int(a.value), duplicated=int(b.value), parked=int(c.value))


REC_WIDE, WIDE_MASK_WORDS = 0x40000000, 80  # include/gtx.h: GTX_REC_WIDE, GTX_WIDE_MASK_WORDS


TASK_HAS_VARIANTS, TASK_COMPACT, COMPACT_WORDS = 1, 2, 8
WORK_HEADER_WORDS = 4  # GTX_WORK_HEADER_WORDS: gtx_align_batch_planes_triaged's queue starts behind them
TRIAGE_ITEMS_ARE_READS = 1  # GTX_TRIAGE_ITEMS_ARE_READS
REPLAY_ENTRY = np.dtype([("item", np.uint32), ("cell", np.uint32), ("order_eps", np.uint32), ("mask_lo", np.uint32), ("mask_hi", np.uint32), ("pad", np.uint32)])


def merge_compact(records, compact, task_flags, n_reads, rec_words):
    """the records of gtx_align_batch_planes_compact as gtx_align_batch would have left them: a task whose byte of the side array
    carries GTX_TASK_COMPACT has its record in `compact` (8 words per read) and an untouched slot -> a copy with those records in
    their slots (host arrays; what parse_records and the tests' comparisons read)"""
    out = np.array(records, np.uint32).reshape(n_reads * 2, rec_words)
    comp = np.asarray(compact, np.uint32).reshape(-1, COMPACT_WORDS)[:n_reads]
    fl = np.asarray(task_flags, np.uint8).reshape(-1)[:2 * n_reads]
    which = np.nonzero(fl[0::2] & TASK_COMPACT)[0]
    assert not (fl[1::2] & TASK_COMPACT).any(), "only forward records are compact"
    out[2 * which, :COMPACT_WORDS] = comp[which]
    out[2 * which, COMPACT_WORDS:] = 0
    return out.reshape(-1)


def parse_records(words, n_reads, rec_words, hap_order, big_records=None):
    """decode gtx_align_batch records into the same structure tests/oracle_lib.parse_path_stream returns
    (plus 'status', with the GTX_ST_EXTERNAL bit removed); Path::var_order is looked up through hap_order.
    big_records: the context's big-record arena (needed when a record carries GTX_ST_EXTERNAL)"""
    words = np.asarray(words, np.uint32).reshape(n_reads * 2, rec_words)
    out = []
    for i in range(n_reads):
        pair = []
        for o in range(2):
            w = words[2 * i + o]
            npaths, status = int(w[0]) & 0xFFFF, int(w[0]) >> 16
            longest, rlen = int(w[1]) & 0xFFFF, (int(w[1]) >> 16) & 0x3FFF  # (bit 31: REC_HAS_VARIANTS, bit 30: REC_WIDE)
            mw = WIDE_MASK_WORDS if int(w[1]) & REC_WIDE else 2
            k = 2
            if status & ST_EXTERNAL:
                w, k = big_records, int(w[2])
                status &= ~ST_EXTERNAL
            paths = []
            for _ in range(npaths):
                st, en, rsre, mmnv = int(w[k]), int(w[k + 1]), int(w[k + 2]), int(w[k + 3])
                k += 4
                vs = []
                for _v in range(mmnv >> 16):
                    hap = int(w[k])
                    alleles = tuple(32 * x + a for x in range(mw) if w[k + 1 + x] for a in range(32) if (int(w[k + 1 + x]) >> a) & 1)
                    k += 1 + mw
                    vs.append((int(hap_order[hap]), alleles))
                paths.append(dict(start=st, end=en, rs=rsre & 0xFFFF, re=rsre >> 16, mm=mmnv & 0xFFFF, vars=vs))
            pair.append(dict(longest=longest, paths=paths, status=status, read_len=rlen))
        out.append(tuple(pair))
    return out
