"""ctypes loader for libbfqhip.so (the HIP kernels + C-ABI of include/bfqzip_hip.h).

There is no CPU fallback: if the library is missing it is built (hipcc), and
if it cannot be loaded or no GPU is present the caller gets an exception.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbfqhip.so")
_LIB = None

SYMBOLS = [
    "bfq_default_params", "bfq_create", "bfq_create_error", "bfq_destroy", "bfq_set_params",
    "bfq_last_error", "bfq_stream", "bfq_device_count", "bfq_pick_device", "bfq_device_lease", "bfq_device_release",
    "bfq_phase_enable", "bfq_phase", "bfq_phase_report", "bfq_output_prefault", "bfq_fastq_rows_estimate", "bfq_build_ebwt", "bfq_count_reads",
    "bfq_smooth_invert", "bfq_run_reads", "bfq_run_reads_device", "bfq_fetch_ebwt",
    "bfq_fastq_out_bound", "bfq_fastq_build_ebwt", "bfq_fastq_run", "bfq_fastq_run_streams",
    "bfq_smooth_invert_fastq", "bfq_fastq_run_job", "bfq_fastq_run_job_edits", "bfq_host_alloc", "bfq_host_free",
    "bfq_text_count_lines", "bfq_text_nth_newline", "bfq_file_put", "bfq_file_map", "bfq_file_unmap", "bfq_fastq_build_ebwt_fd", "bfq_smooth_invert_fastq_fd",
    "bfq_glob_begin", "bfq_glob_local_text", "bfq_glob_pile_counts", "bfq_glob_init_out", "bfq_glob_run_pile", "bfq_glob_finish",
    "bfq_synth_default", "bfq_synth_total", "bfq_synth_host", "bfq_synth_device", "bfq_synth_fastq",
    "bfq_posbin_geometry", "bfq_posbin_sparse_last", "bfq_radix_geometry", "bfq_refine_form", "bfq_prof_enable", "bfq_prof_reset", "bfq_prof_count", "bfq_prof_get", "bfq_prof_trace_select", "bfq_prof_trace",
    "bfq_stream_bound", "bfq_stream_raw_len", "bfq_stream_compress", "bfq_stream_decompress",
    "bfq_stream_reserve", "bfq_stream_compress_device", "bfq_stream_ebwt_decode",
    "bfq_names_compress", "bfq_names_compress_device",
    "bfq_quals_compress", "bfq_quals_compress_device",
    "bfq_fastq_restore_bound", "bfq_fastq_restore", "bfq_fastq_restore_fd",
    "bfq_reorder_key", "bfq_fastq_reorder", "bfq_fastq_reorder_fd",
    "bfq_perm_bound", "bfq_perm_reads", "bfq_perm_encode", "bfq_perm_decode",
    "bfq_fastq_reorder_keep", "bfq_fastq_reorder_keep_fd", "bfq_fastq_unreorder", "bfq_fastq_unreorder_fd",
    "bfq_fastq_restore_ordered", "bfq_fastq_restore_ordered_fd",
    "bfq_fastq_restore_groups", "bfq_stream_members", "bfq_fastq_restore_grouped", "bfq_fastq_restore_grouped_fd",
    "bfq_fastq_compare", "bfq_fastq_compare_fd",
    "bfq_edits_bound", "bfq_edits_member_len", "bfq_edits_info", "bfq_edits_encode", "bfq_edits_decode", "bfq_edits_host_error",
    "bfq_fastq_edits_host", "bfq_fastq_unedit_host", "bfq_edits_make_device", "bfq_edits_apply_device",
    "bfq_fastq_edits", "bfq_fastq_edits_device", "bfq_fastq_edits_fd", "bfq_fastq_unedit", "bfq_fastq_unedit_fd",
    "bfq_fastq_restore_edited", "bfq_fastq_restore_edited_fd",
    "bfq_fastq_kmers", "bfq_fastq_kmers_fd", "bfq_fastq_kmers_host", "bfq_kmers_host_error", "bfq_kmers_geometry",
    "bfq_bgzf_probe", "bfq_bgzf_index", "bfq_bgzf_inflate", "bfq_bgzf_inflate_device", "bfq_bgzf_inflate_fd",
    "bfq_bgzf_deflate_bound", "bfq_bgzf_deflate_host", "bfq_bgzf_deflate", "bfq_bgzf_deflate_device", "bfq_bgzf_deflate_fd",
    "bfq_fastq_restore_bgzf_fd",
    "bfq_gzip_probe", "bfq_gzip_measure", "bfq_gzip_inflate", "bfq_gzip_inflate_device", "bfq_gzip_inflate_fd", "bfq_gzip_inflate_host",
    "bfq_gzip_host_error",
    "bfq_bam_default_opts", "bfq_bam_probe", "bfq_bam_measure", "bfq_bam_to_fastq", "bfq_bam_to_fastq_device", "bfq_bam_to_fastq_fd",
    "bfq_bam_to_fastq_host", "bfq_bam_host_error",
    "bfq_bam_patch_host", "bfq_bam_patch_device", "bfq_bam_patch", "bfq_bam_patch_fd",
    "bfq_ubam_default_opts", "bfq_fastq_to_bam_measure", "bfq_fastq_to_bam_host", "bfq_ubam_host_error", "bfq_fastq_to_bam_device", "bfq_fastq_to_bam",
    "bfq_fastq_to_bam_fd", "bfq_fastq_restore_bam_fd",
    "bfq_pairs_default_opts", "bfq_pairs_host_error",
    "bfq_fastq_deinterleave_measure", "bfq_fastq_deinterleave", "bfq_fastq_deinterleave_device", "bfq_fastq_deinterleave_fd", "bfq_fastq_deinterleave_host",
    "bfq_fastq_interleave_measure", "bfq_fastq_interleave", "bfq_fastq_interleave_device", "bfq_fastq_interleave_fd", "bfq_fastq_interleave_host",
    "bfq_repair_default_opts", "bfq_fastq_repair_measure", "bfq_fastq_repair", "bfq_fastq_repair_device", "bfq_fastq_repair_fd", "bfq_fastq_repair_host",
    "bfq_dedup_default_opts", "bfq_dedup_host_error", "bfq_fastq_dedup_measure", "bfq_fastq_dedup", "bfq_fastq_dedup_device", "bfq_fastq_dedup_fd", "bfq_fastq_dedup_host",
    "bfq_workspace_bytes", "bfq_workspace_read", "bfq_version",
]


class Params(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("K", "m", "v", "f", "t", "term", "M", "B", "ext", "piles", "ws_cap_mib")] + \
               [("reserved", C.c_int32 * 5)]


class Stats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in (
        "num_clust", "num_clust_discarded", "num_clust_amb_discarded", "num_clust_mod",
        "num_clust_alleq", "bases_inside", "qs_smoothed", "modified",
        "n_rows", "n_reads", "n_segments", "n_big_segments")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Synth(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("N", C.c_uint64), ("Lmin", C.c_uint32), ("Lmax", C.c_uint32),
                ("coverage", C.c_uint32), ("err_ppm", C.c_uint32), ("n_ppm", C.c_uint32),
                ("snp_every", C.c_uint32), ("dsnp_every", C.c_uint32), ("both_strands", C.c_uint32),
                ("first", C.c_uint64), ("collection", C.c_uint64), ("reserved", C.c_uint32 * 2)]


MAX_PARTS = 4


class TextPart(C.Structure):
    _fields_ = [("data", C.c_void_p), ("len", C.c_uint64)]


class ReorderOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("k", C.c_int32), ("seed", C.c_uint64), ("reserved", C.c_uint64 * 2)]


class RestoreGroup(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("dna_off", "dna_len", "qs_off", "qs_len", "hdr_off", "hdr_len", "raw_stream", "raw_hdr",
                                          "reads", "text_bound")]


class BgzfMember(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("in_len", C.c_uint32), ("out_len", C.c_uint32)]


class GzipStats(C.Structure):
    """bfq_gzip_stats: members, pieces, decoders started, decoders of the chain, candidates the chain ran past, decoders discarded"""
    _fields_ = [(k, C.c_uint64) for k in ("members", "pieces", "decoders", "chain", "skipped", "discarded")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "GzipStats(%s)" % ", ".join("%s=%d" % kv for kv in self.as_dict().items())


class BamOpts(C.Structure):
    """bfq_bam_opts: exclude_flags, mate_suffix, default_qual, split, paired_check, piece (0: the default), check_names (bfq_bam_patch* only)"""
    _fields_ = [(k, C.c_uint32) for k in ("exclude_flags", "mate_suffix", "default_qual", "split", "paired_check", "piece", "check_names", "reserved")]


class BamStats(C.Structure):
    """bfq_bam_stats: records of the file, written[3], skipped, reversed, no_qual, clamped_quals, n_ref, header_bytes, pieces, walkers,
    dead, repaired, rounds"""
    _fields_ = [("records", C.c_uint64), ("written", C.c_uint64 * 3)] + [(k, C.c_uint64) for k in (
        "skipped", "reversed", "no_qual", "clamped_quals", "n_ref", "header_bytes", "pieces", "walkers", "dead", "repaired", "rounds")]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["written"] = [int(v) for v in self.written]
        return {k: v if k == "written" else int(v) for k, v in d.items()}

    def __repr__(self):
        return "BamStats(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


class BamTagStats(C.Structure):
    """bfq_bam_tag_stats: tags_written, tags_dropped, tag_bytes (of text)"""
    _fields_ = [(k, C.c_uint64) for k in ("tags_written", "tags_dropped", "tag_bytes")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "BamTagStats(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


BAM_OPTS_TAGS = 0x31474154                                         # BFQ_BAM_OPTS_TAGS: o.reserved of a BamTagOpts


class BamTagOpts(C.Structure):
    """bfq_bam_tag_opts: o (a BamOpts whose reserved holds BAM_OPTS_TAGS), n_tags (0: every tag), strict, tag[32][2], stats"""
    _fields_ = [("o", BamOpts), ("n_tags", C.c_uint32), ("strict", C.c_uint32), ("tag", (C.c_uint8 * 2) * 32), ("stats", C.POINTER(BamTagStats))]


class BamPatchStats(C.Structure):
    """bfq_bam_patch_stats: records of the file, patched[3], skipped, reversed, reads_changed, bases_changed, quals_changed, unknown_bases,
    kept_high_quals, kept_absent, raw_len, pieces, repaired"""
    _fields_ = [("records", C.c_uint64), ("patched", C.c_uint64 * 3)] + [(k, C.c_uint64) for k in (
        "skipped", "reversed", "reads_changed", "bases_changed", "quals_changed", "unknown_bases", "kept_high_quals", "kept_absent", "raw_len", "pieces",
        "repaired")]

    def as_dict(self):
        return {k: [int(v) for v in self.patched] if k == "patched" else int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "BamPatchStats(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


class UbamOpts(C.Structure):
    """bfq_ubam_opts: mate_suffix, paired_check, level, reserved; header_text / header_len (NULL: the default header); rg_id (NULL: no tag)"""
    _fields_ = [(k, C.c_uint32) for k in ("mate_suffix", "paired_check", "level", "reserved")] + [
        ("header_text", C.c_void_p), ("header_len", C.c_uint64), ("rg_id", C.c_char_p)]


class UbamStats(C.Structure):
    """bfq_ubam_stats: records, written[3], named, comments_dropped, unknown_bases, raw_len, members"""
    _fields_ = [("records", C.c_uint64), ("written", C.c_uint64 * 3)] + [(k, C.c_uint64) for k in (
        "named", "comments_dropped", "unknown_bases", "raw_len", "members")]

    def as_dict(self):
        return {k: [int(v) for v in self.written] if k == "written" else int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "UbamStats(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


class UbamTagStats(C.Structure):
    """bfq_ubam_tag_stats: tags_written, fields_dropped, tag_bytes (of stream)"""
    _fields_ = [(k, C.c_uint64) for k in ("tags_written", "fields_dropped", "tag_bytes")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "UbamTagStats(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


UBAM_OPTS_TAGS = 0x32474154                                        # BFQ_UBAM_OPTS_TAGS: o.reserved of a UbamTagOpts


class UbamTagOpts(C.Structure):
    """bfq_ubam_tag_opts: o (a UbamOpts whose reserved holds UBAM_OPTS_TAGS), n_tags (0: every field), pad, tag[32][2], stats"""
    _fields_ = [("o", UbamOpts), ("n_tags", C.c_uint32), ("pad", C.c_uint32), ("tag", (C.c_uint8 * 2) * 32), ("stats", C.POINTER(UbamTagStats))]


class PairsOpts(C.Structure):
    """bfq_pairs_opts: check_names, mate_suffix, orphans, reserved (must be 0)"""
    _fields_ = [(k, C.c_uint32) for k in ("check_names", "mate_suffix", "orphans", "reserved")]


class PairsStats(C.Structure):
    """bfq_pairs_stats: records, pairs, singles, out_len[3]"""
    _fields_ = [(k, C.c_uint64) for k in ("records", "pairs", "singles")] + [("out_len", C.c_uint64 * 3)]

    def as_dict(self):
        return {k: [int(v) for v in self.out_len] if k == "out_len" else int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "PairsStats(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


class RepairOpts(C.Structure):
    """bfq_repair_opts: mate_suffix, hash_bits (1..40), seed, reserved[2] (must be 0)"""
    _fields_ = [("mate_suffix", C.c_uint32), ("hash_bits", C.c_uint32), ("seed", C.c_uint64), ("reserved", C.c_uint32 * 2)]


class RepairStats(C.Structure):
    """bfq_repair_stats: records, pairs, singles, out_len[3], n_in[3], dup_groups, mixed_runs, max_run"""
    _fields_ = ([(k, C.c_uint64) for k in ("records", "pairs", "singles")] + [("out_len", C.c_uint64 * 3), ("n_in", C.c_uint64 * 3)] +
                [(k, C.c_uint64) for k in ("dup_groups", "mixed_runs", "max_run")])

    def as_dict(self):
        return {k: [int(v) for v in getattr(self, k)] if k in ("out_len", "n_in") else int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "RepairStats(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


class DedupOpts(C.Structure):
    """bfq_dedup_opts: keep (0: the first unit of a group, 1: the best qualities), hash_bits (1..40), seed, reserved[2] (must be 0)"""
    _fields_ = [("keep", C.c_uint32), ("hash_bits", C.c_uint32), ("seed", C.c_uint64), ("reserved", C.c_uint32 * 2)]


class DedupStats(C.Structure):
    """bfq_dedup_stats: units, kept, removed, dup_groups, max_group, max_group_first, level_groups[32], level_units[32], out_len[2],
    dup_len[2], mixed_runs, max_run, rounds"""
    _fields_ = ([(k, C.c_uint64) for k in ("units", "kept", "removed", "dup_groups", "max_group", "max_group_first")] +
                [("level_groups", C.c_uint64 * 32), ("level_units", C.c_uint64 * 32), ("out_len", C.c_uint64 * 2), ("dup_len", C.c_uint64 * 2)] +
                [(k, C.c_uint64) for k in ("mixed_runs", "max_run", "rounds")])

    def as_dict(self):
        return {k: [int(v) for v in getattr(self, k)] if hasattr(getattr(self, k), "__len__") else int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "DedupStats(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


CMP_SYMS = 6
CMP_POS = 512


class CompareDiff(C.Structure):
    _fields_ = [("read", C.c_uint64), ("pos", C.c_uint32), ("base_a", C.c_uint8), ("base_b", C.c_uint8), ("qual_a", C.c_uint8), ("qual_b", C.c_uint8)]


COMPARE_SCALARS = ("n_reads", "total_bases", "n_diffs", "reads_changed", "reads_bases_changed", "reads_quals_changed", "bases_changed",
                   "quals_changed", "quals_raised", "quals_lowered", "qual_abs_sum", "qual_sq_sum", "qual_abs_max", "first_changed_read",
                   "headers_same", "headers_dropped", "headers_changed")
COMPARE_ARRAYS = (("subst", CMP_SYMS * CMP_SYMS), ("qual_hist_a", 256), ("qual_hist_b", 256), ("changed_base_qual_hist", 256),
                  ("pos_len", CMP_POS), ("pos_bases", CMP_POS), ("pos_quals", CMP_POS), ("pos_abs", CMP_POS))


class CompareReport(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in COMPARE_SCALARS] + [(k, C.c_uint64 * n) for k, n in COMPARE_ARRAYS] + [("reserved", C.c_uint64 * 8)]


class EditStats(C.Structure):
    """bfq_edit_stats: reads, bases, edits, reads_touched, bytes (of the container)"""
    _fields_ = [(k, C.c_uint64) for k in ("reads", "bases", "edits", "reads_touched", "bytes")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}

    def __repr__(self):
        return "EditStats(%s)" % ", ".join("%s=%d" % kv for kv in self.as_dict().items())


class KmerOpts(C.Structure):
    """bfq_kmer_opts: k (8..31), solid (2..15), canonical, reserved (must be 0), part_records (0: what the memory allows)"""
    _fields_ = [(k, C.c_uint32) for k in ("k", "solid", "canonical", "reserved")] + [("part_records", C.c_uint64)]


class KmerEntry(C.Structure):
    _fields_ = [("kmer", C.c_uint64), ("count_a", C.c_uint32), ("count_b", C.c_uint32)]


KMER_SCALARS = ("k", "solid", "canonical", "n_partitions", "n_reads_a", "n_reads_b", "reads_short_a", "reads_short_b", "windows_a", "windows_b",
                "windows_skipped_a", "windows_skipped_b", "distinct_a", "distinct_b", "distinct_both", "only_a", "only_b", "occ_only_a",
                "occ_only_b", "distinct_changed", "n_listed")
KMER_ARRAYS = (("hist_a", 256), ("hist_b", 256), ("joint", 16 * 16), ("trans", 3 * 3))


class KmerReport(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in KMER_SCALARS] + [(k, C.c_uint64 * n) for k, n in KMER_ARRAYS] + [("reserved", C.c_uint64 * 8)]


class FastqJob(C.Structure):
    _fields_ = [("parts", C.POINTER(TextPart)), ("nparts", C.c_int32), ("keep_headers", C.c_int32),
                ("out_fastq", C.c_void_p), ("cap_fastq", C.c_uint64),
                ("out_dna", C.c_void_p), ("out_qs", C.c_void_p), ("cap_stream", C.c_uint64),
                ("out_hdr", C.c_void_p), ("cap_hdr", C.c_uint64),
                ("fastq_len", C.c_uint64), ("stream_len", C.c_uint64), ("hdr_len", C.c_uint64),
                ("n_reads", C.c_uint64), ("total_bases", C.c_uint64),
                ("part_reads", C.c_uint64 * (MAX_PARTS + 1)), ("part_fastq_off", C.c_uint64 * (MAX_PARTS + 1)),
                ("part_stream_off", C.c_uint64 * (MAX_PARTS + 1)), ("part_hdr_off", C.c_uint64 * (MAX_PARTS + 1)),
                ("compress_streams", C.c_int32), ("name_codec", C.c_int32),
                ("dna_bytes", C.c_uint64), ("qs_bytes", C.c_uint64), ("hdr_bytes", C.c_uint64),
                ("qual_codec", C.c_int32), ("reserved1", C.c_int32)]


class JobEdits(C.Structure):
    """bfq_job_edits: out_edits, cap_edits, edits_bytes (what bfq_fastq_run_job_edits takes beside the job)"""
    _fields_ = [("out_edits", C.c_void_p), ("cap_edits", C.c_uint64), ("edits_bytes", C.c_uint64)]


def build(clean=False):
    """Compile libbfqhip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    d = os.path.join(_HERE, "csrc")
    if clean:
        subprocess.check_call(["make", "-s", "-C", d, "clean"])
    subprocess.check_call(["make", "-s", "-j8", "-C", d, "all"])


def lib():
    global _LIB
    if _LIB is None:
        # torch bundles its own HIP/HSA runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7).
        # Two HIP runtimes in one process cannot both own the GPU, so when torch is installed it
        # is imported first and libbfqhip.so binds to the runtime torch already loaded.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            build()
        L = C.CDLL(LIB_PATH)
        L.bfq_create.restype = C.c_void_p
        L.bfq_create.argtypes = [C.c_int, C.POINTER(Params)]
        L.bfq_create_error.restype = C.c_char_p
        L.bfq_destroy.argtypes = [C.c_void_p]
        L.bfq_set_params.argtypes = [C.c_void_p, C.POINTER(Params)]
        L.bfq_last_error.restype = C.c_char_p
        L.bfq_last_error.argtypes = [C.c_void_p]
        L.bfq_stream.restype = C.c_void_p
        L.bfq_stream.argtypes = [C.c_void_p]
        L.bfq_version.restype = C.c_char_p
        L.bfq_workspace_bytes.restype = C.c_uint64
        L.bfq_workspace_bytes.argtypes = [C.c_void_p]
        L.bfq_workspace_read.restype = C.c_uint64
        L.bfq_workspace_read.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        L.bfq_synth_total.restype = C.c_uint64
        vp, u64 = C.c_void_p, C.c_uint64
        L.bfq_pick_device.argtypes = [C.c_char_p, C.c_int]
        L.bfq_device_lease.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double)]
        L.bfq_device_release.argtypes = [C.c_int]
        L.bfq_phase_enable.argtypes = [C.c_int]
        L.bfq_phase.argtypes = [C.c_char_p]
        L.bfq_phase_report.argtypes = [C.c_char_p]
        L.bfq_output_prefault.argtypes = [C.c_int, u64, u64]
        L.bfq_fastq_rows_estimate.restype = u64
        L.bfq_fastq_rows_estimate.argtypes = [C.c_int, u64]
        L.bfq_build_ebwt.argtypes = [vp, vp, vp, vp, u64, C.c_int, vp, vp, vp]
        L.bfq_count_reads.argtypes = [vp, u64, C.c_int, C.POINTER(u64)]
        L.bfq_smooth_invert.argtypes = [vp, vp, vp, vp, C.c_int, u64, vp, vp, vp, C.POINTER(Stats)]
        L.bfq_run_reads.argtypes = [vp, vp, vp, vp, u64, vp, vp, C.POINTER(Stats)]
        L.bfq_run_reads_device.argtypes = [vp, vp, vp, vp, u64, u64, vp, vp, C.POINTER(Stats)]
        L.bfq_fetch_ebwt.argtypes = [vp, vp, vp, vp]
        L.bfq_fastq_out_bound.restype = C.c_uint64
        L.bfq_fastq_out_bound.argtypes = [u64, u64, u64]
        L.bfq_fastq_build_ebwt.argtypes = [vp, vp, u64, C.c_int, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bfq_fastq_run.argtypes = [vp, vp, u64, C.c_int, vp, u64, C.POINTER(u64), C.POINTER(Stats)]
        L.bfq_fastq_run_streams.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64),
                                            C.POINTER(Stats)]
        L.bfq_smooth_invert_fastq.argtypes = [vp, vp, vp, vp, C.c_int, u64, vp, u64, vp, u64, C.POINTER(u64),
                                              C.POINTER(Stats)]
        L.bfq_fastq_run_job.argtypes = [vp, C.POINTER(FastqJob), C.POINTER(Stats)]
        L.bfq_fastq_run_job_edits.argtypes = [vp, C.POINTER(FastqJob), C.POINTER(JobEdits), C.POINTER(Stats)]
        L.bfq_glob_begin.argtypes = [vp, C.POINTER(TextPart), C.c_int, C.POINTER(u64), C.POINTER(u64)]
        L.bfq_glob_local_text.argtypes = [vp, vp, vp]
        L.bfq_glob_pile_counts.argtypes = [vp, vp, u64, vp]
        L.bfq_glob_init_out.argtypes = [vp, vp, vp, u64, vp, vp]
        L.bfq_glob_run_pile.argtypes = [vp, vp, vp, u64, C.c_int, C.c_int, vp, vp, C.POINTER(Stats)]
        L.bfq_glob_finish.argtypes = [vp, vp, vp, C.POINTER(FastqJob)]
        L.bfq_host_alloc.restype = vp
        L.bfq_host_alloc.argtypes = [u64]
        L.bfq_host_free.argtypes = [vp]
        L.bfq_text_count_lines.argtypes = [vp, u64, u64, vp, C.c_int]
        L.bfq_file_put.argtypes = [C.c_int, u64, vp, u64, C.c_int]
        L.bfq_file_map.restype = vp
        L.bfq_file_map.argtypes = [C.c_int, u64, u64, C.c_int]
        L.bfq_file_unmap.argtypes = [vp, u64, u64]
        L.bfq_text_nth_newline.restype = C.c_int64
        L.bfq_text_nth_newline.argtypes = [vp, u64, u64]
        L.bfq_synth_default.argtypes = [C.POINTER(Synth), u64, C.c_uint32]
        L.bfq_synth_total.argtypes = [C.POINTER(Synth)]
        L.bfq_synth_host.argtypes = [C.POINTER(Synth), vp, vp, vp]
        L.bfq_synth_device.argtypes = [vp, C.POINTER(Synth), vp, vp, vp]
        L.bfq_synth_fastq.argtypes = [vp, C.POINTER(Synth), vp, u64, C.POINTER(u64)]
        L.bfq_stream_bound.restype = u64
        L.bfq_stream_bound.argtypes = [u64]
        L.bfq_stream_raw_len.restype = C.c_int64
        L.bfq_stream_raw_len.argtypes = [vp, u64]
        L.bfq_stream_compress.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
        L.bfq_stream_decompress.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
        L.bfq_stream_reserve.argtypes = [vp, u64]
        L.bfq_names_compress.argtypes = [vp, vp, u64, C.c_uint32, vp, u64, C.POINTER(u64)]
        L.bfq_names_compress_device.argtypes = [vp, vp, u64, C.c_uint32, vp, u64, C.POINTER(u64)]
        L.bfq_quals_compress.argtypes = [vp, vp, u64, C.c_uint32, vp, u64, C.POINTER(u64)]
        L.bfq_quals_compress_device.argtypes = [vp, vp, u64, C.c_uint32, vp, u64, C.POINTER(u64)]
        L.bfq_stream_ebwt_decode.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bfq_fastq_restore_bound.restype = C.c_int64
        L.bfq_fastq_restore_bound.argtypes = [vp, u64, vp, u64, vp, u64]
        L.bfq_fastq_restore.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
        L.bfq_fastq_restore_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, C.POINTER(u64), C.POINTER(u64)]
        L.bfq_reorder_key.restype = u64
        L.bfq_reorder_key.argtypes = [vp, u64, C.c_int]
        L.bfq_fastq_reorder.argtypes = [vp, C.POINTER(TextPart), C.c_int, C.POINTER(ReorderOpts), C.POINTER(vp), C.POINTER(u64),
                                        C.POINTER(u64), vp, C.POINTER(u64)]
        L.bfq_fastq_reorder_fd.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(u64), C.c_int, C.POINTER(ReorderOpts), C.POINTER(C.c_int),
                                           C.POINTER(u64), C.POINTER(u64)]
        pu64, pint = C.POINTER(u64), C.POINTER(C.c_int)
        L.bfq_perm_bound.restype = u64
        L.bfq_perm_bound.argtypes = [u64]
        L.bfq_perm_reads.restype = C.c_int64
        L.bfq_perm_reads.argtypes = [vp, u64]
        L.bfq_perm_encode.argtypes = [vp, u64, C.POINTER(ReorderOpts), vp, u64, pu64]
        L.bfq_perm_decode.argtypes = [vp, u64, vp, u64, pu64, C.POINTER(ReorderOpts), pu64]
        L.bfq_fastq_reorder_keep.argtypes = [vp, C.POINTER(TextPart), C.c_int, C.POINTER(ReorderOpts), C.POINTER(vp), pu64, pu64, vp, u64, pu64, pu64]
        L.bfq_fastq_reorder_keep_fd.argtypes = [vp, pint, pu64, C.c_int, C.POINTER(ReorderOpts), pint, C.c_int, pu64, pu64, pu64]
        L.bfq_fastq_unreorder.argtypes = [vp, C.POINTER(TextPart), C.c_int, vp, u64, C.POINTER(vp), pu64, pu64, pu64]
        L.bfq_fastq_unreorder_fd.argtypes = [vp, pint, pu64, C.c_int, C.c_int, u64, pint, pu64, pu64]
        L.bfq_fastq_restore_ordered.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, pu64, pu64]
        L.bfq_fastq_restore_ordered_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, pu64, pu64]
        L.bfq_fastq_restore_groups.restype = C.c_int64
        L.bfq_fastq_restore_groups.argtypes = [vp, u64, vp, u64, vp, u64, C.POINTER(RestoreGroup), u64, C.c_char_p, C.c_int]
        L.bfq_stream_members.restype = C.c_int64
        L.bfq_stream_members.argtypes = [vp, u64]
        L.bfq_fastq_restore_grouped.argtypes = [vp, vp, u64, vp, u64, vp, u64, u64, u64, vp, u64, pu64, pu64]
        L.bfq_fastq_restore_grouped_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, u64, u64, u64, C.c_int, pu64, pu64]
        L.bfq_stream_compress_device.argtypes = [vp, vp, u64, vp, u64, C.POINTER(u64)]
        L.bfq_fastq_compare.argtypes = [vp, C.POINTER(TextPart), C.c_int, C.POINTER(TextPart), C.c_int, vp, u64, C.POINTER(CompareReport), vp, u64]
        L.bfq_fastq_compare_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.POINTER(CompareReport), vp, u64]
        pes = C.POINTER(EditStats)
        L.bfq_edits_bound.restype = u64
        L.bfq_edits_bound.argtypes = [u64, u64]
        L.bfq_edits_member_len.restype = C.c_int64
        L.bfq_edits_member_len.argtypes = [vp, u64]
        L.bfq_edits_info.argtypes = [vp, u64, pu64, pu64, pu64, pu64]
        L.bfq_edits_encode.argtypes = [vp, vp, u64, u64, u64, u64, u64, vp, u64, pu64]
        L.bfq_edits_decode.argtypes = [vp, u64, vp, vp, u64, pu64, pu64, pu64, pu64, pu64, pu64]
        L.bfq_edits_host_error.restype = C.c_char_p
        L.bfq_edits_host_error.argtypes = []
        L.bfq_fastq_edits_host.argtypes = [vp, u64, vp, u64, vp, u64, pu64, pes]
        L.bfq_fastq_unedit_host.argtypes = [vp, u64, vp, u64, vp, u64, pu64, pes]
        L.bfq_edits_make_device.argtypes = [vp, vp, vp, vp, u64, u64, vp, u64, pu64, pes]
        L.bfq_edits_apply_device.argtypes = [vp, vp, u64, vp, vp, u64, u64, C.c_int, pes]
        L.bfq_fastq_edits.argtypes = [vp, C.POINTER(TextPart), C.c_int, C.POINTER(TextPart), C.c_int, vp, u64, pu64, pes]
        L.bfq_fastq_edits_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, pu64, pes]
        L.bfq_fastq_edits_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, pu64, pes]
        L.bfq_fastq_unedit.argtypes = [vp, vp, u64, vp, u64, vp, u64, pu64, pes]
        L.bfq_fastq_unedit_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, pu64, pes]
        L.bfq_fastq_restore_edited.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, vp, u64, pu64, pu64]
        L.bfq_fastq_restore_edited_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, pu64, pu64]
        pko, pkr = C.POINTER(KmerOpts), C.POINTER(KmerReport)
        L.bfq_fastq_kmers.argtypes = [vp, C.POINTER(TextPart), C.c_int, C.POINTER(TextPart), C.c_int, pko, pkr, vp, u64]
        L.bfq_fastq_kmers_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, pko, pkr, vp, u64]
        L.bfq_fastq_kmers_host.argtypes = [vp, u64, vp, u64, pko, pkr, vp, u64]
        L.bfq_kmers_host_error.restype = C.c_char_p
        L.bfq_kmers_host_error.argtypes = []
        L.bfq_kmers_geometry.argtypes = [pu64, pu64, pu64]
        L.bfq_bgzf_probe.argtypes = [vp, u64]
        L.bfq_bgzf_index.argtypes = [vp, u64, C.POINTER(BgzfMember), u64, pu64, pu64, pu64]
        L.bfq_bgzf_inflate.argtypes = [vp, vp, u64, vp, u64, pu64]
        L.bfq_bgzf_inflate_device.argtypes = [vp, vp, u64, vp, u64, pu64]
        L.bfq_bgzf_inflate_fd.argtypes = [vp, C.c_int, u64, C.c_int, pu64]
        L.bfq_bgzf_deflate_bound.restype = u64
        L.bfq_bgzf_deflate_bound.argtypes = [u64]
        L.bfq_bgzf_deflate_host.argtypes = [vp, u64, C.c_int, vp, u64, pu64]
        L.bfq_bgzf_deflate.argtypes = [vp, vp, u64, C.c_int, vp, u64, pu64]
        L.bfq_bgzf_deflate_device.argtypes = [vp, vp, u64, C.c_int, vp, u64, pu64]
        L.bfq_bgzf_deflate_fd.argtypes = [vp, C.c_int, u64, C.c_int, C.c_int, pu64]
        pgs = C.POINTER(GzipStats)
        L.bfq_gzip_probe.argtypes = [vp, u64]
        L.bfq_gzip_measure.argtypes = [vp, vp, u64, u64, pu64, pu64, pgs]
        L.bfq_gzip_inflate.argtypes = [vp, vp, u64, u64, vp, u64, pu64, pgs]
        L.bfq_gzip_inflate_device.argtypes = [vp, vp, u64, u64, vp, u64, pu64, pgs]
        L.bfq_gzip_inflate_fd.argtypes = [vp, C.c_int, u64, u64, C.c_int, pu64, pgs]
        L.bfq_gzip_inflate_host.argtypes = [vp, u64, u64, vp, u64, pu64, pgs]
        L.bfq_gzip_host_error.restype = C.c_char_p
        L.bfq_gzip_host_error.argtypes = []
        # the options go by address: a BamOpts, or the BamTagOpts / UbamTagOpts that begins with one
        pbo, pbs, a3 = vp, C.POINTER(BamStats), C.POINTER(u64)
        L.bfq_bam_default_opts.restype = None
        L.bfq_bam_default_opts.argtypes = [C.POINTER(BamOpts)]
        L.bfq_bam_probe.argtypes = [vp, u64]
        L.bfq_bam_measure.argtypes = [vp, vp, u64, pbo, a3, a3, pbs]
        L.bfq_bam_to_fastq.argtypes = [vp, vp, u64, pbo, C.POINTER(vp), a3, a3, a3, pbs]
        L.bfq_bam_to_fastq_device.argtypes = [vp, vp, u64, pbo, C.POINTER(vp), a3, a3, a3, pbs]
        L.bfq_bam_to_fastq_fd.argtypes = [vp, C.c_int, u64, pbo, C.POINTER(C.c_int), a3, a3, pbs]
        L.bfq_bam_to_fastq_host.argtypes = [vp, u64, pbo, C.POINTER(vp), a3, a3, a3, pbs]
        L.bfq_bam_host_error.restype = C.c_char_p
        L.bfq_bam_host_error.argtypes = []
        pps, i3 = C.POINTER(BamPatchStats), C.POINTER(C.c_int)
        L.bfq_bam_patch_host.argtypes = [vp, u64, pbo, C.POINTER(vp), a3, vp, u64, pps]
        L.bfq_bam_patch_device.argtypes = [vp, vp, u64, pbo, C.POINTER(vp), a3, vp, u64, pu64, pps]
        L.bfq_bam_patch.argtypes = [vp, vp, u64, pbo, C.POINTER(vp), a3, C.c_int, vp, u64, pu64, pps]
        L.bfq_bam_patch_fd.argtypes = [vp, C.c_int, u64, pbo, i3, C.c_int, C.c_int, pu64, pps]
        puo, pus = vp, C.POINTER(UbamStats)
        L.bfq_ubam_default_opts.restype = None
        L.bfq_ubam_default_opts.argtypes = [C.POINTER(UbamOpts)]
        L.bfq_ubam_host_error.restype = C.c_char_p
        L.bfq_ubam_host_error.argtypes = []
        L.bfq_fastq_to_bam_measure.argtypes = [vp, C.POINTER(vp), a3, puo, pu64, a3, pus]
        L.bfq_fastq_to_bam_host.argtypes = [C.POINTER(vp), a3, puo, vp, u64, pu64, pus]
        L.bfq_fastq_to_bam_device.argtypes = [vp, C.POINTER(vp), a3, puo, vp, u64, pu64, pus]
        L.bfq_fastq_to_bam.argtypes = [vp, C.POINTER(vp), a3, puo, vp, u64, pu64, pus]
        L.bfq_fastq_to_bam_fd.argtypes = [vp, i3, puo, C.c_int, pu64, pus]
        L.bfq_fastq_restore_bam_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, u64, puo, C.c_int, pu64, pus]
        ppo, pps2 = C.POINTER(PairsOpts), C.POINTER(PairsStats)
        L.bfq_pairs_default_opts.restype = None
        L.bfq_pairs_default_opts.argtypes = [ppo]
        L.bfq_pairs_host_error.restype = C.c_char_p
        L.bfq_pairs_host_error.argtypes = []
        L.bfq_fastq_deinterleave_measure.argtypes = [vp, vp, u64, ppo, a3, a3, pps2]
        L.bfq_fastq_deinterleave.argtypes = [vp, vp, u64, ppo, C.POINTER(vp), a3, a3, a3, pps2]
        L.bfq_fastq_deinterleave_device.argtypes = [vp, vp, u64, ppo, C.POINTER(vp), a3, a3, a3, pps2]
        L.bfq_fastq_deinterleave_fd.argtypes = [vp, C.c_int, u64, ppo, i3, a3, a3, pps2]
        L.bfq_fastq_deinterleave_host.argtypes = [vp, u64, ppo, C.POINTER(vp), a3, a3, a3, pps2]
        L.bfq_fastq_interleave_measure.argtypes = [vp, C.POINTER(vp), a3, ppo, pu64, a3, pps2]
        L.bfq_fastq_interleave.argtypes = [vp, C.POINTER(vp), a3, ppo, vp, u64, pu64, pps2]
        L.bfq_fastq_interleave_device.argtypes = [vp, C.POINTER(vp), a3, ppo, vp, u64, pu64, pps2]
        L.bfq_fastq_interleave_fd.argtypes = [vp, i3, ppo, C.c_int, pu64, pps2]
        L.bfq_fastq_interleave_host.argtypes = [C.POINTER(vp), a3, ppo, vp, u64, pu64, pps2]
        pro, prs = C.POINTER(RepairOpts), C.POINTER(RepairStats)
        L.bfq_repair_default_opts.restype = None
        L.bfq_repair_default_opts.argtypes = [pro]
        L.bfq_fastq_repair_measure.argtypes = [vp, C.POINTER(vp), a3, pro, a3, a3, prs]
        L.bfq_fastq_repair.argtypes = [vp, C.POINTER(vp), a3, pro, C.POINTER(vp), a3, a3, a3, prs]
        L.bfq_fastq_repair_device.argtypes = [vp, C.POINTER(vp), a3, pro, C.POINTER(vp), a3, a3, a3, prs]
        L.bfq_fastq_repair_fd.argtypes = [vp, i3, pro, i3, a3, a3, prs]
        L.bfq_fastq_repair_host.argtypes = [C.POINTER(vp), a3, pro, C.POINTER(vp), a3, a3, a3, prs]
        pdo, pds, a2, i2 = C.POINTER(DedupOpts), C.POINTER(DedupStats), C.POINTER(u64), C.POINTER(C.c_int)
        L.bfq_dedup_default_opts.restype = None
        L.bfq_dedup_default_opts.argtypes = [pdo]
        L.bfq_dedup_host_error.restype = C.c_char_p
        L.bfq_dedup_host_error.argtypes = []
        L.bfq_fastq_dedup_measure.argtypes = [vp, C.POINTER(vp), a2, pdo, a2, a2, pds]
        L.bfq_fastq_dedup.argtypes = [vp, C.POINTER(vp), a2, pdo, C.POINTER(vp), a2, C.POINTER(vp), a2, a2, a2, pds]
        L.bfq_fastq_dedup_device.argtypes = [vp, C.POINTER(vp), a2, pdo, C.POINTER(vp), a2, C.POINTER(vp), a2, a2, a2, pds]
        L.bfq_fastq_dedup_fd.argtypes = [vp, i2, pdo, i2, i2, a2, a2, pds]
        L.bfq_fastq_dedup_host.argtypes = [C.POINTER(vp), a2, pdo, C.POINTER(vp), a2, C.POINTER(vp), a2, a2, a2, pds]
        L.bfq_fastq_restore_bgzf_fd.argtypes = [vp, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, u64, C.c_int, C.c_int, pu64, pu64, pu64]
        L.bfq_posbin_geometry.argtypes = [u64, C.POINTER(u64), C.POINTER(C.c_int)]
        L.bfq_posbin_sparse_last.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(u64)]
        L.bfq_radix_geometry.argtypes = [u64, C.POINTER(u64), C.POINTER(u64)]
        L.bfq_refine_form.argtypes = [vp]
        L.bfq_prof_enable.argtypes = [vp, C.c_int]
        L.bfq_prof_reset.argtypes = [vp]
        L.bfq_prof_count.argtypes = [vp]
        L.bfq_prof_trace_select.argtypes = [vp, C.c_int]
        L.bfq_prof_trace.restype = C.c_int64
        L.bfq_prof_trace.argtypes = [vp, vp, u64]
        L.bfq_prof_get.argtypes = [vp, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_double),
                                   C.POINTER(u64), C.POINTER(C.c_double)]
        _LIB = L
    return _LIB
