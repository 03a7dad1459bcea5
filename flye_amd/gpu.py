"""ctypes binding of libflyegpu.so + a host-side mirror of the reference's
``VertexIndex`` / ``OverlapDetector`` / ``OverlapContainer`` interface.

The reference is C++ and has no FFI; the binding a Flye
maintainer would add is the C++ stub in INTEGRATION.md.  This Python mirror keeps
the same names, argument meaning and error behaviour so that the parity tests read
like calls into the reference:

* ``VertexIndex.countKmers / buildIndexUnevenCoverage / buildIndexMinimizers /
  clear / getSampleRate``  (reference src/sequence/vertex_index.h:213-218, :260)
* ``OverlapDetector(...)`` ctor arguments (src/sequence/overlap.h:313-336)
* ``OverlapContainer.quickSeqOverlaps / lazySeqOverlaps /
  estimateOverlaperParameters / setDivergenceThreshold``
  (src/sequence/overlap.cpp:518-574, :744-827)
* ``BubbleProcessor(ctx, subs_matrix_path).polishAll(in_bubbles, out_consensus, log_path)``
  (src/polishing/bubble_processor.cpp:32-148; without the homopolymer matrix, which the reference never uses)
* ``BubbleMaker(ctx).make(contigs, alignments_by_contig, err_mode)`` / ``write_bubbles`` / ``uniform_alignments`` /
  ``polish``  (flye/polishing/bubbles.py:87-172 and alignment.py:95-153; alignment records instead of a SAM file)
* ``ContigConsensus(ctx).consensus(contigs, alignments_by_contig)``  (flye/polishing/consensus.py:52-181, get_consensus
  without the SAM reader and the FASTA writer)
* ``SamAlignments(ctx, sam_path, contigs, max_coverage, use_secondary).chunks() / by_contig()``
  (flye/utils/sam_parser.py:123-404, SynchronizedSamReader: get_chunk on fg_expand_cigars); with ``want_cols=False`` it
  keeps runs and SEQ in place of the gapped strings, for ``ContigConsensus.consensus_sam`` and ``BubbleMaker.make_sam`` /
  ``polish_sam`` (fg_contig_consensus_cigars / fg_make_bubbles_cigars: the columns are made and stay on the device); with
  ``device_text=True`` the file's text is cut into records on the device as well (``Context.sam_parse``, fg_sam_parse)
* ``DivergenceFinder(ctx).find_divergence(alignment_path, contigs_path, contigs_info, frequency_path, positions_path,
  div_sum_path, sub_thresh, del_thresh, ins_thresh)`` / ``profile``  (flye/trestle/divergence.py:55-232, on
  fg_divergence_profile); ``find_divergence_sam`` / ``profile_sam`` on fg_divergence_profile_cigars
* ``ReadPartitioner(ctx).partition_reads(edges, it, side, position_path, cons_align_path, template, read_align_path,
  consensuses, confirmed_pos_path, part_file, headers_to_id)`` / ``confirm`` / ``classify``
  (flye/trestle/trestle.py:1075-1628, on fg_confirm_positions and fg_classify_reads); ``partition_reads_sam`` /
  ``classify_sam`` on fg_classify_reads_cigars
* ``PlasmidFinder(ctx).calc_mapping_rates / extract_unmapped_reads / extract_circular_reads / extract_circular_pairs /
  trim_circular_reads / trim_circular_pairs / extract_unique_plasmids``  (flye/short_plasmids/unmapped_reads.py:51-88 and
  circular_sequences.py:33-191, on fg_paf_parse, fg_paf_groups, fg_paf_circular and fg_components)

There is no CPU fallback: if the HIP library or a device is missing every entry
point raises ``FlyeGpuError``.
"""
from __future__ import annotations

import collections
import ctypes as C
import gzip
import os
import random

import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FLYE_GPU_LIB: another build of the same library (kernel tuning experiments)
LIB_PATH = os.environ.get("FLYE_GPU_LIB") or os.path.join(_HERE, "lib", "libflyegpu.so")

REC_DTYPE = np.dtype([("cur_id", "<u4"), ("ext_id", "<u4"), ("cur_begin", "<i4"),
                      ("cur_end", "<i4"), ("cur_len", "<i4"), ("ext_begin", "<i4"),
                      ("ext_end", "<i4"), ("ext_len", "<i4"), ("score", "<i4"),
                      ("seq_divergence", "<f4"), ("chain_length", "<i4"),
                      ("filtered_positions", "<i4"), ("edit_distance", "<i4"),
                      ("hpc_len_cur", "<i4"), ("hpc_len_ext", "<i4")])

ABI_SYMBOLS = ["fg_abi_version", "fg_create", "fg_destroy", "fg_strerror", "fg_last_error",
               "fg_container_info", "fg_set_reads", "fg_set_queries", "fg_build_index_solid", "fg_build_index_minimizers",
               "fg_index_begin_solid", "fg_index_begin_minimizers", "fg_index_build_range", "fg_index_finish",
               "fg_index_kmer_hist", "fg_index_count_slice", "fg_index_batch_freq", "fg_index_batch_select",
               "fg_index_selection_done", "fg_index_gather_begin", "fg_index_gather_end", "fg_memory_stats",
               "fg_import_index", "fg_index_device_arrays", "fg_clear_index", "fg_export_index", "fg_overlaps", "fg_release_batch",
               "fg_kernel_times", "fg_debug_sort_pairs", "fg_debug_sort_pairs64", "fg_debug_sort_packed",
               "fg_debug_edit_distances", "fg_align_cigar_ksw", "fg_release_cigars",
               "fg_align_ranges", "fg_trim_ranges", "fg_release_trims", "fg_edit_ranges", "fg_chain_divergence",
               "fg_chain_alignments", "fg_release_chains",
               "fg_read_coverage", "fg_release_coverage", "fg_coverage_windows", "fg_coverage_verdict",
               "fg_edge_coverage", "fg_release_edge_coverage",
               "fg_subs_matrix_load", "fg_polish_bubbles", "fg_release_polish", "fg_make_bubbles", "fg_release_bubbles",
               "fg_uniform_alignments", "fg_release_uniform", "fg_contig_consensus", "fg_release_consensus",
               "fg_expand_cigars", "fg_release_expand", "fg_cigar_parse", "fg_contig_consensus_cigars", "fg_make_bubbles_cigars",
               "fg_divergence_profile", "fg_release_divergence",
               "fg_confirm_positions", "fg_release_confirm", "fg_classify_reads", "fg_release_classify",
               "fg_divergence_profile_cigars", "fg_classify_reads_cigars",
               "fg_paf_groups", "fg_release_paf_groups", "fg_paf_circular", "fg_release_paf_circular", "fg_components",
               "fg_paf_parse", "fg_release_paf_text", "fg_sam_parse", "fg_release_sam_text",
               "fg_index_keep_targets", "fg_index_shard", "fg_probe_hits", "fg_overlaps_from_hits",
               "fg_index_piece_split", "fg_index_scatter_begin", "fg_index_scatter_end", "fg_debug_probe_skip_check",
               "fg_group_create", "fg_group_destroy", "fg_group_size", "fg_group_member", "fg_group_last_error",
               "fg_group_set_reads", "fg_group_set_queries", "fg_group_build_index_solid",
               "fg_group_build_index_minimizers", "fg_group_clear_index", "fg_group_overlaps", "fg_group_stats",
               "fg_group_build_info", "fg_debug_freq_accumulate", "fg_debug_group_bin_cuts", "fg_debug_scan",
               "fg_debug_radix_sort_pairs", "fg_debug_tie_free", "fg_debug_chain_lazy", "fg_debug_sort_screen",
               "fg_debug_order_free", "fg_debug_sort_radix_segments", "fg_debug_table"]

# struct fg_range_pair: one pair of fg_align_ranges
RANGE_PAIR_DTYPE = np.dtype([("cur_id", "<u4"), ("ext_id", "<u4"), ("cur_begin", "<i4"), ("cur_end", "<i4"),
                             ("ext_begin", "<i4"), ("ext_end", "<i4")])

# struct fg_trim_rec: one piece checkIdyAndTrim keeps of a pair (fg_trim_ranges)
TRIM_REC_DTYPE = np.dtype([("cur_begin", "<i4"), ("cur_end", "<i4"), ("ext_begin", "<i4"), ("ext_end", "<i4"),
                           ("run_start", "<i4"), ("run_end", "<i4"), ("range_err", "<i4"), ("range_len", "<i4"),
                           ("seq_divergence", "<f4")])

# struct fg_paf_hit: one PAF line, names as ids of one name space (fg_paf_groups / fg_paf_circular)
PAF_HIT_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4"), ("query_len", "<i4"), ("query_start", "<i4"), ("query_end", "<i4"),
                          ("target_len", "<i4"), ("target_start", "<i4"), ("target_end", "<i4")])

# struct fg_seed_hit: KmerMatch{curPos, extPos, extId} (overlap.cpp:176-196)
SEED_HIT_DTYPE = np.dtype([("cur_pos", "<i4"), ("ext_pos", "<i4"), ("ext_id", "<u4")])


class FlyeGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libflyegpu error {code}: {msg}")
        self.code = code


class IndexStats(C.Structure):
    _fields_ = [("total_kmers", C.c_uint64), ("selected_kmers", C.c_uint64),
                ("index_entries", C.c_uint64), ("repetitive_kmers", C.c_uint64),
                ("repetitive_frequency", C.c_uint64), ("mean_frequency", C.c_float),
                ("sample_rate", C.c_float), ("build_seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DetectorParams(C.Structure):
    _fields_ = [("max_jump", C.c_int32), ("min_overlap", C.c_int32),
                ("max_overhang", C.c_int32), ("keep_alignment", C.c_uint8),
                ("only_max_ext", C.c_uint8), ("nucl_alignment", C.c_uint8),
                ("partition_bad_mappings", C.c_uint8), ("use_hpc", C.c_uint8),
                ("pad_", C.c_uint8 * 3), ("max_divergence", C.c_float)]


class OverlapBatch(C.Structure):
    _fields_ = [("n_queries", C.c_uint32), ("n_recs", C.c_uint64), ("query_off", C.c_void_p),
                ("recs", C.c_void_p), ("n_div_stats", C.c_uint64), ("div_stats_off", C.c_void_p),
                ("div_stats", C.c_void_p), ("n_matches", C.c_uint64), ("match_off", C.c_void_p),
                ("matches", C.c_void_p), ("needs_trim", C.c_void_p), ("query_bp", C.c_uint64), ("query_kmers", C.c_uint64),
                ("seed_hits", C.c_uint64), ("dp_groups", C.c_uint64), ("dp_elements", C.c_uint64),
                ("dp_elements_small", C.c_uint64),
                ("device_seconds", C.c_double), ("owner_", C.c_void_p)]


class CigarBatch(C.Structure):
    _fields_ = [("n_pairs", C.c_uint32), ("run_off", C.POINTER(C.c_uint64)), ("ops", C.POINTER(C.c_uint8)),
                ("lens", C.POINTER(C.c_int32)), ("err_rate", C.POINTER(C.c_float)), ("owner_", C.c_void_p)]


class TrimBatch(C.Structure):
    _fields_ = [("n_pairs", C.c_uint32), ("rec_off", C.POINTER(C.c_uint64)), ("recs", C.c_void_p), ("owner_", C.c_void_p)]


class ChainParams(C.Structure):
    """struct fg_chain_params: the constants of ReadAligner::chainReadAlignments and of the alignRead lambda's filter
    (read_aligner.cpp:27-30, :158-160)."""
    _fields_ = [("max_jump", C.c_int32), ("max_read_overlap", C.c_int32), ("min_alignment", C.c_int32),
                ("max_separation", C.c_int32), ("long_edge", C.c_int32), ("big_alignment", C.c_int32)]

    @classmethod
    def from_config(cls, cfg: dict, min_overlap: int):
        """MAX_JUMP and MAX_SEP from the configuration, MIN_ALN = Parameters::minimumOverlap, the rest the reference's
        literals."""
        return cls(max_jump=int(cfg["maximum_jump"]), max_read_overlap=50, min_alignment=int(min_overlap),
                   max_separation=int(cfg["max_separation"]), long_edge=900, big_alignment=500)


class ChainBatch(C.Structure):
    _fields_ = [("n_queries", C.c_uint32), ("n_chains", C.c_uint64), ("n_alns", C.c_uint64),
                ("chain_off", C.POINTER(C.c_uint64)), ("aln_off", C.POINTER(C.c_uint64)), ("aln", C.POINTER(C.c_uint64)),
                ("score", C.POINTER(C.c_int32)), ("owner_", C.c_void_p)]


class CoverageParams(C.Structure):
    """struct fg_coverage_params: the constants of ChimeraDetector's coverage test (chimera.cpp:110, :140, :156, :168)."""
    _fields_ = [("window", C.c_int32), ("max_overhang", C.c_int32), ("max_drop_rate", C.c_float),
                ("overlap_coverage", C.c_int32), ("uneven_coverage", C.c_uint8), ("want_vectors", C.c_uint8),
                ("pad_", C.c_uint8 * 2)]

    @classmethod
    def from_config(cls, cfg: dict, overlap_coverage=0, uneven_coverage=False, want_vectors=True):
        """cfg: a preset (config.preset) or config.assemble_stage; the two keys a preset does not carry take the
        values of asm_defaults.cfg (config.ASSEMBLE_STAGE)."""
        from .config import ASSEMBLE_STAGE
        return cls(window=int(cfg.get("chimera_window", ASSEMBLE_STAGE["chimera_window"])), max_overhang=int(cfg["maximum_overhang"]),
                   max_drop_rate=float(cfg.get("max_coverage_drop_rate", ASSEMBLE_STAGE["max_coverage_drop_rate"])),
                   overlap_coverage=int(overlap_coverage),
                   uneven_coverage=int(bool(uneven_coverage)), want_vectors=int(bool(want_vectors)))


class CoverageBatch(C.Structure):
    _fields_ = [("n_queries", C.c_uint32), ("win_off", C.POINTER(C.c_uint64)), ("full", C.POINTER(C.c_int32)),
                ("junction", C.POINTER(C.c_int32)), ("sum", C.POINTER(C.c_int64)), ("max", C.POINTER(C.c_int32)),
                ("median", C.POINTER(C.c_int32)), ("min_good", C.POINTER(C.c_int32)), ("threshold", C.POINTER(C.c_int32)),
                ("chimeric", C.POINTER(C.c_uint8)), ("degenerate", C.POINTER(C.c_uint8)), ("owner_", C.c_void_p)]


class EdgeCoverageBatch(C.Structure):
    _fields_ = [("n_edges", C.c_uint32), ("win_off", C.POINTER(C.c_uint64)), ("cov", C.POINTER(C.c_int32)),
                ("sum", C.POINTER(C.c_int64)), ("max", C.POINTER(C.c_int32)), ("median", C.POINTER(C.c_int32)),
                ("owner_", C.c_void_p)]


class SubsMatrixStruct(C.Structure):
    """struct fg_subs_matrix: score[consensus class][read class], classes A C G T other gap"""
    _fields_ = [("score", (C.c_int64 * 6) * 6)]


class PolishBatch(C.Structure):
    _fields_ = [("n_bubbles", C.c_uint32), ("cand", C.POINTER(C.c_uint8)), ("cand_off", C.POINTER(C.c_uint64)),
                ("n_steps", C.POINTER(C.c_uint32)), ("status", C.POINTER(C.c_uint8)), ("step_off", C.POINTER(C.c_uint64)),
                ("step_score", C.POINTER(C.c_int64)), ("step_seq", C.POINTER(C.c_uint8)),
                ("step_seq_off", C.POINTER(C.c_uint64)), ("owner_", C.c_void_p)]


class BubbleParams(C.Structure):
    """struct fg_bubble_params: cfg.vals of flye/config/py_cfg.py:41-46 and the err_modes entry of the platform"""
    _fields_ = [("solid_kmer_length", C.c_int32), ("simple_kmer_length", C.c_int32), ("max_bubble_length", C.c_int32),
                ("max_bubble_branches", C.c_int32), ("min_polish_aln_len", C.c_int32), ("pad_", C.c_int32),
                ("solid_missmatch", C.c_double), ("solid_indel", C.c_double), ("max_aln_error", C.c_double)]

    # the reference's values (py_cfg.py:41-46, :52-66)
    DEFAULTS = dict(simple_kmer_length=4, solid_kmer_length=10, max_bubble_length=500, max_bubble_branches=50,
                    min_polish_aln_len=500)
    ERR_MODES = dict(pacbio=dict(solid_missmatch=0.2, solid_indel=0.2, max_aln_error=0.25),
                     nano=dict(solid_missmatch=0.3, solid_indel=0.3, max_aln_error=0.25))

    @classmethod
    def for_mode(cls, err_mode, **overrides):
        vals = dict(cls.DEFAULTS)
        vals.update(cls.ERR_MODES[err_mode])
        vals.update(overrides)
        return cls(**vals)


class BubbleBatch(C.Structure):
    _fields_ = [("n_contigs", C.c_uint32), ("n_bubbles", C.c_uint32), ("n_alignments", C.c_uint64),
                ("bubble_off", C.POINTER(C.c_uint64)), ("position", C.POINTER(C.c_int32)), ("cand", C.POINTER(C.c_uint8)),
                ("cand_off", C.POINTER(C.c_uint64)), ("branches", C.POINTER(C.c_uint8)), ("branch_off", C.POINTER(C.c_uint64)),
                ("bubble_branch_off", C.POINTER(C.c_uint64)), ("n_long_bubbles", C.POINTER(C.c_int32)),
                ("n_empty", C.POINTER(C.c_int32)), ("n_long_branch", C.POINTER(C.c_int32)), ("mean_cov", C.POINTER(C.c_int64)),
                ("n_partition", C.POINTER(C.c_int32)), ("in_profile", C.POINTER(C.c_uint8)), ("part_off", C.POINTER(C.c_uint64)),
                ("partition", C.POINTER(C.c_int32)), ("prof_off", C.POINTER(C.c_uint64)), ("coverage", C.POINTER(C.c_int32)),
                ("num_inserts", C.POINTER(C.c_int32)), ("num_deletions", C.POINTER(C.c_int32)),
                ("num_missmatch", C.POINTER(C.c_int32)), ("nucl", C.POINTER(C.c_uint8)), ("owner_", C.c_void_p)]


class UniformResultStruct(C.Structure):
    """struct fg_uniform_result"""
    _fields_ = [("n_contigs", C.c_uint32), ("pad_", C.c_uint32), ("n_alignments", C.c_uint64), ("keep", C.POINTER(C.c_uint8)),
                ("cov_threshold", C.POINTER(C.c_int32)), ("wnd_off", C.POINTER(C.c_uint64)),
                ("wnd_threshold", C.POINTER(C.c_double)), ("owner_", C.c_void_p)]


class ConsensusBatch(C.Structure):
    """struct fg_consensus_batch"""
    _fields_ = [("n_contigs", C.c_uint32), ("pad_", C.c_uint32), ("seq_off", C.POINTER(C.c_uint64)), ("seq", C.POINTER(C.c_uint8)),
                ("prof_off", C.POINTER(C.c_uint64)), ("nucl", C.POINTER(C.c_uint8)), ("match_total", C.POINTER(C.c_int32)),
                ("num_ins", C.POINTER(C.c_int32)), ("max_match", C.POINTER(C.c_uint8)), ("accepted", C.POINTER(C.c_uint8)),
                ("ins_off", C.POINTER(C.c_uint64)), ("ins", C.POINTER(C.c_uint8)), ("owner_", C.c_void_p)]


class ExpandBatch(C.Structure):
    """struct fg_expand_batch"""
    _fields_ = [("n_alignments", C.c_uint64), ("col_off", C.POINTER(C.c_uint64)), ("trg_cols", C.POINTER(C.c_uint8)),
                ("qry_cols", C.POINTER(C.c_uint8)), ("trg_start", C.POINTER(C.c_int32)), ("trg_end", C.POINTER(C.c_int32)),
                ("qry_start", C.POINTER(C.c_int32)), ("qry_end", C.POINTER(C.c_int32)), ("qry_len", C.POINTER(C.c_int32)),
                ("matches", C.POINTER(C.c_int64)), ("err_rate", C.POINTER(C.c_double)), ("owner_", C.c_void_p)]


class DivergenceBatch(C.Structure):
    """struct fg_divergence_batch"""
    _fields_ = [("n_contigs", C.c_uint32), ("pad_", C.c_uint32), ("total_off", C.POINTER(C.c_uint64)),
                ("total_pos", C.POINTER(C.c_int32)), ("sub_off", C.POINTER(C.c_uint64)), ("sub_pos", C.POINTER(C.c_int32)),
                ("del_off", C.POINTER(C.c_uint64)), ("del_pos", C.POINTER(C.c_int32)), ("ins_off", C.POINTER(C.c_uint64)),
                ("ins_pos", C.POINTER(C.c_int32)), ("prof_off", C.POINTER(C.c_uint64)), ("cov", C.POINTER(C.c_int32)),
                ("nucl", C.POINTER(C.c_uint8)), ("mat_ct", C.POINTER(C.c_int32)), ("sub_base", C.POINTER(C.c_uint8)),
                ("sub_ct", C.POINTER(C.c_int32)), ("del_ct", C.POINTER(C.c_int32)), ("ins_base", C.POINTER(C.c_uint8)),
                ("ins_ct", C.POINTER(C.c_int32)), ("flags", C.POINTER(C.c_uint8)), ("owner_", C.c_void_p)]


CONFIRM_LISTS = ("conf_total", "conf_sub", "conf_del", "conf_ins", "rej_total", "rej_sub", "rej_del", "rej_ins")


class ConfirmBatch(C.Structure):
    """struct fg_confirm_batch"""
    _fields_ = [("n_jobs", C.c_uint32), ("pad_", C.c_uint32), ("n_edges", C.c_uint64)] + \
        [f for k in CONFIRM_LISTS for f in ((k + "_off", C.POINTER(C.c_uint64)), (k + "_pos", C.POINTER(C.c_int32)))] + \
        [("cons_off", C.POINTER(C.c_uint64)), ("cons_pos", C.POINTER(C.c_int32)), ("owner_", C.c_void_p)]


class ClassifyBatch(C.Structure):
    """struct fg_classify_batch"""
    _fields_ = [("n_jobs", C.c_uint32), ("pad_", C.c_uint32), ("n_alignments", C.c_uint64), ("read_off", C.POINTER(C.c_uint64)),
                ("status", C.POINTER(C.c_uint8)), ("top_edge", C.POINTER(C.c_int32)), ("top_score", C.POINTER(C.c_int32)),
                ("total_score", C.POINTER(C.c_int32)), ("aln_score", C.POINTER(C.c_int32)), ("aln_counted", C.POINTER(C.c_uint8)),
                ("owner_", C.c_void_p)]


class PafGroupBatch(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("n_groups", C.c_uint32), ("order", C.POINTER(C.c_uint32)),
                ("group_off", C.POINTER(C.c_uint64)), ("group_query", C.POINTER(C.c_uint32)), ("group_target", C.POINTER(C.c_uint32)),
                ("query_cover", C.POINTER(C.c_int64)), ("target_cover", C.POINTER(C.c_int64)), ("owner_", C.c_void_p)]


class PafCircularBatch(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("n_circular", C.c_uint32), ("circ_query", C.POINTER(C.c_uint32)),
                ("circ_hit", C.POINTER(C.c_uint32)), ("n_groups", C.c_uint32), ("group_query", C.POINTER(C.c_uint32)),
                ("group_target", C.POINTER(C.c_uint32)), ("pair_first", C.POINTER(C.c_int32)), ("pair_second", C.POINTER(C.c_int32)),
                ("pair_ok", C.POINTER(C.c_uint8)), ("owner_", C.c_void_p)]


class PafText(C.Structure):
    _fields_ = [("n_hits", C.c_uint64), ("query_name_off", C.POINTER(C.c_uint64)), ("query_name_len", C.POINTER(C.c_uint32)),
                ("target_name_off", C.POINTER(C.c_uint64)), ("target_name_len", C.POINTER(C.c_uint32)),
                ("query_len", C.POINTER(C.c_int32)), ("query_start", C.POINTER(C.c_int32)), ("query_end", C.POINTER(C.c_int32)),
                ("target_len", C.POINTER(C.c_int32)), ("target_start", C.POINTER(C.c_int32)), ("target_end", C.POINTER(C.c_int32)),
                ("owner_", C.c_void_p)]


class SamText(C.Structure):
    _fields_ = ([("n_lines", C.c_uint64), ("n_records", C.c_uint64), ("n_chunks", C.c_uint64), ("n_runs", C.c_uint64),
                 ("chunk_off", C.POINTER(C.c_uint64)), ("line_no", C.POINTER(C.c_uint64)), ("line_off", C.POINTER(C.c_uint64)),
                 ("line_len", C.POINTER(C.c_uint32)), ("status", C.POINTER(C.c_uint8))] +
                [(k + s, C.POINTER(t)) for k in ("tab_rname", "qname", "rname", "cigar", "seq")
                 for s, t in (("_off", C.c_uint64), ("_len", C.c_uint32))] +
                [("flag", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int32)), ("qry_start", C.POINTER(C.c_int64)),
                 ("qry_end", C.POINTER(C.c_int64)), ("run_off", C.POINTER(C.c_uint64)), ("run_op", C.POINTER(C.c_uint8)),
                 ("run_len", C.POINTER(C.c_uint32)), ("owner_", C.c_void_p)])


class BridgeStats(C.Structure):
    _fields_ = [("device_calls", C.c_uint64), ("reads_computed", C.c_uint64), ("requests", C.c_uint64),
                ("cache_hits", C.c_uint64), ("cached_overlaps", C.c_uint64), ("reads_ahead", C.c_uint64),
                ("ahead_hits", C.c_uint64)]


class GroupStats(C.Structure):
    _fields_ = [("hits_moved_bytes", C.c_uint64), ("hits_total", C.c_uint64), ("peer_copies", C.c_uint64),
                ("exchange_seconds", C.c_double)]


class GroupBuildInfo(C.Structure):
    _fields_ = [("selection_batches", C.c_uint32), ("stage_pieces_max", C.c_uint32), ("stage_pieces", C.c_uint64),
                ("freq_bytes", C.c_uint64), ("scatter_bytes", C.c_uint64)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("seconds", C.c_double), ("launches", C.c_uint64)]


_LIB = None


def load_library():
    """Load libflyegpu.so.  Raises if it is missing -- the product never falls
    back to a CPU path."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise FlyeGpuError(-100, f"{LIB_PATH} not built: run __graft_entry__.build()")
        # One HIP runtime per process.  torch ships its own copy of libamdhip64 / libhsa-runtime64; a Python
        # process that uses both this library and torch.cuda (flye_amd/dist.py wraps context memory as torch
        # tensors for the collectives) must load torch's FIRST -- the other order leaves torch with "No HIP GPUs
        # are available" (measured: pytest process, library loaded before the first torch.cuda call).  A C / C++
        # consumer of the C ABI never sees torch.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.fg_abi_version.restype = C.c_int
        L.fg_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
        L.fg_destroy.argtypes = [C.c_void_p]
        L.fg_strerror.restype = C.c_char_p
        L.fg_strerror.argtypes = [C.c_int]
        L.fg_last_error.restype = C.c_char_p
        L.fg_last_error.argtypes = [C.c_void_p]
        L.fg_set_reads.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.fg_set_queries.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.fg_build_index_solid.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_float,
                                           C.c_float, C.POINTER(IndexStats)]
        L.fg_build_index_minimizers.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_float,
                                                C.POINTER(IndexStats)]
        L.fg_index_begin_solid.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_void_p]
        L.fg_index_begin_minimizers.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
        L.fg_index_build_range.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.fg_index_finish.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(IndexStats)]
        L.fg_index_kmer_hist.argtypes = [C.c_void_p, C.c_void_p]
        L.fg_index_count_slice.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_float, C.c_uint32,
                                           C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.fg_index_batch_freq.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.fg_index_batch_select.argtypes = [C.c_void_p, C.c_uint32]
        L.fg_index_selection_done.argtypes = [C.c_void_p, C.c_void_p]
        L.fg_index_gather_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fg_index_gather_end.argtypes = [C.c_void_p, C.c_float]
        L.fg_memory_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
        L.fg_import_index.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_float, C.c_int]
        L.fg_index_device_arrays.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        L.fg_clear_index.argtypes = [C.c_void_p]
        L.fg_export_index.argtypes = [C.c_void_p] + [C.c_void_p] * 7
        L.fg_overlaps.argtypes = [C.c_void_p, C.POINTER(DetectorParams), C.c_void_p, C.c_uint32,
                                  C.c_int32, C.c_uint8, C.POINTER(OverlapBatch)]
        L.fg_release_batch.argtypes = [C.POINTER(OverlapBatch)]
        L.fg_index_keep_targets.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
        L.fg_index_shard.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.fg_index_piece_split.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]
        L.fg_index_scatter_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
        L.fg_index_scatter_end.argtypes = [C.c_void_p, C.c_float]
        L.fg_probe_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p),
                                    C.POINTER(C.c_uint64)]
        L.fg_overlaps_from_hits.argtypes = [C.c_void_p, C.POINTER(DetectorParams), C.c_void_p, C.c_uint32, C.c_int32,
                                            C.c_uint8, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(OverlapBatch)]
        L.fg_kernel_times.argtypes = [C.c_void_p, C.POINTER(KernelTime), C.c_int]
        L.fg_debug_sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.fg_debug_sort_pairs64.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
        L.fg_debug_sort_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int]
        L.fg_debug_sort_pairs32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int,
                                            C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.fg_debug_sort_pairs32_val16.argtypes = L.fg_debug_sort_pairs32.argtypes
        L.fg_debug_hit_val16.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.fg_debug_tie_free.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.fg_debug_sort_screen.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                           C.c_float, C.c_int32, C.c_void_p]
        L.fg_debug_order_free.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.fg_debug_sort_radix_segments.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.fg_debug_probe_skip_check.argtypes =[C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.fg_debug_chain_lazy.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.fg_debug_table.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fg_debug_edit_distances.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fg_align_cigar_ksw.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(CigarBatch)]
        L.fg_release_cigars.argtypes = [C.POINTER(CigarBatch)]
        L.fg_align_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint8, C.POINTER(CigarBatch), C.c_void_p,
                                      C.c_void_p]
        L.fg_trim_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint8, C.c_float, C.c_int32, C.POINTER(TrimBatch)]
        L.fg_release_trims.argtypes = [C.POINTER(TrimBatch)]
        L.fg_release_trims.restype = None
        L.fg_edit_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint8, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]
        L.fg_chain_divergence.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
        L.fg_chain_alignments.argtypes = [C.c_void_p, C.POINTER(ChainParams), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                          C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(ChainBatch)]
        L.fg_release_chains.argtypes = [C.POINTER(ChainBatch)]
        L.fg_release_chains.restype = None
        L.fg_read_coverage.argtypes = [C.c_void_p, C.POINTER(CoverageParams), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.POINTER(CoverageBatch)]
        L.fg_release_coverage.argtypes = [C.POINTER(CoverageBatch)]
        L.fg_release_coverage.restype = None
        L.fg_coverage_windows.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_uint8)]
        L.fg_coverage_verdict.argtypes = [C.POINTER(CoverageParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.fg_edge_coverage.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint8,
                                       C.POINTER(EdgeCoverageBatch)]
        L.fg_release_edge_coverage.argtypes = [C.POINTER(EdgeCoverageBatch)]
        L.fg_release_edge_coverage.restype = None
        L.fg_subs_matrix_load.argtypes = [C.c_char_p, C.POINTER(SubsMatrixStruct)]
        L.fg_polish_bubbles.argtypes = [C.c_void_p, C.POINTER(SubsMatrixStruct), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_uint32, C.c_uint8, C.c_uint8, C.POINTER(PolishBatch)]
        L.fg_release_polish.argtypes = [C.POINTER(PolishBatch)]
        L.fg_release_polish.restype = None
        L.fg_make_bubbles.argtypes = [C.c_void_p, C.POINTER(BubbleParams), C.c_uint32] + [C.c_void_p] * 9 + \
            [C.c_uint8, C.POINTER(BubbleBatch)]
        L.fg_release_bubbles.argtypes = [C.POINTER(BubbleBatch)]
        L.fg_release_bubbles.restype = None
        L.fg_uniform_alignments.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint8, C.POINTER(UniformResultStruct)]
        L.fg_release_uniform.argtypes = [C.POINTER(UniformResultStruct)]
        L.fg_release_uniform.restype = None
        L.fg_contig_consensus.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 8 + [C.c_uint8, C.POINTER(ConsensusBatch)]
        L.fg_release_consensus.argtypes = [C.POINTER(ConsensusBatch)]
        L.fg_release_consensus.restype = None
        L.fg_expand_cigars.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64] + [C.c_void_p] * 7 + \
            [C.c_uint8, C.POINTER(ExpandBatch)]
        L.fg_release_expand.argtypes = [C.POINTER(ExpandBatch)]
        L.fg_release_expand.restype = None
        L.fg_contig_consensus_cigars.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 11 + [C.c_uint8, C.POINTER(ConsensusBatch)]
        L.fg_make_bubbles_cigars.argtypes = [C.c_void_p, C.POINTER(BubbleParams), C.c_uint32] + [C.c_void_p] * 11 + \
            [C.c_uint8, C.POINTER(BubbleBatch)]
        L.fg_cigar_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        L.fg_divergence_profile.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_uint32] + [C.c_void_p] * 6 + \
            [C.c_uint8, C.POINTER(DivergenceBatch)]
        L.fg_release_divergence.argtypes = [C.POINTER(DivergenceBatch)]
        L.fg_release_divergence.restype = None
        L.fg_confirm_positions.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 16 + [C.POINTER(ConfirmBatch)]
        L.fg_release_confirm.argtypes = [C.POINTER(ConfirmBatch)]
        L.fg_release_confirm.restype = None
        L.fg_classify_reads.argtypes = [C.c_void_p, C.c_int32, C.c_uint32] + [C.c_void_p] * 11 + [C.c_uint8, C.POINTER(ClassifyBatch)]
        L.fg_release_classify.argtypes = [C.POINTER(ClassifyBatch)]
        L.fg_release_classify.restype = None
        L.fg_divergence_profile_cigars.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_uint32] + [C.c_void_p] * 9 + \
            [C.c_uint8, C.POINTER(DivergenceBatch)]
        L.fg_classify_reads_cigars.argtypes = [C.c_void_p, C.c_int32, C.c_uint32] + [C.c_void_p] * 14 + [C.c_uint8, C.POINTER(ClassifyBatch)]
        L.fg_debug_group_bin_cuts.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.fg_debug_freq_accumulate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.fg_debug_scan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int]
        L.fg_debug_radix_sort_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int,
                                                C.POINTER(C.c_int)]
        # device group: several contexts of this process behind one handle
        L.fg_group_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_uint32, C.c_int]
        L.fg_group_destroy.argtypes = [C.c_void_p]
        L.fg_group_destroy.restype = None
        L.fg_group_size.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.fg_group_member.restype = C.c_void_p
        L.fg_group_member.argtypes = [C.c_void_p, C.c_uint32]
        L.fg_group_last_error.restype = C.c_char_p
        L.fg_group_last_error.argtypes = [C.c_void_p]
        L.fg_group_set_reads.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.fg_group_set_queries.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        L.fg_group_build_index_solid.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_float, C.c_float,
                                                 C.POINTER(IndexStats)]
        L.fg_group_build_index_minimizers.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.POINTER(IndexStats)]
        L.fg_group_clear_index.argtypes = [C.c_void_p]
        L.fg_group_overlaps.argtypes = [C.c_void_p, C.POINTER(DetectorParams), C.c_void_p, C.c_uint32, C.c_int32,
                                        C.c_uint8, C.POINTER(OverlapBatch)]
        L.fg_group_stats.argtypes = [C.c_void_p, C.POINTER(GroupStats)]
        L.fg_group_build_info.argtypes = [C.c_void_p, C.POINTER(GroupBuildInfo)]
        L.fg_paf_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(PafGroupBatch)]
        L.fg_release_paf_groups.argtypes = [C.POINTER(PafGroupBatch)]
        L.fg_paf_circular.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(PafCircularBatch)]
        L.fg_release_paf_circular.argtypes = [C.POINTER(PafCircularBatch)]
        L.fg_components.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fg_paf_parse.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(PafText)]
        L.fg_release_paf_text.argtypes = [C.POINTER(PafText)]
        L.fg_sam_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(SamText)]
        L.fg_release_sam_text.argtypes = [C.POINTER(SamText)]
        # include/flye_gpu_bridge.h
        L.fgb_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(DetectorParams), C.c_uint32, C.c_uint32]
        L.fgb_destroy.argtypes = [C.c_void_p]
        L.fgb_lazy.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.fgb_quick.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_uint8, C.c_void_p, C.c_uint64,
                                C.POINTER(C.c_uint64)]
        L.fgb_prefetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.fgb_set_divergence_threshold.argtypes = [C.c_void_p, C.c_float]
        L.fgb_divergence_stats.restype = C.c_uint64
        L.fgb_divergence_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.fgb_get_stats.argtypes = [C.c_void_p, C.POINTER(BridgeStats)]
        # on-disk text forms (host only)
        L.fg_overlap_dump.restype = C.c_int64
        L.fg_overlap_dump.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64]
        L.fg_overlap_load.argtypes = [C.c_char_p, C.c_void_p] + [C.POINTER(C.c_uint32)] * 4
        L.fg_alignment_dump.restype = C.c_int64
        L.fg_alignment_dump.argtypes = [C.c_int64, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64]
        L.fg_fasta_record.restype = C.c_int64
        L.fg_fasta_record.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_uint64]
        _LIB = L
    return _LIB


class IndexExport:
    def __init__(self, keys, key_off, entries, repetitive):
        self.keys, self.key_off, self.entries, self.repetitive = keys, key_off, entries, repetitive


class _Arena:
    """Owns one fg_overlap_batch; released when the last array view is gone."""

    def __init__(self, lib, batch):
        self.lib, self.batch = lib, batch

    def __del__(self):
        try:
            self.lib.fg_release_batch(C.byref(self.batch))
        except Exception:
            pass

    def view(self, ptr, ctype, count, dtype):
        if not count:
            return np.empty(0, dtype)
        buf = (ctype * count).from_address(ptr)
        buf._arena = self            # the numpy view keeps buf (its base), buf keeps the arena
        return np.frombuffer(buf, dtype=dtype)


class OverlapResult:
    """Flat result of one batched ``getSeqOverlaps`` call.  The arrays are zero-copy
    views of the library-owned arena; the arena is released when the last view dies."""

    def __init__(self, lib, query_ids, batch):
        arena = _Arena(lib, batch)
        b = batch
        nq = len(query_ids)
        self.query_ids = query_ids
        self.query_off = arena.view(b.query_off, C.c_uint64, nq + 1, np.uint64)
        self.stat_off = arena.view(b.div_stats_off, C.c_uint64, nq + 1, np.uint64)
        self.recs = arena.view(b.recs, C.c_uint8, b.n_recs * REC_DTYPE.itemsize, REC_DTYPE)
        self.stats = arena.view(b.div_stats, C.c_float, b.n_div_stats, np.float32)
        # keep_alignment: kmerMatches of recs[i] = matches[match_off[i]:match_off[i+1]] ((cur, ext) rows)
        self.match_off = self.matches = None
        if b.match_off:
            self.match_off = arena.view(b.match_off, C.c_uint64, b.n_recs + 1, np.uint64)
            self.matches = arena.view(b.matches, C.c_int32, 2 * b.n_matches, np.int32).reshape(-1, 2)
        # partition_bad_mappings: 1 = failed the divergence gate, there for the caller's checkIdyAndTrim
        self.needs_trim = arena.view(b.needs_trim, C.c_uint8, b.n_recs, np.uint8) if b.needs_trim else None
        self.query_bp, self.query_kmers = b.query_bp, b.query_kmers
        self.seed_hits, self.dp_groups, self.dp_elements = b.seed_hits, b.dp_groups, b.dp_elements
        self.dp_elements_small = b.dp_elements_small
        self.device_seconds = b.device_seconds

    def of(self, i):
        return self.recs[int(self.query_off[i]):int(self.query_off[i + 1])]

    def kmerMatches(self, i):
        """OverlapRange::kmerMatches of record i (keep_alignment detectors only)."""
        return self.matches[int(self.match_off[i]):int(self.match_off[i + 1])]

    def match_digests(self):
        """(count, order-sensitive 64-bit digest) per record:
        sum_j (j+1) * (cur_j * 0x9E3779B97F4A7C15 + ext_j + 1) mod 2^64."""
        off = self.match_off.astype(np.int64)
        m = self.matches.astype(np.int64).astype(np.uint64)
        with np.errstate(over="ignore"):
            v = m[:, 0] * np.uint64(0x9E3779B97F4A7C15) + m[:, 1] + np.uint64(1)
            j = np.arange(len(m), dtype=np.int64) - np.repeat(off[:-1], np.diff(off)) + 1
            cs = np.concatenate([[np.uint64(0)], np.cumsum(v * j.astype(np.uint64), dtype=np.uint64)])
            return np.diff(off), cs[off[1:]] - cs[off[:-1]]

    def spliced(self, trims):
        """The records with each one marked in needs_trim replaced, in place and in order, by the pieces checkIdyAndTrim
        keeps of it (overlap.cpp:474-485).  trims = Context.trim_ranges(self.recs[self.needs_trim != 0], ...).  A
        piece is its parent record with the four coordinates and seq_divergence replaced (alignment.cpp:416-417; the
        score, the lengths and kmerMatches are the parent's).  Returns a result of host arrays with lines(), of(),
        kmerMatches(): records, per-query offsets, kmerMatches; no record of it is marked."""
        if self.needs_trim is None:
            raise ValueError("spliced: the result has no needs_trim marks (partition_bad_mappings)")
        rec_off, pieces = trims
        marked = np.flatnonzero(np.asarray(self.needs_trim) != 0)
        if len(rec_off) != len(marked) + 1:
            raise ValueError("spliced: trims must hold one entry per marked record")
        n = len(self.recs)
        mult = np.ones(n, np.int64)
        mult[marked] = np.diff(rec_off.astype(np.int64))
        src = np.repeat(np.arange(n, dtype=np.int64), mult)
        recs = np.asarray(self.recs)[src].copy()
        from_piece = np.repeat(np.asarray(self.needs_trim) != 0, mult)
        assert int(from_piece.sum()) == len(pieces)
        for f in ("cur_begin", "cur_end", "ext_begin", "ext_end", "seq_divergence"):
            recs[f][from_piece] = pieces[f]
        out = object.__new__(OverlapResult)
        out.__dict__.update(self.__dict__)
        out.recs = recs
        out.needs_trim = np.zeros(len(recs), np.uint8)
        new_off = np.concatenate([[0], np.cumsum(mult)])
        out.query_off = new_off[np.asarray(self.query_off).astype(np.int64)].astype(np.uint64)
        if self.match_off is not None:
            off = np.asarray(self.match_off).astype(np.int64)
            cnt = np.diff(off)[src]
            out.match_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
            idx = np.repeat(off[:-1][src] - out.match_off[:-1].astype(np.int64), cnt) + np.arange(int(cnt.sum()), dtype=np.int64)
            out.matches = np.asarray(self.matches)[idx]
        return out

    def lines(self):
        r = self.recs
        bits = r["seq_divergence"].view(np.uint32)
        out = [f"{r['cur_id'][i]} {r['cur_begin'][i]} {r['cur_end'][i]} {r['cur_len'][i]} "
               f"{r['ext_id'][i]} {r['ext_begin'][i]} {r['ext_end'][i]} {r['ext_len'][i]} "
               f"{r['score'][i]} {bits[i]:08x}" for i in range(len(r))]
        if self.match_off is not None:
            cnt, dg = self.match_digests()
            out = [f"{l} {cnt[i]} {int(dg[i]):016x}" for i, l in enumerate(out)]
        return out


def memory_stats(reset_peak=False):
    """(device bytes the library holds now, peak since the last reset) over all contexts of the process"""
    now, peak = C.c_uint64(), C.c_uint64()
    load_library().fg_memory_stats(C.byref(now), C.byref(peak), 1 if reset_peak else 0)
    return now.value, peak.value


def chain_divergence(cur_range, divergence, chain_off):
    """fg_chain_divergence: ReadAligner::getChainBaseDivergence (read_aligner.cpp:410-434) of the chains
    [chain_off[c], chain_off[c + 1]) over per-alignment cur ranges and divergences, in the reference's single-precision
    operation order; float32 array of len(chain_off) - 1 values (NaN for an empty or zero-length chain)."""
    cr = np.ascontiguousarray(cur_range, np.int32)
    dv = np.ascontiguousarray(divergence, np.float32)
    off = np.ascontiguousarray(chain_off, np.uint64)
    if len(cr) != len(dv) or len(off) < 1 or (len(off) > 1 and int(off.max()) > len(cr)):
        raise ValueError("chain_divergence: one divergence per cur_range, offsets inside them")
    n = len(off) - 1
    out = np.zeros(n, np.float32)
    L = load_library()
    rc = L.fg_chain_divergence(cr.ctypes.data if len(cr) else None, dv.ctypes.data if len(dv) else None,
                               off.ctypes.data, n, out.ctypes.data if n else None)
    if rc != 0:
        raise FlyeGpuError(rc, L.fg_strerror(rc).decode())
    return out


def coverage_windows(seq_len, window, max_overhang):
    """fg_coverage_windows: (windows of the coverage vector of a sequence of seq_len bases -- chimera.cpp:114-117, at
    least 1 --, MAX_FLANK of :168-169, whether the vector is the degenerate {0})."""
    n, flank, deg = C.c_int32(), C.c_int32(), C.c_uint8()
    L = load_library()
    rc = L.fg_coverage_windows(int(seq_len), int(window), int(max_overhang), C.byref(n), C.byref(flank), C.byref(deg))
    if rc != 0:
        raise FlyeGpuError(rc, L.fg_strerror(rc).decode())
    return n.value, flank.value, bool(deg.value)


def coverage_verdict(params, n_windows, sums, median, min_good):
    """fg_coverage_verdict: testReadByCoverage's threshold and return value (chimera.cpp:153-182) per vector, from its
    size, sum, median and the minimum over its good range.  Returns (threshold int32, chimeric bool)."""
    nw = np.ascontiguousarray(n_windows, np.int32)
    sm = np.ascontiguousarray(sums, np.int64)
    md = np.ascontiguousarray(median, np.int32)
    mg = np.ascontiguousarray(min_good, np.int32)
    n = len(nw)
    if not (len(sm) == len(md) == len(mg) == n):
        raise ValueError("coverage_verdict: one value of each kind per vector")
    thr = np.zeros(n, np.int32)
    chim = np.zeros(n, np.uint8)
    L = load_library()
    rc = L.fg_coverage_verdict(C.byref(params), n, *(a.ctypes.data if n else None for a in (nw, sm, md, mg, thr, chim)))
    if rc != 0:
        raise FlyeGpuError(rc, L.fg_strerror(rc).decode())
    return thr, chim.astype(bool)


class SubstitutionMatrix:
    """The reference's SubstitutionMatrix (src/polishing/subs_matrix.cpp:58-104) as the 6 x 6 table of
    fg_subs_matrix_load; ``table`` is a numpy view of it."""

    def __init__(self, path=None, table=None):
        self.c = SubsMatrixStruct()
        if path is not None:
            rc = load_library().fg_subs_matrix_load(os.fsencode(path), C.byref(self.c))
            if rc != 0:
                raise FlyeGpuError(rc, f"fg_subs_matrix_load({path})")
        self.table = np.ctypeslib.as_array(self.c.score)
        if table is not None:
            self.table[:] = np.asarray(table, np.int64).reshape(6, 6)


class BubbleResult:
    """fg_bubble_batch copied out of its arena, arrays under the names of the header.  bubbles(i) gives the bubbles of
    contig i as (position, consensus bytes, [branch bytes])."""

    def __init__(self, **arrays):
        self.__dict__.update(arrays)

    def bubbles(self, i):
        cand, br = self.cand.tobytes(), self.branches.tobytes()
        out = []
        for b in range(int(self.bubble_off[i]), int(self.bubble_off[i + 1])):
            rs = range(int(self.bubble_branch_off[b]), int(self.bubble_branch_off[b + 1]))
            out.append((int(self.position[b]), cand[int(self.cand_off[b]):int(self.cand_off[b + 1])],
                        [br[int(self.branch_off[r]):int(self.branch_off[r + 1])] for r in rs]))
        return out

    def same_as(self, other):
        return self.__dict__.keys() == other.__dict__.keys() and all(
            (v is None and other.__dict__[k] is None) or np.array_equal(v, other.__dict__[k]) for k, v in self.__dict__.items())


class UniformResult(BubbleResult):
    """fg_uniform_result copied out of its arena: keep (uint8 per alignment), cov_threshold (per contig) and, with
    want_thresholds, wnd_off / wnd_threshold"""


class ConsensusResult(BubbleResult):
    """fg_consensus_batch copied out of its arena, arrays under the names of the header.  sequence(i) is the string
    _flatten_profile returns for contig i (bytes, possibly empty); insertion(p) the chosen string of profile position p."""

    def sequence(self, i):
        return self.seq[int(self.seq_off[i]):int(self.seq_off[i + 1])].tobytes()

    def insertion(self, p):
        return self.ins[int(self.ins_off[p]):int(self.ins_off[p + 1])].tobytes()


class ExpandResult(BubbleResult):
    """fg_expand_batch copied out of its arena, arrays under the names of the header (trg_cols / qry_cols None without
    want_cols).  columns(a) gives (aln.trg_seq, aln.qry_seq) of alignment a as bytes."""

    def columns(self, a):
        lo, hi = int(self.col_off[a]), int(self.col_off[a + 1])
        return self.trg_cols[lo:hi].tobytes(), self.qry_cols[lo:hi].tobytes()


class DivergenceResult(BubbleResult):
    """fg_divergence_batch copied out of its arena, arrays under the names of the header (the per-position arrays None
    without want_profile).  positions(i) gives contig i's four lists as the reference's dictionary."""

    def positions(self, i):
        return {k: [int(p) for p in getattr(self, k + "_pos")[int(getattr(self, k + "_off")[i]):int(getattr(self, k + "_off")[i + 1])]]
                for k in ("total", "sub", "del", "ins")}


class ConfirmResult(BubbleResult):
    """fg_confirm_batch copied out of its arena, arrays under the names of the header.  positions(j) gives job j's
    (confirmed, rejected) as the reference's dictionaries, consensus_pos(i) the list of edge i of the call."""

    def positions(self, j):
        part = lambda k: [int(p) for p in getattr(self, k + "_pos")[int(getattr(self, k + "_off")[j]):int(getattr(self, k + "_off")[j + 1])]]
        return tuple({k: part(pre + k) for k in ("total", "sub", "ins", "del")} for pre in ("conf_", "rej_"))

    def consensus_pos(self, i):
        return [int(p) for p in self.cons_pos[int(self.cons_off[i]):int(self.cons_off[i + 1])]]


class ClassifyResult(BubbleResult):
    """fg_classify_batch copied out of its arena, arrays under the names of the header (aln_score / aln_counted None
    without want_scores).  reads(j) gives job j's (status, top_edge, top_score, total_score) per read number."""

    def reads(self, j):
        lo, hi = int(self.read_off[j]), int(self.read_off[j + 1])
        return list(zip(self.status[lo:hi].tolist(), self.top_edge[lo:hi].tolist(), self.top_score[lo:hi].tolist(),
                        self.total_score[lo:hi].tolist()))


def cigar_parse(cigar):
    """fg_cigar_parse: the tokens of the reference's re "[0-9]+[MIDNSHP=X]" in a CIGAR (bytes) -> (ops uint8, lens uint32)"""
    L = load_library()
    cigar = bytes(cigar)
    cap = len(cigar) // 2 + 1
    ops, lens = np.zeros(cap, np.uint8), np.zeros(cap, np.uint32)
    n = C.c_uint64()
    rc = L.fg_cigar_parse(cigar, len(cigar), ops.ctypes.data, lens.ctypes.data, cap, C.byref(n))
    if rc != 0:
        raise FlyeGpuError(rc, "fg_cigar_parse: " + L.fg_strerror(rc).decode())
    return ops[:n.value], lens[:n.value]


class PafHits:
    """fg_paf_text copied out of its arena, for the PAF buffer `text`: `hits` (PAF_HIT_DTYPE, file order) with the ids
    of `names` (bytes, the distinct names of the file in ascending byte order); first_seen: the ids in order of first
    appearance, the query before the target of a line."""

    def __init__(self, text, hits, names, first_seen):
        self.text, self.hits, self.names, self.first_seen = text, hits, names, first_seen

    def name(self, i):
        return self.names[int(i)].decode()


def paf_parse(text):
    """fg_paf_parse on a whole PAF buffer (bytes) -> PafHits.  The tokens come from the library; the ids are numpy's:
    the names gathered into fixed-width byte strings, np.unique for the ranks."""
    L = load_library()
    text = bytes(text)
    b = PafText()
    t0 = time.perf_counter()
    rc = L.fg_paf_parse(text, len(text), C.byref(b))
    if rc != 0:
        raise FlyeGpuError(rc, L.fg_last_error(None).decode())
    t1 = time.perf_counter()
    n = int(b.n_hits)
    hits = np.zeros(n, PAF_HIT_DTYPE)
    if n == 0:
        L.fg_release_paf_text(C.byref(b))
        return PafHits(text, hits, [], np.zeros(0, np.uint32))
    take = lambda ptr: np.ctypeslib.as_array(ptr, (n,)).copy()
    for f in ("query_len", "query_start", "query_end", "target_len", "target_start", "target_end"):
        hits[f] = take(getattr(b, f))
    off = np.concatenate([take(b.query_name_off), take(b.target_name_off)]).astype(np.int64)
    ln = np.concatenate([take(b.query_name_len), take(b.target_name_len)]).astype(np.int64)
    L.fg_release_paf_text(C.byref(b))
    width = int(ln.max())
    raw = np.frombuffer(text, np.uint8)
    col = np.arange(width, dtype=np.int64)
    idx = np.minimum(off[:, None] + col[None, :], len(raw) - 1)
    table = np.where(col[None, :] < ln[:, None], raw[idx], 0).astype(np.uint8)
    keys = np.ascontiguousarray(table).view("S%d" % width).ravel()       # a name holds no NUL: no blank ends a field
    names, ids = np.unique(keys, return_inverse=True)
    ids = ids.ravel()
    hits["query"], hits["target"] = ids[:n], ids[n:]
    # position in file order: line i's query is 2 i, its target 2 i + 1
    pos = np.full(len(names), 2 * n, np.int64)
    np.minimum.at(pos, ids, np.concatenate([2 * np.arange(n), 2 * np.arange(n) + 1]))
    out = PafHits(text, hits, [bytes(x) for x in names.tolist()], np.argsort(pos, kind="stable").astype(np.uint32))
    out.parse_seconds, out.id_seconds = t1 - t0, time.perf_counter() - t1        # the tokeniser; the copies and the ids
    return out


class SamTextResult:
    """fg_sam_text copied out of its arena, for the SAM buffer `text` (the bytes the call saw): the counts n_lines,
    n_records, n_chunks, n_runs and one numpy array per field of the struct, under its name.  The status bits are
    FEW_TOKENS (fewer than 11 tokens: the token fields are 0), BAD_FLAG / BAD_POS (int() of the token bytes is the
    caller's), NO_SEQ (SEQ is '*') and RUN_OVERFLOW (a CIGAR length beyond uint32)."""
    FEW_TOKENS, BAD_FLAG, BAD_POS, NO_SEQ, RUN_OVERFLOW = 1, 2, 4, 8, 16
    PER_RECORD = ("line_no", "line_off", "line_len", "status", "tab_rname_off", "tab_rname_len", "qname_off", "qname_len", "rname_off",
                  "rname_len", "cigar_off", "cigar_len", "seq_off", "seq_len", "flag", "pos", "qry_start", "qry_end")
    ARRAYS = ("chunk_off",) + PER_RECORD + ("run_off", "run_op", "run_len")

    def __init__(self, text, **fields):
        self.text = text
        self.__dict__.update(fields)

    def token(self, i, which):
        """the bytes of record i's qname, rname, cigar, seq, tab_rname or line"""
        a = int(getattr(self, which + "_off")[i])
        return bytes(self.text[a:a + int(getattr(self, which + "_len")[i])])

    def runs(self, i):
        """(ops, lens) of record i, views"""
        a, b = int(self.run_off[i]), int(self.run_off[i + 1])
        return self.run_op[a:b], self.run_len[a:b]


class PolishResult:
    """fg_polish_batch copied out of its arena: candidates (bytes per bubble), n_steps, status, and with want_steps
    steps[i] = [(sequence bytes, score), ...]"""

    SKIPPED, OVERFLOW, ITER_LIMIT, FIXED = 1, 2, 4, 8

    def __init__(self, candidates, n_steps, status, steps):
        self.candidates, self.n_steps, self.status, self.steps = candidates, n_steps, status, steps


class ReadCoverage:
    """fg_coverage_batch copied out of its arena: win_off (n + 1), full / junction (None without want_vectors) and one
    value per query of sum, max, median, min_good, threshold, chimeric, degenerate."""

    def __init__(self, **arrays):
        self.__dict__.update(arrays)

    def full_of(self, q):
        return self.full[int(self.win_off[q]):int(self.win_off[q + 1])]

    def junction_of(self, q):
        return self.junction[int(self.win_off[q]):int(self.win_off[q + 1])]


class Context:
    """One fg_ctx: a SequenceContainer's reads resident in HBM on one GPU."""

    def __init__(self, kmer_size=17, device=0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.fg_create(C.byref(h), device, kmer_size)
        if rc != 0:
            raise FlyeGpuError(rc, self.L.fg_strerror(rc).decode())
        self.h = h
        self.k = kmer_size
        self.device = device
        self.first_id = 0
        self.n_reads = 0

    def _check(self, rc):
        if rc != 0:
            raise FlyeGpuError(rc, f"{self.L.fg_strerror(rc).decode()}: {self.L.fg_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):     # a group's member belongs to the group
                self.L.fg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_reads(self, rs, first_seq_id=0):
        self.rs = rs
        self.first_id = first_seq_id
        self.n_reads = rs.n
        self._check(self.L.fg_set_reads(self.h, rs.n, rs.words.ctypes.data, rs.word_off.ctypes.data,
                                        rs.length.ctypes.data, first_seq_id))

    def set_queries(self, rs, first_seq_id):
        """Second container holding the queries (reads vs graph edges, read_aligner.cpp:178-217)."""
        self.qrs = rs
        self._check(self.L.fg_set_queries(self.h, rs.n, rs.words.ctypes.data, rs.word_off.ctypes.data,
                                          rs.length.ctypes.data, first_seq_id))

    def debug_sort_pairs(self, keys, seg_off):
        """Device hit-sort kernel on independent segments; returns (sorted keys, permutation)."""
        k = np.ascontiguousarray(keys, np.uint64).copy()
        off = np.ascontiguousarray(seg_off, np.uint64)
        v = np.empty(len(k), np.uint32)
        for i in range(len(off) - 1):
            a, b = int(off[i]), int(off[i + 1])
            v[a:b] = np.arange(b - a, dtype=np.uint32)
        self._check(self.L.fg_debug_sort_pairs(self.h, k.ctypes.data, v.ctypes.data, off.ctypes.data,
                                               len(off) - 1))
        return k, v

    def debug_sort_pairs64(self, keys, vals, seg_off, cur_bits):
        """The hit sort in its 64-bit key + value form: keys ``ext_id << 32 | cur_pos`` with ``cur_pos < 2^cur_bits``,
        ``vals`` (uint32, one per key) travel with them.  Returns (sorted keys, their values)."""
        k = np.ascontiguousarray(keys, np.uint64).copy()
        v = np.ascontiguousarray(vals, np.uint32).copy()
        off = np.ascontiguousarray(seg_off, np.uint64)
        if len(v) != len(k) or len(k) != int(off[-1]):
            raise ValueError("one value per key, seg_off ending at their number")
        self._check(self.L.fg_debug_sort_pairs64(self.h, k.ctypes.data, v.ctypes.data, off.ctypes.data, len(off) - 1,
                                                 int(cur_bits)))
        return k, v

    def debug_sort_packed(self, keys, vals, seg_off, cur_bits):
        """The hit sort on packed records ``key << 24 | val`` (key = ``record << cur_bits | cur_pos``, val below 2^24),
        which are ordered on the key alone.  Returns (sorted keys, their values), unpacked."""
        k = np.ascontiguousarray(keys, np.uint64)
        v = np.ascontiguousarray(vals, np.uint64)
        off = np.ascontiguousarray(seg_off, np.uint64)
        if len(v) != len(k) or len(k) != int(off[-1]):
            raise ValueError("one value per key, seg_off ending at their number")
        if len(k) and (int(k.max()) >> 40 or int(v.max()) >> 24):
            raise ValueError("a key of more than 40 bits or a value of more than 24")
        rec = np.ascontiguousarray((k << np.uint64(24)) | v)
        self._check(self.L.fg_debug_sort_packed(self.h, rec.ctypes.data, off.ctypes.data, len(off) - 1, int(cur_bits)))
        return rec >> np.uint64(24), (rec & np.uint64(0xFFFFFF)).astype(np.uint32)

    def debug_sort_pairs32(self, keys, seg_off, cur_bits, rec_bits, tie_free=None):
        """The hit sort in its 32-bit key form (``record << cur_bits | cur_pos``) with per-segment tie-free flags
        (None: no flags).  Returns (sorted keys, permutation, segments on the radix path, hits on the radix path)."""
        k = np.ascontiguousarray(keys, np.uint32).copy()
        off = np.ascontiguousarray(seg_off, np.uint64)
        v = np.empty(len(k), np.uint32)
        for i in range(len(off) - 1):
            a, b = int(off[i]), int(off[i + 1])
            v[a:b] = np.arange(b - a, dtype=np.uint32)
        flags = None if tie_free is None else np.ascontiguousarray(tie_free, np.uint32)
        if flags is not None and len(flags) != len(off) - 1:
            raise ValueError("one tie-free flag per segment")
        segs, hits = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fg_debug_sort_pairs32(self.h, k.ctypes.data, v.ctypes.data, off.ctypes.data, len(off) - 1,
                                                 int(cur_bits), int(rec_bits),
                                                 None if flags is None else flags.ctypes.data,
                                                 C.byref(segs), C.byref(hits)))
        return k, v, int(segs.value), int(hits.value)

    def debug_sort_pairs32_val16(self, keys, vals, seg_off, cur_bits, rec_bits, tie_free=None):
        """``debug_sort_pairs32`` in the 16-bit value form: ``vals`` (uint16, one per key) travel with the keys.
        Returns (sorted keys, their values, segments on the radix path, hits on the radix path)."""
        k = np.ascontiguousarray(keys, np.uint32).copy()
        v = np.ascontiguousarray(vals, np.uint16).copy()
        off = np.ascontiguousarray(seg_off, np.uint64)
        if len(v) != len(k) or len(k) != int(off[-1]):
            raise ValueError("one value per key, seg_off ending at their number")
        flags = None if tie_free is None else np.ascontiguousarray(tie_free, np.uint32)
        if flags is not None and len(flags) != len(off) - 1:
            raise ValueError("one tie-free flag per segment")
        segs, hits = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fg_debug_sort_pairs32_val16(self.h, k.ctypes.data, v.ctypes.data, off.ctypes.data, len(off) - 1,
                                                       int(cur_bits), int(rec_bits),
                                                       None if flags is None else flags.ctypes.data,
                                                       C.byref(segs), C.byref(hits)))
        return k, v, int(segs.value), int(hits.value)

    def debug_hit_val16(self):
        """Whether the last sub-range of queries this context expanded carried 16-bit target positions."""
        n = C.c_uint32(0)
        self._check(self.L.fg_debug_hit_val16(self.h, C.byref(n)))
        return bool(n.value)

    def debug_tie_free(self, max_n):
        """The seed expansion's tie-free flags of the last sub-range of queries this context expanded: (index of its
        first query in the call's list, flags).  No flags (empty) on the receiver path and for 64-bit key forms."""
        out = np.zeros(max(int(max_n), 1), np.uint32)
        q0, n = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.fg_debug_tie_free(self.h, out.ctypes.data, int(max_n), C.byref(q0), C.byref(n)))
        if n.value > max_n:
            raise ValueError(f"{n.value} flags, room for {max_n}")
        return int(q0.value), out[:n.value].copy()

    def debug_sort_screen(self, keys, seg_off, cur_bits, rec_bits, tie_free, min_unique, min_overlap):
        """The hit sort's screen (k_sort_screen) on segments of 32-bit keys ``record << cur_bits | cur_pos`` in emission
        order, with the tie-free flag of each: one reason word per segment (0 not screened, 1 order-free, 2 a tied group
        may pass the chaining prefilter's ``min_unique`` / ``min_overlap``, 3 too many tied records)."""
        k = np.ascontiguousarray(keys, np.uint32)
        off = np.ascontiguousarray(seg_off, np.uint64)
        flags = np.ascontiguousarray(tie_free, np.uint32)
        if len(flags) != len(off) - 1:
            raise ValueError("one tie-free flag per segment")
        if len(k) != int(off[-1]):
            raise ValueError("seg_off does not end at the number of keys")
        out = np.zeros(max(len(off) - 1, 1), np.uint32)
        self._check(self.L.fg_debug_sort_screen(self.h, k.ctypes.data, off.ctypes.data, len(off) - 1, int(cur_bits),
                                                int(rec_bits), flags.ctypes.data, float(np.float32(min_unique)),
                                                int(min_overlap), out.ctypes.data))
        return out[:len(off) - 1].copy()

    def debug_order_free(self, max_n):
        """The screen's reason words for the queries ``debug_tie_free`` speaks of: (index of the first query in the
        call's list, reasons).  Empty where the screen did not run."""
        out = np.zeros(max(int(max_n), 1), np.uint32)
        q0, n = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.fg_debug_order_free(self.h, out.ctypes.data, int(max_n), C.byref(q0), C.byref(n)))
        if n.value > max_n:
            raise ValueError(f"{n.value} reason words, room for {max_n}")
        return int(q0.value), out[:n.value].copy()

    def debug_sort_radix_segments(self):
        """Segments the last hit sort on this context sent to the radix path."""
        n = C.c_uint32(0)
        self._check(self.L.fg_debug_sort_radix_segments(self.h, C.byref(n)))
        return int(n.value)

    def debug_freq_accumulate(self, dst, src):
        """k_freq_accumulate on the device: ``dst += src`` in place over uint32 (wrapping).  The device copies sit at
        the same offset inside 16 bytes as the host arrays do: a view that starts off a boundary takes the unaligned
        path."""
        assert dst.dtype == np.uint32 and src.dtype == np.uint32 and len(dst) == len(src)
        assert dst.flags.c_contiguous and src.flags.c_contiguous
        self._check(self.L.fg_debug_freq_accumulate(self.h, dst.ctypes.data, src.ctypes.data, len(dst)))
        return dst

    def debug_scan(self, data, inclusive=False, in_place=True):
        """fgprim::scan on the device over a uint32 / uint64 array (sums modulo 2^width); returns a new array."""
        assert data.dtype in (np.uint32, np.uint64)
        out = np.ascontiguousarray(data).copy()
        self._check(self.L.fg_debug_scan(self.h, out.ctypes.data if len(out) else None, len(out), out.dtype.itemsize,
                                         int(bool(inclusive)), int(bool(in_place))))
        return out

    def debug_radix_sort_pairs(self, keys, vals, begin_bit, end_bit):
        """fgprim::radixSortPairs on the device: stable by bits [begin_bit, end_bit) of the uint64 keys; returns
        (keys, values, onesweep passes launched)."""
        k = np.ascontiguousarray(keys, np.uint64).copy()
        v = np.ascontiguousarray(vals, np.uint64).copy()
        assert len(k) == len(v)
        passes = C.c_int(-1)
        self._check(self.L.fg_debug_radix_sort_pairs(self.h, k.ctypes.data if len(k) else None,
                                                     v.ctypes.data if len(v) else None, len(k), begin_bit, end_bit,
                                                     C.byref(passes)))
        return k, v, int(passes.value)

    def debug_probe_skip_check(self):
        """The probe skip's invariant over all indexed reads: (positions whose "frequent enough for a slot" bit is
        clear, those of them whose k-mer has a slot in the lookup table all the same -- always 0).  (0, 0) where the
        context holds no such bits."""
        clear, bad = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.fg_debug_probe_skip_check(self.h, C.byref(clear), C.byref(bad)))
        return int(clear.value), int(bad.value)

    def debug_table(self):
        """The lookup table of the context's index (fg_debug_table): dict of ``wide``, ``n_parts``, ``n_slots``, the
        per-part ``bound`` (n_parts + 1), ``slot_base``, ``key_base``, ``groups`` and ``slots``: the slot words, or for
        the wide form an (n_slots, 2) array of (key, key index)."""
        wide, parts, n = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        self._check(self.L.fg_debug_table(self.h, C.byref(wide), C.byref(parts), C.byref(n), None, None, None, None, None))
        p = int(parts.value)
        bound, base, kbase = np.zeros(p + 1, np.uint64), np.zeros(p, np.uint64), np.zeros(p, np.uint64)
        groups = np.zeros(p, np.uint32)
        slots = np.zeros(max(1, int(n.value) * (2 if wide.value else 1)), np.uint64)
        self._check(self.L.fg_debug_table(self.h, None, None, None, bound.ctypes.data, base.ctypes.data, kbase.ctypes.data,
                                          groups.ctypes.data, slots.ctypes.data))
        slots = slots[:int(n.value) * (2 if wide.value else 1)]
        return dict(wide=bool(wide.value), n_parts=p, n_slots=int(n.value), bound=bound, slot_base=base, key_base=kbase,
                    groups=groups, slots=slots.reshape(-1, 2) if wide.value else slots)

    def debug_chain_lazy(self):
        """How the groups of the last fg_overlaps call left the chaining stage's backtracking: dict of ``entered``,
        ``fast`` (primary taken straight from the DP tables), ``no_live`` (no chain start) and the fallbacks to the
        full path ``tied_top``, ``root`` and ``overlap_test``."""
        out = (C.c_uint64 * 6)()
        self._check(self.L.fg_debug_chain_lazy(self.h, out))
        return dict(zip(("entered", "fast", "no_live", "tied_top", "root", "overlap_test"), (int(x) for x in out)))

    def debug_edit_distances(self, n_pairs, use_hpc=False):
        """Device edit-distance kernels on the pairs (read 2i, read 2i+1) of the container;
        returns (distances, lengths of A, lengths of B)."""
        d = np.empty(n_pairs, np.int32)
        la = np.empty(n_pairs, np.int32)
        lb = np.empty(n_pairs, np.int32)
        self._check(self.L.fg_debug_edit_distances(self.h, n_pairs, int(bool(use_hpc)), d.ctypes.data,
                                                   la.ctypes.data, lb.ctypes.data))
        return d, la, lb

    def align_cigar_ksw(self, pairs, arrays=False):
        """getAlignmentCigarKsw (alignment.cpp:102-216) of (target, query) pairs of 0..3 arrays on the device:
        list of (error-rate bit pattern as hex, CIGAR text "<len><op> ..."); arrays = True: the batch's arrays instead
        (run offsets, ops, lens, error-rate bit patterns)."""
        n = len(pairs)
        trg = np.concatenate([np.asarray(a, np.uint8) for a, _ in pairs]) if n else np.empty(0, np.uint8)
        qry = np.concatenate([np.asarray(b, np.uint8) for _, b in pairs]) if n else np.empty(0, np.uint8)
        toff = np.zeros(n + 1, np.uint64)
        qoff = np.zeros(n + 1, np.uint64)
        toff[1:] = np.cumsum([len(a) for a, _ in pairs])
        qoff[1:] = np.cumsum([len(b) for _, b in pairs])
        trg = np.ascontiguousarray(trg if len(trg) else np.zeros(1, np.uint8))
        qry = np.ascontiguousarray(qry if len(qry) else np.zeros(1, np.uint8))
        b = CigarBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_align_cigar_ksw(self.h, n, trg.ctypes.data, toff.ctypes.data, qry.ctypes.data,
                                              qoff.ctypes.data, C.byref(b)))
        self.last_align_seconds = time.perf_counter() - t0      # the C call alone (the text below is test harness)
        out = self._cigar_result(b, n, arrays)
        self.L.fg_release_cigars(C.byref(b))
        return out

    @staticmethod
    def _cigar_result(b, n, arrays):
        """Copies of a fg_cigar_batch: (run_off, ops, lens, error-rate bit patterns) as arrays, or the list of
        (error-rate bit pattern as hex, CIGAR text) per pair."""
        run_off = np.ctypeslib.as_array(b.run_off, (n + 1,)).copy() if n else np.zeros(1, np.uint64)
        total = int(run_off[n])
        ops = np.ctypeslib.as_array(b.ops, (total,)).copy() if total else np.empty(0, np.uint8)
        lens = np.ctypeslib.as_array(b.lens, (total,)).copy() if total else np.empty(0, np.int32)
        bits = np.ctypeslib.as_array(b.err_rate, (n,)).copy().view(np.uint32) if n else np.empty(0, np.uint32)
        if arrays:
            return run_off, ops, lens, bits
        out = []
        for i in range(n):
            a0, a1 = int(run_off[i]), int(run_off[i + 1])
            out.append((f"{int(bits[i]):08x}", " ".join(f"{lens[k]}{chr(ops[k])}" for k in range(a0, a1))))
        return out

    @staticmethod
    def _range_pairs(pairs):
        """The fg_range_pair table of (n, 6) integers or of a record array with those fields."""
        pairs = np.asarray(pairs)
        tab = np.zeros(len(pairs), RANGE_PAIR_DTYPE)
        if pairs.dtype.names:
            for f in RANGE_PAIR_DTYPE.names:
                tab[f] = pairs[f]
        elif len(pairs):
            if pairs.ndim != 2 or pairs.shape[1] != 6 or pairs.dtype.kind not in "iu":
                raise ValueError("pairs: an (n, 6) integer array or a record array")
            if (pairs[:, :2] < 0).any() or (pairs[:, :2] > 0xFFFFFFFF).any() or (abs(pairs[:, 2:]) > 0x7FFFFFFF).any():
                raise ValueError("pairs: ids are uint32, positions int32")
            for j, f in enumerate(RANGE_PAIR_DTYPE.names):
                tab[f] = pairs[:, j]
        return tab

    def align_ranges(self, pairs, use_hpc=False, arrays=False):
        """fg_align_ranges: getAlignmentCigarKsw of ranges of the resident sequences, cut out (and, with use_hpc,
        homopolymer-compressed) on the device.  pairs: (n, 6) integers (cur_id, ext_id, cur_begin, cur_end, ext_begin,
        ext_end) or a record array with those fields (the records of an OverlapResult).  Returns (what align_cigar_ksw
        returns for those strings, aligned lengths of the cur side, of the ext side)."""
        tab = self._range_pairs(pairs)
        n = len(tab)
        len_cur = np.zeros(n, np.int32)
        len_ext = np.zeros(n, np.int32)
        b = CigarBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_align_ranges(self.h, tab.ctypes.data if n else None, n, int(bool(use_hpc)), C.byref(b),
                                           len_cur.ctypes.data if n else None, len_ext.ctypes.data if n else None))
        self.last_align_seconds = time.perf_counter() - t0
        out = self._cigar_result(b, n, arrays)
        self.L.fg_release_cigars(C.byref(b))
        return out, len_cur, len_ext

    def trim_ranges(self, pairs_or_recs, use_hpc, max_divergence, min_overlap):
        """fg_trim_ranges: checkIdyAndTrim (alignment.cpp:306-495) of ranges of the resident sequences, on the device.
        pairs_or_recs as for align_ranges.  Returns (rec_off, recs): the pieces of pair i are recs[rec_off[i]:
        rec_off[i + 1]] (TRIM_REC_DTYPE), in the order the reference returns them."""
        tab = self._range_pairs(pairs_or_recs)
        n = len(tab)
        b = TrimBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_trim_ranges(self.h, tab.ctypes.data if n else None, n, int(bool(use_hpc)),
                                          float(np.float32(max_divergence)), int(min_overlap), C.byref(b)))
        self.last_trim_seconds = time.perf_counter() - t0
        rec_off = np.ctypeslib.as_array(b.rec_off, (n + 1,)).copy() if b.rec_off else np.zeros(n + 1, np.uint64)
        total = int(rec_off[n])
        recs = np.empty(total, TRIM_REC_DTYPE)
        if total:
            C.memmove(recs.ctypes.data, b.recs, total * TRIM_REC_DTYPE.itemsize)
        self.L.fg_release_trims(C.byref(b))
        return rec_off, recs

    def edit_ranges(self, pairs_or_recs, use_hpc=False):
        """fg_edit_ranges: getAlignmentErrEdlib (alignment.cpp:218-247) of ranges of the resident sequences, on the
        device.  pairs_or_recs as for align_ranges.  Returns (edit distances, compared lengths of the cur side, of the
        ext side, divergence = float32(dist) / float32(max(lengths)); NaN for two empty strings)."""
        tab = self._range_pairs(pairs_or_recs)
        n = len(tab)
        dist = np.zeros(n, np.int32)
        len_cur = np.zeros(n, np.int32)
        len_ext = np.zeros(n, np.int32)
        div = np.zeros(n, np.float32)
        t0 = time.perf_counter()
        self._check(self.L.fg_edit_ranges(self.h, tab.ctypes.data if n else None, n, int(bool(use_hpc)),
                                          *(a.ctypes.data if n else None for a in (dist, len_cur, len_ext, div))))
        self.last_edit_seconds = time.perf_counter() - t0
        return dist, len_cur, len_ext, div

    def chain_alignments(self, recs, query_off, params, first_ext_id, node_left, node_right):
        """fg_chain_alignments: the filter, the std::sort by curBegin and chainReadAlignments (read_aligner.cpp:24-154,
        :219-236) for the per-read lists recs[query_off[q]:query_off[q + 1]] (REC_DTYPE, any order).  node_left /
        node_right: the nodes of the edge that owns indexed sequence first_ext_id + i.  Returns (chain_off, aln_off, aln,
        score): the chains of query q are chain_off[q] .. chain_off[q + 1], chain c holds recs[aln[aln_off[c]:
        aln_off[c + 1]]], front first, with Chain::score score[c]."""
        r = np.ascontiguousarray(recs, REC_DTYPE)
        off = np.ascontiguousarray(query_off, np.uint64)
        nl = np.ascontiguousarray(node_left, np.uint32)
        nr = np.ascontiguousarray(node_right, np.uint32)
        if len(off) < 1 or len(nl) != len(nr) or (len(off) > 1 and int(off.max()) > len(r)):
            raise ValueError("chain_alignments: offsets inside the records, one node pair per indexed sequence id")
        nq = len(off) - 1
        b = ChainBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_chain_alignments(self.h, C.byref(params), r.ctypes.data if len(r) else None, off.ctypes.data, nq,
                                               int(first_ext_id), len(nl), nl.ctypes.data if len(nl) else None,
                                               nr.ctypes.data if len(nr) else None, C.byref(b)))
        self.last_chain_seconds = time.perf_counter() - t0
        nc, na = int(b.n_chains), int(b.n_alns)
        out = (np.ctypeslib.as_array(b.chain_off, (nq + 1,)).copy(), np.ctypeslib.as_array(b.aln_off, (nc + 1,)).copy(),
               np.ctypeslib.as_array(b.aln, (na,)).copy() if na else np.zeros(0, np.uint64),
               np.ctypeslib.as_array(b.score, (nc,)).copy() if nc else np.zeros(0, np.int32))
        self.L.fg_release_chains(C.byref(b))
        return out

    def read_coverage(self, recs, query_off, query_len, params):
        """fg_read_coverage: the window coverage of ChimeraDetector::getReadCoverage / getCachedCoverage
        (chimera.cpp:106-134, :280-343) and testReadByCoverage's values (:137-202) for the per-read lists
        recs[query_off[q]:query_off[q + 1]] (REC_DTYPE, any order) of reads of query_len[q] bases.  Returns a
        ReadCoverage of numpy arrays."""
        r = np.ascontiguousarray(recs, REC_DTYPE)
        off = np.ascontiguousarray(query_off, np.uint64)
        ln = np.ascontiguousarray(query_len, np.int32)
        if len(off) != len(ln) + 1 or (len(off) > 1 and int(off.max()) > len(r)):
            raise ValueError("read_coverage: one length per query, offsets inside the records")
        nq = len(ln)
        b = CoverageBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_read_coverage(self.h, C.byref(params), r.ctypes.data if len(r) else None, off.ctypes.data, nq,
                                            ln.ctypes.data if nq else None, C.byref(b)))
        self.last_coverage_seconds = time.perf_counter() - t0

        def take(ptr, n, dtype):
            return np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dtype)

        win_off = np.ctypeslib.as_array(b.win_off, (nq + 1,)).copy()
        nw = int(win_off[nq])
        vec = bool(params.want_vectors)
        out = ReadCoverage(win_off=win_off, full=take(b.full, nw, np.int32) if vec else None,
                           junction=take(b.junction, nw, np.int32) if vec else None, sum=take(b.sum, nq, np.int64),
                           max=take(b.max, nq, np.int32), median=take(b.median, nq, np.int32),
                           min_good=take(b.min_good, nq, np.int32), threshold=take(b.threshold, nq, np.int32),
                           chimeric=take(b.chimeric, nq, np.uint8).astype(bool),
                           degenerate=take(b.degenerate, nq, np.uint8).astype(bool))
        self.L.fg_release_coverage(C.byref(b))
        return out

    def polish_bubbles(self, matrix, cand, cand_off, branches, branch_off, bubble_branch_off, fix_dinucleotides=True,
                       want_steps=True):
        """fg_polish_bubbles: GeneralPolisher::polishBubble and DinucleotideFixer::fixBubble for bubbles given as flat
        bytes with offsets (bubble i: cand[cand_off[i]:cand_off[i + 1]], branches bubble_branch_off[i] ..
        bubble_branch_off[i + 1], branch r = branches[branch_off[r]:branch_off[r + 1]]).  Returns a PolishResult."""
        cb = np.frombuffer(bytes(cand), np.uint8)
        bb = np.frombuffer(bytes(branches), np.uint8)
        co = np.ascontiguousarray(cand_off, np.uint64)
        bo = np.ascontiguousarray(branch_off, np.uint64)
        bbo = np.ascontiguousarray(bubble_branch_off, np.uint64)
        n = len(co) - 1
        if n < 0 or len(bbo) != n + 1 or (n and (int(co.max()) > len(cb) or int(bbo.max()) + 1 > len(bo))) or \
                (len(bo) and int(bo.max()) > len(bb)):
            raise ValueError("polish_bubbles: offsets outside their arrays")
        b = PolishBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_polish_bubbles(self.h, C.byref(matrix.c), cb.ctypes.data if len(cb) else None, co.ctypes.data,
                                             bb.ctypes.data if len(bb) else None, bo.ctypes.data if len(bo) else None,
                                             bbo.ctypes.data, n, int(bool(fix_dinucleotides)), int(bool(want_steps)), C.byref(b)))
        self.last_polish_seconds = time.perf_counter() - t0

        def take(ptr, k, dtype):
            return np.ctypeslib.as_array(ptr, (k,)).copy() if k else np.zeros(0, dtype)

        off = take(b.cand_off, n + 1, np.uint64)
        raw = take(b.cand, int(off[n]), np.uint8).tobytes()
        cands = [raw[int(off[i]):int(off[i + 1])] for i in range(n)]
        n_steps, status = take(b.n_steps, n, np.uint32), take(b.status, n, np.uint8)
        steps = None
        if want_steps:
            so = take(b.step_off, n + 1, np.uint64)
            ns = int(so[n])
            sso = take(b.step_seq_off, ns + 1, np.uint64)
            sraw = take(b.step_seq, int(sso[ns]), np.uint8).tobytes()
            score = take(b.step_score, ns, np.int64)
            steps = [[(sraw[int(sso[t]):int(sso[t + 1])], int(score[t])) for t in range(int(so[i]), int(so[i + 1]))]
                     for i in range(n)]
        self.L.fg_release_polish(C.byref(b))
        return PolishResult(cands, n_steps, status, steps)

    def make_bubbles(self, params, contig_len, contig_circular, contig_aln_off, trg_start, trg_end, err_rate, col_off,
                     trg_cols, qry_cols, want_profile=False):
        """fg_make_bubbles: the reference's bubbles.py from _compute_profile onward for a batch of contigs.  Contig i has
        the alignments contig_aln_off[i] .. contig_aln_off[i + 1]; alignment a has the columns col_off[a] .. col_off[a + 1]
        of the gapped strings trg_cols / qry_cols (bytes, '-' the gap).  Returns a BubbleResult."""
        cl = np.ascontiguousarray(contig_len, np.int32)
        n = len(cl)
        cc = np.ascontiguousarray(contig_circular, np.uint8) if contig_circular is not None else np.zeros(n, np.uint8)
        cao = np.ascontiguousarray(contig_aln_off, np.uint64)
        ts, te = np.ascontiguousarray(trg_start, np.int32), np.ascontiguousarray(trg_end, np.int32)
        er = np.ascontiguousarray(err_rate, np.float64)
        co = np.ascontiguousarray(col_off, np.uint64)
        tc, qc = np.frombuffer(bytes(trg_cols), np.uint8), np.frombuffer(bytes(qry_cols), np.uint8)
        if len(cao) != n + 1 or len(cc) != n or len(tc) != len(qc) or len(ts) != len(te) or len(ts) != len(er) or \
                (n and int(cao.max()) > len(ts)) or (len(ts) and len(co) != len(ts) + 1) or (len(co) and int(co.max()) > len(tc)):
            raise ValueError("make_bubbles: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if len(a) else None
        b = BubbleBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_make_bubbles(self.h, C.byref(params), n, ptr(cl), ptr(cc), cao.ctypes.data, ptr(ts), ptr(te), ptr(er),
                                           ptr(co), ptr(tc), ptr(qc), int(bool(want_profile)), C.byref(b)))
        self.last_bubbles_seconds = time.perf_counter() - t0

        return self._bubble_result(b, n, want_profile)

    def _bubble_result(self, b, n, want_profile):
        """the arrays of a struct fg_bubble_batch as a BubbleResult; releases the batch"""
        def take(p, k, dtype):
            return np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, dtype)

        nb = int(b.n_bubbles)
        bbo = take(b.bubble_branch_off, nb + 1, np.uint64)
        bro = take(b.branch_off, int(bbo[nb]) + 1, np.uint64)
        cdo = take(b.cand_off, nb + 1, np.uint64)
        out = dict(bubble_off=take(b.bubble_off, n + 1, np.uint64), position=take(b.position, nb, np.int32),
                   cand=take(b.cand, int(cdo[nb]), np.uint8), cand_off=cdo, branches=take(b.branches, int(bro[-1]), np.uint8),
                   branch_off=bro, bubble_branch_off=bbo, n_long_bubbles=take(b.n_long_bubbles, n, np.int32),
                   n_empty=take(b.n_empty, n, np.int32), n_long_branch=take(b.n_long_branch, n, np.int32),
                   mean_cov=take(b.mean_cov, n, np.int64), n_partition=take(b.n_partition, n, np.int32),
                   in_profile=take(b.in_profile, int(b.n_alignments), np.uint8))
        for k in ("part_off", "partition", "prof_off", "coverage", "num_inserts", "num_deletions", "num_missmatch", "nucl"):
            out[k] = None
        if want_profile:
            out["part_off"], out["prof_off"] = take(b.part_off, n + 1, np.uint64), take(b.prof_off, n + 1, np.uint64)
            out["partition"] = take(b.partition, int(out["part_off"][n]), np.int32)
            npos = int(out["prof_off"][n])
            for k in ("coverage", "num_inserts", "num_deletions", "num_missmatch"):
                out[k] = take(getattr(b, k), npos, np.int32)
            out["nucl"] = take(b.nucl, npos, np.uint8)
        self.L.fg_release_bubbles(C.byref(b))
        return BubbleResult(**out)

    def uniform_alignments(self, contig_len, contig_aln_off, trg_start, trg_end, err_rate, is_secondary=None,
                           want_thresholds=False):
        """fg_uniform_alignments: get_uniform_alignments (flye/polishing/alignment.py:95-153) for a batch of contigs in the
        layout of make_bubbles.  Returns a UniformResult; keep goes into contig_consensus as ``use``."""
        cl = np.ascontiguousarray(contig_len, np.int32)
        n = len(cl)
        cao = np.ascontiguousarray(contig_aln_off, np.uint64)
        ts, te = np.ascontiguousarray(trg_start, np.int32), np.ascontiguousarray(trg_end, np.int32)
        er = np.ascontiguousarray(err_rate, np.float64)
        sec = np.ascontiguousarray(is_secondary, np.uint8) if is_secondary is not None else None
        if len(cao) != n + 1 or len(ts) != len(te) or len(ts) != len(er) or (sec is not None and len(sec) != len(ts)) or \
                (n and int(cao.max()) > len(ts)):
            raise ValueError("uniform_alignments: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        r = UniformResultStruct()
        t0 = time.perf_counter()
        self._check(self.L.fg_uniform_alignments(self.h, n, ptr(cl), cao.ctypes.data, ptr(ts), ptr(te), ptr(er), ptr(sec),
                                                 int(bool(want_thresholds)), C.byref(r)))
        self.last_uniform_seconds = time.perf_counter() - t0

        def take(p, k, dtype):
            return np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, dtype)

        out = dict(keep=take(r.keep, int(r.n_alignments), np.uint8), cov_threshold=take(r.cov_threshold, n, np.int32),
                   wnd_off=None, wnd_threshold=None)
        if want_thresholds:
            out["wnd_off"] = take(r.wnd_off, n + 1, np.uint64)
            out["wnd_threshold"] = take(r.wnd_threshold, int(out["wnd_off"][n]), np.float64)
        self.L.fg_release_uniform(C.byref(r))
        return UniformResult(**out)

    def contig_consensus(self, contig_len, contig_aln_off, trg_start, qry_id, col_off, trg_cols, qry_cols, use=None,
                         want_profile=False):
        """fg_contig_consensus: _contig_profile (after get_uniform_alignments) and _flatten_profile of the reference's
        flye/polishing/consensus.py for a batch of contigs in the layout of make_bubbles; qry_id numbers the reads, use
        (uint8 per alignment, None: all) selects the alignments that take part.  Returns a ConsensusResult."""
        cl = np.ascontiguousarray(contig_len, np.int32)
        n = len(cl)
        cao = np.ascontiguousarray(contig_aln_off, np.uint64)
        ts, qi = np.ascontiguousarray(trg_start, np.int32), np.ascontiguousarray(qry_id, np.int32)
        us = np.ascontiguousarray(use, np.uint8) if use is not None else None
        co = np.ascontiguousarray(col_off, np.uint64)
        tc, qc = np.frombuffer(bytes(trg_cols), np.uint8), np.frombuffer(bytes(qry_cols), np.uint8)
        if len(cao) != n + 1 or len(tc) != len(qc) or len(ts) != len(qi) or (us is not None and len(us) != len(ts)) or \
                (n and int(cao.max()) > len(ts)) or (len(ts) and len(co) != len(ts) + 1) or (len(co) and int(co.max()) > len(tc)):
            raise ValueError("contig_consensus: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        b = ConsensusBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_contig_consensus(self.h, n, ptr(cl), cao.ctypes.data, ptr(ts), ptr(qi), ptr(us), ptr(co), ptr(tc),
                                               ptr(qc), int(bool(want_profile)), C.byref(b)))
        self.last_consensus_seconds = time.perf_counter() - t0

        return self._consensus_result(b, n, want_profile)

    def _consensus_result(self, b, n, want_profile):
        """the arrays of a struct fg_consensus_batch as a ConsensusResult; releases the batch"""
        def take(p, k, dtype):
            return np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, dtype)

        so = take(b.seq_off, n + 1, np.uint64)
        out = dict(seq_off=so, seq=take(b.seq, int(so[n]), np.uint8))
        for k in ("prof_off", "nucl", "match_total", "num_ins", "max_match", "accepted", "ins_off", "ins"):
            out[k] = None
        if want_profile:
            out["prof_off"] = take(b.prof_off, n + 1, np.uint64)
            npos = int(out["prof_off"][n])
            for k, t in (("nucl", np.uint8), ("match_total", np.int32), ("num_ins", np.int32), ("max_match", np.uint8),
                         ("accepted", np.uint8)):
                out[k] = take(getattr(b, k), npos, t)
            out["ins_off"] = np.ctypeslib.as_array(b.ins_off, (npos + 1,)).copy()
            out["ins"] = take(b.ins, int(out["ins_off"][npos]), np.uint8)
        self.L.fg_release_consensus(C.byref(b))
        return ConsensusResult(**out)

    def divergence_profile(self, sub_thresh, del_thresh, ins_thresh, contig_len, contig_aln_off, trg_start, col_off, trg_cols,
                           qry_cols, want_profile=False):
        """fg_divergence_profile: _contig_profile, _count_freqs and _call_position of the reference's
        flye/trestle/divergence.py for a batch of contigs in the layout of make_bubbles; every alignment takes part.
        Returns a DivergenceResult."""
        cl = np.ascontiguousarray(contig_len, np.int32)
        n = len(cl)
        cao = np.ascontiguousarray(contig_aln_off, np.uint64)
        ts = np.ascontiguousarray(trg_start, np.int32)
        co = np.ascontiguousarray(col_off, np.uint64)
        tc, qc = np.frombuffer(bytes(trg_cols), np.uint8), np.frombuffer(bytes(qry_cols), np.uint8)
        if len(cao) != n + 1 or len(tc) != len(qc) or (n and int(cao.max()) > len(ts)) or (len(ts) and len(co) != len(ts) + 1) or \
                (len(co) and int(co.max()) > len(tc)):
            raise ValueError("divergence_profile: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        b = DivergenceBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_divergence_profile(self.h, float(sub_thresh), float(del_thresh), float(ins_thresh), n, ptr(cl),
                                                 cao.ctypes.data, ptr(ts), ptr(co), ptr(tc), ptr(qc), int(bool(want_profile)),
                                                 C.byref(b)))
        self.last_divergence_seconds = time.perf_counter() - t0
        return self._divergence_result(b, n, want_profile)

    def _divergence_result(self, b, n, want_profile):
        def take(p, k, dtype):
            return np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, dtype)

        out = {}
        for k in ("total", "sub", "del", "ins"):
            out[k + "_off"] = take(getattr(b, k + "_off"), n + 1, np.uint64)
            out[k + "_pos"] = take(getattr(b, k + "_pos"), int(out[k + "_off"][n]), np.int32)
        profile = (("cov", np.int32), ("nucl", np.uint8), ("mat_ct", np.int32), ("sub_base", np.uint8), ("sub_ct", np.int32),
                   ("del_ct", np.int32), ("ins_base", np.uint8), ("ins_ct", np.int32), ("flags", np.uint8))
        out["prof_off"] = None
        for k, _ in profile:
            out[k] = None
        if want_profile:
            out["prof_off"] = take(b.prof_off, n + 1, np.uint64)
            npos = int(out["prof_off"][n])
            for k, t in profile:
                out[k] = take(getattr(b, k), npos, t)
        self.L.fg_release_divergence(C.byref(b))
        return DivergenceResult(**out)

    def confirm_positions(self, side, job_edge_off, trg_start, trg_end, qry_start, col_off, trg_cols, qry_cols, total_off, total_pos,
                          sub_off, sub_pos, del_off, del_pos, ins_off, ins_pos):
        """fg_confirm_positions: _evaluate_positions of the reference's flye/trestle/trestle.py for a batch of jobs, one
        collapsed consensus alignment per edge.  Returns a ConfirmResult."""
        sd = np.ascontiguousarray(side, np.uint8)
        n = len(sd)
        jeo, co = np.ascontiguousarray(job_edge_off, np.uint64), np.ascontiguousarray(col_off, np.uint64)
        ts, te, qs = (np.ascontiguousarray(a, np.int32) for a in (trg_start, trg_end, qry_start))
        tc, qc = np.frombuffer(bytes(trg_cols), np.uint8), np.frombuffer(bytes(qry_cols), np.uint8)
        offs = [np.ascontiguousarray(a, np.uint64) for a in (total_off, sub_off, del_off, ins_off)]
        poss = [np.ascontiguousarray(a, np.int32) for a in (total_pos, sub_pos, del_pos, ins_pos)]
        if len(jeo) != n + 1 or len(tc) != len(qc) or not len(ts) == len(te) == len(qs) or int(jeo.max()) > len(ts) or \
                len(co) != len(ts) + 1 or int(co.max()) > len(tc) or any(len(o) != n + 1 or int(o.max()) > len(p) for o, p in zip(offs, poss)):
            raise ValueError("confirm_positions: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        b = ConfirmBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_confirm_positions(self.h, n, ptr(sd), jeo.ctypes.data, ptr(ts), ptr(te), ptr(qs), co.ctypes.data, ptr(tc),
                                                ptr(qc), *[x for o, p in zip(offs, poss) for x in (o.ctypes.data, ptr(p))], C.byref(b)))
        self.last_confirm_seconds = time.perf_counter() - t0
        take = lambda p, k, dtype: np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, dtype)
        out = {}
        for k in CONFIRM_LISTS + ("cons",):
            out[k + "_off"] = take(getattr(b, k + "_off"), (int(b.n_edges) if k == "cons" else n) + 1, np.uint64)
            out[k + "_pos"] = take(getattr(b, k + "_pos"), int(out[k + "_off"][-1]), np.int32)
        self.L.fg_release_confirm(C.byref(b))
        return ConfirmResult(**out)

    def classify_reads(self, buffer_count, job_edge_off, job_n_reads, edge_pos_off, edge_pos, edge_aln_off, read, trg_start, trg_end,
                       col_off, trg_cols, qry_cols, want_scores=False):
        """fg_classify_reads: _classify_reads with _index_mapping of the reference's flye/trestle/trestle.py for a batch of
        jobs.  Returns a ClassifyResult."""
        jnr = np.ascontiguousarray(job_n_reads, np.uint32)
        n = len(jnr)
        jeo, epo, eao, co = (np.ascontiguousarray(a, np.uint64) for a in (job_edge_off, edge_pos_off, edge_aln_off, col_off))
        ep, rd = np.ascontiguousarray(edge_pos, np.int32), np.ascontiguousarray(read, np.uint32)
        ts, te = np.ascontiguousarray(trg_start, np.int32), np.ascontiguousarray(trg_end, np.int32)
        tc, qc = np.frombuffer(bytes(trg_cols), np.uint8), np.frombuffer(bytes(qry_cols), np.uint8)
        if len(jeo) != n + 1 or len(tc) != len(qc) or not len(ts) == len(te) == len(rd) or len(epo) != len(eao) or \
                int(jeo.max()) + 1 > len(epo) or int(epo.max()) > len(ep) or int(eao.max()) > len(ts) or len(co) != len(ts) + 1 or \
                int(co.max()) > len(tc):
            raise ValueError("classify_reads: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        b = ClassifyBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_classify_reads(self.h, int(buffer_count), n, jeo.ctypes.data, ptr(jnr), epo.ctypes.data, ptr(ep),
                                             eao.ctypes.data, ptr(rd), ptr(ts), ptr(te), co.ctypes.data, ptr(tc), ptr(qc),
                                             int(bool(want_scores)), C.byref(b)))
        self.last_classify_seconds = time.perf_counter() - t0
        return self._classify_result(b, n, want_scores)

    def _classify_result(self, b, n, want_scores):
        take = lambda p, k, dtype: np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, dtype)
        out = dict(read_off=take(b.read_off, n + 1, np.uint64), aln_score=None, aln_counted=None)
        nr = int(out["read_off"][n])
        for k, t in (("status", np.uint8), ("top_edge", np.int32), ("top_score", np.int32), ("total_score", np.int32)):
            out[k] = take(getattr(b, k), nr, t)
        if want_scores:
            out["aln_score"] = take(b.aln_score, int(b.n_alignments), np.int32)
            out["aln_counted"] = take(b.aln_counted, int(b.n_alignments), np.uint8)
        self.L.fg_release_classify(C.byref(b))
        return ClassifyResult(**out)

    def expand_cigars(self, contig_off, contig_seq, aln_contig, ctg_pos, run_off, run_op, run_len, read_off, read_seq,
                      want_cols=True):
        """fg_expand_cigars: _parse_cigar (flye/utils/sam_parser.py:260-323) for a batch of SAM records.  Contig i is
        contig_seq[contig_off[i]:contig_off[i + 1]]; alignment a lies on contig aln_contig[a] at SAM POS ctg_pos[a], has the
        runs run_off[a] .. run_off[a + 1] of run_op (ASCII) / run_len and the SEQ bytes read_off[a] .. read_off[a + 1] of
        read_seq.  Returns an ExpandResult."""
        as_bytes = lambda x: np.ascontiguousarray(x, np.uint8) if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), np.uint8)
        cto = np.ascontiguousarray(contig_off, np.uint64)
        cs, rop, rs = as_bytes(contig_seq), as_bytes(run_op), as_bytes(read_seq)
        ac, cp = np.ascontiguousarray(aln_contig, np.uint32), np.ascontiguousarray(ctg_pos, np.int32)
        ro, rdo = np.ascontiguousarray(run_off, np.uint64), np.ascontiguousarray(read_off, np.uint64)
        rl = np.ascontiguousarray(run_len, np.uint32)
        n = len(ac)
        if len(cto) < 1 or len(cp) != n or len(ro) != n + 1 or len(rdo) != n + 1 or len(rop) != len(rl) or \
                int(cto.max()) > len(cs) or int(ro.max()) > len(rl) or int(rdo.max()) > len(rs):
            raise ValueError("expand_cigars: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if len(a) else None
        b = ExpandBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_expand_cigars(self.h, len(cto) - 1, cto.ctypes.data, ptr(cs), n, ptr(ac), ptr(cp), ro.ctypes.data,
                                            ptr(rop), ptr(rl), rdo.ctypes.data, ptr(rs), int(bool(want_cols)), C.byref(b)))
        self.last_expand_seconds = time.perf_counter() - t0

        def take(p, k, dtype):
            return np.ctypeslib.as_array(p, (k,)).copy() if k else np.zeros(0, dtype)

        co = np.ctypeslib.as_array(b.col_off, (n + 1,)).copy()
        out = dict(col_off=co, trg_cols=None, qry_cols=None)
        if want_cols:
            out["trg_cols"], out["qry_cols"] = take(b.trg_cols, int(co[n]), np.uint8), take(b.qry_cols, int(co[n]), np.uint8)
        for k in ("trg_start", "trg_end", "qry_start", "qry_end", "qry_len"):
            out[k] = take(getattr(b, k), n, np.int32)
        out["matches"], out["err_rate"] = take(b.matches, n, np.int64), take(b.err_rate, n, np.float64)
        self.L.fg_release_expand(C.byref(b))
        return ExpandResult(**out)

    @staticmethod
    def _record_arrays(name, contig_off, contig_seq, contig_aln_off, ctg_pos, run_off, run_op, run_len, read_off, read_seq):
        """the record arguments the two fused calls share, as contiguous arrays of the C types, checked against their
        offsets"""
        as_bytes = lambda x: np.ascontiguousarray(x, np.uint8) if isinstance(x, np.ndarray) else np.frombuffer(bytes(x), np.uint8)
        cto, cao = np.ascontiguousarray(contig_off, np.uint64), np.ascontiguousarray(contig_aln_off, np.uint64)
        cs, rop, rs = as_bytes(contig_seq), as_bytes(run_op), as_bytes(read_seq)
        cp = np.ascontiguousarray(ctg_pos, np.int32)
        ro, rdo = np.ascontiguousarray(run_off, np.uint64), np.ascontiguousarray(read_off, np.uint64)
        rl = np.ascontiguousarray(run_len, np.uint32)
        n, na = len(cto) - 1, len(cp)
        if n < 0 or len(cao) != n + 1 or int(cao.max()) > na or len(ro) != na + 1 or len(rdo) != na + 1 or len(rop) != len(rl) or \
                int(cto.max()) > len(cs) or int(ro.max()) > len(rl) or int(rdo.max()) > len(rs):
            raise ValueError(name + ": offsets outside their arrays")
        return n, na, (cto, cs, cao, cp, ro, rop, rl, rdo, rs)

    def contig_consensus_cigars(self, contig_off, contig_seq, contig_aln_off, ctg_pos, run_off, run_op, run_len, read_off,
                                read_seq, qry_id, use=None, want_profile=False):
        """fg_contig_consensus_cigars: expand_cigars and contig_consensus as one call, the columns never leaving the
        device.  The contigs and records are given as for expand_cigars, but grouped by contig (contig i has the
        alignments contig_aln_off[i] .. contig_aln_off[i + 1]); qry_id and use as for contig_consensus.  Returns a
        ConsensusResult equal to the two calls'."""
        n, na, arrs = self._record_arrays("contig_consensus_cigars", contig_off, contig_seq, contig_aln_off, ctg_pos, run_off,
                                          run_op, run_len, read_off, read_seq)
        qi = np.ascontiguousarray(qry_id, np.int32)
        us = np.ascontiguousarray(use, np.uint8) if use is not None else None
        if len(qi) != na or (us is not None and len(us) != na):
            raise ValueError("contig_consensus_cigars: offsets outside their arrays")
        # an offset array is never empty; the others go as NULL when they are
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        b = ConsensusBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_contig_consensus_cigars(self.h, n, *[ptr(a) for a in arrs], ptr(qi), ptr(us), int(bool(want_profile)),
                                                      C.byref(b)))
        self.last_consensus_seconds = time.perf_counter() - t0
        return self._consensus_result(b, n, want_profile)

    def make_bubbles_cigars(self, params, contig_off, contig_seq, contig_circular, contig_aln_off, ctg_pos, run_off, run_op,
                            run_len, read_off, read_seq, err_rate, want_profile=False):
        """fg_make_bubbles_cigars: expand_cigars and make_bubbles as one call, the columns never leaving the device.  The
        contigs and records as for contig_consensus_cigars; err_rate per alignment comes from an earlier
        expand_cigars(want_cols=False).  Returns a BubbleResult equal to the two calls'."""
        n, na, arrs = self._record_arrays("make_bubbles_cigars", contig_off, contig_seq, contig_aln_off, ctg_pos, run_off, run_op,
                                          run_len, read_off, read_seq)
        cc = np.ascontiguousarray(contig_circular, np.uint8) if contig_circular is not None else np.zeros(n, np.uint8)
        er = np.ascontiguousarray(err_rate, np.float64)
        if len(cc) != n or len(er) != na:
            raise ValueError("make_bubbles_cigars: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if len(a) else None
        cto, cs, cao = arrs[:3]
        b = BubbleBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_make_bubbles_cigars(self.h, C.byref(params), n, ptr(cto), ptr(cs), ptr(cc), ptr(cao),
                                                  *[ptr(a) for a in arrs[3:]], ptr(er), int(bool(want_profile)), C.byref(b)))
        self.last_bubbles_seconds = time.perf_counter() - t0
        return self._bubble_result(b, n, want_profile)

    def divergence_profile_cigars(self, sub_thresh, del_thresh, ins_thresh, contig_off, contig_seq, contig_aln_off, ctg_pos, run_off,
                                  run_op, run_len, read_off, read_seq, want_profile=False):
        """fg_divergence_profile_cigars: expand_cigars and divergence_profile as one call, the columns never leaving the
        device.  The contigs and records as for contig_consensus_cigars.  Returns a DivergenceResult equal to the two
        calls'."""
        n, na, arrs = self._record_arrays("divergence_profile_cigars", contig_off, contig_seq, contig_aln_off, ctg_pos, run_off,
                                          run_op, run_len, read_off, read_seq)
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        b = DivergenceBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_divergence_profile_cigars(self.h, float(sub_thresh), float(del_thresh), float(ins_thresh), n,
                                                        *[ptr(a) for a in arrs], int(bool(want_profile)), C.byref(b)))
        self.last_divergence_seconds = time.perf_counter() - t0
        return self._divergence_result(b, n, want_profile)

    def classify_reads_cigars(self, buffer_count, job_edge_off, job_n_reads, edge_pos_off, edge_pos, edge_off, edge_seq, edge_aln_off,
                              read, ctg_pos, run_off, run_op, run_len, read_off, read_seq, want_scores=False):
        """fg_classify_reads_cigars: expand_cigars and classify_reads as one call, the columns never leaving the device.
        Jobs, edges, lists and read numbers as for classify_reads; edge e's consensus is edge_seq[edge_off[e]:edge_off[e + 1]]
        and its alignments (edge_aln_off[e] .. edge_aln_off[e + 1]) are records on it, given as for expand_cigars.  Returns
        a ClassifyResult equal to the two calls'."""
        jnr = np.ascontiguousarray(job_n_reads, np.uint32)
        n = len(jnr)
        jeo, epo = np.ascontiguousarray(job_edge_off, np.uint64), np.ascontiguousarray(edge_pos_off, np.uint64)
        ep, rd = np.ascontiguousarray(edge_pos, np.int32), np.ascontiguousarray(read, np.uint32)
        _, na, (eo, es, eao, cp, ro, rop, rl, rdo, rs) = self._record_arrays(
            "classify_reads_cigars", edge_off, edge_seq, edge_aln_off, ctg_pos, run_off, run_op, run_len, read_off, read_seq)
        if len(jeo) != n + 1 or len(rd) != na or len(epo) != len(eao) or int(jeo.max()) + 1 > len(epo) or int(epo.max()) > len(ep):
            raise ValueError("classify_reads_cigars: offsets outside their arrays")
        ptr = lambda a: a.ctypes.data if a is not None and len(a) else None
        b = ClassifyBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_classify_reads_cigars(self.h, int(buffer_count), n, jeo.ctypes.data, ptr(jnr), epo.ctypes.data, ptr(ep),
                                                    eo.ctypes.data, ptr(es), eao.ctypes.data, ptr(rd), ptr(cp), ro.ctypes.data, ptr(rop),
                                                    ptr(rl), rdo.ctypes.data, ptr(rs), int(bool(want_scores)), C.byref(b)))
        self.last_classify_seconds = time.perf_counter() - t0
        return self._classify_result(b, n, want_scores)

    def edge_coverage(self, window, recs, aln, aln_off, first_ext_id, edge_of, edge_len, want_vectors=True):
        """fg_edge_coverage: the window coverage of MultiplicityInferer::estimateCoverage (multiplicity_inferer.cpp:
        14-41) for the paths recs[aln[aln_off[p]:aln_off[p + 1]]] (the layout chain_alignments returns).  edge_of[i]: the
        edge of indexed sequence first_ext_id + i; edge_len[e]: GraphEdge::length().  Returns (win_off, cov or None, sum,
        max, median) with one value per edge."""
        r = np.ascontiguousarray(recs, REC_DTYPE)
        a = np.ascontiguousarray(aln, np.uint64)
        off = np.ascontiguousarray(aln_off, np.uint64)
        eo = np.ascontiguousarray(edge_of, np.uint32)
        el = np.ascontiguousarray(edge_len, np.int32)
        if len(off) < 1 or (len(off) > 1 and int(off.max()) > len(a)):
            raise ValueError("edge_coverage: offsets inside the alignment indices")
        ne = len(el)
        b = EdgeCoverageBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_edge_coverage(self.h, int(window), r.ctypes.data if len(r) else None, len(r),
                                            a.ctypes.data if len(a) else None, off.ctypes.data, len(off) - 1, int(first_ext_id),
                                            len(eo), eo.ctypes.data if len(eo) else None, ne, el.ctypes.data if ne else None,
                                            int(bool(want_vectors)), C.byref(b)))
        self.last_coverage_seconds = time.perf_counter() - t0
        win_off = np.ctypeslib.as_array(b.win_off, (ne + 1,)).copy()
        nw = int(win_off[ne])

        def take(ptr, n, dtype):
            return np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dtype)

        out = (win_off, take(b.cov, nw, np.int32) if want_vectors else None, take(b.sum, ne, np.int64), take(b.max, ne, np.int32),
               take(b.median, ne, np.int32))
        self.L.fg_release_edge_coverage(C.byref(b))
        return out

    def align_reads(self, detector_params, query_ids, chain_params, node_left, node_right, max_divergence, realign=False,
                    use_hpc=False):
        """The body of ReadAligner::alignReads' alignRead lambda (read_aligner.cpp:212-262) for a batch of reads of the
        fg_set_queries container against the indexed edge sequences, as three device calls and one host fold:
        fg_overlaps with the flags alignReads gives its detector (:186-192: no overhang test, every primary, no
        kmerMatches, no divergence gate, no base-level alignment; max_jump, min_overlap and use_hpc are taken from
        detector_params), fg_chain_alignments, with realign (reads_base_alignment) one fg_edit_ranges call over all
        alignments of all chains, fg_chain_divergence, and the gate chainDivergence < max_divergence (:245).
        node_left / node_right: the nodes of the edge behind indexed sequence id first_id + i, both strands.
        Returns a ReadAlignments."""
        p = DetectorParams(max_jump=detector_params.max_jump, min_overlap=detector_params.min_overlap, max_overhang=0,
                           keep_alignment=0, only_max_ext=0, nucl_alignment=0, partition_bad_mappings=0,
                           use_hpc=detector_params.use_hpc, max_divergence=1.0)
        q = np.ascontiguousarray(query_ids, dtype=np.uint32)
        b = OverlapBatch()
        self._check(self.L.fg_overlaps(self.h, C.byref(p), q.ctypes.data, len(q), 0, 0, C.byref(b)))
        res = OverlapResult(self.L, q, b)
        recs = np.asarray(res.recs)
        nl = np.ascontiguousarray(node_left, np.uint32)
        nr = np.ascontiguousarray(node_right, np.uint32)
        chain_off, aln_off, aln, _ = self.chain_alignments(recs, res.query_off, chain_params, self.first_id, nl, nr)
        alns = recs[aln.astype(np.int64)]
        div = self.edit_ranges(alns, use_hpc)[3] if realign else alns["seq_divergence"]
        chain_div = chain_divergence(alns["cur_end"] - alns["cur_begin"], div, aln_off)
        good = chain_div < np.float32(max_divergence)
        out_chains, out_off = [], [0]
        for i in range(len(q)):
            mine = [alns[int(aln_off[c]):int(aln_off[c + 1])] for c in range(int(chain_off[i]), int(chain_off[i + 1])) if good[c]]
            out_chains += mine + [complement(ch)[::-1] for ch in mine]
            out_off.append(len(out_chains))
        return ReadAlignments(q, out_off, out_chains, self.first_id, nl, nr, chain_off, chain_div)

    def paf_groups(self, hits):
        """fg_paf_groups on hits (PAF_HIT_DTYPE, file order) -> dict of order, group_off, group_query, group_target,
        query_cover, target_cover"""
        h = np.ascontiguousarray(hits, PAF_HIT_DTYPE)
        b = PafGroupBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_paf_groups(self.h, h.ctypes.data if len(h) else None, len(h), C.byref(b)))
        self.last_paf_seconds = time.perf_counter() - t0
        ng = int(b.n_groups)
        take = lambda ptr, n, dtype: np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dtype)
        out = dict(order=take(b.order, len(h), np.uint32), group_off=take(b.group_off, ng + 1, np.uint64),
                   group_query=take(b.group_query, ng, np.uint32), group_target=take(b.group_target, ng, np.uint32),
                   query_cover=take(b.query_cover, ng, np.int64), target_cover=take(b.target_cover, ng, np.int64))
        self.L.fg_release_paf_groups(C.byref(b))
        return out

    def paf_circular(self, hits, max_overhang_read=150, max_overhang_pair=300):
        """fg_paf_circular on hits (PAF_HIT_DTYPE, file order) -> dict of circ_query, circ_hit, group_query,
        group_target, pair_first, pair_second, pair_ok"""
        h = np.ascontiguousarray(hits, PAF_HIT_DTYPE)
        b = PafCircularBatch()
        t0 = time.perf_counter()
        self._check(self.L.fg_paf_circular(self.h, h.ctypes.data if len(h) else None, len(h), int(max_overhang_read),
                                           int(max_overhang_pair), C.byref(b)))
        self.last_paf_seconds = time.perf_counter() - t0
        nc, ng = int(b.n_circular), int(b.n_groups)
        take = lambda ptr, n, dtype: np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dtype)
        out = dict(circ_query=take(b.circ_query, nc, np.uint32), circ_hit=take(b.circ_hit, nc, np.uint32),
                   group_query=take(b.group_query, ng, np.uint32), group_target=take(b.group_target, ng, np.uint32),
                   pair_first=take(b.pair_first, ng, np.int32), pair_second=take(b.pair_second, ng, np.int32),
                   pair_ok=take(b.pair_ok, ng, np.uint8))
        self.L.fg_release_paf_circular(C.byref(b))
        return out

    def components(self, n_vertices, edge_u, edge_v):
        """fg_components: labels[v] = the smallest vertex of v's connected component"""
        u = np.ascontiguousarray(edge_u, np.uint32)
        v = np.ascontiguousarray(edge_v, np.uint32)
        if len(u) != len(v):
            raise ValueError("components: edge_u and edge_v differ in length")
        labels = np.zeros(int(n_vertices), np.uint32)
        self._check(self.L.fg_components(self.h, int(n_vertices), len(u), u.ctypes.data if len(u) else None,
                                         v.ctypes.data if len(v) else None, labels.ctypes.data if len(labels) else None))
        return labels

    def sam_parse(self, data, offset=0, n_bytes=None) -> SamTextResult:
        """fg_sam_parse on the SAM text data[offset : offset + n_bytes] (bytes, bytearray, memoryview or uint8 array;
        by default all of it): lines, records, chunks, tokens, FLAG / POS, CIGAR runs and spans, cut on the device.
        Offsets in the result are relative to the start of that window."""
        buf = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
        n = len(buf) - int(offset) if n_bytes is None else int(n_bytes)
        if offset < 0 or n < 0 or offset + n > len(buf):
            raise ValueError("sam_parse: the window leaves the buffer")
        b = SamText()
        t0 = time.perf_counter()
        self._check(self.L.fg_sam_parse(self.h, buf.ctypes.data + int(offset) if n else None, n, C.byref(b)))
        self.last_sam_seconds = time.perf_counter() - t0
        self.sam_parse_calls = getattr(self, "sam_parse_calls", 0) + 1
        nr, nu = int(b.n_records), int(b.n_runs)
        size = dict(chunk_off=int(b.n_chunks) + 1, run_off=nr + 1, run_op=nu, run_len=nu)
        dtype = {name: np.dtype(t._type_) for name, t in SamText._fields_ if name in SamTextResult.ARRAYS}
        take = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, (n,)).copy() if n else np.zeros(0, dt)
        res = SamTextResult(buf[int(offset):int(offset) + n], n_lines=int(b.n_lines), n_records=nr, n_chunks=int(b.n_chunks), n_runs=nu,
                            **{k: take(getattr(b, k), size.get(k, nr), dtype[k]) for k in SamTextResult.ARRAYS})
        self.L.fg_release_sam_text(C.byref(b))
        return res

    def kernel_times(self):
        arr = (KernelTime * 64)()
        n = self.L.fg_kernel_times(self.h, arr, 64)
        return {arr[i].name.decode(): (arr[i].seconds, arr[i].launches) for i in range(min(n, 64))}


class ReadAlignments:
    """What the alignRead lambda appends to _readAlignments for a batch of reads (read_aligner.cpp:251-278).  Per query i
    the chains chain_off[i] .. chain_off[i + 1]: the good chains, then their complements (every record complemented, the
    chain reversed).  Chain c = recs[aln_off[c]:aln_off[c + 1]] (REC_DTYPE) with the nodes of each alignment's edge in
    node_left / node_right, read from the caller's tables at the record's ext_id -- the complement edge's entry for a
    complemented record.  divergence: chainDivergence of EVERY chain chainReadAlignments returned, good or not, in the
    order divergenceStats.add sees them (:244); query i's are divergence[all_chain_off[i]:all_chain_off[i + 1]]."""

    def __init__(self, query_ids, chain_off, chains, first_ext_id, node_left, node_right, all_chain_off, divergence):
        self.query_ids = query_ids
        self.chain_off = np.asarray(chain_off, np.uint64)
        self.aln_off = np.zeros(len(chains) + 1, np.uint64)
        self.aln_off[1:] = np.cumsum([len(ch) for ch in chains])
        self.recs = np.concatenate(chains) if chains else np.zeros(0, REC_DTYPE)
        at = self.recs["ext_id"].astype(np.int64) - int(first_ext_id)
        self.node_left, self.node_right = node_left[at], node_right[at]
        self.all_chain_off = all_chain_off
        self.divergence = divergence

    def chains_of(self, i):
        return [self.recs[int(self.aln_off[c]):int(self.aln_off[c + 1])]
                for c in range(int(self.chain_off[i]), int(self.chain_off[i + 1]))]


class VertexIndex:
    """Mirror of reference VertexIndex (src/sequence/vertex_index.h:66-300)."""

    def __init__(self, ctx: Context, sample_rate: float):
        self.ctx = ctx
        self._sample_rate_init = float(sample_rate)
        self._counted = False
        self.stats = None

    def countKmers(self):
        """vertex_index.cpp:19-22.  Counting runs fused with the build on the device;
        this only records that the caller asked for it (k > 17 raises like :504-507)."""
        if self.ctx.k > 17:
            raise FlyeGpuError(-6, "Can't use flat counter for k-mer size > 17")
        self._counted = True

    def buildIndexUnevenCoverage(self, globalMinFreq: int, selectRate: float, tandemFreq: int,
                                 repeat_kmer_rate: float = 100.0):
        if not self._counted:
            raise FlyeGpuError(-4, "countKmers() must be called first")
        st = IndexStats()
        L = self.ctx.L
        self.ctx._check(L.fg_build_index_solid(self.ctx.h, globalMinFreq, selectRate, tandemFreq,
                                               repeat_kmer_rate, self._sample_rate_init, C.byref(st)))
        self.stats = st.as_dict()
        return self.stats

    def buildIndexMinimizers(self, minCoverage: int, wndLen: int, repeat_kmer_rate: float = 100.0):
        st = IndexStats()
        L = self.ctx.L
        self.ctx._check(L.fg_build_index_minimizers(self.ctx.h, minCoverage, wndLen, repeat_kmer_rate,
                                                    C.byref(st)))
        self.stats = st.as_dict()
        return self.stats

    def build(self, cfg: dict):
        """Index build exactly as main_assemble.cpp:195-223 selects it."""
        if cfg["use_minimizers"]:
            return self.buildIndexMinimizers(1, int(cfg["minimizer_window"]), cfg["repeat_kmer_rate"])
        self.countKmers()
        return self.buildIndexUnevenCoverage(2, cfg["meta_read_top_kmer_rate"],
                                             int(cfg["meta_read_filter_kmer_freq"]),
                                             cfg["repeat_kmer_rate"])

    # ---- the build in steps (sharded over GPUs: flye_amd/dist.py) -------------------------------------
    INDEX_BINS = 4096

    def begin(self, cfg: dict) -> np.ndarray:
        """Selection step of the build main_assemble.cpp:195-223 selects; returns the number of accepted
        k-mer positions per key bin."""
        hist = np.zeros(self.INDEX_BINS, np.uint64)
        L, h = self.ctx.L, self.ctx.h
        if cfg["use_minimizers"]:
            self.ctx._check(L.fg_index_begin_minimizers(h, 1, int(cfg["minimizer_window"]), cfg["repeat_kmer_rate"],
                                                        hist.ctypes.data))
        else:
            self.countKmers()
            self.ctx._check(L.fg_index_begin_solid(h, 2, cfg["meta_read_top_kmer_rate"],
                                                   int(cfg["meta_read_filter_kmer_freq"]), cfg["repeat_kmer_rate"],
                                                   self._sample_rate_init, hist.ctypes.data))
        return hist

    # solid-mode selection in steps of its own (counters of a key range only; batches of reads)
    def kmer_hist(self) -> np.ndarray:
        """ALL k-mer positions per key bin (what the ranks' key ranges are balanced on)."""
        hist = np.zeros(self.INDEX_BINS, np.uint64)
        self.ctx._check(self.ctx.L.fg_index_kmer_hist(self.ctx.h, hist.ctypes.data))
        return hist

    def count_slice(self, cfg: dict, bin_lo: int, bin_hi: int):
        """-> (distinct canonical k-mers of the range, number of read batches)"""
        self.countKmers()
        d, nb = C.c_uint64(), C.c_uint32()
        self.ctx._check(self.ctx.L.fg_index_count_slice(self.ctx.h, 2, cfg["meta_read_top_kmer_rate"],
                                                        int(cfg["meta_read_filter_kmer_freq"]), cfg["repeat_kmer_rate"],
                                                        self._sample_rate_init, int(bin_lo), int(bin_hi), C.byref(d), C.byref(nb)))
        return d.value, nb.value

    def batch_freq(self, batch: int):
        """-> (device pointer of the batch's uint32 frequencies, their number)"""
        p, n = C.c_void_p(), C.c_uint64()
        self.ctx._check(self.ctx.L.fg_index_batch_freq(self.ctx.h, int(batch), C.byref(p), C.byref(n)))
        return p.value or 0, n.value

    def batch_select(self, batch: int):
        self.ctx._check(self.ctx.L.fg_index_batch_select(self.ctx.h, int(batch)))

    def selection_done(self) -> np.ndarray:
        hist = np.zeros(self.INDEX_BINS, np.uint64)
        self.ctx._check(self.ctx.L.fg_index_selection_done(self.ctx.h, hist.ctypes.data))
        return hist

    def gather_begin(self, n_keys: int, n_entries: int, n_rep: int):
        """-> (full array device pointers [keys, key_off, entries, repetitive], the own piece's, piece sizes
        (keys, entries, repetitive))"""
        full = (C.c_void_p * 4)()
        piece = (C.c_void_p * 4)()
        sizes = (C.c_uint64 * 3)()
        self.ctx._check(self.ctx.L.fg_index_gather_begin(self.ctx.h, int(n_keys), int(n_entries), int(n_rep), full, piece, sizes))
        return [x or 0 for x in full], [x or 0 for x in piece], [int(x) for x in sizes]

    def gather_end(self, sample_rate: float):
        self.ctx._check(self.ctx.L.fg_index_gather_end(self.ctx.h, float(sample_rate)))

    def build_range(self, bin_lo: int, bin_hi: int) -> np.ndarray:
        sums = np.zeros(2, np.uint64)
        self.ctx._check(self.ctx.L.fg_index_build_range(self.ctx.h, int(bin_lo), int(bin_hi), sums.ctypes.data))
        return sums

    def finish(self, total_sums=None):
        st = IndexStats()
        ts = None if total_sums is None else np.ascontiguousarray(total_sums, np.uint64)
        self.ctx._check(self.ctx.L.fg_index_finish(self.ctx.h, None if ts is None else ts.ctypes.data, C.byref(st)))
        self.stats = st.as_dict()
        return self.stats

    def import_index(self, ex: "IndexExport", sample_rate: float, on_device=False, ptrs=None):
        """fg_import_index from host arrays (``ex``) or device pointers (``ptrs`` = keys, key_off, entries,
        repetitive as integers, with the counts in ``ex`` = (n_keys, n_entries, n_rep))."""
        L, h = self.ctx.L, self.ctx.h
        if on_device:
            nk, ne, nr = ex
            self.ctx._check(L.fg_import_index(h, nk, ptrs[0], ptrs[1], ne, ptrs[2], nr, ptrs[3], float(sample_rate), 1))
        else:
            k = np.ascontiguousarray(ex.keys, np.uint64)
            o = np.ascontiguousarray(ex.key_off, np.uint64)
            e = np.ascontiguousarray(ex.entries, np.uint64)
            r = np.ascontiguousarray(ex.repetitive, np.uint64)
            self.ctx._check(L.fg_import_index(h, len(k), k.ctypes.data, o.ctypes.data, len(e), e.ctypes.data, len(r),
                                              r.ctypes.data, float(sample_rate), 0))
            nk, ne, nr = len(k), len(e), len(r)
        self.stats = dict(self.stats or {}, selected_kmers=nk, index_entries=ne, repetitive_kmers=nr,
                          sample_rate=float(np.float32(sample_rate)))

    def device_arrays(self):
        """(n_keys, n_entries, n_rep), (keys, key_off, entries, repetitive) device pointers of the built index."""
        n = [C.c_uint64() for _ in range(3)]
        p = [C.c_void_p() for _ in range(4)]
        self.ctx._check(self.ctx.L.fg_index_device_arrays(self.ctx.h, *[C.byref(x) for x in n], *[C.byref(x) for x in p]))
        return tuple(x.value for x in n), tuple(x.value or 0 for x in p)

    def clear(self):
        self.ctx._check(self.ctx.L.fg_clear_index(self.ctx.h))

    def keep_targets(self, world: int, rank: int) -> int:
        """Option B (fg_index_keep_targets): keep only the entries of the target reads i with i % world == rank.
        Keys, repetitive k-mers, statistics and getSampleRate() stay those of the whole index.  Returns the entries
        kept."""
        n = C.c_uint64()
        self.ctx._check(self.ctx.L.fg_index_keep_targets(self.ctx.h, int(world), int(rank), C.byref(n)))
        return n.value

    def shard(self):
        """(world, rank) of the restriction; (1, 0) for the whole index"""
        w, r = C.c_uint32(), C.c_uint32()
        self.ctx._check(self.ctx.L.fg_index_shard(self.ctx.h, C.byref(w), C.byref(r)))
        return w.value, r.value

    # ---- option B built directly from the key-range pieces (flye_amd/dist.py::scatter_pieces_inplace) ------
    SPLIT_MAX_WORLD = 128

    def split_piece(self, world: int):
        """fg_index_piece_split: the piece's entries partitioned by target owner.  -> (device pointer of the
        world x n_keys count matrix, device pointer of the split entries, entries per destination [world])"""
        cnt, ent = C.c_void_p(), C.c_void_p()
        totals = np.zeros(max(int(world), 1), np.uint64)
        self.ctx._check(self.ctx.L.fg_index_piece_split(self.ctx.h, int(world), C.byref(cnt), C.byref(ent),
                                                        totals.ctypes.data))
        return cnt.value or 0, ent.value or 0, totals

    def scatter_begin(self, world: int, rank: int, n_keys: int, n_shard_entries: int, n_rep: int):
        """fg_index_scatter_begin -> the shard's device pointers [keys, key_off (receives the counts), entries,
        repetitive]"""
        full = (C.c_void_p * 4)()
        self.ctx._check(self.ctx.L.fg_index_scatter_begin(self.ctx.h, int(world), int(rank), int(n_keys),
                                                          int(n_shard_entries), int(n_rep), full))
        return [x or 0 for x in full]

    def scatter_end(self, sample_rate: float):
        self.ctx._check(self.ctx.L.fg_index_scatter_end(self.ctx.h, float(sample_rate)))

    def getSampleRate(self) -> float:
        return self.stats["sample_rate"] if self.stats else self._sample_rate_init

    def export(self) -> IndexExport:
        L, h = self.ctx.L, self.ctx.h
        nk, ne, nr = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ctx._check(L.fg_export_index(h, C.byref(nk), C.byref(ne), C.byref(nr), None, None, None, None))
        keys = np.empty(nk.value, np.uint64)
        off = np.empty(nk.value + 1, np.uint64)
        ent = np.empty(ne.value, np.uint64)
        rep = np.empty(nr.value, np.uint64)
        self.ctx._check(L.fg_export_index(h, C.byref(nk), C.byref(ne), C.byref(nr), keys.ctypes.data,
                                          off.ctypes.data, ent.ctypes.data, rep.ctypes.data))
        return IndexExport(keys, off, ent, rep)


class OverlapDetector:
    """Ctor arguments of reference OverlapDetector (overlap.h:313-336)."""

    def __init__(self, ctx: Context, vertexIndex: VertexIndex, maxJump: int, minOverlap: int,
                 maxOverhang: int, keepAlignment: bool, onlyMaxExt: bool, maxDivergence: float,
                 nuclAlignment: bool, partitionBadMappings: bool, useHpc: bool):
        self.ctx, self.index = ctx, vertexIndex
        self.p = DetectorParams(max_jump=maxJump, min_overlap=minOverlap, max_overhang=maxOverhang,
                                keep_alignment=int(keepAlignment), only_max_ext=int(onlyMaxExt),
                                nucl_alignment=int(nuclAlignment),
                                partition_bad_mappings=int(partitionBadMappings), use_hpc=int(useHpc),
                                max_divergence=float(maxDivergence))

    @classmethod
    def for_assemble(cls, ctx, index, cfg, min_overlap=1000):
        """The detector main_assemble.cpp:229-238 builds."""
        return cls(ctx, index, int(cfg["maximum_jump"]), min_overlap, int(cfg["maximum_overhang"]),
                   False, True, 1.0, bool(cfg["reads_base_alignment"]), False,
                   bool(cfg["hpc_scoring_on"]))

    def getSeqOverlapsBatch(self, query_ids, forceLocal=False, maxOverlaps=0) -> OverlapResult:
        q = np.ascontiguousarray(query_ids, dtype=np.uint32)
        b = OverlapBatch()
        L = self.ctx.L
        self.ctx._check(L.fg_overlaps(self.ctx.h, C.byref(self.p), q.ctypes.data, len(q), maxOverlaps,
                                      int(bool(forceLocal)), C.byref(b)))
        return OverlapResult(L, q, b)

    # ---- option B: index sharded by target read (flye_amd/dist.py) ----------------------------------------------
    def probe_hits(self, query_ids):
        """Seed collection only, against this context's (shard) index: (hits per query as uint64, device pointer
        of the fg_seed_hit array -- query after query, each in emission order; valid until the next call on the
        context --, number of hits)."""
        q = np.ascontiguousarray(query_ids, dtype=np.uint32)
        counts = np.zeros(len(q), np.uint64)
        ptr, n = C.c_void_p(), C.c_uint64()
        self.ctx._check(self.ctx.L.fg_probe_hits(self.ctx.h, q.ctypes.data, len(q), counts.ctypes.data, C.byref(ptr),
                                                 C.byref(n)))
        return counts, ptr.value or 0, n.value

    def getSeqOverlapsFromHits(self, query_ids, counts, hits, forceLocal=False, maxOverlaps=0) -> OverlapResult:
        """getSeqOverlaps of ``query_ids`` from the hits of n_src shards: ``counts[s, q]`` hits of query q from
        source s; ``hits`` holds the sources one after another, inside a source the queries in list order (any order
        inside a run) -- a device pointer (int), a torch tensor or a SEED_HIT_DTYPE numpy array (copied to the
        context's device)."""
        q = np.ascontiguousarray(query_ids, dtype=np.uint32)
        cnt = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1, len(q)) if len(q) else \
            np.zeros((max(1, len(counts)), 0), np.uint64)
        keep = None
        if isinstance(hits, (int, np.integer)):
            ptr = int(hits)
        else:
            import torch
            dev = torch.device("cuda", self.ctx_device())
            if isinstance(hits, np.ndarray):
                hits = torch.from_numpy(np.ascontiguousarray(hits, SEED_HIT_DTYPE).view(np.int32).copy())
            t = hits.reshape(-1)
            if t.numel() != 3 * int(cnt.sum()):
                raise FlyeGpuError(-3, f"{t.numel() // 3} hits given, counts add up to {int(cnt.sum())}")
            keep = t.to(dev, dtype=torch.int32).contiguous() if t.numel() else torch.zeros(3, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)          # the library reads it on its own stream
            ptr = keep.data_ptr()
        b = OverlapBatch()
        L = self.ctx.L
        self.ctx._check(L.fg_overlaps_from_hits(self.ctx.h, C.byref(self.p), q.ctypes.data, len(q), maxOverlaps,
                                                int(bool(forceLocal)), cnt.shape[0], cnt.ctypes.data, ptr or None,
                                                C.byref(b)))
        del keep
        return OverlapResult(L, q, b)

    def ctx_device(self) -> int:
        return getattr(self.ctx, "device", 0)


class Group:
    """One fg_group: several contexts of this process, possibly on different devices, behind one handle -- the
    target-sharded index (option B) built directly and the overlap stage over it, without a process group.
    ``devices`` may name a device more than once."""

    def __init__(self, devices, kmer_size=17):
        self.L = load_library()
        self.devices = [int(d) for d in devices]
        self.k = kmer_size
        self.h = None
        h = C.c_void_p()
        arr = (C.c_int * max(1, len(self.devices)))(*self.devices)
        rc = self.L.fg_group_create(C.byref(h), arr, len(self.devices), kmer_size)
        if rc != 0:
            raise FlyeGpuError(rc, self.L.fg_strerror(rc).decode())
        self.h = h
        self.first_id = 0
        self.n_reads = 0
        self.stats_index = None

    def _check(self, rc):
        if rc != 0:
            raise FlyeGpuError(rc, f"{self.L.fg_strerror(rc).decode()}: {self.L.fg_group_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.L.fg_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        n = C.c_uint32()
        self._check(self.L.fg_group_size(self.h, C.byref(n)))
        return n.value

    def set_reads(self, rs, first_seq_id=0):
        self.rs = rs
        self.first_id = first_seq_id
        self.n_reads = rs.n
        self._check(self.L.fg_group_set_reads(self.h, rs.n, rs.words.ctypes.data, rs.word_off.ctypes.data,
                                              rs.length.ctypes.data, first_seq_id))

    def set_queries(self, rs, first_seq_id):
        self.qrs = rs
        self._check(self.L.fg_group_set_queries(self.h, rs.n, rs.words.ctypes.data, rs.word_off.ctypes.data,
                                                rs.length.ctypes.data, first_seq_id))

    def build(self, cfg: dict, sample_rate=None):
        """The build main_assemble.cpp:195-223 selects (as ``VertexIndex.build``), every member ending with its
        target shard; returns the statistics of the whole index."""
        st = IndexStats()
        if cfg["use_minimizers"]:
            rc = self.L.fg_group_build_index_minimizers(self.h, 1, int(cfg["minimizer_window"]), cfg["repeat_kmer_rate"],
                                                        C.byref(st))
        else:
            if self.k > 17:
                raise FlyeGpuError(-6, "Can't use flat counter for k-mer size > 17")
            rate = float(int(cfg["assemble_kmer_sample"])) if sample_rate is None else float(sample_rate)
            rc = self.L.fg_group_build_index_solid(self.h, 2, cfg["meta_read_top_kmer_rate"],
                                                   int(cfg["meta_read_filter_kmer_freq"]), cfg["repeat_kmer_rate"],
                                                   rate, C.byref(st))
        self._check(rc)
        self.stats_index = st.as_dict()
        return self.stats_index

    def build_info(self) -> dict:
        bi = GroupBuildInfo()
        self._check(self.L.fg_group_build_info(self.h, C.byref(bi)))
        return {k: int(getattr(bi, k)) for k, _ in bi._fields_}

    def clear(self):
        self._check(self.L.fg_group_clear_index(self.h))

    def getSampleRate(self) -> float:
        return self.stats_index["sample_rate"]

    def overlaps(self, params, query_ids, forceLocal=False, maxOverlaps=0) -> OverlapResult:
        """fg_group_overlaps: what ``OverlapDetector.getSeqOverlapsBatch`` gives on one context with the full index.
        ``params``: a ``DetectorParams`` or a detector (its ``.p``)."""
        p = getattr(params, "p", params)
        q = np.ascontiguousarray(query_ids, dtype=np.uint32)
        b = OverlapBatch()
        self._check(self.L.fg_group_overlaps(self.h, C.byref(p), q.ctypes.data, len(q), maxOverlaps,
                                             int(bool(forceLocal)), C.byref(b)))
        return OverlapResult(self.L, q, b)

    def stats(self) -> dict:
        """of the last ``overlaps``"""
        st = GroupStats()
        self._check(self.L.fg_group_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def member(self, i: int) -> Context:
        """Member i as a borrowed ``Context`` (kernel_times, ``VertexIndex(ctx, rate).export()`` / ``.shard()``, the
        step calls of option B); the group keeps owning it."""
        ptr = self.L.fg_group_member(self.h, int(i))
        if not ptr:
            raise FlyeGpuError(-3, f"no member {i}")
        c = Context.__new__(Context)
        c.L, c.h, c.k, c.device, c._borrowed = self.L, C.c_void_p(ptr), self.k, self.devices[int(i)], True
        c.first_id, c.n_reads = self.first_id, self.n_reads
        if hasattr(self, "rs"):
            c.rs = self.rs
        c._group = self                                # the handle outlives the view
        return c


def seed_hits_to_host(ptr: int, n: int, device: int = 0) -> np.ndarray:
    """Copy of n fg_seed_hit records at device pointer ``ptr`` (what probe_hits returns) as a SEED_HIT_DTYPE array."""
    if not n:
        return np.empty(0, SEED_HIT_DTYPE)
    import torch
    arr = {"shape": (3 * n,), "typestr": "<i4", "data": (int(ptr), False), "version": 2}
    holder = type("_DevHits", (), {"__cuda_array_interface__": arr})()
    t = torch.as_tensor(holder, device=torch.device("cuda", device))
    return t.cpu().numpy().view(SEED_HIT_DTYPE).copy()


def seq_name(read_names, first_id, rec_id) -> str:
    """SequenceContainer::seqName: '+' / '-' + the FASTA header (sequence_container.cpp:62, :75)."""
    i = int(rec_id) - int(first_id)
    return ("-" if i & 1 else "+") + read_names[i >> 1]


def dump_overlaps(recs: np.ndarray, cur_name, ext_name, edge_ids=None):
    """OverlapRange::dump (overlap.h:227-236) of every record; ``cur_name`` / ``ext_name`` map a record id
    to its container name.  With ``edge_ids`` the lines take ReadAligner::storeAlignments' form
    (read_aligner.cpp:333-335)."""
    L = load_library()
    buf = C.create_string_buffer(1024)
    out = []
    recs = np.ascontiguousarray(recs)
    for i in range(len(recs)):
        r = recs[i:i + 1]
        cn, en = cur_name(r["cur_id"][0]).encode(), ext_name(r["ext_id"][0]).encode()
        if edge_ids is None:
            n = L.fg_overlap_dump(r.ctypes.data, cn, en, buf, len(buf))
        else:
            n = L.fg_alignment_dump(int(edge_ids[i]), r.ctypes.data, cn, en, buf, len(buf))
        if n < 0:
            raise FlyeGpuError(int(n), "fg_overlap_dump")
        if n >= len(buf):
            buf = C.create_string_buffer(int(n) + 1)
            continue_n = (L.fg_overlap_dump(r.ctypes.data, cn, en, buf, len(buf)) if edge_ids is None else
                          L.fg_alignment_dump(int(edge_ids[i]), r.ctypes.data, cn, en, buf, len(buf)))
            assert continue_n == n
        out.append(buf.value.decode())
    return out


def load_overlaps(lines, cur_id_of, ext_id_of) -> np.ndarray:
    """OverlapRange::load (overlap.h:238-251): ids through the caller's recordByName lookups."""
    L = load_library()
    recs = np.zeros(len(lines), REC_DTYPE)
    offs = [C.c_uint32() for _ in range(4)]
    for i, line in enumerate(lines):
        raw = line.encode()
        rc = L.fg_overlap_load(raw, recs[i:i + 1].ctypes.data, *[C.byref(o) for o in offs])
        if rc != 0:
            raise FlyeGpuError(rc, f"malformed overlap line {i}")
        recs["cur_id"][i] = cur_id_of(raw[offs[0].value:offs[0].value + offs[1].value].decode())
        recs["ext_id"][i] = ext_id_of(raw[offs[2].value:offs[2].value + offs[3].value].decode())
    return recs


def fasta_text(rs, names) -> str:
    """SequenceContainer::writeFasta(records, file, onlyPositiveStrand = true) (sequence_container.cpp:330-357)."""
    L = load_library()
    parts = []
    for i in range(rs.n):
        w = np.ascontiguousarray(rs.words[int(rs.word_off[i]):int(rs.word_off[i + 1])])
        n = int(rs.length[i])
        cap = n + n // 80 + len(names[i]) + 8
        buf = C.create_string_buffer(cap)
        got = L.fg_fasta_record(names[i].encode(), w.ctypes.data, n, buf, cap)
        assert 0 <= got <= cap
        parts.append(buf.raw[:got].decode())
    return "".join(parts)


def complement(recs: np.ndarray) -> np.ndarray:
    """OverlapRange::complement (overlap.h:118-147) on a record array."""
    out = recs.copy()
    out["cur_begin"] = recs["cur_len"] - recs["cur_end"] - 1
    out["cur_end"] = recs["cur_len"] - recs["cur_begin"] - 1
    out["ext_begin"] = recs["ext_len"] - recs["ext_end"] - 1
    out["ext_end"] = recs["ext_len"] - recs["ext_begin"] - 1
    out["cur_id"] = recs["cur_id"] ^ 1
    out["ext_id"] = recs["ext_id"] ^ 1
    return out


class OverlapContainer:
    """Mirror of reference OverlapContainer's query side (overlap.cpp:510-827).

    Flye's worker threads ask for one read at a time; the device wants batches.
    ``prefetch`` computes and caches a batch, ``lazySeqOverlaps`` serves single reads
    from the cache (computing a batch of one on a miss)."""

    def __init__(self, ovlpDetect: OverlapDetector, first_id=None, n_reads=None):
        self.det = ovlpDetect
        self.ctx = ovlpDetect.ctx
        self._cache = {}
        self._mean_true_ovlp_div = 0.0
        self.divergence_stats = []

    def quickSeqOverlaps(self, readId: int, maxOverlaps: int = 0, forceLocal: bool = False):
        res = self.det.getSeqOverlapsBatch([readId], forceLocal, maxOverlaps)
        self.divergence_stats.extend(res.stats.tolist())
        return res.recs.copy()

    def prefetch(self, readIds):
        fwd = sorted({int(r) & ~1 for r in readIds if (int(r) & ~1) not in self._cache})
        if not fwd:
            return
        res = self.det.getSeqOverlapsBatch(fwd, False, 0)
        self.divergence_stats.extend(res.stats.tolist())
        for i, rid in enumerate(fwd):
            f = res.of(i).copy()
            self._cache[rid] = (f, complement(f))

    def lazySeqOverlaps(self, readId: int):
        fid = int(readId) & ~1
        if fid not in self._cache:
            self.prefetch([fid])
        f, r = self._cache[fid]
        return f if (int(readId) & 1) == 0 else r

    def indexSize(self):
        return sum(len(f) for f, _ in self._cache.values())

    def estimateOverlaperParameters(self, libc_rand=None):
        """overlap.cpp:744-817: median over 1000 rand()-picked records of the divergence of
        each record's longest overlap.  ``libc_rand`` defaults to glibc's rand() so the
        draw sequence is the reference's."""
        if libc_rand is None:
            libc = C.CDLL(None)
            libc.rand.restype = C.c_int
            libc_rand = libc.rand
        n_records = 2 * self.ctx.n_reads
        picks = [self.ctx.first_id + (libc_rand() % n_records) for _ in range(1000)]
        res = self.det.getSeqOverlapsBatch(picks, False, 0)
        divs = []
        for i in range(len(picks)):
            o = res.of(i)
            if len(o):
                rng = o["cur_end"] - o["cur_begin"]
                divs.append(o["seq_divergence"][int(np.argmax(rng))])  # first maximum, strict >
        if divs:
            v = sorted(divs)
            self._mean_true_ovlp_div = float(np.float32(v[len(v) // 2]))  # utils.h median()
            self.divergence_stats = []
        else:
            self._mean_true_ovlp_div = 0.5
        return self._mean_true_ovlp_div

    def setDivergenceThreshold(self, threshold: float, isRelative: bool):
        """overlap.cpp:820-827"""
        base = np.float32(self._mean_true_ovlp_div) if isRelative else np.float32(0.0)
        self.det.p.max_divergence = float(base + np.float32(threshold))
        return self.det.p.max_divergence


class ChimeraDetector:
    """Mirror of reference ChimeraDetector (src/assemble/chimera.cpp:31-343) on fg_read_coverage.

    The reference tests one read at a time from its worker threads; ``classify`` is the batched form (one prefetch
    plus one device call), ``isChimeric`` serves single reads from its cache as ``_chimeras`` does."""

    def __init__(self, ctx: Context, ovlpContainer: OverlapContainer, cfg: dict, uneven_coverage: bool):
        self.ctx, self.ovlp, self.cfg = ctx, ovlpContainer, cfg
        self.uneven_coverage = bool(uneven_coverage)
        self._overlapCoverage = 0
        self._chimeras = {}
        self._cached = {}

    def _params(self, want_vectors):
        return CoverageParams.from_config(self.cfg, self._overlapCoverage, self.uneven_coverage, want_vectors)

    def _seq_len(self, readId):
        return int(self.ctx.rs.length[(int(readId) - self.ctx.first_id) >> 1])

    def _coverage(self, readIds, want_vectors):
        """one prefetch and one device call over the lazySeqOverlaps records of readIds"""
        ids = [int(r) for r in readIds]
        self.ovlp.prefetch(ids)
        lists = [self.ovlp.lazySeqOverlaps(r) for r in ids]
        off = np.zeros(len(ids) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in lists])
        recs = np.concatenate(lists) if lists else np.zeros(0, REC_DTYPE)
        return self.ctx.read_coverage(recs, off, [self._seq_len(r) for r in ids], self._params(want_vectors))

    def getReadCoverage(self, readId):
        """chimera.cpp:106-134"""
        return self._coverage([readId], True).full_of(0)

    def classify(self, readIds):
        """testReadByCoverage (:137-202) of every read of readIds in one device call; both strands are cached
        (:49-50).  Returns a bool array."""
        ids = [int(r) for r in readIds]
        todo = sorted({r for r in ids if r not in self._chimeras})
        if todo:
            res = self._coverage(todo, False)
            for r, v in zip(todo, res.chimeric.tolist()):
                if r not in self._chimeras:         # the first verdict of a pair stands, as in the reference
                    self._chimeras[r] = v
                    self._chimeras[r ^ 1] = v
        return np.array([self._chimeras[r] for r in ids], bool)

    def testReadByCoverage(self, readId):
        return bool(self._coverage([readId], False).chimeric[0])

    def isChimeric(self, readId):
        """:31-53"""
        return bool(self.classify([readId])[0])

    def estimateGlobalCoverage(self, libc_rand=None):
        """:55-104: rand() % sampleRate per sequence in container order over both strands, the coverage of the picked
        ones in one device call, the pooled median of the vectors with a non-zero window."""
        if libc_rand is None:
            libc = C.CDLL(None)
            libc.rand.restype = C.c_int
            libc_rand = libc.rand
        n_seqs = 2 * self.ctx.n_reads
        num_samples = min(1000, n_seqs)
        if not num_samples:
            self._overlapCoverage = 0
            return 0
        sample_rate = n_seqs // num_samples
        picks = [self.ctx.first_id + i for i in range(n_seqs) if libc_rand() % sample_rate == 0]
        res = self._coverage(picks, True)
        pooled = [res.full_of(q) for q in range(len(picks)) if res.max[q] != 0]
        if not pooled:
            self._overlapCoverage = 0
        else:
            v = np.sort(np.concatenate(pooled))
            self._overlapCoverage = int(v[min(len(v) * 50 // 100, len(v) - 1)])      # utils.h median()
        return self._overlapCoverage

    def getCachedCoverage(self, readId):
        """:280-343: (coverageFullAln, coverageIncomleteAln) from force-local overlaps"""
        readId = int(readId)
        if readId not in self._cached:
            recs = self.ovlp.quickSeqOverlaps(readId, 0, True)
            res = self.ctx.read_coverage(recs, [0, len(recs)], [self._seq_len(readId)], self._params(True))
            if res.degenerate[0]:
                raise RuntimeError("Zero-sized coverage vector")
            self._cached[readId] = (res.full_of(0), res.junction_of(0))
        return self._cached[readId]

    def isRepetitiveRegion(self, readId, start, end):
        """:204-278, in float32 as written there"""
        HANG_END_RATE = np.float32(0.75)
        REPEAT_WINDOW_RATE = np.float32(0.75)
        window = self._params(True).window
        coverage, junctions = self.getCachedCoverage(readId)
        cdiv = lambda a: abs(int(a)) // window * (1 if a >= 0 else -1)      # C's division truncates
        lo = max(0, cdiv(start))
        hi = min(len(coverage), cdiv(end))
        num_suspicious = range_len = 0
        for pos in range(lo, hi):
            if HANG_END_RATE * np.float32(coverage[pos]) <= np.float32(junctions[pos]):
                num_suspicious += 1
            range_len += 1
        if range_len == 0:
            return False
        return bool(np.float32(num_suspicious) / np.float32(range_len) > REPEAT_WINDOW_RATE)


class BatchingOverlapContainer:
    """Binding of include/flye_gpu_bridge.h: the native batch scheduler that turns the
    one-read-at-a-time calls of Flye's worker threads (overlap.cpp:518-574) into device
    batches.  Every method may be called from any number of Python threads (ctypes releases
    the GIL for the duration of a call); the context must not be used directly meanwhile."""

    def __init__(self, det: OverlapDetector, max_batch=4096, linger_us=200):
        self.ctx = det.ctx
        self.L = det.ctx.L
        h = C.c_void_p()
        self.ctx._check(self.L.fgb_create(C.byref(h), self.ctx.h, C.byref(det.p), max_batch, linger_us))
        self.h = h

    def close(self):
        if self.h:
            self.L.fgb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lazySeqOverlaps(self, readId: int) -> np.ndarray:
        p, n = C.c_void_p(), C.c_uint64()
        self.ctx._check(self.L.fgb_lazy(self.h, int(readId), C.byref(p), C.byref(n)))
        if not n.value:
            return np.empty(0, REC_DTYPE)
        buf = (C.c_uint8 * (n.value * REC_DTYPE.itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=REC_DTYPE).copy()

    def quickSeqOverlaps(self, readId: int, maxOverlaps: int = 0, forceLocal: bool = False) -> np.ndarray:
        n = C.c_uint64()
        cap = 4096
        while True:
            out = np.empty(cap, REC_DTYPE)
            self.ctx._check(self.L.fgb_quick(self.h, int(readId), maxOverlaps, int(bool(forceLocal)),
                                             out.ctypes.data, cap, C.byref(n)))
            if n.value <= cap:
                return out[:n.value]
            cap = int(n.value)

    def prefetch(self, readIds):
        q = np.ascontiguousarray(readIds, dtype=np.uint32)
        self.ctx._check(self.L.fgb_prefetch(self.h, q.ctypes.data, len(q)))

    def setDivergenceThreshold(self, maxDivergence: float):
        self.ctx._check(self.L.fgb_set_divergence_threshold(self.h, float(maxDivergence)))

    def divergenceStats(self) -> np.ndarray:
        n = self.L.fgb_divergence_stats(self.h, None, 0)
        out = np.empty(n, np.float32)
        self.L.fgb_divergence_stats(self.h, out.ctypes.data, n)
        return out

    def stats(self) -> dict:
        st = BridgeStats()
        self.L.fgb_get_stats(self.h, C.byref(st))
        return {k: int(getattr(st, k)) for k, _ in st._fields_}


class BubbleProcessor:
    """Mirror of the reference's BubbleProcessor (src/polishing/bubble_processor.cpp) on fg_polish_bubbles: reads a
    bubbles file as cacheBubbles does (:151-204), polishes every bubble in one device call and writes the consensus file
    and the --debug log as one worker thread would (:75-148)."""

    BUBBLES_CACHE = 100

    def __init__(self, ctx: Context, subs_matrix_path, fix_dinucleotides=True):
        self.ctx = ctx
        self.matrix = SubstitutionMatrix(subs_matrix_path)
        self.fix_dinucleotides = fix_dinucleotides

    @staticmethod
    def read_bubbles(path):
        """-> [(header, position, candidate, [branches])], everything upper-cased, up to the first empty header line"""
        with open(path, "rb") as f:
            lines = f.read().decode("latin-1").split("\n")
        if lines == [""]:
            raise RuntimeError("Empty bubbles file!")
        lines.append("")
        out, at = [], 0
        while at < len(lines) - 1:
            buf = lines[at]
            if not buf:
                break
            elems = buf.split(" ")
            if len(elems) < 3 or elems[0][:1] != ">":
                raise RuntimeError("Error parsing bubbles file")
            cand = lines[min(at + 1, len(lines) - 1)].upper()
            at += 2
            branches = []
            for _ in range(int(elems[2])):
                if not buf:       # the line before was empty: the reference stops counting here and throws
                    raise RuntimeError("Error parsing bubbles file")
                buf = lines[min(at + 1, len(lines) - 1)].upper()
                at += 2
                branches.append(buf)
            out.append((elems[0][1:], int(elems[1]), cand, branches))
        return out

    def polishAll(self, in_bubbles, out_consensus, log_path=None):
        bubbles = self.read_bubbles(in_bubbles)
        cand = "".join(b[2] for b in bubbles).encode("latin-1")
        flat = [w for b in bubbles for w in b[3]]
        res = self.ctx.polish_bubbles(self.matrix, cand, np.cumsum([0] + [len(b[2]) for b in bubbles]),
                                      "".join(flat).encode("latin-1"), np.cumsum([0] + [len(w) for w in flat]),
                                      np.cumsum([0] + [len(b[3]) for b in bubbles]), self.fix_dinucleotides,
                                      want_steps=log_path is not None)
        order = []
        for a in range(0, len(bubbles), self.BUBBLES_CACHE):
            order += range(min(a + self.BUBBLES_CACHE, len(bubbles)) - 1, a - 1, -1)
        with open(out_consensus, "wb") as f:
            for i in order:
                b = bubbles[i]
                f.write((">%s %d %d\n" % (b[0], b[1], len(b[3]))).encode("latin-1") + res.candidates[i] + b"\n")
        if log_path is not None:
            with open(log_path, "wb") as f:
                for i in order:
                    for seq, score in res.steps[i]:
                        f.write(b"%-22s%s\n%-22s%d\n\n" % (b"Consensus: ", seq, b"Score: ", score))
                    f.write(b"-----------------\n")
        return res


class BubbleMaker:
    """Mirror of the reference's flye/polishing/bubbles.py on fg_make_bubbles.  Alignments are records with the fields of
    the reference's Alignment tuple (trg_start, trg_end, trg_seq, qry_seq, err_rate, is_secondary are read); contigs are
    records with id, length and type.  SamAlignments.by_contig() makes the alignments of a SAM file."""

    WINDOW, MIN_COV, COV_RATE = 100, 10, 1.25

    def __init__(self, ctx: Context, **overrides):
        self.ctx = ctx
        self.overrides = overrides
        self.contigs, self.result = [], None

    @classmethod
    def uniform_alignments(cls, alignments, seq_len):
        """get_uniform_alignments (flye/polishing/alignment.py:95-153): per 100 bp window the best alignments up to 1.25
        times the median primary coverage; an alignment stays when it passes in more than half of its windows.  Raises
        ValueError where the reference raises IndexError (an alignment that ends beyond the last window)."""
        n_w = seq_len // cls.WINDOW + 1
        primary = [0] * n_w
        quality = [[] for _ in range(n_w)]
        for aln in alignments:
            for i in range(aln.trg_start // cls.WINDOW, aln.trg_end // cls.WINDOW):
                if i >= n_w:
                    raise ValueError("uniform_alignments: an alignment ends beyond the contig")
                if not aln.is_secondary:
                    primary[i] += 1
                quality[i].append(aln.err_rate)
        ordered = sorted(primary)
        median = ordered[n_w // 2] if n_w % 2 else (ordered[n_w // 2 - 1] + ordered[n_w // 2]) / 2
        cov_threshold = max(int(cls.COV_RATE * median), cls.MIN_COV)
        threshold = [sorted(q)[cov_threshold] if len(q) > cov_threshold else 1.0 for q in quality]
        kept = []
        for aln in alignments:
            first, last = aln.trg_start // cls.WINDOW, aln.trg_end // cls.WINDOW
            good = sum(1 for i in range(first, last) if aln.err_rate <= threshold[i])
            if good > (last - first) // 2:
                kept.append(aln)
        return kept

    @staticmethod
    def uniform_alignments_device(ctx, alignments, seq_len):
        """the same list through fg_uniform_alignments (Context.uniform_alignments)"""
        res = ctx.uniform_alignments([seq_len], [0, len(alignments)], [a.trg_start for a in alignments],
                                     [a.trg_end for a in alignments], [a.err_rate for a in alignments],
                                     [bool(a.is_secondary) for a in alignments])
        return [a for a, k in zip(alignments, res.keep) if k]

    def make(self, contigs, alignments_by_contig, err_mode, want_profile=False):
        """make_bubbles for the contigs in the given order -> (bubbles, coverage_stats, mean_aln_error); bubbles is a list
        of (contig id, position, consensus bytes, [branch bytes]).  mean_aln_error is sum / (n + 1) over the profiled
        alignments summed in contig order (the reference sums in the order its workers finish, so its last bits depend on
        the run)."""
        params = BubbleParams.for_mode(err_mode, **self.overrides)
        alns = [a for c in contigs for a in alignments_by_contig.get(c.id, [])]
        trg = "".join(a.trg_seq for a in alns).encode("latin-1")
        qry = "".join(a.qry_seq for a in alns).encode("latin-1")
        res = self.ctx.make_bubbles(params, [c.length for c in contigs], [c.type == "circular" for c in contigs],
                                    np.cumsum([0] + [len(alignments_by_contig.get(c.id, [])) for c in contigs]),
                                    [a.trg_start for a in alns], [a.trg_end for a in alns], [a.err_rate for a in alns],
                                    np.cumsum([0] + [len(a.trg_seq) for a in alns]), trg, qry, want_profile)
        return self._finish(contigs, alns, res)

    def _finish(self, contigs, alns, res):
        self.contigs, self.result = list(contigs), res
        self.bubbles = [(c.id,) + b for i, c in enumerate(contigs) for b in res.bubbles(i)]
        self.aln_errors = [a.err_rate for a, f in zip(alns, res.in_profile) if f]
        coverage_stats = {c.id: int(res.mean_cov[i]) for i, c in enumerate(contigs)}
        total = 0.0
        for e in self.aln_errors:
            total += e
        return self.bubbles, coverage_stats, total / (len(self.aln_errors) + 1)

    def write_bubbles(self, path):
        """the bubbles of the last make() in the form of _output_bubbles (bubbles.py:159-172)"""
        with open(path, "wb") as f:
            for cid, position, cons, branches in self.bubbles:
                f.write((">%s %d %d\n" % (cid, position, len(branches))).encode("latin-1") + cons + b"\n")
                for k, w in enumerate(branches):
                    f.write(b">%d\n%s\n" % (k, w))

    def make_sam(self, contigs, sam, err_mode, want_profile=False, uniform=True):
        """make() for a SamAlignments made with want_cols=False: fg_uniform_alignments (the reference's make_bubbles
        starts with get_uniform_alignments), then ONE fg_make_bubbles_cigars on the records it keeps, which expands their
        CIGARs on the device straight into the bubble kernels' buffers.  Returns what make() returns for
        sam.by_contig() with every list put through uniform_alignments_device first (uniform=False: for the lists as
        they are); err_rate is the one the want_cols=False expansion counted."""
        params = BubbleParams.for_mode(err_mode, **self.overrides)
        keep = None
        if uniform:
            alns, rec = sam.flatten(contigs)
            keep = self.ctx.uniform_alignments(np.diff(rec["contig_off"]), rec["contig_aln_off"], [a.trg_start for a in alns],
                                               [a.trg_end for a in alns], [a.err_rate for a in alns],
                                               [bool(a.is_secondary) for a in alns]).keep
        alns, rec = sam.flatten(contigs, keep)
        res = self.ctx.make_bubbles_cigars(params, contig_circular=[c.type == "circular" for c in contigs],
                                           err_rate=[a.err_rate for a in alns], want_profile=want_profile, **rec)
        return self._finish(contigs, alns, res)

    def polish_sam(self, contigs, sam, err_mode, matrix, fix_dinucleotides=True, want_steps=False, uniform=True):
        """polish() on make_sam(): the fused call, then Context.polish_bubbles"""
        bubbles, _, _ = self.make_sam(contigs, sam, err_mode, uniform=uniform)
        return bubbles, self._polish_result(matrix, fix_dinucleotides, want_steps)

    def polish(self, contigs, alignments_by_contig, err_mode, matrix, fix_dinucleotides=True, want_steps=False):
        """the two device stages as one call: make() -> upper case (the polisher's reader does that, bubble_processor.cpp:
        151-204) -> Context.polish_bubbles.  Returns (bubbles, PolishResult); the branch bytes go back as they came."""
        bubbles, _, _ = self.make(contigs, alignments_by_contig, err_mode)
        return bubbles, self._polish_result(matrix, fix_dinucleotides, want_steps)

    def _polish_result(self, matrix, fix_dinucleotides, want_steps):
        r = self.result
        upper = lambda a: np.frombuffer(a.tobytes().upper(), np.uint8)
        return self.ctx.polish_bubbles(matrix, upper(r.cand), r.cand_off, upper(r.branches), r.branch_off,
                                       r.bubble_branch_off, fix_dinucleotides, want_steps)


class ContigConsensus:
    """Mirror of the reference's get_consensus (flye/polishing/consensus.py:52-105) on fg_uniform_alignments and
    fg_contig_consensus.  Alignments are records with the fields of the reference's Alignment tuple (qry_id, trg_start,
    trg_end, trg_seq, qry_seq, err_rate, is_secondary are read); contigs are records with id and length.  SamAlignments.by_contig()
    makes the alignments of a SAM file; FASTA writing stays with the caller."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.result, self.uniform, self.aln_errors = None, None, []

    def consensus(self, contigs, alignments_by_contig, uniform=True, want_profile=False):
        """-> ({contig id: sequence} without the empty ones, mean_aln_error).  mean_aln_error is sum / (n + 1) over the
        alignments that took part, summed in contig order (the reference sums in the order its workers finish, so its
        last bits depend on the run).  The strings of qry_id are numbered per contig in the order they first appear."""
        lists = [alignments_by_contig.get(c.id, []) for c in contigs]
        alns = [a for lst in lists for a in lst]
        aln_off = np.cumsum([0] + [len(lst) for lst in lists])
        lengths = [c.length for c in contigs]
        starts = [a.trg_start for a in alns]
        qry_id = []
        for lst in lists:
            number = {}
            qry_id += [number.setdefault(a.qry_id, len(number)) for a in lst]
        use = None
        if uniform:
            self.uniform = self.ctx.uniform_alignments(lengths, aln_off, starts, [a.trg_end for a in alns],
                                                       [a.err_rate for a in alns], [bool(a.is_secondary) for a in alns])
            use = self.uniform.keep
        res = self.ctx.contig_consensus(lengths, aln_off, starts, qry_id, np.cumsum([0] + [len(a.trg_seq) for a in alns]),
                                        "".join(a.trg_seq for a in alns).encode("latin-1"),
                                        "".join(a.qry_seq for a in alns).encode("latin-1"), use, want_profile)
        return self._finish(contigs, alns, use, res)

    def _finish(self, contigs, alns, use, res):
        self.result = res
        self.aln_errors = [a.err_rate for k, a in enumerate(alns) if use is None or use[k]]
        total = 0.0
        for e in self.aln_errors:
            total += e
        out = {}
        for i, c in enumerate(contigs):
            seq = res.sequence(i)
            if len(seq) > 0:
                out[c.id] = seq.decode("latin-1")
        return out, total / (len(self.aln_errors) + 1)

    def consensus_sam(self, contigs, sam, uniform=True, want_profile=False):
        """consensus(contigs, sam.by_contig(), ...) for a SamAlignments made with want_cols=False: one
        fg_uniform_alignments and one fg_contig_consensus_cigars, which expands the CIGARs on the device straight into
        the consensus kernels' buffers.  No gapped string exists on the host at any point."""
        alns, rec = sam.flatten(contigs)
        aln_off = rec["contig_aln_off"]
        qry_id = []
        for i in range(len(contigs)):
            number = {}
            qry_id += [number.setdefault(a.qry_id, len(number)) for a in alns[int(aln_off[i]):int(aln_off[i + 1])]]
        use = None
        if uniform:
            self.uniform = self.ctx.uniform_alignments(np.diff(rec["contig_off"]), aln_off, [a.trg_start for a in alns],
                                                       [a.trg_end for a in alns], [a.err_rate for a in alns],
                                                       [bool(a.is_secondary) for a in alns])
            use = self.uniform.keep
        return self._finish(contigs, alns, use, self.ctx.contig_consensus_cigars(qry_id=qry_id, use=use, want_profile=want_profile,
                                                                                 **rec))


class DivergenceFinder:
    """Mirror of the reference's find_divergence (flye/trestle/divergence.py:146-232) on fg_divergence_profile: the SAM
    file goes through SamAlignments (with max_read_coverage, as the reference's reader), every contig with records
    through ONE device call, and the three text files are written with the reference's format strings.  Kept from the
    reference: each contig's result overwrites the files, so they hold the last contig in chunk order (the reference at
    num_proc = 1; Trestle passes one template); a file without an aligned record writes nothing.  Where a file is
    missing the reference ends in ValueError (_get_median of an empty list); so does this, before it writes anything."""

    WINDOW = 1000

    def __init__(self, ctx: Context, max_read_coverage=1000):
        self.ctx = ctx
        self.max_read_coverage = max_read_coverage
        self.result, self.aln_errors = None, []

    # read_sequence_dict hands the reader contigs whose IUPAC codes stand for A, C, G, T in turn, case kept
    IUPAC = b"URYKMSWBVDHNX"
    TO_ACGT = bytes.maketrans(IUPAC + IUPAC.lower(), (b"ACGT" * 4)[:13] + (b"acgt" * 4)[:13])

    @classmethod
    def read_fasta(cls, path):
        """{header up to the first blank: sequence} of a FASTA file, plain or .gz, as bytes, non-ACGT codes replaced as
        the reference's read_sequence_dict replaces them"""
        opener = gzip.open if path.endswith(".gz") else open
        out, header = {}, None
        with opener(path, "rb") as f:
            for line in f:
                line = line.strip()
                if line.startswith(b">"):
                    header = line[1:].split()[0]
                    out[header] = []
                elif line and header is not None:
                    out[header].append(line)
        return {h: b"".join(s).translate(cls.TO_ACGT) for h, s in out.items() if s}

    def profile(self, alignments_by_contig, contigs, sub_thresh, del_thresh, ins_thresh, want_profile=True):
        """one device call for the contigs (records with id and length) in order -> DivergenceResult; aln_errors takes
        the err_rate of every alignment, as _contig_profile returns them"""
        lists = [alignments_by_contig.get(c.id, []) for c in contigs]
        alns = [a for lst in lists for a in lst]
        self.aln_errors = [a.err_rate for a in alns]
        self.result = self.ctx.divergence_profile(
            sub_thresh, del_thresh, ins_thresh, [c.length for c in contigs], np.cumsum([0] + [len(lst) for lst in lists]),
            [a.trg_start for a in alns], np.cumsum([0] + [len(a.trg_seq) for a in alns]),
            "".join(a.trg_seq for a in alns).encode("latin-1"), "".join(a.qry_seq for a in alns).encode("latin-1"), want_profile)
        return self.result

    @staticmethod
    def frequency_text(res, i):
        """the lines _write_frequency_path writes for contig i of a result with its profile"""
        lo, hi = int(res.prof_off[i]), int(res.prof_off[i + 1])
        out = ["Index\tCov\tMatch\tCount\tSub\tCount\tDel\tCount\tIns\tCount\n"]
        char = [chr(b) for b in range(128)]
        char[0] = ""
        for k, (cov, nucl, mat, sb, sc, dc, ib, ic) in enumerate(zip(
                res.cov[lo:hi].tolist(), res.nucl[lo:hi].tolist(), res.mat_ct[lo:hi].tolist(), res.sub_base[lo:hi].tolist(),
                res.sub_ct[lo:hi].tolist(), res.del_ct[lo:hi].tolist(), res.ins_base[lo:hi].tolist(), res.ins_ct[lo:hi].tolist())):
            out.append("%d\t%d\t%s\t%d\t%s\t%d\t-\t%d\t^%s\t%d\n" % (k, cov, char[nucl], mat, char[sb], sc, dc, char[ib], ic))
        return "".join(out)

    @staticmethod
    def positions_text(pos, sub_thresh, del_thresh, ins_thresh):
        """the four headers and lists of _write_positions"""
        heads = ("Total_positions_{0}_with_thresholds_sub_{1}_del_{2}_ins_{3}".format(len(pos["total"]), sub_thresh, del_thresh, ins_thresh),
                 "Sub_positions_{0}_with_threshold_sub_{1}".format(len(pos["sub"]), sub_thresh),
                 "Del_positions_{0}_with_threshold_del_{1}".format(len(pos["del"]), del_thresh),
                 "Ins_positions_{0}_with_threshold_ins_{1}".format(len(pos["ins"]), ins_thresh))
        return "".join(">{0}\n{1}\n".format(h, ",".join(str(x) for x in pos[k])) for h, k in zip(heads, ("total", "sub", "del", "ins")))

    @classmethod
    def summary_text(cls, pos, seq_len):
        """_write_div_summary: the gaps between called positions and the divergence of windows of 1000"""
        called = pos["total"]
        gaps = [b - a for a, b in zip([0] + called, called + [seq_len])]
        n_win = (seq_len - 1) // cls.WINDOW + 1
        counts = [0] * max(n_win, 0)
        for p in called:
            counts[p // cls.WINDOW] += 1
        divs = [counts[w] / float(min((w + 1) * cls.WINDOW, seq_len) - w * cls.WINDOW) for w in range(len(counts))]
        if not divs:
            raise ValueError("_get_median() arg is an empty sequence")
        ordered = sorted(divs)
        mid = len(divs) // 2
        median = ordered[mid] if len(divs) % 2 else (ordered[mid - 1] + ordered[mid]) / 2
        rows = (("Sequence Length:", "{1}", seq_len, "\n"), ("Average Divergence:", "{1:.4f}", len(called) / float(seq_len), "\n\n"),
                ("Total Substitution Positions:", "{1}", len(pos["sub"]), "\n"), ("Total Deletion Positions:", "{1}", len(pos["del"]), "\n"),
                ("Total Insertion Positions:", "{1}", len(pos["ins"]), "\n"), ("Total Positions:", "{1}", len(called), "\n"),
                ("Mixed Positions:", "{1}", len(pos["sub"]) + len(pos["del"]) + len(pos["ins"]) - len(called), "\n\n"),
                ("Mean Position Gap:", "{1:.2f}", sum(gaps) / len(gaps), "\n"), ("Max Position Gap:", "{1}", max(gaps), "\n"),
                ("Window Length:", "{1}", cls.WINDOW, "\n"), ("Mean Window Divergence:", "{1:.5f}", sum(divs) / len(divs), "\n"),
                ("Median Window Divergence:", "{1:.5f}", median, "\n"), ("Min Window Divergence:", "{1:.5f}", min(divs), "\n"))
        return "Tentative Divergent Position Summary\n\n" + "".join(("{0:33}\t" + fmt + end).format(label, value)
                                                                   for label, fmt, value, end in rows)

    def find_divergence(self, alignment_path, contigs_path, contigs_info, frequency_path, positions_path, div_sum_path,
                        sub_thresh, del_thresh, ins_thresh, device_text=False):
        """-> mean_aln_error = sum(err_rate) / (n + 1), which the reference logs.  contigs_info maps contig id to a record
        with length."""
        if not os.path.isfile(alignment_path) or not os.path.isfile(contigs_path):
            raise ValueError("_get_median() arg is an empty sequence")
        sam = SamAlignments(self.ctx, alignment_path, self.read_fasta(contigs_path), self.max_read_coverage, device_text=device_text)
        chunks = sam.chunks()
        Contig = collections.namedtuple("Contig", ["id", "length"])
        contigs = [Contig(cid, contigs_info[cid].length) for cid, _ in chunks]
        res = self.profile(dict(chunks), contigs, sub_thresh, del_thresh, ins_thresh)
        if contigs:                                     # every contig overwrites the files: the last one stays
            i = len(contigs) - 1
            pos = res.positions(i)
            texts = ((frequency_path, self.frequency_text(res, i)), (positions_path, self.positions_text(pos, sub_thresh, del_thresh, ins_thresh)),
                     (div_sum_path, self.summary_text(pos, contigs[i].length)))
            for path, text in texts:
                with open(path, "w") as f:
                    f.write(text)
        return sum(self.aln_errors) / (len(self.aln_errors) + 1)

    def profile_sam(self, sam, contigs, sub_thresh, del_thresh, ins_thresh, want_profile=True):
        """profile(sam.by_contig(), contigs, ...) for a SamAlignments made with want_cols=False: one
        fg_divergence_profile_cigars, which expands the CIGARs on the device straight into the divergence kernels'
        buffers.  contigs are records with id; their bytes are the reader's.  No gapped string exists on the host."""
        alns, rec = sam.flatten(contigs)
        self.aln_errors = [a.err_rate for a in alns]
        self.result = self.ctx.divergence_profile_cigars(sub_thresh, del_thresh, ins_thresh, want_profile=want_profile, **rec)
        return self.result

    def find_divergence_sam(self, alignment_path, contigs_path, contigs_info, frequency_path, positions_path, div_sum_path,
                            sub_thresh, del_thresh, ins_thresh, device_text=False):
        """find_divergence on profile_sam: the same three files and the same return value.  A contig's positions are
        those of the bytes read from contigs_path, which is where the reference's contigs_info has its lengths from."""
        if not os.path.isfile(alignment_path) or not os.path.isfile(contigs_path):
            raise ValueError("_get_median() arg is an empty sequence")
        sam = SamAlignments(self.ctx, alignment_path, self.read_fasta(contigs_path), self.max_read_coverage, want_cols=False,
                            device_text=device_text)
        Contig = collections.namedtuple("Contig", ["id", "length"])
        contigs = [Contig(cid, contigs_info[cid].length) for cid, _ in sam.chunks()]
        res = self.profile_sam(sam, contigs, sub_thresh, del_thresh, ins_thresh)
        if contigs:                                     # every contig overwrites the files: the last one stays
            i = len(contigs) - 1
            pos = res.positions(i)
            texts = ((frequency_path, self.frequency_text(res, i)), (positions_path, self.positions_text(pos, sub_thresh, del_thresh, ins_thresh)),
                     (div_sum_path, self.summary_text(pos, contigs[i].length)))
            for path, text in texts:
                with open(path, "w") as f:
                    f.write(text)
        return sum(self.aln_errors) / (len(self.aln_errors) + 1)


class ReadPartitioner:
    """Mirror of the reference's partition_reads (flye/trestle/trestle.py:1075-1142) on fg_confirm_positions and
    fg_classify_reads: the SAM files go through SamAlignments (first chunk only, as the reference takes [0]), the
    consensus alignments are collapsed on the host, and the two text files are written with the reference's format
    strings.  Both skip paths are the reference's: a missing file or an empty alignment gives empty lists at it <= 1 and
    the confirmed file of it - 1 later, and the partitioning of it - 1 is written again.  confirm and classify take
    several jobs in ONE device call each."""

    MAX_SUPP_ALIGN_OVERLAP = 100
    KEYS = ("total", "sub", "del", "ins")
    STATUS = ("None", "Tied", "Partitioned")

    def __init__(self, ctx: Context, max_read_coverage=1000, buffer_count=3):
        self.ctx = ctx
        self.max_read_coverage, self.buffer_count = max_read_coverage, buffer_count

    # ---- the text files --------------------------------------------------------------------------------------------
    @classmethod
    def read_positions(cls, path):
        """divergence.py:362-396: lines 1, 3, 5, 7 are the total, sub, del and ins lists"""
        pos = {k: [] for k in cls.KEYS}
        try:
            with open(path, "r") as f:
                for i, line in enumerate(f):
                    line = line.strip()
                    if i < 8 and i % 2 == 1 and line:
                        pos[cls.KEYS[i // 2]] = [int(x) for x in line.split(",")]
                    elif line and not (i < 8 and i % 2 == 0 and line.startswith(">")):
                        raise ValueError("Not a valid positions file")
        except IOError as e:
            raise ValueError(str(e))
        return pos

    @classmethod
    def _write_confirmed_positions(cls, confirmed, rejected, pos, out_file):
        with open(out_file, "w") as f:
            for label, lists in (("Confirmed", confirmed), ("Rejected", rejected), ("Tentative", pos)):
                for k in cls.KEYS:
                    f.write(">{0}_{1}_positions_{2}\n".format(label, k, len(lists[k])))
                    f.write(",".join([str(x) for x in sorted(lists[k])]) + "\n")

    @classmethod
    def _read_confirmed_positions(cls, confirmed_file):
        out = [{k: [] for k in cls.KEYS} for _ in range(3)]
        with open(confirmed_file, "r") as f:
            for i, line in enumerate(f):
                line = line.strip()
                if i % 2 == 1 and i < 24 and line:
                    out[i // 8][cls.KEYS[i % 8 // 2]] = [int(x) for x in line.split(",")]
        return tuple(out)

    @staticmethod
    def _write_partitioning_file(part_list, part_path):
        with open(part_path, "w") as f:
            rows = [["Read_ID", "Status", "Edge", "Top Score", "Total Score", "Header"]] + sorted(part_list)
            for row in rows:
                f.write("\t".join(["{:11}".format(h) for h in row]) + "\n")

    @staticmethod
    def _read_partitioning_file(partitioning_file):
        part_list = []
        with open(partitioning_file, "r") as f:
            for i, line in enumerate(f):
                if i > 0:
                    tokens = [t.strip() for t in line.strip().split("\t")]
                    for k in (0, 3, 4):
                        tokens[k] = int(tokens[k])
                    part_list.append(tuple(tokens))
        return part_list

    # ---- collapsing the consensus alignments (:1160-1331) ----------------------------------------------------------
    @staticmethod
    def _axis_overlap(s1, e1, s2, e2):
        lens = []
        if s2 <= s1 < e2:
            lens.append(e2 - s1 if e1 >= e2 else e1 - s1)
        if s2 < e1 <= e2:
            lens.append(e1 - s2 if s1 <= s2 else e1 - s1)
        if s1 <= s2 < e1:
            lens.append(e1 - s2 if e2 >= e1 else e2 - s2)
        if s1 < e2 <= e1:
            lens.append(e2 - s1 if s2 <= s1 else e2 - s2)
        return min(lens) if lens else 0

    @classmethod
    def _overlap(cls, one, two):
        return max(cls._axis_overlap(one.qry_start, one.qry_end, two.qry_start, two.qry_end),
                   cls._axis_overlap(one.trg_start, one.trg_end, two.trg_start, two.trg_end))

    @staticmethod
    def _merge_alns(first_start, first_end, first_seq, second_start, second_end, second_seq):
        if first_end <= second_start:
            return first_seq + "N" * (second_start - first_end), second_seq, second_end
        if first_end >= second_end:
            return first_seq, "", first_end
        # the second string from behind its first (first_end - second_start) bases on
        bases, cut = 0, len(second_seq)
        for i, b in enumerate(second_seq):
            bases += b != "-"
            if bases == first_end - second_start:
                cut = i + 1
                break
        return first_seq, second_seq[cut:], second_end

    @classmethod
    def _collapse(cls, one, two):
        if one.qry_sign == "-" or two.qry_sign == "-" or cls._overlap(one, two) > cls.MAX_SUPP_ALIGN_OVERLAP:
            return one
        if one.qry_start <= two.qry_start and one.trg_start <= two.trg_start:
            left, right = one, two
        elif two.qry_start <= one.qry_start and two.trg_start <= one.trg_start:
            left, right = two, one
        else:
            return one
        lq, rq, qry_end = cls._merge_alns(left.qry_start, left.qry_end, left.qry_seq, right.qry_start, right.qry_end, right.qry_seq)
        lt, rt, trg_end = cls._merge_alns(left.trg_start, left.trg_end, left.trg_seq, right.trg_start, right.trg_end, right.trg_seq)
        diff = len(lq) + len(rq) - len(lt) - len(rt)
        err_rate = (one.err_rate * len(one.trg_seq) + two.err_rate * len(two.trg_seq)) / (len(one.trg_seq) + len(two.trg_seq))
        return Alignment(one.qry_id, one.trg_id, left.qry_start, qry_end, one.qry_sign, one.qry_len, left.trg_start, trg_end,
                         one.trg_sign, one.trg_len, lq + "-" * max(-diff, 0) + rq, lt + "-" * max(diff, 0) + rt, err_rate, False)

    @classmethod
    def _collapse_cons_aln(cls, cons_aligns):
        coll = None
        for aln in cons_aligns[0]:
            if coll is None:
                coll = aln
            elif cls._overlap(coll, aln) <= cls.MAX_SUPP_ALIGN_OVERLAP:
                coll = cls._collapse(coll, aln)
        return coll

    # ---- the device calls ------------------------------------------------------------------------------------------
    @staticmethod
    def _columns(alns):
        return (np.cumsum([0] + [len(a.trg_seq) for a in alns]), "".join(a.trg_seq for a in alns).encode("latin-1"),
                "".join(a.qry_seq for a in alns).encode("latin-1"))

    def confirm(self, jobs):
        """jobs: [(pos, {edge_id: collapsed alignment}, side)] -> [(confirmed, rejected, {edge_id: consensus_pos})], what
        _evaluate_positions returns per job, in one device call"""
        alns = [a for _, cons, _ in jobs for a in cons.values()]
        lists = [x for k in self.KEYS for x in (np.cumsum([0] + [len(pos[k]) for pos, _, _ in jobs]), [p for pos, _, _ in jobs for p in pos[k]])]
        res = self.ctx.confirm_positions([("in", "out").index(side) for _, _, side in jobs], np.cumsum([0] + [len(cons) for _, cons, _ in jobs]),
                                         [a.trg_start for a in alns], [a.trg_end for a in alns], [a.qry_start for a in alns],
                                         *self._columns(alns), *lists)
        out, e = [], 0
        for j, (_, cons, _) in enumerate(jobs):
            confirmed, rejected = res.positions(j)
            out.append((confirmed, rejected, {edge_id: res.consensus_pos(e + i) for i, edge_id in enumerate(cons)}))
            e += len(cons)
        return out

    def classify(self, jobs):
        """jobs: [(read_aligns {edge_id: [alignments of the first chunk, ...]}, consensus_pos, headers_to_id)] -> the
        partitioning list of _classify_reads per job, in one device call.  Alignments of reads headers_to_id does not
        hold take no part: the reference scores them and never reports them."""
        job_edges, numbers, kept = [], [], []
        for read_aligns, _, headers_to_id in jobs:
            number = {h: i for i, h in enumerate(headers_to_id)}
            numbers.append(number)
            job_edges.append([[a for a in read_aligns[e][0] if a.trg_id != "*" and a.qry_id in number] for e in read_aligns])
        edges = [lst for je in job_edges for lst in je]
        pos = [list(cons_pos[e]) for read_aligns, cons_pos, _ in jobs for e in read_aligns]
        alns = [a for lst in edges for a in lst]
        reads = [number[a.qry_id] for je, number in zip(job_edges, numbers) for lst in je for a in lst]
        res = self.ctx.classify_reads(self.buffer_count, np.cumsum([0] + [len(je) for je in job_edges]), [len(n) for n in numbers],
                                      np.cumsum([0] + [len(p) for p in pos]), [x for p in pos for x in p],
                                      np.cumsum([0] + [len(lst) for lst in edges]), reads, [a.trg_start for a in alns],
                                      [a.trg_end for a in alns], *self._columns(alns))
        out = []
        for j, (read_aligns, _, headers_to_id) in enumerate(jobs):
            ids = list(read_aligns)
            out.append([(headers_to_id[h], self.STATUS[st], str(ids[edge]) if st == 2 else "NA", top, total, h)
                        for h, (st, edge, top, total) in zip(headers_to_id, res.reads(j))])
        return out

    def classify_sam(self, jobs):
        """classify for read alignments kept as SamRecords: jobs are [(read_aligns {edge_id: [records of the first chunk,
        ...]}, consensus_pos, headers_to_id, edge_seqs {edge_id: the bytes of the consensus the first chunk lies on})], and
        ONE fg_classify_reads_cigars expands the CIGARs on the device straight into the scoring kernels' buffers.  No
        gapped string of a read alignment exists on the host."""
        job_edges, numbers, seqs = [], [], []
        for read_aligns, _, headers_to_id, edge_seqs in jobs:
            number = {h: i for i, h in enumerate(headers_to_id)}
            numbers.append(number)
            job_edges.append([[r for r in read_aligns[e][0] if r.trg_id != "*" and r.qry_id in number] for e in read_aligns])
            seqs += [edge_seqs[e] if isinstance(edge_seqs[e], bytes) else edge_seqs[e].encode("latin-1") for e in read_aligns]
        edges = [lst for je in job_edges for lst in je]
        pos = [list(cons_pos[e]) for read_aligns, cons_pos, _, _ in jobs for e in read_aligns]
        recs = [r for lst in edges for r in lst]
        reads = [number[r.qry_id] for je, number in zip(job_edges, numbers) for lst in je for r in lst]
        res = self.ctx.classify_reads_cigars(
            self.buffer_count, np.cumsum([0] + [len(je) for je in job_edges]), [len(n) for n in numbers],
            np.cumsum([0] + [len(p) for p in pos]), [x for p in pos for x in p], np.cumsum([0] + [len(x) for x in seqs]), b"".join(seqs),
            np.cumsum([0] + [len(lst) for lst in edges]), reads, [r.ctg_pos for r in recs], np.cumsum([0] + [len(r.ops) for r in recs]),
            np.concatenate([r.ops for r in recs]) if recs else np.zeros(0, np.uint8),
            np.concatenate([r.lens for r in recs]) if recs else np.zeros(0, np.uint32),
            np.cumsum([0] + [len(r.seq) for r in recs]), b"".join(r.seq for r in recs))
        out = []
        for j, (read_aligns, _, headers_to_id, _) in enumerate(jobs):
            ids = list(read_aligns)
            out.append([(headers_to_id[h], self.STATUS[st], str(ids[edge]) if st == 2 else "NA", top, total, h)
                        for h, (st, edge, top, total) in zip(headers_to_id, res.reads(j))])
        return out

    def _read_records(self, alignment, target_path, device_text=False):
        """-> ([records per chunk], the consensus bytes the first chunk lies on)"""
        sam = SamAlignments(self.ctx, alignment, DivergenceFinder.read_fasta(target_path), self.max_read_coverage, want_cols=False,
                            device_text=device_text)
        chunks = sam.chunks()
        return [recs for _, recs in chunks], sam.contigs[chunks[0][0].encode("latin-1")] if chunks else b""

    def partition_reads_sam(self, edges, it, side, position_path, cons_align_path, template, read_align_path, consensuses,
                            confirmed_pos_path, part_file, headers_to_id, device_text=False):
        """partition_reads with the read SAM files read without columns and scored by classify_sam; the consensus SAM
        files are read as there and go through confirm.  The same two files."""
        skip = False
        pos = self.read_positions(position_path)
        cons_aligns = {}
        for edge_id in edges:
            if not os.path.isfile(cons_align_path.format(it, side, edge_id)):
                skip = True
            else:
                cons_aligns[edge_id] = self._read_alignment(cons_align_path.format(it, side, edge_id), template, device_text)
            if skip or not cons_aligns or not cons_aligns[edge_id] or not cons_aligns[edge_id][0]:
                skip = True
        if skip:
            if it <= 1:
                confirmed, rejected = {k: [] for k in self.KEYS}, {k: [] for k in self.KEYS}
                consensus_pos = pos
            else:
                confirmed, rejected, consensus_pos = self._read_confirmed_positions(confirmed_pos_path.format(it - 1, side))
        else:
            coll = {edge_id: self._collapse_cons_aln(aln) for edge_id, aln in cons_aligns.items()}
            (confirmed, rejected, consensus_pos), = self.confirm([(pos, coll, side)])
        self._write_confirmed_positions(confirmed, rejected, pos, confirmed_pos_path.format(it, side))
        read_aligns, edge_seqs = {}, {}
        for edge_id in edges:
            if not os.path.isfile(read_align_path.format(it, side, edge_id)) or not os.path.isfile(consensuses[(it, side, edge_id)]):
                skip = True
            elif not skip:
                read_aligns[edge_id], edge_seqs[edge_id] = self._read_records(read_align_path.format(it, side, edge_id),
                                                                              consensuses[(it, side, edge_id)], device_text)
            if skip or not read_aligns or not read_aligns[edge_id] or not read_aligns[edge_id][0]:
                skip = True
        if skip:
            partitioning = self._read_partitioning_file(part_file.format(it - 1, side))
        else:
            partitioning, = self.classify_sam([(read_aligns, consensus_pos, headers_to_id, edge_seqs)])
        self._write_partitioning_file(partitioning, part_file.format(it, side))

    def _read_alignment(self, alignment, target_path, device_text=False):
        sam = SamAlignments(self.ctx, alignment, DivergenceFinder.read_fasta(target_path), self.max_read_coverage,
                            device_text=device_text)
        return [alns for _, alns in sam.chunks()]

    def partition_reads(self, edges, it, side, position_path, cons_align_path, template, read_align_path, consensuses,
                        confirmed_pos_path, part_file, headers_to_id, device_text=False):
        skip = False
        pos = self.read_positions(position_path)
        cons_aligns = {}
        for edge_id in edges:
            if not os.path.isfile(cons_align_path.format(it, side, edge_id)):
                skip = True
            else:
                cons_aligns[edge_id] = self._read_alignment(cons_align_path.format(it, side, edge_id), template, device_text)
            if skip or not cons_aligns or not cons_aligns[edge_id] or not cons_aligns[edge_id][0]:
                skip = True
        if skip:
            if it <= 1:
                confirmed, rejected = {k: [] for k in self.KEYS}, {k: [] for k in self.KEYS}
                consensus_pos = pos
            else:
                confirmed, rejected, consensus_pos = self._read_confirmed_positions(confirmed_pos_path.format(it - 1, side))
        else:
            coll = {edge_id: self._collapse_cons_aln(aln) for edge_id, aln in cons_aligns.items()}
            (confirmed, rejected, consensus_pos), = self.confirm([(pos, coll, side)])
        self._write_confirmed_positions(confirmed, rejected, pos, confirmed_pos_path.format(it, side))
        read_aligns = {}
        for edge_id in edges:
            if not os.path.isfile(read_align_path.format(it, side, edge_id)) or not os.path.isfile(consensuses[(it, side, edge_id)]):
                skip = True
            elif not skip:
                read_aligns[edge_id] = self._read_alignment(read_align_path.format(it, side, edge_id), consensuses[(it, side, edge_id)],
                                                               device_text)
            if skip or not read_aligns or not read_aligns[edge_id] or not read_aligns[edge_id][0]:
                skip = True
        if skip:
            partitioning = self._read_partitioning_file(part_file.format(it - 1, side))
        else:
            partitioning, = self.classify([(read_aligns, consensus_pos, headers_to_id)])
        self._write_partitioning_file(partitioning, part_file.format(it, side))


# the reference's Alignment tuple (flye/utils/sam_parser.py:44-48)
Alignment = collections.namedtuple("Alignment", ["qry_id", "trg_id", "qry_start", "qry_end", "qry_sign", "qry_len", "trg_start",
                                                 "trg_end", "trg_sign", "trg_len", "qry_seq", "trg_seq", "err_rate",
                                                 "is_secondary"])


# a record of SamAlignments(want_cols=False): the scalars of Alignment, then SAM POS, the CIGAR runs and the SEQ bytes
SamRecord = collections.namedtuple("SamRecord", ["qry_id", "trg_id", "qry_start", "qry_end", "qry_sign", "qry_len", "trg_start",
                                                 "trg_end", "trg_sign", "trg_len", "err_rate", "is_secondary", "ctg_pos", "ops",
                                                 "lens", "seq"])


class SamAlignments:
    """Mirror of the reference's SynchronizedSamReader (flye/utils/sam_parser.py:123-404) on fg_expand_cigars: the whole
    SAM file (plain or .gz) is read at once, tokenised on the host (CIGARs through fg_cigar_parse) and every record that
    get_chunk would parse goes into ONE device call.  contigs maps contig id to sequence (str or bytes), as the
    reference's reference_fasta.  max_coverage = None makes no cut (the reference compares with None there, which
    Python 3 refuses).  Raises ValueError where the reference raises AlignmentException("Alignment file is not sorted").
    want_cols=False expands without columns (err_rate and the scalars only) and keeps, per record, a SamRecord with the
    runs and the SEQ bytes where want_cols=True builds an Alignment with the two gapped strings: what
    ContigConsensus.consensus_sam and BubbleMaker.make_sam / polish_sam hand to the fused device calls.
    device_text=True tokenises on the device instead: the file's bytes make ONE fg_sam_parse, and the chunks, the
    filters, the cut, the runs and the SEQ bytes come from its arrays; what stays in Python is the unsorted test over the
    chunk names, the seeded shuffle (a permutation of the chunk's record count), int() on a FLAG or POS the device could
    not read, and the loop of the cut.  Records, order and exceptions are those of the host tokeniser.  The default stays
    False: a stand-in context without a device (one that restates expand_cigars alone) still serves the host tokeniser."""

    HEADERS = (b"@PG", b"@HD", b"@SQ", b"@RG", b"@CO")

    def __init__(self, ctx, sam_path, contigs, max_coverage=None, use_secondary=False, want_cols=True, device_text=False):
        self.ctx = ctx
        self.max_coverage, self.use_secondary, self.want_cols = max_coverage, use_secondary, bool(want_cols)
        as_bytes = lambda x: x if isinstance(x, bytes) else x.encode("latin-1")
        self.contigs = {as_bytes(h): as_bytes(s) for h, s in contigs.items()}
        opener = gzip.open if sam_path.endswith(".gz") else open
        with opener(sam_path, "rb") as f:
            if device_text:
                self._chunks = self._finish(*self._select_device(f.read()))
            else:
                self._chunks = self._parse(self._file_chunks(f))

    @classmethod
    def _file_chunks(cls, lines):
        """_read_file_chunk (:168-213) until the end of the file: [(contig, [line])] in file order"""
        out, processed, current = [], set(), None
        for line in lines:
            if line[:3] in cls.HEADERS:
                continue
            tab_1 = line.find(b"\t")
            tab_2 = line.find(b"\t", tab_1 + 1)
            tab_3 = line.find(b"\t", tab_2 + 1)
            if tab_2 == -1 or tab_3 == -1:
                continue
            contig = line[tab_2 + 1:tab_3]
            if contig in processed:
                raise ValueError("Alignment file is not sorted")
            if contig != current:
                if current is not None:
                    processed.add(current)
                current = contig
                out.append((contig, []))
            out[-1][1].append(line)
        return out

    @staticmethod
    def _span(ops, lens):
        """(qry_start, qry_end) of _parse_cigar (:316-320) from the runs alone"""
        lens = lens.astype(np.int64)
        is_h, is_s = ops == ord("H"), ops == ord("S")
        qry_pos = int(lens[(ops == ord("M")) | (ops == ord("I")) | is_s].sum())
        hard_left = int(lens[0]) if len(ops) and is_h[0] else 0
        other = np.flatnonzero(~is_h)
        soft_left = int(lens[other[0]]) if len(other) and is_s[other[0]] else 0
        return hard_left + soft_left, qry_pos + hard_left - (int(lens[is_s].sum()) - soft_left)

    def _parse(self, file_chunks):
        """get_chunk (:325-404) for every chunk; the records that survive its filters and its cut go to the device"""
        kept = []                                   # per chunk: [(tokens, flags, ops, lens)]
        for contig, lines in file_chunks:
            lines = list(lines)
            random.Random(42).shuffle(lines)
            sequence_length, recs = 0, []
            for line in lines:
                tokens = line.strip().split()
                if len(tokens) < 11:
                    continue
                flags = int(tokens[1])
                if flags & 0x4:
                    continue
                if flags & 0x100 and not self.use_secondary:
                    continue
                if tokens[9] == b"*":
                    raise Exception("Error parsing SAM: record without read sequence")
                ops, lens = cigar_parse(tokens[5])
                recs.append((tokens, flags, ops, lens))
                qry_start, qry_end = self._span(ops, lens)
                sequence_length += qry_end - qry_start
                contig_length = len(self.contigs[contig])
                if self.max_coverage is not None and sequence_length // contig_length > self.max_coverage:
                    break
            kept.append(recs)
        return self._finish([contig for contig, _ in file_chunks], kept)

    @staticmethod
    def _gather(arrays, off, length, sel):
        """(offsets, [pieces of each array side by side]): the pieces off[i] .. off[i] + length[i], i in sel"""
        a, n = off[sel].astype(np.int64), length[sel].astype(np.int64)
        cuts = list(zip(a.tolist(), (a + n).tolist()))
        return np.concatenate([np.zeros(1, np.int64), np.cumsum(n)]), \
            [np.concatenate([x[lo:hi] for lo, hi in cuts]) if cuts else np.zeros(0, x.dtype) for x in arrays]

    def _select_device(self, data):
        """_file_chunks and the selection of _parse from the arrays of ONE fg_sam_parse -> (chunk names, kept, text)"""
        t = self.ctx.sam_parse(data)
        off = t.chunk_off.astype(np.int64).tolist()
        names = [t.token(off[c], "tab_rname") for c in range(t.n_chunks)]
        seen = set()
        for name in names:                          # neighbours differ, so "processed" is every chunk name before
            if name in seen:
                raise ValueError("Alignment file is not sorted")
            seen.add(name)
        status, flag, pos = t.status.tolist(), t.flag.tolist(), t.pos.tolist()
        span = (t.qry_end - t.qry_start).tolist()
        kept = []
        for c, contig in enumerate(names):
            order = list(range(off[c], off[c + 1]))
            random.Random(42).shuffle(order)
            sequence_length, recs = 0, []
            for i in order:
                st = status[i]
                if st & t.FEW_TOKENS:
                    continue
                flags = int(t.token(i, "line").split()[1]) if st & t.BAD_FLAG else flag[i]
                if flags & 0x4:
                    continue
                if flags & 0x100 and not self.use_secondary:
                    continue
                if st & t.NO_SEQ:
                    raise Exception("Error parsing SAM: record without read sequence")
                if st & t.RUN_OVERFLOW:
                    cigar_parse(t.token(i, "cigar"))            # raises what the host tokeniser raises here
                ops, lens = t.runs(i)
                tokens = {0: t.token(i, "qname"), 2: t.token(i, "rname"), 3: t.token(i, "line").split()[3] if st & t.BAD_POS else pos[i],
                          9: None if self.want_cols else t.token(i, "seq"), "record": i}
                recs.append((tokens, flags, ops, lens))
                sequence_length += span[i]
                contig_length = len(self.contigs[contig])
                if self.max_coverage is not None and sequence_length // contig_length > self.max_coverage:
                    break
            kept.append(recs)
        return names, kept, t

    def _finish(self, names, kept, text=None):
        """the kept records of every chunk through ONE fg_expand_cigars; text: the SamTextResult they index (their runs and
        SEQ bytes are gathered from its arrays), None: they carry both"""
        flat = [r for recs in kept for r in recs]
        used = []
        for tokens, _, _, _ in flat:
            if tokens[2] not in used:
                used.append(tokens[2])
        number = {h: i for i, h in enumerate(used)}
        if text is None:
            runs_and_reads = lambda: (np.cumsum([0] + [len(r[2]) for r in flat]),
                                      np.concatenate([r[2] for r in flat]) if flat else np.zeros(0, np.uint8),
                                      np.concatenate([r[3] for r in flat]) if flat else np.zeros(0, np.uint32),
                                      np.cumsum([0] + [len(r[0][9]) for r in flat]), b"".join(r[0][9] for r in flat))
        else:
            def runs_and_reads():
                sel = np.array([r[0]["record"] for r in flat], np.int64)
                run_off, (run_op, run_len) = self._gather((text.run_op, text.run_len), text.run_off[:-1],
                                                          np.diff(text.run_off.astype(np.int64)), sel)
                read_off, (read_seq,) = self._gather((text.text,), text.seq_off, text.seq_len, sel)
                return run_off, run_op, run_len, read_off, read_seq
        res = self.ctx.expand_cigars(
            np.cumsum([0] + [len(self.contigs[h]) for h in used]), b"".join(self.contigs[h] for h in used),
            [number[r[0][2]] for r in flat], [int(r[0][3]) for r in flat], *runs_and_reads(), want_cols=self.want_cols)
        self.result = res
        out, a = [], 0
        for contig, recs in zip(names, kept):
            alns = []
            for tokens, flags, ops, lens in recs:
                if not self.want_cols:
                    alns.append(SamRecord(tokens[0].decode(), tokens[2].decode(), int(res.qry_start[a]), int(res.qry_end[a]),
                                          "-" if flags & 0x16 else "+", int(res.qry_len[a]), int(res.trg_start[a]),
                                          int(res.trg_end[a]), "+", len(self.contigs[tokens[2]]), float(res.err_rate[a]),
                                          flags & 0x100, int(tokens[3]), ops, lens, tokens[9]))
                    a += 1
                    continue
                trg, qry = res.columns(a)
                alns.append(Alignment(tokens[0].decode(), tokens[2].decode(), int(res.qry_start[a]), int(res.qry_end[a]),
                                      "-" if flags & 0x16 else "+", int(res.qry_len[a]), int(res.trg_start[a]),
                                      int(res.trg_end[a]), "+", len(self.contigs[tokens[2]]), qry.decode(), trg.decode(),
                                      float(res.err_rate[a]), flags & 0x100))
                a += 1
            alns.sort(key=lambda x: (x.qry_id, -(x.qry_end - x.qry_start)))
            out.append((contig.decode(), alns))
        return out

    def chunks(self):
        """[(contig id, [Alignment])] in file order: what successive get_chunk calls return (want_cols=False: SamRecord
        for Alignment, in the same order)"""
        return self._chunks

    def by_contig(self):
        """{contig id: [Alignment]}: what BubbleMaker.make and ContigConsensus.consensus take"""
        return dict(self._chunks)

    def flatten(self, contigs, keep=None):
        """the SamRecords of the given contigs (records with id), contig by contig, as the arguments the fused calls take:
        (records, dict(contig_off, contig_seq, contig_aln_off, ctg_pos, run_off, run_op, run_len, read_off, read_seq)).
        keep (one flag per record of these contigs, in this order) drops records."""
        if self.want_cols:
            raise ValueError("SamAlignments.flatten: made with want_cols=True, the records carry no runs")
        by = dict(self._chunks)
        lists = [by.get(c.id, []) for c in contigs]
        if keep is not None:
            flags, at = np.asarray(keep).astype(bool), 0
            for k, lst in enumerate(lists):
                lists[k] = [r for r, f in zip(lst, flags[at:at + len(lst)]) if f]
                at += len(lst)
        recs = [r for lst in lists for r in lst]
        seqs = [self.contigs[c.id.encode("latin-1")] for c in contigs]
        return recs, dict(
            contig_off=np.cumsum([0] + [len(x) for x in seqs]), contig_seq=b"".join(seqs),
            contig_aln_off=np.cumsum([0] + [len(lst) for lst in lists]), ctg_pos=[r.ctg_pos for r in recs],
            run_off=np.cumsum([0] + [len(r.ops) for r in recs]),
            run_op=np.concatenate([r.ops for r in recs]) if recs else np.zeros(0, np.uint8),
            run_len=np.concatenate([r.lens for r in recs]) if recs else np.zeros(0, np.uint32),
            read_off=np.cumsum([0] + [len(r.seq) for r in recs]), read_seq=b"".join(r.seq for r in recs))


class PlasmidFinder:
    """Mirror of the reference's short-plasmid rescue (flye/short_plasmids/unmapped_reads.py, circular_sequences.py,
    utils.py) with one device call per pass: a PAF file is read at once, tokenised by fg_paf_parse, and its hits go to
    fg_paf_groups (calc_mapping_rates, extract_unique_plasmids), fg_paf_circular (extract_circular_reads,
    extract_circular_pairs) and fg_components.  The divisions, round(.., 3), the thresholds, the greedy used_reads filter
    and the slices are Python, as in the reference.  Names are str, hits are PafHit records with the reference's fields."""

    PafHit = collections.namedtuple("PafHit", ["query", "query_length", "query_start", "query_end", "target", "target_length",
                                               "target_start", "target_end"])

    def __init__(self, ctx: Context):
        self.ctx = ctx

    @staticmethod
    def read_paf(path):
        opener = gzip.open if path.endswith(".gz") else open
        with opener(path, "rb") as f:
            return paf_parse(f.read())

    @classmethod
    def _hit(cls, paf, i):
        h = paf.hits[int(i)]
        return cls.PafHit(paf.name(h["query"]), int(h["query_len"]), int(h["query_start"]), int(h["query_end"]),
                          paf.name(h["target"]), int(h["target_len"]), int(h["target_start"]), int(h["target_end"]))

    @staticmethod
    def stream_sequence(path):
        """(header, sequence) as str for the records of a FASTA or FASTQ file, plain or .gz, by its suffix"""
        plain = path[:-3] if path.endswith(".gz") else path
        if plain.endswith((".fasta", ".fa")):
            for h, s in DivergenceFinder.read_fasta(path).items():
                yield h.decode(), s.decode()
        elif plain.endswith((".fastq", ".fq")):
            opener = gzip.open if path.endswith(".gz") else open
            with opener(path, "rb") as f:
                lines = [ln.strip() for ln in f if ln.strip()]
            for k in range(0, len(lines) - 3, 4):
                if not lines[k].startswith(b"@") or not lines[k + 2].startswith(b"+"):
                    raise ValueError("Fastq format error: " + path)
                yield lines[k][1:].split()[0].decode(), lines[k + 1].translate(DivergenceFinder.TO_ACGT).decode()
        else:
            raise ValueError("Unknown file extension: " + path)

    def calc_mapping_rates(self, paf_path):
        """{query: {target: rate}} of calc_mapping_rates (unmapped_reads.py:51-61)"""
        paf = paf_path if isinstance(paf_path, PafHits) else self.read_paf(paf_path)
        g = self.ctx.paf_groups(paf.hits)
        first = paf.hits[g["order"][g["group_off"][:-1].astype(np.int64)].astype(np.int64)]
        rates = collections.defaultdict(dict)
        for q, t, cover, length in zip(first["query"].tolist(), first["target"].tolist(), g["query_cover"].tolist(),
                                       first["query_len"].tolist()):
            rates[paf.name(q)][paf.name(t)] = round(cover / length, 3)
        return rates

    def extract_unmapped_reads(self, read_files, paf_path, unmapped_reads_path, mapping_rate_threshold):
        """extract_unmapped_reads (unmapped_reads.py:64-88); returns (total bases, unmapped bases)"""
        rates = self.calc_mapping_rates(paf_path)
        total = unmapped = 0
        with open(unmapped_reads_path, "w") as out:
            for path in read_files:
                for hdr, seq in self.stream_sequence(path):
                    total += len(seq)
                    contigs = rates.get(hdr)
                    if contigs is None or not any(r >= mapping_rate_threshold for r in contigs.values()):
                        unmapped += len(seq)
                        out.write(">{0}\n{1}\n".format(hdr, seq))
        return total, unmapped

    def extract_circular_reads(self, paf_path, max_overhang=150):
        """{read: PafHit} in the reference's dict order (circular_sequences.py:33-44)"""
        paf = paf_path if isinstance(paf_path, PafHits) else self.read_paf(paf_path)
        c = self.ctx.paf_circular(paf.hits, max_overhang, 300)
        return {paf.name(q): self._hit(paf, i) for q, i in zip(c["circ_query"].tolist(), c["circ_hit"].tolist())}

    def extract_circular_pairs(self, paf_path, max_overhang=300):
        """[[hit, hit]] of extract_circular_pairs (:82-118): the device finds every group's candidate, the greedy
        used_reads filter runs here over the groups in order"""
        paf = paf_path if isinstance(paf_path, PafHits) else self.read_paf(paf_path)
        c = self.ctx.paf_circular(paf.hits, 150, max_overhang)
        used, pairs = set(), []
        for k in np.flatnonzero(c["pair_ok"]).tolist():
            q, t = int(c["group_query"][k]), int(c["group_target"][k])
            if q in used or t in used:
                continue
            used.update((q, t))
            pairs.append([self._hit(paf, c["pair_first"][k]), self._hit(paf, c["pair_second"][k])])
        return pairs

    @staticmethod
    def trim_circular_reads(circular_reads, unmapped_reads):
        return {"circular_read_" + str(i): unmapped_reads[read][:hit.target_start].upper()
                for i, (read, hit) in enumerate(circular_reads.items())}

    @staticmethod
    def trim_circular_pairs(circular_pairs, unmapped_reads):
        return {"circular_pair_" + str(i): (unmapped_reads[p[0].query][p[1].query_end:p[0].query_end] +
                                            unmapped_reads[p[0].target][p[0].target_end:]).upper()
                for i, p in enumerate(circular_pairs)}

    def extract_unique_plasmids(self, paf_path, fasta_path, mapping_rate_threshold=0.8, max_length_difference=500,
                                min_sequence_length=1000, vertex_order=None):
        """extract_unique_plasmids (:121-191).  The reference numbers its vertices by list(set(names)), an order that
        changes from process to process, so the representative it reports for a group is arbitrary; here vertex_order
        (names) fixes it, by default the order of first appearance in the file, the query before the target of a line.
        max_length_difference is unused, as in the reference."""
        paf = paf_path if isinstance(paf_path, PafHits) else self.read_paf(paf_path)
        if vertex_order is None:
            vertex_order = [paf.name(i) for i in paf.first_seen.tolist()]
        number = {name: i for i, name in enumerate(vertex_order)}
        g = self.ctx.paf_groups(paf.hits)
        first = paf.hits[g["order"][g["group_off"][:-1].astype(np.int64)].astype(np.int64)]
        eu, ev = [], []
        for q, t, qc, tc, ql, tl in zip(first["query"].tolist(), first["target"].tolist(), g["query_cover"].tolist(),
                                        g["target_cover"].tolist(), first["query_len"].tolist(), first["target_len"].tolist()):
            if q != t and (round(qc / ql, 3) > mapping_rate_threshold or round(tc / tl, 3) > mapping_rate_threshold):
                eu.append(number[paf.name(q)])
                ev.append(number[paf.name(t)])
        labels = self.ctx.components(len(vertex_order), eu, ev)
        size = np.bincount(labels, minlength=len(vertex_order))
        seqs = dict(self.stream_sequence(fasta_path))
        unique = {}
        for v in np.flatnonzero(size > 1).tolist():     # a label is its component's smallest vertex: ascending, as the DFS numbers them
            seq = seqs[vertex_order[v]]
            if len(seq) >= min_sequence_length:
                unique[vertex_order[v]] = seq
        return unique
