"""Thin ctypes binding of libmargin_rphmm.so (the C-ABI in include/margin_rphmm.h).

This is plumbing for the tests and the benchmark: every call goes through the C-ABI exactly as a
C caller (margin's impl/hmm.c adaptor) would.  There is no Python or CPU
implementation of the sweep behind it -- if the library or a device is missing, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRP_LIB_OVERRIDE") or os.path.join(_HERE, "lib", "libmargin_rphmm.so")

MRP_OK = 0
MRP_ERR_ARG, MRP_ERR_NO_DEVICE, MRP_ERR_HIP, MRP_ERR_NOMEM, MRP_ERR_UNSUPPORTED, MRP_ERR_LOOKUP = 1, 2, 3, 4, 5, 6
WIDE_MAX_WIDTH, WIDE_MAX_CELLS = 32768, 1 << 31  # MRP_WIDE_MAX_WIDTH, MRP_WIDE_MAX_CELLS
FLAG_MAX_NOT_SUM = 1
FLAG_INCLUDE_ANCESTOR_SUB_PROB = 2

#: every symbol include/margin_rphmm.h declares (checked by the CPU test-suite)
ABI_VERSION = 6  # MRP_ABI_VERSION of include/margin_rphmm.h as transcribed here

EXPORTED_SYMBOLS = [
    "mrp_last_error", "mrp_version", "mrp_abi_version", "mrp_runtime_init", "mrp_device_count", "mrp_context_create", "mrp_context_destroy",
    "mrp_context_synchronize", "mrp_context_trim", "mrp_hmm_split", "mrp_hmm_split_where_phasing_is_uncertain", "mrp_context_set_phase_groups", "mrp_context_set_test_hooks", "mrp_context_launch_census", "mrp_launch_class_name", "mrp_set_host_threads", "mrp_chunk_create", "mrp_chunk_destroy", "mrp_fb_run", "mrp_batch_create",
    "mrp_batch_add", "mrp_batch_upload", "mrp_batch_launch", "mrp_batch_download", "mrp_batch_destroy",
    "mrp_batch_stats", "mrp_count_bit_vectors", "mrp_emissions", "mrp_get_rp_hmms", "mrp_hmm_destroy", "mrp_free",
    "mrp_hmm_view", "mrp_hmm_forward_backward", "mrp_hmm_prune", "mrp_hmm_forward_trace_back", "mrp_phase_reads",
    "mrp_phase_result_destroy", "mrp_get_rp_hmms_resident", "mrp_phase_reads_many", "mrp_reference_from_bubbles",
    "mrp_profile_seqs_from_bubbles", "mrp_assign_reads_to_haplotypes", "mrp_stitch_create", "mrp_stitch_destroy",
    "mrp_stitch_chunk", "mrp_stitch_size", "mrp_stitch_lookup", "mrp_phase_sets", "mrp_binomial_p_value", "mrp_binomial_coefficient",
    "mrp_symbols_from_chars", "mrp_pair_hmm_reverse_complement", "mrp_band_diagonals", "mrp_forward_probabilities",
    "mrp_allele_read_supports", "mrp_kmer_alignment_anchors", "mrp_phase_chunks_on_devices", "mrp_queue_plan", "mrp_queue_dry_run", "mrp_queue_create", "mrp_queue_destroy",
    "mrp_queue_phase_chunks", "mrp_partition_reads_by_haplotype", "mrp_phase_variants_from_tagged_reads", "mrp_phase_string_chunks",
    "mrp_extract_read_substrings", "mrp_string_chunk_from_extracted", "mrp_string_chunk_units", "mrp_queue_phase_string_chunks",
    "mrp_phase_string_chunks_on_devices", "mrp_phase_string_chunks_with_filtered", "mrp_queue_phase_string_chunks_with_filtered",
    "mrp_phase_string_chunks_with_filtered_on_devices", "mrp_haptag_sites_from_extracted", "mrp_haplotag_aligned_chunks",
    "mrp_kmer_alignment_anchors_many", "mrp_phase_aligned_chunks", "mrp_string_chunk_rest_from_extracted", "mrp_equal_substring_classes",
    "mrp_phase_aligned_chunks_with_filtered", "mrp_aligned_chunk_units", "mrp_queue_phase_aligned_chunks",
    "mrp_queue_phase_aligned_chunks_with_filtered", "mrp_phase_aligned_chunks_on_devices", "mrp_phase_aligned_chunks_with_filtered_on_devices",
    "mrp_haplotag_chunk_units", "mrp_queue_haplotag_aligned_chunks", "mrp_haplotag_aligned_chunks_on_devices",
    "mrp_context_set_wide_pairs", "mrp_context_wide_pair_count", "mrp_queue_set_wide_pairs", "mrp_queue_wide_pair_count", "mrp_pair_diagonal_width",
    "mrp_context_set_sv_split", "mrp_queue_set_sv_split", "mrp_mark_structural_variants",
    "mrp_variant_records_from_extracted", "mrp_phase_aligned_chunks_with_records", "mrp_variants_from_records",
    "mrp_context_set_downsampling", "mrp_queue_set_downsampling", "mrp_context_last_downsampling", "mrp_downsample_draw", "mrp_aln_read_lengths",
    "mrp_downsample_keep_from_extracted", "mrp_downsample_reads",
    "mrp_queue_phase_aligned_chunks_with_records", "mrp_phase_aligned_chunks_with_records_on_devices", "mrp_final_read_tags", "mrp_stitch_values",
    "mrp_close_contig", "mrp_close_contigs", "mrp_contig_out_clear",
    "mrp_posterior_tracebacks", "mrp_posterior_aligned_pairs", "mrp_posterior_pairs_free", "mrp_context_set_posterior_workspace",
    "mrp_context_last_posterior",
    "mrp_band_diagonals_dynamic", "mrp_pair_diagonal_width_dynamic", "mrp_posterior_tracebacks_dynamic", "mrp_posterior_aligned_pairs_dynamic",
    "mrp_context_set_posterior_wide_pairs", "mrp_context_posterior_wide_count",
    "mrp_rle_compress", "mrp_forward_probabilities_rle", "mrp_posterior_aligned_pairs_rle",
    "mrp_context_set_rle_lane_pairs", "mrp_rle_lane_caps", "mrp_allele_read_supports_rle",
    "mrp_ml_repeat_counts", "mrp_rle_expand",
    "mrp_poa_augment", "mrp_poa_free", "mrp_poa_consensus",
]


class MrpError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mrp error {code}: {msg}")
        self.code = code


class HmmJob(C.Structure):
    _fields_ = [("chunk", C.c_void_p), ("n_columns", C.c_int32), ("flags", C.c_uint32),
                ("col_ref_start", C.c_void_p), ("col_length", C.c_void_p), ("col_depth", C.c_void_p),
                ("col_cell_off", C.c_void_p), ("col_read_off", C.c_void_p), ("read_byte_off", C.c_void_p),
                ("partition", C.c_void_p), ("mask_from", C.c_void_p), ("mask_to", C.c_void_p),
                ("mcol_cell_off", C.c_void_p), ("merge_from", C.c_void_p), ("merge_to", C.c_void_p),
                ("cell_next", C.c_void_p), ("cell_prev", C.c_void_p),
                ("cell_forward", C.c_void_p), ("cell_backward", C.c_void_p), ("merge_forward", C.c_void_p),
                ("merge_backward", C.c_void_p), ("col_total", C.c_void_p), ("hmm_forward", C.c_void_p),
                ("hmm_backward", C.c_void_p)]


class LaunchStats(C.Structure):
    _fields_ = [("planes_ms", C.c_double), ("emission_ms", C.c_double), ("sweep_ms", C.c_double), ("n_hmms", C.c_int64),
                ("n_columns", C.c_int64), ("n_cells", C.c_int64), ("n_merge_cells", C.c_int64),
                ("profile_bytes", C.c_int64), ("algorithmic_bytes", C.c_int64), ("popcount_ops", C.c_int64),
                ("units", C.c_int64), ("avg_planes_ms", C.c_double), ("avg_emission_ms", C.c_double), ("avg_sweep_ms", C.c_double),
                ("launches_averaged", C.c_int64), ("n_hmms_int32", C.c_int64), ("n_hmms_lse", C.c_int64), ("n_hmms_generic", C.c_int64)]


class Params(C.Structure):
    """mrp_params (mirror of the stRPHmmParameters fields the L1 code reads)."""
    _fields_ = [("max_not_sum_transitions", C.c_int32), ("include_inverted_partitions", C.c_int32),
                ("include_ancestor_sub_prob", C.c_int32), ("reserved", C.c_int32),
                ("min_partitions_in_a_column", C.c_int64), ("max_partitions_in_a_column", C.c_int64),
                ("min_posterior_probability_for_partition", C.c_double), ("max_coverage_depth", C.c_int64),
                ("min_read_coverage_to_support_phasing_between_heterozygous_sites", C.c_int64),
                ("rounds_of_iterative_refinement", C.c_int64)]

    @classmethod
    def from_reference_names(cls, d: dict) -> "Params":
        """Build from a dict keyed by the reference's parameter names (params/base_params.json)."""
        p = cls()
        p.max_not_sum_transitions = int(d["maxNotSumTransitions"])
        p.include_inverted_partitions = int(d["includeInvertedPartitions"])
        p.include_ancestor_sub_prob = int(d.get("includeAncestorSubProb", 1))
        p.min_partitions_in_a_column = int(d["minPartitionsInAColumn"])
        p.max_partitions_in_a_column = int(d["maxPartitionsInAColumn"])
        p.min_posterior_probability_for_partition = float(d["minPosteriorProbabilityForPartition"])
        p.max_coverage_depth = int(d["maxCoverageDepth"])
        p.min_read_coverage_to_support_phasing_between_heterozygous_sites = int(
            d.get("minReadCoverageToSupportPhasingBetweenHeterozygousSites", 0))
        p.rounds_of_iterative_refinement = int(d.get("roundsOfIterativeRefinement", 0))
        return p


class ReadRec(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ref_start", C.c_int32), ("length", C.c_int32),
                ("forward_strand", C.c_int32), ("reserved", C.c_int32), ("pool_offset", C.c_int64)]


class PhaseResult(C.Structure):
    _fields_ = [("ref_start", C.c_int32), ("length", C.c_int32),
                ("genotype_string", C.POINTER(C.c_uint64)), ("haplotype_string1", C.POINTER(C.c_uint64)),
                ("haplotype_string2", C.POINTER(C.c_uint64)), ("ancestor_string", C.POINTER(C.c_uint64)),
                ("reads_supporting_haplotype1", C.POINTER(C.c_uint64)),
                ("reads_supporting_haplotype2", C.POINTER(C.c_uint64)),
                ("genotype_probs", C.POINTER(C.c_float)), ("haplotype_probs1", C.POINTER(C.c_float)),
                ("haplotype_probs2", C.POINTER(C.c_float)),
                ("reads1", C.POINTER(C.c_int32)), ("reads2", C.POINTER(C.c_int32)),
                ("n_reads1", C.c_int64), ("n_reads2", C.c_int64),
                ("hmm_forward", C.c_double), ("hmm_backward", C.c_double), ("n_sweeps", C.c_int64)]


class PhaseManyStats(C.Structure):
    _fields_ = [("resident", C.c_int32), ("fallback_chunks", C.c_int32), ("levels", C.c_int64), ("hmms", C.c_int64),
                ("columns", C.c_int64), ("cells", C.c_int64), ("merge_cells", C.c_int64), ("device_ms", C.c_double),
                ("cross_ms", C.c_double), ("sweep_ms", C.c_double), ("prune_ms", C.c_double), ("note", C.c_char * 160),
                ("pack_ms", C.c_double), ("cross_emit_ms", C.c_double), ("recursion_ms", C.c_double), ("prune_kernel_ms", C.c_double),
                ("compact_ms", C.c_double)]


MAX_QUEUE_DEVICES = 16


class ChunkDesc(C.Structure):
    _fields_ = [("n_sites", C.c_int64), ("allele_number", C.c_void_p), ("substitution_log_probs", C.c_void_p),
                ("allele_prior_log_probs", C.c_void_p), ("profile_pool", C.c_void_p), ("pool_bytes", C.c_int64),
                ("reads", C.POINTER(ReadRec)), ("n_reads", C.c_int64)]


class QueueStats(C.Structure):
    _fields_ = [("n_devices", C.c_int32), ("reserved", C.c_int32), ("batches", C.c_int64), ("fallback_chunks", C.c_int64),
                ("chunks_per_device", C.c_int64 * MAX_QUEUE_DEVICES), ("units_per_device", C.c_int64 * MAX_QUEUE_DEVICES),
                ("busy_ms_per_device", C.c_double * MAX_QUEUE_DEVICES)]


class Bubbles(C.Structure):
    _fields_ = [("n_bubbles", C.c_int64), ("allele_number", C.c_void_p), ("read_off", C.c_void_p), ("reads", C.c_void_p),
                ("support_off", C.c_void_p), ("allele_read_supports", C.c_void_p)]


class Variant(C.Structure):
    _fields_ = [("pos", C.c_int32), ("gt1", C.c_int32), ("gt2", C.c_int32), ("n_alleles", C.c_int32),
                ("allele_read_off", C.c_void_p), ("allele_reads", C.c_void_p)]


_lib = None


class PairHmm(C.Structure):
    """mrp_pair_hmm: struct _StateMachine3 (impl/stateMachine.c:507-519) + NucleotideEmissions, log space."""
    _TRANSITIONS = ("match_continue", "match_from_gap_x", "match_from_gap_y", "gap_open_x", "gap_open_y", "gap_extend_x", "gap_extend_y",
                    "gap_switch_to_x", "gap_switch_to_y")
    _fields_ = [(n, C.c_double) for n in _TRANSITIONS] + [("e_match", C.c_double * 16), ("e_gap_x", C.c_double * 4), ("e_gap_y", C.c_double * 4)]

    @classmethod
    def default_nucleotide(cls) -> "PairHmm":
        """stateMachine3_constructNucleotide (impl/stateMachine.c:612-644, :409-432): the literals of the reference."""
        m = cls(-0.030064059121770816, -1.272871422049609, -1.272871422049609, -4.21256642, -4.21256642, -0.3388262689231553,
                -0.3388262689231553, -4.910694825551255, -4.910694825551255)
        ma, tv, ti = -1.8917761142, -4.3459578861, -3.760242452
        m.e_match[:] = [ma, tv, ti, tv, tv, ma, tv, ti, ti, tv, ma, tv, tv, ti, tv, ma]
        m.e_gap_x[:] = [-1.3862943611] * 4
        m.e_gap_y[:] = [-1.3862943611] * 4
        return m

    @classmethod
    def from_margin_hmm(cls, hmm_type: int, transitions, emissions) -> "PairHmm":
        """hmm_getStateMachine (impl/stateMachine.c:690-703) for the "type" / "transitions" / "emissions" arrays of a margin
        parameter file: type 2 = threeState (symmetric, :663-682), 3 = threeStateAsymmetric (:646-661); emissions =
        16 match + 4 gap-x + 4 gap-y probabilities (:481-488).  log(0) = -inf, as in C."""
        t = np.asarray(transitions, dtype=np.float64).reshape(3, 3)
        e = np.asarray(emissions, dtype=np.float64)
        assert hmm_type in (2, 3) and e.shape == (24,)
        M, X, Y = 0, 1, 2
        with np.errstate(divide="ignore"):
            lg = lambda v: float(np.log(np.float64(v)))
            if hmm_type == 3:
                vals = [lg(t[M, M]), lg(t[X, M]), lg(t[Y, M]), lg(t[M, X]), lg(t[M, Y]), lg(t[X, X]), lg(t[Y, Y]), lg(t[Y, X]), lg(t[X, Y])]
            else:
                fg, go, ge, gs = lg((t[X, M] + t[Y, M]) / 2.0), lg((t[M, X] + t[M, Y]) / 2.0), lg((t[X, X] + t[Y, Y]) / 2.0), lg((t[Y, X] + t[X, Y]) / 2.0)
                vals = [lg(t[M, M]), fg, fg, go, go, ge, ge, gs, gs]
            m = cls(*vals)
            m.e_match[:] = [lg(v) for v in e[:16]]
            m.e_gap_x[:] = [lg(v) for v in e[16:20]]
            m.e_gap_y[:] = [lg(v) for v in e[20:24]]
        return m

    def copy(self) -> "PairHmm":
        m = PairHmm()
        C.memmove(C.byref(m), C.byref(self), C.sizeof(PairHmm))
        return m

    def reverse_complement(self) -> "PairHmm":
        """the state machine of reverse strand reads (impl/parser.c:356-358)"""
        m = self.copy()
        load().mrp_pair_hmm_reverse_complement(C.byref(m))
        return m


class PairHmmStats(C.Structure):
    _fields_ = [("pairs_lane", C.c_int64), ("pairs_wave", C.c_int64), ("cells", C.c_int64), ("kernel_ms", C.c_double), ("total_ms", C.c_double)]


POSTERIOR_DEFAULT_WORKSPACE = 1 << 30  # MRP_POSTERIOR_DEFAULT_WORKSPACE


class PosteriorOptions(C.Structure):
    """mrp_posterior_options; the defaults are pairwiseAlignmentBandingParameters_construct's (impl/pairwiseAligner.c:1048-1060)"""
    _fields_ = [("threshold", C.c_double), ("expansion", C.c_int64), ("min_diags_between_traceback", C.c_int64), ("traceback_diagonals", C.c_int64),
                ("ragged_left", C.c_int32), ("ragged_right", C.c_int32), ("with_gaps", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, threshold=0.01, expansion=20, min_diags_between_traceback=1000, traceback_diagonals=40, ragged_left=False, ragged_right=False,
                 with_gaps=False, reserved=0):
        super().__init__(float(threshold), int(expansion), int(min_diags_between_traceback), int(traceback_diagonals), int(ragged_left), int(ragged_right),
                         int(with_gaps), int(reserved))


class PosteriorPairs(C.Structure):
    """mrp_posterior_pairs: pair i owns [first[i], first[i + 1])"""
    _fields_ = [("first", C.POINTER(C.c_int64)), ("x", C.POINTER(C.c_int32)), ("y", C.POINTER(C.c_int32)), ("weight", C.POINTER(C.c_int32)),
                ("log_posterior", C.POINTER(C.c_double))]

    def to_numpy(self, n_pairs: int) -> dict:
        first = np.ctypeslib.as_array(self.first, shape=(n_pairs + 1,)).copy()
        n = int(first[-1])
        take = lambda p, dt: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=dt)
        return {"first": first, "x": take(self.x, np.int32), "y": take(self.y, np.int32), "weight": take(self.weight, np.int32),
                "log_posterior": take(self.log_posterior, np.float64)}


class RepeatModelStruct(C.Structure):
    """mrp_repeat_model"""
    _fields_ = [("max_repeat", C.c_int32), ("strand", C.c_int32), ("log_prob", C.POINTER(C.c_double))]


class RepeatModel:
    """The run-length emissions of one model: log_prob float64 [4, R, R] (base A..T, underlying count, observed count:
    RepeatSubMatrix.logProbabilities), strand 1 or 0 (RleNucleotideEmissions.strand).  Nothing is checked here: the entries do."""

    def __init__(self, log_prob, strand=1, max_repeat=None):
        self.log_prob = None if log_prob is None else np.ascontiguousarray(log_prob, dtype=np.float64)
        self.max_repeat = int(max_repeat if max_repeat is not None else self.log_prob.shape[-1])
        self.strand = int(strand)

    def struct(self) -> RepeatModelStruct:
        return RepeatModelStruct(self.max_repeat, self.strand, None if self.log_prob is None else self.log_prob.ctypes.data_as(C.POINTER(C.c_double)))


class RepeatCountOptions(C.Structure):
    """mrp_repeat_count_options"""
    _fields_ = [("walk_backwards", C.c_int32), ("reserved", C.c_int32), ("log_het_substitution", C.c_double), ("reserved2", C.c_int64)]


class RepeatCountStats(C.Structure):
    """mrp_repeat_count_stats"""
    _fields_ = [("observations", C.c_int64), ("nodes_observed", C.c_int64), ("candidates", C.c_int64), ("upload_ms", C.c_double),
                ("ordering_ms", C.c_double), ("estimate_ms", C.c_double), ("total_ms", C.c_double), ("bytes_uploaded", C.c_int64),
                ("bytes_downloaded", C.c_int64)]


class PoaOptions(C.Structure):
    """mrp_poa_options"""
    _fields_ = [("compare_repeat_counts", C.c_int32), ("merge_ends", C.c_int32), ("reference_base_penalty", C.c_double),
                ("want_repeat_count_weight", C.c_int32), ("reserved", C.c_int32), ("reserved2", C.c_int64)]


class Poa(C.Structure):
    """mrp_poa"""
    _fields_ = [("n_nodes", C.c_int64), ("n_consensus", C.c_int64), ("max_repeat", C.c_int32), ("pad", C.c_int32),
                ("base_weight", C.POINTER(C.c_double)), ("repeat_count_weight", C.POINTER(C.c_double)), ("base_pick", C.POINTER(C.c_int32)),
                ("repeat_count_pick", C.POINTER(C.c_int32)), ("insert_first", C.POINTER(C.c_int64)), ("n_inserts", C.c_int64),
                ("insert_str_off", C.POINTER(C.c_int64)), ("insert_str_len", C.POINTER(C.c_int32)), ("insert_weight_forward", C.POINTER(C.c_double)),
                ("insert_weight_reverse", C.POINTER(C.c_double)), ("insert_n_observations", C.POINTER(C.c_int64)), ("pool_len", C.c_int64),
                ("pool_symbols", C.POINTER(C.c_uint8)), ("pool_counts", C.POINTER(C.c_int32)), ("delete_first", C.POINTER(C.c_int64)),
                ("n_deletes", C.c_int64), ("delete_length", C.POINTER(C.c_int32)), ("delete_weight_forward", C.POINTER(C.c_double)),
                ("delete_weight_reverse", C.POINTER(C.c_double)), ("delete_n_observations", C.POINTER(C.c_int64)), ("totals", C.POINTER(C.c_double))]


class PoaStats(C.Structure):
    """mrp_poa_stats"""
    _fields_ = [(k, C.c_int64) for k in ("matches", "deletes", "inserts", "complete_inserts", "complete_deletes", "distinct_inserts", "distinct_deletes",
                                         "longest_run", "table_slots", "bytes_uploaded", "bytes_downloaded")] + \
               [(k, C.c_double) for k in ("upload_ms", "sets_ms", "enumerate_ms", "group_ms", "picks_ms", "check_ms", "total_ms")]


class PosteriorStats(C.Structure):
    _fields_ = [("forward_ms", C.c_double), ("traceback_ms", C.c_double), ("total_ms", C.c_double), ("cells", C.c_int64), ("traceback_cells", C.c_int64),
                ("candidates", C.c_int64), ("downloaded_bytes", C.c_int64), ("groups", C.c_int64)]


class HaptagSites(C.Structure):
    _fields_ = [("n_sites", C.c_int64), ("pool", C.c_void_p), ("pool_bytes", C.c_int64), ("allele_first", C.c_void_p), ("allele_off", C.c_void_p),
                ("allele_len", C.c_void_p), ("compare", C.c_void_p), ("entry_first", C.c_void_p), ("entry_read", C.c_void_p),
                ("entry_off", C.c_void_p), ("entry_len", C.c_void_p)]


VARIANT_NOT_VISITED, VARIANT_CIS, VARIANT_TRANS, VARIANT_TIE = 0, 1, 2, 3


class StringChunk(C.Structure):
    _fields_ = [("n_bubbles", C.c_int64), ("n_reads", C.c_int64), ("pool", C.c_void_p), ("pool_bytes", C.c_int64), ("allele_first", C.c_void_p),
                ("allele_off", C.c_void_p), ("allele_len", C.c_void_p), ("sub_first", C.c_void_p), ("sub_off", C.c_void_p), ("sub_len", C.c_void_p),
                ("sub_read", C.c_void_p), ("read_names", C.c_void_p), ("read_forward_strand", C.c_void_p)]


class ProfileOut(C.Structure):
    _fields_ = [("seqs", C.POINTER(ReadRec)), ("read_of_seq", C.c_void_p), ("n_seqs", C.c_int64), ("pool", C.c_void_p), ("pool_bytes", C.c_int64),
                ("allele_number", C.c_void_p), ("substitution", C.c_void_p), ("prior", C.c_void_p)]


class StringChunksStats(C.Structure):
    _fields_ = [("pairhmm", PairHmmStats), ("phase", PhaseManyStats), ("profile_ms", C.c_double), ("assign_ms", C.c_double),
                ("host_ms", C.c_double), ("total_ms", C.c_double)]


class StringChunkRest(C.Structure):
    _fields_ = [("n_filtered", C.c_int64), ("forward_strand", C.c_void_p), ("pool", C.c_void_p), ("pool_bytes", C.c_int64), ("fsub_first", C.c_void_p),
                ("fsub_off", C.c_void_p), ("fsub_len", C.c_void_p), ("fsub_read", C.c_void_p), ("n_variants", C.c_int64), ("valle_first", C.c_void_p),
                ("valle_off", C.c_void_p), ("valle_len", C.c_void_p), ("gt", C.c_void_p), ("ventry_first", C.c_void_p), ("ventry_read", C.c_void_p),
                ("ventry_off", C.c_void_p), ("ventry_len", C.c_void_p)]


class FilteredOut(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("read_hap", C.c_void_p), ("h1", C.c_void_p), ("h2", C.c_void_p), ("n_variants", C.c_int64),
                ("variant_state", C.c_void_p), ("cis", C.c_void_p), ("trans", C.c_void_p)]


class StringFilteredStats(C.Structure):
    _fields_ = [("chunks", StringChunksStats), ("pairs_scored", C.c_int64), ("pairs_speculative", C.c_int64), ("pairs_read_by_results", C.c_int64),
                ("filtered_ms", C.c_double)]


READ_DROPPED, READ_KEPT, READ_FILTERED = 0, 1, 2


class AlignedChunk(C.Structure):
    _fields_ = [("overlap_start", C.c_int64), ("overlap_end", C.c_int64), ("chunk_start", C.c_int64), ("chunk_end", C.c_int64),
                ("reference", C.c_void_p), ("reference_len", C.c_int64), ("n_variants", C.c_int64), ("variant_pos", C.c_void_p),
                ("allele_first", C.c_void_p), ("allele_off", C.c_void_p), ("allele_len", C.c_void_p), ("allele_chars", C.c_void_p),
                ("allele_bytes", C.c_int64), ("is_sv", C.c_void_p), ("n_reads", C.c_int64), ("pos", C.c_void_p), ("flag", C.c_void_p),
                ("mapq", C.c_void_p), ("l_qseq", C.c_void_p), ("cigar_first", C.c_void_p), ("cigar", C.c_void_p), ("seq_first", C.c_void_p),
                ("seq", C.c_void_p)]


class ExtractOptions(C.Structure):
    _fields_ = [("expansion_small", C.c_int64), ("expansion_sv", C.c_int64), ("min_mapq", C.c_int64), ("include_secondary", C.c_int32),
                ("include_supplementary", C.c_int32), ("indel_size_for_sv_handling", C.c_int32), ("use_run_length_encoding", C.c_int32)]

    @classmethod
    def from_dict(cls, d: dict) -> "ExtractOptions":
        return cls(int(d["expansion_small"]), int(d["expansion_sv"]), int(d["min_mapq"]), int(d["include_secondary"]),
                   int(d["include_supplementary"]), int(d.get("indel_size_for_sv_handling", 0)), int(d.get("use_run_length_encoding", 0)))


def shipped_extract_options() -> dict:
    """params/base_params.json: referenceExpansionForSmallVariants 12, ...StructuralVariants 512, filterAlignmentsWithMapQBelowThisThreshold
    5, includeSecondaryAlignments / includeSupplementaryAlignments false"""
    return dict(expansion_small=12, expansion_sv=512, min_mapq=5, include_secondary=0, include_supplementary=0)


class ExtractedChunk(C.Structure):
    _fields_ = [("n_variants", C.c_int64), ("n_reads", C.c_int64), ("ref_aln_start", C.c_void_p), ("ref_aln_stop_incl", C.c_void_p),
                ("allele_first", C.c_void_p), ("allele_off", C.c_void_p), ("allele_len", C.c_void_p), ("read_status", C.c_void_p),
                ("read_n_substrings", C.c_void_p), ("entry_first", C.c_void_p), ("entry_read", C.c_void_p), ("entry_off", C.c_void_p),
                ("entry_len", C.c_void_p), ("pool", C.c_void_p), ("pool_bytes", C.c_int64)]


class ExtractStats(C.Structure):
    _fields_ = [("reads", C.c_int64), ("cigar_ops", C.c_int64), ("aligned_bases", C.c_int64), ("entries", C.c_int64), ("kernel_ms", C.c_double),
                ("bytes_uploaded", C.c_int64), ("host_ms", C.c_double), ("total_ms", C.c_double)]


class DownsamplingStats(C.Structure):
    _fields_ = [("chunks", C.c_int64), ("chunks_downsampled", C.c_int64), ("reads_discarded", C.c_int64), ("bytes_downloaded", C.c_int64),
                ("downsample_ms", C.c_double)]


class HaplotagAlignedStats(C.Structure):
    _fields_ = [("extract", ExtractStats), ("pairhmm", PairHmmStats), ("sites", C.c_int64), ("active_sites", C.c_int64), ("entries", C.c_int64),
                ("owners", C.c_int64), ("bytes_downloaded", C.c_int64), ("owners_ms", C.c_double), ("total_ms", C.c_double)]


class PhaseAlignedStats(C.Structure):
    _fields_ = [("extract", ExtractStats), ("chunks", StringChunksStats), ("variants", C.c_int64), ("bubbles", C.c_int64), ("entries", C.c_int64),
                ("entries_used", C.c_int64), ("owners", C.c_int64), ("pairs", C.c_int64), ("pairs_anchored", C.c_int64), ("anchors", C.c_int64),
                ("anchor_runs", C.c_int64), ("front_bytes_downloaded", C.c_int64), ("owners_ms", C.c_double), ("anchors_ms", C.c_double), ("total_ms", C.c_double)]


class AlignedChunkRest(C.Structure):
    _fields_ = [("n_variants", C.c_int64), ("variant_pos", C.c_void_p), ("allele_first", C.c_void_p), ("allele_off", C.c_void_p),
                ("allele_len", C.c_void_p), ("allele_chars", C.c_void_p), ("allele_bytes", C.c_int64), ("is_sv", C.c_void_p), ("gt", C.c_void_p)]


class PhaseAlignedFilteredStats(C.Structure):
    _fields_ = [("aligned", PhaseAlignedStats), ("filtered_variants", C.c_int64), ("filtered_reads", C.c_int64), ("filtered_entries", C.c_int64),
                ("pairs_scored", C.c_int64), ("pairs_speculative", C.c_int64), ("pairs_read_by_results", C.c_int64), ("filtered_ms", C.c_double),
                ("classes_ms", C.c_double)]


RECORD_UNTOUCHED, RECORD_UPDATED, RECORD_CLEARED = 0, 1, 2

_RECORD_ARRAYS = (("state", np.uint8, "s"), ("gt", np.int32, "s2"), ("genotype_log_prob", np.float32, "s"), ("hap1_log_prob", np.float32, "s"),
                  ("hap2_log_prob", np.float32, "s"), ("read_first", np.int64, "s1"), ("n_hap1", np.int32, "s"), ("n_hap2", np.int32, "s"),
                  ("reads", np.int32, "r"))


class VariantRecords(C.Structure):
    _fields_ = [("n_primary", C.c_int64), ("n_filtered", C.c_int64)] + [(f, C.c_void_p) for f, _, _ in _RECORD_ARRAYS]


class PhaseAlignedRecordsStats(C.Structure):
    _fields_ = [("filtered", PhaseAlignedFilteredStats), ("records_sites", C.c_int64), ("records_updated", C.c_int64), ("reads_listed", C.c_int64),
                ("records_bytes_downloaded", C.c_int64), ("records_ms", C.c_double)]


class QueueRecordsStats(C.Structure):
    _fields_ = [("records_sites", C.c_int64), ("records_updated", C.c_int64), ("reads_listed", C.c_int64), ("records_bytes_downloaded", C.c_int64),
                ("records_ms", C.c_double)]


class ContigChunk(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("read_names", C.c_void_p), ("read_id", C.c_void_p), ("hap_out", C.c_void_p), ("phred_out", C.c_void_p),
                ("filtered_out", C.POINTER(FilteredOut)), ("filtered_read_out", C.c_void_p), ("records", C.POINTER(VariantRecords)),
                ("n_variants", C.c_int64), ("n_fvariants", C.c_int64), ("variant_pos", C.c_void_p), ("n_alleles", C.c_void_p),
                ("fvariant_pos", C.c_void_p), ("fn_alleles", C.c_void_p)]


class ContigRules(C.Structure):
    _fields_ = [("primary_reads_only", C.c_int32), ("prevent_switching", C.c_int32), ("min_spanning_reads", C.c_int64),
                ("min_binomial_read_split_likelihood", C.c_double), ("max_discordant_ratio", C.c_double)]


class RecordVariants(C.Structure):
    _fields_ = [("n_variants", C.c_int64), ("variants", C.POINTER(Variant)), ("chunk", C.c_void_p), ("site", C.c_void_p),
                ("genotype_log_prob", C.c_void_p), ("hap1_log_prob", C.c_void_p), ("hap2_log_prob", C.c_void_p)]


class ContigOut(C.Structure):
    _fields_ = [("n_chunks", C.c_int64), ("switched", C.c_void_p), ("counts", C.c_void_p), ("final_hap", C.POINTER(C.c_void_p)), ("variants", RecordVariants),
                ("phase_set", C.c_void_p), ("reason", C.c_void_p)]


def load():
    """dlopen the in-tree library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    L.mrp_runtime_init.restype = C.c_int
    L.mrp_runtime_init()  # before the first HIP call of this process (as INTEGRATION.md asks of a caller)
    vp, i64, i32, u32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32
    P = C.POINTER
    L.mrp_last_error.restype = C.c_char_p
    L.mrp_version.restype = C.c_char_p
    L.mrp_abi_version.restype = C.c_int
    if L.mrp_abi_version() != ABI_VERSION:
        raise MrpError(f"libmargin_rphmm.so speaks ABI {L.mrp_abi_version()}, this binding was transcribed from ABI {ABI_VERSION} of include/margin_rphmm.h")
    L.mrp_device_count.restype = C.c_int
    L.mrp_context_create.argtypes = [C.c_int, P(vp)]
    L.mrp_context_destroy.argtypes = [vp]
    L.mrp_context_destroy.restype = None
    L.mrp_context_synchronize.argtypes = [vp]
    L.mrp_context_trim.argtypes = [vp]
    L.mrp_context_set_phase_groups.argtypes = [vp, C.c_int]
    L.mrp_context_set_test_hooks.argtypes = [vp, C.c_int]
    L.mrp_context_launch_census.argtypes = [vp, P(C.c_uint64), C.c_int, C.c_int]
    L.mrp_launch_class_name.argtypes = [C.c_int]
    L.mrp_launch_class_name.restype = C.c_char_p
    L.mrp_set_host_threads.argtypes = [C.c_int]
    L.mrp_chunk_create.argtypes = [vp, i64, vp, vp, vp, vp, i64, P(vp)]
    L.mrp_chunk_destroy.argtypes = [vp]
    L.mrp_chunk_destroy.restype = None
    L.mrp_fb_run.argtypes = [vp, i64, P(HmmJob)]
    L.mrp_batch_create.argtypes = [vp, P(vp)]
    L.mrp_batch_add.argtypes = [vp, P(HmmJob)]
    L.mrp_batch_upload.argtypes = [vp]
    L.mrp_batch_launch.argtypes = [vp]
    L.mrp_batch_download.argtypes = [vp]
    L.mrp_batch_destroy.argtypes = [vp]
    L.mrp_batch_destroy.restype = None
    L.mrp_batch_stats.argtypes = [vp, P(LaunchStats)]
    L.mrp_count_bit_vectors.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.mrp_emissions.argtypes = [vp, vp, i32, i32, i32, vp, u32, i64, vp, vp]
    L.mrp_get_rp_hmms.argtypes = [vp, vp, P(ReadRec), vp, i64, P(Params), vp, P(P(vp)), P(i64)]
    L.mrp_hmm_destroy.argtypes = [vp]
    L.mrp_hmm_destroy.restype = None
    L.mrp_free.argtypes = [vp]
    L.mrp_free.restype = None
    L.mrp_hmm_view.argtypes = [vp, P(HmmJob), P(vp), P(i32), P(i32)]
    L.mrp_hmm_forward_backward.argtypes = [vp, vp, vp, P(Params), vp]
    L.mrp_hmm_prune.argtypes = [vp, P(Params)]
    L.mrp_hmm_forward_trace_back.argtypes = [vp, vp]
    L.mrp_hmm_split.argtypes = [vp, P(ReadRec), i64, vp, i32, P(vp)]
    L.mrp_hmm_split_where_phasing_is_uncertain.argtypes = [vp, vp, P(ReadRec), i64, vp, P(Params), P(P(vp)), P(i64)]
    L.mrp_phase_reads.argtypes = [vp, vp, P(ReadRec), i64, P(Params), vp, P(P(PhaseResult))]
    L.mrp_phase_result_destroy.argtypes = [P(PhaseResult)]
    L.mrp_phase_result_destroy.restype = None
    L.mrp_get_rp_hmms_resident.argtypes = [vp, vp, P(ReadRec), vp, i64, P(Params), P(P(vp)), P(i64)]
    L.mrp_phase_reads_many.argtypes = [vp, i64, P(vp), P(P(ReadRec)), P(i64), P(Params), P(P(PhaseResult)), P(PhaseManyStats)]
    L.mrp_reference_from_bubbles.argtypes = [P(Bubbles), C.c_double, P(vp), P(vp), P(vp)]
    L.mrp_profile_seqs_from_bubbles.argtypes = [P(Bubbles), i64, vp, vp, P(P(ReadRec)), P(vp), P(i64), P(vp), P(i64)]
    L.mrp_assign_reads_to_haplotypes.argtypes = [i64, vp, vp, P(ReadRec), i64, P(PhaseResult), i64, vp, vp]
    L.mrp_stitch_create.argtypes = [P(vp)]
    L.mrp_stitch_destroy.argtypes = [vp]
    L.mrp_stitch_destroy.restype = None
    L.mrp_stitch_chunk.argtypes = [vp, i64, vp, vp, i64, vp, vp, C.c_int, C.c_int, P(C.c_int), vp]
    L.mrp_stitch_size.argtypes = [vp, C.c_int]
    L.mrp_stitch_size.restype = i64
    L.mrp_stitch_lookup.argtypes = [vp, C.c_int, C.c_char_p, P(C.c_double)]
    L.mrp_phase_sets.argtypes = [i64, P(Variant), i64, C.c_double, C.c_double, vp, vp]
    L.mrp_binomial_p_value.argtypes = [i64, i64]
    L.mrp_binomial_p_value.restype = C.c_double
    L.mrp_binomial_coefficient.argtypes = [i64, i64, P(C.c_uint64), P(C.c_uint64)]
    L.mrp_binomial_coefficient.restype = C.c_double
    L.mrp_symbols_from_chars.argtypes = [C.c_char_p, i64, vp]
    L.mrp_symbols_from_chars.restype = None
    L.mrp_pair_hmm_reverse_complement.argtypes = [P(PairHmm)]
    L.mrp_pair_hmm_reverse_complement.restype = None
    L.mrp_band_diagonals.argtypes = [vp, i64, i64, i64, i64, vp, vp]
    L.mrp_pair_diagonal_width.argtypes = [vp, i64, i64, i64, i64, P(i32), P(i64)]
    L.mrp_context_set_wide_pairs.argtypes = [vp, C.c_int]
    L.mrp_context_wide_pair_count.argtypes = [vp, P(i64), P(i64)]
    L.mrp_queue_set_wide_pairs.argtypes = [vp, C.c_int]
    L.mrp_queue_wide_pair_count.argtypes = [vp, P(i64), P(i64)]
    L.mrp_context_set_sv_split.argtypes = [vp, C.c_int]
    L.mrp_queue_set_sv_split.argtypes = [vp, C.c_int]
    L.mrp_mark_structural_variants.argtypes = [P(AlignedChunk), i64, vp]
    L.mrp_context_set_downsampling.argtypes = [vp, i64, C.c_uint64]
    L.mrp_queue_set_downsampling.argtypes = [vp, i64, C.c_uint64]
    L.mrp_context_last_downsampling.argtypes = [vp, P(DownsamplingStats)]
    L.mrp_downsample_draw.argtypes = [C.c_uint64, i64, i64, i64]
    L.mrp_downsample_draw.restype = C.c_double
    L.mrp_aln_read_lengths.argtypes = [P(AlignedChunk), vp]
    L.mrp_downsample_keep_from_extracted.argtypes = [P(ExtractedChunk), vp, i64, C.c_uint64, i64, i64, vp, vp, P(i32)]
    L.mrp_downsample_reads.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, i64, C.c_uint64, vp, vp, vp, vp, P(DownsamplingStats)]
    L.mrp_forward_probabilities.argtypes = [vp, vp, i32, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, C.c_int, C.c_int, vp, P(PairHmmStats)]
    L.mrp_posterior_tracebacks.argtypes = [vp, i64, i64, i64, P(PosteriorOptions), vp, i64, P(i64)]
    L.mrp_posterior_aligned_pairs.argtypes = [vp, vp, i32, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, P(PosteriorOptions), P(PosteriorPairs), P(PosteriorPairs),
                                              P(PosteriorPairs), vp, P(PairHmmStats)]
    L.mrp_posterior_pairs_free.argtypes = [P(PosteriorPairs)]
    L.mrp_posterior_pairs_free.restype = None
    L.mrp_context_set_posterior_workspace.argtypes = [vp, i64]
    L.mrp_context_last_posterior.argtypes = [vp, P(PosteriorStats)]
    L.mrp_band_diagonals_dynamic.argtypes = [vp, i64, i64, i64, vp, vp, vp]
    L.mrp_pair_diagonal_width_dynamic.argtypes = [vp, i64, i64, i64, vp, P(i32), P(i64)]
    L.mrp_posterior_tracebacks_dynamic.argtypes = [vp, vp, i64, i64, i64, P(PosteriorOptions), vp, i64, P(i64)]
    L.mrp_posterior_aligned_pairs_dynamic.argtypes = [vp, vp, i32, i64, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, P(PosteriorOptions), P(PosteriorPairs),
                                                      P(PosteriorPairs), P(PosteriorPairs), vp, vp]
    L.mrp_rle_compress.argtypes = [C.c_char_p, i64, i32, vp, vp]
    L.mrp_rle_compress.restype = i64
    L.mrp_forward_probabilities_rle.argtypes = [vp, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, C.c_int, C.c_int, vp, P(PairHmmStats)]
    L.mrp_posterior_aligned_pairs_rle.argtypes = [vp, vp, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, P(PosteriorOptions), P(PosteriorPairs),
                                                  P(PosteriorPairs), P(PosteriorPairs), vp, P(PairHmmStats)]
    L.mrp_context_set_rle_lane_pairs.argtypes = [vp, C.c_int]
    L.mrp_rle_lane_caps.argtypes = [i32, vp, P(i32)]
    L.mrp_allele_read_supports_rle.argtypes = [vp, P(PairHmm), P(PairHmm), P(RepeatModelStruct), P(RepeatModelStruct), i64, vp, vp, vp, vp, i64, vp, vp, vp, vp,
                                               vp, i64, vp, P(PairHmmStats)]
    L.mrp_ml_repeat_counts.argtypes = [vp, vp, i32, i64, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, P(PosteriorPairs), P(RepeatCountOptions), vp, vp, vp,
                                       P(RepeatCountStats)]
    L.mrp_rle_expand.argtypes = [vp, vp, vp, i64, vp, i64]
    L.mrp_rle_expand.restype = i64
    L.mrp_poa_augment.argtypes = [vp, i32, i64, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, P(PosteriorPairs), P(PosteriorPairs), P(PosteriorPairs),
                                  P(PoaOptions), P(Poa), P(PoaStats)]
    L.mrp_poa_augment.restype = C.c_int
    L.mrp_poa_free.argtypes = [P(Poa)]
    L.mrp_poa_free.restype = None
    L.mrp_poa_consensus.argtypes = [i64] + [vp] * 10 + [i64] + [vp] * 4 + [i32, P(C.POINTER(C.c_uint8)), P(C.POINTER(C.c_int32)), P(i64), P(C.POINTER(C.c_int64))]
    L.mrp_poa_consensus.restype = C.c_int
    L.mrp_context_set_posterior_wide_pairs.argtypes = [vp, C.c_int]
    L.mrp_context_posterior_wide_count.argtypes = [vp, P(i64), P(i64)]
    L.mrp_allele_read_supports.argtypes = [vp, P(PairHmm), P(PairHmm), i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, i64, vp, P(PairHmmStats)]
    L.mrp_partition_reads_by_haplotype.argtypes = [vp, P(PairHmm), P(PairHmm), P(HaptagSites), i64, vp, i64, vp, vp, vp, P(PairHmmStats)]
    L.mrp_phase_variants_from_tagged_reads.argtypes = [vp, P(PairHmm), P(PairHmm), P(HaptagSites), i64, vp, vp, i64, i64, vp, vp, vp, P(PairHmmStats)]
    L.mrp_phase_string_chunks.argtypes = [vp, i64, P(StringChunk), P(PairHmm), P(PairHmm), i64, i64, C.c_double, P(Params), i64, P(P(PhaseResult)),
                                          P(vp), P(vp), P(ProfileOut), P(StringChunksStats)]
    L.mrp_string_chunk_units.argtypes = [P(StringChunk), P(i64)]
    L.mrp_queue_phase_string_chunks.argtypes = [vp, i64, P(StringChunk), P(PairHmm), P(PairHmm), i64, i64, C.c_double, P(Params), i64, i64,
                                                P(P(PhaseResult)), P(vp), P(vp), P(ProfileOut), P(QueueStats)]
    L.mrp_phase_string_chunks_on_devices.argtypes = [vp, i32] + L.mrp_queue_phase_string_chunks.argtypes[1:]
    L.mrp_phase_string_chunks_with_filtered.argtypes = [vp, i64, P(StringChunk), P(StringChunkRest), P(PairHmm), P(PairHmm), i64, i64, C.c_double, P(Params),
                                                        i64, P(P(PhaseResult)), P(vp), P(vp), P(ProfileOut), P(FilteredOut), P(StringFilteredStats)]
    L.mrp_queue_phase_string_chunks_with_filtered.argtypes = [vp, i64, P(StringChunk), P(StringChunkRest), P(PairHmm), P(PairHmm), i64, i64, C.c_double,
                                                              P(Params), i64, i64, P(P(PhaseResult)), P(vp), P(vp), P(ProfileOut), P(FilteredOut), P(QueueStats)]
    L.mrp_phase_string_chunks_with_filtered_on_devices.argtypes = [vp, i32] + L.mrp_queue_phase_string_chunks_with_filtered.argtypes[1:]
    L.mrp_extract_read_substrings.argtypes = [vp, i64, P(AlignedChunk), P(ExtractOptions), P(P(ExtractedChunk)), P(ExtractStats)]
    L.mrp_string_chunk_from_extracted.argtypes = [P(ExtractedChunk), vp, vp, vp, P(StringChunk), P(P(C.c_int64))]
    L.mrp_haptag_sites_from_extracted.argtypes = [i64, P(ExtractedChunk), P(vp), P(HaptagSites), vp]
    L.mrp_haplotag_aligned_chunks.argtypes = [vp, i64, P(AlignedChunk), P(vp), P(ExtractOptions), P(PairHmm), P(PairHmm), i64, P(vp), P(vp), P(vp),
                                              P(HaplotagAlignedStats)]
    ha = L.mrp_haplotag_aligned_chunks.argtypes
    L.mrp_haplotag_chunk_units.argtypes = [P(AlignedChunk), vp, P(i64)]
    # the one call's list with chunks_per_batch behind the expansion and the queue's stats in place of the call's
    L.mrp_queue_haplotag_aligned_chunks.argtypes = ha[:8] + [i64] + ha[8:-1] + [P(QueueStats)]
    L.mrp_haplotag_aligned_chunks_on_devices.argtypes = [vp, i32] + L.mrp_queue_haplotag_aligned_chunks.argtypes[1:]
    L.mrp_phase_aligned_chunks.argtypes = [vp, i64, P(AlignedChunk), P(vp), P(vp), P(ExtractOptions), P(PairHmm), P(PairHmm), i64, i64, C.c_double,
                                           P(Params), i64, P(P(PhaseResult)), P(vp), P(vp), P(ProfileOut), P(vp), P(PhaseAlignedStats)]
    L.mrp_phase_aligned_chunks_with_filtered.argtypes = [vp, i64, P(AlignedChunk), P(AlignedChunkRest), P(vp), P(vp), P(ExtractOptions), P(PairHmm),
                                                         P(PairHmm), i64, i64, C.c_double, P(Params), i64, P(P(PhaseResult)), P(vp), P(vp),
                                                         P(ProfileOut), P(vp), P(FilteredOut), P(vp), P(PhaseAlignedFilteredStats)]
    pa, pf = L.mrp_phase_aligned_chunks.argtypes, L.mrp_phase_aligned_chunks_with_filtered.argtypes
    L.mrp_phase_aligned_chunks_with_records.argtypes = pf[:-1] + [P(VariantRecords), P(PhaseAlignedRecordsStats)]
    L.mrp_variant_records_from_extracted.argtypes = [P(ExtractedChunk), P(ExtractedChunk), vp, vp, i64, P(PhaseResult), vp, vp, vp, i64, i64, vp, vp,
                                                     P(VariantRecords)]
    L.mrp_variants_from_records.argtypes = [i64, P(VariantRecords), P(vp), P(vp), P(vp), P(vp), vp, P(vp), P(RecordVariants)]
    L.mrp_aligned_chunk_units.argtypes = [P(AlignedChunk), P(AlignedChunkRest), P(i64)]
    # the one call's list with chunks_per_batch behind min_phred and the queue's stats in place of the call's
    L.mrp_queue_phase_aligned_chunks.argtypes = pa[:13] + [i64] + pa[13:-1] + [P(QueueStats)]
    L.mrp_queue_phase_aligned_chunks_with_filtered.argtypes = pf[:14] + [i64] + pf[14:-1] + [P(QueueStats)]
    L.mrp_phase_aligned_chunks_on_devices.argtypes = [vp, i32] + L.mrp_queue_phase_aligned_chunks.argtypes[1:]
    L.mrp_phase_aligned_chunks_with_filtered_on_devices.argtypes = [vp, i32] + L.mrp_queue_phase_aligned_chunks_with_filtered.argtypes[1:]
    L.mrp_queue_phase_aligned_chunks_with_records.argtypes = L.mrp_queue_phase_aligned_chunks_with_filtered.argtypes[:-1] + \
        [P(VariantRecords), P(QueueStats), P(QueueRecordsStats)]
    L.mrp_phase_aligned_chunks_with_records_on_devices.argtypes = [vp, i32] + L.mrp_queue_phase_aligned_chunks_with_records.argtypes[1:]
    L.mrp_final_read_tags.argtypes = [i64, vp, P(FilteredOut), vp, vp]
    L.mrp_stitch_values.argtypes = [i64, vp, vp, vp, vp]
    L.mrp_close_contig.argtypes = [i64, P(ContigChunk), P(ContigRules), P(ContigOut)]
    L.mrp_close_contigs.argtypes = [i64, vp, P(ContigChunk), P(ContigRules), P(ContigOut)]
    L.mrp_contig_out_clear.argtypes = [P(ContigOut)]
    L.mrp_contig_out_clear.restype = None
    L.mrp_kmer_alignment_anchors_many.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, vp, P(vp), P(PairHmmStats)]
    L.mrp_string_chunk_rest_from_extracted.argtypes = [P(ExtractedChunk), vp, vp, vp, i64, P(ExtractedChunk), vp, vp, i64, i64, P(StringChunkRest),
                                                       P(vp), P(vp)]
    L.mrp_equal_substring_classes.argtypes = [vp, i64, vp, vp, i64, vp, vp, vp]
    L.mrp_kmer_alignment_anchors.argtypes = [vp, i64, vp, i64, vp]
    L.mrp_kmer_alignment_anchors.restype = i64
    L.mrp_phase_chunks_on_devices.argtypes = [vp, i32, i64, P(ChunkDesc), P(Params), i64, P(P(PhaseResult)), P(QueueStats)]
    L.mrp_queue_create.argtypes = [vp, i32, P(vp)]
    L.mrp_queue_destroy.argtypes = [vp]
    L.mrp_queue_destroy.restype = None
    L.mrp_queue_phase_chunks.argtypes = [vp, i64, P(ChunkDesc), P(Params), i64, P(P(PhaseResult)), P(QueueStats)]
    L.mrp_queue_plan.argtypes = [i64, vp, i64, vp, vp]
    L.mrp_queue_dry_run.argtypes = [i32, i32, i64, vp, i64, C.c_double, vp, vp]
    _lib = L
    return L


def _check(rc: int):
    if rc != MRP_OK:
        raise MrpError(rc, load().mrp_last_error().decode())


def launch_class_names() -> list:
    """the launch classes of the device-resident path, as the library names them (mrp_launch_class_name: slot 0, 1, ... until NULL)"""
    L = load()
    names = []
    while (name := L.mrp_launch_class_name(len(names))) is not None:
        names.append(name.decode())
    return names


class Context:
    def __init__(self, device: int = 0):
        L = load()
        h = C.c_void_p()
        _check(L.mrp_context_create(device, C.byref(h)))
        self.h = h

    def synchronize(self):
        _check(load().mrp_context_synchronize(self.h))

    def trim(self):
        _check(load().mrp_context_trim(self.h))

    def set_phase_groups(self, groups: int):
        _check(load().mrp_context_set_phase_groups(self.h, groups))

    def set_test_hooks(self, hooks: int):
        """test suite only: bit 0 fault injection, bit 1 separate cross product / emission kernels, bit 2 one refused device
        allocation, bit 3 general prune chain, bit 4 one array entry per cell on unit levels, bit 5 no level is launched deferred, bit 6 the
        wide pair-HMM kernel's grid is one workgroup, bit 7 every pair of a posterior call takes the pair-per-workgroup kernels at 128 threads on a
        grid of one workgroup (include/margin_rphmm.h)"""
        _check(load().mrp_context_set_test_hooks(self.h, hooks))

    def launch_census(self, reset: bool = False) -> dict:
        """test suite and probes only: how often this context and its siblings launched each launch class of the device-resident
        path, by the library's own slot names (mrp_launch_class_name); reset zeroes the counts after the read"""
        names = launch_class_names()
        counts = (C.c_uint64 * len(names))()
        _check(load().mrp_context_launch_census(self.h, counts, len(names), int(bool(reset))))
        return dict(zip(names, (int(c) for c in counts)))

    def set_posterior_workspace(self, n_bytes: int):
        """mrp_context_set_posterior_workspace: bytes of forward diagonals a group of posterior_aligned_pairs keeps on the device (0: the default)"""
        _check(load().mrp_context_set_posterior_workspace(self.h, int(n_bytes)))

    def last_posterior(self) -> "PosteriorStats":
        st = PosteriorStats()
        _check(load().mrp_context_last_posterior(self.h, C.byref(st)))
        return st

    def set_posterior_wide_pairs(self, on):
        """mrp_context_set_posterior_wide_pairs: the posterior entries run a pair whose widest diagonal exceeds 2 048 cells (up to WIDE_MAX_WIDTH)"""
        _check(load().mrp_context_set_posterior_wide_pairs(self.h, int(bool(on))))

    def posterior_wide_count(self):
        """mrp_context_posterior_wide_count -> (pairs, band cells) the posterior entries' pair-per-workgroup kernels have taken on this context"""
        pairs, cells = C.c_int64(), C.c_int64()
        _check(load().mrp_context_posterior_wide_count(self.h, C.byref(pairs), C.byref(cells)))
        return pairs.value, cells.value

    def set_rle_lane_pairs(self, on):
        """mrp_context_set_rle_lane_pairs: forward_probabilities_rle runs its eligible pairs (unanchored, within rle_lane_caps) a pair per lane"""
        _check(load().mrp_context_set_rle_lane_pairs(self.h, int(bool(on))))

    def set_wide_pairs(self, on):
        """mrp_context_set_wide_pairs: pairs whose widest diagonal exceeds 2 048 cells are aligned, not refused (up to WIDE_MAX_WIDTH / WIDE_MAX_CELLS)"""
        _check(load().mrp_context_set_wide_pairs(self.h, int(bool(on))))

    def set_sv_split(self, on):
        """mrp_context_set_sv_split: indel_size_for_sv_handling > 0 runs the extraction's walk per class of variant (small, structural), not refused"""
        _check(load().mrp_context_set_sv_split(self.h, int(bool(on))))

    def set_downsampling(self, max_depth: int, seed: int = 0):
        """mrp_context_set_downsampling: max_depth > 0 makes the aligned composites' downsampling mask on the device (0: off); keeps=... is then refused"""
        _check(load().mrp_context_set_downsampling(self.h, int(max_depth), int(seed) & (2**64 - 1)))

    def last_downsampling(self) -> "DownsamplingStats":
        """mrp_context_last_downsampling: what the last composite call (or downsample_reads) on this context did for the downsampling"""
        st = DownsamplingStats()
        _check(load().mrp_context_last_downsampling(self.h, C.byref(st)))
        return st

    def wide_pair_count(self):
        """mrp_context_wide_pair_count -> (pairs, dp cells) the wide kernel has taken on this context"""
        pairs, cells = C.c_int64(), C.c_int64()
        _check(load().mrp_context_wide_pair_count(self.h, C.byref(pairs), C.byref(cells)))
        return pairs.value, cells.value

    def close(self):
        if self.h:
            load().mrp_context_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DeviceChunk:
    """mrp_chunk for a margin_amd.synth.Chunk (or raw arrays)."""

    def __init__(self, ctx: Context, allele_number, sub, prior, pool):
        L = load()
        self.ctx = ctx
        an = np.ascontiguousarray(allele_number, dtype=np.uint32)
        sub = None if sub is None else np.ascontiguousarray(sub, dtype=np.uint16)
        prior = None if prior is None else np.ascontiguousarray(prior, dtype=np.uint16)
        pool = np.ascontiguousarray(pool, dtype=np.uint8)
        h = C.c_void_p()
        _check(L.mrp_chunk_create(ctx.h, an.shape[0], an.ctypes.data,
                                  None if sub is None else sub.ctypes.data,
                                  None if prior is None else prior.ctypes.data,
                                  pool.ctypes.data if pool.size else None, pool.size, C.byref(h)))
        self.h = h

    @classmethod
    def from_chunk(cls, ctx: Context, chunk):
        return cls(ctx, chunk.allele_number, chunk.sub, chunk.prior, chunk.pool)

    def close(self):
        if self.h:
            load().mrp_chunk_destroy(self.h)
            self.h = None


_IN = [("col_ref_start", np.int32), ("col_length", np.int32), ("col_depth", np.int32), ("col_cell_off", np.int64),
       ("col_read_off", np.int64), ("read_byte_off", np.int64), ("partition", np.uint64), ("mask_from", np.uint64),
       ("mask_to", np.uint64), ("mcol_cell_off", np.int64), ("merge_from", np.uint64), ("merge_to", np.uint64)]


class Job:
    """Owns the numpy arrays behind one mrp_hmm_job and its outputs."""

    def __init__(self, dchunk: DeviceChunk, flat: Dict[str, np.ndarray], flags: int, use_indices: bool = True):
        K = int(flat["n_columns"])
        self.K = K
        self.arr = {}
        for name, dt in _IN:
            a = np.ascontiguousarray(flat[name], dtype=dt)
            if a.size == 0:
                a = np.zeros(1, dtype=dt)
            self.arr[name] = a
        nC = int(flat["col_cell_off"][K])
        nM = int(flat["mcol_cell_off"][K - 1]) if K > 1 else 0
        self.n_cells, self.n_merge = nC, nM
        if use_indices and "cell_next" in flat:
            self.arr["cell_next"] = np.ascontiguousarray(flat["cell_next"], dtype=np.uint32)
            self.arr["cell_prev"] = np.ascontiguousarray(flat["cell_prev"], dtype=np.uint32)
        self.out = dict(cell_forward=np.full(nC, np.nan), cell_backward=np.full(nC, np.nan),
                        merge_forward=np.full(max(nM, 1), np.nan), merge_backward=np.full(max(nM, 1), np.nan),
                        col_total=np.full(K, np.nan), hmm_forward=np.full(1, np.nan), hmm_backward=np.full(1, np.nan))
        j = HmmJob()
        j.chunk = dchunk.h
        j.n_columns = K
        j.flags = flags
        for name, _ in _IN:
            setattr(j, name, self.arr[name].ctypes.data)
        j.cell_next = self.arr["cell_next"].ctypes.data if "cell_next" in self.arr else None
        j.cell_prev = self.arr["cell_prev"].ctypes.data if "cell_prev" in self.arr else None
        for name, a in self.out.items():
            setattr(j, name, a.ctypes.data)
        self.c = j

    def results(self) -> Dict[str, np.ndarray]:
        r = dict(self.out)
        r["merge_forward"] = r["merge_forward"][:self.n_merge]
        r["merge_backward"] = r["merge_backward"][:self.n_merge]
        return r


def fb_run(ctx: Context, jobs: Sequence[Job]):
    """mrp_fb_run over the given jobs (one device batch)."""
    arr = (HmmJob * max(len(jobs), 1))()
    for i, j in enumerate(jobs):
        arr[i] = j.c
    _check(load().mrp_fb_run(ctx.h, len(jobs), arr))


class Batch:
    def __init__(self, ctx: Context):
        h = C.c_void_p()
        _check(load().mrp_batch_create(ctx.h, C.byref(h)))
        self.h = h
        self.jobs: List[Job] = []

    def add(self, job: Job, keep: bool = True):
        _check(load().mrp_batch_add(self.h, C.byref(job.c)))
        if keep:
            self.jobs.append(job)

    def upload(self):
        _check(load().mrp_batch_upload(self.h))

    def launch(self):
        _check(load().mrp_batch_launch(self.h))

    def download(self):
        _check(load().mrp_batch_download(self.h))

    def stats(self) -> LaunchStats:
        s = LaunchStats()
        _check(load().mrp_batch_stats(self.h, C.byref(s)))
        return s

    def close(self):
        if self.h:
            load().mrp_batch_destroy(self.h)
            self.h = None


def count_bit_vectors(ctx: Context, dchunk: DeviceChunk, first_site: int, n_sites: int, read_byte_off,
                      n_slots: int) -> np.ndarray:
    off = np.ascontiguousarray(read_byte_off, dtype=np.int64)
    out = np.zeros(max(n_slots, 1) * 8, dtype=np.uint64)
    _check(load().mrp_count_bit_vectors(ctx.h, dchunk.h, first_site, n_sites, off.shape[0],
                                        off.ctypes.data if off.size else None, out.ctypes.data))
    return out[:n_slots * 8]


def emissions(ctx: Context, dchunk: DeviceChunk, first_site: int, n_sites: int, read_byte_off, flags: int,
              partitions) -> np.ndarray:
    off = np.ascontiguousarray(read_byte_off, dtype=np.int64)
    part = np.ascontiguousarray(partitions, dtype=np.uint64)
    out = np.zeros(max(part.shape[0], 1), dtype=np.float64)
    _check(load().mrp_emissions(ctx.h, dchunk.h, first_site, n_sites, off.shape[0],
                                off.ctypes.data if off.size else None, flags, part.shape[0], part.ctypes.data,
                                out.ctypes.data))
    return out[:part.shape[0]]


# ---- host pipeline (rphmm_chunk.c, rphmm_host.c, rphmm_many.c) -------------------------------

def read_records(chunk):
    """mrp_read[] for a margin_amd.synth.Chunk; returns (ctypes array, keep-alive list).  Cached on the chunk."""
    cached = getattr(chunk, "_mrp_records", None)
    if cached is not None and cached[2] == len(chunk.reads):
        return cached[0], cached[1]
    n = len(chunk.reads)
    arr = (ReadRec * max(n, 1))()
    names = [r.name.encode() for r in chunk.reads]
    for i, r in enumerate(chunk.reads):
        arr[i].name = names[i]
        arr[i].ref_start = r.ref_start
        arr[i].length = r.length
        arr[i].forward_strand = r.strand
        arr[i].pool_offset = r.pool_off
    try:
        chunk._mrp_records = (arr, names, n)
    except AttributeError:
        pass
    return arr, names


def _as_np(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(n,)).copy()


def hmm_to_flat(hmm_handle) -> Dict[str, np.ndarray]:
    """Copy a flat mrp_hmm into the same dict layout oracle.orc.flatten produces."""
    L = load()
    v = HmmJob()
    cr = C.c_void_p()
    rs, rl = C.c_int32(), C.c_int32()
    _check(L.mrp_hmm_view(hmm_handle, C.byref(v), C.byref(cr), C.byref(rs), C.byref(rl)))
    K = int(v.n_columns)
    cell_off = _as_np(v.col_cell_off, K + 1, np.int64)
    read_off = _as_np(v.col_read_off, K + 1, np.int64)
    mcol = _as_np(v.mcol_cell_off, K, np.int64)
    nC, nD, nM = int(cell_off[K]), int(read_off[K]), int(mcol[K - 1]) if K > 1 else 0
    d = dict(n_columns=K, ref_start=rs.value, ref_length=rl.value,
             col_ref_start=_as_np(v.col_ref_start, K, np.int32), col_length=_as_np(v.col_length, K, np.int32),
             col_depth=_as_np(v.col_depth, K, np.int32), col_cell_off=cell_off, col_read_off=read_off,
             read_byte_off=_as_np(v.read_byte_off, nD, np.int64), read_ids=_as_np(cr, nD, np.int32).astype(np.int64),
             partition=_as_np(v.partition, nC, np.uint64), mask_from=_as_np(v.mask_from, K - 1, np.uint64),
             mask_to=_as_np(v.mask_to, K - 1, np.uint64), mcol_cell_off=mcol,
             merge_from=_as_np(v.merge_from, nM, np.uint64), merge_to=_as_np(v.merge_to, nM, np.uint64),
             cell_next=_as_np(v.cell_next, nC, np.uint32), cell_prev=_as_np(v.cell_prev, nC, np.uint32))
    if v.cell_forward:
        d.update(cell_forward=_as_np(v.cell_forward, nC, np.float64), cell_backward=_as_np(v.cell_backward, nC, np.float64),
                 merge_forward=_as_np(v.merge_forward, nM, np.float64), merge_backward=_as_np(v.merge_backward, nM, np.float64),
                 col_total=_as_np(v.col_total, K, np.float64),
                 hmm_forward=float(C.cast(v.hmm_forward, C.POINTER(C.c_double))[0]),
                 hmm_backward=float(C.cast(v.hmm_backward, C.POINTER(C.c_double))[0]))
    return d


def get_rp_hmms(ctx: Context, dchunk: DeviceChunk, chunk, params: Params, read_index=None, record: Optional[Batch] = None):
    """mrp_get_rp_hmms; returns list of opaque hmm handles (destroy with hmm_destroy)."""
    L = load()
    recs, _keep = read_records(chunk)
    idx = np.arange(len(chunk.reads), dtype=np.int32) if read_index is None else np.ascontiguousarray(read_index, dtype=np.int32)
    out = C.POINTER(C.c_void_p)()
    n_out = C.c_int64(0)
    _check(L.mrp_get_rp_hmms(ctx.h, dchunk.h, recs, idx.ctypes.data if idx.size else None, idx.shape[0],
                             C.byref(params), record.h if record else None, C.byref(out), C.byref(n_out)))
    hmms = [C.c_void_p(out[i]) for i in range(n_out.value)]
    L.mrp_free(out)
    return hmms


def get_rp_hmms_resident(ctx: Context, dchunk: DeviceChunk, chunk, params: Params, read_index=None):
    """mrp_get_rp_hmms_resident: same result as get_rp_hmms, merge levels resident on the device."""
    L = load()
    recs, _keep = read_records(chunk)
    idx = np.arange(len(chunk.reads), dtype=np.int32) if read_index is None else np.ascontiguousarray(read_index, dtype=np.int32)
    out = C.POINTER(C.c_void_p)()
    n_out = C.c_int64(0)
    _check(L.mrp_get_rp_hmms_resident(ctx.h, dchunk.h, recs, idx.ctypes.data if idx.size else None, idx.shape[0],
                                      C.byref(params), C.byref(out), C.byref(n_out)))
    hmms = [C.c_void_p(out[i]) for i in range(n_out.value)]
    L.mrp_free(out)
    return hmms


def hmm_destroy(h):
    load().mrp_hmm_destroy(h)


def hmm_forward_backward(ctx: Context, dchunk: DeviceChunk, h, params: Params):
    _check(load().mrp_hmm_forward_backward(ctx.h, dchunk.h, h, C.byref(params), None))


def hmm_split(dchunk: DeviceChunk, chunk, h, split_point: int):
    """mrp_hmm_split: h keeps the prefix, returns the suffix hmm."""
    recs, _keep = read_records(chunk)
    out = C.c_void_p()
    _check(load().mrp_hmm_split(dchunk.h, recs, len(chunk.reads), h, int(split_point), C.byref(out)))
    return out


def hmm_split_where_phasing_is_uncertain(ctx: Context, dchunk: DeviceChunk, chunk, h, params: Params):
    """mrp_hmm_split_where_phasing_is_uncertain: list of hmm handles, the first one is h itself."""
    L = load()
    recs, _keep = read_records(chunk)
    out = C.POINTER(C.c_void_p)()
    n_out = C.c_int64(0)
    _check(L.mrp_hmm_split_where_phasing_is_uncertain(ctx.h, dchunk.h, recs, len(chunk.reads), h, C.byref(params), C.byref(out), C.byref(n_out)))
    hmms = [C.c_void_p(out[i]) for i in range(n_out.value)]
    L.mrp_free(out)
    return hmms


def hmm_forward_trace_back(h, n_columns: int) -> np.ndarray:
    path = np.zeros(n_columns, dtype=np.int32)
    _check(load().mrp_hmm_forward_trace_back(h, path.ctypes.data))
    return path


def _phase_result_dict(g) -> dict:
    n = int(g.length)
    return dict(ref_start=int(g.ref_start), length=n,
               reads1=[int(g.reads1[i]) for i in range(g.n_reads1)], reads2=[int(g.reads2[i]) for i in range(g.n_reads2)],
               hap1=_as_np(g.haplotype_string1, n, np.uint64), hap2=_as_np(g.haplotype_string2, n, np.uint64),
               genotype=_as_np(g.genotype_string, n, np.uint64), ancestor=_as_np(g.ancestor_string, n, np.uint64),
               genotype_probs=_as_np(g.genotype_probs, n, np.float32), hap_probs1=_as_np(g.haplotype_probs1, n, np.float32),
               hap_probs2=_as_np(g.haplotype_probs2, n, np.float32),
               support1=_as_np(g.reads_supporting_haplotype1, n, np.uint64),
               support2=_as_np(g.reads_supporting_haplotype2, n, np.uint64),
               hmm_forward=float(g.hmm_forward), hmm_backward=float(g.hmm_backward), n_sweeps=int(g.n_sweeps))


def phase_reads(ctx: Context, dchunk: DeviceChunk, chunk, params: Params, record: Optional[Batch] = None) -> dict:
    """mrp_phase_reads (bubbleGraph.c:2673 driver) -> dict with the same keys as the oracle's."""
    L = load()
    recs, _keep = read_records(chunk)
    res = C.POINTER(PhaseResult)()
    _check(L.mrp_phase_reads(ctx.h, dchunk.h, recs, len(chunk.reads), C.byref(params), record.h if record else None,
                             C.byref(res)))
    out = _phase_result_dict(res.contents)
    L.mrp_phase_result_destroy(res)
    return out


def phase_many_args(dchunks: Sequence[DeviceChunk], chunks: Sequence):
    """the argument arrays of mrp_phase_reads_many for these chunks, built once (a timing loop hands them back through
    `prepared` instead of rebuilding three ctypes arrays per call)"""
    n = len(chunks)
    keep = [read_records(c) for c in chunks]
    ch = (C.c_void_p * max(n, 1))(*[d.h for d in dchunks])
    rd = (C.POINTER(ReadRec) * max(n, 1))(*[C.cast(k[0], C.POINTER(ReadRec)) for k in keep])
    nr = (C.c_int64 * max(n, 1))(*[len(c.reads) for c in chunks])
    return ch, rd, nr, keep


class DeferredResult:
    """an mrp_phase_result the caller converts later (outside a timed region): .get() -> result dict, once"""

    def __init__(self, ptr):
        self.ptr = ptr

    def get(self):
        d = _phase_result_dict(self.ptr.contents)
        load().mrp_phase_result_destroy(self.ptr)
        self.ptr = None
        return d


def phase_reads_many(ctx: Context, dchunks: Sequence[DeviceChunk], chunks: Sequence, params: Params, convert: bool = True, prepared=None, defer=()):
    """mrp_phase_reads_many -> (list of result dicts, PhaseManyStats).  convert=False skips the Python copies of the
    results (timing runs); the results of the chunks listed in `defer` come back as DeferredResult whatever `convert` says;
    prepared = phase_many_args(dchunks, chunks)."""
    L = load()
    n = len(chunks)
    ch, rd, nr, _keep = prepared if prepared is not None else phase_many_args(dchunks, chunks)
    res = (C.POINTER(PhaseResult) * max(n, 1))()
    st = PhaseManyStats()
    _check(L.mrp_phase_reads_many(ctx.h, n, ch, rd, nr, C.byref(params), res, C.byref(st)))
    out = []
    later = set(defer)
    for i in range(n):
        if i in later:
            out.append(DeferredResult(res[i]))
            continue
        out.append(_phase_result_dict(res[i].contents) if convert else None)
        L.mrp_phase_result_destroy(res[i])
    return out, st


# ---- the work queue over the GPUs of a node (mrp_queue.cpp) -----------------------------------

def chunk_descs(chunks):
    """mrp_chunk_desc[] for margin_amd.synth.Chunk objects; returns (ctypes array, keep-alive list)"""
    n = len(chunks)
    arr = (ChunkDesc * max(n, 1))()
    keep = []
    for i, c in enumerate(chunks):
        an = np.ascontiguousarray(c.allele_number, dtype=np.uint32)
        sub = np.ascontiguousarray(c.sub, dtype=np.uint16)
        prior = np.ascontiguousarray(c.prior, dtype=np.uint16)
        pool = np.ascontiguousarray(c.pool, dtype=np.uint8)
        recs, names = read_records(c)
        keep.append((an, sub, prior, pool, recs, names))
        arr[i].n_sites = an.shape[0]
        arr[i].allele_number = an.ctypes.data
        arr[i].substitution_log_probs = sub.ctypes.data if sub.size else None
        arr[i].allele_prior_log_probs = prior.ctypes.data if prior.size else None
        arr[i].profile_pool = pool.ctypes.data if pool.size else None
        arr[i].pool_bytes = pool.size
        arr[i].reads = C.cast(recs, C.POINTER(ReadRec))
        arr[i].n_reads = len(c.reads)
    return arr, keep


def phase_chunks_on_devices(devices, chunks, params: Params, chunks_per_batch: int = 48, descs=None, convert: bool = True):
    """mrp_phase_chunks_on_devices -> (list of result dicts in input order, QueueStats)"""
    L = load()
    n = len(chunks)
    arr, _keep = descs if descs is not None else chunk_descs(chunks)
    dev = (C.c_int32 * len(devices))(*devices)
    res = (C.POINTER(PhaseResult) * max(n, 1))()
    st = QueueStats()
    _check(L.mrp_phase_chunks_on_devices(C.cast(dev, C.c_void_p), len(devices), n, arr, C.byref(params), chunks_per_batch, res, C.byref(st)))
    out = []
    for i in range(n):
        out.append(_phase_result_dict(res[i].contents) if convert else None)
        L.mrp_phase_result_destroy(res[i])
    return out, st


class Queue:
    """mrp_queue: the workers (one per listed device) with their contexts, for repeated calls"""

    def __init__(self, devices):
        dev = (C.c_int32 * len(devices))(*devices)
        self.h = C.c_void_p()
        _check(load().mrp_queue_create(C.cast(dev, C.c_void_p), len(devices), C.byref(self.h)))

    def phase(self, chunks, params: Params, chunks_per_batch: int = 48, descs=None, convert: bool = True, defer=()):
        L = load()
        n = len(chunks)
        arr, _keep = descs if descs is not None else chunk_descs(chunks)
        res = (C.POINTER(PhaseResult) * max(n, 1))()
        st = QueueStats()
        _check(L.mrp_queue_phase_chunks(self.h, n, arr, C.byref(params), chunks_per_batch, res, C.byref(st)))
        out = []
        later = set(defer)
        for i in range(n):
            if i in later:
                out.append(DeferredResult(res[i]))
                continue
            out.append(_phase_result_dict(res[i].contents) if convert else None)
            L.mrp_phase_result_destroy(res[i])
        return out, st

    def phase_string_chunks(self, chunks, forward_model: "PairHmm", reverse_model: "PairHmm", params: Params, min_phred: int = 0,
                            chunks_per_batch: int = 0, expansion: int = 4, sv_threshold: int = 512, het_substitution_probability: float = 0.0,
                            profiles: bool = False, structs=None):
        """mrp_queue_phase_string_chunks -> (phase_string_chunks' list of dicts in input order, QueueStats)"""
        return _queue_phase_string_chunks(self.h, chunks, forward_model, reverse_model, params, min_phred, chunks_per_batch, expansion, sv_threshold,
                                          het_substitution_probability, profiles, structs)

    def phase_aligned_chunks(self, chunks, forward_model: "PairHmm", reverse_model: "PairHmm", params: Params, chunks_per_batch: int = 0, **kw):
        """mrp_queue_phase_aligned_chunks -> (phase_aligned_chunks' list of dicts in input order, QueueStats); further arguments as there"""
        return _phase_aligned(None, chunks, forward_model, reverse_model, params, queue=self.h, chunks_per_batch=chunks_per_batch, **kw)

    def phase_aligned_chunks_with_filtered(self, chunks, rests, forward_model: "PairHmm", reverse_model: "PairHmm", params: Params,
                                           chunks_per_batch: int = 0, **kw):
        """mrp_queue_phase_aligned_chunks_with_filtered -> (phase_aligned_chunks_with_filtered's list of dicts in input order, QueueStats)"""
        return _phase_aligned(None, chunks, forward_model, reverse_model, params, rests=rests, with_rest=True, queue=self.h,
                              chunks_per_batch=chunks_per_batch, **kw)

    def phase_aligned_chunks_with_records(self, chunks, rests, forward_model: "PairHmm", reverse_model: "PairHmm", params: Params,
                                          chunks_per_batch: int = 0, **kw):
        """mrp_queue_phase_aligned_chunks_with_records -> (phase_aligned_chunks_with_records' list of dicts in input order, QueueStats with
        the QueueRecordsStats as its attribute `records`)"""
        return _phase_aligned(None, chunks, forward_model, reverse_model, params, rests=rests, with_rest=True, with_records=True, queue=self.h,
                              chunks_per_batch=chunks_per_batch, **kw)

    def haplotag_aligned_chunks(self, chunks, gts, forward_model: "PairHmm", reverse_model: "PairHmm", options: Optional[dict] = None,
                                totals: bool = True, chunks_per_batch: int = 0, **kw):
        """mrp_queue_haplotag_aligned_chunks -> (haplotag_aligned_chunks' list of dicts in input order, QueueStats)"""
        return _haplotag_aligned(None, chunks, gts, forward_model, reverse_model, options=options, totals=totals, queue=self.h,
                                 chunks_per_batch=chunks_per_batch, **kw)

    def set_wide_pairs(self, on):
        """mrp_queue_set_wide_pairs: Context.set_wide_pairs for every lane's context and the queue's up-front checks"""
        _check(load().mrp_queue_set_wide_pairs(self.h, int(bool(on))))

    def set_sv_split(self, on):
        """mrp_queue_set_sv_split: Context.set_sv_split for every lane's context and the queue's up-front mode check"""
        _check(load().mrp_queue_set_sv_split(self.h, int(bool(on))))

    def set_downsampling(self, max_depth: int, seed: int = 0):
        """mrp_queue_set_downsampling: Context.set_downsampling for every lane's context and the queue's up-front checks"""
        _check(load().mrp_queue_set_downsampling(self.h, int(max_depth), int(seed) & (2**64 - 1)))

    def wide_pair_count(self):
        """mrp_queue_wide_pair_count -> (pairs, dp cells), summed over the lanes"""
        pairs, cells = C.c_int64(), C.c_int64()
        _check(load().mrp_queue_wide_pair_count(self.h, C.byref(pairs), C.byref(cells)))
        return pairs.value, cells.value

    def close(self):
        if self.h:
            load().mrp_queue_destroy(self.h)
            self.h = None


def queue_plan(cost, chunks_per_batch: int):
    cost = np.ascontiguousarray(cost, dtype=np.int64)
    order = np.zeros(len(cost), dtype=np.int64)
    batch = np.zeros(len(cost), dtype=np.int64)
    _check(load().mrp_queue_plan(len(cost), cost.ctypes.data, chunks_per_batch, order.ctypes.data, batch.ctypes.data))
    return order, batch


def queue_dry_run(n_devices: int, lanes: int, cost, chunks_per_batch: int, usec_per_cost: float = 0.0):
    """worker (= device * lanes + lane) and global take position of every chunk"""
    cost = np.ascontiguousarray(cost, dtype=np.int64)
    worker = np.full(len(cost), -1, dtype=np.int32)
    seq = np.full(len(cost), -1, dtype=np.int64)
    _check(load().mrp_queue_dry_run(n_devices, lanes, len(cost), cost.ctypes.data, chunks_per_batch, usec_per_cost, worker.ctypes.data, seq.ctypes.data))
    return worker, seq


# ---- the frame around the path (rphmm_frame.c): host only -------------------------------------

def _bubbles_struct(allele_number, bubble_reads, supports):
    """allele_number[i]; bubble_reads[i] = list of read indices; supports[i] = float32 array [alleleNo][readNo]"""
    an = np.ascontiguousarray(allele_number, dtype=np.uint32)
    read_off = np.zeros(len(an) + 1, dtype=np.int64)
    sup_off = np.zeros(len(an) + 1, dtype=np.int64)
    for i, r in enumerate(bubble_reads):
        read_off[i + 1] = read_off[i] + len(r)
        sup_off[i + 1] = sup_off[i] + int(an[i]) * len(r)
    reads = np.ascontiguousarray([x for r in bubble_reads for x in r], dtype=np.int32)
    sup = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.float32).reshape(-1) for s in supports])
                               if len(supports) else np.zeros(0, np.float32), dtype=np.float32)
    b = Bubbles(len(an), an.ctypes.data, read_off.ctypes.data, reads.ctypes.data, sup_off.ctypes.data, sup.ctypes.data)
    return b, (an, read_off, sup_off, reads, sup)


def reference_from_bubbles(allele_number, bubble_reads, supports, het_substitution_probability):
    L = load()
    b, _keep = _bubbles_struct(allele_number, bubble_reads, supports)
    an, sub, prior = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(L.mrp_reference_from_bubbles(C.byref(b), het_substitution_probability, C.byref(an), C.byref(sub), C.byref(prior)))
    n = len(allele_number)
    A = np.asarray(allele_number, dtype=np.int64)
    out = (_as_np(an, n, np.uint32), _as_np(sub, int((A * A).sum()), np.uint16), _as_np(prior, int(A.sum()), np.uint16))
    for p in (an, sub, prior):
        L.mrp_free(p)
    return out


def profile_seqs_from_bubbles(allele_number, bubble_reads, supports, n_reads):
    """-> (list of dict(read, ref_start, length, pool_offset), pool bytes)"""
    L = load()
    b, _keep = _bubbles_struct(allele_number, bubble_reads, supports)
    seqs = C.POINTER(ReadRec)()
    read_of = C.c_void_p()
    n_seqs, pool_bytes = C.c_int64(0), C.c_int64(0)
    pool = C.c_void_p()
    _check(L.mrp_profile_seqs_from_bubbles(C.byref(b), n_reads, None, None, C.byref(seqs), C.byref(read_of), C.byref(n_seqs),
                                           C.byref(pool), C.byref(pool_bytes)))
    ro = _as_np(read_of, n_seqs.value, np.int32)
    out = [dict(read=int(ro[i]), ref_start=int(seqs[i].ref_start), length=int(seqs[i].length), pool_offset=int(seqs[i].pool_offset))
           for i in range(n_seqs.value)]
    pb = _as_np(pool, pool_bytes.value, np.uint8)
    L.mrp_free(seqs)
    L.mrp_free(read_of)
    L.mrp_free(pool)
    return out, pb


def assign_reads_to_haplotypes(allele_number, pool, recs, n_reads, gf: dict, min_phred: int):
    """gf: dict(ref_start, length, hap1, hap2 (uint64 arrays), reads1, reads2) -> (hap int8[n_reads], phred f64[n_reads])"""
    L = load()
    an = np.ascontiguousarray(allele_number, dtype=np.uint32)
    pl = np.ascontiguousarray(pool, dtype=np.uint8)
    h1 = np.ascontiguousarray(gf["hap1"], dtype=np.uint64)
    h2 = np.ascontiguousarray(gf["hap2"], dtype=np.uint64)
    r1 = np.ascontiguousarray(gf["reads1"], dtype=np.int32)
    r2 = np.ascontiguousarray(gf["reads2"], dtype=np.int32)
    g = PhaseResult()
    g.ref_start, g.length = int(gf["ref_start"]), int(gf["length"])
    g.haplotype_string1 = C.cast(h1.ctypes.data, type(g.haplotype_string1))
    g.haplotype_string2 = C.cast(h2.ctypes.data, type(g.haplotype_string2))
    g.reads1 = C.cast(r1.ctypes.data, type(g.reads1))
    g.reads2 = C.cast(r2.ctypes.data, type(g.reads2))
    g.n_reads1, g.n_reads2 = len(r1), len(r2)
    hap = np.zeros(n_reads, dtype=np.int8)
    phred = np.zeros(n_reads, dtype=np.float64)
    _check(L.mrp_assign_reads_to_haplotypes(len(an), an.ctypes.data, pl.ctypes.data, recs, n_reads, C.byref(g), int(min_phred),
                                            hap.ctypes.data, phred.ctypes.data))
    return hap, phred


class Stitch:
    def __init__(self):
        self.h = C.c_void_p()
        _check(load().mrp_stitch_create(C.byref(self.h)))

    def chunk(self, hap1: dict, hap2: dict, primary_only=False, do_not_switch=False):
        def pack(d):
            names = [k.encode() for k in d]
            arr = (C.c_char_p * max(len(names), 1))(*names)
            pr = np.ascontiguousarray(list(d.values()), dtype=np.float64)
            return arr, pr, names
        a1, p1, k1 = pack(hap1)
        a2, p2, k2 = pack(hap2)
        sw = C.c_int(0)
        counts = np.zeros(4, dtype=np.int64)
        _check(load().mrp_stitch_chunk(self.h, len(hap1), a1, p1.ctypes.data, len(hap2), a2, p2.ctypes.data, int(primary_only),
                                       int(do_not_switch), C.byref(sw), counts.ctypes.data))
        return bool(sw.value), tuple(int(x) for x in counts)

    def lookup(self, hap: int, name: str):
        p = C.c_double(0)
        return p.value if load().mrp_stitch_lookup(self.h, hap, name.encode(), C.byref(p)) else None

    def size(self, hap: int) -> int:
        return int(load().mrp_stitch_size(self.h, hap))

    def close(self):
        if self.h:
            load().mrp_stitch_destroy(self.h)
            self.h = None


def phase_sets(variants, min_spanning, min_binomial, max_discordant):
    """variants: list of dict(pos, gt1, gt2, alleleIdxToReads=[iterable of read ids per allele]) -> [(phase_set, reason code)]"""
    L = load()
    n = len(variants)
    arr = (Variant * max(n, 1))()
    keep = []
    for i, v in enumerate(variants):
        sets = [sorted(s) for s in v["alleleIdxToReads"]]
        off = np.zeros(len(sets) + 1, dtype=np.int64)
        for a, s_ in enumerate(sets):
            off[a + 1] = off[a] + len(s_)
        rd = np.ascontiguousarray([x for s_ in sets for x in s_], dtype=np.int32)
        keep.append((off, rd))
        arr[i].pos, arr[i].gt1, arr[i].gt2, arr[i].n_alleles = v["pos"], v["gt1"], v["gt2"], len(sets)
        arr[i].allele_read_off, arr[i].allele_reads = off.ctypes.data, rd.ctypes.data
    ps = np.zeros(n, dtype=np.int32)
    rs = np.zeros(n, dtype=np.int32)
    _check(L.mrp_phase_sets(n, arr, int(min_spanning), float(min_binomial), float(max_discordant), ps.ctypes.data, rs.ctypes.data))
    return [(int(ps[i]), int(rs[i])) for i in range(n)]


# ---- read x allele alignment likelihoods (pair-HMM forward probability) ----

def symbols_from_chars(seq) -> np.ndarray:
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    out = np.zeros(len(b), dtype=np.uint8)
    load().mrp_symbols_from_chars(b, len(b), out.ctypes.data)
    return out


def band_diagonals(anchors, lx: int, ly: int, expansion: int):
    a = np.ascontiguousarray(np.asarray(anchors, dtype=np.int64).reshape(-1, 2))
    lo, hi = np.zeros(lx + ly + 1, dtype=np.int32), np.zeros(lx + ly + 1, dtype=np.int32)
    _check(load().mrp_band_diagonals(a.ctypes.data if len(a) else None, len(a), lx, ly, expansion, lo.ctypes.data, hi.ctypes.data))
    return lo, hi


def pair_diagonal_width(anchors, lx: int, ly: int, expansion: int):
    """mrp_pair_diagonal_width (host only) -> (cells on the widest diagonal, dp cells inside the band): what decides a pair's kernel"""
    a = np.ascontiguousarray(np.asarray(anchors if anchors is not None else [], dtype=np.int64).reshape(-1, 2))
    width, cells = C.c_int32(), C.c_int64()
    _check(load().mrp_pair_diagonal_width(a.ctypes.data if len(a) else None, len(a), lx, ly, expansion, C.byref(width), C.byref(cells)))
    return width.value, cells.value


def _opt(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


def forward_probabilities(ctx: Context, models, pool, x_off, x_len, y_off, y_len, model_index=None, anchor_off=None, anchors=None,
                          expansion: int = 4, ragged_left: bool = False, ragged_right: bool = False):
    """computeForwardProbability for a batch of pairs -> (float64 [n_pairs], PairHmmStats)"""
    arr = (PairHmm * len(models))(*models)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    xo, xl, yo, yl = _opt(x_off, np.int64), _opt(x_len, np.int32), _opt(y_off, np.int64), _opt(y_len, np.int32)
    mi, ao, an = _opt(model_index, np.uint8), _opt(anchor_off, np.int64), _opt(anchors, np.int64)
    n = len(xo)
    out = np.zeros(n, dtype=np.float64)
    st = PairHmmStats()
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    _check(load().mrp_forward_probabilities(ctx.h, C.cast(arr, C.c_void_p), len(models), n, ptr(pool), pool.size, ptr(xo), ptr(xl), ptr(yo), ptr(yl),
                                            ptr(mi), None if ao is None else ao.ctypes.data, ptr(an), int(expansion), int(ragged_left),
                                            int(ragged_right), ptr(out), C.byref(st)))
    return out, st


def posterior_tracebacks(anchors, lx: int, ly: int, options: PosteriorOptions) -> np.ndarray:
    """mrp_posterior_tracebacks (host only): int64 [n, 3] (d, tracedBackTo, tracedBackFrom), impl/pairwiseAligner.c:746-749,768,819"""
    a = np.ascontiguousarray(np.asarray(anchors if anchors is not None else [], dtype=np.int64).reshape(-1, 2))
    out = np.zeros((lx + ly + 1, 3), dtype=np.int64)
    n = C.c_int64()
    _check(load().mrp_posterior_tracebacks(a.ctypes.data if len(a) else None, len(a), lx, ly, C.byref(options), out.ctypes.data, len(out), C.byref(n)))
    return out[:n.value].copy()


def _anchor_arrays(anchors, anchor_expansion):
    a = np.ascontiguousarray(np.asarray(anchors if anchors is not None else [], dtype=np.int64).reshape(-1, 2))
    e = np.ascontiguousarray(np.asarray(anchor_expansion if anchor_expansion is not None else [], dtype=np.int64).reshape(-1))
    if len(a) != len(e):
        raise ValueError("one expansion per anchor")
    return a, e


def band_diagonals_dynamic(anchors, lx: int, ly: int, anchor_expansion):
    """mrp_band_diagonals_dynamic (host only): band_constructDynamic, impl/pairwiseAligner.c:120-173, one expansion per anchor"""
    a, e = _anchor_arrays(anchors, anchor_expansion)
    lo, hi = np.zeros(lx + ly + 1, dtype=np.int32), np.zeros(lx + ly + 1, dtype=np.int32)
    _check(load().mrp_band_diagonals_dynamic(a.ctypes.data if len(a) else None, len(a), lx, ly, e.ctypes.data if len(e) else None, lo.ctypes.data, hi.ctypes.data))
    return lo, hi


def pair_diagonal_width_dynamic(anchors, lx: int, ly: int, anchor_expansion):
    """mrp_pair_diagonal_width_dynamic (host only) -> (cells on the widest diagonal, cells inside the dynamic band)"""
    a, e = _anchor_arrays(anchors, anchor_expansion)
    width, cells = C.c_int32(), C.c_int64()
    _check(load().mrp_pair_diagonal_width_dynamic(a.ctypes.data if len(a) else None, len(a), lx, ly, e.ctypes.data if len(e) else None, C.byref(width),
                                                  C.byref(cells)))
    return width.value, cells.value


def posterior_tracebacks_dynamic(anchors, anchor_expansion, lx: int, ly: int, options: PosteriorOptions) -> np.ndarray:
    """mrp_posterior_tracebacks_dynamic (host only): posterior_tracebacks over the dynamic band; options.expansion stays the scalar of :748"""
    a, e = _anchor_arrays(anchors, anchor_expansion)
    out = np.zeros((lx + ly + 1, 3), dtype=np.int64)
    n = C.c_int64()
    _check(load().mrp_posterior_tracebacks_dynamic(a.ctypes.data if len(a) else None, e.ctypes.data if len(e) else None, len(a), lx, ly, C.byref(options),
                                                   out.ctypes.data, len(out), C.byref(n)))
    return out[:n.value].copy()


def posterior_aligned_pairs(ctx, models, pool, x_off, x_len, y_off, y_len, model_index=None, anchor_off=None, anchors=None,
                            options: PosteriorOptions = None, want_total: bool = True, anchor_expansion=None, dynamic: bool = False):
    """getPosteriorProbsWithBanding for a batch of pairs (mrp_posterior_aligned_pairs) -> (match, gap_x, gap_y, total, PairHmmStats):
    each list a dict of first / x / y / weight / log_posterior in the reference's order of generation, gap_x and gap_y None without
    options.with_gaps.  ctx may be None (the checks that need no device).  dynamic (or anchor_expansion given):
    mrp_posterior_aligned_pairs_dynamic, the band of band_constructDynamic with one expansion per anchor."""
    options = options if options is not None else PosteriorOptions()
    dynamic = dynamic or anchor_expansion is not None
    ae = _opt(anchor_expansion if anchor_expansion is not None else [], np.int64)
    arr = (PairHmm * len(models))(*models)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    xo, xl, yo, yl = _opt(x_off, np.int64), _opt(x_len, np.int32), _opt(y_off, np.int64), _opt(y_len, np.int32)
    mi, ao, an = _opt(model_index, np.uint8), _opt(anchor_off, np.int64), _opt(anchors, np.int64)
    n = len(xo)
    total = np.zeros(n, dtype=np.float64) if want_total else None
    st = PairHmmStats()
    lists = [PosteriorPairs() for _ in range(3 if options.with_gaps else 1)]
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    front = [ctx.h if ctx is not None else None, C.cast(arr, C.c_void_p), len(models), n, ptr(pool), pool.size, ptr(xo), ptr(xl), ptr(yo), ptr(yl), ptr(mi),
             None if ao is None else ao.ctypes.data, ptr(an)]
    back = [C.byref(options), C.byref(lists[0]), C.byref(lists[1]) if options.with_gaps else None, C.byref(lists[2]) if options.with_gaps else None,
            ptr(total), C.byref(st)]
    if dynamic:  # anchor_expansion behind anchors
        _check(load().mrp_posterior_aligned_pairs_dynamic(*front, ptr(ae), *back))
    else:
        _check(load().mrp_posterior_aligned_pairs(*front, *back))
    out = [l.to_numpy(n) for l in lists]
    for l in lists:
        load().mrp_posterior_pairs_free(C.byref(l))
    return out[0], (out[1] if options.with_gaps else None), (out[2] if options.with_gaps else None), total, st


# ---- run-length emissions (rleNucleotideEmissions_construct, impl/stateMachine.c:716-752) ----

def rle_compress(seq, max_repeat: int):
    """mrp_rle_compress (host only): rleString_construct + the count clamp -> (symbols uint8, counts uint8), one entry per run"""
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    sym, cnt = np.zeros(len(b), dtype=np.uint8), np.zeros(len(b), dtype=np.uint8)
    n = load().mrp_rle_compress(b, len(b), int(max_repeat), sym.ctypes.data, cnt.ctypes.data)
    if n < 0:
        raise ValueError("mrp_rle_compress: bad arguments")
    return sym[:n].copy(), cnt[:n].copy()


def _repeat_array(repeat):
    """the mrp_repeat_model array of a list of RepeatModel (None: a NULL array); the caller keeps `repeat` alive during the call"""
    if repeat is None:
        return None
    return (RepeatModelStruct * len(repeat))(*[r.struct() for r in repeat])


def forward_probabilities_rle(ctx, models, repeat, pool, counts, x_off, x_len, y_off, y_len, model_index=None, anchor_off=None, anchors=None,
                              expansion: int = 4, ragged_left: bool = False, ragged_right: bool = False):
    """mrp_forward_probabilities_rle: forward_probabilities with run-length emissions; repeat one RepeatModel per model, counts uint8
    parallel to pool (None: a NULL array).  ctx may be None (the checks that need no device)."""
    arr = (PairHmm * len(models))(*models)
    rarr = _repeat_array(repeat)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    cnt = _opt(counts, np.uint8)
    xo, xl, yo, yl = _opt(x_off, np.int64), _opt(x_len, np.int32), _opt(y_off, np.int64), _opt(y_len, np.int32)
    mi, ao, an = _opt(model_index, np.uint8), _opt(anchor_off, np.int64), _opt(anchors, np.int64)
    n = len(xo)
    out = np.zeros(n, dtype=np.float64)
    st = PairHmmStats()
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    _check(load().mrp_forward_probabilities_rle(ctx.h if ctx is not None else None, C.cast(arr, C.c_void_p), None if rarr is None else C.cast(rarr, C.c_void_p),
                                                len(models), n, ptr(pool), None if cnt is None else cnt.ctypes.data, pool.size, ptr(xo), ptr(xl), ptr(yo), ptr(yl),
                                                ptr(mi), None if ao is None else ao.ctypes.data, ptr(an), int(expansion), int(ragged_left), int(ragged_right),
                                                out.ctypes.data, C.byref(st)))
    return out, st


def posterior_aligned_pairs_rle(ctx, models, repeat, pool, counts, x_off, x_len, y_off, y_len, model_index=None, anchor_off=None, anchors=None,
                                options: PosteriorOptions = None, want_total: bool = True, anchor_expansion=None):
    """mrp_posterior_aligned_pairs_rle -> as posterior_aligned_pairs; anchor_expansion None: the band of band_construct over
    options.expansion, else the dynamic band"""
    options = options if options is not None else PosteriorOptions()
    ae = _opt(anchor_expansion, np.int64)
    arr = (PairHmm * len(models))(*models)
    rarr = _repeat_array(repeat)
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    cnt = _opt(counts, np.uint8)
    xo, xl, yo, yl = _opt(x_off, np.int64), _opt(x_len, np.int32), _opt(y_off, np.int64), _opt(y_len, np.int32)
    mi, ao, an = _opt(model_index, np.uint8), _opt(anchor_off, np.int64), _opt(anchors, np.int64)
    n = len(xo)
    total = np.zeros(n, dtype=np.float64) if want_total else None
    st = PairHmmStats()
    lists = [PosteriorPairs() for _ in range(3 if options.with_gaps else 1)]
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    _check(load().mrp_posterior_aligned_pairs_rle(
        ctx.h if ctx is not None else None, C.cast(arr, C.c_void_p), None if rarr is None else C.cast(rarr, C.c_void_p), len(models), n, ptr(pool),
        None if cnt is None else cnt.ctypes.data, pool.size, ptr(xo), ptr(xl), ptr(yo), ptr(yl), ptr(mi), None if ao is None else ao.ctypes.data, ptr(an),
        None if ae is None else ae.ctypes.data, C.byref(options), C.byref(lists[0]), C.byref(lists[1]) if options.with_gaps else None,
        C.byref(lists[2]) if options.with_gaps else None, ptr(total), C.byref(st)))
    out = [l.to_numpy(n) for l in lists]
    for l in lists:
        load().mrp_posterior_pairs_free(C.byref(l))
    return out[0], (out[1] if options.with_gaps else None), (out[2] if options.with_gaps else None), total, st


def rle_expand(symbols, counts) -> str:
    """mrp_rle_expand (host only): rleString_expand; counts uint8 (mrp_rle_compress') or int32 (repeat_count_out)"""
    sym = np.ascontiguousarray(symbols, dtype=np.uint8)
    cnt = np.ascontiguousarray(counts)
    if cnt.dtype != np.uint8:
        cnt = cnt.astype(np.int32)
    c8, c32 = (cnt.ctypes.data, None) if cnt.dtype == np.uint8 else (None, cnt.ctypes.data)
    n = load().mrp_rle_expand(sym.ctypes.data, c8, c32, len(sym), None, 0)
    if n < 0:
        raise ValueError("mrp_rle_expand: bad arguments")
    out = C.create_string_buffer(max(int(n), 1))
    if load().mrp_rle_expand(sym.ctypes.data, c8, c32, len(sym), out, n) != n:
        raise ValueError("mrp_rle_expand: bad arguments")
    return out.raw[:n].decode()


def ml_repeat_counts(ctx, log_prob, node_first, symbols, read_first, counts, y_off, y_len, read_forward_strand, matches, x_shift=None, read_in_hap=None,
                     walk_backwards=False, log_het_substitution=0.0, max_repeat=None, want_log_prob=True, reserved=0, reserved2=0, nulls=()):
    """mrp_ml_repeat_counts -> (repeat_count int32 [nodes], log_prob float64 [nodes] or None, non_rle_length int64 [consensus],
    RepeatCountStats).  log_prob float64 [4, R, R]; matches a dict with first, x, y, weight as posterior_aligned_pairs_rle returns it (pair
    i is read i).  ctx may be None (the checks that need no device); nulls names arguments to pass as NULL (for those checks).  The
    outputs are pre-filled with -7 and must come back untouched from an error."""
    table = np.ascontiguousarray(log_prob, dtype=np.float64)
    R = int(max_repeat if max_repeat is not None else table.shape[-1])
    nf, rf = np.ascontiguousarray(node_first, dtype=np.int64), np.ascontiguousarray(read_first, dtype=np.int64)
    sym, cnt = np.ascontiguousarray(symbols, dtype=np.uint8), np.ascontiguousarray(counts, dtype=np.uint8)
    yo, yl, sd = np.ascontiguousarray(y_off, dtype=np.int64), np.ascontiguousarray(y_len, dtype=np.int32), np.ascontiguousarray(read_forward_strand, dtype=np.uint8)
    xs, hap = _opt(x_shift, np.int32), _opt(read_in_hap, np.uint8)
    first = np.ascontiguousarray(matches["first"], dtype=np.int64)
    mx, my, mw = (np.ascontiguousarray(matches[k], dtype=np.int32) for k in ("x", "y", "weight"))
    ip = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a.size else None
    pairs = PosteriorPairs(None if "first" in nulls else ip(first, C.c_int64), None if "x" in nulls else ip(mx, C.c_int32), ip(my, C.c_int32), ip(mw, C.c_int32), None)
    opt = RepeatCountOptions(int(walk_backwards), int(reserved), float(log_het_substitution), int(reserved2))
    n_cons, n_nodes = len(nf) - 1, len(sym)
    rc_out, lp_out, len_out = np.full(n_nodes, -7, np.int32), np.full(n_nodes, -7.0), np.full(n_cons, -7, np.int64)
    st = RepeatCountStats()
    ptr = lambda name, a: None if a is None or name in nulls else a.ctypes.data
    rc = load().mrp_ml_repeat_counts(ctx.h if ctx is not None else None, ptr("log_prob", table), R, n_cons, ptr("node_first", nf), ptr("symbols", sym),
                                     ptr("read_first", rf), ptr("counts", cnt), cnt.size, ptr("y_off", yo), ptr("y_len", yl), ptr("read_forward_strand", sd),
                                     ptr("x_shift", xs), ptr("read_in_hap", hap), None if "matches" in nulls else C.byref(pairs),
                                     None if "opt" in nulls else C.byref(opt), ptr("repeat_count_out", rc_out), lp_out.ctypes.data if want_log_prob else None,
                                     ptr("non_rle_length_out", len_out), C.byref(st))
    if rc != MRP_OK:
        assert (rc_out == -7).all() and (lp_out == -7.0).all() and (len_out == -7).all() and st.observations == 0, "outputs written on an error"
    _check(rc)
    return rc_out, (lp_out if want_log_prob else None), len_out, st


def _pairs_struct(lst, nulls=(), name=""):
    """a PosteriorPairs over a dict's first / x / y / weight -> (struct, the arrays it points into)"""
    first = np.ascontiguousarray(lst["first"], dtype=np.int64)
    x, y, w = (np.ascontiguousarray(lst[k], dtype=np.int32) for k in ("x", "y", "weight"))
    ip = lambda a, t, k: a.ctypes.data_as(C.POINTER(t)) if a.size and f"{name}.{k}" not in nulls else None
    return PosteriorPairs(ip(first, C.c_int64, "first"), ip(x, C.c_int32, "x"), ip(y, C.c_int32, "y"), ip(w, C.c_int32, "weight"), None), (first, x, y, w)


def poa_augment(ctx, max_repeat, node_first, symbols, ref_counts, read_first, read_symbols, read_counts, y_off, y_len, read_forward_strand, matches, deletes,
                inserts, x_shift=None, compare_repeat_counts=True, merge_ends=True, reference_base_penalty=0.5, want_repeat_count_weight=False, reserved=0,
                reserved2=0, pool_bytes=None, nulls=()):
    """mrp_poa_augment -> a dict of numpy arrays named as mrp_poa's fields (repeat_count_weight None unless asked for) plus n_nodes,
    n_consensus, max_repeat and stats (PoaStats).  The three lists are dicts with first, x, y, weight as posterior_aligned_pairs_rle returns
    them (deletes = its gap-x list, inserts = its gap-y list; pair i is read i).  ctx may be None (the checks that need no device); nulls
    names arguments to pass as NULL ("matches", "matches.first", "deletes.x", ...).  The outputs are pre-filled and must come back
    untouched from an error."""
    nf, rf = np.ascontiguousarray(node_first, dtype=np.int64), np.ascontiguousarray(read_first, dtype=np.int64)
    sym, rcn = np.ascontiguousarray(symbols, dtype=np.uint8), np.ascontiguousarray(ref_counts, dtype=np.uint8)
    rs, rc_ = np.ascontiguousarray(read_symbols, dtype=np.uint8), np.ascontiguousarray(read_counts, dtype=np.uint8)
    yo, yl, sd = np.ascontiguousarray(y_off, dtype=np.int64), np.ascontiguousarray(y_len, dtype=np.int32), np.ascontiguousarray(read_forward_strand, dtype=np.uint8)
    xs = _opt(x_shift, np.int32)
    structs = [_pairs_struct(l, nulls, k) for l, k in ((matches, "matches"), (deletes, "deletes"), (inserts, "inserts"))]
    opt = PoaOptions(int(compare_repeat_counts), int(merge_ends), float(reference_base_penalty), int(want_repeat_count_weight), int(reserved), int(reserved2))
    out, st = Poa(), PoaStats()
    out.n_nodes, st.matches = -7, -7
    ptr = lambda name, a: None if a is None or name in nulls or a.size == 0 else a.ctypes.data
    lp = lambda k, name: None if name in nulls else C.byref(structs[k][0])
    rc = load().mrp_poa_augment(ctx.h if ctx is not None else None, int(max_repeat), len(nf) - 1, None if "node_first" in nulls else nf.ctypes.data,
                                ptr("symbols", sym), ptr("ref_counts", rcn), None if "read_first" in nulls else rf.ctypes.data, ptr("read_symbols", rs),
                                ptr("read_counts", rc_), rs.size if pool_bytes is None else int(pool_bytes), ptr("y_off", yo), ptr("y_len", yl),
                                ptr("read_forward_strand", sd), ptr("x_shift", xs), lp(0, "matches"), lp(1, "deletes"), lp(2, "inserts"),
                                None if "opt" in nulls else C.byref(opt), None if "out" in nulls else C.byref(out), C.byref(st))
    if rc != MRP_OK:
        assert out.n_nodes == -7 and not out.base_weight and not out.totals and st.matches == -7, "outputs written on an error"
    _check(rc)
    n, R, ni, nd, nc = int(out.n_nodes), int(out.max_repeat), int(out.n_inserts), int(out.n_deletes), int(out.n_consensus)
    take = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(k,)).copy() if k else np.zeros(0, dtype=dt)
    res = dict(n_nodes=n, n_consensus=nc, max_repeat=R, stats=st,
               base_weight=take(out.base_weight, 5 * n, np.float64).reshape(n, 5),
               repeat_count_weight=take(out.repeat_count_weight, R * n, np.float64).reshape(n, R) if out.repeat_count_weight else None,
               base_pick=take(out.base_pick, n, np.int32), repeat_count_pick=take(out.repeat_count_pick, n, np.int32),
               insert_first=take(out.insert_first, n + 1, np.int64), insert_str_off=take(out.insert_str_off, ni, np.int64),
               insert_str_len=take(out.insert_str_len, ni, np.int32), insert_weight_forward=take(out.insert_weight_forward, ni, np.float64),
               insert_weight_reverse=take(out.insert_weight_reverse, ni, np.float64), insert_n_observations=take(out.insert_n_observations, ni, np.int64),
               pool_symbols=take(out.pool_symbols, int(out.pool_len), np.uint8), pool_counts=take(out.pool_counts, int(out.pool_len), np.int32),
               delete_first=take(out.delete_first, n + 1, np.int64), delete_length=take(out.delete_length, nd, np.int32),
               delete_weight_forward=take(out.delete_weight_forward, nd, np.float64), delete_weight_reverse=take(out.delete_weight_reverse, nd, np.float64),
               delete_n_observations=take(out.delete_n_observations, nd, np.int64), totals=take(out.totals, 4 * nc, np.float64).reshape(nc, 4))
    load().mrp_poa_free(C.byref(out))
    assert not out.base_weight and out.n_nodes == 0
    return res


def poa_consensus(poa: dict, first_node: int, L: int, use_rle: bool = True, nulls=()):
    """mrp_poa_consensus (host only) for the consensus whose prefix node is first_node (node_first[c] + c) and that has L reference
    positions, over poa_augment's dict (or any dict with those arrays) -> (symbols uint8, counts int32, poa_to_consensus_map int64 [L])"""
    k = int(first_node)
    a = {f: np.ascontiguousarray(poa[f]) for f in ("base_weight", "base_pick", "repeat_count_pick", "insert_first", "insert_str_off", "insert_str_len",
                                                    "insert_weight_forward", "insert_weight_reverse", "pool_symbols", "pool_counts", "delete_first",
                                                    "delete_length", "delete_weight_forward", "delete_weight_reverse")}
    at = lambda f, off=0: None if f in nulls else a[f].ctypes.data + off * a[f].itemsize * (5 if f == "base_weight" else 1)
    so, co, mo, n = C.POINTER(C.c_uint8)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_int64)(), C.c_int64(-7)
    rc = load().mrp_poa_consensus(int(L), at("base_weight", k), at("base_pick", k), at("repeat_count_pick", k), at("insert_first", k), at("insert_str_off"),
                                  at("insert_str_len"), at("insert_weight_forward"), at("insert_weight_reverse"), at("pool_symbols"), at("pool_counts"),
                                  a["pool_symbols"].size, at("delete_first", k), at("delete_length"), at("delete_weight_forward"), at("delete_weight_reverse"),
                                  int(use_rle), C.byref(so), C.byref(co), C.byref(n), C.byref(mo))
    if rc != MRP_OK:
        assert not so and not co and not mo and n.value == -7, "outputs written on an error"
    _check(rc)
    take = lambda p, cnt, dt: np.ctypeslib.as_array(p, shape=(cnt,)).copy() if cnt else np.zeros(0, dtype=dt)
    res = take(so, n.value, np.uint8), take(co, n.value, np.int32), take(mo, int(L), np.int64)
    for p in (so, co, mo):
        load().mrp_free(C.cast(p, C.c_void_p))
    return res


def kmer_alignment_anchors(sx, sy) -> np.ndarray:
    """getKmerAlignmentAnchors (impl/pairwiseAligner.c:1563-1627): int64 [n, 2] (x, y) sequence coordinates"""
    sx = np.ascontiguousarray(sx, dtype=np.uint8)
    sy = np.ascontiguousarray(sy, dtype=np.uint8)
    out = np.zeros((max(len(sy), 1), 2), dtype=np.int64)
    n = load().mrp_kmer_alignment_anchors(sx.ctypes.data if sx.size else None, sx.size, sy.ctypes.data if sy.size else None, sy.size, out.ctypes.data)
    return out[:n].copy()


def kmer_alignment_anchors_many(ctx: Optional[Context], pool, x_off, x_len, y_off, y_len, nulls=()):
    """mrp_kmer_alignment_anchors_many: getKmerAlignmentAnchors of every pair on the device -> (anchor_off int64 [n + 1], anchors int64
    [total, 2], PairHmmStats).  ctx None passes a NULL context; nulls names arguments to pass as NULL (for the argument checks)."""
    L = load()
    pool = np.ascontiguousarray(pool, dtype=np.uint8)
    xo, xl, yo, yl = _opt(x_off, np.int64), _opt(x_len, np.int32), _opt(y_off, np.int64), _opt(y_len, np.int32)
    n = len(xo)
    off = np.full(n + 1, -7, dtype=np.int64)
    res = C.c_void_p()
    st = PairHmmStats()
    ptr = lambda name, a: None if name in nulls or a.size == 0 else a.ctypes.data
    rc = L.mrp_kmer_alignment_anchors_many(ctx.h if ctx else None, n, ptr("pool", pool), pool.size, ptr("x_off", xo), ptr("x_len", xl), ptr("y_off", yo),
                                           ptr("y_len", yl), None if "anchor_off" in nulls else off.ctypes.data,
                                           None if "anchors" in nulls else C.byref(res), C.byref(st))
    if rc != MRP_OK:
        assert res.value is None and (off == -7).all(), "outputs written on an error"
    _check(rc)
    total = int(off[n])
    anchors = _as_np(res, 2 * total, np.int64).reshape(total, 2)
    L.mrp_free(res)
    return off, anchors, st


def allele_read_supports(ctx: Context, forward_model: PairHmm, reverse_model: PairHmm, bubbles, expansion: int = 4, sv_threshold: int = 512):
    """bubbles: list of (alleles, reads, read_forward_strand) with alleles / reads lists of uint8 symbol arrays.
    Returns ([float32 array [n_alleles, n_reads] per bubble], PairHmmStats): Bubble.alleleReadSupports (bubbleGraph.c:1421-1464)."""
    strings, a_first, r_first, a_len, r_len, strand = [], [0], [0], [], [], []
    a_off, r_off, pos = [], [], 0
    for alleles, reads, fwd in bubbles:
        for a in alleles:
            a = np.ascontiguousarray(a, dtype=np.uint8)
            strings.append(a); a_off.append(pos); a_len.append(len(a)); pos += len(a)
        for r in reads:
            r = np.ascontiguousarray(r, dtype=np.uint8)
            strings.append(r); r_off.append(pos); r_len.append(len(r)); pos += len(r)
        strand.extend(int(bool(x)) for x in fwd)
        a_first.append(len(a_off))
        r_first.append(len(r_off))
    pool = np.concatenate(strings) if strings else np.zeros(0, dtype=np.uint8)
    af, rf = np.array(a_first, dtype=np.int64), np.array(r_first, dtype=np.int64)
    ao, al = np.array(a_off, dtype=np.int64), np.array(a_len, dtype=np.int32)
    ro, rl = np.array(r_off, dtype=np.int64), np.array(r_len, dtype=np.int32)
    sd = np.array(strand, dtype=np.uint8)
    sizes = [(af[b + 1] - af[b]) * (rf[b + 1] - rf[b]) for b in range(len(bubbles))]
    sup = np.zeros(int(sum(sizes)), dtype=np.float32)
    st = PairHmmStats()
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    _check(load().mrp_allele_read_supports(ctx.h, C.byref(forward_model), C.byref(reverse_model), len(bubbles), af.ctypes.data, rf.ctypes.data,
                                           ptr(pool), pool.size, ptr(ao), ptr(al), ptr(ro), ptr(rl), ptr(sd), int(expansion), int(sv_threshold), ptr(sup), C.byref(st)))
    out, p = [], 0
    for b, sz in enumerate(sizes):
        out.append(sup[p:p + int(sz)].reshape(int(af[b + 1] - af[b]), int(rf[b + 1] - rf[b])))
        p += int(sz)
    return out, st


def rle_lane_caps(n_models: int):
    """mrp_rle_lane_caps (host only) -> ([cap of launch class 0..3], count bound): the longest x string of the pair-per-lane kernel's launch
    classes for a run-length batch of n_models models (-1: no row fits) and the bound every count of an eligible pair lies below"""
    cap = np.zeros(4, dtype=np.int32)
    bound = C.c_int32(0)
    _check(load().mrp_rle_lane_caps(int(n_models), cap.ctypes.data, C.byref(bound)))
    return [int(c) for c in cap], int(bound.value)


def allele_read_supports_rle(ctx, forward_model: PairHmm, reverse_model: PairHmm, forward_repeat, reverse_repeat, bubbles, expansion: int = 4):
    """mrp_allele_read_supports_rle: bubbles a list of (alleles, allele_counts, reads, read_counts, read_forward_strand), alleles / reads lists
    of uint8 symbol arrays and the counts lists of uint8 arrays parallel to them; forward_repeat / reverse_repeat a RepeatModel each.
    Returns ([float32 array [n_alleles, n_reads] per bubble], PairHmmStats): Bubble.alleleReadSupports of the polish loops
    (bubbleGraph.c:1028-1075, :1193-1244).  ctx may be None (the checks that need no device)."""
    strings, cnts, a_first, r_first, a_len, r_len, strand = [], [], [0], [0], [], [], []
    a_off, r_off, pos = [], [], 0
    for alleles, allele_counts, reads, read_counts, fwd in bubbles:
        for a, c in zip(alleles, allele_counts):
            a = np.ascontiguousarray(a, dtype=np.uint8)
            strings.append(a); cnts.append(np.ascontiguousarray(c, dtype=np.uint8)); a_off.append(pos); a_len.append(len(a)); pos += len(a)
        for r, c in zip(reads, read_counts):
            r = np.ascontiguousarray(r, dtype=np.uint8)
            strings.append(r); cnts.append(np.ascontiguousarray(c, dtype=np.uint8)); r_off.append(pos); r_len.append(len(r)); pos += len(r)
        strand.extend(int(bool(x)) for x in fwd)
        a_first.append(len(a_off))
        r_first.append(len(r_off))
    pool = np.concatenate(strings) if strings else np.zeros(0, dtype=np.uint8)
    counts = np.concatenate(cnts) if cnts else np.zeros(0, dtype=np.uint8)
    assert counts.size == pool.size, "counts must be parallel to the symbols"
    af, rf = np.array(a_first, dtype=np.int64), np.array(r_first, dtype=np.int64)
    ao, al = np.array(a_off, dtype=np.int64), np.array(a_len, dtype=np.int32)
    ro, rl = np.array(r_off, dtype=np.int64), np.array(r_len, dtype=np.int32)
    sd = np.array(strand, dtype=np.uint8)
    sizes = [(af[b + 1] - af[b]) * (rf[b + 1] - rf[b]) for b in range(len(bubbles))]
    sup = np.zeros(int(sum(sizes)), dtype=np.float32)
    st = PairHmmStats()
    fr, rr = forward_repeat.struct(), reverse_repeat.struct()
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    _check(load().mrp_allele_read_supports_rle(ctx.h if ctx is not None else None, C.byref(forward_model), C.byref(reverse_model), C.byref(fr), C.byref(rr),
                                               len(bubbles), af.ctypes.data, rf.ctypes.data, ptr(pool), ptr(counts), pool.size, ptr(ao), ptr(al), ptr(ro), ptr(rl),
                                               ptr(sd), int(expansion), ptr(sup), C.byref(st)))
    out, p = [], 0
    for b, sz in enumerate(sizes):
        out.append(sup[p:p + int(sz)].reshape(int(af[b + 1] - af[b]), int(rf[b + 1] - rf[b])))
        p += int(sz)
    return out, st


def _haptag_sites(sites):
    """sites: list of (alleles, (i, j), entries): alleles a list of uint8 symbol arrays, (i, j) the two compared allele
    indices, entries a list of (read index, uint8 symbol array) in the order of the chunk's reads.
    Returns (HaptagSites, the arrays it points into)."""
    strings, a_first, e_first, a_off, a_len, cmp_, e_read, e_off, e_len, pos = [], [0], [0], [], [], [], [], [], [], 0
    for alleles, (i, j), entries in sites:
        for a in alleles:
            a = np.ascontiguousarray(a, dtype=np.uint8)
            strings.append(a); a_off.append(pos); a_len.append(len(a)); pos += len(a)
        for r, sub in entries:
            sub = np.ascontiguousarray(sub, dtype=np.uint8)
            strings.append(sub); e_read.append(int(r)); e_off.append(pos); e_len.append(len(sub)); pos += len(sub)
        cmp_ += [int(i), int(j)]
        a_first.append(len(a_off))
        e_first.append(len(e_off))
    keep = [np.concatenate(strings) if pos else np.zeros(0, dtype=np.uint8), np.array(a_first, dtype=np.int64), np.array(a_off, dtype=np.int64),
            np.array(a_len, dtype=np.int32), np.array(cmp_, dtype=np.int32), np.array(e_first, dtype=np.int64), np.array(e_read, dtype=np.int64),
            np.array(e_off, dtype=np.int64), np.array(e_len, dtype=np.int32)]
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    S = HaptagSites(len(sites), ptr(keep[0]), keep[0].size, *[ptr(a) for a in keep[1:]])
    return S, keep


def partition_reads_by_haplotype(ctx: Context, forward_model: PairHmm, reverse_model: PairHmm, sites, n_reads: int, read_forward_strand,
                                 expansion: int = 4):
    """bubbleGraph_partitionFilteredReadsFromVcfEntries (bubbleGraph.c:1749-1943) for the sites of any number of chunks; sites as
    _haptag_sites takes them, (i, j) = (hap1, hap2) allele.  Returns (hap int32 [n_reads]: 1, 2 or 0, h1, h2, PairHmmStats)."""
    S, keep = _haptag_sites(sites)
    return _partition_reads(ctx, forward_model, reverse_model, S, n_reads, read_forward_strand, expansion)


def _partition_reads(ctx, forward_model, reverse_model, S: HaptagSites, n_reads: int, read_forward_strand, expansion: int):
    sd = np.ascontiguousarray(read_forward_strand, dtype=np.uint8).astype(bool).astype(np.uint8)
    assert sd.size == n_reads
    hap, h1, h2 = np.zeros(n_reads, dtype=np.int32), np.zeros(n_reads), np.zeros(n_reads)
    st = PairHmmStats()
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    _check(load().mrp_partition_reads_by_haplotype(ctx.h, C.byref(forward_model), C.byref(reverse_model), C.byref(S), int(n_reads), ptr(sd),
                                                   int(expansion), ptr(hap), ptr(h1), ptr(h2), C.byref(st)))
    return hap, h1, h2, st


def phase_variants_from_tagged_reads(ctx: Context, forward_model: PairHmm, reverse_model: PairHmm, variants, n_reads: int, read_forward_strand,
                                     read_hap, expansion: int = 4, sv_threshold: int = 512):
    """bubbleGraph_phaseVcfEntriesFromHaplotaggedReads (bubbleGraph.c:2140-2351); variants as _haptag_sites takes them, (i, j) = (gt1, gt2);
    read_hap: 1 / 2 tagged, anything else untagged.  Returns (state int32 [n_variants]: VARIANT_*, cis, trans, PairHmmStats)."""
    S, keep = _haptag_sites(variants)
    sd = np.ascontiguousarray(read_forward_strand, dtype=np.uint8).astype(bool).astype(np.uint8)
    rh = np.ascontiguousarray(read_hap, dtype=np.int32)
    assert sd.size == n_reads and rh.size == n_reads
    n = len(variants)
    state, cis, trans = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n)
    st = PairHmmStats()
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    _check(load().mrp_phase_variants_from_tagged_reads(ctx.h, C.byref(forward_model), C.byref(reverse_model), C.byref(S), int(n_reads), ptr(sd),
                                                       ptr(rh), int(expansion), int(sv_threshold), ptr(state), ptr(cis), ptr(trans), C.byref(st)))
    return state, cis, trans, st


# ---- from read and allele strings to haplotypes and HP tags (mrp_phase_string_chunks) ----

def string_chunk_struct(chunk):
    """mrp_string_chunk for a margin_amd.synth.StringChunk; returns (StringChunk, the arrays it points into)"""
    strings, a_first, a_off, a_len, s_first, s_off, s_len, s_read, pos = [], [0], [], [], [0], [], [], [], 0
    for alleles, reads, subs in chunk.bubbles:
        for a in alleles:
            a = np.ascontiguousarray(a, dtype=np.uint8)
            strings.append(a); a_off.append(pos); a_len.append(len(a)); pos += len(a)
        for r, sub in zip(reads, subs):
            sub = np.ascontiguousarray(sub, dtype=np.uint8)
            strings.append(sub); s_off.append(pos); s_len.append(len(sub)); s_read.append(int(r)); pos += len(sub)
        a_first.append(len(a_off))
        s_first.append(len(s_off))
    names = [n.encode() for n in chunk.read_names]
    keep = dict(pool=np.concatenate(strings) if pos else np.zeros(0, np.uint8), allele_first=np.array(a_first, np.int64), allele_off=np.array(a_off, np.int64),
                allele_len=np.array(a_len, np.int32), sub_first=np.array(s_first, np.int64), sub_off=np.array(s_off, np.int64), sub_len=np.array(s_len, np.int32),
                sub_read=np.array(s_read, np.int32), strand=np.ascontiguousarray(chunk.read_forward_strand, dtype=np.uint8),
                names=(C.c_char_p * max(len(names), 1))(*names), name_bytes=names)
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    S = StringChunk(len(chunk.bubbles), len(chunk.read_names), ptr(keep["pool"]), keep["pool"].size, keep["allele_first"].ctypes.data, ptr(keep["allele_off"]),
                    ptr(keep["allele_len"]), keep["sub_first"].ctypes.data, ptr(keep["sub_off"]), ptr(keep["sub_len"]), ptr(keep["sub_read"]),
                    C.cast(keep["names"], C.c_void_p) if names else None, ptr(keep["strand"]))
    return S, keep


def _profile_dict(P) -> dict:
    n = int(P.n_seqs)
    seqs = [dict(name=P.seqs[i].name.decode(), ref_start=int(P.seqs[i].ref_start), length=int(P.seqs[i].length),
                 forward_strand=int(P.seqs[i].forward_strand), pool_offset=int(P.seqs[i].pool_offset)) for i in range(n)]
    return dict(seqs=seqs, read_of_seq=_as_np(P.read_of_seq, n, np.int32), pool=_as_np(P.pool, int(P.pool_bytes), np.uint8))


class StringChunkArgs:
    """the arrays a string-chunk call takes and fills (mrp_phase_string_chunks, mrp_queue_phase_string_chunks), and its results as dicts"""

    def __init__(self, chunks, profiles: bool, structs=None):
        self.chunks, self.n, self.profiles = chunks, len(chunks), profiles
        n = self.n
        self.built = structs if structs is not None else [string_chunk_struct(c) for c in chunks]
        self.arr = (StringChunk * max(n, 1))(*[b[0] for b in self.built])
        self.haps = [np.zeros(len(c.read_names), dtype=np.int8) for c in chunks]
        self.phreds = [np.zeros(len(c.read_names), dtype=np.float64) for c in chunks]
        self.hp = (C.c_void_p * max(n, 1))(*[h.ctypes.data for h in self.haps])
        self.pp = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in self.phreds])
        self.res = (C.POINTER(PhaseResult) * max(n, 1))()
        self.prof = (ProfileOut * max(n, 1))() if profiles else None

    def results(self):
        L = load()
        out = []
        for i in range(self.n):
            d = dict(result=_phase_result_dict(self.res[i].contents), hap=self.haps[i], phred=self.phreds[i])
            L.mrp_phase_result_destroy(self.res[i])
            if self.profiles:
                P = self.prof[i]
                d["profile"] = _profile_dict(P)
                nb = len(self.chunks[i].bubbles)
                an = _as_np(P.allele_number, nb, np.uint32)
                A = an.astype(np.int64)
                d["profile"].update(allele_number=an, sub=_as_np(P.substitution, int((A * A).sum()), np.uint16), prior=_as_np(P.prior, int(A.sum()), np.uint16))
                for f in ("seqs", "read_of_seq", "pool", "allele_number", "substitution", "prior"):
                    L.mrp_free(C.cast(getattr(P, f), C.c_void_p))
            out.append(d)
        return out


def phase_string_chunks(ctx: Context, chunks, forward_model: PairHmm, reverse_model: PairHmm, params: Params, min_phred: int = 0,
                        expansion: int = 4, sv_threshold: int = 512, het_substitution_probability: float = 0.0, profiles: bool = False,
                        structs=None):
    """mrp_phase_string_chunks -> (list per chunk of dict(result, hap, phred[, profile]), StringChunksStats).  result is the
    phase result dict with reads1 / reads2 naming the chunk's reads; profile (profiles=True) holds the profile sequences, pool
    and site tables; structs = [string_chunk_struct(c) for c in chunks] to reuse them (timing loops)."""
    L = load()
    a = StringChunkArgs(chunks, profiles, structs)
    st = StringChunksStats()
    _check(L.mrp_phase_string_chunks(ctx.h, a.n, a.arr, C.byref(forward_model), C.byref(reverse_model), int(expansion), int(sv_threshold),
                                     float(het_substitution_probability), C.byref(params), int(min_phred), a.res, a.hp, a.pp, a.prof, C.byref(st)))
    return a.results(), st


def string_chunk_units(chunk, struct=None) -> int:
    """mrp_string_chunk_units: the (read, bubble) units of one chunk, what the work queue orders and cuts its batches by"""
    S = struct if struct is not None else string_chunk_struct(chunk)
    u = C.c_int64(-1)
    _check(load().mrp_string_chunk_units(C.byref(S[0]), C.byref(u)))
    return int(u.value)


def _queue_phase_string_chunks(q, chunks, forward_model, reverse_model, params, min_phred, chunks_per_batch, expansion, sv_threshold,
                               het_substitution_probability, profiles, structs):
    a = StringChunkArgs(chunks, profiles, structs)
    st = QueueStats()
    _check(load().mrp_queue_phase_string_chunks(q, a.n, a.arr, C.byref(forward_model), C.byref(reverse_model), int(expansion), int(sv_threshold),
                                                float(het_substitution_probability), C.byref(params), int(min_phred), int(chunks_per_batch), a.res,
                                                a.hp, a.pp, a.prof, C.byref(st)))
    return a.results(), st


def phase_string_chunks_on_devices(devices, chunks, forward_model: PairHmm, reverse_model: PairHmm, params: Params, min_phred: int = 0,
                                   chunks_per_batch: int = 0, expansion: int = 4, sv_threshold: int = 512, het_substitution_probability: float = 0.0,
                                   profiles: bool = False, structs=None):
    """mrp_phase_string_chunks_on_devices -> (phase_string_chunks' list of dicts in input order, QueueStats)"""
    a = StringChunkArgs(chunks, profiles, structs)
    dev = (C.c_int32 * len(devices))(*devices)
    st = QueueStats()
    _check(load().mrp_phase_string_chunks_on_devices(C.cast(dev, C.c_void_p), len(devices), a.n, a.arr, C.byref(forward_model), C.byref(reverse_model),
                                                     int(expansion), int(sv_threshold), float(het_substitution_probability), C.byref(params),
                                                     int(min_phred), int(chunks_per_batch), a.res, a.hp, a.pp, a.prof, C.byref(st)))
    return a.results(), st


# ---- the same with the back half: filtered variants phased, filtered reads tagged (mrp_phase_string_chunks_with_filtered) ----

def string_chunk_rest_struct(chunk, rest):
    """mrp_string_chunk_rest beside chunk (a synth.StringChunk).  rest: None (an empty rest) or a dict with
    forward_strand (per filtered read), fsubs (per bubble of the chunk a list of (filtered read, symbols), ascending reads),
    variants (a list of (alleles, (gt1, gt2), entries), entries a list of (read of the chunk, primary or n_reads + filtered, symbols)).
    Returns (StringChunkRest, the arrays it points into)."""
    if rest is None:
        return StringChunkRest(), {}
    strings, pos = [], 0
    f_first, f_off, f_len, f_read = [0], [], [], []
    fsubs = rest.get("fsubs") or [[] for _ in chunk.bubbles]
    assert len(fsubs) == len(chunk.bubbles)
    for subs in fsubs:
        for r, sub in subs:
            sub = np.ascontiguousarray(sub, dtype=np.uint8)
            strings.append(sub); f_off.append(pos); f_len.append(len(sub)); f_read.append(int(r)); pos += len(sub)
        f_first.append(len(f_off))
    a_first, a_off, a_len, gt, e_first, e_read, e_off, e_len = [0], [], [], [], [0], [], [], []
    for alleles, g, entries in rest.get("variants", []):
        for a in alleles:
            a = np.ascontiguousarray(a, dtype=np.uint8)
            strings.append(a); a_off.append(pos); a_len.append(len(a)); pos += len(a)
        for r, sub in entries:
            sub = np.ascontiguousarray(sub, dtype=np.uint8)
            strings.append(sub); e_read.append(int(r)); e_off.append(pos); e_len.append(len(sub)); pos += len(sub)
        gt += [int(g[0]), int(g[1])]
        a_first.append(len(a_off))
        e_first.append(len(e_off))
    keep = dict(strand=np.ascontiguousarray(rest["forward_strand"], dtype=np.uint8), pool=np.concatenate(strings) if pos else np.zeros(0, np.uint8),
                fsub_first=np.array(f_first, np.int64), fsub_off=np.array(f_off, np.int64), fsub_len=np.array(f_len, np.int32),
                fsub_read=np.array(f_read, np.int32), valle_first=np.array(a_first, np.int64), valle_off=np.array(a_off, np.int64),
                valle_len=np.array(a_len, np.int32), gt=np.array(gt, np.int32), ventry_first=np.array(e_first, np.int64),
                ventry_read=np.array(e_read, np.int32), ventry_off=np.array(e_off, np.int64), ventry_len=np.array(e_len, np.int32))
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    R = StringChunkRest(keep["strand"].size, ptr(keep["strand"]), ptr(keep["pool"]), keep["pool"].size, keep["fsub_first"].ctypes.data, ptr(keep["fsub_off"]),
                        ptr(keep["fsub_len"]), ptr(keep["fsub_read"]), len(rest.get("variants", [])), keep["valle_first"].ctypes.data, ptr(keep["valle_off"]),
                        ptr(keep["valle_len"]), ptr(keep["gt"]), keep["ventry_first"].ctypes.data, ptr(keep["ventry_read"]), ptr(keep["ventry_off"]),
                        ptr(keep["ventry_len"]))
    return R, keep


class StringFilteredArgs(StringChunkArgs):
    """StringChunkArgs with the rests and the back half's results"""

    def __init__(self, chunks, rests, profiles: bool, structs=None, rest_structs=None):
        super().__init__(chunks, profiles, structs)
        assert len(rests) == self.n
        self.rbuilt = rest_structs if rest_structs is not None else [string_chunk_rest_struct(c, r) for c, r in zip(chunks, rests)]
        self.rarr = (StringChunkRest * max(self.n, 1))(*[b[0] for b in self.rbuilt])
        self.fout = (FilteredOut * max(self.n, 1))()

    def results(self):
        L = load()
        out = super().results()
        for i, d in enumerate(out):
            O = self.fout[i]
            nr, nv = int(O.n_reads), int(O.n_variants)
            d["filtered"] = dict(read_hap=_as_np(O.read_hap, nr, np.int32), h1=_as_np(O.h1, nr, np.float64), h2=_as_np(O.h2, nr, np.float64),
                                 variant_state=_as_np(O.variant_state, nv, np.int32), cis=_as_np(O.cis, nv, np.float64), trans=_as_np(O.trans, nv, np.float64))
            for f in ("read_hap", "h1", "h2", "variant_state", "cis", "trans"):
                L.mrp_free(C.cast(getattr(O, f), C.c_void_p))
        return out


def phase_string_chunks_with_filtered(ctx: Context, chunks, rests, forward_model: PairHmm, reverse_model: PairHmm, params: Params, min_phred: int = 0,
                                      expansion: int = 4, sv_threshold: int = 512, het_substitution_probability: float = 0.0, profiles: bool = False,
                                      structs=None, rest_structs=None):
    """mrp_phase_string_chunks_with_filtered -> (phase_string_chunks' list of dicts, each with "filtered": dict(read_hap, h1, h2 over the
    chunk's primary then filtered reads, variant_state, cis, trans), StringFilteredStats).  rests as string_chunk_rest_struct takes them."""
    a = StringFilteredArgs(chunks, rests, profiles, structs, rest_structs)
    st = StringFilteredStats()
    _check(load().mrp_phase_string_chunks_with_filtered(ctx.h, a.n, a.arr, a.rarr, C.byref(forward_model), C.byref(reverse_model), int(expansion),
                                                        int(sv_threshold), float(het_substitution_probability), C.byref(params), int(min_phred), a.res,
                                                        a.hp, a.pp, a.prof, a.fout, C.byref(st)))
    return a.results(), st


def queue_phase_string_chunks_with_filtered(q, chunks, rests, forward_model: PairHmm, reverse_model: PairHmm, params: Params, min_phred: int = 0,
                                            chunks_per_batch: int = 0, expansion: int = 4, sv_threshold: int = 512,
                                            het_substitution_probability: float = 0.0, profiles: bool = False, structs=None, rest_structs=None):
    """mrp_queue_phase_string_chunks_with_filtered on a Queue -> (list of dicts in input order, QueueStats)"""
    a = StringFilteredArgs(chunks, rests, profiles, structs, rest_structs)
    st = QueueStats()
    _check(load().mrp_queue_phase_string_chunks_with_filtered(q.h, a.n, a.arr, a.rarr, C.byref(forward_model), C.byref(reverse_model), int(expansion),
                                                              int(sv_threshold), float(het_substitution_probability), C.byref(params), int(min_phred),
                                                              int(chunks_per_batch), a.res, a.hp, a.pp, a.prof, a.fout, C.byref(st)))
    return a.results(), st


def phase_string_chunks_with_filtered_on_devices(devices, chunks, rests, forward_model: PairHmm, reverse_model: PairHmm, params: Params, min_phred: int = 0,
                                                 chunks_per_batch: int = 0, expansion: int = 4, sv_threshold: int = 512,
                                                 het_substitution_probability: float = 0.0, profiles: bool = False):
    """mrp_phase_string_chunks_with_filtered_on_devices -> (list of dicts in input order, QueueStats)"""
    a = StringFilteredArgs(chunks, rests, profiles)
    dev = (C.c_int32 * len(devices))(*devices)
    st = QueueStats()
    _check(load().mrp_phase_string_chunks_with_filtered_on_devices(C.cast(dev, C.c_void_p), len(devices), a.n, a.arr, a.rarr, C.byref(forward_model),
                                                                   C.byref(reverse_model), int(expansion), int(sv_threshold),
                                                                   float(het_substitution_probability), C.byref(params), int(min_phred),
                                                                   int(chunks_per_batch), a.res, a.hp, a.pp, a.prof, a.fout, C.byref(st)))
    return a.results(), st


def phase_string_chunks_chain(ctx: Context, chunks, forward_model: PairHmm, reverse_model: PairHmm, params: Params, min_phred: int = 0,
                              expansion: int = 4, sv_threshold: int = 512, het_substitution_probability: float = 0.0, timing: Optional[dict] = None,
                              profiles: bool = True):
    """The same through the four calls an integrator chains by hand (examples/phase_from_strings.c): mrp_allele_read_supports
    per chunk -> mrp_profile_seqs_from_bubbles + mrp_reference_from_bubbles -> mrp_chunk_create + mrp_phase_reads_many ->
    mrp_assign_reads_to_haplotypes, read indices translated through read_of_seq.  Same return shape as phase_string_chunks
    (profile included unless profiles=False).  timing (optional dict) receives the wall ms of the four steps."""
    import time
    L = load()
    t = [time.perf_counter()]
    prepared = []
    for c in chunks:
        S, keep = string_chunk_struct(c)
        nb = len(c.bubbles)
        sup_sizes = [len(a) * len(r) for a, r, _ in c.bubbles]
        sup = np.zeros(max(sum(sup_sizes), 1), dtype=np.float32)
        ptr = lambda a: None if a.size == 0 else a.ctypes.data
        strand_of_sub = keep["strand"][keep["sub_read"]] if keep["sub_read"].size else np.zeros(0, np.uint8)
        strand_of_sub = np.ascontiguousarray(strand_of_sub, dtype=np.uint8)
        if nb:
            _check(L.mrp_allele_read_supports(ctx.h, C.byref(forward_model), C.byref(reverse_model), nb, keep["allele_first"].ctypes.data,
                                              keep["sub_first"].ctypes.data, ptr(keep["pool"]), keep["pool"].size, ptr(keep["allele_off"]), ptr(keep["allele_len"]),
                                              ptr(keep["sub_off"]), ptr(keep["sub_len"]), ptr(strand_of_sub), int(expansion), int(sv_threshold), sup.ctypes.data, None))
        prepared.append((S, keep, sup))
    t.append(time.perf_counter())
    built = []
    for c, (S, keep, sup) in zip(chunks, prepared):
        nb = len(c.bubbles)
        an = np.diff(keep["allele_first"]).astype(np.uint32)
        nr = np.diff(keep["sub_first"])
        sup_off = np.zeros(nb + 1, dtype=np.int64)
        np.cumsum(an.astype(np.int64) * nr, out=sup_off[1:])
        b = Bubbles(nb, an.ctypes.data if nb else None, keep["sub_first"].ctypes.data, keep["sub_read"].ctypes.data if keep["sub_read"].size else None,
                    sup_off.ctypes.data, sup.ctypes.data)
        fs = keep["strand"].astype(np.int32)
        seqs = C.POINTER(ReadRec)()
        read_of, pool = C.c_void_p(), C.c_void_p()
        n_seqs, pool_bytes = C.c_int64(0), C.c_int64(0)
        _check(L.mrp_profile_seqs_from_bubbles(C.byref(b), len(c.read_names), C.cast(keep["names"], C.c_void_p), fs.ctypes.data if fs.size else None,
                                               C.byref(seqs), C.byref(read_of), C.byref(n_seqs), C.byref(pool), C.byref(pool_bytes)))
        pa, ps, pp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(L.mrp_reference_from_bubbles(C.byref(b), float(het_substitution_probability), C.byref(pa), C.byref(ps), C.byref(pp)))
        built.append(dict(seqs=seqs, read_of=read_of, n_seqs=n_seqs.value, pool=pool, pool_bytes=pool_bytes.value, an=pa, sub=ps, prior=pp, nb=nb))
    t.append(time.perf_counter())
    handles = []
    for d in built:
        h = C.c_void_p()
        _check(L.mrp_chunk_create(ctx.h, d["nb"], d["an"], d["sub"], d["prior"], d["pool"] if d["pool_bytes"] else None, d["pool_bytes"], C.byref(h)))
        handles.append(h)
    n = len(chunks)
    ch = (C.c_void_p * max(n, 1))(*[h.value for h in handles])
    rd = (C.POINTER(ReadRec) * max(n, 1))(*[d["seqs"] for d in built])
    nr = (C.c_int64 * max(n, 1))(*[d["n_seqs"] for d in built])
    res = (C.POINTER(PhaseResult) * max(n, 1))()
    st = PhaseManyStats()
    _check(L.mrp_phase_reads_many(ctx.h, n, ch, rd, nr, C.byref(params), res, C.byref(st)))
    t.append(time.perf_counter())
    out = []
    for i, (c, d) in enumerate(zip(chunks, built)):
        n_reads = len(c.read_names)
        hap_s = np.zeros(max(d["n_seqs"], 1), dtype=np.int8)
        phred_s = np.zeros(max(d["n_seqs"], 1), dtype=np.float64)
        _check(L.mrp_assign_reads_to_haplotypes(d["nb"], d["an"], d["pool"], d["seqs"], d["n_seqs"], res[i], int(min_phred), hap_s.ctypes.data, phred_s.ctypes.data))
        ro = _as_np(d["read_of"], d["n_seqs"], np.int32)
        hap = np.full(n_reads, -1, dtype=np.int8)
        phred = np.zeros(n_reads, dtype=np.float64)
        hap[ro] = hap_s[:d["n_seqs"]]
        phred[ro] = phred_s[:d["n_seqs"]]
        r = _phase_result_dict(res[i].contents)
        r["reads1"] = [int(ro[q]) for q in r["reads1"]]
        r["reads2"] = [int(ro[q]) for q in r["reads2"]]
        L.mrp_phase_result_destroy(res[i])
        if not profiles:
            out.append(dict(result=r, hap=hap, phred=phred))
            continue
        A = _as_np(d["an"], d["nb"], np.uint32)
        A64 = A.astype(np.int64)
        prof = dict(seqs=[dict(name=d["seqs"][q].name.decode(), ref_start=int(d["seqs"][q].ref_start), length=int(d["seqs"][q].length),
                               forward_strand=int(d["seqs"][q].forward_strand), pool_offset=int(d["seqs"][q].pool_offset)) for q in range(d["n_seqs"])],
                    read_of_seq=ro, pool=_as_np(d["pool"], d["pool_bytes"], np.uint8), allele_number=A,
                    sub=_as_np(d["sub"], int((A64 * A64).sum()), np.uint16), prior=_as_np(d["prior"], int(A64.sum()), np.uint16))
        out.append(dict(result=r, hap=hap, phred=phred, profile=prof))
    t.append(time.perf_counter())
    for h in handles:
        L.mrp_chunk_destroy(h)
    for d in built:
        for f in ("seqs", "read_of", "pool", "an", "sub", "prior"):
            L.mrp_free(C.cast(d[f], C.c_void_p))
    if timing is not None:
        timing.update(supports_ms=1e3 * (t[1] - t[0]), profile_ms=1e3 * (t[2] - t[1]), phase_ms=1e3 * (t[3] - t[2]), assign_ms=1e3 * (t[4] - t[3]))
    return out, st


# ---- read substrings at variant sites from alignments (mrp_extract_read_substrings) ----

_EXTRACTED_ARRAYS = (("ref_aln_start", np.int64, "v"), ("ref_aln_stop_incl", np.int64, "v"), ("allele_first", np.int64, "v1"),
                     ("allele_off", np.int64, "a"), ("allele_len", np.int32, "a"), ("read_status", np.uint8, "r"),
                     ("read_n_substrings", np.int32, "r"), ("entry_first", np.int64, "v1"), ("entry_read", np.int32, "e"),
                     ("entry_off", np.int64, "e"), ("entry_len", np.int32, "e"), ("pool", np.uint8, "p"))


def aligned_chunk_struct(chunk):
    """mrp_aligned_chunk for a margin_amd.synth.AlignedChunk; returns (AlignedChunk, the arrays it points into)"""
    chars = [a.encode() for al in chunk.alleles for a in al]
    a_first = np.zeros(len(chunk.alleles) + 1, np.int64)
    np.cumsum([len(al) for al in chunk.alleles], out=a_first[1:])
    a_len = np.array([len(c) for c in chars], np.int32)
    a_off = np.zeros(len(chars), np.int64)
    if len(chars):
        a_off[1:] = np.cumsum(a_len[:-1])
    keep = dict(reference=chunk.reference.encode(), allele_chars=b"".join(chars), variant_pos=np.ascontiguousarray(chunk.variant_pos, np.int64),
                allele_first=a_first, allele_off=a_off, allele_len=a_len, is_sv=np.ascontiguousarray(chunk.is_sv, np.uint8),
                pos=np.ascontiguousarray(chunk.read_pos, np.int64), flag=np.ascontiguousarray(chunk.flag, np.uint16),
                mapq=np.ascontiguousarray(chunk.mapq, np.uint8), l_qseq=np.ascontiguousarray(chunk.l_qseq, np.int32),
                cigar_first=np.ascontiguousarray(chunk.cigar_first, np.int64), cigar=np.ascontiguousarray(chunk.cigar, np.uint32),
                seq_first=np.ascontiguousarray(chunk.seq_first, np.int64), seq=np.ascontiguousarray(chunk.seq, np.uint8))
    keep["ref_buf"] = C.create_string_buffer(keep["reference"], max(len(keep["reference"]), 1))
    keep["chars_buf"] = C.create_string_buffer(keep["allele_chars"], max(len(keep["allele_chars"]), 1))
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    S = AlignedChunk(int(chunk.overlap_start), int(chunk.overlap_end), int(chunk.chunk_start), int(chunk.chunk_end), C.addressof(keep["ref_buf"]),
                     len(keep["reference"]), len(chunk.alleles), ptr(keep["variant_pos"]), keep["allele_first"].ctypes.data, ptr(keep["allele_off"]),
                     ptr(keep["allele_len"]), C.addressof(keep["chars_buf"]), len(keep["allele_chars"]), ptr(keep["is_sv"]), len(keep["pos"]),
                     ptr(keep["pos"]), ptr(keep["flag"]), ptr(keep["mapq"]), ptr(keep["l_qseq"]), keep["cigar_first"].ctypes.data,
                     ptr(keep["cigar"]), keep["seq_first"].ctypes.data, ptr(keep["seq"]))
    return S, keep


def mark_structural_variants(chunk, indel_size: int, struct=None) -> np.ndarray:
    """mrp_mark_structural_variants -> is_sv [n_variants] (uint8): any allele longer than indel_size; none for indel_size <= 0"""
    S, keep = struct if struct is not None else aligned_chunk_struct(chunk)
    out = np.zeros(int(S.n_variants), np.uint8)
    _check(load().mrp_mark_structural_variants(C.byref(S), int(indel_size), out.ctypes.data if out.size else None))
    return out


def extract_read_substrings(ctx: Optional[Context], chunks, options: Optional[dict] = None, structs=None):
    """mrp_extract_read_substrings -> (list per chunk of dict of the mrp_extracted_chunk arrays as numpy, ExtractStats).
    ctx None passes a NULL context (MRP_ERR_NO_DEVICE); structs = [aligned_chunk_struct(c) ...] to reuse them."""
    L = load()
    n = len(chunks)
    built = structs if structs is not None else [aligned_chunk_struct(c) for c in chunks]
    arr = (AlignedChunk * max(n, 1))(*[b[0] for b in built])
    opt = ExtractOptions.from_dict(options or shipped_extract_options())
    out = C.POINTER(ExtractedChunk)()
    st = ExtractStats()
    _check(L.mrp_extract_read_substrings(ctx.h if ctx else None, n, arr, C.byref(opt), C.byref(out), C.byref(st)))
    res = []
    for i in range(n):
        X = out[i]
        nv, nr = int(X.n_variants), int(X.n_reads)
        af = _as_np(X.allele_first, nv + 1, np.int64)
        ef = _as_np(X.entry_first, nv + 1, np.int64)
        size = dict(v=nv, v1=nv + 1, a=int(af[nv]), r=nr, e=int(ef[nv]), p=int(X.pool_bytes))
        d = {f: _as_np(getattr(X, f), size[k], t) for f, t, k in _EXTRACTED_ARRAYS}
        for f, _, _ in _EXTRACTED_ARRAYS:
            L.mrp_free(C.cast(getattr(X, f), C.c_void_p))
        res.append(d)
    L.mrp_free(C.cast(out, C.c_void_p))
    return res, st


def downsample_draw(seed: int, overlap_start: int, overlap_end: int, k: int) -> float:
    """mrp_downsample_draw: the counter-based u_k of a chunk, in [0, 1)"""
    return float(load().mrp_downsample_draw(int(seed) & (2**64 - 1), int(overlap_start), int(overlap_end), int(k)))


def aln_read_lengths(chunk, struct=None) -> np.ndarray:
    """mrp_aln_read_lengths -> alnReadLength per read of the chunk (int32), as the extraction's walk bound computes it"""
    S, keep = struct if struct is not None else aligned_chunk_struct(chunk)
    out = np.zeros(int(S.n_reads), np.int32)
    _check(load().mrp_aln_read_lengths(C.byref(S), out.ctypes.data if out.size else None))
    return out


def downsample_keep_from_extracted(x: dict, aln_read_length, max_depth: int, seed: int, overlap_start: int, overlap_end: int):
    """mrp_downsample_keep_from_extracted -> (keep uint8 [n_reads], prob float64 [n_reads], downsampled bool): the host definition of the
    downsampling to maxDepth over one extract_read_substrings result"""
    X, hold = extracted_struct(x)
    h = np.ascontiguousarray(aln_read_length, np.int32)
    n = int(X.n_reads)
    assert h.size == n
    keep, prob, did = np.zeros(n, np.uint8), np.zeros(n, np.float64), C.c_int32(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    _check(load().mrp_downsample_keep_from_extracted(C.byref(X), ptr(h), int(max_depth), int(seed) & (2**64 - 1), int(overlap_start), int(overlap_end),
                                                     ptr(keep), ptr(prob), C.byref(did)))
    return keep, prob, bool(did.value)


def downsample_reads(ctx: Optional[Context], n_reads, first, l, h, status, V, max_depth: int, seed: int, overlap_start, overlap_end):
    """mrp_downsample_reads, the kernel's seam: many chunks in one launch -> (keep uint8, prob float64, DownsamplingStats), the arrays over
    the n_total = max(first + n_reads) reads of the call.  ctx None passes a NULL context (MRP_ERR_NO_DEVICE)."""
    a64 = lambda a: np.ascontiguousarray(a, np.int64)
    n_reads, first, V, os_, oe = a64(n_reads), a64(first), a64(V), a64(overlap_start), a64(overlap_end)
    l, h, status = np.ascontiguousarray(l, np.int32), np.ascontiguousarray(h, np.int32), np.ascontiguousarray(status, np.uint8)
    n = int(n_reads.size)
    n_total = max(int((first + n_reads).max()), 0) if n else 0
    assert l.size >= n_total and h.size >= n_total and status.size >= n_total
    keep, prob, st = np.zeros(n_total, np.uint8), np.zeros(n_total, np.float64), DownsamplingStats()
    ptr = lambda a: a.ctypes.data if a.size else None
    _check(load().mrp_downsample_reads(ctx.h if ctx else None, n, ptr(n_reads), ptr(first), ptr(l), ptr(h), ptr(status), ptr(V), int(max_depth),
                                       int(seed) & (2**64 - 1), ptr(os_), ptr(oe), ptr(prob), ptr(keep), C.byref(st)))
    return keep, prob, st


def extracted_struct(x: dict):
    """mrp_extracted_chunk over the numpy arrays of one extract_read_substrings result; returns (ExtractedChunk, arrays)"""
    keep = {f: np.ascontiguousarray(x[f], t) for f, t, _ in _EXTRACTED_ARRAYS}
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    X = ExtractedChunk(len(keep["ref_aln_start"]), len(keep["read_status"]), *[ptr(keep[f]) for f, _, _ in _EXTRACTED_ARRAYS], keep["pool"].size)
    return X, keep


def string_chunk_from_extracted(x: dict, read_names, read_forward_strand, keep=None):
    """mrp_string_chunk_from_extracted -> (margin_amd.synth.StringChunk, bubble -> variant int64 array, the raw arrays)"""
    from margin_amd import synth
    L = load()
    X, hold = extracted_struct(x)
    names = [n.encode() for n in read_names]
    name_arr = (C.c_char_p * max(len(names), 1))(*names)
    strand = np.ascontiguousarray(read_forward_strand, np.uint8)
    km = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    S = StringChunk()
    bv = C.POINTER(C.c_int64)()
    _check(L.mrp_string_chunk_from_extracted(C.byref(X), None if km is None else km.ctypes.data, C.cast(name_arr, C.c_void_p),
                                             strand.ctypes.data if strand.size else None, C.byref(S), C.byref(bv)))
    nb = int(S.n_bubbles)
    a_first = _as_np(S.allele_first, nb + 1, np.int64)
    s_first = _as_np(S.sub_first, nb + 1, np.int64)
    raw = dict(allele_first=a_first, allele_off=_as_np(S.allele_off, int(a_first[nb]), np.int64), allele_len=_as_np(S.allele_len, int(a_first[nb]), np.int32),
               sub_first=s_first, sub_off=_as_np(S.sub_off, int(s_first[nb]), np.int64), sub_len=_as_np(S.sub_len, int(s_first[nb]), np.int32),
               sub_read=_as_np(S.sub_read, int(s_first[nb]), np.int32), bubble_variant=_as_np(C.cast(bv, C.c_void_p), nb, np.int64))
    assert S.pool == (hold["pool"].ctypes.data if hold["pool"].size else None) and S.n_reads == len(hold["read_status"])
    L.mrp_free(C.cast(S.allele_first, C.c_void_p))
    pool = hold["pool"]
    bubbles = []
    for b in range(nb):
        al = [pool[o:o + l].copy() for o, l in zip(raw["allele_off"][a_first[b]:a_first[b + 1]], raw["allele_len"][a_first[b]:a_first[b + 1]])]
        ks = range(int(s_first[b]), int(s_first[b + 1]))
        bubbles.append((al, [int(raw["sub_read"][k]) for k in ks], [pool[raw["sub_off"][k]:raw["sub_off"][k] + raw["sub_len"][k]].copy() for k in ks]))
    sc = synth.StringChunk(bubbles=bubbles, read_names=list(read_names), read_forward_strand=strand, hap=np.zeros(len(names), np.int64),
                           truth=[0] * nb)
    return sc, raw["bubble_variant"], raw


class ExtractedRest:
    """What mrp_string_chunk_rest_from_extracted returned for one chunk: struct (the StringChunkRest itself, pointing into the C block: pass
    it on unchanged), filtered_read (int32, the chunk's read index of every filtered read), raw (numpy copies of every array of the
    struct, "pool" and "forward_strand" included) and rest (the same as the dict capi.string_chunk_rest_struct takes; None for the empty
    rest).  The block is released by close()."""

    def __init__(self, struct, block, filtered_read, raw, rest, hold):
        self.struct, self.block, self.filtered_read, self.raw, self.rest, self._hold = struct, block, filtered_read, raw, rest, hold

    def close(self):
        if self.block is not None:
            load().mrp_free(self.block)
            self.block = None

    def __del__(self):
        self.close()


def string_chunk_rest_from_extracted(x: dict, xf: dict, read_forward_strand, bubble_variant, fvariant_pos, gt, chunk_start: int, chunk_end: int,
                                     keep=None, nulls=()) -> ExtractedRest:
    """mrp_string_chunk_rest_from_extracted over two extract_read_substrings results (x: the primary variants, xf: the same reads over the
    filtered variants); gt: int32 [n, 2] or flat.  nulls names arguments to pass as NULL (for the argument checks)."""
    L = load()
    X, hold_x = extracted_struct(x)
    XF, hold_f = extracted_struct(xf)
    strand = np.ascontiguousarray(read_forward_strand, np.uint8)
    km = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    bv = np.ascontiguousarray(bubble_variant, np.int64)
    fpos = np.ascontiguousarray(fvariant_pos, np.int64)
    g = np.ascontiguousarray(gt, np.int32).reshape(-1)
    ptr = lambda name, a: None if a is None or name in nulls or a.size == 0 else a.ctypes.data
    R = StringChunkRest()
    fr, blk = C.c_void_p(), C.c_void_p()
    _check(L.mrp_string_chunk_rest_from_extracted(None if "x" in nulls else C.byref(X), ptr("keep", km), ptr("strand", strand), ptr("bubble_variant", bv),
                                                  len(bv), None if "xf" in nulls else C.byref(XF), ptr("fvariant_pos", fpos), ptr("gt", g),
                                                  int(chunk_start), int(chunk_end), None if "out" in nulls else C.byref(R),
                                                  None if "filtered_read" in nulls else C.byref(fr), None if "block" in nulls else C.byref(blk)))
    nf, nv, nb = int(R.n_filtered), int(R.n_variants), len(bv)
    if blk.value is None:
        assert nf == 0 and nv == 0 and fr.value is None and bytes(R) == bytes(StringChunkRest()), "an empty rest must be all NULL"
        return ExtractedRest(R, None, np.zeros(0, np.int32), {}, None, (hold_x, hold_f))
    f_first = _as_np(R.fsub_first, nb + 1, np.int64)
    a_first = _as_np(R.valle_first, nv + 1, np.int64)
    e_first = _as_np(R.ventry_first, nv + 1, np.int64)
    nfs, na, ne = int(f_first[nb]), int(a_first[nv]), int(e_first[nv])
    raw = dict(forward_strand=_as_np(R.forward_strand, nf, np.uint8), pool=_as_np(R.pool, int(R.pool_bytes), np.uint8), fsub_first=f_first,
               fsub_off=_as_np(R.fsub_off, nfs, np.int64), fsub_len=_as_np(R.fsub_len, nfs, np.int32), fsub_read=_as_np(R.fsub_read, nfs, np.int32),
               valle_first=a_first, valle_off=_as_np(R.valle_off, na, np.int64), valle_len=_as_np(R.valle_len, na, np.int32),
               gt=_as_np(R.gt, 2 * nv, np.int32), ventry_first=e_first, ventry_read=_as_np(R.ventry_read, ne, np.int32),
               ventry_off=_as_np(R.ventry_off, ne, np.int64), ventry_len=_as_np(R.ventry_len, ne, np.int32))
    pool = raw["pool"]
    cut = lambda o, l: pool[int(o):int(o) + int(l)].copy()
    fsubs = [[(int(raw["fsub_read"][k]), cut(raw["fsub_off"][k], raw["fsub_len"][k])) for k in range(int(f_first[b]), int(f_first[b + 1]))] for b in range(nb)]
    variants = [([cut(raw["valle_off"][a], raw["valle_len"][a]) for a in range(int(a_first[v]), int(a_first[v + 1]))],
                 (int(raw["gt"][2 * v]), int(raw["gt"][2 * v + 1])),
                 [(int(raw["ventry_read"][k]), cut(raw["ventry_off"][k], raw["ventry_len"][k])) for k in range(int(e_first[v]), int(e_first[v + 1]))])
                for v in range(nv)]
    rest = dict(forward_strand=raw["forward_strand"], fsubs=fsubs, variants=variants)
    return ExtractedRest(R, blk, _as_np(fr, nf, np.int32), raw, rest, (hold_x, hold_f))


def equal_substring_classes(ctx: Optional[Context], entry_first, pool, off, length, nulls=()) -> np.ndarray:
    """mrp_equal_substring_classes -> rep int32 [n_entries]: per entry the first entry of its site with the same substring.  ctx None
    passes a NULL context; nulls names arguments to pass as NULL (for the argument checks)."""
    L = load()
    first = np.ascontiguousarray(entry_first, np.int64)
    pool = np.ascontiguousarray(pool, np.uint8)
    off, length = _opt(off, np.int64), _opt(length, np.int32)
    rep = np.full(len(off), -7, np.int32)
    ptr = lambda name, a: None if name in nulls or a.size == 0 else a.ctypes.data
    rc = L.mrp_equal_substring_classes(ctx.h if ctx else None, len(first) - 1, ptr("entry_first", first), ptr("pool", pool), pool.size, ptr("off", off),
                                       ptr("len", length), ptr("rep_out", rep))
    if rc != MRP_OK:
        assert (rep == -7).all(), "outputs written on an error"
    _check(rc)
    return rep


# ---- the phased variant records (mrp_variant_records_from_extracted, mrp_variants_from_records) ----

def _records_dict(R, free: bool = True) -> dict:
    """the arrays of one mrp_variant_records as numpy copies (gt as [n_sites, 2]); the C arrays are released"""
    ns = int(R.n_primary) + int(R.n_filtered)
    first = _as_np(R.read_first, ns + 1, np.int64)
    size = dict(s=ns, s1=ns + 1, s2=2 * ns, r=int(first[ns]))
    d = {f: _as_np(getattr(R, f), size[k], t) for f, t, k in _RECORD_ARRAYS}
    d["gt"] = d["gt"].reshape(ns, 2)
    d["n_primary"], d["n_filtered"] = int(R.n_primary), int(R.n_filtered)
    if free:
        for f, _, _ in _RECORD_ARRAYS:
            load().mrp_free(C.cast(getattr(R, f), C.c_void_p))
    return d


def records_struct(rec: dict):
    """mrp_variant_records over the numpy arrays of a records dict; returns (VariantRecords, the arrays it points into)"""
    keep = {f: np.ascontiguousarray(rec[f], t).reshape(-1) for f, t, _ in _RECORD_ARRAYS}
    ptr = lambda a: a.ctypes.data if a.size else None
    return VariantRecords(int(rec["n_primary"]), int(rec["n_filtered"]), *[ptr(keep[f]) for f, _, _ in _RECORD_ARRAYS]), keep


def phase_result_struct(g: dict):
    """mrp_phase_result over a dict _phase_result_dict made (the arrays a record reads); returns (PhaseResult, the arrays)"""
    keep = dict(h1=np.ascontiguousarray(g["hap1"], np.uint64), h2=np.ascontiguousarray(g["hap2"], np.uint64),
                gp=np.ascontiguousarray(g["genotype_probs"], np.float32), p1=np.ascontiguousarray(g["hap_probs1"], np.float32),
                p2=np.ascontiguousarray(g["hap_probs2"], np.float32))
    R = PhaseResult()
    R.ref_start, R.length = int(g["ref_start"]), int(g["length"])
    as_p = lambda a, t: C.cast(a.ctypes.data if a.size else None, C.POINTER(t))
    R.haplotype_string1, R.haplotype_string2 = as_p(keep["h1"], C.c_uint64), as_p(keep["h2"], C.c_uint64)
    R.genotype_probs, R.haplotype_probs1, R.haplotype_probs2 = as_p(keep["gp"], C.c_float), as_p(keep["p1"], C.c_float), as_p(keep["p2"], C.c_float)
    return R, keep


def variant_records_from_extracted(x: dict, xf: dict, keep, bubble_variant, result: dict, hap, variant_pos, fvariant_pos, chunk_start: int,
                                   chunk_end: int, gt, variant_state, nulls=()) -> dict:
    """mrp_variant_records_from_extracted -> dict of the record arrays (numpy; gt as [n_sites, 2]; n_primary, n_filtered).  result: a dict
    as _phase_result_dict makes it; nulls names arguments to pass as NULL (for the argument checks).  On an error the output struct is
    checked to be unwritten."""
    L = load()
    X, hold_x = extracted_struct(x)
    XF, hold_f = extracted_struct(xf)
    G, hold_g = phase_result_struct(result)
    km = None if keep is None else np.ascontiguousarray(keep, np.uint8)
    arrs = dict(bubble_variant=np.ascontiguousarray(bubble_variant, np.int64), hap=np.ascontiguousarray(hap, np.int8),
                variant_pos=np.ascontiguousarray(variant_pos, np.int64), fvariant_pos=np.ascontiguousarray(fvariant_pos, np.int64),
                gt=np.ascontiguousarray(gt, np.int32).reshape(-1), variant_state=np.ascontiguousarray(variant_state, np.int32))
    ptr = lambda name: None if name in nulls or arrs[name].size == 0 else arrs[name].ctypes.data
    R = VariantRecords()
    R.n_primary = -7
    rc = L.mrp_variant_records_from_extracted(None if "x" in nulls else C.byref(X), None if "xf" in nulls else C.byref(XF),
                                              None if km is None or km.size == 0 else km.ctypes.data, ptr("bubble_variant"), len(arrs["bubble_variant"]),
                                              None if "result" in nulls else C.byref(G), ptr("hap"), ptr("variant_pos"), ptr("fvariant_pos"),
                                              int(chunk_start), int(chunk_end), ptr("gt"), ptr("variant_state"), None if "out" in nulls else C.byref(R))
    if rc != MRP_OK:
        assert R.n_primary == -7 and not any(getattr(R, f) for f, _, _ in _RECORD_ARRAYS), "outputs written on an error"
    _check(rc)
    return _records_dict(R)


def variants_from_records(records, variant_pos, n_alleles, fvariant_pos, fn_alleles, switched, read_id):
    """mrp_variants_from_records over per-chunk lists (records: dicts as variant_records_from_extracted returns) -> (variants as the dicts
    capi.phase_sets takes, each with "chunk", "site" and the three log values after switching)"""
    L = load()
    n = len(records)
    built = [records_struct(r) for r in records]
    arr = (VariantRecords * max(n, 1))(*[b[0] for b in built])

    def table(rows, t):
        keep = [np.ascontiguousarray(r, t) for r in rows]
        return (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in keep]), keep
    vp_, k1 = table(variant_pos, np.int64)
    na_, k2 = table(n_alleles, np.int32)
    fp_, k3 = table(fvariant_pos, np.int64)
    fa_, k4 = table(fn_alleles, np.int32)
    id_, k5 = table(read_id, np.int32)
    sw = np.ascontiguousarray(switched, np.int32)
    out = RecordVariants()
    _check(L.mrp_variants_from_records(n, arr, vp_, na_, fp_, fa_, sw.ctypes.data if sw.size else None, id_, C.byref(out)))
    res = _record_variants_list(out)
    L.mrp_free(C.cast(out.variants, C.c_void_p))
    return res


def _record_variants_list(out) -> list:
    """the variants of a mrp_record_variants block as the dicts capi.phase_sets takes (copies; the block is the caller's to free)"""
    m = int(out.n_variants)
    chunk, site = _as_np(out.chunk, m, np.int32), _as_np(out.site, m, np.int32)
    logs = [_as_np(getattr(out, f), m, np.float32) for f in ("genotype_log_prob", "hap1_log_prob", "hap2_log_prob")]
    res = []
    for i in range(m):
        V = out.variants[i]
        off = _as_np(V.allele_read_off, V.n_alleles + 1, np.int64)
        ids = _as_np(V.allele_reads, int(off[V.n_alleles]), np.int32)
        res.append(dict(pos=int(V.pos), gt1=int(V.gt1), gt2=int(V.gt2), alleleIdxToReads=[ids[off[a]:off[a + 1]].tolist() for a in range(V.n_alleles)],
                        chunk=int(chunk[i]), site=int(site[i]), genotype_log_prob=logs[0][i], hap1_log_prob=logs[1][i], hap2_log_prob=logs[2][i]))
    return res


# ---- closing a contig on the host (mrp_final_read_tags, mrp_stitch_values, mrp_close_contig, mrp_close_contigs) ----

def filtered_out_struct(filtered: dict):
    """mrp_filtered_out over the numpy arrays of a "filtered" dict as phase_aligned_chunks_with_filtered returns it (only read_hap and
    variant_state are required); returns (FilteredOut, the arrays it points into)"""
    keep = dict(read_hap=np.ascontiguousarray(filtered["read_hap"], np.int32), variant_state=np.ascontiguousarray(filtered.get("variant_state", []), np.int32))
    for f in ("h1", "h2", "cis", "trans"):
        if f in filtered:
            keep[f] = np.ascontiguousarray(filtered[f], np.float64)
    ptr = lambda f: keep[f].ctypes.data if f in keep and keep[f].size else None
    return FilteredOut(len(keep["read_hap"]), ptr("read_hap"), ptr("h1"), ptr("h2"), len(keep["variant_state"]), ptr("variant_state"), ptr("cis"), ptr("trans")), keep


def _closed_list(a):
    """an int32 list closed by -1, as filtered_read_out is"""
    return np.ascontiguousarray(list(np.asarray(a, np.int64).reshape(-1)) + [-1], np.int32)


def final_read_tags(hap, filtered: Optional[dict] = None, filtered_read=None, nulls=()) -> np.ndarray:
    """mrp_final_read_tags -> int8 [n_reads]: 1 / 2 / 0.  hap: the call's hap_out; filtered / filtered_read: the chunk's "filtered" dict and
    "filtered_read" (None: the haplotag form).  nulls ("hap", "out") pass NULL.  On an error the output is checked to be unwritten."""
    h = np.ascontiguousarray(hap, np.int8)
    out = np.full(max(len(h), 1), 77, np.int8)
    F = fr = None
    if filtered is not None:
        F, _keep = filtered_out_struct(filtered)
        fr = _closed_list([] if filtered_read is None else filtered_read)
    rc = load().mrp_final_read_tags(len(h), None if "hap" in nulls or not h.size else h.ctypes.data, None if F is None else C.byref(F),
                                    None if fr is None else fr.ctypes.data, None if "out" in nulls else out.ctypes.data)
    if rc != MRP_OK:
        assert (out == 77).all(), "outputs written on an error"
    _check(rc)
    return out[:len(h)]


def stitch_values(hap, phred, final_tag, nulls=()) -> np.ndarray:
    """mrp_stitch_values -> float64 [n_reads]; hap None: the haplotag form (-1.0 for every tagged read)"""
    t = np.ascontiguousarray(final_tag, np.int8)
    h = None if hap is None else np.ascontiguousarray(hap, np.int8)
    p = None if phred is None else np.ascontiguousarray(phred, np.float64)
    out = np.full(max(len(t), 1), 77.0)
    ptr = lambda a, name: None if a is None or name in nulls or not a.size else a.ctypes.data
    rc = load().mrp_stitch_values(len(t), ptr(h, "hap"), ptr(p, "phred"), ptr(t, "final_tag"), None if "out" in nulls else out.ctypes.data)
    if rc != MRP_OK:
        assert (out == 77.0).all(), "outputs written on an error"
    _check(rc)
    return out[:len(t)]


def contig_chunk_struct(ch: dict, nulls=()):
    """mrp_contig_chunk over one chunk's results: dict(read_names, read_id, hap, phred, filtered, filtered_read, records, variant_pos, n_alleles,
    fvariant_pos, fn_alleles).  filtered None: the haplotag form; records None: no sites.  nulls names fields to pass as NULL.  Returns
    (ContigChunk, what it points into)."""
    nr = len(ch["read_names"])
    names = [s.encode() for s in ch["read_names"]]
    keep = dict(names=names, name_arr=(C.c_char_p * max(nr, 1))(*names), read_id=np.ascontiguousarray(ch.get("read_id", np.zeros(nr)), np.int32),
                hap=np.ascontiguousarray(ch["hap"], np.int8))
    if "read_names[0]" in nulls:
        keep["name_arr"][0] = None
    K = ContigChunk()
    K.n_reads = nr
    K.read_names = None if "read_names" in nulls else C.cast(keep["name_arr"], C.c_void_p)
    K.read_id = None if "read_id" in nulls or not nr else keep["read_id"].ctypes.data
    K.hap_out = None if "hap" in nulls or not nr else keep["hap"].ctypes.data
    if ch.get("phred") is not None and "phred" not in nulls:
        keep["phred"] = np.ascontiguousarray(ch["phred"], np.float64)
        K.phred_out = keep["phred"].ctypes.data if nr else None
    if ch.get("filtered") is not None:
        keep["F"], keep["F_arrays"] = filtered_out_struct(ch["filtered"])
        K.filtered_out = C.pointer(keep["F"])
        keep["fr"] = _closed_list(ch.get("filtered_read", []))
        K.filtered_read_out = keep["fr"].ctypes.data
    if ch.get("records") is not None:
        keep["R"], keep["R_arrays"] = records_struct(ch["records"])
        K.records = C.pointer(keep["R"])
        for f, t in (("variant_pos", np.int64), ("n_alleles", np.int32), ("fvariant_pos", np.int64), ("fn_alleles", np.int32)):
            keep[f] = np.ascontiguousarray(ch[f], t)
            setattr(K, f, keep[f].ctypes.data if keep[f].size and f not in nulls else None)
        K.n_variants, K.n_fvariants = len(keep["variant_pos"]), len(keep["fvariant_pos"])
    return K, keep


def _contig_out_dict(O) -> dict:
    """a mrp_contig_out as Python values (copies); the struct is released"""
    n = int(O.n_chunks)
    switched = _as_np(O.switched, n, np.int32)
    d = dict(switched=[int(x) for x in switched], counts=[tuple(int(x) for x in row) for row in _as_np(O.counts, 4 * n, np.int64).reshape(n, 4)])
    d["variants"] = _record_variants_list(O.variants)
    m = len(d["variants"])
    ps, why = _as_np(O.phase_set, m, np.int32), _as_np(O.reason, m, np.int32)
    d["phase_sets"] = [(int(ps[i]), int(why[i])) for i in range(m)]
    return d


def _contig_rules(primary_reads_only, prevent_switching, rules):
    return ContigRules(int(bool(primary_reads_only)), int(bool(prevent_switching)), int(rules[0]), float(rules[1]), float(rules[2]))


def close_contigs(contigs, primary_reads_only: bool = False, prevent_switching: bool = False, rules=(2, 0.05, 0.5), nulls=(), one: bool = False):
    """mrp_close_contigs over a list of contigs, each a list of chunk dicts in genome order (contig_chunk_struct) -> per contig
    dict(switched, counts [(cisH1, cisH2, transH1, transH2)], final_hap [int8 array per chunk], variants (the dicts capi.phase_sets takes),
    phase_sets [(phase set, reason code)]).  one: mrp_close_contig over the single contig given.  On an error the outputs are checked to
    be unwritten."""
    L = load()
    flat = [ch for contig in contigs for ch in contig]
    built = [contig_chunk_struct(ch, nulls if i == 0 else ()) for i, ch in enumerate(flat)]
    arr = (ContigChunk * max(len(flat), 1))(*[b[0] for b in built])
    first = np.ascontiguousarray(np.cumsum([0] + [len(c) for c in contigs]), np.int64)
    R = _contig_rules(primary_reads_only, prevent_switching, rules)
    outs = (ContigOut * max(len(contigs), 1))()
    for O in outs:
        O.n_chunks = -7
    if one:
        assert len(contigs) == 1
        rc = L.mrp_close_contig(len(flat), None if "chunks" in nulls else arr, None if "rules" in nulls else C.byref(R), None if "out" in nulls else outs)
    else:
        rc = L.mrp_close_contigs(len(contigs), None if "first_chunk" in nulls else first.ctypes.data, None if "chunks" in nulls else arr,
                                 None if "rules" in nulls else C.byref(R), None if "out" in nulls else outs)
    if rc != MRP_OK:
        assert all(O.n_chunks == -7 and not O.switched and not O.final_hap and not O.variants.variants for O in outs), "outputs written on an error"
    _check(rc)
    res = []
    for k, contig in enumerate(contigs):
        O = outs[k]
        d = _contig_out_dict(O)
        d["final_hap"] = [_as_np(O.final_hap[c], len(ch["read_names"]), np.int8) for c, ch in enumerate(contig)]
        L.mrp_contig_out_clear(C.byref(O))
        res.append(d)
    return res


def close_contig(chunks, **kw) -> dict:
    """mrp_close_contig over the chunk dicts of one contig -> the dict close_contigs returns per contig"""
    return close_contigs([list(chunks)], one=True, **kw)[0]


# ---- haplotagging aligned reads from a phased VCF (mrp_haptag_sites_from_extracted, mrp_haplotag_aligned_chunks) ----

_HAPTAG_SITE_ARRAYS = (("allele_first", np.int64, "s1"), ("allele_off", np.int64, "a"), ("allele_len", np.int32, "a"), ("compare", np.int32, "s2"),
                       ("entry_first", np.int64, "s1"), ("entry_read", np.int64, "e"), ("entry_off", np.int64, "e"), ("entry_len", np.int32, "e"))


def _genotype_arrays(gts):
    """per chunk an int32 [2 * n_variants] array (None stays NULL) -> (the void* array the C-ABI takes, the arrays it points into)"""
    keep = [None if g is None else np.ascontiguousarray(g, np.int32).reshape(-1) for g in gts]
    arr = (C.c_void_p * max(len(keep), 1))(*[None if g is None or g.size == 0 else g.ctypes.data for g in keep])
    return arr, keep


def haptag_sites_from_extracted(xs, gts, null_gt=False):
    """mrp_haptag_sites_from_extracted over the dicts extract_read_substrings returns (or tests.extract_oracle.as_arrays makes); gts: per
    chunk the phased genotypes, int32 [n_variants, 2].  Returns (dict of the mrp_haptag_sites arrays as numpy copies, with n_sites and
    pool; read_first int64 [n_chunks + 1]).  null_gt passes a NULL genotype table (for the argument checks)."""
    L = load()
    n = len(xs)
    built = [extracted_struct(x) for x in xs]
    arr = (ExtractedChunk * max(n, 1))(*[b[0] for b in built])
    garr, gkeep = _genotype_arrays(gts)
    S = HaptagSites()
    read_first = np.zeros(n + 1, np.int64)
    _check(L.mrp_haptag_sites_from_extracted(n, arr, None if null_gt else garr, C.byref(S), read_first.ctypes.data))
    ns = int(S.n_sites)
    a_first = _as_np(S.allele_first, ns + 1, np.int64)
    e_first = _as_np(S.entry_first, ns + 1, np.int64)
    size = dict(s1=ns + 1, s2=2 * ns, a=int(a_first[ns]), e=int(e_first[ns]))
    out = {f: _as_np(getattr(S, f), size[k], t) for f, t, k in _HAPTAG_SITE_ARRAYS}
    out["pool"] = _as_np(S.pool, int(S.pool_bytes), np.uint8)
    out["n_sites"] = ns
    L.mrp_free(S.allele_first)
    return out, read_first


def partition_reads_from_site_arrays(ctx: Context, forward_model: PairHmm, reverse_model: PairHmm, sites: dict, n_reads: int, read_forward_strand,
                                     expansion: int = 4):
    """mrp_partition_reads_by_haplotype over the arrays haptag_sites_from_extracted returns -> (hap, h1, h2, PairHmmStats)"""
    keep = {f: np.ascontiguousarray(sites[f], t) for f, t, _ in _HAPTAG_SITE_ARRAYS}
    pool = np.ascontiguousarray(sites["pool"], np.uint8)
    ptr = lambda a: None if a.size == 0 else a.ctypes.data
    S = HaptagSites(int(sites["n_sites"]), ptr(pool), pool.size, *[ptr(keep[f]) for f, _, _ in _HAPTAG_SITE_ARRAYS])
    return _partition_reads(ctx, forward_model, reverse_model, S, n_reads, read_forward_strand, expansion)


def haplotag_aligned_chunks(ctx: Optional[Context], chunks, gts, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm],
                            options: Optional[dict] = None, expansion: int = 4, totals: bool = True, structs=None, null_options: bool = False):
    """mrp_haplotag_aligned_chunks -> (per chunk dict(hap int8 [n_reads]: 1 / 2 / 0 / -1, h1, h2 float64 (None without totals)),
    HaplotagAlignedStats).  gts: per chunk int32 [n_variants, 2] (None: NULL).  ctx / a model None pass NULL; structs as
    extract_read_substrings takes them."""
    return _haplotag_aligned(ctx, chunks, gts, forward_model, reverse_model, options, expansion, totals, structs, null_options)


_NO_QUEUE = object()  # (None is the NULL queue)
LAST_HAPLOTAG_CALL_MS = 0.0  # wall time of the last C call _haplotag_aligned made, without the binding's conversions around it (tools/)


def _haplotag_aligned(ctx, chunks, gts, forward_model, reverse_model, options=None, expansion: int = 4, totals: bool = True, structs=None,
                      null_options: bool = False, queue=_NO_QUEUE, devices=None, chunks_per_batch: int = 0):
    """mrp_haplotag_aligned_chunks, or with queue (a mrp_queue handle, or None for a NULL queue) or devices (a list) the work queue's
    twins, which take chunks_per_batch and return a QueueStats"""
    global LAST_HAPLOTAG_CALL_MS
    L = load()
    queued = queue is not _NO_QUEUE or devices is not None
    if devices is not None:
        dev = (C.c_int32 * max(len(devices), 1))(*devices)
        head, fn = (C.cast(dev, C.c_void_p), len(devices)), L.mrp_haplotag_aligned_chunks_on_devices
    elif queued:
        head, fn = (queue,), L.mrp_queue_haplotag_aligned_chunks
    else:
        head, fn = (ctx.h if ctx else None,), L.mrp_haplotag_aligned_chunks
    n = len(chunks)
    built = structs if structs is not None else [aligned_chunk_struct(c) for c in chunks]
    arr = (AlignedChunk * max(n, 1))(*[b[0] for b in built])
    garr, gkeep = _genotype_arrays(gts)
    opt = ExtractOptions.from_dict(options or shipped_extract_options())
    nr = [int(b[0].n_reads) for b in built]
    hap = [np.full(k, 99, np.int8) for k in nr]
    h1 = [np.full(k, np.nan) for k in nr]
    h2 = [np.full(k, np.nan) for k in nr]
    ptrs = lambda arrays: (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrays])
    st = QueueStats() if queued else HaplotagAlignedStats()
    by = lambda m: None if m is None else C.byref(m)
    per_batch = (int(chunks_per_batch),) if queued else ()
    t_call = time.perf_counter()
    rc = fn(*head, n, arr, garr, None if null_options else C.byref(opt), by(forward_model), by(reverse_model), int(expansion), *per_batch, ptrs(hap),
            ptrs(h1) if totals else None, ptrs(h2) if totals else None, C.byref(st))
    LAST_HAPLOTAG_CALL_MS = (time.perf_counter() - t_call) * 1e3
    _check(rc)
    return [dict(hap=hap[c], h1=h1[c] if totals else None, h2=h2[c] if totals else None) for c in range(n)], st


def haplotag_chunk_units(chunk, gt, struct=None) -> int:
    """mrp_haplotag_chunk_units: the (read, het variant) units uniform coverage gives one chunk (a margin_amd.synth.AlignedChunk) with its
    phased genotypes gt (int32 [n_variants, 2]; None: NULL) -- what the work queue orders and cuts haplotagging by"""
    S = struct if struct is not None else aligned_chunk_struct(chunk)
    g = None if gt is None else np.ascontiguousarray(gt, np.int32).reshape(-1)
    u = C.c_int64(-1)
    _check(load().mrp_haplotag_chunk_units(C.byref(S[0]), None if g is None or g.size == 0 else g.ctypes.data, C.byref(u)))
    return int(u.value)


def haplotag_aligned_chunks_on_devices(devices, chunks, gts, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm],
                                       options: Optional[dict] = None, totals: bool = True, chunks_per_batch: int = 0, **kw):
    """mrp_haplotag_aligned_chunks_on_devices -> (haplotag_aligned_chunks' list of dicts in input order, QueueStats)"""
    return _haplotag_aligned(None, chunks, gts, forward_model, reverse_model, options=options, totals=totals, devices=list(devices),
                             chunks_per_batch=chunks_per_batch, **kw)


# ---- from alignments to haplotypes and HP tags in one call (mrp_phase_aligned_chunks) ----

def aligned_chunk_rest_struct(filtered_chunk, gt):
    """mrp_aligned_chunk_rest from a margin_amd.synth.AlignedChunk that holds the filtered variants (its reads are not looked at) and their gt
    (int32 [n, 2] or flat); returns (AlignedChunkRest, the arrays it points into)"""
    S, keep = aligned_chunk_struct(filtered_chunk)
    keep["gt"] = np.ascontiguousarray(gt, np.int32).reshape(-1)
    assert keep["gt"].size == 2 * int(S.n_variants)
    R = AlignedChunkRest(S.n_variants, S.variant_pos, S.allele_first, S.allele_off, S.allele_len, S.allele_chars, S.allele_bytes, S.is_sv,
                         keep["gt"].ctypes.data if keep["gt"].size else None)
    return R, keep


LAST_ALIGNED_CALL_MS = 0.0  # wall time of the last C call _phase_aligned made, without the binding's conversions around it (tools/)


def phase_aligned_chunks_with_filtered(ctx: Optional[Context], chunks, rests, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm],
                                       params: Optional[Params], **kw):
    """mrp_phase_aligned_chunks_with_filtered -> (phase_aligned_chunks' list of dicts, each with "filtered" (dict(read_hap, h1, h2 over the
    chunk's reads then its filtered reads, variant_state, cis, trans)) and "filtered_read" (int32, the chunk's read index of every filtered
    read), PhaseAlignedFilteredStats).  rests: per chunk (filtered AlignedChunk, gt); or None with rest_structs =
    [aligned_chunk_rest_struct(...)].  Further nulls: "rest", "filtered_out", "filtered_read_out", "gt[0]"."""
    return _phase_aligned(ctx, chunks, forward_model, reverse_model, params, rests=rests, with_rest=True, **kw)


def phase_aligned_chunks_with_records(ctx: Optional[Context], chunks, rests, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm],
                                      params: Optional[Params], **kw):
    """mrp_phase_aligned_chunks_with_records -> (phase_aligned_chunks_with_filtered's list of dicts, each with "records" (the record arrays as
    variant_records_from_extracted returns them), PhaseAlignedRecordsStats).  A further null: "records_out"."""
    return _phase_aligned(ctx, chunks, forward_model, reverse_model, params, rests=rests, with_rest=True, with_records=True, **kw)


def phase_aligned_chunks(ctx: Optional[Context], chunks, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm], params: Optional[Params],
                         **kw):
    """mrp_phase_aligned_chunks; arguments and results as _phase_aligned states them"""
    return _phase_aligned(ctx, chunks, forward_model, reverse_model, params, **kw)


def aligned_chunk_units(chunk, rest=None, struct=None, rest_struct=None) -> int:
    """mrp_aligned_chunk_units: the (read, variant) units uniform coverage gives one chunk (a margin_amd.synth.AlignedChunk), with rest (the
    filtered AlignedChunk, or (filtered AlignedChunk, gt)) the rest's variants counted as well -- what the work queue orders and cuts by"""
    S = struct if struct is not None else aligned_chunk_struct(chunk)
    R = rest_struct
    if R is None and rest is not None:
        f, gt = rest if isinstance(rest, tuple) else (rest, np.zeros((len(rest.alleles), 2), np.int32))
        R = aligned_chunk_rest_struct(f, gt)
    u = C.c_int64(-1)
    _check(load().mrp_aligned_chunk_units(C.byref(S[0]), None if R is None else C.byref(R[0]), C.byref(u)))
    return int(u.value)


def phase_aligned_chunks_on_devices(devices, chunks, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm], params: Optional[Params],
                                    chunks_per_batch: int = 0, **kw):
    """mrp_phase_aligned_chunks_on_devices -> (phase_aligned_chunks' list of dicts in input order, QueueStats)"""
    return _phase_aligned(None, chunks, forward_model, reverse_model, params, devices=list(devices), chunks_per_batch=chunks_per_batch, **kw)


def phase_aligned_chunks_with_filtered_on_devices(devices, chunks, rests, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm],
                                                  params: Optional[Params], chunks_per_batch: int = 0, **kw):
    """mrp_phase_aligned_chunks_with_filtered_on_devices -> (phase_aligned_chunks_with_filtered's list of dicts in input order, QueueStats)"""
    return _phase_aligned(None, chunks, forward_model, reverse_model, params, rests=rests, with_rest=True, devices=list(devices),
                          chunks_per_batch=chunks_per_batch, **kw)


def phase_aligned_chunks_with_records_on_devices(devices, chunks, rests, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm],
                                                 params: Optional[Params], chunks_per_batch: int = 0, **kw):
    """mrp_phase_aligned_chunks_with_records_on_devices -> (phase_aligned_chunks_with_records' list of dicts in input order, QueueStats with the
    QueueRecordsStats as its attribute `records`)"""
    return _phase_aligned(None, chunks, forward_model, reverse_model, params, rests=rests, with_rest=True, with_records=True, devices=list(devices),
                          chunks_per_batch=chunks_per_batch, **kw)


def _phase_aligned(ctx: Optional[Context], chunks, forward_model: Optional[PairHmm], reverse_model: Optional[PairHmm], params: Optional[Params],
                   options: Optional[dict] = None, keeps=None, min_phred: int = 0, expansion: int = 4, sv_threshold: int = 512,
                   het_substitution_probability: float = 0.0, profiles: bool = False, structs=None, nulls=(), rests=None, rest_structs=None,
                   with_rest: bool = False, queue=_NO_QUEUE, devices=None, chunks_per_batch: int = 0, with_records: bool = False):
    """mrp_phase_aligned_chunks -> (per chunk dict(result, hap int8 [n_reads], phred, bubble_variant int64 [n_bubbles][, profile]),
    PhaseAlignedStats).  keeps: None, or per chunk None / a uint8 mask over its reads.  ctx / a model / params None pass NULL;
    nulls names further arguments to pass as NULL ("options", "out", "hap_out", "read_names", "hap_out[0]", "phred_out[0]",
    "read_names[0]", "read_names[0][0]": for the argument checks).  On an error the output arrays are checked to be untouched.
    queue (a mrp_queue handle, or None for a NULL queue) or devices (a list) select the work queue's twins, which take
    chunks_per_batch and return a QueueStats."""
    global LAST_ALIGNED_CALL_MS
    L = load()
    queued = queue is not _NO_QUEUE or devices is not None
    if devices is not None:
        dev = (C.c_int32 * max(len(devices), 1))(*devices)
        head = (C.cast(dev, C.c_void_p), len(devices))
    else:
        head = (queue,) if queued else (ctx.h if ctx else None,)
    n = len(chunks)
    built = structs if structs is not None else [aligned_chunk_struct(c) for c in chunks]
    arr = (AlignedChunk * max(n, 1))(*[b[0] for b in built])
    opt = ExtractOptions.from_dict(options or shipped_extract_options())
    nr = [int(b[0].n_reads) for b in built]
    names = [[s.encode() for s in c.read_names] for c in chunks]
    name_arrs = [(C.c_char_p * max(len(x), 1))(*x) for x in names]
    if "read_names[0][0]" in nulls:
        name_arrs[0][0] = None
    name_ptrs = (C.c_void_p * max(n, 1))(*[C.cast(a, C.c_void_p) if k else None for a, k in zip(name_arrs, nr)])
    if "read_names[0]" in nulls:
        name_ptrs[0] = None
    masks = [None if keeps is None or keeps[c] is None else np.ascontiguousarray(keeps[c], np.uint8) for c in range(n)]
    mask_ptrs = (C.c_void_p * max(n, 1))(*[None if m is None or m.size == 0 else m.ctypes.data for m in masks])
    hap = [np.full(k, 99, np.int8) for k in nr]
    phred = [np.full(k, np.nan) for k in nr]
    hp = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in hap])
    pp = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in phred])
    if "hap_out[0]" in nulls:
        hp[0] = None
    if "phred_out[0]" in nulls:
        pp[0] = None
    res = (C.POINTER(PhaseResult) * max(n, 1))()
    prof = (ProfileOut * max(n, 1))() if profiles else None
    bv = (C.c_void_p * max(n, 1))()
    by = lambda m: None if m is None else C.byref(m)
    per_batch = (int(chunks_per_batch),) if queued else ()
    if not with_rest:
        st = QueueStats() if queued else PhaseAlignedStats()
        fn = (L.mrp_phase_aligned_chunks_on_devices if devices is not None else L.mrp_queue_phase_aligned_chunks) if queued else L.mrp_phase_aligned_chunks
        t_call = time.perf_counter()
        rc = fn(*head, n, arr, None if "read_names" in nulls else name_ptrs, None if keeps is None else mask_ptrs,
                None if "options" in nulls else C.byref(opt), by(forward_model), by(reverse_model), int(expansion), int(sv_threshold),
                float(het_substitution_probability), by(params), int(min_phred), *per_batch, None if "out" in nulls else res,
                None if "hap_out" in nulls else hp, pp, prof, bv, C.byref(st))
    else:
        rbuilt = rest_structs if rest_structs is not None else [aligned_chunk_rest_struct(f, g) for f, g in rests]
        rarr = (AlignedChunkRest * max(n, 1))(*[b[0] for b in rbuilt])
        if "gt[0]" in nulls:
            rarr[0].gt = None
        fout = (FilteredOut * max(n, 1))()
        fout[0].n_reads = 77  # (zeroed whatever the outcome)
        fr = (C.c_void_p * max(n, 1))()
        st = QueueStats() if queued else (PhaseAlignedRecordsStats() if with_records else PhaseAlignedFilteredStats())
        if queued and with_records:
            fn = L.mrp_phase_aligned_chunks_with_records_on_devices if devices is not None else L.mrp_queue_phase_aligned_chunks_with_records
        else:
            fn = (L.mrp_phase_aligned_chunks_with_filtered_on_devices if devices is not None else L.mrp_queue_phase_aligned_chunks_with_filtered) if queued \
                else (L.mrp_phase_aligned_chunks_with_records if with_records else L.mrp_phase_aligned_chunks_with_filtered)
        recs = (VariantRecords * max(n, 1))()
        recs[0].n_primary = 77  # (zeroed whatever the outcome)
        tail = (None if "records_out" in nulls else recs,) if with_records else ()
        after = ()
        if queued and with_records:  # the queue's stats, then the records' own (kept as st.records)
            st.records = QueueRecordsStats()
            after = (C.byref(st.records),)
        t_call = time.perf_counter()
        rc = fn(*head, n, arr, None if "rest" in nulls else rarr, None if "read_names" in nulls else name_ptrs,
                None if keeps is None else mask_ptrs, None if "options" in nulls else C.byref(opt), by(forward_model),
                by(reverse_model), int(expansion), int(sv_threshold), float(het_substitution_probability), by(params),
                int(min_phred), *per_batch, None if "out" in nulls else res, None if "hap_out" in nulls else hp, pp, prof, bv,
                None if "filtered_out" in nulls else fout, None if "filtered_read_out" in nulls else fr, *tail, C.byref(st), *after)
    LAST_ALIGNED_CALL_MS = (time.perf_counter() - t_call) * 1e3
    if with_rest:
        if rc != MRP_OK and n > 0 and not {"rest", "filtered_out", "filtered_read_out", "records_out"} & set(nulls):
            if queued and fout[0].n_reads == 77:  # (the queue writes nothing before its lanes start)
                fout[0].n_reads = 0
                if recs[0].n_primary == 77:
                    recs[0].n_primary = 0
            assert bytes(fout) == bytes((FilteredOut * max(n, 1))()) and not any(fr[i] for i in range(n)), "filtered_out not zeroed on an error"
            if with_records and "records_out" not in nulls:
                assert bytes(recs) == bytes((VariantRecords * max(n, 1))()), "records_out not zeroed on an error"
    if rc != MRP_OK:
        # (a queue that stops on a lane's error has written hap_out / phred_out of the batches that were done)
        untouched = (queued or (all((h == 99).all() for h in hap) and all(np.isnan(p).all() for p in phred))) and not any(bool(res[i]) for i in range(n)) and \
            not any(bv[i] for i in range(n)) and (prof is None or not any(prof[i].seqs or prof[i].pool for i in range(n)))
        assert untouched, "outputs written on an error"
    _check(rc)
    out = []
    for i in range(n):
        d = dict(result=_phase_result_dict(res[i].contents), hap=hap[i], phred=phred[i])
        L.mrp_phase_result_destroy(res[i])
        nb = 0
        ends = C.cast(bv[i], C.POINTER(C.c_int64))
        while ends[nb] != -1:  # the list is closed by a -1
            nb += 1
        d["bubble_variant"] = _as_np(bv[i], nb, np.int64)
        L.mrp_free(bv[i])
        if profiles:
            P = prof[i]
            d["profile"] = _profile_dict(P)
            an = _as_np(P.allele_number, nb, np.uint32)
            A = an.astype(np.int64)
            d["profile"].update(allele_number=an, sub=_as_np(P.substitution, int((A * A).sum()), np.uint16), prior=_as_np(P.prior, int(A.sum()), np.uint16))
            for f in ("seqs", "read_of_seq", "pool", "allele_number", "substitution", "prior"):
                L.mrp_free(C.cast(getattr(P, f), C.c_void_p))
        if with_rest:
            O = fout[i]
            nrd, nv = int(O.n_reads), int(O.n_variants)
            d["filtered"] = dict(read_hap=_as_np(O.read_hap, nrd, np.int32), h1=_as_np(O.h1, nrd, np.float64), h2=_as_np(O.h2, nrd, np.float64),
                                 variant_state=_as_np(O.variant_state, nv, np.int32), cis=_as_np(O.cis, nv, np.float64), trans=_as_np(O.trans, nv, np.float64))
            for f in ("read_hap", "h1", "h2", "variant_state", "cis", "trans"):
                L.mrp_free(C.cast(getattr(O, f), C.c_void_p))
            nf = 0
            ends = C.cast(fr[i], C.POINTER(C.c_int32))
            while ends[nf] != -1:  # the list is closed by a -1
                nf += 1
            d["filtered_read"] = _as_np(fr[i], nf, np.int32)
            L.mrp_free(fr[i])
            if with_records:
                d["records"] = _records_dict(recs[i])
        out.append(d)
    return out, st
