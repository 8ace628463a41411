"""ctypes binding of libcfhip.so (include/cfhip.h): the gfx950 device pipeline.

There is NO CPU fallback: if the library is missing or no HIP device is visible, creating a
context raises.  ``load(path)`` exists so that the CPU test-suite can bind the same prototypes
to the host-emulated build of the same kernel sources (tests/emu); the package itself only
ever loads the in-tree ``libcfhip.so``.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcfhip.so")


class Stats(C.Structure):
    """Mirror of ``cf_stats``."""
    _fields_ = [(n, C.c_int64) for n in (
        "n_reads", "n_bases", "n_units", "n_windows", "n_read_kmers", "n_distinct", "n_kept",
        "n_kmers", "n_cloud_entries", "n_emissions", "n_edges", "n_unique", "table_capacity",
        "n_spilled", "hbm_bytes_live", "n_dist_passes", "n_edges_stored")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class Times(C.Structure):
    """Mirror of ``cf_times``."""
    _fields_ = [(n, C.c_float) for n in (
        "load_ms", "count_ms", "select_ms", "clouds_ms", "filter_ms", "postings_ms", "dist_ms",
        "place_ms", "dist_kernel_ms", "count_kernel_ms", "rr_kernel_ms")]

    def as_dict(self):
        return {n: float(getattr(self, n)) for n, _ in self._fields_}


class TandemRead(C.Structure):
    """Mirror of ``cf_tandem_read``."""
    _fields_ = [(n, C.c_int32) for n in (
        "status", "n_windows", "n_rep_kmers", "n_conv", "count", "bin_left", "bin_right", "period", "hook_pos", "hook_index", "n_hook")]


class TandemShape(C.Structure):
    """Mirror of ``cf_tandem_shape``."""
    _fields_ = [(n, C.c_int64) for n in (
        "sort_tile", "rec_tile", "scan_tile", "block", "batch_windows", "key_mode", "code_bits", "read_bits", "pos_bits",
        "pos_shift", "n_batches", "n_key_batches", "n_records", "n_reads")] + [("phase_ms", C.c_float * 6)]


class ConsensusShape(C.Structure):
    """Mirror of ``cf_consensus_shape``."""
    _fields_ = [(n, C.c_int64) for n in (
        "max_len", "block_small", "block_big", "big_from", "launch_cap", "batch_bytes", "k_ins", "n_pos", "n_reads", "n_iters",
        "n_batches")] + [("phase_ms", C.c_float * 5)]


class UalignHit(C.Structure):
    """Mirror of ``cf_ualign_hit``."""
    _fields_ = [(n, C.c_int32) for n in (
        "status", "strand", "score", "r_st", "r_en", "u_st", "m_al_len", "n_ops", "n_match", "n_mismatch", "n_ins", "n_del")]


class UalignShape(C.Structure):
    """Mirror of ``cf_ualign_shape``."""
    _fields_ = [(n, C.c_int64) for n in (
        "max_unit", "cols_per_thread", "block", "row_chunk", "launch_cap", "batch_bytes", "n_reads", "n_score_pairs", "n_move_pairs",
        "n_batches")] + [("phase_ms", C.c_float * 4)]


class MonodecRead(C.Structure):
    """Mirror of ``cf_monodec_read``."""
    _fields_ = [(n, C.c_int32) for n in ("status", "strand", "score", "n_inst", "prefix")]


class MonodecInst(C.Structure):
    """Mirror of ``cf_monodec_inst``."""
    _fields_ = [(n, C.c_int32) for n in ("k", "st", "en", "n_match", "n_mismatch", "n_ins", "n_del")]


class MonodecShape(C.Structure):
    """Mirror of ``cf_monodec_shape``."""
    _fields_ = [(n, C.c_int64) for n in (
        "max_cols", "cols_per_thread", "block", "row_chunk", "launch_cap", "batch_bytes", "n_reads", "n_monomers", "n_cols",
        "n_score_pairs", "n_move_pairs", "n_batches")] + [("phase_ms", C.c_float * 4)]


class Monokmer(C.Structure):
    """Mirror of ``cf_monokmer``."""
    _fields_ = [(n, C.c_int32) for n in ("s", "i", "count", "pos")]


class MonokmerOcc(C.Structure):
    """Mirror of ``cf_monokmer_occ``."""
    _fields_ = [(n, C.c_int32) for n in ("s", "i")]


class MonokmersShape(C.Structure):
    """Mirror of ``cf_monokmers_shape``."""
    _fields_ = [(n, C.c_int64) for n in (
        "sort_tile", "scan_tile", "block", "launch_cap", "n_strings", "n_letters", "k", "min_mult", "with_positions", "n_windows",
        "n_distinct", "n_kmers", "n_occ", "n_rounds", "n_sorts", "n_sort_passes")] + [("phase_ms", C.c_float * 4)]


class MonomapRead(C.Structure):
    """Mirror of ``cf_monomap_read``."""
    _fields_ = [(n, C.c_int32) for n in ("n_hits", "e0", "j0", "i0", "e1", "j1", "i1", "valid", "n_path")]


class MonomapHit(C.Structure):
    """Mirror of ``cf_monomap_hit``."""
    _fields_ = [(n, C.c_int32) for n in ("e", "j", "i")]


class MonomapShape(C.Structure):
    """Mirror of ``cf_monomap_shape``."""
    _fields_ = [(n, C.c_int64) for n in (
        "sort_tile", "scan_tile", "block", "launch_cap", "n_edges", "n_reads", "k", "with_hits", "n_edge_letters", "n_read_letters",
        "n_edge_windows", "n_indexed", "n_hits", "n_path", "n_rounds", "n_sorts")] + [("phase_ms", C.c_float * 4)]


# every symbol include/cfhip.h declares: name -> (restype, argtypes)
_P, _I64, _I32, _U32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32
_PI64 = C.POINTER(C.c_int64)
PROTOTYPES = {
    "cf_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "cf_destroy": (None, [_P]),
    "cf_last_error": (C.c_char_p, [_P]),
    "cf_device_info": (C.c_int, [_P, C.c_char_p, C.c_int, _PI64, C.POINTER(_I32)]),
    "cf_load_reads": (C.c_int, [_P, _P, _P, _I64, _P, _P, _P]),
    "cf_rr_distances": (C.c_int, [_P, _P, _I32, _P, _P, _I64, _I32, _P, _P]),
    "cf_load_units": (C.c_int, [_P, _P, _P, _P]),
    "cf_count_kmers": (C.c_int, [_P, _I32, _I64, _I64]),
    "cf_count_occurrences": (C.c_int, [_P, _I32, _I64, _I64]),
    "cf_top_kmers": (C.c_int, [_P, _I64, _P, _P, _PI64]),
    "cf_reset_table": (C.c_int, [_P, _I32, _I64]),
    "cf_get_table": (C.c_int, [_P, _P, _P, _P, _I64, _PI64]),
    "cf_merge_table": (C.c_int, [_P, _P, _P, _P, _I64]),
    "cf_select_rare": (C.c_int, [_P, _I32, _U32, _U32, _PI64]),
    "cf_set_kmers": (C.c_int, [_P, _P, _I64, _I32]),
    "cf_get_kmers": (C.c_int, [_P, _P, _I64]),
    "cf_build_clouds": (C.c_int, [_P, _PI64]),
    "cf_filter_clouds": (C.c_int, [_P, _U32, _U32, _PI64]),
    "cf_get_clouds": (C.c_int, [_P, _P, _P, _I64]),
    "cf_set_clouds": (C.c_int, [_P, _P, _P, _I64]),
    "cf_dist_edges": (C.c_int, [_P, _I64, _I64, _I32, _I32, _U32, C.c_double, _I32, _I32, _I64, _PI64]),
    "cf_get_edges": (C.c_int, [_P, _P, _I64]),
    "cf_sort_edges": (C.c_int, [_P]),
    "cf_edges_checksum": (C.c_int, [_P, _I64, C.POINTER(C.c_uint64)]),
    "cf_checksum": (C.c_int, [_P, _I32, C.POINTER(C.c_uint64), _PI64]),
    "cf_get_unique_mask": (C.c_int, [_P, _P]),
    "cf_or_unique_mask": (C.c_int, [_P, _P]),
    "cf_reset_unique": (C.c_int, [_P]),
    "cf_place_reads": (C.c_int, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    "cf_contig_build": (C.c_int, [_P, _P, _P, _I64, _I32]),
    "cf_contig_info": (C.c_int, [_P, _PI64, _PI64, _PI64, _PI64, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "cf_contig_coverage": (C.c_int, [_P, _P, _I64]),
    "cf_map_reads": (C.c_int, [_P, _P, _I64, _I32, _I32, _P, _P, _P]),
    "cf_score_reads": (C.c_int, [_P, _P, _I64, _P, _P, _I32, _I32, _P, _P, _P]),
    "cf_contig_spread": (C.c_int, [_P, _I64, _P, _I64, _PI64]),
    "cf_contig_exact_info": (C.c_int, [_P, _PI64, C.POINTER(C.c_float)]),
    "cf_edit_distances": (C.c_int, [_P, _P, _P, _P, _I64, _I32, _P, C.POINTER(C.c_float)]),
    "cf_hpc": (C.c_int, [_P, _P, _P, _I64, _P, _P]),
    "cf_edit_info": (C.c_int, [_P, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_I32), _PI64]),
    "cf_tandem_scan": (C.c_int, [_P, _P, _P, _I64, _I32, _I32, _P]),
    "cf_tandem_hook_positions": (C.c_int, [_P, _P, _P, _I64, _PI64]),
    "cf_tandem_info": (C.c_int, [_P, C.POINTER(TandemShape)]),
    "cf_consensus_run": (C.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _P, C.POINTER(C.c_float)]),
    "cf_consensus_get": (C.c_int, [_P, _I32, _P, _P, _P, _P]),
    "cf_consensus_info": (C.c_int, [_P, C.POINTER(ConsensusShape)]),
    "cf_consensus_run_support": (C.c_int, [_P, _P, _P, _P, _P, _P, _I64, _I32, _I32, _I32, _P, C.POINTER(C.c_float)]),
    "cf_consensus_support": (C.c_int, [_P, _I32, _P]),
    "cf_consensus_reads": (C.c_int, [_P, _I32, _P, _P]),
    "cf_ualign_run": (C.c_int, [_P, _P, _I32, _P, _P, _I64, _I32, _I32, _I32, _P, C.POINTER(C.c_float)]),
    "cf_ualign_ops": (C.c_int, [_P, _P, _P, _I64, _PI64]),
    "cf_ualign_info": (C.c_int, [_P, C.POINTER(UalignShape)]),
    "cf_monodec_run": (C.c_int, [_P, _P, _P, _I32, _P, _P, _I64, _I32, _I32, _I32, _P, C.POINTER(C.c_float)]),
    "cf_monodec_get": (C.c_int, [_P, _P, _P, _I64, _PI64]),
    "cf_monodec_info": (C.c_int, [_P, C.POINTER(MonodecShape)]),
    "cf_monokmers_run": (C.c_int, [_P, _P, _P, _I64, _I64, _I64, _I32, _I32, _PI64, C.POINTER(C.c_float)]),
    "cf_monokmers_get": (C.c_int, [_P, _P, _I64, _PI64, _P, _P, _I64, _PI64]),
    "cf_monokmers_info": (C.c_int, [_P, C.POINTER(MonokmersShape)]),
    "cf_monomap_run": (C.c_int, [_P, _P, _P, _P, _P, _I64, _P, _P, _I64, _I64, _I32, _I32, _P, C.POINTER(C.c_float)]),
    "cf_monomap_get": (C.c_int, [_P, _P, _P, _I64, _PI64, _P, _P, _I64, _PI64]),
    "cf_monomap_info": (C.c_int, [_P, C.POINTER(MonomapShape)]),
    "cf_get_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "cf_get_times": (C.c_int, [_P, C.POINTER(Times)]),
    "cf_set_param": (C.c_int, [_P, C.c_char_p, _I64]),
    "cf_get_param": (C.c_int, [_P, C.c_char_p, _PI64]),
    "cf_param_name": (C.c_char_p, [_I32]),
    "cf_comm_init": (C.c_int, [_P, _I32, _I32, C.c_char_p]),
    "cf_comm_free": (C.c_int, [_P]),
    "cf_comm_info": (C.c_int, [_P, C.POINTER(_I32), C.POINTER(_I32)]),
    "cf_comm_allreduce_i64": (C.c_int, [_P, _P, _I64, _I32]),
    "cf_exchange_table": (C.c_int, [_P, _PI64]),
    "cf_allgather_kmers": (C.c_int, [_P, _PI64]),
    "cf_allgather_clouds": (C.c_int, [_P, _PI64]),
    "cf_allreduce_unique": (C.c_int, [_P, _PI64]),
    "cf_selftest_sort": (C.c_int, [_P, _P, _I64, _I32, _P]),
    "cf_selftest_scan": (C.c_int, [_P, _P, _I64, _P]),
    "cf_selftest_scan_inplace": (C.c_int, [_P, _P, _I64, _P]),
    "cf_selftest_scan_u32": (C.c_int, [_P, _P, _I64, _P]),
    "cf_selftest_sort_rec16": (C.c_int, [_P, _P, _I64, _P, _P, _I32, _P]),
    "cf_selftest_digit_offsets": (C.c_int, [_P, _P, _I32, _I32, _P, _P]),
    "cf_selftest_argmax": (C.c_int, [_P, _P, _I64, _P]),
    "cf_selftest_owner_buckets": (C.c_int, [_P, _I32, _P, _P, _P, _I64, _PI64]),
    "cf_selftest_merge_records": (C.c_int, [_P, _P, _P, _I64]),
}

_cache = {}


def load(path=None):
    """Load a build of the device library and bind every prototype (fails loudly)."""
    path = os.path.abspath(path or LIB_PATH)
    if path in _cache:
        return _cache[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension must be built (`make -C centroflye_amd/csrc hip` "
            "or `python -c 'import __graft_entry__ as g; g.build()'`); there is no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _cache[path] = lib
    return lib
