"""Thin numpy-facing wrapper over the C ABI of the device pipeline (include/cfhip.h).

One ``Engine`` = one ``cf_ctx`` = one GPU.  Every method maps 1:1 onto a C entry point; the
mirrors of the reference's modules (``distance_based_kmer_recruitment``, ``read_kmer_cloud``,
``cloud_contig``, ``read_placer``) are written on top of this class.
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib


class DeviceError(RuntimeError):
    pass


def _ptr(a):
    return a.ctypes.data if a is not None else None


class Engine:
    def __init__(self, device=0, lib=None):
        self._lib = lib if lib is not None else _lib.load()
        self._ctx = C.c_void_p()
        rc = self._lib.cf_create(int(device), C.byref(self._ctx))
        if rc != 0:
            msg = self._lib.cf_last_error(self._ctx).decode(errors="replace") if self._ctx else "allocation failed"
            if self._ctx:
                self._lib.cf_destroy(self._ctx)
                self._ctx = C.c_void_p()
            raise DeviceError(f"cf_create({device}) failed ({rc}): {msg}")
        self.k = None
        self.n_reads = 0
        self.n_units = 0

    # ------------------------------------------------------------------ plumbing
    def close(self):
        ctx, self._ctx = getattr(self, "_ctx", None), None
        if ctx:
            self._lib.cf_destroy(ctx)

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise DeviceError(f"{what} failed ({rc}): {self._lib.cf_last_error(self._ctx).decode(errors='replace')}")

    def device_info(self):
        name = C.create_string_buffer(256)
        hbm, cu = C.c_int64(), C.c_int32()
        self._check(self._lib.cf_device_info(self._ctx, name, 256, C.byref(hbm), C.byref(cu)), "cf_device_info")
        return dict(name=name.value.decode(), hbm_bytes=hbm.value, n_cu=cu.value)

    def set_param(self, name, value):
        self._check(self._lib.cf_set_param(self._ctx, name.encode(), int(value)), f"cf_set_param({name})")

    def get_param(self, name):
        v = C.c_int64()
        self._check(self._lib.cf_get_param(self._ctx, name.encode(), C.byref(v)), f"cf_get_param({name})")
        return v.value

    def param_names(self):
        names = []
        while (n := self._lib.cf_param_name(len(names))) is not None:
            names.append(n.decode())
        return names

    @contextlib.contextmanager
    def knobs(self, **settings):
        """Run the body under these knob settings, set in the order given; on the way out, and when a setting is refused,
        every knob set so far gets the value it had before, last set first."""
        saved = [(name, self.get_param(name)) for name in settings]
        done = 0
        try:
            for name, value in settings.items():
                self.set_param(name, value)
                done += 1
            yield self
        finally:
            for name, value in reversed(saved[:done]):
                self.set_param(name, value)

    def stats(self):
        s = _lib.Stats()
        self._check(self._lib.cf_get_stats(self._ctx, C.byref(s)), "cf_get_stats")
        return s.as_dict()

    def times(self):
        t = _lib.Times()
        self._check(self._lib.cf_get_times(self._ctx, C.byref(t)), "cf_get_times")
        return t.as_dict()

    # ------------------------------------------------------------------ A0 hand-over
    def load_arrays(self, bases, read_off, unit_ptr, unit_start, unit_end):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        unit_ptr = np.ascontiguousarray(unit_ptr, dtype=np.int64)
        unit_start = np.ascontiguousarray(unit_start, dtype=np.int64)
        unit_end = np.ascontiguousarray(unit_end, dtype=np.int64)
        R = read_off.size - 1
        if unit_ptr.size != R + 1 or unit_start.size != unit_end.size or (R >= 0 and unit_start.size != unit_ptr[-1]):
            raise ValueError("inconsistent read / unit arrays")
        self._check(self._lib.cf_load_reads(self._ctx, _ptr(bases), _ptr(read_off), R, _ptr(unit_ptr),
                                            _ptr(unit_start), _ptr(unit_end)), "cf_load_reads")
        self.n_reads, self.n_units = R, int(unit_start.size)

    def load(self, packed, n_motif=1):
        """packed: centroflye_amd._host.PackedReads."""
        unit_ptr, unit_start, unit_end, _ = packed.units(n_motif)
        self.load_arrays(packed.bases, packed.read_off, unit_ptr, unit_start, unit_end)

    def load_units(self, unit_ptr, unit_start, unit_end):
        unit_ptr = np.ascontiguousarray(unit_ptr, dtype=np.int64)
        unit_start = np.ascontiguousarray(unit_start, dtype=np.int64)
        unit_end = np.ascontiguousarray(unit_end, dtype=np.int64)
        self._check(self._lib.cf_load_units(self._ctx, _ptr(unit_ptr), _ptr(unit_start), _ptr(unit_end)), "cf_load_units")
        self.n_units = int(unit_start.size)

    # ------------------------------------------------------------------ A1 / A2
    def count_kmers(self, k, read_lo=0, read_hi=None):
        self._check(self._lib.cf_count_kmers(self._ctx, int(k), int(read_lo),
                                             int(self.n_reads if read_hi is None else read_hi)), "cf_count_kmers")
        self.k = int(k)

    def table(self, sort=True):
        """(keys uint64, pres uint32, multi uint32) of every k-mer seen."""
        n = C.c_int64()
        self._check(self._lib.cf_get_table(self._ctx, None, None, None, 0, C.byref(n)), "cf_get_table")
        keys = np.zeros(n.value, np.uint64)
        pres = np.zeros(n.value, np.uint32)
        multi = np.zeros(n.value, np.uint32)
        if n.value:
            self._check(self._lib.cf_get_table(self._ctx, _ptr(keys), _ptr(pres), _ptr(multi), n.value, C.byref(n)), "cf_get_table")
        if sort:
            o = np.argsort(keys, kind="stable")
            keys, pres, multi = keys[o], pres[o], multi[o]
        return keys, pres, multi

    def count_occurrences(self, k, read_lo=0, read_hi=None):
        """Total occurrence counts of every k-mer; table() then returns count = pres | multi << 32."""
        self._check(self._lib.cf_count_occurrences(self._ctx, int(k), int(read_lo),
                                                   int(self.n_reads if read_hi is None else read_hi)), "cf_count_occurrences")
        self.k = int(k)

    def top_kmers(self, n):
        """(keys uint64, counts uint64) of the n k-mers with the largest (count, k-mer), descending."""
        m = C.c_int64()
        self._check(self._lib.cf_top_kmers(self._ctx, int(n), None, None, C.byref(m)), "cf_top_kmers")
        keys = np.zeros(m.value, np.uint64)
        counts = np.zeros(m.value, np.uint64)
        if m.value:
            self._check(self._lib.cf_top_kmers(self._ctx, int(n), _ptr(keys), _ptr(counts), C.byref(m)), "cf_top_kmers")
        return keys, counts

    def rr_distances(self, unit, reads, read_off, threshold):
        """(dist_fwd, dist_rc) int32[n_reads]: minimum edit distance between the unit / its reverse complement and a
        substring of each read, -1 above the threshold (reference rr.cpp:73-90).  reads: uint8 bytes back to back."""
        unit = np.frombuffer(bytes(unit), dtype=np.uint8)
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        read_off = np.ascontiguousarray(read_off, dtype=np.int64)
        n = read_off.size - 1
        fwd = np.zeros(max(n, 0), np.int32)
        rc = np.zeros(max(n, 0), np.int32)
        self._check(self._lib.cf_rr_distances(self._ctx, _ptr(unit), int(unit.size), _ptr(reads) if reads.size else None, _ptr(read_off),
                                              int(n), int(threshold), _ptr(fwd) if n else None, _ptr(rc) if n else None), "cf_rr_distances")
        return fwd, rc

    def reset_table(self, k, expected_keys):
        self._check(self._lib.cf_reset_table(self._ctx, int(k), int(expected_keys)), "cf_reset_table")
        self.k = int(k)

    def table_size(self):
        n = C.c_int64()
        self._check(self._lib.cf_get_table(self._ctx, None, None, None, 0, C.byref(n)), "cf_get_table")
        return n.value

    # raw-pointer variants: the buffers may live on the host or on this GPU (e.g. torch tensors used
    # for the RCCL exchange); the library copies with hipMemcpyDefault
    def table_into(self, keys_ptr, pres_ptr, multi_ptr, cap):
        n = C.c_int64()
        self._check(self._lib.cf_get_table(self._ctx, keys_ptr, pres_ptr, multi_ptr, int(cap), C.byref(n)), "cf_get_table")
        return n.value

    def merge_table_ptr(self, keys_ptr, pres_ptr, multi_ptr, n):
        self._check(self._lib.cf_merge_table(self._ctx, keys_ptr, pres_ptr, multi_ptr, int(n)), "cf_merge_table")

    def kmers_into(self, ptr, cap):
        self._check(self._lib.cf_get_kmers(self._ctx, ptr, int(cap)), "cf_get_kmers")

    def set_kmers_ptr(self, ptr, n, k):
        self._check(self._lib.cf_set_kmers(self._ctx, ptr, int(n), int(k)), "cf_set_kmers")
        self.k = int(k)

    def clouds_into(self, cloud_ptr_ptr, entries_ptr, cap):
        self._check(self._lib.cf_get_clouds(self._ctx, cloud_ptr_ptr, entries_ptr, int(cap)), "cf_get_clouds")

    def set_clouds_ptr(self, cloud_ptr_ptr, entries_ptr, n_entries):
        self._check(self._lib.cf_set_clouds(self._ctx, cloud_ptr_ptr, entries_ptr, int(n_entries)), "cf_set_clouds")

    def unique_mask_into(self, ptr):
        self._check(self._lib.cf_get_unique_mask(self._ctx, ptr), "cf_get_unique_mask")

    def or_unique_mask_ptr(self, ptr):
        self._check(self._lib.cf_or_unique_mask(self._ctx, ptr), "cf_or_unique_mask")

    def merge_table(self, keys, pres, multi):
        keys = np.ascontiguousarray(keys, np.uint64)
        pres = np.ascontiguousarray(pres, np.uint32)
        multi = np.ascontiguousarray(multi, np.uint32)
        self._check(self._lib.cf_merge_table(self._ctx, _ptr(keys), _ptr(pres), _ptr(multi), keys.size), "cf_merge_table")

    def select_rare(self, max_nonuniq, lo, hi):
        n = C.c_int64()
        lo, hi = max(0, int(lo)), int(hi)
        if hi < lo or hi < 0:
            lo, hi = 1, 0
        self._check(self._lib.cf_select_rare(self._ctx, int(max_nonuniq), lo, min(hi, 2 ** 32 - 1), C.byref(n)), "cf_select_rare")
        return n.value

    def set_kmers(self, kmers, k):
        kmers = np.ascontiguousarray(kmers, np.uint64)
        self._check(self._lib.cf_set_kmers(self._ctx, _ptr(kmers), kmers.size, int(k)), "cf_set_kmers")
        self.k = int(k)

    def kmers(self):
        n = self.stats()["n_kmers"]
        out = np.zeros(n, np.uint64)
        self._check(self._lib.cf_get_kmers(self._ctx, _ptr(out), n), "cf_get_kmers")
        return out

    # ------------------------------------------------------------------ A3 / A4
    def build_clouds(self):
        n = C.c_int64()
        self._check(self._lib.cf_build_clouds(self._ctx, C.byref(n)), "cf_build_clouds")
        return n.value

    def filter_clouds(self, min_mult=2, max_mult=0):
        n = C.c_int64()
        self._check(self._lib.cf_filter_clouds(self._ctx, int(min_mult), int(max_mult), C.byref(n)), "cf_filter_clouds")
        return n.value

    def clouds(self):
        """(cloud_ptr int64[U+1], entries int32[N_ce])."""
        n = self.stats()["n_cloud_entries"]
        ptr = np.zeros(self.n_units + 1, np.int64)
        ent = np.zeros(n, np.int32)
        self._check(self._lib.cf_get_clouds(self._ctx, _ptr(ptr), _ptr(ent), n), "cf_get_clouds")
        return ptr, ent

    def set_clouds(self, cloud_ptr, entries):
        cloud_ptr = np.ascontiguousarray(cloud_ptr, np.int64)
        entries = np.ascontiguousarray(entries, np.int32)
        self._check(self._lib.cf_set_clouds(self._ctx, _ptr(cloud_ptr), _ptr(entries), entries.size), "cf_set_clouds")

    # ------------------------------------------------------------------ A5 + A6
    def dist_edges(self, min_n=0, max_n=2 ** 62, min_d=1, max_d=150, min_cov=4, rel_threshold=0.8,
                   part=0, n_parts=1, edge_cap=None):
        n = C.c_int64()
        if edge_cap is None:
            edge_cap = 0
        self._check(self._lib.cf_dist_edges(self._ctx, int(min_n), int(min(max_n, 2 ** 62)), int(min_d), int(max_d),
                                            int(min_cov), float(rel_threshold), int(part), int(n_parts), int(edge_cap),
                                            C.byref(n)), "cf_dist_edges")
        return n.value

    def edges(self, n):
        """The first n stored edges as (n, 4) uint32 rows (d, a, b, cnt)."""
        out = np.zeros((n, 4), np.uint32)
        self._check(self._lib.cf_get_edges(self._ctx, _ptr(out), n), "cf_get_edges")
        return out

    def sort_edges(self):
        """Sort the stored edges by (d, a, b) on the device."""
        self._check(self._lib.cf_sort_edges(self._ctx), "cf_sort_edges")

    def edges_checksum(self, n=2 ** 62):
        """Order-independent checksum of the first n stored edges, computed on the device (see cfhip.h)."""
        out = C.c_uint64()
        self._check(self._lib.cf_edges_checksum(self._ctx, int(n), C.byref(out)), "cf_edges_checksum")
        return int(out.value)

    def checksum(self, what):
        """(sum, items) of the order-independent device-side checksum of "table" (A1), "kmers" (the installed set), "clouds"
        (the CSR) or "unique" (the k-mers whose unique bit is set) — the oracle's figures (cfhip.h: cf_checksum)."""
        out, n = C.c_uint64(), C.c_int64()
        sel = {"table": 0, "kmers": 1, "clouds": 2, "unique": 3}[what]
        self._check(self._lib.cf_checksum(self._ctx, sel, C.byref(out), C.byref(n)), "cf_checksum")
        return int(out.value), int(n.value)

    def unique_mask(self):
        n = self.stats()["n_kmers"]
        out = np.zeros(n, np.uint8)
        self._check(self._lib.cf_get_unique_mask(self._ctx, _ptr(out)), "cf_get_unique_mask")
        return out.astype(bool)

    def or_unique_mask(self, mask):
        mask = np.ascontiguousarray(mask, np.uint8)
        self._check(self._lib.cf_or_unique_mask(self._ctx, _ptr(mask)), "cf_or_unique_mask")

    def reset_unique(self):
        self._check(self._lib.cf_reset_unique(self._ctx), "cf_reset_unique")

    # ------------------------------------------------------------------ multi-GPU
    def comm_init(self, rank, world, rendezvous=None):
        self._check(self._lib.cf_comm_init(self._ctx, int(rank), int(world), (rendezvous or "").encode()), "cf_comm_init")

    def comm_free(self):
        self._check(self._lib.cf_comm_free(self._ctx), "cf_comm_free")

    def comm_info(self):
        r, w = C.c_int32(), C.c_int32()
        self._check(self._lib.cf_comm_info(self._ctx, C.byref(r), C.byref(w)), "cf_comm_info")
        return r.value, w.value

    def allreduce(self, values, op="sum"):
        v = np.ascontiguousarray(values, np.int64).copy()
        self._check(self._lib.cf_comm_allreduce_i64(self._ctx, _ptr(v), v.size, 1 if op == "max" else 0), "cf_comm_allreduce_i64")
        return v

    def exchange_table(self):
        n = C.c_int64()
        self._check(self._lib.cf_exchange_table(self._ctx, C.byref(n)), "cf_exchange_table")
        return n.value

    def allgather_kmers(self):
        n = C.c_int64()
        self._check(self._lib.cf_allgather_kmers(self._ctx, C.byref(n)), "cf_allgather_kmers")
        return n.value

    def allgather_clouds(self):
        n = C.c_int64()
        self._check(self._lib.cf_allgather_clouds(self._ctx, C.byref(n)), "cf_allgather_clouds")
        return n.value

    def allreduce_unique(self):
        n = C.c_int64()
        self._check(self._lib.cf_allreduce_unique(self._ctx, C.byref(n)), "cf_allreduce_unique")
        return n.value

    # ------------------------------------------------------------------ A8 + A9
    def place_reads(self, classes, id_rank, min_cloud_kmer_freq=2, min_unit=2, min_inters=10, min_prop=3):
        """Returns (read, pos, s0, s1) arrays in the order the reference writes read_positions.csv;
        pos = -1 means None; s0 = -1 marks a prefix read (line 'r_id 0')."""
        R = self.n_reads
        classes = np.ascontiguousarray(classes, np.uint8)
        id_rank = np.ascontiguousarray(id_rank, np.int32)
        out_read = np.zeros(R, np.int64)
        out_pos = np.zeros(R, np.int64)
        out_s0 = np.zeros(R, np.int32)
        out_s1 = np.zeros(R, np.int32)
        self._check(self._lib.cf_place_reads(self._ctx, _ptr(classes), _ptr(id_rank), int(min_cloud_kmer_freq), int(min_unit),
                                             int(min_inters), int(min_prop), _ptr(out_read), _ptr(out_pos), _ptr(out_s0),
                                             _ptr(out_s1)), "cf_place_reads")
        return out_read, out_pos, out_s0, out_s1

    # ------------------------------------------------------------------ A10: batch mapping onto a frozen contig
    def contig_build(self, reads, pos, min_cloud_kmer_freq=2):
        """CloudContig(min_cloud_kmer_freq) + add_read(reads[b], pos[b]) for every backbone read, on the current clouds."""
        reads = np.ascontiguousarray(reads, np.int64).reshape(-1)
        pos = np.ascontiguousarray(pos, np.int64).reshape(-1)
        if reads.size != pos.size:
            raise ValueError("one position per backbone read")
        self._check(self._lib.cf_contig_build(self._ctx, _ptr(reads) if reads.size else None, _ptr(pos) if pos.size else None,
                                              reads.size, int(min_cloud_kmer_freq)), "cf_contig_build")

    def contig_info(self):
        """n_positions (P, the distinct covered positions), max_pos, n_freq_kmers, n_pairs, build_ms, map_ms."""
        v = [C.c_int64() for _ in range(4)]
        b, m = C.c_float(), C.c_float()
        self._check(self._lib.cf_contig_info(self._ctx, *[C.byref(x) for x in v], C.byref(b), C.byref(m)), "cf_contig_info")
        return dict(n_positions=v[0].value, max_pos=v[1].value, n_freq_kmers=v[2].value, n_pairs=v[3].value,
                    build_ms=float(b.value), map_ms=float(m.value))

    def contig_coverage(self):
        """int32 coverage of the positions 0 .. max_pos (empty for an empty contig)."""
        info = self.contig_info()
        n = info["max_pos"] + 1 if info["n_positions"] else 0
        cov = np.zeros(n, np.int32)
        self._check(self._lib.cf_contig_coverage(self._ctx, _ptr(cov) if n else None, n), "cf_contig_coverage")
        return cov

    def map_reads(self, reads=None, threshold=(5, 10)):
        """map_reads_fast on the contig of contig_build: (pos int64, s0, s1 int32) per query read (default: every read, in
        order); pos = -1 for a read that does not map."""
        if reads is None:
            n, q = self.n_reads, None
        else:
            q = np.ascontiguousarray(reads, np.int64).reshape(-1)
            n = q.size
        pos = np.full(n, -1, np.int64)
        s0 = np.zeros(n, np.int32)
        s1 = np.zeros(n, np.int32)
        if q is not None and n == 0:      # (a NULL read list means "all reads": an empty one is passed as a list of its own)
            q = np.zeros(1, np.int64)
        self._check(self._lib.cf_map_reads(self._ctx, _ptr(q) if q is not None else None, n, int(threshold[0]), int(threshold[1]),
                                           _ptr(pos) if n else None, _ptr(s0) if n else None, _ptr(s1) if n else None), "cf_map_reads")
        return pos, s0, s1

    def score_reads(self, reads=None, lo=None, hi=None, min_unit=2, min_inters=10):
        """calc_inters_score(read, lo, hi, min_unit, min_inters) on the contig of contig_build, the EXACT scorer (only k-mers
        that are frequent at the position count): (pos int64, s0, s1 int32) per query read (default: every read, in order);
        pos = -1 for None.  lo, hi: one start per query or a scalar; default 0 and max_pos - units + 1 (map_reads' range)."""
        if reads is None:
            n, q = self.n_reads, None
        else:
            q = np.ascontiguousarray(reads, np.int64).reshape(-1)
            n = q.size

        def bound(v):
            if v is None:
                return None
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int64), (n,)) if np.ndim(v) == 0 else v, np.int64).reshape(-1)
            if v.size != n:
                raise ValueError("one first / last start per query read")
            return v if n else np.zeros(1, np.int64)
        lo, hi = bound(lo), bound(hi)
        pos = np.full(n, -1, np.int64)
        s0 = np.zeros(n, np.int32)
        s1 = np.zeros(n, np.int32)
        if q is not None and n == 0:      # (a NULL read list means "all reads": an empty one is passed as a list of its own)
            q = np.zeros(1, np.int64)
        self._check(self._lib.cf_score_reads(self._ctx, _ptr(q) if q is not None else None, n, _ptr(lo) if lo is not None else None,
                                             _ptr(hi) if hi is not None else None, int(min_unit), int(min_inters),
                                             _ptr(pos) if n else None, _ptr(s0) if n else None, _ptr(s1) if n else None), "cf_score_reads")
        return pos, s0, s1

    def contig_spread(self, max_npos=5):
        """get_spread_kmers(max_npos): the ranks (int32, ascending) of the frequent k-mers with more than max_npos positions."""
        n = C.c_int64()
        self._check(self._lib.cf_contig_spread(self._ctx, int(max_npos), None, 0, C.byref(n)), "cf_contig_spread")
        ranks = np.zeros(n.value, np.int32)
        if n.value:
            self._check(self._lib.cf_contig_spread(self._ctx, int(max_npos), _ptr(ranks), ranks.size, C.byref(n)), "cf_contig_spread")
        return ranks

    def contig_exact_info(self):
        """n_exact_pairs (the (k-mer, position) pairs of freq_clouds), score_ms (device time of the last score_reads)."""
        v, m = C.c_int64(), C.c_float()
        self._check(self._lib.cf_contig_exact_info(self._ctx, C.byref(v), C.byref(m)), "cf_contig_exact_info")
        return dict(n_exact_pairs=v.value, score_ms=float(m.value))

    # ------------------------------------------------------------------ the polisher's comparisons (cf_edit.hip)
    def edit_distances(self, data, a_off, b_off, k=2 ** 31 - 1):
        """Global (NW) edit distances of the pairs (data[a_off[p]:a_off[p + 1]], data[b_off[p]:b_off[p + 1]]), -1 above k, in one
        launch: (int32[n_pairs], device ms).  data: bytes / uint8 array, or None for the bytes hpc() left on the device (its
        input followed by its output)."""
        a_off = np.ascontiguousarray(a_off, np.int64).reshape(-1)
        b_off = np.ascontiguousarray(b_off, np.int64).reshape(-1)
        if a_off.size != b_off.size or a_off.size < 1:
            raise ValueError("a_off and b_off have one entry per pair and one more")
        n = a_off.size - 1
        if data is not None:
            data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
            if n and max(int(a_off[-1]), int(b_off[-1])) > data.size:
                raise ValueError("an offset lies beyond the bytes")
            if data.size == 0:
                data = np.zeros(1, np.uint8)
        dist = np.zeros(n, np.int32)
        ms = C.c_float()
        self._check(self._lib.cf_edit_distances(self._ctx, _ptr(data), _ptr(a_off), _ptr(b_off), n, int(k), _ptr(dist) if n else None,
                                                C.byref(ms)), "cf_edit_distances")
        return dist, float(ms.value)

    def hpc(self, data, off):
        """Homopolymer compression of the sequences data[off[s]:off[s + 1]]: (uint8 bytes back to back, int64 offsets).  The
        input and the output stay on the device for edit_distances(None, ...)."""
        data = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
        off = np.ascontiguousarray(off, np.int64).reshape(-1)
        if off.size < 1 or int(off[-1]) > data.size:
            raise ValueError("off has one entry per sequence and one more, all inside the bytes")
        out = np.zeros(max(int(off[-1]), 1), np.uint8)
        out_off = np.zeros(off.size, np.int64)
        self._check(self._lib.cf_hpc(self._ctx, _ptr(data) if data.size else None, _ptr(off), off.size - 1, _ptr(out), _ptr(out_off)), "cf_hpc")
        return out[:int(out_off[-1])], out_off

    def edit_info(self):
        """The shape of the edit-distance kernel: lds_diags (the LDS/HBM switch point of the wavefronts), lane_bytes, turn_bytes,
        block_small, block_big, resident_bytes."""
        v = [C.c_int32() for _ in range(5)]
        r = C.c_int64()
        self._check(self._lib.cf_edit_info(self._ctx, *[C.byref(x) for x in v], C.byref(r)), "cf_edit_info")
        names = ("lds_diags", "lane_bytes", "turn_bytes", "block_small", "block_big")
        return dict({k: x.value for k, x in zip(names, v)}, resident_bytes=r.value)

    # ------------------------------------------------------------------ period, window and hook of raw reads (cf_tandem.hip)
    TANDEM_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.TandemRead._fields_])
    TANDEM_OK, TANDEM_NO_PERIOD, TANDEM_EXOTIC = 0, 1, 2

    def tandem_scan(self, reads, read_off, k=15, bin_size=10):
        """unit_extractor.py's period, best distance window and hook k-mer of every read reads[read_off[i]:read_off[i + 1]] in one
        batch: a structured array (TANDEM_DTYPE: status, n_windows, n_rep_kmers, n_conv, count, bin_left, bin_right, period,
        hook_pos, hook_index, n_hook), one row per read.  A row with status TANDEM_EXOTIC holds nothing else of use: the read has
        bytes other than upper-case ACGT, which centroflye_amd.unit_extractor redoes on the host."""
        reads = np.frombuffer(reads, np.uint8) if isinstance(reads, (bytes, bytearray, memoryview)) else np.ascontiguousarray(reads, np.uint8)
        read_off = np.ascontiguousarray(read_off, np.int64).reshape(-1)
        if read_off.size < 1:
            raise ValueError("read_off has one entry per read and one more")
        if int(read_off.max()) > reads.size:
            raise ValueError("an offset lies beyond the bytes")
        n = read_off.size - 1
        out = np.zeros(n, self.TANDEM_DTYPE)
        self._check(self._lib.cf_tandem_scan(self._ctx, _ptr(reads) if reads.size else None, _ptr(read_off), n, int(k), int(bin_size),
                                             _ptr(out) if n else None), "cf_tandem_scan")
        return out

    def tandem_hook_positions(self):
        """(ptr int64[n_reads + 1], pos int32): the positions of every read's hook k-mer in the last tandem_scan, ascending."""
        n = C.c_int64()
        self._check(self._lib.cf_tandem_hook_positions(self._ctx, None, None, 0, C.byref(n)), "cf_tandem_hook_positions")
        info = self.tandem_info()
        ptr = np.zeros(info["n_reads"] + 1, np.int64)
        pos = np.zeros(max(n.value, 1), np.int32)
        self._check(self._lib.cf_tandem_hook_positions(self._ctx, _ptr(ptr), _ptr(pos), n.value, C.byref(n)), "cf_tandem_hook_positions")
        return ptr, pos[:n.value]

    def tandem_info(self):
        """The shape of cf_tandem.hip (tile sizes, batch size, key layout of the last scan) and the last scan's device
        milliseconds per phase."""
        s = _lib.TandemShape()
        self._check(self._lib.cf_tandem_info(self._ctx, C.byref(s)), "cf_tandem_info")
        d = {n: int(getattr(s, n)) for n, _ in s._fields_ if n != "phase_ms"}
        d["phase_ms"] = dict(zip(("records", "sorts", "runs", "windows", "hook", "total"), (float(x) for x in s.phase_ms)))
        return d

    # ------------------------------------------------------------------ the built-in consensus polisher (cf_consensus.hip)
    def consensus_run(self, templates, t_off, reads, r_off, pos_ptr, n_iters=4, permille=300, support=False):
        """Every position's reads aligned to its template, a vote per column and insertion slot, n_iters passes, all positions in
        one call (the rule: include/cfhip.h at cf_consensus_run).  templates[t_off[p]:t_off[p + 1]] is the template of position p,
        reads[r_off[q]:r_off[q + 1]] read q, pos_ptr a CSR over the reads.  Returns [(bytes uint8, off int64[n_pos + 1], n_voting
        int32[n_pos], n_excluded int32[n_pos]) for iteration 1 .. n_iters]; consensus_info() has the device times.  support=True
        (cf_consensus_run_support) gives the same and keeps what consensus_support() and consensus_reads() hand out."""
        as_u8 = lambda x: np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, np.uint8)
        templates, reads = as_u8(templates), as_u8(reads)
        t_off = np.ascontiguousarray(t_off, np.int64).reshape(-1)
        r_off = np.ascontiguousarray(r_off, np.int64).reshape(-1)
        pos_ptr = np.ascontiguousarray(pos_ptr, np.int64).reshape(-1)
        if t_off.size < 1 or pos_ptr.size != t_off.size:
            raise ValueError("t_off and pos_ptr have one entry per position and one more")
        if r_off.size < 1 or int(pos_ptr[-1]) != r_off.size - 1:
            raise ValueError("r_off has one entry per read of pos_ptr and one more")
        if int(t_off.max()) > templates.size or int(r_off.max()) > reads.size:
            raise ValueError("an offset lies beyond the bytes")
        n_pos, n_iters = t_off.size - 1, int(n_iters)
        totals = np.zeros(max(n_iters, 1), np.int64)
        ms = C.c_float()
        if support:
            self._check(self._lib.cf_consensus_run_support(self._ctx, _ptr(templates) if templates.size else None, _ptr(t_off), _ptr(reads) if reads.size else None,
                                                           _ptr(r_off), _ptr(pos_ptr), n_pos, n_iters, int(permille), 1, _ptr(totals), C.byref(ms)), "cf_consensus_run_support")
        else:
            self._check(self._lib.cf_consensus_run(self._ctx, _ptr(templates) if templates.size else None, _ptr(t_off), _ptr(reads) if reads.size else None,
                                                   _ptr(r_off), _ptr(pos_ptr), n_pos, n_iters, int(permille), _ptr(totals), C.byref(ms)), "cf_consensus_run")
        out = []
        for i in range(n_iters):
            b, off = np.zeros(max(int(totals[i]), 1), np.uint8), np.zeros(n_pos + 1, np.int64)
            nv, ne = np.zeros(max(n_pos, 1), np.int32), np.zeros(max(n_pos, 1), np.int32)
            self._check(self._lib.cf_consensus_get(self._ctx, i + 1, _ptr(b), _ptr(off), _ptr(nv), _ptr(ne)), "cf_consensus_get")
            out.append((b[:int(totals[i])], off, nv[:n_pos], ne[:n_pos]))
        return out

    def consensus_support(self, iter):
        """int32[total bytes of iteration iter]: beside every byte iteration iter (1 .. n_iters) of the last consensus_run(support=True) emitted,
        the tally of the base emitted (0 for a template byte kept with no vote; the rule: include/cfhip.h at cf_consensus_run).  The
        off array of that iteration cuts it per position like the bytes."""
        s = _lib.ConsensusShape()
        self._check(self._lib.cf_consensus_info(self._ctx, C.byref(s)), "cf_consensus_info")
        off = np.zeros(int(s.n_pos) + 1, np.int64)
        self._check(self._lib.cf_consensus_get(self._ctx, int(iter), None, _ptr(off), None, None), "cf_consensus_support")
        agree = np.zeros(max(int(off[-1]), 1), np.int32)
        self._check(self._lib.cf_consensus_support(self._ctx, int(iter), _ptr(agree)), "cf_consensus_support")
        return agree[:int(off[-1])]

    def consensus_reads(self, iter):
        """(dist int32[n_reads], voted bool[n_reads]) of iteration iter (1 .. n_iters) of the last consensus_run(support=True): whether the read
        voted, and its distance to that iteration's template — exact where it voted, -1 where it did not (never established)."""
        s = _lib.ConsensusShape()
        self._check(self._lib.cf_consensus_info(self._ctx, C.byref(s)), "cf_consensus_info")
        n = int(s.n_reads)
        dist, voted = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        self._check(self._lib.cf_consensus_reads(self._ctx, int(iter), _ptr(dist), _ptr(voted)), "cf_consensus_reads")
        return dist[:n], voted[:n].astype(bool)

    def consensus_info(self):
        """The shape of cf_consensus.hip (max_len, block_small / block_big / big_from, launch_cap, batch_bytes, k_ins), the figures
        of the last run (n_pos, n_reads, n_iters, n_batches) and its device milliseconds per phase."""
        s = _lib.ConsensusShape()
        self._check(self._lib.cf_consensus_info(self._ctx, C.byref(s)), "cf_consensus_info")
        d = {n: int(getattr(s, n)) for n, _ in s._fields_ if n != "phase_ms"}
        d["phase_ms"] = dict(zip(("copies", "align", "vote", "compact", "total"), (float(x) for x in s.phase_ms)))
        return d

    # ------------------------------------------------------------------ the built-in tandem aligner (cf_ualign.hip)
    UALIGN_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.UalignHit._fields_])

    def ualign_run(self, unit, reads, read_off, match=10, mismatch=35, gap=33):
        """Every read reads[read_off[i]:read_off[i + 1]] against the unit read cyclically, both strands, the best stretch per read
        (the rule: include/cfhip.h at cf_ualign_run).  Returns (hits, op_ptr, ops): a structured array (UALIGN_DTYPE: status, strand,
        score, r_st, r_en, u_st, m_al_len, n_ops, n_match, n_mismatch, n_ins, n_del), one row per read, and the alignment columns
        as a CSR over the reads (uint8: 0 match, 1 mismatch, 2 read byte against '-', 3 '-' against unit base)."""
        unit = np.frombuffer(bytes(unit), dtype=np.uint8)
        reads = np.frombuffer(reads, np.uint8) if isinstance(reads, (bytes, bytearray, memoryview)) else np.ascontiguousarray(reads, np.uint8)
        read_off = np.ascontiguousarray(read_off, np.int64).reshape(-1)
        if read_off.size < 1:
            raise ValueError("read_off has one entry per read and one more")
        if int(read_off.max()) > reads.size:
            raise ValueError("an offset lies beyond the bytes")
        n = read_off.size - 1
        hits = np.zeros(n, self.UALIGN_DTYPE)
        ms = C.c_float()
        self._check(self._lib.cf_ualign_run(self._ctx, _ptr(unit) if unit.size else None, int(unit.size), _ptr(reads) if reads.size else None,
                                            _ptr(read_off), n, int(match), int(mismatch), int(gap), _ptr(hits) if n else None, C.byref(ms)), "cf_ualign_run")
        ptr, ops = self.ualign_ops()
        return hits, ptr, ops

    def ualign_ops(self):
        """(ptr int64[n_reads + 1], ops uint8): the alignment columns of every read of the last ualign_run, from r_st on."""
        n = C.c_int64()
        self._check(self._lib.cf_ualign_ops(self._ctx, None, None, 0, C.byref(n)), "cf_ualign_ops")
        ptr = np.zeros(self.ualign_info()["n_reads"] + 1, np.int64)
        ops = np.zeros(max(n.value, 1), np.uint8)
        self._check(self._lib.cf_ualign_ops(self._ctx, _ptr(ptr), _ptr(ops), n.value, C.byref(n)), "cf_ualign_ops")
        return ptr, ops[:n.value]

    def ualign_info(self):
        """The shape of cf_ualign.hip (max_unit, cols_per_thread, block, row_chunk, launch_cap, batch_bytes), the figures of the last
        run (n_reads, n_score_pairs, n_move_pairs, n_batches) and its device milliseconds per phase."""
        s = _lib.UalignShape()
        self._check(self._lib.cf_ualign_info(self._ctx, C.byref(s)), "cf_ualign_info")
        d = {n: int(getattr(s, n)) for n, _ in s._fields_ if n != "phase_ms"}
        d["phase_ms"] = dict(zip(("copies", "score", "moves", "total"), (float(x) for x in s.phase_ms)))
        return d

    # ------------------------------------------------------------------ the built-in monomer decomposer (cf_monodec.hip)
    MONODEC_READ_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.MonodecRead._fields_])
    MONODEC_INST_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.MonodecInst._fields_])

    def monodec(self, monomers, reads, read_off, match=1, mismatch=1, gap=1):
        """Every read reads[read_off[i]:read_off[i + 1]] cut into a chain of monomer instances, both strands (the rule: include/cfhip.h at
        cf_monodec_run).  monomers: a list of byte strings of upper-case A, C, G, T.  Returns (info, ptr, inst): a structured array
        (MONODEC_READ_DTYPE: status, strand, score, n_inst, prefix), one row per read, and the instances as a CSR over the reads
        (MONODEC_INST_DTYPE: k, st, en, n_match, n_mismatch, n_ins, n_del), left to right."""
        monomers = [bytes(m) for m in monomers]
        mono = np.frombuffer(b"".join(monomers), dtype=np.uint8)
        mono_off = np.zeros(len(monomers) + 1, np.int64)
        mono_off[1:] = np.cumsum([len(m) for m in monomers], dtype=np.int64)
        reads = np.frombuffer(reads, np.uint8) if isinstance(reads, (bytes, bytearray, memoryview)) else np.ascontiguousarray(reads, np.uint8)
        read_off = np.ascontiguousarray(read_off, np.int64).reshape(-1)
        if read_off.size < 1:
            raise ValueError("read_off has one entry per read and one more")
        if int(read_off.max()) > reads.size:
            raise ValueError("an offset lies beyond the bytes")
        n = read_off.size - 1
        info = np.zeros(n, self.MONODEC_READ_DTYPE)
        ms = C.c_float()
        self._check(self._lib.cf_monodec_run(self._ctx, _ptr(mono) if mono.size else None, _ptr(mono_off), len(monomers),
                                             _ptr(reads) if reads.size else None, _ptr(read_off), n, int(match), int(mismatch), int(gap),
                                             _ptr(info) if n else None, C.byref(ms)), "cf_monodec_run")
        cnt = C.c_int64()
        self._check(self._lib.cf_monodec_get(self._ctx, None, None, 0, C.byref(cnt)), "cf_monodec_get")
        ptr = np.zeros(n + 1, np.int64)
        inst = np.zeros(max(cnt.value, 1), self.MONODEC_INST_DTYPE)
        self._check(self._lib.cf_monodec_get(self._ctx, _ptr(ptr), _ptr(inst), cnt.value, C.byref(cnt)), "cf_monodec_get")
        return info, ptr, inst[:cnt.value]

    def monodec_info(self):
        """The shape of cf_monodec.hip (max_cols, cols_per_thread, block, row_chunk, launch_cap, batch_bytes), the figures of the last
        run (n_reads, n_monomers, n_cols, n_score_pairs, n_move_pairs, n_batches) and its device milliseconds per phase."""
        s = _lib.MonodecShape()
        self._check(self._lib.cf_monodec_info(self._ctx, C.byref(s)), "cf_monodec_info")
        d = {n: int(getattr(s, n)) for n, _ in s._fields_ if n != "phase_ms"}
        d["phase_ms"] = dict(zip(("copies", "score", "moves", "total"), (float(x) for x in s.phase_ms)))
        return d

    # ------------------------------------------------------------------ exact counts of gap-free windows of monostrings (cf_monokmers.hip)
    MONOKMER_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.Monokmer._fields_])
    MONOKMER_OCC_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.MonokmerOcc._fields_])

    def monokmers(self, strings, k, min_mult, positions=False, gap=b"?"):
        """Every k-mer with at least min_mult valid windows over `strings` (a list of byte strings, or (bytes, offsets)), in the order
        of first occurrence (the rule: include/cfhip.h at cf_monokmers_run).  A window is valid when it lies inside one string and
        holds no gap byte.  Returns a structured array (MONOKMER_DTYPE: s, i, count, pos — the first window's string, index and
        offset in the concatenation), one row per k-mer; with positions=True also (ptr int64[n + 1], occ MONOKMER_OCC_DTYPE): every
        valid window of every k-mer, in ascending (s, i)."""
        flat, off = self._flat_strings(strings)
        gap = gap.encode() if isinstance(gap, str) else bytes(gap)
        if len(gap) != 1:
            raise ValueError("the gap is one byte")
        n = C.c_int64()
        self._check(self._lib.cf_monokmers_run(self._ctx, _ptr(flat) if flat.size else None, _ptr(off), off.size - 1, int(k), int(min_mult), gap[0],
                                               1 if positions else 0, C.byref(n), None), "cf_monokmers_run")
        n_occ = C.c_int64()
        self._check(self._lib.cf_monokmers_get(self._ctx, None, 0, C.byref(n), None, None, 0, C.byref(n_occ)), "cf_monokmers_get")
        first = np.zeros(max(n.value, 1), self.MONOKMER_DTYPE)
        if not positions:
            self._check(self._lib.cf_monokmers_get(self._ctx, _ptr(first), n.value, None, None, None, 0, None), "cf_monokmers_get")
            return first[:n.value]
        ptr = np.zeros(n.value + 1, np.int64)
        occ = np.zeros(max(n_occ.value, 1), self.MONOKMER_OCC_DTYPE)
        self._check(self._lib.cf_monokmers_get(self._ctx, _ptr(first), n.value, None, _ptr(ptr), _ptr(occ), n_occ.value, None), "cf_monokmers_get")
        return first[:n.value], ptr, occ[:n_occ.value]

    def monokmers_info(self):
        """The shape constants of cf_monokmers.hip (sort_tile, scan_tile, block, launch_cap), the figures of the last run (n_strings,
        n_letters, k, min_mult, with_positions, n_windows, n_distinct, n_kmers, n_occ, n_rounds, n_sorts, n_sort_passes) and its device
        milliseconds per phase."""
        s = _lib.MonokmersShape()
        self._check(self._lib.cf_monokmers_info(self._ctx, C.byref(s)), "cf_monokmers_info")
        d = {n: int(getattr(s, n)) for n, _ in s._fields_ if n != "phase_ms"}
        d["phase_ms"] = dict(zip(("copies", "sorts", "glue", "total"), (float(x) for x in s.phase_ms)))
        return d

    # ------------------------------------------------------------------ monoreads mapped to the graph's edges (cf_monomap.hip)
    MONOMAP_READ_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.MonomapRead._fields_])
    MONOMAP_HIT_DTYPE = np.dtype([(n, np.int32) for n, _ in _lib.MonomapHit._fields_])

    @staticmethod
    def _flat_strings(strings):
        """a list of byte strings, or (bytes, offsets) -> (uint8 array, int64 offsets)"""
        if isinstance(strings, tuple):
            flat, off = strings
            flat = np.frombuffer(flat, np.uint8) if isinstance(flat, (bytes, bytearray, memoryview)) else np.ascontiguousarray(flat, np.uint8)
            off = np.ascontiguousarray(off, np.int64).reshape(-1)
        else:
            strings = [s.encode() if isinstance(s, str) else bytes(s) for s in strings]
            flat = np.frombuffer(b"".join(strings), dtype=np.uint8)
            off = np.zeros(len(strings) + 1, np.int64)
            off[1:] = np.cumsum([len(s) for s in strings], dtype=np.int64)
        if off.size < 1:
            raise ValueError("the offsets have one entry per string and one more")
        if int(off.max()) > flat.size:
            raise ValueError("an offset lies beyond the bytes")
        return flat, off

    def monomap(self, edges, edge_uv, reads, k, gap=b"?", hits=False):
        """The reads mapped to the edges (the rule: include/cfhip.h at cf_monomap_run).  edges, reads: a list of byte strings, or
        (bytes, offsets); edge_uv: the nodes (u, v) of every edge, an (E, 2) array.  An edge k-mer is indexed when exactly one valid
        edge window holds it; a hit is a valid read window that equals an indexed k-mer.  Returns a structured array per read
        (MONOMAP_READ_DTYPE: n_hits, the first hit e0 j0 i0, the last hit e1 j1 i1 — -1 without a hit —, valid, n_path) and
        (ptr int64[R + 1], path int32): the reads' paths of edge indices; with hits=True also (hptr int64[R + 1], hits
        MONOMAP_HIT_DTYPE): every hit, in ascending i per read."""
        e_flat, e_off = self._flat_strings(edges)
        r_flat, r_off = self._flat_strings(reads)
        n_edges, n_reads = e_off.size - 1, r_off.size - 1
        uv = np.ascontiguousarray(edge_uv, np.int32).reshape(-1, 2)
        if uv.shape[0] != n_edges:
            raise ValueError("one (u, v) per edge")
        u, v = np.ascontiguousarray(uv[:, 0]), np.ascontiguousarray(uv[:, 1])
        gap = gap.encode() if isinstance(gap, str) else bytes(gap)
        if len(gap) != 1:
            raise ValueError("the gap is one byte")
        info = np.zeros(max(n_reads, 1), self.MONOMAP_READ_DTYPE)
        self._check(self._lib.cf_monomap_run(self._ctx, _ptr(e_flat) if e_flat.size else None, _ptr(e_off), _ptr(u) if n_edges else None,
                                             _ptr(v) if n_edges else None, n_edges, _ptr(r_flat) if r_flat.size else None, _ptr(r_off), n_reads,
                                             int(k), gap[0], 1 if hits else 0, _ptr(info), None), "cf_monomap_run")
        n_path, n_hits = C.c_int64(), C.c_int64()
        self._check(self._lib.cf_monomap_get(self._ctx, None, None, 0, C.byref(n_path), None, None, 0, C.byref(n_hits)), "cf_monomap_get")
        ptr = np.zeros(n_reads + 1, np.int64)
        path = np.zeros(max(n_path.value, 1), np.int32)
        if not hits:
            self._check(self._lib.cf_monomap_get(self._ctx, _ptr(ptr), _ptr(path), n_path.value, None, None, None, 0, None), "cf_monomap_get")
            return info[:n_reads], (ptr, path[:n_path.value])
        hptr = np.zeros(n_reads + 1, np.int64)
        hit = np.zeros(max(n_hits.value, 1), self.MONOMAP_HIT_DTYPE)
        self._check(self._lib.cf_monomap_get(self._ctx, _ptr(ptr), _ptr(path), n_path.value, None, _ptr(hptr), _ptr(hit), n_hits.value, None),
                    "cf_monomap_get")
        return info[:n_reads], (ptr, path[:n_path.value]), (hptr, hit[:n_hits.value])

    def monomap_info(self):
        """The shape constants of cf_monomap.hip (sort_tile, scan_tile, block, launch_cap), the figures of the last run (n_edges,
        n_reads, k, with_hits, n_edge_letters, n_read_letters, n_edge_windows, n_indexed, n_hits, n_path, n_rounds, n_sorts) and its
        device milliseconds per phase."""
        s = _lib.MonomapShape()
        self._check(self._lib.cf_monomap_info(self._ctx, C.byref(s)), "cf_monomap_info")
        d = {n: int(getattr(s, n)) for n, _ in s._fields_ if n != "phase_ms"}
        d["phase_ms"] = dict(zip(("copies", "sorts", "glue", "total"), (float(x) for x in s.phase_ms)))
        return d

    # ------------------------------------------------------------------ self tests of primitives
    def selftest_sort(self, keys, bits=64):
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.zeros_like(keys)
        self._check(self._lib.cf_selftest_sort(self._ctx, _ptr(keys), keys.size, int(bits), _ptr(out)), "cf_selftest_sort")
        return out

    def selftest_argmax(self, cands):
        """Winner (s0, s1, offset, rank, index, valid) of the placement's candidate reduction over rows (s0, s1, offset, rank, valid)."""
        cands = np.ascontiguousarray(cands, np.uint32).reshape(-1, 5)
        out = np.zeros(6, np.uint32)
        self._check(self._lib.cf_selftest_argmax(self._ctx, _ptr(cands) if cands.size else None, cands.shape[0], _ptr(out)), "cf_selftest_argmax")
        return out

    def selftest_scan(self, vals):
        vals = np.ascontiguousarray(vals, np.int64)
        out = np.zeros(vals.size + 1, np.int64)
        self._check(self._lib.cf_selftest_scan(self._ctx, _ptr(vals), vals.size, _ptr(out)), "cf_selftest_scan")
        return out

    def selftest_scan_inplace(self, vals):
        """selftest_scan with one device buffer as input and output."""
        vals = np.ascontiguousarray(vals, np.int64)
        out = np.zeros(vals.size + 1, np.int64)
        self._check(self._lib.cf_selftest_scan_inplace(self._ctx, _ptr(vals), vals.size, _ptr(out)), "cf_selftest_scan_inplace")
        return out

    def selftest_scan_u32(self, vals):
        """Exclusive scan of uint32 counts into int64 offsets; the last element is the total."""
        vals = np.ascontiguousarray(vals, np.uint32)
        out = np.zeros(vals.size + 1, np.int64)
        self._check(self._lib.cf_selftest_scan_u32(self._ctx, _ptr(vals), vals.size, _ptr(out)), "cf_selftest_scan_u32")
        return out

    def selftest_sort_rec16(self, recs, words, bits):
        """cf_radix_sort_rec16 of records of four uint32 by the fields (words[f], bits[f]), least significant field first."""
        recs = np.ascontiguousarray(recs, np.uint32).reshape(-1, 4)
        words = np.ascontiguousarray(words, np.int32)
        bits = np.ascontiguousarray(bits, np.int32)
        if words.size != bits.size:
            raise ValueError("one width per field")
        out = np.zeros_like(recs)
        self._check(self._lib.cf_selftest_sort_rec16(self._ctx, _ptr(recs), recs.shape[0], _ptr(words), _ptr(bits), words.size, _ptr(out)),
                    "cf_selftest_sort_rec16")
        return out

    def selftest_digit_offsets(self, hist, n_tiles, D, with_total=True, fill=-1):
        """cf_tile_digit_offsets of the tile-major counts hist (n_tiles x D uint32) -> (offs int64 in the same layout, total or
        None).  offs and the total start as `fill`: what the call does not write keeps it."""
        hist = np.ascontiguousarray(hist, np.uint32).ravel()
        n_tiles, D = int(n_tiles), int(D)
        if hist.size != n_tiles * max(D, 1):
            raise ValueError("hist holds n_tiles x max(D, 1) counts")
        offs = np.full(hist.size, fill, np.int64)
        total = np.full(1, fill, np.int64)
        self._check(self._lib.cf_selftest_digit_offsets(self._ctx, _ptr(hist), n_tiles, D, _ptr(offs), _ptr(total) if with_total else None),
                    "cf_selftest_digit_offsets")
        return offs.reshape(n_tiles, max(D, 1)), (int(total[0]) if with_total else None)

    def selftest_owner_buckets(self, world):
        """The table bucketed for a virtual world, as cf_exchange_table's send buffer: (start int64[world + 1], keys uint64,
        vals uint64 = pres | multi << 32); owner o's records are start[o] .. start[o + 1] - 1."""
        world = int(world)
        n = C.c_int64()
        start = np.zeros(max(world, 0) + 1, np.int64)
        self._check(self._lib.cf_selftest_owner_buckets(self._ctx, world, _ptr(start), None, None, 0, C.byref(n)), "cf_selftest_owner_buckets")
        keys = np.zeros(max(n.value, 1), np.uint64)
        vals = np.zeros(max(n.value, 1), np.uint64)
        self._check(self._lib.cf_selftest_owner_buckets(self._ctx, world, _ptr(start), _ptr(keys), _ptr(vals), n.value, C.byref(n)),
                    "cf_selftest_owner_buckets")
        return start, keys[:n.value], vals[:n.value]

    def selftest_merge_records(self, keys, vals):
        """A fresh table with the records (keys[i], vals[i] = pres | multi << 32) added into it, as the owner's step of
        cf_exchange_table does with what it received; table() reads it."""
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, np.uint64)
        if keys.size != vals.size:
            raise ValueError("one value per key")
        self._check(self._lib.cf_selftest_merge_records(self._ctx, _ptr(keys) if keys.size else None, _ptr(vals) if vals.size else None,
                                                        keys.size), "cf_selftest_merge_records")
