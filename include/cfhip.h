/*
 * cfhip.h — C ABI of libcfhip.so: the MI355X (gfx950) device pipeline of centroflye_amd.
 *
 * This is the drop-in boundary of the hot path.  The reference has no FFI:
 * its stage scripts are pure Python, so the entry points below are what a ctypes binding
 * inside the reference's own functions would call.  Each entry point cites the reference
 * code it replaces (paths relative to the reference repository root):
 *
 *   cf_load_reads      hand-over of what scripts/ncrf_parser.py:61-118 / :28-59 produce
 *   cf_count_kmers     scripts/distance_based_kmer_recruitment.py:39-63  (A1)
 *   cf_select_rare     scripts/distance_based_kmer_recruitment.py:66-82  (A2)
 *   cf_set_kmers       scripts/read_placer.py:20-27 (genomic k-mer set given from a file)
 *   cf_build_clouds    scripts/read_kmer_cloud.py:17-40                  (A3)
 *   cf_filter_clouds   scripts/read_kmer_cloud.py:43-54                  (A4)
 *   cf_dist_edges      scripts/distance_based_kmer_recruitment.py:85-128 (A5) fused with
 *                      :131-149 (A6)
 *   cf_place_reads     scripts/cloud_contig.py:26-41, :87-95 (A8) and
 *                      scripts/read_placer.py:35-94 (A9)
 *   cf_contig_build    scripts/cloud_contig.py:26-41 (CloudContig.add_read for every backbone read)
 *   cf_map_reads       scripts/cloud_contig.py:87-95, :117-156 (map_reads_fast on the finished contig; A10)
 *   cf_score_reads     scripts/cloud_contig.py:46-76 (calc_inters_score), :98-114 (map_reads), :146-155 (debug)
 *   cf_contig_spread   scripts/cloud_contig.py:78-84 (get_spread_kmers)
 *   cf_edit_distances  scripts/eltr_polisher.py:133-146 (compare_polished_sequences: edlib.align in mode NW)
 *   cf_hpc             scripts/utils/bio.py:60-61 (compress_homopolymer), used by eltr_polisher.py:142-143, :151
 *   cf_tandem_scan     scripts/unit_extractor.py:23-89 (get_repetitive_kmers, get_convolution, get_period_info, get_hook_kmer)
 *   cf_consensus_run   stands in for scripts/eltr_polisher.py:99-114 (run_polishing: one Flye process per position); there is
 *                      NO reference function behind it: the rule in the comment at its declaration is the specification
 *
 * Conventions: plain pointers and sizes only; every function returns 0 or a negative
 * errno-style code and never throws or aborts; cf_last_error() gives the message; the
 * caller allocates every output buffer; the opaque context owns all device memory; one
 * context per process and device, calls serialised by the caller; one HIP stream inside.
 * Host pointers are borrowed for the duration of the call only.
 *
 * k-mers are 2-bit packed, A=0 C=1 G=2 T=3, first base in the most significant position, so
 * unsigned integer order equals the string order the reference sorts by.  Forward strand
 * only — the reference never canonicalises.  1 <= k <= 31.
 */
#ifndef CFHIP_H
#define CFHIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct cf_ctx cf_ctx;

/* Work counters; the counters of the reference's algorithm (n_bases ... n_unique) are identical for the oracle and
 * the HIP path on one input; table_capacity, n_spilled, hbm_bytes_live, n_dist_passes and n_edges_stored describe the device run
 * (n_dist_passes and n_spilled depend on how workgroups interleave and may differ by a few between two runs). */
typedef struct cf_stats {
    int64_t n_reads, n_bases, n_units;
    int64_t n_windows;      /* N_w  = sum max(0, len - k + 1)                       */
    int64_t n_read_kmers;   /* N_rk = sum over reads of #distinct k-mers             */
    int64_t n_distinct;     /* K_dist = distinct k-mers seen                         */
    int64_t n_kept;         /* k-mers surviving the multi-occurrence cut             */
    int64_t n_kmers;        /* size of the current k-mer set (rare / genomic)        */
    int64_t n_cloud_entries;/* N_ce                                                  */
    int64_t n_emissions;    /* E = pair emissions of the last cf_dist_edges          */
    int64_t n_edges;        /* selected edges of the last cf_dist_edges              */
    int64_t n_unique;       /* selected ("unique") k-mers so far                     */
    int64_t table_capacity; /* slots of the HBM k-mer table                          */
    int64_t n_spilled;      /* first k-mers whose (b,d) table had to be partitioned  */
    int64_t hbm_bytes_live; /* device memory currently owned by the context          */
    int64_t n_dist_passes;  /* (first k-mer, partition) table passes of the last cf_dist_edges */
    int64_t n_edges_stored; /* edge rows of the last cf_dist_edges held on the device: n_edges when edge_cap allowed it, else at most edge_cap */
} cf_stats;

/* Device time (HIP events on the context's stream) of the last call of each stage. */
typedef struct cf_times {
    float load_ms, count_ms, select_ms, clouds_ms, filter_ms, postings_ms, dist_ms, place_ms;
    float dist_kernel_ms;   /* the cf_dist_edges main kernel alone                          */
    float count_kernel_ms;  /* the cf_count_kmers main kernel alone                         */
    float rr_kernel_ms;     /* the cf_rr_distances kernel alone                             */
} cf_times;

int  cf_create(int device, cf_ctx** out);
void cf_destroy(cf_ctx* ctx);
const char* cf_last_error(const cf_ctx* ctx);
int  cf_device_info(cf_ctx* ctx, char* name, int name_len, int64_t* hbm_bytes, int32_t* n_cu);

/* Reads: ASCII bases, read_off[R+1]; units: unit_ptr[R+1] indexes global units, unit_start/unit_end are absolute
 * offsets into bases.  Symbols other than upper-case A, C, G, T are allowed: cf_count_kmers skips the windows that hold
 * one (the reference counts those as k-mers of their own, distance_based_kmer_recruitment.py:47-53 — the host side-path
 * cfh_exotic_summary of cfhost.h keeps that count and tells whether any of them could matter downstream), and
 * cf_build_clouds upper-cases a, c, g, t first, as read_kmer_cloud.py:25 does. */
int cf_load_reads(cf_ctx* ctx, const uint8_t* bases, const int64_t* read_off, int64_t n_reads,
                  const int64_t* unit_ptr, const int64_t* unit_start, const int64_t* unit_end);
/* Replace the unit table only (n_motif change). */
int cf_load_units(cf_ctx* ctx, const int64_t* unit_ptr, const int64_t* unit_start, const int64_t* unit_end);

/* A1: presence / multi-occurrence table over the reads [read_lo, read_hi) (the whole set when
 * read_lo = 0, read_hi >= R). */
int cf_count_kmers(cf_ctx* ctx, int32_t k, int64_t read_lo, int64_t read_hi);
/* SURVEY §8(f) rank 2 (scripts/better_consensus_unit_reconstruction.py:127-135, :156-167): table of total
 * OCCURRENCE counts (every window of every read counts; val is one 64-bit count, cf_get_table returns its low /
 * high halves in pres / multi), and the n k-mers with the largest (count, k-mer), sorted descending
 * (size-query with keys_out == NULL: n_out = min(n, distinct)). */
int cf_count_occurrences(cf_ctx* ctx, int32_t k, int64_t read_lo, int64_t read_hi);
int cf_top_kmers(cf_ctx* ctx, int64_t n, uint64_t* keys_out, uint64_t* counts_out, int64_t* n_out);
/* Start an empty table for keys of length k sized for about expected_keys distinct k-mers (owner side of
 * the multi-GPU exchange, followed by cf_merge_table). */
int cf_reset_table(cf_ctx* ctx, int32_t k, int64_t expected_keys);
/* Dump the occupied slots, unordered (tests, multi-GPU merge): size-query with keys == NULL. */
int cf_get_table(cf_ctx* ctx, uint64_t* keys, uint32_t* pres, uint32_t* multi, int64_t cap, int64_t* n_out);
/* Add (key, pres, multi) triples into the table (owner-side merge of the multi-GPU exchange). */
int cf_merge_table(cf_ctx* ctx, const uint64_t* keys, const uint32_t* pres, const uint32_t* multi, int64_t n);

/* A2: k-mer set := { x : multi[x] <= max_nonuniq, lo <= pres[x] <= hi }, sorted ascending. */
int cf_select_rare(cf_ctx* ctx, int32_t max_nonuniq, uint32_t lo, uint32_t hi, int64_t* n_out);
/* Install a k-mer set (sorted ascending, unique). */
int cf_set_kmers(cf_ctx* ctx, const uint64_t* kmers, int64_t n, int32_t k);
int cf_get_kmers(cf_ctx* ctx, uint64_t* out, int64_t cap);

/* A3: per-unit clouds of the current k-mer set as CSR (entries = indices into the set, sorted
 * unique inside each unit).  A unit may hold at most 6144 distinct set k-mers: clouds of up to 1536 are built with a
 * 2048-slot LDS set, a larger one makes the call repeat the launch with 8192 slots, and beyond 6144 it returns -34
 * (no clouds are installed; the context stays usable). */
int cf_build_clouds(cf_ctx* ctx, int64_t* n_entries);
/* A4: keep k-mers present in [min_mult, max_mult] clouds overall (max_mult = 0: no upper bound). */
int cf_filter_clouds(cf_ctx* ctx, uint32_t min_mult, uint32_t max_mult, int64_t* n_entries);
int cf_get_clouds(cf_ctx* ctx, int64_t* cloud_ptr /* U+1 */, int32_t* entries, int64_t cap);
/* Install clouds computed elsewhere (multi-GPU all-gather of per-shard clouds; hand-built clouds of tests).  Any CSR over the loaded
 * units is taken as it is and nothing is checked, so the caller has to keep: cloud_ptr (U + 1 values) starts at 0, never decreases
 * and ends at n_entries; every entry is a rank < n_kmers of the installed k-mer set; a rank occurs at most once per cloud (the
 * placement's "at most two hits per k-mer and score cell" and "nobody else lays this (k-mer, position) pair down in this launch" and
 * the distance stage's tail items rest on it; cf_dist_edges notices a repeated rank, cf_place_reads does not).  A cloud MAY hold more
 * entries than its unit has bases: the call measures the largest cloud and the most entries of one read, and cf_place_reads goes by
 * those figures (below). */
int cf_set_clouds(cf_ctx* ctx, const int64_t* cloud_ptr, const int32_t* entries, int64_t n_entries);

/* A5+A6: for first k-mers a with a % n_parts == part: histogram over (b, d) of the reads
 * [min_n, max_n), then keep (d, a, b, cnt) with cnt >= min_cov and
 * (double)cnt / (double)sum_d cnt >= rel_threshold.  Up to edge_cap edges are stored on the
 * device (all are counted); the unique-k-mer bitmap accumulates across calls until
 * cf_reset_unique().
 * A call that fails leaves NO launch behind: n_edges, n_emissions, n_dist_passes, n_spilled and n_edges_stored of cf_stats are 0,
 * cf_get_edges, cf_sort_edges and cf_edges_checksum see no stored edge (cf_get_edges copies nothing), *n_edges is not written, and
 * the edges of an earlier call are gone too (a failed launch may have written over them).  The context stays usable and owns no
 * more memory than after the same call failing once before.  Most failures (-22, -34: the input does not fit a layout or a field)
 * come before anything runs.  One comes from the kernel itself, after it has run to its end: -34 "cf_dist_edges: (b,d) table could
 * not be partitioned far enough" — one partner b has more distinct distances under one first k-mer than a partition of the LDS table
 * may hold, and the table is split by bits of b, which keeps the keys of one b together however far it goes (a larger "dist_slots",
 * or the default table, takes such an input).  After THAT failure the unique-k-mer bitmap may hold bits of the first k-mers that did
 * fit: call cf_reset_unique() and run the parts again before the bitmap is used. */
int cf_dist_edges(cf_ctx* ctx, int64_t min_n, int64_t max_n, int32_t min_d, int32_t max_d,
                  uint32_t min_cov, double rel_threshold, int32_t part, int32_t n_parts,
                  int64_t edge_cap, int64_t* n_edges);
int cf_get_edges(cf_ctx* ctx, uint32_t* out /* n x 4: d, a, b, cnt */, int64_t cap);   /* the first min(cap, stored) edges */
/* Sort the stored edges by (d, a, b) on the device (they are written in the order workgroups finish; the reference's file
 * order, distance_based_kmer_recruitment.py:165-171, is the insertion order of its dicts and is not reproduced).  Only
 * meaningful when every selected edge was stored (edge_cap >= n_edges of the last cf_dist_edges call). */
int cf_sort_edges(cf_ctx* ctx);
/* Order-independent checksum of the first min(n, stored) edges, computed on the device: the sum over rows (d, a, b, cnt) of
 * mix(mix(mix(mix(d + 0x9E37) ^ a) ^ (b << 1)) ^ (cnt << 2)) mod 2^64 with the 64-bit finaliser of MurmurHash3 as mix (the
 * same figure the oracle reports; full-size parity checks compare every selected edge of
 * distance_based_kmer_recruitment.py:131-149 without copying tens of GB to the host). */
int cf_edges_checksum(cf_ctx* ctx, int64_t n, uint64_t* out);
/* Order-independent checksums of the other resident results, computed on the device (sums mod 2^64 of the oracle's per-element
 * mixes, oracle/c/cf_oracle_mt.c; mix = the 64-bit finaliser of MurmurHash3): what =
 *   CF_CHECKSUM_TABLE   every (key, pres, multi) of the A1 table (distance_based_kmer_recruitment.py:39-63):
 *                       mix(mix(mix(key + 0x7AB1E) ^ pres) ^ (multi << 1));
 *   CF_CHECKSUM_KMERS   the installed k-mer set, after cf_select_rare the rare set (:66-82): mix(kmer ^ 0xABCDEF);
 *   CF_CHECKSUM_CLOUDS  every (unit, entry) of the cloud CSR (read_kmer_cloud.py:17-40): mix(mix(unit + 0x51ED) ^ entry);
 *   CF_CHECKSUM_UNIQUE  the k-mers of the set whose unique bit is set (:145-148), same mix as CF_CHECKSUM_KMERS.
 * n_items (may be NULL): how many elements went into the sum.  Full-size parity checks (BASELINE configs[3]: 1.3e9 table
 * entries, 6.5e8 cloud entries) compare these figures with a committed oracle record instead of copying the arrays back. */
enum { CF_CHECKSUM_TABLE = 0, CF_CHECKSUM_KMERS = 1, CF_CHECKSUM_CLOUDS = 2, CF_CHECKSUM_UNIQUE = 3 };
int cf_checksum(cf_ctx* ctx, int32_t what, uint64_t* sum, int64_t* n_items);
int cf_get_unique_mask(cf_ctx* ctx, uint8_t* mask /* n_kmers bytes of 0/1 */);
int cf_or_unique_mask(cf_ctx* ctx, const uint8_t* mask);
int cf_reset_unique(cf_ctx* ctx);

/* A8+A9: greedy placement.  cls[r]: 0 prefix, 1 internal, 2 suffix; id_rank[r] = rank of the
 * read id in ascending string order (tie-break).  Outputs, in the order the reference writes
 * the file: out_read[i], out_pos[i] (-1 = None), out_s0[i], out_s1[i] for i < R.
 * Counter widths.  The per-read score regions ("place_mode" 2 and 3) count the hits of one (read, offset, unit) in 16 bits — at most
 * two per entry of the unit's cloud and stage, so clouds of up to 32 767 entries fit — and a read's cloud entries in 24 bits.  Both are
 * checked against the installed clouds (cf_build_clouds: bounded by the longest unit; cf_set_clouds: measured): a read set beyond them
 * takes the hash-map path under mode 2, as one with small thresholds does, and returns -34 with the reason under mode 3.  The hash-map
 * path ("place_mode" 1) keeps s0, s1 and the contig's counts in 32 bits each: s0 <= units of a read, s1 <= 2 x cloud entries of a read,
 * a count <= reads — nothing that can be loaded overflows them. */
int cf_place_reads(cf_ctx* ctx, const uint8_t* cls, const int32_t* id_rank, int32_t min_cloud_kmer_freq,
                   int32_t min_unit, int32_t min_inters, int32_t min_prop,
                   int64_t* out_read, int64_t* out_pos, int32_t* out_s0, int32_t* out_s1);

/* A10: batch mapping onto a frozen contig (cf_map.hip).
 * cf_contig_build = CloudContig(min_cloud_kmer_freq) followed by add_read(reads[b], pos[b]) for b < n (cloud_contig.py:9-41; the
 * order plays no part in what is kept): on the current clouds, count[(p, x)] = backbone reads whose unit i holds k-mer x with
 * pos + i == p; x is frequent when count[(p, x)] >= max(1, min_cloud_kmer_freq) at some p (:35-37); the contig keeps EVERY position
 * of every frequent k-mer (kmer_positions, :33), the coverage of each position (:30) and max_pos (:20-24).  reads: distinct indices
 * < R; pos >= 0; pos + units < 2^31; n = 0 gives a valid empty contig.  Errors (-22: duplicate or out-of-range reads, negative or
 * too large positions, no clouds) leave the previous contig and the context as they were.  cf_build_clouds, cf_filter_clouds,
 * cf_set_clouds, cf_set_kmers, cf_load_units and cf_load_reads drop the contig.
 * cf_contig_info: n_positions = P = len(cloud_contig.clouds), the DISTINCT covered positions (a unit with an empty cloud covers its
 * position, :31; P < max_pos + 1 when the coverage has a gap); max_pos (0 for an empty contig); n_freq_kmers = len(freq_kmers);
 * n_pairs = the (k-mer, position) pairs map_reads_fast seeds from (:125-128); build_ms / map_ms = device time (HIP events) of the
 * last cf_contig_build / cf_map_reads (map_ms 0 before the first).  Any pointer may be NULL.
 * cf_contig_coverage: cov[p] for p <= max_pos (cap >= max_pos + 1; nothing is written for an empty contig).
 * cf_map_reads = map_reads_fast(cloud_contig, reads, threshold = (t0, t1)) (:117-156) for the n query reads (reads == NULL: all R
 * reads in order, n is ignored): for every frequent x, every position q of x and every (unit i of the read) holding x with q >= i,
 * scores[q - i][i] += 1 (:87-95); among the starts s with s + units <= P (:135), s0 = units with a hit >= t0 and s1 = hits >= t1
 * (:137-139) the maximum of (s0, s1, s) wins (:140-143).  out_pos = -1 (and s0 = s1 = 0) for a read with no such start.  A query
 * read that is part of the backbone counts its own k-mers, as in the reference.  -22 before a contig exists. */
int cf_contig_build(cf_ctx* ctx, const int64_t* reads, const int64_t* pos, int64_t n, int32_t min_cloud_kmer_freq);
int cf_contig_info(cf_ctx* ctx, int64_t* n_positions, int64_t* max_pos, int64_t* n_freq_kmers, int64_t* n_pairs, float* build_ms,
                   float* map_ms);
int cf_contig_coverage(cf_ctx* ctx, int32_t* cov, int64_t cap);
int cf_map_reads(cf_ctx* ctx, const int64_t* reads, int64_t n, int32_t t0, int32_t t1, int64_t* out_pos, int32_t* out_s0,
                 int32_t* out_s1);

/* A10, the exact scorer (cf_score.hip).  cf_contig_build also keeps freq_clouds (cloud_contig.py:35-36): F(p) = { x :
 * count[(p, x)] >= max(1, min_cloud_kmer_freq) }, the k-mers that are frequent AT p — not every position of a frequent k-mer,
 * which is what cf_map_reads seeds from.
 * cf_score_reads = calc_inters_score(read, min_position = lo[j], max_position = hi[j], min_unit, min_inters) (:46-76) for the n
 * query reads (reads == NULL: all R reads in order, n is ignored; lo == NULL: 0; hi == NULL: max_pos - units + 1 per read, the
 * range of map_reads, :103).  The score of a read of `units` units at start s: for i < min(units, max_pos - s + 1) (:57: a read
 * that overhangs max_pos is truncated, not refused; the limit is max_pos, never P), h_i = |cloud_i & F(s + i)|, s0 = #{i :
 * h_i >= 1}, s1 = sum h_i (:60-66).  A start beyond max_pos scores (0, 0).  Among the starts lo <= s <= hi with s0 >= min_unit and
 * s1 >= min_inters the maximum of (s0, s1, s) wins (:71-75, `>=`: the rightmost of equals).  Starts without a hit take part: with
 * min_unit <= 0 and min_inters <= 0 a read with no hit, or with no units, gets out_pos = hi and the score (0, 0).  out_pos = -1
 * (s0 = s1 = 0) stands for None: no start qualifies, or lo > hi.  hi may lie beyond max_pos.  Defined here: lo < 0 is refused.
 * map_reads (:98-114) is cf_score_reads with lo = hi = NULL and (min_unit, min_inters) = (2, 10), whatever its threshold is,
 * followed on the host by: keep the read iff out_pos == 0 or (s0, s1) > threshold (a strict tuple compare, :107).
 * Errors (-22: no contig, a read out of range, lo < 0) leave the context and the contig as they were.
 * cf_contig_spread = get_spread_kmers(max_npos) (:78-84): the ranks of the frequent k-mers with more than max_npos positions in
 * kmer_positions (ALL their positions, the pairs cf_map_reads seeds from), ascending.  *n_out = their number; ranks == NULL asks
 * for the number alone; otherwise cap >= *n_out ranks are written (-22, with *n_out set, when they do not fit).
 * cf_contig_exact_info: n_exact_pairs = sum over p of |F(p)|; score_ms = device time (HIP events) of the last cf_score_reads (0
 * before the first).  Either pointer may be NULL. */
int cf_score_reads(cf_ctx* ctx, const int64_t* reads, int64_t n, const int64_t* lo, const int64_t* hi, int32_t min_unit,
                   int32_t min_inters, int64_t* out_pos, int32_t* out_s0, int32_t* out_s1);
int cf_contig_spread(cf_ctx* ctx, int64_t max_npos, int32_t* ranks, int64_t cap, int64_t* n_out);
int cf_contig_exact_info(cf_ctx* ctx, int64_t* n_exact_pairs, float* score_ms);

/* The polisher's comparisons (cf_edit.hip; eltr_polisher.py:133-165).
 * cf_edit_distances: the global (NW) unit-cost edit distance of n_pairs pairs of byte strings in one launch: pair p compares
 * bytes[a_off[p], a_off[p + 1]) with bytes[b_off[p], b_off[p + 1]) (both offset arrays have n_pairs + 1 non-decreasing entries >= 0;
 * the two may overlap, e.g. a_off = off, b_off = off + 1 compares every sequence with its successor; the bytes end at the larger
 * of the two last offsets).  Equality is byte equality (N == N, a != A).  k >= 0 bounds the distance as edlib's k does: dist[p] =
 * -1 when the distance exceeds k.  An empty string is allowed (the distance is the other one's length); a string holds at most
 * 2^31 - 256 bytes.  bytes == NULL compares strings of the bytes cf_hpc left on the device: its input followed directly by its
 * output, so offset off[n_seqs] + out_off[s] is where compressed sequence s begins.  *ms (may be NULL): device milliseconds of
 * the call, copies included, by HIP events; nothing is added to cf_times or cf_stats.  One workgroup per pair finds the distance
 * d by furthest-reaching points on diagonals, O(n + m + d^2) work; its wavefronts live in LDS up to the switch point that
 * cf_edit_info reports, in HBM beyond.  n_pairs = 0 is allowed.  Errors (-22: a negative k or count, null or decreasing
 * offsets, no bytes) leave the context as it was.
 * cf_hpc: homopolymer compression of n_seqs sequences back to back (off[0] = 0, off[n_seqs + 1] non-decreasing): byte i of a
 * sequence is kept iff i == 0 or s[i] != s[i - 1].  out_bytes: room for off[n_seqs] bytes (the compressed sequences back to
 * back), out_off[n_seqs + 1] their offsets.  The input and the output stay on the device until the next cf_hpc or cf_destroy.
 * cf_edit_info: lds_diags = the switch point: a pair whose band has more diagonals keeps its wavefronts in HBM (knob
 * "edit_lds_diags"; a band has at most min(k, max(n, m)) + 1 diagonals); lane_bytes = the bytes a lane compares on its own before
 * the wave takes the run over; turn_bytes = the bytes a wave compares per ballot; block_small / block_big = threads per
 * workgroup for bands of up to / more than 2048 diagonals; resident_bytes = the bytes cf_hpc left.  Any pointer may be NULL. */
int cf_edit_distances(cf_ctx* ctx, const uint8_t* bytes, const int64_t* a_off, const int64_t* b_off, int64_t n_pairs, int32_t k,
                      int32_t* dist, float* ms);
int cf_hpc(cf_ctx* ctx, const uint8_t* bytes, const int64_t* off, int64_t n_seqs, uint8_t* out_bytes, int64_t* out_off);
int cf_edit_info(cf_ctx* ctx, int32_t* lds_diags, int32_t* lane_bytes, int32_t* turn_bytes, int32_t* block_small, int32_t* block_big,
                 int64_t* resident_bytes);

/* The HOR period and unit of raw reads (cf_tandem.hip; scripts/unit_extractor.py:23-97), every read of the call in one batch.
 * cf_tandem_scan: reads = n_reads byte strings back to back, read_off[n_reads + 1] non-decreasing and >= 0 (the layout of
 * cf_rr_distances).  1 <= k <= 31, bin_size >= 0, a read holds fewer than 2^31 bases; distances and counts are int32.  Per read,
 * with the repetitive k-mers = the k-mers with two or more start positions, conv = the differences of consecutive positions of
 * every such k-mer sorted ascending (n_conv of them), r(l) = the first index whose distance exceeds conv[l] + 2 bin_size:
 *   n_windows     window starts l = 0, 1, .. the reference's loop visits: up to the first l with r(l) = n_conv
 *   count         C = the largest r(l) - l among them; bin_left = conv[l*], bin_right = conv[r(l*) - 1] for the FIRST l* with count C
 *   period        periods[0] of get_period_info: the median (conv[mid] for an odd count, the floored mean of the two middle
 *                 distances for an even one) of the LAST visited window with count C
 *   hook_index    the largest number of one k-mer's distances inside [bin_left, bin_right] (closed); hook_pos = the first position
 *                 of that k-mer, ties to the k-mer that occurs first; n_hook = its positions (cf_tandem_hook_positions has them)
 * status: CF_TANDEM_OK; CF_TANDEM_NO_PERIOD = no k-mer repeats (shorter than k included): every other field but n_rep_kmers and
 * n_conv (both 0) is 0 and hook_pos -1; CF_TANDEM_EXOTIC = some window holds a byte that is not upper-case A, C, G, T: the device
 * skipped those windows and the other fields must not be used (the reference compares raw strings: centroflye_amd/unit_extractor.py
 * redoes such reads on the host).  n_reads = 0 is allowed.  Device time goes to cf_tandem_info, nothing is added to cf_times or
 * cf_stats.  Errors (-22: a negative count, decreasing offsets, k < 1, k > 31, bin_size < 0, null pointers, a read of 2^31 bases,
 * keys forced where one read alone does not fit them) leave the context and the results of the call before as they were.
 * cf_tandem_hook_positions: the hook's positions of every read of the last cf_tandem_scan as a CSR: ptr[n_reads + 1], pos[ptr[n_reads]]
 * ascending inside a read.  *n_out = the number of positions; ptr == pos == NULL asks for it alone; otherwise cap >= *n_out.
 * cf_tandem_info: the shape the tests straddle and the last scan's figures.  Records are sorted on (read, code) only; a stable
 * sort keeps the positions of a (read, code) run ascending.  key_mode 1: 64-bit keys [position | invalid | read in batch | code]
 * with the position starting at bit pos_shift (a multiple of 8: the sort works on whole bytes); key_mode 2: 16-byte records
 * {code low, code high, read, position}.  A batch is a range of whole reads of at most batch_windows windows (knob
 * "tandem_batch_windows", 0 = 2^26) and, unless records are forced, of few enough reads for the keys; knob "tandem_key_mode": 0
 * = keys where they fit, 1 = keys or -22, 2 = records.  phase_ms: records, sorts, runs and distances, windows, hook, and the whole
 * call with its copies, by HIP events, summed over the batches of the last scan. */
enum { CF_TANDEM_OK = 0, CF_TANDEM_NO_PERIOD = 1, CF_TANDEM_EXOTIC = 2 };
typedef struct cf_tandem_read {
    int32_t status, n_windows, n_rep_kmers, n_conv, count, bin_left, bin_right, period, hook_pos, hook_index, n_hook;
} cf_tandem_read;
typedef struct cf_tandem_shape {
    int64_t sort_tile, rec_tile, scan_tile, block; /* keys / records / scan entries per tile, threads per workgroup */
    int64_t batch_windows;                         /* windows per batch in force                                   */
    int64_t key_mode, code_bits, read_bits, pos_bits, pos_shift; /* layout of the last batch of the last scan      */
    int64_t n_batches, n_key_batches, n_records, n_reads; /* of the last scan                                   */
    float phase_ms[6];
} cf_tandem_shape;
int cf_tandem_scan(cf_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int32_t k, int32_t bin_size,
                   cf_tandem_read* out);
int cf_tandem_hook_positions(cf_ctx* ctx, int64_t* ptr, int32_t* pos, int64_t cap, int64_t* n_out);
int cf_tandem_info(cf_ctx* ctx, cf_tandem_shape* out);

/* The built-in consensus polisher (cf_consensus.hip).  It stands in for the step of scripts/eltr_polisher.py:99-114 (run_polishing:
 * one `flye --polish-target` process per contig position) and has NO reference function behind it: it is not Flye's polisher
 * and does not claim Flye's output.  The rule below is the specification (tests/conscheck.py restates it).
 * cf_consensus_run: n_pos positions; the template of position p is templates[t_off[p], t_off[p + 1]), its reads are the reads
 * pos_ptr[p] .. pos_ptr[p + 1] - 1 (a CSR over the reads, pos_ptr[0] = 0), read q is reads[r_off[q], r_off[q + 1]); all three
 * offset arrays are non-decreasing and >= 0, a string holds at most max_len bytes (cf_consensus_info).  One pass, per position
 * with template t (length m) and reads r_1 .. r_c:
 *   1. D = the full unit-cost NW matrix of (t, r) (byte equality, as cf_edit_distances), d = D[m][n]; the alignment is the walk
 *      back from (m, n) that at (i, j) takes (a) the diagonal if i, j > 0 and D[i-1][j-1] + (t[i-1] != r[j-1]) == D[i][j]: the
 *      read byte r[j-1] sits on column i - 1; (b) else, if i > 0 and D[i-1][j] + 1 == D[i][j], column i - 1 is deleted in
 *      this read; (c) else r[j-1] is an inserted byte of slot i (slot s lies before column s, slot m behind the last column).
 *   2. A read votes iff 1000 d <= permille m; c_v = the voting reads; c_v == 0 leaves t as it is.
 *   3. Column i: a byte A, C, G or T on the diagonal votes for its base, any other byte casts no vote, a deletion votes
 *      "deleted".  Slot s: the k-th byte (k = 0 .. 3) of the read's inserted run, in read order, votes for its base at (s, k) if
 *      it is A, C, G or T; bytes from the fifth on cast no vote (a pass adds at most 4 bases per slot).
 *   4. For s = 0 .. m: for k = 0 .. 3, with v the sum of the four tallies of (s, k): 2 v > c_v emits the base with the largest
 *      tally (ties: the first of A < C < G < T), anything else ends the slot.  Then, for s < m, column s: t[s] if all five
 *      tallies are 0; else the largest tally, a tie going to t[s] if it is one of the tied bases, else to the first of A, C, G,
 *      T, deleted; "deleted" emits nothing.
 * Iteration i has the output of iteration i - 1 as its template; all n_iters (>= 1) outputs of all positions are produced by
 * the one call and stay in the context (host memory) for cf_consensus_get.  total_bytes_out[n_iters] (may be NULL): the bytes
 * of every iteration's output; *ms_out (may be NULL): device milliseconds of the call, copies included.  Per pair the device
 * fills the band |j - i| <= w of D by anti-diagonals, w doubling from the distance of the iteration before until D[m][n] <= w
 * (then the band holds every cell of the walk) or w reaches floor(permille m / 1000) (then the read does not vote), writes
 * the move of every cell (2 bits) to the pair's area of scratch, and walks back; pairs go through in batches whose areas stay
 * under the knob "cons_batch_bytes".  Nothing is added to cf_times or cf_stats.  Errors (-22: null pointers, decreasing or negative
 * offsets, pos_ptr[0] != 0, n_pos < 0, n_iters < 1, a negative permille, a string longer than max_len, given or grown) leave
 * the context and the results of the call before as they were.
 * cf_consensus_get: the output of iteration iter (1 .. n_iters) of the last run: out_bytes (room for total_bytes_out[iter - 1]),
 * out_off[n_pos + 1], n_voting[n_pos] and n_excluded[n_pos] (the reads of that pass that voted / did not); any may be NULL.
 * cf_consensus_info: the shape the tests straddle and the last run's figures.  phase_ms: copies to and from the device,
 * alignment (bands, moves, walks), vote and emission, scan and compaction, the whole call; by HIP events, summed over the
 * iterations of the last run.
 * Support (tests/supportcheck.py restates it).  cf_consensus_run_support is cf_consensus_run with one more argument:
 * with_support == 0 is cf_consensus_run itself (which calls it so), the same kernels storing the same bytes; with_support != 0
 * gives the same outputs bit for bit and keeps beside them what the vote otherwise discards (on request only: at the cenX shape
 * the extra stores and copies cost more than the spread between runs).  Every byte a pass emits carries one
 * number, `agree`:
 *   - an inserted base at (slot s, k): the largest of its four tallies, which is the tally of the base emitted;
 *   - a column base: 0 if all five tallies are 0 (the template byte kept with no vote; c_v == 0 is such a case), otherwise the
 *     tally of the base emitted, which after the tie rule of step 4 equals the top tally;
 *   - a column resolved as "deleted" emits nothing and has no entry;
 *   - the device keeps the number in 16 bits, saturating: a tally above 65 535 (a position with more voting reads than that)
 *     is reported as 65 535.  The bytes are decided on the full tallies.
 * So 0 <= agree <= n_voting[p] for every byte of position p, and an iteration has exactly total_bytes_out[iter - 1] entries, in
 * the order of its bytes (out_off of cf_consensus_get cuts both).  Per read q and iteration the context keeps voted[q] (1 / 0)
 * and dist[q]: the read's distance d to that iteration's template where it voted (exact), -1 where it did not — the band
 * stopped at the permille limit, or the lengths alone put the read beyond it, so d was never established.
 * cf_consensus_support: agree (int32, room for total_bytes_out[iter - 1] entries) of iteration iter (1 .. n_iters) of the last run.
 * cf_consensus_reads: dist[n_reads] and voted[n_reads] of that iteration.  Both refuse another iter with -22 like
 * cf_consensus_get — after a run without support every iter is another one —; either output pointer may be NULL; both read
 * host memory only. */
typedef struct cf_consensus_shape {
    int64_t max_len;                      /* bytes of the longest template or read taken                              */
    int64_t block_small, block_big, big_from; /* threads per workgroup; batches with a band of more than big_from diagonals take block_big */
    int64_t launch_cap;                   /* workgroups of a launch at most                                           */
    int64_t batch_bytes;                  /* move areas per batch in force (knob "cons_batch_bytes", 0 = 2^30)        */
    int64_t k_ins;                        /* bases a pass adds per slot at most                                       */
    int64_t n_pos, n_reads, n_iters, n_batches; /* of the last run (batches summed over its iterations)               */
    float phase_ms[5];
} cf_consensus_shape;
int cf_consensus_run(cf_ctx* ctx, const uint8_t* templates, const int64_t* t_off, const uint8_t* reads, const int64_t* r_off,
                     const int64_t* pos_ptr, int64_t n_pos, int32_t n_iters, int32_t permille, int64_t* total_bytes_out, float* ms_out);
int cf_consensus_get(cf_ctx* ctx, int32_t iter, uint8_t* out_bytes, int64_t* out_off, int32_t* n_voting, int32_t* n_excluded);
int cf_consensus_info(cf_ctx* ctx, cf_consensus_shape* out);
int cf_consensus_run_support(cf_ctx* ctx, const uint8_t* templates, const int64_t* t_off, const uint8_t* reads, const int64_t* r_off,
                             const int64_t* pos_ptr, int64_t n_pos, int32_t n_iters, int32_t permille, int32_t with_support,
                             int64_t* total_bytes_out, float* ms_out);
int cf_consensus_support(cf_ctx* ctx, int32_t iter, int32_t* agree);
int cf_consensus_reads(cf_ctx* ctx, int32_t iter, int32_t* dist, uint8_t* voted);

/* The built-in tandem aligner (cf_ualign.hip): every read against the unit read cyclically, the best stretch per read.  It stands
 * in for the external NCRF binary the reference starts per chunk of reads (scripts/run_ncrf_parallel.py:49-62) and has NO
 * reference function behind it: it is not NCRF, does not use NCRF's scoring and does not claim NCRF's output.  The rule below
 * is the specification (tests/ualigncheck.py restates it).
 * cf_ualign_run: the unit u of m = unit_len (1 .. max_unit) upper-case A, C, G, T; read q is reads[read_off[q], read_off[q + 1])
 * (n bytes, any bytes; offsets non-decreasing and >= 0); match M, mismatch X, gap G, all >= 1.
 *   w(x, y) = +M if (x with bit 5 cleared when it is a letter a .. z, i.e. toupper(x)) == y, else -X: N and every other byte
 *   that is not A, C, G, T after upper-casing is a mismatch.  The "+" problem aligns r to u, the "-" problem r to RC(u).
 *   Columns j = 0 .. m - 1 with p(j) = (j - 1) mod m, rows i = 0 .. n, S[0][j] = 0:
 *     A[i][j] = max(0, S[i-1][p(j)] + w(r[i-1], u[j]), S[i-1][j] - G)
 *     S[i][j] = max(A[i][j], max over 1 <= t < m of A[i][(j - t) mod m] - t G)
 *   (local alignment with linear gaps on a cylinder; a horizontal run around the whole unit costs m G and is dominated).
 *   The end cell is the cell of largest S over both strands; ties go to "+" before "-", then to the smallest i, then to the
 *   smallest j.  Value 0: the read has no hit.  The walk back from the end cell stops at a cell with S == 0; otherwise it takes
 *   (a) the diagonal if S[i-1][p(j)] + w(r[i-1], u[j]) == S[i][j]: column (r[i-1], u[j]); (b) else the vertical if
 *   S[i-1][j] - G == S[i][j]: column (r[i-1], '-'); (c) else the horizontal to (i, p(j)): column ('-', u[j]).
 * hits[n_reads]: status (CF_UALIGN_NONE / CF_UALIGN_HIT), strand (0 "+", 1 "-"), score (the end cell's value), r_st and r_en
 * (the stop row and the end row: the read's bytes [r_st, r_en)), u_st (index in u, or in RC(u) for "-", of the unit base of the
 * first alignment column; the first column is always a diagonal), m_al_len (unit bases on the row), n_ops (alignment columns)
 * and n_match, n_mismatch, n_ins (rule b: read bytes against '-') and n_del (rule c: unit bases against '-').  A read without
 * a hit has status 0 and every other field 0.  At most ONE record per read: a read whose array is interrupted gets its best
 * stretch only.  *ms (may be NULL): device milliseconds of the call, copies included.
 * The device runs two passes, one workgroup per pair, a thread holding cols_per_thread consecutive columns of the current row
 * in registers: the score pass over every (read, strand) keeps the best cell and stores nothing per cell; the moves pass fills
 * the winning strand of every read with a hit again, rows 1 .. r_en only, writes the move of every cell (2 bits) to the pair's
 * area of scratch and walks back.  Pairs of the moves pass go through in batches whose areas stay under the knob
 * "ualign_batch_bytes" (a pair that does not fit alone is taken alone).  Scores are int32: a read with n M >= 2^31 is refused.
 * Nothing is added to cf_times or cf_stats.  Errors (-22: null pointers, decreasing or negative offsets, unit_len outside
 * 1 .. max_unit, a unit byte that is not upper-case A, C, G, T, a score below 1, n M >= 2^31, n_reads < 0 or >= 2^30) leave the
 * context and the results of the call before as they were.  n_reads = 0 and empty reads are allowed.
 * cf_ualign_ops: the alignment columns of the last run as a CSR over its reads, in read order from r_st on: one byte per column,
 * CF_UALIGN_MATCH, _MISMATCH, _INS, _DEL.  *n_out = the number of bytes; ptr == ops == NULL asks for it alone; otherwise
 * cap >= *n_out, ptr[n_reads + 1].
 * cf_ualign_info: the shape the tests straddle and the last run's figures.  phase_ms: copies to and from the device, the score
 * pass, the moves pass with its walks, the whole call; by HIP events. */
enum { CF_UALIGN_NONE = 0, CF_UALIGN_HIT = 1 };
enum { CF_UALIGN_MATCH = 0, CF_UALIGN_MISMATCH = 1, CF_UALIGN_INS = 2, CF_UALIGN_DEL = 3 };
typedef struct cf_ualign_hit {
    int32_t status, strand, score, r_st, r_en, u_st, m_al_len, n_ops, n_match, n_mismatch, n_ins, n_del;
} cf_ualign_hit;
typedef struct cf_ualign_shape {
    int64_t max_unit;                     /* bases of the longest unit taken                                          */
    int64_t cols_per_thread, block;       /* columns of a row per thread; threads per workgroup at most (a launch takes the
                                             multiple of 64 that holds the unit)                                      */
    int64_t row_chunk;                    /* read bytes staged in LDS at a time                                       */
    int64_t launch_cap;                   /* workgroups of a launch at most                                           */
    int64_t batch_bytes;                  /* move areas per batch in force (knob "ualign_batch_bytes", 0 = an eighth of the device's memory, 2^28 .. 2^34)      */
    int64_t n_reads, n_score_pairs, n_move_pairs, n_batches; /* of the last run                                       */
    float phase_ms[4];
} cf_ualign_shape;
int cf_ualign_run(cf_ctx* ctx, const uint8_t* unit, int32_t unit_len, const uint8_t* reads, const int64_t* read_off, int64_t n_reads,
                  int32_t match, int32_t mismatch, int32_t gap, cf_ualign_hit* hits, float* ms);
int cf_ualign_ops(cf_ctx* ctx, int64_t* ptr, uint8_t* ops, int64_t cap, int64_t* n_out);
int cf_ualign_info(cf_ctx* ctx, cf_ualign_shape* out);

/* The built-in monomer decomposer (cf_monodec.hip): every read cut into a chain of monomer instances by one dynamic program against
 * all monomers at once.  It writes what the reference's second pipeline reads as a String Decomposer report (scripts/sd_parser.py)
 * and has NO reference function behind it: it is not String Decomposer and does not claim its output.  The rule below is the
 * specification (tests/monodeccheck.py restates it).
 * cf_monodec_run: monomers u_0 .. u_{K-1}, K = n_monomers >= 1, u_k = monomers[mono_off[k], mono_off[k + 1]) of l_k >= 1 upper-case
 * A, C, G, T, L = sum l_k <= max_cols; read q is reads[read_off[q], read_off[q + 1]) (n bytes, any bytes; offsets non-decreasing
 * and >= 0); match M, mismatch X, gap G, all >= 1.
 *   w(x, y) = +M if toupper(x) == y, else -X.  The "+" problem uses u_k, the "-" problem RC(u_k); the read is never reversed, so
 *   all coordinates are read coordinates on both strands.
 *   Cells V[i][k][j], i = 0 .. n, j = 0 .. l_k - 1; boundaries E[i] = the best score of r[0, i) fully explained.
 *     E[0] = 0, V[0][k][j] = -(j + 1) G; for i >= 1:
 *     D        = (j == 0 ? E[i-1] : V[i-1][k][j-1]) + w(r[i-1], u_k[j])
 *     A[i][k][j]  = max(D, V[i-1][k][j] - G)
 *     V'[i][k][j] = max over 0 <= t <= j of A[i][k][j-t] - t G
 *     E[i]     = max(max over k of V'[i][k][l_k-1], E[i-1] - G)
 *     V[i][k][j]  = max(V'[i][k][j], E[i] - (j + 1) G)
 *   (the last line lets a monomer start at row i with its first bases deleted; G >= 1, so the fed-back term cannot raise E[i]).
 *   The read's score is E[n]; the strand is the larger E[n], a tie goes to "+".
 *   The walk starts at boundary n.  At boundary i > 0: if some V[i][k][l_k-1] == E[i], enter the smallest such k at its last
 *   column (the instance ends at read base i - 1); otherwise read base i - 1 belongs to no monomer, go to boundary i - 1 (such
 *   bases only form a prefix of the read).  Inside an instance at (i, k, j), in this order: (a) i >= 1 and D == V: the diagonal
 *   (j == 0: the instance starts at read base i - 1, continue at boundary i - 1); (b) i >= 1 and V[i-1][k][j] - G == V: the
 *   vertical, to (i - 1, k, j); (c) the horizontal, a deletion of u_k[j], to (i, k, j - 1) (j == 0: continue at boundary i).
 *   Every instance covers its whole monomer (n_match + n_mismatch + n_del == l_k), takes at least one read base (st <= en, both
 *   inclusive), and the instances tile [prefix, n) without gaps.
 * info[n_reads]: status (CF_MONODEC_EMPTY: n = 0, every other field 0; CF_MONODEC_DONE), strand (0 "+", 1 "-"), score (E[n]),
 * n_inst, prefix (the unassigned bases in front).  *ms (may be NULL): device milliseconds of the call, copies included.
 * The device runs two passes, one workgroup per pair (read, strand), a thread holding cols_per_thread consecutive columns of the
 * L columns in registers: the score pass over every pair stores nothing per cell; the moves pass fills the winning strand again,
 * writes the move of every cell (2 bits) and one entry per row for the boundary to the pair's area of scratch and walks back.
 * Pairs of the moves pass go through in batches whose areas stay under the knob "monodec_batch_bytes" (a pair that does not fit
 * alone is taken alone).  Scores are int32: a read with (n + L + 1) max(M, X, G) >= 2^31 is refused.
 * Nothing is added to cf_times or cf_stats.  Errors (-22: null pointers, decreasing or negative offsets, K < 1, an empty monomer,
 * L > max_cols, a monomer byte that is not upper-case A, C, G, T, a score below 1, (n + L + 1) max(M, X, G) >= 2^31, n_reads < 0
 * or >= 2^30) leave the context and the results of the call before as they were.  n_reads = 0 and empty reads are allowed.
 * cf_monodec_get: the instances of the last run as a CSR over its reads, left to right: k, st, en (read bases, inclusive) and
 * n_match, n_mismatch, n_ins (rule b) and n_del (rule c).  *n_out = the number of instances; ptr == inst == NULL asks for it
 * alone; otherwise cap >= *n_out, ptr[n_reads + 1].
 * cf_monodec_info: the shape the tests straddle and the last run's figures.  phase_ms: copies to and from the device, the score
 * pass, the moves pass with its walks, the whole call; by HIP events. */
enum { CF_MONODEC_EMPTY = 0, CF_MONODEC_DONE = 1 };
typedef struct cf_monodec_read {
    int32_t status, strand, score, n_inst, prefix;
} cf_monodec_read;
typedef struct cf_monodec_inst {
    int32_t k, st, en, n_match, n_mismatch, n_ins, n_del;
} cf_monodec_inst;
typedef struct cf_monodec_shape {
    int64_t max_cols;                     /* bases of all monomers together at most                                    */
    int64_t cols_per_thread, block;       /* columns of a row per thread; threads per workgroup at most (a launch takes the
                                             multiple of 64 that holds the columns)                                   */
    int64_t row_chunk;                    /* read bytes staged in LDS at a time                                       */
    int64_t launch_cap;                   /* workgroups of a launch at most                                           */
    int64_t batch_bytes;                  /* move areas per batch in force (knob "monodec_batch_bytes", 0 = an eighth of the device's memory, 2^28 .. 2^34) */
    int64_t n_reads, n_monomers, n_cols, n_score_pairs, n_move_pairs, n_batches; /* of the last run                   */
    float phase_ms[4];
} cf_monodec_shape;
int cf_monodec_run(cf_ctx* ctx, const uint8_t* monomers, const int64_t* mono_off, int32_t n_monomers, const uint8_t* reads,
                   const int64_t* read_off, int64_t n_reads, int32_t match, int32_t mismatch, int32_t gap, cf_monodec_read* info, float* ms);
int cf_monodec_get(cf_ctx* ctx, int64_t* ptr, cf_monodec_inst* inst, int64_t cap, int64_t* n_out);
int cf_monodec_info(cf_ctx* ctx, cf_monodec_shape* out);

/* Exact counts of the gap-free windows of k letters over a set of monostrings (cf_monokmers.hip): what the reference's second
 * pipeline computes in a Python loop over string slices (scripts/debruijn_graph.py get_frequent_kmers and read_kmer_locations,
 * scripts/mono_error_correction.py correct_gaps).  The rule below is the specification (tests/monokmercheck.py
 * restates it).
 * cf_monokmers_run: strings s_0 .. s_{S-1}, S = n_strings >= 0, s_j = bytes[off[j], off[j + 1]) (any bytes; offsets >= 0 and
 * non-decreasing, so a string may be empty), N = off[S] - off[0] < 2^31 letters in all; k >= 1; min_mult >= 1; gap: the gap byte
 * (0 .. 255; the pipeline's is '?').
 *   Window (j, i) is VALID iff i + k <= len(s_j) and none of the bytes s_j[i .. i + k) is the gap byte.  No window reaches from
 *   one string into the next.  Two valid windows are the same k-mer iff their k bytes are equal (bytes are compared, nothing is
 *   hashed).  The result is every k-mer with at least min_mult valid windows, IN THE ORDER OF FIRST OCCURRENCE — the k-mer whose
 *   smallest (j, i) is smallest first, which is the order of the reference's dict and so of its graph's node numbers —, per k-mer
 *   its first (j, i), its count and pos = the first window's offset in the concatenation (bytes[off[0] + pos ..] are its letters).
 *   with_positions != 0: also every valid window of every reported k-mer, as a CSR over the k-mers in ascending (j, i).
 *   *n_kmers (may be NULL): the number of reported k-mers; *ms (may be NULL): device milliseconds of the call, copies included.
 * The device works by prefix doubling on equality ranks: R_1 = the byte, R_2m[p] = the dense id of (R_m[p], R_m[p + m]) over the
 * valid windows of length 2m, and with a the largest power of two not above k one overlapping combine (R_a[p], R_a[p + k - a]);
 * a round is a key pass, the stable record sort of cf_prims.hip with the position as payload, head flags, a scan and a scatter of
 * the ids.  Validity is a per-position distance to the next gap or string end, computed once.  The call keeps nothing on the device.
 * Nothing is added to cf_times or cf_stats.  Errors (-22: k < 1, min_mult < 1, N >= 2^31, offsets that do not ascend or are
 * negative, null pointers, a gap outside 0 .. 255, n_strings outside 0 .. 2^31 - 1) are raised before anything is allocated and
 * leave the context and the results of the call before as they were.
 * cf_monokmers_get: the last run's k-mers (cap >= their number) and, when it kept positions, ptr[n + 1] and the occurrences
 * (occ_cap >= their number).  Every pointer may be NULL; *n_out and *n_occ_out (-1: no positions kept) give the sizes.
 * cf_monokmers_info: the shape constants the tests straddle and the last run's figures: n_windows = the valid windows of length k,
 * n_distinct = the distinct k-mers among them (before min_mult), n_rounds = the combining rounds (0 for k = 1), n_sorts = the
 * record sorts (the rounds', the grouping of the bytes for k = 1, the sort of the classes by first position), n_sort_passes = their
 * 8-bit passes.  phase_ms: copies to and from the device, the sorts, everything else, the whole call; by HIP events. */
typedef struct cf_monokmer {
    int32_t s, i, count, pos;
} cf_monokmer;
typedef struct cf_monokmer_occ {
    int32_t s, i;
} cf_monokmer_occ;
typedef struct cf_monokmers_shape {
    int64_t sort_tile, scan_tile;         /* records per tile of the record sort; values per tile of the scan           */
    int64_t block, launch_cap;            /* threads per workgroup of the streaming passes; their workgroups at most    */
    int64_t n_strings, n_letters, k, min_mult, with_positions; /* of the last run                                       */
    int64_t n_windows, n_distinct, n_kmers, n_occ, n_rounds, n_sorts, n_sort_passes;
    float phase_ms[4];
} cf_monokmers_shape;
int cf_monokmers_run(cf_ctx* ctx, const uint8_t* bytes, const int64_t* off, int64_t n_strings, int64_t k, int64_t min_mult, int32_t gap,
                     int32_t with_positions, int64_t* n_kmers, float* ms);
int cf_monokmers_get(cf_ctx* ctx, cf_monokmer* kmers, int64_t cap, int64_t* n_out, int64_t* occ_ptr, cf_monokmer_occ* occ, int64_t occ_cap,
                     int64_t* n_occ_out);
int cf_monokmers_info(cf_ctx* ctx, cf_monokmers_shape* out);

/* Monoreads mapped to the edges of the de Bruijn graph (cf_monomap.hip): what the reference's DeBruijnGraph.map_reads computes with
 * a dict of every window of every edge and a slice at every read position (scripts/debruijn_graph.py index_edges, map_reads).  The
 * rule below is the specification (tests/monomapcheck.py restates it).
 * cf_monomap_run: edge strings e_0 .. e_{E-1} = edge_bytes[edge_off[e], edge_off[e + 1]), E = n_edges >= 0, with the nodes u[e] and
 * v[e] of every edge; read strings r_0 .. r_{R-1} = read_bytes[read_off[r], read_off[r + 1]), R = n_reads >= 0 (any bytes; offsets
 * >= 0 and non-decreasing, so a string may be empty); N = edge letters + read letters < 2^31; k >= 1; gap: the gap byte (0 .. 255;
 * the pipeline's is '?').
 *   A window of either set is VALID iff it lies inside one string and holds no gap byte.  (An edge window with a gap can never
 *   equal a read window, so leaving it out changes nothing against the reference.)
 *   An edge k-mer is INDEXED iff exactly one valid edge window, over all edges together, has its bytes (a k-mer occurring twice is
 *   dropped, not kept at its first place); its place is (e, j): edge e, letter j.
 *   A HIT of read r is a valid read window (r, i) whose k bytes equal an indexed k-mer; it carries (e, j, i), i counted in the
 *   whole read string, gaps included.  The hits of a read are in ascending i.
 *   The PATH of a read is the edges of its hits with equal neighbours collapsed: a miss between two hits on one edge does not
 *   split the run, A-B-A stays three elements, and no run reaches from one read into the next.
 *   The read is VALID iff v[p_t] == u[p_t+1] for every consecutive pair of its path (a path of 0 or 1 elements is valid).
 *   reads[r] (may be NULL): n_hits, the first hit (e0, j0, i0) and the last hit (e1, j1, i1) — all -1 without a hit —, valid, n_path.
 *   with_hits != 0: every hit is kept for cf_monomap_get.  *ms (may be NULL): device milliseconds of the call, copies included.
 * The device concatenates the edges, then the reads, and runs the doubling rounds of cf_monokmers.hip over both: a read window and
 * an edge window are the same k-mer iff they fall into one class.  The sort is stable and the edges lie in front, so a class is
 * indexed iff its first record is an edge position and its second, if any, a read position.  Then streaming passes: the edge
 * position to every read record of an indexed class, (e, j) by binary search in the offsets, hit flags, a scan and a compaction,
 * run heads, a scan and a compaction into the paths, flags of broken joins and a scan, one pass over the reads.  The call keeps
 * nothing on the device.  Nothing is added to cf_times or cf_stats.  Errors (-22: k < 1, null pointers where a count is positive,
 * offsets that do not ascend or are negative, N >= 2^31, a gap outside 0 .. 255, counts outside 0 .. 2^31 - 1) are raised before
 * anything is allocated and leave the context, the results of the call before and hbm_bytes_live as they were.  -12: no host
 * memory for the results (52 bytes per read, 4 per path element, 12 per kept hit); the results of the call before stay as well.
 * cf_monomap_get: the last run's paths as a CSR over the reads — path_ptr[R + 1] and the edge indices (path_cap >= their number) —
 * and, when it kept them, the hits: hit_ptr[R + 1] and the hits (hit_cap >= their number).  Every pointer may be NULL; *n_path and
 * *n_hits (-1: no hits kept) give the sizes.  Refused (-22) before any run.
 * cf_monomap_info: the shape constants the tests straddle and the last run's figures: n_edge_windows = the valid edge windows,
 * n_indexed = the indexed k-mers, n_rounds and n_sorts as for cf_monokmers_info.  phase_ms: copies to and from the device, the sorts,
 * everything else, the whole call; by HIP events. */
typedef struct cf_monomap_read {
    int32_t n_hits, e0, j0, i0, e1, j1, i1, valid, n_path;
} cf_monomap_read;
typedef struct cf_monomap_hit {
    int32_t e, j, i;
} cf_monomap_hit;
typedef struct cf_monomap_shape {
    int64_t sort_tile, scan_tile;         /* records per tile of the record sort; values per tile of the scan           */
    int64_t block, launch_cap;            /* threads per workgroup of the streaming passes; their workgroups at most    */
    int64_t n_edges, n_reads, k, with_hits; /* of the last run                                                          */
    int64_t n_edge_letters, n_read_letters, n_edge_windows, n_indexed, n_hits, n_path, n_rounds, n_sorts;
    float phase_ms[4];
} cf_monomap_shape;
int cf_monomap_run(cf_ctx* ctx, const uint8_t* edge_bytes, const int64_t* edge_off, const int32_t* u, const int32_t* v, int64_t n_edges,
                   const uint8_t* read_bytes, const int64_t* read_off, int64_t n_reads, int64_t k, int32_t gap, int32_t with_hits,
                   cf_monomap_read* reads, float* ms);
int cf_monomap_get(cf_ctx* ctx, int64_t* path_ptr, int32_t* path, int64_t path_cap, int64_t* n_path, int64_t* hit_ptr, cf_monomap_hit* hits,
                   int64_t hit_cap, int64_t* n_hits);
int cf_monomap_info(cf_ctx* ctx, cf_monomap_shape* out);

int cf_get_stats(cf_ctx* ctx, cf_stats* out);
int cf_get_times(cf_ctx* ctx, cf_times* out);

/* Read recruitment, the stage before the path (reference scripts/read_recruitment/rr.cpp:73-90:
 * edlibAlign(unit, read) and edlibAlign(revcomp(unit), read), mode HW, k = threshold; a read is kept when either result
 * is not -1).  Needs only a context.  unit: 1 .. 4096 upper-case ACGT; reads: any bytes back to back (matching is
 * literal, as in edlib), read_off[n_reads + 1].  dist_fwd / dist_rc [n_reads]: minimum edit distance between the unit /
 * its reverse complement and a substring of the read, -1 when above threshold (threshold < 0: no limit). */
int cf_rr_distances(cf_ctx* ctx, const uint8_t* unit, int32_t unit_len, const uint8_t* reads, const int64_t* read_off,
                    int64_t n_reads, int32_t threshold, int32_t* dist_fwd, int32_t* dist_rc);

/* Multi-GPU (new design — the reference has no distributed code, scripts/ is single-process): one
 * process per GPU, reads sharded across ranks, RCCL over xGMI inside the library on the context's stream.
 *   cf_comm_init         joins the communicator: rank 0 publishes the RCCL unique id at `rendezvous` (a path all ranks
 *                        share), the others read it.  world = 1 is allowed (every collective degenerates).
 *   cf_exchange_table    after cf_count_kmers on the local shard: (key, pres, multi) records are bucketed by
 *                        owner = hash(key) % world on the device and exchanged with one all-to-all (ncclSend/ncclRecv
 *                        pairs in rounds of <= 256 MB); the table then holds the exact global counts of the OWNED keys
 *                        (what distance_based_kmer_recruitment.py:39-63 computes over all reads), so cf_select_rare
 *                        selects the owned rare k-mers.  bytes_sent: bytes this rank sent to its peers.
 *   cf_allgather_kmers   all-gather of the owned rare lists; every rank installs the sorted union (= :66-82's set).
 *   cf_allgather_clouds  after cf_build_clouds on the local shard: all-gather of every rank's per-unit clouds
 *                        (read_kmer_cloud.py:34-40 over all reads, units in rank order); cf_dist_edges then works on
 *                        them, each rank on the first k-mers a % n_parts == part, with no reduction.
 *   cf_allreduce_unique  OR of the selected-k-mer masks of all ranks (filter_dist_tuples' set, :145-148).
 *   cf_comm_allreduce_i64  host values summed (op 0) or maximised (op 1) over ranks: counters, timing, barrier. */
int cf_comm_init(cf_ctx* ctx, int32_t rank, int32_t world, const char* rendezvous);
int cf_comm_free(cf_ctx* ctx);
int cf_comm_info(cf_ctx* ctx, int32_t* rank, int32_t* world);
int cf_comm_allreduce_i64(cf_ctx* ctx, int64_t* vals, int64_t n, int32_t op);
int cf_exchange_table(cf_ctx* ctx, int64_t* bytes_sent);
int cf_allgather_kmers(cf_ctx* ctx, int64_t* n_out);
int cf_allgather_clouds(cf_ctx* ctx, int64_t* n_entries);
int cf_allreduce_unique(cf_ctx* ctx, int64_t* n_unique);

/* Tuning knobs (defaults are chosen for gfx950), one paragraph per name, in the order of cf_param_name.  The default, the
 * accepted values and the refusal of each stand in centroflye_amd/csrc/hip/cf_knobs.h, the one table cf_set_param, cf_get_param
 * and cf_param_name are made of.  Results never depend on the knobs (tests/test_gpu_parity.py).
 *
 * "dist_block": threads per workgroup, 0 = auto.
 *
 * "dist_wgs": workgroups per CU the LDS is split between, 0 = auto: by the pair emissions per first k-mer.
 *
 * "dist_slots": LDS budget of the (b,d) table in 8-byte units, 0 = all that is left.
 *
 * "dist_wide": 1 forces the 8-byte-slot table layout (tests).
 *
 * "dist_post_atomics": 1: postings by a histogram and a fill pass of atomics instead of the sort.
 *
 * "dist_hot_cap": tests: a small cap on the filter's hot-slot list forces the evaluation inside the bucket scan.
 *
 * "lut_shift": the k-mer lookup table of cf_build_clouds gets (2 x k-mers rounded up to a power of two) << lut_shift slots; -1,
 * the default: 2 for sets of up to 1.7e7 k-mers, 1 up to 1.3e8, else 0.
 *
 * "dist_hot_entries": default 32768: first k-mers with more partner entries than this keep no list of hot slots during their
 * inserts — it would overflow — and their filter scans the count fields; -1: always keep it.
 *
 * "dist_regions": 1, 2, 4, 8: force the region layout of the 6-byte slots, which k-mer sets of 2^24 .. 2^27 ranks with long
 * reads take by themselves.
 *
 * "dist_region_bytes": 1: the region layout streams rank and unit index apart, as k-mer sets beyond 2^26 ranks or reads beyond
 * 128 units do by themselves.
 *
 * "dist_dbits": 5 .. 8: cap on the distance-field bits of the 6-byte table slots [d | b]; 0 = 32 minus the bits the k-mer ranks
 * need.
 *
 * "dist_fill_pct": a (b,d) table pass is split when more than this share of the slots is in use.
 *
 * "dist_edge_chunk": edge rows a workgroup reserves in the output per global atomic, 0 = 8192; tests use small chunks.
 *
 * "dist_int_thr": 0: the dominance test always divides in doubles; 1, the default: the literal 0.8 is tested as 5 cnt >= 4
 * total, which is the same predicate.
 *
 * "dist_sketch": 0: every pair goes to the exact table.
 *
 * "dist_sketch_tail": 1, the default: the sketch sweep leaves out the items beyond the largest distance at which min_cov
 * postings of the first k-mer still have a partner unit; 0: it takes every item, in the order of the posting list.
 *
 * "dist_class_bits": 1 .. 16, default 16: bits of the posting list's hash in the sort key that brings equal lists together;
 * fewer bits only lose merges; a TEST knob: few bits make different lists collide, so that the comparison of the lists is what
 * keeps them apart; the library never uses more bits than the 64-bit sort key leaves next to the unit and rank fields.
 *
 * "dist_classes": 1, the default: first k-mers of a launch whose posting lists are equal share one sweep of the distance kernel,
 * which writes the rows of each of them; 0: every first k-mer is swept on its own; the results are the same.
 *
 * "dist_groups": 1, the default: the first k-mers of a launch that share their first posting unit are cut into groups whose
 * posting lists have a union of at most dist_group_cap postings; the distance kernel sweeps the union once into a table of
 * 32-bit masks and every member reads its own counts out of it; 0: classes only, the launch it was before; needs dist_classes 1
 * and the 6-byte-slot layout, the other layouts keep the classes; the results are the same.
 *
 * "dist_filter_once": 1, the default: in a launch with groups the distance kernel filters all members of a group in one section
 * — a thread keeps its hot slot and the masks of its b in registers, loops over the members and the rows are reserved once per
 * group; 0: one filter per member, the code it was before; the results are the same, the order of the rows in the output
 * differs.
 *
 * "dist_group_cap": 1 .. 32, default 32: the postings of a group's union, the bits of a mask; a test and tuning knob.
 *
 * "dist_sketch_bits": bits of a counter of the distance stage's counting sketch: 0, the default: 4 when min_cov <= 9 — twice the
 * counters in the same LDS —, else 8; 8 forces bytes.
 *
 * "dist_est_pct": expected distinct (b,d) keys per 100 pair emissions: sizes the initial number of table partitions.
 *
 * "dist_stage": edges of a pass whose rows do not fit the rest of the workgroup's output chunk, staged in LDS.
 *
 * "place_chunk": place_mode 1: cloud entries per wave step.
 *
 * "place_grid" / "place_block": workgroups and threads per workgroup of the iteration kernel, 0 = 128 x 1024.
 *
 * "place_fused": place_mode 1: 1: score updates applied by the waves that lay a read onto the contig, 0: through an event list
 * and a third kernel per greedy iteration.
 *
 * "place_mode": 2, the default: per-read score regions and one kernel per greedy iteration, cf_place2.hip — for min_inters >= 4;
 * smaller thresholds make nearly every score row a candidate row and take path 1; 3: the regions whatever the threshold; 1: the
 * hash-map path of rounds 1-3, cf_place.hip.
 *
 * "place_row_words": 32 or 64 words per posting row, 0 = by the longest posting list.
 *
 * "place_long_rescans": default 2: a run of the region path whose reads average more than this many rescans of reads with more
 * than four candidate score rows per greedy iteration — k-mers that are not unique to one place of the array, thin coverage — is
 * handed to the hash-map path; -1: at the first look, tests.
 *
 * "place_cmap_bits": log2 of the first capacity of the contig's overflow map — the positions of a k-mer beyond its fourth —, 0 =
 * cloud entries / 8, at least 2^21; grown automatically, times four, when it passes half load.
 *
 * "place_slots_per_unit": score-region slots per unit of a read, 0 = 48; grown automatically when a region fills.
 *
 * "place_l3" / "place_l3_shift": 1: the third level of the placement arg-max, groups of 2^shift blocks of 64 reads kept lazily —
 * built in round 5, measured neutral at 500 000 reads, off by default.
 *
 * "map_window": candidate starts — LDS score slots — that cf_map_reads covers per pass over a read's cloud entries, 0 = 2048, at
 * most 4096; a read whose hits span more starts takes several passes, tests force that with tiny windows.
 *
 * "edit_lds_diags": cf_edit_distances: diagonals per wavefront array up to which a pair's wavefronts stay in LDS, 0 = 16384, at
 * most 16384; tests force the HBM path with small values.
 *
 * "tandem_key_mode" and "tandem_batch_windows": cf_tandem_scan: see there.
 *
 * "cons_batch_bytes": cf_consensus_run: bytes of move areas per batch of pairs, 0 = 2^30, at most 2^36; a batch holds at least
 * one pair; tests force many batches with small values.
 *
 * "ualign_batch_bytes": cf_ualign_run: bytes of move areas per batch of pairs of its moves pass, 0 = an eighth of the device's
 * memory between 2^28 and 2^34, at most 2^36; a batch holds at least one pair.
 *
 * "monodec_batch_bytes": cf_monodec_run: the same for its moves pass.
 *
 * "count_mode": 1: A1 by sort and reduce, 0: the atomic table.
 *
 * "count_bits": bucket bits of the former, 0 = auto.
 *
 * "count_slots" / "count_tile": count_mode 0: 8-byte slots of the LDS set a hash class of a read's windows has to fit, and reads
 * per tile of its launch.
 *
 * "count_skip_exotic": 1: cf_count_occurrences runs on reads with symbols other than upper-case A, C, G, T and skips the windows
 * that hold one — the caller counts those on the host, cfh_exotic_occurrences; 0, the default: it refuses such reads.
 *
 * "comm_round_bytes": bytes per pair of ranks and round of the multi-GPU exchanges, default 2^28; tests force many rounds.
 *
 * "comm_self_p2p": 1: the message a rank sends to itself goes through ncclSend / ncclRecv like every other one, so that a
 * one-GPU box runs the whole p2p path.
 *
 * cf_set_param stores an accepted value (-22 and a message for a refused one or an unknown name; the knob keeps its value).
 * cf_get_param: *value = what is stored (1 for any non-zero value of an on / off knob); an unknown name is refused in the same
 * way, a NULL pointer with -22.  cf_param_name: the name of knob number index, NULL from the number of knobs on; it needs no
 * context. */
int cf_set_param(cf_ctx* ctx, const char* name, int64_t value);
int cf_get_param(cf_ctx* ctx, const char* name, int64_t* value);
const char* cf_param_name(int32_t index);
/* A/B switches: names that cf_set_param and cf_get_param know and cf_param_name does not list — a kernel against the one it
 * replaced, for tests and measurements; not part of what callers tune by, and the results are the same either way.
 *
 * "dist_walk": 1, the default: the kernel that cuts the runs of first k-mers into groups keeps the open group's union in an LDS
 * table from unit to bit, which the lanes of a member's list probe together; 0: the union in the lanes with a broadcast and a
 * compare per posting, the kernel it was before. */

/* Self-tests of the device primitives against host results (used by tests/ only). */
int cf_selftest_sort(cf_ctx* ctx, const uint64_t* keys, int64_t n, int32_t bits, uint64_t* out);
int cf_selftest_scan(cf_ctx* ctx, const int64_t* in, int64_t n, int64_t* out);
/* The other primitives of cf_prims.hip, one call each (tests/primcheck.py).
 * cf_selftest_scan_inplace: cf_selftest_scan with one device buffer as input and output, as two stages call the scan.
 * cf_selftest_scan_u32: the scan of 32-bit counts into 64-bit offsets; out[n] = the total, as for cf_selftest_scan.
 * cf_selftest_sort_rec16: the stable sort of n records of four 32-bit words by n_fields <= 16 fields (words[f] = 0 .. 3,
 * bits[f] = 0 .. 32), least significant field first.  A field is sorted on the whole bytes of its word that hold its
 * bits[f] low bits: the bits of the word above them take no part, the bits between bits[f] and the next byte border do.
 * cf_selftest_digit_offsets: offs[t * D + d] = the exclusive scan, in (digit, tile) order, of the tile-major counts
 * hist[t * D + d] (1 <= D <= 512, else -22); *total = the sum, total may be NULL.  n_tiles = 0 returns 0 and writes
 * neither offs nor *total. */
int cf_selftest_scan_inplace(cf_ctx* ctx, const int64_t* in, int64_t n, int64_t* out);
int cf_selftest_scan_u32(cf_ctx* ctx, const uint32_t* in, int64_t n, int64_t* out);
int cf_selftest_sort_rec16(cf_ctx* ctx, const uint32_t* recs, int64_t n, const int32_t* words, const int32_t* bits, int32_t n_fields,
                           uint32_t* out);
int cf_selftest_digit_offsets(cf_ctx* ctx, const uint32_t* hist, int32_t n_tiles, int32_t D, int64_t* offs, int64_t* total);
/* the arg-max of the greedy placement (read_placer.py:63-78: larger (s0, s1), then the larger offset, then the smaller id rank)
 * over n candidates given as rows (s0, s1, offset, rank, valid); out6 = (s0, s1, offset, rank, index of the winner, valid) */
int cf_selftest_argmax(cf_ctx* ctx, const uint32_t* cands, int64_t n, uint32_t* out6);
/* The two device steps of cf_exchange_table on their own, with no communicator.
 * cf_selftest_owner_buckets: the context's table bucketed for a virtual world of 1 .. 4096 ranks, as the send buffer of the
 * exchange: start[world + 1] (start[0] = 0, start[world] = *n_out = the table's keys), the records of owner o at
 * start[o] .. start[o + 1] - 1 as keys[i] and vals[i] = pres | multi << 32.  keys == NULL asks for start and *n_out alone;
 * otherwise cap >= *n_out.  The table stays as it is.
 * cf_selftest_merge_records: what an owner does with the n records (keys[i], vals[i]) it received: a fresh table of
 * max(1024, 2 n rounded up to a power of two) slots, every record added into it (a key may come any number of times; pres and
 * multi add up separately); it is the context's table afterwards (cf_get_table).  n = 0 leaves an empty table.
 * -22: world out of range, no table, null pointers, cap too small. */
int cf_selftest_owner_buckets(cf_ctx* ctx, int32_t world, int64_t* start /* world + 1 */, uint64_t* keys, uint64_t* vals, int64_t cap,
                              int64_t* n_out);
int cf_selftest_merge_records(cf_ctx* ctx, const uint64_t* keys, const uint64_t* vals, int64_t n);

#ifdef __cplusplus
}
#endif
#endif
