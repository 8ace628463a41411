// The tuning knobs of cf_set_param / cf_get_param, one entry each (no include guard: the file is included wherever the table is
// expanded, with CF_KNOB defined for that use):
//   CF_KNOB(name, member type, default, accepted, stored, refusal)
// `accepted` and `stored` are expressions in the caller's int64_t v (cf_in(v, lo, hi): lo <= v <= hi).  cf_common.h expands the
// table into the members of cf_ctx with their defaults; cf_api.hip into the entries cf_set_param, cf_get_param and cf_param_name
// look a name up in, in this order.  CF_KNOB_AB(...) has the same fields: an A/B switch that cf_set_param and cf_get_param know by name
// and cf_param_name does not list (the listed knobs are the interface callers tune by; a switch between a kernel and the one it replaced is not).  A knob that takes every value (stored as v != 0) has no refusal.  What a knob means to a
// caller stands in include/cfhip.h, in front of cf_set_param (tests/test_emu_params.py holds the two lists of names together).

// threads per workgroup; 0 = chosen with dist_wgs
CF_KNOB(dist_block, int, 0, v == 0 || (cf_in(v, 64, 1024) && v % 64 == 0), (int)v, "dist_block must be 0 (auto) or a multiple of 64 in [64, 1024]")
// workgroups per CU the LDS is split between; 0 = 2 x 512 threads or 1 x 1024, by the pair emissions per first k-mer
CF_KNOB(dist_wgs, int, 0, cf_in(v, 0, 8), (int)v, "dist_wgs out of range (0 = auto, 1 .. 8)")
// LDS budget of the (b,d) table in 8-byte units; 0 = all that is left next to the work lists
CF_KNOB(dist_slots, int, 0, v == 0 || cf_in(v, 256, 19200), (int)v, "dist_slots out of range (0 = auto, 256 .. 19200: table + work lists must fit the 160 KiB LDS)")
// 1 forces the 8-byte-slot table layout (tests)
CF_KNOB(dist_wide, int, 0, true, v != 0, "")
// 1 builds the postings with the histogram + fill passes of atomics instead of the sort (tests, A/B runs)
CF_KNOB(dist_post_atomics, int, 0, true, v != 0, "")
// > 0: cap on the filter's hot-slot list (tests)
CF_KNOB(dist_hot_cap, int, 0, v >= 0, (int)v, "dist_hot_cap must be >= 0")
// the k-mer lookup table of A3 has (2 x k-mers, rounded up to a power of two) << lut_shift slots; -1 = by the set's size
CF_KNOB(lut_shift, int, -1, cf_in(v, -1, 3), (int)v, "lut_shift out of range (-1 = by the set's size, 0 .. 3)")
// first k-mers with more partner entries keep no hot-slot list (it would overflow: ~5 % of the pairs' keys reach min_cov); -1: always keep it
CF_KNOB(dist_hot_entries, int, 32768, cf_in(v, -1, 0x7FFFFFFF), (int)v, "dist_hot_entries out of range (-1 = always keep the list, 0 .. 2^31 - 1)")
// 1, 2, 4, 8: force the region layout of the 6-byte slots with at least that many regions (tests), 0 = only when the ranks need it
CF_KNOB(dist_regions, int, 0, v == 0 || v == 1 || v == 2 || v == 4 || v == 8, (int)v, "dist_regions must be 0 (auto), 1, 2, 4 or 8")
// 1: the region layout streams rank and unit index apart (round 3) even where the 4-byte stream of cf_tab_region26 applies (tests)
CF_KNOB(dist_region_bytes, int, 0, true, v != 0, "")
// 5 .. 8: upper limit of the distance-field bits of the 6-byte-slot layout (tests), 0 = as many as the k-mer ranks leave
CF_KNOB(dist_dbits, int, 0, v == 0 || cf_in(v, 5, 8), (int)v, "dist_dbits must be 0 (auto) or 5 .. 8")
// a (b,d) table pass is split when more than this share of the slots is in use
CF_KNOB(dist_fill_pct, int, 70, cf_in(v, 10, 90), (int)v, "dist_fill_pct out of range (10 .. 90)")
// > 0: edge rows a workgroup reserves per global atomic (tests: small chunks cross often), 0 = 8192
CF_KNOB(dist_edge_chunk, int, 0, cf_in(v, 0, 1 << 20), (int)v, "dist_edge_chunk out of range (0 = default, 1 .. 2^20)")
// 1: rel_threshold == 0.8 is tested as 5 cnt >= 4 total; 0: always the double division (tests)
CF_KNOB(dist_int_thr, int, 1, true, v != 0, "")
// 0: every (b,d) pair goes to the exact table (no counting sketch first)
CF_KNOB(dist_sketch, int, 1, true, v != 0, "")
// the sketch sweep skips the items beyond the largest distance at which min_cov postings still have a partner unit (0: every item, in the old order)
CF_KNOB(dist_sketch_tail, bool, true, true, v != 0, "")
// bits of the posting list's hash in the order key (1 .. 16; tests: few bits make different lists collide, which the comparison of the lists must undo)
CF_KNOB(dist_class_bits, int, 16, cf_in(v, 1, 16), (int)v, "dist_class_bits out of range (1 .. 16)")
// first k-mers with equal posting lists share one sweep of cf_dist_kernel (0: every k-mer on its own, as before)
CF_KNOB(dist_classes, bool, true, true, v != 0, "")
// first k-mers with the same first posting unit share one sweep over the UNION of their lists, a 32-bit mask per (b, d); 0: classes only
CF_KNOB(dist_groups, bool, true, true, v != 0, "")
// the mask table's filter evaluates every (hot slot, member) pair of a group in one section, rows reserved per group; 0: the loop over the members, one filter each
CF_KNOB(dist_filter_once, bool, true, true, v != 0, "")
// the cut of the runs into groups keeps the open group's union in an LDS table unit -> bit that a member's lanes probe together; 0: the union in the lanes, a broadcast and a compare per posting
CF_KNOB_AB(dist_walk, bool, true, true, v != 0, "")
// postings of a group's union (1 .. 32: the mask's bits; tests: small caps close groups early)
CF_KNOB(dist_group_cap, int, 32, cf_in(v, 1, 32), (int)v, "dist_group_cap out of range (1 .. 32)")
// bits of a sketch counter: 0 = 4 when min_cov <= 9, else 8; 8 forces bytes
CF_KNOB(dist_sketch_bits, int, 0, v == 0 || v == 4 || v == 8, (int)v, "dist_sketch_bits must be 0 (by min_cov), 4 or 8")
// expected distinct (b,d) keys per 100 pair emissions: sizes the initial number of table partitions
CF_KNOB(dist_est_pct, int, 80, cf_in(v, 5, 100), (int)v, "dist_est_pct out of range (5 .. 100)")
// edges of a pass whose rows do not fit the rest of the workgroup's output chunk, staged in LDS (more: a sweep of the marked slots)
CF_KNOB(dist_stage, int, 2048, cf_in(v, 0, 2048), (int)v, "dist_stage out of range (0 .. 2048)")
// cf_place: cloud entries per wave step of the fused kernel (1 .. 64)
CF_KNOB(place_chunk, int, 2, cf_in(v, 1, 64), (int)v, "place_chunk out of range (1 .. 64)")
// workgroups of the iteration kernel (0 = one per CU in cf_place, 128 in cf_place2)
CF_KNOB(place_grid, int, 0, cf_in(v, 0, 4096), (int)v, "place_grid out of range (0 = auto, 1 .. 4096)")
// 1: the greedy iteration is arg-max + (pick, add, score updates) = 2 kernels; 0: 3 kernels with an event list
CF_KNOB(place_fused, int, 1, true, v != 0, "")
// 2: per-read score regions, one kernel per greedy iteration (cf_place2.hip); 1: the hash-map path of rounds 1-3 (cf_place.hip)
CF_KNOB(place_mode, int, 2, cf_in(v, 1, 3), (int)v, "place_mode out of range (1 = hash map, 2 = per-read regions unless min_inters < 4, 3 = per-read regions always)")
// cf_place2: threads per workgroup of the iteration kernel (128 .. 1024, a multiple of 128; 0 = 1024)
CF_KNOB(place_block, int, 0, v == 0 || (cf_in(v, 128, 1024) && v % 128 == 0), (int)v, "place_block must be 0 or a multiple of 128 in 128 .. 1024")
// cf_place2: 32-bit words of a posting row (32 or 64); 0 = the smaller one that holds the longest posting list
CF_KNOB(place_row_words, int, 0, v == 0 || v == 32 || v == 64, (int)v, "place_row_words must be 0 (auto), 32 or 64")
// cf_place2: long rescans (reads with more than four candidate rows) per greedy iteration above which the run goes to the hash-map path (-1: at the first look, tests)
CF_KNOB(place_long_rescans, int, 2, cf_in(v, -1, 1000000), (int)v, "place_long_rescans out of range (-1, 0 .. 1000000)")
// cf_place2: log2 of the first capacity of the contig's overflow map (0 = entries / 8, at least 2^21; tests force tiny maps that have to grow)
CF_KNOB(place_cmap_bits, int, 0, cf_in(v, 0, 30), (int)v, "place_cmap_bits out of range (0 = default, 1 .. 30)")
// cf_place2: score-region slots per unit of a read (0 = 48); doubled-up automatically when a region fills
CF_KNOB(place_slots_per_unit, int, 0, cf_in(v, 0, 65536), (int)v, "place_slots_per_unit out of range (0 = default, 1 .. 65536)")
// cf_place2: third level of the arg-max (best candidate per group of 64-read blocks): 1 = on; 0 / 2 = off (measured: no gain at 500 000 reads)
CF_KNOB(place_l3, int, 0, cf_in(v, 0, 2), (int)v, "place_l3 must be 0 (auto), 1 (always) or 2 (never)")
// cf_place2: log2 of the blocks per group (0 = 6: groups of 64 blocks = 4 096 reads; tests use small groups at small read sets)
CF_KNOB(place_l3_shift, int, 0, cf_in(v, 0, 6), (int)v, "place_l3_shift must be 0 (= 6) .. 6")
// cf_map: candidate starts (LDS score slots) a wave covers per pass over a read's entries (0 = 2048; tests force small windows)
CF_KNOB(map_window, int, 0, cf_in(v, 0, 4096), (int)v, "map_window out of range (0 = default, 1 .. 4096: 12 bytes of LDS per slot)")
// cf_edit: diagonals per wavefront array above which a pair's wavefronts live in HBM, not LDS (0 = 16384; tests force small values)
CF_KNOB(edit_lds_diags, int, 0, cf_in(v, 0, 16384), (int)v, "edit_lds_diags out of range (0 = default, 1 .. 16384: 8 bytes of LDS per diagonal)")
// cf_tandem: 0 = 64-bit keys where (read in batch, code, position) fit them, 1 = keys or an error, 2 = 16-byte records
CF_KNOB(tandem_key_mode, int, 0, cf_in(v, 0, 2), (int)v, "tandem_key_mode out of range (0 = auto, 1 = 64-bit keys, 2 = 16-byte records)")
// cf_tandem: windows per batch of whole reads (0 = 2^26; tests force borders inside small inputs)
CF_KNOB(tandem_batch_windows, int64_t, 0, cf_in(v, 0, (int64_t)1 << 31), v, "tandem_batch_windows out of range (0 = default, 1 .. 2^31)")
// cf_consensus: bytes of move areas per batch of pairs (0 = 2^30; tests force borders inside one position's reads)
CF_KNOB(cons_batch_bytes, int64_t, 0, cf_in(v, 0, (int64_t)1 << 36), v, "cons_batch_bytes out of range (0 = default, 1 .. 2^36)")
// cf_ualign: bytes of move areas per batch of pairs of the moves pass (0 = an eighth of the device's memory, 2^28 .. 2^34; tests force one pair per batch)
CF_KNOB(ualign_batch_bytes, int64_t, 0, cf_in(v, 0, (int64_t)1 << 36), v, "ualign_batch_bytes out of range (0 = default, 1 .. 2^36)")
// cf_monodec: bytes of move areas per batch of pairs of the moves pass (0 = an eighth of the device's memory, 2^28 .. 2^34; tests force one pair per batch)
CF_KNOB(monodec_batch_bytes, int64_t, 0, cf_in(v, 0, (int64_t)1 << 36), v, "monodec_batch_bytes out of range (0 = default, 1 .. 2^36)")
// 1: sort and reduce (cf_count2.hip) when it applies; 0: the atomic table of round 1 (cf_count.hip)
CF_KNOB(count_mode, int, 1, true, v != 0, "")
// bucket bits of the sort-and-reduce path; 0 = from the number of windows (tests force small / large values)
CF_KNOB(count_bits, int, 0, cf_in(v, 0, 27), (int)v, "count_bits out of range (0 = auto, 1 .. 27)")
// cf_count (count_mode 0): 8-byte slots of the LDS set a hash class of a read's windows has to fit
CF_KNOB(count_slots, int, 4096, v >= 256 && !(v & (v - 1)) && v * 8 <= 128 * 1024, (int)v, "count_slots must be a power of two in [256, 16384]")
// cf_count (count_mode 0): reads per tile of its launch
CF_KNOB(count_tile, int, 16, cf_in(v, 1, 64), (int)v, "count_tile out of range")
// 1: cf_count_occurrences counts reads with other symbols too, skipping their windows (stage 4 adds them on the host)
CF_KNOB(count_skip_exotic, int, 0, cf_in(v, 0, 1), (int)v, "count_skip_exotic must be 0 or 1")
// bytes per pair and round of the multi-GPU exchanges (tests force small rounds)
CF_KNOB(comm_round_bytes, int64_t, (int64_t)256 << 20, cf_in(v, 16, (int64_t)1 << 30) && v % 16 == 0, v, "comm_round_bytes must be a multiple of 16 in [16, 2^30]")
// 1: a rank's message to itself goes through ncclSend / ncclRecv too (tests: the p2p path on one GPU)
CF_KNOB(comm_self_p2p, int, 0, true, v != 0, "")
