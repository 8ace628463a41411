// cf_common.h — shared declarations of the gfx950 device pipeline (libcfhip.so).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "cfhip.h"

// Every kernel uses one dynamic-LDS window and carves it up itself.
extern __shared__ __attribute__((aligned(16))) unsigned char cf_lds[];

#define CF_WAVE 64

// The dynamic LDS window begins at address 0 of the workgroup's LDS (no kernel of this library has static LDS).  A pointer
// made from that NUMBER lets the compiler fold an array's offset into the offset field of the ds_ instruction; through the
// symbol cf_lds it puts a `v_add_u32 v, 0, v` in front of every access (the symbol's address is assigned after instruction
// selection): four of the 48 vector instructions of cf_dist_kernel's sketch step.  cf_lds_base_ok() is the kernel's check
// of the premise.  (The host emulator of tests/emu defines both itself.)
#ifndef cf_lds_at
typedef __attribute__((address_space(3))) unsigned char cf_lds_u8;
__device__ __forceinline__ unsigned char* cf_lds_at(uint32_t off) { return (unsigned char*)((cf_lds_u8*)(uintptr_t)(off + 16u) - 16); }
__device__ __forceinline__ bool cf_lds_base_ok() { return (uint32_t)(uintptr_t)(cf_lds_u8*)cf_lds == 0u; }
#endif

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ uint64_t cf_mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
__device__ __forceinline__ uint32_t cf_mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// ASCII base -> 2-bit code with A<C<G<T (A 0x41, C 0x43, G 0x47, T 0x54); bit 5 (the case) plays no part
__device__ __forceinline__ uint32_t cf_base2(uint32_t c) { return ((c >> 1) ^ (c >> 2)) & 3u; }
// upper-case A, C, G or T?  (x = c - 'A': bits 0, 2, 6, 19 of the mask)  A window holding anything else has no 2-bit code:
// the device paths skip it (what the reference does with such windows: centroflye_amd/_host.py exotic_summary)
__device__ __forceinline__ bool cf_is_acgt(uint32_t c) { const uint32_t x = c - 0x41u; return x < 20u && ((0x80045u >> x) & 1u); }
__device__ __forceinline__ bool cf_is_acgt_nocase(uint32_t c) { return cf_is_acgt(c & 0xDFu); }
// the string that holds the absolute position p of a concatenation with the offsets off[0 .. n_strings]: the s with
// off[s] <= p < off[s + 1] (empty strings hold nothing)
__device__ __forceinline__ int64_t cf_string_of(const int64_t* __restrict__ off, int64_t n_strings, int64_t p) {
    int64_t lo = 0, hi = n_strings;      // off[lo] <= p < off[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// bit 63 marks an occupied slot in every k-mer keyed table (k <= 31 -> key < 2^62)
#define CF_OCC (1ull << 63)

// 16-byte slot of the HBM k-mer table: key | CF_OCC, then pres (low 32) | multi (high 32)
struct alignas(16) cf_slot {
    unsigned long long key;
    unsigned long long val;
};

// ---------------------------------------------------------------- host side
struct cf_devbuf {
    void* p = nullptr;
    size_t bytes = 0;
};

struct cf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    std::string err;
    int n_cu = 0;
    int64_t hbm_total = 0;
    size_t live = 0;
    // freed device blocks are kept and reused (hipMalloc / hipFree of the per-call work buffers — hundreds of MB each —
    // cost up to tens of ms per step and vary from box to box): size -> block, and the true size of every block handed out
    std::multimap<size_t, void*> pool;
    std::unordered_map<void*, size_t> block_bytes;
    size_t pooled = 0;
    size_t pool_max = (size_t)128 << 30;      // bytes kept for reuse (cf_create: 85 % of the device's memory)

    // reads / units
    uint8_t* d_bases = nullptr;
    int64_t* d_read_off = nullptr;
    int64_t* d_unit_ptr = nullptr;
    int64_t* d_unit_start = nullptr;
    int64_t* d_unit_end = nullptr;
    std::vector<int64_t> h_read_off, h_unit_ptr;
    int64_t max_unit_len = 0;     // bases of the longest unit (bounds the entries of a cloud)
    int64_t n_reads = 0, n_bases = 0, n_units = 0;
    bool has_exotic = false;     // some base is not upper-case A, C, G, T

    // A1 table
    cf_slot* d_table = nullptr;
    uint64_t table_cap = 0;      // slots in use (a power of two)
    uint64_t table_alloc = 0;    // slots allocated (>= table_cap: a smaller table reuses a larger allocation)
    bool table_dense = false;    // the table is a dense array of table_cap occupied slots (cf_count2.hip): scan it, do not probe it
    int k = 0;

    // k-mer set + lookup table
    unsigned long long* d_kmers = nullptr;
    int64_t n_kmers = 0;
    int set_k = 0;
    cf_slot* d_lut = nullptr;        // lookup table k-mer -> rank: lut_cap slots {k-mer | CF_OCC, rank}
    uint64_t lut_cap = 0;
    uint32_t* d_lut_pre = nullptr;   // 8 bits per lookup slot: Bloom words tested before the lookup table (most windows are not in the set)
    uint64_t lut_pre_words = 0;

    // clouds
    int64_t* d_cloud_ptr = nullptr;  // U+1
    int32_t* d_entries = nullptr;
    int64_t n_entries = 0;
    bool have_clouds = false;
    // what cf_place2_fits needs of the INSTALLED clouds: the entries of the largest cloud and of the read with most of them.
    // -1 = not measured: clouds of cf_build_clouds, which hold at most one entry per window of their unit, so max_unit_len bounds
    // a cloud and units x max_unit_len a read.  cf_set_clouds takes any CSR and measures it; cf_filter_clouds only removes entries,
    // so either bound stays valid across it; cf_allgather_clouds fills the distance stage's view (g_*) and leaves these clouds alone.
    int64_t cloud_max_entries = -1, read_max_entries = -1;

    // multi-GPU (cf_exchange.hip): the transport, and the all-gathered clouds of every rank's reads — what the distance
    // stage works on when present (units in rank-major order; reads and bases stay those of the local shard)
    struct cf_comm* comm = nullptr;
    bool have_gview = false;
    int64_t g_reads = 0, g_units = 0, g_entries = 0;
    int64_t* g_unit_ptr = nullptr;    // g_reads + 1
    int64_t* g_cloud_ptr = nullptr;   // g_units + 1
    int32_t* g_entries_d = nullptr;   // g_entries
    std::vector<int64_t> g_h_unit_ptr;
    int64_t exchange_bytes = 0;       // bytes this rank sent in the last cf_exchange_table

    // edges / unique bitmap
    uint32_t* d_edges = nullptr;  // n x 4
    int64_t edge_cap = 0, n_edges_stored = 0;
    uint32_t* d_unique_bits = nullptr;
    int64_t unique_words = 0;

    // frozen contig of cf_contig_build (cf_map.hip): a CSR by k-mer rank of the positions of every frequent k-mer, and the
    // coverage of the positions 0 .. max_pos; dropped with the clouds it was built from
    bool have_contig = false;
    int64_t* d_contig_ptr = nullptr;   // contig_K + 1
    int32_t* d_contig_pos = nullptr;   // contig_pairs
    int32_t* d_contig_cov = nullptr;   // contig_cov_n = max_pos + 1 (0 when nothing is covered)
    int64_t contig_K = 0, contig_pairs = 0, contig_cov_n = 0;
    int64_t contig_P = 0, contig_max_pos = 0, contig_n_freq = 0;
    float contig_build_ms = 0.f, map_ms = 0.f;
    // the same contig by rank, but only the positions where the k-mer is frequent (freq_clouds, cloud_contig.py:35-36): what
    // the exact scorer of cf_score.hip intersects with; built and dropped together with the CSR above
    int64_t* d_exact_ptr = nullptr;    // contig_K + 1
    int32_t* d_exact_pos = nullptr;    // exact_pairs
    int64_t exact_pairs = 0;
    float score_ms = 0.f;

    // sequences left resident by cf_hpc (cf_edit.hip): the caller's bytes, their homopolymer-compressed form right behind them
    // and the padding; cf_edit_distances with bytes == NULL compares strings of these edit_len bytes
    uint8_t* d_edit = nullptr;
    size_t edit_cap = 0;
    int64_t edit_len = 0;

    // results of the last cf_tandem_scan (cf_tandem.hip): the hook positions as a CSR over its reads, and its shape and timings
    std::vector<int64_t> tandem_hook_ptr;
    std::vector<int32_t> tandem_hook_pos;
    cf_tandem_shape tandem_last{};

    // outputs of the last cf_consensus_run (cf_consensus.hip), in host memory: per iteration the bytes, their offsets and the
    // voting / excluded reads of every position; and the run's shape and timings
    std::vector<std::vector<uint8_t>> cons_bytes;
    std::vector<std::vector<int64_t>> cons_off;
    std::vector<std::vector<int32_t>> cons_voting, cons_excluded;
    // per iteration: the support of every output byte (cf_consensus_support; 16 bits, saturated, as the device keeps it), per read
    // its distance or -1 and its vote flag (cf_consensus_reads)
    std::vector<std::vector<uint16_t>> cons_agree;
    std::vector<std::vector<int32_t>> cons_dist;
    std::vector<std::vector<uint8_t>> cons_voted;
    cf_consensus_shape cons_last{};

    // results of the last cf_ualign_run (cf_ualign.hip), in host memory: the hits, the op strings as a CSR over its reads, and the
    // run's shape and timings
    std::vector<cf_ualign_hit> ualign_hits;
    std::vector<int64_t> ualign_op_ptr;
    std::vector<uint8_t> ualign_op_bytes;
    cf_ualign_shape ualign_last{};

    // results of the last cf_monodec_run (cf_monodec.hip), in host memory: the reads' records, the instances as a CSR over its reads,
    // and the run's shape and timings
    std::vector<cf_monodec_read> monodec_reads;
    std::vector<int64_t> monodec_ptr;
    std::vector<cf_monodec_inst> monodec_inst;
    cf_monodec_shape monodec_last{};

    // results of the last cf_monokmers_run (cf_monokmers.hip), in host memory: the k-mers in the order of first occurrence, their
    // occurrences as a CSR (when asked for), and the run's shape and timings
    bool monokmers_have = false;
    std::vector<cf_monokmer> monokmers_first;
    std::vector<int64_t> monokmers_ptr;
    std::vector<cf_monokmer_occ> monokmers_occ;
    cf_monokmers_shape monokmers_last{};

    // results of the last cf_monomap_run (cf_monomap.hip), in host memory: the reads' records, the paths as a CSR over its reads,
    // the hits as a CSR (when asked for), and the run's shape and timings
    bool monomap_have = false;
    std::vector<cf_monomap_read> monomap_reads;
    std::vector<int64_t> monomap_path_ptr, monomap_hit_ptr;
    std::vector<int32_t> monomap_path;
    std::vector<cf_monomap_hit> monomap_hits;
    cf_monomap_shape monomap_last{};

    // host <-> device copies of the caller's (pageable) buffers go through pinned staging slots, one per copy thread
    // (cf_api.hip: cf_copy_h2d / cf_copy_d2h)
    static constexpr int kCopyThreads = 16;      // slots; CF_COPY_THREADS (1 .. 16, default 16) picks how many are used
    void* pin_slot[kCopyThreads] = {nullptr};
    hipStream_t pin_stream[kCopyThreads] = {nullptr};
    size_t pin_bytes = 0;
    int copy_threads = 16;       // CF_COPY_THREADS (1 .. 16), read once by cf_create (round 5: 16 staged threads move 54 GB/s D2H, 8 moved 34 - 40)

    cf_stats stats{};
    cf_times times{};

    // the knobs of cf_set_param: one member per entry of cf_knobs.h, with its default
#define CF_KNOB(name, type, def, accepted, stored, refusal) type name = def;
#define CF_KNOB_AB(name, type, def, accepted, stored, refusal) type name = def;
#include "cf_knobs.h"
#undef CF_KNOB
#undef CF_KNOB_AB
};

int cf_fail(cf_ctx* ctx, int code, const std::string& msg);
// copies between device memory and memory of the CALLER (pageable): staged through pinned slots by several threads; `host`
// may also be a device pointer (the multi-GPU exchange hands device buffers to some getters): then one plain copy
int cf_copy_h2d(cf_ctx* ctx, void* dev, const void* host, size_t bytes);
int cf_copy_d2h(cf_ctx* ctx, void* host, const void* dev, size_t bytes);
int cf_alloc(cf_ctx* ctx, void** p, size_t bytes, const char* what);
void cf_release(cf_ctx* ctx, void* p, size_t bytes);

template <class T>
inline int cf_alloc_t(cf_ctx* ctx, T** p, size_t n, const char* what) {
    return cf_alloc(ctx, (void**)p, n * sizeof(T), what);
}
template <class T>
inline void cf_release_t(cf_ctx* ctx, T*& p, size_t n) {
    cf_release(ctx, (void*)p, n * sizeof(T));
    p = nullptr;
}

// Scratch buffers of one host function: every exit releases what the guard still holds, last taken first, with the size
// it was taken with.  keep() hands a buffer on (to the context or the caller), drop() releases one before the end.
struct cf_scratch {
    explicit cf_scratch(cf_ctx* c) : ctx(c) {}
    cf_scratch(const cf_scratch&) = delete;
    cf_scratch& operator=(const cf_scratch&) = delete;
    ~cf_scratch() { release_all(); }
    template <class T> int get(T** p, size_t n, const char* what) {
        const int rc = cf_alloc_t(ctx, p, n, what);
        if (rc == 0) held.emplace_back((void*)*p, n * sizeof(T));
        return rc;
    }
    void keep(void* p) { const auto it = find(p); if (it != held.end()) held.erase(it); }
    void drop(void* p) {
        const auto it = find(p);
        if (it == held.end()) return;
        cf_release(ctx, it->first, it->second);
        held.erase(it);
    }
    void release_all() {
        for (auto it = held.rbegin(); it != held.rend(); ++it) cf_release(ctx, it->first, it->second);
        held.clear();
    }

private:
    std::vector<std::pair<void*, size_t>>::iterator find(void* p) {
        return p ? std::find_if(held.begin(), held.end(), [p](const std::pair<void*, size_t>& e) { return e.first == p; }) : held.end();
    }
    cf_ctx* ctx;
    std::vector<std::pair<void*, size_t>> held;
};

#define CF_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return cf_fail(ctx, -5, std::string(#expr) + ": " + hipGetErrorString(e_));       \
    } while (0)
#define CF_TRY(expr)                  \
    do {                              \
        int rc_ = (expr);             \
        if (rc_ != 0) return rc_;     \
    } while (0)
#define CF_KERNEL_CHECK(name)                                                                 \
    do {                                                                                      \
        hipError_t e_ = hipGetLastError();                                                    \
        if (e_ != hipSuccess)                                                                 \
            return cf_fail(ctx, -5, std::string("launch of ") + name + ": " + hipGetErrorString(e_)); \
    } while (0)

static inline uint64_t cf_pow2_ceil(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
static inline int cf_grid_for(int64_t items, int per_block, int max_blocks) {
    int64_t b = (items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (int)b;
}

extern "C" int cf_comm_free(cf_ctx* ctx);   // cf_exchange.hip
void cf_edit_free(cf_ctx* ctx);              // cf_edit.hip: drops the sequences cf_hpc left resident

// primitives (cf_prims.hip)
// exclusive scans into 64-bit sums; *total (host; may be null) = the sum, 0 for n <= 0.  d_out == d_in is allowed for the
// 64-bit scan (cf_count.hip and cf_exchange.hip call it so): a thread of cf_scan_local has read its eight items before it
// writes any, and no other thread touches them, so the aliased __restrict__ pair never meets on one element
// (tests/primcheck.py pins in place == out of place through all three levels of the recursion).
int cf_scan_exclusive_i64(cf_ctx* ctx, const int64_t* d_in, int64_t* d_out, int64_t n, int64_t* total);
int cf_scan_exclusive_u32_to_i64(cf_ctx* ctx, const uint32_t* d_in, int64_t* d_out, int64_t n, int64_t* total);
// exclusive scan, in (digit, tile) order, of a tile-major digit histogram hist[tile * D + digit] (1 <= D <= 512, else -22)
// -> offs in the same layout; *d_total = the sum (device; may be null).  d_part, d_base: scratch of
// cf_tile_digit_chunks(n_tiles) * D entries.  n_tiles = 0: returns 0 with no launch; neither offs nor *d_total is written.
int cf_tile_digit_chunks(int n_tiles);
int cf_tile_digit_offsets(cf_ctx* ctx, const uint32_t* d_hist, int n_tiles, int D, int64_t* d_offs, int64_t* d_total, uint32_t* d_part, int64_t* d_base);
// stable LSD radix sort of 64-bit keys on the whole bytes that hold the `bits` low bits; result lands in d_keys (d_tmp is scratch)
int cf_radix_sort_u64(cf_ctx* ctx, unsigned long long* d_keys, unsigned long long* d_tmp, int64_t n, int bits);
int cf_radix_sort_u64_any(cf_ctx* ctx, unsigned long long* d_keys, unsigned long long* d_tmp, int64_t n, int bits, unsigned long long** result);
// stable LSD radix sort of n 16-byte records (four 32-bit words) by n_fields fields, least significant field first; field f
// is word words[f] (0 .. 3) with bits[f] (0 .. 32) significant bits.  The contract of `bits`: a field is sorted on the
// ceil(bits / 8) low BYTES of its word.  The bits of the word above that rounded width take no part (records equal below them
// keep their input order, whatever those bits hold); the bits between `bits` and the rounded width DO take part, so a caller
// whose word holds something else there either wants it sorted on or keeps it equal.  bits = 0 skips the field.  The sorted
// records end in d_recs (d_tmp: scratch of the same size), after an odd number of passes through a copy.
int cf_radix_sort_rec16(cf_ctx* ctx, void* d_recs, void* d_tmp, int64_t n, const int* words, const int* bits, int n_fields);
// keys per tile of the scan and records per tile of cf_radix_sort_rec16
int cf_scan_tile();
int cf_radix_rec16_tile();

// the equality classes of the valid windows of k letters (cf_monokmers.hip): what cf_monokmers_run and cf_monomap_run share
struct __attribute__((aligned(16))) cf_mk_rec { uint32_t w[4]; };
struct cf_mk_ranked {
    cf_mk_rec *rec, *rec2;      // the last round's sorted records (w[2] = the position), and the sort's buffer
    uint32_t *R, *dist, *head;  // per position: the ranks of the round before the last, the letters up to the next gap or string end; per record: head flags
    int64_t *e, *scalar;        // per record: the heads in front of it; two counters
    int64_t n_valid, n_classes, n_rounds, n_sorts, n_sort_passes;
    float sort_ms;
};
// The distances, the doubling rounds and, for k = 1, the grouping of the bytes.  d_bytes: the N letters of all strings back to back
// on the device, padded with zeros to a multiple of 4 and 16 more; d_off: n_strings + 1 offsets (d_off[s] - d_off[0] is where
// string s starts).  1 <= k <= N < 2^31.  Every buffer is taken through the caller's guard, each of N entries rounded up to a
// multiple of 4.  It leaves the last round's records sorted: the n_valid valid windows first, class by class, ascending position
// inside a class; head[i] marks a class's first record and e[i] = the heads in front of record i, so record i is of class
// e[i] + head[i] - 1 of n_classes.  n_valid = 0 when no window of k letters is valid.  who: the caller's name, for messages.
int cf_mk_rank_windows(cf_ctx* ctx, cf_scratch& tmp, const uint8_t* d_bytes, const int64_t* d_off, int64_t n_strings, int64_t N, int64_t k, int32_t gap,
                       const char* who, cf_mk_ranked* out);
int cf_mk_launch_cap(const cf_ctx* ctx);
