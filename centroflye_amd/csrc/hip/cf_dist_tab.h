// cf_dist_tab.h — the table layouts of cf_dist_kernel (cf_dist.hip): the (b, d) table in LDS behind one interface, with the
// launch's arguments, work-list records and constants that the layouts need.
#pragma once
#include "cf_common.h"

#define DIST_STAGE_CAP 1024              /* selected slots whose rows do not fit the workgroup's output chunk, staged per table pass (u16 slot indices) */
#define DIST_STACK 112
#define DIST_UNROLL 4
#define DIST_ITEM (64u * DIST_UNROLL)    /* cloud entries one wave takes per step: DIST_UNROLL consecutive ones per lane */
#define DIST_BM_BITS 65536u              /* bitmap over hash(b): k-mers that may have a selected edge */
#define DIST_HOT_CAP 2048u               /* slots the insert path can hand to the filter per pass (more: the filter scans the table) */
#define DIST_MEMBER_KEYS 8               /* masks of one b (its distances in the table) that a thread of the one-section member filter keeps in registers; a b with more walks its chain per member */
#define DIST_EDGE_CHUNK 8192ull          /* edge rows a workgroup reserves per global atomic */
#define DIST_OVQ 160u                    /* per-wave list of inserts whose first probe did not finish (run through the probe loop down to < 32 after every drain: 31 + the 128 a drain can park) */
#define DIST_LDS_HEAD (DIST_BM_BITS / 8 + 128)  /* bitmap + sh (32 words): the fixed head of the kernel's LDS */
#define DIST_CNT_MASK 0x7FFFFFu          /* 23-bit count */
#define DIST_SEL_BIT (1ull << 23)        /* slot selected by the A6 filter */

// One posting (= one unit g holding the first k-mer): its partner entries — the clouds of the units g+min_d ..
// min(read end, g+max_d) — are ONE contiguous CSR range [e0, e0 + len); ig is the index of g inside its read, nu the number of
// those partner units (cf_dist_edges refuses 2^32 cloud entries and more: e0 has 32 bits).
struct alignas(16) cf_dist_rec { uint32_t e0; uint32_t len; uint32_t ig; uint32_t nu; };

// One item = up to DIST_ITEM consecutive partner entries of one posting: what one wave takes per step.
//   e  index of its first entry in the cloud-entry arrays (32 bits: cf_dist_edges refuses more than 2^32 - DIST_ITEM entries)
//   m  [entries of the item (1 .. DIST_ITEM) : 16 | unit index of the posting inside its read, mod 65536 : 16]
struct alignas(8) cf_dist_item { uint32_t e, m; };
// One first k-mer of the launch, in processing order: its rank, its number of items and where its item records start.
// The records of a first k-mer are laid out per WAVE of the sweeping workgroup (W waves): item j belongs to wave j % W and is its
// record number j / W; wave w's records are the contiguous run [ibase + w * per, ...), per = ceil(n_items / W).
// (measured and not kept: the items dealt in blocks — wave w sweeps the items [w * per, (w + 1) * per), the records lie in item order
// and the fill kernel's stores are nearly coalesced — the set-up gains 0.6 ms of 18 and the kernel loses 15 of 263: dealt round robin
// the waves of a workgroup read neighbouring 1 KB runs of the entry stream at the same time.)
// Items are numbered useful ones first: the sketch sweep takes the items 0 .. n_useful - 1 only, the table sweep all of them (cf_items_fill_kernel).
// A head stands for a CLASS of first k-mers with equal posting lists: a is its representative, n_members how many k-mers it has
// (1 .. DIST_CLASS_CAP) and first_member where they stand, next to each other, in the launch's order list (a = order[first_member]).
struct alignas(16) cf_dist_head { uint32_t a, n_items; unsigned long long ibase; uint32_t n_entries, n_useful, n_members, first_member; };   // n_entries: partner entries (capped at 2^30 - 1)

struct cf_dist_args {
    const int64_t* post_ptr;
    const int32_t* post;
    const int64_t* cloud_ptr;
    const int32_t* entries;
    const int32_t* unit_rend;      // one past the last unit of the unit's read
    const int32_t* unit_rbeg;      // first unit of the unit's read
    const cf_dist_rec* urange;     // per unit: the partner range of a posting at this unit
    const uint16_t* entry_i;       // wide layout: per cloud entry the index of its unit inside its read
    const uint8_t* entry_i8;       // region layout: the same index mod 256
    uint32_t reg_shift;            // region layout: log2 of the number of table regions
    const uint32_t* packed;        // narrow layout: per cloud entry [unit index inside its read mod 256 : 8 | rank : 24]
    int64_t n_kmers;
    int32_t part, n_parts;
    int32_t min_d, max_d;       // min_d already clamped to >= 1
    uint32_t min_cov;
    double thr;
    uint32_t thr_num, thr_den;     // thr as an exact fraction when it is the literal 0.8 (4 / 5), else 0 / 0: the dominance test is then integer
    int32_t slots;
    uint32_t fill_limit;
    uint32_t est_limit;            // emissions one partition is expected to hold (fill_limit / expected distinct share)
    int32_t sketch;                // 1: count first in 8-bit counters, build the exact table only for k-mers that can pass min_cov
    uint32_t sk_counters, sk_shift, sk_mask;   // counters (a power of two that fits the LDS that is dead during the sketch sweep), 32 - log2 of it, and it - 1
    uint32_t sk_fbits, sk_fsh, sk_wshift, sk_fmask, sk_guard, sk_bytes;      // a counter's bits (8 or 4), log2 of that, log2 of the counters per word, its largest value, the value from which an add takes itself back (4-bit counters), bytes of the array
    const cf_dist_head* heads;     // the first k-mers of the launch in processing order (cf_items_fill_kernel) ...
    const cf_dist_item* items;     // ... and the item records of their sweeps, laid out per wave of a workgroup of blockDim.x threads
    uint32_t stage_cap;            // <= DIST_STAGE_CAP
    uint32_t filter_once;          // mask table: the members of a group are filtered in one section (knob dist_filter_once)
    uint32_t hot_cap;              // cap on the filter's list of hot slots (tests: a small one forces the in-scan evaluation)
    uint32_t hot_entries;          // first k-mers with more partner entries than this do not keep the list at all (it would overflow: the filter scans)
    uint32_t* edges;
    unsigned long long edge_cap;
    const uint32_t* member_mask;   // groups: per position of `order`, which postings of its group's union the k-mer has
    const int32_t* order;          // first k-mers of this partition, sorted by their first posting (locality); the members of a class stand next to each other
    int64_t n_order;               // heads of the launch: classes of first k-mers (every first k-mer of `order` when classes are off)
    unsigned long long edge_chunk; // edge rows a workgroup reserves per global atomic (DIST_EDGE_CHUNK; tests: small)
    unsigned long long* holes;     // (start, rows) of the unused rest of every workgroup's last chunk of the edge output
    unsigned long long* counters;  // [0] edge rows reserved (chunks) [6] selected edges [7] holes [1] partner entries swept [2] spilled a [3] (host: self pairs) [4] error flags [5] passes; [16 + 16 x] queue head x
    uint32_t* unique_bits;
};

// The 4-byte entry stream of the narrow / region26 layouts: 16 bytes per lane from entry s_e (wave-uniform) on.  Through a BUFFER
// load (round 5): the array's descriptor sits in four scalar registers, the item's byte offset is the instruction's scalar offset and
// the lane's share the constant 16 x lane — no vector instruction per fetch.  As a global load through a pointer the compiler folded
// the lane's offset into a 64-bit pointer per lane and added the item's offset with a v_lshl_add_u64 whose DESTINATION pair it then
// reused for the loaded data: the loop head had to wait for every load in flight before it could write the address
// (s_waitcnt vmcnt(0) once per D + 1 steps).  The scalar offset is 32 bits of bytes: streams of 2^30 entries and more
// take the layouts that stream rank and unit index apart (cf_dist_edges).  (The host emulator of tests/emu defines CF_NO_BUFFER_LOAD.)
typedef uint32_t cf_raw4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(4))) cf_run4 { uint32_t x, y, z, w; };
__device__ __forceinline__ void cf_load_packed4(const cf_dist_args& A, uint32_t s_e, uint32_t l4, uint32_t& x, uint32_t& y, uint32_t& z, uint32_t& w) {
#if !defined(CF_NO_BUFFER_LOAD)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)A.packed, 0, (int)0xFFFFFFFFu, 0x00020000);
    const cf_raw4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(l4 * 4u), (int)(s_e << 2), 0);
    x = v.x; y = v.y; z = v.z; w = v.w;
#else
    const uint32_t* p = A.packed + s_e;
    const cf_run4 r = *(const cf_run4*)(p + l4);
    x = r.x; y = r.y; z = r.z; w = r.w;
#endif
}

// ---------------------------------------------------------------------------------------------------
// The (b, d) table lives in LDS and is organised in 32-byte buckets read with two ds_read_b128: a probe
// inspects a whole bucket with straight-line code, so a wave does not run a per-lane probe loop in the
// common case.  A key lives in the first bucket, starting at home(b), that held a match or an empty slot
// when it was inserted; slots of a bucket fill in ascending order and never empty, so every (b, .) key sits
// between home(b) and the first bucket that still has an empty slot, and a key is never inserted twice.
// Two layouts with one interface:
//   cf_tab_wide    4 slots of 64 bits  [b:32 | d:8 | sel:1 | cnt:23]            any k-mer set size (cf_tab_wide16: [b:32 | d:16 | sel:1 | cnt:15] for max_d > 255)
//   cf_tab_narrow  8 keys of 32 bits   [d:8 | b:24] + 8 x 16-bit [sel:1 | cnt-1:15]  (6 bytes per slot: a third
//                  more slots in the same LDS, half as many full buckets, 32-bit compares) when the set has
//                  < 2^24 - 1 k-mers and no k-mer has more than 32767 postings.  A claimed slot counts 1 with
//                  its count field still 0 (most pairs are seen once: no second atomic for them); the cloud
//                  entries are pre-packed [unit index mod 256 : 8 | b : 24], so ONE 4-byte load and one
//                  subtraction give the key; hashing uses 24-bit multiplies (full rate, v_mul_u32_u24).
// b is a dense rank, so one odd multiplier spreads it; the home bucket comes from the high bits of the product.
struct alignas(16) cf_u64x2 { unsigned long long x, y; };
struct alignas(16) cf_u32x4 { uint32_t x, y, z, w; };

// DB = bits of the distance field: 8 (count 23 bits) for max_d <= 255, 16 (count 15 bits) beyond
template <int DB>
struct cf_tab_wide_t {
    static constexpr uint32_t kCntBits = 31 - DB, kCntMask = (1u << kCntBits) - 1u, kDMask = (1u << DB) - 1u, kDShift = 32 - DB;
    static constexpr uint32_t kSlotBytes = 8, kPerBucket = 4;
    static constexpr bool kMaskTab = false;      // (cf_tab_mask: a mask of the union's postings per slot)
    struct bucket { cf_u64x2 lo, hi; };
    struct raw { uint32_t b, i; };
    typedef unsigned long long qitem;   // deferred insert: [b:32 | d:8 | bucket to look at next:24]
    static __device__ __forceinline__ qitem q_make(uint32_t b, uint32_t dd, uint32_t bk) { return ((unsigned long long)b << 32) | ((unsigned long long)dd << kDShift) | bk; }
    static __device__ __forceinline__ void q_take(qitem q, uint32_t n_buckets, uint32_t& b, uint32_t& dd, uint32_t& bk) { b = (uint32_t)(q >> 32); dd = ((uint32_t)q >> kDShift) & kDMask; bk = (uint32_t)q & ((1u << kDShift) - 1u); }
    __device__ __forceinline__ qitem q_of(uint32_t b, uint32_t dd, uint32_t n_buckets) const { return q_make(b, dd, home(hash(b), n_buckets)); }
    static __device__ __forceinline__ uint32_t next(uint32_t bk, uint32_t, uint32_t n_buckets) { return bk + 1 == n_buckets ? 0u : bk + 1; }
    __device__ __forceinline__ void configure(const cf_dist_args&, uint32_t) {}
    unsigned long long* tab;
    __device__ __forceinline__ void init(unsigned char* lds, uint32_t) { tab = (unsigned long long*)lds; }
    __device__ __forceinline__ void clear(uint32_t slots, uint32_t t, uint32_t nt) const {
        const cf_u64x2 z{0ull, 0ull};
        for (uint32_t s = t; s < (slots >> 1); s += nt) ((cf_u64x2*)tab)[s] = z;
    }
    // streaming side: one cloud entry -> (b, d)
    // DIST_UNROLL consecutive entries from e on; entries whose bit in ok is clear are not touched in memory
    struct __attribute__((packed, aligned(4))) run4 { uint32_t x, y, z, w; };
    struct __attribute__((packed, aligned(2))) run4h { uint16_t x, y, z, w; };
    // s_e: index of the item's first entry (wave-uniform: the base address is scalar), l4 = 4 * lane
    static __device__ __forceinline__ void load_run(const cf_dist_args& A, uint32_t s_e, uint32_t l4, uint32_t ok, raw (&out)[DIST_UNROLL]) {
        static_assert(DIST_UNROLL == 4, "one 16-byte and one 8-byte load per lane");
        const int32_t* pe = A.entries + s_e;
        const uint16_t* pi = A.entry_i + s_e;
        if (ok == (1u << DIST_UNROLL) - 1u) {      // the whole run lies inside the posting's range (all items but the last of a posting)
            const run4 r = *(const run4*)(pe + l4);
            const run4h h = *(const run4h*)(pi + l4);
            out[0] = raw{r.x, h.x}; out[1] = raw{r.y, h.y}; out[2] = raw{r.z, h.z}; out[3] = raw{r.w, h.w};
            return;
        }
#pragma unroll
        for (int u = 0; u < DIST_UNROLL; ++u) { const uint32_t x = ((ok >> u) & 1u) ? l4 + (uint32_t)u : 0u; out[u] = raw{(uint32_t)pe[x], (uint32_t)pi[x]}; }
    }
    static __device__ __forceinline__ void decode(const raw& r, uint32_t ig, uint32_t, uint32_t& b, uint32_t& dd, uint32_t& qk, uint32_t& lo) { b = r.b; dd = (r.i - ig) & 0xFFFFu; qk = 0u; lo = r.b; }
    __device__ __forceinline__ qitem q_push(uint32_t b, uint32_t dd, uint32_t, uint32_t n_buckets) const { return q_of(b, dd, n_buckets); }   // unit indices are kept mod 65536 and d <= max_d < 65536: the 16-bit difference IS d
    // 24 x 24-bit multiplies only (full rate; a 32-bit multiply or a multiply-high is quarter rate): the low 24 bits of b as in
    // the narrow layout, the high 8 bits through a second multiplier
    static __device__ __forceinline__ uint32_t hash(uint32_t b) { return (b & 0xFFFFFFu) * 0x9E3779u + (b >> 24) * 0x85EBCBu; }
    static __device__ __forceinline__ uint32_t home(uint32_t h, uint32_t n_buckets) { return ((h >> 16) * (n_buckets & 0xFFFFu)) >> 16; }
    static __device__ __forceinline__ uint32_t bm_bit(uint32_t b) { return b & (DIST_BM_BITS - 1u); }      // (k-mer ranks: their low bits are as good as a hash of them, and cost nothing)
    static __device__ __forceinline__ uint32_t sk_hash(uint32_t b, uint32_t dd, uint32_t) { return hash(b) + dd * 0x5BD1E9u; }      // the sketch's counter of the pair (b, d): its high bits
    __device__ __forceinline__ bucket read(uint32_t bk) const { return bucket{*(const cf_u64x2*)&tab[4 * bk], *(const cf_u64x2*)&tab[4 * bk + 2]}; }
    static __device__ __forceinline__ bool is(unsigned long long v, uint32_t b, uint32_t dd) { return (uint32_t)(v >> 32) == b && ((uint32_t)v >> kDShift) == dd; }
    // branch-free: one bit per slot, then find-first-set (nested ?: chains compile to a cascade of exec-mask branches)
    static __device__ __forceinline__ int match(const bucket& k, uint32_t b, uint32_t dd) {   // dd >= 1: an empty slot never matches
        const uint32_t m = (uint32_t)is(k.lo.x, b, dd) | ((uint32_t)is(k.lo.y, b, dd) << 1) | ((uint32_t)is(k.hi.x, b, dd) << 2) | ((uint32_t)is(k.hi.y, b, dd) << 3);
        return __ffs((int)m) - 1;
    }
    static __device__ __forceinline__ int empty(const bucket& k) {
        const uint32_t m = (uint32_t)(k.lo.x == 0ull) | ((uint32_t)(k.lo.y == 0ull) << 1) | ((uint32_t)(k.hi.x == 0ull) << 2) | ((uint32_t)(k.hi.y == 0ull) << 3);
        return __ffs((int)m) - 1;
    }
    // counts one more occurrence of the key in slot i of bucket bk; returns its count after the add
    __device__ __forceinline__ uint32_t add(uint32_t bk, int i) const { return ((uint32_t)atomicAdd(&tab[4 * bk + i], 1ull) & kCntMask) + 1u; }
    static constexpr uint32_t kSlotsPerBucket = 4;
    static constexpr bool kDrainTwoProbes = false;      // (64-bit slots: the drain takes one queued insert per lane through match / claim branches)
    __device__ __forceinline__ void probe2(bool, uint32_t, uint32_t, bool, uint32_t, uint32_t, uint32_t, bool&, bool&, uint32_t&, bool&, bool&, uint32_t&) const {}
    __device__ __forceinline__ uint32_t key_of(uint32_t, uint32_t) const { return 0u; }
    // claim slot i of bucket bk for (b, dd): 0 = claimed (count 1), 1 = the same key got there first (counted), 2 = another key
    __device__ __forceinline__ unsigned long long claim_issue(uint32_t bk, int i, uint32_t b, uint32_t dd) const {
        return atomicCAS(&tab[4 * bk + i], 0ull, ((unsigned long long)b << 32) | ((unsigned long long)dd << kDShift) | 1ull);
    }
    __device__ __forceinline__ int claim_finish(unsigned long long old, uint32_t bk, int i, uint32_t b, uint32_t dd, uint32_t& cnt) const {
        cnt = 1u;
        if (old == 0ull) return 0;
        if (is(old, b, dd)) { cnt = add(bk, i); return 1; }
        return 2;
    }
    // filter side: slot s -> (b, dd, cnt) or false when empty
    __device__ __forceinline__ bool get(uint32_t s, uint32_t& b, uint32_t& dd, uint32_t& cnt) const {
        const unsigned long long v = tab[s];
        b = (uint32_t)(v >> 32); dd = ((uint32_t)v >> kDShift) & kDMask; cnt = (uint32_t)v & kCntMask;
        return v != 0ull;
    }
    __device__ __forceinline__ unsigned long long total_of(uint32_t b, uint32_t n_buckets) const {
        unsigned long long total = 0;
        uint32_t bk = home(hash(b), n_buckets);
        for (uint32_t probe = 0; probe < n_buckets; ++probe) {
            const bucket k = read(bk);
            if ((uint32_t)(k.lo.x >> 32) == b && k.lo.x) total += k.lo.x & (unsigned long long)kCntMask;
            if ((uint32_t)(k.lo.y >> 32) == b && k.lo.y) total += k.lo.y & (unsigned long long)kCntMask;
            if ((uint32_t)(k.hi.x >> 32) == b && k.hi.x) total += k.hi.x & (unsigned long long)kCntMask;
            if ((uint32_t)(k.hi.y >> 32) == b && k.hi.y) total += k.hi.y & (unsigned long long)kCntMask;
            if (empty(k) >= 0) break;
            bk = bk + 1 == n_buckets ? 0u : bk + 1;
        }
        return total;
    }
    // filter side: f(slot, b, dd, cnt, sum over d of cnt(b, .)) for the occupied slots of bucket bk whose count is at least min_cov
    template <class F>
    __device__ __forceinline__ void for_counts_at_least(uint32_t bk, uint32_t n_buckets, uint32_t min_cov, F&& f) const {
        const bucket k = read(bk);
        const unsigned long long v[4] = {k.lo.x, k.lo.y, k.hi.x, k.hi.y};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t cnt = (uint32_t)v[i] & kCntMask;
            if (v[i] != 0ull && cnt >= min_cov) f(4u * bk + (uint32_t)i, (uint32_t)(v[i] >> 32), ((uint32_t)v[i] >> kDShift) & kDMask, cnt, total_of((uint32_t)(v[i] >> 32), n_buckets));
        }
    }
    // filter, two steps: the slots of bucket bk whose count reaches min_cov as a bit mask ...
    static constexpr uint32_t kScanGroup = 4;      // slots per step of the scan (one bucket)
    static __device__ __forceinline__ uint32_t slot_of_bit(uint32_t bit) { return bit; }      // hot_mask: bit i = slot i of the group
    __device__ __forceinline__ uint32_t hot_mask(uint32_t bk, uint32_t min_cov) const {
        const bucket k = read(bk);
        const unsigned long long v[4] = {k.lo.x, k.lo.y, k.hi.x, k.hi.y};
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) m |= (uint32_t)(v[i] != 0ull && ((uint32_t)v[i] & kCntMask) >= min_cov) << i;
        return m;
    }
    // ... and one such slot evaluated: f(slot, b, dd, cnt, sum over d of cnt(b, .))
    template <class F>
    __device__ __forceinline__ void eval_slot(uint32_t s, uint32_t n_buckets, uint32_t min_cov, F&& f) const {
        const unsigned long long v = tab[s];
        const uint32_t cnt = (uint32_t)v & kCntMask;
        if (v != 0ull && cnt >= min_cov) f(s, (uint32_t)(v >> 32), ((uint32_t)v >> kDShift) & kDMask, cnt, total_of((uint32_t)(v >> 32), n_buckets));
    }
    template <class F>
    __device__ __forceinline__ void for_marked(uint32_t bk, F&& f) const {
        const bucket k = read(bk);
        const unsigned long long v[4] = {k.lo.x, k.lo.y, k.hi.x, k.hi.y};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((v[i] >> kCntBits) & 1ull) f(4u * bk + (uint32_t)i, (uint32_t)(v[i] >> 32), ((uint32_t)v[i] >> kDShift) & kDMask, (uint32_t)v[i] & kCntMask);
    }
    __device__ __forceinline__ void mark(uint32_t s) const { atomicOr(&tab[s], 1ull << kCntBits); }
    __device__ __forceinline__ void unmark(uint32_t s) const { atomicAnd(&tab[s], ~(1ull << kCntBits)); }      // (between the members of a class: DESIGN.md 24)
};
typedef cf_tab_wide_t<8> cf_tab_wide;
typedef cf_tab_wide_t<16> cf_tab_wide16;

// DB = bits of the distance field (5 .. 8): the key is [d : DB | b : 32 - DB].  d never exceeds min(max_d, units of the longest
// read - 1), so sets of up to 2^27 - 2 k-mers keep the 6-byte slots when the reads are short enough in units (multi-GPU
// runs sweep the union of all ranks' k-mers: 6e7 at 8 x 50 000 reads).  Hashes use the low 24 bits of b only.
// Two probes of the 6-byte-slot tables side by side (the drain of the table sweep: two queued inserts per lane), ONE probe of its home
// bucket each in straight-line code: match -> count it; no match and a free slot -> claim the first one (the zero count field of a fresh
// slot already means "seen once"; the same key claimed by another lane a moment ago counts as a match); anything else -> park.  Written
// stage by stage for both inserts — both bucket reads, both slot searches, both claims, both count adds — so that the two chains of LDS
// round trips are in flight together.  Two inserts of one lane may meet in one bucket: they then behave like two lanes that do (the
// second claim of the same key sees the key and counts; another key's parks).
// Flags are integers made by selects, the count add is issued by every lane (adding 0 where there is nothing to count): as nested ifs
// that set booleans on divergent paths the drain compiled to ~115 scalar instructions of exec-mask bookkeeping per 64 inserts
// (profiles/r04_dist_phase_insts.md: the inserts were 0.27 of the kernel's 0.58 scalar instructions per pair).  EVERY lane of the wave
// runs it (act = the lane has an insert): under `if (lane < n)` the flags crossed the join in vector registers and came back through
// compares.  A lane without an insert — only the last drain of a sweep has any — reads some bucket and changes nothing.
// (Measured and not kept, round 6: an insert that finds its bucket full without its key, or loses the slot it wanted to another key, gets
// a SECOND straight-line probe at once — of the next bucket of its chain, or the same one again — before it is parked.  On cenX-shaped
// reads 4 % of the inserts park (2.2 trips of the probe loop each, 28 lanes per run: a run takes 4 400 cycles — every LDS round trip under
// this kernel's load is 350-650 cycles; profiles/r06_dist_ab_cenx.log): 117.5 (every lane) / 118.0 ms (parked lanes only) against 108.0
// without on those reads, 249 against 240.6 on the bench's — the second probe's LDS round trips cost every drain more than the parked
// inserts' loop costs the few.)
template <class Tab>
__device__ __forceinline__ void cf_probe2(const Tab& T, bool act0, uint32_t bk0, uint32_t key0, bool act1, uint32_t bk1, uint32_t key1, uint32_t min_cov,
                                          bool& made0, bool& park0, uint32_t& hot0, bool& made1, bool& park1, uint32_t& hot1) {
    constexpr int PB_ = (int)Tab::kPerBucket;
    // (a lambda, called once below: the same lines written straight into the function come out of the compiler in another order and with
    // other registers — the shape the measurements were made with stays)
    auto stage = [&](bool a0, uint32_t k0b, bool a1, uint32_t k1b, bool& md0, bool& pk0, uint32_t& ht0, bool& md1, bool& pk1, uint32_t& ht1) {
        const typename Tab::bucket k0 = T.read(k0b), k1 = T.read(k1b);
        // the slot of the key, else the first empty one, else PB_: two chains of selects over the slots (a compare and a v_cndmask each;
        // as bit masks + find-first-set the two searches took 26 instructions instead of 16)
        uint32_t em0 = (uint32_t)PB_, em1 = (uint32_t)PB_;
#pragma unroll
        for (int j = PB_ - 1; j >= 0; --j) { em0 = k0.k[j] == Tab::kEmpty ? (uint32_t)j : em0; em1 = k1.k[j] == Tab::kEmpty ? (uint32_t)j : em1; }
        uint32_t sl0 = em0, sl1 = em1;
        bool mt0 = false, mt1 = false;
#pragma unroll
        for (int j = PB_ - 1; j >= 0; --j) {
            const bool e0 = k0.k[j] == key0, e1 = k1.k[j] == key1;
            sl0 = e0 ? (uint32_t)j : sl0; mt0 |= e0; sl1 = e1 ? (uint32_t)j : sl1; mt1 |= e1;
        }
        mt0 &= a0; mt1 &= a1;
        const bool claim0 = a0 && !mt0 && em0 < (uint32_t)PB_, claim1 = a1 && !mt1 && em1 < (uint32_t)PB_;
        const uint32_t s0 = (uint32_t)PB_ * k0b + (sl0 & (uint32_t)(PB_ - 1)), s1 = (uint32_t)PB_ * k1b + (sl1 & (uint32_t)(PB_ - 1));      // (nothing to do in a full bucket without the key: slot 0's address for the adds of 0 below)
        uint32_t old0 = key0, old1 = key1;
        if (claim0) old0 = atomicCAS(&T.keys[s0], Tab::kEmpty, key0);
        if (claim1) old1 = atomicCAS(&T.keys[s1], Tab::kEmpty, key1);
        const bool matched0 = mt0 || (claim0 && old0 == key0), fresh0 = claim0 && old0 == Tab::kEmpty;
        const bool matched1 = mt1 || (claim1 && old1 == key1), fresh1 = claim1 && old1 == Tab::kEmpty;
        const uint32_t sh0 = (s0 & 1u) * 16u, sh1 = (s1 & 1u) * 16u;
        const uint32_t was0 = atomicAdd(&T.cnt32[s0 >> 1], matched0 ? 1u << sh0 : 0u);
        const uint32_t was1 = atomicAdd(&T.cnt32[s1 >> 1], matched1 ? 1u << sh1 : 0u);
        const uint32_t cnt0 = matched0 ? ((was0 >> sh0) & 0x7FFFu) + 2u : 1u, cnt1 = matched1 ? ((was1 >> sh1) & 0x7FFFu) + 2u : 1u;
        md0 = fresh0; pk0 = a0 && !(matched0 || fresh0); ht0 = ((matched0 || fresh0) && cnt0 == min_cov) ? s0 : 0xFFFFFFFFu;
        md1 = fresh1; pk1 = a1 && !(matched1 || fresh1); ht1 = ((matched1 || fresh1) && cnt1 == min_cov) ? s1 : 0xFFFFFFFFu;
    };
    stage(act0, bk0, act1, bk1, made0, park0, hot0, made1, park1, hot1);
}

// PB = keys per bucket: 4, one 16-byte read of keys (measured and not kept: 8, two reads — 293.1 ms against 251.7, DESIGN.md "Retired compile-time switches")
template <int DB, int PB = 4>
struct cf_tab_narrow_t {
    static_assert(PB == 4, "a bucket is one 16-byte read of keys");
    static constexpr uint32_t kBBits = 32 - DB, kBMask = (1u << kBBits) - 1u;
    static constexpr uint32_t kSlotBytes = 6, kPerBucket = PB, kAll = (1u << PB) - 1u;
    static constexpr bool kMaskTab = false;
    static constexpr uint32_t kEmpty = 0xFFFFFFFFu;
    struct bucket { uint32_t k[PB]; };
    struct counts { uint32_t w[PB / 2]; };      // PB x 16-bit [sel:1 | count - 1 : 15]
    struct raw { uint32_t v; };
    typedef uint32_t qitem;             // deferred insert: the key; probing restarts at the home bucket
    static __device__ __forceinline__ qitem q_make(uint32_t b, uint32_t dd, uint32_t) { return key_of(b, dd); }
    static __device__ __forceinline__ void q_take(qitem q, uint32_t n_buckets, uint32_t& b, uint32_t& dd, uint32_t& bk) { b = q & kBMask; dd = q >> kBBits; bk = home(hash(b), n_buckets); }
    __device__ __forceinline__ qitem q_of(uint32_t b, uint32_t dd, uint32_t) const { return key_of(b, dd); }
    static __device__ __forceinline__ uint32_t next(uint32_t bk, uint32_t, uint32_t n_buckets) { return bk + 1 == n_buckets ? 0u : bk + 1; }
    __device__ __forceinline__ void configure(const cf_dist_args&, uint32_t) {}
    uint32_t* keys;     // slots x 32-bit [d : DB | b : 32 - DB]
    uint32_t* cnt32;    // slots x 16-bit [sel:1 | count - 1 : 15], two per word
    __device__ __forceinline__ void init(unsigned char* lds, uint32_t slots) { keys = (uint32_t*)lds; cnt32 = keys + slots; }
    __device__ __forceinline__ void clear(uint32_t slots, uint32_t t, uint32_t nt) const {
        const cf_u32x4 e{kEmpty, kEmpty, kEmpty, kEmpty}, z{0u, 0u, 0u, 0u};
        for (uint32_t s = t; s < (slots >> 2); s += nt) ((cf_u32x4*)keys)[s] = e;
        for (uint32_t s = t; s < (slots >> 3); s += nt) ((cf_u32x4*)cnt32)[s] = z;
    }
    // DIST_UNROLL (= 4) consecutive entries from e on with ONE 16-byte load (4-byte aligned); the packed array is
    // padded by DIST_ITEM entries, so a run that starts inside the array may be read whole whatever ok says
    struct __attribute__((packed, aligned(4))) run4 { uint32_t x, y, z, w; };
    static __device__ __forceinline__ void load_run(const cf_dist_args& A, uint32_t s_e, uint32_t l4, uint32_t, raw (&out)[DIST_UNROLL]) {
        static_assert(DIST_UNROLL == 4, "one 16-byte load per lane");
        cf_load_packed4(A, s_e, l4, out[0].v, out[1].v, out[2].v, out[3].v);
    }
    // the unit index is kept mod 2^DB and 1 <= d < 2^DB, so the DB-bit difference IS d; no borrow reaches b
    static __device__ __forceinline__ void decode(const raw& r, uint32_t ig, uint32_t, uint32_t& b, uint32_t& dd, uint32_t& qk, uint32_t& lo) { const uint32_t q = r.v - (ig << kBBits); b = q & kBMask; dd = q >> kBBits; qk = q; lo = r.v; }      // (lo: a word whose low 16 bits are b's — the bitmap's index — that costs nothing to make)
    // (the queued insert IS the difference decode() made: [d | b]; rebuilt from b and d it cost three more instructions per entry)
    __device__ __forceinline__ qitem q_push(uint32_t, uint32_t, uint32_t qk, uint32_t) const { return qk; }
    static __device__ __forceinline__ uint32_t hash(uint32_t b) { return (b & 0xFFFFFFu) * 0x9E3779u; }               // 24 x 24 -> low 32 bits
    static __device__ __forceinline__ uint32_t home(uint32_t h, uint32_t n_buckets) { return ((h >> 16) * (n_buckets & 0xFFFFu)) >> 16; }
    static __device__ __forceinline__ uint32_t bm_bit(uint32_t b) { return b & (DIST_BM_BITS - 1u); }      // (k-mer ranks: their low bits are as good as a hash of them, and cost nothing)
    // the sketch's counter of the pair (b, d), from the decoded difference q = [d | b] itself: one multiply-add (b's low 24 bits times the
    // constant, plus q: d lands in the counter index's high bits, so the pairs of one b never share a counter)
    static __device__ __forceinline__ uint32_t sk_hash(uint32_t, uint32_t, uint32_t qk) { return (qk & 0xFFFFFFu) * 0x9E3779u + qk; }
    __device__ __forceinline__ bucket read(uint32_t bk) const {
        bucket r;
#pragma unroll
        for (int q = 0; q < PB / 4; ++q) { const cf_u32x4 v = *(const cf_u32x4*)&keys[PB * bk + 4 * q]; r.k[4 * q] = v.x; r.k[4 * q + 1] = v.y; r.k[4 * q + 2] = v.z; r.k[4 * q + 3] = v.w; }
        return r;
    }
    __device__ __forceinline__ counts read_counts(uint32_t bk) const {
        counts c;
        const unsigned long long v = *(const unsigned long long*)&cnt32[2 * bk];
        c.w[0] = (uint32_t)v; c.w[1] = (uint32_t)(v >> 32);
        return c;
    }
    static __device__ __forceinline__ uint32_t field(const counts& c, int j) { return (c.w[j >> 1] >> ((j & 1) * 16)) & 0x7FFFu; }      // count - 1 of slot j
    static __device__ __forceinline__ uint32_t key_of(uint32_t b, uint32_t dd) { return (dd << kBBits) | b; }
    // branch-free: one bit per slot, then find-first-set (nested ?: chains compile to a cascade of exec-mask branches)
    static __device__ __forceinline__ uint32_t ne_bit(uint32_t k, uint32_t q) { return min(k ^ q, 1u); }
    static __device__ __forceinline__ int first_equal(const bucket& k, uint32_t q) {
        uint32_t ne = 0;
#pragma unroll
        for (int j = 0; j < PB; ++j) ne |= ne_bit(k.k[j], q) << j;
        return __ffs((int)(ne ^ kAll)) - 1;
    }
    static __device__ __forceinline__ int match(const bucket& k, uint32_t b, uint32_t dd) { return first_equal(k, key_of(b, dd)); }
    static __device__ __forceinline__ int empty(const bucket& k) { return first_equal(k, kEmpty); }
    // counts one more occurrence of the key in slot i of bucket bk; returns its count after the add (the field holds count - 1)
    __device__ __forceinline__ uint32_t add(uint32_t bk, int i) const {
        const uint32_t s = PB * bk + (uint32_t)i, sh_ = (s & 1u) * 16u;
        return ((atomicAdd(&cnt32[s >> 1], 1u << sh_) >> sh_) & 0x7FFFu) + 2u;
    }
    static constexpr uint32_t kSlotsPerBucket = PB;
    __device__ __forceinline__ uint32_t claim_issue(uint32_t bk, int i, uint32_t b, uint32_t dd) const { return atomicCAS(&keys[PB * bk + i], kEmpty, key_of(b, dd)); }
    __device__ __forceinline__ int claim_finish(uint32_t old, uint32_t bk, int i, uint32_t b, uint32_t dd, uint32_t& cnt) const {
        cnt = 1u;
        if (old == kEmpty) return 0;                        // claimed: the zero count field already means "seen once"
        if (old == key_of(b, dd)) { cnt = add(bk, i); return 1; }  // the same key was claimed by someone else: count it
        return 2;
    }
    static constexpr bool kDrainTwoProbes = true;      // the drain of the table sweep: two queued inserts per lane, one straight-line probe each (cf_probe2)
    __device__ __forceinline__ void probe2(bool act0, uint32_t bk0, uint32_t key0, bool act1, uint32_t bk1, uint32_t key1, uint32_t min_cov,
                                           bool& made0, bool& park0, uint32_t& hot0, bool& made1, bool& park1, uint32_t& hot1) const {
        cf_probe2(*this, act0, bk0, key0, act1, bk1, key1, min_cov, made0, park0, hot0, made1, park1, hot1);
    }
    __device__ __forceinline__ bool get(uint32_t s, uint32_t& b, uint32_t& dd, uint32_t& cnt) const {
        const uint32_t q = keys[s];
        b = q & kBMask; dd = q >> kBBits; cnt = ((cnt32[s >> 1] >> ((s & 1u) * 16u)) & 0x7FFFu) + 1u;
        return q != kEmpty;
    }
    // sum of the counts of the keys (b, .) among the PB keys of a bucket
    static __device__ __forceinline__ uint32_t sum_of(const bucket& k, const counts& c, uint32_t b) {
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < PB; ++j)
            if ((k.k[j] & kBMask) == b && k.k[j] != kEmpty) total += field(c, j) + 1u;
        return total;
    }
    __device__ __forceinline__ unsigned long long total_of(uint32_t b, uint32_t n_buckets) const {
        unsigned long long total = 0;
        uint32_t bk = home(hash(b), n_buckets);
        for (uint32_t probe = 0; probe < n_buckets; ++probe) {
            const bucket k = read(bk);
            total += sum_of(k, read_counts(bk), b);
            if (k.k[PB - 1] == kEmpty) break;       // slots fill in ascending order: an empty last slot = the chain ends here
            bk = bk + 1 == n_buckets ? 0u : bk + 1;
        }
        return total;
    }
    template <class F>
    __device__ __forceinline__ void for_counts_at_least(uint32_t bk, uint32_t n_buckets, uint32_t min_cov, F&& f) const {
        const counts c = read_counts(bk);
        const uint32_t need = min_cov ? min_cov - 1u : 0u;     // on the stored field (count - 1)
        bool any = false;
#pragma unroll
        for (int j = 0; j < PB; ++j) any |= field(c, j) >= need;
        if (!any) return;
        const bucket k = read(bk);
        const bool open_bucket = k.k[PB - 1] == kEmpty;
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const uint32_t cnt = field(c, i) + 1u;
            if (cnt >= min_cov && k.k[i] != kEmpty) {
                const uint32_t b = k.k[i] & kBMask;
                // usual case: b lives in its home bucket and the bucket is not full, so all (b, .) keys are in the
                // registers already — no chain walk through LDS
                const unsigned long long total = (open_bucket && home(hash(b), n_buckets) == bk) ? (unsigned long long)sum_of(k, c, b) : total_of(b, n_buckets);
                f((uint32_t)PB * bk + (uint32_t)i, b, k.k[i] >> kBBits, cnt, total);
            }
        }
    }
    // filter, two steps: the slots of bucket bk whose count field reaches min_cov - 1 as a bit mask (an empty slot has the
    // field 0: with min_cov <= 1 it is in the mask and eval_slot drops it) ...
    static constexpr uint32_t kScanGroup = 8;      // slots per step of the scan: 16 bytes of count fields, whatever the bucket size
    // two 16-bit fields per word compared at once: (field & 0x7FFF) + (0x8000 - need) has bit 15 set iff the field reaches need
    // (no carry leaves a half: both terms are <= 0x8000).  Bit 2j of the result = slot 2j of the group, bit 16 + 2j = slot 2j + 1.
    __device__ __forceinline__ uint32_t hot_mask(uint32_t g, uint32_t min_cov) const {
        const cf_u32x4 v = *(const cf_u32x4*)&cnt32[4 * g];
        const uint32_t need = min(min_cov ? min_cov - 1u : 0u, 0x8000u);
        const uint32_t add = 0x80008000u - need * 0x00010001u;
        const uint32_t y0 = ((v.x & 0x7FFF7FFFu) + add) & 0x80008000u, y1 = ((v.y & 0x7FFF7FFFu) + add) & 0x80008000u;
        const uint32_t y2 = ((v.z & 0x7FFF7FFFu) + add) & 0x80008000u, y3 = ((v.w & 0x7FFF7FFFu) + add) & 0x80008000u;
        return (y0 >> 15) | (y1 >> 13) | (y2 >> 11) | (y3 >> 9);
    }
    static __device__ __forceinline__ uint32_t slot_of_bit(uint32_t bit) { return (bit & 15u) + (bit >> 4); }
    // ... and one such slot evaluated: f(slot, b, dd, cnt, sum over d of cnt(b, .)).  Usual case: b lives in its home bucket
    // and the bucket is not full, so all (b, .) keys are among the keys just read — no chain walk through LDS.
    template <class F>
    __device__ __forceinline__ void eval_slot(uint32_t s, uint32_t n_buckets, uint32_t min_cov, F&& f) const {
        const uint32_t bk = s / (uint32_t)PB, i = s % (uint32_t)PB;
        const bucket k = read(bk);
        const counts c = read_counts(bk);
        uint32_t mine = k.k[0], mine_f = field(c, 0);
#pragma unroll
        for (int j = 1; j < PB; ++j) { if (i == (uint32_t)j) { mine = k.k[j]; mine_f = field(c, j); } }
        const uint32_t cnt = mine_f + 1u;
        if (mine == kEmpty || cnt < min_cov) return;
        const uint32_t b = mine & kBMask;
        const unsigned long long total = (k.k[PB - 1] == kEmpty && home(hash(b), n_buckets) == bk) ? (unsigned long long)sum_of(k, c, b) : total_of(b, n_buckets);
        f(s, b, mine >> kBBits, cnt, total);
    }
    template <class F>
    __device__ __forceinline__ void for_marked(uint32_t bk, F&& f) const {
        const counts c = read_counts(bk);
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < PB / 2; ++j) any |= c.w[j];
        if (!(any & 0x80008000u)) return;       // no selected slot in the bucket
        const bucket k = read(bk);
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const uint32_t h = c.w[i >> 1] >> ((i & 1) * 16);
            if (h & 0x8000u) f((uint32_t)PB * bk + (uint32_t)i, k.k[i] & kBMask, k.k[i] >> kBBits, (h & 0x7FFFu) + 1u);
        }
    }
    __device__ __forceinline__ void mark(uint32_t s) const { atomicOr(&cnt32[s >> 1], 0x8000u << ((s & 1u) * 16u)); }
    __device__ __forceinline__ void unmark(uint32_t s) const { atomicAnd(&cnt32[s >> 1], ~(0x8000u << ((s & 1u) * 16u))); }
};
typedef cf_tab_narrow_t<8> cf_tab_narrow;

// The table of a GROUP of first k-mers: the 4-byte stream, the keys [d : DB | b : 32 - DB], the 4-key buckets and the hashes of
// the 6-byte layout, but a slot's second half is a 32-bit MASK of the postings of the group's union U that brought the pair (b, d): an
// insert is a returning `or` of the posting's bit, and for the member a_j with the list mask M_j
//     cnt(a_j, b, d) = popcount(mask & M_j),     sum_d cnt(a_j, b, .) = the same sum over the keys of b.
// Exact because a cloud row is a set (a posting brings a pair at most once).  A group that cannot take masks — ONE first k-mer with more
// postings than the mask has bits, or any first k-mer of clouds that are not sets — is `counting`: the same word is a plain 32-bit count
// (add 1 per occurrence), which is what the other layouts keep.  The selection marks of late rows (cf_dist_kernel) have no bit left in a
// slot: they stand in a bitmap of their own behind the masks.  8 bytes + 1 bit per slot.
template <int DB>
struct cf_tab_mask : cf_tab_narrow_t<DB, 4> {
    typedef cf_tab_narrow_t<DB, 4> N;
    typedef typename N::bucket bucket;
    static constexpr uint32_t kSlotBytes = 8, kEmpty = N::kEmpty, kBMask = N::kBMask, kBBits = N::kBBits;
    static constexpr bool kMaskTab = true;
    uint32_t* msk;      // slots x 32-bit mask (or count)
    uint32_t* mk;       // slots x 1 bit: selected, row not yet written
    uint32_t mm;        // the list mask of the member whose rows are made
    bool counting;      // (uniform over a head) the word is a count
    static __host__ __device__ __forceinline__ uint32_t extra_bytes(uint32_t slots) { return ((slots + 127u) >> 7) * 16u; }
    __device__ __forceinline__ void init(unsigned char* lds, uint32_t slots) { this->keys = (uint32_t*)lds; this->cnt32 = nullptr; msk = this->keys + slots; mk = msk + slots; mm = 0xFFFFFFFFu; counting = false; }
    __device__ __forceinline__ void set_member(uint32_t m, bool c) { mm = m; counting = c; }
    __device__ __forceinline__ void clear(uint32_t slots, uint32_t t, uint32_t nt) const {
        const cf_u32x4 e{kEmpty, kEmpty, kEmpty, kEmpty}, z{0u, 0u, 0u, 0u};
        for (uint32_t s = t; s < (slots >> 2); s += nt) { ((cf_u32x4*)this->keys)[s] = e; ((cf_u32x4*)msk)[s] = z; }
        for (uint32_t s = t; s < ((slots + 127u) >> 7); s += nt) ((cf_u32x4*)mk)[s] = z;
    }
    struct masks { uint32_t w[4]; };
    __device__ __forceinline__ masks read_masks(uint32_t bk) const { const cf_u32x4 v = *(const cf_u32x4*)&msk[4 * bk]; masks m; m.w[0] = v.x; m.w[1] = v.y; m.w[2] = v.z; m.w[3] = v.w; return m; }
    __device__ __forceinline__ uint32_t cnt_of(uint32_t w) const { return counting ? w : (uint32_t)__popc(w & mm); }      // the member's count
    __device__ __forceinline__ uint32_t all_of(uint32_t w) const { return counting ? w : (uint32_t)__popc(w); }          // the union's
    // one more occurrence, brought by posting `bit` of the union: the count of the union after it — or all ones when the posting was there already
    // (it then moved nothing: no count is "reached")
    __device__ __forceinline__ uint32_t add(uint32_t bk, int i, uint32_t bit) const {
        const uint32_t s = 4u * bk + (uint32_t)i;
        if (counting) return atomicAdd(&msk[s], 1u) + 1u;
        const uint32_t was = atomicOr(&msk[s], 1u << bit);
        return ((was >> bit) & 1u) ? 0xFFFFFFFFu : (uint32_t)__popc(was) + 1u;
    }
    __device__ __forceinline__ int claim_finish(uint32_t old, uint32_t bk, int i, uint32_t b, uint32_t dd, uint32_t& cnt, uint32_t bit) const {
        cnt = 0xFFFFFFFFu;
        if (old != kEmpty && old != N::key_of(b, dd)) return 2;
        cnt = add(bk, i, bit);      // (a fresh slot's mask is empty: the claim does not count by itself)
        return old == kEmpty ? 0 : 1;
    }
    // cf_probe2 with masks: two queued inserts per lane side by side, ONE probe of the home bucket each in straight-line code
    __device__ __forceinline__ void probe2m(bool act0, uint32_t bk0, uint32_t key0, uint32_t bit0, bool act1, uint32_t bk1, uint32_t key1, uint32_t bit1, uint32_t min_cov,
                                            bool& made0, bool& park0, uint32_t& hot0, bool& made1, bool& park1, uint32_t& hot1) const {
        const bucket k0 = this->read(bk0), k1 = this->read(bk1);
        uint32_t em0 = 4u, em1 = 4u;
#pragma unroll
        for (int j = 3; j >= 0; --j) { em0 = k0.k[j] == kEmpty ? (uint32_t)j : em0; em1 = k1.k[j] == kEmpty ? (uint32_t)j : em1; }
        uint32_t sl0 = em0, sl1 = em1;
        bool mt0 = false, mt1 = false;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            const bool e0 = k0.k[j] == key0, e1 = k1.k[j] == key1;
            sl0 = e0 ? (uint32_t)j : sl0; mt0 |= e0; sl1 = e1 ? (uint32_t)j : sl1; mt1 |= e1;
        }
        mt0 &= act0; mt1 &= act1;
        const bool claim0 = act0 && !mt0 && em0 < 4u, claim1 = act1 && !mt1 && em1 < 4u;
        const uint32_t s0 = 4u * bk0 + (sl0 & 3u), s1 = 4u * bk1 + (sl1 & 3u);
        uint32_t old0 = key0, old1 = key1;
        if (claim0) old0 = atomicCAS(&this->keys[s0], kEmpty, key0);
        if (claim1) old1 = atomicCAS(&this->keys[s1], kEmpty, key1);
        const bool fresh0 = claim0 && old0 == kEmpty, fresh1 = claim1 && old1 == kEmpty;
        const bool in0 = mt0 || (claim0 && old0 == key0) || fresh0, in1 = mt1 || (claim1 && old1 == key1) || fresh1;
        uint32_t now0, now1;
        bool new0 = in0, new1 = in1;
        if (counting) {
            now0 = atomicAdd(&msk[s0], in0 ? 1u : 0u) + 1u;
            now1 = atomicAdd(&msk[s1], in1 ? 1u : 0u) + 1u;
        } else {
            const uint32_t was0 = atomicOr(&msk[s0], in0 ? 1u << bit0 : 0u);
            const uint32_t was1 = atomicOr(&msk[s1], in1 ? 1u << bit1 : 0u);
            new0 = in0 && !((was0 >> bit0) & 1u); new1 = in1 && !((was1 >> bit1) & 1u);
            now0 = (uint32_t)__popc(was0) + 1u; now1 = (uint32_t)__popc(was1) + 1u;
        }
        made0 = fresh0; park0 = act0 && !in0; hot0 = (new0 && now0 == min_cov) ? s0 : 0xFFFFFFFFu;
        made1 = fresh1; park1 = act1 && !in1; hot1 = (new1 && now1 == min_cov) ? s1 : 0xFFFFFFFFu;
    }
    __device__ __forceinline__ bool get(uint32_t s, uint32_t& b, uint32_t& dd, uint32_t& cnt) const {
        const uint32_t q = this->keys[s];
        b = q & kBMask; dd = q >> kBBits; cnt = cnt_of(msk[s]);
        return q != kEmpty;
    }
    __device__ __forceinline__ uint32_t sum_of(const bucket& k, const masks& m, uint32_t b) const {
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((k.k[j] & kBMask) == b && k.k[j] != kEmpty) total += cnt_of(m.w[j]);
        return total;
    }
    __device__ __forceinline__ unsigned long long total_of(uint32_t b, uint32_t n_buckets) const {
        unsigned long long total = 0;
        uint32_t bk = N::home(N::hash(b), n_buckets);
        for (uint32_t probe = 0; probe < n_buckets; ++probe) {
            const bucket k = this->read(bk);
            total += sum_of(k, read_masks(bk), b);
            if (k.k[3] == kEmpty) break;
            bk = bk + 1 == n_buckets ? 0u : bk + 1;
        }
        return total;
    }
    // (a slot whose MEMBER count stays below min_cov is dropped before the chain walk)
    template <class F>
    __device__ __forceinline__ void for_counts_at_least(uint32_t bk, uint32_t n_buckets, uint32_t min_cov, F&& f) const {
        const masks m = read_masks(bk);
        if (!(m.w[0] | m.w[1] | m.w[2] | m.w[3])) return;
        const bucket k = this->read(bk);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t cnt = cnt_of(m.w[i]);
            if (cnt >= min_cov && k.k[i] != kEmpty) {
                const uint32_t b = k.k[i] & kBMask;
                const unsigned long long total = (k.k[3] == kEmpty && N::home(N::hash(b), n_buckets) == bk) ? (unsigned long long)sum_of(k, m, b) : total_of(b, n_buckets);
                f(4u * bk + (uint32_t)i, b, k.k[i] >> kBBits, cnt, total);
            }
        }
    }
    // the scan that replaces the hot list looks at the UNION's counts: one list for every member
    static constexpr uint32_t kScanGroup = 4;
    static __device__ __forceinline__ uint32_t slot_of_bit(uint32_t bit) { return bit; }
    __device__ __forceinline__ uint32_t hot_mask(uint32_t g, uint32_t min_cov) const {
        const masks m = read_masks(g);
        const uint32_t need = max(min_cov, 1u);      // (an empty slot has no bit and no count)
        return (uint32_t)(all_of(m.w[0]) >= need) | ((uint32_t)(all_of(m.w[1]) >= need) << 1) | ((uint32_t)(all_of(m.w[2]) >= need) << 2) | ((uint32_t)(all_of(m.w[3]) >= need) << 3);
    }
    template <class F>
    __device__ __forceinline__ void eval_slot(uint32_t s, uint32_t n_buckets, uint32_t min_cov, F&& f) const {
        const uint32_t bk = s >> 2, i = s & 3u;
        const bucket k = this->read(bk);
        const masks m = read_masks(bk);
        uint32_t mine = k.k[0], mine_m = m.w[0];
#pragma unroll
        for (int j = 1; j < 4; ++j) { if (i == (uint32_t)j) { mine = k.k[j]; mine_m = m.w[j]; } }
        const uint32_t cnt = cnt_of(mine_m);
        if (mine == kEmpty || cnt < min_cov) return;
        const uint32_t b = mine & kBMask;
        const unsigned long long total = (k.k[3] == kEmpty && N::home(N::hash(b), n_buckets) == bk) ? (unsigned long long)sum_of(k, m, b) : total_of(b, n_buckets);
        f(s, b, mine >> kBBits, cnt, total);
    }
#if defined(CF_DIST_DIAG_COUNT)
    // diagnostic build: does eval_slot(s) walk the chain for its total (total_of), and how many buckets does that walk read?  (0: no walk)
    __device__ __forceinline__ uint32_t diag_walk(uint32_t s, uint32_t n_buckets, uint32_t min_cov) const {
        const uint32_t bk0 = s >> 2, i = s & 3u;
        const bucket k0 = this->read(bk0);
        const uint32_t mine = k0.k[i];
        if (mine == kEmpty || cnt_of(msk[s]) < min_cov) return 0u;
        const uint32_t b = mine & kBMask;
        if (k0.k[3] == kEmpty && N::home(N::hash(b), n_buckets) == bk0) return 0u;
        uint32_t bk = N::home(N::hash(b), n_buckets), n = 0;
        for (uint32_t probe = 0; probe < n_buckets; ++probe) {
            ++n;
            if (this->read(bk).k[3] == kEmpty) break;
            bk = bk + 1 == n_buckets ? 0u : bk + 1;
        }
        return n;
    }
#endif
    template <class F>
    __device__ __forceinline__ void for_marked(uint32_t bk, F&& f) const {
        const uint32_t w = (mk[bk >> 3] >> ((bk & 7u) * 4u)) & 15u;
        if (!w) return;
        const bucket k = this->read(bk);
        const masks m = read_masks(bk);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((w >> i) & 1u) f(4u * bk + (uint32_t)i, k.k[i] & kBMask, k.k[i] >> kBBits, cnt_of(m.w[i]));
    }
    __device__ __forceinline__ void mark(uint32_t s) const { atomicOr(&mk[s >> 5], 1u << (s & 31u)); }
    __device__ __forceinline__ void unmark(uint32_t s) const { atomicAnd(&mk[s >> 5], ~(1u << (s & 31u))); }
};

// The 6-byte slots for k-mer sets of up to 2^27 - 16 k-mers whatever the reads' lengths (distances up to 255): the 32-bit key
// [d : 8 | b >> S : 24] leaves out the low S <= 3 bits of the rank, and the table is cut into 2^S REGIONS of equal size —
// a key lives in the region of its rank's low bits (home bucket, probe chain and the chain walk for the totals all stay
// inside the region), so (region, key) identifies (b, d).  Ranks are dense, so the regions fill evenly.  The cloud entries
// are read as they are (the CSR's 32-bit ranks) plus one byte per entry for the unit index mod 256; a queued insert is
// 64 bits (b, d).  Everything else — 4 keys per bucket, 16-bit count fields, the filter — is the 6-byte layout's.
struct cf_tab_region {
    static constexpr int PB = 4;
    static constexpr uint32_t kBBits = 24, kBMask = (1u << kBBits) - 1u;
    static constexpr uint32_t kSlotBytes = 6, kPerBucket = PB, kAll = (1u << PB) - 1u;
    static constexpr bool kMaskTab = false;
    static constexpr uint32_t kEmpty = 0xFFFFFFFFu;
    struct bucket { uint32_t k[PB]; };
    struct counts { uint32_t w[PB / 2]; };
    struct raw { uint32_t b, i; };
    typedef unsigned long long qitem;   // deferred insert: [b : 32 | d : 32]
    uint32_t* keys;
    uint32_t* cnt32;
    uint32_t S, nb_r;                   // log2(regions), buckets per region
    __device__ __forceinline__ void init(unsigned char* lds, uint32_t slots) { keys = (uint32_t*)lds; cnt32 = keys + slots; S = 0; nb_r = slots / PB; }
    __device__ __forceinline__ void configure(const cf_dist_args& A, uint32_t n_buckets) { S = A.reg_shift; nb_r = n_buckets >> A.reg_shift; }
    __device__ __forceinline__ void clear(uint32_t slots, uint32_t t, uint32_t nt) const {
        const cf_u32x4 e{kEmpty, kEmpty, kEmpty, kEmpty}, z{0u, 0u, 0u, 0u};
        for (uint32_t s = t; s < (slots >> 2); s += nt) ((cf_u32x4*)keys)[s] = e;
        for (uint32_t s = t; s < (slots >> 3); s += nt) ((cf_u32x4*)cnt32)[s] = z;
    }
    struct __attribute__((packed, aligned(4))) run4 { uint32_t x, y, z, w; };
    static __device__ __forceinline__ void load_run(const cf_dist_args& A, uint32_t s_e, uint32_t l4, uint32_t ok, raw (&out)[DIST_UNROLL]) {
        static_assert(DIST_UNROLL == 4, "one 16-byte and one 8-byte load per lane");
        const int32_t* pe = A.entries + s_e;
        if (ok == (1u << DIST_UNROLL) - 1u) {      // the whole run lies inside the posting's range
            const run4 r = *(const run4*)(pe + l4);
            // the 4 index bytes start at any byte address: two ALIGNED dwords around them and a funnel shift (a dword load
            // from a misaligned address takes the slow path of the memory pipeline: the sketch sweep ran 39 % longer with it);
            // the misalignment is the item's (wave-uniform)
            struct __attribute__((packed, aligned(4))) pair2 { uint32_t lo, hi; };
            const uint8_t* pb = A.entry_i8 + (s_e & ~3u);
            const pair2 w = *(const pair2*)(pb + l4);
            const uint32_t sh = (s_e & 3u) * 8u;
            const uint32_t iw = (uint32_t)((((unsigned long long)w.hi << 32) | w.lo) >> sh);
            out[0] = raw{r.x, iw & 0xFFu}; out[1] = raw{r.y, (iw >> 8) & 0xFFu}; out[2] = raw{r.z, (iw >> 16) & 0xFFu}; out[3] = raw{r.w, iw >> 24};
            return;
        }
        const uint8_t* pi = A.entry_i8 + s_e;
#pragma unroll
        for (int u = 0; u < DIST_UNROLL; ++u) { const uint32_t x = ((ok >> u) & 1u) ? l4 + (uint32_t)u : 0u; out[u] = raw{(uint32_t)pe[x], (uint32_t)pi[x]}; }
    }
    static __device__ __forceinline__ void decode(const raw& r, uint32_t ig, uint32_t, uint32_t& b, uint32_t& dd, uint32_t& qk, uint32_t& lo) { b = r.b; dd = (r.i - ig) & 0xFFu; qk = 0u; lo = r.b; }      // unit indices mod 256, d <= 255
    __device__ __forceinline__ qitem q_push(uint32_t b, uint32_t dd, uint32_t, uint32_t n_buckets) const { return q_of(b, dd, n_buckets); }
    static __device__ __forceinline__ uint32_t hash(uint32_t b) { return (b & 0xFFFFFFu) * 0x9E3779u; }      // sketch and bitmap: any function of b will do (ranks that differ above bit 23 share counters and bits)
    static __device__ __forceinline__ uint32_t bm_bit(uint32_t b) { return b & (DIST_BM_BITS - 1u); }      // (k-mer ranks: their low bits are as good as a hash of them, and cost nothing)
    static __device__ __forceinline__ uint32_t sk_hash(uint32_t b, uint32_t dd, uint32_t) { return hash(b) + dd * 0x5BD1E9u; }      // the sketch's counter of the pair (b, d): its high bits
    __device__ __forceinline__ uint32_t key_of(uint32_t b, uint32_t dd) const { return (dd << kBBits) | (b >> S); }
    __device__ __forceinline__ uint32_t region_base(uint32_t b) const { return (b & ((1u << S) - 1u)) * nb_r; }
    __device__ __forceinline__ uint32_t home_of(uint32_t b) const { return region_base(b) + (((((b >> S) * 0x9E3779u) >> 16) * (nb_r & 0xFFFFu)) >> 16); }
    __device__ __forceinline__ uint32_t next(uint32_t bk, uint32_t b, uint32_t) const { const uint32_t r0 = region_base(b); return bk + 1 == r0 + nb_r ? r0 : bk + 1; }
    __device__ __forceinline__ uint32_t region_of(uint32_t bk) const {      // bk / nb_r for at most 8 regions
        uint32_t r = 0;
        for (uint32_t x = nb_r; x <= bk; x += nb_r) ++r;
        return r;
    }
    __device__ __forceinline__ uint32_t b_of(uint32_t key, uint32_t bk) const { return ((key & kBMask) << S) | region_of(bk); }
    __device__ __forceinline__ qitem q_of(uint32_t b, uint32_t dd, uint32_t) const { return ((unsigned long long)b << 32) | dd; }
    __device__ __forceinline__ void q_take(qitem q, uint32_t, uint32_t& b, uint32_t& dd, uint32_t& bk) const { b = (uint32_t)(q >> 32); dd = (uint32_t)q; bk = home_of(b); }
    __device__ __forceinline__ bucket read(uint32_t bk) const {
        bucket r;
        const cf_u32x4 v = *(const cf_u32x4*)&keys[PB * bk];
        r.k[0] = v.x; r.k[1] = v.y; r.k[2] = v.z; r.k[3] = v.w;
        return r;
    }
    __device__ __forceinline__ counts read_counts(uint32_t bk) const {
        counts c;
        const unsigned long long v = *(const unsigned long long*)&cnt32[2 * bk];
        c.w[0] = (uint32_t)v; c.w[1] = (uint32_t)(v >> 32);
        return c;
    }
    static __device__ __forceinline__ uint32_t field(const counts& c, int j) { return (c.w[j >> 1] >> ((j & 1) * 16)) & 0x7FFFu; }
    static __device__ __forceinline__ uint32_t ne_bit(uint32_t k, uint32_t q) { return min(k ^ q, 1u); }
    static __device__ __forceinline__ int first_equal(const bucket& k, uint32_t q) {
        uint32_t ne = 0;
#pragma unroll
        for (int j = 0; j < PB; ++j) ne |= ne_bit(k.k[j], q) << j;
        return __ffs((int)(ne ^ kAll)) - 1;
    }
    __device__ __forceinline__ int match(const bucket& k, uint32_t b, uint32_t dd) const { return first_equal(k, key_of(b, dd)); }
    static __device__ __forceinline__ int empty(const bucket& k) { return first_equal(k, kEmpty); }
    // counts one more occurrence of the key in slot i of bucket bk; returns its count after the add (the field holds count - 1)
    __device__ __forceinline__ uint32_t add(uint32_t bk, int i) const {
        const uint32_t s = PB * bk + (uint32_t)i, sh_ = (s & 1u) * 16u;
        return ((atomicAdd(&cnt32[s >> 1], 1u << sh_) >> sh_) & 0x7FFFu) + 2u;
    }
    static constexpr uint32_t kSlotsPerBucket = PB;
    __device__ __forceinline__ uint32_t claim_issue(uint32_t bk, int i, uint32_t b, uint32_t dd) const { return atomicCAS(&keys[PB * bk + i], kEmpty, key_of(b, dd)); }
    __device__ __forceinline__ int claim_finish(uint32_t old, uint32_t bk, int i, uint32_t b, uint32_t dd, uint32_t& cnt) const {
        cnt = 1u;
        if (old == kEmpty) return 0;
        if (old == key_of(b, dd)) { cnt = add(bk, i); return 1; }
        return 2;
    }
    static constexpr bool kDrainTwoProbes = true;      // (as cf_tab_narrow_t: two queued inserts per lane, cf_probe2)
    __device__ __forceinline__ void probe2(bool act0, uint32_t bk0, uint32_t key0, bool act1, uint32_t bk1, uint32_t key1, uint32_t min_cov,
                                           bool& made0, bool& park0, uint32_t& hot0, bool& made1, bool& park1, uint32_t& hot1) const {
        cf_probe2(*this, act0, bk0, key0, act1, bk1, key1, min_cov, made0, park0, hot0, made1, park1, hot1);
    }
    __device__ __forceinline__ bool get(uint32_t s, uint32_t& b, uint32_t& dd, uint32_t& cnt) const {
        const uint32_t q = keys[s];
        b = b_of(q, s / (uint32_t)PB); dd = q >> kBBits; cnt = ((cnt32[s >> 1] >> ((s & 1u) * 16u)) & 0x7FFFu) + 1u;
        return q != kEmpty;
    }
    // sum of the counts of the keys (b, .) among the keys of a bucket of b's region
    __device__ __forceinline__ uint32_t sum_of(const bucket& k, const counts& c, uint32_t b) const {
        const uint32_t bq = b >> S;
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < PB; ++j)
            if ((k.k[j] & kBMask) == bq && k.k[j] != kEmpty) total += field(c, j) + 1u;
        return total;
    }
    __device__ __forceinline__ unsigned long long total_of(uint32_t b, uint32_t n_buckets) const {
        unsigned long long total = 0;
        uint32_t bk = home_of(b);
        for (uint32_t probe = 0; probe < nb_r; ++probe) {
            const bucket k = read(bk);
            total += sum_of(k, read_counts(bk), b);
            if (k.k[PB - 1] == kEmpty) break;
            bk = next(bk, b, n_buckets);
        }
        return total;
    }
    template <class F>
    __device__ __forceinline__ void for_counts_at_least(uint32_t bk, uint32_t n_buckets, uint32_t min_cov, F&& f) const {
        const counts c = read_counts(bk);
        const uint32_t need = min_cov ? min_cov - 1u : 0u;
        bool any = false;
#pragma unroll
        for (int j = 0; j < PB; ++j) any |= field(c, j) >= need;
        if (!any) return;
        const bucket k = read(bk);
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const uint32_t cnt = field(c, i) + 1u;
            if (cnt >= min_cov && k.k[i] != kEmpty) {
                const uint32_t b = b_of(k.k[i], bk);
                const unsigned long long total = (k.k[PB - 1] == kEmpty && home_of(b) == bk) ? (unsigned long long)sum_of(k, c, b) : total_of(b, n_buckets);
                f((uint32_t)PB * bk + (uint32_t)i, b, k.k[i] >> kBBits, cnt, total);
            }
        }
    }
    static constexpr uint32_t kScanGroup = 8;
    // two 16-bit fields per word compared at once: (field & 0x7FFF) + (0x8000 - need) has bit 15 set iff the field reaches need
    // (no carry leaves a half: both terms are <= 0x8000).  Bit 2j of the result = slot 2j of the group, bit 16 + 2j = slot 2j + 1.
    __device__ __forceinline__ uint32_t hot_mask(uint32_t g, uint32_t min_cov) const {
        const cf_u32x4 v = *(const cf_u32x4*)&cnt32[4 * g];
        const uint32_t need = min(min_cov ? min_cov - 1u : 0u, 0x8000u);
        const uint32_t add = 0x80008000u - need * 0x00010001u;
        const uint32_t y0 = ((v.x & 0x7FFF7FFFu) + add) & 0x80008000u, y1 = ((v.y & 0x7FFF7FFFu) + add) & 0x80008000u;
        const uint32_t y2 = ((v.z & 0x7FFF7FFFu) + add) & 0x80008000u, y3 = ((v.w & 0x7FFF7FFFu) + add) & 0x80008000u;
        return (y0 >> 15) | (y1 >> 13) | (y2 >> 11) | (y3 >> 9);
    }
    static __device__ __forceinline__ uint32_t slot_of_bit(uint32_t bit) { return (bit & 15u) + (bit >> 4); }
    template <class F>
    __device__ __forceinline__ void eval_slot(uint32_t s, uint32_t n_buckets, uint32_t min_cov, F&& f) const {
        const uint32_t bk = s / (uint32_t)PB, i = s % (uint32_t)PB;
        const bucket k = read(bk);
        const counts c = read_counts(bk);
        uint32_t mine = k.k[0], mine_f = field(c, 0);
#pragma unroll
        for (int j = 1; j < PB; ++j) { if (i == (uint32_t)j) { mine = k.k[j]; mine_f = field(c, j); } }
        const uint32_t cnt = mine_f + 1u;
        if (mine == kEmpty || cnt < min_cov) return;
        const uint32_t b = b_of(mine, bk);
        const unsigned long long total = (k.k[PB - 1] == kEmpty && home_of(b) == bk) ? (unsigned long long)sum_of(k, c, b) : total_of(b, n_buckets);
        f(s, b, mine >> kBBits, cnt, total);
    }
    template <class F>
    __device__ __forceinline__ void for_marked(uint32_t bk, F&& f) const {
        const counts c = read_counts(bk);
        if (!((c.w[0] | c.w[1]) & 0x80008000u)) return;
        const bucket k = read(bk);
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            const uint32_t h = c.w[i >> 1] >> ((i & 1) * 16);
            if (h & 0x8000u) f((uint32_t)PB * bk + (uint32_t)i, b_of(k.k[i], bk), k.k[i] >> kBBits, (h & 0x7FFFu) + 1u);
        }
    }
    __device__ __forceinline__ void mark(uint32_t s) const { atomicOr(&cnt32[s >> 1], 0x8000u << ((s & 1u) * 16u)); }
    __device__ __forceinline__ void unmark(uint32_t s) const { atomicAnd(&cnt32[s >> 1], ~(0x8000u << ((s & 1u) * 16u))); }
};

// The region layout's table behind a FOUR-byte stream, for k-mer sets of 2^24 .. 2^26 ranks whose reads have at most 128 units
// (8 x 50 000 reads sharded over 8 GPUs sweep a union of 3.7e7 k-mers: tools/rank_emulation.py).  26 bits of rank leave 6 for
// the unit index — one bit short of the 7 that distances up to 127 need, which is why round 3 streamed rank and index apart
// (a 16-byte and an 8-byte load per lane and step, a funnel shift, 64-bit queue items: 450 ms against 320 at 50 000 reads).
// The partner entries of a posting are sorted by unit, so inside an item of 256 entries "d >= 64" begins at ONE position,
// t64, that the item record carries next to the posting's unit index ([entries : 16 | t64 : 9 | unit index : 7]):
// d = ((i - ig) mod 64) + 64 * [position >= t64].  Table, keys, regions, filter: cf_tab_region's.
struct cf_tab_region26 : cf_tab_region {
    struct raw { uint32_t v; };
    struct __attribute__((packed, aligned(4))) run4 { uint32_t x, y, z, w; };
    static __device__ __forceinline__ void load_run(const cf_dist_args& A, uint32_t s_e, uint32_t l4, uint32_t, raw (&out)[DIST_UNROLL]) {
        static_assert(DIST_UNROLL == 4, "one 16-byte load per lane");
        cf_load_packed4(A, s_e, l4, out[0].v, out[1].v, out[2].v, out[3].v);
    }
    static __device__ __forceinline__ void decode(const raw& r, uint32_t igf, uint32_t pos, uint32_t& b, uint32_t& dd, uint32_t& qk, uint32_t& lo) {
        qk = 0u; lo = r.v;
        b = r.v & 0x3FFFFFFu;
        dd = (((r.v >> 26) - igf) & 63u) + (pos >= (igf >> 7) ? 64u : 0u);      // (igf = t64 << 7 | unit index mod 128: its low 6 bits are all the subtraction keeps)
    }
};
