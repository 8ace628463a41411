// cf_dist.hip — A5 (k-mer pair / unit-distance histogram) fused with A6 (edge filter).
//
// Reference: scripts/distance_based_kmer_recruitment.py:85-128 counts, for every read, every
// pair of unit clouds d units apart (min_d <= d <= max_d) and every ordered pair (a in C_i,
// b in C_{i+d}, a != b), cnt[d][a][b] += 1; :131-149 keeps (d, a, b, cnt) with cnt >= min_cov
// and cnt / sum_d' cnt[d'][a][b] >= 0.8 (true division), and marks a and b as selected.
//
// Device design (the dominant kernel of the path; HBM/L2 streaming + LDS atomics, no MFMA):
//   * dist_cnt[d][a] is owned by the first k-mer a in the reference; so is it here: one workgroup owns one a at a time
//     (ticket queues in the locality order of the first k-mers).  Before the launch two builder kernels cut a's partner
//     entries — for every posting (a unit holding a) the clouds of the later units of that read, ONE contiguous CSR range —
//     into item records of <= 256 entries in HBM; a wave reads its records with one load and both sweeps run on them.
//   * sweep 1 only COUNTS every (b, d) pair in 4-bit counters (8-bit ones for min_cov > 9, or when a 4-bit one wrapped) laid over the
//     table's LDS (most pairs never reach min_cov) and marks hash(b) of the pairs that can; sweep 2 queues the pairs of marked b and inserts them, 64 at a time, into an exact
//     open-addressed LDS table (6-byte slots [d | b] + 15-bit count in 4-key buckets; 8-byte slots / region layouts for
//     large k-mer sets).  The slot hash depends on b only, so all d of one b share a probe chain and sum_d cnt is a chain walk:
//     both filters run in LDS, and the lane that evaluates a selected slot writes the edge row itself, into a chunk of the
//     output the workgroup reserved earlier.
//   * a table that would overflow is split by a second hash of b into 2, 4, ... partitions, each processed (re-streamed)
//     on its own: exact, no HBM spill.
//   * first k-mers partition across GPUs (a % n_parts == part) with no reduction.
#include "cf_common.h"
#include "cf_dist_tab.h"

#include <cstdlib>

void cf_free_edges(cf_ctx* c);
int cf_refresh_unique_count(cf_ctx* ctx);  // cf_clouds.hip

#ifndef cf_ballot
// the mask of a condition straight from the compare that made it (HIP's __ballot takes an int: the condition goes through a 0 / 1 vector
// register and a second compare)
__device__ __forceinline__ unsigned long long cf_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
#endif

__global__ void __launch_bounds__(256)
cf_post_hist_kernel(const int32_t* __restrict__ entries, int64_t e0, int64_t e1, uint32_t part, uint32_t n_parts, uint32_t* __restrict__ cnt) {
    // postings are only needed for the first k-mers of this partition (a % n_parts == part): at N GPUs every rank
    // scans all clouds but keeps 1/N of the postings
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = e0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < e1; i += stride) {
        const uint32_t x = (uint32_t)entries[i];
        if (n_parts == 1u || x % n_parts == part) atomicAdd(&cnt[x], 1u);
    }
}

__global__ void __launch_bounds__(256)
cf_post_fill_kernel(const int64_t* __restrict__ cloud_ptr, const int32_t* __restrict__ entries, int64_t u0, int64_t u1, uint32_t part, uint32_t n_parts,
                    const int64_t* __restrict__ post_ptr, uint32_t* __restrict__ cursor, int32_t* __restrict__ post,
                    uint32_t* __restrict__ first_unit) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t u = u0 + wave; u < u1; u += n_waves) {
        const int64_t a = cloud_ptr[u], b = cloud_ptr[u + 1];
        for (int64_t e = a + lane; e < b; e += 64) {
            const int32_t x = entries[e];
            if (n_parts != 1u && (uint32_t)x % n_parts != part) continue;
            post[post_ptr[x] + atomicAdd(&cursor[x], 1u)] = (int32_t)u;
            if (first_unit[x] > (uint32_t)u) atomicMin(&first_unit[x], (uint32_t)u);
        }
    }
}

// Postings by SORT (one GPU, every first k-mer: n_parts == 1).  The postings are the transpose of the cloud CSR; round 2 built them
// with one device-scope returning atomic per cloud entry (a histogram pass and a fill pass: 12 ms, 40 GB of traffic for 0.45 GB of
// output).  Here every cloud entry becomes one record [unit : high | rank : low kb bits], the records are radix-sorted on the
// rank bits (stable: the units of a k-mer stay in ascending order), and the run boundaries give the counts and the first unit.
__global__ void __launch_bounds__(256)
cf_post_recs_kernel(const int64_t* __restrict__ cloud_ptr, const int32_t* __restrict__ entries, int64_t u0, int64_t u1, int64_t e0, int kb,
                    unsigned long long* __restrict__ recs) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t u = u0 + wave; u < u1; u += n_waves) {
        const int64_t a = cloud_ptr[u], b = cloud_ptr[u + 1];
        for (int64_t e = a + lane; e < b; e += 64) recs[e - e0] = ((unsigned long long)u << kb) | (unsigned long long)(uint32_t)entries[e];
    }
}
// The same for ONE partition of the first k-mers (n_parts > 1: a rank of a multi-GPU run scans all clouds and keeps the entries
// x % n_parts == part, 1 / n_parts of them).  The survivors are compacted in cloud order — per unit a count, a scan, then the fill; one
// wave per unit, ballots inside — so that the stable sort leaves the units of a k-mer ascending, and the sort key is x / n_parts:
// fewer bits, often one radix pass fewer.  (Before: one returning device-scope atomic per kept entry in a histogram pass and again
// in a fill pass, 26 ms per step for a rank of 8 against 19 ms for the whole single-GPU job.)
__global__ void __launch_bounds__(256)
cf_post_ucount_kernel(const int64_t* __restrict__ cloud_ptr, const int32_t* __restrict__ entries, int64_t u0, int64_t u1, uint32_t part, uint32_t n_parts,
                      uint32_t* __restrict__ ucnt) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t u = u0 + wave; u < u1; u += n_waves) {
        const int64_t a = cloud_ptr[u], b = cloud_ptr[u + 1];
        uint32_t c = 0;
        for (int64_t e = a + lane; e < b; e += 64) c += (uint32_t)((uint32_t)entries[e] % n_parts == part);
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, (unsigned)d);
        if (lane == 0) ucnt[u - u0] = c;
    }
}
__global__ void __launch_bounds__(256)
cf_post_recs_part_kernel(const int64_t* __restrict__ cloud_ptr, const int32_t* __restrict__ entries, int64_t u0, int64_t u1, uint32_t part, uint32_t n_parts,
                         const int64_t* __restrict__ uoff, int kb, unsigned long long* __restrict__ recs) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t u = u0 + wave; u < u1; u += n_waves) {
        const int64_t a = cloud_ptr[u], b = cloud_ptr[u + 1];
        int64_t o = uoff[u - u0];
        for (int64_t e0 = a; e0 < b; e0 += 64) {      // (uniform trip count: a ballot inside)
            const int64_t e = e0 + lane;
            const uint32_t x = e < b ? (uint32_t)entries[e] : 0u;
            const bool keep = e < b && x % n_parts == part;
            const unsigned long long m = cf_ballot(keep);
            if (keep) recs[o + __popcll(m & ((1ull << lane) - 1ull))] = ((unsigned long long)u << kb) | (unsigned long long)(x / n_parts);
            o += __popcll(m);
        }
    }
}
// sorted records -> post[] (the units), run starts (rs[x]) / ends (re[x]) of every rank x that occurs, and its first unit
__global__ void __launch_bounds__(256)
cf_post_bounds_kernel(const unsigned long long* __restrict__ recs, int64_t n, int kb, uint32_t part, uint32_t n_parts, int32_t* __restrict__ post,
                      uint32_t* __restrict__ rs, uint32_t* __restrict__ re, uint32_t* __restrict__ first_unit) {
    // (the sort key is the rank itself, or — one partition — rank / n_parts: rank = key * n_parts + part)
    const unsigned long long mask = (1ull << kb) - 1ull;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const unsigned long long r = recs[i];
        const uint32_t j = (uint32_t)(r & mask), u = (uint32_t)(r >> kb), x = j * n_parts + part;
        post[i] = (int32_t)u;
        if (i == 0 || (uint32_t)(recs[i - 1] & mask) != j) { rs[x] = (uint32_t)i; first_unit[x] = u; }
        if (i == n - 1 || (uint32_t)(recs[i + 1] & mask) != j) re[x] = (uint32_t)(i + 1);
    }
}
__global__ void __launch_bounds__(256)
cf_post_counts_kernel(const uint32_t* __restrict__ rs, uint32_t* __restrict__ re_to_cnt, int64_t n_kmers) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n_kmers; x += stride) re_to_cnt[x] = re_to_cnt[x] - rs[x];      // (both 0 for a rank that does not occur)
}

__global__ void __launch_bounds__(256)
cf_unit_rend_kernel(const int64_t* __restrict__ unit_ptr, const int64_t* __restrict__ cloud_ptr, int64_t n_reads, int32_t min_d, int32_t max_d,
                    int32_t* __restrict__ rend, int32_t* __restrict__ rbeg, cf_dist_rec* __restrict__ urange) {
    // per unit: its read's unit range and, precomputed once per launch, the partner range a posting at this unit has
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const int64_t a = unit_ptr[r], b = unit_ptr[r + 1];
        for (int64_t u = a; u < b; ++u) {
            rend[u] = (int32_t)b; rbeg[u] = (int32_t)a;
            const int64_t jlo = u + min_d, jhi = min(b - 1, u + (int64_t)max_d);
            cf_dist_rec x{0u, 0u, (uint32_t)(u - a), 0u};
            if (jhi >= jlo) { const int64_t c0 = cloud_ptr[jlo]; x.e0 = (uint32_t)c0; x.len = (uint32_t)(cloud_ptr[jhi + 1] - c0); x.nu = (uint32_t)(jhi - jlo + 1); }
            urange[u] = x;
        }
    }
}

// per cloud entry the index of its unit inside its read (one wave per unit): as a 16-bit side array (wide table
// layout) or, mod 2^(32 - b_bits), packed above the rank (narrow layouts: one 4-byte load per pair emission)
__global__ void __launch_bounds__(256)
cf_entry_unit_kernel(const int64_t* __restrict__ cloud_ptr, const int32_t* __restrict__ rbeg, const int32_t* __restrict__ entries, int64_t n_units,
                     uint16_t* __restrict__ entry_i, uint32_t* __restrict__ packed, int b_bits, uint8_t* __restrict__ entry_i8,
                     unsigned long long* __restrict__ not_a_set) {
    // not_a_set: raised when a unit's row is not strictly ascending — a rank twice in one cloud (caller-made clouds, cf_set_clouds;
    // cf_build_clouds makes sets).  cf_items_fill_kernel reads it: the bound behind the tail items of the sketch sweep needs sets.
    const int lane = threadIdx.x & 63;
    bool bad = false;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t u = wave; u < n_units; u += n_waves) {
        const uint32_t i = (uint32_t)(u - rbeg[u]);
        const int64_t c0 = cloud_ptr[u], c1 = cloud_ptr[u + 1];
        for (int64_t e = c0 + lane; e < c1; e += 64) {
            const int32_t x = entries[e];
            if (e > c0) bad = bad || entries[e - 1] >= x;      // (the neighbour's word: the same cache line but for one lane in 32)
            if (packed) packed[e] = (i << b_bits) | (uint32_t)x;      // (the shift drops all but the low 32 - b_bits bits of i)
            else if (entry_i8) entry_i8[e] = (uint8_t)i;
            else entry_i[e] = (uint16_t)i;
        }
    }
    if (bad) *not_a_set = 1ull;      // (plain stores of the one value; read by a later kernel of the stream)
}

// keys (first posting unit << 32 | a) of the first k-mers of this partition that have postings
// A wave takes spans of 64 x 16 consecutive k-mers: it counts what it keeps of a span, reserves the output with ONE atomic and then
// writes (the keys are sorted afterwards: their order here is free).  An atomic per 64 k-mers on the one counter was 6.9 ms of an
// emulated rank's 23 ms of set-up (3.7e7 k-mers: 570 000 adds to one address, one after the other).
__global__ void __launch_bounds__(256)
cf_order_keys_kernel(const uint32_t* __restrict__ pcnt, const uint32_t* __restrict__ first_unit, int64_t n_kmers, int part, int n_parts, int ab,
                     unsigned long long* __restrict__ keys, unsigned long long* __restrict__ n_out,
                     int hb, const int64_t* __restrict__ post_ptr, const int32_t* __restrict__ post, const unsigned long long* __restrict__ not_a_set, int by_second) {
    // by_second (groups): the hb bits are the low bits of the k-mer's SECOND posting unit instead of a hash of the list — the k-mers of
    // one first unit whose lists go on alike stand together, and the greedy cut of cf_group_walk_kernel finds small unions (in hash order the
    // unions of the bench's reads sweep 0.70 of the classes' entries, in this order 0.44: tools/dist_groups_cpu.py --order)
    // hb > 0 (classes of first k-mers): hb bits of a hash of the k-mer's posting list stand between the first unit and the
    // rank, so that the sort puts k-mers with equal lists next to each other (they share their first unit).  The hash only brings candidates
    // together: cf_class_mark_kernel compares the lists.  Clouds that are not sets (cf_set_clouds) form no classes: the hash bits stay 0.
    const bool hashed = hb > 0 && *not_a_set == 0ull;
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    constexpr int kRounds = 16;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t s0 = wave * (64 * kRounds); s0 < n_kmers; s0 += n_waves * (64 * kRounds)) {      // (wave-uniform: ballots inside)
        uint32_t takes = 0, total = 0;      // bit r: this lane keeps its k-mer of round r
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int64_t a = s0 + (int64_t)r * 64 + lane;
            const bool take = a < n_kmers && (a % n_parts) == part && pcnt[a] > 0;
            takes |= (uint32_t)take << r;
            total += (uint32_t)__popcll(cf_ballot(take));
        }
        if (total == 0u) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(n_out, (unsigned long long)total);
        base = __shfl(base, 0);
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const bool take = (takes >> r) & 1u;
            const unsigned long long m = cf_ballot(take);
            if (take) {
                const int64_t a = s0 + (int64_t)r * 64 + lane;
                unsigned long long h = 0;
                if (hashed) {
                    const int64_t p0 = post_ptr[a], p1 = post_ptr[a + 1];
                    if (by_second) h = (unsigned long long)(uint32_t)post[p1 - p0 > 1 ? p0 + 1 : p0] & ((1ull << hb) - 1ull);
                    else {
                    h = (unsigned long long)(p1 - p0);
                    for (int64_t p = p0; p < p1; ++p) { h = (h ^ (unsigned long long)(uint32_t)post[p]) * 0x9E3779B97F4A7C15ull; h ^= h >> 29; }
                    h = (h * 0xBF58476D1CE4E5B9ull) >> (64 - hb);
                    }
                }
                keys[base + (unsigned long long)__popcll(m & lt)] = ((unsigned long long)first_unit[a] << (ab + hb)) | (h << ab) | (unsigned long long)a;
            }
            base += (unsigned long long)__popcll(m);
        }
    }
}
__global__ void __launch_bounds__(256)
cf_order_extract_kernel(const unsigned long long* __restrict__ keys, int64_t n, int ab, int32_t* __restrict__ order) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) order[i] = (int32_t)(keys[i] & ((1ull << ab) - 1ull));
}

// Classes of first k-mers.  cnt(a, b, d) depends on the first k-mer a only through its posting list, so the k-mers of the
// launch with EQUAL lists share one sweep of cf_dist_kernel.  The sorted order keys [first unit | hash of the list | a] put candidates
// next to each other; position i continues the class of i - 1 only when the two keys agree above the rank AND the two lists are equal in
// length and in every unit (a hash collision may lose a merge — the sort may put a stranger between two equal lists — and never makes one).
// The thread of a position that does not continue (the head of a run) walks its run and flags the start of every class: the head, and
// every DIST_CLASS_CAP-th position after it (a longer run simply starts a new class).  flags[] is zeroed before the launch.
#define DIST_CLASS_CAP 255u
__device__ __forceinline__ bool cf_same_postings(const int64_t* __restrict__ post_ptr, const int32_t* __restrict__ post, uint32_t x, uint32_t y) {
    const int64_t x0 = post_ptr[x], x1 = post_ptr[x + 1], y0 = post_ptr[y], y1 = post_ptr[y + 1];
    if (x1 - x0 != y1 - y0) return false;
    for (int64_t i = 0; i < x1 - x0; ++i) if (post[x0 + i] != post[y0 + i]) return false;
    return true;
}
__global__ void __launch_bounds__(256)
cf_class_mark_kernel(const unsigned long long* __restrict__ keys, int64_t n, int ab, const int64_t* __restrict__ post_ptr, const int32_t* __restrict__ post,
                     const unsigned long long* __restrict__ not_a_set, uint32_t* __restrict__ flags) {
    const unsigned long long rank_mask = (1ull << ab) - 1ull;
    const bool off = *not_a_set != 0ull;      // clouds that are not sets (read on the device, as cf_items_fill_kernel does): every k-mer its own class
    auto continues = [&](int64_t i) -> bool {      // position i (>= 1) has the posting list of position i - 1
        const unsigned long long k0 = keys[i - 1], k1 = keys[i];
        return (k0 >> ab) == (k1 >> ab) && cf_same_postings(post_ptr, post, (uint32_t)(k0 & rank_mask), (uint32_t)(k1 & rank_mask));
    };
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (off) { flags[i] = 1u; continue; }
        if (i > 0 && continues(i)) continue;
        flags[i] = 1u;
        uint32_t run = 1;
        for (int64_t j = i + 1; j < n && continues(j); ++j) {
            if (run == DIST_CLASS_CAP) { flags[j] = 1u; run = 0; }
            ++run;
        }
    }
}
// class c starts at position cfirst[c] of the order list; cfirst[n_classes] = n (cidx: the exclusive scan of flags)
__global__ void __launch_bounds__(256)
cf_class_first_kernel(const uint32_t* __restrict__ flags, const int64_t* __restrict__ cidx, int64_t n, int64_t n_classes, uint32_t* __restrict__ cfirst) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (flags[i]) cfirst[cidx[i]] = (uint32_t)i;
        if (i == 0) cfirst[n_classes] = (uint32_t)n;
    }
}

// Groups of first k-mers.  The first k-mers of a launch that share their FIRST posting unit come from one place of the array:
// their lists are subsets of one column of read units.  A group is a run of such k-mers, next to each other in the sorted order keys, whose
// lists have a UNION of at most `cap` (<= 32) postings; cf_dist_kernel sweeps the union once into a table of 32-bit masks (cf_tab_mask) and
// every member reads its own counts out of it through the mask of its postings among the union's.  Equal lists are equal masks: a group
// holds what a class held.  The thread at the head of a run of equal first units walks the run and cuts it greedily: a group is closed when
// the next list would bring the union above cap or the members to DIST_CLASS_CAP.  A first k-mer with more than cap postings is a group
// of its own, and when a cloud row is not a set every first k-mer is: such a group COUNTS in its table (an `or` would lose the second
// occurrence of a pair under one posting).  flags[] is zeroed before the launch; the scan that numbered the classes numbers the groups.
#define DIST_GROUP_MAX 32u
// One WAVE walks a run of equal first units (the runs that start among its 64 positions; a thread per run with the union in a private array
// took 100 ms at 50 000 reads: every step of its merges was a round trip to scratch memory).  The union lives in the lanes — lane i holds
// its i-th posting, in the order they joined — and a member's list in the lanes too.  Per position of the sorted keys the kernel writes the
// start flag, the member's mask over its group's union, and which of its own postings were NEW to the union (cf_group_fill_kernel strings
// those together: the union's order is the order of joining, not ascending — the place of a posting in the union only names its bit).
// the lists of a WINDOW of 64 positions are fetched together (lane l walks the list of position wb + l, every load of the
// window in flight at once) and parked in the wave's LDS rows; the greedy cut, sequential by definition, then costs a member one LDS read
// (issued one member ahead) and a broadcast per posting of its list — no trip to memory.  The wave that owns a window (the chunk's own
// wave: every position belongs to exactly one) also sums, on the lists it has just fetched, what cf_dist_edges reports as n_emissions: every
// first k-mer's OWN partner entries and its self pairs (postings (u, v) of one k-mer in one read with min_d <= v - u <= max_d: entries that are
// the first k-mer itself) — with groups a pass sweeps the union's entries, and n_emissions stays what it was.  The lists are ascending
// (postings by sort), so the postings of one read stand next to each other: a lane looks for pairs only where two neighbours share a read.
__device__ __forceinline__ unsigned long long cf_readlane64(unsigned long long v, int l) {
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32) | (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
}
#define DIST_WALK_ROW 33u      // words of a position's LDS row: DIST_GROUP_MAX postings and one of padding (lane l writes row l: 33 l + k takes every bank once)
#define DIST_WALK_LDS(block) ((size_t)((block) / 64) * 64 * DIST_WALK_ROW * 4)
// DESIGN.md 36 (knob dist_walk, kTab): the union of the group that is open lives in a hash table of the wave's LDS, unit -> bit: 64 slots of
// 8 bytes (bit << 32 | unit; at most 32 are in use), home slot cf_walk_home(unit), linear probing that wraps.  A member's lanes probe for
// their postings TOGETHER — one LDS round trip for the list where the lanes' copy of the union took a broadcast, a compare and a ballot
// per posting — and the new postings are put in by their own lanes, numbered by their rank among the new ones (the order the __ffs loop
// gives them).  The bits of the hits go into the member's word of o_or[] with an LDS `or` that nobody waits for: the mask is read when the
// wave leaves the window.  The launch is what it was.  !kTab is the kernel as it was (the union in the lanes).
#define DIST_WALK_TAB 64u      // slots of the union's table (a power of two, at least 2 x DIST_GROUP_MAX: a probe always meets an empty slot)
#define DIST_WALK_WAVE_TAB (64u * DIST_WALK_ROW + DIST_WALK_TAB * 2u + 64u)      // words of a wave with the table: rows, table, o_or[]
#define DIST_WALK_LDS_TAB(block) ((size_t)((block) / 64) * DIST_WALK_WAVE_TAB * 4)
#define DIST_WALK_EMPTY 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ uint32_t cf_walk_home(uint32_t unit) { return (unit * 0x9E3779B1u) >> 26; }      // (tests/walkcheck.py restates it)
#if defined(CF_WALK_STAMPS)
// Diagnostic build only (-DCF_WALK_STAMPS, tools/walk_stamps.py): shader-clock sums per wave, added to dg[] once per wave: [0] cycles inside
// the member loops (without the windows loaded there) [1] inside load_window [2] the waves' lifetimes [3] members walked [4] postings
// tested against a union [5] waves; per workgroup b: [8 + 2 b] max of ~start, [9 + 2 b] max of end (its lifetime: the slowest wave's)
#define WALK_CLOCK() ((unsigned long long)__builtin_amdgcn_s_memtime())
#define WALK_STAMP(...) __VA_ARGS__
#else
#define WALK_STAMP(...)
#endif
template <bool kTab>
__global__ void __launch_bounds__(256)
cf_group_walk_kernel(const unsigned long long* __restrict__ keys, int64_t n, int kb, int ab, const int64_t* __restrict__ post_ptr, const int32_t* __restrict__ post,
                     const unsigned long long* __restrict__ not_a_set, uint32_t cap, const cf_dist_rec* __restrict__ urange, const int32_t* __restrict__ rend, int32_t min_d, int32_t max_d,
                     uint32_t* __restrict__ flags, uint32_t* __restrict__ member_mask, uint32_t* __restrict__ new_mask,
                     unsigned long long* __restrict__ entries_out, unsigned long long* __restrict__ self_out, unsigned long long* __restrict__ dg) {
    // kb: the key's bits below the first unit (rank and order bits); ab: bits of the rank
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* const rows = (uint32_t*)cf_lds + (size_t)(threadIdx.x >> 6) * (kTab ? DIST_WALK_WAVE_TAB : 64u * DIST_WALK_ROW);      // the wave's 64 rows
    unsigned long long* const tab = (unsigned long long*)(rows + 64u * DIST_WALK_ROW);      // kTab: the union's table ...
    uint32_t* const o_or = (uint32_t*)(tab + DIST_WALK_TAB);      // ... and per position of the window the bits of the member's postings the union had
    WALK_STAMP(const unsigned long long dg_t0 = WALK_CLOCK(); unsigned long long dg_mem = 0, dg_load = 0, dg_n = 0, dg_p = 0;)
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const unsigned long long rank_mask = (1ull << ab) - 1ull;
    const bool off = *not_a_set != 0ull;
    if (cap > DIST_GROUP_MAX) cap = DIST_GROUP_MAX;
    unsigned long long ent = 0, self = 0;
    for (int64_t c0 = wave * 64; c0 < n; c0 += n_waves * 64) {      // (wave-uniform)
        // a window of 64 positions: first unit, start and length of the list (lane l: position wb + l), the lists of up to DIST_GROUP_MAX
        // postings in the LDS rows, and what the walk found for the position (written when the wave leaves the window)
        int64_t wb = c0, w_p0 = 0;
        unsigned long long w_fu = ~0ull;
        uint32_t w_len = 0, o_mask = 0, o_new = 0;
        bool o_start = false, o_done = false;
        auto flush = [&]() {
            if (kTab) {      // (the hits' bits: every `or` of the window has been issued, and the LDS takes a wave's operations in order)
                __builtin_amdgcn_wave_barrier();
                o_mask |= o_or[lane];
                o_or[lane] = 0u;
            }
            if (o_done) { const int64_t i = wb + (int64_t)lane; flags[i] = o_start ? 1u : 0u; member_mask[i] = o_mask; new_mask[i] = o_new; }
            o_done = false;
        };
        // all: every list of the window (else: the window a run goes on in — the lists of `fu` only).  own: the chunk of this wave — the emissions of its positions too.
        auto load_window = [&](int64_t b, bool all, bool own, unsigned long long fu) {
            WALK_STAMP(const unsigned long long dg_l0 = WALK_CLOCK(); struct dg_scope { unsigned long long t0, &sum; __device__ ~dg_scope() { sum += WALK_CLOCK() - t0; } } dg_s{dg_l0, dg_load};)
            flush();
            wb = b; w_fu = ~0ull; w_p0 = 0; w_len = 0;
            const int64_t i = b + (int64_t)lane;
            if (i < n) {
                const unsigned long long k = keys[i];
                w_fu = k >> kb;
                if (all || w_fu == fu) { const uint32_t x = (uint32_t)(k & rank_mask); w_p0 = post_ptr[x]; w_len = (uint32_t)(post_ptr[x + 1] - w_p0); }
            }
            const uint32_t len_l = w_len <= DIST_GROUP_MAX ? w_len : 0u;      // (a longer list is a group of its own: the walk never reads it)
            // A TEAM of 8 lanes reads one list, 8 postings to a load (a lane per list, each walking its own, fetched a cache line per lane and
            // load: 6.1 ms for the kernel, as much as the serial walk it replaced): eight rounds of eight lists, the first 8 postings of all 64 lists
            // in flight together, the rest of the longer lists behind.  A lane without a posting reads post[0] or its list's first word: in bounds.
            const uint32_t tl = lane & 7u, team = lane >> 3;
            unsigned long long adj_m = 0;      // the positions of the window with two neighbours of the list in one read
            int64_t t_p0[8];
            uint32_t t_len[8];
            int32_t t_u[8], t_r[8];
            uint32_t t_el[8], t_ig[8];
            __builtin_amdgcn_wave_barrier();      // (the rows are read by every lane: nobody is still reading the window before)
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int m = r * 8 + (int)team;
                t_p0[r] = (int64_t)__shfl((long long)w_p0, m);
                t_len[r] = __shfl(len_l, m);
                t_u[r] = post[t_p0[r] + (int64_t)(tl < t_len[r] ? tl : 0u)];
            }
            if (own) {
#pragma unroll
                for (int r = 0; r < 8; ++r) { t_el[r] = urange[t_u[r]].len; t_ig[r] = urange[t_u[r]].ig; }
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const uint32_t m = (uint32_t)r * 8u + team;
                const bool on = tl < t_len[r];
                if (on) rows[m * DIST_WALK_ROW + tl] = (uint32_t)t_u[r];
                t_r[r] = -1;
                if (own) {
                    if (on) { ent += t_el[r]; t_r[r] = t_u[r] - (int32_t)t_ig[r]; }      // first unit of the posting's read
                    const int32_t prev = __shfl_up(t_r[r], 1u, 8);
                    if (on && tl > 0u && t_r[r] == prev) adj_m |= 1ull << m;
                }
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {      // (lists of more than 8 postings: one in five on the bench's reads)
                const uint32_t m = (uint32_t)r * 8u + team;
                int32_t r_carry = own ? __shfl(t_r[r], 7, 8) : -1;
                for (uint32_t k0 = 8u; cf_ballot(k0 < t_len[r]) != 0ull; k0 += 8u) {      // (wave-uniform trip count)
                    const uint32_t k = k0 + tl;
                    const bool on = k < t_len[r];
                    const int32_t u = post[t_p0[r] + (int64_t)(on ? k : 0u)];
                    if (on) rows[m * DIST_WALK_ROW + k] = (uint32_t)u;
                    if (own) {
                        int32_t rr = -1;
                        if (on) { ent += urange[u].len; rr = u - (int32_t)urange[u].ig; }
                        int32_t prev = __shfl_up(rr, 1u, 8);
                        if (tl == 0u) prev = r_carry;
                        if (on && rr == prev) adj_m |= 1ull << m;
                        r_carry = __shfl(rr, 7, 8);
                    }
                }
            }
            bool adj = false;
            if (own && cf_ballot(adj_m != 0ull) != 0ull) {      // (rare: the bits of the teams, brought together)
                for (int d = 32; d >= 1; d >>= 1) adj_m |= (unsigned long long)__shfl_xor((long long)adj_m, d);
                adj = (adj_m >> lane) & 1ull;
            }
            __builtin_amdgcn_wave_barrier();
            if (!own) return;
            if (adj)      // (rare: the k-mer twice in one read)
                for (uint32_t p = 0; p + 1u < len_l; ++p) {
                    const int32_t up = (int32_t)rows[lane * DIST_WALK_ROW + p], re = rend[up];
                    for (uint32_t q = p + 1u; q < len_l; ++q) {
                        const int32_t v = (int32_t)rows[lane * DIST_WALK_ROW + q];
                        if (v >= re || v - up > max_d) break;
                        self += (unsigned long long)(v - up >= min_d);
                    }
                }
            // the lists that do not fit a row: the wave takes them 64 postings at a time
            unsigned long long lm = cf_ballot(w_len > DIST_GROUP_MAX);
            while (lm) {
                const int sl = __ffsll((long long)lm) - 1;
                lm &= lm - 1ull;
                const int64_t p0 = (int64_t)cf_readlane64((unsigned long long)w_p0, sl), p1 = p0 + (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)w_len, sl);
                for (int64_t p = p0 + (int64_t)lane; p < p1; p += 64) {
                    const int32_t up = post[p], re = rend[up];
                    ent += urange[up].len;
                    for (int64_t q = p + 1; q < p1; ++q) {
                        const int32_t v = post[q];
                        if (v >= re || v - up > max_d) break;
                        self += (unsigned long long)(v - up >= min_d);
                    }
                }
            }
        };
        if (kTab) o_or[lane] = 0u;      // (flush reads it, and load_window starts with one)
        load_window(c0, true, true, 0ull);
        const int64_t i_me = c0 + (int64_t)lane;
        if (off) { if (i_me < n) { flags[i_me] = 1u; member_mask[i_me] = 0u; new_mask[i_me] = 0u; } continue; }
        bool head = i_me < n;
        if (head && i_me > 0) head = (keys[i_me - 1] >> kb) != w_fu;
        unsigned long long hm = cf_ballot(head);
        while (hm) {      // the runs that start in this chunk, one after the other
            const int s = __ffsll((long long)hm) - 1;
            hm &= hm - 1ull;
            if (wb != c0) load_window(c0, true, false, 0ull);      // (a run that went on beyond the chunk is the chunk's last: not taken)
            const unsigned long long fu = cf_readlane64(w_fu, s);
            uint32_t un = 0xFFFFFFFEu, nu = 0, members = 0;      // (no posting is 0xFFFFFFFE or 0xFFFFFFFF: unit numbers have 31 bits)
            WALK_STAMP(const unsigned long long dg_r0 = WALK_CLOCK(), dg_rl = dg_load;)
            uint32_t L_next = rows[(uint32_t)s * DIST_WALK_ROW + (lane & 31u)];      // the list of the member to come, fetched while this one is tested
            for (int64_t j = c0 + s; j < n; ++j) {
                if (j - wb == 64) { load_window(j, false, false, fu); L_next = rows[lane & 31u]; }
                const int sl = (int)(j - wb);
                if (cf_readlane64(w_fu, sl) != fu) break;
                WALK_STAMP(++dg_n;)
                const uint32_t len = (uint32_t)__builtin_amdgcn_readlane((int)w_len, sl);
                const uint32_t L = lane < len ? L_next : 0xFFFFFFFFu;      // (len <= cap below: the list's lanes)
                L_next = rows[(uint32_t)min(sl + 1, 63) * DIST_WALK_ROW + (lane & 31u)];
                uint32_t mask = 0, fresh = 0;
                bool start = true;
                if (len > cap) { nu = 0; members = 0; }      // a group of its own (it counts); the next k-mer starts one too
                else if (kTab) {
                    WALK_STAMP(if (nu) dg_p += len;)
                    bool hit = false;
                    uint32_t bit = 0;
                    if (nu && lane < len)      // (nu == 0: nothing to find, and the table may hold what a list of more than cap postings left standing)
                        for (uint32_t h = cf_walk_home(L);; h = (h + 1u) & (DIST_WALK_TAB - 1u)) {
                            const unsigned long long e = tab[h];
                            if ((uint32_t)e == L) { hit = true; bit = (uint32_t)(e >> 32); break; }
                            if (e == DIST_WALK_EMPTY) break;
                        }
                    const uint32_t found = nu ? (uint32_t)cf_ballot(hit) : 0u;
                    const uint32_t mine = (uint32_t)((1ull << len) - 1ull);
                    uint32_t nm = mine & ~found;
                    start = members == 0u || members == DIST_CLASS_CAP || nu + (uint32_t)__popc(nm) > cap;
                    if (start) {      // a cut: the table is empty again
                        nu = 0; members = 0; nm = mine;
                        __builtin_amdgcn_wave_barrier();
                        tab[lane] = DIST_WALK_EMPTY;
                        __builtin_amdgcn_wave_barrier();
                    } else if (hit) atomicOr(&o_or[sl], 1u << bit);
                    fresh = nm;
                    if (lane < len && ((nm >> lane) & 1u)) {      // (len <= 32: the shifts stay below the word's width) the new postings take the bits nu, nu + 1, ... in the list's order
                        const unsigned long long e = ((unsigned long long)(nu + (uint32_t)__popc(nm & ((1u << lane) - 1u))) << 32) | (unsigned long long)L;
                        for (uint32_t h = cf_walk_home(L); atomicCAS(&tab[h], DIST_WALK_EMPTY, e) != DIST_WALK_EMPTY; h = (h + 1u) & (DIST_WALK_TAB - 1u)) {}
                    }
                    __builtin_amdgcn_wave_barrier();      // (the next member's probes come after these inserts)
                    const uint32_t c = (uint32_t)__popc(nm);
                    mask = (uint32_t)(((1ull << c) - 1ull) << nu);
                    nu += c;
                    ++members;
                }
                else {
                    WALK_STAMP(if (nu) dg_p += len;)
                    uint32_t found = 0;      // the postings of the list that the union has
                    // eight postings to a trip, without a branch: the broadcasts and compares of a trip do not wait for each other.  A posting is in
                    // the union once at most, and the lane that holds it there IS its bit: the ballot goes into the mask as it is.  (The lanes of L
                    // beyond the list hold 0xFFFFFFFF and the lanes of the union beyond nu 0xFFFFFFFE: they never match.)
                    if (nu)
                        for (uint32_t t0 = 0; t0 < len; t0 += 8u) {
#pragma unroll
                            for (uint32_t q = 0; q < 8u; ++q) {
                                const unsigned long long h = cf_ballot(un == (uint32_t)__builtin_amdgcn_readlane((int)L, (int)(t0 + q)));
                                mask |= (uint32_t)h;
                                found |= (uint32_t)(h != 0ull) << (t0 + q);
                            }
                        }
                    const uint32_t mine = (uint32_t)((1ull << len) - 1ull);
                    uint32_t nm = mine & ~found;
                    start = members == 0u || members == DIST_CLASS_CAP || nu + (uint32_t)__popc(nm) > cap;
                    if (start) { nu = 0; members = 0; mask = 0; nm = mine; un = 0xFFFFFFFEu; }
                    fresh = nm;
                    while (nm) {
                        const int t = __ffs((int)nm) - 1;
                        nm &= nm - 1u;
                        const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)L, t);
                        if (lane == nu) un = x;
                        mask |= 1u << nu;
                        ++nu;
                    }
                    ++members;
                }
                if (lane == (uint32_t)sl) { o_start = start; o_mask = mask; o_new = fresh; o_done = true; }
            }
            WALK_STAMP(dg_mem += (WALK_CLOCK() - dg_r0) - (dg_load - dg_rl);)
        }
        flush();
    }
    for (int d = 32; d >= 1; d >>= 1) { ent += __shfl_down(ent, (unsigned)d); self += __shfl_down(self, (unsigned)d); }
    if (lane == 0u) {
        if (ent) atomicAdd(entries_out, ent);
        if (self) atomicAdd(self_out, self);
#if defined(CF_WALK_STAMPS)
        const unsigned long long dg_t1 = WALK_CLOCK();
        atomicAdd(dg + 0, dg_mem); atomicAdd(dg + 1, dg_load); atomicAdd(dg + 2, dg_t1 - dg_t0); atomicAdd(dg + 3, dg_n); atomicAdd(dg + 4, dg_p); atomicAdd(dg + 5, 1ull);
        atomicMax(dg + 8 + 2 * (size_t)blockIdx.x, ~dg_t0); atomicMax(dg + 9 + 2 * (size_t)blockIdx.x, dg_t1);
#endif
    }
}
// Per group g (the k-mers order[gfirst[g] .. gfirst[g + 1])): the union of the members' lists at upost[32 g ..] — every member's new postings, in
// the order of joining — and its size in ulen[g] (bit 31: a counting group — no union, the sweep takes the k-mer's own list).
// A TEAM of DIST_FILL_TEAM lanes per group (a thread per group walked members and bits one load after the other): lane t takes
// member t of a batch, the counts of new postings are prefix-summed across the team, and every member's lane writes its own.  (A group has
// 3.6 members on the bench's reads: teams of 32 left the wave with two chains of loads in flight, 1.68 ms against the thread per group's 1.42.)
#define DIST_FILL_TEAM 8
__global__ void __launch_bounds__(256)
cf_group_fill_kernel(const int32_t* __restrict__ order, const uint32_t* __restrict__ gfirst, int64_t n_groups, const int64_t* __restrict__ post_ptr, const int32_t* __restrict__ post,
                     const unsigned long long* __restrict__ not_a_set, uint32_t cap, const uint32_t* __restrict__ new_mask, const uint32_t* __restrict__ member_mask,
                     int32_t* __restrict__ upost, uint32_t* __restrict__ ulen, unsigned long long* __restrict__ diag, unsigned long long* __restrict__ err) {
    const bool off = *not_a_set != 0ull;
    unsigned long long dg_u = 0, dg_c = 0;
    constexpr uint32_t T = DIST_FILL_TEAM;
    const uint32_t tl = threadIdx.x & (T - 1u);
    const int64_t team = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / T, n_teams = ((int64_t)gridDim.x * blockDim.x) / T;
    for (int64_t g0 = 0; g0 < n_groups; g0 += n_teams) {      // (uniform trip count: shuffles inside)
        const int64_t g = g0 + team;
        const bool on = g < n_groups;
        uint32_t f = 0, e = 0;
        if (on) { f = gfirst[g]; e = gfirst[g + 1]; }
        bool counting = off;
        if (on && e - f == 1u) { const int32_t x = order[f]; counting = counting || (uint32_t)(post_ptr[x + 1] - post_ptr[x]) > cap; }
        const uint32_t n_mem = (on && !counting) ? e - f : 0u;
        uint32_t n_max = n_mem;      // (the wave's teams loop together)
        for (uint32_t d = T; d < 64u; d <<= 1) n_max = max(n_max, __shfl_xor(n_max, (int)d));
        uint32_t k = 0;
        for (uint32_t b = 0; b < n_max; b += T) {
            const uint32_t j = f + b + tl;
            uint32_t nm = b + tl < n_mem ? new_mask[j] : 0u;
            const uint32_t c = (uint32_t)__popc(nm);
            uint32_t incl = c;
            for (uint32_t d = 1; d < T; d <<= 1) { const uint32_t t = __shfl_up(incl, d, (int)T); if (tl >= d) incl += t; }
            uint32_t at = k + incl - c;
            if (nm) {
                const int64_t p0 = post_ptr[order[j]];
                while (nm) {
                    const int t = __ffs((int)nm) - 1;
                    nm &= nm - 1u;
                    if (at < DIST_GROUP_MAX) upost[(size_t)DIST_GROUP_MAX * (size_t)g + at] = post[p0 + t];
                    ++at;
                }
            }
            k += __shfl(incl, (int)T - 1, (int)T);
        }
        if (!on || tl != 0u) continue;      // (no shuffle below)
        if (k > DIST_GROUP_MAX) { atomicOr(err, 4ull); k = DIST_GROUP_MAX; }      // (cf_group_walk_kernel cut the run so that this cannot be: the launch fails)
        ulen[g] = counting ? 0x80000000u : k;
        dg_u += k;
#if defined(CF_DIST_DIAG_COUNT)      /* the group's classes: its distinct member masks (equal lists in one group have equal masks) */
        for (uint32_t j = f; j < e; ++j) {
            bool seen = false;
            for (uint32_t q = f; q < j && !seen; ++q) seen = member_mask[q] == member_mask[j];
            dg_c += (unsigned long long)!seen;
        }
#endif
    }
#if defined(CF_DIST_DIAG_COUNT)
    for (int d = 32; d >= 1; d >>= 1) { dg_u += __shfl_down(dg_u, (unsigned)d); dg_c += __shfl_down(dg_c, (unsigned)d); }
    if ((threadIdx.x & 63) == 0 && dg_c) { atomicAdd(diag, dg_u); atomicAdd(diag + 1, dg_c); }
#else
    (void)diag; (void)dg_u; (void)dg_c; (void)member_mask;
#endif
}


// lanes below this one whose bit is set in a ballot: v_mbcnt_lo + v_mbcnt_hi (2 instructions; popcount(mask & lanemask_lt) is 4)
// bit (off mod 32) of w in ONE instruction: v_bfe_u32 takes the low five bits of its offset operand, which the compiler does not use
// (it masks the offset first, or shifts and masks); the host emulator (tests/emu) defines the macro of the same name
#ifndef cf_bit_of
__device__ __forceinline__ uint32_t cf_bit_of(uint32_t w, uint32_t off) { uint32_t r; asm("v_bfe_u32 %0, %1, %2, 1" : "=v"(r) : "v"(w), "v"(off)); return r; }
#endif
__device__ __forceinline__ uint32_t cf_rank_in(unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

#define DIST_QCAP 384                    /* deferred inserts per wave: fewer than 128 left by the drains before a step + at most 4 x 64 pushed by it */
#define DIST_QSTRIDE DIST_QCAP
#define DIST_FULL_BIT 0x80000000u        /* sh[0]: the table is physically full (the pass is void and will be split) */

// general insert: walk buckets from bk; claims the first empty slot with a CAS when the key is absent.
// Returns 1 when a new key was created; hot := the slot when this occurrence brought its count to exactly min_cov.
template <class Tab>
__device__ __forceinline__ uint32_t cf_dist_insert(const Tab& T, uint32_t n_buckets, uint32_t bk, uint32_t b, uint32_t dd, uint32_t* sh, uint32_t min_cov, uint32_t& hot, unsigned long long* trips = nullptr, uint32_t bit = 0u) {      // (bit: the posting's place in the union, cf_tab_mask only)
    for (uint32_t tries = 0; tries < 9 * n_buckets; ++tries) {
        if (trips) ++*trips;
        const typename Tab::bucket k = T.read(bk);
        const int m = T.match(k, b, dd);
        if (m >= 0) {
            uint32_t now;
            if constexpr (Tab::kMaskTab) now = T.add(bk, m, bit); else now = T.add(bk, m);
            if (now == min_cov) hot = Tab::kSlotsPerBucket * bk + (uint32_t)m;
            return 0u;
        }
        const int e = Tab::empty(k);
        if (e >= 0) {
            uint32_t cnt;
            int st;
            if constexpr (Tab::kMaskTab) st = T.claim_finish(T.claim_issue(bk, e, b, dd), bk, e, b, dd, cnt, bit); else st = T.claim_finish(T.claim_issue(bk, e, b, dd), bk, e, b, dd, cnt);
            if (st != 2 && cnt == min_cov) hot = Tab::kSlotsPerBucket * bk + (uint32_t)e;
            if (st == 0) return 1u;
            if (st == 1) return 0u;
            continue;   // another key took the slot: look at the same bucket again
        }
        bk = T.next(bk, b, n_buckets);
    }
    atomicOr(&sh[0], DIST_FULL_BIT);
    return 0u;
}

// Diagnostic build only (-DCF_DIST_STAMPS, tools/dist_stamps.py): per-phase shader-clock sums of thread 0 of every
// workgroup into counters[8..15]; the shipped library compiles these to nothing.
#if defined(CF_DIST_STAMPS)
#define CF_STAMP(i) do { if (threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); stamp_acc[i] += now_ - stamp_t; stamp_t = now_; } } while (0)
#else
#define CF_STAMP(i) do { } while (0)
#endif

// Round 3: the work lists of the sweeps are built ONCE per launch, in HBM, by two small kernels (one wave per first k-mer),
// instead of once per first k-mer inside cf_dist_kernel.  There every workgroup loaded its postings and their partner ranges
// (two dependent round trips), scanned the item counts, searched the posting of every item and wrote the records to LDS behind
// three barriers: 8 % of the kernel's time, 6.5 KB of its LDS, and every step of both sweeps first had to find its posting
// (round 2: 25 vector + 40 scalar instructions per step).  Now a wave reads its 8-byte records with one coalesced load.
// Both kernels give every first k-mer a GROUP of 16 lanes (most have fewer than 16 postings): four first k-mers per wave are in
// flight at once — the work per first k-mer is a chain of dependent loads (order -> post_ptr -> post -> urange), so the kernels are
// bound by how many chains run side by side.
// cf_items_count_kernel also counts the partner entries that are the first k-mer itself: the pairs of its postings (u, v) in one
// read with min_d <= v - u <= max_d (the reference skips a == b, distance_based_kmer_recruitment.py:118; the sweeps count such an
// entry like any other and the host subtracts this sum).
// GRP (groups): the list of head i is the UNION of its group, upost[32 i .. 32 i + ulen[i]) — or, ulen[i] bit 31, the k-mer's own
// list (a counting group of one); the self pairs are not counted here (cf_group_walk_kernel counts every member's own)
template <bool GRP>
__global__ void __launch_bounds__(256)
cf_items_count_kernel(const int32_t* __restrict__ order, int64_t n_order, const int64_t* __restrict__ post_ptr, const int32_t* __restrict__ post,
                      const cf_dist_rec* __restrict__ urange, const int32_t* __restrict__ rbeg, int32_t min_d, int32_t max_d, uint32_t nw, int sorted_post,
                      uint32_t* __restrict__ n_items, uint32_t* __restrict__ n_alloc, unsigned long long* __restrict__ self_pairs, const uint32_t* __restrict__ cfirst,
                      const int32_t* __restrict__ upost, const uint32_t* __restrict__ ulen) {
    // cfirst != nullptr: n_order CLASSES; class i is the k-mers order[cfirst[i] .. cfirst[i + 1]) — equal posting lists — and order[cfirst[i]] stands
    // for them (the self pairs are the same for every member: counted once, times the members).  nullptr: every k-mer of `order` on its own.
    const int gl = threadIdx.x & 15;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int64_t n_grp = ((int64_t)gridDim.x * blockDim.x) >> 4;
    unsigned long long self = 0;
    // (the first two links of an iteration's chain — order -> post_ptr — are fetched one iteration ahead)
    int64_t p0_n = 0, p1_n = 0;
    const int32_t* lp_n = post;      // the list that p0 / p1 index: post[], or (GRP) the unions
    auto list_of = [&](int64_t i, const int32_t*& lp, int64_t& q0, int64_t& q1) {
        if constexpr (GRP) { const uint32_t n = ulen[i]; if (!(n >> 31)) { lp = upost; q0 = (int64_t)DIST_GROUP_MAX * i; q1 = q0 + (int64_t)n; return; } }
        const int32_t a0 = order[cfirst ? (int64_t)cfirst[i] : i];
        lp = post; q0 = post_ptr[a0]; q1 = post_ptr[a0 + 1];
    };
    if (grp < n_order) list_of(grp, lp_n, p0_n, p1_n);
    for (int64_t i0 = 0; i0 < n_order; i0 += n_grp) {      // (uniform trip count: shuffles inside)
        const int64_t i = i0 + grp;
        const bool on = i < n_order;
        const int64_t p0 = p0_n, p1 = p1_n;
        const int32_t* lp = lp_n;
        { const int64_t in = i + n_grp; p0_n = 0; p1_n = 0; if (in < n_order) list_of(in, lp_n, p0_n, p1_n); }
        const unsigned long long self_before = self, members = (cfirst && on) ? (unsigned long long)(cfirst[i + 1] - cfirst[i]) : 1ull;
        unsigned long long c = 0;
        int64_t np_max = p1 - p0;      // the longest posting list among the wave's four groups bounds the loops
        for (int d = 16; d <= 32; d <<= 1) np_max = max(np_max, __shfl_xor(np_max, d));
        for (int64_t x0 = 0; x0 < np_max; x0 += 16) {
            const bool hx = p0 + x0 + gl < p1;
            const int32_t ux = hx ? lp[p0 + x0 + gl] : 0;
            cf_dist_rec rx_{0u, 0u, 0u, 0u};
            if (hx) rx_ = urange[ux];
            const int32_t rx = hx ? ux - (int32_t)rx_.ig : -1;      // first unit of the posting's read (ig = the unit's index in its read): ONE gather per posting
            if (hx) c += (rx_.len + DIST_ITEM - 1u) / DIST_ITEM;
            if (GRP || np_max < 2) continue;
            if (sorted_post && np_max <= 16) {
                // (round 6) the postings of a k-mer are in ascending unit order (when they were made by the sort: not by the atomics' fill pass), so two of them in ONE read stand next to each other: when
                // no posting of the wave's four first k-mers has its successor in its own read — the usual case: a rare k-mer occurs once per
                // read — there is no pair to count, and the 16 rounds of shuffles below are skipped (with the mask-and-shift of cf_items_fill_kernel: set-up 17.9 -> 17.2 ms)
                const int32_t r_next = __shfl(rx, (gl + 1) & 15, 16);
                const bool adj = hx && gl < 15 && p0 + gl + 1 < p1 && r_next == rx;
                if (!cf_ballot(adj)) continue;
            }
            for (int64_t y0 = 0; y0 < np_max; y0 += 16) {
                const bool hy = p0 + y0 + gl < p1;
                int32_t uy_l = ux, ry_l = hx ? rx : -2;      // (the same 16 postings: nearly every first k-mer has at most 16)
                if (y0 != x0) { uy_l = hy ? lp[p0 + y0 + gl] : 0; ry_l = hy ? uy_l - (int32_t)urange[uy_l].ig : -2; }
                for (int j = 0; j < 16; ++j) {
                    const int32_t uy = __shfl(uy_l, j, 16), ry = __shfl(ry_l, j, 16);
                    const int32_t d = uy - ux;
                    self += (unsigned long long)(hx && ry == rx && d >= min_d && d <= max_d);
                }
            }
        }
        self = self_before + (self - self_before) * members;
        for (int d = 8; d >= 1; d >>= 1) c += __shfl_down(c, (unsigned)d, 16);
        if (on && gl == 0) {
            const uint32_t n = (uint32_t)min(c, 0xFFFFFFFFull - 2048ull);
            n_items[i] = n;
            n_alloc[i] = ((n + nw - 1u) / nw) * nw;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) self += __shfl_down(self, (unsigned)d);
    if ((threadIdx.x & 63) == 0 && self) atomicAdd(self_pairs, self);
}

// The order of a first k-mer's items.  The sketch sweep only has to find the k-mers b with some cnt(a, b, d) >= min_cov.
// A cloud row is a set, so inside the partner range of ONE posting every (b, d) occurs at most once: cnt(a, b, d) <= P_d(a), the
// number of postings of a whose partner range has a unit at distance d.  P_d falls as d grows; with nu_i the partner units of
// posting i, d* = min_d - 1 + (the min_cov-th largest nu_i) is the largest distance with P_d >= min_cov, and an entry of a unit
// further away than d* belongs to a pair that cannot reach min_cov: counting it in the sketch only adds collisions and marks.  So the
// items are numbered USEFUL ones first (0 .. nA - 1), then the TAIL items — those whose first entry lies in a unit beyond d* (an item
// that straddles the boundary is useful: over-counting is safe); inside each group posting by posting, as before.  The sketch sweep
// takes the first nA items, the table sweep all n (the totals of the filter need every distance of a marked b).  Item boundaries,
// their number and the record format are what they were.
// nA = n (every item useful, and then the numbering is exactly the old one) when
//   * tail == 0: the knob dist_sketch_tail is 0, or the launch runs without the sketch (min_cov < 2, dist_sketch 0);
//   * *not_a_set != 0: cf_entry_unit_kernel found a row with a repeated rank in this launch's clouds (cf_set_clouds takes any rows;
//     the bound needs sets) — read here on the device, no host synchronisation;
//   * the first k-mer has more than 16 * DIST_SEL_CHUNKS = 64 postings: the selection below keeps the nu_i of a list in registers, four per
//     lane of the group.  A performance fall-back, not an approximation.
// If fewer than min_cov postings have a partner unit at all, no pair of a can reach min_cov: nA = 0.
// -DCF_DIST_DIAG_COUNT: diag[0] += sum of nA, diag[1] += sum of n over the launch (one atomic each per wave, at the kernel's end).
#define DIST_SEL_CHUNKS 4
template <bool GRP>      // (as in cf_items_count_kernel; the item records then carry the posting's place in the union, the head whether the group counts)
__global__ void __launch_bounds__(256)
cf_items_fill_kernel(const int32_t* __restrict__ order, int64_t n_order, const int64_t* __restrict__ post_ptr, const int32_t* __restrict__ post,
                     const cf_dist_rec* __restrict__ urange, uint32_t nw, const uint32_t* __restrict__ n_items, const int64_t* __restrict__ ibase,
                     cf_dist_head* __restrict__ heads, cf_dist_item* __restrict__ items, const int64_t* __restrict__ cloud_ptr, int stream26, int64_t n_units,
                     int32_t min_d, int32_t max_d, uint32_t min_cov, int tail, const unsigned long long* __restrict__ not_a_set, unsigned long long* __restrict__ diag,
                     const uint32_t* __restrict__ cfirst, const int32_t* __restrict__ upost, const uint32_t* __restrict__ ulen) {
    // cfirst: as in cf_items_count_kernel — n_order classes, the work list of a class made from its representative's postings
    // stream26: the 26-bit stream (cf_tab_region26): the item record's low half is [t64 : 9 | unit index mod 128 : 7]
    const int gl = threadIdx.x & 15;
    const int64_t grp = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int64_t n_grp = ((int64_t)gridDim.x * blockDim.x) >> 4;
    const bool nw_pow2 = (nw & (nw - 1u)) == 0u;
    const uint32_t nw_log2 = 31u - (uint32_t)__clz((int)max(nw, 1u));
    const bool tail_on = tail && min_cov >= 2u && max_d >= min_d && *not_a_set == 0ull;      // (uniform over the launch)
    const int sel_bits = 32 - __clz((int)(max_d >= min_d ? max_d - min_d + 1 : 1));         // nu <= max_d - min_d + 1 <= 65535
#if defined(CF_DIST_DIAG_COUNT)
    unsigned long long dg_a = 0, dg_n = 0;
#endif
    int32_t a_n = 0; int64_t p0_n = 0, p1_n = 0, ib_n = 0; uint32_t n_n = 0;      // (fetched one iteration ahead, as in cf_items_count_kernel)
    uint32_t f_n = 0, m_n = 1;      // the class's first position in `order` and its members
    const int32_t* lp_n = post;      // the list that p0 / p1 index: post[], or (GRP) the unions
    uint32_t cnt_n = 0;              // GRP: bit 31 = a counting group
    auto head_of = [&](int64_t i) {
        f_n = cfirst ? cfirst[i] : (uint32_t)i; m_n = cfirst ? cfirst[i + 1] - f_n : 1u; a_n = order[f_n]; n_n = n_items[i]; ib_n = ibase[i];
        lp_n = post; cnt_n = 0;
        if constexpr (GRP) { cnt_n = ulen[i]; if (!(cnt_n >> 31)) { lp_n = upost; p0_n = (int64_t)DIST_GROUP_MAX * i; p1_n = p0_n + (int64_t)cnt_n; return; } }
        p0_n = post_ptr[a_n]; p1_n = post_ptr[a_n + 1];
    };
    if (grp < n_order) head_of(grp);
    for (int64_t i0 = 0; i0 < n_order; i0 += n_grp) {      // (uniform trip count: shuffles inside)
        const int64_t i = i0 + grp;
        const bool on = i < n_order;
        const int32_t a = a_n;
        const int64_t p0 = p0_n, p1 = p1_n;
        const uint32_t n = n_n, per = (n + nw - 1u) / nw;
        const int64_t ib = ib_n;
        const uint32_t c_first = f_n, c_members = GRP ? (m_n | (cnt_n & 0x80000000u)) : m_n;
        const int32_t* lp = lp_n;
        { const int64_t in = i + n_grp; a_n = 0; p0_n = 0; p1_n = 0; n_n = 0; ib_n = 0; f_n = 0; m_n = 1;
          if (in < n_order) head_of(in); }
        cf_dist_item* out = items + ib;
        int64_t np_max = p1 - p0;
        for (int d = 16; d <= 32; d <<= 1) np_max = max(np_max, __shfl_xor(np_max, d));
        // one posting per lane of the group, DIST_SEL_CHUNKS x 16 of them in registers: the partner range, the posting's unit and (26-bit
        // stream) where, inside the range, the first entry lies whose unit is 64 or more behind the posting's
        auto fetch = [&](int64_t q0, cf_dist_rec& r, int32_t& ux, uint32_t& rel64) {
            r = cf_dist_rec{0u, 0u, 0u, 0u}; ux = 0; rel64 = 0u;
            if (p0 + q0 + gl < p1) {
                ux = lp[p0 + q0 + gl];
                r = urange[ux];
                if (stream26) { const int64_t c64 = (int64_t)ux + 64 <= n_units ? cloud_ptr[(int64_t)ux + 64] : (int64_t)r.e0 + (int64_t)r.len; rel64 = (uint32_t)(min(max(c64, (int64_t)r.e0), (int64_t)r.e0 + (int64_t)r.len) - (int64_t)r.e0); }
            }
        };
        cf_dist_rec rk[DIST_SEL_CHUNKS]; int32_t uk[DIST_SEL_CHUNKS]; uint32_t r64k[DIST_SEL_CHUNKS], ck[DIST_SEL_CHUNKS];
#pragma unroll
        for (int q = 0; q < DIST_SEL_CHUNKS; ++q) {
            rk[q] = cf_dist_rec{0u, 0u, 0u, 0u}; uk[q] = 0; r64k[q] = 0u;
            if ((int64_t)q * 16 < np_max) fetch((int64_t)q * 16, rk[q], uk[q], r64k[q]);
            ck[q] = (rk[q].len + DIST_ITEM - 1u) / DIST_ITEM;      // useful items of the posting: all of them, unless the selection below says less
        }
        uint32_t nA = n;
        const bool exact = tail_on && p1 - p0 <= 16 * DIST_SEL_CHUNKS;      // (uniform in the group)
        if (tail_on) {      // (uniform in the wave: shuffles inside)
            // the min_cov-th largest nu of the group's postings = the largest t with #{nu_i >= t} >= min_cov, bit by bit from the top (0: there is none)
            uint32_t nu_star = 0;
            for (int bit = sel_bits - 1; bit >= 0; --bit) {
                const uint32_t cand = nu_star | (1u << bit);
                uint32_t c = 0;
#pragma unroll
                for (int q = 0; q < DIST_SEL_CHUNKS; ++q) c += (uint32_t)(rk[q].nu >= cand);
                for (int d = 8; d >= 1; d >>= 1) c += __shfl_xor(c, d, 16);
                if (c >= min_cov) nu_star = cand;
            }
            uint32_t sA = 0;
#pragma unroll
            for (int q = 0; q < DIST_SEL_CHUNKS; ++q) {
                // a posting with more partner units than nu_star is cut behind its nu_star-th (at most min_cov - 1 postings of a list are): the
                // unit at distance d* + 1 is the posting's unit + min_d + nu_star, inside its range
                if (exact && rk[q].nu > nu_star) {
                    uint32_t useful = 0;
                    if (nu_star) useful = ((uint32_t)cloud_ptr[(int64_t)uk[q] + min_d + (int64_t)nu_star] - rk[q].e0 + DIST_ITEM - 1u) / DIST_ITEM;
                    ck[q] = min(ck[q], useful);
                }
                sA += ck[q];
            }
            for (int d = 8; d >= 1; d >>= 1) sA += __shfl_xor(sA, d, 16);
            if (exact) nA = sA;
        }
        uint32_t jA0 = 0, jT0 = nA;      // useful / tail items of the postings before this chunk (group-uniform)
        unsigned long long ne = 0;
        auto emit = [&](const cf_dist_rec& r, uint32_t rel64, uint32_t cA, uint32_t q0) {      // (q0 + gl: the posting's place in its list)
            const uint32_t c = (r.len + DIST_ITEM - 1u) / DIST_ITEM;
            uint32_t incA = cA, incT = c - cA;
            for (int d = 1; d < 16; d <<= 1) { const uint32_t o = __shfl_up(incA, (unsigned)d, 16); if (gl >= d) incA += o; }
            if (tail_on) for (int d = 1; d < 16; d <<= 1) { const uint32_t o = __shfl_up(incT, (unsigned)d, 16); if (gl >= d) incT += o; }
            const uint32_t jbA = jA0 + incA - cA, jbT = jT0 + incT - (c - cA) - cA;      // the lane's first useful item; its first tail item less the useful ones before it
            for (uint32_t x = 0; x < c; ++x) {
                const uint32_t j = (x < cA ? jbA : jbT) + x, off = x * DIST_ITEM;
                uint32_t low = r.ig & 0xFFFFu;
                if (stream26) low = ((rel64 > off ? min(rel64 - off, DIST_ITEM) : 0u) << 7) | (r.ig & 127u);
                // (round 6: the waves of a workgroup are a power of two in every launch shape the library picks — a mask and a shift
                // instead of two divisions by a run-time number per item record, 6.9e8 of them at 50 000 reads)
                const uint32_t jw = nw_pow2 ? (j & (nw - 1u)) : j % nw, jq = nw_pow2 ? (j >> nw_log2) : j / nw;
                uint32_t high = min(r.len - off, DIST_ITEM);
                if constexpr (GRP) high |= ((q0 + (uint32_t)gl) & 31u) << 11;      // [place in the union : 5 | 0 : 2 | entries : 9]
                out[(size_t)jw * per + jq] = cf_dist_item{r.e0 + off, (high << 16) | low};
            }
            jA0 += (uint32_t)__shfl((int)incA, 15, 16);
            if (tail_on) jT0 += (uint32_t)__shfl((int)incT, 15, 16);
            unsigned long long l = r.len;
            for (int d = 8; d >= 1; d >>= 1) l += __shfl_down(l, (unsigned)d, 16);
            ne += (unsigned long long)__shfl((long long)l, 0, 16);
        };
#pragma unroll
        for (int q = 0; q < DIST_SEL_CHUNKS; ++q) if ((int64_t)q * 16 < np_max) emit(rk[q], r64k[q], ck[q], (uint32_t)q * 16u);
        for (int64_t q0 = 16 * DIST_SEL_CHUNKS; q0 < np_max; q0 += 16) {      // the rest of a long list (every item useful)
            cf_dist_rec r; int32_t ux; uint32_t rel64;
            fetch(q0, r, ux, rel64);
            emit(r, rel64, (r.len + DIST_ITEM - 1u) / DIST_ITEM, (uint32_t)q0);
        }
        if (on && gl == 0) {
            heads[i] = cf_dist_head{(uint32_t)a, n, (unsigned long long)ib, (uint32_t)min(ne, 0x3FFFFFFFull), nA, c_members, c_first};
#if defined(CF_DIST_DIAG_COUNT)
            dg_a += nA; dg_n += n;
#endif
        }
    }
#if defined(CF_DIST_DIAG_COUNT)
    for (int d = 32; d >= 1; d >>= 1) { dg_a += __shfl_down(dg_a, (unsigned)d); dg_n += __shfl_down(dg_n, (unsigned)d); }
    if ((threadIdx.x & 63) == 0 && dg_n) { atomicAdd(&diag[0], dg_a); atomicAdd(&diag[1], dg_n); }
#else
    (void)diag;
#endif
}

// Sweeps one wave's items: recs = the wave's records in HBM, mine = how many, my0 = the first 64 of them already in registers
// (lane j: the j-th; loaded at the top of the first k-mer's iteration and used by both sweeps).  A step gets its record with
// two v_readlane into SGPRs — the base address of the step's global load is scalar, the per-lane offset is the constant
// 16 * lane.  Software pipeline: D loads in flight per lane.
// pre(final) runs at ONE site before every step and once more (final = true) after the wave's last step: the table sweep drains
// its insert queue there (one copy of that code in the loop instead of one per push site).
// body(bb, dd, qk, lo, ok, len): the decoded entries of a step; ok = per-lane bit mask of the entries that exist (only the last item of
// a posting has lanes past its end: len < DIST_ITEM, wave-uniform, says whether ok needs looking at); returns true to stop the wave.
// (Round 6, measured and removed: the waves of a workgroup SHARING their items — per list one LDS word [items taken from its end | items its
// owner claimed], the owner's claim in flight under the step before, a wave out of items taking half of what the fullest list has left with
// one record load.  Thread 0's stamps had put 22 % of the kernel on cenX-shaped reads (9 % on the bench's) into waiting for the other waves
// at the end of a sweep; with sharing: 114-116 ms against 109.9 without on those reads, 259-271 against 243.3 on the bench's, whatever the
// thresholds (profiles/r06_dist_ab_steal.log) — the wait is not idle hardware: a wave that is through leaves its issue slots and LDS
// cycles to the others, and a thief's first step waits for two round trips to memory.)
template <class Tab, int D, class Pre, class Body>
__device__ __forceinline__ void cf_dist_sweep(const cf_dist_args& A, const cf_dist_item* recs, uint32_t mine, const cf_dist_item& my0, Pre&& pre, Body&& body) {
    const uint32_t lane = threadIdx.x & 63u, l4 = lane * DIST_UNROLL;
    // entries of an item: the record's high half — in a launch with groups (cf_tab_mask) its low 9 bits, under the posting's
    // place in the group's union [bit : 5 | 0 : 2 | entries : 9]
    auto len_of = [](uint32_t m) -> uint32_t { return Tab::kMaskTab ? (m >> 16) & 0x1FFu : m >> 16; };
    auto ok_of = [&](uint32_t m) -> uint32_t {      // per-lane mask of the entries of an item that exist
        uint32_t ok = (1u << DIST_UNROLL) - 1u;
        if (len_of(m) < DIST_ITEM) {      // (wave-uniform) the last item of a posting
            ok = 0;
#pragma unroll
            for (int u = 0; u < DIST_UNROLL; ++u) ok |= (uint32_t)(l4 + (uint32_t)u < len_of(m)) << u;
        }
        return ok;
    };
    // Round 6: pre(false) in front of every step and pre(true) ONCE behind the loop over the windows (rounds 3-5 computed "is this the
    // wave's last step" inside the loop and passed it to the one call site): 251.5 -> 243.3 ms on the bench's reads, 115.4 -> 109.9 on
    // cenX-shaped ones — found while measuring the work sharing above, whose loop had this shape.
    for (uint32_t j0 = 0; j0 < mine; j0 += 64u) {      // (one window whenever the wave has at most 64 items)
        const uint32_t cnt = min(64u, mine - j0);
        cf_dist_item my = my0;
        if (j0) { my = cf_dist_item{0u, 0u}; if (lane < cnt) my = recs[j0 + lane]; }
        // D loads in flight per lane WHILE a step is worked on: D + 1 register sets, the loop unrolled D + 1 times so that every set has
        // fixed registers — at position p the step's data is set p, and the load of the step D ahead goes into set (p + D) mod (D + 1), the
        // one the previous position has just finished with.  (Rounds 3-4 kept D sets, copied the step's set aside and re-filled it at once:
        // the compiler made the copy a chain of v_mov at the END of the unrolled body, behind an s_waitcnt vmcnt(0) — every wave waited
        // out the loads it had just issued, every D steps, whatever D was; round 5, read off the ISA.)
        constexpr int NS = D + 1;
        typename Tab::raw ring[NS][DIST_UNROLL];
#define CF_DIST_FETCH(J, SET) {                                                                                 \
            const uint32_t s_e = (uint32_t)__builtin_amdgcn_readlane((int)my.e, (int)(J));                      \
            const uint32_t fm_ = (uint32_t)__builtin_amdgcn_readlane((int)my.m, (int)(J));                      \
            Tab::load_run(A, s_e, l4, ok_of(fm_), ring[SET]);                                                   \
        }
#pragma unroll
        for (int d = 0; d < D; ++d) CF_DIST_FETCH(min((uint32_t)d, cnt - 1u), d)      // (unconditional, see below)
        // the steps of this window: a lambda, so that "the window's items are through" leaves the unrolled loop by a plain return — with a flag
        // tested at the loop head the compiler saw a path from every exit back into the loop and made the head wait for every load
        // in flight (s_waitcnt vmcnt(0) in front of the first fetch of every D + 1 steps)
        const bool stop = [&]() -> bool {
            uint32_t j = 0;
            for (;;) {
#pragma unroll
                for (int p = 0; p < NS; ++p) {
                    // The fetch of the step D ahead comes FIRST, in front of pre(): the table sweep's drain runs there, and with a register
                    // set of the ring free at that point the compiler used it for the drain's temporaries — a write to a register that an
                    // earlier load had as its destination, which its wait-count pass could only make safe by waiting for every load in
                    // flight (s_waitcnt vmcnt(0) in every drain).  With all D + 1 sets spoken for the drain gets registers of its own.
                    // Unconditional: a wave past its last item fetches that one again — with a fetch under a condition the number of
                    // loads in flight differs between the paths into the loop head and the compiler waits for ALL of them there.
                    CF_DIST_FETCH(min(j + (uint32_t)D, cnt - 1u), (p + D) % NS)
                    pre(false);
                    if (j == cnt) return false;
                    const uint32_t cm = (uint32_t)__builtin_amdgcn_readlane((int)my.m, (int)j);
                    uint32_t bb[DIST_UNROLL], dd_[DIST_UNROLL], qq_[DIST_UNROLL], lo_[DIST_UNROLL];
#pragma unroll
                    for (int u = 0; u < DIST_UNROLL; ++u) Tab::decode(ring[p][u], cm & 0xFFFFu, l4 + (uint32_t)u, bb[u], dd_[u], qq_[u], lo_[u]);
                    const uint32_t len = len_of(cm);      // entries of the item (wave-uniform); < DIST_ITEM only for the last item of a posting
                    if (body(bb, dd_, qq_, lo_, len < DIST_ITEM ? ok_of(cm) : (1u << DIST_UNROLL) - 1u, len, Tab::kMaskTab ? cm >> 27 : 0u)) return true;
                    ++j;
                }
            }
        }();
#undef CF_DIST_FETCH
        if (stop) return;
    }
    pre(true);      // after the wave's last step: the table sweep empties its queues
}

// loads in flight per lane while a step of either sweep is worked on (measured and not kept, round 5, with the pipeline that really keeps
// them in flight: 2 and 3 in the sketch sweep 251.7 / 257.6 ms against 250.6, in the table sweep 251.7 / 255.5 against 250.7; both at 1: 250.1)
#define DIST_PREFETCH 1

// registers per lane: the launch bound (1024 threads, one workgroup per CU) gives 128 = four waves per SIMD
// CLS: the launch has classes of first k-mers — the heads' n_members may exceed 1 and the section from the filter to the
// rows runs once per member.  A launch without classes (knob dist_classes 0, postings from the atomics' fill pass) takes the instance
// without the member loop: the kernel it had before, instruction for instruction — with the loop in it, a launch of singletons
// ran 9 ms of 243 behind that kernel (14 registers spilled where there were none).
template <class Tab, bool CLS>
__global__ void __launch_bounds__(1024, 1) cf_dist_kernel(cf_dist_args A) {
    // LDS: [bitmap | sh] at FIXED offsets (the bitmap at 0: its word address is the hash bits themselves, no base to add), then
    // [table | edge stage | partition stack | insert queues].  The table group is dead while the sketch sweep runs, so its
    // 8-bit counters (sk) lie over ALL of it.  (The item records of the sweeps are in HBM: cf_items_fill_kernel.)
    const int t = threadIdx.x, lane = t & 63, nt = blockDim.x;
    uint32_t* bm = (uint32_t*)cf_lds_at(0u);                          // DIST_BM_BITS bits: hash(b) of the k-mers b that may have a selected edge
    uint32_t* sh = bm + DIST_BM_BITS / 32;                     // [0] keys in table | DIST_FULL_BIT [1] first k-mer [2] sp [3] P [4] idx [5,6] queue ticket [7] E of pass [8] selected [9,10] edge base [11] hot-list cursor [12] items of the first k-mer [13] a counter of the sketch wrapped [14,15] where its item records start [16..22] the next first k-mer's index and head [23] its useful items (the sketch sweep's) [24, 25] the members of its class and where they start in A.order [26..29] the workgroup's chunk of the edge output [30] rows staged [31] a byte counter of the sketch wrapped
    unsigned char* lds_tab = cf_lds_at(DIST_LDS_HEAD);
    Tab T;
    T.init(lds_tab, (uint32_t)A.slots);
    T.configure(A, (uint32_t)A.slots / Tab::kPerBucket);
    uint32_t* sk = (uint32_t*)lds_tab;
    size_t tab_bytes = (size_t)A.slots * Tab::kSlotBytes;
    if constexpr (Tab::kMaskTab) tab_bytes += Tab::extra_bytes((uint32_t)A.slots);      // (the bitmap of the selection marks)
    uint16_t* stage = (uint16_t*)(lds_tab + tab_bytes);   // slot indices of the selected edges of a pass
    // per-wave queue of pending inserts: candidates are compacted here and inserted 64 at a time by a full wave.
    // Only its own wave touches it: LDS operations of one wave execute in order, and wavefront-scope fences (no
    // instructions) keep the compiler from moving the queue accesses across the drain; a volatile pointer would turn
    // every push into a FLAT store followed by a full vmcnt wait (it did: 4 per step in the first version).
    uint32_t* stack = (uint32_t*)(stage + DIST_STAGE_CAP + 8);                   // (P, idx) pairs
    typename Tab::qitem* wq0 = (typename Tab::qitem*)(stack + 2 * DIST_STACK);
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6)), nw = (uint32_t)nt >> 6;      // (the wave's number in a scalar register: so are the addresses of its queues)
    typename Tab::qitem* wq = wq0 + (size_t)wv * DIST_QSTRIDE;
    // inserts whose FIRST probe did not finish (bucket full, or another key took the slot it wanted): parked here and run
    // through the probe loop 32 .. 64 at a time (round 2 ran that loop inside every drain: most drains went around twice for
    // one or two of their 64 lanes)
    typename Tab::qitem* ovq = wq0 + (size_t)(nt >> 6) * DIST_QSTRIDE + (size_t)wv * DIST_OVQ;
    uint16_t* hotl = (uint16_t*)(wq0 + (size_t)(nt >> 6) * (DIST_QSTRIDE + DIST_OVQ));      // DIST_HOT_CAP slots whose count reached min_cov during the inserts of the pass
    // cf_tab_mask: a byte per queued / parked insert next to its 32-bit word — the place, in the group's union, of the posting that brought it
    uint8_t* wqb = (uint8_t*)(hotl + DIST_HOT_CAP) + (size_t)wv * (DIST_QSTRIDE + DIST_OVQ);
    uint8_t* ovqb = wqb + DIST_QSTRIDE;
    const uint32_t slots = (uint32_t)A.slots, n_buckets = slots / Tab::kPerBucket;   // slots is a multiple of 8
    unsigned long long acc_E = 0, acc_spill = 0, acc_pass = 0, acc_edges = 0;  // flushed once per workgroup (thread 0)
#if defined(CF_DIST_DIAG_COUNT)      /* diagnostic build: [0] loop trips of parked inserts [1] overflow calls [2] parked inserts run [3] drains [4] inserts drained */
    unsigned long long dg_swept = 0;      /* thread 0: partner entries of the passes, once per class (acc_E has them once per member) */
    unsigned long long dg_hot = 0, dg_hot_mem = 0, dg_walks = 0, dg_walk_bk = 0, dg_ovf = 0;      /* the member filter (mask table): thread 0: n_hot per pass, n_hot x members; every thread: eval_slot calls that took total_of, buckets read there */
    unsigned long long dg[8] = {0, 0, 0, 0, 0, 0, 0, 0};      /* [5] shader cycles inside the parked-insert runs [6] inside the drains [7] inside the table sweep, per wave (lane 0) */
#define CF_DG(X) X
#define CF_DG_PTR (&dg[0])
#else
#define CF_DG(X)
#define CF_DG_PTR nullptr
#endif
#if defined(CF_DIST_STAMPS)
    unsigned long long stamp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_t = __builtin_amdgcn_s_memtime();
#endif

    // 8 ticket queues over 8 contiguous ranges of the locality-sorted first k-mers: workgroups with equal blockIdx % 8
    // (observed to share an XCD, i.e. an L2) drain one range; idle ones steal
    // The ticket of the next first k-mer is taken in two halves: pop_issue() sends the atomic on this workgroup's own queue and
    // returns at once, pop_finish() — a phase later — looks at what came back and, only when that queue is exhausted, tries the
    // others.  (Round 2 waited for the returning atomic right where it was issued, at the top of every iteration: a round trip
    // to the memory side with the whole workgroup behind thread 0 at the next barrier, 9 % of the kernel.)
    const int64_t q_per = (A.n_order + 7) / 8;
    auto pop_issue = [&]() -> unsigned long long { return atomicAdd(&A.counters[16 + 16 * (blockIdx.x & 7)], 1ull); };
    auto pop_finish = [&](unsigned long long q) -> long long {
        const int x0 = (int)(blockIdx.x & 7);
        const int64_t lo0 = x0 * q_per, hi0 = min((int64_t)(x0 + 1) * q_per, A.n_order);
        if (lo0 + (int64_t)q < hi0) return lo0 + (int64_t)q;
        for (int s8 = 1; s8 < 8; ++s8) {
            const int x = (int)((blockIdx.x + s8) & 7);
            const int64_t lo = x * q_per, hi = min((int64_t)(x + 1) * q_per, A.n_order);
            if (lo >= hi) continue;
            const unsigned long long q2 = atomicAdd(&A.counters[16 + 16 * x], 1ull);
            if (lo + (int64_t)q2 < hi) return lo + (int64_t)q2;
        }
        return -1;
    };
    // Thread 0 fetches the NEXT first k-mer's head (ticket -> heads[]: two dependent round trips) while the workgroup works on
    // the current one; the values wait in its registers until the loop comes around.
    long long nx_idx = -1;
    cf_dist_head nx_head{0u, 0u, 0ull, 0u, 0u, 1u, 0u};      // (a, items, records, partner entries, useful items)
    unsigned long long nx_q = 0;
    if (!cf_lds_base_ok()) { if (t == 0) atomicOr(&A.counters[4], 2ull); return; }      // (cf_common.h: cf_lds_at)
    // Barriers.  A first k-mer whose table needs one pass — nearly all — meets the workgroup SEVEN times: [top] the previous
    // one's edge rows are written, [sketch cleared], [sketch swept], [table cleared], [table swept], [filtered], [rows reserved].
    // Round 2 and the first half of round 3 had fifteen (the head of the next first k-mer published between two barriers of
    // its own, the partition stack read between two more at the top of every pass and again to find it empty, a barrier
    // between reading the number of selected edges and reusing its word): with ~10 steps per wave and sweep the waves arrive
    // skewed at every one of them, and thread 0's stamps put a third of the kernel into those waits.  Now the next first
    // k-mer's head goes into words of its own (sh[16..22]) in front of an existing barrier — the last pass's reservation —
    // and the default pass (one partition) is set up in front of the sketch's barrier.
    auto publish_next = [&]() {      // thread 0
        sh[16] = (uint32_t)(unsigned long long)nx_idx; sh[17] = (uint32_t)((unsigned long long)nx_idx >> 32);
        sh[18] = nx_head.a; sh[19] = nx_head.n_items; sh[20] = (uint32_t)nx_head.ibase; sh[21] = (uint32_t)(nx_head.ibase >> 32);
        sh[22] = nx_head.n_entries;      // partner entries (sizes the passes when every b is marked)
        sh[23] = nx_head.n_useful;
        if (CLS) { sh[24] = nx_head.n_members; sh[25] = nx_head.first_member; }
    };
    auto pop_pass = [&]() {          // thread 0: the next partition of the stack becomes the pass
        const uint32_t sp = sh[2] - 1; sh[2] = sp; sh[3] = stack[2 * sp]; sh[4] = stack[2 * sp + 1]; sh[0] = 0; sh[7] = 0; sh[8] = 0; sh[11] = 0; sh[30] = 0;
    };
    if (t == 0) {
        nx_idx = pop_finish(pop_issue());
        if (nx_idx >= 0) nx_head = A.heads[nx_idx];
        publish_next();
        sh[26] = 0; sh[27] = 0; sh[28] = 0; sh[29] = 0;      // no chunk of the edge output yet
    }
    __syncthreads();

    while (true) {
        const int64_t ai = (int64_t)(((unsigned long long)sh[17] << 32) | sh[16]);
        if (ai < 0) break;
        const uint32_t a = sh[18], n_items = sh[19], n_ent_a = sh[22], n_useful = sh[23];
        const uint32_t n_mem = CLS ? (Tab::kMaskTab ? sh[24] & 0xFFFFu : sh[24]) : 1u, m_first = CLS ? sh[25] : 0u;
        if constexpr (Tab::kMaskTab) T.set_member(0xFFFFFFFFu, (sh[24] >> 31) != 0u);      // (a head of groups says in bit 31 of its members whether its words are counts: cf_items_fill_kernel)
        // Round 6: the list of slots that reach min_cov (one returning LDS add, a wait and a readfirstlane per drain that has one — on
        // cenX-shaped reads every drain has a dozen) is not kept for a first k-mer that would overflow it anyway: its filter scans the count
        // fields, as it did all along once the list was full (12 of 108 ms there)
#if defined(CF_DIST_DIAG_NOHOT)
        const bool use_hot = false;      // (diagnostic build: no first k-mer keeps the list — the filter must scan, not read an empty list)
#else
        const bool use_hot = n_ent_a <= A.hot_entries;
#endif
        // this wave's item records: one coalesced load, in flight while the sketch is cleared; both sweeps run on them
        const uint32_t per_w = (n_items + nw - 1u) / nw;
        const uint32_t mine = wv < n_items ? (n_items - wv + nw - 1u) / nw : 0u;
        // ... and how many of them the sketch sweep takes: the wave's share of the useful items, which come first in every wave's run
        const uint32_t mineA = wv < n_useful ? (n_useful - wv + nw - 1u) / nw : 0u;
        const cf_dist_item* recs = A.items + ((((unsigned long long)sh[21] << 32) | sh[20]) + (unsigned long long)wv * per_w);
        cf_dist_item my0 = cf_dist_item{0u, 0u};
        if ((uint32_t)lane < min(mine, 64u)) my0 = recs[lane];
        if (t == 0) nx_q = pop_issue();                               // next: the ticket (looked at after phase A)
        __syncthreads();      // [top] the rows of the previous first k-mer are out of the table, and everyone has this one's head
        CF_STAMP(0);   // queue pop
        if (n_items == 0u) {
            if (t == 0) { nx_idx = pop_finish(nx_q); if (nx_idx >= 0) nx_head = A.heads[nx_idx]; publish_next(); }
            __syncthreads();
            continue;
        }
        CF_STAMP(1);   // prologue
        // ---- phase A (min_cov >= 2): which k-mers b can have a selected edge at all?  Most (b, d) pairs of a are seen
        // once or twice and can never reach min_cov, but an exact table would have to hold them all.  So first every
        // pair is only COUNTED, in an array of 8-bit counters indexed by hash(b, d) that fills the table's LDS: a
        // counter is never below the count of a pair that maps to it (collisions add), and the add whose returned
        // value shows the counter reaching min_cov marks hash(b) in a bitmap — the last add of a pair with
        // cnt >= min_cov always does.  Phase B then builds the exact table for the marked b only (all their d, so the
        // totals are exact too); unmarked b have no pair with cnt >= min_cov and cannot be selected.  A counter about
        // to wrap (255 -> 0) is seen by the add that wraps it: the first k-mer then falls back to "every b marked".
        bool mark_all = !A.sketch;
        const uint32_t min_cov_m1 = A.min_cov - 1u;      // (the sketch runs with min_cov >= 2)
        // the pass that nearly every first k-mer gets by with: one partition, every marked b in it (set up here, in front of a
        // barrier that is there anyway; "every b marked" below replaces it)
        if (t == 0) { sh[13] = 0; sh[31] = 0; sh[2] = 0; sh[3] = 1; sh[4] = 0; sh[0] = 0; sh[7] = 0; sh[8] = 0; sh[11] = 0; sh[30] = 0; }
        if (A.sketch) {
            // (round 6) the counters' width for THIS attempt: 4-bit counters that wrap — a burst of 16 adds on one counter before the first
            // of them can take itself back: a pair counted 15 times plus a collision — send the first k-mer through the sketch sweep once
            // more with bytes (half as many counters), not straight to "every b marked" with its 4-8 table passes; the marks made so far stay
            // (a mark too many only lets pairs into the exact table).  The two attempts report their wrap in words of their own (sh[13],
            // sh[31]): nobody resets a word that another thread may still be reading.
            uint32_t m_fbits = A.sk_fbits, m_fsh = A.sk_fsh, m_wshift = A.sk_wshift, m_fmask = A.sk_fmask, m_guard = A.sk_guard, m_shift = A.sk_shift, m_flag = 13u;
            for (;;) {
            {
                const cf_u32x4 z{0u, 0u, 0u, 0u};
                for (uint32_t s = (uint32_t)t; s < (A.sk_bytes >> 4); s += (uint32_t)nt) ((cf_u32x4*)sk)[s] = z;
                if (m_flag == 13u) for (uint32_t s = (uint32_t)t; s < DIST_BM_BITS / 128; s += (uint32_t)nt) ((cf_u32x4*)bm)[s] = z;
                __syncthreads();      // [sketch cleared]
            }
            {
                cf_dist_sweep<Tab, DIST_PREFETCH>(A, recs, mineA, my0, [](bool) {}, [&](const uint32_t (&bb)[DIST_UNROLL], const uint32_t (&dd_)[DIST_UNROLL], const uint32_t (&qq_)[DIST_UNROLL], const uint32_t (&lo_)[DIST_UNROLL], uint32_t ok, uint32_t len, uint32_t) -> bool {
                    // (entries equal to a are counted too: the sketch may only over-count, and the table sweep drops them)
                    uint32_t old_[DIST_UNROLL], sft_[DIST_UNROLL], inc_[DIST_UNROLL];
#pragma unroll
                    for (int u = 0; u < DIST_UNROLL; ++u) {
                        // (Measured and not kept, round 6: a counter per b — the low bits of the rank, i.e. of the raw stream word (lo_[u] & A.sk_mask):
                        // no decode, no multiply; Σ_d cnt(a, b, ·) bounds every cnt(a, b, d).  Its collisions NEST with the bitmap's (two counters per
                        // bit), and on reads whose rare k-mers are copy-specific it lets fewer pairs through — 0.355 of the pairs inserted instead of
                        // 0.394 on cenX-shaped reads, 6 100 keys per first k-mer instead of 7 900: 108.0 -> 101.9 ms — but a k-mer that recurs along
                        // the array has pairs at every distance, is marked as a whole, and brings a key per distance into ONE probe chain:
                        // var_len 1 on the same reads 7.75 -> 9.2 ms with 6 x the split tables.  profiles/r06_dist_ab_cenx.log)
                        const uint32_t idx = Tab::sk_hash(bb[u], dd_[u], qq_[u]) >> m_shift;
                        // Round 6: counters of FOUR bits where min_cov allows it (twice as many in the same LDS: on samples of first k-mers 15 % fewer
                        // keys reach the exact table on cenX-shaped reads — 6 800 instead of 7 950 — and 8 % fewer pairs are inserted).  A counter
                        // only has to tell "min_cov - 1 or more": an add that sees 12 or more takes itself back (the counter stays where it is and
                        // every later add still sees >= min_cov - 1), and the add that would wrap a field — it sees 15 — is seen doing it, like the
                        // 255 of the 8-bit counters: the first k-mer falls back to "every b marked".  A carry into the next field only over-counts.
                        sft_[u] = idx << m_fsh;      // (only its low 5 bits are used: the shift and the bit-field extract take them mod 32)
                        inc_[u] = 1u << (sft_[u] & 31u);
                        old_[u] = idx >> m_wshift;
                    }
                    if (len < DIST_ITEM) {      // (wave-uniform) lanes past the end of the posting's range add nothing
#pragma unroll
                        for (int u = 0; u < DIST_UNROLL; ++u) if (!((ok >> u) & 1u)) inc_[u] = 0u;
                    }
#pragma unroll
                    for (int u = 0; u < DIST_UNROLL; ++u) old_[u] = atomicAdd(&sk[old_[u]], inc_[u]);     // all counter adds of the step back to back
                    uint32_t seen_[DIST_UNROLL];
#pragma unroll
                    for (int u = 0; u < DIST_UNROLL; ++u) seen_[u] = __builtin_amdgcn_ubfe(old_[u], sft_[u], m_fbits);     // occurrences before this one (v_bfe_u32 takes the offset mod 32)
                    // ONE test per step: few adds reach min_cov (each of the four branches of round 2 cost a compare, three scalar
                    // exec-mask instructions and a jump)
                    static_assert(DIST_UNROLL == 4, "max of four");
                    const uint32_t seen_max = max(max(seen_[0], seen_[1]), max(seen_[2], seen_[3]));
                    if (seen_max >= min_cov_m1) {
                        // The bit is set without looking first (a read, a wait, a test and a second exec mask per entry: the atomic costs the
                        // LDS what the read did), and lanes past the end of a posting's range (inc 0: they read a counter without adding)
                        // are not told apart: a bit too many in the bitmap only lets entries into the exact table that are then not
                        // selected, and a wrap seen by such a lane only sends the first k-mer down the every-b-marked path.
#pragma unroll
                        for (int u = 0; u < DIST_UNROLL; ++u) {
                            if (seen_[u] >= min_cov_m1) {
                                atomicOr(&bm[Tab::bm_bit(lo_[u]) >> 5], 1u << (lo_[u] & 31u));
                            }
                        }
                        if (seen_max >= m_guard) {      // (4-bit counters only: the guard of the 8-bit ones is beyond their range)
#pragma unroll
                            for (int u = 0; u < DIST_UNROLL; ++u)
                                if (seen_[u] >= m_guard && ((ok >> u) & 1u)) atomicSub(&sk[sft_[u] >> 5], 1u << (sft_[u] & 31u));      // (idx << fsh >> 5 = idx >> wshift: the counter's word; the increment is made again: kept in a register it made the kernel spill)
                        }
                        if (seen_max == m_fmask) sh[m_flag] = 1u;
                    }
                    return false;
                });
                CF_STAMP(6);   // sketch sweep (clear + wave 0's own items)
            }
            __syncthreads();      // [sketch swept]
            CF_STAMP(7);      // (stamp 7: thread 0's wait for the other waves at the end of a sweep)
            if (!sh[m_flag]) break;
            if (m_fbits == 8u) { mark_all = true; break; }
            m_fbits = 8u; m_fsh = 3u; m_wshift = 2u; m_fmask = 255u; m_guard = 0x7FFFFFFFu; m_shift = A.sk_shift + 1u; m_flag = 31u;
            }
        }
        if (t == 0) { nx_idx = pop_finish(nx_q); if (nx_idx >= 0) nx_head = A.heads[nx_idx]; }      // next: its head (published with the last pass's reservation)
        if (mark_all) {
            const cf_u32x4 ones{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
            for (uint32_t s = (uint32_t)t; s < DIST_BM_BITS / 128; s += (uint32_t)nt) ((cf_u32x4*)bm)[s] = ones;
            if (t == 0) {
                // number of partitions of the exact (b, d) table: every pair may need a slot when all b are marked
                // (upper bound from the emission count); with the bitmap only a fraction does — one, set up above
                uint32_t P0 = 1;
                while (P0 < 64u && (unsigned long long)n_ent_a > (unsigned long long)A.est_limit * P0) P0 <<= 1;
                for (uint32_t i = 0; i < P0; ++i) { stack[2 * i] = P0; stack[2 * i + 1] = i; }
                sh[2] = P0;
                pop_pass();
            }
        }
        bool spilled = false;
        T.clear(slots, (uint32_t)t, (uint32_t)nt);      // (the sketch is dead: its counters lay over the table)
        __syncthreads();      // [table cleared] (and, when every b is marked, the bitmap filled and the passes set up)
        while (true) {
            const uint32_t P = sh[3], pidx = sh[4], pmask = P - 1u;   // P is a power of two; P == 1: every b belongs to the pass
            if constexpr (Tab::kMaskTab) { if (t == 0) { ((uint32_t*)stage)[0] = 0u; ((uint32_t*)stage)[3] = 0u; } }      // the one-section member filter's words of its first batch (visible behind [table swept])
            uint32_t my_e = 0, s_e = 0;      // partner entries swept by this lane (split passes) / by this wave (whole passes)
            CF_STAMP(2);   // pop partition + clear table
            // ---- phase B: sweep again; pairs of this partition whose b is marked go to the wave's queue and are
            // inserted into the exact table 64 at a time by a full wave
            {
                uint32_t qtail = 0, otail = 0;      // wave-uniform: queued inserts / parked inserts of this wave
                bool too_full = sh[0] > A.fill_limit;      // (another list of this pass may already have filled the table)
                CF_DG(const unsigned long long t2_ = __builtin_amdgcn_s_memtime();)
                cf_dist_sweep<Tab, DIST_PREFETCH>(A, recs, mine, my0, [&](bool final) {
                    // a step pushes at most 4 x 64 inserts: the queue is brought below a drain's worth first; after the wave's last step
                    // both lists are emptied (a pass whose table got too full is void and drops them)
                    constexpr uint32_t kDrain = Tab::kDrainTwoProbes ? 128u : 64u;      // queued inserts per drain
                    const uint32_t lim = final ? 1u : kDrain;
                    if (qtail < lim && !(final && otail > 0u)) return;      // nothing to drain: no look at the fill level either
                    // The three parts of the drain, as lambdas defined HERE, behind the early return, and inlined into the loop below.  (Defined in
                    // front of the sweep — closures that this one captures — or in front of the return they compile to other code than the one
                    // that was measured: other registers in the region and mask kernels, two or three instructions fewer in every kernel.)
                    // Slots whose count just reached min_cov go to the filter's list (one returning LDS atomic per wave and call): the filter then
                    // evaluates that list instead of scanning every slot of the table for counts >= min_cov (round 2: 3 scan rounds per
                    // first k-mer, 7 % of the kernel).  slot: all ones in the lanes that have none.
                    // (measured and not kept, round 5: the slots handed to the list through blocks of 64 entries that a WAVE reserves with one LDS
                    // atomic per 64 entries, cursor and block end in scalar registers, instead of one returning LDS atomic, a wait and a readfirstlane
                    // per drain — 257.4 ms with the blocks, 251.3 without: the unused entries of every wave's last block, marked 0xFFFF, lengthen
                    // the filter's list by up to 64 x waves entries)
                    auto to_hot_list = [&](uint32_t slot) __attribute__((always_inline)) {
#if defined(CF_DIST_DIAG_NOHOT)
                        if (slot == 0xFFFFFFF0u) sh[11] = 1u;      // (diagnostic build: no hot list; the filter scans)
#else
                        const unsigned long long hm = cf_ballot(slot != 0xFFFFFFFFu);
                        if (hm && use_hot) {
                            uint32_t hb = 0;
                            if (lane == 0) hb = atomicAdd(&sh[11], (uint32_t)__popcll(hm));
                            hb = (uint32_t)__builtin_amdgcn_readfirstlane((int)hb) + cf_rank_in(hm);
                            if (slot != 0xFFFFFFFFu && hb < DIST_HOT_CAP) hotl[hb] = (uint16_t)slot;
                        }
#endif
                    };
                    // pops the last n queued inserts and gives each ONE probe of its home bucket: match -> count it; empty slot -> claim it; bucket
                    // full or the slot lost to another key -> parked in the overflow list, which goes through the probe loop once it holds 32.
                    // The table's fill level is read INSIDE the drain: the load is issued with the queue read and looked at after the bucket came
                    // back — no round trip of its own.  (Measured and not kept: read in front of every drain, 252.1 ms against 251.7.)
                    auto drain = [&](uint32_t n) __attribute__((always_inline)) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        qtail -= n; CF_DG(if (lane == 0) { ++dg[3]; dg[4] += n; })
                        bool made = false, park = false;
                        uint32_t hot = 0xFFFFFFFFu;
                        typename Tab::qitem it = 0;
                        const uint32_t fill = sh[0];
                        if constexpr (Tab::kDrainTwoProbes) {
                            // The 6-byte-slot, mask and region tables: up to 128 queued inserts, two per lane, their probes side by side in straight-line
                            // code (lanes past n: stale words of the queue) — two independent chains (queue word, bucket, claim, count) in flight per
                            // lane: the inserts are bound by that chain of LDS round trips at four waves per SIMD, not by instruction issue
                            // (profiles/r04_dist_phase_insts_after_cuts.md).  (Measured and not kept: one insert per lane through one straight-line
                            // probe, 110.8 ms against 108.0 on cenX-shaped reads, profiles/r06_dist_ab_cenx.log.)
                            bool made2 = false, park2 = false;
                            uint32_t hot2 = 0xFFFFFFFFu;
                            uint32_t xb, xd, xk, yb, yd, yk;
                            it = wq[qtail + (uint32_t)lane];
                            const typename Tab::qitem it2 = wq[qtail + 64u + (uint32_t)lane];
                            T.q_take(it, n_buckets, xb, xd, xk);
                            T.q_take(it2, n_buckets, yb, yd, yk);
                            uint32_t xbit = 0u, ybit = 0u;      // cf_tab_mask: the postings that brought the two pairs
                            if constexpr (Tab::kMaskTab) {
                                xbit = wqb[qtail + (uint32_t)lane] & 31u; ybit = wqb[qtail + 64u + (uint32_t)lane] & 31u;
                                T.probe2m((uint32_t)lane < n, xk, T.key_of(xb, xd), xbit, (uint32_t)lane + 64u < n, yk, T.key_of(yb, yd), ybit, A.min_cov, made, park, hot, made2, park2, hot2);
                            } else
                            T.probe2((uint32_t)lane < n, xk, T.key_of(xb, xd), (uint32_t)lane + 64u < n, yk, T.key_of(yb, yd), A.min_cov, made, park, hot, made2, park2, hot2);
                            const uint32_t n_new = (uint32_t)__popcll(cf_ballot(made)) + (uint32_t)__popcll(cf_ballot(made2));
                            if (n_new && lane == 0) atomicAdd(&sh[0], n_new);
                            const unsigned long long pm = cf_ballot(park), pm2 = cf_ballot(park2);
                            if (pm | pm2) {
                                if (park) { ovq[otail + cf_rank_in(pm)] = it; if constexpr (Tab::kMaskTab) ovqb[otail + cf_rank_in(pm)] = (uint8_t)xbit; }
                                otail += (uint32_t)__popcll(pm);
                                if (park2) { ovq[otail + cf_rank_in(pm2)] = it2; if constexpr (Tab::kMaskTab) ovqb[otail + cf_rank_in(pm2)] = (uint8_t)ybit; }
                                otail += (uint32_t)__popcll(pm2);
                            }
                            to_hot_list(hot);
                            to_hot_list(hot2);
                        } else {
                            // The 64-bit layouts: up to 64 queued inserts, one per lane, through nested match / claim branches (the drain of rounds 2-3)
                            if ((uint32_t)lane < n) {
                                uint32_t xb, xd, xk;
                                it = wq[qtail + (uint32_t)lane];
                                T.q_take(it, n_buckets, xb, xd, xk);
                                const typename Tab::bucket k = T.read(xk);
                                const int mt = T.match(k, xb, xd);
                                if (mt >= 0) { if (T.add(xk, mt) == A.min_cov) hot = Tab::kSlotsPerBucket * xk + (uint32_t)mt; }
                                else {
                                    const int em = Tab::empty(k);
                                    park = true;
                                    if (em >= 0) {
                                        uint32_t cn;
                                        const int st = T.claim_finish(T.claim_issue(xk, em, xb, xd), xk, em, xb, xd, cn);
                                        made = st == 0; park = st == 2;
                                        if (st != 2 && cn == A.min_cov) hot = Tab::kSlotsPerBucket * xk + (uint32_t)em;
                                    }
                                }
                            }
                            const uint32_t n_new = (uint32_t)__popcll(cf_ballot(made));
                            if (n_new && lane == 0) atomicAdd(&sh[0], n_new);
                            const unsigned long long pm = cf_ballot(park);
                            if (pm) {
                                if (park) ovq[otail + cf_rank_in(pm)] = it;
                                otail += (uint32_t)__popcll(pm);
                            }
                            to_hot_list(hot);
                        }
                        too_full = too_full || (uint32_t)__builtin_amdgcn_readfirstlane((int)fill) > A.fill_limit;
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    };
                    // takes the last m (<= 64) parked inserts, one per lane, through the probe loop (cf_dist_insert)
                    auto run_parked = [&](uint32_t m) __attribute__((always_inline)) {
                        otail -= m; CF_DG(if (lane == 0) { ++dg[1]; dg[2] += m; })
                        uint32_t made = 0, hot = 0xFFFFFFFFu;
                        if ((uint32_t)lane < m) {
                            uint32_t xb, xd, xk;
                            T.q_take(ovq[otail + (uint32_t)lane], n_buckets, xb, xd, xk);
                            uint32_t bit = 0u;
                            if constexpr (Tab::kMaskTab) bit = ovqb[otail + (uint32_t)lane] & 31u;
                            made = cf_dist_insert(T, n_buckets, xk, xb, xd, sh, A.min_cov, hot, CF_DG_PTR, bit);
                        }
                        const uint32_t n_new = (uint32_t)__popcll(cf_ballot(made != 0u));
                        if (n_new && lane == 0) atomicAdd(&sh[0], n_new);
                        to_hot_list(hot);
                    };
                    for (;;) {
                        if (too_full) break;      // (seen by the last drain; the limit leaves room for the drains of all waves that run meanwhile)
                        if (qtail >= lim) { CF_DG(const unsigned long long t1_ = __builtin_amdgcn_s_memtime();) drain(min(qtail, kDrain)); CF_DG(if (lane == 0) dg[6] += __builtin_amdgcn_s_memtime() - t1_;) }
                        else if (!(final && otail > 0u)) break;
                        while (otail >= 32u || (final && qtail == 0u && otail > 0u)) { CF_DG(const unsigned long long t0_ = __builtin_amdgcn_s_memtime();) run_parked(min(otail, 64u)); CF_DG(if (lane == 0) dg[5] += __builtin_amdgcn_s_memtime() - t0_;) }
                    }
                }, [&](const uint32_t (&bb)[DIST_UNROLL], const uint32_t (&dd_)[DIST_UNROLL], const uint32_t (&qq_)[DIST_UNROLL], const uint32_t (&lo_)[DIST_UNROLL], uint32_t ok, uint32_t len, uint32_t ib) -> bool {      // (ib: the posting's place in the group's union, wave-uniform; cf_tab_mask only)
                    if (too_full) return true;    // (wave-uniform, set by the drains: the fill only changes there) the pass will be split
                    // Entries equal to a itself are NOT told apart here (round 2 spent 13 vector instructions per step on it): they are
                    // rare (a k-mer twice in one read), the filter never selects a slot whose b is a, and the emission count of the
                    // launch has them subtracted on the host (cf_self_pairs_kernel counts them from the posting lists).
                    uint32_t w_[DIST_UNROLL];
#pragma unroll
                    for (int u = 0; u < DIST_UNROLL; ++u) w_[u] = bm[Tab::bm_bit(lo_[u]) >> 5];
                    // Entries that do not exist (only the last item of a posting has lanes past its end) or belong to another partition
                    // (only a first k-mer whose table was split) get an empty bitmap word, in two wave-uniform branches that are nearly
                    // never taken: the common path tests one bit per entry and nothing else.
                    if (len < DIST_ITEM) {
#pragma unroll
                        for (int u = 0; u < DIST_UNROLL; ++u) if (!((ok >> u) & 1u)) w_[u] = 0u;
                    }
                    if (pmask) {
                        uint32_t live = len < DIST_ITEM ? ok : (1u << DIST_UNROLL) - 1u;
#pragma unroll
                        for (int u = 0; u < DIST_UNROLL; ++u) {
                            const uint32_t hb = Tab::hash(bb[u]);
                            if ((((hb ^ (hb >> 15)) >> 3) & pmask) != pidx) { live &= ~(1u << u); w_[u] = 0u; }
                        }
                        my_e += (uint32_t)__popcll((unsigned long long)live);
                    }
                    s_e += pmask ? 0u : len;      // entries swept, counted on the scalar unit (an `else` here made the compiler keep both
                                                  // counters in a scratch array picked by index: a scratch load + store per step)
                    bool c_[DIST_UNROLL];
#pragma unroll
                    for (int u = 0; u < DIST_UNROLL; ++u) c_[u] = cf_bit_of(w_[u], lo_[u]) != 0u;
#pragma unroll
                    for (int u = 0; u < DIST_UNROLL; ++u) {
                        const unsigned long long cm = cf_ballot(c_[u]);
                        if (cm) {
                            if (c_[u]) {
                                const uint32_t at = qtail + cf_rank_in(cm);
                                wq[at] = T.q_push(bb[u], dd_[u], qq_[u], n_buckets);
                                if constexpr (Tab::kMaskTab) wqb[at] = (uint8_t)ib;      // (the parallel byte queue: which posting of the union brought the pair)
                            }
                            qtail += (uint32_t)__popcll(cm);
                        }
                    }
                    // (measured and not kept: every lane storing — candidates at their rank, the others into a dump word of their own —
                    // to save the four scalar instructions per entry of the skip branches and the exec save / restore: 325 vs 320 ms,
                    // the LDS takes four full-wave writes per step instead of 15 % of the lanes)
                    // (measured and not kept, round 5: the pushes flat — no test for "no candidate in the wave" (a compare of the ballot and a
                    // branch per entry slot), rank and queue word made by every lane, only the store under the mask: 255.1 ms against 251.7,
                    // profiles/r05_dist_ab_2.log)
                    return false;
                });
                CF_DG(if (lane == 0) dg[7] += __builtin_amdgcn_s_memtime() - t2_;)
                CF_STAMP(3);   // table sweep + inserts (wave 0's own items)
            }
            __syncthreads();      // [table swept]
            CF_STAMP(7);
            if (sh[0] > A.fill_limit) {  // overflow: split this partition in two, go on with one of the halves
                __syncthreads();      // (everyone has seen the fill level before thread 0 resets it)
                if (t == 0) {
                    uint32_t sp = sh[2];
                    if (P >= (1u << 20) || sp + 2 > DIST_STACK) { atomicOr(&A.counters[4], 1ull); }      // (the launch fails: -34)
                    else { stack[2 * sp] = 2 * P; stack[2 * sp + 1] = pidx; stack[2 * sp + 2] = 2 * P; stack[2 * sp + 3] = pidx + P; sh[2] = sp + 2; }
                    if (sh[2]) pop_pass(); else { publish_next(); sh[3] = 0; }      // (nothing left only after that error: on to the next first k-mer)
                }
                spilled = true;
                T.clear(slots, (uint32_t)t, (uint32_t)nt);
                __syncthreads();
                if (sh[3] == 0u) break;
                continue;
            }
            // ---- table of the pass complete: count emissions, filter in LDS (selected slots are marked and
            // staged), reserve the edge range with ONE global atomic, then write
            for (int d = 32; d >= 1; d >>= 1) my_e += __shfl_down(my_e, (unsigned)d);
            if (lane == 0 && (my_e + s_e)) atomicAdd(&sh[7], my_e + s_e);
            if (t == 0 && sh[2] == 0u) publish_next();      // the last pass: the next first k-mer's head rides on the filter's barrier
            // Filter in two steps.  (1) A group of slots per thread and round: the slots whose count reaches min_cov (few: the
            // table is sparse and most pairs stay below) are compacted into a list that lies over the insert queues, dead
            // by now.  (2) The list is evaluated one slot per thread with all lanes busy: sum over d from the bucket's
            // registers or a chain walk, the double division, mark + stage.  (Evaluating inside the bucket scan ran the
            // division code at 8 unrolled sites per round with 4 % of the lanes active: 9 100 cycles per first k-mer.)
            // The slots to evaluate: the list the insert path made (slots whose count reached min_cov) — or, when that list
            // overflowed / min_cov < 2 / a test asks for it, a scan of the whole table into a list over the insert queues.
            uint16_t* hot = hotl;
            uint32_t hot_cap = min(A.hot_cap, DIST_HOT_CAP);
            const bool from_inserts = use_hot && A.min_cov >= 2u && sh[11] <= hot_cap;      // (uniform: nothing changes sh[11] after the sweep's barrier)
            const unsigned long long lt = (1ull << lane) - 1ull;
            if (!from_inserts) {
            if (use_hot) {      // (a first k-mer that kept no list — round 6 — finds the cursor as the pass's set-up left it, 0: the inserts only move it when they keep the list; two barriers less)
            __syncthreads();
            if (t == 0) sh[11] = 0;
            __syncthreads();
            }
            hot = (uint16_t*)wq0;
            hot_cap = min(A.hot_cap, (uint32_t)((size_t)(nt >> 6) * DIST_QCAP * sizeof(typename Tab::qitem) / 2));
            const uint32_t n_groups = slots / Tab::kScanGroup;
            for (uint32_t g0 = 0; g0 < n_groups; g0 += (uint32_t)nt) {      // (uniform trip count: ballots inside)
                const uint32_t bk = g0 + (uint32_t)t;                       // a group of kScanGroup consecutive slots
                const uint32_t m = bk < n_groups ? T.hot_mask(bk, A.min_cov) : 0u;
                const uint32_t cnt = (uint32_t)__popc(m);
                if (cf_ballot(cnt != 0u)) {
                    // positions in the list: lanes hand in their k-th hot slot in round k (most lanes have none, few have
                    // two: one or two rounds, against eight ballots — one per slot of the group — before)
                    uint32_t total = 0;
                    for (uint32_t k = 0; k < Tab::kScanGroup; ++k) { const unsigned long long bk_ = cf_ballot(cnt > k); if (!bk_) break; total += (uint32_t)__popcll(bk_); }
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(&sh[11], total);
                    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                    uint32_t mm = m;
                    for (uint32_t k = 0; k < Tab::kScanGroup; ++k) {
                        const unsigned long long bk_ = cf_ballot(cnt > k);
                        if (!bk_) break;
                        if (cnt > k) {
                            const uint32_t bit = (uint32_t)__ffs((int)mm) - 1u;
                            mm &= mm - 1u;
                            const uint32_t pos = base + cf_rank_in(bk_);
                            if (pos < hot_cap) hot[pos] = (uint16_t)(Tab::kScanGroup * bk + Tab::slot_of_bit(bit));
                        }
                        base += (uint32_t)__popcll(bk_);
                    }
                }
            }
            __syncthreads();
            }
            const uint32_t n_hot = sh[11];
            // cnt / total >= thr as Python evaluates it (distance_based_kmer_recruitment.py:143-144: true division of two ints, compared
            // with a double).  For the default threshold — the literal 0.8, the double just above 4 / 5 — the test is exactly
            // 5 cnt >= 4 total: a quotient below 4 / 5 lies at least 1 / (5 total) below it, far more than an ulp for any total < 2^40,
            // and 4 / 5 itself rounds to the literal.  Other thresholds take the double division (about 40 instructions).
            auto dominant = [&](uint32_t cnt, unsigned long long total) -> bool {
                if (A.thr_den) return (unsigned long long)A.thr_den * cnt >= (unsigned long long)A.thr_num * total;
                return ((double)cnt / (double)total) >= A.thr;
            };
            // A selected edge takes its row of the output right here: the workgroup's chunk (DIST_EDGE_CHUNK rows reserved with
            // one global atomic; base in sh[28,29], rows in sh[27], cursor sh[26]) hands out rows through an LDS atomic per wave
            // and round, and the lane that evaluated the slot writes the row from its registers.  Only an edge whose row does not
            // fit the rest of the chunk is marked and staged (count sh[30]); those are written behind a barrier, after thread 0 has
            // reserved the next chunk.  (The first half of round 3 staged EVERY selected slot, met at a barrier for thread 0 to
            // hand out the rows and read the slots again: the write phase was 9 % of the kernel.)
            // The table of the pass is the table of EVERY member of the class (cnt(a, b, d) depends on a only through its posting list): from here
            // to [rows reserved] the pass runs once per member a_j = order[first_member + j] — the same slots, the same totals, `b != a_j` and the
            // row's first column its own.  sh[8] counts the selected rows of all members so far (nobody resets it between members: a member's
            // share is the difference); a class of one takes exactly the path and the barriers of a first k-mer without classes.
            uint32_t sel_prev = 0, sp_left = 0;
            CF_DG(if (t == 0) { dg_hot += n_hot; dg_hot_mem += (unsigned long long)n_hot * n_mem; })
            bool once = false;
            // (uniform.  The layout's constant at the END of the condition repeats the `if constexpr` on purpose: without that term the compiler folds
            // the compare into the two paths that join above — 7 instructions and one SGPR spill more in the mask kernels)
            if constexpr (Tab::kMaskTab) once = A.filter_once != 0u && n_hot <= hot_cap && Tab::kMaskTab;
            if constexpr (Tab::kMaskTab) if (once) {
                // ---- every member of the group in ONE section.  The loops of the member loop below are inverted: a thread takes a hot
                // slot, reads its bucket and the masks of every key of its b ONCE (from the bucket's registers, or one chain walk where eval_slot
                // walks) and then loops over the members in registers — cnt = cnt_of(mine & M_j), total = sum of cnt_of(w_k & M_j).  The members of a
                // batch of 32 arrive with one coalesced load (lane j: M_j and a_j) and are handed out with v_readlane: scalar per member, no wait
                // inside the loop.  Rows are reserved per batch: a lane keeps its selections as a bit per member, a wave takes its range with one
                // returning LDS add, and behind ONE barrier everyone knows the batch's total; only when the rows pass the end of the workgroup's
                // chunk does thread 0 reserve the next chunk(s) behind a second barrier — rows below the chunk's remainder go to the old chunk,
                // the others into the new reservation.  No marks, no stage list, no marked-slot sweep.
                // cw[n % 3]: rows of batch n, cw[3 + n % 3]: its members with a row.  Three words each in turn: thread 0 clears the words of batch
                // n + 1 in front of barrier n (their last readers, of batch n - 2, are past barrier n - 1), and a wave that runs ahead into batch n + 1
                // never touches the words the slow ones still read.  (The words lie at the head of the stage list, which this path does not use.)
                uint32_t* cw = (uint32_t*)stage;
                unsigned long long ch_base = ((unsigned long long)sh[29] << 32) | sh[28];
                uint32_t ch_rows = sh[27], cur = sh[26], batch = 0;      // (uniform: the chunk, and the cursor in it, are kept in registers through the section; batch 0's words cw[0], cw[3] were cleared by thread 0 at the top of the pass loop, in front of [table swept])
                const bool counting = T.counting;
                auto cntf = [&](uint32_t w, uint32_t M) -> uint32_t { return counting ? w : (uint32_t)__popc(w & M); };
                bool p_on = false;      // the previous batch's b of this lane: its unique-mask word is on its way
                uint32_t p_w = 0, p_b = 0;
                auto set_unique = [&](uint32_t w, uint32_t b) { const uint32_t bit = 1u << (b & 31); if (!(w & bit)) atomicOr(&A.unique_bits[b >> 5], bit); };
                for (uint32_t i0 = 0; i0 < n_hot; i0 += (uint32_t)nt) {      // (one round whenever the list is no longer than the workgroup)
                    const uint32_t i = i0 + (uint32_t)t;
                    bool act = false, ovf = false;
                    uint32_t b = 0, dd = 0, mine_m = 0, s = 0xFFFFu;
                    uint32_t w[DIST_MEMBER_KEYS];
#pragma unroll
                    for (int q = 0; q < DIST_MEMBER_KEYS; ++q) w[q] = 0u;
                    if (i < n_hot) s = hot[i];
                    if (s != 0xFFFFu) {      // (0xFFFF: no entry of the list for this thread)
                        const uint32_t bk = s >> 2, si = s & 3u;
                        const typename Tab::bucket k = T.read(bk);
                        const typename Tab::masks m = T.read_masks(bk);
                        uint32_t mine = k.k[0];
                        mine_m = m.w[0];
#pragma unroll
                        for (int j = 1; j < 4; ++j) { if (si == (uint32_t)j) { mine = k.k[j]; mine_m = m.w[j]; } }
                        if (mine != Tab::kEmpty && T.all_of(mine_m) >= A.min_cov) {      // (no member counts more than the union)
                            act = true; b = mine & Tab::kBMask; dd = mine >> Tab::kBBits;
                            if (k.k[3] == Tab::kEmpty && Tab::N::home(Tab::N::hash(b), n_buckets) == bk) {      // eval_slot's rule: every key of b is in this bucket
#pragma unroll
                                for (int j = 0; j < 4; ++j) w[j] = ((k.k[j] & Tab::kBMask) == b && k.k[j] != Tab::kEmpty) ? m.w[j] : 0u;
                            } else {      // one walk of b's chain: the masks of its keys into registers, the first DIST_MEMBER_KEYS of them
                                uint32_t n_w = 0, cb = Tab::N::home(Tab::N::hash(b), n_buckets);
                                for (uint32_t probe = 0; probe < n_buckets; ++probe) {
                                    const typename Tab::bucket k2 = T.read(cb);
                                    CF_DG(++dg_walk_bk;)
                                    const typename Tab::masks m2 = T.read_masks(cb);
#pragma unroll
                                    for (int j = 0; j < 4; ++j)
                                        if ((k2.k[j] & Tab::kBMask) == b && k2.k[j] != Tab::kEmpty) {
#pragma unroll
                                            for (int q = 0; q < DIST_MEMBER_KEYS; ++q) w[q] = n_w == (uint32_t)q ? m2.w[j] : w[q];
                                            ++n_w;
                                        }
                                    if (k2.k[3] == Tab::kEmpty) break;
                                    cb = cb + 1 == n_buckets ? 0u : cb + 1;
                                }
                                ovf = n_w > (uint32_t)DIST_MEMBER_KEYS;      // more keys than registers: this slot walks the chain per member (slow, rare)
                                CF_DG(++dg_walks; dg_ovf += (unsigned long long)ovf;)
                            }
                        }
                    }
                    for (uint32_t j0 = 0; j0 < n_mem; j0 += 32u, ++batch) {      // (uniform) the members, 32 at a time: a bit each in `selbits`
                        const uint32_t nbm = min(32u, n_mem - j0), c = batch % 3u, cn = (batch + 1u) % 3u;
                        uint32_t Mv = 0, Av = 0;
                        if ((uint32_t)lane < nbm) { Mv = A.member_mask[(size_t)m_first + j0 + (uint32_t)lane]; Av = (j0 + (uint32_t)lane) ? (uint32_t)A.order[(size_t)m_first + j0 + (uint32_t)lane] : a; }
                        uint32_t selbits = 0, wave_n = 0, wave_mem = 0;
                        for (uint32_t jj = 0; jj < nbm; ++jj) {
                            const uint32_t M = (uint32_t)__builtin_amdgcn_readlane((int)Mv, (int)jj), aj = (uint32_t)__builtin_amdgcn_readlane((int)Av, (int)jj);
                            const uint32_t cnt = cntf(mine_m, M);
                            bool sel = false;
                            if (act && cnt >= A.min_cov && b != aj) {
                                unsigned long long total = 0;
                                if (ovf) { T.set_member(M, counting); total = T.total_of(b, n_buckets); }
                                else {
#pragma unroll
                                    for (int q = 0; q < DIST_MEMBER_KEYS; ++q) total += cntf(w[q], M);
                                }
                                sel = dominant(cnt, total);
                            }
                            const unsigned long long bal = cf_ballot(sel);
                            selbits |= (uint32_t)sel << jj;
                            wave_n += (uint32_t)__popcll(bal);
                            wave_mem |= (uint32_t)(bal != 0ull) << jj;
                        }
                        uint32_t rel0 = 0;
                        if (lane == 0 && wave_n) { rel0 = atomicAdd(&cw[c], wave_n); atomicOr(&cw[3u + c], wave_mem); }
                        if (t == 0) { cw[cn] = 0u; cw[3u + cn] = 0u; }
                        __syncthreads();      // [batch counted]
                        rel0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)rel0);
                        const uint32_t tot = cw[c], end = cur + tot;
                        unsigned long long nbase = 0;
                        if (end > ch_rows) {      // (uniform; once per chunk) the rows pass the end of the chunk: thread 0 reserves what is missing, in whole chunks
                            if (t == 0) {
                                const unsigned long long take = ((unsigned long long)(end - ch_rows) + A.edge_chunk - 1ull) / A.edge_chunk * A.edge_chunk;
                                const unsigned long long nb = atomicAdd(&A.counters[0], take);
                                sh[28] = (uint32_t)nb; sh[29] = (uint32_t)(nb >> 32); sh[27] = (uint32_t)take;
                            }
                            __syncthreads();      // [rows reserved]
                            nbase = ((unsigned long long)sh[29] << 32) | sh[28];
                        }
                        // a member has rows when any wave selected something for it: its unique bit (thread j of the batch, which holds a_j) and the edge count
                        if ((uint32_t)t < nbm && ((cw[3u + c] >> t) & 1u)) atomicOr(&A.unique_bits[Av >> 5], 1u << (Av & 31u));
                        if (t == 0) acc_edges += tot;
                        if (wave_n) {      // (wave-uniform) the rows, member by member, from registers
                            uint32_t run = cur + rel0;
                            for (uint32_t jj = 0; jj < nbm; ++jj) {
                                const bool bit = ((selbits >> jj) & 1u) != 0u;
                                const unsigned long long bal = cf_ballot(bit);
                                if (!bal) continue;
                                const uint32_t M = (uint32_t)__builtin_amdgcn_readlane((int)Mv, (int)jj), aj = (uint32_t)__builtin_amdgcn_readlane((int)Av, (int)jj);      // (by the whole wave)
                                if (bit) {
                                    const uint32_t r = run + (uint32_t)__popcll(bal & lt);
                                    const unsigned long long o = r < ch_rows ? ch_base + r : nbase + (r - ch_rows);
                                    if (o < A.edge_cap) *(cf_u32x4*)(A.edges + 4 * o) = cf_u32x4{dd, aj, b, cntf(mine_m, M)};
                                }
                                run += (uint32_t)__popcll(bal);
                            }
                        }
                        // b's unique bit once per lane and batch, whatever the number of its rows: the word is requested here and looked at a batch later
                        if (p_on) set_unique(p_w, p_b);
                        p_on = selbits != 0u;
                        if (p_on) { p_w = A.unique_bits[b >> 5]; p_b = b; }
                        if (end > ch_rows) { cur = end - ch_rows; ch_base = nbase; ch_rows = sh[27]; } else cur = end;
                    }
                }
                if (p_on) set_unique(p_w, p_b);      // (the one exposed wait of the group)
                // A pass without a hot slot has met no barrier in this section, and the next first k-mer's head (publish_next above, thread 0)
                // reaches the other waves only behind one: without it a wave that runs ahead reads the OLD head at the top of the loop and
                // goes through this first k-mer again, out of step with the workgroup.  (The member loop below has its [filtered] per member.)
                if (n_hot == 0u) __syncthreads();
                sp_left = sh[2];      // partitions still on the stack (thread 0 changes the word only behind the next barrier)
                if (t == 0) {
                    sh[26] = cur; sh[27] = ch_rows;      // (sh[28, 29] follow every reservation)
                    ++acc_pass; CF_DG(dg_swept += sh[7];)
                }
                CF_STAMP(4);   // filter (all members, rows included)
            }
            if (!once)
            for (uint32_t mj = 0; mj < n_mem; ++mj) {
                const uint32_t am = mj ? (uint32_t)A.order[(size_t)m_first + mj] : a;
                if constexpr (Tab::kMaskTab) T.set_member(A.member_mask[(size_t)m_first + mj], T.counting);      // the member's own postings among the union's
                const unsigned long long ch_base = ((unsigned long long)sh[29] << 32) | sh[28];
                const uint32_t ch_rows = sh[27];
                auto put_row = [&](unsigned long long o, uint32_t b, uint32_t dd, uint32_t cnt) {
                    if (o < A.edge_cap) *(cf_u32x4*)(A.edges + 4 * o) = cf_u32x4{dd, am, b, cnt};
                    const uint32_t bit = 1u << (b & 31);
                    if (!(A.unique_bits[b >> 5] & bit)) atomicOr(&A.unique_bits[b >> 5], bit);
                };
                // the same in two halves (round 6): the row is stored and the word of b's unique bit REQUESTED; the bit is looked at — and set
                // when it is not — a round of the filter later.  A first k-mer of cenX-shaped reads has ~3 500 selected edges: four rounds
                // of the list per thread, each of which waited for its own round trip to the unique mask (18 % of the kernel by thread 0's stamps).
                auto set_unique = [&](uint32_t w, uint32_t b) { const uint32_t bit = 1u << (b & 31); if (!(w & bit)) atomicOr(&A.unique_bits[b >> 5], bit); };
                // called by all lanes of a wave together; true for the lanes whose edge got its row here (the others': behind the barrier below)
                auto keep = [&](bool sel, uint32_t s, uint32_t b, uint32_t dd, uint32_t cnt) -> bool {
                    const unsigned long long m = cf_ballot(sel);
                    if (!m) return false;
                    uint32_t row0 = 0;
                    if (lane == 0) { const uint32_t n = (uint32_t)__popcll(m); atomicAdd(&sh[8], n); row0 = atomicAdd(&sh[26], n); }
                    const uint32_t row = (uint32_t)__builtin_amdgcn_readfirstlane((int)row0) + (uint32_t)__popcll(m & lt);
                    const bool late = sel && row >= ch_rows;
                    const unsigned long long o = ch_base + row;
                    if (sel && !late && o < A.edge_cap) *(cf_u32x4*)(A.edges + 4 * o) = cf_u32x4{dd, am, b, cnt};
                    const unsigned long long ml = cf_ballot(late);
                    if (ml) {
                        uint32_t p0 = 0;
                        if (lane == 0) p0 = atomicAdd(&sh[30], (uint32_t)__popcll(ml));
                        const uint32_t pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)p0) + (uint32_t)__popcll(ml & lt);
                        if (late) { T.mark(s); if (pos < A.stage_cap) stage[pos] = (uint16_t)s; }
                    }
                    return sel && !late;
                };
                if (n_hot <= hot_cap) {
                    bool p_on = false;      // the previous round's edge of this lane: its unique-mask word is on its way
                    uint32_t p_w = 0, p_b = 0;
                    for (uint32_t i0 = 0; i0 < n_hot; i0 += (uint32_t)nt) {
                        const uint32_t i = i0 + (uint32_t)t;
                        bool sel = false;
                        uint32_t s = 0, eb = 0, ed = 0, ec = 0;
                        if (i < n_hot && (s = hot[i]) != 0xFFFFu) {      // (0xFFFF: no slot, as in the one-section filter above; neither the inserts nor the scan write it)
                            if constexpr (Tab::kMaskTab) { CF_DG(const uint32_t wb_ = T.diag_walk(s, n_buckets, A.min_cov); dg_walks += (unsigned long long)(wb_ != 0u); dg_walk_bk += wb_;) }
                            T.eval_slot(s, n_buckets, A.min_cov, [&](uint32_t, uint32_t b, uint32_t dd, uint32_t cnt, unsigned long long total) { sel = b != am && dominant(cnt, total); eb = b; ed = dd; ec = cnt; });
                        }
                        const bool wrote = keep(sel, s, eb, ed, ec);
                        uint32_t w_new = 0;
                        if (wrote) w_new = A.unique_bits[eb >> 5];
                        if (p_on) set_unique(p_w, p_b);
                        p_on = wrote; p_w = w_new; p_b = eb;
                    }
                    if (p_on) set_unique(p_w, p_b);
                } else {        // more than the list holds (never seen with the sketch): evaluate inside the bucket scan, a row per atomic
                    for (uint32_t bk = (uint32_t)t; bk < n_buckets; bk += (uint32_t)nt)
                        T.for_counts_at_least(bk, n_buckets, A.min_cov, [&](uint32_t s, uint32_t b, uint32_t dd, uint32_t cnt, unsigned long long total) {
                            if (b != am && dominant(cnt, total)) {
                                atomicAdd(&sh[8], 1u);
                                const uint32_t row = atomicAdd(&sh[26], 1u);
                                if (row < ch_rows) put_row(ch_base + row, b, dd, cnt);
                                else {
                                    T.mark(s);
                                    const uint32_t pos = atomicAdd(&sh[30], 1u);
                                    if (pos < A.stage_cap) stage[pos] = (uint16_t)s;
                                }
                            }
                        });
                }
                __syncthreads();      // [filtered]
                CF_STAMP(4);   // filter
                const uint32_t n_sel = sh[8] - sel_prev, n_late = sh[30];
                sel_prev += n_sel;
                sp_left = sh[2];      // partitions still on the stack (thread 0 changes the word only behind the next barrier)
                if (t == 0) {
                    acc_E += sh[7];      // (the reference sweeps the pass's entries once per member)
                    if (mj == 0u) { ++acc_pass; CF_DG(dg_swept += sh[7];) }
                    if (n_sel) { acc_edges += n_sel; atomicOr(&A.unique_bits[am >> 5], 1u << (am & 31)); }      // (fire and forget: a load to test the bit first would stall thread 0)
                }
                if (n_late) {      // (uniform; once per DIST_EDGE_CHUNK rows) the chunk is full: the late rows open the next one
                    __syncthreads();      // everyone has read the chunk and the counts
                    if (t == 0) {
                        const unsigned long long take = ((unsigned long long)n_late + A.edge_chunk - 1ull) / A.edge_chunk * A.edge_chunk;
                        const unsigned long long nb = atomicAdd(&A.counters[0], take);
                        sh[28] = (uint32_t)nb; sh[29] = (uint32_t)(nb >> 32); sh[27] = (uint32_t)take; sh[26] = n_late;
                        sh[30] = 0; sh[13] = 0;      // ([13]: cursor of the marked-slot sweep below; the sketch's flag is long read)
                    }
                    __syncthreads();      // [rows reserved]
                    const unsigned long long nbase = ((unsigned long long)sh[29] << 32) | sh[28];
                    if (n_late <= A.stage_cap) {           // the staged slot list
                        for (uint32_t i = (uint32_t)t; i < n_late; i += (uint32_t)nt) {
                            uint32_t b, dd, cnt;
                            if (T.get(stage[i], b, dd, cnt)) put_row(nbase + i, b, dd, cnt);
                        }
                    } else {                               // more late edges than the stage holds: sweep the marked slots, a bucket per thread
                        for (uint32_t bk = (uint32_t)t; bk < n_buckets; bk += (uint32_t)nt)
                            T.for_marked(bk, [&](uint32_t, uint32_t b, uint32_t dd, uint32_t cnt) { put_row(nbase + atomicAdd(&sh[13], 1u), b, dd, cnt); });
                    }
                }
                if (mj + 1u < n_mem) {      // (uniform) the next member filters the same table
                    __syncthreads();      // everyone has read this member's counts and chunk, and its late rows are out of the table
                    if (n_late) {         // (uniform) its marks go: the next member's marked-slot sweep must find its own only
                        for (uint32_t bk = (uint32_t)t; bk < n_buckets; bk += (uint32_t)nt) T.for_marked(bk, [&](uint32_t s, uint32_t, uint32_t, uint32_t) { T.unmark(s); });
                        __syncthreads();
                    }
                }
            }      // (members)
            CF_STAMP(5);   // reserve + write edges
            if (sp_left == 0u) break;
            __syncthreads();      // (more partitions) the rows are out of the table before it is cleared for the next one
            if (t == 0) pop_pass();
            T.clear(slots, (uint32_t)t, (uint32_t)nt);
            __syncthreads();
        }
        if (spilled && t == 0) ++acc_spill;
    }
    if (t == 0) {
        if (acc_E && !Tab::kMaskTab) atomicAdd(&A.counters[1], acc_E);      // (groups: the members' own partner entries were summed by cf_group_walk_kernel; what a pass sweeps is the union's)
        if (acc_spill) atomicAdd(&A.counters[2], acc_spill);
        if (acc_pass) atomicAdd(&A.counters[5], acc_pass);
        if (acc_edges) atomicAdd(&A.counters[6], acc_edges);
        if (sh[27] > sh[26]) {      // the unused rest of the last chunk: a hole for cf_edge_compact_kernel
            const unsigned long long h = atomicAdd(&A.counters[7], 1ull), cb = ((unsigned long long)sh[29] << 32) | sh[28];
            A.holes[2 * h] = cb + sh[26]; A.holes[2 * h + 1] = (unsigned long long)(sh[27] - sh[26]);
        }
#if defined(CF_DIST_STAMPS)
        for (int i = 0; i < 8; ++i) atomicAdd(&A.counters[8 + i], stamp_acc[i]);
#endif
    }
#if defined(CF_DIST_DIAG_COUNT)
    for (int i = 0; i < 8; ++i) if (dg[i]) atomicAdd(&A.counters[8 + i], dg[i]);
    if (t == 0 && dg_swept) atomicAdd(&A.counters[147], dg_swept);
    for (int d = 32; d >= 1; d >>= 1) { dg_walks += __shfl_down(dg_walks, (unsigned)d); dg_walk_bk += __shfl_down(dg_walk_bk, (unsigned)d); dg_ovf += __shfl_down(dg_ovf, (unsigned)d); }
    if (lane == 0 && dg_walks) { atomicAdd(&A.counters[154], dg_walks); atomicAdd(&A.counters[155], dg_walk_bk); if (dg_ovf) atomicAdd(&A.counters[156], dg_ovf); }
    if (t == 0 && dg_hot) { atomicAdd(&A.counters[152], dg_hot); atomicAdd(&A.counters[153], dg_hot_mem); }
#endif
}

__global__ void __launch_bounds__(256)
cf_max_u32_kernel(const uint32_t* __restrict__ v, int64_t n, uint32_t* __restrict__ out) {
    uint32_t m = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) m = max(m, v[i]);
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_down(m, (unsigned)d));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

// Closes the holes of the chunked edge output: row k of the move list goes from the k-th valid row at or above n_valid to the k-th
// hole row below it (segment lists with inclusive prefixes, built on the host from the <= grid holes of the kernel).
__global__ void __launch_bounds__(256)
cf_edge_compact_kernel(uint32_t* __restrict__ edges, const unsigned long long* __restrict__ src_start, const unsigned long long* __restrict__ src_pre, int n_src,
                       const unsigned long long* __restrict__ dst_start, const unsigned long long* __restrict__ dst_pre, int n_dst, unsigned long long n_move) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_move; k += stride) {
        int lo = 0, hi = n_src - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (src_pre[mid] > k) hi = mid; else lo = mid + 1; }
        const unsigned long long from = src_start[lo] + (k - (lo ? src_pre[lo - 1] : 0ull));
        lo = 0; hi = n_dst - 1;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (dst_pre[mid] > k) hi = mid; else lo = mid + 1; }
        const unsigned long long to = dst_start[lo] + (k - (lo ? dst_pre[lo - 1] : 0ull));
        *(cf_u32x4*)(edges + 4 * to) = *(const cf_u32x4*)(edges + 4 * from);
    }
}

// order-independent checksum of stored edges: sum over rows of mix(d, a, b, cnt) mod 2^64 (the oracle's edge checksum:
// tests compare all 3e9 edges of a full-size run without copying 50 GB to the host)
__global__ void __launch_bounds__(256)
cf_edge_checksum_kernel(const uint32_t* __restrict__ edges, int64_t n, unsigned long long* __restrict__ out) {
    unsigned long long s = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const cf_u32x4 e = *(const cf_u32x4*)(edges + 4 * i);
        s += cf_mix64(cf_mix64(cf_mix64(cf_mix64((unsigned long long)e.x + 0x9E37ull) ^ (unsigned long long)e.y) ^ ((unsigned long long)e.z << 1)) ^ ((unsigned long long)e.w << 2));
    }
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, (unsigned)d);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, s);
}

extern "C" {

int cf_edges_checksum(cf_ctx* ctx, int64_t n, uint64_t* out) {
    if (!ctx || !out) return -22;
    *out = 0;
    n = std::min(n, ctx->n_edges_stored);
    if (n <= 0) return 0;
    CF_HIP(hipSetDevice(ctx->device));
    cf_scratch tmp(ctx);
    unsigned long long* d_sum = nullptr;
    CF_TRY(tmp.get(&d_sum, 1, "edge checksum"));
    unsigned long long h = 0;
    CF_HIP(hipMemsetAsync(d_sum, 0, 8, ctx->stream));
    hipLaunchKernelGGL(cf_edge_checksum_kernel, dim3((unsigned)cf_grid_for(n, 256, std::max(1, ctx->n_cu) * 16)), dim3(256), 0, ctx->stream,
                       (const uint32_t*)ctx->d_edges, n, d_sum);
    CF_KERNEL_CHECK("cf_edge_checksum_kernel");
    CF_HIP(hipMemcpyAsync(&h, d_sum, 8, hipMemcpyDeviceToHost, ctx->stream));
    CF_HIP(hipStreamSynchronize(ctx->stream));
    *out = (uint64_t)h;
    return 0;
}

int cf_dist_edges(cf_ctx* ctx, int64_t min_n, int64_t max_n, int32_t min_d, int32_t max_d, uint32_t min_cov,
                  double rel_threshold, int32_t part, int32_t n_parts, int64_t edge_cap, int64_t* n_edges) {
    if (!ctx) return -22;
    // A call that fails leaves no launch behind (cfhip.h): no stored edge, and not the counters of the last launch that succeeded
    ctx->n_edges_stored = 0;
    ctx->stats.n_edges = 0; ctx->stats.n_emissions = 0; ctx->stats.n_spilled = 0; ctx->stats.n_dist_passes = 0;
    if (!ctx->have_clouds && !ctx->have_gview) return cf_fail(ctx, -22, "cf_dist_edges: no clouds built");
    // the clouds the stage works on: the all-gathered ones of every rank (multi-GPU) or the local ones
    const bool gv = ctx->have_gview;
    const int64_t* v_unit_ptr = gv ? ctx->g_unit_ptr : ctx->d_unit_ptr;
    const int64_t* v_cloud_ptr = gv ? ctx->g_cloud_ptr : ctx->d_cloud_ptr;
    const int32_t* v_entries = gv ? ctx->g_entries_d : ctx->d_entries;
    const std::vector<int64_t>& v_h_unit_ptr = gv ? ctx->g_h_unit_ptr : ctx->h_unit_ptr;
    const int64_t v_n_entries = gv ? ctx->g_entries : ctx->n_entries;
    if (n_parts < 1 || part < 0 || part >= n_parts) return cf_fail(ctx, -22, "cf_dist_edges: bad partition");
    if (max_d > 65535) return cf_fail(ctx, -22, "cf_dist_edges: max_d > 65535 does not fit the 16-bit distance field");
    if (v_n_entries >= ((int64_t)1 << 32) - 8 * (int64_t)DIST_ITEM) return cf_fail(ctx, -34, "cf_dist_edges: more than 2^32 cloud entries (the sweeps address them with 32-bit indices)");
    if (edge_cap < 0) edge_cap = 0;
    const int64_t R = gv ? ctx->g_reads : ctx->n_reads, U = gv ? ctx->g_units : ctx->n_units, K = ctx->n_kmers;
    // (no limit on the units of a read: unit indices travel mod 256 / mod 65536 and a difference <= max_d is exact)
    CF_HIP(hipSetDevice(ctx->device));
    CF_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    // Python slice semantics of itertools.islice(items, min_n, max_n) for non-negative bounds
    if (min_n < 0) min_n = 0;
    if (max_n > R) max_n = R;
    if (max_n < min_n) max_n = min_n;
    if (min_n > R) min_n = R;
    const int64_t u0 = v_h_unit_ptr[(size_t)min_n], u1 = v_h_unit_ptr[(size_t)max_n];
    const int32_t min_d_eff = min_d < 1 ? 1 : min_d;  // kmer_clouds[:-0] is empty: d = 0 emits nothing

    uint32_t *d_pcnt = nullptr, *d_cursor = nullptr, *d_first = nullptr;
    unsigned long long *d_okeys = nullptr, *d_otmp = nullptr;
    int32_t* d_order = nullptr;
    int64_t n_order = 0, n_item_slots = 0;
    uint32_t *d_icnt = nullptr, *d_ialloc = nullptr;
    int64_t* d_ibase = nullptr;
    cf_dist_head* d_heads = nullptr;
    cf_dist_item* d_items = nullptr;
    unsigned long long* d_holes = nullptr;
    int64_t n_stored = 0;
    int64_t* d_post_ptr = nullptr;
    int32_t *d_post = nullptr, *d_rend = nullptr, *d_rbeg = nullptr;
    uint16_t* d_entry_i = nullptr;
    uint32_t* d_packed = nullptr;
    cf_dist_rec* d_urange = nullptr;
    bool narrow = false, wide16 = false, region = false, region26 = false;
    int narrow_db = 8, reg_shift = 0;
    uint8_t* d_entry_i8 = nullptr;
    unsigned long long* d_cnt = nullptr;
    int64_t n_post = 0;
    unsigned long long h_cnt[8] = {0};
    const size_t n_cnt = 8 + 16 * 9 + 5;   // counters + 8 queue heads on their own cache lines; [144] a cloud row is not a set (cf_entry_unit_kernel) [145, 146] diagnostic build: useful items, items [147] entries swept once per class [148] postings of the groups' unions [149] classes inside the groups [152..155] the member filter: hot slots, hot slots x members, evaluations that walked the chain, buckets read there [156] hot slots of the one-section filter whose b has more than DIST_MEMBER_KEYS keys
    const int max_blocks = std::max(1, ctx->n_cu) * 8;
    cf_free_edges(ctx);      // (the buffer of this call is allocated below, once the launch shape is known)
    cf_scratch tmp(ctx);
    CF_TRY(tmp.get(&d_pcnt, (size_t)K + 1, "posting counts"));
    CF_TRY(tmp.get(&d_cursor, (size_t)K + 1, "posting cursors"));
    CF_TRY(tmp.get(&d_post_ptr, (size_t)K + 1, "posting offsets"));
    CF_TRY(tmp.get(&d_rend, (size_t)U + 1, "unit read ends"));
    CF_TRY(tmp.get(&d_rbeg, (size_t)U + 1, "unit read begins"));
    CF_TRY(tmp.get(&d_urange, (size_t)U + 1, "unit partner ranges"));
    CF_TRY(tmp.get(&d_cnt, n_cnt, "dist counters"));
    CF_TRY(tmp.get(&d_first, (size_t)K + 1, "first posting units"));
    CF_HIP(hipMemsetAsync(d_pcnt, 0, (size_t)(K + 1) * 4, ctx->stream));
    CF_HIP(hipMemsetAsync(d_cursor, 0, (size_t)(K + 1) * 4, ctx->stream));
    CF_HIP(hipMemsetAsync(d_cnt, 0, n_cnt * 8, ctx->stream));
    CF_HIP(hipMemsetAsync(d_first, 0xFF, (size_t)(K + 1) * 4, ctx->stream));
    int64_t e0 = 0, e1 = 0;
    CF_HIP(hipMemcpy(&e0, v_cloud_ptr + u0, 8, hipMemcpyDeviceToHost));
    CF_HIP(hipMemcpy(&e1, v_cloud_ptr + u1, 8, hipMemcpyDeviceToHost));
    const bool by_sort = !ctx->dist_post_atomics && e1 > e0 && (e1 - e0) < ((int64_t)1 << 32) && U < ((int64_t)1 << 31);
    if (by_sort) {
        int64_t n = e1 - e0;
        const int64_t K_part = (K + n_parts - 1) / n_parts;      // sort keys: the rank, or rank / n_parts for one partition
        int kb = 1; while (kb < 32 && ((int64_t)1 << kb) < std::max<int64_t>(K_part, 2)) ++kb;
        kb = (kb + 7) & ~7;      // whole 8-bit digits: the last radix pass must not reach into the unit bits
        const unsigned g_units = (unsigned)cf_grid_for((u1 - u0) * 64, 256, max_blocks);
        {
            cf_scratch recs(ctx);      // the records are gone again before the tables of the sweeps are taken
            unsigned long long *d_recs = nullptr, *d_rtmp = nullptr, *d_sorted = nullptr;
            uint32_t* d_ucnt = nullptr; int64_t* d_uoff = nullptr;
            if (n_parts > 1) {       // what this partition keeps of every unit's cloud, and where its records go
                CF_TRY(recs.get(&d_ucnt, (size_t)(u1 - u0) + 1, "kept entries per unit"));
                CF_TRY(recs.get(&d_uoff, (size_t)(u1 - u0) + 1, "record offsets per unit"));
                CF_HIP(hipMemsetAsync(d_ucnt + (u1 - u0), 0, 4, ctx->stream));
                hipLaunchKernelGGL(cf_post_ucount_kernel, dim3(g_units), dim3(256), 0, ctx->stream, v_cloud_ptr, v_entries, u0, u1, (uint32_t)part, (uint32_t)n_parts, d_ucnt);
                CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_ucnt, d_uoff, (u1 - u0) + 1, &n));
            }
            CF_TRY(recs.get(&d_recs, (size_t)n + 1, "posting records"));
            CF_TRY(recs.get(&d_rtmp, (size_t)n + 1, "posting records (sort)"));
            if (n_parts > 1)
                hipLaunchKernelGGL(cf_post_recs_part_kernel, dim3(g_units), dim3(256), 0, ctx->stream,
                                   v_cloud_ptr, v_entries, u0, u1, (uint32_t)part, (uint32_t)n_parts, (const int64_t*)d_uoff, kb, d_recs);
            else
                hipLaunchKernelGGL(cf_post_recs_kernel, dim3(g_units), dim3(256), 0, ctx->stream, v_cloud_ptr, v_entries, u0, u1, e0, kb, d_recs);
            if (n) CF_TRY(cf_radix_sort_u64_any(ctx, d_recs, d_rtmp, n, kb, &d_sorted));
            CF_TRY(tmp.get(&d_post, (size_t)n, "postings"));
            n_post = n;
            if (n) hipLaunchKernelGGL(cf_post_bounds_kernel, dim3((unsigned)cf_grid_for(n, 256, max_blocks)), dim3(256), 0, ctx->stream,
                               (const unsigned long long*)d_sorted, n, kb, (uint32_t)part, (uint32_t)n_parts, d_post, d_cursor, d_pcnt, d_first);      // (d_cursor = run starts, d_pcnt = run ends)
            hipLaunchKernelGGL(cf_post_counts_kernel, dim3((unsigned)cf_grid_for(K, 256, max_blocks)), dim3(256), 0, ctx->stream, (const uint32_t*)d_cursor, d_pcnt, K);
            CF_KERNEL_CHECK("the postings-by-sort kernels");
            CF_HIP(hipStreamSynchronize(ctx->stream));
        }
        int64_t n_chk = 0;
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_pcnt, d_post_ptr, K + 1, &n_chk));
        if (n_chk != n_post) return cf_fail(ctx, -5, "cf_dist_edges: internal error, posting counts do not add up");
    } else {
        if (e1 > e0)
            hipLaunchKernelGGL(cf_post_hist_kernel, dim3((unsigned)cf_grid_for(e1 - e0, 256, max_blocks)), dim3(256), 0, ctx->stream,
                               v_entries, e0, e1, (uint32_t)part, (uint32_t)n_parts, d_pcnt);
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_pcnt, d_post_ptr, K + 1, &n_post));
        CF_TRY(tmp.get(&d_post, (size_t)n_post, "postings"));
        if (u1 > u0 && n_post)
            hipLaunchKernelGGL(cf_post_fill_kernel, dim3((unsigned)cf_grid_for((u1 - u0) * 64, 256, max_blocks)), dim3(256), 0, ctx->stream,
                               v_cloud_ptr, v_entries, u0, u1, (uint32_t)part, (uint32_t)n_parts, (const int64_t*)d_post_ptr, d_cursor, d_post, d_first);
    }
    if (R)
        hipLaunchKernelGGL(cf_unit_rend_kernel, dim3((unsigned)cf_grid_for(R, 256, max_blocks)), dim3(256), 0, ctx->stream,
                           v_unit_ptr, v_cloud_ptr, R, min_d_eff, max_d, d_rend, d_rbeg, d_urange);
    // table layout: 6-byte slots (32-bit keys, 16-bit counts) whenever ranks fit 24 bits and counts 15 bits
    uint32_t max_post = 0;
    if (K) {
        hipLaunchKernelGGL(cf_max_u32_kernel, dim3((unsigned)cf_grid_for(K, 256, max_blocks)), dim3(256), 0, ctx->stream,
                           (const uint32_t*)d_pcnt, K, (uint32_t*)(d_cnt + 7));
        CF_HIP(hipMemcpy(&max_post, d_cnt + 7, 4, hipMemcpyDeviceToHost));
    }
    // 6-byte slots [d : DB | b : 32 - DB] need the k-mer ranks in 32 - DB bits and every distance that can occur in DB
    // bits: d <= min(max_d, units of the longest read - 1)
    int64_t u_max = 0;
    for (int64_t r = min_n; r < max_n; ++r) u_max = std::max(u_max, v_h_unit_ptr[(size_t)r + 1] - v_h_unit_ptr[(size_t)r]);
    const int64_t d_need = std::max<int64_t>(1, std::min<int64_t>(max_d, u_max - 1));
    int need_bits = 1; while (((int64_t)1 << need_bits) <= d_need) ++need_bits;
    wide16 = d_need > 255;         // 16-bit distance field: [b:32 | d:16 | sel:1 | cnt:15]
    int kb = 24; while (kb < 32 && K >= ((int64_t)1 << kb) - 1) ++kb;       // ranks 0 .. K - 1 and the all-ones key stays free
    narrow_db = 32 - kb;                                                       // the widest distance field the ranks leave
    if (ctx->dist_dbits) narrow_db = std::min(narrow_db, ctx->dist_dbits);
    // (the 4-byte stream is read with buffer loads whose scalar byte offset has 32 bits: 2^30 entries and more take the other layouts)
    const bool stream4_ok = v_n_entries + (int64_t)DIST_ITEM < ((int64_t)1 << 30);
    narrow = !wide16 && !ctx->dist_wide && narrow_db >= 5 && narrow_db >= need_bits && max_post <= 32767u && stream4_ok;
    if (ctx->dist_dbits && !narrow) return cf_fail(ctx, -22, "cf_dist_edges: dist_dbits does not fit this input (distances or k-mer ranks need more bits)");
    // ranks that do not fit next to the distance: the 6-byte slots in 2^S table regions (the key drops the rank's low S bits)
    if (!narrow || ctx->dist_regions) {
        reg_shift = 0;
        while (reg_shift < 3 && ((K - 1) >> reg_shift) > ((int64_t)1 << 24) - 2) ++reg_shift;
        if (ctx->dist_regions) { int want = 0; while ((1 << want) < ctx->dist_regions) ++want; reg_shift = std::max(reg_shift, want); }
        region = !wide16 && !ctx->dist_wide && !ctx->dist_dbits && reg_shift <= 3 && ((K - 1) >> reg_shift) <= ((int64_t)1 << 24) - 2 && max_post <= 32767u && K < ((int64_t)1 << 31);
        if (ctx->dist_regions && !region) return cf_fail(ctx, -22, "cf_dist_edges: dist_regions does not fit this input");
        if (region) narrow = false;
        // up to 2^26 ranks and distances up to 127: the region table behind the 4-byte stream [unit index mod 64 : 6 | rank : 26]
        region26 = region && !ctx->dist_region_bytes && K <= ((int64_t)1 << 26) && d_need <= 127 && stream4_ok;
    }
    // groups of first k-mers: knob dist_groups, on top of the classes' conditions; the 6-byte layout's stream and keys only
    // (the wide, region and 26-bit-stream layouts keep the classes), and only in a launch that runs the sketch first: without it every partner entry of
    // the union needs a slot of a table that has fewer of them (8 bytes each), and the unions' tables split where the members' own did not.
    // Decided on the device: clouds that are not sets form groups of one that count.
    const bool groups_fit = ctx->dist_groups && ctx->dist_classes && by_sort && narrow && ctx->dist_sketch && min_cov >= 2 && min_cov <= 200;
    if (max_post >= (1u << 23) || (wide16 && max_post > 32767u)) return cf_fail(ctx, -34, wide16 ? "cf_dist_edges: distances above 255 with a k-mer of more than 32767 postings" : "cf_dist_edges: a k-mer has more than 2^23 postings");
    if (narrow || region26) { CF_TRY(tmp.get(&d_packed, (size_t)v_n_entries + DIST_ITEM, "packed cloud entries")); }
    else if (region) { CF_TRY(tmp.get(&d_entry_i8, (size_t)v_n_entries + 4 * DIST_ITEM, "entry unit indices (bytes)")); }
    else CF_TRY(tmp.get(&d_entry_i, (size_t)v_n_entries + 1, "entry unit indices"));
    if (U && v_n_entries)
        hipLaunchKernelGGL(cf_entry_unit_kernel, dim3((unsigned)cf_grid_for(U * 64, 256, max_blocks)), dim3(256), 0, ctx->stream,
                           v_cloud_ptr, (const int32_t*)d_rbeg, v_entries, U, d_entry_i, d_packed, region26 ? 26 : 32 - narrow_db, d_entry_i8, d_cnt + 144);
    CF_KERNEL_CHECK("the postings kernels");
    CF_HIP(hipEventRecord(ctx->ev2, ctx->stream));

    cf_dist_args A;
    A.post_ptr = d_post_ptr; A.post = d_post; A.cloud_ptr = v_cloud_ptr; A.entries = v_entries; A.unit_rend = d_rend; A.unit_rbeg = d_rbeg; A.urange = d_urange; A.entry_i = d_entry_i; A.packed = d_packed; A.entry_i8 = d_entry_i8; A.reg_shift = (uint32_t)reg_shift;
    A.n_kmers = K; A.part = part; A.n_parts = n_parts; A.min_d = min_d_eff; A.max_d = max_d; A.min_cov = min_cov; A.thr = rel_threshold;
    A.thr_num = (rel_threshold == 0.8 && ctx->dist_int_thr) ? 4u : 0u; A.thr_den = A.thr_num ? 5u : 0u;
    A.stage_cap = (uint32_t)std::min(ctx->dist_stage, DIST_STAGE_CAP);
    A.filter_once = ctx->dist_filter_once ? 1u : 0u;
    A.hot_cap = ctx->dist_hot_cap > 0 ? (uint32_t)ctx->dist_hot_cap : 0xFFFFFFFFu;
    A.hot_entries = ctx->dist_hot_entries >= 0 ? (uint32_t)ctx->dist_hot_entries : 0xFFFFFFFFu;
    // launch shape: two 512-thread workgroups per CU (80 KiB of LDS each) overlap each other's latency-bound phases
    // and win when a first k-mer has few pair emissions; with many (long reads, high coverage) the halved table and
    // sketch cost more than the overlap gains, and one 1024-thread workgroup with the whole LDS wins (measured:
    // 20 k emissions per first k-mer: 480 vs 716 ms; 53 k: 437 vs 274 ms; 160 k: 2097 vs 739 ms)
    // pair emissions per first k-mer, ESTIMATED on the host (round 6; rounds 2-5 summed the partner ranges of every posting on the device —
    // a kernel of random gathers, 1.05 ms of every launch, and a blocking copy — for a figure that only picks the launch shape): the
    // partner units of every unit of the reads in range, exactly, times the mean cloud size, times the mean postings per unit
    double per_first = 0.0;
    if (n_post && u1 > u0) {
        unsigned long long partner_units = 0;
        for (int64_t r = min_n; r < max_n; ++r) {
            const int64_t nu = v_h_unit_ptr[(size_t)r + 1] - v_h_unit_ptr[(size_t)r];
            // unit i of a read of nu units has max(0, min(nu - 1, i + max_d) - (i + min_d) + 1) partner units
            const int64_t span = (int64_t)max_d - min_d_eff + 1;
            if (nu <= min_d_eff || span <= 0) continue;
            const int64_t full = std::max<int64_t>(0, nu - max_d);           // units with the whole span behind them
            const int64_t tail = nu - min_d_eff - full;                      // the rest: nu - min_d - i partner units each, down to 1
            partner_units += (unsigned long long)(full * span) + (unsigned long long)(tail > 0 ? tail * (tail + 1) / 2 : 0);
        }
        const double cloud = (double)(e1 - e0) / (double)(u1 - u0), post_per_unit = (double)n_post / (double)(u1 - u0);
        per_first = (double)partner_units * cloud * post_per_unit / (double)std::max<int64_t>(1, (K - part + n_parts - 1) / n_parts);
    }
    // ... and only where a first k-mer has few pair emissions, the regime of the two-workgroup launch shape below.  Measured on cenX-shaped reads
    // (60 000 emissions per first k-mer, var_len 8): one first k-mer brings 7 - 8 000 keys to a mask table whose fill limit is about
    // 9 000, the union of a group more — the tables split and are streamed again: 119.9 ms per step against 89.2 with classes.
    const bool groups = groups_fit && per_first <= 32768.0;
    const uint32_t slot_bytes = groups ? cf_tab_mask<8>::kSlotBytes : (narrow || region) ? cf_tab_narrow::kSlotBytes : cf_tab_wide::kSlotBytes;
    int wgs = ctx->dist_wgs, block = ctx->dist_block;
    if (wgs == 0) wgs = (block > 512 || per_first > 32768.0) ? 1 : 2;
    if (block == 0) block = wgs == 1 ? 1024 : 512;
    // LDS: everything but the table is fixed; dist_slots (the table budget in 8-byte units) defaults to all the rest
    const size_t qitem_bytes = narrow ? sizeof(cf_tab_narrow::qitem) : sizeof(cf_tab_wide::qitem);      // (the region layouts queue 64-bit items, like the wide one)
    const size_t lds_fixed = DIST_LDS_HEAD + (size_t)(2 * DIST_STACK) * 4 + DIST_STAGE_CAP * 2 + 16 + (size_t)(block / 64) * (DIST_QSTRIDE + DIST_OVQ) * qitem_bytes + DIST_HOT_CAP * 2
                             + (groups ? (((size_t)(block / 64) * (DIST_QSTRIDE + DIST_OVQ) + 15) & ~(size_t)15) : 0);      // (groups: a byte per queued insert)
    const int64_t budget8 = ((int64_t)160 * 1024 / wgs - (int64_t)lds_fixed) / 8;
    if (budget8 < 256) return cf_fail(ctx, -22, "cf_dist_edges: dist_wgs leaves no LDS for the table");
    if (ctx->dist_slots > budget8) return cf_fail(ctx, -22, "cf_dist_edges: dist_slots does not fit the 160 KiB LDS next to the work lists");
    const int64_t slots8 = ctx->dist_slots ? ctx->dist_slots : budget8;
    A.slots = (int32_t)((slots8 * 8 / slot_bytes) & ~(region ? (int64_t)(32 << reg_shift) - 1 : 7ll));      // (regions: equal parts of whole 8-slot groups)
    if (groups) {      // 8 bytes per slot and the bitmap of the marks (16 bytes per 128 slots or part of them) inside the same budget
        A.slots = (int32_t)((slots8 * 8 / cf_tab_mask<8>::kSlotBytes) & ~7ll);
        while (A.slots > 8 && (int64_t)A.slots * cf_tab_mask<8>::kSlotBytes + cf_tab_mask<8>::extra_bytes((uint32_t)A.slots) > slots8 * 8) A.slots -= 8;
    }
    const size_t tab_extra = groups ? cf_tab_mask<8>::extra_bytes((uint32_t)A.slots) : 0;
    if (A.slots >= 0xFFFF) return cf_fail(ctx, -22, "cf_dist_edges: more than 65534 table slots (16-bit slot indices; 0xFFFF marks an unused entry of the hot list)");
    A.fill_limit = (uint32_t)((int64_t)A.slots * ctx->dist_fill_pct / 100);   // checked once per wave step: leave slack below the physical size
    {   //  the fill level a drain looks at lags by one drain: every wave may put 2 x 128 fresh keys behind the limit before it
        // stops — the limit leaves that room below the physical size where the table is large enough for it (tables that tests force down
        // to a few hundred slots keep their limit: a pass that fills up there is void and split, as it always was, and all the pairs of ONE
        // b must fit one partition)
        const int64_t slack = (int64_t)(block / 64) * 2 * 128;
        if (slack * 4 <= (int64_t)A.slots) A.fill_limit = (uint32_t)std::min<int64_t>(A.fill_limit, (int64_t)A.slots - slack);
    }
    A.est_limit = (uint32_t)((int64_t)A.fill_limit * 100 / ctx->dist_est_pct);
    A.counters = d_cnt; A.unique_bits = ctx->d_unique_bits;
    const size_t lds = (size_t)A.slots * slot_bytes + tab_extra + lds_fixed;
    A.sketch = (ctx->dist_sketch && min_cov >= 2 && min_cov <= 200) ? 1 : 0;
    A.sk_shift = 32; A.sk_counters = 1;
    const size_t sk_room = (size_t)A.slots * slot_bytes + DIST_STAGE_CAP * 2 + 16 + (size_t)(block / 64) * (DIST_QSTRIDE + DIST_OVQ) * qitem_bytes + 2 * DIST_STACK * 4 + DIST_HOT_CAP * 2;   // table + stage + stack + queues + hot list: all dead while the sketch runs
    while (A.sk_shift > 8 && (size_t)A.sk_counters * 2 <= sk_room) { A.sk_counters *= 2; --A.sk_shift; }
    if (A.sk_counters < 16) A.sketch = 0;
    A.sk_bytes = A.sk_counters;
    // 4-bit counters when min_cov - 1 fits well below their guard ("dist_sketch_bits" 8 keeps the bytes)
    const bool sk4 = A.sketch && min_cov <= 9 && ctx->dist_sketch_bits != 8 && A.sk_shift > 9;
    if (sk4) { A.sk_counters *= 2; --A.sk_shift; A.sk_fbits = 4; A.sk_fsh = 2; A.sk_wshift = 3; A.sk_fmask = 15; A.sk_guard = 12; }
    else { A.sk_fbits = 8; A.sk_fsh = 3; A.sk_wshift = 2; A.sk_fmask = 255; A.sk_guard = 0x7FFFFFFFu; }
    A.sk_mask = A.sk_counters - 1u;
    const int per_cu = std::max(1, std::min((int)((160 * 1024) / lds), 2048 / block));
    // locality order of the first k-mers: sort (first posting unit, a); k-mers without postings drop out
    const int64_t n_a_alloc = (K > part) ? (K - part + n_parts - 1) / n_parts : 0;
    CF_TRY(tmp.get(&d_okeys, (size_t)n_a_alloc, "order keys"));
    CF_TRY(tmp.get(&d_otmp, (size_t)n_a_alloc, "order scratch"));
    CF_TRY(tmp.get(&d_order, (size_t)n_a_alloc, "order"));
    int ab = 1, ub = 1;      // bits of a rank, bits of a unit number
    while (ab < 32 && ((int64_t)1 << ab) < K) ++ab;
    while (ub < 32 && ((int64_t)1 << ub) < std::max<int64_t>(U, 2)) ++ub;
    // classes of first k-mers with equal posting lists: knob dist_classes; off when the postings came from the atomics'
    // fill pass (unordered lists) and — decided on the device — when a cloud row is not a set
    const bool classes = ctx->dist_classes && by_sort;
    const int hb = classes ? std::min(ctx->dist_class_bits, 64 - ab - ub) : 0;      // hash bits of the order key (16: two more radix passes); with groups: bits of the second posting unit
    int64_t n_heads = 0;
    uint32_t *d_cflag = nullptr, *d_cfirst = nullptr, *d_ulen = nullptr, *d_mmask = nullptr, *d_newm = nullptr;
    int32_t* d_upost = nullptr;
    if (K) {
        hipLaunchKernelGGL(cf_order_keys_kernel, dim3((unsigned)cf_grid_for(K, 256, max_blocks)), dim3(256), 0, ctx->stream,
                           (const uint32_t*)d_pcnt, (const uint32_t*)d_first, K, (int)part, (int)n_parts, ab, d_okeys, d_cnt + 6,
                           hb, (const int64_t*)d_post_ptr, (const int32_t*)d_post, (const unsigned long long*)(d_cnt + 144), groups ? 1 : 0);
        unsigned long long h_n = 0;
        CF_HIP(hipMemcpy(&h_n, d_cnt + 6, 8, hipMemcpyDeviceToHost));
        n_order = (int64_t)h_n;
        CF_TRY(cf_radix_sort_u64(ctx, d_okeys, d_otmp, n_order, ab + hb + ub));      // (round 6: the key's own bits — 6 radix passes at 50 000 reads; rounds 2-5 sorted all 64)
        if (n_order)
            hipLaunchKernelGGL(cf_order_extract_kernel, dim3((unsigned)cf_grid_for(n_order, 256, max_blocks)), dim3(256), 0, ctx->stream,
                               (const unsigned long long*)d_okeys, n_order, ab, d_order);
    }
    n_heads = n_order;
    if (classes && n_order) {
        const unsigned g_cls = (unsigned)cf_grid_for(n_order, 256, max_blocks);
        int64_t* d_cidx = (int64_t*)d_otmp;      // (the sort's scratch: free again, and as large)
        CF_TRY(tmp.get(&d_cflag, (size_t)n_order + 1, "class flags"));
        CF_TRY(tmp.get(&d_cfirst, (size_t)n_order + 1, "class starts"));
        CF_HIP(hipMemsetAsync(d_cflag, 0, (size_t)(n_order + 1) * 4, ctx->stream));
        if (groups) { CF_TRY(tmp.get(&d_mmask, (size_t)n_order + 1, "member masks")); CF_TRY(tmp.get(&d_newm, (size_t)n_order + 1, "members' new postings")); }
        if (groups) {      // the cut of the runs into groups, and the members' own emissions
            const bool tab = ctx->dist_walk;      // (the open group's union in an LDS table; 0: in the lanes)
            const unsigned g_walk = g_cls;
            unsigned long long* d_wdg = nullptr;
#if defined(CF_WALK_STAMPS)
            CF_TRY(tmp.get(&d_wdg, 8 + 2 * (size_t)g_walk, "walk stamps"));
            CF_HIP(hipMemsetAsync(d_wdg, 0, (8 + 2 * (size_t)g_walk) * 8, ctx->stream));
#endif
            hipLaunchKernelGGL(tab ? cf_group_walk_kernel<true> : cf_group_walk_kernel<false>, dim3(g_walk), dim3(256), tab ? DIST_WALK_LDS_TAB(256) : DIST_WALK_LDS(256), ctx->stream,
                               (const unsigned long long*)d_okeys, n_order, ab + hb, ab,
                               (const int64_t*)d_post_ptr, (const int32_t*)d_post, (const unsigned long long*)(d_cnt + 144), (uint32_t)ctx->dist_group_cap,
                               (const cf_dist_rec*)d_urange, (const int32_t*)d_rend, min_d_eff, max_d, d_cflag, d_mmask, d_newm, d_cnt + 1, d_cnt + 3, d_wdg);
#if defined(CF_WALK_STAMPS)
            {
                std::vector<unsigned long long> dgh(8 + 2 * (size_t)g_walk);
                if (hipMemcpy(dgh.data(), d_wdg, dgh.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                    unsigned long long wg = 0;      // the workgroups' lifetimes, a wave slot each for every wave of theirs
                    for (size_t b = 0; b < g_walk; ++b) if (dgh[9 + 2 * b]) wg += (dgh[9 + 2 * b] - ~dgh[8 + 2 * b]) * 4ull;
                    std::fprintf(stderr, "[cf_walk stamps] member=%llu load=%llu wave_life=%llu slot_life=%llu members=%llu postings=%llu waves=%llu (shader cycles summed over the waves of %u workgroups; dist_walk=%d)\n",
                                 dgh[0], dgh[1], dgh[2], wg, dgh[3], dgh[4], dgh[5], g_walk, tab ? 1 : 0);
                }
            }
#endif
        } else
        hipLaunchKernelGGL(cf_class_mark_kernel, dim3(g_cls), dim3(256), 0, ctx->stream, (const unsigned long long*)d_okeys, n_order, ab,
                           (const int64_t*)d_post_ptr, (const int32_t*)d_post, (const unsigned long long*)(d_cnt + 144), d_cflag);
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_cflag, d_cidx, n_order, &n_heads));
        hipLaunchKernelGGL(cf_class_first_kernel, dim3(g_cls), dim3(256), 0, ctx->stream, (const uint32_t*)d_cflag, (const int64_t*)d_cidx, n_order, n_heads, d_cfirst);
        if (groups) {      // the unions, and the members' own emissions
            CF_TRY(tmp.get(&d_upost, (size_t)n_heads * DIST_GROUP_MAX + 1, "group unions"));
            CF_TRY(tmp.get(&d_ulen, (size_t)n_heads + 1, "group union sizes"));
            hipLaunchKernelGGL(cf_group_fill_kernel, dim3((unsigned)cf_grid_for(n_heads * DIST_FILL_TEAM, 256, max_blocks)), dim3(256), 0, ctx->stream, (const int32_t*)d_order, (const uint32_t*)d_cfirst, n_heads,
                               (const int64_t*)d_post_ptr, (const int32_t*)d_post, (const unsigned long long*)(d_cnt + 144), (uint32_t)ctx->dist_group_cap, (const uint32_t*)d_newm, (const uint32_t*)d_mmask,
                               d_upost, d_ulen, d_cnt + 148, d_cnt + 4);
        }
        CF_KERNEL_CHECK("the class kernels");
    }
    A.order = d_order; A.n_order = n_heads; A.member_mask = d_mmask;
    // the work lists of the sweeps (heads + item records, laid out for workgroups of `block` threads): count, scan, fill
    if (n_heads) {
        const uint32_t nw = (uint32_t)block / 64u;
        const int g_items = cf_grid_for(n_heads * 16, 256, max_blocks);
        CF_TRY(tmp.get(&d_icnt, (size_t)n_heads + 1, "item counts"));
        CF_TRY(tmp.get(&d_ialloc, (size_t)n_heads + 1, "item slots"));
        CF_TRY(tmp.get(&d_ibase, (size_t)n_heads + 1, "item bases"));
        CF_TRY(tmp.get(&d_heads, (size_t)n_heads, "first k-mer heads"));
        hipLaunchKernelGGL(groups ? cf_items_count_kernel<true> : cf_items_count_kernel<false>, dim3((unsigned)g_items), dim3(256), 0, ctx->stream, (const int32_t*)d_order, n_heads, (const int64_t*)d_post_ptr,
                           (const int32_t*)d_post, (const cf_dist_rec*)d_urange, (const int32_t*)d_rbeg, min_d_eff, max_d, nw, by_sort ? 1 : 0, d_icnt, d_ialloc, d_cnt + 3,
                           (const uint32_t*)d_cfirst, (const int32_t*)d_upost, (const uint32_t*)d_ulen);
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_ialloc, d_ibase, n_heads, &n_item_slots));
        CF_TRY(tmp.get(&d_items, (size_t)n_item_slots + 64, "item records"));
        hipLaunchKernelGGL(groups ? cf_items_fill_kernel<true> : cf_items_fill_kernel<false>, dim3((unsigned)g_items), dim3(256), 0, ctx->stream, (const int32_t*)d_order, n_heads, (const int64_t*)d_post_ptr,
                           (const int32_t*)d_post, (const cf_dist_rec*)d_urange, nw, (const uint32_t*)d_icnt, (const int64_t*)d_ibase, d_heads, d_items,
                           v_cloud_ptr, region26 ? 1 : 0, U, min_d_eff, max_d, min_cov, (ctx->dist_sketch_tail && A.sketch) ? 1 : 0,
                           (const unsigned long long*)(d_cnt + 144), d_cnt + 145, (const uint32_t*)d_cfirst, (const int32_t*)d_upost, (const uint32_t*)d_ulen);
    }
    A.heads = d_heads; A.items = d_items;
    const int64_t n_a = n_heads;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_a, (int64_t)std::max(1, ctx->n_cu) * per_cu));
    CF_KERNEL_CHECK("the work-list kernels");
    CF_HIP(hipEventRecord(ctx->ev2, ctx->stream));
#define CF_DIST_KERN(CLS) (region26 ? cf_dist_kernel<cf_tab_region26, CLS> : region ? cf_dist_kernel<cf_tab_region, CLS> : !narrow ? (wide16 ? cf_dist_kernel<cf_tab_wide16, CLS> : cf_dist_kernel<cf_tab_wide, CLS>) \
                               : narrow_db == 8 ? cf_dist_kernel<cf_tab_narrow_t<8>, CLS> : narrow_db == 7 ? cf_dist_kernel<cf_tab_narrow_t<7>, CLS>                                               \
                               : narrow_db == 6 ? cf_dist_kernel<cf_tab_narrow_t<6>, CLS> : cf_dist_kernel<cf_tab_narrow_t<5>, CLS>)
    void (*kern)(cf_dist_args) = classes ? CF_DIST_KERN(true) : CF_DIST_KERN(false);      // (without classes: the kernel without the member loop)
    if (groups) kern = narrow_db == 8 ? cf_dist_kernel<cf_tab_mask<8>, true> : narrow_db == 7 ? cf_dist_kernel<cf_tab_mask<7>, true> : narrow_db == 6 ? cf_dist_kernel<cf_tab_mask<6>, true> : cf_dist_kernel<cf_tab_mask<5>, true>;
#undef CF_DIST_KERN
    CF_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // the edge output: edge_cap rows + the unused rest of one chunk per workgroup (the holes; closed below), so that every
    // selected edge is in memory whenever edge_cap >= their number
    {
        A.edge_chunk = ctx->dist_edge_chunk > 0 ? (unsigned long long)ctx->dist_edge_chunk : DIST_EDGE_CHUNK;
        const int64_t rows = edge_cap > 0 ? edge_cap + (int64_t)grid * (int64_t)A.edge_chunk : 0;
        CF_TRY(cf_alloc_t(ctx, &ctx->d_edges, (size_t)rows * 4, "edges"));
        ctx->edge_cap = rows;
        A.edges = ctx->d_edges; A.edge_cap = (unsigned long long)rows;
    }
    CF_TRY(tmp.get(&d_holes, 2 * ((size_t)grid + 1), "edge holes"));
    A.holes = d_holes;
    CF_HIP(hipMemsetAsync(d_cnt + 6, 0, 16, ctx->stream));      // [6] selected edges, [7] holes
    if (n_a > 0 && max_d >= min_d_eff && n_post > 0) {
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3((unsigned)block), lds, ctx->stream, A);
        CF_KERNEL_CHECK("cf_dist_kernel");
    }
    CF_HIP(hipEventRecord(ctx->ev3, ctx->stream));
    CF_HIP(hipMemcpyAsync(h_cnt, d_cnt, 64, hipMemcpyDeviceToHost, ctx->stream));
    CF_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    CF_HIP(hipEventSynchronize(ctx->ev1));
#if defined(CF_DIST_DIAG_COUNT)
    {
        unsigned long long st[8];
        if (hipMemcpy(st, d_cnt + 8, 64, hipMemcpyDeviceToHost) == hipSuccess)
            std::fprintf(stderr, "[cf_dist diag] parked-insert loop trips=%llu overflow calls=%llu parked inserts run=%llu drains=%llu inserts drained=%llu cycles(sum over waves): parked runs=%llu drains=%llu table sweeps=%llu; waves=%d passes=%llu\n", st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7], grid * (block / 64), h_cnt[5]);
        unsigned long long su[4], up[2] = {0, 0};      // [0] a cloud row is not a set [1] sum of the useful items [2] sum of the items [3] partner entries swept, once per class; up: postings of the groups' unions, classes inside the groups
        const bool have_up = groups && hipMemcpy(up, d_cnt + 148, 16, hipMemcpyDeviceToHost) == hipSuccess;
        if (hipMemcpy(su, d_cnt + 144, 32, hipMemcpyDeviceToHost) == hipSuccess)
            std::fprintf(stderr, "[cf_dist diag] sketch items=%llu of items=%llu (rows are sets=%d) classes=%lld members=%lld entries swept=%llu of %llu per member\n", su[1], su[2], su[0] ? 0 : 1, have_up ? (long long)up[1] : (long long)n_heads, (long long)n_order, su[3], h_cnt[1]);      // (with groups: the distinct lists inside the groups)
        unsigned long long mf[5];
        if (hipMemcpy(mf, d_cnt + 152, 40, hipMemcpyDeviceToHost) == hipSuccess)
            std::fprintf(stderr, "[cf_dist diag] member filter: n_hot=%llu n_hot x members=%llu eval_slot calls with total_of=%llu buckets read in total_of=%llu slots with more keys than registers=%llu\n", mf[0], mf[1], mf[2], mf[3], mf[4]);
        if (have_up)
            std::fprintf(stderr, "[cf_dist diag] groups=%lld members=%lld union postings=%llu slots=%d split groups=%llu\n", (long long)n_heads, (long long)n_order, up[0], (int)A.slots, h_cnt[2]);
    }
#endif
#if defined(CF_DIST_STAMPS)
    {
        unsigned long long st[8];
        if (hipMemcpy(st, d_cnt + 8, 64, hipMemcpyDeviceToHost) == hipSuccess)
            std::fprintf(stderr, "[cf_dist stamps] pop=%llu prologue=%llu sketch=%llu clear=%llu stream=%llu filter=%llu write=%llu sweep_end_wait=%llu (shader cycles summed over %d workgroups; passes=%llu)\n",
                         st[0], st[1], st[6], st[2], st[3], st[4], st[5], st[7], grid, h_cnt[5]);
    }
#endif
    if (h_cnt[4] & 4ull) return cf_fail(ctx, -5, "cf_dist_edges: internal error, a group's union has more postings than its mask has bits");
    if (h_cnt[4] & 2ull) return cf_fail(ctx, -5, "cf_dist_edges: the kernel's dynamic LDS does not begin at address 0");
    if (h_cnt[4]) return cf_fail(ctx, -34, "cf_dist_edges: (b,d) table could not be partitioned far enough");
    // close the holes of the chunked edge output: the valid rows at or above n_valid move into the holes below it
    {
        const unsigned long long a_cap = std::min<unsigned long long>(h_cnt[0], A.edge_cap);      // rows that exist in memory
        std::vector<unsigned long long> hh(2 * (size_t)h_cnt[7]);
        if (!hh.empty()) {
            CF_HIP(hipMemcpyAsync(hh.data(), d_holes, hh.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
            CF_HIP(hipStreamSynchronize(ctx->stream));
        }
        std::vector<std::pair<unsigned long long, unsigned long long>> holes;      // [start, end) clipped to the rows in memory, sorted
        for (size_t i = 0; i + 1 < hh.size(); i += 2) {
            const unsigned long long s0 = std::min(hh[i], a_cap), s1 = std::min(hh[i] + hh[i + 1], a_cap);
            if (s1 > s0) holes.emplace_back(s0, s1);
        }
        std::sort(holes.begin(), holes.end());
        unsigned long long hole_rows = 0;
        for (auto& h : holes) hole_rows += h.second - h.first;
        const unsigned long long n_valid = a_cap - hole_rows;
        n_stored = (int64_t)std::min<unsigned long long>(n_valid, (unsigned long long)edge_cap);
        std::vector<unsigned long long> dst_start, dst_pre, src_start, src_pre;
        unsigned long long dsum = 0, ssum = 0, at = n_valid;
        for (auto& h : holes) {
            if (h.first < n_valid) { const unsigned long long e1 = std::min(h.second, n_valid); dsum += e1 - h.first; dst_start.push_back(h.first); dst_pre.push_back(dsum); }
            if (h.second > n_valid) {      // valid rows between `at` and this hole's part above n_valid
                const unsigned long long h0 = std::max(h.first, n_valid);
                if (h0 > at) { ssum += h0 - at; src_start.push_back(at); src_pre.push_back(ssum); }
                at = h.second;
            }
        }
        if (a_cap > at) { ssum += a_cap - at; src_start.push_back(at); src_pre.push_back(ssum); }
        if (dsum != ssum) return cf_fail(ctx, -5, "cf_dist_edges: internal error, edge holes do not match the rows above them");
        if (dsum) {
            cf_scratch seg(ctx);
            unsigned long long* d_seg = nullptr;
            const size_t n_seg = src_start.size() * 2 + dst_start.size() * 2;
            CF_TRY(seg.get(&d_seg, n_seg, "edge move lists"));
            std::vector<unsigned long long> pack;
            pack.insert(pack.end(), src_start.begin(), src_start.end()); pack.insert(pack.end(), src_pre.begin(), src_pre.end());
            pack.insert(pack.end(), dst_start.begin(), dst_start.end()); pack.insert(pack.end(), dst_pre.begin(), dst_pre.end());
            CF_HIP(hipMemcpyAsync(d_seg, pack.data(), n_seg * 8, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(cf_edge_compact_kernel, dim3((unsigned)cf_grid_for((int64_t)dsum, 256, max_blocks)), dim3(256), 0, ctx->stream, ctx->d_edges,
                               (const unsigned long long*)d_seg, (const unsigned long long*)(d_seg + src_start.size()), (int)src_start.size(),
                               (const unsigned long long*)(d_seg + 2 * src_start.size()), (const unsigned long long*)(d_seg + 2 * src_start.size() + dst_start.size()), (int)dst_start.size(), dsum);
            CF_KERNEL_CHECK("cf_edge_compact_kernel");
            CF_HIP(hipStreamSynchronize(ctx->stream));
        }
    }
    // (the stage ends behind the compaction of the chunked edge output, not behind the kernel)
    CF_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    CF_HIP(hipEventSynchronize(ctx->ev1));
    (void)hipEventElapsedTime(&ctx->times.dist_ms, ctx->ev0, ctx->ev1);
    (void)hipEventElapsedTime(&ctx->times.postings_ms, ctx->ev0, ctx->ev2);
    (void)hipEventElapsedTime(&ctx->times.dist_kernel_ms, ctx->ev2, ctx->ev3);
    ctx->stats.n_edges = (int64_t)h_cnt[6];
    ctx->stats.n_emissions = (int64_t)h_cnt[1] - (int64_t)h_cnt[3];      // partner entries swept, less those that are the first k-mer itself (a != b in the reference)
    ctx->stats.n_spilled = (int64_t)h_cnt[2];
    ctx->stats.n_dist_passes = (int64_t)h_cnt[5];
    ctx->n_edges_stored = n_stored;      // every selected edge when edge_cap allowed it, else the valid rows below the cap
    CF_TRY(cf_refresh_unique_count(ctx));
    if (n_edges) *n_edges = (int64_t)h_cnt[6];
    return 0;
}

}  // extern "C"
