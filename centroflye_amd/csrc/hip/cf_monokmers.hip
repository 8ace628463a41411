// cf_monokmers.hip — exact counts of every gap-free window of k letters over a set of monostrings, in the order of first occurrence
// (gfx950, wave64).
//
// What the reference's second pipeline does in a Python loop over string slices (scripts/debruijn_graph.py get_frequent_kmers,
// scripts/mono_error_correction.py correct_gaps).  The rule is written out at cf_monokmers_run in include/cfhip.h and restated in
// tests/monokmercheck.py.  Equality of k-mers is equality of bytes: nothing here is a hash.
//
// PREFIX DOUBLING ON EQUALITY RANKS.  R_1[p] is the byte at p.  R_2m[p] is the dense id of the pair (R_m[p], R_m[p + m]) over the
// valid windows of length 2m, so R_m[p] == R_m[q] iff the m bytes at p and at q are equal.  With a the largest power of two not
// above k one overlapping combine (R_a[p], R_a[p + k - a]) gives R_k.  A window (p, L) is valid iff dist[p] >= L, dist[p] = the
// letters from p to the next gap byte or the end of p's string.
//
//   the distances, once   cf_mk_last      the last byte of every non-empty string gets a mark (a byte per position)
//                         cf_mk_stops     stop[p] = byte p is the gap or marked; four positions per thread, 4-byte loads, a 16-byte store
//                         (scan)          e[p] = stops in front of p  (cf_prims.hip)
//                         cf_mk_stop_list the stops' positions, dense: list[e[p]] = p
//                         cf_mk_dist      the first stop q >= p is list[e[p]] and lies in p's string: dist[p] = 0 at a gap, else
//                                         q - p (+ 1 when q is a last byte and no gap); R[p] = the byte
//                         (The issue asked for a segmented backward scan.  The forward count of stops gives the same value from the
//                         scan the library has, with streaming passes only and no new block-level code.)
//   a round (m, d, L)     cf_mk_keys      record p = (R[p], R[p + d], p) where dist[p] >= L, else (D, D, p) with D = the ids of the
//                                         round before — one more than every id — so that the invalid ones sort behind all others
//                         (sort)          the stable 16-byte-record radix sort (cf_prims.hip) by word 1, then word 0, on the bits D needs
//                         cf_mk_heads     head[i] = record i is valid and differs from record i - 1; the last valid index + 1 = V
//                         (scan)          id of record i = heads in front of it + head[i] - 1
//                         cf_mk_ids       R[p] = the id  (in place: the keys were built from the old R)
//   the finish            The sort is stable and the records were built in ascending p, so the records of the LAST round lie class by
//                         class with ascending positions inside a class: a class's first record holds its first occurrence, the
//                         next class's first record ends its count, and the run of records is its occurrence list already.
//                         cf_mk_classes   class c: (first position, index of its first record, -, c)
//                         cf_mk_filter    its count; a class below min_mult takes the first position N: it sorts behind all others
//                         (sort)          the classes by first position
//                         cf_mk_emit      output j: (string, index, count, position), the string by a binary search in the offsets;
//                                         rank[c] = j or -1; the last kept index + 1 = K
//                         (scan)          the CSR's offsets from the counts
//                         cf_mk_occ       record i of a kept class c goes to ptr[rank[c]] + i - first record of c, as (string, index)
// The distances and the rounds are one function, cf_mk_rank_windows (cf_common.h), which cf_monomap.hip runs over the edges of the
// graph and the reads together; the finish is cf_monokmers_run's own.
// Every kernel is a grid-stride streaming pass of 256 threads with 4-, 8- or 16-byte accesses per lane and no LDS, no atomics and no
// wave operation; every index is below N < 2^31 and is checked against its array's length where it is a loaded value.
#include "cf_common.h"

#define CF_MK_BLOCK 256
#define CF_MK_WGS_PER_CU 8

#define CF_MK_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * CF_MK_BLOCK + threadIdx.x; i < (n); i += (int64_t)gridDim.x * CF_MK_BLOCK)

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_last(const int64_t* __restrict__ off, int64_t n_strings, uint8_t* __restrict__ last, int64_t n) {
    CF_MK_LOOP(s, n_strings) {
        const int64_t b = off[s] - off[0], e = off[s + 1] - off[0];
        if (e > b && e <= n) last[e - 1] = 1;
    }
}

// (bytes and last are padded to a multiple of 4 and start on 4-byte borders; stop has room for a multiple of 4 entries)
__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_stops(const uint32_t* __restrict__ bytes4, const uint32_t* __restrict__ last4, uint32_t gap, cf_mk_rec* __restrict__ stop4, int64_t n) {
    const int64_t n4 = (n + 3) >> 2;
    CF_MK_LOOP(q, n4) {
        const uint32_t b = bytes4[q], l = last4[q];
        cf_mk_rec r;
#pragma unroll
        for (int x = 0; x < 4; ++x)
            r.w[x] = (4 * q + x < n && ((((b >> (8 * x)) & 0xffu) == gap) || ((l >> (8 * x)) & 0xffu))) ? 1u : 0u;
        stop4[q] = r;
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_stop_list(const uint32_t* __restrict__ stop, const int64_t* __restrict__ e, uint32_t* __restrict__ list, int64_t n, int64_t n_stops) {
    CF_MK_LOOP(p, n) {
        const int64_t x = e[p];
        if (stop[p] && x >= 0 && x < n_stops) list[x] = (uint32_t)p;
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_dist(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ e, const uint32_t* __restrict__ list, uint32_t gap, uint32_t* __restrict__ dist,
           uint32_t* __restrict__ R, int64_t n, int64_t n_stops) {
    CF_MK_LOOP(p, n) {
        const uint32_t b = bytes[p];
        const int64_t x = e[p];
        uint32_t d = 0;
        if (b != gap && x >= 0 && x < n_stops) {
            const int64_t q = list[x];
            if (q >= p && q < n) d = (uint32_t)(q - p) + ((uint32_t)bytes[q] == gap ? 0u : 1u);
        }
        dist[p] = d;
        R[p] = b;
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_keys(const uint32_t* __restrict__ R, const uint32_t* __restrict__ dist, cf_mk_rec* __restrict__ rec, int64_t n, uint32_t d, uint32_t need,
           uint32_t sentinel) {
    CF_MK_LOOP(p, n) {
        cf_mk_rec r;
        r.w[0] = r.w[1] = sentinel;
        r.w[2] = (uint32_t)p;
        r.w[3] = 0u;
        if (dist[p] >= need && p + (int64_t)d < n) {
            r.w[0] = R[p];
            r.w[1] = R[p + d];
        }
        rec[p] = r;
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_heads(const cf_mk_rec* __restrict__ rec, uint32_t* __restrict__ head, int64_t n, uint32_t sentinel, int64_t* __restrict__ n_valid) {
    CF_MK_LOOP(i, n) {
        const cf_mk_rec r = rec[i];
        const bool valid = r.w[0] != sentinel;
        bool h = valid;
        if (valid && i > 0) {
            const cf_mk_rec l = rec[i - 1];
            h = l.w[0] != r.w[0] || l.w[1] != r.w[1];
        }
        head[i] = h ? 1u : 0u;
        if (valid && (i == n - 1 || rec[i + 1].w[0] == sentinel)) *n_valid = i + 1;      // one thread: the valid records come first
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_ids(const cf_mk_rec* __restrict__ rec, const uint32_t* __restrict__ head, const int64_t* __restrict__ e, uint32_t* __restrict__ R, int64_t n_valid,
          int64_t n) {
    CF_MK_LOOP(i, n_valid) {
        const int64_t p = rec[i].w[2];
        if (p < n) R[p] = (uint32_t)(e[i] + head[i] - 1);
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_classes(const cf_mk_rec* __restrict__ rec, const uint32_t* __restrict__ head, const int64_t* __restrict__ e, cf_mk_rec* __restrict__ cls,
              uint32_t* __restrict__ seg, int64_t n_valid, int64_t n_classes) {
    CF_MK_LOOP(i, n_valid) {
        const int64_t c = e[i];
        if (head[i] && c >= 0 && c < n_classes) {
            cf_mk_rec r;
            r.w[0] = rec[i].w[2]; r.w[1] = (uint32_t)i; r.w[2] = 0u; r.w[3] = (uint32_t)c;
            cls[c] = r;
            seg[c] = (uint32_t)i;
        }
        if (i == 0) seg[n_classes] = (uint32_t)n_valid;
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_filter(cf_mk_rec* __restrict__ cls, const uint32_t* __restrict__ seg, int64_t n_classes, uint32_t min_mult, uint32_t sentinel) {
    CF_MK_LOOP(c, n_classes) {
        const uint32_t cnt = seg[c + 1] - seg[c];
        cf_mk_rec r = cls[c];
        r.w[2] = cnt;
        if (cnt < min_mult) r.w[0] = sentinel;
        cls[c] = r;
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_emit(const cf_mk_rec* __restrict__ cls, int64_t n_classes, uint32_t sentinel, const int64_t* __restrict__ off, int64_t n_strings,
           cf_monokmer* __restrict__ out, int32_t* __restrict__ rank, uint32_t* __restrict__ cnt, int64_t* __restrict__ n_kept) {
    CF_MK_LOOP(j, n_classes) {
        const cf_mk_rec r = cls[j];
        const bool kept = r.w[0] != sentinel;
        if (r.w[3] < (uint64_t)n_classes) rank[r.w[3]] = kept ? (int32_t)j : -1;
        cnt[j] = kept ? r.w[2] : 0u;
        if (kept) {
            const int64_t s = cf_string_of(off, n_strings, (int64_t)r.w[0] + off[0]);
            cf_monokmer o;
            o.s = (int32_t)s; o.i = (int32_t)((int64_t)r.w[0] + off[0] - off[s]); o.count = (int32_t)r.w[2]; o.pos = (int32_t)r.w[0];
            out[j] = o;
            if (j == n_classes - 1 || cls[j + 1].w[0] == sentinel) *n_kept = j + 1;      // one thread: the kept classes come first
        }
    }
}

__global__ void __launch_bounds__(CF_MK_BLOCK)
cf_mk_occ(const cf_mk_rec* __restrict__ rec, const uint32_t* __restrict__ head, const int64_t* __restrict__ e, int64_t n_valid, const uint32_t* __restrict__ seg,
          const int32_t* __restrict__ rank, int64_t n_classes, const int64_t* __restrict__ ptr, int64_t n_kept, int64_t n_occ,
          const int64_t* __restrict__ off, int64_t n_strings, cf_monokmer_occ* __restrict__ occ) {
    CF_MK_LOOP(i, n_valid) {
        const int64_t c = e[i] + head[i] - 1;
        if (c < 0 || c >= n_classes) continue;
        const int64_t j = rank[c];
        if (j < 0 || j >= n_kept) continue;
        const int64_t dst = ptr[j] + (i - (int64_t)seg[c]);
        if (dst < 0 || dst >= n_occ) continue;
        const int64_t p = rec[i].w[2], s = cf_string_of(off, n_strings, p + off[0]);
        cf_monokmer_occ o;
        o.s = (int32_t)s; o.i = (int32_t)(p + off[0] - off[s]);
        occ[dst] = o;
    }
}

int cf_mk_launch_cap(const cf_ctx* ctx) { return std::max(1, ctx->n_cu) * CF_MK_WGS_PER_CU; }
static int cf_mk_bits(uint64_t x) { int b = 1; while (b < 32 && (x >> b)) ++b; return b; }      // bits that hold the value x (at least 1)

// The equality classes of the valid windows of k letters (declared in cf_common.h): the distances, the rounds and the grouping of
// the bytes for k = 1.  d_bytes: the N letters on the device, padded with zeros to a multiple of 4 and 16 more; d_off: the
// n_strings + 1 offsets.  N >= 1 and k <= N.  Every buffer comes from the caller's guard.
int cf_mk_rank_windows(cf_ctx* ctx, cf_scratch& tmp, const uint8_t* d_bytes, const int64_t* d_off, int64_t n_strings, int64_t N, int64_t k, int32_t gap,
                       const char* who, cf_mk_ranked* out) {
    hipEvent_t e2 = ctx->ev2, e3 = ctx->ev3;
    float t = 0.f, sort_ms = 0.f;
    const int cap = cf_mk_launch_cap(ctx);
    const size_t n = (size_t)N, n4 = (n + 3) & ~(size_t)3;
    const uint32_t ugap = (uint32_t)gap, kk = (uint32_t)k;
    auto grid = [&](int64_t items) { return dim3((unsigned)cf_grid_for(items, CF_MK_BLOCK, cap)); };
    int64_t *d_e = nullptr, *d_scalar = nullptr;
    uint32_t *d_R = nullptr, *d_dist = nullptr, *d_head = nullptr;
    cf_mk_rec *d_rec = nullptr, *d_rec2 = nullptr;
    cf_mk_ranked shape{};
    CF_TRY(tmp.get(&d_R, n4, "monokmers ranks"));
    CF_TRY(tmp.get(&d_dist, n4, "monokmers distances"));
    CF_TRY(tmp.get(&d_head, n4, "monokmers head flags"));
    CF_TRY(tmp.get(&d_e, n4, "monokmers scan"));
    CF_TRY(tmp.get(&d_rec, n4, "monokmers records"));
    CF_TRY(tmp.get(&d_rec2, n4, "monokmers sort buffer"));
    CF_TRY(tmp.get(&d_scalar, 2, "monokmers counters"));

    // the distances: the stop flags, the list of stops and the marks of the last bytes live in the record buffers until round 1
    {
        uint32_t* d_stop = (uint32_t*)d_rec;                        // n4 entries
        uint32_t* d_list = (uint32_t*)d_rec + n4;                   // at most n entries
        uint8_t* d_last = (uint8_t*)((uint32_t*)d_rec + 2 * n4);    // n4 bytes
        CF_HIP(hipMemsetAsync(d_last, 0, n4, ctx->stream));
        if (n_strings > 0) {
            hipLaunchKernelGGL(cf_mk_last, grid(n_strings), dim3(CF_MK_BLOCK), 0, ctx->stream, (const int64_t*)d_off, n_strings, d_last, N);
            CF_KERNEL_CHECK("cf_mk_last");
        }
        hipLaunchKernelGGL(cf_mk_stops, grid((int64_t)(n4 / 4)), dim3(CF_MK_BLOCK), 0, ctx->stream, (const uint32_t*)d_bytes, (const uint32_t*)d_last, ugap,
                           (cf_mk_rec*)d_stop, N);
        CF_KERNEL_CHECK("cf_mk_stops");
        int64_t n_stops = 0;
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_stop, d_e, N, &n_stops));
        if (n_stops < 1 || n_stops > N) return cf_fail(ctx, -5, std::string(who) + ": the stops do not add up (internal error)");
        hipLaunchKernelGGL(cf_mk_stop_list, grid(N), dim3(CF_MK_BLOCK), 0, ctx->stream, (const uint32_t*)d_stop, (const int64_t*)d_e, d_list, N, n_stops);
        CF_KERNEL_CHECK("cf_mk_stop_list");
        hipLaunchKernelGGL(cf_mk_dist, grid(N), dim3(CF_MK_BLOCK), 0, ctx->stream, (const uint8_t*)d_bytes, (const int64_t*)d_e, (const uint32_t*)d_list, ugap,
                           d_dist, d_R, N, n_stops);
        CF_KERNEL_CHECK("cf_mk_dist");
    }

    // the rounds: (shift d, length L) = (1, 2), (2, 4), .. (a / 2, a), then (k - a, k) when k is no power of two; k = 1: one
    // grouping of the bytes themselves, which is no combining round
    struct round { uint32_t d, need; };
    std::vector<round> rounds;
    uint32_t a = 1;
    while ((uint64_t)a * 2 <= (uint64_t)kk) { rounds.push_back(round{a, a * 2}); a *= 2; }
    if (a != kk) rounds.push_back(round{kk - a, kk});
    shape.n_rounds = (int64_t)rounds.size();
    if (rounds.empty()) rounds.push_back(round{0u, 1u});
    int64_t n_ids = 256, n_valid = 0, n_classes = 0;      // ids of the round before: the bytes
    for (size_t r = 0; r < rounds.size(); ++r) {
        const bool last = r + 1 == rounds.size();
        const uint32_t sentinel = (uint32_t)n_ids;
        hipLaunchKernelGGL(cf_mk_keys, grid(N), dim3(CF_MK_BLOCK), 0, ctx->stream, (const uint32_t*)d_R, (const uint32_t*)d_dist, d_rec, N, rounds[r].d,
                           rounds[r].need, sentinel);
        CF_KERNEL_CHECK("cf_mk_keys");
        const int b = cf_mk_bits((uint64_t)n_ids);
        const int words[2] = {1, 0}, bits[2] = {b, b};
        CF_HIP(hipEventRecord(e2, ctx->stream));
        if (rounds[r].d == 0) CF_TRY(cf_radix_sort_rec16(ctx, d_rec, d_rec2, N, words + 1, bits + 1, 1));
        else CF_TRY(cf_radix_sort_rec16(ctx, d_rec, d_rec2, N, words, bits, 2));
        CF_HIP(hipEventRecord(e3, ctx->stream));
        CF_HIP(hipEventSynchronize(e3));
        (void)hipEventElapsedTime(&t, e2, e3); sort_ms += t;
        ++shape.n_sorts;
        shape.n_sort_passes += (rounds[r].d == 0 ? 1 : 2) * ((b + 7) / 8);
        CF_HIP(hipMemsetAsync(d_scalar, 0, 16, ctx->stream));
        hipLaunchKernelGGL(cf_mk_heads, grid(N), dim3(CF_MK_BLOCK), 0, ctx->stream, (const cf_mk_rec*)d_rec, d_head, N, sentinel, d_scalar);
        CF_KERNEL_CHECK("cf_mk_heads");
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_head, d_e, N, &n_classes));
        CF_TRY(cf_copy_d2h(ctx, &n_valid, d_scalar, 8));
        if (n_valid < 0 || n_valid > N || n_classes < 0 || n_classes > n_valid || (n_valid > 0) != (n_classes > 0))
            return cf_fail(ctx, -5, std::string(who) + ": the classes of a round do not add up (internal error)");
        if (!last && n_valid > 0) {
            hipLaunchKernelGGL(cf_mk_ids, grid(n_valid), dim3(CF_MK_BLOCK), 0, ctx->stream, (const cf_mk_rec*)d_rec, (const uint32_t*)d_head, (const int64_t*)d_e,
                               d_R, n_valid, N);
            CF_KERNEL_CHECK("cf_mk_ids");
        }
        n_ids = std::max<int64_t>(n_classes, 1);
        if (n_valid == 0) break;      // no window of this length: none of a longer one
    }
    shape.rec = d_rec; shape.rec2 = d_rec2; shape.R = d_R; shape.dist = d_dist; shape.head = d_head; shape.e = d_e; shape.scalar = d_scalar;
    shape.n_valid = n_valid;      // (a break in front of the last round leaves 0)
    shape.n_classes = n_classes;
    shape.sort_ms = sort_ms;
    *out = shape;
    return 0;
}

extern "C" {

int cf_monokmers_info(cf_ctx* ctx, cf_monokmers_shape* out) {
    if (!ctx || !out) return -22;
    *out = ctx->monokmers_last;
    out->sort_tile = cf_radix_rec16_tile();
    out->scan_tile = cf_scan_tile();
    out->block = CF_MK_BLOCK;
    out->launch_cap = cf_mk_launch_cap(ctx);
    return 0;
}

int cf_monokmers_get(cf_ctx* ctx, cf_monokmer* kmers, int64_t cap, int64_t* n_out, int64_t* occ_ptr, cf_monokmer_occ* occ, int64_t occ_cap, int64_t* n_occ_out) {
    if (!ctx) return -22;
    if (!ctx->monokmers_have) return cf_fail(ctx, -22, "cf_monokmers_get: no cf_monokmers_run before");
    const int64_t n = (int64_t)ctx->monokmers_first.size(), n_occ = (int64_t)ctx->monokmers_occ.size();
    if (n_out) *n_out = n;
    if (n_occ_out) *n_occ_out = ctx->monokmers_last.with_positions ? n_occ : -1;
    if (kmers) {
        if (cap < n) return cf_fail(ctx, -22, "cf_monokmers_get: room for " + std::to_string(cap) + " k-mers, " + std::to_string(n) + " needed");
        if (n) std::memcpy(kmers, ctx->monokmers_first.data(), (size_t)n * sizeof(cf_monokmer));
    }
    if (occ_ptr || occ) {
        if (!ctx->monokmers_last.with_positions) return cf_fail(ctx, -22, "cf_monokmers_get: the last run kept no positions");
        if (occ && occ_cap < n_occ)
            return cf_fail(ctx, -22, "cf_monokmers_get: room for " + std::to_string(occ_cap) + " occurrences, " + std::to_string(n_occ) + " needed");
        if (occ_ptr) std::memcpy(occ_ptr, ctx->monokmers_ptr.data(), ((size_t)n + 1) * 8);
        if (occ && n_occ) std::memcpy(occ, ctx->monokmers_occ.data(), (size_t)n_occ * sizeof(cf_monokmer_occ));
    }
    return 0;
}

int cf_monokmers_run(cf_ctx* ctx, const uint8_t* bytes, const int64_t* off, int64_t n_strings, int64_t k, int64_t min_mult, int32_t gap,
                     int32_t with_positions, int64_t* n_kmers_out, float* ms_out) {
    if (!ctx) return -22;
    if (ms_out) *ms_out = 0.f;
    if (n_kmers_out) *n_kmers_out = 0;
    if (k < 1) return cf_fail(ctx, -22, "cf_monokmers_run: k is below 1");
    if (min_mult < 1) return cf_fail(ctx, -22, "cf_monokmers_run: min_mult is below 1");
    if (gap < 0 || gap > 255) return cf_fail(ctx, -22, "cf_monokmers_run: the gap byte is outside 0 .. 255");
    if (n_strings < 0 || n_strings >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_monokmers_run: the number of strings is outside 0 .. 2^31 - 1");
    if (!off) return cf_fail(ctx, -22, "cf_monokmers_run: null offsets");
    if (off[0] < 0) return cf_fail(ctx, -22, "cf_monokmers_run: negative offset");
    for (int64_t s = 0; s < n_strings; ++s)
        if (off[s + 1] < off[s]) return cf_fail(ctx, -22, "cf_monokmers_run: the offsets do not ascend at string " + std::to_string(s));
    const int64_t N = off[n_strings] - off[0];
    if (N >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_monokmers_run: " + std::to_string(N) + " letters: N is 2^31 or more");
    if (N > 0 && !bytes) return cf_fail(ctx, -22, "cf_monokmers_run: null bytes");

    // the results of this call, handed to the context only when everything worked
    std::vector<cf_monokmer> res_first;
    std::vector<int64_t> res_ptr(1, 0);
    std::vector<cf_monokmer_occ> res_occ;
    cf_monokmers_shape shape{};
    shape.n_strings = n_strings;
    shape.n_letters = N;
    shape.k = k;
    shape.min_mult = min_mult;
    shape.with_positions = with_positions ? 1 : 0;
    auto finish = [&]() {
        if (n_kmers_out) *n_kmers_out = (int64_t)res_first.size();
        if (ms_out) *ms_out = shape.phase_ms[3];
        shape.n_kmers = (int64_t)res_first.size();
        shape.n_occ = (int64_t)res_occ.size();
        ctx->monokmers_first.swap(res_first);
        ctx->monokmers_ptr.swap(res_ptr);
        ctx->monokmers_occ.swap(res_occ);
        ctx->monokmers_last = shape;
        ctx->monokmers_have = true;
        return 0;
    };
    if (N == 0 || k > N) return finish();      // no string holds a window

    CF_HIP(hipSetDevice(ctx->device));
    hipEvent_t e0 = ctx->ev0, e1 = ctx->ev1, e2 = ctx->ev2, e3 = ctx->ev3;
    float t = 0.f, sort_ms = 0.f, copy_ms = 0.f;
    const int cap = cf_mk_launch_cap(ctx);
    const size_t n = (size_t)N, n4 = (n + 3) & ~(size_t)3;
    auto grid = [&](int64_t items) { return dim3((unsigned)cf_grid_for(items, CF_MK_BLOCK, cap)); };
    cf_scratch tmp(ctx);
    uint8_t* d_bytes = nullptr;
    int64_t* d_off = nullptr;
    CF_HIP(hipEventRecord(e0, ctx->stream));
    CF_TRY(tmp.get(&d_bytes, n4 + 16, "monokmers letters"));
    CF_TRY(tmp.get(&d_off, (size_t)n_strings + 1, "monokmers offsets"));
    CF_HIP(hipMemsetAsync(d_bytes + n, 0, n4 + 16 - n, ctx->stream));
    CF_TRY(cf_copy_h2d(ctx, d_bytes, bytes + off[0], n));
    CF_TRY(cf_copy_h2d(ctx, d_off, off, ((size_t)n_strings + 1) * 8));
    CF_HIP(hipEventRecord(e1, ctx->stream));
    CF_HIP(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&t, e0, e1); copy_ms += t;

    cf_mk_ranked rk{};
    CF_TRY(cf_mk_rank_windows(ctx, tmp, d_bytes, d_off, n_strings, N, k, gap, "cf_monokmers_run", &rk));
    cf_mk_rec *d_rec = rk.rec, *d_rec2 = rk.rec2;
    uint32_t* d_head = rk.head;
    int64_t *d_e = rk.e, *d_scalar = rk.scalar;
    const int64_t n_valid = rk.n_valid, n_classes = rk.n_classes;
    sort_ms = rk.sort_ms;
    shape.n_rounds = rk.n_rounds;
    shape.n_sorts = rk.n_sorts;
    shape.n_sort_passes = rk.n_sort_passes;
    shape.n_windows = n_valid;      // (a break in front of the last round leaves 0)
    shape.n_distinct = n_valid ? n_classes : 0;

    if (shape.n_windows > 0) {
        const int64_t D = n_classes, V = n_valid;
        tmp.drop(d_rec2);
        d_rec2 = nullptr;
        cf_mk_rec *d_cls = nullptr, *d_cls2 = nullptr;
        uint32_t *d_seg = nullptr, *d_cnt = nullptr;
        int32_t* d_rank = nullptr;
        cf_monokmer* d_out = nullptr;
        int64_t* d_ptr = nullptr;
        CF_TRY(tmp.get(&d_cls, (size_t)D, "monokmers classes"));
        CF_TRY(tmp.get(&d_cls2, (size_t)D, "monokmers class sort buffer"));
        CF_TRY(tmp.get(&d_seg, (size_t)D + 1, "monokmers class starts"));
        CF_TRY(tmp.get(&d_cnt, (size_t)D, "monokmers counts"));
        CF_TRY(tmp.get(&d_rank, (size_t)D, "monokmers output ranks"));
        CF_TRY(tmp.get(&d_out, (size_t)D, "monokmers output"));
        CF_TRY(tmp.get(&d_ptr, (size_t)D + 1, "monokmers occurrence offsets"));
        hipLaunchKernelGGL(cf_mk_classes, grid(V), dim3(CF_MK_BLOCK), 0, ctx->stream, (const cf_mk_rec*)d_rec, (const uint32_t*)d_head, (const int64_t*)d_e, d_cls,
                           d_seg, V, D);
        CF_KERNEL_CHECK("cf_mk_classes");
        const uint32_t mm = (uint32_t)std::min<int64_t>(min_mult, (int64_t)1 << 31), sentinel = (uint32_t)N;
        hipLaunchKernelGGL(cf_mk_filter, grid(D), dim3(CF_MK_BLOCK), 0, ctx->stream, d_cls, (const uint32_t*)d_seg, D, mm, sentinel);
        CF_KERNEL_CHECK("cf_mk_filter");
        const int words[1] = {0}, bits[1] = {cf_mk_bits((uint64_t)N)};
        CF_HIP(hipEventRecord(e2, ctx->stream));
        CF_TRY(cf_radix_sort_rec16(ctx, d_cls, d_cls2, D, words, bits, 1));
        CF_HIP(hipEventRecord(e3, ctx->stream));
        CF_HIP(hipEventSynchronize(e3));
        (void)hipEventElapsedTime(&t, e2, e3); sort_ms += t;
        ++shape.n_sorts;
        shape.n_sort_passes += (bits[0] + 7) / 8;
        CF_HIP(hipMemsetAsync(d_scalar, 0, 16, ctx->stream));
        hipLaunchKernelGGL(cf_mk_emit, grid(D), dim3(CF_MK_BLOCK), 0, ctx->stream, (const cf_mk_rec*)d_cls, D, sentinel, (const int64_t*)d_off, n_strings, d_out,
                           d_rank, d_cnt, d_scalar);
        CF_KERNEL_CHECK("cf_mk_emit");
        int64_t K = 0, n_occ = 0;
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_cnt, d_ptr, D, &n_occ));
        CF_TRY(cf_copy_d2h(ctx, &K, d_scalar, 8));
        if (K < 0 || K > D || n_occ < 0 || n_occ > V) return cf_fail(ctx, -5, "cf_monokmers_run: the kept classes do not add up (internal error)");
        res_first.resize((size_t)K);
        CF_HIP(hipEventRecord(e2, ctx->stream));
        if (K > 0) CF_TRY(cf_copy_d2h(ctx, res_first.data(), d_out, (size_t)K * sizeof(cf_monokmer)));
        CF_HIP(hipEventRecord(e3, ctx->stream));
        CF_HIP(hipEventSynchronize(e3));
        (void)hipEventElapsedTime(&t, e2, e3); copy_ms += t;
        if (with_positions && K > 0) {
            cf_monokmer_occ* d_occ = nullptr;
            CF_TRY(tmp.get(&d_occ, (size_t)n_occ, "monokmers occurrences"));
            hipLaunchKernelGGL(cf_mk_occ, grid(V), dim3(CF_MK_BLOCK), 0, ctx->stream, (const cf_mk_rec*)d_rec, (const uint32_t*)d_head, (const int64_t*)d_e, V,
                               (const uint32_t*)d_seg, (const int32_t*)d_rank, D, (const int64_t*)d_ptr, K, n_occ, (const int64_t*)d_off, n_strings, d_occ);
            CF_KERNEL_CHECK("cf_mk_occ");
            res_ptr.assign((size_t)K + 1, 0);
            res_occ.resize((size_t)n_occ);
            CF_HIP(hipEventRecord(e2, ctx->stream));
            CF_TRY(cf_copy_d2h(ctx, res_ptr.data(), d_ptr, (size_t)K * 8));
            res_ptr[(size_t)K] = n_occ;
            CF_TRY(cf_copy_d2h(ctx, res_occ.data(), d_occ, (size_t)n_occ * sizeof(cf_monokmer_occ)));
            CF_HIP(hipEventRecord(e3, ctx->stream));
            CF_HIP(hipEventSynchronize(e3));
            (void)hipEventElapsedTime(&t, e2, e3); copy_ms += t;
        }
    }
    CF_HIP(hipEventRecord(e1, ctx->stream));
    CF_HIP(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&t, e0, e1);
    shape.phase_ms[0] = copy_ms;
    shape.phase_ms[1] = sort_ms;
    shape.phase_ms[2] = std::max(0.f, t - copy_ms - sort_ms);
    shape.phase_ms[3] = t;
    return finish();
}

}  // extern "C"
