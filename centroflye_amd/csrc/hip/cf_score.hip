// cf_score.hip — the EXACT scorer of a frozen cloud contig, in one batch (gfx950, wave64).
//
// Reference: scripts/cloud_contig.py:46-76 (CloudContig.calc_inters_score), :98-114 (map_reads, built on it), :146-155 (the
// cross-check of map_reads_fast(debug=True)) and :78-84 (get_spread_kmers).  cf_map.hip seeds from EVERY position of a frequent
// k-mer (kmer_positions, :33); the exact scorer intersects unit i of a read laid at start s with freq_clouds[s + i], the k-mers
// that are frequent AT that position (:35-36, :60-61).  cf_contig_build keeps those pairs as a second CSR by rank (exact_ptr,
// exact_pos: the ascending positions p with count[(p, x)] >= f).
//
//   cf_score_reads    one wave per query read with its own range of starts [lo, hi].  Only the starts lo .. min(hi, max_pos)
//                     can have a hit (every position of the CSR is <= max_pos, which is also what truncates a read that
//                     overhangs the contig, :57).  They are scored in windows of `map_window` LDS slots as in cf_map_kernel —
//                     units in ascending order, a per-slot stamp tells a unit's first hit (s0), every hit adds to s1 — but a
//                     lane takes from the row of its rank only the positions that land in the window: it SEARCHES the row for
//                     the first position >= window start + i and walks on from there.  A range that fits one window is one pass
//                     over the read's entries (rescoring a placed read: lo = hi = its position); a wider one first finds the
//                     span of starts with a hit, by two searches per entry, and takes the windows of that span only.
//                     The winner is the maximum of (s0, s1, s) among the starts with s0 >= t0 and s1 >= t1 (:71-75, the
//                     rightmost of equals).  A start without a hit scores (0, 0) and qualifies only when t0 <= 0 and t1 <= 0;
//                     the rightmost of those is hi itself, and it wins only when no start has a hit.
//   cf_contig_spread  the ranks whose row of the all-positions CSR is longer than max_npos: flag, scan, write — ascending.
#include "cf_common.h"

#define CF_SCORE_THREADS 64
#define CF_SCORE_WINDOW_DEFAULT 2048      // (cf_map.hip's default: the same knob sizes both)

// (key, start) <- the better of the two, by selects (profiles/r03_place_miscompile.md: no `if (better) mine = other`)
__device__ __forceinline__ void cf_score_take(unsigned long long& key, long long& start, unsigned long long okey, long long ostart) {
    const bool take = okey > key || (okey == key && ostart > start);
    key = take ? okey : key;
    start = take ? ostart : start;
}

// first j in [a, b) with pos[j] >= key (b when there is none)
__device__ __forceinline__ int64_t cf_score_lower(const int32_t* __restrict__ pos, int64_t a, int64_t b, long long key) {
    while (a < b) {
        const int64_t mid = (a + b) >> 1;
        if ((long long)pos[mid] < key) a = mid + 1; else b = mid;
    }
    return a;
}

__global__ void __launch_bounds__(CF_SCORE_THREADS)
cf_score_kernel(const int64_t* __restrict__ qreads, int64_t nq, const int64_t* __restrict__ qlo, const int64_t* __restrict__ qhi,
                const int64_t* __restrict__ unit_ptr, const int64_t* __restrict__ cloud_ptr, const int32_t* __restrict__ entries,
                const int64_t* __restrict__ xptr, const int32_t* __restrict__ xpos, int64_t max_pos, int W, int32_t t0, int32_t t1,
                int64_t* __restrict__ out_pos, int32_t* __restrict__ out_s0, int32_t* __restrict__ out_s1) {
    unsigned long long* score = (unsigned long long*)cf_lds;      // W x (s0 << 32 | s1)
    uint32_t* stamp = (uint32_t*)(cf_lds + (size_t)W * 8);         // W x (1 + the last unit that hit the slot)
    const int lane = threadIdx.x;
    for (int64_t qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const int64_t r = qreads ? qreads[qi] : qi;
        const int64_t u0 = unit_ptr[r], u1 = unit_ptr[r + 1], n = u1 - u0;
        const long long lo = qlo ? (long long)qlo[qi] : 0ll;
        const long long hi = qhi ? (long long)qhi[qi] : (long long)(max_pos - n + 1);      // (map_reads' range, :103)
        const long long top = hi < (long long)max_pos ? hi : (long long)max_pos;           // the last start that can have a hit
        unsigned long long best = 0;                    // s0 << 32 | s1 of the best start WITH a hit (0: none)
        long long best_s = -1;
        if (n > 0 && lo <= top) {
            long long smin = lo, smax = top;
            if (top - lo >= (long long)W) {
                // more than one window: the span of starts that have a hit, two searches per entry
                smin = 0x7fffffffffffffffll, smax = -1;
                for (int64_t u = u0; u < u1; ++u) {
                    const long long i = (long long)(u - u0);
                    const int64_t e1 = cloud_ptr[u + 1];
                    for (int64_t e = cloud_ptr[u] + lane; e < e1; e += 64) {
                        const int32_t x = entries[e];
                        const int64_t j1 = xptr[x + 1];
                        const int64_t a = cf_score_lower(xpos, xptr[x], j1, lo + i);          // first position >= lo + i
                        const int64_t b = cf_score_lower(xpos, a, j1, top + i + 1);           // first position > top + i
                        const bool any = b > a;
                        const long long first = any ? (long long)xpos[a] - i : smin;
                        const long long last = any ? (long long)xpos[b - 1] - i : smax;
                        smin = first < smin ? first : smin;
                        smax = last > smax ? last : smax;
                    }
                }
                for (int d = 32; d >= 1; d >>= 1) {
                    const long long a = __shfl_xor(smin, d), b = __shfl_xor(smax, d);
                    smin = a < smin ? a : smin;
                    smax = b > smax ? b : smax;
                }
            }
            for (long long wlo = smin; wlo <= smax; wlo += W) {
                const long long whi = (wlo + W <= smax + 1) ? wlo + W : smax + 1;      // starts [wlo, whi) of this window
                const int nslot = (int)(whi - wlo);
                for (int j = lane; j < nslot; j += 64) { score[j] = 0ull; stamp[j] = 0u; }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int64_t u = u0; u < u1; ++u) {
                    const long long i = (long long)(u - u0);
                    const uint32_t mark = (uint32_t)i + 1u;
                    const int64_t e1 = cloud_ptr[u + 1];
                    for (int64_t e = cloud_ptr[u] + lane; e < e1; e += 64) {
                        const int32_t x = entries[e];
                        const int64_t j1 = xptr[x + 1];
                        // the part of the row that lands in this window: positions wlo + i .. whi + i - 1
                        for (int64_t j = cf_score_lower(xpos, xptr[x], j1, wlo + i); j < j1; ++j) {
                            const long long s = (long long)xpos[j] - i;
                            if (s >= whi) break;
                            const int slot = (int)(s - wlo);
                            const uint32_t old = atomicMax(&stamp[slot], mark);      // units come in ascending order: old < mark <=> first hit of unit i here
                            atomicAdd(&score[slot], (old < mark ? (1ull << 32) : 0ull) + 1ull);
                        }
                    }
                    // the stamps of unit i are final before a lane begins unit i + 1
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                for (int j = lane; j < nslot; j += 64) {
                    const unsigned long long key = score[j];
                    const long long s0 = (long long)(key >> 32), s1 = (long long)(key & 0xffffffffull);
                    const bool ok = s1 > 0 && s0 >= (long long)t0 && s1 >= (long long)t1;
                    cf_score_take(best, best_s, ok ? key : 0ull, ok ? wlo + j : -1ll);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long ok = __shfl_xor(best, d);
                const long long os = __shfl_xor(best_s, d);
                cf_score_take(best, best_s, ok, os);
            }
        }
        if (lane == 0) {
            // a start without a hit scores (0, 0): it qualifies under thresholds <= 0 only, loses to any start with a hit, and
            // the rightmost of them is hi (also for a read without units, and beyond max_pos)
            const bool hit = best_s >= 0;
            const bool free_start = !hit && t0 <= 0 && t1 <= 0 && lo <= hi;
            out_pos[qi] = hit ? best_s : (free_start ? hi : -1ll);
            out_s0[qi] = hit ? (int32_t)(best >> 32) : 0;
            out_s1[qi] = hit ? (int32_t)(best & 0xffffffffull) : 0;
        }
    }
}

// ------------------------------------------------------------------ spread k-mers
// flag[k] = the row of rank k (every position of a frequent k-mer; empty for the others) is longer than m >= 0
__global__ void __launch_bounds__(256)
cf_spread_flag_kernel(const int64_t* __restrict__ cptr, int64_t K, int64_t m, uint32_t* __restrict__ flag) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x)
        flag[k] = (cptr[k + 1] - cptr[k] > m) ? 1u : 0u;
}

__global__ void __launch_bounds__(256)
cf_spread_fill_kernel(const uint32_t* __restrict__ flag, const int64_t* __restrict__ idx, int64_t K, int32_t* __restrict__ ranks) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x)
        if (flag[k]) ranks[idx[k]] = (int32_t)k;
}

extern "C" {

int cf_score_reads(cf_ctx* ctx, const int64_t* reads, int64_t n, const int64_t* lo, const int64_t* hi, int32_t min_unit,
                   int32_t min_inters, int64_t* out_pos, int32_t* out_s0, int32_t* out_s1) {
    if (!ctx) return -22;
    if (!ctx->have_clouds) return cf_fail(ctx, -22, "cf_score_reads: no clouds installed");
    if (!ctx->have_contig) return cf_fail(ctx, -22, "cf_score_reads: no contig built (cf_contig_build)");
    const int64_t R = ctx->n_reads;
    if (!reads) n = R;
    if (n < 0) return cf_fail(ctx, -22, "cf_score_reads: negative number of reads");
    if (n > 0 && (!out_pos || !out_s0 || !out_s1)) return cf_fail(ctx, -22, "cf_score_reads: null output");
    for (int64_t i = 0; reads && i < n; ++i)
        if (reads[i] < 0 || reads[i] >= R) return cf_fail(ctx, -22, "cf_score_reads: read " + std::to_string(reads[i]) + " is out of range");
    for (int64_t i = 0; lo && i < n; ++i)
        if (lo[i] < 0) return cf_fail(ctx, -22, "cf_score_reads: negative first start " + std::to_string(lo[i]) + " of query " + std::to_string(i));
    if (n == 0) { ctx->score_ms = 0.f; return 0; }
    CF_HIP(hipSetDevice(ctx->device));
    CF_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    const int W = ctx->map_window > 0 ? ctx->map_window : CF_SCORE_WINDOW_DEFAULT;
    int64_t *d_q = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_pos = nullptr;
    int32_t *d_s0 = nullptr, *d_s1 = nullptr;
    cf_scratch tmp(ctx);
    if (reads) {
        CF_TRY(tmp.get(&d_q, (size_t)n, "query reads"));
        CF_TRY(cf_copy_h2d(ctx, d_q, reads, (size_t)n * 8));
    }
    if (lo) {
        CF_TRY(tmp.get(&d_lo, (size_t)n, "first starts"));
        CF_TRY(cf_copy_h2d(ctx, d_lo, lo, (size_t)n * 8));
    }
    if (hi) {
        CF_TRY(tmp.get(&d_hi, (size_t)n, "last starts"));
        CF_TRY(cf_copy_h2d(ctx, d_hi, hi, (size_t)n * 8));
    }
    CF_TRY(tmp.get(&d_pos, (size_t)n, "scored positions"));
    CF_TRY(tmp.get(&d_s0, (size_t)n, "scored s0"));
    CF_TRY(tmp.get(&d_s1, (size_t)n, "scored s1"));
    const int grid = (int)std::min<int64_t>(n, (int64_t)std::max(1, ctx->n_cu) * 64);
    hipLaunchKernelGGL(cf_score_kernel, dim3((unsigned)grid), dim3(CF_SCORE_THREADS), (size_t)W * 12, ctx->stream, (const int64_t*)d_q, n,
                       (const int64_t*)d_lo, (const int64_t*)d_hi, (const int64_t*)ctx->d_unit_ptr, (const int64_t*)ctx->d_cloud_ptr,
                       (const int32_t*)ctx->d_entries, (const int64_t*)ctx->d_exact_ptr, (const int32_t*)ctx->d_exact_pos,
                       ctx->contig_max_pos, W, min_unit, min_inters, d_pos, d_s0, d_s1);
    CF_KERNEL_CHECK("cf_score_kernel");
    CF_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    CF_HIP(hipEventSynchronize(ctx->ev1));
    (void)hipEventElapsedTime(&ctx->score_ms, ctx->ev0, ctx->ev1);
    CF_TRY(cf_copy_d2h(ctx, out_pos, d_pos, (size_t)n * 8));
    CF_TRY(cf_copy_d2h(ctx, out_s0, d_s0, (size_t)n * 4));
    return cf_copy_d2h(ctx, out_s1, d_s1, (size_t)n * 4);
}

int cf_contig_spread(cf_ctx* ctx, int64_t max_npos, int32_t* ranks, int64_t cap, int64_t* n_out) {
    if (!ctx) return -22;
    if (!ctx->have_contig) return cf_fail(ctx, -22, "cf_contig_spread: no contig built (cf_contig_build)");
    if (!n_out) return cf_fail(ctx, -22, "cf_contig_spread: null count");
    if (cap < 0) return cf_fail(ctx, -22, "cf_contig_spread: negative capacity");
    const int64_t K = ctx->contig_K;
    *n_out = 0;
    if (K == 0) return 0;
    CF_HIP(hipSetDevice(ctx->device));
    const int grid = cf_grid_for(K, 256, std::max(1, ctx->n_cu) * 32);
    uint32_t* d_flag = nullptr;
    int64_t* d_idx = nullptr;
    int32_t* d_ranks = nullptr;
    int64_t total = 0;
    cf_scratch tmp(ctx);
    CF_TRY(tmp.get(&d_flag, (size_t)K, "spread flags"));
    CF_TRY(tmp.get(&d_idx, (size_t)K, "spread offsets"));
    // a frequent k-mer has at least one position, the other ranks have an empty row: max_npos < 0 asks for every frequent one
    hipLaunchKernelGGL(cf_spread_flag_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const int64_t*)ctx->d_contig_ptr, K,
                       std::max<int64_t>(0, max_npos), d_flag);
    CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_flag, d_idx, K, &total));
    *n_out = total;
    if (!ranks || total == 0) return 0;      // the count alone
    if (cap < total) return cf_fail(ctx, -22, "cf_contig_spread: " + std::to_string(total) + " ranks do not fit the buffer");
    CF_TRY(tmp.get(&d_ranks, (size_t)total, "spread ranks"));
    hipLaunchKernelGGL(cf_spread_fill_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const uint32_t*)d_flag, (const int64_t*)d_idx,
                       K, d_ranks);
    CF_KERNEL_CHECK("cf_spread_fill_kernel");
    return cf_copy_d2h(ctx, ranks, d_ranks, (size_t)total * 4);
}

int cf_contig_exact_info(cf_ctx* ctx, int64_t* n_exact_pairs, float* score_ms) {
    if (!ctx) return -22;
    if (!ctx->have_contig) return cf_fail(ctx, -22, "cf_contig_exact_info: no contig built (cf_contig_build)");
    if (n_exact_pairs) *n_exact_pairs = ctx->exact_pairs;
    if (score_ms) *score_ms = ctx->score_ms;
    return 0;
}

}  // extern "C"
