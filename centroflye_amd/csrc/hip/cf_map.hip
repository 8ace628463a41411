// cf_map.hip — batch mapping of reads onto a FROZEN cloud contig (gfx950, wave64).
//
// Reference: scripts/cloud_contig.py:26-41 (CloudContig.add_read, called once per backbone read) and :117-156
// (map_reads_fast with update_mapping_scores, :87-95).  The greedy placer (cf_place*.hip) runs R dependent iterations;
// mapping against a contig that no longer changes has no dependency between reads, so it is one sort and one kernel.
//
//   cf_contig_build   one record [rank | position] per cloud entry of a backbone read -> radix sort (cf_prims.hip) ->
//                     runs of equal records are the counts count[(p, x)]; a rank is FREQUENT when some run is at least
//                     max(1, f) long; the distinct positions of every frequent rank — also those where it is not frequent,
//                     cloud_contig.py:33 / :126-128 — become one CSR row, ascending; rows of other ranks are empty.
//                     Coverage counts units, so a unit with an empty cloud still covers its position (:31), and
//                     P = the number of covered positions (len(cloud_contig.clouds)), which is not max_pos + 1 when the
//                     coverage has a gap.  From the same sorted records a second CSR keeps only the positions where the rank
//                     IS frequent (a run of at least f records: freq_clouds, :35-36) for the exact scorer of cf_score.hip.
//   cf_map_reads      one wave per query read.  The candidate starts s = q - i of the read (q a contig position of a k-mer of
//                     unit i, q >= i, s + n <= P) are scored in windows of `map_window` LDS slots indexed by s - lo: the units
//                     are taken one after another, a per-slot stamp (last unit seen, by a returning max) tells whether a hit
//                     is the unit's first for that start (s0), every hit adds to s1.  A first pass finds the span of starts
//                     that have a hit at all, so a read whose hits cluster takes one window whatever P is.  The winner is the
//                     maximum of (s0, s1, s) among the starts with s0 >= t0 and s1 >= t1 (:137-143).
// Nothing here is sized by a table that could overflow: the records, the CSR and the coverage are exact-size device arrays,
// and a contig longer than one window is scored in as many windows as its hits span.
#include "cf_common.h"

#define CF_MAP_THREADS 64
#define CF_MAP_WINDOW_DEFAULT 2048

void cf_free_contig(cf_ctx* c) {
    cf_release_t(c, c->d_contig_ptr, (size_t)c->contig_K + 1);
    cf_release_t(c, c->d_contig_pos, (size_t)c->contig_pairs);
    cf_release_t(c, c->d_contig_cov, (size_t)c->contig_cov_n);
    cf_release_t(c, c->d_exact_ptr, (size_t)c->contig_K + 1);
    cf_release_t(c, c->d_exact_pos, (size_t)c->exact_pairs);
    c->exact_pairs = 0;
    c->contig_K = c->contig_pairs = c->contig_cov_n = 0;
    c->contig_P = c->contig_max_pos = c->contig_n_freq = 0;
    c->have_contig = false;
}

// ------------------------------------------------------------------ contig build
// cloud entries of each backbone read (its clouds are one contiguous CSR range)
__global__ void __launch_bounds__(256)
cf_contig_sizes_kernel(const int64_t* __restrict__ breads, int64_t n, const int64_t* __restrict__ unit_ptr,
                       const int64_t* __restrict__ cloud_ptr, int64_t* __restrict__ sizes) {
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < n; b += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = breads[b];
        sizes[b] = cloud_ptr[unit_ptr[r + 1]] - cloud_ptr[unit_ptr[r]];
    }
}

// one wave per backbone read: a record (rank << pbits | pos + i) per cloud entry, and one coverage count per unit
__global__ void __launch_bounds__(256)
cf_contig_emit_kernel(const int64_t* __restrict__ breads, const int64_t* __restrict__ bpos, int64_t n,
                      const int64_t* __restrict__ unit_ptr, const int64_t* __restrict__ cloud_ptr,
                      const int32_t* __restrict__ entries, const int64_t* __restrict__ rec_off, int pbits,
                      unsigned long long* __restrict__ recs, int32_t* __restrict__ cov) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; b < n; b += waves) {
        const int64_t r = breads[b], pos = bpos[b];
        const int64_t u0 = unit_ptr[r], u1 = unit_ptr[r + 1];
        for (int64_t i = lane; i < u1 - u0; i += 64) atomicAdd(&cov[pos + i], 1);
        const int64_t e0 = cloud_ptr[u0], e1 = cloud_ptr[u1], off = rec_off[b];
        for (int64_t e = e0 + lane; e < e1; e += 64) {
            // the unit of entry e: the last u in [u0, u1) with cloud_ptr[u] <= e (empty clouds share their successor's offset)
            int64_t lo = u0, hi = u1;
            while (hi - lo > 1) {
                const int64_t mid = (lo + hi) >> 1;
                if (cloud_ptr[mid] <= e) lo = mid; else hi = mid;
            }
            recs[off + (e - e0)] = ((unsigned long long)(uint32_t)entries[e] << pbits) | (unsigned long long)(pos + (lo - u0));
        }
    }
}

// a run of equal records that is at least f long makes its rank frequent: the head of a run sees it f - 1 records on
__global__ void __launch_bounds__(256)
cf_contig_freq_kernel(const unsigned long long* __restrict__ recs, int64_t n, int64_t f, int pbits, uint32_t* __restrict__ freq) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long x = recs[i];
        const bool head = i == 0 || recs[i - 1] != x;
        if (head && f - 1 < n - i && recs[i + (f - 1)] == x) freq[x >> pbits] = 1u;      // (every writer stores the same 1)
    }
}

// flag[i] = record i is the first of its (rank, position) and the rank is frequent: one entry of the CSR
__global__ void __launch_bounds__(256)
cf_contig_flag_kernel(const unsigned long long* __restrict__ recs, int64_t n, int pbits, const uint32_t* __restrict__ freq,
                      uint32_t* __restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long x = recs[i];
        const bool head = i == 0 || recs[i - 1] != x;
        flag[i] = (head && freq[x >> pbits]) ? 1u : 0u;
    }
}

// flag[i] = record i is the first of a run that is at least f long: (rank, position) is an entry of freq_clouds, one entry of
// the exact CSR (the test of cf_contig_freq_kernel, kept per position instead of per rank)
__global__ void __launch_bounds__(256)
cf_contig_exact_flag_kernel(const unsigned long long* __restrict__ recs, int64_t n, int64_t f, uint32_t* __restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long x = recs[i];
        const bool head = i == 0 || recs[i - 1] != x;
        flag[i] = (head && f - 1 < n - i && recs[i + (f - 1)] == x) ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(256)
cf_contig_fill_kernel(const unsigned long long* __restrict__ recs, int64_t n, int pbits, const uint32_t* __restrict__ flag,
                      const int64_t* __restrict__ idx, int32_t* __restrict__ cpos) {
    const unsigned long long pmask = (1ull << pbits) - 1ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (flag[i]) cpos[idx[i]] = (int32_t)(recs[i] & pmask);
}

// contig_ptr[k] = CSR entries of the ranks below k = idx of the first record with rank >= k (idx counts the flags before it);
// first[k] = that record itself, for the second CSR over the same records (cf_contig_ptr_of_first_kernel)
__global__ void __launch_bounds__(256)
cf_contig_ptr_kernel(const unsigned long long* __restrict__ recs, int64_t n, int pbits, const int64_t* __restrict__ idx,
                     int64_t n_pairs, int64_t K, int64_t* __restrict__ cptr, int64_t* __restrict__ first) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= K; k += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long key = (unsigned long long)k << pbits;
        int64_t lo = 0, hi = n;      // first record >= key
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (recs[mid] < key) lo = mid + 1; else hi = mid;
        }
        cptr[k] = lo < n ? idx[lo] : n_pairs;
        first[k] = lo;
    }
}

// ptr[k]: the first record with rank >= k (found above) -> the offset of another scan at that record: no second search
__global__ void __launch_bounds__(256)
cf_contig_ptr_of_first_kernel(int64_t* __restrict__ ptr, int64_t K, int64_t n, const int64_t* __restrict__ idx, int64_t n_pairs) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= K; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = ptr[k];
        ptr[k] = lo < n ? idx[lo] : n_pairs;
    }
}

// out[0] += number of non-zero words of a[0 .. n): one atomic per workgroup
__global__ void __launch_bounds__(256)
cf_contig_nonzero_kernel(const uint32_t* __restrict__ a, int64_t n, unsigned long long* __restrict__ out) {
    unsigned long long* sh = (unsigned long long*)cf_lds;      // 4 wave totals
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) c += a[i] != 0u;
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (unsigned w = 0; w < (blockDim.x >> 6); ++w) t += sh[w];
        if (t) atomicAdd(out, t);
    }
}

// ------------------------------------------------------------------ map kernel
// (key, start) <- the better of the two, by selects (profiles/r03_place_miscompile.md: no `if (better) mine = other`)
__device__ __forceinline__ void cf_map_take(unsigned long long& key, long long& start, unsigned long long okey, long long ostart) {
    const bool take = okey > key || (okey == key && ostart > start);
    key = take ? okey : key;
    start = take ? ostart : start;
}

__global__ void __launch_bounds__(CF_MAP_THREADS)
cf_map_kernel(const int64_t* __restrict__ qreads, int64_t nq, const int64_t* __restrict__ unit_ptr,
              const int64_t* __restrict__ cloud_ptr, const int32_t* __restrict__ entries,
              const int64_t* __restrict__ cptr, const int32_t* __restrict__ cpos, int64_t P, int W, int32_t t0, int32_t t1,
              int64_t* __restrict__ out_pos, int32_t* __restrict__ out_s0, int32_t* __restrict__ out_s1) {
    unsigned long long* score = (unsigned long long*)cf_lds;      // W x (s0 << 32 | s1)
    uint32_t* stamp = (uint32_t*)(cf_lds + (size_t)W * 8);         // W x (1 + the last unit that hit the slot)
    const int lane = threadIdx.x;
    for (int64_t qi = blockIdx.x; qi < nq; qi += gridDim.x) {
        const int64_t r = qreads ? qreads[qi] : qi;
        const int64_t u0 = unit_ptr[r], u1 = unit_ptr[r + 1], n = u1 - u0;
        const long long last = (long long)(P - n);      // the largest start with s + n <= P
        unsigned long long best = 0;                    // s0 << 32 | s1 of the winner (0: none — a start needs a hit)
        long long best_s = -1;
        if (n > 0 && last >= 0) {
            // the span of starts that have a hit
            long long smin = 0x7fffffffffffffffll, smax = -1;
            for (int64_t u = u0; u < u1; ++u) {
                const long long i = (long long)(u - u0);
                const int64_t e1 = cloud_ptr[u + 1];
                for (int64_t e = cloud_ptr[u] + lane; e < e1; e += 64) {
                    const int32_t x = entries[e];
                    const int64_t j1 = cptr[x + 1];
                    for (int64_t j = cptr[x]; j < j1; ++j) {
                        const long long s = (long long)cpos[j] - i;
                        const bool in = s >= 0 && s <= last;
                        smin = (in && s < smin) ? s : smin;
                        smax = (in && s > smax) ? s : smax;
                    }
                }
            }
            for (int d = 32; d >= 1; d >>= 1) {
                const long long a = __shfl_xor(smin, d), b = __shfl_xor(smax, d);
                smin = a < smin ? a : smin;
                smax = b > smax ? b : smax;
            }
            for (long long lo = smin; lo <= smax; lo += W) {
                const long long hi = (lo + W <= smax + 1) ? lo + W : smax + 1;      // starts [lo, hi) of this window
                const int nslot = (int)(hi - lo);
                for (int j = lane; j < nslot; j += 64) { score[j] = 0ull; stamp[j] = 0u; }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int64_t u = u0; u < u1; ++u) {
                    const long long i = (long long)(u - u0);
                    const uint32_t mark = (uint32_t)i + 1u;
                    const int64_t e1 = cloud_ptr[u + 1];
                    for (int64_t e = cloud_ptr[u] + lane; e < e1; e += 64) {
                        const int32_t x = entries[e];
                        const int64_t j1 = cptr[x + 1];
                        for (int64_t j = cptr[x]; j < j1; ++j) {
                            const long long s = (long long)cpos[j] - i;
                            if (s >= lo && s < hi) {
                                const int slot = (int)(s - lo);
                                const uint32_t old = atomicMax(&stamp[slot], mark);      // units come in ascending order: old < mark <=> first hit of unit i here
                                atomicAdd(&score[slot], (old < mark ? (1ull << 32) : 0ull) + 1ull);
                            }
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
                    cf_map_take(best, best_s, ok ? key : 0ull, ok ? lo + j : -1ll);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long ok = __shfl_xor(best, d);
                const long long os = __shfl_xor(best_s, d);
                cf_map_take(best, best_s, ok, os);
            }
        }
        if (lane == 0) {
            out_pos[qi] = best_s;
            out_s0[qi] = best_s >= 0 ? (int32_t)(best >> 32) : 0;
            out_s1[qi] = best_s >= 0 ? (int32_t)(best & 0xffffffffull) : 0;
        }
    }
}

// ------------------------------------------------------------------ host side
static int cf_bits_for(int64_t max_value) {      // bits that hold 0 .. max_value (at least 1)
    int b = 1;
    while (b < 62 && ((int64_t)1 << b) <= max_value) ++b;
    return b;
}

static int contig_build(cf_ctx* ctx, const int64_t* reads, const int64_t* pos, int64_t n, int64_t f, int64_t max_pos, bool covered) {
    const int64_t K = ctx->n_kmers;
    const int pbits = cf_bits_for(max_pos), kbits = cf_bits_for(std::max<int64_t>(K - 1, 0));
    const int max_grid = std::max(1, ctx->n_cu) * 8;
    int64_t *d_breads = nullptr, *d_bpos = nullptr, *d_sizes = nullptr, *d_off = nullptr, *d_idx = nullptr;
    unsigned long long *d_recs = nullptr, *d_tmp = nullptr, *d_counts = nullptr, *sorted = nullptr;
    uint32_t *d_freq = nullptr, *d_flag = nullptr;
    int64_t n_rec = 0, n_pairs = 0, n_exact = 0;
    unsigned long long h_counts[2] = {0, 0};
    ctx->contig_K = K;
    ctx->contig_cov_n = covered ? max_pos + 1 : 0;
    cf_scratch tmp(ctx);
    CF_TRY(cf_alloc_t(ctx, &ctx->d_contig_ptr, (size_t)K + 1, "contig_ptr"));
    CF_TRY(cf_alloc_t(ctx, &ctx->d_contig_cov, (size_t)ctx->contig_cov_n, "contig coverage"));
    CF_TRY(cf_alloc_t(ctx, &ctx->d_exact_ptr, (size_t)K + 1, "exact contig_ptr"));
    CF_TRY(tmp.get(&d_freq, (size_t)K + 1, "frequent ranks"));
    CF_TRY(tmp.get(&d_counts, 2, "contig counters"));
    CF_HIP(hipMemsetAsync(ctx->d_contig_ptr, 0, (size_t)(K + 1) * 8, ctx->stream));
    if (ctx->contig_cov_n) CF_HIP(hipMemsetAsync(ctx->d_contig_cov, 0, (size_t)ctx->contig_cov_n * 4, ctx->stream));
    CF_HIP(hipMemsetAsync(ctx->d_exact_ptr, 0, (size_t)(K + 1) * 8, ctx->stream));
    CF_HIP(hipMemsetAsync(d_freq, 0, (size_t)(K + 1) * 4, ctx->stream));
    CF_HIP(hipMemsetAsync(d_counts, 0, 16, ctx->stream));
    if (n > 0) {
        CF_TRY(tmp.get(&d_breads, (size_t)n, "backbone reads"));
        CF_TRY(tmp.get(&d_bpos, (size_t)n, "backbone positions"));
        CF_TRY(tmp.get(&d_sizes, (size_t)n, "backbone sizes"));
        CF_TRY(tmp.get(&d_off, (size_t)n, "backbone offsets"));
        CF_TRY(cf_copy_h2d(ctx, d_breads, reads, (size_t)n * 8));
        CF_TRY(cf_copy_h2d(ctx, d_bpos, pos, (size_t)n * 8));
        hipLaunchKernelGGL(cf_contig_sizes_kernel, dim3((unsigned)cf_grid_for(n, 256, max_grid)), dim3(256), 0, ctx->stream,
                           (const int64_t*)d_breads, n, (const int64_t*)ctx->d_unit_ptr, (const int64_t*)ctx->d_cloud_ptr, d_sizes);
        CF_TRY(cf_scan_exclusive_i64(ctx, d_sizes, d_off, n, &n_rec));      // (its total sizes the record buffers)
        CF_TRY(tmp.get(&d_recs, (size_t)n_rec, "contig records"));
        CF_TRY(tmp.get(&d_tmp, (size_t)n_rec, "contig sort scratch"));
        hipLaunchKernelGGL(cf_contig_emit_kernel, dim3((unsigned)cf_grid_for(n * 64, 256, max_grid * 4)), dim3(256), 0, ctx->stream,
                           (const int64_t*)d_breads, (const int64_t*)d_bpos, n, (const int64_t*)ctx->d_unit_ptr,
                           (const int64_t*)ctx->d_cloud_ptr, (const int32_t*)ctx->d_entries, (const int64_t*)d_off, pbits, d_recs,
                           ctx->d_contig_cov);
        CF_KERNEL_CHECK("cf_contig_emit_kernel");
    }
    sorted = d_recs;
    if (n_rec > 0) {
        CF_TRY(cf_radix_sort_u64_any(ctx, d_recs, d_tmp, n_rec, pbits + kbits, &sorted));
        CF_TRY(tmp.get(&d_flag, (size_t)n_rec, "contig flags"));
        CF_TRY(tmp.get(&d_idx, (size_t)n_rec, "contig offsets"));
        const int grid = cf_grid_for(n_rec, 256, max_grid * 4);
        hipLaunchKernelGGL(cf_contig_freq_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const unsigned long long*)sorted, n_rec, f,
                           pbits, d_freq);
        hipLaunchKernelGGL(cf_contig_flag_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const unsigned long long*)sorted, n_rec,
                           pbits, (const uint32_t*)d_freq, d_flag);
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_flag, d_idx, n_rec, &n_pairs));
        ctx->contig_pairs = n_pairs;
        CF_TRY(cf_alloc_t(ctx, &ctx->d_contig_pos, (size_t)n_pairs, "contig positions"));
        if (n_pairs)
            hipLaunchKernelGGL(cf_contig_fill_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const unsigned long long*)sorted, n_rec,
                               pbits, (const uint32_t*)d_flag, (const int64_t*)d_idx, ctx->d_contig_pos);
        hipLaunchKernelGGL(cf_contig_ptr_kernel, dim3((unsigned)cf_grid_for(K + 1, 256, max_grid * 4)), dim3(256), 0, ctx->stream,
                           (const unsigned long long*)sorted, n_rec, pbits, (const int64_t*)d_idx, n_pairs, K, ctx->d_contig_ptr,
                           ctx->d_exact_ptr);
        hipLaunchKernelGGL(cf_contig_nonzero_kernel, dim3((unsigned)cf_grid_for(K, 256, max_grid)), dim3(256), 64, ctx->stream,
                           (const uint32_t*)d_freq, K, d_counts + 1);
        // the exact CSR from the same sorted records; the flags and offsets of the CSR above are done with (stream order)
        hipLaunchKernelGGL(cf_contig_exact_flag_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const unsigned long long*)sorted,
                           n_rec, f, d_flag);
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_flag, d_idx, n_rec, &n_exact));
        ctx->exact_pairs = n_exact;
        CF_TRY(cf_alloc_t(ctx, &ctx->d_exact_pos, (size_t)n_exact, "exact contig positions"));
        if (n_exact)
            hipLaunchKernelGGL(cf_contig_fill_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, (const unsigned long long*)sorted, n_rec,
                               pbits, (const uint32_t*)d_flag, (const int64_t*)d_idx, ctx->d_exact_pos);
        hipLaunchKernelGGL(cf_contig_ptr_of_first_kernel, dim3((unsigned)cf_grid_for(K + 1, 256, max_grid * 4)), dim3(256), 0, ctx->stream,
                           ctx->d_exact_ptr, K, n_rec, (const int64_t*)d_idx, n_exact);
    }
    if (ctx->contig_cov_n)
        hipLaunchKernelGGL(cf_contig_nonzero_kernel, dim3((unsigned)cf_grid_for(ctx->contig_cov_n, 256, max_grid)), dim3(256), 64, ctx->stream,
                           (const uint32_t*)ctx->d_contig_cov, ctx->contig_cov_n, d_counts);
    CF_KERNEL_CHECK("the cf_contig kernels");
    CF_HIP(hipMemcpyAsync(h_counts, d_counts, 16, hipMemcpyDeviceToHost, ctx->stream));
    CF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->contig_P = (int64_t)h_counts[0];
    ctx->contig_n_freq = (int64_t)h_counts[1];
    ctx->contig_max_pos = covered ? max_pos : 0;      // (cloud_contig.py:20-24: 0 for an empty contig)
    ctx->have_contig = true;
    return 0;
}

extern "C" {

int cf_contig_build(cf_ctx* ctx, const int64_t* reads, const int64_t* pos, int64_t n, int32_t min_cloud_kmer_freq) {
    if (!ctx) return -22;
    if (!ctx->have_clouds) return cf_fail(ctx, -22, "cf_contig_build: no clouds installed");
    if (n < 0 || (n > 0 && (!reads || !pos))) return cf_fail(ctx, -22, "cf_contig_build: bad backbone arrays");
    // every argument is checked before the previous contig is dropped
    const int64_t R = ctx->n_reads;
    int64_t max_pos = 0;
    bool covered = false;
    {
        std::vector<uint8_t> seen((size_t)R, 0);
        for (int64_t b = 0; b < n; ++b) {
            const int64_t r = reads[b];
            if (r < 0 || r >= R) return cf_fail(ctx, -22, "cf_contig_build: backbone read " + std::to_string(r) + " is out of range");
            if (seen[(size_t)r]) return cf_fail(ctx, -22, "cf_contig_build: backbone read " + std::to_string(r) + " is given twice");
            seen[(size_t)r] = 1;
            if (pos[b] < 0) return cf_fail(ctx, -22, "cf_contig_build: negative position of read " + std::to_string(r));
            const int64_t nu = ctx->h_unit_ptr[(size_t)r + 1] - ctx->h_unit_ptr[(size_t)r];
            if (pos[b] >= ((int64_t)1 << 31) || pos[b] + nu >= ((int64_t)1 << 31))
                return cf_fail(ctx, -22, "cf_contig_build: position + units of read " + std::to_string(r) + " reaches 2^31");
            if (nu > 0) { covered = true; max_pos = std::max(max_pos, pos[b] + nu - 1); }
        }
    }
    CF_HIP(hipSetDevice(ctx->device));
    cf_free_contig(ctx);
    CF_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    const int rc = contig_build(ctx, reads, pos, n, std::max<int64_t>(1, min_cloud_kmer_freq), max_pos, covered);
    if (rc) { cf_free_contig(ctx); return rc; }      // no half-built contig stays behind
    CF_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    CF_HIP(hipEventSynchronize(ctx->ev1));
    CF_HIP(hipEventElapsedTime(&ctx->contig_build_ms, ctx->ev0, ctx->ev1));
    ctx->map_ms = ctx->score_ms = 0.f;
    return 0;
}

int cf_contig_info(cf_ctx* ctx, int64_t* n_positions, int64_t* max_pos, int64_t* n_freq_kmers, int64_t* n_pairs, float* build_ms,
                   float* map_ms) {
    if (!ctx) return -22;
    if (!ctx->have_contig) return cf_fail(ctx, -22, "cf_contig_info: no contig built");
    if (n_positions) *n_positions = ctx->contig_P;
    if (max_pos) *max_pos = ctx->contig_max_pos;
    if (n_freq_kmers) *n_freq_kmers = ctx->contig_n_freq;
    if (n_pairs) *n_pairs = ctx->contig_pairs;
    if (build_ms) *build_ms = ctx->contig_build_ms;
    if (map_ms) *map_ms = ctx->map_ms;
    return 0;
}

int cf_contig_coverage(cf_ctx* ctx, int32_t* cov, int64_t cap) {
    if (!ctx) return -22;
    if (!ctx->have_contig) return cf_fail(ctx, -22, "cf_contig_coverage: no contig built");
    if (cap < ctx->contig_cov_n || (ctx->contig_cov_n && !cov)) return cf_fail(ctx, -22, "cf_contig_coverage: buffer too small");
    CF_HIP(hipSetDevice(ctx->device));
    CF_TRY(cf_copy_d2h(ctx, cov, ctx->d_contig_cov, (size_t)ctx->contig_cov_n * 4));
    return 0;
}

int cf_map_reads(cf_ctx* ctx, const int64_t* reads, int64_t n, int32_t t0, int32_t t1, int64_t* out_pos, int32_t* out_s0, int32_t* out_s1) {
    if (!ctx) return -22;
    if (!ctx->have_clouds) return cf_fail(ctx, -22, "cf_map_reads: no clouds installed");
    if (!ctx->have_contig) return cf_fail(ctx, -22, "cf_map_reads: no contig built (cf_contig_build)");
    const int64_t R = ctx->n_reads;
    if (!reads) n = R;
    if (n < 0) return cf_fail(ctx, -22, "cf_map_reads: negative number of reads");
    if (n > 0 && (!out_pos || !out_s0 || !out_s1)) return cf_fail(ctx, -22, "cf_map_reads: null output");
    for (int64_t i = 0; reads && i < n; ++i)
        if (reads[i] < 0 || reads[i] >= R) return cf_fail(ctx, -22, "cf_map_reads: read " + std::to_string(reads[i]) + " is out of range");
    if (n == 0) { ctx->map_ms = 0.f; return 0; }
    CF_HIP(hipSetDevice(ctx->device));
    CF_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    const int W = ctx->map_window > 0 ? ctx->map_window : CF_MAP_WINDOW_DEFAULT;
    int64_t *d_q = nullptr, *d_pos = nullptr;
    int32_t *d_s0 = nullptr, *d_s1 = nullptr;
    cf_scratch tmp(ctx);
    if (reads) {
        CF_TRY(tmp.get(&d_q, (size_t)n, "query reads"));
        CF_TRY(cf_copy_h2d(ctx, d_q, reads, (size_t)n * 8));
    }
    CF_TRY(tmp.get(&d_pos, (size_t)n, "mapped positions"));
    CF_TRY(tmp.get(&d_s0, (size_t)n, "mapped s0"));
    CF_TRY(tmp.get(&d_s1, (size_t)n, "mapped s1"));
    const int grid = (int)std::min<int64_t>(n, (int64_t)std::max(1, ctx->n_cu) * 64);
    hipLaunchKernelGGL(cf_map_kernel, dim3((unsigned)grid), dim3(CF_MAP_THREADS), (size_t)W * 12, ctx->stream, (const int64_t*)d_q, n,
                       (const int64_t*)ctx->d_unit_ptr, (const int64_t*)ctx->d_cloud_ptr, (const int32_t*)ctx->d_entries,
                       (const int64_t*)ctx->d_contig_ptr, (const int32_t*)ctx->d_contig_pos, ctx->contig_P, W, t0, t1, d_pos, d_s0, d_s1);
    CF_KERNEL_CHECK("cf_map_kernel");
    CF_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    CF_HIP(hipEventSynchronize(ctx->ev1));
    (void)hipEventElapsedTime(&ctx->map_ms, ctx->ev0, ctx->ev1);
    CF_TRY(cf_copy_d2h(ctx, out_pos, d_pos, (size_t)n * 8));
    CF_TRY(cf_copy_d2h(ctx, out_s0, d_s0, (size_t)n * 4));
    return cf_copy_d2h(ctx, out_s1, d_s1, (size_t)n * 4);
}

}  // extern "C"
