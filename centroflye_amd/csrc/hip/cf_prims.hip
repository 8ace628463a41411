// cf_prims.hip — device-wide exclusive scan and LSD radix sort (gfx950, wave64).
// Auxiliary primitives of the pipeline: CSR offsets (clouds, postings) and the ascending
// order of the rare k-mer set (reference: the k-mer file is written sorted,
// scripts/distance_based_kmer_recruitment.py:160-164).
#include "cf_radix.h"

#define SCAN_THREADS 256
#define SCAN_ITEMS 8
#define SCAN_TILE (SCAN_THREADS * SCAN_ITEMS)

// inclusive scan of one value per thread over a 256-thread block; returns exclusive prefix,
// *total = block sum.  lds: at least 8 int64.
__device__ __forceinline__ int64_t cf_block_exclusive(int64_t v, int64_t* lds, int64_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        int64_t o = __shfl_up(inc, (unsigned)d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int64_t wave_off = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        int64_t s = lds[w];
        if (w < wave) wave_off += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return wave_off + inc - v;
}

template <class TIn>
__global__ void __launch_bounds__(SCAN_THREADS)
cf_scan_local(const TIn* __restrict__ in, int64_t* __restrict__ out, int64_t* __restrict__ block_sums, int64_t n) {
    int64_t* lds = (int64_t*)cf_lds;
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int64_t v[SCAN_ITEMS];
    int64_t sum = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        v[i] = (base + i < n) ? (int64_t)in[base + i] : 0;
        sum += v[i];
    }
    int64_t total;
    int64_t pre = cf_block_exclusive(sum, lds, &total);
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i) {
        if (base + i < n) out[base + i] = pre;
        pre += v[i];
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SCAN_THREADS)
cf_scan_add(int64_t* __restrict__ out, const int64_t* __restrict__ block_off, int64_t n) {
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    const int64_t off = block_off[blockIdx.x];
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
        if (base + i < n) out[base + i] += off;
}

template <class TIn>
static int scan_impl(cf_ctx* ctx, const TIn* d_in, int64_t* d_out, int64_t n, int64_t* total) {
    if (n <= 0) { if (total) *total = 0; return 0; }
    const int64_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    cf_scratch tmp(ctx);
    int64_t* d_sums = nullptr;
    CF_TRY(tmp.get(&d_sums, (size_t)nb + 1, "scan block sums"));
    hipLaunchKernelGGL((cf_scan_local<TIn>), dim3((unsigned)nb), dim3(SCAN_THREADS), 64, ctx->stream, d_in, d_out, d_sums, n);
    CF_KERNEL_CHECK("cf_scan_local");
    int64_t tot = 0;
    if (total) *total = 0;
    if (nb > 1) {
        CF_TRY(scan_impl<int64_t>(ctx, d_sums, d_sums, nb, &tot));
        hipLaunchKernelGGL(cf_scan_add, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, ctx->stream, d_out, d_sums, n);
        CF_KERNEL_CHECK("cf_scan_add");
    } else {
        CF_HIP(hipMemcpyAsync(&tot, d_sums, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    CF_HIP(hipStreamSynchronize(ctx->stream));
    if (total) *total = tot;
    return 0;
}

int cf_scan_exclusive_i64(cf_ctx* ctx, const int64_t* d_in, int64_t* d_out, int64_t n, int64_t* total) {
    return scan_impl<int64_t>(ctx, d_in, d_out, n, total);
}
int cf_scan_exclusive_u32_to_i64(cf_ctx* ctx, const uint32_t* d_in, int64_t* d_out, int64_t n, int64_t* total) {
    return scan_impl<uint32_t>(ctx, d_in, d_out, n, total);
}

// ------------------------------------------------------------------ offsets of tile-major digit histograms
// offs[tile][d] = keys with a smaller digit + keys of digit d in earlier tiles = the exclusive scan of hist in (digit, tile)
// order, computed on the tile-major arrays by columns: (1) column sums of chunks of `chunk` tiles, (2) one workgroup turns
// them into the chunks' bases (column totals, scan over the digits, running sums down the chunks), (3) every chunk walks its
// tiles again.  All accesses are runs of D counters (digit-major counters made every counter its own 64-byte sector on the
// way out and on the way back in: 20 GB of A1's 91 GB of HBM traffic).  A walk is latency-bound — its loads
// are issued CF_COL_UNROLL at a time, and the stores of a walk wait for their acknowledgement before the next loads — so
// the chunk is about sqrt(tiles): the walks of (1) and (3) and the one of (2) are equally long.
#define CF_COL_THREADS 512                  /* >= D: a thread per digit */
#define CF_COL_UNROLL 16
__global__ void __launch_bounds__(CF_COL_THREADS)
cf_col_sum_kernel(const uint32_t* __restrict__ hist, int n_tiles, int D, int chunk, uint32_t* __restrict__ part) {
    const int d = threadIdx.x;
    if (d >= D) return;
    const int t0 = blockIdx.x * chunk, t1 = min(n_tiles, t0 + chunk);
    uint32_t acc = 0;
    for (int t = t0; t < t1; t += CF_COL_UNROLL) {
        uint32_t v[CF_COL_UNROLL];
#pragma unroll
        for (int u = 0; u < CF_COL_UNROLL; ++u) v[u] = t + u < t1 ? hist[(int64_t)(t + u) * D + d] : 0u;
#pragma unroll
        for (int u = 0; u < CF_COL_UNROLL; ++u) acc += v[u];
    }
    part[(int64_t)blockIdx.x * D + d] = acc;
}
__global__ void __launch_bounds__(CF_COL_THREADS)
cf_col_base_kernel(const uint32_t* __restrict__ part, int n_chunks, int D, int64_t* __restrict__ base, int64_t* __restrict__ total_out) {
    long long* sh = (long long*)cf_lds;                       // CF_COL_THREADS / 64 wave totals
    const int d = threadIdx.x, lane = d & 63, wave = d >> 6;
    long long tot = 0;
    if (d < D)
        for (int c = 0; c < n_chunks; c += CF_COL_UNROLL) {
            uint32_t v[CF_COL_UNROLL];
#pragma unroll
            for (int u = 0; u < CF_COL_UNROLL; ++u) v[u] = c + u < n_chunks ? part[(int64_t)(c + u) * D + d] : 0u;
#pragma unroll
            for (int u = 0; u < CF_COL_UNROLL; ++u) tot += v[u];
        }
    long long inc = tot;                                       // inclusive scan over the digits
    for (int s = 1; s < 64; s <<= 1) { const long long o = __shfl_up(inc, (unsigned)s); if (lane >= s) inc += o; }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    long long run = inc - tot;
    for (int w = 0; w < wave; ++w) run += sh[w];
    if (total_out && d == D - 1) *total_out = run + tot;
    if (d < D)
        for (int c = 0; c < n_chunks; c += CF_COL_UNROLL) {
            uint32_t v[CF_COL_UNROLL];
#pragma unroll
            for (int u = 0; u < CF_COL_UNROLL; ++u) v[u] = c + u < n_chunks ? part[(int64_t)(c + u) * D + d] : 0u;
#pragma unroll
            for (int u = 0; u < CF_COL_UNROLL; ++u) if (c + u < n_chunks) { base[(int64_t)(c + u) * D + d] = run; run += v[u]; }
        }
}
__global__ void __launch_bounds__(CF_COL_THREADS)
cf_col_offs_kernel(const uint32_t* __restrict__ hist, int n_tiles, int D, int chunk, const int64_t* __restrict__ base, int64_t* __restrict__ offs) {
    const int d = threadIdx.x;
    if (d >= D) return;
    const int t0 = blockIdx.x * chunk, t1 = min(n_tiles, t0 + chunk);
    long long run = base[(int64_t)blockIdx.x * D + d];
    for (int t = t0; t < t1; t += CF_COL_UNROLL) {
        uint32_t v[CF_COL_UNROLL];
#pragma unroll
        for (int u = 0; u < CF_COL_UNROLL; ++u) v[u] = t + u < t1 ? hist[(int64_t)(t + u) * D + d] : 0u;
#pragma unroll
        for (int u = 0; u < CF_COL_UNROLL; ++u) if (t + u < t1) { offs[(int64_t)(t + u) * D + d] = run; run += v[u]; }
    }
}

static int col_chunk(int n_tiles) {       // ~sqrt(n_tiles), a multiple of CF_COL_UNROLL
    int c = CF_COL_UNROLL;
    while ((int64_t)c * c < n_tiles) c += CF_COL_UNROLL;
    return c;
}
int cf_tile_digit_chunks(int n_tiles) { const int c = col_chunk(n_tiles); return (n_tiles + c - 1) / c; }

int cf_tile_digit_offsets(cf_ctx* ctx, const uint32_t* d_hist, int n_tiles, int D, int64_t* d_offs, int64_t* d_total, uint32_t* d_part, int64_t* d_base) {
    if (D < 1 || D > CF_COL_THREADS) return cf_fail(ctx, -22, "cf_tile_digit_offsets: bad digit count");
    const int chunk = col_chunk(n_tiles), n_chunks = cf_tile_digit_chunks(n_tiles);
    if (n_chunks == 0) return 0;
    hipLaunchKernelGGL(cf_col_sum_kernel, dim3((unsigned)n_chunks), dim3(CF_COL_THREADS), 0, ctx->stream, d_hist, n_tiles, D, chunk, d_part);
    hipLaunchKernelGGL(cf_col_base_kernel, dim3(1), dim3(CF_COL_THREADS), 64, ctx->stream, (const uint32_t*)d_part, n_chunks, D, d_base, d_total);
    hipLaunchKernelGGL(cf_col_offs_kernel, dim3((unsigned)n_chunks), dim3(CF_COL_THREADS), 0, ctx->stream, d_hist, n_tiles, D, chunk, (const int64_t*)d_base, d_offs);
    CF_KERNEL_CHECK("cf_col*");
    return 0;
}

// ------------------------------------------------------------------ radix sort of 64-bit keys
// LSD passes of 8-bit digits over tiles of RX_TILE keys.  Per pass: cf_radix_hist writes every tile's digit counts
// (tile-major), cf_tile_digit_offsets turns them into the tile's global offsets, cf_radix_scatter ranks the tile stably in
// LDS (cf_radix.h) and writes every digit's run of the tile as one contiguous piece.  No host synchronisation between passes.
#define RX_ITEMS 16
#define RX_TILE (CF_RX_THREADS * RX_ITEMS)
#define RX_D 256
struct __attribute__((aligned(16))) cf_u64x2 { unsigned long long a, b; };

__global__ void __launch_bounds__(CF_RX_THREADS)
cf_radix_hist(const unsigned long long* __restrict__ in, uint32_t* __restrict__ hist, int64_t n, int shift, int ntiles) {
    uint32_t* h = (uint32_t*)cf_lds;
    const int t = threadIdx.x;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        h[t] = 0;
        __syncthreads();
        const int64_t base = (int64_t)tile * RX_TILE;
        if (base + RX_TILE <= n) {          // whole tile: 16-byte loads (a tile begins on a multiple of RX_TILE keys)
            const cf_u64x2* v = (const cf_u64x2*)(in + base);
#pragma unroll
            for (int j = 0; j < RX_ITEMS / 2; ++j) {
                const cf_u64x2 x = v[j * CF_RX_THREADS + t];
                atomicAdd(&h[(uint32_t)(x.a >> shift) & (RX_D - 1)], 1u);
                atomicAdd(&h[(uint32_t)(x.b >> shift) & (RX_D - 1)], 1u);
            }
        } else {
            for (int j = 0; j < RX_ITEMS; ++j) {
                const int64_t i = base + (int64_t)j * CF_RX_THREADS + t;
                if (i < n) atomicAdd(&h[(uint32_t)(in[i] >> shift) & (RX_D - 1)], 1u);
            }
        }
        __syncthreads();
        hist[(int64_t)tile * RX_D + t] = h[t];
        __syncthreads();
    }
}

// LDS: gbase int64[D] | wcount u32[4][D] | dstart u32[D] | scan_tmp u32[8] | staged keys u64[RX_TILE]
#define RX_SCATTER_LDS (RX_D * 8 + (CF_RX_THREADS / 64) * RX_D * 4 + RX_D * 4 + 32 + 16 + RX_TILE * 8)
__global__ void __launch_bounds__(CF_RX_THREADS)
cf_radix_scatter(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                 const int64_t* __restrict__ offs, int64_t n, int shift, int ntiles) {
    int64_t* gbase = (int64_t*)cf_lds;
    uint32_t* wcount = (uint32_t*)(gbase + RX_D);
    uint32_t* dstart = wcount + (CF_RX_THREADS / 64) * RX_D;
    uint32_t* scan_tmp = dstart + RX_D;
    unsigned long long* srec = (unsigned long long*)(((uintptr_t)(scan_tmp + 8) + 15) & ~(uintptr_t)15);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    uint32_t* wrow = wcount + wave * RX_D;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        gbase[t] = offs[(int64_t)tile * RX_D + t];
        for (int d = lane; d < RX_D; d += 64) wrow[d] = 0;      // (a wave clears its own row: its LDS ops are in order)
        // wave w takes the keys [w * 64 * RX_ITEMS, ...) of the tile in rounds of 64: array order = (wave, round, lane)
        const int64_t base = (int64_t)tile * RX_TILE + (int64_t)wave * 64 * RX_ITEMS + lane;
        unsigned long long key[RX_ITEMS];
        uint32_t rank[RX_ITEMS];
#pragma unroll
        for (int j = 0; j < RX_ITEMS; ++j) { const int64_t i = base + (int64_t)j * 64; key[j] = i < n ? in[i] : 0ull; }
#pragma unroll
        for (int j = 0; j < RX_ITEMS; ++j)
            rank[j] = cf_rx_rank_round<8>((uint32_t)(key[j] >> shift) & (RX_D - 1), base + (int64_t)j * 64 < n, wrow);
        cf_rx_tile_bases<8>(dstart, wcount, scan_tmp);
#pragma unroll
        for (int j = 0; j < RX_ITEMS; ++j)
            if (base + (int64_t)j * 64 < n) { const uint32_t d = (uint32_t)(key[j] >> shift) & (RX_D - 1); srec[dstart[d] + wrow[d] + rank[j]] = key[j]; }
        const uint32_t n_tile = (uint32_t)min((int64_t)RX_TILE, n - (int64_t)tile * RX_TILE);
        __syncthreads();
        for (uint32_t i = t; i < n_tile; i += CF_RX_THREADS) {      // consecutive threads write consecutive addresses inside a digit's run
            const unsigned long long k = srec[i];
            const uint32_t d = (uint32_t)(k >> shift) & (RX_D - 1);
            out[gbase[d] + (int64_t)(i - dstart[d])] = k;
        }
        __syncthreads();
    }
}

int cf_radix_sort_u64(cf_ctx* ctx, unsigned long long* d_keys, unsigned long long* d_tmp, int64_t n, int bits) {
    return cf_radix_sort_u64_any(ctx, d_keys, d_tmp, n, bits, nullptr);
}

// the same; with `result` the sorted keys stay in whichever of the two buffers the last pass wrote (no copy back) and
// *result tells which
int cf_radix_sort_u64_any(cf_ctx* ctx, unsigned long long* d_keys, unsigned long long* d_tmp, int64_t n, int bits, unsigned long long** result) {
    if (result) *result = d_keys;
    if (n <= 1) return 0;
    if ((n + RX_TILE - 1) / RX_TILE >= ((int64_t)1 << 31)) return cf_fail(ctx, -22, "radix sort: too many keys");
    const int ntiles = (int)((n + RX_TILE - 1) / RX_TILE);
    const int64_t nh = (int64_t)ntiles * RX_D, nc = (int64_t)cf_tile_digit_chunks(ntiles) * RX_D;
    const int grid = std::min(ntiles, std::max(1, ctx->n_cu) * 8);
    cf_scratch tmp(ctx);
    uint32_t* d_hist = nullptr;
    int64_t* d_offs = nullptr;
    uint32_t* d_part = nullptr;
    int64_t* d_base = nullptr;
    CF_TRY(tmp.get(&d_hist, (size_t)nh, "radix histogram"));
    CF_TRY(tmp.get(&d_offs, (size_t)nh, "radix offsets"));
    CF_TRY(tmp.get(&d_part, (size_t)nc, "radix column sums"));
    CF_TRY(tmp.get(&d_base, (size_t)nc, "radix column bases"));
    unsigned long long* src = d_keys;
    unsigned long long* dst = d_tmp;
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(cf_radix_hist, dim3((unsigned)grid), dim3(CF_RX_THREADS), RX_D * 4, ctx->stream, (const unsigned long long*)src, d_hist, n, shift, ntiles);
        CF_TRY(cf_tile_digit_offsets(ctx, d_hist, ntiles, RX_D, d_offs, nullptr, d_part, d_base));
        hipLaunchKernelGGL(cf_radix_scatter, dim3((unsigned)grid), dim3(CF_RX_THREADS), RX_SCATTER_LDS, ctx->stream, (const unsigned long long*)src, dst,
                           (const int64_t*)d_offs, n, shift, ntiles);
        CF_KERNEL_CHECK("cf_radix_scatter");
        std::swap(src, dst);
    }
    if (result) *result = src;
    else if (src != d_keys) CF_HIP(hipMemcpyAsync(d_keys, src, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
    CF_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ------------------------------------------------------------------ radix sort of 16-byte records by 32-bit fields
// LSD passes of 8 bits over the fields the caller lists (least significant first): per pass a digit-major histogram of
// tiles of RS_TILE records, its exclusive scan, and a stable ballot-ranked scatter, with a record = four 32-bit words and
// the digit taken from word `word`.
#define RS_THREADS 256
#define RS_ITEMS 8
#define RS_TILE (RS_THREADS * RS_ITEMS)
struct __attribute__((aligned(16))) cf_rec16 { uint32_t w[4]; };

__global__ void __launch_bounds__(RS_THREADS)
cf_rec16_hist(const cf_rec16* __restrict__ in, uint32_t* __restrict__ hist, int64_t n, int word, int shift, int ntiles) {
    uint32_t* h = (uint32_t*)cf_lds;
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RS_TILE;
#pragma unroll
    for (int i = 0; i < RS_ITEMS; ++i) {
        const int64_t idx = base + (int64_t)i * RS_THREADS + threadIdx.x;
        if (idx < n) atomicAdd(&h[(((const uint32_t*)(in + idx))[word] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

__global__ void __launch_bounds__(RS_THREADS)
cf_rec16_scatter(const cf_rec16* __restrict__ in, cf_rec16* __restrict__ out, const int64_t* __restrict__ offs, int64_t n, int word, int shift, int ntiles) {
    int64_t* run = (int64_t*)cf_lds;                       // 256 running offsets, one per digit
    uint32_t* wcount = (uint32_t*)(cf_lds + 256 * 8);      // [4][256] per-wave digit counts
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    run[t] = offs[(int64_t)t * ntiles + blockIdx.x];
    for (int w = 0; w < 4; ++w) wcount[w * 256 + t] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RS_TILE;
    for (int round = 0; round < RS_ITEMS; ++round) {
        const int64_t idx = base + (int64_t)round * RS_THREADS + t;
        const bool valid = idx < n;
        cf_rec16 rec{{0u, 0u, 0u, 0u}};
        if (valid) rec = in[idx];
        const uint32_t digit = (rec.w[word] >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int bit = (digit >> b) & 1;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wcount[wave * 256 + digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        int64_t pos = 0;
        if (valid) {
            pos = run[digit] + rank;
            for (int w = 0; w < wave; ++w) pos += wcount[w * 256 + digit];
        }
        __syncthreads();
        {
            uint32_t sum = 0;
            for (int w = 0; w < 4; ++w) { sum += wcount[w * 256 + t]; wcount[w * 256 + t] = 0; }
            run[t] += sum;
        }
        __syncthreads();
        if (valid) out[pos] = rec;
    }
}

// the tiles of the scan and of the record sort, for the shapes a caller reports (cf_monokmers_info)
int cf_scan_tile() { return SCAN_TILE; }
int cf_radix_rec16_tile() { return RS_TILE; }

// d_recs: n records of 16 bytes; d_tmp: scratch of the same size; fields: n_fields (word index, significant bits), least
// significant field first.  The sorted records end in d_recs.  (What `bits` means when it is no multiple of 8: cf_common.h.)
int cf_radix_sort_rec16(cf_ctx* ctx, void* d_recs, void* d_tmp, int64_t n, const int* words, const int* bits, int n_fields) {
    if (n <= 1) return 0;
    const int ntiles = (int)((n + RS_TILE - 1) / RS_TILE);
    const int64_t nh = (int64_t)ntiles * 256;
    cf_scratch tmp(ctx);
    uint32_t* d_hist = nullptr;
    int64_t* d_offs = nullptr;
    CF_TRY(tmp.get(&d_hist, (size_t)nh, "radix histogram"));
    CF_TRY(tmp.get(&d_offs, (size_t)nh, "radix offsets"));
    cf_rec16* src = (cf_rec16*)d_recs;
    cf_rec16* dst = (cf_rec16*)d_tmp;
    for (int f = 0; f < n_fields; ++f) {
        for (int shift = 0; shift < bits[f]; shift += 8) {
            hipLaunchKernelGGL(cf_rec16_hist, dim3((unsigned)ntiles), dim3(RS_THREADS), 256 * 4, ctx->stream, (const cf_rec16*)src, d_hist, n, words[f], shift, ntiles);
            CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_hist, d_offs, nh, nullptr));
            hipLaunchKernelGGL(cf_rec16_scatter, dim3((unsigned)ntiles), dim3(RS_THREADS), 256 * 8 + 4 * 256 * 4, ctx->stream, (const cf_rec16*)src, dst, (const int64_t*)d_offs, n, words[f], shift, ntiles);
            CF_KERNEL_CHECK("cf_rec16_scatter");
            std::swap(src, dst);
        }
    }
    if (src != (cf_rec16*)d_recs) CF_HIP(hipMemcpyAsync(d_recs, src, (size_t)n * 16, hipMemcpyDeviceToDevice, ctx->stream));
    CF_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
