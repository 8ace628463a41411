// cf_monomap.hip — monoreads mapped to the edges of the de Bruijn graph: per read its hits on uniquely indexed edge k-mers, its path
// of edges and whether the path's joins hold (gfx950, wave64).
//
// What the reference's second pipeline does with a dict of every window of every edge and a slice at every read position
// (scripts/debruijn_graph.py index_edges, map_reads).  The rule is written out at cf_monomap_run in include/cfhip.h and restated
// in tests/monomapcheck.py.  Equality of k-mers is equality of bytes: nothing here is a hash.
//
// The edges are concatenated first, then the reads, and the doubling rounds of cf_monokmers.hip (cf_mk_rank_windows) run once over
// both.  They leave the valid windows' records class by class, ascending position inside a class.  The sort is stable and the
// edges lie in front, so a class's first record is its edge window if it has one: the class is INDEXED iff its first record is an
// edge position and its second record, if any, is a read position.  No atomics and no counting.
//
//   cf_mm_heads     class heads: cls[c] = the edge position of an indexed class, else none; per record: is it an edge window
//   (scan) x 2      the valid edge windows and the indexed k-mers, for cf_monomap_info
//   cf_mm_scatter   every read record of an indexed class: hit[p] = the edge position, flag[p] = 1
//   (scan)          hs[p] = the hits in front of position p; at a read's offset: the index of its first hit
//   cf_mm_compact   hit x = hs[p]: (e, j) by a binary search of the edge position in the offsets, i and the read likewise
//   cf_mm_runs      run head: the first hit of its read, or another edge than the hit before; broken join: a run head that is not
//                   the first of its read with v[edge before] != u[edge]
//   (scan) x 2      ps[x] = the run heads in front of hit x; bs[x] = the broken joins in front of it
//   cf_mm_paths     path[ps[x]] = the edge of run head x
//   cf_mm_reads     per read, from the scans at its two offsets: n_hits, the first and the last hit, n_path, valid, the CSR offsets
// Every kernel is a grid-stride streaming pass of 256 threads with no LDS, no atomics and no wave operation; every index is below
// N < 2^31 and is checked against its array's length where it is a loaded value.
#include "cf_common.h"

#include <new>

#define CF_MM_BLOCK 256
#define CF_MM_NONE 0xffffffffu

#define CF_MM_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * CF_MM_BLOCK + threadIdx.x; i < (n); i += (int64_t)gridDim.x * CF_MM_BLOCK)

__global__ void __launch_bounds__(CF_MM_BLOCK)
cf_mm_heads(const cf_mk_rec* __restrict__ rec, const uint32_t* __restrict__ head, const int64_t* __restrict__ e, uint32_t* __restrict__ cls,
            uint32_t* __restrict__ is_edge, int64_t n_valid, int64_t n_classes, int64_t n_edge_letters) {
    CF_MM_LOOP(i, n_valid) {
        const int64_t p = rec[i].w[2];
        is_edge[i] = p < n_edge_letters ? 1u : 0u;
        const int64_t c = e[i];
        if (head[i] && c >= 0 && c < n_classes) {
            bool indexed = p < n_edge_letters;
            if (indexed && i + 1 < n_valid && !head[i + 1]) indexed = (int64_t)rec[i + 1].w[2] >= n_edge_letters;
            cls[c] = indexed ? (uint32_t)p : CF_MM_NONE;
        }
    }
}

__global__ void __launch_bounds__(CF_MM_BLOCK)
cf_mm_indexed(const uint32_t* __restrict__ cls, uint32_t* __restrict__ flag, int64_t n_classes) {
    CF_MM_LOOP(c, n_classes) flag[c] = cls[c] != CF_MM_NONE ? 1u : 0u;
}

__global__ void __launch_bounds__(CF_MM_BLOCK)
cf_mm_scatter(const cf_mk_rec* __restrict__ rec, const uint32_t* __restrict__ head, const int64_t* __restrict__ e, const uint32_t* __restrict__ cls,
              uint32_t* __restrict__ hit, uint32_t* __restrict__ flag, int64_t n_valid, int64_t n_classes, int64_t n_edge_letters, int64_t n) {
    CF_MM_LOOP(i, n_valid) {
        const int64_t p = rec[i].w[2], c = e[i] + head[i] - 1;
        if (p < n_edge_letters || p >= n || c < 0 || c >= n_classes) continue;
        const uint32_t ep = cls[c];
        if (ep == CF_MM_NONE) continue;
        hit[p] = ep;
        flag[p] = 1u;
    }
}

__global__ void __launch_bounds__(CF_MM_BLOCK)
cf_mm_compact(const uint32_t* __restrict__ flag, const int64_t* __restrict__ hs, const uint32_t* __restrict__ hit, const int64_t* __restrict__ off,
              int64_t n_edges, int64_t n_strings, cf_monomap_hit* __restrict__ hits, int32_t* __restrict__ hit_read, int64_t n, int64_t n_edge_letters,
              int64_t n_hits) {
    CF_MM_LOOP(q, n - n_edge_letters) {
        const int64_t p = n_edge_letters + q;
        if (!flag[p]) continue;
        const int64_t x = hs[p], ep = hit[p];
        if (x < 0 || x >= n_hits || ep >= n_edge_letters || n_edges < 1) continue;
        const int64_t ed = cf_string_of(off, n_edges, ep), s = cf_string_of(off, n_strings, p);
        if (s < n_edges) continue;
        cf_monomap_hit h;
        h.e = (int32_t)ed; h.j = (int32_t)(ep - off[ed]); h.i = (int32_t)(p - off[s]);
        hits[x] = h;
        hit_read[x] = (int32_t)(s - n_edges);
    }
}

// the index of the first hit at or behind position o of the concatenation (o = a read's offset: of its first hit, if it has one)
__device__ __forceinline__ int64_t cf_mm_hits_before(const int64_t* __restrict__ hs, int64_t o, int64_t n, int64_t n_hits) {
    if (o < 0) return 0;
    if (o >= n) return n_hits;
    const int64_t x = hs[o];
    return x < 0 ? 0 : (x > n_hits ? n_hits : x);
}

__global__ void __launch_bounds__(CF_MM_BLOCK)
cf_mm_runs(const cf_monomap_hit* __restrict__ hits, const int32_t* __restrict__ hit_read, const int64_t* __restrict__ off, const int64_t* __restrict__ hs,
           const int32_t* __restrict__ u, const int32_t* __restrict__ v, uint32_t* __restrict__ run_head, uint32_t* __restrict__ broken, int64_t n_hits,
           int64_t n_edges, int64_t n_reads, int64_t n) {
    CF_MM_LOOP(x, n_hits) {
        const int64_t r = hit_read[x], ed = hits[x].e;
        bool first = x == 0;
        if (!first && r >= 0 && r < n_reads) first = x == cf_mm_hits_before(hs, off[n_edges + r], n, n_hits);
        bool h = first, b = false;
        if (!first) {
            const int64_t before = hits[x - 1].e;
            h = before != ed;
            if (h) b = before < 0 || before >= n_edges || ed < 0 || ed >= n_edges || v[before] != u[ed];
        }
        run_head[x] = h ? 1u : 0u;
        broken[x] = b ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(CF_MM_BLOCK)
cf_mm_paths(const cf_monomap_hit* __restrict__ hits, const uint32_t* __restrict__ run_head, const int64_t* __restrict__ ps, int32_t* __restrict__ path,
            int64_t n_hits, int64_t n_path) {
    CF_MM_LOOP(x, n_hits) {
        const int64_t d = ps[x];
        if (run_head[x] && d >= 0 && d < n_path) path[d] = hits[x].e;
    }
}

__global__ void __launch_bounds__(CF_MM_BLOCK)
cf_mm_reads(const int64_t* __restrict__ off, const int64_t* __restrict__ hs, const int64_t* __restrict__ ps, const int64_t* __restrict__ bs,
            const cf_monomap_hit* __restrict__ hits, cf_monomap_read* __restrict__ out, int64_t* __restrict__ path_ptr, int64_t* __restrict__ hit_ptr,
            int64_t n_edges, int64_t n_reads, int64_t n, int64_t n_hits, int64_t n_path, int64_t n_broken) {
    CF_MM_LOOP(r, n_reads) {
        const int64_t h0 = cf_mm_hits_before(hs, off[n_edges + r], n, n_hits);
        const int64_t h_end = cf_mm_hits_before(hs, off[n_edges + r + 1], n, n_hits), h1 = h_end < h0 ? h0 : h_end;
        // the first hit of a read is a run head, so the heads in front of it are the path elements in front of the read
        const int64_t p0 = h0 < n_hits ? ps[h0] : n_path, p1 = h1 < n_hits ? ps[h1] : n_path;
        const int64_t b0 = h0 < n_hits ? bs[h0] : n_broken, b1 = h1 < n_hits ? bs[h1] : n_broken;
        cf_monomap_read o;
        o.n_hits = (int32_t)(h1 - h0);
        o.e0 = o.j0 = o.i0 = o.e1 = o.j1 = o.i1 = -1;
        if (h1 > h0) {
            const cf_monomap_hit a = hits[h0], z = hits[h1 - 1];
            o.e0 = a.e; o.j0 = a.j; o.i0 = a.i;
            o.e1 = z.e; o.j1 = z.j; o.i1 = z.i;
        }
        o.valid = b1 == b0 ? 1 : 0;
        o.n_path = (int32_t)(p1 - p0);
        out[r] = o;
        path_ptr[r] = p0;
        hit_ptr[r] = h0;
    }
}

extern "C" {

int cf_monomap_info(cf_ctx* ctx, cf_monomap_shape* out) {
    if (!ctx || !out) return -22;
    *out = ctx->monomap_last;
    out->sort_tile = cf_radix_rec16_tile();
    out->scan_tile = cf_scan_tile();
    out->block = CF_MM_BLOCK;
    out->launch_cap = cf_mk_launch_cap(ctx);
    return 0;
}

int cf_monomap_get(cf_ctx* ctx, int64_t* path_ptr, int32_t* path, int64_t path_cap, int64_t* n_path_out, int64_t* hit_ptr, cf_monomap_hit* hits,
                   int64_t hit_cap, int64_t* n_hits_out) {
    if (!ctx) return -22;
    if (!ctx->monomap_have) return cf_fail(ctx, -22, "cf_monomap_get: no cf_monomap_run before");
    const int64_t n_path = (int64_t)ctx->monomap_path.size(), n_hits = (int64_t)ctx->monomap_hits.size();
    const bool kept = ctx->monomap_last.with_hits != 0;
    if (n_path_out) *n_path_out = n_path;
    if (n_hits_out) *n_hits_out = kept ? n_hits : -1;
    if (path && path_cap < n_path)
        return cf_fail(ctx, -22, "cf_monomap_get: room for " + std::to_string(path_cap) + " path elements, " + std::to_string(n_path) + " needed");
    if (path_ptr) std::memcpy(path_ptr, ctx->monomap_path_ptr.data(), ctx->monomap_path_ptr.size() * 8);
    if (path && n_path) std::memcpy(path, ctx->monomap_path.data(), (size_t)n_path * 4);
    if (hit_ptr || hits) {
        if (!kept) return cf_fail(ctx, -22, "cf_monomap_get: the last run kept no hits");
        if (hits && hit_cap < n_hits)
            return cf_fail(ctx, -22, "cf_monomap_get: room for " + std::to_string(hit_cap) + " hits, " + std::to_string(n_hits) + " needed");
        if (hit_ptr) std::memcpy(hit_ptr, ctx->monomap_hit_ptr.data(), ctx->monomap_hit_ptr.size() * 8);
        if (hits && n_hits) std::memcpy(hits, ctx->monomap_hits.data(), (size_t)n_hits * sizeof(cf_monomap_hit));
    }
    return 0;
}

// offsets of one of the two string sets: null only with no string; >= 0 and ascending
static int cf_mm_check_offsets(cf_ctx* ctx, const char* what, const int64_t* off, int64_t n, int64_t* letters) {
    *letters = 0;
    if (n == 0) return 0;
    if (!off) return cf_fail(ctx, -22, std::string("cf_monomap_run: null ") + what + " offsets");
    if (off[0] < 0) return cf_fail(ctx, -22, std::string("cf_monomap_run: negative ") + what + " offset");
    for (int64_t s = 0; s < n; ++s)
        if (off[s + 1] < off[s]) return cf_fail(ctx, -22, std::string("cf_monomap_run: the ") + what + " offsets do not ascend at string " + std::to_string(s));
    *letters = off[n] - off[0];
    return 0;
}

int cf_monomap_run(cf_ctx* ctx, const uint8_t* edge_bytes, const int64_t* edge_off, const int32_t* u, const int32_t* v, int64_t n_edges,
                   const uint8_t* read_bytes, const int64_t* read_off, int64_t n_reads, int64_t k, int32_t gap, int32_t with_hits,
                   cf_monomap_read* reads_out, float* ms_out) {
    if (!ctx) return -22;
    if (ms_out) *ms_out = 0.f;
    if (k < 1) return cf_fail(ctx, -22, "cf_monomap_run: k is below 1");
    if (gap < 0 || gap > 255) return cf_fail(ctx, -22, "cf_monomap_run: the gap byte is outside 0 .. 255");
    if (n_edges < 0 || n_edges >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_monomap_run: the number of edges is outside 0 .. 2^31 - 1");
    if (n_reads < 0 || n_reads >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_monomap_run: the number of reads is outside 0 .. 2^31 - 1");
    int64_t NE = 0, NR = 0;
    CF_TRY(cf_mm_check_offsets(ctx, "edge", edge_off, n_edges, &NE));
    CF_TRY(cf_mm_check_offsets(ctx, "read", read_off, n_reads, &NR));
    if (n_edges > 0 && (!u || !v)) return cf_fail(ctx, -22, "cf_monomap_run: null edge nodes");
    if (NE >= (int64_t)1 << 31 || NR >= (int64_t)1 << 31 || NE + NR >= (int64_t)1 << 31)
        return cf_fail(ctx, -22, "cf_monomap_run: " + std::to_string(NE) + " edge letters and " + std::to_string(NR) + " read letters: N is 2^31 or more");
    if (NE > 0 && !edge_bytes) return cf_fail(ctx, -22, "cf_monomap_run: null edge bytes");
    if (NR > 0 && !read_bytes) return cf_fail(ctx, -22, "cf_monomap_run: null read bytes");
    const int64_t N = NE + NR, E = n_edges, R = n_reads, S = E + R;

    // the results of this call, handed to the context only when everything worked
    cf_monomap_read none{};
    none.e0 = none.j0 = none.i0 = none.e1 = none.j1 = none.i1 = -1;
    none.valid = 1;
    std::vector<cf_monomap_read> res_reads;
    std::vector<int64_t> res_pptr, res_hptr;
    try {      // (52 bytes per read of host memory: nothing may be thrown across the C ABI)
        res_reads.assign((size_t)R, none);
        res_pptr.assign((size_t)R + 1, 0);
        res_hptr.assign((size_t)R + 1, 0);
    } catch (const std::bad_alloc&) {
        return cf_fail(ctx, -12, "cf_monomap_run: no host memory for the results of " + std::to_string(R) + " reads");
    }
    std::vector<int32_t> res_path;
    std::vector<cf_monomap_hit> res_hits;
    cf_monomap_shape shape{};
    shape.n_edges = E;
    shape.n_reads = R;
    shape.k = k;
    shape.with_hits = with_hits ? 1 : 0;
    shape.n_edge_letters = NE;
    shape.n_read_letters = NR;
    auto finish = [&]() {
        if (ms_out) *ms_out = shape.phase_ms[3];
        if (reads_out && R > 0) std::memcpy(reads_out, res_reads.data(), (size_t)R * sizeof(cf_monomap_read));
        ctx->monomap_reads.swap(res_reads);
        ctx->monomap_path_ptr.swap(res_pptr);
        ctx->monomap_hit_ptr.swap(res_hptr);
        ctx->monomap_path.swap(res_path);
        ctx->monomap_hits.swap(res_hits);
        ctx->monomap_last = shape;
        ctx->monomap_have = true;
        return 0;
    };
    if (N == 0 || k > N) return finish();      // no string holds a window

    CF_HIP(hipSetDevice(ctx->device));
    hipEvent_t e0 = ctx->ev0, e1 = ctx->ev1, e2 = ctx->ev2, e3 = ctx->ev3;
    float t = 0.f, copy_ms = 0.f;
    const int cap = cf_mk_launch_cap(ctx);
    const size_t n = (size_t)N, n4 = (n + 3) & ~(size_t)3;
    auto grid = [&](int64_t items) { return dim3((unsigned)cf_grid_for(items, CF_MM_BLOCK, cap)); };
    // the offsets of the concatenation: the edges first, then the reads
    std::vector<int64_t> h_off;
    try {
        h_off.assign((size_t)S + 1, 0);
    } catch (const std::bad_alloc&) {
        return cf_fail(ctx, -12, "cf_monomap_run: no host memory for the offsets of " + std::to_string(S) + " strings");
    }
    for (int64_t s = 0; s < E; ++s) h_off[(size_t)s + 1] = edge_off[s + 1] - edge_off[0];
    for (int64_t s = 0; s < R; ++s) h_off[(size_t)(E + s) + 1] = NE + read_off[s + 1] - read_off[0];
    cf_scratch tmp(ctx);
    uint8_t* d_bytes = nullptr;
    int64_t* d_off = nullptr;
    int32_t* d_uv = nullptr;
    CF_HIP(hipEventRecord(e0, ctx->stream));
    CF_TRY(tmp.get(&d_bytes, n4 + 16, "monomap letters"));
    CF_TRY(tmp.get(&d_off, (size_t)S + 1, "monomap offsets"));
    CF_TRY(tmp.get(&d_uv, (size_t)std::max<int64_t>(2 * E, 1), "monomap edge nodes"));
    CF_HIP(hipMemsetAsync(d_bytes + n, 0, n4 + 16 - n, ctx->stream));
    if (NE > 0) CF_TRY(cf_copy_h2d(ctx, d_bytes, edge_bytes + edge_off[0], (size_t)NE));
    if (NR > 0) CF_TRY(cf_copy_h2d(ctx, d_bytes + NE, read_bytes + read_off[0], (size_t)NR));
    CF_TRY(cf_copy_h2d(ctx, d_off, h_off.data(), ((size_t)S + 1) * 8));
    if (E > 0) {
        CF_TRY(cf_copy_h2d(ctx, d_uv, u, (size_t)E * 4));
        CF_TRY(cf_copy_h2d(ctx, d_uv + E, v, (size_t)E * 4));
    }
    CF_HIP(hipEventRecord(e1, ctx->stream));
    CF_HIP(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&t, e0, e1); copy_ms += t;

    cf_mk_ranked rk{};
    CF_TRY(cf_mk_rank_windows(ctx, tmp, d_bytes, d_off, S, N, k, gap, "cf_monomap_run", &rk));
    shape.n_rounds = rk.n_rounds;
    shape.n_sorts = rk.n_sorts;
    const int64_t V = rk.n_valid, D = rk.n_classes;

    if (V > 0 && E > 0) {
        tmp.drop(rk.rec2);
        uint32_t *d_cls = nullptr, *d_f = nullptr;
        int64_t* d_x = nullptr;
        CF_TRY(tmp.get(&d_cls, (size_t)D, "monomap classes"));
        CF_TRY(tmp.get(&d_f, n4, "monomap flags"));
        CF_TRY(tmp.get(&d_x, n4, "monomap scan"));
        hipLaunchKernelGGL(cf_mm_heads, grid(V), dim3(CF_MM_BLOCK), 0, ctx->stream, (const cf_mk_rec*)rk.rec, (const uint32_t*)rk.head, (const int64_t*)rk.e, d_cls,
                           d_f, V, D, NE);
        CF_KERNEL_CHECK("cf_mm_heads");
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_f, d_x, V, &shape.n_edge_windows));
        hipLaunchKernelGGL(cf_mm_indexed, grid(D), dim3(CF_MM_BLOCK), 0, ctx->stream, (const uint32_t*)d_cls, d_f, D);
        CF_KERNEL_CHECK("cf_mm_indexed");
        CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_f, d_x, D, &shape.n_indexed));
        if (shape.n_edge_windows < 0 || shape.n_edge_windows > V || shape.n_indexed < 0 || shape.n_indexed > std::min(D, shape.n_edge_windows))
            return cf_fail(ctx, -5, "cf_monomap_run: the indexed k-mers do not add up (internal error)");

        // the ranks and the distances are done with: their buffers hold the hits' edge positions and the hit flags, per position
        uint32_t *d_hit = rk.R, *d_flag = rk.dist;
        int64_t H = 0, P = 0, B = 0;
        CF_HIP(hipMemsetAsync(d_flag, 0, n4 * 4, ctx->stream));
        if (shape.n_indexed > 0 && NR > 0) {
            hipLaunchKernelGGL(cf_mm_scatter, grid(V), dim3(CF_MM_BLOCK), 0, ctx->stream, (const cf_mk_rec*)rk.rec, (const uint32_t*)rk.head, (const int64_t*)rk.e,
                               (const uint32_t*)d_cls, d_hit, d_flag, V, D, NE, N);
            CF_KERNEL_CHECK("cf_mm_scatter");
            CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_flag, d_x, N, &H));
            if (H < 0 || H > NR) return cf_fail(ctx, -5, "cf_monomap_run: the hits do not add up (internal error)");
        }
        if (H > 0) {
            cf_monomap_hit* d_hits = nullptr;
            int32_t *d_hread = nullptr, *d_path = nullptr;
            uint32_t *d_rf = nullptr, *d_bf = nullptr;
            int64_t *d_ps = rk.e, *d_bs = nullptr, *d_pptr = nullptr, *d_hptr = nullptr;      // (the classes' scan is done with)
            cf_monomap_read* d_reads = nullptr;
            CF_TRY(tmp.get(&d_hits, (size_t)H, "monomap hits"));
            CF_TRY(tmp.get(&d_hread, (size_t)H, "monomap hit reads"));
            CF_TRY(tmp.get(&d_rf, (size_t)H, "monomap run heads"));
            CF_TRY(tmp.get(&d_bf, (size_t)H, "monomap broken joins"));
            CF_TRY(tmp.get(&d_bs, (size_t)H, "monomap join scan"));
            CF_TRY(tmp.get(&d_reads, (size_t)R, "monomap reads"));
            CF_TRY(tmp.get(&d_pptr, (size_t)R, "monomap path offsets"));
            CF_TRY(tmp.get(&d_hptr, (size_t)R, "monomap hit offsets"));
            hipLaunchKernelGGL(cf_mm_compact, grid(NR), dim3(CF_MM_BLOCK), 0, ctx->stream, (const uint32_t*)d_flag, (const int64_t*)d_x, (const uint32_t*)d_hit,
                               (const int64_t*)d_off, E, S, d_hits, d_hread, N, NE, H);
            CF_KERNEL_CHECK("cf_mm_compact");
            hipLaunchKernelGGL(cf_mm_runs, grid(H), dim3(CF_MM_BLOCK), 0, ctx->stream, (const cf_monomap_hit*)d_hits, (const int32_t*)d_hread, (const int64_t*)d_off,
                               (const int64_t*)d_x, (const int32_t*)d_uv, (const int32_t*)(d_uv + E), d_rf, d_bf, H, E, R, N);
            CF_KERNEL_CHECK("cf_mm_runs");
            CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_rf, d_ps, H, &P));
            CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_bf, d_bs, H, &B));
            if (P < 1 || P > H || B < 0 || B > P) return cf_fail(ctx, -5, "cf_monomap_run: the paths do not add up (internal error)");
            CF_TRY(tmp.get(&d_path, (size_t)P, "monomap paths"));
            hipLaunchKernelGGL(cf_mm_paths, grid(H), dim3(CF_MM_BLOCK), 0, ctx->stream, (const cf_monomap_hit*)d_hits, (const uint32_t*)d_rf, (const int64_t*)d_ps,
                               d_path, H, P);
            CF_KERNEL_CHECK("cf_mm_paths");
            hipLaunchKernelGGL(cf_mm_reads, grid(R), dim3(CF_MM_BLOCK), 0, ctx->stream, (const int64_t*)d_off, (const int64_t*)d_x, (const int64_t*)d_ps,
                               (const int64_t*)d_bs, (const cf_monomap_hit*)d_hits, d_reads, d_pptr, d_hptr, E, R, N, H, P, B);
            CF_KERNEL_CHECK("cf_mm_reads");
            try {
                res_path.resize((size_t)P);
                if (with_hits) res_hits.resize((size_t)H);
            } catch (const std::bad_alloc&) {
                return cf_fail(ctx, -12, "cf_monomap_run: no host memory for " + std::to_string(P) + " path elements and " + std::to_string(H) + " hits");
            }
            CF_HIP(hipEventRecord(e2, ctx->stream));
            CF_TRY(cf_copy_d2h(ctx, res_reads.data(), d_reads, (size_t)R * sizeof(cf_monomap_read)));
            CF_TRY(cf_copy_d2h(ctx, res_pptr.data(), d_pptr, (size_t)R * 8));
            CF_TRY(cf_copy_d2h(ctx, res_hptr.data(), d_hptr, (size_t)R * 8));
            CF_TRY(cf_copy_d2h(ctx, res_path.data(), d_path, (size_t)P * 4));
            if (with_hits) CF_TRY(cf_copy_d2h(ctx, res_hits.data(), d_hits, (size_t)H * sizeof(cf_monomap_hit)));
            CF_HIP(hipEventRecord(e3, ctx->stream));
            CF_HIP(hipEventSynchronize(e3));
            (void)hipEventElapsedTime(&t, e2, e3); copy_ms += t;
            res_pptr[(size_t)R] = P;
            res_hptr[(size_t)R] = H;
            shape.n_hits = H;
            shape.n_path = P;
        }
    } else if (V > 0) {
        shape.n_edge_windows = 0;      // no edge at all: every valid window is a read's
    }
    CF_HIP(hipEventRecord(e1, ctx->stream));
    CF_HIP(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&t, e0, e1);
    shape.phase_ms[0] = copy_ms;
    shape.phase_ms[1] = rk.sort_ms;
    shape.phase_ms[2] = std::max(0.f, t - copy_ms - rk.sort_ms);
    shape.phase_ms[3] = t;
    return finish();
}

}  // extern "C"
