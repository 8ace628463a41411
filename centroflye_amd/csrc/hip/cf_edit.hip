// cf_edit.hip — global (NW) unit-cost edit distances of many byte-string pairs, and homopolymer compression (gfx950, wave64).
//
// Reference: scripts/eltr_polisher.py:133-146 (compare_polished_sequences: edlib.align(seq_i, seq_i+1) in its default mode NW,
// on the plain and on the homopolymer-compressed final sequences) and scripts/utils/bio.py:60-61 (compress_homopolymer).
// edlib's banded bit-vector NW costs O(n d / 64); successive polishing iterations differ in far less than 1 %, so the distance
// is found here by furthest-reaching points on diagonals (Ukkonen 1985, Myers 1986: O(n + d^2)).
//
//   cf_edit_kernel   ONE WORKGROUP PER PAIR, pairs taken by a ticket in descending n + m.  With c = j - i the diagonal of the
//                    cell (i of a, j of b) and F_s[c] the furthest i on c after s edits:
//                      F_0[0] = ext(0, 0)
//                      F_s[c] = ext(min(max(F_{s-1}[c] + 1, F_{s-1}[c-1], F_{s-1}[c+1] + 1), n, m - c), c)
//                    over max(-s, -n) <= c <= min(s, m); ext walks on while a[i] == b[i + c]; the answer is the first s with
//                    F_s[m - n] >= n.  A diagonal can lie on a path of at most kk edits only when |c| + |m - n - c| <= kk
//                    (kk = min(k, max(n, m)): the distance never exceeds the longer string), which is a band of at most kk + 1
//                    diagonals: the two wavefront arrays have that many entries, in LDS while they fit the launch's LDS
//                    window and in the workgroup's scratch area in HBM beyond (one __syncthreads() per step orders both).
//                    A step gives every wave 64 consecutive diagonals at a time.  A lane extends its own diagonal with
//                    8-byte compares (unaligned loads) for up to CF_EDIT_LANE_BYTES; a run that is still going is handed to the
//                    whole wave: CF_EDIT_UNROLL chunks of 1 KB per turn, 16 bytes per lane and chunk, one ballot per turn, the
//                    next turn's loads issued before it.  The device copy of the bytes is padded, loads may run past the end
//                    of a string, and every run is clamped to min(n - i, m - i - c): a padding byte never extends a match.
//   cf_hpc_*         keep byte i iff it starts a sequence or differs from byte i - 1: a start bitmap, a keep mask and a count
//                    per 8 bytes, the exclusive scan of cf_prims.hip over the counts, and a compaction.
#include "cf_common.h"

#define CF_EDIT_LDS_DIAGS 16384        // wavefront entries (diagonals) per array held in LDS: 2 x 64 KB of the 160 KB
#define CF_EDIT_HEAD 16                // bytes of the LDS window in front of the arrays: the ticket and the two finish flags
#define CF_EDIT_LANE_BYTES 32          // a lane's own run, in 8-byte compares
#define CF_EDIT_CHUNK 1024             // bytes a wave compares per chunk: 16 per lane
#define CF_EDIT_UNROLL 4               // chunks per turn of the wave
#define CF_EDIT_PAD 64                 // bytes behind the device copy (>= 16: a lane's last load starts below the end of its string)
#define CF_EDIT_NONE (-(1 << 30))      // F of a diagonal that is not part of the previous wavefront
#define CF_EDIT_SMALL_BLOCK 256
#define CF_EDIT_BIG_BLOCK 1024
#define CF_EDIT_BIG_FROM 2048          // bands of more diagonals than this take the large block
#define CF_EDIT_MAX_LEN 0x7fffff00ll

struct cf_u128 { unsigned long long x, y; };

__device__ __forceinline__ unsigned long long cf_edit_ld8(const uint8_t* p) { unsigned long long v; __builtin_memcpy(&v, p, 8); return v; }
__device__ __forceinline__ cf_u128 cf_edit_ld16(const uint8_t* p) { cf_u128 v; __builtin_memcpy(&v, p, 16); return v; }
// equal leading bytes of two 16-byte words (little endian), 0 .. 16
__device__ __forceinline__ int cf_edit_same16(const cf_u128& a, const cf_u128& b) {
    const unsigned long long x = a.x ^ b.x, y = a.y ^ b.y;
    return x ? (__builtin_ctzll(x) >> 3) : (y ? 8 + (__builtin_ctzll(y) >> 3) : 16);
}

struct cf_edit_turn { cf_u128 a[CF_EDIT_UNROLL], b[CF_EDIT_UNROLL]; };

// the loads of one turn of the wave: lane l takes bytes [off + u * 1 KB + 16 l, + 16) of both strings, below `lim` only
__device__ __forceinline__ void cf_edit_turn_load(cf_edit_turn& t, const uint8_t* __restrict__ pa, const uint8_t* __restrict__ pb, int64_t off,
                                                  int64_t lim, int lane) {
#pragma unroll
    for (int u = 0; u < CF_EDIT_UNROLL; ++u) {
        const int64_t o = off + (int64_t)u * CF_EDIT_CHUNK + lane * 16;
        const bool in = o < lim;
        t.a[u] = in ? cf_edit_ld16(pa + o) : cf_u128{0ull, 0ull};
        t.b[u] = in ? cf_edit_ld16(pb + o) : cf_u128{~0ull, ~0ull};      // (a lane at or beyond the limit stops the run)
    }
}

// All 64 lanes: the length of the common prefix of pa[0, lim) and pb[0, lim).
__device__ __forceinline__ int64_t cf_edit_ext_wave(const uint8_t* __restrict__ pa, const uint8_t* __restrict__ pb, int64_t lim, int lane) {
    cf_edit_turn cur, nxt;
    int64_t off = 0, run = lim;
    cf_edit_turn_load(cur, pa, pb, 0, lim, lane);
    while (off < lim) {
        cf_edit_turn_load(nxt, pa, pb, off + CF_EDIT_UNROLL * CF_EDIT_CHUNK, lim, lane);      // issued before this turn's ballot
        int same[CF_EDIT_UNROLL];
        bool stop = false;
#pragma unroll
        for (int u = 0; u < CF_EDIT_UNROLL; ++u) { same[u] = cf_edit_same16(cur.a[u], cur.b[u]); stop |= same[u] < 16; }
        if (__ballot(stop ? 1 : 0) != 0ull) {
            // (uniform) the first chunk with a stopped lane, its first such lane, that lane's equal bytes
            bool found = false;
#pragma unroll
            for (int u = 0; u < CF_EDIT_UNROLL; ++u) {
                const unsigned long long m = __ballot(same[u] < 16 ? 1 : 0);
                if (!found && m != 0ull) {
                    const int src = __builtin_ctzll(m);
                    run = off + (int64_t)u * CF_EDIT_CHUNK + src * 16 + __shfl(same[u], src);
                    found = true;
                }
            }
            break;
        }
        cur = nxt;
        off += CF_EDIT_UNROLL * CF_EDIT_CHUNK;
    }
    return run < lim ? run : lim;
}

__global__ void __launch_bounds__(CF_EDIT_BIG_BLOCK)
cf_edit_kernel(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ a_off, const int64_t* __restrict__ b_off,
               const int64_t* __restrict__ order, int64_t n_pairs, int32_t k, int lds_diags, int32_t* __restrict__ scratch,
               int64_t scratch_diags, unsigned long long* __restrict__ ticket, int32_t* __restrict__ dist) {
    volatile int32_t* head = (volatile int32_t*)cf_lds;      // [0] the pair's ticket, [1 + (s & 1)] the step that reached (n, m)
    int32_t* lds_f = (int32_t*)(cf_lds + CF_EDIT_HEAD);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthreads = blockDim.x;
    for (;;) {
        if (tid == 0) {
            const unsigned long long t = atomicAdd(ticket, 1ull);
            head[0] = t < (unsigned long long)n_pairs ? (int32_t)t : -1;      // (n_pairs < 2^31: the host checks)
            head[1] = -1;
            head[2] = -1;
        }
        __syncthreads();
        const int32_t t = head[0];
        if (t < 0) break;
        const int64_t p = order[t];
        const uint8_t* __restrict__ a = bytes + a_off[p];
        const uint8_t* __restrict__ b = bytes + b_off[p];
        const int32_t n = (int32_t)(a_off[p + 1] - a_off[p]), m = (int32_t)(b_off[p + 1] - b_off[p]);
        const int32_t cd = m - n, acd = cd < 0 ? -cd : cd, longer = n > m ? n : m;
        const int32_t kk = k < longer ? k : longer;
        int32_t result = -1;
        if (n == 0 || m == 0) {
            result = longer <= k ? longer : -1;      // (an empty string: the other one's length, without a step)
        } else if (acd <= kk) {
            // the band: |c| + |cd - c| <= kk, inside [-n, m]
            const int32_t half = (kk - acd) >> 1;
            int32_t cmin = (cd < 0 ? cd : 0) - half, cmax = (cd > 0 ? cd : 0) + half;
            cmin = cmin < -n ? -n : cmin;
            cmax = cmax > m ? m : cmax;
            const int32_t W = cmax - cmin + 1;
            int32_t* f0 = W <= lds_diags ? lds_f : scratch + (int64_t)blockIdx.x * 2 * scratch_diags;
            int32_t* f1 = W <= lds_diags ? lds_f + lds_diags : f0 + scratch_diags;
            if (wave == 0) {
                const int32_t lim = n < m ? n : m;
                const int32_t v = (int32_t)cf_edit_ext_wave(a, b, (int64_t)lim, lane);
                if (lane == 0) {
                    f0[0 - cmin] = v;
                    if (cd == 0 && v >= n) head[1] = 0;
                }
            }
            __syncthreads();
            int32_t s = 0;
            result = head[1];
            while (result < 0 && s < kk) {
                ++s;
                const int32_t* __restrict__ prev = (s & 1) ? f0 : f1;
                int32_t* __restrict__ cur = (s & 1) ? f1 : f0;
                const int32_t lo = -s > cmin ? -s : cmin, hi = s < cmax ? s : cmax;
                const int32_t plo = 1 - s > cmin ? 1 - s : cmin, phi = s - 1 < cmax ? s - 1 : cmax;
                for (int32_t base = lo + wave * 64; base <= hi; base += nthreads) {      // (uniform in the wave)
                    const int32_t c = base + lane;
                    const bool active = c <= hi;
                    int32_t i = 0, lim = 0;
                    bool going = false;
                    if (active) {
                        const int32_t up = (c >= plo && c <= phi) ? prev[c - cmin] + 1 : CF_EDIT_NONE;
                        const int32_t left = (c - 1 >= plo && c - 1 <= phi) ? prev[c - 1 - cmin] : CF_EDIT_NONE;
                        const int32_t right = (c + 1 >= plo && c + 1 <= phi) ? prev[c + 1 - cmin] + 1 : CF_EDIT_NONE;
                        int32_t v = up > left ? up : left;
                        v = right > v ? right : v;
                        const int32_t end = n < m - c ? n : m - c;      // the last i of the diagonal (a padding byte never matches past it)
                        v = v < end ? v : end;
                        lim = end - v;
                        const uint8_t* pa = a + v;
                        const uint8_t* pb = b + (int64_t)v + c;
                        int32_t run = 0;
                        going = lim > 0;
                        while (going && run < CF_EDIT_LANE_BYTES) {
                            const unsigned long long x = cf_edit_ld8(pa + run) ^ cf_edit_ld8(pb + run);
                            if (x != 0ull) { run += __builtin_ctzll(x) >> 3; going = false; }
                            else run += 8;
                            if (run >= lim) going = false;
                        }
                        run = run < lim ? run : lim;
                        i = v + run;
                        lim -= run;
                    }
                    // the runs that are still going, one after the other, by the whole wave
                    unsigned long long pending = __ballot(going ? 1 : 0);
                    while (pending != 0ull) {
                        const int src = __builtin_ctzll(pending);
                        pending &= pending - 1ull;
                        const int32_t ci = __shfl(c, src), ii = __shfl(i, src), li = __shfl(lim, src);
                        const int32_t r = (int32_t)cf_edit_ext_wave(a + ii, b + (int64_t)ii + ci, (int64_t)li, lane);
                        if (lane == src) i += r;
                    }
                    if (active) {
                        cur[c - cmin] = i;
                        if (c == cd && i >= n) head[1 + (s & 1)] = s;
                    }
                }
                __syncthreads();
                result = head[1 + (s & 1)];
            }
        }
        if (tid == 0) dist[p] = result;
        __syncthreads();      // every thread has read the ticket and the flags before they are written again
    }
}

// ------------------------------------------------------------------ homopolymer compression
#define CF_HPC_THREADS 256

// bit (off[s] & 7) of start[off[s] >> 3] for every sequence that begins below the end of the bytes (an empty sequence marks
// the start of the one that follows it at the same offset)
__global__ void __launch_bounds__(CF_HPC_THREADS)
cf_hpc_start_kernel(const int64_t* __restrict__ off, int64_t n_seqs, int64_t total, uint32_t* __restrict__ start) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n_seqs; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = off[s];
        if (o < total) atomicOr(&start[o >> 3], 1u << (uint32_t)(o & 7));
    }
}

// per group of 8 bytes: keep[g] = the bytes that start a sequence or differ from the byte before them; cnt[g] = how many
__global__ void __launch_bounds__(CF_HPC_THREADS)
cf_hpc_flag_kernel(const uint8_t* __restrict__ bytes, int64_t total, uint32_t* __restrict__ keep, uint32_t* __restrict__ cnt) {
    const int64_t G = (total + 7) >> 3;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = g << 3;
        const unsigned long long w = cf_edit_ld8(bytes + o);                          // (8-byte aligned; the copy is padded)
        const unsigned long long before = o > 0 ? (unsigned long long)bytes[o - 1] : 0ull;
        const unsigned long long x = w ^ ((w << 8) | before);                          // byte j: s[o + j] ^ s[o + j - 1]
        uint32_t mask = keep[g];
#pragma unroll
        for (int j = 0; j < 8; ++j) mask |= ((x >> (8 * j)) & 0xffull) ? (1u << j) : 0u;
        const int64_t left = total - o;
        mask &= left >= 8 ? 0xffu : ((1u << (uint32_t)left) - 1u);
        keep[g] = mask;
        cnt[g] = (uint32_t)__popc(mask);
    }
}

__global__ void __launch_bounds__(CF_HPC_THREADS)
cf_hpc_compact_kernel(const uint8_t* __restrict__ bytes, int64_t total, const uint32_t* __restrict__ keep, const int64_t* __restrict__ idx,
                      uint8_t* __restrict__ out) {
    const int64_t G = (total + 7) >> 3;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long w = cf_edit_ld8(bytes + (g << 3));
        const uint32_t mask = keep[g];
        int64_t o = idx[g];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if ((mask >> j) & 1u) out[o++] = (uint8_t)(w >> (8 * j));
    }
}

// out_off[s] = kept bytes in front of off[s]
__global__ void __launch_bounds__(CF_HPC_THREADS)
cf_hpc_off_kernel(const int64_t* __restrict__ off, int64_t n_seqs, int64_t total, int64_t total_out, const uint32_t* __restrict__ keep,
                  const int64_t* __restrict__ idx, int64_t* __restrict__ out_off) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= n_seqs; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = off[s];
        out_off[s] = o < total ? idx[o >> 3] + (int64_t)__popc(keep[o >> 3] & ((1u << (uint32_t)(o & 7)) - 1u)) : total_out;
    }
}

void cf_edit_free(cf_ctx* ctx) {
    if (ctx->d_edit) cf_release_t(ctx, ctx->d_edit, ctx->edit_cap);
    ctx->edit_cap = 0;
    ctx->edit_len = 0;
}

extern "C" {

int cf_edit_info(cf_ctx* ctx, int32_t* lds_diags, int32_t* lane_bytes, int32_t* turn_bytes, int32_t* block_small, int32_t* block_big,
                 int64_t* resident_bytes) {
    if (!ctx) return -22;
    if (lds_diags) *lds_diags = ctx->edit_lds_diags > 0 ? ctx->edit_lds_diags : CF_EDIT_LDS_DIAGS;
    if (lane_bytes) *lane_bytes = CF_EDIT_LANE_BYTES;
    if (turn_bytes) *turn_bytes = CF_EDIT_UNROLL * CF_EDIT_CHUNK;
    if (block_small) *block_small = CF_EDIT_SMALL_BLOCK;
    if (block_big) *block_big = CF_EDIT_BIG_BLOCK;
    if (resident_bytes) *resident_bytes = ctx->edit_len;
    return 0;
}

int cf_edit_distances(cf_ctx* ctx, const uint8_t* bytes, const int64_t* a_off, const int64_t* b_off, int64_t n_pairs, int32_t k,
                      int32_t* dist, float* ms) {
    if (!ctx) return -22;
    if (ms) *ms = 0.f;
    if (n_pairs < 0) return cf_fail(ctx, -22, "cf_edit_distances: negative number of pairs");
    if (n_pairs >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_edit_distances: more than 2^31 pairs");
    if (k < 0) return cf_fail(ctx, -22, "cf_edit_distances: negative distance limit");
    if (n_pairs == 0) return 0;
    if (!a_off || !b_off || !dist) return cf_fail(ctx, -22, "cf_edit_distances: null offsets or output");
    if (!bytes && !ctx->d_edit) return cf_fail(ctx, -22, "cf_edit_distances: no bytes given and none resident (cf_hpc)");
    int64_t total = 0;
    for (int s = 0; s < 2; ++s) {
        const int64_t* off = s ? b_off : a_off;
        if (off[0] < 0) return cf_fail(ctx, -22, "cf_edit_distances: negative offset");
        for (int64_t i = 0; i < n_pairs; ++i) {
            if (off[i + 1] < off[i]) return cf_fail(ctx, -22, "cf_edit_distances: offsets of pair " + std::to_string(i) + " decrease");
            if (off[i + 1] - off[i] > CF_EDIT_MAX_LEN) return cf_fail(ctx, -22, "cf_edit_distances: a string of pair " + std::to_string(i) + " is longer than 2^31 - 256 bytes");
        }
        total = std::max(total, off[n_pairs]);
    }
    if (!bytes && total > ctx->edit_len)
        return cf_fail(ctx, -22, "cf_edit_distances: offset " + std::to_string(total) + " lies beyond the " + std::to_string(ctx->edit_len) + " resident bytes");
    // pairs in descending n + m, and the widest band on either side of the LDS limit
    const int lds_limit = ctx->edit_lds_diags > 0 ? ctx->edit_lds_diags : CF_EDIT_LDS_DIAGS;
    std::vector<int64_t> order((size_t)n_pairs);
    int64_t w_lds = 1, w_hbm = 0;
    for (int64_t i = 0; i < n_pairs; ++i) {
        order[(size_t)i] = i;
        const int64_t n = a_off[i + 1] - a_off[i], m = b_off[i + 1] - b_off[i];
        const int64_t kk = std::min<int64_t>(k, std::max(n, m)), acd = m > n ? m - n : n - m;
        if (acd > kk || n == 0 || m == 0) continue;      // (answered without a wavefront)
        const int64_t half = (kk - acd) >> 1;
        const int64_t cmin = std::max(std::min<int64_t>(m - n, 0) - half, -n), cmax = std::min(std::max<int64_t>(m - n, 0) + half, m);
        const int64_t W = cmax - cmin + 1;
        if (W <= lds_limit) w_lds = std::max(w_lds, W); else w_hbm = std::max(w_hbm, W);
    }
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        return a_off[x + 1] - a_off[x] + b_off[x + 1] - b_off[x] > a_off[y + 1] - a_off[y] + b_off[y + 1] - b_off[y];
    });
    const int lds_diags = (int)((w_lds + 3) & ~(int64_t)3);
    const size_t lds = CF_EDIT_HEAD + (size_t)lds_diags * 8;
    const int block = std::max(w_lds, w_hbm) > CF_EDIT_BIG_FROM ? CF_EDIT_BIG_BLOCK : CF_EDIT_SMALL_BLOCK;
    const int per_cu = std::max(1, std::min((int)(((size_t)160 << 10) / lds), 2048 / block));
    const int grid = (int)std::min<int64_t>(n_pairs, (int64_t)std::max(1, ctx->n_cu) * per_cu);
    const int64_t scratch_diags = (w_hbm + 3) & ~(int64_t)3;
    CF_HIP(hipSetDevice(ctx->device));
    CF_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    uint8_t* d_bytes = nullptr;
    int64_t *d_a = nullptr, *d_b = nullptr, *d_order = nullptr;
    int32_t *d_scratch = nullptr, *d_dist = nullptr;
    unsigned long long* d_ticket = nullptr;
    const size_t n_scratch = (size_t)grid * 2 * (size_t)scratch_diags;
    cf_scratch tmp(ctx);
    if (bytes) {
        CF_TRY(tmp.get(&d_bytes, (size_t)total + CF_EDIT_PAD, "edit bytes"));
        if (total > 0) CF_TRY(cf_copy_h2d(ctx, d_bytes, bytes, (size_t)total));
        CF_HIP(hipMemsetAsync(d_bytes + total, 0, CF_EDIT_PAD, ctx->stream));
    }
    CF_TRY(tmp.get(&d_a, (size_t)n_pairs + 1, "edit offsets"));
    CF_TRY(tmp.get(&d_b, (size_t)n_pairs + 1, "edit offsets"));
    CF_TRY(tmp.get(&d_order, (size_t)n_pairs, "edit order"));
    CF_TRY(tmp.get(&d_dist, (size_t)n_pairs, "edit distances"));
    CF_TRY(tmp.get(&d_ticket, 1, "edit ticket"));
    if (n_scratch) CF_TRY(tmp.get(&d_scratch, n_scratch, "edit wavefronts"));
    CF_TRY(cf_copy_h2d(ctx, d_a, a_off, ((size_t)n_pairs + 1) * 8));
    CF_TRY(cf_copy_h2d(ctx, d_b, b_off, ((size_t)n_pairs + 1) * 8));
    CF_TRY(cf_copy_h2d(ctx, d_order, order.data(), (size_t)n_pairs * 8));
    CF_HIP(hipMemsetAsync(d_ticket, 0, 8, ctx->stream));
    if (lds > ((size_t)64 << 10)) CF_HIP(hipFuncSetAttribute((const void*)cf_edit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(cf_edit_kernel, dim3((unsigned)grid), dim3((unsigned)block), lds, ctx->stream,
                       (const uint8_t*)(bytes ? d_bytes : ctx->d_edit), (const int64_t*)d_a, (const int64_t*)d_b, (const int64_t*)d_order,
                       n_pairs, k, lds_diags, d_scratch, scratch_diags, d_ticket, d_dist);
    CF_KERNEL_CHECK("cf_edit_kernel");
    CF_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    CF_HIP(hipEventSynchronize(ctx->ev1));
    float t = 0.f;
    (void)hipEventElapsedTime(&t, ctx->ev0, ctx->ev1);
    if (ms) *ms = t;
    return cf_copy_d2h(ctx, dist, d_dist, (size_t)n_pairs * 4);
}

int cf_hpc(cf_ctx* ctx, const uint8_t* bytes, const int64_t* off, int64_t n_seqs, uint8_t* out_bytes, int64_t* out_off) {
    if (!ctx) return -22;
    if (n_seqs < 0) return cf_fail(ctx, -22, "cf_hpc: negative number of sequences");
    if (!off || !out_off) return cf_fail(ctx, -22, "cf_hpc: null offsets");
    if (off[0] != 0) return cf_fail(ctx, -22, "cf_hpc: off[0] must be 0");
    for (int64_t i = 0; i < n_seqs; ++i)
        if (off[i + 1] < off[i]) return cf_fail(ctx, -22, "cf_hpc: offsets of sequence " + std::to_string(i) + " decrease");
    const int64_t total = off[n_seqs];
    if (total > 0 && (!bytes || !out_bytes)) return cf_fail(ctx, -22, "cf_hpc: null bytes");
    CF_HIP(hipSetDevice(ctx->device));
    cf_edit_free(ctx);
    if (total == 0) {
        for (int64_t i = 0; i <= n_seqs; ++i) out_off[i] = 0;
        return 0;
    }
    // resident afterwards: the bytes, their compressed form right behind them, the padding
    const size_t cap = (size_t)total * 2 + CF_EDIT_PAD;
    const int64_t G = (total + 7) >> 3;
    const int grid = cf_grid_for(G, CF_HPC_THREADS, std::max(1, ctx->n_cu) * 16);
    const int sgrid = cf_grid_for(n_seqs + 1, CF_HPC_THREADS, std::max(1, ctx->n_cu) * 16);
    uint8_t* d_seq = nullptr;      // the context's once everything worked
    uint32_t *d_keep = nullptr, *d_cnt = nullptr;
    int64_t *d_idx = nullptr, *d_off = nullptr, *d_out_off = nullptr;
    int64_t total_out = 0;
    cf_scratch tmp(ctx);
    CF_TRY(tmp.get(&d_seq, cap, "resident sequences"));
    CF_TRY(tmp.get(&d_keep, (size_t)G, "hpc keep masks"));
    CF_TRY(tmp.get(&d_cnt, (size_t)G, "hpc counts"));
    CF_TRY(tmp.get(&d_idx, (size_t)G, "hpc offsets"));
    CF_TRY(tmp.get(&d_off, (size_t)n_seqs + 1, "sequence offsets"));
    CF_TRY(tmp.get(&d_out_off, (size_t)n_seqs + 1, "compressed offsets"));
    CF_TRY(cf_copy_h2d(ctx, d_seq, bytes, (size_t)total));
    CF_TRY(cf_copy_h2d(ctx, d_off, off, ((size_t)n_seqs + 1) * 8));
    CF_HIP(hipMemsetAsync(d_seq + total, 0, cap - (size_t)total, ctx->stream));
    CF_HIP(hipMemsetAsync(d_keep, 0, (size_t)G * 4, ctx->stream));
    hipLaunchKernelGGL(cf_hpc_start_kernel, dim3((unsigned)sgrid), dim3(CF_HPC_THREADS), 0, ctx->stream, (const int64_t*)d_off, n_seqs, total, d_keep);
    hipLaunchKernelGGL(cf_hpc_flag_kernel, dim3((unsigned)grid), dim3(CF_HPC_THREADS), 0, ctx->stream, (const uint8_t*)d_seq, total, d_keep, d_cnt);
    CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_cnt, d_idx, G, &total_out));
    hipLaunchKernelGGL(cf_hpc_compact_kernel, dim3((unsigned)grid), dim3(CF_HPC_THREADS), 0, ctx->stream, (const uint8_t*)d_seq, total,
                       (const uint32_t*)d_keep, (const int64_t*)d_idx, d_seq + total);
    hipLaunchKernelGGL(cf_hpc_off_kernel, dim3((unsigned)sgrid), dim3(CF_HPC_THREADS), 0, ctx->stream, (const int64_t*)d_off, n_seqs, total, total_out,
                       (const uint32_t*)d_keep, (const int64_t*)d_idx, d_out_off);
    CF_KERNEL_CHECK("the cf_hpc kernels");
    CF_HIP(hipStreamSynchronize(ctx->stream));
    CF_TRY(cf_copy_d2h(ctx, out_bytes, d_seq + total, (size_t)total_out));
    CF_TRY(cf_copy_d2h(ctx, out_off, d_out_off, ((size_t)n_seqs + 1) * 8));
    tmp.keep(d_seq);
    ctx->d_edit = d_seq;
    ctx->edit_cap = cap;
    ctx->edit_len = total + total_out;
    return 0;
}

}  // extern "C"
