// cf_consensus.hip — the built-in consensus polisher: every contig position's reads aligned to the position's template, a vote per
// column and per insertion slot, the next template emitted; all positions and all iterations in one call (gfx950, wave64).
//
// Stands in for scripts/eltr_polisher.py:99-114 (run_polishing: one `flye --polish-target` process per position).  There is NO
// reference function behind it; the rule is written out at cf_consensus_run in include/cfhip.h and restated in tests/conscheck.py.
//
//   cf_cons_align_kernel  ONE WORKGROUP PER (template, read) PAIR, pairs of a batch taken by a ticket in descending m + n.  The
//                         strings go to LDS once.  The band |c| <= w of the NW matrix (c = j - i the diagonal of the cell i of the
//                         template, j of the read) is filled by anti-diagonals a = i + j: the cells of one anti-diagonal depend
//                         on the two before it only, the diagonals of the band that hold a cell of a are every second one, thread
//                         q takes the q-th of them, and val[c] in LDS holds the newest value of diagonal c: a cell reads its own
//                         diagonal (the value of a - 2) and both neighbours (values of a - 1, the other parity) and writes its
//                         own, so one __syncthreads() per anti-diagonal orders everything.  The move of the cell (rule a / b / c,
//                         2 bits) is decided right there and collected per diagonal in LDS, 16 rows to a word that goes to the
//                         pair's area in HBM: word (c - cmin) * RW + (i >> 4), RW = (m >> 4) + 1.  w starts at the pair's distance
//                         of the iteration before (32 at least, |n - m| at least) and doubles until D[m][n] <= w — then every cell
//                         of the walk lies in the band with its exact value, and an overestimated neighbour never satisfies an
//                         equality the true value does not — or until it is floor(permille m / 1000), the largest distance that
//                         still votes: D[m][n] > w there means the read does not vote.  Thread 0 then walks back from (m, n)
//                         through the moves: a byte per column (0 .. 3 the base on the diagonal, 4 deleted, 5 no vote) and 16 bits
//                         per slot (the length of the inserted run capped at 4 in bits 12 .. 14, bits 3k .. 3k + 2 = base and valid
//                         bit of its k-th byte).  Every loop is bounded by m + n, the band or the block.
//   cf_cons_vote_kernel   one thread per (position, slot s and column s): the rows of the position's reads lie back to back, so
//                         the threads of a wave read consecutive bytes of one row; 21 tallies in registers, no atomics; up to
//                         5 bytes and their count per thread, and beside every byte its support `agree` (the tally of the base
//                         emitted, 0 for a template byte kept with no vote: the rule at cf_consensus_run) in 16 bits, saturating at 65 535:
//                         5 x 2 contiguous bytes.  Only for cf_consensus_run_support (template argument SUPPORT): at the cenX shape the
//                         stores and the copies of the support cost more than the spread of the parent's runs.
//   cf_cons_compact_kernel / cf_cons_off_kernel   after the exclusive scan of cf_prims.hip over the counts: the next templates
//                         back to back and their offsets; the support moves with its byte through the same scan indices.
// With support, per read the host keeps, iteration by iteration, the vote flag and the distance as the align kernel left it (exact for a read that
// votes; a read that does not vote never had its distance established: -1), for cf_consensus_reads.
#include "cf_common.h"

#define CF_CONS_MAX_LEN 8192           // bytes of a template or a read: the strings and a full band fit the LDS window
#define CF_CONS_K_INS 4                // bases a pass adds per slot
#define CF_CONS_SMALL_BLOCK 64
#define CF_CONS_BIG_BLOCK 256
#define CF_CONS_BIG_FROM 128           // batches with a band of more diagonals than this take the large block
#define CF_CONS_WGS_PER_CU 8
#define CF_CONS_HEAD 16                // bytes of the LDS window in front of the strings: the ticket
#define CF_CONS_W0 32                  // the first half-width tried
#define CF_CONS_INF (1 << 29)
#define CF_CONS_VOTE_THREADS 256
#define CF_CONS_DEFAULT_BATCH ((int64_t)1 << 30)

// A, C, G, T (upper case only) -> 0 .. 3, anything else 5 ("no vote")
__device__ __forceinline__ uint32_t cf_cons_code(uint32_t b) { return cf_is_acgt(b) ? cf_base2(b) : 5u; }

__device__ __forceinline__ uint8_t cf_cons_letter(int code) { return (uint8_t)(0x54474341u >> (8 * code)); }      // 0 .. 3 -> A, C, G, T

// a tally as the support is stored: 16 bits, saturating
__device__ __forceinline__ uint16_t cf_cons_sat16(int32_t v) { return (uint16_t)(v < 65535 ? v : 65535); }

struct cf_cons_pairs {
    const uint8_t* t;            // the templates of this iteration, back to back
    const int64_t* t_off;        // n_pos + 1
    const uint8_t* r;            // the reads
    const int64_t* r_off;        // n_reads + 1
    const int32_t* pair_pos;     // position of every read
    const int64_t* order;        // pairs in descending m + n
    const int32_t* wcap;         // per pair: the largest half-width tried, -1 = |n - m| alone excludes the read
    const int64_t* area_off;     // per pair: first word of its move area inside the batch's areas
    const int64_t* col_off;      // per pair: first byte of its column row
    const int64_t* slot_off;     // per pair: first entry of its slot row
};

__global__ void __launch_bounds__(CF_CONS_BIG_BLOCK)
cf_cons_align_kernel(cf_cons_pairs in, int64_t first, int64_t last, int32_t permille, uint32_t* __restrict__ area, int32_t* __restrict__ dprev,
                     uint8_t* __restrict__ vote, uint8_t* __restrict__ col, uint16_t* __restrict__ slot, unsigned long long* __restrict__ ticket,
                     int32_t* __restrict__ fault) {
    volatile int64_t* head = (volatile int64_t*)cf_lds;
    const int tid = threadIdx.x, nth = blockDim.x;
    for (;;) {
        if (tid == 0) {
            const unsigned long long x = atomicAdd(ticket, 1ull);
            head[0] = x < (unsigned long long)(last - first) ? first + (int64_t)x : -1;
        }
        __syncthreads();
        const int64_t slot_in_order = head[0];
        if (slot_in_order < 0) break;
        const int64_t p = in.order[slot_in_order];
        const int32_t pos = in.pair_pos[p];
        const uint8_t* __restrict__ gt = in.t + in.t_off[pos];
        const uint8_t* __restrict__ gr = in.r + in.r_off[p];
        const int32_t m = (int32_t)(in.t_off[pos + 1] - in.t_off[pos]), n = (int32_t)(in.r_off[p + 1] - in.r_off[p]);
        const int32_t wcap = in.wcap[p];
        const int32_t cd = n - m, acd = cd < 0 ? -cd : cd;
        const int32_t dmax = (int32_t)(((int64_t)permille * m) / 1000 < (int64_t)CF_CONS_INF ? ((int64_t)permille * m) / 1000 : (int64_t)CF_CONS_INF);
        if (wcap < 0) {      // (uniform) the lengths alone put the read beyond the limit
            if (tid == 0) { vote[p] = 0; dprev[p] = acd; }
            __syncthreads();
            continue;
        }
        // LDS: the template, the read, then val and acc of the widest band of this pair
        uint8_t* lt = cf_lds + CF_CONS_HEAD;
        uint8_t* lr = lt + m;
        const int32_t wmax_diags = (n < wcap ? n : wcap) + (m < wcap ? m : wcap) + 1;
        int32_t* val = (int32_t*)(cf_lds + CF_CONS_HEAD + (((size_t)m + (size_t)n + 15) & ~(size_t)15));
        uint32_t* acc = (uint32_t*)(val + wmax_diags);
        for (int32_t i = tid; i < m; i += nth) lt[i] = gt[i];
        for (int32_t j = tid; j < n; j += nth) lr[j] = gr[j];
        const int32_t RW = (m >> 4) + 1;
        uint32_t* __restrict__ mv_area = area + in.area_off[p];
        int32_t w = dprev[p] > CF_CONS_W0 ? dprev[p] : CF_CONS_W0;
        w = w > acd ? w : acd;
        w = w < wcap ? w : wcap;
        int32_t res = CF_CONS_INF, cmin = 0, cmax = 0;
        __syncthreads();
        for (;;) {      // at most log2(wcap) + 1 rounds: w doubles or ends the loop
            cmin = -(m < w ? m : w);
            cmax = n < w ? n : w;
            for (int32_t a = 0; a <= m + n; ++a) {
                int32_t lo = cmin > -a ? cmin : -a;
                lo = lo > a - 2 * m ? lo : a - 2 * m;
                int32_t hi = cmax < a ? cmax : a;
                hi = hi < 2 * n - a ? hi : 2 * n - a;
                lo += (lo - a) & 1;      // the diagonals of this anti-diagonal have its parity
                for (int32_t c = lo + 2 * tid; c <= hi; c += 2 * nth) {
                    const int32_t i = (a - c) >> 1, j = (a + c) >> 1, k = c - cmin;
                    int32_t D;
                    uint32_t mv;
                    if (i == 0) { D = j; mv = 2u; }
                    else if (j == 0) { D = i; mv = 1u; }
                    else {
                        const int32_t diag = val[k] + (lt[i - 1] != lr[j - 1] ? 1 : 0);
                        const int32_t up = c + 1 <= cmax ? val[k + 1] + 1 : CF_CONS_INF;
                        const int32_t left = c - 1 >= cmin ? val[k - 1] + 1 : CF_CONS_INF;
                        D = diag < up ? diag : up;
                        D = D < left ? D : left;
                        mv = diag == D ? 0u : (up == D ? 1u : 2u);
                    }
                    val[k] = D;
                    uint32_t word = (i == 0 || j == 0 || (i & 15) == 0) ? 0u : acc[k];
                    word |= mv << (2 * (i & 15));
                    acc[k] = word;
                    if ((i & 15) == 15 || i == m || j == n) mv_area[(int64_t)k * RW + (i >> 4)] = word;
                }
                __syncthreads();
            }
            res = val[cd - cmin];
            if (res <= w || w >= wcap) break;      // (uniform: every thread reads the same cell after the barrier)
            __syncthreads();                       // every thread has read res before the next round writes val
            w = 2 * w < wcap ? 2 * w : wcap;
        }
        const bool exact = res <= w;
        if (tid == 0) {
            const bool votes = exact && res <= dmax;
            vote[p] = votes ? 1 : 0;
            dprev[p] = exact ? res : wcap;
            if (votes) {
                uint8_t* __restrict__ crow = col + in.col_off[p];
                uint16_t* __restrict__ srow = slot + in.slot_off[p];
                int32_t i = m, j = n, run_end = n;      // run_end: one past the last inserted byte of the slot being walked
                bool bad = false;
                for (int32_t step = 0; step <= m + n && (i > 0 || j > 0); ++step) {
                    const int32_t c = j - i;
                    if (c < cmin || c > cmax) { bad = true; break; }
                    uint32_t mv = (mv_area[(int64_t)(c - cmin) * RW + (i >> 4)] >> (2 * (i & 15))) & 3u;
                    if (i == 0) mv = 2u;
                    else if (j == 0) mv = 1u;
                    if (mv == 2u) { --j; continue; }
                    // the walk leaves row i: the run of slot i is r[j, run_end)
                    const int32_t len = run_end - j;
                    uint32_t e = (uint32_t)(len < CF_CONS_K_INS ? len : CF_CONS_K_INS) << 12;
                    for (int32_t q = 0; q < CF_CONS_K_INS && q < len; ++q) {
                        const uint32_t code = cf_cons_code(lr[j + q]);
                        if (code < 4u) e |= (code | 4u) << (3 * q);
                    }
                    srow[i] = (uint16_t)e;
                    if (mv == 0u) { crow[i - 1] = (uint8_t)cf_cons_code(lr[j - 1]); --i; --j; }
                    else { crow[i - 1] = 4; --i; }
                    run_end = j;
                }
                if (i != 0 || j != 0) bad = true;
                if (!bad) {      // slot 0: what is left of the read in front of the first column
                    const int32_t len = run_end;
                    uint32_t e = (uint32_t)(len < CF_CONS_K_INS ? len : CF_CONS_K_INS) << 12;
                    for (int32_t q = 0; q < CF_CONS_K_INS && q < len; ++q) {
                        const uint32_t code = cf_cons_code(lr[q]);
                        if (code < 4u) e |= (code | 4u) << (3 * q);
                    }
                    srow[0] = (uint16_t)e;
                } else {
                    *fault = 1;
                    vote[p] = 0;
                }
            }
        }
        __syncthreads();      // the strings and the ticket are read no more before they are written again
    }
}

// position of the global slot g: the last p with base[p] <= g, base[p] = t_off[p] + p
__device__ __forceinline__ int64_t cf_cons_pos_of(const int64_t* __restrict__ t_off, int64_t n_pos, int64_t g) {
    int64_t lo = 0, hi = n_pos - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (t_off[mid] + mid <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <bool SUPPORT>      // SUPPORT: cf_consensus_run_support asked for the support; without it the kernel stores what it always stored
__global__ void __launch_bounds__(CF_CONS_VOTE_THREADS)
cf_cons_vote_kernel(const uint8_t* __restrict__ t, const int64_t* __restrict__ t_off, int64_t n_pos, const int64_t* __restrict__ pos_ptr,
                    const uint8_t* __restrict__ vote, const uint8_t* __restrict__ col, const uint16_t* __restrict__ slot,
                    const int64_t* __restrict__ col_off, const int64_t* __restrict__ slot_off, uint8_t* __restrict__ emit, uint16_t* __restrict__ agree,
                    uint32_t* __restrict__ cnt) {
    const int64_t G = t_off[n_pos] - t_off[0] + n_pos;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = cf_cons_pos_of(t_off, n_pos, g + t_off[0]);
        const int32_t m = (int32_t)(t_off[p + 1] - t_off[p]), s = (int32_t)(g + t_off[0] - t_off[p] - p);
        int32_t ins[CF_CONS_K_INS][4] = {{0}}, cv[5] = {0, 0, 0, 0, 0}, c_v = 0;
        for (int64_t q = pos_ptr[p]; q < pos_ptr[p + 1]; ++q) {
            if (!vote[q]) continue;
            ++c_v;
            const uint32_t e = slot[slot_off[q] + s];
#pragma unroll
            for (int k = 0; k < CF_CONS_K_INS; ++k) {
                const uint32_t f = (e >> (3 * k)) & 7u;
#pragma unroll
                for (int b = 0; b < 4; ++b) ins[k][b] += f == (4u | (uint32_t)b) ? 1 : 0;
            }
            if (s < m) {
                const uint32_t x = col[col_off[q] + s];
#pragma unroll
                for (int b = 0; b < 5; ++b) cv[b] += x == (uint32_t)b ? 1 : 0;
            }
        }
        uint8_t* out = emit + g * (CF_CONS_K_INS + 1);
        uint16_t* sup = SUPPORT ? agree + g * (CF_CONS_K_INS + 1) : nullptr;      // (without SUPPORT there is no such array)
        uint32_t n_out = 0;
        bool open = true;
#pragma unroll
        for (int k = 0; k < CF_CONS_K_INS; ++k) {
            const int32_t v = ins[k][0] + ins[k][1] + ins[k][2] + ins[k][3];
            open = open && 2 * v > c_v;
            if (open) {
                int best = 0;
#pragma unroll
                for (int b = 1; b < 4; ++b) best = ins[k][b] > ins[k][best] ? b : best;
                if (SUPPORT) sup[n_out] = cf_cons_sat16(ins[k][best]);
                out[n_out++] = cf_cons_letter(best);
            }
        }
        if (s < m) {
            const uint32_t tb = t[t_off[p] + s];
            int best = 0;
#pragma unroll
            for (int b = 1; b < 5; ++b) best = cv[b] > cv[best] ? b : best;
            if (cv[best] == 0) { if (SUPPORT) sup[n_out] = 0; out[n_out++] = (uint8_t)tb; }      // the template byte kept with no vote
            else {
                const uint32_t tc = cf_cons_code(tb);
                if (tc < 4u && cv[tc] == cv[best]) best = (int)tc;
                if (best < 4) { if (SUPPORT) sup[n_out] = cf_cons_sat16(cv[best]); out[n_out++] = cf_cons_letter(best); }
            }
        }
        cnt[g] = n_out;
    }
}

template <bool SUPPORT>
__global__ void __launch_bounds__(CF_CONS_VOTE_THREADS)
cf_cons_compact_kernel(const uint8_t* __restrict__ emit, const uint16_t* __restrict__ agree, const uint32_t* __restrict__ cnt,
                       const int64_t* __restrict__ idx, int64_t G, uint8_t* __restrict__ out, uint16_t* __restrict__ out_agree) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < G; g += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t c = cnt[g] <= CF_CONS_K_INS + 1 ? cnt[g] : CF_CONS_K_INS + 1;
        const int64_t o = idx[g];
        for (uint32_t q = 0; q < c; ++q) {
            out[o + q] = emit[g * (CF_CONS_K_INS + 1) + q];
            if (SUPPORT) out_agree[o + q] = agree[g * (CF_CONS_K_INS + 1) + q];
        }
    }
}

// new_off[p] = bytes emitted in front of position p's first slot
__global__ void __launch_bounds__(CF_CONS_VOTE_THREADS)
cf_cons_off_kernel(const int64_t* __restrict__ t_off, int64_t n_pos, const int64_t* __restrict__ idx, int64_t total_out, int64_t* __restrict__ new_off) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= n_pos; p += (int64_t)gridDim.x * blockDim.x)
        new_off[p] = p < n_pos ? idx[t_off[p] - t_off[0] + p] : total_out;
}

static int cf_cons_launch_cap(const cf_ctx* ctx) { return std::max(1, ctx->n_cu) * CF_CONS_WGS_PER_CU; }

extern "C" {

int cf_consensus_info(cf_ctx* ctx, cf_consensus_shape* out) {
    if (!ctx || !out) return -22;
    *out = ctx->cons_last;
    out->max_len = CF_CONS_MAX_LEN;
    out->block_small = CF_CONS_SMALL_BLOCK;
    out->block_big = CF_CONS_BIG_BLOCK;
    out->big_from = CF_CONS_BIG_FROM;
    out->launch_cap = cf_cons_launch_cap(ctx);
    out->batch_bytes = ctx->cons_batch_bytes > 0 ? ctx->cons_batch_bytes : CF_CONS_DEFAULT_BATCH;
    out->k_ins = CF_CONS_K_INS;
    return 0;
}

int cf_consensus_get(cf_ctx* ctx, int32_t iter, uint8_t* out_bytes, int64_t* out_off, int32_t* n_voting, int32_t* n_excluded) {
    if (!ctx) return -22;
    if (iter < 1 || (size_t)iter > ctx->cons_bytes.size())
        return cf_fail(ctx, -22, "cf_consensus_get: iteration " + std::to_string(iter) + " is not one of the " + std::to_string(ctx->cons_bytes.size()) + " of the last run");
    const size_t i = (size_t)iter - 1;
    if (out_bytes && !ctx->cons_bytes[i].empty()) std::memcpy(out_bytes, ctx->cons_bytes[i].data(), ctx->cons_bytes[i].size());
    if (out_off) std::memcpy(out_off, ctx->cons_off[i].data(), ctx->cons_off[i].size() * 8);
    if (n_voting && !ctx->cons_voting[i].empty()) std::memcpy(n_voting, ctx->cons_voting[i].data(), ctx->cons_voting[i].size() * 4);
    if (n_excluded && !ctx->cons_excluded[i].empty()) std::memcpy(n_excluded, ctx->cons_excluded[i].data(), ctx->cons_excluded[i].size() * 4);
    return 0;
}

int cf_consensus_support(cf_ctx* ctx, int32_t iter, int32_t* agree) {
    if (!ctx) return -22;
    if (iter < 1 || (size_t)iter > ctx->cons_agree.size())
        return cf_fail(ctx, -22, "cf_consensus_support: iteration " + std::to_string(iter) + " is not one of the " + std::to_string(ctx->cons_agree.size()) + " of the last run with support (cf_consensus_run_support)");
    const std::vector<uint16_t>& a = ctx->cons_agree[(size_t)iter - 1];
    if (agree) std::copy(a.begin(), a.end(), agree);
    return 0;
}

int cf_consensus_reads(cf_ctx* ctx, int32_t iter, int32_t* dist, uint8_t* voted) {
    if (!ctx) return -22;
    if (iter < 1 || (size_t)iter > ctx->cons_dist.size())
        return cf_fail(ctx, -22, "cf_consensus_reads: iteration " + std::to_string(iter) + " is not one of the " + std::to_string(ctx->cons_dist.size()) + " of the last run with support (cf_consensus_run_support)");
    const size_t i = (size_t)iter - 1;
    if (dist && !ctx->cons_dist[i].empty()) std::memcpy(dist, ctx->cons_dist[i].data(), ctx->cons_dist[i].size() * 4);
    if (voted && !ctx->cons_voted[i].empty()) std::memcpy(voted, ctx->cons_voted[i].data(), ctx->cons_voted[i].size());
    return 0;
}

int cf_consensus_run(cf_ctx* ctx, const uint8_t* templates, const int64_t* t_off, const uint8_t* reads, const int64_t* r_off,
                     const int64_t* pos_ptr, int64_t n_pos, int32_t n_iters, int32_t permille, int64_t* total_bytes_out, float* ms_out) {
    return cf_consensus_run_support(ctx, templates, t_off, reads, r_off, pos_ptr, n_pos, n_iters, permille, 0, total_bytes_out, ms_out);
}

int cf_consensus_run_support(cf_ctx* ctx, const uint8_t* templates, const int64_t* t_off, const uint8_t* reads, const int64_t* r_off,
                             const int64_t* pos_ptr, int64_t n_pos, int32_t n_iters, int32_t permille, int32_t with_support,
                             int64_t* total_bytes_out, float* ms_out) {
    if (!ctx) return -22;
    if (ms_out) *ms_out = 0.f;
    if (n_pos < 0) return cf_fail(ctx, -22, "cf_consensus_run: negative number of positions");
    if (n_pos >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_consensus_run: more than 2^31 positions");
    if (n_iters < 1) return cf_fail(ctx, -22, "cf_consensus_run: fewer than one iteration");
    if (permille < 0) return cf_fail(ctx, -22, "cf_consensus_run: negative divergence limit");
    if (!t_off || !r_off || !pos_ptr) return cf_fail(ctx, -22, "cf_consensus_run: null offsets");
    if (pos_ptr[0] != 0) return cf_fail(ctx, -22, "cf_consensus_run: pos_ptr[0] must be 0");
    if (t_off[0] < 0) return cf_fail(ctx, -22, "cf_consensus_run: negative template offset");
    for (int64_t p = 0; p < n_pos; ++p) {
        if (pos_ptr[p + 1] < pos_ptr[p]) return cf_fail(ctx, -22, "cf_consensus_run: pos_ptr of position index " + std::to_string(p) + " decreases");
        if (t_off[p + 1] < t_off[p]) return cf_fail(ctx, -22, "cf_consensus_run: template offsets of position index " + std::to_string(p) + " decrease");
        if (t_off[p + 1] - t_off[p] > CF_CONS_MAX_LEN)
            return cf_fail(ctx, -22, "cf_consensus_run: the template of position index " + std::to_string(p) + " is longer than " + std::to_string(CF_CONS_MAX_LEN) + " bytes");
    }
    const int64_t n_reads = pos_ptr[n_pos];
    if (n_reads >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_consensus_run: more than 2^31 reads");
    if (r_off[0] < 0) return cf_fail(ctx, -22, "cf_consensus_run: negative read offset");
    for (int64_t q = 0; q < n_reads; ++q) {
        if (r_off[q + 1] < r_off[q]) return cf_fail(ctx, -22, "cf_consensus_run: offsets of read " + std::to_string(q) + " decrease");
        if (r_off[q + 1] - r_off[q] > CF_CONS_MAX_LEN)
            return cf_fail(ctx, -22, "cf_consensus_run: read " + std::to_string(q) + " is longer than " + std::to_string(CF_CONS_MAX_LEN) + " bytes");
    }
    const int64_t t_total = t_off[n_pos] - t_off[0], r_total = r_off[n_reads] - r_off[0];
    if ((t_total > 0 && !templates) || (r_total > 0 && !reads)) return cf_fail(ctx, -22, "cf_consensus_run: null bytes");

    // the results of this call, handed to the context only when everything worked
    std::vector<std::vector<uint8_t>> res_bytes((size_t)n_iters);
    std::vector<std::vector<int64_t>> res_off((size_t)n_iters);
    std::vector<std::vector<int32_t>> res_voting((size_t)n_iters), res_excluded((size_t)n_iters), res_dist(with_support ? (size_t)n_iters : 0);
    const bool support = with_support != 0;
    std::vector<std::vector<uint16_t>> res_agree(support ? (size_t)n_iters : 0);
    std::vector<std::vector<uint8_t>> res_voted(support ? (size_t)n_iters : 0);
    cf_consensus_shape shape{};
    shape.n_pos = n_pos;
    shape.n_reads = n_reads;
    shape.n_iters = n_iters;

    CF_HIP(hipSetDevice(ctx->device));
    hipEvent_t e0 = ctx->ev0, e1 = ctx->ev1, e2 = ctx->ev2, e3 = ctx->ev3;
    float ms = 0.f;
    cf_scratch tmp(ctx);
    // resident for the whole call: the reads, their offsets (from 0), the position of every read, the CSR, the pairs' figures
    std::vector<int64_t> h_r_off((size_t)n_reads + 1), h_t_off((size_t)n_pos + 1);
    for (int64_t q = 0; q <= n_reads; ++q) h_r_off[(size_t)q] = r_off[q] - r_off[0];
    for (int64_t p = 0; p <= n_pos; ++p) h_t_off[(size_t)p] = t_off[p] - t_off[0];
    std::vector<int32_t> h_pair_pos((size_t)n_reads);
    for (int64_t p = 0; p < n_pos; ++p)
        for (int64_t q = pos_ptr[p]; q < pos_ptr[p + 1]; ++q) h_pair_pos[(size_t)q] = (int32_t)p;
    uint8_t *d_reads = nullptr, *d_vote = nullptr;
    int64_t *d_r_off = nullptr, *d_pos_ptr = nullptr, *d_order = nullptr, *d_area_off = nullptr, *d_col_off = nullptr, *d_slot_off = nullptr;
    int32_t *d_pair_pos = nullptr, *d_wcap = nullptr, *d_dprev = nullptr, *d_fault = nullptr;
    unsigned long long* d_ticket = nullptr;
    CF_HIP(hipEventRecord(e0, ctx->stream));
    CF_TRY(tmp.get(&d_reads, (size_t)r_total + 16, "consensus reads"));
    CF_TRY(tmp.get(&d_r_off, (size_t)n_reads + 1, "consensus read offsets"));
    CF_TRY(tmp.get(&d_pos_ptr, (size_t)n_pos + 1, "consensus positions"));
    CF_TRY(tmp.get(&d_pair_pos, (size_t)n_reads + 1, "consensus pair positions"));
    CF_TRY(tmp.get(&d_order, (size_t)n_reads + 1, "consensus order"));
    CF_TRY(tmp.get(&d_area_off, (size_t)n_reads + 1, "consensus area offsets"));
    CF_TRY(tmp.get(&d_col_off, (size_t)n_reads + 1, "consensus column offsets"));
    CF_TRY(tmp.get(&d_slot_off, (size_t)n_reads + 1, "consensus slot offsets"));
    CF_TRY(tmp.get(&d_wcap, (size_t)n_reads + 1, "consensus band limits"));
    CF_TRY(tmp.get(&d_dprev, (size_t)n_reads + 1, "consensus distances"));
    CF_TRY(tmp.get(&d_vote, (size_t)n_reads + 1, "consensus votes"));
    CF_TRY(tmp.get(&d_fault, 1, "consensus fault flag"));
    if (r_total > 0) CF_TRY(cf_copy_h2d(ctx, d_reads, reads + r_off[0], (size_t)r_total));
    CF_TRY(cf_copy_h2d(ctx, d_r_off, h_r_off.data(), ((size_t)n_reads + 1) * 8));
    CF_TRY(cf_copy_h2d(ctx, d_pos_ptr, pos_ptr, ((size_t)n_pos + 1) * 8));
    if (n_reads > 0) CF_TRY(cf_copy_h2d(ctx, d_pair_pos, h_pair_pos.data(), (size_t)n_reads * 4));
    CF_HIP(hipMemsetAsync(d_dprev, 0, ((size_t)n_reads + 1) * 4, ctx->stream));
    CF_HIP(hipMemsetAsync(d_fault, 0, 4, ctx->stream));
    // the templates of the iteration: a buffer per iteration, the caller's first
    uint8_t* d_t = nullptr;
    int64_t* d_t_off = nullptr;
    CF_TRY(tmp.get(&d_t, (size_t)t_total + 16, "consensus templates"));
    CF_TRY(tmp.get(&d_t_off, (size_t)n_pos + 1, "consensus template offsets"));
    if (t_total > 0) CF_TRY(cf_copy_h2d(ctx, d_t, templates + t_off[0], (size_t)t_total));
    CF_TRY(cf_copy_h2d(ctx, d_t_off, h_t_off.data(), ((size_t)n_pos + 1) * 8));
    CF_HIP(hipEventRecord(e1, ctx->stream));
    CF_HIP(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&ms, e0, e1);
    shape.phase_ms[0] += ms;

    const int64_t batch_bytes = ctx->cons_batch_bytes > 0 ? ctx->cons_batch_bytes : CF_CONS_DEFAULT_BATCH;
    const int cap = cf_cons_launch_cap(ctx);
    std::vector<int64_t> order((size_t)n_reads), area_off((size_t)n_reads), col_off((size_t)n_reads), slot_off((size_t)n_reads);
    std::vector<int32_t> wcap((size_t)n_reads);
    std::vector<uint8_t> h_vote((size_t)n_reads);
    for (int32_t it = 0; it < n_iters; ++it) {
        // per pair: the rows, the largest half-width, the words of its move area; pairs in descending m + n, cut into batches
        const int64_t cur_total = h_t_off[(size_t)n_pos];
        int64_t col_total = 0, slot_total = 0;
        std::vector<int64_t> area_words((size_t)n_reads);
        for (int64_t q = 0; q < n_reads; ++q) {
            const int64_t p = h_pair_pos[(size_t)q];
            const int64_t m = h_t_off[(size_t)p + 1] - h_t_off[(size_t)p], n = h_r_off[(size_t)q + 1] - h_r_off[(size_t)q];
            col_off[(size_t)q] = col_total;
            slot_off[(size_t)q] = slot_total;
            col_total += m;
            slot_total += m + 1;
            const int64_t dmax = std::min<int64_t>((int64_t)permille * m / 1000, CF_CONS_INF), acd = n > m ? n - m : m - n;
            const int64_t wc = acd > dmax ? -1 : std::min(dmax, std::max(n, m));
            wcap[(size_t)q] = (int32_t)wc;
            area_words[(size_t)q] = wc < 0 ? 0 : (std::min(n, wc) + std::min(m, wc) + 1) * ((m >> 4) + 1);
            order[(size_t)q] = q;
        }
        std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
            const int64_t px = h_pair_pos[(size_t)x], py = h_pair_pos[(size_t)y];
            return h_t_off[(size_t)px + 1] - h_t_off[(size_t)px] + h_r_off[(size_t)x + 1] - h_r_off[(size_t)x] >
                   h_t_off[(size_t)py + 1] - h_t_off[(size_t)py] + h_r_off[(size_t)y + 1] - h_r_off[(size_t)y];
        });
        struct batch { int64_t first, last, words; int diags; size_t lds; };
        std::vector<batch> batches;
        for (int64_t o = 0; o < n_reads;) {
            batch b{o, o, 0, 1, 0};
            while (b.last < n_reads) {
                const int64_t q = order[(size_t)b.last], words = area_words[(size_t)q];
                if (b.last > b.first && (b.words + words) * 4 > batch_bytes) break;
                area_off[(size_t)q] = b.words;
                b.words += words;
                const int64_t p = h_pair_pos[(size_t)q];
                const int64_t m = h_t_off[(size_t)p + 1] - h_t_off[(size_t)p], n = h_r_off[(size_t)q + 1] - h_r_off[(size_t)q], wc = wcap[(size_t)q];
                const int64_t diags = wc < 0 ? 1 : std::min(n, wc) + std::min(m, wc) + 1;
                b.diags = (int)std::max<int64_t>(b.diags, diags);
                b.lds = std::max(b.lds, (size_t)CF_CONS_HEAD + (((size_t)m + (size_t)n + 15) & ~(size_t)15) + (size_t)diags * 8);
                ++b.last;
            }
            o = b.last;
            batches.push_back(b);
        }
        int64_t max_words = 1;
        for (const batch& b : batches) max_words = std::max(max_words, b.words);
        const int64_t G = cur_total + n_pos;

        CF_HIP(hipEventRecord(e0, ctx->stream));
        cf_scratch iter_tmp(ctx);
        uint32_t *d_area = nullptr, *d_cnt = nullptr;
        uint16_t *d_agree = nullptr, *d_next_agree = nullptr;
        uint8_t *d_col = nullptr, *d_emit = nullptr, *d_next = nullptr;
        uint16_t* d_slot = nullptr;
        int64_t *d_idx = nullptr, *d_next_off = nullptr;
        CF_TRY(iter_tmp.get(&d_area, (size_t)max_words, "consensus move areas"));
        CF_TRY(iter_tmp.get(&d_col, (size_t)col_total + 16, "consensus column rows"));
        CF_TRY(iter_tmp.get(&d_slot, (size_t)slot_total + 16, "consensus slot rows"));
        CF_TRY(iter_tmp.get(&d_emit, (size_t)G * (CF_CONS_K_INS + 1) + 16, "consensus emitted bytes"));
        if (support) CF_TRY(iter_tmp.get(&d_agree, (size_t)G * (CF_CONS_K_INS + 1) + 8, "consensus support"));
        CF_TRY(iter_tmp.get(&d_cnt, (size_t)G + 1, "consensus counts"));
        CF_TRY(iter_tmp.get(&d_idx, (size_t)G + 1, "consensus offsets"));
        CF_TRY(iter_tmp.get(&d_next_off, (size_t)n_pos + 1, "consensus template offsets"));
        CF_TRY(iter_tmp.get(&d_ticket, batches.size() + 1, "consensus tickets"));
        if (n_reads > 0) {
            CF_TRY(cf_copy_h2d(ctx, d_order, order.data(), (size_t)n_reads * 8));
            CF_TRY(cf_copy_h2d(ctx, d_area_off, area_off.data(), (size_t)n_reads * 8));
            CF_TRY(cf_copy_h2d(ctx, d_col_off, col_off.data(), (size_t)n_reads * 8));
            CF_TRY(cf_copy_h2d(ctx, d_slot_off, slot_off.data(), (size_t)n_reads * 8));
            CF_TRY(cf_copy_h2d(ctx, d_wcap, wcap.data(), (size_t)n_reads * 4));
        }
        CF_HIP(hipMemsetAsync(d_ticket, 0, (batches.size() + 1) * 8, ctx->stream));
        CF_HIP(hipEventRecord(e1, ctx->stream));
        CF_HIP(hipEventSynchronize(e1));
        (void)hipEventElapsedTime(&ms, e0, e1);      // (e0 is free again: it marks the end of the scan phase below)
        shape.phase_ms[0] += ms;
        cf_cons_pairs in{d_t, d_t_off, d_reads, d_r_off, d_pair_pos, d_order, d_wcap, d_area_off, d_col_off, d_slot_off};
        for (size_t b = 0; b < batches.size(); ++b) {
            const batch& bt = batches[b];
            const int block = bt.diags > CF_CONS_BIG_FROM ? CF_CONS_BIG_BLOCK : CF_CONS_SMALL_BLOCK;
            const int grid = (int)std::min<int64_t>(bt.last - bt.first, cap);
            if (bt.lds > ((size_t)64 << 10))
                CF_HIP(hipFuncSetAttribute((const void*)cf_cons_align_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bt.lds));
            hipLaunchKernelGGL(cf_cons_align_kernel, dim3((unsigned)grid), dim3((unsigned)block), bt.lds, ctx->stream, in, bt.first, bt.last, permille,
                               d_area, d_dprev, d_vote, d_col, d_slot, d_ticket + b, d_fault);
            CF_KERNEL_CHECK("cf_cons_align_kernel");
        }
        CF_HIP(hipEventRecord(e2, ctx->stream));
        int64_t total_out = 0;
        if (G > 0) {
            const int vgrid = cf_grid_for(G, CF_CONS_VOTE_THREADS, std::max(1, ctx->n_cu) * 16);
            hipLaunchKernelGGL(support ? cf_cons_vote_kernel<true> : cf_cons_vote_kernel<false>, dim3((unsigned)vgrid), dim3(CF_CONS_VOTE_THREADS), 0, ctx->stream, (const uint8_t*)d_t,
                               (const int64_t*)d_t_off, n_pos, (const int64_t*)d_pos_ptr, (const uint8_t*)d_vote, (const uint8_t*)d_col,
                               (const uint16_t*)d_slot, (const int64_t*)d_col_off, (const int64_t*)d_slot_off, d_emit, d_agree, d_cnt);
            CF_KERNEL_CHECK("cf_cons_vote_kernel");
            CF_HIP(hipEventRecord(e3, ctx->stream));
            CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_cnt, d_idx, G, &total_out));
            CF_TRY(iter_tmp.get(&d_next, (size_t)total_out + 16, "consensus templates"));
            if (support) CF_TRY(iter_tmp.get(&d_next_agree, (size_t)total_out + 8, "consensus support"));
            const int pgrid = cf_grid_for(n_pos + 1, CF_CONS_VOTE_THREADS, std::max(1, ctx->n_cu) * 16);
            hipLaunchKernelGGL(support ? cf_cons_compact_kernel<true> : cf_cons_compact_kernel<false>, dim3((unsigned)vgrid), dim3(CF_CONS_VOTE_THREADS), 0, ctx->stream, (const uint8_t*)d_emit,
                               (const uint16_t*)d_agree, (const uint32_t*)d_cnt, (const int64_t*)d_idx, G, d_next, d_next_agree);
            hipLaunchKernelGGL(cf_cons_off_kernel, dim3((unsigned)pgrid), dim3(CF_CONS_VOTE_THREADS), 0, ctx->stream, (const int64_t*)d_t_off, n_pos,
                               (const int64_t*)d_idx, total_out, d_next_off);
            CF_KERNEL_CHECK("the cf_cons_compact kernels");
        } else {
            CF_HIP(hipEventRecord(e3, ctx->stream));
            CF_TRY(iter_tmp.get(&d_next, 16, "consensus templates"));
            CF_HIP(hipMemsetAsync(d_next_off, 0, 8, ctx->stream));
        }
        CF_HIP(hipEventRecord(e0, ctx->stream));
        CF_HIP(hipEventSynchronize(e0));
        // e1 .. e2 alignment, e2 .. e3 vote, e3 .. e0 scan and compaction
        (void)hipEventElapsedTime(&ms, e1, e2); shape.phase_ms[1] += ms;
        (void)hipEventElapsedTime(&ms, e2, e3); shape.phase_ms[2] += ms;
        (void)hipEventElapsedTime(&ms, e3, e0); shape.phase_ms[3] += ms;
        shape.n_batches += (int64_t)batches.size();

        // this iteration's output to the host: it is the result, and its lengths shape the next iteration
        CF_HIP(hipEventRecord(e1, ctx->stream));
        int32_t h_fault = 0;
        CF_TRY(cf_copy_d2h(ctx, &h_fault, d_fault, 4));
        if (h_fault) return cf_fail(ctx, -5, "cf_consensus_run: a walk left its band (internal error)");
        res_bytes[(size_t)it].resize((size_t)total_out);
        res_off[(size_t)it].resize((size_t)n_pos + 1);
        if (total_out > 0) CF_TRY(cf_copy_d2h(ctx, res_bytes[(size_t)it].data(), d_next, (size_t)total_out));
        CF_TRY(cf_copy_d2h(ctx, res_off[(size_t)it].data(), d_next_off, ((size_t)n_pos + 1) * 8));
        if (n_reads > 0) CF_TRY(cf_copy_d2h(ctx, h_vote.data(), d_vote, (size_t)n_reads));
        if (support) {
            res_agree[(size_t)it].resize((size_t)total_out);
            if (total_out > 0) CF_TRY(cf_copy_d2h(ctx, res_agree[(size_t)it].data(), d_next_agree, (size_t)total_out * 2));
            // per read: the distance is exact where the read votes; elsewhere the band stopped at the limit (or the lengths alone
            // excluded the read) and d_dprev holds the next pass's first half-width, not a distance
            res_dist[(size_t)it].resize((size_t)n_reads);
            if (n_reads > 0) CF_TRY(cf_copy_d2h(ctx, res_dist[(size_t)it].data(), d_dprev, (size_t)n_reads * 4));
            for (int64_t q = 0; q < n_reads; ++q)
                if (!h_vote[(size_t)q]) res_dist[(size_t)it][(size_t)q] = -1;
            res_voted[(size_t)it] = h_vote;
        }
        res_voting[(size_t)it].assign((size_t)n_pos, 0);
        res_excluded[(size_t)it].assign((size_t)n_pos, 0);
        for (int64_t q = 0; q < n_reads; ++q) ++(h_vote[(size_t)q] ? res_voting : res_excluded)[(size_t)it][(size_t)h_pair_pos[(size_t)q]];
        h_t_off = res_off[(size_t)it];
        if (it + 1 < n_iters) {
            for (int64_t p = 0; p < n_pos; ++p)
                if (h_t_off[(size_t)p + 1] - h_t_off[(size_t)p] > CF_CONS_MAX_LEN)
                    return cf_fail(ctx, -22, "cf_consensus_run: the template of position index " + std::to_string(p) + " grew beyond " + std::to_string(CF_CONS_MAX_LEN) + " bytes in iteration " + std::to_string(it + 1));
            // the next iteration's templates take the place of this one's
            tmp.drop(d_t);
            tmp.drop(d_t_off);
            d_t = nullptr;
            d_t_off = nullptr;
            CF_TRY(tmp.get(&d_t, (size_t)total_out + 16, "consensus templates"));
            CF_TRY(tmp.get(&d_t_off, (size_t)n_pos + 1, "consensus template offsets"));
            if (total_out > 0) CF_HIP(hipMemcpyAsync(d_t, d_next, (size_t)total_out, hipMemcpyDeviceToDevice, ctx->stream));
            CF_HIP(hipMemcpyAsync(d_t_off, d_next_off, ((size_t)n_pos + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
        }
        CF_HIP(hipEventRecord(e2, ctx->stream));
        CF_HIP(hipEventSynchronize(e2));
        (void)hipEventElapsedTime(&ms, e1, e2);
        shape.phase_ms[0] += ms;
    }
    shape.phase_ms[4] = shape.phase_ms[0] + shape.phase_ms[1] + shape.phase_ms[2] + shape.phase_ms[3];
    for (int32_t it = 0; it < n_iters; ++it)
        if (total_bytes_out) total_bytes_out[it] = (int64_t)res_bytes[(size_t)it].size();
    if (ms_out) *ms_out = shape.phase_ms[4];
    ctx->cons_bytes.swap(res_bytes);
    ctx->cons_off.swap(res_off);
    ctx->cons_voting.swap(res_voting);
    ctx->cons_excluded.swap(res_excluded);
    ctx->cons_agree.swap(res_agree);
    ctx->cons_dist.swap(res_dist);
    ctx->cons_voted.swap(res_voted);
    ctx->cons_last = shape;
    return 0;
}

}  // extern "C"
