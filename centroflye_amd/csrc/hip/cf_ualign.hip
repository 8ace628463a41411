// cf_ualign.hip — the built-in tandem aligner: every read against the unit read cyclically (local alignment with linear gaps on a
// cylinder), the best stretch per read with its alignment columns (gfx950, wave64).
//
// Stands in for the external NCRF binary of scripts/run_ncrf_parallel.py:49-62.  There is NO reference function behind it; the
// rule is written out at cf_ualign_run in include/cfhip.h and restated in tests/ualigncheck.py.
//
//   cf_ua_kernel<MOVES>   ONE WORKGROUP PER PAIR (read, strand), pairs taken by a ticket in descending number of rows.  Thread t holds
//                         the columns 16 t .. 16 t + 15 of the current row in registers (256 threads x 16 = 4 096 columns; a launch
//                         takes the multiple of 64 threads that holds the unit), the read goes through LDS in chunks of 1 024 bytes.
//                         A row is (1) the element-wise step A = max(0, diagonal, vertical): the diagonal input of a thread's first
//                         column is the final value of its left neighbour's last column, which the thread knows from its own carry
//                         of the row before (thread 0: the value of column m - 1, the wrap); (2) the cyclic max-plus scan: a serial
//                         scan of the 16 columns, a wave scan of the thread totals by lane shifts (6 steps, 16 d G per step), the wave
//                         totals through LDS [barrier 1], the value S'[m - 1] of the scan without the wrap through LDS [barrier 2],
//                         and S[j] = max(S'[j], S'[m - 1] - (j + 1) G): the row's end carry fed back to the front once.  Two LDS-only
//                         barriers per row; the LDS slots are double-buffered by the row's parity.  Every carry is clamped at 0: all
//                         values of the matrix are >= 0, so a carry <= 0 changes no cell and no equality of the walk, and no sum of
//                         gap costs leaves int32 (the multiples of G are saturated on the way in).
//                         MOVES = false (score pass): a thread keeps its best cell (first row, then first column among equals); the
//                         block's best goes out as (score, i, j).  Nothing is stored per cell.
//                         MOVES = true (moves pass, the winning strand, rows 1 .. r_en): a thread packs the moves of its 16 cells
//                         (0 stop, 1 rule a, 2 rule b, 3 rule c) into one word; the row's words are one coalesced store to the pair's
//                         area: word (i - 1) RW + t, RW = ceil(m / 16).  Wave 0 then walks back from the end cell, a run of diagonal
//                         moves per round: one op byte per alignment column (last column first; the host turns the string round)
//                         and the tallies.
//   Every loop is bounded by the rows of the pair, the block, or the pair's op capacity r_en + floor(r_en M / G) + 1 (a path of
//   positive score has fewer than M matches / G gap columns).  The only atomic is the ticket.
#include "cf_common.h"

#define CF_UA_MAX_UNIT 4096
#define CF_UA_CPT 16                   // columns of a row per thread
#define CF_UA_BLOCK 256
#define CF_UA_WGS_PER_CU 8
#define CF_UA_CHUNK 1024               // read bytes staged in LDS at a time
// LDS window: the ticket, the wave totals [2][4], S'[m - 1] [2], the threads' best cells [256][3], the read chunk
#define CF_UA_LDS_TOT 16
#define CF_UA_LDS_W 48
#define CF_UA_LDS_RED 64
#define CF_UA_LDS_READ (CF_UA_LDS_RED + CF_UA_BLOCK * 12)
#define CF_UA_LDS_BYTES (CF_UA_LDS_READ + CF_UA_CHUNK)

#ifndef cf_barrier_lds
// workgroup barrier that orders LDS traffic only: the stores of the move words need not have landed before the next row
__device__ __forceinline__ void cf_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#endif

struct cf_ua_pair {
    int64_t r_begin;             // first byte of the read
    int64_t area_off;            // moves pass: first word of the pair's move area
    int64_t ops_off;             // moves pass: first byte of the pair's op string
    int32_t n_rows;              // rows to fill: the read's length (score pass), r_en (moves pass)
    int32_t strand;
    int32_t j_end;               // moves pass: the end cell's column
    int32_t ops_cap;             // moves pass: room of the op string
};

__device__ __forceinline__ int32_t cf_ua_sat(int64_t x) { return x < (int64_t)0x7fffffff ? (int32_t)x : 0x7fffffff; }
__device__ __forceinline__ int32_t cf_ua_max(int32_t a, int32_t b) { return a > b ? a : b; }

template <bool MOVES>
__global__ void __launch_bounds__(CF_UA_BLOCK)
cf_ua_kernel(const cf_ua_pair* __restrict__ pairs, int64_t n_pairs, const uint8_t* __restrict__ reads, const uint8_t* __restrict__ units, int32_t m,
             int32_t M, int32_t X, int32_t G, int32_t* __restrict__ out, uint32_t* __restrict__ area, uint8_t* __restrict__ ops,
             unsigned long long* __restrict__ ticket, int32_t* __restrict__ fault) {
    volatile int64_t* head = (volatile int64_t*)cf_lds;
    volatile int32_t* tot = (volatile int32_t*)(cf_lds + CF_UA_LDS_TOT);
    volatile int32_t* wv = (volatile int32_t*)(cf_lds + CF_UA_LDS_W);
    volatile int32_t* red = (volatile int32_t*)(cf_lds + CF_UA_LDS_RED);
    volatile uint8_t* lr = (volatile uint8_t*)(cf_lds + CF_UA_LDS_READ);
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int32_t j0 = tid * CF_UA_CPT;
    const int32_t RW = (m + CF_UA_CPT - 1) / CF_UA_CPT;
    const int32_t tl = (m - 1) / CF_UA_CPT, kl = (m - 1) % CF_UA_CPT;      // the thread and the register of column m - 1
    const int32_t nact = m - j0 < 0 ? 0 : (m - j0 > CF_UA_CPT ? CF_UA_CPT : m - j0);      // columns of this thread inside the unit
    // multiples of G, saturated: a carry is >= 0 and clamped at 0, so a saturated cost gives the same 0 as the true one
    int32_t gsh[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) gsh[s] = cf_ua_sat((int64_t)G * CF_UA_CPT * (1 << s));
    const int32_t gfront = cf_ua_sat((int64_t)G * (j0 + 1));      // from column m - 1 round to this thread's first column
    const int32_t gleft = cf_ua_sat((int64_t)G * j0);             // ... to its left neighbour's last column
    int32_t gw[3];                                                // from the last column of wave w to that column
#pragma unroll
    for (int w = 0; w < 3; ++w) gw[w] = cf_ua_sat((int64_t)G * (j0 > 1024 * (w + 1) ? j0 - 1024 * (w + 1) : 0));
    for (;;) {
        if (tid == 0) {
            const unsigned long long x = atomicAdd(ticket, 1ull);
            head[0] = x < (unsigned long long)n_pairs ? (int64_t)x : -1;
        }
        __syncthreads();
        const int64_t idx = head[0];
        if (idx < 0) break;
        const cf_ua_pair pr = pairs[idx];
        const uint8_t* __restrict__ gu = units + (pr.strand ? m : 0);
        const uint8_t* __restrict__ gr = reads + pr.r_begin;
        uint32_t* __restrict__ mv_area = area + (MOVES ? pr.area_off : 0);
        const int32_t n_rows = pr.n_rows;
        uint32_t ub[CF_UA_CPT];      // 0xFF beyond the unit: no upper-cased byte equals it
        int32_t S[CF_UA_CPT];
#pragma unroll
        for (int k = 0; k < CF_UA_CPT; ++k) {
            ub[k] = k < nact ? (uint32_t)gu[j0 + k] : 0xFFu;
            S[k] = 0;
        }
        int32_t left = 0;                     // S[i - 1][p(j0)]
        int32_t bS = 0, bI = 0, bJ = 0;       // score pass: this thread's best cell
        for (int32_t i = 1; i <= n_rows; ++i) {
            if (((i - 1) & (CF_UA_CHUNK - 1)) == 0) {
                // (every thread read its byte of the chunk before in front of barrier 1 of the row before)
                for (int32_t x = tid; x < CF_UA_CHUNK && i - 1 + x < n_rows; x += nth) lr[x] = gr[i - 1 + x];
                __syncthreads();
            }
            const uint32_t rb = (uint32_t)lr[(i - 1) & (CF_UA_CHUNK - 1)] & 0xDFu;      // bit 5 cleared: a, c, g, t meet A, C, G, T; no other byte does
            const int buf = i & 1;
            // (1) element-wise, and the serial scan of this thread's columns
            int32_t P[CF_UA_CPT];
            int32_t dprev = left, run = 0;
#pragma unroll
            for (int k = 0; k < CF_UA_CPT; ++k) {
                const int32_t d = dprev + (rb == ub[k] ? M : -X), v = S[k] - G;
                dprev = S[k];
                int32_t a = cf_ua_max(cf_ua_max(d, v), 0);
                a = k < nact ? a : 0;
                run = cf_ua_max(a, run - G);
                P[k] = run;
            }
            // (2) the thread totals across the wave: E = the scan's value at this thread's last column, from this wave's columns
            int32_t E = run;
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const int32_t o = __shfl_up(E, 1u << s);
                if (lane >= (1 << s)) E = cf_ua_max(E, o - gsh[s]);
            }
            int32_t cin = __shfl_up(E, 1u);      // ... at the column in front of this thread's first
            if (lane == 0) cin = 0;
            if (lane == 63) tot[buf * 4 + wave] = E;
            cf_barrier_lds();
#pragma unroll
            for (int w = 0; w < 3; ++w)
                if (w < wave) cin = cf_ua_max(cin, tot[buf * 4 + w] - gw[w]);
            // S' = the scan without the wrap
            int32_t c = cin;
#pragma unroll
            for (int k = 0; k < CF_UA_CPT; ++k) {
                c = cf_ua_max(c - G, 0);
                P[k] = cf_ua_max(P[k], c);
            }
            if (tid == tl) {
                int32_t x = 0;
#pragma unroll
                for (int k = 0; k < CF_UA_CPT; ++k) x = k == kl ? P[k] : x;
                wv[buf] = x;
            }
            cf_barrier_lds();
            const int32_t W = wv[buf];      // S'[m - 1] = S[i][m - 1]
            c = cf_ua_max(W - gfront, 0);
            uint32_t word = 0;
            int32_t rowmax = 0;
            dprev = left;
#pragma unroll
            for (int k = 0; k < CF_UA_CPT; ++k) {
                const int32_t s_new = cf_ua_max(P[k], c);
                c = cf_ua_max(c - G, 0);
                if (MOVES) {
                    const int32_t d = dprev + (rb == ub[k] ? M : -X), v = S[k] - G;
                    dprev = S[k];
                    const uint32_t mv = s_new == 0 ? 0u : (d == s_new ? 1u : (v == s_new ? 2u : 3u));
                    word |= mv << (2 * k);
                } else {
                    rowmax = cf_ua_max(rowmax, s_new);
                }
                S[k] = s_new;
            }
            left = tid == 0 ? W : cf_ua_max(cin, cf_ua_max(W - gleft, 0));
            if (MOVES) {
                if (tid < RW) mv_area[(int64_t)(i - 1) * RW + tid] = word;
            } else if (nact > 0 && rowmax > bS) {
#pragma unroll
                for (int k = 0; k < CF_UA_CPT; ++k)
                    if (k < nact && S[k] > bS) { bS = S[k]; bI = i; bJ = j0 + k; }
            }
        }
        if (!MOVES) {
            red[3 * tid] = bS; red[3 * tid + 1] = bI; red[3 * tid + 2] = bJ;
            __syncthreads();
            if (tid == 0) {      // threads hold ascending columns: the first of the largest score with the smallest row
                int32_t s = 0, bi = 0, bj = 0;
                for (int t = 0; t < nth; ++t) {
                    const int32_t ts = red[3 * t], ti = red[3 * t + 1];
                    if (ts > s || (ts == s && ts > 0 && ti < bi)) { s = ts; bi = ti; bj = red[3 * t + 2]; }
                }
                out[3 * idx] = s; out[3 * idx + 1] = bi; out[3 * idx + 2] = bj;
            }
        } else {
            __syncthreads();      // every move word of the pair is visible to the walking wave
            if (wave == 0) {
                // The walk is a chain of dependent loads from HBM, and nearly every move is a diagonal: lane l looks at the cell l
                // diagonal steps back from (i, j), the leading run of diagonal moves is taken in one round (64 columns per round
                // trip to memory), then the one move that ended it.  Every value below is the same in all lanes.
                uint8_t* __restrict__ po = ops + pr.ops_off;
                int32_t i = n_rows, j = pr.j_end, n_ops = 0, u_st = 0, m_al = 0, cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
                bool stopped = false;
                for (int32_t round = 0; round <= pr.ops_cap; ++round) {      // a round takes at least one column or ends the walk
                    if (n_ops > pr.ops_cap) break;      // (the string has 64 bytes of room behind its capacity: a round writes inside it)
                    const int32_t il = i - lane;
                    int32_t jl = (j - lane) % m;
                    jl = jl < 0 ? jl + m : jl;
                    uint32_t mv = 0u;      // row 0 stops
                    if (il >= 1) mv = (mv_area[(int64_t)(il - 1) * RW + (jl >> 4)] >> (2 * (jl & 15))) & 3u;
                    const unsigned long long diag = __ballot(mv == 1u);
                    const int32_t run = diag == ~0ull ? 64 : (int32_t)__builtin_ctzll(~diag);
                    bool is_match = false;
                    if (lane < run) {
                        is_match = ((uint32_t)gr[il - 1] & 0xDFu) == (uint32_t)gu[jl];
                        po[n_ops + lane] = is_match ? (uint8_t)0 : (uint8_t)1;
                    }
                    const int32_t n_match = (int32_t)__popcll(__ballot(is_match));
                    if (run > 0) u_st = __shfl((int)jl, run - 1);
                    cnt0 += n_match; cnt1 += run - n_match; m_al += run; n_ops += run; i -= run;
                    if (run == 64) { j = __shfl((int)jl, 63); j = j == 0 ? m - 1 : j - 1; continue; }
                    j = __shfl((int)jl, run);
                    const uint32_t end = (uint32_t)__shfl((int)mv, run);      // the move of the cell the run stopped at: not a diagonal
                    if (end == 0u) { stopped = true; break; }
                    if (end == 2u) { --i; ++cnt2; }
                    else { u_st = j; j = j == 0 ? m - 1 : j - 1; ++m_al; ++cnt3; }
                    if (lane == 0) po[n_ops] = (uint8_t)end;
                    ++n_ops;
                }
                if (lane == 0) {
                    if (!stopped || n_ops > pr.ops_cap) *fault = 1;
                    int32_t* o = out + 8 * idx;
                    o[0] = i; o[1] = u_st; o[2] = m_al; o[3] = n_ops; o[4] = cnt0; o[5] = cnt1; o[6] = cnt2; o[7] = cnt3;
                }
            }
        }
        __syncthreads();      // the ticket and the LDS slots are read no more before they are written again
    }
}

// move areas per batch unless the knob says otherwise: an eighth of the device's memory, 2^28 .. 2^34 bytes (a launch should have a
// workgroup for every CU: a pair of 20 000 x 2 055 takes 10 MB)
static int64_t cf_ua_batch_bytes(const cf_ctx* ctx) {
    if (ctx->ualign_batch_bytes > 0) return ctx->ualign_batch_bytes;
    return std::min<int64_t>(std::max<int64_t>(ctx->hbm_total / 8, (int64_t)1 << 28), (int64_t)1 << 34);
}
static int cf_ua_launch_cap(const cf_ctx* ctx) { return std::max(1, ctx->n_cu) * CF_UA_WGS_PER_CU; }
static int cf_ua_block_for(int32_t m) { return std::min(CF_UA_BLOCK, (((m + CF_UA_CPT - 1) / CF_UA_CPT + 63) / 64) * 64); }

extern "C" {

int cf_ualign_info(cf_ctx* ctx, cf_ualign_shape* out) {
    if (!ctx || !out) return -22;
    *out = ctx->ualign_last;
    out->max_unit = CF_UA_MAX_UNIT;
    out->cols_per_thread = CF_UA_CPT;
    out->block = CF_UA_BLOCK;
    out->row_chunk = CF_UA_CHUNK;
    out->launch_cap = cf_ua_launch_cap(ctx);
    out->batch_bytes = cf_ua_batch_bytes(ctx);
    return 0;
}

int cf_ualign_ops(cf_ctx* ctx, int64_t* ptr, uint8_t* ops, int64_t cap, int64_t* n_out) {
    if (!ctx) return -22;
    if (ctx->ualign_op_ptr.empty()) return cf_fail(ctx, -22, "cf_ualign_ops: no cf_ualign_run before");
    const int64_t n = (int64_t)ctx->ualign_op_bytes.size();
    if (n_out) *n_out = n;
    if (!ptr && !ops) return 0;
    if (cap < n) return cf_fail(ctx, -22, "cf_ualign_ops: room for " + std::to_string(cap) + " ops, " + std::to_string(n) + " needed");
    if (ptr) std::memcpy(ptr, ctx->ualign_op_ptr.data(), ctx->ualign_op_ptr.size() * 8);
    if (ops && n) std::memcpy(ops, ctx->ualign_op_bytes.data(), (size_t)n);
    return 0;
}

int cf_ualign_run(cf_ctx* ctx, const uint8_t* unit, int32_t unit_len, const uint8_t* reads, const int64_t* read_off, int64_t n_reads,
                  int32_t match, int32_t mismatch, int32_t gap, cf_ualign_hit* hits, float* ms_out) {
    if (!ctx) return -22;
    if (ms_out) *ms_out = 0.f;
    if (n_reads < 0 || n_reads >= (int64_t)1 << 30) return cf_fail(ctx, -22, "cf_ualign_run: the number of reads is outside 0 .. 2^30 - 1");
    if (unit_len < 1 || unit_len > CF_UA_MAX_UNIT)
        return cf_fail(ctx, -22, "cf_ualign_run: a unit of " + std::to_string(unit_len) + " bases (1 .. " + std::to_string(CF_UA_MAX_UNIT) + " are taken)");
    if (!unit || !read_off || (n_reads > 0 && !hits)) return cf_fail(ctx, -22, "cf_ualign_run: null pointer");
    for (int32_t j = 0; j < unit_len; ++j)
        if (unit[j] != 'A' && unit[j] != 'C' && unit[j] != 'G' && unit[j] != 'T')
            return cf_fail(ctx, -22, "cf_ualign_run: unit byte " + std::to_string(j) + " is not upper-case A, C, G or T");
    if (match < 1 || mismatch < 1 || gap < 1) return cf_fail(ctx, -22, "cf_ualign_run: match, mismatch and gap must be at least 1");
    if (read_off[0] < 0) return cf_fail(ctx, -22, "cf_ualign_run: negative read offset");
    for (int64_t q = 0; q < n_reads; ++q) {
        if (read_off[q + 1] < read_off[q]) return cf_fail(ctx, -22, "cf_ualign_run: offsets of read " + std::to_string(q) + " decrease");
        if ((read_off[q + 1] - read_off[q]) >= (((int64_t)1 << 31) + match - 1) / match)
            return cf_fail(ctx, -22, "cf_ualign_run: read " + std::to_string(q) + " of " + std::to_string(read_off[q + 1] - read_off[q]) + " bytes could score 2^31 or more");
    }
    const int64_t r_total = read_off[n_reads] - read_off[0];
    if (r_total > 0 && !reads) return cf_fail(ctx, -22, "cf_ualign_run: null bytes");
    const int32_t m = unit_len;

    // the results of this call, handed to the context only when everything worked
    std::vector<cf_ualign_hit> res_hits((size_t)n_reads, cf_ualign_hit{});
    std::vector<int64_t> res_ptr((size_t)n_reads + 1, 0);
    std::vector<uint8_t> res_ops;
    cf_ualign_shape shape{};
    shape.n_reads = n_reads;

    // both strands of the unit; the score pass's pairs in descending length (empty reads have no hit and no pair)
    std::vector<uint8_t> h_units((size_t)2 * m);
    for (int32_t j = 0; j < m; ++j) {
        const uint8_t b = unit[m - 1 - j];
        h_units[(size_t)j] = unit[j];
        h_units[(size_t)m + j] = b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'A';
    }
    std::vector<int64_t> by_len;
    for (int64_t q = 0; q < n_reads; ++q)
        if (read_off[q + 1] > read_off[q]) by_len.push_back(q);
    std::stable_sort(by_len.begin(), by_len.end(), [&](int64_t x, int64_t y) { return read_off[x + 1] - read_off[x] > read_off[y + 1] - read_off[y]; });
    std::vector<cf_ua_pair> p1(2 * by_len.size());
    for (size_t o = 0; o < by_len.size(); ++o)
        for (int s = 0; s < 2; ++s) {
            const int64_t q = by_len[o];
            p1[2 * o + s] = cf_ua_pair{read_off[q] - read_off[0], 0, 0, (int32_t)(read_off[q + 1] - read_off[q]), s, 0, 0};
        }
    const int64_t n1 = (int64_t)p1.size();
    shape.n_score_pairs = n1;

    CF_HIP(hipSetDevice(ctx->device));
    hipEvent_t e0 = ctx->ev0, e1 = ctx->ev1, e2 = ctx->ev2;
    float t = 0.f;
    cf_scratch tmp(ctx);
    uint8_t *d_reads = nullptr, *d_units = nullptr;
    cf_ua_pair* d_p1 = nullptr;
    int32_t *d_best = nullptr, *d_fault = nullptr;
    unsigned long long* d_ticket = nullptr;
    CF_HIP(hipEventRecord(e0, ctx->stream));
    CF_TRY(tmp.get(&d_reads, (size_t)r_total + 16, "ualign reads"));
    CF_TRY(tmp.get(&d_units, (size_t)2 * m + 16, "ualign unit"));
    CF_TRY(tmp.get(&d_p1, (size_t)n1 + 1, "ualign score pairs"));
    CF_TRY(tmp.get(&d_best, (size_t)3 * n1 + 4, "ualign best cells"));
    CF_TRY(tmp.get(&d_fault, 1, "ualign fault flag"));
    CF_TRY(tmp.get(&d_ticket, 1, "ualign ticket"));
    if (r_total > 0) CF_TRY(cf_copy_h2d(ctx, d_reads, reads + read_off[0], (size_t)r_total));
    CF_TRY(cf_copy_h2d(ctx, d_units, h_units.data(), (size_t)2 * m));
    if (n1 > 0) CF_TRY(cf_copy_h2d(ctx, d_p1, p1.data(), (size_t)n1 * sizeof(cf_ua_pair)));
    CF_HIP(hipMemsetAsync(d_fault, 0, 4, ctx->stream));
    CF_HIP(hipMemsetAsync(d_ticket, 0, 8, ctx->stream));
    CF_HIP(hipEventRecord(e1, ctx->stream));
    const int cap = cf_ua_launch_cap(ctx), block = cf_ua_block_for(m);
    if (n1 > 0) {
        hipLaunchKernelGGL(cf_ua_kernel<false>, dim3((unsigned)std::min<int64_t>(n1, cap)), dim3((unsigned)block), CF_UA_LDS_BYTES, ctx->stream,
                           (const cf_ua_pair*)d_p1, n1, (const uint8_t*)d_reads, (const uint8_t*)d_units, m, match, mismatch, gap, d_best,
                           (uint32_t*)nullptr, (uint8_t*)nullptr, d_ticket, d_fault);
        CF_KERNEL_CHECK("cf_ua_kernel (score pass)");
    }
    CF_HIP(hipEventRecord(e2, ctx->stream));
    CF_HIP(hipEventSynchronize(e2));
    (void)hipEventElapsedTime(&t, e0, e1); shape.phase_ms[0] += t;
    (void)hipEventElapsedTime(&t, e1, e2); shape.phase_ms[1] += t;

    CF_HIP(hipEventRecord(e0, ctx->stream));
    std::vector<int32_t> best((size_t)3 * n1 + 4);
    if (n1 > 0) CF_TRY(cf_copy_d2h(ctx, best.data(), d_best, (size_t)3 * n1 * 4));
    CF_HIP(hipEventRecord(e1, ctx->stream));
    CF_HIP(hipEventSynchronize(e1));
    (void)hipEventElapsedTime(&t, e0, e1); shape.phase_ms[0] += t;

    // the winning strand of every read with a hit ("+" on a tie); the moves pass's pairs in descending rows, cut into batches
    struct win { int64_t q; int32_t strand, score, i, j; int64_t words, cap; };
    std::vector<win> wins;
    for (size_t o = 0; o < by_len.size(); ++o) {
        const int32_t* f = &best[6 * o];
        const int s = f[3] > f[0] ? 1 : 0;
        if (f[3 * s] <= 0) continue;
        const int64_t i_end = f[3 * s + 1], RW = (m + CF_UA_CPT - 1) / CF_UA_CPT;
        wins.push_back(win{by_len[o], s, f[3 * s], f[3 * s + 1], f[3 * s + 2], i_end * RW, i_end + i_end * (int64_t)match / gap + 1});
    }
    for (const win& w : wins)
        if (w.cap >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_ualign_run: the op string of read " + std::to_string(w.q) + " could hold 2^31 columns or more");
    std::stable_sort(wins.begin(), wins.end(), [](const win& a, const win& b) { return a.i > b.i; });
    const int64_t batch_bytes = cf_ua_batch_bytes(ctx);
    shape.n_move_pairs = (int64_t)wins.size();
    std::vector<std::vector<uint8_t>> rev_ops(wins.size());
    for (size_t first = 0; first < wins.size();) {
        size_t last = first;
        int64_t words = 0, op_bytes = 0;
        std::vector<cf_ua_pair> p2;
        while (last < wins.size()) {
            const win& w = wins[last];
            if (last > first && (words + w.words) * 4 > batch_bytes) break;
            p2.push_back(cf_ua_pair{read_off[w.q] - read_off[0], words, op_bytes, w.i, w.strand, w.j, (int32_t)w.cap});
            words += w.words;
            op_bytes += w.cap + 64;      // (the walking wave writes a round of up to 64 columns before it looks at the room)
            ++last;
        }
        const int64_t n2 = (int64_t)(last - first);
        CF_HIP(hipEventRecord(e0, ctx->stream));
        cf_scratch batch_tmp(ctx);
        cf_ua_pair* d_p2 = nullptr;
        uint32_t* d_area = nullptr;
        uint8_t* d_ops = nullptr;
        int32_t* d_res = nullptr;
        CF_TRY(batch_tmp.get(&d_p2, (size_t)n2, "ualign move pairs"));
        CF_TRY(batch_tmp.get(&d_area, (size_t)words + 1, "ualign move areas"));
        CF_TRY(batch_tmp.get(&d_ops, (size_t)op_bytes + 16, "ualign op strings"));
        CF_TRY(batch_tmp.get(&d_res, (size_t)8 * n2, "ualign walk results"));
        CF_TRY(cf_copy_h2d(ctx, d_p2, p2.data(), (size_t)n2 * sizeof(cf_ua_pair)));
        CF_HIP(hipMemsetAsync(d_ticket, 0, 8, ctx->stream));
        CF_HIP(hipEventRecord(e1, ctx->stream));
        hipLaunchKernelGGL(cf_ua_kernel<true>, dim3((unsigned)std::min<int64_t>(n2, cap)), dim3((unsigned)block), CF_UA_LDS_BYTES, ctx->stream,
                           (const cf_ua_pair*)d_p2, n2, (const uint8_t*)d_reads, (const uint8_t*)d_units, m, match, mismatch, gap, d_res, d_area, d_ops,
                           d_ticket, d_fault);
        CF_KERNEL_CHECK("cf_ua_kernel (moves pass)");
        CF_HIP(hipEventRecord(e2, ctx->stream));
        CF_HIP(hipEventSynchronize(e2));
        (void)hipEventElapsedTime(&t, e0, e1); shape.phase_ms[0] += t;
        (void)hipEventElapsedTime(&t, e1, e2); shape.phase_ms[2] += t;
        CF_HIP(hipEventRecord(e0, ctx->stream));
        int32_t h_fault = 0;
        CF_TRY(cf_copy_d2h(ctx, &h_fault, d_fault, 4));
        if (h_fault) return cf_fail(ctx, -5, "cf_ualign_run: a walk did not end inside its op string (internal error)");
        std::vector<int32_t> res((size_t)8 * n2);
        std::vector<uint8_t> h_ops((size_t)op_bytes);
        CF_TRY(cf_copy_d2h(ctx, res.data(), d_res, (size_t)8 * n2 * 4));
        CF_TRY(cf_copy_d2h(ctx, h_ops.data(), d_ops, (size_t)op_bytes));
        CF_HIP(hipEventRecord(e1, ctx->stream));
        CF_HIP(hipEventSynchronize(e1));
        (void)hipEventElapsedTime(&t, e0, e1); shape.phase_ms[0] += t;
        for (int64_t x = 0; x < n2; ++x) {
            const win& w = wins[first + (size_t)x];
            const int32_t* r = &res[(size_t)8 * x];
            if (r[3] < 0 || r[3] > w.cap) return cf_fail(ctx, -5, "cf_ualign_run: an op string longer than its room (internal error)");
            res_hits[(size_t)w.q] = cf_ualign_hit{CF_UALIGN_HIT, w.strand, w.score, r[0], w.i, r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
            const uint8_t* src = h_ops.data() + p2[(size_t)x].ops_off;
            rev_ops[first + (size_t)x].assign(std::reverse_iterator<const uint8_t*>(src + r[3]), std::reverse_iterator<const uint8_t*>(src));
        }
        ++shape.n_batches;
        first = last;
    }
    // the op strings in read order
    std::vector<size_t> slot_of((size_t)n_reads, (size_t)-1);
    for (size_t x = 0; x < wins.size(); ++x) slot_of[(size_t)wins[x].q] = x;
    for (int64_t q = 0; q < n_reads; ++q) {
        res_ptr[(size_t)q] = (int64_t)res_ops.size();
        if (slot_of[(size_t)q] != (size_t)-1) res_ops.insert(res_ops.end(), rev_ops[slot_of[(size_t)q]].begin(), rev_ops[slot_of[(size_t)q]].end());
    }
    res_ptr[(size_t)n_reads] = (int64_t)res_ops.size();
    shape.phase_ms[3] = shape.phase_ms[0] + shape.phase_ms[1] + shape.phase_ms[2];
    if (n_reads > 0) std::memcpy(hits, res_hits.data(), (size_t)n_reads * sizeof(cf_ualign_hit));
    if (ms_out) *ms_out = shape.phase_ms[3];
    ctx->ualign_hits.swap(res_hits);
    ctx->ualign_op_ptr.swap(res_ptr);
    ctx->ualign_op_bytes.swap(res_ops);
    ctx->ualign_last = shape;
    return 0;
}

}  // extern "C"
