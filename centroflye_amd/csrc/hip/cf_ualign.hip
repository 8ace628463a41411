// cf_ualign.hip — the built-in tandem aligner: every read against the unit read cyclically (local alignment with linear gaps on a
// cylinder), the best stretch per read with its alignment columns (gfx950, wave64).
//
// Stands in for the external NCRF binary of scripts/run_ncrf_parallel.py:49-62.  There is NO reference function behind it; the
// rule is written out at cf_ualign_run in include/cfhip.h and restated in tests/ualigncheck.py.
//
//   cf_ua_kernel<MOVES>   The frame is that of cf_rowdp.h (a workgroup per pair, 16 columns per thread, the read through LDS, the two
//                         passes, the packed moves, the walk by runs of diagonals); the columns are the unit's m bases.  A row is
//                         (1) the element-wise step A = max(0, diagonal, vertical): the diagonal input of a thread's first
//                         column is the final value of its left neighbour's last column, which the thread knows from its own carry
//                         of the row before (thread 0: the value of column m - 1, the wrap); (2) the cyclic max-plus scan: the
//                         serial scan, the wave scan, the wave totals through LDS [barrier 1], the value S'[m - 1] of the scan
//                         without the wrap through LDS [barrier 2], and S[j] = max(S'[j], S'[m - 1] - (j + 1) G): the row's end
//                         carry fed back to the front once.  Every carry is clamped at 0: all values of the matrix are >= 0, so a
//                         carry <= 0 changes no cell and no equality of the walk, and no sum of gap costs leaves int32 (the
//                         multiples of G are saturated on the way in).
//                         MOVES = false (score pass): a thread keeps its best cell (first row, then first column among equals); the
//                         block's best goes out as (score, i, j).
//                         MOVES = true (moves pass, rows 1 .. r_en): the moves are 0 stop, 1 rule a, 2 rule b, 3 rule c; a row of the
//                         area has RW = ceil(m / 16) words.  The walk goes back from the end cell: one op byte per alignment column
//                         (last column first; the host turns the string round) and the tallies.
//   The walk's cap is the pair's op capacity r_en + floor(r_en M / G) + 1 (a path of positive score has fewer than M matches / G gap
//   columns).  The only atomic is the ticket.
#include "cf_rowdp.h"

// LDS window behind the wave totals: S'[m - 1] [2], the threads' best cells [256][3], the read chunk
#define CF_UA_LDS_W 48
#define CF_UA_LDS_RED 64
#define CF_UA_LDS_READ (CF_UA_LDS_RED + CF_RD_BLOCK * 12)
#define CF_UA_LDS_BYTES (CF_UA_LDS_READ + CF_RD_CHUNK)

struct cf_ua_pair {
    int64_t r_begin;             // first byte of the read
    int64_t area_off;            // moves pass: first word of the pair's move area
    int64_t ops_off;             // moves pass: first byte of the pair's op string
    int32_t n_rows;              // rows to fill: the read's length (score pass), r_en (moves pass)
    int32_t strand;
    int32_t j_end;               // moves pass: the end cell's column
    int32_t ops_cap;             // moves pass: room of the op string
};

template <bool MOVES>
__global__ void __launch_bounds__(CF_RD_BLOCK)
cf_ua_kernel(const cf_ua_pair* __restrict__ pairs, int64_t n_pairs, const uint8_t* __restrict__ reads, const uint8_t* __restrict__ units, int32_t m,
             int32_t M, int32_t X, int32_t G, int32_t* __restrict__ out, uint32_t* __restrict__ area, uint8_t* __restrict__ ops,
             unsigned long long* __restrict__ ticket, int32_t* __restrict__ fault) {
    volatile int32_t* tot = (volatile int32_t*)(cf_lds + CF_RD_LDS_TOT);
    volatile int32_t* wv = (volatile int32_t*)(cf_lds + CF_UA_LDS_W);
    volatile int32_t* red = (volatile int32_t*)(cf_lds + CF_UA_LDS_RED);
    volatile uint8_t* lr = (volatile uint8_t*)(cf_lds + CF_UA_LDS_READ);
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int32_t j0 = tid * CF_RD_CPT;
    const int32_t RW = (m + CF_RD_CPT - 1) / CF_RD_CPT;
    const int32_t tl = (m - 1) / CF_RD_CPT, kl = (m - 1) % CF_RD_CPT;      // the thread and the register of column m - 1
    const int32_t nact = m - j0 < 0 ? 0 : (m - j0 > CF_RD_CPT ? CF_RD_CPT : m - j0);      // columns of this thread inside the unit
    // a carry is >= 0 and clamped at 0, so a saturated cost gives the same 0 as the true one
    int32_t gsh[6], gw[3];
#pragma unroll
    for (int s = 0; s < 6; ++s) gsh[s] = cf_rd_gap(G, CF_RD_CPT << s);
    const int32_t gfront = cf_rd_gap(G, j0 + 1);      // from column m - 1 round to this thread's first column
    const int32_t gleft = cf_rd_gap(G, j0);           // ... to its left neighbour's last column
#pragma unroll
    for (int w = 0; w < 3; ++w) gw[w] = cf_rd_gap(G, j0 > 1024 * (w + 1) ? j0 - 1024 * (w + 1) : 0);
    for (;;) {
        const int64_t idx = cf_rd_take(ticket, n_pairs);
        if (idx < 0) break;
        const cf_ua_pair pr = pairs[idx];
        const uint8_t* __restrict__ gu = units + (pr.strand ? m : 0);
        const uint8_t* __restrict__ gr = reads + pr.r_begin;
        uint32_t* __restrict__ mv_area = area + (MOVES ? pr.area_off : 0);
        const int32_t n_rows = pr.n_rows;
        uint32_t ub[CF_RD_CPT];      // 0xFF beyond the unit: no upper-cased byte equals it
        int32_t S[CF_RD_CPT];
#pragma unroll
        for (int k = 0; k < CF_RD_CPT; ++k) {
            ub[k] = k < nact ? (uint32_t)gu[j0 + k] : 0xFFu;
            S[k] = 0;
        }
        int32_t left = 0;                     // S[i - 1][p(j0)]
        int32_t bS = 0, bI = 0, bJ = 0;       // score pass: this thread's best cell
        for (int32_t i = 1; i <= n_rows; ++i) {
            const uint32_t rb = cf_rd_row_byte(lr, gr, i, n_rows, tid, nth);
            const int buf = i & 1;
            // (1) element-wise, and the serial scan of this thread's columns
            int32_t P[CF_RD_CPT];
            int32_t dprev = left, run = 0;
#pragma unroll
            for (int k = 0; k < CF_RD_CPT; ++k) {
                const int32_t d = dprev + (rb == ub[k] ? M : -X), v = S[k] - G;
                dprev = S[k];
                int32_t a = cf_rd_max(cf_rd_max(d, v), 0);
                a = k < nact ? a : 0;
                run = cf_rd_max(a, run - G);
                P[k] = run;
            }
            // (2) the thread totals across the wave: E = the scan's value at this thread's last column, from this wave's columns
            int32_t E = run;
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const int32_t o = __shfl_up(E, 1u << s);
                if (lane >= (1 << s)) E = cf_rd_max(E, o - gsh[s]);
            }
            int32_t cin = __shfl_up(E, 1u);      // ... at the column in front of this thread's first
            if (lane == 0) cin = 0;
            if (lane == 63) tot[buf * 4 + wave] = E;
            cf_barrier_lds();
#pragma unroll
            for (int w = 0; w < 3; ++w)
                if (w < wave) cin = cf_rd_max(cin, tot[buf * 4 + w] - gw[w]);
            // S' = the scan without the wrap
            int32_t c = cin;
#pragma unroll
            for (int k = 0; k < CF_RD_CPT; ++k) {
                c = cf_rd_max(c - G, 0);
                P[k] = cf_rd_max(P[k], c);
            }
            if (tid == tl) {
                int32_t x = 0;
#pragma unroll
                for (int k = 0; k < CF_RD_CPT; ++k) x = k == kl ? P[k] : x;
                wv[buf] = x;
            }
            cf_barrier_lds();
            const int32_t W = wv[buf];      // S'[m - 1] = S[i][m - 1]
            c = cf_rd_max(W - gfront, 0);
            uint32_t word = 0;
            int32_t rowmax = 0;
            dprev = left;
#pragma unroll
            for (int k = 0; k < CF_RD_CPT; ++k) {
                const int32_t s_new = cf_rd_max(P[k], c);
                c = cf_rd_max(c - G, 0);
                if (MOVES) {
                    const int32_t d = dprev + (rb == ub[k] ? M : -X), v = S[k] - G;
                    dprev = S[k];
                    word = cf_rd_pack(word, s_new == 0 ? 0u : (d == s_new ? 1u : (v == s_new ? 2u : 3u)), k);
                } else {
                    rowmax = cf_rd_max(rowmax, s_new);
                }
                S[k] = s_new;
            }
            left = tid == 0 ? W : cf_rd_max(cin, cf_rd_max(W - gleft, 0));
            if (MOVES) {
                if (tid < RW) cf_rd_row(mv_area, i, RW)[tid] = word;
            } else if (nact > 0 && rowmax > bS) {
#pragma unroll
                for (int k = 0; k < CF_RD_CPT; ++k)
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
                // The walk is a chain of dependent loads from HBM, and nearly every move is a diagonal, so a round takes a run of
                // them: lane l looks l diagonal steps back from (i, j).  Every value below is the same in all lanes.
                uint8_t* __restrict__ po = ops + pr.ops_off;
                int32_t i = n_rows, j = pr.j_end, n_ops = 0, u_st = 0, m_al = 0, cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
                bool stopped = false;
                for (int32_t round = 0; round <= pr.ops_cap; ++round) {      // a round takes at least one column or ends the walk
                    if (n_ops > pr.ops_cap) break;      // (the string has 64 bytes of room behind its capacity: a round writes inside it)
                    const int32_t il = i - lane;
                    int32_t jl = (j - lane) % m;
                    jl = jl < 0 ? jl + m : jl;
                    uint32_t mv = 0u;      // row 0 stops
                    if (il >= 1) mv = cf_rd_move(mv_area, il, RW, jl);
                    const int32_t run = cf_rd_diag_len(mv);
                    bool is_match = false;
                    if (lane < run) {
                        is_match = cf_rd_match(gr, il, gu, jl);
                        po[n_ops + lane] = is_match ? (uint8_t)0 : (uint8_t)1;
                    }
                    const int32_t n_match = cf_rd_count(is_match);
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

// what cf_rd_run (cf_rowdp.h) asks of the stage
struct cf_ua_stage {
    typedef cf_ua_pair pair;
    typedef uint8_t item;      // an op
    struct win { int64_t q; int32_t strand, score, rows, j; int64_t words, cap, room; };      // rows = r_en, (rows, j) the end cell; cap of the op string
    static constexpr const char *name = "ualign", *kernel = "cf_ua_kernel", *fault = "cf_ualign_run: a walk did not end inside its op string (internal error)";
    static constexpr int score_words = 3;
    const uint8_t* unit;
    int32_t m, M, X, G;
    std::vector<cf_ualign_hit> hits;
    uint8_t *d_units = nullptr, *d_ops = nullptr;
    int32_t* d_res = nullptr;
    std::vector<int32_t> res;
    std::vector<uint8_t> h_ops;

    int upload(cf_ctx* ctx, cf_scratch& tmp) {
        std::vector<uint8_t> h_units((size_t)2 * m);
        cf_rd_both_strands(unit, m, h_units.data(), h_units.data() + m);
        CF_TRY(tmp.get(&d_units, (size_t)2 * m + 16, "ualign unit"));
        return cf_copy_h2d(ctx, d_units, h_units.data(), (size_t)2 * m);
    }
    pair score_pair(int64_t r_begin, int32_t n, int s) const { return pair{r_begin, 0, 0, n, s, 0, 0}; }
    pair move_pair(const win& w, int64_t r_begin, int64_t area_off, int64_t ops_off) const { return pair{r_begin, area_off, ops_off, w.rows, w.strand, w.j, (int32_t)w.cap}; }
    template <bool MOVES> void launch(cf_ctx* ctx, unsigned grid, const pair* p, int64_t n, const cf_rd_dev& d) const {
        hipLaunchKernelGGL(cf_ua_kernel<MOVES>, dim3(grid), dim3((unsigned)cf_rd_block_for(m)), CF_UA_LDS_BYTES, ctx->stream, p, n, d.reads, (const uint8_t*)d_units,
                           m, M, X, G, MOVES ? d_res : d.score, d.area, d_ops, d.ticket, d.fault);      // (no area and no ops in the score pass)
    }
    // the winning strand of a read with a hit ("+" on a tie)
    int pick(cf_ctx* ctx, int64_t q, int32_t, const int32_t* f, std::vector<win>& wins) const {
        const int s = f[3] > f[0] ? 1 : 0;
        if (f[3 * s] <= 0) return 0;
        const int64_t i_end = f[3 * s + 1], cap = i_end + i_end * (int64_t)M / G + 1;
        if (cap >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_ualign_run: the op string of read " + std::to_string(q) + " could hold 2^31 columns or more");
        wins.push_back(win{q, s, f[3 * s], f[3 * s + 1], f[3 * s + 2], i_end * cf_rd_row_words(m), cap, cap + 64});      // (the walking wave writes a round of up to 64 columns before it looks at the room)
        return 0;
    }
    int batch_get(cf_scratch& tmp, int64_t n2, int64_t op_bytes) {
        CF_TRY(tmp.get(&d_ops, (size_t)op_bytes + 16, "ualign op strings"));
        return tmp.get(&d_res, (size_t)8 * n2, "ualign walk results");
    }
    int fetch(cf_ctx* ctx, const cf_rd_dev&, int64_t n2, int64_t op_bytes) {
        res.resize((size_t)8 * n2);
        h_ops.resize((size_t)op_bytes);
        CF_TRY(cf_copy_d2h(ctx, res.data(), d_res, (size_t)8 * n2 * 4));
        return cf_copy_d2h(ctx, h_ops.data(), d_ops, (size_t)op_bytes);
    }
    int unpack(cf_ctx* ctx, const win* wins, const pair* p2, int64_t n2, std::vector<uint8_t>* rev_ops) {
        for (int64_t x = 0; x < n2; ++x) {
            const win& w = wins[x];
            const int32_t* r = &res[(size_t)8 * x];
            if (r[3] < 0 || r[3] > w.cap) return cf_fail(ctx, -5, "cf_ualign_run: an op string longer than its room (internal error)");
            hits[(size_t)w.q] = cf_ualign_hit{CF_UALIGN_HIT, w.strand, w.score, r[0], w.rows, r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
            const uint8_t* src = h_ops.data() + p2[x].ops_off;
            rev_ops[x].assign(std::reverse_iterator<const uint8_t*>(src + r[3]), std::reverse_iterator<const uint8_t*>(src));
        }
        return 0;
    }
};

extern "C" {

int cf_ualign_info(cf_ctx* ctx, cf_ualign_shape* out) {
    if (!ctx || !out) return -22;
    *out = ctx->ualign_last;
    out->max_unit = CF_RD_MAX_COLS;
    out->cols_per_thread = CF_RD_CPT;
    out->block = CF_RD_BLOCK;
    out->row_chunk = CF_RD_CHUNK;
    out->launch_cap = cf_rd_launch_cap(ctx);
    out->batch_bytes = cf_rd_batch_bytes(ctx, ctx->ualign_batch_bytes);
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
    if (unit_len < 1 || unit_len > CF_RD_MAX_COLS)
        return cf_fail(ctx, -22, "cf_ualign_run: a unit of " + std::to_string(unit_len) + " bases (1 .. " + std::to_string(CF_RD_MAX_COLS) + " are taken)");
    if (!unit || !read_off || (n_reads > 0 && !hits)) return cf_fail(ctx, -22, "cf_ualign_run: null pointer");
    for (int32_t j = 0; j < unit_len; ++j)
        if (unit[j] != 'A' && unit[j] != 'C' && unit[j] != 'G' && unit[j] != 'T')
            return cf_fail(ctx, -22, "cf_ualign_run: unit byte " + std::to_string(j) + " is not upper-case A, C, G or T");
    if (match < 1 || mismatch < 1 || gap < 1) return cf_fail(ctx, -22, "cf_ualign_run: match, mismatch and gap must be at least 1");
    if (read_off[0] < 0) return cf_fail(ctx, -22, "cf_ualign_run: negative read offset");
    CF_TRY(cf_rd_check_reads(ctx, "cf_ualign_run", reads, read_off, n_reads, (((int64_t)1 << 31) + match - 1) / match, " could score 2^31 or more"));

    // the results of this call, handed to the context only when everything worked
    cf_ua_stage st{unit, unit_len, match, mismatch, gap, std::vector<cf_ualign_hit>((size_t)n_reads, cf_ualign_hit{})};
    std::vector<int64_t> res_ptr;
    std::vector<uint8_t> res_ops;
    cf_ualign_shape shape{};
    shape.n_reads = n_reads;
    CF_TRY(cf_rd_run(ctx, st, reads, read_off, n_reads, cf_rd_batch_bytes(ctx, ctx->ualign_batch_bytes), shape, res_ptr, res_ops));
    if (n_reads > 0) std::memcpy(hits, st.hits.data(), (size_t)n_reads * sizeof(cf_ualign_hit));
    if (ms_out) *ms_out = shape.phase_ms[3];
    ctx->ualign_hits.swap(st.hits);
    ctx->ualign_op_ptr.swap(res_ptr);
    ctx->ualign_op_bytes.swap(res_ops);
    ctx->ualign_last = shape;
    return 0;
}

}  // extern "C"
