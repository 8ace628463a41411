// cf_monodec.hip — the built-in monomer decomposer: every read cut into a chain of monomer instances by ONE dynamic program against
// all monomers at once (global alignment with linear gaps of the read against the best sequence of monomers), both strands
// (gfx950, wave64).
//
// Stands in for the String Decomposer report the reference's second pipeline starts from (scripts/sd_parser.py reads it).  There
// is NO reference function behind it and it is NOT String Decomposer: the rule is written out at cf_monodec_run in include/cfhip.h
// and restated in tests/monodeccheck.py.
//
//   cf_md_kernel<MOVES>   The frame is that of cf_rowdp.h (a workgroup per pair, 16 columns per thread, the read through LDS, the two
//                         passes, the packed moves, the walk by runs of diagonals); the monomers stand side by side as L = sum of
//                         their lengths columns.  A row is
//                         (1) the element-wise step A = max(diagonal, vertical): the diagonal input of a monomer's first column is
//                             the block-uniform E[i - 1], that of a thread's first column otherwise the final value of its left
//                             neighbour's last column, which the thread knows from its own carry of the row before;
//                         (2) the max-plus scan SEGMENTED at the monomer starts.  Where the starts lie does not depend on the row, so
//                             the flags of the usual segmented scan are worked out once per launch: a serial scan of the 16 columns
//                             that restarts at a start, a wave scan of the thread totals by lane shifts in which lane l takes the
//                             step of distance d only if no start lies in the threads l - d + 1 .. l (a bit per step, constant),
//                             the wave totals through LDS [barrier 1] taken by the same rule (a bit per wave in front), and the
//                             carry-in applied to the columns in front of the thread's first start;
//                         (3) E[i] = max(the largest V' of an end column, E[i - 1] - G): a wave reduction by lane exchanges, the
//                             wave maxima through LDS [barrier 2]; then V = max(V', E[i] - (j + 1) G), the fed-back term.
//                         No value is clamped: every value a cell takes lies in [-(n + L + 1) max(M, X, G), n M], which the host
//                         keeps inside int32; what a lane computes and then throws away (a carry across a monomer start) may wrap
//                         and is subtracted without signed overflow.
//                         MOVES = false (score pass): E[n] goes out.
//                         MOVES = true (moves pass): the moves are 1 rule a, 2 rule b, 3 rule c; a row of the area has RW + 1 words,
//                         RW = ceil(L / 16); word RW of the row holds the boundary's entry: the smallest end column whose V equals
//                         E[i], or -1 (the reduction of (3) carries the column next to the value).  The walk goes back from
//                         boundary n and writes one record per instance (last first; the host turns them round) to the pair's own
//                         room, then moves them to the batch's dense list.
//   The walk's cap is 2 n + floor(n M / G) + 4 rounds (the path scores at least -n G, so it has at most n + n M / G deleted columns
//   next to its at most n read bytes).  The only atomics are the ticket and, once per pair of the moves pass, the cursor of the
//   batch's dense list of records (ticket[1]).
#include "cf_rowdp.h"

// LDS window behind the wave totals: the wave flags [4], the end-column maxima [2][4] (8 bytes each), the read chunk
#define CF_MD_LDS_FLAG 48
#define CF_MD_LDS_END 64
#define CF_MD_LDS_READ 128
#define CF_MD_LDS_BYTES (CF_MD_LDS_READ + CF_RD_CHUNK)
#define CF_MD_NEG ((int32_t)0x80000000)

struct cf_md_pair {
    int64_t r_begin;             // first byte of the read
    int64_t area_off;            // moves pass: first word of the pair's move area
    int64_t rec_off;             // moves pass: first record of the pair
    int64_t round_cap;           // moves pass: rounds of the walk at most
    int32_t n_rows;              // the read's length
    int32_t strand;
};

template <bool MOVES>
__global__ void __launch_bounds__(CF_RD_BLOCK)
cf_md_kernel(const cf_md_pair* __restrict__ pairs, int64_t n_pairs, const uint8_t* __restrict__ reads, const uint8_t* __restrict__ monos,
             const int32_t* __restrict__ colj, const int32_t* __restrict__ colk, int32_t L, int32_t M, int32_t X, int32_t G,
             int32_t* __restrict__ out, uint32_t* __restrict__ area, int32_t* __restrict__ recs, int32_t* __restrict__ dense,
             unsigned long long* __restrict__ ticket, int32_t* __restrict__ fault) {
    volatile int32_t* tot = (volatile int32_t*)(cf_lds + CF_RD_LDS_TOT);
    volatile int32_t* wflag = (volatile int32_t*)(cf_lds + CF_MD_LDS_FLAG);
    volatile int64_t* wend = (volatile int64_t*)(cf_lds + CF_MD_LDS_END);
    volatile int32_t* wend32 = (volatile int32_t*)(cf_lds + CF_MD_LDS_END);      // the score pass's maxima carry no column
    volatile uint8_t* lr = (volatile uint8_t*)(cf_lds + CF_MD_LDS_READ);
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, wave = tid >> 6, n_waves = nth >> 6;
    const int32_t j0 = tid * CF_RD_CPT;
    const int32_t RW = (L + CF_RD_CPT - 1) / CF_RD_CPT, RW1 = RW + 1;
    // where the monomers start and end among this thread's columns (a column beyond L is a monomer of its own that ends nowhere)
    uint32_t stmask = 0, endmask = 0;
#pragma unroll
    for (int k = 0; k < CF_RD_CPT; ++k) {
        const int32_t c = j0 + k;
        if (c >= L || colj[c] == 0) stmask |= 1u << k;
        if (c < L && (c == L - 1 || colj[c + 1] == 0)) endmask |= 1u << k;
    }
    const int32_t fs = stmask ? (int32_t)__ffs((int)stmask) - 1 : CF_RD_CPT;      // the columns in front of it take the carry-in
    const int32_t jfirst = j0 < L ? colj[j0] : 0;                                  // the first column's index in its monomer
    const int32_t jleft = (tid > 0 && j0 - 1 < L) ? colj[j0 - 1] : 0;              // ... and that of the left neighbour's last column
    const int32_t gfirst = cf_rd_gap(G, jfirst), gleft = cf_rd_gap(G, jleft + 1);
    int32_t gsh[6], gw[3];
#pragma unroll
    for (int s = 0; s < 6; ++s) gsh[s] = cf_rd_gap(G, CF_RD_CPT << s);
#pragma unroll
    for (int w = 0; w < 3; ++w) gw[w] = cf_rd_gap(G, j0 > 1024 * (w + 1) ? j0 - 1024 * (w + 1) : 0);
    // the flags of the segmented scan, once: bit s of `use` = this lane takes the wave scan's step s; bit w of `wuse` = the carry-in
    // takes the total of wave w
    uint32_t use = 0, wuse = 0;
    {
        int F = stmask != 0u;
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const int oF = __shfl_up(F, 1u << s);
            if (lane >= (1 << s)) {
                if (!F) use |= 1u << s;
                F |= oF;
            }
        }
        int cF = __shfl_up(F, 1u);      // a start in this wave's columns in front of this thread
        if (lane == 0) cF = 0;
        if (lane == 63) wflag[wave] = F;
        __syncthreads();
        for (int w = wave - 1; w >= 0; --w) {
            if (!cF) wuse |= 1u << w;
            cF |= wflag[w];
        }
    }
    for (;;) {
        const int64_t idx = cf_rd_take(ticket, n_pairs);
        if (idx < 0) break;
        const cf_md_pair pr = pairs[idx];
        const uint8_t* __restrict__ gu = monos + (pr.strand ? L : 0);
        const uint8_t* __restrict__ gr = reads + pr.r_begin;
        uint32_t* __restrict__ mv_area = area + (MOVES ? pr.area_off : 0);
        const int32_t n_rows = pr.n_rows;
        uint32_t ub[CF_RD_CPT];      // 0xFF beyond L: no upper-cased byte equals it
        int32_t S[CF_RD_CPT];
#pragma unroll
        for (int k = 0; k < CF_RD_CPT; ++k) {
            const int32_t c = j0 + k;
            ub[k] = c < L ? (uint32_t)gu[c] : 0xFFu;
            S[k] = c < L ? -G * (colj[c] + 1) : -G;      // V[0][k][j] = -(j + 1) G
        }
        int32_t left = -gleft;                // V[i - 1] of the column in front of this thread's first
        int32_t Eprev = 0;                    // E[i - 1]
        for (int32_t i = 1; i <= n_rows; ++i) {
            const uint32_t rb = cf_rd_row_byte(lr, gr, i, n_rows, tid, nth);
            const int buf = i & 1;
            // (1) element-wise, and the serial scan of this thread's columns
            int32_t P[CF_RD_CPT];
            int32_t dprev = left, run = 0;
#pragma unroll
            for (int k = 0; k < CF_RD_CPT; ++k) {
                const bool st = (stmask >> k) & 1u;
                const int32_t d = (st ? Eprev : dprev) + (rb == ub[k] ? M : -X), v = S[k] - G;
                dprev = S[k];
                const int32_t a = cf_rd_max(d, v);
                run = (k == 0 || st) ? a : cf_rd_max(a, run - G);
                P[k] = run;
            }
            // (2) the thread totals across the wave: T = the scan's value at this thread's last column, from this wave's columns
            int32_t T = run;
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const int32_t o = __shfl_up(T, 1u << s);
                if ((use >> s) & 1u) T = cf_rd_max(T, cf_rd_sub(o, gsh[s]));
            }
            int32_t cin = __shfl_up(T, 1u);      // ... at the column in front of this thread's first
            if (lane == 0) cin = CF_MD_NEG;
            if (lane == 63) tot[buf * 4 + wave] = T;
            cf_barrier_lds();
#pragma unroll
            for (int w = 2; w >= 0; --w)
                if ((wuse >> w) & 1u) cin = cf_rd_max(cin, cf_rd_sub(tot[buf * 4 + w], gw[w]));
            int32_t c = cin;
#pragma unroll
            for (int k = 0; k < CF_RD_CPT; ++k) {
                c = cf_rd_sub(c, G);
                if (k < fs) P[k] = cf_rd_max(P[k], c);      // P = V'
            }
            // (3) E[i] from the end columns
            int32_t Ei, kstar = -1;
            if (MOVES) {
                // the value above the column, the column counted down: the largest key is the largest value at the smallest column
                int32_t ev = CF_MD_NEG, ec = 0;      // this thread's largest end-column value, at its smallest column
#pragma unroll
                for (int k = CF_RD_CPT - 1; k >= 0; --k)
                    if (((endmask >> k) & 1u) && P[k] >= ev) { ev = P[k]; ec = j0 + k; }
                int64_t em = endmask ? (int64_t)ev * 4294967296ll + (int64_t)(0x7fffffff - ec) : INT64_MIN;
#pragma unroll
                for (int s = 0; s < 6; ++s) {
                    const int64_t o = __shfl_xor(em, 1 << s);
                    em = o > em ? o : em;
                }
                if (lane == 0) wend[buf * 4 + wave] = em;
                cf_barrier_lds();
                int64_t best = wend[buf * 4];
                for (int w = 1; w < n_waves; ++w) {
                    const int64_t o = wend[buf * 4 + w];
                    best = o > best ? o : best;
                }
                const int32_t hi = (int32_t)(best >> 32);
                Ei = cf_rd_max(hi, Eprev - G);
                if (hi == Ei) kstar = 0x7fffffff - (int32_t)(uint32_t)(best & 0xffffffffll);
            } else {
                int32_t em = CF_MD_NEG;
#pragma unroll
                for (int k = 0; k < CF_RD_CPT; ++k)
                    if ((endmask >> k) & 1u) em = cf_rd_max(em, P[k]);
#pragma unroll
                for (int s = 0; s < 6; ++s) em = cf_rd_max(em, __shfl_xor(em, 1 << s));
                if (lane == 0) wend32[buf * 4 + wave] = em;
                cf_barrier_lds();
                Ei = Eprev - G;
                for (int w = 0; w < n_waves; ++w) Ei = cf_rd_max(Ei, wend32[buf * 4 + w]);
            }
            // V = max(V', E[i] - (j + 1) G), and the moves
            int32_t fb = Ei - gfirst;
            uint32_t word = 0;
            dprev = left;
#pragma unroll
            for (int k = 0; k < CF_RD_CPT; ++k) {
                const bool st = (stmask >> k) & 1u;
                fb = st ? Ei - G : fb - G;
                const int32_t s_new = cf_rd_max(P[k], fb);
                if (MOVES) {
                    const int32_t d = (st ? Eprev : dprev) + (rb == ub[k] ? M : -X), v = S[k] - G;
                    dprev = S[k];
                    word = cf_rd_pack(word, d == s_new ? 1u : (v == s_new ? 2u : 3u), k);
                }
                S[k] = s_new;
            }
            left = cf_rd_max(cin, Ei - gleft);
            Eprev = Ei;
            if (MOVES) {
                if (tid < RW) cf_rd_row(mv_area, i, RW1)[tid] = word;
                if (tid == 0) cf_rd_row(mv_area, i, RW1)[RW] = (uint32_t)kstar;
            }
        }
        if (!MOVES) {
            if (tid == 0) out[idx] = Eprev;
        } else {
            __syncthreads();      // every move word of the pair is visible to the walking wave
            if (wave == 0) {
                // Nearly every move is a diagonal, so a round takes a run of them: lane l looks l diagonal steps back from (i, j)
                // inside the instance.  Every value below is the same in all lanes.
                int32_t* pr_rec = recs + 7 * pr.rec_off;
                int32_t i = n_rows, j = 0, c = 0, k_in = 0, i_in = 0, n_inst = 0, prefix = 0, cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
                bool inside = false, done = false;
                for (int64_t round = 0; round <= pr.round_cap; ++round) {      // a round takes at least one column or ends the walk
                    if (!inside) {
                        if (i == 0) { done = true; break; }
                        const int32_t ks = (int32_t)cf_rd_row(mv_area, i, RW1)[RW];
                        if (ks < 0) { prefix = i; done = true; break; }      // unassigned bases are a prefix of the read
                        if (ks >= L || n_inst >= n_rows) break;
                        c = ks; j = colj[ks]; k_in = colk[ks]; i_in = i; inside = true;
                        cnt0 = cnt1 = cnt2 = cnt3 = 0;
                    }
                    const int32_t il = i - lane, jl = j - lane, cl = c - lane;
                    uint32_t mv = 0u;
                    if (il >= 1 && jl >= 0) mv = cf_rd_move(mv_area, il, RW1, cl);
                    const int32_t run = cf_rd_diag_len(mv);
                    bool is_match = false;
                    if (lane < run) is_match = cf_rd_match(gr, il, gu, cl);
                    const int32_t n_match = cf_rd_count(is_match);
                    const uint32_t end = (uint32_t)__shfl((int)mv, run & 63);      // the move of the cell the run stopped at
                    cnt0 += n_match; cnt1 += run - n_match; i -= run; j -= run; c -= run;
                    bool emit = false;
                    if (j < 0) emit = true;                           // the diagonal out of the monomer's first column
                    else if (run == 64) continue;
                    else if (i == 0) { cnt3 += j + 1; emit = true; }  // row 0: the rest of the monomer is deleted
                    else if (end == 2u) { ++cnt2; --i; }
                    else if (end == 3u) { ++cnt3; --j; --c; emit = j < 0; }
                    else break;
                    if (emit) {
                        if (lane == 0) {
                            int32_t* o = pr_rec + 7 * (int64_t)n_inst;
                            o[0] = k_in; o[1] = i; o[2] = i_in - 1; o[3] = cnt0; o[4] = cnt1; o[5] = cnt2; o[6] = cnt3;
                        }
                        ++n_inst;
                        inside = false;
                    }
                }
                if (lane == 0) {
                    if (!done) *fault = 1;
                    // the pair's records move to the batch's dense list (a pair has room for one record per read byte and uses
                    // a hundredth of it: only the dense list is copied to the host)
                    const unsigned long long base = atomicAdd(ticket + 1, (unsigned long long)n_inst);
                    int32_t* __restrict__ dst = dense + 7 * (int64_t)base;
                    for (int64_t x = 0; x < 7 * (int64_t)n_inst; ++x) dst[x] = pr_rec[x];
                    out[4 * idx] = n_inst; out[4 * idx + 1] = prefix;
                    out[4 * idx + 2] = (int32_t)(base & 0xffffffffull); out[4 * idx + 3] = (int32_t)(base >> 32);
                }
            }
        }
        __syncthreads();      // the ticket and the LDS slots are read no more before they are written again
    }
}

// what cf_rd_run (cf_rowdp.h) asks of the stage
struct cf_md_stage {
    typedef cf_md_pair pair;
    typedef cf_monodec_inst item;
    struct win { int64_t q; int32_t strand, score, rows; int64_t words, rounds, room; };      // room: records, one per read byte (an instance takes at least one)
    static constexpr const char *name = "monodec", *kernel = "cf_md_kernel", *fault = "cf_monodec_run: a walk did not end inside its bounds (internal error)";
    static constexpr int score_words = 1;
    const uint8_t* mono;
    const int64_t* mono_off;
    int32_t n_monomers, L, M, X, G;
    std::vector<cf_monodec_read> info;
    uint8_t* d_monos = nullptr;
    int32_t *d_colj = nullptr, *d_colk = nullptr, *d_recs = nullptr, *d_dense = nullptr, *d_res = nullptr;
    unsigned long long n_dense = 0;
    std::vector<int32_t> res, recs;

    // both strands of the monomers, every monomer turned round in its own place; the column tables
    int upload(cf_ctx* ctx, cf_scratch& tmp) {
        std::vector<uint8_t> h_monos((size_t)2 * L);
        std::vector<int32_t> h_colj((size_t)L), h_colk((size_t)L);
        for (int32_t k = 0; k < n_monomers; ++k) {
            const int32_t b = (int32_t)(mono_off[k] - mono_off[0]), len = (int32_t)(mono_off[k + 1] - mono_off[k]);
            cf_rd_both_strands(mono + b, len, &h_monos[(size_t)b], &h_monos[(size_t)L + b]);
            for (int32_t j = 0; j < len; ++j) {
                h_colj[(size_t)b + j] = j;
                h_colk[(size_t)b + j] = k;
            }
        }
        CF_TRY(tmp.get(&d_monos, (size_t)2 * L + 16, "monodec monomers"));
        CF_TRY(tmp.get(&d_colj, (size_t)L + 1, "monodec column table"));
        CF_TRY(tmp.get(&d_colk, (size_t)L + 1, "monodec monomer table"));
        CF_TRY(cf_copy_h2d(ctx, d_monos, h_monos.data(), (size_t)2 * L));
        CF_TRY(cf_copy_h2d(ctx, d_colj, h_colj.data(), (size_t)L * 4));
        return cf_copy_h2d(ctx, d_colk, h_colk.data(), (size_t)L * 4);
    }
    pair score_pair(int64_t r_begin, int32_t n, int s) const { return pair{r_begin, 0, 0, 0, n, s}; }
    pair move_pair(const win& w, int64_t r_begin, int64_t area_off, int64_t rec_off) const { return pair{r_begin, area_off, rec_off, w.rounds, w.rows, w.strand}; }
    template <bool MOVES> void launch(cf_ctx* ctx, unsigned grid, const pair* p, int64_t n, const cf_rd_dev& d) const {
        hipLaunchKernelGGL(cf_md_kernel<MOVES>, dim3(grid), dim3((unsigned)cf_rd_block_for(L)), CF_MD_LDS_BYTES, ctx->stream, p, n, d.reads, (const uint8_t*)d_monos,
                           (const int32_t*)d_colj, (const int32_t*)d_colk, L, M, X, G, MOVES ? d_res : d.score, d.area, d_recs, d_dense, d.ticket, d.fault);      // (no area and no records in the score pass)
    }
    // the winning strand of every read ("+" on a tie)
    int pick(cf_ctx*, int64_t q, int32_t n, const int32_t* f, std::vector<win>& wins) const {
        const int s = f[1] > f[0] ? 1 : 0;
        wins.push_back(win{q, s, f[s], n, (int64_t)n * (cf_rd_row_words(L) + 1), 2 * (int64_t)n + (int64_t)n * M / G + 4, n});
        return 0;
    }
    int batch_get(cf_scratch& tmp, int64_t n2, int64_t n_rec) {
        CF_TRY(tmp.get(&d_recs, (size_t)7 * n_rec + 8, "monodec instances"));
        CF_TRY(tmp.get(&d_dense, (size_t)7 * n_rec + 8, "monodec dense instances"));
        return tmp.get(&d_res, (size_t)4 * n2, "monodec walk results");
    }
    int fetch(cf_ctx* ctx, const cf_rd_dev& d, int64_t n2, int64_t n_rec) {
        CF_TRY(cf_copy_d2h(ctx, &n_dense, d.ticket + 1, 8));
        if (n_dense > (unsigned long long)n_rec) return cf_fail(ctx, -5, "cf_monodec_run: more instances than read bytes (internal error)");
        res.resize((size_t)4 * n2);
        recs.resize((size_t)7 * n_dense + 8);
        CF_TRY(cf_copy_d2h(ctx, res.data(), d_res, (size_t)4 * n2 * 4));
        return n_dense > 0 ? cf_copy_d2h(ctx, recs.data(), d_dense, (size_t)7 * n_dense * 4) : 0;
    }
    int unpack(cf_ctx* ctx, const win* wins, const pair*, int64_t n2, std::vector<cf_monodec_inst>* per_read) {
        for (int64_t x = 0; x < n2; ++x) {
            const win& w = wins[x];
            const int32_t n_inst = res[(size_t)4 * x], prefix = res[(size_t)4 * x + 1];
            const int64_t base = (int64_t)(uint32_t)res[(size_t)4 * x + 2] | ((int64_t)res[(size_t)4 * x + 3] << 32);
            if (n_inst < 0 || n_inst > w.rows || base < 0 || base + n_inst > (int64_t)n_dense)
                return cf_fail(ctx, -5, "cf_monodec_run: a pair's instances lie outside the batch's list (internal error)");
            info[(size_t)w.q] = cf_monodec_read{CF_MONODEC_DONE, w.strand, w.score, n_inst, prefix};
            per_read[x].resize((size_t)n_inst);
            for (int32_t a = 0; a < n_inst; ++a) {      // the walk wrote the last instance first
                const int32_t* r = &recs[(size_t)7 * (base + (n_inst - 1 - a))];
                per_read[x][(size_t)a] = cf_monodec_inst{r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
            }
        }
        return 0;
    }
};

extern "C" {

int cf_monodec_info(cf_ctx* ctx, cf_monodec_shape* out) {
    if (!ctx || !out) return -22;
    *out = ctx->monodec_last;
    out->max_cols = CF_RD_MAX_COLS;
    out->cols_per_thread = CF_RD_CPT;
    out->block = CF_RD_BLOCK;
    out->row_chunk = CF_RD_CHUNK;
    out->launch_cap = cf_rd_launch_cap(ctx);
    out->batch_bytes = cf_rd_batch_bytes(ctx, ctx->monodec_batch_bytes);
    return 0;
}

int cf_monodec_get(cf_ctx* ctx, int64_t* ptr, cf_monodec_inst* inst, int64_t cap, int64_t* n_out) {
    if (!ctx) return -22;
    if (ctx->monodec_ptr.empty()) return cf_fail(ctx, -22, "cf_monodec_get: no cf_monodec_run before");
    const int64_t n = (int64_t)ctx->monodec_inst.size();
    if (n_out) *n_out = n;
    if (!ptr && !inst) return 0;
    if (cap < n) return cf_fail(ctx, -22, "cf_monodec_get: room for " + std::to_string(cap) + " instances, " + std::to_string(n) + " needed");
    if (ptr) std::memcpy(ptr, ctx->monodec_ptr.data(), ctx->monodec_ptr.size() * 8);
    if (inst && n) std::memcpy(inst, ctx->monodec_inst.data(), (size_t)n * sizeof(cf_monodec_inst));
    return 0;
}

int cf_monodec_run(cf_ctx* ctx, const uint8_t* monomers, const int64_t* mono_off, int32_t n_monomers, const uint8_t* reads,
                   const int64_t* read_off, int64_t n_reads, int32_t match, int32_t mismatch, int32_t gap, cf_monodec_read* info, float* ms_out) {
    if (!ctx) return -22;
    if (ms_out) *ms_out = 0.f;
    if (n_reads < 0 || n_reads >= (int64_t)1 << 30) return cf_fail(ctx, -22, "cf_monodec_run: the number of reads is outside 0 .. 2^30 - 1");
    if (n_monomers < 1) return cf_fail(ctx, -22, "cf_monodec_run: no monomer");
    if (n_monomers > CF_RD_MAX_COLS)
        return cf_fail(ctx, -22, "cf_monodec_run: " + std::to_string(n_monomers) + " monomers have more than " + std::to_string(CF_RD_MAX_COLS) + " bases");
    if (!monomers || !mono_off || !read_off || (n_reads > 0 && !info)) return cf_fail(ctx, -22, "cf_monodec_run: null pointer");
    if (mono_off[0] < 0) return cf_fail(ctx, -22, "cf_monodec_run: negative monomer offset");
    for (int32_t k = 0; k < n_monomers; ++k) {
        if (mono_off[k + 1] <= mono_off[k]) return cf_fail(ctx, -22, "cf_monodec_run: monomer " + std::to_string(k) + " is empty (or its offsets decrease)");
        if (mono_off[k + 1] - mono_off[0] > CF_RD_MAX_COLS)
            return cf_fail(ctx, -22, "cf_monodec_run: the monomers have more than " + std::to_string(CF_RD_MAX_COLS) + " bases in all");
    }
    const int32_t L = (int32_t)(mono_off[n_monomers] - mono_off[0]);
    const uint8_t* mono = monomers + mono_off[0];
    for (int32_t c = 0; c < L; ++c)
        if (mono[c] != 'A' && mono[c] != 'C' && mono[c] != 'G' && mono[c] != 'T')
            return cf_fail(ctx, -22, "cf_monodec_run: monomer byte " + std::to_string(c) + " is not upper-case A, C, G or T");
    if (match < 1 || mismatch < 1 || gap < 1) return cf_fail(ctx, -22, "cf_monodec_run: match, mismatch and gap must be at least 1");
    const int64_t worst = std::max<int64_t>(match, std::max<int64_t>(mismatch, gap));
    if (read_off[0] < 0) return cf_fail(ctx, -22, "cf_monodec_run: negative read offset");
    if ((int64_t)(L + 1) * worst >= (int64_t)1 << 31) return cf_fail(ctx, -22, "cf_monodec_run: (L + 1) max(M, X, G) is 2^31 or more");
    // (n + L + 1) worst < 2^31 holds up to n = ceil(2^31 / worst) - L - 2
    CF_TRY(cf_rd_check_reads(ctx, "cf_monodec_run", reads, read_off, n_reads, (((int64_t)1 << 31) + worst - 1) / worst - L - 1, ": (n + L + 1) max(M, X, G) is 2^31 or more"));

    // the results of this call, handed to the context only when everything worked
    cf_md_stage st{mono, mono_off, n_monomers, L, match, mismatch, gap, std::vector<cf_monodec_read>((size_t)n_reads, cf_monodec_read{})};
    std::vector<int64_t> res_ptr;
    std::vector<cf_monodec_inst> res_inst;
    cf_monodec_shape shape{};
    shape.n_reads = n_reads;
    shape.n_monomers = n_monomers;
    shape.n_cols = L;
    CF_TRY(cf_rd_run(ctx, st, reads, read_off, n_reads, cf_rd_batch_bytes(ctx, ctx->monodec_batch_bytes), shape, res_ptr, res_inst));
    if (n_reads > 0) std::memcpy(info, st.info.data(), (size_t)n_reads * sizeof(cf_monodec_read));
    if (ms_out) *ms_out = shape.phase_ms[3];
    ctx->monodec_reads.swap(st.info);
    ctx->monodec_ptr.swap(res_ptr);
    ctx->monodec_inst.swap(res_inst);
    ctx->monodec_last = shape;
    return 0;
}

}  // extern "C"
