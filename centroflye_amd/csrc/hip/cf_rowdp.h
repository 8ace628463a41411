// cf_rowdp.h — what the tandem aligner (cf_ualign.hip) and the monomer decomposer (cf_monodec.hip) share: a dynamic program of a
// read (rows) against up to 4 096 target columns, filled row by row by one workgroup, in two passes (gfx950, wave64).
//
//   The kernels   ONE WORKGROUP PER PAIR (read, strand), pairs taken by a ticket in descending number of rows.  Thread t holds the
//                 columns 16 t .. 16 t + 15 of the current row in registers (256 threads x 16 = 4 096 columns; a launch takes the
//                 multiple of 64 threads that holds the target), the read goes through LDS in chunks of 1 024 bytes.  A row is an
//                 element-wise step, then a max-plus scan along the row: a serial scan of the thread's 16 columns, a wave scan of
//                 the thread totals by lane shifts (6 steps, 16 d G per step), the wave totals through LDS, and a value of the whole
//                 row fed back through LDS: two LDS-only barriers per row, the LDS slots double-buffered by the row's parity.  The
//                 recurrence and the scan's rule are the stage's own and stand in its file.
//                 MOVES = false (score pass): nothing is stored per cell; the pair's result goes out.
//                 MOVES = true (moves pass, the winning strand): a thread packs the 2-bit moves of its 16 cells into one word; the
//                 row's words are one coalesced store to the pair's area, row i - 1 at word (i - 1) x the stage's row stride.  Wave 0
//                 then walks back from the end: lane l looks at the cell l diagonal steps back, the leading run of diagonal moves
//                 (move 1) is taken in one round (64 columns per round trip to memory), then the one move that ended it.
//   Every loop is bounded by the rows of the pair, the block, or a cap on the walk's rounds that the host works out.
//   The host      cf_rd_run: the score pass over both strands of every read, the stage's choice of winners, the moves pass over the
//                 winners in batches of at most batch_bytes of move areas, the results put back in read order.
#pragma once
#include "cf_common.h"

#define CF_RD_CPT 16                   // columns of a row per thread
#define CF_RD_BLOCK 256
#define CF_RD_MAX_COLS (CF_RD_BLOCK * CF_RD_CPT)
#define CF_RD_WGS_PER_CU 8
#define CF_RD_CHUNK 1024               // read bytes staged in LDS at a time
// LDS window of both kernels: the ticket at byte 0, the wave totals [2][4] at byte 16; from byte 48 on the stage's own slots
#define CF_RD_LDS_TOT 16

#ifndef cf_barrier_lds
// workgroup barrier that orders LDS traffic only: the stores of the move words need not have landed before the next row
__device__ __forceinline__ void cf_barrier_lds() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
#endif

__device__ __forceinline__ int32_t cf_rd_sat(int64_t x) { return x < (int64_t)0x7fffffff ? (int32_t)x : 0x7fffffff; }
__device__ __forceinline__ int32_t cf_rd_max(int32_t a, int32_t b) { return a > b ? a : b; }
// a - b modulo 2^32: the result is used only where the true difference fits
__device__ __forceinline__ int32_t cf_rd_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

// the next pair, the same in every thread, or -1 when none is left (the barrier also closes the pair before)
__device__ __forceinline__ int64_t cf_rd_take(unsigned long long* ticket, int64_t n_pairs) {
    volatile int64_t* head = (volatile int64_t*)cf_lds;
    if (threadIdx.x == 0) {
        const unsigned long long x = atomicAdd(ticket, 1ull);
        head[0] = x < (unsigned long long)n_pairs ? (int64_t)x : -1;
    }
    __syncthreads();
    return head[0];
}

// byte i - 1 of the read with bit 5 cleared (a, c, g, t meet A, C, G, T; no other byte does), through the chunk lr in LDS
__device__ __forceinline__ uint32_t cf_rd_row_byte(volatile uint8_t* lr, const uint8_t* gr, int32_t i, int32_t n_rows, int tid, int nth) {
    if (((i - 1) & (CF_RD_CHUNK - 1)) == 0) {
        // (every thread read its byte of the chunk before in front of barrier 1 of the row before)
        for (int32_t x = tid; x < CF_RD_CHUNK && i - 1 + x < n_rows; x += nth) lr[x] = gr[i - 1 + x];
        __syncthreads();
    }
    return (uint32_t)lr[(i - 1) & (CF_RD_CHUNK - 1)] & 0xDFu;
}

// the cost of a gap of n columns, saturated.  Both kernels keep gsh[s] = that of the wave scan's step s (16 x 2^s columns) and
// gw[w] = from the last column of wave w to the column in front of the thread's first (filled in the kernel: tables handed to a
// function by reference come out as different code)
__device__ __forceinline__ int32_t cf_rd_gap(int32_t G, int32_t n) { return cf_rd_sat((int64_t)G * n); }

// The move areas: row i (1 ..) of an area begins at word (i - 1) x stride; a thread's word holds the 2-bit moves of its 16 columns,
// column k at bits 2 k, so the words of a row are one coalesced store and the move of cell (i, c) comes back from word c / 16
// (cf_rd_move spells the address out: through cf_rd_row the compiler allocates the registers of the row loop differently)
__device__ __forceinline__ uint32_t* cf_rd_row(uint32_t* area, int32_t i, int32_t stride) { return area + (int64_t)(i - 1) * stride; }
__device__ __forceinline__ uint32_t cf_rd_pack(uint32_t word, uint32_t mv, int k) { return word | mv << (2 * k); }
__device__ __forceinline__ uint32_t cf_rd_move(const uint32_t* area, int32_t i, int32_t stride, int32_t c) {
    return (area[(int64_t)(i - 1) * stride + (c >> 4)] >> (2 * (c & 15))) & 3u;
}

// The walk's round, lane l at the cell l diagonal steps back: the lanes in front of the first whose move mv is no diagonal; whether
// the read byte of row il equals the target's base of column cl; how many lanes say yes
__device__ __forceinline__ int32_t cf_rd_diag_len(uint32_t mv) {
    const unsigned long long diag = __ballot(mv == 1u);
    return diag == ~0ull ? 64 : (int32_t)__builtin_ctzll(~diag);
}
__device__ __forceinline__ bool cf_rd_match(const uint8_t* gr, int32_t il, const uint8_t* gu, int32_t cl) { return ((uint32_t)gr[il - 1] & 0xDFu) == (uint32_t)gu[cl]; }
__device__ __forceinline__ int32_t cf_rd_count(bool yes) { return (int32_t)__popcll(__ballot(yes)); }

// ---------------------------------------------------------------- host side
// move areas per batch unless the stage's knob says otherwise: an eighth of the device's memory, 2^28 .. 2^34 bytes (a launch should
// have a workgroup for every CU: a pair of 20 000 rows x 3 065 columns takes 15 MB)
static int64_t cf_rd_batch_bytes(const cf_ctx* ctx, int64_t knob) {
    if (knob > 0) return knob;
    return std::min<int64_t>(std::max<int64_t>(ctx->hbm_total / 8, (int64_t)1 << 28), (int64_t)1 << 34);
}
static int cf_rd_launch_cap(const cf_ctx* ctx) { return std::max(1, ctx->n_cu) * CF_RD_WGS_PER_CU; }
static int32_t cf_rd_row_words(int32_t cols) { return (cols + CF_RD_CPT - 1) / CF_RD_CPT; }
static int cf_rd_block_for(int32_t cols) { return std::min(CF_RD_BLOCK, ((cf_rd_row_words(cols) + 63) / 64) * 64); }

// a target of len upper-case bases laid out as [+ | -]: fwd takes it as it is, rev its reverse complement
static void cf_rd_both_strands(const uint8_t* seq, int32_t len, uint8_t* fwd, uint8_t* rev) {
    for (int32_t j = 0; j < len; ++j) {
        const uint8_t b = seq[len - 1 - j];
        fwd[j] = seq[j];
        rev[j] = b == 'A' ? 'T' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'A';
    }
}

// the checks of the reads behind read_off[0] >= 0: offsets that do not decrease, no read of `limit` bytes or more (why: how the
// stage's message about such a read ends), bytes where there are any
static int cf_rd_check_reads(cf_ctx* ctx, const std::string& who, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int64_t limit, const char* why) {
    for (int64_t q = 0; q < n_reads; ++q) {
        const int64_t n = read_off[q + 1] - read_off[q];
        if (n < 0) return cf_fail(ctx, -22, who + ": offsets of read " + std::to_string(q) + " decrease");
        if (n >= limit) return cf_fail(ctx, -22, who + ": read " + std::to_string(q) + " of " + std::to_string(n) + " bytes" + why);
    }
    if (read_off[n_reads] > read_off[0] && !reads) return cf_fail(ctx, -22, who + ": null bytes");
    return 0;
}

// the device buffers of cf_rd_run that a stage's launches and read-backs see.  ticket[0] hands out the pairs; ticket[1] is zeroed
// with it before every launch and is the stage's to use
struct cf_rd_dev {
    const uint8_t* reads;
    int32_t* score;              // the score pass's output, Stage::score_words per pair
    uint32_t* area;              // the batch's move areas
    unsigned long long* ticket;
    int32_t* fault;
};

// The two passes.  phase_ms: [0] set-up and copies, [1] the score pass, [2] the moves pass, [3] their sum.  A stage is a plain struct:
//   pair, win, item         the kernel's pair record; a winner (q, rows, words = its area's words, room = its share of the batch's
//                           output, and what else the stage needs); an element of a read's result
//   name, kernel, fault     for messages: "ualign", "cf_ua_kernel", what to say when a walk set the fault flag
//   score_words             32-bit words the score pass writes per pair
//   upload(tmp)             the target to the device
//   score_pair(..), move_pair(w, ..)   the pair records of the two passes
//   launch<MOVES>(grid, pairs, n, dev)   one pass's kernel on the context's stream
//   pick(q, n, f, wins)     read q of n bytes, f = the score words of its two strands: appends its winner, if it has one
//   batch_get(tmp, n2, room), fetch(dev, n2, room), unpack(w, p, n2, out)   the stage's buffers of a batch of n2 pairs, their
//                           read-back (timed), and the batch's results: per pair its record and out[x] = its items
// out_ptr, out_items: the items of all reads as a CSR in read order.
template <class Stage, class Shape>
static int cf_rd_run(cf_ctx* ctx, Stage& st, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int64_t batch_bytes, Shape& shape,
                     std::vector<int64_t>& out_ptr, std::vector<typename Stage::item>& out_items) {
    typedef typename Stage::pair pair;
    typedef typename Stage::win win;
    const std::string name = Stage::name, kernel = Stage::kernel;
    const int64_t r_total = read_off[n_reads] - read_off[0];
    // the score pass's pairs in descending length (empty reads have no pair)
    std::vector<int64_t> by_len;
    for (int64_t q = 0; q < n_reads; ++q)
        if (read_off[q + 1] > read_off[q]) by_len.push_back(q);
    std::stable_sort(by_len.begin(), by_len.end(), [&](int64_t x, int64_t y) { return read_off[x + 1] - read_off[x] > read_off[y + 1] - read_off[y]; });
    std::vector<pair> p1(2 * by_len.size());
    for (size_t o = 0; o < by_len.size(); ++o)
        for (int s = 0; s < 2; ++s) {
            const int64_t q = by_len[o];
            p1[2 * o + s] = st.score_pair(read_off[q] - read_off[0], (int32_t)(read_off[q + 1] - read_off[q]), s);
        }
    const int64_t n1 = (int64_t)p1.size(), n_sc = n1 * Stage::score_words;
    shape.n_score_pairs = n1;

    CF_HIP(hipSetDevice(ctx->device));
    hipEvent_t e0 = ctx->ev0, e1 = ctx->ev1, e2 = ctx->ev2;
    const auto lap = [&](hipEvent_t a, hipEvent_t b, int phase) { float t = 0.f; (void)hipEventElapsedTime(&t, a, b); shape.phase_ms[phase] += t; };
    cf_scratch tmp(ctx);
    uint8_t* d_reads = nullptr;
    pair* d_p1 = nullptr;
    cf_rd_dev dev{};
    CF_HIP(hipEventRecord(e0, ctx->stream));
    CF_TRY(tmp.get(&d_reads, (size_t)r_total + 16, (name + " reads").c_str()));
    CF_TRY(tmp.get(&d_p1, (size_t)n1 + 1, (name + " score pairs").c_str()));
    CF_TRY(tmp.get(&dev.score, (size_t)n_sc + 4, (name + " scores").c_str()));
    CF_TRY(tmp.get(&dev.fault, 1, (name + " fault flag").c_str()));
    CF_TRY(tmp.get(&dev.ticket, 2, (name + " ticket").c_str()));
    dev.reads = d_reads;
    if (r_total > 0) CF_TRY(cf_copy_h2d(ctx, d_reads, reads + read_off[0], (size_t)r_total));
    CF_TRY(st.upload(ctx, tmp));
    if (n1 > 0) CF_TRY(cf_copy_h2d(ctx, d_p1, p1.data(), (size_t)n1 * sizeof(pair)));
    CF_HIP(hipMemsetAsync(dev.fault, 0, 4, ctx->stream));
    CF_HIP(hipMemsetAsync(dev.ticket, 0, 16, ctx->stream));
    CF_HIP(hipEventRecord(e1, ctx->stream));
    const int cap = cf_rd_launch_cap(ctx);
    if (n1 > 0) {
        st.template launch<false>(ctx, (unsigned)std::min<int64_t>(n1, cap), (const pair*)d_p1, n1, dev);
        CF_KERNEL_CHECK(kernel + " (score pass)");
    }
    CF_HIP(hipEventRecord(e2, ctx->stream));
    CF_HIP(hipEventSynchronize(e2));
    lap(e0, e1, 0); lap(e1, e2, 1);

    CF_HIP(hipEventRecord(e0, ctx->stream));
    std::vector<int32_t> score((size_t)n_sc + 4);
    if (n1 > 0) CF_TRY(cf_copy_d2h(ctx, score.data(), dev.score, (size_t)n_sc * 4));
    CF_HIP(hipEventRecord(e1, ctx->stream));
    CF_HIP(hipEventSynchronize(e1));
    lap(e0, e1, 0);

    // the winners; the moves pass's pairs in descending rows, cut into batches
    std::vector<win> wins;
    for (size_t o = 0; o < by_len.size(); ++o) {
        const int64_t q = by_len[o];
        CF_TRY(st.pick(ctx, q, (int32_t)(read_off[q + 1] - read_off[q]), &score[2 * o * Stage::score_words], wins));
    }
    std::stable_sort(wins.begin(), wins.end(), [](const win& a, const win& b) { return a.rows > b.rows; });
    shape.n_move_pairs = (int64_t)wins.size();
    std::vector<std::vector<typename Stage::item>> per(wins.size());
    for (size_t first = 0; first < wins.size();) {
        size_t last = first;
        int64_t words = 0, room = 0;
        std::vector<pair> p2;
        while (last < wins.size()) {
            const win& w = wins[last];
            if (last > first && (words + w.words) * 4 > batch_bytes) break;
            p2.push_back(st.move_pair(w, read_off[w.q] - read_off[0], words, room));
            words += w.words;
            room += w.room;
            ++last;
        }
        const int64_t n2 = (int64_t)(last - first);
        CF_HIP(hipEventRecord(e0, ctx->stream));
        cf_scratch batch_tmp(ctx);
        pair* d_p2 = nullptr;
        CF_TRY(batch_tmp.get(&d_p2, (size_t)n2, (name + " move pairs").c_str()));
        CF_TRY(batch_tmp.get(&dev.area, (size_t)words + 1, (name + " move areas").c_str()));
        CF_TRY(st.batch_get(batch_tmp, n2, room));
        CF_TRY(cf_copy_h2d(ctx, d_p2, p2.data(), (size_t)n2 * sizeof(pair)));
        CF_HIP(hipMemsetAsync(dev.ticket, 0, 16, ctx->stream));
        CF_HIP(hipEventRecord(e1, ctx->stream));
        st.template launch<true>(ctx, (unsigned)std::min<int64_t>(n2, cap), (const pair*)d_p2, n2, dev);
        CF_KERNEL_CHECK(kernel + " (moves pass)");
        CF_HIP(hipEventRecord(e2, ctx->stream));
        CF_HIP(hipEventSynchronize(e2));
        lap(e0, e1, 0); lap(e1, e2, 2);
        CF_HIP(hipEventRecord(e0, ctx->stream));
        int32_t h_fault = 0;
        CF_TRY(cf_copy_d2h(ctx, &h_fault, dev.fault, 4));
        if (h_fault) return cf_fail(ctx, -5, Stage::fault);
        CF_TRY(st.fetch(ctx, dev, n2, room));
        CF_HIP(hipEventRecord(e1, ctx->stream));
        CF_HIP(hipEventSynchronize(e1));
        lap(e0, e1, 0);
        CF_TRY(st.unpack(ctx, &wins[first], p2.data(), n2, &per[first]));
        ++shape.n_batches;
        first = last;
    }
    // the items in read order
    std::vector<size_t> slot_of((size_t)n_reads, (size_t)-1);
    for (size_t x = 0; x < wins.size(); ++x) slot_of[(size_t)wins[x].q] = x;
    out_ptr.assign((size_t)n_reads + 1, 0);
    for (int64_t q = 0; q < n_reads; ++q) {
        out_ptr[(size_t)q] = (int64_t)out_items.size();
        if (slot_of[(size_t)q] != (size_t)-1) out_items.insert(out_items.end(), per[slot_of[(size_t)q]].begin(), per[slot_of[(size_t)q]].end());
    }
    out_ptr[(size_t)n_reads] = (int64_t)out_items.size();
    shape.phase_ms[3] = shape.phase_ms[0] + shape.phase_ms[1] + shape.phase_ms[2];
    return 0;
}
