// cf_radix.h — the stable, LDS-staged tile ranking shared by the LSD radix passes of A1 (cf_count2.hip) and the generic
// 64-bit key sort (cf_prims.hip).  Workgroups of CF_RX_THREADS threads; a tile's order is wave-major (wave w holds the
// records [w * 64 * items, ...) of the tile in rounds of 64), so array order = (wave, round, lane).
#pragma once
#include "cf_common.h"

#define CF_RX_THREADS 256

// ---- stable ranking of one round (one record per thread) by digit: a ballot match per digit bit
struct cf_rx_rank { uint32_t rank, count; };
template <int NB>
__device__ __forceinline__ cf_rx_rank cf_rx_wave_rank(uint32_t digit, bool valid, int lane) {
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int bit = (digit >> b) & 1;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return cf_rx_rank{(uint32_t)__popcll(peers & ((1ull << lane) - 1ull)), (uint32_t)__popcll(peers)};
}

// A wave ranks its own records by itself — per round a ballot match per digit bit, across rounds a running count per digit
// in the wave's private LDS row — so the workgroup meets only twice per tile: to turn the rows into exclusive offsets
// across waves, and before the rows are reused.  Returns the rank of the record among the records of its wave with the
// same digit.
template <int NB>
__device__ __forceinline__ uint32_t cf_rx_rank_round(uint32_t digit, bool valid, uint32_t* wrow) {     // wrow: this wave's 1 << NB counters
    const int lane = threadIdx.x & 63;
    const cf_rx_rank rk = cf_rx_wave_rank<NB>(digit, valid, lane);
    uint32_t before = 0;
    if (valid) before = wrow[digit];                       // records of earlier rounds (only this wave writes the row; LDS ops of a wave are in order)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (valid && rk.rank == 0) wrow[digit] = before + rk.count;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return before + rk.rank;
}

// after all rounds: wcount rows -> exclusive prefix over the waves (in place), dstart[d] = first position of digit d in
// the tile sorted by digit (exclusive scan of the tile's digit counts; 1 << NB <= 2 * CF_RX_THREADS), scan_tmp[7] = the
// tile's records
template <int NB, int ROWS = CF_RX_THREADS / 64>
__device__ __forceinline__ void cf_rx_tile_bases(uint32_t* dstart, uint32_t* wcount, uint32_t* scan_tmp) {
    __syncthreads();
    const int t = threadIdx.x;
    uint32_t tot[2] = {0, 0};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int d = 2 * t + h;
        if (d < (1 << NB)) {
            uint32_t s = 0;
            for (int w = 0; w < ROWS; ++w) { const uint32_t c = wcount[w * (1 << NB) + d]; wcount[w * (1 << NB) + d] = s; s += c; }
            tot[h] = s;
        }
    }
    // exclusive scan of tot over the threads (2 digits each)
    const int lane = t & 63, wave = t >> 6;
    uint32_t inc = tot[0] + tot[1];
    const uint32_t mine = inc;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, (unsigned)d); if (lane >= d) inc += o; }
    if (lane == 63) scan_tmp[wave] = inc;
    __syncthreads();
    uint32_t off = inc - mine;
    for (int w = 0; w < wave; ++w) off += scan_tmp[w];
    if (2 * t < (1 << NB)) dstart[2 * t] = off;
    if (2 * t + 1 < (1 << NB)) dstart[2 * t + 1] = off + tot[0];
    if (t == CF_RX_THREADS - 1) scan_tmp[7] = off + mine;          // records of the tile
    __syncthreads();
}
