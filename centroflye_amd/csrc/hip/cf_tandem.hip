// cf_tandem.hip — tandem period, best distance window and hook k-mer of many raw reads in one batch (gfx950, wave64).
//
// Reference: scripts/unit_extractor.py:23-30 (get_repetitive_kmers), :33-40 (get_convolution), :43-78 (get_period_info), :81-89
// (get_hook_kmer) and the scan for the hook's positions of :92-97 (split_by_hook), one read at a time in Python dicts.  Here every
// read of a batch goes through the same few passes; no pass depends on another read.
//
//   records     one record per window whose k bases are upper-case A, C, G, T: (read in batch, 2k-bit code, position), written in
//               (read, position) order.  A window that holds another byte writes an invalid record and marks its read "exotic" (the
//               Python layer redoes such reads on the host: the reference compares raw strings).
//   sort        the stable LSD sorts of cf_prims.hip on (read, code) only: the position rides along and stays ascending inside a
//               (read, code) run because the sort is stable.  Keys are 64-bit [position | invalid | read | code] when that fits,
//               16-byte records {code lo, code hi, read, position} otherwise.
//   runs        a record whose predecessor has the same (read, code) yields one distance; the head of a run of two or more is one
//               repetitive k-mer.  Per-read counts are differences of the flags' exclusive scans at the read's segment borders
//               (a binary search per read): no atomics.
//   distances   [read | distance] compacted through the scan and sorted: every read's union_conv, back to back.
//   windows     one thread per l: r(l) by binary search, count = r - l.  The loop of :52-75 visits l only while r(l - 1) < n.  Per
//               read the first and the last visited l with the largest count are two packed 64-bit maxima, reduced over the lanes
//               of a wave that hold the same read and sent with ONE atomic per (wave, read).  The first gives bin_left / bin_right
//               (:73-74 keeps the first best window); the last gives periods[0]: among windows of equal count the period is
//               non-decreasing in l (conv is sorted), so the period "whose first l is largest" is the period of the last one.
//   hook        per (read, code) run the distances inside [bin_left, bin_right] = a difference of one more scan at the run's
//               borders (the run's end by binary search); per read the arg-max of (tandem_index, -first position) as one packed
//               64-bit maximum, again one atomic per (wave, read); the hook's run is the hook's positions (a CSR over reads).
// Every loop is a binary search of at most 64 steps, a loop over the k <= 31 bases of a window or a grid-stride loop.
#include "cf_common.h"

#define CF_TD_THREADS 256
#define CF_TD_SORT_TILE 4096            // keys per tile of cf_radix_sort_u64_any (cf_prims.hip: CF_RX_THREADS x RX_ITEMS)
#define CF_TD_REC_TILE 2048             // records per tile of cf_radix_sort_rec16
#define CF_TD_SCAN_TILE 2048            // entries per tile of the exclusive scan
#define CF_TD_BATCH_WINDOWS ((int64_t)1 << 26)
#define CF_TD_MAX_LEN 0x7fffffffll      // a read holds fewer than 2^31 bases
#define CF_TD_NOREAD 0xffffffffu

struct __attribute__((aligned(16))) cf_td_rec { uint32_t w[4]; };      // code low, code high, read (n_batch = invalid), position

// how a sorted record is read back: mode 1 = 64-bit keys, mode 2 = 16-byte records
struct cf_td_view {
    const unsigned long long* keys;
    const cf_td_rec* recs;
    int mode, code_bits, read_bits, pos_shift;
    uint32_t n_batch;
};

struct cf_td_item { uint32_t read, pos; unsigned long long code; };     // read == CF_TD_NOREAD: an invalid record

__device__ __forceinline__ cf_td_item cf_td_get(const cf_td_view& v, int64_t i) {
    cf_td_item it;
    if (v.mode == 1) {
        const unsigned long long key = v.keys[i];
        it.code = key & ((1ull << v.code_bits) - 1ull);
        const unsigned long long rest = key >> v.code_bits;
        it.read = (uint32_t)(rest & ((1ull << v.read_bits) - 1ull));
        if ((rest >> v.read_bits) & 1ull) it.read = CF_TD_NOREAD;
        it.pos = (uint32_t)(key >> v.pos_shift);
    } else {
        const cf_td_rec r = v.recs[i];
        it.code = (unsigned long long)r.w[0] | ((unsigned long long)r.w[1] << 32);
        it.read = r.w[2] >= v.n_batch ? CF_TD_NOREAD : r.w[2];
        it.pos = r.w[3];
    }
    return it;
}
__device__ __forceinline__ bool cf_td_same(const cf_td_item& a, const cf_td_item& b) { return a.read == b.read && a.code == b.code; }

// the largest value among the lanes of the wave that hold the same `seg` (equal segments are neighbours), sent by the last lane of
// every segment with one atomicMax; seg == CF_TD_NOREAD: a lane without a value.  All 64 lanes call this.
__device__ __forceinline__ void cf_td_wave_seg_max(uint32_t seg, unsigned long long val, unsigned long long* __restrict__ dst) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(val, (unsigned)d);
        const uint32_t os = __shfl_up(seg, (unsigned)d);
        if (lane >= d && os == seg && o > val) val = o;
    }
    const uint32_t next = __shfl_down(seg, 1u);
    const bool tail = lane == 63 || next != seg;
    if (tail && seg != CF_TD_NOREAD && val != 0ull) atomicMax(&dst[seg], val);
}

// ------------------------------------------------------------------ records
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_records_kernel(const uint8_t* __restrict__ bases, const int64_t* __restrict__ read_off, const int64_t* __restrict__ win_off, int64_t nb,
                     int64_t n_win, int k, int mode, int code_bits, int read_bits, int pos_shift, unsigned long long* __restrict__ keys,
                     cf_td_rec* __restrict__ recs, uint32_t* __restrict__ exotic) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_win; i += (int64_t)gridDim.x * blockDim.x) {
        // the read of window slot i: the last r with win_off[r] <= i (reads without a window share their successor's offset)
        int64_t lo = 0, hi = nb;
        for (int s = 0; s < 64 && lo < hi; ++s) {
            const int64_t m = (lo + hi) >> 1;
            if (win_off[m] <= i) lo = m + 1; else hi = m;
        }
        const int64_t r = lo - 1;
        const int64_t p = i - win_off[r];
        const uint8_t* w = bases + read_off[r] + p;
        unsigned long long code = 0;
        bool ok = true;
        for (int j = 0; j < k; ++j) {
            const uint32_t c = w[j];
            ok = ok && cf_is_acgt(c);
            code = (code << 2) | cf_base2(c);
        }
        if (!ok) exotic[r] = 1u;      // (every writer stores the same value)
        if (mode == 1) {
            keys[i] = ok ? (((unsigned long long)p << pos_shift) | ((unsigned long long)r << code_bits) | code)
                         : (((unsigned long long)p << pos_shift) | (1ull << (code_bits + read_bits)));
        } else {
            cf_td_rec o;
            o.w[0] = ok ? (uint32_t)code : 0u;
            o.w[1] = ok ? (uint32_t)(code >> 32) : 0u;
            o.w[2] = ok ? (uint32_t)r : (uint32_t)nb;
            o.w[3] = (uint32_t)p;
            recs[i] = o;
        }
    }
}

// ------------------------------------------------------------------ runs
// is_diff[i]: record i follows a record of the same (read, code); is_rep[i]: record i heads a run of two or more.  Entry n_win of
// both is 0: the scans then hold n_win + 1 prefixes.
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_runs_kernel(cf_td_view v, int64_t n_win, uint32_t* __restrict__ is_diff, uint32_t* __restrict__ is_rep) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_win; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t d = 0, h = 0;
        if (i < n_win) {
            const cf_td_item me = cf_td_get(v, i);
            if (me.read != CF_TD_NOREAD) {
                if (i > 0 && cf_td_same(cf_td_get(v, i - 1), me)) d = 1;
                else if (i + 1 < n_win && cf_td_same(cf_td_get(v, i + 1), me)) h = 1;
            }
        }
        is_diff[i] = d;
        is_rep[i] = h;
    }
}

// seg[r] = the first sorted record of a read >= r, r = 0 .. nb (invalid records sort behind every read)
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_segments_kernel(cf_td_view v, int64_t n_win, int64_t nb, int64_t* __restrict__ seg) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= nb; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = n_win;
        for (int s = 0; s < 64 && lo < hi; ++s) {
            const int64_t m = (lo + hi) >> 1;
            if ((int64_t)cf_td_get(v, m).read < r) lo = m + 1; else hi = m;      // (CF_TD_NOREAD >= nb)
        }
        seg[r] = lo;
    }
}

// dkeys[pre_diff[i]] = read << dshift | (position - predecessor's position)
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_diffs_kernel(cf_td_view v, int64_t n_win, const uint32_t* __restrict__ is_diff, const int64_t* __restrict__ pre_diff, int dshift,
                   unsigned long long* __restrict__ dkeys) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_win; i += (int64_t)gridDim.x * blockDim.x) {
        if (!is_diff[i]) continue;
        const cf_td_item me = cf_td_get(v, i), before = cf_td_get(v, i - 1);
        dkeys[pre_diff[i]] = ((unsigned long long)me.read << dshift) | (unsigned long long)(me.pos - before.pos);
    }
}

// ------------------------------------------------------------------ windows
__device__ __forceinline__ int64_t cf_td_dist(const unsigned long long* __restrict__ dkeys, int64_t i, int dshift) {
    return (int64_t)(dkeys[i] & ((1ull << dshift) - 1ull));
}
// r(l): the first index in (l, c1] whose distance exceeds conv[l] + 2 bin_size
__device__ __forceinline__ int64_t cf_td_window_end(const unsigned long long* __restrict__ dkeys, int64_t l, int64_t c1, int dshift, int64_t bin2) {
    const int64_t lim = cf_td_dist(dkeys, l, dshift) + bin2;
    int64_t lo = l + 1, hi = c1;
    for (int s = 0; s < 64 && lo < hi; ++s) {
        const int64_t m = (lo + hi) >> 1;
        if (cf_td_dist(dkeys, m, dshift) <= lim) lo = m + 1; else hi = m;
    }
    return lo;
}

// best_first[r] = max (count << 32 | ~l), best_last[r] = max (count << 32 | l) over the windows the reference's loop visits (l local)
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_windows_kernel(const unsigned long long* __restrict__ dkeys, int64_t n_diff, int dshift, const int64_t* __restrict__ seg,
                     const int64_t* __restrict__ pre_diff, int64_t bin2, unsigned long long* __restrict__ best_first,
                     unsigned long long* __restrict__ best_last) {
    const int64_t rounds = (n_diff + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x);
    for (int64_t it = 0; it < rounds; ++it) {      // (whole waves stay in the loop: the reduction shuffles)
        const int64_t l = (it * gridDim.x + blockIdx.x) * (int64_t)blockDim.x + threadIdx.x;
        uint32_t r = CF_TD_NOREAD;
        unsigned long long first = 0, last = 0;
        if (l < n_diff) {
            const uint32_t rr = (uint32_t)(dkeys[l] >> dshift);
            const int64_t c0 = pre_diff[seg[rr]], c1 = pre_diff[seg[rr + 1]];
            // visited: l = 0, or r(l - 1) < n, i.e. the last distance lies beyond conv[l - 1] + 2 bin_size
            if (l == c0 || cf_td_dist(dkeys, c1 - 1, dshift) - cf_td_dist(dkeys, l - 1, dshift) > bin2) {
                const unsigned long long count = (unsigned long long)(cf_td_window_end(dkeys, l, c1, dshift, bin2) - l);
                const uint32_t ll = (uint32_t)(l - c0);
                r = rr;
                first = (count << 32) | (unsigned long long)(0xffffffffu - ll);
                last = (count << 32) | (unsigned long long)ll;
            }
        }
        cf_td_wave_seg_max(r, first, best_first);
        cf_td_wave_seg_max(r, last, best_last);
    }
}

// per read: the counts, the best window, the period; bins[2 r], bins[2 r + 1] = bin_left, bin_right (1, 0 without a window)
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_finish_kernel(const unsigned long long* __restrict__ dkeys, int dshift, const int64_t* __restrict__ seg, const int64_t* __restrict__ pre_diff,
                    const int64_t* __restrict__ pre_rep, const uint32_t* __restrict__ exotic, const unsigned long long* __restrict__ best_first,
                    const unsigned long long* __restrict__ best_last, int64_t nb, int64_t bin2, cf_tandem_read* __restrict__ out,
                    int32_t* __restrict__ bins) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < nb; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c0 = pre_diff[seg[r]], c1 = pre_diff[seg[r + 1]], n = c1 - c0;
        cf_tandem_read o;
        o.status = exotic[r] ? CF_TANDEM_EXOTIC : (n > 0 ? CF_TANDEM_OK : CF_TANDEM_NO_PERIOD);
        o.n_windows = 0;
        o.n_rep_kmers = (int32_t)(pre_rep[seg[r + 1]] - pre_rep[seg[r]]);
        o.n_conv = (int32_t)n;
        o.count = 0; o.bin_left = 0; o.bin_right = 0; o.period = 0;
        o.hook_pos = -1; o.hook_index = 0; o.n_hook = 0;
        int32_t bl = 1, br = 0;
        if (n > 0) {
            const int64_t C = (int64_t)(best_first[r] >> 32);
            const int64_t lf = (int64_t)(0xffffffffu - (uint32_t)best_first[r]), ll = (int64_t)(uint32_t)best_last[r];
            bl = (int32_t)cf_td_dist(dkeys, c0 + lf, dshift);
            br = (int32_t)cf_td_dist(dkeys, c0 + lf + C - 1, dshift);
            const int64_t mid = c0 + ll + C / 2;
            o.period = (C & 1) ? (int32_t)cf_td_dist(dkeys, mid, dshift)
                               : (int32_t)((cf_td_dist(dkeys, mid, dshift) + cf_td_dist(dkeys, mid - 1, dshift)) / 2);
            o.count = (int32_t)C; o.bin_left = bl; o.bin_right = br;
            // visited windows: up to the first l with conv[l] + 2 bin_size >= the last distance
            const int64_t need = cf_td_dist(dkeys, c1 - 1, dshift) - bin2;
            int64_t lo = c0, hi = c1 - 1;
            for (int s = 0; s < 64 && lo < hi; ++s) {
                const int64_t m = (lo + hi) >> 1;
                if (cf_td_dist(dkeys, m, dshift) < need) lo = m + 1; else hi = m;
            }
            o.n_windows = (int32_t)(lo - c0 + 1);
        }
        out[r] = o;
        bins[2 * r] = bl;
        bins[2 * r + 1] = br;
    }
}

// ------------------------------------------------------------------ hook
// in_bin[i]: record i yields a distance inside its read's [bin_left, bin_right] (both ends closed)
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_inbin_kernel(cf_td_view v, int64_t n_win, const uint32_t* __restrict__ is_diff, const int32_t* __restrict__ bins, uint32_t* __restrict__ in_bin) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_win; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t f = 0;
        if (i < n_win && is_diff[i]) {
            const cf_td_item me = cf_td_get(v, i), before = cf_td_get(v, i - 1);
            const int64_t d = (int64_t)me.pos - (int64_t)before.pos;
            f = d >= (int64_t)bins[2 * (int64_t)me.read] && d <= (int64_t)bins[2 * (int64_t)me.read + 1];
        }
        in_bin[i] = f;
    }
}

// best_hook[r] = max over the repetitive k-mers of (tandem_index << 32 | ~first position), tandem_index > 0
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_hook_best_kernel(cf_td_view v, int64_t n_win, const uint32_t* __restrict__ is_rep, const int64_t* __restrict__ seg,
                       const int64_t* __restrict__ pre_in, unsigned long long* __restrict__ best_hook) {
    const int64_t rounds = (n_win + (int64_t)gridDim.x * blockDim.x - 1) / ((int64_t)gridDim.x * blockDim.x);
    for (int64_t it = 0; it < rounds; ++it) {
        const int64_t i = (it * gridDim.x + blockIdx.x) * (int64_t)blockDim.x + threadIdx.x;
        uint32_t r = CF_TD_NOREAD;
        unsigned long long val = 0;
        if (i < n_win) {
            const cf_td_item me = cf_td_get(v, i);
            r = me.read;
            if (r != CF_TD_NOREAD && is_rep[i]) {
                int64_t lo = i + 1, hi = seg[r + 1];      // the end of the run: the first record of the read with a larger code
                for (int s = 0; s < 64 && lo < hi; ++s) {
                    const int64_t m = (lo + hi) >> 1;
                    if (cf_td_get(v, m).code <= me.code) lo = m + 1; else hi = m;
                }
                const unsigned long long index = (unsigned long long)(pre_in[lo] - pre_in[i]);
                if (index) val = (index << 32) | (unsigned long long)(0xffffffffu - me.pos);
            }
        }
        cf_td_wave_seg_max(r, val, best_hook);
    }
}

// per read: the hook's code from its first position, its run in the sorted records, the result fields
__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_hook_pick_kernel(cf_td_view v, const uint8_t* __restrict__ bases, const int64_t* __restrict__ read_off, const int64_t* __restrict__ seg,
                       const unsigned long long* __restrict__ best_hook, int64_t nb, int k, cf_tandem_read* __restrict__ out,
                       int64_t* __restrict__ hook_first, uint32_t* __restrict__ hook_n) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= nb; r += (int64_t)gridDim.x * blockDim.x) {
        uint32_t n = 0;
        int64_t first = 0;
        if (r < nb && best_hook[r] != 0ull) {
            const uint32_t pos = 0xffffffffu - (uint32_t)best_hook[r];
            const uint8_t* w = bases + read_off[r] + pos;
            unsigned long long code = 0;
            for (int j = 0; j < k; ++j) code = (code << 2) | cf_base2(w[j]);
            int64_t lo = seg[r], hi = seg[r + 1];
            for (int s = 0; s < 64 && lo < hi; ++s) {
                const int64_t m = (lo + hi) >> 1;
                if (cf_td_get(v, m).code < code) lo = m + 1; else hi = m;
            }
            first = lo;
            hi = seg[r + 1];
            for (int s = 0; s < 64 && lo < hi; ++s) {
                const int64_t m = (lo + hi) >> 1;
                if (cf_td_get(v, m).code <= code) lo = m + 1; else hi = m;
            }
            n = (uint32_t)(lo - first);
            out[r].hook_pos = (int32_t)pos;
            out[r].hook_index = (int32_t)(best_hook[r] >> 32);
            out[r].n_hook = (int32_t)n;
        }
        hook_first[r] = first;
        hook_n[r] = n;      // (entry nb is 0: the scan holds nb + 1 prefixes)
    }
}

__global__ void __launch_bounds__(CF_TD_THREADS)
cf_td_hook_copy_kernel(cf_td_view v, const int64_t* __restrict__ hook_first, const int64_t* __restrict__ hook_ptr, int64_t nb, int64_t n_hook,
                       int32_t* __restrict__ hook_pos) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_hook; j += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = nb;      // the last r with hook_ptr[r] <= j
        for (int s = 0; s < 64 && lo < hi; ++s) {
            const int64_t m = (lo + hi) >> 1;
            if (hook_ptr[m] <= j) lo = m + 1; else hi = m;
        }
        const int64_t r = lo - 1;
        hook_pos[j] = (int32_t)cf_td_get(v, hook_first[r] + (j - hook_ptr[r])).pos;
    }
}

// ------------------------------------------------------------------ host
static int td_bits(uint64_t x) {      // bits that hold the values 0 .. x
    int b = 1;
    while (b < 64 && (x >> b) != 0) ++b;
    return b;
}
static int td_round8(int b) { return (b + 7) & ~7; }

struct td_layout { int mode, code_bits, read_bits, pos_bits, pos_shift; };

// the key layout of a batch of nb reads whose longest has max_len bases; fits = it may use 64-bit keys
static td_layout td_layout_of(int k, int64_t nb, int64_t max_len, bool* fits) {
    td_layout L;
    L.code_bits = 2 * k;
    L.read_bits = td_bits((uint64_t)std::max<int64_t>(nb - 1, 0));
    L.pos_bits = td_bits((uint64_t)std::max<int64_t>(max_len - 1, 0));
    L.pos_shift = td_round8(L.code_bits + L.read_bits + 1);      // (the sort works on whole bytes: the position starts on the next one)
    *fits = L.pos_shift + L.pos_bits <= 64;
    L.mode = *fits ? 1 : 2;
    return L;
}

struct td_events {
    hipEvent_t e[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~td_events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

// one batch: reads [r0, r1) of the caller's arrays
static int td_batch(cf_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t r0, int64_t r1, int k, int64_t bin2, const td_layout& L,
                    td_events& ev, cf_tandem_read* out, std::vector<int64_t>& hook_ptr, std::vector<int32_t>& hook_pos, int64_t* n_records,
                    float* phase_ms) {
    const int64_t nb = r1 - r0, base = read_off[r0], n_bytes = read_off[r1] - base;
    std::vector<int64_t> off((size_t)nb + 1), win((size_t)nb + 1);
    win[0] = 0;
    for (int64_t i = 0; i <= nb; ++i) off[(size_t)i] = read_off[r0 + i] - base;
    for (int64_t i = 0; i < nb; ++i) win[(size_t)i + 1] = win[(size_t)i] + std::max<int64_t>(off[(size_t)i + 1] - off[(size_t)i] - k + 1, 0);
    const int64_t N = win[(size_t)nb];
    *n_records += N;
    const int maxb = std::max(1, ctx->n_cu) * 16;
    const int gN = cf_grid_for(N + 1, CF_TD_THREADS, maxb), gR = cf_grid_for(nb + 1, CF_TD_THREADS, maxb);
    const int dshift = L.pos_bits;
    uint8_t* d_bases = nullptr;
    int64_t *d_off = nullptr, *d_win = nullptr, *d_seg = nullptr, *d_pre_diff = nullptr, *d_pre_rep = nullptr, *d_pre_in = nullptr;
    int64_t *d_hook_first = nullptr, *d_hook_ptr = nullptr;
    unsigned long long *d_keys = nullptr, *d_tmp = nullptr, *d_dkeys = nullptr, *d_dtmp = nullptr, *d_best = nullptr;
    cf_td_rec *d_recs = nullptr, *d_rtmp = nullptr;
    uint32_t *d_exotic = nullptr, *d_is_diff = nullptr, *d_is_rep = nullptr, *d_hook_n = nullptr;
    int32_t *d_bins = nullptr, *d_hook_pos = nullptr;
    cf_tandem_read* d_out = nullptr;
    int64_t n_diff = 0, n_hook = 0;
    cf_scratch tmp(ctx);
    CF_TRY(tmp.get(&d_bases, (size_t)n_bytes + 1, "tandem bases"));
    CF_TRY(tmp.get(&d_off, (size_t)nb + 1, "tandem read offsets"));
    CF_TRY(tmp.get(&d_win, (size_t)nb + 1, "tandem window offsets"));
    CF_TRY(tmp.get(&d_seg, (size_t)nb + 1, "tandem read segments"));
    CF_TRY(tmp.get(&d_exotic, (size_t)nb + 1, "tandem exotic flags"));
    CF_TRY(tmp.get(&d_best, (size_t)nb * 3 + 1, "tandem maxima"));
    CF_TRY(tmp.get(&d_bins, (size_t)nb * 2 + 1, "tandem bins"));
    CF_TRY(tmp.get(&d_out, (size_t)nb + 1, "tandem results"));
    CF_TRY(tmp.get(&d_hook_first, (size_t)nb + 1, "tandem hook runs"));
    CF_TRY(tmp.get(&d_hook_ptr, (size_t)nb + 1, "tandem hook offsets"));
    CF_TRY(tmp.get(&d_hook_n, (size_t)nb + 1, "tandem hook counts"));
    if (L.mode == 1) {
        CF_TRY(tmp.get(&d_keys, (size_t)N + 1, "tandem keys"));
        CF_TRY(tmp.get(&d_tmp, (size_t)N + 1, "tandem keys"));
    } else {
        CF_TRY(tmp.get(&d_recs, (size_t)N + 1, "tandem records"));
        CF_TRY(tmp.get(&d_rtmp, (size_t)N + 1, "tandem records"));
    }
    CF_TRY(tmp.get(&d_is_diff, (size_t)N + 1, "tandem flags"));
    CF_TRY(tmp.get(&d_is_rep, (size_t)N + 1, "tandem flags"));
    CF_TRY(tmp.get(&d_pre_diff, (size_t)N + 1, "tandem prefixes"));
    CF_TRY(tmp.get(&d_pre_rep, (size_t)N + 1, "tandem prefixes"));
    CF_TRY(tmp.get(&d_pre_in, (size_t)N + 1, "tandem prefixes"));
    if (n_bytes > 0) CF_TRY(cf_copy_h2d(ctx, d_bases, reads + base, (size_t)n_bytes));
    CF_TRY(cf_copy_h2d(ctx, d_off, off.data(), ((size_t)nb + 1) * 8));
    CF_TRY(cf_copy_h2d(ctx, d_win, win.data(), ((size_t)nb + 1) * 8));
    CF_HIP(hipMemsetAsync(d_exotic, 0, ((size_t)nb + 1) * 4, ctx->stream));
    CF_HIP(hipMemsetAsync(d_best, 0, ((size_t)nb * 3 + 1) * 8, ctx->stream));
    unsigned long long *d_first = d_best, *d_last = d_best + nb, *d_hook = d_best + 2 * nb;

    // records
    CF_HIP(hipEventRecord(ev.e[0], ctx->stream));
    if (N > 0) {
        hipLaunchKernelGGL(cf_td_records_kernel, dim3((unsigned)gN), dim3(CF_TD_THREADS), 0, ctx->stream, (const uint8_t*)d_bases, (const int64_t*)d_off,
                           (const int64_t*)d_win, nb, N, k, L.mode, L.code_bits, L.read_bits, L.pos_shift, d_keys, d_recs, d_exotic);
        CF_KERNEL_CHECK("cf_td_records_kernel");
    }
    CF_HIP(hipEventRecord(ev.e[1], ctx->stream));
    // sort by (read, code); the position keeps its order
    cf_td_view v{};
    v.mode = L.mode; v.code_bits = L.code_bits; v.read_bits = L.read_bits; v.pos_shift = L.pos_shift; v.n_batch = (uint32_t)nb;
    if (L.mode == 1) {
        unsigned long long* sorted = d_keys;
        CF_TRY(cf_radix_sort_u64_any(ctx, d_keys, d_tmp, N, L.code_bits + L.read_bits + 1, &sorted));
        v.keys = sorted;
    } else {
        int words[3], bits[3], nf = 0;
        words[nf] = 0; bits[nf++] = std::min(32, L.code_bits);
        if (L.code_bits > 32) { words[nf] = 1; bits[nf++] = L.code_bits - 32; }
        words[nf] = 2; bits[nf++] = td_bits((uint64_t)nb);      // (the value nb marks an invalid record)
        CF_TRY(cf_radix_sort_rec16(ctx, d_recs, d_rtmp, N, words, bits, nf));
        v.recs = d_recs;
    }
    CF_HIP(hipEventRecord(ev.e[2], ctx->stream));
    // runs, per-read segments, the distances
    hipLaunchKernelGGL(cf_td_runs_kernel, dim3((unsigned)gN), dim3(CF_TD_THREADS), 0, ctx->stream, v, N, d_is_diff, d_is_rep);
    hipLaunchKernelGGL(cf_td_segments_kernel, dim3((unsigned)gR), dim3(CF_TD_THREADS), 0, ctx->stream, v, N, nb, d_seg);
    CF_KERNEL_CHECK("cf_td_runs_kernel / cf_td_segments_kernel");
    CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_is_diff, d_pre_diff, N + 1, &n_diff));
    CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_is_rep, d_pre_rep, N + 1, nullptr));
    CF_TRY(tmp.get(&d_dkeys, (size_t)n_diff + 1, "tandem distances"));
    CF_TRY(tmp.get(&d_dtmp, (size_t)n_diff + 1, "tandem distances"));
    if (n_diff > 0) {
        hipLaunchKernelGGL(cf_td_diffs_kernel, dim3((unsigned)gN), dim3(CF_TD_THREADS), 0, ctx->stream, v, N, (const uint32_t*)d_is_diff,
                           (const int64_t*)d_pre_diff, dshift, d_dkeys);
        CF_KERNEL_CHECK("cf_td_diffs_kernel");
    }
    CF_HIP(hipEventRecord(ev.e[3], ctx->stream));
    unsigned long long* conv = d_dkeys;
    CF_TRY(cf_radix_sort_u64_any(ctx, d_dkeys, d_dtmp, n_diff, dshift + L.read_bits, &conv));
    CF_HIP(hipEventRecord(ev.e[4], ctx->stream));
    // windows
    if (n_diff > 0) {
        const int gD = cf_grid_for(n_diff, CF_TD_THREADS, maxb);
        hipLaunchKernelGGL(cf_td_windows_kernel, dim3((unsigned)gD), dim3(CF_TD_THREADS), 0, ctx->stream, (const unsigned long long*)conv, n_diff, dshift,
                           (const int64_t*)d_seg, (const int64_t*)d_pre_diff, bin2, d_first, d_last);
    }
    hipLaunchKernelGGL(cf_td_finish_kernel, dim3((unsigned)gR), dim3(CF_TD_THREADS), 0, ctx->stream, (const unsigned long long*)conv, dshift,
                       (const int64_t*)d_seg, (const int64_t*)d_pre_diff, (const int64_t*)d_pre_rep, (const uint32_t*)d_exotic,
                       (const unsigned long long*)d_first, (const unsigned long long*)d_last, nb, bin2, d_out, d_bins);
    CF_KERNEL_CHECK("cf_td_windows_kernel / cf_td_finish_kernel");
    CF_HIP(hipEventRecord(ev.e[5], ctx->stream));
    // hook
    uint32_t* d_in_bin = d_is_diff;      // written in place: entry i depends on is_diff[i] alone, and nothing reads is_diff afterwards
    hipLaunchKernelGGL(cf_td_inbin_kernel, dim3((unsigned)gN), dim3(CF_TD_THREADS), 0, ctx->stream, v, N, (const uint32_t*)d_is_diff, (const int32_t*)d_bins, d_in_bin);
    CF_KERNEL_CHECK("cf_td_inbin_kernel");
    CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_in_bin, d_pre_in, N + 1, nullptr));
    if (N > 0) {
        hipLaunchKernelGGL(cf_td_hook_best_kernel, dim3((unsigned)cf_grid_for(N, CF_TD_THREADS, maxb)), dim3(CF_TD_THREADS), 0, ctx->stream, v, N,
                           (const uint32_t*)d_is_rep, (const int64_t*)d_seg, (const int64_t*)d_pre_in, d_hook);
    }
    hipLaunchKernelGGL(cf_td_hook_pick_kernel, dim3((unsigned)gR), dim3(CF_TD_THREADS), 0, ctx->stream, v, (const uint8_t*)d_bases, (const int64_t*)d_off,
                       (const int64_t*)d_seg, (const unsigned long long*)d_hook, nb, k, d_out, d_hook_first, d_hook_n);
    CF_KERNEL_CHECK("cf_td_hook_best_kernel / cf_td_hook_pick_kernel");
    CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, d_hook_n, d_hook_ptr, nb + 1, &n_hook));
    CF_TRY(tmp.get(&d_hook_pos, (size_t)n_hook + 1, "tandem hook positions"));
    if (n_hook > 0) {
        hipLaunchKernelGGL(cf_td_hook_copy_kernel, dim3((unsigned)cf_grid_for(n_hook, CF_TD_THREADS, maxb)), dim3(CF_TD_THREADS), 0, ctx->stream, v,
                           (const int64_t*)d_hook_first, (const int64_t*)d_hook_ptr, nb, n_hook, d_hook_pos);
        CF_KERNEL_CHECK("cf_td_hook_copy_kernel");
    }
    CF_HIP(hipEventRecord(ev.e[6], ctx->stream));
    CF_HIP(hipEventSynchronize(ev.e[6]));
    {
        // records | sort | runs and distances | sort | windows | hook
        static const int phase_of[6] = {0, 1, 2, 1, 3, 4};
        for (int i = 0; i < 6; ++i) {
            float t = 0.f;
            (void)hipEventElapsedTime(&t, ev.e[i], ev.e[i + 1]);
            phase_ms[phase_of[i]] += t;
        }
    }
    CF_TRY(cf_copy_d2h(ctx, out + r0, d_out, (size_t)nb * sizeof(cf_tandem_read)));
    const size_t h0 = hook_pos.size();
    std::vector<int64_t> ptr((size_t)nb + 1);
    CF_TRY(cf_copy_d2h(ctx, ptr.data(), d_hook_ptr, ((size_t)nb + 1) * 8));
    hook_pos.resize(h0 + (size_t)n_hook);
    if (n_hook > 0) CF_TRY(cf_copy_d2h(ctx, hook_pos.data() + h0, d_hook_pos, (size_t)n_hook * 4));
    for (int64_t i = 1; i <= nb; ++i) hook_ptr.push_back((int64_t)h0 + ptr[(size_t)i]);
    return 0;
}

extern "C" {

int cf_tandem_info(cf_ctx* ctx, cf_tandem_shape* out) {
    if (!ctx || !out) return -22;
    *out = ctx->tandem_last;
    out->sort_tile = CF_TD_SORT_TILE;
    out->rec_tile = CF_TD_REC_TILE;
    out->scan_tile = CF_TD_SCAN_TILE;
    out->block = CF_TD_THREADS;
    out->batch_windows = ctx->tandem_batch_windows > 0 ? ctx->tandem_batch_windows : CF_TD_BATCH_WINDOWS;
    return 0;
}

int cf_tandem_scan(cf_ctx* ctx, const uint8_t* reads, const int64_t* read_off, int64_t n_reads, int32_t k, int32_t bin_size, cf_tandem_read* out) {
    if (!ctx) return -22;
    if (n_reads < 0) return cf_fail(ctx, -22, "cf_tandem_scan: negative number of reads");
    if (k < 1 || k > 31) return cf_fail(ctx, -22, "cf_tandem_scan: k must lie in 1 .. 31");
    if (bin_size < 0) return cf_fail(ctx, -22, "cf_tandem_scan: negative bin size");
    if (!read_off) return cf_fail(ctx, -22, "cf_tandem_scan: null offsets");
    if (read_off[0] < 0) return cf_fail(ctx, -22, "cf_tandem_scan: negative offset");
    for (int64_t i = 0; i < n_reads; ++i) {
        if (read_off[i + 1] < read_off[i]) return cf_fail(ctx, -22, "cf_tandem_scan: offsets of read " + std::to_string(i) + " decrease");
        if (read_off[i + 1] - read_off[i] > CF_TD_MAX_LEN) return cf_fail(ctx, -22, "cf_tandem_scan: read " + std::to_string(i) + " holds 2^31 bases or more");
    }
    if (n_reads > 0 && (!out || (!reads && read_off[n_reads] > read_off[0]))) return cf_fail(ctx, -22, "cf_tandem_scan: null reads or output");
    const int64_t batch_windows = ctx->tandem_batch_windows > 0 ? ctx->tandem_batch_windows : CF_TD_BATCH_WINDOWS;
    // batches: whole reads, up to batch_windows windows (one read at least), and — unless records are forced — only as many reads
    // as leave the keys 64 bits
    struct td_range { int64_t r0, r1; td_layout L; };
    std::vector<td_range> batches;
    for (int64_t r0 = 0; r0 < n_reads;) {
        int64_t r1 = r0, wins = 0, max_len = 0;
        bool fits = false;
        td_layout L{};
        while (r1 < n_reads) {
            const int64_t len = read_off[r1 + 1] - read_off[r1], w = std::max<int64_t>(len - k + 1, 0);
            if (r1 > r0 && wins + w > batch_windows) break;
            if (r1 - r0 >= ((int64_t)1 << 31) - 2) break;
            bool f = false;
            const td_layout cand = td_layout_of(k, r1 - r0 + 1, std::max(max_len, len), &f);
            if (r1 > r0 && fits && !f && ctx->tandem_key_mode != 2) break;      // this read would push the batch out of 64 bits
            L = cand; fits = f;
            wins += w; max_len = std::max(max_len, len);
            ++r1;
        }
        if (ctx->tandem_key_mode == 1 && !fits)
            return cf_fail(ctx, -22, "cf_tandem_scan: tandem_key_mode 1, but read " + std::to_string(r0) + " alone needs more than 64 key bits");
        if (ctx->tandem_key_mode == 2) L.mode = 2;
        batches.push_back({r0, r1, L});
        r0 = r1;
    }
    CF_HIP(hipSetDevice(ctx->device));
    td_events ev;
    for (auto& e : ev.e) CF_HIP(hipEventCreate(&e));
    std::vector<int64_t> hook_ptr(1, 0);
    std::vector<int32_t> hook_pos;
    cf_tandem_shape shape{};
    shape.n_reads = n_reads;
    for (const td_range& b : batches) {
        float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        hipEvent_t start = ctx->ev0, stop = ctx->ev1;
        CF_HIP(hipEventRecord(start, ctx->stream));
        // (on a failure the results of the call before stay)
        CF_TRY(td_batch(ctx, reads, read_off, b.r0, b.r1, k, 2 * (int64_t)bin_size, b.L, ev, out, hook_ptr, hook_pos, &shape.n_records, ms));
        CF_HIP(hipEventRecord(stop, ctx->stream));
        CF_HIP(hipEventSynchronize(stop));
        float all = 0.f;
        (void)hipEventElapsedTime(&all, start, stop);
        for (int i = 0; i < 5; ++i) shape.phase_ms[i] += ms[i];
        shape.phase_ms[5] += all;
        shape.key_mode = b.L.mode; shape.code_bits = b.L.code_bits; shape.read_bits = b.L.read_bits; shape.pos_bits = b.L.pos_bits;
        shape.pos_shift = b.L.pos_shift;
        ++shape.n_batches;
        if (b.L.mode == 1) ++shape.n_key_batches;
    }
    ctx->tandem_hook_ptr.swap(hook_ptr);
    ctx->tandem_hook_pos.swap(hook_pos);
    ctx->tandem_last = shape;
    return 0;
}

int cf_tandem_hook_positions(cf_ctx* ctx, int64_t* ptr, int32_t* pos, int64_t cap, int64_t* n_out) {
    if (!ctx) return -22;
    if (ctx->tandem_hook_ptr.empty()) return cf_fail(ctx, -22, "cf_tandem_hook_positions: no cf_tandem_scan before");
    const int64_t n = (int64_t)ctx->tandem_hook_pos.size();
    if (n_out) *n_out = n;
    if (!ptr && !pos) return 0;
    if (cap < n) return cf_fail(ctx, -22, "cf_tandem_hook_positions: room for " + std::to_string(cap) + " positions, " + std::to_string(n) + " needed");
    if (ptr) std::memcpy(ptr, ctx->tandem_hook_ptr.data(), ctx->tandem_hook_ptr.size() * 8);
    if (pos && n) std::memcpy(pos, ctx->tandem_hook_pos.data(), (size_t)n * 4);
    return 0;
}

}  // extern "C"
