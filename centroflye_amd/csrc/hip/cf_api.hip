// cf_api.hip — context management, hand-over of the packed reads, getters (C ABI: include/cfhip.h).
#include "cf_common.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>

#ifndef CF_COPY_MODE_DEFAULT
#define CF_COPY_MODE_DEFAULT 1      // auto: H2D of 64 MB and more through hipHostRegister, everything else staged (profiles/r05_copy_modes.log)
#endif
struct alignas(16) cf_u32x4_api { uint32_t x, y, z, w; };

int cf_fail(cf_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    return code;
}

// Work buffers are pooled per context, up to ctx->pool_max bytes (85 % of the device's memory: at 8 Gb of reads the two
// record arrays of A1 alone are 128 GB, and giving them back to the driver after every step cost 1.5 s per step).  A
// hipMalloc that fails flushes the pool and tries again, so a large pool never causes an out-of-memory error by itself.

// Several contexts may live on one device (session.engine() next to a ShardedRecruiter, tools that open more than one Engine):
// each keeps freed blocks for reuse, so a hipMalloc that fails flushes the pools of ALL contexts of that device before it gives
// up (round 2 flushed only the caller's: memory idle in a sibling's pool made the allocation fail).  One process-wide lock
// guards the registry and every pool operation (calls on ONE context are serialised by the caller; different contexts may be
// driven from different threads).
static std::mutex g_pool_lock;
static std::vector<cf_ctx*> g_contexts;

static void cf_pool_flush_locked(cf_ctx* ctx) {
    for (auto& kv : ctx->pool) { ctx->block_bytes.erase(kv.second); (void)hipFree(kv.second); }
    ctx->pool.clear();
    ctx->pooled = 0;
}
static void cf_pool_flush(cf_ctx* ctx) {
    std::lock_guard<std::mutex> g(g_pool_lock);
    cf_pool_flush_locked(ctx);
}

int cf_alloc(cf_ctx* ctx, void** p, size_t bytes, const char* what) {
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    const size_t want = (bytes + 255) & ~(size_t)255;
    std::lock_guard<std::mutex> g(g_pool_lock);
    // smallest pooled block that fits without wasting more than a quarter
    auto it = ctx->pool.lower_bound(want);
    if (it != ctx->pool.end() && it->first <= want + want / 4 + 4096) {
        *p = it->second;
        ctx->pooled -= it->first;
        ctx->pool.erase(it);
        ctx->live += bytes;
        return 0;
    }
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess || !*p) {          // give the pooled memory of every context of this device back and try once more
        (void)hipGetLastError();
        for (cf_ctx* c : g_contexts) if (c->device == ctx->device) cf_pool_flush_locked(c);
        cf_pool_flush_locked(ctx);
        e = hipMalloc(p, want);
    }
    if (e != hipSuccess || !*p) {
        *p = nullptr;
        return cf_fail(ctx, -12, std::string("hipMalloc of ") + std::to_string(bytes) + " bytes for " + what + ": " + hipGetErrorString(e));
    }
    ctx->block_bytes[*p] = want;
    ctx->live += bytes;
    return 0;
}

void cf_release(cf_ctx* ctx, void* p, size_t bytes) {
    if (!p) return;
    if (bytes == 0) bytes = 16;
    std::lock_guard<std::mutex> g(g_pool_lock);
    ctx->live -= bytes < ctx->live ? bytes : ctx->live;
    auto it = ctx->block_bytes.find(p);
    if (it == ctx->block_bytes.end() || ctx->pooled + it->second > ctx->pool_max) {
        if (it != ctx->block_bytes.end()) ctx->block_bytes.erase(it);
        (void)hipFree(p);
        return;
    }
    ctx->pool.emplace(it->second, p);
    ctx->pooled += it->second;
}

// ---------------------------------------------------------------------------------------------------------------
// Host hand-over.  The C ABI borrows plain host pointers (numpy arrays: pageable memory); a hipMemcpy from / to pageable
// memory runs at 10 - 25 GB/s on this platform (the runtime stages it through one bounce buffer on one thread: round 2
// measured 22 GB/s for 5.4 GB).  Here kCopyThreads threads each own a pinned slot and a stream: DMA into / out of the slot
// at PCIe speed, memcpy between the slot and the caller's buffer by the same thread, the threads overlapping each other
// (the first touch of a fresh output buffer — page faults — spreads over the threads as well).
static const size_t CF_PIN_SLOT = (size_t)8 << 20;
static const size_t CF_PIN_MIN = (size_t)4 << 20;      // below this a plain copy is as fast

static bool cf_pin_ready(cf_ctx* ctx) {
    if (ctx->pin_bytes) return true;
    for (int i = 0; i < cf_ctx::kCopyThreads; ++i) {
        if (hipHostMalloc(&ctx->pin_slot[i], CF_PIN_SLOT, 0) != hipSuccess || hipStreamCreate(&ctx->pin_stream[i]) != hipSuccess) {
            (void)hipGetLastError();
            for (int j = 0; j <= i; ++j) {
                if (ctx->pin_slot[j]) { (void)hipHostFree(ctx->pin_slot[j]); ctx->pin_slot[j] = nullptr; }
                if (ctx->pin_stream[j]) { (void)hipStreamDestroy(ctx->pin_stream[j]); ctx->pin_stream[j] = nullptr; }
            }
            return false;
        }
    }
    ctx->pin_bytes = CF_PIN_SLOT;
    return true;
}
static void cf_pin_free(cf_ctx* ctx) {
    for (int i = 0; i < cf_ctx::kCopyThreads; ++i) {
        if (ctx->pin_slot[i]) { (void)hipHostFree(ctx->pin_slot[i]); ctx->pin_slot[i] = nullptr; }
        if (ctx->pin_stream[i]) { (void)hipStreamDestroy(ctx->pin_stream[i]); ctx->pin_stream[i] = nullptr; }
    }
    ctx->pin_bytes = 0;
}
static bool cf_is_host_pointer(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return true; }      // unknown to the runtime: ordinary host memory
    return at.type != hipMemoryTypeDevice;
}
// One DMA straight from / into the caller's pages: hipHostRegister pins them for the length of the copy (round 5, VERDICT round 4
// item 7).  Which way is faster depends on the host (pinning costs page-table work per 4-KB page; the staged path costs a memcpy
// through the pinned slots on copy_threads cores): CF_COPY_MODE = "staged" | "register" | "auto" (register from CF_REG_MIN bytes on);
// a registration that fails (locked-memory limit, memory that cannot be pinned) falls back to the staged path.
static const size_t CF_REG_MIN = (size_t)64 << 20;
static int cf_copy_mode() {      // 0 staged, 1 register (from CF_REG_MIN on), 2 register whatever the size above CF_PIN_MIN
    static const int mode = [] {
        const char* e = std::getenv("CF_COPY_MODE");
        if (!e || !*e) return CF_COPY_MODE_DEFAULT;
        return !std::strcmp(e, "staged") ? 0 : !std::strcmp(e, "register") ? 2 : 1;
    }();
    return mode;
}
static int cf_copy_registered(cf_ctx* ctx, void* dst, const void* src, size_t bytes, bool to_device) {
    void* host = to_device ? const_cast<void*>(src) : dst;
    if (hipHostRegister(host, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return 1; }
    hipError_t e = hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipHostUnregister(host);
    if (e != hipSuccess) { (void)hipGetLastError(); return cf_fail(ctx, -5, std::string("registered host copy: ") + hipGetErrorString(e)); }
    return 0;
}
static int cf_copy_staged(cf_ctx* ctx, void* dst, const void* src, size_t bytes, bool to_device) {
    const void* host = to_device ? src : dst;
    if (bytes < CF_PIN_MIN || !cf_is_host_pointer(host) || !cf_pin_ready(ctx)) {
        CF_HIP(hipStreamSynchronize(ctx->stream));
        CF_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
        return 0;
    }
    CF_HIP(hipStreamSynchronize(ctx->stream));      // what the copy reads / overwrites is settled
    // measured on an MI355X box (gpurun_out/c1_copy_modes.log, 0.4 GB of reads / 4 GB of edge rows): H2D 52.7 GB/s registered against 34.9
    // (8 copy threads) / 46.8 (16) staged; D2H 12.9 - 29 GB/s registered (pinning the fresh pages of an output buffer costs more than
    // the copy) against 54 staged with 16 threads.  So "auto" registers host memory for H2D only.
    if (cf_copy_mode() == 2 || (cf_copy_mode() == 1 && to_device && bytes >= CF_REG_MIN)) {
        const int rc = cf_copy_registered(ctx, dst, src, bytes, to_device);
        if (rc <= 0) return rc;      // 1: could not pin — the staged path below
    }
    const size_t n_chunks = (bytes + CF_PIN_SLOT - 1) / CF_PIN_SLOT;
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    auto work = [&](int t) {
        if (hipSetDevice(ctx->device) != hipSuccess) { bad = 1; return; }
        char* slot = (char*)ctx->pin_slot[t];
        for (;;) {
            const size_t c = next.fetch_add(1);
            if (c >= n_chunks || bad.load()) return;
            const size_t off = c * CF_PIN_SLOT, n = std::min(CF_PIN_SLOT, bytes - off);
            if (to_device) {
                std::memcpy(slot, (const char*)src + off, n);
                if (hipMemcpyAsync((char*)dst + off, slot, n, hipMemcpyHostToDevice, ctx->pin_stream[t]) != hipSuccess ||
                    hipStreamSynchronize(ctx->pin_stream[t]) != hipSuccess) { bad = 1; return; }
            } else {
                if (hipMemcpyAsync(slot, (const char*)src + off, n, hipMemcpyDeviceToHost, ctx->pin_stream[t]) != hipSuccess ||
                    hipStreamSynchronize(ctx->pin_stream[t]) != hipSuccess) { bad = 1; return; }
                std::memcpy((char*)dst + off, slot, n);
            }
        }
    };
    const int nt = (int)std::min<size_t>((size_t)ctx->copy_threads, n_chunks);      // (CF_COPY_THREADS, read once by cf_create)
    std::vector<std::thread> th;
    try {
        for (int t = 1; t < nt; ++t) th.emplace_back(work, t);
    } catch (...) { /* fewer threads: the others take the chunks */ }
    work(0);
    for (auto& x : th) x.join();
    if (bad.load()) { (void)hipGetLastError(); return cf_fail(ctx, -5, "staged host copy failed"); }
    return 0;
}
int cf_copy_h2d(cf_ctx* ctx, void* dev, const void* host, size_t bytes) { return bytes ? cf_copy_staged(ctx, dev, host, bytes, true) : 0; }
int cf_copy_d2h(cf_ctx* ctx, void* host, const void* dev, size_t bytes) { return bytes ? cf_copy_staged(ctx, host, dev, bytes, false) : 0; }

// Alphabet check of the RESIDENT bases (round 5: the copy threads of rounds 3-4 looked at every chunk on the host side — a second
// pass of every byte through a core's vector units next to the memcpy): one device pass, 16 bytes per lane and load, over memory
// that runs at terabytes per second.  flag := 1 when some byte is not an upper-case A, C, G or T.
__global__ void __launch_bounds__(256)
cf_alphabet_kernel(const uint8_t* __restrict__ bases, int64_t n, unsigned int* __restrict__ flag) {
    const int64_t n16 = n >> 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const cf_u32x4_api w = *(const cf_u32x4_api*)(bases + 16 * i);      // (d_bases is 256-byte aligned)
        const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // a byte is A (0x41), C (0x43), G (0x47) or T (0x54): the 2-bit code's letter must be the byte itself
            const uint32_t code = ((v[j] >> 1) ^ (v[j] >> 2)) & 0x03030303u;
            const uint32_t letters = 0x54474341u;      // "ACGT", least significant byte first
            uint32_t back = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) back |= ((letters >> (8 * ((code >> (8 * b)) & 3u))) & 0xFFu) << (8 * b);
            bad |= back ^ v[j];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 15)) bad |= cf_is_acgt(bases[(n16 << 4) + threadIdx.x]) ? 0u : 1u;
    if (bad) *flag = 1u;
}
static int cf_check_alphabet(cf_ctx* ctx, const uint8_t* d_bases, int64_t n, bool* exotic) {
    *exotic = false;
    if (n <= 0) return 0;
    cf_scratch tmp(ctx);
    unsigned int* d_flag = nullptr;
    CF_TRY(tmp.get(&d_flag, 4, "alphabet flag"));
    unsigned int h = 0;
    CF_HIP(hipMemsetAsync(d_flag, 0, 16, ctx->stream));
    hipLaunchKernelGGL(cf_alphabet_kernel, dim3((unsigned)cf_grid_for((n >> 4) + 1, 256, std::max(1, ctx->n_cu) * 16)), dim3(256), 0, ctx->stream, d_bases, n, d_flag);
    CF_KERNEL_CHECK("cf_alphabet_kernel");
    CF_HIP(hipMemcpyAsync(&h, d_flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    CF_HIP(hipStreamSynchronize(ctx->stream));
    *exotic = h != 0;
    return 0;
}

static void free_reads(cf_ctx* c) {
    cf_release_t(c, c->d_bases, (size_t)c->n_bases);
    cf_release_t(c, c->d_read_off, (size_t)c->n_reads + 1);
}
static void free_units(cf_ctx* c) {
    cf_release_t(c, c->d_unit_ptr, (size_t)c->n_reads + 1);
    cf_release_t(c, c->d_unit_start, (size_t)c->n_units);
    cf_release_t(c, c->d_unit_end, (size_t)c->n_units);
}
void cf_free_table(cf_ctx* c) {
    if (c->d_table) { cf_release(c, c->d_table, (size_t)c->table_alloc * sizeof(cf_slot)); c->d_table = nullptr; }
    c->table_cap = 0; c->table_alloc = 0; c->table_dense = false;
}
void cf_free_kmers(cf_ctx* c) {
    cf_release_t(c, c->d_kmers, (size_t)c->n_kmers);
    cf_release_t(c, c->d_lut, (size_t)c->lut_cap);
    cf_release_t(c, c->d_lut_pre, (size_t)c->lut_pre_words);
    cf_release_t(c, c->d_unique_bits, (size_t)c->unique_words);
    c->n_kmers = 0; c->lut_cap = 0; c->lut_pre_words = 0; c->unique_words = 0;
}
void cf_free_gview(cf_ctx* c);   // cf_exchange.hip
void cf_free_contig(cf_ctx* c);  // cf_map.hip
void cf_free_clouds(cf_ctx* c) {
    cf_free_gview(c);           // the all-gathered view is derived from the local clouds
    cf_free_contig(c);          // and so is the frozen contig
    cf_release_t(c, c->d_cloud_ptr, (size_t)c->n_units + 1);
    cf_release_t(c, c->d_entries, (size_t)c->n_entries);
    c->n_entries = 0; c->have_clouds = false;
    c->cloud_max_entries = -1; c->read_max_entries = -1;
}
void cf_free_edges(cf_ctx* c) {
    cf_release_t(c, c->d_edges, (size_t)c->edge_cap * 4);
    c->edge_cap = 0; c->n_edges_stored = 0;
}

void cf_comm_apply_params(cf_ctx* ctx);   // cf_exchange.hip

extern "C" {

int cf_create(int device, cf_ctx** out) {
    if (!out) return -22;
    *out = nullptr;
    cf_ctx* ctx = new (std::nothrow) cf_ctx();
    if (!ctx) return -12;
    *out = ctx;  // returned even on failure so the caller can read the error
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return cf_fail(ctx, -19, "no HIP device visible (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return cf_fail(ctx, -22, "device index out of range");
    ctx->device = device;
    CF_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    CF_HIP(hipGetDeviceProperties(&prop, device));
    ctx->n_cu = prop.multiProcessorCount;
    ctx->pool_max = std::max<size_t>((size_t)1 << 30, (size_t)((double)prop.totalGlobalMem * 0.85));
    if (const char* ev = std::getenv("CF_COPY_THREADS")) ctx->copy_threads = std::max(1, std::min((int)cf_ctx::kCopyThreads, std::atoi(ev)));
    ctx->hbm_total = (int64_t)prop.totalGlobalMem;
    CF_HIP(hipStreamCreate(&ctx->stream));
    CF_HIP(hipEventCreate(&ctx->ev0));
    CF_HIP(hipEventCreate(&ctx->ev1));
    CF_HIP(hipEventCreate(&ctx->ev2));
    CF_HIP(hipEventCreate(&ctx->ev3));
    { std::lock_guard<std::mutex> g(g_pool_lock); g_contexts.push_back(ctx); }
    return 0;
}

void cf_destroy(cf_ctx* ctx) {
    if (!ctx) return;
    { std::lock_guard<std::mutex> g(g_pool_lock); g_contexts.erase(std::remove(g_contexts.begin(), g_contexts.end(), ctx), g_contexts.end()); }
    (void)hipSetDevice(ctx->device);
    (void)cf_comm_free(ctx);
    cf_edit_free(ctx);
    cf_free_edges(ctx);
    cf_free_clouds(ctx);
    cf_free_kmers(ctx);
    cf_free_table(ctx);
    free_units(ctx);
    free_reads(ctx);
    cf_pool_flush(ctx);
    cf_pin_free(ctx);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
    if (ctx->ev3) (void)hipEventDestroy(ctx->ev3);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* cf_last_error(const cf_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int cf_device_info(cf_ctx* ctx, char* name, int name_len, int64_t* hbm_bytes, int32_t* n_cu) {
    if (!ctx) return -22;
    hipDeviceProp_t prop;
    CF_HIP(hipGetDeviceProperties(&prop, ctx->device));
    if (name && name_len > 0) std::snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    if (n_cu) *n_cu = prop.multiProcessorCount;
    return 0;
}

static int load_units(cf_ctx* ctx, const int64_t* unit_ptr, const int64_t* unit_start, const int64_t* unit_end) {
    const int64_t R = ctx->n_reads;
    if (unit_ptr[0] != 0) return cf_fail(ctx, -22, "unit_ptr[0] must be 0");
    for (int64_t r = 0; r < R; ++r)
        if (unit_ptr[r + 1] < unit_ptr[r]) return cf_fail(ctx, -22, "unit_ptr must be non-decreasing");
    const int64_t U = unit_ptr[R];
    if (U >= (int64_t)1 << 31) return cf_fail(ctx, -22, "more than 2^31 units");
    int64_t longest = 0;
    for (int64_t r = 0; r < R; ++r) {
        for (int64_t u = unit_ptr[r]; u < unit_ptr[r + 1]; ++u) {
            if (unit_start[u] < ctx->h_read_off[(size_t)r] || unit_end[u] > ctx->h_read_off[(size_t)r + 1] || unit_end[u] < unit_start[u])
                return cf_fail(ctx, -22, "unit " + std::to_string(u) + " lies outside its read");
            longest = std::max(longest, unit_end[u] - unit_start[u]);
        }
    }
    ctx->max_unit_len = longest;
    cf_free_clouds(ctx);
    free_units(ctx);
    ctx->n_units = U;
    ctx->h_unit_ptr.assign(unit_ptr, unit_ptr + R + 1);
    CF_TRY(cf_alloc_t(ctx, &ctx->d_unit_ptr, (size_t)R + 1, "unit_ptr"));
    CF_TRY(cf_alloc_t(ctx, &ctx->d_unit_start, (size_t)U, "unit_start"));
    CF_TRY(cf_alloc_t(ctx, &ctx->d_unit_end, (size_t)U, "unit_end"));
    CF_HIP(hipMemcpyAsync(ctx->d_unit_ptr, unit_ptr, (size_t)(R + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (U) {
        CF_HIP(hipMemcpyAsync(ctx->d_unit_start, unit_start, (size_t)U * 8, hipMemcpyHostToDevice, ctx->stream));
        CF_HIP(hipMemcpyAsync(ctx->d_unit_end, unit_end, (size_t)U * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    CF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stats.n_units = U;
    return 0;
}

int cf_load_reads(cf_ctx* ctx, const uint8_t* bases, const int64_t* read_off, int64_t n_reads,
                  const int64_t* unit_ptr, const int64_t* unit_start, const int64_t* unit_end) {
    if (!ctx) return -22;
    if (!read_off || n_reads < 0 || !unit_ptr) return cf_fail(ctx, -22, "cf_load_reads: null argument");
    if (n_reads >= (int64_t)1 << 31) return cf_fail(ctx, -22, "more than 2^31 reads");
    if (read_off[0] != 0) return cf_fail(ctx, -22, "read_off[0] must be 0");
    for (int64_t r = 0; r < n_reads; ++r)
        if (read_off[r + 1] < read_off[r]) return cf_fail(ctx, -22, "read_off must be non-decreasing");
    const int64_t nb = read_off[n_reads];
    if (nb > 0 && !bases) return cf_fail(ctx, -22, "cf_load_reads: null bases");
    // alphabet (never silently 2-bit-encode other symbols): windows that hold anything but
    // upper-case A, C, G, T are skipped by cf_count_kmers (they have no code; the reference counts them as strings of their
    // own — the host keeps that side: cfh_exotic_summary), and cf_build_clouds upper-cases a, c, g, t as the reference does
    bool exotic = false;      // (found out by a device pass over the resident bases below; every argument check stands above this
                              // line — ADVICE round 4: nothing of the previous state is freed before the arguments are known to be good)
    CF_HIP(hipSetDevice(ctx->device));
    CF_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    cf_free_edges(ctx);
    cf_free_clouds(ctx);
    cf_free_table(ctx);
    free_units(ctx);
    free_reads(ctx);
    ctx->n_reads = n_reads;
    ctx->n_bases = nb;
    ctx->h_read_off.assign(read_off, read_off + n_reads + 1);
    CF_TRY(cf_alloc_t(ctx, &ctx->d_bases, (size_t)nb + 64, "bases"));
    // note: d_bases was allocated with +64 slack; account it under n_bases for release (reads without bases — hand-made clouds — are
    // released as the 16 bytes cf_release takes for an empty buffer: counted as 64 here, every such load took 16 bytes off hbm_bytes_live)
    ctx->live -= nb ? 64 : 48;
    CF_TRY(cf_alloc_t(ctx, &ctx->d_read_off, (size_t)n_reads + 1, "read_off"));
    ctx->has_exotic = false;
    CF_TRY(cf_copy_h2d(ctx, ctx->d_bases, bases, (size_t)nb));      // (host or device memory: cf_copy_staged tells them apart)
    CF_TRY(cf_check_alphabet(ctx, ctx->d_bases, nb, &exotic));
    ctx->has_exotic = exotic;
    CF_HIP(hipMemcpyAsync(ctx->d_read_off, read_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    CF_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stats = cf_stats{};
    ctx->stats.n_reads = n_reads;
    ctx->stats.n_bases = nb;
    CF_TRY(load_units(ctx, unit_ptr, unit_start, unit_end));
    CF_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    CF_HIP(hipEventSynchronize(ctx->ev1));
    CF_HIP(hipEventElapsedTime(&ctx->times.load_ms, ctx->ev0, ctx->ev1));
    return 0;
}

int cf_load_units(cf_ctx* ctx, const int64_t* unit_ptr, const int64_t* unit_start, const int64_t* unit_end) {
    if (!ctx) return -22;
    if (!ctx->d_read_off) return cf_fail(ctx, -22, "cf_load_units: no reads loaded");
    CF_HIP(hipSetDevice(ctx->device));
    return load_units(ctx, unit_ptr, unit_start, unit_end);
}

int cf_get_kmers(cf_ctx* ctx, uint64_t* out, int64_t cap) {
    if (!ctx) return -22;
    if (cap < ctx->n_kmers) return cf_fail(ctx, -22, "cf_get_kmers: buffer too small");
    CF_TRY(cf_copy_d2h(ctx, out, ctx->d_kmers, (size_t)ctx->n_kmers * 8));
    return 0;
}

int cf_get_clouds(cf_ctx* ctx, int64_t* cloud_ptr, int32_t* entries, int64_t cap) {
    if (!ctx) return -22;
    if (!ctx->have_clouds) return cf_fail(ctx, -22, "cf_get_clouds: no clouds built");
    if (cap < ctx->n_entries) return cf_fail(ctx, -22, "cf_get_clouds: buffer too small");
    CF_TRY(cf_copy_d2h(ctx, cloud_ptr, ctx->d_cloud_ptr, (size_t)(ctx->n_units + 1) * 8));
    CF_TRY(cf_copy_d2h(ctx, entries, ctx->d_entries, (size_t)ctx->n_entries * 4));
    return 0;
}

int cf_set_clouds(cf_ctx* ctx, const int64_t* cloud_ptr, const int32_t* entries, int64_t n_entries) {
    if (!ctx) return -22;
    if (!ctx->d_unit_ptr) return cf_fail(ctx, -22, "cf_set_clouds: no units loaded");
    CF_HIP(hipSetDevice(ctx->device));
    cf_free_clouds(ctx);
    CF_TRY(cf_alloc_t(ctx, &ctx->d_cloud_ptr, (size_t)ctx->n_units + 1, "cloud_ptr"));
    ctx->n_entries = n_entries;
    CF_TRY(cf_alloc_t(ctx, &ctx->d_entries, (size_t)n_entries, "cloud entries"));
    CF_TRY(cf_copy_h2d(ctx, ctx->d_cloud_ptr, cloud_ptr, (size_t)(ctx->n_units + 1) * 8));
    CF_TRY(cf_copy_h2d(ctx, ctx->d_entries, entries, (size_t)n_entries * 4));
    // caller-made clouds are not bounded by the length of their units: the placement's packed counters (cf_place2_fits) go by what
    // is installed
    int64_t cloud_max = 0, read_max = 0;
    for (int64_t u = 0; u < ctx->n_units; ++u) cloud_max = std::max(cloud_max, cloud_ptr[u + 1] - cloud_ptr[u]);
    if ((int64_t)ctx->h_unit_ptr.size() == ctx->n_reads + 1)
        for (int64_t r = 0; r < ctx->n_reads; ++r) read_max = std::max(read_max, cloud_ptr[ctx->h_unit_ptr[(size_t)r + 1]] - cloud_ptr[ctx->h_unit_ptr[(size_t)r]]);
    else read_max = n_entries;
    ctx->cloud_max_entries = cloud_max; ctx->read_max_entries = read_max;
    ctx->have_clouds = true;
    ctx->stats.n_cloud_entries = n_entries;
    return 0;
}

int cf_get_edges(cf_ctx* ctx, uint32_t* out, int64_t cap) {
    if (!ctx) return -22;
    const int64_t n = std::min(cap, ctx->n_edges_stored);      // the first min(cap, stored) edges
    if (n < 0 || (n && !out)) return cf_fail(ctx, -22, "cf_get_edges: bad buffer");
    CF_HIP(hipSetDevice(ctx->device));
    CF_TRY(cf_copy_d2h(ctx, out, ctx->d_edges, (size_t)n * 16));
    return 0;
}

int cf_sort_edges(cf_ctx* ctx) {
    if (!ctx) return -22;
    const int64_t n = ctx->n_edges_stored;
    if (n <= 1) return 0;
    cf_scratch tmp(ctx);
    uint32_t* d_tmp = nullptr;
    CF_TRY(tmp.get(&d_tmp, (size_t)n * 4, "edge sort scratch"));
    int kbits = 1;
    while (kbits < 32 && ((int64_t)1 << kbits) < std::max<int64_t>(ctx->n_kmers, 2)) ++kbits;
    const int words[3] = {2, 1, 0}, bits[3] = {kbits, kbits, 16};      // b, then a, then d (<= 65535)
    return cf_radix_sort_rec16(ctx, ctx->d_edges, d_tmp, n, words, bits, 3);
}

int cf_get_stats(cf_ctx* ctx, cf_stats* out) {
    if (!ctx || !out) return -22;
    ctx->stats.hbm_bytes_live = (int64_t)ctx->live;
    ctx->stats.table_capacity = (int64_t)ctx->table_cap;
    ctx->stats.n_kmers = ctx->n_kmers;
    ctx->stats.n_edges_stored = ctx->n_edges_stored;
    *out = ctx->stats;
    return 0;
}

int cf_get_times(cf_ctx* ctx, cf_times* out) {
    if (!ctx || !out) return -22;
    *out = ctx->times;
    return 0;
}

// The knobs: cf_knobs.h as one entry per name, and the three entry points that go through them.
static inline bool cf_in(int64_t v, int64_t lo, int64_t hi) { return lo <= v && v <= hi; }
struct cf_knob {
    const char* name;
    const char* refusal;
    bool (*accepted)(int64_t v);
    void (*store)(cf_ctx* ctx, int64_t v);
    int64_t (*load)(const cf_ctx* ctx);
};
#define CF_KNOB_ENTRY(name, type, def, accepted, stored, refusal) \
    {#name, refusal, [](int64_t v) -> bool { (void)v; return accepted; }, [](cf_ctx* ctx, int64_t v) { ctx->name = stored; }, [](const cf_ctx* ctx) -> int64_t { return ctx->name; }},
static const cf_knob cf_knobs[] = {
#define CF_KNOB CF_KNOB_ENTRY
#define CF_KNOB_AB(...)
#include "cf_knobs.h"
#undef CF_KNOB
#undef CF_KNOB_AB
};
static const cf_knob cf_ab_knobs[] = {      // the A/B switches: found by name, not listed by cf_param_name
#define CF_KNOB(...)
#define CF_KNOB_AB CF_KNOB_ENTRY
#include "cf_knobs.h"
#undef CF_KNOB
#undef CF_KNOB_AB
};
static const int cf_n_knobs = (int)(sizeof(cf_knobs) / sizeof(cf_knobs[0]));

static const cf_knob* cf_find_knob(cf_ctx* ctx, const char* name) {
    for (const cf_knob& k : cf_knobs)
        if (!std::strcmp(k.name, name)) return &k;
    for (const cf_knob& k : cf_ab_knobs)
        if (!std::strcmp(k.name, name)) return &k;
    cf_fail(ctx, -22, std::string("unknown parameter ") + name);
    return nullptr;
}

int cf_set_param(cf_ctx* ctx, const char* name, int64_t value) {
    if (!ctx || !name) return -22;
    const cf_knob* k = cf_find_knob(ctx, name);
    if (!k) return -22;
    if (!k->accepted(value)) return cf_fail(ctx, -22, k->refusal);
    k->store(ctx, value);
    if (!std::strncmp(name, "comm_", 5)) cf_comm_apply_params(ctx);      // the transport keeps its own copy of its knobs
    return 0;
}

int cf_get_param(cf_ctx* ctx, const char* name, int64_t* value) {
    if (!ctx || !name || !value) return -22;
    const cf_knob* k = cf_find_knob(ctx, name);
    if (!k) return -22;
    *value = k->load(ctx);
    return 0;
}

const char* cf_param_name(int32_t index) { return index >= 0 && index < cf_n_knobs ? cf_knobs[index].name : nullptr; }

int cf_selftest_sort(cf_ctx* ctx, const uint64_t* keys, int64_t n, int32_t bits, uint64_t* out) {
    if (!ctx) return -22;
    CF_HIP(hipSetDevice(ctx->device));
    cf_scratch tmp(ctx);
    unsigned long long *a = nullptr, *b = nullptr;
    CF_TRY(tmp.get(&a, (size_t)n, "selftest keys"));
    CF_TRY(tmp.get(&b, (size_t)n, "selftest tmp"));
    if (n && hipMemcpy(a, keys, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) return cf_fail(ctx, -5, "selftest copy");
    CF_TRY(cf_radix_sort_u64(ctx, a, b, n, bits));
    if (n && hipMemcpy(out, a, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return cf_fail(ctx, -5, "selftest copy back");
    return 0;
}

int cf_selftest_scan(cf_ctx* ctx, const int64_t* in, int64_t n, int64_t* out) {
    if (!ctx) return -22;
    CF_HIP(hipSetDevice(ctx->device));
    cf_scratch tmp(ctx);
    int64_t *a = nullptr, *b = nullptr;
    CF_TRY(tmp.get(&a, (size_t)n + 1, "selftest in"));
    CF_TRY(tmp.get(&b, (size_t)n + 1, "selftest out"));
    int64_t total = 0;
    if (n && hipMemcpy(a, in, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) return cf_fail(ctx, -5, "selftest copy");
    CF_TRY(cf_scan_exclusive_i64(ctx, a, b, n, &total));
    if (n && hipMemcpy(out, b, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return cf_fail(ctx, -5, "selftest copy back");
    out[n] = total;
    return 0;
}

// the same with one device buffer as input and output, as cf_count.hip and cf_exchange.hip call the scan
int cf_selftest_scan_inplace(cf_ctx* ctx, const int64_t* in, int64_t n, int64_t* out) {
    if (!ctx) return -22;
    CF_HIP(hipSetDevice(ctx->device));
    cf_scratch tmp(ctx);
    int64_t* a = nullptr;
    CF_TRY(tmp.get(&a, (size_t)n + 1, "selftest in and out"));
    int64_t total = 0;
    if (n && hipMemcpy(a, in, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) return cf_fail(ctx, -5, "selftest copy");
    CF_TRY(cf_scan_exclusive_i64(ctx, a, a, n, &total));
    if (n && hipMemcpy(out, a, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return cf_fail(ctx, -5, "selftest copy back");
    out[n] = total;
    return 0;
}

int cf_selftest_scan_u32(cf_ctx* ctx, const uint32_t* in, int64_t n, int64_t* out) {
    if (!ctx) return -22;
    CF_HIP(hipSetDevice(ctx->device));
    cf_scratch tmp(ctx);
    uint32_t* a = nullptr;
    int64_t* b = nullptr;
    CF_TRY(tmp.get(&a, (size_t)n + 1, "selftest in"));
    CF_TRY(tmp.get(&b, (size_t)n + 1, "selftest out"));
    int64_t total = 0;
    if (n && hipMemcpy(a, in, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) return cf_fail(ctx, -5, "selftest copy");
    CF_TRY(cf_scan_exclusive_u32_to_i64(ctx, a, b, n, &total));
    if (n && hipMemcpy(out, b, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return cf_fail(ctx, -5, "selftest copy back");
    out[n] = total;
    return 0;
}

int cf_selftest_sort_rec16(cf_ctx* ctx, const uint32_t* recs, int64_t n, const int32_t* words, const int32_t* bits, int32_t n_fields, uint32_t* out) {
    if (!ctx) return -22;
    if (n < 0 || n_fields < 0 || n_fields > 16 || (n_fields && (!words || !bits))) return cf_fail(ctx, -22, "cf_selftest_sort_rec16: bad field list");
    int w[16], b[16];
    for (int f = 0; f < n_fields; ++f) {
        if (words[f] < 0 || words[f] > 3 || bits[f] < 0 || bits[f] > 32) return cf_fail(ctx, -22, "cf_selftest_sort_rec16: a field is a word 0 .. 3 and 0 .. 32 bits");
        w[f] = words[f];
        b[f] = bits[f];
    }
    CF_HIP(hipSetDevice(ctx->device));
    cf_scratch tmp(ctx);
    uint32_t *a = nullptr, *t = nullptr;
    CF_TRY(tmp.get(&a, (size_t)n * 4 + 4, "selftest records"));
    CF_TRY(tmp.get(&t, (size_t)n * 4 + 4, "selftest tmp"));
    if (n && hipMemcpy(a, recs, (size_t)n * 16, hipMemcpyHostToDevice) != hipSuccess) return cf_fail(ctx, -5, "selftest copy");
    CF_TRY(cf_radix_sort_rec16(ctx, a, t, n, w, b, n_fields));
    if (n && hipMemcpy(out, a, (size_t)n * 16, hipMemcpyDeviceToHost) != hipSuccess) return cf_fail(ctx, -5, "selftest copy back");
    return 0;
}

int cf_selftest_digit_offsets(cf_ctx* ctx, const uint32_t* hist, int32_t n_tiles, int32_t D, int64_t* offs, int64_t* total) {
    if (!ctx) return -22;
    if (n_tiles < 0) return cf_fail(ctx, -22, "cf_selftest_digit_offsets: negative tile count");
    CF_HIP(hipSetDevice(ctx->device));
    const size_t dd = (size_t)std::max(D, 1), nh = (size_t)n_tiles * dd, nc = (size_t)cf_tile_digit_chunks(n_tiles) * dd;
    cf_scratch tmp(ctx);
    uint32_t *d_hist = nullptr, *d_part = nullptr;
    int64_t *d_offs = nullptr, *d_base = nullptr, *d_total = nullptr;
    CF_TRY(tmp.get(&d_hist, nh + 1, "selftest histogram"));
    CF_TRY(tmp.get(&d_offs, nh + 1, "selftest offsets"));
    CF_TRY(tmp.get(&d_part, nc + 1, "selftest column sums"));
    CF_TRY(tmp.get(&d_base, nc + 1, "selftest column bases"));
    if (total) CF_TRY(tmp.get(&d_total, 1, "selftest total"));
    const bool run = D >= 1 && nh > 0;               // a refused D copies nothing
    if (run && hipMemcpy(d_hist, hist, nh * 4, hipMemcpyHostToDevice) != hipSuccess) return cf_fail(ctx, -5, "selftest copy");
    if (run && hipMemcpy(d_offs, offs, nh * 8, hipMemcpyHostToDevice) != hipSuccess) return cf_fail(ctx, -5, "selftest copy");   // (what the call leaves alone comes back as it went in)
    if (total && hipMemcpy(d_total, total, 8, hipMemcpyHostToDevice) != hipSuccess) return cf_fail(ctx, -5, "selftest copy");
    CF_TRY(cf_tile_digit_offsets(ctx, d_hist, n_tiles, D, d_offs, d_total, d_part, d_base));
    CF_HIP(hipStreamSynchronize(ctx->stream));
    if (run && hipMemcpy(offs, d_offs, nh * 8, hipMemcpyDeviceToHost) != hipSuccess) return cf_fail(ctx, -5, "selftest copy back");
    if (total && hipMemcpy(total, d_total, 8, hipMemcpyDeviceToHost) != hipSuccess) return cf_fail(ctx, -5, "selftest copy back");
    return 0;
}

}  // extern "C"
