// fanout.hip -- the user-space stage of one NUTS broadcast, as a gfx950 kernel.
//
// What write_room_except + write_user do for every listener before write(2) (nuts333.c:1315-1365,
// 1410-1415; restated on the CPU by oracle/nuts_path.c np_fanout_admits / np_write_user_stream):
// decide whether the listener is admitted, then run the shared text through the 1000-byte staging
// buffer and the colour-markup transducer, and cut the output into the chunks the reference hands
// to write(2).  Nothing here issues a system call; the output is one packed byte arena plus the
// packed chunk sizes, byte-exact and boundary-exact with the restatement.
//
// Work is a batch of items: (text offset, text length, colour bit) plus, in broadcast mode, a
// listener record.  One lane per item, because the flush rule depends on the running position.
//   pass 1  nuts_fanout_measure_{batch,broadcast}: admit flag, output bytes, write count per item
//   scan    hipcub DeviceScan::ExclusiveSum of bytes (int64) and write counts (int32)
//   pass 2  nuts_fanout_emit_{batch,broadcast}: bytes into the arena, chunk sizes into write_sizes
// In broadcast mode every item reads the same text, which each block stages in LDS once.
//
// Hard bounds per item of a text of len < 2000 bytes: 6*len + 4 output bytes (a '\n' with colour
// on is the costliest input byte, plus the trailing reset) and 16 writes.  The host sizes its buffers
// by them; pass 2 never writes past the counts pass 1 measured for its own item.
//
// C ABI at the bottom; built with
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC fanout.hip -o _build/libnuts_device.so

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <chrono>
#include <cstdint>
#include <cstdio>

namespace {

constexpr int kOutBuff = 1000;    // nuts333.h:16 OUT_BUFF_SIZE, the write_user staging buffer
constexpr int kTextSize = 2000;   // nuts333.h:280 text[ARR_SIZE*2]: the longest text is 1999 bytes
constexpr int kNumCols = 21;      // nuts333.h:21
constexpr int kMaxWrites = 16;    // hard bound on write(2) calls per item (worst case is 14)
constexpr int kBlock = 256;

// Listener record, one byte: the six fields of struct np_listener, then the colour bit.
constexpr uint8_t kLogin = 1, kHasRoom = 2, kSameRoom = 4, kIgnall = 8, kIgnshout = 16, kSender = 32, kColour = 64;
constexpr int kComShout = 4, kComSemote = 7;    // enum np_com: NP_SHOUT, NP_SEMOTE (nuts333.h:157-201)

// nuts333.h:249-255 two-letter commands, nuts333.h:237-246 their ANSI sequences (ESC [ ... m)
__constant__ char kColCom[kNumCols][2] = {
    {'R', 'S'}, {'O', 'L'}, {'U', 'L'}, {'L', 'I'}, {'R', 'V'}, {'F', 'K'}, {'F', 'R'}, {'F', 'G'}, {'F', 'Y'}, {'F', 'B'},
    {'F', 'M'}, {'F', 'T'}, {'F', 'W'}, {'B', 'K'}, {'B', 'R'}, {'B', 'G'}, {'B', 'Y'}, {'B', 'B'}, {'B', 'M'}, {'B', 'T'},
    {'B', 'W'},
};
// the bytes between "ESC[" and "m": "0" "1" "4" "5" "7" "30".."37" "40".."47"
__constant__ char kColArg[kNumCols][2] = {
    {'0', 0}, {'1', 0}, {'4', 0}, {'5', 0}, {'7', 0}, {'3', '0'}, {'3', '1'}, {'3', '2'}, {'3', '3'}, {'3', '4'},
    {'3', '5'}, {'3', '6'}, {'3', '7'}, {'4', '0'}, {'4', '1'}, {'4', '2'}, {'4', '3'}, {'4', '4'}, {'4', '5'}, {'4', '6'},
    {'4', '7'},
};

// np_fanout_admits (nuts333.c:1410-1415)
__device__ __forceinline__ bool admits(uint8_t l, int rm_is_null, int force_listen, int com_num)
{
    if (l & kLogin) return false;
    if (!(l & kHasRoom)) return false;
    if (!(l & kSameRoom) && !rm_is_null) return false;
    if ((l & kIgnall) && !force_listen) return false;
    if ((l & kIgnshout) && (com_num == kComShout || com_num == kComSemote)) return false;
    if (l & kSender) return false;
    return true;
}

__device__ __forceinline__ int colcom_at(const uint8_t* s, int i, int len)
{
    if (i + 2 >= len) return -1;
    const uint8_t a = s[i + 1], b = s[i + 2];
    for (int c = 0; c < kNumCols; c++)
        if (a == (uint8_t)kColCom[c][0] && b == (uint8_t)kColCom[c][1]) return c;
    return -1;
}

// Output sink: counts only (pass 1) or also stores (pass 2).  Stores are clamped to what pass 1
// measured for this item, so a divergence between the passes can never write past the item's slot.
template <bool EMIT>
struct Sink {
    uint8_t* out;        // this item's arena slot
    int32_t* wsz;        // this item's chunk sizes
    int64_t cap;         // bytes pass 1 measured (pass 2 only)
    int wcap;            // writes pass 1 measured (pass 2 only)
    int64_t n = 0;       // bytes produced
    int writes = 0;      // chunks produced
    int pos = 0;         // staging-buffer position

    __device__ __forceinline__ void put(uint8_t c)
    {
        if (EMIT && n < cap) out[n] = c;
        n++;
        pos++;
    }
    __device__ __forceinline__ void flush()   // one write(2) of the staged bytes
    {
        if (EMIT && writes < wcap) wsz[writes] = pos;
        writes++;
        pos = 0;
    }
    __device__ __forceinline__ void reset_code()    // ESC [ 0 m
    {
        put(27); put('['); put('0'); put('m');
    }
};

// np_write_user_stream (oracle/nuts_path.c; nuts333.c:1315-1365), one item, sequential.
template <bool EMIT>
__device__ void transduce(const uint8_t* s, int len, bool colour, Sink<EMIT>& k)
{
    int i = 0;
    while (i < len) {
        const uint8_t ch = s[i];
        if (ch == '\n') {
            if (k.pos > kOutBuff - 6) k.flush();
            if (colour) k.reset_code();
            k.put('\n');
            k.put('\r');
            i++;
        } else if (ch == '/' && i + 1 < len && s[i + 1] == '~') {
            i++;                        // drop the slash; no fullness check on this path
            continue;
        } else if (i > 0 && ch == '~' && s[i - 1] == '/') {
            k.put('~');                 // the look-behind is on the input, not on what was kept
            i++;
        } else if (ch == '~') {
            if (k.pos > kOutBuff - 6) k.flush();
            const int c = colcom_at(s, i, len);
            if (c >= 0) {
                if (colour) {
                    k.put(27); k.put('['); k.put((uint8_t)kColArg[c][0]);
                    if (kColArg[c][1]) k.put((uint8_t)kColArg[c][1]);
                    k.put('m');
                }
                i += 3;
            } else {
                k.put('~');
                i++;
            }
        } else {
            k.put(ch);
            i++;
        }
        if (k.pos == kOutBuff) k.flush();
    }
    if (k.pos) k.flush();
    if (colour) {                       // the trailing reset is a write of its own (nuts333.c:1363,1365)
        k.reset_code();
        k.flush();
    }
}

// Stage the broadcast's shared text in LDS (every lane of the block reads it byte by byte).
__device__ __forceinline__ const uint8_t* stage_text(uint8_t* lds, const uint8_t* text, int len)
{
    for (int j = threadIdx.x; j < len; j += blockDim.x) lds[j] = text[j];
    __syncthreads();
    return lds;
}

template <bool BROADCAST>
__device__ void measure(const uint8_t* text, const int32_t* text_off, const int32_t* text_len, const uint8_t* rec,
                        int n_items, int rm_is_null, int force_listen, int com_num, uint8_t* admitted, int64_t* nbytes,
                        int32_t* nwrites, int* bound_violations)
{
    __shared__ uint8_t lds[kTextSize];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint8_t* s = text;
    int len;
    if (BROADCAST) {
        len = text_len[0];
        s = stage_text(lds, text, len);
    }
    if (i >= n_items) return;
    if (!BROADCAST) {
        s = text + text_off[i];
        len = text_len[i];
    }
    const uint8_t l = rec[i];
    const bool in = !BROADCAST || admits(l, rm_is_null, force_listen, com_num);
    Sink<false> k{nullptr, nullptr, 0, 0};
    if (in) transduce(s, len, (l & kColour) != 0, k);
    if (k.n > 6 * (int64_t)len + 4 || k.writes > kMaxWrites) atomicAdd(bound_violations, 1);
    admitted[i] = in;
    nbytes[i] = k.n;
    nwrites[i] = k.writes;
}

template <bool BROADCAST>
__device__ void emit(const uint8_t* text, const int32_t* text_off, const int32_t* text_len, const uint8_t* rec,
                     int n_items, const uint8_t* admitted, const int64_t* nbytes, const int32_t* nwrites,
                     const int64_t* out_off, const int32_t* w_off, uint8_t* arena, int64_t arena_cap,
                     int32_t* write_sizes, int64_t wsz_cap)
{
    __shared__ uint8_t lds[kTextSize];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint8_t* s = text;
    int len;
    if (BROADCAST) {
        len = text_len[0];
        s = stage_text(lds, text, len);
    }
    if (i >= n_items || !admitted[i]) return;
    if (!BROADCAST) {
        s = text + text_off[i];
        len = text_len[i];
    }
    // never past the arena or the chunk array, even if pass 1 broke the bounds the host allocated by
    const int64_t room = arena_cap - out_off[i], wroom = (int64_t)wsz_cap - w_off[i];
    const int64_t cap = nbytes[i] < room ? nbytes[i] : (room > 0 ? room : 0);
    const int wcap = (int)(nwrites[i] < wroom ? nwrites[i] : (wroom > 0 ? wroom : 0));
    Sink<true> k{arena + out_off[i], write_sizes + w_off[i], cap, wcap};
    transduce(s, len, (rec[i] & kColour) != 0, k);
}

}  // namespace

// Stable, unmangled kernel names (they are what rocprofv3 reports).
extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_measure_batch(
    const uint8_t* text, const int32_t* text_off, const int32_t* text_len, const uint8_t* rec, int n_items,
    uint8_t* admitted, int64_t* nbytes, int32_t* nwrites, int* bound_violations)
{
    measure<false>(text, text_off, text_len, rec, n_items, 0, 0, 0, admitted, nbytes, nwrites, bound_violations);
}

extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_measure_broadcast(
    const uint8_t* text, const int32_t* text_len, const uint8_t* rec, int n_items, int rm_is_null, int force_listen,
    int com_num, uint8_t* admitted, int64_t* nbytes, int32_t* nwrites, int* bound_violations)
{
    measure<true>(text, nullptr, text_len, rec, n_items, rm_is_null, force_listen, com_num, admitted, nbytes, nwrites,
                  bound_violations);
}

extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_emit_batch(
    const uint8_t* text, const int32_t* text_off, const int32_t* text_len, const uint8_t* rec, int n_items,
    const uint8_t* admitted, const int64_t* nbytes, const int32_t* nwrites, const int64_t* out_off, const int32_t* w_off,
    uint8_t* arena, int64_t arena_cap, int32_t* write_sizes, int64_t wsz_cap)
{
    emit<false>(text, text_off, text_len, rec, n_items, admitted, nbytes, nwrites, out_off, w_off, arena, arena_cap,
                write_sizes, wsz_cap);
}

extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_emit_broadcast(
    const uint8_t* text, const int32_t* text_len, const uint8_t* rec, int n_items, const uint8_t* admitted,
    const int64_t* nbytes, const int32_t* nwrites, const int64_t* out_off, const int32_t* w_off, uint8_t* arena,
    int64_t arena_cap, int32_t* write_sizes, int64_t wsz_cap)
{
    emit<true>(text, nullptr, text_len, rec, n_items, admitted, nbytes, nwrites, out_off, w_off, arena, arena_cap,
               write_sizes, wsz_cap);
}

// ------------------------------------------------------------------------------------------ host library

namespace {

// Device and pinned host buffers, grown on demand and kept across calls (one process, one caller).
struct Buffers {
    size_t cap_items = 0, cap_text = 0, cap_arena = 0, cap_scan = 0;   // chunk sizes: cap_items * kMaxWrites
    size_t cap_host_arena = 0, cap_host_writes = 0;
    uint8_t *d_text = nullptr, *d_rec = nullptr, *d_admitted = nullptr, *d_arena = nullptr;
    int32_t *d_text_off = nullptr, *d_text_len = nullptr, *d_nwrites = nullptr, *d_w_off = nullptr, *d_wsz = nullptr;
    int64_t *d_nbytes = nullptr, *d_out_off = nullptr;
    int* d_violations = nullptr;
    void* d_scan = nullptr;
    uint8_t* h_arena = nullptr;         // pinned: the arena's D2H lands here
    int32_t* h_wsz = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ready = false;
};
Buffers g;
char g_err[512];

int fail(const char* what, hipError_t e)
{
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return -1;
}

#define ND_CHECK(call)                                  \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return fail(#call, e_);   \
    } while (0)

template <typename T>
int grow_dev(T** p, size_t* cap, size_t want, const char* what)
{
    if (want <= *cap) return 0;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc((void**)p, want * sizeof(T));
    if (e != hipSuccess) return fail(what, e);
    *cap = want;
    return 0;
}

template <typename T>
int grow_host(T** p, size_t* cap, size_t want, const char* what)
{
    if (want <= *cap) return 0;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    hipError_t e = hipHostMalloc((void**)p, want * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) return fail(what, e);
    *cap = want;
    return 0;
}

int ensure_ready()
{
    if (g.ready) return 0;
    int n = 0;
    ND_CHECK(hipGetDeviceCount(&n));
    if (n < 1) {
        snprintf(g_err, sizeof(g_err), "no GPU visible");
        return -1;
    }
    ND_CHECK(hipSetDevice(0));
    ND_CHECK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    ND_CHECK(hipEventCreate(&g.ev0));
    ND_CHECK(hipEventCreate(&g.ev1));
    ND_CHECK(hipMalloc((void**)&g.d_violations, sizeof(int)));
    g.ready = true;
    return 0;
}

// Grow every device buffer for n items, text_bytes of text and the hard output bound of the arena.
int reserve(size_t n, size_t text_bytes, size_t arena_bound)
{
    if (n > g.cap_items) {      // the per-item arrays share one capacity
        (void)hipFree(g.d_rec); (void)hipFree(g.d_admitted); (void)hipFree(g.d_text_off); (void)hipFree(g.d_text_len);
        (void)hipFree(g.d_nwrites); (void)hipFree(g.d_w_off); (void)hipFree(g.d_nbytes); (void)hipFree(g.d_out_off);
        (void)hipFree(g.d_wsz); (void)hipFree(g.d_scan);
        g.d_rec = g.d_admitted = nullptr;
        g.d_text_off = g.d_text_len = g.d_nwrites = g.d_w_off = g.d_wsz = nullptr;
        g.d_nbytes = g.d_out_off = nullptr;
        g.d_scan = nullptr;
        g.cap_items = g.cap_scan = 0;
        ND_CHECK(hipMalloc((void**)&g.d_rec, n));
        ND_CHECK(hipMalloc((void**)&g.d_admitted, n));
        ND_CHECK(hipMalloc((void**)&g.d_text_off, n * sizeof(int32_t)));
        ND_CHECK(hipMalloc((void**)&g.d_text_len, n * sizeof(int32_t)));
        ND_CHECK(hipMalloc((void**)&g.d_nwrites, n * sizeof(int32_t)));
        ND_CHECK(hipMalloc((void**)&g.d_w_off, n * sizeof(int32_t)));
        ND_CHECK(hipMalloc((void**)&g.d_nbytes, n * sizeof(int64_t)));
        ND_CHECK(hipMalloc((void**)&g.d_out_off, n * sizeof(int64_t)));
        ND_CHECK(hipMalloc((void**)&g.d_wsz, n * kMaxWrites * sizeof(int32_t)));
        size_t s1 = 0, s2 = 0;
        ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, s1, g.d_nbytes, g.d_out_off, (int)n, g.stream));
        ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, s2, g.d_nwrites, g.d_w_off, (int)n, g.stream));
        g.cap_scan = s1 > s2 ? s1 : s2;
        ND_CHECK(hipMalloc(&g.d_scan, g.cap_scan > 0 ? g.cap_scan : 1));
        g.cap_items = n;
    }
    if (grow_dev(&g.d_text, &g.cap_text, text_bytes > 0 ? text_bytes : 1, "text")) return -1;
    if (grow_dev(&g.d_arena, &g.cap_arena, arena_bound > 0 ? arena_bound : 1, "arena")) return -1;
    return 0;
}

double now_ns()
{
    return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

extern "C" {

// Timings of the last call.
struct nd_timing {
    double kernels_us;      // device events around measure .. emit (both scans included)
    double end_to_end_us;   // host clock: H2D of inputs, kernels, D2H of results, ending in a synchronise
};

const char* nd_last_error(void) { return g_err; }

// Number of visible GPUs (0 when none; negative on a runtime error).
int nd_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e == hipErrorNoDevice) return 0;
    if (e != hipSuccess) return fail("hipGetDeviceCount", e);
    return n;
}

// One fan-out.  broadcast != 0: one shared text (text_off unused, text_len[0] its length), rec[] are listener
// records and the admit predicate runs; broadcast == 0: n independent items, rec[] holds only the colour bit.
// Outputs (host, caller-allocated): admitted[n], out_off[n+1], w_off[n+1].  The arena and the chunk sizes stay in
// pinned memory owned by the library (nd_arena / nd_write_sizes) until the next call.  Returns 0, or -1 with
// nd_last_error() set.  The caller has validated the input (no NUL, len < 2000, offsets inside text).
int nd_fanout(int broadcast, const uint8_t* text, int64_t text_bytes, const int32_t* text_off, const int32_t* text_len,
              const uint8_t* rec, int n, int rm_is_null, int force_listen, int com_num, uint8_t* admitted,
              int64_t* out_off, int32_t* w_off, int64_t arena_bound, nd_timing* timing)
{
    if (ensure_ready()) return -1;
    if (n < 1) {
        snprintf(g_err, sizeof(g_err), "empty batch");
        return -1;
    }
    const double t0 = now_ns();
    if (reserve((size_t)n, (size_t)text_bytes, (size_t)arena_bound)) return -1;
    hipStream_t st = g.stream;
    size_t need1 = 0, need2 = 0;     // the scans' scratch for this n (reserve() sized it for the capacity)
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need1, g.d_nbytes, g.d_out_off, n, st));
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need2, g.d_nwrites, g.d_w_off, n, st));
    if (grow_dev((uint8_t**)&g.d_scan, &g.cap_scan, need1 > need2 ? need1 : need2, "scan scratch")) return -1;
    ND_CHECK(hipMemcpyAsync(g.d_text, text, (size_t)text_bytes, hipMemcpyHostToDevice, st));
    ND_CHECK(hipMemcpyAsync(g.d_text_len, text_len, (broadcast ? 1 : (size_t)n) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (!broadcast) ND_CHECK(hipMemcpyAsync(g.d_text_off, text_off, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    ND_CHECK(hipMemcpyAsync(g.d_rec, rec, (size_t)n, hipMemcpyHostToDevice, st));
    ND_CHECK(hipMemsetAsync(g.d_violations, 0, sizeof(int), st));

    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    ND_CHECK(hipEventRecord(g.ev0, st));
    if (broadcast)
        hipLaunchKernelGGL(nuts_fanout_measure_broadcast, grid, block, 0, st, g.d_text, g.d_text_len, g.d_rec, n,
                           rm_is_null, force_listen, com_num, g.d_admitted, g.d_nbytes, g.d_nwrites, g.d_violations);
    else
        hipLaunchKernelGGL(nuts_fanout_measure_batch, grid, block, 0, st, g.d_text, g.d_text_off, g.d_text_len, g.d_rec,
                           n, g.d_admitted, g.d_nbytes, g.d_nwrites, g.d_violations);
    ND_CHECK(hipGetLastError());
    size_t scan_bytes = g.cap_scan;
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(g.d_scan, scan_bytes, g.d_nbytes, g.d_out_off, n, st));
    scan_bytes = g.cap_scan;
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(g.d_scan, scan_bytes, g.d_nwrites, g.d_w_off, n, st));
    if (broadcast)
        hipLaunchKernelGGL(nuts_fanout_emit_broadcast, grid, block, 0, st, g.d_text, g.d_text_len, g.d_rec, n,
                           g.d_admitted, g.d_nbytes, g.d_nwrites, g.d_out_off, g.d_w_off, g.d_arena,
                           (int64_t)g.cap_arena, g.d_wsz, (int64_t)g.cap_items * kMaxWrites);
    else
        hipLaunchKernelGGL(nuts_fanout_emit_batch, grid, block, 0, st, g.d_text, g.d_text_off, g.d_text_len, g.d_rec, n,
                           g.d_admitted, g.d_nbytes, g.d_nwrites, g.d_out_off, g.d_w_off, g.d_arena,
                           (int64_t)g.cap_arena, g.d_wsz, (int64_t)g.cap_items * kMaxWrites);
    ND_CHECK(hipGetLastError());
    ND_CHECK(hipEventRecord(g.ev1, st));

    // the small per-item arrays first: they say how much of the arena to fetch
    int64_t last_len = 0;
    int32_t last_w = 0;
    int violations = 0;
    ND_CHECK(hipMemcpyAsync(admitted, g.d_admitted, (size_t)n, hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(out_off, g.d_out_off, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(w_off, g.d_w_off, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(&last_len, g.d_nbytes + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(&last_w, g.d_nwrites + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(&violations, g.d_violations, sizeof(int), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipStreamSynchronize(st));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d item(s) exceeded the hard output bounds (6*len+4 bytes, %d writes)",
                 violations, kMaxWrites);
        return -1;
    }
    out_off[n] = out_off[n - 1] + last_len;
    w_off[n] = w_off[n - 1] + last_w;
    if (grow_host(&g.h_arena, &g.cap_host_arena, (size_t)out_off[n] + 1, "pinned arena")) return -1;
    if (grow_host(&g.h_wsz, &g.cap_host_writes, (size_t)w_off[n] + 1, "pinned write sizes")) return -1;
    ND_CHECK(hipMemcpyAsync(g.h_arena, g.d_arena, (size_t)out_off[n], hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(g.h_wsz, g.d_wsz, (size_t)w_off[n] * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipStreamSynchronize(st));
    const double t1 = now_ns();

    float ms = 0.f;
    ND_CHECK(hipEventElapsedTime(&ms, g.ev0, g.ev1));
    if (timing) {
        timing->kernels_us = (double)ms * 1e3;
        timing->end_to_end_us = (t1 - t0) * 1e-3;
    }
    return 0;
}

const uint8_t* nd_arena(void) { return g.h_arena; }
const int32_t* nd_write_sizes(void) { return g.h_wsz; }

}  // extern "C"
