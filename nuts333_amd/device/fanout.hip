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
//   scan    hipcub DeviceScan::ExclusiveSum of bytes (int64) and write counts (int32), over n + 1
//           entries (the last one zero), so that the last offsets are the totals
//   pass 2  nuts_fanout_emit_{batch,broadcast}: bytes into the arena, chunk sizes into write_sizes
// In broadcast mode every item reads the same text, which each block stages in LDS once.  All four
// kernels take one argument struct (Args), filled by the host.  nuts_fanout_{measure,emit}_many do K broadcasts in
// one call, and nuts_roster_{measure,emit} K broadcasts to a roster kept on the device (their sections below).
// nuts_roster_plan answers the same K broadcasts to a roster in another form, a delivery plan: per broadcast its two
// variants (colour off, colour on) with their chunk sizes, and one admit bit per slot -- one kernel, no scan, no arena.
// A roster can also own review rings, the device's record() / .review (nuts333.c:2062-2070, 5192-5222): nuts_roster_record
// stores a plan call's recorded broadcasts in their rooms' rings, nuts_roster_review transduces the rings of a list of
// rooms, one wave per (line, colour variant), parallel over the line's bytes (their section below).
// And it can keep what the speech commands read of a speaker: nuts_roster_speak composes what say(), shout(), emote() and
// semote() write for K (user, command, inpstr, word_count) events, a wave per event, and nuts_roster_speak_plan plans the
// composed texts as nuts_roster_plan would (their section below).  nuts_roster_parse frames and dispatches client reads in
// front of them, and nuts_roster_tell answers the private speech commands, tell() and pemote(), a block per event with
// get_user() parallel over the roster's slots; the slots' revtell rings are roster_record / roster_review at 5 lines.
// nuts_roster_look answers look() for K lookers as texts and lists: the five texts of every distinct room, a line per user
// of those rooms, and per looker the users it is shown, by blocks that walk the roster's slots; nuts_roster_speak_plan
// then gives every text its two variants (its section below).
// nuts_roster_relay answers the clone branch of write_room_except after nuts_roster_plan, in the same call: which of the
// roster's clone records relay each broadcast to their owners, and the prefixed text they send (its section below).
// nuts_roster_go, nuts_roster_access, nuts_roster_clone, nuts_roster_set and nuts_roster_act decide and compose the commands
// that change what the other kernels read -- a user's room, a room's access and the invitations, the clone records, what a
// user sets on itself, and another user's room and muzzle -- each followed by a one-wave kernel that defers the events an
// earlier one of the call touched; none of them writes a kept table (their sections below).  The five are one kind of call,
// the event call, and what they share is
// written once: the head of their arguments (EventArgs), the walk of the order kernels (order_events, with a rule per
// kernel: its keys, what hits, what touches), and on the host the layouts' head and tail (take_events, take_event_texts)
// and the steps of the call from check_events to copy_event_results.
//
// Hard bounds per item of a text of len < 2000 bytes: 6*len + 4 output bytes (a '\n' with colour
// on is the costliest input byte, plus the trailing reset) and 16 writes.  The host sizes its buffers
// by them; pass 2 never writes past the counts pass 1 measured for its own item.
//
// The host library keeps one device block, laid out afresh per call into every array the kernels
// use and the scans' scratch; a roster has an allocation of its own, which nd_roster_plan uses alone (one upload, one
// launch, one download, one synchronise per call).  C ABI at the bottom; built with
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC fanout.hip -o _build/libnuts_device.so

#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>

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

// A roster slot's listener record for one broadcast: the slot's own bits from its flags byte, has_room from its room,
// and the two that the broadcast decides, same_room (never set when rm is -1, every room) and is_sender (sender -1:
// none).
__device__ __forceinline__ uint8_t listener_record(int room, uint8_t slot, int rm, int sender, int j)
{
    return (slot & (kLogin | kIgnall | kIgnshout | kColour)) | (room >= 0 ? kHasRoom : 0) |
           (rm >= 0 && room == rm ? kSameRoom : 0) | (j == sender ? kSender : 0);
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

// Everything a kernel reads or writes, filled on the host and passed by value to all four kernels.  The per-item
// arrays hold n entries; nbytes / nwrites / out_off / w_off hold n + 1, the last count zero, so that the scans
// leave the totals in out_off[n] / w_off[n].
struct Args {
    const uint8_t* text;         // broadcast: the shared text; batch: the items' texts, packed
    const int32_t* text_off;     // batch only
    const int32_t* text_len;     // broadcast: text_len[0] only
    const uint8_t* rec;          // listener record (broadcast) or the colour bit alone (batch)
    int n;
    int rm_is_null, force_listen, com_num;   // broadcast only
    uint8_t* admitted;
    int64_t* nbytes;             // pass 1: bytes per item
    int32_t* nwrites;            // pass 1: write(2) calls per item
    int64_t* out_off;            // scan of nbytes: each item's slot in the arena
    int32_t* w_off;              // scan of nwrites: each item's first entry in wsz
    int* violations;             // items past the hard bounds
    uint8_t* arena;
    int64_t arena_cap;
    int32_t* wsz;                // chunk sizes
    int64_t wsz_cap;
};

// Lane i's item, or false past the end.  In a broadcast the whole block first stages the shared text in LDS
// (every lane reads it byte by byte), so every lane calls this before it may return.
template <bool BROADCAST>
__device__ __forceinline__ bool load_item(const Args& a, int i, const uint8_t*& s, int& len)
{
    if (BROADCAST) {
        __shared__ uint8_t lds[kTextSize];
        len = a.text_len[0];
        for (int j = threadIdx.x; j < len; j += blockDim.x) lds[j] = a.text[j];
        __syncthreads();
        s = lds;
        return i < a.n;
    }
    if (i >= a.n) return false;
    s = a.text + a.text_off[i];
    len = a.text_len[i];
    return true;
}

template <bool BROADCAST>
__device__ void measure(const Args& a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {               // the scans' extra entry
        a.nbytes[a.n] = 0;
        a.nwrites[a.n] = 0;
    }
    const uint8_t* s;
    int len;
    if (!load_item<BROADCAST>(a, i, s, len)) return;
    const uint8_t l = a.rec[i];
    const bool in = !BROADCAST || admits(l, a.rm_is_null, a.force_listen, a.com_num);
    Sink<false> k{nullptr, nullptr, 0, 0};
    if (in) transduce(s, len, (l & kColour) != 0, k);
    if (k.n > 6 * (int64_t)len + 4 || k.writes > kMaxWrites) atomicAdd(a.violations, 1);
    a.admitted[i] = in;
    a.nbytes[i] = k.n;
    a.nwrites[i] = k.writes;
}

template <bool BROADCAST>
__device__ void emit(const Args& a)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint8_t* s;
    int len;
    if (!load_item<BROADCAST>(a, i, s, len) || !a.admitted[i]) return;
    // never past the arena or the chunk array, even if pass 1 broke the bounds the host allocated by
    const int64_t room = a.arena_cap - a.out_off[i], wroom = a.wsz_cap - a.w_off[i];
    const int64_t cap = a.nbytes[i] < room ? a.nbytes[i] : (room > 0 ? room : 0);
    const int wcap = (int)(a.nwrites[i] < wroom ? a.nwrites[i] : (wroom > 0 ? wroom : 0));
    Sink<true> k{a.arena + a.out_off[i], a.wsz + a.w_off[i], cap, wcap};
    transduce(s, len, (a.rec[i] & kColour) != 0, k);
}

// ------------------------------------------------------------------ many broadcasts per call
//
// K broadcasts, each with its own text, flags, command and listener table; item = (broadcast k, listener j), items
// ordered broadcast by broadcast.  One block per (broadcast, 256-listener tile).  A listener's output depends only on
// its colour bit (nuts333.c:1321,1344), so a block transduces its text twice -- colour off on wave 0, colour on on
// wave 1, concurrently -- and every item takes its variant's bytes and writes, or none if it is not admitted.
//   measure  nuts_fanout_measure_many: both variants counted; admit flag, bytes, writes per item
//   scan     as above, over m + 1 entries
//   emit     nuts_fanout_emit_many: both variants transduced into LDS; the tile's items copied out of them with
//            aligned 4-byte stores, kGroup lanes per item, and their chunk sizes likewise
constexpr int kVarCap = 6 * (kTextSize - 1) + 4;   // the hard bound of the longest text: 11998 bytes
constexpr int kGroup = 16;                          // lanes per item in emit (>= kMaxWrites)

struct ManyArgs {
    const uint8_t* text;         // the K texts, packed
    const int32_t* text_off;     // [k]
    const int32_t* text_len;     // [k]
    const uint8_t* flags;        // [k] bit 0 rm_is_null, bit 1 force_listen
    const int32_t* com_num;      // [k]
    const int32_t* item_off;     // [k + 1] broadcast b owns items item_off[b] .. item_off[b + 1] - 1
    const int32_t* tile_off;     // [k + 1] and blocks tile_off[b] .. tile_off[b + 1] - 1
    const uint8_t* rec;          // [m] listener records
    int k, m;
    int* violations;             // items past the hard bounds (zeroed by the host's upload)
    uint8_t* admitted;           // [m]
    int64_t* out_off;            // [m + 1]
    int32_t* w_off;              // [m + 1]
    int64_t* nbytes;             // [m + 1]
    int32_t* nwrites;            // [m + 1]
    uint8_t* arena;
    int64_t arena_cap;
    int32_t* wsz;
    int64_t wsz_cap;
};

struct Tile {
    int b, lo, hi;               // broadcast, first item, one past the last item
};

// This block's broadcast: the b with tile_off[b] <= blockIdx.x < tile_off[b + 1] (every broadcast has >= 1 tile).
__device__ __forceinline__ Tile find_tile(const ManyArgs& a)
{
    const int blk = (int)blockIdx.x;
    int lo = 0, hi = a.k;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.tile_off[mid] <= blk) lo = mid;
        else hi = mid;
    }
    const int first = a.item_off[lo] + (blk - a.tile_off[lo]) * kBlock;
    const int end = a.item_off[lo + 1];
    return {lo, first, first + kBlock < end ? first + kBlock : end};
}

// Stage broadcast b's text in LDS, then transduce it with colour off (lane 0 of wave 0) and on (lane 0 of wave 1).
// EMIT: the bytes go to var[c * kVarCap ..] and the chunk sizes to vwsz[c * kMaxWrites ..], clamped to the hard bounds.
// vn / vw get the full counts, so a bound violation stays visible.  Every thread of the block calls this.
template <bool EMIT, typename A>   // A: ManyArgs or RosterArgs
__device__ __forceinline__ void stage_variants(const A& a, int b, uint8_t* text, uint8_t* var, int32_t* vwsz,
                                               int64_t* vn, int* vw)
{
    const int len = a.text_len[b];
    const uint8_t* src = a.text + a.text_off[b];
    for (int j = threadIdx.x; j < len; j += blockDim.x) text[j] = src[j];
    __syncthreads();
    if (threadIdx.x == 0 || threadIdx.x == 64) {
        const int c = threadIdx.x >> 6;
        Sink<EMIT> k{EMIT ? var + c * kVarCap : nullptr, EMIT ? vwsz + c * kMaxWrites : nullptr, 6 * (int64_t)len + 4,
                     kMaxWrites};
        transduce(text, len, c != 0, k);
        vn[c] = k.n;
        vw[c] = k.writes;
    }
    __syncthreads();
}

__device__ void measure_many(const ManyArgs& a)
{
    __shared__ uint8_t text[kTextSize];
    __shared__ int64_t vn[2];
    __shared__ int vw[2];
    if (blockIdx.x == 0 && threadIdx.x == 0) {      // the scans' extra entry
        a.nbytes[a.m] = 0;
        a.nwrites[a.m] = 0;
    }
    const Tile t = find_tile(a);
    stage_variants<false>(a, t.b, text, nullptr, nullptr, vn, vw);
    const int i = t.lo + (int)threadIdx.x;
    if (i >= t.hi) return;
    const uint8_t l = a.rec[i];
    const int fl = a.flags[t.b];
    const bool in = admits(l, fl & 1, (fl >> 1) & 1, a.com_num[t.b]);
    const int c = (l & kColour) ? 1 : 0;
    const int64_t nb = in ? vn[c] : 0;
    const int nw = in ? vw[c] : 0;
    if (nb > 6 * (int64_t)a.text_len[t.b] + 4 || nw > kMaxWrites) atomicAdd(a.violations, 1);
    a.admitted[i] = in;
    a.nbytes[i] = nb;
    a.nwrites[i] = nw;
}

__device__ void emit_many(const ManyArgs& a)
{
    __shared__ uint8_t text[kTextSize];
    __shared__ uint8_t var[2 * kVarCap];
    __shared__ int32_t vwsz[2 * kMaxWrites];
    __shared__ int64_t vn[2];
    __shared__ int vw[2];
    __shared__ int64_t s_off[kBlock], s_n[kBlock];   // per item of the tile: arena slot, bytes to write there
    __shared__ int32_t s_woff[kBlock], s_nw[kBlock]; // first chunk-size entry, chunk sizes to write
    __shared__ uint8_t s_c[kBlock];                  // variant
    const Tile t = find_tile(a);
    const int len = a.text_len[t.b];
    {   // this item's metadata, loaded before the transduce so that the loads overlap it; clamped so that nothing is
        // written past the arena, the chunk array or the LDS variant, even if measure broke the bounds
        const int i = t.lo + (int)threadIdx.x;
        if (i < t.hi) {
            const bool in = a.admitted[i] != 0;
            const int64_t off = a.out_off[i], woff = a.w_off[i];
            const int64_t room = a.arena_cap - off, wroom = a.wsz_cap - woff;
            int64_t n = in ? a.nbytes[i] : 0;
            n = n < room ? n : room;
            n = n < 6 * (int64_t)len + 4 ? n : 6 * (int64_t)len + 4;
            int64_t nw = in ? a.nwrites[i] : 0;
            nw = nw < wroom ? nw : wroom;
            nw = nw < kMaxWrites ? nw : kMaxWrites;
            s_off[threadIdx.x] = off;
            s_n[threadIdx.x] = n > 0 ? n : 0;
            s_woff[threadIdx.x] = (int32_t)woff;
            s_nw[threadIdx.x] = nw > 0 ? (int32_t)nw : 0;
            s_c[threadIdx.x] = (a.rec[i] & kColour) ? 1 : 0;
        }
    }
    stage_variants<true>(a, t.b, text, var, vwsz, vn, vw);   // its barriers publish the metadata too
    const int g = (int)threadIdx.x / kGroup, lane = (int)threadIdx.x % kGroup;
    for (int j = g; j < t.hi - t.lo; j += kBlock / kGroup) {
        const int c = s_c[j];
        const int64_t n0 = s_n[j], vmax = vn[c] < kVarCap ? vn[c] : kVarCap;
        const int64_t n = n0 < vmax ? n0 : vmax;
        const uint8_t* src = var + c * kVarCap;
        uint8_t* dst = a.arena + s_off[j];
        // w: item-relative offset of a 4-byte word of the arena (the arena is 256-byte aligned), from the word
        // holding the item's first byte; whole words in one store, the item's partial edge words byte by byte
        const int head = (int)(s_off[j] & 3);
        for (int64_t w = 4 * lane - head; w < n; w += 4 * kGroup) {
            if (w >= 0 && w + 4 <= n) {
                const uint32_t v = (uint32_t)src[w] | (uint32_t)src[w + 1] << 8 | (uint32_t)src[w + 2] << 16 |
                                   (uint32_t)src[w + 3] << 24;
                *reinterpret_cast<uint32_t*>(dst + w) = v;
            } else {
                for (int q = 0; q < 4; q++)
                    if (w + q >= 0 && w + q < n) dst[w + q] = src[w + q];
            }
        }
        const int nw = s_nw[j] < vw[c] ? s_nw[j] : vw[c];
        if (lane < nw) a.wsz[s_woff[j] + lane] = vwsz[c * kMaxWrites + lane];
    }
}

static_assert(kGroup >= kMaxWrites, "emit_many writes an item's chunk sizes with one lane each");
static_assert(kBlock % kGroup == 0 && kBlock >= 128, "emit_many: whole lane groups; variants on waves 0 and 1");

// ------------------------------------------------------------------ broadcasts to a resident roster
//
// A roster is the talker's user list kept on the device between calls: per slot a room (-1: none -- an empty slot, or
// a user away over a netlink) and a flags byte holding the login, ignall, ignshout and colour bits of a listener record.
// Broadcast b is addressed as write_room_except addresses it (nuts333.c:1401-1415): room rm[b] (-1: every room) and
// the sender's slot sender[b] (-1: none).  Item (b, j) is slot j of broadcast b; every broadcast has `capacity` items.
// One block per (broadcast, 256-slot tile).
//   measure  nuts_roster_measure: each item's listener record built from its slot and its broadcast, and its admit flag;
//            the first tile of each broadcast also transduces the two variants (stage_variants) and stores their bytes,
//            chunk sizes and counts in the call's variant buffer -- once per broadcast per call
//   scan     as above, over m + 1 entries; an item's bytes and writes are looked up from its broadcast's variant counts
//   emit     nuts_roster_emit: the broadcast's variants staged in LDS from the buffer, the tile's items copied out of
//            them with aligned 4-byte stores, as emit_many does (copy_items)
struct RosterArgs {
    const int32_t* room;         // [capacity] -1: no room
    const uint8_t* slot;         // [capacity] kLogin | kIgnall | kIgnshout | kColour
    const uint8_t* text;         // the K texts, packed
    const int32_t* text_off;     // [k]
    const int32_t* text_len;     // [k]
    const int32_t* rm;           // [k] -1: every room (rm_is_null)
    const int32_t* sender;       // [k] -1: none
    const uint8_t* flags;        // [k] bit 1 force_listen
    const int32_t* com_num;      // [k]
    int k, capacity, tiles;      // tiles per broadcast
    int* violations;             // variants past the hard bounds (zeroed by the host's upload)
    uint8_t* admitted;           // [m], m = k * capacity
    int64_t* out_off;            // [m + 1]
    int32_t* w_off;              // [m + 1]
    uint8_t* var;                // broadcast b's variants: var_at(text_off[b], b), and that plus var_stride(len)
    int64_t* vn;                 // [2k] bytes of broadcast b's colour-off / colour-on variant
    int32_t* vw;                 // [2k] their write(2) counts
    int32_t* vwsz;               // [2k * kMaxWrites] their chunk sizes
    uint8_t* arena;
    int64_t arena_cap;
    int32_t* wsz;
    int64_t wsz_cap;
};

// The variant buffer's layout (Python: _variant_at and _variant_starts of device/__init__.py).  A variant's slot is its
// hard bound rounded up to 4 bytes; text t, whose bytes start at text_off among the call's texts, has its two slots at
// var_at(text_off, t) and that plus var_stride(len).  So every slot is 4-byte aligned, and k texts of text_bytes in all
// need var_at(text_bytes, k) bytes.
__host__ __device__ __forceinline__ int64_t var_stride(int len) { return (6 * (int64_t)len + 4 + 3) & ~(int64_t)3; }
__host__ __device__ __forceinline__ int64_t var_at(int64_t text_off, int64_t t) { return 12 * text_off + 16 * t; }

// Text t's two variants, by every thread of a block: transduced (stage_variants), then their bytes into the variant
// buffer, their chunk sizes and counts into vwsz / vn / vw, and a violation for each that broke the hard bounds.
// Static LDS: every block of a kernel that calls this reserves these ~26 KB, whether it gets here or not.
template <typename A>   // RosterArgs, PlanArgs or SpeakPlanArgs
__device__ __forceinline__ void store_variants(const A& a, int t)
{
    __shared__ uint8_t text[kTextSize];
    __shared__ uint8_t var[2 * kVarCap];
    __shared__ int32_t vwsz[2 * kMaxWrites];
    __shared__ int64_t vn[2];
    __shared__ int vw[2];
    stage_variants<true>(a, t, text, var, vwsz, vn, vw);
    const int len = a.text_len[t];
    const int64_t cap = 6 * (int64_t)len + 4, stride = var_stride(len);
    uint8_t* dst = a.var + var_at(a.text_off[t], t);
    for (int c = 0; c < 2; c++) {
        const int64_t n = vn[c] < cap ? vn[c] : cap;
        for (int64_t q = threadIdx.x; q < n; q += kBlock) dst[c * stride + q] = var[c * kVarCap + q];
        const int nw = vw[c] < kMaxWrites ? vw[c] : kMaxWrites;
        if ((int)threadIdx.x < nw) a.vwsz[(2 * t + c) * kMaxWrites + threadIdx.x] = vwsz[c * kMaxWrites + threadIdx.x];
    }
    if (threadIdx.x < 2) {
        a.vn[2 * t + threadIdx.x] = vn[threadIdx.x];
        a.vw[2 * t + threadIdx.x] = vw[threadIdx.x];
        if (vn[threadIdx.x] > cap || vw[threadIdx.x] > kMaxWrites) atomicAdd(a.violations, 1);
    }
}

__device__ void roster_measure(const RosterArgs& a)
{
    const int b = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - b * a.tiles;
    const int j = tile * kBlock + (int)threadIdx.x;
    if (j < a.capacity) {
        const int rm = a.rm[b];
        const uint8_t l = listener_record(a.room[j], a.slot[j], rm, a.sender[b], j);
        a.admitted[b * a.capacity + j] = admits(l, rm < 0, (a.flags[b] >> 1) & 1, a.com_num[b]);
    }
    // Block-uniform: this broadcast's variants, for the scan and emit.  The admit-only tiles reserve store_variants'
    // LDS too, so at most 6 blocks fit on a CU.  With at most 256 tiles per broadcast and the admit-only blocks this
    // short, that costs little at the sizes measured; a variant stage of its own grid would lift it, for
    // one more dispatch.
    if (tile == 0) store_variants(a, b);
}

// The scans' input: item i's bytes (T = int64_t, v = vn) or writes (T = int32_t, v = vw), its admitted variant's count;
// entry m, the scans' extra one, is zero.
template <typename T>
struct ItemCount {
    const uint8_t* admitted;
    const uint8_t* slot;
    const T* v;
    int capacity, m;
    __host__ __device__ T operator()(int i) const
    {
        if (i >= m || !admitted[i]) return 0;
        const int b = i / capacity;
        return v[2 * b + ((slot[i - b * capacity] & kColour) ? 1 : 0)];
    }
};

// nuts_roster_emit's copy of a tile's items out of the two variants in LDS: emit_many's copy loop, kept apart from it
// (sharing one inlined helper changed the code the compiler makes for emit_many).  Item j takes variant s_c[j], s_n[j]
// bytes into the arena at s_off[j] and s_nw[j] chunk sizes into wsz at s_woff[j], kGroup lanes per item.  The caller
// has clamped s_n / s_nw to the arena, the chunk array and the hard bounds.
__device__ __forceinline__ void copy_items(int count, const uint8_t* var, const int32_t* vwsz, const int64_t* vn,
                                           const int* vw, const int64_t* s_off, const int64_t* s_n,
                                           const int32_t* s_woff, const int32_t* s_nw, const uint8_t* s_c,
                                           uint8_t* arena, int32_t* wsz)
{
    const int g = (int)threadIdx.x / kGroup, lane = (int)threadIdx.x % kGroup;
    for (int j = g; j < count; j += kBlock / kGroup) {
        const int c = s_c[j];
        const int64_t n0 = s_n[j], vmax = vn[c] < kVarCap ? vn[c] : kVarCap;
        const int64_t n = n0 < vmax ? n0 : vmax;
        const uint8_t* src = var + c * kVarCap;
        uint8_t* dst = arena + s_off[j];
        // w: item-relative offset of a 4-byte word of the arena (the arena is 256-byte aligned), from the word
        // holding the item's first byte; whole words in one store, the item's partial edge words byte by byte
        const int head = (int)(s_off[j] & 3);
        for (int64_t w = 4 * lane - head; w < n; w += 4 * kGroup) {
            if (w >= 0 && w + 4 <= n) {
                const uint32_t v = (uint32_t)src[w] | (uint32_t)src[w + 1] << 8 | (uint32_t)src[w + 2] << 16 |
                                   (uint32_t)src[w + 3] << 24;
                *reinterpret_cast<uint32_t*>(dst + w) = v;
            } else {
                for (int q = 0; q < 4; q++)
                    if (w + q >= 0 && w + q < n) dst[w + q] = src[w + q];
            }
        }
        const int nw = s_nw[j] < vw[c] ? s_nw[j] : vw[c];
        if (lane < nw) wsz[s_woff[j] + lane] = vwsz[c * kMaxWrites + lane];
    }
}

__device__ void roster_emit(const RosterArgs& a)
{
    __shared__ uint8_t var[2 * kVarCap];
    __shared__ int32_t vwsz[2 * kMaxWrites];
    __shared__ int64_t vn[2];
    __shared__ int vw[2];
    __shared__ int64_t s_off[kBlock], s_n[kBlock];   // as in emit_many
    __shared__ int32_t s_woff[kBlock], s_nw[kBlock];
    __shared__ uint8_t s_c[kBlock];
    const int b = (int)blockIdx.x / a.tiles, j0 = ((int)blockIdx.x - b * a.tiles) * kBlock;
    const int len = a.text_len[b];
    const int64_t cap = 6 * (int64_t)len + 4;
    {   // this item's metadata, clamped as in emit_many; its bytes and writes are the differences of the scans
        const int j = j0 + (int)threadIdx.x;
        if (j < a.capacity) {
            const int i = b * a.capacity + j;
            const bool in = a.admitted[i] != 0;
            const int64_t off = a.out_off[i], woff = a.w_off[i];
            const int64_t room = a.arena_cap - off, wroom = a.wsz_cap - woff;
            int64_t n = in ? a.out_off[i + 1] - off : 0;
            n = n < room ? n : room;
            n = n < cap ? n : cap;
            int64_t nw = in ? a.w_off[i + 1] - woff : 0;
            nw = nw < wroom ? nw : wroom;
            nw = nw < kMaxWrites ? nw : kMaxWrites;
            s_off[threadIdx.x] = off;
            s_n[threadIdx.x] = n > 0 ? n : 0;
            s_woff[threadIdx.x] = (int32_t)woff;
            s_nw[threadIdx.x] = nw > 0 ? (int32_t)nw : 0;
            s_c[threadIdx.x] = (a.slot[j] & kColour) ? 1 : 0;
        }
    }
    // the broadcast's variants, as measure stored them, clamped to the hard bounds
    const uint8_t* src = a.var + var_at(a.text_off[b], b);
    const int64_t stride = var_stride(len);
    for (int c = 0; c < 2; c++) {
        const int64_t n = a.vn[2 * b + c] < cap ? a.vn[2 * b + c] : cap;
        for (int64_t q = threadIdx.x; q < n; q += kBlock) var[c * kVarCap + q] = src[c * stride + q];
        const int nw = a.vw[2 * b + c] < kMaxWrites ? a.vw[2 * b + c] : kMaxWrites;
        if ((int)threadIdx.x < nw) vwsz[c * kMaxWrites + threadIdx.x] = a.vwsz[(2 * b + c) * kMaxWrites + threadIdx.x];
        if (threadIdx.x == 0) {
            vn[c] = n;
            vw[c] = nw;
        }
    }
    __syncthreads();
    const int count = a.capacity - j0 < kBlock ? a.capacity - j0 : kBlock;
    copy_items(count, var, vwsz, vn, vw, s_off, s_n, s_woff, s_nw, s_c, a.arena, a.wsz);
}

static_assert(2 * kMaxWrites <= kBlock, "roster kernels move a broadcast's chunk sizes with one lane each");

// ------------------------------------------------------------------ a delivery plan for a resident roster
//
// A listener's output depends on nothing but its colour bit, so a broadcast has two outputs, not `capacity`: what a
// talker needs back is the two variants with their write(2) chunk sizes, and who is admitted.  nuts_roster_plan gives
// exactly that, in one launch: no per-item arrays, no scans, no emit, no arena, nothing whose size depends on how many
// slots were admitted.  One block per (broadcast, 256-slot tile), as nuts_roster_measure:
//   admit    each lane builds its slot's listener record as roster_measure does; the wave's 64 answers are one word of
//            the bitmap (__ballot): slot j of broadcast b is bit j % 64 of bits[b * words + j / 64].  Lanes past the
//            capacity vote false, so the tail bits of a broadcast's last word are zero.
//   variants the first tile of each broadcast transduces the two variants (stage_variants) and stores their bytes,
//            chunk sizes and counts, as roster_measure does.  Every block of the kernel reserves their ~26 KB of static
//            LDS, the admit-only tiles too (roster_measure's comment applies).
struct PlanArgs {
    const int32_t* room;         // [capacity] -1: no room
    const uint8_t* slot;         // [capacity] kLogin | kIgnall | kIgnshout | kColour
    const uint8_t* text;         // the K texts, packed
    const int32_t* text_off;     // [k]
    const int32_t* text_len;     // [k]
    const int32_t* rm;           // [k] -1: every room (rm_is_null)
    const int32_t* sender;       // [k] -1: none
    const uint8_t* flags;        // [k] bit 1 force_listen
    const int32_t* com_num;      // [k]
    int k, capacity, tiles;      // tiles per broadcast
    int words;                   // bitmap words per broadcast: ceil(capacity / 64)
    int* violations;             // variants past the hard bounds (zeroed by the host's upload)
    int64_t* vn;                 // [2k] bytes of broadcast b's colour-off / colour-on variant
    int32_t* vw;                 // [2k] their write(2) counts
    int32_t* vwsz;               // [2k * kMaxWrites] their chunk sizes
    uint64_t* bits;              // [k * words] the admit bitmap
    uint8_t* var;                // broadcast b's variants: var_at(text_off[b], b), and that plus var_stride(len)
};

__device__ void roster_plan(const PlanArgs& a)
{
    const int b = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - b * a.tiles;
    const int j = tile * kBlock + (int)threadIdx.x;
    bool in = false;
    if (j < a.capacity) {
        const int rm = a.rm[b];
        const uint8_t l = listener_record(a.room[j], a.slot[j], rm, a.sender[b], j);
        in = admits(l, rm < 0, (a.flags[b] >> 1) & 1, a.com_num[b]);
    }
    const uint64_t word = __ballot(in);          // the wave's 64 slots; every lane of the wave is here
    const int w = j >> 6;                        // word of this broadcast: a tile holds kBlock / 64 of them
    if ((threadIdx.x & 63) == 0 && w < a.words) a.bits[(int64_t)b * a.words + w] = word;
    if (tile == 0) store_variants(a, b);         // block-uniform: this broadcast's variants, as roster_measure's
}

static_assert(kBlock % 64 == 0, "roster_plan: a tile is whole bitmap words, one per wave");

// ------------------------------------------------------------------ review rings of a resident roster
//
// record() keeps the last 15 lines said in a room in a ring of 15 x 202 bytes with a cursor, revline (nuts333.c:2062-2070;
// np_record of oracle/nuts_path.c): strncpy of 200 bytes -- the text cut there, or padded with zeros --, '\n' at byte 200,
// NUL at byte 201, cursor + 1.  A stored line is the C string in its slot: a text below 200 bytes as it is, a longer one
// cut to 200 with the forced '\n' (201 bytes); an empty text stores an empty line.  .review (nuts333.c:5192-5222) sends
// the non-empty lines from the cursor onwards, oldest first, one write_user each.  A roster owns the rings of rooms
// 0 .. review_rooms - 1 and their cursors, in a device allocation of their own that never moves.
//   record   nuts_roster_record, after nuts_roster_plan of a call that records, on that call's uploaded inputs: one block
//            per ring room.  Wave 0 scans the K (flags, rm) pairs 64 at a time; a broadcast's rank among its room's recorded
//            broadcasts of the call is the running count plus the popcount of the ballot below its lane, so the order is
//            the call's own and the same on every run.  Only the last min(count, 15) survive, rank r in slot
//            (revline + r) % 15; the block copies them with byte stores and the cursor advances by count.
//   review   nuts_roster_review, one block per requested room: the ring staged in LDS oldest line first, then one wave
//            per (line, colour variant).  A byte's output depends on the bytes i-3 .. i+2 alone unless the staging buffer
//            flushes in mid-line, and it cannot while the line's output stays at or below kOutBuff - 6 = 994 bytes (the
//            flush test is pos > 994): lane l expands bytes 4l .. 4l+3, a 64-lane scan gives their offsets, the stores are
//            scattered.  A longer output (colour on, more than 165 newlines) takes the sequential transduce<>, a lane
//            per such (line, variant), after the waves.
//            The line outputs are built in LDS and copied out next to each other, so a variant is contiguous.
//   clear    clear_revbuff (nuts333.c: rev[i][0] = 0 for every line, revline = 0) travels as a byte per ring room with
//            the next record or review call.  A room whose byte is set is never read in that call: record starts it from
//            an empty ring, review shows it empty, and extra blocks past the requested rooms store the zeros.
constexpr int kRevLines = 15;                              // nuts333.h:37 REVIEW_LINES
constexpr int kRevLen = 200;                               // nuts333.h:39 REVIEW_LEN
constexpr int kRevSlot = kRevLen + 2;                      // one line of a ring
constexpr int kRevRing = kRevLines * kRevSlot;             // 3030 bytes per room
constexpr int kRevLineCap = 6 * (kRevLen + 1) + 4;         // 1210: 201 newlines with colour on, and the reset
constexpr int kRevLineStride = (kRevLineCap + 1 + 3) & ~3;   // a line's output in LDS, and a spare byte after it
constexpr int kRevLineWrites = 3;                          // 996 + 210 + 4 for that line
constexpr int kRevVarCap = kRevLines * kRevLineCap;        // 18150 bytes per variant
constexpr int rev_var_stride(int lines) { return (lines * kRevLineCap + 3) & ~3; }   // a variant's slot in the download
constexpr int kRevVarStride = rev_var_stride(kRevLines);
constexpr int kTellLines = 5;                              // nuts333.h: REVTELL_LINES, a user's revtell ring
constexpr int kRevWrites = kRevLines * kRevLineWrites;     // 45 writes per variant
constexpr int kRevTasks = 2 * kRevLines;                   // (line, variant) pairs of a room
constexpr int kWaveLimit = kOutBuff - 6;                   // a line output up to here never flushes in mid-line
constexpr uint8_t kRecordBit = 4;                          // bit 2 of a broadcast's flags byte: record it
constexpr int kMaxReviewRooms = 1024;

struct RecordArgs {
    const uint8_t* text;         // the plan call's inputs, as PlanArgs has them
    const int32_t* text_off;     // [k]
    const int32_t* text_len;     // [k]
    const int32_t* rm;           // [k]
    const uint8_t* flags;        // [k] bit 2: record this broadcast into the ring of room rm
    const uint8_t* clear;        // [review_rooms] non-zero: clear the room's ring first; nullptr: none
    int k, review_rooms;
    uint8_t* rings;              // [review_rooms * kRevRing]
    int32_t* revline;            // [review_rooms]
};

// LINES: the lines of a ring -- kRevLines for a room's review ring, kTellLines for a slot's revtell ring, whose "rooms" are
// the roster's slots (RecordArgs.rm the tells' targets, review_rooms the capacity).
template <int LINES>
__device__ void roster_record(const RecordArgs& a)
{
    __shared__ int s_surv[LINES];   // the broadcast of rank r, at r % LINES, for the last LINES ranks
    __shared__ int s_count, s_base;
    const int room = (int)blockIdx.x;
    const bool cleared = a.clear && a.clear[room];
    if (threadIdx.x < 64) {             // wave 0: every lane of it is here
        const int lane = (int)threadIdx.x;
        int count = 0;
        for (int b0 = 0; b0 < a.k; b0 += 64) {
            const int b = b0 + lane;
            const bool hit = b < a.k && (a.flags[b] & kRecordBit) && a.rm[b] == room;
            const uint64_t word = __ballot(hit);
            const int n = __popcll(word);
            const int rank = count + __popcll(word & ((1ull << lane) - 1));
            // the last LINES of this tile are distinct mod LINES; a later tile's stores follow these in program order
            if (hit && rank >= count + n - LINES) s_surv[rank % LINES] = b;
            count += n;
        }
        if (lane == 0) {
            s_count = count;
            s_base = cleared ? 0 : (int)((uint32_t)a.revline[room] % LINES);   // read by the thread that stores it
        }
    }
    __syncthreads();
    const int count = s_count, base = s_base;
    if (!count && !cleared) return;
    uint8_t* ring = a.rings + (size_t)room * LINES * kRevSlot;
    const int nsurv = count < LINES ? count : LINES;
    const int first = (count - nsurv) % LINES;      // rank of the oldest survivor, mod LINES
    if (cleared && threadIdx.x < LINES) {           // empty the slots no survivor lands in
        const int d = ((int)threadIdx.x - base - first + 2 * LINES) % LINES;
        if (d >= nsurv) ring[threadIdx.x * kRevSlot] = 0;
    }
    for (int idx = (int)threadIdx.x; idx < nsurv * kRevSlot; idx += kBlock) {
        const int j = idx / kRevSlot, i = idx - j * kRevSlot;
        const int r = (first + j) % LINES;
        const int b = s_surv[r];
        uint8_t v = 0;
        if (i < kRevLen) {
            if (i < a.text_len[b]) v = a.text[a.text_off[b] + i];
        } else if (i == kRevLen) {
            v = '\n';
        }
        ring[((base + r) % LINES) * kRevSlot + i] = v;
    }
    if (threadIdx.x == 0) a.revline[room] = (base + count % LINES) % LINES;
}

struct ReviewArgs {
    uint8_t* rings;              // [review_rooms * kRevRing]
    int32_t* revline;            // [review_rooms]
    const int32_t* rooms;        // [q] the rooms to review, duplicates allowed
    const uint8_t* clear;        // as RecordArgs.clear
    int q, review_rooms;
    int* violations;             // lines past the hard bounds (zeroed by the host's upload)
    int32_t* line_count;         // [q] non-empty lines
    int32_t* sequential;         // [q] (line, variant) pairs that took the sequential transducer
    int32_t* vn;                 // [2q] bytes of room q's colour-off / colour-on review
    int32_t* vw;                 // [2q] their write(2) counts
    int32_t* vwsz;               // [2q * kRevWrites] their chunk sizes
    uint8_t* lines;              // [q * kRevRing] the ring's slots, oldest first
    uint8_t* var;                // [2q * kRevVarStride] the reviews' bytes
};

// The output of line byte `ch` given the byte before it, p1, and the one after it, n1 (0 outside the line; no line byte
// is 0): its length, and its bytes packed into *v, first byte lowest.  Valid while no flush fires in mid-line.
//   consumed: a command tilde stands one or two bytes before it.  A tilde is a command tilde iff it is not preceded by
//   '/' and a colour command follows (own: which one, for a tilde; else -1); the two letters of a command are never
//   '~', '/' or '\n', so a command tilde is never itself consumed.  A '/' is dropped iff a '~' follows.
//   (transduce<>, without its position.)
__device__ __forceinline__ int expand_byte(uint8_t p1, uint8_t ch, uint8_t n1, bool consumed, int own, bool colour,
                                           uint64_t* v)
{
    *v = ch;
    if (ch == 0 || consumed) return 0;
    if (ch == '\n') {
        if (colour) {
            *v = 27ull | (uint64_t)'[' << 8 | (uint64_t)'0' << 16 | (uint64_t)'m' << 24 | (uint64_t)'\n' << 32 |
                 (uint64_t)'\r' << 40;
            return 6;
        }
        *v = (uint64_t)'\n' | (uint64_t)'\r' << 8;
        return 2;
    }
    if (ch == '/' && n1 == '~') return 0;
    if (ch == '~' && p1 != '/' && own >= 0) {
        if (!colour) return 0;
        const uint64_t a0 = (uint8_t)kColArg[own][0], a1 = (uint8_t)kColArg[own][1];
        *v = 27ull | (uint64_t)'[' << 8 | a0 << 16 | (a1 ? a1 << 24 | (uint64_t)'m' << 32 : (uint64_t)'m' << 24);
        return a1 ? 5 : 4;
    }
    return 1;
}

// LINES as roster_record's: the outputs are then LINES * kRevSlot stored bytes, rev_var_stride(LINES) bytes per variant and
// LINES * kRevLineWrites chunk sizes per variant.
template <int LINES>
__device__ void roster_review(const ReviewArgs& a)
{
    constexpr int TASKS = 2 * LINES;                      // (line, variant) pairs of a ring
    constexpr int RING = LINES * kRevSlot, WRITES = LINES * kRevLineWrites;
    if ((int)blockIdx.x >= a.q) {       // the blocks past the requested rooms store the pending clears, a room per lane
        const int room = ((int)blockIdx.x - a.q) * kBlock + (int)threadIdx.x;
        if (a.clear && room < a.review_rooms && a.clear[room]) {
            for (int i = 0; i < LINES; i++) a.rings[(size_t)room * RING + i * kRevSlot] = 0;
            a.revline[room] = 0;
        }
        return;
    }
    __shared__ uint8_t s_line[LINES][kRevSlot + 2];       // the ring, oldest line first
    __shared__ uint8_t s_out[TASKS][kRevLineStride];      // task 2 * line + colour: its output
    __shared__ int32_t s_wsz[TASKS][kRevLineWrites + 1];  // its chunk sizes
    __shared__ int s_n[TASKS], s_w[TASKS], s_off[TASKS], s_woff[TASKS];
    __shared__ int s_len[LINES], s_seq;
    const int q = (int)blockIdx.x, room = a.rooms[q];
    const bool cleared = a.clear && a.clear[room];   // then the ring is not read: other blocks are storing its zeros
    const int rev = cleared ? 0 : (int)((uint32_t)a.revline[room] % LINES);
    const uint8_t* ring = a.rings + (size_t)room * RING;
    for (int idx = (int)threadIdx.x; idx < RING; idx += kBlock) {
        const int i = idx / kRevSlot, j = idx - i * kRevSlot;
        const uint8_t v = cleared ? 0 : ring[((rev + i) % LINES) * kRevSlot + j];
        s_line[i][j] = v;
        a.lines[(size_t)q * RING + idx] = v;
    }
    if (threadIdx.x == 0) s_seq = 0;
    __syncthreads();

    const int lane = (int)threadIdx.x & 63;
    for (int t = (int)threadIdx.x >> 6; t < TASKS; t += kBlock / 64) {     // wave-uniform
        const int i = t >> 1;
        const bool colour = (t & 1) != 0;
        const uint8_t* s = s_line[i];
        // this lane's bytes 4 * lane .. + 3 at w[3 .. 6], with three bytes before and two after; 0 outside the slot
        uint8_t w[9];
#pragma unroll
        for (int x = 0; x < 9; x++) {
            const int at = 4 * lane - 3 + x;
            w[x] = at >= 0 && at < kRevSlot ? s[at] : 0;
        }
        // the line ends at its first NUL (byte 201 is one, at the latest): blank everything from there on
        const int nul = w[3] == 0 ? 0 : w[4] == 0 ? 1 : w[5] == 0 ? 2 : w[6] == 0 ? 3 : 4;
        const uint64_t ends = __ballot(nul < 4);
        const int end_lane = __ffsll((unsigned long long)ends) - 1;          // >= 0: lane 50 holds byte 201
        const int len = 4 * end_lane + __shfl(nul, end_lane, 64);
#pragma unroll
        for (int x = 0; x < 9; x++)
            if (4 * lane - 3 + x >= len) w[x] = 0;
        // cmd[x]: the colour command of a command tilde at w[x + 1], the bytes 4 * lane - 2 .. + 3; else -1
        // (key[x]: the two letters after a tilde that is not preceded by '/', as one number)
        int cmd[6], key[6];
        bool tilde = false;
#pragma unroll
        for (int x = 0; x < 6; x++) {
            cmd[x] = -1;
            key[x] = w[x + 1] == '~' && w[x] != '/' ? w[x + 2] << 8 | w[x + 3] : -1;
            tilde |= key[x] >= 0;
        }
        if (tilde) {
#pragma unroll 1
            for (int c = 0; c < kNumCols; c++) {
                const int pair = (uint8_t)kColCom[c][0] << 8 | (uint8_t)kColCom[c][1];
#pragma unroll
                for (int x = 0; x < 6; x++) cmd[x] = key[x] == pair ? c : cmd[x];
            }
        }
        int n[4], mine = 0;
        uint64_t v[4];
#pragma unroll
        for (int x = 0; x < 4; x++) {
            n[x] = expand_byte(w[x + 2], w[x + 3], w[x + 4], cmd[x] >= 0 || cmd[x + 1] >= 0, cmd[x + 2], colour, &v[x]);
            mine += n[x];
        }
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        const int body = __shfl(incl, 63, 64);
        uint8_t* out = s_out[t];
        if (len == 0) {                 // .review skips an empty line: not even a reset
            if (lane == 0) {
                s_n[t] = 0;
                s_w[t] = 0;
            }
        } else if (body <= kWaveLimit) {
            int at = incl - mine;
#pragma unroll
            for (int x = 0; x < 4; x++) {
#pragma unroll
                for (int y = 0; y < 6; y++)      // without a branch: what is not output goes to the row's spare byte
                    out[y < n[x] ? at + y : kRevLineStride - 1] = (uint8_t)(v[x] >> (8 * y));
                at += n[x];
            }
            if (colour && lane < 4) out[body + lane] = lane == 0 ? 27 : lane == 1 ? '[' : lane == 2 ? '0' : 'm';
            if (lane == 0) {            // one write of the body if there is one, then the reset in a write of its own
                int nw = 0;
                if (body) s_wsz[t][nw++] = body;
                if (colour) s_wsz[t][nw++] = 4;
                s_n[t] = body + (colour ? 4 : 0);
                s_w[t] = nw;
            }
        } else if (lane == 0) {
            s_n[t] = -1;                // a flush in mid-line: left to the sequential transducer below
        }
        if (lane == 0 && !colour) s_len[i] = len;
    }
    __syncthreads();
    if (threadIdx.x < TASKS && s_n[threadIdx.x] < 0) {   // the sequential transducer knows the flush rule; a lane each
        const int t = (int)threadIdx.x;
        Sink<true> k{s_out[t], s_wsz[t], kRevLineCap, kRevLineWrites};
        transduce(s_line[t >> 1], s_len[t >> 1], (t & 1) != 0, k);
        if (k.n > kRevLineCap || k.writes > kRevLineWrites) atomicAdd(a.violations, 1);
        s_n[t] = k.n < kRevLineCap ? (int)k.n : kRevLineCap;
        s_w[t] = k.writes < kRevLineWrites ? k.writes : kRevLineWrites;
        atomicAdd(&s_seq, 1);
    }
    __syncthreads();
    if (threadIdx.x < TASKS) {      // each task's place in its variant: after the earlier lines' outputs
        const int t = (int)threadIdx.x;
        int off = 0, woff = 0;
        for (int j = t & 1; j < t; j += 2) {
            off += s_n[j];
            woff += s_w[j];
        }
        s_off[t] = off;
        s_woff[t] = woff;
        if (t >= TASKS - 2) {
            a.vn[2 * q + (t & 1)] = off + s_n[t];
            a.vw[2 * q + (t & 1)] = woff + s_w[t];
        }
    }
    if (threadIdx.x == 64) {
        int lines = 0;
        for (int i = 0; i < LINES; i++) lines += s_len[i] > 0;
        a.line_count[q] = lines;
        a.sequential[q] = s_seq;
    }
    __syncthreads();
    for (int t = 0; t < TASKS; t++) {
        const int var = 2 * q + (t & 1);
        uint8_t* dst = a.var + (size_t)var * rev_var_stride(LINES) + s_off[t];
        for (int j = (int)threadIdx.x; j < s_n[t]; j += kBlock) dst[j] = s_out[t][j];
        if ((int)threadIdx.x < s_w[t]) a.vwsz[var * WRITES + s_woff[t] + (int)threadIdx.x] = s_wsz[t][threadIdx.x];
    }
}

static_assert(kBlock / 64 >= 1 && 64 * 4 >= kRevSlot, "roster_review: a wave holds a whole slot, four bytes per lane");
static_assert(kBlock >= kRevTasks + 64 && kBlock >= kRevLines, "roster_review / roster_record: a lane per task, per line");
static_assert(kTellLines <= kRevLines && kRevVarStride == ((kRevVarCap + 3) & ~3), "the revtell ring is the smaller instance");

// ------------------------------------------------------------------ speech commands of a resident roster
//
// The stage in front of write_room_except: say(), shout(), emote() and semote() (nuts333.c:4062-4226; say / shout /
// emote / semote of oracle/talker_port.c) turn (user, command, inpstr, word_count) into a notice to the speaker, or into
// the speaker's echo and the line its room, or every room, gets.  A roster keeps what they read of a speaker, 16 bytes per
// slot in a device allocation of its own that never moves: 12 name bytes, the name's length, a flags byte (vis, muzzled,
// command_mode), the level (read by nuts_roster_parse alone) and a byte of padding.
//   compose  nuts_roster_speak, one wave per event, four events per block.  The wave reads its speaker's state and decides
//            the outcome in the reference's order, wave-uniformly: muzzled, nothing to say, swearing, spoken.  The swear
//            scan is parallel over the bytes: lane l lowers A-Z in bytes 16l .. 16l+18 (its 16 and 3 of overlap) and
//            tests the three words of nuts333.h:275-277 at its 16 positions; a ballot is the answer.  The verb comes from
//            the last byte.  Both texts are composed with parallel byte copies into the call's composed-text buffer:
//            event k's room line in slot k and its reply in slot K + k, each in_len + kSpeakSlack bytes wide at an offset
//            the host computed (a composed text is at most in_len + 32 bytes; the longest notice, 35 bytes, must fit
//            beside an empty inpstr).  A text that does not exist -- the line of an event that was not spoken, the reply
//            of an emote -- has length -1.  Lane 0 stores the lengths, the outcome, and rm / sender / com / flags (the
//            record bit included) of the room line as nuts_roster_plan and nuts_roster_record take them.
//            When the call uploaded the speaker table, the waves read the upload, and blocks past the events' copy it
//            into the kept allocation for the calls that follow.
//   plan     nuts_roster_speak_plan over the 2K composed texts, sharing stage_variants and admits with nuts_roster_plan:
//            one block per (room line, 256-slot tile) as there, then one block per reply, which has variants only (its
//            admit bitmap, the speaker alone, is the host's).  A text of length -1 is void: nobody is admitted and both
//            variants have 0 bytes in 0 writes -- not the 4-byte reset of an empty text.
//   record   nuts_roster_record, as it is, on the arrays the compose kernel wrote.
//   preset   nd_roster_input's events come from nuts_roster_parse with a verdict each (SpeakArgs.preset; see there): a
//            void event has no text at all, an unknown command has exec_com's reply and no line, a forced "Say what?"
//            skips the muzzle and the mode.  Without a preset array every event is what nd_roster_speak was given.
constexpr int kComSay = 3, kComEmote = 6;                  // enum np_com: NP_SAY, NP_EMOTE
constexpr int kArrSize = 1000;                             // nuts333.h:19 ARR_SIZE: inpstr is at most 999 bytes
constexpr int kSpeakSlack = 36;                            // a composed text's slot is this much wider than inpstr
constexpr int kSpeechRec = 16;                             // bytes of speaker state per slot
constexpr int kNameLen = 12;                               // nuts333.h:23 USER_NAME_LEN
constexpr uint8_t kVis = 1, kMuzzled = 2, kCommandMode = 4;   // the flags byte of a slot's speaker state
constexpr int kSpoken = 0, kOutMuzzled = 1, kOutNothing = 2, kOutSwearing = 3;
constexpr int kSwearSlice = 16;                            // bytes of inpstr per lane in the swear scan
constexpr int kNotSpeech = -1;                             // the outcome of an event that no speech command answers
// what nuts_roster_parse decided of an event before the command functions run (SpeakArgs.preset)
constexpr uint8_t kPresetNone = 0, kPresetVoid = 1, kPresetNothing = 2, kPresetUnknown = 3;

// The composed-text buffer's layout (Python: _composed_at of device/__init__.py).  Text t, whose inpstr starts at
// text_off among the call's, has its slot at ctext_at(text_off, t); room line b is text b, its reply text k + b over
// the same inpstr once more (text_off + text_bytes).  So 2k texts need ctext_at(2 * text_bytes, 2k) bytes.
constexpr int64_t ctext_at(int64_t text_off, int64_t t) { return text_off + kSpeakSlack * t; }

// One of the tables a roster keeps on the device between calls, as a call's kernel sees it (the host's pass_kept fills it).
struct Kept {
    const uint32_t* fresh;       // the upload when the table was passed in this call, to be copied to keep; else nullptr
    uint32_t* keep;              // the kept allocation
    int words;                   // the table's size
};

// The copy tail of such a kernel, a word per lane: word w of the uploads among t, one after the other in that order, into
// its kept allocation.  The loop unrolls, so t is indexed statically and stays in the kernel's arguments.
template <int N>
__device__ __forceinline__ void copy_kept(const Kept (&t)[N], int w)
{
#pragma unroll
    for (int i = 0; i < N; i++) {
        const int n = t[i].fresh ? t[i].words : 0;
        if (w < n) {
            t[i].keep[w] = t[i].fresh[w];
            return;
        }
        w -= n;
    }
}

struct SpeakArgs {
    const int32_t* room;         // [capacity] the roster's table: -1, no room
    const uint8_t* speech;       // [capacity * 16] the speaker state this call reads: the upload, or the kept table
    Kept kept[1];                // the speaker table
    const uint8_t* text;         // the K inpstr, packed
    const int32_t* text_off;     // [k]
    const int32_t* text_len;     // [k]
    const int32_t* slot;         // [k] the speaker
    const uint8_t* com;          // [k] NP_SAY, NP_SHOUT, NP_EMOTE or NP_SEMOTE
    const uint8_t* words;        // [k] word_count
    const uint8_t* preset;       // [k] nuts_roster_parse's verdict; nullptr: every event is a speech event as it stands
    const int32_t* ctext_off;    // [2k] where each composed text's slot starts in ctext
    int k, capacity, blocks;     // blocks: those that compose; the ones after them copy the speaker table
    int ban_swearing, record;
    int* violations;             // composed texts past their slot (zeroed by the host's upload)
    uint8_t* ctext;              // the composed texts
    int32_t* clen;               // [2k] their lengths; -1: no such text
    int32_t* rm;                 // [k] the room line's room (-1: every room), as PlanArgs.rm
    int32_t* sender;             // [k] and its sender (-1: none)
    int32_t* com_num;            // [k]
    uint8_t* flags;              // [k] bit 2: record the room line
    int8_t* outcome;             // [k]
};

struct Piece {
    const uint8_t* p;
    int n;
};
template <int N>
__device__ __forceinline__ Piece lit(const char (&s)[N]) { return {reinterpret_cast<const uint8_t*>(s), N - 1}; }

// np_contains_swearing (nuts333.c:2540-2559) over s[0 .. len), len < kArrSize, by a whole wave.
__device__ __forceinline__ bool swears(const uint8_t* s, int len, int lane)
{
    constexpr uint32_t w0 = 'f' | 'u' << 8 | 'c' << 16 | (uint32_t)'k' << 24;
    constexpr uint32_t w1 = 's' | 'h' << 8 | 'i' << 16 | (uint32_t)'t' << 24;
    constexpr uint32_t w2 = 'c' | 'u' << 8 | 'n' << 16 | (uint32_t)'t' << 24;
    uint32_t low[kSwearSlice + 3];
#pragma unroll
    for (int x = 0; x < kSwearSlice + 3; x++) {
        const int at = kSwearSlice * lane + x;
        const uint32_t c = at < len ? s[at] : 0;
        low[x] = c >= 'A' && c <= 'Z' ? c + 32 : c;          // tolower in the C locale
    }
    bool hit = false;
#pragma unroll
    for (int x = 0; x < kSwearSlice; x++) {
        const uint32_t v = low[x] | low[x + 1] << 8 | low[x + 2] << 16 | low[x + 3] << 24;
        hit |= v == w0 || v == w1 || v == w2;
    }
    return __ballot(hit) != 0;
}

// The five pieces, then body[0 .. blen), then '\n' if newline, into dst by a whole wave; returns the text's length, or -1
// and a violation when it would pass cap.  The pieces are shorter than a wave together: lane i stores their byte i.
__device__ __forceinline__ int compose(uint8_t* dst, int cap, const Piece (&pc)[5], const uint8_t* body, int blen,
                                       bool newline, int lane, int* violations)
{
    const uint8_t* src = nullptr;
    int plen = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        if (lane >= plen && lane < plen + pc[i].n) src = pc[i].p + (lane - plen);
        plen += pc[i].n;
    }
    const int total = plen + blen + (newline ? 1 : 0);
    if (plen > 64 || total > cap) {
        if (lane == 0) atomicAdd(violations, 1);
        return -1;
    }
    if (src) dst[lane] = *src;
    for (int i = lane; i < blen; i += 64) dst[plen + i] = body[i];
    if (newline && lane == 0) dst[plen + blen] = '\n';
    return total;
}

__device__ void roster_speak(const SpeakArgs& a)
{
    if ((int)blockIdx.x >= a.blocks) {      // the speaker table just uploaded, into the kept allocation: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - a.blocks) * kBlock + (int)threadIdx.x);
        return;
    }
    const int lane = (int)threadIdx.x & 63;
    const int k = (int)blockIdx.x * (kBlock / 64) + ((int)threadIdx.x >> 6);      // wave-uniform
    if (k >= a.k) return;
    const uint8_t preset = a.preset ? a.preset[k] : kPresetNone;
    const Piece none{nullptr, 0};
    if (preset == kPresetVoid || preset == kPresetUnknown) {   // no speech command runs: no line, nothing recorded, and
        int reply_len = -1;                                    // exec_com's own notice (c:3763, 3782) or nothing at all
        if (preset == kPresetUnknown) {
            const Piece p[5] = {lit("Unknown command.\n"), none, none, none, none};
            reply_len = compose(a.ctext + a.ctext_off[a.k + k], kSpeakSlack, p, nullptr, 0, false, lane, a.violations);
        }
        if (lane == 0) {
            a.clen[k] = -1;
            a.clen[a.k + k] = reply_len;
            a.rm[k] = a.sender[k] = -1;
            a.com_num[k] = 0;
            a.flags[k] = 0;
            a.outcome[k] = (int8_t)kNotSpeech;
        }
        return;
    }
    const int slot = a.slot[k], com = a.com[k], wc = a.words[k], len = a.text_len[k];
    const uint8_t* in = a.text + a.text_off[k];
    const uint8_t* sp = a.speech + (size_t)slot * kSpeechRec;
    const uint8_t state = sp[kNameLen + 1];
    const int nlen = sp[kNameLen] < kNameLen ? sp[kNameLen] : kNameLen;
    const int room = a.room[slot];
    const uint8_t b0 = len > 0 ? in[0] : 0, b1 = len > 1 ? in[1] : 0, last = len > 0 ? in[len - 1] : 0;
    const bool say = com == kComSay, shout = com == kComShout, emote = com == kComEmote;   // else semote

    // say() c:4068-4082, shout() c:4110-4118, emote() c:4192-4200, semote() c:4216-4221, in their order
    int outcome = kSpoken;
    if (preset == kPresetNothing) outcome = kOutNothing;       // exec_com's "Say what?" (c:3826-3829), before say()
    else if (state & kMuzzled) outcome = kOutMuzzled;
    else if (say ? wc < 2 && (state & kCommandMode) : shout ? wc < 2 : wc < 2 && (int8_t)b1 < 33) outcome = kOutNothing;
    else if (a.ban_swearing && com != kComSemote && swears(in, len, lane)) outcome = kOutSwearing;

    uint8_t* line = a.ctext + a.ctext_off[k];
    uint8_t* reply = a.ctext + a.ctext_off[a.k + k];
    const int cap = len + kSpeakSlack;
    int line_len = -1, reply_len = -1;
    if (outcome == kOutMuzzled) {
        const Piece p[5] = {say ? lit("You are muzzled, you cannot speak.\n") : shout ? lit("You are muzzled, you cannot shout.\n")
                                : lit("You are muzzled, you cannot emote.\n"), none, none, none, none};
        reply_len = compose(reply, cap, p, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kOutNothing) {
        const Piece p[5] = {say ? lit("Say what?\n") : shout ? lit("Shout what?\n") : emote ? lit("Emote what?\n")
                                : lit("Shout emote what?\n"), none, none, none, none};
        reply_len = compose(reply, cap, p, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kOutSwearing) {
        const Piece p[5] = {lit("Swearing is not allowed here.\n"), none, none, none, none};
        reply_len = compose(reply, cap, p, nullptr, 0, false, lane, a.violations);
    } else {
        const Piece name = (state & kVis) ? Piece{sp, nlen} : lit("A presence");      // invisname, nuts333.h:150
        const Piece verb = last == '?' ? lit("ask") : last == '!' ? lit("exclaim") : lit("say");   // c:4080-4082
        if (say) {                          // c:4091-4096
            const Piece r[5] = {lit("You "), none, none, verb, lit(": ")};
            const Piece l[5] = {none, name, lit(" "), verb, lit("s: ")};
            reply_len = compose(reply, cap, r, in, len, true, lane, a.violations);
            line_len = compose(line, cap, l, in, len, true, lane, a.violations);
        } else if (shout) {                 // c:4119-4122
            const Piece r[5] = {lit("~OLYou shout:~RS "), none, none, none, none};
            const Piece l[5] = {lit("~OL"), name, lit(" shouts:~RS "), none, none};
            reply_len = compose(reply, cap, r, in, len, true, lane, a.violations);
            line_len = compose(line, cap, l, in, len, true, lane, a.violations);
        } else {                            // c:4202-4203, c:4223-4224: ";x" and "#x" join the name
            const int skip = b0 == (emote ? ';' : '#') ? 1 : 0;
            const Piece l[5] = {emote ? none : lit("~OL!!~RS "), name, skip ? none : lit(" "), none, none};
            line_len = compose(line, cap, l, in + skip, len - skip, true, lane, a.violations);
        }
        if (line_len < 0 || (reply_len < 0 && (say || shout))) line_len = reply_len = -1;   // a violation: the call fails
    }
    if (lane == 0) {
        const bool spoken = line_len >= 0;
        const bool here = say || emote;     // to the speaker's room, and recorded there; else to every room
        a.clen[k] = line_len;
        a.clen[a.k + k] = reply_len;
        a.rm[k] = spoken && here ? room : -1;
        a.sender[k] = spoken && (say || shout) ? slot : -1;
        a.com_num[k] = com;
        a.flags[k] = spoken && here && a.record ? kRecordBit : 0;
        a.outcome[k] = (int8_t)outcome;
    }
}

static_assert(64 * kSwearSlice >= kArrSize, "roster_speak: the swear scan's 64 slices cover the longest inpstr");
static_assert(kSpeechRec % 4 == 0 && kNameLen + 2 <= kSpeechRec, "roster_speak: a slot's speaker state is whole words");

struct SpeakPlanArgs {
    const int32_t* room;         // [capacity] as PlanArgs
    const uint8_t* slot;         // [capacity]
    const uint8_t* text;         // the 2K composed texts' buffer (SpeakArgs.ctext)
    const int32_t* text_off;     // [2k] SpeakArgs.ctext_off
    const int32_t* text_len;     // [2k] SpeakArgs.clen; -1: void
    const int32_t* rm;           // [k] what nuts_roster_speak wrote
    const int32_t* sender;       // [k]
    const int32_t* com_num;      // [k]
    int k, capacity, tiles, words;
    int* violations;
    int64_t* vn;                 // [4k] bytes of text t's colour-off / colour-on variant; room lines first, then replies
    int32_t* vw;                 // [4k]
    int32_t* vwsz;               // [4k * kMaxWrites]
    uint64_t* bits;              // [k * words] the room lines' admit bitmap
    uint8_t* var;                // text t's variants: var_at(text_off[t], t), and that plus var_stride(len)
};

__device__ void roster_speak_plan(const SpeakPlanArgs& a)
{
    const int lines = a.k * a.tiles;        // the blocks of the room lines; then a block per reply
    int t;
    if ((int)blockIdx.x < lines) {
        const int b = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - b * a.tiles;
        const int j = tile * kBlock + (int)threadIdx.x;
        bool in = false;
        if (j < a.capacity && a.text_len[b] >= 0) {
            const int rm = a.rm[b];
            const uint8_t l = listener_record(a.room[j], a.slot[j], rm, a.sender[b], j);
            in = admits(l, rm < 0, 0, a.com_num[b]);
        }
        const uint64_t word = __ballot(in);
        const int w = j >> 6;
        if ((threadIdx.x & 63) == 0 && w < a.words) a.bits[(int64_t)b * a.words + w] = word;
        if (tile != 0) return;              // block-uniform
        t = b;
    } else {
        t = a.k + ((int)blockIdx.x - lines);
    }
    if (a.text_len[t] < 0) {                // block-uniform: a void text has no variant, not even a reset
        if (threadIdx.x < 2) {
            a.vn[2 * t + threadIdx.x] = 0;
            a.vw[2 * t + threadIdx.x] = 0;
        }
        return;
    }
    store_variants(a, t);
}

static_assert(kArrSize - 1 + kSpeakSlack < kTextSize, "roster_speak_plan: a composed text fits stage_variants' LDS text");

// ------------------------------------------------------------------ client reads of a resident roster
//
// The stage in front of the speech commands: what user_input() and exec_com() do with one read(2) of a client in line
// mode before a command function runs (nuts333.c:136-235, 403-432, 2350-2358, 3753-3831; user_input / exec_com of
// oracle/talker_port.c with np_terminate, np_wordfind, np_remove_first, np_command_lookup and np_command_level of
// oracle/nuts_path.c).  The speaker's level is byte 14 of its 16 bytes of speaker state.
//   parse    nuts_roster_parse, one wave per read, four reads per block; lane l owns bytes 16l .. 16l+15 of the read and
//            keeps two 16-bit masks of them: "ends the line" (the byte as a signed char is below 32) and "word byte"
//            (above 32, and in front of the line's end).  Every position the reference finds with a byte loop is the
//            first set bit at or after some index: a ballot over "my slice has one" gives the lane, that lane's mask the
//            byte (first_from).  So come the line's end n, the first word's start and end, and where np_remove_first
//            stops.  np_wordfind cuts a run of word bytes every 39 bytes, so a word starts where the distance from the
//            run's start is a multiple of 39.  The distance a lane's first byte inherits is a segmented scan over the
//            lanes whose operator carries one flag, "this slice is all word bytes"; it collapses to the nearest lane
//            below that is not, found with a ballot, and that lane's trailing word bytes.  The starts are summed over the
//            wave; ten or more count as nine.
//            The command is the first of the 92 names that begins with comword: lane l tests entries l and l + 64 on
//            names packed into twelve bytes, two ballots and the lowest set bit answer.
//            Lane 0 writes what the caller gets (kind, command, word_count, the line's length, where inpstr starts and
//            its length) and, in place, what nuts_roster_speak reads as its event: the same arrays, and a preset.
//   preset   void: no speech command runs, the event has no text at all.  unknown: the reply is exec_com's
//            "Unknown command.\n".  nothing: a say that came through exec_com with fewer than two words is answered
//            "Say what?" there (c:3826-3829), before say() looks at the muzzle or the mode.
constexpr int kReadSlice = 16;                             // bytes of a read per lane
constexpr int kWordLen = 39;                               // nuts333.h:18 WORD_LEN - 1: the longest word[] entry
constexpr int kMaxWords = 10;                              // nuts333.h:17 MAX_WORDS
constexpr int kLevelByte = kNameLen + 2;                   // the speaker's level in its speaker state
constexpr int kKindIac = 0, kKindEmpty = 1, kKindRepeat = 2, kKindUnknown = 3, kKindSpeech = 4, kKindCommand = 5;
constexpr int kComTell = 5, kComPemote = 8, kComEcho = 9;  // enum np_com: NP_TELL, NP_PEMOTE, NP_ECHO
constexpr int kNumCommands = 92;
constexpr int kNew = 0, kUser = 1, kWiz = 2, kArch = 3, kGod = 4;   // nuts333.h:51-55

// A command: its name's bytes 0 .. 7 in lo, 8 and 9 in the low half of hi, padded with zeros; its level in hi's top byte.
struct Command {
    uint64_t lo;
    uint32_t hi;
};
constexpr Command cmd(const char* name, int level)
{
    Command c{0, (uint32_t)level << 24};
    for (int i = 0; name[i]; i++) {
        if (i < 8) c.lo |= (uint64_t)(uint8_t)name[i] << (8 * i);
        else c.hi |= (uint32_t)(uint8_t)name[i] << (8 * (i - 8));
    }
    return c;
}
// names nuts333.h:157-177, minimum levels nuts333.h:206-226, in enum np_com's order
__constant__ Command kCommands[kNumCommands] = {
    cmd("quit", kNew), cmd("look", kNew), cmd("mode", kNew), cmd("say", kNew), cmd("shout", kUser),
    cmd("tell", kUser), cmd("emote", kUser), cmd("semote", kUser), cmd("pemote", kUser), cmd("echo", kUser),
    cmd("go", kUser), cmd("ignall", kUser), cmd("prompt", kNew), cmd("desc", kUser), cmd("inphr", kUser),
    cmd("outphr", kUser), cmd("public", kUser), cmd("private", kUser), cmd("letmein", kUser), cmd("invite", kUser),
    cmd("topic", kUser), cmd("move", kWiz), cmd("bcast", kWiz), cmd("who", kNew), cmd("people", kWiz),
    cmd("help", kNew), cmd("shutdown", kGod), cmd("news", kUser), cmd("read", kNew), cmd("write", kUser),
    cmd("wipe", kWiz), cmd("search", kUser), cmd("review", kUser), cmd("home", kUser), cmd("status", kNew),
    cmd("version", kNew), cmd("rmail", kNew), cmd("smail", kUser), cmd("dmail", kUser), cmd("from", kUser),
    cmd("entpro", kUser), cmd("examine", kUser), cmd("rmst", kNew), cmd("rmsn", kNew), cmd("netstat", kWiz),
    cmd("netdata", kArch), cmd("connect", kGod), cmd("disconnect", kGod), cmd("passwd", kUser), cmd("kill", kArch),
    cmd("promote", kWiz), cmd("demote", kWiz), cmd("listbans", kWiz), cmd("ban", kArch), cmd("unban", kArch),
    cmd("vis", kArch), cmd("invis", kArch), cmd("site", kWiz), cmd("wake", kUser), cmd("wizshout", kWiz),
    cmd("muzzle", kWiz), cmd("unmuzzle", kWiz), cmd("map", kUser), cmd("logging", kGod), cmd("minlogin", kGod),
    cmd("system", kWiz), cmd("charecho", kNew), cmd("clearline", kArch), cmd("fix", kGod), cmd("unfix", kGod),
    cmd("viewlog", kWiz), cmd("accreq", kNew), cmd("revclr", kUser), cmd("clone", kArch), cmd("destroy", kArch),
    cmd("myclones", kArch), cmd("allclones", kUser), cmd("switch", kArch), cmd("csay", kArch), cmd("chear", kArch),
    cmd("rstat", kWiz), cmd("swban", kArch), cmd("afk", kUser), cmd("cls", kNew), cmd("colour", kNew),
    cmd("ignshout", kUser), cmd("igntell", kUser), cmd("suicide", kNew), cmd("delete", kGod), cmd("reboot", kGod),
    cmd("recount", kGod), cmd("revtell", kUser),
};
constexpr int kNameMax = 10;                               // the longest name, "disconnect"

struct ParseArgs {
    const uint8_t* speech;       // [capacity * 16] the speaker state this call reads, as SpeakArgs.speech
    const uint8_t* data;         // the K reads, packed
    const int32_t* read_off;     // [k]
    const int32_t* read_len;     // [k] 1 .. 1000; the last byte ends the line
    const int32_t* slot;         // [k] the speaker
    int k;
    int8_t* kind;                // [k]
    int8_t* com;                 // [k] the command; -1: none.  SpeakArgs.com
    uint8_t* words;              // [k] word_count.  SpeakArgs.words
    int32_t* line_len;           // [k]
    int32_t* text_off;           // [k] where inpstr starts in data.  SpeakArgs.text_off
    int32_t* text_len;           // [k] inpstr's length; -1: none.  SpeakArgs.text_len
    uint8_t* preset;             // [k] SpeakArgs.preset
};

// The index of the first set bit at or after `from` over the wave's 64 x 16 mask bits, or `none`; wave-uniform.
__device__ __forceinline__ int first_from(uint32_t bits, int from, int lane, int none)
{
    const int rel = from - kReadSlice * lane;
    const uint32_t m = rel >= kReadSlice ? 0u : rel <= 0 ? bits : bits & ~((1u << rel) - 1u);
    const uint64_t b = __ballot(m != 0);
    if (!b) return none;
    return __shfl(kReadSlice * lane + __ffs((int)m) - 1, __ffsll((unsigned long long)b) - 1);
}

__device__ void roster_parse(const ParseArgs& a)
{
    const int lane = (int)threadIdx.x & 63;
    const int k = (int)blockIdx.x * (kBlock / 64) + ((int)threadIdx.x >> 6);      // wave-uniform
    if (k >= a.k) return;
    const int len = a.read_len[k];
    const uint8_t* in = a.data + a.read_off[k];
    const uint8_t* sp = a.speech + (size_t)a.slot[k] * kSpeechRec;
    const bool command_mode = (sp[kNameLen + 1] & kCommandMode) != 0;
    const int level = sp[kLevelByte];

    uint32_t ends = 0, wordb = 0;           // a byte past the read counts as 0: it ends the line
#pragma unroll
    for (int x = 0; x < kReadSlice; x++) {
        const int at = kReadSlice * lane + x;
        const int c = at < len ? (int)(int8_t)in[at] : 0;
        ends |= (uint32_t)(c < 32) << x;
        wordb |= (uint32_t)(c > 32) << x;
    }
    const int n = first_from(ends, 0, lane, len);                                  // np_terminate, c:403-411
    const int live = n - kReadSlice * lane;
    wordb &= live >= kReadSlice ? 0xffffu : live <= 0 ? 0u : (1u << live) - 1u;

    // np_wordfind, c:417-432: the distance my first byte inherits, then the word starts of my slice
    const uint64_t full = __ballot(wordb == 0xffffu);
    const uint64_t broken = ~full & ((1ull << lane) - 1);                          // lanes below me that end a run
    const int prev = broken ? 63 - __clzll((long long)broken) : -1;
    const int tail = __shfl(__clz((int)~(wordb << 16)), prev < 0 ? 0 : prev);      // that lane's trailing word bytes
    const int carry = prev < 0 ? kReadSlice * lane : kReadSlice * (lane - 1 - prev) + tail;
    int dist = carry % kWordLen, total = 0;
#pragma unroll
    for (int x = 0; x < kReadSlice; x++) {
        if (wordb >> x & 1) {
            total += dist == 0;
            dist = dist == kWordLen - 1 ? 0 : dist + 1;
        } else {
            dist = 0;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) total += __shfl_xor(total, d);
    const int wc = total >= kMaxWords ? kMaxWords - 1 : total;

    const uint8_t b0 = in[0];
    int kind, com = -1, start = 0, ilen = -1;
    uint8_t preset = kPresetVoid;
    if (b0 == 255) {                                                               // telnet IAC, c:150s
        kind = kKindIac;
    } else if (n == 1 && b0 == '.') {                                              // c:185: the caller's inpstr_old
        kind = kKindRepeat;
    } else if (total == 0) {                                                       // c:207-211
        kind = kKindEmpty;
    } else if (!command_mode && b0 != '.' && b0 != ';' && b0 != '!' && b0 != '<' && b0 != '>' && b0 != '-' && b0 != '#') {
        kind = kKindSpeech;                                                        // c:213-214: say(user, inpstr)
        com = kComSay;
        ilen = n;
        preset = kPresetNone;
    } else {                                                                       // exec_com, c:3753-3785
        const int w0 = first_from(wordb, 0, lane, n);                              // word[0]: there is one
        const int w0_end = first_from(~wordb & 0xffffu, w0, lane, n);
        const int rest = first_from(wordb, w0_end, lane, n);                       // np_remove_first, c:2350-2358
        const int wlen = w0_end - w0 < kWordLen ? w0_end - w0 : kWordLen;
        const uint8_t first = in[w0];
        const int cw = w0 + (first == '.' ? 1 : 0), cwlen = w0 + wlen - cw;        // comword
        kind = kKindUnknown;
        preset = kPresetUnknown;
        if (cwlen > 0) {
            const bool whole = b0 == ';' || b0 == '#';                             // c:3769-3771: inpstr stays whole
            if (whole) {
                com = b0 == ';' ? kComEmote : kComSemote;
            } else if (wlen == 1 && (first == '>' || first == '<' || first == '-' || first == '!')) {
                com = first == '>' ? kComTell : first == '<' ? kComPemote : first == '-' ? kComEcho : kComShout;
            } else if (cwlen <= kNameMax) {                                        // np_command_lookup, c:3776-3781
                uint64_t lo = 0;
                uint32_t hi = 0;
#pragma unroll
                for (int i = 0; i < kNameMax; i++) {
                    const uint64_t c = i < cwlen ? in[cw + i] : 0;
                    if (i < 8) lo |= c << (8 * i);
                    else hi |= (uint32_t)c << (8 * (i - 8));
                }
                const uint64_t mlo = cwlen >= 8 ? ~0ull : (1ull << (8 * cwlen)) - 1;
                const uint32_t mhi = cwlen <= 8 ? 0u : (1u << (8 * (cwlen - 8))) - 1u;
                const Command e0 = kCommands[lane];
                const Command e1 = kCommands[lane + 64 < kNumCommands ? lane + 64 : 0];
                const uint64_t hit0 = __ballot((e0.lo & mlo) == lo && (e0.hi & mhi) == hi);
                const uint64_t hit1 = __ballot(lane + 64 < kNumCommands && (e1.lo & mlo) == lo && (e1.hi & mhi) == hi);
                com = hit0 ? __ffsll((unsigned long long)hit0) - 1 : hit1 ? 64 + __ffsll((unsigned long long)hit1) - 1 : -1;
            }
            if (com >= 0 && (int)(kCommands[com].hi >> 24) > level) com = -1;      // c:3782: as if there were none
            if (com >= 0) {
                const bool speech = com == kComSay || com == kComShout || com == kComEmote || com == kComSemote;
                kind = speech ? kKindSpeech : kKindCommand;
                preset = !speech ? kPresetVoid : com == kComSay && wc < 2 ? kPresetNothing : kPresetNone;
                start = whole ? 0 : rest;
                ilen = n - start;
            }
        }
    }
    if (lane == 0) {
        a.kind[k] = (int8_t)kind;
        a.com[k] = (int8_t)com;
        a.words[k] = (uint8_t)wc;
        a.line_len[k] = n;
        a.text_off[k] = a.read_off[k] + start;
        a.text_len[k] = ilen;
        a.preset[k] = preset;
    }
}

static_assert(64 * kReadSlice >= kArrSize + 1, "roster_parse: the 64 slices cover the longest read and a byte past it");
static_assert(kNumCommands <= 128 && kLevelByte < kSpeechRec, "roster_parse: two table entries per lane; the level's byte");

// ------------------------------------------------------------------ private speech of a resident roster
//
// tell() and pemote() (nuts333.c:4128-4182, 4230-4281; tell / pemote / private_blocked of oracle/talker_port.c) turn (user,
// command, inpstr, word_count) into a notice to the speaker, or into the speaker's echo and the line one other user gets:
// the one get_user() finds (nuts333.c:2362-2379), by an exact-name pass and then a substring pass over the user list, here
// the slots in ascending order.  A slot's speaker state carries two more flags for it, afk and igntell (bits 8 and 16 of
// the flags byte), and a third table kept like the speaker state holds every slot's AFK message: 64 bytes per slot, 60 of
// message padded with zeros, then its length.
//   tell     nuts_roster_tell, ONE BLOCK PER EVENT, because the lookup is the work: it reads every slot once, and a block
//            has four waves to spread the slots over where a wave per event would walk them alone.  Per event that is
//            `capacity` 16-byte speaker records and `capacity` flag bytes (login lives in the table's flags byte): 1000
//            and 1000 at capacity 1000 in 4 steps of the block (16 of a single wave), 65536 and 65536 at capacity 65536 in
//            256 steps (1024).  A slot's room is read for the slot that was found alone: get_user does not look at it.
//            An event that never reaches get_user (muzzled, too few words, a pemote to one's own exact name) reads none.
//            word[1] is found as nuts_roster_parse finds words (16 bytes of inpstr per lane, first_from), by every wave
//            for itself; its first 12 bytes are packed as a name is, the first one capitalised.  Lane l of wave w tests
//            slot 256 i + 64 w + l in step i: the name equals the word (same length, same bytes), or holds it at one of
//            the 13 - length offsets.  Two ballots per step; the first set bit of the first non-empty ballot is the wave's
//            lowest match, a wave that has an exact match stops (a substring match no longer matters), and the four
//            waves' two minima meet in LDS.  No atomics: the same answer on every run.
//            Wave 0 then decides the outcome in the reference's order and composes both texts with compose(), told line k
//            in slot k and its reply in slot K + k of the composed-text buffer, each in_len + kTellSlack bytes wide (a
//            composed text is at most in_len + 38 bytes, the AFK notice up to 94 whatever inpstr holds).  Lane 0 stores
//            the lengths, the outcome, the target, and for nuts_roster_record_tell the ring (the target of a told event,
//            else -1) and the record bit.  Blocks past the events copy an uploaded speaker or AFK-message table into the
//            kept allocation, as nuts_roster_speak's do.
//   plan     both texts need variants only: nuts_roster_speak_plan with no room lines (k = 0), a block per text.
//   record   nuts_roster_record_tell is roster_record<5> over the slots' revtell rings, a block per slot, each scanning the
//            call's K (record bit, target) pairs; nuts_roster_revtell is roster_review<5>.
constexpr int kTellSlack = 96;                             // a composed private text's slot is this much wider than inpstr
constexpr int kAfkRec = 64, kAfkMesgLen = 60;              // a slot's AFK message row; nuts333.h:25 AFK_MESG_LEN
constexpr uint8_t kAfk = 8, kIgntell = 16;                 // more bits of the flags byte of a slot's speaker state
constexpr int kTold = 0, kOutNobody = 4, kOutSelf = 5, kOutAfk = 6, kOutIgnall = 7, kOutIgntell = 8, kOutOffsite = 9;
constexpr int kNoMatch = 0x7fffffff;

constexpr int64_t ptext_at(int64_t text_off, int64_t t) { return text_off + kTellSlack * t; }   // ctext_at, for these texts

struct TellArgs {
    const int32_t* room;         // [capacity] the roster's table: -1, no room
    const uint8_t* slotf;        // [capacity] and its flags byte: kLogin, kIgnall
    const uint8_t* speech;       // [capacity * 16] the speaker state this call reads: the upload, or the kept table
    const uint8_t* afk;          // [capacity * 64] the AFK messages, likewise
    Kept kept[2];                // the speaker table, the AFK messages
    const uint8_t* text;         // the K inpstr, packed
    const int32_t* text_off;     // [k]
    const int32_t* text_len;     // [k]
    const int32_t* slot;         // [k] the speaker
    const uint8_t* com;          // [k] NP_TELL or NP_PEMOTE
    const uint8_t* words;        // [k] word_count
    const int32_t* ctext_off;    // [2k] where each composed text's slot starts in ctext
    int k, capacity, record;
    int* violations;             // composed texts past their slot (zeroed by the host's upload)
    uint8_t* ctext;              // the composed texts
    int32_t* clen;               // [2k] their lengths; -1: no such text
    int8_t* outcome;             // [k]
    int32_t* target;             // [k] the slot get_user found; -1: none, or it was not asked
    int32_t* ring;               // [k] RecordArgs.rm of nuts_roster_record_tell: the target of a told event, else -1
    uint8_t* flags;              // [k] bit 2: record the told line
};

// Does a name (its 12 bytes in lo and hi, padded with zeros, nlen of them used) equal the word (its wlen <= 12 bytes packed
// alike, none of them zero), and does it contain it?  The padding is zero, so a match never runs past the name's end.
__device__ __forceinline__ void name_match(uint64_t lo, uint32_t hi, int nlen, uint64_t wlo, uint32_t whi, int wlen,
                                           bool* exact, bool* sub)
{
    const uint64_t mlo = wlen >= 8 ? ~0ull : (1ull << (8 * wlen)) - 1;
    const uint32_t mhi = wlen <= 8 ? 0u : wlen >= 12 ? ~0u : (1u << (8 * (wlen - 8))) - 1u;
    bool any = false;
#pragma unroll
    for (int o = 0; o <= kNameLen; o++) {                  // the name from its byte o on
        const uint64_t slo = o == 0 ? lo : o < 8 ? lo >> (8 * o) | (uint64_t)hi << (64 - 8 * o) : o < 12 ? (uint64_t)(hi >> (8 * (o - 8))) : 0;
        const uint32_t shi = o == 0 ? hi : o < 4 ? hi >> (8 * o) : 0u;
        const bool hit = o + wlen <= nlen && (slo & mlo) == wlo && (shi & mhi) == whi;
        if (o == 0) *exact = hit && wlen == nlen;
        any |= hit;
    }
    *sub = any;
}

// A word's first 12 bytes packed as a name is, the first one capitalised (get_user c:2366, pemote c:4243).
struct NameWord {
    uint64_t lo;
    uint32_t hi;
};
__device__ __forceinline__ NameWord pack_word(const uint8_t* word, int wlen)
{
    NameWord w{0, 0};
#pragma unroll
    for (int i = 0; i < kNameLen; i++) {
        uint64_t c = i < wlen ? word[i] : 0;
        if (i == 0 && c >= 'a' && c <= 'z') c -= 32;
        if (i < 8) w.lo |= c << (8 * i);
        else w.hi |= (uint32_t)c << (8 * (i - 8));
    }
    return w;
}

// get_user (c:2362-2379) for one wave of a block: its lowest exact match and its lowest substring match among the slots
// 64 wave + 256 i + lane that have a name and no login flag; kNoMatch where there is none.  A wave that has an exact match
// stops: a substring match no longer matters.  Wave-uniform; the block's waves meet in LDS.
struct UserMatch {
    int exact, sub;
};
__device__ __forceinline__ UserMatch wave_get_user(const uint8_t* speech, const uint8_t* slotf, int capacity, NameWord w, int wlen,
                                                   int wave, int lane)
{
    UserMatch best{kNoMatch, kNoMatch};
    if (wlen <= kNameLen) {
        for (int base = 64 * wave; base < capacity; base += kBlock) {
            const int j = base + lane;
            bool exact = false, sub = false;
            if (j < capacity && !(slotf[j] & kLogin)) {
                const uint4 rec = reinterpret_cast<const uint4*>(speech)[j];
                const int jl = (int)(rec.w & 0xff) < kNameLen ? (int)(rec.w & 0xff) : kNameLen;
                if (jl > 0) name_match(rec.x | (uint64_t)rec.y << 32, rec.z, jl, w.lo, w.hi, wlen, &exact, &sub);
            }
            const uint64_t be = __ballot(exact);
            if (be) {
                best.exact = base + __ffsll((unsigned long long)be) - 1;
                break;
            }
            const uint64_t bs = __ballot(sub);
            if (bs && best.sub == kNoMatch) best.sub = base + __ffsll((unsigned long long)bs) - 1;
        }
    }
    return best;
}

__device__ void roster_tell(const TellArgs& a)
{
    if ((int)blockIdx.x >= a.k) {           // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - a.k) * kBlock + (int)threadIdx.x);
        return;
    }
    __shared__ int s_exact[kBlock / 64], s_sub[kBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int k = (int)blockIdx.x;
    const int slot = a.slot[k], wc = a.words[k], len = a.text_len[k];
    const bool pemote = a.com[k] == kComPemote;
    const uint8_t* in = a.text + a.text_off[k];
    const uint8_t* sp = a.speech + (size_t)slot * kSpeechRec;
    const uint8_t state = sp[kNameLen + 1];
    const int nlen = sp[kNameLen] < kNameLen ? sp[kNameLen] : kNameLen;

    // word[1] as np_wordfind finds the line's second word, and where np_remove_first leaves inpstr (c:417-432, 2350-2358)
    uint32_t wordb = 0;
#pragma unroll
    for (int x = 0; x < kReadSlice; x++) {
        const int at = kReadSlice * lane + x;
        wordb |= (uint32_t)(at < len && (int8_t)in[at] > 32) << x;
    }
    const int w0 = first_from(wordb, 0, lane, len);
    const int w0_end = first_from(~wordb & 0xffffu, w0, lane, len);                // <= len: the byte at len is no word byte
    const int rest = first_from(wordb, w0_end, lane, len);
    const int wlen = w0_end - w0 < kWordLen ? w0_end - w0 : kWordLen;
    const NameWord nw = pack_word(in + w0, wlen);
    const uint64_t wlo = nw.lo;
    const uint32_t whi = nw.hi;

    // what comes before get_user, in the reference's order (tell c:4133-4140, pemote c:4235-4247); block-uniform
    int outcome = kTold;
    if (state & kMuzzled) outcome = kOutMuzzled;
    else if (wc < 3) outcome = kOutNothing;
    else if (pemote && wlen == nlen) {
        const uint32_t* n = reinterpret_cast<const uint32_t*>(sp);
        bool exact, sub;
        name_match(n[0] | (uint64_t)n[1] << 32, n[2], nlen, wlo, whi, wlen, &exact, &sub);
        if (exact) outcome = kOutSelf;
    }

    // get_user: this wave's lowest exact match and lowest substring match among its slots, 64 w + 256 i + lane
    int best_exact = kNoMatch, best_sub = kNoMatch;
    if (outcome == kTold) {
        const UserMatch m = wave_get_user(a.speech, a.slotf, a.capacity, nw, wlen, wave, lane);
        best_exact = m.exact;
        best_sub = m.sub;
    }
    if (lane == 0) {
        s_exact[wave] = best_exact;
        s_sub[wave] = best_sub;
    }
    __syncthreads();
    if (wave != 0) return;
    for (int w = 0; w < kBlock / 64; w++) {
        best_exact = s_exact[w] < best_exact ? s_exact[w] : best_exact;
        best_sub = s_sub[w] < best_sub ? s_sub[w] : best_sub;
    }
    int target = -1;
    const uint8_t* tp = sp;                 // the target's speaker state
    if (outcome == kTold) {
        target = best_exact != kNoMatch ? best_exact : best_sub != kNoMatch ? best_sub : -1;
        if (target < 0) {
            outcome = kOutNobody;
        } else if (!pemote && target == slot) {
            outcome = kOutSelf;
        } else {                            // private_blocked, c:4149-4172 / 4251-4273
            tp = a.speech + (size_t)target * kSpeechRec;
            const int mine = sp[kLevelByte], theirs = tp[kLevelByte];
            const bool deaf = mine < kWiz || theirs > mine;
            if (tp[kNameLen + 1] & kAfk) outcome = kOutAfk;
            else if ((a.slotf[target] & kIgnall) && deaf) outcome = kOutIgnall;
            else if ((tp[kNameLen + 1] & kIgntell) && deaf) outcome = kOutIgntell;
            else if (a.room[target] < 0) outcome = kOutOffsite;
        }
    }

    uint8_t* line = a.ctext + a.ctext_off[k];
    uint8_t* reply = a.ctext + a.ctext_off[a.k + k];
    const int cap = len + kTellSlack;
    const Piece none{nullptr, 0};
    const Piece tname{tp, tp[kNameLen] < kNameLen ? tp[kNameLen] : kNameLen};
    int line_len = -1, reply_len = -1;
    if (outcome == kTold) {
        const Piece shown = (state & kVis) ? Piece{sp, nlen} : lit("A presence");
        const uint8_t* body = in + rest;
        const int blen = len - rest;
        if (pemote) {                       // c:4275-4279
            const Piece r[5] = {lit("~OL(To "), tname, lit(")~RS "), shown, lit(" ")};
            const Piece l[5] = {lit("~OL>>~RS "), shown, lit(" "), none, none};
            reply_len = compose(reply, cap, r, body, blen, true, lane, a.violations);
            line_len = compose(line, cap, l, body, blen, true, lane, a.violations);
        } else {                            // c:4174-4180
            const Piece verb = blen > 0 && body[blen - 1] == '?' ? lit("ask") : lit("tell");
            const Piece r[5] = {lit("~OLYou "), verb, lit(" "), tname, lit(":~RS ")};
            const Piece l[5] = {lit("~OL"), shown, lit(" "), verb, lit("s you:~RS ")};
            reply_len = compose(reply, cap, r, body, blen, true, lane, a.violations);
            line_len = compose(line, cap, l, body, blen, true, lane, a.violations);
        }
        if (line_len < 0 || reply_len < 0) line_len = reply_len = -1;              // a violation: the call fails
    } else if (outcome == kOutAfk) {
        const uint8_t* mesg = a.afk + (size_t)target * kAfkRec;
        const int mlen = mesg[kAfkMesgLen] < kAfkMesgLen ? mesg[kAfkMesgLen] : kAfkMesgLen;
        const Piece p[5] = {tname, mlen ? lit(" is AFK, message is: ") : lit(" is AFK at the moment."), none, none, none};
        reply_len = compose(reply, cap, p, mesg, mlen, true, lane, a.violations);
    } else if (outcome == kOutIgnall) {
        const Piece p[5] = {tname, lit(" is ignoring everyone at the moment.\n"), none, none, none};
        reply_len = compose(reply, cap, p, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kOutIgntell) {
        const Piece p[5] = {tname, lit(" is ignoring "), pemote ? lit("private emotes") : lit("tells"), lit(" at the moment.\n"), none};
        reply_len = compose(reply, cap, p, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kOutOffsite) {
        const Piece p[5] = {tname, lit(" is offsite and would not be able to reply to you.\n"), none, none, none};
        reply_len = compose(reply, cap, p, nullptr, 0, false, lane, a.violations);
    } else {
        const Piece p[5] = {outcome == kOutMuzzled ? (pemote ? lit("You are muzzled, you cannot emote.\n")
                                                             : lit("You are muzzled, you cannot tell anyone anything.\n"))
                            : outcome == kOutNothing ? (pemote ? lit("Private emote what?\n") : lit("Tell who what?\n"))
                            : outcome == kOutNobody ? lit("There is no one of that name logged on.\n")
                            : pemote ? lit("Emoting to yourself is the second sign of madness.\n")
                                     : lit("Talking to yourself is the first sign of madness.\n"), none, none, none, none};
        reply_len = compose(reply, cap, p, nullptr, 0, false, lane, a.violations);
    }
    if (lane == 0) {
        const bool told = line_len >= 0;
        a.clen[k] = line_len;
        a.clen[a.k + k] = reply_len;
        a.outcome[k] = (int8_t)outcome;
        a.target[k] = target;
        a.ring[k] = told ? target : -1;
        a.flags[k] = told && a.record ? kRecordBit : 0;
    }
}

static_assert(kAfkRec % 4 == 0 && kAfkMesgLen < kAfkRec, "roster_tell: an AFK message row is whole words and holds its length");
static_assert(kArrSize - 1 + kTellSlack < kTextSize, "nuts_roster_speak_plan: a composed private text fits its LDS text");
static_assert(kNameLen + 22 + 1 <= 64, "compose: the pieces of the longest notice fit a wave");

// ------------------------------------------------------------------ look() of a resident roster
//
// look() (nuts333.c:3942-4004) sends a user its room: five texts that depend on the room alone -- the name, the
// description, the exits, the access sentence with the board's message count, the topic -- and between the third and the
// fourth "You can see:" and one line per user it can see there, or "You are all alone here.", then "\n".  A user's line
// depends on that user alone (name, description, visible or not, AFK); who is listed depends on both: every user of the
// room in list order, here the slots in ascending order, but the looker itself, a slot without a name, and an invisible
// user above the looker's level.  So a call has, like a delivery plan, texts with two variants each and per looker a
// list of them: the five texts of every distinct room, the three fixed ones, and one line per named slot of those rooms,
// each transduced once however many lookers list it.
// A roster with look_rooms > 0 keeps two more tables for it, like the speaker state in device allocations of their own
// that never move: a room table, one 256-byte record per room and then one 816-byte description row per room, and 32
// bytes of description per slot.
//   room record   0 name[20] | 20 its length | 21 access (PUBLIC 0, PRIVATE 1, FIXED_PUBLIC 2, FIXED_PRIVATE 3) |
//                 22 links | 23 the topic's length | 24 netlink (bit 0: a link that is UP, bit 1: allow == IN) |
//                 25 the service's length | 26 the description's length, 2 bytes | 28 mesg_cnt, 4 bytes |
//                 32 link[10], 4 bytes each | 72 topic[60] | 132 service[80] | 212 zeros
//   desc row      0 desc[810] | zeros
//   slot row      0 desc[30] | 30 its length | 31 zero
//   look     nuts_roster_look, one launch whose blocks take roles by their index:
//            ROOM BLOCKS, one per distinct room of the call.  Wave 0 composes the five room texts with compose() into the
//            room's five slots of the composed-text buffer (36, 812, 352, 96 and 80 bytes wide, their longest forms), the
//            exits link by link, and the digits of mesg_cnt a lane each; the first room's also the three fixed texts.
//            Then the block walks the roster, lane l of wave w on slot 256 i + 64 w + l in step i: a slot of the room
//            that has a name is a candidate, and its rank among the room's candidates -- a ballot per wave, the four
//            waves' counts through LDS, a carry over the steps -- is its line's number.  The lane composes the line (at
//            most 69 bytes) into that line's 72-byte slot of the buffer, whole: a description ending in '/' makes the ~RS
//            after it literal, so the transducer has to see the line as one text.  The host, which knows each room's
//            population, gives every room its range of lines; the lines of the range that no candidate took are void.
//            LOOKER BLOCKS, one per looker, walk the roster the same way: the same candidate ranks, and a second ballot
//            for the candidates this looker is shown.  Looker b's members -- the slot and its line -- go to
//            members[m_off[b] ..] and mline[m_off[b] ..] in slot order, the count to nmem[b].  No atomics anywhere:
//            the same result on every run.
//            COPY BLOCKS past those copy freshly uploaded tables into the kept allocations.
//   plan     nuts_roster_speak_plan with no room lines (k = 0), a block per text: both variants and their writes.
//            The transducer is not called from nuts_roster_look: inlined into a loop over the slots it leaves the
//            compiler too few scalar registers, and the kernels here are built without spills.
constexpr int kRoomRec = 256, kRoomDescRow = 816, kUserDescRow = 32;
constexpr int kRoomRow = kRoomRec + kRoomDescRow;          // a room's bytes in the room table
constexpr int kRoomNameLen = 20, kRoomDescLen = 810, kTopicLen = 60, kMaxLinks = 10, kServNameLen = 80, kUserDescLen = 30;
constexpr int kRrNameLen = 20, kRrAccess = 21, kRrLinks = 22, kRrTopicLen = 23, kRrNet = 24, kRrServLen = 25, kRrDescLen = 26,
              kRrMesgCnt = 28, kRrLink = 32, kRrTopic = 72, kRrServ = 132;
constexpr int kMaxLookRooms = 1024;
constexpr int kLookTexts = 5;                              // the room texts: name, description, exits, access, topic
constexpr int kLookTextStride = 1376;                      // a room's five slots in the composed-text buffer
constexpr int look_text_at(int i) { return i == 0 ? 0 : i == 1 ? 36 : i == 2 ? 848 : i == 3 ? 1200 : 1296; }
constexpr int look_text_cap(int i) { return (i == 4 ? kLookTextStride : look_text_at(i + 1)) - look_text_at(i); }
constexpr int kLookFixed = 3;                              // "You can see:", "You are all alone here.", "\n"
constexpr int kLookFixedStride = 48;                       // their slots: 16, 28 and 4 bytes
constexpr int look_fixed_at(int i) { return i == 0 ? 0 : i == 1 ? 16 : 44; }
constexpr int kLineRow = 72;                               // a member line's slot: the longest line is 69 bytes

// The composed-text buffer of a look call over nr rooms and nl lines: the rooms' texts, the fixed ones, the lines.
constexpr int64_t look_ctext_bytes(int64_t nr, int64_t nl) { return nr * kLookTextStride + kLookFixedStride + nl * kLineRow; }

struct LookArgs {
    const int32_t* room;         // [capacity] the roster's table: -1, no room
    const uint8_t* speech;       // [capacity * 16] the speaker state this call reads: the upload, or the kept table
    const uint8_t* rooms;        // [look_rooms * 256] the room records, then [look_rooms * 816] the descriptions; likewise
    const uint8_t* udesc;        // [capacity * 32] the users' descriptions, likewise
    Kept kept[3];                // the speaker table, the room table, the descriptions
    const int32_t* slot;         // [k] the lookers
    const int32_t* lroom;        // [k] their rooms, as indices into rms
    const int32_t* rms;          // [nr] the distinct rooms of the call
    const int32_t* line_off;     // [nr + 1] room i owns lines line_off[i] .. line_off[i + 1] - 1
    const int32_t* m_off;        // [k + 1] looker b owns members m_off[b] .. m_off[b + 1] - 1
    const int32_t* ctext_off;    // [5 nr + 3 + nl] where each text's slot starts in ctext
    int k, nr, capacity, look_rooms;
    int* violations;             // texts past their slots, lines and members past their ranges (zeroed by the host's upload)
    int32_t* nmem;               // [k] the members listed
    int32_t* nline;              // [nr] the lines composed
    int32_t* clen;               // [5 nr + 3 + nl] the texts' lengths; -1: a line nobody took
    uint8_t* ctext;              // the texts
    int32_t* members;            // the listed slots, looker by looker
    int32_t* mline;              // and their lines
    int32_t* line_slot;          // [nl] the slot each line is of
};
// One more compose() behind what a text already holds: at is its length so far, or -1 after a violation.
__device__ __forceinline__ void append(uint8_t* dst, int cap, int& at, const Piece (&pc)[5], const uint8_t* body, int blen,
                                       bool newline, int lane, int* violations)
{
    if (at < 0) return;
    const int n = compose(dst + at, cap - at, pc, body, blen, newline, lane, violations);
    at = n < 0 ? -1 : at + n;
}

// The five texts of room a.rms[r], by one wave.
__device__ void look_room(const LookArgs& a, int r, int lane)
{
    const int rm = a.rms[r];
    const uint8_t* rec = a.rooms + (size_t)rm * kRoomRec;
    const uint8_t* desc = a.rooms + (size_t)a.look_rooms * kRoomRec + (size_t)rm * kRoomDescRow;
    const Piece none{nullptr, 0};
    const int nlen = rec[kRrNameLen] < kRoomNameLen ? rec[kRrNameLen] : kRoomNameLen;
    const int access = rec[kRrAccess] & 3, nlinks = rec[kRrLinks] < kMaxLinks ? rec[kRrLinks] : kMaxLinks;
    const int tlen = rec[kRrTopicLen] < kTopicLen ? rec[kRrTopicLen] : kTopicLen;
    const int net = rec[kRrNet], slen = rec[kRrServLen] < kServNameLen ? rec[kRrServLen] : kServNameLen;
    const int dl = rec[kRrDescLen] | rec[kRrDescLen + 1] << 8, dlen = dl < kRoomDescLen ? dl : kRoomDescLen;
    const int32_t cnt = *reinterpret_cast<const int32_t*>(rec + kRrMesgCnt);
    const int32_t* at = a.ctext_off + kLookTexts * r;
    int32_t* clen = a.clen + kLookTexts * r;
    {   // c:3952-3955
        int len = 0;
        const Piece p[5] = {lit("\n~FTRoom: "), (access & 1) ? lit("~FR") : lit("~FG"), Piece{rec, nlen}, lit("\n\n"), none};
        append(a.ctext + at[0], look_text_cap(0), len, p, nullptr, 0, false, lane, a.violations);
        if (lane == 0) clen[0] = len;
        len = 0;
        const Piece q[5] = {none, none, none, none, none};
        append(a.ctext + at[1], look_text_cap(1), len, q, desc, dlen, false, lane, a.violations);
        if (lane == 0) clen[1] = len;
    }
    {   // c:3956-3973
        uint8_t* t = a.ctext + at[2];
        int len = 0;
        int exits = 0;
        const Piece head[5] = {lit("\n~FTExits are:"), none, none, none, none};
        append(t, look_text_cap(2), len, head, nullptr, 0, false, lane, a.violations);
        for (int i = 0; i < nlinks; i++) {
            const int32_t l = *reinterpret_cast<const int32_t*>(rec + kRrLink + 4 * i);
            if (l < 0 || l >= a.look_rooms) {           // the host has checked them: never past the table
                if (lane == 0) atomicAdd(a.violations, 1);
                len = -1;
                break;
            }
            const uint8_t* lrec = a.rooms + (size_t)l * kRoomRec;
            const int ll = lrec[kRrNameLen] < kRoomNameLen ? lrec[kRrNameLen] : kRoomNameLen;
            const Piece p[5] = {(lrec[kRrAccess] & 1) ? lit("  ~FR") : lit("  ~FG"), none, none, none, none};
            append(t, look_text_cap(2), len, p, lrec, ll, false, lane, a.violations);
            exits++;
        }
        if (net & 1) {
            const Piece p[5] = {(net & 2) ? lit("  ~FR") : lit("  ~FG"), none, none, none, none};
            append(t, look_text_cap(2), len, p, rec + kRrServ, slen, false, lane, a.violations);
            const Piece star[5] = {lit("*"), none, none, none, none};
            append(t, look_text_cap(2), len, star, nullptr, 0, false, lane, a.violations);
        } else if (!exits && len >= 0) {
            len = 0;
            const Piece p[5] = {lit("\n~FTThere are no exits."), none, none, none, none};
            append(t, look_text_cap(2), len, p, nullptr, 0, false, lane, a.violations);
        }
        const Piece tail[5] = {lit("\n\n"), none, none, none, none};
        append(t, look_text_cap(2), len, tail, nullptr, 0, false, lane, a.violations);
        if (lane == 0) clen[2] = len;
    }
    {   // c:3988-3997
        const Piece how = access == 0 ? lit("set to ~FGPUBLIC~RS") : access == 1 ? lit("set to ~FRPRIVATE~RS")
                          : access == 2 ? lit("~FRfixed~RS to ~FGPUBLIC~RS") : lit("~FRfixed~RS to ~FRPRIVATE~RS");
        uint8_t* t = a.ctext + at[3];
        int len = 0;
        const Piece p[5] = {lit("Access is "), how, lit(" and there are ~OL~FM"), none, none};
        append(t, look_text_cap(3), len, p, nullptr, 0, false, lane, a.violations);
        const uint32_t v = cnt > 0 ? (uint32_t)cnt : 0u;   // %d: a lane per digit
        int digits = 1;
        for (uint32_t x = v; x >= 10; x /= 10) digits++;
        if (len >= 0 && len + digits <= look_text_cap(3)) {
            uint32_t x = v;
            for (int i = digits - 1; i > lane; i--) x /= 10;
            if (lane < digits) t[len + lane] = (uint8_t)('0' + x % 10);
            len += digits;
        } else {
            len = -1;
        }
        const Piece q[5] = {lit("~RS messages on the board.\n"), none, none, none, none};
        append(t, look_text_cap(3), len, q, nullptr, 0, false, lane, a.violations);
        if (lane == 0) clen[3] = len;
    }
    {   // c:3998-4003
        const Piece p[5] = {tlen ? lit("Current topic: ") : lit("No topic has been set yet.\n"), none, none, none, none};
        int len = 0;
        append(a.ctext + at[4], look_text_cap(4), len, p, rec + kRrTopic, tlen, tlen != 0, lane, a.violations);
        if (lane == 0) clen[4] = len;
    }
    if (r == 0) {   // c:3979, 3985, 3986: the same for every room
        const int32_t* fat = a.ctext_off + kLookTexts * a.nr;
        int32_t* flen = a.clen + kLookTexts * a.nr;
#pragma unroll
        for (int i = 0; i < kLookFixed; i++) {
            const Piece p[5] = {i == 0 ? lit("~FTYou can see:\n") : i == 1 ? lit("~FTYou are all alone here.\n") : lit("\n"), none,
                                none, none, none};
            int len = 0;
            append(a.ctext + fat[i], i == 0 ? 16 : i == 1 ? 28 : 4, len, p, nullptr, 0, false, lane, a.violations);
            if (lane == 0) flen[i] = len;
        }
    }
}

template <int N>
__device__ __forceinline__ int row_lit(uint8_t* row, int pos, const char (&s)[N])
{
#pragma unroll
    for (int i = 0; i < N - 1; i++) row[pos + i] = (uint8_t)s[i];
    return pos + N - 1;
}

// Slot j's line (c:3980-3983) into row, by one lane; returns its length.
__device__ __forceinline__ int look_line(uint8_t* row, const uint4 rec, int nlen, const uint8_t* udesc, int j)
{
    const uint32_t state = rec.w >> 8 & 0xff;
    const uint4 d0 = reinterpret_cast<const uint4*>(udesc)[2 * j], d1 = reinterpret_cast<const uint4*>(udesc)[2 * j + 1];
    const int dl = (int)(d1.w >> 16 & 0xff), dlen = dl < kUserDescLen ? dl : kUserDescLen;
    int len = (state & kVis) ? row_lit(row, 0, "      ") : row_lit(row, 0, "     ~FR*~RS");
#pragma unroll
    for (int i = 0; i < kNameLen; i++) {                       // all twelve: what follows overwrites the padding
        const uint32_t v = i < 4 ? rec.x : i < 8 ? rec.y : rec.z;
        row[len + i] = (uint8_t)(v >> (8 * (i & 3)));
    }
    len += nlen;
    row[len++] = ' ';
#pragma unroll
    for (int i = 0; i < kUserDescLen; i++) {                   // likewise
        const uint32_t v = i < 4 ? d0.x : i < 8 ? d0.y : i < 12 ? d0.z : i < 16 ? d0.w : i < 20 ? d1.x : i < 24 ? d1.y
                           : i < 28 ? d1.z : d1.w;
        row[len + i] = (uint8_t)(v >> (8 * (i & 3)));
    }
    len += dlen;
    len = row_lit(row, len, "~RS  ");
    if (state & kAfk) len = row_lit(row, len, "~BR(AFK)");
    row[len++] = '\n';
    return len;
}

__device__ void roster_look(const LookArgs& a)
{
    __shared__ int s_cand[kBlock / 64], s_seen[kBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    if ((int)blockIdx.x >= a.nr + a.k) {    // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - a.nr - a.k) * kBlock + (int)threadIdx.x);
        return;
    }
    const bool looker = (int)blockIdx.x >= a.nr;                // block-uniform
    const int b = looker ? (int)blockIdx.x - a.nr : (int)blockIdx.x;
    if (!looker && wave == 0) look_room(a, b, lane);
    const int r = looker ? a.lroom[b] : b, rm = a.rms[r];
    const int u = looker ? a.slot[b] : -1;
    const int ulevel = looker ? a.speech[(size_t)u * kSpeechRec + kLevelByte] : 0;
    const int line0 = a.line_off[r], lines = a.line_off[r + 1] - line0;     // the room's lines
    const int m0 = looker ? a.m_off[b] : 0, mcap = looker ? a.m_off[b + 1] - m0 : 0;
    const int text0 = kLookTexts * a.nr + kLookFixed;           // the first line's text
    int cands = 0, seen = 0;                                    // the carries: candidates, and those this looker is shown
    for (int base = 0; base < a.capacity; base += kBlock) {     // block-uniform
        const int j = base + (int)threadIdx.x;
        bool cand = false, shown = false;
        uint4 rec{};
        int nlen = 0;
        if (j < a.capacity && a.room[j] == rm) {
            rec = reinterpret_cast<const uint4*>(a.speech)[j];
            nlen = (int)(rec.w & 0xff) < kNameLen ? (int)(rec.w & 0xff) : kNameLen;
            cand = nlen > 0;                                    // a slot without a name is no user
            shown = cand && j != u && ((rec.w >> 8 & kVis) || (int)(rec.w >> 16 & 0xff) <= ulevel);    // c:3977
        }
        const uint64_t bc = __ballot(cand), bs = __ballot(shown);
        if (lane == 0) {
            s_cand[wave] = __popcll((unsigned long long)bc);
            s_seen[wave] = __popcll((unsigned long long)bs);
        }
        __syncthreads();
        const uint64_t below = (1ull << lane) - 1;
        int crank = cands + __popcll((unsigned long long)(bc & below)), srank = seen + __popcll((unsigned long long)(bs & below));
#pragma unroll
        for (int x = 0; x < kBlock / 64; x++) {
            if (x < wave) {
                crank += s_cand[x];
                srank += s_seen[x];
            }
            cands += s_cand[x];
            seen += s_seen[x];
        }
        __syncthreads();                    // the next step overwrites the counts
        if (!looker && cand) {
            if (crank < lines) {
                const int t = text0 + line0 + crank;
                a.clen[t] = look_line(a.ctext + a.ctext_off[t], rec, nlen, a.udesc, j);
                a.line_slot[line0 + crank] = j;
            } else {
                atomicAdd(a.violations, 1);
            }
        }
        if (looker && shown) {
            if (srank < mcap && crank < lines) {
                a.members[m0 + srank] = j;
                a.mline[m0 + srank] = line0 + crank;
            } else {
                atomicAdd(a.violations, 1);
            }
        }
    }
    if (looker) {
        if (threadIdx.x == 0) a.nmem[b] = seen < mcap ? seen : mcap;
        return;
    }
    for (int i = cands + (int)threadIdx.x; i < lines; i += kBlock) a.clen[text0 + line0 + i] = -1;    // nobody's lines
    if (threadIdx.x == 0) a.nline[b] = cands < lines ? cands : lines;
}

static_assert(6 + 6 + kNameLen + 1 + kUserDescLen + 5 + 8 + 1 <= kLineRow, "roster_look: the longest member line fits its slot");
static_assert(6 + 6 + kNameLen + 1 + 32 <= kLineRow, "roster_look: the whole description row may be stored before it is cut");
static_assert(kRoomRow % 4 == 0 && kUserDescRow % 4 == 0 && kRrServ + kServNameLen <= kRoomRec, "roster_look: whole words");
static_assert(look_text_cap(0) >= 13 + kRoomNameLen + 2 && look_text_cap(1) >= kRoomDescLen &&
              look_text_cap(2) >= 14 + kMaxLinks * (5 + kRoomNameLen) + 5 + kServNameLen + 1 + 2 &&
              look_text_cap(3) >= 10 + 28 + 21 + 10 + 27 && look_text_cap(4) >= 15 + kTopicLen + 1,
              "roster_look: every room text fits its slot");
static_assert(kLookTextStride < kTextSize, "nuts_roster_speak_plan: a room text fits its LDS text");

// ------------------------------------------------------------------ the clone relay of a resident roster
//
// The clone branch of write_room_except (nuts333.c:1416-1426; clone_relay of oracle/talker_port.c): a clone standing in
// room rm does not receive a broadcast to rm, it sends "~FT[ <room name> ]:~RS " + str to its owner.  A roster keeps C
// clone records apart from its slots, in a device allocation of their own that never moves: the owners' slots (int32, -1:
// an empty record), the rooms (int32) and the clone_hear bytes (0 nothing, 1 swears, 2 all; nuts333.h:60-62), each array in a
// 256-byte slice; and the look rooms' names, 24 bytes per room: 20 of name padded with zeros, then its length.
//   relay    nuts_roster_relay after nuts_roster_plan on the same inputs, one block per broadcast.  Wave 0 scans the text
//            for swearing once (swears).  The block walks the C records a lane per record, 256 at a time: record c relays
//            broadcast b iff rm[b] >= 0, it has an owner, its room is rm[b], c is not csender[b] (the clone that is `user`
//            in write_room_except(rm, str, user), -1: none), hear is not 0, the owner's ignall flag is clear
//            (force_listen does not override it, c:1417), and hear is 2 or the text swears.  A wave's 64 answers are one
//            word of the relay bitmap (__ballot); lanes past C vote false, so the tail bits are zero.  If any record
//            relays, wave 0 composes the relay text into the call's relay-text buffer (compose), slot b at rtext_off[b],
//            len + kRelaySlack bytes wide; a broadcast without relays has length -1.  A relay text that would not fit the
//            reference's text2[ARR_SIZE] is a violation: the call fails.
//            Blocks past the broadcasts copy the clone records and the names just uploaded into the kept allocations.
//   plan     nuts_roster_speak_plan over the K relay texts, a block per text as after nuts_roster_look: stage_variants
//            gives each its two variants, and a text of length -1 is void, 0 bytes in 0 writes.  Composing and transducing
//            in one kernel spills scalar registers: store_variants alone takes every one the compiler has.
constexpr int kRelayNameRow = 24;                          // a look room's row of the relay's name table
constexpr int kRelaySlack = 5 + kRoomNameLen + 7;          // "~FT[ " + name + " ]:~RS ": a relay text's slot is this much wider
constexpr uint8_t kHearNothing = 0, kHearAll = 2;          // nuts333.h:60-62, CLONE_HEAR_SWEARS between them

struct RelayArgs {
    const uint8_t* slot;         // [capacity] the roster's flag bytes: the owners' ignall
    const uint8_t* records;      // the records this call reads, the upload or the kept ones, as take_clones lays them out
    const uint8_t* names;        // [look_rooms * kRelayNameRow] likewise
    Kept kept[2];                // the names, the clone records
    const uint8_t* text;         // the K texts, packed, as PlanArgs
    const int32_t* text_off;     // [k]
    const int32_t* text_len;     // [k]
    const int32_t* rm;           // [k] -1: every room
    const int32_t* csender;      // [k] the clone record that sends the broadcast; -1: none
    int k, capacity, clones, cwords, look_rooms;   // cwords: bitmap words per broadcast, ceil(clones / 64)
    const int32_t* rtext_off;    // [k] where relay text b's slot starts in rtext
    int* violations;             // relay texts past text2[ARR_SIZE] (zeroed by the host's upload)
    uint8_t* rtext;              // the relay texts
    int32_t* rlen;               // [k] their lengths; -1: nothing relays
    uint64_t* rbits;             // [k * cwords] the relay bitmap
};

__device__ void roster_relay(const RelayArgs& a)
{
    if ((int)blockIdx.x >= a.k) {           // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - a.k) * kBlock + (int)threadIdx.x);
        return;
    }
    __shared__ int s_swears, s_any;
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x & 63;
    const int rm = a.rm[b], len = a.text_len[b], except = a.csender[b];
    const uint8_t* text = a.text + a.text_off[b];
    if (threadIdx.x == 0) s_any = 0;
    if (threadIdx.x < 64) {                 // wave 0, whole: contains_swearing(str), once per broadcast
        const bool sw = rm >= 0 && len < kArrSize && swears(text, len, lane);
        if (lane == 0) s_swears = sw;
    }
    __syncthreads();
    const bool sw = s_swears != 0;
    const size_t slice = ((size_t)a.clones * sizeof(int32_t) + 255) & ~(size_t)255;      // a Carver slice of int32 [clones]
    const int32_t* owner = reinterpret_cast<const int32_t*>(a.records);                  // -1: an empty record
    const int32_t* croom = reinterpret_cast<const int32_t*>(a.records + slice);
    const uint8_t* hear = a.records + 2 * slice;
    bool any = false;
    for (int base = 0; base < a.cwords * 64; base += kBlock) {      // block-uniform: every wave votes in every round
        const int c = base + (int)threadIdx.x;
        bool in = false;
        if (c < a.clones && rm >= 0 && rm < a.look_rooms) {
            const int o = owner[c];
            const uint8_t h = hear[c];
            in = o >= 0 && o < a.capacity && croom[c] == rm && c != except && h != kHearNothing &&
                 !(a.slot[o] & kIgnall) && (h == kHearAll || sw);
        }
        const uint64_t word = __ballot(in);
        const int w = c >> 6;
        if (lane == 0 && w < a.cwords) a.rbits[(int64_t)b * a.cwords + w] = word;
        any |= word != 0;
    }
    if (any && lane == 0) s_any = 1;
    __syncthreads();
    if (!s_any) {                           // block-uniform: nothing is relayed
        if (threadIdx.x == 0) a.rlen[b] = -1;
        return;
    }
    if (threadIdx.x < 64) {                 // wave 0: sprintf(text2, "~FT[ %s ]:~RS %s", u->room->name, str), c:1424
        const uint8_t* row = a.names + (size_t)rm * kRelayNameRow;
        const int nlen = row[kRoomNameLen] < kRoomNameLen ? row[kRoomNameLen] : kRoomNameLen;
        const Piece none{nullptr, 0};
        const Piece p[5] = {lit("~FT[ "), Piece{row, nlen}, lit(" ]:~RS "), none, none};
        const int cap = len + kRelaySlack < kArrSize - 1 ? len + kRelaySlack : kArrSize - 1;   // text2[ARR_SIZE]
        const int n = compose(a.rtext + a.rtext_off[b], cap, p, text, len, false, lane, a.violations);
        if (lane == 0) a.rlen[b] = n;
    }
}

static_assert(5 + kRoomNameLen + 7 <= 64 && kRelaySlack == 32, "roster_relay: the prefix pieces fit a wave; the slot's slack");
static_assert(kRelayNameRow % 4 == 0 && kRoomNameLen < kRelayNameRow, "roster_relay: a name row is whole words and holds its length");
static_assert(kArrSize - 1 < kTextSize, "nuts_roster_speak_plan: a relay text fits its LDS text");

// ------------------------------------------------------------------ who() of a resident roster
//
// who(user, 0) (nuts333.c:4792-4856) sends a user the whole talker: a header with the date, a line per user it may see, a
// footer with the counts and a tail.  Like look() it is texts with two variants each and per looker a choice among them:
// a line depends on its user alone, the footer on the roster alone, and only the header (the looker's login flag) and
// which lines are sent (an invisible user above the looker's level is not) depend on the looker.  The listed users are
// the slots with a name and no login flag, in ascending slot order: line l is the l-th of them.
// A roster keeps one more table for it, 8 bytes per slot in a device allocation of its own that never moves: last_login
// (int32) and away (int32: the look room whose netlink a roomless user left through, -1: none).
//   who      nuts_roster_who, one launch whose blocks take roles by their index:
//            LINE BLOCKS, one per 256 slots.  A block first counts the listed slots before its own -- a ballot per wave and
//            step over the name lengths and login flags, the four waves' counts through LDS -- then ranks its own 256 the
//            same way: no atomics, the same result on every run.  The lane of a listed slot composes its line (who_line)
//            into the line's 236-byte slot of the composed-text buffer, whole, as look_line does and for its reason.
//            THE FIXED BLOCK counts the listed and the invisible slots of the whole roster, and its wave 0 composes the two
//            headers, the footer and the tail with compose().  The host sized the call for nl lines from its mirror:
//            a different count here is a violation, and the lines past the count are void.
//            COPY BLOCKS past those copy freshly uploaded tables into the kept allocations.
//            The kernel also writes every text's offset, so that the upload carries the lookers and the date alone.
//   shown    nuts_roster_who_shown, a block per looker and 256 lines, a lane per line: line l of slot line_slot[l] is
//            sent unless its user is invisible and above the looker's level.  A wave's 64 answers (__ballot) are two
//            words of the looker's bitmap; lanes past nl vote false, so the tail bits are zero.  It reads line_slot, which
//            blocks of nuts_roster_who wrote: hence a launch of its own.
//   plan     nuts_roster_speak_plan with no room lines (k = 0), a block per text, as after nuts_roster_look.
constexpr int kWhoRec = 8;                                 // a slot's row of the who table: last_login, away
constexpr int kWhoFixed = 4;                               // the login header, the header, the footer, the tail
constexpr int kWhoHeadRow = 108, kWhoFootRow = 80, kWhoTailRow = 8;
constexpr int kWhoFixedStride = 2 * kWhoHeadRow + kWhoFootRow + kWhoTailRow;
constexpr int who_fixed_at(int i) { return i == 0 ? 0 : i == 1 ? kWhoHeadRow : i == 2 ? 2 * kWhoHeadRow : 2 * kWhoHeadRow + kWhoFootRow; }
constexpr int kWhoDateLen = 79;                            // long_date's dstr[80]
// colour_com_count is at most 25 over "  " + name + " " + desc + "~RS": a count takes a byte of its own and a '~' before
// the first of a run, and a run is at most three ("~FBBM"), so 12 bytes of name hold 6, 30 of description 18, and ~RS is 1
constexpr int kWhoMaxCount = 25;
constexpr int kWhoPadMax = 40 + 3 * kWhoMaxCount;          // the widest first field
constexpr int kWhoLineMax = kWhoPadMax + 3 + 4 + 3 + 1 + kServNameLen + 3 + 9 + 6 + 9;   // 233: ... " : " -35791394 " mins." ~BR(AFK)\n
constexpr int kWhoRow = 236;                               // a line's slot

constexpr int64_t who_ctext_bytes(int64_t nl) { return kWhoFixedStride + nl * kWhoRow; }

struct WhoArgs {
    const int32_t* room;         // [capacity] the roster's table
    const uint8_t* slotf;        // [capacity] and its flag bytes: login
    const uint8_t* speech;       // the tables this call reads, the uploads or the kept ones, as LookArgs
    const uint8_t* rooms;
    const uint8_t* udesc;
    const uint8_t* who;          // [capacity * 8] last_login and away
    Kept kept[4];                // the speaker table, the room table, the descriptions, the who table
    const int32_t* slot;         // [k] the lookers
    const uint8_t* date;         // [date_len] long_date(1)
    int k, nl, capacity, look_rooms, words, date_len;   // words: bitmap words per looker, max(1, ceil(nl / 32))
    int32_t now;
    int* violations;             // texts past their slots, a listed slot without a room name, a count that is not nl
    int32_t* clen;               // [4 + nl] the texts' lengths; -1: a line past the count
    int32_t* ctext_off;          // [4 + nl] where each text's slot starts in ctext
    uint8_t* ctext;              // the texts
    int32_t* line_slot;          // [nl] the slot each line is of
    uint32_t* shown;             // [k * words] the lookers' bitmaps
};

// Where "XY" stands in colcom[] (nuts333.h:249-255), or -1.
__device__ __forceinline__ int who_code(uint8_t x, uint8_t y)
{
    if (x == 'F' || x == 'B') {
        const int c = y == 'K' ? 0 : y == 'R' ? 1 : y == 'G' ? 2 : y == 'Y' ? 3 : y == 'B' ? 4 : y == 'M' ? 5 : y == 'T' ? 6
                      : y == 'W' ? 7 : -1;
        return c < 0 ? -1 : (x == 'F' ? 5 : 13) + c;
    }
    return x == 'R' ? (y == 'S' ? 0 : y == 'V' ? 4 : -1) : x == 'O' ? (y == 'L' ? 1 : -1) : x == 'U' ? (y == 'L' ? 2 : -1)
           : x == 'L' ? (y == 'I' ? 3 : -1) : -1;
}

// colour_com_count (c:2563-2583) over s[0 .. len): after a match it advances one byte and goes on through the rest of
// the table there, so "~FBBM" counts FB, BB and BM.  Two bytes name at most one entry, so the table walk from entry
// `from` on matches iff that entry is not before `from`.
__device__ __forceinline__ int who_count(const uint8_t* s, int len)
{
    int i = 0, cnt = 0;
    while (i < len) {
        if (s[i++] != '~') continue;
        int from = 0;
        while (i + 1 < len) {
            const int c = who_code(s[i], s[i + 1]);
            if (c < from) break;
            cnt++;
            i++;
            from = c + 1;
        }
    }
    return cnt;
}

// Slot j's line (c:4838-4848) into row, by one lane; returns its length.  rname is the room's name or, with `at`, the
// service a roomless user is away over.
__device__ __forceinline__ int who_line(uint8_t* row, const uint4 rec, int nlen, const uint8_t* udesc, int j, const uint8_t* rname,
                                        int rlen, bool at, int32_t mins, int* violations)
{
    const uint32_t state = rec.w >> 8 & 0xff, level = rec.w >> 16 & 0xff;
    const uint4 d0 = reinterpret_cast<const uint4*>(udesc)[2 * j], d1 = reinterpret_cast<const uint4*>(udesc)[2 * j + 1];
    const int dl = (int)(d1.w >> 16 & 0xff), dlen = dl < kUserDescLen ? dl : kUserDescLen;
    int len = (state & kVis) ? row_lit(row, 0, "  ") : row_lit(row, 0, "* ");
#pragma unroll
    for (int i = 0; i < kNameLen; i++) {                       // all twelve: what follows overwrites the padding
        const uint32_t v = i < 4 ? rec.x : i < 8 ? rec.y : rec.z;
        row[len + i] = (uint8_t)(v >> (8 * (i & 3)));
    }
    len += nlen;
    row[len++] = ' ';
#pragma unroll
    for (int i = 0; i < kUserDescLen; i++) {                   // likewise
        const uint32_t v = i < 4 ? d0.x : i < 8 ? d0.y : i < 12 ? d0.z : i < 16 ? d0.w : i < 20 ? d1.x : i < 24 ? d1.y
                           : i < 28 ? d1.z : d1.w;
        row[len + i] = (uint8_t)(v >> (8 * (i & 3)));
    }
    len += dlen;
    len = row_lit(row, len, "~RS");
    int width = 40 + 3 * who_count(row, len);                  // %-*s
    if (width > kWhoPadMax) {                                  // never: kWhoMaxCount
        atomicAdd(violations, 1);
        width = kWhoPadMax;
    }
    while (len < width) row[len++] = ' ';
    len = row_lit(row, len, " : ");
    const uint32_t lname = level == 0 ? 'N' | 'E' << 8 | 'W' << 16 | (uint32_t)' ' << 24
                           : level == 1 ? 'U' | 'S' << 8 | 'E' << 16 | (uint32_t)'R' << 24
                           : level == 2 ? 'W' | 'I' << 8 | 'Z' << 16 | (uint32_t)' ' << 24
                           : level == 3 ? 'A' | 'R' << 8 | 'C' << 16 | (uint32_t)'H' << 24
                                        : 'G' | 'O' << 8 | 'D' << 16 | (uint32_t)' ' << 24;      // %-4s
#pragma unroll
    for (int i = 0; i < 4; i++) row[len + i] = (uint8_t)(lname >> (8 * i));
    len = row_lit(row, len + 4, " : ");
    const int field = len + 12;                                // %-12s
    if (at) row[len++] = '@';
    for (int i = 0; i < rlen; i++) row[len + i] = rname[i];
    len += rlen;
    while (len < field) row[len++] = ' ';
    len = row_lit(row, len, " : ");
    if (mins < 0) row[len++] = '-';                            // %d
    uint32_t v = mins < 0 ? (uint32_t)(-mins) : (uint32_t)mins;
    int digits = 1;
    for (uint32_t x = v; x >= 10; x /= 10) digits++;
    for (int i = digits - 1; i >= 0; i--, v /= 10) row[len + i] = (uint8_t)('0' + v % 10);
    len = row_lit(row, len + digits, " mins.");
    if (state & kAfk) len = row_lit(row, len, "~BR(AFK)");
    row[len++] = '\n';
    return len;
}

// %d of a count, a lane per digit, behind what a text already holds (append).
__device__ __forceinline__ void append_count(uint8_t* dst, int cap, int& at, int count, int lane, int* violations)
{
    if (at < 0) return;
    const uint32_t v = count > 0 ? (uint32_t)count : 0u;
    int digits = 1;
    for (uint32_t x = v; x >= 10; x /= 10) digits++;
    if (at + digits > cap) {
        if (lane == 0) atomicAdd(violations, 1);
        at = -1;
        return;
    }
    uint32_t x = v;
    for (int i = digits - 1; i > lane; i--) x /= 10;
    if (lane < digits) dst[at + lane] = (uint8_t)('0' + x % 10);
    at += digits;
}

// The two headers, the footer and the tail (c:4804-4806, 4849-4853), by one wave.
__device__ void who_fixed(const WhoArgs& a, int total, int invis, int lane)
{
    const Piece none{nullptr, 0};
    const int dlen = a.date_len < kWhoDateLen ? a.date_len : kWhoDateLen;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        uint8_t* t = a.ctext + who_fixed_at(i);
        int len = 0;
        const Piece p[5] = {i == 0 ? lit("\n*** Current users ") : lit("\n~BB*** Current users "), none, none, none, none};
        append(t, kWhoHeadRow, len, p, a.date, dlen, false, lane, a.violations);
        const Piece q[5] = {lit(" ***\n\n"), none, none, none, none};
        append(t, kWhoHeadRow, len, q, nullptr, 0, false, lane, a.violations);
        if (lane == 0) a.clen[i] = len;
    }
    {
        uint8_t* t = a.ctext + who_fixed_at(2);
        int len = 0;
        const Piece p0[5] = {lit("\nThere are "), none, none, none, none};
        append(t, kWhoFootRow, len, p0, nullptr, 0, false, lane, a.violations);
        append_count(t, kWhoFootRow, len, total - invis, lane, a.violations);
        const Piece p1[5] = {lit(" visible, "), none, none, none, none};
        append(t, kWhoFootRow, len, p1, nullptr, 0, false, lane, a.violations);
        append_count(t, kWhoFootRow, len, invis, lane, a.violations);
        const Piece p2[5] = {lit(" invisible, 0 remote users.\nTotal of "), none, none, none, none};
        append(t, kWhoFootRow, len, p2, nullptr, 0, false, lane, a.violations);
        append_count(t, kWhoFootRow, len, total, lane, a.violations);
        const Piece p3[5] = {lit(" users"), none, none, none, none};
        append(t, kWhoFootRow, len, p3, nullptr, 0, false, lane, a.violations);
        if (lane == 0) a.clen[2] = len;
    }
    {
        int len = 0;
        const Piece p[5] = {lit(".\n\n"), none, none, none, none};
        append(a.ctext + who_fixed_at(3), kWhoTailRow, len, p, nullptr, 0, false, lane, a.violations);
        if (lane == 0) a.clen[3] = len;
    }
    if (lane < kWhoFixed) a.ctext_off[lane] = lane == 0 ? who_fixed_at(0) : lane == 1 ? who_fixed_at(1) : lane == 2 ? who_fixed_at(2)
                                                                                                        : who_fixed_at(3);
}

__device__ void roster_who(const WhoArgs& a)
{
    __shared__ int s_cnt[kBlock / 64], s_inv[kBlock / 64], s_own[kBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int line_blocks = (a.capacity + kBlock - 1) / kBlock;
    if ((int)blockIdx.x > line_blocks) {    // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - line_blocks - 1) * kBlock + (int)threadIdx.x);
        return;
    }
    const bool fixed = (int)blockIdx.x == line_blocks;          // block-uniform
    const int first = fixed ? a.capacity : (int)blockIdx.x * kBlock;     // the slots before this block's own
    const uint32_t* state = reinterpret_cast<const uint32_t*>(a.speech);  // word 3 of a slot: name length, flags, level
    int before = 0, invis = 0;                                  // of this wave's share of them: listed, and invisible
    for (int base = 0; base < first; base += kBlock) {          // block-uniform
        const int j = base + (int)threadIdx.x;
        bool listed = false, inv = false;
        if (j < first) {
            const uint32_t w = state[4 * (size_t)j + 3];
            listed = (w & 0xff) != 0 && !(a.slotf[j] & kLogin); // a slot without a name is no user; c:4817
            inv = listed && !(w >> 8 & kVis);
        }
        before += __popcll((unsigned long long)__ballot(listed));
        invis += __popcll((unsigned long long)__ballot(inv));
    }
    if (lane == 0) {
        s_cnt[wave] = before;
        s_inv[wave] = invis;
    }
    __syncthreads();
    int prior = 0, ninv = 0;
#pragma unroll
    for (int x = 0; x < kBlock / 64; x++) {
        prior += s_cnt[x];
        ninv += s_inv[x];
    }
    if (fixed) {
        if (wave == 0) {
            who_fixed(a, prior, ninv, lane);
            if (lane == 0 && prior != a.nl) atomicAdd(a.violations, 1);
        }
        for (int l = prior + (int)threadIdx.x; l < a.nl; l += kBlock) {   // the lines past the count are nobody's
            a.clen[kWhoFixed + l] = -1;
            a.ctext_off[kWhoFixed + l] = kWhoFixedStride + l * kWhoRow;
            a.line_slot[l] = -1;
        }
        return;
    }
    const int j = first + (int)threadIdx.x;
    bool listed = false;
    uint4 rec{};
    if (j < a.capacity) {
        rec = reinterpret_cast<const uint4*>(a.speech)[j];
        listed = (rec.w & 0xff) != 0 && !(a.slotf[j] & kLogin);
    }
    const uint64_t bl = __ballot(listed);
    if (lane == 0) s_own[wave] = __popcll((unsigned long long)bl);
    __syncthreads();
    int l = prior + __popcll((unsigned long long)(bl & ((1ull << lane) - 1)));
#pragma unroll
    for (int x = 0; x < kBlock / 64; x++)
        if (x < wave) l += s_own[x];
    if (!listed || l >= a.nl) return;       // past nl: the fixed block reports the count
    const int t = kWhoFixed + l;
    const int at = kWhoFixedStride + l * kWhoRow;
    a.ctext_off[t] = at;
    a.line_slot[l] = j;
    const int rm = a.room[j];
    const int32_t* wrec = reinterpret_cast<const int32_t*>(a.who) + 2 * (size_t)j;
    const int away = wrec[1];
    const uint8_t* rname = nullptr;
    int rlen = 0;
    const bool roomless = rm < 0;
    if (!roomless && rm < a.look_rooms) {
        rname = a.rooms + (size_t)rm * kRoomRec;
        rlen = rname[kRrNameLen] < kRoomNameLen ? rname[kRrNameLen] : kRoomNameLen;
    } else if (roomless && away >= 0 && away < a.look_rooms) {  // c:4841
        const uint8_t* r = a.rooms + (size_t)away * kRoomRec;
        rname = r + kRrServ;
        rlen = r[kRrServLen] < kServNameLen ? r[kRrServLen] : kServNameLen;
    } else {                                // the host has checked them: never past the table
        atomicAdd(a.violations, 1);
        a.clen[t] = -1;
        return;
    }
    const int nlen = (int)(rec.w & 0xff) < kNameLen ? (int)(rec.w & 0xff) : kNameLen;
    const int32_t mins = (a.now - wrec[0]) / 60;                // both in [0, 2^31): no overflow; C's truncation
    a.clen[t] = who_line(a.ctext + at, rec, nlen, a.udesc, j, rname, rlen, roomless, mins, a.violations);
}

__device__ void roster_who_shown(const WhoArgs& a)
{
    const int tiles = a.nl > kBlock ? (a.nl + kBlock - 1) / kBlock : 1;
    const int b = (int)blockIdx.x / tiles, tile = (int)blockIdx.x - b * tiles;
    const int l = tile * kBlock + (int)threadIdx.x;
    const uint32_t* state = reinterpret_cast<const uint32_t*>(a.speech);
    const int ulevel = (int)(state[4 * (size_t)a.slot[b] + 3] >> 16 & 0xff);
    bool in = false;
    if (l < a.nl) {
        const int j = a.line_slot[l];
        if (j >= 0 && j < a.capacity) {
            const uint32_t w = state[4 * (size_t)j + 3];
            in = (w >> 8 & kVis) || (int)(w >> 16 & 0xff) <= ulevel;     // c:4832-4835
        }
    }
    const uint64_t word = __ballot(in);
    const int w = 2 * (l >> 6);
    if (((int)threadIdx.x & 63) == 0) {
        uint32_t* bits = a.shown + (int64_t)b * a.words;
        if (w < a.words) bits[w] = (uint32_t)word;
        if (w + 1 < a.words) bits[w + 1] = (uint32_t)(word >> 32);
    }
}

static_assert(2 + kNameLen + 1 + kUserDescLen + 3 <= kWhoPadMax && kWhoLineMax <= kWhoRow && kWhoRow % 4 == 0,
              "roster_who: the first field is at most kWhoPadMax wide, and the longest line fits its slot");
static_assert(2 + kNameLen + 1 + 32 <= kWhoRow, "roster_who: the whole description row may be stored before it is cut");
static_assert(22 + kWhoDateLen + 6 <= kWhoHeadRow && 11 + 5 + 10 + 5 + 37 + 5 + 6 <= kWhoFootRow && 3 <= kWhoTailRow,
              "roster_who: every fixed text fits its slot");
static_assert(kWhoRow < kTextSize && kWhoRec % 4 == 0, "nuts_roster_speak_plan: a line fits its LDS text; whole words");

// ------------------------------------------------------------------ rooms() of a resident roster
//
// rooms(user, show_topics) (nuts333.c:5661-5700; .rmst and .rmsn) sends a user the room list: a header of its kind, a
// line per room and a tail.  Nothing but the colour depends on the looker, so a call has at most 3 + 2 R texts for the R
// look rooms -- the two headers, the tail, room r's .rmst line at 3 + r and its .rmsn line at 3 + R + r -- each with two
// variants.  A room whose record has no name is not listed; a kind no looker of the call asks for is not composed.
// A line holds the number of users standing in its room (c:5679-5680): the slots with a name, no login flag and that
// room, who_many's population.  That is a histogram over the whole roster.
// The record's flag byte (kRrNet) holds for it, beside bit 0 (a link that is UP) and bit 1 (allow == IN): bit 2 inlink,
// bit 3 a link that is unconnected, bit 4 a link that is connected and not yet up.  A room has a netlink when bit 0, 3
// or 4 is set; look() and who() read bit 0 alone.
//   count    nuts_roster_rooms_count, one launch whose blocks take roles by their index:
//            COUNT BLOCKS, one per 256 slots, a lane per slot.  The block zeroes a histogram of look_rooms bins in LDS,
//            the lane of a counted slot adds one to its room's bin (ds_add), and after a barrier the block adds its
//            non-zero bins to the roster's counters in global memory, which the host zeroed on the stream before the
//            launch.  Integer adds: the same result on every run, in whatever order the blocks arrive.
//            COPY BLOCKS past those copy freshly uploaded tables into the kept allocations.
//   lines    nuts_roster_rooms_lines, a lane per room, 256 per block: the lane of a listed room composes its line of each
//            kind asked for into the room's rows of the composed-text buffer, whole, as who_line does.  It reads the
//            counters that blocks of nuts_roster_rooms_count wrote: hence a launch of its own.  Wave 0 of one block more
//            composes the headers and the tail with compose().  The kernel writes every text's offset and length and
//            copies the counters next to the other results.
//   plan     nuts_roster_speak_plan with no room lines (k = 0), a block per text, as after nuts_roster_who.
constexpr int kRoomsFixed = 3;                             // the .rmst header, the .rmsn header, the tail
constexpr int kRoomsHeadTRow = 80, kRoomsHeadNRow = 96, kRoomsTailRow = 4;
constexpr int kRoomsFixedStride = kRoomsHeadTRow + kRoomsHeadNRow + kRoomsTailRow;
constexpr int rooms_fixed_at(int i) { return i == 0 ? 0 : i == 1 ? kRoomsHeadTRow : kRoomsHeadTRow + kRoomsHeadNRow; }
constexpr int kRoomsCountMax = 5, kRoomsMesgMax = 10;      // %3d widens: 65536 slots, a mesg_cnt of 2^31 - 1
// "%-20s : %9s~RS    %3d    %3d  %s\n" and "%-20s : %9s~RS    %3d    %3d     %s   %s~RS  %s\n" at their longest
constexpr int kRoomsLineFront = kRoomNameLen + 3 + 9 + 3 + 4 + kRoomsCountMax + 4 + kRoomsMesgMax;
constexpr int kRmstLineMax = kRoomsLineFront + 2 + kTopicLen + 1;                          // 121
constexpr int kRmsnLineMax = kRoomsLineFront + 5 + 3 + 3 + 7 + 3 + 2 + kServNameLen + 1;   // 162
constexpr int kRmstRow = 124, kRmsnRow = 164;              // the lines' slots
constexpr int kRoomsTopics = 1, kRoomsLinks = 2;           // the kinds of a call: .rmst, .rmsn
constexpr int kNetUp = 1, kNetInlink = 4, kNetDown = 8, kNetVerifying = 16;

constexpr int64_t rooms_ctext_bytes(int64_t nr) { return kRoomsFixedStride + nr * (kRmstRow + kRmsnRow); }

struct RoomsArgs {
    const int32_t* room;         // [capacity] the roster's table
    const uint8_t* slotf;        // [capacity] and its flag bytes: login
    const uint8_t* speech;       // the tables this call reads, the uploads or the kept ones, as LookArgs
    const uint8_t* rooms;
    Kept kept[2];                // the speaker table, the room table
    const int32_t* slot;         // [k] the lookers: nothing of a text depends on them
    int k, capacity, look_rooms, kinds;     // kinds: kRoomsTopics | kRoomsLinks, what the lookers ask for
    int* violations;             // texts past their slots
    int32_t* counters;           // [look_rooms] the users per room, zeroed by the host before nuts_roster_rooms_count
    int32_t* counts;             // [look_rooms] and their copy among the results
    int32_t* clen;               // [3 + 2 look_rooms] the texts' lengths; -1: a kind not asked for, a room without a name
    int32_t* ctext_off;          // [3 + 2 look_rooms] where each text's slot starts in ctext
    uint8_t* ctext;              // the texts
};

__device__ void roster_rooms_count(const RoomsArgs& a)
{
    __shared__ int s_hist[kMaxLookRooms];
    const int count_blocks = (a.capacity + kBlock - 1) / kBlock;
    if ((int)blockIdx.x >= count_blocks) {  // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - count_blocks) * kBlock + (int)threadIdx.x);
        return;
    }
    const int bins = a.look_rooms < kMaxLookRooms ? a.look_rooms : kMaxLookRooms;
    for (int i = (int)threadIdx.x; i < bins; i += kBlock) s_hist[i] = 0;
    __syncthreads();
    const int j = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (j < a.capacity) {
        const int rm = a.room[j];
        const uint32_t w = reinterpret_cast<const uint32_t*>(a.speech)[4 * (size_t)j + 3];    // word 3: the name's length first
        // c:5680 counts every non-clone user of the room; a slot without a name is no user, and one at login stage has
        // no room yet in the reference (connect_user sets both at once, c:1745-1758)
        if (rm >= 0 && rm < bins && (w & 0xff) != 0 && !(a.slotf[j] & kLogin)) atomicAdd(&s_hist[rm], 1);
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < bins; i += kBlock) {
        const int n = s_hist[i];
        if (n) atomicAdd(&a.counters[i], n);
    }
}

// "%3d" of v >= 0 into row at pos, by one lane; returns the position behind it.
__device__ __forceinline__ int row_count(uint8_t* row, int pos, int32_t count)
{
    uint32_t v = count > 0 ? (uint32_t)count : 0u;
    int digits = 1;
    for (uint32_t x = v; x >= 10; x /= 10) digits++;
    for (int i = digits; i < 3; i++) row[pos++] = ' ';
    for (int i = digits - 1; i >= 0; i--, v /= 10) row[pos + i] = (uint8_t)('0' + v % 10);
    return pos + digits;
}

// What both kinds of line begin with (c:5682, 5695): "%-20s : %9s~RS    %3d    %3d" of name, access, count and mesg_cnt.
__device__ __forceinline__ int rooms_line_front(uint8_t* row, const uint8_t* rec, int nlen, int32_t count)
{
    for (int i = 0; i < nlen; i++) row[i] = rec[i];
    for (int i = nlen; i < kRoomNameLen; i++) row[i] = ' ';                // %-20s
    int len = row_lit(row, kRoomNameLen, " :  ");                          // " : ", and %9s of eight bytes pads one
    const int access = rec[kRrAccess];
    row[len++] = (access & 2) ? '*' : ' ';                                 // FIXED: access[0] = '*'
    len = (access & 1) ? row_lit(row, len, "~FRPRIV") : row_lit(row, len, " ~FGPUB");
    len = row_lit(row, len, "~RS    ");
    len = row_count(row, len, count);
    len = row_lit(row, len, "    ");
    return row_count(row, len, *reinterpret_cast<const int32_t*>(rec + kRrMesgCnt));
}

__device__ void roster_rooms_lines(const RoomsArgs& a)
{
    const int nr = a.look_rooms;
    const int line_blocks = (nr + kBlock - 1) / kBlock;
    if ((int)blockIdx.x == line_blocks) {   // the fixed texts (c:5672, 5673, 5699), by one wave
        if (threadIdx.x >= 64) return;
        const int lane = (int)threadIdx.x;
        const Piece none{nullptr, 0};
        const Piece top[5] = {lit("\n~BB*** Rooms data ***\n\n"), none, none, none, none};
        const Piece names[5] = {lit("~FTRoom name            : Access  Users  Mesgs  "), none, none, none, none};
#pragma unroll
        for (int i = 0; i < 2; i++) {
            int len = -1;
            if (a.kinds & (i == 0 ? kRoomsTopics : kRoomsLinks)) {
                uint8_t* t = a.ctext + rooms_fixed_at(i);
                const int cap = i == 0 ? kRoomsHeadTRow : kRoomsHeadNRow;
                const Piece rest[5] = {i == 0 ? lit("Topic\n\n") : lit("Inlink  LStat  Service\n\n"), none, none, none, none};
                len = 0;
                append(t, cap, len, top, nullptr, 0, false, lane, a.violations);
                append(t, cap, len, names, nullptr, 0, false, lane, a.violations);
                append(t, cap, len, rest, nullptr, 0, false, lane, a.violations);
            }
            if (lane == 0) a.clen[i] = len;
        }
        int len = 0;
        const Piece tail[5] = {lit("\n"), none, none, none, none};
        append(a.ctext + rooms_fixed_at(2), kRoomsTailRow, len, tail, nullptr, 0, false, lane, a.violations);
        if (lane == 0) a.clen[2] = len;
        if (lane < kRoomsFixed) a.ctext_off[lane] = lane == 0 ? rooms_fixed_at(0) : lane == 1 ? rooms_fixed_at(1) : rooms_fixed_at(2);
        return;
    }
    const int r = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (r >= nr) return;
    const int tt = kRoomsFixed + r, tn = kRoomsFixed + nr + r;
    const int at_t = kRoomsFixedStride + r * kRmstRow, at_n = kRoomsFixedStride + nr * kRmstRow + r * kRmsnRow;
    const int32_t count = a.counters[r];
    a.counts[r] = count;
    a.ctext_off[tt] = at_t;
    a.ctext_off[tn] = at_n;
    const uint8_t* rec = a.rooms + (size_t)r * kRoomRec;
    const int nlen = rec[kRrNameLen] < kRoomNameLen ? rec[kRrNameLen] : kRoomNameLen;
    int len_t = -1, len_n = -1;
    if (nlen && (a.kinds & kRoomsTopics)) {                     // a room without a name is no room of the list
        uint8_t* row = a.ctext + at_t;
        const int tlen = rec[kRrTopicLen] < kTopicLen ? rec[kRrTopicLen] : kTopicLen;
        int len = rooms_line_front(row, rec, nlen, count);
        len = row_lit(row, len, "  ");
        for (int i = 0; i < tlen; i++) row[len + i] = rec[kRrTopic + i];
        len += tlen;
        row[len++] = '\n';
        len_t = len;
    }
    if (nlen && (a.kinds & kRoomsLinks)) {
        uint8_t* row = a.ctext + at_n;
        const int net = rec[kRrNet];
        const bool linked = (net & (kNetUp | kNetDown | kNetVerifying)) != 0;
        const int slen = !linked ? 0 : rec[kRrServLen] < kServNameLen ? rec[kRrServLen] : kServNameLen;   // c:5694
        int len = rooms_line_front(row, rec, nlen, count);
        len = (net & kNetInlink) ? row_lit(row, len, "     YES   ") : row_lit(row, len, "      NO   ");    // noyes1[]
        if (!linked) len = (net & kNetInlink) ? row_lit(row, len, "~FRDOWN") : row_lit(row, len, "   -");   // c:5685-5688
        else if (net & kNetDown) len = row_lit(row, len, "~FRDOWN");                                       // c:5690-5692
        else if (net & kNetUp) len = row_lit(row, len, "  ~FGUP");
        else len = row_lit(row, len, " ~FYVER");
        len = row_lit(row, len, "~RS  ");
        for (int i = 0; i < slen; i++) row[len + i] = rec[kRrServ + i];
        len += slen;
        row[len++] = '\n';
        len_n = len;
    }
    a.clen[tt] = len_t;
    a.clen[tn] = len_n;
}

static_assert(sizeof("\n~BB*** Rooms data ***\n\n~FTRoom name            : Access  Users  Mesgs  Topic\n\n") - 1 <= kRoomsHeadTRow &&
              sizeof("\n~BB*** Rooms data ***\n\n~FTRoom name            : Access  Users  Mesgs  Inlink  LStat  Service\n\n") - 1 <= kRoomsHeadNRow &&
              1 <= kRoomsTailRow, "roster_rooms: every fixed text fits its slot");
static_assert(kRmstLineMax == 121 && kRmsnLineMax == 162 && kRmstLineMax <= kRmstRow && kRmsnLineMax <= kRmsnRow &&
              kRmstRow % 4 == 0 && kRmsnRow % 4 == 0 && kRoomsFixedStride % 4 == 0, "roster_rooms: the longest lines fit their slots");
static_assert(kRmsnRow < kTextSize && kMaxLookRooms * sizeof(int) <= 4096, "roster_rooms: a line fits speak_plan's LDS text; a 4 KB histogram");

// ------------------------------------------------------------------ go() of a resident roster
//
// go() and move_user() (nuts333.c:4305-4459) with get_room (c:2383-2391), has_room_access (c:2412-2421) and what
// reset_access (c:2087-2106) decides.  The device decides and composes; it writes no kept table.  The host binding applies
// the moves to its mirrors afterwards, and the look a move ends with is a nuts_roster_look call of its own.
// A fourth per-slot table kept like the speaker state holds what only this call reads of a user, 88 bytes per slot:
//   go row        0 in_phrase[40] | 40 its length | 41 out_phrase[40] | 81 its length | 82 zeros | 84 int32 invite_room (-1: none)
// An event has four texts, each in a slot of fixed width (their longest forms are pinned by a host test): the enter line the
// target room gets, the leave line the old room gets, the reset line the old room gets when it returns to public, and the
// notice the mover alone gets when it did not move.  With K events, text k is event k's enter line, K + k its leave line,
// 2K + k its reset line and 3K + k its reply.
//   go       nuts_roster_go, ONE BLOCK PER EVENT, in the shape of nuts_roster_tell.  word[1] is found as there, by every wave
//            for itself.  The netlink test (c:4315-4316) is a prefix compare of the word with the room's service, a byte per
//            lane.  get_room: lane l of wave w tests room 256 i + 64 w + l in step i -- a name, at least as long as the
//            word, that begins with it --, a ballot per step, the first hit is the wave's lowest, and the four waves'
//            minima meet in LDS.  The decision chain follows, block-uniform.  For a mover that leaves a room whose access is
//            exactly PRIVATE the block counts who stays behind: a lane per slot (that room, a name, no login flag, not the
//            mover) and a lane per clone record standing there, ballots summed per wave and the four sums through LDS.
//            No atomics: the same answer on every run.  Wave 0 composes the texts with compose() and lane 0 stores the
//            lengths, the outcome, the target, the old room, whether the old room returns to public, and rm / sender /
//            com of the three room texts as nuts_roster_speak_plan takes them: the enter line to the target without a
//            sender, the leave and the reset line to the old room with the mover as sender.  Every event is decided
//            against the tables as they were before the call.
//            Blocks past the events copy freshly uploaded tables into the kept allocations.
//   order    nuts_roster_go_order, ONE WAVE, makes that exact.  It walks the events in call order with two bitmaps in LDS,
//            a bit per look room and a bit per slot, "touched by an earlier event of this call that moved".  An event
//            whose slot, current room or resolved target room is touched is deferred: its outcome becomes kGoDeferred, its
//            four texts void, and it touches nothing.  An event that moved and was not deferred touches its slot, the room
//            it left and the room it entered.  The events that remain are pairwise disjoint in slots and rooms, so each
//            one decided and planned against the snapshot is what running them one after another gives.  The walk is
//            order_events, which the order kernels of the other three event calls share with a rule of their own: the
//            wave loads 64 events at a time, a lane each, and steps through them by shuffles; lane 0 sets the bits.
//   plan     nuts_roster_speak_plan with 3K room lines and K replies, over the table as it was before the call.
constexpr int kGoRec = 88, kPhraseLen = 40;                // a slot's row of the go table; nuts333.h:26 PHRASE_LEN
constexpr int kGoIn = 0, kGoInLen = 40, kGoOut = 41, kGoOutLen = 81, kGoInvite = 84;
constexpr int kComGo = 10;                                 // enum np_com: NP_GO
constexpr int kGoWalked = 0, kGoTeleported = 1, kGoUnseen = 2, kGoWhere = 3, kGoNetlink = 4, kGoNoRoom = 5, kGoAlready = 6,
              kGoNotAdjoined = 7, kGoPrivate = 8, kGoDeferred = 9;      // an event moved iff its outcome is at most kGoUnseen
constexpr uint8_t kAccessPrivate = 1, kAccessFixed = 2;    // nuts333.h: PRIVATE, FIXED
constexpr int kGoTexts = 4;                                // enter, leave, reset, reply
constexpr int kGoMaxSlots = 65536;                         // the most slots of a roster: a bit each in nuts_roster_go_order
// the longest texts: "~FT~OL" + name + " appears in an explosion of blue magic!\n"; name + " " + out_phrase + " to the " +
// room name + ".\n"; "Room access returned to ~FGPUBLIC.\n"; "The " + room name + " is not adjoined to here.\n" (and the
// private notice, as long)
constexpr int kGoEnterMax = 6 + kNameLen + 40, kGoLeaveMax = kNameLen + 1 + kPhraseLen + 8 + kRoomNameLen + 2, kGoResetMax = 35,
              kGoReplyMax = 4 + kRoomNameLen + 26;
constexpr int kGoEnterRow = 60, kGoLeaveRow = 84, kGoResetRow = 36, kGoReplyRow = 52;      // their slots
constexpr int kGoRow = kGoEnterRow + kGoLeaveRow + kGoResetRow + kGoReplyRow;               // an event's bytes of composed text
constexpr int go_row(int kind) { return kind == 0 ? kGoEnterRow : kind == 1 ? kGoLeaveRow : kind == 2 ? kGoResetRow : kGoReplyRow; }
// Where text kind * k + b of a call of k events has its slot: the enter lines, then the leave lines, the reset lines, the replies.
constexpr int64_t go_text_at(int kind, int64_t b, int64_t k)
{
    return (kind == 0 ? 0 : kind == 1 ? kGoEnterRow : kind == 2 ? kGoEnterRow + kGoLeaveRow : kGoEnterRow + kGoLeaveRow + kGoResetRow) * k
           + go_row(kind) * b;
}

// What the compose kernels of the four event calls -- go, access, clone, set -- are all passed, the head of their arguments:
// the host writes the steps that read only these once (check_events .. copy_event_results).  Each call's own members follow
// in one order -- the results, the commands and settings, the tables -- under which nuts_roster_access and nuts_roster_clone,
// which use every scalar register there is, still keep all their arguments in them.
struct EventArgs {
    const int32_t* room;         // [capacity] the roster's table
    const uint8_t* slotf;        // [capacity] and its flag bytes
    const uint8_t* text;         // the K inpstr, packed
    const int32_t* text_off;     // [k]
    const int32_t* text_len;     // [k]
    const int32_t* slot;         // [k] the event's user: the mover, the actor
    const uint8_t* words;        // [k] word_count
    const int32_t* ctext_off;    // [texts * k] where each text's slot starts in ctext
    int k, capacity;
    int* violations;             // composed texts past their slot (zeroed by the host's upload)
    uint8_t* ctext;              // the composed texts
    int32_t* clen;               // [texts * k] their lengths; -1: no such text
    int8_t* outcome;             // [k]
};

struct GoArgs : EventArgs {      // slotf: login
    int32_t* target;             // [k] the room the word resolved to; -1: none, or get_room was not reached
    int32_t* old_room;           // [k] the mover's room before the call
    uint8_t* returned;           // [k] 1: the old room returns to public
    int32_t* rm;                 // [3k] the room texts' rooms, as SpeakPlanArgs.rm
    int32_t* sender;             // [3k] and their senders (-1: none)
    int32_t* com_num;            // [3k]
    int look_rooms, clones, gatecrash_level, min_private_users;
    const uint8_t* speech;       // the tables this call reads, the uploads or the kept ones: the speaker state (name, vis, level),
    const uint8_t* records;      // the clone records as take_clones lays them out (nullptr: the roster has none),
    const uint8_t* rooms;        // the room records,
    const uint8_t* go;           // [capacity * 88] and the go table
    Kept kept[4];                // in that order
};

// Does s[0 .. slen) begin with w[0 .. wlen), wlen <= kWordLen?  strncmp(s, w, strlen(w)) == 0 over a NUL-ended s, by a whole
// wave, a byte per lane; wave-uniform.
__device__ __forceinline__ bool begins_with(const uint8_t* s, int slen, const uint8_t* w, int wlen, int lane)
{
    const bool differs = lane < wlen && (lane >= slen || s[lane] != w[lane]);
    return __ballot(differs) == 0;
}

// get_room (c:2388-2389) for one wave of a block: its lowest room among 64 wave + 256 i + lane that has a name beginning
// with the word, or kNoMatch.  Wave-uniform; the block's waves meet in LDS.
__device__ __forceinline__ int wave_get_room(const uint8_t* rooms, int look_rooms, const uint8_t* word, int wlen, int wave, int lane)
{
    if (wlen > kRoomNameLen) return kNoMatch;
    for (int base = 64 * wave; base < look_rooms; base += kBlock) {
        const int r = base + lane;
        bool hit = false;
        if (r < look_rooms) {
            const uint8_t* rec = rooms + (size_t)r * kRoomRec;
            const int rl = rec[kRrNameLen] < kRoomNameLen ? rec[kRrNameLen] : kRoomNameLen;
            hit = rl > 0 && wlen <= rl;                     // a room without a name is no room
            for (int i = 0; i < wlen && hit; i++) hit = rec[i] == word[i];
        }
        const uint64_t b = __ballot(hit);
        if (b) return base + __ffsll((unsigned long long)b) - 1;
    }
    return kNoMatch;
}

__device__ void roster_go(const GoArgs& a)
{
    if ((int)blockIdx.x >= a.k) {           // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - a.k) * kBlock + (int)threadIdx.x);
        return;
    }
    __shared__ int s_room[kBlock / 64], s_pop[kBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int k = (int)blockIdx.x;
    const int slot = a.slot[k], wc = a.words[k], len = a.text_len[k];
    const uint8_t* in = a.text + a.text_off[k];
    const uint8_t* sp = a.speech + (size_t)slot * kSpeechRec;
    const uint8_t* gp = a.go + (size_t)slot * kGoRec;
    const uint8_t state = sp[kNameLen + 1];
    const int nlen = sp[kNameLen] < kNameLen ? sp[kNameLen] : kNameLen;
    const int level = sp[kLevelByte];
    const int here = a.room[slot];          // a look room: the host checked it
    const uint8_t* hrec = a.rooms + (size_t)here * kRoomRec;

    // word[1] as np_wordfind finds the line's second word (c:417-432): inpstr has lost the first
    uint32_t wordb = 0;
#pragma unroll
    for (int x = 0; x < kReadSlice; x++) {
        const int at = kReadSlice * lane + x;
        wordb |= (uint32_t)(at < len && (int8_t)in[at] > 32) << x;
    }
    const int w0 = first_from(wordb, 0, lane, len);
    const int w0_end = first_from(~wordb & 0xffffu, w0, lane, len);
    const int wlen = w0_end - w0 < kWordLen ? w0_end - w0 : kWordLen;
    const uint8_t* word = in + w0;

    // c:4312-4316: too few words, then the netlink branch, which the caller answers; block-uniform
    int outcome = -1;
    if (wc < 2) outcome = kGoWhere;
    else if (hrec[kRrNet] & (kNetUp | kNetDown | kNetVerifying)) {
        const int slen = hrec[kRrServLen] < kServNameLen ? hrec[kRrServLen] : kServNameLen;
        if (begins_with(hrec + kRrServ, slen, word, wlen, lane)) outcome = kGoNetlink;
    }

    // get_room (c:2388-2389): this wave's lowest room that has a name beginning with the word, among 64 w + 256 i + lane
    int best = outcome < 0 ? wave_get_room(a.rooms, a.look_rooms, word, wlen, wave, lane) : kNoMatch;
    if (lane == 0) s_room[wave] = best;
    __syncthreads();
    for (int w = 0; w < kBlock / 64; w++) best = s_room[w] < best ? s_room[w] : best;

    // c:4384-4404 and move_user's first test (c:4417), block-uniform
    int target = -1;
    bool linked = false;
    if (outcome < 0) {
        if (best == kNoMatch) outcome = kGoNoRoom;
        else {
            target = best;
            const int nlinks = hrec[kRrLinks] < kMaxLinks ? hrec[kRrLinks] : kMaxLinks;
            const int32_t* link = reinterpret_cast<const int32_t*>(hrec + kRrLink);
            for (int i = 0; i < nlinks; i++) linked |= link[i] == target;
            const uint8_t access = a.rooms[(size_t)target * kRoomRec + kRrAccess];
            const int32_t invite = *reinterpret_cast<const int32_t*>(gp + kGoInvite);
            if (target == here) outcome = kGoAlready;
            else if (!linked && level < kWiz) outcome = kGoNotAdjoined;
            else if ((access & kAccessPrivate) && level < a.gatecrash_level && invite != target &&
                     !((access & kAccessFixed) && level >= kWiz)) outcome = kGoPrivate;
            else outcome = !(state & kVis) ? kGoUnseen : linked ? kGoWalked : kGoTeleported;
        }
    }
    const bool moved = outcome <= kGoUnseen;

    // reset_access(old_room) after the move (c:2093-2096): who still stands in a room that is exactly PRIVATE
    int stay = 0;
    if (moved && hrec[kRrAccess] == kAccessPrivate) {       // block-uniform
        for (int base = 0; base < a.capacity; base += kBlock) {
            const int j = base + (int)threadIdx.x;
            const bool in_room = j < a.capacity && j != slot && a.room[j] == here && !(a.slotf[j] & kLogin) &&
                                 a.speech[(size_t)j * kSpeechRec + kNameLen] != 0;
            stay += __popcll(__ballot(in_room));
        }
        if (a.records) {                                    // clones count (c:2095 walks the whole user list)
            const size_t slice = ((size_t)a.clones * sizeof(int32_t) + 255) & ~(size_t)255;
            const int32_t* owner = reinterpret_cast<const int32_t*>(a.records);
            const int32_t* croom = reinterpret_cast<const int32_t*>(a.records + slice);
            for (int base = 0; base < a.clones; base += kBlock) {
                const int c = base + (int)threadIdx.x;
                const bool in_room = c < a.clones && owner[c] >= 0 && croom[c] == here;
                stay += __popcll(__ballot(in_room));
            }
        }
    }
    if (lane == 0) s_pop[wave] = stay;
    __syncthreads();
    if (wave != 0) return;
    stay = 0;
    for (int w = 0; w < kBlock / 64; w++) stay += s_pop[w];
    const bool returns = moved && hrec[kRrAccess] == kAccessPrivate && stay < a.min_private_users;

    const int n = a.k;
    uint8_t* enter = a.ctext + a.ctext_off[k];
    uint8_t* leave = a.ctext + a.ctext_off[n + k];
    const Piece none{nullptr, 0};
    const Piece name{sp, nlen};
    const uint8_t* trec = a.rooms + (size_t)(target < 0 ? here : target) * kRoomRec;
    const Piece tname{trec, trec[kRrNameLen] < kRoomNameLen ? trec[kRrNameLen] : kRoomNameLen};
    int enter_len = -1, leave_len = -1, reset_len = -1, reply_len = -1;
    if (outcome == kGoUnseen) {             // c:4423-4427, invisenter and invisleave
        const Piece e[5] = {lit("A presence enters the room...\n"), none, none, none, none};
        const Piece l[5] = {lit("A presence leaves the room.\n"), none, none, none, none};
        enter_len = compose(enter, kGoEnterRow, e, nullptr, 0, false, lane, a.violations);
        leave_len = compose(leave, kGoLeaveRow, l, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kGoTeleported) {  // c:4428-4434
        const Piece head[5] = {lit("~FT~OL"), name, none, none, none};
        const Piece e[5] = {lit(" appears in an explosion of blue magic!\n"), none, none, none, none};
        const Piece l[5] = {lit(" chants a spell and vanishes into a magical blue vortex!\n"), none, none, none, none};
        enter_len = leave_len = 0;
        append(enter, kGoEnterRow, enter_len, head, nullptr, 0, false, lane, a.violations);
        append(enter, kGoEnterRow, enter_len, e, nullptr, 0, false, lane, a.violations);
        append(leave, kGoLeaveRow, leave_len, head, nullptr, 0, false, lane, a.violations);
        append(leave, kGoLeaveRow, leave_len, l, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kGoWalked) {      // c:4450-4453
        const int ilen = gp[kGoInLen] < kPhraseLen ? gp[kGoInLen] : kPhraseLen;
        const int olen = gp[kGoOutLen] < kPhraseLen ? gp[kGoOutLen] : kPhraseLen;
        const Piece head[5] = {name, lit(" "), none, none, none};
        const Piece e[5] = {lit(".\n"), none, none, none, none};
        const Piece l[5] = {lit(" to the "), tname, lit(".\n"), none, none};
        enter_len = leave_len = 0;
        append(enter, kGoEnterRow, enter_len, head, gp + kGoIn, ilen, false, lane, a.violations);
        append(enter, kGoEnterRow, enter_len, e, nullptr, 0, false, lane, a.violations);
        append(leave, kGoLeaveRow, leave_len, head, gp + kGoOut, olen, false, lane, a.violations);
        append(leave, kGoLeaveRow, leave_len, l, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kGoAlready) {     // c:4388
        const Piece p[5] = {lit("You are already in the "), tname, lit("!\n"), none, none};
        reply_len = compose(a.ctext + a.ctext_off[3 * n + k], kGoReplyRow, p, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kGoNotAdjoined) { // c:4400
        const Piece p[5] = {lit("The "), tname, lit(" is not adjoined to here.\n"), none, none};
        reply_len = compose(a.ctext + a.ctext_off[3 * n + k], kGoReplyRow, p, nullptr, 0, false, lane, a.violations);
    } else if (outcome != kGoNetlink) {     // c:4313, nosuchroom, c:4418
        const Piece p[5] = {outcome == kGoWhere ? lit("Go where?\n") : outcome == kGoNoRoom ? lit("There is no such room.\n")
                            : lit("That room is currently private, you cannot enter.\n"), none, none, none, none};
        reply_len = compose(a.ctext + a.ctext_off[3 * n + k], kGoReplyRow, p, nullptr, 0, false, lane, a.violations);
    }
    if (moved && (enter_len < 0 || leave_len < 0)) enter_len = leave_len = -1;     // a violation: the call fails
    if (returns && enter_len >= 0) {        // c:2097
        const Piece p[5] = {lit("Room access returned to ~FGPUBLIC.\n"), none, none, none, none};
        reset_len = compose(a.ctext + a.ctext_off[2 * n + k], kGoResetRow, p, nullptr, 0, false, lane, a.violations);
    }
    if (lane == 0) {
        a.clen[k] = enter_len;
        a.clen[n + k] = leave_len;
        a.clen[2 * n + k] = reset_len;
        a.clen[3 * n + k] = reply_len;
        a.outcome[k] = (int8_t)outcome;
        a.target[k] = target;
        a.old_room[k] = here;
        a.returned[k] = reset_len >= 0;
        a.rm[k] = target;                   // write_room(rm, ...): nobody is excepted
        a.sender[k] = -1;
        a.rm[n + k] = a.rm[2 * n + k] = here;               // the snapshot still has the mover there
        a.sender[n + k] = a.sender[2 * n + k] = slot;
        a.com_num[k] = a.com_num[n + k] = a.com_num[2 * n + k] = kComGo;
    }
}

static_assert(kGoEnterMax == 58 && kGoLeaveMax == 83 && kGoReplyMax == 50 && kGoEnterMax <= kGoEnterRow && kGoLeaveMax <= kGoLeaveRow &&
              kGoResetMax <= kGoResetRow && kGoReplyMax <= kGoReplyRow, "roster_go: the longest texts fit their slots");
static_assert(sizeof(" appears in an explosion of blue magic!\n") - 1 == 40 && sizeof("Room access returned to ~FGPUBLIC.\n") - 1 == kGoResetMax &&
              6 + kNameLen + sizeof(" chants a spell and vanishes into a magical blue vortex!\n") - 1 <= kGoLeaveMax &&
              sizeof("That room is currently private, you cannot enter.\n") - 1 <= kGoReplyMax &&
              sizeof("You are already in the !\n") - 1 + kRoomNameLen <= kGoReplyMax &&
              sizeof("The  is not adjoined to here.\n") - 1 + kRoomNameLen == kGoReplyMax, "roster_go: the texts are as long as counted");
static_assert(kGoRec % 4 == 0 && kGoInvite % 4 == 0 && kGoOutLen < kGoInvite && kGoRow % 4 == 0 && kGoLeaveRow < kTextSize,
              "roster_go: a go row is whole words, and a text fits speak_plan's LDS text");
static_assert(kWordLen < 64 && sizeof(" chants a spell and vanishes into a magical blue vortex!\n") - 1 <= 64,
              "roster_go: a word is a byte per lane, and the pieces of a compose() fit a wave");

// The order stage of an event call (go, access, clone, set): ONE WAVE walks the call's events in call order and defers those
// that an earlier event of the call, itself effective and not deferred, touched -- so every event that remains was decided
// against a snapshot that nothing before it in the call changed.  What is touched is kept as bits in LDS, zeroed first.  The
// events are taken 64 at a time, a lane each; each event's keys and outcome are then handed to the whole wave in turn, tested
// against the bitmaps, and marked by lane 0 between two barriers that every lane reaches.  A deferred event gets the rule's
// deferred outcome, its texts become void, and the rule clears what else the compose kernel wrote for it.
// A Rule is the kernel's argument struct: outcome[k], clen[kTexts * k], k; kKeys ints an event, which load() reads for
// event b (any in-range value for a lane without an event, which nobody looks at); hit(key, maps), whether an earlier event
// touched one of them; touch(key, outcome, maps), which marks what an effective event touches; kDeferred; kMapWords of
// bitmaps, which the rule divides among its keys; also_void(b).
constexpr int kOrderRoomWords = kMaxLookRooms / 32, kOrderSlotWords = kGoMaxSlots / 32;
__device__ __forceinline__ bool bit_of(const uint32_t* map, int i) { return (map[i >> 5] >> (i & 31)) & 1u; }
__device__ __forceinline__ void set_bit(uint32_t* map, int i) { map[i >> 5] |= 1u << (i & 31); }

template <typename Rule>
__device__ void order_events(const Rule& a)
{
    static_assert(Rule::kMapWords % 4 == 0, "order_events: the bitmaps are zeroed four words a store");
    __shared__ uint4 s_zeroed[Rule::kMapWords / 4];
    uint32_t* s_maps = reinterpret_cast<uint32_t*>(s_zeroed);
    const int lane = (int)threadIdx.x;      // one wave
    for (int i = lane; i < Rule::kMapWords / 4; i += 64) s_zeroed[i] = make_uint4(0, 0, 0, 0);   // most of a small call's time
    __syncthreads();
    for (int base = 0; base < a.k; base += 64) {
        const int k = base + lane;
        const bool live = k < a.k;
        int mine[Rule::kKeys], key[Rule::kKeys];
        a.load(k, live, mine);
        const int out = live ? a.outcome[k] : Rule::kDeferred;
        const int count = a.k - base < 64 ? a.k - base : 64;
        bool defer = false;
        for (int i = 0; i < count; i++) {   // in call order; every lane follows, lane 0 sets the bits
#pragma unroll
            for (int j = 0; j < Rule::kKeys; j++) key[j] = __shfl(mine[j], i);
            const int oc = __shfl(out, i);
            const bool hit = Rule::hit(key, s_maps);
            if (lane == i) defer = hit;
            __syncthreads();
            if (lane == 0 && !hit) Rule::touch(key, oc, s_maps);
            __syncthreads();
        }
        if (live && defer) {
            a.outcome[k] = (int8_t)Rule::kDeferred;
#pragma unroll
            for (int kind = 0; kind < Rule::kTexts; kind++) a.clen[kind * a.k + k] = -1;
            a.also_void(k);
        }
    }
}

// nuts_roster_go_order's rule.  Keys: the mover's slot, the room left, the room the word resolved to (-1: none).  Its bitmaps,
// as nuts_roster_access_order's and nuts_roster_clone_order's: a bit per look room, then a bit per slot.
struct GoOrderArgs {
    const int32_t* slot;         // [k] the movers
    const int32_t* old_room;     // [k] what nuts_roster_go wrote
    const int32_t* target;       // [k]
    int k;
    int8_t* outcome;             // [k] becomes kGoDeferred for a deferred event
    int32_t* clen;               // [4k] whose four texts become void
    uint8_t* returned;           // [k] and whose room does not return

    static constexpr int kKeys = 3, kTexts = kGoTexts, kDeferred = kGoDeferred, kMapWords = kOrderRoomWords + kOrderSlotWords;
    __device__ void load(int b, bool live, int (&key)[kKeys]) const
    {
        key[0] = live ? slot[b] : 0, key[1] = live ? old_room[b] : 0, key[2] = live ? target[b] : -1;
    }
    static __device__ bool hit(const int (&key)[kKeys], const uint32_t* maps)
    {
        return bit_of(maps + kOrderRoomWords, key[0]) || bit_of(maps, key[1]) || (key[2] >= 0 && bit_of(maps, key[2]));
    }
    static __device__ void touch(const int (&key)[kKeys], int outcome, uint32_t* maps)
    {
        if (outcome > kGoUnseen) return;    // a move touches its slot, the room left and the room entered
        set_bit(maps + kOrderRoomWords, key[0]);
        set_bit(maps, key[1]);
        set_bit(maps, key[2]);
    }
    __device__ void also_void(int b) const { returned[b] = 0; }
};

static_assert(kMaxLookRooms % 32 == 0 && kGoMaxSlots % 32 == 0, "roster_go_order: the bitmaps are whole words");

// ------------------------------------------------------------------ a room's door, of a resident roster
//
// set_room_access(), letmein() and invite() (nuts333.c:4543-4693): .public, .private, .letmein and .invite, commands 16 to
// 19.  As with go(), the device decides and composes and writes no kept table; the host binding sets the access and the
// invitations in its mirrors afterwards.  It reads the five tables nuts_roster_go reads.
// An event has four texts in slots of fixed width: the line the actor's room gets without the actor ("here"), the line
// another room gets ("there"), the actor's own line ("reply") and the line an invited user gets ("notice").  With K events,
// text k is event k's here line, K + k its there line, 2K + k its reply and 3K + k its notice: the 2K room lines first, as
// nuts_roster_speak_plan wants them.
//   access   nuts_roster_access, ONE BLOCK PER EVENT, in the shape of nuts_roster_go.  word[1] is found as there.  By the
//            command the block runs get_user over the capitalised word (wave_get_user; first, while little else is
//            live: the search needs the most registers), get_room (wave_get_room), and for a .private that reaches the
//            count (c:4583-4584) the head-count of the room: a lane per slot (that room, a name, no login flag; the actor
//            counts) and a lane per clone record standing there, ballots summed per wave.  The waves' results meet in
//            LDS.  Wave 0 decides in the reference's order and composes: the actor's line from kAccReply, two fixed parts
//            per outcome around a name or the count, the other three texts with compose() / append().  Lane 0 stores the lengths, the outcome, the room and the slot the word resolved to, and rm / sender / com of
//            the two room lines: the here line to the actor's room with the actor as sender, the there line to the other
//            room without one.  No atomics: the same bytes on every run.
//            Blocks past the events copy freshly uploaded tables into the kept allocations.
//   order    nuts_roster_access_order, ONE WAVE: order_events by its own rule.  Set private and set public touch the room
//            whose access changes, invited touches the invited slot.  An event whose actor's room, resolved room or found
//            slot an earlier event of the call that was not itself deferred touched is deferred: its outcome becomes
//            kAccDeferred and its four texts void.
//   plan     nuts_roster_speak_plan with 2K room lines and 2K single-recipient texts.
constexpr int kComPublic = 16, kComPrivate = 17, kComLetmein = 18, kComInvite = 19;        // enum np_com
constexpr int kAccSetPrivate = 0, kAccSetPublic = 1, kAccInvited = 2, kAccAsked = 3, kAccLowLevel = 4, kAccNoRoom = 5, kAccFixed = 6,
              kAccAlreadyPublic = 7, kAccAlreadyPrivate = 8, kAccTooFew = 9, kAccLetWhere = 10, kAccLetNoRoom = 11, kAccLetAlready = 12,
              kAccLetNotAdjoined = 13, kAccLetPublic = 14, kAccInviteWho = 15, kAccInvitePublic = 16, kAccInviteNobody = 17,
              kAccInviteSelf = 18, kAccInviteHere = 19, kAccInviteAlready = 20, kAccDeferred = 21;
constexpr int kAccTexts = 4;                               // here, there, reply, notice
// the longest texts: name + " shouts asking to be let into the " + room name + ".\n"; name + " shouts asking to be let in.\n";
// "You need at least " + ten digits + " users/clones in a room before it can be made private.\n"; name + " has invited you
// into the " + room name + ".\n"
constexpr int kAccHereMax = kNameLen + 34 + kRoomNameLen + 2, kAccThereMax = kNameLen + 29, kAccReplyMax = 18 + 10 + 55,
              kAccNoticeMax = kNameLen + 26 + kRoomNameLen + 2;
constexpr int kAccHereRow = 72, kAccThereRow = 44, kAccReplyRow = 84, kAccNoticeRow = 60;  // their slots
constexpr int kAccRow = kAccHereRow + kAccThereRow + kAccReplyRow + kAccNoticeRow;         // an event's bytes of composed text
constexpr int acc_row(int kind) { return kind == 0 ? kAccHereRow : kind == 1 ? kAccThereRow : kind == 2 ? kAccReplyRow : kAccNoticeRow; }
// Where text kind * k + b of a call of k events has its slot: the here lines, then the there lines, the replies, the notices.
constexpr int64_t acc_text_at(int kind, int64_t b, int64_t k)
{
    return (kind == 0 ? 0 : kind == 1 ? kAccHereRow : kind == 2 ? kAccHereRow + kAccThereRow : kAccHereRow + kAccThereRow + kAccReplyRow) * k
           + acc_row(kind) * b;
}

// The actor's own line by outcome (c:4555-4687, nuts333.h:145-146): two fixed parts, around the room, a name or the count.
struct AccessReply {
    char pre[63];
    uint8_t npre;
    char post[63];
    uint8_t npost;
};
template <int N, int M>
constexpr AccessReply access_reply(const char (&pre)[N], const char (&post)[M])
{
    static_assert(N <= 64 && M <= 64, "access_reply: a part fits its field, and a compose()");
    AccessReply r{};
    for (int i = 0; i < N - 1; i++) r.pre[i] = pre[i];
    for (int i = 0; i < M - 1; i++) r.post[i] = post[i];
    r.npre = N - 1;
    r.npost = M - 1;
    return r;
}
__device__ const AccessReply kAccReply[] = {
    access_reply("Room set to ~FRPRIVATE.\n", ""),                                        // kAccSetPrivate
    access_reply("Room set to ~FGPUBLIC.\n", ""),                                         // kAccSetPublic
    access_reply("You invite ", " in.\n"),                                                // kAccInvited
    access_reply("You shout asking to be let into the ", ".\n"),                          // kAccAsked
    access_reply("You are not a high enough level to use the room option.\n", ""),        // kAccLowLevel
    access_reply("There is no such room.\n", ""),                                         // kAccNoRoom
    access_reply("", "'s access is fixed.\n"),                                            // kAccFixed
    access_reply("", " is already public.\n"),                                            // kAccAlreadyPublic
    access_reply("", " is already private.\n"),                                           // kAccAlreadyPrivate
    access_reply("You need at least ", " users/clones in a room before it can be made private.\n"),      // kAccTooFew
    access_reply("Let you into where?\n", ""),                                            // kAccLetWhere
    access_reply("There is no such room.\n", ""),                                         // kAccLetNoRoom
    access_reply("You are already in the ", "!\n"),                                       // kAccLetAlready
    access_reply("The ", " is not adjoined to here.\n"),                                  // kAccLetNotAdjoined
    access_reply("The ", " is currently public.\n"),                                      // kAccLetPublic
    access_reply("Invite who?\n", ""),                                                    // kAccInviteWho
    access_reply("This room is currently public.\n", ""),                                 // kAccInvitePublic
    access_reply("There is no one of that name logged on.\n", ""),                        // kAccInviteNobody
    access_reply("Inviting yourself to somewhere is the third sign of madness.\n", ""),   // kAccInviteSelf
    access_reply("", " is already here!\n"),                                              // kAccInviteHere
    access_reply("", " has already been invited into here.\n"),                           // kAccInviteAlready
};
static_assert(sizeof(kAccReply) / sizeof(kAccReply[0]) == kAccDeferred, "kAccReply: a line for every outcome nuts_roster_access decides");

struct AccessArgs : EventArgs {  // slotf: login
    int32_t* target_room;        // [k] the room the event is about; -1: none, or the step was not reached
    int32_t* target_slot;        // [k] the slot get_user found; -1: none, or it was not asked
    int32_t* rm;                 // [2k] the room lines' rooms, as SpeakPlanArgs.rm
    int32_t* sender;             // [2k] and their senders (-1: none)
    int32_t* com_num;            // [2k]
    const uint8_t* com;          // [k] NP_PUBLIC, NP_PRIVATE, NP_LETMEIN or NP_INVITE
    int look_rooms, clones, gatecrash_level, min_private_users, ignore_mp_level;
    const uint8_t* speech;       // the tables this call reads, the uploads or the kept ones: the speaker state (name, vis, level),
    const uint8_t* records;      // the clone records as take_clones lays them out (nullptr: the roster has none),
    const uint8_t* rooms;        // the room records,
    const uint8_t* go;           // [capacity * 88] and the go table: invite_room
    Kept kept[4];                // the speaker state, the clone records, the go table, the room records
};

__device__ void roster_access(const AccessArgs& a)
{
    if ((int)blockIdx.x >= a.k) {           // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - a.k) * kBlock + (int)threadIdx.x);
        return;
    }
    __shared__ int s_room[kBlock / 64], s_pop[kBlock / 64], s_exact[kBlock / 64], s_sub[kBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int k = (int)blockIdx.x;
    const int slot = a.slot[k], com = a.com[k], wc = a.words[k], len = a.text_len[k];
    const uint8_t* in = a.text + a.text_off[k];
    const int level = a.speech[(size_t)slot * kSpeechRec + kLevelByte];
    const int here = a.room[slot];          // a look room: the host checked it
    const bool setting = com == kComPublic || com == kComPrivate;

    // word[1] as np_wordfind finds the line's second word (c:417-432): inpstr has lost the first
    uint32_t wordb = 0;
#pragma unroll
    for (int x = 0; x < kReadSlice; x++) {
        const int at = kReadSlice * lane + x;
        wordb |= (uint32_t)(at < len && (int8_t)in[at] > 32) << x;
    }
    const int w0 = first_from(wordb, 0, lane, len);
    const int w0_end = first_from(~wordb & 0xffffu, w0, lane, len);
    const int wlen = w0_end - w0 < kWordLen ? w0_end - w0 : kWordLen;
    const uint8_t* word = in + w0;

    // what comes before get_room and get_user (c:4552-4557, 4622-4624, 4662-4669); block-uniform
    int outcome = -1, rm = -1;
    bool want_room = false;
    if (setting) {
        if (wc < 2) rm = here;
        else if (level < a.gatecrash_level) outcome = kAccLowLevel;
        else want_room = true;
    } else if (com == kComLetmein) {
        if (wc < 2) outcome = kAccLetWhere;
        else want_room = true;
    } else if (wc < 2) outcome = kAccInviteWho;
    else if (!(a.rooms[(size_t)here * kRoomRec + kRrAccess] & kAccessPrivate)) outcome = kAccInvitePublic;

    // get_user over the capitalised word (c:4670), before anything else is kept: the search is what needs registers most
    int best_exact = kNoMatch, best_sub = kNoMatch;
    if (com == kComInvite && outcome < 0) {
        const UserMatch m = wave_get_user(a.speech, a.slotf, a.capacity, pack_word(word, wlen), wlen, wave, lane);
        best_exact = m.exact;
        best_sub = m.sub;
    }

    int best = want_room ? wave_get_room(a.rooms, a.look_rooms, word, wlen, wave, lane) : kNoMatch;
    if (lane == 0) s_room[wave] = best;
    __syncthreads();
    for (int w = 0; w < kBlock / 64; w++) best = s_room[w] < best ? s_room[w] : best;
    if (want_room) {
        if (best == kNoMatch) outcome = setting ? kAccNoRoom : kAccLetNoRoom;
        else rm = best;
    }

    // the head-count of a room that could become private (c:4583-4584)
    int cnt = 0;
    if (com == kComPrivate && outcome < 0 && a.rooms[(size_t)rm * kRoomRec + kRrAccess] == 0) {       // block-uniform
        for (int base = 0; base < a.capacity; base += kBlock) {
            const int j = base + (int)threadIdx.x;
            const bool in_room = j < a.capacity && a.room[j] == rm && !(a.slotf[j] & kLogin) &&
                                 a.speech[(size_t)j * kSpeechRec + kNameLen] != 0;
            cnt += __popcll(__ballot(in_room));
        }
        if (a.records) {                                    // clones count (c:4584 walks the whole user list)
            const size_t slice = ((size_t)a.clones * sizeof(int32_t) + 255) & ~(size_t)255;
            const int32_t* owner = reinterpret_cast<const int32_t*>(a.records);
            const int32_t* croom = reinterpret_cast<const int32_t*>(a.records + slice);
            for (int base = 0; base < a.clones; base += kBlock) {
                const int c = base + (int)threadIdx.x;
                const bool in_room = c < a.clones && owner[c] >= 0 && croom[c] == rm;
                cnt += __popcll(__ballot(in_room));
            }
        }
    }
    if (lane == 0) {
        s_pop[wave] = cnt;
        s_exact[wave] = best_exact;
        s_sub[wave] = best_sub;
    }
    __syncthreads();
    if (wave != 0) return;
    cnt = 0;
    for (int w = 0; w < kBlock / 64; w++) {
        cnt += s_pop[w];
        best_exact = s_exact[w] < best_exact ? s_exact[w] : best_exact;
        best_sub = s_sub[w] < best_sub ? s_sub[w] : best_sub;
    }

    // the three functions' decisions, in their order
    const uint8_t* sp = a.speech + (size_t)slot * kSpeechRec;
    const uint8_t* hrec = a.rooms + (size_t)here * kRoomRec;
    const uint8_t* rrec = a.rooms + (size_t)(rm < 0 ? here : rm) * kRoomRec;
    const uint8_t access = rrec[kRrAccess];
    int target = -1;
    if (outcome < 0 && setting) {           // c:4563-4605
        if (access > kAccessPrivate) outcome = kAccFixed;
        else if (com == kComPublic) outcome = access == 0 ? kAccAlreadyPublic : kAccSetPublic;
        else if (access == kAccessPrivate) outcome = kAccAlreadyPrivate;
        else outcome = cnt < a.min_private_users && level < a.ignore_mp_level ? kAccTooFew : kAccSetPrivate;
    } else if (outcome < 0 && com == kComLetmein) {         // c:4628-4645
        bool linked = false;
        const int nlinks = hrec[kRrLinks] < kMaxLinks ? hrec[kRrLinks] : kMaxLinks;
        const int32_t* link = reinterpret_cast<const int32_t*>(hrec + kRrLink);
        for (int i = 0; i < nlinks; i++) linked |= link[i] == rm;
        outcome = rm == here ? kAccLetAlready : !linked ? kAccLetNotAdjoined : !(access & kAccessPrivate) ? kAccLetPublic : kAccAsked;
    } else if (outcome < 0) {               // c:4670-4687
        target = best_exact != kNoMatch ? best_exact : best_sub != kNoMatch ? best_sub : -1;
        if (target < 0) outcome = kAccInviteNobody;
        else if (target == slot) outcome = kAccInviteSelf;
        else if (a.room[target] == here) outcome = kAccInviteHere;
        else if (*reinterpret_cast<const int32_t*>(a.go + (size_t)target * kGoRec + kGoInvite) == here) outcome = kAccInviteAlready;
        else outcome = kAccInvited;
    }

    const int n = a.k;
    uint8_t* here_t = a.ctext + a.ctext_off[k];
    uint8_t* there_t = a.ctext + a.ctext_off[n + k];
    uint8_t* reply_t = a.ctext + a.ctext_off[2 * n + k];
    uint8_t* notice_t = a.ctext + a.ctext_off[3 * n + k];
    const Piece none{nullptr, 0};
    const Piece name{sp, sp[kNameLen] < kNameLen ? sp[kNameLen] : kNameLen};
    const Piece shown = (sp[kNameLen + 1] & kVis) ? name : lit("A presence");
    const Piece rname{rrec, rrec[kRrNameLen] < kRoomNameLen ? rrec[kRrNameLen] : kRoomNameLen};
    const uint8_t* tp = a.speech + (size_t)(target < 0 ? slot : target) * kSpeechRec;
    const Piece tname{tp, tp[kNameLen] < kNameLen ? tp[kNameLen] : kNameLen};
    const bool mine = rm == here;
    int here_len = -1, there_len = -1, reply_len = 0, notice_len = -1;
    // the actor's line: the outcome's two fixed parts around the room ("This room" or "That room" where set_room_access
    // refuses), the room's name, the found user's name or the count
    {
        const AccessReply& fixed = kAccReply[outcome];
        const uint8_t* mid = nullptr;
        int nmid = 0;
        if (outcome >= kAccFixed && outcome <= kAccAlreadyPrivate) {
            mid = reinterpret_cast<const uint8_t*>(mine ? "This room" : "That room");
            nmid = 9;
        } else if (outcome == kAccAsked || (outcome >= kAccLetAlready && outcome <= kAccLetPublic)) {
            mid = rname.p;
            nmid = rname.n;
        } else if (outcome == kAccInvited || outcome >= kAccInviteHere) {
            mid = tname.p;
            nmid = tname.n;
        }
        const Piece pre[5] = {Piece{reinterpret_cast<const uint8_t*>(fixed.pre), fixed.npre}, none, none, none, none};
        const Piece m[5] = {Piece{mid, nmid}, none, none, none, none};
        const Piece post[5] = {Piece{reinterpret_cast<const uint8_t*>(fixed.post), fixed.npost}, none, none, none, none};
        append(reply_t, kAccReplyRow, reply_len, pre, nullptr, 0, false, lane, a.violations);
        if (outcome == kAccTooFew) append_count(reply_t, kAccReplyRow, reply_len, a.min_private_users, lane, a.violations);   // c:4586
        else append(reply_t, kAccReplyRow, reply_len, m, nullptr, 0, false, lane, a.violations);
        append(reply_t, kAccReplyRow, reply_len, post, nullptr, 0, false, lane, a.violations);
    }
    if (outcome == kAccSetPrivate || outcome == kAccSetPublic) {       // c:4591-4595, 4600-4604
        const Piece to = outcome == kAccSetPrivate ? lit("~FRPRIVATE.\n") : lit("~FGPUBLIC.\n");
        if (mine) {
            const Piece h[5] = {shown, lit(" has set the room to "), to, none, none};
            here_len = compose(here_t, kAccHereRow, h, nullptr, 0, false, lane, a.violations);
        } else {
            const Piece t[5] = {lit("This room has been set to "), to, none, none, none};
            there_len = compose(there_t, kAccThereRow, t, nullptr, 0, false, lane, a.violations);
        }
        if (here_len < 0 && there_len < 0) reply_len = -1;
    } else if (outcome == kAccAsked) {      // c:4647-4650: user->name, even of an invisible asker
        const Piece h0[5] = {name, lit(" shouts asking to be let into the "), none, none, none};
        const Piece h1[5] = {rname, lit(".\n"), none, none, none};
        const Piece t[5] = {name, lit(" shouts asking to be let in.\n"), none, none, none};
        here_len = 0;
        append(here_t, kAccHereRow, here_len, h0, nullptr, 0, false, lane, a.violations);
        append(here_t, kAccHereRow, here_len, h1, nullptr, 0, false, lane, a.violations);
        there_len = compose(there_t, kAccThereRow, t, nullptr, 0, false, lane, a.violations);
    } else if (outcome == kAccInvited) {    // c:4689-4691
        const Piece v[5] = {shown, lit(" has invited you into the "), rname, lit(".\n"), none};
        notice_len = compose(notice_t, kAccNoticeRow, v, nullptr, 0, false, lane, a.violations);
    }
    if (reply_len < 0 || (outcome == kAccAsked && (here_len < 0 || there_len < 0)) || (outcome == kAccInvited && notice_len < 0))
        here_len = there_len = reply_len = notice_len = -1;            // a violation: the call fails
    if (lane == 0) {
        a.clen[k] = here_len;
        a.clen[n + k] = there_len;
        a.clen[2 * n + k] = reply_len;
        a.clen[3 * n + k] = notice_len;
        a.outcome[k] = (int8_t)outcome;
        a.target_room[k] = rm;
        a.target_slot[k] = target;
        a.rm[k] = here;                     // write_room_except(user->room, text, user)
        a.sender[k] = slot;
        a.rm[n + k] = rm < 0 ? here : rm;   // write_room(rm, text): nobody is excepted
        a.sender[n + k] = -1;
        a.com_num[k] = a.com_num[n + k] = com;
    }
}

static_assert(kAccHereMax == 68 && kAccThereMax == 41 && kAccReplyMax == 83 && kAccNoticeMax == 60 && kAccHereMax <= kAccHereRow &&
              kAccThereMax <= kAccThereRow && kAccReplyMax <= kAccReplyRow && kAccNoticeMax <= kAccNoticeRow,
              "roster_access: the longest texts fit their slots");
static_assert(sizeof(" shouts asking to be let into the ") - 1 == 34 && sizeof(" shouts asking to be let in.\n") - 1 == 29 &&
              sizeof("You need at least ") - 1 == 18 && sizeof(" users/clones in a room before it can be made private.\n") - 1 == 55 &&
              sizeof(" has invited you into the ") - 1 == 26 && kNameLen + sizeof(" has set the room to ~FRPRIVATE.\n") - 1 <= kAccHereMax &&
              sizeof("This room has been set to ~FRPRIVATE.\n") - 1 <= kAccThereMax &&
              sizeof("You shout asking to be let into the .\n") - 1 + kRoomNameLen <= kAccReplyMax &&
              sizeof("Inviting yourself to somewhere is the third sign of madness.\n") - 1 <= kAccReplyMax &&
              kNameLen + sizeof(" has already been invited into here.\n") - 1 <= kAccReplyMax, "roster_access: the texts are as long as counted");
static_assert(kAccRow % 4 == 0 && kAccHereRow % 4 == 0 && kAccThereRow % 4 == 0 && kAccReplyRow % 4 == 0 && kAccReplyRow < kTextSize,
              "roster_access: the rows are whole words, and a text fits speak_plan's LDS text");
static_assert(sizeof("You shout asking to be let into the .\n") - 1 + kRoomNameLen <= 64 && kAccNoticeMax <= 64 &&
              sizeof("Inviting yourself to somewhere is the third sign of madness.\n") - 1 <= 64, "roster_access: the pieces of a compose() fit a wave");

// nuts_roster_access_order's rule.  Keys: the actor's room, the room and the slot the word resolved to (-1: none).
struct AccessOrderArgs {
    const int32_t* room;         // [capacity] the roster's table: the actors' rooms
    const int32_t* slot;         // [k] the actors
    const int32_t* target_room;  // [k] what nuts_roster_access wrote
    const int32_t* target_slot;  // [k]
    int k;
    int8_t* outcome;             // [k] becomes kAccDeferred for a deferred event
    int32_t* clen;               // [4k] whose four texts become void

    static constexpr int kKeys = 3, kTexts = kAccTexts, kDeferred = kAccDeferred, kMapWords = kOrderRoomWords + kOrderSlotWords;
    __device__ void load(int b, bool live, int (&key)[kKeys]) const
    {
        key[0] = live ? room[slot[b]] : 0, key[1] = live ? target_room[b] : -1, key[2] = live ? target_slot[b] : -1;
    }
    static __device__ bool hit(const int (&key)[kKeys], const uint32_t* maps)
    {
        return bit_of(maps, key[0]) || (key[1] >= 0 && bit_of(maps, key[1])) || (key[2] >= 0 && bit_of(maps + kOrderRoomWords, key[2]));
    }
    static __device__ void touch(const int (&key)[kKeys], int outcome, uint32_t* maps)
    {                                       // setting an access touches the room, an invitation the invited slot
        if (outcome == kAccSetPrivate || outcome == kAccSetPublic) set_bit(maps, key[1]);
        else if (outcome == kAccInvited) set_bit(maps + kOrderRoomWords, key[2]);
    }
    __device__ void also_void(int) const {}
};

// ------------------------------------------------------------------ the clone commands, of a resident roster
//
// create_clone(), destroy_clone(), clone_say() and clone_hear() (nuts333.c:7100-7210, 7293-7357): .clone, .destroy, .csay and
// .chear, commands 73, 74, 78 and 79.  As with the room's door, the device decides and composes and writes no kept table;
// the host binding creates, destroys and sets the records in its mirrors afterwards.  It reads the five tables
// nuts_roster_access reads.
// An event has six texts: the line the actor's room gets without the actor ("here"), the line the clone's room gets
// ("there"), "Room access returned to ~FGPUBLIC.\n" for a room a destroyed clone leaves too empty ("reset"), the line the
// clone speaks ("said"), the actor's own line ("reply") and the line the owner of a clone destroyed by another gets
// ("notice").  With K events, text kind * K + k is event k's text of that kind, in that order: the 4K room lines first, as
// nuts_roster_speak_plan wants them.  Five kinds have slots of fixed width; a said line has inpstr's length and kSpeakSlack,
// as nuts_roster_speak's lines have.  The slots lie in the texts' order, so that var_at() keeps the variants apart.
//   clone    nuts_roster_clone, ONE BLOCK PER EVENT, in the shape of nuts_roster_access.  word[1] and word[2] are found as
//            np_wordfind finds them in inpstr.  The block runs get_user over the capitalised word[2] (a .destroy of
//            another's clone; first, while little else is live), get_room over word[1], and then walks the clone records
//            twice, lanes striding in block-sized steps: for the lowest record of (owner, room), a ballot per step and the
//            waves' minima through LDS; then for the owner's records in all and those below that lowest one (the two counts
//            create_clone's loop comes down to, see clone_created), and, for a destroy in a room that is exactly PRIVATE,
//            the head-count reset_access takes without the destroyed record: popcounts of ballots, summed per wave and once
//            across the waves through LDS.  No atomics: the same answer on every run.  Wave 0 decides in the reference's
//            order and composes; lane 0 stores the lengths, the outcome, the room, the slot and the record the event
//            resolved to, whether the room returns to public, and rm / sender / com / flags of the four room lines.
//            Blocks past the events copy freshly uploaded tables into the kept allocations.
//   order    nuts_roster_clone_order, ONE WAVE: order_events by its own rule.  A created clone touches its owner and its
//            room, a destroyed one likewise.  An event whose owner -- the user get_user found, else the actor -- or
//            resolved room an earlier event of the call that was not itself deferred touched is deferred: its outcome
//            becomes kCloneDeferred, its six texts void, and nothing of it is recorded.
//   plan     nuts_roster_speak_plan with 4K room lines and 2K single-recipient texts.
//   record   nuts_roster_record over the said lines, as after nuts_roster_speak.
constexpr int kComClone = 73, kComDestroy = 74, kComCsay = 78, kComChear = 79;             // enum np_com
// the first three are the clone_hear values a .chear sets (nuts333.h: CLONE_HEAR_NOTHING, CLONE_HEAR_SWEARS, CLONE_HEAR_ALL)
constexpr int kCloneHearNothing = 0, kCloneHearSwears = 1, kCloneHearAll = 2, kCloneCreated = 3, kCloneDestroyed = 4, kCloneSaid = 5,
              kCloneNoRoom = 6, kClonePrivate = 7, kCloneAlready = 8, kCloneMax = 9, kCloneDestroyNoRoom = 10, kCloneDestroyNobody = 11,
              kCloneDestroyLevel = 12, kCloneDestroyNoneOwn = 13, kCloneDestroyNoneTheirs = 14, kCloneCsayMuzzled = 15,
              kCloneCsayUsage = 16, kCloneCsayNoRoom = 17, kCloneCsayNone = 18, kCloneChearUsage = 19, kCloneChearNoRoom = 20,
              kCloneChearNone = 21, kCloneDeferred = 22;
constexpr int kCloneTexts = 6, kCloneLines = 4;            // here, there, reset, said: the room lines; then reply, notice
constexpr int kCloneHere = 0, kCloneThere = 1, kCloneReset = 2, kCloneSaidText = 3, kCloneReply = 4, kCloneNotice = 5;
// the longest texts: "~FB~OL" + name + " whispers a haunting spell...\n"; "~FB~OLA clone of " + name + " appears in a swirling
// magical mist!\n"; "Room access returned to ~FGPUBLIC.\n"; "~FB~OLYou whisper a haunting spell and a clone is created in the "
// + room name + ".\n"; "~OLSYSTEM: ~FR" + name + " has destroyed your clone in the " + room name + ".\n"
constexpr int kCloneHereMax = 6 + kNameLen + 30, kCloneThereMax = 17 + kNameLen + 37, kCloneResetMax = 35,
              kCloneReplyMax = 65 + kRoomNameLen + 2, kCloneNoticeMax = 14 + kNameLen + 33 + kRoomNameLen + 2;
constexpr int kCloneHereRow = 48, kCloneThereRow = 68, kCloneResetRow = 36, kCloneReplyRow = 88, kCloneNoticeRow = 84;   // their slots
constexpr int kCloneLineRows = kCloneHereRow + kCloneThereRow + kCloneResetRow;             // an event's fixed bytes before its said line
constexpr int kCloneRow = kCloneLineRows + kCloneReplyRow + kCloneNoticeRow;                // and in all, beside the said line
// Where text kind * k + b of a call of k events over text_bytes of inpstr has its slot, text_off being where event b's inpstr
// starts: the here lines, the there lines, the reset lines, the said lines as ctext_at() lays them, the replies, the notices.
constexpr int64_t clone_text_at(int kind, int64_t b, int64_t k, int64_t text_off, int64_t text_bytes)
{
    return kind == kCloneHere ? kCloneHereRow * b
           : kind == kCloneThere ? kCloneHereRow * k + kCloneThereRow * b
           : kind == kCloneReset ? (kCloneHereRow + kCloneThereRow) * k + kCloneResetRow * b
           : kind == kCloneSaidText ? kCloneLineRows * k + ctext_at(text_off, b)
           : kind == kCloneReply ? kCloneLineRows * k + ctext_at(text_bytes, k) + kCloneReplyRow * b
           : kCloneLineRows * k + ctext_at(text_bytes, k) + kCloneReplyRow * k + kCloneNoticeRow * b;
}
constexpr int64_t clone_text_bytes(int64_t k, int64_t text_bytes) { return kCloneRow * k + ctext_at(text_bytes, k); }

// create_clone's walk of the user list (c:7122-7135) without the walk.  Of the actor's records in list order, `found` says
// that one stands in the room, `before` how many precede the first such one, `total` how many there are.  The loop answers
// "already" at that first one unless "maximum" came first, which it does at the max_clones-th record that stands elsewhere:
// when max_clones >= 1 and before >= max_clones.  Past the list it has counted every record, all of them elsewhere.
// ++cnt == max_clones never holds for max_clones 0.  1: already, 2: maximum, 0: created.
__host__ __device__ constexpr int clone_created(bool found, int before, int total, int max_clones)
{
    return found && (max_clones < 1 || before < max_clones) ? 1 : max_clones >= 1 && total >= max_clones ? 2 : 0;
}

struct CloneArgs : EventArgs {   // slotf: login
    int32_t* found;              // [3k] the room the event is about (-1: none, or the step was not reached); at k, the slot
                                 // get_user found (-1: none, or it was not asked); at 2k, the record found or destroyed (-1:
                                 // none).  One array, and one below: the kernel's arguments stay in scalar registers
    uint8_t* reset;              // [k] 1: the room returns to public
    int32_t* line;               // [12k] the room lines' rooms, as SpeakPlanArgs.rm; at 4k, their senders (-1: none); at 8k,
                                 // their com_num
    uint8_t* flags;              // [k] bit 2: record the said line
    const uint8_t* com;          // [k] NP_CLONE, NP_DESTROY, NP_CSAY or NP_CHEAR
    int look_rooms, clones, gatecrash_level, min_private_users, max_clones, record;
    const uint8_t* speech;       // the tables this call reads, the uploads or the kept ones: the speaker state (name, vis, level),
    const uint8_t* records;      // the clone records as take_clones lays them out,
    const uint8_t* rooms;        // the room records,
    const uint8_t* go;           // [capacity * 88] and the go table: invite_room
    Kept kept[4];                // the speaker state, the go table, the room records, the clone records
};

// Who stands in room rm, as reset_access counts (c:2095): the slots with that room, a name and no login flag, and the clone
// records standing there but record `skip`, by a whole block; each wave returns its own share.  nuts_roster_go and
// nuts_roster_access keep their own loops: they skip a slot or nobody where this skips a record, and so their code stays
// what their device tests passed with.
__device__ __forceinline__ int wave_head_count(const int32_t* room, const uint8_t* slotf, const uint8_t* speech, int capacity,
                                               const int32_t* owner, const int32_t* croom, int clones, int rm, int skip)
{
    int cnt = 0;
    for (int base = 0; base < capacity; base += kBlock) {
        const int j = base + (int)threadIdx.x;
        const bool in_room = j < capacity && room[j] == rm && !(slotf[j] & kLogin) && speech[(size_t)j * kSpeechRec + kNameLen] != 0;
        cnt += __popcll(__ballot(in_room));
    }
    for (int base = 0; base < clones; base += kBlock) {
        const int r = base + (int)threadIdx.x;
        const bool in_room = r < clones && r != skip && owner[r] >= 0 && croom[r] == rm;
        cnt += __popcll(__ballot(in_room));
    }
    return cnt;
}

__device__ void roster_clone(const CloneArgs& c)
{
    if ((int)blockIdx.x >= c.k) {           // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(c.kept, ((int)blockIdx.x - c.k) * kBlock + (int)threadIdx.x);
        return;
    }
    __shared__ int s_room[kBlock / 64], s_exact[kBlock / 64], s_sub[kBlock / 64], s_min[kBlock / 64], s_total[kBlock / 64],
        s_before[kBlock / 64], s_pop[kBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int k = (int)blockIdx.x;
    const int slot = c.slot[k], com = c.com[k], wc = c.words[k], len = c.text_len[k];
    const uint8_t* in = c.text + c.text_off[k];

    // word[1] and word[2] as np_wordfind finds the line's second and third word (c:417-432): inpstr has lost the first
    uint32_t wordb = 0;
#pragma unroll
    for (int x = 0; x < kReadSlice; x++) {
        const int at = kReadSlice * lane + x;
        wordb |= (uint32_t)(at < len && (int8_t)in[at] > 32) << x;
    }
    const int w0 = first_from(wordb, 0, lane, len);
    const int w0_end = first_from(~wordb & 0xffffu, w0, lane, len);
    const int w1 = first_from(wordb, w0_end, lane, len);    // where np_remove_first's rest begins, too (c:2350-2358)
    const int w1_end = first_from(~wordb & 0xffffu, w1, lane, len);
    const int wlen = w0_end - w0 < kWordLen ? w0_end - w0 : kWordLen;
    const int wlen2 = w1_end - w1 < kWordLen ? w1_end - w1 : kWordLen;
    const uint8_t* word = in + w0;
    const uint8_t* word2 = in + w1;

    // get_user over the capitalised word[2] of a .destroy with a name (c:7179-7180), before anything else is kept: the search
    // is what needs registers most.  get_room comes first in the reference; the decisions below keep that order
    const bool want_user = com == kComDestroy && wc > 2;
    int best_exact = kNoMatch, best_sub = kNoMatch;
    if (want_user) {
        const UserMatch u = wave_get_user(c.speech, c.slotf, c.capacity, pack_word(word2, wlen2), wlen2, wave, lane);
        best_exact = u.exact;
        best_sub = u.sub;
    }

    const uint8_t* sp = c.speech + (size_t)slot * kSpeechRec;
    const int level = sp[kLevelByte];
    const int here = c.room[slot];          // a look room: the host checked it

    // what comes before get_room (c:7109, 7173, 7300-7307, 7328-7334); block-uniform
    int outcome = -1, rm = -1, hear = -1;
    bool want_room = false;
    if (com == kComClone || com == kComDestroy) {
        if (wc < 2) rm = here;
        else want_room = true;
    } else if (com == kComCsay) {
        if (sp[kNameLen + 1] & kMuzzled) outcome = kCloneCsayMuzzled;
        else if (wc < 3) outcome = kCloneCsayUsage;
        else want_room = true;
    } else {                                // strcmp(word[2], ...): exact
        const auto is = [&](const char* s, int n) {
            bool same = wlen2 == n;
            for (int i = 0; i < n && same; i++) same = word2[i] == (uint8_t)s[i];
            return same;
        };
        hear = is("all", 3) ? kCloneHearAll : is("swears", 6) ? kCloneHearSwears : is("nothing", 7) ? kCloneHearNothing : -1;
        if (wc < 3 || hear < 0) outcome = kCloneChearUsage;
        else want_room = true;
    }

    int best = want_room ? wave_get_room(c.rooms, c.look_rooms, word, wlen, wave, lane) : kNoMatch;
    if (lane == 0) {
        s_room[wave] = best;
        s_exact[wave] = best_exact;
        s_sub[wave] = best_sub;
    }
    __syncthreads();
    for (int w = 0; w < kBlock / 64; w++) {
        best = s_room[w] < best ? s_room[w] : best;
        best_exact = s_exact[w] < best_exact ? s_exact[w] : best_exact;
        best_sub = s_sub[w] < best_sub ? s_sub[w] : best_sub;
    }
    if (want_room) {
        if (best == kNoMatch) outcome = com == kComClone ? kCloneNoRoom : com == kComDestroy ? kCloneDestroyNoRoom
                                        : com == kComCsay ? kCloneCsayNoRoom : kCloneChearNoRoom;
        else rm = best;
    }
    int target = -1;
    if (outcome < 0 && want_user) {         // c:7180-7186
        target = best_exact != kNoMatch ? best_exact : best_sub != kNoMatch ? best_sub : -1;
        if (target < 0) outcome = kCloneDestroyNobody;
        else if (c.speech[(size_t)target * kSpeechRec + kLevelByte] >= level) outcome = kCloneDestroyLevel;
    }
    const int own = target >= 0 ? target : slot;
    const uint8_t* rrec = c.rooms + (size_t)(rm < 0 ? here : rm) * kRoomRec;
    const uint8_t access = rrec[kRrAccess];
    if (outcome < 0 && com == kComClone) {  // has_room_access, c:2416-2419
        const int32_t invite = *reinterpret_cast<const int32_t*>(c.go + (size_t)slot * kGoRec + kGoInvite);
        if ((access & kAccessPrivate) && level < c.gatecrash_level && invite != rm && !((access & kAccessFixed) && level >= kWiz))
            outcome = kClonePrivate;
    }

    // the lowest record of (owner, room): each wave's first hit is its lowest, the waves' minima meet in LDS
    const bool walk = outcome < 0;          // block-uniform
    const size_t slice = ((size_t)c.clones * sizeof(int32_t) + 255) & ~(size_t)255;
    const int32_t* owner = reinterpret_cast<const int32_t*>(c.records);
    const int32_t* croom = reinterpret_cast<const int32_t*>(c.records + slice);
    int m = kNoMatch;
    if (walk) {
        for (int base = 64 * wave; base < c.clones; base += kBlock) {          // wave-uniform
            const int r = base + lane;
            const uint64_t b = __ballot(r < c.clones && owner[r] == own && croom[r] == rm);
            if (b) {
                m = base + __ffsll((unsigned long long)b) - 1;
                break;
            }
        }
    }
    if (lane == 0) s_min[wave] = m;
    __syncthreads();
    for (int w = 0; w < kBlock / 64; w++) m = s_min[w] < m ? s_min[w] : m;
    const bool found = m != kNoMatch;

    // the two counts of create_clone's loop; the head-count of a room a destroyed clone may leave too empty (c:7192)
    int total = 0, before = 0, cnt = 0;
    if (walk && com == kComClone) {
        for (int base = 0; base < c.clones; base += kBlock) {
            const int r = base + (int)threadIdx.x;
            const bool mine = r < c.clones && owner[r] == own;
            total += __popcll(__ballot(mine));
            before += __popcll(__ballot(mine && r < m));
        }
    }
    const bool counted = walk && com == kComDestroy && found && access == kAccessPrivate;
    if (counted) cnt = wave_head_count(c.room, c.slotf, c.speech, c.capacity, owner, croom, c.clones, rm, m);
    if (lane == 0) {
        s_total[wave] = total;
        s_before[wave] = before;
        s_pop[wave] = cnt;
    }
    __syncthreads();
    if (wave != 0) return;
    total = before = cnt = 0;
    for (int w = 0; w < kBlock / 64; w++) {
        total += s_total[w];
        before += s_before[w];
        cnt += s_pop[w];
    }

    // the four functions' decisions
    if (outcome < 0) {
        if (com == kComClone) {
            const int made = clone_created(found, before, total, c.max_clones);
            outcome = made == 1 ? kCloneAlready : made == 2 ? kCloneMax : kCloneCreated;
        } else if (com == kComDestroy) outcome = found ? kCloneDestroyed : target < 0 ? kCloneDestroyNoneOwn : kCloneDestroyNoneTheirs;
        else if (com == kComCsay) outcome = found ? kCloneSaid : kCloneCsayNone;
        else outcome = found ? hear : kCloneChearNone;
    }
    const bool returns = outcome == kCloneDestroyed && counted && cnt < c.min_private_users;
    const int rec = outcome <= kCloneSaid || outcome == kCloneAlready ? (outcome == kCloneCreated ? -1 : m) : -1;

    const int n = c.k;
    const auto slot_of = [&](int kind) { return c.ctext + c.ctext_off[kind * n + k]; };   // at its use: few scalars stay live
    const Piece none{nullptr, 0};
    const Piece name{sp, sp[kNameLen] < kNameLen ? sp[kNameLen] : kNameLen};
    const Piece shown = (sp[kNameLen + 1] & kVis) ? name : lit("A presence");
    const Piece rname{rrec, rrec[kRrNameLen] < kRoomNameLen ? rrec[kRrNameLen] : kRoomNameLen};
    const uint8_t* tp = c.speech + (size_t)own * kSpeechRec;
    const Piece tname{tp, tp[kNameLen] < kNameLen ? tp[kNameLen] : kNameLen};
    int here_len = -1, there_len = -1, reset_len = -1, said_len = -1, reply_len = 0, notice_len = -1;
    const auto reply = [&](Piece p0, Piece p1, Piece p2) {             // three pieces, each shorter than a wave
        const Piece a0[5] = {p0, none, none, none, none}, a1[5] = {p1, p2, none, none, none};
        append(slot_of(kCloneReply), kCloneReplyRow, reply_len, a0, nullptr, 0, false, lane, c.violations);
        append(slot_of(kCloneReply), kCloneReplyRow, reply_len, a1, nullptr, 0, false, lane, c.violations);
    };
    switch (outcome) {
    case kCloneHearNothing: reply(lit("Clone will now hear nothing.\n"), none, none); break;
    case kCloneHearSwears: reply(lit("Clone will now only hear swearing.\n"), none, none); break;
    case kCloneHearAll: reply(lit("Clone will now hear everything.\n"), none, none); break;
    case kCloneCreated:                     // c:7150-7155
        if (rm == here) reply(lit("~FB~OLYou whisper a haunting spell and a clone "), lit("is created here.\n"), none);
        else {
            reply(lit("~FB~OLYou whisper a haunting spell and a clone "), lit("is created in the "), rname);
            reply(lit(".\n"), none, none);
        }
        break;
    case kCloneDestroyed: reply(lit("~FM~OLYou whisper a sharp spell and the clone is destroyed.\n"), none, none); break;
    case kCloneSaid: reply_len = -1; break;                            // say() of a clone writes nothing to its owner
    case kCloneNoRoom:
    case kCloneDestroyNoRoom:
    case kCloneCsayNoRoom:
    case kCloneChearNoRoom: reply(lit("There is no such room.\n"), none, none); break;
    case kClonePrivate: reply(lit("That room is currently private, "), lit("you cannot create a clone there.\n"), none); break;
    case kCloneAlready: reply(lit("You already have a clone in the "), rname, lit(".\n")); break;
    case kCloneMax: reply(lit("You already have the maximum number of clones allowed.\n"), none, none); break;
    case kCloneDestroyNobody: reply(lit("There is no one of that name logged on.\n"), none, none); break;
    case kCloneDestroyLevel: reply(lit("You cannot destroy the clone of a user "), lit("of an equal or higher level.\n"), none); break;
    case kCloneDestroyNoneOwn: reply(lit("You do not have a clone in the "), rname, lit(".\n")); break;
    case kCloneDestroyNoneTheirs:           // c:7208, "a clone the" as it stands
        reply(tname, lit(" does not have a clone the "), rname);
        reply(lit(".\n"), none, none);
        break;
    case kCloneCsayMuzzled: reply(lit("You are muzzled, your clone cannot speak.\n"), none, none); break;
    case kCloneCsayUsage: reply(lit("Usage: csay <room clone is in> <message>\n"), none, none); break;
    case kCloneChearUsage: reply(lit("Usage: chear <room clone is in> all/swears/nothing\n"), none, none); break;
    default: reply(lit("You do not have a clone in that room.\n"), none, none); break;     // kCloneCsayNone, kCloneChearNone
    }
    bool whole = reply_len >= 0 || outcome == kCloneSaid;
    if (outcome == kCloneCreated) {         // c:7156-7160: invisname here, the real name there
        const Piece h[5] = {lit("~FB~OL"), shown, lit(" whispers a haunting spell...\n"), none, none};
        const Piece t0[5] = {lit("~FB~OLA clone of "), name, none, none, none};
        const Piece t1[5] = {lit(" appears in a swirling magical mist!\n"), none, none, none, none};
        here_len = compose(slot_of(kCloneHere), kCloneHereRow, h, nullptr, 0, false, lane, c.violations);
        there_len = 0;
        append(slot_of(kCloneThere), kCloneThereRow, there_len, t0, nullptr, 0, false, lane, c.violations);
        append(slot_of(kCloneThere), kCloneThereRow, there_len, t1, nullptr, 0, false, lane, c.violations);
        whole = whole && here_len >= 0 && there_len >= 0;
    } else if (outcome == kCloneDestroyed) {               // c:7192-7202
        const Piece h[5] = {lit("~FM~OL"), shown, lit(" whispers a sharp spell...\n"), none, none};
        const Piece t[5] = {lit("~FM~OLThe clone of "), tname, lit(" shimmers and vanishes.\n"), none, none};
        here_len = compose(slot_of(kCloneHere), kCloneHereRow, h, nullptr, 0, false, lane, c.violations);
        there_len = compose(slot_of(kCloneThere), kCloneThereRow, t, nullptr, 0, false, lane, c.violations);
        whole = whole && here_len >= 0 && there_len >= 0;
        if (returns) {
            const Piece r[5] = {lit("Room access returned to ~FGPUBLIC.\n"), none, none, none, none};
            reset_len = compose(slot_of(kCloneReset), kCloneResetRow, r, nullptr, 0, false, lane, c.violations);
            whole = whole && reset_len >= 0;
        }
        if (own != slot) {
            const Piece v0[5] = {lit("~OLSYSTEM: ~FR"), name, lit(" has destroyed your clone in the "), none, none};
            const Piece v1[5] = {rname, lit(".\n"), none, none, none};
            notice_len = 0;
            append(slot_of(kCloneNotice), kCloneNoticeRow, notice_len, v0, nullptr, 0, false, lane, c.violations);
            append(slot_of(kCloneNotice), kCloneNoticeRow, notice_len, v1, nullptr, 0, false, lane, c.violations);
            whole = whole && notice_len >= 0;
        }
    } else if (outcome == kCloneSaid) {     // say() of a clone, c:4080-4089: the owner's name as it is, no swear check
        const uint8_t last = len > 0 ? in[len - 1] : 0;    // the last byte of the rest is inpstr's last
        const Piece verb = last == '?' ? lit("ask") : last == '!' ? lit("exclaim") : lit("say");
        const Piece l[5] = {lit("Clone of "), name, lit(" "), verb, lit("s: ")};
        said_len = compose(slot_of(kCloneSaidText), len + kSpeakSlack, l, in + w1, len - w1, true, lane, c.violations);
        whole = said_len >= 0;
    }
    if (!whole) here_len = there_len = reset_len = said_len = reply_len = notice_len = -1;             // a violation: the call fails
    if (lane == 0) {
        c.clen[kCloneHere * n + k] = here_len;
        c.clen[kCloneThere * n + k] = there_len;
        c.clen[kCloneReset * n + k] = reset_len;
        c.clen[kCloneSaidText * n + k] = said_len;
        c.clen[kCloneReply * n + k] = reply_len;
        c.clen[kCloneNotice * n + k] = notice_len;
        c.outcome[k] = (int8_t)outcome;
        c.found[k] = rm;
        c.found[n + k] = target;
        c.found[2 * n + k] = rec;
        c.reset[k] = returns && whole;
        const int to = rm < 0 ? here : rm;
        int32_t* lrm = c.line + k;
        int32_t* sender = lrm + kCloneLines * n;
        int32_t* com_num = sender + kCloneLines * n;
        lrm[kCloneHere * n] = here;         // write_room_except(user->room, text, user)
        sender[kCloneHere * n] = slot;
        lrm[kCloneThere * n] = to;          // write_room_except(rm, text, user) of a created clone, write_room(rm, text) of a destroyed one
        sender[kCloneThere * n] = outcome == kCloneCreated ? slot : -1;
        lrm[kCloneReset * n] = lrm[kCloneSaidText * n] = to;                   // write_room(rm, text): nobody is excepted
        sender[kCloneReset * n] = sender[kCloneSaidText * n] = -1;
        for (int kind = 0; kind < kCloneLines; kind++) com_num[kind * n] = com;
        c.flags[k] = said_len >= 0 && c.record ? kRecordBit : 0;
    }
}

static_assert(kCloneHereMax == 48 && kCloneThereMax == 66 && kCloneResetMax == 35 && kCloneReplyMax == 87 && kCloneNoticeMax == 81 &&
              kCloneHereMax <= kCloneHereRow && kCloneThereMax <= kCloneThereRow && kCloneResetMax <= kCloneResetRow &&
              kCloneReplyMax <= kCloneReplyRow && kCloneNoticeMax <= kCloneNoticeRow, "roster_clone: the longest texts fit their slots");
static_assert(sizeof(" whispers a haunting spell...\n") - 1 == 30 && sizeof("~FB~OLA clone of ") - 1 == 17 &&
              sizeof(" appears in a swirling magical mist!\n") - 1 == 37 && sizeof("Room access returned to ~FGPUBLIC.\n") - 1 == kCloneResetMax &&
              sizeof("~FB~OLYou whisper a haunting spell and a clone is created in the ") - 1 == 65 && sizeof("~OLSYSTEM: ~FR") - 1 == 14 &&
              sizeof(" has destroyed your clone in the ") - 1 == 33 && 6 + kNameLen + sizeof(" whispers a sharp spell...\n") - 1 <= kCloneHereMax &&
              sizeof("~FM~OLThe clone of  shimmers and vanishes.\n") - 1 + kNameLen <= kCloneThereMax &&
              sizeof(" does not have a clone the .\n") - 1 + kNameLen + kRoomNameLen <= kCloneReplyMax &&
              sizeof("You cannot destroy the clone of a user of an equal or higher level.\n") - 1 <= kCloneReplyMax,
              "roster_clone: the texts are as long as counted");
static_assert(kCloneHereRow % 4 == 0 && kCloneThereRow % 4 == 0 && kCloneResetRow % 4 == 0 && kCloneReplyRow % 4 == 0 &&
              kCloneNoticeRow % 4 == 0 && kCloneHereRow - kCloneHereMax < 4 && kCloneThereRow - kCloneThereMax < 4 &&
              kCloneResetRow - kCloneResetMax < 4 && kCloneReplyRow - kCloneReplyMax < 4 && kCloneNoticeRow - kCloneNoticeMax < 4,
              "roster_clone: a row is its longest text rounded up to a whole word");
static_assert(kCloneThereRow < kTextSize && kCloneReplyRow < kTextSize && kCloneNoticeRow < kTextSize && kArrSize - 1 + kSpeakSlack < kTextSize,
              "roster_clone: a text fits speak_plan's LDS text");
static_assert(sizeof("Clone of  exclaims: ") - 1 + kNameLen + 1 <= kSpeakSlack && sizeof("Clone of  exclaims: ") - 1 + kNameLen <= 64 &&
              sizeof("~FM~OLYou whisper a sharp spell and the clone is destroyed.\n") - 1 <= 64 && 14 + kNameLen + 33 <= 64 &&
              sizeof("~FM~OLThe clone of  shimmers and vanishes.\n") - 1 + kNameLen <= 64 && kCloneHereMax <= 64,
              "roster_clone: a said line fits its slot, and the pieces of a compose() fit a wave");
static_assert(clone_created(true, 0, 1, 0) == 1 && clone_created(false, 5, 5, 0) == 0 && clone_created(true, 1, 2, 2) == 1 &&
              clone_created(true, 2, 3, 2) == 2 && clone_created(false, 1, 1, 2) == 0 && clone_created(false, 2, 2, 2) == 2,
              "clone_created: create_clone's loop on paper");

// nuts_roster_clone_order's rule.  Keys: the owner -- the slot get_user found, else the actor -- and the room the word
// resolved to (-1: none).
struct CloneOrderArgs {
    const int32_t* slot;         // [k] the actors
    const int32_t* target_room;  // [k] what nuts_roster_clone wrote
    const int32_t* target_slot;  // [k]
    int k;
    int8_t* outcome;             // [k] becomes kCloneDeferred for a deferred event
    int32_t* clen;               // [6k] whose six texts become void,
    uint8_t* reset;              // [k] whose room does not return to public,
    uint8_t* flags;              // [k] and whose said line is not recorded

    static constexpr int kKeys = 2, kTexts = kCloneTexts, kDeferred = kCloneDeferred, kMapWords = kOrderRoomWords + kOrderSlotWords;
    __device__ void load(int b, bool live, int (&key)[kKeys]) const
    {
        const int found = live ? target_slot[b] : -1;
        key[0] = live ? (found >= 0 ? found : slot[b]) : 0, key[1] = live ? target_room[b] : -1;
    }
    static __device__ bool hit(const int (&key)[kKeys], const uint32_t* maps)
    {
        return bit_of(maps + kOrderRoomWords, key[0]) || (key[1] >= 0 && bit_of(maps, key[1]));
    }
    static __device__ void touch(const int (&key)[kKeys], int outcome, uint32_t* maps)
    {
        if (outcome != kCloneCreated && outcome != kCloneDestroyed) return;     // key[1] >= 0: a clone has a room
        set_bit(maps + kOrderRoomWords, key[0]);
        set_bit(maps, key[1]);
    }
    __device__ void also_void(int b) const { reset[b] = 0, flags[b] = 0; }
};

// ------------------------------------------------------------------ the commands aimed at another user, of a resident roster
//
// move(), wake(), muzzle() and unmuzzle() (nuts333.c:4726-4768, 6496-6522, 6571-6703) with move_user(u, rm, 2)
// (c:4409-4459): .move, .wake, .muzzle and .unmuzzle, commands 21, 58, 60 and 61.  As with the clone commands, the device
// decides and composes and writes no kept table; the host binding moves the targets and sets their muzzles in its mirrors
// afterwards.  It reads the five tables nuts_roster_go reads.  Byte 15 of a slot's speaker state is its muzzle level: a slot's
// muzzle is that byte when the muzzled bit is set and the byte is not 0, WIZ -- the lowest level that can type .muzzle -- when
// the bit is set and the byte is 0, and 0 when the bit is clear.
// An event has six texts in slots of fixed width: the chant line the actor's room gets without the actor ("here"), the vortex
// line the room entered gets ("enter"), the giant-hand line the room left gets without the target ("leave"), "Room access
// returned to ~FGPUBLIC.\n" for a room left too empty ("reset"), the actor's own line ("reply") and the target's own line
// ("notice").  With K events, text kind * K + k is event k's text of that kind, in that order: the 4K room lines first, as
// nuts_roster_speak_plan wants them.
//   act      nuts_roster_act, ONE BLOCK PER EVENT, in the shape of nuts_roster_access.  word[1] and word[2] are found as
//            nuts_roster_clone finds them.  The block runs get_user over the capitalised word[1] (first, while little else is
//            live), get_room over word[2] of a .move of three words -- otherwise the room is the actor's --, and for a move
//            that happens out of a room that is exactly PRIVATE the head-count of the room left without the target, as
//            nuts_roster_go takes it: popcounts of ballots, summed per wave and across the waves through LDS.  No atomics:
//            the same answer on every run.  Wave 0 decides in the reference's order and composes; lane 0 stores the lengths,
//            the outcome, the slot found, the room resolved, the room left, whether it returns to public, and rm / sender /
//            com of the four room lines: the here line to the actor's room with the actor as sender, the enter line to the
//            room entered without one, the leave and the reset line to the room left with the target as sender.
//            Blocks past the events copy freshly uploaded tables into the kept allocations.
//   order    nuts_roster_act_order, ONE WAVE: order_events by its own rule.  A move touches the target's slot, the room left
//            and the room entered; a muzzle set or removed touches the target's slot.  An event whose actor's slot or room,
//            found slot, that slot's room or resolved room an earlier event of the call that was not itself deferred
//            touched is deferred: its outcome becomes kActDeferred, its six texts void, and its room does not return.
//   plan     nuts_roster_speak_plan with 4K room lines and 2K single-recipient texts.
constexpr int kComMove = 21, kComWake = 58, kComMuzzle = 60, kComUnmuzzle = 61;            // enum np_com
constexpr int kMuzzleByte = kNameLen + 3;                  // the muzzle level in a slot's speaker state
// the effective ones first -- an event moved iff its outcome is at most kActMovedUnseen --, then a branch of the reference each
constexpr int kActMoved = 0, kActMovedUnseen = 1, kActMuzzled = 2, kActUnmuzzled = 3, kActWoken = 4, kActMoveUsage = 5,
              kActMoveNobody = 6, kActMoveNoRoom = 7, kActMoveSelf = 8, kActMoveLevel = 9, kActMoveAlready = 10, kActMovePrivate = 11,
              kActMoveAway = 12, kActWakeUsage = 13, kActWakeMuzzled = 14, kActWakeNobody = 15, kActWakeSelf = 16, kActWakeAfk = 17,
              kActMuzzleUsage = 18, kActMuzzleAbsent = 19, kActMuzzleSelf = 20, kActMuzzleLevel = 21, kActMuzzleAlready = 22,
              kActUnmuzzleUsage = 23, kActUnmuzzleAbsent = 24, kActUnmuzzleSelf = 25, kActUnmuzzleNot = 26, kActUnmuzzleAbove = 27,
              kActDeferred = 28;
constexpr int kActTexts = 6, kActLines = 4;                // here, enter, leave, reset: the room lines; then reply, notice
constexpr int kActHere = 0, kActEnter = 1, kActLeave = 2, kActReset = 3, kActReply = 4, kActNotice = 5;
// the longest texts: "~FT~OL" + name + " chants an ancient spell...\n"; "~FT~OL" + name + " falls out of a magical blue
// vortex!\n"; "~FT~OLA giant hand grabs " + name + " who is pulled into a magical blue vortex!\n"; "Room access returned to
// ~FGPUBLIC.\n"; name + "'s muzzle is set to level " + a level's name + ", you do not have the power to remove it.\n";
// "\n~FT~OLA giant hand grabs you and pulls you into a magical blue vortex!\n"
constexpr int kActHereMax = 6 + kNameLen + 28, kActEnterMax = 6 + kNameLen + 37, kActLeaveMax = 25 + kNameLen + 43, kActResetMax = 35,
              kActReplyMax = kNameLen + 26 + 4 + 42, kActNoticeMax = 72;
constexpr int kActHereRow = 48, kActEnterRow = 56, kActLeaveRow = 80, kActResetRow = 36, kActReplyRow = 84, kActNoticeRow = 72;
constexpr int kActRow = kActHereRow + kActEnterRow + kActLeaveRow + kActResetRow + kActReplyRow + kActNoticeRow;
constexpr int act_row(int kind)
{
    return kind == kActHere ? kActHereRow : kind == kActEnter ? kActEnterRow : kind == kActLeave ? kActLeaveRow
           : kind == kActReset ? kActResetRow : kind == kActReply ? kActReplyRow : kActNoticeRow;
}
// Where text kind * k + b of a call of k events has its slot: the kinds in their order, each kind's rows event by event.
constexpr int64_t act_text_at(int kind, int64_t b, int64_t k)
{
    int64_t before = 0;
    for (int i = 0; i < kind; i++) before += act_row(i);
    return before * k + act_row(kind) * b;
}

struct ActArgs : EventArgs {     // slotf: login
    int32_t* found;              // [3k] the slot get_user found (-1: none, or it was not asked); at k, the room the event is
                                 // about (-1: get_room found none, or was not reached); at 2k, the found slot's room (-1: no
                                 // slot).  One array, and one below: the kernel's arguments stay in scalar registers
    uint8_t* returned;           // [k] 1: the room left returns to public
    int32_t* line;               // [12k] the room lines' rooms, as SpeakPlanArgs.rm; at 4k, their senders (-1: none); at 8k,
                                 // their com_num
    const uint8_t* com;          // [k] NP_MOVE, NP_WAKE, NP_MUZZLE or NP_UNMUZZLE
    int look_rooms, clones, gatecrash_level, min_private_users;
    const uint8_t* speech;       // the tables this call reads, the uploads or the kept ones: the speaker state (name, vis, level, muzzle),
    const uint8_t* records;      // the clone records as take_clones lays them out (nullptr: the roster has none),
    const uint8_t* rooms;        // the room records,
    const uint8_t* go;           // [capacity * 88] and the go table: invite_room
    Kept kept[4];                // the clone records, the room records, the go table, the speaker state
};

__device__ __forceinline__ Piece level_piece(int level)   // level_name[] (nuts333.c), as nuts_roster_who prints it
{
    return level == kNew ? lit("NEW") : level == kUser ? lit("USER") : level == kWiz ? lit("WIZ") : level == kArch ? lit("ARCH") : lit("GOD");
}

// p0, then p1 and p2, behind what a text already holds: two compose()s, each shorter than a wave.
__device__ __forceinline__ void append3(uint8_t* dst, int cap, int& at, Piece p0, Piece p1, Piece p2, int lane, int* violations)
{
    const Piece none{nullptr, 0};
    const Piece a0[5] = {p0, none, none, none, none}, a1[5] = {p1, p2, none, none, none};
    append(dst, cap, at, a0, nullptr, 0, false, lane, violations);
    append(dst, cap, at, a1, nullptr, 0, false, lane, violations);
}

__device__ void roster_act(const ActArgs& e)
{
    if ((int)blockIdx.x >= e.k) {           // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(e.kept, ((int)blockIdx.x - e.k) * kBlock + (int)threadIdx.x);
        return;
    }
    __shared__ int s_room[kBlock / 64], s_exact[kBlock / 64], s_sub[kBlock / 64], s_pop[kBlock / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int k = (int)blockIdx.x;
    const int slot = e.slot[k], com = e.com[k], wc = e.words[k], len = e.text_len[k];
    const uint8_t* in = e.text + e.text_off[k];

    // word[1] and word[2] as np_wordfind finds the line's second and third word (c:417-432): inpstr has lost the first
    uint32_t wordb = 0;
#pragma unroll
    for (int x = 0; x < kReadSlice; x++) {
        const int at = kReadSlice * lane + x;
        wordb |= (uint32_t)(at < len && (int8_t)in[at] > 32) << x;
    }
    const int w0 = first_from(wordb, 0, lane, len);
    const int w0_end = first_from(~wordb & 0xffffu, w0, lane, len);
    const int w1 = first_from(wordb, w0_end, lane, len);
    const int w1_end = first_from(~wordb & 0xffffu, w1, lane, len);
    const int wlen = w0_end - w0 < kWordLen ? w0_end - w0 : kWordLen;
    const int wlen2 = w1_end - w1 < kWordLen ? w1_end - w1 : kWordLen;
    const uint8_t* word = in + w0;
    const uint8_t* word2 = in + w1;

    // get_user over the capitalised word[1], before anything else is kept: the search is what needs registers most.  A
    // muzzled waker is refused before it in the reference (c:6505); the decisions below keep that order
    int best_exact = kNoMatch, best_sub = kNoMatch;
    if (wc >= 2) {
        const UserMatch u = wave_get_user(e.speech, e.slotf, e.capacity, pack_word(word, wlen), wlen, wave, lane);
        best_exact = u.exact;
        best_sub = u.sub;
    }
    const bool want_room = com == kComMove && wc >= 3;     // c:4739-4744
    int best = want_room ? wave_get_room(e.rooms, e.look_rooms, word2, wlen2, wave, lane) : kNoMatch;
    if (lane == 0) {
        s_room[wave] = best;
        s_exact[wave] = best_exact;
        s_sub[wave] = best_sub;
    }
    __syncthreads();
    for (int w = 0; w < kBlock / 64; w++) {
        best = s_room[w] < best ? s_room[w] : best;
        best_exact = s_exact[w] < best_exact ? s_exact[w] : best_exact;
        best_sub = s_sub[w] < best_sub ? s_sub[w] : best_sub;
    }

    const uint8_t* sp = e.speech + (size_t)slot * kSpeechRec;
    const int level = sp[kLevelByte];
    const int here = e.room[slot];          // a look room: the host checked it

    // what comes before get_user (c:4733, 6502-6507, 6576, 6648); block-uniform
    int outcome = -1;
    if (wc < 2) outcome = com == kComMove ? kActMoveUsage : com == kComWake ? kActWakeUsage : com == kComMuzzle ? kActMuzzleUsage : kActUnmuzzleUsage;
    else if (com == kComWake && (sp[kNameLen + 1] & kMuzzled)) outcome = kActWakeMuzzled;
    const int target = outcome >= 0 ? -1 : best_exact != kNoMatch ? best_exact : best_sub != kNoMatch ? best_sub : -1;
    const uint8_t* tp = e.speech + (size_t)(target < 0 ? slot : target) * kSpeechRec;
    const int old = target < 0 ? -1 : e.room[target];
    int rm = here;

    // the four functions' decisions, in their order; block-uniform
    if (outcome < 0) {
        const int tlevel = tp[kLevelByte];
        const int muzzle = !(tp[kNameLen + 1] & kMuzzled) ? 0 : tp[kMuzzleByte] ? tp[kMuzzleByte] : kWiz;
        if (com == kComMove) {              // c:4736-4761
            if (want_room) rm = target < 0 || best == kNoMatch ? -1 : best;
            if (target < 0) outcome = kActMoveNobody;
            else if (rm < 0) outcome = kActMoveNoRoom;
            else if (target == slot) outcome = kActMoveSelf;
            else if (tlevel >= level) outcome = kActMoveLevel;
            else if (rm == old) outcome = kActMoveAlready;
            else {                          // has_room_access(user, rm), c:2416-2419: the actor's level and invitation
                const uint8_t access = e.rooms[(size_t)rm * kRoomRec + kRrAccess];
                const int32_t invite = *reinterpret_cast<const int32_t*>(e.go + (size_t)slot * kGoRec + kGoInvite);
                if ((access & kAccessPrivate) && level < e.gatecrash_level && invite != rm && !((access & kAccessFixed) && level >= kWiz))
                    outcome = kActMovePrivate;
                else if (old < 0 || old >= e.look_rooms) outcome = kActMoveAway;
                else outcome = (tp[kNameLen + 1] & kVis) ? kActMoved : kActMovedUnseen;
            }
        } else if (com == kComWake) {       // c:6508-6521
            outcome = target < 0 ? kActWakeNobody : target == slot ? kActWakeSelf : (tp[kNameLen + 1] & kAfk) ? kActWakeAfk : kActWoken;
        } else if (com == kComMuzzle) {     // c:6579-6598
            outcome = target < 0 ? kActMuzzleAbsent : target == slot ? kActMuzzleSelf : tlevel >= level ? kActMuzzleLevel
                      : muzzle >= level ? kActMuzzleAlready : kActMuzzled;
        } else {                            // c:6651-6669
            outcome = target < 0 ? kActUnmuzzleAbsent : target == slot ? kActUnmuzzleSelf : muzzle == 0 ? kActUnmuzzleNot
                      : muzzle > level ? kActUnmuzzleAbove : kActUnmuzzled;
        }
    }
    const bool moved = outcome <= kActMovedUnseen;

    // reset_access(old_room) after the move (c:2093-2096): who still stands in a room that is exactly PRIVATE
    const bool counted = moved && e.rooms[(size_t)old * kRoomRec + kRrAccess] == kAccessPrivate;    // block-uniform
    int stay = 0;
    if (counted) {
        for (int base = 0; base < e.capacity; base += kBlock) {
            const int j = base + (int)threadIdx.x;
            const bool in_room = j < e.capacity && j != target && e.room[j] == old && !(e.slotf[j] & kLogin) &&
                                 e.speech[(size_t)j * kSpeechRec + kNameLen] != 0;
            stay += __popcll(__ballot(in_room));
        }
        if (e.records) {                    // clones count (c:2095 walks the whole user list)
            const size_t slice = ((size_t)e.clones * sizeof(int32_t) + 255) & ~(size_t)255;
            const int32_t* owner = reinterpret_cast<const int32_t*>(e.records);
            const int32_t* croom = reinterpret_cast<const int32_t*>(e.records + slice);
            for (int base = 0; base < e.clones; base += kBlock) {
                const int r = base + (int)threadIdx.x;
                const bool in_room = r < e.clones && owner[r] >= 0 && croom[r] == old;
                stay += __popcll(__ballot(in_room));
            }
        }
    }
    if (lane == 0) s_pop[wave] = stay;
    __syncthreads();
    if (wave != 0) return;
    stay = 0;
    for (int w = 0; w < kBlock / 64; w++) stay += s_pop[w];
    const bool returns = counted && stay < e.min_private_users;

    const int n = e.k;
    const auto slot_of = [&](int kind) { return e.ctext + e.ctext_off[kind * n + k]; };   // at its use: few scalars stay live
    const Piece none{nullptr, 0};
    const Piece name{sp, sp[kNameLen] < kNameLen ? sp[kNameLen] : kNameLen};
    const Piece shown = (sp[kNameLen + 1] & kVis) ? name : lit("A presence");
    const Piece tname{tp, tp[kNameLen] < kNameLen ? tp[kNameLen] : kNameLen};
    const uint8_t* rrec = e.rooms + (size_t)(rm < 0 ? here : rm) * kRoomRec;
    const Piece rname{rrec, rrec[kRrNameLen] < kRoomNameLen ? rrec[kRrNameLen] : kRoomNameLen};
    int here_len = -1, enter_len = -1, leave_len = -1, reset_len = -1, reply_len = 0, notice_len = -1;
    const auto say = [&](int kind, int cap, int& at, Piece p0, Piece p1, Piece p2) {       // p0, and p1 + p2, each shorter than a wave
        append3(slot_of(kind), cap, at, p0, p1, p2, lane, e.violations);
    };
    const auto reply = [&](Piece p0, Piece p1, Piece p2) { say(kActReply, kActReplyRow, reply_len, p0, p1, p2); };
    switch (outcome) {
    case kActMoved:
    case kActMovedUnseen: reply(lit("~FT~OLYou chant an ancient spell...\n"), none, none); break;    // c:4762
    case kActMuzzled:                       // c:6592
        reply(lit("~FR~OL"), tname, lit(" now has a muzzle of level: ~RS~OL"));
        reply(level_piece(level), lit(".\n"), none);
        break;
    case kActUnmuzzled: reply(lit("~FG~OLYou remove "), tname, lit("'s muzzle.\n")); break;
    case kActWoken: reply(lit("Wake up call sent.\n"), none, none); break;
    case kActMoveUsage: reply(lit("Usage: move <user> [<room>]\n"), none, none); break;
    case kActMoveNobody:
    case kActWakeNobody: reply(lit("There is no one of that name logged on.\n"), none, none); break;
    case kActMoveNoRoom: reply(lit("There is no such room.\n"), none, none); break;
    case kActMoveSelf: reply(lit("Trying to move yourself this way is the fourth sign of madness.\n"), none, none); break;
    case kActMoveLevel: reply(lit("You cannot move a user of equal or higher "), lit("level than yourself.\n"), none); break;
    case kActMoveAlready:
        reply(tname, lit(" is already in the "), rname);
        reply(lit(".\n"), none, none);
        break;
    case kActMovePrivate:
        reply(lit("The "), rname, lit(" is currently private, "));
        reply(tname, lit(" cannot be moved there.\n"), none);
        break;
    case kActWakeUsage: reply(lit("Usage: wake <user>\n"), none, none); break;
    case kActWakeMuzzled: reply(lit("You are muzzled, you cannot wake anyone.\n"), none, none); break;
    case kActWakeSelf: reply(lit("Trying to wake yourself up is the eighth sign of madness.\n"), none, none); break;
    case kActWakeAfk: reply(lit("You cannot wake someone who is AFK.\n"), none, none); break;
    case kActMuzzleUsage: reply(lit("Usage: muzzle <user>\n"), none, none); break;
    case kActMuzzleSelf: reply(lit("Trying to muzzle yourself is the ninth sign of madness.\n"), none, none); break;
    case kActMuzzleLevel: reply(lit("You cannot muzzle a user of equal or higher "), lit("level than yourself.\n"), none); break;
    case kActMuzzleAlready: reply(tname, lit(" is already muzzled.\n"), none); break;
    case kActUnmuzzleUsage: reply(lit("Usage: unmuzzle <user>\n"), none, none); break;
    case kActUnmuzzleSelf: reply(lit("Trying to unmuzzle yourself is the tenth sign of madness.\n"), none, none); break;
    case kActUnmuzzleAbove: {               // c:6660: level_name[u->muzzled]
        const int muzzle = tp[kMuzzleByte] ? tp[kMuzzleByte] : kWiz;
        reply(tname, lit("'s muzzle is set to level "), level_piece(muzzle));
        reply(lit(", you do not have the power to remove it.\n"), none, none);
        break;
    }
    default: reply_len = -1; break;         // kActMoveAway and the two absent branches are the caller's; kActUnmuzzleNot
                                            // sprintf()s and writes nothing (c:6656-6658)
    }
    const bool silent = outcome == kActMoveAway || outcome == kActMuzzleAbsent || outcome == kActUnmuzzleAbsent || outcome == kActUnmuzzleNot;
    bool whole = reply_len >= 0 || silent;
    if (moved) {                            // c:4763-4765, then move_user(u, rm, 2), c:4423-4447
        here_len = 0;
        say(kActHere, kActHereRow, here_len, lit("~FT~OL"), shown, lit(" chants an ancient spell...\n"));
        if (outcome == kActMovedUnseen) {
            enter_len = leave_len = 0;
            say(kActEnter, kActEnterRow, enter_len, lit("A presence enters the room...\n"), none, none);
            say(kActLeave, kActLeaveRow, leave_len, lit("A presence leaves the room.\n"), none, none);
        } else {
            enter_len = leave_len = notice_len = 0;
            say(kActNotice, kActNoticeRow, notice_len, lit("\n~FT~OLA giant hand grabs you and pulls you "), lit("into a magical blue vortex!\n"), none);
            say(kActEnter, kActEnterRow, enter_len, lit("~FT~OL"), tname, lit(" falls out of a magical blue vortex!\n"));
            say(kActLeave, kActLeaveRow, leave_len, lit("~FT~OLA giant hand grabs "), tname, none);
            say(kActLeave, kActLeaveRow, leave_len, lit(" who is pulled into a magical blue vortex!\n"), none, none);
            whole = whole && notice_len >= 0;
        }
        whole = whole && here_len >= 0 && enter_len >= 0 && leave_len >= 0;
        if (returns) {                      // c:2097
            reset_len = 0;
            say(kActReset, kActResetRow, reset_len, lit("Room access returned to ~FGPUBLIC.\n"), none, none);
            whole = whole && reset_len >= 0;
        }
    } else if (outcome == kActWoken) {      // c:6518-6520
        notice_len = 0;
        say(kActNotice, kActNoticeRow, notice_len, lit("\07\n~BR*** "), shown, lit(" says: ~OL~LIWAKE UP!!!~RS~BR ***\n\n"));
        whole = whole && notice_len >= 0;
    } else if (outcome == kActMuzzled || outcome == kActUnmuzzled) {   // c:6594, 6665
        notice_len = 0;
        say(kActNotice, kActNoticeRow, notice_len, outcome == kActMuzzled ? lit("~FR~OLYou have been muzzled!\n") : lit("~FG~OLYou have been unmuzzled!\n"),
            none, none);
        whole = whole && notice_len >= 0;
    }
    if (!whole) here_len = enter_len = leave_len = reset_len = reply_len = notice_len = -1;         // a violation: the call fails
    if (lane == 0) {
        e.clen[kActHere * n + k] = here_len;
        e.clen[kActEnter * n + k] = enter_len;
        e.clen[kActLeave * n + k] = leave_len;
        e.clen[kActReset * n + k] = reset_len;
        e.clen[kActReply * n + k] = reply_len;
        e.clen[kActNotice * n + k] = notice_len;
        e.outcome[k] = (int8_t)outcome;
        e.found[k] = target;
        e.found[n + k] = rm;
        e.found[2 * n + k] = old;
        e.returned[k] = returns && whole;
        const int left = moved ? old : here;
        int32_t* lrm = e.line + k;
        int32_t* sender = lrm + kActLines * n;
        int32_t* com_num = sender + kActLines * n;
        lrm[kActHere * n] = here;           // write_room_except(user->room, text, user)
        sender[kActHere * n] = slot;
        lrm[kActEnter * n] = rm < 0 ? here : rm;               // write_room(rm, text): nobody is excepted
        sender[kActEnter * n] = -1;
        lrm[kActLeave * n] = lrm[kActReset * n] = left;        // the snapshot still has the target there
        sender[kActLeave * n] = sender[kActReset * n] = moved ? target : -1;
        for (int kind = 0; kind < kActLines; kind++) com_num[kind * n] = com;
    }
}

static_assert(kActHereMax == 46 && kActEnterMax == 55 && kActLeaveMax == 80 && kActResetMax == 35 && kActReplyMax == 84 && kActNoticeMax == 72 &&
              kActHereMax <= kActHereRow && kActEnterMax <= kActEnterRow && kActLeaveMax <= kActLeaveRow && kActResetMax <= kActResetRow &&
              kActReplyMax <= kActReplyRow && kActNoticeMax <= kActNoticeRow, "roster_act: the longest texts fit their slots");
static_assert(sizeof(" chants an ancient spell...\n") - 1 == 28 && sizeof(" falls out of a magical blue vortex!\n") - 1 == 37 &&
              sizeof("~FT~OLA giant hand grabs ") - 1 == 25 && sizeof(" who is pulled into a magical blue vortex!\n") - 1 == 43 &&
              sizeof("Room access returned to ~FGPUBLIC.\n") - 1 == kActResetMax && sizeof("'s muzzle is set to level ") - 1 == 26 &&
              sizeof(", you do not have the power to remove it.\n") - 1 == 42 && sizeof("A presence enters the room...\n") - 1 <= kActEnterMax &&
              sizeof("\n~FT~OLA giant hand grabs you and pulls you into a magical blue vortex!\n") - 1 == kActNoticeMax &&
              sizeof("\07\n~BR***  says: ~OL~LIWAKE UP!!!~RS~BR ***\n\n") - 1 + kNameLen <= kActNoticeMax &&
              sizeof("The  is currently private,  cannot be moved there.\n") - 1 + kRoomNameLen + kNameLen <= kActReplyMax &&
              sizeof("~FR~OL now has a muzzle of level: ~RS~OL.\n") - 1 + kNameLen + 4 <= kActReplyMax &&
              sizeof("You cannot muzzle a user of equal or higher level than yourself.\n") - 1 <= kActReplyMax &&
              sizeof(" is already in the .\n") - 1 + kNameLen + kRoomNameLen <= kActReplyMax, "roster_act: the texts are as long as counted");
static_assert(kActHereRow % 4 == 0 && kActEnterRow % 4 == 0 && kActLeaveRow % 4 == 0 && kActResetRow % 4 == 0 && kActReplyRow % 4 == 0 &&
              kActNoticeRow % 4 == 0 && kActHereRow - kActHereMax < 4 && kActEnterRow - kActEnterMax < 4 && kActLeaveRow - kActLeaveMax < 4 &&
              kActResetRow - kActResetMax < 4 && kActReplyRow - kActReplyMax < 4 && kActNoticeRow - kActNoticeMax < 4 && kActReplyRow < kTextSize,
              "roster_act: a row is its longest text rounded up to a whole word, and a text fits speak_plan's LDS text");
static_assert(sizeof("Trying to move yourself this way is the fourth sign of madness.\n") - 1 <= 64 &&
              kNameLen + sizeof(" is already in the ") - 1 + kRoomNameLen <= 64 && 4 + kRoomNameLen + sizeof(" is currently private, ") - 1 <= 64 &&
              6 + kNameLen + sizeof(" now has a muzzle of level: ~RS~OL") - 1 <= 64 && kNameLen + 26 + 4 <= 64 && kMuzzleByte < kSpeechRec &&
              sizeof("\n~FT~OLA giant hand grabs you and pulls you ") - 1 <= 64 && 10 + sizeof(" says: ~OL~LIWAKE UP!!!~RS~BR ***\n\n") - 1 <= 64,
              "roster_act: the pieces of a compose() fit a wave; the muzzle's byte");

// nuts_roster_act_order's rule.  Keys: the actor's slot and room, the slot get_user found (-1: none), that slot's room, and
// the room the event resolved to (-1: none).  A slot's room may be no look room: such a room has no bit and touches nothing.
struct ActOrderArgs {
    const int32_t* room;         // [capacity] the roster's table: the actors' rooms
    const int32_t* slot;         // [k] the actors
    const int32_t* found;        // [3k] what nuts_roster_act wrote: the slots found, the rooms resolved, the found slots' rooms
    int k;
    int8_t* outcome;             // [k] becomes kActDeferred for a deferred event
    int32_t* clen;               // [6k] whose six texts become void
    uint8_t* returned;           // [k] and whose room does not return

    static constexpr int kKeys = 5, kTexts = kActTexts, kDeferred = kActDeferred, kMapWords = kOrderRoomWords + kOrderSlotWords;
    __device__ void load(int b, bool live, int (&key)[kKeys]) const
    {
        key[0] = live ? slot[b] : 0, key[1] = live ? room[slot[b]] : -1, key[2] = live ? found[b] : -1;
        key[3] = live ? found[2 * k + b] : -1, key[4] = live ? found[k + b] : -1;
    }
    static __device__ bool room_bit(const uint32_t* maps, int r) { return r >= 0 && r < kMaxLookRooms && bit_of(maps, r); }
    static __device__ bool hit(const int (&key)[kKeys], const uint32_t* maps)
    {
        return bit_of(maps + kOrderRoomWords, key[0]) || room_bit(maps, key[1]) || (key[2] >= 0 && bit_of(maps + kOrderRoomWords, key[2])) ||
               room_bit(maps, key[3]) || room_bit(maps, key[4]);
    }
    static __device__ void touch(const int (&key)[kKeys], int outcome, uint32_t* maps)
    {
        if (outcome > kActUnmuzzled) return;                    // a move or a muzzle touches the target's slot,
        set_bit(maps + kOrderRoomWords, key[2]);
        if (outcome > kActMovedUnseen) return;                  // a move the room left and the room entered: both look rooms
        set_bit(maps, key[3]);
        set_bit(maps, key[4]);
    }
    __device__ void also_void(int b) const { returned[b] = 0; }
};

// ------------------------------------------------------------------ a user's own settings, of a resident roster
//
// toggle_mode (nuts333.c:4009), toggle_ignall (4463), toggle_prompt (4481), set_desc (4494), set_iophrase (4515), set_topic
// (4697), visibility (6434), toggle_charecho (6881), afk (7409), toggle_colour (7458), toggle_ignshout (7484) and
// toggle_igntell (7497): the fourteen commands a user sets its own state with, and the topic of its room.  They need no
// get_user, no get_room and no walk over the roster: an event reads its actor's own rows -- the speaker state, the table's
// flag byte, the AFK message, the description, the two phrases -- and for a .topic its room's record.  As with the door
// commands the device decides and composes and writes no kept table; the host binding applies the result afterwards.
// An event has three texts in slots of fixed width: the line write_room_except(user->room, text, user) sends ("here"), the
// actor's first write_user ("reply") and its second ("reply2": "AFK message set.\n", a write(2) of its own).  With K events
// text k is event k's here line, K + k its reply and 2K + k its reply2: the K room lines first, as nuts_roster_speak_plan
// wants them.
//   set      nuts_roster_set, ONE WAVE PER EVENT, four events per block, in the shape of nuts_roster_speak.  word[1] is
//            found as nuts_roster_go finds it, and where remove_first stops as nuts_roster_tell finds it.  The wave
//            decides in the reference's branch order, wave-uniformly, and composes: the reply from kSetReply, a fixed
//            part per outcome and behind it, where the line quotes one, the kept description, phrase or topic or the
//            inpstr; the here line with compose() / append().  Lane 0 stores the lengths, the outcome, and rm / sender /
//            com of the here line.  No atomics: the same bytes on every run.
//            Blocks past the events copy freshly uploaded tables into the kept allocations.
//   order    nuts_roster_set_order, ONE WAVE: order_events by its own rule.  An effective event touches its actor;
//            one that toggles ignall or colour also its actor's room, as the admit bitmaps and the colour bits of that
//            room's lines read them; a set topic the topic of its room.  An event whose actor an earlier event of the call
//            that was not itself deferred touched, or which has a here line in a room so touched, or which is a .topic in
//            a room whose topic was so set, is deferred: its outcome becomes kSetDeferred and its three texts void.  A
//            room is known by its rank among the rooms of the call's actors (the host's, below 65,536 as the slots are).
//   plan     nuts_roster_speak_plan with K room lines and 2K single-recipient texts.
constexpr int kComMode = 2, kComIgnall = 11, kComPrompt = 12, kComDesc = 13, kComInphr = 14, kComOutphr = 15, kComTopic = 20,
              kComVis = 55, kComInvis = 56, kComCharecho = 66, kComAfk = 82, kComColour = 84, kComIgnshout = 85,
              kComIgntell = 86;                              // enum np_com
constexpr uint8_t kPrompt = 32, kCharecho = 64;            // the last two bits of the flags byte of a slot's speaker state
// the outcomes, the effective ones first: kSetModeCommand .. kSetIgntellOff changed something
constexpr int kSetModeCommand = 0, kSetModeSpeech = 1, kSetIgnallOn = 2, kSetIgnallOff = 3, kSetPromptOn = 4, kSetPromptOff = 5,
              kSetDescSet = 6, kSetInphrSet = 7, kSetOutphrSet = 8, kSetTopicSet = 9, kSetVisible = 10, kSetInvisible = 11,
              kSetCharechoOn = 12, kSetCharechoOff = 13, kSetAfk = 14, kSetAfkLocked = 15, kSetColourOn = 16, kSetColourOff = 17,
              kSetIgnshoutOn = 18, kSetIgnshoutOff = 19, kSetIgntellOn = 20, kSetIgntellOff = 21, kSetColourTest = 22,
              kSetDescQuery = 23, kSetDescClone = 24, kSetDescLong = 25, kSetPhraseLong = 26, kSetInphrQuery = 27,
              kSetOutphrQuery = 28, kSetTopicNone = 29, kSetTopicQuery = 30, kSetTopicLong = 31, kSetAlreadyVisible = 32,
              kSetAlreadyInvisible = 33, kSetAfkLong = 34, kSetDeferred = 35;
constexpr int kSetTexts = 3;                               // here, reply, reply2
// the longest texts: name + " has set the topic to: " + a 60-byte topic + "\n"; "The current topic is: " + topic + "\n";
// "AFK message set.\n"
constexpr int kSetHereMax = kNameLen + 23 + kTopicLen + 1, kSetReplyMax = 22 + kTopicLen + 1, kSetReply2Max = 17;
constexpr int kSetHereRow = 96, kSetReplyRow = 84, kSetReply2Row = 20;      // their slots
constexpr int kSetRow = kSetHereRow + kSetReplyRow + kSetReply2Row;         // an event's bytes of composed text
constexpr int set_row(int kind) { return kind == 0 ? kSetHereRow : kind == 1 ? kSetReplyRow : kSetReply2Row; }
// Where text kind * k + b of a call of k events has its slot: the here lines, then the replies, then the second replies.
constexpr int64_t set_text_at(int kind, int64_t b, int64_t k)
{
    return (kind == 0 ? 0 : kind == 1 ? kSetHereRow : kSetHereRow + kSetReplyRow) * k + set_row(kind) * b;
}

// The actor's first line by outcome: a fixed part, and whether a quoted text and a newline follow it.
struct SetReply {
    char pre[79];
    uint8_t npre;
    bool quotes;
};
template <int N>
constexpr SetReply set_reply(const char (&pre)[N], bool quotes = false)
{
    static_assert(N <= 80, "set_reply: the part fits its field");
    SetReply r{};
    for (int i = 0; i < N - 1; i++) r.pre[i] = pre[i];
    r.npre = N - 1;
    r.quotes = quotes;
    return r;
}
__device__ const SetReply kSetReply[] = {
    set_reply("Now in COMMAND mode.\n"),                                                   // kSetModeCommand    c:4016
    set_reply("Now in SPEECH mode.\n"),                                                    // kSetModeSpeech     c:4013
    set_reply("You are now ignoring everyone.\n"),                                         // kSetIgnallOn       c:4467
    set_reply("You will now hear everyone again.\n"),                                      // kSetIgnallOff      c:4473
    set_reply("Prompt ~FGON.\n"),                                                          // kSetPromptOn       c:4488
    set_reply("Prompt ~FROFF.\n"),                                                         // kSetPromptOff      c:4485
    set_reply("Description set.\n"),                                                       // kSetDescSet        c:4510
    set_reply("In phrase set.\n"),                                                         // kSetInphrSet       c:4529
    set_reply("Out phrase set.\n"),                                                        // kSetOutphrSet      c:4538
    set_reply("Topic set to: ", true),                                                     // kSetTopicSet       c:4716
    set_reply("~FB~OLYou recite a melodic incantation and reappear.\n"),                   // kSetVisible        c:6442
    set_reply("~FB~OLYou recite a melodic incantation and fade out.\n"),                   // kSetInvisible      c:6451
    set_reply("Echoing for character mode clients ~FGON.\n"),                              // kSetCharechoOn     c:6885
    set_reply("Echoing for character mode clients ~FROFF.\n"),                             // kSetCharechoOff    c:6889
    set_reply("You are now AFK, press <return> to reset.\n"),                              // kSetAfk            c:7436, 7445
    set_reply("You are now AFK with the session locked, enter your password to unlock it.\n"),   // kSetAfkLocked c:7425
    set_reply("Colour ~FGON.\n"),                                                          // kSetColourOn       c:7478
    set_reply("Colour ~FROFF.\n"),                                                         // kSetColourOff      c:7473
    set_reply("You are now ignoring shouts and shout emotes.\n"),                          // kSetIgnshoutOn     c:7492
    set_reply("You are no longer ignoring shouts and shout emotes.\n"),                    // kSetIgnshoutOff    c:7488
    set_reply("You are now ignoring tells and private emotes.\n"),                         // kSetIgntellOn      c:7505
    set_reply("You are no longer ignoring tells and private emotes.\n"),                   // kSetIgntellOff     c:7501
    set_reply(""),                                                                         // kSetColourTest: the caller's twenty lines
    set_reply("Your current description is: ", true),                                      // kSetDescQuery      c:4499
    set_reply("You cannot have that description.\n"),                                      // kSetDescClone      c:4504
    set_reply("Description too long.\n"),                                                  // kSetDescLong       c:4507
    set_reply("Phrase too long.\n"),                                                       // kSetPhraseLong     c:4520
    set_reply("Your current in phrase is: ", true),                                        // kSetInphrQuery     c:4524
    set_reply("Your current out phrase is: ", true),                                       // kSetOutphrQuery    c:4533
    set_reply("No topic has been set yet.\n"),                                             // kSetTopicNone      c:4707
    set_reply("The current topic is: ", true),                                             // kSetTopicQuery     c:4709
    set_reply("Topic too long.\n"),                                                        // kSetTopicLong      c:4714
    set_reply("You are already visible.\n"),                                               // kSetAlreadyVisible c:6440
    set_reply("You are already invisible.\n"),                                             // kSetAlreadyInvisible c:6449
    set_reply("AFK message too long.\n"),                                                  // kSetAfkLong        c:7423, 7434
};
static_assert(sizeof(kSetReply) / sizeof(kSetReply[0]) == kSetDeferred, "kSetReply: a line for every outcome nuts_roster_set decides");

struct SetArgs : EventArgs {     // slotf: ignall
    int32_t* rm;                 // [k] the here lines' rooms, as SpeakPlanArgs.rm
    int32_t* sender;             // [k] and their senders
    int32_t* com_num;            // [k]
    const uint8_t* com;          // [k] one of the fourteen commands
    const int32_t* rid;          // [k] the rank of the actor's room among the rooms of the call's actors (nuts_roster_set_order)
    int blocks;                  // those that compose; the ones after them copy the uploaded tables
    const uint8_t* rooms;        // the tables this call reads, the uploads or the kept ones: the room records (nullptr: no .topic),
    const uint8_t* go;           // [capacity * 88] the go table (the two phrases),
    const uint8_t* afk;          // [capacity * 64] the AFK messages,
    const uint8_t* udesc;        // [capacity * 32] the users' descriptions,
    const uint8_t* speech;       // [capacity * 16] and the speaker state: name, vis, command_mode, afk, igntell, prompt, charmode_echo
    Kept kept[5];                // in that order
};

__device__ void roster_set(const SetArgs& a)
{
    if ((int)blockIdx.x >= a.blocks) {      // the tables just uploaded, into the kept allocations: a word per lane
        copy_kept(a.kept, ((int)blockIdx.x - a.blocks) * kBlock + (int)threadIdx.x);
        return;
    }
    const int lane = (int)threadIdx.x & 63;
    const int k = (int)blockIdx.x * (kBlock / 64) + ((int)threadIdx.x >> 6);      // wave-uniform
    if (k >= a.k) return;
    const int slot = a.slot[k], com = a.com[k], wc = a.words[k], len = a.text_len[k];
    const uint8_t* in = a.text + a.text_off[k];
    const uint8_t* sp = a.speech + (size_t)slot * kSpeechRec;
    const uint8_t state = sp[kNameLen + 1], listens = a.slotf[slot];
    const int here = a.room[slot];
    const bool vis = (state & kVis) != 0;

    // word[1] as np_wordfind finds the line's second word (c:417-432), and where remove_first stops behind it (c:2350-2358)
    uint32_t wordb = 0;
#pragma unroll
    for (int x = 0; x < kReadSlice; x++) {
        const int at = kReadSlice * lane + x;
        wordb |= (uint32_t)(at < len && (int8_t)in[at] > 32) << x;
    }
    const int w0 = first_from(wordb, 0, lane, len);
    const int w0_end = first_from(~wordb & 0xffffu, w0, lane, len);
    const int rest = first_from(wordb, w0_end, lane, len);
    const int wlen = w0_end - w0 < kWordLen ? w0_end - w0 : kWordLen;
    const uint8_t* word = in + w0;

    // the kept text a query quotes, the text a set stores, the message an .afk takes
    Piece quoted{nullptr, 0};
    const uint8_t* mesg = in;               // afk: the whole inpstr, or what follows "lock"
    int mesg_len = len;
    int outcome;
    if (com == kComMode) outcome = (state & kCommandMode) ? kSetModeSpeech : kSetModeCommand;               // c:4012-4017
    else if (com == kComIgnall) outcome = (listens & kIgnall) ? kSetIgnallOff : kSetIgnallOn;              // c:4466-4476
    else if (com == kComPrompt) outcome = (state & kPrompt) ? kSetPromptOff : kSetPromptOn;                // c:4484-4489
    else if (com == kComCharecho) outcome = (state & kCharecho) ? kSetCharechoOff : kSetCharechoOn;        // c:6884-6891
    else if (com == kComIgnshout) outcome = (listens & kIgnshout) ? kSetIgnshoutOff : kSetIgnshoutOn;      // c:7487-7493
    else if (com == kComIgntell) outcome = (state & kIgntell) ? kSetIgntellOff : kSetIgntellOn;            // c:7500-7506
    else if (com == kComVis) outcome = vis ? kSetAlreadyVisible : kSetVisible;                             // c:6438-6445
    else if (com == kComInvis) outcome = vis ? kSetInvisible : kSetAlreadyInvisible;                       // c:6448-6454
    else if (com == kComColour) {           // c:7465-7479
        if ((state & kCommandMode) && (listens & kIgnall) && (state & kCharecho)) outcome = kSetColourTest;
        else outcome = (listens & kColour) ? kSetColourOff : kSetColourOn;
    } else if (com == kComDesc) {           // c:4498-4510
        const bool clone = __ballot(lane + 7 <= wlen && word[lane] == '(' && word[lane + 1] == 'C' && word[lane + 2] == 'L' &&
                                    word[lane + 3] == 'O' && word[lane + 4] == 'N' && word[lane + 5] == 'E' && word[lane + 6] == ')') != 0;
        const uint8_t* d = a.udesc + (size_t)slot * kUserDescRow;
        quoted = Piece{d, d[kUserDescLen] < kUserDescLen ? d[kUserDescLen] : kUserDescLen};
        outcome = wc < 2 ? kSetDescQuery : clone ? kSetDescClone : len > kUserDescLen ? kSetDescLong : kSetDescSet;
    } else if (com == kComInphr || com == kComOutphr) {     // c:4519-4538
        const uint8_t* g = a.go + (size_t)slot * kGoRec;
        const bool inp = com == kComInphr;
        const int n = g[inp ? kGoInLen : kGoOutLen];
        quoted = Piece{g + (inp ? kGoIn : kGoOut), n < kPhraseLen ? n : kPhraseLen};
        outcome = len > kPhraseLen ? kSetPhraseLong : wc < 2 ? (inp ? kSetInphrQuery : kSetOutphrQuery) : inp ? kSetInphrSet : kSetOutphrSet;
    } else if (com == kComTopic) {          // c:4705-4721
        const uint8_t* rec = a.rooms + (size_t)here * kRoomRec;        // a look room: the host checked it
        quoted = Piece{rec + kRrTopic, rec[kRrTopicLen] < kTopicLen ? rec[kRrTopicLen] : kTopicLen};
        if (wc < 2) outcome = quoted.n ? kSetTopicQuery : kSetTopicNone;
        else {
            outcome = len > kTopicLen ? kSetTopicLong : kSetTopicSet;
            quoted = Piece{in, len};
        }
    } else {                                // afk, c:7413-7447
        outcome = kSetAfk;
        if (wc > 1) {
            const bool lock = w0_end - w0 == 4 && word[0] == 'l' && word[1] == 'o' && word[2] == 'c' && word[3] == 'k';
            if (lock) {
                outcome = kSetAfkLocked;
                mesg = in + rest;
                mesg_len = len - rest;
            }
            if (mesg_len > kAfkMesgLen) outcome = kSetAfkLong;
        } else mesg_len = 0;                // c:7445: the message is not looked at
    }

    const int n = a.k;
    uint8_t* here_t = a.ctext + a.ctext_off[k];
    uint8_t* reply_t = a.ctext + a.ctext_off[n + k];
    uint8_t* reply2_t = a.ctext + a.ctext_off[2 * n + k];
    const Piece none{nullptr, 0};
    const Piece nothing[5] = {none, none, none, none, none};
    const Piece name{sp, sp[kNameLen] < kNameLen ? sp[kNameLen] : kNameLen};
    int here_len = -1, reply_len = -1, reply2_len = -1;
    bool lines = false;                     // the event has a here line
    if (outcome != kSetColourTest) {        // the actor's line: the outcome's fixed part, then what it quotes and a newline
        const SetReply& fixed = kSetReply[outcome];
        reply_len = compose(reply_t, kSetReplyRow, nothing, reinterpret_cast<const uint8_t*>(fixed.pre), fixed.npre, false, lane, a.violations);
        if (fixed.quotes) append(reply_t, kSetReplyRow, reply_len, nothing, quoted.p, quoted.n, true, lane, a.violations);
    }
    if (outcome == kSetIgnallOn || outcome == kSetIgnallOff) {         // c:4468, 4474: user->name
        const Piece h[5] = {name, outcome == kSetIgnallOn ? lit(" is now ignoring everyone.\n") : lit(" is listening again.\n"), none, none, none};
        here_len = compose(here_t, kSetHereRow, h, nullptr, 0, false, lane, a.violations);
        lines = true;
    } else if (outcome == kSetVisible) {    // c:6443: user->name
        const Piece h0[5] = {lit("~FB~OLYou hear a melodic incantation chanted and "), name, none, none, none};
        const Piece h1[5] = {lit(" materialises!\n"), none, none, none, none};
        here_len = compose(here_t, kSetHereRow, h0, nullptr, 0, false, lane, a.violations);
        append(here_t, kSetHereRow, here_len, h1, nullptr, 0, false, lane, a.violations);
        lines = true;
    } else if (outcome == kSetInvisible) {  // c:6452
        const Piece h0[5] = {lit("~FB~OL"), name, none, none, none};
        const Piece h1[5] = {lit(" recites a melodic incantation and disappears!\n"), none, none, none, none};
        here_len = compose(here_t, kSetHereRow, h0, nullptr, 0, false, lane, a.violations);
        append(here_t, kSetHereRow, here_len, h1, nullptr, 0, false, lane, a.violations);
        lines = true;
    } else if (outcome == kSetTopicSet) {   // c:4718-4720: invisname for an invisible actor
        const Piece h[5] = {vis ? name : lit("A presence"), lit(" has set the topic to: "), none, none, none};
        here_len = compose(here_t, kSetHereRow, h, in, len, true, lane, a.violations);
        lines = true;
    } else if (outcome == kSetAfk || outcome == kSetAfkLocked) {       // c:7426-7429, 7437-7440, 7448-7453
        if (mesg_len > 0) {
            const Piece p[5] = {lit("AFK message set.\n"), none, none, none, none};
            reply2_len = compose(reply2_t, kSetReply2Row, p, nullptr, 0, false, lane, a.violations);
            if (reply2_len < 0) reply_len = -1;
        } else {                            // the message kept from before
            const uint8_t* m = a.afk + (size_t)slot * kAfkRec;
            mesg = m;
            mesg_len = m[kAfkMesgLen] < kAfkMesgLen ? m[kAfkMesgLen] : kAfkMesgLen;
        }
        if (vis) {
            const Piece h[5] = {name, mesg_len > 0 ? lit(" goes AFK: ") : lit(" goes AFK...\n"), none, none, none};
            here_len = compose(here_t, kSetHereRow, h, mesg, mesg_len, mesg_len > 0, lane, a.violations);
            lines = true;
        }
    }
    if ((outcome != kSetColourTest && reply_len < 0) || (lines && here_len < 0)) here_len = reply_len = reply2_len = -1;   // a violation: the call fails
    if (lane == 0) {
        a.clen[k] = here_len;
        a.clen[n + k] = reply_len;
        a.clen[2 * n + k] = reply2_len;
        a.outcome[k] = (int8_t)outcome;
        a.rm[k] = here;                     // write_room_except(user->room, text, user)
        a.sender[k] = slot;
        a.com_num[k] = com;
    }
}

static_assert(kSetHereMax == 96 && kSetReplyMax == 83 && kSetReply2Max == 17 && kSetHereMax <= kSetHereRow && kSetReplyMax <= kSetReplyRow &&
              kSetReply2Max <= kSetReply2Row, "roster_set: the longest texts fit their slots");
static_assert(sizeof(" has set the topic to: ") - 1 == 23 && sizeof("The current topic is: ") - 1 == 22 && sizeof("AFK message set.\n") - 1 == 17 &&
              sizeof("You are now AFK with the session locked, enter your password to unlock it.\n") - 1 <= kSetReplyMax &&
              sizeof("Your current out phrase is: ") - 1 + kPhraseLen + 1 <= kSetReplyMax &&
              sizeof("Your current description is: ") - 1 + kUserDescLen + 1 <= kSetReplyMax && sizeof("Topic set to: ") - 1 + kTopicLen + 1 <= kSetReplyMax &&
              kNameLen + sizeof(" goes AFK: ") - 1 + kAfkMesgLen + 1 <= kSetHereMax &&
              sizeof("~FB~OLYou hear a melodic incantation chanted and  materialises!\n") - 1 + kNameLen <= kSetHereMax &&
              sizeof("~FB~OL recites a melodic incantation and disappears!\n") - 1 + kNameLen <= kSetHereMax &&
              kNameLen + sizeof(" is now ignoring everyone.\n") - 1 <= kSetHereMax, "roster_set: the texts are as long as counted");
static_assert(kSetRow % 4 == 0 && kSetHereRow % 4 == 0 && kSetReplyRow % 4 == 0 && kSetHereRow < kTextSize,
              "roster_set: the rows are whole words, and a text fits speak_plan's LDS text");
static_assert(sizeof("~FB~OLYou hear a melodic incantation chanted and ") - 1 + kNameLen <= 64 &&
              sizeof(" recites a melodic incantation and disappears!\n") - 1 <= 64 && kNameLen + sizeof(" has set the topic to: ") - 1 <= 64,
              "roster_set: the pieces of a compose() fit a wave");
static_assert(64 * kReadSlice >= kArrSize && kWordLen + 7 <= 64, "roster_set: the word masks cover the longest inpstr, a lane per byte of word[1]");

// nuts_roster_set_order's rule.  Keys: the actor, its room's rank, whether the event has a here line, whether it is a .topic.
// Three bitmaps of ranks and slots, fewer than 65,536 each: the actors, the rooms where ignall or colour changed, the rooms
// whose topic was set.
struct SetOrderArgs {
    const int32_t* slot;         // [k] the actors
    const int32_t* rid;          // [k] their rooms' ranks
    const uint8_t* com;          // [k]
    int k;
    int8_t* outcome;             // [k] becomes kSetDeferred for a deferred event
    int32_t* clen;               // [3k] whose three texts become void

    static constexpr int kKeys = 4, kTexts = kSetTexts, kDeferred = kSetDeferred, kMapWords = 3 * kOrderSlotWords;
    __device__ void load(int b, bool live, int (&key)[kKeys]) const
    {
        key[0] = live ? slot[b] : 0, key[1] = live ? rid[b] : 0, key[2] = live && clen[b] >= 0, key[3] = live && com[b] == kComTopic;
    }
    static __device__ bool hit(const int (&key)[kKeys], const uint32_t* slots)
    {
        return bit_of(slots, key[0]) || (key[2] && bit_of(slots + kOrderSlotWords, key[1])) ||
               (key[3] && bit_of(slots + 2 * kOrderSlotWords, key[1]));
    }
    static __device__ void touch(const int (&key)[kKeys], int outcome, uint32_t* slots)
    {
        if (outcome > kSetIgntellOff) return;       // only an effective event touches anything
        set_bit(slots, key[0]);
        if (outcome == kSetIgnallOn || outcome == kSetIgnallOff || outcome == kSetColourOn || outcome == kSetColourOff)
            set_bit(slots + kOrderSlotWords, key[1]);
        if (outcome == kSetTopicSet) set_bit(slots + 2 * kOrderSlotWords, key[1]);
    }
    __device__ void also_void(int) const {}
};

}  // namespace

// Stable, unmangled kernel names (they are what rocprofv3 reports).
extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_measure_batch(Args a) { measure<false>(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_measure_broadcast(Args a) { measure<true>(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_emit_batch(Args a) { emit<false>(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_emit_broadcast(Args a) { emit<true>(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_measure_many(ManyArgs a) { measure_many(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_fanout_emit_many(ManyArgs a) { emit_many(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_measure(RosterArgs a) { roster_measure(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_emit(RosterArgs a) { roster_emit(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_plan(PlanArgs a) { roster_plan(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_record(RecordArgs a) { roster_record<kRevLines>(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_review(ReviewArgs a) { roster_review<kRevLines>(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_speak(SpeakArgs a) { roster_speak(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_speak_plan(SpeakPlanArgs a) { roster_speak_plan(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_parse(ParseArgs a) { roster_parse(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_tell(TellArgs a) { roster_tell(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_record_tell(RecordArgs a) { roster_record<kTellLines>(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_revtell(ReviewArgs a) { roster_review<kTellLines>(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_look(LookArgs a) { roster_look(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_relay(RelayArgs a) { roster_relay(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_who(WhoArgs a) { roster_who(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_who_shown(WhoArgs a) { roster_who_shown(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_rooms_count(RoomsArgs a) { roster_rooms_count(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_rooms_lines(RoomsArgs a) { roster_rooms_lines(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_go(GoArgs a) { roster_go(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_go_order(GoOrderArgs a) { order_events(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_access(AccessArgs a) { roster_access(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_access_order(AccessOrderArgs a) { order_events(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_clone(CloneArgs a) { roster_clone(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_clone_order(CloneOrderArgs a) { order_events(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_act(ActArgs a) { roster_act(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_act_order(ActOrderArgs a) { order_events(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_set(SetArgs a) { roster_set(a); }
extern "C" __global__ void __launch_bounds__(kBlock) nuts_roster_set_order(SetOrderArgs a) { order_events(a); }

// ------------------------------------------------------------------------------------------ host library

namespace {

// One device block, laid out afresh for every call (layout()), and the pinned host buffers the results land in;
// grown on demand and kept across calls (one process, one caller).
struct Buffers {
    uint8_t* d_block = nullptr;
    size_t cap_block = 0, cap_host_arena = 0, cap_host_writes = 0;
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
    g.ready = true;
    return 0;
}

// Carves the block at `base` into arrays, one 256-byte aligned slice per call; `at` is the bytes taken so far.  With
// base 0 the pointers are the arrays' offsets in the block.
struct Carver {
    uintptr_t base;
    size_t at = 0;
    template <typename T>
    void operator()(T*& p, size_t count)
    {
        p = reinterpret_cast<T*>(base + at);
        at += (count * sizeof(T) + 255) & ~(size_t)255;
    }
};

// A call's inputs are packed in pinned memory at h as they lie on the device: `at` names an array by its offset in the
// block, as a layout at base 0 gives it.
struct Put {
    uint8_t* h;
    void operator()(const void* at, const void* src, size_t bytes) const
    {
        if (bytes) memcpy(h + (uintptr_t)at, src, bytes);
    }
};

// And its first results land in pinned memory at h, from the block's byte `first` on: where the array at `at` is.
struct Res {
    const uint8_t* h;
    size_t first;
    const uint8_t* operator()(const void* at) const { return h + ((uintptr_t)at - first); }
};

// Point every device array of a (a.n items, the arena and chunk capacities already set) and *scan into the block at
// base; returns the bytes they span.  layout(0, ...) sizes the block.
size_t layout(uintptr_t base, size_t text_bytes, size_t scan_bytes, Args& a, uint8_t** scan)
{
    Carver take{base};
    const size_t n = (size_t)a.n;
    take(a.text, text_bytes);
    take(a.text_off, n);
    take(a.text_len, n);
    take(a.rec, n);
    take(a.admitted, n);
    take(a.nbytes, n + 1);
    take(a.nwrites, n + 1);
    take(a.out_off, n + 1);
    take(a.w_off, n + 1);
    take(a.violations, 1);
    take(a.arena, (size_t)a.arena_cap);
    take(a.wsz, (size_t)a.wsz_cap);
    take(*scan, scan_bytes);
    return take.at;
}

double now_ns()
{
    return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}

// nd_fanout_many's pinned host buffers (it shares g.d_block and the result buffers with nd_fanout): the inputs packed
// exactly as they lie at the start of the device block, and the first results as they lie after them.
struct ManyHost {
    uint8_t* stage = nullptr;
    uint8_t* res = nullptr;
    size_t cap_stage = 0, cap_res = 0;
};
ManyHost gm;

// The two clocks of a call whose kernels ran between g.ev0 and g.ev1 and whose host work took t0 .. t1.
template <typename T>   // nd_timing or nd_roster_timing
int fill_timing(T* timing, double t0, double t1)
{
    float ms = 0.f;
    ND_CHECK(hipEventElapsedTime(&ms, g.ev0, g.ev1));
    if (timing) {
        timing->kernels_us = (double)ms * 1e3;
        timing->end_to_end_us = (t1 - t0) * 1e-3;
    }
    return 0;
}

// And a roster call's copy volume.
template <typename T>   // nd_roster_timing
int fill_timing(T* timing, double t0, double t1, size_t h2d_bytes, size_t d2h_bytes)
{
    if (fill_timing(timing, t0, t1)) return -1;
    if (timing) {
        timing->h2d_bytes = (int64_t)h2d_bytes;
        timing->d2h_bytes = (int64_t)d2h_bytes;
    }
    return 0;
}

// The kernels count what broke the transducer's hard bounds; any such `what` ("item", "variant") fails the call.
int check_bounds(int violations, const char* what)
{
    if (!violations) return 0;
    snprintf(g_err, sizeof(g_err), "%d %s(s) exceeded the hard output bounds (6*len+4 bytes, %d writes)", violations,
             what, kMaxWrites);
    return -1;
}

// The kernels end here: res_bytes of results from byte res_at of the device block d into gm.res, and a synchronise.
int fetch_results(const uint8_t* d, size_t res_at, size_t res_bytes)
{
    ND_CHECK(hipEventRecord(g.ev1, g.stream));
    ND_CHECK(hipMemcpyAsync(gm.res, d + res_at, res_bytes, hipMemcpyDeviceToHost, g.stream));
    ND_CHECK(hipStreamSynchronize(g.stream));
    return 0;
}

// As layout(), for ManyArgs (a.k, a.m and the capacities set).  The inputs come first and end with violations, so
// one upload fills them all and zeroes violations; violations, admitted, out_off and w_off follow each other, so one
// download fetches them.  layout_many(0, ...) gives every array's offset in the block.
size_t layout_many(uintptr_t base, size_t text_bytes, size_t scan_bytes, ManyArgs& a, uint8_t** scan)
{
    Carver take{base};
    const size_t k = (size_t)a.k, m = (size_t)a.m;
    take(a.text, text_bytes);
    take(a.text_off, k);
    take(a.text_len, k);
    take(a.flags, k);
    take(a.com_num, k);
    take(a.item_off, k + 1);
    take(a.tile_off, k + 1);
    take(a.rec, m);
    take(a.violations, 1);
    take(a.admitted, m);
    take(a.out_off, m + 1);
    take(a.w_off, m + 1);
    take(a.nbytes, m + 1);
    take(a.nwrites, m + 1);
    take(a.arena, (size_t)a.arena_cap);
    take(a.wsz, (size_t)a.wsz_cap);
    take(*scan, scan_bytes);
    return take.at;
}

// A roster's own device allocation and its pinned mirror, laid out alike by layout_roster(): the table (room, slot),
// then the call's inputs ending with violations, then admitted, out_off and w_off.  One upload fills the inputs, and
// the table with them when it changed; one download fetches violations .. w_off.  Both grow on demand; the mirror
// keeps the table across growth, and a new device allocation is filled from it.
constexpr int kMaxRosters = 64;
constexpr int kMaxCapacity = 65536;

// The tables a roster keeps on the device between calls, each in an allocation of its own that the first call to give
// the table makes and that never moves.  A caller passes one only when it changed: see pass_kept().
enum KeptId { kKeptSpeech, kKeptAfk, kKeptRooms, kKeptUdesc, kKeptWho, kKeptClones, kKeptNames, kKeptGo, kKeptCount };
struct KeptTable {
    const char* what;            // for error messages
    uint8_t* d = nullptr;
};

struct Roster {
    bool live = false;
    bool resident = false;       // the device allocation holds the mirror's table
    int capacity = 0;
    int64_t rooms = 0;           // slots with a room: only they can be admitted
    uint8_t* d = nullptr;
    uint8_t* mirror = nullptr;
    size_t cap_d = 0, cap_mirror = 0;
    int review_rooms = 0;        // rooms 0 .. review_rooms - 1 own a review ring
    uint8_t* rings = nullptr;    // the rings, then the cursors: an allocation of its own, made on first use, never moved
    bool revtell = false;        // every slot owns a revtell ring
    uint8_t* tell_rings = nullptr;   // the revtell rings, then their cursors: as rings
    int look_rooms = 0;          // rooms 0 .. look_rooms - 1 own a room record
    int clones = 0;              // clone records 0 .. clones - 1
    KeptTable kept[kKeptCount] = {{"speaker table"}, {"AFK messages"}, {"room table"}, {"user descriptions"},
                                  {"who table"}, {"clone records"}, {"room names"}, {"go table"}};   // by KeptId; kept_bytes() has their sizes
};
Roster g_rosters[kMaxRosters];

// A roster's clone records as they lie on the device, in the upload and in the kept allocation alike: three arrays in a
// 256-byte slice each, so the bytes they span are whole words.
void take_clones(Carver& take, int clones, const int32_t*& owner, const int32_t*& room, const uint8_t*& hear)
{
    take(owner, (size_t)clones);
    take(room, (size_t)clones);
    take(hear, (size_t)clones);
}

// The size of kept table `id` of a roster with these dimensions, a whole number of words.
size_t kept_bytes(int id, int capacity, int look_rooms, int clones)
{
    switch (id) {
    case kKeptSpeech: return (size_t)capacity * kSpeechRec;                // the speakers' state, 16 bytes per slot
    case kKeptAfk: return (size_t)capacity * kAfkRec;                      // the AFK messages, 64 bytes per slot
    case kKeptRooms: return (size_t)look_rooms * kRoomRow;                 // the look rooms' records, then their descriptions
    case kKeptUdesc: return (size_t)capacity * kUserDescRow;               // the users' descriptions, 32 bytes per slot
    case kKeptWho: return (size_t)capacity * kWhoRec;                      // last_login and away, 8 bytes per slot
    case kKeptNames: return (size_t)look_rooms * kRelayNameRow;            // the look rooms' names, 24 bytes per room
    case kKeptGo: return (size_t)capacity * kGoRec;                        // the phrases and the invite, 88 bytes per slot
    default: {                                                             // the clones' owners, rooms and hear bytes
        Carver sized{0};
        const int32_t *owner, *room;
        const uint8_t* hear;
        take_clones(sized, clones, owner, room, hear);
        return sized.at;
    }
    }
}
size_t kept_bytes(const Roster& r, int id) { return kept_bytes(id, r.capacity, r.look_rooms, r.clones); }

// Room for a kept table's upload in a layout; t.fresh is where it lies.
void take_kept(Carver& take, Kept& t, int id, int capacity, int look_rooms = 0, int clones = 0)
{
    take(t.fresh, kept_bytes(id, capacity, look_rooms, clones) / sizeof(uint32_t));
}

// One of a roster's two sets of rings: the rooms' review rings (15 lines each), or the slots' revtell rings (5 lines).
struct RingSet {
    uint8_t** p;                 // r.rings or r.tell_rings
    int count, lines;
    size_t revline_at() const { return ((size_t)count * lines * kRevSlot + 255) & ~(size_t)255; }   // where the cursors start
    size_t bytes() const { return revline_at() + (size_t)count * sizeof(int32_t); }                // the allocation's size
    int32_t* revline() const { return reinterpret_cast<int32_t*>(*p + revline_at()); }
};
RingSet rings_of(Roster& r, bool tell)
{
    return tell ? RingSet{&r.tell_rings, r.revtell ? r.capacity : 0, kTellLines} : RingSet{&r.rings, r.review_rooms, kRevLines};
}

// The head of every layout of a roster's allocation: the table.  Its place depends on the capacity alone, so the table
// stays resident across every kind of call, and a call that does not read it need not upload it.
void take_table(Carver& take, int capacity, const int32_t*& room, const uint8_t*& slot)
{
    take(room, (size_t)capacity);
    take(slot, (size_t)capacity);
}

// Behind its tables every event call's layout has the events as they are uploaded: the inpstr, their offsets and lengths,
// the slots, the commands when the call has them (com; nullptr: nd_roster_go's events have none) and the word counts.
void take_events(Carver& take, EventArgs& s, size_t text_bytes, const uint8_t** com)
{
    const size_t k = (size_t)s.k;
    take(s.text, text_bytes);
    take(s.text_off, k);
    take(s.text_len, k);
    take(s.slot, k);
    if (com) take(*com, k);
    take(s.words, k);
}

// And behind its own results what nuts_roster_speak_plan makes of the call's t texts over ctext_bytes, next to each other
// for the one download: their lengths, the variants' sizes and writes, the admit bitmaps of the `lines` room lines, the
// composed texts and the variants.  p reads the table, the texts and violations where the compose kernel has them.
void take_event_texts(Carver& take, EventArgs& s, SpeakPlanArgs& p, size_t t, size_t lines, size_t ctext_bytes)
{
    take(s.clen, t);
    take(p.vn, 2 * t);
    take(p.vw, 2 * t);
    take(p.vwsz, 2 * t * kMaxWrites);
    take(p.bits, lines * (size_t)p.words);
    take(s.ctext, ctext_bytes);
    take(p.var, (size_t)var_at((int64_t)ctext_bytes, (int64_t)t));
    p.room = s.room;
    p.slot = s.slotf;
    p.text = s.ctext;
    p.text_off = s.ctext_off;
    p.text_len = s.clen;
    p.violations = s.violations;
}

size_t layout_roster(uintptr_t base, size_t text_bytes, RosterArgs& a)
{
    Carver take{base};
    const size_t k = (size_t)a.k, m = k * (size_t)a.capacity;
    take_table(take, a.capacity, a.room, a.slot);
    take(a.text, text_bytes);
    take(a.text_off, k);
    take(a.text_len, k);
    take(a.rm, k);
    take(a.sender, k);
    take(a.flags, k);
    take(a.com_num, k);
    take(a.violations, 1);
    take(a.admitted, m);
    take(a.out_off, m + 1);
    take(a.w_off, m + 1);
    return take.at;
}

// The call's work arrays in the shared device block: the variants, the arena, the chunk sizes and the scans' scratch.
size_t layout_roster_work(uintptr_t base, size_t var_bytes, size_t scan_bytes, RosterArgs& a, uint8_t** scan)
{
    Carver take{base};
    const size_t k = (size_t)a.k;
    take(a.var, var_bytes);
    take(a.vn, 2 * k);
    take(a.vw, 2 * k);
    take(a.vwsz, 2 * k * kMaxWrites);
    take(a.arena, (size_t)a.arena_cap);
    take(a.wsz, (size_t)a.wsz_cap);
    take(*scan, scan_bytes);
    return take.at;
}

// nd_roster_plan's layout of a roster's allocation: the table and the call's inputs as layout_roster() places them,
// then the results, violations .. var, next to each other: one download fetches them all at their bound size.
size_t layout_plan(uintptr_t base, size_t text_bytes, size_t var_bytes, PlanArgs& a, size_t clear_bytes,
                   const uint8_t** clear)
{
    Carver take{base};
    const size_t k = (size_t)a.k;
    take_table(take, a.capacity, a.room, a.slot);
    take(a.text, text_bytes);
    take(a.text_off, k);
    take(a.text_len, k);
    take(a.rm, k);
    take(a.sender, k);
    take(a.flags, k);
    take(a.com_num, k);
    take(*clear, clear_bytes);      // a recording call's pending clears; no bytes, and no change of layout, without them
    take(a.violations, 1);
    take(a.vn, 2 * k);
    take(a.vw, 2 * k);
    take(a.vwsz, 2 * k * kMaxWrites);
    take(a.bits, k * (size_t)a.words);
    take(a.var, var_bytes);
    return take.at;
}

// nd_roster_review's layout of a roster's allocation: the table, which the call neither reads nor uploads, the call's
// inputs ending with violations, then the results next to each other.
size_t layout_review(uintptr_t base, int capacity, size_t clear_bytes, ReviewArgs& a, int lines = kRevLines)
{
    Carver take{base};
    const size_t q = (size_t)a.q;
    const int32_t* room;
    const uint8_t* slot;
    take_table(take, capacity, room, slot);
    take(a.rooms, q);
    take(a.clear, clear_bytes);
    take(a.violations, 1);
    take(a.line_count, q);
    take(a.sequential, q);
    take(a.vn, 2 * q);
    take(a.vw, 2 * q);
    take(a.vwsz, 2 * q * lines * kRevLineWrites);
    take(a.lines, q * lines * kRevSlot);
    take(a.var, 2 * q * rev_var_stride(lines));
    return take.at;
}

// nd_roster_speak's layout of a roster's allocation: the table, then the upload of the
// speaker table (which the kept one, r.kept[], is filled from), the call's inputs ending with violations, the results
// next to each other, and last what only the kernels pass to each other.  One upload starts at the speaker table if it
// was given, else at the inputs; a table the device does not hold goes in front of it (upload()).
// nd_roster_input's (q given) differs in what describes an event: the upload carries the reads' offsets and lengths
// where the inpstr's were, no commands and no word counts; nuts_roster_parse writes those, and they lie among the
// results with what else it found.
size_t layout_speak(uintptr_t base, size_t text_bytes, size_t clear_bytes, SpeakArgs& s, SpeakPlanArgs& p,
                    const uint8_t** clear, ParseArgs* q = nullptr)
{
    Carver take{base};
    const size_t k = (size_t)s.k;
    const size_t ctext_bytes = (size_t)ctext_at(2 * (int64_t)text_bytes, 2 * (int64_t)k);
    take_table(take, s.capacity, s.room, p.slot);
    take_kept(take, s.kept[0], kKeptSpeech, s.capacity);
    take(s.text, text_bytes);
    if (q) {
        take(q->read_off, k);
        take(q->read_len, k);
    } else {
        take(s.text_off, k);
        take(s.text_len, k);
    }
    take(s.slot, k);
    if (!q) {
        take(s.com, k);
        take(s.words, k);
    }
    take(s.ctext_off, 2 * k);
    take(*clear, clear_bytes);
    take(s.violations, 1);
    take(s.outcome, k);
    take(s.clen, 2 * k);
    if (q) {
        take(q->kind, k);
        take(q->com, k);
        take(q->words, k);
        take(q->line_len, k);
        take(q->text_off, k);
        take(q->text_len, k);
    }
    take(p.vn, 4 * k);
    take(p.vw, 4 * k);
    take(p.vwsz, 4 * k * kMaxWrites);
    take(p.bits, k * (size_t)p.words);
    take(s.ctext, ctext_bytes);
    take(p.var, (size_t)var_at((int64_t)ctext_bytes, 2 * (int64_t)k));
    take(s.rm, k);
    take(s.sender, k);
    take(s.com_num, k);
    take(s.flags, k);
    if (q) {
        take(q->preset, k);
        q->data = s.text;
        q->slot = s.slot;
        s.text_off = q->text_off;
        s.text_len = q->text_len;
        s.com = reinterpret_cast<const uint8_t*>(q->com);
        s.words = q->words;
        s.preset = q->preset;
    }
    p.room = s.room;
    p.text = s.ctext;
    p.text_off = s.ctext_off;
    p.text_len = s.clen;
    p.rm = s.rm;
    p.sender = s.sender;
    p.com_num = s.com_num;
    p.violations = s.violations;
    return take.at;
}

// nd_roster_tell's layout of a roster's allocation, after layout_speak's pattern: the table, the uploads of the speaker
// table and of the AFK messages (which the kept ones of r.kept[] are filled from), the call's inputs ending with
// violations, the results next to each other, and last what only the kernels pass to each other.  One upload starts at
// the first of the two tables behind the table that was given, or at the inputs (upload()).
size_t layout_tell(uintptr_t base, size_t text_bytes, size_t clear_bytes, TellArgs& s, SpeakPlanArgs& p, const uint8_t** clear)
{
    Carver take{base};
    const size_t k = (size_t)s.k;
    const size_t ctext_bytes = (size_t)ptext_at(2 * (int64_t)text_bytes, 2 * (int64_t)k);
    take_table(take, s.capacity, s.room, s.slotf);
    take_kept(take, s.kept[0], kKeptSpeech, s.capacity);
    take_kept(take, s.kept[1], kKeptAfk, s.capacity);
    take(s.text, text_bytes);
    take(s.text_off, k);
    take(s.text_len, k);
    take(s.slot, k);
    take(s.com, k);
    take(s.words, k);
    take(s.ctext_off, 2 * k);
    take(*clear, clear_bytes);
    take(s.violations, 1);
    take(s.outcome, k);
    take(s.target, k);
    take(s.clen, 2 * k);
    take(p.vn, 4 * k);
    take(p.vw, 4 * k);
    take(p.vwsz, 4 * k * kMaxWrites);
    take(s.ctext, ctext_bytes);
    take(p.var, (size_t)var_at((int64_t)ctext_bytes, 2 * (int64_t)k));
    take(s.ring, k);
    take(s.flags, k);
    p.room = s.room;
    p.slot = s.slotf;
    p.text = s.ctext;
    p.text_off = s.ctext_off;
    p.text_len = s.clen;
    p.violations = s.violations;
    return take.at;
}

// nd_roster_look's layout of a roster's allocation, after layout_tell's pattern: the table, the uploads of the speaker
// table, of the room table and of the users' descriptions (which the kept ones are filled from), the call's inputs ending
// with violations, then the results next to each other: the counts, the texts and their variants, the lookers' members.
size_t layout_look(uintptr_t base, size_t members, size_t nl, LookArgs& s, SpeakPlanArgs& p)
{
    Carver take{base};
    const size_t k = (size_t)s.k, nr = (size_t)s.nr, t = kLookTexts * nr + kLookFixed + nl;
    const size_t ctext_bytes = (size_t)look_ctext_bytes((int64_t)nr, (int64_t)nl);
    take_table(take, s.capacity, s.room, p.slot);
    take_kept(take, s.kept[0], kKeptSpeech, s.capacity);
    take_kept(take, s.kept[1], kKeptRooms, s.capacity, s.look_rooms);
    take_kept(take, s.kept[2], kKeptUdesc, s.capacity);
    take(s.slot, k);
    take(s.lroom, k);
    take(s.rms, nr);
    take(s.line_off, nr + 1);
    take(s.m_off, k + 1);
    take(s.ctext_off, t);
    take(s.violations, 1);
    take(s.nmem, k);
    take(s.nline, nr);
    take(s.clen, t);
    take(p.vn, 2 * t);
    take(p.vw, 2 * t);
    take(p.vwsz, 2 * t * kMaxWrites);
    take(s.members, members);
    take(s.mline, members);
    take(s.line_slot, nl);
    take(s.ctext, ctext_bytes);
    take(p.var, (size_t)var_at((int64_t)ctext_bytes, (int64_t)t));
    p.room = s.room;
    p.text = s.ctext;
    p.text_off = s.ctext_off;
    p.text_len = s.clen;
    p.violations = s.violations;
    return take.at;
}

// nd_roster_who's layout of a roster's allocation, after layout_look's pattern: the table, the uploads of the speaker table,
// of the room table, of the users' descriptions and of the who table (which the kept ones are filled from; the who table
// last, so that an upload of it alone carries no other), the call's inputs -- the lookers and the date -- ending with
// violations, then the results next to each other, and last the texts' offsets, which only the kernels pass to each other.
size_t layout_who(uintptr_t base, WhoArgs& s, SpeakPlanArgs& p)
{
    Carver take{base};
    const size_t k = (size_t)s.k, nl = (size_t)s.nl, t = kWhoFixed + nl;
    const size_t ctext_bytes = (size_t)who_ctext_bytes((int64_t)nl);
    take_table(take, s.capacity, s.room, s.slotf);
    take_kept(take, s.kept[0], kKeptSpeech, s.capacity);
    take_kept(take, s.kept[1], kKeptRooms, s.capacity, s.look_rooms);
    take_kept(take, s.kept[2], kKeptUdesc, s.capacity);
    take_kept(take, s.kept[3], kKeptWho, s.capacity);
    take(s.slot, k);
    take(s.date, (size_t)kWhoDateLen + 1);
    take(s.violations, 1);
    take(s.clen, t);
    take(s.line_slot, nl);
    take(s.shown, k * (size_t)s.words);
    take(p.vn, 2 * t);
    take(p.vw, 2 * t);
    take(p.vwsz, 2 * t * kMaxWrites);
    take(s.ctext, ctext_bytes);
    take(p.var, (size_t)var_at((int64_t)ctext_bytes, (int64_t)t));
    take(s.ctext_off, t);
    p.room = s.room;
    p.slot = s.slotf;
    p.text = s.ctext;
    p.text_off = s.ctext_off;
    p.text_len = s.clen;
    p.violations = s.violations;
    return take.at;
}

// nd_roster_rooms' layout of a roster's allocation, after layout_who's pattern: the table, the uploads of the speaker table
// and of the room table (which the kept ones are filled from), the call's input -- the lookers -- ending with violations,
// then the results next to each other, and last what only the kernels pass to each other: the texts' offsets and the
// counters, which the host zeroes on the stream and no upload touches.
size_t layout_rooms(uintptr_t base, RoomsArgs& s, SpeakPlanArgs& p)
{
    Carver take{base};
    const size_t k = (size_t)s.k, nr = (size_t)s.look_rooms, t = kRoomsFixed + 2 * nr;
    const size_t ctext_bytes = (size_t)rooms_ctext_bytes((int64_t)nr);
    take_table(take, s.capacity, s.room, s.slotf);
    take_kept(take, s.kept[0], kKeptSpeech, s.capacity);
    take_kept(take, s.kept[1], kKeptRooms, s.capacity, s.look_rooms);
    take(s.slot, k);
    take(s.violations, 1);
    take(s.clen, t);
    take(s.counts, nr);
    take(p.vn, 2 * t);
    take(p.vw, 2 * t);
    take(p.vwsz, 2 * t * kMaxWrites);
    take(s.ctext, ctext_bytes);
    take(p.var, (size_t)var_at((int64_t)ctext_bytes, (int64_t)t));
    take(s.ctext_off, t);
    take(s.counters, nr);
    p.room = s.room;
    p.slot = s.slotf;
    p.text = s.ctext;
    p.text_off = s.ctext_off;
    p.text_len = s.clen;
    p.violations = s.violations;
    return take.at;
}

// nd_roster_go's layout of a roster's allocation, after layout_tell's pattern: the table, the uploads of the speaker table,
// of the clone records, of the room table and of the go table (which the kept ones are filled from; the two that a go call's
// own aftermath changes last), the call's inputs ending with violations, the results next to each other, and last what only
// the kernels pass to each other.  p plans 3k room lines and k replies.
size_t layout_go(uintptr_t base, size_t text_bytes, GoArgs& s, SpeakPlanArgs& p)
{
    Carver take{base};
    const size_t k = (size_t)s.k, t = kGoTexts * k;
    take_table(take, s.capacity, s.room, s.slotf);
    take_kept(take, s.kept[0], kKeptSpeech, s.capacity);
    take_kept(take, s.kept[1], kKeptClones, s.capacity, s.look_rooms, s.clones);
    take_kept(take, s.kept[2], kKeptRooms, s.capacity, s.look_rooms);
    take_kept(take, s.kept[3], kKeptGo, s.capacity);
    take_events(take, s, text_bytes, nullptr);
    take(s.ctext_off, t);
    take(s.violations, 1);
    take(s.outcome, k);
    take(s.target, k);
    take(s.old_room, k);
    take(s.returned, k);
    take_event_texts(take, s, p, t, 3 * k, (size_t)kGoRow * k);
    take(s.rm, 3 * k);
    take(s.sender, 3 * k);
    take(s.com_num, 3 * k);
    p.rm = s.rm;
    p.sender = s.sender;
    p.com_num = s.com_num;
    return take.at;
}

// nd_roster_access's layout of a roster's allocation: layout_go's, with the events' commands, the two targets, and p planning
// 2k room lines and 2k single-recipient texts.  Of the uploads the room table lies last and the go table before it: the
// call's own aftermath changes an access more often than an invitation, and an upload runs from the first table given to
// the end of the inputs.
size_t layout_access(uintptr_t base, size_t text_bytes, AccessArgs& s, SpeakPlanArgs& p)
{
    Carver take{base};
    const size_t k = (size_t)s.k, t = kAccTexts * k;
    take_table(take, s.capacity, s.room, s.slotf);
    take_kept(take, s.kept[0], kKeptSpeech, s.capacity);
    take_kept(take, s.kept[1], kKeptClones, s.capacity, s.look_rooms, s.clones);
    take_kept(take, s.kept[2], kKeptGo, s.capacity);
    take_kept(take, s.kept[3], kKeptRooms, s.capacity, s.look_rooms);     // last: a set access alone uploads nothing else
    take_events(take, s, text_bytes, &s.com);
    take(s.ctext_off, t);
    take(s.violations, 1);
    take(s.outcome, k);
    take(s.target_room, k);
    take(s.target_slot, k);
    take_event_texts(take, s, p, t, 2 * k, (size_t)kAccRow * k);
    take(s.rm, 2 * k);
    take(s.sender, 2 * k);
    take(s.com_num, 2 * k);
    p.rm = s.rm;
    p.sender = s.sender;
    p.com_num = s.com_num;
    return take.at;
}

// nd_roster_clone's layout of a roster's allocation: layout_access's, with the record, the reset and the record flags among
// the results, the pending clears among the inputs, and p planning 4k room lines and 2k single-recipient texts.  Of the
// uploads the clone records lie last: the call's own aftermath changes them, and an upload runs from the first table given
// to the end of the inputs.
size_t layout_clone(uintptr_t base, size_t text_bytes, size_t clear_bytes, CloneArgs& s, SpeakPlanArgs& p, const uint8_t** clear)
{
    Carver take{base};
    const size_t k = (size_t)s.k, t = kCloneTexts * k;
    take_table(take, s.capacity, s.room, s.slotf);
    take_kept(take, s.kept[0], kKeptSpeech, s.capacity);
    take_kept(take, s.kept[1], kKeptGo, s.capacity);
    take_kept(take, s.kept[2], kKeptRooms, s.capacity, s.look_rooms);
    take_kept(take, s.kept[3], kKeptClones, s.capacity, s.look_rooms, s.clones);   // last: a created clone alone uploads nothing else
    take_events(take, s, text_bytes, &s.com);
    take(s.ctext_off, t);
    take(*clear, clear_bytes);
    take(s.violations, 1);
    take(s.outcome, k);
    take(s.reset, k);
    take(s.found, 3 * k);
    take_event_texts(take, s, p, t, kCloneLines * k, (size_t)clone_text_bytes((int64_t)k, (int64_t)text_bytes));
    take(s.line, 3 * kCloneLines * k);
    take(s.flags, k);
    p.rm = s.line;
    p.sender = s.line + kCloneLines * k;
    p.com_num = s.line + 2 * kCloneLines * k;
    return take.at;
}

// nd_roster_act's layout of a roster's allocation: layout_clone's without the said lines and the clears, with the slot found,
// the room resolved and the room left in one array, and p planning 4k room lines and 2k single-recipient texts.  Of the
// uploads the speaker table lies last, behind the go table and the room table: a muzzle set, the call's own aftermath, then
// travels alone, and an upload runs from the first table given to the end of the inputs.
size_t layout_act(uintptr_t base, size_t text_bytes, ActArgs& s, SpeakPlanArgs& p)
{
    Carver take{base};
    const size_t k = (size_t)s.k, t = kActTexts * k;
    take_table(take, s.capacity, s.room, s.slotf);
    take_kept(take, s.kept[0], kKeptClones, s.capacity, s.look_rooms, s.clones);
    take_kept(take, s.kept[1], kKeptRooms, s.capacity, s.look_rooms);
    take_kept(take, s.kept[2], kKeptGo, s.capacity);
    take_kept(take, s.kept[3], kKeptSpeech, s.capacity);                   // last: a muzzle alone uploads nothing else
    take_events(take, s, text_bytes, &s.com);
    take(s.ctext_off, t);
    take(s.violations, 1);
    take(s.outcome, k);
    take(s.returned, k);
    take(s.found, 3 * k);
    take_event_texts(take, s, p, t, kActLines * k, (size_t)kActRow * k);
    take(s.line, 3 * kActLines * k);
    p.rm = s.line;
    p.sender = s.line + kActLines * k;
    p.com_num = s.line + 2 * kActLines * k;
    return take.at;
}

// nd_roster_set's layout of a roster's allocation, after layout_access's: the table, the uploads of the five tables -- the
// room table first, which only a .topic reads, then the slots' tables from the widest row to the narrowest, since an upload
// runs from the first table given to the end of the inputs: a changed speaker table, 16 bytes a slot, travels alone --, the
// events with their rooms' ranks, the results next to each other, p planning k room lines and 2k single-recipient texts, and
// last what only the kernels pass on.
size_t layout_set(uintptr_t base, size_t text_bytes, int look_rooms, SetArgs& s, SpeakPlanArgs& p)
{
    Carver take{base};
    const size_t k = (size_t)s.k, t = kSetTexts * k;
    take_table(take, s.capacity, s.room, s.slotf);
    take_kept(take, s.kept[0], kKeptRooms, s.capacity, look_rooms);
    take_kept(take, s.kept[1], kKeptGo, s.capacity);
    take_kept(take, s.kept[2], kKeptAfk, s.capacity);
    take_kept(take, s.kept[3], kKeptUdesc, s.capacity);
    take_kept(take, s.kept[4], kKeptSpeech, s.capacity);
    take_events(take, s, text_bytes, &s.com);
    take(s.rid, k);
    take(s.ctext_off, t);
    take(s.violations, 1);
    take(s.outcome, k);
    take_event_texts(take, s, p, t, k, (size_t)kSetRow * k);
    take(s.rm, k);
    take(s.sender, k);
    take(s.com_num, k);
    p.rm = s.rm;
    p.sender = s.sender;
    p.com_num = s.com_num;
    return take.at;
}

// nd_roster_relay's layout of a roster's allocation, after layout_plan's pattern: the table, the uploads of the rooms' names
// and of the clone records (which the kept ones are filled from), nd_roster_plan's inputs with the clone senders and the
// relay texts' offsets, ending with violations, then the plan's results and the relay's (p plans the relay texts) next to
// each other: one download.
// The clone records lie last of the tables, so an upload of theirs alone carries nothing else.
size_t layout_relay(uintptr_t base, size_t text_bytes, size_t clear_bytes, PlanArgs& a, RelayArgs& q, SpeakPlanArgs& p, const uint8_t** clear)
{
    Carver take{base};
    const size_t k = (size_t)a.k;
    const size_t rtext_bytes = text_bytes + (size_t)kRelaySlack * k;
    take_table(take, a.capacity, a.room, a.slot);
    take_kept(take, q.kept[0], kKeptNames, q.capacity, q.look_rooms);
    take_kept(take, q.kept[1], kKeptClones, q.capacity, q.look_rooms, q.clones);   // whole slices, as take_clones gives them
    take(a.text, text_bytes);
    take(a.text_off, k);
    take(a.text_len, k);
    take(a.rm, k);
    take(a.sender, k);
    take(a.flags, k);
    take(a.com_num, k);
    take(q.csender, k);
    take(q.rtext_off, k);
    take(*clear, clear_bytes);
    take(a.violations, 1);
    take(a.vn, 2 * k);
    take(a.vw, 2 * k);
    take(a.vwsz, 2 * k * kMaxWrites);
    take(a.bits, k * (size_t)a.words);
    take(a.var, (size_t)var_at((int64_t)text_bytes, (int64_t)k));
    take(q.rbits, k * (size_t)q.cwords);
    take(q.rlen, k);
    take(p.vn, 2 * k);
    take(p.vw, 2 * k);
    take(p.vwsz, 2 * k * kMaxWrites);
    take(q.rtext, rtext_bytes);
    take(p.var, (size_t)var_at((int64_t)rtext_bytes, (int64_t)k));
    q.slot = a.slot;
    q.text = a.text;
    q.text_off = a.text_off;
    q.text_len = a.text_len;
    q.rm = a.rm;
    q.violations = p.violations = a.violations;
    p.text = q.rtext;
    p.text_off = q.rtext_off;
    p.text_len = q.rlen;
    return take.at;
}

// The roster's rings (tell: its revtell rings), made and zeroed in the stream on first use.
int ensure_rings(Roster& r, hipStream_t st, bool tell = false)
{
    const RingSet s = rings_of(r, tell);
    if (*s.p) return 0;
    if (s.count < 1) {
        snprintf(g_err, sizeof(g_err), tell ? "the roster has no revtell rings" : "the roster has no review rings");
        return -1;
    }
    hipError_t e = hipMalloc((void**)s.p, s.bytes());
    if (e != hipSuccess) {
        *s.p = nullptr;
        return fail(tell ? "revtell rings" : "review rings", e);
    }
    ND_CHECK(hipMemsetAsync(*s.p, 0, s.bytes(), st));
    return 0;
}

// Grow r's pinned mirror to want bytes, keeping its first keep bytes (the table); a new mirror starts with every slot
// empty (no room, no flags).
int grow_mirror(Roster& r, size_t want, size_t keep)
{
    if (want <= r.cap_mirror) return 0;
    uint8_t* p = nullptr;
    hipError_t e = hipHostMalloc((void**)&p, want, hipHostMallocDefault);
    if (e != hipSuccess) return fail("pinned roster mirror", e);
    if (r.mirror) {
        memcpy(p, r.mirror, keep);
        (void)hipHostFree(r.mirror);
    } else {
        memset(p, 0, keep);
        memset(p, 0xff, (size_t)r.capacity * sizeof(int32_t));    // room -1
    }
    r.mirror = p;
    r.cap_mirror = want;
    return 0;
}

// The caller's new table into r's mirror, at the offsets a layout gave the table; the device allocation is stale then.
void new_table(Roster& r, const int32_t* room_at, const uint8_t* slot_at, const uint8_t* table)
{
    const int cap = r.capacity;
    memcpy(r.mirror + (uintptr_t)room_at, table, (size_t)cap * sizeof(int32_t));
    memcpy(r.mirror + (uintptr_t)slot_at, table + (size_t)cap * sizeof(int32_t), (size_t)cap);
    const int32_t* room = reinterpret_cast<const int32_t*>(r.mirror + (uintptr_t)room_at);
    r.rooms = std::count_if(room, room + cap, [](int32_t x) { return x >= 0; });
    r.resident = false;
}

// Grow r's device allocation to `need` bytes.  A new one does not hold the table: the next call that reads the table
// uploads it from the mirror.
int grow_roster(Roster& r, size_t need)
{
    const size_t cap_d = r.cap_d;
    if (grow_dev(&r.d, &r.cap_d, need, "roster device allocation")) return -1;
    if (r.cap_d != cap_d) r.resident = false;
    return 0;
}

// The upload of a call whose layout leaves room between the table and the inputs for tables the caller may pass: `first`
// is where the first table that was passed starts, or the inputs when none was.  A device allocation that holds the table
// gets the mirror's bytes from `first` on.  One that does not gets the table as well: in the same copy when `first`
// follows it directly, else in a copy of its own, so that the gap -- room for tables that were not passed, whose bytes in
// the mirror are not current -- does not travel.  *copied is what went up.
int upload(Roster& r, size_t table_bytes, size_t first, size_t in_bytes, size_t* copied)
{
    *copied = in_bytes - first;
    if (!r.resident) {
        *copied += table_bytes;
        if (first == table_bytes) first = 0;
        else ND_CHECK(hipMemcpyAsync(r.d, r.mirror, table_bytes, hipMemcpyHostToDevice, g.stream));
    }
    ND_CHECK(hipMemcpyAsync(r.d + first, r.mirror + first, in_bytes - first, hipMemcpyHostToDevice, g.stream));
    r.resident = true;
    return 0;
}

// One entry of a call's list of kept tables, which names them in the order the call's layout places their uploads:
// everything such a call does about its kept tables follows from that list.
struct Given {
    int id;                      // which of the roster's kept tables
    const uint8_t* src;          // the caller's, passed because it changed; else nullptr
    const uint8_t** read;        // the kernel's pointer to what this call reads: the upload, or the kept table
    bool unused = false;         // this call does not read the table: it is neither asked for, made nor copied, and *read is nullptr
};

// A table the device does not hold yet must be given: `sentence` is the call's own way to say so.  A table of no
// bytes (the room table of a roster without look rooms) is neither asked for, made nor copied.
template <int N>
int check_given(const Roster& r, const Given (&t)[N], const char* sentence)
{
    for (const Given& e : t)
        if (!e.unused && kept_bytes(r, e.id) && !r.kept[e.id].d && !e.src) {
            snprintf(g_err, sizeof(g_err), "%s", sentence);
            return -1;
        }
    return 0;
}

// The caller's table `id` into the mirror at dst, as it lies on the device.  The clone records alone arrive otherwise:
// packed, the int32 owners, the int32 rooms, then the hear bytes, for take_clones' three slices.
void pack_kept(const Roster& r, int id, uint8_t* dst, const uint8_t* src)
{
    if (id != kKeptClones) {
        memcpy(dst, src, kept_bytes(r, id));
        return;
    }
    Carver at{(uintptr_t)dst};
    const int32_t *owner, *room;
    const uint8_t* hear;
    take_clones(at, r.clones, owner, room, hear);
    const size_t n = (size_t)r.clones;
    memcpy(const_cast<int32_t*>(owner), src, n * sizeof(int32_t));
    memcpy(const_cast<int32_t*>(room), src + n * sizeof(int32_t), n * sizeof(int32_t));
    memcpy(const_cast<uint8_t*>(hear), src + 2 * n * sizeof(int32_t), n);
}

// The kept tables of a call whose mirror and allocation are laid out: at[i].fresh is where table i's upload lies in the
// layout at base 0, kept[i].fresh where it lies on the device, and the inputs start at tables_end.  Makes the kept
// allocations that are not there yet and packs the given tables into the mirror.  What lies after the first given table
// travels too, but the kernel is told of the given ones alone, so the mirror's bytes of the others need not be current:
// one walk of the list gives both *first, where upload() starts -- the first given table, or the inputs -- and
// *copy_blocks, the blocks the kernel's copy tail takes after the call's own.  kept[] is left as copy_kept() wants it,
// and every read pointer at the upload or at the kept table.
template <int N>
int pass_kept(Roster& r, const Given (&t)[N], const Kept (&at)[N], Kept (&kept)[N], size_t tables_end, size_t* first,
              unsigned* copy_blocks)
{
    size_t copy_words = 0;
    *first = tables_end;
    for (int i = 0; i < N; i++) {
        if (t[i].unused) {
            kept[i] = Kept{nullptr, nullptr, 0};
            *t[i].read = nullptr;
            continue;
        }
        KeptTable& k = r.kept[t[i].id];
        const size_t bytes = kept_bytes(r, t[i].id);
        if (bytes && !k.d) {
            hipError_t e = hipMalloc((void**)&k.d, bytes);
            if (e != hipSuccess) {
                k.d = nullptr;
                return fail(k.what, e);
            }
        }
        kept[i].keep = reinterpret_cast<uint32_t*>(k.d);
        kept[i].words = (int)(bytes / sizeof(uint32_t));
        if (t[i].src) {
            pack_kept(r, t[i].id, r.mirror + (uintptr_t)at[i].fresh, t[i].src);
            *first = std::min(*first, (size_t)(uintptr_t)at[i].fresh);
            copy_words += bytes / sizeof(uint32_t);
            *t[i].read = reinterpret_cast<const uint8_t*>(kept[i].fresh);
        } else {
            *t[i].read = k.d;
            kept[i].fresh = nullptr;
        }
    }
    *copy_blocks = (unsigned)((copy_words + kBlock - 1) / kBlock);
    return 0;
}

// nuts_roster_record after a call's planning kernel, on device arrays of that call: the k texts, their rooms and flags
// (bit 2: record), and the pending clears (nullptr: none).  tell: the texts are told lines, rm their targets, and the
// rings the slots' revtell rings.  The rings are touched by g.stream alone.
int launch_record(Roster& r, int k, const uint8_t* text, const int32_t* text_off, const int32_t* text_len,
                  const int32_t* rm, const uint8_t* flags, const uint8_t* clear, bool tell = false)
{
    const RingSet s = rings_of(r, tell);
    RecordArgs rec{text, text_off, text_len, rm, flags, clear, k, s.count, *s.p, s.revline()};
    hipLaunchKernelGGL(tell ? nuts_roster_record_tell : nuts_roster_record, dim3((unsigned)s.count), dim3(kBlock), 0,
                       g.stream, rec);
    ND_CHECK(hipGetLastError());
    return 0;
}

// ---- the steps the five event calls share: nd_roster_go, nd_roster_access, nd_roster_clone, nd_roster_set and nd_roster_act.  Each takes
// k events (slots, [coms,] inpstr, words), composes `texts` texts an event of which `lines` are room lines, defers in a
// *_order kernel, plans with nuts_roster_speak_plan and downloads once.  What differs -- the settings, the kept tables and
// their order, the results of its own -- stays in the call.

// The limits every event call shares: k events of `cells` admit cells a slot and `row` bytes of fixed text slots.
bool events_fit(int k, int cap, int cells, int row, int64_t text_bytes, int nrooms)
{
    return k >= 1 && (int64_t)cells * k * cap < INT32_MAX && (int64_t)k * row < INT32_MAX / 16 && text_bytes >= 0 &&
           text_bytes < INT32_MAX / 32 && nrooms <= kMaxLookRooms;
}

// The kernels index by the events' slots and texts: nothing out of range reaches them.  coms is nullptr for events without
// a command, else com_ok(coms[b]) says whether the call knows it.
template <typename ComOk>
int check_events(int k, int cap, const int32_t* slots, const int32_t* text_off, const int32_t* text_len, int64_t text_bytes,
                 const uint8_t* coms, ComOk com_ok)
{
    int64_t sum = 0;
    for (int b = 0; b < k; b++) {
        if (slots[b] < 0 || slots[b] >= cap || text_len[b] < 0 || text_len[b] >= kArrSize || text_off[b] != sum ||
            (coms && !com_ok((int)coms[b]))) {
            snprintf(g_err, sizeof(g_err), "event %d: slot, %stext length or text offset out of range", b, coms ? "command, " : "");
            return -1;
        }
        sum += text_len[b];
    }
    if (sum != text_bytes) {
        snprintf(g_err, sizeof(g_err), "the events' texts hold %lld bytes, not %lld", (long long)sum, (long long)text_bytes);
        return -1;
    }
    return 0;
}

// What both sets of arguments are told before the layouts: `lines` is the number of room lines an event has.
void size_events(EventArgs& s, SpeakPlanArgs& p, int k, int lines, int cap)
{
    s.k = k;
    p.k = lines * k;
    s.capacity = p.capacity = cap;
    p.tiles = (cap + kBlock - 1) / kBlock;
    p.words = (cap + 63) / 64;
}

// The sizes of an event call, from its layout at base 0 (so, po; first_kept is where the table ends and the first kept
// table's upload starts): one upload runs to the end of violations, one download from violations to the end of the variants.
struct EventSizes {
    size_t texts, ctext_bytes, var_bytes, table_bytes, tables_end, in_bytes, res_at, res_bytes;
};
EventSizes event_sizes(const EventArgs& so, const SpeakPlanArgs& po, const void* first_kept, int texts, size_t ctext_bytes)
{
    EventSizes z{};
    z.texts = (size_t)texts * so.k;
    z.ctext_bytes = ctext_bytes;
    z.var_bytes = (size_t)var_at((int64_t)ctext_bytes, (int64_t)z.texts);
    z.table_bytes = (uintptr_t)first_kept;
    z.tables_end = (uintptr_t)so.text;
    z.in_bytes = (uintptr_t)so.violations + sizeof(int);
    z.res_at = (uintptr_t)so.violations;
    z.res_bytes = (uintptr_t)po.var + z.var_bytes - z.res_at;
    return z;
}

// The mirror holds the call's inputs, and the table when the caller gave one.
int take_given_table(Roster& r, const EventArgs& so, const EventSizes& z, const uint8_t* table)
{
    if (grow_mirror(r, z.in_bytes, z.table_bytes)) return -1;
    if (table) new_table(r, so.room, so.slotf, table);
    return 0;
}

// The compose kernel reads the room record of its event's user (`who`: "mover", "actor").
int check_rooms_of(const Roster& r, const EventArgs& so, const int32_t* slots, const char* who)
{
    const int32_t* room = reinterpret_cast<const int32_t*>(r.mirror + (uintptr_t)so.room);
    for (int b = 0; b < so.k; b++)
        if (room[slots[b]] < 0 || room[slots[b]] >= r.look_rooms) {
            snprintf(g_err, sizeof(g_err), "event %d: the %s's room has no room record", b, who);
            return -1;
        }
    return 0;
}

// The events into the mirror as they lie on the device, every text's slot from text_at(kind, b), and violations zeroed.
template <typename TextAt>
void put_events(const Roster& r, const EventArgs& so, const EventSizes& z, const uint8_t* text, int64_t text_bytes,
                const int32_t* text_off, const int32_t* text_len, const int32_t* slots, const uint8_t* words, TextAt text_at)
{
    const Put put{r.mirror};
    const size_t k = (size_t)so.k;
    put(so.text, text, (size_t)text_bytes);
    put(so.text_off, text_off, k * sizeof(int32_t));
    put(so.text_len, text_len, k * sizeof(int32_t));
    put(so.slot, slots, k * sizeof(int32_t));
    put(so.words, words, k);
    int32_t* coff = reinterpret_cast<int32_t*>(r.mirror + (uintptr_t)so.ctext_off);
    for (size_t kind = 0; kind < z.texts / k; kind++)
        for (size_t b = 0; b < k; b++) coff[kind * k + b] = (int32_t)text_at((int)kind, (int)b);
    *reinterpret_cast<int*>(r.mirror + (uintptr_t)so.violations) = 0;
}

// The one upload: the tables' uploads lie between the table and the inputs.
template <int N>
int upload_events(Roster& r, const Given (&given)[N], const Kept (&at)[N], Kept (&kept)[N], const EventSizes& z, size_t* h2d,
                  unsigned* copy_blocks)
{
    size_t first = 0;
    if (pass_kept(r, given, at, kept, z.tables_end, &first, copy_blocks)) return -1;
    return upload(r, z.table_bytes, first, z.in_bytes, h2d);
}

// The three launches: the compose kernel, its order kernel -- one wave --, and the plan of p.k room lines, a block a tile,
// and the other texts, a block each.
template <typename A, typename O>
int launch_events(void (*compose)(A), unsigned blocks, const A& s, void (*order)(O), const O& o, const SpeakPlanArgs& p,
                  const EventSizes& z)
{
    ND_CHECK(hipEventRecord(g.ev0, g.stream));
    hipLaunchKernelGGL(compose, dim3(blocks), dim3(kBlock), 0, g.stream, s);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(order, dim3(1), dim3(64), 0, g.stream, o);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_speak_plan, dim3((unsigned)((size_t)p.k * p.tiles + z.texts - p.k)), dim3(kBlock), 0, g.stream, p);
    ND_CHECK(hipGetLastError());
    return 0;
}

// What every event call hands back, from the pinned results, unless a text broke its bounds.
int copy_event_results(const Res& res, const EventArgs& so, const SpeakPlanArgs& po, const EventSizes& z, int8_t* outcome,
                       int32_t* clen, uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var)
{
    const int violations = *reinterpret_cast<const int*>(res(so.violations));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d text(s) exceeded the hard bounds (a text its slot; 6*len+4 bytes, %d writes transduced)",
                 violations, kMaxWrites);
        return -1;
    }
    memcpy(outcome, res(so.outcome), (size_t)so.k);
    memcpy(clen, res(so.clen), z.texts * sizeof(int32_t));
    memcpy(vn, res(po.vn), 2 * z.texts * sizeof(int64_t));
    memcpy(vw, res(po.vw), 2 * z.texts * sizeof(int32_t));
    memcpy(vwsz, res(po.vwsz), 2 * z.texts * kMaxWrites * sizeof(int32_t));
    memcpy(bits, res(po.bits), (size_t)po.k * po.words * sizeof(uint64_t));
    memcpy(ctext, res(so.ctext), z.ctext_bytes);
    memcpy(var, res(po.var), z.var_bytes);
    return 0;
}

// The scans' inputs for a roster call of m items.
auto item_bytes(const RosterArgs& a, int m)
{
    return rocprim::make_transform_iterator(rocprim::make_counting_iterator(0),
                                            ItemCount<int64_t>{a.admitted, a.slot, a.vn, a.capacity, m});
}
auto item_writes(const RosterArgs& a, int m)
{
    return rocprim::make_transform_iterator(rocprim::make_counting_iterator(0),
                                            ItemCount<int32_t>{a.admitted, a.slot, a.vw, a.capacity, m});
}

Roster* roster_at(int handle)
{
    if (handle < 0 || handle >= kMaxRosters || !g_rosters[handle].live) {
        snprintf(g_err, sizeof(g_err), "no live roster %d", handle);
        return nullptr;
    }
    return &g_rosters[handle];
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
              int64_t* out_off, int32_t* w_off, nd_timing* timing)
{
    if (ensure_ready()) return -1;
    if (n < 1) {
        snprintf(g_err, sizeof(g_err), "empty batch");
        return -1;
    }
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    Args a{};
    a.n = n;
    a.rm_is_null = rm_is_null;
    a.force_listen = force_listen;
    a.com_num = com_num;
    a.arena_cap = 4 * (int64_t)n + 6 * text_bytes * (broadcast ? n : 1);   // the hard bound, summed over the items
    a.wsz_cap = (int64_t)n * kMaxWrites;
    size_t scan1 = 0, scan2 = 0;     // both scans run over n + 1 entries
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan1, a.nbytes, a.out_off, n + 1, st));
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan2, a.nwrites, a.w_off, n + 1, st));
    const size_t scan_bytes = std::max(scan1, scan2);
    uint8_t* scan = nullptr;
    const size_t need = layout(0, (size_t)text_bytes, scan_bytes, a, &scan);
    if (grow_dev(&g.d_block, &g.cap_block, need, "device buffers")) return -1;
    layout((uintptr_t)g.d_block, (size_t)text_bytes, scan_bytes, a, &scan);

    ND_CHECK(hipMemcpyAsync((void*)a.text, text, (size_t)text_bytes, hipMemcpyHostToDevice, st));
    ND_CHECK(hipMemcpyAsync((void*)a.text_len, text_len, (broadcast ? 1 : (size_t)n) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (!broadcast) ND_CHECK(hipMemcpyAsync((void*)a.text_off, text_off, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    ND_CHECK(hipMemcpyAsync((void*)a.rec, rec, (size_t)n, hipMemcpyHostToDevice, st));
    ND_CHECK(hipMemsetAsync(a.violations, 0, sizeof(int), st));

    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(broadcast ? nuts_fanout_measure_broadcast : nuts_fanout_measure_batch, grid, block, 0, st, a);
    ND_CHECK(hipGetLastError());
    size_t bytes = scan_bytes;
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(scan, bytes, a.nbytes, a.out_off, n + 1, st));
    bytes = scan_bytes;
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(scan, bytes, a.nwrites, a.w_off, n + 1, st));
    hipLaunchKernelGGL(broadcast ? nuts_fanout_emit_broadcast : nuts_fanout_emit_batch, grid, block, 0, st, a);
    ND_CHECK(hipGetLastError());
    ND_CHECK(hipEventRecord(g.ev1, st));

    // the small per-item arrays first: they say how much of the arena to fetch
    int violations = 0;
    ND_CHECK(hipMemcpyAsync(admitted, a.admitted, (size_t)n, hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(out_off, a.out_off, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(w_off, a.w_off, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(&violations, a.violations, sizeof(int), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipStreamSynchronize(st));
    if (check_bounds(violations, "item")) return -1;
    if (grow_host(&g.h_arena, &g.cap_host_arena, (size_t)out_off[n] + 1, "pinned arena")) return -1;
    if (grow_host(&g.h_wsz, &g.cap_host_writes, (size_t)w_off[n] + 1, "pinned write sizes")) return -1;
    ND_CHECK(hipMemcpyAsync(g.h_arena, a.arena, (size_t)out_off[n], hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(g.h_wsz, a.wsz, (size_t)w_off[n] * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipStreamSynchronize(st));
    const double t1 = now_ns();

    return fill_timing(timing, t0, t1);
}

const uint8_t* nd_arena(void) { return g.h_arena; }
const int32_t* nd_write_sizes(void) { return g.h_wsz; }

// K broadcasts in one call.  Broadcast b: the text text[text_off[b] .. text_off[b] + text_len[b]), flags[b] (bit 0
// rm_is_null, bit 1 force_listen), com_num[b], and the listener records rec[item_off[b] .. item_off[b + 1]), at least
// one (item_off[0] = 0, m = item_off[k]).  Outputs as nd_fanout's, over the m items: admitted[m], out_off[m+1],
// w_off[m+1]; the arena and the chunk sizes through nd_arena / nd_write_sizes until the next call.  Whatever k and m:
// one upload, four kernels (two of them the scans), three downloads, two synchronises.  The arena holds the hard
// bound sum of N_b * (6 * text_len[b] + 4); the caller keeps it under its cap and has validated the input as for
// nd_fanout.  Returns 0, or -1 with nd_last_error() set.
int nd_fanout_many(int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off, const int32_t* text_len,
                   const uint8_t* flags, const int32_t* com_num, const int32_t* item_off, const uint8_t* rec,
                   uint8_t* admitted, int64_t* out_off, int32_t* w_off, nd_timing* timing)
{
    if (ensure_ready()) return -1;
    if (k < 1 || item_off[0] != 0) {
        snprintf(g_err, sizeof(g_err), "empty call, or item offsets that do not start at 0");
        return -1;
    }
    for (int b = 0; b < k; b++)
        if (item_off[b + 1] <= item_off[b]) {
            snprintf(g_err, sizeof(g_err), "broadcast %d has no listeners", b);
            return -1;
        }
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    ManyArgs a{};
    a.k = k;
    a.m = item_off[k];
    for (int b = 0; b < k; b++) a.arena_cap += (int64_t)(item_off[b + 1] - item_off[b]) * (6 * (int64_t)text_len[b] + 4);
    a.wsz_cap = (int64_t)a.m * kMaxWrites;
    const int m = a.m;
    size_t scan1 = 0, scan2 = 0;     // both scans run over m + 1 entries
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan1, a.nbytes, a.out_off, m + 1, st));
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan2, a.nwrites, a.w_off, m + 1, st));
    const size_t scan_bytes = std::max(scan1, scan2);
    uint8_t* scan = nullptr;
    ManyArgs o = a;                  // offsets of every array in the block
    const size_t need = layout_many(0, (size_t)text_bytes, scan_bytes, o, &scan);
    if (grow_dev(&g.d_block, &g.cap_block, need, "device buffers")) return -1;
    layout_many((uintptr_t)g.d_block, (size_t)text_bytes, scan_bytes, a, &scan);
    const size_t in_bytes = (uintptr_t)o.violations + sizeof(int);
    const size_t res_at = (uintptr_t)o.violations, res_bytes = (uintptr_t)o.nbytes - res_at;
    if (grow_host(&gm.stage, &gm.cap_stage, in_bytes, "pinned staging")) return -1;
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    // pack the inputs as they lie in the block; the block offsets go with them
    uint8_t* h = gm.stage;
    const Put put{h};
    put(o.text, text, (size_t)text_bytes);
    put(o.text_off, text_off, (size_t)k * sizeof(int32_t));
    put(o.text_len, text_len, (size_t)k * sizeof(int32_t));
    put(o.flags, flags, (size_t)k);
    put(o.com_num, com_num, (size_t)k * sizeof(int32_t));
    put(o.item_off, item_off, ((size_t)k + 1) * sizeof(int32_t));
    int32_t* tiles = reinterpret_cast<int32_t*>(h + (uintptr_t)o.tile_off);
    tiles[0] = 0;
    for (int b = 0; b < k; b++) tiles[b + 1] = tiles[b] + (item_off[b + 1] - item_off[b] + kBlock - 1) / kBlock;
    put(o.rec, rec, (size_t)m);
    *reinterpret_cast<int*>(h + (uintptr_t)o.violations) = 0;
    ND_CHECK(hipMemcpyAsync(g.d_block, h, in_bytes, hipMemcpyHostToDevice, st));

    const dim3 grid((unsigned)tiles[k]), block(kBlock);
    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(nuts_fanout_measure_many, grid, block, 0, st, a);
    ND_CHECK(hipGetLastError());
    size_t bytes = scan_bytes;
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(scan, bytes, a.nbytes, a.out_off, m + 1, st));
    bytes = scan_bytes;
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(scan, bytes, a.nwrites, a.w_off, m + 1, st));
    hipLaunchKernelGGL(nuts_fanout_emit_many, grid, block, 0, st, a);
    ND_CHECK(hipGetLastError());

    // violations, admitted and the offsets in one download: they say how much of the arena to fetch
    if (fetch_results(g.d_block, res_at, res_bytes)) return -1;
    const Res res{gm.res, res_at};
    if (check_bounds(*reinterpret_cast<const int*>(res(o.violations)), "item")) return -1;
    memcpy(admitted, res(o.admitted), (size_t)m);
    memcpy(out_off, res(o.out_off), ((size_t)m + 1) * sizeof(int64_t));
    memcpy(w_off, res(o.w_off), ((size_t)m + 1) * sizeof(int32_t));
    if (grow_host(&g.h_arena, &g.cap_host_arena, (size_t)out_off[m] + 1, "pinned arena")) return -1;
    if (grow_host(&g.h_wsz, &g.cap_host_writes, (size_t)w_off[m] + 1, "pinned write sizes")) return -1;
    ND_CHECK(hipMemcpyAsync(g.h_arena, a.arena, (size_t)out_off[m], hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(g.h_wsz, a.wsz, (size_t)w_off[m] * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipStreamSynchronize(st));
    const double t1 = now_ns();

    return fill_timing(timing, t0, t1);
}

// Timings and copy volume of the last nd_roster_fanout call.
struct nd_roster_timing {
    double kernels_us;      // device events around measure .. emit (both scans included)
    double end_to_end_us;   // host clock: packing the inputs, H2D, kernels, D2H of results, ending in a synchronise
    int64_t h2d_bytes;      // the inputs, plus the table when it was given or the device allocation is new
    int64_t d2h_bytes;
};

// A roster of `capacity` slots (1 .. 65536), every slot empty.  Nothing is allocated until its first nd_roster_fanout.
// Returns a handle, or -1 with nd_last_error() set; at most 64 rosters are live at once.
int nd_roster_create(int capacity)
{
    if (capacity < 1 || capacity > kMaxCapacity) {
        snprintf(g_err, sizeof(g_err), "roster capacity %d outside 1 .. %d", capacity, kMaxCapacity);
        return -1;
    }
    for (int h = 0; h < kMaxRosters; h++)
        if (!g_rosters[h].live) {
            g_rosters[h] = Roster{};
            g_rosters[h].live = true;
            g_rosters[h].capacity = capacity;
            return h;
        }
    snprintf(g_err, sizeof(g_err), "%d rosters are live: destroy one first", kMaxRosters);
    return -1;
}

// Frees the roster's device allocation and mirror.  Returns 0, or -1 for a handle that is not live.
int nd_roster_destroy(int handle)
{
    Roster* r = roster_at(handle);
    if (!r) return -1;
    if (r->d) (void)hipFree(r->d);
    if (r->rings) (void)hipFree(r->rings);
    if (r->tell_rings) (void)hipFree(r->tell_rings);
    for (const KeptTable& k : r->kept)
        if (k.d) (void)hipFree(k.d);
    if (r->mirror) (void)hipHostFree(r->mirror);
    *r = Roster{};
    return 0;
}

// K broadcasts to roster `handle`.  Broadcast b: the text text[text_off[b] .. text_off[b] + text_len[b]), room rm[b]
// (-1: every room), sender slot sender[b] (-1: none), flags[b] (bit 1 force_listen, as nd_fanout_many's; rm_is_null is
// rm[b] < 0) and com_num[b].  table is NULL when the roster has not changed since the last call, else all of it:
// `capacity` int32 rooms (-1: none), then `capacity` flag bytes (login 1, ignall 8, ignshout 16, colour 64: their
// listener-record bits).  Outputs as nd_fanout_many's over the m = k * capacity items, item (b, j) at b * capacity + j.
// Whatever k: one upload (the table in it only when given or when the device allocation is new), four kernels (two of
// them the scans), three downloads, two synchronises.  The arena holds the hard bound, the slots with a room times the
// sum of 6 * text_len[b] + 4; the caller keeps it under its cap and has validated the input (texts as for nd_fanout,
// rooms, senders).  Returns 0, or -1 with nd_last_error() set.
int nd_roster_fanout(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                     const int32_t* text_len, const int32_t* rm, const int32_t* sender, const uint8_t* flags,
                     const int32_t* com_num, const uint8_t* table, uint8_t* admitted, int64_t* out_off, int32_t* w_off,
                     nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int64_t m64 = (int64_t)k * r->capacity;
    if (k < 1 || m64 >= INT32_MAX) {
        snprintf(g_err, sizeof(g_err), "%d broadcasts to %d slots: need 1 <= k * capacity < 2^31 - 1", k, r->capacity);
        return -1;
    }
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    const int m = (int)m64, cap = r->capacity;
    RosterArgs a{};
    a.k = k;
    a.capacity = cap;
    a.tiles = (cap + kBlock - 1) / kBlock;
    RosterArgs o = a;                // offsets of every array in the roster's allocation
    const size_t need = layout_roster(0, (size_t)text_bytes, o);
    const size_t table_bytes = (uintptr_t)o.text, in_bytes = (uintptr_t)o.violations + sizeof(int);
    const size_t res_at = (uintptr_t)o.violations, res_bytes = (uintptr_t)o.w_off + ((size_t)m + 1) * sizeof(int32_t) - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (table) new_table(*r, o.room, o.slot, table);
    if (grow_roster(*r, need)) return -1;
    layout_roster((uintptr_t)r->d, (size_t)text_bytes, a);
    for (int b = 0; b < k; b++) a.arena_cap += r->rooms * (6 * (int64_t)text_len[b] + 4);
    a.wsz_cap = r->rooms * k * kMaxWrites;
    size_t scan1 = 0, scan2 = 0;     // both scans run over m + 1 entries
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan1, item_bytes(a, m), a.out_off, m + 1, st));
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan2, item_writes(a, m), a.w_off, m + 1, st));
    const size_t scan_bytes = std::max(scan1, scan2), var_bytes = (size_t)var_at(text_bytes, k);
    uint8_t* scan = nullptr;
    RosterArgs w = a;
    const size_t work = layout_roster_work(0, var_bytes, scan_bytes, w, &scan);
    if (grow_dev(&g.d_block, &g.cap_block, work, "device buffers")) return -1;
    layout_roster_work((uintptr_t)g.d_block, var_bytes, scan_bytes, a, &scan);
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    // the inputs packed after the table, as they lie in the device allocation; the table goes with them if it changed
    uint8_t* h = r->mirror;
    const Put put{h};
    put(o.text, text, (size_t)text_bytes);
    put(o.text_off, text_off, (size_t)k * sizeof(int32_t));
    put(o.text_len, text_len, (size_t)k * sizeof(int32_t));
    put(o.rm, rm, (size_t)k * sizeof(int32_t));
    put(o.sender, sender, (size_t)k * sizeof(int32_t));
    put(o.flags, flags, (size_t)k);
    put(o.com_num, com_num, (size_t)k * sizeof(int32_t));
    *reinterpret_cast<int*>(h + (uintptr_t)o.violations) = 0;
    const size_t from = r->resident ? table_bytes : 0;
    ND_CHECK(hipMemcpyAsync(r->d + from, h + from, in_bytes - from, hipMemcpyHostToDevice, st));
    r->resident = true;

    const dim3 grid((unsigned)(k * a.tiles)), block(kBlock);
    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(nuts_roster_measure, grid, block, 0, st, a);
    ND_CHECK(hipGetLastError());
    size_t bytes = scan_bytes;
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(scan, bytes, item_bytes(a, m), a.out_off, m + 1, st));
    bytes = scan_bytes;
    ND_CHECK(hipcub::DeviceScan::ExclusiveSum(scan, bytes, item_writes(a, m), a.w_off, m + 1, st));
    hipLaunchKernelGGL(nuts_roster_emit, grid, block, 0, st, a);
    ND_CHECK(hipGetLastError());

    // violations, admitted and the offsets in one download: they say how much of the arena to fetch
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const Res res{gm.res, res_at};
    if (check_bounds(*reinterpret_cast<const int*>(res(o.violations)), "variant")) return -1;
    memcpy(admitted, res(o.admitted), (size_t)m);
    memcpy(out_off, res(o.out_off), ((size_t)m + 1) * sizeof(int64_t));
    memcpy(w_off, res(o.w_off), ((size_t)m + 1) * sizeof(int32_t));
    if (grow_host(&g.h_arena, &g.cap_host_arena, (size_t)out_off[m] + 1, "pinned arena")) return -1;
    if (grow_host(&g.h_wsz, &g.cap_host_writes, (size_t)w_off[m] + 1, "pinned write sizes")) return -1;
    ND_CHECK(hipMemcpyAsync(g.h_arena, a.arena, (size_t)out_off[m], hipMemcpyDeviceToHost, st));
    ND_CHECK(hipMemcpyAsync(g.h_wsz, a.wsz, (size_t)w_off[m] * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    ND_CHECK(hipStreamSynchronize(st));
    const double t1 = now_ns();

    return fill_timing(timing, t0, t1, in_bytes - from,
                       res_bytes + (size_t)out_off[m] + (size_t)w_off[m] * sizeof(int32_t));
}

// A delivery plan for K broadcasts to roster `handle`: inputs and table exactly as nd_roster_fanout's.  Outputs (host,
// caller-allocated), with W = ceil(capacity / 64): bits[k * W], slot j of broadcast b is bit j % 64 of
// bits[b * W + j / 64] and the bits past the capacity are zero; vn[2k] / vw[2k], the bytes and write(2) counts of
// broadcast b's colour-off (2b) and colour-on (2b + 1) variant; vwsz[2k * 16] their chunk sizes (entries at or past
// vw are unspecified); var[12 * text_bytes + 16 * k] the variants' bytes, broadcast b's at 12 * text_off[b] + 16 * b and
// that plus (6 * text_len[b] + 4 rounded up to 4), the gaps unspecified.  The results lie next to each other after the
// inputs and are fetched at their bound size, so per call, whatever k and the capacity: one upload (the table in it
// only when given or when the device allocation is new), one kernel, one download, one synchronise, no memset.  May be
// mixed with nd_roster_fanout on one roster in any order.  Returns 0, or -1 with nd_last_error() set.
//
// record (nd_roster_plan_record): also store every broadcast whose flags byte has bit 2 set in the review ring of its
// room rm, in the call's order, as np_record does (the caller has checked 0 <= rm < review_rooms for them), after
// clearing the rings of the rooms whose byte in clear (NULL: none, else review_rooms bytes) is non-zero.  That adds
// nuts_roster_record after nuts_roster_plan in the stream and the clear bytes to the upload: no copy, no synchronise.
static int plan_call(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                     const int32_t* text_len, const int32_t* rm, const int32_t* sender, const uint8_t* flags,
                     const int32_t* com_num, const uint8_t* table, uint64_t* bits, int64_t* vn, int32_t* vw,
                     int32_t* vwsz, uint8_t* var, nd_roster_timing* timing, bool record, const uint8_t* clear)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    if (record && ensure_rings(*r, g.stream)) return -1;
    const int cap = r->capacity, words = (cap + 63) / 64;
    if (k < 1 || (int64_t)k * cap >= INT32_MAX || text_bytes < 0) {
        snprintf(g_err, sizeof(g_err), "%d broadcasts to %d slots: need 1 <= k * capacity < 2^31 - 1", k, cap);
        return -1;
    }
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    PlanArgs a{};
    a.k = k;
    a.capacity = cap;
    a.tiles = (cap + kBlock - 1) / kBlock;
    a.words = words;
    const size_t var_bytes = (size_t)var_at(text_bytes, k);
    PlanArgs o = a;                  // offsets of every array in the roster's allocation
    const size_t clear_bytes = record && clear ? (size_t)r->review_rooms : 0;
    const uint8_t *o_clear = nullptr, *d_clear = nullptr;
    const size_t need = layout_plan(0, (size_t)text_bytes, var_bytes, o, clear_bytes, &o_clear);
    const size_t table_bytes = (uintptr_t)o.text, in_bytes = (uintptr_t)o.violations + sizeof(int);
    const size_t res_at = (uintptr_t)o.violations, res_bytes = (uintptr_t)o.var + var_bytes - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (table) new_table(*r, o.room, o.slot, table);
    if (grow_roster(*r, need)) return -1;
    layout_plan((uintptr_t)r->d, (size_t)text_bytes, var_bytes, a, clear_bytes, &d_clear);
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    // the inputs packed after the table, as they lie in the device allocation; the table goes with them if it changed
    uint8_t* h = r->mirror;
    const Put put{h};
    put(o.text, text, (size_t)text_bytes);
    put(o.text_off, text_off, (size_t)k * sizeof(int32_t));
    put(o.text_len, text_len, (size_t)k * sizeof(int32_t));
    put(o.rm, rm, (size_t)k * sizeof(int32_t));
    put(o.sender, sender, (size_t)k * sizeof(int32_t));
    put(o.flags, flags, (size_t)k);
    put(o.com_num, com_num, (size_t)k * sizeof(int32_t));
    put(o_clear, clear, clear_bytes);
    *reinterpret_cast<int*>(h + (uintptr_t)o.violations) = 0;
    const size_t from = r->resident ? table_bytes : 0;
    ND_CHECK(hipMemcpyAsync(r->d + from, h + from, in_bytes - from, hipMemcpyHostToDevice, st));
    r->resident = true;

    const dim3 grid((unsigned)(k * a.tiles)), block(kBlock);
    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(nuts_roster_plan, grid, block, 0, st, a);
    ND_CHECK(hipGetLastError());
    // on the inputs just uploaded
    if (record && launch_record(*r, k, a.text, a.text_off, a.text_len, a.rm, a.flags, clear_bytes ? d_clear : nullptr))
        return -1;
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, res_at};
    if (check_bounds(*reinterpret_cast<const int*>(res(o.violations)), "variant")) return -1;
    memcpy(vn, res(o.vn), 2 * (size_t)k * sizeof(int64_t));
    memcpy(vw, res(o.vw), 2 * (size_t)k * sizeof(int32_t));
    memcpy(vwsz, res(o.vwsz), 2 * (size_t)k * kMaxWrites * sizeof(int32_t));
    memcpy(bits, res(o.bits), (size_t)k * words * sizeof(uint64_t));
    memcpy(var, res(o.var), var_bytes);

    return fill_timing(timing, t0, t1, in_bytes - from, res_bytes);
}

// The plan alone (plan_call above): bit 2 of flags[] is not looked at, and nothing touches the rings.
int nd_roster_plan(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                   const int32_t* text_len, const int32_t* rm, const int32_t* sender, const uint8_t* flags,
                   const int32_t* com_num, const uint8_t* table, uint64_t* bits, int64_t* vn, int32_t* vw,
                   int32_t* vwsz, uint8_t* var, nd_roster_timing* timing)
{
    return plan_call(handle, k, text, text_bytes, text_off, text_len, rm, sender, flags, com_num, table, bits, vn, vw,
                     vwsz, var, timing, false, nullptr);
}

// The plan, then the records (plan_call above): nd_roster_plan's arguments, and clear.  The roster needs review rings.
int nd_roster_plan_record(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                          const int32_t* text_len, const int32_t* rm, const int32_t* sender, const uint8_t* flags,
                          const int32_t* com_num, const uint8_t* table, uint64_t* bits, int64_t* vn, int32_t* vw,
                          int32_t* vwsz, uint8_t* var, nd_roster_timing* timing, const uint8_t* clear)
{
    return plan_call(handle, k, text, text_bytes, text_off, text_len, rm, sender, flags, com_num, table, bits, vn, vw,
                     vwsz, var, timing, true, clear);
}

// Give roster `handle` review rings for rooms 0 .. n - 1 (0 .. 1024), all empty; before its first recording or
// reviewing call, which allocates them.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_review_rooms(int handle, int n)
{
    Roster* r = roster_at(handle);
    if (!r) return -1;
    if (n < 0 || n > kMaxReviewRooms || r->rings) {
        snprintf(g_err, sizeof(g_err), "review rooms %d outside 0 .. %d, or the rings are already in use", n,
                 kMaxReviewRooms);
        return -1;
    }
    r->review_rooms = n;
    return 0;
}

// What .review sends for each of the q rooms[] (ring rooms, duplicates allowed; the caller has checked them), after
// clearing the rings that clear marks, as nd_roster_plan_record does.  Outputs (host, caller-allocated): line_count[q]
// the non-empty lines; sequential[q] the (line, variant) pairs that took the sequential transducer; vn[2q] / vw[2q] the
// bytes and write(2) counts of room i's colour-off (2i) and colour-on (2i + 1) review; vwsz[2q * 45] their chunk sizes
// (entries at or past vw unspecified); lines[q * 15 * 202] the ring's slots, oldest first; var[2q * 18152] the reviews'
// bytes, variant v at v * 18152, the rest unspecified.  Per call, whatever q and whatever the rings hold: one upload,
// one kernel, one download at the bound size, one synchronise.  Returns 0, or -1 with nd_last_error() set.
//
// tell (nd_roster_revtell): the same over the slots' revtell rings, rooms[] slots, clear `capacity` bytes, 5 lines where
// there were 15: vwsz[2q * 15], lines[q * 5 * 202], var[2q * 6052].
static int review_call(int handle, int q, const int32_t* rooms, const uint8_t* clear, int32_t* line_count,
                       int32_t* sequential, int32_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* lines, uint8_t* var,
                       nd_roster_timing* timing, bool tell)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const RingSet set = rings_of(*r, tell);
    const int nlines = set.lines, stride = rev_var_stride(nlines);
    if (q < 1 || (int64_t)q * 2 * stride >= INT32_MAX) {
        snprintf(g_err, sizeof(g_err), "%d rooms to review: need 1 <= q and 2 * q * %d < 2^31 - 1", q, stride);
        return -1;
    }
    if (ensure_rings(*r, g.stream, tell)) return -1;
    for (int i = 0; i < q; i++)
        if (rooms[i] < 0 || rooms[i] >= set.count) {
            snprintf(g_err, sizeof(g_err), tell ? "slot %d has no revtell ring" : "room %d has no review ring", rooms[i]);
            return -1;
        }
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    ReviewArgs a{};
    a.q = q;
    a.review_rooms = set.count;
    const size_t clear_bytes = clear ? (size_t)set.count : 0;
    ReviewArgs o = a;                // offsets of every array in the roster's allocation
    const size_t need = layout_review(0, r->capacity, clear_bytes, o, nlines);
    const size_t table_bytes = (uintptr_t)o.rooms, in_bytes = (uintptr_t)o.violations + sizeof(int);
    const size_t res_at = (uintptr_t)o.violations, res_bytes = need - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (grow_roster(*r, need)) return -1;
    layout_review((uintptr_t)r->d, r->capacity, clear_bytes, a, nlines);
    if (!clear) a.clear = nullptr;
    a.rings = *set.p;
    a.revline = set.revline();
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    uint8_t* h = r->mirror;
    memcpy(h + (uintptr_t)o.rooms, rooms, (size_t)q * sizeof(int32_t));
    if (clear) memcpy(h + (uintptr_t)o.clear, clear, clear_bytes);
    *reinterpret_cast<int*>(h + (uintptr_t)o.violations) = 0;
    ND_CHECK(hipMemcpyAsync(r->d + table_bytes, h + table_bytes, in_bytes - table_bytes, hipMemcpyHostToDevice, st));

    // one block per requested room, then the blocks that store the pending clears, a ring room per lane
    const unsigned grid = (unsigned)q + (clear ? (unsigned)((set.count + kBlock - 1) / kBlock) : 0u);
    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(tell ? nuts_roster_revtell : nuts_roster_review, dim3(grid), dim3(kBlock), 0, st, a);
    ND_CHECK(hipGetLastError());
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, res_at};
    const int violations = *reinterpret_cast<const int*>(res(o.violations));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d line(s) exceeded the hard output bounds (%d bytes, %d writes)", violations,
                 kRevLineCap, kRevLineWrites);
        return -1;
    }
    memcpy(line_count, res(o.line_count), (size_t)q * sizeof(int32_t));
    memcpy(sequential, res(o.sequential), (size_t)q * sizeof(int32_t));
    memcpy(vn, res(o.vn), 2 * (size_t)q * sizeof(int32_t));
    memcpy(vw, res(o.vw), 2 * (size_t)q * sizeof(int32_t));
    memcpy(vwsz, res(o.vwsz), 2 * (size_t)q * nlines * kRevLineWrites * sizeof(int32_t));
    memcpy(lines, res(o.lines), (size_t)q * nlines * kRevSlot);
    memcpy(var, res(o.var), 2 * (size_t)q * stride);

    return fill_timing(timing, t0, t1, in_bytes - table_bytes, res_bytes);
}

// The rooms' review rings (review_call above).
int nd_roster_review(int handle, int q, const int32_t* rooms, const uint8_t* clear, int32_t* line_count,
                     int32_t* sequential, int32_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* lines, uint8_t* var,
                     nd_roster_timing* timing)
{
    return review_call(handle, q, rooms, clear, line_count, sequential, vn, vw, vwsz, lines, var, timing, false);
}

// Give roster `handle` a revtell ring per slot, all empty; before its first recording nd_roster_tell or nd_roster_revtell,
// which allocates them (1,010 bytes per slot and a cursor).  Returns 0, or -1 with nd_last_error() set.
int nd_roster_revtell_rings(int handle)
{
    Roster* r = roster_at(handle);
    if (!r) return -1;
    r->revtell = true;
    return 0;
}

// What .revtell sends for each of the q slots[] (nd_roster_review's comment, review_call above).
int nd_roster_revtell(int handle, int q, const int32_t* slots, const uint8_t* clear, int32_t* line_count,
                      int32_t* sequential, int32_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* lines, uint8_t* var,
                      nd_roster_timing* timing)
{
    return review_call(handle, q, slots, clear, line_count, sequential, vn, vw, vwsz, lines, var, timing, true);
}

// What nd_roster_input returns of nuts_roster_parse: host arrays of k entries each.
struct ParseOut {
    int8_t* kind;
    int8_t* com;
    uint8_t* words;
    int32_t* line_len;
    int32_t* inp_off;
    int32_t* inp_len;
};

// nd_roster_speak (parsed NULL), and nd_roster_input: there text, text_off and text_len are the reads, coms and words
// are NULL, and nuts_roster_parse runs first.
static int speech_call(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                       const int32_t* text_len, const int32_t* slots, const uint8_t* coms, const uint8_t* words,
                       int ban_swearing, int record, const uint8_t* table, const uint8_t* speech, const uint8_t* clear,
                       int8_t* outcome, int32_t* clen, uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz,
                       uint8_t* ctext, uint8_t* var, nd_roster_timing* timing, const ParseOut* parsed)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nwords = (cap + 63) / 64;
    if (k < 1 || (int64_t)k * cap >= INT32_MAX || text_bytes < 0 || text_bytes >= INT32_MAX / 32) {
        snprintf(g_err, sizeof(g_err), "%d events to %d slots: need 1 <= k * capacity < 2^31 - 1", k, cap);
        return -1;
    }
    int64_t sum = 0;
    for (int b = 0; b < k; b++) {       // the kernels index by these: nothing out of range reaches them
        if (parsed) {                   // a read: 1 .. 1000 bytes, and its last byte ends the line
            if (slots[b] < 0 || slots[b] >= cap || text_len[b] < 1 || text_len[b] > kArrSize || text_off[b] != sum ||
                sum + text_len[b] > text_bytes || (int8_t)text[sum + text_len[b] - 1] >= 32) {
                snprintf(g_err, sizeof(g_err), "read %d: slot, length, offset or last byte out of range", b);
                return -1;
            }
            sum += text_len[b];
            continue;
        }
        const bool com_ok = coms[b] == kComSay || coms[b] == kComShout || coms[b] == kComEmote || coms[b] == kComSemote;
        if (slots[b] < 0 || slots[b] >= cap || !com_ok || text_len[b] < 0 || text_len[b] >= kArrSize ||
            text_off[b] != sum) {
            snprintf(g_err, sizeof(g_err), "event %d: slot, command, text length or text offset out of range", b);
            return -1;
        }
        sum += text_len[b];
    }
    if (sum != text_bytes) {
        snprintf(g_err, sizeof(g_err), "the events' texts hold %lld bytes, not %lld", (long long)sum, (long long)text_bytes);
        return -1;
    }
    SpeakArgs s{};
    const Given given[] = {{kKeptSpeech, speech, &s.speech}};
    if (check_given(*r, given, "the roster's first speech call must give the speaker table")) return -1;
    if (record && ensure_rings(*r, g.stream)) return -1;
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    SpeakPlanArgs p{};
    s.k = p.k = k;
    s.capacity = p.capacity = cap;
    s.blocks = (k + kBlock / 64 - 1) / (kBlock / 64);
    s.ban_swearing = ban_swearing != 0;
    s.record = record != 0;
    p.tiles = (cap + kBlock - 1) / kBlock;
    p.words = nwords;
    const size_t ctext_bytes = (size_t)ctext_at(2 * text_bytes, 2 * (int64_t)k);
    const size_t var_bytes = (size_t)var_at((int64_t)ctext_bytes, 2 * (int64_t)k);
    const size_t clear_bytes = record && clear ? (size_t)r->review_rooms : 0;
    SpeakArgs so = s;                // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const uint8_t *o_clear = nullptr, *d_clear = nullptr;
    ParseArgs q{}, qo{};
    q.k = qo.k = k;
    const size_t need = layout_speak(0, (size_t)text_bytes, clear_bytes, so, po, &o_clear, parsed ? &qo : nullptr);
    const size_t table_bytes = (uintptr_t)so.kept[0].fresh, tables_end = (uintptr_t)so.text;
    const size_t in_bytes = (uintptr_t)so.violations + sizeof(int);
    const size_t res_at = (uintptr_t)so.violations, res_bytes = (uintptr_t)po.var + var_bytes - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (table) new_table(*r, so.room, po.slot, table);
    if (grow_roster(*r, need)) return -1;
    layout_speak((uintptr_t)r->d, (size_t)text_bytes, clear_bytes, s, p, &d_clear, parsed ? &q : nullptr);
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    uint8_t* h = r->mirror;
    const Put put{h};
    put(so.text, text, (size_t)text_bytes);
    put(parsed ? qo.read_off : so.text_off, text_off, (size_t)k * sizeof(int32_t));
    put(parsed ? qo.read_len : so.text_len, text_len, (size_t)k * sizeof(int32_t));
    put(so.slot, slots, (size_t)k * sizeof(int32_t));
    if (!parsed) {
        put(so.com, coms, (size_t)k);
        put(so.words, words, (size_t)k);
    }
    int32_t* coff = reinterpret_cast<int32_t*>(h + (uintptr_t)so.ctext_off);
    for (int b = 0; b < k; b++) {
        coff[b] = (int32_t)ctext_at(text_off[b], b);
        coff[k + b] = (int32_t)ctext_at(text_bytes + text_off[b], k + b);
    }
    put(o_clear, clear, clear_bytes);
    *reinterpret_cast<int*>(h + (uintptr_t)so.violations) = 0;
    // the speaker table's upload lies between the table and the inputs: it travels only when it was given
    size_t first = 0, h2d = 0;
    unsigned copy_blocks = 0;
    if (pass_kept(*r, given, so.kept, s.kept, tables_end, &first, &copy_blocks)) return -1;
    if (upload(*r, table_bytes, first, in_bytes, &h2d)) return -1;

    ND_CHECK(hipEventRecord(g.ev0, st));
    if (parsed) {
        q.speech = s.speech;
        hipLaunchKernelGGL(nuts_roster_parse, dim3((unsigned)s.blocks), dim3(kBlock), 0, st, q);
        ND_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(nuts_roster_speak, dim3((unsigned)s.blocks + copy_blocks), dim3(kBlock), 0, st, s);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_speak_plan, dim3((unsigned)(k * p.tiles + k)), dim3(kBlock), 0, st, p);
    ND_CHECK(hipGetLastError());
    // on the arrays nuts_roster_speak wrote
    if (record && launch_record(*r, k, s.ctext, s.ctext_off, s.clen, s.rm, s.flags, clear_bytes ? d_clear : nullptr))
        return -1;
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, res_at};
    const int violations = *reinterpret_cast<const int*>(res(so.violations));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d text(s) exceeded the hard bounds (inpstr + %d bytes composed; 6*len+4 bytes, "
                 "%d writes transduced)", violations, kSpeakSlack, kMaxWrites);
        return -1;
    }
    if (parsed) {
        memcpy(parsed->kind, res(qo.kind), (size_t)k);
        memcpy(parsed->com, res(qo.com), (size_t)k);
        memcpy(parsed->words, res(qo.words), (size_t)k);
        memcpy(parsed->line_len, res(qo.line_len), (size_t)k * sizeof(int32_t));
        memcpy(parsed->inp_len, res(qo.text_len), (size_t)k * sizeof(int32_t));
        const int32_t* at = reinterpret_cast<const int32_t*>(res(qo.text_off));
        for (int b = 0; b < k; b++) parsed->inp_off[b] = at[b] - text_off[b];      // relative to the read's own data
    }
    memcpy(outcome, res(so.outcome), (size_t)k);
    memcpy(clen, res(so.clen), 2 * (size_t)k * sizeof(int32_t));
    memcpy(vn, res(po.vn), 4 * (size_t)k * sizeof(int64_t));
    memcpy(vw, res(po.vw), 4 * (size_t)k * sizeof(int32_t));
    memcpy(vwsz, res(po.vwsz), 4 * (size_t)k * kMaxWrites * sizeof(int32_t));
    memcpy(bits, res(po.bits), (size_t)k * nwords * sizeof(uint64_t));
    memcpy(ctext, res(so.ctext), ctext_bytes);
    memcpy(var, res(po.var), var_bytes);

    return fill_timing(timing, t0, t1, h2d, res_bytes);
}

// K speech events of roster `handle`, as say(), shout(), emote() and semote() answer them.  Event b: the speaker's slot
// slots[b], the command coms[b] (NP_SAY 3, NP_SHOUT 4, NP_EMOTE 6, NP_SEMOTE 7), inpstr text[text_off[b] .. + text_len[b])
// (packed: text_off[0] = 0, text_off[b + 1] = text_off[b] + text_len[b]; at most 999 bytes each) and word_count words[b].
// table as nd_roster_plan's.  speech is NULL when no speaker state changed since the last nd_roster_speak of this roster,
// else all of it: 16 bytes per slot, the name's 12 bytes, its length, a flags byte (vis 1, muzzled 2, command_mode 4),
// the level and a byte of padding; the first call of a roster must give it.  record: store the spoken says and emotes in their
// rooms' rings, after clearing those that clear marks (NULL: none), as nd_roster_plan_record does; the caller has checked
// that their speakers' rooms are ring rooms.
// Outputs (host, caller-allocated), with W = ceil(capacity / 64) and text t = b for event b's room line, k + b for its
// reply: outcome[k] (0 spoken, 1 muzzled, 2 nothing to say, 3 swearing); clen[2k] the composed texts' lengths, -1 where
// there is none; ctext[2 * text_bytes + 72 * k] their bytes, text t at ctext_off(t) = text_off[b] + 36 * b, plus
// text_bytes + 36 * k for a reply; bits[k * W] the room lines' admit bitmap, as nd_roster_plan's; vn[4k], vw[4k],
// vwsz[4k * 16] the two variants of text t at 2t and 2t + 1, all zero for a text that is not there; var[12 * ctext bytes +
// 32 * k] their bytes, text t's at 12 * ctext_off(t) + 16 * t and that plus (6 * clen[t] + 4 rounded up to 4).
// Per call, whatever k and the capacity: one upload, two kernels (nuts_roster_speak, nuts_roster_speak_plan) and
// nuts_roster_record as a third when record is set, one download at the bound size, one synchronise.
// Returns 0, or -1 with nd_last_error() set.
int nd_roster_speak(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                    const int32_t* text_len, const int32_t* slots, const uint8_t* coms, const uint8_t* words,
                    int ban_swearing, int record, const uint8_t* table, const uint8_t* speech, const uint8_t* clear,
                    int8_t* outcome, int32_t* clen, uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz,
                    uint8_t* ctext, uint8_t* var, nd_roster_timing* timing)
{
    return speech_call(handle, k, text, text_bytes, text_off, text_len, slots, coms, words, ban_swearing, record, table,
                       speech, clear, outcome, clen, bits, vn, vw, vwsz, ctext, var, timing, nullptr);
}

// K reads of clients in line mode, framed and dispatched as user_input() and exec_com() do, and the speech among them
// answered as nd_roster_speak answers it.  Read b: the speaker's slot slots[b] and the bytes data[read_off[b] .. +
// read_len[b]) (packed, 1 .. 1000 bytes each, the last one below 32 as a signed char).  table, speech, record and clear
// as nd_roster_speak's; the speaker's level is byte 14 of its 16 bytes.
// Outputs of the parse, k entries each: kind (0 IAC, 1 empty, 2 repeat, 3 unknown, 4 speech, 5 command), com (-1: none),
// words, line_len, and inp_off / inp_len, where inpstr lies in the read's own bytes (inp_len -1: none).  The others as
// nd_roster_speak's with the reads in the inpstr's place: text t's slot is read_len[b] + 36 bytes wide at read_off[b] +
// 36 * b.  outcome is -1 for a read that no speech command answers: it has no texts, but for an unknown command's reply.
// Per call, whatever k and the capacity: one upload, three kernels (nuts_roster_parse, nuts_roster_speak,
// nuts_roster_speak_plan) and nuts_roster_record as a fourth when record is set, one download at the bound size, one
// synchronise.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_input(int handle, int k, const uint8_t* data, int64_t data_bytes, const int32_t* read_off,
                    const int32_t* read_len, const int32_t* slots, int ban_swearing, int record, const uint8_t* table,
                    const uint8_t* speech, const uint8_t* clear, int8_t* kind, int8_t* com, uint8_t* words,
                    int32_t* line_len, int32_t* inp_off, int32_t* inp_len, int8_t* outcome, int32_t* clen, uint64_t* bits,
                    int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var, nd_roster_timing* timing)
{
    const ParseOut parsed{kind, com, words, line_len, inp_off, inp_len};
    return speech_call(handle, k, data, data_bytes, read_off, read_len, slots, nullptr, nullptr, ban_swearing, record,
                       table, speech, clear, outcome, clen, bits, vn, vw, vwsz, ctext, var, timing, &parsed);
}

// K private speech events of roster `handle`, as tell() and pemote() answer them.  Event b: the speaker's slot slots[b],
// the command coms[b] (NP_TELL 5, NP_PEMOTE 8), inpstr and words[b] as nd_roster_speak's.  table and speech as
// nd_roster_speak's, the speech flags byte with afk 8 and igntell 16 as well; afk is NULL when no AFK message changed
// since the last nd_roster_tell of this roster, else all of them: 64 bytes per slot, 60 of message padded with zeros,
// then its length; the roster's first call must give it.  record: store every told line in its target's revtell ring
// (nd_roster_revtell_rings), after clearing the rings that clear marks (NULL: none, else `capacity` bytes).
// Outputs (host, caller-allocated), text t = b for event b's told line, k + b for its reply: outcome[k] (0 told, 1
// muzzled, 2 nothing, 4 nobody, 5 self, 6 afk, 7 ignall, 8 igntell, 9 offsite); target[k] the slot get_user found, or -1;
// clen[2k]; ctext[2 * text_bytes + 192 * k], text t at text_off[b] + 96 * b, plus text_bytes + 96 * k for a reply; vn[4k],
// vw[4k], vwsz[4k * 16] and var[12 * ctext bytes + 32 * k] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, two kernels (nuts_roster_tell, nuts_roster_speak_plan) and
// nuts_roster_record_tell as a third when record is set, one download at the bound size, one synchronise.
// Returns 0, or -1 with nd_last_error() set.
int nd_roster_tell(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                   const int32_t* text_len, const int32_t* slots, const uint8_t* coms, const uint8_t* words, int record,
                   const uint8_t* table, const uint8_t* speech, const uint8_t* afk, const uint8_t* clear, int8_t* outcome,
                   int32_t* target, int32_t* clen, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var,
                   nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity;
    if (k < 1 || (int64_t)k * cap >= INT32_MAX || text_bytes < 0 || text_bytes >= INT32_MAX / 32) {
        snprintf(g_err, sizeof(g_err), "%d events to %d slots: need 1 <= k * capacity < 2^31 - 1", k, cap);
        return -1;
    }
    int64_t sum = 0;
    for (int b = 0; b < k; b++) {       // the kernels index by these: nothing out of range reaches them
        if (slots[b] < 0 || slots[b] >= cap || (coms[b] != kComTell && coms[b] != kComPemote) || text_len[b] < 0 ||
            text_len[b] >= kArrSize || text_off[b] != sum) {
            snprintf(g_err, sizeof(g_err), "event %d: slot, command, text length or text offset out of range", b);
            return -1;
        }
        sum += text_len[b];
    }
    if (sum != text_bytes) {
        snprintf(g_err, sizeof(g_err), "the events' texts hold %lld bytes, not %lld", (long long)sum, (long long)text_bytes);
        return -1;
    }
    TellArgs s{};
    const Given given[] = {{kKeptSpeech, speech, &s.speech}, {kKeptAfk, afk, &s.afk}};
    if (check_given(*r, given, "the roster's first private speech call must give the speaker table and the AFK messages")) return -1;
    if (record && ensure_rings(*r, g.stream, true)) return -1;
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    SpeakPlanArgs p{};                  // k = 0, tiles = 0: no room lines, a block per text
    s.k = k;
    s.capacity = p.capacity = cap;
    s.record = record != 0;
    const size_t ctext_bytes = (size_t)ptext_at(2 * text_bytes, 2 * (int64_t)k);
    const size_t var_bytes = (size_t)var_at((int64_t)ctext_bytes, 2 * (int64_t)k);
    const size_t clear_bytes = record && clear ? (size_t)cap : 0;
    TellArgs so = s;                    // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const uint8_t *o_clear = nullptr, *d_clear = nullptr;
    const size_t need = layout_tell(0, (size_t)text_bytes, clear_bytes, so, po, &o_clear);
    const size_t table_bytes = (uintptr_t)so.kept[0].fresh, tables_end = (uintptr_t)so.text;
    const size_t in_bytes = (uintptr_t)so.violations + sizeof(int);
    const size_t res_at = (uintptr_t)so.violations, res_bytes = (uintptr_t)po.var + var_bytes - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (table) new_table(*r, so.room, so.slotf, table);
    if (grow_roster(*r, need)) return -1;
    layout_tell((uintptr_t)r->d, (size_t)text_bytes, clear_bytes, s, p, &d_clear);
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    uint8_t* h = r->mirror;
    const Put put{h};
    put(so.text, text, (size_t)text_bytes);
    put(so.text_off, text_off, (size_t)k * sizeof(int32_t));
    put(so.text_len, text_len, (size_t)k * sizeof(int32_t));
    put(so.slot, slots, (size_t)k * sizeof(int32_t));
    put(so.com, coms, (size_t)k);
    put(so.words, words, (size_t)k);
    int32_t* coff = reinterpret_cast<int32_t*>(h + (uintptr_t)so.ctext_off);
    for (int b = 0; b < k; b++) {
        coff[b] = (int32_t)ptext_at(text_off[b], b);
        coff[k + b] = (int32_t)ptext_at(text_bytes + text_off[b], k + b);
    }
    put(o_clear, clear, clear_bytes);
    *reinterpret_cast<int*>(h + (uintptr_t)so.violations) = 0;
    // the tables' uploads lie between the table and the inputs
    size_t first = 0, h2d = 0;
    unsigned copy_blocks = 0;
    if (pass_kept(*r, given, so.kept, s.kept, tables_end, &first, &copy_blocks)) return -1;
    if (upload(*r, table_bytes, first, in_bytes, &h2d)) return -1;

    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(nuts_roster_tell, dim3((unsigned)k + copy_blocks), dim3(kBlock), 0, st, s);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_speak_plan, dim3((unsigned)(2 * k)), dim3(kBlock), 0, st, p);
    ND_CHECK(hipGetLastError());
    // on the arrays nuts_roster_tell wrote
    if (record && launch_record(*r, k, s.ctext, s.ctext_off, s.clen, s.ring, s.flags, clear_bytes ? d_clear : nullptr, true))
        return -1;
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, res_at};
    const int violations = *reinterpret_cast<const int*>(res(so.violations));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d text(s) exceeded the hard bounds (inpstr + %d bytes composed; 6*len+4 bytes, "
                 "%d writes transduced)", violations, kTellSlack, kMaxWrites);
        return -1;
    }
    memcpy(outcome, res(so.outcome), (size_t)k);
    memcpy(target, res(so.target), (size_t)k * sizeof(int32_t));
    memcpy(clen, res(so.clen), 2 * (size_t)k * sizeof(int32_t));
    memcpy(vn, res(po.vn), 4 * (size_t)k * sizeof(int64_t));
    memcpy(vw, res(po.vw), 4 * (size_t)k * sizeof(int32_t));
    memcpy(vwsz, res(po.vwsz), 4 * (size_t)k * kMaxWrites * sizeof(int32_t));
    memcpy(ctext, res(so.ctext), ctext_bytes);
    memcpy(var, res(po.var), var_bytes);

    return fill_timing(timing, t0, t1, h2d, res_bytes);
}

// Give roster `handle` room records for rooms 0 .. n - 1 (0 .. 1024); before its first nd_roster_look, which allocates
// them.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_look_rooms(int handle, int n)
{
    Roster* r = roster_at(handle);
    if (!r) return -1;
    if (n < 0 || n > kMaxLookRooms || r->kept[kKeptRooms].d) {
        snprintf(g_err, sizeof(g_err), "look rooms %d outside 0 .. %d, or the room table is already in use", n, kMaxLookRooms);
        return -1;
    }
    r->look_rooms = n;
    return 0;
}

// What look() writes for the k lookers slots[] of roster `handle` (duplicates allowed), each in a room below the roster's
// look rooms, as texts and lists.  rms[nr] are the distinct rooms of the lookers and lroom[k] each looker's room as an index
// into rms; line_off[nr + 1] gives room i its range of lines, as many as it has slots, and m_off[k + 1] looker b its
// range of members, as many as its room has slots (both from 0, not decreasing: the caller counts the slots).  table and
// speech as nd_roster_tell's; rooms is NULL when no room changed since the last nd_roster_look of this roster, else all
// of them: a 256-byte record per look room, then an 816-byte description row per look room; udesc likewise the users'
// descriptions, 32 bytes per slot (30 of description padded with zeros, then its length); the roster's first call must
// give both.  The layouts are those of the look section above.
// The texts, T = 5 nr + 3 + nl of them with nl = line_off[nr]: text 5 i + j is text j (name, description, exits, access,
// topic) of room rms[i], at 1376 i + (0, 36, 848, 1200, 1296)[j] of ctext; texts 5 nr .. 5 nr + 2 are "You can see:", "You
// are all alone here." and the newline, at 1376 nr + (0, 16, 44); text 5 nr + 3 + l is line l, at 1376 nr + 48 + 72 l.
// Outputs (host, caller-allocated): nmem[k] the members listed for looker b, their slots at members[m_off[b] ..] and
// their lines at mline[m_off[b] ..]; nline[nr] the lines composed for room i, line_off[i] onwards, and line_slot[nl] the
// slot each is of; clen[T] (-1: a line nobody took), ctext[1376 nr + 48 + 72 nl]; vn[2T], vw[2T], vwsz[2T * 16] and
// var[12 * ctext bytes + 16 T] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, two kernels (nuts_roster_look, nuts_roster_speak_plan), one download
// at the bound size, one synchronise.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_look(int handle, int k, const int32_t* slots, const int32_t* lroom, int nr, const int32_t* rms,
                   const int32_t* line_off, const int32_t* m_off, const uint8_t* table, const uint8_t* speech,
                   const uint8_t* rooms, const uint8_t* udesc, int32_t* nmem, int32_t* nline, int32_t* clen, int64_t* vn,
                   int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var, int32_t* members, int32_t* mline,
                   int32_t* line_slot, nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nrooms = r->look_rooms;
    if (k < 1 || nr < 1 || nr > k || nr > nrooms || (int64_t)k * cap >= INT32_MAX) {
        snprintf(g_err, sizeof(g_err), "%d lookers in %d rooms of %d slots and %d look rooms: need 1 <= rooms <= lookers, "
                 "k * capacity < 2^31 - 1", k, nr, cap, nrooms);
        return -1;
    }
    if (line_off[0] || m_off[0]) {
        snprintf(g_err, sizeof(g_err), "the rooms' lines and the lookers' members must start at 0");
        return -1;
    }
    for (int b = 0; b < k; b++)          // the kernels index by these: nothing out of range reaches them
        if (slots[b] < 0 || slots[b] >= cap || lroom[b] < 0 || lroom[b] >= nr || m_off[b + 1] < m_off[b]) {
            snprintf(g_err, sizeof(g_err), "look %d: slot, room or members out of range", b);
            return -1;
        }
    for (int i = 0; i < nr; i++)
        if (rms[i] < 0 || rms[i] >= nrooms || line_off[i + 1] < line_off[i] || line_off[i + 1] > cap * (i + 1)) {
            snprintf(g_err, sizeof(g_err), "room %d of the call: no look room (0 .. %d), or its lines out of range", rms[i], nrooms - 1);
            return -1;
        }
    LookArgs s{};
    const Given given[] = {{kKeptSpeech, speech, &s.speech}, {kKeptRooms, rooms, &s.rooms}, {kKeptUdesc, udesc, &s.udesc}};
    if (check_given(*r, given, "the roster's first look call must give the speaker table, the room table and the descriptions")) return -1;
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    SpeakPlanArgs p{};                  // k = 0, tiles = 0: no room lines, a block per text
    s.k = k;
    s.nr = nr;
    s.capacity = p.capacity = cap;
    s.look_rooms = nrooms;
    const size_t nm = (size_t)m_off[k], nl = (size_t)line_off[nr];
    const size_t texts = (size_t)kLookTexts * nr + kLookFixed + nl, ctext_bytes = (size_t)look_ctext_bytes(nr, (int64_t)nl);
    const size_t var_bytes = (size_t)var_at((int64_t)ctext_bytes, (int64_t)texts);
    LookArgs so = s;                    // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const size_t need = layout_look(0, nm, nl, so, po);
    const size_t table_bytes = (uintptr_t)so.kept[0].fresh, tables_end = (uintptr_t)so.slot;
    const size_t in_bytes = (uintptr_t)so.violations + sizeof(int);
    const size_t res_at = (uintptr_t)so.violations, res_bytes = (uintptr_t)po.var + var_bytes - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (table) new_table(*r, so.room, po.slot, table);
    const int32_t* room_of = reinterpret_cast<const int32_t*>(r->mirror + (uintptr_t)so.room);
    for (int b = 0; b < k; b++)
        if (room_of[slots[b]] != rms[lroom[b]]) {
            snprintf(g_err, sizeof(g_err), "look %d: the looker is in room %d, not in room %d", b, room_of[slots[b]], rms[lroom[b]]);
            return -1;
        }
    if (grow_roster(*r, need)) return -1;
    layout_look((uintptr_t)r->d, nm, nl, s, p);
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    uint8_t* h = r->mirror;
    const Put put{h};
    put(so.slot, slots, (size_t)k * sizeof(int32_t));
    put(so.lroom, lroom, (size_t)k * sizeof(int32_t));
    put(so.rms, rms, (size_t)nr * sizeof(int32_t));
    put(so.line_off, line_off, ((size_t)nr + 1) * sizeof(int32_t));
    put(so.m_off, m_off, ((size_t)k + 1) * sizeof(int32_t));
    int32_t* coff = reinterpret_cast<int32_t*>(h + (uintptr_t)so.ctext_off);
    for (int i = 0; i < nr; i++)
        for (int j = 0; j < kLookTexts; j++) coff[kLookTexts * i + j] = i * kLookTextStride + look_text_at(j);
    for (int j = 0; j < kLookFixed; j++) coff[kLookTexts * nr + j] = nr * kLookTextStride + look_fixed_at(j);
    for (size_t l = 0; l < nl; l++)
        coff[kLookTexts * nr + kLookFixed + l] = (int32_t)(nr * kLookTextStride + kLookFixedStride + l * kLineRow);
    *reinterpret_cast<int*>(h + (uintptr_t)so.violations) = 0;
    // the tables' uploads lie between the table and the inputs
    size_t first = 0, h2d = 0;
    unsigned copy_blocks = 0;
    if (pass_kept(*r, given, so.kept, s.kept, tables_end, &first, &copy_blocks)) return -1;
    if (upload(*r, table_bytes, first, in_bytes, &h2d)) return -1;

    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(nuts_roster_look, dim3((unsigned)(nr + k) + copy_blocks), dim3(kBlock), 0, st, s);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_speak_plan, dim3((unsigned)texts), dim3(kBlock), 0, st, p);
    ND_CHECK(hipGetLastError());
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, res_at};
    const int violations = *reinterpret_cast<const int*>(res(so.violations));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d text(s) exceeded the hard bounds (a room text its slot, a room its lines, a looker its "
                 "members; 6*len+4 bytes, %d writes transduced)", violations, kMaxWrites);
        return -1;
    }
    memcpy(nmem, res(so.nmem), (size_t)k * sizeof(int32_t));
    memcpy(nline, res(so.nline), (size_t)nr * sizeof(int32_t));
    memcpy(clen, res(so.clen), texts * sizeof(int32_t));
    memcpy(vn, res(po.vn), 2 * texts * sizeof(int64_t));
    memcpy(vw, res(po.vw), 2 * texts * sizeof(int32_t));
    memcpy(vwsz, res(po.vwsz), 2 * texts * kMaxWrites * sizeof(int32_t));
    memcpy(members, res(so.members), nm * sizeof(int32_t));
    memcpy(mline, res(so.mline), nm * sizeof(int32_t));
    memcpy(line_slot, res(so.line_slot), nl * sizeof(int32_t));
    memcpy(ctext, res(so.ctext), ctext_bytes);
    memcpy(var, res(po.var), var_bytes);

    return fill_timing(timing, t0, t1, h2d, res_bytes);
}

// Give roster `handle` clone records 0 .. n - 1 (0 .. 65536), all empty; before its first nd_roster_relay, which allocates
// them.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_clones(int handle, int n)
{
    Roster* r = roster_at(handle);
    if (!r) return -1;
    if (n < 0 || n > kMaxCapacity || r->kept[kKeptClones].d) {
        snprintf(g_err, sizeof(g_err), "clone records %d outside 0 .. %d, or the records are already in use", n, kMaxCapacity);
        return -1;
    }
    r->clones = n;
    return 0;
}

// nd_roster_plan (or nd_roster_plan_record) of the k broadcasts, and the clone relay of each: what the clone records
// standing in its room send to their owners (the relay section above has the rule).  The arguments up to `table` and the
// outputs bits .. var are nd_roster_plan's.  csender[k] is the clone record that is `user` of the broadcast, -1: none.
// clones is NULL when no record changed since the last nd_roster_relay of this roster, else all of them: `clones` int32
// owners (-1: empty), `clones` int32 rooms, `clones` hear bytes; names likewise the look rooms' names, 24 bytes per room (20
// of name padded with zeros, then its length); the roster's first call must give both.  The caller has checked that every
// owner is a slot and every owned record's room a look room.
// Outputs (host, caller-allocated), with CW = ceil(clones / 64): rbits[k * CW], record c of broadcast b is bit c % 64 of
// rbits[b * CW + c / 64], the bits past the records zero; rlen[k] the relay texts' lengths, -1 where nothing relays;
// rtext[text_bytes + 32 k], relay text b at text_off[b] + 32 b; rvn[2k], rvw[2k], rvwsz[2k * 16] and rvar[12 * rtext bytes +
// 16 k] as vn .. var, over the relay texts.
// Per call, whatever k, the capacity and the records: one upload, three kernels (nuts_roster_plan, nuts_roster_relay,
// nuts_roster_speak_plan over the relay texts) and nuts_roster_record after the first when recording, one download at the
// bound size, one synchronise.
static int relay_call(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                      const int32_t* text_len, const int32_t* rm, const int32_t* sender, const uint8_t* flags,
                      const int32_t* com_num, const int32_t* csender, const uint8_t* table, const uint8_t* clones,
                      const uint8_t* names, uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* var,
                      uint64_t* rbits, int32_t* rlen, int64_t* rvn, int32_t* rvw, int32_t* rvwsz, uint8_t* rtext,
                      uint8_t* rvar, nd_roster_timing* timing, bool record, const uint8_t* clear)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    if (record && ensure_rings(*r, g.stream)) return -1;
    const int cap = r->capacity, words = (cap + 63) / 64, nc = r->clones, nrooms = r->look_rooms;
    if (k < 1 || (int64_t)k * cap >= INT32_MAX || text_bytes < 0 || nc < 1 || nrooms < 1 ||
        text_bytes + (int64_t)kRelaySlack * k >= INT32_MAX) {
        snprintf(g_err, sizeof(g_err), "%d broadcasts to %d slots, %d clone records and %d look rooms: need 1 <= k * capacity < "
                 "2^31 - 1, a clone record and a look room", k, cap, nc, nrooms);
        return -1;
    }
    for (int b = 0; b < k; b++)          // the kernel indexes by these: nothing out of range reaches it
        if (csender[b] < -1 || csender[b] >= nc || text_off[b] < 0 || text_len[b] < 0 || text_off[b] + (int64_t)text_len[b] > text_bytes) {
            snprintf(g_err, sizeof(g_err), "broadcast %d: clone sender or text out of range", b);
            return -1;
        }
    RelayArgs q{};
    const Given given[] = {{kKeptNames, names, &q.names}, {kKeptClones, clones, &q.records}};
    if (check_given(*r, given, "the roster's first relay call must give the clone records and the rooms' names")) return -1;
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    PlanArgs a{};
    SpeakPlanArgs p{};                   // k = 0, tiles = 0: no room lines, a block per relay text
    a.k = q.k = k;
    a.capacity = q.capacity = p.capacity = cap;
    a.tiles = (cap + kBlock - 1) / kBlock;
    a.words = words;
    q.clones = nc;
    q.cwords = (nc + 63) / 64;
    q.look_rooms = nrooms;
    const size_t var_bytes = (size_t)var_at(text_bytes, k), rtext_bytes = (size_t)text_bytes + (size_t)kRelaySlack * k;
    const size_t rvar_bytes = (size_t)var_at((int64_t)rtext_bytes, k);
    PlanArgs o = a;                      // offsets of every array in the roster's allocation
    RelayArgs qo = q;
    SpeakPlanArgs po = p;
    const size_t clear_bytes = record && clear ? (size_t)r->review_rooms : 0;
    const uint8_t *o_clear = nullptr, *d_clear = nullptr;
    const size_t need = layout_relay(0, (size_t)text_bytes, clear_bytes, o, qo, po, &o_clear);
    const size_t table_bytes = (uintptr_t)qo.kept[0].fresh, tables_end = (uintptr_t)o.text;
    const size_t in_bytes = (uintptr_t)o.violations + sizeof(int);
    const size_t res_at = (uintptr_t)o.violations, res_bytes = (uintptr_t)po.var + rvar_bytes - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (table) new_table(*r, o.room, o.slot, table);
    if (grow_roster(*r, need)) return -1;
    layout_relay((uintptr_t)r->d, (size_t)text_bytes, clear_bytes, a, q, p, &d_clear);
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    uint8_t* h = r->mirror;
    const Put put{h};
    put(o.text, text, (size_t)text_bytes);
    put(o.text_off, text_off, (size_t)k * sizeof(int32_t));
    put(o.text_len, text_len, (size_t)k * sizeof(int32_t));
    put(o.rm, rm, (size_t)k * sizeof(int32_t));
    put(o.sender, sender, (size_t)k * sizeof(int32_t));
    put(o.flags, flags, (size_t)k);
    put(o.com_num, com_num, (size_t)k * sizeof(int32_t));
    put(qo.csender, csender, (size_t)k * sizeof(int32_t));
    int32_t* roff = reinterpret_cast<int32_t*>(h + (uintptr_t)qo.rtext_off);
    for (int b = 0; b < k; b++) roff[b] = text_off[b] + kRelaySlack * b;
    put(o_clear, clear, clear_bytes);
    *reinterpret_cast<int*>(h + (uintptr_t)o.violations) = 0;
    // the tables' uploads lie between the table and the inputs
    size_t first = 0, h2d = 0;
    unsigned copy_blocks = 0;
    if (pass_kept(*r, given, qo.kept, q.kept, tables_end, &first, &copy_blocks)) return -1;
    if (upload(*r, table_bytes, first, in_bytes, &h2d)) return -1;

    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(nuts_roster_plan, dim3((unsigned)(k * a.tiles)), dim3(kBlock), 0, st, a);
    ND_CHECK(hipGetLastError());
    if (record && launch_record(*r, k, a.text, a.text_off, a.text_len, a.rm, a.flags, clear_bytes ? d_clear : nullptr))
        return -1;
    hipLaunchKernelGGL(nuts_roster_relay, dim3((unsigned)k + copy_blocks), dim3(kBlock), 0, st, q);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_speak_plan, dim3((unsigned)k), dim3(kBlock), 0, st, p);
    ND_CHECK(hipGetLastError());
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, res_at};
    const int violations = *reinterpret_cast<const int*>(res(o.violations));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d variant(s) or relay text(s) exceeded the hard bounds (6*len+4 bytes, %d writes; a relay "
                 "text %d bytes)", violations, kMaxWrites, kArrSize - 1);
        return -1;
    }
    memcpy(vn, res(o.vn), 2 * (size_t)k * sizeof(int64_t));
    memcpy(vw, res(o.vw), 2 * (size_t)k * sizeof(int32_t));
    memcpy(vwsz, res(o.vwsz), 2 * (size_t)k * kMaxWrites * sizeof(int32_t));
    memcpy(bits, res(o.bits), (size_t)k * words * sizeof(uint64_t));
    memcpy(var, res(o.var), var_bytes);
    memcpy(rbits, res(qo.rbits), (size_t)k * q.cwords * sizeof(uint64_t));
    memcpy(rlen, res(qo.rlen), (size_t)k * sizeof(int32_t));
    memcpy(rvn, res(po.vn), 2 * (size_t)k * sizeof(int64_t));
    memcpy(rvw, res(po.vw), 2 * (size_t)k * sizeof(int32_t));
    memcpy(rvwsz, res(po.vwsz), 2 * (size_t)k * kMaxWrites * sizeof(int32_t));
    memcpy(rtext, res(qo.rtext), rtext_bytes);
    memcpy(rvar, res(po.var), rvar_bytes);

    return fill_timing(timing, t0, t1, h2d, res_bytes);
}

// The plan and the relay (relay_call above): bit 2 of flags[] is not looked at, and nothing touches the rings.
int nd_roster_relay(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                    const int32_t* text_len, const int32_t* rm, const int32_t* sender, const uint8_t* flags,
                    const int32_t* com_num, const int32_t* csender, const uint8_t* table, const uint8_t* clones,
                    const uint8_t* names, uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* var,
                    uint64_t* rbits, int32_t* rlen, int64_t* rvn, int32_t* rvw, int32_t* rvwsz, uint8_t* rtext,
                    uint8_t* rvar, nd_roster_timing* timing)
{
    return relay_call(handle, k, text, text_bytes, text_off, text_len, rm, sender, flags, com_num, csender, table, clones,
                      names, bits, vn, vw, vwsz, var, rbits, rlen, rvn, rvw, rvwsz, rtext, rvar, timing, false, nullptr);
}

// The plan, the records, then the relay (relay_call above): nd_roster_relay's arguments, and clear as
// nd_roster_plan_record's.  The roster needs review rings.
int nd_roster_relay_record(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off,
                           const int32_t* text_len, const int32_t* rm, const int32_t* sender, const uint8_t* flags,
                           const int32_t* com_num, const int32_t* csender, const uint8_t* table, const uint8_t* clones,
                           const uint8_t* names, uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* var,
                           uint64_t* rbits, int32_t* rlen, int64_t* rvn, int32_t* rvw, int32_t* rvwsz, uint8_t* rtext,
                           uint8_t* rvar, nd_roster_timing* timing, const uint8_t* clear)
{
    return relay_call(handle, k, text, text_bytes, text_off, text_len, rm, sender, flags, com_num, csender, table, clones,
                      names, bits, vn, vw, vwsz, var, rbits, rlen, rvn, rvw, rvwsz, rtext, rvar, timing, true, clear);
}

// What who(user, 0) writes for the k lookers slots[] of roster `handle` (duplicates allowed), as texts and a bitmap.  nl is
// the number of listed users, the slots with a name and no login flag, which the caller counts; each has a room below
// the roster's look rooms, or no room and an away room there.  now is time(0) and date[date_len] long_date(1), at most 79
// bytes.  table, speech, rooms and udesc as nd_roster_look's (it and this call fill the same kept tables); who is NULL when
// no last_login or away changed since the last nd_roster_who of this roster, else all of them: 8 bytes per slot, int32
// last_login and int32 away (-1: none); the roster's first call must give it.
// The texts, T = 4 + nl of them: the header of a looker at the name prompt, the header, the footer and the tail at 0, 108,
// 216 and 296 of ctext, then line l, the line of the l-th listed slot in ascending order, at 304 + 236 l.
// Outputs (host, caller-allocated): clen[T], ctext[304 + 236 nl]; line_slot[nl] the slot each line is of; shown[k * W]
// with W = max(1, ceil(nl / 32)): bit l % 32 of word l / 32 of looker b's W words is set when b is sent line l; vn[2T],
// vw[2T], vwsz[2T * 16] and var[12 * ctext bytes + 16 T] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, three kernels (nuts_roster_who, nuts_roster_who_shown,
// nuts_roster_speak_plan), one download at the bound size, one synchronise.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_who(int handle, int k, const int32_t* slots, int nl, int32_t now, const uint8_t* date, int date_len,
                  const uint8_t* table, const uint8_t* speech, const uint8_t* rooms, const uint8_t* udesc, const uint8_t* who,
                  int32_t* clen, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var, int32_t* line_slot,
                  uint32_t* shown, nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nrooms = r->look_rooms;
    if (k < 1 || (int64_t)k * cap >= INT32_MAX || nl < 0 || nl > cap || now < 0 || date_len < 0 || date_len > kWhoDateLen) {
        snprintf(g_err, sizeof(g_err), "%d lookers, %d lines of %d slots, a date of %d bytes: need k >= 1, k * capacity < 2^31 - 1, "
                 "0 <= lines <= capacity, now >= 0, at most %d bytes of date", k, nl, cap, date_len, kWhoDateLen);
        return -1;
    }
    for (int b = 0; b < k; b++)          // the kernels index by these: nothing out of range reaches them
        if (slots[b] < 0 || slots[b] >= cap) {
            snprintf(g_err, sizeof(g_err), "who %d: slot out of range", b);
            return -1;
        }
    if (!nrooms) rooms = nullptr;        // a roster without look rooms has no room table: its listed users are violations
    WhoArgs s{};
    const Given given[] = {{kKeptSpeech, speech, &s.speech}, {kKeptRooms, rooms, &s.rooms}, {kKeptUdesc, udesc, &s.udesc},
                           {kKeptWho, who, &s.who}};
    if (check_given(*r, given, "the roster's first who call must give the speaker table, the room table, the descriptions "
                               "and the who table"))
        return -1;
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    SpeakPlanArgs p{};                  // k = 0, tiles = 0: no room lines, a block per text
    s.k = k;
    s.nl = nl;
    s.capacity = p.capacity = cap;
    s.look_rooms = nrooms;
    s.words = nl > 32 ? (nl + 31) / 32 : 1;
    s.date_len = date_len;
    s.now = now;
    const size_t texts = (size_t)kWhoFixed + nl, ctext_bytes = (size_t)who_ctext_bytes(nl);
    const size_t var_bytes = (size_t)var_at((int64_t)ctext_bytes, (int64_t)texts);
    WhoArgs so = s;                     // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const size_t need = layout_who(0, so, po);
    const size_t table_bytes = (uintptr_t)so.kept[0].fresh, tables_end = (uintptr_t)so.slot;
    const size_t in_bytes = (uintptr_t)so.violations + sizeof(int);
    const size_t res_at = (uintptr_t)so.violations, res_bytes = (uintptr_t)po.var + var_bytes - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (table) new_table(*r, so.room, so.slotf, table);
    if (grow_roster(*r, need)) return -1;
    layout_who((uintptr_t)r->d, s, p);
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    uint8_t* h = r->mirror;
    const Put put{h};
    put(so.slot, slots, (size_t)k * sizeof(int32_t));
    put(so.date, date, (size_t)date_len);
    *reinterpret_cast<int*>(h + (uintptr_t)so.violations) = 0;
    // the tables' uploads lie between the table and the inputs
    size_t first = 0, h2d = 0;
    unsigned copy_blocks = 0;
    if (pass_kept(*r, given, so.kept, s.kept, tables_end, &first, &copy_blocks)) return -1;
    if (upload(*r, table_bytes, first, in_bytes, &h2d)) return -1;

    const unsigned line_blocks = (unsigned)((cap + kBlock - 1) / kBlock), tiles = nl > kBlock ? (unsigned)((nl + kBlock - 1) / kBlock) : 1u;
    ND_CHECK(hipEventRecord(g.ev0, st));
    hipLaunchKernelGGL(nuts_roster_who, dim3(line_blocks + 1 + copy_blocks), dim3(kBlock), 0, st, s);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_who_shown, dim3((unsigned)k * tiles), dim3(kBlock), 0, st, s);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_speak_plan, dim3((unsigned)texts), dim3(kBlock), 0, st, p);
    ND_CHECK(hipGetLastError());
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, res_at};
    const int violations = *reinterpret_cast<const int*>(res(so.violations));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d text(s) exceeded the hard bounds (a text its slot, a listed slot without a room record, a "
                 "count of listed slots that is not %d; 6*len+4 bytes, %d writes transduced)", violations, nl, kMaxWrites);
        return -1;
    }
    memcpy(clen, res(so.clen), texts * sizeof(int32_t));
    memcpy(line_slot, res(so.line_slot), (size_t)nl * sizeof(int32_t));
    memcpy(shown, res(so.shown), (size_t)k * s.words * sizeof(uint32_t));
    memcpy(vn, res(po.vn), 2 * texts * sizeof(int64_t));
    memcpy(vw, res(po.vw), 2 * texts * sizeof(int32_t));
    memcpy(vwsz, res(po.vwsz), 2 * texts * kMaxWrites * sizeof(int32_t));
    memcpy(ctext, res(so.ctext), ctext_bytes);
    memcpy(var, res(po.var), var_bytes);

    return fill_timing(timing, t0, t1, h2d, res_bytes);
}

// What rooms(user, show_topics) writes for the k lookers slots[] of roster `handle` (duplicates allowed), as texts.  kinds
// says what they ask for between them: bit 0 .rmst (show_topics), bit 1 .rmsn; the texts of a kind not asked for are void.
// table, speech and rooms as nd_roster_look's (it, nd_roster_who and this call fill the same kept tables); the roster needs
// look rooms, R of them.
// The texts, T = 3 + 2 R of them: the .rmst header, the .rmsn header and the tail at 0, 80 and 176 of ctext, then room r's
// .rmst line at 180 + 124 r and its .rmsn line at 180 + 124 R + 164 r; a room without a name has neither.
// Outputs (host, caller-allocated): clen[T] (-1: void), ctext[180 + 288 R]; counts[R] the users per room, the slots with a
// name, no login flag and that room; vn[2T], vw[2T], vwsz[2T * 16] and var[12 * ctext bytes + 16 T] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, three kernels (nuts_roster_rooms_count over counters zeroed on the
// stream, nuts_roster_rooms_lines, nuts_roster_speak_plan), one download at the bound size, one synchronise.  Returns 0,
// or -1 with nd_last_error() set.
int nd_roster_rooms(int handle, int k, const int32_t* slots, int kinds, const uint8_t* table, const uint8_t* speech,
                    const uint8_t* rooms, int32_t* clen, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var,
                    int32_t* counts, nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nrooms = r->look_rooms;
    if (k < 1 || nrooms < 1 || nrooms > kMaxLookRooms || kinds < 1 || kinds > (kRoomsTopics | kRoomsLinks)) {
        snprintf(g_err, sizeof(g_err), "%d lookers of kinds %d over %d look rooms: need k >= 1, 1 <= look rooms <= %d, kinds in 1 .. 3",
                 k, kinds, nrooms, kMaxLookRooms);
        return -1;
    }
    for (int b = 0; b < k; b++)
        if (slots[b] < 0 || slots[b] >= cap) {
            snprintf(g_err, sizeof(g_err), "rooms %d: slot out of range", b);
            return -1;
        }
    RoomsArgs s{};
    const Given given[] = {{kKeptSpeech, speech, &s.speech}, {kKeptRooms, rooms, &s.rooms}};
    if (check_given(*r, given, "the roster's first rooms call must give the speaker table and the room table")) return -1;
    const double t0 = now_ns();
    hipStream_t st = g.stream;
    SpeakPlanArgs p{};                  // k = 0, tiles = 0: no room lines, a block per text
    s.k = k;
    s.capacity = p.capacity = cap;
    s.look_rooms = nrooms;
    s.kinds = kinds;
    const size_t texts = (size_t)kRoomsFixed + 2 * (size_t)nrooms, ctext_bytes = (size_t)rooms_ctext_bytes(nrooms);
    const size_t var_bytes = (size_t)var_at((int64_t)ctext_bytes, (int64_t)texts);
    RoomsArgs so = s;                   // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const size_t need = layout_rooms(0, so, po);
    const size_t table_bytes = (uintptr_t)so.kept[0].fresh, tables_end = (uintptr_t)so.slot;
    const size_t in_bytes = (uintptr_t)so.violations + sizeof(int);
    const size_t res_at = (uintptr_t)so.violations, res_bytes = (uintptr_t)po.var + var_bytes - res_at;
    if (grow_mirror(*r, in_bytes, table_bytes)) return -1;
    if (table) new_table(*r, so.room, so.slotf, table);
    if (grow_roster(*r, need)) return -1;
    layout_rooms((uintptr_t)r->d, s, p);
    if (grow_host(&gm.res, &gm.cap_res, res_bytes, "pinned results")) return -1;

    uint8_t* h = r->mirror;
    const Put put{h};
    put(so.slot, slots, (size_t)k * sizeof(int32_t));
    *reinterpret_cast<int*>(h + (uintptr_t)so.violations) = 0;
    // the tables' uploads lie between the table and the inputs
    size_t first = 0, h2d = 0;
    unsigned copy_blocks = 0;
    if (pass_kept(*r, given, so.kept, s.kept, tables_end, &first, &copy_blocks)) return -1;
    if (upload(*r, table_bytes, first, in_bytes, &h2d)) return -1;

    const unsigned count_blocks = (unsigned)((cap + kBlock - 1) / kBlock), line_blocks = (unsigned)((nrooms + kBlock - 1) / kBlock);
    ND_CHECK(hipEventRecord(g.ev0, st));
    ND_CHECK(hipMemsetAsync(s.counters, 0, (size_t)nrooms * sizeof(int32_t), st));
    hipLaunchKernelGGL(nuts_roster_rooms_count, dim3(count_blocks + copy_blocks), dim3(kBlock), 0, st, s);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_rooms_lines, dim3(line_blocks + 1), dim3(kBlock), 0, st, s);
    ND_CHECK(hipGetLastError());
    hipLaunchKernelGGL(nuts_roster_speak_plan, dim3((unsigned)texts), dim3(kBlock), 0, st, p);
    ND_CHECK(hipGetLastError());
    if (fetch_results(r->d, res_at, res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, res_at};
    const int violations = *reinterpret_cast<const int*>(res(so.violations));
    if (violations) {
        snprintf(g_err, sizeof(g_err), "%d text(s) exceeded the hard bounds (a text its slot; 6*len+4 bytes, %d writes transduced)",
                 violations, kMaxWrites);
        return -1;
    }
    memcpy(clen, res(so.clen), texts * sizeof(int32_t));
    memcpy(counts, res(so.counts), (size_t)nrooms * sizeof(int32_t));
    memcpy(vn, res(po.vn), 2 * texts * sizeof(int64_t));
    memcpy(vw, res(po.vw), 2 * texts * sizeof(int32_t));
    memcpy(vwsz, res(po.vwsz), 2 * texts * kMaxWrites * sizeof(int32_t));
    memcpy(ctext, res(so.ctext), ctext_bytes);
    memcpy(var, res(po.var), var_bytes);

    return fill_timing(timing, t0, t1, h2d, res_bytes);
}

// K .go events of roster `handle`, decided and composed as go() and move_user() do, against the tables as they are: nothing
// the roster keeps is changed, the caller applies the moves.  Event b: the mover's slot slots[b], which stands in a look
// room, inpstr and words[b] as nd_roster_tell's.  gatecrash_level (0 .. 4) and min_private_users (>= 0) are the talker's.
// table, speech and rooms as nd_roster_look's, clones as nd_roster_relay's (NULL for a roster without clone records); go is
// NULL when no go row changed since the last nd_roster_go of this roster, else all of them: 88 bytes per slot, in_phrase[40],
// its length, out_phrase[40], its length, two zeros, int32 invite_room (-1: none); the roster's first call must give it.
// Outputs (host, caller-allocated), with W = ceil(capacity / 64) and text t = b for event b's enter line, k + b its leave
// line, 2k + b its reset line, 3k + b its reply: outcome[k] (0 walked, 1 teleported, 2 unseen, 3 where, 4 netlink, 5 no room,
// 6 already, 7 not adjoined, 8 private, 9 deferred); target[k] the room the word resolved to, or -1; old_room[k];
// returned[k] 1 when the old room returns to public; clen[4k], -1 where there is no text; ctext[232 k], the enter lines at
// 60 b, the leave lines at 60 k + 84 b, the reset lines at 144 k + 36 b, the replies at 180 k + 52 b; bits[3k * W] the admit
// bitmaps of the enter, leave and reset lines; vn[8k], vw[8k], vwsz[8k * 16] and var[12 * 232 k + 64 k] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, three kernels (nuts_roster_go, nuts_roster_go_order,
// nuts_roster_speak_plan), one download at the bound size, one synchronise.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_go(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off, const int32_t* text_len,
                 const int32_t* slots, const uint8_t* words, int gatecrash_level, int min_private_users, const uint8_t* table,
                 const uint8_t* speech, const uint8_t* clones, const uint8_t* rooms, const uint8_t* go, int8_t* outcome,
                 int32_t* target, int32_t* old_room, uint8_t* returned, int32_t* clen, uint64_t* bits, int64_t* vn, int32_t* vw,
                 int32_t* vwsz, uint8_t* ctext, uint8_t* var, nd_roster_timing* timing)
{
    static_assert(kGoMaxSlots == kMaxCapacity, "nuts_roster_go_order has a bit per slot");
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nrooms = r->look_rooms;
    if (!events_fit(k, cap, 1, kGoRow, text_bytes, nrooms) || nrooms < 1 || gatecrash_level < 0 || gatecrash_level > kGod ||
        min_private_users < 0) {
        snprintf(g_err, sizeof(g_err), "%d events to %d slots over %d look rooms: need 1 <= k * capacity < 2^31 - 1, a look room, a "
                 "gatecrash level in 0 .. %d and a minimum of private users >= 0", k, cap, nrooms, kGod);
        return -1;
    }
    if (check_events(k, cap, slots, text_off, text_len, text_bytes, nullptr, [](int) { return true; })) return -1;
    GoArgs s{};
    const Given given[] = {{kKeptSpeech, speech, &s.speech}, {kKeptClones, clones, &s.records}, {kKeptRooms, rooms, &s.rooms},
                           {kKeptGo, go, &s.go}};
    if (check_given(*r, given, "the roster's first go call must give the speaker table, the clone records, the room table and the go table"))
        return -1;
    const double t0 = now_ns();
    SpeakPlanArgs p{};
    size_events(s, p, k, 3, cap);
    s.look_rooms = nrooms;
    s.clones = r->clones;
    s.gatecrash_level = gatecrash_level;
    s.min_private_users = min_private_users;
    GoArgs so = s;                      // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const size_t need = layout_go(0, (size_t)text_bytes, so, po);
    const EventSizes z = event_sizes(so, po, so.kept[0].fresh, kGoTexts, (size_t)kGoRow * k);
    if (take_given_table(*r, so, z, table) || check_rooms_of(*r, so, slots, "mover") || grow_roster(*r, need)) return -1;
    layout_go((uintptr_t)r->d, (size_t)text_bytes, s, p);
    if (grow_host(&gm.res, &gm.cap_res, z.res_bytes, "pinned results")) return -1;

    put_events(*r, so, z, text, text_bytes, text_off, text_len, slots, words, [k](int kind, int b) { return go_text_at(kind, b, k); });
    size_t h2d = 0;
    unsigned copy_blocks = 0;
    if (upload_events(*r, given, so.kept, s.kept, z, &h2d, &copy_blocks)) return -1;

    const GoOrderArgs order{s.slot, s.old_room, s.target, k, s.outcome, s.clen, s.returned};
    if (launch_events(nuts_roster_go, (unsigned)k + copy_blocks, s, nuts_roster_go_order, order, p, z)) return -1;
    if (fetch_results(r->d, z.res_at, z.res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, z.res_at};
    if (copy_event_results(res, so, po, z, outcome, clen, bits, vn, vw, vwsz, ctext, var)) return -1;
    memcpy(target, res(so.target), (size_t)k * sizeof(int32_t));
    memcpy(old_room, res(so.old_room), (size_t)k * sizeof(int32_t));
    memcpy(returned, res(so.returned), (size_t)k);
    return fill_timing(timing, t0, t1, h2d, z.res_bytes);
}

// K .public / .private / .letmein / .invite events of roster `handle`, decided and composed as set_room_access(), letmein()
// and invite() do, against the tables as they are: nothing the roster keeps is changed, the caller sets the access and the
// invitations.  Event b: the actor's slot slots[b], which stands in a look room, coms[b] (16 .. 19), inpstr and words[b] as
// nd_roster_go's.  gatecrash_level (0 .. 4), min_private_users (>= 0) and ignore_mp_level (0 .. 5) are the talker's.  The five
// tables are nd_roster_go's, NULL when unchanged since this roster's last call that took them.
// Outputs (host, caller-allocated), with W = ceil(capacity / 64) and text t = b for event b's here line, k + b its there
// line, 2k + b its reply, 3k + b its notice: outcome[k] (0 set private, 1 set public, 2 invited, 3 asked, 4 .. 20 the
// refusals in the order of kAccLowLevel .. kAccInviteAlready, 21 deferred); target_room[k] and target_slot[k], or -1;
// clen[4k], -1 where there is no text; ctext[260 k], the here lines at 72 b, the there lines at 72 k + 44 b, the replies at
// 116 k + 84 b, the notices at 200 k + 60 b; bits[2k * W] the admit bitmaps of the here and the there lines; vn[8k], vw[8k],
// vwsz[8k * 16] and var[12 * 260 k + 64 k] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, three kernels (nuts_roster_access, nuts_roster_access_order,
// nuts_roster_speak_plan), one download at the bound size, one synchronise.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_access(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off, const int32_t* text_len,
                     const int32_t* slots, const uint8_t* coms, const uint8_t* words, int gatecrash_level, int min_private_users,
                     int ignore_mp_level, const uint8_t* table, const uint8_t* speech, const uint8_t* clones, const uint8_t* rooms,
                     const uint8_t* go, int8_t* outcome, int32_t* target_room, int32_t* target_slot, int32_t* clen, uint64_t* bits,
                     int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var, nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nrooms = r->look_rooms;
    if (!events_fit(k, cap, 1, kAccRow, text_bytes, nrooms) || nrooms < 1 || gatecrash_level < 0 || gatecrash_level > kGod ||
        min_private_users < 0 || ignore_mp_level < 0 || ignore_mp_level > kGod + 1) {
        snprintf(g_err, sizeof(g_err), "%d events to %d slots over %d look rooms: need 1 <= k * capacity < 2^31 - 1, a look room, a "
                 "gatecrash level in 0 .. %d, a minimum of private users >= 0 and an ignore level in 0 .. %d", k, cap, nrooms, kGod, kGod + 1);
        return -1;
    }
    if (check_events(k, cap, slots, text_off, text_len, text_bytes, coms, [](int c) { return c >= kComPublic && c <= kComInvite; }))
        return -1;
    AccessArgs s{};
    const Given given[] = {{kKeptSpeech, speech, &s.speech}, {kKeptClones, clones, &s.records}, {kKeptGo, go, &s.go},
                           {kKeptRooms, rooms, &s.rooms}};
    if (check_given(*r, given, "the roster's first access call must give the speaker table, the clone records, the room table and the go table"))
        return -1;
    const double t0 = now_ns();
    SpeakPlanArgs p{};
    size_events(s, p, k, 2, cap);
    s.look_rooms = nrooms;
    s.clones = r->clones;
    s.gatecrash_level = gatecrash_level;
    s.min_private_users = min_private_users;
    s.ignore_mp_level = ignore_mp_level;
    AccessArgs so = s;                  // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const size_t need = layout_access(0, (size_t)text_bytes, so, po);
    const EventSizes z = event_sizes(so, po, so.kept[0].fresh, kAccTexts, (size_t)kAccRow * k);
    if (take_given_table(*r, so, z, table) || check_rooms_of(*r, so, slots, "actor") || grow_roster(*r, need)) return -1;
    layout_access((uintptr_t)r->d, (size_t)text_bytes, s, p);
    if (grow_host(&gm.res, &gm.cap_res, z.res_bytes, "pinned results")) return -1;

    put_events(*r, so, z, text, text_bytes, text_off, text_len, slots, words, [k](int kind, int b) { return acc_text_at(kind, b, k); });
    Put{r->mirror}(so.com, coms, (size_t)k);
    size_t h2d = 0;
    unsigned copy_blocks = 0;
    if (upload_events(*r, given, so.kept, s.kept, z, &h2d, &copy_blocks)) return -1;

    const AccessOrderArgs order{s.room, s.slot, s.target_room, s.target_slot, k, s.outcome, s.clen};
    if (launch_events(nuts_roster_access, (unsigned)k + copy_blocks, s, nuts_roster_access_order, order, p, z)) return -1;
    if (fetch_results(r->d, z.res_at, z.res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, z.res_at};
    if (copy_event_results(res, so, po, z, outcome, clen, bits, vn, vw, vwsz, ctext, var)) return -1;
    memcpy(target_room, res(so.target_room), (size_t)k * sizeof(int32_t));
    memcpy(target_slot, res(so.target_slot), (size_t)k * sizeof(int32_t));
    return fill_timing(timing, t0, t1, h2d, z.res_bytes);
}

// K .clone / .destroy / .csay / .chear events of roster `handle`, decided and composed as create_clone(), destroy_clone(),
// clone_say() and clone_hear() do, against the tables as they are: nothing the roster keeps is changed but the rings of a
// recording call, the caller creates, destroys and sets the records.  Event b: the actor's slot slots[b], which stands in a
// look room, coms[b] (73, 74, 78 or 79), inpstr and words[b] as nd_roster_go's.  gatecrash_level (0 .. 4), min_private_users
// (>= 0) and max_clones (>= 0) are the talker's.  record: store the said lines in their rooms' rings, after clearing those
// that clear marks (NULL: none), as nd_roster_speak does; the caller has checked that every look room is a ring room.  The
// five tables are nd_roster_go's, NULL when unchanged since this roster's last call that took them; the roster has clone
// records.
// Outputs (host, caller-allocated), with W = ceil(capacity / 64) and text t = kind * k + b for event b's here line (kind
// 0), there line, reset line, said line, reply and notice (kind 5): outcome[k] (0 .. 2 the clone_hear value set, 3 created, 4
// destroyed, 5 said, 6 .. 21 the refusals in the order of kCloneNoRoom .. kCloneChearNone, 22 deferred); target_room[k] and
// target_slot[k], or -1; rec[k] the record found or destroyed, or -1; reset[k] 1 where the room returns to public; clen[6k],
// -1 where there is no text; ctext[324 k + text_bytes + 36 k], the here lines at 48 b, the there lines at 48 k + 68 b, the
// reset lines at 116 k + 36 b, the said lines at 152 k + text_off[b] + 36 b, the replies at 188 k + text_bytes + 88 b, the
// notices at 276 k + text_bytes + 84 b; bits[4k * W] the admit bitmaps of the four room lines; vn[12k], vw[12k], vwsz[12k *
// 16] and var[12 * ctext bytes + 96 k] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, three kernels (nuts_roster_clone, nuts_roster_clone_order,
// nuts_roster_speak_plan) and nuts_roster_record as a fourth when record is set, one download at the bound size, one
// synchronise.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_clone(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off, const int32_t* text_len,
                    const int32_t* slots, const uint8_t* coms, const uint8_t* words, int gatecrash_level, int min_private_users,
                    int max_clones, int record, const uint8_t* table, const uint8_t* speech, const uint8_t* clones, const uint8_t* rooms,
                    const uint8_t* go, const uint8_t* clear, int8_t* outcome, int32_t* target_room, int32_t* target_slot, int32_t* rec,
                    uint8_t* reset, int32_t* clen, uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var,
                    nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nrooms = r->look_rooms;
    if (!events_fit(k, cap, kCloneLines, kCloneRow, text_bytes, nrooms) || nrooms < 1 || r->clones < 1 || cap > kGoMaxSlots ||
        gatecrash_level < 0 || gatecrash_level > kGod || min_private_users < 0 || max_clones < 0) {
        snprintf(g_err, sizeof(g_err), "%d events to %d slots over %d look rooms and %d clone records: need 1 <= 4 k * capacity < 2^31 - 1, "
                 "a look room, a clone record, a gatecrash level in 0 .. %d, a minimum of private users >= 0 and a maximum of clones >= 0",
                 k, cap, nrooms, r->clones, kGod);
        return -1;
    }
    if (check_events(k, cap, slots, text_off, text_len, text_bytes, coms,
                     [](int c) { return c == kComClone || c == kComDestroy || c == kComCsay || c == kComChear; }))
        return -1;
    CloneArgs s{};
    const Given given[] = {{kKeptSpeech, speech, &s.speech}, {kKeptGo, go, &s.go}, {kKeptRooms, rooms, &s.rooms},
                           {kKeptClones, clones, &s.records}};
    if (check_given(*r, given, "the roster's first clone call must give the speaker table, the go table, the room table and the clone records"))
        return -1;
    if (record && (r->review_rooms < nrooms || ensure_rings(*r, g.stream))) {
        if (r->review_rooms < nrooms) snprintf(g_err, sizeof(g_err), "a recording clone call needs a review ring for every look room");
        return -1;
    }
    const double t0 = now_ns();
    SpeakPlanArgs p{};
    size_events(s, p, k, kCloneLines, cap);
    s.look_rooms = nrooms;
    s.clones = r->clones;
    s.gatecrash_level = gatecrash_level;
    s.min_private_users = min_private_users;
    s.max_clones = max_clones;
    s.record = record != 0;
    const size_t clear_bytes = record && clear ? (size_t)r->review_rooms : 0;
    CloneArgs so = s;                   // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const uint8_t *o_clear = nullptr, *d_clear = nullptr;
    const size_t need = layout_clone(0, (size_t)text_bytes, clear_bytes, so, po, &o_clear);
    const EventSizes z = event_sizes(so, po, so.kept[0].fresh, kCloneTexts, (size_t)clone_text_bytes(k, text_bytes));
    if (take_given_table(*r, so, z, table) || check_rooms_of(*r, so, slots, "actor") || grow_roster(*r, need)) return -1;
    layout_clone((uintptr_t)r->d, (size_t)text_bytes, clear_bytes, s, p, &d_clear);
    if (grow_host(&gm.res, &gm.cap_res, z.res_bytes, "pinned results")) return -1;

    put_events(*r, so, z, text, text_bytes, text_off, text_len, slots, words,
               [=](int kind, int b) { return clone_text_at(kind, b, k, text_off[b], text_bytes); });
    const Put put{r->mirror};
    put(so.com, coms, (size_t)k);
    put(o_clear, clear, clear_bytes);
    size_t h2d = 0;
    unsigned copy_blocks = 0;
    if (upload_events(*r, given, so.kept, s.kept, z, &h2d, &copy_blocks)) return -1;

    const CloneOrderArgs order{s.slot, s.found, s.found + k, k, s.outcome, s.clen, s.reset, s.flags};
    if (launch_events(nuts_roster_clone, (unsigned)k + copy_blocks, s, nuts_roster_clone_order, order, p, z)) return -1;
    // on the said lines nuts_roster_clone wrote, less those nuts_roster_clone_order deferred
    if (record && launch_record(*r, k, s.ctext, s.ctext_off + (size_t)kCloneSaidText * k, s.clen + (size_t)kCloneSaidText * k,
                                s.line + (size_t)kCloneSaidText * k, s.flags, clear_bytes ? d_clear : nullptr))
        return -1;
    if (fetch_results(r->d, z.res_at, z.res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, z.res_at};
    if (copy_event_results(res, so, po, z, outcome, clen, bits, vn, vw, vwsz, ctext, var)) return -1;
    memcpy(reset, res(so.reset), (size_t)k);
    const int32_t* found = reinterpret_cast<const int32_t*>(res(so.found));
    memcpy(target_room, found, (size_t)k * sizeof(int32_t));
    memcpy(target_slot, found + k, (size_t)k * sizeof(int32_t));
    memcpy(rec, found + 2 * (size_t)k, (size_t)k * sizeof(int32_t));
    return fill_timing(timing, t0, t1, h2d, z.res_bytes);
}

// K .move / .wake / .muzzle / .unmuzzle events of roster `handle`, decided and composed as move(), wake(), muzzle(), unmuzzle()
// and move_user(u, rm, 2) do, against the tables as they are: nothing the roster keeps is changed, the caller moves the
// targets and sets their muzzles.  Event b: the actor's slot slots[b], which stands in a look room, coms[b] (21, 58, 60 or
// 61), inpstr and words[b] as nd_roster_go's.  gatecrash_level (0 .. 4) and min_private_users (>= 0) are the talker's.  The
// five tables are nd_roster_go's, NULL when unchanged since this roster's last call that took them; byte 15 of a slot's
// speaker state is its muzzle level.
// Outputs (host, caller-allocated), with W = ceil(capacity / 64) and text t = kind * k + b for event b's here line (kind
// 0), enter line, leave line, reset line, reply and notice (kind 5): outcome[k] (0 moved, 1 moved unseen, 2 muzzled, 3
// unmuzzled, 4 woken, 5 .. 27 the refusals in the order of kActMoveUsage .. kActUnmuzzleAbove, 28 deferred); target_slot[k]
// the slot get_user found, target_room[k] the room the event is about and old_room[k] the found slot's room, or -1;
// returned[k] 1 where the room left returns to public; clen[6k], -1 where there is no text; ctext[376 k], the here lines at
// 48 b, the enter lines at 48 k + 56 b, the leave lines at 104 k + 80 b, the reset lines at 184 k + 36 b, the replies at
// 220 k + 84 b, the notices at 304 k + 72 b; bits[4k * W] the admit bitmaps of the four room lines; vn[12k], vw[12k],
// vwsz[12k * 16] and var[12 * 376 k + 96 k] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, three kernels (nuts_roster_act, nuts_roster_act_order,
// nuts_roster_speak_plan), one download at the bound size, one synchronise.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_act(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off, const int32_t* text_len,
                  const int32_t* slots, const uint8_t* coms, const uint8_t* words, int gatecrash_level, int min_private_users,
                  const uint8_t* table, const uint8_t* speech, const uint8_t* clones, const uint8_t* rooms, const uint8_t* go,
                  int8_t* outcome, int32_t* target_slot, int32_t* target_room, int32_t* old_room, uint8_t* returned, int32_t* clen,
                  uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var, nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nrooms = r->look_rooms;
    if (!events_fit(k, cap, 1, kActRow, text_bytes, nrooms) || nrooms < 1 || cap > kGoMaxSlots || gatecrash_level < 0 ||
        gatecrash_level > kGod || min_private_users < 0) {
        snprintf(g_err, sizeof(g_err), "%d events to %d slots over %d look rooms: need 1 <= k * capacity < 2^31 - 1, a look room, a "
                 "gatecrash level in 0 .. %d and a minimum of private users >= 0", k, cap, nrooms, kGod);
        return -1;
    }
    if (check_events(k, cap, slots, text_off, text_len, text_bytes, coms,
                     [](int c) { return c == kComMove || c == kComWake || c == kComMuzzle || c == kComUnmuzzle; }))
        return -1;
    ActArgs s{};
    const Given given[] = {{kKeptClones, clones, &s.records}, {kKeptRooms, rooms, &s.rooms}, {kKeptGo, go, &s.go},
                           {kKeptSpeech, speech, &s.speech}};
    if (check_given(*r, given, "the roster's first act call must give the speaker table, the clone records, the room table and the go table"))
        return -1;
    const double t0 = now_ns();
    SpeakPlanArgs p{};
    size_events(s, p, k, kActLines, cap);
    s.look_rooms = nrooms;
    s.clones = r->clones;
    s.gatecrash_level = gatecrash_level;
    s.min_private_users = min_private_users;
    ActArgs so = s;                     // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const size_t need = layout_act(0, (size_t)text_bytes, so, po);
    const EventSizes z = event_sizes(so, po, so.kept[0].fresh, kActTexts, (size_t)kActRow * k);
    if (take_given_table(*r, so, z, table) || check_rooms_of(*r, so, slots, "actor") || grow_roster(*r, need)) return -1;
    layout_act((uintptr_t)r->d, (size_t)text_bytes, s, p);
    if (grow_host(&gm.res, &gm.cap_res, z.res_bytes, "pinned results")) return -1;

    put_events(*r, so, z, text, text_bytes, text_off, text_len, slots, words, [k](int kind, int b) { return act_text_at(kind, b, k); });
    Put{r->mirror}(so.com, coms, (size_t)k);
    size_t h2d = 0;
    unsigned copy_blocks = 0;
    if (upload_events(*r, given, so.kept, s.kept, z, &h2d, &copy_blocks)) return -1;

    const ActOrderArgs order{s.room, s.slot, s.found, k, s.outcome, s.clen, s.returned};
    if (launch_events(nuts_roster_act, (unsigned)k + copy_blocks, s, nuts_roster_act_order, order, p, z)) return -1;
    if (fetch_results(r->d, z.res_at, z.res_bytes)) return -1;
    const double t1 = now_ns();

    const Res res{gm.res, z.res_at};
    if (copy_event_results(res, so, po, z, outcome, clen, bits, vn, vw, vwsz, ctext, var)) return -1;
    memcpy(returned, res(so.returned), (size_t)k);
    const int32_t* found = reinterpret_cast<const int32_t*>(res(so.found));
    memcpy(target_slot, found, (size_t)k * sizeof(int32_t));
    memcpy(target_room, found + k, (size_t)k * sizeof(int32_t));
    memcpy(old_room, found + 2 * (size_t)k, (size_t)k * sizeof(int32_t));
    return fill_timing(timing, t0, t1, h2d, z.res_bytes);
}

// K events of roster `handle` by which a user sets its own state -- .mode, .ignall, .prompt, .desc, .inphr, .outphr, .topic,
// .vis, .invis, .charecho, .afk, .colour, .ignshout, .igntell -- decided and composed as the reference's functions do (the
// section of nuts_roster_set lists them), against the tables as they are: nothing the roster keeps is changed, the caller
// applies the result.  Event b: the actor's slot slots[b], which has a room, coms[b] (one of the fourteen), inpstr and
// words[b] as nd_roster_go's.  The actor of a .topic stands in a look room.  The six tables are NULL when unchanged since this
// roster's last call that took them; rooms is read, and asked for, only by a call that holds a .topic.
// Outputs (host, caller-allocated), with W = ceil(capacity / 64) and text t = b for event b's here line, k + b its reply,
// 2k + b its second reply: outcome[k] (0 .. 21 the effective outcomes in the order of kSetModeCommand .. kSetIgntellOff,
// 22 .. 34 the video test, the queries and the refusals, 35 deferred); clen[3k], -1 where there is no text; ctext[200 k], the
// here lines at 96 b, the replies at 96 k + 84 b, the second replies at 180 k + 20 b; bits[k * W] the admit bitmaps of the
// here lines; vn[6k], vw[6k], vwsz[6k * 16] and var[12 * 200 k + 48 k] as nd_roster_speak's.
// Per call, whatever k and the capacity: one upload, three kernels (nuts_roster_set, nuts_roster_set_order,
// nuts_roster_speak_plan), one download at the bound size, one synchronise.  Returns 0, or -1 with nd_last_error() set.
int nd_roster_set(int handle, int k, const uint8_t* text, int64_t text_bytes, const int32_t* text_off, const int32_t* text_len,
                  const int32_t* slots, const uint8_t* coms, const uint8_t* words, const uint8_t* table, const uint8_t* speech,
                  const uint8_t* afk, const uint8_t* udesc, const uint8_t* go, const uint8_t* rooms, int8_t* outcome, int32_t* clen,
                  uint64_t* bits, int64_t* vn, int32_t* vw, int32_t* vwsz, uint8_t* ctext, uint8_t* var, nd_roster_timing* timing)
{
    Roster* r = roster_at(handle);
    if (!r || ensure_ready()) return -1;
    const int cap = r->capacity, nrooms = r->look_rooms;
    if (!events_fit(k, cap, 1, kSetRow, text_bytes, nrooms) || nrooms < 0) {
        snprintf(g_err, sizeof(g_err), "%d events to %d slots: need 1 <= k * capacity < 2^31 - 1", k, cap);
        return -1;
    }
    if (check_events(k, cap, slots, text_off, text_len, text_bytes, coms, [](int c) {
            return c == kComMode || (c >= kComIgnall && c <= kComOutphr) || c == kComTopic || c == kComVis || c == kComInvis ||
                   c == kComCharecho || c == kComAfk || (c >= kComColour && c <= kComIgntell);
        }))
        return -1;
    const bool topics = std::find(coms, coms + k, (uint8_t)kComTopic) != coms + k;
    SetArgs s{};
    const Given given[] = {{kKeptRooms, topics ? rooms : nullptr, &s.rooms, !topics}, {kKeptGo, go, &s.go}, {kKeptAfk, afk, &s.afk},
                           {kKeptUdesc, udesc, &s.udesc}, {kKeptSpeech, speech, &s.speech}};
    if (check_given(*r, given, "the roster's first set call must give the go table, the AFK messages, the user descriptions, the speaker "
                               "table and, for a .topic, the room table"))
        return -1;
    const double t0 = now_ns();
    SpeakPlanArgs p{};
    size_events(s, p, k, 1, cap);
    s.blocks = (k + kBlock / 64 - 1) / (kBlock / 64);
    SetArgs so = s;                     // offsets of every array in the roster's allocation
    SpeakPlanArgs po = p;
    const size_t need = layout_set(0, (size_t)text_bytes, nrooms, so, po);
    const EventSizes z = event_sizes(so, po, so.kept[0].fresh, kSetTexts, (size_t)kSetRow * k);
    if (take_given_table(*r, so, z, table)) return -1;
    uint8_t* h = r->mirror;
    const int32_t* room = reinterpret_cast<const int32_t*>(h + (uintptr_t)so.room);
    int32_t* rid = reinterpret_cast<int32_t*>(h + (uintptr_t)so.rid);
    for (int b = 0; b < k; b++) {       // every actor has a room, and a .topic's a record: nuts_roster_set reads it
        rid[b] = room[slots[b]];
        if (rid[b] < 0 || (coms[b] == kComTopic && rid[b] >= nrooms)) {
            snprintf(g_err, sizeof(g_err), "event %d: the actor has no room, or a .topic's room has no room record", b);
            return -1;
        }
    }
    if (grow_roster(*r, need)) return -1;
    layout_set((uintptr_t)r->d, (size_t)text_bytes, nrooms, s, p);
    if (grow_host(&gm.res, &gm.cap_res, z.res_bytes, "pinned results")) return -1;

    put_events(*r, so, z, text, text_bytes, text_off, text_len, slots, words, [k](int kind, int b) { return set_text_at(kind, b, k); });
    Put{h}(so.com, coms, (size_t)k);
    {                                   // the actors' rooms become their ranks among the call's rooms: fewer than 65,536, as the slots are
        int32_t* sorted = reinterpret_cast<int32_t*>(gm.res);           // scratch until the results land there: k * 4 <= res_bytes
        std::copy(rid, rid + k, sorted);
        std::sort(sorted, sorted + k);
        const int32_t* last = std::unique(sorted, sorted + k);
        for (int b = 0; b < k; b++) rid[b] = (int32_t)(std::lower_bound((const int32_t*)sorted, last, rid[b]) - sorted);
    }
    size_t h2d = 0;
    unsigned copy_blocks = 0;
    if (upload_events(*r, given, so.kept, s.kept, z, &h2d, &copy_blocks)) return -1;

    const SetOrderArgs order{s.slot, s.rid, s.com, k, s.outcome, s.clen};
    if (launch_events(nuts_roster_set, (unsigned)s.blocks + copy_blocks, s, nuts_roster_set_order, order, p, z)) return -1;
    if (fetch_results(r->d, z.res_at, z.res_bytes)) return -1;
    const double t1 = now_ns();

    if (copy_event_results(Res{gm.res, z.res_at}, so, po, z, outcome, clen, bits, vn, vw, vwsz, ctext, var)) return -1;
    return fill_timing(timing, t0, t1, h2d, z.res_bytes);
}

}  // extern "C"
