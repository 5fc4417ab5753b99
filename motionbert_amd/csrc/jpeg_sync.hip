// Huffman decoding INSIDE a restart interval, in parallel: the entropy stage for the Motion-JPEG files that have no DRI, whose frames are one
// interval each and so one lane of mbx_jpeg_dec_entropy (jpeg_dec.hip).  The self-synchronising scheme of Klein & Wiseman and of Weissenberger
// & Schmidt ("Accelerating JPEG Decompression on GPUs"), arranged so that it is exact for every input: whatever cannot be proven right is
// decoded again by the one-lane body of jpeg_dec_common.h, which defines every result.  include/mbx.h has the definitions.
//   state       (p, k, z): the raw bit position of the next symbol (counted from the interval's first byte, stuffed bytes included), the
//               block inside the MCU, the next zigzag index (0: a DC symbol comes next).  One 64-bit word: p << 16 | k << 8 | z.
//   subsequence JS_S bytes at a fixed offset from the interval's start; it owns the symbols whose first bit lies in it.  Its exit is the state
//               at the first symbol that begins at or behind its end.  A chunk is JS_CH subsequences, one workgroup, a lane each.
//   A  jpeg_sync_spec_kernel    every lane decodes its subsequence from (first bit, 0, 0), LENIENTLY (a wrong state meets impossible symbols
//                               and must go on), then rounds: lane i takes lane i - 1's exit as entry and decodes again if that differs from
//                               the entry it used.  Lane i is final after round i, so at most JS_CH rounds.  Stored: every lane's entry,
//                               exit and counts (blocks completed, sum of the DC differences per component), the chunk's exit.
//   B  jpeg_sync_verify_kernel  chunk c >= 1 gives chunk c - 1's exit AS A STORED IT to lane 0 and runs the same rounds from the stored lane
//                               states.  If every chunk of an interval reproduces the exit A stored for it, all stored exits are true ones
//                               (chunk 0 starts from the true state and the equalities chain).  Then the exclusive scan of the counts
//                               inside the chunk, through LDS.
//   S  jpeg_sync_scan_kernel    a lane per interval: the chunks' offsets, and route = 1 where a chunk did not reproduce its exit, 3 where the
//                               interval is longer than the host said, 2 where it is empty.
//   C  jpeg_sync_write_kernel   route 0 only.  Every lane decodes once more from its true entry, STRICTLY (the checks of the one-lane body),
//                               and stores the coefficients at the block index and with the DC predictors of the scan.  route = 2 where a
//                               strict check fails, where the interval's bytes end before its blocks do, or where 8 or more bits are left.
//   Z, D                        the intervals with route != 0: zeroed again, then decoded by jpeg_decode_interval, one lane each.
// No workgroup waits for another: the order between the stages is the launch boundary.  Every loop over symbols consumes at least one bit
// per trip and ends at the subsequence's end; every round loop's exit condition comes out of __syncthreads_or, so it is workgroup-uniform.
#include "jpeg_dec_common.h"

#define JS_S MBX_JPEG_SYNC_BYTES
#define JS_CH MBX_JPEG_SYNC_CHUNK
#define JS_MAX_BYTES (1ll << 27)      // bit positions inside an interval stay below 2^30 + 31
#define JS_FALL_THREADS 64

namespace {

typedef unsigned long long u64;

struct SyncWs {                       // N = n_all * max_chunks * JS_CH subsequence slots, M = n_all * max_chunks chunk slots
    uint4* cnt;                       // [N] A: a lane's own counts; B: the exclusive sums inside the chunk.  (blocks, dc0, dc1, dc2)
    uint4* ctot;                      // [M] the chunk's sums
    uint4* coff;                      // [M] the sums of the chunks before it
    u64* entry;                       // [N] the entry a lane used last
    u64* exit_;                       // [N] and the exit it found
    u64* cexit;                       // [M] the chunk's exit, written by A alone
    int* cok;                         // [M] B: the chunk reproduced it
    int* rounds;                      // [M][2] the rounds A and B took (measurement)
};
inline size_t sync_ws_bytes(long long n_all, int max_chunks) {
    const size_t M = (size_t)n_all * max_chunks, N = M * JS_CH;
    return N * 32 + M * 64;           // 16 + 16 + 8 + 4 + 8 = 52 per chunk, rounded up so that every array stays 16-byte aligned
}
inline SyncWs make_sync_ws(void* ws, long long n_all, int max_chunks) {
    const size_t M = (size_t)n_all * max_chunks, N = M * JS_CH;
    SyncWs w;
    unsigned char* p = (unsigned char*)ws;
    w.cnt = (uint4*)p; p += N * 16;
    w.ctot = (uint4*)p; p += M * 16;
    w.coff = (uint4*)p; p += M * 16;
    w.entry = (u64*)p; p += N * 8;
    w.exit_ = (u64*)p; p += N * 8;
    w.cexit = (u64*)p; p += M * 8;
    w.cok = (int*)p; p += M * 4;
    w.rounds = (int*)p;
    return w;
}
inline int sync_max_chunks(long long max_bytes) {
    const long long n_sub = (max_bytes + JS_S - 1) / JS_S, c = (n_sub + JS_CH - 1) / JS_CH;
    return (int)(c < 1 ? 1 : c);
}

struct SyncIv {                       // one interval: its bytes data[lo .. hi), its blocks and where they lie in coef
    long long lo, hi;
    unsigned total;
    size_t coef0;
};
__device__ __forceinline__ SyncIv sync_interval(const long long* __restrict__ pos, long long data_bytes, const DGeo& g, int restart, int n_int,
                                                long long t) {
    const int f = (int)(t / n_int), iv = (int)(t % n_int);
    const long long* p = pos + (size_t)f * (n_int + 1) + iv;
    SyncIv r;
    r.lo = p[0] < 0 ? 0 : p[0] > data_bytes ? data_bytes : p[0];         // the clamps of jpeg_decode_interval
    r.hi = p[1] - 2 < r.lo ? r.lo : p[1] - 2 > data_bytes ? data_bytes : p[1] - 2;
    const int per = restart ? restart : g.n_mcu;
    const long long m0 = (long long)iv * per;
    const int m1 = (int)(m0 + per < g.n_mcu ? m0 + per : g.n_mcu);
    r.total = (unsigned)((m1 - (int)m0) * g.bpm);
    r.coef0 = ((size_t)f * g.n_mcu + (size_t)m0) * g.bpm * 64;
    return r;
}

// BitReader drops the stuffed bytes as it refills, so its (at, n) do not name a place in the file.  This one remembers, for each of the
// bytes it holds, whether a stuffed byte followed it (sm), and so reports and resumes at a raw (byte, bit).  Behind the interval's end it
// reads zeros and goes on counting bytes: `at` then lies past `end` by the number of such bytes.  The reader, the lookup and the decode of a
// subsequence are __host__ __device__, so that a host program can run them under a sanitizer.
struct RawReader {
    const unsigned char* data;
    long long at, end;
    u64 acc;
    unsigned sm;
    int n;
    __host__ __device__ __forceinline__ void fill() {                            // at most 7 trips: each adds 8 bits.  Afterwards 49 <= n <= 56
        while (n <= 48) {
            unsigned b = 0u, st = 0u;
            if (at < end) {
                b = data[at];
                st = (b == 0xffu && at + 1 < end && data[at + 1] == 0u) ? 1u : 0u;
            }
            at += 1 + st;
            acc = (acc << 8) | b;
            sm = (sm << 1) | st;
            n += 8;
        }
    }
    __host__ __device__ __forceinline__ unsigned take(int k) {                   // k <= 16 <= n
        n -= k;
        return (unsigned)(acc >> n) & ((1u << k) - 1u);
    }
    __host__ __device__ __forceinline__ long long bitpos() const {               // the raw position of the next bit, always inside a byte that is data
        const int nb = (n + 7) >> 3;
        return (at - nb - __builtin_popcount(sm & ((1u << nb) - 1u))) * 8 + ((8 - (n & 7)) & 7);
    }
    __host__ __device__ __forceinline__ int real() const {                       // bits held that the interval really has; negative: read past its end
        return n - 8 * (int)(at > end ? at - end : 0);
    }
};

// the code at the head of the 16 bits w -> its length and symbol; 0 where no code matches
__host__ __device__ __forceinline__ int sync_lookup(unsigned w, const unsigned* __restrict__ t, int& sym) {
    const unsigned short* look = reinterpret_cast<const unsigned short*>(t);
    const int* maxcode = reinterpret_cast<const int*>(t + 128);
    const int* valoff = maxcode + 18;
    const unsigned char* vals = reinterpret_cast<const unsigned char*>(t + 164);
    const unsigned e = look[w >> 8];
    int len = (int)(e >> 8);
    sym = (int)(e & 255u);
    if (len < 1 || len > 8) {
        for (len = 9; len <= 16; ++len)
            if ((int)(w >> (16 - len)) <= maxcode[len]) break;
        if (len > 16) return 0;
        sym = vals[((w >> (16 - len)) + valoff[len]) & 255];
    }
    return len;
}

// One subsequence from `entry` to its exit.  Lenient (A, B): no code matches -> one bit on, state unchanged; every AC symbol (r, s) but EOB
// skips r + 1 coefficients and s bits, so that a run past 63 ends the block and (r, 0) is no error.  cnt: the blocks completed and the DC
// differences added up per component, by the symbols this subsequence owns.  STRICT (C): the checks of jpeg_decode_interval; the values are
// stored at block b0 + (blocks completed here) of the interval's `total`, the DC with the predictors `pre`; *bad is set where a check fails,
// where the lane completes the last block and 8 or more bits are left, or where the `last` subsequence ends before the last block does.
// The loop consumes at least one bit per trip and ends at end_bits: at most 8 JS_S + 31 trips.
template <bool STRICT>
__host__ __device__ __forceinline__ u64 sync_decode(const unsigned char* __restrict__ data, const SyncIv& iv, const unsigned* tab, int bpm, u64 entry,
                                           unsigned end_bits, uint4& cnt, short* __restrict__ coef, uint4 pre, bool last, bool* bad) {
    unsigned P = (unsigned)(entry >> 16);
    int k = (int)((entry >> 8) & 255u), z = (int)(entry & 255u);
    unsigned nb = 0u, d0 = 0u, d1 = 0u, d2 = 0u;
    unsigned blk = pre.x;
    bool done = STRICT && blk >= iv.total;                              // STRICT: nothing is left to store
    if (!done && P < end_bits) {
        const int ny = bpm - 2;
        RawReader r;
        r.data = data; r.at = iv.lo + (P >> 3); r.end = iv.hi; r.acc = 0; r.sm = 0; r.n = 0;
        r.fill();
        r.n -= (int)(P & 7u);
        do {
            r.fill();
            const int c = k < ny ? 0 : k - ny + 1;
            int sym;
            const int len = sync_lookup((unsigned)(r.acc >> (r.n - 16)) & 0xffffu, tab + (2 * c + (z ? 1 : 0)) * TW, sym);
            if (len == 0) {
                if (STRICT) { *bad = true; done = true; break; }
                r.n -= 1;
            } else {
                r.n -= len;
                const int s = sym & 15;
                if (z == 0) {
                    const int v = (int)r.take(s);
                    const int d = s == 0 ? 0 : v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
                    d0 += c == 0 ? (unsigned)d : 0u; d1 += c == 1 ? (unsigned)d : 0u; d2 += c == 2 ? (unsigned)d : 0u;
                    if (STRICT) coef[iv.coef0 + (size_t)blk * 64] = (short)(c == 0 ? pre.y + d0 : c == 1 ? pre.z + d1 : pre.w + d2);
                    z = 1;
                } else if (sym == 0) {
                    z = 64;
                } else if (STRICT) {
                    z += sym >> 4;
                    if (s) {
                        if (z > 63) { *bad = true; done = true; break; }
                        const int v = (int)r.take(s);
                        coef[iv.coef0 + (size_t)blk * 64 + z] = (short)(v < (1 << (s - 1)) ? v - (1 << s) + 1 : v);
                    } else if ((sym >> 4) != 15 || z > 63) { *bad = true; done = true; break; }
                    ++z;
                } else {
                    r.n -= s;
                    z += (sym >> 4) + 1;
                }
                if (STRICT && r.real() < 0) { *bad = true; done = true; break; }   // the interval ends inside the symbol
                if (z >= 64) {
                    z = 0;
                    ++nb;
                    k = k + 1 == bpm ? 0 : k + 1;
                    if (STRICT && ++blk == iv.total) {                   // this lane completes the interval: the LEFTOVER rule
                        if (r.at < r.end || r.real() >= 8) *bad = true;
                        done = true;
                        break;
                    }
                }
            }
            P = (unsigned)(r.bitpos() - iv.lo * 8);
        } while (P < end_bits);
    }
    if (STRICT && last && !done) *bad = true;                            // the bytes end before the blocks do
    cnt = make_uint4(nb, d0, d1, d2);
    return (u64)P << 16 | (u64)(unsigned)k << 8 | (u64)(unsigned)z;
}

__host__ __device__ __forceinline__ uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// What A, B and C share: the tables into LDS, then the workgroup's interval t and chunk c; false where the workgroup has nothing to do.
// Every condition is the same for all lanes of the workgroup, so a caller may return on it between barriers.
struct SyncChunk {
    SyncIv iv;
    long long t, n_sub;
    int c, j;                         // the chunk, and this lane's subsequence in the interval
    bool active;
    unsigned end_bits;
    size_t slot, cslot;
};
__device__ __forceinline__ bool sync_chunk(SyncChunk& q, const long long* __restrict__ pos, long long data_bytes, const unsigned* __restrict__ tables,
                                           unsigned* tab, const DGeo& g, int restart, int n_int, int max_chunks, long long max_bytes,
                                           const int* __restrict__ status) {
    for (int i = threadIdx.x; i < 6 * TW; i += JS_CH) tab[i] = tables[i];
    __syncthreads();
    q.t = blockIdx.x / max_chunks;
    q.c = (int)(blockIdx.x % max_chunks);
    if (status[q.t] != MBX_JPEG_DEC_OK) return false;
    q.iv = sync_interval(pos, data_bytes, g, restart, n_int, q.t);
    const long long len = q.iv.hi - q.iv.lo;
    if (len > max_bytes) return false;                                   // route 3 (S): no slot of ws belongs to its subsequences
    q.n_sub = (len + JS_S - 1) / JS_S;                                   // <= max_chunks JS_CH
    if ((long long)q.c * JS_CH >= q.n_sub) return false;
    q.j = q.c * JS_CH + (int)threadIdx.x;
    q.active = q.j < q.n_sub;
    const long long e = (long long)(q.j + 1) * JS_S;
    q.end_bits = (unsigned)((e < len ? e : len) * 8);
    q.cslot = (size_t)q.t * max_chunks + q.c;
    q.slot = (size_t)q.t * max_chunks * JS_CH + q.j;
    return true;
}

// The rounds of A and B.  ex[i]: lane i's exit.  Lane i > 0 takes ex[i - 1], lane 0 takes entry0.  The loop's condition comes out of
// __syncthreads_or, the same value in every lane; lane i cannot change after round i, so JS_CH trips are enough.  -> rounds with a change
__device__ __forceinline__ int sync_rounds(const unsigned char* __restrict__ data, const SyncChunk& q, const unsigned* tab, int bpm, u64* ex,
                                           u64 entry0, u64& entry, u64& exit_, uint4& cnt) {
    const int tid = threadIdx.x;
    int rounds = 0;
    for (int r = 0; r < JS_CH; ++r) {
        __syncthreads();                                                 // the exits of the round before
        const u64 in = tid > 0 ? ex[tid - 1] : entry0;
        const bool redo = q.active && in != entry;
        if (!__syncthreads_or(redo)) break;                              // and every lane has read its neighbour before one writes
        if (redo) {
            entry = in;
            exit_ = sync_decode<false>(data, q.iv, tab, bpm, entry, q.end_bits, cnt, nullptr, make_uint4(0u, 0u, 0u, 0u), false, nullptr);
            ex[tid] = exit_;
        }
        ++rounds;
    }
    return rounds;
}

__global__ __launch_bounds__(JS_CH) void jpeg_sync_spec_kernel(const unsigned char* __restrict__ data, long long data_bytes,
                                                               const long long* __restrict__ pos, const unsigned* __restrict__ tables, DGeo g,
                                                               int restart, int n_int, int max_chunks, long long max_bytes,
                                                               const int* __restrict__ status, SyncWs w) {
    __shared__ unsigned tab[6 * TW];
    __shared__ u64 ex[JS_CH];
    SyncChunk q;
    if (!sync_chunk(q, pos, data_bytes, tables, tab, g, restart, n_int, max_chunks, max_bytes, status)) return;
    const int tid = threadIdx.x;
    u64 entry = 0, exit_ = 0;
    uint4 cnt = make_uint4(0u, 0u, 0u, 0u);
    if (q.active) {
        long long b = q.iv.lo + (long long)q.j * JS_S;                   // < hi, and b - 1 >= lo where j > 0
        if (q.j > 0 && data[b - 1] == 0xffu && data[b] == 0u) ++b;       // the 00 of a straddling FF 00 is no data
        entry = (u64)((b - q.iv.lo) * 8) << 16;
        exit_ = sync_decode<false>(data, q.iv, tab, g.bpm, entry, q.end_bits, cnt, nullptr, make_uint4(0u, 0u, 0u, 0u), false, nullptr);
    }
    ex[tid] = exit_;
    const int rounds = sync_rounds(data, q, tab, g.bpm, ex, entry, entry, exit_, cnt);   // lane 0 keeps its entry
    if (q.active) {
        w.entry[q.slot] = entry;
        w.exit_[q.slot] = exit_;
        w.cnt[q.slot] = cnt;
        if (q.j + 1 == q.n_sub || tid == JS_CH - 1) w.cexit[q.cslot] = exit_;
    }
    if (tid == 0) w.rounds[2 * q.cslot] = 1 + rounds;
}

__global__ __launch_bounds__(JS_CH) void jpeg_sync_verify_kernel(const unsigned char* __restrict__ data, long long data_bytes,
                                                                 const long long* __restrict__ pos, const unsigned* __restrict__ tables, DGeo g,
                                                                 int restart, int n_int, int max_chunks, long long max_bytes,
                                                                 const int* __restrict__ status, SyncWs w) {
    __shared__ unsigned tab[6 * TW];
    __shared__ u64 ex[JS_CH];
    __shared__ uint4 sc[2][JS_CH];
    SyncChunk q;
    if (!sync_chunk(q, pos, data_bytes, tables, tab, g, restart, n_int, max_chunks, max_bytes, status)) return;
    const int tid = threadIdx.x;
    u64 entry = 0, exit_ = 0;
    uint4 cnt = make_uint4(0u, 0u, 0u, 0u);
    if (q.active) {
        entry = w.entry[q.slot];
        exit_ = w.exit_[q.slot];
        cnt = w.cnt[q.slot];
    }
    ex[tid] = exit_;
    const u64 entry0 = q.c > 0 ? w.cexit[q.cslot - 1] : 0ull;            // chunk 0: the interval's first bit, block 0, a DC
    const int rounds = sync_rounds(data, q, tab, g.bpm, ex, entry0, entry, exit_, cnt);
    if (q.active) {
        w.entry[q.slot] = entry;                                         // the true one, if every chunk of the interval is ok
        if (q.j + 1 == q.n_sub || tid == JS_CH - 1) w.cok[q.cslot] = exit_ == w.cexit[q.cslot] ? 1 : 0;
    }
    if (tid == 0) w.rounds[2 * q.cslot + 1] = rounds;
    int cur = 0;                                                         // the inclusive scan of cnt, eight fixed steps
    sc[0][tid] = cnt;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < JS_CH; d <<= 1) {
        uint4 v = sc[cur][tid];
        if (tid >= d) v = add4(v, sc[cur][tid - d]);
        sc[cur ^ 1][tid] = v;
        __syncthreads();
        cur ^= 1;
    }
    const uint4 inc = sc[cur][tid];
    if (q.active) w.cnt[q.slot] = make_uint4(inc.x - cnt.x, inc.y - cnt.y, inc.z - cnt.z, inc.w - cnt.w);
    if (tid == JS_CH - 1) w.ctot[q.cslot] = inc;
}

__global__ __launch_bounds__(JS_FALL_THREADS) void jpeg_sync_scan_kernel(const long long* __restrict__ pos, long long data_bytes, DGeo g, int restart,
                                                                         int n_int, long long n_all, int max_chunks, long long max_bytes,
                                                                         const int* __restrict__ status, int* __restrict__ route, SyncWs w) {
    const long long t = (long long)blockIdx.x * JS_FALL_THREADS + threadIdx.x;
    if (t >= n_all) return;
    if (status[t] != MBX_JPEG_DEC_OK) { route[t] = 0; return; }          // the index's verdict stands; nothing is decoded
    const SyncIv iv = sync_interval(pos, data_bytes, g, restart, n_int, t);
    const long long len = iv.hi - iv.lo;
    if (len > max_bytes) { route[t] = 3; return; }
    if (len == 0) { route[t] = 2; return; }
    const int n_chunk = (int)(((len + JS_S - 1) / JS_S + JS_CH - 1) / JS_CH);   // <= max_chunks
    uint4 run = make_uint4(0u, 0u, 0u, 0u);
    int ok = 1;
    for (int c = 0; c < n_chunk; ++c) {
        const size_t s = (size_t)t * max_chunks + c;
        ok &= w.cok[s];
        w.coff[s] = run;
        run = add4(run, w.ctot[s]);
    }
    route[t] = ok ? 0 : 1;
}

__global__ __launch_bounds__(JS_CH) void jpeg_sync_write_kernel(const unsigned char* __restrict__ data, long long data_bytes,
                                                                const long long* __restrict__ pos, const unsigned* __restrict__ tables, DGeo g,
                                                                int restart, int n_int, int max_chunks, long long max_bytes,
                                                                const int* __restrict__ status, short* __restrict__ coef, int* __restrict__ route,
                                                                SyncWs w) {
    __shared__ unsigned tab[6 * TW];
    SyncChunk q;
    if (!sync_chunk(q, pos, data_bytes, tables, tab, g, restart, n_int, max_chunks, max_bytes, status)) return;
    // Other workgroups of this launch may store 2 into route[q.t] while this one reads it.  Either value is right: a lane that still sees 0
    // only stores coefficients that kernel Z clears again.  No barrier follows
    if (route[q.t] != 0 || !q.active) return;
    uint4 cnt;
    bool bad = false;
    sync_decode<true>(data, q.iv, tab, g.bpm, w.entry[q.slot], q.end_bits, cnt, coef, add4(w.cnt[q.slot], w.coff[q.cslot]), q.j + 1 == q.n_sub, &bad);
    if (bad) route[q.t] = 2;
}

// the blocks of the intervals that go to the fallback, zeroed again: whatever C stored before a check failed
__global__ __launch_bounds__(JS_CH) void jpeg_sync_zero_kernel(const long long* __restrict__ pos, long long data_bytes, DGeo g, int restart, int n_int,
                                                               int max_chunks, const int* __restrict__ route, short* __restrict__ coef) {
    const long long t = blockIdx.x / max_chunks;
    if (route[t] == 0) return;
    const SyncIv iv = sync_interval(pos, data_bytes, g, restart, n_int, t);
    uint4* b4 = reinterpret_cast<uint4*>(coef + iv.coef0);               // 16-byte aligned: coef is, and a block is 128 bytes
    const size_t n = (size_t)iv.total * 8;
    for (size_t i = (size_t)(blockIdx.x % max_chunks) * JS_CH + threadIdx.x; i < n; i += (size_t)max_chunks * JS_CH) b4[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ __launch_bounds__(JS_FALL_THREADS) void jpeg_sync_fallback_kernel(const unsigned char* __restrict__ data, long long data_bytes,
                                                                             const long long* __restrict__ pos, const unsigned* __restrict__ tables,
                                                                             DGeo g, int restart, int n_int, long long n_all, short* __restrict__ coef,
                                                                             int* __restrict__ status, const int* __restrict__ route) {
    __shared__ unsigned tab[6 * TW];
    for (int i = threadIdx.x; i < 6 * TW; i += JS_FALL_THREADS) tab[i] = tables[i];
    __syncthreads();
    const long long t = (long long)blockIdx.x * JS_FALL_THREADS + threadIdx.x;
    if (t >= n_all || route[t] == 0) return;                             // route != 0 only where status[t] is OK
    jpeg_decode_interval(data, data_bytes, pos, tab, g, restart, n_int, t, coef, status);
}

}  // namespace

extern "C" size_t mbx_jpeg_dec_sync_ws(int F, int n_int, long long max_interval_bytes) {
    if (F < 1 || F > MBX_JPEG_MAX_FRAMES || n_int < 1 || n_int > MBX_JPEG_MAX_SIZE * MBX_JPEG_MAX_SIZE / 64 || max_interval_bytes < 0 ||
        max_interval_bytes > JS_MAX_BYTES)
        return 0;
    return sync_ws_bytes((long long)F * n_int, sync_max_chunks(max_interval_bytes));
}

extern "C" int mbx_jpeg_dec_entropy_sync(const unsigned char* data, long long data_bytes, const long long* pos, const unsigned* tables, int F, int H,
                                         int W, int sub, int restart, long long max_interval_bytes, short* coef, int* status, int* route, void* ws,
                                         size_t ws_bytes, void* stream) {
    MBX_CHECK_ARG(F >= 0 && F <= MBX_JPEG_MAX_FRAMES && H >= 1 && H <= MBX_JPEG_MAX_SIZE && W >= 1 && W <= MBX_JPEG_MAX_SIZE,
                  "jpeg_dec_entropy_sync: bad sizes F=%d H=%d W=%d (0 <= F <= %d, 1 <= H, W <= %d)", F, H, W, MBX_JPEG_MAX_FRAMES, MBX_JPEG_MAX_SIZE);
    MBX_CHECK_ARG(sub >= 0 && sub <= 2, "jpeg_dec_entropy_sync: subsampling %d (0: 4:4:4, 1: 4:2:0, 2: 4:2:2)", sub);
    MBX_CHECK_ARG(restart >= 0 && restart <= 65535 && data_bytes >= 0, "jpeg_dec_entropy_sync: restart interval %d (0: none, .. 65535 MCUs), data_bytes %lld",
                  restart, data_bytes);
    MBX_CHECK_ARG(max_interval_bytes >= 0 && max_interval_bytes <= JS_MAX_BYTES, "jpeg_dec_entropy_sync: max_interval_bytes %lld (0 .. %lld)",
                  max_interval_bytes, JS_MAX_BYTES);
    if (F == 0) return 0;
    MBX_CHECK_ARG(data && pos && tables && coef && status && route && ws, "jpeg_dec_entropy_sync: null pointer");
    MBX_CHECK_ARG(((uintptr_t)coef & 15) == 0 && ((uintptr_t)pos & 7) == 0 && ((uintptr_t)tables & 3) == 0 && ((uintptr_t)status & 3) == 0 &&
                      ((uintptr_t)route & 3) == 0 && ((uintptr_t)ws & 15) == 0,
                  "jpeg_dec_entropy_sync: coef and ws must be 16-byte aligned, pos 8-byte, tables, status and route 4-byte");
    const DGeo g = make_dgeo(H, W, sub);
    const int n_int = restart ? (g.n_mcu + restart - 1) / restart : 1;
    const long long n_all = (long long)F * n_int;
    const int max_chunks = sync_max_chunks(max_interval_bytes);
    const size_t need = sync_ws_bytes(n_all, max_chunks);
    MBX_CHECK_ARG(ws_bytes >= need, "jpeg_dec_entropy_sync: workspace of %zu bytes, %zu needed", ws_bytes, need);
    const long long grid = n_all * max_chunks;
    MBX_CHECK_ARG(grid <= 0x7fffffffll, "jpeg_dec_entropy_sync: %lld intervals of up to %d chunks are too many for one launch", n_all, max_chunks);
    const SyncWs w = make_sync_ws(ws, n_all, max_chunks);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(coef, 0, (size_t)F * g.n_mcu * g.bpm * 64 * sizeof(short), s);
    if (e != hipSuccess) return mbx_set_error("jpeg_dec_entropy_sync: memset failed: %s", hipGetErrorString(e));
    const dim3 chunks((unsigned)grid), lanes((unsigned)((n_all + JS_FALL_THREADS - 1) / JS_FALL_THREADS));
    hipLaunchKernelGGL(jpeg_sync_spec_kernel, chunks, dim3(JS_CH), 0, s, data, data_bytes, pos, tables, g, restart, n_int, max_chunks, max_interval_bytes,
                       status, w);
    MBX_LAUNCH_CHECK("jpeg_dec_entropy_sync (speculate)");
    hipLaunchKernelGGL(jpeg_sync_verify_kernel, chunks, dim3(JS_CH), 0, s, data, data_bytes, pos, tables, g, restart, n_int, max_chunks,
                       max_interval_bytes, status, w);
    MBX_LAUNCH_CHECK("jpeg_dec_entropy_sync (verify)");
    hipLaunchKernelGGL(jpeg_sync_scan_kernel, lanes, dim3(JS_FALL_THREADS), 0, s, pos, data_bytes, g, restart, n_int, n_all, max_chunks,
                       max_interval_bytes, status, route, w);
    MBX_LAUNCH_CHECK("jpeg_dec_entropy_sync (scan)");
    hipLaunchKernelGGL(jpeg_sync_write_kernel, chunks, dim3(JS_CH), 0, s, data, data_bytes, pos, tables, g, restart, n_int, max_chunks,
                       max_interval_bytes, status, coef, route, w);
    MBX_LAUNCH_CHECK("jpeg_dec_entropy_sync (write)");
    hipLaunchKernelGGL(jpeg_sync_zero_kernel, chunks, dim3(JS_CH), 0, s, pos, data_bytes, g, restart, n_int, max_chunks, route, coef);
    MBX_LAUNCH_CHECK("jpeg_dec_entropy_sync (zero)");
    hipLaunchKernelGGL(jpeg_sync_fallback_kernel, lanes, dim3(JS_FALL_THREADS), 0, s, data, data_bytes, pos, tables, g, restart, n_int, n_all, coef,
                       status, route);
    MBX_LAUNCH_CHECK("jpeg_dec_entropy_sync (fallback)");
    return 0;
}
