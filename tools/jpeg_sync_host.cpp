// The decode of csrc/jpeg_sync.hip on the host: the reader, the lookup and sync_decode are __host__ __device__, and this program walks the stages
// A (speculate, rounds), B (verify, rounds, sums), S (scan) and C (write) over them lane by lane, as the kernels do, for one interval per
// input.  It is what tests/test_jpeg_sync_host.py builds (host pass only, with AddressSanitizer and UBSan) and runs: the code that reads
// bytes it did not write, checked against the numpy model without a GPU.
//   in : int32 n; per input: int64 bytes, int32 bpm, int32 n_mcu, u32 tables [6][MBX_JPEG_DEC_TABLE_WORDS], the interval's bytes
//   out: per input: int32 route (0, 1 or 2), int32 rounds of A in chunk 0, int16 coef [n_mcu * bpm * 64] (zeros unless route is 0)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../motionbert_amd/csrc/jpeg_sync.hip"

int mbx_set_error(const char* fmt, ...) { (void)fmt; return 1; }

namespace {

struct Lane { u64 entry, exit_; uint4 cnt; };

// the rounds of sync_rounds: every lane reads its neighbour's exit of the round before, then the lanes that were handed a new entry decode
int rounds(const unsigned char* data, const SyncIv& iv, const unsigned* tab, int bpm, std::vector<Lane>& l, long long first, u64 entry0) {
    int n = 0;
    for (int r = 0; r < JS_CH; ++r) {
        std::vector<u64> in(l.size());
        bool any = false;
        for (size_t i = 0; i < l.size(); ++i) {
            in[i] = i ? l[i - 1].exit_ : entry0;
            any |= in[i] != l[i].entry;
        }
        if (!any) break;
        for (size_t i = 0; i < l.size(); ++i)
            if (in[i] != l[i].entry) {
                const long long e = (first + (long long)i + 1) * JS_S, len = iv.hi - iv.lo;
                l[i].entry = in[i];
                l[i].exit_ = sync_decode<false>(data, iv, tab, bpm, in[i], (unsigned)((e < len ? e : len) * 8), l[i].cnt, nullptr, make_uint4(0u, 0u, 0u, 0u),
                                                false, nullptr);
            }
        ++n;
    }
    return n;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    int n = 0;
    if (!fi || !fo || fread(&n, 4, 1, fi) != 1) return 2;
    for (int x = 0; x < n; ++x) {
        long long len;
        int bpm, n_mcu;
        std::vector<unsigned> tab(6 * TW);
        if (fread(&len, 8, 1, fi) != 1 || fread(&bpm, 4, 1, fi) != 1 || fread(&n_mcu, 4, 1, fi) != 1 || fread(tab.data(), 4, tab.size(), fi) != tab.size()) return 2;
        std::vector<unsigned char> raw((size_t)len);                     // exactly the interval: a read past it is the sanitizer's
        if (len && fread(raw.data(), 1, raw.size(), fi) != raw.size()) return 2;
        SyncIv iv;
        iv.lo = 0; iv.hi = len; iv.total = (unsigned)(n_mcu * bpm); iv.coef0 = 0;
        std::vector<short> coef((size_t)iv.total * 64, 0);
        const long long n_sub = (len + JS_S - 1) / JS_S, n_chunk = (n_sub + JS_CH - 1) / JS_CH;
        int route = len == 0 ? 2 : 0, rounds_a = 0;
        std::vector<std::vector<Lane>> lanes((size_t)n_chunk);
        std::vector<u64> cexit((size_t)n_chunk);
        for (long long c = 0; c < n_chunk; ++c) {                        // A
            const long long first = c * JS_CH, last = first + JS_CH < n_sub ? first + JS_CH : n_sub;
            std::vector<Lane>& l = lanes[(size_t)c];
            l.resize((size_t)(last - first));
            for (long long j = first; j < last; ++j) {
                long long b = j * JS_S;
                if (j > 0 && raw[(size_t)b - 1] == 0xffu && raw[(size_t)b] == 0u) ++b;
                const long long e = (j + 1) * JS_S;
                Lane& q = l[(size_t)(j - first)];
                q.entry = (u64)(b * 8) << 16;
                q.exit_ = sync_decode<false>(raw.data(), iv, tab.data(), bpm, q.entry, (unsigned)((e < len ? e : len) * 8), q.cnt, nullptr,
                                             make_uint4(0u, 0u, 0u, 0u), false, nullptr);
            }
            const int r = 1 + rounds(raw.data(), iv, tab.data(), bpm, l, first, l[0].entry);
            if (c == 0) rounds_a = r;
            cexit[(size_t)c] = l.back().exit_;
        }
        for (long long c = 1; c < n_chunk; ++c) {                        // B
            rounds(raw.data(), iv, tab.data(), bpm, lanes[(size_t)c], c * JS_CH, cexit[(size_t)c - 1]);
            if (lanes[(size_t)c].back().exit_ != cexit[(size_t)c]) route = 1;
        }
        if (route == 0) {                                                // S and C
            uint4 run = make_uint4(0u, 0u, 0u, 0u);
            bool bad = false;
            for (long long j = 0; j < n_sub; ++j) {
                Lane& q = lanes[(size_t)(j / JS_CH)][(size_t)(j % JS_CH)];
                const long long e = (j + 1) * JS_S;
                uint4 cnt;
                sync_decode<true>(raw.data(), iv, tab.data(), bpm, q.entry, (unsigned)((e < len ? e : len) * 8), cnt, coef.data(), run, j + 1 == n_sub, &bad);
                run = add4(run, q.cnt);
            }
            if (bad) {
                route = 2;
                coef.assign(coef.size(), 0);
            }
        } else {
            coef.assign(coef.size(), 0);
        }
        fwrite(&route, 4, 1, fo);
        fwrite(&rounds_a, 4, 1, fo);
        fwrite(coef.data(), 2, coef.size(), fo);
    }
    fclose(fi);
    return fclose(fo) ? 2 : 0;
}
