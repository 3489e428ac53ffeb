// CPU-only sanitizer harness for the many-lanes-per-segment entropy stage (csrc/jpeg_scan.hpp: SBits, split_run; csrc/jpeg_parse.hpp:
// split_plan, split_segment_host - the functions k_jpegdec_split runs, here as loops over lanes and rounds).  The contract is
// exactness against the one-lane decoder: for every file given and for mutated copies of it (bit flips, truncations, runs of 0xff)
// y2jpg::decode_ref with a subsequence size must leave the reason, the status and the bytes that y2jpg::decode_ref leaves without one -
// and no access outside the stream, the records or the coefficient blocks.  Links no GPU code.  Built and run by
// tests/test_jpegdec_split_host.py with
//   g++ -std=c++17 -O1 -g -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/fuzz_jpegdec_split.cpp
// usage: fuzz_jpegdec_split <mutations per file> <S> <S> <files...>
#include "../csrc/jpeg_parse.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <vector>
int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    long same = 0, split_segments = 0, fallbacks = 0, refused = 0, mismatch = 0;
    std::mt19937 rng(13579);
    const int rounds = std::atoi(argv[1]), sizes[2] = {std::atoi(argv[2]), std::atoi(argv[3])};
    for (int f = 4; f < argc; ++f) {
        std::ifstream in(argv[f], std::ios::binary);
        std::vector<unsigned char> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (data.size() < 4) continue;
        for (int r = 0; r <= rounds; ++r) {
            std::vector<unsigned char> d = data;
            if (r > 0) {
                const int kind = rng() % 3;
                if (kind == 0) { const int n = 1 + rng() % 8; for (int k = 0; k < n; ++k) d[rng() % d.size()] ^= (unsigned char)(1u << (rng() % 8)); }
                else if (kind == 1) d.resize(1 + rng() % d.size());
                else { const size_t p = rng() % d.size(), n = std::min<size_t>(d.size() - p, 1 + rng() % 64); for (size_t k = 0; k < n; ++k) d[p + k] = 0xff; }
            }
            std::vector<unsigned char> tight(d.begin(), d.end());      // exact-size heap copy: a read one byte past the stream is seen
            y2jpg::Info info;
            y2jpg::parse(tight.data(), tight.size(), info, nullptr);
            const size_t bytes = info.gpu_decodable ? (size_t)info.width * info.height * 3 : 1;
            std::vector<unsigned char> want(bytes), got(bytes);
            int w0 = 0, h0 = 0, st0 = 0;
            const int why0 = y2jpg::decode_ref(tight.data(), tight.size(), want.data(), want.size(), &w0, &h0, &st0);
            if (why0) ++refused;
            for (int S : sizes) {
                int w = 0, h = 0, st = 0;
                double info8[8];
                std::fill(got.begin(), got.end(), 0);
                const int why = y2jpg::decode_ref(tight.data(), tight.size(), got.data(), got.size(), &w, &h, &st, S, info8);
                split_segments += (long)info8[1];
                fallbacks += (long)info8[2];
                const bool ok = why == why0 && (why0 != 0 || (st == st0 && w == w0 && h == h0 && (st0 != 0 || got == want)));
                if (ok) { ++same; continue; }
                ++mismatch;
                std::fprintf(stderr, "%s mutation %d, S %d: reason %d / %d, status %d / %d\n", argv[f], r, S, why, why0, st, st0);
            }
        }
    }
    std::printf("same %ld, split %ld, fallbacks %ld, refused %ld, mismatch %ld\n", same, split_segments, fallbacks, refused, mismatch);
    return mismatch ? 1 : 0;
}
