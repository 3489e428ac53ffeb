// CPU-only sanitizer harness for y2h::write_jpg_rgb24 (host/y2_jpeg.cpp + csrc/jpeg_tables.hpp): the encoder over ragged sizes - 1x1,
// one-row and one-column frames, widths and heights on both sides of multiples of 8 - with noise, flat and 0 / 255 checkerboard
// content at the qualities' extremes, and over capacities from 0 to the stream's size.  Every frame and every output sits exactly
// in its allocation, so a read outside the frame or a write at or beyond the capacity is a sanitizer report; the bytes below a
// small capacity must be the full stream's.  Host code only; build and run on a CPU:
//   g++ -std=c++17 -O1 -g -fwrapv -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -fsanitize=float-cast-overflow tools/jpeg_host_check.cpp host/y2_jpeg.cpp host/y2_host.cpp host/y2_codec.cpp -pthread
// usage: jpeg_host_check [rounds per size]
#include "../host/y2_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 6;
    std::mt19937 rng(20261019);
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 9}, {7, 7}, {8, 8}, {9, 8}, {8, 9}, {15, 17}, {33, 17}, {97, 3}, {3, 97}, {64, 48}, {300, 2}, {5, 211}};
    const int qualities[] = {-5, 0, 1, 30, 50, 80, 100, 1000};
    long calls = 0, bytes = 0;
    for (const auto &s : sizes) {
        const int w = s[0], h = s[1];
        for (int r = 0; r < rounds; ++r) {
            std::vector<uint8_t> frame((size_t)w * h * 3);
            const int kind = r % 3;
            for (size_t i = 0; i < frame.size(); ++i) {
                const size_t px = i / 3;
                frame[i] = kind == 0 ? (uint8_t)rng() : kind == 1 ? (uint8_t)(40 * r) : (uint8_t)(((px % (size_t)w + px / (size_t)w) & 1) ? 255 : 0);
            }
            const int q = qualities[rng() % (sizeof(qualities) / sizeof(qualities[0]))];
            const long n = y2h::write_jpg_rgb24(frame.data(), w, h, q, nullptr, 0);   // capacity 0: the size alone
            if (n < 609 || (size_t)n > y2h::jpg_rgb24_bound(w, h)) { std::printf("%dx%d q%d: size %ld outside 609..bound\n", w, h, q, n); return 1; }
            std::vector<uint8_t> full((size_t)n);
            if (y2h::write_jpg_rgb24(frame.data(), w, h, q, full.data(), full.size()) != n) return 1;
            if (full[0] != 0xFF || full[1] != 0xD8 || full[(size_t)n - 2] != 0xFF || full[(size_t)n - 1] != 0xD9) return 1;
            const size_t caps[] = {1, 606, 607, 608, (size_t)n - 2, (size_t)n - 1, (size_t)(rng() % (unsigned long)n)};
            for (size_t cap : caps) {
                std::vector<uint8_t> part(cap);
                if (y2h::write_jpg_rgb24(frame.data(), w, h, q, part.data(), cap) != n || std::memcmp(part.data(), full.data(), cap) != 0) {
                    std::printf("%dx%d q%d: capacity %zu changes the stream\n", w, h, q, cap);
                    return 1;
                }
                ++calls;
            }
            calls += 2;
            bytes += n;
        }
    }
    // refused before anything is read
    if (y2h::write_jpg_rgb24(nullptr, 4, 4, 80, nullptr, 0) != -1 || y2h::jpg_rgb24_bound(0, 4) != 0 || y2h::jpg_rgb24_bound(4, 65536) != 0) return 1;
    std::printf("%ld calls, %ld stream bytes\n", calls, bytes);
    return 0;
}
