// CPU-only sanitizer harness for y2h::draw_detections_rgb24 (host/y2_host.cpp + csrc/draw_list.hpp): the painter over the extremes -
// 1x1 and one-row frames, boxes far outside the image, NaN and infinite box fields, out-of-int-range products, labels longer than the
// 127-character text, empty and missing labels, classes beyond the label list.  Every frame sits exactly in its allocation, so a
// pixel outside the image is a sanitizer report.  Host code only; build and run on a CPU:
//   g++ -std=c++17 -O1 -g -fwrapv -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -fsanitize=float-cast-overflow tools/draw_host_check.cpp host/y2_host.cpp host/y2_codec.cpp -pthread
// usage: draw_host_check [random records per frame size]
#include "../host/y2_host.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>
int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 2000;
    std::mt19937 rng(20261019);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    const float special[] = {0.f, 1.f, -1.f, .5f, 1e12f, -1e12f, 3e38f, -3e38f, inf, -inf, nan, 1e-30f, 2147483648.f, -2147483904.f, .999999f};
    const std::string long_label(500, 'w'), odd_label = "a_b! Z9.";
    const char *labels[] = {"person", long_label.c_str(), "", odd_label.c_str()};
    const int sizes[][2] = {{1, 1}, {2, 1}, {1, 7}, {33, 17}, {96, 64}, {300, 2}, {5, 40}};
    long drawn = 0, calls = 0;
    std::uniform_real_distribution<float> uni(-.5f, 1.5f);
    for (const auto &s : sizes) {
        const int w = s[0], h = s[1];
        for (int r = 0; r < rounds; ++r) {
            std::vector<uint8_t> frame((size_t)w * h * 3, 7);
            std::vector<y2h::DrawRecord> d(1 + rng() % 4);
            for (auto &x : d) {
                auto pick = [&]() { return rng() % 3 ? uni(rng) : special[rng() % (sizeof(special) / sizeof(special[0]))]; };
                x.frame = 0; x.det = 0;
                x.cls = (int)(rng() % 12) - 1;
                x.prob = rng() % 8 ? uni(rng) : pick();
                x.x = pick(); x.y = pick(); x.w = pick(); x.h = pick();
            }
            const bool with_labels = rng() % 4 != 0;
            drawn += y2h::draw_detections_rgb24(frame.data(), w, h, d.data(), (int)d.size(), .24f, with_labels ? labels : nullptr,
                                                with_labels ? (int)(rng() % 5) : 0);
            ++calls;
        }
    }
    std::printf("%ld calls, %ld records drawn\n", calls, drawn);
    return drawn > 0 ? 0 : 1;
}
