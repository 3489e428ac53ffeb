// CPU-only sanitizer harness for the GPU JPEG decoder's stages (csrc/jpeg_scan.hpp, csrc/jpeg_parse.hpp: the same functions the
// kernels run, here on the host through y2jpg::decode_ref, the body of yolo2_hip_decode_jpeg_ref).  Hostile bytes are tried HERE: every
// file given on the command line, then mutated copies of it (bit flips, truncations, overwritten bytes, runs of 0xff, an RST marker
// removed or doubled).  Every case must end in a refusal, a status, or a picture - no access outside the stream, the coefficient blocks
// or the planes, no undefined shift - and the contract with the host decoder (host/y2_codec.cpp) must hold: status 0 means the host
// decoder's bytes; where the host decoder throws, the stream is refused or flagged.  Links no GPU code.  Built and run by
// tests/test_jpegdec_host.py with
//   g++ -std=c++17 -O1 -g -fwrapv -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/fuzz_jpegdec.cpp host/y2_codec.cpp host/y2_host.cpp
// usage: fuzz_jpegdec <mutations per file> <files...>
#include "../csrc/jpeg_parse.hpp"
#include "../host/y2_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <vector>
int main(int argc, char **argv)
{
    long same = 0, flagged = 0, refused = 0, wrong = 0;
    std::mt19937 rng(24680);
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200;
    for (int f = 2; f < argc; ++f) {
        std::ifstream in(argv[f], std::ios::binary);
        std::vector<unsigned char> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        if (data.size() < 4) continue;
        for (int r = 0; r <= rounds; ++r) {
            std::vector<unsigned char> d = data;
            if (r > 0) {
                const int kind = rng() % 6;
                if (kind == 0) { const int n = 1 + rng() % 8; for (int k = 0; k < n; ++k) d[rng() % d.size()] ^= (unsigned char)(1u << (rng() % 8)); }
                else if (kind == 1) d.resize(1 + rng() % d.size());
                else if (kind == 2) { const size_t p = rng() % d.size(); d[p] = (unsigned char)rng(); if (p + 1 < d.size()) d[p + 1] = (unsigned char)rng(); }
                else if (kind == 3) { const size_t p = rng() % d.size(), n = std::min<size_t>(d.size() - p, 1 + rng() % 64); for (size_t k = 0; k < n; ++k) d[p + k] = 0xff; }
                else {   // an RST marker (if any) removed or doubled
                    std::vector<size_t> at;
                    for (size_t p = 0; p + 1 < d.size(); ++p) if (d[p] == 0xff && d[p + 1] >= 0xd0 && d[p + 1] <= 0xd7) at.push_back(p);
                    if (!at.empty()) {
                        const size_t p = at[rng() % at.size()];
                        if (kind == 4) d.erase(d.begin() + (long)p, d.begin() + (long)p + 2);
                        else d.insert(d.begin() + (long)p, d.begin() + (long)p, d.begin() + (long)p + 2);
                    }
                }
            }
            // exact-size heap copies: the sanitizer sees a read one byte past the stream or a write one byte past the picture
            std::vector<unsigned char> tight(d.begin(), d.end());
            y2jpg::Info info;
            y2jpg::parse(tight.data(), tight.size(), info, nullptr);
            std::vector<unsigned char> rgb(info.gpu_decodable ? (size_t)info.width * info.height * 3 : 1);
            int w = 0, h = 0, status = 0;
            const int why = y2jpg::decode_ref(tight.data(), tight.size(), rgb.data(), rgb.size(), &w, &h, &status);
            bool threw = false;
            y2h::ImageU8 im;
            try { im = y2h::decode_image(tight.data(), tight.size(), "fuzz"); } catch (const std::exception &) { threw = true; }
            if (why != 0) { ++refused; continue; }
            if (status != 0) { ++flagged; continue; }
            if (threw || im.w != w || im.h != h || im.rgb.size() != rgb.size() || memcmp(im.rgb.data(), rgb.data(), rgb.size()) != 0) {
                ++wrong;
                std::fprintf(stderr, "%s mutation %d: status 0 but %s\n", argv[f], r, threw ? "the host decoder throws" : "other bytes than the host decoder's");
            } else {
                ++same;
            }
        }
    }
    std::printf("same %ld, flagged %ld, refused %ld, wrong %ld\n", same, flagged, refused, wrong);
    return wrong ? 1 : 0;
}
