// yolov2_calibrate -- fp32 weight files + calibration images -> the int16 weight set yolov2_detect --precision int16 runs, or
// (--format int8) the int8 weight set of --precision int8: the same statistics, the int8 Q rule, per-channel weight Qs.
//
// The reference makes this set with a separate tool (weights/README.md step 2b); here it is the calibration tier of the HIP library
// behind its C ABI (include/yolo2_hip.h, "calibration"): the exact fp32 pass runs the images, one abs-max per tensor gives the
// ranges, the Q rule turns them into the three tables and the GPU quantises the resident fp32 streams.  Plain C++ host, like
// yolov2_detect: it decodes the images (y2_codec.cpp) or reads raw video frames (--video-raw, any --video-pix-fmt), hands bytes over, and writes the five files in the reference's layout
// (one pad element after every odd-length layer, yolo2_model.cpp:198-224).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/yolo2_hip.h"
#include "y2_host.hpp"

namespace {

struct Config {
    std::string weights_dir = "weights", out_dir, input_dir, input_list, video_raw;
    int video_w = 640, video_h = 480, video_pixfmt = YOLO2_PIX_RGB24, max_frames = 0;   // --video-raw: as yolov2_detect's
    int batch = 8, device = 0;
    float headroom = 1.0f;
    std::string format = "int16";
};

void print_usage(const char *prog)
{
    std::printf(
        "Usage: %s --weights <dir> (--input-dir <dir> | --input-list <file> | --video-raw <file>) --out <dir> [options]\n"
        "  --weights <dir>       Directory with weights_reorg.bin and bias.bin (fp32; default: weights)\n"
        "  --input-dir <dir>     Calibration images: every *.jpg / *.jpeg / *.png / *.ppm / *.pgm of a directory, sorted by name\n"
        "  --input-list <file>   Calibration images, one path per line\n"
        "  --video-raw <file>    Calibration frames: raw video frames as yolov2_detect takes them, with --video-width <w> --video-height <h>\n"
        "                        (default 640x480), --video-pix-fmt <rgb24|yuyv422|nv12|yuv420p|bgr24|rgba|bgra> (default rgb24; also\n"
        "                        yuyv, i420, rgb0, bgr0: the GPU reads the frames as they are; yuyv422 needs an even width, nv12 / yuv420p an even\n"
        "                        width and height; bgr24 is packed B G R, rgba / bgra are R G B X / B G R X with the fourth byte unused) and\n"
        "                        --max-frames <n> (default: all)\n"
        "  --out <dir>           Where weights_reorg_int16.bin, bias_int16.bin, weight_int16_Q.bin, bias_int16_Q.bin and iofm_Q.bin go\n"
        "  --batch <n>           Images per pass of the exact fp32 network (default 8)\n"
        "  --headroom <float>    Factor >= 1 kept free above every conv output's measured maximum (default 1)\n"
        "  --device <n>          HIP device (default 0)\n"
        "  --format <int16|int8> int16 (default): the five files above.  int8: weights_int8.bin (natural order), bias_int32.bin,\n"
        "                        weight_int8_Q.bin (one Q per output channel) and iofm_int8_Q.bin, by the rule\n"
        "                        'the largest Q in -8..24 with headroom * max|x| * 2^Q < 127.5'\n"
        "Q rule: the largest Q in 0..15 with headroom * max|x| * 2^Q < 32767.5 (it still rounds to at most 32767), per tensor.\n",
        prog);
}

Config parse_args(int argc, char **argv)
{
    Config cfg;
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        auto need = [&]() {
            if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", arg.c_str()); std::exit(1); }
            return true;
        };
        if (arg == "--help" || arg == "-h") { print_usage(argv[0]); std::exit(0); }
        else if (arg == "--weights" && need()) cfg.weights_dir = argv[++i];
        else if (arg == "--input-dir" && need()) cfg.input_dir = argv[++i];
        else if (arg == "--input-list" && need()) cfg.input_list = argv[++i];
        else if (arg == "--video-raw" && need()) cfg.video_raw = argv[++i];
        else if (arg == "--video-width" && need()) cfg.video_w = std::atoi(argv[++i]);
        else if (arg == "--video-height" && need()) cfg.video_h = std::atoi(argv[++i]);
        else if (arg == "--max-frames" && need()) cfg.max_frames = std::atoi(argv[++i]);
        else if (arg == "--video-pix-fmt" && need()) {
            const std::string v = argv[++i];
            if (v == "rgb24") cfg.video_pixfmt = YOLO2_PIX_RGB24;
            else if (v == "yuyv422" || v == "yuyv") cfg.video_pixfmt = YOLO2_PIX_YUYV;
            else if (v == "nv12") cfg.video_pixfmt = YOLO2_PIX_NV12;
            else if (v == "yuv420p" || v == "i420") cfg.video_pixfmt = YOLO2_PIX_I420;
            else if (v == "bgr24") cfg.video_pixfmt = YOLO2_PIX_BGR24;
            else if (v == "rgba" || v == "rgb0") cfg.video_pixfmt = YOLO2_PIX_RGBA32;
            else if (v == "bgra" || v == "bgr0") cfg.video_pixfmt = YOLO2_PIX_BGRA32;
            else { std::fprintf(stderr, "Unsupported --video-pix-fmt %s (rgb24 | yuyv422 | nv12 | yuv420p | bgr24 | rgba | bgra)\n", v.c_str()); std::exit(1); }
        }
        else if (arg == "--out" && need()) cfg.out_dir = argv[++i];
        else if (arg == "--batch" && need()) cfg.batch = std::atoi(argv[++i]);
        else if (arg == "--headroom" && need()) cfg.headroom = (float)std::atof(argv[++i]);
        else if (arg == "--device" && need()) cfg.device = std::atoi(argv[++i]);
        else if (arg == "--format" && need()) cfg.format = argv[++i];
        else { std::fprintf(stderr, "Unknown argument: %s\n", arg.c_str()); print_usage(argv[0]); std::exit(1); }
    }
    if (cfg.out_dir.empty() || (int)!cfg.input_dir.empty() + (int)!cfg.input_list.empty() + (int)!cfg.video_raw.empty() != 1) {
        std::fprintf(stderr, "--out and exactly one of --input-dir / --input-list / --video-raw are required\n");
        print_usage(argv[0]);
        std::exit(1);
    }
    if (!cfg.video_raw.empty()) {
        const bool planar = cfg.video_pixfmt == YOLO2_PIX_NV12 || cfg.video_pixfmt == YOLO2_PIX_I420;
        if (cfg.video_w < 1 || cfg.video_h < 1) { std::fprintf(stderr, "--video-width and --video-height must be positive\n"); std::exit(1); }
        if ((cfg.video_pixfmt == YOLO2_PIX_YUYV && (cfg.video_w & 1)) || (planar && ((cfg.video_w | cfg.video_h) & 1))) {
            std::fprintf(stderr, "--video-pix-fmt %s needs an even --video-width%s, not %dx%d\n",
                         cfg.video_pixfmt == YOLO2_PIX_YUYV ? "yuyv422" : (cfg.video_pixfmt == YOLO2_PIX_NV12 ? "nv12" : "yuv420p"),
                         planar ? " and --video-height" : "", cfg.video_w, cfg.video_h);
            std::exit(1);
        }
    }
    if (cfg.format != "int16" && cfg.format != "int8") { std::fprintf(stderr, "--format must be int16 or int8\n"); std::exit(1); }
    if (cfg.batch < 1 || cfg.batch > 1024) { std::fprintf(stderr, "--batch must be 1..1024\n"); std::exit(1); }
    if (!(cfg.headroom >= 1.0f)) { std::fprintf(stderr, "--headroom must be >= 1\n"); std::exit(1); }
    return cfg;
}

std::vector<std::string> list_inputs(const Config &cfg)
{
    namespace fs = std::filesystem;
    std::vector<std::string> files;
    if (!cfg.input_list.empty()) {
        std::ifstream in(cfg.input_list);
        if (!in) throw std::runtime_error("Cannot open " + cfg.input_list);
        std::string line;
        while (std::getline(in, line)) {
            while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
            if (!line.empty()) files.push_back(line);
        }
    } else {
        for (const auto &e : fs::directory_iterator(cfg.input_dir)) {
            const std::string ext = e.path().extension().string();
            if (ext == ".ppm" || ext == ".pgm" || ext == ".jpg" || ext == ".jpeg" || ext == ".png") files.push_back(e.path().string());
        }
        std::sort(files.begin(), files.end());
    }
    if (files.empty()) throw std::runtime_error("no calibration images");
    return files;
}

// the whole frames of a raw video file, as they are (a trailing partial frame is dropped)
std::vector<std::vector<uint8_t>> read_video_frames(const Config &cfg)
{
    const size_t px = (size_t)cfg.video_w * cfg.video_h;
    const size_t bytes = cfg.video_pixfmt == YOLO2_PIX_RGBA32 || cfg.video_pixfmt == YOLO2_PIX_BGRA32 ? 4 * px
                         : cfg.video_pixfmt == YOLO2_PIX_YUYV ? 2 * px
                         : (cfg.video_pixfmt == YOLO2_PIX_NV12 || cfg.video_pixfmt == YOLO2_PIX_I420 ? px * 3 / 2 : 3 * px);
    std::ifstream in(cfg.video_raw, std::ios::binary);
    if (!in) throw std::runtime_error("Cannot open " + cfg.video_raw);
    std::vector<std::vector<uint8_t>> frames;
    while (cfg.max_frames <= 0 || (int)frames.size() < cfg.max_frames) {
        std::vector<uint8_t> f(bytes);
        in.read(reinterpret_cast<char *>(f.data()), (std::streamsize)bytes);
        if ((size_t)in.gcount() != bytes) break;
        frames.push_back(std::move(f));
    }
    if (frames.empty()) throw std::runtime_error("no whole frame in " + cfg.video_raw);
    return frames;
}

std::vector<float> read_floats(const std::string &path, size_t want)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("Cannot open " + path);
    std::vector<float> v(want);
    in.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(want * sizeof(float)));
    if ((size_t)in.gcount() != want * sizeof(float)) throw std::runtime_error(path + " is short of " + std::to_string(want) + " floats");
    return v;
}

template <typename T>
void write_blob(const std::string &path, const std::vector<T> &v)
{
    std::ofstream out(path, std::ios::binary);
    out.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    if (!out) throw std::runtime_error("Cannot write " + path);
}

// the stream with one zero element after every odd-length layer (yolo2_model.cpp:198-224; yolo2_strip_int16_layer_pad undoes it)
std::vector<int16_t> with_layer_pad(const std::vector<int16_t> &flat, const int *len)
{
    std::vector<int16_t> out;
    size_t off = 0;
    for (int o = 0; o < YOLO2_N_CONV; ++o) {
        out.insert(out.end(), flat.begin() + (long)off, flat.begin() + (long)(off + (size_t)len[o]));
        if (len[o] & 1) out.push_back(0);
        off += (size_t)len[o];
    }
    return out;
}

void check(int rc)
{
    if (rc != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
}

int run(const Config &cfg)
{
    const bool video = !cfg.video_raw.empty();
    const std::vector<std::string> files = video ? std::vector<std::string>() : list_inputs(cfg);
    const std::vector<float> w = read_floats(cfg.weights_dir + "/weights_reorg.bin", (size_t)YOLO2_N_WEIGHTS);
    const std::vector<float> b = read_floats(cfg.weights_dir + "/bias.bin", (size_t)YOLO2_N_BIAS);
    std::vector<y2h::ImageU8> images;
    for (const std::string &f : files) images.push_back(y2h::load_image_u8(f));
    std::vector<const uint8_t *> ptrs;
    std::vector<int> ws, hs;
    for (const y2h::ImageU8 &im : images) { ptrs.push_back(im.rgb.data()); ws.push_back(im.w); hs.push_back(im.h); }
    const std::vector<std::vector<uint8_t>> frames = video ? read_video_frames(cfg) : std::vector<std::vector<uint8_t>>();
    for (const std::vector<uint8_t> &f : frames) { ptrs.push_back(f.data()); ws.push_back(cfg.video_w); hs.push_back(cfg.video_h); }

    yolo2_hip_ctx *ctx = nullptr;
    check(yolo2_hip_create(cfg.device, &ctx));
    struct Guard { yolo2_hip_ctx *c; ~Guard() { yolo2_hip_destroy(c); } } guard{ctx};
    check(yolo2_hip_load_weights_fp32(ctx, w.data(), w.size(), b.data(), b.size()));
    check(yolo2_hip_calib_images_pix_host(ctx, ptrs.data(), ws.data(), hs.data(), video ? cfg.video_pixfmt : YOLO2_PIX_RGB24, (int)ptrs.size(), cfg.batch));
    float act_max[YOLO2_N_CONV + 1], w_max[YOLO2_N_CONV], b_max[YOLO2_N_CONV];
    long seen = 0;
    check(yolo2_hip_calib_stats(ctx, act_max, w_max, b_max, &seen));
    if (cfg.format == "int8") {
        std::vector<int32_t> aq8(YOLO2_N_CONV + 1), wq8((size_t)YOLO2_N_BIAS), b32((size_t)YOLO2_N_BIAS);
        std::vector<int8_t> w8((size_t)YOLO2_N_WEIGHTS);
        check(yolo2_hip_calib_q8_tables(ctx, cfg.headroom, aq8.data()));
        check(yolo2_hip_quantize_weights_int8(ctx, aq8.data(), w8.data(), w8.size(), b32.data(), b32.size(), wq8.data()));
        std::printf("calibrated on %ld images (batch %d, headroom %g), int8\n", seen, cfg.batch, (double)cfg.headroom);
        std::printf("input        max|x| %-12.6g act_q %d\n", (double)act_max[0], aq8[0]);
        std::printf("%-5s %-14s %-12s %-14s %s\n", "conv", "max|w|", "weight_q", "max|out|", "act_q");
        size_t off = 0;
        for (int o = 0; o < YOLO2_N_CONV; ++o) {
            const auto mm = std::minmax_element(wq8.begin() + (long)off, wq8.begin() + (long)(off + (size_t)yolo2_bias_len[o]));
            std::printf("%-5d %-14.6g %3d..%-7d %-14.6g %d\n", o, (double)w_max[o], *mm.first, *mm.second, (double)act_max[o + 1], aq8[(size_t)o + 1]);
            off += (size_t)yolo2_bias_len[o];
        }
        std::filesystem::create_directories(cfg.out_dir);
        write_blob(cfg.out_dir + "/weights_int8.bin", w8);
        write_blob(cfg.out_dir + "/bias_int32.bin", b32);
        write_blob(cfg.out_dir + "/weight_int8_Q.bin", wq8);
        write_blob(cfg.out_dir + "/iofm_int8_Q.bin", aq8);
        std::printf("wrote weights_int8.bin, bias_int32.bin, weight_int8_Q.bin, iofm_int8_Q.bin to %s\n", cfg.out_dir.c_str());
        return 0;
    }
    std::vector<int32_t> wq(YOLO2_N_CONV), bq(YOLO2_N_CONV), aq(YOLO2_N_CONV + 1);
    check(yolo2_hip_calib_q_tables(ctx, cfg.headroom, wq.data(), bq.data(), aq.data()));
    std::vector<int16_t> wi((size_t)YOLO2_N_WEIGHTS), bi((size_t)YOLO2_N_BIAS);
    long clamped = 0;
    check(yolo2_hip_quantize_weights_int16(ctx, wq.data(), bq.data(), wi.data(), wi.size(), bi.data(), bi.size(), &clamped));

    std::printf("calibrated on %ld images (batch %d, headroom %g)\n", seen, cfg.batch, (double)cfg.headroom);
    std::printf("input        max|x| %-12.6g act_q %d\n", (double)act_max[0], aq[0]);
    std::printf("%-5s %-14s %-8s %-14s %-6s %-14s %s\n", "conv", "max|w|", "weight_q", "max|b|", "bias_q", "max|out|", "act_q");
    for (int o = 0; o < YOLO2_N_CONV; ++o)
        std::printf("%-5d %-14.6g %-8d %-14.6g %-6d %-14.6g %d\n", o, (double)w_max[o], wq[(size_t)o], (double)b_max[o], bq[(size_t)o],
                    (double)act_max[o + 1], aq[(size_t)o + 1]);
    std::printf("values clamped to +-32767: %ld\n", clamped);

    std::filesystem::create_directories(cfg.out_dir);
    write_blob(cfg.out_dir + "/weights_reorg_int16.bin", with_layer_pad(wi, yolo2_weight_len));
    write_blob(cfg.out_dir + "/bias_int16.bin", with_layer_pad(bi, yolo2_bias_len));
    write_blob(cfg.out_dir + "/weight_int16_Q.bin", wq);
    write_blob(cfg.out_dir + "/bias_int16_Q.bin", bq);
    write_blob(cfg.out_dir + "/iofm_Q.bin", aq);
    std::printf("wrote weights_reorg_int16.bin, bias_int16.bin, weight_int16_Q.bin, bias_int16_Q.bin, iofm_Q.bin to %s\n", cfg.out_dir.c_str());
    return 0;
}

}  // namespace

int main(int argc, char **argv)
{
    const Config cfg = parse_args(argc, argv);
    try {
        return run(cfg);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "yolov2_calibrate: %s\n", e.what());
        return 1;
    }
}
