// yolov2_detect -- the repo's own detection CLI with `--backend hip`.
//
// Same role and flags as the reference CLI (src/models/yolov2/yolov2_main.cpp:83-132, 234-335):
// parse cfg, load names, load + letterbox the image, run the accelerator path, dump the region
// tensors, decode boxes, NMS, draw, save.  The accelerator path is the HIP library behind its C ABI
// (include/yolo2_hip.h); there is no CPU backend here -- `--backend hls|cpu` names the reference's
// own binaries and is rejected with a pointer to them.
//
// Differences that are deliberate: images are decoded by the host's own JPEG / PNG decoder (y2_codec.cpp: the bytes the
// reference's stb_image produces, reproduced byte for byte; binary PPM/PGM are read too),
// the annotated result is written as PPM, boxes are also printed as text and (--json) JSON lines;
// `--batch N` runs the same frame N times through one batched call to show the batched entry.
//
// Streaming frontend (the role of the reference's yolo2_linux --video/--camera loop, linux_app/src/main.c:878-1288):
//   --input-list <file> | --input-dir <dir> | --video-raw <file|-> --video-width W --video-height H [--video-pix-fmt rgb24|yuyv422|nv12|yuv420p|bgr24|rgba|bgra]
//   | --video-mjpeg <file|-> (concatenated JPEG streams); --decode gpu sends baseline JPEG streams to the device compressed
// Frames are taken in chunks of --batch per device, go to the GPU as BYTES (letterbox on the GPU), through the
// int16 network on --devices a,b,... (contiguous frame shards, weights broadcast once by the library) and through the
// region + boxes + NMS tail (--post gpu: yolo2_hip_postprocess_int16; --post host: the threaded host code).  Per frame it
// prints the reference's "Frame %d (infer %d) inference time: %.2f ms" line (parsed by scripts/yolo2_report.py:685-729)
// and, with --jsonl <path> (--output-json is accepted too, the reference's name), writes one record per frame with the
// reference's fields (main.c:1028-1077): mode, source, frame_index, inference_index, width, height, detections[class_id,
// label, prob, bbox_norm{x,y,w,h}, bbox_px{x0,y0,x1,y1}].
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <map>
#include <fstream>
#include <algorithm>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/yolo2_hip.h"
#include "y2_host.hpp"

namespace {

struct AppConfig {
    std::string cfg_path = "config/yolov2.cfg";
    std::string names_path = "config/coco.names";
    std::string input_path = "examples/test_images/dog.jpg";
    std::string weights_dir = "weights";
    std::string output_prefix;
    float thresh = 0.25f;  // the reference's code default (its usage text says 0.5: yolov2_main.cpp:36,69)
    float nms = 0.45f;
    float hier_thresh = 0.5f;
    std::string backend = "hip";
    std::string precision = "int16";
    int batch = 1;
    int device = 0;
    bool json = false;
    // streaming frontend
    std::vector<int> devices;          // --devices a,b,...: frame shards over several GPUs
    std::string input_list, input_dir, video_raw, jsonl_path, save_dir;
    std::string video_mjpeg;        // --video-mjpeg: concatenated JPEG streams (a camera's MJPEG), cut where each stream ends
    std::string decode = "host";    // --decode: where JPEG streams are decoded - host (the decode pool) or gpu (yolo2_hip_run_images_jpeg_dets)
    bool annotate_gpu = false;   // --annotate-gpu: annotated frames come from yolo2_hip_annotate_images_pix_host, in the reference's look
    std::string annotated_format;   // --annotated-format jpg: they are encoded on the GPU too (yolo2_hip_annotate_images_pix_jpeg_host); "" / ppm: PPM;
                                    // nv12 / yuv420p (--loop-gpu): raw planar YUV 4:2:0 frames, converted by the painter (YOLO2_LOOP_OUT_NV12 / _I420)
    int jpeg_quality = 80;          // --jpeg-quality, the reference streamer's default
    bool loop_gpu = false;          // --loop-gpu: records and annotated frames from ONE accelerator call per chunk (yolo2_hip_loop_images_pix)
    int video_w = 640, video_h = 480;
    int video_pixfmt = YOLO2_PIX_RGB24; // --video-pix-fmt: what a --video-raw frame holds (RGB24, or packed YUYV 4:2:2 / planar NV12 / I420 / packed BGR24 / RGBA32 / BGRA32 read by the GPU as they are)
    int max_frames = 0;                // 0 = all
    int infer_every = 1;
    std::string post = "gpu";          // region + boxes + NMS: gpu | host
    std::string tail = "core";         // whose arithmetic the tail restates: the reference's src/core, or its camera loop's (linux_app)
    int chunk_batches = 4;             // batches per device and accelerator call (streaming)
    int decode_split = 0;              // --decode-split: option jpegdec_split of the GPU decoder (0: one lane per restart interval)
    int decode_threads = 0;            // image decode pool; 0 = all host cores
    bool strict = false;               // streaming: stop at the first undecodable input instead of skipping the frame
    bool plan_cache = true;            // int16: keep bounds / forms / timed conv plans of this weight set in <weights>/weights_reorg_int16.bin.y2plan
    bool streaming() const { return !input_list.empty() || !input_dir.empty() || !video_raw.empty() || !video_mjpeg.empty(); }
};

void print_usage(const char *prog)
{
    std::printf(
        "Usage: %s [options] [image]\n"
        "  --cfg <path>          Network cfg file (default: config/yolov2.cfg)\n"
        "  --names <path>        Class names file (default: config/coco.names)\n"
        "  --input <path>        Input image: JPEG (baseline / progressive), PNG, or binary PPM/PGM\n"
        "  --weights <dir>       Directory with weights_reorg_int16.bin, bias_int16.bin, *_Q.bin (default: weights)\n"
        "  --output <prefix>     Output file prefix without extension (default: results/<input>_prediction)\n"
        "  --thresh <float>      Confidence threshold (default: 0.25)\n"
        "  --nms <float>         NMS IoU threshold (default: 0.45)\n"
        "  --hier <float>        Hierarchical threshold (accepted, unused by region layers)\n"
        "  --backend <hip>       Backend selector (hip = MI355X library; hls/cpu live in the reference build)\n"
        "  --precision <int16|fp32|fp32fast|fp16|int8>  int16 = the batched fixed-point path; fp32 = the exact fp32 pass (tiled, batched);\n"
        "                            fp32fast = the fp32 weight files on the matrix cores in split-fp16 form (hi + lo halves, three MFMAs per\n"
        "                            product: boxes within 1e-3 of fp32's, ~7x the exact pass's rate); fp16 = fp16 operands, fp32 accumulate (approximate)\n"
        "                            int8 = the quantised pass on the i8 matrix cores; --weights names a directory written by\n"
        "                            yolov2_calibrate --format int8 (a single image, --batch, or streaming on one device: below)\n"
        "  --batch <n>           Frames per accelerator call (default 1)\n"
        "  --device <n>          HIP device (default 0)\n"
        "  --devices <a,b,..>    Several HIP devices: frames shard contiguously, weights are broadcast once (RCCL)\n"
        "  --json                Also print detections as JSON lines\n"
        "streaming (frames in chunks of --batch per device, bytes to the GPU, letterbox + network + NMS there):\n"
        "  --input-list <file>   One image path per line\n"
        "  --input-dir <dir>     Every *.jpg / *.jpeg / *.png / *.ppm / *.pgm of a directory, sorted by name\n"
        "  --video-raw <file|->  Raw RGB24 frames (e.g. from `ffmpeg -f rawvideo -pix_fmt rgb24 -`), with\n"
        "  --video-width <w> --video-height <h>   frame size (default 640x480)\n"
        "  --video-pix-fmt <rgb24|yuyv422>   what --video-raw holds (default rgb24).  yuyv422 (also: yuyv): packed YUYV 4:2:2, a V4L2 camera's\n"
        "                        native frames (`ffmpeg -f v4l2 -pix_fmt yuyv422 ... -f rawvideo -`), 2 bytes per pixel, even width; they go to\n"
        "                        the GPU as they are and are converted where they are read (every --precision, --devices)\n"
        "                        nv12 | yuv420p (also: i420): planar YUV 4:2:0, what video decoders emit (`ffmpeg -i file -f rawvideo -pix_fmt\n"
        "                        nv12 -`), w * h * 3 / 2 bytes per frame, even width and height; read and converted on the GPU the same way\n"
        "                        bgr24 | rgba | bgra (also: rgb0, bgr0 - the same layouts): packed B G R (OpenCV's frames), R G B X and B G R X\n"
        "                        (GUI toolkits, screen capture), 3 / 4 bytes per pixel, any size; the GPU picks the bytes where it reads the\n"
        "                        frame, the fourth byte is never used (every --precision, --annotate-gpu, --loop-gpu, --devices)\n"
        "  --video-mjpeg <file|->  Concatenated JPEG streams, what a camera delivers as MJPEG; each frame ends where its stream does\n"
        "  --decode <host|gpu>   Where JPEG streams are decoded (default host: the decode pool).  gpu, with --input-list, --input-dir or\n"
        "                        --video-mjpeg and --post gpu: baseline 1- and 3-component streams go to the device compressed and are decoded\n"
        "                        there (yolo2_hip_run_images_jpeg_dets); progressive / CMYK JPEG, PNG and PNM files are decoded on the pool and\n"
        "                        ride in the same call; a stream the GPU decoder flags is decoded on the host and run again.  Same log and\n"
        "                        JSONL.  With --save-annotated-dir only through --loop-gpu (yolo2_hip_loop_images_jpeg: the decoded frame is\n"
        "                        painted and encoded where the decoder left it); same files\n"
        "  --max-frames <n>      Stop after n inference frames (default: all)\n"
        "  --infer-every <n>     Run inference on every n-th frame (default 1)\n"
        "  --jsonl <path>        One JSON record per frame (fields of the reference's --output-json)\n"
        "  --save-annotated-dir <dir>   Write annotated frames as PPM\n"
        "  --annotate-gpu        with --save-annotated-dir: the frames are painted on the GPU right behind the detections, in the\n"
        "                        reference's look (boxes and \"<label> <prob>\" tags, labels from --names; yolo2_hip_annotate_images_pix_host);\n"
        "                        needs --post gpu\n"
        "  --annotated-format <ppm|jpg>  with --annotate-gpu: jpg writes frame_NNNNNN.jpg, the reference's MJPEG stream of the frame,\n"
        "                        encoded on the GPU (yolo2_hip_annotate_images_pix_jpeg_host); default ppm\n"
        "                        nv12 | yuv420p (also: i420), with --loop-gpu only: frame_NNNNNN.nv12 / frame_NNNNNN.yuv, the frame as raw planar\n"
        "                        YUV 4:2:0 (w * h * 3 / 2 bytes, even sizes; the names of --video-pix-fmt), converted where the GPU paints it;\n"
        "                        `cat` of the files is a rawvideo stream for a video encoder (ffmpeg -f rawvideo -pix_fmt nv12 | yuv420p)\n"
        "  --jpeg-quality <1..100>  quality of --annotated-format jpg (default 80)\n"
        "  --loop-gpu            with --annotate-gpu --save-annotated-dir and --post gpu: one accelerator call per chunk makes the records AND\n"
        "                        the annotated frames from one upload (yolo2_hip_loop_images_pix; with --decode gpu\n"
        "                        yolo2_hip_loop_images_jpeg, from the compressed streams); same log, JSONL and files\n"
        "  --chunk-batches <n>   Batches per device and accelerator call (default 4)\n"
        "  --decode-split <bytes> With --decode gpu: many lanes per restart interval, one per <bytes> of entropy-coded data (option\n"
        "                        jpegdec_split: a multiple of 16 in 16..4096; for streams without restart markers).  Same records.\n"
        "  --decode-threads <n>  Host threads decoding images ahead of the accelerators (default: all cores; one pool feeds every device)\n"
        "  --strict              Stop at the first input that cannot be read or decoded (default: log it, skip the frame, go on)\n"
        "  --no-plan-cache       int16: do not read / write <weights>/weights_reorg_int16.bin.y2plan (the weight set's bounds, forms and\n"
        "                        timed conv plans; with it a weight set is timed once and every later run uses the same kernels)\n"
        "  --post <gpu|host>     Where region + boxes + NMS run (default gpu; host: int16 only)\n"
        "  --tail <core|app>     Which of the reference's two detection tails: core = src/core (default), app = its camera loop's\n"
        "                        linux_app/src/yolo2_postprocess.c (float sigmoid / softmax / boxes, NMS at every --nms)\n"
        "  --precision int16 | fp16 | fp32fast   also when streaming: fp16 / fp32fast read weights_reorg.bin + bias.bin and run layers 0+1\n"
        "                        straight from the image bytes on the matrix cores (yolo2_hip_run_images_pix_dets_f16)\n"
        "  --precision int8      also when streaming (--input-list, --input-dir, --video-raw in any --video-pix-fmt), on one device with\n"
        "                        --post gpu: one kernel goes from the image bytes to layer 1 (yolo2_hip_run_images_pix_dets_int8); --jsonl,\n"
        "                        --tail app and --annotate-gpu --save-annotated-dir work as for fp16.  Refused: --loop-gpu and more than one\n"
        "                        device (the loop and multi-GPU entries have no int8 form)\n",
        prog);
}

AppConfig parse_args(int argc, char **argv)
{
    AppConfig cfg;
    for (int i = 1; i < argc; ++i) {
        const std::string arg(argv[i]);
        auto need = [&](const char *) { return i + 1 < argc; };
        if (arg == "--help" || arg == "-h") { print_usage(argv[0]); std::exit(0); }
        else if (arg == "--cfg" && need("")) cfg.cfg_path = argv[++i];
        else if (arg == "--names" && need("")) cfg.names_path = argv[++i];
        else if (arg == "--input" && need("")) cfg.input_path = argv[++i];
        else if (arg == "--weights" && need("")) cfg.weights_dir = argv[++i];
        else if (arg == "--output" && need("")) cfg.output_prefix = argv[++i];
        else if (arg == "--thresh" && need("")) cfg.thresh = std::strtof(argv[++i], nullptr);
        else if (arg == "--nms" && need("")) cfg.nms = std::strtof(argv[++i], nullptr);
        else if (arg == "--hier" && need("")) cfg.hier_thresh = std::strtof(argv[++i], nullptr);
        else if (arg == "--batch" && need("")) cfg.batch = std::atoi(argv[++i]);
        else if (arg == "--device" && need("")) cfg.device = std::atoi(argv[++i]);
        else if (arg == "--json") cfg.json = true;
        else if (arg == "--devices" && need("")) {
            std::string v = argv[++i];
            size_t pos = 0;
            while (pos <= v.size()) {
                const size_t c = v.find(',', pos);
                const std::string tok = v.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
                if (!tok.empty()) cfg.devices.push_back(std::atoi(tok.c_str()));
                if (c == std::string::npos) break;
                pos = c + 1;
            }
        }
        else if (arg == "--input-list" && need("")) cfg.input_list = argv[++i];
        else if (arg == "--input-dir" && need("")) cfg.input_dir = argv[++i];
        else if (arg == "--video-raw" && need("")) cfg.video_raw = argv[++i];
        else if (arg == "--video-mjpeg" && need("")) cfg.video_mjpeg = argv[++i];
        else if (arg == "--decode" && need("")) {
            cfg.decode = argv[++i];
            if (cfg.decode != "host" && cfg.decode != "gpu") { std::fprintf(stderr, "Unsupported --decode %s (host | gpu)\n", cfg.decode.c_str()); std::exit(1); }
        }
        else if (arg == "--video-width" && need("")) cfg.video_w = std::atoi(argv[++i]);
        else if (arg == "--video-height" && need("")) cfg.video_h = std::atoi(argv[++i]);
        else if (arg == "--video-pix-fmt" && need("")) {
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
        else if (arg == "--max-frames" && need("")) cfg.max_frames = std::atoi(argv[++i]);
        else if (arg == "--infer-every" && need("")) cfg.infer_every = std::max(1, std::atoi(argv[++i]));
        else if ((arg == "--jsonl" || arg == "--output-json") && need("")) cfg.jsonl_path = argv[++i];
        else if (arg == "--save-annotated-dir" && need("")) cfg.save_dir = argv[++i];
        else if (arg == "--annotate-gpu") cfg.annotate_gpu = true;
        else if (arg == "--loop-gpu") cfg.loop_gpu = true;
        else if (arg == "--annotated-format" && need("")) cfg.annotated_format = argv[++i];
        else if (arg == "--jpeg-quality" && need("")) cfg.jpeg_quality = std::atoi(argv[++i]);
        else if (arg == "--chunk-batches" && need("")) cfg.chunk_batches = std::max(1, std::atoi(argv[++i]));
        else if (arg == "--decode-threads" && need("")) cfg.decode_threads = std::atoi(argv[++i]);
        else if (arg == "--decode-split" && need("")) {
            cfg.decode_split = std::atoi(argv[++i]);
            if (cfg.decode_split < 16 || cfg.decode_split > 4096 || cfg.decode_split % 16) {
                std::fprintf(stderr, "Unsupported --decode-split %s (a multiple of 16 in 16..4096)\n", argv[i]);
                std::exit(1);
            }
        }
        else if (arg == "--strict") cfg.strict = true;
        else if (arg == "--no-plan-cache") cfg.plan_cache = false;
        else if (arg == "--post" && need("")) {
            cfg.post = argv[++i];
            if (cfg.post != "gpu" && cfg.post != "host") { std::fprintf(stderr, "Unsupported --post %s (gpu | host)\n", cfg.post.c_str()); std::exit(1); }
        } else if (arg == "--tail" && need("")) {
            cfg.tail = argv[++i];
            if (cfg.tail != "core" && cfg.tail != "app") { std::fprintf(stderr, "Unsupported --tail %s (core | app)\n", cfg.tail.c_str()); std::exit(1); }
        }
        else if (arg == "--backend" && need("")) {
            cfg.backend = argv[++i];
            if (cfg.backend != "hip") {
                std::fprintf(stderr, "Unsupported backend '%s'. This build provides 'hip' only; 'hls'/'cpu' are the reference's "
                             "own yolov2_detect.\n", cfg.backend.c_str());
                std::exit(1);
            }
        } else if (arg == "--precision" && need("")) {
            cfg.precision = argv[++i];
            if (cfg.precision == "float" || cfg.precision == "f32") cfg.precision = "fp32";
            if (cfg.precision == "i16" || cfg.precision == "fixed") cfg.precision = "int16";
            if (cfg.precision == "half" || cfg.precision == "f16") cfg.precision = "fp16";
            if (cfg.precision == "f32fast" || cfg.precision == "fp32tol") cfg.precision = "fp32fast";
            if (cfg.precision == "i8") cfg.precision = "int8";
            if (cfg.precision != "int16" && cfg.precision != "fp32" && cfg.precision != "fp16" && cfg.precision != "fp32fast" && cfg.precision != "int8") {
                std::fprintf(stderr, "Unsupported precision: %s (the hip backend runs int16, fp32, fp32fast, fp16 and int8)\n", cfg.precision.c_str());
                std::exit(1);
            }
        } else if (arg.rfind("--", 0) == 0) {
            std::fprintf(stderr, "Unknown option: %s\n", arg.c_str());
            print_usage(argv[0]);
            std::exit(1);
        } else cfg.input_path = arg;
    }
    if (cfg.loop_gpu && !(cfg.annotate_gpu && !cfg.save_dir.empty() && cfg.post == "gpu" && cfg.streaming())) {
        std::fprintf(stderr, "--loop-gpu joins the detections and the annotated frames of a streaming run: it needs --annotate-gpu, "
                             "--save-annotated-dir <dir> and --post gpu\n");
        std::exit(1);
    }
    if (cfg.precision == "int8" && cfg.streaming() && (cfg.loop_gpu || cfg.devices.size() > 1)) {
        std::fprintf(stderr, "--precision int8 streams on one device through the images entries only: the loop entries (--loop-gpu) and the "
                             "multi-GPU entries (--devices with more than one device) have no int8 form.\n");
        std::exit(1);
    }
    if (cfg.precision == "int8" && cfg.streaming() && !std::filesystem::exists(cfg.weights_dir + "/weights_int8.bin")) {
        // (before a device is opened or a frame is read: the int16 set that --weights usually names is not what this pass loads)
        std::fprintf(stderr, "--precision int8 when streaming: %s/weights_int8.bin not found; --weights names a directory written by "
                             "yolov2_calibrate --format int8\n", cfg.weights_dir.c_str());
        std::exit(1);
    }
    if (cfg.decode == "gpu" && (!(!cfg.input_list.empty() || !cfg.input_dir.empty() || !cfg.video_mjpeg.empty()) || cfg.post != "gpu" ||
                                (!cfg.save_dir.empty() && !cfg.loop_gpu))) {
        std::fprintf(stderr, "--decode gpu decodes the JPEG streams of --input-list, --input-dir or --video-mjpeg in front of --post gpu; "
                             "with --save-annotated-dir only through --loop-gpu (--annotate-gpu)\n");
        std::exit(1);
    }
    if (cfg.decode_split && cfg.decode != "gpu") {
        std::fprintf(stderr, "--decode-split is the GPU decoder's: it needs --decode gpu\n");
        std::exit(1);
    }
    if (cfg.video_pixfmt == YOLO2_PIX_YUYV && !cfg.video_raw.empty() && (cfg.video_w & 1)) {
        std::fprintf(stderr, "--video-pix-fmt yuyv422 needs an even --video-width, not %d\n", cfg.video_w);
        std::exit(1);
    }
    if ((cfg.video_pixfmt == YOLO2_PIX_NV12 || cfg.video_pixfmt == YOLO2_PIX_I420) && !cfg.video_raw.empty() && ((cfg.video_w | cfg.video_h) & 1)) {
        std::fprintf(stderr, "--video-pix-fmt %s needs an even --video-width and --video-height, not %dx%d\n",
                     cfg.video_pixfmt == YOLO2_PIX_NV12 ? "nv12" : "yuv420p", cfg.video_w, cfg.video_h);
        std::exit(1);
    }
    // a raw file says nothing about what it holds, so a file that cannot be read is reported here with what would have been read from
    // it, before anything is loaded (std::filesystem, not an open: the path may be a FIFO whose writer must not see a reader come and go)
    if (!cfg.video_raw.empty() && cfg.video_raw != "-") {
        std::error_code ec;
        if (!std::filesystem::exists(cfg.video_raw, ec) || std::filesystem::is_directory(cfg.video_raw, ec)) {
            const char *fmt = cfg.video_pixfmt == YOLO2_PIX_YUYV ? "yuyv422" : cfg.video_pixfmt == YOLO2_PIX_NV12 ? "nv12"
                              : cfg.video_pixfmt == YOLO2_PIX_I420 ? "yuv420p" : cfg.video_pixfmt == YOLO2_PIX_BGR24 ? "bgr24"
                              : cfg.video_pixfmt == YOLO2_PIX_RGBA32 ? "rgba" : cfg.video_pixfmt == YOLO2_PIX_BGRA32 ? "bgra" : "rgb24";
            std::fprintf(stderr, "Cannot read --video-raw %s (%dx%d frames, --video-pix-fmt %s)\n", cfg.video_raw.c_str(), cfg.video_w, cfg.video_h, fmt);
            std::exit(1);
        }
    }
    return cfg;
}

std::string default_output_prefix(const std::string &input_path)
{
    std::string base = std::filesystem::path(input_path).stem().string();
    return base + "_prediction";
}

void dump_floats(const char *path, const float *data, size_t n)
{
    FILE *fp = std::fopen(path, "w");
    if (!fp) { std::fprintf(stderr, "Warning: cannot open dump file %s\n", path); return; }
    for (size_t i = 0; i < n; ++i) std::fprintf(fp, "%.9g\n", data[i]);  // same format as yolo2_model.cpp:47
    std::fclose(fp);
    std::printf("Dumped %zu floats to %s\n", n, path);
}

// the parsed .cfg must be the network the batched entry implements
void check_topology(const y2h::Network &net)
{
    if ((int)net.layers.size() != yolo2_hip_num_layers()) throw std::runtime_error("cfg does not describe the 32-layer YOLOv2 network the hip backend implements");
    for (int i = 0; i < (int)net.layers.size(); ++i) {
        int d[9];
        yolo2_hip_layer_desc(i, d);
        const y2h::Layer &l = net.layers[i];
        bool ok = d[0] == (int)l.type;
        if (l.type == y2h::CONV) ok = ok && d[1] == l.c && d[2] == l.h && d[3] == l.w && d[4] == l.n && d[5] == l.size && d[6] == l.stride && d[7] == l.pad && d[8] == (int)l.leaky;
        if (l.type == y2h::MAXPOOL) ok = ok && d[1] == l.c && d[2] == l.h && d[3] == l.w && d[5] == l.size && d[6] == l.stride;
        if (l.type == y2h::REORG) ok = ok && d[1] == l.c && d[2] == l.h && d[6] == l.stride;
        int src[4];
        const int n_src = yolo2_hip_layer_routes(i, src);   // (0 for a layer that is no route: the cfg's list is empty there too)
        ok = ok && n_src == (int)l.route_layers.size() && std::equal(l.route_layers.begin(), l.route_layers.end(), src);
        if (!ok) throw std::runtime_error("cfg layer " + std::to_string(i) + " differs from the network the hip backend implements");
    }
}

// ---- JSONL records with the reference's fields (linux_app/src/main.c:1028-1077)
struct OutDet {
    int class_id;
    float prob;
    y2h::Box box;
};

void json_escaped(FILE *fp, const std::string &sv)
{
    std::fputc('"', fp);
    for (unsigned char ch : sv) {
        if (ch == '"' || ch == '\\') { std::fputc('\\', fp); std::fputc(ch, fp); }
        else if (ch < 0x20) std::fprintf(fp, "\\u%04x", ch);
        else std::fputc(ch, fp);
    }
    std::fputc('"', fp);
}

void write_jsonl(FILE *fp, const char *mode, const std::string &source, int frame_index, int infer_index, int w, int h,
                 const std::vector<OutDet> &dets, const std::vector<std::string> &names)
{
    std::fprintf(fp, "{\"mode\":\"%s\",\"source\":", mode);
    json_escaped(fp, source);
    std::fprintf(fp, ",\"frame_index\":%d,\"inference_index\":%d,\"width\":%d,\"height\":%d,\"detections\":[", frame_index, infer_index, w, h);
    bool first = true;
    for (const OutDet &d : dets) {
        const y2h::Box &b = d.box;
        const int x0 = (int)((b.x - b.w * 0.5f) * (float)w), y0 = (int)((b.y - b.h * 0.5f) * (float)h);
        const int x1 = (int)((b.x + b.w * 0.5f) * (float)w), y1 = (int)((b.y + b.h * 0.5f) * (float)h);
        if (!first) std::fputc(',', fp);
        first = false;
        std::fprintf(fp, "{\"class_id\":%d,\"label\":", d.class_id);
        json_escaped(fp, d.class_id < (int)names.size() ? names[(size_t)d.class_id] : "unknown");
        std::fprintf(fp, ",\"prob\":%.6f,\"bbox_norm\":{\"x\":%.6f,\"y\":%.6f,\"w\":%.6f,\"h\":%.6f},", d.prob, b.x, b.y, b.w, b.h);
        std::fprintf(fp, "\"bbox_px\":{\"x0\":%d,\"y0\":%d,\"x1\":%d,\"y1\":%d}}", x0, y0, x1, y1);
    }
    std::fprintf(fp, "]}\n");
    std::fflush(fp);
}

// the reference's rule for a record (main.c:1040-1052): a detection's best class, if its prob exceeds the threshold
std::vector<OutDet> best_class_dets(const std::vector<y2h::Detection> &dets, int total, int classes, float thresh)
{
    std::vector<OutDet> out;
    for (int i = 0; i < total; ++i) {
        int best = -1;
        float bp = 0.f;
        for (int j = 0; j < classes; ++j)
            if (dets[(size_t)i].prob[(size_t)j] > bp) { bp = dets[(size_t)i].prob[(size_t)j]; best = j; }
        if (bp <= thresh || best < 0) continue;
        out.push_back({best, bp, dets[(size_t)i].bbox});
    }
    return out;
}

// bytes of one --video-raw frame
static size_t video_frame_bytes(int w, int h, int pixfmt)
{
    const size_t px = (size_t)w * h;
    if (pixfmt == YOLO2_PIX_RGBA32 || pixfmt == YOLO2_PIX_BGRA32) return 4 * px;
    return pixfmt == YOLO2_PIX_YUYV ? 2 * px : (pixfmt == YOLO2_PIX_NV12 || pixfmt == YOLO2_PIX_I420 ? px * 3 / 2 : 3 * px);
}
// y2h::plain_box_frame's name for it
static int host_frame_fmt(int pixfmt)
{
    if (pixfmt == YOLO2_PIX_BGR24) return y2h::kFrameBgr24;
    if (pixfmt == YOLO2_PIX_RGBA32) return y2h::kFrameRgba32;
    if (pixfmt == YOLO2_PIX_BGRA32) return y2h::kFrameBgra32;
    return pixfmt == YOLO2_PIX_YUYV ? y2h::kFrameYuyv : pixfmt == YOLO2_PIX_NV12 ? y2h::kFrameNv12 : pixfmt == YOLO2_PIX_I420 ? y2h::kFrameI420 : y2h::kFrameRgb24;
}

struct SrcFrame {
    std::string source;
    int frame_index = 0;    // 1-based position in the stream
    y2h::ImageU8 img;       // (a --video-pix-fmt yuyv422 / nv12 / yuv420p frame: img.rgb holds its 2 w h / 1.5 w h bytes, as they were read; bgr24 / rgba / bgra likewise, 3 w h / 4 w h bytes)
    std::vector<uint8_t> jpeg;   // --video-mjpeg: the frame's stream; --decode gpu: the stream that goes to the device (img then has w, h only)
};

// Frame source: a list of image files, a directory, or a raw RGB24 stream.  next_ref() enumerates the frames selected for
// inference (--infer-every) WITHOUT decoding image files: the reader decodes a whole chunk in parallel (decode()).
class FrameSource {
  public:
    explicit FrameSource(const AppConfig &cfg) : cfg_(cfg)
    {
        namespace fs = std::filesystem;
        if (!cfg.input_list.empty()) {
            std::ifstream in(cfg.input_list);
            if (!in) throw std::runtime_error("Cannot open " + cfg.input_list);
            std::string line;
            while (std::getline(in, line)) {
                while (!line.empty() && (line.back() == '\r' || line.back() == ' ')) line.pop_back();
                if (!line.empty() && line[0] != '#') files_.push_back(line);
            }
            mode_ = "list";
        } else if (!cfg.input_dir.empty()) {
            for (const auto &e : fs::directory_iterator(cfg.input_dir)) {
                const std::string ext = e.path().extension().string();
                if (ext == ".ppm" || ext == ".pgm" || ext == ".jpg" || ext == ".jpeg" || ext == ".png") files_.push_back(e.path().string());
            }
            std::sort(files_.begin(), files_.end());
            mode_ = "dir";
        } else if (!cfg.video_mjpeg.empty()) {
            raw_ = cfg.video_mjpeg == "-" ? stdin : std::fopen(cfg.video_mjpeg.c_str(), "rb");
            if (!raw_) throw std::runtime_error("Cannot open " + cfg.video_mjpeg);
            mode_ = "mjpeg";
        } else {
            if (cfg.video_w <= 0 || cfg.video_h <= 0) throw std::runtime_error("--video-width / --video-height must be positive");
            raw_ = cfg.video_raw == "-" ? stdin : std::fopen(cfg.video_raw.c_str(), "rb");
            if (!raw_) throw std::runtime_error("Cannot open " + cfg.video_raw);
            mode_ = "video";
        }
        if (mode_ != "video" && mode_ != "mjpeg" && files_.empty()) throw std::runtime_error("no input images");
        gpu_decode = cfg.decode == "gpu";
    }
    ~FrameSource() { if (raw_ && raw_ != stdin) std::fclose(raw_); }
    const char *mode() const { return mode_.c_str(); }
    bool is_video() const { return mode_ == "video"; }
    // next frame selected for inference (honours --infer-every); false at the end of the stream.  Video frames arrive with
    // their pixels, image files with their path only.
    bool next_ref(SrcFrame &out)
    {
        for (;;) {
            SrcFrame f;
            if (mode_ == "video") {
                f.img.w = cfg_.video_w; f.img.h = cfg_.video_h;
                f.img.rgb.resize(video_frame_bytes(cfg_.video_w, cfg_.video_h, cfg_.video_pixfmt));
                const size_t rd = std::fread(f.img.rgb.data(), 1, f.img.rgb.size(), raw_);
                if (rd != f.img.rgb.size()) return false;    // EOF (a trailing partial frame is dropped like the reference's reader)
                f.source = cfg_.video_raw;
            } else if (mode_ == "mjpeg") {
                if (!next_mjpeg(f.jpeg)) return false;
                f.source = cfg_.video_mjpeg;
            } else {
                if (pos_ >= files_.size()) return false;
                f.source = files_[pos_++];
            }
            const bool take = (count_ % cfg_.infer_every) == 0;
            ++count_;
            if (!take) continue;
            f.frame_index = count_;
            out = std::move(f);
            return true;
        }
    }
    // One frame on the decode pool.  --decode host: the file (or the MJPEG frame's bytes) decoded as ever.  --decode gpu: a JPEG stream the
    // GPU decoder takes (yolo2_hip_jpeg_probe) stays compressed - f.jpeg, with its size in f.img - everything else is decoded here.
    static inline bool gpu_decode = false;
    static void decode(SrcFrame &f)
    {
        if (gpu_decode && f.jpeg.empty()) {     // a file: its bytes, if they are a JPEG stream
            std::ifstream in(f.source, std::ios::binary);
            std::vector<uint8_t> d((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
            if (d.size() >= 2 && d[0] == 0xff && d[1] == 0xd8) f.jpeg = std::move(d);
        }
        if (gpu_decode && !f.jpeg.empty()) {
            yolo2_hip_jpeg_info_t info;
            if (yolo2_hip_jpeg_probe(f.jpeg.data(), f.jpeg.size(), &info) == YOLO2_SUCCESS && info.gpu_decodable) {
                f.img.w = info.width; f.img.h = info.height;
                f.img.rgb.clear();
                return;
            }
        }
        if (!f.jpeg.empty()) {
            f.img = y2h::decode_image(f.jpeg.data(), f.jpeg.size(), f.source);
            f.jpeg.clear();
        } else {
            f.img = y2h::load_image_u8(f.source);
        }
    }

  private:
    // the next stream of a --video-mjpeg input: from its SOI to where yolo2_hip_jpeg_probe says it ends; bytes between streams are skipped
    bool next_mjpeg(std::vector<uint8_t> &out)
    {
        for (;;) {
            size_t soi = mj_at_;
            while (soi + 1 < mj_.size() && !(mj_[soi] == 0xff && mj_[soi + 1] == 0xd8)) ++soi;
            if (soi + 1 < mj_.size()) {
                yolo2_hip_jpeg_info_t info;
                yolo2_hip_jpeg_probe(mj_.data() + soi, mj_.size() - soi, &info);
                if (info.stream_bytes < mj_.size() - soi || mj_eof_) {     // the stream ends inside what has been read (or nothing more comes)
                    out.assign(mj_.begin() + (long)soi, mj_.begin() + (long)(soi + info.stream_bytes));
                    mj_at_ = soi + info.stream_bytes;
                    return true;
                }
            } else if (mj_eof_) {
                return false;
            }
            mj_.erase(mj_.begin(), mj_.begin() + (long)std::min(soi, mj_.size()));     // read on
            mj_at_ = 0;
            const size_t have = mj_.size(), more = std::max<size_t>((size_t)1 << 20, have);
            mj_.resize(have + more);
            const size_t rd = std::fread(mj_.data() + have, 1, more, raw_);
            mj_.resize(have + rd);
            if (rd == 0) mj_eof_ = true;
        }
    }
    std::vector<uint8_t> mj_;
    size_t mj_at_ = 0;
    bool mj_eof_ = false;
    const AppConfig &cfg_;
    std::vector<std::string> files_;
    size_t pos_ = 0;
    int count_ = 0;
    FILE *raw_ = nullptr;
    std::string mode_;
};

// a bounded hand-off between two pipeline stages
template <typename T>
class Channel {
  public:
    explicit Channel(size_t cap) : cap_(cap) {}
    void push(T v)
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_space_.wait(lk, [&] { return q_.size() < cap_ || closed_; });
        if (closed_) return;
        q_.push_back(std::move(v));
        cv_item_.notify_one();
    }
    bool pop(T &out)     // false once the channel is closed and drained
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_item_.wait(lk, [&] { return !q_.empty() || closed_; });
        if (q_.empty()) return false;
        out = std::move(q_.front());
        q_.pop_front();
        cv_space_.notify_one();
        return true;
    }
    void close()
    {
        std::lock_guard<std::mutex> lk(mu_);
        closed_ = true;
        cv_item_.notify_all();
        cv_space_.notify_all();
    }

  private:
    std::mutex mu_;
    std::condition_variable cv_item_, cv_space_;
    std::deque<T> q_;
    size_t cap_;
    bool closed_ = false;
};

struct Chunk {
    long seq = 0;                            // position in the stream: the writer emits chunks in this order
    int device_slot = 0;                     // which device lane ran it
    std::vector<SrcFrame> frames;            // frames whose image could not be decoded are dropped before the accelerator (see skipped)
    std::vector<std::pair<int, std::string>> skipped;   // (frame_index, reason)
    std::vector<std::vector<OutDet>> dets;   // filled by the accelerator stage
    std::vector<std::vector<uint8_t>> annotated;   // --annotate-gpu: the frames as RGB24 with boxes and tags, from the accelerator stage
    double seconds = 0;                      // wall time of the accelerator call for this chunk
};

// A pool of decode threads that lives as long as the stream (round 3 created and joined the threads per chunk).  decode()
// spreads the frames of one chunk over the pool and returns when all are done; a frame whose file cannot be read or decoded
// keeps an empty image and its reason in `error` - one bad file must not end a stream of thousands.
class DecodePool {
  public:
    explicit DecodePool(int n)
    {
        for (int i = 0; i < std::max(1, n); ++i) th_.emplace_back([this] { work(); });
    }
    ~DecodePool()
    {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_job_.notify_all();
        for (auto &t : th_) t.join();
    }
    int size() const { return (int)th_.size(); }
    void decode(std::vector<SrcFrame> &frames, std::vector<std::string> &errors)
    {
        errors.assign(frames.size(), std::string());
        std::unique_lock<std::mutex> lk(mu_);
        frames_ = &frames; errors_ = &errors; next_ = 0; left_ = frames.size();
        ++gen_;
        cv_job_.notify_all();
        cv_done_.wait(lk, [&] { return left_ == 0; });
        frames_ = nullptr;
    }

  private:
    void work()
    {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_job_.wait(lk, [&] { return stop_ || (frames_ && next_ < frames_->size()); });
            if (stop_) return;
            const size_t i = next_++;
            std::vector<SrcFrame> *fr = frames_;
            std::vector<std::string> *er = errors_;
            lk.unlock();
            try { FrameSource::decode((*fr)[i]); }
            catch (const std::exception &e) { (*er)[i] = e.what(); if ((*er)[i].empty()) (*er)[i] = "decode failed"; }
            lk.lock();
            if (--left_ == 0) cv_done_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable cv_job_, cv_done_;
    std::vector<SrcFrame> *frames_ = nullptr;
    std::vector<std::string> *errors_ = nullptr;
    size_t next_ = 0, left_ = 0;
    unsigned long gen_ = 0;
    bool stop_ = false;
};

// The streaming frontend as overlapped stages (the reference's loop, linux_app/src/main.c:878-1288, does them in turn per
// frame):  reader (file I/O + JPEG / PNG decode of the next chunk on a persistent pool of host threads)  ->  one ACCELERATOR LANE
// PER DEVICE (each pops the next decoded chunk from the shared queue: bytes in, letterbox + network + region / boxes / NMS on its
// device, detection records out - the region tensor never leaves HBM)  ->  writer (log lines, JSONL, annotated frames, in stream
// order).  Round 3 drove all devices from one call per chunk (every chunk was split over all devices and joined): a chunk was as
// slow as its slowest device and the reader fed them in lock step.  Now a chunk belongs to ONE device, devices take chunks as
// they become free (work-conserving, no join across devices), and the writer restores the order by chunk number.
// a float blob of at least `want` elements (weights_reorg.bin / bias.bin)
std::vector<float> read_floats(const std::string &path, size_t want)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("Cannot open " + path);
    const size_t n = (size_t)f.tellg() / sizeof(float);
    if (n < want) throw std::runtime_error(path + " is too small (" + std::to_string(n) + " floats, need " + std::to_string(want) + ")");
    std::vector<float> v(n);
    f.seekg(0);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(n * sizeof(float)));
    return v;
}

template <typename T>
std::vector<T> read_blob(const std::string &path, size_t want)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("Cannot open " + path);
    std::vector<T> v(want);
    f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(want * sizeof(T)));
    if ((size_t)f.gcount() != want * sizeof(T) || f.peek() != std::ifstream::traits_type::eof())
        throw std::runtime_error(path + " does not hold exactly " + std::to_string(want) + " elements");
    return v;
}

void run_stream(AppConfig cfg)
{
    namespace fs = std::filesystem;
    static char outbuf[1 << 16];
    std::setvbuf(stdout, outbuf, _IOFBF, sizeof(outbuf));    // thousands of frames a second: no write() per line
    // fp16 / fp32fast: the matrix-core passes from image bytes (yolo2_hip_run_images_pix_dets_f16), split = 0 / 1
    const bool f16 = cfg.precision == "fp16" || cfg.precision == "fp32fast";
    const int split = cfg.precision == "fp32fast" ? 1 : 0;
    // int8: the quantised pass from image bytes (yolo2_hip_run_images_pix_dets_int8), one device
    const bool i8 = cfg.precision == "int8";
    // what the frames' bytes are: decoded image files are RGB24, a raw video stream is what --video-pix-fmt says
    const int pixfmt = !cfg.video_raw.empty() && cfg.input_list.empty() && cfg.input_dir.empty() ? cfg.video_pixfmt : YOLO2_PIX_RGB24;
    const bool gpu_decode = cfg.decode == "gpu";
    if (cfg.precision != "int16" && !f16 && !i8) throw std::runtime_error("the streaming frontend runs the int16, fp16, fp32fast and int8 paths");
    if ((f16 || i8) && cfg.post == "host")
        throw std::runtime_error("--post host runs the int16 region tensor only; --precision " + cfg.precision + " needs --post gpu");
    if (cfg.devices.empty()) cfg.devices.push_back(cfg.device);
    if (cfg.batch <= 0) throw std::runtime_error("--batch must be positive");
    const bool annotate_gpu = cfg.annotate_gpu && !cfg.save_dir.empty();
    if (annotate_gpu && cfg.post != "gpu") throw std::runtime_error("--annotate-gpu paints the records of --post gpu");
    if (cfg.annotated_format == "i420") cfg.annotated_format = "yuv420p";
    const bool annotate_yuv = cfg.annotated_format == "nv12" || cfg.annotated_format == "yuv420p";
    if (!cfg.annotated_format.empty() && cfg.annotated_format != "ppm" && cfg.annotated_format != "jpg" && !annotate_yuv)
        throw std::runtime_error("--annotated-format is ppm, jpg, nv12 or yuv420p, not " + cfg.annotated_format);
    if (annotate_yuv && !cfg.loop_gpu)
        throw std::runtime_error("--annotated-format " + cfg.annotated_format + " needs --loop-gpu: the YUV 4:2:0 frames are made by the loop call's painter");
    const char *annotated_ext = cfg.annotated_format == "jpg" ? "jpg" : cfg.annotated_format == "nv12" ? "nv12" : annotate_yuv ? "yuv" : "ppm";
    const bool annotate_jpg = cfg.annotated_format == "jpg";
    if (annotate_jpg && !annotate_gpu) throw std::runtime_error("--annotated-format jpg encodes the frames of --annotate-gpu --save-annotated-dir");
    const y2h::Network net = y2h::parse_cfg(cfg.cfg_path);
    check_topology(net);
    const std::vector<std::string> names = y2h::load_names(cfg.names_path);
    const y2h::Layer &last = net.layers.back();
    std::vector<const char *> labels;
    for (const std::string &s : names) labels.push_back(s.c_str());
    FrameSource src(cfg);
    const int ndev = (int)cfg.devices.size();
    std::printf("YOLOv2 Object Detection - streaming (%s)\n  devices:", src.mode());
    for (int d : cfg.devices) std::printf(" %d", d);
    std::printf("\n  batch per device: %d\n  post-processing: %s (%s tail)\n", cfg.batch, cfg.post.c_str(), cfg.tail.c_str());

    yolo2_hip_multi *m = nullptr;
    if (yolo2_hip_multi_create(cfg.devices.data(), ndev, &m) != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
    struct Guard { yolo2_hip_multi *m; ~Guard() { yolo2_hip_multi_destroy(m); } } guard{m};
    if (i8) {   // the four files of yolov2_calibrate --format int8, on the one device
        if (ndev != 1 || cfg.loop_gpu) throw std::runtime_error("--precision int8 streams on one device, without --loop-gpu");
        const std::vector<int8_t> w = read_blob<int8_t>(cfg.weights_dir + "/weights_int8.bin", (size_t)YOLO2_N_WEIGHTS);
        const std::vector<int32_t> b = read_blob<int32_t>(cfg.weights_dir + "/bias_int32.bin", (size_t)YOLO2_N_BIAS);
        const std::vector<int32_t> wq = read_blob<int32_t>(cfg.weights_dir + "/weight_int8_Q.bin", (size_t)YOLO2_N_BIAS);
        const std::vector<int32_t> aq = read_blob<int32_t>(cfg.weights_dir + "/iofm_int8_Q.bin", (size_t)YOLO2_N_CONV + 1);
        if (yolo2_hip_load_weights_int8(yolo2_hip_multi_ctx(m, 0), w.data(), w.size(), b.data(), b.size(), wq.data(), aq.data()) != YOLO2_SUCCESS)
            throw std::runtime_error(yolo2_hip_last_error());
    } else if (f16) {
        const std::vector<float> w = read_floats(cfg.weights_dir + "/weights_reorg.bin", (size_t)YOLO2_N_WEIGHTS);
        const std::vector<float> b = read_floats(cfg.weights_dir + "/bias.bin", (size_t)YOLO2_N_BIAS);
        if (yolo2_hip_multi_load_weights_fp32(m, w.data(), w.size(), b.data(), b.size()) != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
    } else {
        // the weight-side cache (include/yolo2_hip.h): beside the interchange file, one per weight set, shared by every device
        if (cfg.plan_cache)
            for (int i = 0; i < yolo2_hip_multi_num_devices(m); ++i)
                if (yolo2_hip_set_plan_cache(yolo2_hip_multi_ctx(m, i), (cfg.weights_dir + "/weights_reorg_int16.bin.y2plan").c_str()) != YOLO2_SUCCESS)
                    throw std::runtime_error(yolo2_hip_last_error());
        std::vector<int> wlen(yolo2_weight_len, yolo2_weight_len + YOLO2_N_CONV), blen(yolo2_bias_len, yolo2_bias_len + YOLO2_N_CONV);
        const y2h::WeightsI16 wp = y2h::load_weights_int16(cfg.weights_dir, wlen, blen);
        if (yolo2_hip_multi_load_weights_int16(m, wp.weights.data(), wp.weights.size(), wp.bias.data(), wp.bias.size(), wp.weight_q.data(),
                                               (int)wp.weight_q.size(), wp.bias_q.data(), (int)wp.bias_q.size(), wp.act_q.data(),
                                               (int)wp.act_q.size()) != YOLO2_SUCCESS)
            throw std::runtime_error(yolo2_hip_last_error());
    }
    std::printf("  weights on %d device(s)%s\n", yolo2_hip_multi_num_devices(m), yolo2_hip_multi_uses_rccl(m) ? " (RCCL broadcast)" : "");
    auto plan_source_name = [](int s) { return s == 1 ? "plan table" : s == 2 ? "timed in this process" : s == 3 ? "static defaults" : s == 4 ? "forced" : s == 5 ? "weight cache" : "none"; };
    FILE *jf = nullptr;
    if (!cfg.jsonl_path.empty()) {
        jf = std::fopen(cfg.jsonl_path.c_str(), "w");
        if (!jf) throw std::runtime_error("Failed to open JSON output " + cfg.jsonl_path);
    }
    if (!cfg.save_dir.empty()) fs::create_directories(cfg.save_dir);

    // a chunk = what one accelerator call on ONE device takes: `chunk_batches` batches, so that the fill / drain of the call's
    // internal upload-compute-download pipeline is a small part of it
    const int chunk = cfg.batch * std::max(1, cfg.chunk_batches);
    const int threads = cfg.decode_threads > 0 ? cfg.decode_threads : (int)std::max(1u, std::thread::hardware_concurrency());
    std::printf("  decode threads: %d (host feed: one pool for all devices; the host side, not the GPUs, bounds a multi-device run - DESIGN.md 6)\n", threads);
    Channel<std::unique_ptr<Chunk>> to_run((size_t)2 * ndev), to_write((size_t)2 * ndev + 2);
    std::mutex err_mu;
    std::string err;
    auto fail_with = [&](const std::string &what) {
        { std::lock_guard<std::mutex> lk(err_mu); if (err.empty()) err = what; }
        to_run.close(); to_write.close();
    };
    const auto t_start = std::chrono::steady_clock::now();

    std::thread reader([&] {
        try {
            DecodePool pool(threads);
            int taken = 0;
            long seq = 0;
            bool more = true;
            // the first chunks are short (one batch, then doubling): the accelerators start after `batch` decoded images each
            int want = std::min(chunk, cfg.batch);
            std::vector<std::string> errors;
            while (more) {
                auto ck = std::make_unique<Chunk>();
                const int this_chunk = want;
                if (seq % ndev == ndev - 1) want = std::min(chunk, want * 2);     // every device has had a chunk of this size
                while ((int)ck->frames.size() < this_chunk && (cfg.max_frames <= 0 || taken + (int)ck->frames.size() < cfg.max_frames)) {
                    SrcFrame f;
                    if (!src.next_ref(f)) { more = false; break; }
                    ck->frames.push_back(std::move(f));
                }
                taken += (int)ck->frames.size();
                if (cfg.max_frames > 0 && taken >= cfg.max_frames) more = false;
                if (ck->frames.empty()) break;
                if (!src.is_video()) {     // decode the chunk's files on the pool
                    pool.decode(ck->frames, errors);
                    std::vector<SrcFrame> good;
                    good.reserve(ck->frames.size());
                    for (size_t i = 0; i < ck->frames.size(); ++i) {
                        if (errors[i].empty()) { good.push_back(std::move(ck->frames[i])); continue; }
                        if (cfg.strict) throw std::runtime_error(ck->frames[i].source + ": " + errors[i]);
                        ck->skipped.emplace_back(ck->frames[i].frame_index, ck->frames[i].source + ": " + errors[i]);
                    }
                    ck->frames = std::move(good);
                }
                ck->seq = seq++;
                to_run.push(std::move(ck));
            }
        } catch (const std::exception &e) { fail_with(e.what()); }
        to_run.close();
    });

    int infer_idx = 0, skipped_total = 0;
    std::thread writer([&] {
        try {
            std::unique_ptr<Chunk> ck;
            std::map<long, std::unique_ptr<Chunk>> held;      // chunks that arrived ahead of their turn (another device was faster)
            long next_seq = 0;
            auto emit = [&](Chunk &c) {
                for (const auto &sk : c.skipped) {
                    ++skipped_total;
                    std::printf("Frame %d skipped: %s\n", sk.first, sk.second.c_str());
                    std::fprintf(stderr, "Warning: frame %d skipped: %s\n", sk.first, sk.second.c_str());
                }
                const int n = (int)c.frames.size();
                for (int f = 0; f < n; ++f) {
                    ++infer_idx;
                    const SrcFrame &fr = c.frames[(size_t)f];
                    // the per-frame share of the chunk's wall time (the frames of a chunk run as one batched call)
                    std::printf("Frame %d (infer %d) inference time: %.2f ms\n", fr.frame_index, infer_idx, c.seconds * 1e3 / n);
                    for (const OutDet &d : c.dets[(size_t)f])
                        std::printf("  %s: %.0f%%  (x=%.4f y=%.4f w=%.4f h=%.4f)\n", d.class_id < (int)names.size() ? names[(size_t)d.class_id].c_str() : "?",
                                    d.prob * 100, d.box.x, d.box.y, d.box.w, d.box.h);
                    if (jf) write_jsonl(jf, src.mode(), fr.source, fr.frame_index, infer_idx, fr.img.w, fr.img.h, c.dets[(size_t)f], names);
                    if (annotate_gpu) {
                        char name[64];
                        std::snprintf(name, sizeof(name), "frame_%06d.%s", infer_idx, annotated_ext);
                        const std::string path = (fs::path(cfg.save_dir) / name).string();
                        FILE *pf = std::fopen(path.c_str(), "wb");
                        if (!pf) throw std::runtime_error("Cannot write " + path);
                        if (!annotate_jpg && !annotate_yuv) std::fprintf(pf, "P6\n%d %d\n255\n", fr.img.w, fr.img.h);   // (jpg, nv12, yuv: the bytes as they came)
                        std::fwrite(c.annotated[(size_t)f].data(), 1, c.annotated[(size_t)f].size(), pf);
                        std::fclose(pf);
                    } else if (!cfg.save_dir.empty()) {
                        std::vector<y2h::DrawRecord> recs;
                        for (const OutDet &d : c.dets[(size_t)f]) recs.push_back({0, 0, d.class_id, d.prob, d.box.x, d.box.y, d.box.w, d.box.h});
                        const y2h::Image im = y2h::plain_box_frame(fr.img.rgb.data(), fr.img.w, fr.img.h, host_frame_fmt(pixfmt), recs.data(),
                                                                   (int)recs.size(), last.classes);
                        char name[64];
                        std::snprintf(name, sizeof(name), "frame_%06d.ppm", infer_idx);
                        y2h::save_ppm(im, (fs::path(cfg.save_dir) / name).string());
                    }
                }
                std::fflush(stdout);
            };
            while (to_write.pop(ck)) {
                held[ck->seq] = std::move(ck);
                for (auto it = held.find(next_seq); it != held.end(); it = held.find(next_seq)) {
                    emit(*it->second);
                    held.erase(it);
                    ++next_seq;
                }
            }
            if (!held.empty() && err.empty()) throw std::runtime_error("stream ended with chunks out of order");
        } catch (const std::exception &e) { fail_with(e.what()); }
    });

    // ---- one accelerator lane per device
    std::vector<double> accel_s((size_t)ndev, 0.0);
    auto lane = [&](int slot) {
        try {
            yolo2_hip_ctx *ctx = yolo2_hip_multi_ctx(m, slot);
            if (cfg.decode_split && yolo2_hip_set_option(ctx, "jpegdec_split", std::to_string(cfg.decode_split).c_str()) != YOLO2_SUCCESS)
                throw std::runtime_error(yolo2_hip_last_error());
            // while the reader decodes its first chunk: plan the batch (activation tensors, lanes) on this device (int16; the fp16
            // passes build their launch table at the first chunk)
            if (!f16 && !i8) {
                if (yolo2_hip_set_batch(ctx, cfg.batch) != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
                if (slot == 0) std::printf("  conv plans: %s\n", plan_source_name(yolo2_hip_plan_source(ctx)));
            }
            std::unique_ptr<Chunk> ck;
            std::vector<int16_t> region;
            std::vector<yolo2_hip_det> recs;
            const int post_threads = std::max(1, threads / ndev);
            const int det_flags = YOLO2_DETS_BEST_CLASS | (cfg.tail == "app" ? YOLO2_DETS_APP_TAIL : 0);
            while (to_run.pop(ck)) {
                const int n = (int)ck->frames.size();
                ck->device_slot = slot;
                ck->dets.assign((size_t)n, {});
                if (n > 0) {
                    std::vector<const uint8_t *> ptrs((size_t)n);
                    std::vector<int> ws((size_t)n), hs((size_t)n);
                    for (int i = 0; i < n; ++i) { ptrs[(size_t)i] = ck->frames[(size_t)i].img.rgb.data(); ws[(size_t)i] = ck->frames[(size_t)i].img.w; hs[(size_t)i] = ck->frames[(size_t)i].img.h; }
                    int q = 0;
                    const auto t0 = std::chrono::steady_clock::now();
                    double t_annotate = 0;     // --annotate-gpu: upload, painting and download of the annotated frames, kept out of the inference time
                    if (cfg.post == "gpu") {
                        // one record per detection (its best class, main.c:1040-1052): at most 845 per frame, never truncated
                        const int cap = 845;
                        recs.resize((size_t)n * cap);
                        std::vector<int> counts((size_t)n);
                        // (--decode gpu) streams the decoder flagged: decoded on the host like any file, to be run again as raw frames;
                        // one that the host decoder cannot read either is skipped, as the reader skips such files
                        auto host_decode_flagged = [&](const std::vector<int> &redo) {
                            std::vector<int> again;
                            for (int i : redo) {
                                SrcFrame &fr = ck->frames[(size_t)i];
                                try {
                                    fr.img = y2h::decode_image(fr.jpeg.data(), fr.jpeg.size(), fr.source);
                                    fr.jpeg.clear();
                                    again.push_back(i);
                                } catch (const std::exception &e) {
                                    if (cfg.strict) throw std::runtime_error(fr.source + ": " + e.what());
                                    ck->skipped.emplace_back(fr.frame_index, fr.source + ": " + e.what());
                                    fr.frame_index = -1;      // dropped below
                                }
                            }
                            return again;
                        };
                        if (cfg.loop_gpu) {     // records and annotated frames from one call: the frames go up once
                            ck->annotated.resize((size_t)n);
                            const int prec = f16 ? (split ? YOLO2_LOOP_F32TOL : YOLO2_LOOP_FP16) : YOLO2_LOOP_INT16;
                            // one loop call over the frames `idx` of the chunk - with --decode gpu the streams go up compressed and the pool's
                            // frames ride along as raw frames (size 0); returns the frames whose scan the GPU decoder flagged
                            auto loop_call = [&](const std::vector<int> &idx) {
                                const int m2 = (int)idx.size();
                                std::vector<const uint8_t *> p2((size_t)m2);
                                std::vector<size_t> s2((size_t)m2, 0), caps((size_t)m2), sizes((size_t)m2);
                                std::vector<int> w2((size_t)m2), h2((size_t)m2), c2((size_t)m2), st2((size_t)m2, 0);
                                std::vector<yolo2_hip_det> r2((size_t)m2 * cap);
                                std::vector<uint8_t *> outs((size_t)m2);
                                for (int k = 0; k < m2; ++k) {
                                    const SrcFrame &fr = ck->frames[(size_t)idx[(size_t)k]];
                                    p2[(size_t)k] = fr.jpeg.empty() ? fr.img.rgb.data() : fr.jpeg.data();
                                    s2[(size_t)k] = fr.jpeg.size();
                                    w2[(size_t)k] = fr.img.w; h2[(size_t)k] = fr.img.h;
                                }
                                for (int attempt = 0; attempt < 2; ++attempt) {     // (JPEG: room as below, a second call with the encoder's bound)
                                    for (int k = 0; k < m2; ++k) {
                                        std::vector<uint8_t> &a = ck->annotated[(size_t)idx[(size_t)k]];
                                        const size_t raw = (size_t)w2[(size_t)k] * h2[(size_t)k] * 3 / (annotate_yuv ? 2 : 1), bound = yolo2_hip_jpeg_bound(w2[(size_t)k], h2[(size_t)k]);
                                        caps[(size_t)k] = !annotate_jpg ? raw : attempt ? bound : std::min(bound, raw + 4096);
                                        a.resize(caps[(size_t)k]);
                                        outs[(size_t)k] = a.data();
                                        sizes[(size_t)k] = 0;
                                    }
                                    const int fmt = annotate_jpg ? YOLO2_LOOP_OUT_JPEG : cfg.annotated_format == "nv12" ? YOLO2_LOOP_OUT_NV12
                                                    : annotate_yuv ? YOLO2_LOOP_OUT_I420 : YOLO2_LOOP_OUT_RGB24;
                                    const int rc = gpu_decode ? yolo2_hip_loop_images_jpeg(ctx, prec, p2.data(), s2.data(), w2.data(), h2.data(), m2, cfg.batch, cfg.thresh,
                                                                                           cfg.nms, det_flags, r2.data(), cap, c2.data(), &q, labels.data(),
                                                                                           (int)labels.size(), fmt, cfg.jpeg_quality, outs.data(), caps.data(),
                                                                                           sizes.data(), nullptr, st2.data())
                                                              : yolo2_hip_loop_images_pix(ctx, prec, p2.data(), w2.data(), h2.data(), pixfmt, m2, cfg.batch, cfg.thresh,
                                                                                          cfg.nms, det_flags, r2.data(), cap, c2.data(), &q, labels.data(),
                                                                                          (int)labels.size(), fmt, cfg.jpeg_quality, outs.data(), caps.data(),
                                                                                          sizes.data(), nullptr);
                                    if (rc == YOLO2_SUCCESS) break;
                                    bool too_small = false, flagged = false;
                                    for (int k = 0; k < m2; ++k) {
                                        too_small = too_small || sizes[(size_t)k] > caps[(size_t)k];
                                        flagged = flagged || st2[(size_t)k] != 0;
                                    }
                                    if (!attempt && annotate_jpg && too_small) continue;
                                    if (too_small || !flagged) throw std::runtime_error(yolo2_hip_last_error());
                                    break;     // (complete but for the flagged frames)
                                }
                                std::vector<int> redo;
                                for (int k = 0; k < m2; ++k) {
                                    const int i = idx[(size_t)k];
                                    if (st2[(size_t)k]) { redo.push_back(i); continue; }
                                    counts[(size_t)i] = c2[(size_t)k];
                                    std::copy(r2.begin() + (long)k * cap, r2.begin() + (long)k * cap + std::min(c2[(size_t)k], cap), recs.begin() + (long)i * cap);
                                    ck->annotated[(size_t)i].resize(sizes[(size_t)k]);
                                    ck->annotated[(size_t)i].shrink_to_fit();
                                }
                                return redo;
                            };
                            std::vector<int> all((size_t)n);
                            for (int i = 0; i < n; ++i) all[(size_t)i] = i;
                            const std::vector<int> again = host_decode_flagged(loop_call(all));
                            if (!again.empty() && !loop_call(again).empty()) throw std::runtime_error("a raw frame came back flagged by the JPEG decoder");
                        } else if (gpu_decode) {
                            // streams the GPU decoder takes go up compressed, the pool's frames ride along as raw frames (size 0)
                            const int prec = i8 ? YOLO2_JPEG_INT8 : f16 ? (split ? YOLO2_LOOP_F32TOL : YOLO2_LOOP_FP16) : YOLO2_LOOP_INT16;
                            std::vector<size_t> sizes((size_t)n);
                            std::vector<int> status((size_t)n, 0);
                            for (int i = 0; i < n; ++i) {
                                SrcFrame &fr = ck->frames[(size_t)i];
                                sizes[(size_t)i] = fr.jpeg.size();
                                if (!fr.jpeg.empty()) ptrs[(size_t)i] = fr.jpeg.data();
                            }
                            int rc = yolo2_hip_run_images_jpeg_dets(ctx, prec, ptrs.data(), sizes.data(), ws.data(), hs.data(), n, cfg.batch, cfg.thresh, cfg.nms,
                                                                    det_flags, recs.data(), cap, counts.data(), &q, status.data());
                            std::vector<int> redo;
                            for (int i = 0; i < n; ++i) if (status[(size_t)i]) redo.push_back(i);
                            if (rc != YOLO2_SUCCESS && redo.empty()) throw std::runtime_error(yolo2_hip_last_error());
                            // a stream the decoder flagged: decoded on the host like any file, and run again as a raw frame
                            const std::vector<int> again = host_decode_flagged(redo);
                            if (!again.empty()) {
                                const int m2 = (int)again.size();
                                std::vector<const uint8_t *> p2((size_t)m2);
                                std::vector<size_t> s2((size_t)m2, 0);
                                std::vector<int> w2((size_t)m2), h2((size_t)m2), c2((size_t)m2), st2((size_t)m2);
                                std::vector<yolo2_hip_det> r2((size_t)m2 * cap);
                                for (int k = 0; k < m2; ++k) {
                                    const SrcFrame &fr = ck->frames[(size_t)again[(size_t)k]];
                                    p2[(size_t)k] = fr.img.rgb.data(); w2[(size_t)k] = fr.img.w; h2[(size_t)k] = fr.img.h;
                                }
                                if (yolo2_hip_run_images_jpeg_dets(ctx, prec, p2.data(), s2.data(), w2.data(), h2.data(), m2, cfg.batch, cfg.thresh, cfg.nms, det_flags,
                                                                   r2.data(), cap, c2.data(), &q, st2.data()) != YOLO2_SUCCESS)
                                    throw std::runtime_error(yolo2_hip_last_error());
                                for (int k = 0; k < m2; ++k) {
                                    const int i = again[(size_t)k];
                                    counts[(size_t)i] = c2[(size_t)k];
                                    std::copy(r2.begin() + (long)k * cap, r2.begin() + (long)k * cap + std::min(c2[(size_t)k], cap), recs.begin() + (long)i * cap);
                                }
                            }
                        } else {
                            const int rc = i8 ? yolo2_hip_run_images_pix_dets_int8(ctx, ptrs.data(), ws.data(), hs.data(), pixfmt, n, cfg.batch, cfg.thresh, cfg.nms,
                                                                                   det_flags, recs.data(), cap, counts.data())
                                           : f16 ? yolo2_hip_run_images_pix_dets_f16(ctx, split, ptrs.data(), ws.data(), hs.data(), pixfmt, n, cfg.batch, cfg.thresh,
                                                                                   cfg.nms, det_flags, recs.data(), cap, counts.data())
                                               : yolo2_hip_run_images_pix_dets(ctx, ptrs.data(), ws.data(), hs.data(), pixfmt, n, cfg.batch, cfg.thresh, cfg.nms,
                                                                               det_flags, recs.data(), cap, counts.data(), &q);
                            if (rc != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
                        }
                        const auto t_dets = std::chrono::steady_clock::now();
                        if (cfg.loop_gpu) {     // (the call above made the frames)
                        } else if (annotate_gpu && annotate_jpg) {     // painted and encoded on the GPU: only the streams come back
                            ck->annotated.resize((size_t)n);
                            std::vector<uint8_t *> outs((size_t)n);
                            std::vector<size_t> caps((size_t)n), sizes((size_t)n);
                            // room for the raw frame's size; a frame that compresses to more than that (noise at quality 100) gets a
                            // second call with the encoder's bound
                            for (int attempt = 0; attempt < 2; ++attempt) {
                                for (int f = 0; f < n; ++f) {
                                    const size_t bound = yolo2_hip_jpeg_bound(ws[(size_t)f], hs[(size_t)f]);
                                    caps[(size_t)f] = attempt ? bound : std::min(bound, (size_t)ws[(size_t)f] * hs[(size_t)f] * 3 + 4096);
                                    ck->annotated[(size_t)f].resize(caps[(size_t)f]);
                                    outs[(size_t)f] = ck->annotated[(size_t)f].data();
                                    sizes[(size_t)f] = 0;
                                }
                                const int rc = yolo2_hip_annotate_images_pix_jpeg_host(ctx, ptrs.data(), ws.data(), hs.data(), pixfmt, n, cfg.batch, recs.data(),
                                                                                       cap, counts.data(), cfg.thresh, labels.data(), (int)labels.size(),
                                                                                       cfg.jpeg_quality, outs.data(), caps.data(), sizes.data(), nullptr);
                                if (rc == YOLO2_SUCCESS) break;
                                bool too_small = false;
                                for (int f = 0; f < n; ++f) too_small = too_small || sizes[(size_t)f] > caps[(size_t)f];
                                if (attempt || !too_small) throw std::runtime_error(yolo2_hip_last_error());
                            }
                            for (int f = 0; f < n; ++f) {
                                ck->annotated[(size_t)f].resize(sizes[(size_t)f]);
                                ck->annotated[(size_t)f].shrink_to_fit();
                            }
                        } else if (annotate_gpu) {     // the chunk's frames with these records painted in, while both are at hand
                            ck->annotated.resize((size_t)n);
                            std::vector<uint8_t *> outs((size_t)n);
                            for (int f = 0; f < n; ++f) {
                                ck->annotated[(size_t)f].resize((size_t)ws[(size_t)f] * hs[(size_t)f] * 3);
                                outs[(size_t)f] = ck->annotated[(size_t)f].data();
                            }
                            if (yolo2_hip_annotate_images_pix_host(ctx, ptrs.data(), ws.data(), hs.data(), pixfmt, n, cfg.batch, recs.data(), cap, counts.data(),
                                                                   cfg.thresh, labels.data(), (int)labels.size(), outs.data(), nullptr) != YOLO2_SUCCESS)
                                throw std::runtime_error(yolo2_hip_last_error());
                        }
                        t_annotate = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_dets).count();
                        for (int f = 0; f < n; ++f) {
                            if (counts[(size_t)f] > cap) throw std::runtime_error("detection records truncated");   // cannot happen in best-class mode
                            for (int k = 0; k < counts[(size_t)f]; ++k) {
                                const yolo2_hip_det &r = recs[(size_t)f * cap + k];
                                if (r.prob > cfg.thresh) ck->dets[(size_t)f].push_back({r.cls, r.prob, {r.x, r.y, r.w, r.h}});
                            }
                        }
                    } else {
                        region.resize((size_t)n * YOLO2_REGION_ELEMS);
                        if (yolo2_hip_run_images_pix_host(ctx, ptrs.data(), ws.data(), hs.data(), pixfmt, n, cfg.batch, region.data(), &q) != YOLO2_SUCCESS)
                            throw std::runtime_error(yolo2_hip_last_error());
                        auto all = cfg.tail == "app" ? y2h::postprocess_batch_app(region.data(), n, q, ws.data(), hs.data(), cfg.thresh, cfg.nms, post_threads)
                                                     : y2h::postprocess_batch(region.data(), n, q, ws.data(), hs.data(), cfg.thresh, cfg.nms, post_threads);
                        for (int f = 0; f < n; ++f) ck->dets[(size_t)f] = best_class_dets(all[(size_t)f], (int)all[(size_t)f].size(), last.classes, cfg.thresh);
                    }
                    for (int f = n - 1; f >= 0; --f)     // (--decode gpu) frames that neither decoder could read: skipped, as the reader skips them
                        if (ck->frames[(size_t)f].frame_index < 0) {
                            ck->frames.erase(ck->frames.begin() + f);
                            ck->dets.erase(ck->dets.begin() + f);
                            if (!ck->annotated.empty()) ck->annotated.erase(ck->annotated.begin() + f);
                        }
                    ck->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() - t_annotate;
                    accel_s[(size_t)slot] += ck->seconds;
                }
                to_write.push(std::move(ck));
            }
        } catch (const std::exception &e) { fail_with(e.what()); }
    };
    std::vector<std::thread> lanes;
    for (int i = 1; i < ndev; ++i) lanes.emplace_back(lane, i);
    lane(0);                                   // device 0's lane runs on this thread
    for (auto &t : lanes) t.join();
    to_write.close();
    to_run.close();
    reader.join();
    writer.join();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    if (jf) std::fclose(jf);
    if (!err.empty()) throw std::runtime_error(err);
    if (infer_idx == 0) throw std::runtime_error("No inference frames processed");
    const double busiest = *std::max_element(accel_s.begin(), accel_s.end());
    if (skipped_total) std::printf("\n%d frame(s) skipped: undecodable input (use --strict to stop at the first one)\n", skipped_total);
    std::printf("\nStreaming inference completed successfully (%d inference frames; %.1f frames/s end to end incl. file I/O, decode and "
                "output; %.1f frames/s inside the accelerator calls)\n", infer_idx, infer_idx / std::max(wall, 1e-9), infer_idx / std::max(busiest, 1e-9));
    std::fflush(stdout);
}

void run_detector(AppConfig cfg)
{
    if (cfg.streaming()) { run_stream(cfg); return; }
    std::setbuf(stdout, nullptr);
    namespace fs = std::filesystem;
    if (cfg.output_prefix.empty()) cfg.output_prefix = default_output_prefix(cfg.input_path);
    {
        fs::path prefix(cfg.output_prefix);
        if (!prefix.has_parent_path()) { fs::create_directories("results"); prefix = fs::path("results") / prefix; }
        else fs::create_directories(prefix.parent_path());
        cfg.output_prefix = prefix.string();
    }
    std::printf("YOLOv2 Object Detection - Starting\n  cfg:    %s\n  names:  %s\n  input:  %s\n  precision: %s\n  backend: hip (device %d, batch %d)\n  output: %s[.ppm]\n",
                cfg.cfg_path.c_str(), cfg.names_path.c_str(), cfg.input_path.c_str(), cfg.precision.c_str(), cfg.device, cfg.batch,
                cfg.output_prefix.c_str());

    const y2h::Network net = y2h::parse_cfg(cfg.cfg_path);
    check_topology(net);
    const std::vector<std::string> names = y2h::load_names(cfg.names_path);
    y2h::Image im = y2h::load_image(cfg.input_path);   // load_image_stb(path, 3) of the reference, own decoders
    std::printf("Input img: %s (w=%d, h=%d, c=%d)\n", cfg.input_path.c_str(), im.w, im.h, im.c);
    const y2h::Image sized = y2h::letterbox_image(im, net.w, net.h);

    const y2h::Layer &last = net.layers.back();
    std::vector<float> raw(YOLO2_REGION_ELEMS), proc(YOLO2_REGION_ELEMS);
    yolo2_hip_ctx *ctx = nullptr;
    if (yolo2_hip_create(cfg.device, &ctx) != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
    double elapsed = 0;
    int frames_run = cfg.batch;
    if (cfg.precision == "fp32" || cfg.precision == "fp16" || cfg.precision == "fp32fast") {
        // weights/weights_reorg.bin + weights/bias.bin, the files load_weights() reads at Precision::FP32 (yolo2_model.cpp:171-183)
        const std::vector<float> w = read_floats(cfg.weights_dir + "/weights_reorg.bin", (size_t)YOLO2_N_WEIGHTS);
        const std::vector<float> b = read_floats(cfg.weights_dir + "/bias.bin", (size_t)YOLO2_N_BIAS);
        if (yolo2_hip_load_weights_fp32(ctx, w.data(), w.size(), b.data(), b.size()) != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
        // the tiled exact fp32 pass (bit-identical to the reference's fp32 path); --batch N repeats the frame like the int16 branch
        std::vector<float> frames((size_t)cfg.batch * YOLO2_FRAME_ELEMS), regions((size_t)cfg.batch * YOLO2_REGION_ELEMS);
        for (int b = 0; b < cfg.batch; ++b) std::memcpy(frames.data() + (size_t)b * YOLO2_FRAME_ELEMS, sized.data.data(), sizeof(float) * YOLO2_FRAME_ELEMS);
        const auto t0 = std::chrono::high_resolution_clock::now();
        // (fp16: the MFMA path on the same weights - not the reference's arithmetic, max |error| ~0.006 on a +-4.7 region tensor)
        const int rc = cfg.precision == "fp16" ? yolo2_hip_run_batch_fp16_host(ctx, frames.data(), cfg.batch, regions.data())
                       : cfg.precision == "fp32fast" ? yolo2_hip_run_batch_f32tol_host(ctx, frames.data(), cfg.batch, regions.data())
                                                     : yolo2_hip_run_batch_fp32_host(ctx, frames.data(), cfg.batch, regions.data());
        if (rc != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
        elapsed = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        std::memcpy(raw.data(), regions.data(), sizeof(float) * YOLO2_REGION_ELEMS);
    } else if (cfg.precision == "int8") {
        // the four files of yolov2_calibrate --format int8: natural-order int8 weights, int32 biases, per-channel weight Qs, 24 tensor Qs
        const std::vector<int8_t> w = read_blob<int8_t>(cfg.weights_dir + "/weights_int8.bin", (size_t)YOLO2_N_WEIGHTS);
        const std::vector<int32_t> b = read_blob<int32_t>(cfg.weights_dir + "/bias_int32.bin", (size_t)YOLO2_N_BIAS);
        const std::vector<int32_t> wq = read_blob<int32_t>(cfg.weights_dir + "/weight_int8_Q.bin", (size_t)YOLO2_N_BIAS);
        const std::vector<int32_t> aq = read_blob<int32_t>(cfg.weights_dir + "/iofm_int8_Q.bin", (size_t)YOLO2_N_CONV + 1);
        if (yolo2_hip_load_weights_int8(ctx, w.data(), w.size(), b.data(), b.size(), wq.data(), aq.data()) != YOLO2_SUCCESS)
            throw std::runtime_error(yolo2_hip_last_error());
        std::vector<float> frames((size_t)cfg.batch * YOLO2_FRAME_ELEMS), regions((size_t)cfg.batch * YOLO2_REGION_ELEMS);
        for (int f = 0; f < cfg.batch; ++f) std::memcpy(frames.data() + (size_t)f * YOLO2_FRAME_ELEMS, sized.data.data(), sizeof(float) * YOLO2_FRAME_ELEMS);
        const auto t0 = std::chrono::high_resolution_clock::now();
        if (yolo2_hip_run_batch_int8_host(ctx, frames.data(), cfg.batch, regions.data()) != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
        elapsed = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        std::memcpy(raw.data(), regions.data(), sizeof(float) * YOLO2_REGION_ELEMS);   // a float region tensor: the float tail below
    } else {
        std::vector<int> wlen(yolo2_weight_len, yolo2_weight_len + YOLO2_N_CONV), blen(yolo2_bias_len, yolo2_bias_len + YOLO2_N_CONV);
        const y2h::WeightsI16 wp = y2h::load_weights_int16(cfg.weights_dir, wlen, blen);
        if (cfg.plan_cache && yolo2_hip_set_plan_cache(ctx, (cfg.weights_dir + "/weights_reorg_int16.bin.y2plan").c_str()) != YOLO2_SUCCESS)
            throw std::runtime_error(yolo2_hip_last_error());
        if (yolo2_hip_load_weights_int16(ctx, wp.weights.data(), wp.weights.size(), wp.bias.data(), wp.bias.size(), wp.weight_q.data(),
                                         (int)wp.weight_q.size(), wp.bias_q.data(), (int)wp.bias_q.size(), wp.act_q.data(),
                                         (int)wp.act_q.size()) != YOLO2_SUCCESS)
            throw std::runtime_error(yolo2_hip_last_error());
        if (yolo2_hip_set_batch(ctx, cfg.batch) != YOLO2_SUCCESS) throw std::runtime_error(yolo2_hip_last_error());
        std::vector<float> frames((size_t)cfg.batch * YOLO2_FRAME_ELEMS);
        for (int b = 0; b < cfg.batch; ++b) std::memcpy(frames.data() + (size_t)b * YOLO2_FRAME_ELEMS, sized.data.data(), sizeof(float) * YOLO2_FRAME_ELEMS);
        std::vector<int16_t> region((size_t)cfg.batch * YOLO2_REGION_ELEMS);
        int q = 0;
        const auto t0 = std::chrono::high_resolution_clock::now();
        if (yolo2_hip_run_batch_int16_host(ctx, frames.data(), cfg.batch, region.data(), &q) != YOLO2_SUCCESS)
            throw std::runtime_error(yolo2_hip_last_error());
        elapsed = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
        // dequantise (yolo2_model.cpp:415-421)
        const float scale = std::ldexp(1.0f, -q);
        for (int t = 0; t < YOLO2_REGION_ELEMS; ++t) raw[t] = (float)region[t] * scale;
    }
    std::printf("%s: Predicted in %.3f seconds.\n", cfg.input_path.c_str(), elapsed);
    std::printf("inference time: %.2f ms\n", elapsed * 1e3 / frames_run);  // line format parsed by scripts/yolo2_report.py:685-729
    yolo2_hip_destroy(ctx);

    // dumps with the reference's env-var names (yolo2_model.cpp:426-439, yolov2_main.cpp:297-306)
    const char *nd = std::getenv("YOLO2_NO_DUMP");
    const bool do_dump = !(nd && nd[0] && nd[0] != '0');
    const char *raw_path = std::getenv("YOLO2_DUMP_REGION_RAW");
    if (!raw_path || !raw_path[0]) raw_path = "yolov2_region_raw_hip.txt";
    if (do_dump) dump_floats(raw_path, raw.data(), raw.size());
    const bool app_tail = cfg.tail == "app";
    if (app_tail) y2h::app_region_forward(last, raw.data(), proc.data());
    else y2h::region_forward(last, raw.data(), proc.data());
    const char *proc_path = std::getenv("YOLO2_DUMP_REGION");
    if (!proc_path || !proc_path[0]) proc_path = "yolov2_region_proc_hip.txt";
    if (do_dump) dump_floats(proc_path, proc.data(), proc.size());

    std::vector<y2h::Detection> dets = app_tail ? y2h::app_region_detections(last, proc.data(), im.w, im.h, net.w, net.h, cfg.thresh)
                                                : y2h::region_boxes(last, proc.data(), im.w, im.h, net.w, net.h, cfg.thresh);
    int total = (int)dets.size();
    if (app_tail) { if (total > 0) total = y2h::app_nms_sort(dets, last.classes, cfg.nms); }   // main.c:856-858: at every nms
    else if (cfg.nms > 0.0f) total = y2h::nms_sort(dets, last.classes, cfg.nms);
    if ((int)names.size() < last.classes)
        std::fprintf(stderr, "Warning: names file provides %d labels, but network expects %d classes.\n", (int)names.size(), last.classes);

    int shown = 0;
    for (int i = 0; i < total; ++i) {
        for (int j = 0; j < last.classes; ++j) {
            if (dets[i].prob[j] <= cfg.thresh) continue;
            const y2h::Box &b = dets[i].bbox;
            const char *label = j < (int)names.size() ? names[j].c_str() : "?";
            std::printf("%s: %.0f%%  (x=%.4f y=%.4f w=%.4f h=%.4f)\n", label, dets[i].prob[j] * 100, b.x, b.y, b.w, b.h);
            if (cfg.json)
                std::printf("{\"label\":\"%s\",\"class\":%d,\"prob\":%.6f,\"x\":%.6f,\"y\":%.6f,\"w\":%.6f,\"h\":%.6f}\n", label, j, dets[i].prob[j], b.x, b.y, b.w, b.h);
            const int x1 = (int)((b.x - b.w / 2.) * im.w), x2 = (int)((b.x + b.w / 2.) * im.w);
            const int y1 = (int)((b.y - b.h / 2.) * im.h), y2 = (int)((b.y + b.h / 2.) * im.h);
            const float hue = (float)((j * 123457) % last.classes) / last.classes;
            y2h::draw_box(im, x1, y1, x2, y2, std::max(1, (int)(im.h * .006)), hue, 1.f - hue, 0.5f);
            ++shown;
        }
    }
    std::printf("%d detection(s) above %.2f\n", shown, cfg.thresh);
    if (!cfg.jsonl_path.empty()) {
        FILE *jf = std::fopen(cfg.jsonl_path.c_str(), "w");
        if (!jf) throw std::runtime_error("Failed to open JSON output " + cfg.jsonl_path);
        write_jsonl(jf, "image", cfg.input_path, 1, 1, im.w, im.h, best_class_dets(dets, total, last.classes, cfg.thresh), names);
        std::fclose(jf);
    }
    y2h::save_ppm(im, cfg.output_prefix + ".ppm");
    std::printf("Output written to %s.ppm\nYOLOv2 Object Detection - Complete\n", cfg.output_prefix.c_str());
}

}  // namespace

int main(int argc, char **argv)
{
    try {
        run_detector(parse_args(argc, argv));
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "Fatal error: %s\n", ex.what());  // yolov2_main.cpp:339-347
        return 1;
    }
    return 0;
}
