// y2_pix_cli.hpp -- what yolov2_detect and yolov2_calibrate need to know about a --video-pix-fmt, from the one format list
// (csrc/pix_formats.hpp).  Include after include/yolo2_hip.h (the list's rows are then checked against YOLO2_PIX_*) and y2_host.hpp.
#pragma once
#include <string>

#include "../csrc/pix_formats.hpp"
#include "y2_host.hpp"

namespace y2cli {

// a spelling or an alias -> the format (nullptr: not a video format); its YOLO2_PIX_* fourcc is ->pixfmt, its canonical spelling ->cli
inline const y2pix::Format *pix_by_spelling(const std::string &v)
{
    for (const y2pix::Format &f : y2pix::kFormats)
        if ((f.cli && v == f.cli) || (f.alias && v == f.alias)) return &f;
    return nullptr;
}
// by fourcc: one of the list's (a CLI only holds what pix_by_spelling gave it, or YOLO2_PIX_RGB24)
inline const y2pix::Format &pix(int pixfmt) { return *y2pix::by_fourcc(pixfmt); }
// "rgb24 | yuyv422 | ...": the canonical spellings, for the Unsupported message
inline std::string pix_spellings()
{
    std::string s;
    for (const y2pix::Format &f : y2pix::kFormats)
        if (f.cli) s += (s.empty() ? "" : " | ") + std::string(f.cli);
    return s;
}
// the parity rule of a frame size (the library's own check names the format's least size)
inline bool pix_parity_ok(const y2pix::Format &f, int w, int h) { return !(f.even_w && (w & 1)) && !(f.even_h && (h & 1)); }
// y2h::plain_box_frame's code for the format
inline int pix_host_frame(int pixfmt)
{
    switch (pixfmt) {
#define Y2_PIX_ROW(ID, FOURCC, KIND, CH, BITS, EVEN_W, EVEN_H, ALIGN, MIN_SIDE, CLI, ALIAS, FRAME, MSG) \
    case FOURCC: return FRAME;
        Y2_PIX_FORMATS(Y2_PIX_ROW)
#undef Y2_PIX_ROW
    }
    return -1;
}

}  // namespace y2cli
