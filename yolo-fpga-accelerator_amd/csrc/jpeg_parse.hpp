// jpeg_parse.hpp -- the host's side of the GPU JPEG decoder, plain C++ (no HIP): the probe (which streams the GPU decoder takes, with a
// reason for the others, and where a stream ends), the per-frame descriptor the kernels read (geometry, tables, segment table), and
// decode_ref: jpeg_scan.hpp's stages run one after the other on the host - the body of yolo2_hip_decode_jpeg_ref, which the CPU tests
// and tools/fuzz_jpegdec.cpp compare with host/y2_codec.cpp.  With a subsequence size it runs the entropy stage as option jpegdec_split
// does (split_plan, split_segment_host): the body of yolo2_hip_decode_jpeg_split_ref.
//
// The header checks restate Jpeg::segment / frame_header / scan_header of y2_codec.cpp and are never weaker: a stream that decoder
// throws on is refused here (kDamaged), and so is what it tolerates but this walk does not (bytes between segments, a header that runs
// past the end of the stream, DNL, segments between the scan and EOI): refused streams go through the host decoder.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

#include "jpeg_scan.hpp"

namespace y2jpg {

// yolo2_hip_jpeg_info_t::reason (include/yolo2_hip.h: YOLO2_JPEG_*)
enum Reason {
    kAccepted = 0,
    kDamaged = 1,        // no SOI, a bad segment, a header the host decoder throws on, no EOI behind the scan
    kProgressive = 2,    // SOF2
    kUnsupportedSof = 3, // arithmetic, lossless, hierarchical, 12-bit
    kComponents = 4,     // 4 components (CMYK / YCCK)
    kRgbColour = 5,      // component ids R,G,B, or Adobe transform 0 without JFIF
    kSampling = 6,       // chroma not 1x1, or luma H / V not 1 or 2
    kScans = 7,          // more than one scan, a scan that does not hold all components, anything but EOI behind the scan
    kMissingTable = 8,   // the scan names a Huffman table that is not defined
    kTooLarge = 9        // more than 16384 in a direction or 2^26 pixels
};

struct Info {
    int width = 0, height = 0, components = 0, hmax = 0, vmax = 0, restart_interval = 0;
    int gpu_decodable = 0, reason = kDamaged;
    size_t stream_bytes = 0;
};

// One accepted stream: descriptor (offsets relative to the frame; the caller places it), its table set, its segments (byte offsets
// relative to the stream), and the status the host already knows (kRestartOutOfStep where the RSTn count does not fit the geometry).
struct Parsed {
    Frame f;
    Tables t;
    std::vector<Segment> segs;
    int status = kOk;
};

namespace detail {

struct Rd {
    const uint8_t *d;
    size_t n, p = 0;
    bool over = false;
    int u8() { if (p < n) return d[p++]; over = true; return 0; }
    int u16() { const int a = u8(); return (a << 8) | u8(); }
    // the next marker: FF, any number of FF, the code; -1 where the next byte is not FF
    int marker()
    {
        int x = u8();
        if (x != 0xff) return -1;
        while (x == 0xff) x = u8();
        return over ? -1 : x;
    }
};

// from `p` inside entropy-coded data to the FF of the marker that ends the scan (FF followed by anything but 00, FF or D0..D7), or n
inline size_t scan_end(const uint8_t *d, size_t n, size_t p)
{
    while (p < n) {
        const uint8_t *q = (const uint8_t *)memchr(d + p, 0xff, n - p);
        if (!q) return n;
        const size_t at = (size_t)(q - d);
        size_t k = at + 1;
        while (k < n && d[k] == 0xff) ++k;
        if (k >= n) return n;
        if (d[k] != 0 && !(d[k] >= 0xd0 && d[k] <= 0xd7)) return at;
        p = k + 1;
    }
    return n;
}

// offset just past EOI, walking the segments by their lengths and the scans by scan_end; n where the walk fails
inline size_t stream_end(const uint8_t *d, size_t n)
{
    Rd r{d, n};
    if (r.marker() != 0xd8) return n;
    for (;;) {
        const int m = r.marker();
        if (m < 0) return n;
        if (m == 0xd9) return r.p;
        if (m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;
        const int L = r.u16();
        if (r.over || L < 2 || (size_t)(L - 2) > n - r.p) return n;
        r.p += (size_t)(L - 2);
        if (m == 0xda) r.p = scan_end(d, n, r.p);
    }
}

inline bool build_huff(Huff &h, const int counts[16], const uint8_t *symbols, int nsym)
{
    memset(&h, 0, sizeof(h));
    memcpy(h.vals, symbols, (size_t)nsym);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        h.valptr[len] = k;
        h.mincode[len] = code;
        for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code)
            if (len <= 9) {
                const int first = code << (9 - len), span = 1 << (9 - len);
                if (first + span > 512) return false;
                for (int j = 0; j < span; ++j) h.look[first + j] = (uint16_t)((len << 8) | symbols[k]);
            }
        if (code > (1 << len)) return false;
        h.maxcode[len] = counts[len - 1] ? code - 1 : -1;
        code <<= 1;
    }
    h.maxcode[0] = h.mincode[0] = -1;
    h.defined = 1;
    return true;
}

}  // namespace detail

// Classifies the stream and, when `out` is given and the stream is accepted, fills it.  Returns info.reason.
inline int parse(const uint8_t *d, size_t n, Info &info, Parsed *out)
{
    using namespace detail;
    info = Info();
    info.stream_bytes = stream_end(d, n);
    auto refuse = [&](int why) { info.gpu_decodable = 0; info.reason = why; return why; };
    Rd r{d, n};
    if (r.marker() != 0xd8) return refuse(kDamaged);
    // the tables live on the heap: Parsed is ~10 KB, the 8 candidate tables another 12
    struct Work {
        uint16_t dq[4][64];
        Huff hdc[4], hac[4];
    };
    std::vector<Work> work_store(1);
    Work &w = work_store[0];
    memset(&w, 0, sizeof(w));
    bool jfif = false;
    int adobe = -1, ri = 0;
    // ---- Jpeg::segment
    auto segment = [&](int m) -> bool {
        if (m == 0xdd) {
            if (r.u16() != 4) return false;
            ri = r.u16();
            return !r.over;
        }
        if (m == 0xdb) {
            int L = r.u16() - 2;
            while (L > 0 && !r.over) {
                const int q = r.u8(), wide = q >> 4, t = q & 15;
                if (wide > 1 || t > 3) return false;
                for (int i = 0; i < 64; ++i) w.dq[t][zigzag(i)] = (uint16_t)(wide ? r.u16() : r.u8());
                L -= wide ? 129 : 65;
            }
            return L == 0 && !r.over;
        }
        if (m == 0xc4) {
            int L = r.u16() - 2;
            while (L > 0 && !r.over) {
                const int q = r.u8(), tc = q >> 4, th = q & 15;
                if (tc > 1 || th > 3) return false;
                int counts[16], ns = 0;
                for (int &c : counts) { c = r.u8(); ns += c; }
                if (ns > 256) return false;
                uint8_t syms[256];
                for (int i = 0; i < ns; ++i) syms[i] = (uint8_t)r.u8();
                if (r.over || !build_huff((tc ? w.hac : w.hdc)[th], counts, syms, ns)) return false;
                L -= 17 + ns;
            }
            return L == 0 && !r.over;
        }
        if ((m >= 0xe0 && m <= 0xef) || m == 0xfe) {
            int L = r.u16();
            if (L < 2) return false;
            L -= 2;
            if ((size_t)L > n - r.p) return false;
            const uint8_t *b = d + r.p;
            if (m == 0xe0 && L >= 5 && memcmp(b, "JFIF\0", 5) == 0) jfif = true;
            if (m == 0xee && L >= 12 && memcmp(b, "Adobe\0", 6) == 0) adobe = b[11];
            r.p += (size_t)L;
            return true;
        }
        return false;
    };
    int m = r.marker();
    while (m != 0xc0 && m != 0xc1) {
        if (m == 0xc2) return refuse(kProgressive);
        if (m == 0xc3 || (m >= 0xc5 && m <= 0xcf && m != 0xcc)) return refuse(kUnsupportedSof);
        if (m < 0 || !segment(m)) return refuse(kDamaged);
        m = r.marker();
    }
    // ---- Jpeg::frame_header
    const int Lf = r.u16();
    if (Lf < 11) return refuse(kDamaged);
    const int prec = r.u8();
    const int height = r.u16(), width = r.u16(), ncomp = r.u8();
    if (r.over) return refuse(kDamaged);
    if (prec != 8) return refuse(kUnsupportedSof);
    if (!height || !width) return refuse(kDamaged);
    if (ncomp != 1 && ncomp != 3 && ncomp != 4) return refuse(kDamaged);
    if (Lf != 8 + 3 * ncomp) return refuse(kDamaged);
    info.width = width; info.height = height; info.components = ncomp;
    int id[4], ch[4], cv[4], tq[4], hmax = 1, vmax = 1, rgb_ids = 0;
    for (int i = 0; i < ncomp; ++i) {
        id[i] = r.u8();
        if (ncomp == 3 && id[i] == "RGB"[i]) ++rgb_ids;
        const int q = r.u8();
        ch[i] = q >> 4; cv[i] = q & 15;
        tq[i] = r.u8();
        if (r.over || !ch[i] || ch[i] > 4 || !cv[i] || cv[i] > 4 || tq[i] > 3) return refuse(kDamaged);
        hmax = ch[i] > hmax ? ch[i] : hmax;
        vmax = cv[i] > vmax ? cv[i] : vmax;
    }
    for (int i = 0; i < ncomp; ++i)
        if (hmax % ch[i] != 0 || vmax % cv[i] != 0) return refuse(kDamaged);
    if ((long long)width * height * ncomp > (1LL << 30)) return refuse(kDamaged);
    if (ncomp == 4) return refuse(kComponents);
    if (ncomp == 1) { ch[0] = cv[0] = hmax = vmax = 1; }      // one component: its own blocks in raster order whatever its factors say
    info.hmax = hmax; info.vmax = vmax;
    // ---- up to the scan
    m = r.marker();
    while (m != 0xda) {
        if (m < 0 || m == 0xd9 || m == 0xdc || !segment(m)) return refuse(kDamaged);
        m = r.marker();
    }
    info.restart_interval = ri;
    // ---- Jpeg::scan_header
    const int Ls = r.u16(), scan_n = r.u8();
    if (r.over || scan_n < 1 || scan_n > 4 || scan_n > ncomp || Ls != 6 + 2 * scan_n) return refuse(kDamaged);
    int order[3] = {0, 0, 0}, hd[3] = {0, 0, 0}, ha[3] = {0, 0, 0}, seen = 0;
    for (int i = 0; i < scan_n; ++i) {
        const int cid = r.u8(), q = r.u8();
        int which = 0;
        while (which < ncomp && id[which] != cid) ++which;
        if (r.over || which == ncomp || (q >> 4) > 3 || (q & 15) > 3) return refuse(kDamaged);
        hd[which] = q >> 4; ha[which] = q & 15;
        order[i] = which;
        seen |= 1 << which;
    }
    const int ss = r.u8();
    r.u8();
    const int a = r.u8();
    if (r.over || ss != 0 || a != 0) return refuse(kDamaged);
    // ---- what the host decoder takes but the GPU stages do not
    if (ncomp == 3 && (rgb_ids == 3 || (adobe == 0 && !jfif))) return refuse(kRgbColour);
    if (ncomp == 3 && (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || ch[0] > 2 || cv[0] > 2)) return refuse(kSampling);
    if (scan_n != ncomp || seen != (1 << ncomp) - 1) return refuse(kScans);
    for (int i = 0; i < ncomp; ++i)
        if (!w.hdc[hd[i]].defined || !w.hac[ha[i]].defined) return refuse(kMissingTable);
    if (width > 16384 || height > 16384 || (long long)width * height > (1LL << 26)) return refuse(kTooLarge);
    const size_t scan_at = r.p, scan_stop = scan_end(d, n, scan_at);
    {   // behind the scan: EOI, and nothing else
        Rd e{d, n, scan_stop};
        const int end_marker = e.marker();
        if (end_marker < 0) return refuse(kDamaged);
        if (end_marker != 0xd9) return refuse(kScans);
        info.stream_bytes = e.p;
    }
    info.gpu_decodable = 1;
    info.reason = kAccepted;
    if (!out) return kAccepted;

    Frame &f = out->f;
    memset(&f, 0, sizeof(f));
    f.width = width; f.height = height; f.ncomp = ncomp; f.hmax = hmax; f.vmax = vmax; f.restart_interval = ri;
    f.mcu_x = (width + hmax * 8 - 1) / (hmax * 8);
    f.mcu_y = (height + vmax * 8 - 1) / (vmax * 8);
    uint32_t off = 0;
    memset(&out->t, 0, sizeof(out->t));
    for (int i = 0; i < ncomp; ++i) {
        Comp &c = f.comp[i];
        c.h = ch[i]; c.v = cv[i];
        c.x = (width * c.h + hmax - 1) / hmax;
        c.y = (height * c.v + vmax - 1) / vmax;
        c.w2 = f.mcu_x * c.h * 8;
        c.h2 = f.mcu_y * c.v * 8;
        c.off = off;
        off += (uint32_t)c.w2 * (uint32_t)c.h2;
        f.order[i] = order[i];
        out->t.dc[i] = w.hdc[hd[i]];
        out->t.ac[i] = w.hac[ha[i]];
        memcpy(out->t.q[i], w.dq[tq[i]], sizeof(w.dq[0]));
    }
    f.samples = off;
    f.blocks = (int)(off / 64);
    // ---- the segment table: one entry per restart interval, cut at the RSTn markers a byte scan finds
    const int total = f.mcu_x * f.mcu_y, per = ri > 0 ? ri : total, want = (total + per - 1) / per;
    out->segs.clear();
    out->status = kOk;
    size_t begin = scan_at;
    for (size_t p = scan_at; p < scan_stop;) {
        const uint8_t *q = (const uint8_t *)memchr(d + p, 0xff, scan_stop - p);
        if (!q) break;
        size_t k = (size_t)(q - d) + 1;
        while (k < scan_stop && d[k] == 0xff) ++k;
        if (k >= scan_stop) break;
        if (d[k] >= 0xd0 && d[k] <= 0xd7) {
            Segment s = {(uint32_t)begin, (uint32_t)(k + 1), 0, 0, 0, 0};
            out->segs.push_back(s);
            begin = k + 1;
        }
        p = k + 1;
    }
    Segment tail = {(uint32_t)begin, (uint32_t)info.stream_bytes, 0, 0, 0, 1};
    out->segs.push_back(tail);
    if ((int)out->segs.size() != want) {
        // more or fewer markers than intervals: what the host decoder makes of that depends on state carried across intervals
        out->status = kRestartOutOfStep;
        out->segs.clear();
    }
    for (size_t i = 0; i < out->segs.size(); ++i) {
        out->segs[i].first_mcu = (int)i * per;
        out->segs[i].n_mcu = total - (int)i * per < per ? total - (int)i * per : per;
    }
    f.n_seg = (int)out->segs.size();
    return kAccepted;
}

// How option jpegdec_split = `split` bytes cuts one segment: data_end (the first FF of the marker that ends it), the subsequence in
// raw bytes (`split`, doubled until at most kSplitMaxSub of them cover the data) and their number.  n_sub < 2: the segment takes
// decode_segment's one lane (too short, or it does not end in a marker).
struct SplitPlan {
    uint32_t data_end;
    int sub, n_sub;
};
inline SplitPlan split_plan(const uint8_t *base, const Segment &s, int split)
{
    SplitPlan p = {s.begin, split, 0};
    if (split <= 0 || s.end < s.begin + 2 || base[s.end - 1] == 0 || base[s.end - 1] == 0xff || base[s.end - 2] != 0xff) return p;
    uint32_t e = s.end - 2;
    while (e > s.begin && base[e - 1] == 0xff) --e;
    p.data_end = e;
    const uint32_t len = e - s.begin;
    while (((uint64_t)len + (uint32_t)p.sub - 1) / (uint32_t)p.sub > (uint64_t)kSplitMaxSub) p.sub *= 2;
    p.n_sub = (int)((len + (uint32_t)p.sub - 1) / (uint32_t)p.sub);
    return p;
}

// One segment by many lanes, the lanes and rounds as loops (what k_jpegdec_split does with a workgroup): speculate, synchronise, scan,
// accept, write.  true: accepted, coefficients written (the segment's status is 0).  false: nothing written; decode_segment decides.
inline bool split_segment_host(const Frame &f, const Tables &t, const uint8_t *base, const Segment &s, const SplitPlan &sp, int16_t *coef, int *rounds)
{
    int bpm = 0;
    const uint32_t smap = split_slot_map(f, bpm), n_blocks = (uint32_t)s.n_mcu * (uint32_t)bpm;
    const int ns = sp.n_sub, turns = 8 * sp.sub + 16;
    auto sub_end = [&](int j) { const uint64_t e = (uint64_t)s.begin + (uint64_t)(j + 1) * (uint32_t)sp.sub; return e < sp.data_end ? (uint32_t)e : sp.data_end; };
    std::vector<SplitRec> rec((size_t)ns), cur((size_t)ns);
    std::vector<char> done((size_t)ns, 0);
    SplitWrite none = {};
    for (int i = 0; i < ns; ++i) {      // 1. speculate
        split_run<false>(f, t, base, sp.data_end, sub_end(i), smap, bpm, turns, s.begin + (uint32_t)i * (uint32_t)sp.sub, 0u, rec[(size_t)i], none);
        cur[(size_t)i] = rec[(size_t)i];
        done[(size_t)i] = (rec[(size_t)i].meta & kSplitStopped) != 0;
    }
    *rounds = 0;
    for (int r = 0; r < ns - 1; ++r) {  // 2. synchronise (lane i touches record i + r + 1 only: the order of the lanes does not matter)
        bool any = false;
        for (int i = 0; i + r + 1 < ns; ++i) {
            if (done[(size_t)i]) continue;
            const int j = i + r + 1;
            SplitRec out;
            split_run<false>(f, t, base, sp.data_end, sub_end(j), smap, bpm, turns, cur[(size_t)i].off, cur[(size_t)i].meta & kSplitStateMask, out, none);
            *rounds = r + 1;
            if (split_same(out, rec[(size_t)j])) { done[(size_t)i] = 1; continue; }
            rec[(size_t)j] = cur[(size_t)i] = out;
            if (out.meta & kSplitStopped) done[(size_t)i] = 1;
            else any = true;
        }
        if (!any) break;
    }
    // 3. scan, 4. accept
    std::vector<SplitRec> before((size_t)ns);
    SplitRec run = {};
    bool closes = false, overshoots = false;
    for (int i = 0; i < ns; ++i) {
        before[(size_t)i] = run;
        const bool stopped_before = (run.meta & kSplitStopped) != 0;
        closes |= split_closes(run.nblk, stopped_before, rec[(size_t)i], n_blocks);
        overshoots |= split_overshoots(run.nblk, stopped_before, rec[(size_t)i], n_blocks);
        run.nblk += rec[(size_t)i].nblk;
        for (int k = 0; k < 3; ++k) run.dc[k] = (int32_t)((uint32_t)run.dc[k] + (uint32_t)rec[(size_t)i].dc[k]);
        run.meta |= rec[(size_t)i].meta & kSplitStopped;
    }
    if (!closes || overshoots) return false;
    for (int i = 0; i < ns; ++i) {      // 5. write
        const SplitRec &b = before[(size_t)i];
        if ((b.meta & kSplitStopped) || b.nblk >= n_blocks) break;
        SplitWrite w = {(int)b.nblk, (int)n_blocks, s.first_mcu, {b.dc[0], b.dc[1], b.dc[2]}, coef};
        SplitRec out;
        split_run<true>(f, t, base, sp.data_end, sub_end(i), smap, bpm, turns, i ? rec[(size_t)i - 1].off : s.begin,
                        i ? rec[(size_t)i - 1].meta & kSplitStateMask : 0u, out, w);
    }
    return true;
}

// The stages one after the other on the host, one frame: status as the kernels would leave it, RGB24 where it is 0.
// Returns the probe's reason (0: accepted, rgb / status filled; the picture is w * h * 3 bytes, cap must hold it: -1 otherwise).
// split > 0: the entropy stage as option jpegdec_split runs it (yolo2_hip_decode_jpeg_split_ref); info8 = subsequences, segments
// split-decoded, fallen back, too short, most rounds of a segment, split, 0, 0.
inline int decode_ref(const uint8_t *d, size_t n, uint8_t *rgb, size_t cap, int *width, int *height, int *status, int split = 0, double *info8 = nullptr)
{
    if (info8) {
        for (int i = 0; i < 8; ++i) info8[i] = 0;
        info8[5] = split;
    }
    Info info;
    std::vector<Parsed> ps(1);
    Parsed &P = ps[0];
    const int why = parse(d, n, info, &P);
    if (width) *width = info.width;
    if (height) *height = info.height;
    if (why) return why;
    if (cap < (size_t)info.width * info.height * 3) return -1;
    int st = P.status;
    std::vector<int16_t> coef(P.f.samples, 0);
    std::vector<uint8_t> planes(P.f.samples, 0);
    for (size_t i = 0; i < P.segs.size() && st == kOk; ++i) {
        if (split > 0) {
            const SplitPlan sp = split_plan(d, P.segs[i], split);
            int rounds = 0;
            const bool took = sp.n_sub >= 2 && split_segment_host(P.f, P.t, d, P.segs[i], sp, coef.data(), &rounds);
            if (info8) {
                if (sp.n_sub >= 2) info8[0] += sp.n_sub;
                info8[sp.n_sub < 2 ? 3 : (took ? 1 : 2)] += 1;
                if (rounds > info8[4]) info8[4] = rounds;
            }
            if (took) continue;
        }
        st = decode_segment(P.f, P.t, d, P.segs[i], coef.data());
    }
    if (status) *status = st;
    if (st) return kAccepted;
    for (int k = 0; k < P.f.ncomp; ++k) {
        const Comp &c = P.f.comp[k];
        const int bw = c.w2 / 8, bh = c.h2 / 8;
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx)
                idct_block(planes.data() + c.off + (size_t)by * 8 * c.w2 + (size_t)bx * 8, c.w2, coef.data() + c.off + ((size_t)by * bw + bx) * 64);
    }
    for (int y = 0; y < P.f.height; ++y)
        for (int x = 0; x < P.f.width; ++x) rgb_pixel(P.f, planes.data(), x, y, rgb + ((size_t)y * P.f.width + x) * 3);
    return kAccepted;
}

}  // namespace y2jpg
