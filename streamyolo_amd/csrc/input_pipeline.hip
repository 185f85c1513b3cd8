// input_pipeline.hip — the frame-pair input pipeline on the device.
//
// The reference prepares every sample on CPU workers — `_mirror` + `preproc` (letterbox on a 114 canvas,
// HWC uint8 -> CHW float32; exps/data/data_augment_flip.py:140-167), `np.concatenate((img, support_img))`
// (exps/data/tal_flip_mosaicdetection.py:257) — ships fp32 [B,6,H,W] over PCIe (13.8 MB per 600x960 pair,
// exps/train_utils/double_data_prefetcher.py:50-51) and, for multi-scale training, resizes the batch with
// `F.interpolate(mode="bilinear", align_corners=False)` (Exp.preprocess, cfgs/l_s50_onex_dfp_tal_filp.py:161-172).
// The streaming loop does the same per camera frame inside its timed region (sAP/streamyolo/streamyolo_det.py:176-179).
//
// Here the uint8 HWC frames go to the device as they are (1/4 of the bytes) and ONE kernel does mirror, letterbox,
// the optional exact 2x decimation, the optional bilinear resize to the training size and the layout change —
// either to the reference's fp32 NCHW tensor (drop-in) or straight to the Focus-packed NHWC16 operand of the stem
// convolution (space-to-depth order TL, BL, TR, BR — trap T4).  HBM-bound: 3 B read, <= 4 B written per pixel/channel.
//
// cv2.resize parity (OpenCV is not available where this was built: all three cases are restated from OpenCV's published
// resize.cpp, PARITY UNPINNED against a cv2 binary — oracle/input_oracle.py states the same arithmetic in numpy):
//   decimate 1   same size: copy;
//   decimate 2   exact 2x: cv::resize turns INTER_LINEAR into the INTER_AREA fast path when both scale factors are exactly
//                2, (a + b + c + d + 2) >> 2 — Argoverse's 1200x1920 -> 600x960;
//   decimate 0   any other camera size: `preproc`'s r = min(H / h, W / w), cv2.resize(img, (int(w r), int(h r)),
//                INTER_LINEAR) (data_augment_flip.py:151-167) = OpenCV's fixed-point bilinear for 8-bit images: source
//                coordinate fx = (float)((dx + 0.5) * scale - 0.5), taps sx = floor(fx), sx + 1 (horizontally: clamped at the
//                borders with the fraction zeroed; vertically: row indices clamped, fraction kept), coefficients saturate_cast<short>(frac * 2048) (round half to even), horizontal pass
//                in int32, vertical pass ((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.
//
// Pixel formats (sy_frames_u8_pack_fmt, sy_frame_src.format).  Frames are BGR as cv2.imread delivers them; a deployment gets RGB
// (PIL, torchvision, GStreamer) or NV12 (hardware video decoders) and would convert on the CPU first.  Here the conversion is part
// of the same launch, per SOURCE pixel and before any decimation or bilinear tap: for every format the output is bit for bit what
// the BGR path writes for the converted uint8 [Hs, Ws, 3] frame.  The BGR kernels are the ones they were (frame_at, sample and
// focus_pixel keep their expressions); RGB reads byte 2 - c; NV12 has kernels of its own that form the (B, G, R) triple of a source
// pixel ONCE (the other paths call sample() once per channel).
//   NV12 layout  ONE pitch for both planes: Hs rows of luma, then — starting at row Hs — Hs / 2 rows of interleaved chroma (U, V):
//                the [Hs * 3 / 2, Ws] array cv2.cvtColor takes, with an optional pitch; Hs, Ws even.  Chroma of pixel (y, x) = the
//                pair at chroma row y >> 1, byte 2 * (x >> 1) (nearest).  That is sy_frames_u8_pack_fmt's and sy_frame_src's layout;
//                a surface whose chroma plane starts elsewhere (a padded luma height, a detached plane, a pitch of its own) is
//                described by sy_frame_surf (below).
//   arithmetic   BT.601 limited range in the int32 fixed point OpenCV publishes for COLOR_YUV2BGR_NV12 (nv12_bgr below) — like the
//                resize arithmetic restated from published source, PARITY UNPINNED against a cv2 binary.
//   fast path    NV12 -> Focus layout without the canvas resize, decimate 1 | 2 (1200x1920 -> 600x960 is this case): one thread
//                owns one Focus pixel = 2x2 output pixels; decimate 2: a 4x4 luma block and 2x2 chroma pairs in six 32-bit loads
//                (decimate 1: 2x2 luma, one pair, three 16-bit loads) instead of 24 single-byte loads.  Taken — per launch, per
//                row in the rows kernel — only when base pointers, pitch and image stride are multiples of the load width and ws is
//                even; a Focus pixel not wholly inside the image takes the generic path.  Bit-identical with the generic path.
//
// Decoder surfaces (sy_frames_u8_pack_surfaces, sy_frame_surf).  A hardware decoder's surface is read where it lies: the row's
// descriptor names both planes (plane1 = the chroma plane at any address, with its own pitch), so a padded luma height (1080 ->
// 1088 rows) or a detached chroma allocation needs no repacking and no staging copy.  The NV12 sample fetch takes the chroma base,
// the chroma pitch and a sample step (ChromaAt); the single-allocation sources fill them with cur + row_stride * Hs, row_stride
// and step 1: ONE code path, whose bits the NV12 tests pin.  P010 (10-bit decoders: two planes of little-endian 16-bit words, the
// significant bits on top) is the same path with a step of 2 bytes and an offset of 1: the 8-bit sample is the word's HIGH byte
// (word >> 8: truncation, no rounding, no dithering) — the project's definition, no OpenCV conversion exists to pin it against.
// The wide-load fast path is decided per row from BOTH planes' addresses and pitches; P010 takes the generic path only.
#include "sy_pointwise.h"
#include "sy_nv12.h"

namespace {

using namespace sy_nv12;                                         // Chroma, nv12_chroma, nv12_bgr, sat8

// One frame after the load-time resize: what the per-pixel sampling needs besides the pixels.  Resolved from the camera size, the
// decimate mode and the canvas by frame_geom() — on the host for sy_frames_u8_pack (one geometry per batch), on the device for
// sy_frames_u8_pack_rows (one per batch row, from its descriptor): the same function, the same double arithmetic.
struct FrameGeom {
    int row_stride;             // bytes between rows
    int hs, ws;                 // size AFTER the load-time resize (decimation or general ratio)
    int dec;                    // 1 or 2; 0 = general-ratio fixed-point bilinear from a src_h x src_w frame
    int src_h, src_w;
    double scale_y, scale_x;    // dec == 0: source / destination size ratios (OpenCV: 1. / ((double)dst / src))
};

// decimate (1 | 2 | 0 | -1, range and evenness already checked) of an Hs x Ws frame on an H x W canvas -> hs, ws, dec, scales
__host__ __device__ inline int frame_geom(int Hs, int Ws, int decimate, int H, int W, FrameGeom& g) {
    int hs, ws;
    g.src_h = Hs; g.src_w = Ws; g.scale_y = 1.0; g.scale_x = 1.0;
    if (decimate == 0 || decimate == -1) {
        if (decimate == 0) {
            // preproc: r = min(H / h, W / w); resized to (int(w * r), int(h * r)) — the same double arithmetic as the Python code
            const double r = ((double)H / Hs < (double)W / Ws) ? (double)H / Hs : (double)W / Ws;
            hs = (int)(Hs * r); ws = (int)(Ws * r);
        } else {
            // streaming: cv2.resize(img, (w_img, h_img)) with the canvas = (int(h * in_scale), int(w * in_scale)) — each axis
            // stretched on its own, no letterbox (sAP/streamyolo/streamyolo_det.py:176-178)
            hs = H; ws = W;
            decimate = 0;
        }
        if (hs < 1 || ws < 1 || hs > H || ws > W) return SY_ERR_UNSUPPORTED;
        g.scale_y = 1.0 / ((double)hs / Hs); g.scale_x = 1.0 / ((double)ws / Ws);
        if (hs == Hs && ws == Ws) decimate = 1;                          // r == 1: cv::resize copies
        else if (2 * hs == Hs && 2 * ws == Ws) decimate = 2;             // both factors exactly 2: OpenCV's INTER_AREA fast path
    } else {
        hs = Hs / decimate; ws = Ws / decimate;
        // preproc's ratio r = min(H / h, W / w) must be exactly 1 after the decimation (see the header)
        if (hs > H || ws > W || (hs != H && ws != W)) return SY_ERR_UNSUPPORTED;
    }
    g.hs = hs; g.ws = ws; g.dec = decimate;
    return SY_OK;
}

// OpenCV's INTER_LINEAR tap set of one destination coordinate (resize.cpp, 8-bit fixed-point path)
struct Tap { int s0, s1; int a0, a1; };
// HORIZ: OpenCV zeroes the fraction at the left / right border (xofs / alpha tables); the vertical pass keeps the fraction
// and only clamps the two row indices (srows[k] = clip(sy + k)) — both taps then read the same row with b0 + b1 = 2048
template <bool HORIZ> __device__ __forceinline__ Tap frame_tap(int d, double scale, int ssize) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (HORIZ) {
        if (s < 0) { f = 0.0f; s = 0; }
        if (s >= ssize - 1) { f = 0.0f; s = ssize - 1; }
    }
    Tap t;
    t.s0 = s < 0 ? 0 : (s > ssize - 1 ? ssize - 1 : s);
    t.s1 = s + 1 < 0 ? 0 : (s + 1 > ssize - 1 ? ssize - 1 : s + 1);
    t.a0 = (int)rintf((1.0f - f) * 2048.0f);            // saturate_cast<short>(float) = cvRound (round half to even)
    t.a1 = (int)rintf(f * 2048.0f);
    return t;
}

// value of channel c at (y, x) of the letterboxed canvas of the frame at p — the per-pixel arithmetic of BOTH pack kernels.
// Reads stay inside src_h x src_w: dec 1 / 2 address rows < dec * hs <= src_h and bytes < dec * ws * 3 <= row_stride, the
// bilinear taps are clamped to [0, src - 1].
__device__ __forceinline__ float frame_at(const unsigned char* p, const FrameGeom& g, bool mirror, int c, int y, int x) {
    if (y >= g.hs || x >= g.ws) return 114.0f;
    if (mirror) x = g.ws - 1 - x;
    if (g.dec == 1) return (float)p[(long long)y * g.row_stride + x * 3 + c];
    if (g.dec == 0) {
        const Tap ty = frame_tap<false>(y, g.scale_y, g.src_h), tx = frame_tap<true>(x, g.scale_x, g.src_w);
        const unsigned char* r0 = p + (long long)ty.s0 * g.row_stride + c;
        const unsigned char* r1 = p + (long long)ty.s1 * g.row_stride + c;
        const int S0 = (int)r0[tx.s0 * 3] * tx.a0 + (int)r0[tx.s1 * 3] * tx.a1;      // horizontal pass, scaled by 2^11
        const int S1 = (int)r1[tx.s0 * 3] * tx.a0 + (int)r1[tx.s1 * 3] * tx.a1;
        const int v = (((ty.a0 * (S0 >> 4)) >> 16) + ((ty.a1 * (S1 >> 4)) >> 16) + 2) >> 2;
        return (float)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
    const unsigned char* r0 = p + (long long)(2 * y) * g.row_stride + (2 * x) * 3 + c;
    const unsigned char* r1 = r0 + g.row_stride;
    return (float)(((int)r0[0] + (int)r0[3] + (int)r1[0] + (int)r1[3] + 2) >> 2);
}

// ---- NV12: Chroma, nv12_chroma, sat8 and nv12_bgr (the per-pixel conversion) live in sy_nv12.h, shared with crop.hip
// Where the chroma plane of an NV12 image lies and how its samples are stored: the interleaved (U, V) plane at `uv` with `pitch`
// bytes between rows; sample k of a row (either plane) is the byte at (k << sh) + sh.  sh = 0: NV12 proper.  sh = 1: P010 — 16-bit
// little-endian words whose HIGH byte is the 8-bit sample (a step of 2 bytes and an offset of 1: the same arithmetic on other
// bytes, not a second conversion).  The single-allocation sources fill it with p + row_stride * src_h, row_stride and the
// literal 0, which the compiler folds: their address arithmetic is what it was.
struct ChromaAt {
    const unsigned char* uv;
    int pitch;
    int sh;
};
// (B, G, R) of source pixel (sy, sx) of the NV12 image whose luma plane is at p: luma row sy, chroma row sy >> 1, pair 2 * (sx >> 1)
__device__ __forceinline__ void nv12_px(const unsigned char* p, const ChromaAt& ch, const FrameGeom& g, int sy, int sx, int o[3]) {
    const unsigned char* uv = ch.uv + (long long)(sy >> 1) * ch.pitch + ((2 * (sx >> 1)) << ch.sh) + ch.sh;
    nv12_bgr((int)p[(long long)sy * g.row_stride + (sx << ch.sh) + ch.sh], nv12_chroma((int)uv[0], (int)uv[1 << ch.sh]), o);
}

// frame_at for an NV12 image, all three channels of canvas pixel (y, x) at once: every source pixel is converted once and the
// integer arithmetic of frame_at runs on the triples.  Reads stay inside src_h luma rows and src_h / 2 chroma rows of
// src_w << sh bytes each (<= the plane's pitch): nothing between src_w and a pitch, nothing between the planes.
__device__ __forceinline__ void frame_at3_nv12(const unsigned char* p, const ChromaAt& ch, const FrameGeom& g, bool mirror, int y,
                                               int x, float o[3]) {
    if (y >= g.hs || x >= g.ws) { o[0] = 114.0f; o[1] = 114.0f; o[2] = 114.0f; return; }
    if (mirror) x = g.ws - 1 - x;
    if (g.dec == 1) {
        int a[3];
        nv12_px(p, ch, g, y, x, a);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (float)a[c];
        return;
    }
    if (g.dec == 0) {
        const Tap ty = frame_tap<false>(y, g.scale_y, g.src_h), tx = frame_tap<true>(x, g.scale_x, g.src_w);
        int p00[3], p01[3], p10[3], p11[3];
        nv12_px(p, ch, g, ty.s0, tx.s0, p00); nv12_px(p, ch, g, ty.s0, tx.s1, p01);
        nv12_px(p, ch, g, ty.s1, tx.s0, p10); nv12_px(p, ch, g, ty.s1, tx.s1, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int S0 = p00[c] * tx.a0 + p01[c] * tx.a1;                              // horizontal pass, scaled by 2^11
            const int S1 = p10[c] * tx.a0 + p11[c] * tx.a1;
            const int v = (((ty.a0 * (S0 >> 4)) >> 16) + ((ty.a1 * (S1 >> 4)) >> 16) + 2) >> 2;
            o[c] = (float)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
        return;
    }
    // the 2x2 source block of an exact 2x decimation shares one chroma pair: chroma row y, pair 2 x
    const int at = ((2 * x) << ch.sh) + ch.sh, next = 1 << ch.sh;
    const unsigned char* r0 = p + (long long)(2 * y) * g.row_stride + at;
    const unsigned char* r1 = r0 + g.row_stride;
    const unsigned char* uv = ch.uv + (long long)y * ch.pitch + at;
    const Chroma k = nv12_chroma((int)uv[0], (int)uv[next]);
    int a[3], b[3], c_[3], d[3];
    nv12_bgr((int)r0[0], k, a); nv12_bgr((int)r0[next], k, b); nv12_bgr((int)r1[0], k, c_); nv12_bgr((int)r1[next], k, d);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (float)((a[c] + b[c] + c_[c] + d[c] + 2) >> 2);
}

// 16 / 32 bits at an address that is a multiple of the width (the fast path's precondition)
__device__ __forceinline__ unsigned load_u16(const unsigned char* p) { return *reinterpret_cast<const unsigned short*>(p); }
__device__ __forceinline__ unsigned load_u32(const unsigned char* p) { return *reinterpret_cast<const unsigned int*>(p); }

// The NV12 fast path: the Focus pixel (h2, w2) = output pixels (2 h2 + i, 2 w2 + j) of an image it lies wholly inside (2 h2 + 1
// < hs, 2 w2 + 1 < ws), dec 1 | 2, ws even, sh = 0, p, row_stride, ch.uv and ch.pitch multiples of 2 (dec 1) / 4 (dec 2) ->
// px[i][j][c], j counted in
// IMAGE order (mirrored: output column 2 w2 + j is px[.][1 - j] — the caller selects, so that every index here is a constant
// and the block stays in registers).  The same integers as frame_at3_nv12 from wide loads.
__device__ __forceinline__ void nv12_focus_block(const unsigned char* p, const ChromaAt& ch, const FrameGeom& g, bool mirror, int h2,
                                                 int w2, int px[2][2][3]) {
    const int xs = mirror ? g.ws - 2 - 2 * w2 : 2 * w2;             // the pair's left column in the (unmirrored) image: even
    if (g.dec == 1) {
        const unsigned uv = load_u16(ch.uv + (long long)h2 * ch.pitch + xs);
        const Chroma k = nv12_chroma((int)(uv & 255u), (int)(uv >> 8));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned l = load_u16(p + (long long)(2 * h2 + i) * g.row_stride + xs);
            nv12_bgr((int)(l & 255u), k, px[i][0]);
            nv12_bgr((int)(l >> 8), k, px[i][1]);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        // output row 2 h2 + i: luma rows 4 h2 + 2 i and the next, chroma row 2 h2 + i; bytes 2 xs .. 2 xs + 3 of each
        const unsigned char* r0 = p + (long long)(4 * h2 + 2 * i) * g.row_stride + 2 * xs;
        const unsigned l0 = load_u32(r0), l1 = load_u32(r0 + g.row_stride);
        const unsigned uv = load_u32(ch.uv + (long long)(2 * h2 + i) * ch.pitch + 2 * xs);
#pragma unroll
        for (int j = 0; j < 2; ++j) {                               // image column xs + j
            const Chroma k = nv12_chroma((int)((uv >> (16 * j)) & 255u), (int)((uv >> (16 * j + 8)) & 255u));
            int a[3], b[3], c_[3], d[3];
            nv12_bgr((int)((l0 >> (16 * j)) & 255u), k, a); nv12_bgr((int)((l0 >> (16 * j + 8)) & 255u), k, b);
            nv12_bgr((int)((l1 >> (16 * j)) & 255u), k, c_); nv12_bgr((int)((l1 >> (16 * j + 8)) & 255u), k, d);
#pragma unroll
            for (int c = 0; c < 3; ++c) px[i][j][c] = (a[c] + b[c] + c_[c] + d[c] + 2) >> 2;
        }
    }
}
// what the fast path needs of an image besides dec 1 | 2: even ws and every row start — of BOTH planes — a multiple of the load
// width.  addr_bits: every base address and every pitch besides g.row_stride, OR-ed (a chroma plane of its own: its address and
// its pitch; the single-allocation layout's chroma rows start at multiples of row_stride from the base)
__host__ __device__ inline bool nv12_fast_ok(const FrameGeom& g, unsigned long long addr_bits) {
    if ((g.dec != 1 && g.dec != 2) || (g.ws & 1)) return false;
    return ((addr_bits | (unsigned long long)g.row_stride) & (g.dec == 2 ? 3ull : 1ull)) == 0;
}

struct FrameSrc {               // uint8 HWC frames of one batch, one geometry: current and (optional) support
    const unsigned char* img[2];
    long long image_stride;     // bytes between images
    FrameGeom g;
    const unsigned char* mirror;    // [B] flags or nullptr
    // value of channel c at (y, x) of the letterboxed H x W canvas of image n, frame f
    __device__ __forceinline__ float at(int n, int f, int c, int y, int x) const {
        if (y >= g.hs || x >= g.ws) return 114.0f;
        return frame_at(img[f] + n * image_stride, g, mirror != nullptr && mirror[n], c, y, x);
    }
};

struct FrameSrcRGB : FrameSrc {  // the same frames in RGB order
    __device__ __forceinline__ float at(int n, int f, int c, int y, int x) const { return FrameSrc::at(n, f, 2 - c, y, x); }
};
struct FrameSrcNV12 : FrameSrc { // [B] NV12 images of src_h * 3 / 2 rows
    __device__ __forceinline__ const unsigned char* image(int n, int f) const { return img[f] + n * image_stride; }
    __device__ __forceinline__ ChromaAt chroma(int n, int f) const {         // one pitch, chroma at row src_h
        ChromaAt ch;
        ch.uv = image(n, f) + (long long)g.src_h * g.row_stride; ch.pitch = g.row_stride; ch.sh = 0;
        return ch;
    }
    __device__ __forceinline__ bool mirrored(int n) const { return mirror != nullptr && mirror[n]; }
    __device__ __forceinline__ void at3(int n, int f, int y, int x, float o[3]) const {
        if (y >= g.hs || x >= g.ws) { o[0] = 114.0f; o[1] = 114.0f; o[2] = 114.0f; return; }
        frame_at3_nv12(image(n, f), chroma(n, f), g, mirrored(n), y, x, o);
    }
};

// One batch row of sy_frames_u8_pack_rows / sy_frames_u8_pack_surfaces: its descriptor, resolved.  A row without a frame — or with
// a descriptor no frame can have (the host cannot see the table: the caller validates it) — has hs = ws = 0: the plain 114
// canvas, nothing is read.  fmt is SY_PIX_BGR | RGB | NV12 for the sampling: a P010 surface is NV12 with ch.sh = 1.
struct RowSrc {
    const unsigned char* p;
    FrameGeom g;
    bool mirror;
    int fmt;                    // SY_PIX_*: scalar, like g.dec
    bool fast;                  // NV12: the image qualifies for the fast path (nv12_fast_ok)
    ChromaAt ch;                // NV12: the chroma plane
    __device__ __forceinline__ void clear() {
        p = nullptr; mirror = false; fmt = SY_PIX_BGR; fast = false;
        ch.uv = nullptr; ch.pitch = 0; ch.sh = 0;
        g.row_stride = 0; g.hs = 0; g.ws = 0; g.dec = 1; g.src_h = 0; g.src_w = 0; g.scale_y = 1.0; g.scale_x = 1.0;
    }
    // a surface: the planes where they lie, each with its own pitch
    __device__ __forceinline__ RowSrc(const sy_frame_surf* rows, int b, int H, int W) {
        const sy_frame_surf d = rows[b];                        // one 48-byte load per workgroup (b = blockIdx.y: uniform)
        clear();
        if (d.plane0 == nullptr || d.Hs <= 0 || d.Ws <= 0 || d.decimate < -1 || d.decimate > 2) return;
        if (d.format != SY_PIX_BGR && d.format != SY_PIX_RGB && d.format != SY_PIX_NV12 && d.format != SY_PIX_P010) return;
        const bool yuv = d.format == SY_PIX_NV12 || d.format == SY_PIX_P010;
        const int sh = d.format == SY_PIX_P010 ? 1 : 0;
        if ((d.decimate == 2 || yuv) && ((d.Hs & 1) || (d.Ws & 1))) return;
        const long long row_bytes = yuv ? ((long long)d.Ws << sh) : (long long)d.Ws * 3;
        if ((long long)d.row_stride < row_bytes) return;
        const int cpitch = d.chroma_stride != 0 ? d.chroma_stride : d.row_stride;
        if (yuv && (d.chroma_stride < 0 || (long long)cpitch < row_bytes)) return;
        FrameGeom r;
        if (frame_geom(d.Hs, d.Ws, d.decimate, H, W, r) != SY_OK) return;
        r.row_stride = d.row_stride;
        r.dec = sy_uniform(r.dec);
        g = r; p = d.plane0; mirror = d.mirror != 0;
        fmt = sy_uniform(yuv ? (int)SY_PIX_NV12 : d.format);
        if (yuv) {
            ch.uv = d.plane1 != nullptr ? d.plane1 : d.plane0 + (long long)d.row_stride * d.Hs;
            ch.pitch = cpitch;
            ch.sh = sy_uniform(sh);
            // the wide loads need BOTH planes aligned: the chroma plane's own address and pitch, not the luma's
            const unsigned long long bits = (unsigned long long)(uintptr_t)p | (unsigned long long)(uintptr_t)ch.uv |
                                            (unsigned long long)cpitch;
            fast = sy_uniform(sh == 0 && nv12_fast_ok(r, bits) ? 1 : 0) != 0;
        }
    }
    // sy_frame_src: one allocation, one pitch, chroma at row Hs
    __device__ __forceinline__ RowSrc(const sy_frame_src* rows, int b, int H, int W) {
        const sy_frame_src d = rows[b];                         // one 32-byte load per workgroup (b = blockIdx.y: uniform)
        clear();
        if (d.cur == nullptr || d.Hs <= 0 || d.Ws <= 0 || d.decimate < -1 || d.decimate > 2) return;
        if (d.format != SY_PIX_BGR && d.format != SY_PIX_RGB && d.format != SY_PIX_NV12) return;
        const bool nv12 = d.format == SY_PIX_NV12;
        if ((d.decimate == 2 || nv12) && ((d.Hs & 1) || (d.Ws & 1))) return;
        if ((long long)d.row_stride < (long long)d.Ws * (nv12 ? 1 : 3)) return;
        FrameGeom r;
        if (frame_geom(d.Hs, d.Ws, d.decimate, H, W, r) != SY_OK) return;
        r.row_stride = d.row_stride;
        r.dec = sy_uniform(r.dec);                              // the sampling branches on it: scalar, the whole workgroup one way
        g = r; p = d.cur; mirror = d.mirror != 0;
        fmt = sy_uniform(d.format);
        fast = sy_uniform(nv12 && nv12_fast_ok(r, (unsigned long long)(uintptr_t)d.cur) ? 1 : 0) != 0;
        ch.uv = d.cur + (long long)d.row_stride * d.Hs; ch.pitch = d.row_stride;
    }
    __device__ __forceinline__ float at(int, int, int c, int y, int x) const {
        return frame_at(p, g, mirror, fmt == SY_PIX_RGB ? 2 - c : c, y, x);
    }
    __device__ __forceinline__ const unsigned char* image(int, int) const { return p; }
    __device__ __forceinline__ bool mirrored(int) const { return mirror; }
    __device__ __forceinline__ ChromaAt chroma(int, int) const { return ch; }
    __device__ __forceinline__ void at3(int, int, int y, int x, float o[3]) const { frame_at3_nv12(p, ch, g, mirror, y, x, o); }
};

struct PlaneSrc {               // fp32 NCHW tensor (Exp.preprocess's input)
    const float* in;
    int C, H, W;
    __device__ __forceinline__ float at(int n, int f, int c, int y, int x) const {
        return in[(((long long)n * C + f * 3 + c) * H + y) * W + x];
    }
};

// torch's upsample_bilinear2d, align_corners=False: scale = in / out (float), src = max(0, scale * (dst + 0.5) - 0.5),
// i0 = (int)src, i1 = i0 + (i0 < in - 1), lambda1 = src - i0 (aten/src/ATen/native/UpSample.h area_pixel_compute_*)
struct Lerp {
    int i0, i1;
    float l0, l1;
    __device__ __forceinline__ Lerp(int dst, float scale, int in_size) {
        float s = scale * ((float)dst + 0.5f) - 0.5f;
        if (s < 0.0f) s = 0.0f;
        i0 = (int)s;
        if (i0 > in_size - 1) i0 = in_size - 1;
        i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
        l1 = s - (float)i0;
        l0 = 1.0f - l1;
    }
};

template <typename S>
__device__ __forceinline__ float sample(const S& src, int n, int f, int c, int y, int x, bool resize, float sy, float sx,
                                        int H, int W) {
    if (!resize) return src.at(n, f, c, y, x);
    const Lerp ly(y, sy, H), lx(x, sx, W);
    return ly.l0 * (lx.l0 * src.at(n, f, c, ly.i0, lx.i0) + lx.l1 * src.at(n, f, c, ly.i0, lx.i1)) +
           ly.l1 * (lx.l0 * src.at(n, f, c, ly.i1, lx.i0) + lx.l1 * src.at(n, f, c, ly.i1, lx.i1));
}

// sample() for a source that delivers whole pixels (NV12): the same expressions per channel, every tap converted once
template <typename S>
__device__ __forceinline__ void sample3(const S& src, int n, int f, int y, int x, bool resize, float sy, float sx, int H, int W,
                                        float o[3]) {
    if (!resize) { src.at3(n, f, y, x, o); return; }
    const Lerp ly(y, sy, H), lx(x, sx, W);
    float a[3], b[3], c_[3], d[3];
    src.at3(n, f, ly.i0, lx.i0, a); src.at3(n, f, ly.i0, lx.i1, b);
    src.at3(n, f, ly.i1, lx.i0, c_); src.at3(n, f, ly.i1, lx.i1, d);
#pragma unroll
    for (int c = 0; c < 3; ++c)
        o[c] = ly.l0 * (lx.l0 * a[c] + lx.l1 * b[c]) +
               ly.l1 * (lx.l0 * c_[c] + lx.l1 * d[c]);
}

// -> fp32 NCHW [B, 3*F, Ho, Wo]; one thread per output element, x fastest (coalesced stores)
template <typename S>
__global__ __launch_bounds__(kBlock) void frames_to_nchw_kernel(S src, int B, int F, int H, int W, int Ho, int Wo,
                                                                float* out) {
    const bool resize = Ho != H || Wo != W;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const long long total = (long long)B * F * 3 * Ho * Wo;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int x = (int)(i % Wo);
        const int y = (int)((i / Wo) % Ho);
        const int ch = (int)((i / ((long long)Wo * Ho)) % (3 * F));
        const int n = (int)(i / ((long long)Wo * Ho * 3 * F));
        out[i] = sample(src, n, ch / 3, ch % 3, y, x, resize, sy, sx, H, W);
    }
}

// NV12 -> fp32 NCHW: one thread per output PIXEL, its three channel planes written from one conversion
__global__ __launch_bounds__(kBlock) void frames_nv12_to_nchw_kernel(FrameSrcNV12 src, int B, int F, int H, int W, int Ho, int Wo,
                                                                     float* out) {
    const bool resize = Ho != H || Wo != W;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const long long plane = (long long)Ho * Wo, total = (long long)B * F * plane;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < total; i += (long long)gridDim.x * kBlock) {
        const int x = (int)(i % Wo);
        const int y = (int)((i / Wo) % Ho);
        const int f = (int)((i / plane) % F);
        const int n = (int)(i / (plane * F));
        float v[3];
        sample3(src, n, f, y, x, resize, sy, sx, H, W, v);
        float* o = out + (((long long)n * F + f) * 3 * Ho + y) * Wo + x;
        o[0] = v[0]; o[plane] = v[1]; o[2 * plane] = v[2];
    }
}

// sixteen elements of one Focus pixel -> dst (two or four 16-byte stores)
template <typename T>
__device__ __forceinline__ void focus_store(const typename T::elem (&o)[16], typename T::elem* dst_elems) {
    typedef typename T::elem elem;
    uint4* dst = reinterpret_cast<uint4*>(dst_elems);
    constexpr int NV = (int)(16 * sizeof(elem) / 16);
    uint4 v[NV];
    __builtin_memcpy(v, o, sizeof(o));
#pragma unroll
    for (int k = 0; k < NV; ++k) dst[k] = v[k];
}

// focus_pixel for a source that delivers whole pixels (NV12).  FAST (a wave-uniform property of the image, nv12_fast_ok, and no
// canvas resize): a Focus pixel wholly inside the image comes from nv12_focus_block's wide loads.
template <typename T, typename S>
__device__ __forceinline__ void focus_pixel3(const S& src, bool fast, int n, int f, int h2, int w2, bool resize, float sy, float sx,
                                             int H, int W, typename T::elem* dst_elems) {
    typedef typename T::elem elem;
    elem o[16];
    if (fast && 2 * h2 + 1 < src.g.hs && 2 * w2 + 1 < src.g.ws) {
        int px[2][2][3];
        const bool mirror = src.mirrored(n);
        nv12_focus_block(src.image(n, f), src.chroma(n, f), src.g, mirror, h2, w2, px);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                o[q * 3 + c] = T::from_f32((float)(mirror ? px[q & 1][1 - (q >> 1)][c] : px[q & 1][q >> 1][c]));
        }
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v[3];
            sample3(src, n, f, 2 * h2 + (q & 1), 2 * w2 + (q >> 1), resize, sy, sx, H, W, v);
#pragma unroll
            for (int c = 0; c < 3; ++c) o[q * 3 + c] = T::from_f32(v[c]);
        }
    }
#pragma unroll
    for (int c = 12; c < 16; ++c) o[c] = T::from_f32(0.0f);
    focus_store<T>(o, dst_elems);
}

// NV12 -> Focus-packed NHWC16, the indexing of frames_to_focus_kernel.  FAST: chosen per launch by the host (nv12_fast_ok over
// both base pointers and the image stride, no canvas resize)
template <typename T, bool FAST>
__global__ __launch_bounds__(kBlock) void frames_nv12_to_focus_kernel(FrameSrcNV12 src, int B, int F, int H, int W, int Ho, int Wo,
                                                                      typename T::elem* out0, typename T::elem* out1) {
    const bool resize = Ho != H || Wo != W;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const int H2 = Ho >> 1, W2 = Wo >> 1;
    const long long per_frame = (long long)B * H2 * W2;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < per_frame * F; i += (long long)gridDim.x * kBlock) {
        const int f = (int)(i / per_frame);
        const long long r = i - f * per_frame;
        const int w2 = (int)(r % W2);
        const int h2 = (int)((r / W2) % H2);
        const int n = (int)(r / ((long long)W2 * H2));
        focus_pixel3<T>(src, FAST, n, f, h2, w2, resize, sy, sx, H, W, (f == 0 ? out0 : out1) + r * 16);
    }
}

// one Focus-packed output pixel (h2, w2) of image n, frame f -> 16 elements at dst
template <typename T, typename S>
__device__ __forceinline__ void focus_pixel(const S& src, int n, int f, int h2, int w2, bool resize, float sy, float sx, int H, int W,
                                            typename T::elem* dst_elems) {
    typedef typename T::elem elem;
    elem o[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = 2 * h2 + (q & 1), x = 2 * w2 + (q >> 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[q * 3 + c] = T::from_f32(sample(src, n, f, c, y, x, resize, sy, sx, H, W));
    }
#pragma unroll
    for (int c = 12; c < 16; ++c) o[c] = T::from_f32(0.0f);
    uint4* dst = reinterpret_cast<uint4*>(dst_elems);
    constexpr int NV = (int)(16 * sizeof(elem) / 16);
    uint4 v[NV];
    __builtin_memcpy(v, o, sizeof(o));
#pragma unroll
    for (int k = 0; k < NV; ++k) dst[k] = v[k];
}

// -> Focus-packed NHWC16 [B, Ho/2, Wo/2, 16] per frame (12 real channels, q*3 + c with q = TL, BL, TR, BR; 4 zero)
template <typename T, typename S>
__global__ __launch_bounds__(kBlock) void frames_to_focus_kernel(S src, int B, int F, int H, int W, int Ho, int Wo,
                                                                 typename T::elem* out0, typename T::elem* out1) {
    const bool resize = Ho != H || Wo != W;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const int H2 = Ho >> 1, W2 = Wo >> 1;
    const long long per_frame = (long long)B * H2 * W2;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < per_frame * F; i += (long long)gridDim.x * kBlock) {
        const int f = (int)(i / per_frame);
        const long long r = i - f * per_frame;
        const int w2 = (int)(r % W2);
        const int h2 = (int)((r / W2) % H2);
        const int n = (int)(r / ((long long)W2 * H2));
        focus_pixel<T>(src, n, f, h2, w2, resize, sy, sx, H, W, (f == 0 ? out0 : out1) + r * 16);
    }
}

// ---- per-row sources (sy_frames_u8_pack_rows: D = sy_frame_src; sy_frames_u8_pack_surfaces: D = sy_frame_surf): blockIdx.y =
// the batch row, its workgroups stride over that row's outputs.  The grid depends on (B, Ho, Wo, layout) only: a recorded
// launch serves any table contents.
template <typename D>
__global__ __launch_bounds__(kBlock) void rows_to_nchw_kernel(const D* rows, int H, int W, int Ho, int Wo, float* out) {
    const int n = blockIdx.y;
    const RowSrc src(rows, n, H, W);
    const bool resize = Ho != H || Wo != W;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const int per_row = 3 * Ho * Wo;
    float* o = out + (long long)n * per_row;
    if (src.fmt == SY_PIX_NV12) {                               // (scalar) one thread per pixel, three planes from one conversion
        const int plane = Ho * Wo;
        for (int i = blockIdx.x * kBlock + threadIdx.x; i < plane; i += gridDim.x * kBlock) {
            float v[3];
            sample3(src, n, 0, i / Wo, i % Wo, resize, sy, sx, H, W, v);
            o[i] = v[0]; o[plane + i] = v[1]; o[2 * plane + i] = v[2];
        }
        return;
    }
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < per_row; i += gridDim.x * kBlock) {
        const int x = i % Wo, y = (i / Wo) % Ho, c = i / (Wo * Ho);
        o[i] = sample(src, n, 0, c, y, x, resize, sy, sx, H, W);
    }
}

template <typename T, typename D>
__global__ __launch_bounds__(kBlock) void rows_to_focus_kernel(const D* rows, int H, int W, int Ho, int Wo,
                                                               typename T::elem* out) {
    const int n = blockIdx.y;
    const RowSrc src(rows, n, H, W);
    const bool resize = Ho != H || Wo != W;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const int H2 = Ho >> 1, W2 = Wo >> 1;
    const int per_row = H2 * W2;
    typename T::elem* o = out + (long long)n * per_row * 16;
    if (src.fmt == SY_PIX_NV12) {                               // (scalar: the whole workgroup one way)
        const bool fast = src.fast && !resize;
        for (int r = blockIdx.x * kBlock + threadIdx.x; r < per_row; r += gridDim.x * kBlock)
            focus_pixel3<T>(src, fast, n, 0, r / W2, r % W2, resize, sy, sx, H, W, o + (long long)r * 16);
        return;
    }
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < per_row; r += gridDim.x * kBlock)
        focus_pixel<T>(src, n, 0, r / W2, r % W2, resize, sy, sx, H, W, o + (long long)r * 16);
}

// workgroups per batch row: enough for the row's outputs, the whole grid capped like grid_for's
inline dim3 rows_grid(long long per_row, int B) {
    long long gx = (per_row + kBlock - 1) / kBlock, cap = (256 * 8 + B - 1) / B;
    if (gx > cap) gx = cap;
    return dim3((unsigned)(gx < 1 ? 1 : gx), (unsigned)B);
}

}  // namespace

namespace {

// S = FrameSrc (BGR: the launches sy_frames_u8_pack always made) or FrameSrcRGB
template <typename S>
int frames_pack_launch(const S& src, int B, int F, int H, int W, int Ho, int Wo, int layout, void* out_cur, void* out_sup, int dtype,
                       void* stream) {
    if (layout == SY_FRAMES_NCHW) {
        const long long work = (long long)B * F * 3 * Ho * Wo;
        SY_LAUNCH((frames_to_nchw_kernel<S>), dim3(grid_for(work)), dim3(kBlock), 0, stream, src, B, F, H, W, Ho, Wo,
                  (float*)out_cur);
        return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
    }
    if (layout != SY_FRAMES_FOCUS) return SY_ERR_ARG;
    if ((Ho & 1) || (Wo & 1) || (F == 2 && out_sup == nullptr)) return SY_ERR_ARG;
    const long long work = (long long)B * F * (Ho / 2) * (Wo / 2);
    SY_DISPATCH_DTYPE(dtype, SY_LAUNCH((frames_to_focus_kernel<T, S>), dim3(grid_for(work)), dim3(kBlock), 0, stream,
                                       src, B, F, H, W, Ho, Wo, (typename T::elem*)out_cur, (typename T::elem*)out_sup));
}

int frames_pack_launch_nv12(const FrameSrcNV12& src, int B, int F, int H, int W, int Ho, int Wo, int layout, void* out_cur,
                            void* out_sup, int dtype, void* stream) {
    if (layout == SY_FRAMES_NCHW) {
        const long long work = (long long)B * F * Ho * Wo;
        SY_LAUNCH(frames_nv12_to_nchw_kernel, dim3(grid_for(work)), dim3(kBlock), 0, stream, src, B, F, H, W, Ho, Wo,
                  (float*)out_cur);
        return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
    }
    if (layout != SY_FRAMES_FOCUS) return SY_ERR_ARG;
    if ((Ho & 1) || (Wo & 1) || (F == 2 && out_sup == nullptr)) return SY_ERR_ARG;
    const long long work = (long long)B * F * (Ho / 2) * (Wo / 2);
    const unsigned long long bits = (unsigned long long)(uintptr_t)src.img[0] | (unsigned long long)(uintptr_t)src.img[1] |
                                    (unsigned long long)src.image_stride;
    if (Ho == H && Wo == W && nv12_fast_ok(src.g, bits)) {
        SY_DISPATCH_DTYPE(dtype, SY_LAUNCH((frames_nv12_to_focus_kernel<T, true>), dim3(grid_for(work)), dim3(kBlock), 0, stream,
                                           src, B, F, H, W, Ho, Wo, (typename T::elem*)out_cur, (typename T::elem*)out_sup));
    }
    SY_DISPATCH_DTYPE(dtype, SY_LAUNCH((frames_nv12_to_focus_kernel<T, false>), dim3(grid_for(work)), dim3(kBlock), 0, stream,
                                       src, B, F, H, W, Ho, Wo, (typename T::elem*)out_cur, (typename T::elem*)out_sup));
}

}  // namespace

extern "C" int sy_frames_u8_pack_fmt(const uint8_t* cur, const uint8_t* sup, int B, int Hs, int Ws, int64_t image_stride,
                                     int row_stride, int decimate, const uint8_t* mirror, int H, int W, int Ho, int Wo,
                                     int layout, void* out_cur, void* out_sup, int dtype, int format, void* stream) {
    if (cur == nullptr || out_cur == nullptr || B <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0)
        return SY_ERR_ARG;
    if (format != SY_PIX_BGR && format != SY_PIX_RGB && format != SY_PIX_NV12) return SY_ERR_ARG;
    const bool nv12 = format == SY_PIX_NV12;
    if (decimate < -1 || decimate > 2) return SY_ERR_UNSUPPORTED;
    if ((decimate == 2 || nv12) && ((Hs & 1) || (Ws & 1))) return SY_ERR_UNSUPPORTED;
    if (nv12 ? (row_stride < Ws || image_stride < (int64_t)row_stride * Hs * 3 / 2)
             : (row_stride < Ws * 3 || image_stride < (int64_t)row_stride * Hs)) return SY_ERR_ARG;
    FrameSrc src;
    const int rc = frame_geom(Hs, Ws, decimate, H, W, src.g);
    if (rc != SY_OK) return rc;
    const int F = sup != nullptr ? 2 : 1;
    src.img[0] = cur; src.img[1] = sup; src.image_stride = image_stride; src.g.row_stride = row_stride;
    src.mirror = mirror;
    if (nv12) {
        FrameSrcNV12 s;
        static_cast<FrameSrc&>(s) = src;
        return frames_pack_launch_nv12(s, B, F, H, W, Ho, Wo, layout, out_cur, out_sup, dtype, stream);
    }
    if (format == SY_PIX_RGB) {
        FrameSrcRGB s;
        static_cast<FrameSrc&>(s) = src;
        return frames_pack_launch(s, B, F, H, W, Ho, Wo, layout, out_cur, out_sup, dtype, stream);
    }
    return frames_pack_launch(src, B, F, H, W, Ho, Wo, layout, out_cur, out_sup, dtype, stream);
}

extern "C" int sy_frames_u8_pack(const uint8_t* cur, const uint8_t* sup, int B, int Hs, int Ws, int64_t image_stride,
                                 int row_stride, int decimate, const uint8_t* mirror, int H, int W, int Ho, int Wo,
                                 int layout, void* out_cur, void* out_sup, int dtype, void* stream) {
    return sy_frames_u8_pack_fmt(cur, sup, B, Hs, Ws, image_stride, row_stride, decimate, mirror, H, W, Ho, Wo, layout, out_cur,
                                 out_sup, dtype, SY_PIX_BGR, stream);
}

namespace {

template <typename D>
int rows_pack_launch(const D* rows, int B, int H, int W, int Ho, int Wo, int layout, void* out_cur, int dtype, void* stream) {
    if (rows == nullptr || out_cur == nullptr || B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return SY_ERR_ARG;
    if (dtype != SY_DT_BF16 && dtype != SY_DT_F16 && dtype != SY_DT_F32) return SY_ERR_ARG;
    if (B > 65535 || (long long)3 * Ho * Wo > (1LL << 30)) return SY_ERR_UNSUPPORTED;      // grid.y; 32-bit per-row indices + stride
    if (layout == SY_FRAMES_NCHW) {
        if (dtype != SY_DT_F32) return SY_ERR_ARG;
        SY_LAUNCH((rows_to_nchw_kernel<D>), rows_grid((long long)3 * Ho * Wo, B), dim3(kBlock), 0, stream, rows, H, W, Ho, Wo,
                  (float*)out_cur);
        return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
    }
    if (layout != SY_FRAMES_FOCUS) return SY_ERR_ARG;
    if ((Ho & 1) || (Wo & 1)) return SY_ERR_ARG;
    const dim3 grid = rows_grid((long long)(Ho / 2) * (Wo / 2), B);
    SY_DISPATCH_DTYPE(dtype, SY_LAUNCH((rows_to_focus_kernel<T, D>), grid, dim3(kBlock), 0, stream, rows, H, W, Ho, Wo,
                                       (typename T::elem*)out_cur));
}

}  // namespace

extern "C" int sy_frames_u8_pack_rows(const sy_frame_src* rows, int B, int H, int W, int Ho, int Wo, int layout, void* out_cur,
                                      int dtype, void* stream) {
    return rows_pack_launch(rows, B, H, W, Ho, Wo, layout, out_cur, dtype, stream);
}

extern "C" int sy_frames_u8_pack_surfaces(const sy_frame_surf* rows, int B, int H, int W, int Ho, int Wo, int layout, void* out_cur,
                                          int dtype, void* stream) {
    return rows_pack_launch(rows, B, H, W, Ho, Wo, layout, out_cur, dtype, stream);
}

extern "C" int sy_resize_bilinear_nchw(const float* in, int N, int C, int H, int W, float* out, int Ho, int Wo,
                                       void* stream) {
    if (in == nullptr || out == nullptr || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return SY_ERR_ARG;
    if (C % 3) return SY_ERR_UNSUPPORTED;                   // frames are 3-channel planes (3 = on_pipe, 6 = a pair)
    PlaneSrc src;
    src.in = in; src.C = C; src.H = H; src.W = W;
    const long long work = (long long)N * C * Ho * Wo;
    SY_LAUNCH((frames_to_nchw_kernel<PlaneSrc>), dim3(grid_for(work)), dim3(kBlock), 0, stream, src, N, C / 3, H, W, Ho, Wo, out);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}
