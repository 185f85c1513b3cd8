// overlay.hip — draw a tick's boxes, class labels and track ids into camera surfaces in device memory, in place.
//
// The opposite direction of sy_frames_u8_pack_surfaces (input_pipeline.hip): what leaves the detector is a list of boxes per
// batch row; whoever feeds a monitor wall, a recorder or an encoder wants them IN the frame, without the host read that
// detect_device exists to avoid.  The rendering rule (seven points) is stated in include/streamyolo_hip.h; this file is one way
// to compute it.
//
// Kernel shape: a gather.  blockIdx = (tile column, tile row, batch row); a workgroup of 256 threads owns one kTileH x kTileW
// tile of one row's surface.
//   1. Thread i resolves list entry i of the row (at most 256 are looked at: one per thread) into integers: the rectangle, the
//      tab rectangle, the label's glyph codes, the class's eight palette bytes.  Everything the rule decides "before clipping"
//      is decided here.
//   2. The entries whose outer rectangle or tab meets the tile are compacted into LDS in list order (a ballot per wave, the
//      four wave counts through LDS).  No entry: the workgroup leaves without touching memory — most of a frame has no box.
//   3. Every thread walks the tile's short list for its own pixels and stops at the first cover (lowest index = on top).
//      BGR / RGB: lane l of wave w owns column l of the tile rows w, w + 4, w + 8, w + 12 — a wave's stores are a run of one
//      surface row.  NV12 / P010: thread i owns the 2 x 2 block (i % 32, i / 32) of the tile with its chroma sample — a wave
//      covers two block rows, its luma stores are two runs of each of four surface rows, its chroma stores two runs.
// No atomics, no thread writes a pixel it does not own, nothing uncovered is written (byte stores only: a store never spans a
// byte the rule does not cover).
#include "sy_device.h"
#include "../../include/streamyolo_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kTileW = SY_OVERLAY_TILE_W, kTileH = SY_OVERLAY_TILE_H;
constexpr int kMaxText = 16;                                     // glyph codes of one label: 8 (name) + 1 + 5 (id) fits
typedef unsigned long long u64;
static_assert(kThreads == SY_OVERLAY_MAX_BOXES, "one list entry per thread");
static_assert(sizeof(sy_overlay_row) == 64, "header and kernel disagree");
static_assert(kTileW == kWave && kTileH % (kThreads / kWave) == 0, "BGR: a wave owns whole tile rows");
static_assert((kTileW / 2) * (kTileH / 2) == kThreads, "NV12 / P010: one 2 x 2 block per thread");

struct Entry {                                                   // one box that meets the tile: 48 bytes of LDS
    int x1, y1, x2, y2;                                          // the rectangle, inclusive
    int ty, tw;                                                  // tab: first row, width in pixels (0: no tab); left edge = x1
    u64 pal;                                                     // the class's palette row, byte i in bits 8 i ..
    u64 text[kMaxText / 8];                                      // glyph codes, likewise (kept in registers while it is built)
    __device__ __forceinline__ unsigned pal_at(int i) const { return (unsigned)(pal >> (8 * i)) & 0xFFu; }
    __device__ __forceinline__ unsigned text_at(int i) const { return (unsigned)(text[i >> 3] >> (8 * (i & 7))) & 0xFFu; }
    __device__ __forceinline__ void put(int i, unsigned code) {
        if (i < 8) text[0] |= (u64)code << (8 * i);
        else text[1] |= (u64)code << (8 * (i - 8));
    }
};

struct Lds {
    Entry e[kThreads];
    int wave_n[kThreads / kWave];
};

// floor(c / divisor + 0.5) as an integer; false: not finite
__device__ __forceinline__ bool round_px(float c, float divisor, int& out) {
    const float v = c / divisor + 0.5f;
    if (!(fabsf(c) <= 3.0e38f) || !(fabsf(v) <= 3.0e38f)) return false;       // (NaN fails both comparisons)
    const float f = fminf(fmaxf(floorf(v), -1073741824.0f), 1073741824.0f);
    out = (int)f;
    return true;
}

// what covers pixel (x, y): -1 nothing, else 2 k + (1: a glyph pixel of entry k's tab)
__device__ __forceinline__ int cover(const Entry* e, int m, int x, int y, int t, int s, const uint8_t* glyphs) {
    for (int k = 0; k < m; ++k) {
        const Entry& b = e[k];
        if (b.tw > 0 && x >= b.x1 && x < b.x1 + b.tw && y >= b.ty && y < b.ty + 8 * s) {
            const int px = (x - b.x1) / s, py = (y - b.ty) / s;  // font pixel: column over the whole string, row
            const unsigned code = b.text_at(px >> 3);
            const unsigned bits = code < 64u ? glyphs[code * 8 + py] : 0u;
            return 2 * k + (int)((bits >> (7 - (px & 7))) & 1u);
        }
        if (x >= b.x1 && x <= b.x2 && y >= b.y1 && y <= b.y2 &&
            !(x >= b.x1 + t && x <= b.x2 - t && y >= b.y1 + t && y <= b.y2 - t))
            return 2 * k;
    }
    return -1;
}

__global__ __launch_bounds__(kThreads) void overlay_draw_kernel(const sy_overlay_row* rows, const float* boxes, int layout, int max_list,
                                                                const int32_t* ids, const int32_t* cnt, const uint8_t* palette,
                                                                const uint8_t* class_text, int num_classes, const uint8_t* glyphs) {
    __shared__ Lds sm;
    const int b = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int tx0 = (int)blockIdx.x * kTileW, ty0 = (int)blockIdx.y * kTileH;
    const sy_overlay_row d = rows[b];                            // one 64-byte load per workgroup (b: uniform)

    // ---- the row's surface; everything here is uniform over the workgroup, so is every early return ----
    if (d.plane0 == nullptr || d.Hs <= 0 || d.Ws <= 0 || tx0 >= d.Ws || ty0 >= d.Hs) return;
    if (d.format != SY_PIX_BGR && d.format != SY_PIX_RGB && d.format != SY_PIX_NV12 && d.format != SY_PIX_P010) return;
    const bool yuv = d.format == SY_PIX_NV12 || d.format == SY_PIX_P010;
    const int sh = d.format == SY_PIX_P010 ? 1 : 0;
    if (yuv && ((d.Hs & 1) || (d.Ws & 1))) return;
    const long long row_bytes = yuv ? ((long long)d.Ws << sh) : (long long)d.Ws * 3;
    if ((long long)d.row_stride < row_bytes) return;
    const int cpitch = d.chroma_stride != 0 ? d.chroma_stride : d.row_stride;
    if (yuv && (d.chroma_stride < 0 || (long long)cpitch < row_bytes)) return;
    int n = sy_min(sy_min(cnt[b], max_list), kThreads);
    if (d.max_boxes > 0) n = sy_min(n, d.max_boxes);
    if (n <= 0) return;
    const int t = sy_min(sy_max(d.thickness, 1), 16), s = sy_min(sy_max(d.text_scale, 0), 4);
    const int tx1 = sy_min(tx0 + kTileW, d.Ws) - 1, ty1 = sy_min(ty0 + kTileH, d.Hs) - 1;      // the tile inside the surface, inclusive

    // ---- 1. list entry `tid` ----
    Entry e;
    bool hit = false;
    if (tid < n) {
        const int cols = layout == 0 ? 7 : 6;
        const float* r = boxes + ((long long)b * max_list + tid) * cols;
        const float score = layout == 0 ? r[4] * r[5] : r[4];
        const float cls_f = layout == 0 ? r[6] : r[5];
        bool ok = score >= d.min_score;                          // (a NaN score is not drawn)
        ok = round_px(r[0], d.divisor, e.x1) && ok;
        ok = round_px(r[1], d.divisor, e.y1) && ok;
        ok = round_px(r[2], d.divisor, e.x2) && ok;
        ok = round_px(r[3], d.divisor, e.y2) && ok;
        if (ok) {
            e.x2 -= 1; e.y2 -= 1;
            ok = e.x2 >= e.x1 && e.y2 >= e.y1;
        }
        if (ok) {
            const int cls = cls_f >= 0.0f && cls_f < (float)num_classes ? (int)cls_f : -1;
            const uint8_t* pal = palette + (cls < 0 ? 0 : cls) * 8;
            e.pal = 0; e.text[0] = 0; e.text[1] = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) e.pal |= (u64)pal[i] << (8 * i);
            int L = 0;
            if (s > 0) {
                if (cls >= 0 && class_text != nullptr)
                    for (; L < 8 && class_text[cls * 8 + L] != 0xFF; ++L) e.put(L, class_text[cls * 8 + L]);
                if ((d.flags & SY_OVERLAY_ID) && ids != nullptr) {
                    int v = ids[(long long)b * max_list + tid] % 100000;
                    if (v < 0) v += 100000;
                    ++L;                                         // ' ' = code 0
                    int div = 10000;
                    while (div > 1 && v < div) div /= 10;        // no leading zeros
                    for (; div >= 1; div /= 10) e.put(L++, 16u + (unsigned)((v / div) % 10));      // '0' = ASCII 48 = code 16
                } else if (d.flags & SY_OVERLAY_SCORE) {
                    const int v = sy_min(sy_max((int)(100.0f * score), 0), 99);
                    ++L;
                    e.put(L++, 16u + (unsigned)(v / 10));
                    e.put(L++, 16u + (unsigned)(v % 10));
                    e.put(L++, 5u);                              // '%' = ASCII 37
                }
            }
            e.tw = 8 * s * L;
            e.ty = e.y1 - 8 * s < 0 ? e.y1 : e.y1 - 8 * s;
            hit = e.x1 <= tx1 && e.x2 >= tx0 && e.y1 <= ty1 && e.y2 >= ty0;
            if (e.tw > 0) hit = hit || (e.x1 <= tx1 && e.x1 + e.tw - 1 >= tx0 && e.ty <= ty1 && e.ty + 8 * s - 1 >= ty0);
        }
    }

    // ---- 2. compact, order kept ----
    const unsigned long long hits = __ballot(hit ? 1 : 0);
    if (lane == 0) sm.wave_n[wave] = __popcll(hits);
    __syncthreads();
    int base = 0, m = 0;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) {
        base += w < wave ? sm.wave_n[w] : 0;
        m += sm.wave_n[w];
    }
    if (m == 0) return;                                          // (uniform) nothing of any box in this tile
    if (hit) sm.e[base + __popcll(hits & ((1ull << lane) - 1ull))] = e;
    __syncthreads();

    // ---- 3. own pixels ----
    if (!yuv) {
        const int x = tx0 + lane;
        if (x >= d.Ws) return;
        const int c0 = d.format == SY_PIX_RGB ? 2 : 0;           // palette byte of the pixel's first channel
        for (int i = wave; i < kTileH; i += kThreads / kWave) {
            const int y = ty0 + i;
            if (y >= d.Hs) break;
            const int c = cover(sm.e, m, x, y, t, s, glyphs);
            if (c < 0) continue;
            const Entry& b = sm.e[c >> 1];
            uint8_t* p = d.plane0 + (long long)y * d.row_stride + (long long)x * 3;
            const unsigned char v0 = (unsigned char)b.pal_at((c & 1) ? 3 : c0), v1 = (unsigned char)b.pal_at((c & 1) ? 3 : 1),
                                v2 = (unsigned char)b.pal_at((c & 1) ? 3 : 2 - c0);
            p[0] = v0; p[1] = v1; p[2] = v2;
        }
        return;
    }
    const int x = tx0 + 2 * (tid & (kTileW / 2 - 1)), y = ty0 + 2 * (tid / (kTileW / 2));
    if (x >= d.Ws || y >= d.Hs) return;                          // (even sizes: the whole block is inside or outside)
    uint8_t* chroma = d.plane1 != nullptr ? d.plane1 : d.plane0 + (long long)d.row_stride * d.Hs;
    int first = -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int px = x + (q & 1), py = y + (q >> 1);
        const int c = cover(sm.e, m, px, py, t, s, glyphs);
        if (c < 0) continue;
        if (first < 0) first = c;
        uint8_t* p = d.plane0 + (long long)py * d.row_stride + ((long long)px << sh);
        const unsigned char v = (unsigned char)sm.e[c >> 1].pal_at((c & 1) ? 7 : 4);
        if (sh) { p[0] = 0; p[1] = v; } else p[0] = v;
    }
    if (first < 0) return;
    const unsigned char u = (first & 1) ? 128 : (unsigned char)sm.e[first >> 1].pal_at(5),
                        v = (first & 1) ? 128 : (unsigned char)sm.e[first >> 1].pal_at(6);
    uint8_t* p = chroma + (long long)(y >> 1) * cpitch + ((long long)x << sh);       // pair x / 2: 2 samples of 1 << sh bytes
    if (sh) { p[0] = 0; p[1] = u; p[2] = 0; p[3] = v; } else { p[0] = u; p[1] = v; }
}

}  // namespace

extern "C" int sy_overlay_draw(const sy_overlay_row* rows, int B, int Hmax, int Wmax, const float* boxes, int layout, int max_list,
                               const int32_t* ids, const int32_t* cnt, const uint8_t* palette, const uint8_t* class_text,
                               int num_classes, const uint8_t* glyphs, void* stream) {
    if (rows == nullptr || boxes == nullptr || cnt == nullptr || palette == nullptr || glyphs == nullptr || B <= 0 || Hmax <= 0 ||
        Wmax <= 0 || max_list <= 0 || num_classes <= 0 || (layout != 0 && layout != 1))
        return SY_ERR_ARG;
    if (num_classes > 128 || B > 65535 || (Hmax + kTileH - 1) / kTileH > 65535) return SY_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((Wmax + kTileW - 1) / kTileW), (unsigned)((Hmax + kTileH - 1) / kTileH), (unsigned)B);
    SY_LAUNCH(overlay_draw_kernel, grid, dim3(kThreads), 0, stream, rows, boxes, layout, max_list, ids, cnt, palette, class_text,
              num_classes, glyphs);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}
