// redact.hip — pixelate or fill a tick's boxes in camera surfaces in device memory, in place.
//
// The third gather beside overlay.hip and crop.hip: what leaves the pipeline towards a recorder, a monitor wall or a dataset
// export is the frame WITHOUT the people and vehicles in it, and the box lists (with tracking: lists that survive a missed
// detection) already lie in device memory.  The rule (nine points) is stated in include/streamyolo_hip.h; this file is one way
// to compute it.
//
// Kernel shape: blockIdx = (tile column, tile row, batch row); a workgroup of 256 threads owns one kTileH x kTileW tile of one
// row's surface.  Both tile sides are multiples of the largest cell (32) and cells are aligned to the surface origin, so EVERY
// CELL LIES IN EXACTLY ONE TILE: a workgroup reads only pixels it owns, reads all of them before a barrier and writes behind it —
// no workgroup reads a byte another one writes, which is what makes pixelation in place safe.
//   1. The row's list is walked in chunks of 256 (one entry per thread, no cap on the list): an entry is resolved into the padded
//      integer rectangle, the ones that meet the tile are compacted into LDS (a ballot per wave, the four wave counts through LDS,
//      as overlay.hip) and every thread ORs the chunk's cover of its own pixels into a register.  Coverage is a union: no order.
//      No entry of any chunk meets the tile: the workgroup leaves without touching pixel memory — most of a frame has no box.
//   2. PIXELATE: covered pixels flag their cell; the pixels of flagged cells are read (covered or not) and summed per cell —
//      in registers down a thread's rows, across neighbouring lanes by two shuffles, then integer LDS adds (order-independent);
//      one thread per cell divides.  A cell nobody flagged is neither read nor written.
//   3. Covered pixels take the cell's mean or the fill colour.  Byte stores only: a store never spans a byte the rule leaves alone.
// BGR / RGB: lane l of wave w owns column l of the tile rows 8 w .. 8 w + 7 — a wave's accesses are runs of one surface row.
// NV12 / P010: thread i owns the 2 x 2 blocks (i % 32, i / 32) and (i % 32, i / 32 + 8) of the tile with their chroma samples —
// a wave covers two block rows, runs of four luma rows and two chroma rows.
#include "sy_device.h"
#include "../../include/streamyolo_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kTileW = SY_REDACT_TILE_W, kTileH = SY_REDACT_TILE_H;
constexpr int kRows = kTileH / kWaves;                           // BGR / RGB: tile rows of one wave
constexpr int kMinCell = 4, kMaxCell = 32;
constexpr int kCellsX = kTileW / kMinCell, kCellsY = kTileH / kMinCell;
constexpr int kCells = kCellsX * kCellsY;                        // cells of a tile at the smallest cell size
static_assert(sizeof(sy_redact_row) == 88, "header and kernel disagree");
static_assert(kTileW % kMaxCell == 0 && kTileH % kMaxCell == 0, "every cell lies in exactly one tile");
static_assert(kTileW == kWave && kRows * kWaves == kTileH, "BGR: a wave owns whole tile rows");
static_assert((kTileW / 2) * (kTileH / 2) == 2 * kThreads, "NV12 / P010: two 2 x 2 blocks per thread");
static_assert(kCells <= kThreads, "one thread per cell divides");

struct Entry {                                                   // one entry that meets the tile: 32 bytes of LDS
    int x1, y1, x2, y2;                                          // the padded rectangle clipped to the tile, inclusive
    int cx, cy;                                                  // ellipse: 2 X1 + W, 2 Y1 + H of the UNCLIPPED padded rectangle
    int w, h;                                                    // ellipse: its W and H (<= SY_REDACT_MAX_SIDE); 0: a rectangle
};

struct Lds {
    Entry e[kThreads];
    int wave_n[2][kWaves];                                       // double-buffered over the chunks: one barrier per empty chunk
    unsigned flag[kCells];                                       // the cell has a covered pixel
    unsigned sum[kCells][3];                                     // B, G, R or Y, U, V: the cell's sums, then its means
};

// floor(c / divisor + 0.5) as an integer; false: not finite (overlay.hip's round_px: the same rule 1)
__device__ __forceinline__ bool round_px(float c, float divisor, int& out) {
    const float v = c / divisor + 0.5f;
    if (!(fabsf(c) <= 3.0e38f) || !(fabsf(v) <= 3.0e38f)) return false;       // (NaN fails both comparisons)
    const float f = fminf(fmaxf(floorf(v), -1073741824.0f), 1073741824.0f);
    out = (int)f;
    return true;
}

// rule 3 over the tile's short list: does any entry cover pixel (x, y)?
__device__ __forceinline__ bool covered(const Entry* e, int m, int x, int y) {
    for (int k = 0; k < m; ++k) {
        const Entry& b = e[k];
        if (x < b.x1 || x > b.x2 || y < b.y1 || y > b.y2) continue;
        if (b.w == 0) return true;
        // |dx| < 2 W and |dy| < 2 H inside the rectangle, W and H <= 2^14: every product stays below 2^60
        const long long dx = (long long)(2 * x + 1) - b.cx, dy = (long long)(2 * y + 1) - b.cy;
        const long long ww = (long long)b.w * b.w, hh = (long long)b.h * b.h;
        if (dx * dx * hh + dy * dy * ww <= ww * hh) return true;
    }
    return false;
}

__global__ __launch_bounds__(kThreads) void redact_kernel(const sy_redact_row* rows, const float* boxes, int layout, int max_list,
                                                          const int32_t* cnt) {
    __shared__ Lds sm;
    const int b = (int)blockIdx.z, tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int tx0 = (int)blockIdx.x * kTileW, ty0 = (int)blockIdx.y * kTileH;
    const sy_redact_row d = rows[b];                             // one 88-byte load per workgroup (b: uniform)

    // ---- the row's surface (rule 9); everything here is uniform over the workgroup, so is every early return ----
    if (d.plane0 == nullptr || d.Hs <= 0 || d.Ws <= 0 || tx0 >= d.Ws || ty0 >= d.Hs) return;
    if (d.format != SY_PIX_BGR && d.format != SY_PIX_RGB && d.format != SY_PIX_NV12 && d.format != SY_PIX_P010) return;
    const bool yuv = d.format == SY_PIX_NV12 || d.format == SY_PIX_P010;
    const int sh = d.format == SY_PIX_P010 ? 1 : 0;
    if (yuv && ((d.Hs & 1) || (d.Ws & 1))) return;
    const long long row_bytes = yuv ? ((long long)d.Ws << sh) : (long long)d.Ws * 3;
    if ((long long)d.row_stride < row_bytes) return;
    const int cpitch = d.chroma_stride != 0 ? d.chroma_stride : d.row_stride;
    if (yuv && (d.chroma_stride < 0 || (long long)cpitch < row_bytes)) return;
    if (d.cell != 4 && d.cell != 8 && d.cell != 16 && d.cell != 32) return;
    if ((d.mode != SY_REDACT_PIXELATE && d.mode != SY_REDACT_FILL) || (d.shape != SY_REDACT_RECT && d.shape != SY_REDACT_ELLIPSE)) return;
    const int n = sy_min(cnt[b], max_list);
    if (n <= 0) return;
    const int lg = d.cell == 4 ? 2 : d.cell == 8 ? 3 : d.cell == 16 ? 4 : 5;
    const int tx1 = sy_min(tx0 + kTileW, d.Ws) - 1, ty1 = sy_min(ty0 + kTileH, d.Hs) - 1;      // the tile inside the surface, inclusive
    const long long pad = sy_min(sy_max(d.pad_q8, 0), 256);

    if (tid < kCells) {                                          // (ordered before their first use by the first chunk's barrier)
        sm.flag[tid] = 0u;
        sm.sum[tid][0] = 0u; sm.sum[tid][1] = 0u; sm.sum[tid][2] = 0u;
    }

    // own pixels.  BGR / RGB: (px, py0 + r), r < 8.  NV12 / P010: the blocks at (px, py0) and (px, py0 + 16); bit 4 j + q of `cov`
    // is pixel (px + (q & 1), py0 + 16 j + (q >> 1))
    const int px = yuv ? tx0 + 2 * (tid & (kTileW / 2 - 1)) : tx0 + lane;
    const int py0 = yuv ? ty0 + 2 * (tid / (kTileW / 2)) : ty0 + wave * kRows;
    const bool in_x = px < d.Ws;                                 // (even sizes: a whole block is inside or outside)
    unsigned cov = 0u;

    // ---- 1. the list in chunks of 256: resolve, compact, OR the cover of the own pixels ----
    bool any = false;
    for (int k0 = 0, turn = 0; k0 < n; k0 += kThreads, ++turn) {
        Entry e;
        bool hit = false;
        const int k = k0 + tid;
        if (k < n) {
            const float* r = boxes + ((long long)b * max_list + k) * (layout == 0 ? 7 : 6);
            const float score = layout == 0 ? r[4] * r[5] : r[4];
            const float cls_f = layout == 0 ? r[6] : r[5];
            int X1 = 0, Y1 = 0, X2 = 0, Y2 = 0;
            bool ok = score >= d.min_score;                      // (a NaN score is skipped)
            ok = round_px(r[0], d.divisor, X1) && ok;
            ok = round_px(r[1], d.divisor, Y1) && ok;
            ok = round_px(r[2], d.divisor, X2) && ok;
            ok = round_px(r[3], d.divisor, Y2) && ok;
            ok = ok && cls_f >= 0.0f && cls_f < 128.0f;          // (a NaN class is skipped)
            if (ok) {
                const int cls = (int)cls_f;
                const unsigned word = cls < 64 ? (cls < 32 ? d.class_mask[0] : d.class_mask[1]) : (cls < 96 ? d.class_mask[2] : d.class_mask[3]);
                X2 -= 1; Y2 -= 1;
                ok = ((word >> (cls & 31)) & 1u) != 0u && X2 >= X1 && Y2 >= Y1;
            }
            if (ok) {                                            // rule 2 in 64 bits: |r(c)| <= 2^30, nothing overflows
                long long x1 = X1, y1 = Y1, x2 = X2, y2 = Y2;
                long long W = x2 - x1 + 1, H = y2 - y1 + 1;
                const long long gx = (W * pad + 128) >> 8, gy = (H * pad + 128) >> 8;
                x1 -= gx; x2 += gx; y1 -= gy; y2 += gy;
                W += 2 * gx; H += 2 * gy;
                hit = x1 <= tx1 && x2 >= tx0 && y1 <= ty1 && y2 >= ty0;
                if (hit) {                                       // clipped to the tile everything fits 32 bits
                    e.x1 = (int)sy_max(x1, (long long)tx0); e.x2 = (int)sy_min(x2, (long long)tx1);
                    e.y1 = (int)sy_max(y1, (long long)ty0); e.y2 = (int)sy_min(y2, (long long)ty1);
                    // an ellipse no larger than the limit that meets the tile starts within 2^14 pixels of it
                    const bool ell = d.shape == SY_REDACT_ELLIPSE && W <= SY_REDACT_MAX_SIDE && H <= SY_REDACT_MAX_SIDE;
                    e.w = ell ? (int)W : 0; e.h = ell ? (int)H : 0;
                    e.cx = ell ? (int)(2 * x1 + W) : 0; e.cy = ell ? (int)(2 * y1 + H) : 0;
                }
            }
        }
        const unsigned long long hits = __ballot(hit ? 1 : 0);
        int* wn = sm.wave_n[turn & 1];
        if (lane == 0) wn[wave] = __popcll(hits);
        __syncthreads();
        int base = 0, m = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            base += w < wave ? wn[w] : 0;
            m += wn[w];
        }
        if (m == 0) continue;                                    // (uniform) nothing of this chunk in this tile
        any = true;
        if (hit) sm.e[base + __popcll(hits & ((1ull << lane) - 1ull))] = e;
        __syncthreads();
        if (!in_x) continue;                                     // (the barriers above are the chunk's only ones)
        if (!yuv) {
#pragma unroll
            for (int r = 0; r < kRows; ++r)
                if (!((cov >> r) & 1u) && py0 + r < d.Hs && covered(sm.e, m, px, py0 + r)) cov |= 1u << r;
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int y = py0 + (kTileH / 2) * (q >> 2) + ((q >> 1) & 1);
                if (!((cov >> q) & 1u) && y < d.Hs && covered(sm.e, m, px + (q & 1), y)) cov |= 1u << q;
            }
        }
    }
    if (!any) return;                                            // (uniform) no entry meets the tile: no pixel memory is touched

    uint8_t* chroma = d.plane1 != nullptr ? d.plane1 : d.plane0 + (long long)d.row_stride * d.Hs;
    const int c0 = d.format == SY_PIX_RGB ? 2 : 0;               // the byte of a BGR / RGB pixel that holds B
    const int cell_x = (px - tx0) >> lg;                         // the own pixels' cell column in the tile
    auto cell_at = [&](int y) { return ((y - ty0) >> lg) * kCellsX + cell_x; };

    if (d.mode == SY_REDACT_PIXELATE) {
        // ---- 2a. covered pixels flag their cell (every writer stores the same 1) ----
        if (!yuv) {
#pragma unroll
            for (int r = 0; r < kRows; ++r)
                if ((cov >> r) & 1u) sm.flag[cell_at(py0 + r)] = 1u;
        } else {
            if (cov & 0x0Fu) sm.flag[cell_at(py0)] = 1u;
            if (cov & 0xF0u) sm.flag[cell_at(py0 + kTileH / 2)] = 1u;
        }
        __syncthreads();
        // ---- 2b. sum the ORIGINAL pixels of flagged cells.  Every lane takes part in the shuffles: no early exit here ----
        // lanes l ^ 1, l ^ 2 (BGR: columns) or l ^ 1, l ^ 32 (NV12: the next block column / row) lie in the same cell at every cell size
        auto flush = [&](int cell, unsigned s0, unsigned s1, unsigned s2, int m0, int m1) {
            s0 += __shfl_xor(s0, m0); s1 += __shfl_xor(s1, m0); s2 += __shfl_xor(s2, m0);
            s0 += __shfl_xor(s0, m1); s1 += __shfl_xor(s1, m1); s2 += __shfl_xor(s2, m1);
            if ((lane & (m0 | m1)) == 0 && (s0 | s1 | s2) != 0u) {
                atomicAdd(&sm.sum[cell][0], s0); atomicAdd(&sm.sum[cell][1], s1); atomicAdd(&sm.sum[cell][2], s2);
            }
        };
        if (!yuv) {
            unsigned s0 = 0u, s1 = 0u, s2 = 0u;
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                const int y = py0 + r, cell = cell_at(y);
                if (in_x && y < d.Hs && sm.flag[cell] != 0u) {
                    const uint8_t* p = d.plane0 + (long long)y * d.row_stride + (long long)px * 3;
                    s0 += p[0]; s1 += p[1]; s2 += p[2];
                }
                if (r == kRows - 1 || ((y + 1 - ty0) & (d.cell - 1)) == 0) {      // (uniform over the wave) the cell row ends
                    flush(cell, s0, s1, s2, 1, 2);
                    s0 = s1 = s2 = 0u;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int y = py0 + (kTileH / 2) * j, cell = cell_at(y);
                unsigned s0 = 0u, s1 = 0u, s2 = 0u;
                if (in_x && y < d.Hs && sm.flag[cell] != 0u) {
                    const uint8_t* p = d.plane0 + (long long)y * d.row_stride + ((long long)px << sh) + sh;      // P010: the high bytes
                    const uint8_t* q = chroma + (long long)(y >> 1) * cpitch + ((long long)px << sh) + sh;
                    s0 = (unsigned)p[0] + p[1 << sh] + p[d.row_stride] + p[d.row_stride + (1 << sh)];
                    s1 = q[0]; s2 = q[1 << sh];
                }
                flush(cell, s0, s1, s2, 1, 32);
            }
        }
        __syncthreads();
        // ---- 2c. one thread per cell: the rounded means (rule 6; chroma: over the cell's (cell / 2)^2 samples, clipped alike) ----
        if (tid < kCells && sm.flag[tid] != 0u) {
            const int i0 = tx0 + ((tid % kCellsX) << lg), j0 = ty0 + ((tid / kCellsX) << lg);
            const unsigned nx = (unsigned)(sy_min(i0 + d.cell, d.Ws) - i0), ny = (unsigned)(sy_min(j0 + d.cell, d.Hs) - j0);
            const unsigned nl = nx * ny, nc = yuv ? (nx >> 1) * (ny >> 1) : nl;
            sm.sum[tid][0] = (sm.sum[tid][0] + (nl >> 1)) / nl;
            sm.sum[tid][1] = (sm.sum[tid][1] + (nc >> 1)) / nc;
            sm.sum[tid][2] = (sm.sum[tid][2] + (nc >> 1)) / nc;
        }
        __syncthreads();
    }

    // ---- 3. covered pixels take their cell's mean or the fill colour.  Every read of pixel memory lies before the last barrier ----
    if (cov == 0u) return;
    const bool fill = d.mode == SY_REDACT_FILL;
    if (!yuv) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            if (!((cov >> r) & 1u)) continue;
            const int y = py0 + r;
            const unsigned* s = sm.sum[cell_at(y)];
            const unsigned char v0 = (unsigned char)(fill ? d.fill[c0] : s[0]), v1 = (unsigned char)(fill ? d.fill[1] : s[1]),
                                v2 = (unsigned char)(fill ? d.fill[2 - c0] : s[2]);
            uint8_t* p = d.plane0 + (long long)y * d.row_stride + (long long)px * 3;
            p[0] = v0; p[1] = v1; p[2] = v2;
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const unsigned c4 = (cov >> (4 * j)) & 0xFu;
        if (c4 == 0u) continue;
        const int y = py0 + (kTileH / 2) * j;
        const unsigned* s = sm.sum[cell_at(y)];
        const unsigned char vy = (unsigned char)(fill ? d.fill[4] : s[0]), vu = (unsigned char)(fill ? d.fill[5] : s[1]),
                            vv = (unsigned char)(fill ? d.fill[6] : s[2]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!((c4 >> q) & 1u)) continue;
            uint8_t* p = d.plane0 + (long long)(y + (q >> 1)) * d.row_stride + ((long long)(px + (q & 1)) << sh);
            if (sh) { p[0] = 0; p[1] = vy; } else p[0] = vy;
        }
        uint8_t* p = chroma + (long long)(y >> 1) * cpitch + ((long long)px << sh);       // pair px / 2: 2 samples of 1 << sh bytes
        if (sh) { p[0] = 0; p[1] = vu; p[2] = 0; p[3] = vv; } else { p[0] = vu; p[1] = vv; }
    }
}

}  // namespace

extern "C" int sy_redact(const sy_redact_row* rows, int B, int Hmax, int Wmax, const float* boxes, int layout, int max_list,
                         const int32_t* cnt, void* stream) {
    if (rows == nullptr || boxes == nullptr || cnt == nullptr || B <= 0 || Hmax <= 0 || Wmax <= 0 || max_list <= 0 ||
        (layout != 0 && layout != 1))
        return SY_ERR_ARG;
    if (B > 65535 || (Hmax + kTileH - 1) / kTileH > 65535) return SY_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((Wmax + kTileW - 1) / kTileW), (unsigned)((Hmax + kTileH - 1) / kTileH), (unsigned)B);
    SY_LAUNCH(redact_kernel, grid, dim3(kThreads), 0, stream, rows, boxes, layout, max_list, cnt);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}
