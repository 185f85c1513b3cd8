// crop.hip — crop a tick's boxes out of camera surfaces in device memory into a dense batch of fixed-size crops.
//
// The gather that mirrors overlay.hip: what a second stage (traffic-light state, plate and sign readers, attribute classifiers,
// re-ID) needs is the detected objects as images at the camera's own resolution, without the host read that detect_device exists
// to avoid.  The rule (eight points) is stated in include/streamyolo_hip.h; this file is one way to compute it.
//
// Two launches, both with grids that do not depend on what the tables and lists hold:
//   crop_plan_kernel    ONE workgroup of 256 threads walks the batch rows in order.  Thread k resolves list entry k of the row into
//                       the integer rectangle the rule samples; the kept entries are numbered in list order with a ballot per wave
//                       and the four wave counts through LDS (overlay.hip's compaction), the row cap counts kept entries.  It writes
//                       out_index, out_rect and out_count — and these ARE the gather's plan: no workspace, no atomics.  The walk
//                       is serial over rows, so a row's descriptor, count, entry and id are loaded one row ahead.
//   crop_gather_kernel  blockIdx = (slot, tile).  A workgroup whose slot is at or past out_count[0] leaves at once.  The per-column
//                       (tap, tap, wx) triples are computed once into LDS, the tap columns already clamped into the surface with
//                       an "inside" bit each; a thread owns 8 consecutive output columns of one output row, fetches its 4 taps
//                       per pixel with byte loads from the clamped position (always a payload byte; neighbouring lanes share
//                       cache lines) and replaces what it loaded by the fill colour where the tap lies outside — no branch per tap;
//                       every YUV tap is converted before it is weighted.  Each of the three planes is written with one 8- / 16- /
//                       32-byte run per thread — the store side is where the bytes are.
#include "sy_device.h"
#include "sy_nv12.h"
#include "../../include/streamyolo_hip.h"

namespace {

using sy_nv12::nv12_bgr;
using sy_nv12::nv12_chroma;

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kCols = 8;                                         // output columns of one thread
constexpr int kMaxC = 512;                                       // Ch, Cw <= kMaxC
static_assert(kThreads == SY_CROP_MAX_BOXES, "one list entry per thread");
static_assert(sizeof(sy_crop_row) == 72, "header and kernel disagree");

// floor(c / divisor + 0.5) as an integer; false: not finite (overlay.hip's round_px: the same rule 1)
__device__ __forceinline__ bool round_px(float c, float divisor, int& out) {
    const float v = c / divisor + 0.5f;
    if (!(fabsf(c) <= 3.0e38f) || !(fabsf(v) <= 3.0e38f)) return false;       // (NaN fails both comparisons)
    const float f = fminf(fmaxf(floorf(v), -1073741824.0f), 1073741824.0f);
    out = (int)f;
    return true;
}

// a descriptor a surface can have (rule 8); uniform over a workgroup
__device__ __forceinline__ bool row_ok(const sy_crop_row& d) {
    if (d.plane0 == nullptr || d.Hs <= 0 || d.Ws <= 0) return false;
    if (d.format != SY_PIX_BGR && d.format != SY_PIX_RGB && d.format != SY_PIX_NV12 && d.format != SY_PIX_P010) return false;
    const bool yuv = d.format == SY_PIX_NV12 || d.format == SY_PIX_P010;
    if (yuv && ((d.Hs & 1) || (d.Ws & 1))) return false;
    const long long row_bytes = yuv ? ((long long)d.Ws << (d.format == SY_PIX_P010 ? 1 : 0)) : (long long)d.Ws * 3;
    if ((long long)d.row_stride < row_bytes) return false;
    const int cpitch = d.chroma_stride != 0 ? d.chroma_stride : d.row_stride;
    if (yuv && (d.chroma_stride < 0 || (long long)cpitch < row_bytes)) return false;
    return true;
}

// one list entry as the plan loads it: everything of it that lies in memory, fetched before anything is decided
struct Entry {
    float x1, y1, x2, y2, score, cls;
    int id;
};

__global__ __launch_bounds__(kThreads) void crop_plan_kernel(const sy_crop_row* rows, int B, const float* boxes, int layout, int max_list,
                                                             const int32_t* ids, const int32_t* cnt, int Ch, int Cw, int flags,
                                                             int capacity, int32_t* out_index, int32_t* out_rect, int32_t* out_count) {
    __shared__ int wave_n[2][kThreads / kWave];                  // double-buffered over the rows that get this far: one barrier per row
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const bool mine = tid < max_list;                            // entry `tid` of a row exists in memory (whatever cnt says)
    // Everything a row needs — descriptor, count, the thread's entry and its id — is loaded one row AHEAD, with addresses that
    // depend on nothing loaded: the walk costs one memory round trip per row, overlapped with the previous row's arithmetic.
    auto fetch = [&](int b, Entry& e) {
        e = Entry{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1};
        if (!mine) return;
        const float* r = boxes + ((long long)b * max_list + tid) * (layout == 0 ? 7 : 6);
        e.x1 = r[0]; e.y1 = r[1]; e.x2 = r[2]; e.y2 = r[3];
        if (layout == 0) { e.score = r[4] * r[5]; e.cls = r[6]; }
        else { e.score = r[4]; e.cls = r[5]; }
        if (ids != nullptr) e.id = ids[(long long)b * max_list + tid];
    };
    sy_crop_row d_next = rows[0];
    int cnt_next = cnt[0];
    Entry e_next;
    fetch(0, e_next);
    int total = 0, turn = 0;                                     // kept entries of the rows before b; rows compacted so far (uniform)
    for (int b = 0; b < B; ++b) {
        const sy_crop_row d = d_next;
        const Entry e = e_next;
        const int n = sy_min(sy_min(cnt_next, max_list), kThreads);
        if (b + 1 < B) {
            d_next = rows[b + 1];
            cnt_next = cnt[b + 1];
            fetch(b + 1, e_next);
        }
        if (n <= 0 || !row_ok(d)) continue;                      // (uniform)
        long long x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        int cls = 0;
        bool ok = false;
        if (tid < n) {
            int X1 = 0, Y1 = 0, X2 = 0, Y2 = 0;
            ok = e.score >= d.min_score;                         // (a NaN score is skipped)
            ok = round_px(e.x1, d.divisor, X1) && ok;
            ok = round_px(e.y1, d.divisor, Y1) && ok;
            ok = round_px(e.x2, d.divisor, X2) && ok;
            ok = round_px(e.y2, d.divisor, Y2) && ok;
            ok = ok && e.cls >= 0.0f && e.cls < 128.0f;          // (a NaN class is skipped)
            if (ok) {
                cls = (int)e.cls;
                const unsigned word = cls < 64 ? (cls < 32 ? d.class_mask[0] : d.class_mask[1]) : (cls < 96 ? d.class_mask[2] : d.class_mask[3]);
                ok = ((word >> (cls & 31)) & 1u) != 0u;
                X2 -= 1; Y2 -= 1;
                ok = ok && X2 >= X1 && Y2 >= Y1 && X2 >= 0 && X1 < d.Ws && Y2 >= 0 && Y1 < d.Hs;
            }
            if (ok) {                                            // rules 2 and 3 in 64 bits: |r(c)| <= 2^30, nothing overflows
                x1 = X1; y1 = Y1; x2 = X2; y2 = Y2;
                const long long q = sy_min(sy_max(d.pad_q8, 0), 256);
                long long W = x2 - x1 + 1, H = y2 - y1 + 1;
                const long long px = (W * q + 128) >> 8, py = (H * q + 128) >> 8;
                x1 -= px; x2 += px; y1 -= py; y2 += py;
                W += 2 * px; H += 2 * py;
                // rule 3 only grows a side, so a padded side above the limit is skipped whatever follows; what is left fits 32 bits
                // (a side <= 2^14, Ch and Cw <= 2^9): the walk over the rows is serial, and a 64-bit division here is its longest step
                ok = W <= SY_CROP_MAX_SIDE && H <= SY_CROP_MAX_SIDE;
                if (ok && (flags & SY_CROP_KEEP_ASPECT)) {
                    const unsigned w = (unsigned)W, h = (unsigned)H, ch = (unsigned)Ch, cw = (unsigned)Cw;
                    if (w * ch < h * cw) {
                        const unsigned w2 = (h * cw + ch - 1) / ch;
                        x1 -= (w2 - w) >> 1; x2 = x1 + w2 - 1;
                        ok = w2 <= SY_CROP_MAX_SIDE;
                    } else if (w * ch > h * cw) {
                        const unsigned h2 = (w * ch + cw - 1) / cw;
                        y1 -= (h2 - h) >> 1; y2 = y1 + h2 - 1;
                        ok = h2 <= SY_CROP_MAX_SIDE;
                    }
                }
            }
        }
        // number the kept entries, order kept
        const unsigned long long hits = __ballot(ok ? 1 : 0);
        int* wn = wave_n[turn++ & 1];
        if (lane == 0) wn[wave] = __popcll(hits);
        __syncthreads();
        int base = 0, m = 0;
#pragma unroll
        for (int w = 0; w < kThreads / kWave; ++w) {
            base += w < wave ? wn[w] : 0;
            m += wn[w];
        }
        const int rank = base + __popcll(hits & ((1ull << lane) - 1ull));
        if (d.max_crops > 0) m = sy_min(m, d.max_crops);
        if (ok && rank < m && total + rank < capacity) {
            const long long s = (long long)(total + rank) * 4;
            out_index[s] = b; out_index[s + 1] = tid; out_index[s + 2] = e.id; out_index[s + 3] = cls;
            out_rect[s] = (int)x1; out_rect[s + 1] = (int)y1; out_rect[s + 2] = (int)x2; out_rect[s + 3] = (int)y2;
        }
        total += m;                                              // (<= 1024 rows of <= 256)
    }
    if (tid == 0) {
        out_count[0] = sy_min(total, capacity);
        out_count[1] = total;
    }
}

// rule 4 on one axis: output index j of C over a side of W pixels -> the two clamped tap offsets and the 8-bit weight
__device__ __forceinline__ void axis_taps(int j, int W, int C, int& t0, int& t1, int& w) {
    const int n = (2 * j + 1) * W - C, d = 2 * C;                // |n| < 1025 * 16384: int32
    const int q = n >= 0 ? n / d : -((-n + d - 1) / d);          // floor
    const int f = n - q * d;
    w = (256 * f + C) / d;
    t0 = sy_min(sy_max(q, 0), W - 1);
    t1 = sy_min(sy_max(q + 1, 0), W - 1);
}

// One tap position on one axis: the coordinate clamped into the surface (what is loaded: always a payload byte) and whether the
// tap itself lies inside (else the fill colour replaces what was loaded — no branch, no address outside the payload).
constexpr int kInA = 1 << 9, kInB = 1 << 10;                     // bits of a column's weight word beside wx (0..256)

// 8 output columns of output row i for one surface kind.  YUV: NV12 / P010 (sh: 0 / 1), every tap converted before it is weighted.
template <bool YUV>
__device__ __forceinline__ void gather8(const sy_crop_row& d, const int* col_a, const int* col_b, const int* col_w, int ya, int yb,
                                        int wy, int v[3][kCols]) {
    const bool in_ya = (unsigned)ya < (unsigned)d.Hs, in_yb = (unsigned)yb < (unsigned)d.Hs;
    const int yca = sy_min(sy_max(ya, 0), d.Hs - 1), ycb = sy_min(sy_max(yb, 0), d.Hs - 1);
    const uint8_t* ra = d.plane0 + (long long)yca * d.row_stride;
    const uint8_t* rb = d.plane0 + (long long)ycb * d.row_stride;
    const int f0 = d.fill[0], f1 = d.fill[1], f2 = d.fill[2];
    const int sh = d.format == SY_PIX_P010 ? 1 : 0;
    const int c0 = d.format == SY_PIX_RGB ? 2 : 0;               // the byte of a BGR / RGB pixel that holds B
    const uint8_t* ua = nullptr;
    const uint8_t* ub = nullptr;
    if (YUV) {
        const uint8_t* uv = d.plane1 != nullptr ? d.plane1 : d.plane0 + (long long)d.row_stride * d.Hs;
        const int cpitch = d.chroma_stride != 0 ? d.chroma_stride : d.row_stride;
        ua = uv + (long long)(yca >> 1) * cpitch;
        ub = uv + (long long)(ycb >> 1) * cpitch;
    }
    // (B, G, R) of the pixel in column x of the row at r (chroma row at u), or the fill colour
    auto tap = [&](const uint8_t* r, const uint8_t* u, int x, bool inside, int o[3]) {
        if (YUV) {                                               // input_pipeline.hip's nv12_px; P010: the high bytes
            const int at = ((x & ~1) << sh) + sh;
            nv12_bgr((int)r[(x << sh) + sh], nv12_chroma((int)u[at], (int)u[at + (1 << sh)]), o);
        } else {
            const uint8_t* p = r + x * 3;
            o[0] = (int)p[c0]; o[1] = (int)p[1]; o[2] = (int)p[2 - c0];
        }
        o[0] = inside ? o[0] : f0; o[1] = inside ? o[1] : f1; o[2] = inside ? o[2] : f2;
    };
#pragma unroll
    for (int k = 0; k < kCols; ++k) {
        const int xa = col_a[k], xb = col_b[k], ww = col_w[k], wx = ww & 511;
        const bool in_xa = (ww & kInA) != 0, in_xb = (ww & kInB) != 0;
        int p00[3], p01[3], p10[3], p11[3];
        tap(ra, ua, xa, in_xa && in_ya, p00); tap(ra, ua, xb, in_xb && in_ya, p01);
        tap(rb, ub, xa, in_xa && in_yb, p10); tap(rb, ub, xb, in_xb && in_yb, p11);
        const int w00 = (256 - wx) * (256 - wy), w01 = wx * (256 - wy), w10 = (256 - wx) * wy, w11 = wx * wy;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][k] = (w00 * p00[c] + w01 * p01[c] + w10 * p10[c] + w11 * p11[c] + 32768) >> 16;
    }
}

template <int DT>
__global__ __launch_bounds__(kThreads) void crop_gather_kernel(const sy_crop_row* rows, int Ch, int Cw, int flags, const float* mean3,
                                                               const float* scale3, void* out, const int32_t* out_index,
                                                               const int32_t* out_rect, const int32_t* out_count) {
    __shared__ int col_a[kMaxC], col_b[kMaxC], col_w[kMaxC];     // per output column: two clamped tap columns, wx | inside bits
    const int slot = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (slot >= out_count[0]) return;                            // (uniform) nothing of this slot is written
    const int G = Cw / kCols;                                    // column groups of a row
    const int item = (int)blockIdx.y * kThreads + tid;           // (output row, column group)
    const sy_crop_row d = rows[out_index[(long long)slot * 4]];
    const int X1 = out_rect[(long long)slot * 4], Y1 = out_rect[(long long)slot * 4 + 1];
    const int W = out_rect[(long long)slot * 4 + 2] - X1 + 1, H = out_rect[(long long)slot * 4 + 3] - Y1 + 1;
    for (int j = tid; j < Cw; j += kThreads) {
        int t0, t1, w;
        axis_taps(j, W, Cw, t0, t1, w);
        const int xa = X1 + t0, xb = X1 + t1;
        col_a[j] = sy_min(sy_max(xa, 0), d.Ws - 1);
        col_b[j] = sy_min(sy_max(xb, 0), d.Ws - 1);
        col_w[j] = w | ((unsigned)xa < (unsigned)d.Ws ? kInA : 0) | ((unsigned)xb < (unsigned)d.Ws ? kInB : 0);
    }
    __syncthreads();
    if (item >= Ch * G) return;
    const int i = item / G, j0 = (item - i * G) * kCols;

    int ty0, ty1, wy;
    axis_taps(i, H, Ch, ty0, ty1, wy);
    int v[3][kCols];
    if (d.format == SY_PIX_NV12 || d.format == SY_PIX_P010) gather8<true>(d, col_a + j0, col_b + j0, col_w + j0, Y1 + ty0, Y1 + ty1, wy, v);
    else gather8<false>(d, col_a + j0, col_b + j0, col_w + j0, Y1 + ty0, Y1 + ty1, wy, v);

    // rule 6: plane c of the output is channel c of (B, G, R), or of (R, G, B)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int* vc = v[(flags & SY_CROP_RGB_OUT) ? 2 - c : c];
        const long long at = (((long long)slot * 3 + c) * Ch + i) * Cw + j0;       // a multiple of 8 elements
        if (DT == SY_CROP_DT_U8) {
            uint2 o;
            o.x = (unsigned)vc[0] | ((unsigned)vc[1] << 8) | ((unsigned)vc[2] << 16) | ((unsigned)vc[3] << 24);
            o.y = (unsigned)vc[4] | ((unsigned)vc[5] << 8) | ((unsigned)vc[6] << 16) | ((unsigned)vc[7] << 24);
            *reinterpret_cast<uint2*>(static_cast<uint8_t*>(out) + at) = o;
            continue;
        }
        const float mean = mean3 != nullptr ? mean3[c] : 0.0f, scale = scale3 != nullptr ? scale3[c] : 1.0f;
        float f[kCols];
#pragma unroll
        for (int k = 0; k < kCols; ++k) f[k] = ((float)vc[k] - mean) * scale;
        if (DT == SY_DT_F32) {
            float4* o = reinterpret_cast<float4*>(static_cast<float*>(out) + at);
            o[0] = make_float4(f[0], f[1], f[2], f[3]);
            o[1] = make_float4(f[4], f[5], f[6], f[7]);
        } else if (DT == SY_DT_F16) {
            *reinterpret_cast<uint4*>(static_cast<unsigned short*>(out) + at) =
                make_uint4(F16::pack2(f[0], f[1]), F16::pack2(f[2], f[3]), F16::pack2(f[4], f[5]), F16::pack2(f[6], f[7]));
        } else {
            *reinterpret_cast<uint4*>(static_cast<unsigned short*>(out) + at) =
                make_uint4(BF16::pack2(f[0], f[1]), BF16::pack2(f[2], f[3]), BF16::pack2(f[4], f[5]), BF16::pack2(f[6], f[7]));
        }
    }
}

}  // namespace

extern "C" int sy_crop_gather(const sy_crop_row* rows, int B, const float* boxes, int layout, int max_list, const int32_t* ids,
                              const int32_t* cnt, int Ch, int Cw, int flags, int out_dtype, const float* mean3, const float* scale3,
                              void* out, int capacity, int32_t* out_index, int32_t* out_rect, int32_t* out_count, void* stream) {
    if (rows == nullptr || boxes == nullptr || cnt == nullptr || out == nullptr || out_index == nullptr || out_rect == nullptr ||
        out_count == nullptr || B <= 0 || max_list <= 0 || capacity <= 0 || (layout != 0 && layout != 1) ||
        (flags & ~(SY_CROP_KEEP_ASPECT | SY_CROP_RGB_OUT)) != 0 ||
        (out_dtype != SY_DT_BF16 && out_dtype != SY_DT_F16 && out_dtype != SY_DT_F32 && out_dtype != SY_CROP_DT_U8))
        return SY_ERR_ARG;
    if (Cw % kCols != 0 || Ch < 8 || Ch > kMaxC || Cw < 8 || Cw > kMaxC || B > 1024) return SY_ERR_UNSUPPORTED;
    SY_LAUNCH(crop_plan_kernel, dim3(1), dim3(kThreads), 0, stream, rows, B, boxes, layout, max_list, ids, cnt, Ch, Cw, flags, capacity,
              out_index, out_rect, out_count);
    if (SY_LAUNCH_OK() != 0) return SY_ERR_LAUNCH;
    const dim3 grid((unsigned)capacity, (unsigned)((Ch * (Cw / kCols) + kThreads - 1) / kThreads));
    switch (out_dtype) {
    case SY_DT_BF16:
        SY_LAUNCH(crop_gather_kernel<SY_DT_BF16>, grid, dim3(kThreads), 0, stream, rows, Ch, Cw, flags, mean3, scale3, out,
                  (const int32_t*)out_index, (const int32_t*)out_rect, (const int32_t*)out_count);
        break;
    case SY_DT_F16:
        SY_LAUNCH(crop_gather_kernel<SY_DT_F16>, grid, dim3(kThreads), 0, stream, rows, Ch, Cw, flags, mean3, scale3, out,
                  (const int32_t*)out_index, (const int32_t*)out_rect, (const int32_t*)out_count);
        break;
    case SY_DT_F32:
        SY_LAUNCH(crop_gather_kernel<SY_DT_F32>, grid, dim3(kThreads), 0, stream, rows, Ch, Cw, flags, mean3, scale3, out,
                  (const int32_t*)out_index, (const int32_t*)out_rect, (const int32_t*)out_count);
        break;
    default:
        SY_LAUNCH(crop_gather_kernel<SY_CROP_DT_U8>, grid, dim3(kThreads), 0, stream, rows, Ch, Cw, flags, mean3, scale3, out,
                  (const int32_t*)out_index, (const int32_t*)out_rect, (const int32_t*)out_count);
        break;
    }
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}
