// score.hip — COCO-style detection scoring (AP / AR, the sAP numbers) on the device.
//
// Replaces pycocotools' COCOeval for boxes, as the reference calls it in sAP/det/__init__.py::eval_ccf (:180-195) and in
// exps/evaluators/onex_stream_evaluator.py (:252-262): computeIoU + evaluateImg per (image, class), then accumulate.
//   score_reset_kernel        clears the counters of a scorer state
//   score_match_kernel        one batch of images: blockIdx = (batch row, class), ONE wave; ranks the class's detections, orders
//                             its ground truths per area range, runs COCOeval's greedy walk with lane = (area range, threshold)
//                             and appends one record per kept detection to the class's arena
//   score_accumulate_kernel   blockIdx = class: sorts the class's records by (score descending, image, rank) in the caller's
//                             workspace and walks them once per (area range, maxDet, threshold) = thread
// Every IoU, precision and recall operation is an IEEE double operation in COCOeval's order (the library is built with
// -ffp-contract=off and HIP's correctly rounded division), on thresholds the host computed with numpy: the outputs equal a
// float64 numpy restatement to the last bit.  Counters are integers moved by integer atomics and a record's place in the arena
// carries no meaning (its sequence number does), so the result does not depend on the order the workgroups ran in.
//
// State (one device allocation of sy_score_state_bytes): int32 used[C], int32 npig[C][4], int32 overflow, padding to 32 bytes,
// then C arenas of `capacity` records of 32 bytes.
#include "sy_device.h"
#include "../../include/streamyolo_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxDet = SY_SCORE_MAX_DET;                        // detections kept per (image, class): COCOeval's maxDets[-1]
constexpr int kMaxGt = SY_SCORE_MAX_GT;
constexpr int kMaxThr = SY_SCORE_MAX_THR;
constexpr int kMaxArea = SY_SCORE_MAX_AREA;
constexpr int kSortN = 256;                                      // the ranking buffer: the best 128 so far + 128 newcomers
constexpr int kAccThreads = 256;                                 // >= kMaxArea * SY_SCORE_MAX_MAXDET * kMaxThr
static_assert(kMaxArea * kMaxThr <= kWave, "one lane per (area range, threshold)");
static_assert(kMaxArea * SY_SCORE_MAX_MAXDET * kMaxThr <= kAccThreads, "one thread per (area range, maxDet, threshold)");
static_assert(kMaxDet <= 128 && kMaxGt % kWave == 0, "buffer sizes");

struct Record {                                                  // 32 bytes
    unsigned score_bits;                                         // the float32 score (>= 0)
    unsigned seq;                                                // image * 128 + rank
    unsigned long long matched;                                  // bit a * n_thr + t
    unsigned long long ignored;
    int rank;                                                    // 0-based place among the image's detections of the class
    int reserved;
};
static_assert(sizeof(Record) == 32, "record layout");

struct StateView {
    int32_t* used;                                               // [C]
    int32_t* npig;                                               // [C][4]
    int32_t* overflow;
    Record* rec;                                                 // [C][cap]
    int C, cap;
};

inline long long header_bytes(int C) { return (((long long)C * 5 + 1) * 4 + 31) / 32 * 32; }

inline StateView view_of(void* state, int C, int cap) {
    StateView v;
    v.used = (int32_t*)state;
    v.npig = v.used + C;
    v.overflow = v.used + 5 * C;
    v.rec = (Record*)((unsigned char*)state + header_bytes(C));
    v.C = C; v.cap = cap;
    return v;
}

struct MatchParams {                                             // what the match launch needs of sy_score_params, by value
    int n_thr, n_area;
    double thr[kMaxThr];
    double lo[kMaxArea], hi[kMaxArea];
};

struct AccParams {
    int n_thr, n_rec, n_area, n_maxdet;
    int maxdet[SY_SCORE_MAX_MAXDET];
    double eps;
    double rec[SY_SCORE_MAX_REC];
};

struct MatchLds {
    unsigned long long keys[kSortN];
    double dx[kMaxDet], dy[kMaxDet], dw[kMaxDet], dh[kMaxDet];
    float dscore[kMaxDet];
    double gx[kMaxGt], gy[kMaxGt], gw[kMaxGt], gh[kMaxGt], garea[kMaxGt];
    unsigned char gcrowd[kMaxGt];
    unsigned short order[kMaxArea][kMaxGt];                      // ground truths of an area range: non-ignored first, input order kept
    unsigned long long gtm[kMaxGt / 64][kWave];                  // per lane: the ground truths taken at its (area range, threshold)
};

__global__ void score_reset_kernel(int32_t* hdr, int n) {
    for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) hdr[i] = 0;
}

// ascending bitonic sort of the kSortN keys in LDS by one wave (wave-private LDS: a fence per pass)
__device__ __forceinline__ void sort_keys(unsigned long long* keys, int lane) {
    for (int k = 2; k <= kSortN; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < kSortN; i += kWave) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = keys[i], b = keys[ixj];
                    const bool up = ((i & k) == 0);
                    if ((a > b) == up) { keys[i] = b; keys[ixj] = a; }
                }
            }
            sy_wave_fence();
        }
    }
}

__global__ __launch_bounds__(kWave) void score_match_kernel(const float* det, const int32_t* cnt, int max_det, int layout,
                                                            const float* divisor, const double* gt, const int32_t* gt_cnt, int max_gt,
                                                            long long image_base, MatchParams prm, StateView st) {
    __shared__ MatchLds sm;
    const int b = (int)blockIdx.x, k = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int cols = layout == SY_SCORE_LAYOUT_NMS ? 7 : 6;
    const int n_all = sy_min(sy_max(cnt[b], 0), max_det), g_all = sy_min(sy_max(gt_cnt[b], 0), max_gt);
    const float* D = det + (long long)b * max_det * cols;
    const double* G = gt + (long long)b * max_gt * 7;

    // ---- 1. rank: the class's detections by score descending, ties by input row (key = ~score_bits << 32 | row), best 100.
    // keys[0..128) hold the best so far in ascending key order, newcomers are staged in keys[128..256) and sorted in ----
    for (int i = lane; i < kSortN; i += kWave) sm.keys[i] = ~0ull;
    sy_wave_fence();
    int staged = 0;
    for (int j0 = 0; j0 < n_all; j0 += kWave) {
        if (staged > kSortN / 2 - kWave) {
            sort_keys(sm.keys, lane);
            for (int i = kSortN / 2 + lane; i < kSortN; i += kWave) sm.keys[i] = ~0ull;
            sy_wave_fence();
            staged = 0;
        }
        const int j = j0 + lane;
        bool mine = false;
        unsigned long long key = ~0ull;
        if (j < n_all) {
            const float* r = D + (long long)j * cols;
            const float s = layout == SY_SCORE_LAYOUT_NMS ? r[4] * r[5] : r[4];
            mine = (int)r[cols - 1] == k;
            key = ((unsigned long long)(~__builtin_bit_cast(unsigned, s)) << 32) | (unsigned)j;
        }
        const unsigned long long who = __ballot(mine ? 1 : 0);
        if (mine) sm.keys[kSortN / 2 + staged + __popcll(who & ((1ull << lane) - 1ull))] = key;
        staged += __popcll(who);
        sy_wave_fence();
    }
    if (staged > 0) sort_keys(sm.keys, lane);
    int nd = 0;
    for (int i = lane; i < kSortN / 2; i += kWave) nd += __popcll(__ballot(sm.keys[i] != ~0ull ? 1 : 0));
    nd = sy_min(nd, kMaxDet);

    // ---- 2. the class's ground truths in input order ----
    int ng = 0;
    for (int g0 = 0; g0 < g_all; g0 += kWave) {
        const int g = g0 + lane;
        const double* r = G + (long long)sy_min(g, g_all - 1) * 7;
        const bool mine = g < g_all && (int)r[4] == k;
        const unsigned long long who = __ballot(mine ? 1 : 0);
        if (mine) {
            const int o = ng + __popcll(who & ((1ull << lane) - 1ull));
            sm.gx[o] = r[0]; sm.gy[o] = r[1]; sm.gw[o] = r[2]; sm.gh[o] = r[3];
            sm.gcrowd[o] = r[5] != 0.0 ? 1 : 0;
            sm.garea[o] = r[6];
        }
        ng += __popcll(who);
    }
    if (nd == 0 && ng == 0) return;                              // (uniform) the image does not exist for this class
    sy_wave_fence();

    // ---- 3. the detections: divide in float32, w = x2 - x1 and h = y2 - y1 in float32 (the xywh layout brings them), then double ----
    const float div = divisor != nullptr ? divisor[b] : 1.0f;
    for (int d = lane; d < nd; d += kWave) {
        const int j = (int)(sm.keys[d] & 0xffffffffull);
        const float* r = D + (long long)j * cols;
        float x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
        if (divisor != nullptr) { x1 = x1 / div; y1 = y1 / div; x2 = x2 / div; y2 = y2 / div; }
        const float w = layout == SY_SCORE_LAYOUT_XYWH ? x2 : x2 - x1, h = layout == SY_SCORE_LAYOUT_XYWH ? y2 : y2 - y1;
        sm.dx[d] = (double)x1; sm.dy[d] = (double)y1; sm.dw[d] = (double)w; sm.dh[d] = (double)h;
        sm.dscore[d] = layout == SY_SCORE_LAYOUT_NMS ? r[4] * r[5] : r[4];
    }

    // ---- 4. ground-truth order per area range: non-ignored first, each group in input order ----
    int nnon_of[kMaxArea];
#pragma unroll
    for (int a = 0; a < kMaxArea; ++a) {
        nnon_of[a] = 0;
        if (a < prm.n_area) {
            const double lo = prm.lo[a], hi = prm.hi[a];
            int nn = 0;
            for (int g0 = 0; g0 < ng; g0 += kWave) {
                const int g = g0 + lane;
                const bool keep = g < ng && !(sm.gcrowd[g] != 0 || sm.garea[g] < lo || sm.garea[g] > hi);
                const unsigned long long who = __ballot(keep ? 1 : 0);
                if (keep) sm.order[a][nn + __popcll(who & ((1ull << lane) - 1ull))] = (unsigned short)g;
                nn += __popcll(who);
            }
            int ni = nn;
            for (int g0 = 0; g0 < ng; g0 += kWave) {
                const int g = g0 + lane;
                const bool ign = g < ng && (sm.gcrowd[g] != 0 || sm.garea[g] < lo || sm.garea[g] > hi);
                const unsigned long long who = __ballot(ign ? 1 : 0);
                if (ign) sm.order[a][ni + __popcll(who & ((1ull << lane) - 1ull))] = (unsigned short)g;
                ni += __popcll(who);
            }
            nnon_of[a] = nn;
        }
    }
#pragma unroll
    for (int w = 0; w < kMaxGt / 64; ++w) sm.gtm[w][lane] = 0ull;
    sy_wave_fence();

    // ---- 5. the walk: lane = a * n_thr + t runs evaluateImg's loops for its area range and threshold ----
    const int n_lanes = prm.n_area * prm.n_thr;
    const bool active = lane < n_lanes;
    const int a = active ? lane / prm.n_thr : 0, t = active ? lane % prm.n_thr : 0;
    int nnon = 0;
#pragma unroll
    for (int q = 0; q < kMaxArea; ++q) if (q == a) nnon = nnon_of[q];
    const double thr = prm.thr[t], lo = prm.lo[a], hi = prm.hi[a];
    const double cap1 = 1.0 - 1e-10;
    const double best0 = thr < cap1 ? thr : cap1;
    unsigned long long my_m[2] = {0ull, 0ull}, my_i[2] = {0ull, 0ull};   // lane d & 63 keeps the bit sets of detection d
    for (int d = 0; d < nd; ++d) {
        bool mt = false, ig = false;
        if (active) {
            const double x = sm.dx[d], y = sm.dy[d], w = sm.dw[d], h = sm.dh[d];
            const double da = w * h;
            double best = best0;
            int m = -1;
            bool m_ign = false;
            for (int gi = 0; gi < ng; ++gi) {
                const int g = sm.order[a][gi];
                const bool g_ign = gi >= nnon, crowd = sm.gcrowd[g] != 0;
                if (((sm.gtm[g >> 6][lane] >> (g & 63)) & 1ull) != 0ull && !crowd) continue;
                if (m >= 0 && !m_ign && g_ign) break;
                const double gx = sm.gx[g], gy = sm.gy[g], gw = sm.gw[g], gh = sm.gh[g];
                const double xr = x + w, gxr = gx + gw, yb = y + h, gyb = gy + gh;
                double iw = (xr < gxr ? xr : gxr) - (x > gx ? x : gx);
                double ih = (yb < gyb ? yb : gyb) - (y > gy ? y : gy);
                if (iw <= 0.0) iw = 0.0;
                if (ih <= 0.0) ih = 0.0;
                const double inter = iw * ih;
                const double uni = crowd ? da : (da + gw * gh) - inter;
                const double iou = inter / uni;
                if (iou < best) continue;
                best = iou;
                m = g;
                m_ign = g_ign;
            }
            if (m >= 0) {
                mt = true;
                ig = m_ign;
                sm.gtm[m >> 6][lane] |= 1ull << (m & 63);
            } else {
                ig = da < lo || da > hi;
            }
        }
        const unsigned long long mm = __ballot(mt ? 1 : 0), im = __ballot(ig ? 1 : 0);
        if (lane == (d & 63)) { my_m[d >> 6] = mm; my_i[d >> 6] = im; }
    }

    // ---- 6. out: non-ignored ground-truth counts, then the records ----
    if (lane < prm.n_area) {
        int nn = 0;
#pragma unroll
        for (int q = 0; q < kMaxArea; ++q) if (q == lane) nn = nnon_of[q];
        if (nn > 0) atomicAdd(&st.npig[k * 4 + lane], nn);
    }
    int base = 0;
    if (lane == 0 && nd > 0) base = atomicAdd(&st.used[k], nd);
    base = __shfl(base, 0);
    int fit = nd;
    if (base < 0 || base >= st.cap) fit = 0;                     // (a counter that ran over stays over: nothing more is written)
    else if (st.cap - base < nd) fit = st.cap - base;
    if (lane == 0 && fit < nd) atomicAdd(st.overflow, nd - fit);
    Record* arena = st.rec + (long long)k * st.cap;
    const unsigned image = (unsigned)(image_base + b);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int d = c * kWave + lane;
        if (d < fit) {
            Record r;
            r.score_bits = __builtin_bit_cast(unsigned, sm.dscore[d]);
            r.seq = image * 128u + (unsigned)d;
            r.matched = my_m[c];
            r.ignored = my_i[c];
            r.rank = d;
            r.reserved = 0;
            arena[base + d] = r;
        }
    }
}

// One workgroup per class.  ws: [C][n2cap] pairs (key, record index), n2cap = the capacity rounded up to a power of two.
__global__ __launch_bounds__(kAccThreads) void score_accumulate_kernel(StateView st, AccParams prm, unsigned long long* ws,
                                                                       long long n2cap, double* precision, double* recall,
                                                                       double* overflow) {
    const int k = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (k == 0 && tid == 0 && overflow != nullptr) *overflow = (double)*st.overflow;   // rides in the caller's one copy of the results
    const int n = sy_min(sy_max(st.used[k], 0), st.cap);
    const Record* arena = st.rec + (long long)k * st.cap;
    unsigned long long* pairs = ws + (long long)k * n2cap * 2;
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    for (int i = tid; i < n2; i += kAccThreads) {
        unsigned long long key = ~0ull;
        if (i < n) key = ((unsigned long long)(~arena[i].score_bits) << 32) | arena[i].seq;
        pairs[2 * (long long)i] = key;
        pairs[2 * (long long)i + 1] = (unsigned long long)i;
    }
    __syncthreads();
    // bitonic network over global memory (once per evaluation); ascending keys = COCOeval's argsort(-scores, 'mergesort') over
    // the image-major concatenation
    for (int kk = 2; kk <= n2; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += kAccThreads) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long ka = pairs[2 * (long long)i], kb = pairs[2 * (long long)ixj];
                    const bool up = ((i & kk) == 0);
                    if ((ka > kb) == up) {
                        const unsigned long long pa = pairs[2 * (long long)i + 1], pb = pairs[2 * (long long)ixj + 1];
                        pairs[2 * (long long)i] = kb; pairs[2 * (long long)i + 1] = pb;
                        pairs[2 * (long long)ixj] = ka; pairs[2 * (long long)ixj + 1] = pa;
                    }
                }
            }
            __syncthreads();
        }
    }

    const int T = prm.n_thr, R = prm.n_rec, A = prm.n_area, M = prm.n_maxdet, K = st.C;
    if (tid >= A * M * T) return;
    const int a = tid / (M * T), m = (tid / T) % M, t = tid % T;
    const int maxdet = prm.maxdet[m], bit = a * T + t;
    const int npig = st.npig[k * 4 + a];
    // precision [T, R, K, A, M], recall [T, K, A, M]
    double* P = precision + ((((long long)t * R) * K + k) * A + a) * M + m;
    const long long pstep = (long long)K * A * M;
    double* Rc = recall + (((long long)t * K + k) * A + a) * M + m;
    if (npig == 0) {
        for (int r = 0; r < R; ++r) P[r * pstep] = -1.0;
        *Rc = -1.0;
        return;
    }
    // forward: the totals over the records with rank < maxDet
    int nd = 0, tp = 0, fp = 0;
    for (int i = 0; i < n; ++i) {
        const Record& r = arena[pairs[2 * (long long)i + 1]];
        if (r.rank >= maxdet) continue;
        ++nd;
        if ((r.ignored >> bit) & 1ull) continue;
        if ((r.matched >> bit) & 1ull) ++tp; else ++fp;
    }
    const double dn = (double)npig;
    const double rc_last = (double)tp / dn;
    *Rc = nd > 0 ? rc_last : 0.0;
    // p = the recall thresholds reached at all (searchsorted 'left': the first i with rc[i] >= threshold); the others read 0
    int p = 0;
    if (nd > 0) while (p < R && prm.rec[p] <= rc_last) ++p;
    for (int r = p; r < R; ++r) P[r * pstep] = 0.0;
    // backward: env = pr made non-increasing from the back; a threshold is settled where rc drops below it.  Ignored records repeat
    // their neighbour's (tp, fp) — before the first counted record that is (0, 0), pr = 0 — so they never move env.
    double env = 0.0;
    for (int i = n - 1; i >= 0 && p > 0; --i) {
        const Record& r = arena[pairs[2 * (long long)i + 1]];
        if (r.rank >= maxdet || ((r.ignored >> bit) & 1ull)) continue;
        const double pr = (double)tp / (((double)fp + (double)tp) + prm.eps);
        if (pr > env) env = pr;
        if ((r.matched >> bit) & 1ull) {
            --tp;
            const double rc_before = (double)tp / dn;
            while (p > 0 && prm.rec[p - 1] > rc_before) { P[(p - 1) * pstep] = env; --p; }
        } else {
            --fp;
        }
    }
    while (p > 0) { P[(p - 1) * pstep] = env; --p; }
}

inline bool params_ok(const sy_score_params* p) {
    if (p == nullptr || p->n_thr < 1 || p->n_thr > kMaxThr || p->n_area < 1 || p->n_area > kMaxArea || p->n_rec < 1 ||
        p->n_rec > SY_SCORE_MAX_REC || p->n_maxdet < 1 || p->n_maxdet > SY_SCORE_MAX_MAXDET)
        return false;
    for (int i = 0; i < p->n_maxdet; ++i)
        if (p->maxdet[i] < 1 || p->maxdet[i] > kMaxDet) return false;
    for (int i = 1; i < p->n_rec; ++i)
        if (!(p->rec_thr[i] >= p->rec_thr[i - 1])) return false;  // (the accumulate walk relies on ascending recall thresholds)
    return true;
}

inline bool sizes_ok(int C, int cap) { return C >= 1 && C <= 65535 && cap >= 1 && cap <= (1 << 30) / C; }

inline long long pow2_at_least(long long v) { long long p = 1; while (p < v) p <<= 1; return p; }

}  // namespace

extern "C" int64_t sy_score_state_bytes(int num_classes, int capacity) {
    if (!sizes_ok(num_classes, capacity)) return -1;
    return header_bytes(num_classes) + (int64_t)num_classes * capacity * (int64_t)sizeof(Record);
}

extern "C" int64_t sy_score_workspace_bytes(int num_classes, int capacity) {
    if (!sizes_ok(num_classes, capacity)) return -1;
    return (int64_t)num_classes * pow2_at_least(capacity) * 16;
}

extern "C" int sy_score_reset(void* state, int num_classes, int capacity, void* stream) {
    if (state == nullptr || !sizes_ok(num_classes, capacity)) return SY_ERR_ARG;
    SY_LAUNCH(score_reset_kernel, dim3(1), dim3(kWave), 0, stream, (int32_t*)state, (int)(header_bytes(num_classes) / 4));
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}

extern "C" int sy_score_match(const float* det, const int32_t* cnt, int B, int max_det, int layout, const float* divisor,
                              const double* gt, const int32_t* gt_cnt, int max_gt, int64_t image_base,
                              const sy_score_params* params, void* state, int num_classes, int capacity, void* stream) {
    if (det == nullptr || cnt == nullptr || gt == nullptr || gt_cnt == nullptr || state == nullptr || B < 0 || B > 65535 ||
        max_det < 1 || max_gt < 1 || max_gt > kMaxGt || (layout != SY_SCORE_LAYOUT_NMS && layout != SY_SCORE_LAYOUT_TRACK && layout != SY_SCORE_LAYOUT_XYWH) ||
        image_base < 0 || image_base + B > (1ll << 25) || !params_ok(params) || !sizes_ok(num_classes, capacity))
        return SY_ERR_ARG;
    if (B == 0) return SY_OK;
    MatchParams p;
    p.n_thr = params->n_thr; p.n_area = params->n_area;
    for (int i = 0; i < kMaxThr; ++i) p.thr[i] = i < p.n_thr ? params->iou_thr[i] : 0.0;
    for (int i = 0; i < kMaxArea; ++i) { p.lo[i] = i < p.n_area ? params->area_lo[i] : 0.0; p.hi[i] = i < p.n_area ? params->area_hi[i] : 0.0; }
    SY_LAUNCH(score_match_kernel, dim3(B, num_classes), dim3(kWave), 0, stream, det, cnt, max_det, layout, divisor, gt, gt_cnt, max_gt,
              (long long)image_base, p, view_of(state, num_classes, capacity));
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}

extern "C" int sy_score_accumulate(const void* state, int num_classes, int capacity, const sy_score_params* params, void* workspace,
                                   double* precision, double* recall, double* overflow, void* stream) {
    if (state == nullptr || workspace == nullptr || precision == nullptr || recall == nullptr || !params_ok(params) ||
        !sizes_ok(num_classes, capacity))
        return SY_ERR_ARG;
    AccParams p;
    p.n_thr = params->n_thr; p.n_rec = params->n_rec; p.n_area = params->n_area; p.n_maxdet = params->n_maxdet;
    for (int i = 0; i < SY_SCORE_MAX_MAXDET; ++i) p.maxdet[i] = i < p.n_maxdet ? params->maxdet[i] : 0;
    p.eps = params->eps;
    for (int i = 0; i < SY_SCORE_MAX_REC; ++i) p.rec[i] = i < p.n_rec ? params->rec_thr[i] : 0.0;
    SY_LAUNCH(score_accumulate_kernel, dim3(num_classes), dim3(kAccThreads), 0, stream, view_of(const_cast<void*>(state), num_classes, capacity),
              p, (unsigned long long*)workspace, (long long)pow2_at_least(capacity), precision, recall, overflow);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}
