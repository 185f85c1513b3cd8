// track.hip — per-stream tracking and forecasting behind the NMS of a batched streaming tick.
//
// Replaces (per batch row) the reference's streaming post-processing step, which runs on the CPU per sequence:
// sAP/forecast/pps_forecast_kf.py (--forecast-before-assoc: batched Kalman filter, :73-97, :170-273),
// sAP/track/__init__.py::iou_assoc (:90-134, greedy IoU association) and sAP/forecast/__init__.py::extrap_clean_up (:33-56).
// Boxes are ltwh in camera coordinates, the state of a track is x = (l, t, w, h, vl, vt, vw, vh) with its 8 x 8 covariance.
//   track_update_kernel     one tick: reset / predict / associate / rebuild / store / forecast, blockIdx.x = the batch row
//   track_forecast_kernel   the forecast step alone for a table of (slot, horizon, image size); the state is only read
// Which row belongs to which stream, and everything else that changes from tick to tick, is read through device pointers (the
// mechanism of stream_state.hip: a launch tape replays argument VALUES).
//
// Kernel shape: ONE wave per batch row, lane i owns tracks i, i + 64, i + 128, i + 192 (and detections likewise).  The
// association is serial over the detections (detection j may only take what detections 0..j-1 left), so the latency of one
// step is what counts: with one wave a step is a readlane broadcast of the detection, up to four IoUs per lane, a wave maximum
// on the VALU (DPP) and a ballot — no workgroup barrier and no LDS round trip, which a 256-lane workgroup would pay twice
// per detection for its cross-wave reduction.  The covariances are only needed before the loop (predict) and after it
// (update): they wait in LDS meanwhile, the loop itself keeps four boxes per lane in registers.
//
// Differences from the reference, on purpose: at most max_tracks detections per row are used (the pools are fixed-size; the
// detections arrive in descending score, so the weakest are the ones dropped); fresh ids are next_id++ in detection order
// (the reference advances its counter twice when nothing matches); P is kept as its upper triangle (the reference's
// P -= K P[:4] is symmetric up to rounding only).
#include "sy_device.h"
#include "../../include/streamyolo_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kPerLane = 4;
constexpr int kMaxT = kWave * kPerLane;
constexpr int kNP = 36;                                          // entries of the upper triangle of an 8 x 8 matrix
static_assert(kMaxT == SY_TRACK_MAX_TRACKS, "header and kernel disagree");

struct TrackLds {                                                // 49152 bytes
    float P[kNP][kMaxT];                                         // predicted covariances, by OLD track index
    float x[8][kMaxT];                                           // predicted states by old index; behind the rebuild: the new states
    float d[3][kMaxT];                                           // score, label, id of the tracks the forecast writes, by track index
    int oid[kMaxT];                                              // ids of the old tracks
};

// index of (i, j), i <= j, in the row-major upper triangle
__device__ __forceinline__ constexpr int tri(int i, int j) { return i * 8 - i * (i - 1) / 2 + (j - i); }

struct Pools {
    float* x;
    float* P;
    float* score;
    int32_t* label;
    int32_t* id;
    int32_t* hdr;
    int n_slots, T;
};

__device__ __forceinline__ float as_f(int v) { return __builtin_bit_cast(float, v); }
__device__ __forceinline__ int as_i(float v) { return __builtin_bit_cast(int, v); }

// Step 7: the tracks of sm (x by track index, d rows 0..2 = score, label, id) moved to `horizon`, cleaned up as
// extrap_clean_up(..., lt=True) does and written compacted in track order.  All 64 lanes call it.
__device__ __forceinline__ void forecast_and_write(const TrackLds& sm, int n, int n_matched, float horizon, float img_w, float img_h,
                                                   int min_size, int T, float* out, int32_t* out_id, int32_t* out_cnt, int lane) {
    int base = 0;
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
        const int k = c * kWave + lane;
        bool keep = false;
        float l = 0.0f, t = 0.0f, r = 0.0f, b = 0.0f;
        if (k < n) {
            l = sm.x[0][k]; t = sm.x[1][k];
            float w = sm.x[2][k], h = sm.x[3][k];
            if (k < n_matched) {
                l = l + horizon * sm.x[4][k]; t = t + horizon * sm.x[5][k];
                w = w + horizon * sm.x[6][k]; h = h + horizon * sm.x[7][k];
            }
            keep = w > 0.0f && h > 0.0f;
            r = l + w; b = t + h;
            l = fminf(fmaxf(l, 0.0f), img_w); r = fminf(fmaxf(r, 0.0f), img_w);
            t = fminf(fmaxf(t, 0.0f), img_h); b = fminf(fmaxf(b, 0.0f), img_h);
            // (keep first: a NaN box never reaches the conversions)
            keep = keep && (int)(r - l) * (int)(b - t) >= min_size;
        }
        const unsigned long long kept = __ballot(keep ? 1 : 0);
        if (keep) {
            const int o = base + __popcll(kept & ((1ull << lane) - 1ull));
            float* row = out + (long long)o * 6;
            row[0] = l; row[1] = t; row[2] = r; row[3] = b; row[4] = sm.d[0][k]; row[5] = (float)as_i(sm.d[1][k]);
            out_id[o] = as_i(sm.d[2][k]);
        }
        base += __popcll(kept);
    }
    (void)T;
    if (lane == 0) *out_cnt = base;
}

__global__ __launch_bounds__(kWave) void track_update_kernel(const float* det, const int32_t* cnt, int max_det, const int32_t* row_slot,
                                                             const uint8_t* row_first, const sy_track_tick* ticks, Pools st,
                                                             sy_track_params prm, float* out, int32_t* out_id, int32_t* out_cnt) {
    __shared__ TrackLds sm;
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int slot = row_slot[b];
    if (slot < 0 || slot >= st.n_slots) {                        // the row carries no frame: nothing of any pool is touched
        if (lane == 0) out_cnt[b] = 0;
        return;
    }
    const int T = st.T;
    const sy_track_tick tk = ticks[b];
    int32_t* hdr = st.hdr + (long long)slot * 4;
    float* gx = st.x + (long long)slot * 8 * T;
    float* gP = st.P + (long long)slot * kNP * T;
    float* gscore = st.score + (long long)slot * T;
    int32_t* glabel = st.label + (long long)slot * T;
    int32_t* gid = st.id + (long long)slot * T;
    out += (long long)b * T * 6;
    out_id += (long long)b * T;

    // ---- 1. reset ----
    const bool first = row_first[b] != 0;
    int n = first ? 0 : hdr[0], n_matched = first ? 0 : hdr[1], next_id = first ? 0 : hdr[2];
    n = sy_min(sy_max(n, 0), T);                                 // (a pool nobody initialised cannot lead outside it)
    n_matched = sy_min(sy_max(n_matched, 0), n);
    int m = cnt[b];
    m = sy_min(sy_min(sy_max(m, 0), T), max_det);                // ---- 3. truncate ----
    const float dt = (float)tk.dt_frames;
    const float* D = det + (long long)b * max_det * 7;

    // ---- 2. predict: x <- F x, P <- F P F' + Q, into LDS; the loop's copy of the boxes stays in registers ----
    float bl[kPerLane], bt[kPerLane], bw[kPerLane], bh[kPerLane];
    int blab[kPerLane];
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
        const int t = c * kWave + lane;
        bl[c] = bt[c] = bw[c] = bh[c] = 0.0f;
        blab[c] = -1;
        if (t < n) {
            float x[8], P[8][8];
#pragma unroll
            for (int i = 0; i < 8; ++i) x[i] = gx[i * T + t];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = i; j < 8; ++j) P[i][j] = P[j][i] = gP[tri(i, j) * T + t];
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = x[i] + dt * x[i + 4];
            // (F P) F' in the reference's order: rows first, then columns
            float FP[8][8];
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 8; ++j) FP[i][j] = i < 4 ? P[i][j] + dt * P[i + 4][j] : P[i][j];
            const float qd = dt * dt * prm.q;
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = i; j < 8; ++j) {
                    float v = j < 4 ? FP[i][j] + dt * FP[i][j + 4] : FP[i][j];
                    if (i == j) v = v + qd;
                    sm.P[tri(i, j)][t] = v;
                    if (m == 0) gP[tri(i, j) * T + t] = v;      // no detections: the predicted state IS the new state
                }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                sm.x[i][t] = x[i];
                if (m == 0) gx[i * T + t] = x[i];
            }
            bl[c] = x[0]; bt[c] = x[1]; bw[c] = x[2]; bh[c] = x[3];
            blab[c] = glabel[t];
            sm.oid[t] = gid[t];
            if (m == 0) {
                sm.d[0][t] = gscore[t];
                sm.d[1][t] = as_f(blab[c]);
                sm.d[2][t] = as_f(sm.oid[t]);
            }
        }
    }
    if (m == 0) {                                                // n, n_matched, labels, scores, ids stay as they are
        if (first && lane == 0) { hdr[0] = 0; hdr[1] = 0; hdr[2] = 0; }
        sy_wave_fence();
        forecast_and_write(sm, n, n_matched, tk.horizon, tk.img_w, tk.img_h, prm.min_size, T, out, out_id, out_cnt + b, lane);
        return;
    }

    // the detections in camera coordinates, ltwh: lane jj keeps detections jj, jj + 64, ... in registers
    float zl[kPerLane], zt[kPerLane], zw[kPerLane], zh[kPerLane], zscore[kPerLane];
    int zlab[kPerLane], mtr[kPerLane], posr[kPerLane];           // mtr: the old track the detection took, or -1; posr: its rank
#pragma unroll                                                   //   among the matched / the unmatched detections
    for (int c = 0; c < kPerLane; ++c) {
        const int j = c * kWave + lane;
        zl[c] = zt[c] = zw[c] = zh[c] = zscore[c] = 0.0f;
        zlab[c] = -2;
        mtr[c] = -1;
        posr[c] = j;
        if (j < m) {
            const float* r = D + (long long)j * 7;
            const float x1 = r[0] / tk.divisor, y1 = r[1] / tk.divisor, x2 = r[2] / tk.divisor, y2 = r[3] / tk.divisor;
            zl[c] = x1; zt[c] = y1; zw[c] = x2 - x1; zh[c] = y2 - y1;
            zscore[c] = r[4] * r[5];
            zlab[c] = (int)r[6];
        }
    }

    // ---- 4. associate: serial over the detections; per step a readlane broadcast of the detection, up to four IoUs per lane, a
    // wave maximum on the VALU (sy_wave_max) and one ballot per track chunk for the winner — nothing goes through LDS ----
    int n_m = 0;
    if (n > 0) {
        unsigned taken = 0u;                                     // bit c: this lane's track c has been matched
        int n_u = 0;
        const float th = prm.match_iou_th;
#pragma unroll
        for (int cd = 0; cd < kPerLane; ++cd) {
            const int jn = sy_min(m - cd * kWave, kWave);
            for (int jj = 0; jj < jn; ++jj) {
                const float dl = sy_readlane(zl[cd], jj), dtp = sy_readlane(zt[cd], jj), dw = sy_readlane(zw[cd], jj),
                            dh = sy_readlane(zh[cd], jj);
                const int dlab = sy_readlane(zlab[cd], jj);
                const float da = dw * dh;
                float v[kPerLane], best = -1.0f;
#pragma unroll
                for (int c = 0; c < kPerLane; ++c) {
                    const int t = c * kWave + lane;
                    v[c] = -1.0f;
                    if (t < n && !((taken >> c) & 1u) && blab[c] == dlab) {
                        const float iw = fmaxf(fminf(bl[c] + bw[c], dl + dw) - fmaxf(bl[c], dl), 0.0f);
                        const float ih = fmaxf(fminf(bt[c] + bh[c], dtp + dh) - fmaxf(bt[c], dtp), 0.0f);
                        const float inter = iw * ih;
                        const float iou = inter / (bw[c] * bh[c] + da - inter);
                        if (iou >= th) v[c] = iou;               // (a NaN IoU of two empty boxes stays out)
                    }
                    best = fmaxf(best, v[c]);
                }
                const float mx = sy_wave_max(best);
                // the winner: the HIGHEST track index among the tracks at the maximum, as the reference's scan replaces its best
                // on >= (th > 0, so an excluded track's -1 never equals the maximum)
                int ti = -1;
                if (mx >= th) {
#pragma unroll
                    for (int c = kPerLane - 1; c >= 0; --c) {
                        if (ti < 0) {
                            const unsigned long long at = __ballot(v[c] == mx ? 1 : 0);
                            if (at != 0ull) ti = c * kWave + 63 - __builtin_clzll(at);
                        }
                    }
                }
                if (ti >= 0) {
                    if ((ti & (kWave - 1)) == lane) taken |= 1u << (ti >> 6);
                    if (jj == lane) { mtr[cd] = ti; posr[cd] = n_m; }
                    ++n_m;
                } else {
                    if (jj == lane) posr[cd] = n_u;
                    ++n_u;
                }
            }
        }
    }

    sy_wave_fence();                                             // the predicted tracks of every lane are in LDS

    // ---- 5. rebuild + 6. store: detection j becomes track k; the lane keeps what the forecast needs ----
    float nx[kPerLane][8], nscore[kPerLane];
    int nk[kPerLane], nlab[kPerLane], nid[kPerLane];
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
        const int j = c * kWave + lane;
        nk[c] = -1;
        if (j < m) {
            const int ti = mtr[c];
            const int k = ti >= 0 ? posr[c] : n_m + posr[c];
            const float z[4] = {zl[c], zt[c], zw[c], zh[c]};
            float x[8];
            if (ti >= 0) {
                float P[8][8];
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = sm.x[i][ti];
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int jj = i; jj < 8; ++jj) P[i][jj] = P[jj][i] = sm.P[tri(i, jj)][ti];
                // S = P[:4, :4] + r I = L L' (symmetric positive definite), S^-1 = L^-T L^-1
                float L[4][4], Li[4][4], Si[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) { L[i][jj] = 0.0f; Li[i][jj] = 0.0f; }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int jj = 0; jj <= i; ++jj) {
                        float s = P[i][jj] + (i == jj ? prm.r : 0.0f);
#pragma unroll
                        for (int q = 0; q < jj; ++q) s = s - L[i][q] * L[jj][q];
                        L[i][jj] = i == jj ? sqrtf(s) : s / L[jj][jj];
                    }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    Li[jj][jj] = 1.0f / L[jj][jj];
#pragma unroll
                    for (int i = jj + 1; i < 4; ++i) {
                        float s = 0.0f;
#pragma unroll
                        for (int q = jj; q < i; ++q) s = s - L[i][q] * Li[q][jj];
                        Li[i][jj] = s / L[i][i];
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        float s = 0.0f;
#pragma unroll
                        for (int q = (i > jj ? i : jj); q < 4; ++q) s = s + Li[q][i] * Li[q][jj];
                        Si[i][jj] = s;
                    }
                // K = P[:, :4] S^-1;  x += K (z - x[:4]);  P -= K P[:4, :]
                float K[8][4], y[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) y[i] = z[i] - x[i];
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        float s = 0.0f;
#pragma unroll
                        for (int q = 0; q < 4; ++q) s = s + P[i][q] * Si[q][jj];
                        K[i][jj] = s;
                    }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float s = 0.0f;
#pragma unroll
                    for (int q = 0; q < 4; ++q) s = s + K[i][q] * y[q];
                    x[i] = x[i] + s;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int jj = i; jj < 8; ++jj) {
                        float s = 0.0f;
#pragma unroll
                        for (int q = 0; q < 4; ++q) s = s + K[i][q] * P[q][jj];
                        gP[tri(i, jj) * T + k] = P[i][jj] - s;
                    }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) x[i] = i < 4 ? z[i] : 0.0f;
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int jj = i; jj < 8; ++jj) gP[tri(i, jj) * T + k] = i == jj ? prm.p_init : 0.0f;
            }
            const int id = ti >= 0 ? sm.oid[ti] : next_id + posr[c];
            const int lab = zlab[c];
            const float score = zscore[c];
#pragma unroll
            for (int i = 0; i < 8; ++i) { gx[i * T + k] = x[i]; nx[c][i] = x[i]; }
            gscore[k] = score; glabel[k] = lab; gid[k] = id;
            nk[c] = k; nscore[c] = score; nlab[c] = lab; nid[c] = id;
        }
    }
    if (lane == 0) { hdr[0] = m; hdr[1] = n_m; hdr[2] = next_id + (m - n_m); hdr[3] = 0; }
    sy_wave_fence();                                             // every lane has read the old tracks: LDS takes the new ones
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
        if (nk[c] >= 0) {
            const int k = nk[c];
#pragma unroll
            for (int i = 0; i < 8; ++i) sm.x[i][k] = nx[c][i];
            sm.d[0][k] = nscore[c]; sm.d[1][k] = as_f(nlab[c]); sm.d[2][k] = as_f(nid[c]);
        }
    }
    sy_wave_fence();
    // ---- 7. forecast ----
    forecast_and_write(sm, m, n_m, tk.horizon, tk.img_w, tk.img_h, prm.min_size, T, out, out_id, out_cnt + b, lane);
}

__global__ __launch_bounds__(kWave) void track_forecast_kernel(const sy_track_query* queries, Pools st, sy_track_params prm, float* out,
                                                               int32_t* out_id, int32_t* out_cnt) {
    __shared__ TrackLds sm;
    const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
    const sy_track_query q = queries[e];
    if (q.slot < 0 || q.slot >= st.n_slots) {
        if (lane == 0) out_cnt[e] = 0;
        return;
    }
    const int T = st.T;
    const int32_t* hdr = st.hdr + (long long)q.slot * 4;
    const int n = sy_min(sy_max(hdr[0], 0), T), n_matched = sy_min(sy_max(hdr[1], 0), n);
    const float* gx = st.x + (long long)q.slot * 8 * T;
#pragma unroll
    for (int c = 0; c < kPerLane; ++c) {
        const int t = c * kWave + lane;
        if (t < n) {
#pragma unroll
            for (int i = 0; i < 8; ++i) sm.x[i][t] = gx[i * T + t];
            sm.d[0][t] = st.score[(long long)q.slot * T + t];
            sm.d[1][t] = as_f(st.label[(long long)q.slot * T + t]);
            sm.d[2][t] = as_f(st.id[(long long)q.slot * T + t]);
        }
    }
    sy_wave_fence();
    forecast_and_write(sm, n, n_matched, q.horizon, q.img_w, q.img_h, prm.min_size, T, out + (long long)e * T * 6,
                       out_id + (long long)e * T, out_cnt + e, lane);
}

inline bool pools_ok(const sy_track_state* s, Pools& p) {
    if (s == nullptr || s->x == nullptr || s->P == nullptr || s->score == nullptr || s->label == nullptr || s->id == nullptr ||
        s->hdr == nullptr || s->n_slots <= 0 || s->max_tracks <= 0 || s->max_tracks > kMaxT)
        return false;
    p.x = s->x; p.P = s->P; p.score = s->score; p.label = s->label; p.id = s->id; p.hdr = s->hdr;
    p.n_slots = s->n_slots; p.T = s->max_tracks;
    return true;
}

}  // namespace

extern "C" int sy_track_update(const float* det, const int32_t* cnt, int B, int max_det, const int32_t* row_slot,
                               const uint8_t* row_first, const sy_track_tick* ticks, const sy_track_state* state,
                               const sy_track_params* params, float* out, int32_t* out_id, int32_t* out_cnt, void* stream) {
    Pools p;
    if (det == nullptr || cnt == nullptr || row_slot == nullptr || row_first == nullptr || ticks == nullptr || params == nullptr ||
        out == nullptr || out_id == nullptr || out_cnt == nullptr || B <= 0 || B > 65535 || max_det <= 0 || !pools_ok(state, p))
        return SY_ERR_ARG;
    if (!(params->match_iou_th > 0.0f)) return SY_ERR_ARG;      // (the arg-max key of the association orders positive IoUs)
    SY_LAUNCH(track_update_kernel, dim3(B), dim3(kWave), 0, stream, det, cnt, max_det, row_slot, row_first, ticks, p, *params, out,
              out_id, out_cnt);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}

extern "C" int sy_track_forecast(const sy_track_query* queries, int n, const sy_track_state* state, const sy_track_params* params,
                                 float* out, int32_t* out_id, int32_t* out_cnt, void* stream) {
    Pools p;
    if (queries == nullptr || params == nullptr || out == nullptr || out_id == nullptr || out_cnt == nullptr || n <= 0 || n > 65535 ||
        !pools_ok(state, p))
        return SY_ERR_ARG;
    SY_LAUNCH(track_forecast_kernel, dim3(n), dim3(kWave), 0, stream, queries, p, *params, out, out_id, out_cnt);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}
