// stream_state.hip — per-stream DFP state of a batched streaming tick: row-indexed movers for the NHWC PAN buffers.
//
// Replaces (per batch row) the `buffer` hand-over of the reference's on_pipe loop (dfp_pafpn.py:211-228): the support operand of
// the fusion is the previous frame's pre-fusion PAN output of THE SAME CAMERA, or the current one at a sequence start (node
// 'star', :211-214); the current PAN outputs are kept as that camera's next support (:226).  One detector serves many cameras
// from one batched plan: camera state lives in a pool [S][H][W][C] per PAN level, and two small device tables say, per batch row
// of this tick, which pool slot the row belongs to (row_slot, < 0 = the row carries no frame) and whether its sequence starts
// here (row_first).
//   stream_state_gather_kernel    one level: sup[b] <- row continues ? pool[row_slot[b]] : cur[b]
//   stream_state_scatter_kernel   all levels (descriptor table, one launch): pool[row_slot[b]] <- cur[b] for rows with a slot
// The tables are read through device pointers inside the kernels: a launch tape replays argument VALUES, so a slot passed by value
// would be the one of the recording tick for ever (the mechanism of sy_scaler_state, optim.hip).  Pure data movement, any dtype:
// everything is counted in 16-byte pieces (C * element size, the pixel pitches and the batch strides are multiples of 16 bytes),
// one piece per lane and trip, grid-strided inside a row; blockIdx.y = the batch row, so the table reads are wave-uniform.
#include "sy_device.h"
#include "../../include/streamyolo_hip.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxBlocksPerRow = 512;                            // x 16 B x 256 lanes = 2 MiB per trip and batch row

// [pixels][pieces] 16-byte pieces of one image: src / dst pixel pitches in pieces
__device__ __forceinline__ void copy_image(const uint4* src, long long src_pitch, uint4* dst, long long dst_pitch, int pieces,
                                           long long total, long long first, long long step) {
    for (long long i = first; i < total; i += step) {
        const long long pix = i / pieces;
        const int cc = (int)(i - pix * pieces);
        dst[pix * dst_pitch + cc] = src[pix * src_pitch + cc];
    }
}

__global__ __launch_bounds__(kBlock) void stream_state_gather_kernel(const uint4* cur, long long cur_pitch, long long cur_bs,
                                                                     const uint4* pool, int n_slots, uint4* sup,
                                                                     long long sup_pitch, long long sup_bs, int pixels, int pieces,
                                                                     const int32_t* row_slot, const uint8_t* row_first) {
    const int b = (int)blockIdx.y;
    const int slot = row_slot[b];
    // an out-of-range slot is treated like an inactive row: nothing outside the pool is ever read
    const bool from_pool = slot >= 0 && slot < n_slots && row_first[b] == 0;
    const uint4* src = from_pool ? pool + (long long)slot * pixels * pieces : cur + (long long)b * cur_bs;
    const long long src_pitch = from_pool ? (long long)pieces : cur_pitch;
    copy_image(src, src_pitch, sup + (long long)b * sup_bs, sup_pitch, pieces, (long long)pixels * pieces,
               (long long)blockIdx.x * kBlock + threadIdx.x, (long long)gridDim.x * kBlock);
}

// the scatter's descriptor table, by value in the kernel-argument segment (addresses in 16-byte pieces)
constexpr int kMaxLevels = 8;
struct ScatterLevel {
    const uint4* cur;
    uint4* pool;
    long long cur_pitch, cur_bs;
    int pixels, pieces, block0, blocks;                          // workgroups [block0, block0 + blocks) of a row belong to this level
};
struct ScatterTable {
    ScatterLevel l[kMaxLevels];
    int n;
};

__global__ __launch_bounds__(kBlock) void stream_state_scatter_kernel(ScatterTable t, int n_slots, const int32_t* row_slot) {
    const int b = (int)blockIdx.y;
    const int slot = row_slot[b];
    if (slot < 0 || slot >= n_slots) return;                     // the row carries no frame: its state stays as it is
    ScatterLevel e = t.l[0];                                     // last level with block0 <= blockIdx.x (a handful of levels)
#pragma unroll
    for (int k = 1; k < kMaxLevels; ++k)
        if (k < t.n && t.l[k].block0 <= (int)blockIdx.x) e = t.l[k];
    copy_image(e.cur + (long long)b * e.cur_bs, e.cur_pitch, e.pool + (long long)slot * e.pixels * e.pieces, (long long)e.pieces,
               e.pieces, (long long)e.pixels * e.pieces, ((long long)blockIdx.x - e.block0) * kBlock + threadIdx.x,
               (long long)e.blocks * kBlock);
}

inline bool aligned16(unsigned long long v) { return (v & 15ull) == 0ull; }
inline int elem_bytes(int dtype) { return dtype == SY_DT_F32 ? 4 : (dtype == SY_DT_F16 || dtype == SY_DT_BF16) ? 2 : 0; }

}  // namespace

static int blocks_for(long long pieces_per_image) {
    long long b = (pieces_per_image + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    return (int)(b > kMaxBlocksPerRow ? kMaxBlocksPerRow : b);
}

extern "C" int sy_stream_state_gather(const void* cur, int ld_cur, int64_t cur_bs, const void* pool, int n_slots, void* sup,
                                      int ld_sup, int64_t sup_bs, int B, int H, int W, int C, const int32_t* row_slot,
                                      const uint8_t* row_first, int dtype, void* stream) {
    const int es = elem_bytes(dtype);
    if (cur == nullptr || pool == nullptr || sup == nullptr || row_slot == nullptr || row_first == nullptr || es == 0) return SY_ERR_ARG;
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || C <= 0 || n_slots <= 0 || ld_cur < C || ld_sup < C) return SY_ERR_ARG;
    if (cur_bs < (int64_t)H * W * ld_cur || sup_bs < (int64_t)H * W * ld_sup) return SY_ERR_ARG;
    if (!aligned16((unsigned long long)cur) || !aligned16((unsigned long long)pool) || !aligned16((unsigned long long)sup) ||
        !aligned16((unsigned long long)C * es) || !aligned16((unsigned long long)ld_cur * es) || !aligned16((unsigned long long)ld_sup * es) ||
        !aligned16((unsigned long long)cur_bs * es) || !aligned16((unsigned long long)sup_bs * es))
        return SY_ERR_ARG;
    const int pixels = H * W, pieces = C * es / 16;
    SY_LAUNCH(stream_state_gather_kernel, dim3(blocks_for((long long)pixels * pieces), B), dim3(kBlock), 0, stream,
              (const uint4*)cur, (long long)ld_cur * es / 16, (long long)(cur_bs * es / 16), (const uint4*)pool, n_slots, (uint4*)sup,
              (long long)ld_sup * es / 16, (long long)(sup_bs * es / 16), pixels, pieces, row_slot, row_first);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}

extern "C" int sy_stream_state_scatter(const sy_stream_level* levels, int n_levels, int n_slots, int B, const int32_t* row_slot,
                                       int dtype, void* stream) {
    const int es = elem_bytes(dtype);
    if (levels == nullptr || row_slot == nullptr || es == 0 || n_levels <= 0 || n_levels > kMaxLevels || n_slots <= 0 || B <= 0 ||
        B > 65535)
        return SY_ERR_ARG;
    ScatterTable t;
    __builtin_memset(&t, 0, sizeof(t));
    t.n = n_levels;
    int total = 0;
    for (int k = 0; k < n_levels; ++k) {
        const sy_stream_level& v = levels[k];
        if (v.cur == nullptr || v.pool == nullptr || v.H <= 0 || v.W <= 0 || v.C <= 0 || v.ld < v.C || v.bs < (int64_t)v.H * v.W * v.ld)
            return SY_ERR_ARG;
        if (!aligned16((unsigned long long)v.cur) || !aligned16((unsigned long long)v.pool) || !aligned16((unsigned long long)v.C * es) ||
            !aligned16((unsigned long long)v.ld * es) || !aligned16((unsigned long long)v.bs * es))
            return SY_ERR_ARG;
        ScatterLevel& e = t.l[k];
        e.cur = (const uint4*)v.cur;
        e.pool = (uint4*)v.pool;
        e.cur_pitch = (long long)v.ld * es / 16;
        e.cur_bs = (long long)(v.bs * es / 16);
        e.pixels = v.H * v.W;
        e.pieces = v.C * es / 16;
        e.block0 = total;
        e.blocks = blocks_for((long long)e.pixels * e.pieces);
        total += e.blocks;
    }
    SY_LAUNCH(stream_state_scatter_kernel, dim3(total, B), dim3(kBlock), 0, stream, t, n_slots, row_slot);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}
