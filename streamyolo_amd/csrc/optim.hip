// optim.hip — the whole optimizer + EMA step of a training iteration in ONE launch.
//
// Replaces: `self.scaler.step(self.optimizer)` + `self.ema_model.update(self.model)`
// (exps/train_utils/double_trainer.py:115-119) — in the reference 2 x 768 tiny launches per iteration:
//   * torch.optim.SGD(momentum, nesterov=True) over the three YOLOX parameter groups (BatchNorm weights, conv /
//     linear weights with weight decay, biases), on fp32 master parameters;
//   * yolox ModelEMA.update: every floating state_dict entry v <- d*v + (1-d)*x, d = decay*(1 - exp(-updates/2000))
//     (parameters AND BatchNorm running statistics; d is computed by the host).
// HBM-bound streaming work: per parameter element read p, g, buf, ema and write p, buf, ema (28 B); per buffer
// element 12 B.  One workgroup = one 1024-element chunk of one tensor, found by bisection over the table's chunk
// prefix.  Arithmetic order follows torch.optim.SGD exactly (d = g*scale; d += wd*p; buf = first ? d : m*buf + d;
// d += m*buf; p -= lr*d) with -ffp-contract=off, then the EMA reads the UPDATED parameter, as the reference's
// call order does.
//
// Dynamic loss scaling (GradScaler.step / .update of double_trainer.py:115-116) lives here too, device-resident:
//   grad_nonfinite_kernel   one read of the gradients, found_inf = 1 if any element is inf / nan;
//   sgd_ema_kernel<true>    the same update with grad_scale = extra_scale * state->inv_scale, its parameter / momentum half
//                           predicated on found_inf == 0 (the EMA half runs either way, as ema_model.update does after a
//                           skipped scaler.step);
//   loss_scale_update_kernel  GradScaler.update()'s rule on the state.
// The state is read through a device pointer inside the kernels: a launch tape replays argument VALUES, a scale passed by value
// would be the one of the recording step for ever.
#include "sy_device.h"
#include "../../include/streamyolo_hip.h"

namespace {

constexpr int kChunk = 1024;

// kScaled: grad_scale is multiplied by the state's inv_scale and the parameter half is skipped when found_inf is set.  There is
// no first_step then — the host cannot know whether step 0 was skipped.  The momentum buffer starts zeroed instead:
// 0 * momentum + d == d, the value torch's `buf = clone(d)` of the first TAKEN step has (a -0.0 gradient leaves +0.0 where torch
// leaves -0.0; no later value depends on the sign of a zero).
template <bool kScaled>
__global__ __launch_bounds__(256) void sgd_ema_kernel(const sy_optim_entry* entries, int n_entries, float lr, float momentum,
                                                      float grad_scale, float ema_d, int first_step,
                                                      const sy_scaler_state* scaler) {
    int lo = 0, hi = n_entries - 1;                           // last entry with chunk0 <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (entries[mid].chunk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    sy_optim_entry e = entries[lo];
    if (kScaled) {
        grad_scale = grad_scale * scaler->inv_scale;
        if (scaler->found_inf != 0) e.g = nullptr;            // skipped step: p and buf untouched (not even read), EMA of the old p
    }
    const long long base = ((long long)blockIdx.x - e.chunk0) * kChunk;
    const float one_minus_d = 1.0f - ema_d;
    for (int k = threadIdx.x; k < kChunk; k += 256) {
        const long long i = base + k;
        if (i >= e.n) break;
        float x = e.p[i];
        if (e.g != nullptr) {
            float d = e.g[i] * grad_scale;
            if (e.weight_decay != 0.0f) d = d + e.weight_decay * x;
            float b = d;
            if (e.buf != nullptr) {
                if (!first_step) b = e.buf[i] * momentum + d;
                e.buf[i] = b;
                d = d + momentum * b;                         // nesterov
            }
            x = x - (lr * e.lr_mult) * d;
            e.p[i] = x;
        }
        if (e.ema != nullptr) {
            float v = e.ema[i] * ema_d;
            v = v + one_minus_d * x;
            e.ema[i] = v;
        }
    }
}

// found_inf = 1 if any gradient element is inf / nan (exponent bits all ones).  A workgroup owns `per_block` consecutive
// 1024-element chunks of the table: one bisection for the first, then the entry index only moves forward.  A thread reads 16 bytes
// per chunk where the chunk's start is 16-byte aligned (always, on the flat arena's 64-element-aligned slots; a scattered .grad
// may start anywhere) and whole; the flag leaves through LDS and ONE ordinary store of thread 0 — every writer stores the same 1.
__global__ __launch_bounds__(256) void grad_nonfinite_kernel(const sy_optim_entry* entries, int n_entries, int total_chunks,
                                                             int per_block, sy_scaler_state* scaler) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    int chunk = (int)blockIdx.x * per_block;
    int end = chunk + per_block;
    if (end > total_chunks) end = total_chunks;
    int lo = 0, hi = n_entries - 1;                           // last entry with chunk0 <= chunk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (entries[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    unsigned bad = 0u;                                        // exponent field == 0xff in any element seen by this thread
    auto test = [&](unsigned u) { bad |= (unsigned)((u & 0x7f800000u) == 0x7f800000u); };
    for (; chunk < end; ++chunk) {
        while (lo + 1 < n_entries && entries[lo + 1].chunk0 <= chunk) ++lo;
        const unsigned* g = reinterpret_cast<const unsigned*>(entries[lo].g);
        if (g == nullptr) continue;
        const long long n = entries[lo].n;
        const long long base = ((long long)chunk - entries[lo].chunk0) * kChunk;
        const long long left = n - base;                      // >= 1: chunk0 counts ceil(n / 1024) chunks per entry
        if (left >= kChunk && (reinterpret_cast<unsigned long long>(g + base) & 15ull) == 0ull) {
            const uint4 v = reinterpret_cast<const uint4*>(g + base)[threadIdx.x];
            test(v.x); test(v.y); test(v.z); test(v.w);
        } else {
            for (int k = threadIdx.x; k < kChunk && k < left; k += 256) test(g[base + k]);
        }
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0 && s_bad != 0) scaler->found_inf = 1;
}

// torch.amp.GradScaler.update (torch/amp/grad_scaler.py, _amp_update_scale_): one thread.
__global__ void loss_scale_update_kernel(sy_scaler_state* scaler, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float scale = scaler->scale;
    if (scaler->found_inf != 0) {
        scale = scale * backoff;
        scaler->growth_tracker = 0;
        scaler->steps_skipped = scaler->steps_skipped + 1;
    } else {
        const int t = scaler->growth_tracker + 1;
        if (t == interval) {
            const float grown = scale * growth;
            if ((__builtin_bit_cast(unsigned, grown) & 0x7f800000u) != 0x7f800000u) scale = grown;   // never grow into inf
            scaler->growth_tracker = 0;
        } else {
            scaler->growth_tracker = t;
        }
        scaler->steps_taken = scaler->steps_taken + 1;
    }
    scaler->scale = scale;
    scaler->inv_scale = (float)(1.0 / (double)scale);         // GradScaler.unscale_: scale.double().reciprocal().float()
    scaler->found_inf = 0;
}

}  // namespace

extern "C" int sy_sgd_ema_step(const sy_optim_entry* entries, int n_entries, int total_chunks, float lr, float momentum,
                               float grad_scale, float ema_decay, int first_step, void* stream) {
    if (entries == nullptr || n_entries <= 0 || total_chunks <= 0) return SY_ERR_ARG;
    SY_LAUNCH(sgd_ema_kernel<false>, dim3(total_chunks), dim3(256), 0, stream, entries, n_entries, lr, momentum, grad_scale,
              ema_decay, first_step, (const sy_scaler_state*)nullptr);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}

extern "C" int sy_grad_nonfinite(const sy_optim_entry* entries, int n_entries, int total_chunks, void* scaler_state,
                                 void* stream) {
    if (entries == nullptr || n_entries <= 0 || total_chunks <= 0 || scaler_state == nullptr) return SY_ERR_ARG;
    // a few resident workgroups per CU, each streaming a contiguous run of chunks (the l arena: 53 k chunks -> 13 per workgroup)
    constexpr int kMaxBlocks = 4096;
    const int per_block = (total_chunks + kMaxBlocks - 1) / kMaxBlocks;
    const int blocks = (total_chunks + per_block - 1) / per_block;
    SY_LAUNCH(grad_nonfinite_kernel, dim3(blocks), dim3(256), 0, stream, entries, n_entries, total_chunks, per_block,
              (sy_scaler_state*)scaler_state);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}

extern "C" int sy_sgd_ema_step_scaled(const sy_optim_entry* entries, int n_entries, int total_chunks, float lr, float momentum,
                                      float extra_scale, float ema_decay, const void* scaler_state, void* stream) {
    if (entries == nullptr || n_entries <= 0 || total_chunks <= 0 || scaler_state == nullptr) return SY_ERR_ARG;
    SY_LAUNCH(sgd_ema_kernel<true>, dim3(total_chunks), dim3(256), 0, stream, entries, n_entries, lr, momentum, extra_scale,
              ema_decay, 0, (const sy_scaler_state*)scaler_state);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}

extern "C" int sy_loss_scale_update(void* scaler_state, float growth_factor, float backoff_factor, int growth_interval,
                                    void* stream) {
    if (scaler_state == nullptr || growth_interval <= 0 || !(growth_factor > 1.0f) || !(backoff_factor > 0.0f && backoff_factor < 1.0f))
        return SY_ERR_ARG;
    SY_LAUNCH(loss_scale_update_kernel, dim3(1), dim3(64), 0, stream, (sy_scaler_state*)scaler_state, growth_factor,
              backoff_factor, growth_interval);
    return SY_LAUNCH_OK() == 0 ? SY_OK : SY_ERR_LAUNCH;
}
