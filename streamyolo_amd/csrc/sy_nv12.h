// sy_nv12.h — the per-pixel NV12 -> (B, G, R) conversion shared by the kernels that read camera surfaces (input_pipeline.hip packs
// frames with it, crop.hip converts every tap with it): the arithmetic include/streamyolo_hip.h states for SY_PIX_NV12.
#pragma once
#include "sy_device.h"

namespace sy_nv12 {

// ---- NV12 (see the header): BT.601 limited range, int32 fixed point with 20 fractional bits.  No intermediate leaves int32:
// |1220542 y'| <= 2.92e8, the chroma terms with the rounding constant are within [-1.62e8, 2.70e8].
struct Chroma { int b, g, r; };         // the chroma terms of B, G, R with the rounding constant: once per (U, V) pair
__device__ __forceinline__ Chroma nv12_chroma(int U, int V) {
    const int u = U - 128, v = V - 128;
    Chroma k;
    k.b = 2116026 * u + (1 << 19);
    k.g = -409993 * u - 852492 * v + (1 << 19);
    k.r = 1673527 * v + (1 << 19);
    return k;
}
__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ void nv12_bgr(int Y, const Chroma& k, int o[3]) {
    const int y = 1220542 * (Y - 16 < 0 ? 0 : Y - 16);
    o[0] = sat8((y + k.b) >> 20);
    o[1] = sat8((y + k.g) >> 20);
    o[2] = sat8((y + k.r) >> 20);
}

}  // namespace sy_nv12
