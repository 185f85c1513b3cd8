/* streamyolo_hip.h — C ABI of libstreamyolo_hip.so (MI355X / gfx950 only).
 *
 * The reference (yancie-yjr/StreamYOLO) has NO native boundary on this path: its hot path is a
 * tree of Python nn.Modules dispatching cuDNN/ATen/torchvision kernels one op at a time
 * (SURVEY.md §0, §8(b)).  The drop-in surface a user sees stays Python (package `streamyolo_amd`
 * mirrors exps/model/ and cfgs/); THIS header is the seam underneath it — plain pointers, sizes
 * and a hipStream_t, no torch types — and each entry point names the reference code it replaces.
 *
 * Conventions
 *   - activations are NHWC "views": (ptr, ld = elements between consecutive pixels, batch stride);
 *     a view may be a channel slice of a wider buffer, which is how every torch.cat on the path
 *     (trap T6) disappears: producers write straight into their slice.
 *   - dtype codes: 0 = bf16, 1 = fp16, 2 = fp32 (storage of activations and packed weights;
 *     accumulation and epilogues are always fp32).
 *   - every function returns 0 on success, >0 on error (1 bad argument, 2 launch failure,
 *     3 unsupported shape); nothing aborts, nothing synchronises, everything is enqueued on `stream`.
 */
#ifndef STREAMYOLO_HIP_H
#define STREAMYOLO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SY_ABI_VERSION 7
#define SY_API __attribute__((visibility("default")))

enum { SY_DT_BF16 = 0, SY_DT_F16 = 1, SY_DT_F32 = 2 };

/* epilogue selectors of sy_conv2d */
enum {
    SY_EPI_LINEAR = 0,      /* y = acc*scale + shift                                   */
    SY_EPI_SILU = 1,        /* y = silu(acc*scale + shift) [+ residual]  (BaseConv)    */
    SY_EPI_SIGMOID = 2,     /* y = sigmoid(acc*scale + shift)            (cls preds)   */
    SY_EPI_DECODE = 3,      /* ch0,1: (v+grid)*stride; ch2,3: exp(v)*stride; ch4: sigmoid (reg+obj preds) */
    SY_EPI_BNR = 4          /* SY_CONV_DGRAD only (16-bit types, first write): y = acc, and the BatchNorm-backward REDUCE of the layer whose
                               activation gradient this launch produces rides in the epilogue — with z = that layer's raw conv output
                               (passed as `res`, same pixel / batch strides as y), its folded affine in `scale` / `shift`:
                               g = acc * silu'(scale*z + shift);  stat_sum[r][0][c] += sum g,  stat_sum[r][1][c] += sum g*z  over the
                               tile's pixels, replica r = tile % stat_copies ([copies][2][Cout] as sy_bn_silu_bwd_reduce's `sums`, but
                               the second row is the RAW moment: sy_bn_silu_bwd_apply takes it with bit 2 of dres_accumulate).
                               Replaces one sy_bn_silu_bwd_reduce launch and its read of dA (autograd of BatchNorm2d + SiLU,
                               exps/model/darknet.py:115-165 BaseConv). */
};

/* workgroup tiles of sy_conv2d (output channels x output pixels) */
enum { SY_TILE_AUTO = 0, SY_TILE_256x256 = 1, SY_TILE_128x256 = 2, SY_TILE_128x128 = 3, SY_TILE_64x256 = 4, SY_TILE_32x256 = 5,
       SY_TILE_128x64 = 6, SY_TILE_64x64 = 7, SY_TILE_256x64 = 8, SY_TILE_256x128 = 9,
       SY_TILE_RS = 16,   /* add to a tile code: register-staged variant instead of the 4-deep LDS-DMA ring */
       SY_TILE_DMA2 = 32, /* add: 2-deep LDS-DMA ring */
       SY_TILE_DMA3 = 48, /* add: 3-deep LDS-DMA ring */
       SY_TILE_WR = 80,   /* add: register-staged pixels + fragment-packed weights loaded straight into VGPRs */
       SY_TILE_HALO = 112, /* 114..118 (HALO + 2..6): 3x3 stride-1 kernel with the input tile + halo resident in LDS (csrc/conv3x3_halo.h;
                             needs wfrag): 128 ch x 2 rows x 32 px (8 waves) | 128 x 2 | 64 x 8 | 128 x 2 and 128 x 4 software-pipelined;
                             112, 113: software-pipelined, one 32 x 32 MFMA tile per wave (small launches): 64 ch x 2 rows | 128 ch x 2 rows;
                             107, 104: software-pipelined, 128 ch x 3 rows | 128 ch x 5 rows (three / five MFMAs per weight fragment);
                             101, 100, 98, 109 (96, 97: on 64 channels): THIRD generation (csrc/conv3x3_halo3.h) of 117 / 107 / 118 / 104: fragment reads with immediate
                             offsets, hand-placed instruction stream, prefetch across the channel-slab boundary (same summation order);
                             105, 106, 111: K GROUPS inside the workgroup (small launches; partial tiles summed through LDS in group order — another
                             fp32 summation order than the tiles above): 105 stride 2 forward 64 ch x 1 row, 2 groups | 106 32 ch, 4 groups |
                             111 64 ch, 2 groups (all 2 rows x 32 px);
                             119: FUSED Bottleneck forward (1x1 -> 3x3, the hidden activation kept in LDS; sy_conv_desc::pre_*);
                             110: STRIDE 2 forward, 128 ch x 2 output rows x 32 px, input window split by column parity;
                             108: STRIDE 2 data gradient (csrc/conv3x3_s2dgrad.h), four output-parity classes */
       SY_TILE_1X1K = 121 /* 121..124: 1x1 stride-1 kernel with the tile's whole K extent requested in one burst (csrc/conv1x1_tile.h; needs
                             wfrag, 16-bit types, Cin 64 / 128 / 256 / 512): 128 ch x 64 px | 64 ch x 128 px | 128 ch x 128 px | 64 ch x 64 px */ };

/* gather modes of sy_conv2d */
enum {
    SY_CONV_FWD = 0,        /* out(ho,wo) <- in(ho*s - p + kh, wo*s - p + kw)                  */
    SY_CONV_DGRAD = 1       /* out(h,w)  <- in((h + p - kh)/s, (w + p - kw)/s) when divisible  */
};

typedef struct sy_conv_desc {
    /* tensors */
    const void* x;          /* input view,  [N, H, W, Cin]   */
    const void* w;          /* packed weights [Cout][KH*KW][Cin] in `dtype`, K-contiguous      */
    const float* scale;     /* [Cout] fp32 (folded BN gamma/sqrt(var+eps), or NULL = 1)        */
    const float* shift;     /* [Cout] fp32 (folded BN shift / conv bias, or NULL = 0)          */
    const void* res;        /* optional residual view added after the activation (or NULL)    */
    void* y;                /* output view, [N, Ho, Wo, Cout]                                  */
    float* stat_sum;        /* optional [Cout]: += sum over pixels of acc   (training BN)      */
    float* stat_sqsum;      /* optional [Cout]: += sum over pixels of acc^2                    */
    /* geometry */
    int32_t N, H, W, Cin;
    int32_t Ho, Wo, Cout;
    int32_t KH, KW, stride, pad;
    int32_t ldx, ldy, ldr;              /* pixel strides, elements                              */
    int64_t xbs, ybs, rbs;              /* batch strides, elements                              */
    /* behaviour */
    int32_t dtype;                      /* SY_DT_* of x, w, res (and y unless y_f32)            */
    int32_t y_f32;                      /* 1: y is fp32 regardless of dtype                      */
    int32_t mode;                       /* SY_CONV_FWD | SY_CONV_DGRAD                           */
    int32_t epilogue;                   /* SY_EPI_*                                              */
    int32_t accumulate;                 /* 1: y += result (gradient fan-in)                      */
    float dec_stride;                   /* SY_EPI_DECODE: the level's stride (8/16/32)           */
    int32_t stat_copies;                /* stat arrays hold this many replicas [copies][Cout] (>=1) */
    int32_t stat_segments;              /* 0/1: one set of statistics; S > 1: the N images form S equal groups with
                                           separate statistics, arrays [S][copies][Cout] (N % S == 0) */
    int32_t tile;                       /* SY_TILE_AUTO or a forced workgroup tile (channels x pixels) */
    int64_t x_bytes, w_bytes;           /* bytes addressable from x / w (buffer bounds of the fast gather; 0 = unknown) */
    const void* wfrag;                  /* optional: weights re-packed in MFMA-fragment order (SY_TILE_WR variants) */
    int64_t wfrag_bytes;
    /* k_splits S > 1 (tiles 117 / 118, forward, y_f32 = 1, SY_EPI_LINEAR, no scale / shift / res / statistics): the channel slabs
       of the contraction are cut into S ranges, one per gridDim.z; split z writes its fp32 PARTIAL sums as images [z*N, (z+1)*N) of
       y (which must hold S*N images, batch stride ybs).  sy_splitk_epilogue sums the partials and applies the epilogue.  For the
       deep small-map layers of the batch-1 streaming step: 36-72 workgroups become 144-288. */
    int32_t k_splits;
    /* Fused Bottleneck forward (tile 119, eval epilogues only; csrc/bottleneck_fused.h): this 3x3 stride-1 launch first computes its
       own input h = silu(pre_scale * (pre_w x) + pre_shift) — the 1x1 BaseConv in front of it — for the tile's halo window and keeps
       it in LDS.  x is then the 1x1 convolution's input ([N, H, W, pre_cin]); Cin stays the 3x3 convolution's input width (the hidden
       channels); pre_w: that 1x1 convolution's weights in MFMA-fragment order ([Cin][pre_cin], as `wfrag` of a 1x1 launch);
       pre_scale / pre_shift: its folded BatchNorm affine, fp32 [Cin].  pre_cin + Cin <= 544, both multiples of 32.
       Replaces yolox Bottleneck.conv1 -> conv2 (+ x) as two launches. */
    int32_t pre_cin;
    const void* pre_w;
    int64_t pre_w_bytes;
    const float* pre_scale;
    const float* pre_shift;
} sy_conv_desc;

/* Implicit-GEMM convolution on the MFMA units with the fused epilogue.
 * Replaces: yolox BaseConv.forward / fuseforward = Conv2d -> BatchNorm2d -> SiLU as three kernels
 * (call sites exps/model/darknet.py:115-165, dfp_pafpn.py:33-105,168-170, tal_head.py:55-131,162-171),
 * the Bottleneck shortcut add, the DFP `+ current` add (dfp_pafpn.py:168-170), the eval-time
 * sigmoid/decode of tal_head.py:197-199,245-260, and (mode DGRAD) cuDNN's backward-data. */
SY_API int sy_conv2d(const sy_conv_desc* d, void* stream);

/* Weight gradient (fp32, +=): dw[co][tap][ci] = sum_pixels dy[p][co] * x[p@tap][ci]; with
 * dw_oihw = 1 the result lands in the nn.Parameter layout [Cout][Cin][KH][KW] (so .grad can be a
 * view of the gradient arena).  Replaces cuDNN backward-filter under autograd (double_trainer.py:114). */
typedef struct sy_wgrad_desc {
    const void* x;  const void* dy;  float* dw;
    int32_t N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad;
    int32_t ldx, lddy;  int64_t xbs, dybs;
    int32_t dtype;
    int32_t dw_oihw;
    void* workspace;                    /* optional fp32 scratch for split-K slabs (NULL: one split) */
    int64_t workspace_bytes;
    int32_t tile, target_blocks;        /* tuning knobs (0 = heuristic): workgroup tile, workgroups aimed for by split-K.
                                         * tile: 1-6 = (k rows x output channels) per workgroup, operands transposed into LDS by
                                         * scatter stores; +16 / +32 = the same tiles with both operands parked in LDS as they lie in
                                         * HBM (LDS-DMA ring of 3 / 4 slabs) and gathered by ds_read_b64_tr_b16; 3x3 stride-1, 16-bit,
                                         * Cin % 32 == 0, Cout % 16 == 0 only: 52 = all nine taps per workgroup (x halo window in LDS),
                                         * 59 = 52 with the slab loop as one instruction stream, 60 = 59 on eight waves with 64 input
                                         * channels per workgroup (Cin % 64 == 0).  52 / 59 / 60 on a layer they do not cover:
                                         * SY_ERR_UNSUPPORTED; any other unknown code: the heuristic tile. */
    int64_t x_bytes, dy_bytes;          /* bytes addressable from x / dy (buffer bounds; 0 = unknown) */
} sy_wgrad_desc;
SY_API int sy_conv2d_wgrad(const sy_wgrad_desc* d, void* stream);

/* Focus space-to-depth (trap T4: TL,BL,TR,BR) fused with NCHW fp32 -> NHWC `dtype` conversion.
 * in: [N, Ctot, H, W] fp32 planes, takes channels [c0, c0+3); out: [N, H/2, W/2, 16] (12 used, 4 zero).
 * Replaces yolox Focus.forward slicing + cat (exps/model/darknet.py:115) and torch.split (dfp_pafpn.py:120,145). */
SY_API int sy_focus_pack(const float* in, int N, int Ctot, int c0, int H, int W, void* out, int dtype, void* stream);

/* Device-side input pipeline: uint8 HWC frames -> model input in ONE launch.
 * cur / sup: [B, Hs, Ws, 3] uint8 (BGR as cv2.imread delivers them; sup = NULL for a single on_pipe frame),
 * image_stride / row_stride in bytes.  Steps, in the reference's order:
 *   decimate (1 | 2 | 0 | -1): the load-time cv2.resize (exps/dataset/tal_flip_one_future_argoversedataset.py:179-187,
 *       streamyolo_det.py:177): 1 = copy, 2 = exact 2x = (a+b+c+d+2)>>2 (OpenCV's INTER_AREA fast path), 0 = any other
 *       camera size: r = min(H/Hs, W/Ws), OpenCV's fixed-point INTER_LINEAR to (int(Ws r), int(Hs r)) (`preproc`,
 *       exps/data/data_augment_flip.py:151-167); restated from OpenCV's source, unpinned against a cv2 binary;
 *       -1 = the streaming detector's cv2.resize(img, (W, H)): each axis stretched on its own to exactly the H x W canvas
 *       (sAP/streamyolo/streamyolo_det.py:176-178, canvas = (int(Hs * in_scale), int(Ws * in_scale))), same arithmetic;
 *   mirror[b] != 0: `_mirror`'s image[:, ::-1], the same flag for both frames of a pair
 *       (exps/data/data_augment_flip.py:140-148, DoubleTrainTransform :219-222);
 *   letterbox onto an H x W canvas filled with 114, image at the top-left (`preproc` :151-167);
 *   bilinear resize of the canvas to Ho x Wo when they differ (Exp.preprocess's F.interpolate(mode="bilinear",
 *       align_corners=False), cfgs/l_s50_onex_dfp_tal_filp.py:161-172);
 *   layout SY_FRAMES_NCHW: out_cur = fp32 [B, 3 or 6, Ho, Wo] (current channels first — np.concatenate((img,
 *       support_img)), exps/data/tal_flip_mosaicdetection.py:257); out_sup unused;
 *   layout SY_FRAMES_FOCUS: out_cur / out_sup = Focus-packed [B, Ho/2, Wo/2, 16] of `dtype` (what sy_focus_pack
 *       would produce from the NCHW tensor: the stem convolution's operand). */
enum { SY_FRAMES_NCHW = 0, SY_FRAMES_FOCUS = 1 };
SY_API int sy_frames_u8_pack(const uint8_t* cur, const uint8_t* sup, int B, int Hs, int Ws, int64_t image_stride,
                             int row_stride, int decimate, const uint8_t* mirror, int H, int W, int Ho, int Wo,
                             int layout, void* out_cur, void* out_sup, int dtype, void* stream);

/* sy_frames_u8_pack for frames in another pixel format (sy_frames_u8_pack itself = SY_PIX_BGR).  For every format the
 * output is bit for bit what sy_frames_u8_pack writes for the frame first converted to uint8 [Hs, Ws, 3] BGR: the conversion
 * happens per SOURCE pixel, before any decimation or bilinear tap — what cv2.cvtColor in front of the reference's loop does.
 *   SY_PIX_RGB   [B, Hs, Ws, 3] as BGR, channel c of the converted frame = byte 2 - c (PIL, torchvision, GStreamer).
 *   SY_PIX_NV12  what hardware video decoders deliver: cur / sup are [B] images of Hs * 3 / 2 rows of ONE pitch
 *                (row_stride >= Ws bytes): Hs rows of luma, then — starting at row Hs — Hs / 2 rows of interleaved chroma
 *                (U, V): the [Hs * 3 / 2, Ws] array cv2.cvtColor(.., COLOR_YUV2BGR_NV12) takes, with an optional pitch.
 *                A surface whose chroma plane starts elsewhere (a padded luma height, a detached plane, a pitch of its
 *                own) goes through sy_frames_u8_pack_surfaces below, which reads it in place.
 *                Hs and Ws even (else SY_ERR_UNSUPPORTED); image_stride >= row_stride * Hs * 3 / 2 (else SY_ERR_ARG).
 *                Chroma of pixel (y, x) = the pair at chroma row y >> 1, byte 2 * (x >> 1): nearest, no interpolation.
 *                BT.601 limited range in int32 fixed point, as OpenCV publishes it for COLOR_YUV2BGR_NV12 (restated from
 *                published source, unpinned against a cv2 binary):
 *                    y' = max(Y - 16, 0), u = U - 128, v = V - 128
 *                    B = sat8((1220542 y' + 2116026 u            + (1 << 19)) >> 20)
 *                    G = sat8((1220542 y' -  409993 u - 852492 v + (1 << 19)) >> 20)
 *                    R = sat8((1220542 y' + 1673527 v            + (1 << 19)) >> 20)
 * Reads stay inside Hs (NV12: Hs * 3 / 2) rows of row_stride bytes.  An unknown format: SY_ERR_ARG. */
enum { SY_PIX_BGR = 0, SY_PIX_RGB = 1, SY_PIX_NV12 = 2 };
SY_API int sy_frames_u8_pack_fmt(const uint8_t* cur, const uint8_t* sup, int B, int Hs, int Ws, int64_t image_stride,
                                 int row_stride, int decimate, const uint8_t* mirror, int H, int W, int Ho, int Wo,
                                 int layout, void* out_cur, void* out_sup, int dtype, int format, void* stream);

/* The same pipeline with one frame source PER BATCH ROW, read on the device: cameras of different resolutions in one batch
 * (MultiStreamDetector's mixed mode).  rows: B descriptors in DEVICE memory; row b of out_cur is bit for bit what
 * sy_frames_u8_pack writes for that frame alone (same Hs, Ws, decimate, mirror, H, W, Ho, Wo, layout, dtype; sup = NULL).
 * ONE launch whose grid depends on (B, Ho, Wo, layout) only, so a recorded launch serves any table contents.  A row with
 * cur == NULL or Hs == 0 has no frame: the plain 114 canvas, nothing is read.  The host cannot see the table: the caller
 * validates it (every frame addressable for Hs rows of row_stride >= 3 Ws bytes — SY_PIX_NV12: Hs * 3 / 2 rows of
 * row_stride >= Ws bytes; decimate as above); a descriptor that sy_frames_u8_pack_fmt would refuse (an unknown format and an
 * odd NV12 size included) is written as a row without a frame, never read through.  The format is per-row data like the size:
 * cameras of different formats share one launch.
 * layout SY_FRAMES_NCHW: out_cur = fp32 [B, 3, Ho, Wo] (dtype = SY_DT_F32); SY_FRAMES_FOCUS: [B, Ho/2, Wo/2, 16] of `dtype`. */
typedef struct sy_frame_src {      /* 32 bytes */
    const uint8_t* cur;            /* [Hs, Ws, 3] BGR / RGB or NV12 [Hs * 3 / 2, Ws]; NULL or Hs == 0: the row has no frame */
    int32_t Hs, Ws, row_stride;    /* row_stride in bytes */
    int32_t decimate;              /* 1 | 2 | 0 | -1, exactly as sy_frames_u8_pack */
    int32_t mirror;                /* != 0: image[:, ::-1] */
    int32_t format;                /* SY_PIX_*; 0 = BGR (the field was `reserved`, always 0) */
} sy_frame_src;
SY_API int sy_frames_u8_pack_rows(const sy_frame_src* rows, int B, int H, int W, int Ho, int Wo, int layout, void* out_cur,
                                  int dtype, void* stream);

/* sy_frames_u8_pack_rows for hardware decoder surfaces, read where they lie: every row names BOTH planes, each with a pitch of
 * its own, so a padded luma height (a 1080-row stream decodes into 1088 luma rows), a chroma plane in its own allocation and a
 * 10-bit stream need no repacking and no staging copy.
 *   Repacked equivalence: row b of out_cur is bit for bit what sy_frames_u8_pack_rows writes for the same frame repacked into
 *       sy_frame_src's layout (dense planes, one pitch, chroma at row Hs) — all four decimate modes, mirror, both layouts, the
 *       three Focus dtypes and the Ho x Wo canvas resize.  For SY_PIX_P010 the repacked frame is the NV12 frame of the samples'
 *       high bytes (below).
 *   ONE launch whose grid depends on (B, Ho, Wo, layout) only: a recorded launch serves any table contents — formats, pitches,
 *       plane addresses and sizes are data.
 *   SY_PIX_P010 (valid ONLY here: the other entry points keep treating 3 as an unknown format): two planes of little-endian
 *       16-bit samples with the 10 significant bits in the HIGH bits of each word; row_stride >= 2 Ws, and the chroma row of
 *       interleaved (U, V) words needs >= 2 Ws bytes too.  The 8-bit sample is the word's high byte (word >> 8: truncation, no
 *       rounding, no dithering); then SY_PIX_NV12's arithmetic applies unchanged.  This is the project's own definition: no
 *       OpenCV conversion exists to pin it against.
 *   Reads (rows; bytes per row):  plane0 BGR / RGB: < Hs; < 3 Ws.   plane0 NV12: < Hs; < Ws.   plane0 P010: < Hs; < 2 Ws.
 *       plane1 NV12: < Hs / 2; < Ws.   plane1 P010: < Hs / 2; < 2 Ws.  Nothing between Ws and a pitch, and nothing between the
 *       planes, is ever read.
 *   The host cannot see the table: the caller validates it.  A descriptor no frame can have — an unknown format, odd Hs / Ws for
 *       NV12 / P010 or decimate 2, a pitch (either one) below the row's bytes, a negative chroma_stride — is written as a row
 *       without a frame (the plain 114 canvas), never read through.
 *   rows, out_cur, B, the sizes, layout and dtype: the status codes of sy_frames_u8_pack_rows.
 *   NV12's wide-load fast path applies per row when plane0, plane1 and BOTH pitches meet its alignment (multiples of 2 for
 *       decimate 1, of 4 for decimate 2) — decided from the chroma plane's own address and pitch; bit-identical with the generic
 *       path, which P010 always takes. */
enum { SY_PIX_P010 = 3 };             /* valid ONLY in sy_frames_u8_pack_surfaces */
typedef struct sy_frame_surf {        /* 48 bytes */
    const uint8_t* plane0;            /* BGR / RGB pixels, or the luma plane; NULL or Hs == 0: the row has no frame */
    const uint8_t* plane1;            /* NV12 / P010: the interleaved (U, V) plane, wherever it lies.  NULL: plane0 + row_stride * Hs
                                         (sy_frame_src's single-allocation layout).  Ignored for BGR / RGB */
    int32_t Hs, Ws;
    int32_t row_stride;               /* bytes between rows of plane0 */
    int32_t chroma_stride;            /* bytes between rows of plane1; 0 = row_stride */
    int32_t decimate, mirror, format; /* exactly as sy_frame_src */
    int32_t reserved;                 /* 0 */
} sy_frame_surf;
SY_API int sy_frames_u8_pack_surfaces(const sy_frame_surf* rows, int B, int H, int W, int Ho, int Wo, int layout,
                                      void* out_cur, int dtype, void* stream);

/* Exp.preprocess's multi-scale resize on the reference's own tensor: fp32 NCHW [N, C, H, W] -> [N, C, Ho, Wo],
 * torch bilinear, align_corners=False (cfgs/l_s50_onex_dfp_tal_filp.py:161-172).  C = 3 or 6. */
SY_API int sy_resize_bilinear_nchw(const float* in, int N, int C, int H, int W, float* out, int Ho, int Wo, void* stream);

/* Nearest-neighbour resize to a target SIZE (trap T3), writing into a channel slice.
 * Replaces F.interpolate(size=..., mode='nearest') + torch.cat (dfp_pafpn.py:125-126,130-131). */
SY_API int sy_resize_nearest(const void* in, int N, int Hi, int Wi, int C, int ldi, int64_t ibs,
                      void* out, int Ho, int Wo, int ldo, int64_t obs, int dtype, void* stream);

/* SPP pooling: buf holds x in channels [0,C) of a 4C-wide view; writes maxpool 5/9/13 (stride 1,
 * -inf padding) into [C,2C), [2C,3C), [3C,4C) (trap T5).  Replaces SPPBottleneck's three
 * nn.MaxPool2d + cat (exps/model/darknet.py:156).  argmax (optional, training): [N,H,W,3,C] bytes,
 * the window offset of each pooled maximum, consumed by sy_spp_pool_bwd. */
SY_API int sy_spp_pool(void* buf, int N, int H, int W, int C, int ld, int64_t bs, void* argmax, int dtype,
                       void* stream);

/* The head's output transform as a stand-alone in-place pass over out [B, A, 5+nc] fp32 (anchors level-major, row-major):
 * flags & 1: boxes (xy + grid) * stride, exp(wh) * stride — TALHead.decode_outputs (exps/model/tal_head.py:245-260), what
 * tools/eval.py:187-188 calls when the head ran with decode_in_inference = False; flags & 2: sigmoid of the objectness column
 * (tal_head.py:197-199 applies it in both modes); flags & 4 (after the others): boxes (cx, cy, w, h) -> corners (cx - w/2, cy - h/2,
 * cx + w/2, cy + h/2), the in-place rewrite yolox.utils.postprocess performs on its argument before the confidence filter (the
 * reference's evaluator sees it: exps/evaluators/onex_stream_evaluator.py:148-150).  level_h / level_w / level_stride: HOST arrays of nlevels (<= 8) entries
 * (copied into the launch by value), sum h*w == A. */
SY_API int sy_head_decode(float* out, int B, int A, int nch, const int32_t* level_h, const int32_t* level_w,
                          const float* level_stride, int nlevels, int flags, void* stream);

/* Box decode + confidence filter + class-aware greedy NMS for a batch of images.
 * pred: [B, A, 5+nc] fp32 (cx,cy,w,h,obj,cls...) as produced by the head (tal_head.py:245-260).
 * Outputs per image i: out_count[i] kept detections; out_det[i][k][0..6] = x1,y1,x2,y2,obj,
 * class_conf,class_id; out_index[i][k] = anchor index; kept in descending score order.
 * Replaces yolox.utils.postprocess (exps/evaluators/onex_stream_evaluator.py:148-150) and the
 * inline `inference()` of sAP/streamyolo/streamyolo_det.py:62-83 incl. torchvision batched_nms.
 * `workspace` must hold sy_postprocess_workspace_bytes(B, A) bytes. */
SY_API int64_t sy_postprocess_workspace_bytes(int B, int A);
SY_API int sy_postprocess(const float* pred, int B, int A, int num_classes, float conf_thre, float nms_thre,
                   int max_det, float* out_det, int32_t* out_index, int32_t* out_count,
                   void* workspace, void* stream);

/* sy_postprocess with a policy PER BATCH ROW: what counts as a detection is table data, read on the device, so one recorded
 * launch list serves cameras with different thresholds, class lists, NMS modes and output caps.  `rows`: B records in DEVICE
 * memory.  Everything else is as in sy_postprocess (same workspace, same output layout: out_det [B, max_det, 7], out_index
 * [B, max_det], out_count [B]).  Per row b:
 *   1. candidates   the anchors with obj * max_c cls >= conf_thre whose arg-max class (first maximum wins) has its bit set in
 *                   class_mask.  A masked-out anchor is gone BEFORE the NMS: it suppresses nothing, in either mode.
 *   2. order        score descending, ties by ascending anchor index (the 64-bit sort key of sy_postprocess).  With
 *                   max_candidates = k > 0 only the first k entries of that order remain.
 *   3. class-aware  (flags bit 0 clear) exactly what sy_postprocess returns for a prediction tensor that holds only the
 *                   remaining candidates' anchors: the class offset unit max_coord + 1 is taken over the REMAINING candidates
 *                   (with a cut: a second reduction behind the sort), not over everything that passed the confidence filter.
 *   4. agnostic     (flags bit 0 set) the same walk with offset 0 — torchvision.ops.nms on the raw corner boxes, as
 *                   yolox.utils.postprocess(class_agnostic=True) calls it.  The output rows still carry the arg-max class and
 *                   its class_conf.
 *   5. max_det      the output is the first max_det rows of the uncapped kept list; out_count = min(kept, max_det).  The serial
 *                   walk stops as soon as that many boxes survive (later chunks could only append).  Entries of out_det /
 *                   out_index past out_count are unspecified.
 *   6. default row  {the thresholds, flags 0, both caps 0, every class bit set} gives, bit for bit, det / index / count of
 *                   sy_postprocess with those thresholds.  An all-zero record (no class bit) gives count 0.
 * SY_ERR_UNSUPPORTED for num_classes > 128 and, as sy_postprocess, for A above the LDS sort limit (16384). */
typedef struct sy_det_policy {      /* 40 bytes, one per batch row, DEVICE memory */
    float    conf_thre;             /* candidate iff obj * class_conf >= conf_thre */
    float    nms_thre;              /* a later box is suppressed iff IoU > nms_thre with an earlier kept box */
    int32_t  flags;                 /* bit 0: class-agnostic NMS (no per-class coordinate offset) */
    int32_t  max_candidates;        /* > 0: only the best max_candidates candidates enter the NMS; 0: all */
    int32_t  max_det;               /* > 0: at most this many detections are written (clamped to the launch's max_det); 0: the launch's */
    int32_t  reserved;              /* 0 */
    uint32_t class_mask[4];         /* bit c % 32 of word c / 32: class c is reported (num_classes <= 128) */
} sy_det_policy;
#define SY_DET_AGNOSTIC 1
SY_API int sy_postprocess_rows(const float* pred, int B, int A, int num_classes, const sy_det_policy* rows,
                               int max_det, float* out_det, int32_t* out_index, int32_t* out_count,
                               void* workspace, void* stream);

/* Optimizer + EMA step of one training iteration in one launch.  Replaces
 * `scaler.step(optimizer)` + `ema_model.update(model)` (exps/train_utils/double_trainer.py:115-119):
 * torch.optim.SGD(momentum, nesterov=True) semantics per entry — d = g*grad_scale; d += weight_decay*p;
 * buf = first_step ? d : momentum*buf + d; d += momentum*buf; p -= lr*lr_mult*d — then yolox ModelEMA:
 * ema = ema_decay*ema + (1-ema_decay)*p on the UPDATED p.  g == NULL: EMA only (BatchNorm running statistics);
 * buf == NULL: no momentum; ema == NULL: no EMA.  grad_scale folds GradScaler's 1/scale and the 1/world_size of the
 * gradient all-reduce.  chunk0 = prefix sum of ceil(n/1024) over the preceding entries; `entries` is DEVICE memory. */
typedef struct sy_optim_entry {
    float* p;
    const float* g;
    float* buf;
    float* ema;
    int64_t n;
    float weight_decay;
    float lr_mult;
    int32_t chunk0;
    int32_t reserved;
} sy_optim_entry;
SY_API int sy_sgd_ema_step(const sy_optim_entry* entries, int n_entries, int total_chunks, float lr, float momentum,
                           float grad_scale, float ema_decay, int first_step, void* stream);

/* ---- dynamic loss scaling without a host read -----------------------------------------------------------------
 * Replaces `self.scaler.scale(loss).backward(); self.scaler.step(self.optimizer); self.scaler.update()` of the reference's
 * --fp16 trainer (exps/train_utils/double_trainer.py:113-119) on the fused path: torch.amp.GradScaler's rule, with its state in
 * DEVICE memory.  Every entry point below takes a device POINTER to the state and reads it inside the kernel: a launch tape
 * stores argument values, so a scale passed by value would be frozen at recording time; a pointer is read anew at every replay.
 * One iteration:  sy_tal_loss_scaled (gradients = scale x true gradients)  ->  backward pass  ->  [all-reduce]  ->
 * sy_grad_nonfinite  ->  sy_sgd_ema_step_scaled  ->  sy_loss_scale_update.  Added to ABI 7 (nothing existing changed). */
typedef struct sy_scaler_state {
    float scale;                /* the loss scale S the next sy_tal_loss_scaled multiplies d_raw by                      */
    float inv_scale;            /* (float)(1.0 / (double)S), as GradScaler.unscale_ computes it; kept by sy_loss_scale_update */
    int32_t growth_tracker;     /* consecutive taken steps since the last change of S (GradScaler._growth_tracker)       */
    int32_t found_inf;          /* set to 1 by sy_grad_nonfinite, read by sy_sgd_ema_step_scaled, cleared by the update  */
    int32_t steps_taken;        /* iterations whose parameter update was applied                                         */
    int32_t steps_skipped;      /* iterations skipped because a gradient was inf / nan                                   */
    int32_t reserved[2];
} sy_scaler_state;
/* found_inf = 1 if any gradient element of the table (entries with g != NULL; same table and chunk0 prefix as
 * sy_sgd_ema_step) is +-inf or nan; denormals and FLT_MAX are finite.  One read of the gradients, nothing else written. */
SY_API int sy_grad_nonfinite(const sy_optim_entry* entries, int n_entries, int total_chunks, void* scaler_state, void* stream);
/* sy_sgd_ema_step with grad_scale = extra_scale * state->inv_scale (extra_scale: 1/world_size when the caller has not divided
 * yet) and the parameter / momentum half applied only when state->found_inf == 0; the EMA half runs either way, on the
 * (possibly unchanged) parameter — the reference calls ema_model.update after a skipped scaler.step too.  There is no first_step
 * flag (the host cannot know whether step 0 was skipped): momentum buffers must start ZEROED, 0*momentum + d == d. */
SY_API int sy_sgd_ema_step_scaled(const sy_optim_entry* entries, int n_entries, int total_chunks, float lr, float momentum,
                                  float extra_scale, float ema_decay, const void* scaler_state, void* stream);
/* GradScaler.update(): found_inf ? (S *= backoff, tracker = 0, ++steps_skipped)
 *                                : (++steps_taken; ++tracker == growth_interval ? (S *= growth if that is finite, tracker = 0) : -);
 * then found_inf = 0 and inv_scale recomputed.  One single-thread launch. */
SY_API int sy_loss_scale_update(void* scaler_state, float growth_factor, float backoff_factor, int growth_interval, void* stream);

/* Per-step weight staging: the nn.Parameters stay OIHW fp32 (the optimizer's master copy,
 * exps/train_utils/double_trainer.py:114-119); ONE launch re-derives, for every convolution of the step, the
 * layouts the MFMA kernels read.  Entry: a source block w[co_n][ci_n][taps] fp32 written as rows r0..r0+co_n of
 *   packed   [R][taps][CI]       forward / weight-gradient operand (K-contiguous), CI >= ci_n (zero padded once)
 *   packed_t [CI][taps][R_t]     data-gradient operand, element [ci][tap][r0 + co]
 *   frag / frag_t                the same two matrices in SY_TILE_WR fragment order
 *                                [rows/32][channels/BK][taps][2][2][32][EPC]  (BK = 64 bytes of channels)
 * Any destination may be NULL.  Several entries may target one destination (reg + obj predictors share a matrix).
 * Padding rows / channels are never written: allocate destinations zeroed.  `entries` is DEVICE memory. */
typedef struct sy_pack_entry {
    const float* w;
    void* packed;
    void* packed_t;
    void* frag;
    void* frag_t;
    int32_t co_n, ci_n, taps, r0, R, R_t, CI, dtype;
    int32_t tile0;              /* prefix sum over the preceding entries of ceil(co_n/32) * ceil(ci_n/32) */
    int32_t reserved;
} sy_pack_entry;
/* total_tiles = the prefix sum over ALL entries (one workgroup per 32x32 tile); taps <= 9. */
SY_API int sy_pack_weights(const sy_pack_entry* entries, int n_entries, int total_tiles, void* stream);

/* SEGMENTS (nseg >= 1): the two frames of a pair pass through the shared backbone separately in the reference, so each
 * BatchNorm normalises them with separate batch statistics (dfp_pafpn.py:120-165).  Here both frames run in ONE launch
 * per layer: segment s owns rows [s*pixels, (s+1)*pixels) of every activation view (`pixels` = rows PER segment,
 * `count` likewise), its own statistics [s][copies][C] / sums [s][copies][2][C] and its own affine / mean / invstd
 * [s][C]; gamma, beta, dgamma, dbeta are shared.  sy_conv2d's stat_segments splits its pixel range the same way.
 * nseg = 1 is an ordinary single-call BatchNorm.
 *
 * Training-mode BatchNorm helpers around sy_conv2d(stat_sum/stat_sqsum).
 * Replaces nn.BatchNorm2d in training mode (momentum/eps patched by init_yolo, cfgs/<name>.py:40-44).
 * sy_bn_finalize: every array is one of its own — scale / shift / mean / invstd / running_* overlap neither each other nor
 * sum / sqsum / gamma / beta (the kernel takes them as __restrict__); above 64 rows, rows [0, 32) of sum / sqsum are overwritten
 * with the folded totals. */
SY_API int sy_bn_finalize(const float* sum, const float* sqsum, int C, int copies, double count, const float* gamma,
                   const float* beta, float eps, float momentum, float* running_mean,
                   float* running_var, float* scale, float* shift, float* mean, float* invstd,
                   int nseg, void* stream);
/* Running-statistics update of MANY BatchNorm modules in one launch, from the same replica arrays sy_bn_finalize
 * folds (pass running_mean = NULL there).  Entry i describes one nn.BatchNorm2d and the 1 or 2 calls it received
 * this step IN CALL ORDER (the backbone / neck modules are called once per frame, current frame first —
 * exps/model/dfp_pafpn.py:120-165): for each call, running = (1 - momentum) * running + momentum * batch_stat
 * with the unbiased variance, exactly torch.nn.functional.batch_norm(training=True).  `entries` is DEVICE memory. */
typedef struct sy_bn_running_entry {
    float* running_mean;
    float* running_var;
    const float* sum[2];        /* [copies][C] replica arrays of call 0 / call 1 (call 1 NULL when calls == 1) */
    const float* sqsum[2];
    double count[2];            /* elements per channel of each call */
    int32_t C, copies, calls;
    float momentum;
    int32_t ld;                 /* elements between consecutive replicas (0 = C): > C when the module's channels are a slice of a
                                   wider statistics array (sibling convolutions stacked into one launch) */
    int32_t reserved;
    int64_t* num_batches_tracked; /* NULL, or the module's counter: += calls (nn.BatchNorm2d increments it once per training-mode
                                   forward; the shared backbone / neck modules are called once per frame) — ABI 7 */
} sy_bn_running_entry;
SY_API int sy_bn_running_update(const sy_bn_running_entry* entries, int n_entries, int max_C, void* stream);
/* sy_bn_finalize + sy_bn_silu_apply in one launch (the training forward of every BaseConv: nn.BatchNorm2d in training mode
   followed by nn.SiLU, yolox BaseConv.forward; one kernel boundary less on the critical path per layer).  Statistics
   [nseg][copies][C] as sy_conv2d's epilogue leaves them, count = elements per channel per segment; scale / shift / mean /
   invstd [nseg][C] are OUTPUTS (the backward pass reads them); running statistics: sy_bn_running_update.  C must have a
   divisor <= 64 that is a multiple of the 16-byte chunk (every width of the reference's models has). */
SY_API int sy_bn_finalize_apply(const float* sum, const float* sqsum, int copies, double count, const float* gamma,
                                const float* beta, float eps, float* scale, float* shift, float* mean, float* invstd,
                                const void* y, int ldy, const void* res, int ldr, void* out, int ldo, int64_t pixels, int C,
                                int dtype, int nseg, void* stream);

/* a = silu(scale*y + shift) [+ res], y raw conv output; views as in sy_conv2d. */
SY_API int sy_bn_silu_apply(const void* y, int ldy, const float* scale, const float* shift, const void* res,
                     int ldr, void* out, int ldo, int64_t pixels, int C, int dtype, int nseg, void* stream);
/* Backward of (BN-train + SiLU): reduce pass then apply pass.
 * reduce: sums[r][0][c] += sum dz, sums[r][1][c] += sum dz*xhat over replica r = workgroup % copies,
 * with dz = da * silu'(scale*y+shift). */
SY_API int sy_bn_silu_bwd_reduce(const void* y, int ldy, const void* da, int ldda, const float* scale,
                                 const float* shift, const float* mean, const float* invstd, float* sums,
                                 int copies, int64_t pixels, int C, int dtype, int nseg, void* stream);
/* apply: dy = gamma*invstd*(dz - S0/M - xhat*S1/M) with S = sums folded over its `copies` replicas
 * ([copies][2][C]); optionally dgamma += S1, dbeta += S0.  dres (optional): the gradient view of the residual input of
 * y = silu(bn(conv)) + res (Bottleneck shortcut, DFP add): dres = da, or dres += da when (dres_accumulate & 1) — the same
 * pass that already reads da (replaces a separate sy_view_copy).  dres_accumulate & 2: dgamma / dbeta are accumulated with
 * atomics even for nseg == 1 (the two frames of a pair go through separate launches on different streams).
 * dres_accumulate & 4: row 1 of `sums` holds the raw moment sum dz*y as a data gradient's fused reduce leaves it (SY_EPI_BNR);
 * converted here: sum dz*xhat = invstd * (sum dz*y - mean * sum dz). */
SY_API int sy_bn_silu_bwd_apply(const void* y, int ldy, const void* da, int ldda, const float* scale,
                                const float* shift, const float* mean, const float* invstd,
                                const float* gamma, const float* sums, int copies, void* dy, int lddy,
                                int64_t pixels, int C, float* dgamma, float* dbeta, void* dres, int lddres,
                                int dres_accumulate, int dtype, int nseg, void* stream);
/* LIVE ROWS of the backward sums.  The exact mode sizes `sums` for the reduce cap (768 rows per segment); one reduce launch
 * writes only the rows its own workgroups map to — the prefix [0, min(grid.x, copies)) of each segment — and leaves the rest
 * +0.0f.  The library reports grid.x from the launch's own geometry and the apply pass folds only those rows: the same additions
 * in the same order as the fold over all rows (x + 0.0f == x), so every bit of the result is unchanged.
 * Added to ABI 7 (nothing existing changed).
 * sy_bn_bwd_reduce_live_rows: *rows = grid.x of sy_bn_silu_bwd_reduce(pixels, C, dtype, nseg) under the cap in force NOW
 *   (sy_bn_grid_caps); no stream, nothing is launched.  The caller takes min(rows, copies).
 * sy_bn_silu_bwd_apply_live: sy_bn_silu_bwd_apply whose replica fold stops at row `live` (1 <= live <= copies; one live row
 *   needs no fold launch; 0 = all rows through the original fold). */
SY_API int sy_bn_bwd_reduce_live_rows(int64_t pixels, int C, int dtype, int nseg, int32_t* rows);
SY_API int sy_bn_silu_bwd_apply_live(const void* y, int ldy, const void* da, int ldda, const float* scale,
                                     const float* shift, const float* mean, const float* invstd,
                                     const float* gamma, const float* sums, int copies, int live, void* dy, int lddy,
                                     int64_t pixels, int C, float* dgamma, float* dbeta, void* dres, int lddres,
                                     int dres_accumulate, int dtype, int nseg, void* stream);

/* SimOTA assignment + Trend-Aware loss, forward and gradient, for a whole batch, no host sync.
 * raw [B, A, 5+nc] fp32 raw head logits (reg4, obj, cls); labels/support [B, max_labels, 5] fp32 rows
 * (cls, cx, cy, w, h) zero padded; level_h/w/stride describe the anchor grid (level-major, row-major).
 * Outputs: d_raw [B, A, 5+nc] = d total_loss / d raw; losses[8] = total, 5*iou, l1, conf, cls,
 * num_fg/num_gt, num_fg, num_gt (device); optional fg_mask [B, A] int32; optional d_pad [B, A, 16] in `pad_dtype` (SY_DT_*,
 * num_classes <= 8): the same gradient as columns [reg 4 | obj | 5..7 untouched | cls nc | rest untouched] — the operand layout
 * of the prediction convolutions' data / weight gradients, so that no repacking pass stands between the loss and the backward.
 * Replaces TALHead.get_losses / get_assignments / dynamic_k_matching (exps/model/tal_head.py:262-712)
 * and autograd's backward over them. */
SY_API int64_t sy_tal_loss_workspace_bytes(int B, int A, int max_gt);
SY_API int sy_tal_loss(const float* raw, int B, int A, int num_classes, const float* labels,
                       const float* support, int max_labels, const int32_t* level_h,
                       const int32_t* level_w, const float* level_stride, int nlevels, float gamma,
                       float ignore_thr, float ignore_value, int use_l1, float* d_raw, float* losses,
                       int32_t* fg_mask, void* workspace, void* d_pad, int pad_dtype, void* stream);
/* The same launches with the loss scale folded in (GradScaler.scale(loss).backward(), double_trainer.py:113-114): every element
 * of d_raw and d_pad is multiplied by scaler_state->scale (device sy_scaler_state; in fp32, before d_pad's conversion) where it
 * is written; losses[0..7] stay the TRUE loss.  scaler_state == NULL: sy_tal_loss, bit for bit. */
SY_API int sy_tal_loss_scaled(const float* raw, int B, int A, int num_classes, const float* labels,
                              const float* support, int max_labels, const int32_t* level_h,
                              const int32_t* level_w, const float* level_stride, int nlevels, float gamma,
                              float ignore_thr, float ignore_value, int use_l1, float* d_raw, float* losses,
                              int32_t* fg_mask, void* workspace, void* d_pad, int pad_dtype, const void* scaler_state,
                              void* stream);

/* Assignment of the LAST sy_tal_loss call on `workspace` (same B, A, max_labels): matched_gt [B, A] int32 = index of the matched
 * ground truth of every anchor, -1 for background; matched_iou [B, A] fp32 = its IoU (either may be NULL).  The reference's
 * get_assignments returns the same pair for the foreground anchors (exps/model/tal_head.py:559-600); diagnostics and parity tests. */
SY_API int sy_tal_loss_assignment(const void* workspace, int B, int A, int max_labels, int32_t* matched_gt,
                                  float* matched_iou, void* stream);

/* Workgroup caps of the BatchNorm row kernels (grid-stride maps over pixel rows: results do not depend on them, except that the
 * backward reduce's cap is the number of replica rows the exact mode sizes its sums for): caps4 = {sy_bn_silu_apply,
 * sy_bn_finalize_apply, sy_bn_silu_bwd_reduce, sy_bn_silu_bwd_apply}.  set4 (may be NULL): entries > 0 replace the cap, others keep
 * it; get4 (may be NULL) receives the caps in force afterwards.  Process-wide; defaults 2048 / 2048 / 768 / 1024 (or SY_BN_*_BLOCKS
 * in the environment, read at first use).  Takes no stream: nothing is launched (ABI 7; replaces an import-time environment write). */
SY_API int sy_bn_grid_caps(const int32_t* set4, int32_t* get4);

/* Zero fill of rows x row_bytes bytes at pitch_bytes (all multiples of 4; rows == 1: one dense run): the clears of a training
 * step — statistics / gradient arenas, the not-yet-written channel ranges of a gradient buffer before an accumulating data
 * gradient (autograd's zero-initialised .grad accumulation) — as launches of the plan's own tape instead of ATen fills (ABI 7). */
SY_API int sy_zero_rows(void* ptr, int64_t rows, int64_t row_bytes, int64_t pitch_bytes, void* stream);

/* elementwise helpers on views: out (+)= in */
SY_API int sy_view_copy(const void* in, int ldi, void* out, int ldo, int64_t pixels, int C, int dtype,
                 int accumulate, void* stream);

/* ---- per-stream DFP state of a batched streaming tick (many cameras, one on_pipe plan) ------------------------------
 * Stand in, per batch row, for the `buffer` hand-over of dfp_pafpn.py:211-228: a camera's previous pre-fusion PAN outputs
 * live in slot s of a dense pool [n_slots][H][W][C] per level.  row_slot (int32 [B]) and row_first (uint8 [B]) are DEVICE
 * tables read inside the kernels — a launch tape replays argument values, the tables' CONTENT is read anew at every replay
 * (the mechanism of sy_scaler_state): row_slot[b] < 0 (or >= n_slots) = row b carries no frame this tick, row_first[b] != 0 =
 * row b starts a sequence.  Views as in sy_conv2d: ld = pixel pitch, bs = batch stride, both in elements; every 16-byte piece
 * must be aligned (pointers, C, ld and bs x element size multiples of 16), else SY_ERR_ARG.  Any dtype (pure data movement).
 * Added to ABI 7 (nothing existing changed).
 *
 * sy_stream_state_gather, one level (dfp_pafpn.py:211-214 per row): sup[b] <- pool[row_slot[b]] when the row has a slot and
 * does not start a sequence, else cur[b] (node 'star': the frame fuses with itself; inactive rows too, so that nothing
 * uninitialised is read). */
SY_API int sy_stream_state_gather(const void* cur, int ld_cur, int64_t cur_bs, const void* pool, int n_slots, void* sup,
                                  int ld_sup, int64_t sup_bs, int B, int H, int W, int C, const int32_t* row_slot,
                                  const uint8_t* row_first, int dtype, void* stream);
/* sy_stream_state_scatter, all levels in one launch (dfp_pafpn.py:226-228, `buffer_` kept for the next frame, per row):
 * pool_k[row_slot[b]] <- cur_k[b] for every level k of the table and every row with a slot; other rows write nothing.
 * `levels` is HOST memory (n_levels <= 8), validated and copied into the launch.  A slot must not appear in two rows. */
typedef struct sy_stream_level {
    const void* cur;        /* this level's pre-fusion PAN output view [B, H, W, C]           */
    void* pool;             /* dense [n_slots, H, W, C]                                       */
    int64_t bs;             /* batch stride of `cur`, elements                                */
    int32_t H, W, C, ld;    /* ld = pixel pitch of `cur`, elements                            */
} sy_stream_level;
SY_API int sy_stream_state_scatter(const sy_stream_level* levels, int n_levels, int n_slots, int B, const int32_t* row_slot,
                                   int dtype, void* stream);

/* ---- per-stream tracking and forecasting behind the NMS (many cameras, one tick) -----------------------------------
 * Stand in, per batch row, for the reference's streaming post-processing step (sAP/forecast/pps_forecast_kf.py with
 * --forecast-before-assoc, sAP/track/__init__.py::iou_assoc, sAP/forecast/__init__.py::extrap_clean_up): a constant-velocity
 * Kalman filter per track over ltwh boxes in camera coordinates, greedy IoU association of a tick's detections (in the order
 * sy_postprocess delivers them: descending score) with the predicted tracks of the same class, and the clipped forecast of
 * every track `horizon` frames ahead.  A camera's tracks live in slot s of the pools of sy_track_state, the slot of a batch
 * row is row_slot[b] as in sy_stream_state_gather (the same DEVICE tables; row_first[b] != 0 restarts the slot: no tracks,
 * ids from 0), and what varies per tick and row is the DEVICE table `ticks`.  At most max_tracks detections of a row are
 * used; the ones beyond (the lowest scores) are dropped.  Fresh ids are next_id++ in detection order (the reference advances
 * its counter twice when nothing matches).  All arithmetic fp32, no atomics: bit-reproducible.  Added to ABI 7 (nothing
 * existing changed). */
typedef struct sy_track_tick {      /* 32 bytes of DEVICE memory per batch row                                           */
    int32_t dt_frames;              /* frames since this stream's previous tick (ignored where row_first is set)        */
    float horizon;                  /* forecast distance of the output, frames                                          */
    float img_w, img_h;             /* the stream's camera size: the forecast is clipped to [0, img_w] x [0, img_h]      */
    float divisor;                  /* det[..., :4] / divisor = camera coordinates                                      */
    int32_t reserved[3];
} sy_track_tick;
typedef struct sy_track_query {     /* 16 bytes of DEVICE memory per forecast entry                                      */
    int32_t slot;                   /* < 0 or >= n_slots: the entry reports 0 boxes                                      */
    float horizon, img_w, img_h;
} sy_track_query;
typedef struct sy_track_params {    /* HOST memory, copied into the launch: constants of a detector's life              */
    float match_iou_th;             /* a pair may match from this IoU on                      (reference: 0.3)           */
    float r, q, p_init;             /* R = r I, Q = dt^2 q I, P of a fresh track = p_init I   (reference: 10, 1, 100)    */
    int32_t min_size;               /* a forecast box is kept from int(w) * int(h) >= min_size (reference: 75)           */
    int32_t reserved[3];
} sy_track_params;
#define SY_TRACK_MAX_TRACKS 256     /* the compiled maximum of sy_track_state::max_tracks                                */
typedef struct sy_track_state {     /* HOST memory, copied into the launch; the pools are dense DEVICE tensors, T = max_tracks:
                                       lane i of the kernel owns track i, so the track index is the fastest one          */
    float* x;                       /* [n_slots][8][T]   l, t, w, h and their velocities per frame                       */
    float* P;                       /* [n_slots][36][T]  upper triangle of the 8 x 8 covariance, row-major               */
    float* score;                   /* [n_slots][T]      obj * class_conf of the detection the track was last built from */
    int32_t* label;                 /* [n_slots][T]                                                                      */
    int32_t* id;                    /* [n_slots][T]                                                                      */
    int32_t* hdr;                   /* [n_slots][4]      n (live tracks), n_matched (the first n_matched tracks were matched
                                                         at their last rebuild: only they move in a forecast), next_id, 0 */
    int32_t n_slots, max_tracks;
} sy_track_state;
/* sy_track_update, one launch per tick (B workgroups): det [B, max_det, 7] / cnt [B] as sy_postprocess writes them.  Per row
 * with a slot: reset (row_first), predict by dt_frames, associate, rebuild the slot's track list (matched pairs first, then the
 * unmatched detections as fresh tracks; unmatched tracks are dropped; cnt == 0 keeps the predicted tracks), store, forecast to
 * `horizon`: out [B, T, 6] = x1, y1, x2, y2, score, label of the surviving tracks in track order, out_id [B, T], out_cnt [B].
 * A row without a slot (row_slot < 0 or >= n_slots) writes nothing but out_cnt[b] = 0. */
SY_API int sy_track_update(const float* det, const int32_t* cnt, int B, int max_det, const int32_t* row_slot,
                           const uint8_t* row_first, const sy_track_tick* ticks, const sy_track_state* state,
                           const sy_track_params* params, float* out, int32_t* out_id, int32_t* out_cnt, void* stream);
/* sy_track_forecast: the forecast step alone for n entries of the DEVICE table `queries` (the state is only read): out
 * [n, T, 6], out_id [n, T], out_cnt [n] as above. */
SY_API int sy_track_forecast(const sy_track_query* queries, int n, const sy_track_state* state, const sy_track_params* params,
                             float* out, int32_t* out_id, int32_t* out_cnt, void* stream);

/* ---- COCO-style scoring of detections on the device (AP / AR, the sAP numbers) ---------------------------------------
 * Stands in for pycocotools' COCOeval on boxes, as the reference calls it (sAP/det/__init__.py::eval_ccf,
 * exps/evaluators/onex_stream_evaluator.py): computeIoU + evaluateImg per (image, class) in sy_score_match, accumulate in
 * sy_score_accumulate.  A scorer state is ONE device allocation of sy_score_state_bytes(num_classes, capacity):
 *   int32 used[C] (records appended per class; may run past capacity once the overflow counter is set), int32 npig[C][4]
 *   (non-ignored ground truths per class and area range), int32 overflow (records dropped for want of room), padding to a
 *   multiple of 32 bytes, then C arenas of `capacity` records of 32 bytes:
 *   uint32 score bits (float32, >= 0) | uint32 seq = image * 128 + rank | uint64 matched | uint64 ignored | int32 rank | int32 0
 *   with bit (a * n_thr + t) of matched / ignored = evaluateImg's dtMatches != 0 / dtIgnore at area range a, threshold t.
 * All IoU, precision and recall arithmetic is IEEE double in COCOeval's operation order on the thresholds the HOST supplies
 * (np.linspace values, np.spacing(1)): results equal a float64 numpy restatement bit for bit, whatever order the workgroups
 * ran in (integer atomics only; a record's position in its arena carries no meaning).  Added to ABI 7 (nothing existing
 * changed). */
#define SY_SCORE_MAX_THR 16         /* IoU thresholds                                                                    */
#define SY_SCORE_MAX_AREA 4         /* area ranges                                                                       */
#define SY_SCORE_MAX_MAXDET 4       /* maxDets entries, each in 1..SY_SCORE_MAX_DET                                      */
#define SY_SCORE_MAX_REC 128        /* recall thresholds (ascending)                                                     */
#define SY_SCORE_MAX_DET 100        /* detections kept per (image, class): the best by score, ties by input row          */
#define SY_SCORE_MAX_GT 256         /* the compiled maximum of max_gt (ground truths per image)                          */
#define SY_SCORE_LAYOUT_NMS 0       /* det [B, max_det, 7]: x1, y1, x2, y2, obj, class_conf, class; score = obj * class_conf (fp32) */
#define SY_SCORE_LAYOUT_TRACK 1     /* det [B, max_det, 6]: x1, y1, x2, y2, score, label (sy_track_update's out)          */
#define SY_SCORE_LAYOUT_XYWH 2      /* det [B, max_det, 6]: x, y, w, h, score, label (COCO result rows)                  */
typedef struct sy_score_params {    /* HOST memory, copied into the launch                                               */
    int32_t n_thr, n_rec, n_area, n_maxdet;
    int32_t maxdet[SY_SCORE_MAX_MAXDET];
    double eps;                     /* np.spacing(1)                                                                      */
    double iou_thr[SY_SCORE_MAX_THR];
    double area_lo[SY_SCORE_MAX_AREA], area_hi[SY_SCORE_MAX_AREA];   /* both ends inclusive                               */
    double rec_thr[SY_SCORE_MAX_REC];
} sy_score_params;
/* bytes of a state / of the workspace of sy_score_accumulate (16 bytes per record slot, the capacity rounded up to a power of
 * two); -1 for sizes out of range (num_classes in 1..65535, capacity >= 1, num_classes * capacity <= 2^30) */
SY_API int64_t sy_score_state_bytes(int num_classes, int capacity);
SY_API int64_t sy_score_workspace_bytes(int num_classes, int capacity);
/* clears the counters of a state (the arenas need no clearing) */
SY_API int sy_score_reset(void* state, int num_classes, int capacity, void* stream);
/* One batch of images, B x num_classes workgroups of one wave: row b is image number image_base + b (< 2^25).  det / cnt [B]
 * in `layout`; divisor: NULL or float32 [B], each coordinate is divided by divisor[b] in float32; then w = x2 - x1, h = y2 - y1
 * in float32, everything else in double.  gt [B, max_gt, 7] float64: x, y, w, h, class, iscrowd, area; gt_cnt int32 [B].
 * B == 0 does nothing. */
SY_API int sy_score_match(const float* det, const int32_t* cnt, int B, int max_det, int layout, const float* divisor,
                          const double* gt, const int32_t* gt_cnt, int max_gt, int64_t image_base,
                          const sy_score_params* params, void* state, int num_classes, int capacity, void* stream);
/* precision [n_thr, n_rec, num_classes, n_area, n_maxdet] and recall [n_thr, num_classes, n_area, n_maxdet] (float64, every
 * entry written; -1 where a class has no non-ignored ground truth in the area range) from the state, which is only read.
 * One workgroup per class sorts the class's records in `workspace` (sy_score_workspace_bytes).  overflow: NULL, or one double
 * that receives the state's overflow counter (placed behind recall it travels in the caller's one copy of the results). */
SY_API int sy_score_accumulate(const void* state, int num_classes, int capacity, const sy_score_params* params, void* workspace,
                               double* precision, double* recall, double* overflow, void* stream);

/* ---- drawing a tick's boxes, class labels and track ids into camera surfaces, in place --------------------------------
 * The opposite direction of sy_frames_u8_pack_surfaces: ONE launch writes the outlines and label tabs of every batch row's
 * box list into that row's BGR / RGB / NV12 / P010 surface in DEVICE memory, from the device tensors the tick produced — no
 * host read.  Geometry and style are per-row table data (sy_overlay_row, DEVICE memory); the grid depends on (B, Hmax, Wmax)
 * only, so one recorded launch serves any table contents.  Added to ABI 7 (nothing existing changed).
 *
 * Box lists.  layout 0: boxes = det [B, max_list, 7] (x1, y1, x2, y2, obj, class_conf, class; score = obj * class_conf in
 *   fp32), sy_postprocess's output.  layout 1: boxes = [B, max_list, 6] (x1, y1, x2, y2, score, label) with ids [B, max_list],
 *   sy_track_update's output.  cnt [B] is the live length; row b looks at its first
 *       n = min(cnt[b], max_list, SY_OVERLAY_MAX_BOXES, row.max_boxes when > 0)       (cnt < 0 counts as 0)
 *   entries.  SY_OVERLAY_MAX_BOXES = 256 is what a workgroup stages in LDS.
 * Palette.  palette [num_classes][8] bytes: B, G, R, text value (0 or 255), Y, U, V, text luma (16 or 235).  The kernel does no
 *   colour conversion: BGR / RGB surfaces take bytes 0..2 (RGB: in the order R, G, B) and a glyph pixel takes byte 3 in all
 *   three channels; NV12 / P010 take byte 4 as luma and (5, 6) as (U, V), a glyph pixel takes byte 7 as luma and (128, 128).
 * Labels.  class_text [num_classes][8]: glyph codes, 0xFF ends a name (NULL: no names).  glyphs [64][8]: an 8 x 8 bitmap font,
 *   code c = ASCII 32 + c, one byte per glyph row, the MSB is the left pixel; a code in 64..254 is drawn blank.  A box whose
 *   class is outside [0, num_classes) (NaN included) takes class 0's colours and has no name.
 *
 * The rendering rule (t = thickness clamped to 1..16, s = text_scale clamped to 0..4; all arithmetic on coordinates is fp32
 * IEEE without contraction, then integer):
 * 1. Rectangle.  With r(c) = floor(c / divisor + 0.5):  X1 = r(x1), Y1 = r(y1), X2 = r(x2) - 1, Y2 = r(y2) - 1, inclusive.
 *    A box is skipped when any c or c / divisor + 0.5 is not finite, when X2 < X1 or Y2 < Y1, or when its score is below
 *    min_score or NaN.  All of this is decided before clipping.  (r(c) is clamped to +-2^30 before it becomes an integer.)
 * 2. Outline.  The pixels of [X1, X2] x [Y1, Y2] that are not in [X1 + t, X2 - t] x [Y1 + t, Y2 - t]: a box narrower than 2 t
 *    is filled.
 * 3. Label tab (s > 0).  The string is the class name, then — when there is a suffix — a space and the suffix.  flags bit 0
 *    (SY_OVERLAY_ID; ignored when ids == NULL): the suffix is the decimal digits of id mod 100000 (the non-negative
 *    remainder, no leading zeros).  Otherwise flags bit 1 (SY_OVERLAY_SCORE): min(max(int(100 * score), 0), 99) as two
 *    digits, then '%' (100 * score in fp32, int() truncates).  Neither: the name alone.  A string of L glyphs (L <= 14; L == 0:
 *    no tab) has a tab 8 s L pixels wide and 8 s high with its left edge at X1, on the rows Y1 - 8 s .. Y1 - 1 directly
 *    above the box, or — when Y1 - 8 s < 0 — inside it on the rows Y1 .. Y1 + 8 s - 1.  The tab is filled with the class
 *    colour; every set font bit is an s x s block of the text value.
 * 4. Precedence.  Everything is opaque: a pixel takes the colour of the LOWEST list index k whose tab or outline covers it —
 *    inside k's tab the glyph value or the fill, else the outline colour.  Lists come in descending score, so the best box
 *    ends on top.  Nothing is blended, so nothing depends on the order of writes.
 * 5. Clipping.  Drawing is clipped to [0, Ws) x [0, Hs).  (Hs <= Hmax and Ws <= Wmax is the caller's duty: the launch has no
 *    workgroups for tiles beyond Hmax x Wmax, what lies there is not drawn.)
 * 6. NV12 / P010.  Luma as above.  A chroma sample (one (U, V) pair per 2 x 2 luma block) is written iff at least one of its
 *    four luma pixels is covered, and takes the (U, V) of the first covered one in raster order (x, y), (x + 1, y),
 *    (x, y + 1), (x + 1, y + 1).  P010 stores every sample v as the little-endian word v << 8 (bytes 0, v): read back by
 *    sy_frames_u8_pack_surfaces' high-byte rule it is the same 8-bit sample.
 * 7. Untouched bytes.  No byte the rule leaves uncovered is written at all: uncovered pixels, the bytes between a row's
 *    payload and its pitch, padded luma rows, anything between the planes.  Drawing in place costs only what is drawn.
 *
 * Kernel shape: a gather.  A workgroup of 256 threads owns one SY_OVERLAY_TILE_H x SY_OVERLAY_TILE_W tile of one row's surface
 * (a wavefront's stores are runs of one surface row; in the two-plane formats a thread owns one 2 x 2 block with its chroma
 * sample), resolves the row's first n boxes (one per thread), compacts — order kept — those whose rectangle or tab meets the
 * tile into LDS and leaves without touching memory when none does.  No atomics; no thread writes a pixel it does not own.
 *
 * Status: SY_ERR_ARG for rows / boxes / cnt / palette / glyphs == NULL, B / max_list / num_classes / Hmax / Wmax <= 0, a
 * layout other than 0 or 1; SY_ERR_UNSUPPORTED for num_classes > 128 or B > 65535.  The host cannot see the table: a
 * descriptor no surface can have (plane0 == NULL, Hs or Ws <= 0, an unknown format, odd NV12 / P010 sizes, a pitch — either
 * one — below the row's bytes, a negative chroma_stride) is skipped on the device, never written through. */
#define SY_OVERLAY_MAX_BOXES 256    /* list entries a launch looks at per row: the LDS staging cap                        */
#define SY_OVERLAY_TILE_W 64        /* pixels: the tile of one workgroup                                                   */
#define SY_OVERLAY_TILE_H 16
#define SY_OVERLAY_ID 1             /* sy_overlay_row::flags                                                               */
#define SY_OVERLAY_SCORE 2
typedef struct sy_overlay_row {     /* 64 bytes, one per batch row, DEVICE memory                                          */
    uint8_t* plane0;                /* BGR / RGB pixels or the luma plane; NULL or Hs == 0: nothing is drawn for this row  */
    uint8_t* plane1;                /* NV12 / P010 chroma plane; NULL: plane0 + row_stride * Hs.  Ignored for BGR / RGB    */
    int32_t Hs, Ws, row_stride, chroma_stride;   /* as sy_frame_surf (chroma_stride 0 = row_stride)                        */
    int32_t format;                 /* SY_PIX_BGR / RGB / NV12 / P010                                                      */
    float divisor;                  /* box coordinate / divisor = surface pixel (detections: the row's in_scale; tracks: 1) */
    float min_score;                /* boxes with score < min_score are not drawn                                          */
    int32_t max_boxes;              /* > 0: at most the first max_boxes list entries are looked at; 0: the launch's cap    */
    int32_t thickness;              /* outline width in pixels, 1..16 (clamped)                                            */
    int32_t text_scale;             /* 0: no label tab; 1..4: glyph cells of 8*scale x 8*scale pixels (clamped)            */
    int32_t flags;                  /* SY_OVERLAY_ID: the label ends with the track id; SY_OVERLAY_SCORE: with the score   */
    int32_t reserved;               /* 0 */
} sy_overlay_row;
SY_API int sy_overlay_draw(const sy_overlay_row* rows, int B, int Hmax, int Wmax, const float* boxes, int layout, int max_list,
                           const int32_t* ids, const int32_t* cnt, const uint8_t* palette, const uint8_t* class_text,
                           int num_classes, const uint8_t* glyphs, void* stream);

/* ---- cropping a tick's boxes out of camera surfaces: a dense batch of fixed-size crops for a second stage ----------------
 * The gather that mirrors sy_overlay_draw: the box lists the tick left in DEVICE memory become out [capacity, 3, Ch, Cw], every
 * kept box resampled to Ch x Cw from its batch row's BGR / RGB / NV12 / P010 surface at the camera's own resolution — no host
 * read.  Geometry and filters are per-row table data (sy_crop_row, DEVICE memory); both launches' grids depend on (capacity, Ch,
 * Cw) only, so one recorded call serves any table and list contents.  Added to ABI 7 (nothing existing changed).
 *
 * boxes / layout / max_list / ids / cnt: exactly as sy_overlay_draw (layout 0: det [B, max_list, 7], score = obj * class_conf in
 * fp32; layout 1: [B, max_list, 6] with ids [B, max_list] or NULL).  Row b looks at its first
 *     n = min(cnt[b], max_list, SY_CROP_MAX_BOXES)                                          (cnt < 0 counts as 0)
 * entries.
 *
 * The rule (all arithmetic on coordinates is fp32 IEEE without contraction up to the integer rectangle, integer from there on):
 * 1. Rectangle.  Rule 1 of sy_overlay_draw: with r(c) = floor(c / divisor + 0.5) (clamped to +-2^30),  X1 = r(x1), Y1 = r(y1),
 *    X2 = r(x2) - 1, Y2 = r(y2) - 1, inclusive.  An entry is skipped when any c or c / divisor + 0.5 is not finite, when X2 < X1
 *    or Y2 < Y1, when its score is below min_score or NaN, when its class is NaN, outside [0, 128) or (as an integer, truncated)
 *    has no bit in class_mask (bit c & 31 of word c >> 5), or when this unpadded rectangle does not meet [0, Ws) x [0, Hs).
 * 2. Padding.  With W = X2 - X1 + 1 and px = (W * pad_q8 + 128) >> 8:  X1 -= px, X2 += px; the same in y with H.  (pad_q8 is
 *    clamped to 0..256.)
 * 3. Aspect (flags & SY_CROP_KEEP_ASPECT; otherwise each axis is stretched on its own).  With the padded W and H: when
 *    W * Ch < H * Cw,  W' = ceil(H * Cw / Ch), X1 -= (W' - W) >> 1, X2 = X1 + W' - 1 (an odd growth puts the extra pixel on the
 *    right); when W * Ch > H * Cw the same in y with H' = ceil(W * Ch / Cw) (the extra pixel at the bottom).
 *    With or without the flag, an entry whose W or H now exceeds SY_CROP_MAX_SIDE is skipped.
 * 4. Sampling: half-pixel centres, bilinear, 8-bit weights, edge replicate inside the rectangle.  For output column j:
 *    n = (2 j + 1) W - Cw, d = 2 Cw, x0 = floor(n / d), f = n - x0 d, wx = (256 f + Cw) / d (integer division); the two taps are
 *    the columns X1 + clamp(x0, 0, W - 1) and X1 + clamp(x0 + 1, 0, W - 1).  Rows likewise with i, H, Ch: wy and two tap rows.
 *    Per channel:  v = ((256 - wx)(256 - wy) v00 + wx (256 - wy) v01 + (256 - wx) wy v10 + wx wy v11 + 32768) >> 16.
 * 5. Taps.  A tap outside [0, Ws) x [0, Hs) is (fill[0], fill[1], fill[2]) as (B, G, R).  Inside it is the pixel's (B, G, R): BGR
 *    as stored, RGB swapped, NV12 by the per-pixel conversion of sy_frames_u8_pack_fmt (nearest chroma: pair x >> 1 of chroma
 *    row y >> 1; BT.601 limited range in the fixed point stated there), P010 the same on the HIGH bytes.  Conversion is per tap,
 *    before interpolation: the crop equals the BGR rule applied to the converted frame.  No byte between a row's payload and its
 *    pitch, in padded luma rows or between the planes is ever read.
 * 6. Output.  Planar [slot][3][Ch][Cw]; planes are B, G, R, or R, G, B with SY_CROP_RGB_OUT.  SY_CROP_DT_U8 stores v; the float
 *    types store (float(v) - mean3[c]) * scale3[c] computed in fp32 — a subtraction, then a multiplication, c the OUTPUT plane;
 *    NULL = 0 / 1 — fp16 / bf16 rounded to nearest even.
 * 7. Slots.  Kept entries are numbered with rows ascending, list index ascending within a row (no atomics: the same inputs
 *    give the same slots).  A row contributes at most max_crops kept entries (max_crops > 0; the cap counts KEPT entries, the
 *    entries skipped before them do not use it up).  Slot s < capacity receives its crop, out_index[s] = (batch row, list
 *    index, id or -1 when ids == NULL, class) and out_rect[s] = (X1, Y1, X2, Y2) of the sampled rectangle (after 2 and 3; it
 *    may leave the surface).  out_count = (min(total, capacity), total).  Slots at or past out_count[0] are not written at all,
 *    in none of the three outputs.
 * 8. Descriptors and status.  A descriptor no surface can have (the list of sy_overlay_draw: plane0 == NULL, Hs or Ws <= 0, an
 *    unknown format, odd NV12 / P010 sizes, a pitch — either one — below the row's bytes, a negative chroma_stride) keeps
 *    nothing and nothing of it is read.  SY_ERR_ARG for rows / boxes / cnt / out / out_index / out_rect / out_count == NULL,
 *    B / max_list / capacity <= 0, a layout other than 0 or 1, unknown flag bits, an unknown out_dtype; SY_ERR_UNSUPPORTED for
 *    Cw % 8 != 0, Ch or Cw outside 8..512, B > 1024.
 *
 * Kernel shape: two launches.  Plan: ONE workgroup of 256 threads walks the rows in order, thread k resolves list entry k, a
 * ballot per wave and the four wave counts through LDS number the kept entries; it writes out_index, out_rect and out_count —
 * which are also the gather's plan, there is no workspace.  Gather: grid (capacity, tiles of 256 x 8 output pixels); a workgroup
 * whose slot is at or past out_count[0] leaves at once; the per-column (tap, tap, wx) triples go through LDS; a thread owns 8
 * consecutive output columns of one row and writes each plane with one 8- / 16- / 32-byte run. */
#define SY_CROP_MAX_BOXES 256       /* list entries a launch looks at per row                                              */
#define SY_CROP_MAX_SIDE 16384      /* a padded rectangle wider or taller than this is skipped                              */
#define SY_CROP_KEEP_ASPECT 1       /* flags                                                                               */
#define SY_CROP_RGB_OUT 2           /* output planes in R, G, B order (default B, G, R)                                    */
#define SY_CROP_DT_U8 3             /* out_dtype besides SY_DT_BF16 / SY_DT_F16 / SY_DT_F32                                */
typedef struct sy_crop_row {        /* 72 bytes, one per batch row, DEVICE memory                                          */
    const uint8_t* plane0;          /* BGR / RGB pixels or the luma plane; NULL or Hs == 0: the row keeps nothing          */
    const uint8_t* plane1;          /* NV12 / P010 chroma plane; NULL: plane0 + row_stride * Hs.  Ignored for BGR / RGB    */
    int32_t Hs, Ws, row_stride, chroma_stride;   /* as sy_frame_surf (chroma_stride 0 = row_stride)                        */
    int32_t format;                 /* SY_PIX_BGR / RGB / NV12 / P010                                                      */
    float divisor;                  /* box coordinate / divisor = surface pixel (detections: the row's in_scale; tracks: 1) */
    float min_score;                /* entries with score < min_score are skipped                                          */
    int32_t max_crops;              /* > 0: at most this many KEPT entries of the row; <= 0: no row cap                    */
    int32_t pad_q8;                 /* context padding per side in 1/256 of the box side, 0..256 (clamped)                 */
    uint8_t fill[4];                /* B, G, R of a tap outside the surface; byte 3 = 0                                    */
    uint32_t class_mask[4];         /* as sy_det_policy: bit c & 31 of word c >> 5 set = class c is kept                   */
} sy_crop_row;
SY_API int sy_crop_gather(const sy_crop_row* rows, int B, const float* boxes, int layout, int max_list, const int32_t* ids,
                          const int32_t* cnt, int Ch, int Cw, int flags, int out_dtype, const float* mean3, const float* scale3,
                          void* out, int capacity, int32_t* out_index, int32_t* out_rect, int32_t* out_count, void* stream);

/* ---- redacting a tick's boxes in camera surfaces: pixelate or fill what was detected, in place ----------------------------
 * What sy_overlay_draw cannot do — outlines and tabs hide nothing: ONE launch makes the objects of every batch row's box list
 * unrecognisable in that row's BGR / RGB / NV12 / P010 surface in DEVICE memory, from the device tensors the tick produced — no
 * host read.  Geometry and style are per-row table data (sy_redact_row, DEVICE memory); the grid depends on (B, Hmax, Wmax)
 * only, so one recorded launch serves any table and list contents.  Added to ABI 7 (nothing existing changed).
 *
 * boxes / layout / max_list / cnt: exactly as sy_overlay_draw (layout 0: det [B, max_list, 7], score = obj * class_conf in fp32;
 * layout 1: [B, max_list, 6]).  Row b looks at its first
 *     n = min(cnt[b], max_list)                                                              (cnt < 0 counts as 0)
 * entries.  There is NO cap of 256: coverage is a union, the kernel walks the list in chunks of 256 (its LDS staging size) and
 * ORs.  A redaction that drops entry 257 is a leak.
 *
 * The rule (all arithmetic on coordinates is fp32 IEEE without contraction up to the integer rectangle, 64-bit integers from
 * there on):
 * 1. Rectangle.  Rule 1 of sy_overlay_draw with the class filter of sy_crop_gather: with r(c) = floor(c / divisor + 0.5)
 *    (clamped to +-2^30),  X1 = r(x1), Y1 = r(y1), X2 = r(x2) - 1, Y2 = r(y2) - 1, inclusive.  An entry is skipped when any c or
 *    c / divisor + 0.5 is not finite, when X2 < X1 or Y2 < Y1, when its score is below min_score or NaN, when its class is NaN,
 *    outside [0, 128) or (as an integer, truncated) has no bit in class_mask (bit c & 31 of word c >> 5).  All of this is
 *    decided before padding and clipping: a box off the surface whose padding reaches into it is redacted there.
 * 2. Padding.  Rule 2 of sy_crop_gather: with W = X2 - X1 + 1 and px = (W * pad_q8 + 128) >> 8:  X1 -= px, X2 += px; the same
 *    in y with H.  (pad_q8 is clamped to 0..256.)
 * 3. Shape.  SY_REDACT_RECT: every pixel of the padded rectangle is COVERED.  SY_REDACT_ELLIPSE: with the padded W and H, pixel
 *    (x, y) of the rectangle is covered iff
 *        ((2 x + 1) - (2 X1 + W))^2 H^2 + ((2 y + 1) - (2 Y1 + H))^2 W^2 <= W^2 H^2
 *    — the pixel's centre lies inside the inscribed ellipse.  An entry whose W or H exceeds SY_REDACT_MAX_SIDE is covered as a
 *    rectangle: the products stay inside 64 bits, and nothing is ever skipped for being large.
 * 4. Union and clipping.  A pixel of [0, Ws) x [0, Hs) is covered iff any kept entry covers it; the result does not depend on
 *    the order of the list.  (Hs <= Hmax and Ws <= Wmax is the caller's duty, as for sy_overlay_draw.)
 * 5. SY_REDACT_FILL.  A covered pixel takes `fill`: BGR bytes 0..2, RGB the same bytes in the order R, G, B, luma byte 4.
 * 6. SY_REDACT_PIXELATE.  Cells are aligned to the SURFACE's origin, not to the box: cell (i, j) is the pixels
 *    x in [i cell, min((i + 1) cell, Ws) - 1], y in [j cell, min((j + 1) cell, Hs) - 1].  With n the cell's pixel count and S_c
 *    the sum of the ORIGINAL values of channel c over the whole cell, covered or not, every covered pixel of the cell takes
 *    (S_c + (n >> 1)) / n (integer division) in each channel.  A cell without a covered pixel is neither read nor written.
 *    cell is 4, 8, 16 or 32; anything else makes the descriptor impossible (rule 9).
 * 7. NV12 / P010.  Luma by rules 5 and 6.  A chroma sample is covered iff at least one of its four luma pixels is (rule 6 of
 *    sy_overlay_draw).  FILL gives it (fill[5], fill[6]); PIXELATE averages U and V separately over the chroma samples of the
 *    same cell — a (cell / 2) x (cell / 2) block clipped to the plane — with the same rounding.  P010 reads the HIGH byte of
 *    every sample and writes v << 8 (bytes 0, v): the low bits of a redacted sample are gone too.
 * 8. Untouched bytes.  Rule 7 of sy_overlay_draw, word for word: no byte the rule leaves uncovered is written at all —
 *    uncovered pixels, the bytes between a row's payload and its pitch, padded luma rows, anything between the planes — and none
 *    of those outside the payload is read.
 * 9. Descriptors and status.  A descriptor no surface can have (the list of sy_overlay_draw: plane0 == NULL, Hs or Ws <= 0, an
 *    unknown format, odd NV12 / P010 sizes, a pitch — either one — below the row's bytes, a negative chroma_stride; and here a
 *    cell other than 4, 8, 16, 32, a mode or a shape outside 0..1) is skipped on the device, never written through.
 *    SY_ERR_ARG for rows / boxes / cnt == NULL, B / max_list / Hmax / Wmax <= 0, a layout other than 0 or 1;
 *    SY_ERR_UNSUPPORTED for B > 65535 or more than 65535 tile rows.
 *
 * Kernel shape: a gather.  A workgroup of 256 threads owns one SY_REDACT_TILE_H x SY_REDACT_TILE_W tile of one row's surface;
 * both sides are multiples of the largest cell, so every cell lies in exactly one tile: a workgroup reads only pixels it owns,
 * all of them before a barrier, and writes behind it — no workgroup reads a byte another one writes, which is what makes
 * pixelation in place safe (a blur, whose window crosses tiles, would not be).  It compacts the entries that meet its tile chunk
 * by chunk, leaves without touching pixel memory when none does, sums flagged cells with integer LDS adds (no order), then
 * writes.  In the two-plane formats a thread owns 2 x 2 luma blocks with their chroma samples. */
#define SY_REDACT_TILE_W 64         /* pixels: the tile of one workgroup; both sides multiples of 32                       */
#define SY_REDACT_TILE_H 32
#define SY_REDACT_MAX_SIDE 16384    /* an ellipse wider or taller than this is covered as its rectangle                    */
#define SY_REDACT_PIXELATE 0        /* sy_redact_row::mode                                                                 */
#define SY_REDACT_FILL 1
#define SY_REDACT_RECT 0            /* sy_redact_row::shape                                                                */
#define SY_REDACT_ELLIPSE 1
typedef struct sy_redact_row {      /* 88 bytes, one per batch row, DEVICE memory                                          */
    uint8_t* plane0;                /* BGR / RGB pixels or the luma plane; NULL or Hs == 0: nothing is redacted in this row */
    uint8_t* plane1;                /* NV12 / P010 chroma plane; NULL: plane0 + row_stride * Hs.  Ignored for BGR / RGB    */
    int32_t Hs, Ws, row_stride, chroma_stride;   /* as sy_frame_surf (chroma_stride 0 = row_stride)                        */
    int32_t format;                 /* SY_PIX_BGR / RGB / NV12 / P010                                                      */
    float divisor;                  /* box coordinate / divisor = surface pixel (detections: the row's in_scale; tracks: 1) */
    float min_score;                /* entries with score < min_score (or NaN) are skipped                                 */
    int32_t pad_q8;                 /* growth per side in 1/256 of the box side, 0..256 (clamped)                          */
    int32_t mode;                   /* SY_REDACT_PIXELATE / SY_REDACT_FILL                                                 */
    int32_t cell;                   /* pixelation cell in luma pixels: 4, 8, 16 or 32 (checked in both modes)              */
    int32_t shape;                  /* SY_REDACT_RECT / SY_REDACT_ELLIPSE                                                  */
    int32_t reserved;               /* 0 */
    uint8_t fill[8];                /* B, G, R, 0, Y, U, V, 0: the fill colour in both spaces; the kernel converts nothing */
    uint32_t class_mask[4];         /* as sy_det_policy: bit c & 31 of word c >> 5 set = class c is redacted               */
} sy_redact_row;
SY_API int sy_redact(const sy_redact_row* rows, int B, int Hmax, int Wmax, const float* boxes, int layout, int max_list,
                     const int32_t* cnt, void* stream);

/* backward of sy_resize_nearest (scatter-add into the source grid) */
SY_API int sy_resize_nearest_bwd(const void* dout, int N, int Ho, int Wo, int C, int lddo, int64_t dobs,
                          void* din, int Hi, int Wi, int lddi, int64_t dibs, int accumulate,
                          int dtype, void* stream);
/* backward of sy_spp_pool: dbuf holds grads of the 4 slices; routes pooled grads to their arg-max into slice 0 */
SY_API int sy_spp_pool_bwd(void* dbuf, const void* argmax, int N, int H, int W, int C, int ld, int64_t bs,
                    int dtype, void* stream);

/* Second half of a split-K convolution (sy_conv_desc::k_splits): y[p][c] = act(scale[c] * sum_z part[z][p][c] + shift[c]) (+ res),
 * part = fp32 [splits][pixels][C] dense, act per `epilogue` (SY_EPI_LINEAR | SY_EPI_SILU), y / res views in `dtype` with pixel
 * strides ldy / ldr.  The partials are summed in split order (deterministic). */
SY_API int sy_splitk_epilogue(const float* part, int splits, int64_t pixels, int C, const float* scale, const float* shift,
                              const void* res, int ldr, void* y, int ldy, int dtype, int epilogue, void* stream);

/* ---- small fp32 helpers of the backward plan ---------------------------------------------------------------------
 * sy_rows_add_f32: dst[r][0..cols) += src[r][0..cols) for r < rows (row pitches in elements); zero_src != 0 zeroes the
 * source behind the read (a scratch the next accumulating sy_conv2d_wgrad launch reuses).  Used where a weight gradient is
 * computed in a padded layout (Focus stem: 12 real + 4 zero channels).
 * sy_pred_grad_fold: the parameter gradients of one head level's three 1x1 prediction convs (autograd of
 * tal_head.py:167-171): bias gradients (+)= column sums of d_raw over the level's B x rows anchors (deterministic two-stage
 * sum), weight gradients (+)= the [reg 0-3 | obj 4] / [cls] rows of `scratch` ([2][scratch_rows][ld] fp32, filled by two
 * sy_conv2d_wgrad launches), scratch zeroed behind the read.  `workspace`: sy_pred_grad_fold_workspace_floats floats. */
SY_API int sy_rows_add_f32(float* dst, int64_t ldd, float* src, int64_t lds, int rows, int cols, int zero_src, void* stream);
SY_API int64_t sy_pred_grad_fold_workspace_floats(int num_classes);
SY_API int sy_pred_grad_fold(const float* d_raw, int B, int64_t batch_stride, int rows, int num_classes, float* scratch,
                             int scratch_rows, int ld, int cin, float* g_reg, float* g_obj, float* g_cls, float* gb_reg, float* gb_obj, float* gb_cls,
                             float* workspace, void* stream);

/* ---- native launch tapes ---------------------------------------------------------------------------------------
 * Replaces the per-iteration Python dispatch of the reference trainer / evaluator loops
 * (exps/train_utils/double_trainer.py:95-131: ~2000 eager ops per train_one_iter; sAP/streamyolo/streamyolo_det.py:176-184
 * per streamed frame).  A plan's step is a fixed launch list: sy_tape_begin() opens a recording on the calling thread —
 * every kernel launch of every entry point above still executes, and its closure (kernel, grid, block, LDS size, argument
 * values) is appended; sy_tape_mark() appends stream-control entries between them; sy_tape_end() returns the tape.
 * sy_tape_replay() re-issues the list from C on the given streams, starting at entry *pos: it returns at a BREAK entry (and
 * at BUCKET entries when stop_buckets != 0) with *pos = the entry to resume at, *stop_kind / *stop_arg = that entry and
 * *stop_on_side = 1 if the launch cursor is on the side stream; at the end *stop_kind = SY_TAPE_END.  side_stream == NULL
 * (or == main_stream): one-stream replay, the stream marks are ignored.  A tape holds raw pointers: it is valid while the
 * buffers it was recorded over live.  Not thread safe per tape; recordings do not nest. */
enum { SY_TAPE_END = -1, SY_TAPE_LAUNCH = 0,
       SY_TAPE_SIDE = 1,     /* side stream waits for main; cursor -> side                                    */
       SY_TAPE_FORK = 2,     /* side stream waits for main; cursor unchanged                                  */
       SY_TAPE_SIDE_NW = 3,  /* cursor -> side, no new dependency                                             */
       SY_TAPE_MAIN = 4,     /* cursor -> main; arg >= 0: event on side = "ring slot `arg` is free again"      */
       SY_TAPE_ACQUIRE = 5,  /* main waits for the event of ring slot `arg` (if one is pending)               */
       SY_TAPE_JOIN = 6,     /* main waits for everything issued on side                                      */
       SY_TAPE_BREAK = 7,    /* return to the caller (host-side snippet `arg` runs there)                     */
       SY_TAPE_BUCKET = 8,   /* gradient bucket `arg` is final on every stream                                */
       /* plans with more than two chains (sy_tape_replay_n: streams[0] = main, [1] = side, [2..] = further chains) */
       SY_TAPE_CUR = 9,      /* cursor -> stream `arg`, no new dependency                                     */
       SY_TAPE_DEP = 10,     /* stream (arg >> 4) records an event, stream (arg & 15) waits for it            */
       SY_TAPE_SLOT_DONE = 11,   /* event on the CURRENT stream = "this stream's readers of ring slot `arg` are done"; a slot keeps
                                    one such event PER STREAM, the first one after an acquisition starts a new set      */
       SY_TAPE_ACQUIRE_CUR = 12  /* the CURRENT stream waits for every event of slot `arg`'s set recorded on ANOTHER stream
                                    (the set stays: several chains may acquire their part of one slot)                  */ };
SY_API void* sy_tape_begin(void);
SY_API int sy_tape_mark(int kind, int arg);
SY_API void* sy_tape_end(void);
SY_API int sy_tape_size(const void* tape, int* n_entries, int* n_launches);
/* events recorded / stream-waits issued by the last (or current) replay pass of `tape` */
SY_API int sy_tape_counters(const void* tape, int* n_events, int* n_waits);
SY_API int sy_tape_replay(void* tape, void* main_stream, void* side_stream, int* pos, int stop_buckets, int* stop_kind,
                          int* stop_arg, int* stop_on_side);
/* the same over n_streams (1..8) streams; *stop_stream = index of the cursor stream at a BREAK / BUCKET return.  A chain index
 * beyond n_streams (or a NULL entry) runs on streams[0]: a three-chain tape replays correctly on one or two streams. */
SY_API int sy_tape_replay_n(void* tape, void* const* streams, int n_streams, int* pos, int stop_buckets, int* stop_kind,
                            int* stop_arg, int* stop_stream);
SY_API void sy_tape_free(void* tape);

SY_API const char* sy_version(void);
SY_API int sy_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* STREAMYOLO_HIP_H */
