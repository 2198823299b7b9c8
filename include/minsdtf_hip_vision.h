/* minsdtf_hip_vision.h — C ABI of libminsdtf_hip_vision.so: the three steps of the CLIP ViT-H/14 vision tower that the core
 * library has no kernel for, the sixth library beside libminsdtf_hip.so, libminsdtf_hip_ext.so, libminsdtf_hip_dynthresh.so,
 * libminsdtf_hip_control.so and libminsdtf_hip_ipadapter.so.  The rest of the tower (LayerNorm, the stacked q|k|v projection,
 * attention, the residual GEMMs) runs on the core's entry points; minsdtf_amd/engine.py emit_clip_vision is the launch plan.
 *
 * The five other ABIs are frozen at their entry points.  The conventions are the core's: raw DEVICE pointers, caller-owned memory
 * (nothing is allocated or freed), stream-ordered work that never synchronises and is capturable into a hipGraph, `int` return
 * codes - 0 on success, a negative MSD_E_* code of minsdtf_hip.h for an argument error (nothing was launched), a positive
 * hipError_t from the launch - and msdv_last_error() for the text.  The memory contract is the core's too: no entry point writes
 * a byte outside the extents of its outputs, and no value outside the extents (padding columns included) influences a result.
 * No atomics, no scratch memory; every order of sums depends on the shapes alone, so a sample's bits do not depend on its batch.
 */
#ifndef MINSDTF_HIP_VISION_H
#define MINSDTF_HIP_VISION_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDV_ABI_VERSION 1
/* the one geometry that is built: ViT-H/14 (anything else in the structs below: MSD_E_UNSUPPORTED = -3) */
#define MSDV_IMAGE 224      /* picture rows / columns */
#define MSDV_PATCH 14       /* patch rows / columns, = the stride */
#define MSDV_GRID 16        /* patches per picture row / column */
#define MSDV_TOKENS 257     /* MSDV_GRID^2 patches + the class token (token 0) */
#define MSDV_WIDTH 1280     /* channels of a token */
#define MSDV_PATCH_K 588    /* MSDV_PATCH^2 * 3: columns of the patch matrix */
#define MSDV_PROJ 1024      /* columns of the image embedding */
#define MSDV_MAX_BATCH 8

typedef void* msdv_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the functions marked MSDV_API below are its WHOLE dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define MSDV_API __attribute__((visibility("default")))
#else
#define MSDV_API
#endif

MSDV_API int msdv_abi_version(void);
MSDV_API const char* msdv_last_error(void);

/* ------------------------------------------------------------------------------------------
 * msdv_patch_embed — from pixels to the input of encoder layer 0 in ONE launch: normalisation, the 14 x 14 / stride-14 patch
 * convolution, class token, position embedding and the pre-LayerNorm.  For sample b:
 *
 *     x[y][x][c]  = bf16(fma(pixels[b][y][x][c], scale[c], shift[c]))                       (the one rounding of the pixels)
 *     acc[p][n]   = sum_k x[14 py + ky][14 px + kx][c] * w[n][k]     k = (ky * 14 + kx) * 3 + c,  p = 16 py + px
 *     e[0][n]     = cls[n] + pos[0][n]              e[1 + p][n] = acc[p][n] + pos[1 + p][n]
 *     out[b][t][n] = bf16((e[t][n] - mean_t) * rstd_t * gamma[n] + beta[n])
 *
 * The patch product runs on v_mfma_f32_16x16x32_bf16 with fp32 accumulation over k ascending in steps of 32 (K is padded to 608
 * with zeros on chip: the columns >= 588 of a w row are NOT part of the product, whatever they hold).  The LayerNorm is fp32:
 * mean_t = (sum_n e) / 1280 first, then var_t = (sum_n (e - mean_t)^2) / 1280, rstd_t = 1 / sqrt(var_t + eps); never
 * E[x^2] - mean^2.  Both sums run in one fixed order (a lane's 80 values ascending, then the 16 partial sums of the token
 * ascending).  One rounding to bf16, at the store.  A workgroup owns one picture row of 16 patches (four waves of 320 columns: the
 * whole 1280-wide row stays in accumulators), one more workgroup per sample the class token.  The columns 1280 .. o_ld - 1 of an
 * out row are not written.  out lies apart from every input.
 * Every pointer 16-byte aligned; 1 <= batch <= MSDV_MAX_BATCH; w_ld a multiple of 8 and >= 592 (the first multiple of 8 that
 * holds the 588 columns); o_ld a multiple of 8 and >= 1280; eps > 0: otherwise MSD_E_ARG.  image / patch / width must be
 * 224 / 14 / 1280 (MSD_E_UNSUPPORTED). */
typedef struct MsdvPatchEmbed {
    const float* pixels;      /* fp32 [batch][224][224][3], on the 0 .. 255 scale */
    const void* w;            /* bf16 [1280][w_ld] rows (k contiguous) */
    const float* cls;         /* fp32 [1280] */
    const float* pos;         /* fp32 [257][1280] */
    const float* gamma;       /* fp32 [1280] */
    const float* beta;        /* fp32 [1280] */
    void* out;                /* bf16 [batch][257][o_ld] */
    float scale[3];           /* 1 / (255 std_c), computed by the host in float64 */
    float shift[3];           /* -mean_c / std_c */
    float eps;
    int32_t batch, image, patch, width;
    int32_t w_ld, o_ld;
} MsdvPatchEmbed;
MSDV_API int msdv_patch_embed(const MsdvPatchEmbed* p, msdv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msdv_gelu — the exact (erf) GELU of the tower's MLP, with the one rounding to bf16:
 *
 *     out[r][c] = bf16(0.5f * x * (1.0f + erff(x * 0.70710678f)))      x = in[r][c],  0 <= r < rows, 0 <= c < cols
 *
 * evaluated in fp32 exactly as written.  fc1 runs as msd_conv_gemm with its bias and an fp32 output; this launch performs the
 * rounding a fused epilogue would.  16-byte accesses: cols a multiple of 8, ld_in a multiple of 4, ld_out a multiple of 8,
 * ld_in / ld_out >= cols, both pointers 16-byte aligned, rows >= 1, rows * max(ld_in, ld_out) < 2^31.  The columns >= cols of
 * a row are neither read nor written.  out lies apart from in. */
MSDV_API int msdv_gelu(const float* in, void* out, int32_t rows, int32_t cols, int32_t ld_in, int32_t ld_out, msdv_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msdv_pool_project — the pooled head: LayerNorm of the class token, then the bias-free 1280 -> 1024 projection.  For sample b:
 *
 *     y[k]      = (x[b][k] - mean) * rstd * gamma[k] + beta[k]            fp32, NOT rounded; mean / var / rstd as above
 *     out[b][n] = sum_k y[k] * w[n][k]                                     fp32 FMAs
 *
 * Every workgroup (16 output columns of one sample) recomputes the row's statistics with the same code.  A wave owns 4 columns;
 * lane l of it takes the k = 8 (l + 64 j) + 0 .. 7, j = 0, 1, 2, ascending in one fmaf chain, then the 64 lane sums are added in
 * the fixed order of the core's wave reduction.  w is the matrix layout.py packs for `visual_projection`: w_layout 0 - bf16
 * [1024][1280] rows; w_layout 1 - the chunk-major image [1280 / 64][1024][64] of the same matrix (packing.chunk_major; what the
 * package stores, K being a multiple of 64).  Both give the same bits.
 * Every pointer 16-byte aligned; 1 <= batch <= MSDV_MAX_BATCH; x_stride (elements between two samples' rows) a multiple of 8 and
 * >= 1280; w_layout 0 or 1; eps > 0: otherwise MSD_E_ARG.  width / proj must be 1280 / 1024 (MSD_E_UNSUPPORTED).  out lies apart
 * from every input. */
typedef struct MsdvPoolProject {
    const void* x;            /* bf16: row b at x + b * x_stride elements, 1280 values */
    const float* gamma;       /* fp32 [1280] */
    const float* beta;        /* fp32 [1280] */
    const void* w;            /* bf16 [1024][1280] (w_layout 0) or [20][1024][64] (w_layout 1) */
    float* out;               /* fp32 [batch][1024] */
    int64_t x_stride;
    float eps;
    int32_t batch, width, proj, w_layout;
} MsdvPoolProject;
MSDV_API int msdv_pool_project(const MsdvPoolProject* p, msdv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSDTF_HIP_VISION_H */
