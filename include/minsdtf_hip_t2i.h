/* minsdtf_hip_t2i.h — C ABI of libminsdtf_hip_t2i.so: the kernels of a T2I-Adapter (TencentARC t2iadapter_*_sd15v2; diffusers'
 * T2IAdapter "full adapter"), the eighth library beside libminsdtf_hip.so, libminsdtf_hip_ext.so, libminsdtf_hip_dynthresh.so,
 * libminsdtf_hip_control.so, libminsdtf_hip_ipadapter.so, libminsdtf_hip_vision.so and libminsdtf_hip_resampler.so.  The adapter's
 * convolutions run on the core's msd_conv_gemm; minsdtf_amd/engine.py emit_t2i_adapter is the launch plan of the network and
 * UNetVariant.t2i_site records the per-step add.
 *
 * The seven other ABIs are frozen at their entry points.  The conventions are the core's: raw DEVICE pointers, caller-owned memory
 * (nothing is allocated or freed), stream-ordered work that never synchronises and is capturable into a hipGraph, `int` return
 * codes - 0 on success, a negative MSD_E_* code of minsdtf_hip.h for an argument error (nothing was launched), a positive
 * hipError_t from the launch - and msda_last_error() for the text.  The memory contract is the core's too: no entry point writes
 * a byte outside the extents of its outputs, and no value outside the extents influences a result.  No atomics, no LDS, no scratch
 * memory, no workspace; every trip count depends on the shapes alone, and every element is computed from its own operands in a
 * pinned order, so a sample's bits do not depend on its batch.
 */
#ifndef MINSDTF_HIP_T2I_H
#define MINSDTF_HIP_T2I_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDA_ABI_VERSION 1
#define MSDA_MAX_UNITS 3   /* adapters of one job (diffusers' MultiAdapter): their terms add */
#define MSDA_SITES 4       /* the four points of the UNet's down path a full adapter feeds */
#define MSDA_CHUNK 2048    /* elements of a row that one workgroup of msda_feature_add owns (256 lanes x 8) */

typedef void* msda_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the functions marked MSDA_API below are its WHOLE dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define MSDA_API __attribute__((visibility("default")))
#else
#define MSDA_API
#endif

MSDA_API int msda_abi_version(void);
MSDA_API const char* msda_last_error(void);

/* ------------------------------------------------------------------------------------------
 * msda_feature_add — the adapters' feature of one site added to a UNet activation, in place, the same feature to every row:
 *
 *     row  = clamp(*step_ptr, 0, num_steps - 1)                  (step_ptr NULL: row 0)
 *     s_u  = scales[row][u][site]                                u = 0 .. units - 1
 *     acc  = float(x[r][e]);  for u ascending with s_u != 0:  acc = fmaf(s_u, float(feat[u][e]), acc)
 *     x[r][e] = bf16(acc)                                        ONE rounding, to nearest even
 *
 * A unit whose scale is exactly 0 is not read (its buffer may hold anything, NaN included).  When every scale of the row is 0
 * the launch neither reads nor writes x: it keeps its bits, NaN payloads included.  A workgroup owns MSDA_CHUNK elements of `n`
 * and walks the rows, so a feature element is loaded once per launch, not once per row.
 * x, feat[u < units] and scales 16-byte aligned and non-null; step_ptr 4-byte aligned or NULL; 1 <= rows <= 65535; n a positive
 * multiple of 8; 1 <= units <= MSDA_MAX_UNITS; 0 <= site < MSDA_SITES; num_steps >= 1; x apart from every feat[u], from scales
 * and from step_ptr: otherwise MSD_E_ARG. */
typedef struct MsdaFeatureAdd {
    void* x;                           /* bf16 [rows][n] */
    const void* feat[MSDA_MAX_UNITS];  /* bf16 [n] each; the entries >= units are ignored */
    const float* scales;               /* fp32 [num_steps][units][MSDA_SITES] */
    const int32_t* step_ptr;
    int32_t rows, n, units, site, num_steps;
} MsdaFeatureAdd;
MSDA_API int msda_feature_add(const MsdaFeatureAdd* p, msda_stream_t stream);

/* msda_unshuffle — PixelUnshuffle(8) of a picture and its one rounding: in fp32 [batch][h][w][cin] -> out bf16
 * [batch][h / 8][w / 8][64 cin], out[b][y][x][c * 64 + dy * 8 + dx] = bf16(in[b][8 y + dy][8 x + dx][c]) (torch's channel order).
 * in / out 16-byte aligned, non-null and apart; batch >= 1; h, w positive multiples of 8; 1 <= cin <= 4; fewer than 2^31
 * elements: otherwise MSD_E_ARG. */
MSDA_API int msda_unshuffle(const float* in, void* out, int32_t batch, int32_t h, int32_t w, int32_t cin, msda_stream_t stream);

/* msda_relu — x[i] = x[i] > 0 ? x[i] : +0 over n bf16 elements in place: +0 for every x <= 0, both zeros included; a NaN keeps
 * its bits.  x 16-byte aligned and non-null; n a positive multiple of 8: otherwise MSD_E_ARG. */
MSDA_API int msda_relu(void* x, int64_t n, msda_stream_t stream);

/* msda_avgpool2 — AvgPool2d(2, 2): in bf16 [batch][h][w][c] -> out bf16 [batch][h / 2][w / 2][c],
 * out[b][y][x][k] = bf16(((a00 + a01) + (a10 + a11)) * 0.25f) in fp32, a_ij = in[b][2 y + i][2 x + j][k]: the order is pinned, one
 * rounding.  in / out 16-byte aligned, non-null and apart; batch >= 1; h, w positive and even; c a positive multiple of 8; fewer
 * than 2^31 input elements: otherwise MSD_E_ARG. */
MSDA_API int msda_avgpool2(const void* in, void* out, int32_t batch, int32_t h, int32_t w, int32_t c, msda_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSDTF_HIP_T2I_H */
