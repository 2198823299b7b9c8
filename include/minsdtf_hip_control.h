/* minsdtf_hip_control.h — C ABI of libminsdtf_hip_control.so: the ControlNet units' combine, the fourth library beside
 * libminsdtf_hip.so, libminsdtf_hip_ext.so and libminsdtf_hip_dynthresh.so.
 *
 * The three other ABIs are frozen at their entry points.  The conventions are the core's: raw DEVICE pointers, caller-owned memory
 * (nothing is allocated or freed), stream-ordered work that never synchronises and is capturable into a hipGraph, `int` return
 * codes - 0 on success, a negative MSD_E_* code of minsdtf_hip.h for an argument error (nothing was launched), a positive
 * hipError_t from the launch - and msdc_last_error() for the text.  The memory contract is the core's too: no entry point writes
 * a byte outside the extents of its outputs, and no value outside the extents influences a result.
 */
#ifndef MINSDTF_HIP_CONTROL_H
#define MINSDTF_HIP_CONTROL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDC_ABI_VERSION 1
#define MSDC_TAPS 13        /* the 12 skip connections of the UNet's down path and the mid block's output */
#define MSDC_MAX_UNITS 3
#define MSDC_CHUNK 2048     /* elements of one (tensor, row) a workgroup takes: 256 lanes x 8 */

typedef void* msdc_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the functions marked MSDC_API below are its WHOLE dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define MSDC_API __attribute__((visibility("default")))
#else
#define MSDC_API
#endif

MSDC_API int msdc_abi_version(void);
MSDC_API const char* msdc_last_error(void);

/* ------------------------------------------------------------------------------------------
 * msdc_control_combine — the residuals of up to three ControlNet units, scaled and added to the 13 skip tensors of one UNet
 * pass, in ONE launch.  For tap k, row b and element e of the row:
 *
 *     step = *step_ptr clamped to 0 .. num_steps - 1 (0 when step_ptr is NULL);  col = 0 (u) for b < rows_u, else 1 (c)
 *     s_n  = scales[step][n][k][col]
 *     v    = fp32(skip_k[b][e]);  for n = 0 .. units - 1 with s_n != 0:  v = fmaf(s_n, resid_n,k[b][e], v)
 *     skip_k[b][e] = bf16_rne(v)
 *
 * Every fmaf is single-rounded and they are taken in unit order; there is one rounding to bf16.  A unit whose scale is exactly 0
 * is NOT READ, so whatever its residual holds (NaN included) does not reach the result; a (tap, row) whose scales are all 0 is
 * neither read nor written: its bits stay.  Nothing couples two rows, so a row's bits do not depend on its batch; no LDS, no
 * atomics, no workspace; every trip count depends on the shapes alone.  The step counter is read, never written.
 * The skips are written in place and lie apart from the residuals, the table and the step counter.  Every pointer 16-byte aligned
 * (step_ptr: 4-byte); 1 <= units <= MSDC_MAX_UNITS (the residual pointers of the units behind are ignored); 1 <= rows <= 65535;
 * 0 <= rows_u <= rows; every count a positive multiple of 8; num_steps >= 1;
 * chunk_prefix[0] = 0, chunk_prefix[k + 1] = chunk_prefix[k] + ceil(count[k] / MSDC_CHUNK). */
typedef struct MsdcControlCombine {
    void* skip[MSDC_TAPS];                          /* bf16 [rows][count[k]] */
    const float* resid[MSDC_MAX_UNITS][MSDC_TAPS];  /* fp32 [rows][count[k]], read only */
    const float* scales;                            /* fp32 [num_steps][units][MSDC_TAPS][2] */
    const int32_t* step_ptr;                        /* device int32 step index, or NULL */
    int32_t count[MSDC_TAPS];                       /* elements of one row of tap k: h_k * w_k * c_k */
    int32_t chunk_prefix[MSDC_TAPS + 1];            /* workgroups per row in front of tap k; [MSDC_TAPS]: per row in all */
    int32_t rows, rows_u, units, num_steps;
} MsdcControlCombine;
MSDC_API int msdc_control_combine(const MsdcControlCombine* p, msdc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSDTF_HIP_CONTROL_H */
