/* minsdtf_hip_dynthresh.h — C ABI of libminsdtf_hip_dynthresh.so: dynamic thresholding, the third library beside
 * libminsdtf_hip.so and libminsdtf_hip_ext.so.
 *
 * The core ABI (include/minsdtf_hip.h) and the extension ABI (include/minsdtf_hip_ext.h) are frozen at their entry points.  The
 * conventions are the core's: raw DEVICE pointers, caller-owned memory (nothing is allocated or freed), stream-ordered work that
 * never synchronises and is capturable into a hipGraph, `int` return codes - 0 on success, a negative MSD_E_* code of
 * minsdtf_hip.h for an argument error (nothing was launched), a positive hipError_t from the launch - and msdt_last_error() for
 * the text.  The memory contract is the core's too: no entry point writes a byte outside the extents of its outputs, and no value
 * outside the extents influences a result.
 */
#ifndef MINSDTF_HIP_DYNTHRESH_H
#define MINSDTF_HIP_DYNTHRESH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDT_ABI_VERSION 1

typedef void* msdt_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the functions marked MSDT_API below are its WHOLE dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define MSDT_API __attribute__((visibility("default")))
#else
#define MSDT_API
#endif

MSDT_API int msdt_abi_version(void);
MSDT_API const char* msdt_last_error(void);

/* ------------------------------------------------------------------------------------------
 * msdt_dynamic_threshold — the combined noise prediction of a classifier-free-guidance step with dynamic thresholding (the
 * sd-dynamic-thresholding extension's dynthresh() with sep_feat_channels = True).  One PLANE is the P = h * w values of one
 * (sample, channel); u = eps rows [0, batch), c = eps rows [batch, 2 * batch):
 *
 *     (g, m) = scales[step][0 .. 1], step = *step_ptr clamped to 0 .. num_steps - 1 (0 when step_ptr is NULL)
 *     d = c - u;  cfg = fma(g, d, u);  mim = fma(m, d, u)
 *     mean_cfg, mean_mim = plane means;  cc = cfg - mean_cfg;  mc = mim - mean_mim
 *     measure 0 ("ad"):  mim_ref = max |mc|
 *                        cfg_ref = s[lo] + frac * (s[hi] - s[lo]),  s = the plane's |cc| sorted ascending, hi = min(lo + 1, P - 1):
 *                        an EXACT order statistic (a radix selection over the 32 key bits), torch.quantile's "linear" rule
 *     measure 1 ("std"): mim_ref = sqrt(sum mc^2 / (P - 1)),  cfg_ref = sqrt(sum cc^2 / (P - 1))
 *     startpoint 0 ("mean"), measure 0:  mx = max(mim_ref, cfg_ref);  r = clamp(cc, -mx, mx) * (mim_ref / mx) + mean_cfg
 *     startpoint 0 ("mean"), measure 1:  r = cc * (mim_ref / cfg_ref) + mean_cfg
 *     startpoint 1 ("zero"):             r = cfg * (mim_ref / cfg_ref)
 *     out = phi * r + (1 - phi) * cfg;   a plane whose divisor (mx, or cfg_ref) is exactly 0:  out = cfg
 *
 * Sums are fp32, the mean first and then the deviations from it, in an order that depends on (h, w) alone; nothing couples two
 * samples, so a sample's bits do not depend on its batch and a launch is reproducible.  Every loop's trip count depends on the
 * shape alone: a plane of NaNs gives unspecified values in that plane and nothing else.  No global atomics, no floating-point
 * atomics, no workspace.  The step counter is read, never written.
 * `out` is `eps` itself (the u rows are overwritten in place) or lies apart from all of `eps`; it lies apart from scales, params
 * and the step counter.  Every pointer 16-byte aligned (step_ptr: 4-byte); 1 <= batch <= 65535; P >= 2; n = h * w * 4 < 2^31;
 * num_steps >= 1. */
typedef struct MsdtDynamicThreshold {
    const float* eps;          /* fp32 [2 * batch][n], n = h * w * 4 (NHWC, 4 channels): the u rows, then the c rows */
    float* out;                /* fp32 [batch][n] */
    const float* scales;       /* fp32 [num_steps][2]: the cfg scale and the mimic scale of every step */
    const int32_t* step_ptr;   /* device int32 step index, or NULL */
    const void* params;        /* 32 bytes: int32 lo, int32 measure, int32 startpoint, fp32 frac, fp32 phi, 12 bytes reserved */
    int32_t batch, h, w, num_steps;
} MsdtDynamicThreshold;
MSDT_API int msdt_dynamic_threshold(const MsdtDynamicThreshold* p, msdt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSDTF_HIP_DYNTHRESH_H */
