/* minsdtf_hip_ext.h — C ABI of libminsdtf_hip_ext.so: the extension library beside libminsdtf_hip.so.
 *
 * The core ABI (include/minsdtf_hip.h) is frozen at its entry points; optional features whose kernels are not part of the plain
 * denoise step live here.  The conventions are the core's: raw DEVICE pointers, caller-owned memory (nothing is allocated or
 * freed), stream-ordered work that never synchronises and is capturable into a hipGraph, `int` return codes - 0 on success, a
 * negative MSD_E_* code of minsdtf_hip.h for an argument error (nothing was launched), a positive hipError_t from the launch -
 * and msdx_last_error() for the text.  The memory contract is the core's too: an operand described as [rows][ld] carrying
 * `cols` columns is the (rows - 1) * ld + cols elements from its base address, no entry point writes a byte outside the extents
 * of its outputs, and no value outside the extents influences a result.
 */
#ifndef MINSDTF_HIP_EXT_H
#define MINSDTF_HIP_EXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDX_ABI_VERSION 1

typedef void* msdx_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the functions marked MSDX_API below are its WHOLE dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define MSDX_API __attribute__((visibility("default")))
#else
#define MSDX_API
#endif

MSDX_API int msdx_abi_version(void);
MSDX_API const char* msdx_last_error(void);

/* ------------------------------------------------------------------------------------------
 * msdx_attention_colsum — the attention each KEY receives in a self-attention layer (self-attention guidance, Hong et al. 2023):
 *
 *     out[b][j] = (1 / heads) * sum_h sum_i softmax_j(q_h k_h^T)[i][j]          (so sum_j out[b][j] = s)
 *
 * Operands as msd_attention's in its q_prescaled form: q carries scale * log2(e), the probabilities are exp2(q.k - m_i) / l_i with
 * m_i the row maximum and l_i the row sum.  Two kernels behind the one entry: (a) one wave per (sample, head, 32 queries) walks
 * the keys in blocks of 32 and writes (m_i, l_i) to `workspace`; (b) one workgroup per (sample, 64 keys), its waves sharing the
 * heads, walks the heads and then the queries in ascending blocks of 32, recomputes the same scores on the same MFMA chain
 * (v_mfma_f32_32x32x16_bf16, keys on rows), keeps the probabilities in fp32 and adds them up per key in a fixed order.  No
 * atomics: the order of every sum depends on (heads, s) alone, so a sample's bits do not depend on its batch and a launch is
 * reproducible.  s = 1 gives exactly 1.0f.
 * head_dim = 160 only (the UNet's mid block); 1 <= s <= 4096; heads >= 1; q_ld / k_ld multiples of 8 and >= heads * head_dim;
 * every pointer 16-byte aligned; out and workspace apart from each other and from q / k. */
typedef struct MsdxAttentionColsum {
    const void* q;             /* bf16 [batch][s][q_ld] carrying heads * head_dim columns, pre-scaled by scale * log2(e) */
    const void* k;             /* bf16 [batch][s][k_ld] carrying heads * head_dim columns */
    float* out;                /* fp32 [batch][s] */
    float* workspace;          /* fp32 [batch][heads][s][2]: (row maximum, row sum); unspecified content afterwards */
    int64_t workspace_floats;  /* >= batch * heads * s * 2 */
    int32_t batch, heads, head_dim, s;
    int32_t q_ld, k_ld;
} MsdxAttentionColsum;
MSDX_API int msdx_attention_colsum(const MsdxAttentionColsum* p, msdx_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msdx_sag_degrade — the degraded latent of a self-attention-guidance step (diffusers StableDiffusionSAGPipeline.sag_masking):
 *
 *     alpha = coef[step * coef_stride], sigma = coef[step * coef_stride + 1], step = *step_ptr (0 when step_ptr is NULL)
 *     x0    = (latent - sigma * eps) / alpha
 *     blur  = 9-tap Gaussian of x0 per channel, reflect borders, separable: horizontal, then vertical, each a product and
 *             eight fused multiply-adds in ascending tap order with taps params[0..8]
 *     M     = colsum[b][(y * mh / h) * mw + (x * mw / w)] > params[9]               (integer divisions: a nearest upsample)
 *     out   = M ? fma(alpha, blur, sigma * eps) : latent                             (outside the mask: the latent's own bits)
 *
 * The step counter is read, never advanced.  h, w >= 5 (reflect padding of 4) and <= 4096; 1 <= mh <= h, 1 <= mw <= w;
 * out apart from every input; latent / eps / out 16-byte aligned, coef / colsum / params 4-byte aligned. */
typedef struct MsdxSagDegrade {
    const float* latent;       /* fp32 [batch][h][w][4] */
    const float* eps;          /* fp32 [batch][h][w][4]: the noise prediction the map came from */
    const float* coef;         /* fp32 [num_steps][coef_stride]: columns 0 and 1 are alpha_t and sigma_t */
    const int32_t* step_ptr;   /* device int32 step index (clamped to 0 .. num_steps - 1), or NULL */
    const float* colsum;       /* fp32 [batch][mh * mw]: msdx_attention_colsum's output */
    const float* params;       /* fp32 [10]: the 9 taps, then the threshold */
    float* out;                /* fp32 [batch][h][w][4] */
    int32_t batch, h, w, mh, mw;
    int32_t coef_stride, num_steps;
} MsdxSagDegrade;
MSDX_API int msdx_sag_degrade(const MsdxSagDegrade* p, msdx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSDTF_HIP_EXT_H */
