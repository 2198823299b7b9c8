/* minsdtf_hip_resampler.h — C ABI of libminsdtf_hip_resampler.so: the attention of an IP-Adapter "plus" Resampler (the Perceiver
 * resampler of IP-Adapter's resampler.py; diffusers' IPAdapterPlusImageProjection), the seventh library beside libminsdtf_hip.so,
 * libminsdtf_hip_ext.so, libminsdtf_hip_dynthresh.so, libminsdtf_hip_control.so, libminsdtf_hip_ipadapter.so and
 * libminsdtf_hip_vision.so.  The rest of the resampler (LayerNorm, the projections, the exact GELU, the residual GEMMs) runs on the
 * core's and the vision library's entry points; minsdtf_amd/engine.py emit_ip_resampler is the launch plan.
 *
 * The six other ABIs are frozen at their entry points.  The conventions are the core's: raw DEVICE pointers, caller-owned memory
 * (nothing is allocated or freed), stream-ordered work that never synchronises and is capturable into a hipGraph, `int` return
 * codes - 0 on success, a negative MSD_E_* code of minsdtf_hip.h for an argument error (nothing was launched), a positive
 * hipError_t from the launch - and msdr_last_error() for the text.  The memory contract is the core's too: no entry point writes
 * a byte outside the extents of its outputs, and no value outside the extents (padding columns included) influences a result.
 * No atomics, no scratch memory, no workspace; every order of sums depends on the shapes alone, so a sample's bits do not depend on
 * its batch.
 */
#ifndef MINSDTF_HIP_RESAMPLER_H
#define MINSDTF_HIP_RESAMPLER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDR_ABI_VERSION 1
#define MSDR_HEAD_DIM 64     /* the one head size that is built (anything else: MSD_E_UNSUPPORTED = -3) */
#define MSDR_MAX_QUERIES 16  /* n: the latent queries, which are also the keys of the second segment */
#define MSDR_MAX_TX 272      /* t_x: the keys of the first segment (257 for the CLIP ViT-H/14 tower) */
#define MSDR_KEY_TILE 16     /* keys of one score tile: tile j holds the key rows 16 j .. 16 j + 15 (see below) */

typedef void* msdr_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the functions marked MSDR_API below are its WHOLE dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define MSDR_API __attribute__((visibility("default")))
#else
#define MSDR_API
#endif

MSDR_API int msdr_abi_version(void);
MSDR_API const char* msdr_last_error(void);

/* ------------------------------------------------------------------------------------------
 * msdr_perceiver_attention — the attention of one PerceiverAttention layer in ONE launch over two key segments that stay where
 * their GEMMs wrote them (nothing is concatenated or copied).  For sample b, head h, query i < n, with D = 64:
 *
 *     s[j]  = scale * sum_c q[b][i][64 h + c] * key_j[64 h + c]             j = 0 .. t_x + n - 1, the x keys first:
 *                 key_j = k_x[b][j] for j < t_x,  k_l[b][j - t_x] behind them;  v_j likewise from vt_x / vt_l
 *     m     = max_j s[j]                                                     over ALL t_x + n keys, before any exponential
 *     p[j]  = exp2(s[j] - m)                l = sum_j p[j]
 *     out[b][i][64 h + d] = bf16(sum_j bf16(p[j] * (1 / l)) * v_j[64 h + d])
 *
 * The softmax is base 2: the caller folds log2(e) into `scale` (or into q, with scale = 1).  The pinned arithmetic: the dot products
 * run on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, c ascending in two steps of 32; the product with `scale` is one fp32
 * multiplication; all t_x + n scores of a row are held on chip, so m is the true row maximum and there is NO online rescale;
 * exp2 is the hardware's v_exp_f32; 1 / l is an IEEE division; p[j] * (1 / l) is rounded to bf16 ONCE (round to nearest even) and
 * the products with V accumulate in fp32 on the same MFMA, keys ascending in steps of 32; ONE more rounding to bf16, at the store.
 * Key rows: the x keys sit at rows 0 .. t_x - 1 and the latent keys at rows t8 .. t8 + n - 1, t8 = roundup8(t_x); a row of neither
 * segment has probability exactly 0 by its INDEX.  A workgroup is one (sample, head) and has four waves: wave w computes the score
 * tiles j = w, w + 4, ... (MSDR_KEY_TILE key rows each); the four partial maxima, then the four partial sums, are merged through LDS
 * in the order ((w0 + w1) + w2) + w3 (a lane's own sum runs over its tiles ascending, then over the four key groups of a tile in
 * the fixed order of two butterfly steps); then wave w computes the output channels 16 w .. 16 w + 15 of all queries over all keys.
 * So the order of every sum depends on (t_x, n) alone, and a sample's bits do not depend on `batch`.
 *
 * Padding: the columns >= t_x of a vt_x row and >= n of a vt_l row are padding; whatever they hold, NaN included, never reaches
 * out.  The columns >= heads * 64 of an out row are not written.  out lies apart from every input.
 * Every pointer 16-byte aligned; 1 <= n <= MSDR_MAX_QUERIES; 1 <= t_x <= MSDR_MAX_TX; batch, heads in 1 .. 65535; every ld a
 * multiple of 8; q_ld, kx_ld, kl_ld, o_ld >= heads * 64; vtx_ld >= t_x; vtl_ld >= n; scale finite: otherwise MSD_E_ARG.
 * head_dim must be 64 (MSD_E_UNSUPPORTED). */
typedef struct MsdrPerceiverAttention {
    const void* q;      /* bf16 [batch][n][q_ld]; head h at columns [64 h, 64 h + 64) */
    const void* k_x;    /* bf16 [batch][t_x][kx_ld] */
    const void* vt_x;   /* bf16 [batch][heads * 64][vtx_ld], key index contiguous */
    const void* k_l;    /* bf16 [batch][n][kl_ld] */
    const void* vt_l;   /* bf16 [batch][heads * 64][vtl_ld] */
    void* out;          /* bf16 [batch][n][o_ld] */
    float scale;
    int32_t batch, heads, head_dim, n, t_x;
    int32_t q_ld, kx_ld, vtx_ld, kl_ld, vtl_ld, o_ld;
} MsdrPerceiverAttention;
MSDR_API int msdr_perceiver_attention(const MsdrPerceiverAttention* p, msdr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSDTF_HIP_RESAMPLER_H */
