/* minsdtf_hip_ipadapter.h — C ABI of libminsdtf_hip_ipadapter.so: the decoupled cross-attention of an IP-Adapter image prompt, the
 * fifth library beside libminsdtf_hip.so, libminsdtf_hip_ext.so, libminsdtf_hip_dynthresh.so and libminsdtf_hip_control.so.
 *
 * The four other ABIs are frozen at their entry points.  The conventions are the core's: raw DEVICE pointers, caller-owned memory
 * (nothing is allocated or freed), stream-ordered work that never synchronises and is capturable into a hipGraph, `int` return
 * codes - 0 on success, a negative MSD_E_* code of minsdtf_hip.h for an argument error (nothing was launched), a positive
 * hipError_t from the launch - and msdi_last_error() for the text.  The memory contract is the core's too: no entry point writes
 * a byte outside the extents of its outputs, and no value outside the extents influences a result.
 */
#ifndef MINSDTF_HIP_IPADAPTER_H
#define MINSDTF_HIP_IPADAPTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSDI_ABI_VERSION 1
#define MSDI_LAYERS 16      /* columns of the scale table: the UNet's attention blocks in forward order (engine.PAG_LAYERS) */
#define MSDI_KEYS 96        /* keys of the one tile: roundup8(t) + n <= MSDI_KEYS */
#define MSDI_MAX_TOKENS 16  /* image tokens: 4 (base adapter) or 16 ("plus") */

typedef void* msdi_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the functions marked MSDI_API below are its WHOLE dynamic symbol table. */
#if defined(__GNUC__) || defined(__clang__)
#define MSDI_API __attribute__((visibility("default")))
#else
#define MSDI_API
#endif

MSDI_API int msdi_abi_version(void);
MSDI_API const char* msdi_last_error(void);

/* ------------------------------------------------------------------------------------------
 * msdi_attention_decoupled — cross-attention over the text context plus, decoupled from it, over the image tokens of an
 * IP-Adapter, in ONE launch.  For sample b, head h and query i:
 *
 *     step = *step_ptr clamped to 0 .. num_steps - 1 (0 when step_ptr is NULL);  sc = scales[step][layer]
 *     out = softmax2(q k^T) v + sc * softmax2(q k_ip^T) v_ip          softmax2(x)_j = 2^x_j / sum_j 2^x_j
 *
 * two independent softmaxes over the same query: the first over the t text keys, the second over the n image keys.  q carries
 * head_dim^-0.5 * log2(e), as for msd_region_attention.  The scores are fp32 sums of bf16 products; each softmax takes its own
 * true row maximum and its own fp32 row sum; a text probability is 2^(x - max_text) * (1 / sum_text), an image probability
 * 2^(x - max_ip) * (sc / sum_ip), each rounded ONCE to bf16; the output is the fp32 sum of their products with v / v_ip over all
 * t + n keys, rounded once to bf16.
 * With sc == 0 exactly the image term is dropped BEFORE anything of it is loaded: k_ip and vt_ip are NOT READ, so whatever they
 * hold (NaN included) does not reach the result, which has the bits of the same launch with any other content there.
 * Padding - the columns t .. vt_ld - 1 of a vt row, n .. vtip_ld - 1 of a vt_ip row, and every column of a q / k / k_ip / out row
 * outside the heads * head_dim it carries - may hold anything and is not written.  Nothing couples two samples or two heads, so
 * a sample's bits do not depend on its batch or on the row it occupies; no atomics, no workspace; every trip count depends on
 * the shapes alone.  The step counter and the table are read, never written.  out lies apart from every input.
 * Every pointer 16-byte aligned (step_ptr: 4-byte); head_dim 40, 80 or 160; s >= 1; t >= 1; 1 <= n <= MSDI_MAX_TOKENS;
 * roundup8(t) + n <= MSDI_KEYS; every leading dimension a multiple of 8; q_ld, k_ld, kip_ld, o_ld >= heads * head_dim;
 * vt_ld >= t; vtip_ld >= n; 0 <= layer < MSDI_LAYERS; num_steps >= 1; 1 <= batch, heads <= 65535. */
typedef struct MsdiAttentionDecoupled {
    const void* q;            /* bf16 [batch][s][q_ld] */
    const void* k;            /* bf16 [batch][t][k_ld] */
    const void* vt;           /* bf16 [batch][heads * head_dim][vt_ld] */
    const void* k_ip;         /* bf16 [batch][n][kip_ld] */
    const void* vt_ip;        /* bf16 [batch][heads * head_dim][vtip_ld] */
    void* out;                /* bf16 [batch][s][o_ld] */
    const float* scales;      /* fp32 [num_steps][MSDI_LAYERS] */
    const int32_t* step_ptr;  /* device int32 step index, or NULL */
    int32_t batch, heads, head_dim, s, t, n;
    int32_t q_ld, k_ld, vt_ld, kip_ld, vtip_ld, o_ld;
    int32_t layer, num_steps;
} MsdiAttentionDecoupled;
MSDI_API int msdi_attention_decoupled(const MsdiAttentionDecoupled* p, msdi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSDTF_HIP_IPADAPTER_H */
