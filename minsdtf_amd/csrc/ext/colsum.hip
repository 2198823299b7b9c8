// msdx_attention_colsum: the head-mean attention every key receives, summed over the queries (include/minsdtf_hip_ext.h has the
// formula; minsdtf_amd/sag.py is the host side of self-attention guidance).
//
// Two kernels, no atomics, no scratch memory, fp32 probabilities (there is no PV product, so nothing is rounded to bf16):
//  (a) colsum_stats_kernel: one wave per (sample, head, 32 queries).  S^T = K Q^T on v_mfma_f32_32x32x16_bf16 with the keys on the
//      rows: a lane holds ONE query's scores against 16 keys of the block (the other 16 on lane ^ 32), so the running row maximum
//      and row sum are in-lane apart from one exchange between the wave's halves per block.  Writes (m_i, l_i) per query.
//  (b) colsum_sum_kernel: one workgroup of eight waves per (sample, 64 keys): wave w owns the 32 keys of half w & 1 and the heads
//      w >> 1, (w >> 1) + 4, ... (the walk over the heads is a chain of dependent loads: four chains side by side per key half).
//      A wave walks its heads, then the queries in ascending blocks of 32, recomputes the scores with THE SAME operands on THE
//      SAME MFMA chain as (a) - so exp2(s - m) is exactly 1 where (a) found the maximum - and adds exp2(s - m_i) / l_i into 16
//      per-lane accumulators (one per key row of the lane).  At the end the partial sums of a key - 32 lanes of each of its four
//      waves - are added through LDS, head group by head group and lane by lane in ascending order, and the result is scaled by
//      1 / heads once.
// Every order depends on (heads, s) alone: a sample's bits do not depend on its batch, and a launch is reproducible.
// The operands are read straight from global memory as MFMA fragments (16 bytes per lane and k-step, 32 rows per load instruction):
// nothing is staged through LDS.  At the shapes this runs at (the UNet's mid block: s = 64 at 512 x 512, 256 at 1024 x 1024,
// d = 160) a workgroup's life is a short chain of such loads, each followed by ten MFMAs; DESIGN.md 4.14 has the measured period
// and what a staged form would save.
#include <math.h>
#include "../common.h"
#include "../../../include/minsdtf_hip_ext.h"

typedef __attribute__((ext_vector_type(16))) float f32x16;

#define CS_D 160
#define CS_KS (CS_D / 16)   // k-steps of the 32x32x16 MFMA over one head

struct CSArgs {
    const bf16_t* q;
    const bf16_t* k;
    float* out;
    float* ws;
    int heads, s, q_ld, k_ld;
    float inv_heads;
};

// fragment of row `row` (A operand: matrix row r = lane & 31; B operand: matrix column r), k = 16 ks + 8 (lane >> 5) + 0 .. 7
__device__ __forceinline__ void cs_load(const bf16_t* row, int half, bf16x8* f) {
#pragma unroll
    for (int ks = 0; ks < CS_KS; ++ks) f[ks] = *reinterpret_cast<const bf16x8*>(row + ks * 16 + 8 * half);
}

// 32 keys (rows) x 32 queries (columns): register e of a lane is key row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), query lane & 31
__device__ __forceinline__ f32x16 cs_scores(const bf16x8* kf, const bf16x8* qf) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
    for (int ks = 0; ks < CS_KS; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], acc, 0, 0, 0);
    return acc;
}
__device__ __forceinline__ int cs_row(int e, int half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

// grid: x = 32-query block, y = head, z = sample; one wave
__global__ __launch_bounds__(64) void colsum_stats_kernel(const CSArgs p) {
    const int lane = threadIdx.x, r = lane & 31, half = lane >> 5;
    const int q0 = blockIdx.x * 32, h = blockIdx.y, b = blockIdx.z, s = p.s;
    const int qi = min(q0 + r, s - 1);   // (a query past the end repeats the last one: computed, never written)
    bf16x8 qf[CS_KS], kf[CS_KS];
    cs_load(p.q + ((size_t)b * s + qi) * p.q_ld + h * CS_D, half, qf);
    float m = -INFINITY, l = 0.0f;
    for (int k0 = 0; k0 < s; k0 += 32) {
        const int ki = min(k0 + r, s - 1);
        cs_load(p.k + ((size_t)b * s + ki) * p.k_ld + h * CS_D, half, kf);
        f32x16 sc = cs_scores(kf, qf);
        float bm = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            if (k0 + cs_row(e, half) >= s) sc[e] = -INFINITY;
            bm = fmaxf(bm, sc[e]);
        }
        // the block holds at least one key, on one of the two halves: the common maximum is finite on both
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);
        float t = 0.0f;
#pragma unroll
        for (int e = 0; e < 16; ++e) t += __builtin_amdgcn_exp2f(sc[e] - mn);
        l = l * __builtin_amdgcn_exp2f(m - mn) + t;
        m = mn;
    }
    l = l + __shfl_xor(l, 32, 64);   // (a + b on one half, b + a on the other: the same bits)
    if (half == 0 && q0 + r < s)
        *reinterpret_cast<float2*>(p.ws + (((size_t)b * p.heads + h) * s + q0 + r) * 2) = make_float2(m, l);
}

#define CS_HG 4   // head groups of a workgroup: wave w walks the heads w >> 1, (w >> 1) + CS_HG, ...

// grid: x = 64-key tile, y = sample; eight waves, wave w owns keys [64 x + 32 (w & 1), + 32) and the head group w >> 1
__global__ __launch_bounds__(2 * CS_HG * 64) void colsum_sum_kernel(const CSArgs p) {
    __shared__ float red[2 * CS_HG][32][33];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, half = lane >> 5;
    const int k0 = blockIdx.x * 64 + (wave & 1) * 32, b = blockIdx.y, s = p.s;
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    if (k0 < s) {   // (wave-uniform)
        const int ki = min(k0 + r, s - 1);   // (a key past the end repeats the last one: computed, never written)
        bf16x8 qf[CS_KS], kf[CS_KS];
        for (int h = wave >> 1; h < p.heads; h += CS_HG) {
            cs_load(p.k + ((size_t)b * s + ki) * p.k_ld + h * CS_D, half, kf);
            const float2* st = reinterpret_cast<const float2*>(p.ws) + ((size_t)b * p.heads + h) * s;
            for (int q0 = 0; q0 < s; q0 += 32) {
                const int qi = min(q0 + r, s - 1);
                const bool live = q0 + r < s;
                cs_load(p.q + ((size_t)b * s + qi) * p.q_ld + h * CS_D, half, qf);
                const float2 ml = st[qi];
                const float rl = 1.0f / ml.y;
                const f32x16 sc = cs_scores(kf, qf);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float pr = __builtin_amdgcn_exp2f(sc[e] - ml.x) * rl;
                    acc[e] += live ? pr : 0.0f;
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave][cs_row(e, half)][r] = acc[e];
    __syncthreads();
    if (threadIdx.x < 64) {
        const int w2 = threadIdx.x >> 5, row = threadIdx.x & 31;
        const int key = blockIdx.x * 64 + w2 * 32 + row;
        float t = 0.0f;
        for (int g = 0; g < CS_HG; ++g)
            for (int c = 0; c < 32; ++c) t += red[2 * g + w2][row][c];
        if (key < s) p.out[(size_t)b * s + key] = t * p.inv_heads;
    }
}

static bool cs_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

extern "C" int msdx_attention_colsum(const MsdxAttentionColsum* p, msdx_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "attention_colsum: null argument");
    if (!p->q || !p->k || !p->out || !p->workspace) MSD_FAIL(MSD_E_ARG, "attention_colsum: null q / k / out / workspace");
    if (!msd_aligned16(p->q) || !msd_aligned16(p->k) || !msd_aligned16(p->out) || !msd_aligned16(p->workspace))
        MSD_FAIL(MSD_E_ARG, "attention_colsum: q / k / out / workspace must be 16-byte aligned");
    if (p->head_dim != CS_D) MSD_FAIL(MSD_E_ARG, "attention_colsum: head_dim %d (160 only)", p->head_dim);
    if (p->heads < 1 || p->heads > 64) MSD_FAIL(MSD_E_ARG, "attention_colsum: %d heads (1 .. 64)", p->heads);
    if (p->s < 1 || p->s > 4096) MSD_FAIL(MSD_E_ARG, "attention_colsum: s = %d (1 .. 4096)", p->s);
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "attention_colsum: batch %d (1 .. 65535)", p->batch);
    const int c = p->heads * CS_D;
    if (p->q_ld < c || (p->q_ld % 8) || p->k_ld < c || (p->k_ld % 8))
        MSD_FAIL(MSD_E_ARG, "attention_colsum: q_ld %d / k_ld %d (multiples of 8, at least heads * head_dim = %d)", p->q_ld, p->k_ld, c);
    const int64_t need = (int64_t)p->batch * p->heads * p->s * 2;
    if (p->workspace_floats < need)
        MSD_FAIL(MSD_E_ARG, "attention_colsum: workspace of %lld floats, %lld needed", (long long)p->workspace_floats, (long long)need);
    {   // out and workspace lie apart from each other and from the operands
        const int64_t rows = (int64_t)p->batch * p->s;
        const uintptr_t q0 = (uintptr_t)p->q, q1 = q0 + (uintptr_t)((rows - 1) * p->q_ld + c) * 2;
        const uintptr_t k0 = (uintptr_t)p->k, k1 = k0 + (uintptr_t)((rows - 1) * p->k_ld + c) * 2;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)rows * 4;
        const uintptr_t w0 = (uintptr_t)p->workspace, w1 = w0 + (uintptr_t)need * 4;
        if (cs_overlap(o0, o1, w0, w1) || cs_overlap(o0, o1, q0, q1) || cs_overlap(o0, o1, k0, k1) || cs_overlap(w0, w1, q0, q1) ||
            cs_overlap(w0, w1, k0, k1))
            MSD_FAIL(MSD_E_ARG, "attention_colsum: out / workspace overlap each other or q / k");
    }
    CSArgs a;
    a.q = reinterpret_cast<const bf16_t*>(p->q);
    a.k = reinterpret_cast<const bf16_t*>(p->k);
    a.out = p->out;
    a.ws = p->workspace;
    a.heads = p->heads;
    a.s = p->s;
    a.q_ld = p->q_ld;
    a.k_ld = p->k_ld;
    a.inv_heads = 1.0f / (float)p->heads;
    hipLaunchKernelGGL(colsum_stats_kernel, dim3((unsigned)((p->s + 31) / 32), (unsigned)p->heads, (unsigned)p->batch), dim3(64), 0, stream, a);
    MSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(colsum_sum_kernel, dim3((unsigned)((p->s + 63) / 64), (unsigned)p->batch), dim3(2 * CS_HG * 64), 0, stream, a);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
