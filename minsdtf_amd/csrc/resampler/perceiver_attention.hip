// msdr_perceiver_attention: the attention of one PerceiverAttention layer of an IP-Adapter "plus" Resampler
// (include/minsdtf_hip_resampler.h has the operands and the pinned arithmetic, minsdtf_amd/resampler.py attention_reference the
// float64 statement, DESIGN.md 4.20 the budget).
//
//   out(q) = softmax2(scale * q [K_x ; K_l]^T) [V_x ; V_l]          n <= 16 queries, t_x + n keys, one softmax over both segments
//
// The transposed products of ../ipadapter/ip_attention.hip: S^T[key, q] = K Q^T and O^T[d, q] = V^T P^T on 16x16x32 MFMAs, the query
// on the MFMA column, so a lane owns ONE query.  There are only 16 queries, so every K row and every V^T row is used exactly once per
// (sample, head): the A fragments are read straight from global memory - 16 bytes per lane, from whichever segment the key row belongs
// to by its index - and neither K nor V^T is staged in LDS.  Key rows: x keys at [0, t), latent keys at [t8, t8 + n), t8 =
// roundup8(t), so a 16-byte chunk of a V^T row belongs to one segment; the chunk's columns behind its segment's last key are forced
// to 0 (ia_keep's rule), and a key row of neither segment gets probability exactly 0 by its index.
//
// Work split: one workgroup = 4 waves = one (sample, head).  Wave w owns the score tiles w, w + 4, ... (16 key rows each); the row
// maximum and the row sum are merged across the waves through LDS in the order ((w0 + w1) + w2) + w3; the normalised probabilities,
// rounded once to bf16, go to LDS as P[query][key]; then wave w computes the output channels 16 w .. 16 w + 15 over ALL keys, so no
// partial output is ever merged.  No atomics, no scratch, no workspace.
#include "../common.h"
#include "../../../include/minsdtf_hip_resampler.h"

struct PAArgs {
    const bf16_t* q; const bf16_t* k_x; const bf16_t* vt_x; const bf16_t* k_l; const bf16_t* vt_l; bf16_t* out;
    float scale;
    int batch, heads, n, t, q_ld, kx_ld, vtx_ld, kl_ld, vtl_ld, o_ld;
};

#define PA_KEYS (MSDR_MAX_TX + MSDR_MAX_QUERIES)            // 288 key rows at the most (MSDR_MAX_TX is a multiple of 8)
static_assert(MSDR_MAX_TX % 8 == 0 && PA_KEYS % 32 == 0 && MSDR_KEY_TILE == 16 && MSDR_HEAD_DIM == 64, "geometry");
constexpr int PA_TILES = PA_KEYS / 16;                      // 18 score tiles
constexpr int PA_TPW = (PA_TILES + 3) / 4;                  // 5 score tiles per wave at the most
constexpr int PA_NKK = PA_KEYS / 32;                        // 9 steps of the P V product
constexpr int PA_PROW = PA_KEYS * 2 + 16;                   // bytes of a P row; an odd number of 16-byte slots

// the first `valid` (< 8) bf16 of a 16-byte chunk kept, the rest forced to 0: the columns behind a segment's last key are padding
__device__ __forceinline__ uint4 pa_keep(uint4 v, int valid) {
    uint32_t* u = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (2 * j >= valid) u[j] = 0;
        else if (2 * j + 1 >= valid) u[j] &= 0xFFFFu;
    }
    return v;
}

__global__ __launch_bounds__(256) void perceiver_attention_kernel(const PAArgs p) {
    __shared__ __attribute__((aligned(16))) char sP[16 * PA_PROW];
    __shared__ float sM[4][16];
    __shared__ float sL[4][16];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int bh = blockIdx.x, b = bh / p.heads, h = bh - b * p.heads;
    const int n = p.n, t = p.t, t8 = (t + 7) & ~7;
    const int tend = t8 + n;                      // one past the last key row in use (<= PA_KEYS)
    const int nkk = (tend + 31) >> 5;             // 32-key steps of the P V product
    const int ntile = 2 * nkk;                    // score tiles: all of those steps' key rows get a probability (0 behind tend)
    const size_t C = (size_t)p.heads * 64;

    // this lane's query (the columns r >= n repeat the last one; they are never stored)
    bf16x8 qf[2];
    {
        const bf16_t* qp = p.q + ((size_t)b * n + min(r, n - 1)) * p.q_ld + h * 64 + 8 * g;
        qf[0] = *reinterpret_cast<const bf16x8*>(qp);
        qf[1] = *reinterpret_cast<const bf16x8*>(qp + 32);
    }
    // the K fragments of this wave's score tiles: key row kf * 16 + r, channels ks * 32 + 8 g .. + 7
    bf16x8 kfr[PA_TPW][2];
#pragma unroll
    for (int i = 0; i < PA_TPW; ++i) {
        const int key = (wave + 4 * i) * 16 + r;
        const bf16_t* src = nullptr;
        if (wave + 4 * i < ntile) {
            if (key < t) src = p.k_x + ((size_t)b * t + key) * p.kx_ld;
            else if (key >= t8 && key < tend) src = p.k_l + ((size_t)b * n + (key - t8)) * p.kl_ld;
        }
        kfr[i][0] = kfr[i][1] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        if (src) {
            src += h * 64 + 8 * g;
            kfr[i][0] = *reinterpret_cast<const bf16x8*>(src);
            kfr[i][1] = *reinterpret_cast<const bf16x8*>(src + 32);
        }
    }
    // the V^T fragments of this wave's 16 output channels: channel 16 w + r, keys kk * 32 + 8 g .. + 7 (in flight under the softmax)
    uint4 rv[PA_NKK];
    {
        const size_t row = (size_t)b * C + h * 64 + 16 * wave + r;
        const bf16_t* vx = p.vt_x + row * p.vtx_ld;
        const bf16_t* vl = p.vt_l + row * p.vtl_ld;
#pragma unroll
        for (int kk = 0; kk < PA_NKK; ++kk) {
            const int c0 = kk * 32 + 8 * g;       // the chunk's first key row
            rv[kk] = make_uint4(0, 0, 0, 0);
            if (kk < nkk) {
                // (c0 < t <= vtx_ld, c0 - t8 < n <= vtl_ld and all multiples of 8: the 16 bytes lie inside the row)
                if (c0 < t) rv[kk] = pa_keep(*reinterpret_cast<const uint4*>(vx + c0), min(t - c0, 8));
                else if (c0 >= t8 && c0 < tend) rv[kk] = pa_keep(*reinterpret_cast<const uint4*>(vl + (c0 - t8)), min(tend - c0, 8));
            }
        }
    }

    // S^T = K Q^T, times scale; lane holds keys kf * 16 + 4 g + e of query r
    f32x4 s[PA_TPW];
    float m = -1e30f;
#pragma unroll
    for (int i = 0; i < PA_TPW; ++i) {
        const int kf = wave + 4 * i;
        s[i] = (f32x4){0, 0, 0, 0};
        if (kf < ntile) {
            s[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[i][0], qf[0], s[i], 0, 0, 0);
            s[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfr[i][1], qf[1], s[i], 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = kf * 16 + 4 * g + e;
            s[i][e] = __fmul_rn(s[i][e], p.scale);
            if (key < t || (key >= t8 && key < tend)) m = fmaxf(m, s[i][e]);
        }
    }
    // the true row maximum over all keys of both segments: the four key groups, then the four waves
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    if (g == 0) sM[wave][r] = m;
    __syncthreads();
    m = fmaxf(fmaxf(fmaxf(sM[0][r], sM[1][r]), sM[2][r]), sM[3][r]);

    // the exponentials in place (neither segment: exactly 0) and the fp32 row sum
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < PA_TPW; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = (wave + 4 * i) * 16 + 4 * g + e;
            float pe = 0.f;
            if (key < t || (key >= t8 && key < tend)) { pe = __builtin_amdgcn_exp2f(s[i][e] - m); l += pe; }
            s[i][e] = pe;
        }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (g == 0) sL[wave][r] = l;
    __syncthreads();
    l = ((sL[0][r] + sL[1][r]) + sL[2][r]) + sL[3][r];
    const float c = 1.0f / l;                     // t >= 1: l >= 1

    // P[query][key], normalised before its one rounding to bf16
#pragma unroll
    for (int i = 0; i < PA_TPW; ++i) {
        const int kf = wave + 4 * i;
        if (kf < ntile) {
            uint2 v;
            v.x = pack_bf2(__fmul_rn(s[i][0], c), __fmul_rn(s[i][1], c));
            v.y = pack_bf2(__fmul_rn(s[i][2], c), __fmul_rn(s[i][3], c));
            *reinterpret_cast<uint2*>(sP + r * PA_PROW + (kf * 16 + 4 * g) * 2) = v;
        }
    }
    __syncthreads();

    // O^T = V^T P^T over all keys; lane holds channels 16 w + 4 g + e of query r
    f32x4 o = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < PA_NKK; ++kk) {
        if (kk < nkk) {
            const bf16x8 pf = *reinterpret_cast<const bf16x8*>(sP + r * PA_PROW + (kk * 32 + 8 * g) * 2);
            union { uint4 u; bf16x8 v; } vf;
            vf.u = rv[kk];
            o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, pf, o, 0, 0, 0);
        }
    }
    if (r < n) {
        uint2 v;
        v.x = pack_bf2(o[0], o[1]);
        v.y = pack_bf2(o[2], o[3]);
        *reinterpret_cast<uint2*>(p.out + ((size_t)b * n + r) * p.o_ld + h * 64 + 16 * wave + 4 * g) = v;
    }
}

static bool pa_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

extern "C" int msdr_perceiver_attention(const MsdrPerceiverAttention* p, msdr_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "perceiver_attention: null argument");
    if (!p->q || !p->k_x || !p->vt_x || !p->k_l || !p->vt_l || !p->out)
        MSD_FAIL(MSD_E_ARG, "perceiver_attention: null q / k_x / vt_x / k_l / vt_l / out");
    if (!msd_aligned16(p->q) || !msd_aligned16(p->k_x) || !msd_aligned16(p->vt_x) || !msd_aligned16(p->k_l) || !msd_aligned16(p->vt_l) ||
        !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "perceiver_attention: q / k_x / vt_x / k_l / vt_l / out must be 16-byte aligned");
    if (p->head_dim != MSDR_HEAD_DIM) MSD_FAIL(MSD_E_UNSUPPORTED, "perceiver_attention: head_dim %d (%d only)", p->head_dim, MSDR_HEAD_DIM);
    if (p->n < 1 || p->n > MSDR_MAX_QUERIES) MSD_FAIL(MSD_E_ARG, "perceiver_attention: n = %d latent queries (1 .. %d)", p->n, MSDR_MAX_QUERIES);
    if (p->t_x < 1 || p->t_x > MSDR_MAX_TX) MSD_FAIL(MSD_E_ARG, "perceiver_attention: t_x = %d keys (1 .. %d)", p->t_x, MSDR_MAX_TX);
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "perceiver_attention: batch %d (1 .. 65535)", p->batch);
    if (p->heads < 1 || p->heads > 65535) MSD_FAIL(MSD_E_ARG, "perceiver_attention: heads %d (1 .. 65535)", p->heads);
    if (!(p->scale == p->scale) || p->scale - p->scale != 0.0f) MSD_FAIL(MSD_E_ARG, "perceiver_attention: scale must be finite");
    const int64_t C = (int64_t)p->heads * MSDR_HEAD_DIM;
    if (p->q_ld % 8) MSD_FAIL(MSD_E_ARG, "perceiver_attention: q_ld = %d must be a multiple of 8", p->q_ld);
    if (p->kx_ld % 8) MSD_FAIL(MSD_E_ARG, "perceiver_attention: kx_ld = %d must be a multiple of 8", p->kx_ld);
    if (p->vtx_ld % 8) MSD_FAIL(MSD_E_ARG, "perceiver_attention: vtx_ld = %d must be a multiple of 8", p->vtx_ld);
    if (p->kl_ld % 8) MSD_FAIL(MSD_E_ARG, "perceiver_attention: kl_ld = %d must be a multiple of 8", p->kl_ld);
    if (p->vtl_ld % 8) MSD_FAIL(MSD_E_ARG, "perceiver_attention: vtl_ld = %d must be a multiple of 8", p->vtl_ld);
    if (p->o_ld % 8) MSD_FAIL(MSD_E_ARG, "perceiver_attention: o_ld = %d must be a multiple of 8", p->o_ld);
    if (p->q_ld < C || p->kx_ld < C || p->kl_ld < C || p->o_ld < C)
        MSD_FAIL(MSD_E_ARG, "perceiver_attention: q_ld / kx_ld / kl_ld / o_ld smaller than heads * head_dim");
    if (p->vtx_ld < p->t_x) MSD_FAIL(MSD_E_ARG, "perceiver_attention: vtx_ld = %d < t_x = %d", p->vtx_ld, p->t_x);
    if (p->vtl_ld < p->n) MSD_FAIL(MSD_E_ARG, "perceiver_attention: vtl_ld = %d < n = %d", p->vtl_ld, p->n);
    const int64_t wgs = (int64_t)p->batch * p->heads;
    if (wgs >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "perceiver_attention: 2^31 or more workgroups");
    {   // out lies apart from every input
        const int64_t rows = (int64_t)p->batch * p->n;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)(((rows - 1) * p->o_ld + C) * 2);
        const uintptr_t q0 = (uintptr_t)p->q, q1 = q0 + (uintptr_t)(((rows - 1) * p->q_ld + C) * 2);
        const uintptr_t k0 = (uintptr_t)p->k_x, k1 = k0 + (uintptr_t)((((int64_t)p->batch * p->t_x - 1) * p->kx_ld + C) * 2);
        const uintptr_t v0 = (uintptr_t)p->vt_x, v1 = v0 + (uintptr_t)((int64_t)p->batch * C * p->vtx_ld * 2);
        const uintptr_t kl0 = (uintptr_t)p->k_l, kl1 = kl0 + (uintptr_t)(((rows - 1) * p->kl_ld + C) * 2);
        const uintptr_t vl0 = (uintptr_t)p->vt_l, vl1 = vl0 + (uintptr_t)((int64_t)p->batch * C * p->vtl_ld * 2);
        if (pa_overlap(o0, o1, q0, q1) || pa_overlap(o0, o1, k0, k1) || pa_overlap(o0, o1, v0, v1) || pa_overlap(o0, o1, kl0, kl1) ||
            pa_overlap(o0, o1, vl0, vl1))
            MSD_FAIL(MSD_E_ARG, "perceiver_attention: out overlaps an input");
    }
    PAArgs a;
    a.q = (const bf16_t*)p->q; a.k_x = (const bf16_t*)p->k_x; a.vt_x = (const bf16_t*)p->vt_x;
    a.k_l = (const bf16_t*)p->k_l; a.vt_l = (const bf16_t*)p->vt_l; a.out = (bf16_t*)p->out;
    a.scale = p->scale;
    a.batch = p->batch; a.heads = p->heads; a.n = p->n; a.t = p->t_x;
    a.q_ld = p->q_ld; a.kx_ld = p->kx_ld; a.vtx_ld = p->vtx_ld; a.kl_ld = p->kl_ld; a.vtl_ld = p->vtl_ld; a.o_ld = p->o_ld;
    hipLaunchKernelGGL(perceiver_attention_kernel, dim3((unsigned)wgs), dim3(256), 0, stream, a);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
