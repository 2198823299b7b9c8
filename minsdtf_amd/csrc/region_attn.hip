// msd_region_attention: regional prompting inside cross-attention ("attention couple"; include/minsdtf_hip.h has the operands and
// the pinned arithmetic, minsdtf_amd/regions.py builds the per-level weight planes, DESIGN.md 4.10 the budget).
//
//   out(q) = sum_r w_r(q) * softmax(q K_r^T) V_r        regions ascending, a weight of exactly 0 is not accumulated
//
// A fork of attention_kernel's transposed products (attention.hip): S^T[key, q] = K Q^T and O^T[d, q] = V^T P^T on 16x16x32 MFMAs,
// the query on the MFMA column, so a lane owns ONE query: its maximum, its row sum, its weight and the running weighted sum over
// the regions are lane-local.  The text context is at most 96 keys, so a region's K and V^T are ONE tile: no online softmax, the
// row maximum is the true one and every exponential is <= 1.
//
// Work split: one workgroup = 4 waves = 64 queries of one (sample, head); a wave owns 16 queries (one MFMA column block) at every
// head size - at d = 160 the attention accumulator and the regional accumulator are 40 registers each.  The regions are walked in
// order; each one's K [96][d] and V^T [d][96] are staged in the one LDS buffer between two barriers.  A region whose weights are 0
// at all 64 queries of the workgroup is skipped before the first barrier (every wave looks at the same 64 weights, so the
// decision is workgroup-uniform): nothing is staged and nothing computed, and since a lane never accumulates a region of weight
// 0 anyway, the skip changes no bit.  With box masks that leaves most workgroups one region: the cost of a plain cross-attention.
#include "common.h"

struct RAArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* vt; const float* w; bf16_t* out;
    int batch, heads, s, t, regions, q_ld, k_ld, vt_ld, w_ld, o_ld;
};

#define RA_KEYS 96   // keys of the one tile (the text context: t <= 96)

template <int D>
struct RAGeom {
    static constexpr int DPAD = ((D + 31) / 32) * 32;   // QK^T k-dimension, zero-padded to whole 32-channel MFMA steps
    static constexpr int KS = DPAD / 32;
    static constexpr int DF = (D + 15) / 16;             // 16-row blocks of O^T
    static constexpr int KROW = DPAD * 2 + 16;           // bytes; an odd number of 16-byte slots: conflict-free fragment reads
    static constexpr int VROW = RA_KEYS * 2 + 16;        // 13 slots
    static constexpr int DCH = D / 8;                    // 16-byte chunks of a K row
    static constexpr int K_BYTES = RA_KEYS * KROW;
    static constexpr int LDS = K_BYTES + DF * 16 * VROW;
};
static_assert(RAGeom<160>::LDS <= 64 * 1024 && RAGeom<80>::LDS <= 64 * 1024 && RAGeom<40>::LDS <= 64 * 1024, "LDS budget");

template <int D>
__global__ __launch_bounds__(256) void region_attention_kernel(const RAArgs p) {
    using G = RAGeom<D>;
    constexpr int KS = G::KS, DF = G::DF, KROW = G::KROW, VROW = G::VROW, DCH = G::DCH;
    constexpr int NKF = RA_KEYS / 16, NKK = RA_KEYS / 32, VCHUNKS = RA_KEYS / 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const sK = smem;
    char* const sV = smem + G::K_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    // all query tiles of one (sample, head) on one XCD: its regions' K / V^T stay in that XCD's L2
    const int qtiles = (p.s + 63) / 64;
    const int wi = xcd_remap(blockIdx.x, qtiles * p.heads * p.batch);
    const int bh = wi / qtiles, b = bh / p.heads, h = bh - b * p.heads;
    const int qwg = (wi - bh * qtiles) * 64;      // first query of the workgroup
    const int qrow = qwg + wave * 16 + r;         // this lane's query

    // zero the LDS image once: the pad columns of K (d = 40 / 80) and the pad rows of V^T are never written afterwards (the first
    // barrier of the region loop orders the fill in front of the staging stores)
    for (int off = tid * 16; off < G::LDS; off += 256 * 16) *reinterpret_cast<uint4*>(smem + off) = make_uint4(0, 0, 0, 0);

    bf16x8 qf[KS];
    {
        const int qr = qrow < p.s ? qrow : p.s - 1;
        const bf16_t* qp = p.q + ((size_t)b * p.s + qr) * p.q_ld + h * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int d0 = ks * 32 + 8 * g;
            if (d0 < D) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + d0);
            else qf[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
    }

    f32x4 acc[DF];
#pragma unroll
    for (int df = 0; df < DF; ++df) acc[df] = (f32x4){0, 0, 0, 0};
    bool started = false;   // some region was accumulated for this lane's query

    constexpr int KCH = (RA_KEYS * DCH + 255) / 256, VCH = (D * VCHUNKS + 255) / 256;

    for (int reg = 0; reg < p.regions; ++reg) {
        const float* wrow = p.w + (size_t)reg * p.w_ld;
        // the workgroup's 64 weights, one per lane, the same in every wave
        const float wtile = qwg + lane < p.s ? wrow[qwg + lane] : 0.f;
        if (__builtin_amdgcn_ballot_w64(wtile > 0.f) == 0) continue;
        const float wq = qrow < p.s ? wrow[qrow] : 0.f;

        const size_t row0 = (size_t)reg * p.batch + b;
        const bf16_t* kbase = p.k + row0 * p.t * p.k_ld + h * D;
        const bf16_t* vbase = p.vt + (row0 * p.heads + h) * D * p.vt_ld;

        __syncthreads();   // the previous region's tile is consumed by every wave
        {
            uint4 rk[KCH], rv[VCH];
#pragma unroll
            for (int i = 0; i < KCH; ++i) {
                const int idx = tid + 256 * i, row = idx / DCH, ch = idx - row * DCH;
                rk[i] = make_uint4(0, 0, 0, 0);
                if (idx < RA_KEYS * DCH && row < p.t) rk[i] = *reinterpret_cast<const uint4*>(kbase + (size_t)row * p.k_ld + ch * 8);
            }
#pragma unroll
            for (int i = 0; i < VCH; ++i) {
                const int idx = tid + 256 * i, d = idx / VCHUNKS, ch = idx - d * VCHUNKS;
                rv[i] = make_uint4(0, 0, 0, 0);
                // (ch * 8 < t <= vt_ld and vt_ld % 8 == 0: the 16 bytes lie inside the row)
                if (idx < D * VCHUNKS && ch * 8 < p.t) rv[i] = *reinterpret_cast<const uint4*>(vbase + (size_t)d * p.vt_ld + ch * 8);
            }
#pragma unroll
            for (int i = 0; i < KCH; ++i) {
                const int idx = tid + 256 * i, row = idx / DCH, ch = idx - row * DCH;
                if (idx < RA_KEYS * DCH) *reinterpret_cast<uint4*>(sK + row * KROW + ch * 16) = rk[i];
            }
#pragma unroll
            for (int i = 0; i < VCH; ++i) {
                const int idx = tid + 256 * i, d = idx / VCHUNKS, ch = idx - d * VCHUNKS;
                if (idx >= D * VCHUNKS) continue;
                uint4 v = rv[i];
                const int valid = p.t - ch * 8;   // keys >= t are padding of unspecified content: forced to 0
                if (valid < 8) {
                    uint32_t* u = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (2 * j >= valid) u[j] = 0;
                        else if (2 * j + 1 >= valid) u[j] &= 0xFFFFu;
                    }
                }
                *reinterpret_cast<uint4*>(sV + d * VROW + ch * 16) = v;
            }
        }
        __syncthreads();

        // S^T = K Q^T (q carries scale * log2(e)); lane holds keys kf * 16 + 4 g + e of query r
        f32x4 s[NKF];
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf) {
            s[kf] = (f32x4){0, 0, 0, 0};
            if (kf * 16 < p.t) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const bf16x8 kfrag = *reinterpret_cast<const bf16x8*>(sK + (kf * 16 + r) * KROW + ks * 64 + g * 16);
                    s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag, qf[ks], s[kf], 0, 0, 0);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (kf * 16 + 4 * g + e >= p.t) s[kf][e] = -1e30f;
        }
        float m = s[0][0];
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
            for (int e = 0; e < 4; ++e) m = fmaxf(m, s[kf][e]);
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));

        // P = exp2(S - m) rounded to bf16: the B operand of the second product, and what the row sum adds up
        f32x4 o[DF];
#pragma unroll
        for (int df = 0; df < DF; ++df) o[df] = (f32x4){0, 0, 0, 0};
        float l = 0.f;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            if (kk * 32 >= p.t) continue;
            union { bf16x8 v; uint32_t u[4]; } pk;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x4 sv = s[2 * kk + j];
                pk.u[2 * j] = pack_bf2(__builtin_amdgcn_exp2f(sv[0] - m), __builtin_amdgcn_exp2f(sv[1] - m));
                pk.u[2 * j + 1] = pack_bf2(__builtin_amdgcn_exp2f(sv[2] - m), __builtin_amdgcn_exp2f(sv[3] - m));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) l += bf_lo(pk.u[j]) + bf_hi(pk.u[j]);
#pragma unroll
            for (int df = 0; df < DF; ++df) {
                union { bf16x8 v; uint2 h2[2]; } vf;
                const char* vp = sV + (df * 16 + r) * VROW + kk * 64 + g * 8;
                vf.h2[0] = *reinterpret_cast<const uint2*>(vp);
                vf.h2[1] = *reinterpret_cast<const uint2*>(vp + 32);
                o[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, pk.v, o[df], 0, 0, 0);
            }
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;

        // the lane's query: the first region of positive weight starts the sum, every later one is one fused multiply-add
        if (wq > 0.f) {
#pragma unroll
            for (int df = 0; df < DF; ++df)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ov = __fmul_rn(o[df][e], inv);
                    acc[df][e] = started ? __fmaf_rn(wq, ov, acc[df][e]) : __fmul_rn(wq, ov);
                }
            started = true;
        }
    }

    if (qrow < p.s) {
        bf16_t* op = p.out + ((size_t)b * p.s + qrow) * p.o_ld + h * D;
#pragma unroll
        for (int df = 0; df < DF; ++df) {
            const int d = df * 16 + 4 * g;
            if (d < D) {
                uint2 v;
                v.x = pack_bf2(acc[df][0], acc[df][1]);
                v.y = pack_bf2(acc[df][2], acc[df][3]);
                *reinterpret_cast<uint2*>(op + d) = v;
            }
        }
    }
}

static bool g_ra_attr_done = false;

template <int D>
static hipError_t ra_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&region_attention_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               RAGeom<D>::LDS);
}

static bool ra_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

extern "C" int msd_region_attention(const MsdRegionAttention* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "region_attention: null argument");
    if (!p->q || !p->k || !p->vt || !p->w || !p->out) MSD_FAIL(MSD_E_ARG, "region_attention: null q / k / vt / w / out");
    if (!msd_aligned16(p->q) || !msd_aligned16(p->k) || !msd_aligned16(p->vt) || !msd_aligned16(p->w) || !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "region_attention: q / k / vt / w / out must be 16-byte aligned");
    if (p->head_dim != 40 && p->head_dim != 80 && p->head_dim != 160)
        MSD_FAIL(MSD_E_ARG, "region_attention: head_dim %d (40, 80 or 160)", p->head_dim);
    if (p->t < 1 || p->t > RA_KEYS) MSD_FAIL(MSD_E_ARG, "region_attention: t = %d keys (1 .. %d)", p->t, RA_KEYS);
    if (p->regions < 1 || p->regions > MSD_REGION_MAX) MSD_FAIL(MSD_E_ARG, "region_attention: %d regions (1 .. %d)", p->regions, MSD_REGION_MAX);
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "region_attention: batch %d (1 .. 65535)", p->batch);
    if (p->heads < 1 || p->heads > 65535 || p->s < 1) MSD_FAIL(MSD_E_ARG, "region_attention: heads = %d (1 .. 65535), s = %d (>= 1)", p->heads, p->s);
    const int64_t C = (int64_t)p->heads * p->head_dim;
    if (p->w_ld < p->s) MSD_FAIL(MSD_E_ARG, "region_attention: w_ld = %d < s = %d", p->w_ld, p->s);
    if ((p->q_ld % 8) || (p->k_ld % 8) || (p->vt_ld % 8) || (p->o_ld % 8))
        MSD_FAIL(MSD_E_ARG, "region_attention: q_ld / k_ld / vt_ld / o_ld must be multiples of 8");
    if (p->q_ld < C || p->k_ld < C || p->o_ld < C) MSD_FAIL(MSD_E_ARG, "region_attention: q_ld / k_ld / o_ld smaller than heads * head_dim");
    if (p->vt_ld < p->t) MSD_FAIL(MSD_E_ARG, "region_attention: vt_ld = %d < t = %d", p->vt_ld, p->t);
    const int64_t qtiles = ((int64_t)p->s + 63) / 64, wgs = qtiles * p->heads * p->batch;
    if (wgs >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "region_attention: 2^31 or more workgroups");
    {   // out lies apart from every input
        const int64_t rows = (int64_t)p->batch * p->s, krows = (int64_t)p->regions * p->batch * p->t;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)(((rows - 1) * p->o_ld + C) * 2);
        const uintptr_t q0 = (uintptr_t)p->q, q1 = q0 + (uintptr_t)(((rows - 1) * p->q_ld + C) * 2);
        const uintptr_t k0 = (uintptr_t)p->k, k1 = k0 + (uintptr_t)(((krows - 1) * p->k_ld + C) * 2);
        const uintptr_t v0 = (uintptr_t)p->vt, v1 = v0 + (uintptr_t)((int64_t)p->regions * p->batch * C * p->vt_ld * 2);
        const uintptr_t w0 = (uintptr_t)p->w, w1 = w0 + (uintptr_t)(((int64_t)(p->regions - 1) * p->w_ld + p->s) * 4);
        if (ra_overlap(o0, o1, q0, q1) || ra_overlap(o0, o1, k0, k1) || ra_overlap(o0, o1, v0, v1) || ra_overlap(o0, o1, w0, w1))
            MSD_FAIL(MSD_E_ARG, "region_attention: out overlaps an input");
    }
    if (!g_ra_attr_done) {
        hipError_t e = ra_attr<40>();
        if (e == hipSuccess) e = ra_attr<80>();
        if (e == hipSuccess) e = ra_attr<160>();
        if (e != hipSuccess) MSD_FAIL((int)e, "hipFuncSetAttribute(region_attention): %s", hipGetErrorString(e));
        g_ra_attr_done = true;
    }
    RAArgs a;
    a.q = (const bf16_t*)p->q; a.k = (const bf16_t*)p->k; a.vt = (const bf16_t*)p->vt; a.w = p->w; a.out = (bf16_t*)p->out;
    a.batch = p->batch; a.heads = p->heads; a.s = p->s; a.t = p->t; a.regions = p->regions;
    a.q_ld = p->q_ld; a.k_ld = p->k_ld; a.vt_ld = p->vt_ld; a.w_ld = p->w_ld; a.o_ld = p->o_ld;
    const dim3 grid((unsigned)wgs);
    switch (p->head_dim) {
        case 40: hipLaunchKernelGGL(region_attention_kernel<40>, grid, dim3(256), RAGeom<40>::LDS, stream, a); break;
        case 80: hipLaunchKernelGGL(region_attention_kernel<80>, grid, dim3(256), RAGeom<80>::LDS, stream, a); break;
        default: hipLaunchKernelGGL(region_attention_kernel<160>, grid, dim3(256), RAGeom<160>::LDS, stream, a); break;
    }
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
