// msd_attention_joint / msd_reference_latent: reference-only control (include/minsdtf_hip.h has the operands and the pinned
// arithmetic, minsdtf_amd/reference.py the float64 statement, DESIGN.md 4.11 the budget).
//
//   joint(q) = softmax(q [K_own ; K_ref]^T) [V_own ; V_ref]        plain(q) = softmax(q K_own^T) V_own
//   out      = mix * plain + (1 - mix) * joint                      mix per sample
//
// A fork of region_attention_kernel's transposed products (region_attn.hip): S^T[key, q] = K Q^T and O^T[d, q] = V^T P^T on
// 16x16x32 MFMAs, the query on the MFMA column, so a lane owns ONE query: its running maximum, its row sum and its blend are
// lane-local.  Unlike there the keys are many tiles, so the softmax is attention_kernel's online one: a running maximum, the
// accumulator rescaled by exp2(m_old - m_new) at every tile (no lazy rescaling: the snapshot below is then exact by construction).
//
// Work split: one workgroup = 4 waves = 64 queries of one (sample, head); a wave owns 16 queries at every head size.  The keys are
// walked in 64-key tiles, the own segment first, then the reference segment; either segment's last tile may be partial (the own
// one's in the middle of the walk): its missing keys are staged as zeros and their scores masked.  After the last own tile the
// state IS the plain attention: plain = O * (1 / l) is kept in registers (40 at d = 160) when the sample's mix is not 0; a sample
// with mix == 1 stops there and never reads the reference segment.  mix is one value per sample and a workgroup is one sample, so
// both decisions are workgroup-uniform.
//
// Staging: K [64][d] and V^T [d][64] of a tile are one LDS image (44.5 KB at d = 160); the next tile's global loads are issued into
// registers before the current tile's products and stored to LDS behind them, so the loads fly under the MFMAs.  d = 40 / 80 keep
// TWO images and pay one barrier per tile (the store of tile i + 1 goes to the image tile i - 1 left); d = 160 keeps one image
// and two barriers (two images of 44.5 KB for each of a CU's two workgroups exceed its 160 KB).
#include <type_traits>
#include "common.h"

// maximum over the four 16-lane rows (lanes l, l ^ 16, l ^ 32, l ^ 48), on every lane: two row swaps (wave_max's last two steps,
// common.h) instead of two ds_bpermute round trips in the middle of every tile's dependency chain
__device__ __forceinline__ float ja_rows_max(float v) {
    const uint32_t u = __float_as_uint(v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const uint32_t w = __float_as_uint(v);
    auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

struct JAArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* vt; const bf16_t* k_ref; const bf16_t* vt_ref; const float* mix; bf16_t* out;
    int batch, heads, s, t, t_ref, q_ld, k_ld, vt_ld, o_ld;
};

#define JA_KEYS 64   // keys of a tile

template <int D>
struct JAGeom {
    static constexpr int DPAD = ((D + 31) / 32) * 32;   // QK^T k-dimension, zero-padded to whole 32-channel MFMA steps
    static constexpr int KS = DPAD / 32;
    static constexpr int DF = (D + 15) / 16;             // 16-row blocks of O^T
    static constexpr int KROW = DPAD * 2 + 16;           // bytes; an odd number of 16-byte slots: conflict-free fragment reads
    static constexpr int VROW = JA_KEYS * 2 + 16;        // 9 slots
    static constexpr int DCH = D / 8;                    // 16-byte chunks of a K row
    static constexpr int K_BYTES = JA_KEYS * KROW;
    static constexpr int TILE = K_BYTES + DF * 16 * VROW;   // one tile's K and V^T image
    static constexpr int NBUF = D < 160 ? 2 : 1;            // d = 40 / 80: two images, ONE barrier per tile (d = 160: 2 x 44.5 KB x 2 workgroups > 160 KB)
    static constexpr int LDS = NBUF * TILE;
};
static_assert(JAGeom<160>::LDS <= 64 * 1024 && JAGeom<80>::LDS <= 64 * 1024 && JAGeom<40>::LDS <= 64 * 1024, "LDS budget");

template <int D>
__global__ __launch_bounds__(256, D == 40 ? 4 : D == 80 ? 2 : 1) void attention_joint_kernel(const JAArgs p) {   // (d = 40: 128 registers, 4 waves per SIMD)
    using G = JAGeom<D>;
    constexpr int KS = G::KS, DF = G::DF, KROW = G::KROW, VROW = G::VROW, DCH = G::DCH;
    constexpr int NKF = JA_KEYS / 16, NKK = JA_KEYS / 32, VCHUNKS = JA_KEYS / 8;
    constexpr int KCH = (JA_KEYS * DCH + 255) / 256, VCH = (D * VCHUNKS + 255) / 256;
    constexpr int NBUF = G::NBUF;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    // all query tiles of one (sample, head) on one XCD: its K / V^T (and the shared reference row's) stay in that XCD's L2
    const int qtiles = (p.s + 63) / 64;
    const int wi = xcd_remap(blockIdx.x, qtiles * p.heads * p.batch);
    const int bh = wi / qtiles, b = bh / p.heads, h = bh - b * p.heads;
    const int qrow = (wi - bh * qtiles) * 64 + wave * 16 + r;   // this lane's query

    const float f = p.mix ? p.mix[b] : 0.f;   // one value per sample: uniform over the workgroup
    const int nt1 = (p.t + JA_KEYS - 1) / JA_KEYS;
    const int ntot = nt1 + (f == 1.0f ? 0 : (p.t_ref + JA_KEYS - 1) / JA_KEYS);   // mix == 1: the reference segment is not read

    // zero the LDS image once: the pad columns of K (d = 40 / 80) and the pad rows of V^T are never written afterwards (the first
    // barrier of the tile loop orders the fill in front of the staging stores)
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

    const bf16_t* const k_own = p.k + (size_t)b * p.t * p.k_ld + h * D;
    const bf16_t* const v_own = p.vt + ((size_t)b * p.heads + h) * D * p.vt_ld;
    const bf16_t* const k_rf = p.k_ref + h * D;
    const bf16_t* const v_rf = p.vt_ref + (size_t)h * D * p.vt_ld;

    uint4 rk[KCH], rv[VCH];
    // tile i of the walk -> registers; keys past the segment's end come back as zeros (never read from memory)
    auto fetch = [&](int i) {
        const bool own = i < nt1;
        const int key0 = (own ? i : i - nt1) * JA_KEYS;
        const int left = (own ? p.t : p.t_ref) - key0;   // >= 1 keys of the segment from key0 on
        const bf16_t* kb = (own ? k_own : k_rf) + (size_t)key0 * p.k_ld;
        const bf16_t* vb = (own ? v_own : v_rf) + key0;
#pragma unroll
        for (int j = 0; j < KCH; ++j) {
            const int idx = tid + 256 * j, row = idx / DCH, ch = idx - row * DCH;
            rk[j] = make_uint4(0, 0, 0, 0);
            if (idx < JA_KEYS * DCH && row < left) rk[j] = *reinterpret_cast<const uint4*>(kb + (size_t)row * p.k_ld + ch * 8);
        }
#pragma unroll
        for (int j = 0; j < VCH; ++j) {
            const int idx = tid + 256 * j, d = idx / VCHUNKS, ch = idx - d * VCHUNKS;
            rv[j] = make_uint4(0, 0, 0, 0);
            // (key0 + ch * 8 < segment length <= vt_ld and vt_ld % 8 == 0: the 16 bytes lie inside the row)
            if (idx < D * VCHUNKS && ch * 8 < left) {
                uint4 v = *reinterpret_cast<const uint4*>(vb + (size_t)d * p.vt_ld + ch * 8);
                const int valid = left - ch * 8;   // keys >= the segment length are padding of unspecified content: forced to 0
                if (valid < 8) {
                    uint32_t* u = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (2 * e >= valid) u[e] = 0;
                        else if (2 * e + 1 >= valid) u[e] &= 0xFFFFu;
                    }
                }
                rv[j] = v;
            }
        }
    };

    f32x4 o[DF], snap[DF];
#pragma unroll
    for (int df = 0; df < DF; ++df) o[df] = snap[df] = (f32x4){0, 0, 0, 0};
    float m = -1e30f;   // running maximum of this lane's query (the same on its four g lanes)
    float l = 0.f;      // this lane's share of the row sum (keys 4 g + e of every 16): reduced over g where it is used

    // the fetched tile: registers -> LDS image `buf`
    auto stage = [&](int buf) {
        char* const dK = smem + buf * G::TILE;
        char* const dV = dK + G::K_BYTES;
#pragma unroll
        for (int j = 0; j < KCH; ++j) {
            const int idx = tid + 256 * j, row = idx / DCH, ch = idx - row * DCH;
            if (idx < JA_KEYS * DCH) *reinterpret_cast<uint4*>(dK + row * KROW + ch * 16) = rk[j];
        }
#pragma unroll
        for (int j = 0; j < VCH; ++j) {
            const int idx = tid + 256 * j, d = idx / VCHUNKS, ch = idx - d * VCHUNKS;
            if (idx < D * VCHUNKS) *reinterpret_cast<uint4*>(dV + d * VROW + ch * 16) = rv[j];
        }
    };

    fetch(0);
    __syncthreads();   // the zero fill, in front of the first staging stores
    stage(0);
    for (int i = 0; i < ntot; ++i) {
        const int valid = (i < nt1 ? p.t - i * JA_KEYS : p.t_ref - (i - nt1) * JA_KEYS);   // keys of this tile (may exceed 64)
        const char* const sK = smem + (i % NBUF) * G::TILE;
        const char* const sV = sK + G::K_BYTES;

        __syncthreads();   // tile i is staged by every wave (two images: and every wave is through with tile i - 1, whose image tile i + 1 takes)
        if (i + 1 < ntot) fetch(i + 1);   // in flight under this tile's products

        // the tile's arithmetic, compiled twice: FULL (all 64 keys: straight-line code, nothing masked - every tile of a segment but
        // its last) and partial (key fragments past `valid` skipped, their scores masked).  On a full tile the two give the same bits.
        auto tile = [&](auto full_c) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_c)::value;
        // S^T = K Q^T (q carries scale * log2(e)); lane holds keys kf * 16 + 4 g + e of query r
        f32x4 s[NKF];
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf) {
            s[kf] = (f32x4){0, 0, 0, 0};
            if (FULL || kf * 16 < valid) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const bf16x8 kfrag = *reinterpret_cast<const bf16x8*>(sK + (kf * 16 + r) * KROW + ks * 64 + g * 16);
                    s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag, qf[ks], s[kf], 0, 0, 0);
                }
            }
            if (!FULL) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kf * 16 + 4 * g + e >= valid) s[kf][e] = -1e30f;
            }
        }
        float mt = s[0][0];
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
            for (int e = 0; e < 4; ++e) mt = fmaxf(mt, s[kf][e]);
        mt = ja_rows_max(mt);
        const float mn = fmaxf(m, mt);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);   // 0 at the first tile (m = -1e30, o = 0, l = 0)
        m = mn;
        l *= alpha;
#pragma unroll
        for (int df = 0; df < DF; ++df)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[df][e] *= alpha;

        // P = exp2(S - m) rounded to bf16: the B operand of the second product, and what the row sum adds up
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            if (!FULL && kk * 32 >= valid) continue;
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
        };
        // (d = 160 keeps the one masked form: two copies of its loop body cost the second wave per SIMD - 256 registers)
        if (D < 160 && valid >= JA_KEYS) tile(std::true_type{});
        else tile(std::false_type{});

        // the segment boundary: the state is the plain self-attention's (skipped where it is not used: mix == 0)
        if (i == nt1 - 1 && f != 0.f) {
            float l1 = l;
            l1 += __shfl_xor(l1, 16);
            l1 += __shfl_xor(l1, 32);
            const float inv1 = 1.0f / l1;
#pragma unroll
            for (int df = 0; df < DF; ++df)
#pragma unroll
                for (int e = 0; e < 4; ++e) snap[df][e] = __fmul_rn(o[df][e], inv1);
        }

        if (i + 1 < ntot) {
            if (NBUF == 1) __syncthreads();   // one image: tile i is consumed by every wave before tile i + 1 overwrites it
            stage((i + 1) % NBUF);
        }
    }

    if (f != 1.0f) {
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        const float inv = 1.0f / l;
        const float fj = 1.0f - f;
#pragma unroll
        for (int df = 0; df < DF; ++df)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float joint = __fmul_rn(o[df][e], inv);
                snap[df][e] = f == 0.f ? joint : __fmaf_rn(f, snap[df][e], __fmul_rn(fj, joint));
            }
    }

    if (qrow < p.s) {
        bf16_t* op = p.out + ((size_t)b * p.s + qrow) * p.o_ld + h * D;
#pragma unroll
        for (int df = 0; df < DF; ++df) {
            const int d = df * 16 + 4 * g;
            if (d < D) {
                uint2 v;
                v.x = pack_bf2(snap[df][0], snap[df][1]);
                v.y = pack_bf2(snap[df][2], snap[df][3]);
                *reinterpret_cast<uint2*>(op + d) = v;
            }
        }
    }
}

static bool g_ja_attr_done = false;

template <int D>
static hipError_t ja_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_joint_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               JAGeom<D>::LDS);
}

static bool ja_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

extern "C" int msd_attention_joint(const MsdAttentionJoint* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "attention_joint: null argument");
    if (!p->q || !p->k || !p->vt || !p->k_ref || !p->vt_ref || !p->out)
        MSD_FAIL(MSD_E_ARG, "attention_joint: null q / k / vt / k_ref / vt_ref / out");
    if (!msd_aligned16(p->q) || !msd_aligned16(p->k) || !msd_aligned16(p->vt) || !msd_aligned16(p->k_ref) || !msd_aligned16(p->vt_ref) ||
        !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "attention_joint: q / k / vt / k_ref / vt_ref / out must be 16-byte aligned");
    if (p->mix && !msd_aligned16(p->mix)) MSD_FAIL(MSD_E_ARG, "attention_joint: mix must be 16-byte aligned");
    if (p->head_dim != 40 && p->head_dim != 80 && p->head_dim != 160)
        MSD_FAIL(MSD_E_ARG, "attention_joint: head_dim %d (40, 80 or 160)", p->head_dim);
    if (p->t < 1 || p->t_ref < 1 || p->s < 1) MSD_FAIL(MSD_E_ARG, "attention_joint: s = %d, t = %d, t_ref = %d (each >= 1)", p->s, p->t, p->t_ref);
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "attention_joint: batch %d (1 .. 65535)", p->batch);
    if (p->heads < 1 || p->heads > 65535) MSD_FAIL(MSD_E_ARG, "attention_joint: heads = %d (1 .. 65535)", p->heads);
    const int64_t C = (int64_t)p->heads * p->head_dim;
    if ((p->q_ld % 8) || (p->k_ld % 8) || (p->vt_ld % 8) || (p->o_ld % 8))
        MSD_FAIL(MSD_E_ARG, "attention_joint: q_ld / k_ld / vt_ld / o_ld must be multiples of 8");
    if (p->q_ld < C || p->k_ld < C || p->o_ld < C) MSD_FAIL(MSD_E_ARG, "attention_joint: q_ld / k_ld / o_ld smaller than heads * head_dim");
    if (p->vt_ld < p->t || p->vt_ld < p->t_ref)
        MSD_FAIL(MSD_E_ARG, "attention_joint: vt_ld = %d < max(t, t_ref) = %d", p->vt_ld, p->t > p->t_ref ? p->t : p->t_ref);
    const int64_t qtiles = ((int64_t)p->s + 63) / 64, wgs = qtiles * p->heads * p->batch;
    if (wgs >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "attention_joint: 2^31 or more workgroups");
    {   // out lies apart from every input
        const int64_t rows = (int64_t)p->batch * p->s, krows = (int64_t)p->batch * p->t;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)(((rows - 1) * p->o_ld + C) * 2);
        const uintptr_t q0 = (uintptr_t)p->q, q1 = q0 + (uintptr_t)(((rows - 1) * p->q_ld + C) * 2);
        const uintptr_t k0 = (uintptr_t)p->k, k1 = k0 + (uintptr_t)(((krows - 1) * p->k_ld + C) * 2);
        const uintptr_t v0 = (uintptr_t)p->vt, v1 = v0 + (uintptr_t)((int64_t)p->batch * C * p->vt_ld * 2);
        const uintptr_t kr0 = (uintptr_t)p->k_ref, kr1 = kr0 + (uintptr_t)((((int64_t)p->t_ref - 1) * p->k_ld + C) * 2);
        const uintptr_t vr0 = (uintptr_t)p->vt_ref, vr1 = vr0 + (uintptr_t)(C * p->vt_ld * 2);
        bool bad = ja_overlap(o0, o1, q0, q1) || ja_overlap(o0, o1, k0, k1) || ja_overlap(o0, o1, v0, v1) ||
                   ja_overlap(o0, o1, kr0, kr1) || ja_overlap(o0, o1, vr0, vr1);
        if (p->mix) {
            const uintptr_t m0 = (uintptr_t)p->mix, m1 = m0 + (uintptr_t)p->batch * 4;
            bad = bad || ja_overlap(o0, o1, m0, m1);
        }
        if (bad) MSD_FAIL(MSD_E_ARG, "attention_joint: out overlaps an input");
    }
    if (!g_ja_attr_done) {
        hipError_t e = ja_attr<40>();
        if (e == hipSuccess) e = ja_attr<80>();
        if (e == hipSuccess) e = ja_attr<160>();
        if (e != hipSuccess) MSD_FAIL((int)e, "hipFuncSetAttribute(attention_joint): %s", hipGetErrorString(e));
        g_ja_attr_done = true;
    }
    JAArgs a;
    a.q = (const bf16_t*)p->q; a.k = (const bf16_t*)p->k; a.vt = (const bf16_t*)p->vt;
    a.k_ref = (const bf16_t*)p->k_ref; a.vt_ref = (const bf16_t*)p->vt_ref; a.mix = p->mix; a.out = (bf16_t*)p->out;
    a.batch = p->batch; a.heads = p->heads; a.s = p->s; a.t = p->t; a.t_ref = p->t_ref;
    a.q_ld = p->q_ld; a.k_ld = p->k_ld; a.vt_ld = p->vt_ld; a.o_ld = p->o_ld;
    const dim3 grid((unsigned)wgs);
    switch (p->head_dim) {
        case 40: hipLaunchKernelGGL(attention_joint_kernel<40>, grid, dim3(256), JAGeom<40>::LDS, stream, a); break;
        case 80: hipLaunchKernelGGL(attention_joint_kernel<80>, grid, dim3(256), JAGeom<80>::LDS, stream, a); break;
        default: hipLaunchKernelGGL(attention_joint_kernel<160>, grid, dim3(256), JAGeom<160>::LDS, stream, a); break;
    }
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}

// ---- msd_reference_latent: the reference row's UNet input of this step, x_r = a z_ref + b n_ref ---------------------------------
__global__ __launch_bounds__(256) void reference_latent_kernel(const float4* z, const float4* noise, const float* coef, const int32_t* step_ptr,
                                                               float4* out, int n4, int num_steps) {
    int step = step_ptr ? *step_ptr : 0;
    if (step > num_steps - 1) step = num_steps - 1;
    if (step < 0) step = 0;
    const float a = coef[2 * step], b = coef[2 * step + 1];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 zv = z[i], nv = noise[i];
    float4 r;
    r.x = __fmaf_rn(b, nv.x, __fmul_rn(a, zv.x));
    r.y = __fmaf_rn(b, nv.y, __fmul_rn(a, zv.y));
    r.z = __fmaf_rn(b, nv.z, __fmul_rn(a, zv.z));
    r.w = __fmaf_rn(b, nv.w, __fmul_rn(a, zv.w));
    out[i] = r;
}

extern "C" int msd_reference_latent(const MsdReferenceLatent* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "reference_latent: null argument");
    if (!p->z || !p->noise || !p->coef || !p->out) MSD_FAIL(MSD_E_ARG, "reference_latent: null z / noise / coef / out");
    if (!msd_aligned16(p->z) || !msd_aligned16(p->noise) || !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "reference_latent: z / noise / out must be 16-byte aligned");
    if (p->n < 4 || (p->n % 4) || p->num_steps < 1) MSD_FAIL(MSD_E_ARG, "reference_latent: n = %d (a positive multiple of 4), num_steps = %d (>= 1)", p->n, p->num_steps);
    {
        const uintptr_t nb = (uintptr_t)p->n * 4, o0 = (uintptr_t)p->out, z0 = (uintptr_t)p->z, n0 = (uintptr_t)p->noise;
        const uintptr_t c0 = (uintptr_t)p->coef, cb = (uintptr_t)p->num_steps * 8;
        if (ja_overlap(o0, o0 + nb, z0, z0 + nb) || ja_overlap(o0, o0 + nb, n0, n0 + nb) || ja_overlap(z0, z0 + nb, n0, n0 + nb) ||
            ja_overlap(o0, o0 + nb, c0, c0 + cb))
            MSD_FAIL(MSD_E_ARG, "reference_latent: z, noise and out must be distinct (and out apart from coef)");
        if (p->step_ptr && ja_overlap(o0, o0 + nb, (uintptr_t)p->step_ptr, (uintptr_t)p->step_ptr + 4))
            MSD_FAIL(MSD_E_ARG, "reference_latent: out overlaps step_ptr");
    }
    const int n4 = p->n / 4;
    hipLaunchKernelGGL(reference_latent_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, (const float4*)p->z,
                       (const float4*)p->noise, p->coef, p->step_ptr, (float4*)p->out, n4, p->num_steps);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
