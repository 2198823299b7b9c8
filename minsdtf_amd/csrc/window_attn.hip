// msd_attention_windowed: HyperTile - self-attention inside non-overlapping rectangular windows of the feature map
// (include/minsdtf_hip.h has the operands and the pinned properties, minsdtf_amd/hypertile.py the float64 statement, DESIGN.md 4.12
// the budget and the kernel choice).
//
//   token (y, x) of the h x w image belongs to window (y / wh, x / ww); inside a window queries and keys are numbered row-major,
//   j -> (j / ww, j % ww);  per sample, head and window:  out = softmax(q k^T) v  over that window's wh * ww keys only
//
// A fork of attention_joint_kernel (joint_attn.hip): the transposed products S^T[key, q] = K Q^T and O^T[d, q] = V^T P^T on
// 16x16x32 MFMAs, the query on the MFMA column, one query per lane, the online softmax with the rescale applied at every tile, K /
// V^T of a 64-key tile register-staged into one LDS image with the next tile's loads in flight under the products.  The only new
// idea is addressing: that kernel's staging already computes one global address per K row and per V^T chunk, here the address
// goes through the window map.  The operands stay where the q|k|v GEMM wrote them, in image order - nothing is gathered.
//
//   K row of window key j:        token(j) * k_ld,   token(j) = (wy * wh + j / ww) * w + wx * ww + j % ww
//   V^T chunk of keys j .. j + 7: column token(j) of the V^T row; ww % 8 == 0, so the 8 keys are one window row's and the 16 bytes
//                                 are aligned (w % 8 == 0 follows); wh * ww % 8 == 0, so a chunk is whole or absent
//
// Work split: one workgroup = 4 waves = 64 window-linear queries of one (sample, head, window); keys in window-linear order in
// 64-key tiles, the last one partial when wh * ww % 64 != 0 (its missing keys staged as zeros, their scores masked).  Nothing
// outside the window is ever addressed, so what other windows or the columns >= s of vt hold cannot reach the output, and the
// arithmetic is that of a launch with h = wh, w = ww on the window's gathered tokens, bit for bit.
#include <type_traits>
#include "common.h"

__device__ __forceinline__ float wa_rows_max(float v) {   // maximum over lanes l, l ^ 16, l ^ 32, l ^ 48 (joint_attn.hip)
    const uint32_t u = __float_as_uint(v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const uint32_t w = __float_as_uint(v);
    auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

struct WAArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* vt; bf16_t* out;
    int batch, heads, w, wh, ww, nw, nwin, q_ld, k_ld, vt_ld, o_ld;
    uint32_t ww_magic;   // udiv_magic_of(ww)
};

#define WA_KEYS 64   // keys of a tile

template <int D>
struct WAGeom {
    static constexpr int DPAD = ((D + 31) / 32) * 32;   // QK^T k-dimension, zero-padded to whole 32-channel MFMA steps
    static constexpr int KS = DPAD / 32;
    static constexpr int DF = (D + 15) / 16;             // 16-row blocks of O^T
    static constexpr int KROW = DPAD * 2 + 16;           // bytes; an odd number of 16-byte slots: conflict-free fragment reads
    static constexpr int VROW = WA_KEYS * 2 + 16;        // 9 slots
    static constexpr int DCH = D / 8;                    // 16-byte chunks of a K row
    static constexpr int K_BYTES = WA_KEYS * KROW;
    static constexpr int TILE = K_BYTES + DF * 16 * VROW;   // one tile's K and V^T image
    static constexpr int NBUF = D < 160 ? 2 : 1;            // as attention_joint_kernel: two images and one barrier per tile below d = 160
    static constexpr int LDS = NBUF * TILE;
};
static_assert(WAGeom<160>::LDS <= 64 * 1024 && WAGeom<80>::LDS <= 64 * 1024 && WAGeom<40>::LDS <= 64 * 1024, "LDS budget");

template <int D>
__global__ __launch_bounds__(256, D == 40 ? 4 : D == 80 ? 2 : 1) void attention_windowed_kernel(const WAArgs p) {
    using G = WAGeom<D>;
    constexpr int KS = G::KS, DF = G::DF, KROW = G::KROW, VROW = G::VROW, DCH = G::DCH;
    constexpr int NKF = WA_KEYS / 16, NKK = WA_KEYS / 32, VCHUNKS = WA_KEYS / 8;
    constexpr int KCH = (WA_KEYS * DCH + 255) / 256, VCH = (D * VCHUNKS + 255) / 256;
    constexpr int NBUF = G::NBUF;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int wlen = p.wh * p.ww;   // tokens of a window
    const int s = p.w * (p.nwin / p.nw) * p.wh;   // tokens of the image (h = nh * wh)
    // all windows and query tiles of one (sample, head) on one XCD: the head's K / V^T stays in that XCD's L2
    const int qtiles = (wlen + 63) / 64;
    const int per_bh = qtiles * p.nwin;
    const int wi = xcd_remap(blockIdx.x, per_bh * p.heads * p.batch);
    const int bh = wi / per_bh, b = bh / p.heads, h = bh - b * p.heads;
    const int rem = wi - bh * per_bh, win = rem / qtiles;
    const int wy = win / p.nw, wx = win - wy * p.nw;
    const int tok0 = wy * p.wh * p.w + wx * p.ww;   // the window's first token
    // window-linear index j (< wlen) -> token of the image
    auto token = [&](int j) {
        const int jy = udiv_magic(j, p.ww, p.ww_magic);
        return tok0 + jy * p.w + (j - jy * p.ww);
    };
    const int qj = (rem - win * qtiles) * 64 + wave * 16 + r;   // this lane's query, window-linear
    const int nt = (wlen + WA_KEYS - 1) / WA_KEYS;

    // zero the LDS image once: the pad columns of K (d = 40 / 80) and the pad rows of V^T are never written afterwards (the first
    // barrier of the tile loop orders the fill in front of the staging stores)
    for (int off = tid * 16; off < G::LDS; off += 256 * 16) *reinterpret_cast<uint4*>(smem + off) = make_uint4(0, 0, 0, 0);

    const int qtok = token(qj < wlen ? qj : wlen - 1);
    bf16x8 qf[KS];
    {
        const bf16_t* qp = p.q + ((size_t)b * s + qtok) * p.q_ld + h * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int d0 = ks * 32 + 8 * g;
            if (d0 < D) qf[ks] = *reinterpret_cast<const bf16x8*>(qp + d0);
            else qf[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
    }

    const bf16_t* const kbase = p.k + (size_t)b * s * p.k_ld + h * D;
    const bf16_t* const vbase = p.vt + ((size_t)b * p.heads + h) * D * p.vt_ld;

    uint4 rk[KCH], rv[VCH];
    // tile i of the walk -> registers; keys past the window's end come back as zeros (never read from memory)
    auto fetch = [&](int i) {
        const int key0 = i * WA_KEYS;
        const int left = wlen - key0;   // >= 1 keys of the window from key0 on
#pragma unroll
        for (int j = 0; j < KCH; ++j) {
            const int idx = tid + 256 * j, row = idx / DCH, ch = idx - row * DCH;
            rk[j] = make_uint4(0, 0, 0, 0);
            if (idx < WA_KEYS * DCH && row < left) rk[j] = *reinterpret_cast<const uint4*>(kbase + (size_t)token(key0 + row) * p.k_ld + ch * 8);
        }
        // (256 % VCHUNKS == 0: a thread's V^T chunks are the same 8 keys of VCH channels - one token per thread and tile.  The chunk
        // is whole or absent: wlen % 8 == 0.  Its 8 keys are consecutive tokens of one window row: ww % 8 == 0)
        const int vch = tid % VCHUNKS;
        const bool vin = vch * 8 < left;
        const bf16_t* const vb = vbase + token(vin ? key0 + vch * 8 : 0);
#pragma unroll
        for (int j = 0; j < VCH; ++j) {
            const int d = (tid + 256 * j) / VCHUNKS;
            rv[j] = make_uint4(0, 0, 0, 0);
            if (d < D && vin) rv[j] = *reinterpret_cast<const uint4*>(vb + (size_t)d * p.vt_ld);
        }
    };

    f32x4 o[DF];
#pragma unroll
    for (int df = 0; df < DF; ++df) o[df] = (f32x4){0, 0, 0, 0};
    float m = -1e30f;   // running maximum of this lane's query (the same on its four g lanes)
    float l = 0.f;      // this lane's share of the row sum (keys 4 g + e of every 16): reduced over g at the end

    // the fetched tile: registers -> LDS image `buf`
    auto stage = [&](int buf) {
        char* const dK = smem + buf * G::TILE;
        char* const dV = dK + G::K_BYTES;
#pragma unroll
        for (int j = 0; j < KCH; ++j) {
            const int idx = tid + 256 * j, row = idx / DCH, ch = idx - row * DCH;
            if (idx < WA_KEYS * DCH) *reinterpret_cast<uint4*>(dK + row * KROW + ch * 16) = rk[j];
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
    for (int i = 0; i < nt; ++i) {
        const int valid = wlen - i * WA_KEYS;   // keys of this tile (may exceed 64)
        const char* const sK = smem + (i % NBUF) * G::TILE;
        const char* const sV = sK + G::K_BYTES;

        __syncthreads();   // tile i is staged by every wave (two images: and every wave is through with tile i - 1, whose image tile i + 1 takes)
        if (i + 1 < nt) fetch(i + 1);   // in flight under this tile's products

        // the tile's arithmetic, compiled twice: FULL (all 64 keys, nothing masked) and partial (key fragments past `valid` skipped,
        // their scores masked).  On a full tile the two give the same bits.
        auto tile = [&](auto full_c) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_c)::value;
        // S^T = K Q^T (q carries scale * log2(e)); lane holds keys kf * 16 + 4 g + e of query r
        f32x4 sc[NKF];
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf) {
            sc[kf] = (f32x4){0, 0, 0, 0};
            if (FULL || kf * 16 < valid) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const bf16x8 kfrag = *reinterpret_cast<const bf16x8*>(sK + (kf * 16 + r) * KROW + ks * 64 + g * 16);
                    sc[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag, qf[ks], sc[kf], 0, 0, 0);
                }
            }
            if (!FULL) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (kf * 16 + 4 * g + e >= valid) sc[kf][e] = -1e30f;
            }
        }
        float mt = sc[0][0];
#pragma unroll
        for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
            for (int e = 0; e < 4; ++e) mt = fmaxf(mt, sc[kf][e]);
        mt = wa_rows_max(mt);
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
                const f32x4 sv = sc[2 * kk + j];
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
        // (d = 160 keeps the one masked form, as attention_joint_kernel does: two copies of its loop body cost registers)
        if (D < 160 && valid >= WA_KEYS) tile(std::true_type{});
        else tile(std::false_type{});

        if (i + 1 < nt) {
            if (NBUF == 1) __syncthreads();   // one image: tile i is consumed by every wave before tile i + 1 overwrites it
            stage((i + 1) % NBUF);
        }
    }

    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = 1.0f / l;

    if (qj < wlen) {
        bf16_t* op = p.out + ((size_t)b * s + qtok) * p.o_ld + h * D;
#pragma unroll
        for (int df = 0; df < DF; ++df) {
            const int d = df * 16 + 4 * g;
            if (d < D) {
                uint2 v;
                v.x = pack_bf2(__fmul_rn(o[df][0], inv), __fmul_rn(o[df][1], inv));
                v.y = pack_bf2(__fmul_rn(o[df][2], inv), __fmul_rn(o[df][3], inv));
                *reinterpret_cast<uint2*>(op + d) = v;
            }
        }
    }
}

static bool g_wa_attr_done = false;

template <int D>
static hipError_t wa_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_windowed_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               WAGeom<D>::LDS);
}

static bool wa_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

extern "C" int msd_attention_windowed(const MsdAttentionWindowed* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "attention_windowed: null argument");
    if (!p->q || !p->k || !p->vt || !p->out) MSD_FAIL(MSD_E_ARG, "attention_windowed: null q / k / vt / out");
    if (!msd_aligned16(p->q) || !msd_aligned16(p->k) || !msd_aligned16(p->vt) || !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "attention_windowed: q / k / vt / out must be 16-byte aligned");
    if (p->head_dim != 40 && p->head_dim != 80 && p->head_dim != 160)
        MSD_FAIL(MSD_E_ARG, "attention_windowed: head_dim %d (40, 80 or 160)", p->head_dim);
    if (p->h < 1 || p->w < 1 || p->wh < 1 || p->ww < 1)
        MSD_FAIL(MSD_E_ARG, "attention_windowed: h = %d, w = %d, wh = %d, ww = %d (each >= 1)", p->h, p->w, p->wh, p->ww);
    if ((p->h % p->wh) || (p->w % p->ww) || (p->ww % 8))
        MSD_FAIL(MSD_E_ARG, "attention_windowed: h = %d, w = %d, wh = %d, ww = %d (h %% wh == 0, w %% ww == 0, ww %% 8 == 0)", p->h, p->w,
                 p->wh, p->ww);
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "attention_windowed: batch %d (1 .. 65535)", p->batch);
    if (p->heads < 1 || p->heads > 65535) MSD_FAIL(MSD_E_ARG, "attention_windowed: heads = %d (1 .. 65535)", p->heads);
    const int64_t C = (int64_t)p->heads * p->head_dim, s = (int64_t)p->h * p->w;
    if ((p->q_ld % 8) || (p->k_ld % 8) || (p->vt_ld % 8) || (p->o_ld % 8))
        MSD_FAIL(MSD_E_ARG, "attention_windowed: q_ld / k_ld / vt_ld / o_ld must be multiples of 8");
    if (p->q_ld < C || p->k_ld < C || p->o_ld < C) MSD_FAIL(MSD_E_ARG, "attention_windowed: q_ld / k_ld / o_ld smaller than heads * head_dim");
    if (p->vt_ld < s) MSD_FAIL(MSD_E_ARG, "attention_windowed: vt_ld = %d < s = h * w = %lld", p->vt_ld, (long long)s);
    const int nh = p->h / p->wh, nw = p->w / p->ww;
    const int64_t wlen = (int64_t)p->wh * p->ww, qtiles = (wlen + 63) / 64, wgs = qtiles * nh * nw * p->heads * p->batch;
    if (wgs >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "attention_windowed: 2^31 or more workgroups");
    {   // out lies apart from every input
        const int64_t rows = (int64_t)p->batch * s;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)(((rows - 1) * p->o_ld + C) * 2);
        const uintptr_t q0 = (uintptr_t)p->q, q1 = q0 + (uintptr_t)(((rows - 1) * p->q_ld + C) * 2);
        const uintptr_t k0 = (uintptr_t)p->k, k1 = k0 + (uintptr_t)(((rows - 1) * p->k_ld + C) * 2);
        const uintptr_t v0 = (uintptr_t)p->vt, v1 = v0 + (uintptr_t)((int64_t)p->batch * C * p->vt_ld * 2);
        if (wa_overlap(o0, o1, q0, q1) || wa_overlap(o0, o1, k0, k1) || wa_overlap(o0, o1, v0, v1))
            MSD_FAIL(MSD_E_ARG, "attention_windowed: out overlaps an input");
    }
    if (!g_wa_attr_done) {
        hipError_t e = wa_attr<40>();
        if (e == hipSuccess) e = wa_attr<80>();
        if (e == hipSuccess) e = wa_attr<160>();
        if (e != hipSuccess) MSD_FAIL((int)e, "hipFuncSetAttribute(attention_windowed): %s", hipGetErrorString(e));
        g_wa_attr_done = true;
    }
    WAArgs a;
    a.q = (const bf16_t*)p->q; a.k = (const bf16_t*)p->k; a.vt = (const bf16_t*)p->vt; a.out = (bf16_t*)p->out;
    a.batch = p->batch; a.heads = p->heads; a.w = p->w; a.wh = p->wh; a.ww = p->ww; a.nw = nw; a.nwin = nh * nw;
    a.q_ld = p->q_ld; a.k_ld = p->k_ld; a.vt_ld = p->vt_ld; a.o_ld = p->o_ld;
    a.ww_magic = udiv_magic_of(p->ww);
    const dim3 grid((unsigned)wgs);
    switch (p->head_dim) {
        case 40: hipLaunchKernelGGL(attention_windowed_kernel<40>, grid, dim3(256), WAGeom<40>::LDS, stream, a); break;
        case 80: hipLaunchKernelGGL(attention_windowed_kernel<80>, grid, dim3(256), WAGeom<80>::LDS, stream, a); break;
        default: hipLaunchKernelGGL(attention_windowed_kernel<160>, grid, dim3(256), WAGeom<160>::LDS, stream, a); break;
    }
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
