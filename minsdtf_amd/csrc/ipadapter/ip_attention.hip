// msdi_attention_decoupled: the decoupled cross-attention of an IP-Adapter image prompt (include/minsdtf_hip_ipadapter.h has the
// operands and the pinned arithmetic, minsdtf_amd/ipadapter.py attention_reference the float64 statement, DESIGN.md 4.18 the budget).
//
//   out(q) = softmax(q K_text^T) V_text + sc * softmax(q K_ip^T) V_ip        sc = scales[*step_ptr][layer]
//
// A fork of region_attention_kernel's transposed products (../region_attn.hip): S^T[key, q] = K Q^T and O^T[d, q] = V^T P^T on
// 16x16x32 MFMAs, the query on the MFMA column, so a lane owns ONE query and both of its softmaxes are lane-local (plus two
// shuffles across the four key groups).  Both segments live in the ONE 96-key tile the cross-attention kernels use: the text keys at
// rows [0, t), the image keys at rows [t8, t8 + n) with t8 = roundup8(t) - so a 16-byte chunk of a V^T row belongs to one
// segment - and the launch is one S^T product, two row maxima and two row sums per lane, ONE O^T product over
// [P_text / l_text | sc * P_ip / l_ip] and one store.  Both maxima are true maxima: no online softmax.  A key row of neither segment
// (t .. t8 - 1, and everything behind t8 + n) gets probability exactly 0 by its INDEX, and its V^T column is staged as 0.
//
// Work split: one workgroup = 4 waves = 64 queries of one (sample, head); a wave owns 16 queries (one MFMA column block) at every
// head size.  sc is read once, from the table, by every lane alike: with sc == 0 the workgroup stages no image key at all (n is
// taken as 0), so k_ip / vt_ip are not read and the launch is the text attention.  No atomics, no scratch, no workspace.
#include "../common.h"
#include "../../../include/minsdtf_hip_ipadapter.h"

struct IAArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* vt; const bf16_t* k_ip; const bf16_t* vt_ip; bf16_t* out;
    const float* scales; const int32_t* step_ptr;
    int batch, heads, s, t, n, q_ld, k_ld, vt_ld, kip_ld, vtip_ld, o_ld, layer, num_steps;
};

#define IA_KEYS MSDI_KEYS

template <int D>
struct IAGeom {
    static constexpr int DPAD = ((D + 31) / 32) * 32;   // QK^T k-dimension, zero-padded to whole 32-channel MFMA steps
    static constexpr int KS = DPAD / 32;
    static constexpr int DF = (D + 15) / 16;             // 16-row blocks of O^T
    static constexpr int KROW = DPAD * 2 + 16;           // bytes; an odd number of 16-byte slots: conflict-free fragment reads
    static constexpr int VROW = IA_KEYS * 2 + 16;        // 13 slots
    static constexpr int DCH = D / 8;                    // 16-byte chunks of a K row
    static constexpr int K_BYTES = IA_KEYS * KROW;
    static constexpr int LDS = K_BYTES + DF * 16 * VROW;
};
static_assert(IAGeom<160>::LDS <= 64 * 1024 && IAGeom<80>::LDS <= 64 * 1024 && IAGeom<40>::LDS <= 64 * 1024, "LDS budget");

// the first `valid` (< 8) bf16 of a 16-byte chunk kept, the rest forced to 0: the columns behind a segment's last key are padding
__device__ __forceinline__ uint4 ia_keep(uint4 v, int valid) {
    uint32_t* u = reinterpret_cast<uint32_t*>(&v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (2 * j >= valid) u[j] = 0;
        else if (2 * j + 1 >= valid) u[j] &= 0xFFFFu;
    }
    return v;
}

template <int D>
__global__ __launch_bounds__(256) void ip_attention_kernel(const IAArgs p) {
    using G = IAGeom<D>;
    constexpr int KS = G::KS, DF = G::DF, KROW = G::KROW, VROW = G::VROW, DCH = G::DCH;
    constexpr int NKF = IA_KEYS / 16, NKK = IA_KEYS / 32, VCHUNKS = IA_KEYS / 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const sK = smem;
    char* const sV = smem + G::K_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, g = lane >> 4;
    // all query tiles of one (sample, head) on one XCD: its K / V^T stay in that XCD's L2
    const int qtiles = (p.s + 63) / 64;
    const int wi = xcd_remap(blockIdx.x, qtiles * p.heads * p.batch);
    const int bh = wi / qtiles, b = bh / p.heads, h = bh - b * p.heads;
    const int qwg = (wi - bh * qtiles) * 64;      // first query of the workgroup
    const int qrow = qwg + wave * 16 + r;         // this lane's query

    // the scale of this launch: one table entry, the same for every lane of every workgroup
    int step = p.step_ptr ? *p.step_ptr : 0;
    step = min(max(step, 0), p.num_steps - 1);
    const float sc = p.scales[(size_t)step * MSDI_LAYERS + p.layer];
    const int t = p.t, t8 = (t + 7) & ~7;
    const int n = sc == 0.0f ? 0 : p.n;           // sc == 0: no image key exists for this launch, none is loaded
    const int tend = t8 + n;                      // one past the last key row in use (<= IA_KEYS)

    // zero the LDS image once: the pad columns of K (d = 40 / 80) and the pad rows of V^T are never written afterwards (the
    // barrier orders the fill in front of the staging stores)
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

    constexpr int KCH = (IA_KEYS * DCH + 255) / 256, VCH = (D * VCHUNKS + 255) / 256;
    {
        const bf16_t* kbase = p.k + (size_t)b * t * p.k_ld + h * D;
        const bf16_t* vbase = p.vt + ((size_t)b * p.heads + h) * D * p.vt_ld;
        const bf16_t* kibase = p.k_ip + (size_t)b * p.n * p.kip_ld + h * D;
        const bf16_t* vibase = p.vt_ip + ((size_t)b * p.heads + h) * D * p.vtip_ld;
        uint4 rk[KCH], rv[VCH];
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int idx = tid + 256 * i, row = idx / DCH, ch = idx - row * DCH;
            rk[i] = make_uint4(0, 0, 0, 0);
            if (idx < IA_KEYS * DCH) {
                if (row < t) rk[i] = *reinterpret_cast<const uint4*>(kbase + (size_t)row * p.k_ld + ch * 8);
                else if (row >= t8 && row < tend) rk[i] = *reinterpret_cast<const uint4*>(kibase + (size_t)(row - t8) * p.kip_ld + ch * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int idx = tid + 256 * i, d = idx / VCHUNKS, c0 = (idx - d * VCHUNKS) * 8;   // c0: the chunk's first key row
            rv[i] = make_uint4(0, 0, 0, 0);
            if (idx < D * VCHUNKS) {
                // (c0 < t <= vt_ld, c0 - t8 < n <= vtip_ld and both multiples of 8: the 16 bytes lie inside the row)
                if (c0 < t) rv[i] = ia_keep(*reinterpret_cast<const uint4*>(vbase + (size_t)d * p.vt_ld + c0), min(t - c0, 8));
                else if (c0 >= t8 && c0 < tend)
                    rv[i] = ia_keep(*reinterpret_cast<const uint4*>(vibase + (size_t)d * p.vtip_ld + (c0 - t8)), min(tend - c0, 8));
            }
        }
        __syncthreads();   // the zero fill is complete
#pragma unroll
        for (int i = 0; i < KCH; ++i) {
            const int idx = tid + 256 * i, row = idx / DCH, ch = idx - row * DCH;
            if (idx < IA_KEYS * DCH) *reinterpret_cast<uint4*>(sK + row * KROW + ch * 16) = rk[i];
        }
#pragma unroll
        for (int i = 0; i < VCH; ++i) {
            const int idx = tid + 256 * i, d = idx / VCHUNKS, ch = idx - d * VCHUNKS;
            if (idx < D * VCHUNKS) *reinterpret_cast<uint4*>(sV + d * VROW + ch * 16) = rv[i];
        }
    }
    __syncthreads();

    // S^T = K Q^T (q carries scale * log2(e)); lane holds keys kf * 16 + 4 g + e of query r
    f32x4 s[NKF];
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) {
        s[kf] = (f32x4){0, 0, 0, 0};
        if (kf * 16 < tend) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const bf16x8 kfrag = *reinterpret_cast<const bf16x8*>(sK + (kf * 16 + r) * KROW + ks * 64 + g * 16);
                s[kf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag, qf[ks], s[kf], 0, 0, 0);
            }
        }
    }
    // the two maxima: every key row is text (< t), image (t8 <= . < tend) or neither, by its index alone
    float mt = -1e30f, mi = -1e30f;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = kf * 16 + 4 * g + e;
            if (key < t) mt = fmaxf(mt, s[kf][e]);
            else if (key >= t8 && key < tend) mi = fmaxf(mi, s[kf][e]);
        }
    mt = fmaxf(mt, __shfl_xor(mt, 16));
    mt = fmaxf(mt, __shfl_xor(mt, 32));
    mi = fmaxf(mi, __shfl_xor(mi, 16));
    mi = fmaxf(mi, __shfl_xor(mi, 32));

    // the exponentials in place (neither segment: exactly 0) and the two fp32 row sums
    float lt = 0.f, li = 0.f;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int key = kf * 16 + 4 * g + e;
            float pe = 0.f;
            if (key < t) { pe = __builtin_amdgcn_exp2f(s[kf][e] - mt); lt += pe; }
            else if (key >= t8 && key < tend) { pe = __builtin_amdgcn_exp2f(s[kf][e] - mi); li += pe; }
            s[kf][e] = pe;
        }
    lt += __shfl_xor(lt, 16);
    lt += __shfl_xor(lt, 32);
    li += __shfl_xor(li, 16);
    li += __shfl_xor(li, 32);
    const float ct = 1.0f / lt;                       // t >= 1: lt >= 1
    const float ci = n > 0 ? sc / li : 0.f;           // n >= 1: li >= 1

    // O^T = V^T P^T over the whole tile, P normalised (and the image part scaled) before its one rounding to bf16
    f32x4 o[DF];
#pragma unroll
    for (int df = 0; df < DF; ++df) o[df] = (f32x4){0, 0, 0, 0};
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
        if (kk * 32 >= tend) continue;
        union { bf16x8 v; uint32_t u[4]; } pk;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int kf = 2 * kk + j;
            const float c = kf * 16 + 4 * g < t ? ct : ci;   // (t8 is a multiple of 8: a lane's four keys whose first is >= t hold no text key, and the others' non-text keys are 0)
            const f32x4 sv = s[kf];
            pk.u[2 * j] = pack_bf2(__fmul_rn(sv[0], c), __fmul_rn(sv[1], c));
            pk.u[2 * j + 1] = pack_bf2(__fmul_rn(sv[2], c), __fmul_rn(sv[3], c));
        }
#pragma unroll
        for (int df = 0; df < DF; ++df) {
            union { bf16x8 v; uint2 h2[2]; } vf;
            const char* vp = sV + (df * 16 + r) * VROW + kk * 64 + g * 8;
            vf.h2[0] = *reinterpret_cast<const uint2*>(vp);
            vf.h2[1] = *reinterpret_cast<const uint2*>(vp + 32);
            o[df] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, pk.v, o[df], 0, 0, 0);
        }
    }

    if (qrow < p.s) {
        bf16_t* op = p.out + ((size_t)b * p.s + qrow) * p.o_ld + h * D;
#pragma unroll
        for (int df = 0; df < DF; ++df) {
            const int d = df * 16 + 4 * g;
            if (d < D) {
                uint2 v;
                v.x = pack_bf2(o[df][0], o[df][1]);
                v.y = pack_bf2(o[df][2], o[df][3]);
                *reinterpret_cast<uint2*>(op + d) = v;
            }
        }
    }
}

static bool g_ia_attr_done = false;

template <int D>
static hipError_t ia_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&ip_attention_kernel<D>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               IAGeom<D>::LDS);
}

static bool ia_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

extern "C" int msdi_attention_decoupled(const MsdiAttentionDecoupled* p, msdi_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "attention_decoupled: null argument");
    if (!p->q || !p->k || !p->vt || !p->k_ip || !p->vt_ip || !p->out || !p->scales)
        MSD_FAIL(MSD_E_ARG, "attention_decoupled: null q / k / vt / k_ip / vt_ip / out / scales");
    if (!msd_aligned16(p->q) || !msd_aligned16(p->k) || !msd_aligned16(p->vt) || !msd_aligned16(p->k_ip) || !msd_aligned16(p->vt_ip) ||
        !msd_aligned16(p->out) || !msd_aligned16(p->scales))
        MSD_FAIL(MSD_E_ARG, "attention_decoupled: q / k / vt / k_ip / vt_ip / out / scales must be 16-byte aligned");
    if (((uintptr_t)p->step_ptr) & 3u) MSD_FAIL(MSD_E_ARG, "attention_decoupled: step_ptr must be 4-byte aligned");
    if (p->head_dim != 40 && p->head_dim != 80 && p->head_dim != 160)
        MSD_FAIL(MSD_E_ARG, "attention_decoupled: head_dim %d (40, 80 or 160)", p->head_dim);
    if (p->t < 1 || p->t > MSDI_KEYS) MSD_FAIL(MSD_E_ARG, "attention_decoupled: t = %d text keys (1 .. %d)", p->t, MSDI_KEYS);
    if (p->n < 1 || p->n > MSDI_MAX_TOKENS) MSD_FAIL(MSD_E_ARG, "attention_decoupled: n = %d image keys (1 .. %d)", p->n, MSDI_MAX_TOKENS);
    if ((p->t + 7) / 8 * 8 + p->n > MSDI_KEYS)
        MSD_FAIL(MSD_E_ARG, "attention_decoupled: roundup8(t = %d) + n = %d keys exceed the one tile of %d", p->t, p->n, MSDI_KEYS);
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "attention_decoupled: batch %d (1 .. 65535)", p->batch);
    if (p->heads < 1 || p->heads > 65535 || p->s < 1)
        MSD_FAIL(MSD_E_ARG, "attention_decoupled: heads = %d (1 .. 65535), s = %d (>= 1)", p->heads, p->s);
    if (p->layer < 0 || p->layer >= MSDI_LAYERS) MSD_FAIL(MSD_E_ARG, "attention_decoupled: layer %d (0 .. %d)", p->layer, MSDI_LAYERS - 1);
    if (p->num_steps < 1) MSD_FAIL(MSD_E_ARG, "attention_decoupled: num_steps %d (>= 1)", p->num_steps);
    const int64_t C = (int64_t)p->heads * p->head_dim;
    if ((p->q_ld % 8) || (p->k_ld % 8) || (p->vt_ld % 8) || (p->kip_ld % 8) || (p->vtip_ld % 8) || (p->o_ld % 8))
        MSD_FAIL(MSD_E_ARG, "attention_decoupled: q_ld / k_ld / vt_ld / kip_ld / vtip_ld / o_ld must be multiples of 8");
    if (p->q_ld < C || p->k_ld < C || p->kip_ld < C || p->o_ld < C)
        MSD_FAIL(MSD_E_ARG, "attention_decoupled: q_ld / k_ld / kip_ld / o_ld smaller than heads * head_dim");
    if (p->vt_ld < p->t) MSD_FAIL(MSD_E_ARG, "attention_decoupled: vt_ld = %d < t = %d", p->vt_ld, p->t);
    if (p->vtip_ld < p->n) MSD_FAIL(MSD_E_ARG, "attention_decoupled: vtip_ld = %d < n = %d", p->vtip_ld, p->n);
    const int64_t qtiles = ((int64_t)p->s + 63) / 64, wgs = qtiles * p->heads * p->batch;
    if (wgs >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "attention_decoupled: 2^31 or more workgroups");
    {   // out lies apart from every input
        const int64_t rows = (int64_t)p->batch * p->s;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)(((rows - 1) * p->o_ld + C) * 2);
        const uintptr_t q0 = (uintptr_t)p->q, q1 = q0 + (uintptr_t)(((rows - 1) * p->q_ld + C) * 2);
        const uintptr_t k0 = (uintptr_t)p->k, k1 = k0 + (uintptr_t)((((int64_t)p->batch * p->t - 1) * p->k_ld + C) * 2);
        const uintptr_t v0 = (uintptr_t)p->vt, v1 = v0 + (uintptr_t)((int64_t)p->batch * C * p->vt_ld * 2);
        const uintptr_t ki0 = (uintptr_t)p->k_ip, ki1 = ki0 + (uintptr_t)((((int64_t)p->batch * p->n - 1) * p->kip_ld + C) * 2);
        const uintptr_t vi0 = (uintptr_t)p->vt_ip, vi1 = vi0 + (uintptr_t)((int64_t)p->batch * C * p->vtip_ld * 2);
        const uintptr_t s0 = (uintptr_t)p->scales, s1 = s0 + (uintptr_t)p->num_steps * MSDI_LAYERS * 4;
        const uintptr_t c0 = (uintptr_t)p->step_ptr;
        if (ia_overlap(o0, o1, q0, q1) || ia_overlap(o0, o1, k0, k1) || ia_overlap(o0, o1, v0, v1) || ia_overlap(o0, o1, ki0, ki1) ||
            ia_overlap(o0, o1, vi0, vi1) || ia_overlap(o0, o1, s0, s1) || (p->step_ptr && ia_overlap(o0, o1, c0, c0 + 4)))
            MSD_FAIL(MSD_E_ARG, "attention_decoupled: out overlaps an input");
    }
    if (!g_ia_attr_done) {
        hipError_t e = ia_attr<40>();
        if (e == hipSuccess) e = ia_attr<80>();
        if (e == hipSuccess) e = ia_attr<160>();
        if (e != hipSuccess) MSD_FAIL((int)e, "hipFuncSetAttribute(attention_decoupled): %s", hipGetErrorString(e));
        g_ia_attr_done = true;
    }
    IAArgs a;
    a.q = (const bf16_t*)p->q; a.k = (const bf16_t*)p->k; a.vt = (const bf16_t*)p->vt;
    a.k_ip = (const bf16_t*)p->k_ip; a.vt_ip = (const bf16_t*)p->vt_ip; a.out = (bf16_t*)p->out;
    a.scales = p->scales; a.step_ptr = p->step_ptr;
    a.batch = p->batch; a.heads = p->heads; a.s = p->s; a.t = p->t; a.n = p->n;
    a.q_ld = p->q_ld; a.k_ld = p->k_ld; a.vt_ld = p->vt_ld; a.kip_ld = p->kip_ld; a.vtip_ld = p->vtip_ld; a.o_ld = p->o_ld;
    a.layer = p->layer; a.num_steps = p->num_steps;
    const dim3 grid((unsigned)wgs);
    switch (p->head_dim) {
        case 40: hipLaunchKernelGGL(ip_attention_kernel<40>, grid, dim3(256), IAGeom<40>::LDS, stream, a); break;
        case 80: hipLaunchKernelGGL(ip_attention_kernel<80>, grid, dim3(256), IAGeom<80>::LDS, stream, a); break;
        default: hipLaunchKernelGGL(ip_attention_kernel<160>, grid, dim3(256), IAGeom<160>::LDS, stream, a); break;
    }
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
