// msd_reference_adain: reference AdaIN of a reference-only job (include/minsdtf_hip.h has the formula and the pinned arithmetic;
// minsdtf_amd/reference.py the float64 statement).  Every generated row's feature map [hw][c] is renormalised, channel by
// channel, to the mean and standard deviation the reference row has at the same place, in place.
//
// A workgroup owns ONE generated row and a slab of AD_SLAB = 64 adjacent channels: 128 contiguous bytes of every pixel, read
// and written as 16 bytes per lane.  Lane l of wave w holds channel octet l & 7 and walks the pixels p = 8 w + (l >> 3),
// p + L, p + 2 L, ... in ascending order (L = 8 x waves pixel lanes): eight consecutive lanes cover a pixel's 128 bytes, a wave
// instruction eight pixels.  The lanes that share an octet are summed by cross-lane moves inside a wave (one DPP row rotate and
// the two row swaps: no LDS), the waves through LDS, always in ascending wave order, so the order of both reductions depends
// on hw alone.  Each workgroup recomputes the reference row's statistics for its own slab - with the same code, so a row that
// is a copy of the reference gets s = 1 and Bc = 0 exactly; the reference read is shared through L2 and costs no exchange, no
// buffer of statistics and no second launch.
//
// The launch is bound by latency, not by bytes (a site tensor of a 512 px job is 160 KB to 2.6 MB per row, and only rows x c / 64
// workgroups exist), so the forms are chosen to keep a workgroup's dependent round trips to memory few.  Up to AD_RESIDENT_HW =
// 1024 pixels BOTH slabs - the row's and the reference's - are loaded once, all loads in flight together, and stay in registers
// through the three passes (mean, squared deviations, apply): four waves, 32 pixel lanes, at most 32 pixels x 2 slabs x 16
// bytes = 256 VGPRs per lane, no scratch.  Above that sixteen waves read the slabs again in every pass (from L2: a 64-channel
// slab of 4096 pixels is 512 KB).  No cluster exchange, no atomics, no scratch, no workspace.
#include "common.h"

#define AD_SLAB 64            // channels of a workgroup
#define AD_RES_WAVES 4        // waves of a workgroup whose slabs stay in registers: 32 pixel lanes, up to 512 VGPRs per lane
#define AD_MAX_WAVES 16       // ... of a workgroup that reads its slabs again in every pass: 128 pixel lanes
#define AD_RESIDENT_HW 1024   // the largest hw whose slabs stay in registers

// sum over the 8 lanes of a wave that share (lane & 7), on every one of them, in a fixed order
__device__ __forceinline__ float octet_sum(float v) {
    v = __fadd_rn(v, MSD_DPP(v, 0x128));   // row_ror:8
    const uint32_t u = __float_as_uint(v);
    auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    v = __fadd_rn(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const uint32_t w = __float_as_uint(v);
    auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
    return __fadd_rn(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

// a[8] / b[8]: this lane's partial sums of its octet for the row and for the reference -> the workgroup's, on every lane
// (red: [waves][2][AD_SLAB], used once per call site: no barrier behind the reads)
template <int WAVES>
__device__ __forceinline__ void slab_sum(float* a, float* b, float (*red)[2][AD_SLAB], int wave, int lane) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        a[j] = octet_sum(a[j]);
        b[j] = octet_sum(b[j]);
    }
    if (lane < 8) {
        float4* da = reinterpret_cast<float4*>(&red[wave][0][lane * 8]);
        float4* db = reinterpret_cast<float4*>(&red[wave][1][lane * 8]);
        da[0] = make_float4(a[0], a[1], a[2], a[3]);
        da[1] = make_float4(a[4], a[5], a[6], a[7]);
        db[0] = make_float4(b[0], b[1], b[2], b[3]);
        db[1] = make_float4(b[4], b[5], b[6], b[7]);
    }
    __syncthreads();
    const int o = (lane & 7) * 8;
#pragma unroll
    for (int h = 0; h < 2; ++h) {   // (two float4s per operand; every lane of an octet reads the same addresses: broadcasts)
        float4 sa = *reinterpret_cast<const float4*>(&red[0][0][o + 4 * h]);
        float4 sb = *reinterpret_cast<const float4*>(&red[0][1][o + 4 * h]);
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const float4 ta = *reinterpret_cast<const float4*>(&red[w][0][o + 4 * h]);
            const float4 tb = *reinterpret_cast<const float4*>(&red[w][1][o + 4 * h]);
            sa = make_float4(__fadd_rn(sa.x, ta.x), __fadd_rn(sa.y, ta.y), __fadd_rn(sa.z, ta.z), __fadd_rn(sa.w, ta.w));
            sb = make_float4(__fadd_rn(sb.x, tb.x), __fadd_rn(sb.y, tb.y), __fadd_rn(sb.z, tb.z), __fadd_rn(sb.w, tb.w));
        }
        a[4 * h] = sa.x; a[4 * h + 1] = sa.y; a[4 * h + 2] = sa.z; a[4 * h + 3] = sa.w;
        b[4 * h] = sb.x; b[4 * h + 1] = sb.y; b[4 * h + 2] = sb.z; b[4 * h + 3] = sb.w;
    }
}

__device__ __forceinline__ void add8(float* s, const uint4& v) {
    float f[8];
    unpack8(v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = __fadd_rn(s[j], f[j]);
}
__device__ __forceinline__ void dev8(float* q, const uint4& v, const float* mean) {
    float f[8];
    unpack8(v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float d = __fsub_rn(f[j], mean[j]);
        q[j] = __fmaf_rn(d, d, q[j]);
    }
}
__device__ __forceinline__ uint4 apply8(const uint4& v, const float* A, const float* Bc) {
    float f[8];
    unpack8(v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = __fmaf_rn(f[j], A[j], Bc[j]);
    return pack8(f);
}

// WAVES x 64 lanes, L = 8 WAVES pixel lanes.  NP > 0: both slabs in registers, hw <= L * NP.  NP = 0: read again in every pass.
// (x is written; ref lies apart from the rows of x: the host checks it)
template <int WAVES, int NP>
__global__ __launch_bounds__(WAVES * 64) void reference_adain_kernel(uint4* x, const uint4* __restrict__ ref,
                                                                    const float* __restrict__ mix, int hw, int c8, float inv_n, float eps) {
    // grid: x = slab of 64 channels, y = generated row
    constexpr int L = 8 * WAVES;
    __shared__ float red[2][WAVES][2][AD_SLAB];
    const int row = blockIdx.y;
    const float f = mix ? mix[row] : 0.0f;
    if (f == 1.0f) return;   // (uniform over the workgroup) the row is neither read nor written
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int oct = blockIdx.x * (AD_SLAB / 8) + (lane & 7);
    const bool on = oct < c8;   // (c need not be a multiple of 64: the last slab's tail lanes add zeros)
    const int p0 = wave * 8 + (lane >> 3);
    uint4* xr = x + (int64_t)row * hw * c8 + oct;   // pixel p of this lane's octet: xr[p * c8]; hw * c < 2^31
    const uint4* rr = ref + oct;

    constexpr int NR = NP > 0 ? NP : 1;
    uint4 xv[NR], rv[NR];
    float sx[8], sr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sx[j] = sr[j] = 0.0f;
    if (on) {
        if constexpr (NP > 0) {
#pragma unroll
            for (int i = 0; i < NP; ++i) {   // (every load of both slabs in flight before the first add)
                const int p = p0 + i * L;
                if (p < hw) {
                    xv[i] = xr[p * c8];
                    rv[i] = rr[p * c8];
                }
            }
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (p0 + i * L < hw) {
                    add8(sx, xv[i]);
                    add8(sr, rv[i]);
                }
        } else {
#pragma unroll 4
            for (int p = p0; p < hw; p += L) {
                add8(sx, xr[p * c8]);
                add8(sr, rr[p * c8]);
            }
        }
    }
    slab_sum<WAVES>(sx, sr, red[0], wave, lane);
    float mx[8], mr[8], qx[8], qr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        mx[j] = __fmul_rn(sx[j], inv_n);
        mr[j] = __fmul_rn(sr[j], inv_n);
        qx[j] = qr[j] = 0.0f;
    }
    if (on) {
        if constexpr (NP > 0) {
#pragma unroll
            for (int i = 0; i < NP; ++i)
                if (p0 + i * L < hw) {
                    dev8(qx, xv[i], mx);
                    dev8(qr, rv[i], mr);
                }
        } else {
#pragma unroll 4
            for (int p = p0; p < hw; p += L) {
                dev8(qx, xr[p * c8], mx);
                dev8(qr, rr[p * c8], mr);
            }
        }
    }
    slab_sum<WAVES>(qx, qr, red[1], wave, lane);
    if (!on) return;
    const float g = __fsub_rn(1.0f, f);
    float A[8], Bc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float sd_x = __fsqrt_rn(__fadd_rn(fmaxf(__fmul_rn(qx[j], inv_n), 0.0f), eps));
        const float sd_r = __fsqrt_rn(__fadd_rn(fmaxf(__fmul_rn(qr[j], inv_n), 0.0f), eps));
        const float s = __fdiv_rn(sd_r, sd_x);
        A[j] = __fmaf_rn(g, s, f);
        Bc[j] = __fmul_rn(g, __fmaf_rn(-mx[j], s, mr[j]));
    }
    if constexpr (NP > 0) {
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int p = p0 + i * L;
            if (p < hw) xr[p * c8] = apply8(xv[i], A, Bc);
        }
    } else {
#pragma unroll 4
        for (int p = p0; p < hw; p += L) xr[p * c8] = apply8(xr[p * c8], A, Bc);
    }
}

extern "C" int msd_reference_adain(const MsdReferenceAdain* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "reference_adain: null argument");
    if (!p->x || !p->ref) MSD_FAIL(MSD_E_ARG, "reference_adain: null x / ref");
    if (!msd_aligned16(p->x) || !msd_aligned16(p->ref) || !msd_aligned16(p->mix))
        MSD_FAIL(MSD_E_ARG, "reference_adain: x / ref / mix must be 16-byte aligned");
    if (p->rows < 1 || p->rows > 65535) MSD_FAIL(MSD_E_ARG, "reference_adain: rows = %d (1 .. 65535)", p->rows);
    if (p->hw < 1) MSD_FAIL(MSD_E_ARG, "reference_adain: hw = %d (at least 1)", p->hw);
    if (p->c < 8 || (p->c % 8)) MSD_FAIL(MSD_E_ARG, "reference_adain: c = %d (a positive multiple of 8)", p->c);
    if (!(p->eps > 0.0f) || !(p->eps <= 3.4028234e38f)) MSD_FAIL(MSD_E_ARG, "reference_adain: eps = %g (finite and positive)", (double)p->eps);
    const int64_t row_elems = (int64_t)p->hw * p->c;
    if (row_elems >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "reference_adain: 2^31 or more elements in a row");
    {   // the reference row lies apart from the rows that are rewritten (directly behind them is the engine's layout)
        const uintptr_t x0 = (uintptr_t)p->x, x1 = x0 + (uintptr_t)p->rows * (uintptr_t)row_elems * 2;
        const uintptr_t r0 = (uintptr_t)p->ref, r1 = r0 + (uintptr_t)row_elems * 2;
        if (r0 < x1 && x0 < r1) MSD_FAIL(MSD_E_ARG, "reference_adain: ref overlaps the rows of x");
        if (p->mix) {
            const uintptr_t m0 = (uintptr_t)p->mix, m1 = m0 + (uintptr_t)p->rows * 4;
            if (m0 < x1 && x0 < m1) MSD_FAIL(MSD_E_ARG, "reference_adain: mix overlaps the rows of x");
        }
    }
    const int c8 = p->c / 8;
    const dim3 grid((unsigned)((p->c + AD_SLAB - 1) / AD_SLAB), (unsigned)p->rows);
    const float inv_n = 1.0f / (float)p->hw;
    uint4* x = reinterpret_cast<uint4*>(p->x);
    const uint4* ref = reinterpret_cast<const uint4*>(p->ref);
#define AD_LAUNCH(WAVES, NP) \
    hipLaunchKernelGGL((reference_adain_kernel<WAVES, NP>), grid, dim3(WAVES * 64), 0, stream, x, ref, p->mix, p->hw, c8, inv_n, p->eps)
    // (measured: with both slabs resident four waves beat eight and sixteen at hw = 256 and lose 7 % to eight at hw = 1024, whose
    // form spills)
    if (p->hw <= 64) AD_LAUNCH(AD_RES_WAVES, 2);
    else if (p->hw <= 256) AD_LAUNCH(AD_RES_WAVES, 8);
    else if (p->hw <= AD_RESIDENT_HW) AD_LAUNCH(AD_RES_WAVES, AD_RESIDENT_HW / (8 * AD_RES_WAVES));
    else AD_LAUNCH(AD_MAX_WAVES, 0);
#undef AD_LAUNCH
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
