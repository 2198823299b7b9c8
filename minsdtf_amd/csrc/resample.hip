// msd_latent_resample: separable four-tap resampling of the fp32 NHWC latent (C = 4) fused with the re-noise of a hires job's
// hand-off (include/minsdtf_hip.h has the formula and the pinned order of the sums; minsdtf_amd/hires.py builds the tap rows).
//
// One lane = one output pixel = one float4.  The two tap rows of a pixel are four 16-byte loads (a wave's 64 lanes walk
// consecutive wx rows and share one or two wy rows), its sixteen source pixels sixteen 16-byte loads that hit L2 (the largest source,
// 96 x 96 x 4 fp32 per sample, is 144 KB), the result one 16-byte store.  The largest launch (128 x 128 outputs per sample) is
// 64 workgroups per sample: the kernel sits at the launch floor, which is the point - the hand-off stays stream-ordered device
// work between two captured loops.  Nothing couples two pixels, so a sample's bits do not depend on its batch.
#include "common.h"

#define RS_THREADS 256

// (a * b rounded once: never contracted into a neighbouring add)
__device__ __forceinline__ float4 rs_mul(float w, const float4& p) {
    return make_float4(__fmul_rn(w, p.x), __fmul_rn(w, p.y), __fmul_rn(w, p.z), __fmul_rn(w, p.w));
}
__device__ __forceinline__ float4 rs_fma(float w, const float4& p, const float4& acc) {
    return make_float4(__fmaf_rn(w, p.x, acc.x), __fmaf_rn(w, p.y, acc.y), __fmaf_rn(w, p.z, acc.z), __fmaf_rn(w, p.w, acc.w));
}

template <bool NOISE>
__global__ __launch_bounds__(RS_THREADS) void latent_resample_kernel(const float4* __restrict__ in, float4* __restrict__ out,
                                                                     const float4* __restrict__ noise, const MsdResampleRow* __restrict__ wx,
                                                                     const MsdResampleRow* __restrict__ wy, int h_in, int w_in, int h_out,
                                                                     int w_out, float a, float s) {
    // grid: x = RS_THREADS consecutive pixels of a sample's output (row-major), y = sample
    const int pix = blockIdx.x * RS_THREADS + threadIdx.x;
    if (pix >= h_out * w_out) return;
    const int y = pix / w_out, x = pix - y * w_out;
    const int b = blockIdx.y;
    const int4 ix = *reinterpret_cast<const int4*>(wx[x].idx);
    const float4 fx = *reinterpret_cast<const float4*>(wx[x].w);
    const int4 iy = *reinterpret_cast<const int4*>(wy[y].idx);
    const float4 fy = *reinterpret_cast<const float4*>(wy[y].w);
    // (the rows arrive clamped; clamping again costs eight v_med3 and keeps a bad table inside `in`)
    const int cx[4] = {min(max(ix.x, 0), w_in - 1), min(max(ix.y, 0), w_in - 1), min(max(ix.z, 0), w_in - 1), min(max(ix.w, 0), w_in - 1)};
    const int cy[4] = {min(max(iy.x, 0), h_in - 1), min(max(iy.y, 0), h_in - 1), min(max(iy.z, 0), h_in - 1), min(max(iy.w, 0), h_in - 1)};
    const float wxv[4] = {fx.x, fx.y, fx.z, fx.w};
    const float wyv[4] = {fy.x, fy.y, fy.z, fy.w};
    const float4* src = in + (int64_t)b * h_in * w_in;
    float4 p[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) p[j][i] = src[(int64_t)cy[j] * w_in + cx[i]];   // all sixteen loads in flight before the first sum
    float4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float4 r = rs_mul(wxv[0], p[j][0]);
#pragma unroll
        for (int i = 1; i < 4; ++i) r = rs_fma(wxv[i], p[j][i], r);
        v = j == 0 ? rs_mul(wyv[0], r) : rs_fma(wyv[j], r, v);
    }
    const int64_t o = ((int64_t)b * h_out + y) * w_out + x;
    float4 res = rs_mul(a, v);
    if (NOISE) res = rs_fma(s, noise[o], res);
    out[o] = res;
}

extern "C" int msd_latent_resample(const MsdLatentResample* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "latent_resample: null argument");
    if (!p->in || !p->out || !p->wx || !p->wy) MSD_FAIL(MSD_E_ARG, "latent_resample: null in / out / wx / wy");
    const int lim = 16384;
    if (p->batch <= 0 || p->batch > 65535 || p->h_in <= 0 || p->w_in <= 0 || p->h_out < p->h_in || p->w_out < p->w_in || p->h_out > lim ||
        p->w_out > lim)
        MSD_FAIL(MSD_E_ARG, "latent_resample: batch %d, %d x %d -> %d x %d (batch 1 .. 65535, sizes 1 .. %d, upscaling only)", p->batch, p->h_in,
                 p->w_in, p->h_out, p->w_out, lim);
    if ((int64_t)p->batch * p->h_out * p->w_out * 4 >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "latent_resample: 2^31 or more output elements");
    if (!msd_aligned16(p->in) || !msd_aligned16(p->out) || !msd_aligned16(p->noise) || !msd_aligned16(p->wx) || !msd_aligned16(p->wy))
        MSD_FAIL(MSD_E_ARG, "latent_resample: in / out / noise / wx / wy must be 16-byte aligned");
    {   // out must not overlap in: a pixel is read by many lanes
        const uintptr_t i0 = (uintptr_t)p->in, i1 = i0 + (uintptr_t)p->batch * p->h_in * p->w_in * 16;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)p->batch * p->h_out * p->w_out * 16;
        if (i0 < o1 && o0 < i1) MSD_FAIL(MSD_E_ARG, "latent_resample: out overlaps in");
    }
    const dim3 grid((unsigned)((p->h_out * p->w_out + RS_THREADS - 1) / RS_THREADS), (unsigned)p->batch);
    const float4* in = reinterpret_cast<const float4*>(p->in);
    float4* out = reinterpret_cast<float4*>(p->out);
    if (p->noise)
        hipLaunchKernelGGL(latent_resample_kernel<true>, grid, dim3(RS_THREADS), 0, stream, in, out, reinterpret_cast<const float4*>(p->noise),
                           p->wx, p->wy, p->h_in, p->w_in, p->h_out, p->w_out, p->a, p->s);
    else
        hipLaunchKernelGGL(latent_resample_kernel<false>, grid, dim3(RS_THREADS), 0, stream, in, out, (const float4*)nullptr, p->wx, p->wy,
                           p->h_in, p->w_in, p->h_out, p->w_out, p->a, p->s);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
