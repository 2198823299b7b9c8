// msdx_sag_degrade: the degraded latent of a self-attention-guidance step (include/minsdtf_hip_ext.h has the formula and the pinned
// order; minsdtf_amd/sag.py degrade_host is the float64 statement).
//
// One workgroup = a 16 x 16 tile of one sample's latent, one lane = one pixel = one float4.  The tile's x0 with a 4-pixel reflected
// halo (24 x 24) goes through LDS, the horizontal pass writes 24 x 16 to LDS, the vertical pass and the blend stay in registers.
// A 64 x 64 latent is 16 workgroups per sample: the kernel sits at the launch floor, one more launch between the two UNet passes
// of the step, inside the captured graph.  Nothing couples two samples.
#include "../common.h"
#include "../../../include/minsdtf_hip_ext.h"

#define SD_T 16            // tile side
#define SD_R 4             // blur radius
#define SD_E (SD_T + 2 * SD_R)

struct SDArgs {
    const float4* latent;
    const float4* eps;
    const float* coef;
    const int* step_ptr;
    const float* colsum;
    const float* params;
    float4* out;
    int h, w, mh, mw, coef_stride, num_steps;
};

// reflect without repeating the border (torch 'reflect'), then clamp: only a tile's overhang beyond the image is ever clamped,
// and no pixel that is stored reads such a position
__device__ __forceinline__ int sd_reflect(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ float4 sd_mul(float t, float4 a) {
    return make_float4(__fmul_rn(t, a.x), __fmul_rn(t, a.y), __fmul_rn(t, a.z), __fmul_rn(t, a.w));
}
__device__ __forceinline__ float4 sd_fma(float t, float4 a, float4 v) {
    return make_float4(__fmaf_rn(t, a.x, v.x), __fmaf_rn(t, a.y, v.y), __fmaf_rn(t, a.z, v.z), __fmaf_rn(t, a.w, v.w));
}

// grid: x = tile column, y = tile row, z = sample
__global__ __launch_bounds__(SD_T * SD_T) void sag_degrade_kernel(const SDArgs p) {
    __shared__ float4 sx[SD_E][SD_E];   // x0 with halo
    __shared__ float4 sh[SD_E][SD_T];   // after the horizontal pass
    const int tid = threadIdx.x, lx = tid % SD_T, ly = tid / SD_T;
    const int x0t = blockIdx.x * SD_T, y0t = blockIdx.y * SD_T, b = blockIdx.z;
    const int h = p.h, w = p.w;
    int step = p.step_ptr ? *p.step_ptr : 0;
    step = min(max(step, 0), p.num_steps - 1);
    const float alpha = p.coef[(size_t)step * p.coef_stride], sigma = p.coef[(size_t)step * p.coef_stride + 1];
    float tap[2 * SD_R + 1];
#pragma unroll
    for (int i = 0; i < 2 * SD_R + 1; ++i) tap[i] = p.params[i];
    const float threshold = p.params[2 * SD_R + 1];
    const size_t base = (size_t)b * h * w;

    for (int i = tid; i < SD_E * SD_E; i += SD_T * SD_T) {
        const int ey = i / SD_E, ex = i % SD_E;
        const int gy = sd_reflect(y0t + ey - SD_R, h), gx = sd_reflect(x0t + ex - SD_R, w);
        const float4 x = p.latent[base + (size_t)gy * w + gx], e = p.eps[base + (size_t)gy * w + gx];
        // x0 = (x - sigma e) / alpha: one fused multiply-add, one IEEE division (no reciprocal multiply)
        sx[ey][ex] = make_float4(__fdiv_rn(__fmaf_rn(-sigma, e.x, x.x), alpha), __fdiv_rn(__fmaf_rn(-sigma, e.y, x.y), alpha),
                                 __fdiv_rn(__fmaf_rn(-sigma, e.z, x.z), alpha), __fdiv_rn(__fmaf_rn(-sigma, e.w, x.w), alpha));
    }
    __syncthreads();
    for (int i = tid; i < SD_E * SD_T; i += SD_T * SD_T) {
        const int ey = i / SD_T, ox = i % SD_T;
        float4 v = sd_mul(tap[0], sx[ey][ox]);
#pragma unroll
        for (int t = 1; t < 2 * SD_R + 1; ++t) v = sd_fma(tap[t], sx[ey][ox + t], v);
        sh[ey][ox] = v;
    }
    __syncthreads();
    float4 blur = sd_mul(tap[0], sh[ly][lx]);
#pragma unroll
    for (int t = 1; t < 2 * SD_R + 1; ++t) blur = sd_fma(tap[t], sh[ly + t][lx], blur);

    const int y = y0t + ly, x = x0t + lx;
    if (y >= h || x >= w) return;
    const size_t at = base + (size_t)y * w + x;
    const float4 lat = p.latent[at];
    const int my = (int)(((int64_t)y * p.mh) / h), mx = (int)(((int64_t)x * p.mw) / w);
    const float a = p.colsum[(size_t)b * p.mh * p.mw + (size_t)my * p.mw + mx];
    float4 o = lat;
    if (a > threshold) {
        const float4 e = p.eps[at];
        o = sd_fma(alpha, blur, sd_mul(sigma, e));
    }
    p.out[at] = o;
}

static bool sd_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

extern "C" int msdx_sag_degrade(const MsdxSagDegrade* p, msdx_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "sag_degrade: null argument");
    if (!p->latent || !p->eps || !p->coef || !p->colsum || !p->params || !p->out)
        MSD_FAIL(MSD_E_ARG, "sag_degrade: null latent / eps / coef / colsum / params / out");
    if (!msd_aligned16(p->latent) || !msd_aligned16(p->eps) || !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "sag_degrade: latent / eps / out must be 16-byte aligned");
    if ((((uintptr_t)p->coef) | ((uintptr_t)p->colsum) | ((uintptr_t)p->params) | ((uintptr_t)p->step_ptr)) & 3u)
        MSD_FAIL(MSD_E_ARG, "sag_degrade: coef / colsum / params / step_ptr must be 4-byte aligned");
    if (p->h < 5 || p->w < 5 || p->h > 4096 || p->w > 4096)
        MSD_FAIL(MSD_E_ARG, "sag_degrade: latent of %d x %d (5 .. 4096 per side: reflect padding of 4)", p->h, p->w);
    if (p->mh < 1 || p->mw < 1 || p->mh > p->h || p->mw > p->w)
        MSD_FAIL(MSD_E_ARG, "sag_degrade: map of %d x %d for a latent of %d x %d", p->mh, p->mw, p->h, p->w);
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "sag_degrade: batch %d (1 .. 65535)", p->batch);
    if (p->num_steps < 1 || p->coef_stride < 2) MSD_FAIL(MSD_E_ARG, "sag_degrade: num_steps %d, coef_stride %d (>= 1, >= 2)", p->num_steps, p->coef_stride);
    {   // out lies apart from every input
        const uintptr_t n = (uintptr_t)p->batch * p->h * p->w * 16;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + n;
        const uintptr_t l0 = (uintptr_t)p->latent, e0 = (uintptr_t)p->eps, c0 = (uintptr_t)p->coef, a0 = (uintptr_t)p->colsum, t0 = (uintptr_t)p->params;
        const uintptr_t cn = ((uintptr_t)(p->num_steps - 1) * p->coef_stride + 2) * 4, an = (uintptr_t)p->batch * p->mh * p->mw * 4;
        if (sd_overlap(o0, o1, l0, l0 + n) || sd_overlap(o0, o1, e0, e0 + n) || sd_overlap(o0, o1, c0, c0 + cn) || sd_overlap(o0, o1, a0, a0 + an) ||
            sd_overlap(o0, o1, t0, t0 + 40) || (p->step_ptr && sd_overlap(o0, o1, (uintptr_t)p->step_ptr, (uintptr_t)p->step_ptr + 4)))
            MSD_FAIL(MSD_E_ARG, "sag_degrade: out overlaps an input");
    }
    SDArgs a;
    a.latent = reinterpret_cast<const float4*>(p->latent);
    a.eps = reinterpret_cast<const float4*>(p->eps);
    a.coef = p->coef;
    a.step_ptr = p->step_ptr;
    a.colsum = p->colsum;
    a.params = p->params;
    a.out = reinterpret_cast<float4*>(p->out);
    a.h = p->h;
    a.w = p->w;
    a.mh = p->mh;
    a.mw = p->mw;
    a.coef_stride = p->coef_stride;
    a.num_steps = p->num_steps;
    const dim3 grid((unsigned)((p->w + SD_T - 1) / SD_T), (unsigned)((p->h + SD_T - 1) / SD_T), (unsigned)p->batch);
    hipLaunchKernelGGL(sag_degrade_kernel, grid, dim3(SD_T * SD_T), 0, stream, a);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
