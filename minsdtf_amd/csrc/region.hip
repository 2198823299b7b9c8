// msd_region_combine: the per-step combine of a regional-prompting job (include/minsdtf_hip.h has the formula and the pinned order
// of the sum; minsdtf_amd/regions.py builds and normalises the weights).
//
// One lane = one latent pixel of one sample = one float4.  A pixel under R regions costs R 16-byte loads, R 4-byte weight loads
// (consecutive lanes read consecutive words: coalesced) and one 16-byte store.  A 64 x 64 latent is 16 workgroups per sample, so
// the kernel sits at the launch floor, which is the point - it is one more launch in the step plan, in front of the sampler
// step, inside the captured graph.  An output element reads only its own position of each region's row, so the in-place form
// (out == eps: region 0's rows) has no race and needs no atomics, and nothing couples two pixels or two samples.
#include "common.h"

#define RC_THREADS 256

// (eps and out may be the same buffer: no __restrict__ on either)
__global__ __launch_bounds__(RC_THREADS) void region_combine_kernel(const float4* eps, const float* __restrict__ w, float4* out,
                                                                    int regions, int batch, int pixels) {
    // grid: x = RC_THREADS consecutive pixels of a sample, y = sample
    const int pix = blockIdx.x * RC_THREADS + threadIdx.x;
    if (pix >= pixels) return;
    const int b = blockIdx.y;
    const float4 x0 = eps[(int64_t)b * pixels + pix];
    const float w0 = w[pix];
    float4 v = make_float4(__fmul_rn(w0, x0.x), __fmul_rn(w0, x0.y), __fmul_rn(w0, x0.z), __fmul_rn(w0, x0.w));
    for (int r = 1; r < regions; ++r) {
        const float4 x = eps[((int64_t)r * batch + b) * pixels + pix];
        const float wr = w[(int64_t)r * pixels + pix];
        v = make_float4(__fmaf_rn(wr, x.x, v.x), __fmaf_rn(wr, x.y, v.y), __fmaf_rn(wr, x.z, v.z), __fmaf_rn(wr, x.w, v.w));
    }
    out[(int64_t)b * pixels + pix] = v;
}

extern "C" int msd_region_combine(const MsdRegionCombine* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "region_combine: null argument");
    if (!p->eps || !p->w || !p->out) MSD_FAIL(MSD_E_ARG, "region_combine: null eps / w / out");
    if (!msd_aligned16(p->eps) || !msd_aligned16(p->w) || !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "region_combine: eps / w / out must be 16-byte aligned");
    if (p->n < 4 || (p->n % 4)) MSD_FAIL(MSD_E_ARG, "region_combine: n = %d (a positive multiple of 4: whole pixels)", p->n);
    if (p->regions < 1 || p->regions > MSD_REGION_MAX) MSD_FAIL(MSD_E_ARG, "region_combine: %d regions (1 .. %d)", p->regions, MSD_REGION_MAX);
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "region_combine: batch %d (1 .. 65535)", p->batch);
    const int64_t n_eps = (int64_t)p->regions * p->batch * p->n;
    if (n_eps >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "region_combine: 2^31 or more elements in eps");
    {   // out is eps itself (region 0's rows are rewritten in place) or lies apart from it; w lies apart from both
        const uintptr_t e0 = (uintptr_t)p->eps, e1 = e0 + (uintptr_t)n_eps * 4;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)p->batch * p->n * 4;
        const uintptr_t w0 = (uintptr_t)p->w, w1 = w0 + (uintptr_t)p->regions * (p->n / 4) * 4;
        if (o0 != e0 && o0 < e1 && e0 < o1) MSD_FAIL(MSD_E_ARG, "region_combine: out overlaps eps (only out == eps is allowed)");
        if ((w0 < e1 && e0 < w1) || (w0 < o1 && o0 < w1)) MSD_FAIL(MSD_E_ARG, "region_combine: w overlaps eps or out");
    }
    const int pixels = p->n / 4;
    const dim3 grid((unsigned)((pixels + RC_THREADS - 1) / RC_THREADS), (unsigned)p->batch);
    hipLaunchKernelGGL(region_combine_kernel, grid, dim3(RC_THREADS), 0, stream, reinterpret_cast<const float4*>(p->eps), p->w,
                       reinterpret_cast<float4*>(p->out), p->regions, p->batch, pixels);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
