// msdv_pool_project: LayerNorm of the class token + the bias-free 1280 -> 1024 projection (include/minsdtf_hip_vision.h): the pooled
// head of the CLIP vision tower.
//
// Grid (64, batch), four waves; a workgroup owns 16 output columns of one sample, a wave 4 of them.  Every workgroup recomputes
// the row's statistics with the same code (1280 values: 5 per thread, the core's fixed-order wave reduction, the four wave sums
// added ascending), keeps the normalised row in LDS as fp32 - never rounded - and then runs one fmaf chain per lane and column
// over k = 8 (lane + 64 j) + 0 .. 7, j = 0, 1, 2 (16-byte weight loads, rows or chunk-major), closed by the same wave reduction.
// The orders depend on the shape alone: a sample's bits do not depend on its batch.  No atomics, no scratch.
#include <math.h>
#include "../common.h"
#include "../../../include/minsdtf_hip_vision.h"

#define PP_C MSDV_WIDTH
#define PP_N MSDV_PROJ
#define PP_COLS 16   // output columns of a workgroup

struct PPArgs {
    const bf16_t* x;
    const float* gamma;
    const float* beta;
    const bf16_t* w;
    float* out;
    int64_t x_stride;
    float eps;
    int w_layout;
};

__global__ __launch_bounds__(256) void pool_project_kernel(const PPArgs p) {
    __shared__ __attribute__((aligned(16))) float y[PP_C];
    __shared__ float red[4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.y;
    const bf16_t* xr = p.x + (size_t)b * p.x_stride;
    float v[5], s = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        v[j] = bf2f(xr[tid + 256 * j]);
        s += v[j];
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float mean = (((red[0] + red[1]) + red[2]) + red[3]) * (1.0f / PP_C);
    __syncthreads();
    float q = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        v[j] -= mean;
        q += v[j] * v[j];
    }
    q = wave_sum(q);
    if (lane == 0) red[wave] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf((((red[0] + red[1]) + red[2]) + red[3]) * (1.0f / PP_C) + p.eps);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int n = tid + 256 * j;
        y[n] = v[j] * rstd * p.gamma[n] + p.beta[n];
    }
    __syncthreads();

#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int n = blockIdx.x * PP_COLS + wave * 4 + c;
        float a = 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int k = 8 * (lane + 64 * j);
            if (k < PP_C) {
                const bf16_t* wp = p.w_layout ? p.w + ((size_t)(k >> 6) * PP_N + n) * 64 + (k & 63) : p.w + (size_t)n * PP_C + k;
                float wf[8];
                unpack8(*reinterpret_cast<const uint4*>(wp), wf);
#pragma unroll
                for (int e = 0; e < 8; ++e) a = __builtin_fmaf(y[k + e], wf[e], a);
            }
        }
        a = wave_sum(a);
        if (lane == 0) p.out[(size_t)b * PP_N + n] = a;
    }
}

static bool pp_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bn && b0 < a0 + an;
}

extern "C" int msdv_pool_project(const MsdvPoolProject* p, msdv_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "pool_project: null argument");
    if (!p->x || !p->gamma || !p->beta || !p->w || !p->out) MSD_FAIL(MSD_E_ARG, "pool_project: null x / gamma / beta / w / out");
    if (!msd_aligned16(p->x) || !msd_aligned16(p->gamma) || !msd_aligned16(p->beta) || !msd_aligned16(p->w) || !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "pool_project: every pointer must be 16-byte aligned");
    if (p->width != MSDV_WIDTH || p->proj != MSDV_PROJ)
        MSD_FAIL(MSD_E_UNSUPPORTED, "pool_project: width %d / proj %d (ViT-H/14 only: %d / %d)", p->width, p->proj, MSDV_WIDTH, MSDV_PROJ);
    if (p->batch < 1 || p->batch > MSDV_MAX_BATCH) MSD_FAIL(MSD_E_ARG, "pool_project: batch %d (1 .. %d)", p->batch, MSDV_MAX_BATCH);
    if (p->x_stride < MSDV_WIDTH || (p->x_stride % 8) || p->x_stride > ((int64_t)1 << 40))
        MSD_FAIL(MSD_E_ARG, "pool_project: x_stride %lld (a multiple of 8, at least %d)", (long long)p->x_stride, MSDV_WIDTH);
    if (p->w_layout != 0 && p->w_layout != 1) MSD_FAIL(MSD_E_ARG, "pool_project: w_layout %d (0: rows, 1: chunk-major)", p->w_layout);
    if (!(p->eps > 0.0f)) MSD_FAIL(MSD_E_ARG, "pool_project: eps %g (> 0)", (double)p->eps);
    {
        const size_t on = (size_t)p->batch * PP_N * 4, vec = (size_t)PP_C * 4;
        if (pp_overlap(p->out, on, p->x, ((size_t)(p->batch - 1) * p->x_stride + PP_C) * 2) || pp_overlap(p->out, on, p->gamma, vec) ||
            pp_overlap(p->out, on, p->beta, vec) || pp_overlap(p->out, on, p->w, (size_t)PP_N * PP_C * 2))
            MSD_FAIL(MSD_E_ARG, "pool_project: out overlaps an input");
    }
    PPArgs a;
    a.x = reinterpret_cast<const bf16_t*>(p->x);
    a.gamma = p->gamma;
    a.beta = p->beta;
    a.w = reinterpret_cast<const bf16_t*>(p->w);
    a.out = p->out;
    a.x_stride = p->x_stride;
    a.eps = p->eps;
    a.w_layout = p->w_layout;
    hipLaunchKernelGGL(pool_project_kernel, dim3(PP_N / PP_COLS, (unsigned)p->batch), dim3(256), 0, stream, a);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
