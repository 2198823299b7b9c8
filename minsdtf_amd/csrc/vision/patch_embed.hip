// msdv_patch_embed: pixels -> the input of encoder layer 0 of the CLIP ViT-H/14 vision tower (include/minsdtf_hip_vision.h has the
// formulas).
//
// One kernel, grid (17, batch), four waves.  Workgroups 0 .. 15 of a sample own one picture row of 16 patches each:
//  * its pixels are 14 CONTIGUOUS image rows (14 x 672 floats): read once with 16-byte loads, normalised (one fma), rounded to
//    bf16 and laid into LDS as the [16 patches][588 -> 608] operand, k = (ky * 14 + kx) * 3 + c, the tail zeroed;
//  * C^T = W X^T on v_mfma_f32_16x16x32_bf16: the weight rows are the A operand (read straight from global memory as fragments,
//    16 bytes per lane: the 1.5 MB matrix is L2-resident across the 16 workgroups of a sample), the patches the B operand, so a
//    lane's accumulator registers are 4 CONSECUTIVE CHANNELS of ONE patch (row 4 g + i, column r).  Wave w owns the channels
//    [320 w, 320 w + 320): 20 accumulator fragments, the whole 1280-wide row of the 16 patches stays in registers;
//  * the last k-step (576 .. 607) reads only what a w row holds: lanes g = 0 their 8 values, g = 1 the four of 584 .. 587 (588 ..
//    591 are inside w_ld >= 592 but padding: masked to zero), g >= 2 nothing;
//  * LayerNorm in fp32 over the accumulators: a lane sums its 80 values ascending, the 16 partial sums of a patch (4 waves x 4
//    lane groups) meet in LDS and every lane adds them in the same ascending order; mean first, then the squared deviations.
// Workgroup 16 is the class token: cls + pos[0], the same LayerNorm over 5 channels per thread.
// Nothing depends on the batch; no atomics, no scratch.
#include <math.h>
#include "../common.h"
#include "../../../include/minsdtf_hip_vision.h"

#define PE_ROWF (MSDV_IMAGE * 3)            // 672 floats of one image row
#define PE_K MSDV_PATCH_K                   // 588
#define PE_KSTEPS 19                        // ceil(588 / 32)
#define PE_KP (PE_KSTEPS * 32)              // 608
#define PE_ROW (PE_KP + 8)                  // LDS row stride in bf16 (1232 bytes: 16-byte aligned, off the 128-byte period)
#define PE_NB 20                            // 16-channel blocks of a wave: 320 channels
#define PE_C MSDV_WIDTH

struct PEArgs {
    const float* pixels;
    const bf16_t* w;
    const float* cls;
    const float* pos;
    const float* gamma;
    const float* beta;
    bf16_t* out;
    float sc0, sc1, sc2, sh0, sh1, sh2, eps;
    int w_ld, o_ld;
};

__device__ __forceinline__ float pe_total(float (*red)[4][16], int r) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int g = 0; g < 4; ++g) t += red[w][g][r];
    return t;
}

__global__ __launch_bounds__(256) void patch_embed_kernel(const PEArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t sA[16 * PE_ROW];
    __shared__ float red[4][4][16];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
    const int py = blockIdx.x, b = blockIdx.y;

    if (py == MSDV_GRID) {   // (workgroup-uniform) the class token: channels tid + 256 j
        float e[5], s = 0.0f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            e[j] = p.cls[tid + 256 * j] + p.pos[tid + 256 * j];
            s += e[j];
        }
        s = wave_sum(s);
        if (lane == 0) red[0][0][wave] = s;
        __syncthreads();
        const float mean = (((red[0][0][0] + red[0][0][1]) + red[0][0][2]) + red[0][0][3]) * (1.0f / PE_C);
        __syncthreads();
        float q = 0.0f;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            e[j] -= mean;
            q += e[j] * e[j];
        }
        q = wave_sum(q);
        if (lane == 0) red[0][0][wave] = q;
        __syncthreads();
        const float var = (((red[0][0][0] + red[0][0][1]) + red[0][0][2]) + red[0][0][3]) * (1.0f / PE_C);
        const float rstd = 1.0f / sqrtf(var + p.eps);
        bf16_t* o = p.out + (size_t)b * MSDV_TOKENS * p.o_ld;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int n = tid + 256 * j;
            o[n] = f2bf(e[j] * rstd * p.gamma[n] + p.beta[n]);
        }
        return;
    }

    // ---- stage the 16 patches: 14 image rows x 672 floats, contiguous
    {
        const float4* src = reinterpret_cast<const float4*>(p.pixels + ((size_t)b * MSDV_IMAGE + py * MSDV_PATCH) * PE_ROWF);
        for (int v = tid; v < MSDV_PATCH * PE_ROWF / 4; v += 256) {
            const float4 f = src[v];
            const float fv[4] = {f.x, f.y, f.z, f.w};
            const int idx = v * 4, ky = idx / PE_ROWF, rem = idx - ky * PE_ROWF;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int x = rem + e, pt = x / (MSDV_PATCH * 3), kk = x - pt * (MSDV_PATCH * 3), c = x % 3;
                const float sc = c == 0 ? p.sc0 : (c == 1 ? p.sc1 : p.sc2), sh = c == 0 ? p.sh0 : (c == 1 ? p.sh1 : p.sh2);
                sA[pt * PE_ROW + ky * (MSDV_PATCH * 3) + kk] = f2bf(__builtin_fmaf(fv[e], sc, sh));
            }
        }
        for (int i = tid; i < 16 * (PE_KP - PE_K); i += 256) sA[(i / (PE_KP - PE_K)) * PE_ROW + PE_K + i % (PE_KP - PE_K)] = 0;
    }
    __syncthreads();

    // ---- C^T = W X^T: accumulator register i of fragment nb is channel 320 wave + 16 nb + 4 g + i of patch r
    f32x4 acc[PE_NB];
#pragma unroll
    for (int nb = 0; nb < PE_NB; ++nb) acc[nb] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    const bf16_t* wrow = p.w + (size_t)(wave * (PE_NB * 16) + r) * p.w_ld + 8 * g;
    const bf16_t* xrow = sA + r * PE_ROW + 8 * g;
    const size_t wstep = (size_t)16 * p.w_ld;
    for (int ks = 0; ks < PE_KSTEPS - 1; ++ks) {
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xrow + ks * 32);
        bf16x8 wf[PE_NB];
#pragma unroll
        for (int nb = 0; nb < PE_NB; ++nb) wf[nb] = *reinterpret_cast<const bf16x8*>(wrow + nb * wstep + ks * 32);
#pragma unroll
        for (int nb = 0; nb < PE_NB; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[nb], xf, acc[nb], 0, 0, 0);
    }
    {   // the ragged last step: k = 576 + 8 g + 0 .. 7, of which 576 .. 587 exist
        const int ks = PE_KSTEPS - 1;
        const bf16x8 xf = *reinterpret_cast<const bf16x8*>(xrow + ks * 32);
#pragma unroll
        for (int nb = 0; nb < PE_NB; ++nb) {
            bf16x8 wf = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
            if (g < 2) wf = *reinterpret_cast<const bf16x8*>(wrow + nb * wstep + ks * 32);   // g = 1: 584 .. 591 < w_ld
            if (g == 1) wf[4] = wf[5] = wf[6] = wf[7] = 0;                                    // 588 .. 591 are padding
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf, acc[nb], 0, 0, 0);
        }
    }

    // ---- + position embedding, LayerNorm
    const int tok = 1 + py * MSDV_GRID + r, n0 = wave * (PE_NB * 16) + 4 * g;
    const float* posr = p.pos + (size_t)tok * PE_C + n0;
    float s = 0.0f;
#pragma unroll
    for (int nb = 0; nb < PE_NB; ++nb) {
        const float4 pv = *reinterpret_cast<const float4*>(posr + nb * 16);
        acc[nb][0] += pv.x; acc[nb][1] += pv.y; acc[nb][2] += pv.z; acc[nb][3] += pv.w;
        s += acc[nb][0]; s += acc[nb][1]; s += acc[nb][2]; s += acc[nb][3];
    }
    red[wave][g][r] = s;
    __syncthreads();
    const float mean = pe_total(red, r) * (1.0f / PE_C);
    __syncthreads();
    float q = 0.0f;
#pragma unroll
    for (int nb = 0; nb < PE_NB; ++nb)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[nb][i] -= mean;
            q += acc[nb][i] * acc[nb][i];
        }
    red[wave][g][r] = q;
    __syncthreads();
    const float rstd = 1.0f / sqrtf(pe_total(red, r) * (1.0f / PE_C) + p.eps);
    bf16_t* o = p.out + ((size_t)b * MSDV_TOKENS + tok) * p.o_ld + n0;
#pragma unroll
    for (int nb = 0; nb < PE_NB; ++nb) {
        const float4 ga = *reinterpret_cast<const float4*>(p.gamma + n0 + nb * 16);
        const float4 be = *reinterpret_cast<const float4*>(p.beta + n0 + nb * 16);
        uint2 v;
        v.x = pack_bf2(acc[nb][0] * rstd * ga.x + be.x, acc[nb][1] * rstd * ga.y + be.y);
        v.y = pack_bf2(acc[nb][2] * rstd * ga.z + be.z, acc[nb][3] * rstd * ga.w + be.w);
        *reinterpret_cast<uint2*>(o + nb * 16) = v;
    }
}

static bool pe_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bn && b0 < a0 + an;
}

extern "C" int msdv_patch_embed(const MsdvPatchEmbed* p, msdv_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "patch_embed: null argument");
    if (!p->pixels || !p->w || !p->cls || !p->pos || !p->gamma || !p->beta || !p->out)
        MSD_FAIL(MSD_E_ARG, "patch_embed: null pixels / w / cls / pos / gamma / beta / out");
    if (!msd_aligned16(p->pixels) || !msd_aligned16(p->w) || !msd_aligned16(p->cls) || !msd_aligned16(p->pos) || !msd_aligned16(p->gamma) ||
        !msd_aligned16(p->beta) || !msd_aligned16(p->out))
        MSD_FAIL(MSD_E_ARG, "patch_embed: every pointer must be 16-byte aligned");
    if (p->image != MSDV_IMAGE || p->patch != MSDV_PATCH || p->width != MSDV_WIDTH)
        MSD_FAIL(MSD_E_UNSUPPORTED, "patch_embed: image %d / patch %d / width %d (ViT-H/14 only: %d / %d / %d)", p->image, p->patch, p->width,
                 MSDV_IMAGE, MSDV_PATCH, MSDV_WIDTH);
    if (p->batch < 1 || p->batch > MSDV_MAX_BATCH) MSD_FAIL(MSD_E_ARG, "patch_embed: batch %d (1 .. %d)", p->batch, MSDV_MAX_BATCH);
    if ((p->w_ld % 8) || p->w_ld < MSDV_PATCH_K)
        MSD_FAIL(MSD_E_ARG, "patch_embed: w_ld %d (a multiple of 8, at least %d)", p->w_ld, MSDV_PATCH_K);
    if ((p->o_ld % 8) || p->o_ld < MSDV_WIDTH) MSD_FAIL(MSD_E_ARG, "patch_embed: o_ld %d (a multiple of 8, at least %d)", p->o_ld, MSDV_WIDTH);
    if (!(p->eps > 0.0f)) MSD_FAIL(MSD_E_ARG, "patch_embed: eps %g (> 0)", (double)p->eps);
    {
        const size_t on = ((size_t)p->batch * MSDV_TOKENS - 1) * p->o_ld * 2 + (size_t)MSDV_WIDTH * 2;
        const size_t vec = (size_t)MSDV_WIDTH * 4;
        if (pe_overlap(p->out, on, p->pixels, (size_t)p->batch * MSDV_IMAGE * PE_ROWF * 4) ||
            pe_overlap(p->out, on, p->w, ((size_t)(MSDV_WIDTH - 1) * p->w_ld + MSDV_PATCH_K) * 2) || pe_overlap(p->out, on, p->cls, vec) ||
            pe_overlap(p->out, on, p->pos, (size_t)MSDV_TOKENS * vec) || pe_overlap(p->out, on, p->gamma, vec) || pe_overlap(p->out, on, p->beta, vec))
            MSD_FAIL(MSD_E_ARG, "patch_embed: out overlaps an input");
    }
    PEArgs a;
    a.pixels = p->pixels;
    a.w = reinterpret_cast<const bf16_t*>(p->w);
    a.cls = p->cls;
    a.pos = p->pos;
    a.gamma = p->gamma;
    a.beta = p->beta;
    a.out = reinterpret_cast<bf16_t*>(p->out);
    a.sc0 = p->scale[0]; a.sc1 = p->scale[1]; a.sc2 = p->scale[2];
    a.sh0 = p->shift[0]; a.sh1 = p->shift[1]; a.sh2 = p->shift[2];
    a.eps = p->eps;
    a.w_ld = p->w_ld;
    a.o_ld = p->o_ld;
    hipLaunchKernelGGL(patch_embed_kernel, dim3(MSDV_GRID + 1, (unsigned)p->batch), dim3(256), 0, stream, a);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
