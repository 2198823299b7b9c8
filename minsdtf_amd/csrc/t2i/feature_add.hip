// msda_feature_add: the T2I-Adapter features of one site added to a UNet activation in place, the same feature to every row
// (include/minsdtf_hip_t2i.h has the formula; minsdtf_amd/t2iadapter.py add_reference is the float64 statement).
//
// One 256-lane workgroup owns one chunk of MSDA_CHUNK = 2048 elements of `n` (a lane: 8 adjacent elements, one 16-byte vector) and
// walks the rows: the features of its chunk are loaded ONCE, into registers, and every row costs one 16-byte load and one 16-byte
// store.  The other layout - a workgroup per (chunk, row), msdc_control_combine's - loads the feature once per row: with the 2 to 8
// rows of a guidance batch that is up to half of the launch's bytes again.  The grid is ceil(n / 2048) workgroups: 640 at the
// 64 x 64 x 320 site of a 512 x 512 job, 40 at the 8 x 8 x 1280 one.  The scales of the step are wave-uniform: when all are 0 the
// workgroup returns before any load, and a unit whose scale is 0 is skipped, loads included.  The tail of `n` is a lane
// predicate (n is a multiple of 8: whole vectors).  No LDS, no atomics, no scratch; the trip count is `rows`.
#include "../common.h"
#include "../../../include/minsdtf_hip_t2i.h"
#include "t2i_common.h"

#define FA_LANES 256

struct FAArgs {
    MsdaFeatureAdd p;   // the ABI block as it is
};

__device__ __forceinline__ void fa_load(float* g, const void* feat, size_t e) {
    unpack8(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(feat) + e), g);
}

__device__ __forceinline__ void fa_fma(float* f, float s, const float* g) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = __fmaf_rn(s, g[i], f[i]);
}

__global__ __launch_bounds__(FA_LANES) void feature_add_kernel(const FAArgs a) {
    const MsdaFeatureAdd& p = a.p;
    int step = p.step_ptr ? *p.step_ptr : 0;
    step = min(max(step, 0), p.num_steps - 1);
    const float* s = p.scales + ((size_t)step * p.units) * MSDA_SITES + p.site;
    const float s0 = s[0];
    const float s1 = p.units > 1 ? s[MSDA_SITES] : 0.0f;
    const float s2 = p.units > 2 ? s[2 * MSDA_SITES] : 0.0f;
    if (s0 == 0.0f && s1 == 0.0f && s2 == 0.0f) return;   // (wave-uniform: the whole workgroup leaves, nothing was loaded)
    const size_t e = (size_t)blockIdx.x * MSDA_CHUNK + (size_t)threadIdx.x * 8;
    if (e >= (size_t)p.n) return;                          // the tail of the row
    float g0[8], g1[8], g2[8];
    if (s0 != 0.0f) fa_load(g0, p.feat[0], e);
    if (s1 != 0.0f) fa_load(g1, p.feat[1], e);
    if (s2 != 0.0f) fa_load(g2, p.feat[2], e);
    bf16_t* x = reinterpret_cast<bf16_t*>(p.x) + e;
#pragma unroll 2
    for (int r = 0; r < p.rows; ++r) {
        uint4* dst = reinterpret_cast<uint4*>(x + (size_t)r * (size_t)p.n);
        float f[8];
        unpack8(*dst, f);
        if (s0 != 0.0f) fa_fma(f, s0, g0);
        if (s1 != 0.0f) fa_fma(f, s1, g1);
        if (s2 != 0.0f) fa_fma(f, s2, g2);
        *dst = pack8(f);
    }
}

extern "C" int msda_feature_add(const MsdaFeatureAdd* p, msda_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "feature_add: null argument");
    if (p->units < 1 || p->units > MSDA_MAX_UNITS) MSD_FAIL(MSD_E_ARG, "feature_add: units %d (1 .. %d)", p->units, MSDA_MAX_UNITS);
    if (p->site < 0 || p->site >= MSDA_SITES) MSD_FAIL(MSD_E_ARG, "feature_add: site %d (0 .. %d)", p->site, MSDA_SITES - 1);
    if (p->rows < 1 || p->rows > 65535) MSD_FAIL(MSD_E_ARG, "feature_add: rows %d (1 .. 65535)", p->rows);
    if (p->n < 8 || (p->n & 7)) MSD_FAIL(MSD_E_ARG, "feature_add: n %d (a positive multiple of 8)", p->n);
    if (p->num_steps < 1) MSD_FAIL(MSD_E_ARG, "feature_add: num_steps %d (>= 1)", p->num_steps);
    if (!p->x || !msd_aligned16(p->x)) MSD_FAIL(MSD_E_ARG, "feature_add: x must be non-null and 16-byte aligned");
    if (!p->scales || !msd_aligned16(p->scales)) MSD_FAIL(MSD_E_ARG, "feature_add: scales must be non-null and 16-byte aligned");
    if (((uintptr_t)p->step_ptr) & 3u) MSD_FAIL(MSD_E_ARG, "feature_add: step_ptr must be 4-byte aligned");
    const uintptr_t x0 = (uintptr_t)p->x, x1 = x0 + (uintptr_t)p->rows * (uintptr_t)p->n * 2;
    const uintptr_t s0 = (uintptr_t)p->scales, s1 = s0 + (uintptr_t)p->num_steps * p->units * MSDA_SITES * 4;
    const uintptr_t c0 = (uintptr_t)p->step_ptr;
    if (msda_overlap(x0, x1, s0, s1) || (p->step_ptr && msda_overlap(x0, x1, c0, c0 + 4)))
        MSD_FAIL(MSD_E_ARG, "feature_add: x overlaps scales / step_ptr");
    for (int u = 0; u < p->units; ++u) {
        const void* f = p->feat[u];
        if (!f || !msd_aligned16(f)) MSD_FAIL(MSD_E_ARG, "feature_add: feat[%d] must be non-null and 16-byte aligned", u);
        const uintptr_t f0 = (uintptr_t)f;
        if (msda_overlap(x0, x1, f0, f0 + (uintptr_t)p->n * 2)) MSD_FAIL(MSD_E_ARG, "feature_add: x overlaps feat[%d]", u);
    }
    FAArgs a;
    a.p = *p;
    const unsigned chunks = (unsigned)(((int64_t)p->n + MSDA_CHUNK - 1) / MSDA_CHUNK);
    hipLaunchKernelGGL(feature_add_kernel, dim3(chunks), dim3(FA_LANES), 0, stream, a);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
