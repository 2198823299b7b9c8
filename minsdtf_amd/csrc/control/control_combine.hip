// msdc_control_combine: the scaled residuals of up to three ControlNet units added to the 13 skip tensors of one UNet pass
// (include/minsdtf_hip_control.h has the formula; minsdtf_amd/control.py combine_host is the float64 statement).
//
// One 256-lane workgroup = one chunk of MSDC_CHUNK = 2048 elements of one (tap, row): blockIdx.y is the row, blockIdx.x counts the
// chunks of a row over all 13 taps, and the tap is found by twelve wave-uniform compares against the host-computed prefix.  A lane
// owns 8 adjacent channels: one 16-byte bf16 load and store, two 16-byte fp32 loads per unit.  The tail of a row (1 x 1 x 1280 is
// not a whole chunk) is a lane predicate.  The scales of the (tap, row) are wave-uniform: when all are 0 the workgroup returns
// before any load, and a unit whose scale is 0 is skipped, loads included.  No LDS, no atomics, no scratch; pure streaming, so the
// launch costs its bytes: 2 + 2 + 4 N per element.
#include "../common.h"
#include "../../../include/minsdtf_hip_control.h"

#define CC_LANES 256

struct CCArgs {
    MsdcControlCombine p;   // the ABI block as it is: kernel arguments live in constant memory, indexed by the wave-uniform tap
};

__device__ __forceinline__ void cc_add(float* f, float s, const float* r, size_t off) {
    const float4 a = *reinterpret_cast<const float4*>(r + off), b = *reinterpret_cast<const float4*>(r + off + 4);
    f[0] = __fmaf_rn(s, a.x, f[0]); f[1] = __fmaf_rn(s, a.y, f[1]); f[2] = __fmaf_rn(s, a.z, f[2]); f[3] = __fmaf_rn(s, a.w, f[3]);
    f[4] = __fmaf_rn(s, b.x, f[4]); f[5] = __fmaf_rn(s, b.y, f[5]); f[6] = __fmaf_rn(s, b.z, f[6]); f[7] = __fmaf_rn(s, b.w, f[7]);
}

__global__ __launch_bounds__(CC_LANES) void control_combine_kernel(const CCArgs a) {
    const MsdcControlCombine& p = a.p;
    const int chunk = (int)blockIdx.x, row = (int)blockIdx.y;
    int t = 0;
#pragma unroll
    for (int k = 1; k < MSDC_TAPS; ++k) t += chunk >= p.chunk_prefix[k] ? 1 : 0;
    const int count = p.count[t];
    int step = p.step_ptr ? *p.step_ptr : 0;
    step = min(max(step, 0), p.num_steps - 1);
    const float* s = p.scales + ((size_t)step * p.units * MSDC_TAPS + t) * 2 + (row < p.rows_u ? 0 : 1);
    const float s0 = s[0];
    const float s1 = p.units > 1 ? s[2 * MSDC_TAPS] : 0.0f;
    const float s2 = p.units > 2 ? s[4 * MSDC_TAPS] : 0.0f;
    if (s0 == 0.0f && s1 == 0.0f && s2 == 0.0f) return;   // (wave-uniform: the whole workgroup leaves, nothing was loaded)
    const int e = (chunk - p.chunk_prefix[t]) * MSDC_CHUNK + (int)threadIdx.x * 8;
    if (e >= count) return;                                // the tail of the row (count is a multiple of 8: whole vectors)
    const size_t off = (size_t)row * (size_t)count + (size_t)e;
    uint4* dst = reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(p.skip[t]) + off);
    float f[8];
    unpack8(*dst, f);
    if (s0 != 0.0f) cc_add(f, s0, p.resid[0][t], off);
    if (s1 != 0.0f) cc_add(f, s1, p.resid[1][t], off);
    if (s2 != 0.0f) cc_add(f, s2, p.resid[2][t], off);
    *dst = pack8(f);
}

static bool cc_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

extern "C" int msdc_control_combine(const MsdcControlCombine* p, msdc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "control_combine: null argument");
    if (p->units < 1 || p->units > MSDC_MAX_UNITS) MSD_FAIL(MSD_E_ARG, "control_combine: units %d (1 .. %d)", p->units, MSDC_MAX_UNITS);
    if (p->rows < 1 || p->rows > 65535) MSD_FAIL(MSD_E_ARG, "control_combine: rows %d (1 .. 65535)", p->rows);
    if (p->rows_u < 0 || p->rows_u > p->rows) MSD_FAIL(MSD_E_ARG, "control_combine: rows_u %d of %d rows", p->rows_u, p->rows);
    if (p->num_steps < 1) MSD_FAIL(MSD_E_ARG, "control_combine: num_steps %d (>= 1)", p->num_steps);
    if (!p->scales || !msd_aligned16(p->scales)) MSD_FAIL(MSD_E_ARG, "control_combine: scales must be non-null and 16-byte aligned");
    if (((uintptr_t)p->step_ptr) & 3u) MSD_FAIL(MSD_E_ARG, "control_combine: step_ptr must be 4-byte aligned");
    if (p->chunk_prefix[0] != 0) MSD_FAIL(MSD_E_ARG, "control_combine: chunk_prefix[0] = %d (0)", p->chunk_prefix[0]);
    const uintptr_t s0 = (uintptr_t)p->scales, s1 = s0 + (uintptr_t)p->num_steps * p->units * MSDC_TAPS * 8;
    const uintptr_t c0 = (uintptr_t)p->step_ptr;
    for (int k = 0; k < MSDC_TAPS; ++k) {
        const int n = p->count[k];
        if (n < 8 || (n & 7)) MSD_FAIL(MSD_E_ARG, "control_combine: count[%d] = %d (a positive multiple of 8)", k, n);
        const int64_t chunks = ((int64_t)n + MSDC_CHUNK - 1) / MSDC_CHUNK;
        if ((int64_t)p->chunk_prefix[k + 1] != (int64_t)p->chunk_prefix[k] + chunks)
            MSD_FAIL(MSD_E_ARG, "control_combine: chunk_prefix[%d] = %d, expected %lld", k + 1, p->chunk_prefix[k + 1],
                     (long long)((int64_t)p->chunk_prefix[k] + chunks));
        if (!p->skip[k] || !msd_aligned16(p->skip[k])) MSD_FAIL(MSD_E_ARG, "control_combine: skip[%d] must be non-null and 16-byte aligned", k);
        const uintptr_t o0 = (uintptr_t)p->skip[k], o1 = o0 + (uintptr_t)p->rows * (uintptr_t)n * 2;
        if (cc_overlap(o0, o1, s0, s1) || (p->step_ptr && cc_overlap(o0, o1, c0, c0 + 4)))
            MSD_FAIL(MSD_E_ARG, "control_combine: skip[%d] overlaps scales / step_ptr", k);
        for (int u = 0; u < p->units; ++u) {
            const float* r = p->resid[u][k];
            if (!r || !msd_aligned16(r)) MSD_FAIL(MSD_E_ARG, "control_combine: resid[%d][%d] must be non-null and 16-byte aligned", u, k);
            const uintptr_t r0 = (uintptr_t)r;
            if (cc_overlap(o0, o1, r0, r0 + (uintptr_t)p->rows * (uintptr_t)n * 4))
                MSD_FAIL(MSD_E_ARG, "control_combine: skip[%d] overlaps resid[%d][%d]", k, u, k);
        }
    }
    CCArgs a;
    a.p = *p;
    hipLaunchKernelGGL(control_combine_kernel, dim3((unsigned)p->chunk_prefix[MSDC_TAPS], (unsigned)p->rows), dim3(CC_LANES), 0, stream, a);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
