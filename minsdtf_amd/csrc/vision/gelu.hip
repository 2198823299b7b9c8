// msdv_gelu: out = bf16(0.5 x (1 + erf(x / sqrt 2))) over an fp32 matrix (include/minsdtf_hip_vision.h): the exact GELU of the CLIP
// vision tower's MLP and the one rounding of fc1's output.  One thread per 8 columns: two 16-byte loads, one 16-byte store.
#include <math.h>
#include "../common.h"
#include "../../../include/minsdtf_hip_vision.h"

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678f)); }

__global__ __launch_bounds__(256) void gelu_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int rows, int cv, int ld_in, int ld_out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * cv) return;
    const int r = (int)(idx / cv), c = (int)(idx - (int64_t)r * cv) * 8;
    const float4* src = reinterpret_cast<const float4*>(in + (size_t)r * ld_in + c);
    const float4 a = src[0], b = src[1];
    const float f[8] = {gelu_erf(a.x), gelu_erf(a.y), gelu_erf(a.z), gelu_erf(a.w), gelu_erf(b.x), gelu_erf(b.y), gelu_erf(b.z), gelu_erf(b.w)};
    *reinterpret_cast<uint4*>(out + (size_t)r * ld_out + c) = pack8(f);
}

extern "C" int msdv_gelu(const float* in, void* out, int32_t rows, int32_t cols, int32_t ld_in, int32_t ld_out, msdv_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!in || !out) MSD_FAIL(MSD_E_ARG, "gelu: null in / out");
    if (!msd_aligned16(in) || !msd_aligned16(out)) MSD_FAIL(MSD_E_ARG, "gelu: in / out must be 16-byte aligned");
    if (rows < 1 || cols < 8 || (cols % 8)) MSD_FAIL(MSD_E_ARG, "gelu: rows %d, cols %d (rows >= 1, cols a positive multiple of 8)", rows, cols);
    if (ld_in < cols || (ld_in % 4) || ld_out < cols || (ld_out % 8))
        MSD_FAIL(MSD_E_ARG, "gelu: ld_in %d / ld_out %d (at least cols = %d; multiples of 4 / 8)", ld_in, ld_out, cols);
    if ((int64_t)rows * (ld_in > ld_out ? ld_in : ld_out) >= (int64_t)1 << 31)
        MSD_FAIL(MSD_E_ARG, "gelu: rows %d x ld %d / %d (fewer than 2^31 elements)", rows, ld_in, ld_out);
    {
        const uintptr_t i0 = (uintptr_t)in, i1 = i0 + ((size_t)(rows - 1) * ld_in + cols) * 4;
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + ((size_t)(rows - 1) * ld_out + cols) * 2;
        if (i0 < o1 && o0 < i1) MSD_FAIL(MSD_E_ARG, "gelu: out overlaps in");
    }
    const int cv = cols / 8;
    const int64_t n = (int64_t)rows * cv;
    hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, reinterpret_cast<bf16_t*>(out), rows, cv, ld_in, ld_out);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
