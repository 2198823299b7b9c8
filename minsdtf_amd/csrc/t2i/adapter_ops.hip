// msda_unshuffle, msda_relu, msda_avgpool2: the three layer types of a T2I-Adapter the core library has no kernel of
// (include/minsdtf_hip_t2i.h; minsdtf_amd/t2iadapter.py forward_host is the float64 statement of the network).  They run once per
// job, between the core's convolutions.  One thread per 16-byte vector of the output: 8 bf16.  No LDS, no atomics, no scratch.
#include "../common.h"
#include "../../../include/minsdtf_hip_t2i.h"
#include "t2i_common.h"

#define AO_LANES 256

// ---- PixelUnshuffle(8): a thread writes the 8 channels c * 64 + dy * 8 + (0 .. 7) of one output pixel: 8 picture pixels of one row
__global__ __launch_bounds__(AO_LANES) void unshuffle_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t total,
                                                             int ho, int wo, int cin) {
    const int64_t idx = (int64_t)blockIdx.x * AO_LANES + threadIdx.x;   // ((b * ho + y) * wo + x) * cin * 8 + c * 8 + dy
    if (idx >= total) return;
    const int cd = (int)(idx % (cin * 8));
    const int64_t pix = idx / (cin * 8);
    const int c = cd >> 3, dy = cd & 7;
    const int x = (int)(pix % wo);
    const int64_t by = pix / wo;                     // b * ho + y: the picture row is 8 * (b * ho + y) + dy of b's h = 8 ho rows
    const float* src = in + ((by * 8 + dy) * ((int64_t)wo * 8) + (int64_t)x * 8) * cin + c;
    float f[8];
    if (cin == 1) {                                   // (wave-uniform) 8 adjacent floats, 32-byte aligned
        const float4 a = reinterpret_cast<const float4*>(src)[0], b = reinterpret_cast<const float4*>(src)[1];
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
#pragma unroll
        for (int dx = 0; dx < 8; ++dx) f[dx] = src[dx * cin];
    }
    *reinterpret_cast<uint4*>(out + idx * 8) = pack8(f);   // idx * 8 = pix * 64 cin + c * 64 + dy * 8
}

extern "C" int msda_unshuffle(const float* in, void* out, int32_t batch, int32_t h, int32_t w, int32_t cin, msda_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!in || !out || !msd_aligned16(in) || !msd_aligned16(out)) MSD_FAIL(MSD_E_ARG, "unshuffle: in / out must be non-null and 16-byte aligned");
    if (batch < 1 || h < 8 || w < 8 || (h & 7) || (w & 7)) MSD_FAIL(MSD_E_ARG, "unshuffle: batch %d, picture %d x %d (multiples of 8)", batch, h, w);
    if (cin < 1 || cin > 4) MSD_FAIL(MSD_E_ARG, "unshuffle: cin %d (1 .. 4)", cin);
    const int64_t elems = (int64_t)batch * h * w * cin;
    if (elems >= (int64_t)1 << 31) MSD_FAIL(MSD_E_ARG, "unshuffle: %lld elements (fewer than 2^31)", (long long)elems);
    if (msda_overlap((uintptr_t)in, (uintptr_t)in + (uintptr_t)elems * 4, (uintptr_t)out, (uintptr_t)out + (uintptr_t)elems * 2))
        MSD_FAIL(MSD_E_ARG, "unshuffle: out overlaps in");
    const int64_t total = elems / 8;
    hipLaunchKernelGGL(unshuffle_kernel, dim3((unsigned)((total + AO_LANES - 1) / AO_LANES)), dim3(AO_LANES), 0, stream, in,
                       reinterpret_cast<bf16_t*>(out), total, h / 8, w / 8, cin);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}

// ---- ReLU in place, on the bits: a set sign bit that is no NaN's becomes +0; everything else (a NaN included) is kept as it is
__device__ __forceinline__ uint32_t relu2(uint32_t v) {
    const uint32_t lo = v & 0xFFFFu, hi = v >> 16;
    const uint32_t l = ((lo & 0x8000u) && (lo & 0x7FFFu) <= 0x7F80u) ? 0u : lo;
    const uint32_t h = ((hi & 0x8000u) && (hi & 0x7FFFu) <= 0x7F80u) ? 0u : hi;
    return l | (h << 16);
}

__global__ __launch_bounds__(AO_LANES) void relu_kernel(uint4* __restrict__ x, int64_t vecs) {
    const int64_t idx = (int64_t)blockIdx.x * AO_LANES + threadIdx.x;
    if (idx >= vecs) return;
    uint4 v = x[idx];
    v.x = relu2(v.x); v.y = relu2(v.y); v.z = relu2(v.z); v.w = relu2(v.w);
    x[idx] = v;
}

extern "C" int msda_relu(void* x, int64_t n, msda_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!x || !msd_aligned16(x)) MSD_FAIL(MSD_E_ARG, "relu: x must be non-null and 16-byte aligned");
    if (n < 8 || (n & 7) || n >= (int64_t)1 << 38) MSD_FAIL(MSD_E_ARG, "relu: n %lld (a positive multiple of 8, below 2^38)", (long long)n);
    const int64_t vecs = n / 8;
    hipLaunchKernelGGL(relu_kernel, dim3((unsigned)((vecs + AO_LANES - 1) / AO_LANES)), dim3(AO_LANES), 0, stream,
                       reinterpret_cast<uint4*>(x), vecs);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}

// ---- AvgPool2d(2, 2): a thread writes 8 channels of one output pixel from four 16-byte loads
__global__ __launch_bounds__(AO_LANES) void avgpool2_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int64_t total, int ho,
                                                            int wo, int cv) {
    const int64_t idx = (int64_t)blockIdx.x * AO_LANES + threadIdx.x;   // ((b * ho + y) * wo + x) * cv + k
    if (idx >= total) return;
    const int k = (int)(idx % cv);
    const int64_t pix = idx / cv;
    const int x = (int)(pix % wo);
    const int64_t by = pix / wo;                     // b * ho + y: the input row is 2 * (b * ho + y) of b's h = 2 ho rows
    const int64_t C = (int64_t)cv * 8, row = (int64_t)wo * 2 * C;
    const bf16_t* src = in + by * 2 * row + (int64_t)x * 2 * C + (int64_t)k * 8;
    float a00[8], a01[8], a10[8], a11[8], f[8];
    unpack8(*reinterpret_cast<const uint4*>(src), a00);
    unpack8(*reinterpret_cast<const uint4*>(src + C), a01);
    unpack8(*reinterpret_cast<const uint4*>(src + row), a10);
    unpack8(*reinterpret_cast<const uint4*>(src + row + C), a11);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = ((a00[i] + a01[i]) + (a10[i] + a11[i])) * 0.25f;
    *reinterpret_cast<uint4*>(out + idx * 8) = pack8(f);
}

extern "C" int msda_avgpool2(const void* in, void* out, int32_t batch, int32_t h, int32_t w, int32_t c, msda_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!in || !out || !msd_aligned16(in) || !msd_aligned16(out)) MSD_FAIL(MSD_E_ARG, "avgpool2: in / out must be non-null and 16-byte aligned");
    if (batch < 1 || h < 2 || w < 2 || (h & 1) || (w & 1)) MSD_FAIL(MSD_E_ARG, "avgpool2: batch %d, map %d x %d (positive and even)", batch, h, w);
    if (c < 8 || (c & 7)) MSD_FAIL(MSD_E_ARG, "avgpool2: c %d (a positive multiple of 8)", c);
    const int64_t elems = (int64_t)batch * h * w * c;
    if (elems >= (int64_t)1 << 31) MSD_FAIL(MSD_E_ARG, "avgpool2: %lld input elements (fewer than 2^31)", (long long)elems);
    if (msda_overlap((uintptr_t)in, (uintptr_t)in + (uintptr_t)elems * 2, (uintptr_t)out, (uintptr_t)out + (uintptr_t)(elems / 4) * 2))
        MSD_FAIL(MSD_E_ARG, "avgpool2: out overlaps in");
    const int64_t total = elems / 32;                 // output vectors: batch * (h / 2) * (w / 2) * (c / 8)
    hipLaunchKernelGGL(avgpool2_kernel, dim3((unsigned)((total + AO_LANES - 1) / AO_LANES)), dim3(AO_LANES), 0, stream,
                       reinterpret_cast<const bf16_t*>(in), reinterpret_cast<bf16_t*>(out), total, h / 2, w / 2, c / 8);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
