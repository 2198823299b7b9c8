// msdt_dynamic_threshold: the combined prediction of a guidance step with dynamic thresholding (include/minsdtf_hip_dynthresh.h has
// the formula; minsdtf_amd/dynthresh.py dynthresh_host is the float64 statement).
//
// One 1024-lane workgroup = one sample, as cfg_step_kernel: a lane's pixels are tid, tid + 1024, ..., each one float4 = all four
// channels, so the four planes of a sample share every load, every barrier and every pass.  The launch is a chain of dependent
// rounds on `batch` workgroups:
//   A  load u and c, cfg = fma(g, c - u, u), mim = fma(m, c - u, u), the plane sums              -> the two means
//   B  deviations from the means: max |mc| ("ad") or the two sums of squares ("std")
//   C  ("ad") the lo-th smallest |cc|: four 8-bit radix passes over the key bits, most significant first.  |cc| >= 0, so its bit
//      pattern orders as the value does.  A pass counts the keys that match the prefix found so far into LDS histograms (integer
//      counts), one of 4 x 256 lanes per (channel, bin) sums its copies, an in-wave scan and the four wave totals of the channel
//      give every bin its range of ranks, and the one bin that holds the rank extends the prefix.  After four passes the prefix
//      IS s[lo]: an exact order statistic, ties included (the rank inside the last bin counts the ties in front)
//   D  s[hi]: s[lo] again when more than lo + 1 values are <= s[lo], otherwise the smallest key above it (one min reduction)
//      (lo = P - 1, percentile 1, the default: s[lo] is the largest key - one max reduction stands for C and D)
//   E  the output
// Up to P = 8192 pixels cfg stays in registers between the rounds (NPT float4 per lane) and up to P = 4096 (a 512 x 512 picture)
// mim does too; where they are not held they are recomputed from u and c, which this workgroup has just read (L2), by the SAME
// two instructions, so every round sees the same bits.  Above P = 8192 the generic form (NPT = 0) holds nothing: a 1024-lane
// workgroup has 128 VGPRs per lane, 16 held pixels would be 64 of them and the compiler then spills (8 .. 24 bytes per lane
// measured), and the kernel is to run without scratch.
// Every sum: a per-lane chain over the lane's pixels in ascending order, a fixed cross-lane tree inside the wave (wave_sum), the 16
// waves in ascending order through LDS - an order that depends on (h, w) alone.  Trip counts depend on P alone.
#include "../common.h"
#include "../../../include/minsdtf_hip_dynthresh.h"

#define DT_LANES 1024
#define DT_WAVES (DT_LANES / 64)
#define DT_COPIES 8          // histogram copies, selected by lane & 7: a wave's lanes mostly hit ONE bin in the first pass
#define DT_HOLD_MIM_MAX 4    // pixels per lane up to which mim is held beside cfg (VGPR budget of a 1024-lane workgroup: 128)

struct DTArgs {
    const float4* u;      // [batch][P]
    const float4* c;      // [batch][P]
    float4* out;          // [batch][P]
    const float* scales;
    const int* step_ptr;
    const int* params;
    int P, num_steps;
};

__device__ __forceinline__ float4 dt_comb(float s, const float4 u, const float4 c) {
    return make_float4(__fmaf_rn(s, __fsub_rn(c.x, u.x), u.x), __fmaf_rn(s, __fsub_rn(c.y, u.y), u.y),
                       __fmaf_rn(s, __fsub_rn(c.z, u.z), u.z), __fmaf_rn(s, __fsub_rn(c.w, u.w), u.w));
}
__device__ __forceinline__ uint32_t dt_key(float v, float mean) { return __float_as_uint(__fsub_rn(v, mean)) & 0x7FFFFFFFu; }

// wave-wide reduction of a 32-bit integer, result on every lane: wave_sum's cross-lane moves (common.h)
#define DT_DPPU(v, ctrl) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), 0xF, 0xF, true))
template <class Op>
__device__ __forceinline__ uint32_t dt_wave_reduce(uint32_t v, Op op) {
    v = op(v, DT_DPPU(v, 0xB1));
    v = op(v, DT_DPPU(v, 0x4E));
    v = op(v, DT_DPPU(v, 0x124));
    v = op(v, DT_DPPU(v, 0x128));
    auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = op((uint32_t)a[0], (uint32_t)a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return op((uint32_t)b[0], (uint32_t)b[1]);
}

// the lane's pixels in ascending order: f(k, px), k the register slot
template <int NPT, class F>
__device__ __forceinline__ void dt_each(int tid, int P, F f) {   // (the lambdas are always_inline: what they capture stays in registers)
    if constexpr (NPT > 0) {
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int px = tid + k * DT_LANES;
            if (px < P) f(k, px);
        }
    } else {
#pragma unroll 1   // (generic form: left to itself the compiler unrolls further and spills; this form runs without scratch too)
        for (int px = tid; px < P; px += 2 * DT_LANES) {   // two pixels' loads in flight
            f(0, px);
            if (px + DT_LANES < P) f(0, px + DT_LANES);
        }
    }
}

// K sums (MAX: maxima) over the workgroup, on every lane: wave tree, then the waves in ascending order
template <int K, bool MAX>
__device__ __forceinline__ void dt_block_reduce(float (&v)[K], float (*red)[8], int lane, int wave) {
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = MAX ? wave_max(v[j]) : wave_sum(v[j]);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < K; ++j) red[wave][j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = red[0][j];
#pragma unroll 4   // (not all 16 x K values in flight at once: the held pixels own the registers)
    for (int w = 1; w < DT_WAVES; ++w) {
#pragma unroll
        for (int j = 0; j < K; ++j) v[j] = MAX ? fmaxf(v[j], red[w][j]) : __fadd_rn(v[j], red[w][j]);
    }
}

template <int NPT>
__global__ __launch_bounds__(DT_LANES) void dynthresh_kernel(const DTArgs p) {
    constexpr bool HOLD = NPT > 0, HOLD_MIM = NPT > 0 && NPT <= DT_HOLD_MIM_MAX;
    __shared__ __attribute__((aligned(16))) int hist[4 * 256 * DT_COPIES];   // [channel][bin][copy]: 32 KiB
    __shared__ float red_a[DT_WAVES][8], red_b[DT_WAVES][8];
    __shared__ uint32_t red_c[DT_WAVES][4];
    __shared__ int wtot[DT_WAVES];
    __shared__ int sel[4][4];   // per channel: the bin that holds the rank, the rank inside it, its count

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int P = p.P;
    const size_t base = (size_t)blockIdx.x * P;
    const float4* U = p.u + base;
    const float4* C = p.c + base;
    float4* O = p.out + base;

    int step = p.step_ptr ? *p.step_ptr : 0;
    step = min(max(step, 0), p.num_steps - 1);
    const float g = p.scales[2 * (size_t)step], m = p.scales[2 * (size_t)step + 1];
    const int lo = min(max(p.params[0], 0), P - 1);
    const int measure = p.params[1], startpoint = p.params[2];
    const float frac = __int_as_float(p.params[3]), phi = __int_as_float(p.params[4]);

    {   // the lane's own (channel, bin) counters
        int4* h4 = reinterpret_cast<int4*>(hist) + tid * (DT_COPIES / 4);
        h4[0] = make_int4(0, 0, 0, 0);
        h4[1] = make_int4(0, 0, 0, 0);
    }

    float4 rc[HOLD ? NPT : 1], rm[HOLD_MIM ? NPT : 1];
    auto cfg_at = [&](int k, int px) __attribute__((always_inline)) -> float4 {
        if constexpr (HOLD) return rc[k];
        else return dt_comb(g, U[px], C[px]);
    };
    auto mim_at = [&](int k, int px) __attribute__((always_inline)) -> float4 {
        if constexpr (HOLD_MIM) return rm[k];
        else return dt_comb(m, U[px], C[px]);
    };

    // ---- A: the means
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    dt_each<NPT>(tid, P, [&](int k, int px) __attribute__((always_inline)) {
        const float4 u = U[px], c = C[px];
        const float4 cf = dt_comb(g, u, c), mi = dt_comb(m, u, c);
        if constexpr (HOLD) rc[k] = cf;
        if constexpr (HOLD_MIM) rm[k] = mi;
        s[0] = __fadd_rn(s[0], cf.x); s[1] = __fadd_rn(s[1], cf.y); s[2] = __fadd_rn(s[2], cf.z); s[3] = __fadd_rn(s[3], cf.w);
        s[4] = __fadd_rn(s[4], mi.x); s[5] = __fadd_rn(s[5], mi.y); s[6] = __fadd_rn(s[6], mi.z); s[7] = __fadd_rn(s[7], mi.w);
    });
    dt_block_reduce<8, false>(s, red_a, lane, wave);
    float mean_cfg[4], mean_mim[4];
    const float fP = (float)P;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mean_cfg[j] = __fdiv_rn(s[j], fP);
        mean_mim[j] = __fdiv_rn(s[4 + j], fP);
    }

    // ---- B: the spread of mim (and, "std", of cfg)
    float mim_ref[4], cfg_ref[4];
    if (measure == 0) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        dt_each<NPT>(tid, P, [&](int k, int px) __attribute__((always_inline)) {
            const float4 mi = mim_at(k, px);
            t[0] = fmaxf(t[0], fabsf(__fsub_rn(mi.x, mean_mim[0])));
            t[1] = fmaxf(t[1], fabsf(__fsub_rn(mi.y, mean_mim[1])));
            t[2] = fmaxf(t[2], fabsf(__fsub_rn(mi.z, mean_mim[2])));
            t[3] = fmaxf(t[3], fabsf(__fsub_rn(mi.w, mean_mim[3])));
        });
        dt_block_reduce<4, true>(t, red_b, lane, wave);
#pragma unroll
        for (int j = 0; j < 4; ++j) mim_ref[j] = t[j];
    } else {
        float t[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        dt_each<NPT>(tid, P, [&](int k, int px) __attribute__((always_inline)) {
            const float4 mi = mim_at(k, px), cf = cfg_at(k, px);
            const float d0 = __fsub_rn(mi.x, mean_mim[0]), d1 = __fsub_rn(mi.y, mean_mim[1]);
            const float d2 = __fsub_rn(mi.z, mean_mim[2]), d3 = __fsub_rn(mi.w, mean_mim[3]);
            const float e0 = __fsub_rn(cf.x, mean_cfg[0]), e1 = __fsub_rn(cf.y, mean_cfg[1]);
            const float e2 = __fsub_rn(cf.z, mean_cfg[2]), e3 = __fsub_rn(cf.w, mean_cfg[3]);
            t[0] = __fmaf_rn(d0, d0, t[0]); t[1] = __fmaf_rn(d1, d1, t[1]); t[2] = __fmaf_rn(d2, d2, t[2]); t[3] = __fmaf_rn(d3, d3, t[3]);
            t[4] = __fmaf_rn(e0, e0, t[4]); t[5] = __fmaf_rn(e1, e1, t[5]); t[6] = __fmaf_rn(e2, e2, t[6]); t[7] = __fmaf_rn(e3, e3, t[7]);
        });
        dt_block_reduce<8, false>(t, red_b, lane, wave);
        const float fP1 = (float)(P - 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mim_ref[j] = __fsqrt_rn(__fdiv_rn(t[j], fP1));
            cfg_ref[j] = __fsqrt_rn(__fdiv_rn(t[4 + j], fP1));
        }
    }

    if (measure == 0 && lo == P - 1) {
        // ---- C': percentile 1 (the default): s[P - 1] is the largest key, one max reduction; frac is 0 there (hi = lo)
        uint32_t mxk[4] = {0u, 0u, 0u, 0u};
        dt_each<NPT>(tid, P, [&](int k, int px) __attribute__((always_inline)) {
            const float4 cf = cfg_at(k, px);
            mxk[0] = max(mxk[0], dt_key(cf.x, mean_cfg[0]));
            mxk[1] = max(mxk[1], dt_key(cf.y, mean_cfg[1]));
            mxk[2] = max(mxk[2], dt_key(cf.z, mean_cfg[2]));
            mxk[3] = max(mxk[3], dt_key(cf.w, mean_cfg[3]));
        });
#pragma unroll
        for (int j = 0; j < 4; ++j) mxk[j] = dt_wave_reduce(mxk[j], [](uint32_t x, uint32_t y) __attribute__((always_inline)) { return max(x, y); });
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red_c[wave][j] = mxk[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) mxk[j] = red_c[0][j];
#pragma unroll 4
        for (int w = 1; w < DT_WAVES; ++w) {
#pragma unroll
            for (int j = 0; j < 4; ++j) mxk[j] = max(mxk[j], red_c[w][j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cfg_ref[j] = __uint_as_float(mxk[j]);
    } else if (measure == 0) {
        // ---- C: the lo-th smallest key of every channel
        uint32_t prefix[4] = {0u, 0u, 0u, 0u};
        int rk[4] = {lo, lo, lo, lo}, cnt_sel[4] = {0, 0, 0, 0};
        const int copy = lane & (DT_COPIES - 1);
        const int ch = tid >> 8;   // the (channel, bin) this lane scans: four waves per channel
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            dt_each<NPT>(tid, P, [&](int k, int px) __attribute__((always_inline)) {
                const float4 cf = cfg_at(k, px);
                const uint32_t key[4] = {dt_key(cf.x, mean_cfg[0]), dt_key(cf.y, mean_cfg[1]), dt_key(cf.z, mean_cfg[2]),
                                         dt_key(cf.w, mean_cfg[3])};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (pass == 0 || (key[j] >> ((shift + 8) & 31)) == prefix[j])
                        atomicAdd(&hist[(j * 256 + (int)((key[j] >> shift) & 255u)) * DT_COPIES + copy], 1);
                }
            });
            __syncthreads();
            int4* h4 = reinterpret_cast<int4*>(hist) + tid * (DT_COPIES / 4);
            const int4 a = h4[0], b = h4[1];
            h4[0] = make_int4(0, 0, 0, 0);
            h4[1] = make_int4(0, 0, 0, 0);
            const int cnt = a.x + a.y + a.z + a.w + b.x + b.y + b.z + b.w;
            int incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            int before = 0;
#pragma unroll
            for (int w = 0; w < 3; ++w) before += (ch * 4 + w < wave) ? wtot[ch * 4 + w] : 0;
            incl += before;
            const int excl = incl - cnt;
            const int mine = ch == 0 ? rk[0] : ch == 1 ? rk[1] : ch == 2 ? rk[2] : rk[3];
            if (excl <= mine && mine < incl) {
                sel[ch][0] = tid & 255;
                sel[ch][1] = mine - excl;
                sel[ch][2] = cnt;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                prefix[j] = (prefix[j] << 8) | (uint32_t)sel[j][0];
                rk[j] = sel[j][1];
                cnt_sel[j] = sel[j][2];
            }
        }
        // ---- D: s[hi]
        uint32_t mn[4] = {~0u, ~0u, ~0u, ~0u};
        dt_each<NPT>(tid, P, [&](int k, int px) __attribute__((always_inline)) {
            const float4 cf = cfg_at(k, px);
            const uint32_t key[4] = {dt_key(cf.x, mean_cfg[0]), dt_key(cf.y, mean_cfg[1]), dt_key(cf.z, mean_cfg[2]),
                                     dt_key(cf.w, mean_cfg[3])};
#pragma unroll
            for (int j = 0; j < 4; ++j) mn[j] = key[j] > prefix[j] ? min(mn[j], key[j]) : mn[j];
        });
#pragma unroll
        for (int j = 0; j < 4; ++j) mn[j] = dt_wave_reduce(mn[j], [](uint32_t x, uint32_t y) __attribute__((always_inline)) { return min(x, y); });
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) red_c[wave][j] = mn[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) mn[j] = red_c[0][j];
#pragma unroll 4
        for (int w = 1; w < DT_WAVES; ++w) {
#pragma unroll
            for (int j = 0; j < 4; ++j) mn[j] = min(mn[j], red_c[w][j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t v = mn[j];
            const float s_lo = __uint_as_float(prefix[j]);
            // the (lo + 1)-th smallest is s[lo] again unless lo is the last of its ties; hi = min(lo + 1, P - 1)
            const bool next = rk[j] + 1 >= cnt_sel[j] && lo + 1 <= P - 1;
            const float s_hi = next ? __uint_as_float(v) : s_lo;
            cfg_ref[j] = __fmaf_rn(frac, __fsub_rn(s_hi, s_lo), s_lo);
        }
    }

    // ---- E: the output
    const bool zero = startpoint != 0, clampit = startpoint == 0 && measure == 0;
    float lim[4], scale[4], add[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float div = clampit ? fmaxf(mim_ref[j], cfg_ref[j]) : cfg_ref[j];
        ok[j] = div != 0.0f;
        scale[j] = __fdiv_rn(mim_ref[j], div);
        lim[j] = clampit ? div : __builtin_inff();
        add[j] = zero ? 0.0f : mean_cfg[j];
    }
    const float keep = __fsub_rn(1.0f, phi);
    auto one = [&](float cf, int j) __attribute__((always_inline)) -> float {
        const float cc = __fsub_rn(cf, mean_cfg[j]);
        const float x = zero ? cf : fminf(fmaxf(cc, -lim[j]), lim[j]);
        const float r = __fmaf_rn(x, scale[j], add[j]);
        return ok[j] ? __fmaf_rn(phi, r, __fmul_rn(keep, cf)) : cf;
    };
    dt_each<NPT>(tid, P, [&](int k, int px) __attribute__((always_inline)) {
        const float4 cf = cfg_at(k, px);
        O[px] = make_float4(one(cf.x, 0), one(cf.y, 1), one(cf.z, 2), one(cf.w, 3));
    });
}

static bool dt_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

template <int NPT>
static void dt_launch(const DTArgs& a, int batch, hipStream_t stream) {
    hipLaunchKernelGGL(dynthresh_kernel<NPT>, dim3((unsigned)batch), dim3(DT_LANES), 0, stream, a);
}

extern "C" int msdt_dynamic_threshold(const MsdtDynamicThreshold* p, msdt_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "dynamic_threshold: null argument");
    if (!p->eps || !p->out || !p->scales || !p->params) MSD_FAIL(MSD_E_ARG, "dynamic_threshold: null eps / out / scales / params");
    if (!msd_aligned16(p->eps) || !msd_aligned16(p->out) || !msd_aligned16(p->scales) || !msd_aligned16(p->params))
        MSD_FAIL(MSD_E_ARG, "dynamic_threshold: eps / out / scales / params must be 16-byte aligned");
    if (((uintptr_t)p->step_ptr) & 3u) MSD_FAIL(MSD_E_ARG, "dynamic_threshold: step_ptr must be 4-byte aligned");
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "dynamic_threshold: batch %d (1 .. 65535)", p->batch);
    if (p->h < 1 || p->w < 1 || (int64_t)p->h * p->w < 2)
        MSD_FAIL(MSD_E_ARG, "dynamic_threshold: planes of %d x %d (at least 2 values)", p->h, p->w);
    if ((int64_t)p->h * p->w * 4 >= ((int64_t)1 << 31))
        MSD_FAIL(MSD_E_ARG, "dynamic_threshold: %d x %d x 4 values per sample (fewer than 2^31)", p->h, p->w);
    if (p->num_steps < 1) MSD_FAIL(MSD_E_ARG, "dynamic_threshold: num_steps %d (>= 1)", p->num_steps);
    const int P = p->h * p->w;
    {   // out is eps itself, or apart from all of eps; apart from the small operands either way
        const uintptr_t rows = (uintptr_t)p->batch * (uintptr_t)P * 16;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + rows, e0 = (uintptr_t)p->eps, e1 = e0 + 2 * rows;
        if (o0 != e0 && dt_overlap(o0, o1, e0, e1)) MSD_FAIL(MSD_E_ARG, "dynamic_threshold: out is neither eps nor apart from it");
        const uintptr_t s0 = (uintptr_t)p->scales, t0 = (uintptr_t)p->params, c0 = (uintptr_t)p->step_ptr;
        if (dt_overlap(o0, o1, s0, s0 + (uintptr_t)p->num_steps * 8) || dt_overlap(o0, o1, t0, t0 + 32) ||
            (p->step_ptr && dt_overlap(o0, o1, c0, c0 + 4)))
            MSD_FAIL(MSD_E_ARG, "dynamic_threshold: out overlaps scales / params / step_ptr");
    }
    DTArgs a;
    a.u = reinterpret_cast<const float4*>(p->eps);
    a.c = a.u + (size_t)p->batch * P;
    a.out = reinterpret_cast<float4*>(p->out);
    a.scales = p->scales;
    a.step_ptr = p->step_ptr;
    a.params = reinterpret_cast<const int*>(p->params);
    a.P = P;
    a.num_steps = p->num_steps;
    const int per_lane = (P + DT_LANES - 1) / DT_LANES;
    if (per_lane <= 1) dt_launch<1>(a, p->batch, stream);
    else if (per_lane <= 2) dt_launch<2>(a, p->batch, stream);
    else if (per_lane <= 4) dt_launch<4>(a, p->batch, stream);        // 64 x 64 latents
    else if (per_lane <= 8) dt_launch<8>(a, p->batch, stream);        // cfg held, mim recomputed
    else dt_launch<0>(a, p->batch, stream);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
