// msd_lora_merge: a LoRA switch rewrites the packed weights in place (include/minsdtf_hip.h; minsdtf_amd/lora.py).
//
// One wave per workgroup, LR_ROWS logical rows of one job per workgroup.  The rows' up-factors are staged in LDS ([rank][LR_ROWS],
// read as broadcasts); each lane owns 8 consecutive columns per pass (pass width 512), so its loads of master / down are 32-byte
// runs and its stores are one 16-byte vector in every bf16 layout (rows, chunk-major, fragment-major: 8 consecutive k aligned to 8
// are contiguous in all three).  The low-rank product is fp32 FMA in rank order; the master add, the row scale and the column scale
// are separately rounded (__fadd_rn / __fmul_rn), so a rank-0 job reproduces the load-time packing bit for bit.
#include "common.h"

#define LR_ROWS 8
#define LR_LANES 64
#define LR_COLS 8
#define LR_MAX_RANK 512

static __constant__ const int kFragRow[16] = {0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15};   // packing.FRAGMENT_ROW_ORDER (an involution)

__device__ __forceinline__ void load8(const float* p, int k0, int K, bool vec, float* v) {
    if (vec && k0 + 8 <= K) {
        const float4 a = *reinterpret_cast<const float4*>(p + k0), b = *reinterpret_cast<const float4*>(p + k0 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (k0 + e < K) ? p[k0 + e] : 0.f;
    }
}

__device__ __forceinline__ uint4 pack8_bits(const uint16_t* h) {
    uint4 w;
    w.x = h[0] | ((uint32_t)h[1] << 16); w.y = h[2] | ((uint32_t)h[3] << 16);
    w.z = h[4] | ((uint32_t)h[5] << 16); w.w = h[6] | ((uint32_t)h[7] << 16);
    return w;
}

__global__ __launch_bounds__(LR_LANES) void lora_merge_kernel(const MsdLoraJob* __restrict__ jobs, int num_jobs) {
    extern __shared__ float su[];   // [rank][LR_ROWS]
    const int bid = blockIdx.x, lane = threadIdx.x;
    // the job of this workgroup: the last one whose first_block <= bid
    int lo = 0, hi = num_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= bid) lo = mid; else hi = mid - 1;
    }
    const MsdLoraJob J = jobs[lo];
    const int n0 = (bid - J.first_block) * LR_ROWS;
    const int N = J.n, K = J.k, R = J.rank;
    for (int i = lane; i < R * LR_ROWS; i += LR_LANES) {
        const int j = i / LR_ROWS, r = i % LR_ROWS;
        su[i] = (n0 + r < N) ? J.up[(int64_t)(n0 + r) * R + j] : 0.f;
    }
    __syncthreads();

    int dest[LR_ROWS];
    float rs[LR_ROWS];
#pragma unroll
    for (int r = 0; r < LR_ROWS; ++r) {
        const int n = n0 + r;
        int d = -1;
        if (n < N) {
            d = (J.rowmap ? J.rowmap[n] : n) + J.row_off;
            if (d < 0 || d >= J.out_rows) d = -1;
        }
        dest[r] = d;
        rs[r] = (n < N && J.rowscale) ? J.rowscale[n] : 1.f;
    }
    const bool mvec = ((J.master_ld & 3) == 0) && ((((uintptr_t)J.master) & 15) == 0);
    const bool dvec = ((K & 3) == 0) && ((((uintptr_t)J.down) & 15) == 0);
    const bool cvec = (((uintptr_t)J.colscale) & 15) == 0;
    const bool bf = J.out_dtype == MSD_OUT_BF16;
    double csum[LR_ROWS];
#pragma unroll
    for (int r = 0; r < LR_ROWS; ++r) csum[r] = 0.0;

    for (int k0 = lane * LR_COLS; k0 < K; k0 += LR_LANES * LR_COLS) {
        float acc[LR_ROWS][LR_COLS];
#pragma unroll
        for (int r = 0; r < LR_ROWS; ++r)
#pragma unroll
            for (int e = 0; e < LR_COLS; ++e) acc[r][e] = 0.f;
        for (int j = 0; j < R; ++j) {
            float d[LR_COLS];
            load8(J.down + (int64_t)j * K, k0, K, dvec, d);
            const float4 ua = *reinterpret_cast<const float4*>(&su[j * LR_ROWS]);
            const float4 ub = *reinterpret_cast<const float4*>(&su[j * LR_ROWS + 4]);
            const float u[LR_ROWS] = {ua.x, ua.y, ua.z, ua.w, ub.x, ub.y, ub.z, ub.w};
#pragma unroll
            for (int r = 0; r < LR_ROWS; ++r)
#pragma unroll
                for (int e = 0; e < LR_COLS; ++e) acc[r][e] = __builtin_fmaf(u[r], d[e], acc[r][e]);
        }
        float cs[LR_COLS];
        if (J.colscale) load8(J.colscale, k0, K, cvec, cs);
        const int nvalid = min(LR_COLS, K - k0);
        const int c0 = J.col_off + k0;   // destination column of element 0
#pragma unroll
        for (int r = 0; r < LR_ROWS; ++r) {
            if (dest[r] < 0) continue;
            const int64_t drow = dest[r];
            float v[LR_COLS];
            load8(J.master + (int64_t)(n0 + r) * J.master_ld, k0, K, mvec, v);
#pragma unroll
            for (int e = 0; e < LR_COLS; ++e) {
                if (R > 0) v[e] = __fadd_rn(v[e], acc[r][e]);
                if (J.rowscale) v[e] = __fmul_rn(v[e], rs[r]);
                if (J.colscale) v[e] = __fmul_rn(v[e], cs[e]);
            }
            if (bf) {
                uint16_t h[LR_COLS];
#pragma unroll
                for (int e = 0; e < LR_COLS; ++e) {
                    h[e] = f2bf(v[e]);
                    if (e < nvalid) csum[r] += (double)bf2f(h[e]);
                }
                uint16_t* o = reinterpret_cast<uint16_t*>(J.out);
                // primary layout
                const bool full = nvalid == LR_COLS && (c0 & 7) == 0;
                if (J.layout == 0) {
                    const int64_t idx = drow * J.ld + c0;
                    if (full && (idx & 7) == 0 && (((uintptr_t)o) & 15) == 0) {
                        *reinterpret_cast<uint4*>(o + idx) = pack8_bits(h);
                    } else {
#pragma unroll
                        for (int e = 0; e < LR_COLS; ++e) if (e < nvalid) o[idx + e] = h[e];
                    }
                } else {   // chunk-major
                    if (full && (((uintptr_t)o) & 15) == 0) {
                        const int64_t idx = ((int64_t)(c0 >> 6) * J.out_rows + drow) * 64 + (c0 & 63);
                        *reinterpret_cast<uint4*>(o + idx) = pack8_bits(h);
                    } else {
#pragma unroll
                        for (int e = 0; e < LR_COLS; ++e) {
                            const int c = c0 + e;
                            if (e < nvalid) o[((int64_t)(c >> 6) * J.out_rows + drow) * 64 + (c & 63)] = h[e];
                        }
                    }
                }
                if (J.out_frag) {   // [K/64][N/16][2][4][16][8]
                    uint16_t* f = reinterpret_cast<uint16_t*>(J.out_frag);
                    const int64_t nb = drow >> 4, rp = kFragRow[drow & 15], NB = J.out_rows >> 4;
                    auto fidx = [&](int c) -> int64_t {
                        return (((((int64_t)(c >> 6) * NB + nb) * 2 + ((c >> 5) & 1)) * 4 + ((c >> 3) & 3)) * 16 + rp) * 8 + (c & 7);
                    };
                    if (full && (((uintptr_t)f) & 15) == 0) {
                        *reinterpret_cast<uint4*>(f + fidx(c0)) = pack8_bits(h);
                    } else {
#pragma unroll
                        for (int e = 0; e < LR_COLS; ++e) if (e < nvalid) f[fidx(c0 + e)] = h[e];
                    }
                }
            } else {
                float* o = reinterpret_cast<float*>(J.out);
                if (J.layout == 0) {
                    const int64_t idx = drow * J.ld + c0;
                    if (nvalid == LR_COLS && (idx & 3) == 0 && (((uintptr_t)o) & 15) == 0) {
                        *reinterpret_cast<float4*>(o + idx) = make_float4(v[0], v[1], v[2], v[3]);
                        *reinterpret_cast<float4*>(o + idx + 4) = make_float4(v[4], v[5], v[6], v[7]);
                    } else {
#pragma unroll
                        for (int e = 0; e < LR_COLS; ++e) if (e < nvalid) o[idx + e] = v[e];
                    }
                } else {   // transposed rows
#pragma unroll
                    for (int e = 0; e < LR_COLS; ++e) if (e < nvalid) o[(int64_t)(c0 + e) * J.out_rows + drow] = v[e];
                }
            }
        }
    }
    if (J.colsum) {   // fixed-order butterfly over the wave, lane 0 writes
#pragma unroll
        for (int r = 0; r < LR_ROWS; ++r) {
            double s = csum[r];
            for (int m = 1; m < LR_LANES; m <<= 1) s += __shfl_xor(s, m);
            if (lane == 0 && dest[r] >= 0) J.colsum[dest[r]] = (float)s;
        }
    }
}

static int lr_check(const MsdLoraJob& j, int i, int64_t expect_first) {
    if (!j.master || !j.out) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: null master / out", i);
    if (j.n <= 0 || j.k <= 0 || j.rank < 0 || j.rank > LR_MAX_RANK)
        MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: n %d, k %d, rank %d (rank <= %d)", i, j.n, j.k, j.rank, LR_MAX_RANK);
    if (j.rank > 0 && (!j.up || !j.down)) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: rank %d without up / down", i, j.rank);
    if (j.master_ld < j.k) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: master_ld %d < k %d", i, j.master_ld, j.k);
    if (j.out_dtype != MSD_OUT_BF16 && j.out_dtype != MSD_OUT_F32) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: out_dtype %d", i, j.out_dtype);
    if (j.layout < 0 || j.layout > 2) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: layout %d", i, j.layout);
    if (j.layout == 1 && (j.out_dtype != MSD_OUT_BF16 || j.out_cols % 64))
        MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: chunk-major needs bf16 and out_cols %% 64 == 0", i);
    if (j.layout == 2 && j.out_dtype != MSD_OUT_F32) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: the transposed layout is fp32", i);
    if (j.out_rows <= 0 || j.out_cols <= 0) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: destination %d x %d", i, j.out_rows, j.out_cols);
    if (j.layout == 0 && j.ld < j.out_cols) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: ld %d < out_cols %d", i, j.ld, j.out_cols);
    if (j.col_off < 0 || (int64_t)j.col_off + j.k > j.out_cols) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: columns outside the destination", i);
    if (j.row_off < 0 && !j.rowmap) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: row_off %d", i, j.row_off);
    if (!j.rowmap && (int64_t)j.row_off + j.n > j.out_rows) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: rows outside the destination", i);
    if (j.out_frag && (j.out_dtype != MSD_OUT_BF16 || j.out_rows % 16 || j.out_cols % 64))
        MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: the fragment-major copy needs bf16, out_rows %% 16 == 0, out_cols %% 64 == 0", i);
    if (j.colsum && (j.out_dtype != MSD_OUT_BF16 || j.col_off != 0 || j.k != j.out_cols))
        MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: colsum needs bf16 and whole destination rows", i);
    if ((((uintptr_t)j.master) | ((uintptr_t)j.up) | ((uintptr_t)j.down) | ((uintptr_t)j.rowscale) | ((uintptr_t)j.colscale) |
         ((uintptr_t)j.rowmap) | ((uintptr_t)j.colsum)) & 3)
        MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: fp32 / int32 operands must be 4-byte aligned", i);
    if ((((uintptr_t)j.out) | ((uintptr_t)j.out_frag)) & (j.out_dtype == MSD_OUT_F32 ? 3 : 1))
        MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: misaligned destination", i);
    if (j.first_block != expect_first) MSD_FAIL(MSD_E_ARG, "lora_merge: job %d: first_block %d, expected %lld", i, j.first_block, (long long)expect_first);
    return MSD_OK;
}

extern "C" int msd_lora_merge(const MsdLoraMerge* p, msd_stream_t stream) {
    if (!p) MSD_FAIL(MSD_E_ARG, "lora_merge: null argument");
    if (p->num_jobs < 0) MSD_FAIL(MSD_E_ARG, "lora_merge: num_jobs %d", p->num_jobs);
    if (p->num_jobs == 0) return MSD_OK;
    if (!p->jobs || !p->jobs_dev) MSD_FAIL(MSD_E_ARG, "lora_merge: null job array");
    int64_t blocks = 0;
    int max_rank = 0;
    for (int i = 0; i < p->num_jobs; ++i) {
        const int rc = lr_check(p->jobs[i], i, blocks);
        if (rc) return rc;
        max_rank = max(max_rank, p->jobs[i].rank);
        blocks += (p->jobs[i].n + LR_ROWS - 1) / LR_ROWS;
        if (blocks > 0x7FFFFFFF) MSD_FAIL(MSD_E_ARG, "lora_merge: too many rows in one launch");
    }
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)blocks), dim3(LR_LANES), max_rank * LR_ROWS * sizeof(float), (hipStream_t)stream, p->jobs_dev, p->num_jobs);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
