// msd_tile_consensus: the per-step hand-off of a tiled-diffusion job (include/minsdtf_hip.h has the formula and the pinned order
// of the sums; minsdtf_amd/tiled.py builds the offsets and the weight rows).
//
// One lane = one canvas pixel of one sample = one float4.  The views that cover a pixel are a contiguous range of view rows
// times a contiguous range of view columns (the offsets of an axis ascend strictly), found by walking the two offset lists,
// which sit in the kernel arguments: a wave reads them through the scalar cache.  A pixel under n views costs n 16-byte loads,
// n + 1 16-byte stores and two fp32 weights per view; a 1024 x 768 canvas (96 x 128 latent pixels) is 48 workgroups per sample,
// so the kernel sits at the launch floor, which is the point - it is one more launch in the step plan, inside the captured
// graph.  Each tile entry belongs to exactly one canvas pixel: the in-place rewrite of the tiles needs no atomics, and nothing
// couples two pixels, so a sample's bits do not depend on its batch.
#include "common.h"

#define TC_THREADS 256

struct TcOffsets {
    int ys[MSD_TILE_MAX_VIEWS];
    int xs[MSD_TILE_MAX_VIEWS];
};

// first / last view of an axis that covers coordinate p (off ascends strictly: the covering views are one range)
__device__ __forceinline__ void tc_cover(const int* off, int n, int t, int p, int& first, int& last) {
    first = n;
    last = -1;
    for (int i = 0; i < n; ++i) {
        const int d = p - off[i];
        if (d >= 0 && d < t) {
            first = min(first, i);
            last = i;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(TC_THREADS) void tile_consensus_kernel(float4* __restrict__ tiles, float4* __restrict__ canvas,
                                                                    const float* __restrict__ wy, const float* __restrict__ wx,
                                                                    const TcOffsets off, int rows, int cols, int th, int tw, int H, int W) {
    // grid: x = TC_THREADS consecutive pixels of a sample's canvas (row-major), y = sample
    const int pix = blockIdx.x * TC_THREADS + threadIdx.x;
    if (pix >= H * W) return;
    const int Y = pix / W, X = pix - Y * W;
    const int b = blockIdx.y;
    int r0, r1, c0, c1;
    tc_cover(off.ys, rows, th, Y, r0, r1);
    tc_cover(off.xs, cols, tw, X, c0, c1);
    if (r1 < r0 || c1 < c0) return;   // (the host checked that the views cover the canvas)
    float4* tb = tiles + (int64_t)b * rows * cols * th * tw;
    const int64_t o = (int64_t)b * H * W + pix;
    float4 v;
    if (MODE == 1) {
        v = canvas[o];
    } else {
        if (r1 == r0 && c1 == c0) {   // one cover: the entry itself, and the tile already holds it
            canvas[o] = tb[((int64_t)(r0 * cols + c0) * th + (Y - off.ys[r0])) * tw + (X - off.xs[c0])];
            return;
        }
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        float wsum = 0.f;
        for (int r = r0; r <= r1; ++r) {
            const int dy = Y - off.ys[r];
            const float fy = wy[dy];
            for (int c = c0; c <= c1; ++c) {
                const int dx = X - off.xs[c];
                const float w = __fmul_rn(fy, wx[dx]);   // (rounded once: never contracted into the sums)
                const float4 x = tb[((int64_t)(r * cols + c) * th + dy) * tw + dx];
                acc = make_float4(__fmaf_rn(w, x.x, acc.x), __fmaf_rn(w, x.y, acc.y), __fmaf_rn(w, x.z, acc.z), __fmaf_rn(w, x.w, acc.w));
                wsum = __fadd_rn(wsum, w);
            }
        }
        v = make_float4(__fdiv_rn(acc.x, wsum), __fdiv_rn(acc.y, wsum), __fdiv_rn(acc.z, wsum), __fdiv_rn(acc.w, wsum));
        canvas[o] = v;
    }
    for (int r = r0; r <= r1; ++r) {
        const int dy = Y - off.ys[r];
        for (int c = c0; c <= c1; ++c) tb[((int64_t)(r * cols + c) * th + dy) * tw + (X - off.xs[c])] = v;
    }
}

// offsets of one axis: start at 0, end at L - t, ascend strictly in steps of at most t
static bool tc_axis_ok(const int32_t* off, int n, int t, int L) {
    if (off[0] != 0 || off[n - 1] != L - t) return false;
    for (int i = 1; i < n; ++i)
        if (off[i] <= off[i - 1] || off[i] - off[i - 1] > t) return false;
    return true;
}

extern "C" int msd_tile_consensus(const MsdTileConsensus* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "tile_consensus: null argument");
    if (!p->tiles || !p->canvas || !p->wy || !p->wx) MSD_FAIL(MSD_E_ARG, "tile_consensus: null tiles / canvas / wy / wx");
    if (!msd_aligned16(p->tiles) || !msd_aligned16(p->canvas) || !msd_aligned16(p->wy) || !msd_aligned16(p->wx))
        MSD_FAIL(MSD_E_ARG, "tile_consensus: tiles / canvas / wy / wx must be 16-byte aligned");
    if (p->mode != 0 && p->mode != 1) MSD_FAIL(MSD_E_ARG, "tile_consensus: mode %d (0: consensus, 1: gather)", p->mode);
    if (p->batch < 1 || p->batch > 65535 || p->th < 1 || p->tw < 1 || p->H < p->th || p->W < p->tw)
        MSD_FAIL(MSD_E_ARG, "tile_consensus: batch %d, tile %d x %d, canvas %d x %d (batch 1 .. 65535, sizes >= 1, canvas >= tile)", p->batch,
                 p->th, p->tw, p->H, p->W);
    if (p->rows < 1 || p->rows > MSD_TILE_MAX_VIEWS || p->cols < 1 || p->cols > MSD_TILE_MAX_VIEWS)
        MSD_FAIL(MSD_E_ARG, "tile_consensus: %d x %d views (1 .. %d per axis)", p->rows, p->cols, MSD_TILE_MAX_VIEWS);
    if (!tc_axis_ok(p->ys, p->rows, p->th, p->H))
        MSD_FAIL(MSD_E_ARG, "tile_consensus: ys must start at 0, end at H - th = %d and ascend strictly in steps of at most th = %d", p->H - p->th,
                 p->th);
    if (!tc_axis_ok(p->xs, p->cols, p->tw, p->W))
        MSD_FAIL(MSD_E_ARG, "tile_consensus: xs must start at 0, end at W - tw = %d and ascend strictly in steps of at most tw = %d", p->W - p->tw,
                 p->tw);
    const int64_t n_canvas = (int64_t)p->batch * p->H * p->W * 4;
    const int64_t n_tiles = (int64_t)p->batch * p->rows * p->cols * p->th * p->tw * 4;
    if (n_canvas >= (1ll << 31) || n_tiles >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "tile_consensus: 2^31 or more elements in tiles or canvas");
    {   // a tile entry and a canvas pixel are written by different lanes
        const uintptr_t t0 = (uintptr_t)p->tiles, t1 = t0 + (uintptr_t)n_tiles * 4;
        const uintptr_t c0 = (uintptr_t)p->canvas, c1 = c0 + (uintptr_t)n_canvas * 4;
        if (t0 < c1 && c0 < t1) MSD_FAIL(MSD_E_ARG, "tile_consensus: canvas overlaps tiles");
    }
    TcOffsets off;
    for (int i = 0; i < MSD_TILE_MAX_VIEWS; ++i) {
        off.ys[i] = i < p->rows ? p->ys[i] : 0;
        off.xs[i] = i < p->cols ? p->xs[i] : 0;
    }
    const dim3 grid((unsigned)((p->H * p->W + TC_THREADS - 1) / TC_THREADS), (unsigned)p->batch);
    float4* tiles = reinterpret_cast<float4*>(p->tiles);
    float4* canvas = reinterpret_cast<float4*>(p->canvas);
    if (p->mode == 0)
        hipLaunchKernelGGL(tile_consensus_kernel<0>, grid, dim3(TC_THREADS), 0, stream, tiles, canvas, p->wy, p->wx, off, p->rows, p->cols,
                           p->th, p->tw, p->H, p->W);
    else
        hipLaunchKernelGGL(tile_consensus_kernel<1>, grid, dim3(TC_THREADS), 0, stream, tiles, canvas, p->wy, p->wx, off, p->rows, p->cols,
                           p->th, p->tw, p->H, p->W);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
