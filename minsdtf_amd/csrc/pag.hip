// msd_attention_identity: self-attention with the identity attention map, the perturbed branch of perturbed-attention guidance
// (include/minsdtf_hip.h has the contract; minsdtf_amd/pag.py the host side).  With the identity map every query attends to its
// own key alone, so the layer's output is V itself - which the step plan holds only TRANSPOSED, as msd_attention's `vt` operand.
// The kernel is therefore a bf16 transpose  vt [channels][vt_ld] -> out [s][o_ld]  per sample, through LDS.
//
// One workgroup = one 64 (channels) x 64 (keys) tile.  Both global sides move 16 bytes per lane: a row of vt is read in 16-byte
// granules of 8 keys, a row of out is written in granules of 8 channels.  In between, a lane of the output side owns 8 channels x 2
// adjacent keys: it reads 8 dwords (one per channel row, each holding the key pair) and sorts their low / high halves into the two
// output granules.
//
// LDS layout: [64 rows][8 granules] of 16 bytes, granule g of row r stored at position g ^ ((r >> 3) & 7).  (Rows of 16-byte
// granules have a stride that is a multiple of 4 dwords, so 8 consecutive rows always land a multiple of 32 banks apart and no
// padding separates the 8 channel groups of a column read; the XOR does.)
//   store side, ds_write_b128, groups of 8 consecutive lanes: the 8 granules of ONE row, a permutation of its 128 bytes - every
//     bank once;
//   load side, ds_read_b32, groups of 32 lanes = 8 channel groups x 4 key pairs of one granule column: bank = 4 * (g ^ group) +
//     pair, 32 different banks.
// Neither side has a conflict.  Edge tiles: a granule is fetched only if its first key is < s (vt_ld % 8 == 0 keeps the whole
// granule inside the row) and its row is < channels; what the padding columns hold lands in tile positions of keys >= s, which no
// lane writes out.
#include "common.h"

#define AI_TILE 64
#define AI_THREADS 256

__global__ __launch_bounds__(AI_THREADS) void attention_identity_kernel(const bf16_t* __restrict__ vt, bf16_t* __restrict__ out,
                                                                        int channels, int s, int vt_ld, int o_ld) {
    // grid: x = 64 keys, y = 64 channels, z = sample
    __shared__ uint4 tile[AI_TILE * 8];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * AI_TILE, c0 = blockIdx.y * AI_TILE;
    const bf16_t* src = vt + (int64_t)blockIdx.z * channels * vt_ld;
    bf16_t* dst = out + (int64_t)blockIdx.z * s * o_ld;
#pragma unroll
    for (int i = tid; i < AI_TILE * 8; i += AI_THREADS) {
        const int r = i >> 3, g = i & 7;
        const int c = c0 + r, k = k0 + g * 8;
        if (c < channels && k < s)
            tile[r * 8 + (g ^ ((r >> 3) & 7))] = *reinterpret_cast<const uint4*>(src + (int64_t)c * vt_ld + k);
    }
    __syncthreads();
    const int grp = tid & 7, pair = tid >> 3;   // 8 channels c0 + 8 grp .., keys k0 + 2 pair, + 1
    const int c = c0 + grp * 8, k = k0 + 2 * pair;
    if (c >= channels || k >= s) return;
    const uint32_t* t32 = reinterpret_cast<const uint32_t*>(tile);
    const int col = (((pair >> 2) ^ grp) << 2) + (pair & 3);   // (rows 8 grp .. 8 grp + 7 share the swizzle term grp)
    uint32_t d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = t32[(grp * 8 + j) * 32 + col];
    uint4 lo, hi;
    lo.x = (d[0] & 0xFFFFu) | (d[1] << 16); hi.x = (d[0] >> 16) | (d[1] & 0xFFFF0000u);
    lo.y = (d[2] & 0xFFFFu) | (d[3] << 16); hi.y = (d[2] >> 16) | (d[3] & 0xFFFF0000u);
    lo.z = (d[4] & 0xFFFFu) | (d[5] << 16); hi.z = (d[4] >> 16) | (d[5] & 0xFFFF0000u);
    lo.w = (d[6] & 0xFFFFu) | (d[7] << 16); hi.w = (d[6] >> 16) | (d[7] & 0xFFFF0000u);
    *reinterpret_cast<uint4*>(dst + (int64_t)k * o_ld + c) = lo;
    if (k + 1 < s) *reinterpret_cast<uint4*>(dst + (int64_t)(k + 1) * o_ld + c) = hi;
}

extern "C" int msd_attention_identity(const MsdAttentionIdentity* p, msd_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p) MSD_FAIL(MSD_E_ARG, "attention_identity: null argument");
    if (!p->vt || !p->out) MSD_FAIL(MSD_E_ARG, "attention_identity: null vt / out");
    if (!msd_aligned16(p->vt) || !msd_aligned16(p->out)) MSD_FAIL(MSD_E_ARG, "attention_identity: vt / out must be 16-byte aligned");
    if (p->batch < 1 || p->batch > 65535) MSD_FAIL(MSD_E_ARG, "attention_identity: batch %d (1 .. 65535)", p->batch);
    if (p->s < 1) MSD_FAIL(MSD_E_ARG, "attention_identity: s = %d (>= 1)", p->s);
    if (p->channels < 8 || (p->channels % 8)) MSD_FAIL(MSD_E_ARG, "attention_identity: channels = %d (a positive multiple of 8)", p->channels);
    if (p->vt_ld % 8) MSD_FAIL(MSD_E_ARG, "attention_identity: vt_ld = %d (vt_ld %% 8 == 0: rows are read in 16-byte granules)", p->vt_ld);
    if (p->vt_ld < p->s) MSD_FAIL(MSD_E_ARG, "attention_identity: vt_ld = %d < s = %d", p->vt_ld, p->s);
    if (p->o_ld < p->channels) MSD_FAIL(MSD_E_ARG, "attention_identity: o_ld = %d < channels = %d", p->o_ld, p->channels);
    if (p->o_ld % 8) MSD_FAIL(MSD_E_ARG, "attention_identity: o_ld = %d (o_ld %% 8 == 0: rows of out must be 16-byte aligned)", p->o_ld);
    const int64_t n_vt = (int64_t)p->batch * p->channels * p->vt_ld, n_out = (int64_t)p->batch * p->s * p->o_ld;
    if (n_vt >= (1ll << 31) || n_out >= (1ll << 31)) MSD_FAIL(MSD_E_ARG, "attention_identity: 2^31 or more elements in vt or out");
    {   // the bytes read and the bytes written lie apart (the last row of each ends where its data ends, not at its stride)
        const int64_t e_vt = n_vt - p->vt_ld + (p->s + 7) / 8 * 8, e_out = n_out - p->o_ld + p->channels;
        const uintptr_t v0 = (uintptr_t)p->vt, v1 = v0 + (uintptr_t)e_vt * 2;
        const uintptr_t o0 = (uintptr_t)p->out, o1 = o0 + (uintptr_t)e_out * 2;
        if (v0 < o1 && o0 < v1) MSD_FAIL(MSD_E_ARG, "attention_identity: out overlaps vt");
    }
    const dim3 grid((unsigned)((p->s + AI_TILE - 1) / AI_TILE), (unsigned)((p->channels + AI_TILE - 1) / AI_TILE), (unsigned)p->batch);
    hipLaunchKernelGGL(attention_identity_kernel, grid, dim3(AI_THREADS), 0, stream, reinterpret_cast<const bf16_t*>(p->vt),
                       reinterpret_cast<bf16_t*>(p->out), p->channels, p->s, p->vt_ld, p->o_ld);
    MSD_CHECK_LAUNCH();
    return MSD_OK;
}
