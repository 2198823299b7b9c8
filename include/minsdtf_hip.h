/* minsdtf_hip.h — C ABI of libminsdtf_hip.so: the MI355X (gfx950) kernels behind the
 * SD1.5 denoise hot path of cpuimage/minSDTF.
 *
 * The reference has no native / FFI boundary (it is pure Python over Keras), so
 * there is no reference header to mirror.  Each entry point below replaces the stock Keras op(s)
 * the reference's hot path invokes; the reference call site is cited per function
 * (paths relative to /root/reference/stable_diffusion/).
 *
 * Conventions
 *  - every pointer is a raw DEVICE pointer (hipMalloc / torch tensor.data_ptr()); the caller owns
 *    all memory, including workspaces; nothing is allocated or freed inside the library;
 *  - activations are NHWC ("channels_last", like the reference's Keras tensors), bf16 unless noted;
 *  - `stream` is a hipStream_t; all work is stream-ordered, never synchronises, and is capturable
 *    into a hipGraph;
 *  - return value: 0 on success, a negative MSD_E_* code for an argument error (nothing was
 *    launched), or a positive hipError_t from the launch; msd_last_error() gives the text;
 *  - `step_ptr` (nullable) points at a device int32 holding the current denoise-step index, so a
 *    captured step graph can be replayed for every step: per-step tables (time-embedding
 *    projections, scheduler coefficients) are indexed with it on the device.
 *
 * Memory contract (tests/_extents.py restates it as formulas; the guard bands of the kernel tests, tests/_guard.py, hold every
 * entry point to it, tests/test_plan_extents_cpu.py the launch plans): the comment of every
 * operand below gives its extent - [rows][ld] carrying `cols` columns means the (rows - 1) * ld + cols elements from its base
 * address, a [batch][...][ld] operand described with whole rows means all of them.  No entry point writes a byte outside the
 * extents of its outputs (nor any byte of an input: the unused columns of a wide leading dimension are not its own), and no
 * value outside the extents, nor inside a region documented as padding ("ignored", "unspecified content"), influences a
 * result: callers pack buffers back to back and recycle them, so such bytes hold whatever the previous tenant left, NaN
 * included.  Operands of one launch may overlap only where a comment says so (msd_replicate src == dst, msd_add_f32_bf16
 * out == a, msd_conv_gemm residual == out, msd_region_combine out == eps).
 */
#ifndef MINSDTF_HIP_H
#define MINSDTF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSD_ABI_VERSION 12

#define MSD_OK 0
#define MSD_E_ARG (-1)      /* bad / inconsistent argument */
#define MSD_E_ALIGN (-2)    /* pointer or leading dimension not aligned as required */
#define MSD_E_UNSUPPORTED (-3)
#define MSD_E_WORKSPACE (-4) /* workspace too small */

typedef void* msd_stream_t; /* hipStream_t */

/* The library is built with -fvisibility=hidden: the functions marked MSD_API below are its WHOLE dynamic symbol
 * table (tests/test_host_cpu.py compares `nm -D --defined-only` with this header). */
#if defined(__GNUC__) || defined(__clang__)
#define MSD_API __attribute__((visibility("default")))
#else
#define MSD_API
#endif

MSD_API int msd_abi_version(void);
MSD_API const char* msd_last_error(void);
/* One-time per-process set-up (raises the dynamic-LDS limits of the kernels). Idempotent. */
MSD_API int msd_init(void);
/* Tuning / A-B switches, e.g. ("conv_dense", 0|1), ("attn_qf", 0|1|2|4), ("attn_form", 0|1|2). Returns MSD_E_ARG for an unknown key. */
MSD_API int msd_set_option(const char* key, int value);

/* ------------------------------------------------------------------------------------------
 * msd_conv_gemm — implicit-GEMM convolution / dense layer on MFMA (bf16 in, fp32 accumulate).
 * Replaces: PaddedConv2D 3x3 s1/s2 and 1x1 (layers.py:17-25; diffusion_model.py:29,34,38,62,67,
 * 136,200,209,218), keras Dense (diffusion_model.py:60-65,90,102-108,146; layers.py:33-36),
 * UpSampling2D(2)+conv (diffusion_model.py:132-139; image_decoder.py:36-47), Concatenate feeding
 * a conv (diffusion_model.py:237-273) and the GEGLU gate (diffusion_model.py:142-153).
 *
 *   out[m, n] = epilogue( sum_k A[m, k] * W[n, k] )
 *   m = (b, y, x) output pixel / token,  M = batch*h_out*w_out
 *   k = (tap, c): tap = ky*ksize+kx, c over the concatenated channels of a0|a1, K = taps*(c0+c1)
 *   A[m,(tap,c)] = in[b, y*stride+ky-pad, x*stride+kx-pad, c]  (zero outside; with `upsample`
 *                  the logical input is the stored tensor repeated 2x2, nearest)
 *   W is pre-packed [N][K] bf16 (k contiguous) — see minsdtf_amd/packing.py.
 * Requirements: c0 % 64 == 0, c1 % 64 == 0, N % 4 == 0, all pointers 16-byte aligned,
 *               leading dimensions multiples of 4 elements.
 * Epilogue order: [LayerNorm fold] -> + bias[n] -> + rowvec[step, b, n] -> act -> + residual[m, n] -> store.
 *
 * LayerNorm fold (diffusion_model.py:84-88 followed by a Dense, :102-108 / :146): LN(x) W^T =
 * rstd[m] * (x (gamma*W)^T - mean[m] * colsum[n]) + (beta W^T)[n], so the LayerNormalization in front of
 * a Dense is this GEMM on the RAW rows with gamma folded into W (packing.py), corrected per row in the
 * epilogue; the row moments come from the GEMM that PRODUCED x: with `ln_out` set, a launch writes, per
 * output row and per column tile, the partial (sum, sum of squares) of the bf16 values it stored
 * (float2 [M][ln_out_slots], ln_out_slots = ceil(N / tile_n)); a launch with `ln_in` set sums the
 * `ln_in_slots` partials of each of its rows in a fixed order (bit-reproducible) and applies
 * acc <- rstd * (acc - mean * ln_colsum[n]) before the rest of the epilogue (bias then carries beta W^T + b).
 * Both are plain-K only (no split-K); `ln_out` needs plain mode with a bf16 output.
 */
#define MSD_ACT_NONE 0
#define MSD_ACT_SILU 1
#define MSD_ACT_GEGLU 2 /* W rows interleaved in 16-column x|gate groups; writes N/2 columns */
#define MSD_ACT_QUICK_GELU 3 /* x * sigmoid(1.702 x)  (CLIP MLP, text_encoder.py:100-101) */

#define MSD_OUT_BF16 0
#define MSD_OUT_F32 1

typedef struct MsdConvGemm {
    const void* a0;      /* bf16 [batch][h_in][w_in][c0] */
    const void* a1;      /* bf16 [batch][h_in][w_in][c1] or NULL (channel concat a0|a1) */
    const void* w;       /* bf16 [N][K] */
    const float* bias;   /* [N] or NULL */
    const float* rowvec; /* fp32, element (step*rv_step_stride + b*rv_batch_stride + n) or NULL */
    const int32_t* step_ptr; /* device int32 or NULL (step = 0) */
    const void* residual;    /* bf16 [M][res_ld] or NULL */
    void* out;           /* bf16 or fp32 [M][out_ld]  (split mode: part 0) */
    void* out1;          /* split mode part 1: bf16 [M][out1_ld] */
    void* out2;          /* split mode part 2: bf16 TRANSPOSED [batch][N-ns0-ns1][out2_ld] (token contiguous) */
    float* workspace;    /* fp32 split-K partial slabs, >= splitk*M*N floats (or NULL if splitk<=1) */
    int64_t workspace_floats;
    int32_t batch, h_in, w_in, c0, c1;
    int32_t h_out, w_out;
    int32_t ksize;       /* 1 or 3 */
    int32_t stride;      /* 1 or 2 */
    int32_t pad;         /* 0 or 1 */
    int32_t upsample;    /* 0 or 1: nearest x2 of the stored input before the conv */
    int32_t N;
    int32_t act;
    int32_t out_dtype;
    int32_t out_ld, res_ld;
    int32_t rv_step_stride, rv_batch_stride;
    int32_t split_mode;  /* 0: plain; 1: columns [0,ns0)->out, [ns0,ns0+ns1)->out1, rest->out2 transposed */
    int32_t ns0, ns1, out1_ld, out2_ld;
    int32_t splitk;      /* >=1; K-tiles are divided over this many slices */
    int32_t tile_n;      /* 0 = auto, else 64, 80 or 128 */
    int32_t tile_m;      /* 0 = 128, else 64 / 128 / 256; valid (tile_m x tile_n): 128x128 128x64 64x64 64x128 256x128 128x80;
                            1128 / 1256 = halo-tile 3x3 kernel with 8x16 / 16x16 pixel tiles (x 64 / 80 / 128 channels;
                            falls back if not eligible).  The 80-wide tiles serve N = 320 / 640 at small batch, where
                            they make the workgroup count a multiple of the 256 CUs;
                            4000 + rows (4064 / 4128 / 4256) = the wreg form (csrc/conv_wreg.hip): the weights are read global ->
                            VGPR from the fragment-major image (w_layout 2, required: MSD_E_ARG with any other layout), only the
                            activation tile goes through LDS; tile_n x stages must name a built configuration (MSD_E_UNSUPPORTED
                            otherwise: there is no fallback, the other forms cannot read that image); N % 16 == 0.  Same K walk
                            and epilogue as the tile kernel: the same results bit for bit;
                            5000 + rows (5256 / 5128) = the big form (csrc/conv_big.hip) for M >= 8192: 256 x 256 / 256 x 160 / 256 x 128 /
                            128 x 256 macro tiles on 8 waves whose two halves run one barrier apart (one multiplies while the other
                            reads fragments and issues the LDS-DMAs of the K tile one or two ahead); w_layout 0 or 1; no ln_out;
                            fewer than 2^24 input pixels; tile_n x stages must name a built configuration (MSD_E_UNSUPPORTED
                            otherwise).  Same K walk and epilogue as the tile kernel: the same results bit for bit.
                            tile_m >= 6000: MSD_E_ARG */
    int32_t stages;      /* 0 = default LDS ring depth of the tile; deeper rings built: 128x128:4 64x64:8 64x128:5 128x64:5
                            128x80:4; halo tiles 1128x64:8 1128x128:6 1128x80:8 1256x80:5 (an unknown depth = the default);
                            10 + depth = the tile on 8 waves (two per SIMD): 64x64:14 128x64:13 64x128:13;
                            20 + depth = 64x64 per wave: 128x128:23/24 128x64:24 64x128:24;
                            30 + depth = halo tiles with 3 filter taps (one filter row) per K step: 1128x64:33/34 1128x80:33
                            2128x64:33; 60 + depth = the same with two loader waves that do all the staging: 1128x64:63 1128x80:63;
                            90 + depth = the 60s' form with the K loop rotated (a step's barrier sits between its second and third tap, the
                            next step's first fragments are read under the third tap's MFMAs; same taps in the same order, same bits): 1128x64:93 1128x80:93;
                            150 + depth = the one-tap form rotated (the fragments of tap t + 1 are read under the MFMAs of tap t, every ring
                            stage in flight; same bits): 1128x64:153/158 1128x128:153/156 1128x80:158 1256x80:153/155 1256x128:153;
                            wreg form (tile_m 4000 + rows): depth 3 / 4, + 10 = 8 waves (4256x128: a 2 x 4 wave grid),
                            + 20 = two K tiles (128 channels) per ring stage: 4064x64:4/23/24 4064x128:3/4/23/24 4064x256:3/4/23
                            4128x64:3/4/23 4128x128:3/4/13/23 4256x64:3 4256x128:13/14;
                            big form (tile_m 5000 + rows): a configuration code, not a depth: 5256x256:0 (2 x 2 quadrant phases, 2 K-tile
                            buffers) 5256x160:0/1/2 (quadrants x 3 buffers / row halves x 3 / quadrants x 2) 5256x128:0/1 5128x256:0/1
                            (row halves / quadrants, 3 buffers); + 10 = the same configuration walking K chunk-major (3x3 convs without a
                            shortcut operand only): the halo-tile kernel's order of sums, hence ITS bits instead of the tile kernel's;
                            20 + code with tile_m 5256 = that chunk-major walk over a STAGED 18 x 18-pixel halo per 64-channel chunk
                            (3x3 / stride 1 / pad 1, with or without `upsample`, h_out and w_out multiples of 16; otherwise
                            MSD_E_UNSUPPORTED): 5256x160:20 5256x128:20/21 (weight ring of 3 / 4).  With a shortcut operand (a2) a
                            slice's shortcut chunks follow its main chunks; since round 6 the halo tiles (tile_m 1128 / 2128 / 1256, any
                            of their `stages`) walk a shortcut operand in exactly that order: one numerics class, the halo tiles for
                            small launches, this form from about 128 workgroups on */
    const float* ln_in;      /* float2 [M][ln_in_slots] row-moment partials of the input rows, or NULL */
    const float* ln_colsum;  /* [N]: sum_k W[n][k] of the gamma-folded bf16 weights (with ln_in) */
    float* ln_out;           /* float2 [M][ln_out_slots] row-moment partials of the stored output, or NULL */
    int32_t ln_in_slots;     /* 1..20 */
    int32_t ln_out_slots;    /* must equal ceil(N / tile_n) of this launch (msd_conv_gemm_ln_slots) */
    float ln_eps;
    /* Shortcut operand (ResBlock, diffusion_model.py:36-38,50: conv2(h) + conv_shortcut(x) as ONE contraction): after the
     * ksize*ksize*(c0+c1) taps of a0|a1, K continues with the channels of a2|a3 read at the OUTPUT pixel (a 1x1 tap);
     * W rows are [taps of a0|a1 ... | channels of a2|a3], K = ksize*ksize*(c0+c1) + c2 + c3.  Needs stride 1, same-size
     * output, c2 % 64 == 0, c3 % 64 == 0.  On the tile / wreg / big forms the shortcut chunks are K tiles behind the last tap
     * (tap-major class); on the halo tiles and the staged-halo big form they follow each split-K slice's main chunks, dealt
     * over the slices in order (chunk-major class; round 6). */
    const void* a2;          /* bf16 [batch][h_out][w_out][c2] or NULL */
    const void* a3;          /* bf16 [batch][h_out][w_out][c3] or NULL (channel concat a2|a3) */
    int32_t c2, c3;
    /* Storage order of w.  0: [N][K] rows.  1: chunk-major [K/64][N][64] — the 64-element K chunk kc of ALL output
     * columns is one contiguous N x 128-byte run, so the weight tile of a K step (any tile_n, any column offset) is a
     * single contiguous block of HBM instead of tile_n pieces of 128 bytes K*2 bytes apart (the packed form the
     * models keep; same values, same K order, same results).  2: fragment-major [K/64][N/16][2][64][8] — the operand
     * registers of v_mfma_f32_16x16x32_bf16 laid out in memory: lane l = 16 g + r of fragment (K tile kt, 16-column block
     * nb, half ks) holds W[16 nb + rho(r)][64 kt + 32 ks + 8 g .. + 8], rho = (0,1,2,3,8,9,10,11,4,5,6,7,12,13,14,15), at
     * byte 16 l of the fragment's contiguous KiB (minsdtf_amd/packing.py fragment_major); read by the wreg form only
     * (tile_m 4000 + rows), which loads a fragment with one coalesced global_load_dwordx4 per wave. */
    int32_t w_layout;
} MsdConvGemm;

/* Number of row-moment partials per row a launch with these parameters writes to `ln_out`
 * (= its number of column tiles), or a negative MSD_E_* code. */
MSD_API int msd_conv_gemm_ln_slots(const MsdConvGemm* p);

MSD_API int msd_conv_gemm(const MsdConvGemm* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_conv_direct — small-channel direct convolution / dense on vector FMAs (fp32 weights).
 * For the layers whose channel counts cannot fill an MFMA tile: UNet conv_in 4->320 and conv_out
 * 320->4 (diffusion_model.py:191,279), VAE post_quant/conv_in/conv_out (image_decoder.py:28-29,53),
 * HintNet (control_net.py:14-30), the time-embedding MLP and the per-ResBlock time projections
 * (diffusion_model.py:30,184-188) evaluated for all steps at once.
 *   w: fp32 Keras layout [ksize][ksize][c_in][c_out];  in: fp32 or bf16 NHWC;  batch index of the
 *   input is (b % in_batch_mod) so one latent can feed the cond and uncond halves.
 * Epilogue: (+bias) -> act(SiLU optional) -> (+residual bf16) -> out as bf16 / fp32 / uint8 where
 * uint8 = clip(trunc(((v+1)*0.5)*255), 0, 255) (stable_diffusion.py:483-486).
 */
#define MSD_OUT_U8 2
typedef struct MsdConvDirect {
    const void* in;
    const float* w;
    const float* bias;     /* or NULL */
    const void* residual;  /* bf16 [M][c_out] or NULL */
    void* out;
    int32_t batch, in_batch_mod, h_in, w_in, c_in;
    int32_t h_out, w_out, c_out;
    int32_t ksize, stride, pad;
    int32_t in_dtype;      /* MSD_OUT_BF16 or MSD_OUT_F32 */
    int32_t out_dtype;     /* MSD_OUT_BF16 / MSD_OUT_F32 / MSD_OUT_U8 */
    int32_t act;           /* MSD_ACT_NONE or MSD_ACT_SILU */
    int32_t act_in;        /* apply SiLU to the input values as they are read (0/1) */
    float in_scale;        /* input multiplier (VAE Rescaling 1/0.18215, image_decoder.py:27) */
} MsdConvDirect;

MSD_API int msd_conv_direct(const MsdConvDirect* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_group_norm — GroupNormalization(groups=32, eps) [+ swish], NHWC, fp32 statistics.
 * Replaces keras GroupNormalization + Activation("swish") (diffusion_model.py:27-28,32-33,57,
 * 277-278; layers.py:32,66-68,78-79; image_decoder.py:51-52) and the Concatenate in front of it
 * (reads x0|x1 through two base pointers, never materialised).
 *   x0: bf16 [batch][hw][c0], x1: bf16 [batch][hw][c1] or NULL;  out: bf16 [batch][hw][c0+c1]
 *   stats:    fp32 [batch][32][2] scratch; receives {mean, rstd} per group
 *   partials: fp32 scratch for per-workgroup partial moments, >= batch * MSD_GN_MAX_CHUNKS * 64
 *             floats is always enough; summed in a fixed order (no atomics: results are
 *             bit-reproducible run to run)
 *   sync:     NULL, or >= batch * MSD_GN_SYNC_WORDS_PER_SAMPLE 32-bit words, 8-byte aligned, ZERO when first used and
 *             written by nothing but msd_group_norm launches of ONE stream at a time (launches that may run concurrently
 *             need a block each).  With it, tensors of >= 2048 pixels per sample whose group slab fits in registers run as
 *             ONE launch in which 2 / 4 / 8 workgroups share each (sample, group) and exchange their partial moments
 *             through this block (ticket counters + {value, epoch} words; the parts are summed in part order:
 *             bit-reproducible).  GIVE-UP FLAG: the exchange poll is bounded (so that an out-of-order dispatch can never hang
 *             the GPU); a workgroup that gives up sets word [8] of its 64-word slot AND word [8] of the block (sync[8]) to 1
 *             and the launch ends with WRONG numbers in that group.  The return code cannot report it (the launch is
 *             asynchronous), so the CALLER must read sync[8] once per job, after the work has completed, and treat a
 *             non-zero word as a failed job (minsdtf_amd/engine.py: check_gn_sync raises HipExtensionError).  Never observed
 *             under in-order dispatch.  Without `sync`: statistics + apply launches, no exchange, no flag.
 *             Samples of >= 9216 pixels (msd_set_option "gn_rows"; 4096 pays from batch 2 per GPU) whose parts fit in registers take the
 *             ROW-MAJOR form of the same exchange: 4-64 parts per SAMPLE (each shared by 1 / 2 / 4 workgroups by channels when the launch
 *             would otherwise leave the chip idle: placement only, msd_set_option "gn_rows_q"), a part = a contiguous pixel range with all its
 *             channels (16-byte accesses), 64 granules per part; it shares the block (second region of every sample's share)
 *             and the give-up word.  (ABI 10: the share grew from 6,144 to 16,384 words for it.)
 *             The per-(sample, group) form deals its workgroups by XCD (an XCD takes the pixel ranges whose rows the conv launches
 *             around it give it; msd_set_option "gn_xmap" 0 = a group's parts on consecutive ids): placement only, the same bits.
 */
#define MSD_GN_SYNC_WORDS_PER_SAMPLE 16384
#define MSD_GN_MAX_CHUNKS 1024
typedef struct MsdGroupNorm {
    const void* x0;
    const void* x1;
    const float* gamma; /* [c0+c1] */
    const float* beta;  /* [c0+c1] */
    float* stats;
    float* partials;
    int64_t partials_floats;
    void* out;
    int32_t batch, hw, c0, c1;
    int32_t silu; /* 0/1 */
    float eps;
    uint32_t* sync;
    int64_t sync_words;
} MsdGroupNorm;

MSD_API int msd_group_norm(const MsdGroupNorm* p, msd_stream_t stream);

/* msd_layer_norm — LayerNormalization(eps) over the last axis (diffusion_model.py:84-88).
 * x, out: bf16 [rows][c], c % 8 == 0, c <= 2048. */
MSD_API int msd_layer_norm(const void* x, const float* gamma, const float* beta, void* out, int32_t rows, int32_t c,
                   float eps, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_attention — fused scaled-dot-product attention, online softmax, MFMA QK^T and PV.
 * Replaces einsum/softmax/einsum of CrossAttention.call (diffusion_model.py:110-127); the
 * (B,heads,S,T) score tensor never exists in HBM.
 *   q:  bf16 [batch][s][q_ld], head h at columns [h*d, (h+1)*d)
 *   k:  bf16 [batch][t][k_ld]
 *   vt: bf16 [batch][heads*d][vt_ld]  (V transposed: key index contiguous; vt_ld % 8 == 0,
 *       vt_ld >= t; columns >= t are padding and are ignored)
 *   out: bf16 [batch][s][o_ld]
 *   softmax(scale * q k^T) v, scale applied to the scores (diffusion_model.py:105,123).
 * head_dim in {40, 80, 160} (UNet) and 64 (CLIP text encoder).  causal != 0 (needs s == t) masks
 * key index > query index, the additive -inf upper triangle of text_encoder.py:75-78.
 */
typedef struct MsdAttention {
    const void* q;
    const void* k;
    const void* vt;
    void* out;
    int32_t batch, heads, head_dim;
    int32_t s, t;
    int32_t q_ld, k_ld, vt_ld, o_ld;
    float scale;
    int32_t causal;
    int32_t q_prescaled; /* != 0: q already carries the factor scale * log2(e) (folded into the weights of the projection that
                            produced it, minsdtf_amd/models.py), so the kernel takes exp2 of q k^T directly; `scale` is then
                            not applied again.  0: softmax(scale * q k^T) as written above. */
    /* ABI 9 - head_dim 512 only (the VAE's single-head AttentionBlock, layers.py:28-59): scratch for a 4-way split of the KEY walk,
     * >= 4 * batch * heads * s * (512 + 2) floats, 16-byte aligned, caller-owned, or NULL.  With it (and t >= 2048, t % 128 == 0) every
     * query tile is served by four workgroups that each walk a quarter of the keys and a merge launch adds their partial results in
     * part order (the one head at 512x512 is otherwise 64 workgroups on a 256-CU chip).  Whether the split runs depends on t and on
     * this pointer only, never on the batch; results with and without it differ in rounding. */
    float* workspace;
    int64_t workspace_floats;
} MsdAttention;

MSD_API int msd_attention(const MsdAttention* p, msd_stream_t stream);

/* msd_cross_attention_q — cross-attention over a short context with its query projection inside: the `attn2.to_q` Dense
 * (with the LayerNormalization in front of it folded in, as MsdConvGemm.ln_in does) and the attention over the text
 * context (diffusion_model.py:102-127, context = 77 tokens) as ONE launch instead of two latency-bound ones.
 *   q = LN(x) Wq^T computed per (64 queries, head) as rstd * (x wq^T - mean * ln_colsum) + bias, rounded to bf16;
 *   out = softmax(q k^T) v with the softmax as exp2 of the raw product: wq MUST carry scale * log2(e) (q_prescaled form).
 * x: bf16 [batch*s][c] (the block's raw rows), ln_in: float2 [batch*s][ln_in_slots] (the producer's ln_out partials),
 * wq: bf16 gamma-folded weights [c][c] in `w_layout`, ln_colsum / bias: [c]; k: bf16 [batch][t][k_ld], vt: bf16
 * [batch][heads][head_dim][vt_ld] (key contiguous), out: bf16 [batch*s][o_ld].  heads = 8, head_dim 40, 80 or 160, t <= 96
 * (160: the head's 400 KB of weights are streamed through a four-stage LDS ring instead of waiting in LDS). */
typedef struct MsdCrossAttnQ {
    const void* x;
    const float* ln_in;
    const void* wq;
    const float* ln_colsum;
    const float* bias;       /* [c] or NULL */
    const void* k;
    const void* vt;
    void* out;
    int32_t batch, heads, head_dim, s, t;
    int32_t k_ld, vt_ld, o_ld;
    int32_t ln_in_slots;
    float ln_eps;
    int32_t w_layout;        /* 0: [c][c] rows, 1: chunk-major [c/64][c][64] (MsdConvGemm.w_layout) */
} MsdCrossAttnQ;

MSD_API int msd_cross_attention_q(const MsdCrossAttnQ* p, msd_stream_t stream);

/* msd_softmax_rows — out[r, :cols] = softmax(scale * x[r, :cols]); x fp32 [rows][ld_in], out bf16
 * [rows][ld_out] (VAE single-head attention, layers.py:48-50). cols % 8 == 0. */
MSD_API int msd_softmax_rows(const float* x, void* out, int64_t rows, int32_t cols, int32_t ld_in, int32_t ld_out, float scale,
                     msd_stream_t stream);

/* msd_embedding_sum — out[r, :] = bf16(tok_table[tokens[r], :] + pos_table[positions[r], :]).
 * Replaces CLIPEmbedding.call (text_encoder.py:22-33): two Embedding lookups and their sum.
 * tables fp32 [vocab][dim] / [max_len][dim], tokens / positions int32 [rows], dim % 4 == 0; ids outside
 * their table are an argument error reported through `status` (device int32, set to 1; may be NULL). */
MSD_API int msd_embedding_sum(const int32_t* tokens, const int32_t* positions, const float* tok_table, const float* pos_table,
                      void* out, int32_t rows, int32_t dim, int32_t vocab, int32_t max_len, int32_t* status,
                      msd_stream_t stream);

/* msd_replicate (ABI 11) — dst = `copies` replicas of the `bytes` bytes at src, back to back (bytes % 16 == 0; src == dst: replica 0
 * stays where it is; any other overlap: MSD_E_ARG).  The classifier-free-guidance pair of one step (stable_diffusion.py:454-457: the
 * unconditional and the conditioned call get the SAME latent and time embedding) is identical up to the first cross-attention
 * (diffusion_model.py:191-196: conv_in, down_blocks.0.resnets.0, and norm / proj_in / attn1 of down_blocks.0.attentions.0); the fused
 * batch computes that prefix once per image and replicates three tensors (engine.SHARE_CFG_PREFIX). */
MSD_API int msd_replicate(const void* src, void* dst, int64_t bytes, int32_t copies, msd_stream_t stream);

/* msd_memset_zero — stream-ordered hipMemsetAsync(ptr, 0, bytes) (GroupNorm statistic slots). */
MSD_API int msd_memset_zero(void* ptr, int64_t bytes, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_cfg_step — classifier-free guidance + guidance rescale + sampler step, fp32, one launch.
 * Replaces stable_diffusion.py:458-461 (CFG, rescale_noise_cfg :304-315) and Scheduler.step
 * non-TCD branch (scheduler.py:272-285,308-312).
 *   eps:    fp32 [2*batch][n]  rows [0,batch) = unconditional, [batch,2*batch) = text-conditioned
 *           (guidance <= 0: fp32 [batch][n], used as is — stable_diffusion.py:462-467)
 *   latent: fp32 [batch][n], updated in place
 *   coef:   fp32 [steps][4] = {signal_rate[t], noise_rate[t], A, B}: x0 = (x - noise_rate eps) / signal_rate,
 *           x' = A x0 + B eps.  Deterministic sampler: A, B = signal / noise rate of t_prev and {1, 0} on
 *           the last step (x' = x0).  TCD sampler (scheduler.py:286-307): the gamma-sampling coefficients,
 *           plus x' += noise_coef[step] * step_noise[step][b][:] when step_noise != NULL
 *           (step_noise fp32 [steps][batch][n] = the per-step N(0,1) draws, noise_coef fp32 [steps]).
 *   The row used is coef[*step_ptr]; after the update *step_ptr is incremented when advance != 0:
 *   advance = 1 by a second one-thread launch; advance = 2 inside the launch, by the workgroup that finishes last — then
 *   step_ptr points at TWO ints {step, ticket}, ticket zero when first used and touched by nothing else.
 *   step_ptr == NULL (advance 0 only) uses row 0.  A counter outside 0 .. steps - 1 is clamped into that range for the
 *   coefficient row, noise_coef and the step_noise row, but what advance stores is the counter AS READ plus one (-3 -> -2,
 *   steps + 2 -> steps + 3): a counter that left the range stays outside it until the caller resets it.
 *   Inpainting (stable_diffusion.py:469-475), when inpaint_mask != NULL: after the sampler step
 *   latent = origin * (1 - mask) + latent * mask with origin = signal_rate[t] * inpaint_init +
 *   noise_rate[t] * inpaint_noise at the CURRENT timestep t (the reference re-noises the encoded
 *   image at t, not t_prev).  inpaint_init fp32 [n] (one image, shared by the batch), inpaint_noise
 *   fp32 [batch][n], inpaint_mask fp32 [n] (the latent-resolution mask repeated over the channels).
 */
typedef struct MsdCfgStep {
    const float* eps;
    float* latent;
    const float* coef;
    int32_t* step_ptr;
    int32_t batch, n, num_steps;
    float guidance, guidance_rescale;
    int32_t advance;
    const float* inpaint_init;
    const float* inpaint_noise;
    const float* inpaint_mask;
    const float* step_noise;
    const float* noise_coef;
} MsdCfgStep;

MSD_API int msd_cfg_step(const MsdCfgStep* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_sampler_step (ABI 12) — classifier-free guidance + guidance rescale + a multistep / ancestral sampler step, fp32, one
 * launch: msd_cfg_step's guidance, rescale, step counter (advance 0 / 1 / 2) and inpaint blend, with a general linear update
 * that carries the previous evaluation's denoised estimate (minsdtf_amd/samplers.py: DPM++ 2M, DPM++ 2M SDE, Euler ancestral).
 *   eps, latent, step_ptr, batch, n, num_steps, guidance, guidance_rescale, advance, inpaint_*: as msd_cfg_step.
 *   coef:          fp32 [steps][8] = {alpha_i, sigma_i, c_x, c_D, c_P, c_z, 0, 0}:  e = CFG(+rescale) of eps,
 *                  D = (x - sigma_i e) / alpha_i,  x' = c_x x + c_D D + c_P P + c_z z,  then P = D.
 *                  The inpaint blend (inpaint_mask != NULL) re-noises inpaint_init with the row's alpha_i / sigma_i.
 *   denoised_prev: fp32 [batch][n] = P, required: read only where the row's c_P != 0 (the first executed row has c_P = 0, so
 *                  the buffer needs no initial value), written with D on every step.
 *   step_noise:    fp32 [steps][batch][n] = the per-step N(0,1) draws z, or NULL (then c_z is ignored).
 * Argument errors (a NULL eps / latent / coef / denoised_prev, bad dims, advance outside 0..2 or without step_ptr, an
 * inpaint_mask without inpaint_init / inpaint_noise) return MSD_E_ARG without launching.
 */
typedef struct MsdSamplerStep {
    const float* eps;
    float* latent;
    const float* coef;
    int32_t* step_ptr;
    int32_t batch, n, num_steps;
    float guidance, guidance_rescale;
    int32_t advance;
    const float* inpaint_init;
    const float* inpaint_noise;
    const float* inpaint_mask;
    const float* step_noise;
    float* denoised_prev;
} MsdSamplerStep;

MSD_API int msd_sampler_step(const MsdSamplerStep* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_lora_merge — LoRA switch at run time: rewrites packed weight matrices IN PLACE (same tensors, same layouts), so launch
 * plans and captured graphs that hold their addresses stay valid (minsdtf_amd/lora.py; DESIGN.md "LoRA switch").  One launch
 * over `num_jobs` job descriptors; per job, for every logical element (n, k) of an N x K matrix:
 *   v   = master[n][k] + sum_j up[n][j] * down[j][k]      fp32, j = 0 .. rank-1 in order, fused multiply-add; rank 0: v = master
 *   v   = (v * rowscale[n]) * colscale[k]               each factor optional (NULL), in this order, no contraction
 *   out = bf16 (round to nearest even) or fp32 of v
 * stored at destination row r = (rowmap ? rowmap[n] : n) + row_off and column c = col_off + k of an out_rows x out_cols matrix:
 *   layout 0: rows, out[r * ld + c];  1: chunk-major [out_cols/64][out_rows][64] (bf16 only);
 *   layout 2: transposed rows out[c * out_rows + r] (fp32 only: the direct-conv form of a Dense);
 * and, when out_frag != NULL, into the fragment-major copy of the same bf16 matrix (MsdConvGemm.w_layout = 2, packing.fragment_major;
 * out_rows % 16 == 0, out_cols % 64 == 0); when colsum != NULL (bf16, the job spans whole destination rows) colsum[r] = fp32 of the
 * fp64 sum of the row's ROUNDED values (the .lncs vector of a LayerNorm fold).  Rows whose destination row r falls outside
 * [0, out_rows) are not written: neither their elements of out and out_frag nor colsum[r].  A job writes nothing else: the other
 * rows and columns of the destination, the gap columns of a wide ld and every input keep their bits.  master, down and colscale may
 * start on any 4-byte boundary and master_ld, k, ld, col_off need not be multiples of 4 or 8 (the vector forms are taken only where
 * they apply; the result is the same).  Deterministic: every element and every row sum has one fixed evaluation order.
 * `jobs` is the host array (validated here: argument errors return MSD_E_ARG before anything is launched); `jobs_dev` is a device
 * copy of the same entries, which the kernel reads.  first_block = sum over the earlier jobs of ceil(n / 8).  rank <= 512.
 */
typedef struct MsdLoraJob {
    const float* master;     /* [n][master_ld] fp32 */
    const float* up;         /* [n][rank] fp32 (NULL when rank == 0) */
    const float* down;       /* [rank][k] fp32 (NULL when rank == 0) */
    const float* rowscale;   /* [n] or NULL */
    const float* colscale;   /* [k] or NULL */
    const int32_t* rowmap;   /* [n] or NULL */
    void* out;
    void* out_frag;          /* bf16 fragment-major copy, or NULL */
    float* colsum;           /* [out_rows] fp32, or NULL */
    int32_t n, k, rank, master_ld;
    int32_t layout, out_dtype, ld;
    int32_t out_rows, out_cols, row_off, col_off;
    int32_t first_block;
} MsdLoraJob;

typedef struct MsdLoraMerge {
    const MsdLoraJob* jobs;      /* host array */
    const MsdLoraJob* jobs_dev;  /* device copy */
    int32_t num_jobs;
} MsdLoraMerge;

MSD_API int msd_lora_merge(const MsdLoraMerge* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_latent_resample — separable resampling of the fp32 NHWC latent (C = 4) fused with a re-noise: the hand-off between the
 * two passes of a hires job (minsdtf_amd/hires.py).  An addition to ABI 12: nothing else changed.
 *
 *   out[b,y,x,:] = a * sum_j wy[y].w[j] * ( sum_i wx[x].w[i] * in[b, wy[y].idx[j], wx[x].idx[i], :] ) + s * noise[b,y,x,:]
 *
 *   in:    fp32 [batch][h_in][w_in][4];   out: fp32 [batch][h_out][w_out][4] (must not overlap in)
 *   noise: fp32 [batch][h_out][w_out][4], or NULL: the term is skipped and `s` is ignored
 *   wx:    MsdResampleRow [w_out], wy: MsdResampleRow [h_out] — one row of four taps per output coordinate of the axis, computed
 *          by the host in float64 and stored as fp32 (hires.taps / hires.pack_rows: the semantics of torch's interpolate with
 *          align_corners = False for nearest / nearest-exact / bilinear / bicubic).  Indices are already clamped to the source
 *          (replicate border, clamped per tap); unused taps have weight 0 and any valid index.  (The kernel clamps every index to
 *          the source once more, so a bad table reads the wrong pixel, never outside `in`.)
 * Order of the sums (pinned; every product and sum is fp32, FMAs are single-rounded):
 *   r_j = wx.w[0] * p_j0;  r_j = fma(wx.w[i], p_ji, r_j) for i = 1, 2, 3        (p_ji = the source pixel of taps j, i)
 *   v   = wy.w[0] * r_0;   v   = fma(wy.w[j], r_j, v)    for j = 1, 2, 3
 *   out = a * v  without noise;  out = fma(s, noise, a * v)  with it
 * per channel.  One output pixel is one lane's float4; a sample's bits do not depend on the batch it runs in.
 * All five pointers 16-byte aligned; batch in 1 .. 65535 (one grid row per sample), sizes in 1 .. 16384 with
 * h_out >= h_in, w_out >= w_in, fewer than 2^31 output elements.
 * Argument errors (a NULL struct / in / out / wx / wy, bad sizes, a misaligned pointer, out overlapping in) return
 * MSD_E_ARG without launching.  Nothing is allocated; the launch is stream-ordered and capturable. */
typedef struct MsdResampleRow {
    int32_t idx[4];
    float w[4];
} MsdResampleRow;

typedef struct MsdLatentResample {
    const float* in;
    float* out;
    const float* noise;          /* or NULL */
    const MsdResampleRow* wx;    /* [w_out] */
    const MsdResampleRow* wy;    /* [h_out] */
    int32_t batch, h_in, w_in, h_out, w_out;
    float a, s;
} MsdLatentResample;

MSD_API int msd_latent_resample(const MsdLatentResample* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_tile_consensus — the per-step hand-off of a tiled-diffusion job (MultiDiffusion; minsdtf_amd/tiled.py): the
 * views of a canvas are batch rows of the denoise engine's latent, and after every sampler step each canvas pixel - and every
 * view's entry for it - becomes the weighted mean of the stepped views that cover it.  An addition to ABI 12: nothing else changed.
 *
 *   tiles:  fp32 [batch * rows * cols][th][tw][4], row b * (rows * cols) + r * cols + c (sample-major, views row-major); view
 *           (r, c) covers canvas rows ys[r] .. ys[r] + th - 1 and columns xs[c] .. xs[c] + tw - 1.  Read and rewritten in place.
 *   canvas: fp32 [batch][H][W][4] (must not overlap tiles)
 *   wy:     fp32 [th], wx: fp32 [tw] - separable blend weights, > 0, computed by the host in float64 (tiled.weight_row)
 *
 * mode 0 (consensus), per canvas pixel (Y, X) of a sample, per channel, over the covering views in ascending (r, c) order:
 *   one cover:   out = x_v                                       (copied bit for bit)
 *   otherwise:   w_v  = wy[Y - ys[r]] * wx[X - xs[c]]            (fp32, rounded once)
 *                acc  = fma(w_v, x_v, acc),  wsum = wsum + w_v   (both from 0, fp32, the FMA single-rounded)
 *                out  = acc / wsum                               (one IEEE division)
 *   canvas[Y, X] = out, and every covering view's entry = out.
 * mode 1 (gather): every covering view's entry = canvas[Y, X] (plain copies; the canvas is only read).
 *
 * One canvas pixel of one sample is one lane's float4.  Each tile entry belongs to exactly one canvas pixel, so the in-place
 * update is free of races and needs no atomics; nothing couples two pixels, so a sample's bits do not depend on its batch.
 * The offsets travel by value (in the kernel arguments: a captured graph holds them).  Checked on the host, without a device:
 * tiles / canvas / wy / wx non-NULL and 16-byte aligned; batch in 1 .. 65535, th, tw >= 1, H >= th, W >= tw; rows, cols in
 * 1 .. MSD_TILE_MAX_VIEWS; per axis the offsets start at 0, end at L - t and ascend strictly in steps of at most t (every canvas
 * pixel is covered); tiles and canvas do not overlap; fewer than 2^31 elements in each; mode 0 or 1.  Argument errors return
 * MSD_E_ARG without launching.  Nothing is allocated; the launch is stream-ordered and capturable. */
#define MSD_TILE_MAX_VIEWS 64

typedef struct MsdTileConsensus {
    float* tiles;
    float* canvas;
    int32_t ys[MSD_TILE_MAX_VIEWS];   /* [rows] used */
    int32_t xs[MSD_TILE_MAX_VIEWS];   /* [cols] used */
    int32_t rows, cols, th, tw, H, W, batch;
    const float* wy;             /* [th] */
    const float* wx;             /* [tw] */
    int32_t mode;                /* 0: consensus, 1: gather */
} MsdTileConsensus;

MSD_API int msd_tile_consensus(const MsdTileConsensus* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_region_combine — the per-step combine of a regional-prompting job (Latent Couple / MultiDiffusion region control;
 * minsdtf_amd/regions.py): the UNet's conditional rows are evaluated once per region prompt, and in front of the
 * guidance / sampler step every latent pixel's conditional eps becomes the weighted sum of the regions' predictions for it.
 * An addition to ABI 12: nothing else changed.
 *
 *   eps: fp32 [regions * batch][n], row r * batch + b (region-major, like the pass's context rows); n = h * w * 4 (NHWC, C = 4)
 *   w:   fp32 [regions][n / 4] - the weight of region r at each pixel, shared by the batch and by the 4 channels; >= 0 and
 *        normalised by the host (regions.weights: weight_r * mask_r / sum in float64, rounded once) - the kernel does not divide
 *   out: fp32 [batch][n]; may be eps itself (region 0's rows are then rewritten in place)
 *
 * Per sample b, pixel p and channel c, over r = 0 .. regions - 1 in this order (pinned; all fp32, the FMA single-rounded):
 *   v = w[0][p] * eps[0 * batch + b][p, c]
 *   v = fma(w[r][p], eps[r * batch + b][p, c], v)        r = 1 .. regions - 1
 *   out[b][p, c] = v
 * Where one region's weight is exactly 1.0 and every other one exactly 0.0, a finite non-zero value of that region is copied
 * bit for bit (a zero may change sign).  A region of weight 0 still takes part in the sum: its NaN / Inf reach the output.
 *
 * One pixel of one sample is one lane's float4, one grid row per sample.  An output element reads only its own position of each
 * region's row, so the in-place form is free of races and needs no atomics; nothing couples two pixels or two samples, so a
 * sample's bits do not depend on its batch.  Checked on the host, without a device: eps / w / out non-NULL and 16-byte aligned;
 * n a positive multiple of 4; regions in 1 .. MSD_REGION_MAX; batch in 1 .. 65535 (one grid row per sample); fewer than 2^31
 * elements in eps; out == eps or out apart from all of eps; w apart from both.  Argument errors return MSD_E_ARG without
 * launching.  Nothing is allocated; the launch is stream-ordered and capturable. */
#define MSD_REGION_MAX 16

typedef struct MsdRegionCombine {
    const float* eps;
    const float* w;
    float* out;
    int32_t regions, batch, n;
} MsdRegionCombine;

MSD_API int msd_region_combine(const MsdRegionCombine* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_attention_identity — self-attention with the IDENTITY attention map: the perturbed forward of perturbed-attention
 * guidance (PAG, Ahn et al. 2024; minsdtf_amd/pag.py).  Where msd_attention computes softmax(q k^T) v, the
 * perturbed layer's output is v itself; the step plan holds v only transposed, as msd_attention's `vt` operand, so this is
 * the transpose back, recorded for the perturbed batch rows in place of (or next to) the msd_attention launch, with the same
 * operands.  An addition to ABI 12: nothing else changed.
 *
 *   vt:  bf16 [batch][channels][vt_ld], key index contiguous (all heads: channels = heads * head_dim); vt_ld % 8 == 0,
 *        vt_ld >= s; columns >= s are padding, whatever they hold (NaN included) does not reach out
 *   out: bf16 [batch][s][o_ld]; out[b][k][c] = vt[b][c][k] for k < s, c < channels, bit for bit; columns >= channels of a
 *        row (o_ld > channels) are not written
 *
 * A tiled transpose through LDS, 16-byte global loads along vt_ld and 16-byte global stores along channels; one workgroup
 * per 64 x 64 tile per sample.  Checked on the host, without a device: vt / out non-NULL and 16-byte aligned; batch in
 * 1 .. 65535; s >= 1; channels a positive multiple of 8; vt_ld % 8 == 0 and vt_ld >= s; o_ld >= channels and o_ld % 8 == 0
 * (every row of out 16-byte aligned); fewer than 2^31 elements in vt and in out; the bytes of out apart from the bytes of vt.
 * Argument errors return MSD_E_ARG without launching.  Nothing is allocated; the launch is stream-ordered and capturable. */
typedef struct MsdAttentionIdentity {
    const void* vt;
    void* out;
    int32_t batch, channels, s;
    int32_t vt_ld, o_ld;
} MsdAttentionIdentity;

MSD_API int msd_attention_identity(const MsdAttentionIdentity* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_region_attention — regional prompting inside cross-attention ("attention couple"; minsdtf_amd/regions.py; DESIGN.md
 * §4.10): the conditional rows of an attn2 layer attend to every region's text context and mix the results per query, so the
 * UNet runs the plain job's rows whatever the number of regions.  An addition to ABI 12: nothing else changed.
 *
 *   q:   bf16 [batch][s][q_ld], head h at columns [h * d, (h + 1) * d), d = head_dim; q MUST carry scale * log2(e) (the
 *        q_prescaled form of msd_attention, as msd_cross_attention_q requires of its weights); q_ld >= heads * d
 *   k:   bf16 [regions * batch][t][k_ld], row r * batch + b (region-major, like msd_region_combine); k_ld >= heads * d
 *   vt:  bf16 [regions * batch][heads * d][vt_ld], key index contiguous; vt_ld % 8 == 0, vt_ld >= t; columns >= t are
 *        padding, whatever they hold (NaN included) never reaches out
 *   w:   fp32 [regions][w_ld]; w[r][i] = the weight of region r at query i, i < s; >= 0 and normalised by the host
 *        (regions.Resolved.level_weights), shared by the batch and the heads - the kernel does not divide by their sum
 *   out: bf16 [batch][s][o_ld]; columns >= heads * d of a row are not written
 *
 * head_dim is 40, 80 or 160; 1 <= t <= 96 (all keys are one tile); 1 <= regions <= MSD_REGION_MAX.
 *
 * Per sample, head, query i and channel c, the regions in ascending order (pinned; fp32):
 *   m_r = max_key q.k_r[key]        P_r[key] = bf16(exp2(q.k_r[key] - m_r))        l_r = sum_key P_r[key]
 *   O_r = (sum_key P_r[key] * v_r[key][c]) * (1 / l_r)
 *   acc = w[r][i] * O_r                      at the first region with w[r][i] > 0
 *   acc = fma(w[r][i], O_r, acc)             at each later region with w[r][i] > 0
 *   out = bf16(acc)                          (0 where no region is positive)
 * A region whose weight at a query is exactly 0 is NOT accumulated for that query: acc keeps its bits.  So a query that one
 * region covers alone (weight exactly 1.0, the others 0.0) gets that region's attention bit for bit - what a launch with that
 * region alone and w = 1 writes - and the K / V^T of a region that is nowhere positive may hold anything, NaN included.  A
 * workgroup (64 queries of one sample and head) skips a region whose weights are 0 at all of its queries without reading its
 * K / V^T; by the rule above that changes no bit.
 *
 * Both products run on MFMAs with K / V^T staged in LDS per region; plain vector loads and stores, no atomics; nothing couples
 * two samples, so a sample's bits do not depend on its batch.  Checked on the host, without a device: q / k / vt / w / out
 * non-NULL and 16-byte aligned; head_dim, t and regions in range; batch and heads in 1 .. 65535; s >= 1; w_ld >= s; q_ld, k_ld,
 * vt_ld and o_ld multiples of 8; q_ld, k_ld, o_ld >= heads * head_dim; vt_ld >= t; fewer than 2^31 workgroups; the extent of
 * out apart from the extent of every input.  Argument errors return MSD_E_ARG without launching.  Nothing is allocated; the
 * launch is stream-ordered and capturable. */
typedef struct MsdRegionAttention {
    const void* q;
    const void* k;
    const void* vt;
    const float* w;
    void* out;
    int32_t batch, heads, head_dim, s, t, regions;
    int32_t q_ld, k_ld, vt_ld, w_ld, o_ld;
} MsdRegionAttention;

MSD_API int msd_region_attention(const MsdRegionAttention* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_attention_joint — self-attention over the row's own keys AND the keys of one shared reference row: "reference-only"
 * control (minsdtf_amd/reference.py).  softmax(own ‖ ref) is not a sum of two softmaxes, so this is one flash
 * kernel that walks two key segments; the blend with the plain self-attention (diffusers' style_fidelity) is the online
 * softmax's state at the segment boundary, kept for later.  An addition to ABI 12: nothing else changed.
 *
 *   q:      bf16 [batch][s][q_ld], head h at columns [h * d, (h + 1) * d), d = head_dim; q MUST carry scale * log2(e) (the
 *           q_prescaled form of msd_attention); q_ld >= heads * d
 *   k:      bf16 [batch][t][k_ld]                the row's own keys; k_ld >= heads * d
 *   vt:     bf16 [batch][heads * d][vt_ld]       its own V^T, key index contiguous; columns >= t are padding
 *   k_ref:  bf16 [t_ref][k_ld]                   ONE row, shared by the batch (same leading dimension as k)
 *   vt_ref: bf16 [heads * d][vt_ld]              columns >= t_ref are padding
 *   mix:    fp32 [batch] in [0, 1], or NULL = all 0: the share of the plain self-attention in the sample's output
 *   out:    bf16 [batch][s][o_ld]; columns >= heads * d of a row are not written
 *
 * head_dim is 40, 80 or 160; s, t, t_ref >= 1; vt_ld % 8 == 0 and vt_ld >= max(t, t_ref).  Padding columns of vt / vt_ref,
 * whatever they hold (NaN included), never reach out.
 *
 * Per sample b, head, query and channel (pinned; fp32).  The own keys are walked in ascending tiles of 64 keys, then the
 * reference keys the same way; a segment's last tile may be partial, the own segment's too (in the middle of the walk).  With
 * the state m = -1e30, l = 0, O = 0, every tile does
 *   m' = max(m, max_key score[key])      a = exp2(m - m')      l = l * a      O = O * a      m = m'
 *   P[key] = bf16(exp2(score[key] - m))  l += sum_key P[key]   O += sum_key P[key] * v[key][c]
 * (P rounded to bf16 is both the operand of the second product and what the row sum adds; the rescale is applied at every
 * tile, never deferred).  Then
 *   after the last own tile:        plain = O * (1 / l)
 *   after the last reference tile:  joint = O * (1 / l)
 *   f = mix[b] (0 when mix is NULL):
 *     f == 0:     out = bf16(joint)                                    the bits of a launch with mix = NULL
 *     f == 1:     out = bf16(plain)                                    the reference segment is NOT read for that sample:
 *                                                                      k_ref / vt_ref may hold anything, NaN included
 *     otherwise:  out = bf16(fma(f, plain, (1.0f - f) * joint))
 * plain depends on the own segment alone: nothing the reference keys do to the running maximum afterwards moves it.  A
 * workgroup is 64 queries of one sample and head, so the branch on f is uniform over it.
 *
 * Both products run on MFMAs with K / V^T tiles staged in LDS; plain vector loads and stores, no atomics, no scratch buffer;
 * nothing couples two samples, so a sample's bits do not depend on its batch.  Checked on the host, without a device: q / k /
 * vt / k_ref / vt_ref / out non-NULL and 16-byte aligned; mix NULL or 16-byte aligned (its values are not checked); head_dim in
 * range; batch and heads in 1 .. 65535; s, t, t_ref >= 1; q_ld, k_ld, vt_ld and o_ld multiples of 8; q_ld, k_ld, o_ld >= heads *
 * head_dim; vt_ld >= max(t, t_ref); fewer than 2^31 workgroups; the extent of out apart from the extent of every input.
 * Argument errors return MSD_E_ARG without launching.  Nothing is allocated; the launch is stream-ordered and capturable. */
typedef struct MsdAttentionJoint {
    const void* q;
    const void* k;
    const void* vt;
    const void* k_ref;
    const void* vt_ref;
    const float* mix;
    void* out;
    int32_t batch, heads, head_dim, s, t, t_ref;
    int32_t q_ld, k_ld, vt_ld, o_ld;
} MsdAttentionJoint;

MSD_API int msd_attention_joint(const MsdAttentionJoint* p, msd_stream_t stream);

/* msd_reference_latent — the reference row's UNet input of the current step (reference-only control):
 *   out[i] = fma(coef[step][1], noise[i], coef[step][0] * z[i])          fp32, i < n, on float4s
 * z / noise / out: fp32 [n], 16-byte aligned, pairwise distinct; n a positive multiple of 4.  coef: fp32 [num_steps][2], the
 * signal and noise rate at which each step's UNet evaluation sees its latent (reference.rates).  step = *step_ptr (0 when
 * step_ptr is NULL), clamped to 0 .. num_steps - 1 like msd_cfg_step's.  Argument errors return MSD_E_ARG without launching;
 * nothing is allocated; the launch is stream-ordered and capturable. */
typedef struct MsdReferenceLatent {
    const float* z;
    const float* noise;
    const float* coef;
    const int32_t* step_ptr;
    float* out;
    int32_t n, num_steps;
} MsdReferenceLatent;

MSD_API int msd_reference_latent(const MsdReferenceLatent* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_reference_adain — reference AdaIN of a reference-only job (minsdtf_amd/reference.py): every generated
 * row's feature map is renormalised, channel by channel, to the mean and standard deviation that the reference row has at the
 * same place, in place.  An addition to ABI 12: nothing else changed.
 *
 *   x:    bf16 [rows][hw][c], dense; rewritten in place
 *   ref:  bf16 [hw][c]: the reference row; never written; may not overlap x[0 .. rows) (directly behind it is fine)
 *   mix:  fp32 [rows] or NULL = all 0: the share of the row's own values in its result
 *   rows in 1 .. 65535, hw >= 1, c a positive multiple of 8, hw * c < 2^31, eps finite and positive (1e-6 from the engine)
 *
 * Per row b and channel c (pinned; every operation a single-rounded fp32 one), with n = hw and inv_n = fp32(1) / fp32(n):
 *   mean = (sum_p x[b][p][c]) * inv_n                 first the mean,
 *   var  = (sum_p fma(d, d, .)) * inv_n, d = x - mean  then the squared deviations from THAT mean (never E[x^2] - mean^2)
 *   std  = sqrt(max(var, 0) + eps)                    (correctly rounded sqrt)
 *   mean_r, std_r likewise from ref
 *   f = mix[b] (0 when mix is NULL), g = 1 - f, s = std_r / std (correctly rounded division)
 *   A = fma(g, s, f)      Bc = g * fma(-mean, s, mean_r)      out = bf16(fma(x, A, Bc))
 * which is out = f x + (1 - f) ((x - mean) s + mean_r).  Both sums run in the same order for x and for ref: a lane adds the
 * pixels p0, p0 + L, p0 + 2 L, ... (p0 < L; L = 32 pixel lanes up to hw = 1024, 128 above) in ascending order, the eight lanes of
 * a wave that share a channel by three cross-lane adds, the waves in ascending order ((w0 + w1) + w2) + ... - an order that
 * depends on hw alone, so a row that is a copy of the reference gets s = 1 and Bc = 0 exactly and comes back bit for bit.  A row with f == 1 is neither read nor written (it may hold NaN); a
 * workgroup is one row and 64 adjacent channels, so that branch is uniform over it.  A row's bits depend on its own data, the
 * reference row and its own mix entry: not on rows, the grid or the other rows of the launch.  Up to hw = 1024 the row's and
 * the reference's slab stay in registers between the passes; above that they are read again.
 *
 * Plain 16-byte vector loads and stores, no atomics, no scratch, no workspace.  Checked on the host, without a device: x / ref
 * non-NULL; x / ref / mix 16-byte aligned; rows, hw, c, eps as above; ref and mix apart from x[0 .. rows).  Argument errors
 * return MSD_E_ARG without launching.  Nothing is allocated; the launch is stream-ordered and capturable. */
typedef struct MsdReferenceAdain {
    void* x;
    const void* ref;
    const float* mix;
    int32_t rows, hw, c;
    float eps;
} MsdReferenceAdain;

MSD_API int msd_reference_adain(const MsdReferenceAdain* p, msd_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * msd_attention_windowed — HyperTile: self-attention inside non-overlapping rectangular windows of the h x w feature map
 * (minsdtf_amd/hypertile.py).  The operands are those of msd_attention in its q_prescaled form, over the whole
 * image, where the q|k|v GEMM wrote them: nothing is gathered.  An addition to ABI 12: nothing else changed.
 *
 *   q:   bf16 [batch][s][q_ld], s = h * w, head hd at columns [hd * d, (hd + 1) * d), d = head_dim; q MUST carry
 *        scale * log2(e); q_ld >= heads * d
 *   k:   bf16 [batch][s][k_ld]; k_ld >= heads * d
 *   vt:  bf16 [batch][heads * d][vt_ld], key (token) index contiguous; vt_ld >= s; columns >= s are padding
 *   out: bf16 [batch][s][o_ld]; columns >= heads * d of a row are not written
 *
 * Geometry: h % wh == 0, w % ww == 0, ww % 8 == 0; head_dim is 40, 80 or 160.  Token (y, x) (row y * w + x) belongs to window
 * (y / wh, x / ww); inside a window queries and keys are numbered row-major, j -> (j / ww, j % ww), j < wh * ww.  Per sample,
 * head and window
 *   out = softmax(q k^T) v        over that window's wh * ww keys only
 * in msd_attention_joint's pinned arithmetic with one key segment: the window's keys in ascending window-linear tiles of 64
 * (the last tile partial when wh * ww % 64 != 0: its missing keys are staged as zeros and their scores masked); state m = -1e30,
 * l = 0, O = 0; per tile m' = max(m, max score), a = exp2(m - m'), l = l * a, O = O * a, P = bf16(exp2(score - m')),
 * l += sum P, O += sum P * v; out = bf16(O * (1 / l)).  A workgroup is 64 window-linear queries of one (sample, head, window).
 *
 * Pinned properties (tests/test_hypertile_gpu.py):
 *   - The arithmetic of a window depends only on that window's tokens in window-linear order: a launch on the image gives, for
 *     every window, bit for bit what a launch with h = wh, w = ww on that window's gathered tokens gives.
 *   - Nothing outside a window is addressed for it: what other windows hold in q / k / vt, NaN included, never reaches a
 *     window's output, and columns >= s of vt never reach any output.
 *   - Nothing couples two samples: a sample's bits do not depend on its batch, and runs repeat.
 *
 * Both products run on MFMAs with K / V^T tiles staged in LDS; plain vector loads and stores, no atomics, no scratch buffer.
 * Checked on the host, without a device: q / k / vt / out non-NULL and 16-byte aligned; head_dim in range; h, w, wh, ww >= 1
 * with the three divisibilities above; batch and heads in 1 .. 65535; q_ld, k_ld, vt_ld and o_ld multiples of 8; q_ld, k_ld,
 * o_ld >= heads * head_dim; vt_ld >= s; fewer than 2^31 workgroups; the extent of out apart from the extent of every input.
 * Argument errors return MSD_E_ARG without launching.  Nothing is allocated; the launch is stream-ordered and capturable. */
typedef struct MsdAttentionWindowed {
    const void* q;
    const void* k;
    const void* vt;
    void* out;
    int32_t batch, heads, head_dim;
    int32_t h, w, wh, ww;
    int32_t q_ld, k_ld, vt_ld, o_ld;
} MsdAttentionWindowed;

MSD_API int msd_attention_windowed(const MsdAttentionWindowed* p, msd_stream_t stream);

/* msd_add_bf16 — out = a + b elementwise on bf16. n % 8 == 0. */
MSD_API int msd_add_bf16(const void* a, const void* b, void* out, int64_t n, msd_stream_t stream);
/* msd_add_f32_bf16 — out = bf16(a + b), a / out bf16, b fp32, summed in fp32 (may run in place, out == a).  The ControlNet
 * residual adds of diffusion_model.py:230-234 when the 13 residuals arrive over the model boundary as fp32 arrays
 * (DiffusionModel.predict_on_batch); the fused device loop has no such launch: there the adds are the epilogue residual of
 * the ControlNet's own 1x1 "zero" convs (msd_conv_gemm with residual == out). n % 8 == 0. */
MSD_API int msd_add_f32_bf16(const void* a, const float* b, void* out, int64_t n, msd_stream_t stream);

/* msd_cast_f32_to_bf16 / msd_cast_bf16_to_f32 — dtype conversion of a contiguous buffer. */
MSD_API int msd_cast_f32_to_bf16(const float* in, void* out, int64_t n, msd_stream_t stream);
MSD_API int msd_cast_bf16_to_f32(const void* in, float* out, int64_t n, msd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MINSDTF_HIP_H */
