// The kernel form a conv / dense launch names with MsdConvGemm.tile_m / tile_n / stages (include/minsdtf_hip.h), decoded ONCE on this
// side of the ABI: msd_conv_gemm, msd_conv_gemm_ln_slots and the launchers of the conv files read a CGForm, never the raw codes.
// minsdtf_amd/tuning.py form_of is the same decoder on the Python side.  Host only: plain integers, no table walk.
#pragma once

enum CGFamily {
    CG_TILE,       // tile_m < 1000: rows x cols LDS-DMA tile (conv_gemm.hip)
    CG_HALO,       // [1000, 3000): 3x3 on a staged halo of (pixels / 16) x 16 pixels (conv_halo.hip)
    CG_ROWPANEL,   // [3000, 4000): row-panel Dense kernel (conv_rowpanel.hip)
    CG_WREG,       // [4000, 5000): weights global -> VGPR (conv_wreg.hip)
    CG_BIG,        // [5000, 6000): 256-row macro tiles (conv_big.hip) ...
    CG_BIGHALO,    //   ... `stages` 20 + code: on a staged 18 x 18-pixel halo per chunk
    CG_NONE        // tile_m >= 6000 names no kernel form
};
struct CGForm {
    CGFamily family;
    bool valid;         // 0 <= tile_m < 6000 (a negative tile_m decodes as a tile and is refused like 6000 and up)
    int rows;           // rows (halo: pixels) per workgroup: tile_m less the family's base; tile: as given (0 = by size)
    int cols;           // tile_n as given (tile / halo: 0 = by size)
    int code;           // the configuration's code in its family's table: `stages` as given; big: less the + 10 / + 20 of the walk
    bool chunk_major;   // K walk: for every 64-channel chunk its nine taps (halo, big + 10, big + 20) instead of tap-major
    int variant;        // tile: 1 = `stages` 10 + depth (8 waves), 2 = 20 + depth (64x64 per wave); halo: 1 = tile_m 2000 + pixels (8 waves)
    int th;             // halo: tile height in pixels (8 / 16 for the built tiles)
};
static inline CGForm cg_decode_form(int tile_m, int tile_n, int stages) {
    const int walk = stages >= 20 ? 2 : stages >= 10 ? 1 : 0;
    CGForm f = {CG_TILE, tile_m >= 0 && tile_m < 6000, tile_m, tile_n, stages, false, 0, 0};
    if (tile_m >= 6000) f.family = CG_NONE;
    else if (tile_m < 1000) f.variant = walk;
    else if (tile_m >= 5000) {   // code + 10: the chunk-major walk, + 20: the same walk on the staged halo
        f.family = walk == 2 ? CG_BIGHALO : CG_BIG;
        f.rows = tile_m - 5000; f.code = stages - 10 * walk; f.chunk_major = walk > 0;
    } else if (tile_m >= 3000) {   // (wreg code: conv_wreg.hip wreg_code, depth + 10 for 8 waves + 20 for two K tiles per stage)
        f.family = tile_m >= 4000 ? CG_WREG : CG_ROWPANEL;
        f.rows = tile_m % 1000;
    } else if (tile_m >= 1000) {   // (code: conv_halo.hip MSD_HALO_CFGS, 0 / 30 / 60 / 90 / 150 + ring depth)
        f.family = CG_HALO;
        f.rows = tile_m % 1000; f.th = f.rows / 16; f.variant = tile_m >= 2000 ? 1 : 0; f.chunk_major = true;
    }
    return f;
}
static inline bool cg_is_big(const CGForm& f) { return f.family == CG_BIG || f.family == CG_BIGHALO; }

// the launchers behind msd_conv_gemm (included behind CGArgs, conv_common.h): each takes the decoded form of a configuration its file builds
int msd_conv_halo_launch(const CGArgs& a, const CGForm& f, int slices, hipStream_t stream);
bool msd_conv_rowpanel_eligible(const CGArgs& a, int rows, int wg_cols);
int msd_conv_rowpanel_launch(CGArgs a, int rows, int wg_cols, hipStream_t stream);
int msd_conv_wreg_nj(const CGForm& f);      // 16-column blocks per wave of a built configuration, 0: not built
int msd_conv_wreg_launch(const CGArgs& a, const CGForm& f, int slices, bool dense, hipStream_t stream);
int msd_conv_big_nj(const CGForm& f);       // conv_big.hip: 16-column blocks per wave of a built configuration, 0: not built
int msd_conv_big_launch(const CGArgs& a, const CGForm& f, int slices, bool dense, hipStream_t stream);
int msd_conv_bighalo_nj(const CGForm& f);   // conv_big.hip, halo-image variant (tile_m 5256, stages 20 + code)
int msd_conv_bighalo_launch(const CGArgs& a, const CGForm& f, int slices, hipStream_t stream);
