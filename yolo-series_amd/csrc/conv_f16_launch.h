// Private interface between the fp16 dispatch (conv_f16.hip) and the kernel families it launches
// (conv_f16_ring.hip, conv_f16_pring.hip, conv_f16_p8.hip, conv_det.hip, conv_det_nc.hip).  Each family exports one
// non-template launch function per kernel, selected by a row of the family's table below: the tables
// list every instantiation the library holds.  An unknown row is hipErrorInvalidValue.
#pragma once
#include "yv7_kernels.h"

namespace yv7 {

// `one` of a row: the 1x1 / stride-1 / pad-0 form (K walks channels only) is instantiated for ...
enum OneForms { ONE_BOTH = -1, ONE_NEVER = 0, ONE_ONLY = 1 };

// conv_f16_ring.hip: the register-staged tile kernel, conv_f16_kernel<BM, BN, WM, ONE, DET, PF, POOL>
// res: conv_f16_res_kernel<BM, BN, WM, ONE>, the same tile with the residual epilogue (ConvParams::res)
struct TileRow { int bm, bn, wm, one, pf; bool det, pool, res = false; };
enum TileCfg { T128x32, T128x64, T128x128, T256x32, T256x64, T128x64pf2, T128x128pf2,
               T128x64pool, T128x128pool, T64x128pool, T64x256det, T128x32res, T128x64res, T128x128res, NTILE };
constexpr TileRow tile_rows[NTILE] = {
    {128, 32, 4, ONE_BOTH, 1, false, false},  {128, 64, 2, ONE_BOTH, 1, false, false},
    {128, 128, 2, ONE_BOTH, 1, false, false}, {256, 32, 4, ONE_BOTH, 1, false, false},
    {256, 64, 4, ONE_BOTH, 1, false, false},  {128, 64, 2, ONE_BOTH, 2, false, false},
    {128, 128, 2, ONE_BOTH, 2, false, false}, {128, 64, 2, ONE_NEVER, 1, false, true},
    {128, 128, 2, ONE_NEVER, 1, false, true}, {64, 128, 1, ONE_NEVER, 1, false, true},
    {64, 256, 1, ONE_ONLY, 1, true, false},   {128, 32, 4, ONE_BOTH, 1, false, false, true},
    {128, 64, 2, ONE_BOTH, 1, false, false, true}, {128, 128, 2, ONE_BOTH, 1, false, false, true}};
hipError_t launch_tile(const ConvParams& p, int row, hipStream_t st);

// conv_f16_ring.hip: the 8-wave LDS-DMA ring, conv_f16_ring_kernel<BM, BN, WM, WN, STAGES, ONE, DET>.
// The first NCFG rows are the configurations the split-K rule chooses from (variant 100 + 10 * row + S).
// (Round 6: 128 x 128 / 128 x 64 rings with 5-6 stages, 3-4 in flight, one block per CU, were slower on
// every 20^2 / 40^2 deep-K 1x1 layer: 1024->512 @20 25.9 -> 31.7 us, profiles/r6_ring_deep/tune.txt.)
// res: conv_f16_ring_res_kernel, the residual epilogue (split-K included); row RRES + c is configuration c < NCFG
struct RingRow { int bm, bn, wm, wn, stages, one; bool det, res = false; };
enum RingCfg { R256x256, R256x128, R128x128s3, R128x128s2, R128x64, R256x64, NCFG,
               R512x64 = NCFG, R256x128s2, R128x64s4, R128x256det, R64x256det, RRES, NRING = RRES + NCFG };
constexpr RingRow ring_rows[NRING] = {
    {256, 256, 2, 4, 2, ONE_BOTH, false}, {256, 128, 4, 2, 3, ONE_BOTH, false}, {128, 128, 2, 2, 3, ONE_BOTH, false},
    {128, 128, 2, 2, 2, ONE_BOTH, false}, {128, 64, 2, 2, 3, ONE_BOTH, false},  {256, 64, 4, 2, 3, ONE_BOTH, false},
    {512, 64, 8, 1, 2, ONE_BOTH, false},  {256, 128, 4, 2, 2, ONE_BOTH, false}, {128, 64, 2, 2, 4, ONE_BOTH, false},
    {128, 256, 2, 4, 3, ONE_ONLY, true},  {64, 256, 1, 4, 2, ONE_ONLY, true},
    {256, 256, 2, 4, 2, ONE_BOTH, false, true}, {256, 128, 4, 2, 3, ONE_BOTH, false, true},
    {128, 128, 2, 2, 3, ONE_BOTH, false, true}, {128, 128, 2, 2, 2, ONE_BOTH, false, true},
    {128, 64, 2, 2, 3, ONE_BOTH, false, true},  {256, 64, 4, 2, 3, ONE_BOTH, false, true}};
// S >= 1: S K-splits (ConvParams::ksplit = S; the caller sized the scratch with conv_splitk_part_bytes);
// S = 0: one block per tile, p as it stands
hipError_t launch_ring(const ConvParams& p, int row, int S, hipStream_t st);

// conv_f16_pring.hip: the persistent ring, conv_f16_pring_kernel<BM, BN, WM, WN, STAGES, ONE, ACT, 64, WS, HOOK>
// for every ACT.  ws > 0: the weight-stationary 1x1 forms holding ws K steps (PR_WS one N tile, PR_WSN
// N-split); hook: the convbench forms 296-298.
enum PringKind { PR_PLAIN, PR_WS, PR_WSN, PR_HOOK };
struct PringRow { int bm, bn, wm, wn, stages, kind, ws, hook, occ; };
enum PringCfg { P256x256, P256x128, P128x128s3, P128x128s2, P256x128s2, P128x256,
                PWS128x256, PWS256x128, PWS128x128, PWSN256x128, PHOOK296, PHOOK297, PHOOK298, NPRING };
// occ: resident blocks per CU the grid of a PR_PLAIN row is sized for
constexpr PringRow pring_rows[NPRING] = {
    {256, 256, 2, 4, 2, PR_PLAIN, 0, 0, 1}, {256, 128, 4, 2, 3, PR_PLAIN, 0, 0, 1}, {128, 128, 2, 2, 3, PR_PLAIN, 0, 0, 1},
    {128, 128, 2, 2, 2, PR_PLAIN, 0, 0, 2}, {256, 128, 4, 2, 2, PR_PLAIN, 0, 0, 1}, {128, 256, 2, 4, 2, PR_PLAIN, 0, 0, 1},
    {128, 256, 2, 4, 2, PR_WS, 4, 0, 1},    {256, 128, 4, 2, 2, PR_WS, 4, 0, 1},    {128, 128, 2, 4, 2, PR_WS, 8, 0, 1},
    {256, 128, 4, 2, 3, PR_WSN, 4, 0, 1},   {256, 256, 2, 4, 2, PR_HOOK, 0, 296, 1}, {256, 256, 2, 4, 2, PR_HOOK, 0, 297, 1},
    {256, 256, 2, 4, 2, PR_HOOK, 0, 298, 1}};
hipError_t launch_pring(const ConvParams& p, int row, hipStream_t st);

// conv_f16_p8.hip: the 8-phase rings, conv_f16_p8_kernel<ONE, ACT> (256 x 256) and conv_f16_p8n_kernel<ONE, ACT>
// (256 x 128), every ONE and ACT; uniform K steps only (1x1, or cin % 64 == 0)
enum P8Cfg { P8_256x256, P8_256x128 };
hipError_t launch_p8(const ConvParams& p, int cfg, hipStream_t st);

// conv_det.hip: the persistent Detect heads (conv_det_pring_kernel, conv_det_1tile_kernel,
// conv_det_rw_kernel); launch_det_pring picks among them and reads p.variant for their forced forms / hooks
bool det_pring_supported(const ConvParams& p);
hipError_t launch_det_pring(const ConvParams& p, hipStream_t st);

// conv_det_nc.hip: the class-count-generic Detect head (conv_det_nc_kernel<NW>): any na <= 4 and any no up
// to its widest compile-time tile, with or without raw logits.  det_nc_width: the tile width a head of `no`
// values per anchor runs (0: none)
int det_nc_width(int no);
bool det_nc_supported(const ConvParams& p);
hipError_t launch_det_nc(const ConvParams& p, hipStream_t st);

// A kernel configuration of the fp16 CONV dispatch the ABI may force (yv7_set_op_variant), as opposed
// to a microbenchmark hook or no variant at all: read from the dispatch's forced-variant table.
bool conv_f16_variant_is_config(int v);
// ... and one of a family that implements the residual epilogue (the tile kernel's variant 1, the rings 4, 6 and
// 100 + 10 * configuration + K splits): what yv7_set_op_variant accepts on a conv that carries a residual.
bool conv_f16_variant_has_residual(int v);

}  // namespace yv7
