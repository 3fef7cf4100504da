// fp16 implicit-GEMM convolution for gfx950 (the bench / serving path), bordered NHWC activations,
// KRSC weights: the dispatch.  This file is host code; it decides which kernel a layer runs (pick) and
// launches it (launch_pick).  The kernels live one family per file: conv_f16_ring.hip (register-staged
// tile kernel, 8-wave LDS-DMA ring with split-K), conv_f16_pring.hip (persistent ring and its
// weight-stationary forms), conv_f16_p8.hip (8-phase rings), conv_det.hip / conv_det_nc.hip (Detect heads), and the 3x3 /
// register-weight kernels of conv_lr / conv_s2 / conv_w1 / conv_hring / conv_ws / conv_halo.hip.
//
// Replaces ATen conv2d + BN-folded bias + SiLU/LeakyReLU (Conv.fuseforward models/common.py:110-111,
// RepConv deploy common.py:498-500) and the Detect head conv + decode (models/yolo.py:46-57).
//
// GEMM view: M = B*Ho*Wo pixels, N = cout, K = k*k*cin ordered (r, s, ci).
//  * K step 64 (128 bytes per tile row), two v_mfma_f32_16x16x32_f16 sub-steps per tile per step;
//  * operands come in through raw buffer loads: each tile row (an output pixel's receptive-field
//    origin in the bordered input, or a weight row) is a per-lane byte offset computed once, the K
//    step's tap / channel position is a scalar offset (cin % 64 == 0: a K step never straddles two
//    taps), and the zero frame around every image replaces the padding tests — the K loop spends no
//    vector instructions on addressing.  Rows past M / cout land beyond the buffer range: zeros;
//  * LDS rows of 8 x 16-byte chunks, chunk index XOR-swizzled with (row & 7) so the 16-lane groups
//    of ds_read_b128 hit distinct 16-byte slots;
//  * operands swapped (weights as the MFMA A operand) so each lane's accumulator holds 4
//    consecutive output channels of one pixel: the epilogue packs them into 8-byte LDS writes, and
//    the tile leaves as full 16-byte NHWC row chunks into the output's channel slice (zero-copy concat);
//  * accumulators start at the bias; the activation is a compile-time constant in the epilogue;
//  * XCD-aware bijective block remap: consecutive tiles (all N tiles of an M tile) share an XCD's L2.
#include "conv_f16_common.h"
#include "conv_f16_launch.h"

namespace yv7 {

int device_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

namespace {

// YV7_CONV_F16=<n> forces variant <n> on every op that carries no variant of its own
int env_variant() {
  static const int v = env_int("YV7_CONV_F16", 0);
  return v;
}
// YV7_LR=0 takes conv_lr.hip out of the tuned rules: lr_default_cfg (stride 1) and pick_tuned's stride-2 rule
int env_lr() {
  static const int v = env_int("YV7_LR", 1);
  return v;
}

// What the dispatch decided for one layer: the kernel family, its configuration (a row of the family's
// table in conv_f16_launch.h, or the cfg of the family's own launcher) and K splits.
enum Family { F_INVALID, F_TILE, F_RING, F_PRING, F_P8, F_DET, F_DETNC, F_LR, F_S2, F_W1, F_HRING, F_WS64, F_HALO };
struct Pick {
  Family fam;
  int cfg = 0;
  int S = 0;   // F_RING: K splits (launch_ring)
};

// The dispatch's 8-phase-ring rule (pick_tuned quotes the measurements behind it).
bool p8_default(const ConvParams& p) {
  static const int on = env_int("YV7_P8", 1);
  const bool one = p.k == 1 && p.s == 1 && p.pad == 0;
  const long t256 = (long)((p.M + 255) / 256) * ((p.cout + 255) / 256);
  // (1x1 K = 512 -> 512 @80, 1600 tiles: 167 -> 159 us in-network, profiles/r3u_tune.txt)
  // Round 4, yolov7-w6 1280 bs 8 (profiles/r4_w6stem/tune_w6_dispatch.txt, one layer forced at a time,
  // us): 1x1 768->768 @40 31.2 -> 28.4 and 1536->768 @40 49.9 -> 44.2 at 150 tiles; 3x3 s2 128->256
  // @320 183.1 -> 156.1 and @160 47.0 -> 40.0 (the 128-input stride-2 layers).
  const bool w6 = t256 >= 150 && ((one && p.K >= 768 && p.cout >= 768) ||
                                  (p.k == 3 && p.s == 2 && p.cin == 128 && p.cout >= 256 && t256 >= 200));
  return on && !p.pool && p.cout >= 256 && p.cout <= 1024 && p.cout % 8 == 0 &&
         ((t256 >= 200 && ((one && p.K >= 1024) || (one && p.K >= 512 && p.cout >= 512 && t256 >= 1600) ||
                           (p.k == 3 && p.cin >= 256 && p.cin % BKE == 0))) ||
          w6);
}

// The ring rule: a configuration of the first NCFG rows of ring_rows (conv_f16_launch.h) with its K splits.
struct Choice {
  int cfg = -1;   // ring configuration, -1 = the legacy dispatch (halo / tile kernels / old variants)
  int S = 1;      // K splits
};

long ring_tiles(const ConvParams& p, int cfg) {
  const int bm = ring_rows[cfg].bm, bn = ring_rows[cfg].bn;
  return (long)((p.M + bm - 1) / bm) * ((p.cout + bn - 1) / bn);
}

// variant 100 + 10 * cfg + S forces ring configuration cfg with S K-splits (microbenchmarks).
Choice choose(const ConvParams& p, int variant) {
  Choice c;
  if (p.cout <= 32) return c;
  const int nk = p.kpad / BKE;
  if (variant >= 100 && variant < 100 + 10 * NCFG) {
    c.cfg = (variant - 100) / 10;
    c.S = variant % 10 ? variant % 10 : 1;
  } else if (variant == 0 && !halo_supported(p) && !ws64_supported(p)) {
    // Low-resolution layers (scripts/convbench.hip, bs 32, us): with at most 400 tiles of 128 x 128
    // (and for short-K 1x1 layers up to 3200) the 2-stage 128 x 128 ring (2 blocks per CU) beats the
    // wide tiles and the register-staged tile kernel (3x3 256->128 @40 50 -> 44, s2 512->512 @40
    // 88 -> 82, 1x1 256->256 @80 70 -> 61, 2048->512 @20 40 -> 37); the narrowest 1x1 take 128 x 64
    // (512->256 @20 11.7 -> 10.5); deep-K 3x3 layers under one round of tiles split K in two
    // (256->256 @20 35 -> 30, 512->256 @20 65 -> 47, s2 256->256 @40 36 -> 30; sc1 hand-off,
    // splitk_reduce), in four when a round of tiles covers at most half the CUs.  Wider grids keep the tuned wide tiles below.
    const long t128 = ring_tiles(p, R128x128s2);
    if (p.k > 1) {
      if (t128 <= 400) c.cfg = R128x128s2;
      if (t128 <= 256 && nk >= 36) c.S = 2;
      static const long s4max = env_int("YV7_SPLIT4_TILES", 128);
      // yolov7-w6 bs 8, 512->512 @20: 100 tiles x 4 K parts (72 -> 35 us); at 200 tiles (yolov7 bs 32,
      // 256->256 @20) four parts lose to two: 33 -> 46 us (YV7_SPLIT4_TILES=256 A/B)
      if (t128 <= s4max && nk >= 36) c.S = 4;
    } else {
      if (t128 <= 400 || (p.K <= 256 && t128 <= 3200)) c.cfg = R128x128s2;
      // 128 x 64 tiles under 200 tiles of 128 x 128, K split in two for K >= 2048 at <= 200 of them
      // (yolov7-w6 1280 bs 8 @20, profiles/r4_w6stem/tune_w6_dispatch.txt, us: 1024->1024 21.0 -> 15.4,
      // 2048->1024 33.0 -> 25.2, 1024->512 18.9 -> 13.7, 2048->512 32.6 -> 18.4 split, 512->384 12.3 -> 9.5)
      if (t128 <= 200) c.cfg = R128x64;
      if (t128 <= 200 && p.K >= 2048 && ring_tiles(p, R128x64) <= 200) c.S = 2;
    }
  }
  if (c.S > nk) c.S = nk;
  if (c.cfg >= 0 && c.S > 1 &&
      (double)ring_tiles(p, c.cfg) * c.S * ring_rows[c.cfg].bm * ring_rows[c.cfg].bn * 4 >= 2147483648.0)
    c.S = 1;   // partial tiles are addressed with 32-bit buffer offsets
  return c;
}

}  // namespace

// The split-K queries answer from the ring rule alone (plan_layout.cpp calls them with parameters that
// carry no output pitch or offset).
size_t conv_splitk_part_bytes(const ConvParams& p) {
  const Choice c = choose(p, p.variant ? p.variant : env_variant());   // (choose() keeps this under 2 GiB)
  if (c.cfg < 0 || c.S <= 1) return 0;
  return (size_t)ring_tiles(p, c.cfg) * c.S * ring_rows[c.cfg].bm * ring_rows[c.cfg].bn * 4;
}

int conv_splitk_tiles(const ConvParams& p) {
  const Choice c = choose(p, p.variant ? p.variant : env_variant());
  return (c.cfg < 0 || c.S <= 1) ? 0 : (int)ring_tiles(p, c.cfg);
}

int lr_default_cfg(const ConvParams& p) {
  if (env_lr() && !p.pool && (long)p.M <= 204800 && p.k == 3 && p.s == 1 &&
      !((long)p.B * (p.H / 16) * (p.W / 16) >= 800 && ws64_supported(p))) {
    const bool t5 = p.H % 5 == 0;
    const long t128 = (long)((p.B + 3) / 4) * (p.H / (t5 ? 5 : 4)) * (p.W / 4) * (p.cout / 128);
    int cfg = (p.cout % 128 == 0 && t128 >= 400 ? 0 : 1) + (t5 ? 0 : 2);
    // 160-pixel tiles (10 rows: each weight fragment feeds twice the MFMAs) where they keep >= 400 / 640
    // blocks (profiles/r4lr/tune_tm10*.txt, us): 160 x 128 for the channel-doubling RepConvs up to 384
    // inputs (yolov7 128->256 @80 115.5 -> 111.9, 256->512 @40 105.9 -> 100.2; w6 256->512 @80 104.2 ->
    // 95.9, 384->768 @40 62.2 -> 56.7), 160 x 64 for the other wide / 64-channel layers (512->512 @20
    // 61.9 -> 57.4, 512->1024 @20 103.8 -> 99.3, 128->64 @80 40.5 -> 37.7, 256->256 @40 56.3 -> 54.9)
    if (p.H % 10 == 0) {
      const long g10 = (long)((p.B + 3) / 4) * (p.H / 10) * (p.W / 4);
      if (p.cout % 128 == 0 && p.cout >= 2 * p.cin && p.cin <= 384 && g10 * (p.cout / 128) >= 400) cfg = 5;
      // (round 6: the 128-output exclusion kept only for 128-input layers — 256->128 took 160 x 64 by 1-2 us in
      // every sweep: yolov7 @40 ops 49 / 66, w6 @80 ops 57 / 73, profiles/r6_tune/tune_{yolov7,w6}_all.txt)
      else if ((p.cout != 128 || p.cin >= 256) && p.cout % 64 == 0 && g10 * (p.cout / 64) >= 480) cfg = 6;
    }
    // Round 5 (profiles/r5_misc/tune_small_w6.txt, us): 160 x 64 from 480 such tiles (w6 bs 8 384->384 @40
    // 38.0 / 37.9 / 37.1 / 37.3 -> 35.6-35.9); 64-pixel tiles on the 3 200-pixel layers (w6 bs 8 @20:
    // 512->512 25.3 / 25.0 / 25.2 -> 23.7-24.1, 512->256 18.4 -> 17.1, 256->256 11.3 -> 10.4)
    // (round 6, profiles/r6_tune/tune_w6_all.txt: not for cout 1024 — w6 bs 8 512->1024 @20 42.2 -> 36.9 us on
    // the 128-pixel tiles)
    if (cfg == 1 && p.M <= 6400 && p.cout <= 512 && lr_supported(p, 3)) cfg = 3;
    if (lr_supported(p, cfg)) return cfg;
  }
  return -1;
}

namespace {

// The register-staged tile kernel by output width: the last rule of the tuned path, and what a forced
// variant runs where its own form does not apply.
Pick pick_tile(const ConvParams& p) {
  return {F_TILE, p.cout <= 32 ? T128x32 : p.cout <= 64 ? T128x64 : T128x128};
}

// MP folded into a 1x1 conv: register-staged tile kernel (the max needs the operands in VGPRs)
Pick pick_pool(const ConvParams& p, bool det) {
  if (p.pool != 2 || p.k != 1 || p.s != 2 || p.pad != 0 || det || p.cin % 64) return {F_INVALID};
  // in-network A/B over the five yolov7 MP+1x1 pairs (us, 128x128 / 64x128): 256->128 @160 111 / 104,
  // 512->256 @80 71 / 68, 256->256 @40 16.9 / 15.1 (1024->512 @40 folds no more: 52 vs 46.5 unfused)
  static const int pcfg = env_int("YV7_POOL_CFG", 0);
  if (p.cout <= 64) return {F_TILE, T128x64pool};
  return {F_TILE, pcfg == 1 ? T128x128pool : T64x128pool};
}

Pick pick_det(const ConvParams& p, int variant) {
  // Detect head: the persistent head (conv_det_pring_kernel) where it applies; 98 = its
  // microbenchmark hook (no staging), 99 = the 64 x 256 ring below (the round-2 default).
  // DETECT variants: 89 = the class-count-generic head (conv_det_nc_kernel), 92 = the 64 x 256 tile kernel,
  // 94 = the persistent head with staged weights, 97 = the 128 x 256 ring, 99 = the 64 x 256 ring (the ABI
  // accepts these five); 91 / 93 / 95 / 96 / 98 = microbenchmark hooks of the (3, 85) heads.
  static const int det_pring = env_int("YV7_DET_PRING", 1);
  // Every head but the standard (na, no) = (3, 85) — with or without raw logits — runs the class-count-
  // generic head (conv_det_nc.hip: per-anchor tiles of the head's own width); variant 89 forces it on any
  // head, the standard one included.  The 256-wide forms below decode ONE N tile as channels 0 .. 255, so a
  // head with more channels (na * no > 256) is refused there, forced or not.
  // Measured against the 64 x 256 ring (bs 32, 256 @80^2 / 512 @40^2 / 1024 @20^2, us, ring -> this head,
  // profiles/det_nc/): nc 1 94.6 / 36.0 / 26.8 -> 53.3 / 22.6 / 13.3, nc 20 122 / 45.6 / 31.6 -> 68.3 / 27.7 /
  // 15.3, nc 40 139 / 50.4 / 34.1 -> 103 / 37.1 / 19.2, nc 59 154 / 54.1 / 35.0 -> 126 / 45.4 / 22.5, nc 70
  // 158-159 / 55.0 / 36.3 -> 155-156 / 51.9 / 24.1; nc 79 (252 channels: the ring's tile is full, this head
  // computes 3 x 96) 159-161 / 54.3 / 36.0 -> 164-167 / 56.4-57.4 / 25.0-26.7.  So the ring keeps the heads
  // that fill more than 15/16 of its tile (240 < na * no < 256) on levels of more than one 64-pixel tile per CU.
  if ((variant == 89 || (variant == 0 && !(p.na == 3 && p.no == 85))) && det_nc_supported(p)) {
    const bool ring_wins = p.cout > 240 && p.cout < 256 && (p.M + 63) / 64 > device_cus();
    if (variant == 89 || !ring_wins) return {F_DETNC};
  }
  if (((variant == 0 && det_pring) || variant == 94 || variant == 98 || variant == 96 || variant == 95 ||
       variant == 93 || variant == 91) && det_pring_supported(p))
    return {F_DET};
  // BN = 256 covers the na*no = 255 channels of a pixel
  // (scripts/detbench.hip, bs 32, row scores on: 64 x 256 ring, 2 blocks per CU so one block's
  // epilogue runs beside the other's main loop: 124 / 42 / 25 us at 80 / 40 / 20; 128 x 256 ring
  // 127 / 42 / 29; register-staged 64 x 256 tile 141 / 47 / 30)
  if (p.cout > 256) return {F_INVALID};
  if (variant == 92) return {F_TILE, T64x256det};
  if (variant == 97) return {F_RING, R128x256det};
  return {F_RING, R64x256det};
}

// The forced path: variants first .. last run `fam` with configuration cfg + (variant - first); where set,
// cfg32 / cfg64 / cfg128 replace it on layers of at most 32 / 64 / 128 outputs.  abi: yv7_set_op_variant
// accepts it as a kernel configuration (the rest are microbenchmark hooks and unchecked experiment
// schedules).
struct Forced {
  int first, last;
  Family fam;
  int cfg;
  bool abi;
  int cfg64 = -1, cfg128 = -1, cfg32 = -1;
};
constexpr Forced forced_rows[] = {
    {1, 1, F_TILE, T128x128, true, T128x64, -1, T128x32},   // the register-staged tile kernel (pick_tile)
    {2, 2, F_TILE, T128x128, true, T256x64, -1, T256x32},   // tall tiles for narrow layers
    {4, 4, F_RING, R256x128, true, R256x64},
    {5, 5, F_RING, R256x256, true, R512x64, R256x128s2},
    {6, 6, F_RING, R128x128s2, true, R128x64},
    {7, 7, F_RING, R128x128s3, true, R128x64s4},
    {8, 8, F_TILE, T128x128pf2, true, T128x64pf2, -1, T128x32},   // its PF = 2 form
    {10, 10, F_HALO, 0, true},
    // the persistent weight-stationary 64 -> 64 3x3 (conv_ws.hip): 11, its forms 15 and 17; 12-14 and 16 are its
    // microbenchmark hooks, 18-19 unchecked experiment schedules
    {11, 11, F_WS64, 0, true},
    {12, 14, F_WS64, 0, false},
    {15, 15, F_WS64, 0, true},
    {16, 16, F_WS64, 0, false},
    {17, 17, F_WS64, 0, true},
    {18, 19, F_WS64, 0, false},
    // 100 + 10 * ring configuration + K splits (choose(); the ABI takes up to 4 splits)
    {100, 100 + 10 * NCFG - 1, F_RING, 0, true},
    // persistent ring configurations (microbenchmarks: 201..206)
    {201, 206, F_PRING, P256x256, true},
    // 8-phase persistent ring (conv_f16_p8_kernel).  Round 4 removed the forced-only forms DESIGN §8
    // records as slower (BK-32 and 3-per-CU rings 211-218, pipelined rings 221-223, the p8 schedules
    // 233 / 237, the 512 x 128 p8 238, the first halo rings 260 / 261, the stand-alone 240).
    {231, 232, F_P8, P8_256x256, true},   // 231: 256 x 256 tiles, 232: 256 x 128
    // weight-stationary 1x1 rings (conv_f16_pring_kernel, WS): 234 = 128 x 256 tiles (K <= 256),
    // 235 = 256 x 128 (K <= 256), 236 = 128 x 128 (K <= 512)
    {234, 236, F_PRING, PWS128x256, true},
    // N-split weight-stationary 1x1 (K <= 256, 128 < cout <= 512): 256 x 128 tiles, three stages
    {239, 239, F_PRING, PWSN256x128, true},
    // the column-group 3x3 halo ring (conv_hring.hip, variant 262; 911-914: its microbenchmark hooks),
    // forced only where every N tile is full: the masked last tile of a cout that 128 does not divide has
    // no layer in the checked networks
    {262, 262, F_HRING, 0, true},
    // the low-resolution 3x3 kernel (conv_lr.hip): 270 + tile configuration
    {270, 279, F_LR, 0, true},
    // the register-weight stride-2 kernel (conv_s2.hip): 280 + tile configuration
    {280, 288, F_S2, 0, true},
    // the register-weight 1x1 kernel (conv_w1.hip): 290 + configuration
    {290, 295, F_W1, 0, true},
    {296, 298, F_PRING, PHOOK296, false},   // the persistent 256 x 256 ring's convbench hooks
    {299, 299, F_W1, 1, false},             // conv_w1's hooks, on its configuration 1
    {300, 300, F_W1, 1, false},
    {301, 301, F_W1, 1, false},
    {302, 303, F_W1, 6, true},              // its rows 6-7
    {911, 914, F_HRING, 0, false},
};

// The forced form's own *_supported test (the launchers' alignment tests are errors, not this)
bool forced_supported(const ConvParams& p, const Pick& k) {
  const bool one = p.k == 1 && p.s == 1 && p.pad == 0;
  switch (k.fam) {
    case F_HRING: return hring_supported(p) && p.cout % 128 == 0;
    case F_LR: return lr_supported(p, k.cfg);
    case F_S2: return s2_supported(p, k.cfg);
    case F_W1: return w1_supported(p, k.cfg);
    case F_TILE: return true;
    default: break;
  }
  if (p.cout <= 32) return false;   // the rings, ws64 and halo start at 33 outputs
  switch (k.fam) {
    case F_WS64: return ws64_supported(p);
    case F_HALO: return halo_supported(p);
    case F_P8: return one || p.cin % BKE == 0;
    case F_PRING: {
      const PringRow& r = pring_rows[k.cfg];
      if (r.kind == PR_WS) return one && p.cout <= r.bn && p.kpad <= r.ws * 64;
      if (r.kind == PR_WSN) return one && p.cout > 128 && p.cout <= 512 && p.kpad <= r.ws * 64;
      return true;
    }
    default: return true;
  }
}

Pick pick_forced(const ConvParams& p, int variant) {
  for (const Forced& f : forced_rows) {
    if (variant < f.first || variant > f.last) continue;
    Pick k{f.fam, f.cfg + (variant - f.first)};
    if (p.cout <= 32 && f.cfg32 >= 0) k.cfg = f.cfg32;
    else if (p.cout <= 64 && f.cfg64 >= 0) k.cfg = f.cfg64;
    else if (p.cout <= 128 && f.cfg128 >= 0) k.cfg = f.cfg128;
    if (variant >= 100 && f.fam == F_RING) {   // the ring rule's forced branch clamps the splits
      const Choice c = choose(p, variant);
      if (c.cfg < 0) break;
      k.cfg = c.cfg, k.S = c.S;
    }
    if (forced_supported(p, k)) return k;
    break;
  }
  // A forced variant whose form does not apply to the layer does not fall back to the tuned dispatch: it
  // runs the register-staged tile kernel (but variant 2 with cout <= 64: its tall tiles, in the table).
  return pick_tile(p);
}

Pick pick_tuned(const ConvParams& p) {
  const bool one = p.k == 1 && p.s == 1 && p.pad == 0;
  // The register-weight 3x3 kernel (conv_s2.hip) at stride 1, checked before the low-resolution rule
  // below (which would take the 204 800-pixel layers).  In-network, one layer forced at a time
  // (profiles/r5_s2/tune_s1_*.txt, us, dispatch -> s2 S=1): yolov7 bs 32 64->64 @320 228.2 -> 222.9
  // (cfg 6), 128->128 @80 65.6 -> 62.2 / 65.0 -> 63.0 (cfg 7), 128->256 @80 116.2 -> 108.2 (cfg 8);
  // yolov7-w6 bs 8 128->128 @160 68.4 -> 61.4, 128->256 @160 116.2 -> 106.5.  64->64 below 1 M pixels
  // and the 64-output 128-input layers (57.1 vs 38.3) keep the dispatch below.  YV7_S1=0: off.
  static const int s1k = env_int("YV7_S1", 1);
  if (s1k && p.k == 3 && p.s == 1 && !p.pool && (long)p.M >= 204800) {
    int cfg = -1;
    if (p.cin == 64 && p.cout == 64 && (long)p.M >= 1000000) cfg = 6;
    else if (p.cin == 128 && p.cout >= 128) cfg = p.cout >= 256 ? 8 : 7;
    if (cfg >= 0 && s2_supported(p, cfg)) return {F_S2, cfg};
  }
  // 3x3 stride-1 layers of up to 204 800 output pixels (yolov7 640 bs 32 from 80^2 down, yolov7-w6 1280
  // bs 8 from 160^2 down): the low-resolution kernel (conv_lr.hip) — one layer forced at a time in the bs-32
  // forward (profiles/r4lr/tune3.txt, us, dispatch -> lr): 3x3 256->256 @20 32.2 -> 22.1, 512->512 @20
  // 80.8 -> 62.7, 512->256 @20 48.8 -> 37.0, 512->1024 @20 119.8 -> 107.5, 128->128 @40 24.5 -> 21.9,
  // 256->128 @40 43.5 -> 35.6, 256->256 @40 69.9 -> 59.5, 256->512 @40 129.8 -> 108.5, 128->128 @80
  // 74.3 -> 63.4, 128->256 @80 123.9 -> 119.5, 128->64 @80 50.2 -> 40.8, 64->64 @80 31.6 -> 27.4.
  // 80 x 128 tiles when there are >= 400 of them, else 80 x 64 (64-pixel tiles when 5 does not divide
  // the height); w6 1280 bs 8 (profiles/r4lr/tune_w6.txt): 384->384 @40 38.7 -> 36.3 and 384->768 @40
  // 73.0 -> 66.0 with 80 x 128 (480 / 960 tiles); yolov7's 512->512 @20 and 128->128 / 256->128 @40
  // (640) are equal either way.  YV7_LR=0: off.
  if (const int cfg = lr_default_cfg(p); cfg >= 0) return {F_LR, cfg};
  // 3x3 stride-2 layers with 64 / 128 input channels and at least 204 800 output pixels: the register-weight
  // stride-2 kernel (conv_s2.hip).  In-network, one layer forced at a time (scripts/tune_ops.py,
  // profiles/r5_s2/tune_*.txt, us, dispatch -> s2): yolov7 bs 32 64->128 s2 @320 186.1 -> 130.4 (cfg 0),
  // 128->128 s2 @160 102.2 -> 74.0 (cfg 3); yolov7-w6 bs 8 128->256 s2 @320 159.2 -> 123.6 (cfg 4).  The
  // 51 200-pixel layers (128->128 s2 @80, w6 128->256 s2 @160) are equal either way and keep the
  // dispatch below.  YV7_S2=0: off.
  static const int s2k = env_int("YV7_S2", 1);
  if (s2k && p.k == 3 && p.s == 2 && (long)p.M >= 204800 && (p.cin == 64 || p.cin == 128)) {
    const int cfg = p.cin == 64 ? 0 : (p.cout >= 256 ? 4 : 3);
    if (s2_supported(p, cfg)) return {F_S2, cfg};
  }
  // 1x1 stride-1 layers with 128 / 256 / 512 inputs: the register-weight 1x1 kernel (conv_w1.hip).  In-
  // network, one layer forced at a time (scripts/tune_ops.py, profiles/r5_w1/tune_*.txt, us, dispatch ->
  // w1): yolov7 bs 32 128->128 @160 87.5 -> 75.2 (cfg 0), 256->256 @160 187.5 -> 163.5, @80 58.3 -> 49.1
  // (cfg 3), 512->512 @80 147.5 -> 119.9, @40 47.6 -> 39.6 (cfg 5), 512->384 @80 131.1 -> 113.1 (cfg 2);
  // yolov7-w6 bs 8 128->128 @320 91.3 -> 73.3, 512->256 @160 90.7 -> 65.5; 256->128 with a 128-channel
  // N slice (cfg 7; profiles/r5_misc/tune_small_w6.txt) @320 139.9 -> 123.6, @160 43.7 -> 34.1.  Narrower
  // grids keep the rings below.  YV7_W1=0: off.
  static const int w1k = env_int("YV7_W1", 1);
  if (w1k && one && !p.pool) {
    int cfg = -1;
    if (p.cin == 128 && p.M >= 409600) cfg = 0;
    else if (p.cin == 256 && p.M >= 204800) cfg = p.cout == 128 ? 7 : 3;
    else if (p.cin == 512 && p.M >= 51200) cfg = p.cout % 256 == 0 ? 5 : (p.M >= 204800 ? 2 : -1);
    if (cfg >= 0 && w1_supported(p, cfg)) return {F_W1, cfg};
  }
  // 3x3 stride-2 layers the 128 x 128 ring would split K for (under 256 of its tiles: yolov7's 256->256
  // s2 @40, w6's 768->1024 s2 @40): the stride-2 low-resolution form (profiles/r4lr/convbench_s2.txt:
  // 256->256 s2 @40 29.6 -> 25.4 us)
  // and the stride-2 layers of at most 12 800 output pixels but those with a round of 256 x 128 tiles
  // and cout >= 512, which the 8-phase ring below serves better (profiles/r4_w6stem/tune_*.txt, us:
  // w6 bs 8 512->768 s2 @80 134.6 -> 107.6, 256->384 s2 @80 39.5 -> 35.7; yolov7 bs 32 512->512 s2 @40
  // p8n 76.8 vs 90.5 here)
  const long t2n_s2 = (long)((p.M + 255) / 256) * ((p.cout + 127) / 128);
  // Round 5: the 80-pixel stride-2 tile (cfg 7, 5 output rows) on the 12 800-pixel layers with cout >= 384
  // (one layer forced at a time, profiles/r5_s2/tune_deep_w6.txt, us, cfg 4 -> 7: yolov7-w6 bs 8 512->768
  // s2 @80 109.1 -> 101.5, 256->384 s2 @80 37.7 -> 31.3; yolov7 bs 32 256->256 s2 @40 keeps cfg 4: 27.0
  // vs 28.8)
  if (env_lr() && p.k == 3 && p.s == 2 &&
      ((long)((p.M + 127) / 128) * ((p.cout + 127) / 128) <= 256 ||
       (p.M <= 12800 && !(t2n_s2 >= 150 && t2n_s2 <= 250 && p.cout >= 512)))) {
    const int cfg = (p.M >= 12800 && p.cout >= 384 && lr_supported(p, 7)) ? 7 : 4;
    if (lr_supported(p, cfg)) return {F_LR, cfg};
  }
  // 3x3 stride-1 layers with 128-channel output tiles and at least one round of 16 x 16 x 128 tiles: the
  // column-group halo ring (conv_hring.hip, variant 262).  Single-layer sweep, bs 32 640, same box
  // (profiles/r3_hring2_tune.txt, us, dispatch -> 262): 3x3 128->128 @80 80.0 / 80.4 / 82.7 / 81.0 ->
  // 67.2 / 67.9 / 69.3 / 68.4, 128->256 @80 139.1 -> 121.4.  YV7_HRING=0: off.
  static const int hring = env_int("YV7_HRING", 1);
  if (hring && hring_supported(p) && p.cout % 128 == 0 &&
      (long)p.B * (p.Ho / 16) * (p.Wo / 16) * (p.cout / 128) >= device_cus())
    return {F_HRING};
  if (p.cout > 32 && p.cout <= 1024 && p.cout % 8 == 0) {
    // Persistent ring (scripts/convbench.hip, bs 32, same box, us): short-K 1x1 layers and the
    // 128-channel / low-resolution 512-channel 3x3 layers, whose per-tile fill + epilogue the
    // non-persistent kernels cannot hide.  256 x 256 tiles once every CU gets >= 6 of them
    // (1x1 256->256 @160 304 -> 226, 512->512 @80 208 -> 183), else 128 x 128 with two blocks per
    // CU (1x1 128->128 @160 110 -> 89, 256->128 @160 161 -> 131, 256->256 @80 61 -> 55, 3x3
    // 128->128 @80 86 -> 81, s2 128->128 @160 96 -> 90, 512->512 @20 80 -> 76).
    const long t256 = (long)((p.M + 255) / 256) * ((p.cout + 255) / 256);
    // Wide layers with at least 200 tiles of 256 x 256 (in-network sweep of every ring configuration,
    // yolov7 bs 32, us, default -> persistent 256 x 256): 1x1 1024->1024 @40 156 -> 135, 1024->512 @40
    // 79 -> 69, 512->512 @40 55 -> 48, 1024->1024 @20 44 -> 39; 3x3 256->256 @40 86 -> 70, s2 256->256
    // @80 90 -> 77, 256->512 @40 157 -> 134, 512->1024 @20 146 -> 128.  Under 200 tiles (@20 with
    // cout <= 512) the persistent 256 x 256 ring loses (2048->512 @20 41 -> 59).  YV7_WIDE_PRING=0: off.
    static const int wide = env_int("YV7_WIDE_PRING", 1);
    // The 8-phase ring (conv_f16_p8_kernel) where it measured faster in-network (scripts/tune_ops.py,
    // one layer forced at a time, bs 32, us, dispatch before -> p8): 3x3 256->256 @40 76 -> 67, s2
    // 256->256 @80 79 -> 72, 256->512 @40 137 -> 126, 512->1024 @20 130 -> 114; 1x1 with K >= 1024:
    // 1024->1024 @40 142 -> 138, 1024->512 @40 74 -> 70, 1024->256 @40 41 -> 39.  Short-K 1x1 and
    // 128-input 3x3 layers stay on the 2-phase ring (1x1 256->256 @160 199 -> 216, 3x3 128->256 @80
    // 137 -> 144).  YV7_P8=0: off.

    // Weight-stationary 1x1 (K <= 256, 128 < cout <= 256, >= 80x80 at bs 32; tune_ops, us): 256->256
    // @160 213 -> 201, @80 70 -> 66 / 66 -> 65; narrower or lower-resolution 1x1 layers lose.
    // YV7_WS1=0: off.
    static const int ws1 = env_int("YV7_WS1", 1);
    // Round 3: its N-split form (two blocks per 256-pixel tile, each holding one 128-channel half of the
    // weights, three activation stages in flight instead of two; tune_ops, us: 256->256 @160 197.6 ->
    // 188.9, @80 60.3 -> 59.8 and 62.1 -> 58.6, profiles/r3w_tune.txt).
    if (ws1 && one && p.kpad <= 256 && p.cout > 128 && p.cout <= 256 && p.M >= 204800)
      return {F_PRING, PWSN256x128};
    // 3x3 stride-2 layers with about one round of 256 x 128 tiles: the 8-phase ring on 256 x 128 tiles
    // (all-layer sweep, profiles/r3y_tune.txt, us: 512->512 s2 @40 81.9 -> 75.5, 128->128 s2 @80
    // 29.6 -> 26.5)
    if (p.k == 3 && p.s == 2 && p.cin >= 128 && p.cin % BKE == 0 && p.cout % 128 == 0 && p.cout <= 1024) {
      const long t2n = (long)((p.M + 255) / 256) * (p.cout / 128);
      if (t2n >= 150 && t2n <= 250) return {F_P8, P8_256x128};
    }
    if (p8_default(p)) return {F_P8, P8_256x256};
    if (one) {
      // (a cout that is not a multiple of 256 — the tensor-fused pair 512->256+128 @80 — would leave
      // half of every last 256-wide N tile idle: the 128 x 128 ring below, 148.8 -> 124.2 us in-network,
      // profiles/r3r/tune.txt)
      const bool n256 = p.cout % 256 == 0 || p.K > 512;
      if (n256 && p.K >= 256 && p.cout >= 256 && t256 >= 1600) return {F_PRING, P256x256};
      if (n256 && wide && p.cout >= 256 && t256 >= 200) return {F_PRING, P256x256};
      if (p.K <= 512 && p.M >= 51200) return {F_PRING, P128x128s2};
    } else if (wide && p.k == 3 && p.cin >= 256 && p.cout >= 256 && t256 >= 200) {
      return {F_PRING, P256x256};
    } else if (p.k == 3 && p.cout == 128) {
      // (3x3 512->512 @20 and s2 from @40 take the non-persistent 128 x 128 ring of choose() below:
      // in-network 92 (this ring) / 89 (256 x 128 persistent) -> 79 us; with fewer tiles than CUs,
      // yolov7-w6 at bs 8, it splits K: 72 -> 35 us)
      return {F_PRING, P128x128s2};
    }
  }
  if (const Choice ch = choose(p, 0); ch.cfg >= 0) return {F_RING, ch.cfg, ch.S};
  if (p.cout > 32) {
    // 64 -> 64 3x3: the persistent weight-stationary kernel from 800 tiles of 16 x 16 (scripts/
    // convbench.hip, bs 32, same box: @320 423 -> 337 us, @160 95 -> 79 us vs the halo kernel).  Round 5:
    // its 8-wave form also takes the 800-tile layers from conv_lr (one layer forced at a time,
    // profiles/r5_misc/tune_small_*.txt, us: yolov7 bs 32 @80 27.3 / 26.2 / 26.8 -> 24.1 / 24.2 / 24.1,
    // yolov7-w6 bs 8 @160 25.7 / 26.3 / 25.7 -> 24.1 / 24.5 / 24.5)
    if ((long)p.B * (p.H / 16) * (p.W / 16) >= 800 && ws64_supported(p)) return {F_WS64};
    if (halo_supported(p)) return {F_HALO};
    if (p.cout >= 256) {
      // wide layers: the 8-wave ring kernels win once their grid still covers the chip
      // (scripts/convbench.hip, bs 32: 3x3 256->256 @40 112 -> 80 us, 512->1024 @20 208 -> 142 us,
      // 1x1 512->512 @80 243 -> 216 us); 512->512 @20 has 100 256x256 tiles -> 256x128 (88 vs 102 us)
      const long mt = (p.M + 255) / 256;
      if (mt * ((p.cout + 255) / 256) >= 150) return {F_RING, R256x256};
      if (mt * ((p.cout + 127) / 128) >= 150) return {F_RING, R256x128};
    }
  }
  return pick_tile(p);
}

// A conv that carries a residual (ConvParams::res): only the two families whose epilogue adds it, the
// register-staged tile kernel and the 8-wave ring (conv_f16_ring.hip).  Tuned: the ring rule where it applies,
// the wide rings while their grid covers the chip, else the 128 x 128 ring; up to 32 outputs the tile kernel.  A
// forced variant of another family (yv7_set_op_variant refuses it; YV7_CONV_F16 can still name one) runs the
// tile kernel, as a forced form that does not apply does.  The pooled and Detect paths refuse a residual.
Pick pick_res(const ConvParams& p, bool det, int variant) {
  if (det || p.pool) return {F_INVALID};
  Pick k;
  if (variant) {
    k = pick_forced(p, variant);
  } else if (p.cout <= 32) {
    k = pick_tile(p);
  } else if (const Choice ch = choose(p, 0); ch.cfg >= 0) {
    k = {F_RING, ch.cfg, ch.S};
  } else {
    const long mt = (p.M + 255) / 256;
    k = {F_RING, p.cout >= 256 && mt * ((p.cout + 255) / 256) >= 150   ? R256x256
                 : p.cout >= 256 && mt * ((p.cout + 127) / 128) >= 150 ? R256x128
                                                                        : R128x128s2};
  }
  if (k.fam == F_RING && k.cfg < NCFG) return {F_RING, RRES + k.cfg, k.S};
  const Pick t = pick_tile(p);   // (also a ring row without a residual form: the narrow-layer rows of 5 and 7)
  return {F_TILE, t.cfg == T128x32 ? T128x32res : t.cfg == T128x64 ? T128x64res : T128x128res};
}

Pick pick(const ConvParams& p, bool det) {
  const int variant = p.variant ? p.variant : env_variant();
  if (p.res) return pick_res(p, det, variant);
  if (p.pool) return pick_pool(p, det);
  if (det) return pick_det(p, variant);
  return variant ? pick_forced(p, variant) : pick_tuned(p);
}

hipError_t launch_pick(const ConvParams& p, const Pick& k, hipStream_t st) {
  switch (k.fam) {
    case F_TILE: return launch_tile(p, k.cfg, st);
    case F_RING: return launch_ring(p, k.cfg, k.S, st);
    case F_PRING: return launch_pring(p, k.cfg, st);
    case F_P8: return launch_p8(p, k.cfg, st);
    case F_DET: return launch_det_pring(p, st);
    case F_DETNC: return launch_det_nc(p, st);
    case F_LR: return launch_conv_lr(p, k.cfg, st);
    case F_S2: return launch_conv_s2(p, k.cfg, st);
    case F_W1: return launch_conv_w1(p, k.cfg, st);
    case F_HRING: return launch_conv_hring(p, st);
    case F_WS64: return launch_conv_ws64(p, st);
    case F_HALO: return launch_conv_halo(p, st);
    case F_INVALID: break;
  }
  return hipErrorInvalidValue;
}

}  // namespace

bool conv_f16_variant_is_config(int v) {
  for (const Forced& f : forced_rows)
    if (v >= f.first && v <= f.last) return f.abi && (v < 100 || f.fam != F_RING || v % 10 <= 4);
  return false;
}

bool conv_f16_variant_has_residual(int v) {
  return v == 1 || v == 4 || v == 6 || (v >= 100 && v < 100 + 10 * NCFG && v % 10 <= 4);
}

hipError_t launch_conv_f16(const ConvParams& p, bool det, hipStream_t st) { return launch_pick(p, pick(p, det), st); }

}  // namespace yv7
