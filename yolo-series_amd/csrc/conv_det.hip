// The Detect heads of fp16 plans (models/yolo.py:46-57): the 1x1 255-channel conv of one level and its
// decode in one kernel.  Three forms — the persistent head with staged weights, the one-tile head with a
// deep ring, the register-weight head — and launch_det_pring, which picks among them.
#include <cstdlib>

#include "conv_det.h"
#include "conv_f16_launch.h"

namespace yv7 {

namespace {

template <int HOOK = 0>
__global__ __launch_bounds__(512, 1) void conv_det_pring_kernel(const ConvParams p) {
  constexpr int BM = 64, BN = 256, WM = 2, WN = 4, NW = 8, NTH = 512;
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int RB = BN / 8 / NW;                  // 4 weight wave-instructions per stage (A: 1)
  constexpr int PER = HOOK == 4 ? 1 : 1 + RB;   // (hook 4: no weight DMA)
  constexpr int STAGE = (BM + BN) * ROWB;          // 40 KiB
  constexpr int RING = 2 * STAGE;
  constexpr int LDS = RING + det_lds(BM, BN);
  static_assert(LDS <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS];
  unsigned char* es = smem + RING;                 // zs + row table

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int g = lane >> 4, li = lane & 15;
  const int T = (p.M + BM - 1) / BM;
  const int nk = p.kpad / BKE;
  const TileWalk tw = xcd_tile_walk(T);
  const int ntl = tw.count();
  if (ntl == 0) return;

  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.w, p.wbytes);
  const int lr = lane >> 3;
  const int c = (lane & 7) ^ lr;
  uint32_t b_off[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) b_off[j] = (uint32_t)((((j * NW + wave) * 8 + lr) * p.kpad + c * 8) * 2);
  const int hw = p.Ho * p.Wo;
  auto a_off = [&](int it) -> uint32_t {
    if (it >= ntl) return OOB;
    const int m = tw.at(it) * BM + wave * 8 + lr;
    if (m >= p.M) return OOB;
    const int b = m / hw, cell = m - b * hw, ho = cell / p.Wo, wo = cell - ho * p.Wo;
    return (uint32_t)((pix_index(b, ho, wo, p.H, p.W) * p.xc + p.xoff + c * 8) * 2);
  };
  // stage q = (tile it, K step k) into slot q & 1
  int i_it = 0, i_k = 0, i_q = 0;
  uint32_t i_aoff = a_off(0);
  auto issue = [&]() __attribute__((always_inline)) {
    unsigned char* As = smem + (i_q & 1) * STAGE;
    unsigned char* Bs = As + BM * ROWB;
    const bool live = i_it < ntl;
    const uint32_t so = (uint32_t)i_k * BKE * 2;
    dma16(xr, As + wave * 8 * ROWB, i_aoff, so);
    if constexpr (HOOK != 4) {
#pragma unroll
      for (int j = 0; j < RB; ++j) dma16(wr, Bs + (j * NW + wave) * 8 * ROWB, live ? b_off[j] : OOB, so);
    }
    asm volatile("" ::: "memory");
    ++i_q;
    if (++i_k == nk) {
      i_k = 0;
      ++i_it;
      i_aoff = a_off(i_it);
    }
  };

  const f4 bias0 = {0.0f, 0.0f, 0.0f, 0.0f};
  f4 bv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = wn * WTN + j * 16 + g * 4;
    bv[j] = bias0;
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[j][e] = col + e < p.cout ? p.bias[col + e] : 0.0f;
  }
  const int nst = p.best ? 10 : 8;   // epilogue stores per wave per tile (det_tail_fixed)

  // z slot of each of this lane's 16 channels (j, e) in the tile's [na][BM][no] image (tile-invariant;
  // the padding channel 255 -> a spare slot)
  constexpr int NO = 85, NA = 3;
  int zo[TN][4];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ch = wn * WTN + j * 16 + g * 4 + e;
      const int ca = ch / NO;
      zo[j][e] = ca < NA ? ca * BM * NO + (ch - ca * NO) : NA * BM * NO;
    }
  // the level's anchors once (a per-lane kernel-argument load: its wait stays out of the tile loop)
  if (tid < 8) det_tab_ptrs<BM, BN>(es).anc[tid] = p.anchor[tid];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  issue();
  issue();
  for (int it = 0; it < ntl; ++it) {
    const int m0 = tw.at(it) * BM;
    f4 acc[TN][TM];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i) acc[j][i] = bv[j];
    for (int k = 0; k < nk; ++k) {
      // stage (it, k) landed: younger are stage (it, 1) and the previous epilogue's stores at k = 0,
      // the previous epilogue's stores at k = 1 (both stages of a tile start are issued before them)
      if (k == 0) {
        if (it > 0 && nst == 10) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER + 10) : "memory");
        else if (it > 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER + 8) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
      } else if (k == 1 && it > 0) {
        if (nst == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();
      if (k >= 1) issue();              // stage (it, k + 1) or the next tile's first stage
      if (k == 0) det_table<BM, BN, NTH, false>(p, es, m0, tid);   // read after the K loop's last barrier
      const unsigned char* As = smem + ((it * nk + k) & 1) * STAGE;
      const unsigned char* Bs = As + BM * ROWB;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int ch = s * 4 + g;
        u4 xa[TM], wb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = wm * WTM + i * 16 + li;
          xa[i] = *reinterpret_cast<const u4*>(As + row * ROWB + swz(row, ch) * 16);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int row = wn * WTN + j * 16 + li;
          wb[j] = *reinterpret_cast<const u4*>(Bs + row * ROWB + swz(row, ch) * 16);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int i = 0; i < TM; ++i)
            acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wb[j]),
                                                               __builtin_bit_cast(h8, xa[i]), acc[j][i], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // epilogue: ring reads done -> the next tile's stage (it + 1, 1) into the free slot
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    issue();
    if constexpr (HOOK != 1 && HOOK != 3) {
      // staging: the sigmoid of every logit into zs (z's layout); the 4 box columns of each row are
      // decoded in det_tail_fixed (one (row, column) per thread there, beside the row scores)
      float* zs = reinterpret_cast<float*>(es);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int roff = (wm * WTM + i * 16 + li) * NO;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) zs[zo[j][e] + (zo[j][e] < NA * BM * NO ? roff : 0)] = det_sig(acc[j][i][e]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // z / record rows of this tile relative to its first pixel's row (offsets stay 32-bit at any batch)
    const int mb = m0 / hw;
    const long long zb = (long long)mb * p.nrows + p.row_off + (m0 - mb * hw);
    const auto zr = make_rsrc(p.z + (size_t)zb * 85, 0x7fffffffu);
    const auto br = make_rsrc(p.best ? p.best + (size_t)zb * 4 : p.z, 0x7fffffffu);
    if constexpr (HOOK < 2) det_tail_fixed<BM, NTH>(p, es, tid, zr, br, zb);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One-tile Detect head (round 6): where a level has at most one 64-pixel tile per CU (yolov7 bs 32's P5 head,
// 1024 -> 255 @20: 200 tiles), every block of the persistent head runs ONE tile, and its two-slot ring waits out
// an L2 round trip at each of the 16 K steps (PMC: 65 % of the wave cycles waiting, profiles/r5_pmc_kernels/).
// With no next tile to prefetch, the z staging image needs no room of its own during the K loop: four 40 KiB
// stages (three in flight) fill the LDS, and the staging image + row table reuse it after the loop.  Same
// arithmetic as conv_det_pring_kernel (bit-identical z and row records).
__global__ __launch_bounds__(512, 1) void conv_det_1tile_kernel(const ConvParams p) {
  constexpr int BM = 64, BN = 256, WM = 2, WN = 4, NW = 8, NTH = 512;
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int RB = BN / 8 / NW;                  // 4 weight wave-instructions per stage (A: 1)
  constexpr int PER = 1 + RB;
  constexpr int STAGE = (BM + BN) * ROWB;          // 40 KiB
  constexpr int NS = 4;
  constexpr int LDS = NS * STAGE;
  static_assert(LDS <= 160 * 1024 && det_lds(BM, BN) <= LDS, "LDS budget");
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS];
  unsigned char* es = smem;                        // zs + row table, after the K loop

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int g = lane >> 4, li = lane & 15;
  const int m0 = blockIdx.x * BM;
  if (m0 >= p.M) return;
  const int nk = p.kpad / BKE;
  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.w, p.wbytes);
  const int lr = lane >> 3;
  const int c = (lane & 7) ^ lr;
  uint32_t b_off[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) b_off[j] = (uint32_t)((((j * NW + wave) * 8 + lr) * p.kpad + c * 8) * 2);
  const int hw = p.Ho * p.Wo;
  uint32_t aoff = OOB;
  {
    const int m = m0 + wave * 8 + lr;
    if (m < p.M) {
      const int b = m / hw, cell = m - b * hw, ho = cell / p.Wo, wo = cell - ho * p.Wo;
      aoff = (uint32_t)((pix_index(b, ho, wo, p.H, p.W) * p.xc + p.xoff + c * 8) * 2);
    }
  }
  auto issue = [&](int k, int slot) __attribute__((always_inline)) {
    unsigned char* As = smem + slot * STAGE;
    unsigned char* Bs = As + BM * ROWB;
    const uint32_t so = (uint32_t)k * BKE * 2;
    dma16(xr, As + wave * 8 * ROWB, aoff, so);
#pragma unroll
    for (int j = 0; j < RB; ++j) dma16(wr, Bs + (j * NW + wave) * 8 * ROWB, b_off[j], so);
    asm volatile("" ::: "memory");
  };
  f4 acc[TN][TM];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = wn * WTN + j * 16 + g * 4;
    f4 bv;
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = col + e < p.cout ? p.bias[col + e] : 0.0f;
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[j][i] = bv;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // bias
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nk) issue(s, s);
  for (int k = 0; k < nk; ++k) {
    ring_wait<PER, NS - 2>(nk - 1 - k);   // stage k landed; up to NS - 2 later stages in flight
    __builtin_amdgcn_s_barrier();
    if (k + NS - 1 < nk) issue(k + NS - 1, (k + NS - 1) & (NS - 1));   // into the slot step k - 1 read
    const unsigned char* As = smem + (k & (NS - 1)) * STAGE;
    const unsigned char* Bs = As + BM * ROWB;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int ch = s * 4 + g;
      u4 xa[TM], wb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 16 + li;
        xa[i] = *reinterpret_cast<const u4*>(As + row * ROWB + swz(row, ch) * 16);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * WTN + j * 16 + li;
        wb[j] = *reinterpret_cast<const u4*>(Bs + row * ROWB + swz(row, ch) * 16);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i)
          acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wb[j]),
                                                             __builtin_bit_cast(h8, xa[i]), acc[j][i], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();   // the ring is free: the staging image and row table take its place
  if (tid < 8) det_tab_ptrs<BM, BN>(es).anc[tid] = p.anchor[tid];
  det_table<BM, BN, NTH, false>(p, es, m0, tid);
  {
    constexpr int NO = 85, NA = 3;
    float* zs = reinterpret_cast<float*>(es);
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = wn * WTN + j * 16 + g * 4 + e;
        const int ca = ch / NO;
        const int zo = ca < NA ? ca * BM * NO + (ch - ca * NO) : NA * BM * NO;
#pragma unroll
        for (int i = 0; i < TM; ++i)
          zs[zo + (zo < NA * BM * NO ? (wm * WTM + i * 16 + li) * NO : 0)] = det_sig(acc[j][i][e]);
      }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  const int mb = m0 / hw;
  const long long zb = (long long)mb * p.nrows + p.row_off + (m0 - mb * hw);
  const auto zr = make_rsrc(p.z + (size_t)zb * 85, 0x7fffffffu);
  const auto br = make_rsrc(p.best ? p.best + (size_t)zb * 4 : p.z, 0x7fffffffu);
  det_tail_fixed<BM, NTH>(p, es, tid, zr, br, zb);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Register-weight Detect head (round 5, the default for K = 256 / 512: yolov7's P3 / P4 heads, w6's P3
// / P4).  scripts/detbench.hip's hook 93 (the persistent head above without its weight DMA,
// profiles/r5_det/detbench_hooks_noweights.txt) runs 256->255 @80 bs 32 in 41-50 us against 91-92 and
// 512->255 @40 in 20 against 40: restaging the 256-channel weight tile (4 of the 5 pieces of every K
// step) for every 64-pixel tile costs as much as the whole rest of the kernel.  Here the weights never
// move: wave w keeps channels 32 w .. 32 w + 31 for all of K in VGPRs (2 x NCH fragments from the
// fragment-packed copy: 64 VGPRs at K = 256, 128 at K = 512), the ring stages only the tile's pixels (8
// KiB per K step), and the wave computes those 32 channels for all 64 pixels (4 pixel fragments per read
// step, each feeding 2 MFMAs).  Epilogue and row records as conv_det_pring_kernel (det_tail_fixed; the
// same sigmoid and decode: bit-identical z and records).
// HOOK (detbench only, variant 91; the ABI never accepts it): 1 = no pixel DMA (stale LDS operands)
// D (round 6): pixel stages in flight ahead of the one being read.  D = 0 is the round-5 schedule (a
// two-slot ring: the K step's stage issued one step ahead, plus the next tile's second stage before the
// epilogue).  D > 0: a (D + 1)-slot ring, one stage issued per K step D steps ahead, so at K = 256 (4 steps)
// the whole next tile's pixels are in flight during this tile's epilogue instead of being waited for inside
// its K loop.  Stage s is read at global step s; the stores of the epilogue between two tiles are younger
// than the stages issued before it, so the counted wait at step k of a tile allows D - 1 younger stages,
// plus the previous epilogue's nst stores while those stages were issued before it (k < D, tile > 0).
// BM (round 6): pixels per tile, 64 or 32 — at 32 the four pixel pieces of a stage are issued by waves 0-3 and
// again by waves 4-7 (the same bytes to the same rows), so every wave's counted waits stay the same.
template <int NCH, int HOOK = 0, int D = 0, int BM = 64>
__global__ __launch_bounds__(512, 1) void conv_det_rw_kernel(const ConvParams p) {
  constexpr int BN = 256, NTH = 512, TM = BM / 16, TN = 2, NK = NCH / 2;
  static_assert(BM == 64 || BM == 32, "tile");
  // epilogue stores per wave per tile (det_tail_fixed): row records, z rows
  constexpr int NREC = (BM * 3 * 4 + NTH - 1) / NTH, NZS = (3 * (BM / 4) + NTH / 85 - 1) / (NTH / 85);
  constexpr int NSTB = NREC + NZS, NSTN = NZS;
  constexpr int PER = HOOK == 1 ? 0 : 1;           // one A piece per wave per stage
  constexpr int STAGE = BM * ROWB;                 // 8 KiB
  constexpr int R = D > 0 ? D + 1 : 2;             // ring slots
  constexpr int RING = R * STAGE;
  constexpr int LDS = RING + det_lds(BM, BN);
  static_assert(LDS <= 160 * 1024, "LDS budget");
  static_assert(D == 0 || ((D - 1) * PER + NSTB <= 63 && D <= NK), "counted waits");
  constexpr int NO = 85, NA = 3;
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS];
  unsigned char* es = smem + RING;                 // zs + row table

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int T = (p.M + BM - 1) / BM;
  const TileWalk tw = xcd_tile_walk(T);
  const int ntl = tw.count();
  if (ntl == 0) return;

  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.wf, p.wfbytes);
  // the wave's weights: fragment (16-channel group 2 wave + j, K step c) at ((2 wave + j) * NCH + c) KiB
  u4 wreg[TN][NCH];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const uint32_t base = (uint32_t)(((2 * wave + j) * NCH) * 1024 + lane * 16);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      wreg[j][c] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(wr, base, (uint32_t)(c * 1024), 0));
  }
  const int lr = lane >> 3;
  const int c8 = (lane & 7) ^ lr;
  const int hw = p.Ho * p.Wo;
  auto a_off = [&](int it) -> uint32_t {
    if (it >= ntl) return OOB;
    const int m = tw.at(it) * BM + (wave % (BM / 8)) * 8 + lr;
    if (m >= p.M) return OOB;
    const int b = m / hw, cell = m - b * hw, ho = cell / p.Wo, wo = cell - ho * p.Wo;
    return (uint32_t)((pix_index(b, ho, wo, p.H, p.W) * p.xc + p.xoff + c8 * 8) * 2);
  };
  // stage q = (tile it, K step k) into slot q % R
  int i_it = 0, i_k = 0, i_slot = 0;
  uint32_t i_aoff = a_off(0);
  auto issue = [&]() __attribute__((always_inline)) {
    if constexpr (HOOK != 1) dma16(xr, smem + i_slot * STAGE + (wave % (BM / 8)) * 8 * ROWB, i_aoff, (uint32_t)i_k * BKE * 2);
    asm volatile("" ::: "memory");
    if (++i_slot == R) i_slot = 0;
    if (++i_k == NK) {
      i_k = 0;
      ++i_it;
      i_aoff = a_off(i_it);
    }
  };

  f4 bv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = wave * 32 + j * 16 + g * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[j][e] = col + e < p.cout ? p.bias[col + e] : 0.0f;
  }
  const int nst = p.best ? NSTB : NSTN;
  // z slot of each of this lane's 8 channels (the padding channel 255 -> a spare slot)
  int zo[TN][4];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ch = wave * 32 + j * 16 + g * 4 + e;
      const int ca = ch / NO;
      zo[j][e] = ca < NA ? ca * BM * NO + (ch - ca * NO) : NA * BM * NO;
    }
  if (tid < 8) det_tab_ptrs<BM, BN>(es).anc[tid] = p.anchor[tid];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // weights, bias, anchors
#pragma unroll
  for (int d = 0; d < (D > 0 ? D : 2); ++d) issue();
  int r_slot = 0;   // the slot of the stage the next K step reads
  for (int it = 0; it < ntl; ++it) {
    const int m0 = tw.at(it) * BM;
    f4 acc[TN][TM];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i) acc[j][i] = bv[j];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if constexpr (D == 0) {
        // stage (it, k) landed: younger are stage (it, 1) and the previous epilogue's stores at k = 0, the
        // previous epilogue's stores at k = 1 (both stages of a tile start are issued before them)
        if (k == 0) {
          if (it > 0 && nst == NSTB) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER + NSTB) : "memory");
          else if (it > 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER + NSTN) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
        } else if (k == 1 && it > 0) {
          if (nst == NSTB) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSTB) : "memory");
          else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSTN) : "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
      } else {
        if (k >= D || it == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * PER) : "memory");
        else if (nst == NSTB) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * PER + NSTB) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 1) * PER + NSTN) : "memory");
      }
      __builtin_amdgcn_s_barrier();
      if (D > 0 || k >= 1) issue();     // D > 0: stage s + D; D = 0: stage (it, k + 1) or the next tile's first
      if (k == 0) det_table<BM, BN, NTH, false>(p, es, m0, tid);   // read after the K loop's last barrier
      const unsigned char* As = smem + r_slot * STAGE;
      if (++r_slot == R) r_slot = 0;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int ch = s2 * 4 + g;
        u4 xa[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = i * 16 + li;
          xa[i] = *reinterpret_cast<const u4*>(As + row * ROWB + swz(row, ch) * 16);
        }
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int i = 0; i < TM; ++i)
            acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wreg[j][2 * k + s2]),
                                                               __builtin_bit_cast(h8, xa[i]), acc[j][i], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
      }
    }
    // epilogue: ring reads done (D = 0: -> the next tile's stage (it + 1, 1) into the free slot)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (D == 0) issue();
    // staging: the sigmoid of every logit into zs (z's layout); the box columns are decoded in
    // det_tail_fixed
    float* zs = reinterpret_cast<float*>(es);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int roff = (i * 16 + li) * NO;
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) zs[zo[j][e] + (zo[j][e] < NA * BM * NO ? roff : 0)] = det_sig(acc[j][i][e]);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const int mb = m0 / hw;
    const long long zb = (long long)mb * p.nrows + p.row_off + (m0 - mb * hw);
    const auto zr = make_rsrc(p.z + (size_t)zb * 85, 0x7fffffffu);
    const auto br = make_rsrc(p.best ? p.best + (size_t)zb * 4 : p.z, 0x7fffffffu);
    det_tail_fixed<BM, NTH, NCH == 8 ? 0 : 2>(p, es, tid, zr, br, zb);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

bool det_rw_supported(const ConvParams& p) {
  return p.wf && (p.kpad == 256 || p.kpad == 512) && p.wfbytes >= (uint32_t)(256 * p.kpad * 2);
}

}  // namespace

bool det_pring_supported(const ConvParams& p) {
  const int hw = p.Ho * p.Wo;
  return p.k == 1 && p.s == 1 && p.na == 3 && p.no == 85 && p.cout == 255 && p.raw == nullptr &&
         p.kpad == p.cin && p.cin % BKE == 0 && p.cin >= 2 * BKE && hw % 4 == 0 && p.row_off % 4 == 0 &&
         p.nrows % 4 == 0 && p.xoff % 8 == 0 && p.xc % 8 == 0 && p.H == p.Ho && p.W == p.Wo;
}

hipError_t launch_det_pring(const ConvParams& p, hipStream_t st) {
  const long T = (p.M + 63) / 64, cus = device_cus();
  const long per = (T + cus - 1) / cus;
  const int grid = (int)((T + per - 1) / per);
  // microbenchmark hooks (scripts/detbench.hip; the ABI never accepts them): 98 = no sigmoid staging,
  // 96 = no tail (decode, row scores, z / record stores), 95 = neither (the GEMM, its ring and the
  // epilogue barriers only)
  // the register-weight head (conv_det_rw_kernel) by default where the plan packed its weights (K = 256 /
  // 512); 94 = the persistent head with staged weights, kept as a forced variant.  YV7_DET_RW=0: off.
  // In-network A/B, same box (profiles/r5_det/rw/, rw512/): 256->255 @80 82.7 -> 67.3 us, 512->255 @40
  // 38.9 -> 35.6 us.
  static const int rw = env_int("YV7_DET_RW", 1);
  if (rw && (p.variant == 0 || p.variant == 91) && det_rw_supported(p)) {
    if (p.variant == 91) {   // its hook (no pixel DMA)
      if (p.kpad == 256) YV7_LAUNCH((conv_det_rw_kernel<8, 1>), dim3(grid), dim3(512), 0, st, p);
      else YV7_LAUNCH((conv_det_rw_kernel<16, 1>), dim3(grid), dim3(512), 0, st, p);
      return hipGetLastError();
    }
    // YV7_DET_RWD: pixel stages in flight (conv_det_rw_kernel's D; 0 = the round-5 two-slot schedule)
    static const int rwd = env_int("YV7_DET_RWD", 4);
    // 32-pixel tiles at K = 512 (round 6): 1x1 512->255 @40 at bs 32 is 800 tiles of 64 = 4 rounds on 200
    // blocks, or 1600 of 32 = 7 half-size rounds on 229 — 33.7 -> 31.5 us in-network, same box; at K = 256
    // (256->255 @80, 3200 / 6400 tiles) the halved tiles lose, 60.6 -> 70.0 (profiles/r6_det/bm32/).
    // YV7_DET_BM=32 / 64 forces either.
    static const int bm_env = env_int("YV7_DET_BM", 0);
    const int bm = bm_env ? bm_env : (p.kpad == 512 ? 32 : 64);
    if (bm == 32 && rwd == 4) {
      const long T2 = (p.M + 31) / 32, per2 = (T2 + cus - 1) / cus;
      const int grid2 = (int)((T2 + per2 - 1) / per2);
      if (p.kpad == 256) YV7_LAUNCH((conv_det_rw_kernel<8, 0, 4, 32>), dim3(grid2), dim3(512), 0, st, p);
      else YV7_LAUNCH((conv_det_rw_kernel<16, 0, 4, 32>), dim3(grid2), dim3(512), 0, st, p);
      return hipGetLastError();
    }
    if (p.kpad == 256) {
      if (rwd == 0) YV7_LAUNCH(conv_det_rw_kernel<8>, dim3(grid), dim3(512), 0, st, p);
      else YV7_LAUNCH((conv_det_rw_kernel<8, 0, 4>), dim3(grid), dim3(512), 0, st, p);
    } else {   // K = 512 (6 and 8 stages ahead measured no faster than 4: profiles/r6_det/ring_k512/)
      if (rwd == 0) YV7_LAUNCH(conv_det_rw_kernel<16>, dim3(grid), dim3(512), 0, st, p);
      else YV7_LAUNCH((conv_det_rw_kernel<16, 0, 4>), dim3(grid), dim3(512), 0, st, p);
    }
    return hipGetLastError();
  }
  // one 64-pixel tile per CU at most (yolov7 bs 32's P5 head): the one-tile head with its deep ring (round 6;
  // YV7_DET_1T=0: off)
  static const int one_tile = env_int("YV7_DET_1T", 1);
  if (one_tile && p.variant == 0 && T <= cus && det_lds(64, 256) <= 4 * (64 + 256) * ROWB) {
    YV7_LAUNCH(conv_det_1tile_kernel, dim3((unsigned)T), dim3(512), 0, st, p);
    return hipGetLastError();
  }
  if (p.variant == 98) YV7_LAUNCH(conv_det_pring_kernel<1>, dim3(grid), dim3(512), 0, st, p);
  else if (p.variant == 96) YV7_LAUNCH(conv_det_pring_kernel<2>, dim3(grid), dim3(512), 0, st, p);
  else if (p.variant == 95) YV7_LAUNCH(conv_det_pring_kernel<3>, dim3(grid), dim3(512), 0, st, p);
  else if (p.variant == 93) YV7_LAUNCH(conv_det_pring_kernel<4>, dim3(grid), dim3(512), 0, st, p);   // no weight DMA
  else YV7_LAUNCH(conv_det_pring_kernel<0>, dim3(grid), dim3(512), 0, st, p);
  return hipGetLastError();
}

}  // namespace yv7
