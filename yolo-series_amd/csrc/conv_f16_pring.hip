// The persistent ring of the fp16 implicit-GEMM conv (conv_f16.hip describes the GEMM view) and its
// weight-stationary forms; launch_pring launches a row of pring_rows (conv_f16_launch.h).
#include "conv_f16_common.h"
#include "conv_f16_launch.h"

namespace yv7 {

namespace {

// Persistent ring (short-K layers).  Non-persistent tiles pay, per tile, the ring fill latency and
// an LDS-staged epilogue during which nothing streams; for K = 128..512 that is most of the tile.
// Here every block walks tiles t = blockIdx.x, + gridDim.x, ...:
//  * the LDS-DMA ring of K steps runs on across tile boundaries — the next tile's first stages are
//    in flight while the current tile finishes and writes back;
//  * the epilogue goes straight from the accumulators (bias from LDS at accumulator init,
//    compile-time activation, fp16, one v_permlane16_swap per dword so a lane holds 8 consecutive
//    channels, 16-byte stores into the destination channel slice), so the ring never stops for
//    LDS staging;
//  * counted vmcnt waits: the loads younger than the awaited stage are the next stages and, right
//    after a tile boundary, the previous tile's stores (their number is known per step).
// WS > 0: weight-stationary 1x1 form — the layer's whole weight matrix (cout <= BN, K <= WS steps)
// is DMA'd into LDS once per block and every tile's K steps read it from there, so only the
// activation tile streams (a third of the DMA issue of the 256 x 256 ring); bias in registers.
// HOOK (scripts/convbench.hip only, 256 x 256 form; the ABI never accepts them): 296 activation without
// stores, 297 neither, 298 no operand DMA.  Compile-time: a runtime test in the K loop splits the DMA
// issue into a block of its own on every K step of the production kernel.
template <int BM, int BN, int WM, int WN, int STAGES, bool ONE, int ACT, int BK, int WS = 0, int HOOK = 0>
__global__ __launch_bounds__(64 * WM * WN, (STAGES * (BM + BN) * BK * 2 <= 48 * 1024 && WM * WN == 4) ? 3 : (STAGES * (BM + BN) * BK * 2 <= 76 * 1024) ? 2 : 1) void conv_f16_pring_kernel(
    const ConvParams p) {
  constexpr int NW = WM * WN, NTH = 64 * NW;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int RB_ = BK * 2;              // LDS bytes per tile row
  constexpr int CPR = RB_ / 16;            // 16-byte chunks per row
  constexpr int RPI = 64 / CPR;            // tile rows per DMA wave-instruction (1 KiB)
  constexpr int RA = BM / RPI / NW, RB = BN / RPI / NW;
  static_assert(RA * RPI * NW == BM && RB * RPI * NW == BN, "tile rows must split into DMA groups per wave");
  static_assert(TN % 2 == 0, "the epilogue pairs 16-channel groups");
  static_assert(STAGES >= 2 && STAGES <= 4, "counted waits cover up to two stages in flight");
  static_assert(WS == 0 || ONE, "weight-stationary form: 1x1 convs only");
  constexpr int PER = RA + (WS ? 0 : RB);
  constexpr int NST = TM * TN / 2;   // epilogue stores per lane per tile
  constexpr int STAGE = (BM + (WS ? 0 : BN)) * RB_;
  constexpr int WREG = WS ? BN * WS * RB_ : 0;   // stationary weights: [K step][BN rows][RB_]
  constexpr int BIAS = WS ? 0 : 4096;            // bias vector (<= 1024 channels) behind the ring
  __shared__ __attribute__((aligned(16))) unsigned char smem[STAGES * STAGE + WREG + BIAS];
  float* bias_l = reinterpret_cast<float*>(smem + STAGES * STAGE + WREG);
  unsigned char* wl = smem + STAGES * STAGE;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int g = lane >> 4, li = lane & 15;
  const int lr = lane / CPR;                          // row within the DMA group
  const int c = swz_bk<BK>(lr, lane % CPR);           // source chunk this lane fetches (slot = lane % CPR)

  const int nN = (p.cout + BN - 1) / BN;
  const int nk = p.kpad / BK;
  // N-split weight-stationary form (WS with cout > BN): block b holds output-channel tile nb's weights
  // and walks the M tiles only; the nN blocks of one virtual block share an XCD and walk the same M
  // tiles in the same order, so each activation tile comes from HBM once and from that XCD's L2 for
  // the other N tiles.  The launcher sizes the grid to a multiple of 8 nN.
  const bool nsplit = WS != 0 && nN > 1;
  const int nb = nsplit ? (int)((blockIdx.x / 8) % nN) : 0;
  const int T = nsplit ? (p.M + BM - 1) / BM : ((p.M + BM - 1) / BM) * nN;
  const TileWalk tw = nsplit ? xcd_tile_walk_g(T, gridDim.x / nN, (int)((blockIdx.x / (8 * nN)) * 8 + blockIdx.x % 8))
                             : xcd_tile_walk(T);   // XCD-major persistent tile order
  const int ntl = tw.count();
  if (ntl == 0) return;
  const int nsteps = ntl * nk;
  auto tile_m0 = [&](int t) { return nsplit ? t * BM : (t / nN) * BM; };
  auto tile_n0 = [&](int t) { return nsplit ? nb * BN : (t % nN) * BN; };

  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.w, p.wbytes);
  const auto yr = make_rsrc(p.y, 0x7fffffffu);

  float bias_r[WS ? TN : 1][4];
  if constexpr (WS == 0) {
    for (int i = tid; i < p.cout; i += NTH) bias_l[i] = p.bias[i];
  } else {
    // (one N tile per block: cn0 = nb * BN) this lane's channels, and the tile's weights into LDS once
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = nb * BN + wn * WTN + j * 16 + g * 4 + e;
        bias_r[j][e] = col < p.cout ? p.bias[col] : 0.0f;
      }
    constexpr int GPS = BN / RPI;   // DMA groups per K step
    for (int q = wave; q < nk * GPS; q += NW) {
      const int ks = q / GPS, rg = q - ks * GPS;
      dma16(wr, wl + (ks * BN + rg * RPI) * RB_, (uint32_t)(((nb * BN + rg * RPI + lr) * p.kpad + c * 8) * 2),
            (uint32_t)ks * BK * 2);
    }
  }

  // ---- issue cursor: global step ig = (local tile it, step ikt)
  AWalk<ONE, RA, BK> aw;
  uint32_t b_off[RB];
  int ig = 0, it = 0, ikt = 0;
  auto issue_next = [&]() __attribute__((always_inline)) {
    if (ikt == 0) {
      const int t = tw.at(it);
      const int m0 = tile_m0(t), n0 = tile_n0(t);
      aw.init(p, c, 0);
      PixelWalk pw(p, m0 + wave * RPI + lr);
#pragma unroll
      for (int j = 0; j < RA; ++j) {
        if (j) pw.advance(p, NW * RPI);
        aw.off[j] = a_origin(p, pw.b, pw.ho, pw.wo, c);
      }
#pragma unroll
      for (int j = 0; j < RB; ++j) b_off[j] = (uint32_t)(((n0 + (j * NW + wave) * RPI + lr) * p.kpad + c * 8) * 2);
    }
    const int slot = ig % STAGES;
    unsigned char* As = smem + slot * STAGE;
    unsigned char* Bs = As + BM * RB_;
    if constexpr (HOOK != 298) {   // 298: microbenchmark hook, no operand traffic (times the rest)
      aw.step(p, ikt, [&](int j, uint32_t vo, uint32_t so) { dma16(xr, As + (j * NW + wave) * RPI * RB_, vo, so); });
      if constexpr (WS == 0) {
#pragma unroll
        for (int j = 0; j < RB; ++j) dma16(wr, Bs + (j * NW + wave) * RPI * RB_, b_off[j], (uint32_t)ikt * BK * 2);
      }
    }
    ++ig;
    if (++ikt == nk) { ikt = 0; ++it; }
  };

  // ---- compute cursor
  f4 acc[TN][TM];
  int cm0 = 0, cn0 = 0;
  auto init_tile = [&](int i) __attribute__((always_inline)) {
    const int t = tw.at(i);
    cm0 = tile_m0(t);
    cn0 = tile_n0(t);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = cn0 + wn * WTN + j * 16 + g * 4;
      f4 bv;
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = WS ? bias_r[WS ? j : 0][e] : (col + e < p.cout ? bias_l[col + e] : 0.0f);
#pragma unroll
      for (int ii = 0; ii < TM; ++ii) acc[j][ii] = bv;
    }
  };
  const uint32_t lane_ch = (uint32_t)(16 * (g & 1) + 8 * (g >> 1));
  auto epilogue = [&]() __attribute__((always_inline)) {
    // the accumulators are final only here: without this the compiler speculates the activation's
    // first instructions (scale, v_exp) for every accumulator into every K step, ahead of the
    // tile-end branch (~20 VALU per step on the 128 x 128 ring)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int ii = 0; ii < TM; ++ii) asm volatile("" : "+v"(acc[j][ii]));
    if constexpr (HOOK == 296 || HOOK == 297) {   // microbenchmark hooks: 296 activation, no stores; 297 neither
      float sink = 0.0f;
#pragma unroll
      for (int ii = 0; ii < TM; ++ii)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) sink += HOOK == 297 ? acc[j][ii][e] : act_t<ACT>(acc[j][ii][e]);
      if (sink == 12345.0f) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, sink), yr, 0, 0, 0);
      return;
    }
    PixelWalk pw(p, cm0 + wm * WTM + li);
#pragma unroll
    for (int ii = 0; ii < TM; ++ii) {
      if (ii) pw.advance(p, 16);
      const int m = cm0 + wm * WTM + ii * 16 + li;
      const uint32_t yo = (uint32_t)((pix_index(pw.b, pw.ho, pw.wo, p.Ho, p.Wo) * p.yc + p.yoff) * 2);
#pragma unroll
      for (int mp = 0; mp < TN / 2; ++mp) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
        h4 va, vb;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          va[e] = (_Float16)act_t<ACT>(acc[2 * mp][ii][e]);
          vb[e] = (_Float16)act_t<ACT>(acc[2 * mp + 1][ii][e]);
        }
        const u2 a = __builtin_bit_cast(u2, va), b = __builtin_bit_cast(u2, vb);
        const auto s0 = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
        const u4 v = {s0[0], s1[0], s0[1], s1[1]};
        const int n = cn0 + wn * WTN + mp * 32 + (int)lane_ch;
        // rows past M / channels past cout: an offset beyond the buffer drops the store
        const uint32_t off = (m < p.M && n < p.cout) ? yo + (uint32_t)n * 2 : 0xffffffffu;
        __builtin_amdgcn_raw_buffer_store_b128(v, yr, off, 0, 0);
      }
    }
  };

#pragma unroll
  for (int s0 = 0; s0 < STAGES - 1; ++s0)
    if (ig < nsteps) issue_next();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // bias_l writes of this wave
  __builtin_amdgcn_s_barrier();
  init_tile(0);

  int ci = 0, ckt = 0;
  // One K step; SLOT = gs % STAGES as a compile-time constant (the loop below is unrolled by STAGES),
  // so every fragment read is a loop-invariant per-lane offset plus an immediate slot offset — no
  // address arithmetic per read and step.
  auto kstep = [&](int gs, auto slotc) __attribute__((always_inline)) {
    constexpr int SLOT = decltype(slotc)::value;   // -1: gs % STAGES at run time
    // stage gs has landed once at most `younger` vector-memory ops of this wave are outstanding
    const int ndma = min(STAGES - 2, nsteps - 1 - gs);
    const bool st = ci > 0 && ckt <= STAGES - 2;
    const int younger = ndma * PER + (st ? NST : 0);
    if (younger == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (younger == PER) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
    else if (younger == 2 * PER) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");
    else if (younger == NST) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NST) : "memory");
    else if (younger == PER + NST) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER + NST) : "memory");
    else if (younger == 2 * PER + NST) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER + NST) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (ig < nsteps) issue_next();   // refills the slot every wave finished reading at step gs-1
    const unsigned char* As = smem + (SLOT >= 0 ? SLOT : gs % STAGES) * STAGE;
    const unsigned char* Bs = WS ? wl + ckt * BN * RB_ : As + BM * RB_;
    // every fragment of the step is read up front: the second sub-step's reads are in flight under
    // the first sub-step's MFMAs
    constexpr int NSB = BK / 32;
    u4 xa[NSB][TM], wb[NSB][TN];
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb) {
      const int ch = sb * 4 + g;
#pragma unroll
      for (int ii = 0; ii < TM; ++ii) {
        const int row = wm * WTM + ii * 16 + li;
        xa[sb][ii] = *reinterpret_cast<const u4*>(As + row * RB_ + swz_bk<BK>(row, ch) * 16);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * WTN + j * 16 + li;
        wb[sb][j] = *reinterpret_cast<const u4*>(Bs + row * RB_ + swz_bk<BK>(row, ch) * 16);
      }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int sb = 0; sb < NSB; ++sb)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int ii = 0; ii < TM; ++ii)
          acc[j][ii] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wb[sb][j]),
                                                              __builtin_bit_cast(h8, xa[sb][ii]), acc[j][ii], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    if (++ckt == nk) {
      epilogue();
      ckt = 0;
      if (++ci < ntl) init_tile(ci);
    }
  };
  int gs = 0;
  // unrolled only where every slot offset fits a ds_read immediate (16 bits): the 64 KiB stages of the
  // 256 x 256 ring would need a second base register per slot and spill
  constexpr bool UNROLL = STAGES * STAGE <= 65536;
  if constexpr (!UNROLL) {
    for (; gs < nsteps; ++gs) kstep(gs, std::integral_constant<int, -1>{});
  }
  for (; UNROLL && gs + STAGES <= nsteps; gs += STAGES) {
    kstep(gs, std::integral_constant<int, 0>{});
    kstep(gs + 1, std::integral_constant<int, 1>{});
    if constexpr (STAGES > 2) kstep(gs + 2, std::integral_constant<int, (STAGES > 2 ? 2 : 0)>{});
    if constexpr (STAGES > 3) kstep(gs + 3, std::integral_constant<int, (STAGES > 3 ? 3 : 0)>{});
  }
  if constexpr (UNROLL) {
    if (gs < nsteps) kstep(gs++, std::integral_constant<int, 0>{});   // remainder: slots 0, 1, 2 in order
    if (STAGES > 2 && gs < nsteps) kstep(gs++, std::integral_constant<int, 1>{});
    if (STAGES > 3 && gs < nsteps) kstep(gs++, std::integral_constant<int, (STAGES > 3 ? 2 : 0)>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

hipError_t launch_pring(const ConvParams& p, int row, hipStream_t st) {
  const bool one = p.k == 1 && p.s == 1 && p.pad == 0;
  return launch_with_row<NPRING>(row, [&](auto I) {
    constexpr PringRow r = pring_rows[decltype(I)::value];
    constexpr int BM = r.bm, BN = r.bn;
    const dim3 block(64 * r.wm * r.wn);
    if constexpr (r.kind == PR_HOOK) {
      const long T = (long)((p.M + 255) / 256) * ((p.cout + 255) / 256);
      const int grid = (int)(T < (long)device_cus() ? T : (long)device_cus());
      if (one) YV7_LAUNCH((conv_f16_pring_kernel<BM, BN, r.wm, r.wn, r.stages, true, 1, 64, 0, r.hook>), dim3(grid), block, 0, st, p);
      else YV7_LAUNCH((conv_f16_pring_kernel<BM, BN, r.wm, r.wn, r.stages, false, 1, 64, 0, r.hook>), dim3(grid), block, 0, st, p);
      return hipGetLastError();
    } else if constexpr (r.kind == PR_WSN) {
      // the N-split weight-stationary 1x1 ring (cout > BN: block b holds N tile (b / 8) % nN; three stages)
      const int nN = (p.cout + BN - 1) / BN;
      if (nN < 2 || p.cout % 8 || p.yoff % 8 || p.yc % 8 || p.kpad > r.ws * 64 || p.k != 1 || p.s != 1 || p.pad)
        return hipErrorInvalidValue;
      const long T = (long)((p.M + BM - 1) / BM);
      long per = device_cus() / nN / 8 * 8;   // virtual blocks per N tile, a multiple of 8
      if (per > (T + 7) / 8 * 8) per = (T + 7) / 8 * 8;
      if (per < 8) per = 8;
      const int grid = (int)(per * nN);
      return launch_with_act(p.act, [&](auto A) {
        YV7_LAUNCH((conv_f16_pring_kernel<BM, BN, r.wm, r.wn, r.stages, true, decltype(A)::value, 64, r.ws>), dim3(grid), block, 0, st, p);
        return hipGetLastError();
      });
    } else if constexpr (r.kind == PR_WS) {
      // the weight-stationary 1x1 ring (one N tile, whole K in LDS)
      if (p.cout > BN || p.cout % 8 || p.yoff % 8 || p.yc % 8 || p.kpad > r.ws * 64 || p.k != 1 || p.s != 1 || p.pad)
        return hipErrorInvalidValue;
      const long T = (long)((p.M + BM - 1) / BM);
      const int grid = (int)(T < (long)device_cus() ? T : (long)device_cus());
      return launch_with_act(p.act, [&](auto A) {
        YV7_LAUNCH((conv_f16_pring_kernel<BM, BN, r.wm, r.wn, r.stages, true, decltype(A)::value, 64, r.ws>), dim3(grid), block, 0, st, p);
        return hipGetLastError();
      });
    } else {
      if (p.cout > 1024 || p.cout % 8 || p.yoff % 8 || p.yc % 8) return hipErrorInvalidValue;
      const long T = (long)((p.M + BM - 1) / BM) * ((p.cout + BN - 1) / BN);
      const int grid = (int)(T < (long)device_cus() * r.occ ? T : (long)device_cus() * r.occ);
      return launch_with_act(p.act, [&](auto A) {
        if (one) YV7_LAUNCH((conv_f16_pring_kernel<BM, BN, r.wm, r.wn, r.stages, true, decltype(A)::value, 64>), dim3(grid), block, 0, st, p);
        else YV7_LAUNCH((conv_f16_pring_kernel<BM, BN, r.wm, r.wn, r.stages, false, decltype(A)::value, 64>), dim3(grid), block, 0, st, p);
        return hipGetLastError();
      });
    }
  });
}

}  // namespace yv7
