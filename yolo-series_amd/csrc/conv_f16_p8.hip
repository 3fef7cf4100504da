// The two 8-phase persistent rings of the fp16 implicit-GEMM conv (conv_f16.hip describes the GEMM view):
// 256 x 256 tiles (conv_f16_p8_kernel) and 256 x 128 tiles (conv_f16_p8n_kernel).
#include "conv_f16_common.h"
#include "conv_f16_launch.h"

namespace yv7 {

namespace {

// 8-phase persistent ring (256 x 256 tiles, 8 waves = 2 stagger groups x 4, BK 64): the structure of
// the guide's 256^2 "8-phase" GEMM template (cdna_hip_programming.md §5: counted vmcnt across raw
// barriers, one half-tile of LDS-DMA per phase, two wave groups offset by one barrier so that one
// group's MFMA cluster runs while the other issues its LDS reads and DMA), rebuilt for the implicit
// GEMM of a conv and made persistent across output tiles like conv_f16_pring_kernel.
//
//  * LDS: two K-tile buffers, each four 16 KiB half-tiles [A0 A1 B0 B1] (A = 128 pixel rows,
//    B = 128 weight rows, 64 k each, XOR-swizzled 128-byte rows as everywhere here) + the bias.
//  * K-tile k runs four phases, one block quadrant (ha, hb) each in the order (0,0) (0,1) (1,1) (1,0):
//    every wave computes its 64 x 32 part of the quadrant (16 MFMAs), reading A half ha (8
//    ds_read_b128) and/or B half hb (4): phase 0 both, then B1, A1, B0 — so the halves' last reads
//    fall in phases 0 (A0), 1 (B1), 2 (A1), 3 (B0).
//  * every wave retires its phase's LDS reads (lgkmcnt(0)) before the phase's first barrier, so a
//    half can be restaged ONE phase after its last read even with the groups staggered (the other
//    group's DMA issue follows that barrier): phase 0 stages B0 of k+1, phase 1 A0 of k+2, phase 2
//    B1 of k+2, phase 3 A1 of k+2; the only wait is phase 3's vmcnt(6): K-tile k+1 retired, three
//    halves of k+2 still in flight, and the reads of k+1 start one phase (and so one more barrier of
//    the other group) later.
//  * the finished tile's epilogue (bias in the accumulators, activation, fp16, permlane16 pairing,
//    16-byte NHWC stores) runs between the last K-tile's phase 3 and the next tile's phase 0.
// acc[hb][j][ha][i] = channels hb*128 + wn*32 + j*16 + g*4 + e of pixel ha*128 + wm*64 + i*16 + li.
// Persistent tile order: XCD-major (xcd_tile_walk; 1x1 1024->1024 @40 140 -> 133 us, tune_ops).  The
// round-2 schedule experiments (DMA before the reads, no s_setprio, one group retiring early, B half 0
// kept in registers, stream-K, 512 x 128 tiles: DESIGN §4.5, §8) were removed in round 4.
template <bool ONE, int ACT, int BM = 256, int BN = 256>
__global__ __launch_bounds__(512, 1) void conv_f16_p8_kernel(const ConvParams p) {
  constexpr int NTH = 512;
  constexpr int AHR = BM / 2, BHR = BN / 2;          // rows per A / B half-tile
  constexpr int AHB = AHR * ROWB, BHB = BHR * ROWB;  // bytes per A / B half-tile
  constexpr int BUF = 2 * AHB + 2 * BHB;             // one K-tile: A0 A1 B0 B1
  constexpr int AP = AHR / 64, BP = BHR / 64;        // 1 KiB DMA pieces per wave per A / B half
  constexpr int VMC = 2 * AP + BP;                   // loads of three half-tiles (A0, B1, A1) per wave
  constexpr int WNC = BHR / 32;                      // waves across a B half (32 channels each)
  static_assert(AP >= 1 && BP >= 1 && (AHR / 64) * WNC == 8, "8 waves of 64 x 32 per block quadrant");
  constexpr int BIASB = (2 * BUF + 4096 + 16 <= 163840) ? 4096 : 0;   // bias in LDS when it fits
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF + BIASB];
  float* bias_l = reinterpret_cast<float*>(smem + 2 * BUF);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WNC, wn = wave % WNC;
  const int grp = wave >> 2;                         // stagger group (one wave of each per SIMD)
  const int g = lane >> 4, li = lane & 15;
  const int lr = lane >> 3;                          // DMA: row within an 8-row piece
  const int c = (lane & 7) ^ lr;                     // DMA: source chunk of slot lane & 7

  const int nN = (p.cout + BN - 1) / BN;
  const int T = ((p.M + BM - 1) / BM) * nN;
  const int nk = p.kpad / BKE;
  const TileWalk tw = xcd_tile_walk(T);
  const int ntl = tw.count();
  const int total = ntl * nk;                        // K-tiles this block computes
  if (total == 0) return;
  auto tile_at = [&](int it) { return tw.at(it); };

  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.w, p.wbytes);
  const auto yr = make_rsrc(p.y, 0x7fffffffu);
  if constexpr (BIASB != 0)
    for (int i = tid; i < p.cout; i += NTH) bias_l[i] = p.bias[i];

  // ---- staging cursors (A and B halves are staged in different phases, each in K-tile order)
  int a_it = 0, a_kt = 0, b_it = 0, b_kt = 0;
  uint32_t a_off[2][AP], b_off[2][BP], a_so = 0;
  KWalk sa, sb;   // (!ONE) the A and B halves' chunk-major K walks (staged in different phases)
  auto stage_a = [&](int h, int par) {   // half h (0 / 1) of the next A K-tile, into buffer par
    if (h == 0) {
      if (a_kt == 0) {
        const int t = tile_at(a_it);
        PixelWalk pw(p, (t / nN) * BM + wave * 8 + lr);
#pragma unroll
        for (int q = 0; q < 2 * AP; ++q) {
          if (q) pw.advance(p, 64);
          a_off[q / AP][q % AP] = a_origin(p, pw.b, pw.ho, pw.wo, c);
        }
        sa.init();
      }
      a_so = ONE ? (uint32_t)a_kt * BKE * 2 : sa.a_offset(p);
      if (!ONE) sa.advance(p);
    }
    unsigned char* d = smem + par * BUF + h * AHB;
#pragma unroll
    for (int j = 0; j < AP; ++j) dma16(xr, d + (j * 8 + wave) * 8 * ROWB, a_off[h][j], a_so);
    if (h == 1) {
      if (++a_kt == nk) { a_kt = 0; ++a_it; }
    }
  };
  uint32_t b_so = 0;
  auto stage_b = [&](int h, int par) {   // half h of the next B K-tile into buffer par; B1 first, then B0
    if (h == 1) {
      if (b_kt == 0) {
        const int n0 = tile_at(b_it) % nN * BN;
#pragma unroll
        for (int q = 0; q < 2 * BP; ++q)
          b_off[q / BP][q % BP] =
              (uint32_t)(((n0 + (q / BP) * BHR + ((q % BP) * 8 + wave) * 8 + lr) * p.kpad + c * 8) * 2);
        sb.init();
      }
      b_so = ONE ? (uint32_t)b_kt * BKE * 2 : sb.b_offset(p);
      if (!ONE) sb.advance(p);
    }
    unsigned char* d = smem + par * BUF + 2 * AHB + h * BHB;
#pragma unroll
    for (int j = 0; j < BP; ++j) dma16(wr, d + (j * 8 + wave) * 8 * ROWB, b_off[h][j], b_so);
    if (h == 0) {
      if (++b_kt == nk) { b_kt = 0; ++b_it; }
    }
  };

  // ---- compute side
  f4 acc[2][2][2][4];
  int cm0 = 0, cn0 = 0;
  auto init_tile = [&](int i) {
    const int t = tile_at(i);
    cm0 = (t / nN) * BM;
    cn0 = (t % nN) * BN;
#pragma unroll
    for (int hb = 0; hb < 2; ++hb)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = cn0 + hb * BHR + wn * 32 + j * 16 + g * 4;
        f4 bv;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          bv[e] = col + e < p.cout ? (BIASB ? bias_l[col + e] : p.bias[col + e]) : 0.0f;
#pragma unroll
        for (int ha = 0; ha < 2; ++ha)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[hb][j][ha][i] = bv;
      }
  };
  const uint32_t lane_ch = (uint32_t)(16 * (g & 1) + 8 * (g >> 1));
  auto epilogue = [&]() {
#pragma unroll
    for (int ha = 0; ha < 2; ++ha) {
      PixelWalk pw(p, cm0 + ha * AHR + wm * 64 + li);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i) pw.advance(p, 16);
        const int m = cm0 + ha * AHR + wm * 64 + i * 16 + li;
        const uint32_t yo = (uint32_t)((pix_index(pw.b, pw.ho, pw.wo, p.Ho, p.Wo) * p.yc + p.yoff) * 2);
#pragma unroll
        for (int hb = 0; hb < 2; ++hb) {
          typedef _Float16 h4 __attribute__((ext_vector_type(4)));
          typedef uint32_t u2 __attribute__((ext_vector_type(2)));
          h4 va, vb;
          const f4 a0 = acc[hb][0][ha][i], a1 = acc[hb][1][ha][i];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            va[e] = (_Float16)act_t<ACT>(a0[e]);
            vb[e] = (_Float16)act_t<ACT>(a1[e]);
          }
          const u2 a = __builtin_bit_cast(u2, va), b = __builtin_bit_cast(u2, vb);
          const auto s0 = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
          const u4 v = {s0[0], s1[0], s0[1], s1[1]};
          const int n = cn0 + hb * BHR + wn * 32 + (int)lane_ch;
          const uint32_t off = (m < p.M && n < p.cout) ? yo + (uint32_t)n * 2 : 0xffffffffu;
          __builtin_amdgcn_raw_buffer_store_b128(v, yr, off, 0, 0);
        }
      }
    }
  };

  // ---- prologue: K-tile 0 whole, K-tile 1's A0, B1 and A1 in flight
  stage_a(0, 0); stage_b(1, 0); stage_a(1, 0); stage_b(0, 0);
  if (total > 1) {
    stage_a(0, 1); stage_b(1, 1); stage_a(1, 1);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // bias_l
  __builtin_amdgcn_s_barrier();
  int ci = 0, ckt = 0;   // compute cursor: tile, K step
  init_tile(ci);
  if (grp == 1) __builtin_amdgcn_s_barrier();   // group 1 runs one barrier behind group 0

  u4 xa[2][4], wb[2][2];
  auto read_a = [&](const unsigned char* h) {
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wm * 64 + i * 16 + li;
        xa[sb][i] = *reinterpret_cast<const u4*>(h + row * ROWB + swz(row, sb * 4 + g) * 16);
      }
  };
  auto read_b = [&](const unsigned char* h) {
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = wn * 32 + j * 16 + li;
        wb[sb][j] = *reinterpret_cast<const u4*>(h + row * ROWB + swz(row, sb * 4 + g) * 16);
      }
  };
  auto mfma_q = [&](int ha, int hb) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this phase's reads retired (WAR: see above)
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          acc[hb][j][ha][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wb[sb][j]),
                                                                     __builtin_bit_cast(h8, xa[sb][i]),
                                                                     acc[hb][j][ha][i], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();
  };

  // one K-tile: four phases over buffer par (K-tile k + 1's B0 and K-tile k + 2's A0, B1, A1 staged on
  // the way when n1 / n2)
  auto ktile = [&](auto par, bool n1, bool n2) __attribute__((always_inline)) {
    const int P = par;   // a compile-time constant (integral_constant) or the K-tile's parity
    const unsigned char* bk = smem + P * BUF;
    // phase 0: quadrant (0,0)
    read_b(bk + 2 * AHB);
    read_a(bk);
    if (n1) stage_b(0, P ^ 1);
    mfma_q(0, 0);
    // phase 1: (0,1)
    read_b(bk + 2 * AHB + BHB);
    if (n2) stage_a(0, P);
    mfma_q(0, 1);
    // phase 2: (1,1)
    read_a(bk + AHB);
    if (n2) stage_b(1, P);
    mfma_q(1, 1);
    // phase 3: (1,0); K-tile k+1 retired (k+2's A0, B1 and A1 may stay in flight)
    read_b(bk + 2 * AHB);
    if (n2) {
      stage_a(1, P);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    mfma_q(1, 0);
  };
  // (ONE, nk even) the staging without cursors: the A / B halves' offsets for tile t (fresh_*), and one
  // half's LDS-DMA at K offset so into buffer par
  auto fresh_a = [&](int t) __attribute__((always_inline)) {
    PixelWalk pw(p, (t / nN) * BM + wave * 8 + lr);
#pragma unroll
    for (int q = 0; q < 2 * AP; ++q) {
      if (q) pw.advance(p, 64);
      a_off[q / AP][q % AP] = a_origin(p, pw.b, pw.ho, pw.wo, c);
    }
  };
  auto fresh_b = [&](int t) __attribute__((always_inline)) {
    const int n0 = t % nN * BN;
#pragma unroll
    for (int q = 0; q < 2 * BP; ++q)
      b_off[q / BP][q % BP] = (uint32_t)(((n0 + (q / BP) * BHR + ((q % BP) * 8 + wave) * 8 + lr) * p.kpad + c * 8) * 2);
  };
  auto dma_a = [&](int h, int par, uint32_t so) __attribute__((always_inline)) {
    unsigned char* d = smem + par * BUF + h * AHB;
#pragma unroll
    for (int j = 0; j < AP; ++j) dma16(xr, d + (j * 8 + wave) * 8 * ROWB, a_off[h][j], so);
  };
  auto dma_b = [&](int h, int par, uint32_t so) __attribute__((always_inline)) {
    unsigned char* d = smem + par * BUF + 2 * AHB + h * BHB;
#pragma unroll
    for (int j = 0; j < BP; ++j) dma16(wr, d + (j * 8 + wave) * 8 * ROWB, b_off[h][j], so);
  };
  // the same four phases, staging K-tile k + 1's B0 at so1 and K-tile k + 2's A0, B1, A1 at so2 (of tile t2,
  // whose offsets are computed first when fresh2)
  auto ktile_one = [&](auto par, bool n1, bool n2, uint32_t so1, uint32_t so2, bool fresh2, int t2)
      __attribute__((always_inline)) {
    constexpr int P = decltype(par)::value;
    const unsigned char* bk = smem + P * BUF;
    read_b(bk + 2 * AHB);
    read_a(bk);
    if (n1) dma_b(0, P ^ 1, so1);
    mfma_q(0, 0);
    read_b(bk + 2 * AHB + BHB);
    if (n2) {
      if (fresh2) fresh_a(t2);
      dma_a(0, P, so2);
    }
    mfma_q(0, 1);
    read_a(bk + AHB);
    if (n2) {
      if (fresh2) fresh_b(t2);
      dma_b(1, P, so2);
    }
    mfma_q(1, 1);
    read_b(bk + 2 * AHB);
    if (n2) {
      dma_a(1, P, so2);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    mfma_q(1, 0);
  };
  if (ONE && (nk & 1) == 0) {
    // 1x1, nk even: the staging cursors follow from the compute cursor.  The pair (ckt, ckt + 1) stages
    // K-tiles ckt + 1 .. ckt + 3; only ckt + 2 == nk moves the staging to the next tile, and then K-tile
    // k + 2 (the even K-tile's A0 / B1 / A1) is that tile's first: its offsets are computed there, once.
    for (int k = 0; k < total; k += 2) {
      const bool more = k + 2 < total;
      const bool wrap = ckt + 2 == nk;
      const uint32_t s2 = wrap ? 0u : (uint32_t)(ckt + 2) * BKE * 2;
      ktile_one(std::integral_constant<int, 0>{}, true, more, (uint32_t)(ckt + 1) * BKE * 2, s2, wrap,
                wrap && more ? tile_at(ci + 1) : 0);
      ktile_one(std::integral_constant<int, 1>{}, more, more, s2, s2 + BKE * 2, false, 0);
      ckt += 2;
      if (ckt == nk) {
        epilogue();
        if (more) {
          ckt = 0;
          init_tile(++ci);
        }
      }
    }
  } else if ((nk & 1) == 0) {
    // nk even (round 6): every tile starts on an even K-tile, so two K-tiles per trip give each phase its
    // buffer as a compile-time constant (the LDS read bases and DMA destinations are loop-invariant
    // instead of recomputed from the K-tile's parity every phase), and only the odd K-tile can end a tile.
    // total is even: n1 holds for the even K-tile, and k + 2 < total stands for the rest.
    for (int k = 0; k < total; k += 2) {
      const bool more = k + 2 < total;
      ktile(std::integral_constant<int, 0>{}, true, more);
      ktile(std::integral_constant<int, 1>{}, more, more);
      ckt += 2;
      if (ckt == nk) {
        epilogue();
        if (more) {
          ckt = 0;
          init_tile(++ci);
        }
      }
    }
  } else {
    for (int k = 0; k < total; ++k) {
      ktile(k & 1, k + 1 < total, k + 2 < total);
      if (++ckt == nk) {
        epilogue();
        if (k != total - 1) {
          ckt = 0;
          init_tile(++ci);
        }
      }
    }
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();   // equal barrier counts in both groups
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// 8-phase-style persistent ring for 256 x 128 tiles (128-channel outputs, and 256-channel layers
// with too few 256 x 256 tiles): 8 waves in two stagger groups as in conv_f16_p8_kernel, but with
// three K-tile buffers of 48 KiB [A0 A1 B0 B1] (A halves 128 pixel rows, B halves 64 weight rows),
// two phases per K-tile (phase h: A half h x the whole B tile, 16 MFMAs per wave on its 32 x 64
// part), K-tile k+2 staged during K-tile k (A_h + B_h in phase h) into the buffer K-tile k-1 left,
// and one counted vmcnt(6) per K-tile that retires K-tile k+1.
// acc[h][j][i] = channels wn*64 + j*16 + g*4 + e of pixel h*128 + wm*32 + i*16 + li.
template <bool ONE, int ACT>
__global__ __launch_bounds__(512, 1) void conv_f16_p8n_kernel(const ConvParams p) {
  constexpr int BM = 256, BN = 128, NTH = 512;
  constexpr int AH = 128 * 128, BH = 64 * 128;
  constexpr int BUF = 2 * AH + 2 * BH;
  __shared__ __attribute__((aligned(16))) unsigned char smem[3 * BUF + 4096];
  float* bias_l = reinterpret_cast<float*>(smem + 3 * BUF);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wave >> 2;                         // stagger group (one wave of each per SIMD)
  const int wm = wave >> 1, wn = wave & 1;
  const int g = lane >> 4, li = lane & 15;
  const int lr = lane >> 3;
  const int c = (lane & 7) ^ lr;

  const int nN = (p.cout + BN - 1) / BN;
  const int T = ((p.M + BM - 1) / BM) * nN;
  const int nk = p.kpad / BKE;
  // XCD-major tile order (round 5): the nN tiles of one pixel block run on one XCD and share its input
  // rows in that L2 (round robin put them on nN different XCDs)
  const TileWalk tw = xcd_tile_walk(T);
  const int ntl = tw.count();
  const int total = ntl * nk;
  if (total == 0) return;

  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.w, p.wbytes);
  const auto yr = make_rsrc(p.y, 0x7fffffffu);
  for (int i = tid; i < p.cout; i += NTH) bias_l[i] = p.bias[i];

  // ---- staging cursor: K-tile s_gk, half h = A half h + B half h
  int s_it = 0, s_kt = 0;
  uint32_t a_off[2][2], b_off[2], a_so = 0, b_so = 0;
  KWalk su;
  auto stage = [&](int h, int par) {   // half h of the next K-tile into buffer par
    if (h == 0) {
      if (s_kt == 0) {
        const int t = tw.at(s_it);
        PixelWalk pw(p, (t / nN) * BM + wave * 8 + lr);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q) pw.advance(p, 64);
          a_off[q >> 1][q & 1] = a_origin(p, pw.b, pw.ho, pw.wo, c);
        }
        const int n0 = t % nN * BN;
#pragma unroll
        for (int q = 0; q < 2; ++q) b_off[q] = (uint32_t)(((n0 + q * 64 + wave * 8 + lr) * p.kpad + c * 8) * 2);
        su.init();
      }
      a_so = ONE ? (uint32_t)s_kt * BKE * 2 : su.a_offset(p);
      b_so = ONE ? (uint32_t)s_kt * BKE * 2 : su.b_offset(p);
      if (!ONE) su.advance(p);
    }
    unsigned char* d = smem + par * BUF;
#pragma unroll
    for (int j = 0; j < 2; ++j) dma16(xr, d + h * AH + (j * 8 + wave) * 8 * ROWB, a_off[h][j], a_so);
    dma16(wr, d + 2 * AH + h * BH + wave * 8 * ROWB, b_off[h], b_so);
    if (h == 1) {
      if (++s_kt == nk) { s_kt = 0; ++s_it; }
    }
  };

  f4 acc[2][4][2];
  int cm0 = 0, cn0 = 0;
  auto init_tile = [&](int i) {
    const int t = tw.at(i);
    cm0 = (t / nN) * BM;
    cn0 = (t % nN) * BN;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = cn0 + wn * 64 + j * 16 + g * 4;
      f4 bv;
#pragma unroll
      for (int e = 0; e < 4; ++e) bv[e] = col + e < p.cout ? bias_l[col + e] : 0.0f;
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[h][j][i] = bv;
    }
  };
  const uint32_t lane_ch = (uint32_t)(16 * (g & 1) + 8 * (g >> 1));
  auto epilogue = [&]() {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      PixelWalk pw(p, cm0 + h * 128 + wm * 32 + li);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (i) pw.advance(p, 16);
        const int m = cm0 + h * 128 + wm * 32 + i * 16 + li;
        const uint32_t yo = (uint32_t)((pix_index(pw.b, pw.ho, pw.wo, p.Ho, p.Wo) * p.yc + p.yoff) * 2);
#pragma unroll
        for (int mp = 0; mp < 2; ++mp) {
          typedef _Float16 h4 __attribute__((ext_vector_type(4)));
          typedef uint32_t u2 __attribute__((ext_vector_type(2)));
          h4 va, vb;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            va[e] = (_Float16)act_t<ACT>(acc[h][2 * mp][i][e]);
            vb[e] = (_Float16)act_t<ACT>(acc[h][2 * mp + 1][i][e]);
          }
          const u2 a = __builtin_bit_cast(u2, va), b = __builtin_bit_cast(u2, vb);
          const auto s0 = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
          const u4 v = {s0[0], s1[0], s0[1], s1[1]};
          const int n = cn0 + wn * 64 + mp * 32 + (int)lane_ch;
          const uint32_t off = (m < p.M && n < p.cout) ? yo + (uint32_t)n * 2 : 0xffffffffu;
          __builtin_amdgcn_raw_buffer_store_b128(v, yr, off, 0, 0);
        }
      }
    }
  };

  // ---- prologue: K-tiles 0 and 1 staged, 0 retired
  stage(0, 0); stage(1, 0);
  if (total > 1) {
    stage(0, 1); stage(1, 1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  init_tile(0);
  if (grp == 1) __builtin_amdgcn_s_barrier();

  u4 xa[2][2], wb[2][4];
  auto mfma_h = [&](int h) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
          acc[h][j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wb[sb][j]),
                                                                __builtin_bit_cast(h8, xa[sb][i]), acc[h][j][i], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_barrier();
  };
  auto read_a = [&](const unsigned char* ah) {
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wm * 32 + i * 16 + li;
        xa[sb][i] = *reinterpret_cast<const u4*>(ah + row * ROWB + swz(row, sb * 4 + g) * 16);
      }
  };

  // one K-tile over buffer par (K-tile k + 2 staged on the way into buffer (par + 2) % 3 when n2)
  auto ktile = [&](auto par, bool n2) __attribute__((always_inline)) {
    const int P = par;   // a compile-time constant (integral_constant) or k % 3
    const unsigned char* bk = smem + P * BUF;
    const int P2 = P == 0 ? 2 : P - 1;
    // phase 0: the wave's whole B part (kept for phase 1) + A half 0
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = j * 16 + li;   // within B half wn
        wb[sb][j] = *reinterpret_cast<const u4*>(bk + 2 * AH + wn * BH + row * ROWB + swz(row, sb * 4 + g) * 16);
      }
    read_a(bk);
    if (n2) stage(0, P2);
    mfma_h(0);
    // phase 1: A half 1; K-tile k+1 retired (k+2 may stay in flight)
    read_a(bk + AH);
    if (n2) {
      stage(1, P2);
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    mfma_h(1);
  };
  int ci = 0, ckt = 0;
  if (nk % 3 == 0) {
    // nk a multiple of 3 (every 3x3 layer here: nk = 9 cin / 64; round 6): every tile starts on a K-tile
    // k = 0 mod 3, so three K-tiles per trip give each its buffer as a compile-time constant, and only the
    // third can end a tile
    for (int k = 0; k < total; k += 3) {
      ktile(std::integral_constant<int, 0>{}, k + 2 < total);
      ktile(std::integral_constant<int, 1>{}, k + 3 < total);
      ktile(std::integral_constant<int, 2>{}, k + 4 < total);
      ckt += 3;
      if (ckt == nk) {
        epilogue();
        ckt = 0;
        if (++ci < ntl) init_tile(ci);
      }
    }
  } else {
    for (int k = 0; k < total; ++k) {
      ktile(k % 3, k + 2 < total);
      if (++ckt == nk) {
        epilogue();
        ckt = 0;
        if (++ci < ntl) init_tile(ci);
      }
    }
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

hipError_t launch_p8(const ConvParams& p, int cfg, hipStream_t st) {
  const bool one = p.k == 1 && p.s == 1 && p.pad == 0;
  if (cfg != P8_256x256 && cfg != P8_256x128) return hipErrorInvalidValue;
  if (p.cout > 1024 || p.cout % 8 || p.yoff % 8 || p.yc % 8 || (!one && p.cin % BKE)) return hipErrorInvalidValue;
  const int bn = cfg == P8_256x256 ? 256 : 128;
  const long T = (long)((p.M + 255) / 256) * ((p.cout + bn - 1) / bn);
  const int cus = device_cus();
  const int grid = (int)(T < (long)cus ? T : (long)cus);
  return launch_with_act(p.act, [&](auto A) {
    constexpr int ACT = decltype(A)::value;
    if (cfg == P8_256x256) {
      if (one) YV7_LAUNCH((conv_f16_p8_kernel<true, ACT>), dim3(grid), dim3(512), 0, st, p);
      else YV7_LAUNCH((conv_f16_p8_kernel<false, ACT>), dim3(grid), dim3(512), 0, st, p);
    } else {
      if (one) YV7_LAUNCH((conv_f16_p8n_kernel<true, ACT>), dim3(grid), dim3(512), 0, st, p);
      else YV7_LAUNCH((conv_f16_p8n_kernel<false, ACT>), dim3(grid), dim3(512), 0, st, p);
    }
    return hipGetLastError();
  });
}

}  // namespace yv7
