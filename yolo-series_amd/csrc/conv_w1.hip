// 1x1 / stride-1 fp16 convolution with the layer's WEIGHTS RESIDENT IN VGPRs — the short-K pointwise
// convs of the ELAN stacks whose cin is 128, 256 or 512 (Conv(c1, c2, 1, 1) in Conv.fuseforward,
// models/common.py:110-111; cfg/deploy/yolov7.yaml:22-23, 30, 35-36, ...: 128->128 / 256->256 @160,
// 256->256 / 512->128 / 512->256 @80 at bs 32).  y = act(x W'^T + b').
//
// Why (round 5): these layers are HBM-bound (1x1 256->256 @160 moves 838 MB for 107 GFLOP) but ran at
// 0.54-0.59 of their HBM roof on the LDS-DMA rings, which re-stage a weight tile for every output tile
// (as many L2 -> LDS bytes as the activations) and run the tile epilogue (the SiLU of every output, about
// the MFMA time at K = 256) with every wave of the block at once.  Here, as in conv_s2.hip:
//  * the block's N slice of the weights lives in VGPRs for the whole persistent launch (wave (ng, pg)
//    keeps TN x NCH fragments of 16 channels x 32 K, <= 128 VGPRs), loaded once from the fragment-packed
//    copy (pack_frag, 1 tap);
//  * activations stream: a tile is TPX = PG x TPF x 16 consecutive output pixels, its input rows DMA'd
//    (buffer_load ... lds, 8 whole 128-byte lines per piece = one 64-channel chunk of 8 pixels) into an
//    NS-slot LDS ring one chunk per interval, issued spread over the interval's K steps, L = NS - 1 - STG
//    chunks ahead; every pixel-fragment read feeds TN MFMAs (K 256: 4, 0.25 reads per MFMA);
//  * a pixel's 128 bytes are 8 16-byte positions, K-step half h's part g at (4 h + g) ^ ((px >> 1) & 7):
//    conflict-free ds_read_b128 for the MFMA B operand (16 consecutive pixels; checked against the gfx950
//    lane groups, scripts/w1_swizzle_check.py); the swizzle is on the DMA's per-lane source address;
//  * STG > 0: waves 4-7 run STG intervals behind waves 0-3 (a SIMD hosts w and w + 4), so one group's
//    tile epilogue issues beside the other group's MFMAs.
// Pixel m -> bordered NHWC index: m + 2 r + (2 b + 1)(W + 2) + 1, r = m / W, b = r / H.  Only the tile's
// first pixel m0 is decomposed, once per tile and wave-uniform (Div24 multiply-highs, scalar unit); a lane's
// pixel m0 + off then lies floor((c0 + off) / W) rows on (c0 = m0's column) and past the image's last row
// iff off >= (H - h0) W - c0, so its index is base(m0) + off + 2 [off >= W - c0] + 2 [off >= 2 W - c0] +
// 2 (W + 2) [next image]: compares of the lane's launch-invariant offset against per-tile scalars, no
// division and no multiply per lane.  That needs a tile to wrap at most NWR = 2 rows (TPX - 2 < 2 W) and
// one image (H >= 2); narrower tensors keep the per-lane decomposition bpix() (float reciprocal with an
// exact integer correction; M < 2^24).
#include "yv7_kernels.h"

namespace yv7 {

namespace {

constexpr int DC = 64;          // channels per DMA chunk (one 128-byte line per pixel; two MFMA K steps)
constexpr int NWR = 2;          // row wraps inside a tile the stepped index covers

// bordered pixel index of output pixel m (H, W: the tensor's interior size; rW = 1 / W, rH = 1 / H)
__device__ __forceinline__ uint32_t bpix(int m, int H, int W, float rW, float rH) {
  int r = (int)((float)m * rW);
  if ((r + 1) * W <= m) ++r;
  if (r * W > m) --r;
  int b = (int)((float)r * rH);
  if ((b + 1) * H <= r) ++b;
  if (b * H > r) --b;
  return (uint32_t)(m + 2 * r + (2 * b + 1) * (W + 2) + 1);
}

// Wave-uniform decomposition of a tile's first pixel m0: idx = its bordered index; offsets off >= t1 + w W
// (w = 0 .. NWR - 1) are w + 1 rows on, offsets >= tb in the next image, offsets >= rem past the tensor.
struct TileBase {
  uint32_t idx;
  int t1, tb, rem;
};
__device__ __forceinline__ TileBase tile_base(int m0, const ConvParams& p) {
  const int R0 = div24(m0, p.d0), c0 = m0 - R0 * p.Wo;
  const int b0 = div24(R0, p.d1), h0 = R0 - b0 * p.Ho;
  return TileBase{(uint32_t)(m0 + 2 * R0 + (2 * b0 + 1) * (p.Wo + 2) + 1), p.Wo - c0, (p.Ho - h0) * p.Wo - c0,
                  p.M - m0};
}
// Byte offset of the lane's pixel at tile offset lo + ok (lo: the lane's part, ok: wave-uniform) given the
// offset `s` of the same pixel were it on the tile's first row: + row2 per wrapped row (2 border pixels),
// + img2 into the next image (2 border rows); OOB past the tensor.
__device__ __forceinline__ uint32_t step_pix(uint32_t s, int lo, int ok, const TileBase& tb, int W, uint32_t row2,
                                             uint32_t img2) {
#pragma unroll
  for (int w = 0; w < NWR; ++w) s += lo >= tb.t1 + w * W - ok ? row2 : 0u;
  s += lo >= tb.tb - ok ? img2 : 0u;
  return lo < tb.rem - ok ? s : OOB;
}

template <int NCH, int TN, int TPF, int PG, int NG, int NS, int STG, int IC>
struct W1Geo {
  static_assert(NG * PG == 8, "eight waves");
  static_assert(NCH % 2 == 0 && TN * NCH <= 32, "whole DMA chunks, <= 128 weight VGPRs");
  static constexpr int NDC = NCH / 2;            // DMA chunks per tile
  static_assert(NDC % IC == 0, "whole intervals per tile");
  static constexpr int NIV = NDC / IC;           // intervals per tile
  static constexpr int TPX = PG * TPF * 16;      // pixels per tile
  static_assert((IC * TPX) % 64 == 0, "whole DMA pieces per wave");
  static constexpr int PPC = TPX / 8;            // 1 KiB pieces per chunk (8 pixels each)
  static constexpr int PW = IC * TPX / 64;       // pieces per wave per interval
  static constexpr int SB = IC * TPX * 128;      // bytes per ring slot (IC chunks, chunk-major)
  static_assert(NS * SB + NG * TN * 64 <= 160 * 1024, "LDS budget");
  static constexpr int L = NS - 1 - STG;         // DMA lead in intervals
  static_assert(L >= 1 && L <= 8 && STG >= 0 && STG <= 3, "lead, stagger");
  static constexpr int BN = NG * TN * 16;
  static constexpr int NST = TN % 2 == 0 ? TPF * TN / 2 : TPF * TN;   // epilogue stores per wave per tile
};

// wave = pg * NG + ng; group = wave >> 2.  Tile = TPX consecutive output pixels x the block's BN channels;
// an interval (one barrier) covers IC DMA chunks (IC = NDC: the whole tile, so a stagger of one interval
// puts one group's tile epilogue beside the other group's whole tile of MFMAs).
// HOOK (convbench only, variants 299-301 on cfg 1; the ABI never accepts them): 2 = no DMA, 3 = no
// epilogue (a store under a condition that never holds keeps the MFMAs), 4 = DMA, waits, barriers only.
template <int NCH, int TN, int TPF, int PG, int NG, int NS, int STG, int IC, int ACT, int HOOK = 0>
__global__ __launch_bounds__(512, 2) void conv1x1_rw_kernel(const ConvParams p, int nN) {
  using G = W1Geo<NCH, TN, TPF, PG, NG, NS, STG, IC>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * G::SB + G::BN * 4];
  float* bias_l = reinterpret_cast<float*>(smem + NS * G::SB);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ng = wave % NG, pg = wave / NG, grp = STG ? (wave >> 2) : 0;
  const int g = lane >> 4, li = lane & 15;

  const int b = blockIdx.x, Gd = gridDim.x;
  const int nt = (b / 8) % nN;
  const int vb = (b / (8 * nN)) * 8 + b % 8, vG = Gd / nN;
  const int T = (p.M + G::TPX - 1) / G::TPX;
  const TileWalk tw = xcd_tile_walk_g(T, vG, vb);
  const int ntl = tw.count();
  if (ntl == 0) return;   // (uniform over the block)
  const int n0 = nt * G::BN;
  const float rW = 1.0f / (float)p.Wo, rH = 1.0f / (float)p.Ho;

  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.wf, p.wfbytes);
  const auto yr = make_rsrc(p.y, 0x7fffffffu);

  // ---- resident weights: fragment (nf, K step c) at (nf * NCH + c) KiB, lane-linear
  u4 wreg[TN][NCH];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const uint32_t base = (uint32_t)((n0 / 16 + ng * TN + j) * NCH * 1024 + lane * 16);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      wreg[j][c] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(wr, base, (uint32_t)(c * 1024), 0));
  }
  // bias: the block's slice in LDS (re-read at every tile start rather than held in 4 TN VGPRs; a global
  // load there would sit behind the in-flight DMA in vmcnt order and drain the ring)
  for (int i = tid; i < G::BN; i += 512) bias_l[i] = n0 + i < p.cout ? p.bias[n0 + i] : 0.0f;
  f4 acc[TN][TPF];
  auto init_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const f4 bv = *reinterpret_cast<const f4*>(bias_l + ng * TN * 16 + j * 16 + g * 4);
#pragma unroll
      for (int f = 0; f < TPF; ++f) acc[j][f] = bv;
    }
  };

  // ---- DMA: interval v = (tile v / NIV, chunks (v % NIV) * IC ..); piece k = wave + 8 m of the interval:
  // chunk k / PPC, pixels 8 (k % PPC) .. + 7; lane -> pixel 8 (k % PPC) + lane / 8, LDS position lane % 8
  // = source part (lane % 8) ^ ((px >> 1) & 7) of the chunk's 128-byte line
  const uint32_t xoffb = (uint32_t)p.xoff * 2, pitch = (uint32_t)p.xc * 2;
  // stepped index (header): a tile wraps at most NWR rows and one image; launch-invariant
  // (TIGHT: two kinds of slice keep the per-lane decomposition and the per-store channel test.  Where the weights
  // and accumulators fill the register file, the lane's parts held across the tile loop would cost VGPRs those
  // configurations do not have (they spill); and the cin-512 slices, NCH 16, measured 3-5 % slower per launch
  // with the stepped index in the yolov7 bs-32 forward, profiles/addr_trim/README.md)
  constexpr bool TIGHT = TN * (NCH + TPF) * 4 >= 192 || NCH == 16;
  const bool stepped = !TIGHT && G::TPX - 2 < NWR * p.Wo && p.Ho >= NWR;
  uint32_t src[G::PW];   // per-lane source offsets of the tile's pieces (chunk within the interval folded in)
  // a piece's pixel offset is 8 (k % PPC) + lane / 8 with k % 2 = wave % 2 (PPC is even), so the swizzle term
  // (px >> 1) & 7 = 4 (wave & 1) | lane / 16 is the lane's for the whole launch
  const int lo8 = lane >> 3;
  const uint32_t dma_lane = (uint32_t)lo8 * pitch + (uint32_t)(((lane & 7) ^ (lane >> 4) ^ (4 * (wave & 1))) * 16);
  auto set_tile = [&](int it) __attribute__((always_inline)) {
    const int m0 = it < ntl ? tw.at(it) * G::TPX : p.M;
    if (stepped) {
      const TileBase tb = tile_base(m0, p);
      const uint32_t base = tb.idx * pitch + xoffb;
      // the wave's pieces k = wave + 8 mm cover only NPX different pixel groups k % PPC (PPC / 8 of them, or
      // one when PPC = 4), each in several chunks k / PPC: one stepped offset per group, + the chunk's
      constexpr int NPX = G::PPC >= 8 ? G::PPC / 8 : 1;
      static_assert(G::PPC % 8 == 0 || G::PPC == 4, "pixel groups of a wave's pieces");
      uint32_t pa[NPX];
#pragma unroll
      for (int j = 0; j < NPX; ++j) {
        const int ok = ((wave + 8 * j) % G::PPC) * 8;
        pa[j] = step_pix(dma_lane + (base + (uint32_t)ok * pitch), lo8, ok, tb, p.Wo, 2 * pitch,
                         2 * (uint32_t)(p.Wo + 2) * pitch);
      }
#pragma unroll
      for (int mm = 0; mm < G::PW; ++mm)   // (OOB + a chunk offset stays past every tensor)
        src[mm] = pa[mm % NPX] + (uint32_t)(((wave + 8 * mm) / G::PPC) * DC * 2);
      return;
    }
#pragma unroll
    for (int mm = 0; mm < G::PW; ++mm) {
      const int k = wave + 8 * mm;
      const int px = (k % G::PPC) * 8 + (lane >> 3);
      const int m = m0 + px;
      src[mm] = m < p.M ? bpix(m, p.Ho, p.Wo, rW, rH) * pitch + xoffb + (uint32_t)((k / G::PPC) * DC * 2) +
                              (uint32_t)(((lane & 7) ^ ((px >> 1) & 7)) * 16)
                        : OOB;
    }
  };
  int v_it = -1;
  auto issue_part = [&](int v, int m0p, int m1p) __attribute__((always_inline)) {
    if constexpr (HOOK == 2) return;
    const int it = v / G::NIV, iv = v - it * G::NIV;
    if (it != v_it) {
      set_tile(it);
      v_it = it;
    }
    unsigned char* dst = smem + (v % NS) * G::SB + wave * 1024;
#pragma unroll
    for (int mm = 0; mm < G::PW; ++mm)
      if (mm >= m0p && mm < m1p) dma16(xr, dst + mm * 8 * 1024, src[mm], (uint32_t)(iv * IC * DC * 2));
  };

  // ---- reads: chunk ci of the slot, px = pg * TPF * 16 + f * 16 + li; half h's part g at
  // (4 h + g) ^ ((li >> 1) & 7)
  uint32_t a_off[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    a_off[h] = (uint32_t)((pg * TPF * 16 + li) * 128 + (((4 * h + g) ^ ((li >> 1) & 7)) * 16));

  // one interval: IC chunks x 2 K steps; the DMA of interval vn goes out in 2 IC parts, one per K step
  auto compute = [&](int v, int iv, int vn) __attribute__((always_inline)) {
    const unsigned char* pb = smem + (v % NS) * G::SB;
#pragma unroll
    for (int ci = 0; ci < IC; ++ci)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int t2 = ci * 2 + h;
        issue_part(vn, t2 * G::PW / (2 * IC), (t2 + 1) * G::PW / (2 * IC));
        const int c = (iv * IC + ci) * 2 + h;
        u4 xa[TPF];
#pragma unroll
        for (int f = 0; f < TPF; ++f) xa[f] = *reinterpret_cast<const u4*>(pb + ci * G::TPX * 128 + a_off[h] + f * 16 * 128);
#pragma unroll
        for (int f = 0; f < TPF; ++f)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[j][f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wreg[j][c]),
                                                               __builtin_bit_cast(h8, xa[f]), acc[j][f], 0, 0, 0);
      }
  };
  // the lane's store channels, launch-invariant: byte offset, or past every offset the buffer accepts when
  // the channel is outside the layer (pixel offsets stay below 2^31, so the sum neither wraps nor lands)
  constexpr uint32_t CH_OOB = 0x7fffffffu;
  constexpr int NSC = TN % 2 == 0 ? TN / 2 : TN;
  const uint32_t ypitch = (uint32_t)p.yc * 2;
  const uint32_t y_lane = (uint32_t)li * ypitch;
  uint32_t ch_off[NSC];
#pragma unroll
  for (int c = 0; c < NSC; ++c) {
    const int n = n0 + ng * TN * 16 + (TN % 2 == 0 ? c * 32 + 16 * (g & 1) + 8 * (g >> 1) : c * 16 + g * 4);
    ch_off[c] = n < p.cout ? (uint32_t)n * 2 : CH_OOB;
  }
  // a store's offset: TIGHT keeps the test per store
  auto st_off = [&](uint32_t yo, bool live, int c) __attribute__((always_inline)) {
    if constexpr (TIGHT) {
      const int n = n0 + ng * TN * 16 + (TN % 2 == 0 ? c * 32 + 16 * (g & 1) + 8 * (g >> 1) : c * 16 + g * 4);
      return (live && n < p.cout) ? yo + (uint32_t)n * 2 : 0xffffffffu;
    } else {
      return yo + ch_off[c];
    }
  };
  auto epilogue = [&](int it) __attribute__((always_inline)) {
    const int mt = tw.at(it) * G::TPX;
    const int m0 = mt + pg * TPF * 16 + li;
    TileBase tb{};
    uint32_t ybase = 0;
    if (stepped) {
      tb = tile_base(mt, p);
      ybase = tb.idx * ypitch + (uint32_t)p.yoff * 2;
    }
#pragma unroll
    for (int f = 0; f < TPF; ++f) {
      uint32_t yo;
      bool live = true;   // (only TIGHT's stores look at it)
      if (stepped) {
        const int ok = pg * TPF * 16 + f * 16;
        yo = step_pix(y_lane + (ybase + (uint32_t)ok * ypitch), li, ok, tb, p.Wo, 2 * ypitch,
                      2 * (uint32_t)(p.Wo + 2) * ypitch);
      } else {
        const int m = m0 + f * 16;
        live = m < p.M;
        yo = live ? (uint32_t)((bpix(m, p.Ho, p.Wo, rW, rH) * p.yc + p.yoff) * 2) : OOB;
      }
      typedef _Float16 h4 __attribute__((ext_vector_type(4)));
      typedef uint32_t u2 __attribute__((ext_vector_type(2)));
      if constexpr (TN % 2 == 0) {
#pragma unroll
        for (int mp = 0; mp < TN / 2; ++mp) {
          h4 va, vb;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            va[e] = (_Float16)act_t<ACT>(acc[2 * mp][f][e]);
            vb[e] = (_Float16)act_t<ACT>(acc[2 * mp + 1][f][e]);
          }
          const u2 a = __builtin_bit_cast(u2, va), bb = __builtin_bit_cast(u2, vb);
          const auto s0 = __builtin_amdgcn_permlane16_swap(a[0], bb[0], false, false);
          const auto s1 = __builtin_amdgcn_permlane16_swap(a[1], bb[1], false, false);
          const u4 vv = {s0[0], s1[0], s0[1], s1[1]};
          __builtin_amdgcn_raw_buffer_store_b128(vv, yr, st_off(yo, live, mp), 0, 0);
        }
      } else {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          h4 va;
#pragma unroll
          for (int e = 0; e < 4; ++e) va[e] = (_Float16)act_t<ACT>(acc[j][f][e]);
          __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, va), yr, st_off(yo, live, j), 0, 0);
        }
      }
    }
  };
  auto barrier = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  // vmcnt before the barrier that ends interval v: the pieces of the interval the next barrier opens
  // (issued L - 1 intervals ago) landed; younger: the L - 1 later piece batches and the epilogue stores of
  // intervals v - L + 1 .. v that ended a tile (intervals before the first do not exist)
  // (hooks: 3 / 4 issue no epilogue stores and 2 no DMA pieces, so those terms are 0 there — ADVICE r5: a
  // looser count would let a wave past the barrier before its pieces landed and time a racy ring)
  auto wait_next = [&](int v) __attribute__((always_inline)) {
    constexpr int LB = HOOK == 2 ? 0 : G::PW * (G::L - 1);
    constexpr int NSTW = (HOOK == 3 || HOOK == 4) ? 0 : G::NST;
    int ends = 0;
#pragma unroll
    for (int d = 0; d < G::L; ++d) {
      const int vv = v - d;
      if (vv >= 0 && vv % G::NIV == G::NIV - 1) ++ends;
    }
    if (ends == 0) vmwait<LB>();
    else if (ends == 1) vmwait<(LB + NSTW < 63 ? LB + NSTW : 63)>();
    else if (ends == 2) vmwait<(LB + 2 * NSTW < 63 ? LB + 2 * NSTW : 63)>();
    else vmwait<(LB + 3 * NSTW < 63 ? LB + 3 * NSTW : 63)>();
  };

  // ---- prologue
#pragma unroll
  for (int v = 0; v < G::L; ++v) issue_part(v, 0, G::PW);
  vmwait<G::PW * (G::L - 1)>();
  barrier();
  if (STG && grp == 1) {   // group 1 runs STG intervals behind, issuing intervals L .. L + STG - 1 meanwhile
#pragma unroll
    for (int t = 0; t < STG; ++t) {
      issue_part(G::L + t, 0, G::PW);
      vmwait<G::PW * (G::L - 1)>();
      barrier();
    }
  }
  const int ahead = G::L + STG * grp;
  for (int it = 0; it < ntl; ++it) {
    init_acc();
#pragma unroll
    for (int iv = 0; iv < G::NIV; ++iv) {
      const int v = it * G::NIV + iv;
      if constexpr (HOOK == 4) issue_part(v + ahead, 0, G::PW);
      else compute(v, iv, v + ahead);
      if (iv == G::NIV - 1) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int f = 0; f < TPF; ++f) asm volatile("" : "+v"(acc[j][f]));
        if constexpr (HOOK == 3 || HOOK == 4) {
          if (p.cout < 0) epilogue(it);
        } else {
          epilogue(it);
        }
      }
      wait_next(v);
      barrier();
    }
  }
  if (STG && grp == 0) {
#pragma unroll
    for (int t = 0; t < STG; ++t) barrier();
  }
  vmwait<0>();
}

// configurations (variants 290 + row for rows 0-5, 296 + row for rows 6-7): {NCH, TN, TPF, PG, NG, NS,
// STG, IC}.  0-2: an interval per 64-channel chunk (cin 128 / 256 / 512), no stagger; 3-5: an interval per
// tile, stagger 1; 6-7: cin 256 with a 128-channel N slice (cfg 3's is 256: half its waves would compute
// masked channels of a 128-output layer).
struct W1Row { int nch, tn, tpf, pg, ng, ns, stg, ic; };
constexpr W1Row w1_rows[] = {
    {4, 8, 2, 8, 1, 4, 0, 1}, {8, 4, 4, 2, 4, 8, 0, 1}, {16, 2, 4, 2, 4, 8, 0, 1}, {8, 4, 2, 2, 4, 4, 1, 4},
    {4, 8, 1, 8, 1, 4, 1, 2}, {16, 2, 2, 1, 8, 4, 1, 8}, {8, 4, 1, 4, 2, 4, 1, 4}, {8, 2, 2, 2, 4, 4, 1, 4}};
constexpr int W1_NCFG = sizeof(w1_rows) / sizeof(w1_rows[0]);

template <int ROW, int HOOK = 0>
hipError_t launch_row(const ConvParams& p0, hipStream_t st) {
  constexpr W1Row r = w1_rows[ROW];
  ConvParams p = p0;
  p.d0 = make_div24(p.Wo);
  p.d1 = make_div24(p.Ho);
  using G = W1Geo<r.nch, r.tn, r.tpf, r.pg, r.ng, r.ns, r.stg, r.ic>;
  const int nN = (p.cout + G::BN - 1) / G::BN;
  const long T = ((long)p.M + G::TPX - 1) / G::TPX;
  long per = device_cus() / (8 * nN);
  const long need = (T + 7) / 8;
  if (per > need) per = need;
  if (per < 1) per = 1;
  const int grid = (int)(per * 8 * nN);
  if (HOOK) {
    YV7_LAUNCH((conv1x1_rw_kernel<r.nch, r.tn, r.tpf, r.pg, r.ng, r.ns, r.stg, r.ic, 1, HOOK>), dim3(grid), dim3(512), 0, st, p, nN);
    return hipGetLastError();
  }
  return launch_with_act(p.act, [&](auto A) {
    YV7_LAUNCH((conv1x1_rw_kernel<r.nch, r.tn, r.tpf, r.pg, r.ng, r.ns, r.stg, r.ic, decltype(A)::value>), dim3(grid), dim3(512), 0, st, p, nN);
    return hipGetLastError();
  });
}

}  // namespace

bool w1_supported(const ConvParams& p, int cfg) {
  if (cfg < 0 || cfg >= W1_NCFG) return false;
  return p.wf && p.k == 1 && p.s == 1 && p.pad == 0 && !p.pool && p.cin == w1_rows[cfg].nch * 32 &&
         p.H == p.Ho && p.W == p.Wo && (long)p.M < (1L << 24) && p.cout % 16 == 0 && p.cout <= 1024 &&
         p.xoff % 8 == 0 && p.xc % 8 == 0 && p.yoff % 8 == 0 && p.yc % 8 == 0;
}

hipError_t launch_conv_w1(const ConvParams& p, int cfg, hipStream_t st) {
  if (!w1_supported(p, cfg)) return hipErrorInvalidValue;
  if (p.act == 1 && cfg == 1 && p.variant >= 299 && p.variant <= 301) {   // hooks (convbench)
    if (p.variant == 299) return launch_row<1, 2>(p, st);
    if (p.variant == 300) return launch_row<1, 3>(p, st);
    return launch_row<1, 4>(p, st);
  }
  return launch_with_row<W1_NCFG>(cfg, [&](auto I) { return launch_row<decltype(I)::value>(p, st); });
}

}  // namespace yv7
