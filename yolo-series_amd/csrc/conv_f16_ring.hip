// The two non-persistent main loops of the fp16 implicit-GEMM conv (conv_f16.hip describes the GEMM
// view): the 4-wave register-staged tile kernel (2-3 blocks per CU, any width; also the MP-folded 1x1)
// and the 8-wave LDS-DMA ring for wide layers, with its split-K hand-off.  Both have a DET form that
// ends in the fused Detect epilogue (conv_det.h) and a RES form whose epilogue adds a residual operand.
#include "conv_det.h"
#include "conv_f16_launch.h"

namespace yv7 {

namespace {

// 2x2 max of four 16-byte fp16 vectors (MP folded into a 1x1 conv's operand loads)
__device__ __forceinline__ u4 hmax4(u4 a, u4 b, u4 c, u4 d) {
  const h8 m = __builtin_elementwise_max(__builtin_elementwise_max(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b)),
                                         __builtin_elementwise_max(__builtin_bit_cast(h8, c), __builtin_bit_cast(h8, d)));
  return __builtin_bit_cast(u4, m);
}

// POOL: 1x1 conv over the 2x2 / stride-2 max of the input (ConvParams::pool; k = 1, s = 2, pad = 0): each A
// row's origin is the window's top-left pixel, the other three are fixed byte offsets.
// RES: the residual epilogue (a Shortcut, models/common.py:80-86, folded into the conv that produces one of its
// operands): after bias and activation in fp32 the fp16 residual at the same (pixel, channel) is added and the sum
// rounded once.  Each lane fetches the four channels of its accumulator fragments as 8-byte buffer loads from the
// residual slice (pitch rc, offset roff, the output's geometry); rows past M and channels past cout take the
// out-of-range offset and read nothing.  The loads follow the K loop, ahead of the epilogue's LDS staging — not
// behind the tile's stores.  A compile-time flag of the shared body: the kernels without it are the code they were.
template <int TM>
__device__ __forceinline__ void res_rows(const ConvParams& p, int m_first, uint32_t (&ro)[TM]) {
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m_first + i * 16;
    ro[i] = OOB;
    if (m < p.M) {
      PixelWalk pw(p, m);
      ro[i] = (uint32_t)((pix_index(pw.b, pw.ho, pw.wo, p.Ho, p.Wo) * p.rc + p.roff) * 2);
    }
  }
}
typedef _Float16 h4r __attribute__((ext_vector_type(4)));
__device__ __forceinline__ h4r res_load(__amdgpu_buffer_rsrc_t rr, uint32_t row, int n, int cout) {
  const uint32_t vo = (row != OOB && n < cout) ? row + (uint32_t)n * 2 : OOB;
  return __builtin_bit_cast(h4r, __builtin_amdgcn_raw_buffer_load_b64(rr, vo, 0, 0));
}

template <int BM, int BN, int WM, bool ONE, bool DET, int PF, bool POOL, bool RES>
__device__ __forceinline__ void conv_f16_body(const ConvParams& p) {
  constexpr int WN = 4 / WM;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int RA = BM / 32;                 // A rows per thread (32 rows per pass of 256 threads)
  constexpr int RB = (BN + 31) / 32;
  constexpr int STAGE = (BM + BN) * ROWB;
  constexpr int CPITCH = BN * 2 + 16;
  constexpr int EPI0 = BM * CPITCH + BM * 4;   // staged C tile + output row table
  constexpr int EPI = (DET && det_lds(BM, BN) > EPI0) ? det_lds(BM, BN) : EPI0;
  constexpr int LDS = (2 * STAGE > EPI) ? 2 * STAGE : EPI;
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int g = lane >> 4, li = lane & 15;

  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  const int nN = (p.cout + BN - 1) / BN;
  const int m0 = (wgid / nN) * BM, n0 = (wgid % nN) * BN;

  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.w, p.wbytes);

  const int c = tid & 7;     // 16-byte chunk column this thread moves
  const int r0 = tid >> 3;   // first row this thread moves (then every 32nd)

  AWalk<ONE, RA> aw;
  aw.init(p, c);
  {
    PixelWalk pw(p, m0 + r0);
#pragma unroll
    for (int j = 0; j < RA; ++j) {
      if (j) pw.advance(p, 32);
      aw.off[j] = a_origin(p, pw.b, pw.ho, pw.wo, c);
    }
  }
  uint32_t b_off[RB];   // weight rows past cout_pad32 fall beyond the weight buffer (zeros)
#pragma unroll
  for (int j = 0; j < RB; ++j) b_off[j] = (uint32_t)(((n0 + r0 + 32 * j) * p.kpad + c * 8) * 2);

  const int nk = p.kpad / BKE;
  const uint32_t pdx = (uint32_t)p.xc * 2, pdy = (uint32_t)(p.W + 2 * BORDER) * p.xc * 2;   // POOL window steps
  auto gload = [&](int kt, u4 (&ra)[RA], u4 (&rb)[RB]) {
    aw.step(p, kt, [&](int j, uint32_t vo, uint32_t so) {
      if constexpr (POOL) {
        const u4 a = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(xr, vo, so, 0));
        const u4 b = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(xr, vo + pdx, so, 0));
        const u4 c2 = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(xr, vo + pdy, so, 0));
        const u4 d = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(xr, vo + pdy + pdx, so, 0));
        ra[j] = hmax4(a, b, c2, d);
      } else {
        ra[j] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(xr, vo, so, 0));
      }
    });
#pragma unroll
    for (int j = 0; j < RB; ++j)
      rb[j] = __builtin_bit_cast(u4, __builtin_amdgcn_raw_buffer_load_b128(wr, b_off[j], (uint32_t)kt * BKE * 2, 0));
  };
  auto lstore = [&](int buf, const u4 (&ra)[RA], const u4 (&rb)[RB]) {
    unsigned char* As = smem + buf * STAGE;
    unsigned char* Bs = As + BM * ROWB;
#pragma unroll
    for (int j = 0; j < RA; ++j) {
      const int row = r0 + 32 * j;
      *reinterpret_cast<u4*>(As + row * ROWB + swz(row, c) * 16) = ra[j];
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const int row = r0 + 32 * j;
      if (BN % 32 == 0 || row < BN) *reinterpret_cast<u4*>(Bs + row * ROWB + swz(row, c) * 16) = rb[j];
    }
  };

  // accumulators start at the bias (one VALU add per output element less in the epilogue)
  f4 acc[TN][TM];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * WTN + j * 16 + g * 4;
    f4 bv;
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = col + e < p.cout ? p.bias[col + e] : 0.0f;
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[j][i] = bv;
  }

  auto compute = [&](int buf) {
    const unsigned char* As = smem + buf * STAGE;
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
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i)
          acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wb[j]),
                                                             __builtin_bit_cast(h8, xa[i]), acc[j][i], 0, 0, 0);
    }
  };

  u4 ra[RA], rb[RB];
  gload(0, ra, rb);
  lstore(0, ra, rb);
  if constexpr (PF == 1) {
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      if (kt + 1 < nk) gload(kt + 1, ra, rb);
      compute(kt & 1);
      if (kt + 1 < nk) lstore((kt & 1) ^ 1, ra, rb);
      __syncthreads();
    }
  } else {
    // two register sets: the loads of step kt+2 are issued before step kt's MFMAs and have two steps
    // of MFMA work (instead of one) to land before their LDS write
    u4 ra2[RA], rb2[RB];
    if (nk > 1) gload(1, ra2, rb2);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
      if (kt + 2 < nk) gload(kt + 2, ra, rb);
      compute(0);
      if (kt + 1 < nk) lstore(1, ra2, rb2);
      __syncthreads();
      if (kt + 1 >= nk) break;
      if (kt + 3 < nk) gload(kt + 3, ra2, rb2);
      compute(1);
      if (kt + 2 < nk) lstore(0, ra, rb);
      __syncthreads();
    }
  }

  // accumulator acc[j][i][e]: output channel n = n0 + wn*WTN + j*16 + g*4 + e, pixel m = m0 + wm*WTM + i*16 + li
  if constexpr (DET) {
    det_epilogue<BM, BN, NT>(p, smem, acc, m0, wm, wn, g, li, tid);
    return;
  }

  // output row table: element offset of each tile row's pixel in the bordered output (or ~0u past M)
  uint32_t* yrow = reinterpret_cast<uint32_t*>(smem + BM * CPITCH);
  if (tid < BM) {
    const int m = m0 + tid;
    uint32_t v = ~0u;
    if (m < p.M) {
      PixelWalk pw(p, m);
      v = (uint32_t)(pix_index(pw.b, pw.ho, pw.wo, p.Ho, p.Wo) * p.yc + p.yoff);
    }
    yrow[tid] = v;
  }
  unsigned char* Cs = smem;
  [[maybe_unused]] uint32_t rrow[TM];
  [[maybe_unused]] const auto rr = make_rsrc(RES ? p.res : p.zero, RES ? p.rbytes : 0u);
  if constexpr (RES) res_rows<TM>(p, m0 + wm * WTM + li, rrow);
  with_act(p.act, [&](auto actc) {
    constexpr int ACT = decltype(actc)::value;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * WTN + j * 16 + g * 4;
      [[maybe_unused]] h4r rv[TM];
      if constexpr (RES) {
#pragma unroll
        for (int i = 0; i < TM; ++i) rv[i] = res_load(rr, rrow[i], n0 + col, p.cout);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 16 + li;
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        h4 v;
        if constexpr (RES) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (_Float16)(act_t<ACT>(acc[j][i][e]) + (float)rv[i][e]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (_Float16)act_t<ACT>(acc[j][i][e]);
        }
        *reinterpret_cast<h4*>(Cs + row * CPITCH + col * 2) = v;
      }
    }
  });
  __syncthreads();
  constexpr int CPR = BN * 2 / 16;
  _Float16* __restrict__ y = reinterpret_cast<_Float16*>(p.y);
  for (int cc = tid; cc < BM * CPR; cc += NT) {
    const int row = cc / CPR, ch = cc - row * CPR;
    const uint32_t yo = yrow[row];
    const int n = n0 + ch * 8;
    if (yo != ~0u && n < p.cout)
      *reinterpret_cast<u4*>(y + yo + n) = *reinterpret_cast<const u4*>(Cs + row * CPITCH + ch * 16);
  }
}

// Split-K hand-off between the S blocks of one output tile (last arriver reduces).  Every block
// publishes its fp32 partial tile ([TN*TM][NTH] float4, coalesced) to p.part, then counts itself in
// p.cnt[tile]; the block that counts last sums the S partials in split order 0..S-1 (the result does
// not depend on arrival order), re-arms the counter and runs the epilogue; the others exit.
// Protocol (MI355X_MICROARCH.md, inter-workgroup visibility, write-through form): partial stores
// and loads are sc1 (write-through, L1-bypassing; no agent release fence, whose L2 write-back of
// every dirty line of the XCD would cost more than the split saves), every wave's vmcnt(0), a
// barrier, then one lane's relaxed agent atomic add; the last arriver's waves load after that add
// returned and a barrier.  Each tile's partial lines are written once and read once per launch.
constexpr int CPOL_SC1 = 16;

template <int NTH, int TN, int TM>
__device__ __forceinline__ bool splitk_reduce(const ConvParams& p, unsigned char* smem, f4 (&acc)[TN][TM], int tile,
                                              int ks, int S, int tid) {
  constexpr int Q = TN * TM;
  const auto pr = make_rsrc(p.part, 0x7fffffffu);
  const uint32_t tbase = (uint32_t)tile * S * Q * NTH * 16;
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, acc[j][i]), pr,
                                             tbase + ((uint32_t)(ks * Q + j * TM + i) * NTH + tid) * 16, 0, CPOL_SC1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int* flag = reinterpret_cast<int*>(smem);
  if (tid == 0) {
    const int old = __hip_atomic_fetch_add(p.cnt + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = old == S - 1;
    if (last) __hip_atomic_store(p.cnt + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = last;
  }
  __syncthreads();
  const bool last = *flag != 0;
  __syncthreads();   // the flag word is epilogue LDS
  if (!last) return false;
  f4 sum[TN][TM];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i) sum[j][i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  for (int s = 0; s < S; ++s) {
    if (s == ks) {
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i) sum[j][i] += acc[j][i];
    } else {
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int i = 0; i < TM; ++i)
          sum[j][i] += __builtin_bit_cast(
              f4, __builtin_amdgcn_raw_buffer_load_b128(pr, tbase + ((uint32_t)(s * Q + j * TM + i) * NTH + tid) * 16, 0,
                                                        CPOL_SC1));
    }
  }
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[j][i] = sum[j][i];
  return true;
}

// ---------------------------------------------------------------------------------------------
// 8-wave LDS-DMA ring (wide layers).
//  * 512 threads = 8 waves (2 per SIMD, so one wave's fragment reads hide under the other's MFMAs),
//    BM x BN tile, BK = 64, STAGES-deep ring of LDS stages filled by buffer_load_dwordx4 ... lds —
//    no VGPR staging and no ds_write pass;
//  * each wave-instruction fills 8 tile rows (1 KiB, lane-linear in LDS), so the XOR swizzle is
//    applied on the SOURCE chunk (c = slot ^ (row & 7)) and the ds_read side uses the same swz();
//  * counted `s_waitcnt vmcnt(PER)` keeps the next stage in flight across a raw s_barrier (never
//    __syncthreads in the loop: its fence would drain the DMA); the stage refilled at step kt is the
//    one every wave finished reading at step kt-1 (its MFMAs consumed those reads before the barrier).
template <int BM, int BN, int WM, int WN, int STAGES, bool ONE, bool DET, bool RES>
__device__ __forceinline__ void conv_f16_ring_body(const ConvParams& p) {
  constexpr int NW = WM * WN, NTH = 64 * NW;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int RA = BM / 8 / NW, RB = BN / 8 / NW;   // wave-instructions per wave per stage
  static_assert(RA * 8 * NW == BM && RB * 8 * NW == BN, "tile rows must split into 8-row groups per wave");
  constexpr int PER = RA + RB;
  constexpr int STAGE = (BM + BN) * ROWB;
  constexpr int CPITCH = BN * 2 + 16;
  constexpr int EPI0 = BM * CPITCH + BM * 4;
  constexpr int EPI = (DET && det_lds(BM, BN) > EPI0) ? det_lds(BM, BN) : EPI0;
  constexpr int LDS = (STAGES * STAGE > EPI) ? STAGES * STAGE : EPI;
  static_assert(LDS <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int g = lane >> 4, li = lane & 15;

  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
  // split-K: the S blocks of one output tile are adjacent work ids, each sums the K steps [kb, ke)
  const int S = (!DET && p.ksplit > 1) ? p.ksplit : 1;
  const int tile = wgid / S, ks = wgid - tile * S;
  const int nN = (p.cout + BN - 1) / BN;
  const int m0 = (tile / nN) * BM, n0 = (tile % nN) * BN;
  const int nk_all = p.kpad / BKE;
  const int kb = ks * nk_all / S, ke = (ks + 1) * nk_all / S;

  const auto xr = make_rsrc(p.x, p.xbytes);
  const auto wr = make_rsrc(p.w, p.wbytes);

  const int lr = lane >> 3;            // row within the 8-row group (== row & 7)
  const int c = (lane & 7) ^ lr;       // source chunk this lane fetches

  AWalk<ONE, RA> aw;
  aw.init(p, c, kb);
  {
    PixelWalk pw(p, m0 + wave * 8 + lr);
#pragma unroll
    for (int j = 0; j < RA; ++j) {
      if (j) pw.advance(p, NW * 8);
      aw.off[j] = a_origin(p, pw.b, pw.ho, pw.wo, c);
    }
  }
  uint32_t b_off[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) b_off[j] = (uint32_t)(((n0 + (j * NW + wave) * 8 + lr) * p.kpad + c * 8) * 2);

  const int nk = ke - kb;   // K steps of this block; local step kt is global step kb + kt
  auto issue = [&](int kt, int slot) {
    unsigned char* As = smem + slot * STAGE;
    unsigned char* Bs = As + BM * ROWB;
    aw.step(p, kb + kt, [&](int j, uint32_t vo, uint32_t so) { dma16(xr, As + (j * NW + wave) * 8 * ROWB, vo, so); });
#pragma unroll
    for (int j = 0; j < RB; ++j) dma16(wr, Bs + (j * NW + wave) * 8 * ROWB, b_off[j], (uint32_t)(kb + kt) * BKE * 2);
  };

  // accumulators start at the bias (split 0 only)
  f4 acc[TN][TM];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = n0 + wn * WTN + j * 16 + g * 4;
    f4 bv;
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[e] = (col + e < p.cout && ks == 0) ? p.bias[col + e] : 0.0f;
#pragma unroll
    for (int i = 0; i < TM; ++i) acc[j][i] = bv;
  }

#pragma unroll
  for (int s0 = 0; s0 < STAGES - 1; ++s0)
    if (s0 < nk) issue(s0, s0);

  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    // stage kt must have landed; the (at most STAGES-2) stages issued after it may stay in flight
    const int ahead = nk - 1 - kt;
    ring_wait<PER, STAGES - 2>(ahead);
    __builtin_amdgcn_s_barrier();
    if (kt + STAGES - 1 < nk) {
      int fs = slot + STAGES - 1;
      if (fs >= STAGES) fs -= STAGES;
      issue(kt + STAGES - 1, fs);
    }
    const unsigned char* As = smem + slot * STAGE;
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
    if (++slot == STAGES) slot = 0;
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();

  if (S > 1 && !splitk_reduce<NTH, TN, TM>(p, smem, acc, tile, ks, S, tid)) return;

  if constexpr (DET) {
    det_epilogue<BM, BN, NTH>(p, smem, acc, m0, wm, wn, g, li, tid);
    return;
  }
  uint32_t* yrow = reinterpret_cast<uint32_t*>(smem + BM * CPITCH);
  for (int t = tid; t < BM; t += NTH) {
    const int m = m0 + t;
    uint32_t v = ~0u;
    if (m < p.M) {
      PixelWalk pw(p, m);
      v = (uint32_t)(pix_index(pw.b, pw.ho, pw.wo, p.Ho, p.Wo) * p.yc + p.yoff);
    }
    yrow[t] = v;
  }
  unsigned char* Cs = smem;
  [[maybe_unused]] uint32_t rrow[TM];
  [[maybe_unused]] const auto rr = make_rsrc(RES ? p.res : p.zero, RES ? p.rbytes : 0u);
  if constexpr (RES) res_rows<TM>(p, m0 + wm * WTM + li, rrow);
  with_act(p.act, [&](auto actc) {
    constexpr int ACT = decltype(actc)::value;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int col = wn * WTN + j * 16 + g * 4;
      [[maybe_unused]] h4r rv[TM];
      if constexpr (RES) {
#pragma unroll
        for (int i = 0; i < TM; ++i) rv[i] = res_load(rr, rrow[i], n0 + col, p.cout);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 16 + li;
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        h4 v;
        if constexpr (RES) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (_Float16)(act_t<ACT>(acc[j][i][e]) + (float)rv[i][e]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (_Float16)act_t<ACT>(acc[j][i][e]);
        }
        *reinterpret_cast<h4*>(Cs + row * CPITCH + col * 2) = v;
      }
    }
  });
  __syncthreads();
  constexpr int CPR = BN * 2 / 16;
  _Float16* __restrict__ y = reinterpret_cast<_Float16*>(p.y);
  for (int cc = tid; cc < BM * CPR; cc += NTH) {
    const int row = cc / CPR, ch = cc - row * CPR;
    const uint32_t yo = yrow[row];
    const int n = n0 + ch * 8;
    if (yo != ~0u && n < p.cout)
      *reinterpret_cast<u4*>(y + yo + n) = *reinterpret_cast<const u4*>(Cs + row * CPITCH + ch * 16);
  }
}

template <int BM, int BN, int WM, bool ONE, bool DET, int PF = 1, bool POOL = false>
__global__ __launch_bounds__(NT, 2) void conv_f16_kernel(const ConvParams p) {
  conv_f16_body<BM, BN, WM, ONE, DET, PF, POOL, false>(p);
}
template <int BM, int BN, int WM, bool ONE>
__global__ __launch_bounds__(NT, 2) void conv_f16_res_kernel(const ConvParams p) {
  conv_f16_body<BM, BN, WM, ONE, false, 1, false, true>(p);
}
template <int BM, int BN, int WM, int WN, int STAGES, bool ONE, bool DET = false>
__global__ __launch_bounds__(64 * WM * WN, (STAGES * (BM + BN) * 128 <= 80 * 1024) ? 2 : 1) void conv_f16_ring_kernel(const ConvParams p) {
  conv_f16_ring_body<BM, BN, WM, WN, STAGES, ONE, DET, false>(p);
}
template <int BM, int BN, int WM, int WN, int STAGES, bool ONE>
__global__ __launch_bounds__(64 * WM * WN, (STAGES * (BM + BN) * 128 <= 80 * 1024) ? 2 : 1) void conv_f16_ring_res_kernel(const ConvParams p) {
  conv_f16_ring_body<BM, BN, WM, WN, STAGES, ONE, false, true>(p);
}

template <int BM, int BN, int WM, bool ONE, bool DET, int PF, bool POOL, bool RES>
hipError_t launch_t(const ConvParams& p, hipStream_t st) {
  const int nM = (p.M + BM - 1) / BM, nN = (p.cout + BN - 1) / BN;
  if (DET && p.cout > BN) return hipErrorInvalidValue;   // det_epilogue decodes one N tile: channels 0 .. BN - 1
  if constexpr (RES) {
    static_assert(!DET && !POOL && PF == 1, "the residual rows are plain tiles");
    if (!p.res) return hipErrorInvalidValue;
    YV7_LAUNCH((conv_f16_res_kernel<BM, BN, WM, ONE>), dim3(nM * nN), dim3(NT), 0, st, p);
  } else {
    if (p.res) return hipErrorInvalidValue;   // a row without the residual epilogue would drop the operand
    YV7_LAUNCH((conv_f16_kernel<BM, BN, WM, ONE, DET, PF, POOL>), dim3(nM * nN), dim3(NT), 0, st, p);
  }
  return hipGetLastError();
}

template <int BM, int BN, int WM, int WN, int STAGES, bool ONE, bool DET, bool RES>
hipError_t launch_r(const ConvParams& p0, int S, hipStream_t st) {
  ConvParams p = p0;
  if (DET && p.cout > BN) return hipErrorInvalidValue;   // det_epilogue decodes one N tile: channels 0 .. BN - 1
  const long tiles = (long)((p.M + BM - 1) / BM) * ((p.cout + BN - 1) / BN);
  unsigned nblk = (unsigned)tiles;
  if (S >= 1) {
    p.ksplit = S;
    if (S > 1 && (!p.part || !p.cnt || p.part_bytes < (size_t)tiles * S * BM * BN * 4 || p.cnt_n < tiles))
      return hipErrorInvalidValue;   // the caller sized the scratch with conv_splitk_part_bytes
    nblk = (unsigned)(tiles * S);
  }
  if constexpr (RES) {
    static_assert(!DET, "the residual rows are plain rings");
    if (!p.res) return hipErrorInvalidValue;
    YV7_LAUNCH((conv_f16_ring_res_kernel<BM, BN, WM, WN, STAGES, ONE>), dim3(nblk), dim3(64 * WM * WN), 0, st, p);
  } else {
    if (p.res) return hipErrorInvalidValue;
    YV7_LAUNCH((conv_f16_ring_kernel<BM, BN, WM, WN, STAGES, ONE, DET>), dim3(nblk), dim3(64 * WM * WN), 0, st, p);
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_tile(const ConvParams& p, int row, hipStream_t st) {
  const bool one = p.k == 1 && p.s == 1 && p.pad == 0;
  return launch_with_row<NTILE>(row, [&](auto I) {
    constexpr TileRow r = tile_rows[decltype(I)::value];
    if constexpr (r.one != ONE_BOTH) return launch_t<r.bm, r.bn, r.wm, r.one == ONE_ONLY, r.det, r.pf, r.pool, r.res>(p, st);
    else return one ? launch_t<r.bm, r.bn, r.wm, true, r.det, r.pf, r.pool, r.res>(p, st)
                    : launch_t<r.bm, r.bn, r.wm, false, r.det, r.pf, r.pool, r.res>(p, st);
  });
}

hipError_t launch_ring(const ConvParams& p, int row, int S, hipStream_t st) {
  const bool one = p.k == 1 && p.s == 1 && p.pad == 0;
  return launch_with_row<NRING>(row, [&](auto I) {
    constexpr RingRow r = ring_rows[decltype(I)::value];
    if constexpr (r.one != ONE_BOTH) return launch_r<r.bm, r.bn, r.wm, r.wn, r.stages, r.one == ONE_ONLY, r.det, r.res>(p, S, st);
    else return one ? launch_r<r.bm, r.bn, r.wm, r.wn, r.stages, true, r.det, r.res>(p, S, st)
                    : launch_r<r.bm, r.bn, r.wm, r.wn, r.stages, false, r.det, r.res>(p, S, st);
  });
}

}  // namespace yv7
