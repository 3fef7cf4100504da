// Device helpers shared by the fp16 implicit-GEMM conv kernels (conv_f16_ring.hip, conv_f16_pring.hip,
// conv_f16_p8.hip, conv_det.hip): tile constants, the LDS swizzle, and the pixel / K walks that turn
// operand addressing into per-lane offsets computed once plus scalar steps (LDS-DMA itself, dma16, is in
// yv7_kernels.h).  conv_f16.hip's header describes the GEMM view they serve.
#pragma once
#include "yv7_kernels.h"

namespace yv7 {

namespace {

constexpr int NT = 256;
constexpr int BKE = 64;    // K elements per step
constexpr int ROWB = 128;  // LDS bytes per tile row

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ (row & 7); }

// Output pixel m -> (b, ho, wo) once, then stepped: rows a thread moves are `step` pixels apart.
// Rows past M walk into image B, whose offsets lie beyond the input buffer (zeros).
struct PixelWalk {
  int b, ho, wo;
  __device__ __forceinline__ PixelWalk(const ConvParams& p, int m) {
    const int hw = p.Ho * p.Wo;
    b = m / hw;
    const int rem = m - b * hw;
    ho = rem / p.Wo;
    wo = rem - ho * p.Wo;
  }
  __device__ __forceinline__ void advance(const ConvParams& p, int step) {
    wo += step;
    while (wo >= p.Wo) {
      wo -= p.Wo;
      if (++ho == p.Ho) { ho = 0; ++b; }
    }
  }
};

// Byte offset in the bordered input of output pixel (b, ho, wo)'s receptive-field origin (tap 0,0),
// channel xoff + 8 * chunk.
__device__ __forceinline__ uint32_t a_origin(const ConvParams& p, int b, int ho, int wo, int chunk) {
  return (uint32_t)((pix_index(b, ho * p.s - p.pad, wo * p.s - p.pad, p.H, p.W) * p.xc + p.xoff + chunk * 8) * 2);
}

// The K-step cursor: tap (rr, ss) and channel ci of a K position, advanced BK at a time.
template <int BK = BKE>
struct KCursor {
  int ci, rr, ss, tap;
  __device__ __forceinline__ void init(const ConvParams& p, int k) {
    ci = k; rr = ss = tap = 0;
    while (ci >= p.cin) { ci -= p.cin; ++tap; if (++ss == p.k) { ss = 0; ++rr; } }
  }
  __device__ __forceinline__ void advance(const ConvParams& p) {
    ci += BK;
    while (ci >= p.cin) { ci -= p.cin; ++tap; if (++ss == p.k) { ss = 0; ++rr; } }
  }
  // byte offset of (rr, ss, ci) relative to the receptive-field origin
  __device__ __forceinline__ uint32_t offset(const ConvParams& p) const {
    return (uint32_t)(((rr * (p.W + 2 * BORDER) + ss) * p.xc + ci) * 2);
  }
};

// Chunk-major K walk of a 3x3 (or 1x1 strided) implicit GEMM with cin % 64 == 0, for the 8-phase rings:
// K step kt = (64-channel chunk cc, tap) with the tap fastest, so the nine taps of one chunk — which share
// most of their 128-byte input lines (stride 2: each line serves ~2.25 taps; stride 1: ~9) — are staged
// within nine consecutive K steps instead of one whole channel sweep apart (tap-major: 256 pixels x cin
// between two taps of a line, more than an XCD's L2 holds with every block of the XCD doing the same;
// round 5: 512->512 s2 @40 read its input 8.3 times from HBM / MALL, profiles/r5_pmc_ops.txt).  The
// weights keep the tap-major [cout][k * k * cin] layout; the B offset follows the same (tap, cc).
struct KWalk {
  int cc, tap, rr, ss;
  __device__ __forceinline__ void init() { cc = tap = rr = ss = 0; }
  __device__ __forceinline__ void advance(const ConvParams& p) {
    if (++tap == p.k * p.k) {
      tap = rr = ss = 0;
      ++cc;
    } else if (++ss == p.k) {
      ss = 0;
      ++rr;
    }
  }
  __device__ __forceinline__ uint32_t a_offset(const ConvParams& p) const {
    return (uint32_t)(((rr * (p.W + 2 * BORDER) + ss) * p.xc + cc * BKE) * 2);
  }
  __device__ __forceinline__ uint32_t b_offset(const ConvParams& p) const {
    return (uint32_t)((tap * p.cin + cc * BKE) * 2);
  }
};

// A-operand source of one K step (BK deep) for RA rows: uniform case (1x1, or cin % BK == 0) = per-row
// offset + scalar step offset; otherwise per-lane tap tracking (cin of 8..56: tiny's narrow layers).
template <bool ONE, int RA, int BK = BKE>
struct AWalk {
  uint32_t off[RA];   // row origin + this lane's chunk
  KCursor<BK> su;     // uniform cursor (k = kt*BK)
  KCursor<BK> ln;     // per-lane cursor (k = kt*BK + chunk*8), non-uniform case only
  bool uni;
  int c16;
  __device__ __forceinline__ void init(const ConvParams& p, int chunk, int kt0 = 0) {
    uni = ONE || (p.cin % BK) == 0;
    c16 = chunk * 16;
    su.init(p, kt0 * BK);
    if (!uni) ln.init(p, kt0 * BK + chunk * 8);
  }
  // voffset / soffset of row j for step kt (call step() once per K step, in order)
  template <typename F>
  __device__ __forceinline__ void step(const ConvParams& p, int kt, F&& load) {
    if (ONE) {
      const uint32_t so = (uint32_t)kt * BK * 2;
      if ((kt + 1) * BK <= p.K) {
#pragma unroll
        for (int j = 0; j < RA; ++j) load(j, off[j], so);
      } else {   // ragged last step (cin % BK != 0): lanes past K read zeros
        const bool kin = kt * BK + c16 / 2 < p.K;
#pragma unroll
        for (int j = 0; j < RA; ++j) load(j, kin ? off[j] : OOB, so);
      }
    } else if (uni) {
      const uint32_t so = su.offset(p);
      su.advance(p);
#pragma unroll
      for (int j = 0; j < RA; ++j) load(j, off[j], so);
    } else {
      const bool kin = kt * BK + c16 / 2 < p.K;
      const uint32_t d = ln.offset(p) - (uint32_t)c16;
      ln.advance(p);
#pragma unroll
      for (int j = 0; j < RA; ++j) load(j, kin ? off[j] + d : OOB, 0u);
    }
  }
};

// LDS image of a BK-deep stage: rows of BK*2 bytes in 16-byte chunks, the chunk index XOR-swizzled
// per row so that the 16-lane groups of every ds_read_b128 (lanes (g, li) read chunk g of rows
// base + li) hit 16 distinct 4-bank groups.  BK 64: 8 chunks per row, key row & 7.  BK 32: 4 chunks
// per 64-byte row (4 rows per 256-byte bank sweep), key (-(row >> 2)) & 3 (found by exhaustive
// check of the four lane groups of ds_read_b128).
template <int BK>
__device__ __forceinline__ int swz_bk(int row, int chunk) {
  if constexpr (BK == 64) return chunk ^ (row & 7);
  else return chunk ^ ((-(row >> 2)) & 3);
}

// vmcnt before ring step kt: stage kt landed, the min(MAXN, ahead) stages issued after it (PER DMA
// instructions each) may stay in flight — an immediate per case
template <int PER, int MAXN>
__device__ __forceinline__ void ring_wait(int ahead) {
  if constexpr (MAXN <= 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    static_assert(MAXN * PER <= 63, "vmcnt range");
    if (ahead >= MAXN) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MAXN * PER) : "memory");
    else ring_wait<PER, MAXN - 1>(ahead);
  }
}

}  // namespace

}  // namespace yv7
