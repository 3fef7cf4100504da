// The fused Detect decode epilogue: used by the DET instantiations of the tile and ring kernels
// (conv_f16_ring.hip) and by the Detect heads (conv_det.hip).
#pragma once
#include "conv_f16_common.h"

namespace yv7 {

namespace {

// Fused Detect epilogue (models/yolo.py:52-57, IDetect.fuseforward yolo.py:140-176) shared by the
// tile and ring kernels.  BN >= na*no covers every head channel of BM consecutive pixels.
// LDS: zs = the tile's z values in z's own layout, [na][BM][no] fp32 (so z leaves as straight 16-byte
// copies), then a per-pixel table {z row of anchor 0 (int64, -1 past M), grid x, grid y} and the
// level's pixel anchors.
constexpr int det_tab(int BM, int BN) { return BM * BN * 4; }
constexpr int det_lds(int BM, int BN) { return det_tab(BM, BN) + BM * 16 + 64; }

__device__ __forceinline__ float det_sig(float v) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
}

struct DetTab {
  long long* zrow0;
  float *gx, *gy, *anc;
};

template <int BM, int BN>
__device__ __forceinline__ DetTab det_tab_ptrs(unsigned char* smem) {
  unsigned char* tab = smem + det_tab(BM, BN);
  DetTab t;
  t.zrow0 = reinterpret_cast<long long*>(tab);
  t.gx = reinterpret_cast<float*>(tab + BM * 8);
  t.gy = t.gx + BM;
  t.anc = t.gy + BM;
  return t;
}

// Step 0 (every thread; the caller then syncs): the per-pixel table.
template <int BM, int BN, int NTH, bool ANC = true>
__device__ __forceinline__ void det_table(const ConvParams& p, unsigned char* smem, int m0, int tid) {
  const DetTab t = det_tab_ptrs<BM, BN>(smem);
  const int hw = p.Ho * p.Wo;
  for (int r = tid; r < BM; r += NTH) {
    const int m = m0 + r;
    const int mm = m < p.M ? m : p.M - 1;
    const int b = mm / hw, cell = mm - b * hw;
    const int gy = cell / p.Wo, gx = cell - gy * p.Wo;
    t.zrow0[r] = m < p.M ? (long long)b * p.nrows + p.row_off + cell : -1;
    t.gx[r] = (float)gx;
    t.gy[r] = (float)gy;
  }
  if (ANC && tid < 8) t.anc[tid] = p.anchor[tid];
}

// Step 1 (registers): sigmoid of every logit, the Detect decode for the 4 box columns in the
// reference's op order (xy = (s*2 - 0.5 + grid)*stride, wh = (s*2)^2 * anchor_px), into zs; the raw
// logits (xs, optional) leave straight from the accumulators.  acc[j][i][e] = channel
// wn*WTN + j*16 + g*4 + e of pixel m0 + wm*WTM + i*16 + li.  NOC / NAC: compile-time no / na (0 =
// read p.no / p.na).  Branch-free per value: only the one 16-column block per wave that holds a box
// column runs the decode (a wave-uniform test), the padding column past na*no lands on a dummy slot.
template <int BM, int BN, int TN, int TM, int NOC, int NAC>
__device__ __forceinline__ void det_stage(const ConvParams& p, unsigned char* smem, const f4 (&acc)[TN][TM], int m0,
                                          int wm, int wn, int g, int li) {
  constexpr int WTM = TM * 16, WTN = TN * 16;
  const DetTab t = det_tab_ptrs<BM, BN>(smem);
  float* zs = reinterpret_cast<float*>(smem);
  const int NO = NOC ? NOC : p.no, NA = NAC ? NAC : p.na;
  const int dummy = NA * BM * NO;   // one spare float inside BM*BN (BN > na*no)
  const int wnu = __builtin_amdgcn_readfirstlane(wn);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int cb = wnu * WTN + j * 16;
    bool dec = false;
    for (int a = 0; a < NA; ++a) dec |= cb < a * NO + 4 && cb + 16 > a * NO;
    int zoff[4], co[4];
    bool live[4];
    float anc_wh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = cb + g * 4 + e;
      const int ca = c / NO;
      co[e] = c - ca * NO;
      live[e] = ca < NA;
      zoff[e] = live[e] ? ca * BM * NO + co[e] : dummy;
      anc_wh[e] = dec ? t.anc[(live[e] ? 2 * ca : 0) + (co[e] == 3 ? 1 : 0)] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * WTM + i * 16 + li;
      const int roff = row * NO;
      if (dec) {
        const float gxv = t.gx[row], gyv = t.gy[row];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s = det_sig(acc[j][i][e]);
          const float t2 = s * 2.0f;
          const float xy = (t2 - 0.5f + (co[e] == 0 ? gxv : gyv)) * p.stride;
          const float wh = (t2 * t2) * anc_wh[e];
          zs[zoff[e] + (live[e] ? roff : 0)] = co[e] < 2 ? xy : (co[e] < 4 ? wh : s);
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) zs[zoff[e] + (live[e] ? roff : 0)] = det_sig(acc[j][i][e]);
      }
    }
  }
  if (p.raw) {
    const int hw = p.Ho * p.Wo;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 16 + li;
        const int m = m0 + row;
        if (m >= p.M) continue;
        const int b = m / hw, cell = m - b * hw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = wnu * WTN + j * 16 + g * 4 + e;
          const int ca = c / NO, co = c - ca * NO;
          if (ca < NA) p.raw[((size_t)(b * NA + ca) * hw + cell) * NO + co] = acc[j][i][e];
        }
      }
  }
}

template <int BM, int BN, int NTH, int NOC, int NAC>
__device__ __forceinline__ void det_tail(const ConvParams& p, unsigned char* smem, int tid);

// The whole epilogue after the main loop (LDS free): table, values, scores + z.
template <int BM, int BN, int NTH, int TN, int TM>
__device__ __forceinline__ void det_epilogue(const ConvParams& p, unsigned char* smem, const f4 (&acc)[TN][TM], int m0,
                                             int wm, int wn, int g, int li, int tid) {
  det_table<BM, BN, NTH>(p, smem, m0, tid);
  __syncthreads();
  const bool std85 = p.no == 85 && p.na == 3;
  if (std85) det_stage<BM, BN, TN, TM, 85, 3>(p, smem, acc, m0, wm, wn, g, li);
  else det_stage<BM, BN, TN, TM, 0, 0>(p, smem, acc, m0, wm, wn, g, li);
  __syncthreads();
  if (std85) det_tail<BM, BN, NTH, 85, 3>(p, smem, tid);
  else det_tail<BM, BN, NTH, 0, 0>(p, smem, tid);
}

// yv7_row_best record of one (anchor, pixel) row: objectness, first-max class score obj * cls_c and
// its class, from the same sigmoid values z receives.  Four lanes per row, each over the classes
// c = part, part + 4, ... (first maximum per lane), merged by shuffles: the larger score wins, an
// equal score goes to the smaller class — the first maximum (general.py:683-684).
// (NB: the lane's classes are loaded in NB batches — 2 under register pressure — and scanned in order.)
template <int NC, int NB = 1>
__device__ __forceinline__ void det_best_lane(const float* sg, int nc, int part, float& best, int& bc) {
  const float obj = sg[4];
  best = -1.0f;
  bc = 0x7fffffff;
  if constexpr (NC > 0) {
    constexpr int NV = NC / 4 / NB;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float v[NV];
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = sg[5 + part + 4 * (b * NV + i)];
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const float s = v[i] * obj;
        if (s > best) { best = s; bc = part + 4 * (b * NV + i); }
      }
    }
  } else if (nc > 1) {
    for (int c = part; c < nc; c += 4) {
      const float s = sg[5 + c] * obj;
      if (s > best) { best = s; bc = c; }
    }
  } else if (part == 0) {
    best = obj;
    bc = 0;
  }
}

// Steps 2-3 (after det_stage and a barrier): the row scores, then z as 16-byte copies.
template <int BM, int BN, int NTH, int NOC, int NAC>
__device__ __forceinline__ void det_tail(const ConvParams& p, unsigned char* smem, int tid) {
  const DetTab t = det_tab_ptrs<BM, BN>(smem);
  const float* zs = reinterpret_cast<const float*>(smem);
  const int hw = p.Ho * p.Wo;
  const int NO = NOC ? NOC : p.no, NA = NAC ? NAC : p.na;
  if (p.best) {
    const int nc = NO - 5;
    for (int t0 = 0; t0 < BM * NA * 4; t0 += NTH) {
      const int tt = t0 + tid;
      const int r = tt >> 2, part = tt & 3;     // r = a * BM + pixel
      const int pr = r % BM, a = r / BM;
      const bool live = r < BM * NA && t.zrow0[pr] >= 0;
      const float* sg = zs + (live ? r : 0) * NO;
      float best;
      int bc;
      if (NOC == 85) det_best_lane<80>(sg, nc, part, best, bc);
      else det_best_lane<0>(sg, nc, part, best, bc);
#pragma unroll
      for (int d = 1; d < 4; d <<= 1) {
        const float ob = __shfl_xor(best, d, 64);
        const int oc = __shfl_xor(bc, d, 64);
        if (ob > best || (ob == best && oc < bc)) { best = ob; bc = oc; }
      }
      if (live && part == 0) {
        f4 rec;
        rec[0] = sg[4];
        rec[1] = best;
        rec[2] = __builtin_bit_cast(float, bc);
        rec[3] = 0.0f;
        // z and the row records are streamed out (non-temporal): nothing re-reads them before the NMS
        __builtin_nontemporal_store(rec, reinterpret_cast<f4*>(p.best + (size_t)(t.zrow0[pr] + (long long)a * hw) * 4));
      }
    }
  }
  // A 4-row group of one anchor (4 consecutive pixels of one image = 4 consecutive z rows) is no
  // float4 chunks in zs and in z.  Thread t owns chunk t % no of the groups it visits; a group whose
  // first z row is divisible by 4 (a 16-byte aligned block) leaves as 16-byte stores, any other one
  // (image boundary, rows past M, odd level sizes) element by element.
  constexpr int G = BM / 4;
  static_assert(BM % 4 == 0, "4-row groups");
  const int gpp = NTH / NO;
  const int c = tid % NO, gg = tid / NO;
  if (gg < gpp) {
    for (int idx = gg; idx < NA * G; idx += gpp) {
      const int a = idx / G, grp = idx - a * G;
      const long long aoff = (long long)a * hw;
      const long long z0 = t.zrow0[grp * 4];
      const f4 v = reinterpret_cast<const f4*>(zs + (a * BM + grp * 4) * NO)[c];
      if (z0 >= 0 && t.zrow0[grp * 4 + 3] == z0 + 3 && ((z0 + aoff) & 3) == 0) {
        __builtin_nontemporal_store(v, reinterpret_cast<f4*>(p.z + (size_t)(z0 + aoff) * NO) + c);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int e = 4 * c + k, rk = e / NO, ok = e - rk * NO;
          const long long zr = t.zrow0[grp * 4 + rk];
          if (zr >= 0) __builtin_nontemporal_store(v[k], p.z + (size_t)(zr + aoff) * NO + ok);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Persistent Detect head (round 3): the head conv + decode of one level (yolo.py:42-63) for the
// standard head (na = 3, no = 85, 1x1, K = cin a multiple of 64, level size a multiple of 4, no raw
// logits).  Measured on the tile kernel (scripts/detbench.hip hooks 90/93/94/95): at 80^2 its GEMM,
// staging, row scores and z stores take 37 + 27 + 9 + 54 us and do not overlap — both blocks of a CU
// run the same phase at the same time, so the z stores (209 MB at 80^2) drain while nothing else runs.
// Here one block per CU walks 64-pixel tiles with the K-step ring running across tiles:
//  * 8 waves (2 x 4), 64 pixels x 256 channels per tile, two 40 KiB ring stages + the z staging
//    image (zs, the tile's z rows in z's layout) and the row table: 146 KiB of LDS;
//  * the tile epilogue (sigmoid / decode into zs, row scores, z + row-record stores) runs after the
//    K loop; its first barrier frees the ring, so the next tile's first TWO stages are issued before
//    the epilogue and its K loop starts with both landed;
//  * every wave issues the same stores in every tile (10 with row records: 2 record + 8 z stores per
//    wave; rows past M, lanes without work and the other 3 lanes of a row's record go to an offset past
//    the buffer range, where the store is dropped), so the epilogue's stores stay in flight behind
//    counted vmcnt waits — they drain under the next tile's K loop and epilogue instead of stalling it.
// Same arithmetic as det_stage / det_tail (bit-identical z and records).
// ZU: the z-store loop's unroll (2 under register pressure: the register-weight head at K = 512)
template <int BM, int NTH, int ZU = 0>
__device__ __forceinline__ void det_tail_fixed(const ConvParams& p, unsigned char* smem, int tid,
                                               __amdgpu_buffer_rsrc_t zr, __amdgpu_buffer_rsrc_t br, long long zb) {
  constexpr int NO = 85, NA = 3, BN = 256;
  const DetTab t = det_tab_ptrs<BM, BN>(smem);
  const float* zs = reinterpret_cast<const float*>(smem);
  const int hw = p.Ho * p.Wo;
  float* zw = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int t0 = 0; t0 < BM * NA * 4; t0 += NTH) {
    // task (row r = anchor a x pixel pr, part): box column `part` of the row (the Detect decode in
    // det_stage's op order, yolo.py:52-57) and a quarter of its row-score scan
    const int tt = t0 + tid;
    const int r = tt >> 2, part = tt & 3;
    const int pr = r % BM, a = r / BM;
    const bool inr = r < BM * NA;
    const bool live = inr && t.zrow0[pr] >= 0;
    if (inr) {
      const float sgv = zs[r * NO + part];
      const float t2 = sgv * 2.0f;
      const float xy = (t2 - 0.5f + (part == 0 ? t.gx[pr] : t.gy[pr])) * p.stride;
      const float wh = (t2 * t2) * t.anc[2 * a + (part == 3 ? 1 : 0)];
      zw[r * NO + part] = part < 2 ? xy : wh;
    }
    if (p.best) {
      const float* sg = zs + (live ? r : 0) * NO;
      float best;
      int bc;
      det_best_lane<80, ZU ? 2 : 1>(sg, NO - 5, part, best, bc);
#pragma unroll
      for (int d = 1; d < 4; d <<= 1) {
        const float ob = __shfl_xor(best, d, 64);
        const int oc = __shfl_xor(bc, d, 64);
        if (ob > best || (ob == best && oc < bc)) { best = ob; bc = oc; }
      }
      f4 rec;
      rec[0] = sg[4];
      rec[1] = best;
      rec[2] = __builtin_bit_cast(float, bc);
      rec[3] = 0.0f;
      const uint32_t off = (live && part == 0) ? (uint32_t)((t.zrow0[pr] - zb + (long long)a * hw) * 16) : 0xffffffffu;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, rec), br, off, 0, 2);   // nt
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // decoded box columns visible to the z stores
  __builtin_amdgcn_s_barrier();
  constexpr int G = BM / 4;            // 4-row groups per anchor
  constexpr int GPP = NTH / NO;        // groups in flight per pass
  constexpr int IT = (NA * G + GPP - 1) / GPP;
  const int c = tid % NO, gg = tid / NO;
  constexpr int ZUN = ZU ? ZU : IT;
#pragma unroll ZUN
  for (int k = 0; k < IT; ++k) {
    const int idx = gg + GPP * k;
    const bool valid = gg < GPP && idx < NA * G;
    const int ii = valid ? idx : 0;
    const int a = ii / G, grp = ii - a * G;
    const long long z0 = t.zrow0[grp * 4];
    const f4 v = reinterpret_cast<const f4*>(zs + (a * BM + grp * 4) * NO)[c];
    const uint32_t off = (valid && z0 >= 0) ? (uint32_t)((z0 - zb + (long long)a * hw) * NO * 4 + c * 16) : 0xffffffffu;
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), zr, off, 0, 2);       // nt
  }
}

}  // namespace

}  // namespace yv7
