// The class-count-generic Detect head of fp16 plans (models/yolo.py:46-57): the 1x1 head conv of one
// level and its decode for any (na, no) the plan validation admits (na <= 4, nc <= 128), with or without
// raw logits.  The tuned heads of conv_det.hip serve (na, no) = (3, 85) only, and the 256-wide DET forms
// of conv_f16_ring.hip cover na * no <= 256 channels of a pixel at the cost of a 256-wide tile whatever
// nc is; this kernel tiles per anchor instead.
//
//  * One block = 64 consecutive pixels x the `no` channels of ONE anchor, `no` rounded up to the
//    compile-time width NW in {32, 64, 96, 144} (nc <= 27 / 59 / 91 / 128).  4 waves; wave w owns pixels
//    16 w .. 16 w + 15 and all NW / 16 channel fragments, so every accumulator index is compile-time.
//  * Operands as in the ring kernels: K steps of 64 through an LDS-DMA ring of NS slots, NS - 1 stages in
//    flight (rows of 128 bytes, XOR-swizzled chunks), weights as the MFMA A operand.  The anchor's weight rows a * no .. a * no + no - 1
//    are read in place from the packed head weight (rows past `no` beyond the buffer range: zeros), its
//    bias slice likewise.  K is any multiple of 8: the packed weights are zero beyond cin up to kpad, and
//    the pixel lanes past cin in the last step read beyond the buffer range.
//  * Per-anchor tiling makes the epilogue a copy: anchor a's z rows of consecutive pixels of one image are
//    one contiguous span of z (and of the raw logits [B, na, ny, nx, no]).  The tile's values are staged
//    in LDS in that order — each image's span shifted by 0..3 floats so that it is 16-byte congruent with
//    its destination — and leave as 16-byte stores (the ragged head / tail of a span element by element).
//    No c / no division per value; a tile that straddles images is one span per image.
//  * Arithmetic of conv_det.h: accumulators start at the bias, mfma_f32_16x16x32_f16 over K in ascending
//    32-channel steps, det_sig, the decode in the reference's op order, det_best_lane<0> for the row
//    records — z is bit-equal to the ring head's where that one is valid.
//  * Grid: T tiles x na anchors, laid out so that the na blocks of a tile are neighbours on ONE XCD (block
//    b: XCD b % 8, then anchor-fastest), sharing the tile's pixels in that L2.
#include "conv_det.h"
#include "conv_f16_launch.h"

namespace yv7 {

namespace {

constexpr int NC_BM = 64, NC_NTH = 256;
// floats of one staged image: the tile's rows, 4 spare floats per image it can span, and the slack of the
// last 16-byte slot
constexpr int nc_img(int NW) { return NC_BM * NW + 4 * NC_BM + 8; }

// The tile's rows [0, rows) of one staged image to their destination: one span per image.  grow[r]: the
// destination row of tile row r; off[r]: its float offset in img (congruent mod 4 with the destination's
// float address); base4: the destination base address in floats.
__device__ __forceinline__ void nc_copy_spans(const float* img, const int* off, const long long* grow, float* dst,
                                              long long base4, int no, int rows, int hw, int cell0, int tid) {
  int r0 = 0, cell = cell0;
  while (r0 < rows) {
    const int len = min(hw - cell, rows - r0);
    const long long G = grow[r0] * no;
    const int sh = (int)((base4 + G) & 3);
    const int n = len * no;
    float* gb = dst + (G - sh);
    const f4* lb = reinterpret_cast<const f4*>(img + (off[r0] - sh));
    const int nv = (sh + n + 3) >> 2;
    for (int v = tid; v < nv; v += NC_NTH) {
      const f4 val = lb[v];
      const int e0 = 4 * v - sh;
      if (e0 >= 0 && e0 + 4 <= n) {
        // z, the raw logits and the row records are streamed out (non-temporal), as in conv_det.h
        __builtin_nontemporal_store(val, reinterpret_cast<f4*>(gb) + v);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (e0 + k >= 0 && e0 + k < n) __builtin_nontemporal_store(val[k], gb + 4 * v + k);
      }
    }
    r0 += len;
    cell = 0;
  }
}

template <int NW, int NS>
__global__ __launch_bounds__(NC_NTH) void conv_det_nc_kernel(const ConvParams p) {
  constexpr int BM = NC_BM, NWV = 4, TN = NW / 16;
  static_assert(NS == 2 || NS == 3, "ring slots");
  static_assert(NW % 16 == 0, "16-channel fragments");
  constexpr int RA = BM / 8 / NWV;                    // pixel wave-instructions per wave per stage
  constexpr int RB = (NW / 8 + NWV - 1) / NWV;        // weight ones (every wave issues the same count)
  constexpr int NWL = RB * NWV * 8;                   // weight rows staged (>= NW)
  constexpr int STAGE = (BM + NWL) * ROWB;
  constexpr int IMG = nc_img(NW);
  constexpr int PER = RA + RB;
  constexpr int OVL = NS * STAGE > 2 * IMG * 4 ? NS * STAGE : 2 * IMG * 4;   // ring, then the z / raw images
  constexpr int LDS = OVL + BM * 32;
  static_assert(LDS <= 80 * 1024, "two blocks per CU");
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS];
  // the row table (its own room: written before the K loop, read after it)
  long long* zrow = reinterpret_cast<long long*>(smem + OVL);   // z row of tile row r, -1 past M
  long long* xrow = zrow + BM;                                  // raw-logit row
  int* zoff = reinterpret_cast<int*>(xrow + BM);                // float offset of the row in the z image
  int* xoff = zoff + BM;                                        // ... in the raw image
  float* gxs = reinterpret_cast<float*>(xoff + BM);
  float* gys = gxs + BM;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, li = lane & 15;
  const int T = (p.M + BM - 1) / BM;
  const int bq = blockIdx.x >> 3;
  const int a = bq % p.na;
  const int tile = (bq / p.na) * 8 + (blockIdx.x & 7);
  if (tile >= T) return;
  const int m0 = tile * BM;
  const int no = p.no, hw = p.Ho * p.Wo;
  const int b0 = m0 / hw;
  const long long zbase4 = (long long)(reinterpret_cast<uintptr_t>(p.z) >> 2);
  const long long xbase4 = (long long)(reinterpret_cast<uintptr_t>(p.raw) >> 2);

  // the anchor's bias slice first: its latency passes under the address arithmetic below
  f4 bv[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = j * 16 + g * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) bv[j][e] = col + e < no ? p.bias[a * no + col + e] : 0.0f;
  }

  if (tid < BM) {
    const int r = tid, m = m0 + r;   // (rows past M: a virtual image B, never copied out)
    const int b = m / hw, cell = m - b * hw;
    const int gy = cell / p.Wo, gx = cell - gy * p.Wo;
    const long long zr = (long long)b * p.nrows + p.row_off + (long long)a * hw + cell;
    const long long xr = ((long long)b * p.na + a) * hw + cell;
    zrow[r] = m < p.M ? zr : -1;
    xrow[r] = xr;
    zoff[r] = r * no + 4 * (b - b0) + (int)((zbase4 + zr * no - (long long)r * no) & 3);
    xoff[r] = r * no + 4 * (b - b0) + (int)((xbase4 + xr * no - (long long)r * no) & 3);
    gxs[r] = (float)gx;
    gys[r] = (float)gy;
  }

  const auto xres = make_rsrc(p.x, p.xbytes);
  const auto wres = make_rsrc(p.w, p.wbytes);
  const int lr = lane >> 3;
  const int c = (lane & 7) ^ lr;
  uint32_t a_off[RA], b_off[RB];
#pragma unroll
  for (int j = 0; j < RA; ++j) {
    const int m = m0 + (j * NWV + wave) * 8 + lr;
    a_off[j] = OOB;
    if (m < p.M) {
      const int b = m / hw, cell = m - b * hw, ho = cell / p.Wo, wo = cell - ho * p.Wo;
      a_off[j] = (uint32_t)((pix_index(b, ho, wo, p.H, p.W) * p.xc + p.xoff + c * 8) * 2);
    }
  }
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const int row = (j * NWV + wave) * 8 + lr;
    b_off[j] = row < no ? (uint32_t)((((size_t)a * no + row) * p.kpad + c * 8) * 2) : OOB;
  }
  const int nk = p.kpad / BKE;
  auto issue = [&](int k, int slot) __attribute__((always_inline)) {
    unsigned char* As = smem + slot * STAGE;
    unsigned char* Bs = As + BM * ROWB;
    const uint32_t so = (uint32_t)k * BKE * 2;
    const bool kin = k * BKE + c * 8 < p.cin;   // the last step's lanes past cin (cin % 64 != 0): zeros
#pragma unroll
    for (int j = 0; j < RA; ++j) dma16(xres, As + (j * NWV + wave) * 8 * ROWB, kin ? a_off[j] : OOB, so);
#pragma unroll
    for (int j = 0; j < RB; ++j) dma16(wres, Bs + (j * NWV + wave) * 8 * ROWB, b_off[j], so);
    asm volatile("" ::: "memory");
  };

  // acc[j][e] = channel j * 16 + g * 4 + e of anchor a, pixel m0 + 16 wave + li; starts at the bias
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // bias (the ring's counted waits count DMA only)
  f4 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j) acc[j] = bv[j];
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nk) issue(s, s);
  int slot = 0;
  for (int k = 0; k < nk; ++k) {
    ring_wait<PER, NS - 2>(nk - 1 - k);                // stage k landed; up to NS - 2 later stages in flight
    __builtin_amdgcn_s_barrier();
    if (k + NS - 1 < nk) {                             // into the slot step k - 1 read
      int fs = slot + NS - 1;
      if (fs >= NS) fs -= NS;
      issue(k + NS - 1, fs);
    }
    const unsigned char* As = smem + slot * STAGE;
    if (++slot == NS) slot = 0;
    const unsigned char* Bs = As + BM * ROWB;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int ch = s * 4 + g;
      const int row = wave * 16 + li;
      const u4 xa = *reinterpret_cast<const u4*>(As + row * ROWB + swz(row, ch) * 16);
      u4 wb[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int wrow = j * 16 + li;
        wb[j] = *reinterpret_cast<const u4*>(Bs + wrow * ROWB + swz(wrow, ch) * 16);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, wb[j]), __builtin_bit_cast(h8, xa),
                                                        acc[j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __syncthreads();   // the ring is free: the z and raw images take its place

  float* zs = reinterpret_cast<float*>(smem);
  float* xs = zs + IMG;
  {
    const int row = wave * 16 + li;
    const int zo = zoff[row], xo = xoff[row];
    const float gxv = gxs[row], gyv = gys[row];
    const float aw = a == 0 ? p.anchor[0] : a == 1 ? p.anchor[2] : a == 2 ? p.anchor[4] : p.anchor[6];
    const float ah = a == 0 ? p.anchor[1] : a == 1 ? p.anchor[3] : a == 2 ? p.anchor[5] : p.anchor[7];
    const bool raw = p.raw != nullptr;
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int col = j * 16 + g * 4 + e;
        if (col >= no) continue;
        const float v = acc[j][e];
        float out = det_sig(v);
        if (j == 0 && col < 4) {   // the box columns (yolo.py:52-57), det_stage's op order
          const float t2 = out * 2.0f;
          const float xy = (t2 - 0.5f + (col == 0 ? gxv : gyv)) * p.stride;
          const float wh = (t2 * t2) * (col == 3 ? ah : aw);
          out = col < 2 ? xy : wh;
        }
        zs[zo + col] = out;
        if (raw) xs[xo + col] = v;
      }
  }
  __syncthreads();
  const int rows = min(BM, p.M - m0);
  if (p.best) {
    // one row per 4 lanes (BM * 4 = NTH), as det_tail
    const int r = tid >> 2, part = tid & 3;
    const bool live = r < rows;
    const float* sg = zs + zoff[live ? r : 0];
    float best;
    int bc;
    det_best_lane<0>(sg, no - 5, part, best, bc);
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
      __builtin_nontemporal_store(rec, reinterpret_cast<f4*>(p.best + (size_t)zrow[r] * 4));
    }
  }
  const int cell0 = m0 - b0 * hw;
  nc_copy_spans(zs, zoff, zrow, p.z, zbase4, no, rows, hw, cell0, tid);
  if (p.raw) nc_copy_spans(xs, xoff, xrow, p.raw, xbase4, no, rows, hw, cell0, tid);
}

}  // namespace

int det_nc_width(int no) { return no <= 32 ? 32 : no <= 64 ? 64 : no <= 96 ? 96 : no <= 144 ? 144 : 0; }

bool det_nc_supported(const ConvParams& p) {
  return p.k == 1 && p.s == 1 && p.pad == 0 && !p.pool && !p.res && p.na >= 1 && p.na <= 4 && p.no >= 6 &&
         det_nc_width(p.no) > 0 && p.cout == p.na * p.no && p.xoff % 8 == 0 && p.xc % 8 == 0 && p.cin % 8 == 0 &&
         p.kpad % BKE == 0 && p.kpad >= p.cin && p.H == p.Ho && p.W == p.Wo;
}

hipError_t launch_det_nc(const ConvParams& p, hipStream_t st) {
  if (!det_nc_supported(p)) return hipErrorInvalidValue;
  const long T = (p.M + NC_BM - 1) / NC_BM;
  const long nblk = (T + 7) / 8 * 8 * p.na;
  if (nblk > 0x7fffffffL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)nblk), block(NC_NTH);
  // Ring slots.  Two everywhere but on small grids of the narrow tiles: blocks per CU (LDS) hide more latency
  // than a deeper ring does, except where a level has at most 4 blocks per CU to begin with — there three
  // slots (two stages in flight) win at NW <= 64, bs 32, 20^2 (profiles/det_nc/ops_ring_slots.txt, us, 2 -> 3
  // slots: nc 1 15.1 -> 13.3, nc 20 18.1 -> 15.3, nc 40 21.0 -> 19.2, nc 59 24.1 -> 22.5; 40^2 ties; 80^2
  // 53.3 -> 57.4, 102.8 -> 106.7).  At NW >= 96 the third slot costs a resident block and loses at every
  // level (nc 83: 168 -> 190, 56.5 -> 62.6, 25.2 -> 31.5), so those forms were removed after the A/B.
  // YV7_DET_NC_NS=2 / 3 forces either where both exist.
  static const int ns_env = env_int("YV7_DET_NC_NS", 0);
  const int w = det_nc_width(p.no);
  const int ns = w > 64 ? 2 : (ns_env == 2 || ns_env == 3) ? ns_env : (nblk <= 4L * device_cus() ? 3 : 2);
  switch (w * 10 + ns) {
    case 322: YV7_LAUNCH((conv_det_nc_kernel<32, 2>), grid, block, 0, st, p); break;
    case 323: YV7_LAUNCH((conv_det_nc_kernel<32, 3>), grid, block, 0, st, p); break;
    case 642: YV7_LAUNCH((conv_det_nc_kernel<64, 2>), grid, block, 0, st, p); break;
    case 643: YV7_LAUNCH((conv_det_nc_kernel<64, 3>), grid, block, 0, st, p); break;
    case 962: YV7_LAUNCH((conv_det_nc_kernel<96, 2>), grid, block, 0, st, p); break;
    default: YV7_LAUNCH((conv_det_nc_kernel<144, 2>), grid, block, 0, st, p); break;
  }
  return hipGetLastError();
}

}  // namespace yv7
