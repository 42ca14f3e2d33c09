// irx — the forward half of libjpeg's integer chain, shared by the JPEG round trip (degrade_jpeg.hip) and the
// baseline encoder (jpeg_encode.hip): RGB -> YCbCr (16-bit fixed point), 4:2:0 down-sampling, the jfdctint "islow"
// passes and the quantiser's exact division.  Device code only; include from .hip files.
#pragma once
#include "ops.h"

namespace irx {
namespace jpegdev {

constexpr int FIX16(double x) { return (int)(x * 65536 + 0.5); }

constexpr int kC0298 = 2446, kC0390 = 3196, kC0541 = 4433, kC0765 = 6270, kC0899 = 7373, kC1175 = 9633;
constexpr int kC1501 = 12299, kC1847 = 15137, kC1961 = 16069, kC2053 = 16819, kC2562 = 20995, kC3072 = 25172;
constexpr int kConstBits = 13, kPass1Bits = 2;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one 1-D pass in place.  FIRST: rows (outputs scaled up by 2^PASS1_BITS); else columns.
template <bool FIRST>
__device__ __forceinline__ void fdct8(int d[8]) {
  constexpr int n = FIRST ? kConstBits - kPass1Bits : kConstBits + kPass1Bits;
  int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if (FIRST) {
    d[0] = (t10 + t11) << kPass1Bits;
    d[4] = (t10 - t11) << kPass1Bits;
  } else {
    d[0] = descale(t10 + t11, kPass1Bits);
    d[4] = descale(t10 - t11, kPass1Bits);
  }
  int z1 = (t12 + t13) * kC0541;
  d[2] = descale(z1 + t13 * kC0765, n);
  d[6] = descale(z1 - t12 * kC1847, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * kC1175;
  t4 *= kC0298; t5 *= kC2053; t6 *= kC3072; t7 *= kC1501;
  z1 *= -kC0899; z2 *= -kC2562;
  z3 = z3 * -kC1961 + z5;
  z4 = z4 * -kC0390 + z5;
  d[7] = descale(t4 + z1 + z3, n);
  d[5] = descale(t5 + z2 + z4, n);
  d[3] = descale(t6 + z2 + z3, n);
  d[1] = descale(t7 + z1 + z4, n);
}

// sign(c) * ((|c| + 4q) / 8q).  |c| + 4q < 2^24 and 8q < 2^11, so the fp32 quotient estimate is within one
// of the integer quotient; the remainder test makes it exact.
__device__ __forceinline__ int quantise(int c, int q) {
  const int den = 8 * q, num = abs(c) + 4 * q;
  int e = (int)((float)num * __frcp_rn((float)den));
  const int r = num - e * den;
  e += r >= den ? 1 : (r < 0 ? -1 : 0);
  return c < 0 ? -e : e;
}

// a tile of 4 MCUs: 64 x 16 pixels, 24 blocks; a block's 8 x 8 ints are stored with row stride 9 (row reads
// and column reads are both conflict-free: lanes step by 9 or by 1 across 32 banks, blocks by 72 = 8 mod 32)
constexpr int kJT = 192, kJTileW = 64, kJTileH = 16, kJBlkStride = 72, kJRow = 9;
constexpr int kJRawBytes = kJTileH * kJTileW * 3, kJBlkInts = 24 * kJBlkStride;

// The tile at (x0, y0) of one image (`base`, [H][W][3]), by all kJT lanes of a block: staged edge-clamped into
// `raw`, converted and down-sampled into `blk` (block m * 6 + {Y00, Y01, Y10, Y11, Cb, Cr} of MCU m, level-
// shifted), then the forward row pass in place.  Returns after the barrier that publishes the rows: lane
// (bi = tid >> 3, l = tid & 7) then owns column l of block bi.
__device__ __forceinline__ void jpeg_tile_rows(const uint8_t* __restrict__ base, int H, int W, int rgb, int x0, int y0,
                                               uint8_t* raw, int* blk) {
  const int tid = threadIdx.x, CH = (H + 1) / 2;
  {  // stage the tile, edge-clamped: lane = (pixel column, channel), one tile row per iteration
    const int px = tid / 3, c = tid - px * 3, sx = min(x0 + px, W - 1);
#pragma unroll 4
    for (int py = 0; py < kJTileH; ++py)
      raw[py * kJTileW * 3 + tid] = base[((long)min(y0 + py, H - 1) * W + sx) * 3 + c];
  }
  __syncthreads();
  const int ir = rgb ? 0 : 2, ib = 2 - ir;
  for (int p = tid; p < kJTileH * kJTileW; p += kJT) {
    const int py = p / kJTileW, px = p % kJTileW;
    const uint8_t* s = raw + p * 3;
    const int R = s[ir], G = s[1], Bc = s[ib];
    const int Y = (FIX16(.299) * R + FIX16(.587) * G + FIX16(.114) * Bc + 32768) >> 16;
    blk[((px >> 4) * 6 + (py >> 3) * 2 + ((px >> 3) & 1)) * kJBlkStride + (py & 7) * kJRow + (px & 7)] = Y - 128;
  }
  for (int p = tid; p < 8 * 32; p += kJT) {
    const int cyl = p >> 5, cxl = p & 31;
    // chroma rows are replicated after down-sampling: rows past the last real one repeat it
    const int r0 = 2 * min(y0 / 2 + cyl, CH - 1) - y0;     // in [0, 14]: the tile holds source row min(y, H-1)
    int cb = 0, cr = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint8_t* s = raw + ((r0 + (e >> 1)) * kJTileW + 2 * cxl + (e & 1)) * 3;
      const int R = s[ir], G = s[1], Bc = s[ib];
      cb += (-FIX16(.16874) * R - FIX16(.33126) * G + FIX16(.5) * Bc + (128 << 16) + 32767) >> 16;
      cr += (FIX16(.5) * R - FIX16(.41869) * G - FIX16(.08131) * Bc + (128 << 16) + 32767) >> 16;
    }
    const int bias = 1 + (cxl & 1);                          // x0 / 2 is even: the column parity is cxl's
    int* d = blk + ((cxl >> 3) * 6 + 4) * kJBlkStride + cyl * kJRow + (cxl & 7);
    d[0] = ((cb + bias) >> 2) - 128;
    d[kJBlkStride] = ((cr + bias) >> 2) - 128;
  }
  __syncthreads();
  {  // forward rows
    int d[8];
    int* p = blk + (tid >> 3) * kJBlkStride + (tid & 7) * kJRow;
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = p[e];
    fdct8<true>(d);
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] = d[e];
  }
  __syncthreads();
}

}  // namespace jpegdev
}  // namespace irx
