// irx — the inverse half of libjpeg's integer chain, shared by the JPEG round trip (degrade_jpeg.hip) and the
// baseline decoder (jpeg_decode.hip): the jidctint "islow" passes, the output stage, fancy h2v2 up-sampling and
// YCbCr -> RGB (16-bit fixed point).  Dequantisation is a plain product in front of the column pass and stays with
// the callers (one takes a quotient it has just formed, the other a stored coefficient).  Device code only.
//
// Output stage: a plain clamp of sample + 128 to 0..255.  libjpeg's C code indexes a masked table instead
// (range_limit[x & RANGE_MASK], which wraps where an intermediate leaves the 10-bit window), but Pillow's
// libjpeg-turbo runs the SIMD islow IDCT, which saturates: a single 1023-valued coefficient decodes to 255 / 0 there,
// not to the table's wrapped values (tests/test_jpeg_decode_host.py, the crafted file).
#pragma once
#include "jpeg_fdct.h"

namespace irx {
namespace jpegdev {

// jidctint.c, one 1-D pass in place, descaled by n bits (columns: 11, rows: 18)
template <int n>
__device__ __forceinline__ void idct8(int c[8]) {
  int z2 = c[2], z3 = c[6];
  int z1 = (z2 + z3) * kC0541;
  int t2 = z1 - z3 * kC1847, t3 = z1 + z2 * kC0765;
  int t0 = (c[0] + c[4]) << kConstBits, t1 = (c[0] - c[4]) << kConstBits;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = c[7]; t1 = c[5]; t2 = c[3]; t3 = c[1];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
  int z4 = t1 + t3;
  const int z5 = (z3 + z4) * kC1175;
  t0 *= kC0298; t1 *= kC2053; t2 *= kC3072; t3 *= kC1501;
  z1 *= -kC0899; z2 *= -kC2562;
  z3 = z3 * -kC1961 + z5;
  z4 = z4 * -kC0390 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  c[0] = descale(t10 + t3, n); c[7] = descale(t10 - t3, n);
  c[1] = descale(t11 + t2, n); c[6] = descale(t11 - t2, n);
  c[2] = descale(t12 + t1, n); c[5] = descale(t12 - t1, n);
  c[3] = descale(t13 + t0, n); c[4] = descale(t13 - t0, n);
}

constexpr int kIdctColBits = kConstBits - kPass1Bits, kIdctRowBits = kConstBits + kPass1Bits + 3;

// the output stage of one sample (see the head of this file)
__device__ __forceinline__ int sample_limit(int v) { return min(max(v + 128, 0), 255); }

// the eight samples of a row after the row pass, packed low byte first
__device__ __forceinline__ uint2 pack_row(const int d[8]) {
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lo |= (uint32_t)sample_limit(d[e]) << (8 * e);
    hi |= (uint32_t)sample_limit(d[e + 4]) << (8 * e);
  }
  return uint2{lo, hi};
}

// Pixels (2cx, 2cx + 1) of row y of one H x W image from its reconstructed planes (Y: row stride W16; Cb, Cr:
// row stride W16 / 2, the ceil(H/2) x ceil(W/2) corner is real): triangle-filter up-sampling with the neighbours
// clamped at the real extents, then the colour conversion.  o: the image's [H][W][3] output.
__device__ __forceinline__ void upsample_pair(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cbp,
                                              const uint8_t* __restrict__ crp, int H, int W, int W16, int rgb, int cx,
                                              int y, uint8_t* __restrict__ out) {
  const int CH = (H + 1) / 2, CW = (W + 1) / 2;
  const int cy = y >> 1, ny = min(max((y & 1) ? cy + 1 : cy - 1, 0), CH - 1);
  const int xl = max(cx - 1, 0), xr = min(cx + 1, CW - 1);
  int c[2][2];                                               // [Cb, Cr][even, odd pixel], level-shifted
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint8_t* pl = k ? crp : cbp;
    const uint8_t* r0 = pl + (long)cy * (W16 / 2);
    const uint8_t* r1 = pl + (long)ny * (W16 / 2);
    const int sl = 3 * r0[xl] + r1[xl], sc = 3 * r0[cx] + r1[cx], sr = 3 * r0[xr] + r1[xr];
    c[k][0] = ((3 * sc + sl + 8) >> 4) - 128;
    c[k][1] = ((3 * sc + sr + 7) >> 4) - 128;
  }
  const uint8_t* yr = yp + (long)y * W16 + 2 * cx;
  uint8_t* o = out + ((long)y * W + 2 * cx) * 3;
  const int ir = rgb ? 0 : 2, ib = 2 - ir;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    if (2 * cx + e >= W) break;
    const int Y = yr[e], cb = c[0][e], cr = c[1][e];
    o[3 * e + ir] = (uint8_t)min(max(Y + ((FIX16(1.402) * cr + 32768) >> 16), 0), 255);
    o[3 * e + 1] = (uint8_t)min(max(Y + ((-FIX16(.34414) * cb + 32768 - FIX16(.71414) * cr) >> 16), 0), 255);
    o[3 * e + ib] = (uint8_t)min(max(Y + ((FIX16(1.772) * cb + 32768) >> 16), 0), 255);
  }
}

}  // namespace jpegdev
}  // namespace irx
