// irx — JPEG round trip on the GPU: the pixels of add_jpeg_compression
// (scripts/make_synthetic_pairs.py:38-43, cv2.imencode('.jpg') -> cv2.imdecode) for uint8 [B][H][W][3] batches
// resident in HBM.  The entropy coder is lossless, so the decoded pixels are libjpeg's integer chain alone:
//   RGB -> YCbCr (16-bit fixed point), 4:2:0 down-sampling, jfdctint "islow" DCT, quantise, dequantise,
//   jidctint "islow" IDCT, fancy h2v2 up-sampling, YCbCr -> RGB.
// Restated operation for operation in int32 (degrade_host.py jpeg_roundtrip_ref is the same chain in numpy and is
// pinned bit-exact to Pillow + libjpeg-turbo).  Two kernels:
//   * jpeg_block_kernel: a block of 192 lanes owns 4 horizontally adjacent 16x16 MCUs = 24 8x8 blocks, one lane
//     per 8-sample row or column; the transposes between the 1-D passes go through LDS.  The forward column pass
//     and the inverse column pass are adjacent in the chain, so quantisation happens in registers between them.
//     Reconstructed Y / Cb / Cr planes (padded to whole MCUs) go to the caller's workspace.
//   * jpeg_upsample_kernel: triangle-filter up-sampling of the ceil(H/2) x ceil(W/2) chroma and the colour
//     conversion back.  It reads a one-sample halo of neighbouring MCUs' chroma, hence the second launch.
// Two padding rules (both libjpeg's): the Y plane and the full-resolution chroma columns are edge-replicated to
// whole MCUs, but chroma ROWS are replicated after down-sampling (the last down-sampled row repeats), and the
// up-sampler clamps its neighbours at exactly ceil(H/2) x ceil(W/2), not at the padded extents.
#include "ops.h"

namespace irx {
namespace {

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

// sign(c) * ((|c| + 4q) / 8q) * q.  |c| + 4q < 2^24 and 8q < 2^11, so the fp32 quotient estimate is within one
// of the integer quotient; the remainder test makes it exact.
__device__ __forceinline__ int quant_dequant(int c, int q) {
  const int den = 8 * q, num = abs(c) + 4 * q;
  int e = (int)((float)num * __frcp_rn((float)den));
  const int r = num - e * den;
  e += r >= den ? 1 : (r < 0 ? -1 : 0);
  return (c < 0 ? -e : e) * q;
}

// a tile of 4 MCUs: 64 x 16 pixels, 24 blocks; a block's 8 x 8 ints are stored with row stride 9 (row reads
// and column reads are both conflict-free: lanes step by 9 or by 1 across 32 banks, blocks by 72 = 8 mod 32)
constexpr int kJT = 192, kJTileW = 64, kJTileH = 16, kJBlkStride = 72, kJRow = 9;

__global__ __launch_bounds__(kJT) void jpeg_block_kernel(const uint8_t* __restrict__ img, int H, int W,
                                                         const int* __restrict__ qt, int rgb,
                                                         uint8_t* __restrict__ yp, uint8_t* __restrict__ cbp,
                                                         uint8_t* __restrict__ crp) {
  __shared__ uint8_t raw[kJTileH * kJTileW * 3];
  __shared__ int blk[24 * kJBlkStride];
  const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * kJTileW, y0 = blockIdx.y * kJTileH;
  const int H16 = (H + 15) & ~15, W16 = (W + 15) & ~15, CH = (H + 1) / 2;
  const uint8_t* base = img + (long)b * H * W * 3;
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
  const int bi = tid >> 3, l = tid & 7, mcu = bi / 6, bk = bi - mcu * 6;
  int d[8];
  {  // forward rows
    int* p = blk + bi * kJBlkStride + l * kJRow;
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = p[e];
    fdct8<true>(d);
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] = d[e];
  }
  __syncthreads();
  {  // forward columns, quantise, dequantise, inverse columns
    int* p = blk + bi * kJBlkStride + l;
    const int* q = qt + ((long)b * 2 + (bk >= 4)) * 64 + l;
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = p[e * kJRow];
    fdct8<false>(d);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = quant_dequant(d[e], min(max(q[e * 8], 1), 255));
    idct8<kConstBits - kPass1Bits>(d);
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e * kJRow] = d[e];
  }
  __syncthreads();
  {  // inverse rows, level shift, saturate, store one 8-byte row
    const int* p = blk + bi * kJBlkStride + l * kJRow;
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = p[e];
    idct8<kConstBits + kPass1Bits + 3>(d);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      lo |= (uint32_t)min(max(d[e] + 128, 0), 255) << (8 * e);
      hi |= (uint32_t)min(max(d[e + 4] + 128, 0), 255) << (8 * e);
    }
    if (x0 + 16 * mcu < W16) {
      uint8_t* dst;
      if (bk < 4) {
        dst = yp + ((long)b * H16 + y0 + (bk >> 1) * 8 + l) * W16 + x0 + 16 * mcu + (bk & 1) * 8;
      } else {
        dst = (bk == 4 ? cbp : crp) + ((long)b * (H16 / 2) + y0 / 2 + l) * (W16 / 2) + x0 / 2 + 8 * mcu;
      }
      *reinterpret_cast<uint2*>(dst) = uint2{lo, hi};        // planes are 8-aligned: widths are multiples of 8
    }
  }
}

// one lane per horizontal pixel pair (2cx, 2cx + 1) of one output row
__global__ __launch_bounds__(256) void jpeg_upsample_kernel(const uint8_t* __restrict__ yp,
                                                            const uint8_t* __restrict__ cbp,
                                                            const uint8_t* __restrict__ crp, int B, int H, int W,
                                                            int rgb, uint8_t* __restrict__ out) {
  const int H16 = (H + 15) & ~15, W16 = (W + 15) & ~15, CH = (H + 1) / 2, CW = (W + 1) / 2;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * H * CW) return;
  const int cx = (int)(i % CW), y = (int)((i / CW) % H), b = (int)(i / ((long)CW * H));
  const int cy = y >> 1, ny = min(max((y & 1) ? cy + 1 : cy - 1, 0), CH - 1);
  const int xl = max(cx - 1, 0), xr = min(cx + 1, CW - 1);
  int c[2][2];                                               // [Cb, Cr][even, odd pixel], level-shifted
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint8_t* pl = (k ? crp : cbp) + (long)b * (H16 / 2) * (W16 / 2);
    const uint8_t* r0 = pl + (long)cy * (W16 / 2);
    const uint8_t* r1 = pl + (long)ny * (W16 / 2);
    const int sl = 3 * r0[xl] + r1[xl], sc = 3 * r0[cx] + r1[cx], sr = 3 * r0[xr] + r1[xr];
    c[k][0] = ((3 * sc + sl + 8) >> 4) - 128;
    c[k][1] = ((3 * sc + sr + 7) >> 4) - 128;
  }
  const uint8_t* yr = yp + ((long)b * H16 + y) * W16 + 2 * cx;
  uint8_t* o = out + (((long)b * H + y) * W + 2 * cx) * 3;
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

inline long pad16(int v) { return ((long)v + 15) & ~15L; }

}  // namespace

long degrade_jpeg_ws_bytes(int B, int H, int W) { return (long)B * pad16(H) * pad16(W) * 3 / 2; }

void degrade_jpeg(const uint8_t* img, int B, int H, int W, const int* qt_dev, int rgb, void* ws, uint8_t* out,
                  hipStream_t s) {
  IRX_CHECK(B <= 65535 && pad16(H) / 16 <= 65535, "batch and H / 16 must fit a grid dimension");
  IRX_CHECK(((uintptr_t)ws & 7) == 0, "workspace must be 8-byte aligned");
  const long H16 = pad16(H), W16 = pad16(W);
  uint8_t* yp = static_cast<uint8_t*>(ws);
  uint8_t* cbp = yp + (long)B * H16 * W16;
  uint8_t* crp = cbp + (long)B * H16 * W16 / 4;
  jpeg_block_kernel<<<dim3((unsigned)((W16 + kJTileW - 1) / kJTileW), (unsigned)(H16 / 16), B), kJT, 0, s>>>(
      img, H, W, qt_dev, rgb, yp, cbp, crp);
  IRX_LAUNCH_CHECK();
  const long n = (long)B * H * ((W + 1) / 2);
  jpeg_upsample_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(yp, cbp, crp, B, H, W, rgb, out);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
