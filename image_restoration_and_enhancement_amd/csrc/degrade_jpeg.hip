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
// The forward half (colour conversion, down-sampling, forward DCT, the quantiser's division) lives in jpeg_fdct.h,
// shared with the baseline encoder (jpeg_encode.hip); the inverse half (IDCT passes, output stage, up-sampling,
// colour conversion back) in jpeg_idct.h, shared with the baseline decoder (jpeg_decode.hip).
#include "jpeg_idct.h"

namespace irx {
namespace {

using namespace jpegdev;

__device__ __forceinline__ int quant_dequant(int c, int q) { return quantise(c, q) * q; }

__global__ __launch_bounds__(kJT) void jpeg_block_kernel(const uint8_t* __restrict__ img, int H, int W,
                                                         const int* __restrict__ qt, int rgb,
                                                         uint8_t* __restrict__ yp, uint8_t* __restrict__ cbp,
                                                         uint8_t* __restrict__ crp) {
  __shared__ uint8_t raw[kJRawBytes];
  __shared__ int blk[kJBlkInts];
  const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * kJTileW, y0 = blockIdx.y * kJTileH;
  const int H16 = (H + 15) & ~15, W16 = (W + 15) & ~15;
  jpeg_tile_rows(img + (long)b * H * W * 3, H, W, rgb, x0, y0, raw, blk);
  const int bi = tid >> 3, l = tid & 7, mcu = bi / 6, bk = bi - mcu * 6;
  int d[8];
  {  // forward columns, quantise, dequantise, inverse columns
    int* p = blk + bi * kJBlkStride + l;
    const int* q = qt + ((long)b * 2 + (bk >= 4)) * 64 + l;
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = p[e * kJRow];
    fdct8<false>(d);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = quant_dequant(d[e], min(max(q[e * 8], 1), 255));
    idct8<kIdctColBits>(d);
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e * kJRow] = d[e];
  }
  __syncthreads();
  {  // inverse rows, level shift, saturate, store one 8-byte row
    const int* p = blk + bi * kJBlkStride + l * kJRow;
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = p[e];
    idct8<kIdctRowBits>(d);
    const uint2 row = pack_row(d);
    if (x0 + 16 * mcu < W16) {
      uint8_t* dst;
      if (bk < 4) {
        dst = yp + ((long)b * H16 + y0 + (bk >> 1) * 8 + l) * W16 + x0 + 16 * mcu + (bk & 1) * 8;
      } else {
        dst = (bk == 4 ? cbp : crp) + ((long)b * (H16 / 2) + y0 / 2 + l) * (W16 / 2) + x0 / 2 + 8 * mcu;
      }
      *reinterpret_cast<uint2*>(dst) = row;                 // planes are 8-aligned: widths are multiples of 8
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
  upsample_pair(yp + (long)b * H16 * W16, cbp + (long)b * (H16 / 2) * (W16 / 2), crp + (long)b * (H16 / 2) * (W16 / 2), H,
                W, W16, rgb, cx, y, out + (long)b * H * W * 3);
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
