// Real-ESRGAN's compact network (SRVGGNetCompact 3 -> 64 x 32 -> 48, pixel shuffle 4, + nearest x4 of the input;
// srvgg_host.py / the reference's src/inference.py:335-336, :579-591): the kernels of the Srvgg model (models.h).
//
// fp16 engine (the product: the reference's half=True on a GPU), three kernels:
//   srvgg_head_kernel        uint8 [B][H][W][3] -> the host's float[256] table (k / 255) rounded to fp16 -> conv 3 -> 64,
//                            bias, PReLU -> fp16 NHWC.  3.5 kFLOP and 128 B written per pixel: memory-bound, plain VALU,
//                            a thread per pixel and 8 output channels, the 64 x 27 weights in LDS.
//   srvgg_conv_kernel<0>     a body layer: 3x3, 64 -> 64, pad 1, bias + PReLU, fp16 in, fp32 accumulate, fp16 out.
//                            Persistent blocks of 256 threads.  A block copies the layer's whole [64][3][3][64] panel
//                            into LDS once (rows padded 1152 -> 1168 B: conflict-free ds_read_b128 across 16 rows), then
//                            walks 8 x 32 pixel tiles of one image: the 10 x 34 x 64 halo tile in LDS (pixels padded
//                            128 -> 144 B), the next tile's halo in flight in registers while this one computes.  A wave
//                            owns two tile rows (2 x 32 pixels) x 64 output channels: four 32x32 accumulators,
//                            mfma_f32_32x32x16_f16 with A = weights (row = output channel) and B = pixels (column =
//                            pixel), so a lane ends up with 4 consecutive output channels of one pixel per register
//                            quad: 8-byte stores.  Per output element the K order is tap-major, then channel, 36 MFMA
//                            steps on one accumulator: it does not depend on the tile, the block or the batch.
//                            Rows and columns outside the image are zeros in the halo tile; a tile never spans two
//                            images, so the neighbouring image is never read.
//   srvgg_conv_kernel<1>     the tail: the same main loop on the 64 -> 48 conv (panel rows 48..63 zero), and in the
//                            epilogue bias, pixel shuffle out[b][4y+i][4x+j][c] = conv[b][y][x][16c+4i+j], + the input
//                            pixel (re-derived from the uint8 image and the table), clamp, * 255, rint -> uint8
//                            [B][4H][4W][3] (and the unclamped fp32 value of the same fp16 result to out_f if not null).
//                            No [B][H][W][48] tensor goes to memory.
// Rounding contract of the fp16 engine (srvgg_host.forward(half=True)): bias and slope rounded to fp16 when read from
// the fp32 blob; acc + bias in fp32 -> fp16; PReLU v > 0 ? v : slope * v with the product in fp32 -> fp16; the final
// add in fp32 -> fp16.  Compiled with -ffp-contract=off: no product is fused into a sum.
//
// Shared with the fp32 parity engine and the unfused fp16 graph (conv2d between these):
//   srvgg_input_kernel<T>    uint8 -> table -> T NHWC, channels padded with zeros to 16 bytes (4 fp32 / 8 fp16)
//   srvgg_prelu_kernel<T>    per-channel PReLU of [rows][C]
//   srvgg_shuffle_kernel<T>  the tail's epilogue on a stored [B][H][W][48] conv output
// Every index that scales with the batch is 64-bit.
#include <algorithm>
#include <string>

#include "ops.h"
#include "profile.h"

namespace irx {

int g_srvgg_fused = 1;    // irx_set_option("srvgg_fused", 0): the fp16 engine as conv2d + PReLU kernels (A/B)
int g_srvgg_blocks = 0;   // irx_set_option("srvgg_blocks", n): persistent blocks of the body / tail grid (0: one per CU)

namespace {

constexpr int SV_NT = 256;
constexpr int SV_TH = 8, SV_TW = 32;                      // output tile (pixels)
constexpr int SV_HH = SV_TH + 2, SV_HW = SV_TW + 2;       // halo tile
constexpr int SV_PIX_B = 144;                             // LDS bytes per halo pixel: 64 fp16 + 16 pad
constexpr int SV_ROW_B = 1168;                            // LDS bytes per panel row: 576 fp16 + 16 pad
constexpr int SV_PANEL_B = 64 * SV_ROW_B;                 // 74 752
constexpr int SV_HALO_B = SV_HH * SV_HW * SV_PIX_B;       // 48 960
constexpr int SV_CHUNKS = SV_HH * SV_HW * 8;              // 16-byte chunks of a halo tile
constexpr int SV_LD = (SV_CHUNKS + SV_NT - 1) / SV_NT;    // ... per thread
constexpr int SV_LDS = SV_PANEL_B + SV_HALO_B;            // 123 712 B: one block per CU
constexpr int SV_CUS = 256;

// nearest fp16 value.  A plain conversion pair, not Mfma<f16_t>::round with its register pin: nothing here feeds an FMA
// into the conversion (the file is built with -ffp-contract=off), and without the pin the PReLU select stays a
// v_cndmask instead of a divergent branch per element.
__device__ __forceinline__ float r16(float v) { return (float)(f16_t)v; }
__device__ __forceinline__ float prelu16(float v, float slope) {
  const float p = r16(slope * v);
  return v > 0.f ? v : p;
}
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }

struct ConvArgs {
  const f16_t* x;        // [B][H][W][64]
  const f16_t* w;        // [64 or 48][3][3][64]
  const float* bias;     // [64 or 48]
  const float* slope;    // [64] (body)
  f16_t* y;              // [B][H][W][64] (body)
  const uint8_t* img;    // [B][H][W][3] (tail)
  const float* lut;      // [256] (tail)
  uint8_t* out_u8;       // [B][4H][4W][3] (tail)
  float* out_f;          // the same shape or null (tail)
  int H, W, tiles_x, tiles_img;
  long tiles;
};

template <int TAIL>
__global__ __launch_bounds__(SV_NT, 1) void srvgg_conv_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* panel = smem;
  char* halo = smem + SV_PANEL_B;
  constexpr int COUT = TAIL ? 48 : 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int c = tid; c < 64 * 72; c += SV_NT) {
    const int row = c / 72, part = c % 72;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (row < COUT) v = reinterpret_cast<const uint4*>(a.w)[row * 72 + part];
    *reinterpret_cast<uint4*>(panel + row * SV_ROW_B + part * 16) = v;
  }

  uint4 pf[SV_LD];
  auto load = [&](long t) {
    const int b = (int)(t / a.tiles_img), r = (int)(t % a.tiles_img);
    const int y0 = (r / a.tiles_x) * SV_TH - 1, x0 = (r % a.tiles_x) * SV_TW - 1;
    const f16_t* img = a.x + (long)b * a.H * a.W * 64;
#pragma unroll
    for (int i = 0; i < SV_LD; ++i) {
      const int c = tid + i * SV_NT;
      const int pix = c >> 3, part = c & 7;
      const int gy = y0 + pix / SV_HW, gx = x0 + pix % SV_HW;
      pf[i] = make_uint4(0, 0, 0, 0);
      if (c < SV_CHUNKS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
        pf[i] = *reinterpret_cast<const uint4*>(img + ((long)gy * a.W + gx) * 64 + part * 8);
    }
  };

  long t = blockIdx.x;
  if (t < a.tiles) load(t);
  const int r = lane & 31, h = lane >> 5;
  const char* wp = panel + r * SV_ROW_B + h * 16;
  const char* hp = halo + ((wave * 2) * SV_HW + r) * SV_PIX_B + h * 16;
  // this lane's output channels are 32 m + 8 g + 4 h + i in every tile: their bias and slope stay in registers
  float br[2][4][4], sr[2][4][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 32 * m + 8 * g + 4 * h + i;
        br[m][g][i] = c < COUT ? r16(a.bias[c]) : 0.f;
        sr[m][g][i] = TAIL ? 0.f : r16(a.slope[c]);
      }

  for (; t < a.tiles; t += gridDim.x) {
#pragma unroll
    for (int i = 0; i < SV_LD; ++i) {
      const int c = tid + i * SV_NT;
      if (c < SV_CHUNKS) *reinterpret_cast<uint4*>(halo + (c >> 3) * SV_PIX_B + (c & 7) * 16) = pf[i];
    }
    __syncthreads();   // (the first pass: the panel too)
    const long tn = t + gridDim.x;
    if (tn < a.tiles) load(tn);   // in flight while this tile computes

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int wo = (ky * 3 + kx) * 128 + s * 32;
          const uint4 a0 = *reinterpret_cast<const uint4*>(wp + wo);
          const uint4 a1 = *reinterpret_cast<const uint4*>(wp + 32 * SV_ROW_B + wo);
          const uint4 b0 = *reinterpret_cast<const uint4*>(hp + (ky * SV_HW + kx) * SV_PIX_B + s * 32);
          const uint4 b1 = *reinterpret_cast<const uint4*>(hp + ((ky + 1) * SV_HW + kx) * SV_PIX_B + s * 32);
          acc[0][0] = Mfma<f16_t>::m32x32x16(a0, b0, acc[0][0]);
          acc[1][0] = Mfma<f16_t>::m32x32x16(a1, b0, acc[1][0]);
          acc[0][1] = Mfma<f16_t>::m32x32x16(a0, b1, acc[0][1]);
          acc[1][1] = Mfma<f16_t>::m32x32x16(a1, b1, acc[1][1]);
        }

    // D[row = output channel][col = pixel]: lane (r, h) holds pixel r, channels 32 m + 8 g + 4 h + (0..3) in
    // registers 4 g .. 4 g + 3
    const int b = (int)(t / a.tiles_img), rt = (int)(t % a.tiles_img);
    const int px = (rt % a.tiles_x) * SV_TW + r;
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const int py = (rt / a.tiles_x) * SV_TH + wave * 2 + n;
      if (px < a.W && py < a.H) {
        const long pixel = ((long)b * a.H + py) * a.W + px;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int c0 = 32 * m + 8 * g + 4 * h;
            if (TAIL && 32 * m + 8 * g >= COUT) continue;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = r16(acc[m][n][4 * g + i] + br[m][g][i]);
            if (!TAIL) {
#pragma unroll
              for (int i = 0; i < 4; ++i) v[i] = prelu16(v[i], sr[m][g][i]);
              uint2 o;
              o.x = Mfma<f16_t>::pack2(v[0], v[1]);
              o.y = Mfma<f16_t>::pack2(v[2], v[3]);
              *reinterpret_cast<uint2*>(a.y + pixel * 64 + c0) = o;
            } else {
              const int ch = c0 >> 4, ii = (c0 & 15) >> 2;
              const float xin = r16(a.lut[a.img[pixel * 3 + ch]]);
              const long o = (((long)b * 4 * a.H + 4 * py + ii) * (4L * a.W) + 4 * px) * 3 + ch;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float f = r16(v[j] + xin);
                a.out_u8[o + 3 * j] = to_u8(f);
                if (a.out_f) a.out_f[o + 3 * j] = f;
              }
            }
          }
      }
    }
    __syncthreads();   // every wave is done with this halo tile before the next one lands
  }
}

// ---------------------------------------------------------------------------------------------- head
struct HeadArgs {
  const uint8_t* img;
  const float* lut;
  const f16_t* w;        // [64][3][3][cp]
  const float* bias;
  const float* slope;
  f16_t* y;              // [B][H][W][64]
  int H, W, cp;
  long npix;
};

__global__ __launch_bounds__(SV_NT) void srvgg_head_kernel(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float wt[27][64];   // [tap * 3 + channel][output channel]
  __shared__ float tab[256];
  __shared__ float bs[128];
  const int tid = threadIdx.x;
  for (int i = tid; i < 27 * 64; i += SV_NT) {
    const int k = i / 64, co = i % 64;
    wt[k][co] = (float)a.w[(co * 9 + k / 3) * a.cp + k % 3];
  }
  tab[tid] = r16(a.lut[tid]);
  if (tid < 64) {
    bs[tid] = r16(a.bias[tid]);
    bs[64 + tid] = r16(a.slope[tid]);
  }
  __syncthreads();
  const long gid = (long)blockIdx.x * SV_NT + tid;
  const long p = gid >> 3;
  const int c0 = (int)(gid & 7) * 8;
  if (p >= a.npix) return;
  const int x = (int)(p % a.W), y = (int)((p / a.W) % a.H);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int gy = y + ky - 1, gx = x + kx - 1;
      if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) continue;
      const uint8_t* q = a.img + (p + (long)(ky - 1) * a.W + (kx - 1)) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = tab[q[c]];
        const float* wr = &wt[(ky * 3 + kx) * 3 + c][c0];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(v, wr[j], acc[j]);   // fp16 x fp16 is exact in fp32
      }
    }
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float v0 = prelu16(r16(acc[2 * j] + bs[c0 + 2 * j]), bs[64 + c0 + 2 * j]);
    const float v1 = prelu16(r16(acc[2 * j + 1] + bs[c0 + 2 * j + 1]), bs[64 + c0 + 2 * j + 1]);
    o[j] = Mfma<f16_t>::pack2(v0, v1);
  }
  *reinterpret_cast<uint4*>(a.y + p * 64 + c0) = make_uint4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------------------------- shared glue
template <typename T> __device__ __forceinline__ float rnd(float v);
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd<f16_t>(float v) { return r16(v); }

template <typename T>   // a pixel per thread: 3 bytes -> 16 bytes of T (channels 3.. zero)
__global__ __launch_bounds__(SV_NT) void srvgg_input_kernel(const uint8_t* __restrict__ img, long npix,
                                                            const float* __restrict__ lut, uint4* __restrict__ out) {
  const long p = (long)blockIdx.x * SV_NT + threadIdx.x;
  if (p >= npix) return;
  float f[Vec16<T>::N];
#pragma unroll
  for (int i = 0; i < Vec16<T>::N; ++i) f[i] = i < 3 ? lut[img[p * 3 + i]] : 0.f;
  out[p] = Vec16<T>::pack(f);
}

template <typename T>   // 16 bytes per thread; C % Vec16<T>::N == 0; x == y is allowed
__global__ __launch_bounds__(SV_NT) void srvgg_prelu_kernel(const uint4* x, long nvec, int C,
                                                            const float* __restrict__ slope, uint4* y) {
  constexpr int N = Vec16<T>::N;
  const long i = (long)blockIdx.x * SV_NT + threadIdx.x;
  if (i >= nvec) return;
  const int c0 = (int)((i * N) % C);
  float f[N];
  Vec16<T>::unpack(x[i], f);
#pragma unroll
  for (int k = 0; k < N; ++k) f[k] = f[k] > 0.f ? f[k] : rnd<T>(rnd<T>(slope[c0 + k]) * f[k]);
  y[i] = Vec16<T>::pack(f);
}

template <typename T>   // a thread per (input pixel, output row i of its 4 x 4 block): 12 contiguous output bytes
__global__ __launch_bounds__(SV_NT) void srvgg_shuffle_kernel(const T* __restrict__ conv,
                                                              const uint8_t* __restrict__ img, long npix, int H, int W,
                                                              const float* __restrict__ lut, uint8_t* __restrict__ out_u8,
                                                              float* __restrict__ out_f) {
  const long gid = (long)blockIdx.x * SV_NT + threadIdx.x;
  const long p = gid >> 2;
  const int ii = (int)(gid & 3);
  if (p >= npix) return;
  const int x = (int)(p % W), y = (int)((p / W) % H);
  const long b = p / ((long)W * H);
  const long o = ((b * 4 * H + 4 * y + ii) * (4L * W) + 4 * x) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float xin = rnd<T>(lut[img[p * 3 + c]]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float f = rnd<T>(ld_f<T>(conv + p * 48 + 16 * c + 4 * ii + j) + xin);
      out_u8[o + 3 * j + c] = to_u8(f);
      if (out_f) out_f[o + 3 * j + c] = f;
    }
  }
}

std::string kn(const char* k) { return prof_on() ? std::string("irx::(anonymous namespace)::") + k : std::string(); }

unsigned blocks_for(long threads) {
  const long blocks = (threads + SV_NT - 1) / SV_NT;
  IRX_CHECK(threads > 0 && blocks <= 0x7fffffffL, "tensor empty or too large for one launch");
  return (unsigned)blocks;
}

template <int TAIL>
void launch_conv(ConvArgs& a, int B, hipStream_t s) {
  IRX_CHECK(B > 0 && a.H > 0 && a.W > 0, "SRVGG conv: batch and sizes must be positive");
  IRX_CHECK(((uintptr_t)a.x % 16) == 0 && ((uintptr_t)a.w % 16) == 0 && (TAIL || ((uintptr_t)a.y % 16) == 0),
            "SRVGG conv: buffers must be 16-byte aligned");
  a.tiles_x = (a.W + SV_TW - 1) / SV_TW;
  a.tiles_img = a.tiles_x * ((a.H + SV_TH - 1) / SV_TH);
  a.tiles = (long)B * a.tiles_img;
  const long want = g_srvgg_blocks > 0 ? g_srvgg_blocks : SV_CUS;
  const unsigned grid = (unsigned)std::min(want, a.tiles);
  auto k = srvgg_conv_kernel<TAIL>;
  IRX_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, SV_LDS));
  const double flops = 2.0 * B * a.H * a.W * 576.0 * (TAIL ? 48 : 64);
  ProfScope pr(kn(TAIL ? "srvgg_conv_kernel<1>" : "srvgg_conv_kernel<0>"), flops, s);
  hipLaunchKernelGGL(k, dim3(grid), dim3(SV_NT), SV_LDS, s, a);
  IRX_LAUNCH_CHECK();
}

}  // namespace

void srvgg_conv(const void* x, int B, int H, int W, const void* w, const float* bias, const float* slope, void* y,
                hipStream_t s) {
  IRX_CHECK(x && w && bias && slope && y && x != y, "SRVGG conv: null or aliased buffer");
  ConvArgs a{};
  a.x = (const f16_t*)x; a.w = (const f16_t*)w; a.bias = bias; a.slope = slope; a.y = (f16_t*)y;
  a.H = H; a.W = W;
  launch_conv<0>(a, B, s);
}

void srvgg_tail(const void* x, const uint8_t* img, int B, int H, int W, const float* lut, const void* w,
                const float* bias, uint8_t* out_u8, float* out_f, hipStream_t s) {
  IRX_CHECK(x && img && lut && w && bias && out_u8, "SRVGG tail: null buffer");
  ConvArgs a{};
  a.x = (const f16_t*)x; a.w = (const f16_t*)w; a.bias = bias; a.img = img; a.lut = lut;
  a.out_u8 = out_u8; a.out_f = out_f;
  a.H = H; a.W = W;
  launch_conv<1>(a, B, s);
}

void srvgg_head(const uint8_t* img, int B, int H, int W, const float* lut, const void* w, int cp, const float* bias,
                const float* slope, void* y, hipStream_t s) {
  IRX_CHECK(img && lut && w && bias && slope && y, "SRVGG head: null buffer");
  IRX_CHECK(B > 0 && H > 0 && W > 0 && cp >= 3, "SRVGG head: bad shape");
  IRX_CHECK(((uintptr_t)y % 16) == 0, "SRVGG head: output must be 16-byte aligned");
  HeadArgs a{img, lut, (const f16_t*)w, bias, slope, (f16_t*)y, H, W, cp, (long)B * H * W};
  ProfScope pr(kn("srvgg_head_kernel"), 2.0 * a.npix * 27 * 64, s);
  hipLaunchKernelGGL(srvgg_head_kernel, dim3(blocks_for(a.npix * 8)), dim3(SV_NT), 0, s, a);
  IRX_LAUNCH_CHECK();
}

void srvgg_input(int dtype, const uint8_t* img, long npix, const float* lut, void* out, hipStream_t s) {
  IRX_CHECK(dtype == F32 || dtype == F16, "SRVGG: fp32 or fp16");
  IRX_CHECK(img && lut && out && ((uintptr_t)out % 16) == 0, "SRVGG input: null or unaligned buffer");
  const dim3 grid(blocks_for(npix));
  ProfScope pr(kn("srvgg_input_kernel"), 0.0, s);
  if (dtype == F32) hipLaunchKernelGGL(srvgg_input_kernel<float>, grid, dim3(SV_NT), 0, s, img, npix, lut, (uint4*)out);
  else hipLaunchKernelGGL(srvgg_input_kernel<f16_t>, grid, dim3(SV_NT), 0, s, img, npix, lut, (uint4*)out);
  IRX_LAUNCH_CHECK();
}

void srvgg_prelu(int dtype, const void* x, long rows, int C, const float* slope, void* y, hipStream_t s) {
  IRX_CHECK(dtype == F32 || dtype == F16, "SRVGG: fp32 or fp16");
  const int n = dtype == F32 ? 4 : 8;
  IRX_CHECK(x && slope && y && rows > 0 && C > 0 && C % n == 0, "SRVGG PReLU: null buffer or C not 16 bytes of elements");
  IRX_CHECK(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, "SRVGG PReLU: buffers must be 16-byte aligned");
  const long nvec = rows * C / n;
  const dim3 grid(blocks_for(nvec));
  ProfScope pr(kn("srvgg_prelu_kernel"), 0.0, s);
  if (dtype == F32)
    hipLaunchKernelGGL(srvgg_prelu_kernel<float>, grid, dim3(SV_NT), 0, s, (const uint4*)x, nvec, C, slope, (uint4*)y);
  else
    hipLaunchKernelGGL(srvgg_prelu_kernel<f16_t>, grid, dim3(SV_NT), 0, s, (const uint4*)x, nvec, C, slope, (uint4*)y);
  IRX_LAUNCH_CHECK();
}

void srvgg_shuffle_add(int dtype, const void* conv, const uint8_t* img, int B, int H, int W, const float* lut,
                       uint8_t* out_u8, float* out_f, hipStream_t s) {
  IRX_CHECK(dtype == F32 || dtype == F16, "SRVGG: fp32 or fp16");
  IRX_CHECK(conv && img && lut && out_u8 && B > 0 && H > 0 && W > 0, "SRVGG shuffle: null buffer or empty shape");
  const long npix = (long)B * H * W;
  const dim3 grid(blocks_for(npix * 4));
  ProfScope pr(kn("srvgg_shuffle_kernel"), 0.0, s);
  if (dtype == F32)
    hipLaunchKernelGGL(srvgg_shuffle_kernel<float>, grid, dim3(SV_NT), 0, s, (const float*)conv, img, npix, H, W, lut,
                       out_u8, out_f);
  else
    hipLaunchKernelGGL(srvgg_shuffle_kernel<f16_t>, grid, dim3(SV_NT), 0, s, (const f16_t*)conv, img, npix, H, W, lut,
                       out_u8, out_f);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
