// Real-ESRGAN's RRDBNet (RealESRGAN_x4plus.pth: conv_first, 23 RRDBs of three 5-conv dense blocks, conv_body, two
// nearest x2 + conv stages, conv_hr, conv_last; rrdb_host.py / the reference's src/inference.py:335-346, :579-591): the
// kernels of the Rrdb model (models.h).
//
// fp16 engine (the product), two kernels:
//   rrdb_head_kernel       uint8 [B][H][W][3] -> the host's float[256] table rounded to fp16 -> conv_first 3 -> 64 +
//                          bias (no activation) -> fp16, to one or two destinations with a pixel stride.  Plain VALU.
//   rrdb_conv_kernel<M, RES>  every other conv: 3x3, pad 1, Cin in {32, 64, .., 192} read from channels [0, Cin) of a
//                          buffer whose pixels are ldx elements apart, Cout = 32 M written to a channel slice of a
//                          buffer with pixel stride ldy.  A dense block lives in one 192-channel NHWC buffer: conv k
//                          reads channels [0, 32 (k + 1)) and writes [32 (k + 1), 32 (k + 2)); conv5 reads all 192 and
//                          writes channels 0..63 of the next block's buffer with the residuals in its epilogue.  There
//                          is no concatenation and no separate 32- or 64-channel intermediate.
//                          Persistent blocks of 256 threads walk 8 x 32 pixel tiles of one image.  A 192 -> 64 weight
//                          panel (221 KB) does not fit the LDS, so the K loop runs over 32-channel slabs: per slab the
//                          10 x 34 halo tile's 32 channels (pixels padded 64 -> 80 B) and the [Cout][9][32] weight slab
//                          (rows padded 576 -> 592 B) sit in one of two LDS buffers; while the MFMAs run on one buffer
//                          the next slab (of this tile or the first of the block's next tile) is in flight in registers
//                          and is stored to the other buffer after the compute: one barrier per slab.  Both paddings
//                          make the row stride 20 banks (mod 64), so the 16 rows one ds_read_b128 phase covers fall on
//                          16 different 4-bank groups.  LDS: 2 x (32 M x 592 + 340 x 80) = 130 176 B (M = 2) or
//                          92 288 B (M = 1) of the 160 KB: one block per CU.
//                          <M, RES = true>: where the whole [32 M][9][Cin] panel fits next to the two halo slabs
//                          (32 M (18 Cin + 16) + 54 400 <= 163 840 B: Cin <= 160 at M = 1, Cin = 64 at M = 2, i.e.
//                          every conv but the 192 -> 64 one) a block may copy it to LDS once and stream only halo
//                          slabs.  Measured 9 % faster per conv at 32 tiles per block and 8 % slower at 2 (the copy is
//                          not hidden), so the launcher takes it from 16 tiles per block.  Rows are padded by 16 B,
//                          which leaves every row stride at 4, 20, 36 or 52 banks (mod 64): conflict-free as above.
//                          The K order is the same, so the two forms give the same bits (option rrdb_resident, A/B).
//                          A wave owns two tile rows x 32 M output channels (2 M accumulators of 32 x 32),
//                          mfma_f32_32x32x16_f16 with A = weights and B = pixels as in srvgg_conv_kernel.  Per output
//                          element the K order is slab, then tap, then channel: 18 Cin / 32 MFMA steps on one
//                          accumulator, independent of tile, block and batch.  Rows and columns outside the image are
//                          zeros in the halo tile; a tile never spans two images.
//                          `up`: the source is the [H / 2][W / 2] tensor and halo pixel (y, x) loads source pixel
//                          (y >> 1, x >> 1): nearest x2 + conv without the upsampled tensor.
//                          Tail (out_u8): conv_last 64 -> 3 on the M = 1 kernel with rows 3..31 of the slab zero; the
//                          epilogue clamps, * 255, rint -> uint8 [B][H][W][3] (and the unclamped value to out_f).
// Rounding contract of the fp16 engine (rrdb_host.forward(half=True), PyTorch's eager fp16): bias rounded to fp16 when
// read; acc + bias in fp32 -> fp16; LeakyReLU v > 0 ? v : 0.2f * v with the product in fp32 -> fp16 (the slope is the
// fp32 scalar, not an fp16 value: where it differs from srvgg.hip's PReLU); each `t * 0.2 + x` is r16(r16(0.2f t) + x).
// Compiled with -ffp-contract=off.
//
// The glue of the conv2d graph (fp32 parity engine, and fp16 with rrdb_fused = 0): rrdb_gather_kernel<T> (a channel
// prefix of a strided buffer -> dense rows), rrdb_epilogue_kernel<T> (the epilogue above on a stored fp32 conv sum) and
// rrdb_output_kernel<T> (conv_last's end).  Every index that scales with the batch is 64-bit.
#include <algorithm>
#include <string>

#include "ops.h"
#include "profile.h"

namespace irx {

int g_rrdb_fused = 1;    // irx_set_option("rrdb_fused", 0): the fp16 engine as conv2d + glue kernels (A/B)
int g_rrdb_blocks = 0;   // irx_set_option("rrdb_blocks", n): persistent blocks of the conv grid (0: one per CU)
int g_rrdb_resident = 1; // irx_set_option("rrdb_resident", 0 / 2): weight panel never / always in LDS (A/B; same bits)

namespace {

constexpr int RB_NT = 256;
constexpr int RB_TH = 8, RB_TW = 32;                      // output tile (pixels)
constexpr int RB_HH = RB_TH + 2, RB_HW = RB_TW + 2;       // halo tile
constexpr int RB_PIX_B = 80;                              // LDS bytes per halo pixel of a slab: 32 fp16 + 16 pad
constexpr int RB_ROW_B = 592;                             // LDS bytes per weight row of a slab: 9 x 32 fp16 + 16 pad
constexpr int RB_HALO_B = RB_HH * RB_HW * RB_PIX_B;       // 27 200
constexpr int RB_HCHUNKS = RB_HH * RB_HW * 4;             // 16-byte chunks of a halo slab
constexpr int RB_HLD = (RB_HCHUNKS + RB_NT - 1) / RB_NT;  // ... per thread (6)
constexpr int RB_CUS = 256;
constexpr int RB_LDS_MAX = 160 * 1024;
constexpr int RB_RES_TILES = 16;                          // tiles per block from which the panel stays in LDS
constexpr float RB_SLOPE = 0.2f;

template <int M> struct Slab {
  static constexpr int ROWS = 32 * M;
  static constexpr int W_B = ROWS * RB_ROW_B;             // 18 944 / 37 888
  static constexpr int WCHUNKS = ROWS * 36;               // 16-byte chunks of a weight slab
  static constexpr int WLD = (WCHUNKS + RB_NT - 1) / RB_NT;
  static constexpr int BUF_B = W_B + RB_HALO_B;
  static constexpr int LDS = 2 * BUF_B;                   // 92 288 / 130 176
};

__device__ __forceinline__ float r16(float v) { return (float)(f16_t)v; }
__device__ __forceinline__ float lrelu16(float v) {
  const float p = r16(RB_SLOPE * v);
  return v > 0.f ? v : p;
}
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }
__device__ __forceinline__ void unpack4(uint2 u, float* f) {
  const f16x2 lo = __builtin_bit_cast(f16x2, u.x), hi = __builtin_bit_cast(f16x2, u.y);
  f[0] = (float)lo[0]; f[1] = (float)lo[1]; f[2] = (float)hi[0]; f[3] = (float)hi[1];
}

struct KArgs {
  const f16_t* x; int ldx, cin, up;
  const f16_t* w; const float* bias;
  int cout, lrelu;             // valid weight rows / output channels (3 for the tail)
  const f16_t* r1; int ldr1, r1_scaled;
  const f16_t* r2; int ldr2;
  f16_t* y; int ldy;
  uint8_t* out_u8; float* out_f;
  int H, W, Hs, Ws;            // output size; source size (== H, W unless up)
  int tiles_x, tiles_img;
  long tiles;
};

// RES: the whole [32 M][9][Cin] panel stays in LDS for the launch (rows padded by 16 B) and only halo slabs stream
template <int M, bool RES>
__global__ __launch_bounds__(RB_NT, 1) void rrdb_conv_kernel(KArgs a) {
  using S = Slab<M>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ns = a.cin >> 5;
  const int row_b = RES ? a.cin * 18 + 16 : RB_ROW_B;
  auto wbuf = [&](int buf) { return RES ? smem : smem + buf * S::BUF_B; };
  auto hbuf = [&](int buf) { return RES ? smem + S::ROWS * row_b + buf * RB_HALO_B : smem + buf * S::BUF_B + S::W_B; };
  if (RES) {
    const int cpr = a.cin * 18 / 16;             // 16-byte chunks of a panel row
    for (int c = tid; c < S::ROWS * cpr; c += RB_NT) {
      const int row = c / cpr, part = c % cpr;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (row < a.cout) v = *reinterpret_cast<const uint4*>(a.w + (long)row * 9 * a.cin + part * 8);
      *reinterpret_cast<uint4*>(smem + row * row_b + part * 16) = v;
    }
  }

  uint4 ph[RB_HLD], pw[S::WLD];
  auto load = [&](long t, int s) {
    const int b = (int)(t / a.tiles_img), rt = (int)(t % a.tiles_img);
    const int y0 = (rt / a.tiles_x) * RB_TH - 1, x0 = (rt % a.tiles_x) * RB_TW - 1;
    const f16_t* img = a.x + (long)b * a.Hs * a.Ws * a.ldx + s * 32;
#pragma unroll
    for (int i = 0; i < RB_HLD; ++i) {
      const int c = tid + i * RB_NT;
      const int pix = c >> 2, part = c & 3;
      const int gy = y0 + pix / RB_HW, gx = x0 + pix % RB_HW;
      ph[i] = make_uint4(0, 0, 0, 0);
      if (c < RB_HCHUNKS && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
        const int sy = a.up ? gy >> 1 : gy, sx = a.up ? gx >> 1 : gx;
        ph[i] = *reinterpret_cast<const uint4*>(img + ((long)sy * a.Ws + sx) * a.ldx + part * 8);
      }
    }
    if (!RES) {
#pragma unroll
      for (int i = 0; i < S::WLD; ++i) {
        const int c = tid + i * RB_NT;
        const int row = c / 36, q = c % 36;          // q = tap * 4 + part
        pw[i] = make_uint4(0, 0, 0, 0);
        if (c < S::WCHUNKS && row < a.cout)
          pw[i] = *reinterpret_cast<const uint4*>(a.w + ((long)(row * 9 + (q >> 2)) * a.cin + s * 32 + (q & 3) * 8));
      }
    }
  };
  auto store = [&](int buf) {
    char* wb = wbuf(buf);
    char* hb = hbuf(buf);
#pragma unroll
    for (int i = 0; i < RB_HLD; ++i) {
      const int c = tid + i * RB_NT;
      if (c < RB_HCHUNKS) *reinterpret_cast<uint4*>(hb + (c >> 2) * RB_PIX_B + (c & 3) * 16) = ph[i];
    }
    if (!RES) {
#pragma unroll
      for (int i = 0; i < S::WLD; ++i) {
        const int c = tid + i * RB_NT;
        if (c < S::WCHUNKS) *reinterpret_cast<uint4*>(wb + (c / 36) * RB_ROW_B + (c % 36) * 16) = pw[i];
      }
    }
  };

  const int r = lane & 31, h = lane >> 5;
  // this lane's output channels are 32 m + 8 g + 4 h + i in every tile: their bias stays in registers
  float br[M][4][4];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = 32 * m + 8 * g + 4 * h + i;
        br[m][g][i] = c < a.cout ? r16(a.bias[c]) : 0.f;
      }

  long t = blockIdx.x;
  int s = 0, buf = 0;
  if (t < a.tiles) {
    load(t, 0);
    store(0);
  }
  __syncthreads();

  f32x16 acc[M][2];
  while (t < a.tiles) {
    long tn = t;
    int sn = s + 1;
    if (sn == ns) {
      sn = 0;
      tn = t + gridDim.x;
    }
    const bool more = tn < a.tiles;
    if (more) load(tn, sn);   // in flight while this slab computes

    if (s == 0) {
#pragma unroll
      for (int m = 0; m < M; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
    }
    const char* wp = wbuf(buf) + r * row_b + h * 16 + (RES ? s * 64 : 0);
    const char* hp = hbuf(buf) + ((wave * 2) * RB_HW + r) * RB_PIX_B + h * 16;
    const int tap_b = RES ? a.cin * 2 : 64;      // bytes from one tap of a weight row to the next
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int wo = (ky * 3 + kx) * tap_b + kk * 32;
          const uint4 b0 = *reinterpret_cast<const uint4*>(hp + (ky * RB_HW + kx) * RB_PIX_B + kk * 32);
          const uint4 b1 = *reinterpret_cast<const uint4*>(hp + ((ky + 1) * RB_HW + kx) * RB_PIX_B + kk * 32);
#pragma unroll
          for (int m = 0; m < M; ++m) {
            const uint4 am = *reinterpret_cast<const uint4*>(wp + m * 32 * row_b + wo);
            acc[m][0] = Mfma<f16_t>::m32x32x16(am, b0, acc[m][0]);
            acc[m][1] = Mfma<f16_t>::m32x32x16(am, b1, acc[m][1]);
          }
        }

    if (s == ns - 1) {
      // D[row = output channel][col = pixel]: lane (r, h) holds pixel r, channels 32 m + 8 g + 4 h + (0..3) in
      // registers 4 g .. 4 g + 3
      const int b = (int)(t / a.tiles_img), rt = (int)(t % a.tiles_img);
      const int px = (rt % a.tiles_x) * RB_TW + r;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int py = (rt / a.tiles_x) * RB_TH + wave * 2 + n;
        if (px < a.W && py < a.H) {
          const long pixel = ((long)b * a.H + py) * a.W + px;
          if (a.out_u8) {
            if (h == 0) {
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                const float f = r16(acc[0][n][i] + br[0][0][i]);
                a.out_u8[pixel * 3 + i] = to_u8(f);
                if (a.out_f) a.out_f[pixel * 3 + i] = f;
              }
            }
          } else {
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const int c0 = 32 * m + 8 * g + 4 * h;
                float v[4], q[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = r16(acc[m][n][4 * g + i] + br[m][g][i]);
                if (a.lrelu) {
#pragma unroll
                  for (int i = 0; i < 4; ++i) v[i] = lrelu16(v[i]);
                }
                if (a.r1) {
                  unpack4(*reinterpret_cast<const uint2*>(a.r1 + pixel * a.ldr1 + c0), q);
#pragma unroll
                  for (int i = 0; i < 4; ++i) v[i] = r16((a.r1_scaled ? r16(RB_SLOPE * v[i]) : v[i]) + q[i]);
                }
                if (a.r2) {
                  unpack4(*reinterpret_cast<const uint2*>(a.r2 + pixel * a.ldr2 + c0), q);
#pragma unroll
                  for (int i = 0; i < 4; ++i) v[i] = r16(r16(RB_SLOPE * v[i]) + q[i]);
                }
                uint2 o;
                o.x = Mfma<f16_t>::pack2(v[0], v[1]);
                o.y = Mfma<f16_t>::pack2(v[2], v[3]);
                *reinterpret_cast<uint2*>(a.y + pixel * a.ldy + c0) = o;
              }
          }
        }
      }
    }
    if (more) store(buf ^ 1);   // every wave left that buffer before the last barrier
    __syncthreads();
    buf ^= 1;
    t = tn;
    s = sn;
  }
}

// ---------------------------------------------------------------------------------------------- head
struct HeadArgs {
  const uint8_t* img;
  const float* lut;
  const f16_t* w;        // [64][3][3][cp]
  const float* bias;
  f16_t* y; int ldy;
  f16_t* y2; int ldy2;   // or null
  int H, W, cp;
  long npix;
};

__global__ __launch_bounds__(RB_NT) void rrdb_head_kernel(HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float wt[27][64];   // [tap * 3 + channel][output channel]
  __shared__ float tab[256];
  __shared__ float bs[64];
  const int tid = threadIdx.x;
  for (int i = tid; i < 27 * 64; i += RB_NT) {
    const int k = i / 64, co = i % 64;
    wt[k][co] = (float)a.w[(co * 9 + k / 3) * a.cp + k % 3];
  }
  tab[tid] = r16(a.lut[tid]);
  if (tid < 64) bs[tid] = r16(a.bias[tid]);
  __syncthreads();
  const long gid = (long)blockIdx.x * RB_NT + tid;
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
  for (int j = 0; j < 4; ++j)
    o[j] = Mfma<f16_t>::pack2(r16(acc[2 * j] + bs[c0 + 2 * j]), r16(acc[2 * j + 1] + bs[c0 + 2 * j + 1]));
  const uint4 v = make_uint4(o[0], o[1], o[2], o[3]);
  *reinterpret_cast<uint4*>(a.y + p * a.ldy + c0) = v;
  if (a.y2) *reinterpret_cast<uint4*>(a.y2 + p * a.ldy2 + c0) = v;
}

// ---------------------------------------------------------------------------------------------- glue
template <typename T> __device__ __forceinline__ float rnd(float v);
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd<f16_t>(float v) { return r16(v); }

template <typename T>   // 16 bytes per thread
__global__ __launch_bounds__(RB_NT) void rrdb_gather_kernel(const uint4* __restrict__ x, long ldv, long nvec, int cv,
                                                            uint4* __restrict__ y) {
  const long i = (long)blockIdx.x * RB_NT + threadIdx.x;
  if (i >= nvec) return;
  y[i] = x[(i / cv) * ldv + i % cv];
}

struct EpiArgs {
  const float* acc; const float* bias;
  const void* r1; const void* r2; void* y;
  long nvec;
  int C, lrelu, ldr1, r1_scaled, ldr2, ldy;
};

template <typename T>   // 16 bytes of T per thread
__global__ __launch_bounds__(RB_NT) void rrdb_epilogue_kernel(EpiArgs a) {
  constexpr int N = Vec16<T>::N;
  const long i = (long)blockIdx.x * RB_NT + threadIdx.x;
  if (i >= a.nvec) return;
  const int cv = a.C / N;
  const long row = i / cv;
  const int c0 = (int)(i % cv) * N;
  float v[N], q[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    v[k] = rnd<T>(a.acc[row * a.C + c0 + k] + rnd<T>(a.bias[c0 + k]));
    if (a.lrelu) {
      const float p = rnd<T>(RB_SLOPE * v[k]);
      v[k] = v[k] > 0.f ? v[k] : p;
    }
  }
  if (a.r1) {
    Vec16<T>::unpack(*reinterpret_cast<const uint4*>((const T*)a.r1 + row * a.ldr1 + c0), q);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = rnd<T>((a.r1_scaled ? rnd<T>(RB_SLOPE * v[k]) : v[k]) + q[k]);
  }
  if (a.r2) {
    Vec16<T>::unpack(*reinterpret_cast<const uint4*>((const T*)a.r2 + row * a.ldr2 + c0), q);
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = rnd<T>(rnd<T>(RB_SLOPE * v[k]) + q[k]);
  }
  *reinterpret_cast<uint4*>((T*)a.y + row * a.ldy + c0) = Vec16<T>::pack(v);
}

template <typename T>   // a pixel per thread
__global__ __launch_bounds__(RB_NT) void rrdb_output_kernel(const float* __restrict__ acc, int ldacc, long rows,
                                                            const float* __restrict__ bias,
                                                            uint8_t* __restrict__ out_u8, float* __restrict__ out_f) {
  const long p = (long)blockIdx.x * RB_NT + threadIdx.x;
  if (p >= rows) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float f = rnd<T>(acc[p * ldacc + c] + rnd<T>(bias[c]));
    out_u8[p * 3 + c] = to_u8(f);
    if (out_f) out_f[p * 3 + c] = f;
  }
}

std::string kn(const char* k) { return prof_on() ? std::string("irx::(anonymous namespace)::") + k : std::string(); }

unsigned blocks_for(long threads) {
  const long blocks = (threads + RB_NT - 1) / RB_NT;
  IRX_CHECK(threads > 0 && blocks <= 0x7fffffffL, "tensor empty or too large for one launch");
  return (unsigned)blocks;
}

template <int M, bool RES>
void launch_conv(KArgs& a, int B, int lds, hipStream_t s) {
  const long want = g_rrdb_blocks > 0 ? g_rrdb_blocks : RB_CUS;
  const unsigned grid = (unsigned)std::min(want, a.tiles);
  auto k = rrdb_conv_kernel<M, RES>;
  IRX_HIP(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, RES ? RB_LDS_MAX : lds));
  const double flops = 2.0 * B * a.H * a.W * 9.0 * a.cin * a.cout;
  ProfScope pr(kn(M == 2 ? (RES ? "rrdb_conv_kernel<2, true>" : "rrdb_conv_kernel<2, false>")
                         : (RES ? "rrdb_conv_kernel<1, true>" : "rrdb_conv_kernel<1, false>")), flops, s);
  hipLaunchKernelGGL(k, dim3(grid), dim3(RB_NT), lds, s, a);
  IRX_LAUNCH_CHECK();
}

bool al(const void* p, int n) { return ((uintptr_t)p % n) == 0; }

}  // namespace

void rrdb_conv(const RrdbConv& c, hipStream_t s) {
  const bool tail = c.out_u8 != nullptr;
  IRX_CHECK(c.x && c.w && c.bias && (tail || c.y), "RRDB conv: null buffer");
  IRX_CHECK(c.B > 0 && c.H > 0 && c.W > 0, "RRDB conv: batch and sizes must be positive");
  IRX_CHECK(c.cin >= 32 && c.cin <= 192 && c.cin % 32 == 0, "RRDB conv: Cin must be a multiple of 32 in [32, 192]");
  IRX_CHECK(tail ? c.cout == 3 : (c.cout == 32 || c.cout == 64), "RRDB conv: Cout must be 32 or 64 (3 for the tail)");
  IRX_CHECK(c.ldx >= c.cin && c.ldx % 8 == 0 && al(c.x, 16) && al(c.w, 16),
            "RRDB conv: source rows and weights must be 16-byte aligned");
  IRX_CHECK(!c.up || (c.H % 2 == 0 && c.W % 2 == 0), "RRDB conv: an upsampled output has even sizes");
  IRX_CHECK((long)c.B * c.H * c.W <= 0x7fffffffL, "RRDB conv: batch x image too large for one call");
  if (!tail) {
    IRX_CHECK(c.ldy >= c.cout && c.ldy % 4 == 0 && al(c.y, 8), "RRDB conv: output slice must be 8-byte aligned");
    IRX_CHECK(!c.r1 || (c.ldr1 >= c.cout && c.ldr1 % 4 == 0 && al(c.r1, 8)), "RRDB conv: res1 must be 8-byte aligned");
    IRX_CHECK(!c.r2 || (c.ldr2 >= c.cout && c.ldr2 % 4 == 0 && al(c.r2, 8)), "RRDB conv: res2 must be 8-byte aligned");
    // the written slice must not overlap the channels that are read: other blocks still load them as halo
    const char* xs = (const char*)c.x;
    const char* ys = (const char*)c.y;
    const long span_x = ((long)c.B * (c.up ? c.H / 2 : c.H) * (c.up ? c.W / 2 : c.W) - 1) * c.ldx * 2 + c.cin * 2;
    const long span_y = ((long)c.B * c.H * c.W - 1) * c.ldy * 2 + c.cout * 2;
    const bool apart = ys + span_y <= xs || xs + span_x <= ys;
    const bool interleaved = !c.up && c.ldx == c.ldy && ys >= xs + c.cin * 2 && ys + c.cout * 2 <= xs + c.ldx * 2;
    IRX_CHECK(apart || interleaved, "RRDB conv: the output slice overlaps the channels that are read");
  } else {
    IRX_CHECK(!c.r1 && !c.r2 && !c.lrelu, "RRDB conv: the tail has no activation and no residual");
  }
  KArgs a{};
  a.x = (const f16_t*)c.x; a.ldx = c.ldx; a.cin = c.cin; a.up = c.up ? 1 : 0;
  a.w = (const f16_t*)c.w; a.bias = c.bias; a.cout = c.cout; a.lrelu = c.lrelu;
  a.r1 = (const f16_t*)c.r1; a.ldr1 = c.ldr1; a.r1_scaled = c.r1_scaled;
  a.r2 = (const f16_t*)c.r2; a.ldr2 = c.ldr2;
  a.y = (f16_t*)c.y; a.ldy = c.ldy; a.out_u8 = c.out_u8; a.out_f = c.out_f;
  a.H = c.H; a.W = c.W; a.Hs = c.up ? c.H / 2 : c.H; a.Ws = c.up ? c.W / 2 : c.W;
  a.tiles_x = (a.W + RB_TW - 1) / RB_TW;
  a.tiles_img = a.tiles_x * ((a.H + RB_TH - 1) / RB_TH);
  a.tiles = (long)c.B * a.tiles_img;
  // the whole panel next to two halo slabs where that fits the LDS: Cin <= 160 at 32 rows, Cin = 64 at 64 rows
  const int rows = c.cout == 64 ? 64 : 32;
  const int res_lds = rows * (c.cin * 18 + 16) + 2 * RB_HALO_B;
  // ... and where a block walks enough tiles to pay for the panel copy (measured, DESIGN section 24: a gain from 32
  // tiles per block, a loss at 2); rrdb_resident = 2: wherever it fits, 0: never
  const long grid = std::min((long)(g_rrdb_blocks > 0 ? g_rrdb_blocks : RB_CUS), a.tiles);
  const bool res = res_lds <= RB_LDS_MAX &&
                   (g_rrdb_resident == 2 || (g_rrdb_resident == 1 && a.tiles >= RB_RES_TILES * grid));
  if (rows == 64) {
    if (res) launch_conv<2, true>(a, c.B, res_lds, s);
    else launch_conv<2, false>(a, c.B, Slab<2>::LDS, s);
  } else {
    if (res) launch_conv<1, true>(a, c.B, res_lds, s);
    else launch_conv<1, false>(a, c.B, Slab<1>::LDS, s);
  }
}

void rrdb_head(const uint8_t* img, int B, int H, int W, const float* lut, const void* w, int cp, const float* bias,
               void* y, int ldy, void* y2, int ldy2, hipStream_t s) {
  IRX_CHECK(img && lut && w && bias && y, "RRDB head: null buffer");
  IRX_CHECK(B > 0 && H > 0 && W > 0 && cp >= 3, "RRDB head: bad shape");
  IRX_CHECK(al(y, 16) && ldy >= 64 && ldy % 8 == 0 && (!y2 || (al(y2, 16) && ldy2 >= 64 && ldy2 % 8 == 0)),
            "RRDB head: outputs must be 16-byte aligned");
  HeadArgs a{img, lut, (const f16_t*)w, bias, (f16_t*)y, ldy, (f16_t*)y2, ldy2, H, W, cp, (long)B * H * W};
  ProfScope pr(kn("rrdb_head_kernel"), 2.0 * a.npix * 27 * 64, s);
  hipLaunchKernelGGL(rrdb_head_kernel, dim3(blocks_for(a.npix * 8)), dim3(RB_NT), 0, s, a);
  IRX_LAUNCH_CHECK();
}

void rrdb_gather(int dtype, const void* x, int ldx, long rows, int C, void* y, hipStream_t s) {
  IRX_CHECK(dtype == F32 || dtype == F16, "RRDB: fp32 or fp16");
  const int n = dtype == F32 ? 4 : 8;
  IRX_CHECK(x && y && rows > 0 && C > 0 && C % n == 0 && ldx >= C && ldx % n == 0 && al(x, 16) && al(y, 16),
            "RRDB gather: null, unaligned or ragged buffer");
  const long nvec = rows * (C / n);
  ProfScope pr(kn("rrdb_gather_kernel"), 0.0, s);
  hipLaunchKernelGGL(rrdb_gather_kernel<float>, dim3(blocks_for(nvec)), dim3(RB_NT), 0, s, (const uint4*)x,
                     (long)(ldx / n), nvec, C / n, (uint4*)y);
  IRX_LAUNCH_CHECK();
}

void rrdb_epilogue(int dtype, const float* acc, long rows, int C, const float* bias, int lrelu, const void* r1,
                   int ldr1, int r1_scaled, const void* r2, int ldr2, void* y, int ldy, hipStream_t s) {
  IRX_CHECK(dtype == F32 || dtype == F16, "RRDB: fp32 or fp16");
  const int n = dtype == F32 ? 4 : 8;
  IRX_CHECK(acc && bias && y && rows > 0 && C > 0 && C % n == 0, "RRDB epilogue: null buffer or ragged C");
  IRX_CHECK(al(y, 16) && ldy % n == 0 && (!r1 || (al(r1, 16) && ldr1 % n == 0)) &&
                (!r2 || (al(r2, 16) && ldr2 % n == 0)),
            "RRDB epilogue: buffers must be 16-byte aligned");
  EpiArgs a{acc, bias, r1, r2, y, rows * (C / n), C, lrelu, ldr1, r1_scaled, ldr2, ldy};
  const dim3 grid(blocks_for(a.nvec));
  ProfScope pr(kn("rrdb_epilogue_kernel"), 0.0, s);
  if (dtype == F32) hipLaunchKernelGGL(rrdb_epilogue_kernel<float>, grid, dim3(RB_NT), 0, s, a);
  else hipLaunchKernelGGL(rrdb_epilogue_kernel<f16_t>, grid, dim3(RB_NT), 0, s, a);
  IRX_LAUNCH_CHECK();
}

void rrdb_output(int dtype, const float* acc, int ldacc, long rows, const float* bias, uint8_t* out_u8, float* out_f,
                 hipStream_t s) {
  IRX_CHECK(dtype == F32 || dtype == F16, "RRDB: fp32 or fp16");
  IRX_CHECK(acc && bias && out_u8 && rows > 0 && ldacc >= 3, "RRDB output: null buffer or empty shape");
  const dim3 grid(blocks_for(rows));
  ProfScope pr(kn("rrdb_output_kernel"), 0.0, s);
  if (dtype == F32)
    hipLaunchKernelGGL(rrdb_output_kernel<float>, grid, dim3(RB_NT), 0, s, acc, ldacc, rows, bias, out_u8, out_f);
  else
    hipLaunchKernelGGL(rrdb_output_kernel<f16_t>, grid, dim3(RB_NT), 0, s, acc, ldacc, rows, bias, out_u8, out_f);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
