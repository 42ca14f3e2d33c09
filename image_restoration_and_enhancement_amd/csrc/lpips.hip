// LPIPS (AlexNet) around the fp32 conv trunk (lpips_host.py / the reference's src/metrics.py:97-111): the three
// kernels the metric needs besides the five convolutions, which go through gemm()'s exact-f32 path.
//
//   lpips_input_kernel      uint8 [B][H][W][3] of pred and of gt -> fp32 NHWC4 [2B][H][W][4] (pred images first), each
//                           value read from the host's float[256][3] table of the scaling layer (lpips_host.input_table):
//                           the trunk's input is bit-equal to the restatement's.  Channel 3 is 0 (conv1's padded Cin).
//   lpips_relu_pool_kernel  ReLU, then the max over a WIN x WIN window at stride S with no padding, fp32 NHWC, a
//                           float4 of channels per thread: (3, 2) the two pools, (1, 1) the ReLU copy in front of
//                           conv4 / conv5 (the convs store their pre-ReLU output).
//   lpips_head_kernel       one tap: a wave per pixel holds the (ReLU'd) channels of the pred pixel and of the gt pixel
//                           in registers (channel j * 64 + lane, at most 6 per lane and image), reduces the two
//                           squared norms across the wave, and forms  sum_c w_c (a_c / (|a| + eps) - b_c / (|b| + eps))^2
//                           in a second pass over the registers — the difference first, never the expanded square, which
//                           cancels for near-identical images.  A wave adds its pixels' values in fp64 in pixel order,
//                           the block's four waves are added by a fixed tree, one partial per block goes to the workspace.
//   lpips_finalize_kernel   one block per image: thread t adds partials t, t + 256, ... in that order, the fixed tree,
//                           divide by the pixel count (metrics.hip's rule).  The last tap also writes the total as the
//                           sum of the five taps in index order.
// No atomics: the same bits on every run; the tiling of a tap depends on its h x w alone, so an image's head sums do
// not depend on its position in the batch or on the batch size.
#include <string>

#include "ops.h"
#include "profile.h"

namespace irx {
namespace {

constexpr int LP_NT = 256;
constexpr int LP_WAVES = LP_NT / 64;
// pixels per head block (4 per wave): the deep taps have few pixels (31 x 31 at 512 x 512), and a wave's pixels are a
// serial chain of loads and two wave reductions each, so short chains over many blocks (64 per block: 17 us per tap at
// 512 x 512, batch 1)
constexpr int LP_PPB = 16;
constexpr float LP_EPS = 1e-10f;

// ---------------------------------------------------------------------------------------------- input
// four pixels (12 bytes, three dwords) per thread; n = pixels of one source (B * H * W)
__global__ __launch_bounds__(LP_NT) void lpips_input_kernel(const uint8_t* __restrict__ pred,
                                                            const uint8_t* __restrict__ gt, long n,
                                                            const float* __restrict__ lut, float4* __restrict__ out) {
  __shared__ float tab[256 * 3];
  for (int i = threadIdx.x; i < 256 * 3; i += LP_NT) tab[i] = lut[i];
  __syncthreads();
  const long groups = (n + 3) / 4;
  const long g = (long)blockIdx.x * LP_NT + threadIdx.x;
  if (g >= groups) return;
  const uint8_t* src = blockIdx.y ? gt : pred;
  const long p0 = g * 4;
  const int np = (int)min(4L, n - p0);
  const uint8_t* s = src + p0 * 3;
  uint32_t w[3] = {0, 0, 0};
  if (np == 4 && ((uintptr_t)s & 3) == 0) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(s);
    w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
  } else {
    for (int i = 0; i < np * 3; ++i) w[i >> 2] |= (uint32_t)s[i] << (8 * (i & 3));
  }
  float4* o = out + (long)blockIdx.y * n + p0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < np) {
      const int b0 = 3 * i, b1 = 3 * i + 1, b2 = 3 * i + 2;
      const uint32_t r = (w[b0 >> 2] >> (8 * (b0 & 3))) & 255u;
      const uint32_t gg = (w[b1 >> 2] >> (8 * (b1 & 3))) & 255u;
      const uint32_t b = (w[b2 >> 2] >> (8 * (b2 & 3))) & 255u;
      o[i] = make_float4(tab[r * 3], tab[gg * 3 + 1], tab[b * 3 + 2], 0.f);
    }
  }
}

// ---------------------------------------------------------------------------------------------- ReLU + max pool
struct PoolArgs {
  const float4* x;
  float4* y;
  int H, W, Ho, Wo, C4;     // C4 = C / 4
  long total;               // N * Ho * Wo * C4
};

__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }

template <int WIN, int S>
__global__ __launch_bounds__(LP_NT) void lpips_relu_pool_kernel(PoolArgs a) {
  const long i = (long)blockIdx.x * LP_NT + threadIdx.x;
  if (i >= a.total) return;
  const int c = (int)(i % a.C4);
  long r = i / a.C4;
  const int ox = (int)(r % a.Wo);
  r /= a.Wo;
  const int oy = (int)(r % a.Ho);
  const long n = r / a.Ho;
  // the window lies inside the image: (Ho - 1) * S + WIN <= H by the output size formula
  const float4* p = a.x + ((n * a.H + (long)oy * S) * a.W + (long)ox * S) * a.C4 + c;
  float4 m = make_float4(0.f, 0.f, 0.f, 0.f);        // max(relu(.)) starts from relu's floor
#pragma unroll
  for (int dy = 0; dy < WIN; ++dy)
#pragma unroll
    for (int dx = 0; dx < WIN; ++dx) {
      const float4 v = p[((long)dy * a.W + dx) * a.C4];
      m.x = fmaxf(m.x, relu(v.x));
      m.y = fmaxf(m.y, relu(v.y));
      m.z = fmaxf(m.z, relu(v.z));
      m.w = fmaxf(m.w, relu(v.w));
    }
  a.y[i] = m;
}

// ---------------------------------------------------------------------------------------------- head
struct HeadArgs {
  const float* f;       // [2B][hw][C] pre-ReLU features, pred images first
  const float* w;       // [C] lin weights
  double* part;         // [B][nblk]
  int B, hw, nblk;
};

__device__ __forceinline__ float wave_sum(float v) {   // butterfly: every lane ends with the same sum, same order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int NPL>   // channels per lane: C = 64 * NPL
__global__ __launch_bounds__(LP_NT) void lpips_head_kernel(HeadArgs a) {
  constexpr int C = 64 * NPL;
  __shared__ double red[LP_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const float* fa = a.f + (long)b * a.hw * C;
  const float* fb = a.f + (long)(a.B + b) * a.hw * C;
  float wt[NPL];
#pragma unroll
  for (int j = 0; j < NPL; ++j) wt[j] = a.w[j * 64 + lane];
  const int p0 = blockIdx.x * LP_PPB;
  const int p1 = min(p0 + LP_PPB, a.hw);
  double acc = 0.0;
  for (int p = p0 + wave; p < p1; p += LP_WAVES) {
    float x[NPL], y[NPL];
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      x[j] = relu(fa[(long)p * C + j * 64 + lane]);
      y[j] = relu(fb[(long)p * C + j * 64 + lane]);
      sa += x[j] * x[j];
      sb += y[j] * y[j];
    }
    const float na = sqrtf(wave_sum(sa)) + LP_EPS, nb = sqrtf(wave_sum(sb)) + LP_EPS;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
      const float d = x[j] / na - y[j] / nb;
      v += wt[j] * (d * d);
    }
    acc += (double)wave_sum(v);
  }
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.part[(long)b * a.nblk + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// lay: [B][5] in the workspace (always written); layers: the caller's [B][5] or null; total: [B], written by tap 4
__global__ __launch_bounds__(LP_NT) void lpips_finalize_kernel(const double* part, int nblk, double npix, int tap,
                                                               double* lay, double* layers, double* total) {
  __shared__ double red[LP_NT];
  const int tid = threadIdx.x;
  const double* w = part + (long)blockIdx.x * nblk;
  double s = 0.0;
  for (int i = tid; i < nblk; i += LP_NT) s += w[i];
  red[tid] = s;
  __syncthreads();
#pragma unroll
  for (int h = LP_NT / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    const double v = red[0] / npix;
    double* l = lay + (long)blockIdx.x * 5;
    l[tap] = v;
    if (layers) layers[(long)blockIdx.x * 5 + tap] = v;
    if (tap == 4) total[blockIdx.x] = (((l[0] + l[1]) + l[2]) + l[3]) + v;
  }
}

std::string kn(const char* k) { return prof_on() ? std::string("irx::(anonymous namespace)::") + k : std::string(); }

}  // namespace

void lpips_input(const uint8_t* pred, const uint8_t* gt, int B, int H, int W, const float* lut, float* out,
                 hipStream_t s) {
  const long n = (long)B * H * W;
  const long blocks = ((n + 3) / 4 + LP_NT - 1) / LP_NT;
  IRX_CHECK(n > 0 && blocks <= 0x7fffffffL, "image batch empty or too large for one launch");
  ProfScope pr(kn("lpips_input_kernel"), 0.0, s);
  hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)blocks, 2), dim3(LP_NT), 0, s, pred, gt, n, lut, (float4*)out);
  IRX_LAUNCH_CHECK();
}

void lpips_relu_pool(const float* x, int N, int H, int W, int C, int win, int stride, float* y, hipStream_t s) {
  IRX_CHECK((win == 3 && stride == 2) || (win == 1 && stride == 1), "ReLU + pool: (window, stride) (3, 2) or (1, 1)");
  IRX_CHECK(N > 0 && C > 0 && C % 4 == 0 && H >= win && W >= win, "ReLU + pool: C % 4 == 0, H, W >= window");
  PoolArgs a;
  a.x = (const float4*)x; a.y = (float4*)y;
  a.H = H; a.W = W; a.Ho = (H - win) / stride + 1; a.Wo = (W - win) / stride + 1; a.C4 = C / 4;
  a.total = (long)N * a.Ho * a.Wo * a.C4;
  const long blocks = (a.total + LP_NT - 1) / LP_NT;
  IRX_CHECK(blocks <= 0x7fffffffL, "tensor too large for one launch");
  ProfScope pr(kn("lpips_relu_pool_kernel"), 0.0, s);
  if (win == 3) hipLaunchKernelGGL((lpips_relu_pool_kernel<3, 2>), dim3((unsigned)blocks), dim3(LP_NT), 0, s, a);
  else hipLaunchKernelGGL((lpips_relu_pool_kernel<1, 1>), dim3((unsigned)blocks), dim3(LP_NT), 0, s, a);
  IRX_LAUNCH_CHECK();
}

int lpips_head_blocks(int hw) { return (hw + LP_PPB - 1) / LP_PPB; }

void lpips_head(const float* f, int B, int hw, int C, const float* w, int tap, double* part, double* lay,
                double* layers, double* total, hipStream_t s) {
  IRX_CHECK(B > 0 && B <= 65535 && hw > 0 && tap >= 0 && tap < 5, "LPIPS head: bad shape");
  HeadArgs a;
  a.f = f; a.w = w; a.part = part; a.B = B; a.hw = hw; a.nblk = lpips_head_blocks(hw);
  const dim3 grid(a.nblk, B);
  {
    ProfScope pr(kn("lpips_head_kernel"), 0.0, s);
    switch (C) {
      case 64: hipLaunchKernelGGL(lpips_head_kernel<1>, grid, dim3(LP_NT), 0, s, a); break;
      case 192: hipLaunchKernelGGL(lpips_head_kernel<3>, grid, dim3(LP_NT), 0, s, a); break;
      case 256: hipLaunchKernelGGL(lpips_head_kernel<4>, grid, dim3(LP_NT), 0, s, a); break;
      case 384: hipLaunchKernelGGL(lpips_head_kernel<6>, grid, dim3(LP_NT), 0, s, a); break;
      default: throw Error("LPIPS head: C must be 64, 192, 256 or 384");
    }
    IRX_LAUNCH_CHECK();
  }
  ProfScope pr(kn("lpips_finalize_kernel"), 0.0, s);
  hipLaunchKernelGGL(lpips_finalize_kernel, dim3(B), dim3(LP_NT), 0, s, part, a.nblk, (double)hw, tap, lay, layers,
                     total);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
