// FID features (InceptionV3) around the fp32 conv trunk (fid_host.py / the reference's src/metrics.py:70-80, 150-223):
// the kernels the metric needs besides the 94 convolutions, which go through gemm()'s exact-f32 path.
//
//   fid_input_kernel       one uint8 [H][W][3] image -> fp32 [299][299][4]: v / 255, the antialiased bilinear resize as
//                          ATen's _upsample_bilinear2d_aa does it (width pass first, then the height pass, each output
//                          `t = src[0] * w[0]; t += src[j] * w[j]` over the host's tap tables), (t - mean) / std, channel
//                          3 zero.  A block owns a 32 x 8 output tile: the width pass of the source rows the tile needs
//                          goes to LDS 32 rows at a time, and each thread carries its pixel's three height sums across
//                          the chunks in tap order, so the LDS footprint does not grow with the down-scale.
//   fid_bn_relu_kernel     y = max(x * a_c + b_c, 0), a float4 of channels per thread, output rows `ldo` floats apart
//                          (a branch's last unit writes its slice of the block's concat buffer).
//   fid_avgpool3_kernel    3 x 3 / 1 / pad 1, the taps inside the image added row by row, left to right, then / 9.
//   fid_maxpool3s2_kernel  3 x 3 / 2 without padding, output rows `ldo` floats apart.
//   fid_gap_kernel         a thread per (image, channel): the pixels added in order, one division.
// No atomics and no cross-thread sums: the same bits on every run, and nothing depends on the batch size or position.
#include <string>

#include "ops.h"
#include "profile.h"

namespace irx {
namespace {

constexpr int FD_NT = 256;
constexpr int IN_TX = 32, IN_TY = 8;     // output tile (IN_TX * IN_TY == FD_NT: a thread per output pixel)
constexpr int IN_R = 32;                 // source rows per LDS chunk
static_assert(IN_TX * IN_TY == FD_NT, "one thread per output pixel of the tile");

struct InputArgs {
  const uint8_t* img;
  int H, W;
  const int *xs, *xn, *ys, *yn;
  const float *xw, *yw;
  int kx, ky;
  float4* out;
};

__global__ __launch_bounds__(FD_NT) void fid_input_kernel(InputArgs a) {
  __shared__ float mid[IN_R][IN_TX][3];          // 12 KiB: the width pass of one chunk of source rows
  __shared__ int sxs[IN_TX], sxn[IN_TX];
  const int tid = threadIdx.x;
  const int ox0 = blockIdx.x * IN_TX, oy0 = blockIdx.y * IN_TY;
  if (tid < IN_TX) {
    const int ox = min(ox0 + tid, FID_SIDE - 1);
    const int s = min(max(a.xs[ox], 0), a.W - 1);      // a table entry never leaves the image
    sxs[tid] = s;
    sxn[tid] = max(min(min(a.xn[ox], a.kx), a.W - s), 0);
  }
  const int tx = tid % IN_TX, ty = tid / IN_TX;
  const int ox = ox0 + tx, oy = oy0 + ty;
  const bool live = ox < FID_SIDE && oy < FID_SIDE;
  const int oyc = min(oy, FID_SIDE - 1);
  const int y0 = min(max(a.ys[oyc], 0), a.H - 1);
  const int yn = max(min(min(a.yn[oyc], a.ky), a.H - y0), 0);
  const float* wy = a.yw + (long)oyc * a.ky;
  // the source rows of the whole tile (every thread computes the same two numbers)
  int rlo = a.H, rhi = 0;
  for (int i = 0; i < IN_TY; ++i) {
    const int r = min(oy0 + i, FID_SIDE - 1);
    const int s = min(max(a.ys[r], 0), a.H - 1);
    const int n = max(min(min(a.yn[r], a.ky), a.H - s), 0);
    rlo = min(rlo, s);
    rhi = max(rhi, s + n);
  }
  float acc[3] = {0.f, 0.f, 0.f};
  __syncthreads();
  for (int c0 = rlo; c0 < rhi; c0 += IN_R) {
    const int nr = min(IN_R, rhi - c0);
    for (int e = tid; e < nr * IN_TX * 3; e += FD_NT) {
      const int c = e % 3, x = (e / 3) % IN_TX, r = e / (3 * IN_TX);
      const uint8_t* src = a.img + ((long)(c0 + r) * a.W + sxs[x]) * 3 + c;
      const float* w = a.xw + (long)min(ox0 + x, FID_SIDE - 1) * a.kx;
      const int n = sxn[x];
      float t = 0.f;
      if (n > 0) t = ((float)src[0] / 255.0f) * w[0];
      for (int j = 1; j < n; ++j) t += ((float)src[j * 3] / 255.0f) * w[j];
      mid[r][x][c] = t;
    }
    __syncthreads();
    // this pixel's taps that fall into the chunk, in tap order
    const int j0 = max(c0 - y0, 0), j1 = min(c0 + nr - y0, yn);
    for (int j = j0; j < j1; ++j) {
      const float* m = mid[y0 + j - c0][tx];
      const float w = wy[j];
      if (j == 0) { acc[0] = m[0] * w; acc[1] = m[1] * w; acc[2] = m[2] * w; }
      else { acc[0] += m[0] * w; acc[1] += m[1] * w; acc[2] += m[2] * w; }
    }
    __syncthreads();
  }
  if (live)
    a.out[(long)oy * FID_SIDE + ox] = make_float4((acc[0] - 0.485f) / 0.229f, (acc[1] - 0.456f) / 0.224f,
                                                  (acc[2] - 0.406f) / 0.225f, 0.f);
}

// ---------------------------------------------------------------------------------------------- BatchNorm + ReLU
__global__ __launch_bounds__(FD_NT) void fid_bn_relu_kernel(const float4* x, long total, int C4,
                                                            const float4* __restrict__ a, const float4* __restrict__ b,
                                                            float* y, int ldo) {
  const long i = (long)blockIdx.x * FD_NT + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4);
  const long r = i / C4;
  const float4 v = x[i], s = a[c], t = b[c];
  float4 o;
  o.x = fmaxf(v.x * s.x + t.x, 0.f);
  o.y = fmaxf(v.y * s.y + t.y, 0.f);
  o.z = fmaxf(v.z * s.z + t.z, 0.f);
  o.w = fmaxf(v.w * s.w + t.w, 0.f);
  *reinterpret_cast<float4*>(y + r * ldo + (long)c * 4) = o;
}

// ---------------------------------------------------------------------------------------------- pools
struct PoolArgs {
  const float4* x;
  float* y;
  int H, W, Ho, Wo, C4, ldo;
  long total;               // N * Ho * Wo * C4
};

__global__ __launch_bounds__(FD_NT) void fid_avgpool3_kernel(PoolArgs a) {
  const long i = (long)blockIdx.x * FD_NT + threadIdx.x;
  if (i >= a.total) return;
  const int c = (int)(i % a.C4);
  long r = i / a.C4;
  const int ox = (int)(r % a.W);
  r /= a.W;
  const int oy = (int)(r % a.H);
  const long n = r / a.H;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int dy = -1; dy <= 1; ++dy) {
    const int yy = oy + dy;
    if (yy < 0 || yy >= a.H) continue;
    for (int dx = -1; dx <= 1; ++dx) {
      const int xx = ox + dx;
      if (xx < 0 || xx >= a.W) continue;
      const float4 v = a.x[((n * a.H + yy) * a.W + xx) * a.C4 + c];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  s.x /= 9.0f; s.y /= 9.0f; s.z /= 9.0f; s.w /= 9.0f;
  reinterpret_cast<float4*>(a.y)[i] = s;
}

__global__ __launch_bounds__(FD_NT) void fid_maxpool3s2_kernel(PoolArgs a) {
  const long i = (long)blockIdx.x * FD_NT + threadIdx.x;
  if (i >= a.total) return;
  const int c = (int)(i % a.C4);
  const long row = i / a.C4;          // (n, oy, ox)
  long r = row;
  const int ox = (int)(r % a.Wo);
  r /= a.Wo;
  const int oy = (int)(r % a.Ho);
  const long n = r / a.Ho;
  // the window lies inside the image: (Ho - 1) * 2 + 3 <= H by the output size formula
  const float4* p = a.x + ((n * a.H + (long)oy * 2) * a.W + (long)ox * 2) * a.C4 + c;
  float4 m = p[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float4 v = p[((long)dy * a.W + dx) * a.C4];
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  *reinterpret_cast<float4*>(a.y + row * a.ldo + (long)c * 4) = m;
}

// ---------------------------------------------------------------------------------------------- global average
__global__ __launch_bounds__(FD_NT) void fid_gap_kernel(const float* __restrict__ x, int B, int hw, int C,
                                                        float* __restrict__ y) {
  const long i = (long)blockIdx.x * FD_NT + threadIdx.x;
  if (i >= (long)B * C) return;
  const int c = (int)(i % C);
  const long b = i / C;
  const float* p = x + b * hw * C + c;
  float s = p[0];
  for (int k = 1; k < hw; ++k) s += p[(long)k * C];
  y[i] = s / (float)hw;
}

std::string kn(const char* k) { return prof_on() ? std::string("irx::(anonymous namespace)::") + k : std::string(); }

unsigned blocks_for(long total) {
  const long blocks = (total + FD_NT - 1) / FD_NT;
  IRX_CHECK(total > 0 && blocks <= 0x7fffffffL, "tensor empty or too large for one launch");
  return (unsigned)blocks;
}

}  // namespace

void fid_input(const uint8_t* img, int H, int W, const int* xs, const int* xn, const float* xw, int kx, const int* ys,
               const int* yn, const float* yw, int ky, float* out, hipStream_t s) {
  IRX_CHECK(H > 0 && W > 0 && kx > 0 && ky > 0 && (long)H * W * 3 <= 0x7fffffffL, "FID input: bad image or table size");
  InputArgs a;
  a.img = img; a.H = H; a.W = W; a.xs = xs; a.xn = xn; a.ys = ys; a.yn = yn; a.xw = xw; a.yw = yw; a.kx = kx; a.ky = ky;
  a.out = (float4*)out;
  const dim3 grid((FID_SIDE + IN_TX - 1) / IN_TX, (FID_SIDE + IN_TY - 1) / IN_TY);
  ProfScope pr(kn("fid_input_kernel"), 0.0, s);
  hipLaunchKernelGGL(fid_input_kernel, grid, dim3(FD_NT), 0, s, a);
  IRX_LAUNCH_CHECK();
}

void fid_bn_relu(const float* x, long rows, int C, const float* a, const float* b, float* y, int ldo, hipStream_t s) {
  IRX_CHECK(rows > 0 && C > 0 && C % 4 == 0 && ldo >= C && ldo % 4 == 0, "BN + ReLU: C, ldo % 4 == 0, ldo >= C");
  const long total = rows * (C / 4);
  ProfScope pr(kn("fid_bn_relu_kernel"), 0.0, s);
  hipLaunchKernelGGL(fid_bn_relu_kernel, dim3(blocks_for(total)), dim3(FD_NT), 0, s, (const float4*)x, total, C / 4,
                     (const float4*)a, (const float4*)b, y, ldo);
  IRX_LAUNCH_CHECK();
}

void fid_avgpool3(const float* x, int N, int H, int W, int C, float* y, hipStream_t s) {
  IRX_CHECK(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "average pool: C % 4 == 0");
  PoolArgs a;
  a.x = (const float4*)x; a.y = y; a.H = H; a.W = W; a.Ho = H; a.Wo = W; a.C4 = C / 4; a.ldo = C;
  a.total = (long)N * H * W * a.C4;
  ProfScope pr(kn("fid_avgpool3_kernel"), 0.0, s);
  hipLaunchKernelGGL(fid_avgpool3_kernel, dim3(blocks_for(a.total)), dim3(FD_NT), 0, s, a);
  IRX_LAUNCH_CHECK();
}

void fid_maxpool3s2(const float* x, int N, int H, int W, int C, float* y, int ldo, hipStream_t s) {
  IRX_CHECK(N > 0 && H >= 3 && W >= 3 && C > 0 && C % 4 == 0 && ldo >= C && ldo % 4 == 0,
            "max pool: H, W >= 3, C, ldo % 4 == 0, ldo >= C");
  PoolArgs a;
  a.x = (const float4*)x; a.y = y; a.H = H; a.W = W; a.Ho = (H - 3) / 2 + 1; a.Wo = (W - 3) / 2 + 1; a.C4 = C / 4;
  a.ldo = ldo;
  a.total = (long)N * a.Ho * a.Wo * a.C4;
  ProfScope pr(kn("fid_maxpool3s2_kernel"), 0.0, s);
  hipLaunchKernelGGL(fid_maxpool3s2_kernel, dim3(blocks_for(a.total)), dim3(FD_NT), 0, s, a);
  IRX_LAUNCH_CHECK();
}

void fid_gap(const float* x, int B, int hw, int C, float* y, hipStream_t s) {
  IRX_CHECK(B > 0 && hw > 0 && C > 0, "global average: empty tensor");
  ProfScope pr(kn("fid_gap_kernel"), 0.0, s);
  hipLaunchKernelGGL(fid_gap_kernel, dim3(blocks_for((long)B * C)), dim3(FD_NT), 0, s, x, B, hw, C, y);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
