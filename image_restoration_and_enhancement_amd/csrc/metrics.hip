// Evaluation metrics on uint8 image pairs (metrics.py / the reference's src/metrics.py): the squared error behind
// PSNR, skimage's SSIM and the mean dE76, one launch per batch plus a finalize launch; and cv2's INTER_LINEAR
// resize for pairs whose shapes differ.
//
// SSIM.  skimage crops the SSIM map by 3 pixels, which removes exactly the 7x7 windows that touch the border, so the
// value is the mean of S over the (H - 6)(W - 6) fully interior windows of every channel and no border mode exists
// here.  For a window with the integer sums sx, sy, sxx, syy, sxy over its n = 49 pixels, k = n(n - 1):
//   A1 = 2 sx sy + C1 n^2             B1 = sx^2 + sy^2 + C1 n^2
//   A2 = 2 (n sxy - sx sy) + C2 k     B2 = (n sxx - sx^2) + (n syy - sy^2) + C2 k          S = A1 A2 / (B1 B2)
// which is skimage's formula (sample covariance) times n^2 k / (n^2 k).  Every term but C1 n^2 and C2 k is an integer
// below 2^53, so fp64 forms it exactly; only the products, the quotient and the sum round.
//
// One 256-thread block per tile of MT_TW x MT_TH windows of one image:
//   1. the (th + 6) x (tw + 6) pixels under the tile go to LDS for both images (tile_load: whole dwords, the
//      unaligned head and tail of a 3-byte-pixel row byte by byte, every load in flight before the first store);
//   2. the block's own pixels (its tile, plus the 6-pixel rim for the last tile of a row / column: every pixel has
//      one owner) give the squared error and, if asked, dE76 (Lab in fp64 from the float32 sRGB table);
//   3. horizontal pass: the 7-tap sums of every (row, column, channel) into LDS as three words,
//      sx | sy << 16, sxx + syy, sxy (B2 only needs the sum of the two squares);
//   4. vertical pass: a thread per (column, channel, row segment) slides down its column, adding the row that enters
//      and subtracting the one that leaves, and adds S of each window to its fp64 sum in row order;
//   5. the block's three sums are reduced by a fixed LDS tree and stored as its partial in the workspace.
// metrics_finalize_kernel (one block per image) adds an image's partials in a fixed order.  No atomics: the integer
// sum does not depend on the order anyway, and the fp64 sums see the same order on every run, for every position in
// the batch and every batch size (the tiling depends on H, W and C alone).
#include <string>

#include "ops.h"
#include "profile.h"

namespace irx {
namespace {

constexpr int MT_TW = 32, MT_TH = 32;     // windows per tile (metrics_gpu.TILE_W / TILE_H)
constexpr int MT_NT = 256;
constexpr int MT_WIN = 7, MT_HALO = MT_WIN - 1;
constexpr int MT_ROWS = MT_TH + MT_HALO;  // pixel rows / columns under a tile
constexpr int MT_COLS = MT_TW + MT_HALO;

template <int C>
struct MtLayout {
  static constexpr int NCOL = MT_TW * C;                       // (column, channel) pairs of a tile
  static constexpr int NSEG = MT_NT / NCOL;                    // row segments of the vertical pass (C = 3: 2, C = 1: 8)
  static constexpr int SEG_ROWS = (MT_TH + NSEG - 1) / NSEG;
  static constexpr int STRIDE = (MT_COLS * C + 3 + 3) & ~3;    // LDS bytes per pixel row (3: the row's address mod 4)
  static constexpr int OFF_GT = MT_ROWS * STRIDE;
  static constexpr int OFF_H = 2 * MT_ROWS * STRIDE;           // three planes of [MT_ROWS][NCOL] words
  static constexpr int OFF_LUT = OFF_H + 3 * MT_ROWS * NCOL * 4;
  static constexpr int BYTES = OFF_LUT + 256 * 4;
  static_assert(NSEG >= 1 && NSEG * NCOL <= MT_NT, "a thread per (column, channel, segment)");
  static_assert(3 * MT_NT * 8 <= 3 * MT_ROWS * NCOL * 4, "the block reduction reuses the horizontal planes");
  static_assert(BYTES <= 64 * 1024, "dynamic LDS default limit");
};

struct MetricsArgs {
  const uint8_t *pred, *gt;
  const float* lut;       // sRGB linearisation of the 256 byte values (null: no dE)
  double* ws;             // [batch][blocks per image][3] 8-byte words: sse (as int64), sum S, sum dE
  int H, W;
  int nwx, nwy;           // windows per row / column = W - 6, H - 6
  int de;
  double c1n2, c2k;       // C1 n^2, C2 n (n - 1)
};

// The pixels under a tile, for both images: `rows` segments of n bytes, row r at global address g + r * gstride, into
// LDS at l + r * lstride + (address mod 4).  Whole dwords move as dwords; a head or tail dword is put together from
// its bytes inside [address, address + n) (nothing outside is read) and stored whole (the other bytes of that LDS
// dword are zero and never read).  Every load of both images is issued before the first store, so their latencies
// overlap; the index runs over the full tile's row length (a compile-time divisor) and skips what this tile lacks.
template <int C>
__device__ __forceinline__ void tile_load(const uint8_t* gp, const uint8_t* gg, size_t gstride, uint8_t* lp, uint8_t* lg,
                                          int lstride, int rows, int n, int tid) {
  constexpr int ND = (MT_COLS * C + 6) >> 2;          // dwords a full-width segment can touch at any phase
  constexpr int IT = (MT_ROWS * ND + MT_NT - 1) / MT_NT;
  uint32_t v[2][IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int idx = tid + k * MT_NT, r = idx / ND, d = (idx - r * ND) * 4;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const uint8_t* gr = (m ? gg : gp) + (size_t)r * gstride;
      const int ph = (int)((uintptr_t)gr & 3);
      const int a = max(d, ph), b = min(d + 4, ph + n);
      const uint8_t* g0 = gr - ph + d;                // dword aligned; only bytes [a - d, b - d) of it are read
      uint32_t w = 0;
      if (r < rows && a < b) {
        if (b - a == 4) {
          w = *reinterpret_cast<const uint32_t*>(g0);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (d + i >= a && d + i < b) w |= (uint32_t)g0[i] << (8 * i);
        }
      }
      v[m][k] = w;
    }
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const int idx = tid + k * MT_NT, r = idx / ND, d = (idx - r * ND) * 4;
    if (r < rows && d < n + 3) {                      // inside the LDS row: d + 3 <= n + 5 < lstride
      *reinterpret_cast<uint32_t*>(lp + r * lstride + d) = v[0][k];
      *reinterpret_cast<uint32_t*>(lg + r * lstride + d) = v[1][k];
    }
  }
}

// skimage rgb2lab (D65, 2 degree) of one pixel from the linearised channels
__device__ __forceinline__ void lab_of(double r, double g, double b, double& L, double& A, double& B) {
  double x = r * 0.412453 + g * 0.357580 + b * 0.180423;
  double y = r * 0.212671 + g * 0.715160 + b * 0.072169;
  double z = r * 0.019334 + g * 0.119193 + b * 0.950227;
  x = x / 0.95047;
  z = z / 1.08883;
  x = x > 0.008856 ? cbrt(x) : 7.787 * x + 16.0 / 116.0;
  y = y > 0.008856 ? cbrt(y) : 7.787 * y + 16.0 / 116.0;
  z = z > 0.008856 ? cbrt(z) : 7.787 * z + 16.0 / 116.0;
  L = 116.0 * y - 16.0;
  A = 500.0 * (x - y);
  B = 200.0 * (y - z);
}

// the block's three sums by one fixed tree over its 256 threads (the same pairs are added on every run);
// red: [3][MT_NT] 8-byte words
__device__ __forceinline__ void block_sum3(double* red, unsigned long long& e, double& s, double& d, int tid) {
  unsigned long long* re = reinterpret_cast<unsigned long long*>(red);
  double *rs = red + MT_NT, *rd = red + 2 * MT_NT;
  re[tid] = e;
  rs[tid] = s;
  rd[tid] = d;
  __syncthreads();
#pragma unroll
  for (int h = MT_NT / 2; h > 0; h >>= 1) {
    if (tid < h) {
      re[tid] += re[tid + h];
      rs[tid] += rs[tid + h];
      rd[tid] += rd[tid + h];
    }
    __syncthreads();
  }
  e = re[0];
  s = rs[0];
  d = rd[0];
}

template <int C>
__global__ __launch_bounds__(MT_NT) void metrics_pair_kernel(MetricsArgs a) {
  using Ly = MtLayout<C>;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * MT_TW, y0 = blockIdx.y * MT_TH;
  const int tw = min(MT_TW, a.nwx - x0), th = min(MT_TH, a.nwy - y0);        // windows of this tile, >= 1
  const int cols = tw + MT_HALO, rows = th + MT_HALO;                         // pixels under it, inside the image
  const size_t rowb = (size_t)a.W * C;
  const size_t base = ((size_t)blockIdx.z * a.H + y0) * rowb + (size_t)x0 * C;
  uint8_t* lp = lds;
  uint8_t* lg = lds + Ly::OFF_GT;
  uint32_t* hxy = reinterpret_cast<uint32_t*>(lds + Ly::OFF_H);
  uint32_t* hsq = hxy + MT_ROWS * Ly::NCOL;
  uint32_t* hpr = hsq + MT_ROWS * Ly::NCOL;
  float* lut = reinterpret_cast<float*>(lds + Ly::OFF_LUT);

  tile_load<C>(a.pred + base, a.gt + base, rowb, lp, lg, Ly::STRIDE, rows, cols * C, tid);
  if (C == 3 && a.de) lut[tid] = a.lut[tid];
  __syncthreads();
  // pred and gt have the same shape: row r of either sits at the same phase only if the two base addresses agree
  // modulo 4, so each image keeps its own
  const int php = (int)((uintptr_t)(a.pred + base) & 3), phg = (int)((uintptr_t)(a.gt + base) & 3);
  const int rstep = (int)(rowb & 3);

  // the pixels this block owns
  const int ox = blockIdx.x == gridDim.x - 1 ? cols : tw, oy = blockIdx.y == gridDim.y - 1 ? rows : th;
  uint32_t sse = 0;
  for (int i = tid; i < oy * ox * C; i += MT_NT) {
    const int r = i / (ox * C), j = i - r * (ox * C);
    const int d = (int)lg[r * Ly::STRIDE + ((phg + r * rstep) & 3) + j] -
                  (int)lp[r * Ly::STRIDE + ((php + r * rstep) & 3) + j];
    sse += (uint32_t)(d * d);
  }
  double de = 0.0;
  if (C == 3 && a.de) {
    for (int i = tid; i < oy * ox; i += MT_NT) {
      const int r = i / ox, x = i - r * ox;
      const uint8_t* p = lp + r * Ly::STRIDE + ((php + r * rstep) & 3) + x * 3;
      const uint8_t* g = lg + r * Ly::STRIDE + ((phg + r * rstep) & 3) + x * 3;
      double l0, a0, b0, l1, a1, b1;
      lab_of((double)lut[p[0]], (double)lut[p[1]], (double)lut[p[2]], l0, a0, b0);
      lab_of((double)lut[g[0]], (double)lut[g[1]], (double)lut[g[2]], l1, a1, b1);
      const double dl = l0 - l1, da = a0 - a1, db = b0 - b1;
      de += sqrt(dl * dl + da * da + db * db);
    }
  }

  // horizontal 7-tap sums; x = gt, y = pred (the formula is symmetric in the two)
  const int ncol = tw * C;
  for (int i = tid; i < rows * ncol; i += MT_NT) {
    const int r = i / ncol, j = i - r * ncol;
    const uint8_t* p = lp + r * Ly::STRIDE + ((php + r * rstep) & 3) + j;
    const uint8_t* g = lg + r * Ly::STRIDE + ((phg + r * rstep) & 3) + j;
    uint32_t sx = 0, sy = 0, sq = 0, pr = 0;
#pragma unroll
    for (int t = 0; t < MT_WIN; ++t) {
      const uint32_t x = g[t * C], y = p[t * C];
      sx += x;
      sy += y;
      sq += x * x + y * y;
      pr += x * y;
    }
    hxy[r * Ly::NCOL + j] = sx | (sy << 16);    // sums of 49 bytes stay below 2^14: the halves never carry
    hsq[r * Ly::NCOL + j] = sq;
    hpr[r * Ly::NCOL + j] = pr;
  }
  __syncthreads();

  // vertical pass
  double ss = 0.0;
  {
    const int seg = tid / Ly::NCOL, j = tid - seg * Ly::NCOL;
    const int r0 = seg * Ly::SEG_ROWS, r1 = min(r0 + Ly::SEG_ROWS, th);
    if (seg < Ly::NSEG && j < ncol && r0 < r1) {
      uint32_t vxy = 0, vsq = 0, vpr = 0;
#pragma unroll
      for (int t = 0; t < MT_HALO; ++t) {
        vxy += hxy[(r0 + t) * Ly::NCOL + j];
        vsq += hsq[(r0 + t) * Ly::NCOL + j];
        vpr += hpr[(r0 + t) * Ly::NCOL + j];
      }
      for (int r = r0; r < r1; ++r) {
        vxy += hxy[(r + MT_HALO) * Ly::NCOL + j];
        vsq += hsq[(r + MT_HALO) * Ly::NCOL + j];
        vpr += hpr[(r + MT_HALO) * Ly::NCOL + j];
        const double sx = (double)(vxy & 0xffffu), sy = (double)(vxy >> 16);
        const double n = (double)(MT_WIN * MT_WIN);
        const double sxsy = sx * sy, sq2 = sx * sx + sy * sy;
        const double A1 = 2.0 * sxsy + a.c1n2;
        const double B1 = sq2 + a.c1n2;
        const double A2 = 2.0 * (n * (double)vpr - sxsy) + a.c2k;
        const double B2 = (n * (double)vsq - sq2) + a.c2k;
        ss += (A1 * A2) / (B1 * B2);
        vxy -= hxy[r * Ly::NCOL + j];
        vsq -= hsq[r * Ly::NCOL + j];
        vpr -= hpr[r * Ly::NCOL + j];
      }
    }
  }
  __syncthreads();                              // the planes are consumed: the reductions reuse them

  unsigned long long bsse = sse;
  double bss = ss, bde = de;
  block_sum3(reinterpret_cast<double*>(lds + Ly::OFF_H), bsse, bss, bde, tid);
  if (tid == 0) {
    const size_t nblk = (size_t)gridDim.x * gridDim.y;
    double* w = a.ws + ((size_t)blockIdx.z * nblk + (size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
    w[0] = __longlong_as_double((long long)bsse);
    w[1] = bss;
    w[2] = bde;
  }
}

// one block per image: thread t adds partials t, t + 256, ... in that order, then the fixed tree
__global__ __launch_bounds__(MT_NT) void metrics_finalize_kernel(const double* ws, int nblk, double nwin, double npix,
                                                                 long long* sse, double* ssim, double* de) {
  __shared__ double red[3 * MT_NT];
  const int tid = threadIdx.x;
  const double* w = ws + (size_t)blockIdx.x * nblk * 3;
  unsigned long long e = 0;
  double s = 0.0, d = 0.0;
  for (int i = tid; i < nblk; i += MT_NT) {
    e += (unsigned long long)__double_as_longlong(w[3 * i]);
    s += w[3 * i + 1];
    d += w[3 * i + 2];
  }
  block_sum3(red, e, s, d, tid);
  if (tid == 0) {
    sse[blockIdx.x] = (long long)e;
    ssim[blockIdx.x] = s / nwin;
    if (de) de[blockIdx.x] = d / npix;
  }
}

struct ResizeArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int *xt, *yt;     // [out][3] = (i0, i1, w1), w0 = 2048 - w1
  int H, W, h, w;
  long long total;        // output bytes
};

// four consecutive output bytes per thread (one dword store where dst allows it)
template <int C>
__global__ __launch_bounds__(MT_NT) void resize_linear_kernel(ResizeArgs a) {
  const long long first = ((long long)blockIdx.x * MT_NT + threadIdx.x) * 4;
  if (first >= a.total) return;
  const int orow = a.w * C;
  uint32_t v[4];
  const int n = (int)min(4LL, a.total - first);
  for (int i = 0; i < n; ++i) {
    const long long idx = first + i;
    const long long row = idx / orow;
    const int j = (int)(idx - row * orow);
    const int x = j / C, c = j - x * C;
    const int b = (int)(row / a.h), y = (int)(row - (long long)b * a.h);
    // the clamps keep every read inside the image whatever the tables say
    const int xi0 = min(max(a.xt[3 * x], 0), a.W - 1), xi1 = min(max(a.xt[3 * x + 1], 0), a.W - 1);
    const int yi0 = min(max(a.yt[3 * y], 0), a.H - 1), yi1 = min(max(a.yt[3 * y + 1], 0), a.H - 1);
    const int wx1 = min(max(a.xt[3 * x + 2], 0), 2048), wy1 = min(max(a.yt[3 * y + 2], 0), 2048);
    const int wx0 = 2048 - wx1, wy0 = 2048 - wy1;
    const uint8_t* s = a.src + (size_t)b * a.H * a.W * C + c;
    const uint8_t* s0 = s + (size_t)yi0 * a.W * C;
    const uint8_t* s1 = s + (size_t)yi1 * a.W * C;
    const int t0 = (int)s0[(size_t)xi0 * C] * wx0 + (int)s0[(size_t)xi1 * C] * wx1;
    const int t1 = (int)s1[(size_t)xi0 * C] * wx0 + (int)s1[(size_t)xi1 * C] * wx1;
    const int o = (t0 * wy0 + t1 * wy1 + (1 << 21)) >> 22;   // <= 255 * 2^22 + 2^21 < 2^31
    v[i] = (uint32_t)min(max(o, 0), 255);
  }
  uint8_t* d = a.dst + first;
  if (n == 4 && ((uintptr_t)d & 3) == 0) {
    *reinterpret_cast<uint32_t*>(d) = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
  } else {
    for (int i = 0; i < n; ++i) d[i] = (uint8_t)v[i];
  }
}

}  // namespace

// tiles of one image; 0 when the shape is outside what one launch covers
static long metrics_blocks(int B, int H, int W, int C) {
  if (B <= 0 || B > 65535 || H < MT_WIN || W < MT_WIN || (C != 1 && C != 3)) return 0;
  const long nbx = (W - MT_HALO + MT_TW - 1) / MT_TW, nby = (H - MT_HALO + MT_TH - 1) / MT_TH;
  if (nby > 65535 || nbx * nby > (1L << 30)) return 0;
  return nbx * nby;
}

long metrics_ws_bytes(int B, int H, int W, int C) { return metrics_blocks(B, H, W, C) * B * 3 * (long)sizeof(double); }

void metrics_pair_u8(const uint8_t* pred, const uint8_t* gt, int B, int H, int W, int C, const float* lut, void* ws,
                     long long* sse, double* ssim, double* de, hipStream_t s) {
  const long nblk = metrics_blocks(B, H, W, C);
  IRX_CHECK(nblk > 0, "image or batch too large for one launch");
  MetricsArgs a;
  a.pred = pred; a.gt = gt; a.lut = lut; a.ws = static_cast<double*>(ws);
  a.H = H; a.W = W; a.nwx = W - MT_HALO; a.nwy = H - MT_HALO;
  a.de = de != nullptr;
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double n = MT_WIN * MT_WIN;
  a.c1n2 = C1 * (n * n);
  a.c2k = C2 * (n * (n - 1.0));
  const dim3 grid((a.nwx + MT_TW - 1) / MT_TW, (a.nwy + MT_TH - 1) / MT_TH, B);
  {
    ProfScope pr(prof_on() ? std::string("irx::(anonymous namespace)::metrics_pair_kernel") : std::string(), 0.0, s);
    if (C == 1) hipLaunchKernelGGL(metrics_pair_kernel<1>, grid, dim3(MT_NT), MtLayout<1>::BYTES, s, a);
    else hipLaunchKernelGGL(metrics_pair_kernel<3>, grid, dim3(MT_NT), MtLayout<3>::BYTES, s, a);
    IRX_LAUNCH_CHECK();
  }
  ProfScope pr(prof_on() ? std::string("irx::(anonymous namespace)::metrics_finalize_kernel") : std::string(), 0.0, s);
  hipLaunchKernelGGL(metrics_finalize_kernel, dim3(B), dim3(MT_NT), 0, s, a.ws, (int)nblk,
                     (double)a.nwx * a.nwy * C, (double)H * W, sse, ssim, de);
  IRX_LAUNCH_CHECK();
}

void resize_linear_u8(const uint8_t* src, int B, int H, int W, int C, const int* xt, const int* yt, int h, int w,
                      uint8_t* dst, hipStream_t s) {
  ResizeArgs a;
  a.src = src; a.dst = dst; a.xt = xt; a.yt = yt;
  a.H = H; a.W = W; a.h = h; a.w = w;
  a.total = (long long)B * h * w * C;
  const long long blocks = (a.total + 4LL * MT_NT - 1) / (4LL * MT_NT);
  IRX_CHECK(blocks <= 0x7fffffffLL, "output too large for one launch");
  ProfScope pr(prof_on() ? std::string("irx::(anonymous namespace)::resize_linear_kernel") : std::string(), 0.0, s);
  if (C == 1) hipLaunchKernelGGL(resize_linear_kernel<1>, dim3((unsigned)blocks), dim3(MT_NT), 0, s, a);
  else hipLaunchKernelGGL(resize_linear_kernel<3>, dim3((unsigned)blocks), dim3(MT_NT), 0, s, a);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
