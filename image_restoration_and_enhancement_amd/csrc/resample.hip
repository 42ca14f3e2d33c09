// PIL Image.resize(LANCZOS | BICUBIC) on 8-bit images, byte for byte: Pillow's ImagingResample as one fused kernel.
// With the tables of irx_resample_coeffs (resample_coeffs.cpp) both passes are integer arithmetic:
//   out = clip8((2^21 + sum_t pixel[first + t] * k[t]) >> 22),
// horizontal pass first, its result rounded to uint8 (Pillow's temporary image), then the vertical pass.
//
// One 256-thread block per output tile of RS_TW x th pixels:
//   1. the tile's source window (rows [ymin(first row), ymax(last row)), columns [xmin(first col), xmax(last col)))
//      goes to an LDS staging area, a chunk of rows at a time (rows_xfer: 16-byte slots, the unaligned head and
//      tail of every row dword by dword and byte by byte);
//   2. horizontal pass, one wave per window row and one lane per tile column (its weights differ per lane: they sit
//      in LDS transposed, [tap][column]), into the uint8 intermediate [window rows][tile columns] in LDS;
//   3. vertical pass, one wave per tile row (its weights are uniform along the row: scalar loads) and four
//      neighbouring bytes per lane from one LDS dword per tap, into an LDS image of the output tile;
//   4. the tile is stored with rows_xfer.
// When only one axis changes, the other stage is a copy through LDS (x unchanged) or skipped (y unchanged: step 4
// stores the intermediate).  Every LDS image of a global row keeps that row's address modulo 16, so that 16-byte
// slots are aligned on both sides.
#include <algorithm>
#include <cmath>
#include <string>

#include "ops.h"
#include "profile.h"

namespace irx {
namespace {

constexpr int RS_TW = 64;            // tile width in pixels = lanes of a wave
constexpr int RS_NT = 256;
constexpr int RS_WAVES = RS_NT / 64;
constexpr int RS_LDS = 64 * 1024;    // per block, the default dynamic-LDS limit (160 KiB per CU: >= 2 blocks per CU)
constexpr int RS_STAGE = 32 * 1024;  // staging area at most (the window streams through it in row chunks)
constexpr int RS_PREC = 22;          // Pillow's PRECISION_BITS for 8-bit channels
constexpr int RS_MAX_K = 97;         // IRX_RESAMPLE_MAX_KSIZE

struct ResampleArgs {
  const uint8_t* src;
  uint8_t* dst;
  const int *xb, *xc, *yb, *yc;      // bounds [out][2], weights [out][k]; null weights = that pass is skipped
  int H, W, h, w, xk, yk;
  int th;                            // tile height
  int cap_cols, cap_rows;            // what a tile's source window can span (host bound from the scale)
  int ss, chunk_rows;                // staging: row stride (bytes), rows
  int is;                            // intermediate / output-tile row stride (bytes)
  int off_inter, off_stage;          // LDS byte offsets (the x tables start at 0)
};

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> RS_PREC, 0), 255); }

// `rows` row segments of n bytes, row r at global address g + r * gstride and in LDS at l + r * lstride + (address
// mod 16).  16-byte slots: a slot inside the segment moves as one uint4; the head and tail slots move their whole
// dwords as dwords and the rest byte by byte.  Nothing outside [address, address + n) is touched on either side.
template <bool STORE>
__device__ __forceinline__ void rows_xfer(uint8_t* g, size_t gstride, uint8_t* l, int lstride, int rows, int n,
                                          int tid) {
  const int ns = (n + 30) >> 4;      // slots a segment can touch at any phase
  for (int idx = tid; idx < rows * ns; idx += RS_NT) {
    const int r = idx / ns, s = idx - r * ns;
    uint8_t* gr = g + (size_t)r * gstride;
    const int ph = (int)((uintptr_t)gr & 15);
    const int lo = s * 16;
    const int a = max(lo, ph), b = min(lo + 16, ph + n);
    if (a >= b) continue;
    uint8_t* lr = l + r * lstride;
    uint8_t* g0 = gr - ph;           // g0 + i <-> lr + i; 16-byte aligned (only [a, b) is dereferenced)
    if (b - a == 16) {
      if (STORE) *reinterpret_cast<uint4*>(g0 + lo) = *reinterpret_cast<const uint4*>(lr + lo);
      else *reinterpret_cast<uint4*>(lr + lo) = *reinterpret_cast<const uint4*>(g0 + lo);
      continue;
    }
    for (int d = lo; d < lo + 16; d += 4) {
      const int da = max(d, a), db = min(d + 4, b);
      if (db - da == 4) {
        if (STORE) *reinterpret_cast<uint32_t*>(g0 + d) = *reinterpret_cast<const uint32_t*>(lr + d);
        else *reinterpret_cast<uint32_t*>(lr + d) = *reinterpret_cast<const uint32_t*>(g0 + d);
      } else {
        for (int i = da; i < db; ++i) {
          if (STORE) g0[i] = lr[i];
          else lr[i] = g0[i];
        }
      }
    }
  }
}

template <int C>
__global__ __launch_bounds__(RS_NT) void resample_kernel(ResampleArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool has_x = a.xc != nullptr, has_y = a.yc != nullptr;
  const int x0 = blockIdx.x * RS_TW, y0 = blockIdx.y * a.th;
  const int tw = min(RS_TW, a.w - x0), th = min(a.th, a.h - y0);
  const size_t rowb = (size_t)a.W * C, orowb = (size_t)a.w * C;
  const uint8_t* src = a.src + (size_t)blockIdx.z * a.H * rowb;
  uint8_t* dst = a.dst + ((size_t)blockIdx.z * a.h + y0) * orowb + (size_t)x0 * C;

  // the tile's source window; the clamps keep every access inside the images and the LDS areas whatever the tables say
  int wx0 = x0, wcols = tw, wy0 = y0, wrows = th;
  if (has_x) {
    const int xl = x0 + tw - 1;
    wx0 = a.xb[2 * x0];
    wcols = a.xb[2 * xl] + a.xb[2 * xl + 1] - wx0;
  }
  if (has_y) {
    const int yl = y0 + th - 1;
    wy0 = a.yb[2 * y0];
    wrows = a.yb[2 * yl] + a.yb[2 * yl + 1] - wy0;
  }
  wx0 = min(max(wx0, 0), a.W - 1);
  wcols = min(max(wcols, 1), min(a.cap_cols, a.W - wx0));
  wy0 = min(max(wy0, 0), a.H - 1);
  wrows = min(max(wrows, 1), min(a.cap_rows, a.H - wy0));

  int* xcl = reinterpret_cast<int*>(lds);          // [xk][RS_TW] weights, then per column: first tap's window
  int* xoff = xcl + a.xk * RS_TW;                  // column, tap count
  int* xn = xoff + RS_TW;
  uint8_t* inter = lds + a.off_inter;
  uint8_t* stage = lds + a.off_stage;              // the vertical pass reuses it for the output tile
  if (has_x) {
    for (int i = tid; i < a.xk * RS_TW; i += RS_NT) {
      const int t = i >> 6, x = i & 63;
      xcl[i] = x < tw ? a.xc[(size_t)(x0 + x) * a.xk + t] : 0;
    }
    if (tid < RS_TW) {
      int off = 0, n = 0;
      if (tid < tw) {
        n = min(min(max(a.xb[2 * (x0 + tid) + 1], 0), a.xk), wcols);
        off = min(max(a.xb[2 * (x0 + tid)] - wx0, 0), wcols - n);
      }
      xoff[tid] = off;
      xn[tid] = n;
    }
  }

  const uint8_t* swin = src + (size_t)wy0 * rowb + (size_t)wx0 * C;
  for (int cr = 0; cr < wrows; cr += a.chunk_rows) {
    const int nr = min(a.chunk_rows, wrows - cr);
    if (cr) __syncthreads();                       // the previous chunk is consumed
    rows_xfer<false>(const_cast<uint8_t*>(swin + (size_t)cr * rowb), rowb, stage, a.ss, nr, wcols * C, tid);
    __syncthreads();                               // (first chunk: the x tables are written too, their loads
                                                   // overlapped the window's)
    for (int r = wave; r < nr; r += RS_WAVES) {
      const int ir = cr + r;
      const uint8_t* srow = stage + r * a.ss + (int)((uintptr_t)(swin + (size_t)ir * rowb) & 15);
      // without a vertical pass the intermediate is the output tile: its rows take the output rows' phase
      uint8_t* irow = inter + ir * a.is + (has_y ? 0 : (int)((uintptr_t)(dst + (size_t)ir * orowb) & 15));
      if (has_x) {
        if (lane < tw) {
          const int n = xn[lane];
          const uint8_t* p = srow + xoff[lane] * C;
          int acc[C];
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PREC - 1);
#pragma unroll 4
          for (int t = 0; t < n; ++t) {
            // |k| < 2^23 (sum |k| * 255 + 2^21 < 2^31): the 24-bit multiply is exact, the sum Pillow's int accumulator
            const int k = xcl[t * RS_TW + lane];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += __mul24((int)p[t * C + c], k);
          }
#pragma unroll
          for (int c = 0; c < C; ++c) irow[lane * C + c] = (uint8_t)clip8(acc[c]);
        }
      } else {
        for (int i = lane; i < tw * C; i += 64) irow[i] = srow[i];
      }
    }
  }
  __syncthreads();

  if (!has_y) {
    rows_xfer<true>(dst, orowb, inter, a.is, th, tw * C, tid);
    return;
  }
  uint8_t* otile = stage;
  const int nd = (tw * C + 3) >> 2, isd = a.is >> 2;
  for (int r = wave; r < th; r += RS_WAVES) {
    const int y = y0 + r;
    const int n = min(min(max(a.yb[2 * y + 1], 0), a.yk), wrows);
    const int first = min(max(a.yb[2 * y] - wy0, 0), wrows - n);
    const int* kc = a.yc + (size_t)y * a.yk;
    uint8_t* orow = otile + r * a.is + (int)((uintptr_t)(dst + (size_t)r * orowb) & 15);
    for (int j = lane; j < nd; j += 64) {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(inter + first * a.is) + j;
      int a0 = 1 << (RS_PREC - 1), a1 = a0, a2 = a0, a3 = a0;
#pragma unroll 4
      for (int t = 0; t < n; ++t) {
        const int k = kc[t];
        const uint32_t v = p[t * isd];
        a0 += __mul24((int)(v & 255u), k);
        a1 += __mul24((int)((v >> 8) & 255u), k);
        a2 += __mul24((int)((v >> 16) & 255u), k);
        a3 += __mul24((int)(v >> 24), k);
      }
      const int o[4] = {clip8(a0), clip8(a1), clip8(a2), clip8(a3)};
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (4 * j + i < tw * C) orow[4 * j + i] = (uint8_t)o[i];
    }
  }
  __syncthreads();
  rows_xfer<true>(dst, orowb, otile, a.is, th, tw * C, tid);
}

int round16(int v) { return (v + 15) & ~15; }

}  // namespace

// Tile height from the vertical scale: the window of a th-row tile spans about th * scale + 2 * support rows, and
// the intermediate holds all of them (at most 114 rows of 208 bytes at 1/16).  Independent of the batch.
int resample_tile_h(int H, int h, bool has_y) {
  if (!has_y || H <= h) return 32;
  const double s = (double)H / h;
  return s <= 2 ? 16 : s <= 4 ? 8 : s <= 8 ? 4 : 2;
}

void resample_u8(const uint8_t* src, int B, int H, int W, int C, const int* xb, const int* xc, int xk, const int* yb,
                 const int* yc, int yk, int h, int w, uint8_t* dst, hipStream_t s) {
  const bool has_x = xc != nullptr, has_y = yc != nullptr;
  if (!has_x && !has_y) {
    IRX_HIP(hipMemcpyAsync(dst, src, (size_t)B * H * W * C, hipMemcpyDeviceToDevice, s));
    return;
  }
  IRX_CHECK((!has_x || (xk >= 1 && xk <= RS_MAX_K)) && (!has_y || (yk >= 1 && yk <= RS_MAX_K)),
            "resize ratio outside the kernel's range: ksize " + std::to_string(std::max(has_x ? xk : 0, has_y ? yk : 0)) +
                " > " + std::to_string(RS_MAX_K) + " (LANCZOS down to 1/16)");
  ResampleArgs a;
  a.src = src; a.dst = dst;
  a.xb = has_x ? xb : nullptr; a.xc = xc; a.yb = has_y ? yb : nullptr; a.yc = yc;
  a.H = H; a.W = W; a.h = h; a.w = w;
  a.xk = has_x ? xk : 0; a.yk = has_y ? yk : 0;
  a.th = resample_tile_h(H, h, has_y);
  // window bounds: first = (int)(c0 - support + .5) >= c0 - support - .5, last <= c1 + support + .5 and
  // c1 - c0 = (tile - 1) * scale, 2 * support <= ksize - 1
  a.cap_cols = has_x ? std::min(W, (int)std::ceil((RS_TW - 1) * ((double)W / w)) + (xk - 1) + 2) : RS_TW;
  a.cap_rows = has_y ? std::min(H, (int)std::ceil((a.th - 1) * ((double)H / h)) + (yk - 1) + 2) : a.th;
  a.is = round16(RS_TW * C + 15);
  a.ss = round16(a.cap_cols * C + 15);
  const int tab = has_x ? (a.xk + 2) * RS_TW * (int)sizeof(int) : 0;
  a.off_inter = tab;
  a.off_stage = tab + a.cap_rows * a.is;
  const int otile = a.th * a.is;
  const int room = std::min(RS_LDS - a.off_stage, RS_STAGE);
  IRX_CHECK(room >= a.ss && room >= otile, "resample: the tile does not fit the LDS budget");
  a.chunk_rows = std::min(a.cap_rows, room / a.ss);
  const size_t lds = (size_t)a.off_stage + std::max(a.chunk_rows * a.ss, otile);
  const dim3 grid((w + RS_TW - 1) / RS_TW, (h + a.th - 1) / a.th, B);
  IRX_CHECK(grid.y <= 65535u && grid.z <= 65535u, "resample: image or batch too large for one launch");
  ProfScope pr(prof_on() ? std::string("irx::(anonymous namespace)::resample_kernel") : std::string(), 0.0, s);
  if (C == 1) hipLaunchKernelGGL(resample_kernel<1>, grid, dim3(RS_NT), lds, s, a);
  else hipLaunchKernelGGL(resample_kernel<3>, grid, dim3(RS_NT), lds, s, a);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
