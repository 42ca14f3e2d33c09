// irx — baseline JPEG encoder on the GPU: the scan PIL.Image.save(f, "JPEG", quality=q) writes for uint8
// [B][H][W][3] batches resident in HBM (scripts/generate_predictions.py:83-84 saves every output that way), byte
// for byte.  libjpeg's integer chain up to the quantiser is jpeg_fdct.h (shared with the JPEG round trip,
// degrade_jpeg.hip); this file adds the entropy coder.  jpeg_host.py is the same coder in numpy and the oracle.
//
// Seven launches, none of which walks an image's blocks on one lane:
//   1 jpeg_coef_kernel     the tile of the round trip (4 MCUs, 192 lanes); stops after the quantiser and writes the
//                          quotients as int16 in zigzag order, [b][mcu][6][64].  libjpeg pads to whole 8x8 blocks only:
//                          a Y block beyond ceil(W/8) x ceil(H/8) is a dummy (AC zero, DC that of the previous block of
//                          its MCU, jccoefct.c), materialised here so that the coder needs no geometry.
//   2 jpeg_huff_kernel<0>  sizing.  A workgroup of 4 waves owns 8 consecutive MCUs = 48 blocks; a wave codes one 8x8
//                          block at a time, one lane per zigzag coefficient.  __ballot gives the non-zero mask, a
//                          lane's zero run is a count-leading-zeros below it; every non-zero lane forms its own string
//                          (<= 3 ZRL + a <= 16-bit code + <= 10 value bits = 59 bits), lane 0 the DC difference (its
//                          predecessor's DC is read from the coefficients), the lane after the last non-zero one
//                          the EOB.  A wave prefix sum of the lengths places the strings in the block, a prefix sum
//                          over the 48 block totals places the blocks.  Writes the bits of the workgroup.
//   3 jpeg_scan_kernel     per image: exclusive scan of the workgroup bits -> bit offsets; clears the dword at every
//                          offset and at the end of the stream (the only dwords step 4 ORs into; callers hand over
//                          garbage workspaces).
//   4 jpeg_huff_kernel<1>  the same code, now OR-ing the strings into an LDS bit buffer whose dwords are aligned with
//                          the stream's, then storing whole dwords of the unstuffed stream: atomicOr on the first dword
//                          and on a partial last one (shared with the neighbouring workgroups), plain stores between.
//   5 jpeg_ff_count_kernel 0xFF bytes per 2048-byte segment of the unstuffed stream (the final 1-padding applied).
//   6 jpeg_scan_kernel     per image: exclusive scan of the counts; lens[b] = bytes + 0xFFs.
//   7 jpeg_stuff_kernel    copies every byte to its final offset, a 0x00 after every 0xFF.
//
// Bounds (derived, not measured).  A block is at most 22 bits of DC (the longest DC code, chroma category 11, has
// 11 bits, + 11 value bits) + 63 x (16 + 10) bits of AC = 1660 bits <= 208 bytes.  Unstuffed scan <= 6 * MCUs * 208
// bytes; stuffed <= twice that, + 2 (jpeg_encode_bound).  LDS of the coder: 48 * 1660 bits + 31 bits of alignment
// -> 2492 dwords of bit buffer (9968 B), 536 dwords of code tables (2144 B), 2 x 49 ints of block totals: 12.5 KB.
#include "block_scan.h"
#include "jpeg_fdct.h"
#include "jpeg_tables.h"

namespace irx {
namespace {

using namespace jpegdev;
using namespace jpegtab;

struct InvZigzag {
  uint8_t v[64];
};
constexpr InvZigzag make_inv() {
  InvZigzag t{};
  for (int k = 0; k < 64; ++k) t.v[kZigzag[k]] = (uint8_t)k;
  return t;
}
__constant__ InvZigzag kNatToZz = make_inv();      // zigzag position of a natural (row-major) index
__constant__ CodeTable kCodes = make_codes();

constexpr int kBlockMaxBits = 22 + 63 * 26, kBlockMaxBytes = 208;
static_assert(kBlockMaxBits == 1660 && kBlockMaxBits <= 8 * kBlockMaxBytes, "per-block bound");
constexpr int kHT = 256, kHMcus = 8, kHBlocks = 6 * kHMcus, kHPerWave = kHBlocks / 4;
constexpr int kBitDwords = (31 + kHBlocks * kBlockMaxBits) / 32 + 1;
constexpr int kScanT = 256;
constexpr int kSegT = 256, kSegBytes = kSegT * 8;

// ------------------------------------------------------------------ 1: coefficients
__global__ __launch_bounds__(kJT) void jpeg_coef_kernel(const uint8_t* __restrict__ img, int H, int W,
                                                        const int* __restrict__ qt, int rgb,
                                                        uint32_t* __restrict__ coef) {
  __shared__ uint8_t raw[kJRawBytes];
  __shared__ int blk[kJBlkInts];
  __shared__ int16_t zz[24 * 64];
  const int tid = threadIdx.x, b = blockIdx.z, x0 = blockIdx.x * kJTileW, y0 = blockIdx.y * kJTileH;
  jpeg_tile_rows(img + (long)b * H * W * 3, H, W, rgb, x0, y0, raw, blk);
  {  // forward columns, quantise; the quotient goes to its zigzag position
    const int bi = tid >> 3, l = tid & 7, bk = bi % 6;
    int d[8];
    const int* p = blk + bi * kJBlkStride + l;
    const int* q = qt + ((long)b * 2 + (bk >= 4)) * 64 + l;
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = p[e * kJRow];
    fdct8<false>(d);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      zz[bi * 64 + kNatToZz.v[e * 8 + l]] = (int16_t)quantise(d[e], min(max(q[e * 8], 1), 255));
  }
  __syncthreads();
  // the tile's 4 MCUs are consecutive in raster order: 24 x 32 dwords, contiguous in coef
  const int mcuw = (W + 15) >> 4, mcuh = (H + 15) >> 4, bw = (W + 7) >> 3, bh = (H + 7) >> 3;
  const int my = blockIdx.y, nm = min(4, mcuw - 4 * (int)blockIdx.x);
  uint32_t* dst = coef + (((long)b * mcuh + my) * mcuw + 4 * blockIdx.x) * (6 * 32);
  for (int j = tid; j < nm * 6 * 32; j += kJT) {
    const int bi = j >> 5, pair = j & 31, m = bi / 6, bk = bi - m * 6, mx = 4 * blockIdx.x + m;
    int src = bk;                                            // a dummy takes the DC of the block before it
    if (bk < 4)
      while (src > 0 && (2 * mx + (src & 1) >= bw || 2 * my + (src >> 1) >= bh)) --src;
    const bool dummy = src != bk;
    int lo = dummy ? 0 : zz[bi * 64 + 2 * pair], hi = dummy ? 0 : zz[bi * 64 + 2 * pair + 1];
    if (pair == 0) lo = zz[(m * 6 + src) * 64];
    dst[j] = (uint32_t)(lo & 0xFFFF) | ((uint32_t)hi << 16);
  }
}

// ------------------------------------------------------------------ 2, 4: the Huffman coder (scans: block_scan.h)
template <bool EMIT>
__global__ __launch_bounds__(kHT) void jpeg_huff_kernel(const int16_t* __restrict__ coef, int nmcu, int ngroups,
                                                        long* __restrict__ wgbits, uint32_t* __restrict__ stream,
                                                        long stream_dwords) {
  __shared__ uint32_t tab[kCodeWords];
  __shared__ int blkbits[kHBlocks], blkoff[kHBlocks + 1];
  __shared__ uint32_t bitbuf[EMIT ? kBitDwords : 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = blockIdx.x, b = blockIdx.y;
  for (int i = tid; i < kCodeWords; i += kHT) tab[i] = kCodes.w[i];
  if (tid < kHBlocks) blkbits[tid] = 0;
  const int nblk = 6 * min(kHMcus, nmcu - g * kHMcus);
  const int16_t* c = coef + ((long)b * nmcu + (long)g * kHMcus) * (6 * 64);
  __syncthreads();
  unsigned long long str[kHPerWave];
  int place[kHPerWave];                                      // bit offset in the block | length << 12
#pragma unroll
  for (int i = 0; i < kHPerWave; ++i) {
    const int j = wave * kHPerWave + i;
    str[i] = 0;
    place[i] = 0;
    if (j >= nblk) continue;                                 // wave-uniform
    const int bk = j % 6, tbl = bk >= 4;
    const int v = c[j * 64 + lane];
    const unsigned long long mask = __ballot(lane > 0 && v != 0);
    unsigned long long s = 0;
    int len = 0;
    if (lane == 0) {
      // the previous block of the same component in scan order: Y01..Y11 follow a Y of their MCU, Y00 the Y11 and
      // a chroma block its like of the MCU before (which may belong to the workgroup before); the first has 0
      const int pj = bk == 0 ? j - 3 : (bk < 4 ? j - 1 : j - 6);
      const int pred = (pj >= 0 || g > 0) ? c[(long)pj * 64] : 0;
      const int d = v - pred, a = abs(d), nb = min(a ? 32 - __clz(a) : 0, 11);
      const uint32_t w = tab[512 + tbl * 12 + nb];
      s = ((unsigned long long)(w & 0xFFFF) << nb) | (uint32_t)((d < 0 ? d - 1 : d) & ((1 << nb) - 1));
      len = (int)(w >> 16) + nb;
    } else if (v != 0) {
      const unsigned long long below = mask & ((1ull << lane) - 1);
      const int prev = below ? 63 - __clzll(below) : 0, run = lane - prev - 1;
      const int a = abs(v), nb = 32 - __clz(a);
      const uint32_t w = tab[tbl * 256 + (((run & 15) << 4) | nb)], z = tab[tbl * 256 + 0xF0];
      const int nz = run >> 4, zl = (int)(z >> 16);
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k < nz) {
          s = (s << zl) | (z & 0xFFFF);
          len += zl;
        }
      s = (((s << (w >> 16)) | (w & 0xFFFF)) << nb) | (uint32_t)((v < 0 ? v - 1 : v) & ((1 << nb) - 1));
      len += (int)(w >> 16) + nb;
    } else {
      const int last = mask ? 63 - __clzll(mask) : 0;
      if (lane == last + 1) {                                // EOB (none when coefficient 63 is non-zero)
        const uint32_t w = tab[tbl * 256];
        s = w & 0xFFFF;
        len = (int)(w >> 16);
      }
    }
    const int incl = wave_incl_scan(len, lane);
    str[i] = s;
    place[i] = (incl - len) | (len << 12);
    if (lane == 63) blkbits[j] = incl;
  }
  __syncthreads();
  if (wave == 0) {
    const int v = lane < kHBlocks ? blkbits[lane] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (lane < kHBlocks) blkoff[lane] = incl - v;
    if (lane == 63) blkoff[kHBlocks] = incl;
  }
  __syncthreads();
  const int total = blkoff[kHBlocks];
  if (!EMIT) {
    if (tid == 0) wgbits[(long)b * ngroups + g] = total;
    return;
  }
  const long off = wgbits[(long)b * ngroups + g];            // after the scan: the bit offset in the image's stream
  const int shift = (int)(off & 31), ndw = (shift + total + 31) >> 5;
  for (int i = tid; i < ndw; i += kHT) bitbuf[i] = 0;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kHPerWave; ++i) {
    const int len = place[i] >> 12;
    if (len == 0) continue;
    const int p = shift + blkoff[wave * kHPerWave + i] + (place[i] & 4095);
    const int w = p >> 5, o = p & 31;
    const unsigned long long t = str[i] << (64 - len);       // left-aligned; 1 <= len <= 59
    atomicOr(&bitbuf[w], (uint32_t)(t >> (32 + o)));
    const unsigned long long rem = t << (32 - o);
    if (o + len > 32) atomicOr(&bitbuf[w + 1], (uint32_t)(rem >> 32));
    if (o + len > 64) atomicOr(&bitbuf[w + 2], (uint32_t)rem);
  }
  __syncthreads();
  uint32_t* dst = stream + (long)b * stream_dwords + (off >> 5);
  const bool ragged = ((shift + total) & 31) != 0;
  for (int i = tid; i < ndw; i += kHT) {
    const uint32_t val = __builtin_bswap32(bitbuf[i]);       // the stream is MSB first: byte 0 holds bits 31..24
    if (i == 0 || (ragged && i == ndw - 1))
      atomicOr(dst + i, val);
    else
      dst[i] = val;
  }
}

// ------------------------------------------------------------------ 3, 6: per-image exclusive scans
// a[b][0..n) -> exclusive prefix in place, total[b] = sum.  CLEAR: also zero the stream dword at every prefix (in
// bits) and at the total, the dwords jpeg_huff_kernel<true> ORs into.
__global__ __launch_bounds__(kScanT) void jpeg_scan_bits_kernel(long* __restrict__ a, int n, long* __restrict__ total,
                                                                uint32_t* __restrict__ stream, long stream_dwords) {
  __shared__ long part[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  long carry = 0;
  uint32_t* st = stream + (long)b * stream_dwords;
  for (int base = 0; base < n; base += kScanT) {
    const int i = base + tid;
    const long v = i < n ? a[(long)b * n + i] : 0;
    long sum;
    const long ex = carry + block_excl_scan(v, part, &sum);
    if (i < n) {
      a[(long)b * n + i] = ex;
      st[ex >> 5] = 0;
    }
    carry += sum;
  }
  if (tid == 0) {
    total[b] = carry;
    st[carry >> 5] = 0;
  }
}

// cnt[b][0..nseg_b) -> exclusive prefix in place (nseg_b from the image's own length); lens[b] = bytes + 0xFFs
__global__ __launch_bounds__(kScanT) void jpeg_scan_ff_kernel(int* __restrict__ cnt, int nsegmax,
                                                              const long* __restrict__ total, int* __restrict__ lens) {
  __shared__ int part[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nbytes = (int)((total[b] + 7) >> 3), n = (nbytes + kSegBytes - 1) / kSegBytes;
  int carry = 0;
  for (int base = 0; base < n; base += kScanT) {
    const int i = base + tid;
    const int v = i < n ? cnt[(long)b * nsegmax + i] : 0;
    int sum;
    const int ex = carry + block_excl_scan(v, part, &sum);
    if (i < n) cnt[(long)b * nsegmax + i] = ex;
    carry += sum;
  }
  if (tid == 0) lens[b] = nbytes + carry;
}

// ------------------------------------------------------------------ 5, 7: byte stuffing
// the lane's 8 bytes of the unstuffed stream (byte k in bits 8k..8k+7): bytes at or past nbytes read as 0, the last
// byte is completed with 1-bits.  i0 < nbytes; the stream is 8-byte aligned and its capacity a multiple of 8.
__device__ __forceinline__ unsigned long long stream8(const uint8_t* st, int i0, int nbytes, long bits) {
  const uint2 v = *reinterpret_cast<const uint2*>(st + i0);
  unsigned long long x = v.x | ((unsigned long long)v.y << 32);
  const int n = nbytes - i0;                                 // >= 1
  if (n <= 8) {
    if (n < 8) x &= (1ull << (8 * n)) - 1;
    const int used = (int)(bits & 7);
    if (used) x |= (unsigned long long)(0xFF >> used) << (8 * (n - 1));
  }
  return x;
}

__device__ __forceinline__ int count_ff(unsigned long long x) {
  int c = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) c += ((x >> (8 * k)) & 0xFF) == 0xFF;
  return c;
}

__global__ __launch_bounds__(kSegT) void jpeg_ff_count_kernel(const uint8_t* __restrict__ stream, long stream_bytes,
                                                              const long* __restrict__ total, int nsegmax,
                                                              int* __restrict__ cnt) {
  __shared__ int part[4];
  const int seg = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const long bits = total[b];
  const int nbytes = (int)((bits + 7) >> 3), i0 = seg * kSegBytes + tid * 8;
  if (seg * kSegBytes >= nbytes) return;                     // block-uniform
  const int c = i0 < nbytes ? count_ff(stream8(stream + (long)b * stream_bytes, i0, nbytes, bits)) : 0;
  int sum;
  block_excl_scan(c, part, &sum);
  if (tid == 0) cnt[(long)b * nsegmax + seg] = sum;
}

__global__ __launch_bounds__(kSegT) void jpeg_stuff_kernel(const uint8_t* __restrict__ stream, long stream_bytes,
                                                           const long* __restrict__ total, int nsegmax,
                                                           const int* __restrict__ segoff, uint8_t* __restrict__ out,
                                                           long out_stride) {
  __shared__ int part[4];
  const int seg = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const long bits = total[b];
  const int nbytes = (int)((bits + 7) >> 3), i0 = seg * kSegBytes + tid * 8;
  if (seg * kSegBytes >= nbytes) return;                     // block-uniform
  const bool live = i0 < nbytes;
  const unsigned long long x = live ? stream8(stream + (long)b * stream_bytes, i0, nbytes, bits) : 0;
  int sum;
  const int before = block_excl_scan(live ? count_ff(x) : 0, part, &sum);
  if (!live) return;
  uint8_t* dst = out + (long)b * out_stride + i0 + segoff[(long)b * nsegmax + seg] + before;
  const int n = min(8, nbytes - i0);
  for (int k = 0; k < n; ++k) {
    const uint8_t v = (uint8_t)(x >> (8 * k));
    *dst++ = v;
    if (v == 0xFF) *dst++ = 0;
  }
}

inline long mcus(int H, int W) { return (((long)H + 15) >> 4) * (((long)W + 15) >> 4); }
inline long align16(long v) { return (v + 15) & ~15L; }

struct Layout {
  long nmcu, ngroups, nsegmax, stream_bytes;                 // per image
  long coef, wgbits, total, segcnt, stream, end;             // byte offsets in the workspace
};

Layout layout(int B, int H, int W) {
  Layout l;
  l.nmcu = mcus(H, W);
  l.ngroups = (l.nmcu + kHMcus - 1) / kHMcus;
  const long cap = 6 * l.nmcu * kBlockMaxBytes;              // the unstuffed bound; a multiple of 8
  l.stream_bytes = cap + 8;                                  // + the dword the scan clears at the very end
  l.nsegmax = (cap + kSegBytes - 1) / kSegBytes;
  l.coef = 0;
  l.wgbits = align16(l.coef + (long)B * l.nmcu * 6 * 64 * 2);
  l.total = align16(l.wgbits + (long)B * l.ngroups * 8);
  l.segcnt = align16(l.total + (long)B * 8);
  l.stream = align16(l.segcnt + (long)B * l.nsegmax * 4);
  l.end = l.stream + (long)B * l.stream_bytes;
  return l;
}

}  // namespace

long jpeg_encode_bound(int H, int W) { return 2 * 6 * mcus(H, W) * kBlockMaxBytes + 2; }

long jpeg_encode_ws_bytes(int B, int H, int W) { return layout(B, H, W).end; }

void jpeg_encode(const uint8_t* img, int B, int H, int W, const int* qt_dev, int rgb, void* ws, uint8_t* out,
                 long out_stride, int* lens, hipStream_t s) {
  const Layout l = layout(B, H, W);
  IRX_CHECK(B <= 65535 && ((long)H + 15) / 16 <= 65535, "batch and H / 16 must fit a grid dimension");
  IRX_CHECK(6 * l.nmcu * kBlockMaxBytes < (1L << 31), "image too large: the scan bound must stay below 2 GiB");
  IRX_CHECK(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  char* w = static_cast<char*>(ws);
  uint32_t* coef = reinterpret_cast<uint32_t*>(w + l.coef);
  long* wgbits = reinterpret_cast<long*>(w + l.wgbits);
  long* total = reinterpret_cast<long*>(w + l.total);
  int* segcnt = reinterpret_cast<int*>(w + l.segcnt);
  uint8_t* stream = reinterpret_cast<uint8_t*>(w + l.stream);
  const int mcuw = (W + 15) >> 4, mcuh = (H + 15) >> 4;
  const dim3 hgrid((unsigned)l.ngroups, B), sgrid((unsigned)l.nsegmax, B);
  jpeg_coef_kernel<<<dim3((unsigned)((mcuw + 3) / 4), (unsigned)mcuh, B), kJT, 0, s>>>(img, H, W, qt_dev, rgb, coef);
  IRX_LAUNCH_CHECK();
  const int16_t* c16 = reinterpret_cast<const int16_t*>(coef);
  uint32_t* st32 = reinterpret_cast<uint32_t*>(stream);
  jpeg_huff_kernel<false><<<hgrid, kHT, 0, s>>>(c16, (int)l.nmcu, (int)l.ngroups, wgbits, st32, l.stream_bytes / 4);
  IRX_LAUNCH_CHECK();
  jpeg_scan_bits_kernel<<<B, kScanT, 0, s>>>(wgbits, (int)l.ngroups, total, st32, l.stream_bytes / 4);
  IRX_LAUNCH_CHECK();
  jpeg_huff_kernel<true><<<hgrid, kHT, 0, s>>>(c16, (int)l.nmcu, (int)l.ngroups, wgbits, st32, l.stream_bytes / 4);
  IRX_LAUNCH_CHECK();
  jpeg_ff_count_kernel<<<sgrid, kSegT, 0, s>>>(stream, l.stream_bytes, total, (int)l.nsegmax, segcnt);
  IRX_LAUNCH_CHECK();
  jpeg_scan_ff_kernel<<<B, kScanT, 0, s>>>(segcnt, (int)l.nsegmax, total, lens);
  IRX_LAUNCH_CHECK();
  jpeg_stuff_kernel<<<sgrid, kSegT, 0, s>>>(stream, l.stream_bytes, total, (int)l.nsegmax, segcnt, out, out_stride);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
