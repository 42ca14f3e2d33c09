// irx — baseline JPEG decoder on the GPU: the pixels PIL.Image.open(f).convert("RGB") returns (src/metrics.py:40-46
// load_image, scripts/generate_predictions.py:68) for the files PIL.save and cv2.imwrite write by default, bit for
// bit, from the entropy-coded bytes resident in HBM.  The marker walk is jpeg_parse.cpp (host); the pixel half
// (dequantise, jidctint IDCT, output stage, fancy up-sampling, YCbCr -> RGB) is jpeg_idct.h, shared with the JPEG round
// trip (degrade_jpeg.hip).  This file adds the entropy decoder.  jpeg_host.py is the same decoder, sequential, in
// Python and the oracle.
//
// A Huffman stream has no known symbol boundaries and these files carry no restart markers, so the decoder is the
// self-synchronising kind: the unstuffed bit stream of an image is cut into subsequences of S = subseq_bits, a lane
// owns the symbols that START in its subsequence, and what it needs to decode them is its entry state: (bit offset
// of its first symbol, block index within the MCU, zigzag position).  A lane started in a wrong state usually falls
// into step with the true symbol sequence after a while (the code is not prefix-synchronised, but wrong paths do
// not survive long), after which its exit state is the true one whatever it started from.
//
// Eight launches and one memset per batch (+ one device copy per image when the caller asks for the coefficients),
// none of which walks an image's symbols on one lane:
//   1 jd_count_kernel    stuffed 0x00 bytes (a 0x00 after a 0xFF) per 2048-byte segment of the scan.
//   2 jd_scan_kernel     per image: exclusive scan of the counts; the unstuffed length.
//   3 jd_compact_kernel  copies every other byte to its final offset; 0xFF after the last byte (bits past the end of
//                        the stream read as 1, the padding libjpeg writes; all-ones is no code of any table).
//   4 jd_sync_kernel     entry states.  One workgroup per image walks the subsequences in passes of 256 lanes and
//                        carries the state from pass to pass.  Round 0 decodes every subsequence of the pass from
//                        (0, 0, 0), the first one from the carried state, which is right.  Round r re-decodes each
//                        lane whose predecessor's exit state changed in round r - 1 from that state.  After round r,
//                        lanes 0..r of the pass have their true entry and exit states (induction: lane 0 has them
//                        from round 0, and lane i + 1 decodes in round r + 1 from lane i's exit state of round r).
//                        A round in which no exit state changes is the fixed point: every lane's entry state is its
//                        predecessor's exit state, lane 0 is right, so all are.  At most 257 rounds per pass (the
//                        loop bound), decided by __syncthreads_or, so the count is uniform.  Then a prefix sum of the
//                        blocks each lane begins gives every lane the index of its first block.
//   5 jd_write_kernel    grid-wide: every subsequence once more from its resolved entry state, storing the int16
//                        coefficients (DC: the difference) at [block][64] in zigzag order; blocks past the frame's
//                        count are dropped.  The coefficients of the whole batch are one region, zeroed by one memset.
//   6 jd_dc_kernel       per image and component: prefix sum of the DC differences in scan order.
//   7 jd_idct_kernel     24 blocks per workgroup, 8 lanes per block: dequantise with the file's tables, both IDCT
//                        passes (transposed through LDS), output stage.  4:2:0: Y / Cb / Cr planes padded to whole
//                        MCUs in the workspace (the dummy blocks of the last MCU column and row land in the padding and
//                        are never read); one component: straight to the output, [H][W] or replicated to [H][W][3].
//                        Status 4 where a block is outside the range in which libjpeg's C and SIMD IDCTs agree.
//   8 jd_upsample_kernel 4:2:0 only: fancy up-sampling and colour conversion, as the round trip's second kernel.
// No kernel waits on a flag written by another workgroup.
//
// Bounds that can be read off the code.  Every decode step consumes at least one bit: an assigned code has a length
// >= 1; an unassigned one (no code of the table matches the next 16 bits) consumes exactly one bit and leaves
// (block, zigzag) alone; bits past the end read as 1.  So a lane's loop runs at most S times per round.  A symbol is
// at most 16 + 11 = 27 bits, so a lane overshoots its subsequence by at most 26 bits (5 bits of the packed state) and
// a symbol never spans a whole subsequence (S >= 32).  Stream reads are two aligned dwords at p >> 5 with p below
// the stream's bit length, inside the 0xFF tail written by kernel 3.
//
// Budget.  LDS: the four Huffman tables of the image, 4 x 904 B = 3616 B (an 8-bit first-level table of
// length << 8 | symbol, then maxcode / offset per length 9..16 and the symbols, jdhuff.c's slow path), + 1 KB of exit
// states + scan slots in kernel 4: 4.7 KB per workgroup.  The decode loop holds the 32-bit window, the state and a
// handful of table words: about 40 VGPRs, no scratch (nothing is indexed dynamically in registers).
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/irx.h"
#include "block_scan.h"
#include "jpeg_idct.h"
#include "jpeg_tables.h"

namespace irx {
namespace {

using namespace jpegdev;
using jpegtab::kZigzag;

constexpr int kT = 256;                       // lanes of every per-image kernel; the pass width of kernel 4
constexpr int kSegBytes = kT * 8;
constexpr int kDefaultSubseqBits = 1024;
constexpr int kStreamTail = 16;               // bytes of capacity past the stuffed length rounded up to 4
constexpr long kMaxScanBytes = 1L << 27;      // bit offsets stay below 2^30

struct HuffDev {
  uint16_t fast[256];                         // by the next 8 bits: length << 8 | symbol; 0: longer than 8 bits
  int maxcode[17];                            // [l]: the largest code of length l, -1: none (used for l = 9..16)
  int delta[17];                              // [l]: index of the first symbol of length l - its code
  uint8_t vals[256];
};
static_assert(sizeof(HuffDev) == 904, "LDS budget in the header of this file");

struct ImgDesc {
  int H, W, ncomp, bpm, nblocks, mcuw;        // bpm: blocks per MCU (6 or 1); mcuw: MCUs (blocks) per row
  int scan_len, nseg, nsub_cap, pad;
  long scan_off;                              // in `scans`
  long segcnt, stream, entry, blkbase, coef, planes;   // byte offsets in the workspace
  long out_off;
  uint8_t dct[6], act[6], qtb[6], pad2[6];    // per block of the MCU: DC table, AC table, quantisation table
  uint16_t qt[2][64];
  HuffDev dc[2], ac[2];
};

struct Tables {
  HuffDev h[4];                               // dc0 dc1 ac0 ac1
};

__device__ __forceinline__ void load_tables(const ImgDesc* d, Tables* t) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&d->dc[0]);
  uint32_t* dst = reinterpret_cast<uint32_t*>(t);
  for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 4); i += blockDim.x) dst[i] = src[i];
}

// ------------------------------------------------------------------ 1-3: unstuffing
// the lane's 8 bytes and the one before them; bytes past the scan read as 0x01 (neither 0x00 nor 0xFF)
__device__ __forceinline__ void scan8(const uint8_t* sc, int i0, int len, uint8_t v[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const int i = i0 - 1 + k;
    v[k] = (i >= 0 && i < len) ? sc[i] : 1;
  }
}

__global__ __launch_bounds__(kT) void jd_count_kernel(const uint8_t* __restrict__ scans, const ImgDesc* __restrict__ desc,
                                                      char* __restrict__ ws) {
  __shared__ int part[4];
  const ImgDesc* d = desc + blockIdx.y;
  const int seg = blockIdx.x, tid = threadIdx.x, i0 = seg * kSegBytes + tid * 8;
  if (seg >= d->nseg) return;                                // block-uniform
  uint8_t v[9];
  scan8(scans + d->scan_off, i0, d->scan_len, v);
  int c = 0;
#pragma unroll
  for (int k = 1; k < 9; ++k) c += v[k] == 0 && v[k - 1] == 0xFF;
  int sum;
  block_excl_scan(c, part, &sum);
  if (tid == 0) reinterpret_cast<int*>(ws + d->segcnt)[seg] = sum;
}

__global__ __launch_bounds__(kT) void jd_scan_kernel(const ImgDesc* __restrict__ desc, char* __restrict__ ws,
                                                     int* __restrict__ nbytes) {
  __shared__ int part[4];
  const ImgDesc* d = desc + blockIdx.x;
  const int tid = threadIdx.x, n = d->nseg;
  int* cnt = reinterpret_cast<int*>(ws + d->segcnt);
  int carry = 0;
  for (int base = 0; base < n; base += kT) {
    const int i = base + tid;
    const int v = i < n ? cnt[i] : 0;
    int sum;
    const int ex = carry + block_excl_scan(v, part, &sum);
    if (i < n) cnt[i] = ex;
    carry += sum;
  }
  if (tid == 0) nbytes[blockIdx.x] = d->scan_len - carry;
}

__global__ __launch_bounds__(kT) void jd_compact_kernel(const uint8_t* __restrict__ scans,
                                                        const ImgDesc* __restrict__ desc, char* __restrict__ ws,
                                                        const int* __restrict__ nbytes) {
  __shared__ int part[4];
  const ImgDesc* d = desc + blockIdx.y;
  const int seg = blockIdx.x, tid = threadIdx.x, i0 = seg * kSegBytes + tid * 8, len = d->scan_len;
  if (seg >= d->nseg) return;                                // block-uniform
  uint8_t* st = reinterpret_cast<uint8_t*>(ws + d->stream);
  if (seg == 0 && tid < kStreamTail) {                       // the tail: capacity is align4(len) + kStreamTail
    const int n = nbytes[blockIdx.y], i = n + tid;
    if (i < ((len + 3) & ~3) + kStreamTail) st[i] = 0xFF;
  }
  uint8_t v[9];
  scan8(scans + d->scan_off, i0, len, v);
  int c = 0;
#pragma unroll
  for (int k = 1; k < 9; ++k) c += v[k] == 0 && v[k - 1] == 0xFF;
  int sum;
  int at = i0 - (reinterpret_cast<const int*>(ws + d->segcnt)[seg] + block_excl_scan(c, part, &sum));
#pragma unroll
  for (int k = 1; k < 9; ++k) {
    if (i0 + k - 1 >= len) break;
    if (v[k] == 0 && v[k - 1] == 0xFF) continue;
    st[at++] = v[k];                                         // at <= i0 + k - 1 < len
  }
}

// ------------------------------------------------------------------ the decode step (kernels 4 and 5)
// 32 bits of the stream at bit p (MSB first).  p < 8 * nbytes; reads dwords p >> 5 and (p >> 5) + 1.
__device__ __forceinline__ uint32_t peek32(const uint32_t* __restrict__ st, int p) {
  const int w = p >> 5, o = p & 31;
  const uint32_t d0 = __builtin_bswap32(st[w]), d1 = __builtin_bswap32(st[w + 1]);
  return o ? (d0 << o) | (d1 >> (32 - o)) : d0;
}

// packed state: bits 0..4 the bit offset past the lane's first bit, 5..7 the block of the MCU, 8..13 the zigzag
// position (0: a DC symbol is due)
__device__ __forceinline__ uint32_t pack_state(int off, int k, int z) { return (uint32_t)off | (k << 5) | (z << 8); }

// One symbol at (p, k, z).  Returns the bits consumed (>= 1).  *begun: a DC symbol was decoded (a block begins);
// *pos / *val: the coefficient to store (*pos < 0: none); *err: an unassigned code, or a run past position 63.
__device__ __forceinline__ int decode_step(const uint32_t* __restrict__ st, const Tables* t, const ImgDesc* d, int p,
                                           int& k, int& z, int bpm, bool* begun, int* pos, int* val, bool* err) {
  const uint32_t w = peek32(st, p);
  const HuffDev* h = z == 0 ? &t->h[d->dct[k]] : &t->h[2 + d->act[k]];
  const uint32_t w16 = w >> 16;
  int len = 0, sym = 0;
  const uint32_t e = h->fast[w16 >> 8];
  if (e) {
    len = (int)(e >> 8);
    sym = (int)(e & 255);
  } else {
#pragma unroll
    for (int l = 9; l <= 16; ++l) {
      const int c = (int)(w16 >> (16 - l));
      if (len == 0 && c <= h->maxcode[l]) {
        len = l;
        sym = h->vals[(c + h->delta[l]) & 255];
      }
    }
  }
  *begun = false;
  *pos = -1;
  *err = false;
  if (len == 0) {                                            // unassigned: one bit, (k, z) stay
    *err = true;
    return 1;
  }
  int used = len;
  if (z == 0) {
    const int s = min(sym, 11);                              // the parser admits no DC category above 11
    int v = s ? (int)((w << len) >> (32 - s)) : 0;
    if (s && v < (1 << (s - 1))) v -= (1 << s) - 1;
    used += s;
    *begun = true;
    *pos = 0;
    *val = v;
    z = 1;
  } else {
    const int r = sym >> 4, s = min(sym & 15, 10);           // ... and no AC size above 10
    if (s == 0) {
      z = r == 15 ? z + 16 : 64;
      *err = r == 15 && z > 63;
    } else {
      z += r;
      int v = (int)((w << len) >> (32 - s));
      if (v < (1 << (s - 1))) v -= (1 << s) - 1;
      used += s;
      if (z > 63) {
        *err = true;
      } else {
        *pos = z;
        *val = v;
      }
      z += 1;
    }
  }
  if (z >= 64) {
    k = k + 1 == bpm ? 0 : k + 1;
    z = 0;
  }
  return used;
}

// subsequence i from `entry`: the exit state (its offset counted from the end of the subsequence, which is the
// start of subsequence i + 1 or, in the last one, the end of the stream) and the blocks begun
__device__ __forceinline__ uint32_t run_subseq(const uint32_t* __restrict__ st, const Tables* t, const ImgDesc* d,
                                               int i, int S, int nbits, uint32_t entry, int* blocks) {
  int p = i * S + (int)(entry & 31), k = (int)(entry >> 5) & 7, z = (int)(entry >> 8) & 63;
  const int end = min((i + 1) * S, nbits), bpm = d->bpm;
  int n = 0;
  while (p < end) {                                          // at most S steps: each consumes >= 1 bit
    bool begun, err;
    int pos, val;
    p += decode_step(st, t, d, p, k, z, bpm, &begun, &pos, &val, &err);
    n += begun;
  }
  *blocks = n;
  return pack_state(p - end, k, z);                          // 0 <= p - end <= 26
}

// ------------------------------------------------------------------ 4: entry states
__global__ __launch_bounds__(kT) void jd_sync_kernel(const ImgDesc* __restrict__ desc, char* __restrict__ ws,
                                                     const int* __restrict__ nbytes, int S, int* __restrict__ status,
                                                     int* __restrict__ rounds) {
  __shared__ Tables tab;
  __shared__ uint32_t ex[kT];
  __shared__ int part[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const ImgDesc* d = desc + b;
  load_tables(d, &tab);
  const uint32_t* st = reinterpret_cast<const uint32_t*>(ws + d->stream);
  uint32_t* entry_out = reinterpret_cast<uint32_t*>(ws + d->entry);
  int* base_out = reinterpret_cast<int*>(ws + d->blkbase);
  const int nbits = 8 * nbytes[b], nsub = (nbits + S - 1) / S;
  __syncthreads();
  uint32_t carry = 0;                                        // the true entry state of the pass's first lane
  int blkcarry = 0, worst = 0;
  for (int base = 0; base < nsub; base += kT) {
    const int i = base + tid;
    const bool live = i < nsub;
    uint32_t entry = tid == 0 ? carry : 0, exit = 0;
    int cnt = 0;
    if (live) exit = run_subseq(st, &tab, d, i, S, nbits, entry, &cnt);
    ex[tid] = exit;
    __syncthreads();
    int r = 1;
    for (; r <= kT; ++r) {                                   // round r; lanes 0..r-1 of the pass are already right
      const uint32_t want = tid == 0 ? carry : ex[tid - 1];
      __syncthreads();                                       // every lane has read its predecessor's exit state
      int changed = 0;
      if (live && want != entry) {
        entry = want;
        const uint32_t e = run_subseq(st, &tab, d, i, S, nbits, entry, &cnt);
        changed = e != exit;
        exit = e;
        ex[tid] = e;
      }
      if (!__syncthreads_or(changed)) break;
    }
    worst = max(worst, min(r, kT) + 1);                      // rounds 0..r
    if (live) entry_out[i] = entry;
    int sum;
    const int first = blkcarry + block_excl_scan(cnt, part, &sum);
    if (live) base_out[i] = first;
    blkcarry += sum;
    carry = ex[kT - 1];                                      // used only when another pass follows: then all lanes are live
    __syncthreads();                                         // ... and read before the next pass overwrites ex[]
    if (base + kT >= nsub && tid == nsub - 1 - base) {
      // the last lane: every block of the frame was begun and finished, and no symbol ran past the end
      const bool bad = blkcarry != d->nblocks || exit != 0;  // exit: offset past the end, block of the MCU, position
      status[b] = bad ? 2 : 0;
    }
  }
  if (tid == 0) {
    rounds[b] = worst;
    if (nsub == 0) status[b] = 2;
  }
}

// ------------------------------------------------------------------ 5: coefficients
__global__ __launch_bounds__(kT) void jd_write_kernel(const ImgDesc* __restrict__ desc, char* __restrict__ ws,
                                                      const int* __restrict__ nbytes, int S,
                                                      int* __restrict__ status) {
  __shared__ Tables tab;
  const int b = blockIdx.y, tid = threadIdx.x;
  const ImgDesc* d = desc + b;
  const int nbits = 8 * nbytes[b], nsub = (nbits + S - 1) / S;
  if ((int)blockIdx.x * kT >= nsub) return;                  // block-uniform
  load_tables(d, &tab);
  __syncthreads();
  const int i = blockIdx.x * kT + tid;
  if (i >= nsub) return;
  const uint32_t* st = reinterpret_cast<const uint32_t*>(ws + d->stream);
  int16_t* coef = reinterpret_cast<int16_t*>(ws + d->coef);
  const uint32_t entry = reinterpret_cast<const uint32_t*>(ws + d->entry)[i];
  int next = reinterpret_cast<const int*>(ws + d->blkbase)[i];     // the index of the next block to begin
  int p = i * S + (int)(entry & 31), k = (int)(entry >> 5) & 7, z = (int)(entry >> 8) & 63;
  int cur = next - 1;                                        // the block under way (unused while z == 0)
  const int end = min((i + 1) * S, nbits), bpm = d->bpm, nblocks = d->nblocks;
  bool bad = false;
  while (p < end) {
    if (z == 0 && next >= nblocks) break;                    // the padding behind the last block
    bool begun, err;
    int pos, val;
    p += decode_step(st, &tab, d, p, k, z, bpm, &begun, &pos, &val, &err);
    bad |= err;
    if (begun) cur = next++;
    if (pos >= 0 && cur >= 0 && cur < nblocks) coef[(long)cur * 64 + pos] = (int16_t)val;
  }
  if (bad) atomicOr(status + b, 1);
}

// ------------------------------------------------------------------ 6: DC prediction
__global__ __launch_bounds__(kT) void jd_dc_kernel(const ImgDesc* __restrict__ desc, char* __restrict__ ws) {
  __shared__ int part[4];
  const ImgDesc* d = desc + blockIdx.y;
  const int comp = blockIdx.x, tid = threadIdx.x;
  if (comp >= d->ncomp) return;                              // block-uniform
  int16_t* coef = reinterpret_cast<int16_t*>(ws + d->coef);
  const int nmcu = d->nblocks / d->bpm, per = (d->bpm == 6 && comp == 0) ? 4 : 1, n = nmcu * per;
  const int first = d->bpm == 6 ? (comp == 0 ? 0 : 3 + comp) : 0;
  int carry = 0;
  for (int base = 0; base < n; base += kT) {                 // fixed order: the sums are integers anyway
    const int i = base + tid;
    int16_t* c = coef + ((long)(i / per) * d->bpm + first + i % per) * 64;
    const int v = i < n ? *c : 0;
    int sum;
    const int ex = carry + block_excl_scan(v, part, &sum);
    if (i < n) *c = (int16_t)(ex + v);                       // libjpeg keeps the predictor as int, the block as short
    carry += sum;
  }
}

// ------------------------------------------------------------------ 7, 8: pixels
struct InvZigzag {
  uint8_t v[64];
};
constexpr InvZigzag make_inv() {
  InvZigzag t{};
  for (int k = 0; k < 64; ++k) t.v[kZigzag[k]] = (uint8_t)k;
  return t;
}
__constant__ InvZigzag kNatToZz = make_inv();      // zigzag position of a natural (row-major) index

inline __host__ __device__ long pad16(long v) { return (v + 15) & ~15L; }

// Status 4: the inputs of a 1-D pass sum to more than 32767 in magnitude, or a column-pass output exceeds it.  Below
// that every intermediate of jidctint fits 32 bits and every 16-bit partial sum of libjpeg-turbo's SIMD version
// fits its lane, so the C code, the SIMD code and this kernel agree; above it they do not (the SIMD code saturates
// and wraps 16-bit lanes), and the file is left to PIL.  Coefficients that come from 8-bit pixels stay far below:
// the inputs of a pass have a 2-norm of at most 8192, so their magnitudes sum to at most 23171.
constexpr int kIdctSafeSum = 32767;

__device__ __forceinline__ int abs_sum8(const int v[8]) {
  int s = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += min(abs(v[e]), 1 << 20);  // 8 x 2^20 cannot overflow
  return s;
}

__global__ __launch_bounds__(kJT) void jd_idct_kernel(const ImgDesc* __restrict__ desc, char* __restrict__ ws, int rgb,
                                                      uint8_t* __restrict__ out, int* __restrict__ status) {
  __shared__ int blk[kJBlkInts];
  const ImgDesc* d = desc + blockIdx.y;
  const int tid = threadIdx.x, bi = tid >> 3, l = tid & 7;
  if ((int)blockIdx.x * 24 >= d->nblocks) return;            // block-uniform
  const int j = blockIdx.x * 24 + bi;                        // the block in scan order
  const bool live = j < d->nblocks;
  const int bpm = d->bpm, mcu = j / bpm, bk = j - mcu * bpm;
  int v[8];
  bool unsafe = false;
  if (live) {                                                // dequantise, inverse columns
    const int16_t* c = reinterpret_cast<const int16_t*>(ws + d->coef) + (long)j * 64;
    const uint16_t* q = d->qt[d->qtb[bk]];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (int)c[kNatToZz.v[e * 8 + l]] * (int)q[e * 8 + l];
    unsafe = abs_sum8(v) > kIdctSafeSum;
    if (unsafe) {                                            // keep the arithmetic below inside 32 bits
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0;
    }
    idct8<kIdctColBits>(v);
#pragma unroll
    for (int e = 0; e < 8; ++e) unsafe |= abs(v[e]) > kIdctSafeSum;
    int* p = blk + bi * kJBlkStride + l;
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e * kJRow] = v[e];
  }
  __syncthreads();
  if (!live) return;
  const int* p = blk + bi * kJBlkStride + l * kJRow;         // inverse rows, output stage
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = p[e];
  if (abs_sum8(v) > kIdctSafeSum) {
    unsafe = true;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0;
  }
  if (unsafe) atomicOr(status + blockIdx.y, 4);
  idct8<kIdctRowBits>(v);
  const int H = d->H, W = d->W, mx = mcu % d->mcuw, my = mcu / d->mcuw;
  if (bpm == 6) {
    const long H16 = pad16(H), W16 = pad16(W);
    uint8_t* yp = reinterpret_cast<uint8_t*>(ws + d->planes);
    uint8_t* dst;
    if (bk < 4)
      dst = yp + ((long)my * 16 + (bk >> 1) * 8 + l) * W16 + mx * 16 + (bk & 1) * 8;
    else
      dst = yp + H16 * W16 + (bk - 4) * (H16 * W16 / 4) + ((long)my * 8 + l) * (W16 / 2) + mx * 8;
    *reinterpret_cast<uint2*>(dst) = pack_row(v);            // planes are 8-aligned: widths are multiples of 8
  } else {
    const int y = my * 8 + l, x0 = mx * 8, ch = rgb ? 3 : 1;
    if (y >= H) return;
    uint8_t* o = out + d->out_off + ((long)y * W + x0) * ch;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (x0 + e >= W) break;
      const uint8_t s = (uint8_t)sample_limit(v[e]);
      if (rgb) {
        o[3 * e] = s;
        o[3 * e + 1] = s;
        o[3 * e + 2] = s;
      } else {
        o[e] = s;
      }
    }
  }
}

// one lane per horizontal pixel pair of one output row (4:2:0 images only)
__global__ __launch_bounds__(kT) void jd_upsample_kernel(const ImgDesc* __restrict__ desc, const char* __restrict__ ws,
                                                         uint8_t* __restrict__ out) {
  const ImgDesc* d = desc + blockIdx.y;
  if (d->bpm != 6) return;
  const int H = d->H, W = d->W, CW = (W + 1) / 2;
  const long i = (long)blockIdx.x * kT + threadIdx.x;
  if (i >= (long)H * CW) return;
  const long H16 = pad16(H), W16 = pad16(W);
  const uint8_t* yp = reinterpret_cast<const uint8_t*>(ws + d->planes);
  const uint8_t* cbp = yp + H16 * W16;
  upsample_pair(yp, cbp, cbp + H16 * W16 / 4, H, W, (int)W16, 1, (int)(i % CW), (int)(i / CW), out + d->out_off);
}

// ------------------------------------------------------------------ host
inline long align16(long v) { return (v + 15) & ~15L; }

void make_huff(const uint8_t* bits, const uint8_t* vals, int count, HuffDev* h) {
  std::memset(h, 0, sizeof(*h));
  std::memcpy(h->vals, vals, (size_t)count);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    h->maxcode[l] = -1;
    h->delta[l] = k - code;
    for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code)
      if (l <= 8)
        for (int f = 0; f < (1 << (8 - l)); ++f) h->fast[(code << (8 - l)) + f] = (uint16_t)((l << 8) | vals[k]);
    if (bits[l - 1]) h->maxcode[l] = code - 1;
    code <<= 1;
  }
}

struct Plan {
  std::vector<ImgDesc> desc;
  long desc_off = 0, nbytes_off = 0, coef_off = 0, coef_bytes = 0, end = 0;   // the coefficients of all images: one region
  int max_nseg = 0, max_nsub = 0, max_nblocks = 0;
  long max_pairs = 0;
};

// what jpeg_parse.cpp guarantees of a table and make_huff relies on: the symbols are as many as the code counts say,
// and the codes fit their lengths with all-ones left free (so no index leaves HuffDev::fast or the symbol array)
bool table_ok(const uint8_t* bits, int count, int cap) {
  if (count < 1 || count > cap) return false;
  int n = 0;
  long code = 0;
  for (int l = 0; l < 16; ++l) {
    n += bits[l];
    code += bits[l];
    if (code > (1L << (l + 1)) - 1) return false;
    code <<= 1;
  }
  return n == count;
}

bool info_ok(const irx_jpeg_info& f) {
  if (f.H < 8 || f.W < 8 || f.H > 65535 || f.W > 65535 || (f.ncomp != 1 && f.ncomp != 3)) return false;
  if (f.scan_len < 1 || f.scan_len > kMaxScanBytes) return false;
  for (int c = 0; c < f.ncomp; ++c) {
    if ((unsigned)f.qsel[c] > 1 || (unsigned)f.dcsel[c] > 1 || (unsigned)f.acsel[c] > 1) return false;
    if (f.qt[f.qsel[c]][0] == 0) return false;
  }
  for (int t = 0; t < 2; ++t) {                              // a table the file does not define has count 0
    if (f.dc_count[t] != 0 && !table_ok(f.dc_bits[t], f.dc_count[t], 16)) return false;
    if (f.ac_count[t] != 0 && !table_ok(f.ac_bits[t], f.ac_count[t], 256)) return false;
  }
  for (int c = 0; c < f.ncomp; ++c)
    if (f.dc_count[f.dcsel[c]] == 0 || f.ac_count[f.acsel[c]] == 0) return false;
  return true;
}

bool subseq_ok(int S) { return S >= 32 && S <= 65536 && S % 32 == 0; }

Plan plan(const irx_jpeg_info* infos, int B, int S) {
  Plan pl;
  pl.desc.resize(B);
  long at = 0;
  pl.desc_off = at;
  at = align16(at + (long)B * sizeof(ImgDesc));
  pl.nbytes_off = at;
  at = align16(at + (long)B * 4);
  for (int b = 0; b < B; ++b) {
    const irx_jpeg_info& f = infos[b];
    ImgDesc& d = pl.desc[b];
    std::memset(&d, 0, sizeof(d));
    d.H = f.H;
    d.W = f.W;
    d.ncomp = f.ncomp;
    d.bpm = f.ncomp == 3 ? 6 : 1;
    const int unit = f.ncomp == 3 ? 16 : 8;
    d.mcuw = (f.W + unit - 1) / unit;
    d.nblocks = d.mcuw * ((f.H + unit - 1) / unit) * d.bpm;
    d.scan_len = (int)f.scan_len;
    d.nseg = (d.scan_len + kSegBytes - 1) / kSegBytes;
    d.nsub_cap = (int)((8L * d.scan_len + S - 1) / S);
    for (int k = 0; k < d.bpm; ++k) {
      const int c = d.bpm == 6 ? (k < 4 ? 0 : k - 3) : 0;
      d.dct[k] = (uint8_t)f.dcsel[c];
      d.act[k] = (uint8_t)f.acsel[c];
      d.qtb[k] = (uint8_t)f.qsel[c];
    }
    std::memcpy(d.qt, f.qt, sizeof(d.qt));
    for (int t = 0; t < 2; ++t) {                            // info_ok has checked the tables
      if (f.dc_count[t]) make_huff(f.dc_bits[t], f.dc_vals[t], f.dc_count[t], &d.dc[t]);
      if (f.ac_count[t]) make_huff(f.ac_bits[t], f.ac_vals[t], f.ac_count[t], &d.ac[t]);
    }
    d.segcnt = at;
    at = align16(at + 4L * d.nseg);
    d.stream = at;
    at = align16(at + ((d.scan_len + 3) & ~3) + kStreamTail);
    d.entry = at;
    at = align16(at + 4L * d.nsub_cap);
    d.blkbase = at;
    at = align16(at + 4L * d.nsub_cap);
    d.planes = at;
    if (d.bpm == 6) at = align16(at + pad16(f.H) * pad16(f.W) * 3 / 2);
    pl.max_nseg = std::max(pl.max_nseg, d.nseg);
    pl.max_nsub = std::max(pl.max_nsub, d.nsub_cap);
    pl.max_nblocks = std::max(pl.max_nblocks, d.nblocks);
    if (d.bpm == 6) pl.max_pairs = std::max(pl.max_pairs, (long)f.H * ((f.W + 1) / 2));
  }
  pl.coef_off = at;                                          // 128 bytes per block: every image's part is 16-aligned
  for (int b = 0; b < B; ++b) {
    pl.desc[b].coef = at;
    at += 128L * pl.desc[b].nblocks;
  }
  pl.coef_bytes = at - pl.coef_off;
  pl.end = align16(at);
  return pl;
}

// The descriptors travel through pinned memory so that the copy is ordered on the caller's stream and the call does
// not wait for the device; the buffer is reused once the previous call's copy has completed.
struct Staging {
  void* p = nullptr;                                         // portable pinned memory: any device may copy from it
  size_t cap = 0;
  hipEvent_t ev = nullptr;                                   // belongs to device `dev`
  int dev = -1;
  bool pending = false;                                      // a copy from p may be in flight; ev follows it
};
thread_local Staging g_stage;

// the buffer, free to be overwritten, with an event of the current device
void* stage(size_t bytes) {
  Staging& g = g_stage;
  if (g.pending) {
    IRX_HIP(hipEventSynchronize(g.ev));
    g.pending = false;
  }
  int dev = 0;
  IRX_HIP(hipGetDevice(&dev));
  if (g.ev && g.dev != dev) {                                // the thread has switched GPUs: nothing is pending here
    IRX_HIP(hipEventDestroy(g.ev));
    g.ev = nullptr;
  }
  if (!g.ev) {
    IRX_HIP(hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
    g.dev = dev;
  }
  if (g.cap < bytes) {
    if (g.p) IRX_HIP(hipHostFree(g.p));
    g.p = nullptr;
    g.cap = 0;
    IRX_HIP(hipHostMalloc(&g.p, bytes, hipHostMallocPortable));
    g.cap = bytes;
  }
  return g.p;
}

// the staged bytes to dst on stream s.  Should the copy or the event fail, the stream is drained before the error
// leaves, so the buffer is never overwritten under a copy that is still in flight.
void stage_copy(void* dst, size_t bytes, hipStream_t s) {
  Staging& g = g_stage;
  hipError_t e = hipMemcpyAsync(dst, g.p, bytes, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(g.ev, s);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    throw Error(std::string("jpeg_decode: staging the descriptors failed: ") + hipGetErrorString(e));
  }
  g.pending = true;
}

}  // namespace

long jpeg_decode_ws_bytes(const irx_jpeg_info* infos, int B, int subseq_bits) {
  const int S = subseq_bits ? subseq_bits : kDefaultSubseqBits;
  if (!infos || B < 0 || !subseq_ok(S)) return 0;
  for (int b = 0; b < B; ++b)
    if (!info_ok(infos[b])) return 0;
  return plan(infos, B, S).end;
}

void jpeg_decode(const uint8_t* scans, const long* scan_off, const irx_jpeg_info* infos, int B, int subseq_bits,
                 int rgb, void* ws, uint8_t* out, const long* out_off, int* status, int* rounds, int16_t* coef,
                 const long* coef_off, hipStream_t s) {
  const int S = subseq_bits ? subseq_bits : kDefaultSubseqBits;
  IRX_CHECK(subseq_ok(S), "subseq_bits must be a multiple of 32 in 32 .. 65536 (or 0 for the default)");
  IRX_CHECK(B <= 65535, "batch must fit a grid dimension");
  IRX_CHECK(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  for (int b = 0; b < B; ++b) {
    IRX_CHECK(info_ok(infos[b]), "an info irx_jpeg_parse did not fill, or a scan above 128 MiB");
    IRX_CHECK(rgb || infos[b].ncomp == 1, "rgb == 0 (mode L) takes one-component files only");
    IRX_CHECK(scan_off[b] >= 0 && out_off[b] >= 0 && (!coef || coef_off[b] >= 0), "negative offset");
  }
  Plan pl = plan(infos, B, S);
  for (int b = 0; b < B; ++b) {
    pl.desc[b].scan_off = scan_off[b];
    pl.desc[b].out_off = out_off[b];
  }
  char* w = static_cast<char*>(ws);
  const size_t dbytes = (size_t)B * sizeof(ImgDesc);
  void* host = stage(dbytes);
  std::memcpy(host, pl.desc.data(), dbytes);
  stage_copy(w + pl.desc_off, dbytes, s);
  const ImgDesc* desc = reinterpret_cast<const ImgDesc*>(w + pl.desc_off);
  int* nbytes = reinterpret_cast<int*>(w + pl.nbytes_off);
  IRX_HIP(hipMemsetAsync(w + pl.coef_off, 0, pl.coef_bytes, s));   // the op zeroes the coefficients itself
  const dim3 sgrid((unsigned)pl.max_nseg, B);
  jd_count_kernel<<<sgrid, kT, 0, s>>>(scans, desc, w);
  IRX_LAUNCH_CHECK();
  jd_scan_kernel<<<B, kT, 0, s>>>(desc, w, nbytes);
  IRX_LAUNCH_CHECK();
  jd_compact_kernel<<<sgrid, kT, 0, s>>>(scans, desc, w, nbytes);
  IRX_LAUNCH_CHECK();
  jd_sync_kernel<<<B, kT, 0, s>>>(desc, w, nbytes, S, status, rounds);
  IRX_LAUNCH_CHECK();
  jd_write_kernel<<<dim3((unsigned)((pl.max_nsub + kT - 1) / kT), B), kT, 0, s>>>(desc, w, nbytes, S, status);
  IRX_LAUNCH_CHECK();
  jd_dc_kernel<<<dim3(3, B), kT, 0, s>>>(desc, w);
  IRX_LAUNCH_CHECK();
  if (coef)                                                  // the tests' output: one copy per image, to the caller's offsets
    for (int b = 0; b < B; ++b)
      IRX_HIP(hipMemcpyAsync(coef + coef_off[b], w + pl.desc[b].coef, 128L * pl.desc[b].nblocks,
                             hipMemcpyDeviceToDevice, s));
  jd_idct_kernel<<<dim3((unsigned)((pl.max_nblocks + 23) / 24), B), kJT, 0, s>>>(desc, w, rgb, out, status);
  IRX_LAUNCH_CHECK();
  if (pl.max_pairs) {
    jd_upsample_kernel<<<dim3((unsigned)((pl.max_pairs + kT - 1) / kT), B), kT, 0, s>>>(desc, w, out);
    IRX_LAUNCH_CHECK();
  }
}

}  // namespace irx
