// The Stable Diffusion safety checker around its CLIP vision tower (safety_host.py; diffusers 0.35.2
// StableDiffusionSafetyChecker.forward, which the reference's img2img calls end with: src/inference.py:486, :566, :664).
// The tower's GEMMs, LayerNorms and attention are the engine's (safety_model.cpp); these are the four kernels besides.
//
//   safety_patches_kernel  uint8 [B][S][S][3], already resized and cropped -> patch rows [B * P][Kpad] of the engine
//                          dtype: column k = (c * pz + ky) * pz + kx, the flatten of the patch conv's weight
//                          [D][3][pz][pz]; every value is read from the host's float[256][3] table of the processor's
//                          rescale + normalise (safety_host.input_table) and then cast, columns [3 pz pz, Kpad) are 0.
//   safety_tokens_kernel   tokens[b][0] = class_embedding + pos[0], tokens[b][1 + p] = patch_out[b][p] + pos[1 + p]:
//                          one fp32 add of the two rounded operands, one rounding to the engine dtype.
//   safety_head_kernel     one block per image, all fp32: |x| from a fixed strided + butterfly sum, x / max(|x|, 1e-12)
//                          as F.normalize writes it, one wave per concept row for the dot products (the same strided +
//                          butterfly order), then thread 0 runs the decision loop: (cos - thr) + adj, * 1000, rintf > 0.
//                          Nothing in it depends on the batch: an image's scores have the same bits at every B.
//   safety_blank_kernel    zeroes image b (and its fp32 [0, 1] copy) where flags[b] != 0; flags are read from device
//                          memory, so the host never waits for the decision.
// Built with -ffp-contract=off: the decision's subtract, add and multiply stay three roundings, as numpy's.
#include <algorithm>
#include <string>

#include "ops.h"
#include "profile.h"

namespace irx {
namespace {

constexpr int SF_NT = 256;
constexpr int SF_WAVES = SF_NT / 64;

template <typename T>
__global__ __launch_bounds__(SF_NT) void safety_patches_kernel(const uint8_t* __restrict__ img, int S, int pz, int Kpad,
                                                               long total, const float* __restrict__ lut,
                                                               T* __restrict__ out) {
  __shared__ float tab[256 * 3];
  for (int i = threadIdx.x; i < 256 * 3; i += SF_NT) tab[i] = lut[i];
  __syncthreads();
  const long idx = (long)blockIdx.x * SF_NT + threadIdx.x;
  if (idx >= total) return;
  const int G = S / pz, P = G * G, K = 3 * pz * pz;
  const long row = idx / Kpad;
  const int k = (int)(idx - row * Kpad);
  float v = 0.f;
  if (k < K) {
    const int c = k / (pz * pz), r = k - c * pz * pz, ky = r / pz, kx = r - ky * pz;
    const long b = row / P;
    const int p = (int)(row - b * P), py = p / G, px = p - py * G;
    const int y = py * pz + ky, x = px * pz + kx;
    v = tab[(int)img[((b * S + y) * S + x) * 3 + c] * 3 + c];
  }
  out[idx] = from_f<T>(v);
}

template <typename T>
__global__ __launch_bounds__(SF_NT) void safety_tokens_kernel(const T* __restrict__ patch, const float* __restrict__ cls,
                                                              const T* __restrict__ pos, int P, int D, long total,
                                                              T* __restrict__ out) {
  const long idx = (long)blockIdx.x * SF_NT + threadIdx.x;
  if (idx >= total) return;
  const int d = (int)(idx % D);
  const long tokrow = idx / D;                    // b * (P + 1) + t
  const long b = tokrow / (P + 1);
  const int t = (int)(tokrow - b * (P + 1));
  const T c = from_f<T>(cls[d]);                  // the class embedding as the engine dtype holds it
  const float a = t == 0 ? ld_f<T>(&c) : ld_f<T>(patch + ((b * P + t - 1) * D + d));
  out[idx] = from_f<T>(a + ld_f<T>(pos + (long)t * D + d));
}

// sum over a wave in a fixed butterfly order (every lane ends with the same bits)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int SF_MAX_ROWS = 64;      // n_special + n_concepts at most
constexpr int SF_MAX_PROJ = 4096;    // projection_dim at most (the normalised embedding sits in LDS)

__global__ __launch_bounds__(SF_NT) void safety_head_kernel(const float* __restrict__ emb, int n,
                                                            const float* __restrict__ special, int ns,
                                                            const float* __restrict__ conc, int nc,
                                                            const float* __restrict__ thr_special,
                                                            const float* __restrict__ thr_concept,
                                                            float* __restrict__ scores, int* __restrict__ flags) {
  __shared__ float xn[SF_MAX_PROJ];
  __shared__ float part[SF_WAVES];
  __shared__ float cosv[SF_MAX_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = emb + (long)blockIdx.x * n;
  float ss = 0.f;
  for (int i = tid; i < n; i += SF_NT) ss += x[i] * x[i];
  ss = wave_sum(ss);
  if (lane == 0) part[wave] = ss;
  __syncthreads();
  const float norm = fmaxf(sqrtf((part[0] + part[1]) + (part[2] + part[3])), 1e-12f);
  for (int i = tid; i < n; i += SF_NT) xn[i] = x[i] / norm;
  __syncthreads();
  const int rows = ns + nc;
  for (int q = wave; q < rows; q += SF_WAVES) {
    const float* e = q < ns ? special + (long)q * n : conc + (long)(q - ns) * n;
    float acc = 0.f;
    for (int i = lane; i < n; i += 64) acc += xn[i] * e[i];
    acc = wave_sum(acc);
    if (lane == 0) cosv[q] = acc;
  }
  __syncthreads();
  if (tid < rows) scores[(long)blockIdx.x * rows + tid] = cosv[tid];
  if (tid == 0) {
    float adj = 0.f;
    for (int k = 0; k < ns; ++k) {
      const float v = ((cosv[k] - thr_special[k]) + adj) * 1000.0f;
      if (rintf(v) > 0.f) adj = 0.01f;
    }
    int flagged = 0;
    for (int k = 0; k < nc; ++k) {
      const float v = ((cosv[ns + k] - thr_concept[k]) + adj) * 1000.0f;
      if (rintf(v) > 0.f) flagged = 1;
    }
    flags[blockIdx.x] = flagged;
  }
}

// zero n bytes at p: bytes up to the first 16-byte boundary, uint4 stores, the tail bytes
__device__ __forceinline__ void zero_bytes(uint8_t* p, long n, long t, long nthreads) {
  const long head = min(n, (long)((16 - ((uintptr_t)p & 15)) & 15));
  const long nvec = (n - head) / 16;
  const long tail0 = head + nvec * 16;
  for (long i = t; i < head; i += nthreads) p[i] = 0;
  uint4* v = reinterpret_cast<uint4*>(p + head);
  for (long i = t; i < nvec; i += nthreads) v[i] = make_uint4(0u, 0u, 0u, 0u);
  for (long i = tail0 + t; i < n; i += nthreads) p[i] = 0;
}

__global__ __launch_bounds__(SF_NT) void safety_blank_kernel(uint8_t* __restrict__ img, float* __restrict__ f01, long n,
                                                             const int* __restrict__ flags) {
  const long b = blockIdx.y;
  if (flags[b] == 0) return;
  const long t = (long)blockIdx.x * SF_NT + threadIdx.x, nt = (long)gridDim.x * SF_NT;
  zero_bytes(img + b * n, n, t, nt);
  if (f01) zero_bytes(reinterpret_cast<uint8_t*>(f01 + b * n), n * (long)sizeof(float), t, nt);
}

#define SF_DISPATCH(dtype, KERNEL_CALL)        \
  do {                                         \
    if ((dtype) == F32) {                      \
      using T = float;                         \
      KERNEL_CALL;                             \
    } else if ((dtype) == F16) {               \
      using T = f16_t;                         \
      KERNEL_CALL;                             \
    } else {                                   \
      using T = bf16_t;                        \
      KERNEL_CALL;                             \
    }                                          \
    IRX_LAUNCH_CHECK();                        \
  } while (0)

int nblk(long n) { return (int)((n + SF_NT - 1) / SF_NT); }

}  // namespace

void safety_patches(int dtype, const uint8_t* img, int B, int S, int pz, int Kpad, const float* lut, void* out,
                    hipStream_t s) {
  IRX_CHECK(B > 0 && pz > 0 && S >= pz && S % pz == 0, "safety patches: the image side must be a multiple of the patch");
  IRX_CHECK(Kpad >= 3 * pz * pz, "safety patches: padded K below 3 * patch * patch");
  const long total = (long)B * (S / pz) * (S / pz) * Kpad;
  IRX_CHECK(total / SF_NT < (1L << 31) - 1, "safety patches: batch too large for one launch");
  ProfScope ps(prof_on() ? std::string("irx::(anonymous namespace)::safety_patches_kernel") : std::string(), 0.0, s);
  SF_DISPATCH(dtype, (safety_patches_kernel<T><<<nblk(total), SF_NT, 0, s>>>(img, S, pz, Kpad, total, lut, (T*)out)));
}

void safety_tokens(int dtype, const void* patch, const float* cls, const void* pos, int B, int P, int D, void* out,
                   hipStream_t s) {
  IRX_CHECK(B > 0 && P > 0 && D > 0, "safety tokens: empty");
  const long total = (long)B * (P + 1) * D;
  IRX_CHECK(total / SF_NT < (1L << 31) - 1, "safety tokens: batch too large for one launch");
  ProfScope ps(prof_on() ? std::string("irx::(anonymous namespace)::safety_tokens_kernel") : std::string(), 0.0, s);
  SF_DISPATCH(dtype, (safety_tokens_kernel<T><<<nblk(total), SF_NT, 0, s>>>((const T*)patch, cls, (const T*)pos, P, D,
                                                                            total, (T*)out)));
}

void safety_head(const float* emb, int B, int n, const float* special, int ns, const float* conc, int nc,
                 const float* thr_special, const float* thr_concept, float* scores, int* flags, hipStream_t s) {
  IRX_CHECK(B > 0 && n > 0 && n <= SF_MAX_PROJ, "safety head: projection_dim must be in [1, 4096]");
  IRX_CHECK(ns >= 0 && nc >= 1 && ns + nc <= SF_MAX_ROWS, "safety head: at most 64 embedding rows, one concept at least");
  ProfScope ps(prof_on() ? std::string("irx::(anonymous namespace)::safety_head_kernel") : std::string(), 0.0, s);
  safety_head_kernel<<<B, SF_NT, 0, s>>>(emb, n, special, ns, conc, nc, thr_special, thr_concept, scores, flags);
  IRX_LAUNCH_CHECK();
}

void safety_blank(uint8_t* img, float* f01, int B, long n, const int* flags, hipStream_t s) {
  IRX_CHECK(B > 0 && B <= 65535 && n > 0, "safety blank: batch in [1, 65535], a non-empty image");
  const int bx = (int)std::min<long>(256, (n + SF_NT * 16 - 1) / (SF_NT * 16));
  ProfScope ps(prof_on() ? std::string("irx::(anonymous namespace)::safety_blank_kernel") : std::string(), 0.0, s);
  safety_blank_kernel<<<dim3(bx, B), SF_NT, 0, s>>>(img, f01, n, flags);
  IRX_LAUNCH_CHECK();
}

}  // namespace irx
