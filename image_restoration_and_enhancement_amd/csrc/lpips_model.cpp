// irx — LPIPS(alex) as a native model (models.h LpipsAlex): the torchvision AlexNet `features` convolutions under
// their state_dict names, the lpips package's five `lin` weights, and the forward pass over pred and gt as one batch.
//
//   input table -> conv 3(4)->64 11x11 s4 p2  [tap 0] -> ReLU + pool 3/2 -> conv 64->192 5x5 p2 [tap 1] -> ReLU + pool 3/2
//   -> conv 192->384 3x3 p1 [tap 2] -> ReLU -> conv 384->256 3x3 p1 [tap 3] -> ReLU -> conv 256->256 3x3 p1 [tap 4]
//
// Every conv stores its pre-ReLU output: the head applies the ReLU on load and the pool / copy kernels apply it in
// front of the next conv, so gemm()'s epilogues stay as they are.  Each tap's head runs right after its conv.
#include <climits>

#include "models.h"

namespace irx {

namespace {
struct ConvSpec { const char* name; int cout, cin, k, stride, pad; };
constexpr ConvSpec kConvs[5] = {{"features.0", 64, 3, 11, 4, 2},
                                {"features.3", 192, 64, 5, 1, 2},
                                {"features.6", 384, 192, 3, 1, 1},
                                {"features.8", 256, 384, 3, 1, 1},
                                {"features.10", 256, 256, 3, 1, 1}};
int conv_out(int n, const ConvSpec& c) { return (n + 2 * c.pad - c.k) / c.stride + 1; }
int pool_out(int n) { return (n - 3) / 2 + 1; }
}  // namespace

LpipsAlex::LpipsAlex(const irx_model_config& cfg, int dtype) : Model(IRX_MODEL_LPIPS, cfg, dtype) {
  IRX_CHECK(dtype == F32, "the LPIPS model is fp32 only");
  for (int i = 0; i < 5; ++i) {
    const ConvSpec& c = kConvs[i];
    const std::string n = c.name;
    cw_[i] = conv(n + ".weight", c.cout, c.k, c.k, (c.cin + 3) / 4 * 4);   // conv1: Cin 3 -> 4, zero padded
    cb_[i] = vec(n + ".bias", c.cout);
  }
  for (int i = 0; i < 5; ++i) lw_[i] = vec("lin" + std::to_string(i) + ".model.1.weight", kConvs[i].cout);
}

void LpipsAlex::run(Ctx& c, const uint8_t* pred, const uint8_t* gt, int B, int H, int W, const float* lut,
                    double* total, double* layers) {
  const bool dry = c.ws->dry();
  const int N = 2 * B;
  const int h0 = conv_out(H, kConvs[0]), w0 = conv_out(W, kConvs[0]);
  double* lay = (double*)c.ws->alloc((size_t)B * 5 * sizeof(double));
  double* part = (double*)c.ws->alloc((size_t)B * lpips_head_blocks(h0 * w0) * sizeof(double));   // tap 0 has the most

  Act x = new_act(c, N, H, W, 4);
  if (!dry) lpips_input(pred, gt, B, H, W, lut, (float*)x.p, c.s);
  for (int i = 0; i < 5; ++i) {
    const ConvSpec& k = kConvs[i];
    Act f = new_act(c, N, conv_out(x.h, k), conv_out(x.w, k), k.cout);
    conv2d(c, x, nullptr, cw_[i], cb_[i], k.cout, k.k, k.stride, k.pad, k.pad, x.h, x.w, f);
    drop(c, x);
    if (!dry)
      lpips_head((const float*)f.p, B, f.h * f.w, k.cout, fptr(lw_[i]), i, part, lay, layers, total, c.s);
    if (i < 4) {
      const int win = i < 2 ? 3 : 1, st = i < 2 ? 2 : 1;
      x = new_act(c, N, i < 2 ? pool_out(f.h) : f.h, i < 2 ? pool_out(f.w) : f.w, k.cout);
      if (!dry) lpips_relu_pool((const float*)f.p, N, f.h, f.w, k.cout, win, st, (float*)x.p, c.s);
    }
    drop(c, f);
  }
  c.ws->free(part);
  c.ws->free(lay);
}

size_t LpipsAlex::workspace_bytes(int B, int H, int W) {
  IRX_CHECK(B > 0 && B <= 32767 && H >= kMinSide && W >= kMinSide, "LPIPS: batch in [1, 32767], H, W >= 31");
  IRX_CHECK((long)2 * B * H * W * 4 <= (long)INT_MAX, "LPIPS: batch x image too large for one call");
  Arena ar;
  ar.reset(nullptr, 0);
  Ctx c{nullptr, &ar};
  run(c, nullptr, nullptr, B, H, W, nullptr, nullptr, nullptr);
  return ar.peak();
}

void LpipsAlex::score(hipStream_t s, const uint8_t* pred, const uint8_t* gt, int B, int H, int W, const float* lut,
                      double* total, double* layers, char* ws, size_t cap) {
  IRX_CHECK(blob_, "weights not bound");
  IRX_CHECK(((uintptr_t)ws % 16) == 0, "workspace must be 16-byte aligned");
  // sized before the first launch: a short workspace is refused whole, not met half way through the trunk
  const size_t need = workspace_bytes(B, H, W);
  IRX_CHECK(cap >= need, "workspace too small: " + std::to_string(cap) + " < " + std::to_string(need));
  Arena ar;
  ar.reset(ws, cap);
  Ctx c{s, &ar};
  run(c, pred, gt, B, H, W, lut, total, layers);
}

}  // namespace irx
