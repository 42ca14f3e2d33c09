// irx — Real-ESRGAN's compact network as a native model (models.h Srvgg): SRVGGNetCompact(3, 3, num_feat=64,
// num_conv=32, upscale=4, act_type='prelu') under its state_dict names (`body.{0,2,..,66}` the convs, `body.{1,3,..,65}`
// the PReLU slopes), the net the reference constructs (src/inference.py:335-336).
//
//   fp16, srvgg_fused = 1 (the product):  head -> 32 x body layer -> tail (srvgg.hip), two ping-pong activations
//   fp32, or fp16 with srvgg_fused = 0:   input table -> 33 x (conv2d + PReLU kernel) -> conv2d 64 -> 48 -> shuffle/add
// The fp32 graph runs every conv on gemm()'s exact-f32 path (Cin 3 padded to 4, as LPIPS does; to 8 in fp16).
#include <climits>

#include "models.h"

namespace irx {

Srvgg::Srvgg(const irx_model_config& cfg, int dtype) : Model(IRX_MODEL_SRVGG, cfg, dtype) {
  IRX_CHECK(dtype == F32 || dtype == F16, "the SRVGG model is fp16 (the product) or fp32 (parity); bf16 is refused");
  cin0_ = dtype == F32 ? 4 : 8;   // conv 0: Cin 3 zero padded to 16 bytes of elements
  for (int i = 0; i < kConvs; ++i) {
    const std::string n = "body." + std::to_string(2 * i);
    const int co = i == kConvs - 1 ? kOut : kFeat;
    cw_[i] = conv(n + ".weight", co, 3, 3, i == 0 ? cin0_ : kFeat);
    cb_[i] = vec(n + ".bias", co);
    if (i < kConvs - 1) sl_[i] = vec("body." + std::to_string(2 * i + 1) + ".weight", kFeat);
  }
}

void Srvgg::run(Ctx& c, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8, float* out_f) {
  const bool dry = c.ws->dry();
  if (dt_ == F16 && g_srvgg_fused) {
    Act x = new_act(c, B, H, W, kFeat), y = new_act(c, B, H, W, kFeat);
    if (!dry) srvgg_head(img, B, H, W, lut, ptr(cw_[0]), cin0_, fptr(cb_[0]), fptr(sl_[0]), x.p, c.s);
    for (int i = 1; i < kConvs - 1; ++i) {
      if (!dry) srvgg_conv(x.p, B, H, W, ptr(cw_[i]), fptr(cb_[i]), fptr(sl_[i]), y.p, c.s);
      std::swap(x, y);
    }
    if (!dry) srvgg_tail(x.p, img, B, H, W, lut, ptr(cw_[kConvs - 1]), fptr(cb_[kConvs - 1]), out_u8, out_f, c.s);
    drop(c, y);
    drop(c, x);
    return;
  }
  Act x = new_act(c, B, H, W, cin0_);
  if (!dry) srvgg_input(dt_, img, (long)B * H * W, lut, x.p, c.s);
  for (int i = 0; i < kConvs; ++i) {
    const int co = i == kConvs - 1 ? kOut : kFeat;
    Act f = new_act(c, B, H, W, co);
    conv2d(c, x, nullptr, cw_[i], cb_[i], co, 3, 1, 1, 1, H, W, f);
    drop(c, x);
    if (i < kConvs - 1) {
      if (!dry) srvgg_prelu(dt_, f.p, (long)B * H * W, kFeat, fptr(sl_[i]), f.p, c.s);   // in place
    } else if (!dry) {
      srvgg_shuffle_add(dt_, f.p, img, B, H, W, lut, out_u8, out_f, c.s);
    }
    x = f;
  }
  drop(c, x);
}

size_t Srvgg::workspace_bytes(int B, int H, int W) {
  IRX_CHECK(B > 0 && H > 0 && W > 0, "SRVGG: batch, H and W must be positive");
  // conv2d's rows and the output's elements are ints: the largest tensors are [B][H][W][64] and [B][4H][4W][3]
  IRX_CHECK((long)B * H * W * kFeat <= (long)INT_MAX, "SRVGG: batch x image too large for one call");
  Arena ar;
  ar.reset(nullptr, 0);
  Ctx c{nullptr, &ar};
  run(c, nullptr, B, H, W, nullptr, nullptr, nullptr);
  return ar.peak();
}

void Srvgg::enhance(hipStream_t s, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8,
                    float* out_f, char* ws, size_t cap) {
  IRX_CHECK(blob_, "weights not bound");
  IRX_CHECK(((uintptr_t)ws % 16) == 0, "workspace must be 16-byte aligned");
  // sized before the first launch: a short workspace is refused whole, not met half way through the body
  const size_t need = workspace_bytes(B, H, W);
  IRX_CHECK(cap >= need, "workspace too small: " + std::to_string(cap) + " < " + std::to_string(need));
  Arena ar;
  ar.reset(ws, cap);
  Ctx c{s, &ar};
  run(c, img, B, H, W, lut, out_u8, out_f);
}

}  // namespace irx
