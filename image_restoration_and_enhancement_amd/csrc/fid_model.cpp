// irx — torchvision's InceptionV3 trunk as a native model (models.h InceptionFid): the 94 BasicConv2d units under their
// state_dict names, in the order the forward pass runs them, and the forward pass to the 2048 pooled features.
//
//   stem: 1a 3x3/2 -> 2a 3x3 -> 2b 3x3 p1 -> max 3/2 -> 3b 1x1 -> 4a 3x3 -> max 3/2
//   Mixed_5b/5c/5d (A) -> Mixed_6a (B) -> Mixed_6b..6e (C) -> Mixed_7a (D) -> Mixed_7b/7c (E) -> global average
//
// A unit is conv (no bias, gemm()'s exact-f32 path, epilogue untouched) into a compact buffer, then fid_bn_relu with the
// host-folded scale / shift: in place for a unit inside a branch, into channels [off, off + cout) of the block's concat
// buffer for a branch's last unit, so no block copies its branches together.  The two max pools of Mixed_6a / Mixed_7a
// write their slice the same way.  Every intermediate is freed as soon as its last reader has been enqueued.
#include <climits>

#include "models.h"

namespace irx {

int InceptionFid::unit(const std::string& name, int cin, int cout, int kh, int kw, int stride, int ph, int pw) {
  Unit u;
  u.cin = cin; u.cout = cout; u.kh = kh; u.kw = kw; u.stride = stride; u.ph = ph; u.pw = pw;
  u.w = conv(name + ".conv.weight", cout, kh, kw, (cin + 3) / 4 * 4);   // the stem: Cin 3 -> 4, zero padded
  u.sc = vec(name + ".bn.scale", cout);
  u.sh = vec(name + ".bn.shift", cout);
  units_.push_back(u);
  return (int)units_.size() - 1;
}

InceptionFid::InceptionFid(const irx_model_config& cfg, int dtype) : Model(IRX_MODEL_FID, cfg, dtype) {
  IRX_CHECK(dtype == F32, "the FID model is fp32 only");
  unit("Conv2d_1a_3x3", 3, 32, 3, 3, 2);
  unit("Conv2d_2a_3x3", 32, 32, 3, 3);
  unit("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1);
  unit("Conv2d_3b_1x1", 64, 80, 1, 1);
  unit("Conv2d_4a_3x3", 80, 192, 3, 3);
  const struct { const char* n; int cin, pf; } A[3] = {{"Mixed_5b", 192, 32}, {"Mixed_5c", 256, 64}, {"Mixed_5d", 288, 64}};
  for (const auto& a : A) {
    const std::string n = a.n;
    unit(n + ".branch1x1", a.cin, 64, 1, 1);
    unit(n + ".branch5x5_1", a.cin, 48, 1, 1);
    unit(n + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2);
    unit(n + ".branch3x3dbl_1", a.cin, 64, 1, 1);
    unit(n + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
    unit(n + ".branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1);
    unit(n + ".branch_pool", a.cin, a.pf, 1, 1);
  }
  unit("Mixed_6a.branch3x3", 288, 384, 3, 3, 2);
  unit("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1);
  unit("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
  unit("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2);
  const struct { const char* n; int c7; } Cb[4] = {{"Mixed_6b", 128}, {"Mixed_6c", 160}, {"Mixed_6d", 160}, {"Mixed_6e", 192}};
  for (const auto& b : Cb) {
    const std::string n = b.n;
    const int c7 = b.c7;
    unit(n + ".branch1x1", 768, 192, 1, 1);
    unit(n + ".branch7x7_1", 768, c7, 1, 1);
    unit(n + ".branch7x7_2", c7, c7, 1, 7, 1, 0, 3);
    unit(n + ".branch7x7_3", c7, 192, 7, 1, 1, 3, 0);
    unit(n + ".branch7x7dbl_1", 768, c7, 1, 1);
    unit(n + ".branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0);
    unit(n + ".branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3);
    unit(n + ".branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0);
    unit(n + ".branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3);
    unit(n + ".branch_pool", 768, 192, 1, 1);
  }
  unit("Mixed_7a.branch3x3_1", 768, 192, 1, 1);
  unit("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2);
  unit("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1);
  unit("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3);
  unit("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0);
  unit("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2);
  const struct { const char* n; int cin; } E[2] = {{"Mixed_7b", 1280}, {"Mixed_7c", 2048}};
  for (const auto& e : E) {
    const std::string n = e.n;
    unit(n + ".branch1x1", e.cin, 320, 1, 1);
    unit(n + ".branch3x3_1", e.cin, 384, 1, 1);
    unit(n + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1);
    unit(n + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0);
    unit(n + ".branch3x3dbl_1", e.cin, 448, 1, 1);
    unit(n + ".branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1);
    unit(n + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1);
    unit(n + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0);
    unit(n + ".branch_pool", e.cin, 192, 1, 1);
  }
}

// ---------------------------------------------------------------------------------------------- units and pools
static int out_side(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }

Act InceptionFid::cbr(Ctx& c, const Act& x, int& ui) {
  const Unit& u = units_[ui++];
  IRX_CHECK(x.c == (u.cin + 3) / 4 * 4, "FID trunk: unit fed the wrong channel count");
  Act y = new_act(c, x.n, out_side(x.h, u.kh, u.stride, u.ph), out_side(x.w, u.kw, u.stride, u.pw), u.cout);
  conv2d(c, x, u.w, u.cout, u.kh, u.kw, u.stride, u.ph, u.pw, y);
  if (!c.ws->dry()) fid_bn_relu((const float*)y.p, y.pix(), u.cout, fptr(u.sc), fptr(u.sh), (float*)y.p, u.cout, c.s);
  return y;
}

void InceptionFid::cbr_into(Ctx& c, const Act& x, int& ui, Act& cat, int off) {
  const Unit& u = units_[ui++];
  IRX_CHECK(x.c == u.cin, "FID trunk: unit fed the wrong channel count");
  Act y = new_act(c, x.n, out_side(x.h, u.kh, u.stride, u.ph), out_side(x.w, u.kw, u.stride, u.pw), u.cout);
  IRX_CHECK(y.h == cat.h && y.w == cat.w && off % 4 == 0 && off + u.cout <= cat.c, "FID trunk: slice outside the concat");
  conv2d(c, x, u.w, u.cout, u.kh, u.kw, u.stride, u.ph, u.pw, y);
  if (!c.ws->dry())
    fid_bn_relu((const float*)y.p, y.pix(), u.cout, fptr(u.sc), fptr(u.sh), (float*)cat.p + off, cat.c, c.s);
  drop(c, y);
}

Act InceptionFid::avgpool(Ctx& c, const Act& x) {
  Act y = new_act(c, x.n, x.h, x.w, x.c);
  if (!c.ws->dry()) fid_avgpool3((const float*)x.p, x.n, x.h, x.w, x.c, (float*)y.p, c.s);
  return y;
}

Act InceptionFid::stem_pool(Ctx& c, Act& x) {   // the input is a ReLU output: lpips.hip's ReLU + pool is the plain pool
  Act y = new_act(c, x.n, out_side(x.h, 3, 2, 0), out_side(x.w, 3, 2, 0), x.c);
  if (!c.ws->dry()) lpips_relu_pool((const float*)x.p, x.n, x.h, x.w, x.c, 3, 2, (float*)y.p, c.s);
  drop(c, x);
  return y;
}

void InceptionFid::maxpool_into(Ctx& c, const Act& x, Act& cat, int off) {
  IRX_CHECK(out_side(x.h, 3, 2, 0) == cat.h && out_side(x.w, 3, 2, 0) == cat.w && off % 4 == 0 && off + x.c <= cat.c,
            "FID trunk: pool slice outside the concat");
  if (!c.ws->dry()) fid_maxpool3s2((const float*)x.p, x.n, x.h, x.w, x.c, (float*)cat.p + off, cat.c, c.s);
}

// ---------------------------------------------------------------------------------------------- blocks
Act InceptionFid::block_a(Ctx& c, Act& x, int& u) {
  const int pf = units_[u + 6].cout;
  Act cat = new_act(c, x.n, x.h, x.w, 224 + pf);
  cbr_into(c, x, u, cat, 0);
  Act t = cbr(c, x, u);
  cbr_into(c, t, u, cat, 64);
  drop(c, t);
  t = cbr(c, x, u);
  Act t2 = cbr(c, t, u);
  drop(c, t);
  cbr_into(c, t2, u, cat, 128);
  drop(c, t2);
  t = avgpool(c, x);
  cbr_into(c, t, u, cat, 224);
  drop(c, t);
  drop(c, x);
  return cat;
}

Act InceptionFid::block_b(Ctx& c, Act& x, int& u) {
  Act cat = new_act(c, x.n, out_side(x.h, 3, 2, 0), out_side(x.w, 3, 2, 0), 384 + 96 + x.c);
  cbr_into(c, x, u, cat, 0);
  Act t = cbr(c, x, u);
  Act t2 = cbr(c, t, u);
  drop(c, t);
  cbr_into(c, t2, u, cat, 384);
  drop(c, t2);
  maxpool_into(c, x, cat, 480);
  drop(c, x);
  return cat;
}

Act InceptionFid::block_c(Ctx& c, Act& x, int& u) {
  Act cat = new_act(c, x.n, x.h, x.w, 768);
  cbr_into(c, x, u, cat, 0);
  Act t = cbr(c, x, u);
  Act t2 = cbr(c, t, u);
  drop(c, t);
  cbr_into(c, t2, u, cat, 192);
  drop(c, t2);
  t = cbr(c, x, u);
  for (int i = 0; i < 3; ++i) {
    t2 = cbr(c, t, u);
    drop(c, t);
    t = t2;
  }
  cbr_into(c, t, u, cat, 384);
  drop(c, t);
  t = avgpool(c, x);
  cbr_into(c, t, u, cat, 576);
  drop(c, t);
  drop(c, x);
  return cat;
}

Act InceptionFid::block_d(Ctx& c, Act& x, int& u) {
  Act cat = new_act(c, x.n, out_side(x.h, 3, 2, 0), out_side(x.w, 3, 2, 0), 320 + 192 + x.c);
  Act t = cbr(c, x, u);
  cbr_into(c, t, u, cat, 0);
  drop(c, t);
  t = cbr(c, x, u);
  for (int i = 0; i < 2; ++i) {
    Act t2 = cbr(c, t, u);
    drop(c, t);
    t = t2;
  }
  cbr_into(c, t, u, cat, 320);
  drop(c, t);
  maxpool_into(c, x, cat, 512);
  drop(c, x);
  return cat;
}

Act InceptionFid::block_e(Ctx& c, Act& x, int& u) {
  Act cat = new_act(c, x.n, x.h, x.w, 2048);
  cbr_into(c, x, u, cat, 0);
  Act t = cbr(c, x, u);
  cbr_into(c, t, u, cat, 320);
  cbr_into(c, t, u, cat, 704);
  drop(c, t);
  t = cbr(c, x, u);
  Act t2 = cbr(c, t, u);
  drop(c, t);
  cbr_into(c, t2, u, cat, 1088);
  cbr_into(c, t2, u, cat, 1472);
  drop(c, t2);
  t = avgpool(c, x);
  cbr_into(c, t, u, cat, 1856);
  drop(c, t);
  drop(c, x);
  return cat;
}

// ---------------------------------------------------------------------------------------------- forward
void InceptionFid::run(Ctx& c, const float* in, int B, int H, int W, float* out) {
  Act x0;   // the caller's buffer: never freed here
  x0.p = (void*)in; x0.n = B; x0.h = H; x0.w = W; x0.c = 4;
  int u = 0;
  Act x = cbr(c, x0, u);
  for (int i = 0; i < 2; ++i) {
    Act y = cbr(c, x, u);
    drop(c, x);
    x = y;
  }
  x = stem_pool(c, x);
  for (int i = 0; i < 2; ++i) {
    Act y = cbr(c, x, u);
    drop(c, x);
    x = y;
  }
  x = stem_pool(c, x);
  for (int i = 0; i < 3; ++i) x = block_a(c, x, u);
  x = block_b(c, x, u);
  for (int i = 0; i < 4; ++i) x = block_c(c, x, u);
  x = block_d(c, x, u);
  for (int i = 0; i < 2; ++i) x = block_e(c, x, u);
  IRX_CHECK(u == (int)units_.size() && x.c == kFeatures, "FID trunk: units out of step with the graph");
  if (!c.ws->dry()) fid_gap((const float*)x.p, B, x.h * x.w, x.c, out, c.s);
  drop(c, x);
}

size_t InceptionFid::workspace_bytes(int B, int H, int W) {
  IRX_CHECK(B > 0 && B <= 4096 && H >= kMinSide && W >= kMinSide, "FID: batch in [1, 4096], H, W >= 75");
  // the largest activation is Conv2d_2b's: 64 channels at (H - 4) / 2 x (W - 4) / 2; bound all of them by B * H * W * 16
  IRX_CHECK((long)B * H * W * 16 <= (long)INT_MAX, "FID: batch x image too large for one call");
  Arena ar;
  ar.reset(nullptr, 0);
  Ctx c{nullptr, &ar};
  run(c, (const float*)(uintptr_t)4096, B, H, W, nullptr);
  return ar.peak();
}

void InceptionFid::features(hipStream_t s, const float* x, int B, int H, int W, float* out, char* ws, size_t cap) {
  IRX_CHECK(blob_, "weights not bound");
  IRX_CHECK(((uintptr_t)ws % 16) == 0 && ((uintptr_t)x % 16) == 0, "input and workspace must be 16-byte aligned");
  // sized before the first launch: a short workspace is refused whole, not met half way through the trunk
  const size_t need = workspace_bytes(B, H, W);
  IRX_CHECK(cap >= need, "workspace too small: " + std::to_string(cap) + " < " + std::to_string(need));
  Arena ar;
  ar.reset(ws, cap);
  Ctx c{s, &ar};
  run(c, x, B, H, W, out);
}

}  // namespace irx
