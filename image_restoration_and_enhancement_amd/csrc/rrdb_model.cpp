// irx — Real-ESRGAN's RRDBNet as a native model (models.h Rrdb): RRDBNet(3, 3, num_feat=64, num_block,
// num_grow_ch=32, scale=4) under its state_dict names (`conv_first`, `body.{i}.rdb{1,2,3}.conv{1..5}`, `conv_body`,
// `conv_up1`, `conv_up2`, `conv_hr`, `conv_last`), the network of RealESRGAN_x4plus.pth (src/inference.py:326-350).
//
// One graph, two forms of each conv:
//   fp16, rrdb_fused = 1 (the product):  rrdb_head, then rrdb_conv (rrdb.hip) for every other conv
//   fp32, or fp16 with rrdb_fused = 0:   input table -> per conv: gather of the channel prefix (unless dense), conv2d
//                                        to an fp32 sum without bias, rrdb_epilogue with the same rounding points
// A dense block lives in one [pixels][192] buffer (x | x1 | x2 | x3 | x4); three of them rotate: rdb1 in A, rdb2 in B,
// rdb3 in C, and rdb3's conv5 writes the RRDB's result over its input in A (res2 == out: each thread reads its own
// elements before it writes them; nobody reads A's halo in that launch).  The fp32 graph runs every conv on gemm()'s
// exact-f32 path (conv_first's Cin 3 padded to 4; to 8 in fp16).
#include <climits>

#include "models.h"

namespace irx {

Rrdb::Cv Rrdb::make(const std::string& name, int co, int ci) {
  Cv v;
  v.w = conv(name + ".weight", co, 3, 3, ci);
  v.b = vec(name + ".bias", co);
  return v;
}

Rrdb::Rrdb(const irx_model_config& cfg, int dtype) : Model(IRX_MODEL_RRDB, cfg, dtype) {
  IRX_CHECK(dtype == F32 || dtype == F16, "the RRDB model is fp16 (the product) or fp32 (parity); bf16 is refused");
  nb_ = cfg.num_layers;
  IRX_CHECK(nb_ >= 1 && nb_ <= 64, "RRDB: num_block (num_layers) must be in [1, 64]");
  IRX_CHECK(cfg.hidden_size == kFeat && cfg.intermediate_size == kGrow,
            "RRDB: the kernels are built for num_feat = 64 (hidden_size) and num_grow_ch = 32 (intermediate_size)");
  cin0_ = dtype == F32 ? 4 : 8;   // conv_first: Cin 3 zero padded to 16 bytes of elements
  first_ = make("conv_first", kFeat, cin0_);
  for (int i = 0; i < nb_; ++i)
    for (int j = 1; j <= 3; ++j) {
      Rdb r;
      for (int k = 0; k < 5; ++k)
        r.c[k] = make("body." + std::to_string(i) + ".rdb" + std::to_string(j) + ".conv" + std::to_string(k + 1),
                      k == 4 ? kFeat : kGrow, kFeat + k * kGrow);
      rdb_.push_back(r);
    }
  body_ = make("conv_body", kFeat, kFeat);
  up1_ = make("conv_up1", kFeat, kFeat);
  up2_ = make("conv_up2", kFeat, kFeat);
  hr_ = make("conv_hr", kFeat, kFeat);
  last_ = make("conv_last", kLastPad, kFeat);   // Cout 3 zero padded to 8 rows for the general conv kernels
}

void Rrdb::conv_glue(Ctx& c, const void* x, int ldx, int cin, int B, int Hs, int Ws, int up, const Cv& cv, int cout,
                     int lrelu, const void* r1, int ldr1, int r1_scaled, const void* r2, int ldr2, void* y, int ldy) {
  const bool dry = c.ws->dry();
  const int H = up ? 2 * Hs : Hs, W = up ? 2 * Ws : Ws;
  Act src;
  src.n = B; src.h = Hs; src.w = Ws; src.c = cin;
  Act dense;
  if (ldx != cin) {
    dense = new_act(c, B, Hs, Ws, cin);
    if (!dry) rrdb_gather(dt_, x, ldx, (long)B * Hs * Ws, cin, dense.p, c.s);
    src.p = dense.p;
  } else {
    src.p = const_cast<void*>(x);
  }
  Act acc;   // fp32 sums
  acc.n = B; acc.h = H; acc.w = W; acc.c = cout;
  acc.p = c.ws->alloc((size_t)B * H * W * cout * sizeof(float));
  conv2d(c, src, nullptr, cv.w, P{}, cout, 3, 1, 1, 1, H, W, acc, nullptr, 0, nullptr, 1);
  if (dense.p) drop(c, dense);
  if (!dry)
    rrdb_epilogue(dt_, (const float*)acc.p, (long)B * H * W, cout, fptr(cv.b), lrelu, r1, ldr1, r1_scaled, r2, ldr2, y,
                  ldy, c.s);
  drop(c, acc);
}

void Rrdb::run(Ctx& c, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8, float* out_f) {
  const bool dry = c.ws->dry();
  const bool fused = dt_ == F16 && g_rrdb_fused;
  const size_t es = dsize(dt_);
  // channel `ch` of a [pixels][ld] buffer
  auto at = [&](const Act& a, int ch) { return dry ? nullptr : (void*)((char*)a.p + (size_t)ch * es); };
  // one conv in either form; Hs x Ws is the source's size
  auto cv = [&](const void* x, int ldx, int cin, int Hs, int Ws, int up, const Cv& w, int cout, int lrelu,
                const void* r1, int ldr1, int r1s, const void* r2, int ldr2, void* y, int ldy) {
    if (!fused) {
      conv_glue(c, x, ldx, cin, B, Hs, Ws, up, w, cout, lrelu, r1, ldr1, r1s, r2, ldr2, y, ldy);
      return;
    }
    if (dry) return;
    RrdbConv a;
    a.x = x; a.ldx = ldx; a.cin = cin; a.up = up;
    a.w = ptr(w.w); a.bias = fptr(w.b); a.cout = cout; a.lrelu = lrelu;
    a.r1 = r1; a.ldr1 = ldr1; a.r1_scaled = r1s; a.r2 = r2; a.ldr2 = ldr2;
    a.y = y; a.ldy = ldy;
    a.B = B; a.H = up ? 2 * Hs : Hs; a.W = up ? 2 * Ws : Ws;
    rrdb_conv(a, c.s);
  };

  Act feat0 = new_act(c, B, H, W, kFeat);
  Act buf[3] = {new_act(c, B, H, W, kWide), new_act(c, B, H, W, kWide), new_act(c, B, H, W, kWide)};
  if (fused) {
    if (!dry)
      rrdb_head(img, B, H, W, lut, ptr(first_.w), cin0_, fptr(first_.b), feat0.p, kFeat, buf[0].p, kWide, c.s);
  } else {
    Act x = new_act(c, B, H, W, cin0_);
    if (!dry) srvgg_input(dt_, img, (long)B * H * W, lut, x.p, c.s);
    Act acc;
    acc.n = B; acc.h = H; acc.w = W; acc.c = kFeat;
    acc.p = c.ws->alloc((size_t)B * H * W * kFeat * sizeof(float));
    conv2d(c, x, nullptr, first_.w, P{}, kFeat, 3, 1, 1, 1, H, W, acc, nullptr, 0, nullptr, 1);
    if (!dry) {
      const long rows = (long)B * H * W;
      rrdb_epilogue(dt_, (const float*)acc.p, rows, kFeat, fptr(first_.b), 0, nullptr, 0, 0, nullptr, 0, feat0.p, kFeat,
                    c.s);
      rrdb_epilogue(dt_, (const float*)acc.p, rows, kFeat, fptr(first_.b), 0, nullptr, 0, 0, nullptr, 0, buf[0].p,
                    kWide, c.s);
    }
    drop(c, acc);
    drop(c, x);
  }
  for (int i = 0; i < nb_; ++i)
    for (int j = 0; j < 3; ++j) {
      const Rdb& r = rdb_[3 * i + j];
      const Act& p = buf[j];
      const Act& q = buf[(j + 1) % 3];      // rdb3's result goes back to A = buf[0]
      for (int k = 0; k < 4; ++k)
        cv(p.p, kWide, kFeat + k * kGrow, H, W, 0, r.c[k], kGrow, 1, nullptr, 0, 0, nullptr, 0,
           at(p, kFeat + k * kGrow), kWide);
      const bool end = j == 2;              // ... with the RRDB's own residual, read from A before it is overwritten
      cv(p.p, kWide, kWide, H, W, 0, r.c[4], kFeat, 0, p.p, kWide, 1, end ? q.p : nullptr, end ? kWide : 0, q.p,
         kWide);
    }
  Act f = new_act(c, B, H, W, kFeat);
  cv(buf[0].p, kWide, kFeat, H, W, 0, body_, kFeat, 0, feat0.p, kFeat, 0, nullptr, 0, f.p, kFeat);
  for (int j = 2; j >= 0; --j) drop(c, buf[j]);
  drop(c, feat0);
  Act u1 = new_act(c, B, 2 * H, 2 * W, kFeat);
  cv(f.p, kFeat, kFeat, H, W, 1, up1_, kFeat, 1, nullptr, 0, 0, nullptr, 0, u1.p, kFeat);
  drop(c, f);
  Act u2 = new_act(c, B, 4 * H, 4 * W, kFeat);
  cv(u1.p, kFeat, kFeat, 2 * H, 2 * W, 1, up2_, kFeat, 1, nullptr, 0, 0, nullptr, 0, u2.p, kFeat);
  drop(c, u1);
  Act hr = new_act(c, B, 4 * H, 4 * W, kFeat);
  cv(u2.p, kFeat, kFeat, 4 * H, 4 * W, 0, hr_, kFeat, 1, nullptr, 0, 0, nullptr, 0, hr.p, kFeat);
  drop(c, u2);
  if (fused) {
    if (!dry) {
      RrdbConv a;
      a.x = hr.p; a.ldx = kFeat; a.cin = kFeat;
      a.w = ptr(last_.w); a.bias = fptr(last_.b); a.cout = 3;
      a.out_u8 = out_u8; a.out_f = out_f;
      a.B = B; a.H = 4 * H; a.W = 4 * W;
      rrdb_conv(a, c.s);
    }
  } else {
    Act acc;
    acc.n = B; acc.h = 4 * H; acc.w = 4 * W; acc.c = kLastPad;
    acc.p = c.ws->alloc((size_t)B * 16 * H * W * kLastPad * sizeof(float));
    conv2d(c, hr, nullptr, last_.w, P{}, kLastPad, 3, 1, 1, 1, 4 * H, 4 * W, acc, nullptr, 0, nullptr, 1);
    if (!dry) rrdb_output(dt_, (const float*)acc.p, kLastPad, (long)B * 16 * H * W, fptr(last_.b), out_u8, out_f, c.s);
    drop(c, acc);
  }
  drop(c, hr);
}

size_t Rrdb::workspace_bytes(int B, int H, int W) {
  IRX_CHECK(B > 0 && H > 0 && W > 0, "RRDB: batch, H and W must be positive");
  const long hr_pix = (long)B * 16 * H * W;
  // the fused kernels index in 64 bits and count pixels in an int; conv2d counts the elements of [B][4H][4W][64]
  if (dt_ == F16 && g_rrdb_fused) IRX_CHECK(hr_pix <= (long)INT_MAX, "RRDB: batch x image too large for one call");
  else IRX_CHECK(hr_pix * kFeat <= (long)INT_MAX, "RRDB: batch x image too large for one call on the conv2d graph");
  Arena ar;
  ar.reset(nullptr, 0);
  Ctx c{nullptr, &ar};
  run(c, nullptr, B, H, W, nullptr, nullptr, nullptr);
  return ar.peak();
}

void Rrdb::enhance(hipStream_t s, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8,
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
