// irx — native model graphs (UNet2DConditionModel, AutoencoderKL, CLIPTextModel, LPIPS AlexNet, FID InceptionV3,
// Real-ESRGAN SRVGGNetCompact, StableDiffusionSafetyChecker) over the irx kernels.
#pragma once
#include <map>
#include <memory>
#include <vector>

#include "../../include/irx.h"
#include "ops.h"

namespace irx {

extern int g_vae_attn_rows;   // VAE mid-block attention: query rows per score block (0 = auto, capped bytes)
extern int g_vae_flash;       // VAE mid-block attention in the 16-bit engines: flash kernel (1) / row-blocked (0)

// Deterministic first-fit allocator over a caller-owned workspace.  Run once with base == nullptr
// ("dry run": no kernels launched) to size the workspace, then for real with identical calls.
class Arena {
 public:
  void reset(char* base, size_t cap) {
    base_ = base; cap_ = cap; end_ = 0; peak_ = 0; free_.clear(); live_.clear(); ids_.clear(); next_id_ = 0;
  }
  void* alloc(size_t bytes);
  void free(void* p);
  size_t peak() const { return peak_; }
  bool dry() const { return base_ == nullptr; }

 private:
  char* base_ = nullptr;
  size_t cap_ = 0, end_ = 0, peak_ = 0;
  std::map<size_t, size_t> free_;    // offset -> size of free holes below end_
  std::map<size_t, size_t> live_;    // offset -> size
  std::map<size_t, int> ids_;        // offset -> allocation index (guard diagnostics)
  int next_id_ = 0;
};
// diagnostics (irx_set_option("arena_guard", 1)): every workspace allocation is followed by a 64 KiB guard filled with
// 0xA5, checked when the allocation is freed (device-synchronous; reports overruns on stderr)
extern int g_arena_guard;

struct P { size_t off = 0; bool set = false; };   // parameter reference into the weight blob

struct ParamEntry {
  std::string name;
  int layout, dtype;
  std::vector<int64_t> shape;
  size_t off, bytes;
  float row_scale = 1.f;     // packer scales rows [0, scale_rows) (folded attention scale)
  int64_t scale_rows = 0;
  std::string aux;           // irx_param_info::aux (LayerNorm fold sources)
};

struct Act {   // NHWC activation view
  void* p = nullptr;
  int n = 0, h = 0, w = 0, c = 0;
  double* gnp = nullptr;   // GroupNorm partials emitted by its producer (GemmArgs::gn_part), else null
  int gnr = 0;             // ... rows per partial (divides h * w)
  long pix() const { return (long)n * h * w; }
};

class Model {
 public:
  Model(int kind, const irx_model_config& cfg, int dtype) : kind_(kind), cfg_(cfg), dt_(dtype) {}
  virtual ~Model() = default;
  int kind() const { return kind_; }
  int dtype() const { return dt_; }
  const std::vector<ParamEntry>& manifest() const { return params_; }
  size_t blob_bytes() const { return blob_bytes_; }
  void bind(void* blob, size_t bytes);
  char* blob() const { return blob_; }   // the bound device blob (nullptr before bind)

 protected:
  P reg(const std::string& name, int layout, int dtype, std::vector<int64_t> shape, float row_scale = 1.f,
        int64_t scale_rows = 0, const std::string& aux = std::string());
  P vec(const std::string& name, int64_t n) { return reg(name, IRX_LAYOUT_VEC, F32, {n}); }
  P mat(const std::string& name, int64_t n, int64_t k) { return reg(name, IRX_LAYOUT_MAT, dt_, {n, k}); }
  P conv(const std::string& name, int64_t co, int64_t kh, int64_t kw, int64_t ci) {
    return reg(name, IRX_LAYOUT_CONV, dt_, {co, kh, kw, ci});
  }
  template <typename X = void> const X* ptr(P p) const { return (const X*)(blob_ + p.off); }
  const float* fptr(P p) const { return (const float*)(blob_ + p.off); }

  // ---- op helpers (skip launches in dry-run mode)
  struct Ctx { hipStream_t s; Arena* ws; };
  Act new_act(Ctx& c, int n, int h, int w, int ch);
  void drop(Ctx& c, Act& a) {
    c.ws->free(a.p);
    a.p = nullptr;
    if (a.gnp) c.ws->free(a.gnp);
    a.gnp = nullptr;
    a.gnr = 0;
  }
  // `stats`: the output feeds a GroupNorm -> the epilogue also emits its partial sums when it can (Act::gnp)
  void conv2d(Ctx& c, const Act& x0, const Act* x1, P w, P b, int cout, int k, int stride, int pad_t, int pad_l,
              int hv, int wv, Act& out, const float* rowadd = nullptr, long rowadd_ld = 0,
              const void* residual = nullptr, int out_f32 = 0, int ldc = -1, bool stats = false,
              long res_rows = 0);
  // the same with a kh x kw kernel ((1, 7), (7, 1), (1, 3), (3, 1) of InceptionV3): no bias, no epilogue extras
  void conv2d(Ctx& c, const Act& x, P w, int cout, int kh, int kw, int stride, int pad_t, int pad_l, Act& out,
              int ldc = -1);
  void linear(Ctx& c, const void* A, long lda, int M, int K, P w, int N, const float* bias, void* C, long ldc,
              int act = ACT_NONE, const void* residual = nullptr, long ldr = 0, int out_f32 = 0, int imgs = 0,
              Act* stats = nullptr, long res_rows = 0);
  void run_gemm(Ctx& c, GemmArgs& a, Act* stats = nullptr);   // split-K partials / GroupNorm partials
  void gnorm(Ctx& c, const Act& x0, const Act* x1, P g, P b, float eps, int silu, const Act& out);
  // GroupNorm(+SiLU) of (x0 | x1) followed by a 3x3 / stride-1 / pad-1 conv into `out`: folded into the
  // conv's halo operand path where it fits (gemm_gn_fusable), else a normalised copy and the plain conv
  void gn_conv3(Ctx& c, const Act& x0, const Act* x1, P g, P gb, float eps, int silu, P w, P b, int cout,
                Act& out, const float* rowadd = nullptr, long rowadd_ld = 0, const void* residual = nullptr,
                bool stats = false);
  void lnorm(Ctx& c, const void* x, int rows, int C, P g, P b, float eps, void* out);
  // diffusers Upsample2D (nearest resize to out's size, conv 3x3 pad 1): as 4 per-parity 2x2 convs of x (w2:
  // IRX_LAYOUT_CONV_UP2) when out is exactly 2x and the large-tile path takes the shape, else the resize conv (w)
  void upsample_conv(Ctx& c, const Act& x, P w, P w2, P b, int cout, Act& out, bool stats);
  P up2_weights(const std::string& name, int ch);   // IRX_LAYOUT_CONV_UP2 entry (16-bit engines; unset for fp32)
  // GroupNorm + SiLU + 3x3 conv to a narrow output head in one kernel (gn_conv_narrow); false: not taken
  bool gn_conv_out(Ctx& c, const Act& x, P g, P gb, float eps, P w, P b, int cout, void* out, int ldo, int out_f32);
  // one pre-LN CLIP encoder layer (transformers CLIPEncoderLayer; fused q|k|v): the text model's with the causal mask,
  // the safety checker's vision tower without.  make_clip_layer registers `<b>layer_norm1 ... mlp.fc2` in that order;
  // clip_layer updates the residual stream h [B][L][D] in place through the caller's scratch (n, att [M][D], qkv
  // [M][3D], f [M][F]); imgs: the images the rows span (GemmArgs::imgs; 0: not image-indexed)
  struct ClipLayerW { P ln1w, ln1b, qkvw, qkvb, ow, ob, ln2w, ln2b, f1w, f1b, f2w, f2b; };
  struct ClipScratch { void *n = nullptr, *qkv = nullptr, *att = nullptr, *f = nullptr; };
  ClipLayerW make_clip_layer(const std::string& b, int D, int F);
  void clip_layer(Ctx& c, const ClipLayerW& l, void* h, int B, int L, int D, int F, int H, float eps, int act,
                  int causal, int imgs, const ClipScratch& t);

  int kind_;
  irx_model_config cfg_;
  int dt_;
  std::vector<ParamEntry> params_;
  size_t blob_bytes_ = 0;
  char* blob_ = nullptr;
};

// ------------------------------------------------------------------ shared blocks
struct ResW {
  P n1w, n1b, c1w, c1b, n2w, n2b, c2w, c2b, scw, scb;
  int cin = 0, cout = 0;
  bool shortcut = false;
  long temb_off = -1;     // column offset into the fused time_emb_proj output (UNet only)
};

// LayerNorm row statistics a producer's epilogue wrote (GemmArgs::ln_out): the final (rstd, rstd * mean) pairs
// (T == 0) or T partials of W columns per row; p == nullptr: none, the consumer runs the statistics pass
struct LnStats { const float2* p = nullptr; int T = 0; int W = 0; };

class Unet : public Model {
 public:
  Unet(const irx_model_config& cfg, int dtype);
  int cin_pad() const { return cin_pad_; }
  // cfg_share: the caller promises that rows b and b + B / 2 carry the same input and timestep (the two halves of a
  // classifier-free-guidance batch), so the 16-bit engines run everything up to the first cross-attention on B / 2
  // images (run()); B must be even.  The fp32 engine ignores the promise (operation for operation the oracle).
  // time_proj: one fp32 [temb_cols] row of time_table() that holds for every image of the batch (they share one
  // timestep); run() then skips the time-embedding chain and does not read t.
  size_t workspace_bytes(int B, int h, int w, int cfg_share = 0, const float* time_proj = nullptr);
  // every resnet's time-embedding projection for n timesteps at once (t: device fp32 [n], n <= 256): table fp32
  // [n][temb_cols()], row i bit-identical to what forward() computes for an image at t[i]
  long temb_cols() const { return temb_cols_; }
  size_t time_table_ws(int n);
  void time_table(hipStream_t s, const float* t, int n, float* table, char* ws, size_t cap);
  size_t context_bytes(int B, int L) const { return (size_t)B * L * kv_cols_ * dsize(dt_); }
  void prepare_context(hipStream_t s, const void* ctx, int B, int L, void* kv, char* ws, size_t cap);
  void forward(hipStream_t s, const void* x, int B, int h, int w, const float* t, const void* kv, int L, float* eps,
               char* ws, size_t cap, int cfg_share = 0, const float* time_proj = nullptr);

 private:
  struct XfW {
    P nw, nb, piw, pib, ln1w, ln1b, qkvw, o1w, o1b, ln2w, ln2b, q2w, o2w, o2b, ln3w, ln3b, ffw, ffb, ff2w, ff2b, pow,
        pob;
    // LayerNorm fold (16-bit engines, ln_fold_): qkvw / q2w / ffw hold W * gamma; u = row sums of those, v = bias +
    // W beta (GemmArgs::ln_rs / ln_u)
    P qkvu, qkvv, q2u, q2v, ffu, ffv;
    // ff.net.2 folded through proj_out (16-bit engines): [W_po | W_po W_ff2] and b_po + W_po b_ff2 (IRX_LAYOUT_*_CHAIN)
    P pofw, pofb;
    int c = 0;
    long kv_off = 0;      // column offset into the fused cross-attention K|V cache
  };
  struct Block {
    std::vector<ResW> res;
    std::vector<XfW> attn;
    bool has_attn = false, resample = false;
    P rsw, rsb;           // down/upsampler conv
    P rsw2;               // upsampler: per-parity 2x2 weights (IRX_LAYOUT_CONV_UP2; 16-bit engines)
    int ch = 0;
  };
  ResW make_res(const std::string& p, int cin, int cout);
  XfW make_xf(const std::string& p, int c);
  void run(Ctx& c, const void* x, int B, int h, int w, const float* t, const void* kv, int L, float* eps,
           int cfg_share, const float* time_proj);
  void time_chain(Ctx& c, const float* t, int n, float* tproj);
  // (tld: row stride of tproj per image; 0: one row for the whole batch)
  Act resnet(Ctx& c, const ResW& r, Act& x0, Act* x1, const float* tproj, long tld, float eps);
  // dup: x holds the shared half of a classifier-free-guidance batch (run()): everything up to attn2.to_q runs on
  // x.n images, cross-attention reads that Q against the K|V of 2 x.n images, and the result has 2 x.n images
  Act transformer(Ctx& c, const XfW& a, Act& x, const void* kv, int L, bool dup = false);
  // LayerNorm(x) -> projection g (g.A / lda / bias set here): folded into g's epilogue when ln_fold_ and the shape
  // takes it — with the statistics from `parts` (the producer of x emitted them) or from a statistics pass written
  // to `st` — else through the normalised copy `nbuf`
  void ln_gemm(Ctx& c, GemmArgs& g, const void* x, int rows, int C, P lnw, P lnb, P u, P v, const float* bias,
               void* nbuf, float2* st, LnStats parts = LnStats());
  // a transformer projection that writes the residual stream (proj_in, to_out, to_out2): out = A W^T + bias
  // (+ residual), emitting the output's LayerNorm statistics into `lnp` where the epilogue can: final pairs at
  // C == 320, else partials per 320- or 128-column tile, whichever the planned tile gives (option ln_parts 2)
  // (res_rows: the residual repeats every res_rows rows, GemmArgs::res_rows)
  LnStats xf_proj(Ctx& c, const void* A, int M, int C, P w, const float* bias, void* out, const void* residual,
                  int imgs, float2* lnp, long res_rows = 0);

  int cin_pad_ = 8;
  bool ln_fold_ = false;   // LayerNorm folded into the transformer projections (fixed at creation: the blob layout)
  int temb_dim_ = 1280;
  long temb_cols_ = 0, kv_cols_ = 0;
  std::vector<std::string> temb_names_w_, temb_names_b_, kv_names_;
  P conv_in_w, conv_in_b, t1w, t1b, t2w, t2b, tpw, tpb, kvw, nout_w, nout_b, conv_out_w, conv_out_b;
  std::vector<Block> down_, up_;
  ResW mid_res0_, mid_res1_;
  XfW mid_attn_;
};

class Vae : public Model {
 public:
  Vae(const irx_model_config& cfg, int dtype);
  size_t encode_ws(int B, int H, int W);
  size_t decode_ws(int B, int h, int w);
  void encode(hipStream_t s, const void* img, int B, int H, int W, void* moments, char* ws, size_t cap);
  void decode(hipStream_t s, const void* z, int B, int h, int w, void* out, char* ws, size_t cap);

 private:
  struct AttW { P gw, gb, qkvw, qkvb, ow, ob; int c = 0; };
  ResW make_res(const std::string& p, int cin, int cout);
  AttW make_attn(const std::string& p, int c);
  Act resnet(Ctx& c, const ResW& r, Act& x);
  Act attn(Ctx& c, const AttW& a, Act& x);
  void run_encode(Ctx& c, const void* img, int B, int H, int W, void* moments);
  void run_decode(Ctx& c, const void* z, int B, int h, int w, void* out);

  P e_cin_w, e_cin_b, e_nout_w, e_nout_b, e_cout_w, e_cout_b, qw, qb, pqw, pqb, d_cin_w, d_cin_b, d_nout_w,
      d_nout_b, d_cout_w, d_cout_b;
  std::vector<std::vector<ResW>> e_res_, d_res_;
  std::vector<P> e_down_w_, e_down_b_, d_up_w_, d_up_b_, d_up2_w_;
  ResW e_mid0_, e_mid1_, d_mid0_, d_mid1_;
  AttW e_att_, d_att_;
};

class Clip : public Model {
 public:
  Clip(const irx_model_config& cfg, int dtype);
  size_t workspace_bytes(int B, int L);
  void encode(hipStream_t s, const int* ids, int B, int L, void* out, char* ws, size_t cap);

 private:
  void run(Ctx& c, const int* ids, int B, int L, void* out);
  P tok, pos, fw, fb;
  std::vector<ClipLayerW> layers_;
};

// diffusers' StableDiffusionSafetyChecker (safety_host.py; run_safety_checker at the end of the reference's img2img
// calls, src/inference.py:486, :566, :664): the CLIP vision tower (`vision_model.vision_model.*`: a bias-free patch conv
// as a GEMM over safety_patches' rows, class + position embeddings, pre_layrnorm, cfg.num_layers encoder layers without
// a mask, post_layernorm of token 0), `visual_projection`, and the cosine head of safety.hip against the blob's
// `special_care_embeds` / `concept_embeds` (fp32; packed as given: safety_gpu normalises them on the host) and their
// `*_weights` thresholds.  The tower runs in the model dtype, the projection's output and the head in fp32.  Every
// GEMM is planned for the canonical batch and the head is per image: an image's scores do not depend on the batch.
class SafetyChecker : public Model {
 public:
  SafetyChecker(const irx_model_config& cfg, int dtype);
  static constexpr int kMaxBatch = 64;   // per call (above it the small-M plans of the pooled rows would change)
  int side() const { return cfg_.image_size; }
  int rows() const { return cfg_.n_special + cfg_.n_concepts; }
  size_t workspace_bytes(int B);
  // crop uint8 [B][S][S][3]; lut float[256][3]; scores fp32 [B][n_special + n_concepts]; flags int [B]; embeds (or
  // null) fp32 [B][projection_dim], the image embeddings the head reads
  void check(hipStream_t s, const uint8_t* crop, int B, const float* lut, float* scores, int* flags, float* embeds,
             char* ws, size_t cap);

 private:
  void run(Ctx& c, const uint8_t* crop, int B, const float* lut, float* scores, int* flags, float* embeds);
  int kpad_ = 0;
  P patch_w, cls, pos, pre_w, pre_b, post_w, post_b, proj_w, sp_e, co_e, sp_t, co_t;
  std::vector<ClipLayerW> layers_;
};

// LPIPS(alex) v0.1, eval mode, spatial = false (lpips_host.py; the reference's src/metrics.py:97-111): the AlexNet
// trunk on gemm()'s exact-f32 path over NHWC fp32 activations, pred and gt as one batch of 2B images, and the per-tap
// heads of lpips.hip.  fp32 only; the config is not read.
class LpipsAlex : public Model {
 public:
  LpipsAlex(const irx_model_config& cfg, int dtype);
  static constexpr int kMinSide = 31;   // below it the second pool has no window left
  size_t workspace_bytes(int B, int H, int W);
  // pred / gt uint8 [B][H][W][3]; lut float[256][3] (lpips_host.input_table); total [B]; layers [B][5] or null
  void score(hipStream_t s, const uint8_t* pred, const uint8_t* gt, int B, int H, int W, const float* lut,
             double* total, double* layers, char* ws, size_t cap);

 private:
  void run(Ctx& c, const uint8_t* pred, const uint8_t* gt, int B, int H, int W, const float* lut, double* total,
           double* layers);
  P cw_[5], cb_[5], lw_[5];
};

// torchvision's InceptionV3 trunk in eval mode up to the 2048 pooled features (fid_host.py; the reference's
// src/metrics.py:70-80, 150-223): every BasicConv2d as a bias-free conv on gemm()'s exact-f32 path followed by
// fid_bn_relu with the host-folded BatchNorm scale / shift; a branch's last unit writes its slice of the block's
// concat buffer.  fp32 only; the config is not read.
class InceptionFid : public Model {
 public:
  InceptionFid(const irx_model_config& cfg, int dtype);
  static constexpr int kMinSide = 75;   // below it Mixed_7a's pool has no window left
  static constexpr int kFeatures = 2048;
  size_t workspace_bytes(int B, int H, int W);
  // x fp32 NHWC4 [B][H][W][4] (channel 3 zero); out fp32 [B][2048]
  void features(hipStream_t s, const float* x, int B, int H, int W, float* out, char* ws, size_t cap);

 private:
  struct Unit { P w, sc, sh; int cin, cout, kh, kw, stride, ph, pw; };
  int unit(const std::string& name, int cin, int cout, int kh, int kw, int stride = 1, int ph = 0, int pw = 0);
  Act cbr(Ctx& c, const Act& x, int& u);                       // the next unit into a new activation
  void cbr_into(Ctx& c, const Act& x, int& u, Act& cat, int off);   // ... into channels [off, off + cout) of cat
  Act avgpool(Ctx& c, const Act& x);
  Act stem_pool(Ctx& c, Act& x);
  void maxpool_into(Ctx& c, const Act& x, Act& cat, int off);
  Act block_a(Ctx& c, Act& x, int& u);
  Act block_b(Ctx& c, Act& x, int& u);
  Act block_c(Ctx& c, Act& x, int& u);
  Act block_d(Ctx& c, Act& x, int& u);
  Act block_e(Ctx& c, Act& x, int& u);
  void run(Ctx& c, const float* x, int B, int H, int W, float* out);
  std::vector<Unit> units_;
};

// Real-ESRGAN's SRVGGNetCompact(3, 3, num_feat=64, num_conv=32, upscale=4, act_type='prelu') (srvgg_host.py; the
// reference's src/inference.py:335-336, :579-591): uint8 RGB in, uint8 RGB x4 out.  fp16 is the product (the fused
// kernels of srvgg.hip, or conv2d + PReLU with srvgg_fused = 0), fp32 the parity engine on gemm()'s exact-f32 path;
// bf16 is refused.  The config is not read.
class Srvgg : public Model {
 public:
  Srvgg(const irx_model_config& cfg, int dtype);
  static constexpr int kConvs = 34, kFeat = 64, kOut = 48;
  size_t workspace_bytes(int B, int H, int W);
  // img uint8 [B][H][W][3]; lut float[256] (srvgg_host.input_table); out_u8 [B][4H][4W][3]; out_f the same shape
  // (the unclamped result, fp32) or null
  void enhance(hipStream_t s, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8,
               float* out_f, char* ws, size_t cap);

 private:
  void run(Ctx& c, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8, float* out_f);
  P cw_[kConvs], cb_[kConvs], sl_[kConvs - 1];
  int cin0_ = 4;
};

// Real-ESRGAN's RRDBNet(3, 3, num_feat=64, num_block, num_grow_ch=32, scale=4) (rrdb_host.py; the network of
// RealESRGAN_x4plus.pth, the file the reference names at src/inference.py:326-350; enhance, :579-591): uint8 RGB in,
// uint8 RGB x4 out.  fp16 is the product (the slab conv kernel of rrdb.hip, or conv2d + glue kernels with rrdb_fused =
// 0), fp32 the parity engine on gemm()'s exact-f32 path; bf16 is refused.  The config gives num_block (num_layers),
// num_feat (hidden_size) and num_grow_ch (intermediate_size).
class Rrdb : public Model {
 public:
  Rrdb(const irx_model_config& cfg, int dtype);
  static constexpr int kFeat = 64, kGrow = 32, kWide = kFeat + 4 * kGrow, kLastPad = 8;
  size_t workspace_bytes(int B, int H, int W);
  void enhance(hipStream_t s, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8,
               float* out_f, char* ws, size_t cap);

 private:
  struct Cv { P w, b; };
  struct Rdb { Cv c[5]; };
  void run(Ctx& c, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8, float* out_f);
  void run_fused(Ctx& c, const uint8_t* img, int B, int H, int W, const float* lut, uint8_t* out_u8, float* out_f);
  // the conv2d graph's form of one rrdb_conv call: gather (unless x is dense), conv2d to an fp32 sum, epilogue
  void conv_glue(Ctx& c, const void* x, int ldx, int cin, int B, int Hs, int Ws, int up, const Cv& cv, int cout,
                 int lrelu, const void* r1, int ldr1, int r1_scaled, const void* r2, int ldr2, void* y, int ldy);
  Cv make(const std::string& name, int co, int ci);
  int nb_ = 0, cin0_ = 4;
  Cv first_, body_, up1_, up2_, hr_, last_;
  std::vector<Rdb> rdb_;   // 3 per RRDB
};

}  // namespace irx
