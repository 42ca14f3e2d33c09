// irx — diffusers' StableDiffusionSafetyChecker as a native model (models.h SafetyChecker; safety_host.py is the
// restatement): what run_safety_checker computes at the end of the reference's img2img calls (src/inference.py:486,
// :566, :664), from the resized and cropped uint8 image to the per-image flag.
//
//   safety_patches -> patch GEMM [B P][Kpad] x [D][Kpad]^T (no bias) -> safety_tokens (+ class, + position) ->
//   pre_layrnorm -> num_layers x Model::clip_layer (no mask) -> post_layernorm of the B token-0 rows ->
//   visual_projection (fp32 out) -> safety_head
// The parameters carry the checkpoint's names (`vision_model.vision_model.*`, `visual_projection.weight`,
// `concept_embeds`, ...); `position_ids` is a buffer of the checkpoint and is not read.  The patch conv's [D][3][p][p]
// weight is packed as a [D][3 p p] matrix zero padded to Kpad columns, the multiple of 64 the large tiles' K loop takes.
#include <algorithm>

#include "models.h"

namespace irx {

SafetyChecker::SafetyChecker(const irx_model_config& cfg, int dtype) : Model(IRX_MODEL_SAFETY, cfg, dtype) {
  const int D = cfg.hidden_size, F = cfg.intermediate_size, S = cfg.image_size, pz = cfg.patch_size;
  IRX_CHECK(D > 0 && F > 0 && cfg.num_layers > 0 && cfg.heads > 0 && D % cfg.heads == 0, "bad safety checker config");
  IRX_CHECK(D % 8 == 0 && F % 8 == 0, "safety checker: hidden and intermediate sizes must be multiples of 8");
  IRX_CHECK(pz > 0 && S >= pz && S % pz == 0, "safety checker: image_size must be a multiple of patch_size");
  IRX_CHECK(cfg.projection_dim > 0 && cfg.projection_dim % 8 == 0 && cfg.projection_dim <= 4096,
            "safety checker: projection_dim must be a multiple of 8, at most 4096");
  IRX_CHECK(cfg.n_special >= 0 && cfg.n_concepts >= 1 && cfg.n_special + cfg.n_concepts <= 64,
            "safety checker: at most 64 embedding rows, one concept at least");
  const int P = (S / pz) * (S / pz), n = cfg.projection_dim;
  kpad_ = (3 * pz * pz + 63) / 64 * 64;
  const std::string p = "vision_model.vision_model.";
  patch_w = mat(p + "embeddings.patch_embedding.weight", D, kpad_);
  cls = vec(p + "embeddings.class_embedding", D);
  pos = reg(p + "embeddings.position_embedding.weight", IRX_LAYOUT_EMB, dt_, {P + 1, D});
  pre_w = vec(p + "pre_layrnorm.weight", D); pre_b = vec(p + "pre_layrnorm.bias", D);
  for (int i = 0; i < cfg.num_layers; ++i)
    layers_.push_back(make_clip_layer(p + "encoder.layers." + std::to_string(i) + ".", D, F));
  post_w = vec(p + "post_layernorm.weight", D); post_b = vec(p + "post_layernorm.bias", D);
  proj_w = mat("visual_projection.weight", n, D);
  sp_e = reg("special_care_embeds", IRX_LAYOUT_MAT, F32, {std::max(cfg.n_special, 1), n});
  co_e = reg("concept_embeds", IRX_LAYOUT_MAT, F32, {cfg.n_concepts, n});
  sp_t = vec("special_care_embeds_weights", std::max(cfg.n_special, 1));
  co_t = vec("concept_embeds_weights", cfg.n_concepts);
}

void SafetyChecker::run(Ctx& c, const uint8_t* crop, int B, const float* lut, float* scores, int* flags,
                        float* embeds) {
  const int D = cfg_.hidden_size, F = cfg_.intermediate_size, H = cfg_.heads, S = cfg_.image_size, pz = cfg_.patch_size;
  const int P = (S / pz) * (S / pz), L = P + 1, n = cfg_.projection_dim;
  const long M = (long)B * L;
  const size_t es = dsize(dt_);
  const float eps = cfg_.layer_norm_eps;
  const bool dry = c.ws->dry();
  void* h = c.ws->alloc(M * D * es);
  ClipScratch t;
  t.n = c.ws->alloc(M * D * es);
  t.qkv = c.ws->alloc(M * 3 * D * es);
  t.att = c.ws->alloc(M * D * es);
  t.f = c.ws->alloc(M * F * es);
  void* rows = c.ws->alloc((size_t)B * P * kpad_ * es);
  void* pout = c.ws->alloc((size_t)B * P * D * es);
  if (!dry) safety_patches(dt_, crop, B, S, pz, kpad_, lut, rows, c.s);
  linear(c, rows, kpad_, B * P, kpad_, patch_w, D, nullptr, pout, D, ACT_NONE, nullptr, 0, 0, B);
  if (!dry) {
    safety_tokens(dt_, pout, fptr(cls), ptr(pos), B, P, D, t.n, c.s);
    layer_norm(dt_, t.n, D, (int)M, D, eps, fptr(pre_w), fptr(pre_b), h, D, c.s);
  }
  c.ws->free(pout);
  c.ws->free(rows);
  for (auto& l : layers_)
    clip_layer(c, l, h, B, L, D, F, H, eps, cfg_.quick_gelu ? ACT_QUICK_GELU : ACT_GELU, 0, B, t);
  // pooled = post_layernorm(token 0 of every image): rows L * D apart
  void* pooled = c.ws->alloc((size_t)B * D * es);
  float* emb = (float*)c.ws->alloc((size_t)B * n * sizeof(float));
  if (!dry) layer_norm(dt_, h, (long)L * D, B, D, eps, fptr(post_w), fptr(post_b), pooled, D, c.s);
  linear(c, pooled, D, B, D, proj_w, n, nullptr, emb, n, ACT_NONE, nullptr, 0, 1);
  if (!dry) {
    if (scores)   // (null: the embeddings alone, irx_safety_embed_u8)
      safety_head(emb, B, n, fptr(sp_e), cfg_.n_special, fptr(co_e), cfg_.n_concepts, fptr(sp_t), fptr(co_t), scores,
                  flags, c.s);
    if (embeds) IRX_HIP(hipMemcpyAsync(embeds, emb, (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, c.s));
  }
  c.ws->free(emb);
  c.ws->free(pooled);
  c.ws->free(t.f);
  c.ws->free(t.att);
  c.ws->free(t.qkv);
  c.ws->free(t.n);
  c.ws->free(h);
}

size_t SafetyChecker::workspace_bytes(int B) {
  IRX_CHECK(B > 0 && B <= kMaxBatch, "safety checker: batch must be in [1, " + std::to_string(kMaxBatch) + "]");
  Arena ar;
  ar.reset(nullptr, 0);
  Ctx c{nullptr, &ar};
  run(c, nullptr, B, nullptr, nullptr, nullptr, nullptr);
  return ar.peak();
}

void SafetyChecker::check(hipStream_t s, const uint8_t* crop, int B, const float* lut, float* scores, int* flags,
                          float* embeds, char* ws, size_t cap) {
  IRX_CHECK(blob_, "weights not bound");
  IRX_CHECK(((uintptr_t)ws % 16) == 0, "workspace must be 16-byte aligned");
  const size_t need = workspace_bytes(B);   // sized before the first launch: a short workspace is refused whole
  IRX_CHECK(cap >= need, "workspace too small: " + std::to_string(cap) + " < " + std::to_string(need));
  Arena ar;
  ar.reset(ws, cap);
  Ctx c{s, &ar};
  run(c, crop, B, lut, scores, flags, embeds);
}

}  // namespace irx
