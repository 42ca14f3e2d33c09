/* irx — MI355X-native Stable Diffusion restoration engine: public C ABI.
 *
 * The reference has no native interface: `src/inference.py` (RestorationPipeline,
 * src/inference.py:48-890) calls diffusers pipelines whose components are the boundary this
 * library replaces.  Each entry point below names the reference-side call it stands in for.
 * Conventions:
 *   - every function returns 0 on success, non-zero on failure; irx_last_error() gives a
 *     thread-local message (reference error behaviour: the Python layer logs it and falls back,
 *     src/inference.py:496-498, :575-577, :679-681, :774-776);
 *   - tensors are raw DEVICE pointers owned by the caller (PyTorch-ROCm tensors used as
 *     containers); the library never allocates or frees caller memory;
 *   - activations are NHWC; `dtype` is IRX_F32 (parity mode), IRX_BF16 or IRX_F16 (throughput modes);
 *   - `stream` is a hipStream_t passed as void*; work is enqueued, nothing synchronises;
 *   - a model handle is not thread-safe; use one handle per stream.
 */
#ifndef IRX_H_
#define IRX_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRX_F32 0
#define IRX_BF16 1
#define IRX_F16 2   /* IEEE half: the reference's own GPU dtype (src/inference.py:57), BASELINE configs[4] */

#define IRX_MODEL_UNET 0
#define IRX_MODEL_VAE 1
#define IRX_MODEL_CLIP 2
#define IRX_MODEL_LPIPS 3   /* LPIPS(alex) v0.1 (src/metrics.py:97-111): fp32 only, the config is not read */
#define IRX_MODEL_FID 4     /* InceptionV3 pooled features (src/metrics.py:70-80): fp32 only, the config is not read */
/* Real-ESRGAN's SRVGGNetCompact(3, 3, 64, 32, upscale 4, prelu) (src/inference.py:335-336): IRX_F16 (the product, the
 * reference's half on a GPU) or IRX_F32 (parity); IRX_BF16 is refused at creation; the config is not read */
#define IRX_MODEL_SRVGG 5
/* diffusers' StableDiffusionSafetyChecker (run_safety_checker at the end of the img2img calls, src/inference.py:486,
 * :566, :664): the CLIP vision tower in the model dtype, the cosine head in fp32.  Reads hidden_size, intermediate_size,
 * num_layers, heads, layer_norm_eps, quick_gelu and the five safety fields at the end of irx_model_config */
#define IRX_MODEL_SAFETY 6
/* Real-ESRGAN's RRDBNet(3, 3, num_feat=64, num_block, num_grow_ch=32, scale=4), the network RealESRGAN_x4plus.pth
 * belongs to (the file src/inference.py:326-350 names): IRX_F16 (the product) or IRX_F32 (parity); IRX_BF16 is refused
 * at creation.  Reads three existing fields of irx_model_config, so the struct does not grow: num_layers = num_block
 * (1..64), hidden_size = num_feat and intermediate_size = num_grow_ch (the kernels are built for 64 and 32; any other
 * value is refused at creation) */
#define IRX_MODEL_RRDB 7

/* weight layouts of manifest entries (how the host packs diffusers tensors into the blob) */
#define IRX_LAYOUT_VEC 0   /* [n] fp32, zero padded                                  */
#define IRX_LAYOUT_MAT 1   /* [N][K] from [N][K] or [N][K][1][1], zero padded         */
#define IRX_LAYOUT_CONV 2  /* [Cout][KH][KW][Cin] from OIHW, zero padded on Cout/Cin   */
#define IRX_LAYOUT_EMB 3   /* [rows][D] embedding table                                */
/* GEGLU projection (diffusers ff.net.0.proj, rows [values; gates]) re-ordered into (64 value rows,
 * 64 gate rows) block pairs: packed row r <- source row (r/128)*64 + r%64 (+ N/2 if r%128 >= 64) */
#define IRX_LAYOUT_MAT_GEGLU64 4
#define IRX_LAYOUT_VEC_GEGLU64 5
/* LayerNorm folded into the projection it feeds (16-bit UNets; diffusers BasicTransformerBlock norm1/2/3 ->
 * attn1.to_q|k|v, attn2.to_q, ff.net.0.proj).  The matrix entry names its LN weight in `aux`: the packer scales
 * its columns by gamma (after any re-ordering / row scaling, before the cast).  Two fp32 vectors follow it,
 * named after the same matrix spec:
 *   VEC_LN_U  u[n] = sum_k of the packed (cast) matrix row n
 *   VEC_LN_V  v[n] = bias[n] + sum_k W[n][k] * beta[k]  (W re-ordered / row-scaled as packed, before gamma);
 *             aux = "<beta name>;<bias spec or empty>" */
#define IRX_LAYOUT_VEC_LN_U 6
#define IRX_LAYOUT_VEC_LN_V 7
/* Two linear layers with nothing between them folded into one (16-bit UNets: a Transformer2DModel's ff.net.2 ->
 * proj_out, the residual add between them distributing over proj_out): name "<A>|<B>" with A [N][C] the second
 * layer (proj_out.weight) and B [C][K] the first (ff.net.2.weight):
 *   MAT_CHAIN  [N][C + K] = [A | A B]   (product in fp64, then the cast): proj_out(h + ff2(g)) = [A | AB] [h; g] + ...
 *   VEC_CHAIN  [N] = a + A b, aux = "<a name>;<b name>" (the biases: proj_out.bias; ff.net.2.bias) */
#define IRX_LAYOUT_MAT_CHAIN 8
#define IRX_LAYOUT_VEC_CHAIN 9
/* A nearest-2x upsampler's 3x3 conv (diffusers Upsample2D: interpolate(scale 2, nearest) -> conv 3x3 pad 1) folded per
 * output parity (16-bit engines): output pixel (2y + a, 2x + b) only sees low-resolution rows y - 1 + a .. y + a and
 * columns x - 1 + b .. x + b, so each parity p = 2a + b is a 2x2 conv of the low-resolution input.  [4][Cout][2][2][Cin]
 * (as [4 Cout][2][2][Cin]) from OIHW: tap (i, j) of parity (a, b) = sum of the original taps ky in R(a, i), kx in
 * R(b, j), R(0, 0) = {0}, R(0, 1) = {1, 2}, R(1, 0) = {0, 1}, R(1, 1) = {2} (sums in fp64, then the cast).  4 / 9 of
 * the upsampled conv's MACs. */
#define IRX_LAYOUT_CONV_UP2 10

typedef struct irx_model irx_model;

typedef struct {
  /* UNet2DConditionModel (unet/config.json) / AutoencoderKL (vae/config.json) */
  int in_channels, out_channels, latent_channels;
  int n_blocks;
  int block_out_channels[8];
  int layers_per_block;
  int heads;                /* UNet: "attention_head_dim" (= head count in SD-1.5) */
  int cross_attention_dim;
  int norm_groups;
  float norm_eps;
  int flip_sin_to_cos;
  float freq_shift;
  int down_attn[8], up_attn[8];
  /* CLIPTextModel (text_encoder/config.json) */
  int vocab_size, hidden_size, intermediate_size, num_layers, max_positions;
  float layer_norm_eps;
  int quick_gelu;
  /* StableDiffusionSafetyChecker (safety_checker/config.json "vision_config", "projection_dim"; the rows of
     special_care_embeds / concept_embeds); the tower reuses hidden_size .. quick_gelu above */
  int image_size, patch_size, projection_dim, n_special, n_concepts;
} irx_model_config;

typedef struct {
  const char* name;   /* diffusers/transformers parameter name(s); '|' joins tensors concatenated on dim 0 */
  int layout;         /* IRX_LAYOUT_* */
  int dtype;          /* IRX_F32 or IRX_BF16 storage in the blob */
  int ndim;
  int64_t shape[4];   /* engine shape (padded) */
  size_t offset;      /* byte offset in the weight blob */
  size_t bytes;
  /* the packer multiplies rows [0, scale_rows) by row_scale (in fp32, before the cast): the attention
   * softmax scale * log2(e) folded into to_q in the 16-bit engines (the kernels then take q pre-scaled) */
  float row_scale;
  int64_t scale_rows;
  const char* aux;    /* IRX_LAYOUT_MAT*: column-scale vector name ("" = none); VEC_LN_V: "<beta>;<bias>" */
} irx_param_info;

const char* irx_last_error(void);
int irx_version(void);

/* engine options: "large_tiles" (1 = 8-wave LDS-DMA GEMM/conv path where eligible, 0 = 4-wave kernel) */
int irx_set_option(const char* name, int value);
int irx_get_option(const char* name, int* value);   /* current value of a runtime option (tests save / restore) */
const char* irx_option_name(int i);                 /* i-th option name, NULL past the last */

/* ---- optional per-launch HIP-event timing of the MFMA kernels (bench.py roofline) ---- */
int irx_profile_begin(void);
int irx_profile_end(int* n_kernels);   /* synchronises, aggregates per kernel instantiation */
int irx_profile_get(int i, const char** name, long* launches, double* total_ms, double* total_flops);

/* ---- HIP-graph capture of a launch sequence (the denoising loop: every UNet eval + fused step kernel).
   begin/end bracket ordinary irx calls on `stream` (a non-default stream; the calls are recorded, not run);
   end instantiates an executable graph, launch replays it on a stream, destroy frees it.  Buffers, shapes
   and scalar arguments are baked in at capture: replay re-runs exactly the recorded launches. ---- */
typedef struct irx_graph irx_graph;
int irx_graph_begin(void* stream);
int irx_graph_end(void* stream, irx_graph** out);
int irx_graph_launch(irx_graph* g, void* stream);
int irx_graph_destroy(irx_graph* g);

/* ---- model lifetime: replaces diffusers/transformers from_pretrained (src/inference.py:162-172) ---- */
int irx_model_create(int kind, const irx_model_config* cfg, int dtype, irx_model** out);
int irx_model_destroy(irx_model* m);
int irx_model_num_params(const irx_model* m, int* n);
int irx_model_param_info(const irx_model* m, int i, irx_param_info* info);
int irx_model_blob_bytes(const irx_model* m, size_t* bytes);
/* bind a device blob packed per the manifest (after upload or RCCL broadcast) */
int irx_model_bind(irx_model* m, void* device_blob, size_t bytes);

/* ---- UNet2DConditionModel.forward (diffusers; called per step at src/inference.py:486/:566/:664/:758) ---- */
int irx_unet_workspace_bytes(const irx_model* m, int batch, int h, int w, size_t* bytes);
int irx_unet_context_bytes(const irx_model* m, int batch, int ctx_len, size_t* bytes);
/* cross-attention K/V of all transformer blocks for a fixed text context (computed once per call) */
int irx_unet_prepare_context(irx_model* m, void* stream, const void* ctx, int batch, int ctx_len, void* ctx_kv,
                             void* ws, size_t ws_bytes);
/* x: [batch][h][w][cin_pad] dtype; t: device fp32 [batch]; eps_out: fp32 [batch][h][w][out_channels] */
int irx_unet_forward(irx_model* m, void* stream, const void* x, int batch, int h, int w, const float* t,
                     const void* ctx_kv, int ctx_len, float* eps_out, void* ws, size_t ws_bytes);
int irx_unet_input_channels(const irx_model* m, int* cin_pad);
/* Extended forward.  opts->cfg_share != 0 is the caller's promise that rows b and b + batch / 2 of x and t are
   identical — the [uncond x B, cond x B] batch of classifier-free guidance, whose halves differ only in ctx_kv.  The
   16-bit engines then run everything up to the first cross-attention (down_blocks.0.resnets.0 and its transformer up
   to attn2.to_q) on batch / 2 images; eps_out is bit-identical to irx_unet_forward on the same batch.  batch must be
   even; the fp32 engine ignores the promise.
   opts->time_proj != NULL: one row of irx_unet_time_table for the timestep every image of this batch is at; the
   time-embedding chain is skipped and t is not read (may be NULL).  Give the workspace query the same opts.
   opts == NULL or all zero: irx_unet_forward / irx_unet_workspace_bytes. */
typedef struct irx_unet_opts {
  int cfg_share;
  const float* time_proj;   /* device fp32 [irx_unet_time_table row], 16-byte aligned */
} irx_unet_opts;
int irx_unet_workspace_bytes_ex(const irx_model* m, int batch, int h, int w, const irx_unet_opts* opts, size_t* bytes);
int irx_unet_forward_ex(irx_model* m, void* stream, const void* x, int batch, int h, int w, const float* t,
                        const void* ctx_kv, int ctx_len, float* eps_out, const irx_unet_opts* opts, void* ws,
                        size_t ws_bytes);

/* The time-embedding chain (sinusoid -> linear_1 -> SiLU -> linear_2 -> SiLU -> every resnet's time_emb_proj) for
   the n timesteps of a whole schedule at once, n <= 256: t device fp32 [n] -> table fp32 [n][table_bytes / (4 n)],
   row i bit-identical to what irx_unet_forward computes for an image at t[i].  The weights are streamed once per
   loop instead of once per evaluation. */
int irx_unet_time_table_bytes(const irx_model* m, int n, size_t* table_bytes, size_t* ws_bytes);
int irx_unet_time_table(irx_model* m, void* stream, const float* t, int n, float* table, void* ws, size_t ws_bytes);

/* ---- AutoencoderKL.encode / .decode (diffusers; img2img prepare_latents / final decode) ---- */
int irx_vae_encode_workspace_bytes(const irx_model* m, int batch, int H, int W, size_t* bytes);
/* img: [batch][H][W][8] dtype in [-1,1]; moments: [batch][H/8][W/8][8] dtype (mean 0..3, logvar 4..7) */
int irx_vae_encode(irx_model* m, void* stream, const void* img, int batch, int H, int W, void* moments, void* ws,
                   size_t ws_bytes);
int irx_vae_decode_workspace_bytes(const irx_model* m, int batch, int h, int w, size_t* bytes);
/* z: [batch][h][w][8] dtype (latents / scaling_factor, channels 4..7 zero); out: [batch][8h][8w][4] dtype */
int irx_vae_decode(irx_model* m, void* stream, const void* z, int batch, int h, int w, void* out, void* ws,
                   size_t ws_bytes);

/* ---- CLIPTextModel.last_hidden_state (transformers; encode_prompt) ---- */
int irx_clip_workspace_bytes(const irx_model* m, int batch, int len, size_t* bytes);
/* ids: device int32 [batch][len]; out: [batch][len][hidden] dtype */
int irx_clip_encode(irx_model* m, void* stream, const int* ids, int batch, int len, void* out, void* ws,
                    size_t ws_bytes);

/* ---- scheduler / pipeline glue (PNDMScheduler.step_plms, DDIMScheduler.step, CFG combine, add_noise,
 *      DiagonalGaussianDistribution.sample, VaeImageProcessor pre/post) ---- */
typedef struct {
  int dtype;
  int batch, h, w;
  const float* eps; int cfg; float guidance;
  float* hist_store; const float* hist[4]; float hw[5]; float e_div; float e_mul;
  int mode; float c0, c1, c2, c3;
  const float* x_src; float* cur_store; float* x_out;
  void* unet_in; int cin_pad; int inpaint; const float* mask; const float* masked;
} irx_step_params;
int irx_sched_step(void* stream, const irx_step_params* p);
int irx_pack_unet_input(void* stream, int dtype, const float* lat, int batch, int h, int w, int cfg, int cin_pad,
                        int inpaint, const float* mask, const float* masked, void* out);
int irx_latent_sample(void* stream, int dtype, const void* moments, int batch, int h, int w, const float* eps,
                      const float* noise, int bcast, float scaling_factor, float a, float b, float* out);
int irx_latents_to_vae(void* stream, int dtype, const float* lat, int batch, int h, int w, float scaling_factor,
                       void* z);
/* mask (nullable): fp32 [batch][H][W], 1 = region to inpaint; masked pixels become 0 (init_image * (mask < 0.5)) */
int irx_image_to_tensor(void* stream, int dtype, const uint8_t* img, const float* mask, int batch, int H, int W,
                        int cpad, void* out);
int irx_tensor_to_image(void* stream, int dtype, const void* x, int batch, int H, int W, int ldc, uint8_t* img,
                        float* f01);

/* ---- synthetic degradations (scripts/make_synthetic_pairs.py) ----
 * uint8 HWC batches in device memory, one pass each, no allocation. */
/* add_gaussian_noise (make_synthetic_pairs.py:29-35): out = uint8(clip(f32(img) + f32(z) * sigma, 0, 255));
 * z = `noise` (n floats, e.g. numpy's randn draws) or, if null, Philox4x32-10 normals keyed by `seed` */
int irx_degrade_noise(void* stream, const uint8_t* img, long n, float sigma, const float* noise,
                      unsigned long long seed, uint8_t* out);
/* degrade_sr (:67-81): cv2.GaussianBlur(k, sigma 0) with k = ksize[b] in {3,5,7} (device int[batch]) into
 * `blur` [batch][H][W][C]; if `lr`, cv2.resize(INTER_CUBIC) to [batch][H/scale][W/scale][C] */
int irx_degrade_blur_down(void* stream, const uint8_t* img, int batch, int H, int W, int C, const int* ksize,
                          int scale, uint8_t* blur, uint8_t* lr);
/* to_grayscale (:84-90): mode 0 = cv2 BGR2GRAY, 1 = L of cv2 BGR2Lab; rgb != 0: input channel order R,G,B */
int irx_degrade_gray(void* stream, const uint8_t* img, long npix, int mode, int rgb, uint8_t* out);
/* random_free_form_mask (:104-114) + masked input (:196-198): segs int[nseg][4] (x0,y0,x1,y1), thick int[nseg],
 * seg_off int[batch+1]; mask [batch][H][W] = 255 inside any stroke; img/masked (nullable) [batch][H][W][3] */
int irx_degrade_strokes(void* stream, int batch, int H, int W, const int* segs, const int* thick, const int* seg_off,
                        uint8_t* mask, const uint8_t* img, uint8_t* masked);
/* add_motion_blur (:46-64): cv2.filter2D(img, -1, kernel) for the line kernel whose non-zero cells (all 1/n) are
 * image b's taps[tap_off[b] .. tap_off[b+1]) (int[ntap][2] = (dy, dx) from the centre, raster order; tap_off
 * int[batch+1]; both device memory).  BORDER_REFLECT_101, fp32 accumulation in tap order, rint.  img/out
 * [batch][H][W][C], C = 1 or 3; H, W >= 8 */
int irx_degrade_motion_blur(void* stream, const uint8_t* img, int batch, int H, int W, int C, const int* taps,
                            const int* tap_off, uint8_t* out);
/* add_jpeg_compression (:38-43): the decoded pixels of cv2.imencode('.jpg') -> cv2.imdecode for a baseline 4:2:0
 * JPEG with image b's quantisation tables qtables[b][2][64] (device int; luma, chroma; natural order, 1..255):
 * libjpeg's integer chain without the (lossless) entropy coder.  img/out [batch][H][W][3], rgb != 0: channel
 * order R,G,B; H, W >= 8.  ws: irx_degrade_jpeg_ws_bytes(batch, H, W) bytes of device memory, 8-byte aligned
 * (0 is returned for arguments irx_degrade_jpeg would refuse) */
long irx_degrade_jpeg_ws_bytes(int batch, int H, int W);
int irx_degrade_jpeg(void* stream, const uint8_t* img, int batch, int H, int W, const int* qtables, int rgb,
                     void* ws, uint8_t* out);

/* ---- baseline JPEG encoder (PIL.Image.save(path) on a .jpg name, scripts/generate_predictions.py:83-84: the file
 * Pillow + libjpeg-turbo writes for an RGB image at a quality, byte for byte: baseline sequential, 4:2:0, the
 * Annex K Huffman tables, no restart markers).  A file is irx_jpeg_header's bytes, the scan, FF D9. ---- */
/* Device memory irx_jpeg_encode needs as ws (16-byte aligned), and the capacity in bytes it needs per image in
 * out: 2 * (6 * MCUs * 208) + 2, from 1660 bits per 8x8 block at most (22 of DC, 63 x 26 of AC) and one stuffed
 * 0x00 per byte at worst.  0 is returned for arguments irx_jpeg_encode would refuse. */
long irx_jpeg_encode_ws_bytes(int batch, int H, int W);
long irx_jpeg_encode_bound(int H, int W);
/* The entropy-coded scan of every image of img [batch][H][W][3] (device uint8; rgb != 0: R,G,B order, else B,G,R)
 * under image b's tables qtables[b][2][64] (device int; luma, chroma; natural order, 1..255).  8 <= H, W <= 65535.
 * Image b's scan goes to out + b * out_stride (device; out_stride >= irx_jpeg_encode_bound(H, W)), its length to
 * lens[b] (device int); exactly lens[b] bytes of image b are written and nothing else in out.  ws may hold
 * anything on entry. */
int irx_jpeg_encode(void* stream, const uint8_t* img, int batch, int H, int W, const int* qtables, int rgb, void* ws,
                    uint8_t* out, long out_stride, int* lens);
/* Host only: the bytes in front of the scan (SOI, APP0, DQT x 2, SOF0, DHT x 4, SOS; 623 of them) for an H x W
 * image and the host tables qtables[2][64] (natural order).  Returns the length written to buf (capacity cap), or
 * a negative status with irx_last_error set. */
int irx_jpeg_header(int H, int W, const int* qtables, uint8_t* buf, int cap);

/* ---- baseline JPEG decoder (PIL.Image.open(path).convert("RGB"), src/metrics.py:40-46 load_image and
 * scripts/generate_predictions.py:68: the pixels Pillow + libjpeg-turbo decode, bit for bit).  The contract is the
 * kind of file PIL.save and cv2.imwrite write by default: baseline SOF0, 8 bit, one scan, no restart interval, JFIF,
 * either 4:2:0 with sampling (2,2)(1,1)(1,1) or one component.  Everything else is refused by the parser and stays
 * with PIL. ---- */
/* What irx_jpeg_parse reads out of a file (plain data, no pointers). */
typedef struct irx_jpeg_info {
  int H, W;                    /* 8 .. 65535 */
  int ncomp;                   /* 1 (grayscale) or 3 (Y, Cb, Cr at 4:2:0) */
  int qsel[3], dcsel[3], acsel[3]; /* per component: quantisation, DC and AC Huffman table, each 0 or 1 */
  uint16_t qt[2][64];          /* quantisation tables, natural (row-major) order; 0: the file defines none */
  uint8_t dc_bits[2][16];      /* DC tables: codes per length 1..16, then the symbols in code order */
  uint8_t dc_vals[2][16];
  uint8_t ac_bits[2][16];      /* AC tables likewise */
  uint8_t ac_vals[2][256];
  int dc_count[2], ac_count[2]; /* symbols per table; 0: the file defines none */
  long scan_off, scan_len;     /* the entropy-coded bytes: file[scan_off .. scan_off + scan_len), up to the first
                                  FF xx with xx != 00 (which is the EOI marker) */
} irx_jpeg_info;
/* irx_jpeg_parse's refusals; each sets irx_last_error */
#define IRX_JPEG_TRUNCATED (-1)   /* the file ends inside the header or a segment */
#define IRX_JPEG_NOT_JPEG (-2)    /* empty, or no SOI */
#define IRX_JPEG_SOF (-3)         /* SOF1, SOF2, ...: extended, progressive, lossless or arithmetic coding */
#define IRX_JPEG_PRECISION (-4)   /* sample precision other than 8 bits */
#define IRX_JPEG_DQT16 (-5)       /* 16-bit quantisation table */
#define IRX_JPEG_SAMPLING (-6)    /* three components sampled other than (2,2)(1,1)(1,1) */
#define IRX_JPEG_MULTISCAN (-7)   /* a scan without every component, or data after the scan other than EOI */
#define IRX_JPEG_DRI (-8)         /* a non-zero restart interval, or a restart marker in the scan */
#define IRX_JPEG_ADOBE (-9)       /* Adobe APP14 marker (a colour transform PIL honours) */
#define IRX_JPEG_RGB_IDS (-10)    /* component ids 'R','G','B' (libjpeg takes the file for RGB) */
#define IRX_JPEG_COMPONENTS (-11) /* CMYK / YCCK, or a component count other than 1 or 3 */
#define IRX_JPEG_SIZE (-12)       /* H or W below 8 (the inverse half's minimum, as irx_degrade_jpeg) */
#define IRX_JPEG_TABLES (-13)     /* a table id above 1, a table that is named but not defined, DC category > 11,
                                     AC size > 10 */
#define IRX_JPEG_SCAN_CUT (-14)   /* the file ends inside the scan */
#define IRX_JPEG_MALFORMED (-15)  /* anything else that is not a well-formed file */
/* Host only.  Walks the markers of file[0 .. len) and fills *info; APPn and COM are skipped, the Huffman tables are
 * the file's own.  Returns 0, or one of the statuses above.  Never reads past len. */
int irx_jpeg_parse(const uint8_t* file, long len, irx_jpeg_info* info);
/* Device memory irx_jpeg_decode needs as ws (16-byte aligned) for these files (host infos) at this subseq_bits;
 * 0 for arguments irx_jpeg_decode would refuse. */
long irx_jpeg_decode_ws_bytes(const irx_jpeg_info* infos, int batch, int subseq_bits);
/* Decodes a batch of parsed files.  scans (device): the entropy-coded bytes of every file, image b's at
 * scans + scan_off[b], infos[b].scan_len of them (infos[b].scan_off is not used); scan_off, infos, out_off and
 * coef_off are host arrays of `batch` entries.  subseq_bits: the bits of the stream one lane of the
 * self-synchronising Huffman decoder owns, a multiple of 32, 32 .. 65536; 0: the default (1024).  rgb != 0: every
 * image is written as uint8 [H][W][3] R,G,B (a one-component file replicated to three channels); rgb == 0: every
 * file must have one component and is written as [H][W].  Image b goes to out + out_off[b] (device); exactly its
 * H * W * C bytes are written and nothing else in out.  status[b] (device int) != 0: the stream of image b is not a
 * valid scan of its frame (bit 0: an unassigned code or a run past coefficient 63 on the decoded path; bit 1: too few
 * or too many blocks, or a symbol that runs past the end), or (bit 2) a block's coefficients are so large that
 * libjpeg's C and SIMD IDCTs disagree; its pixels are unspecified but inside its H * W * C bytes, the other images
 * are unaffected.  rounds[b] (device int): the most rounds any pass of the
 * entry-state kernel took.  coef (device, may be NULL): image b's quantised coefficients as int16 [block][64] in
 * zigzag order at coef + coef_off[b] (in elements; blocks in scan order).  ws may hold anything on entry.  An info
 * that irx_jpeg_parse did not fill is checked like the parser checks a file (sizes, selectors, and that every Huffman
 * table has as many symbols as its code counts say and is not over-subscribed) and refused otherwise. */
int irx_jpeg_decode(void* stream, const uint8_t* scans, const long* scan_off, const irx_jpeg_info* infos, int batch,
                    int subseq_bits, int rgb, void* ws, uint8_t* out, const long* out_off, int* status, int* rounds,
                    int16_t* coef, const long* coef_off);

/* ---- fast non-local means (cv2.fastNlMeansDenoising / ...Colored as src/inference.py:509-515 calls them in the
 * classical denoise fallback _denoise_opencv :500-522).  OpenCV's integer invoker, exact. ---- */
/* Host only: the invoker's weight table (almost_dist2weight) for filter strength h over `cn`-channel groups,
 * truncated at its first zero; writes *lut_len and, if `lut`, the entries (cap = capacity of lut). */
int irx_nlm_weights(float h, int cn, int template_size, int search_size, int* lut, int cap, int* lut_len);
/* Denoise one channel group (cn = 1 or 2 channels starting at ch_off) of uint8 [batch][H][W][pix_stride] images
 * from src into the same channels of dst (src != dst); lut = device copy of irx_nlm_weights' table.
 * (template, search) in {(7, 21), (3, 5)}. */
int irx_nlmeans_u8(void* stream, const uint8_t* src, uint8_t* dst, int batch, int H, int W, int pix_stride,
                   int ch_off, int cn, int template_size, int search_size, const int* lut, int lut_len);

/* ---- the filters after the NLM pass in _denoise_opencv (src/inference.py:517-520) ---- */
/* Host only: cv2.bilateralFilter's tables (BilateralFilter_8u): color_w[256*cn] = f32(exp(-i^2 / 2sc^2)), and for
 * the circular window (row-major, sqrt(i^2+j^2) <= radius) space_w[k] = f32(exp(-r^2 / 2ss^2)), space_dydx[2k] =
 * (i, j).  Null table pointers: sizes only.  Writes *maxk and *radius. */
int irx_bilateral_tables(int d, double sigma_color, double sigma_space, int cn, float* color_w, float* space_w,
                         int* space_dydx, int cap, int* maxk, int* radius);
/* cv2.bilateralFilter(img, d = 9, ...) on uint8 [batch][H][W][3] (src != dst), tables in device memory. */
int irx_bilateral_u8(void* stream, const uint8_t* src, uint8_t* dst, int batch, int H, int W, int radius,
                     const float* space_w, const int* space_dydx, int maxk, const float* color_w);
/* The colour conversions of cv2.fastNlMeansDenoisingColored (denoising.cpp): direction 0 = COLOR_LBGR2Lab,
 * 1 = COLOR_Lab2LBGR, 8-bit, `npix` packed 3-byte pixels (in place allowed); fp64, see classical.rgb_to_lab_u8. */
int irx_lab_convert_u8(void* stream, const uint8_t* src, uint8_t* dst, long npix, int direction);
/* _auto_mask_from_image (src/inference.py:805-840) for uint8 RGB [batch][H][W][3]: mask [batch][H][W] (255 = damaged)
 * after MORPH_CLOSE + MORPH_OPEN (5x5), counts[batch] = its non-zero pixels (device int); tmp = [batch][H][W]
 * scratch.  The caller applies the reference's 1 % rule. */
int irx_auto_mask_u8(void* stream, const uint8_t* img, int batch, int H, int W, uint8_t* mask, uint8_t* tmp,
                     int* counts);
/* _colorize_lab (src/inference.py:683-703) for `npix` RGB pixels: L of RGB2LAB (sRGB) via lin_lut[256] (device
 * doubles, the sRGB linearisation of each byte value), then out = color_map[L] (device uint8 [256][3]). */
int irx_colorize_lab_u8(void* stream, const uint8_t* img, long npix, const double* lin_lut, const uint8_t* color_map,
                        uint8_t* out);
/* cv2.medianBlur(img, 5) on uint8 [batch][H][W][C], C <= 4 (src != dst). */
int irx_median_blur_u8(void* stream, const uint8_t* src, uint8_t* dst, int batch, int H, int W, int C, int ksize);

/* ---- PIL `Image.resize(size, LANCZOS | BICUBIC)` on 8-bit images, byte for byte (Pillow's ImagingResample): the
 * LANCZOS fallback of super-resolution (src/inference.py:593-596), the SR area cap (:552-559), the mask resize of
 * _normalize_mask (:790-801) and the VaeImageProcessor resize of the img2img / inpaint preprocess (SURVEY.md A.1 /
 * A.2: to a multiple of 8, to 512x512, the inpaint mask as "L").  `box` / `reducing_gap` and modes with alpha
 * (premultiplied by Pillow) are not covered. ---- */
#define IRX_RESAMPLE_LANCZOS 0
#define IRX_RESAMPLE_BICUBIC 1
#define IRX_RESAMPLE_MAX_KSIZE 97   /* per axis, what irx_resample_u8 accepts: LANCZOS down to 1/16 */
/* Host only: one axis' tables for in_size -> out_size.  bounds[out_size][2] = (first source index, taps n),
 * coeffs[out_size][ksize] = the 22-bit fixed-point weights (entries from n on are 0); cap = capacity of `coeffs`
 * in ints.  Null table pointers: sizes only.  Writes *ksize (any ratio; the kernel's limit is checked there). */
int irx_resample_coeffs(int in_size, int out_size, int filter, int* bounds, int* coeffs, int cap, int* ksize);
/* uint8 [batch][H][W][C] -> [batch][h][w][C], C = 1 or 3, src != dst; the tables are device copies of
 * irx_resample_coeffs' (x: W -> w, y: H -> h).  Horizontal pass first, its result rounded to uint8 as Pillow's
 * temporary image, then the vertical pass; null x tables with W == w skip the horizontal pass, null y tables with
 * H == h the vertical one (both: a copy).  One fused kernel, no allocation.  xk or yk above
 * IRX_RESAMPLE_MAX_KSIZE: a status, nothing launched. */
int irx_resample_u8(void* stream, const uint8_t* src, int batch, int H, int W, int C, const int* xbounds,
                    const int* xcoeffs, int xk, const int* ybounds, const int* ycoeffs, int yk, int h, int w,
                    uint8_t* dst);

/* ---- evaluation metrics on uint8 pairs (src/metrics.py; `evaluate_task`, scripts/evaluate_model.py) ----
 * pred / gt [batch][H][W][C] in device memory, C = 1 or 3, H, W >= 7.  Per image:
 *   sse[b]     = sum (gt - pred)^2 over pixels and channels, exact: skimage's peak_signal_noise_ratio is
 *                10 log10(255^2 / (sse / (H W C))) (calculate_psnr, src/metrics.py:82-87);
 *   ssim[b]    = skimage structural_similarity(gt, pred, data_range=255, channel_axis=2) with its defaults (7x7
 *                uniform window, sample covariance, K1 0.01, K2 0.03, crop 3): calculate_ssim, src/metrics.py:89-95.
 *                Window sums are exact integers, S and its sum fp64;
 *   delta_e[b] = mean dE76 of skimage rgb2lab (calculate_delta_e, src/metrics.py:113-148), C = 3 only, when delta_e
 *                is not NULL; srgb_lut = device float[256], the float32 sRGB linearisation of v / 255 for every byte
 *                value (what rgb2lab computes in float32); the rest is fp64.
 * The fp64 sums are added in a fixed order (block partials in ws, then a fixed tree; no atomics): bit-identical from
 * run to run, for every position in the batch and every batch size.  Two launches, no allocation, no synchronisation.
 * ws: irx_metrics_ws_bytes(batch, H, W, C) bytes of device memory, 8-byte aligned (0 is returned for arguments
 * irx_metrics_pair_u8 would refuse).  A refused argument (null pointer, batch <= 0, C not 1 or 3, H or W < 7, delta_e
 * with C = 1, null ws) is a status and launches nothing. */
long irx_metrics_ws_bytes(int batch, int H, int W, int C);
int irx_metrics_pair_u8(void* stream, const uint8_t* pred, const uint8_t* gt, int batch, int H, int W, int C,
                        const float* srgb_lut, void* ws, long long* sse, double* ssim, double* delta_e);
/* cv2.resize(img, (w, h)) with INTER_LINEAR for uint8, the shape match in front of every metric
 * (src/metrics.py:84-86): [batch][H][W][C] -> [batch][h][w][C], C = 1 or 3, src != dst.  xtab int[w][3], ytab
 * int[h][3] (device) = (i0, i1, w1) per output index: the two source indices and the 11-bit weight of the second
 * (w0 = 2048 - w1); out = clip8((sum + 2^21) >> 22).  Integer, exact. */
int irx_resize_linear_u8(void* stream, const uint8_t* src, int batch, int H, int W, int C, const int* xtab,
                         const int* ytab, int h, int w, uint8_t* dst);

/* ---- LPIPS(alex) (MetricsCalculator.calculate_lpips, src/metrics.py:97-111; image_to_tensor, :49-55) ----
 * lpips.LPIPS(net='alex') v0.1 in eval mode, spatial=False, on uint8 RGB pairs: m is an IRX_MODEL_LPIPS model whose
 * blob holds torchvision's AlexNet `features.{0,3,6,8,10}.{weight,bias}` and the lpips package's
 * `lin{0..4}.model.1.weight`.  pred / gt [batch][H][W][3] in device memory, H, W >= 31.  in_lut = device
 * float[256][3]: the scaling layer's output for byte value v in channel c, (float32(v) / 255 * 2 - 1 - shift[c]) /
 * scale[c] in float32 (lpips_host.input_table).  total[b] = the score, layers[b][k] (NULL: not wanted) = the five
 * taps' terms; total is their sum in index order.  The trunk runs in exact fp32 (MFMA), the per-pixel head terms are
 * added in fp64 in a fixed order (block partials, a fixed tree, no atomics): the same bits on every run.
 * ws: irx_lpips_workspace_bytes(m, batch, H, W) bytes of device memory, 16-byte aligned.  A refused argument (null
 * pointer, batch <= 0, H or W < 31, a model of another kind or without a bound blob, a short workspace) is a status
 * and launches nothing.  Enqueues on `stream`: no allocation, no synchronisation. */
int irx_lpips_workspace_bytes(const irx_model* m, int batch, int H, int W, size_t* bytes);
int irx_lpips_u8(irx_model* m, void* stream, const uint8_t* pred, const uint8_t* gt, int batch, int H, int W,
                 const float* in_lut, double* total, double* layers, void* ws, size_t ws_bytes);
/* the two data-movement kernels of the LPIPS trunk on their own (tests): the input conversion of irx_lpips_u8 into
 * out fp32 [2 batch][H][W][4] (pred images first, channel 3 zero), and ReLU followed by a win x win / stride max pool
 * without padding, (win, stride) = (3, 2) or (1, 1), over fp32 NHWC x [n][H][W][C], C % 4 == 0, into
 * out [n][(H - win) / stride + 1][(W - win) / stride + 1][C] */
int irx_op_lpips_input(void* stream, const uint8_t* pred, const uint8_t* gt, int batch, int H, int W,
                       const float* in_lut, float* out);
int irx_op_lpips_relu_pool(void* stream, const float* x, int n, int H, int W, int C, int win, int stride, float* out);

/* ---- FID features (MetricsCalculator.get_inception_features / calculate_fid, src/metrics.py:150-223; the model and
 * its transform, :70-80) ----
 * torchvision's inception_v3(transform_input=False) in eval mode with fc = Identity: m is an IRX_MODEL_FID model whose
 * blob holds every trunk unit's `<unit>.conv.weight` and the BatchNorm of the unit folded on the host into
 * `<unit>.bn.scale` = gamma / sqrt(var + 1e-3) and `<unit>.bn.shift` = beta - mean * scale (fid_host.fold_bn, fp64,
 * stored fp32).  x fp32 NHWC [batch][H][W][4] in device memory, channel 3 zero, H, W >= 75 (the metric feeds 299 x 299
 * from irx_op_fid_input); out fp32 [batch][2048].  The convolutions run in exact fp32 (MFMA); no atomics anywhere: the
 * same bits on every run, and an image's features do not depend on its position in the batch or on the batch size.
 * ws: irx_fid_workspace_bytes(m, batch, H, W) bytes, 16-byte aligned.  A refused argument (null pointer, batch <= 0, a
 * side below 75, a model of another kind or without a bound blob, a short workspace) is a status and launches nothing.
 * Enqueues on `stream`: no allocation, no synchronisation. */
int irx_fid_workspace_bytes(const irx_model* m, int batch, int H, int W, size_t* bytes);
int irx_fid_features(irx_model* m, void* stream, const float* x, int batch, int H, int W, float* out, void* ws,
                     size_t ws_bytes);
/* The trunk's glue kernels on their own (tests).
 * irx_op_fid_input: ToTensor, transforms.Resize((299, 299)) on the tensor (bilinear, antialias) and Normalize of
 * src/metrics.py:74-80 for one uint8 [H][W][3] image -> out fp32 [299][299][4], channel 3 zero.  xstart / xcount
 * int[299] and xweight float[299][kx] are the width taps, the y tables the height taps (fid_host.aa_taps); the width
 * pass runs first, as ATen's.
 * irx_op_fid_bn_relu: out[r][coff + c] = max(x[r][c] * scale[c] + shift[c], 0), x fp32 [rows][C], out rows ldo floats.
 * irx_op_fid_avgpool3: F.avg_pool2d(x, 3, 1, 1) (always / 9) over fp32 NHWC.
 * irx_op_fid_maxpool3s2: F.max_pool2d(x, 3, 2) over fp32 NHWC into out[n][ho][wo] rows of ldo floats at channel coff.
 * irx_op_fid_gap: the mean over the hw pixels of x fp32 [batch][hw][C], added in pixel order, one division.
 * C, ldo and coff are multiples of 4; buffers 16-byte aligned. */
int irx_op_fid_input(void* stream, const uint8_t* img, int H, int W, const int* xstart, const int* xcount,
                     const float* xweight, int kx, const int* ystart, const int* ycount, const float* yweight, int ky,
                     float* out);
int irx_op_fid_bn_relu(void* stream, const float* x, long rows, int C, const float* scale, const float* shift,
                       float* out, int ldo, int coff);
int irx_op_fid_avgpool3(void* stream, const float* x, int n, int H, int W, int C, float* out);
int irx_op_fid_maxpool3s2(void* stream, const float* x, int n, int H, int W, int C, float* out, int ldo, int coff);
int irx_op_fid_gap(void* stream, const float* x, int batch, int hw, int C, float* out);

/* ---- Real-ESRGAN, the compact network (RestorationPipeline._sr_realesrgan, src/inference.py:579-591: model.enhance
 * at outscale 4; the net it constructs, :335-336; half = (device == "cuda"), :338-346) ----
 * m is an IRX_MODEL_SRVGG model whose blob holds `body.{0,2,..,66}.{weight,bias}` (convs [64,3,3,3], 32 x [64,64,3,3],
 * [48,64,3,3]) and `body.{1,3,..,65}.weight` (PReLU slopes [64]), the keys of realesr-general-x4v3.pth.
 * in_u8 [batch][H][W][3] RGB in device memory, H, W >= 1; in_lut = device float[256], float32(v) / 255
 * (srvgg_host.input_table); out_u8 [batch][4H][4W][3] = round_half_even(clamp(net(x), 0, 1) * 255) with
 * net(x) = pixel_shuffle(body(x), 4) + nearest_x4(x); out_f (NULL: not wanted) fp32 of the same shape = net(x) before
 * the clamp.  An IRX_F16 model rounds to fp16 after each conv + bias, each PReLU and the final add, accumulating in
 * fp32 (the fused kernels of srvgg.hip; option srvgg_fused = 0: the same graph on the general conv kernels); an IRX_F32
 * model runs every conv in exact fp32.  The same bits on every run and at every batch position.
 * ws: irx_srvgg_workspace_bytes(m, batch, H, W) bytes of device memory, 16-byte aligned (it depends on srvgg_fused).
 * The kernels index with 64-bit offsets, but the general conv kernels count rows in an int, so batch * H * W * 64 >
 * INT_MAX is refused for both engines.  A refused argument (null pointer, batch <= 0, H or W < 1, that size limit, a
 * model of another kind or without a bound blob, a short workspace) is a status and launches nothing.  Enqueues on
 * `stream`: no allocation, no synchronisation. */
int irx_srvgg_workspace_bytes(const irx_model* m, int batch, int H, int W, size_t* bytes);
int irx_srvgg_u8(irx_model* m, void* stream, const uint8_t* in_u8, int batch, int H, int W, const float* in_lut,
                 uint8_t* out_u8, float* out_f, void* ws, size_t ws_bytes);
/* the kernels of the network on their own (tests).  x / out: fp16 NHWC [batch][H][W][64], x != out; weight fp16
 * [Cout][3][3][64]; bias and slope fp32, rounded to fp16 when read.
 * irx_op_srvgg_conv: one body layer, out = prelu(fp16(conv3x3(x) + bias)) (srvgg_arch.py: conv, then PReLU).
 * irx_op_srvgg_tail: the last conv (Cout 48) + bias, pixel shuffle 4, + the input pixel from in_u8 / in_lut, as
 *   irx_srvgg_u8 finishes: out_u8 [batch][4H][4W][3], out_f the same shape or NULL.
 * irx_op_srvgg_prelu: out[r][c] = x[r][c] > 0 ? x[r][c] : slope[c] * x[r][c] over [rows][C] of dtype IRX_F32 or
 *   IRX_F16 (slope and product rounded to fp16), C a multiple of 16 bytes of elements; x == out is allowed. */
int irx_op_srvgg_conv(void* stream, const void* x, int batch, int H, int W, const void* weight, const float* bias,
                      const float* slope, void* out);
int irx_op_srvgg_tail(void* stream, const void* x, const uint8_t* in_u8, int batch, int H, int W, const float* in_lut,
                      const void* weight, const float* bias, uint8_t* out_u8, float* out_f);
int irx_op_srvgg_prelu(void* stream, int dtype, const void* x, long rows, int C, const float* slope, void* out);

/* ---- the Stable Diffusion safety checker (StableDiffusionImg2ImgPipeline.run_safety_checker, which ends the
 * reference's img2img calls at src/inference.py:486, :566 and :664; switched off for inpainting, :444-451, :746-752) ----
 * m is an IRX_MODEL_SAFETY model whose blob holds the checkpoint's `vision_model.vision_model.*` tower,
 * `visual_projection.weight`, `special_care_embeds` / `concept_embeds` (rows already divided by max(|row|, 1e-12): the
 * host normalises them once in fp64) and `special_care_embeds_weights` / `concept_embeds_weights` (the thresholds).
 * crop_u8 [batch][S][S][3] in device memory, S = image_size: the decoded uint8 image after CLIPImageProcessor's resize
 * (shortest edge to S, Pillow BICUBIC: irx_resample_u8 with the coefficient tables sliced to the crop window) and centre
 * crop; in_lut = device float[256][3], the processor's rescale + normalise of byte v in channel c
 * (safety_host.input_table).  scores [batch][n_special + n_concepts] = the fp32 cosines (special rows first, not
 * rounded), flags int [batch] = has_nsfw_concept: adj = 0; every special row with rint(((cos - thr) + adj) * 1000) > 0
 * sets adj = 0.01 for the rows after it; flagged if any concept row has rint(((cos - thr) + adj) * 1000) > 0 (numpy's
 * round(x, 3) > 0 on float32, ties to even).  The tower's GEMMs are planned for the canonical batch and the head is one
 * block per image with fixed-order sums: image i has the same scores at every batch size.  batch <= 64.
 * ws: irx_safety_workspace_bytes(m, batch) bytes of device memory, 16-byte aligned.  A refused argument (null pointer,
 * batch outside [1, 64], a model of another kind or without a bound blob, a short workspace) is a status and launches
 * nothing.  Enqueues on `stream`: no allocation, no synchronisation.
 * irx_safety_embed_u8: the fp32 image embeddings [batch][projection_dim] the head reads, without the head (tests).
 * irx_safety_blank_u8: img[b] (uint8 [batch][H][W][3]) and, if not NULL, f01[b] (fp32, the same shape) become zeros
 * for every b with flags[b] != 0: the black image run_safety_checker returns.  flags is device memory. */
int irx_safety_workspace_bytes(const irx_model* m, int batch, size_t* bytes);
int irx_safety_check_u8(irx_model* m, void* stream, const uint8_t* crop_u8, int batch, const float* in_lut,
                        float* scores, int* flags, void* ws, size_t ws_bytes);
int irx_safety_embed_u8(irx_model* m, void* stream, const uint8_t* crop_u8, int batch, const float* in_lut,
                        float* embeds, void* ws, size_t ws_bytes);
int irx_safety_blank_u8(void* stream, uint8_t* img, float* f01, int batch, int H, int W, const int* flags);
/* the kernels of the checker on their own (tests).
 * irx_op_safety_patches: crop_u8 [batch][S][S][3] -> out [batch * (S / patch)^2][kpad] of `dtype`, column
 *   (c * patch + ky) * patch + kx = in_lut[byte][c] cast to dtype, columns [3 patch^2, kpad) zero.
 * irx_op_safety_tokens: out[b][0] = cls + pos[0], out[b][1 + p] = patch_out[b][p] + pos[1 + p] (fp32 sum, one
 *   rounding); patch_out [batch][P][D], pos [P + 1][D], out [batch][P + 1][D] of `dtype`; cls fp32 [D].
 * irx_op_safety_head: embeds fp32 [batch][n]; special [n_special][n], concepts [n_concepts][n] (unit rows) and the
 *   thresholds fp32 -> scores, flags as irx_safety_check_u8 writes them. */
int irx_op_safety_patches(void* stream, int dtype, const uint8_t* crop_u8, int batch, int S, int patch, int kpad,
                          const float* in_lut, void* out);
int irx_op_safety_tokens(void* stream, int dtype, const void* patch_out, const float* cls, const void* pos, int batch,
                         int P, int D, void* out);
int irx_op_safety_head(void* stream, const float* embeds, int batch, int n, const float* special, int n_special,
                       const float* concepts, int n_concepts, const float* thr_special, const float* thr_concepts,
                       float* scores, int* flags);

/* ---- Real-ESRGAN, the RRDBNet of RealESRGAN_x4plus.pth (the RealESRGANer the reference builds at
 * src/inference.py:335-346 around the file it names, and model.enhance in _sr_realesrgan, :579-591, at outscale 4,
 * tile 0, pre_pad 0) ----
 * m is an IRX_MODEL_RRDB model whose blob holds `conv_first`, `body.{0..num_block-1}.rdb{1,2,3}.conv{1..5}`,
 * `conv_body`, `conv_up1`, `conv_up2`, `conv_hr`, `conv_last` (.weight / .bias), the keys of RealESRGAN_x4plus.pth.
 * in_u8 [batch][H][W][3] RGB in device memory, H, W >= 1; in_lut = device float[256], float32(v) / 255
 * (srvgg_host.input_table); out_u8 [batch][4H][4W][3] = round_half_even(clamp(net(x), 0, 1) * 255); out_f (NULL: not
 * wanted) fp32 of the same shape = net(x) before the clamp.  net: feat = conv_first(x); 23 x RRDB (three dense blocks
 * x5 * 0.2 + x, then * 0.2 + the RRDB's input); feat += conv_body(.); lrelu(conv_up1(nearest x2)); lrelu(conv_up2(
 * nearest x2)); conv_last(lrelu(conv_hr(.))); LeakyReLU slope 0.2.  An IRX_F16 model accumulates in fp32 and rounds to
 * fp16 after each conv + bias (bias read as fp16), each LeakyReLU (v > 0 ? v : fp16(0.2f * v)) and each step of
 * fp16(fp16(0.2f * t) + x): PyTorch's eager fp16 rounding points (the kernels of rrdb.hip; option rrdb_fused = 0: the
 * same graph and rounding points on the general conv kernels).  An IRX_F32 model runs every conv in exact fp32.  The
 * same bits on every run and at every batch position.
 * ws: irx_rrdb_workspace_bytes(m, batch, H, W) bytes of device memory, 16-byte aligned (it depends on rrdb_fused).
 * The fused kernels index with 64-bit offsets; the general conv kernels count elements in an int, so on that path
 * batch * 4H * 4W * 64 > INT_MAX is refused.  A refused argument (null pointer, batch <= 0, H or W < 1, a size limit, a
 * model of another kind or without a bound blob, a short workspace) is a status and launches nothing.  Enqueues on
 * `stream`: no allocation, no synchronisation. */
int irx_rrdb_workspace_bytes(const irx_model* m, int batch, int H, int W, size_t* bytes);
int irx_rrdb_u8(irx_model* m, void* stream, const uint8_t* in_u8, int batch, int H, int W, const float* in_lut,
                uint8_t* out_u8, float* out_f, void* ws, size_t ws_bytes);
/* the body kernel of that network on its own (tests): one 3x3 / pad 1 conv of the dense block, as the fp16 engine
 * calls it for RRDBNet's forward (basicsr rrdbnet_arch.py; what model.enhance runs at src/inference.py:579-591).
 * x: fp16 NHWC [batch][H][W] pixels ldx elements apart, channels [0, cin) read, cin a multiple of 32 in [32, 192];
 * weight fp16 [cout][3][3][cin], cout 32 or 64; bias fp32 [cout], rounded to fp16 when read.
 * v = fp16(conv + bias); lrelu != 0: v = v > 0 ? v : fp16(0.2f * v); res1 != NULL: v = fp16((res1_scaled ?
 * fp16(0.2f * v) : v) + res1[pixel * ldr1 + c]); res2 != NULL: v = fp16(fp16(0.2f * v) + res2[pixel * ldr2 + c]);
 * out[pixel * ldo + c] = v for c in [0, cout): `out` points at the first channel of the slice and nothing else is
 * written.  out may equal res2 (the end of an RRDB) but must not overlap the channels of x that are read.
 * ldx, ldo % 8 == 0, ldr1, ldr2 % 4 == 0; x and weight 16-byte, out, res1 and res2 8-byte aligned. */
int irx_op_rrdb_conv(void* stream, const void* x, int ldx, int cin, int batch, int H, int W, const void* weight,
                     const float* bias, int cout, int lrelu, const void* res1, int ldr1, int res1_scaled,
                     const void* res2, int ldr2, void* out, int ldo);

/* ---- multi-GPU: RCCL over xGMI (SURVEY.md §8b `irx_weights_bcast(handle, rcclComm)`, §8e) ----
   The reference has no multi-device path (src/inference.py:52-57 picks one device; it stands in for
   `pipe.to("cuda")` at src/inference.py:175-176 on every rank but the first).  One process per GPU: rank 0
   creates the id, the caller ships its 128 bytes to the other ranks over any host channel (the torchrun
   store), each rank creates its communicator on its current HIP device, and the packed weight blob bound to
   a model is broadcast in place from `root`, enqueued on `stream`.  No per-step collectives exist. */
#define IRX_RCCL_ID_BYTES 128
int irx_rccl_available(void);                        /* 1 when librccl can be loaded, else 0 */
int irx_rccl_unique_id(unsigned char* id);           /* id: IRX_RCCL_ID_BYTES bytes (ncclGetUniqueId) */
int irx_rccl_comm_init(const unsigned char* id, int nranks, int rank, void** comm);   /* ncclCommInitRank */
/* the same with a deadline: ncclCommInitRankConfig(blocking = 0) polled with ncclCommGetAsyncError; on an error or
   after timeout_ms the half-made communicator is released with ncclCommAbort, *comm stays NULL and the call fails
   (irx_last_error says which), so a rank whose peers fail or never arrive leaves the init.  timeout_ms <= 0: the
   blocking form.  Communicators made this way are non-blocking: irx_rccl_broadcast / irx_weights_bcast wait for
   each enqueue themselves. */
int irx_rccl_comm_init_timeout(const unsigned char* id, int nranks, int rank, int timeout_ms, void** comm);
int irx_rccl_comm_destroy(void* comm);
int irx_rccl_broadcast(void* comm, void* buf, size_t bytes, int root, void* stream);  /* in place, uint8 */
/* broadcast the model's bound weight blob (irx_model_bind) from `root`; every rank must have bound a blob of
   irx_model_blob_bytes first (non-root ranks: uninitialised memory that this call fills) */
int irx_weights_bcast(irx_model* m, void* comm, int root, void* stream);

/* ---- single-op entry points (parity tests, composition) ---- */
int irx_op_conv2d(void* stream, int dtype, const void* x0, const void* x1, int c0, int c1, int n, int hin, int win,
                  int hv, int wv, const void* weight, const float* bias, int cout, int kh, int kw, int stride,
                  int pad_t, int pad_l, int ho, int wo, const float* rowadd, long rowadd_ld, const void* residual,
                  void* out, int out_f32, int act);
int irx_op_gemm(void* stream, int dtype, int M, int N, int K, const void* A, long lda, const void* B, long ldb,
                void* C, long ldc, const float* bias, float alpha, int act, const void* residual, long ldr,
                int out_f32, int batch, long sA, long sB, long sC, long sR);
/* C[M][N] = A[M][K] B[N][K]^T + bias + residual[m < res_rows ? m : m - res_rows][:] (all contiguous): the repeating
   residual of the shared classifier-free-guidance prefix (irx_unet_forward_ex).  16-bit dtypes, batch 1 and
   res_rows < M <= 2 res_rows only; anything else is an error. */
int irx_op_gemm_res_rows(void* stream, int dtype, int M, int N, int K, const void* A, const void* B, const float* bias,
                         const void* residual, long res_rows, void* C, int batch);
/* split-K partial bytes a dense [M][K] x [N][K]^T GEMM of this shape takes from its caller's workspace (the models
   carve them from their arena; bare irx_op_gemm calls use the library's scratch) */
size_t irx_op_gemm_workspace_bytes(int dtype, int M, int N, int K, int act, int out_f32, int imgs);
int irx_op_group_norm(void* stream, int dtype, const void* x0, const void* x1, int c0, int c1, int n, int hw,
                      int groups, float eps, const float* gamma, const float* beta, int silu, void* out, void* ws);
size_t irx_op_group_norm_ws_bytes(int n, int hw, int groups);
/* GroupNorm(+SiLU) of (x0 | x1) folded into a 3x3 / stride-1 / pad-1 conv's halo operand path (the form the
   UNet / VAE resnets run); bias / rowadd / residual as irx_op_conv2d.  Fails (IRX error) when the shape does
   not take the fused path: *fused reports whether it would (query with out == NULL, nothing launched).
   ws: irx_op_gn_conv3_ws_bytes(n, h * w, groups, c0 + c1) bytes
   (= round_up(n * (c0 + c1) * 8, 256) + irx_op_group_norm_ws_bytes). */
size_t irx_op_gn_conv3_ws_bytes(int n, int hw, int groups, int channels);
int irx_op_gn_conv3(void* stream, int dtype, const void* x0, const void* x1, int c0, int c1, int n, int h, int w,
                    int groups, float eps, const float* gamma, const float* beta, int silu, const void* weight,
                    const float* bias, int cout, const float* rowadd, long rowadd_ld, const void* residual,
                    void* out, void* ws, int* fused);
/* GroupNorm(+SiLU) -> 3x3 / stride-1 / pad-1 conv to cout <= 16 channels in one kernel: the output heads of the UNet
   and VAE that src/inference.py:486 runs (conv_norm_out -> conv_out).  x [n][h][w][c] (16-bit, c % 64 == 0),
   weight [cout][3][3][c], out [n][h][w][ldo] (fp32 when out_f32, else the dtype).  Statistics by a pass over x.
   ws: irx_op_gn_conv3_ws_bytes(n, h * w, groups, c) bytes. */
int irx_op_gn_conv_narrow(void* stream, int dtype, const void* x, int n, int h, int w, int c, int groups, float eps,
                          const float* gamma, const float* beta, int silu, const void* weight, const float* bias,
                          int cout, void* out, int ldo, int out_f32, void* ws);
/* GroupNorm (no SiLU) -> projection: the diffusers Transformer2DModel norm -> proj_in of the UNet that
   src/inference.py:486 runs.  out[i][p][:] = GN(x)[i][p][:] W^T + bias for x [n][hw][k], W [nout][k], out [n][hw][nout].
   With option gn_fold (default) and a shape whose large-tile row tiles never straddle two images, GroupNorm is folded
   into per-image weights o = round(W diag(a_i)) and biases bias + W beta - o mean_i (the engine's form; the normalised
   tensor is never written); otherwise GroupNorm then GEMM.  *folded = 1 when the fold runs, *splits = the large-tile
   K splits (0: not on the large tiles); query both with out == NULL (nothing launched).
   ws: irx_op_gn_proj_ws_bytes(n, hw, groups, k, nout) bytes. */
size_t irx_op_gn_proj_ws_bytes(int n, int hw, int groups, int k, int nout);
int irx_op_gn_proj(void* stream, int dtype, const void* x, int n, int hw, int k, int groups, float eps,
                   const float* gamma, const float* beta, const void* w, const float* bias, int nout, void* out,
                   void* ws, int* folded, int* splits);
int irx_op_layer_norm(void* stream, int dtype, const void* x, int rows, int c, float eps, const float* gamma,
                      const float* beta, void* out);
int irx_op_attention(void* stream, int dtype, int batch, int heads, int lq, int lk, int d, const void* q, long ldq,
                     long sq, const void* k, long ldk, long sk, const void* v, long ldv, long sv, void* o, long ldo,
                     long so, float scale, int causal);
/* heads laid out [batch][heads][len][d] (q, k, v and o), contiguous */
int irx_op_attention_hm(void* stream, int dtype, int batch, int heads, int lq, int lk, int d, const void* q,
                        const void* k, const void* v, void* o, float scale);
/* The launch as the models make it: every operand with its own row stride (ld*), batch stride (s*) and head stride
   (hs*; 0 = heads interleaved in a row, stride d), all in elements, so head-major and row-major operands mix and K / V
   may be column slices of a wider buffer.  q_scaled != 0: q already carries scale * log2(e) (folded into the to_q
   weights), the kernel applies no scale of its own. */
int irx_op_attention_ex(void* stream, int dtype, int batch, int heads, int lq, int lk, int d, const void* q, long ldq,
                        long sq, long hsq, const void* k, long ldk, long sk, long hsk, const void* v, long ldv, long sv,
                        long hsv, void* o, long ldo, long so, long hso, float scale, int causal, int q_scaled);
int irx_op_geglu(void* stream, int dtype, const void* proj, int M, int F, void* out);
/* C[M][N/2] = GEGLU(A B^T + bias) with B/bias in the GEGLU64 row order (fused epilogue, bf16 large tiles) */
int irx_op_gemm_geglu(void* stream, int dtype, int M, int N, int K, const void* A, const void* B, const float* bias,
                      void* C);
/* Transformer residual-stream producer (the diffusers Transformer2D proj_in / attn.to_out at src/inference.py:486's
   UNet): C = A B^T + bias (+ residual, may alias C), also writing the LayerNorm statistics of C's rows:
   final_rs == 0: parts[m][N / 320] = (mean, sum of squared deviations) per 320-column group;
   final_rs != 0 (N == 320): parts[m] = (rstd, rstd * mean) with rstd = rsqrt(var + eps), the folded consumer's rs.
   Error if the shape cannot emit them. */
int irx_op_gemm_ln_out(void* stream, int dtype, int M, int N, int K, const void* A, const void* B, const float* bias,
                       const void* residual, void* C, void* parts, int final_rs, float eps);
/* LayerNorm folded into the following projection (norm1/2/3 -> to_q|k|v / attn2.to_q / ff.net.0.proj):
   C = rs.x * (A B^T) - rs.y * u + v with B = W diag(gamma), u = row sums of B, v = bias + W beta, and per row
   rs = (rstd, rstd * mean) of A given directly (rs, from a statistics pass) or merged from T producer partials
   (parts, irx_op_gemm_ln_out; K = 320 T).  geglu != 0: B / u / v in the GEGLU64 row order, C gets N / 2 columns. */
int irx_op_gemm_ln_fold(void* stream, int dtype, int M, int N, int K, const void* A, const void* B, const float* u,
                        const float* v, const void* rs, const void* parts, int T, int geglu, void* C);
/* The same pair with the partial group width given: `width` = 320 or 128 columns per partial (the producer's tile
   width: parts[m][N / width], K = width T), and for the producer a residual that repeats every res_rows rows
   (0: one residual row per output row; M <= 2 res_rows). */
int irx_op_gemm_ln_out_w(void* stream, int dtype, int M, int N, int K, const void* A, const void* B, const float* bias,
                         const void* residual, long res_rows, void* C, void* parts, int width, int final_rs,
                         float eps);
int irx_op_gemm_ln_fold_w(void* stream, int dtype, int M, int N, int K, const void* A, const void* B, const float* u,
                          const float* v, const void* rs, const void* parts, int T, int width, int geglu, void* C);
/* GroupNorm statistics from producer partials: the 16-bit UNet / VAE GroupNorms read (sum, sum of squares) blocks
   written by the kernel that stored the tensor instead of making a statistics pass.  The three producers below run
   the GEMM exactly as the models do (same arguments, same plan, split-K partials from `ws`) and write, next to the
   output, parts[block][channel] = (sum, sum of squares) (two doubles) of the stored values over blocks of *rows
   consecutive output rows of one image (row = pixel of the [n][ho][wo] output); the strip halo tiles' blocks are 8 x 32
   pixel strips, and only an image's total is defined there.  *rows == 0: this call emits none and `parts` stays
   untouched.  With out / C == NULL nothing is launched: the call only fills the out-parameters, *ws_bytes included
   (the bytes `ws` must hold).
   conv: the arguments of irx_op_conv2d; *splits = K splits of the large-tile path (0: not on it), *halo = the halo
   main loop the plan launches (0: not a halo conv; 2 whole-row tiles, 5 strip tiles, 8 four 8x8 images per tile).
   *rows == 64 with *splits > 2 is the split-K reduce kernel's emission; two splits reduce in the kernel. */
int irx_op_conv2d_gn_parts(void* stream, int dtype, const void* x0, const void* x1, int c0, int c1, int n, int hin,
                           int win, int hv, int wv, const void* weight, const float* bias, int cout, int kh, int kw,
                           int stride, int pad_t, int pad_l, int ho, int wo, const float* rowadd, long rowadd_ld,
                           const void* residual, void* out, int out_f32, int act, double* parts, void* ws, int* rows,
                           int* splits, int* halo, size_t* ws_bytes);
/* dense: C[M][N] = A[M][K] B[N][K]^T + bias + residual (all contiguous) over `imgs` images of M / imgs rows */
int irx_op_gemm_gn_parts(void* stream, int dtype, int M, int N, int K, const void* A, const void* B, const float* bias,
                         const void* residual, int imgs, void* C, double* parts, void* ws, int* rows, int* splits,
                         size_t* ws_bytes);
/* nearest-2x upsample + 3x3 conv as four per-parity 2x2 convs (IRX_LAYOUT_CONV_UP2 weights w2 [4][c][2][2][c]):
   x [n][h][w][c] -> out [n][2h][2w][c].  Partial block (image * 4 + p) * (h w / *rows) + j holds rows j * *rows ...
   of the low-resolution pixels of parity p = 2a + b, i.e. of out[image][a::2][b::2] flattened; parts has
   4 n h w / *rows blocks.  *up2_ok = 0: the shape does not take this form (running it is an error). */
int irx_op_upsample_conv_gn_parts(void* stream, int dtype, const void* x, int n, int h, int w, int c, const void* w2,
                                  const float* bias, void* out, double* parts, void* ws, int* up2_ok, int* rows,
                                  size_t* ws_bytes);
/* the consumers: GroupNorm(+SiLU) of (x0 | x1) from the partials p0 / p1 of r0 / r1 rows per block (finalize + apply,
   or the fused kernel of option gn_fa); ws: irx_op_group_norm_ws_bytes */
int irx_op_group_norm_parts(void* stream, int dtype, const void* x0, const void* x1, int c0, int c1, int n, int hw,
                            int groups, float eps, const float* gamma, const float* beta, int silu, void* out,
                            const double* p0, int r0, const double* p1, int r1, void* ws);
/* ... the finalize alone: ab[n][c0] = (gamma rstd, beta - mean gamma rstd), mr[n][groups] = (mean, rstd) (mr may be
   NULL); both pairs of floats */
int irx_op_group_norm_parts_ab(void* stream, int c0, int n, int hw, int groups, float eps, const float* gamma,
                               const float* beta, const double* p0, int r0, void* ab, void* mr);
/* The elementwise kernels the models run between GEMMs, one entry each.
   softmax_rows: out[r][0, cols) = softmax(in[r][0, cols)) of fp32 rows (row strides ldi, ldo); it also ZEROES the
   padded columns [cols, ldo) of every output row (the fp32 VAE attention multiplies them with V^T's padding).
   transpose2d: out[z][c][r] = in[z][r][c] per batch z (strides s_in, s_out); columns [rows, ldo) of out are left alone.
   timestep_embed: out[b][dim] = the sinusoidal embedding of t[b] (diffusers get_timestep_embedding, max_period 1e4).
   embed_tokens: out[b][l][:] = tok[ids[b][l]][:] + pos[l][:], summed in fp32. */
int irx_op_softmax_rows(void* stream, int dtype, const float* in, long ldi, int rows, int cols, void* out, long ldo);
int irx_op_transpose2d(void* stream, int dtype, const void* in, long ldi, int rows, int cols, void* out, long ldo,
                       int batch, long s_in, long s_out);
int irx_op_timestep_embed(void* stream, int dtype, const float* t, int B, int dim, int flip_sin_to_cos, float shift,
                          void* out);
int irx_op_embed_tokens(void* stream, int dtype, const int* ids, int B, int L, const void* tok, const void* pos, int D,
                        void* out);

#ifdef __cplusplus
}
#endif
#endif /* IRX_H_ */
