/* mlimgsynth_amd.h — model graphs, sampler and the generation driver of the MI355X engine.
 *
 * Mirrors, for the hot path only, the reference's model/sampler interfaces:
 *   UnetParams / unet_*      src/unet.h:10-62        VaeParams / sdvae_decode   src/vae.h:10-53
 *   SdTaeParams / sdtae_*    src/tae.h               ClipParams / clip_text_*   src/clip.h
 *   DenoiseSampler           src/sampling.h:17-46    Solver (Euler)             src/solvers.h:65-77
 *   RngPhilox                src/ccommon/rng_philox.h:10-22
 *   mlis_generate slice      include/mlimgsynth.h:414-558, src/mlimgsynth.c:1634-1773
 * Differences that are the point of the exercise: every graph takes a batch dimension N
 * (the reference rejects n_batch > 1, src/mlimgsynth.c:1640), cond and uncond evaluations
 * of classifier-free guidance run as ONE batch-2B UNet evaluation, and the latent, the
 * Euler(-ancestral) update and the CFG mix stay on the device between steps.
 * Return convention: >=1 ok, <0 error (reference TRY convention), text in mlsd_last_error().
 */
#pragma once
#include "mlblock_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- UNet (src/unet.h) */
typedef struct {
	int n_ch_in, n_ch_out, n_res_blk;
	int attn_res[4];
	int ch_mult[5];
	int transf_depth[5];
	int n_te, n_head, d_head, n_ctx, n_ch, ch_adm_in;
	int clip_norm, cond_label, uncond_empty_zero, vparam;
	int n_step_train;
	float sigma_min, sigma_max;
	int zsnr;                /* the sigma table unet_t_to_sigma / unet_sigma_to_t / dnsamp_schedule read: 0 the scaled-linear one, 1 its zero-terminal-SNR rescale
	                          * (unet_params_set_zsnr keeps sigma_max in step); not in the reference's structure: appended */
} UnetParams;

/* "sd1" | "sd2" | "sdxl" (g_unet_sd1/sd2/sdxl, src/unet.c:21-83) | "tiny" | "tinyxl" (test configs) */
int unet_params_get(const char* model, UnetParams* out);

MLTensor* mlb_unet_denoise(MLCtx* C, MLTensor* x, MLTensor* time, MLTensor* c, MLTensor* label, const UnetParams* P);

void  unet_params_init(void);
float unet_sigma_to_t(const UnetParams* P, float sigma);
float unet_t_to_sigma(const UnetParams* P, float t);
/* The zero-terminal-SNR table ("Common Diffusion Noise Schedules and Sample Steps are Flawed", 2023, Algorithm 1; not in the reference), built beside the plain one
 * from the same double-precision cumulative products abar_i: s_i = sqrt(abar_i), s'_i = (s_i - s_999) s_0 / (s_0 - s_999), abar'_i = s'_i^2, the last clamped to
 * 4.8973451890853435e-08 (sigma 4518.76; the front ends' constant as recalled, parity-unpinned), sigma'_i = sqrt((1 - abar'_i) / abar'_i), stored as float logs.
 * unet_log_sigmas: the 1000 stored logs of either table.  unet_params_set_zsnr: the flag and the sigma range that goes with it.  unet_params_sizeof: sizeof(UnetParams). */
const float* unet_log_sigmas(int zsnr);
void  unet_params_set_zsnr(UnetParams* P, int zsnr);
int   unet_params_sizeof(void);

typedef struct {
	MLCtx* ctx;
	const UnetParams* par;
	unsigned nfe;
	int lw, lh, n_batch;           /* graph batch N (= 2*images with CFG) */
	MLTensor *t_x, *t_t, *t_c, *t_l, *t_out;
} UnetState;

/* (LocalTensor, the host tensor of the reference's boundary == MLIS_Tensor of include/mlimgsynth.h:409-413, and its ltensor_*
 * calls are declared in mlblock_amd.h) */

/* the reference's own entry points, same signatures (src/unet.h:55-62): batch 1, graph built at init, weights loaded afterwards
 * (mlctx_params_synth / mlctx_tstore_load on C).  `split` (--unet-split weight streaming, src/unet.c:390-458) is accepted and
 * ignored: weights are resident.  x [lw,lh,4,1], cond [n_ctx,77,1,1], label [adm,1,1,1] or NULL -> dx like x (resized). */
int unet_denoise_init(UnetState* S, MLCtx* C, const UnetParams* P, unsigned lw, unsigned lh, bool split);
int unet_denoise_run(UnetState* S, const LocalTensor* x, const LocalTensor* cond, const LocalTensor* label, float sigma, LocalTensor* dx);

/* builds the batch-N graph on C (prefix "unet"); weights are loaded afterwards with
 * mlctx_params_synth / mlctx_param_set */
int unet_denoise_init_n(UnetState* S, MLCtx* C, const UnetParams* P, unsigned lw, unsigned lh, unsigned n_batch);
/* the same with a context of n_ctx_tok rows (77 x W, windowed prompt; 0 = 77): input "c" is [n_ctx, n_ctx_tok, N] */
int unet_denoise_init_nc(UnetState* S, MLCtx* C, const UnetParams* P, unsigned lw, unsigned lh, unsigned n_batch, int n_ctx_tok);
/* second half of the init: records the graph and calls mlctx_prep (split so that the x input can first be
 * bound to a device-resident latent with mlctx_input_bind) */
int unet_denoise_build(UnetState* S);
/* host-boundary evaluation (tests, drop-in for src/unet.c:460-498 with a batch): x [N][4][lh][lw] NCHW,
 * cond [N][77][n_ctx] (N x the plan's n_ctx_tok rows), label [N][adm] or NULL, sigma[N] -> dx like x.  Applies c_in, sigma->t, v-param. */
int unet_denoise_run_n(UnetState* S, const float* x, const float* cond, const float* label,
	const float* sigma, float* dx);

/* ---------------------------------------------------------------- ControlNet (not in the reference; the published cldm.py layout)
 * A trainable copy of the UNet's encoder and middle block that also sees a control image (pose, depth, edges, tile).  Its outputs -- one per tensor the UNet pushes
 * on its skip stack, through a 1x1 "zero" convolution each, and one for the middle block -- are added, times a gain, to the UNet's skip tensors and to mid.2's output.
 * Three plans: the hint block (control_hint_*, once per image), the ControlNet (controlnet_*, per evaluation, on the UNet plan's inputs) and a UNet plan built with
 * unet_denoise_build_ctrl, which reads the residuals where the ControlNet plan leaves them (channels-last fp32) and the gain from one float of device memory. */
#define MLB_CONTROL_MAX 48
typedef struct {
	int n;                              /* residuals: skip tensors + 1 */
	const float* r[MLB_CONTROL_MAX];    /* device, channels-last fp32 [n_img][rows][ld] */
	int64_t ld[MLB_CONTROL_MAX];
	int c[MLB_CONTROL_MAX], rows[MLB_CONTROL_MAX];   /* channels and rows per image of each */
	int n_img;                          /* images the residuals hold; image n of the UNet plan reads image n % n_img */
	const float* gain;                  /* device: the gain of the next evaluation (0: the residuals are not read) */
} UnetControl;
MLTensor* mlb_unet_denoise_ctrl(MLCtx* C, MLTensor* x, MLTensor* time, MLTensor* c, MLTensor* label, const UnetParams* P, const UnetControl* K);   /* K NULL: mlb_unet_denoise */
int unet_denoise_build_ctrl(UnetState* S, const UnetControl* K);       /* unet_denoise_build with the control inputs; K NULL: the plain plan, op for op */
/* FreeU (version 2 of the published code; not in the reference): at every decoder concatenation whose backbone has n_ch x the top multiplier channels (stage 1) or
 * half of that (stage 2) the backbone's first half is scaled by (b - 1) x its normalised channel-mean map + 1 (mlsd_freeu_backbone) and the skip tensor's four lowest
 * spatial frequencies by s (mlsd_freeu_skip), both into fresh fp32 tensors.  The factors are device data: plans and captured graphs never change with them. */
typedef struct {
	const float* f;                     /* device: b1, b2, s1, s2 (four floats, each read on its own) */
	int n_stage1, n_stage2;             /* out: concatenations treated at each stage */
} UnetFreeU;
MLTensor* mlb_unet_denoise_freeu(MLCtx* C, MLTensor* x, MLTensor* time, MLTensor* c, MLTensor* label, const UnetParams* P, const UnetControl* K, UnetFreeU* F);   /* F NULL: mlb_unet_denoise_ctrl */
int unet_denoise_build_freeu(UnetState* S, const UnetControl* K, UnetFreeU* F);      /* unet_denoise_build_ctrl with FreeU; F NULL: that plan, op for op */

typedef struct {
	MLCtx* ctx;
	const UnetParams* par;
	int lw, lh, n_batch;
	MLTensor *t_x, *t_t, *t_c, *t_l;    /* the UNet plan's inputs, same shapes */
	MLTensor *t_hint;                   /* hint embedding, fp32 channels-last [n_batch][lh lw][n_ch]: the caller writes its device memory (mlctx_tensor_device_f32) */
	int n_res;
	MLTensor* t_res[MLB_CONTROL_MAX];   /* residuals in skip-stack push order, the middle block's last */
} ControlState;
/* hint block: RGB image [w,h,3,1] in [0,1] at pixel size -> [w/8,h/8,n_ch,1]; prefix "control" (parameters control.hint.<0|2|..|14>) */
int control_hint_init(MLCtx* C, const UnetParams* P, unsigned w, unsigned h, MLTensor** t_img);
int control_hint_build(MLCtx* C, const UnetParams* P, MLTensor* t_img);
/* the ControlNet for a base model with parameters P at the UNet plan's size and batch (prefix "control"); init / build split like the UNet's so that x can be bound */
int controlnet_init_nc(ControlState* S, MLCtx* C, const UnetParams* P, unsigned lw, unsigned lh, unsigned n_batch, int n_ctx_tok);
int controlnet_build(ControlState* S);
MLTensor* mlb_controlnet(MLCtx* C, ControlState* S, MLTensor* x, MLTensor* time, MLTensor* c, MLTensor* label, MLTensor* hint, const UnetParams* P);
int controlnet_control(const ControlState* S, const float* gain_dev, UnetControl* K);     /* the residuals of a built plan, for unet_denoise_build_ctrl */

/* ---------------------------------------------------------------- VAE / TAE decoders */
typedef struct {
	int ch_x, ch_z, ch, n_res, n_res_blk;
	int ch_mult[5];
	int d_embed, f_down;
	float scale_factor;
} VaeParams;
int vae_params_get(const char* model, VaeParams* out);   /* "sd1" | "sdxl" | "tiny" */
MLTensor* mlb_sdvae_decoder(MLCtx* C, MLTensor* x, const VaeParams* P);
/* builds the decode graph for n images of lw x lh latents on C (prefix "vae"); result [8lw,8lh,3,n] */
int sdvae_decode_init(MLCtx* C, const VaeParams* P, unsigned lw, unsigned lh, unsigned n_batch, MLTensor** t_latent);
/* host-boundary decode incl. the (x+1)/2 post (src/vae.h:43-47): latent NCHW [n][4][lh][lw] -> img [n][3][8lh][8lw] */
int sdvae_decode_run(MLCtx* C, MLTensor* t_latent, const float* latent, float* img);
/* graph build + prep only (the driver binds the resident latent and calls mlctx_compute itself) */
int sdvae_decode_build(MLCtx* C, const VaeParams* P, MLTensor* t_latent);

/* encoder (img2img / in-painting source; src/vae.c:76-128,231-316): image [n][3][h][w] in [0,1] -> moments
 * [n][2*ch_z][h/8][w/8] = (mean | logvar); the latent sample is a separate step (mlsd_latent_sample) */
MLTensor* mlb_sdvae_encoder(MLCtx* C, MLTensor* x, const VaeParams* P);
int sdvae_encode_init(MLCtx* C, const VaeParams* P, unsigned w, unsigned h, unsigned n_batch, MLTensor** t_img);
int sdvae_encode_build(MLCtx* C, const VaeParams* P, MLTensor* t_img);
int sdvae_encode_run(MLCtx* C, MLTensor* t_img, const float* img, float* moments);

typedef struct { int ch_x, ch_inner, ch_z, n_blk; } SdTaeParams;
MLTensor* mlb_sdtae_decoder(MLCtx* C, MLTensor* x, const SdTaeParams* P);
int sdtae_decode_init(MLCtx* C, unsigned lw, unsigned lh, unsigned n_batch, MLTensor** t_latent);
int sdtae_decode_run(MLCtx* C, MLTensor* t_latent, const float* latent, float* img);
int sdtae_decode_build(MLCtx* C, MLTensor* t_latent);
MLTensor* mlb_sdtae_encoder(MLCtx* C, MLTensor* x, const SdTaeParams* P);       /* src/tae.c:43-63 */
int sdtae_encode_init(MLCtx* C, unsigned w, unsigned h, unsigned n_batch, MLTensor** t_img);
int sdtae_encode_build(MLCtx* C, MLTensor* t_img);
int sdtae_encode_run(MLCtx* C, MLTensor* t_img, const float* img, float* latent);

/* ---------------------------------------------------------------- CLIP text encoder (src/clip.h) */
typedef struct {
	int n_vocab, n_token, d_embed, n_interm, n_head, n_layer;
	int tok_start, tok_end, tok_pad;
} ClipParams;
int clip_params_get(const char* model, ClipParams* out);   /* "vit_l" | "vit_h" | "vit_bigg" | "tiny" */
/* clip_text_encode (src/clip.c:439-488) for a batch of n prompts: toks [n][n_tok] (without BOS/EOS/PAD,
 * all prompts padded by the caller to the same n_tok), embed out [n][77][d] or NULL, feat out [n][d] or NULL */
int clip_text_encode(MLCtx* C, const ClipParams* P, const char* tprefix, unsigned n_prompt, unsigned n_tok,
	const int32_t* toks, float* embed, float* feat, int clip_skip, bool norm, uint64_t synth_seed);

/* resident variant: graph + weights stay on the device between prompts (the reference rebuilds the graph
 * and re-uploads the weights for every clip_text_encode call, src/clip.c:458-486) */
typedef struct {
	MLCtx* C;
	ClipParams P;
	MLTensor *t_tokens, *t_embed;
	unsigned n_prompt;
	int want_feat;
	char prefix[16];
	float* text_proj_host;
	MLTensor* t_tap;          /* init_ex with tap_skip > 0: copy of the hidden state clip_skip = tap_skip layers from the end (no norm) */
	void* tap_dev;
} ClipEncoder;
int clip_encoder_init(ClipEncoder* E, MLCtx* C, const ClipParams* P, const char* tprefix, unsigned n_prompt,
	int clip_skip, bool norm, bool want_feat);         /* then load weights: mlctx_params_synth / mlctx_param_set */
int clip_encoder_run(ClipEncoder* E, unsigned n_tok, const int32_t* toks, float* embed, float* feat);
/* one pass for both things SDXL wants from open_clip bigG (src/mlimgsynth.c:1517-1543 runs the tower twice): the whole stack
 * with final norm (pooled feature) AND the un-normed hidden state `tap_skip` layers from the end (the embedding), tapped by a
 * device copy; and prompts of different lengths in one run (prompt + negative prompt): n_tok[p], toks[p] for p < n_used
 * (<= the n_prompt the encoder was built for).  embed / tap out [n_used][77][d], feat out [n_used][d]; any may be NULL. */
int clip_encoder_init_ex(ClipEncoder* E, MLCtx* C, const ClipParams* P, const char* tprefix, unsigned n_prompt,
	int clip_skip, bool norm, bool want_feat, int tap_skip);
int clip_encoder_run_ex(ClipEncoder* E, unsigned n_used, const int* n_tok, const int32_t* const* toks, float* embed, float* tap, float* feat);
void clip_encoder_free(ClipEncoder* E);
/* SDXL vector conditioning (src/mlimgsynth.c:1542-1557): [pooled | emb(h,w) | emb(0,0) | emb(h,w)], 256 dims each */
int sdxl_label_build(const float* feat, int n_feat, int width, int height, float* label, int n_label);

/* ---- text conditioning on resident towers: mlis_text_cond_encode / mlis_clip_tokens_encode
 * (src/mlimgsynth.c:1423-1468,1501-1563).  model "sd1" | "sdxl" | "tiny" | "tinyxl"; tokens without BOS/EOS/padding.
 * cond [77][n_ctx]; label [n_label] (SDXL: pooled bigG feature || size embeddings; NULL for SD1). */
typedef struct MLIS_AmdTextCond MLIS_AmdTextCond;
typedef struct MLIS_AmdCtx MLIS_AmdCtx;          /* the generation driver, below */
MLIS_AmdTextCond* mlis_amd_textcond_create(const char* model, int width, int height, uint64_t weight_seed, void* stream);
/* clip_skip 0 = model default; defer_weights != 0: the towers are built without weights, the caller loads them into
 * mlis_amd_textcond_ctx(T, i) for i < mlis_amd_textcond_n_towers(T) (mlctx_tstore_load / mlctx_param_set) */
MLIS_AmdTextCond* mlis_amd_textcond_create_ex(const char* model, int width, int height, uint64_t weight_seed, void* stream,
	int clip_skip, int defer_weights);
int mlis_amd_textcond_n_towers(const MLIS_AmdTextCond* T);
MLCtx* mlis_amd_textcond_ctx(MLIS_AmdTextCond* T, int i);
int mlis_amd_textcond_set_size(MLIS_AmdTextCond* T, int width, int height);     /* SDXL size embeddings of the label */
/* with per-token weights (prompt emphasis, src/mlimgsynth.c:1457-1463); weights NULL = all 1 */
int mlis_amd_textcond_encode_w(MLIS_AmdTextCond* T, const int32_t* toks, const float* weights, int n_tok, float* cond, float* label);
int mlis_amd_textcond_encode_pair_w(MLIS_AmdTextCond* T, const int32_t* toks, const float* w, int n_tok,
	const int32_t* neg, const float* nw, int n_neg, float* cond, float* label, float* ncond, float* nlabel);   /* both prompts, one run per tower */
void mlis_amd_textcond_destroy(MLIS_AmdTextCond* T);
int mlis_amd_textcond_dims(const MLIS_AmdTextCond* T, int* n_ctx, int* n_label);
double mlis_amd_textcond_flops(const MLIS_AmdTextCond* T);
int mlis_amd_textcond_encode(MLIS_AmdTextCond* T, const int32_t* toks, int n_tok, float* cond, float* label);
/* prompt + negative prompt; an EMPTY negative prompt on SDXL zeroes ncond (uncond_empty_zero, :1702-1703) */
int mlis_amd_textcond_encode_pair(MLIS_AmdTextCond* T, const int32_t* toks, int n_tok, const int32_t* neg, int n_neg,
	float* cond, float* label, float* ncond, float* nlabel);

/* prompt + negative prompt encoded and written into an engine's conditioning inputs in one call (launchers; rank 0 of a multi-GPU job) */
const void* mlis_amd_cond_device(MLIS_AmdCtx* S, int what);   /* the plan's conditioning inputs (0: cond, 1: label), read-only */
int mlis_amd_textcond_apply(MLIS_AmdTextCond* T, MLIS_AmdCtx* E, const int32_t* toks, int n_tok, const int32_t* neg, int n_neg);

/* Prompts longer than 75 tokens: the token list is cut, in order, into WINDOWS of 75 tokens (the last one holds the rest; no
 * comma backtracking, no BREAK keyword).  Each window is encoded as its own 77-token CLIP sequence (BOS, its tokens, EOS,
 * padding) and the windows' embeddings are concatenated along the token axis: [77 W][n_ctx].  A prompt of <= 75 tokens is W = 1
 * and encodes exactly as the functions above. */
#define MLIS_AMD_MAX_WINDOWS 4
#define MLIS_AMD_WINDOW_TOKENS 75
/* the split of n_tok tokens: returns W (1 for an empty prompt) and fills start[W], len[W] (either may be NULL); -1 above 300 tokens */
int mlis_amd_prompt_windows(int n_tok, int* start, int* len);
int mlis_amd_n_ctx_tok(const MLIS_AmdCtx* S);        /* context rows the engine's UNet plan was built for (77 W) */
/* windowed encodings; they return W.  cond [77 W][n_ctx] (the caller sizes it with mlis_amd_prompt_windows), label [n_label] from
 * window 0 at its EOS without weights; weights (emphasis, may be NULL) scale rows 1..len of each window.  The pair pads the
 * side with fewer windows to the other's W with encodings of the empty window; cond and ncond then both hold [77 W][n_ctx].
 * An empty SDXL negative prompt gives ncond = 0 over all 77 W rows (as mlis_amd_textcond_encode_pair). */
int mlis_amd_textcond_encode_ex(MLIS_AmdTextCond* T, const int32_t* toks, const float* weights, int n_tok, float* cond, float* label);
int mlis_amd_textcond_encode_pair_ex(MLIS_AmdTextCond* T, const int32_t* toks, const float* w, int n_tok,
	const int32_t* neg, const float* nw, int n_neg, float* cond, float* label, float* ncond, float* nlabel);

/* ---- CLIP BPE tokenizer (host).  Replaces clip_tokenize and helpers, src/clip.c:59-278 (public entry
 * mlis_text_tokenize, include/mlimgsynth.h); pinned by the 14 KATs of src/test_text_tokenize_clip.c:41-66.
 * The merge table is run-time data here (the reference compiles src/clip_merges.c.h in): id pairs in rank order
 * (token 512+i = merge i) or OpenAI's public bpe_simple_vocab_16e6.txt / merges.txt.  All functions return
 * counts (>= 0) or < 0 on error (mlsd_last_error()). */
typedef struct ClipTokenizer ClipTokenizer;
ClipTokenizer* clip_tokr_new(void);
void clip_tokr_free(ClipTokenizer* T);
int clip_tokr_set_merges(ClipTokenizer* T, const int32_t* pairs /* [n][2] */, int n);
int clip_tokr_load_merges_txt(ClipTokenizer* T, const char* path, int max_merges /* <= 0: CLIP's 48894 */);
int clip_tokr_n_merges(const ClipTokenizer* T);
int clip_tokr_n_vocab(const ClipTokenizer* T);              /* 512 + merges + start/end */
int clip_tokr_byte_to_token(int byte);                      /* clip_tokr_byte_to_token, src/clip.c:113-125 */
int clip_tokr_token_to_byte(int token);
/* text (UTF-8, len < 0: NUL-terminated) -> token ids without BOS/EOS/padding; returns the count */
int clip_tokenize(const ClipTokenizer* T, const char* text, int64_t len, int32_t* out, int max_out);
/* bytes a byte/merge token stands for; returns the byte count (may exceed max: nothing is written past it) */
int clip_token_decode(const ClipTokenizer* T, int32_t token, char* out, int max, int* end_of_word);

/* ---------------------------------------------------------------- checkpoint loading
 * tensor-name conversion: tnconv_sd, src/tensor_name_conv.c:274-324 (0 unused, 1 converted, 2 = open_clip fused in_proj) */
enum { TNCONV_R_UNUSED = 0, TNCONV_R_GOOD = 1, TNCONV_R_QKV_PROJ = 2 };
int tnconv_sd(const char* name, char* out, size_t out_size);
/* ControlNet files, original (cldm.py) layout with or without a leading "control_model.": -> "control.<...>" (the encoder copy through the UNet's rules,
 * input_hint_block.K -> hint.K, zero_convs.I.0 -> zero.I, middle_block_out.0 -> mid_out); 0 for anything else (UNet decoder names, diffusers-named files) */
int tnconv_controlnet(const char* name, char* out, size_t out_size);
/* tensor index over an mmap'd safetensors file (src/ccompute/tensorstore_safet.c:152-205, tensorstore.c:184-323) */
typedef struct MLTStore MLTStore;
typedef struct { char* name; int dtype; int n_dim; int64_t shape[4]; /* shape[0] fastest */ size_t size; const void* data; } MLTSEntry;
/* convert_names != 0: names go through tnconv_sd, unused tensors are dropped and open_clip in_proj tensors are split into
 * q/k/v_proj views (tensor_callback_main / open_clip_attn_conv, src/mlimgsynth.c:989-1055) */
MLTStore* mlts_open(const char* path, int convert_names);              /* safetensors or GGUF v2/v3, detected by content */
MLTStore* mlts_open_safetensors(const char* path, int convert_names);  /* same (kept name) */
int       mlts_entry_to_f32(const MLTSEntry* e, float* out, int64_t n); /* any stored type (incl. GGUF block-quantised) -> fp32 */
void mlts_close(MLTStore* S);
/* LoRA (src/lora.c:9-138, tensor_callback_lora src/mlimgsynth.c:1068-1092): open a kohya-named LoRA file, merge it into the
 * model store: W += (scale | alpha/rank | 1) * mult * up.down for every "<X>.lora_down.weight"; returns the number of tensors patched */
MLTStore* mlts_open_lora(const char* path);
MLTStore* mlts_open_controlnet(const char* path);   /* a ControlNet file: names through tnconv_controlnet ("control.<...>"), unknown tensors dropped */
int mlts_lora_apply(MLTStore* model, const MLTStore* lora, float mult, int wtype);
/* the two halves of mlts_lora_apply, for the path that patches weights already on the device (mlctx_param_lora): the same validation, the same error texts.
 * mlts_lora_resolve: entry i of the adapter -> 0 (not a "<X>.lora_down.weight"), 1 with the item filled, < 0 on error.  mlts_lora_operands: up [n1][n_inner] and
 * down [n_inner][n0] as the merge reads them (fp32, rounded to F16 values unless wtype is F32). */
typedef struct { char key[600]; /* "<X>.weight" */ const MLTSEntry *down, *up; int64_t n0, n1, n_inner; float scale; /* (scale | alpha / n_inner | 1) * mult */ } MLTSLoraItem;
int mlts_lora_resolve(const MLTStore* model, const MLTStore* lora, int i, float mult, MLTSLoraItem* item);
int mlts_lora_operands(const MLTSLoraItem* item, int wtype, float* up, float* down);
int mlts_count(const MLTStore* S);
const MLTSEntry* mlts_at(const MLTStore* S, int i);
const MLTSEntry* mlts_find(const MLTStore* S, const char* name);
int mlts_stats(const MLTStore* S, int* n_unused, int* n_split);
int mlts_markers(const MLTStore* S, int* v_pred, int* ztsnr);      /* marker tensors "v_pred" / "ztsnr" of the file (mlis_amd_prediction_resolve) */
/* mlis_model_identify (src/mlimgsynth.c:1206-1249): "sd1" | "sd2" | "sdxl" or NULL; *wtype = dtype of the probe tensor */
const char* mlts_model_identify(const MLTStore* S, int* wtype);
/* mlctx_tstore_load (src/mlblock.c:266-292): every parameter of the prepared plan by name; element count checked */
int mlctx_tstore_load(MLCtx* C, const MLTStore* S);
int mlctx_tstore_load_key(MLCtx* C, const MLTStore* S, const char* key);      /* one of them */

/* ---------------------------------------------------------------- ESRGAN upscaler (host/upscaler.c; not in the reference)
 * RRDBNet x4 (num_feat 64, num_grow_ch 32, num_block from the file) on mlsd_conv3x3_dense.  spec: a safetensors file with BasicSR's names (conv_first,
 * body.{i}.rdb{1..3}.conv{1..5}, conv_body, conv_up1, conv_up2, conv_hr, conv_last, each .weight and .bias; an optional "params_ema." / "params." prefix), or
 * "synth[:seed[:blocks]]" (default seed 1234, 2 blocks).  The x2 pixel-unshuffle variant (conv_first with 12 input channels), a missing tensor and a wrong shape fail
 * with the tensor's name in mlsd_last_error().  run: src [n_img][3][h][w] planar floats in 0..1 on the host -> dst [n_img][3][4h][4w] (not clamped); the work buffers
 * are one device allocation kept between calls and grown on demand.  Zero padding at the image border, whatever the context's tiling. */
typedef struct MLIS_AmdUpscaler MLIS_AmdUpscaler;
MLIS_AmdUpscaler* mlis_amd_upscaler_create(const char* spec);      /* NULL on error */
void mlis_amd_upscaler_destroy(MLIS_AmdUpscaler* U);
int mlis_amd_upscaler_info(const MLIS_AmdUpscaler* U, int* n_block, int* scale);
int mlis_amd_upscaler_run(MLIS_AmdUpscaler* U, const float* src, int w, int h, int n_img, float* dst);

/* ---------------------------------------------------------------- prompt pre-processing (src/prompt_preproc.h:104-209)
 * text = the prompt with emphasis marks / options removed; chunks index into it; loras name into lora_names */
typedef struct { int begin, len; float w; } MLISPromptChunk;
typedef struct { int name_off, len; float w; } MLISPromptLora;
typedef struct {
	char* text; int n_text;
	MLISPromptChunk* chunks; int n_chunk;
	char* lora_names; int n_lora_chars;
	MLISPromptLora* loras; int n_lora;
} MLISPrompt;
int mlis_prompt_set_raw(MLISPrompt* P, const char* text);       /* prompt_text_set_raw */
int mlis_prompt_set_parse(MLISPrompt* P, const char* text);     /* prompt_text_set_parse; MLIS_E_PROMPT_PARSE (-5) on error */
void mlis_prompt_free(MLISPrompt* P);

/* ---------------------------------------------------------------- RNG / schedule / sampler */
typedef struct { uint64_t seed; uint32_t offset; } RngPhilox;   /* src/ccommon/rng_philox.h */
void rng_philox_randn(RngPhilox* S, unsigned n, float* out);
/* values [i0, i1) of the draw the generator stands at, without advancing it (the engine cuts a draw into ranges over host threads) */
void rng_philox_randn_range(const RngPhilox* S, unsigned i0, unsigned i1, float* out);

enum { DNSAMP_SCHED_UNIFORM = 1, DNSAMP_SCHED_KARRAS = 2 };      /* src/sampling.h:11-14 */
enum { SOLVER_METHOD_EULER = 1, SOLVER_METHOD_HEUN = 2, SOLVER_METHOD_TAYLOR3 = 3, SOLVER_METHOD_DPMPP2M = 4,
       SOLVER_METHOD_DPMPP2S = 5 };                              /* src/solvers.h:56-62 == MLIS_Method */

/* dnsamp_init schedule (src/sampling.c:28-96): fills sigmas[0..n_step], returns n_step */
int  dnsamp_schedule(const UnetParams* P, int n_step, int sched, float f_t_ini, float f_t_end, float* sigmas);
void dnsamp_ancestral(float s1, float s2, float eta, float* s_down, float* s_up);

/* ---------------------------------------------------------------- generation driver (mlis_generate slice) */
typedef struct {
	const char* model;       /* "sd1" | "sdxl" | "tiny" | "tinyxl" */
	int width, height;       /* pixels (multiple of 8) */
	int n_batch;             /* images generated together on this GPU */
	int n_step;              /* 20 */
	float cfg_scale;         /* 7 */
	float s_ancestral;       /* 1 = euler_a */
	int sched;               /* DNSAMP_SCHED_UNIFORM */
	int use_tae;             /* decode with TAESD instead of the KL-VAE */
	int use_hipgraph;        /* replay each UNet evaluation as one hipGraph launch */
	uint64_t weight_seed;    /* synthetic weights seed (1234) */
	/* sampler options of dnsamp_init (src/sampling.h:34-38); zero = the reference's defaults */
	int method;              /* SOLVER_METHOD_* (0 -> euler, src/sampling.c:33); 2-NFE solvers halve the step count (:47-49) */
	float s_noise;           /* stochastic sampling noise level (src/sampling.c:139-151) */
	float f_t_ini, f_t_end;  /* relative initial / final time: 0,0 -> 1,0 (txt2img); f_t_ini < 1 = img2img */
	int defer_weights;       /* 1: do not synthesise weights: the caller loads them (mlctx_param_set on the *_ctx handles) */
	int unet_split;          /* > 0: the UNet's weights are STREAMED (the reference's --unet-split / MLIS_OPT_UNET_SPLIT, src/unet.c:390-458): master copy in pinned host
	                          * memory, three to five device slabs (3 for SDXL) of `unet_split` MiB each (1 = the default 512 MiB: 1.5 GiB of slabs + 0.68 GB of resident step-invariant
	                          * weights instead of 4.8 GiB) filled under the launches; excludes use_hipgraph */
	int n_ctx_tok;           /* rows of the text context: 77 x W for a prompt of W 75-token windows (W <= 4); 0 = 77 */
	/* (`control` lies in what was the structure's tail padding: the Python mirror keeps the layout before it as engine.AmdConfig and adds engine.AmdControlConfig,
	 * of the same size.  A field added after it grows the structure: both mirrors then have to follow, and the size equality tests/test_controlnet_cpu.py asserts goes) */
	int control;             /* flags, MLIS_AMD_CONTROL_*.  bit 0 (_NET): the engine holds a ControlNet (hint plan, ControlNet plan, UNet plan with control inputs);
	                          * bit 1 (_FREEU): the UNet plan runs the FreeU passes at its decoder concatenations (mlis_amd_set_freeu);
	                          * bit 2 (_HYPERTILE): HyperTile, with the tile in units of 8 px in bits 8..20 and the depth in bits 24..25 (MLIS_AMD_CONTROL_HYPERTILE_OF builds
	                          * all three; mlis_amd_hypertile_info); bit 3 (_PAG): perturbed-attention guidance, the UNet plan carries a third row group (mlis_amd_set_pag);
	                          * 0: every plan as without this field */
} MLIS_AmdConfig;
enum { MLIS_AMD_CONTROL_NET = 1, MLIS_AMD_CONTROL_FREEU = 2, MLIS_AMD_CONTROL_HYPERTILE = 4, MLIS_AMD_CONTROL_PAG = 8 };
/* the bits of `control` for HyperTile with a tile of tile_px pixels (32 .. 8192, a multiple of 8) down to UNet depth `depth` (0 .. 3); tile_px 0: no bits */
#define MLIS_AMD_CONTROL_HYPERTILE_OF(tile_px, depth) ((tile_px) > 0 ? (MLIS_AMD_CONTROL_HYPERTILE | ((((tile_px) / 8) & 0x1FFF) << 8) | (((depth) & 3) << 24)) : 0)
#define MLIS_AMD_CONTROL_HYPERTILE_PX(control)    ((((control) >> 8) & 0x1FFF) * 8)
#define MLIS_AMD_CONTROL_HYPERTILE_DEPTH(control) (((control) >> 24) & 3)

/* progress callback (MLIS_Callback, include/mlimgsynth.h:405): called after every COMPLETED step (the stream is
 * synchronised first); a negative return aborts the generation and is returned by mlis_amd_denoise/generate */
typedef int (*mlis_amd_progress_fn)(void* user, int step, int n_step, int nfe);

MLIS_AmdCtx* mlis_amd_create(const MLIS_AmdConfig* cfg, void* stream);        /* = mlis_amd_create_ex(cfg, 0, stream) */
/* seamless tiling: every spatial convolution of the UNet, decoder and encoder plans pads circularly (mlctx_set_conv_wrap): 0 none, 1 x (left and right edges
 * meet), 2 y, 3 xy.  The tiled KL-VAE plans (mlis_amd_set_vae_tile) do not wrap: tiles cannot see the opposite edge. */
MLIS_AmdCtx* mlis_amd_create_ex(const MLIS_AmdConfig* cfg, int tiling, void* stream);
int mlis_amd_tiling(const MLIS_AmdCtx* S);
/* Tiled diffusion (MultiDiffusion): cfg->width x height is the CANVAS (sampler state, noise, mask, decoder, encoder), the UNet plan is built for one window of
 * min(tile, canvas) per axis.  Every evaluation cuts the canvas into overlapping windows (mlis_amd_window_starts per axis, row-major, y outer), runs the plan on each
 * -- window j of every image of the batch in one evaluation -- and blends the raw outputs by a weighted average (mlsd_window_blend) before the CFG mix; the solvers
 * never notice.  tile_w, tile_h, overlap in pixels: multiples of 8, 2 x overlap <= tile.  tile 0, or a tile that covers the canvas on both axes: mlis_amd_create_ex.
 * With `tiling`, the plan's convolutions wrap only along an axis its window spans; along the others the windows form a ring and one straddles the seam.
 * use_hipgraph and unet_split work (with unet_split every plan evaluation streams the weights again).
 * _packed: up to `pack` (1 .. MLSD_WINDOW_MAX_PACK = 16) windows of one evaluation run as ONE plan evaluation.  With the effective pack P of mlis_amd_tile_pack the
 * UNet plan is that of a plain engine for P x n_batch images with the shared prompt (activation memory included), the windows are evaluated in groups of P in their
 * order, the unused slots of a short last group repeat its last window, and the blend is the one of P = 1 bit for bit given the same plan outputs.  Everything else
 * -- sampler state, noise, RNG streams, codecs, callback, NFE count -- keeps the canvas batch.  mlis_amd_create_tiled is pack = 1. */
MLIS_AmdCtx* mlis_amd_create_tiled(const MLIS_AmdConfig* cfg, int tiling, int tile_w, int tile_h, int overlap, void* stream);
MLIS_AmdCtx* mlis_amd_create_tiled_packed(const MLIS_AmdConfig* cfg, int tiling, int tile_w, int tile_h, int overlap, int pack, void* stream);
/* the pack rule (pure): P0 = min(pack, n_win, 16, 64 / n_batch), *n_eval = ceil(n_win / P0) plan evaluations per UNet evaluation, returns P = ceil(n_win / *n_eval);
 * -1 for pack, n_win or n_batch below 1.  _info: the values of an engine; a plain engine reports 0, 1. */
int mlis_amd_tile_pack(int n_win, int n_batch, int pack, int* n_eval);
int mlis_amd_tile_pack_info(const MLIS_AmdCtx* S, int* pack, int* n_eval);
/* window starts along one axis: canvas extent L, window extent T, minimum overlap O (latent pixels), wrap != 0: the canvas tiles along the axis.  T >= L: one window
 * at 0.  Else n = ceil((L - O) / (T - O)) windows at floor(i (L - T) / (n - 1)), or on a wrapped axis n = ceil(L / (T - O)) at floor(i L / n), window i covering
 * (starts[i] + k) mod L.  Returns n; -1 for O < 0, 2 O > T, T < 1, L < 1 or n > cap. */
int mlis_amd_window_starts(int L, int T, int O, int wrap, int* starts, int cap);
int mlis_amd_tile_info(const MLIS_AmdCtx* S, int* n_win, int* win_w, int* win_h);   /* windows per evaluation (0 = not tiled), window size in latent pixels; any may be NULL */
int mlis_amd_tile_windows(const MLIS_AmdCtx* S, int* xs, int* ys, int cap);          /* start of every window in evaluation order (latent pixels); returns the count */
/* one evaluation, for tests and tools: x host [B][4][lh][lw], dx = dxdt(x, sigma) host (UNet evaluation + CFG mix + v-prediction rescale, as one solver stage sees
 * it).  Needs the conditioning; plain and tiled engines alike; the engine's latent is not touched. */
int mlis_amd_dxdt(MLIS_AmdCtx* S, const float* x_host, float sigma, float* dx_host);
void mlis_amd_destroy(MLIS_AmdCtx* S);
/* conditioning for the whole batch (shared prompt, as generate.sh): cond/uncond [n_ctx_tok][n_ctx] fp32 host (77 rows unless the config says otherwise),
 * label/unlabel [adm] or NULL */
int mlis_amd_set_cond(MLIS_AmdCtx* S, const float* cond, const float* label, const float* uncond, const float* unlabel);
/* device-resident variant used after an RCCL broadcast: pointers are DEVICE pointers of the same shapes */
int mlis_amd_set_cond_device(MLIS_AmdCtx* S, const void* cond, const void* label, const void* uncond, const void* unlabel);
/* runs the denoising loop for n_batch images with seeds[i] (offset 0 per image, src/generate.sh:56-59
 * semantics) and decodes; everything is enqueued on the stream, the call returns after the final sync.
 * latents_out [n][4][lh][lw] and/or images_out [n][3][h][w] (host, may be NULL) */
int mlis_amd_generate(MLIS_AmdCtx* S, const uint64_t* seeds, float* latents_out, float* images_out);
int mlis_amd_set_callback(MLIS_AmdCtx* S, mlis_amd_progress_fn fn, void* user);
/* change the sampler options between generations (plans and weights stay); 0 / negative values = the reference's defaults */
int mlis_amd_set_sampler(MLIS_AmdCtx* S, int n_step, int method, int sched, float cfg_scale, float s_ancestral, float s_noise,
	float f_t_ini, float f_t_end);
/* per-image Philox streams (seed_i, offset 0).  mlis_amd_denoise/generate with seeds == NULL continue the streams, like the
 * reference's never-reset g_rng (src/ccommon/rng_philox.c:50) */
int mlis_amd_seed(MLIS_AmdCtx* S, const uint64_t* seeds);
int mlis_amd_seed_ex(MLIS_AmdCtx* S, const uint64_t* seeds, uint32_t offset);    /* resume streams at a Philox offset */
uint32_t mlis_amd_rng_offset(const MLIS_AmdCtx* S);                           /* calls made so far on every stream */
/* img2img / in-painting inputs (MLIS_TUF_LATENT / MLIS_TUF_LMASK, src/mlimgsynth.c:1652-1687): initial latent host NCHW
 * [n][4][lh][lw] (consumed by the next denoise), latent mask host [lh][lw] (1 = keep the original; NULL clears) */
int mlis_amd_set_init_latent(MLIS_AmdCtx* S, const float* latent);
int mlis_amd_set_lmask(MLIS_AmdCtx* S, const float* lmask);
/* mlis_image_encode (src/mlimgsynth.c:1301-1330): images host NCHW [n][3][h][w] in [0,1] -> resident latent (VAE: sampled
 * when sample != 0 with one Philox call per image, else the mean; TAE: direct), marked as the next initial latent */
int mlis_amd_encode(MLIS_AmdCtx* S, const float* images, int sample);
MLCtx* mlis_amd_encoder_ctx(MLIS_AmdCtx* S);                                /* NULL before the first encode / prepare */
MLCtx* mlis_amd_encoder_prepare(MLIS_AmdCtx* S);
MLCtx* mlis_amd_ctx_at(MLIS_AmdCtx* S, int i);     /* every plan of the engine: 0 UNet, 1 decoder, 2 encoder, 3 tile decoder, 4 tile encoder, 5 ControlNet, 6 hint block; NULL where there is none */
/* ControlNet (engines created with MLIS_AmdConfig.control = 1; without a control image they behave as at strength 0).
 * set_control_image: host NCHW [3][height][width] in [0,1] at the canvas's pixel size, shared by the batch; runs the hint plan; NULL clears the image.  _device: the
 * same from device memory.  set_control: strength in [0, 2] (default 1) and the step window 0 <= start <= end <= 1 (default 0, 1), else an error; both may change
 * between generations without touching a plan (the gain is device data: also under use_hipgraph).
 * control_active (pure): 1 iff start n_step <= i_step + 0.5 < end n_step; both evaluations of a 2-NFE step share their step's answer, mlis_amd_dxdt has no step and is
 * always controlled.  In a controlled evaluation with strength > 0 the ControlNet plan runs before the UNet plan (per window group on a tiled engine, on the
 * group's crops of the hint embedding); otherwise it is skipped and the gain is 0.
 * control_info: residuals of the ControlNet plan (0: none) and the evaluations of the last denoise / dxdt in which it ran. */
int mlis_amd_set_control_image(MLIS_AmdCtx* S, const float* hint);
int mlis_amd_set_control_image_device(MLIS_AmdCtx* S, const void* hint_dev);
int mlis_amd_set_control(MLIS_AmdCtx* S, float strength, float start, float end);
int mlis_amd_control_active(int i_step, int n_step, float start, float end);
int mlis_amd_control_info(const MLIS_AmdCtx* S, int* n_residuals, int* evals_controlled);
/* a caller's mark on the image the engine holds (0 after every set_control_image*, and without an image): a caller that sets the same image per generation can skip it */
void mlis_amd_control_tag_set(MLIS_AmdCtx* S, uint64_t tag);
uint64_t mlis_amd_control_tag(const MLIS_AmdCtx* S);
const void* mlis_amd_control_image_device(MLIS_AmdCtx* S);   /* the control image the hint plan read: device NCHW fp32 [3][height][width], NULL without one */
/* the same copied to the host: host_dst (may be NULL) gets [3][height][width] floats, *w and *h (may be NULL) the size.  Returns 1, 0 when no image is held, -1 on a copy error */
int mlis_amd_control_image_get(const MLIS_AmdCtx* S, float* host_dst, int* w, int* h);
/* FreeU (engines created with MLIS_AMD_CONTROL_FREEU in MLIS_AmdConfig.control).  set_freeu: the backbone factors b1, b2 and the skip factors s1, s2 of stage 1
 * (backbone of n_ch x the top multiplier channels) and stage 2 (half of that), each in [0, 4], else an error; they are four floats of device memory, so they change
 * between generations, and under use_hipgraph, without touching a plan.  All four start at 1: until they are set the engine computes what one without the flag does.
 * freeu_info: the decoder concatenations the plan treats at each stage (0, 0 without the flag).  Tiled and packed engines apply FreeU per window plan evaluation:
 * the channel-mean map is normalised, and the skip planes are filtered, over the window, as an untiled evaluation of that window would. */
int mlis_amd_set_freeu(MLIS_AmdCtx* S, float b1, float b2, float s1, float s2);
int mlis_amd_freeu_info(const MLIS_AmdCtx* S, int* n_stage1, int* n_stage2);
/* HyperTile (engines created with MLIS_AMD_CONTROL_HYPERTILE_OF(tile_px, depth) in MLIS_AmdConfig.control; not in the reference).  Inside a spatial transformer
 * everything between proj_in and proj_out is per token except the self-attention, so the token rows are brought into tile-major order once at the block's entry and
 * back once at its exit (mlsd_tile_permute on the fp16 operands of proj_in and proj_out), and every self-attention in between is the launch it always was with
 * images x tiles batches of th tw tokens.  Cross-attention, convolutions, norms and Linear layers see what they saw.
 * hypertile_side: the tile's side, in tokens, on an axis of `side` tokens at px_per_token image pixels per token (8 x the UNet downscale): with
 * m = min(max(tile_px / px_per_token, 4), side) (integer division; the floor of 4 tokens keeps degenerate tiles out), the smallest divisor of side that is >= m.
 * Pure, host.  A level of h x w tokens at downscale ds is TILED when (side(h), side(w)) != (h, w) and log2(ds) <= depth; a level that is not gets no ops at all.
 * This is the published rule with its random choice among the divisors (swap_size) fixed to the first, written from memory: parity with the published code is not
 * pinned by a test.  The rule is applied to the UNet plan's own size: tiled-diffusion engines apply it to their window, and the ControlNet's encoder copy follows it.
 * hypertile_info: the UNet plan's spatial transformers that are tiled / not tiled, and th, tw, nh, nw for each depth 0..3 (zeros where the depth is not tiled);
 * (0, all, zeros) for an engine without the flag.  Any of the three pointers may be NULL.  Returns 1.
 * unet_hypertile_cuts: how many spatial transformers of a UNet plan of lw x lh latent pixels the setting tiles (pure, host; the walk of the plan builder, held to
 * built plans by tests/test_hypertile_cpu.py); mlis_generate takes the plain engine under the plain key for a pass where it is 0.
 * The permuted rows are the dense fp16 operands of proj_in and proj_out, whole 16-byte pieces: the channel counts of a spatial transformer are multiples of 32
 * (its GroupNorm), so this always holds; a plan builder that asked for a tiled level on rows that are not is refused with an error, the level is not left whole. */
int mlis_amd_hypertile_side(int side, int px_per_token, int tile_px);
int unet_hypertile_cuts(const UnetParams* P, int lw, int lh, int tile_px, int depth);
int mlis_amd_hypertile_info(const MLIS_AmdCtx* S, int* n_tiled, int* n_untiled, int tiles[4][4]);
/* Perturbed-attention guidance, PAG (engines created with MLIS_AMD_CONTROL_PAG in MLIS_AmdConfig.control; "Self-Rectifying Diffusion Sampling with
 * Perturbed-Attention Guidance", 2024; not in the reference).  The rule, as recalled from the publication and the front ends that ship it -- parity with the published
 * code is NOT pinned by a test, the rule below is:
 *   - beside the cond (and, at cfg_scale > 1, uncond) evaluation the UNet is evaluated once more per image on the cond row's inputs (latent, timestep, context, label),
 *     with softmax(q k^T) v replaced by v in the self-attentions (attn1) of the MIDDLE block's spatial transformer: attn1(x) = out_proj(v_proj(x)).  Cross-attention,
 *     the feed-forwards and every other block are what they are;
 *   - with c, u, p the cond, uncond and perturbed outputs (after the v-prediction rescale where the model has one): dx = g + pag_scale (c - p), g the plain mix
 *     (c f + u (1 - f), or c at cfg_scale <= 1).  So it also guides where CFG does nothing.
 * Here it is a third group of B rows in the one batched plan, not a second pass: an evaluation has mlis_amd_eval_rows(B, cfg_scale, pag) rows
 * [cond B | uncond B (cfg_scale > 1) | perturbed B], every writer of the plan's inputs fills the last group with the cond group's values, and only mid.1 differs: its
 * fused q|k|v projection and its attention launch cover the other groups, one more GEMM on the v_proj slice of the fused weight (no new parameter: checkpoints,
 * LoRAs and weight streaming see what they saw) writes the perturbed group's rows of the buffer out_proj reads.  HyperTile keeps working (images are contiguous row
 * runs in tile-major order too); the ControlNet's encoder copy is never perturbed, its plan holds the other groups and the UNet plan's sums hand the perturbed group
 * the cond group's residuals; tiled and packed engines blend three groups (the mix is affine in eps).  An engine whose rows per plan evaluation exceed what a plain
 * engine may hold (128) is refused at creation.
 * set_pag: the scale, 0 .. 20, else an error; a field of the engine handed to the mix kernels (mlsd_dxdt_guided, mlsd_euler_guided_update: the ones every engine runs) by value, so it changes between
 * generations, and under use_hipgraph, without touching a plan.  Engines start at 0, where the flag alone computes what the plain mix does (the third group is
 * evaluated and not read).  pag_info: the perturbed self-attentions of the UNet plan (0 without the flag) and the rows of one evaluation.
 * Not included: layer selections other than the middle block; a step window or an adaptive scale (a plan is fixed: outside a window the perturbed rows would still be
 * computed, and saving them needs a plain plan beside this one on one set of weights); self-attention guidance.  (Guidance rescale: mlis_amd_set_cfg_rescale.) */
#define MLIS_AMD_MAX_EVAL_ROWS 128        /* rows of one plan evaluation: what a plain engine of the largest batch holds (2 x 64) */
int mlis_amd_eval_rows(int B, float cfg_scale, int pag);
int mlis_amd_set_pag(MLIS_AmdCtx* S, float scale);
int mlis_amd_pag_info(const MLIS_AmdCtx* S, int* n_attn, int* rows);
/* Prediction type, zero-terminal-SNR schedule and guidance rescale ("Common Diffusion Noise Schedules and Sample Steps are Flawed", 2023; not in the reference): what
 * a v-prediction SDXL checkpoint trained on the rescaled schedule needs.  All three are fields of the engine handed over per generation, as mlis_amd_set_pag hands
 * over its scale: none is in a plan or in the engine key, none rebuilds or recaptures anything, and at their defaults no new code runs.
 *   set_prediction: vparam 1 = the mix maps the output through out*c_out + x*c_skip (0: eps), zsnr 1 = schedule and sigma <-> t read the second table
 *     (unet_log_sigmas); negative = the model type's own.  With zsnr the uniform schedule starts at the clamped last entry, sigma 4518.76: c_in = 1/sqrt(sigma^2 + 1) is
 *     applied to the fp32 latent by the kernel that writes the plan's fp16 input, c_skip and c_out are formed in fp32 as ever, and t = 999 is an ordinary timestep.
 *     Karras with zsnr spends its steps between 4518 and sigma_min: allowed, the user's choice.  No trailing / SGM spacing here.
 *   set_cfg_rescale: phi 0 .. 1 (0 = off; front ends use 0.7).  Where phi > 0 and the guided prediction differs from the cond one (cfg_scale > 1, or PAG with a scale),
 *     dxdt_finish and the fused Euler step run mlsd_guidance_stats on the raw outputs (of a tiled engine: the blended canvas, so the statistics are the whole image's)
 *     and hand its factors to mlsd_dxdt_guided / mlsd_euler_guided_update: three launches per mix.  The hires fix rescales in both passes; the statistics are per image, so a
 *     multi-GPU split needs no communication.
 *   guidance_info: the resolved values, the sigma range, phi, the rescaled mixes so far and the last mix's factors (returns how many were written).
 * prediction_resolve: the pure rule of the `prediction` / `zsnr` options.  opt_prediction 0 auto, 1 eps, 2 v; opt_zsnr 0 auto, 1 off, 2 on; ckpt_v_pred / ckpt_ztsnr:
 * the checkpoint carries a tensor named "v_pred" / "ztsnr" (mlts_markers; the published v-pred SDXL checkpoints' marker convention AS RECALLED, parity-unpinned).
 * auto = sd2 and tinyv are v, a v_pred marker makes any model v, everything else eps; the second table only with a ztsnr marker.  Explicit values always win. */
int mlis_amd_set_prediction(MLIS_AmdCtx* S, int vparam, int zsnr);
int mlis_amd_set_cfg_rescale(MLIS_AmdCtx* S, float phi);
int mlis_amd_guidance_info(MLIS_AmdCtx* S, int* vparam, int* zsnr, float* sigma_min, float* sigma_max, float* phi, int* n_evals, float* factors, int max_factors);
int mlis_amd_last_rows(MLIS_AmdCtx* S, float* out, size_t nbytes);      /* the raw outputs the last mix read, host [N][4][hw] (tests, tools) */
int mlis_amd_prediction_resolve(const char* model, int ckpt_v_pred, int ckpt_ztsnr, int opt_prediction, int opt_zsnr, int* vparam, int* zsnr);
/* VAE tiling (MLIS_OPT_VAE_TILE, src/vae.c:245-300,333-391): tile size in pixels (rounded up to 64; 0 = off).  Decode / encode then
 * run tile by tile through tile-sized plans; *_tile_prepare build them (NULL when tiling does not apply: TAE, or one tile covers all).
 * set_vae_tile with another size drops the tile plans AND the tile-sized buffers; the next prepare makes them for the new tile.
 * The tile plans take one image; a batch walks them image by image (tile buffers hold every image's tile), so an image's result does not depend on the batch size.
 * A deliberate extension of the reference: a dimension that one tile covers while the other is tiled (512 x 768 at vae_tile 512: the latent is 64 wide, a tile
 * 80) is one tile pasted whole.  The reference pastes only the tile less its margin there and leaves the last 64 pixel columns of the image (8 of the moments)
 * unwritten, divides by zero at exactly 128 pixels and runs no tile below; every pixel it does write has the same bits here.  Tiles the reference evaluates twice
 * (its count ceil(full / step) repeats the last, clamped origin) run once: same values on the same pixels.
 * vae_tile_walk: the walk of one dimension that decode and encode share (lengths in units of `unit` image pixels: f over the latent, 1 over the image; margin 8
 * resp. 8 f); tile t reads [origin, origin + n) and pastes [src_off, src_off + width) of its result at origin + src_off.  Returns the number of tiles.
 * vae_tile_info: tile size, allocated bytes of the tile's input / output buffer, tiles per pass and plan evaluations of the last tiled pass of the decode (which 0)
 * or encode (which 1) tile plan; returns 1 with a plan, 0 without. */
int mlis_amd_set_vae_tile(MLIS_AmdCtx* S, int tile_px);
MLCtx* mlis_amd_decoder_tile_prepare(MLIS_AmdCtx* S);
MLCtx* mlis_amd_encoder_tile_prepare(MLIS_AmdCtx* S);                            /* build the encoder plan now (weights: synth or caller-loaded) */
int mlis_amd_vae_tile_walk(int full, int tile_px, int unit, int margin, int* n_out, int* origin, int* src_off, int* width, int max_tiles);
int mlis_amd_vae_tile_info(MLIS_AmdCtx* S, int which, int* tile_w, int* tile_h, size_t* in_bytes, size_t* out_bytes, int* n_tiles, int* n_evals);
int mlis_amd_last_n_step(MLIS_AmdCtx* S);
/* passes (denoising loop, decode, encode) that were run AGAIN on the hand-off-free plan after an in-launch hand-off (stream-K slab, LayerNorm statistics) timed out --
 * the GPU was shared or the stream CU-masked.  The call that hit it still succeeds; results then come from plain tiles / separate LayerNorm launches. */
int mlis_amd_handoff_retries(const MLIS_AmdCtx* S);
/* pieces, for tests and for the multi-GPU driver */
int mlis_amd_denoise(MLIS_AmdCtx* S, const uint64_t* seeds);               /* latent stays on device */
int mlis_amd_decode(MLIS_AmdCtx* S);                                        /* image stays on device; asynchronous UNLESS the decoder plan hands data over inside launches
                                                                             * (stream-K tiles: the SDXL VAE has them): then the stream is drained here to check the hand-offs */
int mlis_amd_sync(MLIS_AmdCtx* S);                                          /* wait for the engine's stream */
void* mlis_amd_latent_device(MLIS_AmdCtx* S);                               /* fp32 NCHW [n][4][lh][lw] */
void* mlis_amd_image_device(MLIS_AmdCtx* S);                                /* fp32 NCHW [n][3][h][w] */
/* multi-GPU exchange steps over RCCL (mlsd_rccl_* communicator): conditioning broadcast from `root` into the plan's inputs;
 * all-gather of the final latents (what 0) or images (what 1) into recv_dev [world][per-rank bytes] */
int mlis_amd_bcast_cond(MLIS_AmdCtx* S, void* comm, int root);
int mlis_amd_gather_results(MLIS_AmdCtx* S, void* comm, int what, void* recv_dev);
int mlis_amd_info(MLIS_AmdCtx* S, double* unet_flops_per_eval, double* decode_flops, int* unet_ops, size_t* mem_params,
	size_t* mem_compute);
MLCtx* mlis_amd_unet_ctx(MLIS_AmdCtx* S);
MLCtx* mlis_amd_decoder_ctx(MLIS_AmdCtx* S);
/* time of the last mlis_amd_denoise spent in UNet evaluations, measured with HIP events on the stream (ms) */
float mlis_amd_last_unet_ms(MLIS_AmdCtx* S);
int mlis_amd_last_nfe(MLIS_AmdCtx* S);

#ifdef __cplusplus
}
#endif
