/* The public libmlimgsynth API (include/mlis_abi.h == the reference's include/mlimgsynth.h:414-571) on the MI355X engine.
 * Re-creation of the slices of src/mlimgsynth.c that sit on the hot path:
 *   context + options        mlis_ctx_create_i :446-478, mlis_option_set[_str] :787-949 + mlimgsynth_options_set.c.h
 *   setup                    mlis_setup :1250-1299 (backend, model header, identification, weight type)
 *   conditioning             mlis_text_tokenize :1405-1421, mlis_clip_tokens_encode :1423-1468, mlis_text_cond_encode :1501-1563
 *   generation               mlis_generate :1634-1773, mlis_image_get :1775-1793, mlis_infotext_update :1589-1632
 *   codec / tensors          mlis_image_encode/decode :1301-1357, mlis_mask_encode :1359-1365, MLIS_Tensor helpers
 * What differs by design: the graphs, weights and CLIP towers stay RESIDENT between generations (the reference rebuilds
 * and re-uploads them inside every mlis_generate); BATCH_SIZE > 1 works (image i uses seed + i, generate.sh:56-59);
 * the CLIP vocabulary is data found through AUX_DIR (the reference compiles src/clip_merges.c.h in); MODEL may be
 * "synth:<sd1|sd2|sdxl|tiny|tinyxl|tinyv>[:seed]" for the synthetic-weight models used by the benchmark and the tests.
 * LoRA files (kohya naming) are merged into the weights at load time on the host (src/lora.c:9-138) when nothing is resident yet; a change of the LoRA set or of a
 * multiplier while engines or text towers are resident patches their weights in place on the GPU, with the host merge's arithmetic (loras_apply_warm).
 */
#include "mlblock_int.h"
#include "mlimgsynth_amd.h"
#include "mlis_abi.h"
#include <ctype.h>
#include <math.h>
#include <stdarg.h>
#include <time.h>
#include <inttypes.h>
#include <sys/stat.h>

#define CTX_SIGNATURE 0x4d4c4953u
enum { CF_USE_TAE = 1, CF_NO_DECODE = 2, CF_NO_PROMPT_PARSE = 4, CF_UNET_SPLIT = 8, CF_WEIGHT_TYPE_SET = 16, CF_MODEL_TYPE_SET = 32 };
enum { READY_BACKEND = 1, READY_MODEL = 2, READY_LORAS = 4 };
enum { LF_PROMPT = 1 };
#define MAX_LORAS 32
#define LT_F_OWNMEM 1      /* src/localtensor.h:22-27 */
#define LT_F_READY 2
#define N_TMP_TENSORS 4
#define MAX_IMAGES 64

struct MLIS_Ctx {
	uint32_t signature;
	/* options (struct c of the reference's MLIS_Ctx, src/mlimgsynth.c:360-395) */
	char *backend, *path_model, *path_tae, *path_aux, *path_lora_dir, *prompt_raw, *nprompt_raw;
	MLISPrompt prompt, nprompt;
	int32_t *ptok[2]; float *ptokw[2]; int n_ptok[2], have_ptok[2];     /* mlis_amd_prompt_tokens_set */
	int model_type, width, height, n_batch, clip_skip, vae_tile, n_thread, dump_flags, flags, tuflags, wtype;
	int tiling;             /* MLIS_OPT_AMD_TILING: 0 none, 1 x, 2 y, 3 xy */
	float hires_scale, hires_denoise; int hires_steps, hires_upscaler;      /* MLIS_OPT_AMD_HIRES_*: the two-pass generation of mlis_generate */
	int unet_tile, unet_tile_overlap;       /* MLIS_OPT_AMD_UNET_TILE*: tiled diffusion, pixels; 0 = off, overlap -1 = auto */
	int tiled_tile, tiled_overlap;          /* of the last generation, if one of its passes was tiled (infotext) */
	/* MLIS_OPT_AMD_CONTROL_*: the ControlNet file (or "synth[:seed]"), the control image as given (any size; resampled per pass), strength and step window */
	char *path_control; MLTStore *ts_control;
	MLIS_Tensor control_image;
	uint64_t control_image_gen;             /* counts the control images set: the mark an engine keeps on the one it holds (never 0 once an image is set) */
	float control_strength, control_start, control_end;
	int control_evals[2], control_pass;     /* controlled evaluations of the last generation's passes (mlis_amd_control_evals) */
	char *path_upscale; MLIS_AmdUpscaler *upscaler;       /* MLIS_OPT_AMD_UPSCALE_MODEL and the resident upscaler built from it (dropped whenever the option changes) */
	int n_upscaler_builds, hires_use_model;                                     /* mlis_amd_upscaler_builds; MLIS_OPT_AMD_HIRES_USE_MODEL */
	int downscale_filter;   /* MLIS_OPT_AMD_DOWNSCALE_FILTER: 0 none, else MLIS_AMD_AA_* + 1: the filter of the resamples that shrink (hires model path, control image) */
	int control_preprocess; float canny_low, canny_high; int canny_l2;   /* MLIS_OPT_AMD_CONTROL_PREPROCESS (MLIS_AMD_PREPROCESS_*) and MLIS_OPT_AMD_CANNY_*: what control_apply runs behind its resample */
	/* MLIS_OPT_AMD_INPAINT_* / MASK_*: region inpainting (generate_inpaint); the rectangle and processing size of the last generation (mlis_amd_inpaint_info) */
	int inpaint_area, inpaint_padding, mask_grow, mask_invert, inpaint_composite; float mask_blur;
	int inp_region[4], inp_proc[2], inp_done;
	int control_rect_on, control_rect[4], control_rect_W, control_rect_H;      /* the region a masked pass hands to control_apply, of an image of that size */
	int freeu; float freeu_f[4];            /* MLIS_OPT_AMD_FREEU*: on / off (part of the engine key) and b1, b2, s1, s2 (device data of the engine: never rebuild anything) */
	float cfg_rescale;                      /* MLIS_OPT_AMD_CFG_RESCALE: phi of the guidance rescale, handed to the engine per generation (never part of the engine key) */
	int prediction, zsnr;                   /* MLIS_OPT_AMD_PREDICTION (0 auto, 1 eps, 2 v) / MLIS_OPT_AMD_ZSNR (0 auto, 1 off, 2 on): resolved per generation (guidance_resolve) */
	int ckpt_v_pred, ckpt_ztsnr;            /* the checkpoint's marker tensors (mlts_markers); 0 for the synthetic models */
	float pag_scale;                        /* MLIS_OPT_AMD_PAG_SCALE: > 0 is part of the engine key as on / off; the value is handed to the engine per generation */
	int hypertile, hypertile_depth;         /* MLIS_OPT_AMD_HYPERTILE*: tile in pixels (0 = off) and deepest tiled UNet level; both part of the engine key */
	int unet_tile_batch, tiled_pack;        /* MLIS_OPT_AMD_UNET_TILE_BATCH: at most this many windows per plan evaluation; the effective pack of the last tiled pass (infotext) */
	float cfg_scale;
	int method, sched, n_step;
	float f_t_ini, f_t_end, s_noise, s_ancestral;
	uint64_t seed; uint32_t rng_offset;
	MLIS_Callback callback; void* callback_ud;
	MLIS_ErrorHandler errh; void* errh_ud;
	/* state */
	int rflags;
	struct { char* path; float mult; int flags; } loras[MAX_LORAS]; int n_lora;
	/* what the weights reflect: the adapters merged into S->ts (ts_merged) or patched into the resident plans on the device, in order; the keys they patched */
	struct { char* path; float mult; } applied[MAX_LORAS]; int n_applied;
	char** lkeys; int n_lkeys, cap_lkeys;
	int ts_merged;          /* S->ts holds host-merged tensors: plans built from it need no patch; 0: S->ts is the checkpoint, new plans are loaded and then patched */
	int ts_partial;         /* a host merge failed midway: S->ts is neither */
	int n_lora_restored, n_lora_patched, n_lora_cold;      /* mlis_amd_lora_stats */
	char mname[16];
	uint64_t synth_seed; int synth;
	MLTStore *ts, *ts_tae;
	MLIS_AmdCtx* eng; char eng_key[96];       /* the engine used last */
	MLIS_AmdCtx* eng2; char eng2_key[96];     /* the one used before it (engine_get): a two-size workflow rebuilds nothing */
	int n_eng_builds;
	int ctx_tok;            /* rows of the conditioning the engine is built for: 77 W (windowed prompt); 0 = 77 */
	MLIS_AmdTextCond* tc; char tc_key[64];
	ClipTokenizer* tok;
	MLIS_Tensor image, mask, latent, lmask, cond, label, ncond, nlabel, tmp[N_TMP_TENSORS];
	MLIS_Image imgex[MAX_IMAGES];
	MLIS_BackendInfo backend_info; struct MLIS_BackendDeviceInfo devs[16]; char dev_names[16][2][96];
	MLIS_Progress prg; double t_last;
	char errstr[600];
	char* infotext;
	int32_t* tokens; float* tokens_w; int n_tokens;
	int last_n_step, last_nfe;      /* of the generation as the infotext reports it: after a hires generation the steps of its FIRST pass ("Steps:") and the evaluations of both */
	int nfe_base;           /* evaluations of the first hires pass while the second one runs: progress and last_nfe count both */
};

/* ------------------------------------------------------------------ small helpers */
static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + ts.tv_nsec*1e-9; }

static void str_set(char** p, const char* s) { free(*p); *p = strdup(s ? s : ""); }
static int str_empty(const char* s) { return !s || !*s; }

static int api_error(MLIS_Ctx* S, int code, const char* fmt, ...)
{	/* ERROR_LOG + mlis_error_handle: text into errstr, the handler (if any) is called */
	va_list ap; va_start(ap, fmt); vsnprintf(S->errstr, sizeof(S->errstr), fmt, ap); va_end(ap);
	if (S->errh) { MLIS_ErrorInfo ei = { (MLIS_ErrorCode)code, S->errstr }; S->errh(S->errh_ud, S, &ei); }
	return code;
}
/* an error produced below the API (text in mlsd_last_error) */
static int api_error_lib(MLIS_Ctx* S, int code) { return api_error(S, code < 0 ? code : MLIS_E_UNKNOWN, "%s", mlsd_last_error()); }

/* identifier comparison of option / enum names: case-insensitive, '-' == '_' (mlimgsynth.h:446-451) */
static int id_eq(const char* a, size_t n, const char* b)
{
	if (strlen(b) != n) return 0;
	for (size_t i=0;i<n;++i) {
		char x = (char)tolower((unsigned char)a[i]), y = b[i];
		if (x == '-') x = '_';
		if (x != y) return 0;
	}
	return 1;
}

/* ------------------------------------------------------------------ enum <-> string tables (src/mlimgsynth.c:210-302) */
static const char* const k_stage[][2] = { {"idle","Idle"}, {"cond_encode","Conditioning encoding"}, {"image_encode","Image encoding"},
	{"image_decode","Image decoding"}, {"denoise","Denoising"} };
static const char* const k_method[] = { "none", "euler", "heun", "taylor3", "dpmpp2m", "dpmpp2s" };
static const char* const k_sched[] = { "none", "uniform", "karras" };
static const char* const k_model[][2] = { {"none","None"}, {"sd1","Stable Diffusion 1.x"}, {"sd2","Stable Diffusion 2.x"}, {"sdxl","Stable Diffusion XL"} };
static const struct { const char* n; int id; } k_loglvl[] = { {"none",0}, {"error",10}, {"warning",20}, {"info",30}, {"verbose",40}, {"debug",50}, {"max",255} };
#define COUNTOF(a) ((int)(sizeof(a)/sizeof((a)[0])))

static int from_list(const char* const* list, int n, int stride, const char* s, size_t len)
{
	for (int i=0;i<n;++i) if (id_eq(s, len, list[i*stride])) return i;
	return -1;
}
MLB_API const char* mlis_stage_str(MLIS_Stage x) { return (x >= 0 && x < COUNTOF(k_stage)) ? k_stage[x][0] : "???"; }
MLB_API const char* mlis_stage_desc(MLIS_Stage x) { return (x >= 0 && x < COUNTOF(k_stage)) ? k_stage[x][1] : "???"; }
MLB_API MLIS_Stage mlis_stage_fromz(const char* s) { return (MLIS_Stage)from_list(&k_stage[0][0], COUNTOF(k_stage), 2, s, strlen(s)); }
MLB_API const char* mlis_method_str(MLIS_Method x) { return (x >= 0 && x < COUNTOF(k_method)) ? k_method[x] : "???"; }
MLB_API MLIS_Method mlis_method_fromz(const char* s) { return (MLIS_Method)from_list(k_method, COUNTOF(k_method), 1, s, strlen(s)); }
MLB_API const char* mlis_sched_str(MLIS_Scheduler x) { return (x >= 0 && x < COUNTOF(k_sched)) ? k_sched[x] : "???"; }
MLB_API MLIS_Scheduler mlis_sched_fromz(const char* s) { return (MLIS_Scheduler)from_list(k_sched, COUNTOF(k_sched), 1, s, strlen(s)); }
MLB_API const char* mlis_loglvl_str(MLIS_LogLvl id) { for (int i=0;i<COUNTOF(k_loglvl);++i) if (k_loglvl[i].id == (int)id) return k_loglvl[i].n; return "???"; }
MLB_API MLIS_LogLvl mlis_loglvl_fromz(const char* s) { for (int i=0;i<COUNTOF(k_loglvl);++i) if (id_eq(s, strlen(s), k_loglvl[i].n)) return (MLIS_LogLvl)k_loglvl[i].id; return (MLIS_LogLvl)-1; }
static const char* const k_tiling[] = { "none", "x", "y", "xy" };
static const char* const k_resample[] = { "nearest", "bilinear", "bicubic" };
static const char* const k_downscale[] = { "none", "box", "bilinear", "bicubic", "lanczos" };            /* 0, MLIS_AMD_AA_* + 1 */
static const char* const k_preprocess[] = { "none", "canny", "invert" };                                 /* MLIS_AMD_PREPROCESS_* */
static const char* const k_prediction[] = { "auto", "eps", "v" };
static const char* const k_zsnr[] = { "auto", "off", "on" };
static const char* const k_inpaint_area[] = { "whole", "masked" };                                       /* MLIS_AMD_INPAINT_* */

static const char* model_name(int mt)
{
	switch (mt) { case MLIS_MODEL_TYPE_SD1: return "sd1"; case MLIS_MODEL_TYPE_SD2: return "sd2"; case MLIS_MODEL_TYPE_SDXL: return "sdxl";
	case MLIS_MODEL_TYPE_AMD_TINY: return "tiny"; case MLIS_MODEL_TYPE_AMD_TINYXL: return "tinyxl"; case MLIS_MODEL_TYPE_AMD_TINYV: return "tinyv"; }
	return NULL;
}
static int model_from(const char* s, size_t n)
{
	int r = from_list(&k_model[0][0], COUNTOF(k_model), 2, s, n);
	if (r >= 0) return r;
	if (id_eq(s, n, "tiny")) return MLIS_MODEL_TYPE_AMD_TINY;
	if (id_eq(s, n, "tinyxl")) return MLIS_MODEL_TYPE_AMD_TINYXL;
	if (id_eq(s, n, "tinyv")) return MLIS_MODEL_TYPE_AMD_TINYV;
	return -1;
}
MLB_API const char* mlis_model_type_str(MLIS_ModelType x) { const char *m = model_name(x); return m ? m : (x == 0 ? "none" : "???"); }
MLB_API const char* mlis_model_type_desc(MLIS_ModelType x) { return (x >= 0 && x < COUNTOF(k_model)) ? k_model[x][1] : (model_name(x) ? "test model" : "???"); }
MLB_API MLIS_ModelType mlis_model_type_fromz(const char* s) { return (MLIS_ModelType)model_from(s, strlen(s)); }

/* ------------------------------------------------------------------ MLIS_Tensor helpers (src/localtensor.h) */
MLB_API size_t mlis_tensor_count(const MLIS_Tensor* t) { return t ? (size_t)t->n[0]*t->n[1]*t->n[2]*t->n[3] : 0; }
MLB_API void mlis_tensor_free(MLIS_Tensor* t) { if (t) { if (t->flags & LT_F_OWNMEM) free(t->d); memset(t, 0, sizeof(*t)); } }
MLB_API void mlis_tensor_resize(MLIS_Tensor* t, int n0, int n1, int n2, int n3)
{
	const size_t n = (size_t)n0*n1*n2*n3;
	if (!(t->flags & LT_F_OWNMEM)) t->d = NULL;
	t->d = (float*)realloc(t->d, (n ? n : 1) * sizeof(float));
	t->n[0]=n0; t->n[1]=n1; t->n[2]=n2; t->n[3]=n3;
	t->flags |= LT_F_OWNMEM;
}
MLB_API void mlis_tensor_resize_like(MLIS_Tensor* t, const MLIS_Tensor* s) { mlis_tensor_resize(t, s->n[0], s->n[1], s->n[2], s->n[3]); }
MLB_API void mlis_tensor_copy(MLIS_Tensor* d, const MLIS_Tensor* s) { mlis_tensor_resize_like(d, s); memcpy(d->d, s->d, mlis_tensor_count(s)*sizeof(float)); }
MLB_API float mlis_tensor_similarity(const MLIS_Tensor* a, const MLIS_Tensor* b)
{	/* cosine similarity (ltensor_similarity) */
	const size_t n = mlis_tensor_count(a);
	if (n != mlis_tensor_count(b) || !n) return 0;
	double ab = 0, aa = 0, bb = 0;
	for (size_t i=0;i<n;++i) { ab += (double)a->d[i]*b->d[i]; aa += (double)a->d[i]*a->d[i]; bb += (double)b->d[i]*b->d[i]; }
	return (float)(ab / sqrt(aa * bb));
}
static int tensor_good(const MLIS_Tensor* t) { return t->d && mlis_tensor_count(t) > 0; }

static int lora_add(MLIS_Ctx* S, const char* name, size_t len, float mult, int flags);
static void loras_remove(MLIS_Ctx* S, int only_prompt);
static void options_init(MLIS_Ctx* S);       /* the initial value of every option in the table (k_opt) */

/* ------------------------------------------------------------------ context */
MLB_API MLIS_Ctx* mlis_ctx_create_i(int version)
{
	if (!(0x000400 <= version && version < 0x000500)) { mlsd_set_error(MLIS_E_VERSION, "mlis incompatible version %06x", version); return NULL; }
	unet_params_init();
	MLIS_Ctx *S = (MLIS_Ctx*)calloc(1, sizeof(*S));
	if (!S) return NULL;
	S->signature = CTX_SIGNATURE;
	S->wtype = MLT_F16;
	options_init(S);
	struct timespec ts; clock_gettime(CLOCK_REALTIME, &ts);
	S->seed = (uint64_t)ts.tv_sec * 1000 + ts.tv_nsec / 1000000;      /* g_rng.seed = timing_timeofday()*1000 (:458) */
	return S;
}

static void engine_drop(MLIS_Ctx* S)
{
	/* (the context's Philox offset is copied back after every SEEDED use of an engine -- generate / image encode -- and nowhere else:
	 * an engine that was only built for mlis_image_decode still has offset 0 and must not reset the context's running offset) */
	if (S->eng) { mlis_amd_destroy(S->eng); S->eng = NULL; S->eng_key[0] = 0; }
	if (S->eng2) { mlis_amd_destroy(S->eng2); S->eng2 = NULL; S->eng2_key[0] = 0; }
}
static int engine_has_control(MLIS_AmdCtx* e)
{	/* asked of the engine itself, not read out of its key */
	int n_res = 0;
	return e && mlis_amd_control_info(e, &n_res, NULL) > 0 && n_res > 0;
}
/* `prediction` / `zsnr` resolved against the model type and the checkpoint's markers (mlis_amd_prediction_resolve) */
static int guidance_resolve(MLIS_Ctx* S, int* vparam, int* zsnr)
{
	return mlis_amd_prediction_resolve(S->mname, S->ckpt_v_pred, S->ckpt_ztsnr, S->prediction, S->zsnr, vparam, zsnr);
}
static int engine_has_pag(MLIS_AmdCtx* e)
{
	int n = 0;
	return e && mlis_amd_pag_info(e, &n, NULL) > 0 && n > 0;
}
static int engine_has_freeu(MLIS_AmdCtx* e)
{
	int n1 = 0, n2 = 0;
	return e && mlis_amd_freeu_info(e, &n1, &n2) > 0 && n1 + n2 > 0;
}
static void control_engines_drop(MLIS_Ctx* S)
{	/* the resident engines built with a ControlNet */
	if (engine_has_control(S->eng2)) { mlis_amd_destroy(S->eng2); S->eng2 = NULL; S->eng2_key[0] = 0; }
	if (engine_has_control(S->eng)) {
		mlis_amd_destroy(S->eng); S->eng = S->eng2; memcpy(S->eng_key, S->eng2_key, sizeof(S->eng_key));
		S->eng2 = NULL; S->eng2_key[0] = 0;
	}
}
static void upscaler_drop(MLIS_Ctx* S) { if (S->upscaler) { mlis_amd_upscaler_destroy(S->upscaler); S->upscaler = NULL; } }
static void textcond_drop(MLIS_Ctx* S) { if (S->tc) { mlis_amd_textcond_destroy(S->tc); S->tc = NULL; S->tc_key[0] = 0; } }
static void applied_clear(MLIS_Ctx* S)
{
	for (int i=0;i<S->n_applied;++i) free(S->applied[i].path);
	S->n_applied = 0;
}
static void lkeys_clear(MLIS_Ctx* S) { for (int i=0;i<S->n_lkeys;++i) free(S->lkeys[i]); S->n_lkeys = 0; }
static void lkey_add(MLIS_Ctx* S, const char* key)
{
	for (int i=0;i<S->n_lkeys;++i) if (!strcmp(S->lkeys[i], key)) return;
	if (S->n_lkeys == S->cap_lkeys) { S->cap_lkeys = S->cap_lkeys ? S->cap_lkeys*2 : 64; S->lkeys = (char**)realloc(S->lkeys, sizeof(char*) * (size_t)S->cap_lkeys); }
	S->lkeys[S->n_lkeys++] = strdup(key);
}
static void lora_state_reset(MLIS_Ctx* S) { applied_clear(S); lkeys_clear(S); S->ts_merged = S->ts_partial = 0; }

static void model_drop(MLIS_Ctx* S)
{
	engine_drop(S); textcond_drop(S);
	lora_state_reset(S);
	if (S->ts) { mlts_close(S->ts); S->ts = NULL; }
	if (S->ts_tae) { mlts_close(S->ts_tae); S->ts_tae = NULL; }
	S->rflags &= ~READY_MODEL;
}

MLB_API void mlis_ctx_destroy(MLIS_Ctx** pctx)
{
	if (!pctx || !*pctx) return;
	MLIS_Ctx *S = *pctx;
	if (S->signature != CTX_SIGNATURE) return;
	model_drop(S);
	if (S->tok) clip_tokr_free(S->tok);
	upscaler_drop(S); free(S->path_upscale);
	free(S->path_control); if (S->ts_control) mlts_close(S->ts_control); mlis_tensor_free(&S->control_image);
	free(S->backend); free(S->path_model); free(S->path_tae); free(S->path_aux); free(S->path_lora_dir); free(S->prompt_raw); free(S->nprompt_raw);
	mlis_prompt_free(&S->prompt); mlis_prompt_free(&S->nprompt);
	for (int i=0;i<2;++i) { free(S->ptok[i]); free(S->ptokw[i]); }
	MLIS_Tensor *ts[] = { &S->image, &S->mask, &S->latent, &S->lmask, &S->cond, &S->label, &S->ncond, &S->nlabel };
	for (int i=0;i<8;++i) mlis_tensor_free(ts[i]);
	for (int i=0;i<N_TMP_TENSORS;++i) mlis_tensor_free(&S->tmp[i]);
	for (int i=0;i<MAX_IMAGES;++i) if (S->imgex[i].flags & LT_F_OWNMEM) free(S->imgex[i].d);
	free(S->infotext); free(S->tokens); free(S->tokens_w);
	loras_remove(S, 0);
	free(S->lkeys);
	S->signature = 0;
	free(S);
	*pctx = NULL;
}

MLB_API const char* mlis_errstr_get(const MLIS_Ctx* S) { return S ? S->errstr : mlsd_last_error(); }
MLB_API struct MLIS_AmdCtx* mlis_amd_engine_get(MLIS_Ctx* S) { return S ? S->eng : NULL; }
/* controlled evaluations of pass 0 / 1 of the last mlis_generate (a hires generation has two passes); -1 for a pass that did not run */
MLB_API int mlis_amd_control_evals(MLIS_Ctx* S, int pass)
{
	if (!S || S->signature != CTX_SIGNATURE || pass < 0 || pass >= S->control_pass) return -1;
	return S->control_evals[pass];
}
MLB_API int mlis_amd_engine_builds(MLIS_Ctx* S) { return (S && S->signature == CTX_SIGNATURE) ? S->n_eng_builds : -1; }
MLB_API int mlis_amd_lora_stats(MLIS_Ctx* S, int* n_restored, int* n_patched, int* n_cold_merges)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	if (n_restored) *n_restored = S->n_lora_restored;
	if (n_patched) *n_patched = S->n_lora_patched;
	if (n_cold_merges) *n_cold_merges = S->n_lora_cold;
	return 1;
}

/* ------------------------------------------------------------------ options */
/* by_option: the type comes from MLIS_OPT_MODEL_TYPE (it then survives a checkpoint whose type cannot be detected); a type that
 * mlis_setup DETECTED describes that checkpoint only and must not excuse the next, unidentifiable one */
static int model_type_set_ex(MLIS_Ctx* S, int mt, int by_option);
static int model_type_set(MLIS_Ctx* S, int mt) { return model_type_set_ex(S, mt, 1); }
static int model_type_set_ex(MLIS_Ctx* S, int mt, int by_option)
{	/* mlis_model_type_set :738-786: per-model defaults of size and clip_skip */
	int w = 0, skip = 0;
	switch (mt) {
	case MLIS_MODEL_TYPE_NONE: break;
	case MLIS_MODEL_TYPE_SD1: w = 512; skip = 1; break;
	case MLIS_MODEL_TYPE_SD2: w = 768; skip = 2; break;
	case MLIS_MODEL_TYPE_SDXL: w = 1024; skip = 2; break;
	case MLIS_MODEL_TYPE_AMD_TINY: case MLIS_MODEL_TYPE_AMD_TINYV: w = 64; skip = 1; break;
	case MLIS_MODEL_TYPE_AMD_TINYXL: w = 64; skip = 2; break;
	default: return api_error(S, MLIS_E_OPT_VALUE, "invalid model type %d", mt);
	}
	if (mt) { if (S->width <= 0) S->width = w; if (S->height <= 0) S->height = S->width; if (S->clip_skip <= 0) S->clip_skip = skip; }
	S->model_type = mt;
	if (by_option) { if (mt) S->flags |= CF_MODEL_TYPE_SET; else S->flags &= ~CF_MODEL_TYPE_SET; }
	snprintf(S->mname, sizeof(S->mname), "%s", mt ? model_name(mt) : "");
	return 1;
}

static int image_to_tensor(MLIS_Tensor* T, const MLIS_Image* I)
{	/* mlis_tensor_from_image :141-158: u8 HWC -> f32 CHW / 255 */
	const int n0 = (int)I->w, n1 = (int)I->h, n2 = (int)I->c;
	if (!(n0 * n1 * n2 > 0 && I->d)) return MLIS_E_IMAGE;
	mlis_tensor_resize(T, n0, n1, n2, 1);
	const float f = 1 / 255.0;
	for (int y=0;y<n1;++y) for (int x=0;x<n0;++x) for (int c=0;c<n2;++c)
		T->d[(size_t)n0*n1*c + (size_t)n0*y + x] = I->d[(size_t)n0*n2*y + (size_t)n2*x + c] * f;
	return 1;
}

/* the prompt text just stored in prompt_raw / nprompt_raw, taken apart */
static int prompt_parse(MLIS_Ctx* S, int neg)
{
	MLISPrompt *P = neg ? &S->nprompt : &S->prompt;
	const char *text = neg ? S->nprompt_raw : S->prompt_raw;
	S->have_ptok[neg] = 0;
	if (S->flags & CF_NO_PROMPT_PARSE) mlis_prompt_set_raw(P, text);
	else if (mlis_prompt_set_parse(P, text) < 0) return api_error_lib(S, MLIS_E_PROMPT_PARSE);
	else for (int i=0; i<P->n_lora; ++i) {            /* <lora:NAME:MULT> in the prompt (:49-52) */
		int r = lora_add(S, P->lora_names + P->loras[i].name_off, (size_t)P->loras[i].len, P->loras[i].w, LF_PROMPT);
		if (r < 0) return r;
	}
	return 1;
}

static int file_exists(const char* p);

/* mlis_cfg_lora_add + mlis_lora_path_find (:632-680): a path, or NAME -> <lora_dir>/NAME.safetensors */
static int lora_add(MLIS_Ctx* S, const char* name, size_t len, float mult, int flags)
{
	if (S->n_lora >= MAX_LORAS) return api_error(S, MLIS_E_UNKNOWN, "too many loras");
	char path[1200];
	snprintf(path, sizeof(path), "%.*s", (int)len, name);
	if (!file_exists(path)) {
		const char *d = S->path_lora_dir ? S->path_lora_dir : "";
		const size_t dl = strlen(d);
		snprintf(path, sizeof(path), "%s%s%.*s.safetensors", d, (dl && d[dl-1] != '/' && d[dl-1] != '\\') ? "/" : "", (int)len, name);
		if (!file_exists(path)) return api_error(S, MLIS_E_FILE_NOT_FOUND, "lora model file not found '%s'", path);
	}
	S->loras[S->n_lora].path = strdup(path); S->loras[S->n_lora].mult = mult; S->loras[S->n_lora].flags = flags;
	S->n_lora++;
	S->rflags &= ~READY_LORAS;
	return 1;
}

static void loras_remove(MLIS_Ctx* S, int only_prompt)
{
	int k = 0;
	for (int i=0;i<S->n_lora;++i) {
		if (only_prompt && !(S->loras[i].flags & LF_PROMPT)) { S->loras[k++] = S->loras[i]; continue; }
		free(S->loras[i].path);
		S->rflags &= ~READY_LORAS;
	}
	S->n_lora = k;
}

typedef struct { int is_str; va_list* ap; const char* cur; const char* arg_b; size_t arg_n; } ArgSrc;

static void next_str_arg(ArgSrc* A)
{	/* value_str_next :845-864: comma separated, optional double quotes */
	const char *cur = A->cur;
	if (*cur == ',') cur++;
	if (*cur == '"') { cur++; A->arg_b = cur; while (*cur && *cur != '"') cur++; A->arg_n = cur - A->arg_b; if (*cur == '"') cur++; }
	else { A->arg_b = cur; while (*cur && *cur != ',') cur++; A->arg_n = cur - A->arg_b; }
	A->cur = cur;
}
static int arg_int(ArgSrc* A, int mn, int mx, int def, int* out)
{
	int v;
	if (A->is_str) {
		next_str_arg(A);
		char *tail = (char*)A->arg_b + A->arg_n;
		v = A->arg_n ? (int)strtol(A->arg_b, &tail, 10) : def;
		if (tail != A->arg_b + A->arg_n) return 0;
	} else v = va_arg(*A->ap, int);
	if (!(mn <= v && v <= mx)) return 0;
	*out = v; return 1;
}
static int arg_float(ArgSrc* A, float mn, float mx, float def, float* out)
{
	float v;
	if (A->is_str) {
		next_str_arg(A);
		char *tail = (char*)A->arg_b + A->arg_n;
		v = A->arg_n ? strtof(A->arg_b, &tail) : def;
		if (tail != A->arg_b + A->arg_n) return 0;
	} else v = (float)va_arg(*A->ap, double);
	if (!(mn <= v && v <= mx)) return 0;
	*out = v; return 1;
}
static int arg_bool(ArgSrc* A, int* out)
{
	if (!A->is_str) { *out = !!va_arg(*A->ap, int); return 1; }
	next_str_arg(A);
	static const char* const t[] = {"true","yes","y","1"}; static const char* const f[] = {"false","no","n","0"};
	for (int i=0;i<4;++i) { if (A->arg_n == strlen(t[i]) && !memcmp(A->arg_b, t[i], A->arg_n)) { *out = 1; return 1; }
	                        if (A->arg_n == strlen(f[i]) && !memcmp(A->arg_b, f[i], A->arg_n)) { *out = 0; return 1; } }
	return 0;
}
/* whole remaining value (ARG_STR_NO_PARSE) or one comma-separated piece (ARG_STR); returns a malloc'd copy */
static char* arg_str(ArgSrc* A, int whole, size_t mn)
{
	if (!A->is_str) { const char *s = va_arg(*A->ap, const char*); if (!s || strlen(s) < mn) return NULL; return strdup(s); }
	if (whole) { A->arg_b = A->cur; A->arg_n = strlen(A->cur); A->cur += A->arg_n; } else next_str_arg(A);
	if (A->arg_n < mn) return NULL;
	char *r = (char*)malloc(A->arg_n + 1); memcpy(r, A->arg_b, A->arg_n); r[A->arg_n] = 0;
	return r;
}

/* One row per option (k_opt): everything the API knows about it.  Names, setting, getting and the values of a new context all derive from the rows.
 * Adding an option: the enumerator in mlis_abi.h, the field of MLIS_Ctx plus its row here, the constant in mlimgsynth.py. */
enum { OK_NONE,
	OK_INT,         /* int field: decimal text or int */
	OK_FLOAT,       /* float field: strtof text or double */
	OK_FLAG,        /* the reference's booleans, a bit of S->flags: arg_bool (variadic: any int, !!v) */
	OK_BOOL,        /* int field: arg_bool in text, an int in 0..1 variadic */
	OK_ENUM,        /* int field: a name of `names`, else a whole-token decimal; variadic any int; 0 <= v < n_names */
	OK_STR,         /* char* field: the whole remaining text, or a const char*, of at least `mn` characters */
	OK_CUSTOM };    /* option_custom reads the arguments itself */
enum { OF_GET = 1,       /* mlis_option_get serves it: int* (OK_CUSTOM: what `get` gives), float* or const char** (never NULL, "" while unset) */
       OF_RETAKE = 2 };  /* a changed value makes the engines take the control image again (control_apply), as after a new image */
typedef struct OptRow {
	int id; const char* name;
	int kind, flags;
	size_t where;                   /* offsetof the field in MLIS_Ctx; OK_FLAG: the bit */
	double mn, mx;                  /* inclusive range */
	double init, empty;             /* the value of a new context; the value an empty string stands for: one outside the range (NAN, -1) refuses it */
	const char* const* names; int n_names;
	const char* letters;            /* OK_ENUM: letters[v] is a one-letter, case-sensitive name of value v ('-': none) */
	int (*valid)(double v);         /* what a range cannot express */
	int (*after)(MLIS_Ctx* S, int changed);          /* runs once the value is stored; its result is the call's */
	int (*get)(const MLIS_Ctx* S);
} OptRow;

static int opt_bad_value(MLIS_Ctx* S, const OptRow* o, const ArgSrc* A)
{
	return A->is_str ? api_error(S, MLIS_E_OPT_VALUE, "invalid argument '%.*s' for option '%s'", (int)A->arg_n, A->arg_b ? A->arg_b : "", o->name)
		: api_error(S, MLIS_E_OPT_VALUE, "invalid argument for option '%s'", o->name);
}

/* ---- rules a range cannot express */
static int valid_mult8(double v) { return (int)v % 8 == 0; }
static int valid_hires_scale(double v) { return !(v > 0 && v < 1); }           /* 0 and 1: off */
static int valid_positive(double v) { return v > 0; }
static int valid_hypertile(double v) { return (int)v % 8 == 0 && (v == 0 || v >= 32); }      /* 0: off; the rule is applied per pass size (engine_get) */
static int valid_tile_overlap(double v) { return v <= 0 || (int)v % 8 == 0; }  /* -1: auto */

/* ---- what follows a stored value */
static int after_model(MLIS_Ctx* S, int changed) { (void)changed; model_drop(S); return 1; }
static int after_tae(MLIS_Ctx* S, int changed)
{
	(void)changed;
	if (*S->path_tae) S->flags |= CF_USE_TAE; else S->flags &= ~CF_USE_TAE;
	engine_drop(S); return 1;
}
static int after_aux_dir(MLIS_Ctx* S, int changed) { (void)changed; if (S->tok) { clip_tokr_free(S->tok); S->tok = NULL; } return 1; }
static int after_prompt(MLIS_Ctx* S, int changed) { (void)changed; return prompt_parse(S, 0); }
static int after_nprompt(MLIS_Ctx* S, int changed) { (void)changed; return prompt_parse(S, 1); }
static int after_control_model(MLIS_Ctx* S, int changed)
{	/* a changed ControlNet drops the engines that hold one (their ControlNet plans have the old weights); plain engines stay */
	if (changed) { control_engines_drop(S); if (S->ts_control) { mlts_close(S->ts_control); S->ts_control = NULL; } }
	return 1;
}
static int after_upscale_model(MLIS_Ctx* S, int changed) { if (changed) upscaler_drop(S); return 1; }      /* the next use builds the new one */

/* ---- OK_CUSTOM: options whose arguments are pointers, two values or a grammar of their own (src/mlimgsynth_options_set.c.h, option by option) */
static int get_model_type(const MLIS_Ctx* S) { return S->model_type; }
static int get_control_image(const MLIS_Ctx* S) { return tensor_good(&S->control_image); }      /* whether one is set */
static int option_custom(MLIS_Ctx* S, const OptRow* o, ArgSrc* A)
{
	int i = 0, j = 0, err = 1; float f = 0; char *s = NULL;
#define BAD_VALUE do { free(s); return opt_bad_value(S, o, A); } while (0)
#define NO_STR do { if (A->is_str) return api_error(S, MLIS_E_OPT_VALUE, "option '%s' cannot be set with a string value", o->name); } while (0)
	switch (o->id) {
	case MLIS_OPT_BACKEND: {
		if (!(s = arg_str(A, 0, 0))) BAD_VALUE;
		char *p2 = A->is_str ? arg_str(A, 0, 0) : NULL;
		if (!A->is_str) { const char *p = va_arg(*A->ap, const char*); (void)p; }
		free(p2);
		str_set(&S->backend, s); S->rflags &= ~READY_BACKEND;
	} break;
	case MLIS_OPT_MODEL_TYPE:
		if (A->is_str) { next_str_arg(A); i = model_from(A->arg_b, A->arg_n); if (i < 0) BAD_VALUE; } else i = va_arg(*A->ap, int);
		if (model_type_set(S, i) < 0) return MLIS_E_OPT_VALUE;
		model_drop(S);
		break;
	case MLIS_OPT_LORA: {
		if (!(s = arg_str(A, 0, 1))) BAD_VALUE;
		f = 1;
		if (A->is_str) { if (!arg_float(A, 0, 1, 1, &f)) BAD_VALUE; } else f = (float)va_arg(*A->ap, double);
		err = lora_add(S, s, strlen(s), f, 0);
	} break;
	case MLIS_OPT_LORA_CLEAR: loras_remove(S, 0); break;
	case MLIS_OPT_IMAGE_DIM: if (!arg_int(A, 0, 65535, 0, &i) || !arg_int(A, 0, 65535, 0, &j)) BAD_VALUE; S->width = i; S->height = j; break;
	case MLIS_OPT_METHOD:          /* (variadic: like the scheduler, not range-checked) */
		if (A->is_str) {
			next_str_arg(A);
			size_t n = A->arg_n; int anc = 0;
			if (n > 2 && !memcmp(A->arg_b + n - 2, "_a", 2)) { n -= 2; anc = 1; }        /* "euler_a": ancestral shortcut (:88-99) */
			i = from_list(k_method, COUNTOF(k_method), 1, A->arg_b, n);
			if (i < 0) { if (anc) return api_error(S, MLIS_E_OPT_VALUE, "invalid method name '%.*s'", (int)A->arg_n, A->arg_b); BAD_VALUE; }
			if (anc) S->s_ancestral = 1;
		} else i = va_arg(*A->ap, int);
		S->method = i; break;
	case MLIS_OPT_SCHEDULER:       /* a name only, no decimal: not an OK_ENUM */
		if (A->is_str) { next_str_arg(A); i = from_list(k_sched, COUNTOF(k_sched), 1, A->arg_b, A->arg_n); if (i < 0) BAD_VALUE; } else i = va_arg(*A->ap, int);
		S->sched = i; break;
	case MLIS_OPT_IMAGE: {
		NO_STR;
		const MLIS_Image *img = va_arg(*A->ap, const MLIS_Image*);
		if (!img || (img->c != 3 && img->c != 4)) return api_error(S, MLIS_E_IMAGE, "invalid number of channels in image: %d", img ? (int)img->c : 0);
		if (image_to_tensor(&S->image, img) < 0) return api_error(S, MLIS_E_IMAGE, "invalid image");
		S->tuflags |= MLIS_TUF_IMAGE;
		if (S->image.n[2] == 4) {   /* alpha channel = in-painting mask */
			const size_t wh = (size_t)S->image.n[0] * S->image.n[1];
			mlis_tensor_resize(&S->mask, S->image.n[0], S->image.n[1], 1, 1);
			memcpy(S->mask.d, S->image.d + wh*3, wh*4);
			S->image.n[2] = 3;
			S->tuflags |= MLIS_TUF_MASK;
		}
	} break;
	case MLIS_OPT_IMAGE_MASK: {
		NO_STR;
		const MLIS_Image *img = va_arg(*A->ap, const MLIS_Image*);
		if (!img || img->c != 1) return api_error(S, MLIS_E_IMAGE, "invalid number of channels in image mask: %d", img ? (int)img->c : 0);
		if (image_to_tensor(&S->mask, img) < 0) return api_error(S, MLIS_E_IMAGE, "invalid image mask");
		S->tuflags |= MLIS_TUF_MASK;
	} break;
	case MLIS_OPT_SEED:
		if (A->is_str) {
			if (!A->cur[0]) break;                                   /* empty string: keep the random seed */
			next_str_arg(A);
			char *tail = NULL; uint64_t v = (uint64_t)strtoll(A->arg_b, &tail, 10);
			if (tail != A->arg_b + A->arg_n) BAD_VALUE;
			S->seed = v;
		} else S->seed = va_arg(*A->ap, uint64_t);
		break;
	case MLIS_OPT_AMD_CONTROL_IMAGE: {
		NO_STR;
		const MLIS_Image *img = va_arg(*A->ap, const MLIS_Image*);
		if (!img) { mlis_tensor_free(&S->control_image); break; }
		if (img->c != 3) return api_error(S, MLIS_E_IMAGE, "invalid number of channels in control image: %d (3: the finished control map as RGB)", (int)img->c);
		if (image_to_tensor(&S->control_image, img) < 0) return api_error(S, MLIS_E_IMAGE, "invalid control image");
		S->control_image_gen++;      /* engines holding the previous image take this one at their next pass (control_apply) */
	} break;
	case MLIS_OPT_WEIGHT_TYPE:
		if (S->n_applied) { S->ts_partial = 1; S->rflags &= ~READY_LORAS; }      /* the merge's operand rounding follows the weight type: active adapters are merged again, the cold way */
		if (A->is_str) {
			next_str_arg(A);
			static const struct { const char* n; int t; } wt[] = { {"f32", MLT_F32}, {"f16", MLT_F16}, {"bf16", MLT_BF16} };
			int found = 0;
			for (int k=0;k<3;++k) if (id_eq(A->arg_b, A->arg_n, wt[k].n)) { S->wtype = wt[k].t; S->flags |= CF_WEIGHT_TYPE_SET; found = 1; }
			if (found) break;
			char *tail = (char*)A->arg_b + A->arg_n; i = A->arg_n ? (int)strtol(A->arg_b, &tail, 10) : 0;
			if (tail != A->arg_b + A->arg_n) BAD_VALUE;
		} else i = va_arg(*A->ap, int);
		if (i == -1) { S->wtype = MLT_F16; S->flags &= ~CF_WEIGHT_TYPE_SET; }
		else if (i == MLT_F32 || i == MLT_F16 || i == MLT_BF16) { S->wtype = i; S->flags |= CF_WEIGHT_TYPE_SET; }
		else return api_error(S, MLIS_E_OPT_VALUE, "weight type %d is not supported (f32, f16, bf16; quantised ggml types are not)", i);
		break;
	case MLIS_OPT_CALLBACK: NO_STR; S->callback = va_arg(*A->ap, MLIS_Callback); S->callback_ud = va_arg(*A->ap, void*); break;
	case MLIS_OPT_ERROR_HANDLER: NO_STR; S->errh = va_arg(*A->ap, MLIS_ErrorHandler); S->errh_ud = va_arg(*A->ap, void*); break;
	case MLIS_OPT_LOG_LEVEL:
		if (A->is_str) { next_str_arg(A); } else (void)va_arg(*A->ap, int);   /* this library does not log: accepted, ignored */
		break;
	}
	free(s);
	return err;
#undef BAD_VALUE
#undef NO_STR
}

/* ---- the rows.  AT fails to compile unless the field has the type the row's kind reads and writes. */
#define AT(type, field) _Generic(&((MLIS_Ctx*)0)->field, type*: offsetof(MLIS_Ctx, field))
#define ROW(ID, NAME, KIND, ...) { .id = ID, .name = NAME, .kind = KIND, __VA_ARGS__ }
#define O_INT(ID, NAME, FIELD, MN, MX, INIT, EMPTY, ...) ROW(ID, NAME, OK_INT, .where = AT(int, FIELD), .mn = MN, .mx = MX, .init = INIT, .empty = EMPTY, __VA_ARGS__)
#define O_FLOAT(ID, NAME, FIELD, MN, MX, INIT, EMPTY, ...) ROW(ID, NAME, OK_FLOAT, .where = AT(float, FIELD), .mn = MN, .mx = MX, .init = INIT, .empty = EMPTY, __VA_ARGS__)
#define O_FLAG(ID, NAME, BIT) ROW(ID, NAME, OK_FLAG, .where = BIT)
#define O_BOOL(ID, NAME, FIELD, ...) ROW(ID, NAME, OK_BOOL, .where = AT(int, FIELD), __VA_ARGS__)
#define O_ENUM(ID, NAME, FIELD, LIST, INIT, EMPTY, ...) ROW(ID, NAME, OK_ENUM, .where = AT(int, FIELD), .names = LIST, .n_names = COUNTOF(LIST), .init = INIT, .empty = EMPTY, __VA_ARGS__)
#define O_STR(ID, NAME, FIELD, MINLEN, ...) ROW(ID, NAME, OK_STR, .where = AT(char*, FIELD), .mn = MINLEN, __VA_ARGS__)
#define O_CUSTOM(ID, NAME, ...) ROW(ID, NAME, OK_CUSTOM, __VA_ARGS__)
#define REFUSED NAN
static const OptRow k_opt[] = {
	ROW(MLIS_OPT_NONE, "none", OK_NONE, .where = 0),
	O_CUSTOM(MLIS_OPT_BACKEND, "backend"),
	O_STR(MLIS_OPT_MODEL, "model", path_model, 1, .flags = OF_GET, .after = after_model),
	O_STR(MLIS_OPT_TAE, "tae", path_tae, 0, .after = after_tae),
	O_STR(MLIS_OPT_LORA_DIR, "lora_dir", path_lora_dir, 0),
	O_CUSTOM(MLIS_OPT_LORA, "lora"),
	O_CUSTOM(MLIS_OPT_LORA_CLEAR, "lora_clear"),
	O_STR(MLIS_OPT_PROMPT, "prompt", prompt_raw, 0, .flags = OF_GET, .after = after_prompt),
	O_STR(MLIS_OPT_NPROMPT, "nprompt", nprompt_raw, 0, .flags = OF_GET, .after = after_nprompt),
	O_CUSTOM(MLIS_OPT_IMAGE_DIM, "image_dim"),
	O_INT(MLIS_OPT_BATCH_SIZE, "batch_size", n_batch, 0, 1024, 0, 0),
	O_INT(MLIS_OPT_CLIP_SKIP, "clip_skip", clip_skip, 0, 255, 0, 0),
	O_FLOAT(MLIS_OPT_CFG_SCALE, "cfg_scale", cfg_scale, 0, 255, 7, REFUSED),
	O_CUSTOM(MLIS_OPT_METHOD, "method"),
	O_CUSTOM(MLIS_OPT_SCHEDULER, "scheduler"),
	O_INT(MLIS_OPT_STEPS, "steps", n_step, 0, 1000, 0, 0),
	O_FLOAT(MLIS_OPT_F_T_INI, "f_t_ini", f_t_ini, 0, 1, 1, REFUSED),
	O_FLOAT(MLIS_OPT_F_T_END, "f_t_end", f_t_end, 0, 1, 0, REFUSED),
	O_FLOAT(MLIS_OPT_S_NOISE, "s_noise", s_noise, 0, 255, 0, REFUSED),
	O_FLOAT(MLIS_OPT_S_ANCESTRAL, "s_ancestral", s_ancestral, 0, 255, 0, REFUSED),
	O_CUSTOM(MLIS_OPT_IMAGE, "image"),
	O_CUSTOM(MLIS_OPT_IMAGE_MASK, "image_mask"),
	O_FLAG(MLIS_OPT_NO_DECODE, "no_decode", CF_NO_DECODE),
	O_INT(MLIS_OPT_TENSOR_USE_FLAGS, "tensor_use_flags", tuflags, 0, 0x7fffffff, 0, 0),
	O_CUSTOM(MLIS_OPT_SEED, "seed"),
	O_INT(MLIS_OPT_VAE_TILE, "vae_tile", vae_tile, 0, 65535, 0, 0),
	O_FLAG(MLIS_OPT_UNET_SPLIT, "unet_split", CF_UNET_SPLIT),      /* weight streaming through three device slabs (engine_get) */
	O_INT(MLIS_OPT_THREADS, "threads", n_thread, 0, 65535, 0, 0),
	O_INT(MLIS_OPT_DUMP_FLAGS, "dump_flags", dump_flags, 0, 0x7fffffff, 0, 0),
	O_STR(MLIS_OPT_AUX_DIR, "aux_dir", path_aux, 0, .after = after_aux_dir),
	O_CUSTOM(MLIS_OPT_CALLBACK, "callback"),
	O_CUSTOM(MLIS_OPT_ERROR_HANDLER, "error_handler"),
	O_CUSTOM(MLIS_OPT_LOG_LEVEL, "log_level"),
	O_CUSTOM(MLIS_OPT_MODEL_TYPE, "model_type", .flags = OF_GET, .get = get_model_type),
	O_CUSTOM(MLIS_OPT_WEIGHT_TYPE, "weight_type"),
	O_FLAG(MLIS_OPT_NO_PROMPT_PARSE, "no_prompt_parse", CF_NO_PROMPT_PARSE),
	/* a changed tiling mode, freeu, hypertile or hypertile_depth, or pag_scale going on / off, selects another engine (engine_get key) */
	O_ENUM(MLIS_OPT_AMD_TILING, "tiling", tiling, k_tiling, 0, -1, .flags = OF_GET),
	O_FLOAT(MLIS_OPT_AMD_HIRES_SCALE, "hires_scale", hires_scale, 0, 4, 0, REFUSED, .flags = OF_GET, .valid = valid_hires_scale),
	O_FLOAT(MLIS_OPT_AMD_HIRES_DENOISE, "hires_denoise", hires_denoise, 0, 1, 0.7, REFUSED, .flags = OF_GET, .valid = valid_positive),
	O_INT(MLIS_OPT_AMD_HIRES_STEPS, "hires_steps", hires_steps, 0, 1000, 0, 0, .flags = OF_GET),
	O_ENUM(MLIS_OPT_AMD_HIRES_UPSCALER, "hires_upscaler", hires_upscaler, k_resample, MLIS_AMD_RESAMPLE_BILINEAR, -1, .flags = OF_GET),
	O_INT(MLIS_OPT_AMD_UNET_TILE, "unet_tile", unet_tile, 0, 65535, 0, 0, .flags = OF_GET, .valid = valid_mult8),      /* the relation to the overlap is checked when an engine is needed (unet_tile_check) */
	O_INT(MLIS_OPT_AMD_UNET_TILE_OVERLAP, "unet_tile_overlap", unet_tile_overlap, -1, 65535, -1, -1, .flags = OF_GET, .valid = valid_tile_overlap),
	O_INT(MLIS_OPT_AMD_UNET_TILE_BATCH, "unet_tile_batch", unet_tile_batch, 1, MLSD_WINDOW_MAX_PACK, 1, 1, .flags = OF_GET),      /* an upper bound: mlis_amd_tile_pack gives the effective pack */
	O_STR(MLIS_OPT_AMD_CONTROL_MODEL, "control_model", path_control, 0, .flags = OF_GET, .after = after_control_model),
	O_CUSTOM(MLIS_OPT_AMD_CONTROL_IMAGE, "control_image", .flags = OF_GET, .get = get_control_image),
	O_FLOAT(MLIS_OPT_AMD_CONTROL_STRENGTH, "control_strength", control_strength, 0, 2, 1, 1, .flags = OF_GET),
	O_FLOAT(MLIS_OPT_AMD_CONTROL_START, "control_start", control_start, 0, 1, 0, 0, .flags = OF_GET),      /* start <= end: checked by mlis_generate, the two are set one by one */
	O_FLOAT(MLIS_OPT_AMD_CONTROL_END, "control_end", control_end, 0, 1, 1, 1, .flags = OF_GET),
	O_BOOL(MLIS_OPT_AMD_FREEU, "freeu", freeu, .flags = OF_GET),
	O_FLOAT(MLIS_OPT_AMD_FREEU_B1, "freeu_b1", freeu_f[0], 0, 4, 1.3, 1.3, .flags = OF_GET),      /* (mlis_abi.h on where the four initial values come from) */
	O_FLOAT(MLIS_OPT_AMD_FREEU_B2, "freeu_b2", freeu_f[1], 0, 4, 1.4, 1.4, .flags = OF_GET),
	O_FLOAT(MLIS_OPT_AMD_FREEU_S1, "freeu_s1", freeu_f[2], 0, 4, 0.9, 0.9, .flags = OF_GET),
	O_FLOAT(MLIS_OPT_AMD_FREEU_S2, "freeu_s2", freeu_f[3], 0, 4, 0.2, 0.2, .flags = OF_GET),
	O_STR(MLIS_OPT_AMD_UPSCALE_MODEL, "upscale_model", path_upscale, 0, .flags = OF_GET, .after = after_upscale_model),
	O_BOOL(MLIS_OPT_AMD_HIRES_USE_MODEL, "hires_use_model", hires_use_model, .flags = OF_GET),
	O_ENUM(MLIS_OPT_AMD_DOWNSCALE_FILTER, "downscale_filter", downscale_filter, k_downscale, 0, -1, .flags = OF_GET | OF_RETAKE),
	O_ENUM(MLIS_OPT_AMD_CONTROL_PREPROCESS, "control_preprocess", control_preprocess, k_preprocess, 0, -1, .flags = OF_GET | OF_RETAKE),
	O_FLOAT(MLIS_OPT_AMD_CANNY_LOW, "canny_low", canny_low, 0, 32767, 100, 100, .flags = OF_GET | OF_RETAKE),
	O_FLOAT(MLIS_OPT_AMD_CANNY_HIGH, "canny_high", canny_high, 0, 32767, 200, 200, .flags = OF_GET | OF_RETAKE),
	O_BOOL(MLIS_OPT_AMD_CANNY_L2, "canny_l2", canny_l2, .flags = OF_GET | OF_RETAKE),
	O_ENUM(MLIS_OPT_AMD_INPAINT_AREA, "inpaint_area", inpaint_area, k_inpaint_area, 0, -1, .flags = OF_GET),
	O_INT(MLIS_OPT_AMD_INPAINT_PADDING, "inpaint_padding", inpaint_padding, 0, 512, 32, 32, .flags = OF_GET),
	O_FLOAT(MLIS_OPT_AMD_MASK_BLUR, "mask_blur", mask_blur, 0, MLSD_GAUSS_MAX_SIGMA, 0, 0, .flags = OF_GET),
	O_INT(MLIS_OPT_AMD_MASK_GROW, "mask_grow", mask_grow, -MLSD_MASK_GROW_MAX, MLSD_MASK_GROW_MAX, 0, 0, .flags = OF_GET),
	O_BOOL(MLIS_OPT_AMD_MASK_INVERT, "mask_invert", mask_invert, .flags = OF_GET),
	O_BOOL(MLIS_OPT_AMD_INPAINT_COMPOSITE, "inpaint_composite", inpaint_composite, .flags = OF_GET),
	O_INT(MLIS_OPT_AMD_HYPERTILE, "hypertile", hypertile, 0, 8192, 0, 0, .flags = OF_GET, .valid = valid_hypertile),
	O_INT(MLIS_OPT_AMD_HYPERTILE_DEPTH, "hypertile_depth", hypertile_depth, 0, 3, 3, 3, .flags = OF_GET),
	O_FLOAT(MLIS_OPT_AMD_PAG_SCALE, "pag_scale", pag_scale, 0, 20, 0, 0, .flags = OF_GET),      /* the value is handed to the engine per generation, as cfg_rescale */
	O_FLOAT(MLIS_OPT_AMD_CFG_RESCALE, "cfg_rescale", cfg_rescale, 0, 1, 0, 0, .flags = OF_GET),
	O_ENUM(MLIS_OPT_AMD_PREDICTION, "prediction", prediction, k_prediction, 0, 0, .flags = OF_GET),
	O_ENUM(MLIS_OPT_AMD_ZSNR, "zsnr", zsnr, k_zsnr, 0, 0, .flags = OF_GET, .letters = "-ny"),
};
#undef REFUSED

static const OptRow* option_row(int id)
{
	for (int k=0;k<COUNTOF(k_opt);++k) if (k_opt[k].id == id) return &k_opt[k];
	return NULL;
}
MLB_API const char* mlis_option_str(MLIS_Option x) { const OptRow *o = option_row((int)x); return o ? o->name : "???"; }
MLB_API MLIS_Option mlis_option_fromz(const char* s)
{
	for (int k=0;k<COUNTOF(k_opt);++k) if (id_eq(s, strlen(s), k_opt[k].name)) return (MLIS_Option)k_opt[k].id;
	return (MLIS_Option)-1;
}

static void options_init(MLIS_Ctx* S)
{
	for (const OptRow *o = k_opt; o < k_opt + COUNTOF(k_opt); ++o) {
		void *p = (char*)S + o->where;
		if (o->kind == OK_FLOAT) *(float*)p = (float)o->init;
		else if (o->kind == OK_INT || o->kind == OK_BOOL || o->kind == OK_ENUM) *(int*)p = (int)o->init;
	}
}

static int arg_enum(ArgSrc* A, const OptRow* o, int* out)
{
	int v;
	if (A->is_str) {
		next_str_arg(A);
		v = from_list(o->names, o->n_names, 1, A->arg_b, A->arg_n);
		const char *l = (v < 0 && o->letters && A->arg_n == 1) ? strchr(o->letters, A->arg_b[0]) : NULL;
		if (l && *l != '-') v = (int)(l - o->letters);
		if (v < 0) {
			char *tail = (char*)A->arg_b + A->arg_n; v = A->arg_n ? (int)strtol(A->arg_b, &tail, 10) : (int)o->empty;
			if (tail != A->arg_b + A->arg_n) v = -1;
		}
	} else v = va_arg(*A->ap, int);
	if (v < 0 || v >= o->n_names) return 0;
	*out = v; return 1;
}

static int option_apply(MLIS_Ctx* S, int id, ArgSrc* A)
{
	const OptRow *o = option_row(id);
	if (!o || o->kind == OK_NONE) return api_error(S, MLIS_E_UNK_OPT, "unknown option %u", (unsigned)id);
	void *p = (char*)S + o->where;
	int i = 0, ok = 0, changed; float f = 0;
	switch (o->kind) {
	case OK_CUSTOM: return option_custom(S, o, A);
	case OK_FLAG:
		if (!arg_bool(A, &i)) return opt_bad_value(S, o, A);
		if (i) S->flags |= (int)o->where; else S->flags &= ~(int)o->where;
		return 1;
	case OK_STR: {
		char **ps = (char**)p, *s = arg_str(A, 1, (size_t)o->mn);
		if (!s) return opt_bad_value(S, o, A);
		changed = !*ps || strcmp(*ps, s);
		free(*ps); *ps = s;
		return o->after ? o->after(S, changed) : 1;
	}
	case OK_FLOAT: ok = arg_float(A, (float)o->mn, (float)o->mx, (float)o->empty, &f); break;
	case OK_INT: ok = arg_int(A, (int)o->mn, (int)o->mx, (int)o->empty, &i); break;
	case OK_BOOL: ok = A->is_str ? arg_bool(A, &i) : arg_int(A, 0, 1, 0, &i); break;
	case OK_ENUM: ok = arg_enum(A, o, &i); break;
	}
	const int is_f = o->kind == OK_FLOAT;
	if (!ok || (o->valid && !o->valid(is_f ? (double)f : (double)i))) return opt_bad_value(S, o, A);
	changed = is_f ? f != *(float*)p : i != *(int*)p;
	if (changed && (o->flags & OF_RETAKE) && tensor_good(&S->control_image)) S->control_image_gen++;
	if (is_f) *(float*)p = f; else *(int*)p = i;
	return o->after ? o->after(S, changed) : 1;
}

MLB_API int mlis_option_set(MLIS_Ctx* S, MLIS_Option id, ...)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	va_list ap; va_start(ap, id);
	ArgSrc A = { 0, &ap, NULL, NULL, 0 };
	int r = option_apply(S, (int)id, &A);
	va_end(ap);
	return r;
}

MLB_API int mlis_option_set_str(MLIS_Ctx* S, const char* name, const char* value)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	int id = name ? (int)mlis_option_fromz(name) : -1;
	if (id <= 0) return api_error(S, MLIS_E_UNK_OPT, "unknown option '%s'", name ? name : "");
	ArgSrc A = { 1, NULL, value ? value : "", NULL, 0 };
	return option_apply(S, id, &A);
}

MLB_API int mlis_option_get(MLIS_Ctx* S, MLIS_Option id, ...)
{	/* src/mlimgsynth_options_get.c.h implements four options (MODEL, MODEL_TYPE, PROMPT, NPROMPT); here also every MLIS_OPT_AMD_* one */
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	const OptRow *o = option_row((int)id);
	if (!o || !(o->flags & OF_GET)) return api_error(S, MLIS_E_UNK_OPT, "unknown option %u", (unsigned)id);
	const void *p = (const char*)S + o->where;
	va_list ap; va_start(ap, id);
	if (o->kind == OK_FLOAT) { float *out = va_arg(ap, float*); if (out) *out = *(const float*)p; }
	else if (o->kind == OK_STR) { const char **out = va_arg(ap, const char**); if (out) *out = *(char* const*)p ? *(char* const*)p : ""; }
	else { int *out = va_arg(ap, int*); if (out) *out = o->kind == OK_CUSTOM ? o->get(S) : *(const int*)p; }
	va_end(ap);
	return 1;
}

MLB_API int mlis_amd_prompt_tokens_set(MLIS_Ctx* S, const int32_t* tokens, const float* weights, int n, int negative)
{
	const int k = negative ? 1 : 0;
	if (n < 0 || (n && !tokens)) return api_error(S, MLIS_E_OPT_VALUE, "invalid token list");
	free(S->ptok[k]); free(S->ptokw[k]);
	S->ptok[k] = (int32_t*)malloc(sizeof(int32_t) * (n ? n : 1)); S->ptokw[k] = (float*)malloc(sizeof(float) * (n ? n : 1));
	for (int i=0;i<n;++i) { S->ptok[k][i] = tokens[i]; S->ptokw[k][i] = weights ? weights[i] : 1.0f; }
	S->n_ptok[k] = n; S->have_ptok[k] = 1;
	return 1;
}

/* ------------------------------------------------------------------ setup */
MLB_API const MLIS_BackendInfo* mlis_backend_info_get(MLIS_Ctx* S, unsigned idx, int flags)
{	/* one backend: "HIP" with its devices (mlis_backend_info_get :572-612) */
	(void)flags;
	if (!S || idx != 0) return NULL;
	int n = mlsd_device_count(); if (n > 16) n = 16; if (n < 0) n = 0;
	for (int d=0; d<n; ++d) {
		int ncu = 0; size_t tot = 0, fr = 0;
		mlsd_device_info(d, S->dev_names[d][1], 96, S->dev_names[d][0], 96, &ncu, &tot, &fr);
		char nm[96]; snprintf(nm, sizeof(nm), "HIP%d", d); snprintf(S->dev_names[d][0], 96, "%s", nm);
		S->devs[d].name = S->dev_names[d][0]; S->devs[d].desc = S->dev_names[d][1]; S->devs[d].mem_free = fr; S->devs[d].mem_total = tot;
	}
	S->backend_info.name = "HIP"; S->backend_info.n_dev = (unsigned)n; S->backend_info.devs = S->devs;
	return &S->backend_info;
}

static int file_exists(const char* p) { struct stat st; return p && *p && !stat(p, &st); }

static int backend_setup(MLIS_Ctx* S)
{
	if (!(S->rflags & READY_BACKEND)) {
		/* mlis_backend_init :1119-1161: "" / "HIP" / "HIPn" select a device; anything else is an unknown backend */
		int dev = 0;
		if (!str_empty(S->backend)) {
			if (!strncasecmp(S->backend, "hip", 3) || !strncasecmp(S->backend, "rocm", 4)) dev = atoi(S->backend + (tolower((unsigned char)S->backend[0]) == 'h' ? 3 : 4));
			else return api_error(S, MLIS_E_UNKNOWN, "backend '%s' not available (this library drives MI355X through HIP only)", S->backend);
		}
		if (!mlsd_runtime_is_dry()) {
			if (mlsd_device_count() <= 0) return api_error(S, MLIS_E_UNKNOWN, "no HIP device available (there is no CPU fallback)");
			if (mlsd_device_set(dev)) return api_error_lib(S, MLIS_E_UNKNOWN);
		}
		S->rflags |= READY_BACKEND;
	}
	return 1;
}

/* ------------------------------------------------------------------ LoRA */
static int loras_same_as_applied(const MLIS_Ctx* S)
{
	if (S->n_lora != S->n_applied) return 0;
	for (int i=0;i<S->n_lora;++i) if (strcmp(S->loras[i].path, S->applied[i].path) || S->loras[i].mult != S->applied[i].mult) return 0;
	return 1;
}
static void applied_from_options(MLIS_Ctx* S)
{
	applied_clear(S);
	for (int i=0;i<S->n_lora;++i) { S->applied[i].path = strdup(S->loras[i].path); S->applied[i].mult = S->loras[i].mult; }
	S->n_applied = S->n_lora;
}

/* every plan with weights on the device: both engine slots' UNet, decoder, encoder and tile plans, the text towers (a plan built but not loaded yet is
 * patched when it is loaded, ctx_weights) */
#define MAX_RESIDENT 16
static int resident_ctxs(MLIS_Ctx* S, MLCtx** out)
{
	int n = 0;
	MLIS_AmdCtx *eng[2] = { S->eng, S->eng2 };
	for (int e=0;e<2;++e) for (int i=0; eng[e] && i<5; ++i) {      /* (plans 5 and 6, the ControlNet's, are left out: LoRAs do not touch it) */
		MLCtx *c = mlis_amd_ctx_at(eng[e], i);
		if (c && mlctx_params_loaded(c)) out[n++] = c;
	}
	for (int i=0; S->tc && i<mlis_amd_textcond_n_towers(S->tc) && n<MAX_RESIDENT; ++i) {
		MLCtx *c = mlis_amd_textcond_ctx(S->tc, i);
		if (c && mlctx_params_loaded(c)) out[n++] = c;
	}
	return n;
}

/* The device path gives the host merge's bits when the weight on the device IS the value the merge starts from: an F16 parameter with F16 operand rounding
 * (weight types F16 and BF16), or an F32 parameter with weight type F32.  The engine keeps every matrix weight in F16, so a checkpoint used at weight type F32
 * -- the host merge then adds to the unrounded fp32 weight and rounds once -- cannot be patched on the device: such a change goes the cold way. */
static int lora_exact_on_device(const MLIS_Ctx* S, const MLCtx* C, int ip)
{
	int type = -1;
	mlctx_param_info(C, ip, NULL, &type, NULL);
	return S->wtype != MLT_F32 ? type == MLT_F16 : type == MLT_F32;
}

/* one adapter onto the plans of `ctxs` that hold its targets; the keys are noted BEFORE they are patched (a failure restores them).  S->ts is the checkpoint. */
static int lora_patch(MLIS_Ctx* S, const MLTStore* L, float mult, MLCtx** ctxs, int nc)
{
	MLTSLoraItem it;
	const int n = mlts_count(L);
	for (int i=0;i<n;++i) {
		int r = mlts_lora_resolve(S->ts, L, i, mult, &it);
		if (r < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
		if (!r) continue;
		float *up = NULL, *down = NULL;
		for (int k=0; k<nc && r>0; ++k) {
			const int ip = mlctx_param_find(ctxs[k], it.key);
			if (ip < 0) continue;
			if (!lora_exact_on_device(S, ctxs[k], ip)) { r = api_error(S, MLIS_E_UNKNOWN, "lora: '%s' cannot be patched on the device at this weight type", it.key); break; }
			if (!up) {
				up = (float*)malloc(sizeof(float) * (size_t)(it.n1 * it.n_inner)); down = (float*)malloc(sizeof(float) * (size_t)(it.n_inner * it.n0));
				if (!up || !down || it.n_inner > 0x7fffffff) { r = api_error(S, MLIS_E_UNKNOWN, "lora: out of memory"); break; }
				mlts_lora_operands(&it, S->wtype, up, down);
			}
			lkey_add(S, it.key);
			if (mlctx_param_lora(ctxs[k], it.key, up, down, it.n0, it.n1, (int)it.n_inner, it.scale) < 0) { r = api_error_lib(S, MLIS_E_UNKNOWN); break; }
			S->n_lora_patched++;
		}
		free(up); free(down);
		if (r < 0) return r;
	}
	return 1;
}

/* every key an adapter patched back to the checkpoint's weight, in every plan that holds it */
static int lora_restore(MLIS_Ctx* S, MLCtx** ctxs, int nc)
{
	for (int i=0;i<S->n_lkeys;++i) for (int k=0;k<nc;++k) {
		if (mlctx_param_find(ctxs[k], S->lkeys[i]) < 0) continue;
		if (mlctx_tstore_load_key(ctxs[k], S->ts, S->lkeys[i]) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
		S->n_lora_restored++;
	}
	lkeys_clear(S);
	return 1;
}

static int ts_reopen(MLIS_Ctx* S)
{	/* the checkpoint again: the header parsed over an mmap, no data copied */
	MLTStore *p = mlts_open_safetensors(S->path_model, 1);
	if (!p) return api_error_lib(S, MLIS_E_UNKNOWN);
	mlts_close(S->ts);
	S->ts = p; S->ts_merged = S->ts_partial = 0;
	return 1;
}

/* The LoRA list changed while plans are resident: nothing is dropped or rebuilt.  All adapters are opened and validated first (mlts_lora_resolve: the host
 * merge's checks and error texts), so that a missing tensor or a bad shape leaves the device untouched; then every weight the old set patched is restored from
 * the checkpoint and the new set is applied in option order -- F16 weights round between adapters exactly as the host merge stores F16 between them.  A failure
 * midway (a non-finite result) restores what was touched: the plans then hold the checkpoint's weights.  Returns 1, 0 when this change has to go the cold way. */
static int loras_apply_warm(MLIS_Ctx* S)
{
	MLCtx *ctxs[MAX_RESIDENT];
	const int nc = resident_ctxs(S, ctxs);
	MLTStore *L[MAX_LORAS] = { NULL };
	int R = 1;
	if (S->ts_merged && ts_reopen(S) < 0) return -1;
	for (int i=0; i<S->n_lora && R>0; ++i) {
		if (!(L[i] = mlts_open_lora(S->loras[i].path))) { R = api_error_lib(S, MLIS_E_UNKNOWN); break; }
		MLTSLoraItem it;
		for (int j=0; j<mlts_count(L[i]) && R>0; ++j) {
			const int r = mlts_lora_resolve(S->ts, L[i], j, S->loras[i].mult, &it);
			if (r < 0) R = api_error_lib(S, MLIS_E_UNKNOWN);
			for (int k=0; k<nc && r>0 && R>0; ++k) {
				const int ip = mlctx_param_find(ctxs[k], it.key);
				if (ip >= 0 && !lora_exact_on_device(S, ctxs[k], ip)) R = 0;
			}
		}
	}
	if (R > 0) {
		if (lora_restore(S, ctxs, nc) < 0) R = -1;
		else {
			applied_clear(S);
			for (int i=0; i<S->n_lora && R>0; ++i)
				if (lora_patch(S, L[i], S->loras[i].mult, ctxs, nc) < 0) {
					char why[sizeof(S->errstr)]; snprintf(why, sizeof(why), "%s", S->errstr);
					R = lora_restore(S, ctxs, nc) < 0 ? -2 : -1;
					snprintf(S->errstr, sizeof(S->errstr), "%s", why);
				}
		}
		if (R == -2 || (R < 0 && S->n_lkeys)) {          /* a restore failed: the plans' weights are unknown, they go */
			engine_drop(S); textcond_drop(S); lkeys_clear(S); applied_clear(S);
		}
		if (R > 0) applied_from_options(S);
	}
	for (int i=0;i<S->n_lora;++i) if (L[i]) mlts_close(L[i]);
	if (!R) {       /* the cold way: the plans are rebuilt from a merged store */
		engine_drop(S); textcond_drop(S);
	}
	return R < 0 ? MLIS_E_UNKNOWN : R;
}

/* nothing resident: every active adapter is merged into a freshly read store on the host (:1276-1296); the plans built later load the merged weights */
static int loras_apply_cold(MLIS_Ctx* S)
{
	engine_drop(S); textcond_drop(S);
	if ((S->ts_merged || S->ts_partial) && ts_reopen(S) < 0) { S->rflags &= ~READY_MODEL; return MLIS_E_UNKNOWN; }
	applied_clear(S); lkeys_clear(S);
	for (int i=0;i<S->n_lora;++i) {
		MLTStore *L = mlts_open_lora(S->loras[i].path);
		if (!L) return api_error_lib(S, MLIS_E_UNKNOWN);
		MLTSLoraItem it;
		for (int j=0;j<mlts_count(L);++j) if (mlts_lora_resolve(S->ts, L, j, S->loras[i].mult, &it) > 0) lkey_add(S, it.key);
		S->ts_partial = 1;
		int r = mlts_lora_apply(S->ts, L, S->loras[i].mult, S->wtype);
		mlts_close(L);
		if (r < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
		S->ts_partial = 0; S->ts_merged = 1;
		S->n_lora_cold++;
		S->applied[S->n_applied].path = strdup(S->loras[i].path); S->applied[S->n_applied].mult = S->loras[i].mult; S->n_applied++;
	}
	return 1;
}

MLB_API int mlis_setup(MLIS_Ctx* S)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	int rb = backend_setup(S); if (rb < 0) return rb;
	if (!(S->rflags & READY_MODEL)) {
		if (str_empty(S->path_model)) return api_error(S, MLIS_E_FILE_NOT_FOUND, "no model set (option MODEL)");
		if (S->ts) { mlts_close(S->ts); S->ts = NULL; }               /* left over from a set-up that failed after opening the file */
		if (S->ts_tae) { mlts_close(S->ts_tae); S->ts_tae = NULL; }
		if (!strncmp(S->path_model, "synth:", 6)) {
			char nm[32]; snprintf(nm, sizeof(nm), "%s", S->path_model + 6);
			char *c = strchr(nm, ':'); S->synth_seed = 1234;
			if (c) { *c = 0; S->synth_seed = strtoull(c + 1, NULL, 10); }
			const int mt = model_from(nm, strlen(nm));
			if (mt <= 0) return api_error(S, MLIS_E_OPT_VALUE, "unknown synthetic model '%s'", nm);
			if (model_type_set_ex(S, mt, 0) < 0) return MLIS_E_OPT_VALUE;
			S->synth = 1; S->ckpt_v_pred = S->ckpt_ztsnr = 0;
		} else {
			/* mlis_model_load :1163-1204 + mlis_model_identify :1206-1249 */
			S->synth = 0;
			S->ts = mlts_open_safetensors(S->path_model, 1);
			if (!S->ts) return api_error_lib(S, file_exists(S->path_model) ? MLIS_E_UNKNOWN : MLIS_E_FILE_NOT_FOUND);
			mlts_markers(S->ts, &S->ckpt_v_pred, &S->ckpt_ztsnr);      /* what `prediction` / `zsnr` = auto resolve to (guidance_resolve) */
			int wt = -1;
			const char *m = mlts_model_identify(S->ts, &wt);
			if (m) { if (model_type_set_ex(S, model_from(m, strlen(m)), 0) < 0) { mlts_close(S->ts); S->ts = NULL; return MLIS_E_OPT_VALUE; } }
			else if (!(S->flags & CF_MODEL_TYPE_SET)) { mlts_close(S->ts); S->ts = NULL; return api_error(S, MLIS_E_UNKNOWN, "could not detect the model type"); }
			if (wt >= 0 && !(S->flags & CF_WEIGHT_TYPE_SET)) S->wtype = (wt == MLT_F32 || wt == MLT_BF16) ? wt : MLT_F16;   /* quantised GGUF weights: dequantised, kept as F16 */
		}
		if ((S->flags & CF_USE_TAE) && !S->synth && !str_empty(S->path_tae)) {
			S->ts_tae = mlts_open_safetensors(S->path_tae, 0);
			if (!S->ts_tae) { if (S->ts) { mlts_close(S->ts); S->ts = NULL; } return api_error_lib(S, file_exists(S->path_tae) ? MLIS_E_UNKNOWN : MLIS_E_FILE_NOT_FOUND); }
		}
		S->rflags |= READY_MODEL;
		S->rflags &= ~READY_LORAS;
		lora_state_reset(S);
	}
	if (!(S->rflags & READY_LORAS)) {
		/* :1276-1296 merges every active LoRA into a freshly read store and rebuilds what is resident.  Here: the same list of (file, multiplier) as the one the
		 * weights reflect costs nothing (a prompt's <lora:> two generations running); with engines or text towers resident they are patched in place; with
		 * nothing resident, or where the device cannot repeat the host's arithmetic (loras_apply_warm), the adapters are merged on the host like there */
		if (S->ts_partial || !loras_same_as_applied(S)) {
			if (S->synth) return api_error(S, MLIS_E_UNKNOWN, "LoRA needs a checkpoint file (the synthetic models have no tensor store)");
			int r = 0;
			if (!S->ts_partial && (S->eng || S->eng2 || S->tc) && (r = loras_apply_warm(S)) < 0) return r;
			if (!r && (r = loras_apply_cold(S)) < 0) return r;
		}
		S->rflags |= READY_LORAS;
	}
	return 1;
}

/* TAE files carry bare names ("decoder.layers.N..."): the reference prefixes them with "tae." at load
 * (tensor_callback_prefix_add, src/mlimgsynth.c:1057-1066).  Here: lookup with the prefix stripped. */
static int tae_load(MLIS_Ctx* S, MLCtx* C)
{
	const int np = mlctx_param_count(C);
	for (int i=0;i<np;++i) {
		const char *key; int type; int64_t ne[4];
		mlctx_param_info(C, i, &key, &type, ne);
		const MLTSEntry *e = mlts_find(S->ts_tae, !strncmp(key, "tae.", 4) ? key + 4 : key);
		if (!e) return api_error(S, MLIS_E_UNKNOWN, "tensor '%s' not found", key);
		const int64_t cnt = e->shape[0]*e->shape[1]*e->shape[2]*e->shape[3];
		if (cnt != ne[0]*ne[1]*ne[2]*ne[3]) return api_error(S, MLIS_E_UNKNOWN, "tensor '%s': wrong element count", key);
		if (mlctx_param_set(C, key, e->dtype, e->data, cnt) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	}
	return 1;
}

static int ctx_weights(MLIS_Ctx* S, MLCtx* C, int is_tae)
{
	if (S->synth) return mlctx_params_synth(C, S->synth_seed) < 0 ? api_error_lib(S, MLIS_E_UNKNOWN) : 1;
	if (is_tae) { if (!S->ts_tae) return api_error(S, MLIS_E_FILE_NOT_FOUND, "no TAE model set (option TAE)"); return tae_load(S, C); }
	if (mlctx_tstore_load(C, S->ts) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	/* the store is the checkpoint and adapters are active on the device: a plan built now gets them the same way, and so the same weights */
	for (int i=0; !S->ts_merged && i<S->n_applied; ++i) {
		MLTStore *L = mlts_open_lora(S->applied[i].path);
		int r = L ? lora_patch(S, L, S->applied[i].mult, &C, 1) : api_error_lib(S, MLIS_E_UNKNOWN);
		if (L) mlts_close(L);
		if (r < 0) { mlctx_params_unload(C); return r; }
	}
	return 1;
}

static int sampler_defaults(MLIS_Ctx* S, int* n_step, int* method, int* sched)
{
	*n_step = S->n_step >= 1 ? S->n_step : 20;                       /* sampling.c:41-42 */
	*method = S->method > 0 ? S->method : MLIS_METHOD_EULER;         /* :33 */
	*sched = S->sched > 0 ? S->sched : MLIS_SCHED_UNIFORM;           /* :69 */
	return 1;
}

/* the engine for (model, size, batch, guidance on/off, codec), built when none of the two resident ones has that key: the context keeps the
 * engine used last (S->eng) and the one used before it; a third key takes the place of the latter */
/* tiled diffusion: the overlap in effect (auto: a quarter of the tile, rounded down to a multiple of 8), and the refusal of a pair the windows cannot be laid out with */
static int unet_tile_overlap_eff(const MLIS_Ctx* S) { return S->unet_tile_overlap >= 0 ? S->unet_tile_overlap : S->unet_tile / 4 / 8 * 8; }
static int unet_tile_check(MLIS_Ctx* S)
{
	if (S->unet_tile > 0 && 2 * unet_tile_overlap_eff(S) > S->unet_tile)
		return api_error(S, MLIS_E_OPT_VALUE, "invalid unet_tile_overlap %d for unet_tile %d: neighbouring windows can share at most half a tile", unet_tile_overlap_eff(S), S->unet_tile);
	return 1;
}

/* the ControlNet's weights into plans 5 (ControlNet) and 6 (hint block) of the engine just built: "synth[:seed]" with a synthetic model, else a safetensors file in
 * the original layout (its own store: the ControlNet is no part of the checkpoint).  A file of another architecture fails naming the first tensor that is
 * missing or has the wrong element count (mlctx_tstore_load). */
static int control_weights(MLIS_Ctx* S)
{
	const char *p = S->path_control;
	const int is_synth = !strncmp(p, "synth", 5) && (!p[5] || p[5] == ':');
	for (int i=5; i<=6; ++i) {
		MLCtx *C = mlis_amd_ctx_at(S->eng, i);
		if (!C) return api_error(S, MLIS_E_UNKNOWN, "internal: the engine has no ControlNet plan");
		mlctx_set_wtype(C, S->wtype);
		if (is_synth) {
			if (!S->synth) return api_error(S, MLIS_E_OPT_VALUE, "control_model '%s' needs a synth: model (a checkpoint takes a ControlNet file)", p);
			const uint64_t seed = p[5] == ':' ? strtoull(p + 6, NULL, 10) : S->synth_seed;
			if (mlctx_params_synth(C, seed) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
			continue;
		}
		if (!S->ts_control) {
			if (!file_exists(p)) return api_error(S, MLIS_E_FILE_NOT_FOUND, "ControlNet file '%s' not found", p);
			if (!(S->ts_control = mlts_open_controlnet(p))) return api_error_lib(S, MLIS_E_UNKNOWN);
		}
		if (mlctx_tstore_load(C, S->ts_control) < 0) return api_error(S, MLIS_E_UNKNOWN, "ControlNet '%s' does not fit the model %s: %s", p, S->mname, mlsd_last_error());
	}
	return 1;
}

/* Canny of device planes [planes][h][w] into d_dst [3][h][w] (mlsd_canny with the thresholds of mlsd_canny_thresholds and a workspace of its own); waits for the
 * default stream.  0, or mlsd's error */
static int canny_device(const float* d_src, int w, int h, int planes, float low, float high, int l2, int wrap, float* d_dst)
{
	int lo = 0, hi = 0;
	void *d_ws = NULL;
	int r = mlsd_canny_thresholds(low, high, l2, &lo, &hi);
	if (!r) r = mlsd_malloc(&d_ws, mlsd_canny_ws_bytes(w, h));
	if (!r) r = mlsd_canny(d_src, w, h, planes, lo, hi, l2, wrap, d_dst, 3, d_ws, NULL, NULL);
	if (!r) r = mlsd_device_sync();
	if (d_ws) mlsd_free(d_ws);
	return r;
}

/* the control image at the pass's pixel size into the engine (resampled on the GPU: bilinear, as mlis_amd_tensor_resample does, or with the downscale_filter
 * where that is set and an axis shrinks, as mlis_amd_tensor_resample_aa does; then through the control_preprocess at that size, as mlis_amd_tensor_canny does with
 * the tiling as wrap), strength and window */
/* rect (NULL: none, the behaviour of every pass but a masked inpaint's): x0, y0, x1, y1 of a W x H picture that the control image is taken to cover; the image is
 * first cropped (mlsd_window_gather) to the rectangle scaled to its own size, floor(x0 Wc / W) .. ceil(x1 Wc / W) and likewise in y, then treated as ever.  An
 * engine does not keep a cropped image for its next pass. */
static int control_apply(MLIS_Ctx* S, int w_img, int h_img, const int* rect, int W, int H)
{
	if (str_empty(S->path_control)) return 1;
	/* the engine has one pixel size: it still holds this very image, resampled, preprocessed and through the hint plan, unless the option was set again since, the
	 * downscale_filter, the control_preprocess or a canny_* option changed (each counts control_image_gen on) or the tiling changed the edges (another engine) */
	if (!rect && mlis_amd_control_tag(S->eng) == S->control_image_gen)
		return mlis_amd_set_control(S->eng, S->control_strength, S->control_start, S->control_end) < 0 ? api_error_lib(S, MLIS_E_UNKNOWN) : 1;
	const MLIS_Tensor *src = &S->control_image;
	const int Wc = src->n[0], Hc = src->n[1];
	int cx0 = 0, cy0 = 0, sw = Wc, sh = Hc;
	if (rect) {
		cx0 = (int)((int64_t)rect[0] * Wc / W); cy0 = (int)((int64_t)rect[1] * Hc / H);
		sw = (int)(((int64_t)rect[2] * Wc + W - 1) / W) - cx0; sh = (int)(((int64_t)rect[3] * Hc + H - 1) / H) - cy0;
	}
	const size_t n_full = (size_t)3 * Wc * Hc, n_src = (size_t)3 * sw * sh, n_dst = (size_t)3 * w_img * h_img;
	const int aa = S->downscale_filter && (w_img < sw || h_img < sh);
	const int pre = S->control_preprocess;
	void *d_full = NULL, *d_src = NULL, *d_dst = NULL, *d_ws = NULL, *d_pre = NULL;
	int r = 1;
	if (mlsd_malloc(&d_src, n_src * 4) || mlsd_malloc(&d_dst, n_dst * 4) || (pre && mlsd_malloc(&d_pre, n_dst * 4))
			|| (rect ? (mlsd_malloc(&d_full, n_full * 4) || mlsd_memcpy(d_full, src->d, n_full * 4, 0, NULL)
					|| mlsd_window_gather((const float*)d_full, Wc, Hc, (float*)d_src, sw, sh, cx0, cy0, 3, NULL))
				: mlsd_memcpy(d_src, src->d, n_src * 4, 0, NULL))
			|| (aa ? (mlsd_malloc(&d_ws, mlsd_resample2d_aa_ws_bytes(sw, sh, w_img, h_img, 3, S->downscale_filter - 1))
					|| mlsd_resample2d_aa((const float*)d_src, sw, sh, (float*)d_dst, w_img, h_img, 3, S->downscale_filter - 1, S->tiling, d_ws, NULL))
				: mlsd_resample2d((const float*)d_src, sw, sh, (float*)d_dst, w_img, h_img, 3, MLIS_AMD_RESAMPLE_BILINEAR, S->tiling, NULL))
			|| (pre == MLIS_AMD_PREPROCESS_CANNY && canny_device((const float*)d_dst, w_img, h_img, 3, S->canny_low, S->canny_high, S->canny_l2, S->tiling, (float*)d_pre))
			|| (pre == MLIS_AMD_PREPROCESS_INVERT && mlsd_invert((const float*)d_dst, (float*)d_pre, (int64_t)n_dst, NULL))
			|| mlsd_device_sync()
			|| mlis_amd_set_control_image_device(S->eng, pre ? d_pre : d_dst) < 0
			|| mlis_amd_set_control(S->eng, S->control_strength, S->control_start, S->control_end) < 0)
		r = api_error_lib(S, MLIS_E_UNKNOWN);
	if (r > 0) mlis_amd_control_tag_set(S->eng, rect ? 0 : S->control_image_gen);      /* (0 is no image's mark: the next pass takes the image again) */
	if (d_full) mlsd_free(d_full);
	if (d_src) mlsd_free(d_src);
	if (d_dst) mlsd_free(d_dst);
	if (d_ws) mlsd_free(d_ws);
	if (d_pre) mlsd_free(d_pre);
	return r;
}

/* HyperTile: a pass the rule does not touch (unet_hypertile_cuts, host/unet.c, beside the builder whose walk it repeats) takes the plain engine under the plain key:
 * the 512 px first pass of a hires generation with hypertile 512 */
static int hypertile_cuts(const char* model, int lw, int lh, int tile_px, int depth)
{
	UnetParams P;
	if (tile_px <= 0) return 0;
	if (unet_params_get(model, &P) < 0) return 1;
	return unet_hypertile_cuts(&P, lw, lh, tile_px, depth);
}

static int engine_get(MLIS_Ctx* S, int lw, int lh)
{
	const int f = 8, B = S->n_batch > 0 ? S->n_batch : 1, tae = !!(S->flags & CF_USE_TAE);
	const int ctx_tok = S->ctx_tok > 0 ? S->ctx_tok : 77;
	if (unet_tile_check(S) < 0) return MLIS_E_OPT_VALUE;
	/* a size that fits in the tile on both axes gets the plain engine under the plain key: the first pass of a hires generation shares it with untiled use */
	const int tile = (S->unet_tile > 0 && (S->unet_tile < lw * f || S->unet_tile < lh * f)) ? S->unet_tile : 0, overlap = tile ? unet_tile_overlap_eff(S) : 0;
	char key[96];
	int nk = snprintf(key, sizeof(key), "%s/%dx%d/b%d/g%d/t%d/w%d/s%d/c%d/x%d", S->mname, lw, lh, B, S->cfg_scale > 1, tae, S->wtype, !!(S->flags & CF_UNET_SPLIT), ctx_tok, S->tiling);
	if (tile && nk > 0 && nk < (int)sizeof(key)) nk += snprintf(key + nk, sizeof(key) - nk, "/u%do%dp%d", tile, overlap, S->unet_tile_batch);
	const int control = !str_empty(S->path_control);      /* (one ControlNet per context: a changed file drops the engines, so the key only says whether) */
	if (control && nk > 0 && nk < (int)sizeof(key)) nk += snprintf(key + nk, sizeof(key) - nk, "/k1");
	const int freeu = S->freeu != 0;                      /* (the factors are device data of the engine: only on / off is built in) */
	if (freeu && nk > 0 && nk < (int)sizeof(key)) nk += snprintf(key + nk, sizeof(key) - nk, "/f1");
	/* (the UNet plan of a tiled pass has the size of one window: the rule sees that) */
	const int plw = tile && tile / f < lw ? tile / f : lw, plh = tile && tile / f < lh ? tile / f : lh;
	const int hypertile = hypertile_cuts(S->mname, plw, plh, S->hypertile, S->hypertile_depth) ? S->hypertile : 0;
	if (hypertile && nk > 0 && nk < (int)sizeof(key)) nk += snprintf(key + nk, sizeof(key) - nk, "/h%dd%d", hypertile, S->hypertile_depth);
	const int pag = S->pag_scale > 0;                     /* (the scale is an argument of the mix kernels: only on / off is built in) */
	if (pag && nk > 0 && nk < (int)sizeof(key)) snprintf(key + nk, sizeof(key) - nk, "/p1");
	if (pag) {      /* the third row group must fit what an engine holds per plan evaluation: refused here as a bad option value, before anything is built */
		int pk = 1, xs[MLSD_WINDOW_MAX_AXIS];
		if (tile) {
			const int nx = mlis_amd_window_starts(lw, tile / f, overlap / f, S->tiling & 1, xs, MLSD_WINDOW_MAX_AXIS), ny = mlis_amd_window_starts(lh, tile / f, overlap / f, S->tiling & 2, xs, MLSD_WINDOW_MAX_AXIS);
			if (nx > 0 && ny > 0) pk = mlis_amd_tile_pack(nx * ny, B, S->unet_tile_batch, NULL);
		}
		const int rows = mlis_amd_eval_rows(B, S->cfg_scale, 1) * (pk > 0 ? pk : 1);
		if (rows > MLIS_AMD_MAX_EVAL_ROWS) return api_error(S, MLIS_E_OPT_VALUE, "pag_scale: %d rows per UNet evaluation (batch %d), at most %d", rows, B, MLIS_AMD_MAX_EVAL_ROWS);
	}
	int n_step, method, sched;
	sampler_defaults(S, &n_step, &method, &sched);
	/* (a slot serves when its key matches AND it holds a ControlNet exactly if one is wanted: a key cut short by a long model name cannot pass one for the other) */
#define SLOT_IS(e, k) ((e) && !strcmp(key, (k)) && engine_has_control(e) == control && engine_has_freeu(e) == freeu && engine_has_pag(e) == pag)
	if (!SLOT_IS(S->eng, S->eng_key) && SLOT_IS(S->eng2, S->eng2_key)) {      /* the other resident engine: they change places */
		MLIS_AmdCtx *e = S->eng; char k[sizeof(S->eng_key)]; memcpy(k, S->eng_key, sizeof(k));
		S->eng = S->eng2; memcpy(S->eng_key, S->eng2_key, sizeof(k));
		S->eng2 = e; memcpy(S->eng2_key, k, sizeof(k));
	}
	if (!SLOT_IS(S->eng, S->eng_key)) {
#undef SLOT_IS
		if (S->eng) {           /* the engine used last moves to the second slot; what was there, the least recently used one, goes */
			if (S->eng2) mlis_amd_destroy(S->eng2);
			S->eng2 = S->eng; memcpy(S->eng2_key, S->eng_key, sizeof(S->eng_key));
			S->eng = NULL; S->eng_key[0] = 0;
		}
		MLIS_AmdConfig c; memset(&c, 0, sizeof(c));
		c.model = S->mname; c.width = lw * f; c.height = lh * f; c.n_batch = B; c.n_step = n_step; c.cfg_scale = S->cfg_scale;
		c.s_ancestral = S->s_ancestral; c.sched = sched; c.use_tae = tae; c.weight_seed = S->synth_seed; c.method = method;
		c.s_noise = S->s_noise; c.f_t_ini = S->f_t_ini; c.f_t_end = S->f_t_end; c.defer_weights = 1;
		c.unet_split = (S->flags & CF_UNET_SPLIT) ? 1 : 0;      /* MLIS_OPT_UNET_SPLIT (src/mlimgsynth.c:1629 unet_split): the UNet's weights are streamed, not resident */
		c.n_ctx_tok = ctx_tok;                                  /* windowed prompt: the UNet's cross attentions see 77 W context rows */
		c.control = (control ? MLIS_AMD_CONTROL_NET : 0) | (freeu ? MLIS_AMD_CONTROL_FREEU : 0) | MLIS_AMD_CONTROL_HYPERTILE_OF(hypertile, S->hypertile_depth) |
			(pag ? MLIS_AMD_CONTROL_PAG : 0);
		S->eng = mlis_amd_create_tiled_packed(&c, S->tiling, tile, tile, overlap, S->unet_tile_batch, NULL);
		if (!S->eng) return api_error_lib(S, MLIS_E_UNKNOWN);
		S->n_eng_builds++;
		mlctx_set_wtype(mlis_amd_unet_ctx(S->eng), S->wtype);
		if (ctx_weights(S, mlis_amd_unet_ctx(S->eng), 0) < 0 || ctx_weights(S, mlis_amd_decoder_ctx(S->eng), tae) < 0 || (control && control_weights(S) < 0)) {
			mlis_amd_destroy(S->eng); S->eng = NULL; return -1;
		}
		snprintf(S->eng_key, sizeof(S->eng_key), "%s", key);
		if (S->dump_flags & 4) {   /* MLIS_DUMP_GRAPH (src/mlimgsynth.c:432,1298 -> MLB_F_DUMP -> "dump-graph-<name>.txt", src/mlblock.c:111-116) */
			mlctx_block_graph_dump_path(mlis_amd_unet_ctx(S->eng), "dump-graph-unet.txt");
			mlctx_block_graph_dump_path(mlis_amd_decoder_ctx(S->eng), tae ? "dump-graph-tae.txt" : "dump-graph-vae.txt");
		}
	}
	if (mlis_amd_set_sampler(S->eng, n_step, method, sched, S->cfg_scale, S->s_ancestral, S->s_noise, S->f_t_ini, S->f_t_end) < 0)
		return api_error_lib(S, MLIS_E_OPT_VALUE);
	/* VAE_TILE (:1318,1345): tile-sized decoder plan, weights loaded like the full-size one */
	mlis_amd_set_vae_tile(S->eng, S->vae_tile);
	MLCtx *tc = mlis_amd_decoder_tile_prepare(S->eng);
	if (tc && !mlctx_params_loaded(tc) && ctx_weights(S, tc, 0) < 0) return -1;
	return 1;
}

static int textcond_get(MLIS_Ctx* S, int w, int h)
{
	char key[64];
	snprintf(key, sizeof(key), "%s/skip%d", S->mname, S->clip_skip);
	if (!S->tc || strcmp(key, S->tc_key)) {
		textcond_drop(S);
		S->tc = mlis_amd_textcond_create_ex(S->mname, w, h, S->synth_seed, NULL, S->clip_skip, 1);
		if (!S->tc) return api_error_lib(S, MLIS_E_UNKNOWN);
		for (int i=0;i<mlis_amd_textcond_n_towers(S->tc);++i)
			if (ctx_weights(S, mlis_amd_textcond_ctx(S->tc, i), 0) < 0) { textcond_drop(S); return -1; }
		snprintf(S->tc_key, sizeof(S->tc_key), "%s", key);
	}
	mlis_amd_textcond_set_size(S->tc, w, h);
	return 1;
}

/* ------------------------------------------------------------------ text */
static int tokenizer_get(MLIS_Ctx* S)
{
	if (S->tok) return 1;
	static const char* const names[] = { "bpe_simple_vocab_16e6.txt", "merges.txt", "clip_merges.txt" };
	static const char* const dirs[] = { NULL, ".", "/usr/share/mlimgsynth", "/usr/local/share/mlimgsynth" };   /* mlis_file_find :711-735 */
	char path[1024];
	for (int d=0; d<4; ++d) for (int n=0; n<3; ++n) {
		const char *dir = d == 0 ? S->path_aux : dirs[d];
		if (str_empty(dir)) continue;
		snprintf(path, sizeof(path), "%s/%s", dir, names[n]);
		if (!file_exists(path)) continue;
		S->tok = clip_tokr_new();
		if (clip_tokr_load_merges_txt(S->tok, path, 0) < 0) { clip_tokr_free(S->tok); S->tok = NULL; return api_error_lib(S, MLIS_E_UNKNOWN); }
		return 1;
	}
	return api_error(S, MLIS_E_FILE_NOT_FOUND, "CLIP vocabulary not found: put bpe_simple_vocab_16e6.txt (or merges.txt) in the AUX_DIR directory");
}

/* mlis_prompt_text_tokenize :1367-1403: chunks are tokenized one by one, every token carries its chunk's weight */
static int prompt_tokenize(MLIS_Ctx* S, const MLISPrompt* P, int32_t** ptok, float** pw)
{
	int n = 0, cap = 128;
	int32_t *tok = (int32_t*)malloc(sizeof(int32_t) * cap); float *w = (float*)malloc(sizeof(float) * cap);
	int nonempty = 0;
	for (int i=0;i<P->n_chunk;++i) if (P->chunks[i].len > 0) nonempty = 1;
	if (nonempty) { int r = tokenizer_get(S); if (r < 0) { free(tok); free(w); return r; } }
	for (int i=0; i<P->n_chunk && nonempty; ++i) {
		int32_t buf[512];
		int k = clip_tokenize(S->tok, P->text + P->chunks[i].begin, P->chunks[i].len, buf, 512);
		if (k < 0) { free(tok); free(w); return api_error_lib(S, MLIS_E_UNKNOWN); }
		if (n + k > cap) { cap = (n + k) * 2; tok = (int32_t*)realloc(tok, sizeof(int32_t)*cap); w = (float*)realloc(w, sizeof(float)*cap); }
		for (int j=0;j<k;++j) { tok[n+j] = buf[j]; w[n+j] = P->chunks[i].w; }
		n += k;
	}
	*ptok = tok; *pw = w;
	return n;
}

MLB_API int mlis_text_tokenize(MLIS_Ctx* S, const char* text, int32_t** ptokens, MLIS_SubModel model)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	if (model != MLIS_SUBMODEL_CLIP && model != MLIS_SUBMODEL_CLIP2) return api_error(S, MLIS_E_UNKNOWN, "invalid model for text tokenization: %d", model);
	mlis_prompt_set_raw(&S->prompt, text);                            /* prompt_text_set_raw (:1411) */
	free(S->tokens); free(S->tokens_w); S->tokens = NULL; S->tokens_w = NULL;
	int n = prompt_tokenize(S, &S->prompt, &S->tokens, &S->tokens_w);
	if (n < 0) return n;
	S->n_tokens = n;
	if (ptokens) *ptokens = S->tokens;
	return n;
}

MLB_API int mlis_clip_text_encode(MLIS_Ctx* S, const char* text, MLIS_Tensor* embed, MLIS_Tensor* feat, MLIS_SubModel model, int flags)
{	/* :1470-1483 -> mlis_clip_tokens_encode: one tower, clip_skip option, final norm unless MLIS_CTEF_NO_NORM */
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	int r = mlis_setup(S); if (r < 0) return r;
	int32_t *tk = NULL;
	int n = mlis_text_tokenize(S, text, &tk, model); if (n < 0) return n;
	const int xl = !strcmp(S->mname, "sdxl") || !strcmp(S->mname, "tinyxl");
	if (model == MLIS_SUBMODEL_CLIP2 && !xl) return api_error(S, MLIS_E_UNKNOWN, "invalid model for text tokenize: %d", model);
	const char *tower = model == MLIS_SUBMODEL_CLIP2 ? (S->mname[0] == 's' ? "vit_bigg" : "tiny")
		: (!strcmp(S->mname, "sd2") ? "vit_h" : (S->mname[0] == 's' ? "vit_l" : "tiny"));
	ClipParams P; if (clip_params_get(tower, &P) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	MLCtx *C = mlctx_new(NULL);
	ClipEncoder E;
	r = clip_encoder_init(&E, C, &P, model == MLIS_SUBMODEL_CLIP2 ? "clip2" : "clip", 1, S->clip_skip, !(flags & MLIS_CTEF_NO_NORM), feat != NULL);
	if (r > 0) r = ctx_weights(S, C, 0); else api_error_lib(S, MLIS_E_UNKNOWN);
	if (r > 0) {
		if (embed) mlis_tensor_resize(embed, P.d_embed, P.n_token, 1, 1);
		if (feat) mlis_tensor_resize(feat, P.d_embed, 1, 1, 1);
		r = clip_encoder_run(&E, (unsigned)n, tk, embed ? embed->d : NULL, feat ? feat->d : NULL);
		if (r < 0) api_error_lib(S, MLIS_E_UNKNOWN);
	}
	clip_encoder_free(&E); mlctx_destroy(C);
	return r < 0 ? r : 1;
}

/* tokens + emphasis weights of the prompt (neg = 0) or the negative prompt: explicit ids or the parsed prompt text */
static int prompt_tokens(MLIS_Ctx* S, int neg, int32_t** ptok, float** ptw)
{
	if (S->have_ptok[neg]) {
		const int n = S->n_ptok[neg];
		*ptok = (int32_t*)malloc(sizeof(int32_t)*(n ? n : 1)); *ptw = (float*)malloc(sizeof(float)*(n ? n : 1));
		memcpy(*ptok, S->ptok[neg], sizeof(int32_t)*n); memcpy(*ptw, S->ptokw[neg], sizeof(float)*n);
		return n;
	}
	MLISPrompt *P = neg ? &S->nprompt : &S->prompt;
	if (!P->n_chunk) mlis_prompt_set_raw(P, "");
	return prompt_tokenize(S, P, ptok, ptw);
}

/* mlis_text_cond_encode :1501-1563 for the prompt and (with_neg) the negative prompt: one run per tower for both */
static int text_cond_encode(MLIS_Ctx* S, int with_neg, int w, int h)
{
	int32_t *tok[2] = {NULL, NULL}; float *tw[2] = {NULL, NULL}; int n[2] = {0, 0};
	int r = -1;
	if ((n[0] = prompt_tokens(S, 0, &tok[0], &tw[0])) < 0) { r = n[0]; goto end; }
	if (with_neg && (n[1] = prompt_tokens(S, 1, &tok[1], &tw[1])) < 0) { r = n[1]; goto end; }
	if (textcond_get(S, w, h) < 0) goto end;
	int n_ctx = 0, n_label = 0, W = 0;
	mlis_amd_textcond_dims(S->tc, &n_ctx, &n_label);
	/* prompts of more than 75 tokens: 75-token windows, cond / ncond [n_ctx, 77 W] with the same W on both sides (CFG batches them) */
	for (int p=0; p<1+!!with_neg; ++p) {
		const int Wp = mlis_amd_prompt_windows(n[p], NULL, NULL);
		if (Wp < 0) { r = api_error_lib(S, MLIS_E_UNKNOWN); goto end; }
		if (Wp > W) W = Wp;
	}
	mlis_tensor_resize(&S->cond, n_ctx, 77 * W, 1, 1);
	if (n_label) mlis_tensor_resize(&S->label, n_label, 1, 1, 1);
	if (with_neg) {
		mlis_tensor_resize(&S->ncond, n_ctx, 77 * W, 1, 1);
		if (n_label) mlis_tensor_resize(&S->nlabel, n_label, 1, 1, 1);
		r = mlis_amd_textcond_encode_pair_ex(S->tc, tok[0], tw[0], n[0], tok[1], tw[1], n[1], S->cond.d, n_label ? S->label.d : NULL,
			S->ncond.d, n_label ? S->nlabel.d : NULL);
	} else r = mlis_amd_textcond_encode_ex(S->tc, tok[0], tw[0], n[0], S->cond.d, n_label ? S->label.d : NULL);
	if (r < 0) r = api_error_lib(S, MLIS_E_UNKNOWN);
end:
	free(tok[0]); free(tw[0]); free(tok[1]); free(tw[1]);
	return r < 0 ? r : 1;
}

/* ------------------------------------------------------------------ codec */
static int progress(MLIS_Ctx* S, MLIS_Stage stage, int step, int step_end)
{	/* mlis_callback :614-629 */
	const double t = now_s();
	S->prg.stage = stage; S->prg.step = step; S->prg.step_end = step_end; S->prg.step_time = t - S->t_last; S->prg.time = t;
	S->t_last = t;
	if (S->callback) { int r = S->callback(S->callback_ud, S, &S->prg); if (r < 0) return r; }
	return 1;
}

MLB_API int mlis_mask_encode(MLIS_Ctx* S, const MLIS_Tensor* mask, MLIS_Tensor* lmask, int flags)
{	/* ltensor_downsize(lmask, mask, f, f, 1, 1): box average (src/localtensor.c:161-194) */
	(void)flags;
	const int f = 8, w = mask->n[0], h = mask->n[1], lw = w / f, lh = h / f;
	float *out = (float*)malloc(sizeof(float) * ((size_t)lw*lh + 1));
	const float fn = 1.0f / (f*f);
	for (int i1=0;i1<lh;++i1) for (int i0=0;i0<lw;++i0) {
		float v = 0;
		for (int j1=0;j1<f;++j1) for (int j0=0;j0<f;++j0) v += mask->d[i0*f + j0 + (size_t)(i1*f + j1)*w];
		out[i0 + (size_t)i1*lw] = v * fn;
	}
	mlis_tensor_resize(lmask, lw, lh, 1, 1);
	memcpy(lmask->d, out, sizeof(float) * (size_t)lw * lh);
	free(out);
	(void)S;
	return 1;
}

/* seamless tiling needs the whole image in one plan: the tiles of VAE_TILE cannot see the opposite edge (TAESD is never tiled) */
static int tiling_check(MLIS_Ctx* S)
{
	if (S->tiling && S->vae_tile > 0 && !(S->flags & CF_USE_TAE))
		return api_error(S, MLIS_E_OPT_VALUE, "tiling '%s' cannot be combined with vae_tile %d (tiled VAE decoding / encoding does not wrap)", k_tiling[S->tiling], S->vae_tile);
	return 1;
}

static int engine_for_image(MLIS_Ctx* S, int w, int h)
{
	if (w % 8 || h % 8 || w < 8 || h < 8) return api_error(S, MLIS_E_IMAGE, "invalid input image shape: %dx%d", w, h);
	return engine_get(S, w / 8, h / 8);
}

MLB_API int mlis_image_encode(MLIS_Ctx* S, const MLIS_Tensor* image, MLIS_Tensor* latent, int flags)
{	/* :1301-1330; batch: the same image for every batch element, or (n[3] == BATCH_SIZE: the hires fix with an upscale model) one image each */
	(void)flags;
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	int r = mlis_setup(S); if (r < 0) return r;
	const int Bi = S->n_batch > 0 ? S->n_batch : 1;
	if (image->n[2] != 3 || (image->n[3] != 1 && image->n[3] != Bi)) return api_error(S, MLIS_E_IMAGE, "invalid input image shape: %dx%dx%dx%d", image->n[0], image->n[1], image->n[2], image->n[3]);
	const int w = image->n[0], h = image->n[1];
	if ((r = tiling_check(S)) < 0) return r;
	if (engine_for_image(S, w, h) < 0) return -1;
	MLCtx *ec = mlis_amd_encoder_tile_prepare(S->eng);          /* VAE_TILE: the tile-sized encoder, when tiling applies */
	if (!ec) ec = mlis_amd_encoder_ctx(S->eng);
	if (!ec) ec = mlis_amd_encoder_prepare(S->eng);
	if (!ec) return api_error_lib(S, MLIS_E_UNKNOWN);
	if (!mlctx_params_loaded(ec) && ctx_weights(S, ec, !!(S->flags & CF_USE_TAE)) < 0) return -1;
	const int B = S->n_batch > 0 ? S->n_batch : 1;
	const size_t per = (size_t)3 * w * h;
	float *imgs = (float*)malloc(per * B * 4);
	for (int b=0;b<B;++b) memcpy(imgs + per*b, image->d + (image->n[3] == B ? per*b : 0), per*4);
	uint64_t seeds[MAX_IMAGES]; for (int b=0;b<B && b<MAX_IMAGES;++b) seeds[b] = S->seed + b;
	mlis_amd_seed_ex(S->eng, seeds, S->rng_offset);
	r = mlis_amd_encode(S->eng, imgs, 1);
	free(imgs);
	if (r < 0) return api_error_lib(S, r == MLIS_E_NAN ? MLIS_E_NAN : MLIS_E_UNKNOWN);
	S->rng_offset = mlis_amd_rng_offset(S->eng);
	const int n_lat = image->n[3];      /* one latent per image given */
	mlis_tensor_resize(latent, w/8, h/8, 4, n_lat);
	if (mlsd_memcpy(latent->d, mlis_amd_latent_device(S->eng), (size_t)n_lat*4*(w/8)*(h/8)*4, 1, NULL) || mlsd_device_sync()) return api_error_lib(S, MLIS_E_UNKNOWN);
	return progress(S, MLIS_STAGE_IMAGE_ENCODE, 1, 1);
}

static int image_fetch(MLIS_Ctx* S, MLIS_Tensor* image, int w, int h)
{
	const int B = S->n_batch > 0 ? S->n_batch : 1;
	mlis_tensor_resize(image, w, h, 3, B);
	if (mlis_amd_sync(S->eng) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);        /* the decode was enqueued on the engine's own stream */
	if (mlsd_memcpy(image->d, mlis_amd_image_device(S->eng), (size_t)B*3*w*h*4, 1, NULL) || mlsd_device_sync()) return api_error_lib(S, MLIS_E_UNKNOWN);
	const size_t n = mlis_tensor_count(image);
	for (size_t i=0;i<n;++i) if (!isfinite(image->d[i])) return api_error(S, MLIS_E_NAN, "NaN found in decoded image");   /* :1348-1349 */
	image->flags |= LT_F_READY;
	return 1;
}

MLB_API int mlis_image_decode(MLIS_Ctx* S, const MLIS_Tensor* latent, MLIS_Tensor* image, int flags)
{	/* :1332-1357; the latent of batch element 0 is replicated when the tensor holds one image */
	(void)flags;
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	int r = mlis_setup(S); if (r < 0) return r;
	if (latent->n[2] != 4) return api_error(S, MLIS_E_UNKNOWN, "latent must have 4 channels");
	const int lw = latent->n[0], lh = latent->n[1], B = S->n_batch > 0 ? S->n_batch : 1;
	if ((r = tiling_check(S)) < 0) return r;
	if (engine_get(S, lw, lh) < 0) return -1;
	const size_t per = (size_t)4*lw*lh;
	float *l = (float*)malloc(per * B * 4);
	for (int b=0;b<B;++b) memcpy(l + per*b, latent->d + (latent->n[3] == B ? per*b : 0), per*4);
	r = mlis_amd_set_init_latent(S->eng, l);
	free(l);
	if (r < 0 || mlis_amd_decode(S->eng) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	mlis_amd_set_init_latent(S->eng, NULL);
	if (image_fetch(S, image, lw*8, lh*8) < 0) return -1;
	return progress(S, MLIS_STAGE_IMAGE_DECODE, 1, 1);
}

/* ------------------------------------------------------------------ resampling */
/* host tensor -> device, mlsd_resample2d, -> host tensor; src may be dst (it is on the device before dst is resized) */
static int tensor_resample(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, int w, int h, int mode)
{
	if (mode < MLIS_AMD_RESAMPLE_NEAREST || mode > MLIS_AMD_RESAMPLE_BICUBIC) return api_error(S, MLIS_E_OPT_VALUE, "invalid resampling mode %d", mode);
	if (!src || !dst || !tensor_good(src) || src->n[0] < 1 || src->n[1] < 1 || src->n[2] < 1 || src->n[3] < 1)
		return api_error(S, MLIS_E_OPT_VALUE, "invalid tensor to resample");
	const int sw = src->n[0], sh = src->n[1], c = src->n[2], b = src->n[3];
	const size_t n_src = mlis_tensor_count(src), n_dst = (size_t)c * b * (w > 0 ? w : 0) * (h > 0 ? h : 0);
	if (w < 1 || h < 1 || w > 65535 || h > 65535 || n_src >= ((size_t)1 << 31) || n_dst >= ((size_t)1 << 31))
		return api_error(S, MLIS_E_OPT_VALUE, "invalid size to resample to: %dx%d", w, h);
	int r = backend_setup(S); if (r < 0) return r;
	void *d_src = NULL, *d_dst = NULL;
	if (mlsd_malloc(&d_src, n_src * 4) || mlsd_malloc(&d_dst, n_dst * 4) || mlsd_memcpy(d_src, src->d, n_src * 4, 0, NULL)
			|| mlsd_resample2d((const float*)d_src, sw, sh, (float*)d_dst, w, h, c * b, mode, S->tiling, NULL))
		r = api_error_lib(S, MLIS_E_UNKNOWN);
	if (r > 0) {
		mlis_tensor_resize(dst, w, h, c, b);
		if (mlsd_memcpy(dst->d, d_dst, n_dst * 4, 1, NULL) || mlsd_device_sync()) r = api_error_lib(S, MLIS_E_UNKNOWN);
	}
	if (d_src) mlsd_free(d_src);
	if (d_dst) mlsd_free(d_dst);
	return r;
}

MLB_API int mlis_amd_tensor_resample(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, int w, int h, int mode)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	return tensor_resample(S, src, dst, w, h, mode);
}

/* the same through mlsd_resample2d_aa (filter: MLIS_AMD_AA_*) */
static int tensor_resample_aa(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, int w, int h, int filter)
{
	if (filter < MLIS_AMD_AA_BOX || filter > MLIS_AMD_AA_LANCZOS) return api_error(S, MLIS_E_OPT_VALUE, "invalid resampling filter %d", filter);
	if (!src || !dst || !tensor_good(src) || src->n[0] < 1 || src->n[1] < 1 || src->n[2] < 1 || src->n[3] < 1)
		return api_error(S, MLIS_E_OPT_VALUE, "invalid tensor to resample");
	const int sw = src->n[0], sh = src->n[1], c = src->n[2], b = src->n[3];
	const size_t n_src = mlis_tensor_count(src), n_dst = (size_t)c * b * (w > 0 ? w : 0) * (h > 0 ? h : 0), n_mid = (size_t)c * b * sh * (w > 0 ? w : 0);
	if (w < 1 || h < 1 || w > 65535 || h > 65535 || n_src >= ((size_t)1 << 31) || n_dst >= ((size_t)1 << 31) || n_mid >= ((size_t)1 << 31))
		return api_error(S, MLIS_E_OPT_VALUE, "invalid size to resample to: %dx%d", w, h);
	int r = backend_setup(S); if (r < 0) return r;
	void *d_src = NULL, *d_dst = NULL, *d_ws = NULL;
	if (mlsd_malloc(&d_src, n_src * 4) || mlsd_malloc(&d_dst, n_dst * 4) || mlsd_malloc(&d_ws, mlsd_resample2d_aa_ws_bytes(sw, sh, w, h, c * b, filter))
			|| mlsd_memcpy(d_src, src->d, n_src * 4, 0, NULL)
			|| mlsd_resample2d_aa((const float*)d_src, sw, sh, (float*)d_dst, w, h, c * b, filter, S->tiling, d_ws, NULL))
		r = api_error_lib(S, MLIS_E_UNKNOWN);
	if (r > 0) {
		mlis_tensor_resize(dst, w, h, c, b);
		if (mlsd_memcpy(dst->d, d_dst, n_dst * 4, 1, NULL) || mlsd_device_sync()) r = api_error_lib(S, MLIS_E_UNKNOWN);
	}
	if (d_src) mlsd_free(d_src);
	if (d_dst) mlsd_free(d_dst);
	if (d_ws) mlsd_free(d_ws);
	return r;
}

MLB_API int mlis_amd_tensor_resample_aa(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, int w, int h, int filter)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	return tensor_resample_aa(S, src, dst, w, h, filter);
}

/* ------------------------------------------------------------------ control image preprocessor (hip/canny.hip) */
/* host tensor -> device, mlsd_canny, -> host tensor [w][h][3][1]; src may be dst */
MLB_API int mlis_amd_tensor_canny(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, float low, float high, int l2, int wrap)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	if (!src || !dst || !tensor_good(src) || src->n[0] < 1 || src->n[1] < 1 || (src->n[2] != 1 && src->n[2] != 3) || src->n[3] != 1)
		return api_error(S, MLIS_E_OPT_VALUE, "invalid tensor for canny (one image of 1 or 3 channels)");
	if (!(low >= 0 && low <= 32767) || !(high >= 0 && high <= 32767) || (l2 & ~1) || (wrap & ~3))
		return api_error(S, MLIS_E_OPT_VALUE, "invalid canny arguments: low %g, high %g (0 .. 32767), l2 %d (0, 1), wrap %d (0 .. 3)", low, high, l2, wrap);
	const int w = src->n[0], h = src->n[1], c = src->n[2];
	const size_t n = (size_t)w * h;
	if (!mlsd_canny_ws_bytes(w, h)) return api_error(S, MLIS_E_OPT_VALUE, "invalid size for canny: %dx%d", w, h);
	int r = backend_setup(S); if (r < 0) return r;
	void *d_src = NULL, *d_dst = NULL;
	if (mlsd_malloc(&d_src, n * c * 4) || mlsd_malloc(&d_dst, n * 3 * 4) || mlsd_memcpy(d_src, src->d, n * c * 4, 0, NULL)
			|| canny_device((const float*)d_src, w, h, c, low, high, l2, wrap, (float*)d_dst))
		r = api_error_lib(S, MLIS_E_UNKNOWN);
	if (r > 0) {
		mlis_tensor_resize(dst, w, h, 3, 1);
		if (mlsd_memcpy(dst->d, d_dst, n * 3 * 4, 1, NULL) || mlsd_device_sync()) r = api_error_lib(S, MLIS_E_UNKNOWN);
	}
	if (d_src) mlsd_free(d_src);
	if (d_dst) mlsd_free(d_dst);
	return r;
}

/* ------------------------------------------------------------------ region inpainting, piece by piece (hip/inpaint.hip) */
/* each: host tensor -> device, one mlsd_ call, -> host tensor; src may be dst (it is on the device before dst is resized) */
enum { MASK_OP_WEIGHT, MASK_OP_GROW, MASK_OP_BLUR };
static int tensor_mask_op(MLIS_Ctx* S, int op, const MLIS_Tensor* src, MLIS_Tensor* dst, int iarg, float farg, int wrap)
{
	static const char* const names[] = { "mask_weight", "mask_grow", "gauss_blur" };
	if (!src || !dst || !tensor_good(src) || src->n[0] < 1 || src->n[1] < 1 || src->n[2] < 1 || src->n[3] < 1 || mlis_tensor_count(src) >= ((size_t)1 << 31)
			|| (op == MASK_OP_GROW && (src->n[2] != 1 || src->n[3] != 1)))
		return api_error(S, MLIS_E_OPT_VALUE, "invalid tensor for %s%s", names[op], op == MASK_OP_GROW ? " (one plane)" : "");
	if ((wrap & ~3) || (op == MASK_OP_WEIGHT && (iarg & ~1)) || (op == MASK_OP_GROW && (iarg < -MLSD_MASK_GROW_MAX || iarg > MLSD_MASK_GROW_MAX))
			|| (op == MASK_OP_BLUR && !(farg >= 0 && farg <= MLSD_GAUSS_MAX_SIGMA)))
		return api_error(S, MLIS_E_OPT_VALUE, "invalid %s arguments: %d, %g, wrap %d", names[op], iarg, farg, wrap);
	const int w = src->n[0], h = src->n[1], c = src->n[2], b = src->n[3];
	const size_t n = mlis_tensor_count(src);
	int r = backend_setup(S); if (r < 0) return r;
	void *d_src = NULL, *d_dst = NULL, *d_ws = NULL;
	if (mlsd_malloc(&d_src, n * 4) || mlsd_malloc(&d_dst, n * 4) || mlsd_memcpy(d_src, src->d, n * 4, 0, NULL)
			|| (op == MASK_OP_WEIGHT && mlsd_mask_weight((const float*)d_src, (float*)d_dst, (int64_t)n, iarg, NULL))
			|| (op == MASK_OP_GROW && (mlsd_malloc(&d_ws, n * 4) || mlsd_mask_grow((const float*)d_src, (float*)d_dst, w, h, iarg, wrap, d_ws, NULL)))
			|| (op == MASK_OP_BLUR && (mlsd_malloc(&d_ws, mlsd_gauss_blur_ws_bytes(w, h, c * b)) || mlsd_gauss_blur((const float*)d_src, (float*)d_dst, w, h, c * b, farg, wrap, d_ws, NULL))))
		r = api_error_lib(S, MLIS_E_UNKNOWN);
	if (r > 0) {
		mlis_tensor_resize(dst, w, h, c, b);
		if (mlsd_memcpy(dst->d, d_dst, n * 4, 1, NULL) || mlsd_device_sync()) r = api_error_lib(S, MLIS_E_UNKNOWN);
	}
	if (d_src) mlsd_free(d_src);
	if (d_dst) mlsd_free(d_dst);
	if (d_ws) mlsd_free(d_ws);
	return r;
}

static int tensor_mask_bbox(MLIS_Ctx* S, const MLIS_Tensor* src, int bbox[4])
{
	if (!src || !bbox || !tensor_good(src) || src->n[0] < 1 || src->n[1] < 1 || src->n[2] != 1 || src->n[3] != 1 || mlis_tensor_count(src) >= ((size_t)1 << 31))
		return api_error(S, MLIS_E_OPT_VALUE, "invalid tensor for mask_bbox (one plane)");
	const size_t n = mlis_tensor_count(src);
	int r = backend_setup(S); if (r < 0) return r;
	void *d_src = NULL, *d_box = NULL;
	if (mlsd_malloc(&d_src, n * 4) || mlsd_malloc(&d_box, 4 * sizeof(int)) || mlsd_memcpy(d_src, src->d, n * 4, 0, NULL)
			|| mlsd_mask_bbox((const float*)d_src, src->n[0], src->n[1], (int*)d_box, NULL) || mlsd_memcpy(bbox, d_box, 4 * sizeof(int), 1, NULL) || mlsd_device_sync())
		r = api_error_lib(S, MLIS_E_UNKNOWN);
	if (d_src) mlsd_free(d_src);
	if (d_box) mlsd_free(d_box);
	return r;
}

/* dst may be orig or patch: all three inputs are on the device before dst is resized */
static int tensor_composite(MLIS_Ctx* S, MLIS_Tensor* dst, const MLIS_Tensor* orig, const MLIS_Tensor* patch, const MLIS_Tensor* p, int x0, int y0)
{
	if (!dst || !orig || !patch || !p || !tensor_good(orig) || !tensor_good(patch) || !tensor_good(p))
		return api_error(S, MLIS_E_OPT_VALUE, "invalid tensor for composite");
	const int W = orig->n[0], H = orig->n[1], c = orig->n[2], B = patch->n[3], cw = patch->n[0], ch = patch->n[1];
	if (W < 1 || H < 1 || c < 1 || B < 1 || patch->n[2] != c || (orig->n[3] != 1 && orig->n[3] != B) || p->n[0] != W || p->n[1] != H || p->n[2] != 1 || p->n[3] != 1
			|| (double)W * H * c * B >= 2147483648.0)
		return api_error(S, MLIS_E_OPT_VALUE, "composite: orig %dx%dx%dx%d, patch %dx%dx%dx%d and p %dx%dx%dx%d do not fit together", orig->n[0], orig->n[1], orig->n[2], orig->n[3],
			patch->n[0], patch->n[1], patch->n[2], patch->n[3], p->n[0], p->n[1], p->n[2], p->n[3]);
	if (cw < 1 || ch < 1 || x0 < 0 || y0 < 0 || cw > W - x0 || ch > H - y0)
		return api_error(S, MLIS_E_OPT_VALUE, "composite: a patch of %dx%d at (%d, %d) does not lie inside the %dx%d image", cw, ch, x0, y0, W, H);
	const int n_orig = orig->n[3];
	const size_t n_dst = (size_t)W * H * c * B, n_o = (size_t)W * H * c * n_orig, n_patch = mlis_tensor_count(patch), n_p = (size_t)W * H;
	int r = backend_setup(S); if (r < 0) return r;
	void *d_dst = NULL, *d_orig = NULL, *d_patch = NULL, *d_p = NULL;
	if (mlsd_malloc(&d_dst, n_dst * 4) || mlsd_malloc(&d_orig, n_o * 4) || mlsd_malloc(&d_patch, n_patch * 4) || mlsd_malloc(&d_p, n_p * 4)
			|| mlsd_memcpy(d_orig, orig->d, n_o * 4, 0, NULL) || mlsd_memcpy(d_patch, patch->d, n_patch * 4, 0, NULL) || mlsd_memcpy(d_p, p->d, n_p * 4, 0, NULL)
			|| mlsd_composite((float*)d_dst, (const float*)d_orig, n_orig, (const float*)d_patch, (const float*)d_p, W, H, c, B, x0, y0, cw, ch, NULL))
		r = api_error_lib(S, MLIS_E_UNKNOWN);
	if (r > 0) {
		mlis_tensor_resize(dst, W, H, c, B);
		if (mlsd_memcpy(dst->d, d_dst, n_dst * 4, 1, NULL) || mlsd_device_sync()) r = api_error_lib(S, MLIS_E_UNKNOWN);
	}
	if (d_dst) mlsd_free(d_dst);
	if (d_orig) mlsd_free(d_orig);
	if (d_patch) mlsd_free(d_patch);
	if (d_p) mlsd_free(d_p);
	return r;
}

/* dst = the cw x ch window of every plane of src at (x0, y0), inside the image (mlsd_window_gather); src may be dst */
static int tensor_crop(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, int x0, int y0, int cw, int ch)
{
	const int W = src->n[0], H = src->n[1], c = src->n[2], b = src->n[3];
	if (cw < 1 || ch < 1 || x0 < 0 || y0 < 0 || cw > W - x0 || ch > H - y0) return api_error(S, MLIS_E_OPT_VALUE, "crop: %dx%d at (%d, %d) of a %dx%d image", cw, ch, x0, y0, W, H);
	const size_t n_src = mlis_tensor_count(src), n_dst = (size_t)cw * ch * c * b;
	int r = backend_setup(S); if (r < 0) return r;
	void *d_src = NULL, *d_dst = NULL;
	if (mlsd_malloc(&d_src, n_src * 4) || mlsd_malloc(&d_dst, n_dst * 4) || mlsd_memcpy(d_src, src->d, n_src * 4, 0, NULL)
			|| mlsd_window_gather((const float*)d_src, W, H, (float*)d_dst, cw, ch, x0, y0, c * b, NULL))
		r = api_error_lib(S, MLIS_E_UNKNOWN);
	if (r > 0) {
		mlis_tensor_resize(dst, cw, ch, c, b);
		if (mlsd_memcpy(dst->d, d_dst, n_dst * 4, 1, NULL) || mlsd_device_sync()) r = api_error_lib(S, MLIS_E_UNKNOWN);
	}
	if (d_src) mlsd_free(d_src);
	if (d_dst) mlsd_free(d_dst);
	return r;
}

MLB_API int mlis_amd_tensor_mask_weight(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, int invert)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	return tensor_mask_op(S, MASK_OP_WEIGHT, src, dst, invert, 0, 0);
}
MLB_API int mlis_amd_tensor_mask_grow(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, int radius, int wrap)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	return tensor_mask_op(S, MASK_OP_GROW, src, dst, radius, 0, wrap);
}
MLB_API int mlis_amd_tensor_gauss_blur(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst, float sigma, int wrap)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	return tensor_mask_op(S, MASK_OP_BLUR, src, dst, 0, sigma, wrap);
}
MLB_API int mlis_amd_tensor_mask_bbox(MLIS_Ctx* S, const MLIS_Tensor* src, int bbox[4])
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	return tensor_mask_bbox(S, src, bbox);
}
MLB_API int mlis_amd_tensor_composite(MLIS_Ctx* S, MLIS_Tensor* dst, const MLIS_Tensor* orig, const MLIS_Tensor* patch, const MLIS_Tensor* p, int x0, int y0)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	return tensor_composite(S, dst, orig, patch, p, x0, y0);
}

/* the region rule (mlis_abi.h) */
MLB_API int mlis_amd_inpaint_region(int W, int H, const int bbox[4], int padding, int tw, int th, int out[4])
{
	if (!bbox || !out || W < 1 || H < 1 || tw < 1 || th < 1 || padding < 0) return -1;
	if (bbox[0] < 0 || bbox[1] < 0 || bbox[2] > W || bbox[3] > H || bbox[0] >= bbox[2] || bbox[1] >= bbox[3]) return -1;
	int64_t x0 = (int64_t)bbox[0] - padding, y0 = (int64_t)bbox[1] - padding, x1 = (int64_t)bbox[2] + padding, y1 = (int64_t)bbox[3] + padding;
	if (x0 < 0) x0 = 0;
	if (y0 < 0) y0 = 0;
	if (x1 > W) x1 = W;
	if (y1 > H) y1 = H;
	int64_t cw = x1 - x0, ch = y1 - y0;
	if (cw * th < ch * tw) {
		int64_t n = (ch * tw + th - 1) / th; if (n > W) n = W;
		x0 -= (n - cw) / 2; cw = n;
		if (x0 < 0) x0 = 0;
		if (x0 + cw > W) x0 = W - cw;
	} else {
		int64_t n = (cw * th + tw - 1) / tw; if (n > H) n = H;
		y0 -= (n - ch) / 2; ch = n;
		if (y0 < 0) y0 = 0;
		if (y0 + ch > H) y0 = H - ch;
	}
	out[0] = (int)x0; out[1] = (int)y0; out[2] = (int)(x0 + cw); out[3] = (int)(y0 + ch);
	return 1;
}

MLB_API int mlis_amd_inpaint_info(MLIS_Ctx* S, int region[4], int proc[2])
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	for (int i=0; region && i<4; ++i) region[i] = S->inp_done ? S->inp_region[i] : 0;
	for (int i=0; proc && i<2; ++i) proc[i] = S->inp_done ? S->inp_proc[i] : 0;
	return S->inp_done;
}

/* ------------------------------------------------------------------ model upscaling (ESRGAN, host/upscaler.c) */
/* the context's upscaler for the upscale_model option as it stands: built on first use, resident until the option changes */
static int upscaler_get(MLIS_Ctx* S)
{
	if (str_empty(S->path_upscale)) return api_error(S, MLIS_E_OPT_VALUE, "no upscale_model is set");
	if (S->upscaler) return 1;
	int r = backend_setup(S); if (r < 0) return r;
	S->upscaler = mlis_amd_upscaler_create(S->path_upscale);
	if (!S->upscaler) return api_error_lib(S, MLIS_E_UNKNOWN);
	S->n_upscaler_builds++;
	return 1;
}

/* src may be dst (the result is computed into a buffer of its own first) */
static int tensor_upscale(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst)
{
	if (str_empty(S->path_upscale)) return api_error(S, MLIS_E_OPT_VALUE, "no upscale_model is set");
	if (!src || !dst || !tensor_good(src) || src->n[0] < 1 || src->n[1] < 1 || src->n[2] != 3 || src->n[3] < 1)
		return api_error(S, MLIS_E_OPT_VALUE, "invalid tensor to upscale: an image of 3 channels is needed");
	const int w = src->n[0], h = src->n[1], b = src->n[3];
	if ((double)w * h * b * 16 * 3 >= 2147483648.0) return api_error(S, MLIS_E_OPT_VALUE, "image too large to upscale: %dx%d x %d", w, h, b);
	int r = upscaler_get(S); if (r < 0) return r;
	float *out = (float*)malloc(sizeof(float) * (size_t)16 * w * h * 3 * b);
	if (!out) return api_error(S, MLIS_E_UNKNOWN, "out of memory");
	if (mlis_amd_upscaler_run(S->upscaler, src->d, w, h, b, out) < 0) { free(out); return api_error_lib(S, MLIS_E_UNKNOWN); }
	mlis_tensor_resize(dst, 4 * w, 4 * h, 3, b);
	memcpy(dst->d, out, sizeof(float) * (size_t)16 * w * h * 3 * b);
	free(out);
	return 1;
}

MLB_API int mlis_amd_tensor_upscale(MLIS_Ctx* S, const MLIS_Tensor* src, MLIS_Tensor* dst)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	return tensor_upscale(S, src, dst);
}

MLB_API int mlis_amd_upscaler_builds(MLIS_Ctx* S, int* resident)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	if (resident) *resident = S->upscaler != NULL;
	return S->n_upscaler_builds;
}

/* ------------------------------------------------------------------ generation */
static int denoise_cb(void* user, int step, int n_step, int nfe)
{
	MLIS_Ctx *S = (MLIS_Ctx*)user;
	S->prg.nfe = S->nfe_base + nfe;
	return progress(S, MLIS_STAGE_DENOISE, step, n_step);
}

static int hires_on(const MLIS_Ctx* S) { return S->hires_scale > 1; }

/* a model file's name as the infotext gives it: the basename without its extension, *len characters from the result */
static const char* path_stem(const char* path, int* len)
{
	const char *b = path ? path : "", *sl = strrchr(b, '/'); if (sl) b = sl + 1;
	const char *e = strrchr(b, '.'); if (!e) e = b + strlen(b);
	*len = (int)(e - b);
	return b;
}

static void infotext_update(MLIS_Ctx* S, int w, int h, int hires_n_step)
{	/* mlis_infotext_update :1589-1632 (imitates stable-diffusion-webui create_infotext) */
	char buf[4096]; int n = 0;
#define ADD(...) n += snprintf(buf + n, sizeof(buf) - n > 0 ? sizeof(buf) - n : 0, __VA_ARGS__)
	int n_step, method, sched; sampler_defaults(S, &n_step, &method, &sched);
	ADD("%s\n", S->prompt_raw ? S->prompt_raw : "");
	if (!str_empty(S->nprompt_raw)) ADD("Negative prompt: %s\n", S->nprompt_raw);
	ADD("Seed: %" PRIu64, S->seed);
	ADD(", Sampler: %s", mlis_method_str((MLIS_Method)method));
	if (S->s_ancestral == 1) ADD(" ancestral");
	ADD(", Schedule type: %s", mlis_sched_str((MLIS_Scheduler)sched));
	if (S->s_ancestral > 0) ADD(", Ancestral: %g", S->s_ancestral);
	if (S->s_noise > 0) ADD(", SNoise: %g", S->s_noise);
	if (S->cfg_scale > 1) ADD(", CFG scale: %g", S->cfg_scale);
	if (S->f_t_ini < 1) ADD(", Mode: %s, f_t_ini: %g", tensor_good(&S->lmask) ? "inpaint" : "img2img", S->f_t_ini);
	ADD(", Steps: %u", (unsigned)S->last_n_step);
	ADD(", NFE: %u", (unsigned)S->last_nfe);
	ADD(", Size: %ux%u", (unsigned)w, (unsigned)h);
	ADD(", Clip skip: %d", S->clip_skip);
	int nb; const char *b = path_stem(S->path_model, &nb);
	ADD(", Model: %.*s", nb, b);
	if (S->flags & CF_USE_TAE) ADD(", VAE: tae");
	if (S->tiling) ADD(", Tiling: %s", k_tiling[S->tiling]);
	b = path_stem(S->path_upscale, &nb);
	if (hires_on(S) && S->hires_use_model)
		ADD(", Hires upscale: %g, Hires steps: %d, Hires upscaler: %.*s, Denoising strength: %g", S->hires_scale, hires_n_step, nb, b, S->hires_denoise);
	else if (hires_on(S)) ADD(", Hires upscale: %g, Hires steps: %d, Hires upscaler: %s, Denoising strength: %g", S->hires_scale, hires_n_step,
		k_resample[S->hires_upscaler], S->hires_denoise);
	if (S->tiled_tile) ADD(", Tiled diffusion: %d, Tile overlap: %d", S->tiled_tile, S->tiled_overlap);
	if (S->tiled_tile && S->tiled_pack > 1) ADD(", Tile batch: %d", S->tiled_pack);
	b = path_stem(S->path_control, &nb);
	if (!str_empty(S->path_control)) ADD(", ControlNet: %.*s, Control strength: %g, Control window: %g-%g", nb, b, S->control_strength, S->control_start, S->control_end);
	if (S->freeu) ADD(", FreeU: %g %g %g %g", S->freeu_f[0], S->freeu_f[1], S->freeu_f[2], S->freeu_f[3]);
	if (S->hypertile) ADD(", HyperTile: %d, HyperTile depth: %d", S->hypertile, S->hypertile_depth);
	if (S->pag_scale > 0) ADD(", PAG: %g", S->pag_scale);
	if (S->cfg_rescale > 0) ADD(", CFG rescale: %g", S->cfg_rescale);
	{	/* the prediction type and the schedule, where they are not the model type's own */
		int vp = 0, zs = 0, vp0 = 0;
		if (guidance_resolve(S, &vp, &zs) > 0 && mlis_amd_prediction_resolve(S->mname, 0, 0, 0, 0, &vp0, NULL) > 0) {
			if (vp != vp0) ADD(", Prediction: %s", vp ? "v-prediction" : "eps");
			if (zs) ADD(", Schedule: zsnr");
		}
	}
	if (S->downscale_filter) ADD(", Downscale filter: %s", k_downscale[S->downscale_filter]);
	if (!str_empty(S->path_control) && S->control_preprocess == MLIS_AMD_PREPROCESS_CANNY) ADD(", Control preprocess: canny %g %g%s", S->canny_low, S->canny_high, S->canny_l2 ? " L2" : "");
	else if (!str_empty(S->path_control) && S->control_preprocess) ADD(", Control preprocess: %s", k_preprocess[S->control_preprocess]);
	if (tensor_good(&S->lmask) && !hires_on(S)) {      /* region inpainting: the items that are set */
		if (S->inpaint_area == MLIS_AMD_INPAINT_MASKED) ADD(", Inpaint area: masked, Padding: %d", S->inpaint_padding);
		else if (S->inpaint_composite) ADD(", Inpaint area: whole, Composite: 1");
		if (S->mask_blur > 0) ADD(", Mask blur: %g", S->mask_blur);
		if (S->mask_grow) ADD(", Mask grow: %d", S->mask_grow);
		if (S->mask_invert) ADD(", Mask invert: 1");
	}
	ADD(", Version: MLImgSynth v%s", MLIS_VERSION_STR);
#undef ADD
	free(S->infotext); S->infotext = strdup(buf);
}

/* one generation from the options as they stand (the whole of mlis_generate but its first checks and its clean-up): conditioning, engine,
 * sampling, the latent fetched, the decode when `decode`; *pw_img x *ph_img = the size generated */
static int generate_pass(MLIS_Ctx* S, int decode, int* pw_img, int* ph_img)
{
	int r;
	const int B = S->n_batch > 0 ? S->n_batch : 1;
	int w = S->width / 8, h = S->height / 8;

	/* img2img source (:1652-1657) */
	if (S->tuflags & MLIS_TUF_IMAGE) {
		if ((r = mlis_image_encode(S, &S->image, &S->latent, 0)) < 0) return r;
		S->tuflags |= MLIS_TUF_LATENT;
	}
	if (S->tuflags & MLIS_TUF_LATENT) { w = S->latent.n[0]; h = S->latent.n[1]; }
	if (w < 1 || h < 1) return api_error(S, MLIS_E_OPT_VALUE, "image size not set");
	const int w_img = w * 8, h_img = h * 8;
	*pw_img = w_img; *ph_img = h_img;

	/* conditioning (:1688-1707), before the engine: its length (77 W rows) is part of the UNet plan */
	if (!(S->tuflags & MLIS_TUF_CONDITIONING)) {
		if ((r = text_cond_encode(S, S->cfg_scale > 1, w_img, h_img)) < 0) return r;
		if (S->cfg_scale > 1) {
			UnetParams U; unet_params_get(S->mname, &U);
			const int neg_empty = S->have_ptok[1] ? S->n_ptok[1] == 0 : str_empty(S->nprompt_raw);
			if (U.uncond_empty_zero && neg_empty) memset(S->ncond.d, 0, mlis_tensor_count(&S->ncond) * 4);   /* :1702-1703 */
		}
		if ((r = progress(S, MLIS_STAGE_COND_ENCODE, 1, 1)) < 0) return r;
	}
	if (!tensor_good(&S->cond) || (S->cfg_scale > 1 && !tensor_good(&S->ncond))) return api_error(S, MLIS_E_UNKNOWN, "conditioning tensors are not set");
	{
		const int T = S->cond.n[1];
		if (T < 77 || T % 77 || T > 77 * MLIS_AMD_MAX_WINDOWS)
			return api_error(S, MLIS_E_UNKNOWN, "conditioning of %d tokens (77 x W, W <= %d)", T, MLIS_AMD_MAX_WINDOWS);
		if (S->cfg_scale > 1 && S->ncond.n[1] != T)
			return api_error(S, MLIS_E_UNKNOWN, "conditioning lengths differ: cond %d, ncond %d tokens", T, S->ncond.n[1]);
		S->ctx_tok = T;
	}
	if ((r = engine_get(S, w, h)) < 0) return r;
	{	/* tiled diffusion: did this pass run in windows (infotext) */
		int n_win = 0;
		mlis_amd_tile_info(S->eng, &n_win, NULL, NULL);
		if (n_win) { S->tiled_tile = S->unet_tile; S->tiled_overlap = unet_tile_overlap_eff(S); mlis_amd_tile_pack_info(S->eng, &S->tiled_pack, NULL); }
	}
	if (S->tuflags & MLIS_TUF_LATENT) {
		if (S->latent.n[2] != 4) return api_error(S, MLIS_E_UNKNOWN, "latent must have 4 channels");
		const size_t per = (size_t)4*w*h;
		float *l = (float*)malloc(per * B * 4);
		for (int b=0;b<B;++b) memcpy(l + per*b, S->latent.d + (S->latent.n[3] == B ? per*b : 0), per*4);
		r = mlis_amd_set_init_latent(S->eng, l);
		free(l);
		if (r < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	} else mlis_amd_set_init_latent(S->eng, NULL);

	/* mask -> latent mask (:1673-1686) */
	if (S->tuflags & MLIS_TUF_MASK) { mlis_mask_encode(S, &S->mask, &S->lmask, 0); S->tuflags |= MLIS_TUF_LMASK; }
	if ((S->tuflags & MLIS_TUF_LMASK) && tensor_good(&S->lmask)) {
		if (S->lmask.n[0] != w || S->lmask.n[1] != h) return api_error(S, MLIS_E_IMAGE, "latent mask %dx%d does not match the latent %dx%d", S->lmask.n[0], S->lmask.n[1], w, h);
		if (mlis_amd_set_lmask(S->eng, S->lmask.d) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	} else { mlis_amd_set_lmask(S->eng, NULL); if (!(S->tuflags & MLIS_TUF_LMASK)) mlis_tensor_free(&S->lmask); }

	if ((r = control_apply(S, w_img, h_img, S->control_rect_on ? S->control_rect : NULL, S->control_rect_W, S->control_rect_H)) < 0) return r;
	if (S->freeu && mlis_amd_set_freeu(S->eng, S->freeu_f[0], S->freeu_f[1], S->freeu_f[2], S->freeu_f[3]) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	if (S->pag_scale > 0 && mlis_amd_set_pag(S->eng, S->pag_scale) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	{	/* prediction type, sigma table and guidance rescale: fields of the engine, set for every pass (a resident engine may have served other settings) */
		int vp = 0, zs = 0;
		if (guidance_resolve(S, &vp, &zs) < 0 || mlis_amd_set_prediction(S->eng, vp, zs) < 0 || mlis_amd_set_cfg_rescale(S->eng, S->cfg_rescale) < 0)
			return api_error_lib(S, MLIS_E_UNKNOWN);
	}
	if (mlis_amd_set_cond(S->eng, S->cond.d, tensor_good(&S->label) ? S->label.d : NULL, S->cfg_scale > 1 ? S->ncond.d : NULL,
			(S->cfg_scale > 1 && tensor_good(&S->nlabel)) ? S->nlabel.d : NULL) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
	S->image.flags &= ~LT_F_READY;

	/* sampling (:1720-1748): image i of the batch has its own Philox stream seed + i, continuing at the context's offset */
	uint64_t seeds[MAX_IMAGES]; for (int b=0;b<B;++b) seeds[b] = S->seed + b;
	mlis_amd_seed_ex(S->eng, seeds, S->rng_offset);
	mlis_amd_set_callback(S->eng, S->callback ? denoise_cb : NULL, S);
	r = mlis_amd_denoise(S->eng, NULL);
	S->rng_offset = mlis_amd_rng_offset(S->eng);
	if (S->control_pass < 2) mlis_amd_control_info(S->eng, NULL, &S->control_evals[S->control_pass++]);
	S->last_n_step = mlis_amd_last_n_step(S->eng); S->last_nfe = S->nfe_base + mlis_amd_last_nfe(S->eng); S->prg.nfe = S->last_nfe;
	if (r < 0) {
		if (r < -1 && r != MLIS_E_NAN) return r;                                  /* the callback's abort code */
		return api_error_lib(S, r == MLIS_E_NAN || strstr(mlsd_last_error(), "NaN") ? MLIS_E_NAN : MLIS_E_UNKNOWN);
	}
	mlis_tensor_resize(&S->latent, w, h, 4, B);
	if (mlsd_memcpy(S->latent.d, mlis_amd_latent_device(S->eng), (size_t)B*4*w*h*4, 1, NULL) || mlsd_device_sync()) return api_error_lib(S, MLIS_E_UNKNOWN);

	/* decode (:1752-1756) */
	if (decode) {
		if (mlis_amd_decode(S->eng) < 0) return api_error_lib(S, MLIS_E_UNKNOWN);
		if ((r = image_fetch(S, &S->image, w_img, h_img)) < 0) return r;
		if ((r = progress(S, MLIS_STAGE_IMAGE_DECODE, 1, 1)) < 0) return r;
	}
	return 1;
}

/* hires fix: the txt2img pass at IMAGE_DIM (never decoded), its latent upscaled, then the img2img-from-latent pass at the target size with
 * f_t_ini = hires_denoise -- what a caller gets from generate (NO_DECODE) + mlis_amd_tensor_resample + generate (MLIS_TUF_LATENT), with the
 * prompt, the token ids and the prompt's LoRAs in place until the end and the Philox streams running on from the first pass.  With hires_use_model the first pass
 * IS decoded, its image goes 4x through the upscale model and a plain resample to the target size, and the second pass is img2img from that image */
static int generate_hires(MLIS_Ctx* S, int decode, int* pw_img, int* ph_img, int* hires_n_step)
{
	static const struct { int flag; const char* what; } inputs[] = { {MLIS_TUF_IMAGE, "an input image (image)"}, {MLIS_TUF_LATENT, "an input latent (tensor_use_flags latent)"},
		{MLIS_TUF_MASK, "a mask (image_mask)"}, {MLIS_TUF_LMASK, "a latent mask (tensor_use_flags lmask)"} };
	for (int i=0;i<COUNTOF(inputs);++i) if (S->tuflags & inputs[i].flag)
		return api_error(S, MLIS_E_OPT_VALUE, "hires_scale %g cannot be combined with %s: the hires fix is a txt2img feature", S->hires_scale, inputs[i].what);
	const float f_t_ini = S->f_t_ini; const int n_step = S->n_step, tuflags = S->tuflags;
	const int use_model = S->hires_use_model;
	int r = generate_pass(S, use_model, pw_img, ph_img);
	if (r >= 0) {
		const int steps1 = S->last_n_step, lw = S->latent.n[0], lh = S->latent.n[1];
		const int tw = (int)floor((double)lw * S->hires_scale + 0.5), th = (int)floor((double)lh * S->hires_scale + 0.5);      /* the target latent size, either way */
		if (use_model) {
			/* the decoded first pass upscaled 4x by the model, brought to the target pixel size by a plain resample -- or, with a downscale_filter and an axis that
			 * shrinks, by that filter --; the second pass encodes it (generate_pass, MLIS_TUF_IMAGE): what a caller gets from generate + mlis_amd_tensor_upscale +
			 * mlis_amd_tensor_resample (or _resample_aa) + generate with an input image */
			r = tensor_upscale(S, &S->image, &S->image);
			if (r >= 0 && S->downscale_filter && (tw * 8 < S->image.n[0] || th * 8 < S->image.n[1])) r = tensor_resample_aa(S, &S->image, &S->image, tw * 8, th * 8, S->downscale_filter - 1);
			else if (r >= 0) r = tensor_resample(S, &S->image, &S->image, tw * 8, th * 8, S->hires_upscaler);
		} else r = tensor_resample(S, &S->latent, &S->latent, tw, th, S->hires_upscaler);
		if (r >= 0) {
			S->tuflags = (tuflags & MLIS_TUF_CONDITIONING) | (use_model ? MLIS_TUF_IMAGE : MLIS_TUF_LATENT);
			S->f_t_ini = S->hires_denoise;
			if (S->hires_steps > 0) S->n_step = S->hires_steps;
			int method, sched; sampler_defaults(S, hires_n_step, &method, &sched);   /* "Hires steps": the count asked for (as "Steps" does, webui's convention); with f_t_ini < 1 the pass runs fewer */
			S->nfe_base = S->last_nfe;
			r = generate_pass(S, decode, pw_img, ph_img);
			S->nfe_base = 0;
			S->last_n_step = steps1;        /* "Steps" of the infotext: the first pass, the second one is "Hires steps" */
		}
	}
	S->f_t_ini = f_t_ini; S->n_step = n_step; S->tuflags = tuflags;
	return r;
}

/* region inpainting: any of the six options off its default */
static int inpaint_on(const MLIS_Ctx* S)
{
	return S->inpaint_area != MLIS_AMD_INPAINT_WHOLE || S->inpaint_composite || S->mask_grow || S->mask_blur > 0 || S->mask_invert;
}
static int inpaint_composites(const MLIS_Ctx* S) { return S->inpaint_area == MLIS_AMD_INPAINT_MASKED || S->inpaint_composite; }

/* what generate_inpaint refuses; before mlis_setup, so that none of them needs a model */
static int inpaint_check(MLIS_Ctx* S)
{
	const int masked = S->inpaint_area == MLIS_AMD_INPAINT_MASKED;
	if (masked && S->tiling) return api_error(S, MLIS_E_OPT_VALUE, "inpaint_area masked cannot be combined with tiling '%s': a crop is not periodic", k_tiling[S->tiling]);
	if (inpaint_composites(S)) {
		const char *what = masked ? "inpaint_area masked" : "inpaint_composite";
		if (!(S->tuflags & MLIS_TUF_IMAGE) || !(S->tuflags & MLIS_TUF_MASK) || !tensor_good(&S->image) || !tensor_good(&S->mask))
			return api_error(S, MLIS_E_OPT_VALUE, "%s needs an input image (image) and a mask (image_mask)", what);
		if (S->flags & CF_NO_DECODE) return api_error(S, MLIS_E_OPT_VALUE, "%s cannot be combined with no_decode: the composite is made of decoded images", what);
	}
	if ((S->tuflags & MLIS_TUF_MASK) && (S->tuflags & MLIS_TUF_IMAGE) && tensor_good(&S->mask) && tensor_good(&S->image)
			&& (S->mask.n[0] != S->image.n[0] || S->mask.n[1] != S->image.n[1]))
		return api_error(S, MLIS_E_IMAGE, "the mask %dx%d does not match the image %dx%d", S->mask.n[0], S->mask.n[1], S->image.n[0], S->image.n[1]);
	return 1;
}

/* the resample of a masked pass, to the processing size and back: antialiased with the downscale_filter where that is set and an axis shrinks, else plain in `mode`
 * -- the choice of the hires model path */
static int inpaint_resample(MLIS_Ctx* S, MLIS_Tensor* t, int w, int h, int mode)
{
	if (S->downscale_filter && (w < t->n[0] || h < t->n[1])) return tensor_resample_aa(S, t, t, w, h, S->downscale_filter - 1);
	return tensor_resample(S, t, t, w, h, mode);
}

/* region inpainting around generate_pass -- what a caller gets from the public calls in this order: mlis_amd_tensor_mask_weight, _mask_grow, _gauss_blur (p),
 * _mask_bbox, mlis_amd_inpaint_region, a crop of the image and of 1 - p, mlis_amd_tensor_resample (or _resample_aa) of both to IMAGE_DIM, mlis_generate with image and
 * mask, a resample back, mlis_amd_tensor_composite into the untouched image.  With inpaint_area whole the pass runs on the whole image with 1 - p as its mask and,
 * with inpaint_composite, its decoded images are composited over the input through p.  Without a mask there is nothing to process: the plain pass. */
static int generate_inpaint(MLIS_Ctx* S, int decode, int* pw_img, int* ph_img)
{
	if (!(S->tuflags & MLIS_TUF_MASK) || !tensor_good(&S->mask)) return generate_pass(S, decode, pw_img, ph_img);
	const int masked = S->inpaint_area == MLIS_AMD_INPAINT_MASKED, composite = inpaint_composites(S);
	const int W = S->mask.n[0], H = S->mask.n[1];
	if (S->mask.n[2] != 1 || S->mask.n[3] != 1) return api_error(S, MLIS_E_IMAGE, "the mask must be one plane");
	MLIS_Tensor p = {0}, orig = {0};
	int r, box[4] = {0}, reg[4] = { 0, 0, W, H };
	if ((r = tensor_mask_op(S, MASK_OP_WEIGHT, &S->mask, &p, S->mask_invert, 0, 0)) < 0) goto done;
	if (S->mask_grow && (r = tensor_mask_op(S, MASK_OP_GROW, &p, &p, S->mask_grow, 0, S->tiling)) < 0) goto done;
	if (S->mask_blur > 0 && (r = tensor_mask_op(S, MASK_OP_BLUR, &p, &p, 0, S->mask_blur, S->tiling)) < 0) goto done;
	if ((r = tensor_mask_bbox(S, &p, box)) < 0) goto done;
	if (box[2] <= box[0]) { r = api_error(S, MLIS_E_OPT_VALUE, "the mask leaves nothing to repaint (mask_invert %d, mask_grow %d)", S->mask_invert, S->mask_grow); goto done; }
	for (size_t i=0, n=(size_t)W*H; i<n; ++i) S->mask.d[i] = 1.0f - p.d[i];      /* the pass's mask: 1 = keep */
	if (composite) mlis_tensor_copy(&orig, &S->image);
	if (masked) {
		const int tw = S->width, th = S->height;
		if (tw < 8 || th < 8 || tw % 8 || th % 8) { r = api_error(S, MLIS_E_OPT_VALUE, "inpaint_area masked: invalid processing size %dx%d (image_dim)", tw, th); goto done; }
		if (mlis_amd_inpaint_region(W, H, box, S->inpaint_padding, tw, th, reg) < 0) { r = api_error(S, MLIS_E_UNKNOWN, "internal: inpaint region"); goto done; }
		const int cw = reg[2] - reg[0], ch = reg[3] - reg[1];
		const int mask_mode = S->hires_upscaler == MLIS_AMD_RESAMPLE_BICUBIC ? MLIS_AMD_RESAMPLE_BILINEAR : S->hires_upscaler;      /* the mask stays in 0 .. 1 */
		if ((r = tensor_crop(S, &S->image, &S->image, reg[0], reg[1], cw, ch)) < 0 || (r = tensor_crop(S, &S->mask, &S->mask, reg[0], reg[1], cw, ch)) < 0
				|| (r = inpaint_resample(S, &S->image, tw, th, S->hires_upscaler)) < 0 || (r = inpaint_resample(S, &S->mask, tw, th, mask_mode)) < 0) goto done;
		S->control_rect_on = 1; memcpy(S->control_rect, reg, sizeof(reg)); S->control_rect_W = W; S->control_rect_H = H;
		r = generate_pass(S, 1, pw_img, ph_img);
		S->control_rect_on = 0;
		if (r < 0) goto done;
		if ((r = inpaint_resample(S, &S->image, cw, ch, S->hires_upscaler)) < 0) goto done;
	} else if ((r = generate_pass(S, decode, pw_img, ph_img)) < 0) goto done;
	if (composite) {
		S->inp_proc[0] = *pw_img; S->inp_proc[1] = *ph_img;
		if ((r = tensor_composite(S, &S->image, &orig, &S->image, &p, reg[0], reg[1])) < 0) goto done;
		S->image.flags |= LT_F_READY;
		memcpy(S->inp_region, reg, sizeof(reg)); S->inp_done = 1;
		*pw_img = W; *ph_img = H;
	}
done:
	mlis_tensor_free(&p); mlis_tensor_free(&orig);
	return r;
}

MLB_API int mlis_generate(MLIS_Ctx* S)
{
	if (!S || S->signature != CTX_SIGNATURE) return -1;
	S->inp_done = 0;
	if (inpaint_on(S)) { int c = inpaint_check(S); if (c < 0) return c; }
	if (hires_on(S) && S->hires_use_model && str_empty(S->path_upscale))
		return api_error(S, MLIS_E_OPT_VALUE, "hires_use_model is set but no upscale_model");
	int r = mlis_setup(S); if (r < 0) return r;
	const int B = S->n_batch > 0 ? S->n_batch : 1;
	if (B > MAX_IMAGES) return api_error(S, MLIS_E_OPT_VALUE, "batch size > %d not supported", MAX_IMAGES);
	if ((r = tiling_check(S)) < 0) return r;
	if ((r = unet_tile_check(S)) < 0) return r;
	{	/* ControlNet: model and image come together, the window is an interval */
		const int has_model = !str_empty(S->path_control), has_image = tensor_good(&S->control_image);
		if (has_model && !has_image) return api_error(S, MLIS_E_OPT_VALUE, "control_model '%s' without a control_image", S->path_control);
		if (has_image && !has_model) return api_error(S, MLIS_E_OPT_VALUE, "control_image without a control_model");
		if (S->control_start > S->control_end) return api_error(S, MLIS_E_OPT_VALUE, "invalid control window: control_start %g > control_end %g", S->control_start, S->control_end);
	}
	S->control_evals[0] = S->control_evals[1] = S->control_pass = 0;
	S->tiled_tile = S->tiled_overlap = S->tiled_pack = 0;
	S->t_last = now_s(); memset(&S->prg, 0, sizeof(S->prg));
	int w_img = 0, h_img = 0, hires_n_step = 0;
	const int decode = !(S->flags & CF_NO_DECODE);
	r = hires_on(S) ? generate_hires(S, decode, &w_img, &h_img, &hires_n_step)      /* (it refuses image and mask inputs) */
		: inpaint_on(S) ? generate_inpaint(S, decode, &w_img, &h_img) : generate_pass(S, decode, &w_img, &h_img);
	if (r < 0) return r;
	infotext_update(S, w_img, h_img, hires_n_step);
	/* mlis_prompt_clear :692-709 */
	str_set(&S->prompt_raw, ""); str_set(&S->nprompt_raw, "");
	mlis_prompt_free(&S->prompt); mlis_prompt_free(&S->nprompt);
	S->have_ptok[0] = S->have_ptok[1] = 0;
	S->f_t_ini = 1; S->f_t_end = 0; S->tuflags = 0;
	loras_remove(S, 1);                                  /* mlis_cfg_loras_prompt_remove */
	return 1;
}

MLB_API MLIS_Image* mlis_image_get(MLIS_Ctx* S, int idx)
{	/* :1775-1793 + mlis_tensor_to_image :118-139: u8 = clamp(v*255, 0, 255) truncated */
	if (!S || S->signature != CTX_SIGNATURE) return NULL;
	if (!(S->image.flags & LT_F_READY)) { api_error(S, MLIS_E_UNKNOWN, "image not ready"); return NULL; }
	if (idx < 0 || idx >= S->image.n[3] || idx >= MAX_IMAGES) { api_error(S, MLIS_E_UNKNOWN, "only image idx < %d available", S->image.n[3]); return NULL; }
	const int n0 = S->image.n[0], n1 = S->image.n[1], n2 = S->image.n[2];
	MLIS_Image *I = &S->imgex[idx];
	I->w = n0; I->h = n1; I->c = n2; I->sz = (size_t)n0*n1*n2;
	I->d = (uint8_t*)realloc((I->flags & LT_F_OWNMEM) ? I->d : NULL, I->sz ? I->sz : 1);
	I->flags |= LT_F_OWNMEM;
	const float *td = S->image.d + (size_t)n0*n1*n2*idx;
	for (int y=0;y<n1;++y) for (int x=0;x<n0;++x) for (int c=0;c<n2;++c) {
		float v = td[(size_t)n0*n1*c + (size_t)n0*y + x] * 255;
		v = v < 0 ? 0 : (v > 255 ? 255 : v);
		I->d[(size_t)n0*n2*y + (size_t)n2*x + c] = (uint8_t)v;
	}
	return I;
}

MLB_API const char* mlis_infotext_get(MLIS_Ctx* S, int idx)
{
	if (!S || S->signature != CTX_SIGNATURE || idx < 0) return NULL;
	return S->infotext;
}

MLB_API MLIS_Tensor* mlis_tensor_get(MLIS_Ctx* S, MLIS_TensorId id)
{	/* :1795-1820 */
	if (!S || S->signature != CTX_SIGNATURE) return NULL;
	switch ((int)id) {
	case MLIS_TENSOR_IMAGE: return &S->image;   case MLIS_TENSOR_MASK: return &S->mask;
	case MLIS_TENSOR_LATENT: return &S->latent; case MLIS_TENSOR_LMASK: return &S->lmask;
	case MLIS_TENSOR_COND: return &S->cond;     case MLIS_TENSOR_LABEL: return &S->label;
	case MLIS_TENSOR_NCOND: return &S->ncond;   case MLIS_TENSOR_NLABEL: return &S->nlabel;
	}
	if ((int)id >= MLIS_TENSOR_TMP && (int)id < MLIS_TENSOR_TMP + N_TMP_TENSORS) return &S->tmp[(int)id - MLIS_TENSOR_TMP];
	api_error(S, MLIS_E_UNKNOWN, "invalid tensor id %d", (int)id);
	return NULL;
}
