/* mlis_abi.h — the public libmlimgsynth C-ABI, as exported by libmlimgsynth_amd.so.
 *
 * Binary-compatible re-declaration of the reference's include/mlimgsynth.h:57-575 (v0.4.x): the enum values, struct layouts
 * and symbol names below ARE the interface its FFI binds (python/mlimgsynth.py:165-208 loads a shared library and calls
 * exactly these), so a program or binding written against the reference header runs on this library unchanged
 * (MLIS_LIB_PATH=.../libmlimgsynth_amd.so).  Each group cites the reference lines it mirrors.  Behavioural differences are
 * listed in INTEGRATION.md section 4 (batches > 1 are supported; the CLIP vocabulary is run-time data found through AUX_DIR;
 * MODEL accepts "synth:<model>" for the synthetic-weight benchmark models).
 */
#ifndef MLIS_ABI_H
#define MLIS_ABI_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MLIS_VERSION 0x000402                     /* mlimgsynth.h:60; accepted by mlis_ctx_create_i: 0x000400 <= v < 0x000500 */
#define MLIS_VERSION_STR "0.4.2"

/* mlimgsynth.h:68-77 */
typedef enum { MLIS_E_UNKNOWN = -1, MLIS_E_VERSION = -2, MLIS_E_UNK_OPT = -3, MLIS_E_OPT_VALUE = -4, MLIS_E_PROMPT_PARSE = -5,
               MLIS_E_FILE_NOT_FOUND = -6, MLIS_E_NAN = -7, MLIS_E_IMAGE = -8 } MLIS_ErrorCode;
/* :81-87 */
typedef enum { MLIS_STAGE_IDLE = 0, MLIS_STAGE_COND_ENCODE = 1, MLIS_STAGE_IMAGE_ENCODE = 2, MLIS_STAGE_IMAGE_DECODE = 3,
               MLIS_STAGE_DENOISE = 4 } MLIS_Stage;
/* :91-99, :103-108 */
typedef enum { MLIS_METHOD_NONE = 0, MLIS_METHOD_EULER = 1, MLIS_METHOD_HEUN = 2, MLIS_METHOD_TAYLOR3 = 3, MLIS_METHOD_DPMPP2M = 4,
               MLIS_METHOD_DPMPP2S = 5, MLIS_METHOD__LAST = 5 } MLIS_Method;
typedef enum { MLIS_SCHED_NONE = 0, MLIS_SCHED_UNIFORM = 1, MLIS_SCHED_KARRAS = 2, MLIS_SCHED__LAST = 2 } MLIS_Scheduler;
/* :112-122 */
typedef enum { MLIS_LOGLVL_NONE = 0, MLIS_LOGLVL_ERROR = 10, MLIS_LOGLVL_WARNING = 20, MLIS_LOGLVL_INFO = 30, MLIS_LOGLVL_VERBOSE = 40,
               MLIS_LOGLVL_DEBUG = 50, MLIS_LOGLVL_MAX = 255, MLIS_LOGLVL__INCREASE = 0x100 | 10, MLIS_LOGLVL__DECREASE = 0x200 | 10 } MLIS_LogLvl;
/* :126-138, :142-148 */
typedef enum { MLIS_TENSOR_IMAGE = 1, MLIS_TENSOR_MASK = 2, MLIS_TENSOR_LATENT = 3, MLIS_TENSOR_LMASK = 4, MLIS_TENSOR_COND = 5,
               MLIS_TENSOR_LABEL = 6, MLIS_TENSOR_NCOND = 7, MLIS_TENSOR_NLABEL = 8, MLIS_TENSOR_TMP = 0x100 } MLIS_TensorId;
typedef enum { MLIS_TUF_IMAGE = 1, MLIS_TUF_MASK = 2, MLIS_TUF_LATENT = 4, MLIS_TUF_LMASK = 8, MLIS_TUF_CONDITIONING = 16 } MLIS_TensorUseFlag;
/* :152-158 (+ this library's test models, outside the reference's range) */
typedef enum { MLIS_MODEL_TYPE_NONE = 0, MLIS_MODEL_TYPE_SD1 = 1, MLIS_MODEL_TYPE_SD2 = 2, MLIS_MODEL_TYPE_SDXL = 3, MLIS_MODEL_TYPE__LAST = 3,
               MLIS_MODEL_TYPE_AMD_TINY = 101, MLIS_MODEL_TYPE_AMD_TINYXL = 102, MLIS_MODEL_TYPE_AMD_TINYV = 103 } MLIS_ModelType;
/* :162-169 */
typedef enum { MLIS_SUBMODEL_NONE = 0, MLIS_SUBMODEL_UNET = 1, MLIS_SUBMODEL_VAE = 2, MLIS_SUBMODEL_TAE = 3, MLIS_SUBMODEL_CLIP = 4,
               MLIS_SUBMODEL_CLIP2 = 5 } MLIS_SubModel;
/* :174-346: option ids; argument types as in the reference's comments (str = const char*, float options take double) */
typedef enum {
	MLIS_OPT_NONE = 0, MLIS_OPT_BACKEND = 1, MLIS_OPT_MODEL = 2, MLIS_OPT_TAE = 3, MLIS_OPT_LORA_DIR = 4, MLIS_OPT_LORA = 5,
	MLIS_OPT_LORA_CLEAR = 6, MLIS_OPT_PROMPT = 7, MLIS_OPT_NPROMPT = 8, MLIS_OPT_IMAGE_DIM = 9, MLIS_OPT_BATCH_SIZE = 10,
	MLIS_OPT_CLIP_SKIP = 11, MLIS_OPT_CFG_SCALE = 12, MLIS_OPT_METHOD = 13, MLIS_OPT_SCHEDULER = 14, MLIS_OPT_STEPS = 15,
	MLIS_OPT_F_T_INI = 16, MLIS_OPT_F_T_END = 17, MLIS_OPT_S_NOISE = 18, MLIS_OPT_S_ANCESTRAL = 19, MLIS_OPT_IMAGE = 20,
	MLIS_OPT_IMAGE_MASK = 21, MLIS_OPT_NO_DECODE = 22, MLIS_OPT_TENSOR_USE_FLAGS = 23, MLIS_OPT_SEED = 24, MLIS_OPT_VAE_TILE = 25,
	MLIS_OPT_UNET_SPLIT = 26, MLIS_OPT_THREADS = 27, MLIS_OPT_DUMP_FLAGS = 28, MLIS_OPT_AUX_DIR = 29, MLIS_OPT_CALLBACK = 30,
	MLIS_OPT_ERROR_HANDLER = 31, MLIS_OPT_LOG_LEVEL = 32, MLIS_OPT_MODEL_TYPE = 33, MLIS_OPT_WEIGHT_TYPE = 34,
	MLIS_OPT_NO_PROMPT_PARSE = 35, MLIS_OPT__LAST = 35,
	/* extensions of this implementation (ids from 101, as MLIS_MODEL_TYPE_AMD_*; MLIS_OPT__LAST stays the reference's last option) */
	MLIS_OPT_AMD_TILING = 101,     /* "tiling": seamless tiling, none|x|y|xy or 0..3 (int); the UNet and codec convolutions pad circularly */
	/* hires fix (two-pass txt2img): generate at IMAGE_DIM, upscale the latent, denoise again at the larger size.  The four persist across generations. */
	MLIS_OPT_AMD_HIRES_SCALE = 102,    /* "hires_scale" (float): 0 or 1 = off, else 1 < s <= 4; target latent = floor(l s + 0.5) per side */
	MLIS_OPT_AMD_HIRES_DENOISE = 103,  /* "hires_denoise" (float, default 0.7): 0 < d <= 1, the second pass's f_t_ini */
	MLIS_OPT_AMD_HIRES_STEPS = 104,    /* "hires_steps" (int): step count the second pass is scheduled with, 0 = the STEPS value (it runs the last hires_denoise share of them) */
	MLIS_OPT_AMD_HIRES_UPSCALER = 105, /* "hires_upscaler": nearest|bilinear|bicubic or 0..2 (int; MLIS_AMD_RESAMPLE_*), default bilinear */
	/* tiled diffusion (MultiDiffusion): a pass whose size exceeds the tile on an axis evaluates the UNet in overlapping windows of the tile's size and blends their
	 * outputs; a pass that fits runs as ever (the first pass of a hires generation, typically).  Both persist across generations.  (A block of its own from 111.) */
	MLIS_OPT_AMD_UNET_TILE = 111,          /* "unet_tile" (int, pixels): 0 = off (default), else a multiple of 8 -- the size the model was trained at: 512 SD1, 1024 SDXL */
	MLIS_OPT_AMD_UNET_TILE_OVERLAP = 112,  /* "unet_tile_overlap" (int, pixels): minimum overlap of neighbouring windows, a multiple of 8 with 2 x overlap <= tile; 0 is allowed;
	                                        * -1 = auto (default): a quarter of the tile, rounded down to a multiple of 8 */
	/* packed windows: up to this many windows of a tiled pass run as one batched UNet evaluation (the effective count: mlis_amd_tile_pack).  Persists across
	 * generations; costs the activation memory of a plan for that many windows x the batch.  (A block of its own from 121.) */
	MLIS_OPT_AMD_UNET_TILE_BATCH = 121,    /* "unet_tile_batch" (int): 1 .. 16, default 1 = one window per evaluation */
	/* ControlNet: the UNet is conditioned on a control image (pose, depth, edges, tile: the finished map, or a picture for the control_preprocess of 171) through a copy of its encoder */
	MLIS_OPT_AMD_CONTROL_MODEL = 131,      /* "control_model" (string): a safetensors ControlNet in the original (cldm.py) layout for the base model, or "synth[:seed]" with a
	                                        * "synth:" model; "" = off.  Engines with and without it coexist in the two resident slots */
	MLIS_OPT_AMD_CONTROL_IMAGE = 132,      /* "control_image" (const MLIS_Image*, 3 channels; NULL clears; mlis_option_get gives an int: 1 if one is set): any size, resampled on the GPU to each pass's pixel size
	                                        * (bilinear; with the downscale_filter where that is set and an axis shrinks); it stays set across generations, like the model */
	MLIS_OPT_AMD_CONTROL_STRENGTH = 133,   /* "control_strength" (float, default 1): 0 .. 2, the gain on the ControlNet's residuals */
	MLIS_OPT_AMD_CONTROL_START = 134,      /* "control_start" (float, default 0) and */
	MLIS_OPT_AMD_CONTROL_END = 135,        /* "control_end" (float, default 1): the share of the steps that is controlled, 0 <= start <= end <= 1 (checked by mlis_generate) */
	/* FreeU (version 2 of the published code): at the decoder's concatenations the backbone's first half of channels is amplified by a structure map and the skip
	 * tensor's lowest spatial frequencies are damped; no weights, no training.  Stage 1 is the concatenations whose backbone has the UNet's top channel count (1280),
	 * stage 2 those with half of it.  The defaults of the four factors are the authors' recommendation for version 2 as recalled when this was written; it could
	 * not be checked against the publication then -- front ends list per-model values, set them explicitly where it matters.  A factor of 1 switches its part off. */
	MLIS_OPT_AMD_FREEU = 141,              /* "freeu" (int 0 / 1, default 0): part of the engine key, engines with and without coexist in the two resident slots */
	MLIS_OPT_AMD_FREEU_B1 = 142,           /* "freeu_b1" (float 0 .. 4, default 1.3): backbone factor of stage 1 */
	MLIS_OPT_AMD_FREEU_B2 = 143,           /* "freeu_b2" (float 0 .. 4, default 1.4): backbone factor of stage 2 */
	MLIS_OPT_AMD_FREEU_S1 = 144,           /* "freeu_s1" (float 0 .. 4, default 0.9): skip factor of stage 1 */
	MLIS_OPT_AMD_FREEU_S2 = 145,           /* "freeu_s2" (float 0 .. 4, default 0.2): skip factor of stage 2.  The four are device data of the engine: a change rebuilds nothing */
	/* ESRGAN upscaler (RRDBNet x4): a learned pixel-space upscaler for mlis_amd_tensor_upscale and, with hires_use_model, for the hires fix */
	MLIS_OPT_AMD_UPSCALE_MODEL = 151,      /* "upscale_model" (string): a safetensors RRDBNet in BasicSR's naming, or "synth[:seed[:blocks]]"; empty clears it and frees the
	                                        * resident upscaler.  The upscaler is built on first use and stays resident, keyed by this string */
	MLIS_OPT_AMD_HIRES_USE_MODEL = 152,    /* "hires_use_model" (int 0 / 1, default 0): the hires fix decodes its first pass, upscales the IMAGE 4x with upscale_model, resamples it
	                                        * to the target size (in the hires_upscaler mode, a plain resample; with the downscale_filter where that is set) and runs the second
	                                        * pass as img2img from it */
	/* antialiased downscaling: the filter of the resamples that shrink an image -- the hires fix's model path to its target size and the control image to a pass's size --,
	 * its support grows with the shrink factor (mlis_amd_tensor_resample_aa).  A resample where neither axis shrinks runs as with "none"; the latent upscale of the plain
	 * hires fix stays on hires_upscaler.  Persists across generations.  (A block of its own from 161.) */
	MLIS_OPT_AMD_DOWNSCALE_FILTER = 161,   /* "downscale_filter": none|box|bilinear|bicubic|lanczos or 0..4 (int; 0 = none, else MLIS_AMD_AA_* + 1), default none = the plain resamples */
	/* control image preprocessor: run on the GPU AFTER the control image was resampled to a pass's pixel size ("pixel perfect"), so the hires second pass and tiled
	 * canvases get one-pixel edges at their own resolution.  canny: mlis_amd_tensor_canny with the three options below and the context's "tiling" as wrap; invert:
	 * 1 - x (a black-on-white drawing for a scribble or line-art ControlNet).  A change of any of the four while a control image is set makes the engines take the
	 * image again at their next pass; nothing is rebuilt.  They persist across generations.  (A block of its own from 171.) */
	MLIS_OPT_AMD_CONTROL_PREPROCESS = 171, /* "control_preprocess": none|canny|invert or 0..2 (int; MLIS_AMD_PREPROCESS_*), default none = the control image is the finished map */
	MLIS_OPT_AMD_CANNY_LOW = 172,          /* "canny_low" (float 0 .. 32767, default 100) and */
	MLIS_OPT_AMD_CANNY_HIGH = 173,         /* "canny_high" (float 0 .. 32767, default 200): the hysteresis thresholds on the gradient magnitude of the 8-bit image; swapped if low > high */
	MLIS_OPT_AMD_CANNY_L2 = 174,           /* "canny_l2" (int 0 / 1, default 0): the magnitude is sqrt(dx^2 + dy^2) (compared squared) instead of |dx| + |dy| */
	/* region inpainting: what front ends call "inpaint area: only masked", "mask blur" and the paste-back.  When any of the six is off its default and the generation
	 * has a mask (image_mask, or the alpha of image), the mask goes through mlis_amd_tensor_mask_weight (mask_invert), _mask_grow (mask_grow) and _gauss_blur (mask_blur)
	 * to the repaint weight p, and the pass runs with 1 - p as its mask.  With all six at their defaults none of that runs and a generation gives the bytes it gave
	 * before these existed.  They persist across generations.  mlis_generate refuses: masked with a tiling other than none (a crop is not periodic), masked or
	 * inpaint_composite without an image and a mask, or with no_decode, and a mask that leaves nothing to repaint.  (A block of its own from 181.) */
	MLIS_OPT_AMD_INPAINT_AREA = 181,       /* "inpaint_area": whole|masked or 0..1 (int; MLIS_AMD_INPAINT_*), default whole.  masked: the region of mlis_amd_inpaint_region around the
	                                        * bounding box of p > 0 is cropped from the image (any size, not only multiples of 8) and from 1 - p, both are resampled to IMAGE_DIM (the
	                                        * image in the hires_upscaler mode, the mask in that mode but bilinear for bicubic so that it stays in 0 .. 1; where an axis shrinks and a
	                                        * downscale_filter is set, with that filter), inpainted there as img2img, the result is resampled back to the region's size by the same
	                                        * choice and composited into the untouched image through p.  A control image is taken to cover the whole picture and cropped likewise */
	MLIS_OPT_AMD_INPAINT_PADDING = 182,    /* "inpaint_padding" (int pixels, 0 .. 512, default 32): what the bounding box is padded by on each side */
	MLIS_OPT_AMD_MASK_BLUR = 183,          /* "mask_blur" (float sigma, 0 .. 64, default 0): the Gaussian blur of the repaint weight (mlis_amd_tensor_gauss_blur) */
	MLIS_OPT_AMD_MASK_GROW = 184,          /* "mask_grow" (int pixels, -256 .. 256, default 0): the repainted area grows by so many pixels, or shrinks if negative */
	MLIS_OPT_AMD_MASK_INVERT = 185,        /* "mask_invert" (int 0 / 1, default 0): the mask says 1 = repaint, the front ends' convention, not the reference's 1 = keep */
	MLIS_OPT_AMD_INPAINT_COMPOSITE = 186,  /* "inpaint_composite" (int 0 / 1, default 0): with inpaint_area whole, the decoded images are composited over the input image through
	                                        * p, so that pixels with p == 0 are the input's, exactly.  masked implies it */
	/* HyperTile: every UNet (and ControlNet) self-attention is computed inside tiles of its token map; convolutions and cross-attention keep the whole picture.  No
	 * weights, no training.  The tile of a level is chosen per axis by mlis_amd_hypertile_side (include/mlimgsynth_amd.h), per pass size: a pass whose levels all come
	 * out as one tile (the 512 px first pass of a hires run with hypertile 512) runs the plain plan.  The rule is the published one with its random choice among the
	 * divisors fixed to the first, as recalled when this was written; it could not be checked against the publication then.  Both are part of the engine key: engines
	 * with different settings coexist in the two resident slots.  They persist across generations.  (A block of its own from 191.) */
	MLIS_OPT_AMD_HYPERTILE = 191,          /* "hypertile" (int, pixels): 0 = off (default), else 32 .. 8192 and a multiple of 8: the tile's side in image pixels */
	MLIS_OPT_AMD_HYPERTILE_DEPTH = 192,    /* "hypertile_depth" (int 0 .. 3, default 3): the deepest UNet level (log2 of its downscale) that is tiled */
	/* Perturbed-attention guidance (PAG): beside the cond and uncond evaluations the UNet is evaluated once more per image with the self-attentions of its middle block
	 * replaced by the identity (softmax(q k^T) v -> v), and dx = cfg mix + pag_scale (cond - perturbed).  No weights, no training; it composes with CFG and also guides
	 * at cfg_scale <= 1, where CFG does nothing (few-step distilled checkpoints).  The rule (include/mlimgsynth_amd.h) is written as recalled from the publication and the
	 * front ends that ship it: parity with them is not pinned by a test.  pag_scale > 0 is part of the engine key as on / off: the engine's UNet plan carries a third row
	 * group (about 1.5 x the work of a CFG evaluation, 2 x at cfg_scale <= 1); the value is a kernel argument and changes without building anything.  With 0 none of it
	 * runs: the plain engine under the plain key.  A batch whose rows per evaluation the engine refuses (more than 128) is MLIS_E_OPT_VALUE at generation.  Not
	 * included: other layer selections, a step window or adaptive scale, self-attention guidance (guidance rescale: cfg_rescale below).  (A block of its own from 201.) */
	MLIS_OPT_AMD_PAG_SCALE = 201,          /* "pag_scale" (float 0 .. 20, default 0 = off; front ends default to 3 when it is switched on) */
	/* v-prediction checkpoints on a zero-terminal-SNR schedule, and the guidance rescale they are sampled with ("Common Diffusion Noise Schedules and Sample Steps are
	 * Flawed", 2023).  The prediction type is no longer tied to the model type: an SDXL checkpoint may be v-prediction.  None of the three is part of the engine key and
	 * none builds anything: they are handed to the engine per generation (include/mlimgsynth_amd.h, mlis_amd_set_prediction / _set_cfg_rescale).  At the defaults every
	 * generation returns the bytes it returned without them.  `auto` is what the model type says (sd2, tinyv: v) and what the checkpoint says: a tensor named "v_pred"
	 * makes it v-prediction, one named "ztsnr" selects the rescaled sigma table -- the published checkpoints' marker convention as recalled, parity-unpinned; the
	 * explicit values always win.  With zsnr the uniform schedule starts at sigma 4518.76 (the clamped last entry).  Not included: trailing / SGM timestep spacing, a
	 * step window for the rescale, dynamic thresholding, APG, CFG++.  (A block of its own from 211.) */
	MLIS_OPT_AMD_CFG_RESCALE = 211,        /* "cfg_rescale" (float 0 .. 1, default 0 = off; front ends use 0.7): phi of the guidance rescale */
	MLIS_OPT_AMD_PREDICTION = 212,         /* "prediction" (auto|eps|v or 0 .. 2, default auto) */
	MLIS_OPT_AMD_ZSNR = 213                /* "zsnr" (auto|off|on or 0 .. 2, default auto; n|y are accepted for off|on) */
} MLIS_Option;
enum { MLIS_AMD_INPAINT_WHOLE = 0, MLIS_AMD_INPAINT_MASKED = 1 };
enum { MLIS_AMD_RESAMPLE_NEAREST = 0, MLIS_AMD_RESAMPLE_BILINEAR = 1, MLIS_AMD_RESAMPLE_BICUBIC = 2 };
enum { MLIS_AMD_AA_BOX = 0, MLIS_AMD_AA_TRIANGLE = 1, MLIS_AMD_AA_CUBIC = 2, MLIS_AMD_AA_LANCZOS = 3 };
enum { MLIS_AMD_PREPROCESS_NONE = 0, MLIS_AMD_PREPROCESS_CANNY = 1, MLIS_AMD_PREPROCESS_INVERT = 2 };

typedef struct MLIS_Ctx MLIS_Ctx;                                                                            /* :352 */
typedef struct MLIS_Image { uint8_t* d; size_t sz; unsigned w, h, c; int flags; } MLIS_Image;                /* :356-363 */
typedef struct MLIS_Progress { MLIS_Stage stage; int step, step_end, nfe; double step_time, time; } MLIS_Progress;   /* :367-374 */
typedef struct MLIS_ErrorInfo { MLIS_ErrorCode code; const char* desc; } MLIS_ErrorInfo;                     /* :378-381 */
typedef struct MLIS_BackendInfo {                                                                            /* :385-394 */
	const char* name; unsigned n_dev;
	struct MLIS_BackendDeviceInfo { const char *name, *desc; size_t mem_free, mem_total; } *devs;
} MLIS_BackendInfo;
typedef struct MLIS_Tensor { float* d; int n[4]; int flags; } MLIS_Tensor;                                   /* :399-403 */
typedef int (*MLIS_Callback)(void*, MLIS_Ctx*, const MLIS_Progress*);                                       /* :408 */
typedef void (*MLIS_ErrorHandler)(void*, MLIS_Ctx*, const MLIS_ErrorInfo*);                                 /* :412 */

#define mlis_ctx_create() mlis_ctx_create_i(MLIS_VERSION)
MLIS_Ctx* mlis_ctx_create_i(int version);                                                                    /* :418-419 */
void mlis_ctx_destroy(MLIS_Ctx** pctx);                                                                      /* :423 */
const char* mlis_errstr_get(const MLIS_Ctx* ctx);                                                            /* :427 */
int mlis_option_set(MLIS_Ctx* ctx, MLIS_Option id, ...);                                                     /* :433 */
int mlis_option_set_str(MLIS_Ctx* ctx, const char* name, const char* value);                                 /* :443 */
int mlis_option_get(MLIS_Ctx* ctx, MLIS_Option id, ...);                                                     /* :450 */
int mlis_generate(MLIS_Ctx* ctx);                                                                            /* :457 */
MLIS_Image* mlis_image_get(MLIS_Ctx* ctx, int idx);                                                          /* :462 */
const char* mlis_infotext_get(MLIS_Ctx* ctx, int idx);                                                       /* :468 */
int mlis_setup(MLIS_Ctx* ctx);                                                                               /* :474 */
MLIS_Tensor* mlis_tensor_get(MLIS_Ctx* ctx, MLIS_TensorId id);                                               /* :479 */
const MLIS_BackendInfo* mlis_backend_info_get(MLIS_Ctx* ctx, unsigned idx, int flags);                       /* :485-486 */
/* :490-508 */
const char* mlis_stage_str(MLIS_Stage id);
const char* mlis_stage_desc(MLIS_Stage id);
MLIS_Stage mlis_stage_fromz(const char* str);
const char* mlis_method_str(MLIS_Method id);
MLIS_Method mlis_method_fromz(const char* str);
const char* mlis_sched_str(MLIS_Scheduler id);
MLIS_Scheduler mlis_sched_fromz(const char* str);
const char* mlis_loglvl_str(MLIS_LogLvl id);
MLIS_LogLvl mlis_loglvl_fromz(const char* str);
const char* mlis_model_type_str(MLIS_ModelType id);
const char* mlis_model_type_desc(MLIS_ModelType id);
MLIS_ModelType mlis_model_type_fromz(const char* str);
const char* mlis_option_str(MLIS_Option id);
MLIS_Option mlis_option_fromz(const char* str);
/* :515-549 */
int mlis_image_encode(MLIS_Ctx* ctx, const MLIS_Tensor* image, MLIS_Tensor* latent, int flags);
int mlis_image_decode(MLIS_Ctx* ctx, const MLIS_Tensor* latent, MLIS_Tensor* image, int flags);
int mlis_mask_encode(MLIS_Ctx* ctx, const MLIS_Tensor* mask, MLIS_Tensor* lmask, int flags);
int mlis_text_tokenize(MLIS_Ctx* ctx, const char* text, int32_t** ptokens, MLIS_SubModel model);
int mlis_clip_text_encode(MLIS_Ctx* ctx, const char* text, MLIS_Tensor* embed, MLIS_Tensor* feat, MLIS_SubModel model, int flags);
enum { MLIS_CTEF_NO_NORM = 1 };
/* :552-558 */
void mlis_tensor_free(MLIS_Tensor*);
size_t mlis_tensor_count(const MLIS_Tensor*);
void mlis_tensor_resize(MLIS_Tensor*, int n0, int n1, int n2, int n3);
void mlis_tensor_resize_like(MLIS_Tensor*, const MLIS_Tensor*);
void mlis_tensor_copy(MLIS_Tensor*, const MLIS_Tensor*);
float mlis_tensor_similarity(const MLIS_Tensor*, const MLIS_Tensor*);

/* ---- additions of this library (not in the reference) */
/* token ids instead of text for the next generation (no vocabulary needed: benchmarks, tests).  Cleared after generation
 * like PROMPT.  weights may be NULL. */
int mlis_amd_prompt_tokens_set(MLIS_Ctx* ctx, const int32_t* tokens, const float* weights, int n, int negative);
/* the engine behind the context (NULL before the first setup/generate): for multi-GPU drivers and profiling */
struct MLIS_AmdCtx* mlis_amd_engine_get(MLIS_Ctx* ctx);
/* engines constructed by this context so far.  A context keeps its two most recently used engines (one per model / size / batch / ... key),
 * so a workflow that alternates between two sizes -- the hires fix -- rebuilds nothing; mlis_amd_engine_get returns the one used last. */
int mlis_amd_engine_builds(MLIS_Ctx* ctx);
/* ControlNet: evaluations of pass 0 / 1 of the last mlis_generate in which the ControlNet ran (a hires generation has two passes); -1 for a pass that did not run */
int mlis_amd_control_evals(MLIS_Ctx* ctx, int pass);
/* LoRA bookkeeping, cumulative like mlis_amd_engine_builds.  A change of the LoRA set or of a multiplier while engines or text towers are resident is applied
 * to their weights in place on the GPU: every weight the old set had patched is restored from the checkpoint (n_restored counts weights per plan), the new
 * set's adapters are applied in option order by a kernel that repeats the host merge's arithmetic (n_patched, per plan and adapter tensor).  With nothing
 * resident the adapters are merged into the tensor store on the host before the first engine is built (n_cold_merges counts adapters).  The same list of
 * (file, multiplier) as the one applied costs nothing.  Any pointer may be NULL.  Returns 1. */
int mlis_amd_lora_stats(MLIS_Ctx* ctx, int* n_restored, int* n_patched, int* n_cold_merges);
/* dst = src resampled to w x h on the GPU (pixel centres, no antialiasing; mode MLIS_AMD_RESAMPLE_*): every n[2] * n[3] plane of src on its own.
 * Tap indices outside a plane are clamped to the border, or wrap around along the axes of the context's "tiling" option.  src == dst is allowed.
 * Returns 1, MLIS_E_OPT_VALUE for a bad mode or size. */
int mlis_amd_tensor_resample(MLIS_Ctx* ctx, const MLIS_Tensor* src, MLIS_Tensor* dst, int w, int h, int mode);
/* dst = src resampled to w x h on the GPU with a filter whose support grows with the shrink factor (MLIS_AMD_AA_*: box, triangle = antialiased bilinear, Keys cubic
 * with a = -0.5, lanczos3; what PIL's resize and torch's interpolate(antialias=True) compute); when enlarging, the filters interpolate.  Edges: taps outside a plane
 * are dropped and the rest renormalised, or wrap around along the axes of the context's "tiling" option.  src == dst is allowed; otherwise the contract of
 * mlis_amd_tensor_resample.  Returns 1, MLIS_E_OPT_VALUE for a bad filter or size. */
int mlis_amd_tensor_resample_aa(MLIS_Ctx* ctx, const MLIS_Tensor* src, MLIS_Tensor* dst, int w, int h, int filter);
/* dst = the Canny edge map of src on the GPU: src [w][h][1 or 3][1] floats in 0..1 -> dst [w][h][3][1], 1 on edges and 0 elsewhere, the three channels equal
 * (the rules: mlsd_canny in mlsd_kernels.h -- OpenCV's Canny(img_u8, low, high) with aperture 3 as recalled, parity-unpinned against OpenCV).  low, high: 0 .. 32767,
 * swapped if low > high; l2: 0 / 1; wrap: bit 0 columns, bit 1 rows wrap around (what "tiling" x / y / xy mean), 0 .. 3.  src == dst is allowed.  Needs no model.
 * Returns 1, MLIS_E_OPT_VALUE for bad arguments. */
int mlis_amd_tensor_canny(MLIS_Ctx* ctx, const MLIS_Tensor* src, MLIS_Tensor* dst, float low, float high, int l2, int wrap);
/* Region inpainting, piece by piece (the kernels and their rules: mlsd_kernels.h, "region inpainting").  Each goes from host tensors to the GPU and back, needs no model and
 * allows src == dst; wrap as in mlis_amd_tensor_canny.  They return 1, MLIS_E_OPT_VALUE for bad arguments.
 *   mask_weight  dst = clamp(invert ? src : 1 - src, 0, 1), any shape: the repaint weight p of a mask
 *   mask_grow    src [w][h][1][1]: maximum (radius > 0) or minimum (radius < 0) over the (2 |radius| + 1)^2 square, |radius| <= 256
 *   gauss_blur   every plane of src blurred with sigma 0 .. 64: radius (int)(2.5 sigma + 0.5), taps normalised in double; a border pixel is replicated (both as recalled
 *                from the front ends' OpenCV calls, parity-unpinned)
 *   mask_bbox    bbox = x0, y0, x1, y1 (half open) of the pixels of src [w][h][1][1] with a value > 0; 0, 0, 0, 0 if none
 *   composite    dst [W][H][c][B] = orig outside the rectangle at (x0, y0) of the patch's size, orig (1 - p) + patch p inside (fp32, each operation rounded once);
 *                orig [W][H][c][1 or B], patch [cw][ch][c][B], p [W][H][1][1].  dst may be orig or patch */
int mlis_amd_tensor_mask_weight(MLIS_Ctx* ctx, const MLIS_Tensor* src, MLIS_Tensor* dst, int invert);
int mlis_amd_tensor_mask_grow(MLIS_Ctx* ctx, const MLIS_Tensor* src, MLIS_Tensor* dst, int radius, int wrap);
int mlis_amd_tensor_gauss_blur(MLIS_Ctx* ctx, const MLIS_Tensor* src, MLIS_Tensor* dst, float sigma, int wrap);
int mlis_amd_tensor_mask_bbox(MLIS_Ctx* ctx, const MLIS_Tensor* src, int bbox[4]);
int mlis_amd_tensor_composite(MLIS_Ctx* ctx, MLIS_Tensor* dst, const MLIS_Tensor* orig, const MLIS_Tensor* patch, const MLIS_Tensor* p, int x0, int y0);
/* The region that inpaint_area masked processes, out = x0, y0, x1, y1 (half open), from the bounding box of the repaint weight; integers only, no context, no GPU.
 * This project's own rule:
 *  1. the box is padded by `padding` on each side and clamped to the W x H image; cw x ch is its size.
 *  2. the shorter side grows to the aspect tw : th of the processing size: if cw th < ch tw the width becomes min(W, ceil(ch tw / th)), otherwise the height becomes
 *     min(H, ceil(cw th / tw)).  Of the extra pixels floor(extra / 2) go to the left (top), the rest to the other side; a rectangle that then crosses an edge of the
 *     image is shifted back inside.
 * Returns 1; -1 for an empty or misplaced box (x0 < x1, y0 < y1, inside the image), W, H, tw or th below 1, or a negative padding. */
int mlis_amd_inpaint_region(int W, int H, const int bbox[4], int padding, int tw, int th, int out[4]);
/* of the last mlis_generate: region = the rectangle composited (the whole image with inpaint_area whole), proc = the size the pass ran at.  Returns 1, or 0 (and zeros) if
 * that generation composited nothing.  Either pointer may be NULL. */
int mlis_amd_inpaint_info(MLIS_Ctx* ctx, int region[4], int proc[2]);
/* dst = src upscaled 4x by the model of the "upscale_model" option: src [w][h][3][n] floats in 0..1 -> dst [4w][4h][3][n] (not clamped).  src == dst is allowed.
 * The upscaler is built on the first use and stays resident in the context until the option changes (mlis_amd_upscaler_builds counts the builds); the image border is
 * padded with zeros whatever "tiling" says.  Returns 1, MLIS_E_OPT_VALUE when no upscale_model is set or src is not a 3-channel image. */
int mlis_amd_tensor_upscale(MLIS_Ctx* ctx, const MLIS_Tensor* src, MLIS_Tensor* dst);
/* upscalers constructed by this context so far (cumulative, like mlis_amd_engine_builds); *resident = 1 while one is held */
int mlis_amd_upscaler_builds(MLIS_Ctx* ctx, int* resident);

#ifdef __cplusplus
}
#endif
#endif
