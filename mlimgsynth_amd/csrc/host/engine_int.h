/* The engine's state, shared by engine.c (creation, options, the denoising loop) and engine_vae.c (the VAE codec).  Private to csrc/host. */
#pragma once
#include "mlblock_int.h"
#include "mlimgsynth_amd.h"

#define MAX_STEPS 1001     /* the public option STEPS accepts 0..1000 like the reference (mlimgsynth_options_set.c.h); buffers that follow the step count are sized in ensure_steps */
#define MAX_BATCH 64
#define MAX_DRAWS (2 * MAX_STEPS + 2)
#define N_TMP 2

/* One direction of the VAE codec (engine_vae.c): the plan of the whole latent / image, and the tile-sized plan of MLIS_OPT_VAE_TILE (src/vae.c:245-300,333-391),
 * built on first use, with the buffers that hold one tile of every image of the batch: they follow the tile size. */
enum { CODEC_DEC, CODEC_ENC };
typedef struct { MLCtx *ctx; MLTensor *t_in; } CodecPlan;     /* a plan and its bound input */
typedef struct {
	CodecPlan full, tile;
	int tile_w, tile_h;         /* the tile plan's input size (decode: latent pixels, encode: image pixels) */
	float *d_tile_in, *d_tile_out;
	size_t tile_in_bytes, tile_out_bytes;   /* allocated bytes of the two */
	int n_tile_evals;           /* tile plan evaluations of the last tiled pass */
} CodecState;

struct MLIS_AmdCtx {
	MLIS_AmdConfig c;
	char model[16];
	void* stream;
	UnetParams unet_p;
	VaeParams vae_p;
	int lw, lh, hw, B, N;
	MLCtx *unet_ctx;
	int tiling;                 /* seamless tiling: mlctx_set_conv_wrap mode of the UNet, decoder and encoder plans (0 none, 1 x, 2 y, 3 xy) */
	UnetState unet;
	/* device state */
	float *d_x;                 /* latent [B][4][hw] NCHW fp32 */
	float *d_xsave;             /* copy of a caller-given initial latent while the denoising loop may have to be re-run (hand-off retry) */
	int n_handoff_retries;      /* denoise / decode / encode passes re-run on the hand-off-free plan after a timed-out in-launch hand-off */
	float *d_xin;               /* what the UNet plan reads (1 MB d2d copy per evaluation; keeps the plan independent of the solver) */
	float *d_dx;                /* dxdt */
	float *d_tmp[N_TMP];        /* solver state vectors (solver_tmp_get, solvers.c:54-76) */
	float *d_x0, *d_lmask;      /* in-painting: original latent, latent mask [hw] */
	float *d_img;               /* image  [B][3][H][W] fp32 */
	float *d_img_in;            /* encoder input image (NCHW fp32 [B][3][H][W], [0,1]) */
	float *d_cin;               /* [B] current c_in (read by the UNet input conversion) */
	float *d_noise;             /* [MAX draws][B][4*hw] */
	float *h_noise;             /* pinned, same shape */
	void *up_stream;            /* the draws are uploaded on a stream of their own (a 1 MB copy queued on the compute stream waits behind the copy engine's current job:
	                             * with streamed weights that is a 500 MB upload, 9 ms of an 80 ms evaluation); ev_draw[k] orders draw k before its consumer */
	void **ev_draw; int n_ev_draw;
	int32_t *d_nan;
	void *ev[2 * MAX_STEPS][2];
	int n_ev;
	float last_unet_ms;
	int last_nfe, last_n_step;
	int cond_set, have_init_latent, have_lmask;
	int own_stream;
	RngPhilox rng[MAX_BATCH];
	int cap_steps;
	int n_draw_max, n_draw_gen, k_draw;  /* noise draws of the current denoise call: planned / generated so far / consumed so far */
	int i_eval;
	mlis_amd_progress_fn cb; void* cb_user;
	/* the VAE codec (engine_vae.c) */
	CodecState codec[2];        /* CODEC_DEC, CODEC_ENC */
	int vae_tile;               /* MLIS_OPT_VAE_TILE (pixels) */
	int vae_attn;               /* mlis_amd_set_vae_attn: the mid-block attention of the KL-VAE plans (mlctx_set_vae_attn), full-size and tile-sized alike */
	float *d_mom;               /* moments of a tiled encode, NCHW [B][8][lh][lw] */
	/* tiled diffusion (mlis_amd_create_tiled_packed): the UNet plan has the size of one window (times `pack` in the batch), lw x lh above is the canvas */
	int n_win;                  /* windows per evaluation; 0: the plan takes the whole latent */
	int win_w, win_h, win_ox, win_oy;       /* window extent and overlap per axis, latent pixels */
	int tile_px, tile_overlap_px;           /* as asked for (pixels, square): infotext, engine key */
	int n_win_x, n_win_y, *win_xs, *win_ys; /* starts per axis (mlis_amd_window_starts); window j = (xs[j % n_win_x], ys[j / n_win_x]) */
	int pack, n_eval;           /* windows per plan evaluation (mlis_amd_tile_pack; 0: not tiled) and plan evaluations per UNet evaluation */
	int PB, PN;                 /* images and rows of the UNet plan: B and N, times pack when tiled */
	float *d_eps_canvas;        /* blended UNet output NHWC [N][hw][4] */
	float *d_wsum;              /* [hw] sum of the blend weights of the windows covering a pixel */
	/* ControlNet (MLIS_AmdConfig.control): the hint plan runs once per control image at the canvas's pixel size, the ControlNet plan before the UNet plan in every
	 * controlled evaluation, on the UNet plan's inputs; the UNet plan was built with the residuals' addresses and reads its gain from d_gain */
	MLCtx *ctl_ctx, *hint_ctx;
	ControlState ctl;
	UnetControl ctl_k;
	MLTensor *t_hint_img;
	float *d_gain;              /* [1] gain of the evaluation being enqueued: the strength, or 0 (outside the step window, no image, strength 0) */
	int ctl_image;              /* a control image is set: the hint embedding is current */
	uint64_t ctl_tag;           /* the caller's mark on that image (mlis_amd_control_tag_set) */
	float ctl_strength, ctl_start, ctl_end;
	int ctl_step_on;            /* the current step lies in the window (mlis_amd_control_active); mlis_amd_dxdt has no step: always */
	int ctl_evals;              /* evaluations of the last denoise / dxdt in which the ControlNet plan ran */
	/* FreeU (MLIS_AMD_CONTROL_FREEU): the UNet plan was built with the address of d_freeu; mlis_amd_set_freeu writes the four floats */
	UnetFreeU fu;
	float *d_freeu;             /* [4] b1, b2, s1, s2; all 1 (the plan's FreeU passes copy) until they are set */
	float freeu_f[4];
	/* perturbed-attention guidance (MLIS_AMD_CONTROL_PAG): the UNet plan carries a third row group, [cond | uncond | perturbed] (mlis_amd_eval_rows), whose middle-block
	 * self-attentions are the identity (mlctx_set_pag); dxdt_finish and the fused Euler step mix it in with pag_scale, a by-value kernel argument */
	int pag;                    /* the flag */
	float pag_scale;            /* 0 .. 20 (mlis_amd_set_pag); 0: the plain mix, the perturbed rows are computed and not read */
	int CN;                     /* rows of the ControlNet plan: PN without the perturbed group (it is never perturbed; the UNet plan's sums hand that group the cond residuals) */
	float tome_ratio; int tome_max_ds;      /* token merging (mlis_amd_set_tome): given to the UNet and ControlNet plans before they are built; a change rebuilds them */
	int ht_px, ht_depth;       /* HyperTile (MLIS_AMD_CONTROL_HYPERTILE): tile in pixels (0: off) and deepest tiled level, given to the UNet and ControlNet plans before they are built */
	/* guidance rescale (mlis_amd_set_cfg_rescale): the mix multiplies the guided prediction by a per-image factor (mlsd_guidance_stats).  The buffers exist only once
	 * a phi > 0 was set; the prediction type and the sigma table (mlis_amd_set_prediction) live in unet_p (vparam, zsnr).  None of it is in a plan. */
	float cfg_rescale;          /* phi, 0 .. 1; 0: the plain mix kernels */
	double *d_gr_part;          /* [B][mlsd_guidance_blocks(hw)][4] partial sums */
	float *d_gr_factor;         /* [B] the factors of the last rescaled mix */
	size_t gr_part_bytes;
	int gr_evals;               /* rescaled mixes since the engine was created */
	int vparam_model;           /* the model type's own prediction type (mlis_amd_set_prediction with a negative value goes back to it) */
	/* guidance limiters (mlis_amd_set_guidance_limit): dynamic thresholding or APG on the raw outputs, where cfg_scale > 1.  The buffers exist only once a mode was
	 * set; like the rescale, none of it is in a plan. */
	int limit_mode;             /* 0 off, MLSD_GLIMIT_DYNTHRESH, MLSD_GLIMIT_APG */
	float mimic, percentile;    /* thresholding: the scale whose range is kept (>= 1), the quantile of |g - mean| (0.5 .. 1) */
	float apg_eta, apg_norm;    /* APG: what is kept of the component parallel to cond (0 .. 1), the cap on |cond - uncond| per image (0: none) */
	double *d_gl_part;          /* mlsd_guidance_limit_scratch_bytes(B, 4, hw) */
	float *d_gl_means;          /* [B][4][2] plane means of the last thresholded mix */
	float *d_gl_lim;            /* [B][4][3] its triples, or [B][2] the coefficients of the last APG mix */
	size_t gl_part_bytes;
	int gl_evals, gl_lim_mode;  /* limited mixes since the engine was created; the mode of the last one (whose values d_gl_lim holds) */
};

static inline int fail(const char* msg) { return mlsd_set_error(-1, "%s", msg); }

/* engine.c */
const float* noise_draw(MLIS_AmdCtx* S, int k);      /* draw k for a consumer enqueued next on the compute stream */

/* engine_vae.c */
enum { CODEC_DROP_DEC = 1 << CODEC_DEC, CODEC_DROP_ENC = 1 << CODEC_ENC, CODEC_DROP_TILE = 4, CODEC_DROP_TILE_BUFS = 8, CODEC_DROP_ALL = 15 };
MLCtx* codec_full_prepare(MLIS_AmdCtx* S, int dir);
void codec_plans_drop(MLIS_AmdCtx* S, int which);
