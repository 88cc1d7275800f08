/* Generation driver — the slice of the reference's mlis_generate (src/mlimgsynth.c:1634-1773) that drives the hot
 * path: [image encode] -> schedule -> initial noise -> n_step x [dxdt (CFG UNet evaluation) + solver update
 * (+ ancestral / stochastic noise, in-painting blend)] -> latent decode.  The loop is a re-creation of
 * dnsamp_init / dnsamp_step (src/sampling.c:28-185) and of the five solvers (src/solvers.c:82-296) whose vector
 * loops run on the device (csrc/hip/sampler.hip, same fp32/fp64 operation order) while every scalar stays on the
 * host exactly as in the reference.  MI355X-first differences:
 *   - n_batch images per GPU; cond and uncond of all images form ONE batch-2B UNet evaluation
 *     (the reference runs two sequential batch-1 evaluations per dxdt, mlimgsynth.c:1578-1582);
 *   - the latent never leaves the device: c_in scaling happens in the UNet's input conversion, the CFG mix and
 *     the solver updates are elementwise kernels with by-value scalars; nothing in the loop synchronises
 *     (unless a progress callback is installed);
 *   - the Philox/Box-Muller noise is generated on the host (bit-exact integer stream, fp64 Box-Muller like
 *     src/ccommon/rng_philox.c) WHILE the GPU runs the UNet evaluation enqueued just before, then copied
 *     asynchronously; one independent stream per image (seed_i, offset 0: generate.sh:56-59 semantics);
 *   - weights stay resident in HBM (288 GB) for the lifetime of the context instead of being re-uploaded per
 *     generate (mlblock.c:266-292) or per half-graph (--unet-split, unet.c:390-458).
 */
#define _GNU_SOURCE       /* sched_getaffinity, CPU_COUNT */
#include "mlblock_int.h"
#include "mlimgsynth_amd.h"
#include <math.h>
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <unistd.h>


#define MAX_STEPS 1001     /* the public option STEPS accepts 0..1000 like the reference (mlimgsynth_options_set.c.h); buffers that follow the step count are sized in ensure_steps */
#define MAX_BATCH 64
#define MAX_DRAWS (2 * MAX_STEPS + 2)
#define N_TMP 2

struct MLIS_AmdCtx {
	MLIS_AmdConfig c;
	char model[16];
	void* stream;
	UnetParams unet_p;
	VaeParams vae_p;
	int lw, lh, hw, B, N;
	MLCtx *unet_ctx, *dec_ctx, *enc_ctx;
	int tiling;                 /* seamless tiling: mlctx_set_conv_wrap mode of the UNet, decoder and encoder plans (0 none, 1 x, 2 y, 3 xy) */
	UnetState unet;
	MLTensor *t_lat_dec, *t_img_enc;
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
	/* VAE tiling (MLIS_OPT_VAE_TILE; src/vae.c:245-300,333-391): tile-sized plans, built on first use */
	int vae_tile, tl_w, tl_h, ti_w, ti_h;             /* option (pixels); latent / image tile size of the decode and encode plans */
	MLCtx *dect_ctx, *enct_ctx;
	MLTensor *t_lat_dect, *t_img_enct;
	float *d_lat_tile, *d_img_tile, *d_imgin_tile, *d_mom_tile, *d_mom;
	size_t tile_bytes[4];                             /* allocated bytes of d_lat_tile, d_img_tile, d_imgin_tile, d_mom_tile: they follow the tile size */
	int n_tile_evals[2];                              /* tile plan evaluations of the last tiled decode / encode */
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
	int ht_px, ht_depth;        /* HyperTile (MLIS_AMD_CONTROL_HYPERTILE): tile in pixels (0: off) and deepest tiled level, given to the UNet and ControlNet plans before they are built */
	/* guidance rescale (mlis_amd_set_cfg_rescale): the mix multiplies the guided prediction by a per-image factor (mlsd_guidance_stats).  The buffers exist only once
	 * a phi > 0 was set; the prediction type and the sigma table (mlis_amd_set_prediction) live in unet_p (vparam, zsnr).  None of it is in a plan. */
	float cfg_rescale;          /* phi, 0 .. 1; 0: the plain mix kernels */
	double *d_gr_part;          /* [B][mlsd_guidance_blocks(hw)][4] partial sums */
	float *d_gr_factor;         /* [B] the factors of the last rescaled mix */
	size_t gr_part_bytes;
	int gr_evals;               /* rescaled mixes since the engine was created */
	int vparam_model;           /* the model type's own prediction type (mlis_amd_set_prediction with a negative value goes back to it) */
};

static int fail(const char* msg) { return mlsd_set_error(-1, "%s", msg); }

MLB_API void mlis_amd_destroy(MLIS_AmdCtx* S)
{
	if (!S) return;
	mlsd_stream_sync(S->stream);
	if (S->unet_ctx) mlctx_destroy(S->unet_ctx);
	if (S->ctl_ctx) mlctx_destroy(S->ctl_ctx);
	if (S->hint_ctx) mlctx_destroy(S->hint_ctx);
	mlsd_free(S->d_gain);
	mlsd_free(S->d_freeu);
	mlsd_free(S->d_gr_part); mlsd_free(S->d_gr_factor);
	if (S->dec_ctx) mlctx_destroy(S->dec_ctx);
	if (S->enc_ctx) mlctx_destroy(S->enc_ctx);
	if (S->dect_ctx) mlctx_destroy(S->dect_ctx);
	if (S->enct_ctx) mlctx_destroy(S->enct_ctx);
	mlsd_free(S->d_lat_tile); mlsd_free(S->d_img_tile); mlsd_free(S->d_imgin_tile); mlsd_free(S->d_mom_tile); mlsd_free(S->d_mom);
	mlsd_free(S->d_xin); mlsd_free(S->d_xsave);
	mlsd_free(S->d_eps_canvas); mlsd_free(S->d_wsum); free(S->win_xs); free(S->win_ys);
	mlsd_free(S->d_x); mlsd_free(S->d_dx); mlsd_free(S->d_x0); mlsd_free(S->d_lmask); mlsd_free(S->d_img); mlsd_free(S->d_img_in);
	for (int i=0;i<N_TMP;++i) mlsd_free(S->d_tmp[i]);
	mlsd_free(S->d_cin); mlsd_free(S->d_noise); mlsd_free(S->d_nan);
	mlsd_host_free(S->h_noise);
	for (int i=0;i<S->n_ev;++i) { mlsd_event_destroy(S->ev[i][0]); mlsd_event_destroy(S->ev[i][1]); }
	for (int i=0;i<S->n_ev_draw;++i) mlsd_event_destroy(S->ev_draw[i]);
	free(S->ev_draw);
	if (S->up_stream) { mlsd_stream_sync(S->up_stream); mlsd_stream_destroy(S->up_stream); }
	if (S->own_stream) mlsd_stream_destroy(S->stream);
	free(S);
}

/* buffers whose size follows the step count: noise draws (<= 2 per step + 2) and events (<= 2 per step) */
static int ensure_steps(MLIS_AmdCtx* S, int ns)
{
	if (ns >= MAX_STEPS) return fail("too many steps (max 1000)");
	if (ns <= S->cap_steps) return 1;
	const size_t lat_elems = (size_t)S->B * 4 * S->hw;
	mlsd_stream_sync(S->stream);
	if (S->up_stream) mlsd_stream_sync(S->up_stream);
	mlsd_free(S->d_noise); mlsd_host_free(S->h_noise);
	S->d_noise = NULL; S->h_noise = NULL; S->cap_steps = 0;
	S->n_draw_max = 2 * ns + 2;
	if (mlsd_malloc((void**)&S->d_noise, (size_t)S->n_draw_max*lat_elems*4)) return -1;
	if (mlsd_host_alloc((void**)&S->h_noise, (size_t)S->n_draw_max*lat_elems*4)) return -1;
	for (int i=S->n_ev; i<2*ns; ++i) { if (mlsd_event_create(&S->ev[i][0]) || mlsd_event_create(&S->ev[i][1])) return -1; S->n_ev = i+1; }
	if (!S->up_stream && mlsd_stream_create(&S->up_stream)) return -1;
	{	void **e = (void**)realloc(S->ev_draw, sizeof(void*) * (size_t)S->n_draw_max);
		if (!e) return fail("out of memory");
		S->ev_draw = e;
		for (int i=S->n_ev_draw; i<S->n_draw_max; ++i) { if (mlsd_event_create(&S->ev_draw[i])) return -1; S->n_ev_draw = i+1; }
	}
	S->cap_steps = ns;
	return 1;
}

static int solver_nfe(int method)
{	/* SolverClass.n_fe, src/solvers.c:90-296 */
	return (method == SOLVER_METHOD_HEUN || method == SOLVER_METHOD_DPMPP2S) ? 2 : 1;
}

/* rows of one UNet evaluation for B images: [cond B | uncond B (cfg_scale > 1) | perturbed B (pag)].  Pure; -1 for B < 1 */
MLB_API int mlis_amd_eval_rows(int B, float cfg_scale, int pag)
{
	if (B < 1) return -1;
	return (cfg_scale > 1 ? 2 * B : B) + (pag ? B : 0);
}

MLB_API MLIS_AmdCtx* mlis_amd_create(const MLIS_AmdConfig* cfg, void* stream) { return mlis_amd_create_ex(cfg, 0, stream); }

MLB_API int mlis_amd_tiling(const MLIS_AmdCtx* S) { return S ? S->tiling : 0; }

MLB_API MLIS_AmdCtx* mlis_amd_create_ex(const MLIS_AmdConfig* cfg, int tiling, void* stream) { return mlis_amd_create_tiled_packed(cfg, tiling, 0, 0, 0, 1, stream); }
MLB_API MLIS_AmdCtx* mlis_amd_create_tiled(const MLIS_AmdConfig* cfg, int tiling, int tile_w, int tile_h, int overlap, void* stream)
{
	return mlis_amd_create_tiled_packed(cfg, tiling, tile_w, tile_h, overlap, 1, stream);
}

/* ------------------------------------------------------------------ tiled diffusion: window geometry
 * Starts of the windows along one axis: canvas extent L, window extent T, minimum overlap O (latent pixels), wrap != 0 if the canvas tiles along the axis.
 *   T >= L          one window at 0 (its extent is L)
 *   T < L, no wrap  n = ceil((L - O) / (T - O)), starts[i] = floor(i (L - T) / (n - 1)): the first touches 0, the last touches L, the rest are spread evenly
 *   T < L, wrap     n = ceil(L / (T - O)), starts[i] = floor(i L / n): a ring, window i covers (starts[i] + k) mod L for k < T, one of them straddles the seam
 * Neighbours are at most T - O apart, so they share at least O pixels.  Returns n, or -1 for O < 0, 2 O > T, T < 1, L < 1 or n > cap. */
MLB_API int mlis_amd_window_starts(int L, int T, int O, int wrap, int* starts, int cap)
{
	if (!starts || O < 0 || T < 1 || L < 1 || 2 * (long)O > T) return -1;
	const long step = T - O;
	const long n = T >= L ? 1 : (wrap ? (L + step - 1) / step : (L - O + step - 1) / step);
	if (n > cap) return -1;
	for (long i=0; i<n; ++i) starts[i] = n == 1 ? 0 : (int)(wrap ? i * L / n : i * (L - T) / (n - 1));
	return (int)n;
}

/* The pack rule: n_win windows of n_batch images each, at most `pack` windows per plan evaluation.  P0 = min(pack, n_win, MLSD_WINDOW_MAX_PACK, MAX_BATCH / n_batch)
 * (a packed plan never holds more images than a plain engine may), *n_eval = ceil(n_win / P0) plan evaluations, and the pack returned is ceil(n_win / n_eval): the
 * smallest plan that reaches that count.  Group g holds windows g P .. min((g + 1) P, n_win) - 1 in evaluation order; only the last can be short.  -1 for an
 * argument below 1. */
MLB_API int mlis_amd_tile_pack(int n_win, int n_batch, int pack, int* n_eval)
{
	if (pack < 1 || n_win < 1 || n_batch < 1) return -1;
	int p0 = pack < n_win ? pack : n_win;
	if (p0 > MLSD_WINDOW_MAX_PACK) p0 = MLSD_WINDOW_MAX_PACK;
	if (p0 > MAX_BATCH / n_batch) p0 = MAX_BATCH / n_batch;
	if (p0 < 1) p0 = 1;
	const int ne = (n_win + p0 - 1) / p0;
	if (n_eval) *n_eval = ne;
	return (n_win + ne - 1) / ne;
}

MLB_API int mlis_amd_tile_pack_info(const MLIS_AmdCtx* S, int* pack, int* n_eval)
{	/* windows per plan evaluation and plan evaluations per UNet evaluation; a plain engine reports 0, 1 */
	if (!S) return -1;
	if (pack) *pack = S->n_win ? S->pack : 0;
	if (n_eval) *n_eval = S->n_win ? S->n_eval : 1;
	return 1;
}

/* the windows of a tiled engine: lists per axis, the weight-sum plane, the blended output */
static int windows_init(MLIS_AmdCtx* S, int tile_lw, int tile_lh, int overlap)
{
	int xs[MLSD_WINDOW_MAX_AXIS], ys[MLSD_WINDOW_MAX_AXIS];
	const int nx = mlis_amd_window_starts(S->lw, tile_lw, overlap, S->tiling & 1, xs, MLSD_WINDOW_MAX_AXIS);
	const int ny = mlis_amd_window_starts(S->lh, tile_lh, overlap, S->tiling & 2, ys, MLSD_WINDOW_MAX_AXIS);
	if (nx < 1 || ny < 1) return mlsd_set_error(-1, "tiled diffusion: no window layout for a %dx%d latent with %dx%d windows, overlap %d (2 x overlap <= window, at most %d windows per axis)",
		S->lw, S->lh, tile_lw, tile_lh, overlap, MLSD_WINDOW_MAX_AXIS);
	S->win_w = tile_lw < S->lw ? tile_lw : S->lw; S->win_h = tile_lh < S->lh ? tile_lh : S->lh;
	S->win_ox = S->win_oy = overlap;
	S->n_win_x = nx; S->n_win_y = ny; S->n_win = nx * ny;
	S->win_xs = (int*)malloc(sizeof(int) * (size_t)nx); S->win_ys = (int*)malloc(sizeof(int) * (size_t)ny);
	if (!S->win_xs || !S->win_ys) return fail("out of memory");
	memcpy(S->win_xs, xs, sizeof(int) * (size_t)nx); memcpy(S->win_ys, ys, sizeof(int) * (size_t)ny);
	if (mlsd_malloc((void**)&S->d_eps_canvas, (size_t)S->N * S->hw * 4 * 4) || mlsd_malloc((void**)&S->d_wsum, (size_t)S->hw * 4)) return -1;
	if (mlsd_window_wsum(S->d_wsum, S->lw, S->lh, S->win_w, S->win_h, xs, nx, ys, ny, S->win_ox, S->win_oy, S->stream)) return -1;
	return 1;
}

MLB_API int mlis_amd_tile_info(const MLIS_AmdCtx* S, int* n_win, int* win_w, int* win_h)
{	/* windows per evaluation (0: not tiled) and their size in latent pixels (not tiled: the latent's) */
	if (!S) return -1;
	if (n_win) *n_win = S->n_win;
	if (win_w) *win_w = S->n_win ? S->win_w : S->lw;
	if (win_h) *win_h = S->n_win ? S->win_h : S->lh;
	return 1;
}

MLB_API int mlis_amd_tile_windows(const MLIS_AmdCtx* S, int* xs, int* ys, int cap)
{	/* start of every window in evaluation order (row-major, y outer), latent pixels; returns their count, -1 if cap is too small */
	if (!S || S->n_win > cap) return -1;
	for (int j=0; j<S->n_win; ++j) { if (xs) xs[j] = S->win_xs[j % S->n_win_x]; if (ys) ys[j] = S->win_ys[j / S->n_win_x]; }
	return S->n_win;
}

/* Tiled diffusion (MultiDiffusion): cfg->width x height is the CANVAS -- sampler state, noise, mask, decoder and encoder have its size -- and the UNet plan is built
 * for P windows of min(tile, canvas) per axis, P = mlis_amd_tile_pack(windows, n_batch, pack): the plan of a plain engine for P x n_batch images with the shared
 * prompt.  Every evaluation runs the plan on each group of P windows and blends the outputs (unet_eval).  tile_w, tile_h, overlap in pixels (multiples of 8,
 * 2 x overlap <= tile); a tile of 0, or one that covers the canvas on both axes, gives the plain engine of mlis_amd_create_ex. */
MLB_API MLIS_AmdCtx* mlis_amd_create_tiled_packed(const MLIS_AmdConfig* cfg, int tiling, int tile_w, int tile_h, int overlap, int pack, void* stream)
{
	if (pack < 1 || pack > MLSD_WINDOW_MAX_PACK) { mlsd_set_error(-1, "tiled diffusion: %d windows per evaluation: 1 .. %d", pack, MLSD_WINDOW_MAX_PACK); return NULL; }
	const int tiled = tile_w > 0 && tile_h > 0 && (tile_w < cfg->width || tile_h < cfg->height);
	if (tiled && (tile_w % 8 || tile_h % 8 || overlap < 0 || overlap % 8 || 2 * overlap > tile_w || 2 * overlap > tile_h)) {
		mlsd_set_error(-1, "tiled diffusion: tile %dx%d, overlap %d: multiples of 8 with 2 x overlap <= tile", tile_w, tile_h, overlap); return NULL;
	}
	if (tiling < 0 || tiling > 3) { mlsd_set_error(-1, "tiling mode %d: 0 none, 1 x, 2 y, 3 xy", tiling); return NULL; }
	MLIS_AmdCtx *S = (MLIS_AmdCtx*)calloc(1, sizeof(*S));
	if (!S) { fail("out of memory"); return NULL; }
	S->tiling = tiling;
	S->c = *cfg; S->stream = stream;
	if (!stream) {   /* own non-default stream: stream capture (hipGraph) is not permitted on the NULL stream */
		if (mlsd_stream_create(&S->stream)) { free(S); return NULL; }
		S->own_stream = 1;
		stream = S->stream;
	}
	snprintf(S->model, sizeof(S->model), "%s", cfg->model ? cfg->model : "sd1");
	S->c.model = S->model;
	if (S->c.n_step < 1) S->c.n_step = 20;
	if (S->c.n_step >= MAX_STEPS) { fail("too many steps (max 1000)"); goto err; }
	if (S->c.n_batch < 1) S->c.n_batch = 1;
	if (!S->c.n_ctx_tok) S->c.n_ctx_tok = 77;
	if (S->c.n_ctx_tok < 0 || S->c.n_ctx_tok % 77 || S->c.n_ctx_tok > 77 * MLIS_AMD_MAX_WINDOWS) { mlsd_set_error(-1, "n_ctx_tok %d: 77 x W context rows, W <= %d", S->c.n_ctx_tok, MLIS_AMD_MAX_WINDOWS); goto err; }
	if (S->c.n_batch > MAX_BATCH) { fail("n_batch > 64 not supported"); goto err; }
	if (!(S->c.cfg_scale > 0)) S->c.cfg_scale = 7;          /* default cfg 7, src/mlimgsynth.c:474 */
	if (!S->c.sched) S->c.sched = DNSAMP_SCHED_UNIFORM;
	if (S->c.method <= 0) S->c.method = SOLVER_METHOD_EULER;   /* sampling.c:33 */
	if (S->c.method > SOLVER_METHOD_DPMPP2S) { mlsd_set_error(-1, "invalid sampling method %d", S->c.method); goto err; }
	if (!(S->c.f_t_ini > 0)) S->c.f_t_ini = 1;
	if (!S->c.weight_seed) S->c.weight_seed = 1234;
	{	/* the bits of `control`: 0 ControlNet, 1 FreeU, 2 HyperTile with its tile (bits 8..20, units of 8 px) and depth (bits 24..25), 3 perturbed-attention guidance */
		const int ht = S->c.control & MLIS_AMD_CONTROL_HYPERTILE, ht_bits = (0x1FFF << 8) | (3 << 24), ht_px = MLIS_AMD_CONTROL_HYPERTILE_PX(S->c.control);
		if (S->c.control & ~(MLIS_AMD_CONTROL_NET | MLIS_AMD_CONTROL_FREEU | MLIS_AMD_CONTROL_HYPERTILE | MLIS_AMD_CONTROL_PAG | ht_bits) || (!ht && (S->c.control & ht_bits))) {
			mlsd_set_error(-1, "control %d: bit 0 ControlNet, bit 1 FreeU, bit 2 HyperTile (tile / 8 in bits 8..20, depth in bits 24..25), bit 3 PAG", S->c.control); goto err;
		}
		S->pag = (S->c.control & MLIS_AMD_CONTROL_PAG) != 0;
		if (ht && (ht_px < 32 || ht_px > 8192)) { mlsd_set_error(-1, "HyperTile tile of %d px: 32 .. 8192, a multiple of 8", ht_px); goto err; }
		S->ht_px = ht ? ht_px : 0; S->ht_depth = ht ? MLIS_AMD_CONTROL_HYPERTILE_DEPTH(S->c.control) : 0;
	}
	S->ctl_strength = 1; S->ctl_start = 0; S->ctl_end = 1; S->ctl_step_on = 1;
	if (unet_params_get(S->model, &S->unet_p) < 0) goto err;
	S->vparam_model = S->unet_p.vparam;
	if (vae_params_get(S->model, &S->vae_p) < 0) goto err;
	if (S->c.width % 8 || S->c.height % 8 || S->c.width < 8 || S->c.height < 8) { fail("image size must be a multiple of 8"); goto err; }
	S->lw = S->c.width / S->vae_p.f_down; S->lh = S->c.height / S->vae_p.f_down; S->hw = S->lw * S->lh;
	S->B = S->c.n_batch;
	S->N = mlis_amd_eval_rows(S->B, S->c.cfg_scale, S->pag);
	S->PB = S->B; S->PN = S->N;
	/* (a plain engine holds at most 2 x MAX_BATCH rows: the third group must fit under the same cap) */
	if (S->N > MLIS_AMD_MAX_EVAL_ROWS) { mlsd_set_error(-1, "PAG: %d rows per evaluation (batch %d), at most %d", S->N, S->B, MLIS_AMD_MAX_EVAL_ROWS); goto err; }
	const int B = S->B, ns = S->c.n_step;
	const size_t lat_elems = (size_t)B * 4 * S->hw;

	if (mlsd_malloc((void**)&S->d_x, lat_elems*4)) goto err;
	if (mlsd_malloc((void**)&S->d_xin, lat_elems*4)) goto err;   /* the UNet plan's input: the evaluation point (x, or x1 of heun / dpmpp2s) is copied in */
	if (mlsd_malloc((void**)&S->d_dx, lat_elems*4)) goto err;
	for (int i=0;i<N_TMP;++i) if (mlsd_malloc((void**)&S->d_tmp[i], lat_elems*4)) goto err;
	if (mlsd_malloc((void**)&S->d_x0, lat_elems*4)) goto err;
	if (mlsd_malloc((void**)&S->d_lmask, (size_t)S->hw*4)) goto err;
	if (mlsd_malloc((void**)&S->d_img, (size_t)B*3*S->c.width*S->c.height*4)) goto err;
	if (mlsd_malloc((void**)&S->d_nan, 256)) goto err;
	if (ensure_steps(S, ns) < 0) goto err;
	/* tiled: the plan takes `pack` windows of every image.  It wraps only along an axis its window spans; elsewhere the ring of windows carries the wrap and a window edge pads with zeros */
	int ulw = S->lw, ulh = S->lh, unet_wrap = S->tiling;
	if (tiled) {
		S->tile_px = tile_w; S->tile_overlap_px = overlap;
		if (windows_init(S, tile_w / S->vae_p.f_down, tile_h / S->vae_p.f_down, overlap / S->vae_p.f_down) < 0) goto err;
		ulw = S->win_w; ulh = S->win_h;
		unet_wrap = S->tiling & ((ulw == S->lw ? 1 : 0) | (ulh == S->lh ? 2 : 0));
		S->pack = mlis_amd_tile_pack(S->n_win, B, pack, &S->n_eval);
		S->PB = S->pack * B; S->PN = S->pack * S->N;
		if (S->PN > MLIS_AMD_MAX_EVAL_ROWS) { mlsd_set_error(-1, "PAG: %d rows per plan evaluation (%d windows of batch %d), at most %d", S->PN, S->pack, B, MLIS_AMD_MAX_EVAL_ROWS); goto err; }
		mlsd_free(S->d_xin); S->d_xin = NULL;
		if (mlsd_malloc((void**)&S->d_xin, (size_t)S->PB * 4 * ulw * ulh * 4)) goto err;
	}
	if (mlsd_malloc((void**)&S->d_cin, (size_t)S->PB*4)) goto err;
	S->CN = S->PN - (S->pag ? S->PB : 0);

	/* ---- ControlNet: the hint plan at the canvas's pixel size and the ControlNet plan on the UNet plan's inputs, both before the UNet plan, which takes the residuals' addresses */
	if (S->c.control & MLIS_AMD_CONTROL_NET) {
		if (mlsd_malloc((void**)&S->d_gain, 256) || mlsd_memset(S->d_gain, 0, 256, stream)) goto err;
		S->hint_ctx = mlctx_new(stream);
		mlctx_set_conv_wrap(S->hint_ctx, S->tiling);
		if (control_hint_init(S->hint_ctx, &S->unet_p, S->c.width, S->c.height, &S->t_hint_img) < 0) goto err;
		if (control_hint_build(S->hint_ctx, &S->unet_p, S->t_hint_img) < 0) goto err;
		if (!S->c.defer_weights && mlctx_params_synth(S->hint_ctx, S->c.weight_seed) < 0) goto err;
		S->ctl_ctx = mlctx_new(stream);
		mlctx_set_conv_wrap(S->ctl_ctx, unet_wrap);
		mlctx_set_hypertile(S->ctl_ctx, S->ht_px, S->ht_depth);
		if (S->c.use_hipgraph && S->c.unet_split <= 0) mlctx_set_flags(S->ctl_ctx, MLB_F_HIPGRAPH);      /* (its weights stay resident with unet_split too) */
		if (controlnet_init_nc(&S->ctl, S->ctl_ctx, &S->unet_p, ulw, ulh, S->CN, S->c.n_ctx_tok) < 0) goto err;
		if (mlctx_input_bind(S->ctl.t_x, S->d_xin, S->PB, S->d_cin, 1.0f, 0) < 0) { fail("input bind failed"); goto err; }
		if (controlnet_build(&S->ctl) < 0) goto err;
		if (!S->c.defer_weights && mlctx_params_synth(S->ctl_ctx, S->c.weight_seed) < 0) goto err;
		if (controlnet_control(&S->ctl, S->d_gain, &S->ctl_k) < 0) goto err;
		{	/* the hint embedding travels as dense rows of n_ch floats: from the hint plan's result into the ControlNet plan's hint tensor (mlsd_window_gather_nhwc) */
			int64_t ldh = 0, ldw = 0;
			if (!mlctx_tensor_device_f32(S->hint_ctx, mlctx_result(S->hint_ctx), &ldh) || !mlctx_tensor_device_f32(S->ctl_ctx, S->ctl.t_hint, &ldw) ||
			    ldh != S->unet_p.n_ch || ldw != S->unet_p.n_ch) { mlsd_set_error(-1, "internal: hint embedding rows of %lld / %lld floats, %d channels", (long long)ldh, (long long)ldw, S->unet_p.n_ch); goto err; }
		}
	}

	/* ---- UNet plan, x bound to the resident evaluation point (c_in scaling + cond/uncond duplication in the gather) */
	S->unet_ctx = mlctx_new(stream);
	mlctx_set_conv_wrap(S->unet_ctx, unet_wrap);
	mlctx_set_hypertile(S->unet_ctx, S->ht_px, S->ht_depth);
	mlctx_set_pag(S->unet_ctx, S->pag ? S->PB : 0);
	if (S->c.unet_split > 0) {     /* --unet-split: the UNet's weights are streamed through three slabs (mlblock.c "weight streaming"); one evaluation = one pass over them */
		if (mlctx_set_weight_streaming(S->unet_ctx, S->c.unet_split > 1 ? (size_t)S->c.unet_split << 20 : 0) < 0) goto err;
	} else if (S->c.use_hipgraph) mlctx_set_flags(S->unet_ctx, MLB_F_HIPGRAPH);
	if (unet_denoise_init_nc(&S->unet, S->unet_ctx, &S->unet_p, ulw, ulh, S->PN, S->c.n_ctx_tok) < 0) goto err;
	if (mlctx_input_bind(S->unet.t_x, S->d_xin, S->PB, S->d_cin, 1.0f, 0) < 0) { fail("input bind failed"); goto err; }
	if (S->c.control & MLIS_AMD_CONTROL_FREEU) {      /* the factors live in device memory from the start: all 1, every FreeU pass of the plan a copy */
		for (int i=0;i<4;++i) S->freeu_f[i] = 1;
		if (mlsd_malloc((void**)&S->d_freeu, 256) || mlsd_memset(S->d_freeu, 0, 256, stream) || mlsd_memcpy(S->d_freeu, S->freeu_f, sizeof(S->freeu_f), 0, stream)
				|| mlsd_stream_sync(stream)) goto err;
		S->fu.f = S->d_freeu;
	}
	if (unet_denoise_build_freeu(&S->unet, (S->c.control & MLIS_AMD_CONTROL_NET) ? &S->ctl_k : NULL, (S->c.control & MLIS_AMD_CONTROL_FREEU) ? &S->fu : NULL) < 0) goto err;
	if (!S->c.defer_weights && mlctx_params_synth(S->unet_ctx, S->c.weight_seed) < 0) goto err;

	/* ---- decoder plan, latent input bound to the same resident latent */
	S->dec_ctx = mlctx_new(stream);
	mlctx_set_conv_wrap(S->dec_ctx, S->tiling);
	if (S->c.use_tae) {
		if (sdtae_decode_init(S->dec_ctx, S->lw, S->lh, B, &S->t_lat_dec) < 0) goto err;
		if (mlctx_input_bind(S->t_lat_dec, S->d_x, B, NULL, 1.0f, 1) < 0) goto err;
		if (sdtae_decode_build(S->dec_ctx, S->t_lat_dec) < 0) goto err;
	} else {
		if (sdvae_decode_init(S->dec_ctx, &S->vae_p, S->lw, S->lh, B, &S->t_lat_dec) < 0) goto err;
		if (mlctx_input_bind(S->t_lat_dec, S->d_x, B, NULL, 1 / S->vae_p.scale_factor, 0) < 0) goto err;
		if (sdvae_decode_build(S->dec_ctx, &S->vae_p, S->t_lat_dec) < 0) goto err;
	}
	if (!S->c.defer_weights && mlctx_params_synth(S->dec_ctx, S->c.weight_seed) < 0) goto err;
	return S;
err:
	mlis_amd_destroy(S);
	return NULL;
}

/* sampler options may change between generations without rebuilding the plans (the reference re-reads them in dnsamp_init on
 * every mlis_generate).  cfg_scale may change freely on its side of 1 (crossing it changes the UNet batch: new context). */
MLB_API int mlis_amd_set_sampler(MLIS_AmdCtx* S, int n_step, int method, int sched, float cfg_scale, float s_ancestral, float s_noise,
	float f_t_ini, float f_t_end)
{
	if (n_step < 1) n_step = 20;
	if (method <= 0) method = SOLVER_METHOD_EULER;
	if (method > SOLVER_METHOD_DPMPP2S) return mlsd_set_error(-4, "invalid sampling method %d", method);
	if (sched && sched != DNSAMP_SCHED_UNIFORM && sched != DNSAMP_SCHED_KARRAS) return mlsd_set_error(-4, "invalid sampling scheduler %d", sched);
	if (!(cfg_scale > 0)) cfg_scale = 7;
	if ((cfg_scale > 1) != (S->c.cfg_scale > 1)) return fail("cfg_scale crossing 1 changes the UNet batch: create a new context");
	if (ensure_steps(S, n_step) < 0) return -1;
	S->c.n_step = n_step; S->c.method = method; S->c.sched = sched ? sched : DNSAMP_SCHED_UNIFORM; S->c.cfg_scale = cfg_scale;
	S->c.s_ancestral = s_ancestral; S->c.s_noise = s_noise; S->c.f_t_ini = f_t_ini > 0 ? f_t_ini : 1; S->c.f_t_end = f_t_end;
	return 1;
}

MLB_API int mlis_amd_set_callback(MLIS_AmdCtx* S, mlis_amd_progress_fn fn, void* user)
{
	S->cb = fn; S->cb_user = user;
	return 1;
}

static int fill_cond(MLIS_AmdCtx* S, MLTensor* t, int rows, const void* a, const void* b, size_t per_bytes, int kind)
{	/* rows 0..PB-1 <- a (cond), rows PB..2PB-1 <- b (uncond) when the plan has that group, and the perturbed group (the UNet plan of a PAG engine: its last PB of
	 * `rows` rows) <- a again; the shared prompt is replicated per image (of every window of a packed plan) */
	char *dst = (char*)mlctx_input_device_ptr(t);
	const int p0 = S->pag && rows == S->PN ? rows - S->PB : rows;
	for (int n=0; n<rows; ++n) {
		const void *src = n < S->PB || n >= p0 ? a : b;
		if (!src) return fail("missing (un)conditioning");
		if (mlsd_memcpy(dst + (size_t)n*per_bytes, src, per_bytes, kind, S->stream)) return -1;
	}
	return 1;
}

static int set_cond(MLIS_AmdCtx* S, const void* cond, const void* label, const void* uncond, const void* unlabel, int kind)
{
	const UnetParams *P = &S->unet_p;
	if (fill_cond(S, S->unet.t_c, S->PN, cond, uncond, (size_t)S->c.n_ctx_tok*P->n_ctx*4, kind) < 0) return -1;
	if (P->ch_adm_in && fill_cond(S, S->unet.t_l, S->PN, label, unlabel, (size_t)P->ch_adm_in*4, kind) < 0) return -1;
	if (S->ctl_ctx) {      /* the ControlNet plan takes the same conditioning */
		if (fill_cond(S, S->ctl.t_c, S->CN, cond, uncond, (size_t)S->c.n_ctx_tok*P->n_ctx*4, kind) < 0) return -1;
		if (P->ch_adm_in && fill_cond(S, S->ctl.t_l, S->CN, label, unlabel, (size_t)P->ch_adm_in*4, kind) < 0) return -1;
	}
	if (mlsd_stream_sync(S->stream)) return -1;
	S->cond_set = 1;
	return 1;
}

MLB_API int mlis_amd_set_cond(MLIS_AmdCtx* S, const float* cond, const float* label, const float* uncond, const float* unlabel)
{
	return set_cond(S, cond, label, uncond, unlabel, 0);
}

MLB_API int mlis_amd_set_cond_device(MLIS_AmdCtx* S, const void* cond, const void* label, const void* uncond, const void* unlabel)
{
	return set_cond(S, cond, label, uncond, unlabel, 2);
}

/* ------------------------------------------------------------------ multi-GPU (one process per GPU, images sharded over ranks)
 * rank `root` has set the conditioning (mlis_amd_set_cond*); every rank then calls this: the plan's conditioning inputs are
 * broadcast in place over RCCL (cond [N][77][n_ctx] + label [N][adm] fp32: 1.3 MB for SDXL), no host hop, no per-step collective */
MLB_API int mlis_amd_bcast_cond(MLIS_AmdCtx* S, void* comm, int root)
{
	const UnetParams *P = &S->unet_p;
	if (mlsd_rccl_bcast(comm, mlctx_input_device_ptr(S->unet.t_c), (size_t)S->PN*S->c.n_ctx_tok*P->n_ctx*4, root, S->stream)) return -1;
	if (P->ch_adm_in && mlsd_rccl_bcast(comm, mlctx_input_device_ptr(S->unet.t_l), (size_t)S->PN*P->ch_adm_in*4, root, S->stream)) return -1;
	S->cond_set = 1;
	return 1;
}

/* all-gather of the final latents (what = 0: [B][4][lh][lw] fp32 per rank) or decoded images (what = 1: [B][3][H][W] fp32) into
 * `recv_dev` (world x the per-rank size, rank-major) on every rank; asynchronous on the engine's stream */
MLB_API int mlis_amd_gather_results(MLIS_AmdCtx* S, void* comm, int what, void* recv_dev)
{
	const size_t nb = what ? (size_t)S->B*3*S->c.width*S->c.height*4 : (size_t)S->B*4*S->hw*4;
	return mlsd_rccl_all_gather(comm, what ? (void*)S->d_img : (void*)S->d_x, recv_dev, nb, S->stream) ? -1 : 1;
}

/* read-only view of the conditioning the UNet plan will use (what = 0: cond [N][n_ctx_tok][n_ctx] fp32, 1: label [N][adm]): tests */
MLB_API const void* mlis_amd_cond_device(MLIS_AmdCtx* S, int what)
{
	MLTensor *t = what ? S->unet.t_l : S->unet.t_c;
	return t ? t->in_stage : NULL;
}

MLB_API int mlis_amd_seed(MLIS_AmdCtx* S, const uint64_t* seeds)
{
	for (int b=0;b<S->B;++b) { S->rng[b].seed = seeds[b]; S->rng[b].offset = 0; }
	return 1;
}

MLB_API int mlis_amd_seed_ex(MLIS_AmdCtx* S, const uint64_t* seeds, uint32_t offset)
{
	for (int b=0;b<S->B;++b) { S->rng[b].seed = seeds[b]; S->rng[b].offset = offset; }
	return 1;
}
MLB_API uint32_t mlis_amd_rng_offset(const MLIS_AmdCtx* S) { return S->rng[0].offset; }

/* initial latent for img2img (MLIS_TUF_LATENT, src/mlimgsynth.c:1661-1666): host NCHW [B][4][lh][lw], or NULL to go back
 * to txt2img (zero latent) */
MLB_API int mlis_amd_set_init_latent(MLIS_AmdCtx* S, const float* latent)
{
	if (!latent) { S->have_init_latent = 0; return 1; }
	if (mlsd_memcpy(S->d_x, latent, (size_t)S->B*4*S->hw*4, 0, S->stream) || mlsd_stream_sync(S->stream)) return -1;
	S->have_init_latent = 1;
	return 1;
}

/* latent mask for in-painting (MLIS_TUF_LMASK): host [lh][lw], 1 = keep the original latent; NULL clears it */
MLB_API int mlis_amd_set_lmask(MLIS_AmdCtx* S, const float* lmask)
{
	if (!lmask) { S->have_lmask = 0; return 1; }
	if (mlsd_memcpy(S->d_lmask, lmask, (size_t)S->hw*4, 0, S->stream) || mlsd_stream_sync(S->stream)) return -1;
	S->have_lmask = 1;
	return 1;
}

/* ------------------------------------------------------------------ noise draws
 * Every dnsamp_noise_add (src/sampling.c:112-117) is one rng_randn call of the whole latent per image.  Which draws a
 * run makes is known from the schedule alone, so draw k is generated on the host as soon as the evaluation before it
 * has been enqueued (the GPU is busy for tens of ms) and uploaded asynchronously. */
/* One draw = rng_philox_randn of the whole latent per image (src/ccommon/rng_philox.c:23-51): value i of image b is a pure function of (seed_b, offset_b, i), so the
 * B x 4 x hw values are cut into ranges over host threads -- bit-identical by construction (round 5: the single-threaded draw of the FIRST noise, 4 x 65 536 Box-Muller values
 * in fp64 before any GPU work, was 12 ms of every SDXL batch-4 step). */
typedef struct { const RngPhilox* rng; unsigned i0, i1; float* out; } DrawJob;
enum { DRAW_MAXT = 16, DRAW_MIN_CHUNK = 8192 };      /* (a range per 8192 values at least, 16 threads at most) */

/* CPUs this process is GRANTED, not the ones the machine has: scheduler affinity and the cgroup CPU quota -- the GPU box shows 256 logical CPUs and grants 16;
 * on a pod with a quota of 1-4 a thread per online CPU would oversubscribe the very thread that enqueues the GPU work. */
static int granted_cpus(void)
{
	long n = sysconf(_SC_NPROCESSORS_ONLN);
	if (n < 1) n = 1;
	cpu_set_t set;
	if (!sched_getaffinity(0, sizeof(set), &set)) { const int a = CPU_COUNT(&set); if (a >= 1 && a < n) n = a; }
	FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");                      /* cgroup v2: "<quota|max> <period>" */
	if (f) {
		char q[32]; long per = 0;
		if (fscanf(f, "%31s %ld", q, &per) == 2 && per > 0 && q[0] != 'm') { const long c = atol(q) / per; if (c >= 1 && c < n) n = c; else if (c < 1) n = 1; }
		fclose(f);
	} else {
		long q = -1, per = 0;                                             /* cgroup v1 */
		if ((f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"))) { if (fscanf(f, "%ld", &q) != 1) q = -1; fclose(f); }
		if ((f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r"))) { if (fscanf(f, "%ld", &per) != 1) per = 0; fclose(f); }
		if (q > 0 && per > 0) { const long c = q / per; if (c >= 1 && c < n) n = c; else if (c < 1) n = 1; }
	}
	return (int)n;
}

/* A small PERSISTENT pool (process-wide, started at the first multi-range draw, alive until exit): a draw used to create and join up to 15 threads each time.  The caller
 * publishes the job array, works on it itself, and returns when every range is done; a pool of zero workers (one granted CPU, or pthread_create failing) degrades to the
 * caller running every range.  One draw at a time (call_mu): engines of different threads share the workers. */
static struct {
	pthread_mutex_t call_mu, mu; pthread_cond_t cv_work, cv_done;
	const DrawJob *jobs; int n_jobs, next, done, n_workers, started;
} g_draw = { PTHREAD_MUTEX_INITIALIZER, PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, PTHREAD_COND_INITIALIZER, NULL, 0, 0, 0, 0, 0 };

static void* draw_pool_worker(void* arg)
{
	(void)arg;
	pthread_mutex_lock(&g_draw.mu);
	for (;;) {
		while (g_draw.next >= g_draw.n_jobs) pthread_cond_wait(&g_draw.cv_work, &g_draw.mu);
		const DrawJob *j = &g_draw.jobs[g_draw.next++];
		pthread_mutex_unlock(&g_draw.mu);
		rng_philox_randn_range(j->rng, j->i0, j->i1, j->out);
		pthread_mutex_lock(&g_draw.mu);
		if (++g_draw.done == g_draw.n_jobs) pthread_cond_signal(&g_draw.cv_done);
	}
	return NULL;
}

static void draw_run(const DrawJob* jobs, int nj)
{
	if (nj <= 1) { for (int j=0;j<nj;++j) rng_philox_randn_range(jobs[j].rng, jobs[j].i0, jobs[j].i1, jobs[j].out); return; }
	pthread_mutex_lock(&g_draw.call_mu);
	pthread_mutex_lock(&g_draw.mu);
	if (!g_draw.started) {
		g_draw.started = 1;
		int want = granted_cpus(); if (want > DRAW_MAXT) want = DRAW_MAXT;
		pthread_attr_t at; pthread_attr_init(&at); pthread_attr_setdetachstate(&at, PTHREAD_CREATE_DETACHED);
		for (int k=1;k<want;++k) { pthread_t t; if (pthread_create(&t, &at, draw_pool_worker, NULL)) break; g_draw.n_workers++; }      /* (the caller is thread 0) */
		pthread_attr_destroy(&at);
	}
	g_draw.jobs = jobs; g_draw.n_jobs = nj; g_draw.next = 0; g_draw.done = 0;
	pthread_cond_broadcast(&g_draw.cv_work);
	while (g_draw.next < g_draw.n_jobs) {
		const DrawJob *j = &g_draw.jobs[g_draw.next++];
		pthread_mutex_unlock(&g_draw.mu);
		rng_philox_randn_range(j->rng, j->i0, j->i1, j->out);
		pthread_mutex_lock(&g_draw.mu);
		g_draw.done++;
	}
	while (g_draw.done < g_draw.n_jobs) pthread_cond_wait(&g_draw.cv_done, &g_draw.mu);
	g_draw.jobs = NULL; g_draw.n_jobs = 0; g_draw.next = 0; g_draw.done = 0;
	pthread_mutex_unlock(&g_draw.mu);
	pthread_mutex_unlock(&g_draw.call_mu);
}

static void draw_all(MLIS_AmdCtx* S, float* hn, size_t per)
{
	static int ncpu = 0;
	if (!ncpu) { const int n = granted_cpus(); ncpu = n > DRAW_MAXT ? DRAW_MAXT : n; }
	const size_t total = (size_t)S->B * per;
	int nt = (int)(total / DRAW_MIN_CHUNK); if (nt > ncpu) nt = ncpu; if (nt < 1) nt = 1;
	int per_img = (nt + S->B - 1) / S->B; if (per_img < 1) per_img = 1;       /* ranges never straddle images */
	DrawJob jobs[MAX_BATCH * DRAW_MAXT];
	int nj = 0;
	for (int b=0;b<S->B;++b) for (int q=0;q<per_img;++q) {
		const unsigned i0 = (unsigned)(per * q / per_img), i1 = (unsigned)(per * (q + 1) / per_img);
		jobs[nj++] = (DrawJob){ &S->rng[b], i0, i1, hn + (size_t)b*per + i0 };
	}
	draw_run(jobs, nj);
	for (int b=0;b<S->B;++b) S->rng[b].offset++;
}

static const float* noise_gen(MLIS_AmdCtx* S, int k)
{	/* generate and upload every draw up to k (upload stream; nothing is enqueued on the compute stream) */
	const size_t per = (size_t)4 * S->hw, lat_elems = (size_t)S->B * per;
	if (k >= S->n_draw_max) { fail("internal: too many noise draws"); return NULL; }
	for (; S->n_draw_gen <= k; S->n_draw_gen++) {
		float *hn = S->h_noise + (size_t)S->n_draw_gen*lat_elems, *dn = S->d_noise + (size_t)S->n_draw_gen*lat_elems;
		draw_all(S, hn, per);
		if (mlsd_memcpy(dn, hn, lat_elems*4, 0, S->up_stream) || mlsd_event_record(S->ev_draw[S->n_draw_gen], S->up_stream)) return NULL;
	}
	return S->d_noise + (size_t)k*lat_elems;
}
static const float* noise_draw(MLIS_AmdCtx* S, int k)
{	/* draw k for a consumer enqueued next on the compute stream: that stream waits for the draw's upload */
	const float *nz = noise_gen(S, k);
	if (nz && mlsd_stream_wait_event(S->stream, S->ev_draw[k])) return NULL;
	return nz;
}

/* the in-launch hand-offs of the plans an evaluation runs (UNet, ControlNet): checked together, switched off together */
static int eval_handoff_ops(MLIS_AmdCtx* S) { return mlctx_handoff_ops(S->unet_ctx) + (S->ctl_ctx ? mlctx_handoff_ops(S->ctl_ctx) : 0); }
static int eval_handoff_check(MLIS_AmdCtx* S)
{
	const int a = mlctx_handoff_check(S->unet_ctx), b = S->ctl_ctx ? mlctx_handoff_check(S->ctl_ctx) : 0;      /* (both: a check also clears the plan's flags) */
	return a < 0 || b < 0 ? -1 : 0;
}
static void eval_handoffs_off(MLIS_AmdCtx* S) { mlctx_handoffs_off(S->unet_ctx); if (S->ctl_ctx) mlctx_handoffs_off(S->ctl_ctx); }

/* mlis_denoise_dxdt + unet_denoise_run_n (src/mlimgsynth.c:1565-1587, src/unet.c:460-498): one batched evaluation at
 * x_eval (device), sigma -> raw UNet output stays in the plan's result tensor.  `prefetch_draws`: noise draws to generate
 * on the host while this evaluation runs. */
static int unet_eval(MLIS_AmdCtx* S, const float* x_eval, float sigma, int prefetch_upto)
{
	const UnetParams *P = &S->unet_p;
	const int B = S->B, N = S->N;
	void *st = S->stream;
	if (S->i_eval >= 2*S->cap_steps) return fail("internal: too many evaluations");
	const float t = unet_sigma_to_t(P, sigma);
	const float c_in = 1 / sqrt(sigma*sigma + 1);                /* unet.c:471 */
	float *d_t_in = (float*)mlctx_input_device_ptr(S->unet.t_t);
	/* the same timestep for every row and the same c_in for every image: written by a kernel from its arguments.  (As two 64-byte copies they queued behind the copy
	 * engine's current job -- with streamed weights a 500 MB upload: 10 ms gaps in front of 4 of 20 evaluations, MLSD_ENGINE_TRACE.) */
	if (mlsd_fill2_f32(d_t_in, S->PN, t, S->d_cin, S->PB, c_in, st)) return -1;
	/* ControlNet: the plan runs in front of the UNet plan when this evaluation is controlled; either way the UNet plan's sums read the gain written here */
	const int ctl_on = S->ctl_ctx && S->ctl_image && S->ctl_strength > 0 && S->ctl_step_on;
	if (S->ctl_ctx && mlsd_fill2_f32((float*)mlctx_input_device_ptr(S->ctl.t_t), S->CN, t, S->d_gain, 1, ctl_on ? S->ctl_strength : 0.f, st)) return -1;
	if (ctl_on) S->ctl_evals++;
	int64_t ld = 0;
	const float *eps = mlctx_tensor_device_f32(S->unet_ctx, S->unet.t_out, &ld);
	if (S->n_win) {
		/* tiled diffusion: the plan runs on every window of the canvas, a group of `pack` windows of every image in one evaluation; the raw outputs are blended into
		 * d_eps_canvas group after group, and inside a group in slot order (a fixed summation order: that of one launch per window).  The unused slots of a short
		 * last group repeat its last window -- the plan sees real inputs everywhere -- and the blend skips them.  Exact, not an approximation: the CFG mix and the
		 * v-prediction rescale that follow are affine in eps with coefficients that depend only on sigma and on x_eval at the same pixel. */
		const int whw = S->win_w * S->win_h, P = S->pack;
		mlsd_event_record(S->ev[S->i_eval][0], st);
		if (mlsd_memset(S->d_eps_canvas, 0, (size_t)N * S->hw * 4 * 4, st)) return -1;
		for (int g=0; g<S->n_eval; ++g) {
			const int n_used = S->n_win - g*P < P ? S->n_win - g*P : P;
			int xs[MLSD_WINDOW_MAX_PACK], ys[MLSD_WINDOW_MAX_PACK];
			for (int s=0; s<P; ++s) {
				const int j = g*P + (s < n_used ? s : n_used - 1);
				xs[s] = S->win_xs[j % S->n_win_x]; ys[s] = S->win_ys[j / S->n_win_x];
			}
			if (mlsd_window_gather_packed(x_eval, S->lw, S->lh, S->d_xin, S->win_w, S->win_h, xs, ys, P, B*4, st)) return -1;
			if (ctl_on) {      /* every slot's crop of the canvas's hint embedding, for the cond and the uncond rows of the plan: [N / B][P][B] images */
				const int nch = S->unet_p.n_ch;              /* (both row strides are n_ch: checked when the engine was created) */
				const float *hs = mlctx_tensor_device_f32(S->hint_ctx, mlctx_result(S->hint_ctx), NULL);
				float *hw_ = (float*)mlctx_tensor_device_f32(S->ctl_ctx, S->ctl.t_hint, NULL);
				for (int q=0; q<S->CN/S->PB; ++q)
					if (mlsd_window_gather_nhwc(hs, S->lw, S->lh, nch, hw_ + (size_t)q * P * B * whw * nch, S->win_w, S->win_h, xs, ys, P, B, st)) return -1;
				if (mlctx_compute(S->ctl_ctx) < 0) return -1;
			}
			if (mlctx_compute(S->unet_ctx) < 0) return -1;
			/* (the blend takes one or two row groups: the third group of a PAG engine is a launch of its own, on that group's part of both buffers) */
			for (int q=0; q<N/B; q+=2) {
				const int nq = N/B - q < 2 ? N/B - q : 2;
				if (mlsd_window_blend_packed(eps + (size_t)q * P * B * whw * ld, ld, S->d_eps_canvas + (size_t)q * B * S->hw * 4, S->d_wsum, S->lw, S->lh, S->win_w, S->win_h, xs, ys,
						n_used, P, S->win_ox, S->win_oy, B, nq, 4, st)) return -1;
			}
			if (mlsd_count_nonfinite(eps, (size_t)S->PN*whw*ld, S->d_nan, st)) return -1;
			if (g == 0 && prefetch_upto >= 0 && !noise_gen(S, prefetch_upto)) return -1;
		}
		mlsd_event_record(S->ev[S->i_eval][1], st);
		S->i_eval++;
		S->last_nfe += N / B;
		return 1;
	}
	if (x_eval != S->d_xin && mlsd_memcpy(S->d_xin, x_eval, (size_t)B*4*S->hw*4, 2, st)) return -1;
	mlsd_event_record(S->ev[S->i_eval][0], st);
	if (ctl_on && mlctx_compute(S->ctl_ctx) < 0) return -1;
	if (mlctx_compute(S->unet_ctx) < 0) return -1;               /* cond + uncond of all images: one evaluation */
	mlsd_event_record(S->ev[S->i_eval][1], st);
	S->i_eval++;
	S->last_nfe += N / B;
	if (mlsd_count_nonfinite(eps, (size_t)N*S->hw*ld, S->d_nan, st)) return -1;   /* ltensor_finite_check, unet.c:487 */
	if (prefetch_upto >= 0 && !noise_gen(S, prefetch_upto)) return -1;
	return 1;
}

/* the UNet output the solvers read, NHWC [2B|B][hw][*ld]: the plan's result tensor, or the blend of the windows' */
static const float* eps_get(MLIS_AmdCtx* S, int64_t* ld)
{
	if (S->n_win) { *ld = 4; return S->d_eps_canvas; }
	return mlctx_tensor_device_f32(S->unet_ctx, S->unet.t_out, ld);
}

/* guidance rescale runs where phi > 0 and the guided prediction is not the cond prediction itself; elsewhere no factor, and the plain mix's bytes */
static int rescale_on(const MLIS_AmdCtx* S) { return S->cfg_rescale > 0 && (S->c.cfg_scale > 1 || (S->pag && S->pag_scale != 0)); }

/* what the mix entries take beside cfg_scale: the PAG scale and, with the rescale on, the factors of this evaluation's raw outputs (the blended canvas of a tiled
 * engine: the whole image), whose statistics are enqueued here; < 0 on error */
static int guidance_args(MLIS_AmdCtx* S, const float* eps, int64_t ld, float* pag, const float** factor)
{
	*pag = S->pag ? S->pag_scale : 0;
	*factor = NULL;
	if (!rescale_on(S)) return 1;
	*factor = S->d_gr_factor;
	S->gr_evals++;
	return mlsd_guidance_stats(eps, ld, S->B, 4, S->hw, S->c.cfg_scale, *pag, S->cfg_rescale, S->d_gr_part, S->gr_part_bytes, S->d_gr_factor, S->stream) ? -1 : 1;
}

/* dx = guidance mix (+ v-param rescale) of the evaluation just enqueued */
static int dxdt_finish(MLIS_AmdCtx* S, const float* x_eval, float sigma, float* dx)
{
	int64_t ld = 0;
	const float *eps = eps_get(S, &ld), *factor;
	const float c_skip = sigma / (sigma*sigma + 1), c_out = 1 / sqrt(sigma*sigma + 1);   /* unet.c:491-492 */
	float pag;
	if (guidance_args(S, eps, ld, &pag, &factor) < 0) return -1;
	return mlsd_dxdt_guided(eps, ld, x_eval, dx, S->B, 4, S->hw, S->c.cfg_scale, pag, factor, S->unet_p.vparam, c_out, c_skip, S->stream) ? -1 : 1;
}

/* one evaluation for tests and tools: x host [B][4][lh][lw] -> dx = dxdt(x, sigma) host, through the very unet_eval + dxdt_finish the denoising loop uses (plain
 * and tiled engines alike).  The latent of the engine is left alone. */
MLB_API int mlis_amd_dxdt(MLIS_AmdCtx* S, const float* x_host, float sigma, float* dx_host)
{
	if (!S || !x_host || !dx_host || !(sigma >= 0)) return fail("mlis_amd_dxdt: bad argument");
	if (!S->cond_set) return fail("mlis_amd_dxdt: conditioning not set");
	const size_t nb = (size_t)S->B * 4 * S->hw * 4;
	void *st = S->stream;
	for (int attempt=0; ; ++attempt) {
		S->i_eval = 0; S->last_nfe = 0; S->ctl_evals = 0; S->ctl_step_on = 1;
		if (mlsd_memset(S->d_nan, 0, 4, st) || mlsd_memcpy(S->d_tmp[0], x_host, nb, 0, st)) return -1;
		if (unet_eval(S, S->d_tmp[0], sigma, -1) < 0 || dxdt_finish(S, S->d_tmp[0], sigma, S->d_dx) < 0) return -1;
		int32_t nan_count = 0;
		if (mlsd_memcpy(dx_host, S->d_dx, nb, 1, st) || mlsd_memcpy(&nan_count, S->d_nan, 4, 1, st) || mlsd_stream_sync(st)) return -1;
		if (eval_handoff_check(S) < 0) {      /* as mlis_amd_denoise: once more on the hand-off-free plans */
			if (attempt) return -1;
			eval_handoffs_off(S); S->n_handoff_retries++;
			continue;
		}
		if (nan_count) return mlsd_set_error(-7 /* MLIS_E_NAN */, "NaN found in UNet output (%d values)", nan_count);
		return 1;
	}
}

static int denoise_body(MLIS_AmdCtx* S, const uint64_t* seeds, int* retry_wanted)
{
	if (!S->cond_set) return fail("mlis_amd_denoise: conditioning not set");
	const UnetParams *P = &S->unet_p;
	const int B = S->B, method = S->c.method;
	const int64_t nel = (int64_t)B * 4 * S->hw;
	void *st = S->stream;
	if (seeds) mlis_amd_seed(S, seeds);

	/* ---- dnsamp_init (src/sampling.c:28-96) */
	float sigmas[MAX_STEPS+1];
	int n_req = S->c.n_step;
	const int nfe_solver = solver_nfe(method);
	if (nfe_solver > 1) n_req = (n_req + nfe_solver - 1) / nfe_solver;        /* keep the NFE count (:47-49) */
	const int n_step = dnsamp_schedule(P, n_req, S->c.sched, S->c.f_t_ini, S->c.f_t_end, sigmas);
	if (n_step < 0 || n_step > S->c.n_step) return fail("schedule failed");
	float solver_t = sigmas[0];                                               /* :92 */
	unsigned i_step_solver = 0;
	float dt_prev = 0, h_last = 0;                                            /* taylor3 / dpmpp2m scalar state */
	S->n_draw_gen = 0; S->i_eval = 0; S->last_nfe = 0; S->last_n_step = n_step;
	S->k_draw = 0; S->ctl_evals = 0;
	if (mlsd_memset(S->d_nan, 0, 4, st)) return -1;
	if (!S->have_init_latent && mlsd_memset(S->d_x, 0, (size_t)nel*4, st)) return -1;   /* mlimgsynth.c:1669-1670 */
	if (method == SOLVER_METHOD_TAYLOR3 || method == SOLVER_METHOD_DPMPP2M) {
		/* solver tmp tensors start zeroed (ltensor_resize of an empty tensor; values unused until i_step >= 1) */
		if (mlsd_memset(S->d_tmp[0], 0, (size_t)nel*4, st) || mlsd_memset(S->d_tmp[1], 0, (size_t)nel*4, st)) return -1;
	}

	for (int s=0; s<n_step; ++s) {
		float s_up = 0, s_down = sigmas[s+1];
		S->ctl_step_on = mlis_amd_control_active(s, n_step, S->ctl_start, S->ctl_end);      /* both evaluations of a 2-NFE step share it */
		if (s == 0) {                                                         /* sampling.c:129-137 */
			if (S->have_lmask && mlsd_memcpy(S->d_x0, S->d_x, (size_t)nel*4, 2, st)) return -1;
			const float *nz = noise_draw(S, S->k_draw++);
			if (!nz || mlsd_noise_add_s(S->d_x, nz, sigmas[0], nel, st)) return -1;
			if (S->have_lmask && mlsd_mask_apply(S->d_x, S->d_x0, S->d_lmask, S->hw, nel, st)) return -1;
		}
		if (S->c.s_noise > 0 && s > 0) {                                      /* :139-151 */
			float s_curr = sigmas[s], s_hat = s_curr * sqrt(2) * S->c.s_noise, s_n = sqrt(s_hat*s_hat - s_curr*s_curr);
			const float *nz = noise_draw(S, S->k_draw++);
			if (!nz || mlsd_noise_add_s(S->d_x, nz, s_n, nel, st)) return -1;
			if (S->have_lmask && mlsd_mask_apply(S->d_x, S->d_x0, S->d_lmask, S->hw, nel, st)) return -1;
			solver_t = s_hat;
		}
		if (S->c.s_ancestral > 0) dnsamp_ancestral(sigmas[s], sigmas[s+1], S->c.s_ancestral, &s_down, &s_up);   /* :153-166 */
		const int anc_noise = (s_up > 0 && s+1 != n_step);
		/* draws to have ready by the end of this step's first evaluation: the ancestral one and the next step's s_noise one */
		int k_prefetch = S->k_draw - 1 + anc_noise + ((S->c.s_noise > 0 && s+1 < n_step) ? 1 : 0);
		/* ... and ONE STEP FURTHER: the draws of step s+1 are generated and submitted while evaluation s is being enqueued.  A draw submitted after an evaluation's
		 * uploads (weight streaming) sits behind them in the copy engine's queue -- behind the next evaluation's first segments, which wait for the end of this one:
		 * the noise arrived one upload (10 ms) after the evaluation that needed it (MLSD_ENGINE_TRACE: gaps in front of 4 of 20 evaluations).  Exactly the draws the
		 * schedule will consume: the generator state at the end of the call does not change. */
		if (s + 1 < n_step) {
			float sd2 = sigmas[s+2], su2 = 0;
			if (S->c.s_ancestral > 0) dnsamp_ancestral(sigmas[s+1], sigmas[s+2], S->c.s_ancestral, &sd2, &su2);
			k_prefetch += ((su2 > 0 && s+2 != n_step) ? 1 : 0) + ((S->c.s_noise > 0 && s+2 < n_step) ? 1 : 0);
		}

		/* ---- solver_step(&S->solver, s_down, x)  (src/solvers.c:43-52) */
		const float t0 = solver_t, t1 = s_down;
		if (!(t0 >= 0)) return fail("negative solver time");
		switch (method) {
		case SOLVER_METHOD_EULER: {                                           /* :82-88 */
			if (unet_eval(S, S->d_x, t0, k_prefetch) < 0) return -1;
			if (!P->vparam) {   /* fused: CFG mix, x += dx*dt and the ancestral noise of sampling.c:170-172 in one launch */
				int64_t ld = 0;
				const float *eps = eps_get(S, &ld), *factor;
				const float *nz = anc_noise ? noise_draw(S, S->k_draw) : NULL;
				float pag;
				if (anc_noise && !nz) return -1;
				if (guidance_args(S, eps, ld, &pag, &factor) < 0) return -1;
				if (mlsd_euler_guided_update(S->d_x, eps, ld, B, 4, S->hw, S->c.cfg_scale, pag, factor, t1 - t0, nz, s_up, st)) return -1;
				if (nz) { S->k_draw++; s_up = -1; }                               /* noise already added */
			} else {
				if (dxdt_finish(S, S->d_x, t0, S->d_dx) < 0) return -1;
				if (mlsd_vec_axpy(S->d_x, S->d_x, S->d_dx, t1 - t0, nel, st)) return -1;
			}
		} break;
		case SOLVER_METHOD_HEUN: {                                            /* :96-117 */
			const float dt = t1 - t0;
			float *x1 = S->d_tmp[0], *d1 = S->d_tmp[1];
			if (unet_eval(S, S->d_x, t0, k_prefetch) < 0 || dxdt_finish(S, S->d_x, t0, S->d_dx) < 0) return -1;
			if (mlsd_vec_axpy(x1, S->d_x, S->d_dx, dt, nel, st)) return -1;
			if (!(t1 > 0)) { if (mlsd_memcpy(S->d_x, x1, (size_t)nel*4, 2, st)) return -1; }
			else {
				if (unet_eval(S, x1, t1, -1) < 0 || dxdt_finish(S, x1, t1, d1) < 0) return -1;
				if (mlsd_solver_heun_corr(S->d_x, S->d_dx, d1, dt, nel, st)) return -1;
			}
		} break;
		case SOLVER_METHOD_TAYLOR3: {                                         /* :137-168 */
			const float dt = t1 - t0;
			if (unet_eval(S, S->d_x, t0, k_prefetch) < 0 || dxdt_finish(S, S->d_x, t0, S->d_dx) < 0) return -1;
			float idtp = i_step_solver >= 1 ? 1 / dt_prev : 0, f2 = i_step_solver >= 1 ? dt*dt/2 : 0,
			      f3 = i_step_solver >= 2 ? dt*dt*dt/6 : 0;
			if (mlsd_solver_taylor3(S->d_x, S->d_dx, S->d_tmp[0], S->d_tmp[1], dt, idtp, f2, f3, nel, st)) return -1;
			dt_prev = dt;
		} break;
		case SOLVER_METHOD_DPMPP2M: {                                         /* :207-233 */
			float a = t1 / t0, h = -log(a), c = h / (2*h_last);
			if (i_step_solver == 0 || !(t1 > 0)) c = 0;
			if (unet_eval(S, S->d_x, t0, k_prefetch) < 0 || dxdt_finish(S, S->d_x, t0, S->d_dx) < 0) return -1;
			if (mlsd_solver_dpmpp2m(S->d_x, S->d_dx, S->d_tmp[0], t0, a, c, nel, st)) return -1;
			h_last = h;
		} break;
		case SOLVER_METHOD_DPMPP2S: {                                         /* :264-289 */
			float *x1 = S->d_tmp[0], *dx1 = S->d_tmp[1];
			if (unet_eval(S, S->d_x, t0, k_prefetch) < 0 || dxdt_finish(S, S->d_x, t0, S->d_dx) < 0) return -1;
			if (!(t1 > 0)) { if (mlsd_vec_axpy(S->d_x, S->d_x, S->d_dx, t1 - t0, nel, st)) return -1; }
			else {
				float tm = sqrt(t1 * t0), dt1 = tm - t0, a = t1 / t0;
				if (mlsd_vec_axpy(x1, S->d_x, S->d_dx, dt1, nel, st)) return -1;
				if (unet_eval(S, x1, tm, -1) < 0 || dxdt_finish(S, x1, tm, dx1) < 0) return -1;
				if (mlsd_solver_dpmpp2s(S->d_x, x1, dx1, tm, a, nel, st)) return -1;
			}
		} break;
		default: return fail("invalid sampling method");
		}
		solver_t = t1; i_step_solver++;                                       /* solvers.c:49-50 */

		if (s_up > 0 && s+1 != n_step) {                                      /* sampling.c:170-174 */
			const float *nz = noise_draw(S, S->k_draw++);
			if (!nz || mlsd_noise_add_s(S->d_x, nz, s_up, nel, st)) return -1;
		}
		if (anc_noise) solver_t = sigmas[s+1];
		if (S->have_lmask && mlsd_mask_apply(S->d_x, S->d_x0, S->d_lmask, S->hw, nel, st)) return -1;   /* :176-178 */

		if (S->cb) {   /* mlis_callback (mlimgsynth.c:1741-1745): reports COMPLETED steps, a negative return aborts */
			if (mlsd_stream_sync(st)) return -1;
			int r = S->cb(S->cb_user, s + 1, n_step, S->last_nfe);
			if (r < 0) return r;
		}
	}
	int32_t nan_count = 0;
	if (mlsd_memcpy(&nan_count, S->d_nan, 4, 1, st) || mlsd_stream_sync(st)) return -1;
	S->ctl_step_on = 1;
	if (eval_handoff_check(S) < 0) {                                         /* an in-launch hand-off of the plan gave up waiting: results invalid (mlis_amd_denoise retries) */
		if (retry_wanted) *retry_wanted = 1;                                 /* out of band: a user callback may abort with any negative value, -8 included */
		return -1;
	}
	float tot = 0;
	for (int i=0; i<S->i_eval; ++i) { float ms = 0; mlsd_event_elapsed_ms(S->ev[i][0], S->ev[i][1], &ms); tot += ms; }
	{	/* diagnostics (MLSD_ENGINE_TRACE=1): per evaluation, its duration on the device and the gap to the next one */
		static int tr = -1;
		if (tr < 0) { const char *e = getenv("MLSD_ENGINE_TRACE"); tr = e && *e && *e != '0'; }
		if (tr) for (int i=0; i<S->i_eval; ++i) {
			float d = 0, g = 0, t0 = 0;
			mlsd_event_elapsed_ms(S->ev[0][0], S->ev[i][0], &t0); mlsd_event_elapsed_ms(S->ev[i][0], S->ev[i][1], &d);
			if (i + 1 < S->i_eval) mlsd_event_elapsed_ms(S->ev[i][1], S->ev[i+1][0], &g);
			fprintf(stderr, "[engine] evaluation %2d: starts at %8.2f ms, runs %7.2f ms, gap to the next %6.2f ms\n", i, t0, d, g);
		}
	}
	S->last_unet_ms = tot;
	S->unet.nfe += S->last_nfe;
	S->have_init_latent = 0;                /* f_t_ini / latent use flags are cleared after a generation (mlimgsynth.c:700-706) */
	if (nan_count) return mlsd_set_error(-7 /* MLIS_E_NAN */, "NaN found in UNet output (%d values)", nan_count);
	return 1;
}

/* denoise_body + the clean-up of a call that ends early (callback abort, error): the one-step-ahead prefetch has generated -- and advanced the Philox states past -- draws
 * the loop never consumed, and their uploads may still be pending while the next call rewrites h_noise.  The upload stream is drained and every image's
 * generator is rewound to the draws actually consumed, so a following call with seeds = NULL continues the stream where this one stopped. */
static int denoise_once(MLIS_AmdCtx* S, const uint64_t* seeds, int* retry_wanted)
{
	const int r = denoise_body(S, seeds, retry_wanted);
	if (r < 0) {
		if (S->up_stream) mlsd_stream_sync(S->up_stream);
		const int ahead = S->n_draw_gen - S->k_draw;
		if (ahead > 0) for (int b=0;b<S->B;++b) S->rng[b].offset -= (uint32_t)ahead;
		S->n_draw_gen = S->k_draw;
	}
	return r;
}

/* The denoising loop with ONE retry on the hand-off-free plan: a timed-out in-launch hand-off (stream-K slab, LayerNorm statistics: a partner block
 * was not resident -- CUs shared with another process, CU-masked stream) is detected when the results are read back; the loop is deterministic in (initial latent,
 * Philox states, conditioning), so those are kept and the whole loop runs again with plain tiles and separate LayerNorm launches.  Never by restarting the process. */
MLB_API int mlis_amd_denoise(MLIS_AmdCtx* S, const uint64_t* seeds)
{
	if (seeds) mlis_amd_seed(S, seeds);
	const int guard = eval_handoff_ops(S) > 0;
	const int had_init = S->have_init_latent;
	const size_t xbytes = (size_t)S->B * 4 * S->hw * 4;
	RngPhilox keep[MAX_BATCH];
	if (guard) {
		memcpy(keep, S->rng, sizeof(S->rng[0]) * (size_t)S->B);
		if (had_init) {
			if (!S->d_xsave && mlsd_malloc((void**)&S->d_xsave, xbytes)) return -1;
			if (mlsd_memcpy(S->d_xsave, S->d_x, xbytes, 2, S->stream)) return -1;
		}
	}
	int retry = 0;
	int r = denoise_once(S, NULL, &retry);
	if (!retry || !guard) return r;
	eval_handoffs_off(S);
	S->n_handoff_retries++;
	memcpy(S->rng, keep, sizeof(S->rng[0]) * (size_t)S->B);
	S->have_init_latent = had_init;
	if (had_init && mlsd_memcpy(S->d_x, S->d_xsave, xbytes, 2, S->stream)) return -1;
	retry = 0;
	return denoise_once(S, NULL, &retry);
}

/* ------------------------------------------------------------------ ControlNet
 * 1 iff step i_step of n_step lies in the window: start n_step <= i_step + 0.5 < end n_step (the step's midpoint; in double from the float arguments) */
MLB_API int mlis_amd_control_active(int i_step, int n_step, float start, float end)
{
	const double m = (double)i_step + 0.5;
	return (double)start * n_step <= m && m < (double)end * n_step;
}

MLB_API int mlis_amd_set_control(MLIS_AmdCtx* S, float strength, float start, float end)
{
	if (!S || !S->ctl_ctx) return fail("mlis_amd_set_control: the engine was created without a ControlNet");
	if (!(strength >= 0 && strength <= 2)) return mlsd_set_error(-1, "control strength %g: 0 .. 2", strength);
	if (!(start >= 0 && start <= end && end <= 1)) return mlsd_set_error(-1, "control window %g .. %g: 0 <= start <= end <= 1", start, end);
	S->ctl_strength = strength; S->ctl_start = start; S->ctl_end = end;
	return 1;
}

/* the control image -> the hint embedding (once per image), and for a plain engine a copy of it per plan image (a tiled engine cuts windows out per evaluation).
 * kind: 0 host, 2 device pointer. */
static int set_control_image(MLIS_AmdCtx* S, const float* hint, int kind)
{
	if (!S || !S->ctl_ctx) return fail("mlis_amd_set_control_image: the engine was created without a ControlNet");
	S->ctl_tag = 0;
	if (!hint) { S->ctl_image = 0; return 1; }
	void *st = S->stream;
	S->ctl_image = 0;
	if (mlsd_memcpy(mlctx_input_device_ptr(S->t_hint_img), hint, (size_t)3 * S->c.width * S->c.height * 4, kind, st)) return -1;
	if (mlctx_compute_checked(S->hint_ctx) < 0) return -1;
	if (!S->n_win) {
		const float *hs = mlctx_tensor_device_f32(S->hint_ctx, mlctx_result(S->hint_ctx), NULL);
		float *hw_ = (float*)mlctx_tensor_device_f32(S->ctl_ctx, S->ctl.t_hint, NULL);
		const int zero = 0;
		if (mlsd_window_gather_nhwc(hs, S->lw, S->lh, S->unet_p.n_ch, hw_, S->lw, S->lh, &zero, &zero, 1, S->CN, st)) return -1;
	}
	if (mlsd_stream_sync(st)) return -1;
	S->ctl_image = 1;
	return 1;
}
MLB_API int mlis_amd_set_control_image(MLIS_AmdCtx* S, const float* hint) { return set_control_image(S, hint, 0); }
MLB_API int mlis_amd_set_control_image_device(MLIS_AmdCtx* S, const void* hint_dev) { return set_control_image(S, (const float*)hint_dev, 2); }

/* a caller's mark on the control image the engine holds (0 after every mlis_amd_set_control_image*): lets it skip setting the same image again */
MLB_API void mlis_amd_control_tag_set(MLIS_AmdCtx* S, uint64_t tag) { if (S && S->ctl_image) S->ctl_tag = tag; }
MLB_API uint64_t mlis_amd_control_tag(const MLIS_AmdCtx* S) { return S && S->ctl_image ? S->ctl_tag : 0; }
/* the control image as the hint plan reads it: device, NCHW fp32 [3][height][width]; NULL without a ControlNet or an image (tests) */
MLB_API const void* mlis_amd_control_image_device(MLIS_AmdCtx* S) { return S && S->ctl_ctx && S->ctl_image ? S->t_hint_img->in_stage : NULL; }
/* ... and copied to the host: what a pass was really conditioned on */
MLB_API int mlis_amd_control_image_get(const MLIS_AmdCtx* S, float* host_dst, int* w, int* h)
{
	if (!S || !S->ctl_ctx || !S->ctl_image) return 0;
	if (w) *w = S->c.width;
	if (h) *h = S->c.height;
	if (host_dst && (mlsd_memcpy(host_dst, S->t_hint_img->in_stage, (size_t)3 * S->c.width * S->c.height * 4, 1, S->stream) || mlsd_stream_sync(S->stream))) return -1;
	return 1;
}

MLB_API int mlis_amd_control_info(const MLIS_AmdCtx* S, int* n_residuals, int* evals_controlled)
{
	if (!S) return -1;
	if (n_residuals) *n_residuals = S->ctl_ctx ? S->ctl.n_res : 0;
	if (evals_controlled) *evals_controlled = S->ctl_evals;
	return 1;
}

/* ------------------------------------------------------------------ HyperTile: what the rule did to the UNet plan (the plan was built with it: nothing to set) */
MLB_API int mlis_amd_hypertile_info(const MLIS_AmdCtx* S, int* n_tiled, int* n_untiled, int tiles[4][4])
{
	if (!S || !S->unet_ctx) return fail("mlis_amd_hypertile_info: no engine");
	return mlctx_hypertile_info(S->unet_ctx, n_tiled, n_untiled, tiles);
}

/* ------------------------------------------------------------------ FreeU
 * the factors of the next evaluations: four floats in device memory that the UNet plan's FreeU passes read when they run (a factor of exactly 1 makes its
 * passes copies).  Nothing is rebuilt or captured again; tiled and packed engines need nothing more, every window plan evaluation runs the same passes. */
MLB_API int mlis_amd_set_freeu(MLIS_AmdCtx* S, float b1, float b2, float s1, float s2)
{
	if (!S || !S->d_freeu) return fail("mlis_amd_set_freeu: the engine was created without FreeU");
	const float f[4] = { b1, b2, s1, s2 };
	for (int i=0;i<4;++i) if (!(f[i] >= 0 && f[i] <= 4)) return mlsd_set_error(-1, "FreeU factor %g: 0 .. 4", f[i]);
	if (mlsd_stream_sync(S->stream)) return -1;      /* (the source of the copy is engine memory: nothing in flight reads the old values afterwards) */
	memcpy(S->freeu_f, f, sizeof(f));
	if (mlsd_memcpy(S->d_freeu, S->freeu_f, sizeof(f), 0, S->stream) || mlsd_stream_sync(S->stream)) return -1;
	return 1;
}

MLB_API int mlis_amd_freeu_info(const MLIS_AmdCtx* S, int* n_stage1, int* n_stage2)
{
	if (!S) return -1;
	if (n_stage1) *n_stage1 = S->d_freeu ? S->fu.n_stage1 : 0;
	if (n_stage2) *n_stage2 = S->d_freeu ? S->fu.n_stage2 : 0;
	return 1;
}

/* ------------------------------------------------------------------ perturbed-attention guidance
 * the scale of the next evaluations: a field of the engine that dxdt_finish and the fused Euler step hand to their kernels by value.  Nothing is rebuilt or captured
 * again (the mix is not part of the captured evaluation).  Tiled and packed engines need nothing more: the mix is affine in eps, so blending raw outputs stays exact. */
MLB_API int mlis_amd_set_pag(MLIS_AmdCtx* S, float scale)
{
	if (!S || !S->pag) return fail("mlis_amd_set_pag: the engine was created without PAG");
	if (!(scale >= 0 && scale <= 20)) return mlsd_set_error(-1, "PAG scale %g: 0 .. 20", scale);
	S->pag_scale = scale;
	return 1;
}

MLB_API int mlis_amd_pag_info(const MLIS_AmdCtx* S, int* n_attn, int* rows)
{	/* the perturbed self-attentions of the UNet plan (0 without the flag) and the rows of one evaluation */
	if (!S) return -1;
	int n = 0;
	if (S->pag && S->unet_ctx) mlctx_pag_info(S->unet_ctx, &n, NULL);
	if (n_attn) *n_attn = n;
	if (rows) *rows = S->N;
	return 1;
}

/* ------------------------------------------------------------------ prediction type, sigma table, guidance rescale
 * Fields of the engine that the schedule, sigma <-> t and the mix read: set per generation, nothing is rebuilt or captured again (the mix is outside the captured
 * evaluation, the schedule is host arithmetic).  vparam / zsnr: 0 or 1, negative: what the model type says (zsnr: off). */
MLB_API int mlis_amd_set_prediction(MLIS_AmdCtx* S, int vparam, int zsnr)
{
	if (!S) return fail("mlis_amd_set_prediction: no engine");
	if (vparam > 1 || zsnr > 1) return mlsd_set_error(-1, "mlis_amd_set_prediction: vparam %d, zsnr %d (0, 1 or negative for the model type's)", vparam, zsnr);
	S->unet_p.vparam = vparam < 0 ? S->vparam_model : vparam;
	unet_params_set_zsnr(&S->unet_p, zsnr > 0);
	return 1;
}

/* the raw outputs the last mix read (the plan's result, or the blended canvas of a tiled engine): host [N][4][hw], N = mlis_amd_eval_rows.  For tests and tools. */
MLB_API int mlis_amd_last_rows(MLIS_AmdCtx* S, float* out, size_t nbytes)
{
	if (!S || !out || nbytes != (size_t)S->N * 4 * S->hw * 4) return fail("mlis_amd_last_rows: bad argument");
	int64_t ld = 0;
	const float *eps = eps_get(S, &ld);
	const size_t rows = (size_t)S->N * S->hw;
	float *tmp = (float*)malloc(rows * ld * 4);
	if (!tmp) return fail("out of memory");
	if (mlsd_memcpy(tmp, eps, rows * ld * 4, 1, S->stream) || mlsd_stream_sync(S->stream)) { free(tmp); return -1; }
	for (int n=0; n<S->N; ++n) for (int p=0; p<S->hw; ++p) for (int c=0; c<4; ++c)
		out[((size_t)n*4 + c)*S->hw + p] = tmp[((size_t)n*S->hw + p)*ld + c];
	free(tmp);
	return 1;
}

MLB_API int mlis_amd_prediction_resolve(const char* model, int ckpt_v_pred, int ckpt_ztsnr, int opt_prediction, int opt_zsnr, int* vparam, int* zsnr)
{
	UnetParams U;
	if (!model || unet_params_get(model, &U) < 0) return -1;
	if (opt_prediction < 0 || opt_prediction > 2 || opt_zsnr < 0 || opt_zsnr > 2) return mlsd_set_error(-1, "prediction %d / zsnr %d: 0 .. 2", opt_prediction, opt_zsnr);
	if (vparam) *vparam = opt_prediction ? opt_prediction == 2 : (U.vparam || ckpt_v_pred);
	if (zsnr) *zsnr = opt_zsnr ? opt_zsnr == 2 : ckpt_ztsnr != 0;
	return 1;
}

MLB_API int mlis_amd_set_cfg_rescale(MLIS_AmdCtx* S, float phi)
{
	if (!S) return fail("mlis_amd_set_cfg_rescale: no engine");
	if (!(phi >= 0 && phi <= 1)) return mlsd_set_error(-1, "guidance rescale %g: 0 .. 1", phi);
	if (phi > 0 && !S->d_gr_part) {
		const size_t nb = mlsd_guidance_scratch_bytes(S->B, S->hw);
		if (mlsd_malloc((void**)&S->d_gr_part, nb) || mlsd_malloc((void**)&S->d_gr_factor, (size_t)S->B * 4)) return -1;
		S->gr_part_bytes = nb;
	}
	S->cfg_rescale = phi;
	return 1;
}

/* the resolved prediction type and table, the sigma range the schedule walks, phi, the rescaled mixes so far, and the factors of the last one (at most max_factors of
 * the B; the stream is synchronised for them).  Returns the number of factors written: 0 before the first rescaled mix. */
MLB_API int mlis_amd_guidance_info(MLIS_AmdCtx* S, int* vparam, int* zsnr, float* sigma_min, float* sigma_max, float* phi, int* n_evals, float* factors, int max_factors)
{
	if (!S) return -1;
	if (vparam) *vparam = S->unet_p.vparam;
	if (zsnr) *zsnr = S->unet_p.zsnr;
	if (sigma_min) *sigma_min = S->unet_p.sigma_min;
	if (sigma_max) *sigma_max = S->unet_p.sigma_max;
	if (phi) *phi = S->cfg_rescale;
	if (n_evals) *n_evals = S->gr_evals;
	if (!factors || max_factors < 1 || !S->gr_evals || !S->d_gr_factor) return 0;
	const int n = max_factors < S->B ? max_factors : S->B;
	if (mlsd_memcpy(factors, S->d_gr_factor, (size_t)n * 4, 1, S->stream) || mlsd_stream_sync(S->stream)) return -1;
	return n;
}

/* ------------------------------------------------------------------ VAE tiling
 * sdvae_decode / sdvae_encode with tile_px > 0 (src/vae.c:333-391, 245-300): the latent (image) is cut into overlapping
 * tiles of tile_px (+ a margin of k = 8 latent pixels / 64 image pixels on every side), each tile runs through a tile-sized
 * plan, and the interior of its result is pasted into the output in the reference's order (later tiles overwrite the
 * margins of earlier ones).  TAE codecs are never tiled (the reference only tiles sdvae_*).
 *
 * A deliberate extension of the reference: where one tile covers a dimension (n == full) while the other dimension is tiled,
 * the reference's loop (vae.c:262-291, 353-385) gives every tile of that dimension the origin 0 and pastes only n - k of it, so
 * the last margin of the output is never written (there: whatever realloc returned); at exactly 2k it divides by zero and below
 * 2k it runs no tile at all.  Here such a dimension is ONE tile at origin 0 pasted whole: the same tile at the same origin as the
 * reference's, so every pixel the reference writes has the same bits, and the pixels it leaves undefined are defined.  Where a
 * dimension is tiled (n < full) the rule is the reference's, without the tiles it repeats: ceil(full / step) counts tiles whose
 * origins all clamp to full - n; they paste the same values onto the same pixels again, so dropping them changes no bit. */
MLB_API int mlis_amd_set_vae_tile(MLIS_AmdCtx* S, int tile_px)
{
	if (tile_px < 0) tile_px = 0;
	if (tile_px != S->vae_tile) {
		mlsd_stream_sync(S->stream);
		if (S->dect_ctx) { mlctx_destroy(S->dect_ctx); S->dect_ctx = NULL; }
		if (S->enct_ctx) { mlctx_destroy(S->enct_ctx); S->enct_ctx = NULL; }
		/* the tile buffers have the size of one tile: the next *_tile_prepare allocates them for the new one */
		mlsd_free(S->d_lat_tile); mlsd_free(S->d_img_tile); mlsd_free(S->d_imgin_tile); mlsd_free(S->d_mom_tile);
		S->d_lat_tile = S->d_img_tile = S->d_imgin_tile = S->d_mom_tile = NULL;
		memset(S->tile_bytes, 0, sizeof(S->tile_bytes));
		S->tl_w = S->tl_h = S->ti_w = S->ti_h = 0;
		S->vae_tile = tile_px;
	}
	return 1;
}

static int tile_dims(int tile_px, int margin2, int full, int unit)
{	/* n = min(round_up(tile_px, 64)/unit + 2k, full); returns full when one tile covers everything (tiling disabled) */
	const int t = (tile_px + 63) / 64 * 64;
	const int n = t / unit + margin2;
	return n < full ? n : full;
}

/* The tile walk of ONE dimension, for decode and encode alike.  Lengths are in units of `unit` image pixels (decode: f, the walk
 * is over latent pixels; encode: 1): `full` the dimension, `margin` the overlap k (decode 8, encode 8 f), tile_px the option.
 * *n_out = the tile length min(round_up(tile_px, 64) / unit + 2k, full).  Tile t reads [origin[t], origin[t] + n) of the input and
 * pastes [src_off[t], src_off[t] + width[t]) of its result at origin[t] + src_off[t] of the output:
 *   n < full   tile 0 pastes [0, n - k); tile t > 0 at i0 = min(t step, full - n), step = n - 2k, pastes [i0 + k, i0 + n); the
 *              walk ends with the first tile at full - n (vae.c:269-289, 365-384 without the repeats of that last origin)
 *   n == full  one tile at 0 pasted whole (see above)
 * Returns the number of tiles (at most max_tiles of them are written; the arrays may be NULL with max_tiles 0), < 0 for arguments
 * no walk exists for. */
MLB_API int mlis_amd_vae_tile_walk(int full, int tile_px, int unit, int margin, int* n_out, int* origin, int* src_off, int* width, int max_tiles)
{
	if (full < 1 || tile_px < 1 || tile_px > 65535 || unit < 1 || margin < 0 || margin > 65535) return -1;
	const int k = margin, n = tile_dims(tile_px, 2*k, full, unit);
	if (n_out) *n_out = n;
	if (n == full) {
		if (max_tiles > 0) { origin[0] = 0; src_off[0] = 0; width[0] = full; }
		return 1;
	}
	const int step = n - 2*k, last = full - n;
	if (step < 1) return -1;                    /* unit > round_up(tile_px, 64) */
	int cnt = 0;
	for (int i0 = 0; ; i0 = i0 + step < last ? i0 + step : last) {
		if (cnt < max_tiles) { origin[cnt] = i0; src_off[cnt] = i0 ? k : 0; width[cnt] = n - k; }
		++cnt;
		if (i0 == last) break;
	}
	return cnt;
}

typedef struct { int n, cnt, *org, *off, *wid; } TileWalk;

static int tile_walk_new(TileWalk* w, int full, int tile_px, int unit, int margin)
{
	w->org = NULL;
	w->cnt = mlis_amd_vae_tile_walk(full, tile_px, unit, margin, &w->n, NULL, NULL, NULL, 0);
	if (w->cnt < 1) return mlsd_set_error(-1, "VAE tiling: no tile walk for length %d, tile %d", full, tile_px);
	w->org = (int*)malloc((size_t)3 * w->cnt * sizeof(int));
	if (!w->org) return mlsd_set_error(-1, "out of host memory");
	w->off = w->org + w->cnt; w->wid = w->off + w->cnt;
	mlis_amd_vae_tile_walk(full, tile_px, unit, margin, &w->n, w->org, w->off, w->wid, w->cnt);
	return 0;
}

/* (re)allocates one tile buffer when the tile needs more than it holds */
static int tile_buf(MLIS_AmdCtx* S, float** p, int which, size_t nbytes)
{
	if (*p && S->tile_bytes[which] >= nbytes) return 0;
	mlsd_free(*p); *p = NULL; S->tile_bytes[which] = 0;
	if (mlsd_malloc((void**)p, nbytes)) return -1;
	S->tile_bytes[which] = nbytes;
	return 0;
}

/* builds (once) the decode tile plan; returns NULL with no error when tiling does not apply.
 * The tile plans take ONE image: a batch walks them image by image (the tile buffers hold the tile of every image, the plan's input moves from one to the next).
 * A tile of image b is then computed by the same launches whatever the batch size -- GEMM tiles and K splits are chosen by M = images x pixels, so a plan of
 * B images would round differently from the plan of one -- and the plan's activations, what tiling is there to bound, do not grow with the batch. */
MLB_API MLCtx* mlis_amd_decoder_tile_prepare(MLIS_AmdCtx* S)
{
	if (S->dect_ctx) return S->dect_ctx;
	if (S->vae_tile <= 0 || S->c.use_tae) return NULL;
	const int f = S->vae_p.f_down, k = 8;
	const int n0 = tile_dims(S->vae_tile, 2*k, S->lw, f), n1 = tile_dims(S->vae_tile, 2*k, S->lh, f);
	if (n0 == S->lw && n1 == S->lh) return NULL;                                      /* one tile: disabled (vae.c:347-348) */
	const int B = S->B;
	if (tile_buf(S, &S->d_lat_tile, 0, (size_t)B*4*n0*n1*4)) return NULL;
	if (tile_buf(S, &S->d_img_tile, 1, (size_t)B*3*n0*f*n1*f*4)) return NULL;
	MLCtx *C = mlctx_new(S->stream);
	int ok = sdvae_decode_init(C, &S->vae_p, n0, n1, 1, &S->t_lat_dect) >= 0 &&
	         mlctx_input_bind(S->t_lat_dect, S->d_lat_tile, 1, NULL, 1 / S->vae_p.scale_factor, 0) >= 0 &&
	         sdvae_decode_build(C, &S->vae_p, S->t_lat_dect) >= 0;
	if (ok && !S->c.defer_weights) ok = mlctx_params_synth(C, S->c.weight_seed) >= 0;
	if (!ok) { mlctx_destroy(C); return NULL; }
	S->dect_ctx = C; S->tl_w = n0; S->tl_h = n1;
	return C;
}

MLB_API MLCtx* mlis_amd_encoder_tile_prepare(MLIS_AmdCtx* S)
{
	if (S->enct_ctx) return S->enct_ctx;
	if (S->vae_tile <= 0 || S->c.use_tae) return NULL;
	const int f = S->vae_p.f_down, k = f*8, W = S->c.width, H = S->c.height;
	const int n0 = tile_dims(S->vae_tile, 2*k, W, 1), n1 = tile_dims(S->vae_tile, 2*k, H, 1);
	if (n0 == W && n1 == H) return NULL;
	const int B = S->B;
	if (!S->d_img_in && mlsd_malloc((void**)&S->d_img_in, (size_t)B*3*W*H*4)) return NULL;
	if (tile_buf(S, &S->d_imgin_tile, 2, (size_t)B*3*n0*n1*4)) return NULL;
	if (tile_buf(S, &S->d_mom_tile, 3, (size_t)B*8*(n0/f)*(n1/f)*4)) return NULL;
	if (!S->d_mom && mlsd_malloc((void**)&S->d_mom, (size_t)B*8*S->hw*4)) return NULL;
	MLCtx *C = mlctx_new(S->stream);
	int ok = sdvae_encode_init(C, &S->vae_p, n0, n1, 1, &S->t_img_enct) >= 0 &&
	         mlctx_input_bind(S->t_img_enct, S->d_imgin_tile, 1, NULL, 1.0f, 2) >= 0 &&
	         sdvae_encode_build(C, &S->vae_p, S->t_img_enct) >= 0;
	if (ok && !S->c.defer_weights) ok = mlctx_params_synth(C, S->c.weight_seed) >= 0;
	if (!ok) { mlctx_destroy(C); return NULL; }
	S->enct_ctx = C; S->ti_w = n0; S->ti_h = n1;
	return C;
}

static int decode_tiled(MLIS_AmdCtx* S)
{	/* src/vae.c:351-383, walked by mlis_amd_vae_tile_walk */
	const int f = S->vae_p.f_down, k = 8, B = S->B;
	const int lat_n0 = S->lw, lat_n1 = S->lh, n0 = S->tl_w, n1 = S->tl_h;
	const int img_n0 = lat_n0*f, img_n1 = lat_n1*f;
	void *st = S->stream;
	MLTensor *r = mlctx_result(S->dect_ctx);
	int64_t ld = 0;
	const float *y = mlctx_tensor_device_f32(S->dect_ctx, r, &ld);
	TileWalk w0, w1 = {0};
	int R = -1;
	S->n_tile_evals[0] = 0;
	if (tile_walk_new(&w0, lat_n0, S->vae_tile, f, k) || tile_walk_new(&w1, lat_n1, S->vae_tile, f, k)) goto end;
	if (w0.n != n0 || w1.n != n1) { mlsd_set_error(-1, "VAE tiling: the decode tile plan is %dx%d, the walk's tile %dx%d", n0, n1, w0.n, w1.n); goto end; }
	for (int t1=0; t1<w1.cnt; ++t1) {
		const int i1 = w1.org[t1], d1 = w1.off[t1];
		for (int t0=0; t0<w0.cnt; ++t0) {
			const int i0 = w0.org[t0], d0 = w0.off[t0];
			if (mlsd_copy_slice2(S->d_lat_tile, n0, n1, S->d_x, lat_n0, lat_n1, n0, n1, 0, 0, i0, i1, B*4, st)) goto end;
			for (int b=0; b<B; ++b) {
				if (mlctx_input_rebind(S->dect_ctx, S->t_lat_dect, S->d_lat_tile + (size_t)b*4*n0*n1) < 0) goto end;
				if (mlctx_compute(S->dect_ctx) < 0) goto end;
				S->n_tile_evals[0]++;
				if (mlsd_nhwc_to_nchw_f32(y, ld, 1, 3, n0*f*n1*f, S->d_img_tile + (size_t)b*3*n0*f*n1*f, 0.5f, 0.5f, st)) goto end;   /* (x+1)/2: elementwise, commutes with the paste */
			}
			if (mlsd_copy_slice2(S->d_img, img_n0, img_n1, S->d_img_tile, n0*f, n1*f, w0.wid[t0]*f, w1.wid[t1]*f, (i0+d0)*f, (i1+d1)*f,
					d0*f, d1*f, B*3, st)) goto end;
		}
	}
	R = 1;
end:
	free(w0.org); free(w1.org);
	return R;
}

static int encode_tiled(MLIS_AmdCtx* S)
{	/* src/vae.c:262-299: tiles of the image -> moments tiles -> pasted into the full moments tensor (NCHW [B][8][lh][lw]) */
	const int f = S->vae_p.f_down, k = f*8, B = S->B;
	const int img_n0 = S->c.width, img_n1 = S->c.height, n0 = S->ti_w, n1 = S->ti_h;
	const int lat_n0 = img_n0/f, lat_n1 = img_n1/f;
	void *st = S->stream;
	MLTensor *r = mlctx_result(S->enct_ctx);
	int64_t ld = 0;
	const float *y = mlctx_tensor_device_f32(S->enct_ctx, r, &ld);
	TileWalk w0, w1 = {0};
	int R = -1;
	S->n_tile_evals[1] = 0;
	if (tile_walk_new(&w0, img_n0, S->vae_tile, 1, k) || tile_walk_new(&w1, img_n1, S->vae_tile, 1, k)) goto end;
	if (w0.n != n0 || w1.n != n1) { mlsd_set_error(-1, "VAE tiling: the encode tile plan is %dx%d, the walk's tile %dx%d", n0, n1, w0.n, w1.n); goto end; }
	for (int t1=0; t1<w1.cnt; ++t1) {
		const int i1 = w1.org[t1], d1 = w1.off[t1];
		for (int t0=0; t0<w0.cnt; ++t0) {
			const int i0 = w0.org[t0], d0 = w0.off[t0];
			if (mlsd_copy_slice2(S->d_imgin_tile, n0, n1, S->d_img_in, img_n0, img_n1, n0, n1, 0, 0, i0, i1, B*3, st)) goto end;
			for (int b=0; b<B; ++b) {
				if (mlctx_input_rebind(S->enct_ctx, S->t_img_enct, S->d_imgin_tile + (size_t)b*3*n0*n1) < 0) goto end;
				if (mlctx_compute(S->enct_ctx) < 0) goto end;
				S->n_tile_evals[1]++;
				if (mlsd_count_nonfinite(y, (size_t)(n0/f)*(n1/f)*ld, S->d_nan, st)) goto end;
				if (mlsd_nhwc_to_nchw_f32(y, ld, 1, 8, (n0/f)*(n1/f), S->d_mom_tile + (size_t)b*8*(n0/f)*(n1/f), 1.0f, 0.0f, st)) goto end;
			}
			if (mlsd_copy_slice2(S->d_mom, lat_n0, lat_n1, S->d_mom_tile, n0/f, n1/f, w0.wid[t0]/f, w1.wid[t1]/f, (i0+d0)/f, (i1+d1)/f,
					d0/f, d1/f, B*8, st)) goto end;
		}
	}
	R = 1;
end:
	free(w0.org); free(w1.org);
	return R;
}

/* the tile plan of the decoder (which 0) or the encoder (which 1) as it stands: the tile size (latent / image pixels; 0 x 0 without a plan), the bytes allocated for
 * the tile's input and output buffers (the tile of every image of the batch), the tiles one pass walks and the plan evaluations of the last tiled pass (tiles x images).  Returns 1 with a plan, 0 without. */
MLB_API int mlis_amd_vae_tile_info(MLIS_AmdCtx* S, int which, int* tile_w, int* tile_h, size_t* in_bytes, size_t* out_bytes, int* n_tiles, int* n_evals)
{
	if (!S || which < 0 || which > 1) return -1;
	MLCtx *C = which ? S->enct_ctx : S->dect_ctx;
	const int f = S->vae_p.f_down;
	int n = 0;
	if (C) {
		const int c0 = mlis_amd_vae_tile_walk(which ? S->c.width : S->lw, S->vae_tile, which ? 1 : f, which ? 8*f : 8, NULL, NULL, NULL, NULL, 0);
		const int c1 = mlis_amd_vae_tile_walk(which ? S->c.height : S->lh, S->vae_tile, which ? 1 : f, which ? 8*f : 8, NULL, NULL, NULL, NULL, 0);
		n = c0 > 0 && c1 > 0 ? c0 * c1 : -1;
	}
	if (tile_w) *tile_w = C ? (which ? S->ti_w : S->tl_w) : 0;
	if (tile_h) *tile_h = C ? (which ? S->ti_h : S->tl_h) : 0;
	if (in_bytes) *in_bytes = S->tile_bytes[which ? 2 : 0];
	if (out_bytes) *out_bytes = S->tile_bytes[which ? 3 : 1];
	if (n_tiles) *n_tiles = n;
	if (n_evals) *n_evals = S->n_tile_evals[which];
	return C ? 1 : 0;
}

/* after the launches of a decode / encode were enqueued: if the plan hands data over inside launches, drain and check; 1 = clean, 0 = gave up -> the plan is now
 * hand-off-free and the caller runs its launches again, < 0 = error */
static int handoffs_clean(MLIS_AmdCtx* S, MLCtx* C, int attempt)
{
	if (!mlctx_handoff_ops(C) && !attempt) return 1;
	if (mlsd_stream_sync(S->stream)) return -1;
	if (mlctx_handoff_check(C) == 0) return 1;
	if (attempt) return -1;
	mlctx_handoffs_off(C);
	S->n_handoff_retries++;
	return 0;
}

MLB_API int mlis_amd_decode(MLIS_AmdCtx* S)
{
	if (S->vae_tile > 0 && !S->c.use_tae && mlis_amd_decoder_tile_prepare(S)) {
		for (int attempt=0; attempt<2; ++attempt) {
			if (decode_tiled(S) < 0) return -1;
			const int ok = handoffs_clean(S, S->dect_ctx, attempt);
			if (ok) return ok;
		}
		return -1;
	}
	for (int attempt=0; ; ++attempt) {
		if (mlctx_compute(S->dec_ctx) < 0) return -1;
		const int ok = handoffs_clean(S, S->dec_ctx, attempt);
		if (ok < 0) return -1;
		if (ok) break;
	}
	int64_t ld = 0;
	MLTensor *r = mlctx_result(S->dec_ctx);
	const float *y = mlctx_tensor_device_f32(S->dec_ctx, r, &ld);
	const int HW = S->c.width * S->c.height;
	/* sdvae_decoder_post (x+1)/2 (vae.h:43-47); TAE output is used as-is */
	const float mul = S->c.use_tae ? 1.0f : 0.5f, add = S->c.use_tae ? 0.0f : 0.5f;
	if (mlsd_nhwc_to_nchw_f32(y, ld, S->B, 3, HW, S->d_img, mul, add, S->stream)) return -1;
	return 1;
}

/* builds the encoder plan (once) without running it; with defer_weights the caller loads its parameters before the first encode */
MLB_API MLCtx* mlis_amd_encoder_prepare(MLIS_AmdCtx* S)
{
	if (S->enc_ctx) return S->enc_ctx;
	const int B = S->B, W = S->c.width, H = S->c.height;
	void *st = S->stream;
	if (!S->d_img_in && mlsd_malloc((void**)&S->d_img_in, (size_t)B*3*W*H*4)) return NULL;
	MLCtx *C = mlctx_new(st);
	mlctx_set_conv_wrap(C, S->tiling);
	int ok = 0;
	if (S->c.use_tae) {
		ok = sdtae_encode_init(C, W, H, B, &S->t_img_enc) >= 0 && mlctx_input_bind(S->t_img_enc, S->d_img_in, B, NULL, 1.0f, 0) >= 0 &&
		     sdtae_encode_build(C, S->t_img_enc) >= 0;
	} else {
		ok = sdvae_encode_init(C, &S->vae_p, W, H, B, &S->t_img_enc) >= 0 &&
		     mlctx_input_bind(S->t_img_enc, S->d_img_in, B, NULL, 1.0f, 2) >= 0 &&       /* mode 2: x*2-1 (vae.h:36-40) */
		     sdvae_encode_build(C, &S->vae_p, S->t_img_enc) >= 0;
	}
	if (ok && !S->c.defer_weights) ok = mlctx_params_synth(C, S->c.weight_seed) >= 0;
	if (!ok) { mlctx_destroy(C); return NULL; }
	S->enc_ctx = C;
	return C;
}

/* mlis_image_encode (src/mlimgsynth.c:1301-1330): images host NCHW [B][3][H][W] in [0,1] -> the resident latent becomes
 * the sampled (VAE: mean + std*N(0,1), one Philox call per image, src/vae.c:203-229) or direct (TAE) encoding and is
 * marked as the initial latent of the next denoise.  The encoder plan is built on first use. */
MLB_API int mlis_amd_encode(MLIS_AmdCtx* S, const float* images, int sample)
{
	const int B = S->B, W = S->c.width, H = S->c.height;
	const size_t img_elems = (size_t)B*3*W*H;
	void *st = S->stream;
	const int tiled = S->vae_tile > 0 && !S->c.use_tae && mlis_amd_encoder_tile_prepare(S) != NULL;
	if (!tiled && !S->enc_ctx && !mlis_amd_encoder_prepare(S)) return -1;
	if (mlsd_memcpy(S->d_img_in, images, img_elems*4, 0, st)) return -1;
	if (mlsd_memset(S->d_nan, 0, 4, st)) return -1;
	const float *y; int64_t ld = 0;
	for (int attempt=0; ; ++attempt) {            /* (second pass only after a timed-out in-launch hand-off: the plan is hand-off-free then) */
		if (attempt && mlsd_memset(S->d_nan, 0, 4, st)) return -1;
		if (tiled) {
			if (encode_tiled(S) < 0) return -1;
			y = NULL;
		} else {
			if (mlctx_compute(S->enc_ctx) < 0) return -1;
			y = mlctx_tensor_device_f32(S->enc_ctx, mlctx_result(S->enc_ctx), &ld);
			if (mlsd_count_nonfinite(y, (size_t)B*S->hw*ld, S->d_nan, st)) return -1;
		}
		const int ok = handoffs_clean(S, tiled ? S->enct_ctx : S->enc_ctx, attempt);
		if (ok < 0) return -1;
		if (ok) break;
	}
	if (S->c.use_tae) {
		if (mlsd_nhwc_to_nchw_f32(y, ld, B, 4, S->hw, S->d_x, 1.0f, 0.0f, st)) return -1;
	} else {
		const float *rnd = NULL;
		if (sample) {   /* sdvae_latent_sample: rng_randn(n) per image, before any denoising draw */
			S->n_draw_gen = 0;
			rnd = noise_draw(S, 0);
			if (!rnd) return -1;
		}
		if (tiled) { if (mlsd_latent_sample_nchw(S->d_mom, rnd, S->d_x, B, S->vae_p.ch_z, S->hw, S->vae_p.scale_factor, st)) return -1; }
		else if (mlsd_latent_sample(y, ld, rnd, S->d_x, B, S->vae_p.ch_z, S->hw, S->vae_p.scale_factor, st)) return -1;
	}
	int32_t nan_count = 0;
	if (mlsd_memcpy(&nan_count, S->d_nan, 4, 1, st) || mlsd_stream_sync(st)) return -1;
	if (nan_count) return mlsd_set_error(-7, "NaN found in encoded latent");   /* mlimgsynth.c:1323 */
	S->have_init_latent = 1;
	return 1;
}

MLB_API int mlis_amd_generate(MLIS_AmdCtx* S, const uint64_t* seeds, float* latents_out, float* images_out)
{
	int r = mlis_amd_denoise(S, seeds);
	if (r < 0) return r;
	if (latents_out && mlsd_memcpy(latents_out, S->d_x, (size_t)S->B*4*S->hw*4, 1, S->stream)) return -1;
	if (mlis_amd_decode(S) < 0) return -1;
	if (images_out && mlsd_memcpy(images_out, S->d_img, (size_t)S->B*3*S->c.width*S->c.height*4, 1, S->stream)) return -1;
	if (mlsd_stream_sync(S->stream)) return -1;
	return 1;
}

MLB_API int mlis_amd_handoff_retries(const MLIS_AmdCtx* S) { return S->n_handoff_retries; }   /* denoise / decode / encode passes re-run on the hand-off-free plan */

MLB_API int mlis_amd_sync(MLIS_AmdCtx* S) { return mlsd_stream_sync(S->stream) ? -1 : 1; }
MLB_API void* mlis_amd_latent_device(MLIS_AmdCtx* S) { return S->d_x; }
MLB_API void* mlis_amd_image_device(MLIS_AmdCtx* S) { return S->d_img; }
MLB_API MLCtx* mlis_amd_unet_ctx(MLIS_AmdCtx* S) { return S->unet_ctx; }
MLB_API MLCtx* mlis_amd_decoder_ctx(MLIS_AmdCtx* S) { return S->dec_ctx; }
MLB_API MLCtx* mlis_amd_encoder_ctx(MLIS_AmdCtx* S) { return S->enc_ctx; }
/* every plan the engine holds, built or not yet: UNet, decoder, encoder, tile decoder, tile encoder, ControlNet, hint block (i < 7; NULL where there is none) */
MLB_API MLCtx* mlis_amd_ctx_at(MLIS_AmdCtx* S, int i)
{
	if (!S) return NULL;
	switch (i) { case 0: return S->unet_ctx; case 1: return S->dec_ctx; case 2: return S->enc_ctx; case 3: return S->dect_ctx; case 4: return S->enct_ctx;
	             case 5: return S->ctl_ctx; case 6: return S->hint_ctx; }
	return NULL;
}
MLB_API float mlis_amd_last_unet_ms(MLIS_AmdCtx* S) { return S->last_unet_ms; }
MLB_API int mlis_amd_last_nfe(MLIS_AmdCtx* S) { return S->last_nfe; }
MLB_API int mlis_amd_n_ctx_tok(const MLIS_AmdCtx* S) { return S ? S->c.n_ctx_tok : -1; }     /* context rows of the UNet plan: 77 W */
MLB_API int mlis_amd_last_n_step(MLIS_AmdCtx* S) { return S->last_n_step; }

MLB_API int mlis_amd_info(MLIS_AmdCtx* S, double* unet_flops, double* dec_flops, int* unet_ops, size_t* mem_params, size_t* mem_compute)
{
	MLCtxInfo a, b;
	mlctx_info(S->unet_ctx, &a); mlctx_info(S->dec_ctx, &b);
	if (unet_flops) *unet_flops = a.flops * (S->n_win ? S->n_eval : 1);    /* per evaluation of the whole latent: the work done, padded slots of a packed plan included */
	if (dec_flops) *dec_flops = b.flops;
	if (unet_ops) *unet_ops = (int)a.n_ops;
	if (mem_params) *mem_params = a.mem_params + b.mem_params;
	if (mem_compute) *mem_compute = a.mem_compute + b.mem_compute;
	return 1;
}
