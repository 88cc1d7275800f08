/* UNet denoiser on the MI355X plan builder — re-creation of the reference's src/unet.c.
 * Topology, hyper-parameters and parameter names follow the reference line by line; the graph
 * takes a batch N (cond and uncond of every image together), activations are channels-last and
 * the ggml permute/cont/reshape/concat nodes have no counterpart (they are free here).
 */
#include "mlblock_int.h"
#include "mlimgsynth_amd.h"
#include <math.h>

#define T true
#define MLN(NAME,X)  mlctx_tensor_add(C, (NAME), (X))

/* ------------------------------------------------------------------ hyper-parameters (src/unet.c:21-83) */
MLB_API int unet_params_get(const char* model, UnetParams* U)
{
	memset(U, 0, sizeof(*U));
	U->n_ch_in=4; U->n_ch_out=4; U->n_res_blk=2; U->n_te=1280; U->n_ch=320;
	U->n_step_train=1000; U->sigma_min=0.029167158f; U->sigma_max=14.614641f;
	if (!strcmp(model,"sd1")) {
		int a[4]={4,2,1,0}, m[5]={1,2,4,4,0}, d[5]={1,1,1,1,0};
		memcpy(U->attn_res,a,sizeof(a)); memcpy(U->ch_mult,m,sizeof(m)); memcpy(U->transf_depth,d,sizeof(d));
		U->n_head=8; U->n_ctx=768; U->clip_norm=1;
	} else if (!strcmp(model,"sd2")) {
		int a[4]={4,2,1,0}, m[5]={1,2,4,4,0}, d[5]={1,1,1,1,0};
		memcpy(U->attn_res,a,sizeof(a)); memcpy(U->ch_mult,m,sizeof(m)); memcpy(U->transf_depth,d,sizeof(d));
		U->d_head=64; U->n_ctx=1024; U->clip_norm=1; U->vparam=1;
	} else if (!strcmp(model,"sdxl")) {
		int a[4]={4,2,0,0}, m[5]={1,2,4,0,0}, d[5]={1,2,10,0,0};
		memcpy(U->attn_res,a,sizeof(a)); memcpy(U->ch_mult,m,sizeof(m)); memcpy(U->transf_depth,d,sizeof(d));
		U->d_head=64; U->n_ctx=2048; U->ch_adm_in=2816; U->cond_label=1; U->uncond_empty_zero=1;
	} else if (!strcmp(model,"tiny")) {
		int a[4]={2,1,0,0}, m[5]={1,2,0,0,0}, d[5]={1,1,0,0,0};
		memcpy(U->attn_res,a,sizeof(a)); memcpy(U->ch_mult,m,sizeof(m)); memcpy(U->transf_depth,d,sizeof(d));
		U->n_ch=64; U->n_te=256; U->n_head=2; U->n_ctx=64; U->n_res_blk=1; U->clip_norm=1;
	} else if (!strcmp(model,"tinyv")) {   /* tiny with v-prediction (SD2-style: d_head given, vparam) */
		int a[4]={2,1,0,0}, m[5]={1,2,0,0,0}, d[5]={1,1,0,0,0};
		memcpy(U->attn_res,a,sizeof(a)); memcpy(U->ch_mult,m,sizeof(m)); memcpy(U->transf_depth,d,sizeof(d));
		U->n_ch=64; U->n_te=256; U->d_head=32; U->n_ctx=64; U->n_res_blk=1; U->clip_norm=1; U->vparam=1;
	} else if (!strcmp(model,"tinyxl")) {
		int a[4]={2,0,0,0}, m[5]={1,2,0,0,0}, d[5]={1,2,0,0,0};
		memcpy(U->attn_res,a,sizeof(a)); memcpy(U->ch_mult,m,sizeof(m)); memcpy(U->transf_depth,d,sizeof(d));
		U->n_ch=64; U->n_te=256; U->d_head=64; U->n_ctx=128; U->n_res_blk=2; U->ch_adm_in=96;
		U->cond_label=1; U->uncond_empty_zero=1;
	} else return mlsd_set_error(-1, "unknown UNet model '%s'", model);
	return 1;
}

static bool static_vector_in(const int* svec, int v)
{
	for (unsigned i=0; svec[i]; ++i) if (v == svec[i]) return true;
	return false;
}

/* HyperTile's tile rule (include/mlimgsynth_amd.h): the smallest divisor of `side` that is at least min(max(tile_px / px_per_token, 4), side) */
MLB_API int mlis_amd_hypertile_side(int side, int px_per_token, int tile_px)
{
	if (side < 1 || px_per_token < 1) return side;
	int m = tile_px / px_per_token;
	if (m < 4) m = 4;
	if (m > side) m = side;
	while (side % m) ++m;
	return m;
}

/* one permuting copy of a tiled spatial transformer: the dense fp16 rows of `t` (n maps of h x w tokens) into a fresh fp16 tensor, image order -> tile-major order
 * or back (mlsd_tile_permute).  It rides on the copy kind: nbytes is the whole extent, the geometry says how the rows move. */
static MLTensor* mlb_tile_permute16(MLCtx* C, MLTensor* t, int th, int tw, int inverse)
{
	const void *src = mlt_need16(C, t);
	if (!src) return NULL;
	/* (cannot happen in a spatial transformer: both operands have d_embed or the block's channel count, a multiple of 32 by the GroupNorm in front of it, so their
	 * fp16 rows are dense and whole 16-byte pieces; a builder that came here with anything else gets an error, not a silently untiled level) */
	if (t->ld16 != t->c || (t->c * 2) % 16) { mlctx_fail(C, "hypertile: rows of %d halfs at stride %lld", t->c, (long long)t->ld16); return NULL; }
	MLTensor *y = mlt_new(C, t->n, t->h, t->w, t->c);
	y->sz16 = (size_t)t->n * t->h * t->w * t->c * 2;
	y->d16 = mlctx_dalloc(C, y->sz16, 0); y->ld16 = t->c;
	if (!y->d16) return NULL;
	MLOp *op = mlctx_op_new(C, OP_COPY_F32, inverse ? "hypertile_untile" : "hypertile_tile");
	mlb_copy_args *a = &op->u.copy;
	a->src = src; a->dst = y->d16; a->nbytes = y->sz16;
	a->n_img = t->n; a->H = t->h; a->W = t->w; a->th = th; a->tw = tw; a->row_bytes = t->c * 2; a->inverse = inverse;
	return y;
}

/* src/unet.c:110-145.  Consumes nothing: x0 stays valid (it is the block's residual).
 * ds is the UNet downscale of the level.  HyperTile (mlctx_set_hypertile): on a level the rule cuts, the token rows are in tile-major order from proj_in's A operand
 * to proj_out's A operand, and every self-attention in between runs per tile (C->ht.nt).  The two copies sit on the fp16 operands, not on the fp32 token matrix:
 * half the bytes, proj_in still ends with the first LayerNorm (that fold needs the LayerNorm right behind the GEMM that defines its input), and the GroupNorm
 * statistics wiring sees the producers it saw (x0's producer before the block, proj_out behind it).  proj_in / proj_out are 1x1 convolutions: per token, so
 * the order of the rows does not matter to them; the residual x0 and the block's output are in image order. */
static MLTensor* mlb_spatial_transf(MLCtx* C, MLTensor* x, MLTensor* ctx,
	int d_embed, int d_head, int n_head, int n_depth, int ds)
{
	MLTensor *x0 = x;
	char name[64];
	mlctx_block_begin(C);
	const int ch_in = x->c;
	if (!n_head)  n_head  = d_embed / d_head;
	if (!d_head)  d_head  = d_embed / n_head;
	if (!d_embed) d_embed = d_head * n_head;
	int th = x->h, tw = x->w, lvl = 0;
	while ((1 << lvl) < ds) ++lvl;
	if (C->ht.tile_px > 0 && lvl <= C->ht.depth && lvl < 4) {
		th = mlis_amd_hypertile_side(x->h, 8 * ds, C->ht.tile_px);
		tw = mlis_amd_hypertile_side(x->w, 8 * ds, C->ht.tile_px);
	}
	const int tiled = th != x->h || tw != x->w;
	if (tiled) { C->ht.n_tiled++; int *q = C->ht.tiles[lvl]; q[0] = th; q[1] = tw; q[2] = x->h / th; q[3] = x->w / tw; }
	else C->ht.n_untiled++;

	MLTensor *h = MLN("norm", mlb_groupnorm_ex(C, x, 32, 1e-6f, 0, 0, NULL));
	if (tiled && h) {
		MLTensor *hp = mlb_tile_permute16(C, h, th, tw, 0);
		if (!hp) return NULL;
		mlb_release(C, h);
		h = hp;
	}
	/* proj_in: 1x1 conv; its output IS the token matrix [N][h*w][d_embed] (no permute needed) */
	x = MLN("proj_in", mlb_conv2d_ex(C, h, d_embed, 1, 1, 0, 0, T, NULL));
	if (!x || !mlt_need32(C, x)) return NULL;
	mlb_release(C, h);
	if (tiled) C->ht.nt = (x0->h / th) * (x0->w / tw);
	for (int i=0; i<n_depth; ++i) {
		sprintf(name, "transf.%d", i);
		x = MLN(name, mlb_basic_transf(C, x, ctx, d_embed, d_embed, n_head));   /* consumes x */
		if (!x) { C->ht.nt = 0; return NULL; }
	}
	C->ht.nt = 0;
	if (tiled) {
		MLTensor *xi = mlb_tile_permute16(C, x, th, tw, 1);
		if (!xi) return NULL;
		mlb_release(C, x);
		x = xi;
	}
	MLEpilogue ep = {0}; ep.resid = x0;
	MLTensor *y = MLN("proj_out", mlb_conv2d_ex(C, x, ch_in, 1, 1, 0, 0, T, &ep));
	mlb_release(C, x);
	return y;
}

/* src/unet.c:147-165 */
static MLTensor* mlb_unet__embed(MLCtx* C, MLTensor* time, MLTensor* label, const UnetParams* P)
{
	MLTensor *te = mlb_timestep_embedding(C, time, P->n_ch, 10000);
	MLEpilogue silu = {0}; silu.act = MLSD_ACT_SILU;
	MLTensor *e0 = MLN("time_embed.0", mlb_linear_ex(C, te, P->n_te, T, &silu, 0));
	MLTensor *emb = MLN("time_embed.2", mlb_linear_ex(C, e0, P->n_te, T, NULL, 0));
	if (!emb) return NULL;
	if (P->ch_adm_in && label) {
		MLTensor *l0 = MLN("label_embed.0", mlb_linear_ex(C, label, P->n_te, T, &silu, 0));
		if (!mlt_need32(C, emb)) return NULL;
		MLEpilogue add = {0}; add.resid = emb;       /* emb + label_embed (ggml_add :161) */
		MLTensor *le = MLN("label_embed.2", mlb_linear_ex(C, l0, P->n_te, T, &add, 0));
		mlb_release(C, l0);
		emb = le;
	}
	if (!mlt_need32(C, emb)) return NULL;
	mlb_release(C, te); mlb_release(C, e0);
	return emb;
}

/* total width of all cross-attention k/v projections of the graph (same walk as __in/__mid/__out) */
static int unet_cross_kv_width_ex(const UnetParams* P, int with_out)
{
	int total = 0, im = 0, ds = 1;
	for (; P->ch_mult[im]; ++im) {
		if (im) ds *= 2;
		if (static_vector_in(P->attn_res, ds)) total += P->n_res_blk * P->transf_depth[im] * 2 * P->n_ch * P->ch_mult[im];          /* in  */
	}
	im--;
	total += P->transf_depth[im] * 2 * P->n_ch * P->ch_mult[im];                                                                  /* mid */
	if (!with_out) return total;                                                                                                  /* (the ControlNet: encoder and middle block) */
	for (; im >= 0; --im, ds /= 2)
		if (static_vector_in(P->attn_res, ds)) total += (P->n_res_blk + 1) * P->transf_depth[im] * 2 * P->n_ch * P->ch_mult[im];   /* out */
	return total;
}

static int unet_cross_kv_width(const UnetParams* P) { return unet_cross_kv_width_ex(P, 1); }

/* HyperTile: the spatial transformers of a UNet plan of lw x lh latent pixels that mlb_spatial_transf would tile with this setting (same walk: a level's map is the
 * ceil-half of the one above -- 3x3 stride-2 convolution, padding 1 --, n_res_blk encoder and n_res_blk + 1 decoder transformers on the levels of attn_res, the
 * middle block's at the deepest level whatever that list says).  0: the plan is the plain plan.  tests/test_hypertile_cpu.py holds it to what built plans report. */
MLB_API int unet_hypertile_cuts(const UnetParams* P, int lw, int lh, int tile_px, int depth)
{
	int n = 0;
	if (tile_px <= 0) return 0;
	for (int im=0, ds=1, w=lw, h=lh; P->ch_mult[im]; ++im, ds*=2, w=(w+1)/2, h=(h+1)/2) {
		const int count = (static_vector_in(P->attn_res, ds) ? 2 * P->n_res_blk + 1 : 0) + (P->ch_mult[im+1] ? 0 : 1);
		if (count && im <= depth && im < 4 && (mlis_amd_hypertile_side(h, 8 * ds, tile_px) != h || mlis_amd_hypertile_side(w, 8 * ds, tile_px) != w)) n += count;
	}
	return n;
}

/* total width of the resnets' time-embedding projections (same walk; every resnet projects emb to its ch_out) */
static int unet_emb_proj_width_ex(const UnetParams* P, int with_out)
{
	int total = 0, im = 0;
	for (; P->ch_mult[im]; ++im) total += P->n_res_blk * P->n_ch * P->ch_mult[im];       /* in  */
	im--;
	total += 2 * P->n_ch * P->ch_mult[im];                                                /* mid */
	if (!with_out) return total;
	for (; im >= 0; --im) total += (P->n_res_blk + 1) * P->n_ch * P->ch_mult[im];         /* out */
	return total;
}

/* base + gain * ctrl as a FRESH fp32 tensor (mlsd_ctrl_add): `ctrl` is a residual of the ControlNet plan, channels-last fp32 in that plan's memory, the gain one float
 * in device memory.  The result has no producing GEMM and no fp16 form: a GroupNorm that reads it computes its own statistics (the producer's column statistics
 * describe `base`), and nothing cached for `base` (d16, silu16) is taken for the sum. */
static MLTensor* mlb_ctrl_add(MLCtx* C, MLTensor* base, const UnetControl* K, int i)
{
	if (!base || C->err) return NULL;
	const int64_t rows = (int64_t)base->n * base->h * base->w;
	/* image n reads control image n % K->n_img: whole repeats of the control batch, or -- a plan with a perturbed group (mlctx_set_pag), whose ControlNet plan holds the
	 * other groups only -- that batch once and then its FIRST images, the cond group the perturbed group copies, for the last pag.n_img images */
	const int pag_tail = C->pag.n_img > 0 && base->n == K->n_img + C->pag.n_img && C->pag.n_img <= K->n_img;
	if (i < 0 || i >= K->n || !K->r[i] || !K->gain || K->c[i] != base->c || K->rows[i] != base->h * base->w || K->n_img < 1 || (base->n % K->n_img && !pag_tail)) {
		mlctx_fail(C, "unet: control residual %d does not match a %d x %d x %d map", i, base->n, base->h * base->w, base->c); return NULL;
	}
	const float *b = mlt_need32(C, base);
	if (!b) return NULL;
	MLTensor *y = mlt_new(C, base->n, base->h, base->w, base->c);
	y->sz32 = (size_t)rows * base->c * sizeof(float);
	y->d32 = (float*)mlctx_dalloc(C, y->sz32, 0); y->ld32 = base->c;
	if (!y->d32) return NULL;
	MLOp *op = mlctx_op_new(C, OP_CTRL_ADD, "ctrl_add");
	op->u.cadd.dst = y->d32; op->u.cadd.ld_dst = y->ld32; op->u.cadd.base = b; op->u.cadd.ld_base = base->ld32;
	op->u.cadd.ctrl = K->r[i]; op->u.cadd.ld_ctrl = K->ld[i];
	op->u.cadd.n_img = base->n; op->u.cadd.rows = base->h * base->w; op->u.cadd.C = base->c; op->u.cadd.n_ctrl = K->n_img; op->u.cadd.gain = K->gain;
	return y;
}

static int unet_emb_proj_width(const UnetParams* P) { return unet_emb_proj_width_ex(P, 1); }

/* FreeU on one operand of a decoder concatenation, as a FRESH fp32 tensor like mlb_ctrl_add's (no producer statistics, no cached fp16 form): kind OP_FREEU_BACKBONE
 * (mlsd_freeu_backbone) or OP_FREEU_SKIP (mlsd_freeu_skip); `f` is the factor, one float in device memory.  The workspace is plan memory, free again for whatever
 * is recorded after the op. */
static MLTensor* mlb_freeu(MLCtx* C, MLTensor* t, const float* f, MLOpKind kind)
{
	if (!t || C->err) return NULL;
	if (!f || (t->c & 7) || t->h < 2 || t->w < 2) {
		mlctx_fail(C, "unet: FreeU on a %d x %d x %d map (channels a multiple of 8, at least 2 x 2 pixels)", t->w, t->h, t->c); return NULL;
	}
	const float *src = mlt_need32(C, t);
	if (!src) return NULL;
	const int64_t rows = (int64_t)t->n * t->h * t->w;
	MLTensor *y = mlt_new(C, t->n, t->h, t->w, t->c);
	y->sz32 = (size_t)rows * t->c * sizeof(float);
	y->d32 = (float*)mlctx_dalloc(C, y->sz32, 0); y->ld32 = t->c;
	const size_t sz_ws = mlsd_freeu_ws_bytes(t->n, t->h, t->w, t->c);
	float *ws = (float*)mlctx_dalloc(C, sz_ws, 0);
	if (!y->d32 || !ws) return NULL;
	MLOp *op = mlctx_op_new(C, kind, kind == OP_FREEU_BACKBONE ? "freeu_backbone" : "freeu_skip");
	op->u.freeu.dst = y->d32; op->u.freeu.ld_dst = y->ld32; op->u.freeu.src = src; op->u.freeu.ld_src = t->ld32;
	op->u.freeu.n_img = t->n; op->u.freeu.H = t->h; op->u.freeu.W = t->w; op->u.freeu.C = t->c; op->u.freeu.ws = ws; op->u.freeu.f = f;
	mlctx_drelease(C, ws, sz_ws);
	return y;
}


MLB_API MLTensor* mlb_unet_denoise(MLCtx* C, MLTensor* x, MLTensor* time, MLTensor* ctx, MLTensor* label, const UnetParams* P)
{
	return mlb_unet_denoise_ctrl(C, x, time, ctx, label, P, NULL);
}

/* K != NULL: the UNet of a ControlNet (cldm.py ControlledUnetModel): mid.2's output and every tensor popped from the skip stack get g x the matching residual added
 * (K->r[i] for the i-th tensor pushed, K->r[K->n - 1] for the middle block).  K == NULL records exactly the plan of mlb_unet_denoise. */
MLB_API MLTensor* mlb_unet_denoise_ctrl(MLCtx* C, MLTensor* x, MLTensor* time, MLTensor* ctx, MLTensor* label, const UnetParams* P, const UnetControl* K)
{
	return mlb_unet_denoise_freeu(C, x, time, ctx, label, P, K, NULL);
}

/* F != NULL: FreeU (version 2 of the published code) at the decoder's concatenations.  The stage follows the BACKBONE's channel count as the published forward does:
 * n_ch x the top multiplier (1280 for SD1 / SD2 / SDXL) is stage 1 with (b1, s1), half of that stage 2 with (b2, s2), anything else is left alone.  There the
 * backbone goes through mlsd_freeu_backbone and the popped skip tensor -- after the control sum, where there is one -- through mlsd_freeu_skip, then the two are
 * concatenated.  F->n_stage1 / n_stage2 count the concatenations treated.  F == NULL records exactly the plan of mlb_unet_denoise_ctrl. */
MLB_API MLTensor* mlb_unet_denoise_freeu(MLCtx* C, MLTensor* x, MLTensor* time, MLTensor* ctx, MLTensor* label, const UnetParams* P, const UnetControl* K,
	UnetFreeU* F)
{
	char name[64];
	mlctx_block_begin(C);
	if (mlb_cross_kv_batch(C, ctx, unet_cross_kv_width(P)) < 0) return NULL;
	MLTensor *emb = mlb_unet__embed(C, time, label, P);
	if (!emb) return NULL;
	if (mlb_emb_proj_batch(C, emb, unet_emb_proj_width(P)) < 0) return NULL;

	/* ---- mlb_unet__in, src/unet.c:167-203 */
	MLTensor *stack[40]; int ns = 0;
	x = MLN("in.conv", mlb_conv2d_ex(C, x, P->n_ch, 3, 1, 1, 0, T, NULL));
	if (!x || !mlt_need32(C, x)) return NULL;
	stack[ns++] = x;
	int im=0, i_blk=0, ds=1, ch=P->n_ch;
	for (; P->ch_mult[im]; ++im) {
		if (im) {
			ds *= 2; i_blk++;
			sprintf(name, "in.%d.0", i_blk);
			x = MLN(name, mlb_downsample(C, x, ch, false));
			if (!x || !mlt_need32(C, x)) return NULL;
			stack[ns++] = x;
		}
		for (int j=0; j<P->n_res_blk; ++j) {
			i_blk++;
			sprintf(name, "in.%d.0", i_blk);
			ch = P->n_ch * P->ch_mult[im];
			x = MLN(name, mlb_resnet_ex(C, x, emb, ch));
			if (!x || !mlt_need32(C, x)) return NULL;
			if (static_vector_in(P->attn_res, ds)) {
				sprintf(name, "in.%d.1", i_blk);
				MLTensor *y = MLN(name, mlb_spatial_transf(C, x, ctx, ch, P->d_head, P->n_head, P->transf_depth[im], ds));
				if (!y || !mlt_need32(C, y)) return NULL;
				mlb_release(C, x);
				x = y;
			}
			stack[ns++] = x;
		}
	}

	/* ---- mlb_unet__mid, src/unet.c:205-217 */
	im = 0; while (P->ch_mult[im+1]) im++;
	ch = P->n_ch * P->ch_mult[im];
	{
		MLTensor *y = MLN("mid.0", mlb_resnet_ex(C, x, emb, ch));   /* x stays on the skip stack */
		if (!y || !mlt_need32(C, y)) return NULL;
		x = y;
		/* perturbed-attention guidance (mlctx_set_pag): the self-attentions of this block, and of no other, treat the plan's last pag.n_img images as perturbed */
		C->pag.cur = C->pag.n_img;
		y = MLN("mid.1", mlb_spatial_transf(C, x, ctx, ch, P->d_head, P->n_head, P->transf_depth[im], ds));
		C->pag.cur = 0;
		if (!y || !mlt_need32(C, y)) return NULL;
		mlb_release(C, x); x = y;
		y = MLN("mid.2", mlb_resnet_ex(C, x, emb, ch));
		if (!y || !mlt_need32(C, y)) return NULL;
		mlb_release(C, x); x = y;
		if (K) {
			if (K->n != ns + 1) { mlctx_fail(C, "unet: %d control residuals for %d skip tensors and the middle block", K->n, ns); return NULL; }
			y = mlb_ctrl_add(C, x, K, K->n - 1);
			if (!y) return NULL;
			mlb_release(C, x); x = y;
		}
	}

	/* ---- mlb_unet__out, src/unet.c:219-261 */
	im = 0; ds = 1;
	while (P->ch_mult[im+1]) { im++; ds *= 2; }
	const int ch_top = P->n_ch * P->ch_mult[im];
	if (F) { F->n_stage1 = F->n_stage2 = 0; if (!F->f) { mlctx_fail(C, "unet: FreeU without its factors"); return NULL; } }
	for (int i_oblk=0; im>=0; --im) {
		for (int j=0; j<P->n_res_blk+1; ++j, ++i_oblk) {
			if (ns <= 0) { mlctx_fail(C, "unet: skip stack underflow"); return NULL; }
			MLTensor *hsk = stack[--ns];
			const int fu_stage = !F ? 0 : x->c == ch_top ? 1 : 2 * x->c == ch_top ? 2 : 0;
			if (fu_stage) {
				MLTensor *xb = mlb_freeu(C, x, F->f + (fu_stage - 1), OP_FREEU_BACKBONE);
				if (!xb) return NULL;
				mlb_release(C, x); x = xb;
			}
			if (K) {
				MLTensor *hc = mlb_ctrl_add(C, hsk, K, ns);
				if (!hc) return NULL;
				mlb_release(C, hsk); hsk = hc;
			}
			if (fu_stage) {
				MLTensor *hf = mlb_freeu(C, hsk, F->f + 2 + (fu_stage - 1), OP_FREEU_SKIP);
				if (!hf) return NULL;
				mlb_release(C, hsk); hsk = hf;
				if (fu_stage == 1) F->n_stage1++; else F->n_stage2++;
			}
			MLTensor *cat = mlb_concat_ch(C, x, hsk);            /* ggml_concat(x, h, 2): zero-copy */
			int i_sub = 0;
			ch = P->n_ch * P->ch_mult[im];
			sprintf(name, "out.%d.%d", i_oblk, i_sub++);
			MLTensor *y = MLN(name, mlb_resnet_ex(C, cat, emb, ch));
			if (!y || !mlt_need32(C, y)) return NULL;
			mlb_release(C, x); mlb_release(C, hsk);
			x = y;
			if (static_vector_in(P->attn_res, ds)) {
				sprintf(name, "out.%d.%d", i_oblk, i_sub++);
				y = MLN(name, mlb_spatial_transf(C, x, ctx, ch, P->d_head, P->n_head, P->transf_depth[im], ds));
				if (!y || !mlt_need32(C, y)) return NULL;
				mlb_release(C, x); x = y;
			}
			if (im != 0 && j == P->n_res_blk) {
				sprintf(name, "out.%d.%d", i_oblk, i_sub++);
				y = MLN(name, mlb_upsample(C, x, ch));
				if (!y || !mlt_need32(C, y)) return NULL;
				mlb_release(C, x); x = y;
				ds /= 2;
			}
		}
	}
	if (ns != 0) { mlctx_fail(C, "unet: skip stack not empty"); return NULL; }

	MLTensor *h = MLN("out.norm", mlb_groupnorm_ex(C, x, 32, 1e-6f, 1, 0, NULL));
	mlb_release(C, x);
	x = MLN("out.conv", mlb_conv2d_ex(C, h, P->n_ch_out, 3, 1, 1, 0, T, NULL));
	if (!x || !mlt_need32(C, x)) return NULL;
	mlb_release(C, h);
	mlb_release(C, emb);
	return x;
}

/* ------------------------------------------------------------------ sigma tables (src/unet.c:283-334) */
static float g_log_sigmas_sd[1000];
/* the zero-terminal-SNR table (UnetParams.zsnr; "Common Diffusion Noise Schedules and Sample Steps are Flawed", 2023, Algorithm 1; not in the reference): with
 * s_i = sqrt(abar_i) of the table above, s'_i = (s_i - s_999) s_0 / (s_0 - s_999), abar'_i = s'_i^2.  abar'_999 would be 0 and its sigma infinite, which a
 * k-diffusion sampler cannot walk, so the last entry is clamped to the constant below: the front ends' value AS RECALLED, not pinned against their code. */
#define UNET_ZSNR_ABAR_LAST 4.8973451890853435e-08
static float g_log_sigmas_zsnr[1000];

MLB_API void unet_params_init(void)
{
	if (g_log_sigmas_sd[0]) return;
	unsigned n = 1000;
	double linear_start = 0.00085, linear_end = 0.0120,
	       b = sqrt(linear_start), e = sqrt(linear_end),
	       f = (e - b) / (n - 1), alpha_cumprod = 1.0;
	double abar[1000];
	for (unsigned i=0; i<n; ++i) {
		double beta = b + f*i, alpha = 1.0 - beta*beta;
		alpha_cumprod *= alpha;
		abar[i] = alpha_cumprod;
	}
	/* both tables from the doubles of that one loop; the plain table's first entry, the "done" mark above, is written last */
	const double s0 = sqrt(abar[0]), sT = sqrt(abar[n-1]);
	for (unsigned i=0; i<n; ++i) {
		double sz = (sqrt(abar[i]) - sT) * s0 / (s0 - sT), az = i == n-1 ? UNET_ZSNR_ABAR_LAST : sz * sz;
		g_log_sigmas_zsnr[i] = log(sqrt((1 - az) / az));
	}
	for (unsigned i=n; i-- > 0; ) {
		double sigma = sqrt((1 - abar[i]) / abar[i]);
		g_log_sigmas_sd[i] = log(sigma);
	}
}

MLB_API const float* unet_log_sigmas(int zsnr) { unet_params_init(); return zsnr ? g_log_sigmas_zsnr : g_log_sigmas_sd; }
MLB_API int unet_params_sizeof(void) { return (int)sizeof(UnetParams); }

/* the sigma range of the table a model walks: UnetParams.sigma_min / sigma_max follow its zsnr flag (the plain table's are the reference's constants) */
MLB_API void unet_params_set_zsnr(UnetParams* P, int zsnr)
{
	unet_params_init();
	P->zsnr = zsnr ? 1 : 0;
	P->sigma_min = 0.029167158f;
	P->sigma_max = zsnr ? (float)exp(g_log_sigmas_zsnr[999]) : 14.614641f;
}

static float linear_interp(unsigned n, const float* vec, float t)
{
	int ti = t;
	if (ti < 0) ti = 0; else if (ti > (int)n-1) ti = (int)n-1;
	float v1 = vec[ti], v2 = ti+1 < (int)n ? vec[ti+1] : v1;
	return v1*(ti+1-t) + v2*(t-ti);
}

/* position where vec crosses v: first index with vec[i] >= v, then the slope of the FOLLOWING interval
 * (BISECT_RIGHT with a comparison that is never 0: src/unet.c:315-322, src/ccommon/bisect.h:38-51) */
static float linear_est(unsigned n, const float* vec, float v)
{
	size_t b = 0, e = n;
	while (b < e) {
		size_t i = (b + e) / 2;
		if (copysign(1, vec[i] - v) < 0) b = i + 1; else e = i;
	}
	size_t idx = b;
	if (idx + 1 >= n) return n - 1;
	float v1 = vec[idx], v2 = vec[idx+1];
	return idx + (v - v1) / (v2 - v1);
}

MLB_API float unet_sigma_to_t(const UnetParams* P, float sigma)
{
	unet_params_init();
	float ls = log(sigma);
	return linear_est(P->n_step_train, P->zsnr ? g_log_sigmas_zsnr : g_log_sigmas_sd, ls);
}

MLB_API float unet_t_to_sigma(const UnetParams* P, float t)
{
	unet_params_init();
	float ls = linear_interp(P->n_step_train, P->zsnr ? g_log_sigmas_zsnr : g_log_sigmas_sd, t);
	return exp(ls);
}

/* ------------------------------------------------------------------ graph setup / host-boundary run */
MLB_API int unet_denoise_init_n(UnetState* S, MLCtx* C, const UnetParams* P, unsigned lw, unsigned lh, unsigned n_batch)
{
	return unet_denoise_init_nc(S, C, P, lw, lh, n_batch, 77);
}

MLB_API int unet_denoise_init_nc(UnetState* S, MLCtx* C, const UnetParams* P, unsigned lw, unsigned lh, unsigned n_batch, int n_ctx_tok)
{
	if (!n_ctx_tok) n_ctx_tok = 77;
	if (n_ctx_tok < 0 || n_ctx_tok % 77 || n_ctx_tok > 77 * MLIS_AMD_MAX_WINDOWS) return mlsd_set_error(-1, "unet: context of %d rows (77 x W, W <= %d)", n_ctx_tok, MLIS_AMD_MAX_WINDOWS);
	unet_params_init();
	memset(S, 0, sizeof(*S));
	mlctx_begin(C, "UNet");
	mlctx_set_tprefix(C, "unet");
	S->t_x = mlctx_input_new_img(C, "x", lw, lh, P->n_ch_in, n_batch);
	S->t_t = mlctx_input_new_seq(C, "t", MLT_F32, n_batch, 1, 1);
	S->t_c = mlctx_input_new_seq(C, "c", MLT_F32, P->n_ctx, n_ctx_tok, n_batch);
	if (P->ch_adm_in) S->t_l = mlctx_input_new_seq(C, "l", MLT_F32, P->ch_adm_in, 1, n_batch);
	S->ctx = C; S->par = P; S->lw = lw; S->lh = lh; S->n_batch = n_batch;
	return 1;
}

/* second half of init, split so that callers may bind the x input to a resident latent first */
MLB_API int unet_denoise_build(UnetState* S) { return unet_denoise_build_ctrl(S, NULL); }

MLB_API int unet_denoise_build_ctrl(UnetState* S, const UnetControl* K) { return unet_denoise_build_freeu(S, K, NULL); }

MLB_API int unet_denoise_build_freeu(UnetState* S, const UnetControl* K, UnetFreeU* F)
{
	MLCtx *C = S->ctx;
	S->t_out = mlb_unet_denoise_freeu(C, S->t_x, S->t_t, S->t_c, S->t_l, S->par, K, F);
	if (!S->t_out) return -1;
	if (mlctx_prep(C) < 0) return -1;
	return 1;
}

MLB_API int unet_denoise_run_n(UnetState* S, const float* x, const float* cond, const float* label,
	const float* sigma, float* dx)
{
	MLCtx *C = S->ctx;
	const UnetParams *P = S->par;
	const int N = S->n_batch, hw = S->lw * S->lh, nc = P->n_ch_in;
	const size_t nx = (size_t)N * nc * hw;
	float *xs = (float*)malloc(nx * sizeof(float));
	float *ts = (float*)malloc(N * sizeof(float));
	for (int n=0; n<N; ++n) {
		ts[n] = unet_sigma_to_t(P, sigma[n]);
		float c_in = 1 / sqrt(sigma[n]*sigma[n] + 1);                 /* src/unet.c:470-472 */
		for (size_t i=0; i<(size_t)nc*hw; ++i) xs[(size_t)n*nc*hw + i] = x[(size_t)n*nc*hw + i] * c_in;
	}
	int R = 1;
	if (mlctx_input_set(C, S->t_x, xs, nx*4) < 0) R = -1;
	if (R > 0 && mlctx_input_set(C, S->t_t, ts, N*4) < 0) R = -1;
	if (R > 0 && mlctx_input_set(C, S->t_c, cond, (size_t)N*S->t_c->w*P->n_ctx*4) < 0) R = -1;    /* (w: the plan's context rows) */
	if (R > 0 && S->t_l && mlctx_input_set(C, S->t_l, label, (size_t)N*P->ch_adm_in*4) < 0) R = -1;
	if (R > 0 && mlctx_compute_checked(C) < 0) R = -1;            /* (re-runs on the hand-off-free plan after a timed-out in-launch hand-off) */
	if (R > 0 && mlctx_output_get(C, S->t_out, dx, nx*4) < 0) R = -1;
	S->nfe++;
	if (R > 0) {
		for (size_t i=0; i<nx; ++i) if (!isfinite(dx[i])) { R = mlsd_set_error(-1, "NaN found in UNet output"); break; }   /* :487 */
	}
	if (R > 0 && P->vparam) {                                                                  /* :490-494 */
		for (int n=0; n<N; ++n) {
			float s = sigma[n], c_skip = s / (s*s + 1), c_out = 1 / sqrt(s*s + 1);
			for (size_t i=0; i<(size_t)nc*hw; ++i) { size_t k = (size_t)n*nc*hw + i; dx[k] = dx[k]*c_out + x[k]*c_skip; }
		}
	}
	free(xs); free(ts);
	return R;
}

/* ------------------------------------------------------------------ the reference's signatures (src/unet.h:55-62, src/unet.c:336-388,460-498) */
MLB_API int unet_denoise_init(UnetState* S, MLCtx* C, const UnetParams* P, unsigned lw, unsigned lh, bool split)
{
	(void)split;   /* --unet-split re-uploads half the weights per half-graph to save memory (:390-458): replaced by residency */
	if (unet_denoise_init_n(S, C, P, lw, lh, 1) < 0) return -1;
	return unet_denoise_build(S);
}

MLB_API int unet_denoise_run(UnetState* S, const LocalTensor* x, const LocalTensor* cond, const LocalTensor* label, float sigma, LocalTensor* dx)
{
	const UnetParams *P = S->par;
	if (!x || !cond || !dx || x->n[0] != S->lw || x->n[1] != S->lh || x->n[2] != P->n_ch_in || x->n[3] != 1)
		return mlsd_set_error(-1, "unet_denoise_run: x shape does not match the initialised graph");
	if (cond->n[0] != P->n_ctx || cond->n[1] != 77) return mlsd_set_error(-1, "unet_denoise_run: cond must be [%d,77]", P->n_ctx);
	if (P->ch_adm_in && (!label || label->n[0] != P->ch_adm_in)) return mlsd_set_error(-1, "unet_denoise_run: label must be [%d]", P->ch_adm_in);
	if (dx != x) ltensor_resize(dx, x->n[0], x->n[1], x->n[2], x->n[3]);   /* ltensor_resize_like(dx, x) (:466) */
	return unet_denoise_run_n(S, x->d, cond->d, label ? label->d : NULL, &sigma, dx->d);
}

/* ------------------------------------------------------------------ ControlNet (not in the reference; the published cldm.py ControlNet / ControlledUnetModel)
 * A copy of the UNet's encoder and middle block that also sees a control image.  Parameters under the prefix "control":
 *   time_embed.*, label_embed.*, in.*, mid.*      as under "unet."
 *   hint.<0|2|..|14>                              input_hint_block: eight 3x3 convolutions on the RGB image at pixel size, SiLU between them, three of stride 2
 *   zero.<i>                                      1x1 convolution on the i-th tensor the UNet would push on its skip stack; its output is residual i
 *   mid_out                                       1x1 convolution on mid.2's output: the last residual
 * The hint block depends on the image alone, so it is a plan of its own (control_hint_*) that runs once per image; the ControlNet plan takes its output as the fp32
 * channels-last tensor `t_hint`, one copy per plan image, and adds it to in.conv's output in that convolution's epilogue. */
MLB_API int control_hint_init(MLCtx* C, const UnetParams* P, unsigned w, unsigned h, MLTensor** t_img)
{
	if (w % 8 || h % 8 || !w || !h) return mlsd_set_error(-1, "control hint: image size %ux%u must be a multiple of 8", w, h);
	mlctx_begin(C, "ControlHint");
	mlctx_set_tprefix(C, "control");
	*t_img = mlctx_input_new_img(C, "hint", w, h, 3, 1);
	(void)P;
	return 1;
}

MLB_API int control_hint_build(MLCtx* C, const UnetParams* P, MLTensor* t_img)
{
	static const int width[7] = { 16, 16, 32, 32, 96, 96, 256 }, stride[8] = { 1, 1, 2, 1, 2, 1, 2, 1 };
	char name[32];
	MLTensor *x = t_img;
	mlctx_block_begin(C);
	for (int i=0; i<8; ++i) {
		MLEpilogue silu = {0}; silu.act = MLSD_ACT_SILU;
		sprintf(name, "hint.%d", 2*i);
		MLTensor *y = MLN(name, mlb_conv2d_ex(C, x, i < 7 ? width[i] : P->n_ch, 3, stride[i], 1, 0, T, i < 7 ? &silu : NULL));
		if (!y) return -1;
		if (i == 7) { if (!mlt_need32(C, y)) return -1; }
		else if (!mlt_need16(C, y)) return -1;
		if (i) mlb_release(C, x);
		x = y;
	}
	if (mlctx_prep(C) < 0) return -1;
	return 1;
}

MLB_API int controlnet_init_nc(ControlState* S, MLCtx* C, const UnetParams* P, unsigned lw, unsigned lh, unsigned n_batch, int n_ctx_tok)
{
	if (!n_ctx_tok) n_ctx_tok = 77;
	if (n_ctx_tok < 0 || n_ctx_tok % 77 || n_ctx_tok > 77 * MLIS_AMD_MAX_WINDOWS) return mlsd_set_error(-1, "controlnet: context of %d rows (77 x W, W <= %d)", n_ctx_tok, MLIS_AMD_MAX_WINDOWS);
	unet_params_init();
	memset(S, 0, sizeof(*S));
	mlctx_begin(C, "ControlNet");
	mlctx_set_tprefix(C, "control");
	S->t_x = mlctx_input_new_img(C, "x", lw, lh, P->n_ch_in, n_batch);
	S->t_t = mlctx_input_new_seq(C, "t", MLT_F32, n_batch, 1, 1);
	S->t_c = mlctx_input_new_seq(C, "c", MLT_F32, P->n_ctx, n_ctx_tok, n_batch);
	if (P->ch_adm_in) S->t_l = mlctx_input_new_seq(C, "l", MLT_F32, P->ch_adm_in, 1, n_batch);
	/* the hint embedding, channels-last fp32 [n_batch][lh lw][n_ch]: written by the caller straight into device memory (mlctx_tensor_device_f32), never by an op */
	MLTensor *th = mlt_new(C, n_batch, lh, lw, P->n_ch);
	th->sz32 = 0; th->ld32 = P->n_ch; th->def_op = -1;
	th->d32 = (float*)mlctx_dalloc(C, (size_t)n_batch * lw * lh * P->n_ch * sizeof(float), 0);
	snprintf(th->name, sizeof(th->name), "hint");
	S->t_hint = th;
	S->ctx = C; S->par = P; S->lw = lw; S->lh = lh; S->n_batch = n_batch;
	return th->d32 ? 1 : -1;
}

/* residual i: zero.<i> on a tensor of the ControlNet's forward path (which goes on unchanged) */
static int control_zero(MLCtx* C, ControlState* S, MLTensor* x, const char* name)
{
	if (S->n_res >= MLB_CONTROL_MAX) return mlctx_fail(C, "controlnet: more than %d residuals", MLB_CONTROL_MAX);
	MLTensor *r = MLN(name, mlb_conv2d_ex(C, x, x->c, 1, 1, 0, 0, T, NULL));
	if (!r || !mlt_need32(C, r)) return -1;
	S->t_res[S->n_res++] = r;         /* never released: the UNet plan reads it */
	return 1;
}

MLB_API MLTensor* mlb_controlnet(MLCtx* C, ControlState* S, MLTensor* x, MLTensor* time, MLTensor* ctx, MLTensor* label, MLTensor* hint, const UnetParams* P)
{
	char name[64];
	mlctx_block_begin(C);
	if (mlb_cross_kv_batch(C, ctx, unet_cross_kv_width_ex(P, 0)) < 0) return NULL;
	MLTensor *emb = mlb_unet__embed(C, time, label, P);
	if (!emb) return NULL;
	if (mlb_emb_proj_batch(C, emb, unet_emb_proj_width_ex(P, 0)) < 0) return NULL;
	S->n_res = 0;

	/* ---- the walk of mlb_unet__in; a zero convolution wherever the UNet pushes */
	MLEpilogue eh = {0}; eh.resid = hint;                       /* h = in.conv(x) + hint block (cldm.py: guided_hint is added after the first input block only) */
	x = MLN("in.conv", mlb_conv2d_ex(C, x, P->n_ch, 3, 1, 1, 0, T, &eh));
	if (!x || !mlt_need32(C, x)) return NULL;
	if (control_zero(C, S, x, "zero.0") < 0) return NULL;
	int im=0, i_blk=0, ds=1, ch=P->n_ch;
	for (; P->ch_mult[im]; ++im) {
		if (im) {
			ds *= 2; i_blk++;
			sprintf(name, "in.%d.0", i_blk);
			MLTensor *y = MLN(name, mlb_downsample(C, x, ch, false));
			if (!y || !mlt_need32(C, y)) return NULL;
			mlb_release(C, x); x = y;
			sprintf(name, "zero.%d", S->n_res);
			if (control_zero(C, S, x, name) < 0) return NULL;
		}
		for (int j=0; j<P->n_res_blk; ++j) {
			i_blk++;
			sprintf(name, "in.%d.0", i_blk);
			ch = P->n_ch * P->ch_mult[im];
			MLTensor *y = MLN(name, mlb_resnet_ex(C, x, emb, ch));
			if (!y || !mlt_need32(C, y)) return NULL;
			mlb_release(C, x); x = y;
			if (static_vector_in(P->attn_res, ds)) {
				sprintf(name, "in.%d.1", i_blk);
				y = MLN(name, mlb_spatial_transf(C, x, ctx, ch, P->d_head, P->n_head, P->transf_depth[im], ds));
				if (!y || !mlt_need32(C, y)) return NULL;
				mlb_release(C, x); x = y;
			}
			sprintf(name, "zero.%d", S->n_res);
			if (control_zero(C, S, x, name) < 0) return NULL;
		}
	}

	/* ---- mlb_unet__mid, then mid_out */
	im = 0; while (P->ch_mult[im+1]) im++;
	ch = P->n_ch * P->ch_mult[im];
	MLTensor *y = MLN("mid.0", mlb_resnet_ex(C, x, emb, ch));
	if (!y || !mlt_need32(C, y)) return NULL;
	mlb_release(C, x); x = y;
	y = MLN("mid.1", mlb_spatial_transf(C, x, ctx, ch, P->d_head, P->n_head, P->transf_depth[im], ds));
	if (!y || !mlt_need32(C, y)) return NULL;
	mlb_release(C, x); x = y;
	y = MLN("mid.2", mlb_resnet_ex(C, x, emb, ch));
	if (!y || !mlt_need32(C, y)) return NULL;
	mlb_release(C, x); x = y;
	if (control_zero(C, S, x, "mid_out") < 0) return NULL;
	mlb_release(C, x);
	mlb_release(C, emb);
	return S->t_res[S->n_res - 1];
}

MLB_API int controlnet_build(ControlState* S)
{
	MLCtx *C = S->ctx;
	if (!mlb_controlnet(C, S, S->t_x, S->t_t, S->t_c, S->t_l, S->t_hint, S->par)) return -1;
	if (mlctx_prep(C) < 0) return -1;
	return 1;
}

/* what the UNet plan needs to know of a built ControlNet plan: where its residuals lie.  gain_dev: the float (device memory) every sum reads its gain from */
MLB_API int controlnet_control(const ControlState* S, const float* gain_dev, UnetControl* K)
{
	memset(K, 0, sizeof(*K));
	if (!S || !S->n_res || !gain_dev) return mlsd_set_error(-1, "controlnet_control: no built ControlNet plan");
	for (int i=0; i<S->n_res; ++i) {
		const MLTensor *r = S->t_res[i];
		K->r[i] = r->d32; K->ld[i] = r->ld32; K->c[i] = r->c; K->rows[i] = r->h * r->w;
	}
	K->n = S->n_res; K->n_img = S->n_batch; K->gain = gain_dev;
	return 1;
}
