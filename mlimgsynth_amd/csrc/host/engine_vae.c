/* The engine's VAE codec: the decoder and encoder plans (KL-VAE or TAESD), their tile-sized plans and the tiled pass, mlis_amd_decode and mlis_amd_encode.
 * Both directions are one code path, read off a record per direction (CodecDir, below) and a state per direction (CodecState, engine_int.h). */
#include "engine_int.h"

/* What tells the two directions apart.  Indexed [use_tae] where the KL-VAE and TAESD differ. */
typedef struct {
	const char *name;
	int ch_in, ch_out;          /* KL-VAE: latent 4 -> image 3; image 3 -> 8 moments */
	int up;                     /* 1: lengths are latent pixels (tile walk: unit f, margin 8) and the output's are the input's x f; 0: image pixels (unit 1, margin 8 f), input / f */
	int bind_unscale[2];        /* mlctx_input_bind scale: 1 / scale_factor, else 1 */
	int bind_mode[2];           /* mlctx_input_bind mode; 2: x*2-1 (vae.h:36-40) */
	float post_mul[2], post_add[2];     /* the result's NHWC -> NCHW conversion; decode: sdvae_decoder_post (x+1)/2 (vae.h:43-47), TAE output is used as-is */
	int count_nonfinite;        /* the result's non-finite values are counted into d_nan (mlimgsynth.c:1323) */
} CodecDir;

static const CodecDir codec_dirs[2] = {
	[CODEC_DEC] = { "decode", 4, 3, 1, { 1, 0 }, { 0, 1 }, { 0.5f, 1.0f }, { 0.5f, 0.0f }, 0 },
	[CODEC_ENC] = { "encode", 3, 8, 0, { 0, 0 }, { 2, 0 }, { 1.0f, 1.0f }, { 0.0f, 0.0f }, 1 },
};

/* a direction's input extent and the unit and margin of its tile walk (mlis_amd_vae_tile_walk), in the input's pixels */
typedef struct { int w, h, unit, margin; } CodecGeom;
static CodecGeom codec_geom(const MLIS_AmdCtx* S, int dir)
{
	const int f = S->vae_p.f_down;
	return codec_dirs[dir].up ? (CodecGeom){ S->lw, S->lh, f, 8 } : (CodecGeom){ S->c.width, S->c.height, 1, 8*f };
}
/* a length of the input as a length of the output */
static int codec_out(const MLIS_AmdCtx* S, int dir, int n) { return codec_dirs[dir].up ? n * S->vae_p.f_down : n / S->vae_p.f_down; }

/* the whole-size buffers of a direction, NCHW [B][ch][h][w].  out 0: what the full plan reads and a tiled pass gathers from; out 1: what a tiled pass pastes into */
static float** codec_full_buf(MLIS_AmdCtx* S, int dir, int out)
{
	float **buf[2][2] = { [CODEC_DEC] = { &S->d_x, &S->d_img }, [CODEC_ENC] = { &S->d_img_in, &S->d_mom } };
	return buf[dir][out];
}
/* ... allocated at its first use (the encoder's; the decoder's exist from creation on) */
static int codec_full_buf_alloc(MLIS_AmdCtx* S, int dir, int out)
{
	const CodecGeom G = codec_geom(S, dir);
	const size_t px = out ? (size_t)codec_out(S, dir, G.w) * codec_out(S, dir, G.h) : (size_t)G.w * G.h;
	float **p = codec_full_buf(S, dir, out);
	return !*p && mlsd_malloc((void**)p, (size_t)S->B * (out ? codec_dirs[dir].ch_out : codec_dirs[dir].ch_in) * px * 4) ? -1 : 0;
}

/* A codec plan for `batch` inputs of w x h (decode: latent pixels, encode: image pixels) read from `bound`, its convolutions wrapping as `wrap` says; the input
 * tensor goes to *t_in.  The parameters are synthesised, or with defer_weights left for the caller to load.  Returns the plan, or NULL if it did not build --
 * unless `failed` is given: then the plan comes back either way, *failed says which, and computing a failed one reports its error. */
static MLCtx* codec_plan_build(MLIS_AmdCtx* S, int dir, int w, int h, int batch, float* bound, int wrap, MLTensor** t_in, int* failed)
{
	const CodecDir *D = &codec_dirs[dir];
	const int tae = S->c.use_tae != 0, dec = dir == CODEC_DEC;
	MLCtx *C = mlctx_new(S->stream);
	mlctx_set_conv_wrap(C, wrap);
	mlctx_set_vae_attn(C, S->vae_attn);
	int ok = (tae ? (dec ? sdtae_decode_init : sdtae_encode_init)(C, w, h, batch, t_in) : (dec ? sdvae_decode_init : sdvae_encode_init)(C, &S->vae_p, w, h, batch, t_in)) >= 0 &&
	         mlctx_input_bind(*t_in, bound, batch, NULL, D->bind_unscale[tae] ? 1 / S->vae_p.scale_factor : 1.0f, D->bind_mode[tae]) >= 0 &&
	         (tae ? (dec ? sdtae_decode_build : sdtae_encode_build)(C, *t_in) : (dec ? sdvae_decode_build : sdvae_encode_build)(C, &S->vae_p, *t_in)) >= 0;
	if (ok && !S->c.defer_weights) ok = mlctx_params_synth(C, S->c.weight_seed) >= 0;
	if (failed) *failed = !ok;
	else if (!ok) { mlctx_destroy(C); C = NULL; }
	return C;
}

/* builds (once) the plan of the whole latent / image, with the engine's seamless tiling; the decoder's at creation, the encoder's before the first untiled encode */
MLCtx* codec_full_prepare(MLIS_AmdCtx* S, int dir)
{
	CodecPlan *p = &S->codec[dir].full;
	const CodecGeom G = codec_geom(S, dir);
	if (p->ctx) return p->ctx;
	if (codec_full_buf_alloc(S, dir, 0)) return NULL;
	return p->ctx = codec_plan_build(S, dir, G.w, G.h, S->B, *codec_full_buf(S, dir, 0), S->tiling, &p->t_in, NULL);
}

static void codec_plan_drop(CodecPlan* p) { if (p->ctx) mlctx_destroy(p->ctx); p->ctx = NULL; }

/* destroys what `which` names (CODEC_DROP_*): the decoder, the encoder, both tile plans, both directions' tile buffers; the caller has drained the stream */
void codec_plans_drop(MLIS_AmdCtx* S, int which)
{
	for (int dir=0; dir<2; ++dir) {
		CodecState *K = &S->codec[dir];
		if (which & (1 << dir)) codec_plan_drop(&K->full);
		if (which & CODEC_DROP_TILE) codec_plan_drop(&K->tile);
		if (which & CODEC_DROP_TILE_BUFS) {
			mlsd_free(K->d_tile_in); mlsd_free(K->d_tile_out);
			K->d_tile_in = K->d_tile_out = NULL;
			K->tile_in_bytes = K->tile_out_bytes = 0;
		}
	}
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
		/* the tile buffers have the size of one tile: the next *_tile_prepare allocates them for the new one */
		codec_plans_drop(S, CODEC_DROP_TILE | CODEC_DROP_TILE_BUFS);
		S->vae_tile = tile_px;
	}
	return 1;
}

/* The mid-block attention of the KL-VAE plans: 0 = scores in memory (the default), 1 = one flash launch (mlsd_attention_wide).  A change drops the codec plans
 * only: the full-size decoder is rebuilt here (its parameters are synthesised again, or left for the caller to load: mlctx_params_loaded, as at creation), the
 * encoder and the two tile plans at their next use.  The UNet plan, its weights and every device buffer of the engine stay.  TAESD has no attention: nothing to do. */
MLB_API int mlis_amd_set_vae_attn(MLIS_AmdCtx* S, int mode)
{
	if (!S) return fail("mlis_amd_set_vae_attn: no engine");
	if (mode != 0 && mode != 1) return mlsd_set_error(-1, "mlis_amd_set_vae_attn: mode %d (0 scores, 1 flash)", mode);
	if (mode == S->vae_attn) return 1;
	S->vae_attn = mode;
	if (S->c.use_tae) return 1;
	mlsd_stream_sync(S->stream);
	codec_plans_drop(S, CODEC_DROP_TILE | CODEC_DROP_ENC);
	CodecPlan *dec = &S->codec[CODEC_DEC].full;
	MLCtx *old = dec->ctx;
	int failed = 0;
	dec->ctx = codec_plan_build(S, CODEC_DEC, S->lw, S->lh, S->B, S->d_x, S->tiling, &dec->t_in, &failed);      /* (a plan that failed to build stays in place: the next decode reports its error) */
	mlctx_destroy(old);
	return failed ? -1 : 1;
}
MLB_API int mlis_amd_vae_attn_mode(const MLIS_AmdCtx* S) { return S ? S->vae_attn : -1; }

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
static int tile_buf(float** p, size_t* have, size_t nbytes)
{
	if (*p && *have >= nbytes) return 0;
	mlsd_free(*p); *p = NULL; *have = 0;
	if (mlsd_malloc((void**)p, nbytes)) return -1;
	*have = nbytes;
	return 0;
}

/* builds (once) the tile plan of a direction; returns NULL with no error when tiling does not apply.
 * The tile plans take ONE image: a batch walks them image by image (the tile buffers hold the tile of every image, the plan's input moves from one to the next).
 * A tile of image b is then computed by the same launches whatever the batch size -- GEMM tiles and K splits are chosen by M = images x pixels, so a plan of
 * B images would round differently from the plan of one -- and the plan's activations, what tiling is there to bound, do not grow with the batch.
 * They are built without the convolution wrap: a tile's edge is not the image's. */
static MLCtx* codec_tile_prepare(MLIS_AmdCtx* S, int dir)
{
	const CodecDir *D = &codec_dirs[dir];
	CodecState *K = &S->codec[dir];
	if (K->tile.ctx) return K->tile.ctx;
	if (S->vae_tile <= 0 || S->c.use_tae) return NULL;
	const CodecGeom G = codec_geom(S, dir);
	const int n0 = tile_dims(S->vae_tile, 2*G.margin, G.w, G.unit), n1 = tile_dims(S->vae_tile, 2*G.margin, G.h, G.unit);
	if (n0 == G.w && n1 == G.h) return NULL;                                          /* one tile: disabled (vae.c:347-348) */
	const size_t B = S->B;
	if (codec_full_buf_alloc(S, dir, 0)) return NULL;
	if (tile_buf(&K->d_tile_in, &K->tile_in_bytes, B * D->ch_in * n0 * n1 * 4)) return NULL;
	if (tile_buf(&K->d_tile_out, &K->tile_out_bytes, B * D->ch_out * codec_out(S, dir, n0) * codec_out(S, dir, n1) * 4)) return NULL;
	if (codec_full_buf_alloc(S, dir, 1)) return NULL;
	K->tile.ctx = codec_plan_build(S, dir, n0, n1, 1, K->d_tile_in, 0, &K->tile.t_in, NULL);
	if (K->tile.ctx) { K->tile_w = n0; K->tile_h = n1; }
	return K->tile.ctx;
}
MLB_API MLCtx* mlis_amd_decoder_tile_prepare(MLIS_AmdCtx* S) { return codec_tile_prepare(S, CODEC_DEC); }
MLB_API MLCtx* mlis_amd_encoder_tile_prepare(MLIS_AmdCtx* S) { return codec_tile_prepare(S, CODEC_ENC); }

/* One tiled pass (src/vae.c:351-383 decode, 262-299 encode), walked by mlis_amd_vae_tile_walk: per tile, its slice of every image is gathered, each image runs
 * through the tile plan and is converted to NCHW (elementwise: commutes with the paste), and the interiors are pasted into the whole-size output. */
static int codec_run_tiled(MLIS_AmdCtx* S, int dir)
{
	const CodecDir *D = &codec_dirs[dir];
	CodecState *K = &S->codec[dir];
	const CodecGeom G = codec_geom(S, dir);
	const int B = S->B, n0 = K->tile_w, n1 = K->tile_h, o0 = codec_out(S, dir, n0), o1 = codec_out(S, dir, n1);
	const float *src = *codec_full_buf(S, dir, 0);
	float *dst = *codec_full_buf(S, dir, 1);
	void *st = S->stream;
	int64_t ld = 0;
	const float *y = mlctx_tensor_device_f32(K->tile.ctx, mlctx_result(K->tile.ctx), &ld);
	TileWalk w0, w1 = {0};
	int R = -1;
	K->n_tile_evals = 0;
	if (tile_walk_new(&w0, G.w, S->vae_tile, G.unit, G.margin) || tile_walk_new(&w1, G.h, S->vae_tile, G.unit, G.margin)) goto end;
	if (w0.n != n0 || w1.n != n1) { mlsd_set_error(-1, "VAE tiling: the %s tile plan is %dx%d, the walk's tile %dx%d", D->name, n0, n1, w0.n, w1.n); goto end; }
	for (int t1=0; t1<w1.cnt; ++t1) {
		const int i1 = w1.org[t1], d1 = w1.off[t1];
		for (int t0=0; t0<w0.cnt; ++t0) {
			const int i0 = w0.org[t0], d0 = w0.off[t0];
			if (mlsd_copy_slice2(K->d_tile_in, n0, n1, src, G.w, G.h, n0, n1, 0, 0, i0, i1, B*D->ch_in, st)) goto end;
			for (int b=0; b<B; ++b) {
				if (mlctx_input_rebind(K->tile.ctx, K->tile.t_in, K->d_tile_in + (size_t)b*D->ch_in*n0*n1) < 0) goto end;
				if (mlctx_compute(K->tile.ctx) < 0) goto end;
				K->n_tile_evals++;
				if (D->count_nonfinite && mlsd_count_nonfinite(y, (size_t)o0*o1*ld, S->d_nan, st)) goto end;
				if (mlsd_nhwc_to_nchw_f32(y, ld, 1, D->ch_out, o0*o1, K->d_tile_out + (size_t)b*D->ch_out*o0*o1, D->post_mul[0], D->post_add[0], st)) goto end;
			}
			if (mlsd_copy_slice2(dst, codec_out(S, dir, G.w), codec_out(S, dir, G.h), K->d_tile_out, o0, o1, codec_out(S, dir, w0.wid[t0]), codec_out(S, dir, w1.wid[t1]),
					codec_out(S, dir, i0+d0), codec_out(S, dir, i1+d1), codec_out(S, dir, d0), codec_out(S, dir, d1), B*D->ch_out, st)) goto end;
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
	const CodecState *K = &S->codec[which];
	const int have = K->tile.ctx != NULL;
	int n = 0;
	if (have) {
		const CodecGeom G = codec_geom(S, which);
		const int c0 = mlis_amd_vae_tile_walk(G.w, S->vae_tile, G.unit, G.margin, NULL, NULL, NULL, NULL, 0);
		const int c1 = mlis_amd_vae_tile_walk(G.h, S->vae_tile, G.unit, G.margin, NULL, NULL, NULL, NULL, 0);
		n = c0 > 0 && c1 > 0 ? c0 * c1 : -1;
	}
	if (tile_w) *tile_w = have ? K->tile_w : 0;
	if (tile_h) *tile_h = have ? K->tile_h : 0;
	if (in_bytes) *in_bytes = K->tile_in_bytes;
	if (out_bytes) *out_bytes = K->tile_out_bytes;
	if (n_tiles) *n_tiles = n;
	if (n_evals) *n_evals = K->n_tile_evals;
	return have;
}

/* The launches of one pass of a direction, on its tile plan or on its full plan.  If the plan hands data over inside launches, they are drained and checked: after
 * a hand-off that gave up waiting the plan is made hand-off-free and the launches run once more -- at most one retry, then -1.  The count of non-finite values
 * starts again with the second attempt. */
static int codec_run(MLIS_AmdCtx* S, int dir, int tiled)
{
	const CodecDir *D = &codec_dirs[dir];
	MLCtx *C = tiled ? S->codec[dir].tile.ctx : S->codec[dir].full.ctx;
	for (int attempt=0; ; ++attempt) {
		if (attempt && D->count_nonfinite && mlsd_memset(S->d_nan, 0, 4, S->stream)) return -1;
		if (tiled) {
			if (codec_run_tiled(S, dir) < 0) return -1;
		} else {
			if (mlctx_compute(C) < 0) return -1;
			int64_t ld = 0;
			const float *y = mlctx_tensor_device_f32(C, mlctx_result(C), &ld);
			if (D->count_nonfinite && mlsd_count_nonfinite(y, (size_t)S->B*S->hw*ld, S->d_nan, S->stream)) return -1;
		}
		if (!mlctx_handoff_ops(C) && !attempt) return 1;
		if (mlsd_stream_sync(S->stream)) return -1;
		if (mlctx_handoff_check(C) == 0) return 1;
		if (attempt) return -1;
		mlctx_handoffs_off(C);
		S->n_handoff_retries++;
	}
}

MLB_API int mlis_amd_decode(MLIS_AmdCtx* S)
{
	const CodecDir *D = &codec_dirs[CODEC_DEC];
	if (codec_tile_prepare(S, CODEC_DEC)) return codec_run(S, CODEC_DEC, 1);
	if (codec_run(S, CODEC_DEC, 0) < 0) return -1;
	MLCtx *C = S->codec[CODEC_DEC].full.ctx;
	const int tae = S->c.use_tae != 0;
	int64_t ld = 0;
	const float *y = mlctx_tensor_device_f32(C, mlctx_result(C), &ld);
	if (mlsd_nhwc_to_nchw_f32(y, ld, S->B, D->ch_out, S->c.width * S->c.height, S->d_img, D->post_mul[tae], D->post_add[tae], S->stream)) return -1;
	return 1;
}

/* builds the encoder plan (once) without running it; with defer_weights the caller loads its parameters before the first encode */
MLB_API MLCtx* mlis_amd_encoder_prepare(MLIS_AmdCtx* S) { return codec_full_prepare(S, CODEC_ENC); }

/* mlis_image_encode (src/mlimgsynth.c:1301-1330): images host NCHW [B][3][H][W] in [0,1] -> the resident latent becomes
 * the sampled (VAE: mean + std*N(0,1), one Philox call per image, src/vae.c:203-229) or direct (TAE) encoding and is
 * marked as the initial latent of the next denoise.  The encoder plan is built on first use. */
MLB_API int mlis_amd_encode(MLIS_AmdCtx* S, const float* images, int sample)
{
	const CodecDir *D = &codec_dirs[CODEC_ENC];
	const int B = S->B, W = S->c.width, H = S->c.height, tae = S->c.use_tae != 0;
	const size_t img_elems = (size_t)B*3*W*H;
	void *st = S->stream;
	const int tiled = codec_tile_prepare(S, CODEC_ENC) != NULL;
	if (!tiled && !codec_full_prepare(S, CODEC_ENC)) return -1;
	if (mlsd_memcpy(S->d_img_in, images, img_elems*4, 0, st)) return -1;
	if (mlsd_memset(S->d_nan, 0, 4, st)) return -1;
	if (codec_run(S, CODEC_ENC, tiled) < 0) return -1;
	MLCtx *C = S->codec[CODEC_ENC].full.ctx;
	int64_t ld = 0;
	const float *y = tiled ? NULL : mlctx_tensor_device_f32(C, mlctx_result(C), &ld);
	if (tae) {
		if (mlsd_nhwc_to_nchw_f32(y, ld, B, 4, S->hw, S->d_x, D->post_mul[tae], D->post_add[tae], st)) return -1;
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
