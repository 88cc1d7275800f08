/* ESRGAN / Real-ESRGAN upscaler: RRDBNet x4 on mlsd_conv3x3_dense (csrc/hip/upscale.hip).  Not in the reference (stable-diffusion.cpp ships one as its `upscale` mode).
 *
 * The network is RRDBNet as published with ESRGAN / BasicSR (basicsr/archs/rrdbnet_arch.py), AS RECALLED WHEN THIS WAS WRITTEN: neither the publication nor a weight file
 * was at hand to check it against.  num_feat 64, num_grow_ch 32, scale 4, num_block read from the file:
 *
 *   fea   = conv_first(x)                      3 -> 64
 *   trunk = conv_body(RRDB^nb(fea));  fea = fea + trunk
 *   fea   = lrelu(conv_up1(nearest2x(fea)));   fea = lrelu(conv_up2(nearest2x(fea)))
 *   out   = conv_last(lrelu(conv_hr(fea)))     64 -> 64 -> 3
 *   RDB : x1 = lrelu(conv1(x)); x2 = lrelu(conv2(x|x1)); x3 = lrelu(conv3(x|x1|x2)); x4 = lrelu(conv4(x|x1|x2|x3)); out = 0.2 conv5(x|x1|x2|x3|x4) + x
 *   RRDB: out = 0.2 rdb3(rdb2(rdb1(x))) + x          (all convolutions 3x3, padding 1; LeakyReLU slope 0.2)
 *
 * Data flow.  Two ping-pong fp16 "dense" buffers [pixels][192]: conv1..4 of an RDB write their 32 channels straight into the slices 64.., 96.., 128.., 160.. of the buffer
 * they read (columns [0, Cin) are read, columns >= Cin written: no concatenation is ever materialised), conv5 writes the fp16 copy of its result into channels 0..63 of the
 * OTHER buffer.  The trunk is kept in fp32 beside them: conv5 of every RDB writes C32 = 0.2 conv + trunk, the third RDB of an RRDB also applies the RRDB's own residual
 * (resid2 = the RRDB's input, scale2 = 0.2), so the 3 nb + 1 residual adds are fp32 adds and no fp16 accumulation chain exists.  conv_first reads the input packed to 32
 * channels (weights zero-padded), conv_last (64 -> 3, fp32 out) goes through mlsd_gemm.  Input and output are planar float in 0..1; the caller clamps.  Zero padding always.
 *
 * Weights: a safetensors file (fp16 / fp32 / bf16 through tstore.c) with BasicSR's names, an optional "params_ema." or "params." prefix stripped (the older model.N naming is
 * mapped as well: up_old_name, unverified); or
 * "synth[:seed[:blocks]]": mlsd_synth_fill with standard deviation 0.1 sqrt(2 / fan_in) for the convolutions of the dense blocks (BasicSR's scaled initialisation of exactly
 * those, as recalled) and sqrt(2 / fan_in) for the seven others -- scaled by 0.1 as well, the five convolutions behind the trunk would shrink it to 1e-5 of their own
 * biases and the output would not depend on the blocks at all (tests/test_upscale_cpu.py asserts that it does); biases of deviation 0.05. */
#include "mlblock_int.h"
#include "mlimgsynth_amd.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

enum { UP_FEAT = 64, UP_GROW = 32, UP_DENSE = 192, UP_MAX_BLOCKS = 64 };

typedef struct { void* w; float* b; int cin, cin_pad, cout; } UpConv;

struct MLIS_AmdUpscaler {
	int n_block;
	UpConv first, *body /* [n_block][3][5] */, conv_body, up1, up2, hr, last;
	void* arena; size_t arena_bytes;
};

static uint64_t up_mix64(uint64_t z)
{
	z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
	z ^= z >> 27; z *= 0x94D049BB133111EBULL;
	z ^= z >> 31; return z;
}
static uint64_t up_key(const char* name, uint64_t seed)
{	/* the key derivation of mlctx_params_synth (oracle/o_core.c orc_synth_fill) */
	uint64_t h = 0xCBF29CE484222325ULL;
	for (const char *s = name; *s; ++s) { h ^= (unsigned char)*s; h *= 0x100000001B3ULL; }
	return up_mix64(h ^ (seed * 0x9E3779B97F4A7C15ULL));
}

static void conv_free(UpConv* c) { if (c->w) mlsd_free(c->w); if (c->b) mlsd_free(c->b); c->w = NULL; c->b = NULL; }

static int conv_alloc(UpConv* c, int cin, int cout)
{
	c->cin = cin; c->cin_pad = (cin + 31) / 32 * 32; c->cout = cout;
	if (mlsd_malloc(&c->w, (size_t)cout * 9 * c->cin_pad * 2) || mlsd_malloc((void**)&c->b, (size_t)cout * 4)) return -1;
	return 0;
}

static int conv_synth(UpConv* c, const char* name, uint64_t seed)
{
	char key[96];
	const float ws = (float)((strncmp(name, "body.", 5) ? 1.0 : 0.1) * sqrt(2.0 / (9.0 * c->cin))), bs = 0.05f;
	if (c->cin_pad != c->cin && mlsd_memset(c->w, 0, (size_t)c->cout * 9 * c->cin_pad * 2, NULL)) return -1;
	snprintf(key, sizeof(key), "%s.weight", name);
	if (mlsd_synth_fill(c->w, 1, (int64_t)c->cout * c->cin * 9, up_key(key, seed), 0, (float)((double)ws * 1.7320508075688772 / 65536.0), 1,
			3, 3, c->cin, c->cout, c->cin_pad, NULL)) return -1;
	snprintf(key, sizeof(key), "%s.bias", name);
	return mlsd_synth_fill(c->b, 0, c->cout, up_key(key, seed), 0, (float)((double)bs * 1.7320508075688772 / 65536.0), 0, 0, 0, 0, 0, 0, NULL) ? -1 : 0;
}

/* prefix "model.": the naming of the first ESRGAN release (an nn.Sequential), AS RECALLED AND UNVERIFIED -- no such file was at hand:
 *   conv_first model.0, body.{i}.rdb{j}.conv{k} model.1.sub.{i}.RDB{j}.conv{k}.0, conv_body model.1.sub.{num_block}, conv_up1 model.3, conv_up2 model.6, conv_hr model.8, conv_last model.10 */
static const char k_old_prefix[] = "model.";
static void up_old_name(const char* name, int n_block, char* out, size_t out_size)
{
	int i, j, k;
	if (sscanf(name, "body.%d.rdb%d.conv%d", &i, &j, &k) == 3) snprintf(out, out_size, "model.1.sub.%d.RDB%d.conv%d.0", i, j, k);
	else if (!strcmp(name, "conv_first")) snprintf(out, out_size, "model.0");
	else if (!strcmp(name, "conv_body")) snprintf(out, out_size, "model.1.sub.%d", n_block);
	else snprintf(out, out_size, "model.%d", !strcmp(name, "conv_up1") ? 3 : !strcmp(name, "conv_up2") ? 6 : !strcmp(name, "conv_hr") ? 8 : 10);
}

/* entry "<prefix><name>.weight|.bias" of the file */
static const MLTSEntry* up_find(const MLTStore* ts, const char* prefix, const char* name, int n_block, const char* suffix, char* key, size_t key_size)
{
	if (prefix == k_old_prefix) { char old[96]; up_old_name(name, n_block, old, sizeof(old)); snprintf(key, key_size, "%s.%s", old, suffix); }
	else snprintf(key, key_size, "%s%s.%s", prefix, name, suffix);
	return mlts_find(ts, key);
}

static int conv_load(UpConv* c, const MLTStore* ts, const char* prefix, const char* name, int n_block)
{
	char key[160];
	const MLTSEntry *ew = up_find(ts, prefix, name, n_block, "weight", key, sizeof(key));
	if (!ew) return mlsd_set_error(-1, "upscaler: tensor '%s' is missing", key);
	if (ew->n_dim != 4 || ew->shape[0] != 3 || ew->shape[1] != 3 || ew->shape[2] != c->cin || ew->shape[3] != c->cout) {
		if (c->cin == 3 && ew->n_dim == 4 && ew->shape[2] == 12)
			return mlsd_set_error(-1, "upscaler: '%s' has 12 input channels: the x2 pixel-unshuffle variant of RRDBNet is not supported (x4 only)", key);
		return mlsd_set_error(-1, "upscaler: '%s' has shape [%lld, %lld, %lld, %lld], expected [%d, %d, 3, 3]", key, (long long)ew->shape[3], (long long)ew->shape[2],
			(long long)ew->shape[1], (long long)ew->shape[0], c->cout, c->cin);
	}
	const int64_t nw = (int64_t)c->cout * c->cin * 9;
	const size_t np = (size_t)c->cout * 9 * c->cin_pad;
	float *f = (float*)malloc(sizeof(float) * (size_t)nw);
	uint16_t *h = (uint16_t*)calloc(np, 2);
	int r = (f && h) ? 0 : mlsd_set_error(-1, "upscaler: out of host memory");
	if (!r && mlts_entry_to_f32(ew, f, nw) < 0) r = -1;
	if (!r) {	/* [cout][cin][kh][kw] -> [cout][kh][kw][cin_pad], rounded to fp16 (nearest even) */
		for (int o=0;o<c->cout;++o) for (int i=0;i<c->cin;++i) for (int t=0;t<9;++t)
			h[((size_t)o * 9 + t) * c->cin_pad + i] = mlb_f32_to_f16_bits(f[((size_t)o * c->cin + i) * 9 + t]);
		if (mlsd_memcpy(c->w, h, np * 2, 0, NULL)) r = -1;
	}
	free(f); free(h);
	if (r) return r;
	const MLTSEntry *eb = up_find(ts, prefix, name, n_block, "bias", key, sizeof(key));
	if (!eb) return mlsd_set_error(-1, "upscaler: tensor '%s' is missing", key);
	if (eb->shape[0] != c->cout || eb->shape[1] * eb->shape[2] * eb->shape[3] != 1)
		return mlsd_set_error(-1, "upscaler: '%s' has %lld elements, expected %d", key, (long long)(eb->shape[0] * eb->shape[1] * eb->shape[2] * eb->shape[3]), c->cout);
	float b[UP_FEAT];
	if (mlts_entry_to_f32(eb, b, c->cout) < 0 || mlsd_memcpy(c->b, b, (size_t)c->cout * 4, 0, NULL)) return -1;
	return 0;
}

/* the prefix the file's names carry ("params_ema.", "params." or none; k_old_prefix for the older naming) and its block count; < 0 when it is no RRDBNet in either naming */
static int up_file_layout(const MLTStore* ts, const char** prefix)
{
	static const char* const pre[] = { "", "params_ema.", "params." };
	char key[160];
	*prefix = NULL;
	for (int i=0;i<3 && !*prefix;++i) { snprintf(key, sizeof(key), "%sconv_first.weight", pre[i]); if (mlts_find(ts, key)) *prefix = pre[i]; }
	if (!*prefix && mlts_find(ts, "model.0.weight")) *prefix = k_old_prefix;
	if (!*prefix) return mlsd_set_error(-1, "upscaler: tensor 'conv_first.weight' is missing: not an RRDBNet file in BasicSR's naming (nor 'model.0.weight' of the older one; .pth pickles are not read)");
	int nb = 0;
	for (; nb <= UP_MAX_BLOCKS; ++nb) {
		if (*prefix == k_old_prefix) snprintf(key, sizeof(key), "model.1.sub.%d.RDB1.conv1.0.weight", nb);
		else snprintf(key, sizeof(key), "%sbody.%d.rdb1.conv1.weight", *prefix, nb);
		if (!mlts_find(ts, key)) break;
	}
	if (nb < 1 && *prefix == k_old_prefix) return mlsd_set_error(-1, "upscaler: tensor 'model.1.sub.0.RDB1.conv1.0.weight' is missing");
	if (nb < 1) return mlsd_set_error(-1, "upscaler: tensor '%sbody.0.rdb1.conv1.weight' is missing", *prefix);
	if (nb > UP_MAX_BLOCKS) return mlsd_set_error(-1, "upscaler: more than %d blocks", UP_MAX_BLOCKS);
	return nb;
}

MLB_API void mlis_amd_upscaler_destroy(MLIS_AmdUpscaler* U)
{
	if (!U) return;
	UpConv *fixed[] = { &U->first, &U->conv_body, &U->up1, &U->up2, &U->hr, &U->last };
	for (int i=0;i<6;++i) conv_free(fixed[i]);
	if (U->body) for (int i=0;i<U->n_block*15;++i) conv_free(&U->body[i]);
	free(U->body);
	if (U->arena) mlsd_free(U->arena);
	free(U);
}

/* "synth[:seed[:blocks]]" -> 1 with seed and blocks, 0 for anything else (a path), < 0 for a malformed synth spec */
static int up_parse_synth(const char* spec, uint64_t* seed, int* blocks)
{
	*seed = 1234; *blocks = 2;
	if (strncmp(spec, "synth", 5) || (spec[5] && spec[5] != ':')) return 0;
	if (!spec[5]) return 1;
	char *end = NULL;
	*seed = (uint64_t)strtoull(spec + 6, &end, 10);
	if (end == spec + 6 || (*end && *end != ':')) return mlsd_set_error(-1, "upscaler: invalid synthetic model '%s' (synth[:seed[:blocks]])", spec);
	if (*end == ':') {
		const char *b = end + 1;
		const long v = strtol(b, &end, 10);
		if (end == b || *end || v < 1 || v > UP_MAX_BLOCKS) return mlsd_set_error(-1, "upscaler: invalid block count in '%s' (1 .. %d)", spec, UP_MAX_BLOCKS);
		*blocks = (int)v;
	}
	return 1;
}

MLB_API MLIS_AmdUpscaler* mlis_amd_upscaler_create(const char* spec)
{
	if (!spec || !*spec) { mlsd_set_error(-1, "upscaler: no model given"); return NULL; }
	uint64_t seed; int nb;
	const int synth = up_parse_synth(spec, &seed, &nb);
	if (synth < 0) return NULL;
	MLTStore *ts = NULL; const char *prefix = "";
	if (!synth) {
		ts = mlts_open(spec, 0);
		if (!ts) return NULL;
		if ((nb = up_file_layout(ts, &prefix)) < 0) { mlts_close(ts); return NULL; }
	}
	MLIS_AmdUpscaler *U = (MLIS_AmdUpscaler*)calloc(1, sizeof(*U));
	if (U) { U->n_block = nb; U->body = (UpConv*)calloc((size_t)nb * 15, sizeof(UpConv)); }
	int r = (U && U->body) ? 0 : mlsd_set_error(-1, "upscaler: out of host memory");
	char name[96];
#define UP_CONV(c, cin, cout, ...) do { if (!r) { snprintf(name, sizeof(name), __VA_ARGS__); \
		r = conv_alloc(c, cin, cout) ? -1 : (synth ? conv_synth(c, name, seed) : conv_load(c, ts, prefix, name, nb)); } } while (0)
	if (!r) {
		UP_CONV(&U->first, 3, UP_FEAT, "conv_first");
		for (int i=0;i<nb;++i) for (int j=0;j<3;++j) for (int k=0;k<5;++k)
			UP_CONV(&U->body[(i * 3 + j) * 5 + k], UP_FEAT + UP_GROW * k, k < 4 ? UP_GROW : UP_FEAT, "body.%d.rdb%d.conv%d", i, j + 1, k + 1);
		UP_CONV(&U->conv_body, UP_FEAT, UP_FEAT, "conv_body");
		UP_CONV(&U->up1, UP_FEAT, UP_FEAT, "conv_up1");
		UP_CONV(&U->up2, UP_FEAT, UP_FEAT, "conv_up2");
		UP_CONV(&U->hr, UP_FEAT, UP_FEAT, "conv_hr");
		UP_CONV(&U->last, UP_FEAT, 3, "conv_last");
	}
#undef UP_CONV
	if (!r && !mlsd_runtime_is_dry() && mlsd_device_sync()) r = -1;      /* (the dry runtime has no device: its copies are host copies) */
	if (ts) mlts_close(ts);
	if (r) { mlis_amd_upscaler_destroy(U); return NULL; }
	return U;
}

MLB_API int mlis_amd_upscaler_info(const MLIS_AmdUpscaler* U, int* n_block, int* scale)
{
	if (!U) return -1;
	if (n_block) *n_block = U->n_block;
	if (scale) *scale = 4;
	return 1;
}

static int dconv(const UpConv* c, const void* A, int64_t lda, int n_img, int H, int W, int upsample, int lrelu, float scale, const float* resid,
	float scale2, const float* resid2, float* C32, void* C16, int64_t ldc16)
{
	mlsd_dconv_args a; memset(&a, 0, sizeof(a));
	a.A = A; a.lda = lda; a.n_img = n_img; a.H = H; a.W = W; a.Cin = c->cin_pad; a.upsample = upsample;
	a.W_ = c->w; a.N = c->cout; a.bias = c->b; a.lrelu = lrelu;
	a.scale = scale; a.resid = resid; a.ldr = UP_FEAT; a.scale2 = scale2; a.resid2 = resid2; a.ldr2 = UP_FEAT;
	a.C32 = C32; a.ldc32 = UP_FEAT; a.C16 = C16; a.ldc16 = ldc16;
	return mlsd_conv3x3_dense(&a, NULL);
}

/* src [n_img][3][h][w] planar floats on the HOST -> dst [n_img][3][4h][4w] on the host */
MLB_API int mlis_amd_upscaler_run(MLIS_AmdUpscaler* U, const float* src, int w, int h, int n_img, float* dst)
{
	if (!U || !src || !dst || w < 1 || h < 1 || n_img < 1) return mlsd_set_error(-1, "upscaler: invalid arguments");
	if ((double)w * h * n_img * 16 >= 2147483648.0 / 4) return mlsd_set_error(-1, "upscaler: %d images of %dx%d are too large for one pass (tiled upscaling is not implemented)", n_img, w, h);
	const size_t P = (size_t)n_img * h * w;
	/* one arena, grown when a larger job comes: a failed allocation leaves nothing half allocated */
	size_t off = 0;
#define UP_TAKE(var, bytes) const size_t var = off; off += (((size_t)(bytes)) + 255) & ~(size_t)255
	UP_TAKE(o_in, P * 3 * 4); UP_TAKE(o_x16, P * 32 * 2);
	UP_TAKE(o_d0, P * UP_DENSE * 2); UP_TAKE(o_d1, P * UP_DENSE * 2);
	UP_TAKE(o_f, P * UP_FEAT * 4); UP_TAKE(o_r0, P * UP_FEAT * 4); UP_TAKE(o_r1, P * UP_FEAT * 4); UP_TAKE(o_r2, P * UP_FEAT * 4);
	UP_TAKE(o_u1, 4 * P * UP_FEAT * 2); UP_TAKE(o_u2, 16 * P * UP_FEAT * 2); UP_TAKE(o_u3, 16 * P * UP_FEAT * 2);
	UP_TAKE(o_o32, 16 * P * 4 * 4); UP_TAKE(o_out, 16 * P * 3 * 4);
#undef UP_TAKE
	if (U->arena_bytes < off) {
		if (U->arena) mlsd_free(U->arena);
		U->arena = NULL; U->arena_bytes = 0;
		if (mlsd_malloc(&U->arena, off)) return -1;
		U->arena_bytes = off;
	}
	char *base = (char*)U->arena;
	float *in32 = (float*)(base + o_in), *F = (float*)(base + o_f), *R[3] = { (float*)(base + o_r0), (float*)(base + o_r1), (float*)(base + o_r2) };
	float *o32 = (float*)(base + o_o32), *out = (float*)(base + o_out);
	uint16_t *x16 = (uint16_t*)(base + o_x16), *D[2] = { (uint16_t*)(base + o_d0), (uint16_t*)(base + o_d1) };
	uint16_t *u1 = (uint16_t*)(base + o_u1), *u2 = (uint16_t*)(base + o_u2), *u3 = (uint16_t*)(base + o_u3);

	if (mlsd_memcpy(in32, src, P * 3 * 4, 0, NULL)) return -1;
	if (mlsd_nchw_to_nhwc_f16(in32, n_img, 3, h * w, x16, n_img, 32, NULL, 1.0f, 0, NULL)) return -1;
	int cur = 0;
	if (dconv(&U->first, x16, 32, n_img, h, w, 0, 0, 1.0f, NULL, 0, NULL, F, D[cur], UP_DENSE)) return -1;
	const float *t_in = F;          /* the fp32 trunk entering the RRDB */
	for (int i=0;i<U->n_block;++i) {
		float *a = R[0], *b = R[1];     /* a takes rdb1's and then the RRDB's result, b rdb2's; R[2] is spare (from the second RRDB on it holds the input) */
		for (int j=0;j<3;++j) {
			const UpConv *c = &U->body[(i * 3 + j) * 5];
			for (int k=0;k<4;++k)
				if (dconv(&c[k], D[cur], UP_DENSE, n_img, h, w, 0, 1, 1.0f, NULL, 0, NULL, NULL, D[cur] + UP_FEAT + UP_GROW * k, UP_DENSE)) return -1;
			const float *res = j == 0 ? t_in : (j == 1 ? a : b);
			if (dconv(&c[4], D[cur], UP_DENSE, n_img, h, w, 0, 0, 0.2f, res, 0.2f, j == 2 ? t_in : NULL, j == 1 ? b : a, D[cur ^ 1], UP_DENSE)) return -1;
			cur ^= 1;
		}
		float *old_in = t_in == F ? R[2] : (float*)t_in;      /* conv_first's output stays for the long skip */
		t_in = a; R[0] = b; R[1] = old_in; R[2] = a;
	}
	/* trunk = conv_body(.); fea = fea + trunk (fp32 add in the epilogue), fp16 into the other dense buffer */
	if (dconv(&U->conv_body, D[cur], UP_DENSE, n_img, h, w, 0, 0, 1.0f, F, 0, NULL, NULL, D[cur ^ 1], UP_DENSE)) return -1;
	cur ^= 1;
	if (dconv(&U->up1, D[cur], UP_DENSE, n_img, h, w, 1, 1, 1.0f, NULL, 0, NULL, NULL, u1, UP_FEAT)) return -1;
	if (dconv(&U->up2, u1, UP_FEAT, n_img, 2 * h, 2 * w, 1, 1, 1.0f, NULL, 0, NULL, NULL, u2, UP_FEAT)) return -1;
	if (dconv(&U->hr, u2, UP_FEAT, n_img, 4 * h, 4 * w, 0, 1, 1.0f, NULL, 0, NULL, NULL, u3, UP_FEAT)) return -1;
	{	/* conv_last: 64 -> 3, fp32 out, on mlsd_gemm (the small-Cout streaming convolution where the image is large enough for it) */
		mlsd_gemm_args g; memset(&g, 0, sizeof(g));
		g.A = u3; g.lda = UP_FEAT; g.conv = 1; g.n_img = n_img; g.H = 4 * h; g.W = 4 * w; g.Cin = UP_FEAT; g.OH = 4 * h; g.OW = 4 * w;
		g.KH = 3; g.KW = 3; g.stride = 1; g.pad = 1;
		g.W_ = U->last.w; g.ldb = 9 * UP_FEAT; g.M = (int)(16 * P); g.N = 3; g.K = 9 * UP_FEAT;
		g.bias = U->last.b; g.rows_per_batch = 16 * h * w; g.ldrb = 3; g.act = MLSD_ACT_NONE;
		g.C32 = o32; g.ldc32 = 4;
		if (mlsd_gemm(&g, NULL)) return -1;
	}
	if (mlsd_nhwc_to_nchw_f32(o32, 4, n_img, 3, 16 * h * w, out, 1.0f, 0.0f, NULL)) return -1;
	if (mlsd_memcpy(dst, out, 16 * P * 3 * 4, 1, NULL) || mlsd_device_sync()) return -1;
	return 1;
}
