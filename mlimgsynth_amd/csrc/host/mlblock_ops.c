/* What the executor knows about each kind of plan op, written once: k_op_class[kind] (MLOpClass, mlblock_int.h).
 * mlblock.c looks everything up here and holds no switch over the kinds.  To add a kind: DESIGN.md section 4. */
#include "mlblock_int.h"
#include <stddef.h>

/* ------------------------------------------------------------------ launches */
static int run_gemm(const MLOp* op, void* st) { return mlsd_gemm(&op->u.gemm, st); }
static int run_attn(const MLOp* op, void* st) { return mlsd_attention(&op->u.attn, st); }
static int run_attn_ctx(const MLOp* op, void* st) { return mlsd_attention_ctx(&op->u.attn, st); }   /* cross attention over more than 96 context rows (windowed prompt) */
static int run_gn(const MLOp* op, void* st)
{
	if (op->fused) return 0;                    /* its producer's reduce pass ends with it (wire_gn_fold) */
	return mlsd_groupnorm(&op->u.gn, st);
}
static int run_ln(const MLOp* op, void* st)
{
	const mlb_ln_args *a = &op->u.ln;
	if (op->fused) return 0;                    /* its producer ends with it (wire_ln_fold) */
	return mlsd_layernorm(a->x, a->ldx, a->rows, a->d, a->eps, a->g, a->b, a->y16, a->y32, st);
}
static int run_n2h(const MLOp* op, void* st)
{
	const mlb_n2h_args *a = &op->u.n2h;
	return mlsd_nchw_to_nhwc_f16(a->src, a->n_src, a->C, a->HW, a->dst, a->n_dst, a->Cpad, a->scale, a->scale0, a->mode, st);
}
static int run_h2n(const MLOp* op, void* st)
{
	const mlb_h2n_args *a = &op->u.h2n;
	return mlsd_nhwc_to_nchw_f32(a->src, a->ld, a->n, a->C, a->HW, a->dst, a->mul, a->add, st);
}
static int run_temb(const MLOp* op, void* st)
{
	const mlb_temb_args *a = &op->u.temb;
	return mlsd_timestep_embedding(a->t, a->n, a->dim, a->maxp, a->out, st);
}
static int run_act(const MLOp* op, void* st) { return mlsd_act_f32_to_f16(op->u.act.x, op->u.act.y, op->u.act.n, op->u.act.act, st); }
static int run_cemb(const MLOp* op, void* st)
{
	const mlb_cemb_args *a = &op->u.cemb;
	return mlsd_clip_embed(a->tok, a->n, a->T, a->d, a->tw, a->pw, a->out, st);
}
static int run_smax(const MLOp* op, void* st)
{
	const mlb_smax_args *a = &op->u.smax;
	return mlsd_softmax_rows(a->in, a->ld_in, a->out, a->ld_out, a->rows, a->cols, a->scale, st);
}
static int run_copy(const MLOp* op, void* st)
{
	const mlb_copy_args *a = &op->u.copy;
	if (a->th > 0) return mlsd_tile_permute(a->src, a->dst, a->n_img, a->H, a->W, a->th, a->tw, a->row_bytes, a->inverse, st);      /* HyperTile's row permutation */
	return mlsd_memcpy(a->dst, a->src, a->nbytes, 2, st);
}
static int run_xavt(const MLOp* op, void* st)
{
	const mlb_xavt_args *a = &op->u.xavt;
	return mlsd_xattn_pack_vt(a->v, a->ldv, a->n_img, a->Tk, a->N, a->vt, st);
}
static int run_cadd(const MLOp* op, void* st)
{
	const mlb_cadd_args *a = &op->u.cadd;
	return mlsd_ctrl_add(a->dst, a->ld_dst, a->base, a->ld_base, a->ctrl, a->ld_ctrl, a->n_img, a->rows, a->C, a->n_ctrl, a->gain, st);
}
static int run_freeu_backbone(const MLOp* op, void* st)
{
	const mlb_freeu_args *a = &op->u.freeu;
	return mlsd_freeu_backbone(a->dst, a->ld_dst, a->src, a->ld_src, a->n_img, a->H * a->W, a->C, a->ws, a->f, st);
}
static int run_freeu_skip(const MLOp* op, void* st)
{
	const mlb_freeu_args *a = &op->u.freeu;
	return mlsd_freeu_skip(a->dst, a->ld_dst, a->src, a->ld_src, a->n_img, a->H, a->W, a->C, a->ws, a->f, st);
}

/* ------------------------------------------------------------------ outputs that are not simply "the field, if set" */
static int gemm_outputs(const MLOp* op, const void* out[MLOP_MAX_OUTPUTS])
{
	const mlsd_gemm_args *g = &op->u.gemm;
	int n = 0;
	if (g->C32) out[n++] = g->C32;
	if (g->C16) out[n++] = g->C16;
	if (g->ln_y16) out[n++] = g->ln_y16;
	if (g->gn_y16) out[n++] = g->gn_y16;
	if (g->xa_k) out[n++] = g->xa_out;          /* (the cross-attention ending is on when it has its keys) */
	return n;
}

/* ------------------------------------------------------------------ algorithmic HBM bytes: every operand read once, every output written once (DESIGN.md "roofline") */
static double gemm_bytes(const MLOp* op)
{
	const mlsd_gemm_args *g = &op->u.gemm;
	const double nout = g->act == MLSD_ACT_GEGLU ? g->N / 2 : g->N;
	double b = g->conv ? 2.0 * g->n_img * g->H * g->W * g->Cin : 2.0 * g->M * (double)g->K;
	b += 2.0 * g->N * (double)g->K;
	if (g->bias) b += 4.0 * g->N;
	if (g->rowbias) b += 4.0 * (g->M / (g->rows_per_batch > 0 ? g->rows_per_batch : 1)) * (double)g->N;
	if (g->resid) b += 4.0 * g->M * nout;
	if (g->C32) b += 4.0 * g->M * nout;
	if (g->C16) b += 2.0 * g->M * nout;
	if (g->xa_k) b += 2.0 * g->M * nout + 2.0 * 2.0 * (g->M / g->xa_Tq) * (double)g->xa_Tk * g->N;      /* the attention's output + the images' K and V */
	return b;
}
static double attn_bytes(const MLOp* op)
{
	const mlsd_attn_args *a = &op->u.attn;
	const double D = (double)a->n_head * a->d_head;
	return 2.0 * a->n_batch * D * (2.0 * a->Tq + 2.0 * a->Tk);
}
static double gn_bytes(const MLOp* op)
{
	const mlsd_gn_args *a = &op->u.gn;
	if (op->fused) return 0.0;
	const double n = (double)a->n_img * a->HW * (a->C1 + a->C2);
	return n * (4.0 + 2.0 + (a->raw16 ? 2.0 : 0.0));
}
static double ln_bytes(const MLOp* op)
{
	if (op->fused) return 0.0;
	return (double)op->u.ln.rows * op->u.ln.d * (4.0 + (op->u.ln.y16 ? 2.0 : 0.0) + (op->u.ln.y32 ? 4.0 : 0.0));
}
static double smax_bytes(const MLOp* op) { return (double)op->u.smax.rows * op->u.smax.cols * 6.0; }
static double act_bytes(const MLOp* op) { return (double)op->u.act.n * 6.0; }
static double copy_bytes(const MLOp* op) { return 2.0 * op->u.copy.nbytes; }
static double cadd_bytes(const MLOp* op) { return 12.0 * op->u.cadd.n_img * (double)op->u.cadd.rows * op->u.cadd.C; }      /* base and ctrl read, dst written (gain 0: ctrl is not read) */
static double freeu_bytes(const MLOp* op) { return 12.0 * op->u.freeu.n_img * (double)op->u.freeu.H * op->u.freeu.W * op->u.freeu.C; }      /* src read by the reduction and by the apply, dst written (factor 1: one read) */

/* ------------------------------------------------------------------ MLB_F_OPSHAPES: what follows "<label> " */
static const char* gemm_unnamed(const MLOp* op) { return mlsd_gemm_variant(&op->u.gemm); }
static void gemm_shape(const MLOp* op, char* buf, size_t n)
{
	const mlsd_gemm_args *g = &op->u.gemm;
	snprintf(buf, n, "%dx%dx%d%s%s", g->M, g->N, g->K, g->C32 ? " f32" : "", g->resid ? "+res" : "");
}
static void attn_shape(const MLOp* op, char* buf, size_t n)
{
	const mlsd_attn_args *a = &op->u.attn;
	snprintf(buf, n, "b%d h%d d%d %dx%d", a->n_batch, a->n_head, a->d_head, a->Tq, a->Tk);
}
static void ln_shape(const MLOp* op, char* buf, size_t n) { snprintf(buf, n, "%dx%d", op->u.ln.rows, op->u.ln.d); }
static void gn_shape(const MLOp* op, char* buf, size_t n)
{
	const mlsd_gn_args *a = &op->u.gn;
	snprintf(buf, n, "n%d hw%d c%d+%d%s%s", a->n_img, a->HW, a->C1, a->C2, a->raw16 ? " +raw" : "", a->cs1 ? " stats" : "");   /* "stats": first pass replaced by the producers' column statistics */
}

/* ------------------------------------------------------------------ the table */
#define ARGS(m)      sizeof(((MLOp*)0)->u.m)
#define F(m, f)      offsetof(MLOp, u.m.f)
#define FIELDS(...)  { (int)(sizeof((size_t[]){ __VA_ARGS__ }) / sizeof(size_t)), { __VA_ARGS__ } }

const MLOpClass k_op_class[] = {
	[OP_GEMM] = { "gemm", ARGS(gemm), run_gemm, .outputs = gemm_outputs,
		.params = FIELDS(F(gemm, W_), F(gemm, bias), F(gemm, bias_m), F(gemm, ln_gamma), F(gemm, ln_beta),
		                 F(gemm, gn_gamma), F(gemm, gn_beta)),      /* (gn_*: a GroupNorm folded into the reduce pass, EXPERIMENTS builds) */
		.bytes = gemm_bytes, .shape = gemm_shape, .unnamed = gemm_unnamed,
		.fused_is_no_launch = 1 },                                   /* the Linear runs as the second GEMM of its producer's launch */
	[OP_ATTN] = { "attn", ARGS(attn), run_attn, .out = FIELDS(F(attn, out)), .bytes = attn_bytes, .shape = attn_shape },
	[OP_GN] = { "gn", ARGS(gn), run_gn, .out = FIELDS(F(gn, y16), F(gn, raw16)), .params = FIELDS(F(gn, gamma), F(gn, beta)),
		.bytes = gn_bytes, .shape = gn_shape, .fused_is_no_launch = 1 },
	[OP_LN] = { "ln", ARGS(ln), run_ln, .out = FIELDS(F(ln, y16), F(ln, y32)), .params = FIELDS(F(ln, g), F(ln, b)),
		.bytes = ln_bytes, .shape = ln_shape, .fused_is_no_launch = 1 },
	[OP_NCHW2NHWC] = { "n2h", ARGS(n2h), run_n2h, .out = FIELDS(F(n2h, dst)) },
	[OP_NHWC2NCHW] = { "h2n", ARGS(h2n), run_h2n, .out = FIELDS(F(h2n, dst)) },
	[OP_TEMB] = { "temb", ARGS(temb), run_temb, .out = FIELDS(F(temb, out)) },
	[OP_ACT] = { "act", ARGS(act), run_act, .out = FIELDS(F(act, y)), .bytes = act_bytes },
	[OP_CLIP_EMBED] = { "cemb", ARGS(cemb), run_cemb, .out = FIELDS(F(cemb, out)), .params = FIELDS(F(cemb, tw), F(cemb, pw)) },
	[OP_SOFTMAX] = { "smax", ARGS(smax), run_smax, .out = FIELDS(F(smax, out)), .bytes = smax_bytes },
	[OP_COPY_F32] = { "copy", ARGS(copy), run_copy, .out = FIELDS(F(copy, dst)), .bytes = copy_bytes },
	[OP_XA_VT] = { "xavt", ARGS(xavt), run_xavt, .out = FIELDS(F(xavt, vt)) },
	[OP_ATTN_CTX] = { "attn_ctx", ARGS(attn), run_attn_ctx, .out = FIELDS(F(attn, out)), .bytes = attn_bytes, .shape = attn_shape },
	[OP_CTRL_ADD] = { "cadd", ARGS(cadd), run_cadd, .out = FIELDS(F(cadd, dst)), .bytes = cadd_bytes },
	[OP_FREEU_BACKBONE] = { "freeu_backbone", ARGS(freeu), run_freeu_backbone, .out = FIELDS(F(freeu, dst), F(freeu, ws)), .bytes = freeu_bytes },
	[OP_FREEU_SKIP] = { "freeu_skip", ARGS(freeu), run_freeu_skip, .out = FIELDS(F(freeu, dst), F(freeu, ws)), .bytes = freeu_bytes },
};
_Static_assert(sizeof(k_op_class) / sizeof(k_op_class[0]) == OP_KIND_COUNT, "k_op_class: one entry per MLOpKind");

int mlop_outputs(const MLOp* op, const void* out[MLOP_MAX_OUTPUTS])
{
	const MLOpClass *k = &k_op_class[op->kind];
	if (k->outputs) return k->outputs(op, out);
	int n = 0;
	for (int q=0; q<k->out.n; ++q) {
		const void *p = *(void* const*)((const char*)op + k->out.off[q]);
		if (p) out[n++] = p;
	}
	return n;
}

MLB_API int mlctx_op_kind_info(int kind, const char** name, size_t* args_bytes)
{
	if (kind < 0 || kind >= OP_KIND_COUNT) return 0;
	if (name) *name = k_op_class[kind].name;
	if (args_bytes) *args_bytes = k_op_class[kind].args_bytes;
	return 1;
}

MLB_API int mlctx_op_kind_can_fuse(int kind) { return kind >= 0 && kind < OP_KIND_COUNT && k_op_class[kind].fused_is_no_launch; }
