/* mlsd_kernels.h — the thin C-ABI shim into the hand-written HIP kernels (gfx950).
 *
 * This is the layer that replaces the ggml op call sites of the reference's hot path
 * (SURVEY.md §2.3).  Plain pointers and sizes only; every pointer is a DEVICE pointer
 * unless stated otherwise; `stream` is a hipStream_t passed as void* (NULL = default).
 * Return convention: 0 = success (like ggml_status / ggml_backend_graph_compute,
 * reference src/mlblock.c:301-307), <0 = error with text in mlsd_last_error().
 *
 * Data layout (MI355X-first, differs from the reference on purpose):
 *   activations  : channels-last.  An image tensor [N,H,W,C] and a token tensor [N,T,C]
 *                  are the same memory, so the reference's permute/cont/reshape nodes
 *                  (src/unet.c:126-137, src/mlblock_nn.c:204-227) disappear.
 *                  Residual streams are fp32; GEMM/conv/attention operands are fp16
 *                  (ggml rounds activations to F16 before every F16-weight mul_mat/im2col,
 *                  SURVEY App. A), accumulation fp32 on MFMA.
 *   weights      : fp16 [n_out][K] row-major, K = n_in (linear) or (kh,kw,cin) with cin
 *                  fastest (conv; repacked from the reference's [cout][cin][kh][kw]).
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- runtime (replaces ggml_backend_*:
 * src/mlimgsynth.c:1131-1161, src/localtensor.h:96-106, src/mlblock.c:257) */
const char* mlsd_last_error(void);
const char* mlsd_peek_runtime_error(void);   /* diagnostics: HIP's pending error text (not cleared), "" if none */
/* dry mode: memory calls are served from host memory so the plan builder can run without a GPU; no kernel
 * can be launched (every launcher fails).  Used by the CPU-only tests of the host logic. */
void mlsd_runtime_dry(int on);
int mlsd_runtime_is_dry(void);
int mlsd_device_count(void);
int mlsd_device_set(int dev);
int mlsd_device_info(int dev, char* name, int name_len, char* arch, int arch_len, int* n_cu,
                     size_t* mem_total, size_t* mem_free);
int mlsd_malloc(void** out, size_t nbytes);
int mlsd_free(void* p);
int mlsd_host_alloc(void** out, size_t nbytes);      /* pinned host memory */
int mlsd_host_free(void* p);
int mlsd_memset(void* dst, int value, size_t nbytes, void* stream);
int mlsd_memcpy(void* dst, const void* src, size_t nbytes, int kind /*0 h2d,1 d2h,2 d2d*/, void* stream);
int mlsd_stream_create(void** out);
int mlsd_stream_create_masked(void** out, const uint32_t* cu_mask, int n_words);   /* kernels of this stream run on the masked CUs only */
int mlsd_cu_census(unsigned* out_dev, int n_blocks, int spin_cycles, void* stream); /* diagnostics: out[block] = (XCC id << 16) | HW_ID[15:0] */
int mlsd_stream_destroy(void* s);
int mlsd_stream_sync(void* s);
int mlsd_device_sync(void);
int mlsd_event_create(void** out);
int mlsd_event_destroy(void* e);
int mlsd_event_record(void* e, void* stream);
int mlsd_event_sync(void* e);
int mlsd_event_elapsed_ms(void* e0, void* e1, float* ms);
int mlsd_stream_wait_event(void* stream, void* e);
int mlsd_capture_begin(void* stream);
int mlsd_capture_end(void* stream, void** graph_exec);
int mlsd_graph_launch(void* graph_exec, void* stream);
int mlsd_graph_destroy(void* graph_exec);

/* ---------------------------------------------------------------- RCCL over xGMI (librccl opened lazily with dlopen)
 * The two exchange steps of the image-sharded multi-GPU job: broadcast of the conditioning, gather of the
 * results.  One communicator per process (one process per GPU); the 128-byte unique id from rank 0 reaches the other ranks by
 * any side channel of the launcher.  Buffers are device pointers; calls are asynchronous on `stream`. */
int mlsd_rccl_unique_id(void* out128);
int mlsd_rccl_init(void** comm, int world, int rank, const void* id128);
int mlsd_rccl_destroy(void* comm);
/* the same communicator interface over a HOST transport supplied by the launcher (gloo, MPI, ...): the engine's exchange entry
 * points (mlis_amd_bcast_cond / mlis_amd_gather_results) run unchanged; device buffers are staged through host memory (in the
 * dry runtime they already are host memory).  Callbacks return 0 on success. */
typedef int (*mlsd_host_bcast_fn)(void* user, void* buf, size_t nbytes, int root);
typedef int (*mlsd_host_allgather_fn)(void* user, const void* send, void* recv, size_t nbytes_per_rank);
int mlsd_comm_host(void** comm, int world, int rank, mlsd_host_bcast_fn bcast, mlsd_host_allgather_fn all_gather, void* user);
int mlsd_comm_count(void* comm, int* count, int* kind);   /* ranks as the transport reports them (ncclCommCount); kind: 0 = RCCL, 1 = host transport */
int mlsd_rccl_bcast(void* comm, void* buf, size_t nbytes, int root, void* stream);
int mlsd_rccl_all_gather(void* comm, const void* send, void* recv, size_t nbytes_per_rank, void* stream);

/* ---------------------------------------------------------------- GEMM / implicit-GEMM conv
 * Replaces ggml_mul_mat (+ggml_add bias) at src/mlblock_nn.c:22-25 and ggml_conv_2d (+bias) at
 * src/mlblock_nn.c:44-50, with the adjacent elementwise nodes fused as epilogues:
 *   time-embedding add  src/mlblock_nn.c:141-143     residual add  :154, :242,:247,:251, src/unet.c:143
 *   SiLU src/unet.c:153,159   GELU/quick-GELU src/clip.c:354-356   ReLU src/tae.c:30-37
 *   GEGLU (chunk+gelu+mul) src/mlblock_nn.c:164-169   nearest-2x upsample folded into the gather (:122)
 * C[M,N] = A[M,K] . W[N,K]^T, fp16 operands, fp32 accumulate (v_mfma_f32_32x32x16_f16).
 */
enum { MLSD_ACT_NONE = 0, MLSD_ACT_SILU = 1, MLSD_ACT_GELU = 2, MLSD_ACT_GELU_QUICK = 3, MLSD_ACT_RELU = 4,
       MLSD_ACT_GEGLU = 5 };

/* Tile variants of mlsd_gemm that the plan builder or the launcher name (the index in the launcher's variant table; mlsd_gemm_variant
 * prints the label in the comment).  The numbers never change: the tuning table, mlsd_gemm_force_variant and the tools that force
 * variants use them.  mlsd_gemm_args.tile_variant holds MLSD_TILE_ARG(v). */
enum {
	MLSD_TILE_128x128 = 0,          /* 128x128x64s2 */
	MLSD_TILE_64x128 = 1,           /* 64x128x64s2 */
	MLSD_TILE_256x128 = 3,          /* 256x128x64s2 */
	MLSD_TILE_256x128_S3 = 4,       /* 256x128x32s3 */
	MLSD_TILE_256x256 = 9,          /* 256x256x64s2w16 */
	MLSD_TILE_128x320 = 16,         /* 128x320x64s2 */
	MLSD_TILE_PP_256x256 = 17,      /* 256x256x64pp: ping-pong */
	MLSD_TILE_PP_128x320 = 18,      /* 128x320x64pp */
	MLSD_TILE_PPSK_256x256 = 19,    /* 256x256x64ppsk: stream-K */
	MLSD_TILE_PP2_128x320 = 20,     /* 128x320x64pp2: two phases per K tile */
	MLSD_TILE_PP2_256x256 = 21,     /* 256x256x64pp2 */
	MLSD_TILE_PPB_128x320 = 22,     /* 128x320x64ppb (EXPERIMENTS builds) */
	MLSD_TILE_PP2_256x128 = 25,     /* 256x128x64pp2 (EXPERIMENTS builds) */
	MLSD_TILE_W4_256x256 = 26,      /* 256x256x64w4 (EXPERIMENTS builds) */
	MLSD_TILE_W4_128x320 = 27,      /* 128x320x64w4 (EXPERIMENTS builds) */
	MLSD_TILE_PPSK_128x320 = 28,    /* 128x320x64ppsk */
	MLSD_TILE_SKINNY = 29,          /* skinny128x64: M <= 128 weight streaming */
	MLSD_TILE_TT = 30,              /* 128x160x64tt: two tiles in flight per CU */
	MLSD_TILE_CONV_SMALLN = 31      /* conv3x3n16: small-Cout streaming convolution */
};
#define MLSD_TILE_ARG(v) ((v) + 1)      /* mlsd_gemm_args.tile_variant that asks for tile variant v */

typedef struct mlsd_gemm_args {
	/* A operand: fp16 activations */
	const void* A;
	int64_t lda;            /* elements between consecutive rows (linear) / pixels (conv) */
	int conv;               /* 0: A is a plain [M][K] matrix; 1: implicit im2col over an NHWC image */
	int n_img, H, W, Cin;   /* conv: source image dims (before the optional 2x upsample) */
	int OH, OW;             /* conv: output dims; M must equal n_img*OH*OW */
	int KH, KW, stride, pad;
	int upsample;           /* conv: 1 = the conv reads nearest-2x-upsampled input (ggml_upscale + conv) */
	/* B operand: fp16 weights [N][ldb], K-contiguous */
	const void* W_;
	int64_t ldb;
	int M, N, K;            /* K % 8 == 0; conv: K = KH*KW*Cin */
	/* epilogue */
	const float* bias;      /* [N] or NULL */
	const float* rowbias;   /* [M/rows_per_batch][ldrb] added per batch element (time embedding) or NULL */
	int rows_per_batch;
	int64_t ldrb;
	const float* resid;     /* fp32 [M][ldr] residual added after activation, or NULL */
	int64_t ldr;
	int act;                /* MLSD_ACT_*; GEGLU: W rows interleaved in blocks of 32 (value,gate), output has N/2 columns */
	float* C32;             /* fp32 output [M][ldc32] or NULL */
	int64_t ldc32;
	void* C16;              /* fp16 output [M][ldc16] or NULL */
	int64_t ldc16;
	const float* bias_m;    /* [M] per-row bias (operands swapped: V^T = Wv . x^T in the VAE attention) or NULL */
	int act_after_resid;    /* 1: activation applied after the residual add (TAESD block: relu(conv + x), src/tae.c:36-37) */
	int tile_variant;       /* 0 = automatic choice; MLSD_TILE_ARG(k) = use tile variant k (set by the plan's autotuner) */
	/* split-K (small-M, long-K problems that cannot fill 256 CUs with output tiles: the SD1.5 batch-1 convs):
	 * ksplit > 1 slices K over gridDim.y, each slice writes fp32 partial sums to ws, a second kernel sums the
	 * slices in fixed order and applies the epilogue.  Ignored (no split) for GEGLU, when ws is NULL, or when
	 * N / the output strides are not multiples of 4. */
	int ksplit;
	void* ws;               /* >= mlsd_gemm_splitk_ws_bytes(M, N, ksplit) bytes, 16-byte aligned */
	size_t ws_bytes;
	/* column statistics of the fp32 output for a consuming GroupNorm (its first pass disappears): per block of
	 * mlsd_gemm_colstats_rows(args) consecutive rows and per column the sum and the sum of squares of C32, written as
	 * colstats[block][0][n] and colstats[block][1][n] (floats, 2*N per block); with colstats_shift (below) the sums of
	 * (x - K) and (x - K)^2 instead.  Only the launches for which mlsd_gemm_colstats_rows() > 0 honour it (ping-pong tiles,
	 * fp32 output without activation); NULL = off. */
	float* colstats;
	int colstats_rows;      /* > 0: the consumer was wired for statistics blocks of this many rows: mlsd_gemm FAILS unless this
	                         * launch writes exactly those (a tile / epilogue knob changed between planning and launching) */
	/* 4096 zeroed 32-bit words that stay zero between launches (the kernels that use them clear them again):
	 *  - stream-K (tile variant 19): a flag per persistent block beside the workspace `ws` (>= 256 fp32 slabs of 256 x 256:
	 *    mlsd_gemm_streamk_ws_bytes()).  NULL: the launch runs as variant 17.
	 *  - split-K (ksplit > 1): a ticket counter per output tile; the slices are then added inside the launch (no second launch).
	 *    NULL, or more than 4096 tiles: the two-launch form. */
	unsigned* sk_flags;
	/* LayerNorm at the END of the launch (round 3): when ln_y16 is set and mlsd_gemm_ln_fused(args) says so, the launch also writes
	 * ln_y16[m][n] = fp16(LayerNorm(C32 row m) * ln_gamma + ln_beta) (row stride ldln halfs, eps ln_eps): the LayerNorm that would follow
	 * (ggml_norm + mul + add, src/mlblock_nn.c:65-71) needs no launch of its own.  Linear launches on the 128x320 ping-pong tile (or the 128x160 tile) whose tiles are all
	 * resident at once (M % 128 == 0, N % 320 == 0, (M/128)(N/320) <= 256), fp32 output (+ residual), at most 8 column tiles per row block.  The column tiles of a row
	 * block exchange their row statistics inside the launch as self-tagged records (round 6: no counters, nothing to reset): ln_ws = scratch OF THIS LAUNCH'S OWN
	 * (zeroed once, never shared with another launch: >= M * (N / tile columns) * 16 bytes -- 16 bytes per row and column tile); ln_cnt = a block of 8192 32-bit words
	 * zeroed once and NEVER shared between two ops or shapes (a tile takes the tag of its records from its own record of the op's previous launch); ln_cnt word 8191 = sticky give-up indicator like sk_flags[4095] (ln_slot: unused since the records carry their generation).
	 * mlsd_gemm FAILS when ln_y16 is set and the launch cannot honour it. */
	void* ln_y16; int64_t ldln;
	const float *ln_gamma, *ln_beta;
	float ln_eps;
	float* ln_ws;
	unsigned* ln_cnt;
	int ln_slot;
	/* GroupNorm at the END of a split-K launch's reduce pass (round 4; mlsd_gemm_gn_fused): when gn_y16 is set and the launch qualifies -- general tile, ksplit > 1, fp32
	 * output, N % gn_groups == 0 with N / gn_groups a multiple of 4, an (image, group) slab of gn_hw * N / gn_groups <= 10240 values -- the reduce pass runs one block
	 * per (image, group): slices added in slice order + the epilogue (C32 bit-identical to splitk_reduce), then
	 * gn_y16[m][n] = fp16(silu?((C32 - mean) rstd gn_gamma[n] + gn_beta[n])), statistics over the gn_hw rows of the image and the group's columns
	 * (ggml_group_norm + mul + add [+ silu], src/mlblock_nn.c:86-99,135-136).  M must be a multiple of gn_hw.  mlsd_gemm FAILS when gn_y16 is set and the launch cannot honour it. */
	void* gn_y16; int64_t gn_ldy;
	const float *gn_gamma, *gn_beta;
	float gn_eps;
	int gn_groups, gn_hw, gn_silu;
	/* CROSS ATTENTION at the end of its q projection (round 6; the 128 x 320 ping-pong tile = 128 query rows x 5 heads of 64).  When xa_k is set and
	 * mlsd_gemm_xattn_fused(args) == 1 the launch does NOT store the projection: a tile's q (rounded to fp16 exactly as the unfused launch's C16 would hold it) stays in LDS
	 * and the launch ends with  xa_out[m][64 h + d] = fp16( softmax_key( q_h[m] . K_h[key] / sqrt(64) ) . V_h )  over the xa_Tk <= 80 keys of row m's image -- what
	 * mlb_nn_linear (q_proj) + ggml_nn_attention compute at src/mlblock_nn.c:200-223, src/ggml_extend.c:200-222 for the text context (77 keys).  One dispatch and one
	 * round trip of q through HBM fewer per cross attention (70 per SDXL evaluation).  Operands: xa_k = K [n_img * xa_Tk][xa_ldk] fp16 (key r of image b in row
	 * b * xa_Tk + r; the N columns are the projection's: head h = columns 64 h ..); xa_vt = V TRANSPOSED and zero padded, [n_img][N][96] fp16 (mlsd_xattn_pack_vt, run
	 * once per conditioning); xa_Tq = query rows per image (a multiple of 128: a tile never straddles two images).  Needs N % 320 == 0, M % 128 == 0, fp16 arithmetic
	 * as the unfused pair (fp16 q, K, V, P; fp32 accumulation and softmax).  mlsd_gemm FAILS when xa_k is set and the launch cannot honour it. */
	const void* xa_k; int64_t xa_ldk;
	const void* xa_vt;
	void* xa_out; int64_t xa_ldo;
	int xa_Tq, xa_Tk;
	/* conv, PHASE FORM of an upsampling convolution (the ping-pong tiles only; every other kernel refuses them; 0 = off).  A 3x3 convolution over a nearest-2x
	 * upsampled H x W source equals four 2x2 convolutions over the SOURCE, one per output parity (py, px), with the weights mlsd_ups_phase_weights derives:
	 *   tap_oy / tap_ox  moves the tap window along its axis: tap (kh, kw) of output pixel (oh, ow) reads source pixel (oh stride - pad + tap_oy + kh, ow stride - pad
	 *                    + tap_ox + kw), bounds-checked or wrapped like any tap.  A phase launch: KH = KW = 2, stride 1, pad 1, tap_oy = py, tap_ox = px, OH = H, OW = W.
	 *   out_phase        1 + 2 py + px: row (n, y, x) of the launch is stored at pixel (2 y + py, 2 x + px) of a [n][2 OH][2 OW] image whose pixels are ldc32 floats apart
	 *                    (C32 = that image; fp32 output, bias or none, nothing else in the epilogue).  Needs OW % 16 == 0: a 16-row block of the epilogue lies in one
	 *                    image row.  The four launches write disjoint pixels and need no order among themselves.
	 * (These three stand before colstats_shift and wrap, which tests/test_tiling_cpu.py pins as the record's last two fields.) */
	int tap_oy, tap_ox;
	int out_phase;
	/* 1: colstats holds SHIFTED sums, sum (x - K) and sum (x - K)^2 with K = C32[first row of the block][n], which the consuming
	 * GroupNorm reads back from C32 (mlsd_gn_args.cs_shifted).  0: the plain sums of x and x^2.  Plain fp32 sums of squares lose
	 * ~2^-24 sqrt(rows) r^2 of a group's variance (r = |mean| / std: percents at r = 300), which no later double arithmetic recovers;
	 * the plan builder always asks for 1, 0 keeps the meaning the field had for callers that do not set it. */
	int colstats_shift;
	/* conv: circular padding (seamless tiling).  Bit 0 wraps columns, bit 1 rows: a tap outside the (upsampled) source image reads the pixel at
	 * that coordinate modulo the extent, in the same image, instead of zero.  Needs pad <= the extent of each wrapped axis (one fold); mlsd_gemm
	 * fails otherwise.  A launch none of whose taps can leave the image runs exactly as with 0. */
	int wrap;
} mlsd_gemm_args;

int mlsd_gemm(const mlsd_gemm_args* a, void* stream);
/* The phase weights of an upsampling 3x3 convolution: src fp16 [cout][3][3][cin] (cin = the padded channel count of the weight's rows) ->
 * dst fp16 [4][cout][2][2][cin], phase = 2 py + px, dst[phase][o][a][b][c] = fp16_rne( fp32 sum over kh in S(py, a), kw in S(px, b), ascending (kh, kw), of src[o][kh][kw][c] )
 * with S(0, 0) = {0}, S(0, 1) = {1, 2}, S(1, 0) = {0, 1}, S(1, 1) = {2}: the taps of one axis that land on the same source pixel. */
int mlsd_ups_phase_weights(const void* src, void* dst, int cout, int cin, void* stream);
int mlsd_ups_phase_weights_host(const void* src, void* dst, int cout, int cin);      /* the same rule on host memory (the master copy of a weight-streaming plan) */
/* The index maps of a convolution launch without the upsample in its gather, restated on the host (tests): the source pixel (n H + ih) W + iw that tap (kh, kw) of
 * row m reads, -1 where it reads a zero; and the pixel of the output that row m is stored at (out_phase: of the [n][2 OH][2 OW] image).  -2: bad arguments. */
long mlsd_conv_tap_source(const mlsd_gemm_args* a, int m, int kh, int kw);
long mlsd_conv_out_pixel(const mlsd_gemm_args* a, int m);
/* Phase form of the upsampling convolutions in the plans built from now on (mlb_upsample): -1 = where it wins (W % 16 == 0, enough rows), 0 = never,
 * 2 = wherever the kernels take it (A/B and tests).  Default: MLSD_UPS_PHASES from the environment, else -1. */
int mlsd_gemm_phase_form(const mlsd_gemm_args* a);      /* 1 if a launch with these phase fields runs, 0 if mlsd_gemm would refuse it */
void mlsd_gemm_set_ups_phases(int mode);
int mlsd_gemm_ups_phases(void);
/* rows per statistics block (64 or 128) if this launch would write a->colstats, 0 if its kernel cannot */
int mlsd_gemm_colstats_rows(const mlsd_gemm_args* a);
/* != 0 if this launch (ln_* fields set) ends with the LayerNorm of its output (see mlsd_gemm_args.ln_y16): 1 = inside the launch, the tiles of a row block exchanging their
 * row statistics (128x320 ping-pong tile; an in-launch hand-off); 2 = in the reduce pass of a split-K launch (one block per finished row: no hand-off; ln_ws / ln_cnt unused) */
int mlsd_gemm_ln_fused(const mlsd_gemm_args* a);
/* 1 if this launch (xa_* fields set) ends with the cross attention of the q it projects: see mlsd_gemm_args.xa_k.  MLSD_XATTN=0 in the environment answers 0 (A/B). */
int mlsd_gemm_xattn_fused(const mlsd_gemm_args* a);
/* 0 = never, 1 = where the fused launch wins (128 x 320 tiles on more than half of the CUs: the default), 2 = wherever the kernel takes the launch (A/B, kernel tests); other: back to MLSD_XATTN */
void mlsd_gemm_set_xattn(int mode);
/* vt[b][n][key] = v[b * Tk + key][n] for key < Tk, 0 for Tk <= key < 96: the V operand of the fused launch (fp16; v row stride ldv halfs; N columns; Tk <= 96) */
int mlsd_xattn_pack_vt(const void* v, int64_t ldv, int n_img, int Tk, int N, void* vt, void* stream);
/* name of the kernel variant mlsd_gemm would pick for these args (for profiling reports) */
/* 1 if this launch (gn_* fields set) ends its split-K reduce pass with the GroupNorm of its output (see mlsd_gemm_args.gn_y16) */
int mlsd_gemm_gn_fused(const mlsd_gemm_args* a);
const char* mlsd_gemm_variant(const mlsd_gemm_args* a);
/* What mlsd_gemm would run for these args, in one answer (the queries above read the same decision) */
typedef struct mlsd_gemm_route_info {
	int variant;            /* tile variant that launches, after every fall-back */
	int asked;              /* 1 if that is the tile the launch asked for (forced variant, shape rule, tile_variant or the static choice) */
	int nsplit;             /* K slices over the grid (1: none) */
	int stats_rows;         /* as mlsd_gemm_colstats_rows */
	int ln;                 /* as mlsd_gemm_ln_fused */
	int gn;                 /* as mlsd_gemm_gn_fused */
	int xattn;              /* as mlsd_gemm_xattn_fused */
	int handoff;            /* 1 if blocks of the launch wait for other blocks of the same launch (stream-K, LayerNorm ending, split-K added in the launch) */
	int stats_rows_if;      /* stats_rows if the args asked for column statistics (colstats set) */
	int ln_if;              /* ln if a LayerNorm were attached (ln_* fields set) */
	size_t ln_ws_bytes_if;  /* the ln_ws scratch that ending needs (0: none) */
} mlsd_gemm_route_info;
int mlsd_gemm_route(const mlsd_gemm_args* a, mlsd_gemm_route_info* out);     /* 0, or -1 for a NULL argument */
/* tile order inside an XCD's range: column panels `mode` tiles wide (default 8; 0 = row-major).  A/B timing knob. */
void mlsd_gemm_set_panel(int width);
void mlsd_gemm_set_mode(int mode);     /* older name of mlsd_gemm_set_panel */
/* diagnostics: force a tile variant (-1 = automatic choice) / the scalar epilogue (1) instead of the wide one (0) */
void mlsd_gemm_force_variant(int v);
int mlsd_gemm_num_variants(void);
void mlsd_gemm_set_epilogue(int e);
/* timing-only builds of the main loop (needs -DMLSD_GEMM_EXPERIMENTS; otherwise ignored) */
void mlsd_gemm_set_debug(int d);
/* 1: split-K launches that were given ticket counters (mlsd_gemm_args.sk_flags) add their K slices INSIDE the launch (the block that
 * finishes a tile last sums the slabs in slice order and runs the epilogue: bit-identical to the two-launch form).  Default 0: the
 * two-launch form measured faster on MI355X (profiles/r3_gemm_splitk_inline.txt) */
void mlsd_gemm_set_splitk_inline(int on);
/* split-K launches (ksplit > 1, ticket counters in sk_flags) on the 64x128 / 128x128 tiles add their K slices INSIDE the launch, all blocks of a tile sharing the work
 * (round 4; bit-identical to the two-launch form).  Measured SLOWER than the second launch (a dispatch boundary is the cheaper grid-wide barrier on MI355X): only in
 * builds with EXPERIMENTS=1, and off unless switched on here / by MLSD_SPLITK_PAR=1. */
void mlsd_gemm_set_splitk_parallel(int on);
int mlsd_gemm_splitk_parallel(const mlsd_gemm_args* a);   /* 1 if this launch would do so (an in-launch hand-off: mlctx_handoff_check covers it) */
/* != 0 if mlsd_gemm runs this launch on the small-Cout streaming convolution (tile variant 31, conv_smalln.hip): 3x3, stride 1, pad 1, Cout <= 16, Cin 64 / 128, fp32 output + bias --
 * the KL-VAE decoder's conv_out (src/vae.c:163-165) and TAESD's last layer (src/tae.c:88-89).  MLSD_CONV_SMALLN=0 in the environment keeps the implicit-GEMM tile (A/B). */
int mlsd_conv_smalln_eligible(const mlsd_gemm_args* a);
void mlsd_conv_smalln_set(int ring_rows, int strip_rows);   /* diagnostics: input-row ring depth (4..6) and strip height of the next launches */
size_t mlsd_gemm_streamk_ws_bytes(void);   /* workspace of a stream-K launch (slabs); the flags are 256 x 4 bytes, zeroed once */
void mlsd_gemm_set_cus(int n);      /* CUs a persistent GEMM launch occupies (default 256; 128 for half-chip partitions) */
void mlsd_gemm_set_trace(void* buf);        /* diagnostics: device buffer of 256 x 8 uint64 cycle stamps filled by the ping-pong kernels (NULL = off) */
size_t mlsd_gemm_splitk_ws_bytes(int M, int N, int ksplit);

/* ---------------------------------------------------------------- fused attention
 * Replaces ggml_nn_attention (src/ggml_extend.c:200-222: mul_mat, scale, [diag_mask_inf], soft_max,
 * mul_mat with materialised scores) and the head split/merge permutes around it
 * (src/mlblock_nn.c:204-227).  Flash-style: online softmax, scores never leave the CU.
 * q [n_batch][Tq][ldq], k/v [n_batch][Tk][ldk/ldv] fp16 with head h at column h*d_head; out fp16
 * [n_batch][Tq][ldo], heads merged.  d_head in {40,64,80,160} (any multiple of 8 up to 160). */
typedef struct mlsd_attn_args {
	const void *q, *k, *v;
	void* out;
	int64_t ldq, ldk, ldv, ldo;          /* row strides in elements */
	int64_t bsq, bsk, bsv, bso;          /* batch strides in elements */
	int n_batch, n_head, d_head, Tq, Tk;
	int causal;                           /* 1: key index > query index masked (CLIP, src/clip.c:407-408) */
} mlsd_attn_args;

int mlsd_attention(const mlsd_attn_args* a, void* stream);
/* The same attention over 96 < Tk <= 320 keys (cross attention of a windowed text context, 77 x W rows), no causal mask, d_head in
 * {32,40,64,80,160}: groups of up to 96 keys in one pass each, merged by an online softmax (attn_ctx_kernel).  q, k, v 16-byte aligned with
 * ldq / ldk / ldv and their batch strides multiples of 8; out 8-byte aligned with ldo and bso multiples of 4.
 * Outside that range: an error.  mlsd_attention's dispatch is not affected. */
int mlsd_attention_ctx(const mlsd_attn_args* a, void* stream);
/* The kernel instantiation mlsd_attention (ctx = 0) or mlsd_attention_ctx (ctx = 1) would launch for these arguments under the current switches, from the
 * route the launch itself switches on; NULL where the launch would refuse (mlsd_gemm_variant's counterpart; the string is valid until the thread's next call):
 *   attn<tile,dD[,causal][,mfmasum]>   attn_kernel<D>, the 64-key tile loop (mfmasum: mlsd_attention_vsum(0))
 *   attn<tk96,dD[,w4]>                 attn_tk96_kernel<D>, Tk <= 96 in one pass (w4: mlsd_attention_tk96(2, .))
 *   attn<64x2[,mfmasum]>               attn64x2_kernel, d_head 64, 64 query rows per wave
 *   attn<64x2s,dD>                     attn64x2s_kernel<D>, software-pipelined, D = 64 or 40
 *   attn<ctx,dD,resident|slot>         attn_ctx_kernel<D>, 96 < Tk <= 320
 *   attn<pp,Rrows,wW>                  attn64pp_kernel (EXPERIMENTS builds), R query rows per wave */
const char* mlsd_attention_variant(const mlsd_attn_args* a, int ctx);
int mlsd_attention_ctx_takes(const mlsd_attn_args* a);   /* 1 where the plan runs a Tk > 96 cross attention on mlsd_attention_ctx (measured not slower than mlsd_attention) */
void mlsd_attention_ctx_mode(int mode);    /* A-B timing: 0 (default) = keys resident in LDS where they take <= 64 KiB, else one 96-key slot restaged per group; 1 = the slot always */
/* diagnostics / A-B timing: 1 = the d_head 64 problems also run on the general kernel instead of the 64-rows-per-wave one */
void mlsd_attention_force_old(int on);
void mlsd_attention_x2_min_tq(int tq);     /* smallest Tq (multiple of 256) the 64-rows-per-wave kernel takes (default 2048) */
void mlsd_attention_sp(int mode);          /* d_head 64 or 40, no mask, Tq % 256 == 0, Tk % 64 == 0 and >= 128: 1 (default) = from Tq = 768 on, when the launch has at least 128 blocks of 256 rows, the software-pipelined kernel (attn64x2s_kernel, round 6: Q pre-scaled in fp16), 2 = from Tq = 256 on (kernel tests), 0 = the tile-loop kernels (A/B) */
void mlsd_attention_pp(int mode);          /* d_head 64 ping-pong kernel: 0 off, 1 by shape (default), 2 always 32 rows per wave, 3 always 64, 4 = 32 rows with one block per CU; + 16 / 32: s_setprio 1 around the MFMA clusters / the vector phase (A-B timing) */
void mlsd_attention_tk96(int on, int qb);  /* Tk <= 96 one-pass kernel on/off (A-B timing); qb = 128-row query blocks per workgroup, 0 = automatic */
void mlsd_attention_wide_stores(int on);  /* diagnostics / A-B timing: 0 = the output in 8-byte pieces per lane */
void mlsd_attention_vsum(int on);         /* diagnostics / A-B timing: 1 = row sums of the 64-rows-per-wave kernel on the VALU instead of ones.P MFMAs */

/* row softmax over fp32 scores -> fp16 probabilities (VAE mid attention, d=512 single head,
 * src/vae.c:46-74, computed as GEMM + softmax + GEMM).  in [rows][ld_in] f32, out [rows][ld_out] f16 */
int mlsd_softmax_rows(const float* in, int64_t ld_in, void* out, int64_t ld_out, int rows, int cols,
                      float scale, void* stream);

/* ---------------------------------------------------------------- normalisation
 * GroupNorm: ggml_group_norm + mul + add (+ silu) at src/mlblock_nn.c:86-99,135-136,146-147.
 * Two fp32 sources (x1 with C1 channels, x2 with C2 channels, either row-strided) give the
 * channel concat of src/unet.c:233 for free.  Output fp16 [n_img][HW][C1+C2]; optional raw fp16 copy
 * of the (concatenated) input for the 1x1 skip conv. `ws` = workspace of mlsd_groupnorm_ws_bytes(). */
typedef struct mlsd_gn_args {
	const float *x1, *x2;
	int64_t ld1, ld2;                     /* pixel strides in elements */
	int C1, C2;                           /* C2 = 0 if no second source */
	int n_img, HW, n_grp;
	float eps;
	const float *gamma, *beta;            /* [C1+C2] */
	int silu;
	void* y16;                            /* fp16 [n_img][HW][C1+C2] */
	void* raw16;                          /* optional fp16 copy of the un-normalised input, or NULL */
	void* ws;
	/* statistics written by the producing GEMMs (mlsd_gemm_args.colstats, [rows / rb_rows][2][C_i]) instead of the first pass
	 * over x: used when every source has them (rb_rows_i > 0) and HW is a multiple of rb_rows_i */
	const float *cs1, *cs2;
	int rb_rows1, rb_rows2;
	int cs_shifted;                       /* 1: cs1 / cs2 were written with mlsd_gemm_args.colstats_shift = 1; x_i must then be the C32
	                                       * they were written with (the finalize reads each block's shift back from it) */
} mlsd_gn_args;

size_t mlsd_groupnorm_ws_bytes(int n_img, int HW, int n_grp);
int mlsd_groupnorm(const mlsd_gn_args* a, void* stream);
/* 1 if these dimensions run as ONE dispatch (small maps: the (image, group) slab is held in registers; SD1.5 batch 1 is bound by its dispatch count) */
int mlsd_groupnorm_single_pass(int n_img, int HW, int C, int n_grp);
void mlsd_groupnorm_set_single(int on);     /* diagnostics / A-B timing: 0 = always the two-kernel form */
void mlsd_groupnorm_set_finalize2(int on);  /* diagnostics / A-B timing: 0 = the one-level finalize of the producers' statistics also on large maps */

/* LayerNorm over the last dim: ggml_norm + mul + add at src/mlblock_nn.c:65-71.  x fp32 [rows][ldx] ->
 * y fp16 [rows][d] (and/or y32 fp32 [rows][d]) */
int mlsd_layernorm(const float* x, int64_t ldx, int rows, int d, float eps, const float* gamma,
                   const float* beta, void* y16, float* y32, void* stream);
void mlsd_layernorm_stream_blocks(int n);   /* diagnostics / A-B timing: blocks of the streaming form (default 1024), 0 = one row per wave */

/* ---------------------------------------------------------------- small ops */
/* NCHW fp32 [n_src][C][HW] -> NHWC fp16 [n_dst][HW][Cpad] (channels >= C zero-filled);
 * dst image n reads src image n % n_src (cond/uncond duplication of src/mlimgsynth.c:1578-1582);
 * value = f(src * scale[n % n_src]) with scale NULL -> scalar `scale0`
 * (c_in of src/unet.c:470-472; 1/scale_factor of src/vae.c:174);
 * mode 1: 3*tanh(x/3) clamp of src/tae.c:71-73 applied first; mode 2: x*2-1 (sdvae_encoder_pre, src/vae.h:36-40) applied first. */
int mlsd_nchw_to_nhwc_f16(const float* src, int n_src, int C, int HW, void* dst, int n_dst, int Cpad,
                          const float* scale, float scale0, int mode, void* stream);
/* NHWC fp32 [n][HW][ld] (first C channels) -> NCHW fp32 [n][C][HW]; out = in*mul + add
 * ((x+1)/2 of src/vae.h:43-47) */
int mlsd_nhwc_to_nchw_f32(const float* src, int64_t ld, int n, int C, int HW, float* dst, float mul, float add,
                          void* stream);
/* ggml_timestep_embedding(t, dim, 10000) (src/unet.c:150): t fp32 [n] -> fp16 [n][dim] (cos | sin) */
int mlsd_timestep_embedding(const float* t, int n, int dim, float max_period, void* out16, void* stream);
/* y16 = act(x32) elementwise (silu of the embedding, src/mlblock_nn.c:140) */
int mlsd_act_f32_to_f16(const float* x, void* y16, size_t n, int act, void* stream);
/* ggml_get_rows + position add (src/clip.c:337-342): tokens int32 [n][T] -> x fp32 [n][T][d] */
int mlsd_clip_embed(const int32_t* tokens, int n, int T, int d, const void* tok_w16, const float* pos_w,
                    float* out, void* stream);
/* Euler(-ancestral) update with CFG mix on device (src/mlimgsynth.c:1583, src/solvers.c:86,
 * src/sampling.c:170-174):  x[b] += (eps_c*f + eps_u*(1-f)) * dt[b] + noise[b]*s_up[b]
 * x, noise: NCHW fp32 [B][C][HW]; eps: NHWC fp32 [2B][HW][ld] (cond rows 0..B-1, uncond B..2B-1;
 * f<=1: only cond is read).  dt, s_up: fp32 [B] on device. noise may be NULL. */
int mlsd_sampler_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg,
                        const float* dt, const float* noise, const float* s_up, void* stream);
/* dnsamp_noise_add (src/sampling.c:112-117): x[b] += noise[b] * s[b]; x, noise fp32 [B][per], s fp32 [B] on device */
int mlsd_noise_add(float* x, const float* noise, const float* s, int B, int64_t per, void* stream);
/* ---- general sampler (all solvers / in-painting / img2img / v-prediction): one launch per loop of the reference, same
 * fp32/fp64 operation order (bit-identical to the host arithmetic).  x, dx, tmp vectors: NCHW fp32 [B][C][HW], n = B*C*HW.
 * Scalars by value (they are wave-uniform kernel arguments: nothing to upload or sync). */
/* The guidance mix (csrc/hip/guidance.hip): the guided prediction of one evaluation, from the UNet output eps NHWC [N][HW][ld] with the row groups
 * [cond B | uncond B (only at cfg > 1) | perturbed B (only read at pag != 0)].  Classifier-free guidance is src/mlimgsynth.c:1565-1587; perturbed-attention guidance
 * ("Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance", 2024) and guidance rescale ("Common Diffusion Noise Schedules and Sample Steps are Flawed",
 * 2023, Algorithm 2) are not in the reference.  Per element, every operation rounded once:
 *   guided(c, u, p):  g = c;   cfg > 1: g = fadd(fmul(c, cfg), fmul(u, 1 - cfg));   pag != 0: g = fadd(g, fmul(pag, fsub(c, p)))
 *   v(e) = vparam ? fadd(fmul(e, c_out), fmul(x_eval, c_skip)) : e                                                          (src/unet.c:490-494)
 *   factor == NULL:  dx = guided(v(c), v(u), v(p))            -- the v map on each group, then the mix
 *   factor != NULL:  dx = v(fmul(guided(c, u, p), factor[b])) -- the mix of the RAW outputs, the rescale, then the v map once (other arithmetic, on purpose)
 * Rows a launch does not need (uncond at cfg <= 1, perturbed at pag == 0) are never read.  cfg, pag and the scalars go by value (wave-uniform): they change between
 * launches, and under a captured evaluation, without anything being rebuilt; factor is a device pointer to B floats.
 * Forms, all of the same bytes: C == 4, ld % 4 == 0 and eps 16-byte aligned: a thread owns pixels, one 16-byte load per group row -- four pixels where HW % 4 == 0
 * and x, out and noise are 16-byte aligned, else one; everything else: element by element.  ld = 4 (the tiled canvas) and the plan's padded stride alike.
 * euler_guided_update: the fused Euler(-ancestral) step (eps models: no v map), x updated in place: fadd(x, fmul(dx, dt)), then fadd(., fmul(noise, s_up)) where
 * noise is given -- dxdt_guided + mlsd_vec_axpy + mlsd_noise_add_s bit for bit (src/solvers.c:86, src/sampling.c:170-174).
 * Refused before any launch, by every entry below: a NULL eps, dx or x (x_eval may be NULL without vparam), B, C or HW below 1, ld < C, pag < 0 or NaN, cfg NaN,
 * 2^31 elements or more.  (The two *_cfg entries launched unchecked, and the two *_pag entries took a NaN cfg, before the mix was stated once.) */
int mlsd_dxdt_guided(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg, float pag, const float* factor /* NULL: no rescale */,
                     int vparam, float c_out, float c_skip, void* stream);
int mlsd_euler_guided_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, const float* factor, float dt,
                             const float* noise, float s_up, void* stream);
/* the narrow names: the general entries with some arguments fixed; error texts name the entry that was called */
int mlsd_dxdt_cfg(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg,
                  int vparam, float c_out, float c_skip, void* stream);                                                   /* pag 0, factor NULL */
int mlsd_euler_cfg_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float dt,
                          const float* noise, float s_up, void* stream);                                                  /* pag 0, factor NULL */
int mlsd_dxdt_pag(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg, float pag,
                  int vparam, float c_out, float c_skip, void* stream);                                                   /* factor NULL */
int mlsd_euler_pag_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, float dt,
                          const float* noise, float s_up, void* stream);                                                  /* factor NULL */
int mlsd_dxdt_rescaled(const float* eps, int64_t ld, const float* x_eval, float* dx, int B, int C, int HW, float cfg, float pag,
                       const float* factor, int vparam, float c_out, float c_skip, void* stream);                         /* a NULL factor is refused */
int mlsd_euler_rescaled_update(float* x, const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, const float* factor, float dt,
                               const float* noise, float s_up, void* stream);                                             /* a NULL factor is refused */
/* The factor of the guidance rescale, per image b over its n = C*HW elements, c, u, p the RAW outputs of the groups (a v model's own prediction, before the v map):
 *   f = phi*sqrt(M2(c) / M2(guided(c, u, p))) + (1 - phi),  M2 the sum of squared deviations from the mean (the n - 1 of the standard deviations cancels); formed in
 *       double, rounded once to float; 1 where M2(g) is zero or not finite, where n == 1, and where g is c (cfg <= 1 and pag == 0: the statistics are not launched)
 * guidance_stats writes factor[b] (device, B floats): one launch of (mlsd_guidance_blocks(HW), B) blocks -- a rule of HW alone -- that accumulate sums and sums of
 * squares in double (lanes, then waves, then LDS; each block stores four doubles to scratch[b][block][4]), one launch that sums an image's partials in block order.  No
 * atomics and no block waits on another, so the factors are the same bits on every run.  scratch: mlsd_guidance_scratch_bytes(B, HW) bytes (at most
 * B * MLSD_GUIDANCE_MAX_BLOCKS * 32), 8-byte aligned.  A rescaled mix is three launches: these two and the mix.
 * Refused before any launch: what the mix entries refuse, a NULL scratch or factor, phi outside 0 .. 1 or NaN, a scratch smaller than mlsd_guidance_scratch_bytes. */
#define MLSD_GUIDANCE_MAX_BLOCKS 64
int    mlsd_guidance_blocks(int HW);
size_t mlsd_guidance_scratch_bytes(int B, int HW);
int mlsd_guidance_stats(const float* eps, int64_t ld, int B, int C, int HW, float cfg, float pag, float phi, double* scratch, size_t scratch_bytes,
                        float* factor, void* stream);
int mlsd_vec_axpy(float* out, const float* x, const float* d, float dt, int64_t n, void* stream);     /* out = x + d*dt (solvers.c:86,105,278) */
int mlsd_solver_heun_corr(float* x, const float* dx, const float* d1, float dt, int64_t n, void* stream);   /* solvers.c:112-113 */
int mlsd_solver_taylor3(float* x, const float* dx, float* dp1, float* dp2, float dt, float idtp, float f2, float f3,
                        int64_t n, void* stream);                                                            /* solvers.c:150-165 */
int mlsd_solver_dpmpp2m(float* x, const float* dx, float* dprev, float t_cur, float a, float c, int64_t n, void* stream);   /* :222-229 */
int mlsd_solver_dpmpp2s(float* x, const float* x1, const float* dx1, float t1, float a, int64_t n, void* stream);           /* :281-284 */
int mlsd_fill2_f32(float* a, int na, float va, float* b, int nb, float vb, void* stream);   /* a[0..na) = va, b[0..nb) = vb from kernel arguments (per-evaluation scalars: no copy-engine job) */
int mlsd_noise_add_s(float* x, const float* noise, float s, int64_t n, void* stream);                /* sampling.c:115, scalar sigma */
int mlsd_mask_apply(float* x, const float* x0, const float* mask /*[HW]*/, int HW, int64_t n, void* stream);   /* sampling.c:98-110 */
/* sdvae_latent_sample / sdvae_latent_mean (src/vae.c:188-229): moments NHWC fp32 [B][HW][ld] (mean | logvar) -> latent NCHW
 * [B][cz][HW]; rnd NCHW [B][cz][HW] or NULL (mean only) */
int mlsd_latent_sample(const float* moments, int64_t ld, const float* rnd, float* latent, int B, int cz, int HW, float scale,
                       void* stream);
int mlsd_latent_sample_nchw(const float* moments /* NCHW [B][2cz][HW] */, const float* rnd, float* latent, int B, int cz, int HW,
                            float scale, void* stream);
/* ltensor_copy_slice2 (src/localtensor.h:84-94; VAE tiling, src/vae.c:283-297,368-382) on NCHW fp32 [planes][h][w] tensors */
int mlsd_copy_slice2(float* dst, int dw, int dh, const float* src, int sw, int sh, int n0, int n1, int di0, int di1,
                     int si0, int si1, int planes, void* stream);
/* Resampling of NCHW fp32 planes [planes][sh][sw] -> [planes][dh][dw] (the latent upscaler of the two-pass "hires fix"; not in the reference).
 * Pixel centres: output pixel d samples the source at (d + 0.5) s_in / s_out - 0.5 on each axis (torch's F.interpolate(align_corners=False)
 * for nearest-exact / bilinear / bicubic, no antialiasing).  The tap index and the fractional position come from the exact integer quotient
 * and remainder of ((2 d + 1) s_in - s_out) / (2 s_out); weights and sums are fp32 (tap weights first along the row, then the rows).
 *   MLSD_RESAMPLE_NEAREST   index floor((d + 0.5) s_in / s_out)
 *   MLSD_RESAMPLE_BILINEAR  2 x 2 taps
 *   MLSD_RESAMPLE_BICUBIC   4 x 4 taps, Keys kernel with a = -0.75
 * A tap index outside the plane is clamped to the border; along an axis named in `wrap` (bit 0 columns, bit 1 rows, as mlsd_gemm_args.wrap) it
 * is taken modulo the extent.  Every extent is 1 .. MLSD_RESAMPLE_MAX_EXTENT (the fractional position is in [0, 1) only while 2 s_out is exact
 * in fp32) and planes * dh * dw < 2^31; anything else returns -1.  Equal sizes copy the planes bit for bit.  src and dst must not overlap. */
enum { MLSD_RESAMPLE_NEAREST = 0, MLSD_RESAMPLE_BILINEAR = 1, MLSD_RESAMPLE_BICUBIC = 2 };
enum { MLSD_RESAMPLE_MAX_EXTENT = 1 << 22 };
int mlsd_resample2d(const float* src, int sw, int sh, float* dst, int dw, int dh, int planes, int mode, int wrap, void* stream);
/* Antialiased resampling of the same planes (hip/resample_aa.hip; not in the reference): a filter whose support grows with the shrink factor, as PIL's resize
 * and torch's interpolate(antialias=True).  Per axis, with scale = s_in / s_out and fs = max(scale, 1), output index d has the centre c = scale (d + 0.5) and the
 * taps j in [lo, hi), lo = floor(c - sup fs + 0.5), hi = floor(c + sup fs + 0.5): the exact integer floor divisions of s_in (2 d + 1) + s_out -+ (2 sup) max(s_in, s_out)
 * by 2 s_out.  Without wrap lo and hi are clipped to [0, s_in]; with wrap they are not, the tap index is taken modulo s_in (a window may go around a small plane
 * several times).  The weight of tap j is f((j - c + 0.5) / fs), computed and normalised to sum 1 in double, rounded once to fp32.
 *   MLSD_AA_BOX       sup 0.5  f = 1 on -0.5 < x <= 0.5 (integer factors: the average of the block)
 *   MLSD_AA_TRIANGLE  sup 1    1 - |x|                              (torch: bilinear, antialias=True)
 *   MLSD_AA_CUBIC     sup 2    Keys cubic, a = -0.5 (not the -0.75 of MLSD_RESAMPLE_BICUBIC)      (torch: bicubic, antialias=True)
 *   MLSD_AA_LANCZOS3  sup 3    sinc(x) sinc(x / 3)                  (PIL: LANCZOS)
 * mlsd_resample_aa_taps fills start[s_out], count[s_out] and w[s_out][k_max] (the row's tail beyond its count is zero) for one axis and returns the largest count,
 * or -1 for a bad argument or a k_max below it; mlsd_resample_aa_max_taps returns the largest count of the unclipped windows, an upper bound for either wrap.  Host
 * code, no GPU needed.
 * mlsd_resample2d_aa: two passes, rows first ([planes][sh][dw] in the workspace), then columns; an axis whose extents are equal is skipped, equal sizes on both copy
 * the planes bit for bit.  Every sum is fp32 in ascending tap order, products and additions rounded one by one: the result is a function of the tables alone.
 * wrap as mlsd_resample2d.  ws: mlsd_resample2d_aa_ws_bytes of device memory (the tables, built on the host per call and uploaded on the stream, which is waited for
 * once, and the intermediate): not for captured plans.  Returns -1 before any launch for non-positive extents, extents above MLSD_RESAMPLE_MAX_EXTENT, 2^31 elements or
 * more in src, dst or the intermediate, a bad filter or wrap, a NULL workspace, or src, dst and ws overlapping. */
enum { MLSD_AA_BOX = 0, MLSD_AA_TRIANGLE = 1, MLSD_AA_CUBIC = 2, MLSD_AA_LANCZOS3 = 3 };
int mlsd_resample_aa_taps(int s_in, int s_out, int filter, int wrap_axis, int* start, int* count, float* w, int k_max);
int mlsd_resample_aa_max_taps(int s_in, int s_out, int filter);
size_t mlsd_resample2d_aa_ws_bytes(int sw, int sh, int dw, int dh, int planes, int filter);
int mlsd_resample2d_aa(const float* src, int sw, int sh, float* dst, int dw, int dh, int planes, int filter, int wrap, void* ws, void* stream);
/* for measurements (tools/resample_aa_measure.py): the LDS bytes a block of the horizontal pass may use, 0 .. 32 KiB (the default); a launch whose tile needs more reads
 * global memory directly, so 0 runs every shape that way.  The results do not depend on it.  A negative value only asks; returns the previous limit. */
int mlsd_resample2d_aa_lds_limit(int bytes);
/* Canny edge detection of NCHW fp32 planes (hip/canny.hip; not in the reference): the preprocessor of a ControlNet's control image.  The specification is
 * OpenCV's Canny with aperture 3 as recalled, written out here; OpenCV was not at hand: parity-unpinned against OpenCV, pinned to these rules.  Everything
 * behind (a) is integer arithmetic, so the result is held bit for bit (tests/canny_ref.py restates it twice).
 *  (a) q = min(255, max(0, (int)floorf(v * 255.0f + 0.5f))) per plane (product and sum rounded one by one; resamples overshoot, hence the clamp).
 *  (b) thresholds (mlsd_canny_thresholds, host only): the two are swapped if low > high; L1: lo = floor(low), hi = floor(high); L2: both are limited to 32767
 *      (and to 0 from below) first, then lo = floor(low)^2, hi = floor(high)^2 -- magnitudes are compared squared, there is no square root.  Returns 0, -1 for a NaN
 *      or a NULL pointer.  mlsd_canny takes lo and hi as this gives them.
 *  (c) Sobel per plane in int: dx = (q[y-1][x+1] + 2 q[y][x+1] + q[y+1][x+1]) - (the same at x-1), dy likewise down minus up; taps outside the image replicate
 *      the border pixel, or wrap around on an axis named in `wrap` (bit 0 columns, bit 1 rows, as mlsd_resample2d).
 *  (d) m = |dx| + |dy| (L1) or dx^2 + dy^2 (L2); with 3 planes a pixel takes dx, dy and m from the plane with the largest m, the lowest plane index on ties.
 *      m outside the image counts as 0, on a wrapped axis it is the wrapped pixel's.
 *  (e) non-maximum suppression of the pixels with m > lo: with x = |dx|, y = |dy| << 15, t22 = 13573 x, t67 = t22 + (x << 16): if y < t22 the pixel is kept when
 *      m > m[y][x-1] && m >= m[y][x+1]; else if y > t67 when m > m[y-1][x] && m >= m[y+1][x]; else, with s = -1 if (dx ^ dy) < 0 and 1 otherwise, when
 *      m > m[y-1][x-s] && m > m[y+1][x+s].  A kept pixel is strong if m > hi, else weak.
 *  (f) hysteresis: an edge is every strong pixel and every weak pixel 8-connected to a strong one through weak or strong pixels, around wrapped axes too.
 * dst [planes_out][h][w] gets 1.0f on edges and 0.0f elsewhere, every plane the same.  ws: mlsd_canny_ws_bytes(w, h) of device memory from mlsd_malloc (two
 * byte maps and the sweeps' flags; 0 for a size mlsd_canny refuses).  The hysteresis runs as sweeps over 128 x 128 tiles, launched in small groups whose flags the
 * host reads back, waiting for the stream: not for captured plans.  *n_passes (host, may be NULL): the sweeps up to and including the first that changed nothing,
 * at least 1 and at most w h + 1, which is also the cap of the host's loop (up to mlsd_canny_tile(4) - 1 further launched sweeps copied their input).
 * Returns -1 before any launch for planes or planes_out not 1 or 3, an extent below 1 or above MLSD_CANNY_MAX_EXTENT, 2^31 elements or more in 3 planes, a bad wrap
 * or l2, a NULL workspace, or src, dst and ws overlapping.
 * mlsd_canny_tile: the kernels' constants for tests and measurements -- 0, 1: tile of the classification (x, y); 2, 3: tile of a sweep; 4: sweeps per group.
 * mlsd_invert: dst[i] = 1 - src[i] (one rounding), src == dst allowed. */
enum { MLSD_CANNY_MAX_EXTENT = 1 << 20 };
size_t mlsd_canny_ws_bytes(int w, int h);
int mlsd_canny(const float* src, int w, int h, int planes, int low, int high, int l2, int wrap, float* dst, int planes_out, void* ws, int* n_passes, void* stream);
int mlsd_canny_thresholds(double low, double high, int l2, int* lo, int* hi);
int mlsd_canny_tile(int which);
int mlsd_invert(const float* src, float* dst, int64_t n, void* stream);
/* Region inpainting, the image-space pieces (hip/inpaint.hip; not in the reference): fp32 planes [planes][h][w].  wrap: bit 0 the x axis, bit 1 the y axis, as
 * everywhere.  An index outside a plane replicates the border pixel (what OpenCV's BORDER_REPLICATE does; the border mode front ends blur their masks with is
 * BORDER_REFLECT_101 as recalled, which could not be checked when this was written: parity-unpinned, pinned to this rule); on a wrapped axis it is taken modulo
 * the extent, a true modulo, so a radius may exceed the extent.  No float atomics anywhere: two calls give identical bytes.  Crops are mlsd_window_gather.
 *   mlsd_mask_weight  p[i] = min(max(invert ? m[i] : 1 - m[i], 0), 1), the repaint weight; NaN gives 0.  The reference's masks say 1 = keep, 0 = repaint; invert
 *                     takes the front ends' convention (white = repaint).  mask == p is allowed.
 *   mlsd_mask_grow    one plane.  radius > 0: the maximum over the (2 r + 1)^2 square around a pixel; radius < 0: the minimum over the (2 |r| + 1)^2 square; 0: a
 *                     copy of the bits.  |radius| <= MLSD_MASK_GROW_MAX.  Separable: rows into ws (w h floats), then columns.  Maximum and minimum are exact, the
 *                     result is held bit for bit.
 *   mlsd_gauss_taps   host only.  Radius r = (int)(2.5 sigma + 0.5) -- the kernel size OpenCV's GaussianBlur gets from the front ends' "mask blur" as recalled
 *                     (ksize = 2 int(2.5 sigma + 0.5) + 1); it could not be checked: parity-unpinned, pinned to this rule.  Weights exp(-k^2 / (2 sigma^2)),
 *                     k = -r .. r, computed and normalised to sum 1 in double, then rounded to float.  Returns 2 r + 1, or -1 when that exceeds k_max or sigma is
 *                     outside 0 .. MLSD_GAUSS_MAX_SIGMA (so r <= 160, at most MLSD_GAUSS_MAX_TAPS taps).  r == 0 (sigma < 0.2): one tap of 1.0.
 *   mlsd_gauss_blur   dst[y][x] = sum_j t[j] (sum_k t[k] src[y - r + j][x - r + k]): rows first into the workspace, then columns; each sum is fp32 in ascending
 *                     tap order, every product and addition rounded on its own (no contraction), so every route to the kernel agrees bit for bit, whatever the
 *                     tile.  r == 0 copies the bits.  ws: mlsd_gauss_blur_ws_bytes(w, h, planes) of device memory (the taps, uploaded on the stream, which is
 *                     waited for once, and the intermediate): not for captured plans.  The row pass stages its tile's span in LDS and reads global memory
 *                     directly where the span of 4 rows exceeds the limit: mlsd_gauss_blur_lds_limit(bytes) lowers that limit (0 .. 32768; 0 runs every shape
 *                     the direct way; negative only asks; returns the previous limit) for tests and measurements.  The results do not depend on it.
 *   mlsd_mask_bbox    out4_dev (4 ints in device memory) = x0, y0, x1, y1, half open, of the pixels with p > 0 (1e-30 counts, -0.0 and NaN do not); 0, 0, 0, 0
 *                     when there are none.  Integer minima and maxima (integer atomics: order-independent): an initialising fill, the reduction, and a
 *                     one-thread launch that writes the zeros of the empty case.
 *   mlsd_composite    dst [B][planes][H][W]; orig [n_orig][planes][H][W], n_orig 1 (shared) or B; patch [B][planes][ch][cw]; p [H][W].  Outside the rectangle
 *                     [x0, x0 + cw) x [y0, y0 + ch) dst = orig, a copy; inside dst = orig (1 - p) + patch p in mask_apply's arithmetic: 1 - p, the two products
 *                     and the sum each rounded once.  So p == 0 gives the original's value, p == 1 the patch's, and the result is numpy's fp32 expression.
 *                     dst may be orig when n_orig == B.
 * All return -1 before any launch for a NULL pointer, an extent below 1 or above MLSD_INPAINT_MAX_EXTENT, 2^31 elements or more, a bad wrap, radius, sigma or
 * rectangle, and buffers that overlap other than as allowed above. */
enum { MLSD_INPAINT_MAX_EXTENT = 1 << 20, MLSD_MASK_GROW_MAX = 256, MLSD_GAUSS_MAX_SIGMA = 64, MLSD_GAUSS_MAX_TAPS = 321 };
int mlsd_mask_weight(const float* mask, float* p, int64_t n, int invert, void* stream);
int mlsd_mask_grow(const float* src, float* dst, int w, int h, int radius, int wrap, void* ws, void* stream);
int mlsd_gauss_taps(float sigma, float* w, int k_max);
size_t mlsd_gauss_blur_ws_bytes(int w, int h, int planes);
int mlsd_gauss_blur(const float* src, float* dst, int w, int h, int planes, float sigma, int wrap, void* ws, void* stream);
int mlsd_gauss_blur_lds_limit(int bytes);
int mlsd_mask_bbox(const float* p, int w, int h, int* out4_dev, void* stream);
int mlsd_composite(float* dst, const float* orig, int n_orig, const float* patch, const float* p, int W, int H, int planes, int B, int x0, int y0, int cw, int ch,
                   void* stream);
/* Tiled diffusion (MultiDiffusion; not in the reference): the canvas latent is evaluated in overlapping windows of the UNet plan's size, the windows'
 * outputs are blended by a weighted average.  Window pixel (v, u) of a ww x wh window that starts at (x0, y0) lies on canvas pixel
 * ((y0 + v) mod H, (x0 + u) mod W): a window may straddle the seam of a wrapped axis; on an axis that does not wrap the caller keeps x0 + ww <= W.
 * Its weight is r_y(v) r_x(u), r(i) = min(i + 1, T - i, O + 1) / (O + 1) with the window's extent T and the overlap O of that axis (fp32 from integers).
 * All three return -1 before any launch for non-positive extents, a window larger than the canvas, a start outside the canvas, 2^31 elements or more,
 * or buffers that overlap.
 *   gather: win [planes][wh][ww] <- canvas [planes][H][W] (NCHW fp32), a copy of the bits.
 *   blend:  eps_canvas[n][q][c] += (w(v, u) / wsum[q]) * eps_win[n][v ww + u][c] for the first C = 4 channels of eps_win NHWC [N][wh ww][ld_win]; eps_canvas NHWC
 *           [N][H W][4] dense (16-byte aligned), wsum [H W].  No atomics: a window touches a canvas pixel once, the windows of one evaluation are blended by
 *           successive launches on one stream into a canvas zeroed before the first.
 *   wsum:   wsum[q] = sum of the weights of the nx x ny windows (starts xs, ys: HOST arrays, at most MLSD_WINDOW_MAX_AXIS each) that cover q, y outer. */
enum { MLSD_WINDOW_MAX_AXIS = 64 };
int mlsd_window_gather(const float* canvas, int W, int H, float* win, int ww, int wh, int x0, int y0, int planes, void* stream);
int mlsd_window_blend(const float* eps_win, int64_t ld_win, float* eps_canvas, const float* wsum, int W, int H, int ww, int wh,
                      int x0, int y0, int ox, int oy, int N, int C, void* stream);
int mlsd_window_wsum(float* wsum, int W, int H, int ww, int wh, const int* xs, int nx, const int* ys, int ny, int ox, int oy, void* stream);
/* The same for the P windows of one batched plan evaluation (mlis_amd_tile_pack), one launch each.  xs, ys: HOST arrays of n_slots window starts, slot order.
 *   gather_packed: win [n_slots][planes][wh][ww] <- for slot s, canvas [planes][H][W] at ((ys[s] + v) mod H, (xs[s] + u) mod W), a copy of the bits.
 *   blend_packed:  eps_win is the packed plan's output, NHWC [G][n_slots][B][wh ww][ld_win] (G = 2 with guidance: cond of every slot, then uncond of every slot),
 *                  eps_canvas [G][B][H W][4] dense.  Slots 0 .. n_used-1 are blended, slots n_used .. n_slots-1 are never read.  One thread per canvas pixel walks
 *                  the slots in order, so the canvas holds, bit for bit, what n_used successive mlsd_window_blend launches in slot order leave.
 * Both refuse, before any launch, what the single-window entry points refuse, n_slots outside 1 .. MLSD_WINDOW_MAX_PACK, n_used outside 1 .. n_slots, B < 1,
 * G not 1 or 2, C != 4, 2^31 elements or more, and overlapping buffers. */
enum { MLSD_WINDOW_MAX_PACK = 16 };
int mlsd_window_gather_packed(const float* canvas, int W, int H, float* win, int ww, int wh, const int* xs, const int* ys, int n_slots, int planes, void* stream);
int mlsd_window_blend_packed(const float* eps_win, int64_t ld_win, float* eps_canvas, const float* wsum, int W, int H, int ww, int wh, const int* xs, const int* ys,
                             int n_used, int n_slots, int ox, int oy, int B, int G, int C, void* stream);
/* ControlNet (csrc/hip/control.hip; not in the reference).
 *   ctrl_add:  dst[n][r][c] = base[n][r][c] + gain * ctrl[n % n_ctrl_img][r][c], fp32 channels-last maps of rows_per_img rows x C with row strides ld_* (floats), the
 *              product and the sum rounded separately.  gain is ONE float in device memory, read when the kernel runs: it may change between launches of a captured graph.
 *              gain == 0: dst gets base's bits and ctrl is never read (it may hold NaN).  dst == base with equal strides is allowed (in place).
 *              Refused before any launch: C or a stride not a multiple of 4, a stride below C, a pointer not 16-byte aligned, n_ctrl_img outside 1 .. n_img, dst
 *              overlapping ctrl or (other than in place) base.
 *   window_gather_nhwc:  dst [n_slots][n_rep][wh][ww][C] <- src [H][W][C] at ((ys[s] + v) mod H, (xs[s] + u) mod W): the window of slot s, n_rep copies of it, bit for
 *              bit.  Starts as in mlsd_window_gather_packed.  Refuses C not a multiple of 4, pointers not 16-byte aligned, a window larger than the canvas, a start
 *              outside it, n_slots outside 1 .. MLSD_WINDOW_MAX_PACK, overlapping buffers. */
int mlsd_ctrl_add(float* dst, int64_t ld_dst, const float* base, int64_t ld_base, const float* ctrl, int64_t ld_ctrl, int n_img, int rows_per_img, int C, int n_ctrl_img,
                  const float* gain_dev, void* stream);
int mlsd_window_gather_nhwc(const float* src, int W, int H, int C, float* dst, int ww, int wh, const int* xs, const int* ys, int n_slots, int n_rep, void* stream);
/* FreeU, version 2 of the published code (csrc/hip/freeu.hip; not in the reference).  Channels-last fp32 maps of n_img images with row strides ld_* (floats).
 *   freeu_backbone: m[n,p] = mean_c src[n,p,c]; mh = (m - min_p m) / (max_p m - min_p m) per image; dst[n,p,c] = src[n,p,c] ((b - 1) mh[n,p] + 1) for c < C / 2,
 *              src's bits for c >= C / 2.  Where max == min (the published code divides by zero) the factor is 1.
 *   freeu_skip:  the published Fourier_filter with threshold 1 on planes of H x W, per image and channel: the four centred DFT bins {0,-1} x {0,-1} times s, the real
 *              part of the inverse, in closed form (seven plane sums, a seven-term apply).  The form holds for H, W >= 2; 2 .. 1024 per side are accepted.
 *   b_dev / s_dev are ONE float in device memory, read when the kernels run: they may change between launches of a captured graph.  A value of exactly 1 makes dst
 *   a bit copy of src: no reduction runs and the workspace is never read.
 *   ws: mlsd_freeu_ws_bytes(n_img, H, W, C) bytes (rows_per_img = H W for the backbone; the size serves either call), 16-byte aligned, contents irrelevant.
 *   Sums are taken in a fixed order without atomics (the same bits every run): 256 slots that each add ceil(n / 256) terms in sequence, then a balanced tree of 8
 *   levels; mlsd_freeu_depth(n) = ceil(n / 256) - 1 + 8 (pure, host) is the largest number of fp32 additions between a term and its finished sum of n terms
 *   (n = C for the backbone's mean, n = H W for the filter's plane sums).
 *   Refused before any launch: C not a multiple of 8 (C / 2 must fall on a 16-byte vector), a stride below C or not a multiple of 4, a pointer not 16-byte
 *   aligned, H or W outside 2 .. 1024 (skip), dst, src, ws and the factor overlapping one another. */
int mlsd_freeu_backbone(float* dst, int64_t ld_dst, const float* src, int64_t ld_src, int n_img, int rows_per_img, int C, float* ws, const float* b_dev, void* stream);
int mlsd_freeu_skip(float* dst, int64_t ld_dst, const float* src, int64_t ld_src, int n_img, int H, int W, int C, float* ws, const float* s_dev, void* stream);
size_t mlsd_freeu_ws_bytes(int n_img, int H, int W, int C);
int mlsd_freeu_depth(int n_terms);
/* HyperTile's row permutation (csrc/hip/hypertile.hip; not in the reference).  src and dst are dense [n_img][H W] rows of row_bytes bytes each.  With nh = H / th,
 * nw = W / tw:
 *   inverse 0:  dst row ((img nh + ty) nw + tx) th tw + y tw + x  =  src row img H W + (ty th + y) W + tx tw + x    (image order -> tile-major order)
 *   inverse 1:  the same map with the roles of the two sides swapped                                                (tile-major order -> image order)
 *   so that every tile of th x tw tokens is a contiguous run of th tw rows.  Bytes are moved, nothing is computed: fp16 and fp32 rows alike, NaN payloads survive.
 *   All offsets are 64-bit.  Refused with an error and no launch: th not dividing H or tw not dividing W, row_bytes not a multiple of 16, a pointer not 16-byte
 *   aligned, src == dst or overlapping ranges (there is no in-place form), a count below 1. */
int mlsd_tile_permute(const void* src, void* dst, int n_img, int H, int W, int th, int tw, int row_bytes, int inverse, void* stream);
/* Dense-block convolution of the ESRGAN upscaler (csrc/hip/upscale.hip; not in the reference): 3x3, stride 1, zero padding 1, Cin in {32, 64, 96, 128, 160, 192} to N in
 * {32, 64} output channels over a channels-last fp16 image [n_img][H][W] with lda halfs between pixels (lda >= Cin: A may be a channel slice of a wider buffer; columns >= Cin
 * are never read).  upsample 1: the output is 2H x 2W and the taps read the nearest-2x upsampled image (folded into the gather, as mlsd_gemm_args.upsample).
 * W_: fp16 [N][3][3][Cin], K-contiguous (mlsd_gemm's conv layout).  Outputs C16 (fp16, stride ldc16) and / or C32 (fp32, stride ldc32), each possibly a channel slice: columns
 * outside [0, N) of a destination row are never written.
 * Arithmetic: fp16 operands, fp32 accumulation on MFMA (v_mfma_f32_16x16x32_f16), nothing else rounded; then in fp32, each operation rounded once:
 *   z = acc + bias[n];  a = lrelu ? (z >= 0 ? z : 0.2f z) : z;  y = a * scale + resid[m][n]  (scale applies even without resid);  resid2: y = y * scale2 + resid2[m][n];
 *   C32 = y, C16 = y rounded to nearest even.  Deterministic: the same input gives the same bits.
 * Refused with an error and no launch: Cin or N outside the lists; A or W_ not 16-byte aligned, lda not a multiple of 8; C32 / resid / resid2 not 16-byte aligned or a stride
 * of theirs not a multiple of 4; C16 not 8-byte aligned or ldc16 not a multiple of 4; a stride below its width; an output that aliases A (a tap reads neighbours that
 * another wave may already have overwritten) -- except an fp16 slice of A's own rows (ldc16 == lda, no upsample) in columns >= Cin, which the taps never read; C32
 * overlapping a residual other than in place (same pointer and stride). */
typedef struct mlsd_dconv_args {
	const void* A; int64_t lda;
	int n_img, H, W, Cin;
	int upsample;
	const void* W_; int N;
	const float* bias;          /* [N] or NULL */
	int lrelu;                  /* LeakyReLU(0.2) */
	float scale;
	const float* resid; int64_t ldr;      /* fp32 [M][ldr] or NULL */
	float scale2;
	const float* resid2; int64_t ldr2;    /* fp32 [M][ldr2] or NULL */
	float* C32; int64_t ldc32;
	void* C16; int64_t ldc16;
} mlsd_dconv_args;
int mlsd_conv3x3_dense(const mlsd_dconv_args* a, void* stream);
/* label of the kernel instantiation these arguments launch, "dconv3x3<n32,c192[,up]>" (mlsd_gemm_variant's counterpart; valid until the thread's next call) */
const char* mlsd_dconv_variant(const mlsd_dconv_args* a);
/* finite check (ltensor_finite_check, src/unet.c:487): counts non-finite values into *count (device int32) */
int mlsd_count_nonfinite(const float* x, size_t n, int32_t* count, void* stream);
/* deterministic synthetic parameter fill, bit-identical to oracle/o_core.c orc_synth_fill.
 * Writes element i (reference-layout index, ne[0] fastest) at position perm(i):
 *   layout 0: identity;  layout 1: conv weight [k0,k1,cin,cout] (reference) -> [cout][k1][k0][cin_pad];
 *   layout 2: GEGLU row interleave of a [n_in, 2*d] linear weight; layout 3: same for its bias.
 * dtype: 0 fp32, 1 fp16.  The destination must be zero-initialised when padding is present. */
int mlsd_synth_fill(void* dst, int dtype, int64_t n, uint64_t key, float offset, float kf, int layout,
                    int64_t p0, int64_t p1, int64_t p2, int64_t p3, int64_t p4, void* stream);
/* LoRA update of a device weight in place (hip/lora.hip): for the reference element i = o n0 + c, o < n1, c < n0,
 *   W[dst(i)] = W[dst(i)] + (sum over r ascending of up[o][r] * down[r][c]) * scale,  rounded to nearest even at the weight's type,
 * with dst the layout rule of mlsd_synth_fill (layouts 0, 1, 2; p0..p4 as there; padding elements are never written) and the host merge's arithmetic
 * (mlts_lora_apply: separate multiply and add, one rounding of the result), so that the weight equals the one merged on the host bit for bit.
 * up [n1][r] and down [r][n0] are fp32 on the device, already rounded to the operand precision of the merge.  *flag (device) is set to 1 when any
 * result is not finite (the weight then holds that result: the caller restores it).  dtype: 0 fp32, 1 fp16. */
int mlsd_lora_apply(void* W, int dtype, int64_t n0, int64_t n1, const float* up, const float* down, int r, float scale, int layout,
                    int64_t p0, int64_t p1, int64_t p2, int64_t p3, int64_t p4, int* flag, void* stream);

/* co-issue probe (round 6, tools/coissue_probe.py): 8 x {one 32x32x16 MFMA if mf, nv (3 / 6) vector instructions of kind vk (1 fma, 2 exp, 3 pk_fma, 4 cvt_pk, 5 max3, 6 pk_add, 7 add,
 * 8 dot2_f32_f16, 9 pk_mul, 10 pk_fma_f16, 11 exp_f16)} per iteration; nthreads 256 / 512 = one / two waves per SIMD; clocks[nblocks] */
int mlsd_probe_coissue(const void* src, int iters, int nblocks, int nthreads, int mf, int vk, int nv, void* clocks, void* sink, void* stream);

#ifdef __cplusplus
}
#endif
