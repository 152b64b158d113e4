/*
 * regione_hip.h - C ABI of libregione_hip.so: RegionE's region-aware denoising hot path as
 * hand-written HIP kernels for gfx950 (MI355X / CDNA4).
 *
 * The reference (Peyton-Chen/RegionE) is pure Python + one Triton kernel and has NO native
 * surface; each entry point below names the reference Python function (file:line under
 * /root/reference/RegionE/FluxKontext/) it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - tensors are dense row-major; `ld*` arguments are row strides in ELEMENTS;
 *   - dtype codes: RGN_F32 = 0, RGN_BF16 = 1;
 *   - `stream` is a hipStream_t (PyTorch: torch.cuda.current_stream().cuda_stream); all work is
 *     enqueued on it, nothing synchronises, nothing allocates, buffers are borrowed;
 *   - return value: 0 on success, otherwise a negative RGN_E_* code or a positive hipError_t;
 *     rgn_last_error() returns a static string describing the last failure on this thread.
 */
#ifndef REGIONE_HIP_H
#define REGIONE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGN_F32 0
#define RGN_BF16 1

#define RGN_E_BADARG (-1)
#define RGN_E_UNSUPPORTED (-2)

/* Bumped whenever a struct layout or a signature of this header changes.  rgn_version() returns the value the LIBRARY was built
 * with, rgn_abi_struct_bytes() = sizeof(rgn_qkv_epilogue) * 1000 + sizeof(rgn_gemm_problem) as the library sees them: a binding
 * compiled against another header (a stale libregione_torch.so next to a rebuilt libregione_hip.so) compares both at load time
 * and refuses to run instead of misreading structs passed by pointer. */
#define RGN_ABI_VERSION 124
int rgn_version(void);
size_t rgn_abi_struct_bytes(void);
const char* rgn_last_error(void);
/* Launch-plan override: the library's one test / measurement hook (no reference counterpart).  Every knob is -1 (= the launch cost
 * models decide) in a shipped run.  `key` in {gemm_pieces (1 = one plain launch, n >= 2 = n K pieces of a round's remainder),
 * gemm_geometry (128 | 256), gemm_asm (0 = compiler-scheduled kernels only), gemm_quarter (0 never | 1 always), attn_waves (4 | 8),
 * attn_split (0 = never cut KV), attn_streamk (0 = equal pieces only | 1 = wherever possible), attn_asm (0 = compiler-scheduled
 * loop), rowbands (0 = rgn_rowband_fork does nothing | 1 = on, the default | 2..98 = on, band 0 takes that share in percent of the row
 * tiles)}; value -1 restores the default; key NULL resets every knob.  Process-wide, not synchronised with launches in flight on other
 * threads.  The same knobs can be preset once per process with RGN_PLAN_OVERRIDE="key=value,key=value" - the only environment
 * variable libregione_hip.so reads, at the first launch.  Results never depend on a knob beyond fp32 summation order. */
int rgn_plan_override(const char* key, int value);
/* The current value of one knob (-1 = not forced), so that a scoped override can restore what it found instead of resetting
 * (nested scopes, a process preset through RGN_PLAN_OVERRIDE). */
int rgn_plan_override_get(const char* key, int* value);
/* The launch plan the GEMM planner chose for the last rgn_gemm_group call on this thread (introspection for tests and traces; the
 * reference has no counterpart): bits 0-7 = K pieces of the remainder (1 = none), bit 8 = quarter-tile remainder, bit 10 =
 * 256 x 256 tile geometry, bit 11 = launched as two row bands (rgn_rowband_fork), bits 12-15 = K pieces of the remainder on the
 * 128 x 128 geometry (0 = not cut; only ever set with bit 10 clear). */
int rgn_gemm_last_plan(void);
/* The plan the planner WOULD choose for a group of `nprob` (<= 4) problems with M = Ms[i] rows, N output channels, depth K, `distinct_w`
 * different weight matrices (problems of one stream share W), bf16 (w8 = 0) or fp8 (w8 = 1) weights, or fp8 weights AND fp8 activations
 * (w8 = 2: `ascale`, whole-K tiles only - never K pieces) and a workspace of `workspace_bytes` (0 = none): same bits as rgn_gemm_last_plan.  Pure host arithmetic on the launch cost model - no launch, no GPU
 * (CPU tests pin the planner's decisions for the region-step shapes with it); negative RGN_E_* on a bad argument. */
int rgn_gemm_plan_query(const int* Ms, int nprob, int N, int K, int distinct_w, int w8, size_t workspace_bytes);

/* Row bands (no reference counterpart: scheduling only).  Between two attentions every stage of a transformer block is row-wise - output
 * projection, LN-modulate, the feed-forward GEMMs, the next block's Q/K/V projection - so the rows can be cut ONCE into two bands whose
 * chains run on two streams: the partially filled last round of one band's GEMM is filled by the other band's next launch.
 *   rgn_rowband_fork(stream): the library's side stream (one per thread and device, created at the first fork) waits for everything
 *     enqueued on `stream`; from here on rgn_gemm_group and rgn_ln_modulate / rgn_ln_modulate_segs calls of THIS thread on `stream` cut
 *     their rows at the band boundary and launch band 0 on `stream`, band 1 on the side stream.
 *   rgn_rowband_join(stream): `stream` waits for the side stream; launches are whole again.  Without a fork it does nothing.
 * Ordering is hipEventRecord / hipStreamWaitEvent only.  The CALLER guarantees that every call between fork and join is row-wise in the
 * same rows (reads only the rows it writes, of buffers the earlier calls wrote with the same problem sizes) and joins before anything
 * that is not (attention, a call with other row counts, another stream).
 * Boundary: the problem (LN: row segment) with the most rows - of equal ones the one highest in memory - is cut at a multiple of 256 rows
 * from its first row, so that band 0 (every other problem whole + its first rows) holds its share (half) of the 256-row tiles; a problem of
 * fewer than two tiles is not cut (everything is band 0).  A band launch uses the tile geometry the planner picks for the whole group and
 * runs whole tiles only - no K pieces, no reduce pass, no quarter tiles, no workspace - so banded results are bit-identical to the
 * unbanded launch under gemm_pieces = 1; the fused Q/K/V epilogue's row_base advances with the pointers (rotary rows, kv_rows, K slab
 * rows and V^T positions stay those of the unbanded launch).
 *   rgn_rowband_query: the boundary for `nprob` (1..4) problems of Ms[i] rows listed in memory order - returns 1 and the cut (problem
 *     *cut_problem keeps rows [0, *cut_row) in band 0, its rows from *cut_row on are band 1), 0 when nothing is cut (*cut_problem = -1);
 *     pure host arithmetic, no GPU.
 *   rgn_rowband_side_launches: how many band-1 launches this thread has sent to a side stream so far (tests). */
int rgn_rowband_fork(void* stream);
int rgn_rowband_join(void* stream);
int rgn_rowband_query(const int* Ms, int nprob, int* cut_problem, int* cut_row);
long long rgn_rowband_side_launches(void);

/* ------------------------------------------------------------------------------------------
 * a1/a2  Adaptive Region Partition.  Replaces token_selector (utils.py:282-354) + morphology
 * (utils.py:124-237) + the one-step estimate of the scheduler (inplace.py:650).
 *
 *   est   = model_output ? f32(sample) + round_mo(round_mo(dt_final) * model_output) : f32(sample)
 *   sim   = sum_d normalize(est)[d] * normalize(cond)[d]   (each normalised in its own dtype)
 *   raw   = sim <= threshold
 *   mask  = erosion_dilation ? dilate5x5(erode3x3cross(raw)) : raw     on the [h_tok,w_tok] grid
 *   edited_ids / unedited_ids = ascending token ids with mask 1 / 0;  *count = number edited.
 *
 * sample [L,D] (f32 or bf16, upcast like inplace.py:610), model_output [L,D] or NULL,
 * cond [L,D]; D must be 64 (packed 2x2x16 latent channels).  sim_out may be NULL.
 * Two launches: rows -> similarity -> raw mask (one wave per token), then one workgroup does
 * morphology in LDS and the ballot/popcount prefix-sum compaction.
 */
int rgn_arp_partition(const void* sample, int sample_dtype, const void* model_output, int mo_dtype,
                      const void* cond, int cond_dtype, float dt_final, float threshold,
                      int L, int D, int h_tok, int w_tok, int erosion_dilation,
                      int64_t* edited_ids, int64_t* unedited_ids, uint8_t* raw_mask, uint8_t* mask,
                      float* sim_out, int32_t* count, void* stream);

/* a2 alone: remove_scattered_points (utils.py:214-237) on a u8 [h,w] mask + compaction. */
int rgn_morph_compact(const uint8_t* raw_mask, int h_tok, int w_tok, int erosion_dilation,
                      int64_t* edited_ids, int64_t* unedited_ids, uint8_t* mask, int32_t* count,
                      void* stream);

/* ------------------------------------------------------------------------------------------
 * a3  ids_gather (utils.py:260-279) / ids_scatter (utils.py:240-257) on rows of `row_bytes`
 * bytes (multiple of 4).  dst[k] = src[ids[k]]   /   dst[ids[k]] = src[k].   ids are int64.
 */
int rgn_gather_rows(const void* src, const int64_t* ids, void* dst, int K, int row_bytes, void* stream);
int rgn_scatter_rows(const void* src, const int64_t* ids, void* dst, int K, int row_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * a5  RegionEFlowMatchEulerDiscreteScheduler.step (inplace.py:581-691), arithmetic part.
 *   out[l,:] = cast_v( f32(sample[l,:]) + round_v(round_v(dt_l) * v[l,:]) )
 *   dt_l = mask ? (mask[l] ? dt : dt_direct) : dt        (split Euler on partition/refresh steps)
 * sample f32|bf16, v f32|bf16, out has v's dtype (inplace.py:686).  Gather-free: one pass over
 * the L rows instead of the reference's 4 gathers + 2 scatters + zeros + 2 axpy.
 */
int rgn_euler_step(const void* sample, int sample_dtype, const void* v, int v_dtype, void* out,
                   const uint8_t* mask, float dt, float dt_direct, int L, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * a6  Adaptive Velocity Decay cache hit (inplace.py:315-318):
 *   out[k,:] = round_c( r * cache[ids ? ids[k] : k, :] ),   r = round_ratio ? round_c(ratio) : ratio
 * The optional ids fuse the first-hit gather (inplace.py:316-317).
 * `cache * ratio` multiplies a bf16 tensor by a 0-dim fp32 tensor.  Torch's CPU kernel keeps the
 * scalar in fp32 (round_ratio = 0, what the reference-generated fixtures contain); its CUDA kernel
 * casts a *device* 0-dim tensor to bf16 first (round_ratio = 1).  Both are offered.
 */
int rgn_avd_apply(const void* cache, int dtype, const int64_t* ids, float ratio, int round_ratio, void* out,
                  int K, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * a11  classifier-free-guidance combine of the cond / uncond velocities, rows of 64 channels:
 *   mode 0  FLUX true-CFG (inplace.py:364)                      out = neg + s*(pos-neg)
 *   mode 1  Step1X norm-rescaled (Step1XEdit/inplace.py:401-410) out = neg + s*(pos-neg)/f(||pos-neg||),
 *           f(n) = n > 1 ? n^power : (n < 1 ? 1 : n)
 *   mode 2  Qwen norm-preserving (QwenImageEdit/inplace.py:401-405)
 *           c = neg + s*(pos-neg);  out = c * (||pos|| / ||c||)
 * Every intermediate is rounded to the tensor dtype like the eager op sequence.
 */
int rgn_cfg_combine(const void* pos, const void* neg, void* out, int dtype, float scale, int mode, float power,
                    int K, int D, void* stream);

/* ------------------------------------------------------------------------------------------
 * MFMA GEMM  C = epilogue(A[M,K] @ W[N,K]^T + bias)  (bf16 activations, bf16 or fp8 weights, fp32 accumulate): ONE entry point,
 * rgn_gemm_group, one descriptor (rgn_gemm_problem) per problem.  Replaces torch nn.Linear calls of the block bodies [EXT diffusers]
 * and, with `out_rows`, the Triton index-scatter GEMM _partially_linear (fused_kernels.py:9-101).
 *   epilogue: RGN_EPI_BIAS        C[r] = bf16(acc + bias)
 *             RGN_EPI_GELU        C[r] = bf16(gelu_tanh(bf16(acc + bias)))  for columns >= gelu_from_col (rounded up to 8)
 *             RGN_EPI_GATE_RESID  C[r] = bf16(f32(resid[r]) + f32(bf16(gate[n] * bf16(acc + bias))))
 *             RGN_EPI_QKV         the fused Q/K/V epilogue below; gelu_from_col <= 0 means "no GELU columns" (= N)
 *   r = out_rows ? out_rows[m] : m   (row scatter; out_rows int64 or NULL)
 * K % 64 == 0; M, N arbitrary (N > 0; M == 0 problems are skipped, a call of empty problems only returns 0).  resid uses ldc and may
 * alias C.  A, W, C, resid 16-byte aligned; lda, ldc (and ldw of bf16 weights) multiples of 8.
 *
 * Up to FOUR problems with the same N, K, epilogue and weight format go in ONE launch: the text and image streams of a double block
 * (the small problem's tiles fill the tail of the large one instead of running as an under-occupied launch of their own), for BOTH
 * classifier-free-guidance branches (reference: the B = 2 batched CFG forward, Step1XEdit/inplace.py:381-399;
 * Step1XEditV1P2/inplace.py:398,416 and QwenImageEdit/inplace.py:371-405 run the branches in sequence - rows of different
 * branches never interact in a Linear, so one launch computes both).  Each problem keeps its own activations, output,
 * gate / residual (per-branch AdaLN gates) and - with RGN_EPI_QKV - its own Q/K/V epilogue descriptor (per-branch K / V^T
 * cache slabs, rotary tables and cache-row lists); problems may share W (streamed from HBM once for both branches).
 * Per output element the accumulation order depends only on the tile geometry and the split-K piece count the planner
 * picks for the launch, never on which other problems share it.
 * `out_rows` and a strided W (`ldw` other than 0 / K) are accepted only in a launch of exactly one non-empty problem, `out_rows` not
 * with RGN_EPI_QKV (RGN_E_UNSUPPORTED otherwise).
 *
 * fp8 weights (BASELINE.json configs[4]: "fp8 weights on CDNA4"): `wscale` != NULL - then for every problem of the call - says W is
 * stored as OCP e4m3fn bytes ([N, K], ldw in BYTES, a multiple of 16) with one fp32 scale per output channel (`wscale[N]`, 16-byte
 * aligned): C = epilogue((A @ dequant(W8)^T) * wscale[n] + bias).  Activations, bias, outputs and every epilogue stay bf16 / fp32
 * exactly as with bf16 weights; the fp8 -> bf16 conversion is exact (v_cvt_scalef32_pk_bf16_fp8 in registers, after the LDS read),
 * the scale multiplies the fp32 accumulator.  Replaces nothing in the reference (which ships bf16 weights): storage format of the
 * [EXT] Linear weights only; quantisation (per-channel absmax / 448) is done by the caller
 * (regione_amd.harness.flux.FluxTransformer2DModel.quantize_fp8_).  The fp8 tiles are converted in registers inside the
 * hand-scheduled K loop.  A/B switch RGN_W8_WIDEN_MIN_M=<rows> (default 0 = never): with a workspace and at least that many rows in
 * total the call first widens W8 to bf16 (exact) into the TAIL of the workspace (N x K x 2 bytes per distinct weight matrix, >= 64 MiB
 * left for the split remainders) and runs the bf16 K loop on it - same result bit for bit, weights stay fp8 in HBM.
 *
 * fp8 activations (opt-in; no reference counterpart): `ascale` != NULL - then for every problem of the call - says A is stored as OCP
 * e4m3fn bytes ([M, K], lda in BYTES, a multiple of 16) with one fp32 scale per ROW of A (`ascale[M]`, what rgn_quantize_rows_a8 /
 * rgn_ln_modulate_a8 write): C = epilogue((A8 @ W8^T) * ascale[m] * wscale[n] + bias), the two multiplications in fp32 in that order.
 * Both operands go to the matrix unit as bytes: one v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, unit block scales) per 16 x 16 tile
 * and K tile of 128, twice the bf16 rate per clock.  Needs `wscale` (fp8 weights), K % 128 == 0 and RGN_EPI_BIAS, RGN_EPI_GELU or
 * RGN_EPI_QKV; RGN_EPI_GATE_RESID, `out_rows` and a call that mixes A formats return RGN_E_UNSUPPORTED before anything is written.
 * Such a call runs whole-K tiles only (256 x 256 tiles plus the quarter-tile remainder, or 128 x 128 tiles): no K pieces, no workspace use.
 *
 * `workspace` (optional, fp32 scratch, rgn_gemm_workspace_bytes()) enables the round-aware schedule: output tiles that do not fill a
 * whole round of the chip's workgroup slots are cut along K, spread over all CUs and finished by a reduce pass (8 workgroups per
 * tile, epilogue in registers; bit-identical to a reduce by the tile's own workgroup).  NULL = plain single launch.
 * Sizing: rgn_gemm_workspace_bytes() is a shape-independent upper bound (256 MiB = 255 remainder tiles x 4 pieces x 256 KiB of
 * fp32 fragments, plus room for the fp8 weight widening); any smaller buffer is valid too - the planner only considers piece counts
 * whose partials fit in `workspace_bytes` (and skips the split / the widening when nothing fits).
 * A workspace belongs to ONE stream at a time: calls on two streams need two buffers.
 *
 * RGN_EPI_QKV, the fused QKV projection (reference: the Linear projections + `attn.norm_q/k` + `apply_rotary_emb` + K/V cache
 * placement of RegoionEFluxAttnProcessor2_0.__call__, FluxKontext/inplace.py:735-794; the K/V partial update
 * `_partially_linear`, fused_kernels.py:81-101).  The same GEMM, but the epilogue of each 256-column block of C does what
 * rgn_qk_norm_rope_store does as a separate pass:
 *   columns [k_col, k_col + heads*128): per-head RMSNorm + RoPE (k tables, row kv_rows[r]) -> k_slab row kv_rows[r]
 *   columns [v_col, ...):               transposed into vt_slab (kv index permuted as rgn_attention expects)
 *   columns [q_col, ...):               per-head RMSNorm + RoPE (q tables, row r) -> C in place
 *   columns >= gelu_from_col:           GELU-tanh -> C           (the fused MLP half of a single-stream block)
 * K and V columns are NOT written to C.  r = row_base + local row (row_base: where this problem's rows sit in
 * the joint [text | image] sequence that the tables / kv_rows are indexed by).  Results are bit-identical to
 * RGN_EPI_BIAS followed by rgn_qk_norm_rope_store. */
#define RGN_EPI_BIAS 0
#define RGN_EPI_GELU 1
#define RGN_EPI_GATE_RESID 2
#define RGN_EPI_QKV 3
#define RGN_EPI_CONV 4            /* rgn_conv_bf16 only */
typedef struct rgn_qkv_epilogue {
    const void* wq;            /* [128] bf16 RMSNorm weights of this stream (norm_q / norm_added_q) */
    const void* wk;
    const float* cos_q;        /* [rows][128] fp32 */
    const float* sin_q;
    const float* cos_k;
    const float* sin_k;
    const int64_t* kv_rows;    /* joint row -> K/V cache row, NULL = identity */
    void* k_slab;              /* [kv rows][heads*128] bf16 */
    void* vt_slab;             /* [heads*128][skv_pad] bf16 */
    int row_base, skv_pad, k_col, v_col, q_col, heads;
    float eps;
    int fp16_roundtrip;        /* 1: K / V columns round fp32 -> fp16 -> bf16 like the reference's partial-update kernel
                                  (fused_kernels.py:80); 0: one rounding, like F.linear on store / plain steps */
} rgn_qkv_epilogue;
typedef struct rgn_gemm_problem {
    const void* A;             /* [M, K] bf16, row stride lda (elements); with `ascale`: e4m3fn bytes, lda in bytes */
    const void* W;             /* [N, K], row stride ldw */
    const float* wscale;       /* per-output-channel fp32 scale: W is OCP e4m3fn bytes; NULL: W is bf16 */
    const void* bias;          /* [N] bf16 or NULL */
    void* C;                   /* [M, N] bf16, row stride ldc */
    const void* gate;          /* RGN_EPI_GATE_RESID */
    const void* resid;
    const rgn_qkv_epilogue* qkv;   /* RGN_EPI_QKV */
    const int64_t* out_rows;   /* row scatter, NULL = identity */
    int lda, ldc, M;
    int ldw;                   /* 0 = W is dense: K elements (bf16) / K bytes (fp8) */
    const float* ascale;       /* per-row fp32 scale of A: A is OCP e4m3fn bytes (needs wscale); NULL: A is bf16 */
} rgn_gemm_problem;
int rgn_gemm_group(const rgn_gemm_problem* probs, int nprob, int N, int K, int epilogue, int gelu_from_col, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t rgn_gemm_workspace_bytes(void);

/* Skinny GEMV for the AdaLN modulation / timestep embedders:
 *   y[b,n] = bf16( sum_k W[n,k] * act(x[b,k]) + bias[n] ),  act = silu (rounded to bf16) if silu_input.
 * B <= 4, K % 8 == 0.  HBM-bound on W. */
int rgn_gemv_bf16(const void* x, int ldx, const void* W, const void* bias, void* y, int ldy, int B, int N,
                  int K, int silu_input, void* stream);

/* out[m,:] = bf16(bf16(x[m,:] * rsqrt(mean(x^2) + eps)) * w)  - RMSNorm over rows of width d
 * (QwenImageTransformer2DModel.txt_norm [EXT], call site QwenImageEdit/inplace.py:514). */
int rgn_rms_norm_rows(const void* x, int ldx, const void* w, void* out, int ldo, int M, int d, float eps,
                      void* stream);

/* y = bf16(silu(x)) elementwise on bf16 (F.silu of the AdaLN conditioning vector). */
int rgn_silu_bf16(const void* x, void* y, size_t n, void* stream);

/* y = bf16(a + b) elementwise on bf16 (fp32 add, one rounding = torch's bf16 add): `timesteps_emb + guidance_emb`, `+ pooled_projections`
 * of CombinedTimestepGuidanceTextProjEmbeddings [EXT] (call site inplace.py:476-480).  y may alias a or b. */
int rgn_add_bf16(const void* a, const void* b, void* y, size_t n, void* stream);

/* out[i] = i (i < T), out[T + k] = T + edited_ids[k]: the cache rows [text ; T + edited ids] a region step rewrites -
 * `selection = torch.cat((arange(txt_len), edited_ids + txt_len))`, inplace.py:732-733.  out: int64 [T + K]. */
int rgn_sel_rows(const int64_t* edited_ids, int K, int T, int64_t* out, void* stream);

/* hipMemsetAsync(ptr, 0, bytes) on `stream`: zero-initialises a K / V^T cache slab (the padding rows up to skv_pad must be finite;
 * the reference's caches have no padding) without a torch fill kernel. */
int rgn_fill_zero(void* ptr, size_t bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm(eps, no affine) * (1 + scale) + shift over rows of width d (AdaLN-Zero modulate).
 * Rows < split_row use (shift0, scale0), the others (shift1, scale1) - the text / image streams
 * of a double block in one launch.  Rounding points follow the eager bf16 op sequence.
 */
int rgn_ln_modulate(const void* x, int ldx, void* out, int ldo, int M, int d, float eps, int split_row,
                    const void* shift0, const void* scale0, const void* shift1, const void* scale1,
                    void* stream);

/* The same with up to FOUR row segments: rows [seg_end[i-1], seg_end[i]) use (shift[i], scale[i]); seg_end[nseg-1] == M.
 * `seg_end_host`, `shift_host`, `scale_host` are HOST arrays (of ints / device pointers) read at call time.  Used by the
 * batched CFG forward: [text_cond ; image_cond ; text_uncond ; image_uncond] rows with per-stream, per-branch AdaLN vectors
 * (reference: the B = 2 forward, Step1XEdit/inplace.py:381-399, where `temb` has one row per branch). */
int rgn_ln_modulate_segs(const void* x, int ldx, void* out, int ldo, int M, int d, float eps, int nseg,
                         const int* seg_end_host, const void* const* shift_host, const void* const* scale_host, void* stream);

/* fp8 activations for rgn_gemm_group's `ascale` (opt-in; no reference counterpart).  bf16 rows x [M, K] (row stride ldx elements) become
 * OCP e4m3fn bytes q [M, K] (row stride ldq BYTES, a multiple of 8; q 8-byte aligned) plus one fp32 scale per row, the arithmetic of the
 * per-channel weight quantiser restated per row:  scale[m] = max(amax_k |x[m,k]|, 1e-12) / 448,  q[m,k] = e4m3fn_rne(f32(x[m,k]) / scale[m])
 * - IEEE fp32 divisions, round to nearest even: bit-identical to the torch expression on the CPU.  One wave per row, the row stays in
 * registers between the amax pass and the convert pass; K % 8 == 0, K <= 16384; no atomics. */
int rgn_quantize_rows_a8(const void* x, int ldx, void* q, int ldq, float* scale, int M, int K, void* stream);
/* rgn_ln_modulate / rgn_ln_modulate_segs whose output leaves as fp8 bytes + row scales: each row forms exactly the bf16 values the bf16
 * entry would store and quantises them as rgn_quantize_rows_a8 does, in one pass over HBM - bit-identical to
 * rgn_quantize_rows_a8(rgn_ln_modulate(x)).  Row bands cut these launches like the bf16 ones. */
int rgn_ln_modulate_a8(const void* x, int ldx, void* q, int ldq, float* scale, int M, int d, float eps, int split_row,
                       const void* shift0, const void* scale0, const void* shift1, const void* scale1, void* stream);
int rgn_ln_modulate_segs_a8(const void* x, int ldx, void* q, int ldq, float* scale, int M, int d, float eps, int nseg,
                            const int* seg_end_host, const void* const* shift_host, const void* const* scale_host, void* stream);

/* "mx8 rows": activations as OCP MXFP8 (opt-in; no reference counterpart) - the format of GEMM inputs that no row-wise kernel produces
 * (GELU and attention outputs), where one scale per row would need a pass of its own over the row:
 *   q [M, K]     OCP e4m3fn bytes, row stride in BYTES, a multiple of 16; q 16-byte aligned;
 *   s [M, K/32]  E8M0 bytes, value 2^(b - 127), one per 32 consecutive k; row stride in BYTES, a multiple of 4; s 4-byte aligned - every
 *                K tile of 128 has one aligned dword of scales per row;
 *   K % 128 == 0.
 * The quantiser of a block of 32 bf16 values with amax a:  X = 2^(b - 127) is the smallest power of two with a / X <= 448, taken from the
 * bits of a (exponent field E, mantissa m in [1, 2): b = E - 8, + 1 if m > 1.75), b clamped to [0, 254] - 255, the NaN of E8M0, is
 * never written; a block of zeros (either sign) gets b = 127;  q = e4m3fn_rne(x / X), an exact quotient, and with this X nothing
 * saturates; -0 keeps its sign (code 0x80).  Non-finite input is the caller's error and is not detected: a NaN does not enter the amax
 * and becomes the NaN code 0x7f, a block that holds an infinity gets b = 247 and its infinities become what the hardware convert makes
 * of them (0x7f or +-448); no other block is affected.  tests/gemm_mx8_model.py is the specification in numpy; every kernel that writes
 * mx8 rows equals it bit for bit.
 *
 * rgn_quantize_rows_mx8: bf16 rows x [M, K] (row stride ldx elements, rows 16-byte aligned) become mx8 rows in one pass, written at
 * destination columns [col0, col0 + K) of q and scale columns [col0 / 32, (col0 + K) / 32) of s (col0 % 128 == 0, ldq >= col0 + K,
 * lds >= (col0 + K) / 32): a result can land in some columns of a wider buffer whose other columns another producer fills.  Nothing
 * outside those columns is written.  One wave per row, plain vector loads and stores, one writer per byte, no atomics; row bands cut
 * it like rgn_quantize_rows_a8 (a launch per band on the band's rows). */
int rgn_quantize_rows_mx8(const void* x, int ldx, void* q, int ldq, void* s, int lds, int col0, int M, int K, void* stream);

/* ------------------------------------------------------------------------------------------
 * Region-Instruction KV-cache write (RegoionEFluxAttnProcessor2_0, inplace.py:717-763,792-794):
 * per-head RMSNorm(q), RMSNorm(k) + RoPE on raw projections and placement into the K / V^T slab.
 *   qkv     [M, ld] bf16 with column blocks k_raw @ k_col, v_raw @ v_col, q_raw @ q_col (H*128 each)
 *   q is normalised + rotated IN PLACE (cos/sin row = rope_q_rows ? rope_q_rows[m] : m of table q);
 *   k row m goes to slab row kv_rows ? kv_rows[m] : m, rotated with the FULL-id table at that row
 *     (MANAGER.image_rotary_emb, inplace.py:499);  v row m goes to column kvpos(row) of V^T.
 *   rows < split_row use (wq0, wk0) RMSNorm weights (text stream: norm_added_q/k), others (wq1, wk1).
 * K slab: [Skv_pad, H*128] bf16.  V^T slab: [H*128, Skv_pad] bf16 with the kv index permuted inside
 * every 16-group (bits 2<->3 swapped) so that the attention kernel's PV operand is one 16-byte read.
 */
int rgn_qk_norm_rope_store(void* qkv, int ld, int k_col, int v_col, int q_col, int M, int H,
                           int split_row, const void* wq0, const void* wk0, const void* wq1, const void* wk1,
                           float eps, const float* cos_q, const float* sin_q, const float* cos_k,
                           const float* sin_k, const int64_t* kv_rows, void* k_slab, void* vt_slab,
                           int skv_pad, void* stream);

/* ------------------------------------------------------------------------------------------
 * Joint attention over the compacted query set against the full K/V cache; replaces
 * flash_attn_func / SDPA (inplace.py:796-806).  softmax(Q K^T / sqrt(128)) V, non-causal,
 * Sq != Skv allowed, head_dim 128, fp32 online softmax, bf16 MFMA.
 *   Q [Sq, H*128] (row stride ldq) ; K slab / V^T slab as written by rgn_qk_norm_rope_store;
 *   O [Sq, H*128] (row stride ldo), may alias Q (each workgroup reads its Q tile before writing;
 *   with a workspace, split items write O only in the final combine pass).
 * What the kernels read behind Skv (skv_pad >= Skv rounded up to 64; tests/test_gpu_region_attn_probes.py):
 *   K slab rows [Skv, round_up(Skv, 64)): the pad rows of the last 64-key tile are LOADED and their scores masked to -inf before
 *     the row maximum - any bits, NaN included, are harmless;
 *   V^T slab columns of that tile that hold no key (kvpos(r) of no r < Skv): LOADED and multiplied by P = 0 - they must be FINITE
 *     (0 * NaN and 0 * inf would reach the output), any finite value is harmless;
 *   nothing at or behind row / column round_up(Skv, 64) of either slab is read, and nothing outside [Sq, H*128] of O is written.
 */
int rgn_attention(const void* Q, int ldq, const void* k_slab, const void* vt_slab, int skv_pad, void* O,
                  int ldo, int Sq, int Skv, int H, float scale, void* workspace, size_t workspace_bytes,
                  void* stream);
/* The same with a caller-provided bound on the scores: the caller GUARANTEES |q . k| * scale <= score_bound for every (query,
 * key) pair of the call - e.g. q and k are RMS-normalised per head (norm_q / norm_k, inplace.py:760-763) and rotated, so
 * |q . k| <= 128 * max|w_q| * max|w_k|.  With score_bound * log2(e) <= 96 the hand-scheduled kernel then computes
 * P = exp2(s * log2 e) without a running row maximum (no per-tile max, no rescale: ~11 % fewer VALU instructions per KV tile); the
 * result is the same softmax up to fp32 / bf16 rounding.  A bound of 0 (or one that is too large) = rgn_attention.  A violated
 * bound is the caller's error (overflow). */
int rgn_attention_bounded(const void* Q, int ldq, const void* k_slab, const void* vt_slab, int skv_pad, void* O, int ldo,
                          int Sq, int Skv, int H, float scale, float score_bound, void* workspace, size_t workspace_bytes,
                          void* stream);
/* Optional fp32 scratch for the round-aware schedule: (head, q-block) items that do not fill a whole
 * round of the chip's workgroup slots are cut along KV (equal pieces or stream-K runs, chosen per launch) and merged by a
 * combine kernel.  NULL disables the split (results are identical up to fp32 summation order).  The returned size (128 MiB)
 * is a shape-independent upper bound; a smaller buffer limits the piece count.  One workspace per stream. */
size_t rgn_attention_workspace_bytes(int Sq, int H);
/* Introspection of the round-aware schedule (tests, traces; no reference counterpart): the plan of the last rgn_attention* call on this
 * thread / the plan the scheduler WOULD choose for (Sq, Skv, H) with a workspace of `workspace_bytes` (0 = none) - pure host arithmetic,
 * no launch, no GPU.  Bits 0-3 = equal KV pieces of the remainder items (1 = not split), bit 4 = stream-K remainder, bit 5 = 8-wave
 * workgroups (256 query rows; clear = 4 waves x 128 rows for tiny query sets). */
int rgn_attention_last_plan(void);
int rgn_attention_plan_query(int Sq, int Skv, int H, size_t workspace_bytes);

/* ---- f4: VAE decode, the host-side step behind the loop ------------------------------------------------------
 * Replaces `self.vae.decode(latents, return_dict=False)[0]` (reference FluxKontext/inplace.py:396-402; Step1XEdit / Step1XEditV1P2
 * the same call) for the [EXT] AutoencoderKL of the public FLUX.1 / Step1X-Edit checkpoints (16 latent channels, block widths
 * 128-256-512-512, 3 ResNet blocks per up level, one mid-block attention head of width 512, GroupNorm(32, eps 1e-6) + SiLU).
 * Activation layout of every entry: a ZERO-BORDERED pixel-major image [Hp * Wp, C] bf16, Hp = H + 2, Wp = W + 2, row = y * Wp + x of
 * the PADDED image, channels contiguous.  The caller allocates >= Wp + 1 + group rows of readable memory in front of row 0 and behind
 * the last row (guard rows: a 3 x 3 window reads them for border outputs, which are then written as zeros).
 * What a launch reads WITH AN EFFECT on what it stores (tests/test_gpu_conv_probes.py, probe f, holds this with NaN everywhere else):
 *   - the image X itself, border rows included: they must be zero (they are the convolution's padding);
 *   - group = 1, 1 x 1, rgn_conv_s2_bf16 and rgn_conv_up2_bf16: nothing outside the image - guard rows of X may hold anything, NaN
 *     included (the stride-2 launch carries them into its scratch row only);
 *   - 3 x 3 with group > 1: the block-Toeplitz matrix multiplies the whole window of group + 2 pixels per kernel row, its zeros
 *     included, so the up to group - 1 guard rows of X directly in front of row 0 and the up to group - 1 directly behind the last
 *     row are added into INTERIOR outputs of the first / last image row through zero weights: they must hold FINITE values (0 x NaN
 *     is NaN).  Zero-initialised guard rows, the zeros a pixel-group launch writes behind its image and the zeroed scratch row of
 *     rgn_conv_up2_bf16 satisfy this; the scratch row of rgn_conv_s2_bf16 (the first guard row behind ITS output, real convolution
 *     values, racing stores) is finite whenever its input and that input's guard rows are, but is no defined value: do not feed a
 *     stride-2 output to a 3 x 3 pixel-group launch without clearing that row;
 *   - resid: interior pixels only (border and guard rows of the skip image may hold anything);
 *   - Wt / bias: N rows of K values / N values, nothing behind them.
 * What a launch writes: rgn_conv_bf16 every row of the image (border rows as zeros), columns [0, Cout) of each - columns [Cout, ldy)
 * are left untouched for group = 1 and written as zeros for group > 1 - plus, for group > 1, zeros to the rows up to group - 1 behind
 * the image; the table launches only the rows their tables name.
 *
 * rgn_conv_bf16: Y = conv(X, Wt) + bias (+ resid), border rows of Y written as ZEROS.  taps = 9: 3 x 3, stride 1, zero padding 1, as an
 * implicit GEMM on the hand-scheduled MFMA loop (K = 9 Cin in (ky, kx, c) order: inside one kernel row the three taps' channels are
 * contiguous in this layout, so the A tile of a K step is the plain GEMM's at another byte offset); Wt = [Cout, 3, 3, Cin] (the
 * checkpoint's [Cout, Cin, 3, 3] permuted once at load), needs ldx == Cin.  taps = 1: 1 x 1 (ResNet shortcut, attention projections),
 * Wt = [Cout, Cin].  Cin % 64 == 0; resid (or NULL) has Y's layout; fp32 accumulation, one bf16 rounding of acc + bias, one of the
 * residual sum.
 * group > 1 (narrow outputs: Cout = 128, the RGB head): one GEMM row = `group` consecutive pixels, its output row = group x ldy columns, and
 * Wt is the caller-built block-Toeplitz matrix [group * ldy, 3 * (group + 2) * Cin] (taps = 9; row p * ldy + c holds W[c, ky, kx] at
 * window pixel p + kx of kernel row ky, zeros elsewhere and in the padding channels) or [group * ldy, group * Cin] (taps = 1, block
 * diagonal); bias = [group * ldy].  The 256-wide tile is then full: MFMA work (group + 2) / 3 of the ideal instead of 256 / Cout.  Rows of Y
 * up to group - 1 past the image are written (zeros): the caller's guard rows.
 * gn_partial != NULL: the epilogue also leaves the GroupNorm(32) statistics of the STORED image in the caller's groupnorm workspace - per tile
 * 32 x (sum, sum of squares), folded in a fixed order - and writes the tile count to *gn_blocks_host (a HOST int); passing that count as
 * rgn_groupnorm_silu's `precomputed_blocks` skips its statistics pass (one read of the image less per ResNet half). */
int rgn_conv_bf16(const void* X, int ldx, const void* Wt, const void* bias, const void* resid, void* Y, int ldy, int Hp, int Wp,
                  int Cin, int Cout, int taps, int group, float* gn_partial, int* gn_blocks_host, void* stream);
/* The encoder's downsampling convolution (VAE encode of the condition image, inside the host's `prepare_latents`, reference call site
 * FluxKontext/inplace.py:210-226): 3 x 3, stride 2, F.pad(x, (0, 1, 0, 1)) + padding 0.  X = padded image [Hp * Wp, Cin] (even H, W);
 * GEMM row m = yo * Wp + xo on the INPUT pitch (the A row is image row 2 m + Wp + 1: the same loop with a row stride of two pixels);
 * out_rows[m] (int64, (Hp - 2) / 2 * Wp entries, device) = the row of Y it is stored to - the caller's table: the padded row of output
 * pixel (yo, xo) for xo < W / 2, a scratch row for the unused columns of the wide grid.  Wt = [Cout, 3, 3, Cin]; no border test. */
int rgn_conv_s2_bf16(const void* X, const void* Wt, const void* bias, void* Y, int ldy, int Hp, int Wp, int Cin, int Cout,
                     const int64_t* out_rows, void* stream);
/* The decoder's `upsamplers.0` (nearest 2 x upsample, then a 3 x 3 convolution) WITHOUT the upsampled image: every output phase (a, b) of
 * pixel (2y + a, 2x + b) is a 2 x 2 convolution of the LOW-resolution image X [Hp * Wp, Cin] with tap-summed weights (16 / 36 of the FLOPs).
 * Wt4 = [4 phases (a * 2 + b)][Cout, 2, 2, Cin] (caller: kernel row 0 / 1 of phase a = 0 holds w[0] / w[1] + w[2], of a = 1 w[0] + w[1] / w[2];
 * columns alike with b); out_rows4 = [4][Hp * Wp] int64 (device): the row of the high-resolution padded image Y each low-resolution padded pixel's
 * phase is stored to (border pixels: a scratch row; their values are zeroed); Y's own border rows are not written (the caller keeps them
 * zero).  One launch of four problems.  gn_partial / gn_blocks_host as rgn_conv_bf16 (the statistics of all of Y). */
int rgn_conv_up2_bf16(const void* X, const void* Wt4, const void* bias, void* Y, int ldy, int Hp, int Wp, int Cin, int Cout,
                      const int64_t* out_rows4, float* gn_partial, int* gn_blocks_host, void* stream);
/* GroupNorm(32 groups) over the valid pixels + optional SiLU: Y = silu((X - mean_g) * rstd_g * gamma + beta), border rows of Y = 0.
 * C in {128, 256, 512}.  Statistics: per-block fp32 partial sums folded in a fixed order + one double-precision pass (no atomics:
 * bit-reproducible).  `workspace`: rgn_groupnorm_workspace_bytes() bytes, 16-byte aligned, one per stream.  precomputed_blocks > 0: X was
 * written by rgn_conv_bf16 with gn_partial = this workspace, which left that many tiles' sums there: no statistics pass. */
size_t rgn_groupnorm_workspace_bytes(void);
size_t rgn_groupnorm_partial_bytes(void);          /* the leading part of the workspace a convolution's gn_partial may fill */
int rgn_groupnorm_silu(const void* X, void* Y, int Hp, int Wp, int C, const void* gamma, const void* beta, float eps, int silu,
                       void* workspace, int precomputed_blocks, void* stream);
/* Nearest-neighbour 2 x upsample of a padded image [Hp * Wp, C] into the padded image [(2 Hp - 2) * (2 Wp - 2), C] (border zero). */
int rgn_upsample2x(const void* X, void* Y, int Hp, int Wp, int C, void* stream);
/* Mid-block attention = three GEMMs (rgn_gemm_group) + this pass: S [Hp * Wp, ld] holds q . k for every (query, key) pixel of the
 * padded image; in place P = softmax(scale * S) per row over the VALID key columns (border pixels and the padding columns
 * [Hp * Wp, ld) get probability 0).  ld % 8 == 0, ld <= 24576. */
int rgn_softmax_rows(void* S, int ld, int Hp, int Wp, float scale, void* stream);
/* Mid-block attention fused (no score matrix in memory): O = softmax(scale * Q K^T) V + b_v over the VALID pixels of a zero-bordered,
 * pixel-major image.  Q, K, V, O: [Hp * Wp, C] bf16 (row stride C, 16-byte aligned), C in {384, 512}; b_v: [C] bf16 or NULL.  Border
 * pixels are never keys (their K and V rows are not read); border rows of O are NOT written (the `to_out` convolution zeroes them).
 * O may be Q itself (a query's Q row is read before its O row is written, by the same block); it may not overlap K or V.
 * S in fp32 from bf16 operands, online softmax in fp32 (running max, exp2), P rounded to bf16 for the P V MFMA, O accumulated in fp32
 * and rounded to bf16 once; fixed reduction order: a repeated call is bit-identical.  Any Hp, Wp >= 3 (64-bit addressing). */
int rgn_vae_attention_bf16(const void* Q, const void* K, const void* V, const void* b_v, void* O, int Hp, int Wp, int C, float scale,
                           void* stream);
/* z [Cz, H, W] bf16 (one NCHW image) -> padded pixel-major [Hp * Wp, Cpad], channels [Cz, Cpad) and the border zero; and back:
 * the first Co channels of a padded image with row stride ld -> [Co, H, W] bf16. */
int rgn_nchw_to_padded(const void* Z, void* Y, int Cz, int H, int W, int Cpad, void* stream);
int rgn_padded_to_nchw(const void* X, int ld, void* O, int Co, int H, int W, void* stream);
/* The same conversion for the Qwen-Image VAE's outputs: clamp_unit != 0 clamps to [-1, 1] (the decoded image, `torch.clamp(out, -1, 1)`);
 * out_fp32 != 0 stores fp32, else bf16 (the host VAE's dtype). */
int rgn_padded_to_nchw_cvt(const void* X, int ld, void* O, int Co, int H, int W, int clamp_unit, int out_fp32, void* stream);
/* Qwen-Image (Wan-2.1) VAE `RMS_norm` (bias-free) per pixel over the channels, optional SiLU:
 * Y = silu(X / max(||X[:C_valid]||_2, 1e-12) * sqrt(C_valid) * gamma), on a padded image [Hp * Wp, C_pad] (C_pad = row stride, a multiple of
 * 64, <= 512; C_valid <= C_pad, e.g. the 96-channel level stored at 128).  fp32 sum of squares folded in a fixed order (bit-reproducible), one
 * bf16 rounding of the output; border rows and channels >= C_valid of Y are written as zeros.  gamma: [C_pad] bf16, 16-byte aligned. */
int rgn_rms_norm_silu(const void* X, void* Y, int Hp, int Wp, int C_valid, int C_pad, const void* gamma, int silu, void* stream);

/* ------------------------------------------------------------------------------------------
 * f4  text encoders of FLUX.1 Kontext: `encode_prompt` (FluxKontext/inplace.py:185-211) runs [EXT] transformers CLIPTextModel
 * (pooler_output) and T5EncoderModel (last_hidden_state).  Projections are rgn_gemm_group; these are the pieces around it.
 *
 * Self-attention with head dim 64, read straight from the fused QKV GEMM output: QKV [L, 3 H 64] bf16 (columns q | k | v, head-major
 * inside each), O [L, H 64] bf16; both 16-byte aligned.  Per head and query i:
 *   O[i] = softmax_j(scale * q_i . k_j + bias[h][j - i + Lmax - 1]) v_j     over j < L (j <= i when causal != 0)
 * bias: NULL or a bf16 table [H][2 Lmax - 1] (T5's relative-position bias for every offset), L <= Lmax <= 4096.  Scores and the online
 * softmax in fp32, P rounded to bf16 for the P V MFMA, O rounded once; fixed reduction order: a repeated call is bit-identical.
 * 1 <= L <= 4096, 1 <= H <= 1024, 0 < scale < inf (T5: 1; CLIP: 1/8). */
int rgn_text_attention_bf16(const void* QKV, void* O, int L, int H, float scale, int causal, const void* bias, int Lmax, void* stream);
/* out[i, :] = tok[ids[i], :] (+ pos[i, :], one bf16 rounding: CLIP's `token_embedding + position_embedding`); an id outside
 * [0, vocab) gives a zero row (the table is never read out of bounds).  ids int64 [L]; tok [vocab, d], pos [npos, d] (NULL: T5's
 * plain gather; else L <= npos), out [L, d]: bf16, 16-byte aligned, d % 8 == 0. */
int rgn_text_embed(const int64_t* ids, int L, const void* tok, int vocab, const void* pos, int npos, void* out, int d, void* stream);
/* T5 v1.1 gated-GELU product: y[m, f] = bf16(x[m, F + f] * x[m, f]) - x is the output of ONE rgn_gemm_group problem over [wi_1 ; wi_0] with
 * RGN_EPI_GELU from column F (linear half, then GELU-tanh half); `hidden_gelu * hidden_linear` of T5DenseGatedActDense.
 * F % 8 == 0, ldx >= 2 F, ldy >= F (strides multiples of 8), x and y 16-byte aligned. */
int rgn_geglu_bf16(const void* x, int ldx, void* y, int ldy, int M, int F, void* stream);
/* CLIP's quick_gelu on bf16 with the eager op sequence's roundings: t = bf16(1.702 x), s = bf16(sigmoid(t)), y = bf16(x s).  y may be x. */
int rgn_quick_gelu_bf16(const void* x, void* y, size_t n, void* stream);
/* Affine LayerNorm over rows of width d (nn.LayerNorm on bf16): fp32 mean, fp32 variance about it, both in a fixed order,
 * out = bf16(gamma * (rstd * (x - mean)) + beta).  gamma, beta: [d] bf16. */
int rgn_layer_norm_rows(const void* x, int ldx, const void* gamma, const void* beta, void* out, int ldo, int M, int d, float eps,
                        void* stream);
/* CLIPTextModel's pooled row, chosen on the device (no host sync): index = argmax(int32(ids)) when eos_token_id == 2, else the first
 * position with int32(ids) == eos_token_id (0 when there is none); out[:d] = x[index, :d].  ids int64 [L]; x, out bf16. */
int rgn_text_pool_row(const int64_t* ids, int L, int eos_token_id, const void* x, int ldx, int d, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * f4  language model of the Qwen2.5-VL prompt encoder: `encode_prompt` of QwenImageEditPipeline / QwenImageEditPlusPipeline
 * (QwenImageEdit/inplace.py, QwenImageEditPlus/inplace.py) runs [EXT] transformers Qwen2_5_VLForConditionalGeneration.  Projections are
 * rgn_gemm_group, the norms rgn_rms_norm_rows, the embedding rgn_text_embed; these are the pieces around them.
 *
 * Causal grouped-query self-attention with head dim 128, read straight from the fused QKV GEMM output: QKV [L, (Hq + 2 Hkv) 128] bf16
 * (columns q | k | v, head-major inside each), O [L, Hq 128] bf16; both 16-byte aligned.  Query head h uses KV head h / (Hq / Hkv):
 *   O[i, h] = softmax_{j <= i}(scale * q_{i,h} . k_{j,kv(h)}) v_{j,kv(h)}
 * Replaces the attention interface call of Qwen2_5_VLAttention.forward (repeat_kv + softmax(QK^T * scaling + causal mask) V).  Key tiles
 * wholly above the diagonal are skipped.  Scores and the online softmax in fp32, P rounded to bf16 for the P V MFMA, O accumulated in
 * fp32 and rounded once; fixed reduction order: a repeated call is bit-identical.
 * 1 <= L <= 4096, 1 <= Hkv <= Hq <= 1024, Hq % Hkv == 0, 0 < scale < inf (Qwen2.5-VL-7B: Hq 28, Hkv 4, scale 1/sqrt(128)). */
int rgn_lm_attention_bf16(const void* QKV, void* O, int L, int Hq, int Hkv, float scale, void* stream);
/* Multimodal RoPE on the q and k columns (the first (Hq + Hkv) 128 of each row) of that QKV buffer, in place; the v columns are not
 * touched.  cos, sin: bf16 [L, 128], the tables AFTER the mrope_section selection (one row per token, shared by every head).  Replaces
 * `apply_multimodal_rotary_pos_emb(q, k, cos, sin, mrope_section)` with its eager bf16 op sequence, three roundings:
 *   x <- bf16(bf16(x * cos) + bf16(rotate_half(x) * sin)),   rotate_half(x) = [-x[64:], x[:64]] per head.
 * ld = row stride of QKV in elements (>= (Hq + 2 Hkv) 128, a multiple of 8); QKV, cos, sin 16-byte aligned. */
int rgn_mrope_bf16(void* QKV, int ld, const void* cos, const void* sin, int L, int Hq, int Hkv, void* stream);
/* SwiGLU product: y[m, f] = bf16(bf16(silu(x[m, f])) * x[m, F + f]) - x is the output of ONE rgn_gemm_group problem over [gate_proj ; up_proj];
 * `self.act_fn(self.gate_proj(x)) * self.up_proj(x)` of Qwen2MLP.forward with its two roundings.
 * F % 8 == 0, ldx >= 2 F, ldy >= F (strides multiples of 8), x and y 16-byte aligned. */
int rgn_swiglu_bf16(const void* x, int ldx, void* y, int ldy, int M, int F, void* stream);

/* ------------------------------------------------------------------------------------------
 * f4  greedy decode of that language model (`generate`, one new token per step against a KV cache; csrc/decode.hip).  The row kernels
 * above run at M = 1 (rgn_rms_norm_rows, rgn_mrope_bf16 with a one-row table, rgn_swiglu_bf16, rgn_text_embed reading the id from device
 * memory); these are the pieces a one-row step needs besides.  No atomics, fixed reduction orders: a repeated call is bit-identical.
 *
 * One-row linear layer: y[n] = bf16(sum_k W[n,k] x[k] + bias[n]); with resid != NULL y[n] = bf16(bf16(sum + bias) + resid[n]), the two
 * roundings of torch's `h + linear(a)` (what RGN_EPI_GATE_RESID with a gate of ones gives the prefill); y may be resid.  bf16 in, fp32
 * accumulation in a fixed order; W [N, K] row-major and dense, W and x 16-byte aligned, K % 64 == 0; bias may be NULL.  Weights go from
 * global memory straight to registers (8 16-byte loads per lane in flight); HBM-bound on W. */
int rgn_lm_gemv_bf16(const void* W, const void* x, const void* bias, const void* resid, void* y, int N, int K, void* stream);
/* The same one-row linear layer over fp8 weights (ops.quantize_w8: OCP e4m3fn bytes W8 [N, K] dense, one fp32 scale per output channel):
 * v = wscale[n] * sum_k f32(W8[n,k]) x[k] (+ bias[n]) in fp32, y[n] = bf16(v), with resid != NULL y[n] = bf16(bf16(v) + resid[n]); what
 * rgn_gemm_group computes for one row of A with `wscale`.  The conversion is exact (v_cvt_pk_f32_fp8), the scale multiplies the reduced
 * sum once; fixed reduction order, no atomics.  K % 16 == 0, K >= 64; W8, wscale, x and y 16-byte aligned; x, bias, resid, y bf16; y may
 * be resid.  Half the bytes of rgn_lm_gemv_bf16 per row. */
int rgn_lm_gemv_w8(const void* W8, const float* wscale, const void* x, const void* bias, const void* resid, void* y, int N, int K,
                   void* stream);
/* cache[row0 + i, :] = QKV[i, Hq 128 : (Hq + 2 Hkv) 128] for i < L: the k | v columns of packed QKV rows (after rgn_mrope_bf16) into a
 * cache [cap, 2 Hkv 128] bf16, bit for bit.  ld = row stride of QKV in elements; 0 <= row0, row0 + L <= cap <= 4096; QKV and cache 16-byte
 * aligned.  The prefill appends its L rows, a decode step one. */
int rgn_lm_kv_append_bf16(const void* QKV, int ld, void* cache, int cap, int row0, int L, int Hq, int Hkv, void* stream);
/* One query token against the first n rows of that cache: O[h] = softmax_{j < n}(scale * q_h . k_{j,kv(h)}) v_{j,kv(h)}, kv(h) = h / (Hq / Hkv).
 * q: bf16 [Hq 128] (the q columns of the token's QKV row), O: bf16 [Hq 128].  One wave takes one KV head and 64 keys for all Hq / Hkv
 * query heads of the group; scores, softmax and O in fp32; partials (m, l, o[128]) per (head, slice) go to `workspace` and a second
 * kernel folds them in slice order.  Cache rows >= n are never read.  1 <= n <= 4096, Hq % Hkv == 0, Hq / Hkv <= 8, 0 < scale < inf;
 * q, cache, O, workspace 16-byte aligned; workspace_bytes >= rgn_lm_decode_attention_workspace_bytes(Hq, n). */
int rgn_lm_decode_attention_bf16(const void* q, const void* cache, void* O, int n, int Hq, int Hkv, float scale, void* workspace,
                                 size_t workspace_bytes, void* stream);
size_t rgn_lm_decode_attention_workspace_bytes(int Hq, int n);
/* Greedy pick over the vocabulary: z[v] = sum_k W[v,k] x[k] in fp32 (never rounded to bf16: rounding first turns near-ties into ties),
 * token_out[0] = argmax_v z[v] as int64 in device memory, the LOWEST index among equal values.  Per-block (value, index) pairs in
 * `workspace`, then one finalize block.  logits_out != NULL also receives all of z (fp32 [V]).  W [V, K] bf16 dense, W and x 16-byte
 * aligned, K % 64 == 0, token_out 8-byte aligned; workspace_bytes >= rgn_lm_head_workspace_bytes(V). */
int rgn_lm_head_argmax(const void* W, const void* x, int V, int K, void* token_out, float* logits_out, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t rgn_lm_head_workspace_bytes(int V);
/* The same decode step for B sequences at once (`generate` over a batch of up to RGN_LM_MAX_BATCH prompts): every weight is streamed ONCE
 * per step for all of them.  The batch is invariant: row b of each result below is BIT FOR BIT what the one-sequence entry above gives for
 * row b alone, for every B in 1..8 - the same per-lane fmaf chain in the same k order, the same wave butterfly, the same roundings.  No
 * atomics, fixed reduction orders, a repeated call is bit-identical.  The row kernels (rgn_rms_norm_rows, rgn_mrope_bf16, rgn_swiglu_bf16,
 * rgn_text_embed) run at M = B.  Per-sequence lengths are HOST arrays of B ints that travel to the kernel by value: no device read, no upload.
 * B = 1 of a `_rows` entry IS the one-sequence entry above: the same checks, the same kernels with the same grid, so a decode loop calls
 * the `_rows` entries for every B.  No stride is read at B = 1 (one row has none), so the stride conditions below bind from B = 2 on.
 *
 * Y[b, n] = the layer of rgn_lm_gemv_bf16 applied to row b of X, b < B.  X [B, ldx], Y [B, ldy], resid [B, ldr] bf16; strides in elements,
 * multiples of 8, ldx >= K, ldy >= N, ldr >= N; Y may be resid.  Rows >= B and columns >= N are never written.  A weight vector is loaded
 * once (non-temporal) and converted once for all rows; x is widened to fp32 once per block and kept in LDS (B x 8 KB). */
#define RGN_LM_MAX_BATCH 8
int rgn_lm_gemv_bf16_rows(const void* W, const void* X, int ldx, const void* bias, const void* resid, int ldr, void* Y, int ldy, int B, int N,
                          int K, void* stream);
/* The same over fp8 weights: row b bit-identical to rgn_lm_gemv_w8 on X[b] (exact v_cvt_pk_f32_fp8, the scale once on the reduced sum). */
int rgn_lm_gemv_w8_rows(const void* W8, const float* wscale, const void* X, int ldx, const void* bias, const void* resid, int ldr, void* Y,
                        int ldy, int B, int N, int K, void* stream);
/* rgn_lm_head_argmax for B rows of X from one stream of W: token_out[b * token_stride] (int64 elements) = the argmax of row b, the lowest
 * index on a tie; logits_out != NULL receives fp32 [B, V] with row stride ldl >= V.  The finalize step runs one block per row.
 * workspace_bytes >= B * rgn_lm_head_workspace_bytes(V). */
int rgn_lm_head_argmax_rows(const void* W, const void* X, int ldx, int B, int V, int K, void* token_out, int token_stride, float* logits_out,
                            int ldl, void* workspace, size_t workspace_bytes, void* stream);
/* Row b of QKV [B, ld] (after rgn_mrope_bf16) into cache b = cache + b * cache_stride (elements; a multiple of 8, >= cap 2 Hkv 128) at row
 * row0_host[b], 0 <= row0_host[b] < cap <= 4096, bit for bit.  B = 1 is rgn_lm_kv_append_bf16 with L = 1. */
int rgn_lm_kv_append_bf16_rows(const void* QKV, int ld, void* cache, size_t cache_stride, int cap, const int* row0_host, int B, int Hq, int Hkv,
                               void* stream);
/* B query tokens, query b (row b of Q [B, ldq]: the q columns of its QKV row) against the first n_host[b] rows of cache b; O [B, ldo].
 * 1 <= n_host[b] <= 4096.  One grid with the batch on its z axis, sized for the longest cache: a block whose 64-key slice lies at or past
 * n[b] returns before any barrier.  Partials and the merge are per row; row b is bit-identical to rgn_lm_decode_attention_bf16 at n[b], and
 * cache rows >= n[b] are never read.  workspace_bytes >= B * rgn_lm_decode_attention_workspace_bytes(Hq, max_b n[b]). */
int rgn_lm_decode_attention_bf16_rows(const void* Q, int ldq, const void* cache, size_t cache_stride, void* O, int ldo, const int* n_host, int B,
                                      int Hq, int Hkv, float scale, void* workspace, size_t workspace_bytes, void* stream);
/* R query tokens of ONE sequence against ONE cache (a step that verifies R - 1 drafted tokens; HipQwen25VLTextEncoder(lookup=True)):
 * query r (row r of Q [R, ldq]) sees cache rows [0, n0 + r); O [R, ldo].  1 <= R <= RGN_LM_MAX_BATCH, n0 >= 1, n0 + R - 1 <= 4096.  Row r
 * is BIT FOR BIT rgn_lm_decode_attention_bf16(Q + r ldq, cache, ..., n = n0 + r): the same 64-key slices, per-thread fmaf chains, quad and
 * wave folds and wave order; the merge runs over that row's own ceil((n0 + r) / 64) slices in slice order; a key at or past a row's length
 * has score -inf, p = 0 and v = 0.  One block per (slice, KV head) loads its K and V once and walks the queries that own the slice, so the
 * cache is read once, in two launches.  Cache rows >= n0 + R - 1 are never read.  ldq, ldo multiples of 8 and >= Hq 128; Q, cache, O,
 * workspace 16-byte aligned; workspace_bytes >= R * rgn_lm_decode_attention_workspace_bytes(Hq, n0 + R - 1). */
int rgn_lm_verify_attention_bf16(const void* Q, int ldq, const void* cache, void* O, int ldo, int n0, int R, int Hq, int Hkv, float scale,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* The end of such a step, ONE block: accept, then propose.  seq: int64 ids of one sequence in one run (prompt, then new tokens);
 * seq[0, n) settled, seq[n - 1] was row 0 of the step, seq[n, n + R - 1) the drafts that were rows 1..R-1; head[r * head_stride] (int64)
 * the argmax after row r.
 *   accept   a = the largest a <= R - 1 with seq[n + i] == head[i] for all i < a (the first mismatch decides); seq[n + a] = head[a];
 *            n' = n + a + 1.
 *   propose  kcap = max(0, min(K, limit - n' - 1)), `limit` the end of the new-token run.  guess == NULL: the rule of transformers'
 *            PromptLookupCandidateGenerator over seq[0, n'): n-gram sizes from min(max_ngram, n' - 1) down to 1; per size the LOWEST
 *            window index idx whose window equals the trailing n-gram and whose continuation [idx + size, min(idx + size + kcap, n')) is
 *            not empty; those k' ids go to seq[n', n' + k'); no match: k' = 0.  guess != NULL (int64 [guess_len], a guess of the whole
 *            continuation, L the prompt length): draft i = guess[(n' - L) + i] while that index is < guess_len, at most kcap.
 *   result   int64 [2 + R]: a, k', then the a + 1 accepted tokens.
 * Nothing outside seq[n, limit) and result[0, 2 + R) is written; no atomics, plain vector stores.  1 <= R <= 32, 0 <= K <= 31,
 * 1 <= max_ngram <= 8, 0 <= L <= n, n >= 1, n + R <= limit; pointers 8-byte aligned. */
int rgn_lm_lookup_step(void* seq, int n, int R, const void* head, int head_stride, int limit, int K, int max_ngram, const void* guess,
                       int guess_len, int L, void* result, void* stream);
/* rgn_lm_lookup_step for a step whose head[r] is the PICK after row r (rgn_lm_pick_verify) instead of the argmax: the same accept, propose
 * and `result`, and then seen[seq[n + i]] = 1 for 0 <= i <= a with the id inside [0, V) - the a accepted drafts and the step's own token,
 * i.e. what the plain sampled loop's picks would have marked.  A rejected draft marks nothing, an id outside [0, V) marks nothing.  Still
 * ONE block, plain byte stores.  seen == NULL is rgn_lm_lookup_step exactly (V is not read); with a map 1 <= V <= 1048576. */
int rgn_lm_lookup_step_mark(void* seq, int n, int R, const void* head, int head_stride, int limit, int K, int max_ngram, const void* guess,
                            int guess_len, int L, void* result, void* seen, int V, void* stream);
/* The WIDE step (opt-in; HipQwen25VLTextEncoder(batch_kernels="mfma")): the three weight-streaming layers for 1 <= B <=
 * RGN_LM_MAX_WIDE_BATCH rows as a skinny GEMM on v_mfma_f32_16x16x32_bf16 (csrc/decode.hip: lm_gemm_rows_kernel).  Every weight byte is loaded
 * from HBM once per call for all rows (16-byte non-temporal loads straight into the MFMA B operand); the rows of X are staged once per block
 * in LDS as bf16 and read as A fragments, rows >= B of a 16-row tile are zero and never written out.
 * k order: a block owns 16 weight rows and walks K in chunks of 1024; wave w of 4 owns k in [256 w, 256 w + 256) of a chunk, 8 MFMAs; MFMA m
 * reads, as element j of lane group g = lane / 16, k = 32 m + 8 g + j of those 256 for bf16 weights and k = 64 (m / 2) + 16 g + 8 (m % 2) + j
 * for fp8 weights (a 16-byte load holds 16 of them), X under the same map.  The four waves' fp32 partial sums are folded in LDS in wave order;
 * no atomics, a repeated call is bit-identical.  None of this reads B: row b's result depends on (W, scale, bias, X[b], resid[b], N, K)
 * only - not on B, not on what the other rows hold - and B = 1 runs the same kernel.  The sums differ from the `_rows` entries' in the last
 * bits (another summation order), which is why this is a path of its own and not a replacement.
 *
 * Y[b, n] = bf16(sum_k W[n, k] X[b, k] + bias[n]), or with resid bf16(bf16(sum + bias) + resid[b, n]) (the two roundings of
 * rgn_lm_gemv_bf16).  W [N, K] bf16 dense row-major, K % 64 == 0, K >= 64, N >= 1; strides as for rgn_lm_gemv_bf16_rows (elements, multiples
 * of 8, ldx >= K, ldy >= N, ldr >= N, binding from B = 2 on); W and X 16-byte aligned; Y may be resid.  Columns >= N are never written. */
#define RGN_LM_MAX_WIDE_BATCH 32
int rgn_lm_gemm_rows_bf16(const void* W, const void* X, int ldx, const void* bias, const void* resid, int ldr, void* Y, int ldy, int B, int N,
                          int K, void* stream);
/* The same over ops.quantize_w8 weights (OCP e4m3fn bytes, one fp32 scale per output channel): each byte is converted in registers to the
 * bf16 that equals it (e4m3fn is a subset of bf16) and goes through the same MFMA; wscale[n] multiplies the folded fp32 sum once:
 * v = fma(sum, wscale[n], bias[n]). */
int rgn_lm_gemm_rows_w8(const void* W8, const float* wscale, const void* X, int ldx, const void* bias, const void* resid, int ldr, void* Y,
                        int ldy, int B, int N, int K, void* stream);
/* lm_head over B <= 32 rows on the same kernel: fp32 logits, never rounded to bf16; token_out[b * token_stride] (int64) = the argmax of row
 * b, the LOWEST index among equal values; logits_out != NULL receives fp32 [B, V] with row stride ldl >= V.  One maximum per block of 16
 * vocabulary rows and sequence goes to the workspace; the finalize step runs one block per row.
 * workspace_bytes >= rgn_lm_head_wide_workspace_bytes(V, B). */
int rgn_lm_head_argmax_wide(const void* W, const void* X, int ldx, int B, int V, int K, void* token_out, int token_stride, float* logits_out,
                            int ldl, void* workspace, size_t workspace_bytes, void* stream);
size_t rgn_lm_head_wide_workspace_bytes(int V, int B);
/* rgn_lm_pick_rows for 1 <= B <= RGN_LM_MAX_WIDE_BATCH rows in ONE launch: the same kernel, one block per row, so up to 32 CUs pick side by
 * side (groups of 8 rows through rgn_lm_pick_rows run one after another: 2.2 ms a step at 32 rows against 0.5).  Row b is bit for bit
 * rgn_lm_pick on row b alone; every other rule is rgn_lm_pick_rows'.  B = 1 is rgn_lm_pick's one-block launch. */
int rgn_lm_pick_wide(const float* logits, int ldl, int B, int V, void* seen, size_t seen_stride, float penalty, int sample, float temperature,
                     int top_k, double top_p, const float* uniform, void* token_out, int token_stride, float* scores_out, int lds,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Repetition penalty and sampling for that decode (transformers' RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
 * TopKLogitsWarper, TopPLogitsWarper and the multinomial draw, in the order of _get_logits_processor).
 *
 * seen[ids[i]] = 1 for i < n: the byte map [V] of the token ids of the sequence so far (int64 ids, 8-byte aligned; an id outside [0, V)
 * marks nothing).  Plain byte stores, no atomics.  Called once per generate over the whole prompt, image placeholders included, after
 * rgn_fill_zero; rgn_lm_pick marks every token it picks. */
int rgn_lm_seen_mark(const void* ids, int n, void* seen, int V, void* stream);
/* One pick over the fp32 logits z [V] that rgn_lm_head_argmax(..., logits_out) wrote, in ONE launch of one block; z is not modified.
 *   1. penalty p > 0 over seen: z < 0 ? z * p : z / p (fp32, once per token id); p == 1 skips the stage
 *   2. sample != 0: s = z / temperature in fp32 (IEEE division); sample == 0 skips stages 2 to 4
 *   3. top_k > 0: every s[v] below the k-th largest VALUE becomes -inf; ties with the k-th value stay (0, or k >= V: off)
 *   4. top_p < 1: with softmax(s) over what is left, in ascending order of s, a token is dropped while the mass up to and including it
 *      and every token of the same score is <= 1 - top_p; the largest is never dropped (min_tokens_to_keep = 1).  Equal scores are kept
 *      or dropped TOGETHER; transformers' sort splits such a group when it straddles the boundary, this entry keeps all of it.
 *   5. sample == 0: token = argmax, the lowest index on a tie.  sample != 0: q = softmax over the kept tokens, token = the lowest kept
 *      index v with sum_{w <= v} q[w] > uniform[0] (u in [0, 1), fp32 in device memory; the entry has no generator of its own), the
 *      last kept token if rounding leaves none.  token_out[0] = token as int64, seen[token] = 1.
 *   6. scores_out != NULL receives the processed scores (fp32 [V], -inf where filtered); it may not be z.
 * The k-th value and the top-p threshold come from radix selects over the key bits of s (4 bits a round, per-thread fp64 bins in LDS
 * folded in a fixed order), the draw from fp64 wave sums per 64 tokens and a block scan in token order: no atomics, no sort, a repeated
 * call is bit-identical.  Masses are expf(s - max) in fp32 summed in fp64: a cumulative mass is within 2^-23 (ln V + 6) of the exact
 * one (expf taken at 3 ulp).  1 <= V <= 1048576; token_out 8-byte, z / scores_out / workspace / uniform 4-byte aligned;
 * workspace_bytes >= rgn_lm_pick_workspace_bytes(V).  temperature, top_k and top_p are validated whatever `sample` is. */
int rgn_lm_pick(const float* logits, int V, void* seen, float penalty, int sample, float temperature, int top_k, double top_p,
                const float* uniform, void* token_out, float* scores_out, void* workspace, size_t workspace_bytes, void* stream);
size_t rgn_lm_pick_workspace_bytes(int V);
/* rgn_lm_pick for the B rows of a batched decode step, one configuration for all of them: row b reads logits + b * ldl (fp32 [B, ldl], what
 * rgn_lm_head_argmax_rows(..., logits_out, ldl) wrote), the byte map seen + b * seen_stride (bytes) and uniform[b] (fp32 [B], this step's;
 * read only when sample != 0), writes token_out[b * token_stride] (int64 elements) and, with scores_out != NULL, row b of scores_out
 * [B, lds], and sets seen_b[token] = 1.  ONE launch, one block per row: a block is the 16-wave block of rgn_lm_pick with its 128 KB of
 * LDS, so it has a CU to itself and up to RGN_LM_MAX_BATCH CUs work side by side.  Blocks never communicate: no atomics, no reduction
 * across rows.  Row b's result - the token, the processed scores, the seen bytes - is BIT FOR BIT what rgn_lm_pick gives for row b
 * alone, for every B in 1..8 (both kernels run the same device function).  Rows >= B and columns >= V of every buffer are never written,
 * the logits never at all.  1 <= B <= RGN_LM_MAX_BATCH; ldl >= V, lds >= V (with scores_out), seen_stride >= V, token_stride >= 1; the
 * ranges and alignments of rgn_lm_pick; scores_out may not overlap the logits; workspace_bytes >= B * rgn_lm_pick_workspace_bytes(V).
 * B = 1 is rgn_lm_pick itself (its one-block launch; no stride is read), except that this entry still refuses any overlap.
 * Every refusal is raised before the launch.  The prompt ids of row b are marked by rgn_lm_seen_mark on seen + b * seen_stride. */
int rgn_lm_pick_rows(const float* logits, int ldl, int B, int V, void* seen, size_t seen_stride, float penalty, int sample, float temperature,
                     int top_k, double top_p, const float* uniform, void* token_out, int token_stride, float* scores_out, int lds,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The picks of a VERIFICATION step (HipQwen25VLTextEncoder(lookup=True, sampling=True, lookup_sampling=True)): the R rows are the last
 * settled token and R - 1 drafted tokens of ONE sequence, drafts int64 [R - 1].  Row r reads logits + r * ldl and uniform[r] and picks
 * under the byte map  seen U {drafts[i] : i < r, 0 <= drafts[i] < V}  - the map the plain loop has at that position exactly when drafts
 * 0..r-1 were accepted, which is when row r counts at all; it is known before the step runs, so the R picks are independent.  Row r's
 * token (token_out[r * token_stride]) and processed scores (row r of scores_out [R, lds]) are BIT FOR BIT what rgn_lm_pick gives on that
 * row with a map holding exactly those marks: the block runs the device function of rgn_lm_pick with this membership test in its first
 * pass and without its final store.  A membership: an id is penalised once however often it occurs (in `seen` and drafted, or drafted
 * twice).  `seen` is NEVER written (rgn_lm_lookup_step_mark marks what the step settles), the logits never, rows >= R and columns >= V of
 * no buffer.  ONE launch, one block per row (the 16-wave block with its 128 KB of LDS, a CU each), plain vector stores, no atomics, blocks
 * never communicate.  1 <= R <= RGN_LM_MAX_WIDE_BATCH; R = 1 reads no draft (drafts may be NULL).  Every refusal is rgn_lm_pick_rows'
 * (ranges, alignments, scores_out may not overlap the logits, workspace_bytes >= R * rgn_lm_pick_workspace_bytes(V)) plus drafts non-null
 * and 8-byte aligned when R > 1, raised before the launch. */
int rgn_lm_pick_verify(const float* logits, int ldl, int R, int V, const void* seen, const void* drafts, float penalty, int sample,
                       float temperature, int top_k, double top_p, const float* uniform, void* token_out, int token_stride, float* scores_out,
                       int lds, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * f4  vision tower of the Qwen2.5-VL prompt encoder ([EXT] transformers Qwen2_5_VisionTransformerPretrainedModel: `get_image_features`
 * of the encode_prompt above).  Projections (the patch embedding included) are rgn_gemm_group, the norms rgn_rms_norm_rows, the MLP
 * product rgn_swiglu_bf16, the window reorder rgn_gather_rows / the GEMM's out_rows; these are the pieces around them (csrc/vision.hip).
 *
 * Non-causal self-attention over packed segments (the windows of a window block, one segment per image of a full-attention block), read
 * straight from the fused QKV GEMM output: QKV [L, 3 H Dp] bf16 (all q heads | all k heads | all v heads), O [L, H Dp] bf16.  Dp in
 * {32, 64, 96, 128} is the head width padded with ZERO columns to a multiple of 32 (zero weight rows and bias entries: the dot products
 * and the real output columns are unchanged, the output's pad columns are exactly 0); `scale` is the caller's (real width ^ -0.5).
 * items: int32 [n_items, 4] on the device = (q0, n_q, k_lo, k_hi): queries [q0, q0 + n_q), 1 <= n_q <= 64, attend to keys [k_lo, k_hi);
 * one workgroup per (item, head).  The kernel relates queries to keys through the item alone: the vision tower names a segment as the
 * key range of its own queries (no item crosses a segment), the Step1X connector names keys [0, n_valid) for runs of valid rows and key
 * 0 alone, (q0, n_q, 0, 1), for runs of padded rows, whose output is then v[0] of the head bit for bit.  An item outside [0, L) is
 * skipped; rows no item names are not written.  Replaces the per-chunk attention interface calls of Qwen2_5_VLVisionAttention.forward.  Arithmetic and determinism as
 * rgn_lm_attention_bf16 (same tile core).  QKV, O, items 16-byte aligned; 1 <= H <= 1024; 0 < scale < inf. */
int rgn_vision_attention_bf16(const void* QKV, void* O, int L, int H, int Dp, float scale, const int* items, int n_items, void* stream);
/* apply_rotary_pos_emb_vision on the q and k columns (the first 2 H Dp of each row) of that QKV buffer, in place:
 *   x <- bf16(f32(x) * cos + f32(rotate_half(x)) * sin),   rotate_half(x) = [-x[D/2:], x[:D/2]] per head over the REAL width D
 * both products and the sum rounded to fp32, one rounding to bf16 (bit-equal to the eager op).  cos, sin: fp32 [L, D], one row per token.
 * Columns D..Dp of each head and the v columns are not written.  D % 8 == 0, Dp >= D with Dp % 32 == 0, ld >= 3 H Dp (a multiple of 8);
 * QKV, cos, sin 16-byte aligned. */
int rgn_vision_rope_bf16(void* QKV, int ld, const float* cos, const float* sin, int L, int H, int D, int Dp, void* stream);
/* nn.GELU() in its exact form on bf16: y = bf16(0.5 x (1 + erf(x / sqrt 2))) in fp32 (the patch merger; RGN_EPI_GELU is the tanh form).
 * y may be x. */
int rgn_gelu_erf_bf16(const void* x, void* y, size_t n, void* stream);
/* y[m, :K] = bf16(x[m, :K]), y[m, K:Kp] = 0: x [M, K] fp32 (RGN_F32) or bf16 (RGN_BF16) with row stride ldx, y [M, Kp] bf16 contiguous,
 * 16-byte aligned, Kp % 8 == 0.  `pixel_values.to(bfloat16)` padded to a GEMM reduction width (K = 1176 -> Kp = 1216). */
int rgn_cast_pad_rows(const void* x, int x_dtype, int ldx, void* y, int M, int K, int Kp, void* stream);

/* ------------------------------------------------------------------------------------------
 * f4  Step1X-Edit's per-step `connector` ([EXT] Qwen2Connector, a token refiner conditioned on the timestep; Step1XEdit/inplace.py:514-516,
 * Step1XEditV1P2/inplace.py:602-609 call it once per CFG branch per computed step).  Projections are rgn_gemm_group, the embedders
 * rgn_gemv_bf16, the norms rgn_layer_norm_rows, the attention rgn_vision_attention_bf16 with Dp = 128; these are the row kernels around
 * them (csrc/connector.hip).  No atomics, fixed reduction orders: a repeated call is bit-identical.
 *
 * The pooled context `(x * m).sum(1) / m.sum(1)` for a mask of n_valid leading ones, times a scalar:
 *   out[c] = bf16(bf16(sum_{l < n_valid} x[l, c] / n_valid) * scale),   the sum in fp32
 * scale = 1 gives the plain mean (the inner rounding is then the only one).  x [L, d] bf16 with row stride ldx, out [d] bf16; d % 8 == 0,
 * ldx >= d (a multiple of 8), 1 <= n_valid <= L, scale finite; x and out 16-byte aligned.  Rows >= n_valid are not read. */
int rgn_masked_mean_rows(const void* x, int ldx, int L, int d, int n_valid, float scale, void* out, void* stream);
/* Per-head RMSNorm of width 128 on the q and k columns (the first 2 H 128) of packed QKV rows [L, 3 H 128], in place; the v columns and
 * anything past them up to ld are not written.  x <- bf16(bf16(x * rsqrt(mean x^2 + eps)) * w), w = wq for the q heads and wk for the k
 * heads (bf16 [128] each): the roundings, and the summation order, of rgn_rms_norm_rows on the heads as [L H, 128] rows - bit-equal to
 * it.  rgn_qk_norm_rope_store without RoPE and without the slabs.  ld >= 3 H 128 (a multiple of 8), 1 <= H <= 1024, 0 <= eps < inf; QKV,
 * wq, wk 16-byte aligned. */
int rgn_head_rms_norm_bf16(void* QKV, int ld, const void* wq, const void* wk, int L, int H, float eps, void* stream);
/* y[m, n] = bf16(f32(resid[m, n]) + f32(bf16(gate[n] * p[m, n]))): the elementwise half of RGN_EPI_GATE_RESID, for a projection p that
 * was computed once (bias included, rounded to bf16) and a gate that changes per step - bit-equal to the fused epilogue on the same
 * p.  p, resid, y [M, N] bf16 with row strides ldp, ldr, ldy (>= N, multiples of 8), gate bf16 [N]; N % 8 == 0; all 16-byte aligned.
 * y may be resid. */
int rgn_gate_resid_rows(const void* p, int ldp, const void* gate, const void* resid, int ldr, void* y, int ldy, int M, int N, void* stream);

/* ------------------------------------------------------------------------------------------
 * a10  one masked MMDiT block per call (csrc/block.hip: host code only, no kernel of its own).  The entries make the launches the
 * harness blocks make (regione_amd/harness/flux.py, FUSE_QKV path), in their order and with their arguments, through the library's own
 * rgn_ln_modulate, rgn_gemm_group (RGN_EPI_QKV / RGN_EPI_GELU / RGN_EPI_GATE_RESID), rgn_attention_bounded and rgn_rowband_*: a caller
 * needs neither the launch order, nor the buffer layout, nor the K / V^T slab protocol, nor the row-band rules.
 *
 * Buffers (caller-owned, bf16, rows [text 0..T) ; image T..T+M)): x [T+M, d] the residual stream, updated in place; nrm [T+M, d]
 * scratch (LN-modulate output); wide [T+M, 3 d + d_ff] scratch, columns [k | v | q | mlp] (K and V columns are never written: they go
 * to the slabs).  heads * 128 == d.
 * AdaLN vectors (bf16, Modulation.chunk order): double block adaln / adaln_txt = [6 d] of the image / text stream =
 * (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp); single block adaln = [3 d] = (shift, scale, gate), adaln_txt unused.
 * Weights: rgn_block_weight = (W, wscale, bias) with wscale != NULL meaning fp8 exactly as in rgn_gemm_problem; every W is dense.
 *   double: w_kvq / w_add_kvq [3 d, d] (rows k | v | q), w_out / w_add_out [d, d], ff_w1 / ffc_w1 [d_ff, d], ff_w2 / ffc_w2 [d, d_ff]
 *           (the `add` / `ffc` ones belong to the text stream); norm_q, norm_k, norm_added_q, norm_added_k [128];
 *   single: w_kvqm [3 d + d_ff, d] (rows k | v | q | mlp), w_po [d, d + d_ff]; norm_q, norm_k.
 * K / V destination, as the attention processor's kv_target returns it: k_slab [skv_pad, d], vt_slab [d, skv_pad], attention over the
 * first skv rows.  kv_rows == NULL: identity rows (a plain or a store step; skv_pad >= T + M).  kv_rows != NULL (int64 [T + M]): a
 * partial update, the K / V columns take the fp16 round trip (fp16_roundtrip = 1: every row of a single block, the image rows of a
 * double block).  cos_q / sin_q: rotary rows of this call's rows; cos_k / sin_k: rotary rows by CACHE row.
 * score_bound: as rgn_attention_bounded (0 = running maximum).  gemm_ws / attn_ws: the workspaces of rgn_gemm_group / rgn_attention,
 * same rules (NULL = plain launches, one per stream).
 * rowbands = 1: rgn_rowband_join(stream) before the attention and rgn_rowband_fork(stream) behind it, so that the row-wise stages from
 * there to the next block's attention run as two bands; the caller joins behind the last block of the chain.
 * RGN_E_UNSUPPORTED (these stay with the caller): an odd head count, out_rows != 0 (the row-skipping last block), branches != 1
 * (several CFG branches in one call).  Bad arguments (a NULL buffer, d % 64, d_ff % 64, heads * 128 != d, T < 0, M <= 0, a pointer that
 * is not 16-byte aligned, a stride that is no multiple of 8, skv_pad % 64, skv_pad < skv, skv < 1) give RGN_E_BADARG before any launch.
 * Zero the descriptor first: the fields a block kind does not read (single block: adaln_txt, norm_added_q / k and the eight double-block
 * weights; double block: w_kvqm, w_po) must be NULL - the pointer checks run over the whole struct, so garbage there is RGN_E_BADARG.
 * M is explicit (not derived from the buffers): x, nrm and wide may hold more rows than the T + M this call uses.
 *
 * rgn_mmdit_double_block replaces FluxTransformerBlock.forward [EXT] with RegoionEFluxAttnProcessor2_0.__call__ inside it,
 *   FluxKontext/inplace.py:518-524 (call site) and :704-824: LN-modulate (two segments) -> Q/K/V pair with the fused epilogue ->
 *   attention -> output-projection pair (gate + residual) -> LN-modulate -> FF-up pair (GELU) -> FF-down pair (gate + residual).
 * rgn_mmdit_single_block replaces FluxSingleTransformerBlock.forward [EXT], FluxKontext/inplace.py:549-555 and :704-824:
 *   LN-modulate -> fused k | v | q | mlp GEMM -> attention -> proj_out (gate + residual).
 * rgn_mmdit_block_bytes() = sizeof(rgn_mmdit_block) as the library sees it (a binding compares it at load). */
typedef struct rgn_block_weight {
    const void* W;
    const float* wscale;
    const void* bias;
} rgn_block_weight;
typedef struct rgn_mmdit_block {
    void* x; void* nrm; void* wide;
    int ldx, ldnrm, ldwide;
    int T, M, d, d_ff, heads;
    const void* adaln; const void* adaln_txt;
    rgn_block_weight w_kvq, w_add_kvq, w_out, w_add_out, ff_w1, ffc_w1, ff_w2, ffc_w2;     /* double block */
    rgn_block_weight w_kvqm, w_po;                                                         /* single block */
    const void* norm_q; const void* norm_k; const void* norm_added_q; const void* norm_added_k;
    void* k_slab; void* vt_slab;
    const int64_t* kv_rows;
    const float* cos_q; const float* sin_q; const float* cos_k; const float* sin_k;
    int skv, skv_pad;
    float score_bound;
    int rowbands;
    int out_rows;              /* 0; anything else asks for the row-skipping last block: RGN_E_UNSUPPORTED */
    int branches;              /* 1; anything else asks for several CFG branches in one call: RGN_E_UNSUPPORTED */
    void* gemm_ws; size_t gemm_ws_bytes;
    void* attn_ws; size_t attn_ws_bytes;
} rgn_mmdit_block;
int rgn_mmdit_double_block(const rgn_mmdit_block* b, void* stream);
int rgn_mmdit_single_block(const rgn_mmdit_block* b, void* stream);
size_t rgn_mmdit_block_bytes(void);

/* ------------------------------------------------------------------------------------------
 * a11  LoRA merge into a bf16 weight (csrc/lora.hip; no reference counterpart: the reference runs whatever modules the host pipeline
 * holds, PEFT side paths included).  Adoption-time work, never on the per-step path:
 *   dst[n, k] = bf16_rne(t),   t = f32(W[n, k]);   for each term in order:  acc = 0;  for r ascending: acc = fmaf(B[n, r], A[r, k], acc);
 *                                                                           t = fmaf(scale, acc, t)
 * One rounding to bf16 per element; the delta is never rounded on its own; fixed order, no atomics: a repeated call is bit-identical.
 * dst, W [N, K] bf16 with row strides ldd, ldw in elements (>= K, multiples of 8): a destination may be a row range of a packed tensor.
 * dst == W with ldd == ldw is the in-place form (every element is read once and written once by the same lane); any other overlap
 * of dst with W is undefined.  `terms` is a HOST array of n_terms descriptors read at call time; A [r, K] and B [N, r] are dense
 * row-major fp32 DEVICE tensors (A 16-byte aligned).  1 <= n_terms <= RGN_LORA_MAX_TERMS, 1 <= r <= RGN_LORA_MAX_RANK, K % 8 == 0,
 * dst and W 16-byte aligned; N == 0 returns 0 without looking further.  Every refusal is RGN_E_BADARG before any launch. */
#define RGN_LORA_MAX_TERMS 8
#define RGN_LORA_MAX_RANK 1024
typedef struct rgn_lora_term {
    const float* A;            /* [r, K] */
    const float* B;            /* [N, r] */
    int r;
    float scale;
} rgn_lora_term;
int rgn_lora_merge_bf16(void* dst, int ldd, const void* W, int ldw, int N, int K, const rgn_lora_term* terms, int n_terms, void* stream);

/* ------------------------------------------------------------------------------------------
 * a12  Image pre- and post-processing around the VAEs and the vision tower (csrc/image.hip; no reference counterpart: the reference
 * leaves this to the host pipeline's PIL / numpy / torch code).  The contract of every entry is EQUALITY OF BITS with that host code;
 * integer and table arithmetic, one writer per output element, no atomics: a repeated call is bit-identical.  Images are uint8
 * [H, W, 3] (interleaved RGB, dense); src / dst / X pointers are 16-byte aligned, except the src of rgn_image_patchify_u8, which is
 * read byte by byte and may sit anywhere; at most 2^28 pixels per image (RGN_E_UNSUPPORTED).
 * Every other refusal is RGN_E_BADARG before any launch.
 *
 * rgn_image_resample_u8: ONE separable pass of Pillow's 8-bit resampler.  axis 0 resamples along x (src [in_h, in_w, 3] ->
 * dst [in_h, out_w, 3]), axis 1 along y (-> dst [out_h, in_w, 3]); the other dimension must not change.  Per output index i of the
 * resampled dimension the DEVICE tables give bounds[2 i] = first, bounds[2 i + 1] = count (int32) and weights[i * ksize + k], k < count
 * (int32, 22-bit fixed point; the host builds them in float64 as Pillow's precompute_coeffs + normalize_coeffs_8bpc do):
 *   acc = 1 << 21;  for k < count: acc += src[first + k] * weights[i, k];  dst = clip(acc >> 22, 0, 255)       (int32, arithmetic shift)
 * A table entry outside the input (first < 0, count < 0, count > ksize, first + count > size) reads nothing and stores 0.  A resize is
 * the x pass into a uint8 intermediate, then the y pass; the caller skips a pass whose size does not change, as Pillow does. */
int rgn_image_resample_u8(const void* src, int in_h, int in_w, void* dst, int out_h, int out_w, const void* bounds, const void* weights,
                          int ksize, int axis, void* stream);
/* dst[c, y, x] = table[src[y, x, c]]: uint8 [H, W, 3] -> bf16 [1, 3, H, W] through a 256-entry bf16 DEVICE table (the caller builds it
 * with the host's own expression, e.g. 2 * (v / 255) - 1 in fp32 rounded to bf16). */
int rgn_image_u8_to_nchw_bf16(const void* src, void* dst, int H, int W, const void* table, void* stream);
/* The patch rows of the Qwen2-VL image processor (patch 14, merge 2, temporal 2 with the one frame duplicated) from uint8 [H, W, 3], H and
 * W positive multiples of 28: N = (H / 14) (W / 14) rows; row ((bh * (W / 28) + bw) * 2 + ih) * 2 + iw is the patch (2 bh + ih, 2 bw + iw),
 * column ((c * 2 + t) * 14 + dy) * 14 + dx = table[c * 256 + byte] (table: fp32 [3, 256] on the device, the processor's
 * rescale-then-normalise of every byte).  out_bf16 = 0: dst fp32 [N, 1176], ldo = 1176 (what the processor returns); out_bf16 = 1: dst
 * bf16 [N, ldo], ldo >= 1176 a multiple of 8, columns [1176, ldo) zero (what rgn_cast_pad_rows makes of the fp32 rows). */
int rgn_image_patchify_u8(const void* src, int H, int W, const void* table, void* dst, int out_bf16, int ldo, void* stream);
/* A decoded bf16 image -> uint8 [H, W, 3].  layout RGN_IMAGE_PADDED: X is a padded pixel-major image (pixel (y, x) = row
 * (y + 1) (W + 2) + x + 1 of `ld` bf16, channels 0..2; ld a multiple of 4; the border is skipped); RGN_IMAGE_NCHW: X is [1, 3, H, W]
 * (ld ignored).  Per element, as torch on bf16 and numpy on fp32 round:
 *   t = bf16(x * 0.5);  t = bf16(t + 0.5);  t = clamp(t, 0, 1);  dst = (uint8) rint_half_even(float(t) * 255.0f)
 * NaN is out of contract. */
#define RGN_IMAGE_PADDED 0
#define RGN_IMAGE_NCHW 1
int rgn_image_bf16_to_u8(const void* X, int layout, int ld, void* dst, int H, int W, void* stream);

/* Device properties the host side needs for roofline reporting (no torch types). */
int rgn_device_info(int* cu_count, int* clock_khz, size_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* REGIONE_HIP_H */
