/*
 * ldt_hip.h — C-ABI of libldt_hip.so: the MI355X (gfx950) kernels behind LDT's sampling hot path.
 *
 * The upstream reference (Negai-98/LDT) has NO native/FFI seam on this path — everything is torch.nn
 * (SURVEY.md §8b).  The seam a drop-in keeps is the Python class surface (ldt_amd/: Score, Compressor,
 * DiffusionVPSDE, Trainer); this library sits underneath it and each entry point below names the
 * reference code it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + sizes + a hipStream_t passed as void* (0 = default stream);
 *     no torch types, no exceptions, no ownership transfer, no allocation of caller-visible memory.
 *   - every function returns int: 0 ok; <0 argument/shape/alignment error (LDT_E*); >0 a hipError_t.
 *     ldt_last_error() returns a thread-local message for the last non-zero status.
 *   - bf16 buffers are uint16_t* (raw bfloat16 bits); matrices are row-major with explicit leading dims
 *     in ELEMENTS; "token-major": activations are [rows = batch*tokens][channels].
 *   - step-dependent operands (AdaLN tables, sampler coefficients, injected noise) are addressed as
 *     base + (*step_ptr) * step_stride with step_ptr a DEVICE int, so one captured HIP graph of a single
 *     reverse-SDE step can be replayed for every step (NULL step_ptr = step 0 / host step where given).
 */
#ifndef LDT_HIP_H
#define LDT_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LDT_ABI_VERSION 26
#define LDT_OK 0
#define LDT_EARG (-1)    /* null / inconsistent argument */
#define LDT_ESHAPE (-2)  /* unsupported shape */
#define LDT_EALIGN (-3)  /* pointer / leading-dim alignment */
#define LDT_MAX_BLOCKS 64

int ldt_abi_version(void);
const char* ldt_last_error(void);

/* ---- packing ------------------------------------------------------------------------------------
 * fp32 [rows][cols] (ld_src) -> bf16 [rows][cols_pad] (ld_dst), zero padded to cols_pad (multiple of 4).
 * Used to pack Conv1d/Linear weights (out,in,1) once per weight version (after
 * EMA.swap_parameters_with_ema, tools/utils.py:80-101) and to feed fp32 latents to the MFMA GEMM. */
int ldt_cast_pad_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst,
                      int64_t rows, int32_t cols, int32_t cols_pad, void* stream);

/* ---- token-linear layers: bf16 MFMA GEMM with fused epilogue --------------------------------------
 * out[M,N] = epi( X[M,K] · W[N,K]^T + bias[N] ).  Replaces every 1x1 nn.Conv1d / nn.Linear on the path:
 * model/layers.py:159-161 (fc_q, fc_kv, fc_o), :121-124 (MLP fc/out), model/scorenet/score.py:110 (ln_in),
 * model/layers.py:239 (FinalLayer.ln) and the Compressor's twins.  K % 64 == 0 (pad), rows 16-B aligned. */
enum ldt_epilogue {
    LDT_EPI_F32 = 0,        /* out fp32 = acc + bias */
    LDT_EPI_BF16 = 1,       /* out bf16 = acc + bias */
    LDT_EPI_GELU_BF16 = 2,  /* out bf16 = gelu_erf(acc + bias)            (layers.py:127-129) */
    LDT_EPI_RELU_BF16 = 3,  /* out bf16 = relu(acc + bias [+ skip bf16])  (Compressor/layers.py:115-160) */
    LDT_EPI_RESID_F32 = 4   /* out fp32 = resid + gate[s,:] * (acc + bias) (layers.py:218-219; gate NULL = 1) */
};
int ldt_gemm_bf16(int32_t epilogue, const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw,
                  const float* bias, void* out, int64_t ldo,
                  const float* resid, int64_t ldr, const uint16_t* skip, int64_t ldskip,
                  const float* gate, int64_t gate_sample_stride, int32_t rows_per_sample,
                  const int32_t* step_ptr, int64_t gate_step_stride,
                  int32_t M, int32_t N, int32_t K, void* stream);

/* ---- LayerNorm folded into the neighbouring GEMMs (batch-shared AdaLN modulation) ------------------------------
 * The reference's  x = x + gate * fc(...) ; h = LN(x) * (1 + scale) + shift ; y = W h + b  (model/layers.py:218-219 with
 * :136-137 and tools/utils.py:127-133) without a LayerNorm pass over x.  With mu, r = mean and rstd of a row of x:
 *     y = r * (W xs) - r * mu * S + C,   xs = x (1 + scale),  S[n] = sum_k (1 + scale[k]) W[n][k],  C[n] = sum_k shift[k] W[n][k] + b[n].
 * ldt_gemm_resid_lnstats (producer):  out = out + gate * (X W^T + bias) in place (LDT_EPI_RESID_F32), plus
 *     xs[M][N] = bf16(out * (1 + ln_scale[n])) and stats_out[N/256][M][2] = per-row (sum, sum of squares) of out over
 *     each 256-column tile (deterministic: no atomics).
 * ldt_gemm_lnfold (consumer):  out bf16 = epi(r * (Xs W^T) - r * mu * fold_S + fold_C), epilogue LDT_EPI_BF16 or
 *     LDT_EPI_GELU_BF16; the row statistics are those of the K = stats_parts*256 input channels (K <= 1024).
 * ln_scale / fold_S / fold_C / gate are addressed base + (*step_ptr) * their step stride (step_ptr NULL = 0).
 * stats_parts selects the statistics granule and with it the kernel family: N/256 (producer) | K/256 (consumer) partials per row — the
 *     256-tile kernels: M, N multiples of 256, K >= 256, K <= 1024 for the consumer; N/32 | K/32 — the mid-size tile kernels (the fold
 *     route of batches of 1-2 k rows, whose GEMMs stay below the 256-tile kernels' fill rule): M a multiple of 128, N of 64.  A producer and the consumer
 *     of its statistics must use the same granule.  The host builds S and C in fp32 from the SAME bf16 W the GEMM reads. */
int ldt_gemm_resid_lnstats(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias,
                           float* out, int64_t ldo, const float* gate, int64_t gate_sample_stride,
                           int32_t rows_per_sample, const float* ln_scale, uint16_t* xs, int64_t ldxs,
                           float* stats_out, const int32_t* step_ptr, int64_t gate_step_stride,
                           int64_t ln_step_stride, int32_t M, int32_t N, int32_t K, int32_t stats_parts, void* stream);
int ldt_gemm_lnfold(int32_t epilogue, const uint16_t* Xs, int64_t ldx, const uint16_t* W, int64_t ldw,
                    const float* stats_in, const float* fold_S, const float* fold_C, uint16_t* out, int64_t ldo,
                    const int32_t* step_ptr, int64_t fold_step_stride, int32_t M, int32_t N, int32_t K, int32_t stats_parts,
                    void* stream);

/* ---- LayerNorm(eps 1e-6) [+affine] [+AdaLN modulate] -> bf16 -----------------------------------------
 * y = LN(x)[*w+b] * (1 + scale[s]) + shift[s].  tools/utils.py:127-133 + model/layers.py:136-137,218-219.
 * shift/scale: fp32 [samples or 1][...] addressed base + step*mod_step_stride + sample*mod_sample_stride. */
int ldt_layernorm_modulate(const float* x, int64_t ldx, uint16_t* y, int64_t ldy,
                           const float* w, const float* b, const float* shift, const float* scale,
                           int64_t mod_sample_stride, int32_t rows_per_sample,
                           const int32_t* step_ptr, int64_t mod_step_stride,
                           int64_t M, int32_t C, void* stream);

/* ---- fused multi-head attention ---------------------------------------------------------------------
 * O[b,h,n,:] = softmax(Q K^T / sqrt(Dh)) V, heads at channel offset h*Dh of each row; output is the
 * contiguous [B][H][Nq][Dh] buffer the reference reinterprets as (B,N,C) (model/layers.py:190-197, Q1).
 * head_dim 8, 16, 32 or 64.  K and V share kv_batch_stride. */
int ldt_attention_fwd(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride,
                      const uint16_t* K, int64_t ldk, const uint16_t* V, int64_t ldv, int64_t kv_batch_stride,
                      uint16_t* O, int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim, void* stream);
/* Which kernel ldt_attention_fwd runs for a problem of this shape (a query, not a launch; the return value is the route, not a status):
 * 0 = streaming (attn_fwd_kernel<head_dim>), 1 = resident (attn_fwd_resident_kernel<head_dim>), 2 = whole-head
 * (attn_fwd_head_kernel<64, ceil(Nk / 64)>), 3 = narrow heads (attn_fwd_narrow_kernel<head_dim>: every shape with head_dim 8 or 16).  bench.py uses it to name the rocprofv3 symbol of the kernel it timed. */
int ldt_attention_route(int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim);
/* Which kernel ldt_gemm_bf16 (fold = 0), ldt_gemm_resid_lnstats / ldt_gemm_lnfold (fold = 256 or 32: the statistics granule; producer when
 * epilogue == LDT_EPI_RESID_F32, consumer otherwise) runs for a problem of this shape (a query, not a launch; the return value is the route,
 * not a status).  The launchers and this query evaluate the same decision function.  Packed:
 *     (family << 28) | (tiles_per_workgroup << 20) | (BM << 10) | BN
 * family 1 = 256 x 256 persistent kernel, every workgroup one tile; 2 = the same kernel, workgroups loop over up to tiles_per_workgroup
 * tiles; 3 = mid-size tile kernel (128 x 256 / 128 x 192 / 128 x 128 / 64 x 128 / 64 x 64, loader waves); 4 = v1 kernel (128 x 128 /
 * 128 x 64 / 64 x 64, ragged N); 0 = no kernel takes it (the launch would return LDT_ESHAPE / LDT_EALIGN).  The query assumes what
 * ldt_gemm_bf16's common call has: the residual in place (ldr = ldo), no per-sample gate stride or skip operand that breaks 16-byte rows.
 * max_wgs: cap on the workgroups of the launch (0 = all CUs), as ldt_score_plan.gemm_wgs.  tiles_per_workgroup saturates at 255. */
int ldt_gemm_route(int32_t epilogue, int32_t M, int32_t N, int32_t K, int64_t ldo, int32_t fold, int32_t max_wgs);
/* The "q | k | v projection + attention" step of a Score block, launched exactly as ldt_score_forward launches it (the forward calls the same
 * function), so that the fused kernels can be driven alone:
 *     self-attention (kv_cond NULL):  [q | k | v] = bf16(X[B*tokens, K] . W[3*hidden, K]^T + bias),  O = attention(q, k, v)
 *     cross-attention (kv_cond set):  q = bf16(X . W[hidden, K]^T + bias),  K | V = rows of kv_cond (K at column 0, V at column `hidden`, row
 *                                     stride ldkv, sample stride kv_batch_stride, elements; cond_tokens rows per sample)
 *     folded (stats set, self only):  X = the LN-folded producer's xs, [q | k | v] = bf16(r (X W^T) - r mu fold_S + fold_C) as ldt_gemm_lnfold
 *                                     (stats[stats_parts][B*tokens][2], K / 256 or K / 32 parts; fold_S / fold_C at + *step_ptr *
 *                                     fold_step_stride; bias NULL: it is part of fold_C)
 * O is the contiguous [B][heads][tokens][head_dim] buffer of ldt_attention_fwd; the softmax weights are rounded to bf16 before P V.
 * One launch when a fused form takes the shape (ldt_qkv_attention_route != 0): QKV is then not written.  Otherwise ldt_gemm_bf16 /
 * ldt_gemm_lnfold into QKV[B*tokens][3*hidden] (q alone in the cross form) and ldt_attention_fwd.  head_dim 8, 16, 32 or 64 (the fused forms take 64 only: narrow heads run the two kernels); K % 64 == 0. */
int ldt_qkv_attention(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias,
                      const float* stats, int32_t stats_parts, const float* fold_S, const float* fold_C, int64_t fold_step_stride,
                      const uint16_t* kv_cond, int64_t ldkv, int64_t kv_batch_stride, uint16_t* O, uint16_t* QKV,
                      int32_t B, int32_t tokens, int32_t cond_tokens, int32_t hidden, int32_t heads, int32_t K, int32_t max_wgs,
                      const int32_t* step_ptr, void* stream);
/* Which form ldt_qkv_attention (and the forward) runs for this shape (a query, not a launch; the return value is the route, not a status):
 * 0 = two kernels, 1 = 32-token self-attention form (128 x 192 tiles of the mid-size tile kernel), 2 = 256-token self-attention form (256 x 192
 * tiles of the persistent kernel), 3 = 32 x 32-token cross-attention form (64 x 64 tiles).  cond_tokens > 0: cross-attention.  fold: 0 plain,
 * 32 / 256 = folded with statistics per that many columns.  The launchers and this query evaluate the same shape rules (and the same
 * LDT_QKV_ATTN / LDT_QKV_ATTN256 / LDT_Q_XATTN switches); a misaligned operand still sends a launch to the two-kernel path. */
int ldt_qkv_attention_route(int32_t B, int32_t tokens, int32_t cond_tokens, int32_t hidden, int32_t heads, int32_t K, int32_t fold,
                            int32_t max_wgs);
/* Attention + output projection + gated residual in one kernel, for narrow blocks (the Compressor: Dh = 32,
 * C = H*Dh in {64, 128}; model/layers.py:183-200 then :218 / :225):
 *     X[b] += gate[b] * (Wo . O'[b] + bo),   O' = softmax(Q K^T / sqrt(Dh)) V written as [H][Nq][Dh] and re-read as
 * (Nq, C) rows without permuting the heads back (quirk Q1) — so the rows a workgroup produces for head h and query
 * block q0 are rows h*Nq/H + q0/H ... of X.  Needs Nq % H == 0.  X fp32 [B*Nq][ldx] updated in place (X must not alias
 * Q/K/V); Wo bf16 [C][C] dense; gate fp32 per-sample vectors (nullable = 1). */
int ldt_attention_oproj_resid(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk,
                              const uint16_t* V, int64_t ldv, int64_t kv_batch_stride, int32_t B, int32_t H,
                              int32_t Nq, int32_t Nk, int32_t head_dim, const uint16_t* Wo, const float* bo, float* X,
                              int64_t ldx, const float* gate, int64_t gate_sample_stride, void* stream);

/* ---- fp32 linear for the small precision-critical layers ---------------------------------------------
 * C[M,N] = act_out( act_in(A[M,K]) · Bw[N,K]^T + bias ), fp32 FMA accumulate; out fp32 or bf16.
 * TimeEmbedding.mlp (model/layers.py:17), adaLN Linear (:172,:238), K<=64 convs, MiniPointnet, prior heads. */
enum ldt_act { LDT_ACT_NONE = 0, LDT_ACT_SILU = 1, LDT_ACT_RELU = 2, LDT_ACT_GELU = 3 };
int ldt_sgemm(const float* A, int64_t lda, const float* Bw, int64_t ldb, const float* bias,
              void* C, int64_t ldc, int32_t out_bf16, int32_t act_in, int32_t act_out,
              int32_t M, int32_t N, int32_t K, void* stream);
/* Which of its seven kernel forms ldt_sgemm runs for this problem (a query, not a launch; the return value is the route, not a status; no
 * device is touched).  The launcher and this query evaluate the same decision function.  misaligned: bit 0 A, bit 1 Bw, bit 2 C, bit 3 bias
 * is not 16-byte aligned (a NULL bias leaves bit 3 clear).  "Rows of A and Bw load 16 bytes" below means K % 4 == 0, lda % 4 == 0,
 * ldb % 4 == 0 and bits 0 and 1 clear.  The forms in the order they are tried, the first that takes the problem runs:
 *   4 / 5 = linear_smalln_kernel<4> / <8> (N <= 4 / N <= 8): M >= 8192, N <= 8, rows of A and Bw load 16 bytes;
 *   6 / 7 = linear_smallk_kernel<4> / <8> (K <= 4 / K <= 8): M >= 8192, K <= 8, N % 4 == 0 with N / 4 in 8..256 dividing 256 (N = 32, 64,
 *           128, 256, 512, 1024), ldc % 4 == 0, bits 2 and 3 clear;
 *   3 = sgemm_mfma_kernel<32,128,1,4,32>: M <= 48, K >= 8, M * N >= 4096, rows of A and Bw load 16 bytes;
 *   2 = sgemm_mfma_kernel<128,128,2,2>: M > 48, otherwise as 3, and ceil(M / 128) < 65536;
 *   1 = sgemm_nt_kernel: everything else with ceil(M / 64) < 65536 (it stages with 16-byte loads when rows of A and Bw allow, else scalar);
 *   0 = no kernel takes it: M, N or K <= 0, or M beyond the last limit (the launch would return LDT_ESHAPE).
 * Environment, read once per process: LDT_SGEMM_VALU set (to anything) removes the two MFMA forms, LDT_SGEMM_SKINNY=0 the four streaming ones. */
int ldt_sgemm_route(int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t misaligned);

/* sinusoidal embedding of continuous t (model/layers.py:20-36): e[n][2*half] = [sin(t f) | cos(t f)];
 * freq[half] is built by the host with the reference's fp32 expression (quirk Q5). */
int ldt_sinusoid(const float* t, const float* freq, float* e, int32_t n, int32_t half, void* stream);

/* ---- reverse-SDE predictor update (diffusion/diffusion_continuous.py:141-191) ---------------------------
 * mode 0 = ancestral in the reference's op order (coef[step] = {beta, std, sqrt(1-beta), sqrt(beta)});
 * mode 1 = folded x_mean = A x + B params, x = x_mean + C z (coef[step] = {A,B,C,0}).
 * z = noise[step*noise_step_stride + i] if noise != NULL (parity mode: injected CPU draws), else Philox4x32-10
 * keyed by (seed, stream id = step*philox_mul + philox_add, elem_offset + i) — independent of how the batch is
 * sharded across GPUs; predictor-only loops use (1, 0), predictor+corrector loops number every draw.
 * step = *step_ptr if step_ptr else step_host.  x_out may alias x; x_mean_out may be NULL. */
int ldt_sampler_step(const float* x, const float* params, const float* noise, int64_t noise_step_stride,
                     float* x_out, float* x_mean_out, const float* coef,
                     const int32_t* step_ptr, int32_t step_host, int32_t mode,
                     int64_t n, int64_t elem_offset, uint64_t seed,
                     int32_t philox_mul, int32_t philox_add, void* stream);
/* The same step with the sample loop's trajectory store: x after the step is also written to traj[step*n + i] (traj NULL: none). */
int ldt_sampler_step_traj(const float* x, const float* params, const float* noise, int64_t noise_step_stride,
                          float* x_out, float* x_mean_out, float* traj, const float* coef,
                          const int32_t* step_ptr, int32_t step_host, int32_t mode,
                          int64_t n, int64_t elem_offset, uint64_t seed,
                          int32_t philox_mul, int32_t philox_add, void* stream);
int ldt_philox_normal(float* out, int64_t n, int64_t elem_offset, int32_t step, uint64_t seed, void* stream);

/* ---- LangevinCorrector (diffusion/diffusion_continuous.py:193-210) --------------------------------------
 * ldt_batch_norm_sum: *sum_out = sum_b ||x[b,:]||_2 over B samples of per_sample fp32 values each — the numerator of
 *   torch.norm(v.reshape(B,-1), dim=-1).mean() (:204-205); norms_scratch[B] receives the per-sample norms.
 *   Fixed reduction order, no atomics.  When the batch is sharded the caller all-reduces the two sums.
 * ldt_langevin_coef: sums = {sum_b ||params_b||, sum_b ||z_b||} over n_total samples -> coef_out[4] = {1, -step/std,
 *   sqrt(2 step), 0}, step = (snr * noise_norm / grad_norm)^2 * 2 with grad = -params/std (:206, alpha = 1), the row
 *   ldt_sampler_step(mode 1) applies: x_mean = x + step*grad, x = x_mean + sqrt(2 step) z (:207-208). */
int ldt_batch_norm_sum(const float* x, int32_t B, int64_t per_sample, float* norms_scratch, float* sum_out, void* stream);
int ldt_langevin_coef(const float* sums, int32_t n_total, float snr, float std_t, float* coef_out, void* stream);

/* ---- PNDM (diffusion/diffusion_continuous.py:260-316) -----------------------------------------------------
 * ldt_pndm_transfer: out = x + d * (p*x - q*et), the transfer() of :263-274 with the batch-uniform schedule scalars
 *   d = at_next - at, p = 1/(sqrt(at)(sqrt(at)+sqrt(at_next))), q = 1/(sqrt(at)(sqrt((1-at_next)at)+sqrt((1-at)at_next)))
 *   formed by the host in fp32; reference op order, no FMA contraction.  out may alias x.
 * ldt_lincomb4: out = s * (((c0 a0 + c1 a1) + c2 a2) + c3 a3): the Runge-Kutta average of :291 and the 4-step
 *   multistep combination of :300. */
int ldt_pndm_transfer(const float* x, const float* et, float d, float p, float q, float* out, int64_t n, void* stream);
int ldt_lincomb4(const float* a0, const float* a1, const float* a2, const float* a3, float c0, float c1, float c2, float c3,
                 float s, float* out, int64_t n, void* stream);

/* ---- small fp32 element-wise helpers of the host orchestration ---------------------------------------------
 * ldt_vpsde_score: out[b,:] = -params[b,:] / sqrt(var(t[b])), var(t) = 1 - (1 - sigma2_0) exp(-beta0 t - (beta1-beta0) t^2 / 2)
 *   in fp32 — the `score` half of Trainer.score_fn's return value (trainer/Latent_SDE_Trainer.py:57-61 with
 *   DiffusionVPSDE.var, diffusion/diffusion_continuous.py:649-651).
 * ldt_add_f32: out = a + b (c = t_emb + label / image-condition embedding, model/scorenet/score.py:135).
 * ldt_widen_bf16: fp32 copy of a packed bf16 panel (exact). */
int ldt_vpsde_score(const float* params, const float* t, float beta0, float beta1, float sigma2_0, float* out, int32_t B,
                    int64_t per_sample, void* stream);
/* ldt_sde_score: the same for the other SDE families make_diffusion builds (diffusion/diffusion_continuous.py:18-29):
 *   kind 0 vpsde (c0..c2 = beta0, beta1, sigma2_0), 1 sub_vpsde (:705-707; same constants), 2 vesde / geometric_sde
 *   (:746-747 / :615-616; c0..c2 = sigma2_min, sigma2_max / sigma2_min, sigma2_0). */
int ldt_sde_score(const float* params, const float* t, int32_t kind, float c0, float c1, float c2, float* out, int32_t B,
                  int64_t per_sample, void* stream);
int ldt_add_f32(const float* a, const float* b, float* out, int64_t n, void* stream);

/* ---- probability-flow ODE sampling: the device half of RK45 (diffusion/diffusion_continuous.py:88-131) -------
 * `sample_mode: continuous` integrates dx/dt = f(t) x - g2(t)/2 score with scipy's Dormand-Prince 5(4) pair (torchdiffeq's
 * scipy_solver / RK45).  These three streaming kernels are what scipy's rk_step, RK45._step_impl / _estimate_error_norm and
 * select_initial_step (scipy/integrate/_ivp/rk.py, common.py) do between two Score evaluations, on the flattened state as scipy
 * holds it: y and the stage derivatives K[0..6] are float64 [n].  The step controller stays on the host (ldt_amd/ode.py) and reads
 * one double back per step attempt.  fp64 / fp32 arithmetic exactly as written (no FMA contraction), fixed reduction order, no
 * atomics.  n must be a positive multiple of 2 (two fp64 per 16-byte access); fp64 buffers 16-byte, fp32 buffers 8-byte aligned.
 * ldt_ode_stage: y_out = y + h * (((a0 k0 + a1 k1) + a2 k2) + ...), nterms = 1..6 terms left to right (k_s beyond nterms are not
 *   read and may be NULL), and x_out = (float)y_out, the Score's input: stages 1-5 (rows of the tableau A), y_new (the row B) and
 *   the Euler probe of select_initial_step (a0 = 1).  y_out must not alias an input.
 * ldt_ode_rhs: k_out = (double)(-(f x - (0.5 g2) score)), score = -p / sd (is_score = 0: p holds the Score's params, the two
 *   steps of Trainer.score_fn and of fun() in DiffusionBase.sample_model_ode, in fp32 in their operation order) or score = p
 *   (is_score = 1: an opaque score_fn's own score).  f, g2 and sd = sqrt(var(t)) are batch-uniform fp32 scalars the host forms
 *   with the SDE object's f / g2 / var at the evaluation time t = -s (the ODE runs in reversed time s, hence the leading minus).
 * ldt_ode_scaled_sumsq: *out = sum_i ((sum_j c_j v_j[i]) / (atol + rtol max(|ya[i]|, |yb[i]|)))^2 over nvec = 1..7 vectors: the
 *   square of scipy's norm(error / scale) (c_j = E_j over K[0..6], ya = y, yb = y_new; the host applies |h|) and of the three norms of
 *   select_initial_step (y0; f0; f1 - f0 with ya = yb = y0).  Two stages: per-workgroup partials into scratch[scratch_len]
 *   (LDT_ODE_SUMSQ_SCRATCH doubles always suffice; fewer cap the grid), then one workgroup.  Repeats bit for bit. */
#define LDT_ODE_SUMSQ_SCRATCH 1024
int ldt_ode_stage(const double* y, const double* k0, const double* k1, const double* k2, const double* k3, const double* k4,
                  const double* k5, double a0, double a1, double a2, double a3, double a4, double a5, int32_t nterms, double h,
                  double* y_out, float* x_out, int64_t n, void* stream);
int ldt_ode_rhs(const float* x, const float* p, int32_t is_score, float f, float g2, float sd, double* k_out, int64_t n, void* stream);
int ldt_ode_scaled_sumsq(const double* v0, const double* v1, const double* v2, const double* v3, const double* v4, const double* v5,
                         const double* v6, double c0, double c1, double c2, double c3, double c4, double c5, double c6, int32_t nvec,
                         const double* ya, const double* yb, double atol, double rtol, double* scratch, int32_t scratch_len,
                         double* out, int64_t n, void* stream);
/* ldt_block_activation: x = act(x) in place on bf16 rows [M][C] (row stride ld, elements) — the block activation of the reference's
 *   no-condition ResidualBlock branches (`decoder_act`: model/layers.py:224-226, `self.act` from tools/utils.py:104-124), applied to the
 *   LayerNorm output that fc_q / the MLP read.  rrelu in its eval-mode form. */
enum ldt_block_act { LDT_BACT_NONE = 0, LDT_BACT_GELU = 1, LDT_BACT_SILU = 2, LDT_BACT_RELU = 3, LDT_BACT_LEAKY_001 = 4, LDT_BACT_LEAKY_02 = 5,
                     LDT_BACT_RRELU_EVAL = 6, LDT_BACT_HARDSWISH = 7, LDT_BACT_SELU = 8 };
int ldt_block_activation(uint16_t* x, int64_t ld, int64_t M, int32_t C, int32_t kind, void* stream);
int ldt_widen_bf16(const uint16_t* src, float* dst, int64_t n, void* stream);

/* ---- the other norms `get_norm` builds (tools/utils.py:168-181; ResidualBlock.norm1 / norm2, FinalLayer.norm: model/layers.py:163-164,235) ----
 * `norm: group_norm` = nn.GroupNorm(min(C / 4, 16), C, eps = 1e-6) applied to the channels-first (B, C, N) activations: statistics per sample and
 * group over (C / G channels) x (N tokens), ALWAYS affine (the elementwise_affine flag is ignored upstream).  `norm: ~` = Identity.
 * (`norm: batch_norm` is undefined upstream: its wrapper feeds (B, N, C) to BatchNorm1d(C) and fails unless tokens == channels.)
 * ldt_group_stats: stats[b][g] = (mean, rstd) of sample b's `T` token rows x[b*T .. (b+1)*T)[g*C/G .. (g+1)*C/G), biased variance.
 * ldt_norm_apply:  y[m][c] = bf16( ((x[m][c] - mean) * rstd * w[c] + b[c]) * (1 + scale[s][c]) + shift[s][c] ), (mean, rstd) =
 *   stats[m / rows_per_stat][c / (C/G)] (stats NULL: 0, 1), w / b NULL: 1 / 0, s = m / rows_per_sample, shift / scale NULL: 0 (layers.py:136-137). */
int ldt_group_stats(const float* x, int64_t ldx, int32_t B, int32_t T, int32_t C, int32_t G, float eps, float* stats, void* stream);
int ldt_norm_apply(const float* x, int64_t ldx, uint16_t* y, int64_t ldy, int64_t M, int32_t C, const float* stats, int32_t G,
                   int32_t rows_per_stat, const float* w, const float* b, const float* shift, const float* scale,
                   int64_t mod_sample_stride, int32_t rows_per_sample, void* stream);

/* LN-folding monitor: *out = max over the M rows of mean^2 / variance, from the row statistics stats[parts][M][2] a
 * ldt_gemm_resid_lnstats launch wrote (K = parts * 256 channels).  The folded projections' rounding error grows as
 * (1 + mean^2 / variance); the sampler falls back to the LayerNorm kernels when this exceeds its bound. */
int ldt_fold_mean_ratio(const float* stats, int32_t parts, int64_t M, int32_t K, float* out, void* stream);

/* ---- Compressor encoder front end (model/Compressor/layers.py:65-112, 288-319; Network.py:26-29,76,86-107) ----
 * Clouds are fp32 [B][n][3]; index outputs are int32.
 * ldt_fps: farthest point sampling, m centres per cloud, semantics of the vendored CUDA twin
 *   model/functional/src/sampling/sampling.cu:86-167 (start index 0, ties to the smaller (k%512, k/512)).
 *   The reference calls pointnet2_ops.furthest_point_sample (Compressor/layers.py:106; third party, not vendored).
 * ldt_knn: k nearest points of each of the S centres by square_distance (layers.py:65-84) + topk(largest=False,
 *   sorted=False) (:97): an UNORDERED index set [B][S][k]; dist_out (nullable) receives the [B][S][n] distances.
 * ldt_group_normalize: LocalGrouper normalisation (:297-315): per-sample unbiased std of (g - origin)
 *   (stats: fp64 scratch [2*B]), rows U[b,s,j,:] = [alpha*(g-origin)/(std+1e-5)+beta | centre feature], bf16, K padded to ldu.
 *   center_mode 0 = 'anchor' (origin = the centre point's [feature|xyz], :309-311; the Compressor, cluster_norm),
 *   1 = 'center' (origin = mean over the group's k rows, :307-308; ConditionNet, model/scorenet/score.py:22) with
 *   group_mean an fp32 workspace [B][S][D+3] (may be NULL in mode 0).
 * ldt_gather_rows: index_points (:46-62), out[b,s,:] = src[b, idx[b,s], :].
 * ldt_maxpool: max over the middle axis of [G][n][C] (bf16 or fp32 input) -> fp32 [G][C] (:186, Network.py:97).
 * ldt_actnorm: in place (x - shift[t,c]) * exp(-log_scale[t,c]) (model/layers.py:103-107, eval).
 * ldt_reparam: mu|logvar split, clamp(logvar, lo, hi), eps = mu + exp(logvar/2)*noise into a strided slice
 *   (Network.py:26-29,75-77); mu_out/logvar_out nullable.
 * ldt_chamfer: distChamfer (evaluation/evaluation_metrics.py:23-33): dl[b][nb] = min over a, dr[b][na] = min over b. */
int ldt_fps(const float* xyz, int32_t B, int32_t n, int32_t m, int32_t skip_near_origin, int32_t* idx_out, void* stream);
/* ldt_norm_points: Compressor.norm_pts (Network.py:170-174; cfg.compressor.norm_input): per cloud and coordinate (p - mean) / std,
 *   unbiased std over the n points; out may alias xyz.
 * ldt_mixture_seed: InitialSet with max_outputs None (Compressor/layers.py:17-24,38-41): out[r][d] = sum_m (eps[r][m][d] sig[m][d] +
 *   mu[m][d]) softmax(logits)[m] over rows r = b*N + n; the `output` MLP that follows is two ldt_sgemm calls. */
int ldt_norm_points(const float* xyz, int32_t B, int32_t n, float* out, void* stream);
int ldt_mixture_seed(const float* eps, const float* sig, const float* mu, const float* logits, int32_t n_mix, int32_t D, int64_t rows,
                     float* out, void* stream);
int ldt_knn(const float* xyz, const float* centers, int32_t B, int32_t n, int32_t S, int32_t k,
            int32_t* idx_out, float* dist_out, void* stream);
int ldt_group_normalize(const float* feat, const float* xyz, const int32_t* fps_idx, const int32_t* knn_idx,
                        const float* alpha, const float* beta, double* stats, int32_t B, int32_t n, int32_t S,
                        int32_t k, int32_t D, uint16_t* U, int32_t ldu, int32_t center_mode, float* group_mean,
                        void* stream);
int ldt_gather_rows(const float* src, const int32_t* idx, int32_t B, int32_t n, int32_t S, int32_t C, float* out, void* stream);
/* Grouping + PreExtraction + neighbour max in ONE kernel (Compressor/layers.py:288-319 LocalGrouper.forward with
 * normalize='anchor', :115-160 PreExtraction, :186 max over the k neighbours): out fp32 [B*S][128] = max_j relu(W3 . relu(W2 . h1 + b2)
 * + b3 + h1), h1 = relu(W1 . u_j + b1), u_j = the grouped row [alpha*((g_j - anchor)/(std+1e-5)) + beta | anchor features] that
 * ldt_group_normalize would write (never materialised here).  D must be 128, k one of 8, 16 or a multiple of 32.  stats: workspace double[2B].
 * wimg: the three eval-BatchNorm-folded weight panels as bf16 MFMA fragments, 132 x 1 KB:
 *   fragment f, lane l = 32 h + i, slot e (0..7)  ->  W[32 blk + i][col(step, h, e)]
 *   layer 1  f = 4 step + blk, step 0..16: col = 16 step + 8 h + e (steps 0..7: normalised features), 131 + 16 (step - 8) + 8 h + e
 *            (steps 8..15: anchor features), step 16: 128 + e for h = 0, e < 3 (xyz), zero weight elsewhere;
 *   layer 2  f = 68 + 4 step + blk,  layer 3  f = 100 + 4 step + blk, step 0..7: col = 16 step + 8 (e >> 2) + 4 h + (e & 3). */
int ldt_grouper_mlp(const float* feat, const float* xyz, const int32_t* fps_idx, const int32_t* knn_idx, const float* alpha,
                    const float* beta, double* stats, int32_t B, int32_t n, int32_t S, int32_t k, int32_t D,
                    const uint16_t* wimg, const float* b1, const float* b2, const float* b3, float* out, void* stream);
int ldt_maxpool(const void* in, int32_t in_bf16, int64_t ld, int64_t G, int32_t n, int32_t C, float* out, void* stream);
int ldt_actnorm(float* x, const float* shift, const float* log_scale, int64_t B, int64_t per_sample, void* stream);
int ldt_reparam(const float* post, const float* noise, float* out, int64_t ldo, float* mu_out, float* logvar_out,
                int64_t rows, int32_t z, float lo, float hi, void* stream);
int ldt_chamfer(const float* a, const float* b, int32_t B, int32_t na, int32_t nb, float* dl, float* dr, void* stream);

/* ---- held-out evaluation: the loss arithmetic between the encode, the Score forward and the metrics (eval_loss.hip) ----
 * Single-pass fp32 kernels, fixed summation order (no atomics): two calls on the same input return the same bits.
 * ldt_reparam_kl: ldt_reparam (out / mu_out / logvar_out are bit-identical to it) plus, per element and in the reference's fp32 operation
 *   order (model/Compressor/Network.py:12-19 log_p_var_normal / log_p_normal, :221-224 top_down):
 *       logqz = -0.5 (eps - mu)^2 / exp(logvar) - 0.5 logvar - 0.9189385332,  logpz = -0.5 eps^2 - 0.9189385332,  kl = logqz - logpz
 *   written token-major [rows][z] to logqz_out / kl_out, and kl_sample_sum[b] = the sum of kl over sample b's rows_per_sample x z elements
 *   (rows = samples x rows_per_sample).  Every output but `out` may be NULL (mu_out / logvar_out together).  16-byte accesses when z and ldo
 *   are multiples of 4 and the buffers 16-byte aligned; any other shape takes the scalar form of the same kernel.
 * ldt_diffuse_q: DiffusionBase.sample_q with per-sample scalars (diffusion/diffusion_continuous.py:78-81; trainer/Latent_SDE_Trainer.py:79-81
 *   `xt = eps * e2int_f + torch.sqrt(var) * eta`): xt[b][i] = x0[b][i] * m[b] + sqrtf(var[b]) * eta[b][i], each product and the sum rounded
 *   separately and the root correctly rounded (bit-equal to the fp32 expression evaluated with IEEE operations).  eta_in given: that noise (also copied to eta_out when eta_out is given).  eta_in NULL:
 *   eta is drawn from the Philox stream exactly as ldt_philox_normal(eta_out, B * per_sample, 0, step, seed) would fill it, and written to
 *   eta_out (required then).  m, var: DEVICE fp32 [B].  per_sample % 4 == 0, buffers 16-byte aligned.
 * ldt_dsm_loss: the denoising score-matching loss (trainer/Latent_SDE_Trainer.py:83-87): distance = |eta - params| (l1 != 0) or
 *   (eta - params)^2, times weight[b] (DEVICE fp32 [B]; NULL = 1); sample_loss[b] (required: it is the first stage's output) = the mean
 *   over sample b, *mean_loss (nullable) = the mean over everything.  The results stay on the device: no host synchronisation. */
int ldt_reparam_kl(const float* post, const float* noise, float* out, int64_t ldo, float* mu_out, float* logvar_out,
                   float* kl_out, float* logqz_out, float* kl_sample_sum, int64_t rows, int64_t rows_per_sample, int32_t z,
                   float lo, float hi, void* stream);
int ldt_diffuse_q(const float* x0, const float* eta_in, const float* m, const float* var, float* xt, float* eta_out,
                  int64_t B, int64_t per_sample, uint64_t seed, int32_t step, void* stream);
int ldt_dsm_loss(const float* eta, const float* params, const float* weight, int64_t B, int64_t per_sample, int32_t l1,
                 float* sample_loss, float* mean_loss, void* stream);

/* ---- hybrid-trainer evaluation: the latent NELBO's sums and the JSD metric's occupancy histograms (nelbo_terms.hip, occupancy_grid.hip) ----
 * Like the block above: status codes before any launch, fixed-order or integer reductions, no floating-point atomics, bit-reproducible.
 * ldt_nelbo_terms: the two sums of the KL term of trainer/Hybrid_Trainer.py:139-143 in one pass over eta, params, logqz (DEVICE fp32
 *   [B][per_sample]) and weight (DEVICE fp32 [B]; NULL = 1): sample_sums[b] = {sum_i (eta - params)^2 * weight[b], sum_i logqz} (fp32 [B][2],
 *   required: the first stage's output), batch_sums (nullable) = the two sums over the batch (fp32 [2]).  Each term is formed in fp32 with
 *   the reference's three roundings, the partial sums are carried in float64 and rounded once.  16-byte accesses when per_sample % 4 == 0
 *   and the buffers are 16-byte aligned, the scalar form otherwise.  kl = (batch_sums[0] + batch_sums[1]) / (B per_sample) + c.
 * ldt_occupancy_grid: evaluation/evaluation_metrics.py:376-389.  pts fp32 [S][n][3], cells fp32 [G][3], G <= 32768.  For every point the
 *   nearest cell under the float64 squared distance (dx^2 + dy^2) + dz^2 of the fp32 coordinates (products and sums rounded, no FMA: what
 *   sklearn's tree evaluates), the lowest index winning a tie: counters[g] += 1 per point, bernoulli[g] += 1 once per cloud with a point in
 *   g.  Both uint32 [G] are ADDED to (zero them for one set's histogram).  Integer adds: exact, the same bits every run. */
int ldt_nelbo_terms(const float* eta, const float* params, const float* logqz, const float* weight, int64_t B, int64_t per_sample,
                    float* sample_sums, float* batch_sums, void* stream);
int ldt_occupancy_grid(const float* pts, int32_t S, int32_t n, const float* cells, int32_t G, uint32_t* counters, uint32_t* bernoulli,
                       void* stream);

/* ---- Score training: the backward pieces and the optimizer (score_bwd.hip, attention_bwd.hip, optim.hip) ----
 * What trainer/Latent_SDE_Trainer.py:137-140 (`loss.backward()`, clip_grad_norm_, EMA(Adam).step()) needs under the forward kernels above,
 * for the AdaLN LayerNorm Score blocks the shipped YAMLs train.  The backward GEMMs are NOT here: dgrad dX = dY . W and wgrad dW = dY^T . X
 * are ldt_gemm_bf16 (LDT_EPI_F32 / LDT_EPI_BF16) on operands ldt_transpose_cast_bf16 prepares.  Like the evaluation kernels: status codes
 * before any launch, every reduction in a fixed order, no floating-point atomics — a step repeats bit for bit.
 * ldt_transpose_cast_bf16: src fp32 (src_bf16 = 0) or bf16 [R][C] (row stride ld_src) -> dst bf16 [C][R_pad] (row stride ld_dst), columns R ..
 *   R_pad - 1 zero: W^T panels for dgrad, dY^T and X^T (the contraction over the R rows, padded to the GEMM's K % 64) for wgrad.
 * ldt_colsum: out[c] = sum_m dy[m][c] over M rows of an fp32 or bf16 matrix — the bias gradient of every 1x1 conv / Linear (model/layers.py:
 *   121-124,159-161,239; score.py:110).  float64 partials, one rounding.
 * ldt_layernorm_modulate_bwd: backward of ldt_layernorm_modulate without affine (tools/utils.py:127-133 + model/layers.py:136-137,218-219,
 *   243-245): from the saved fp32 x and the fp32 gradient dy of y = LN(x) (1 + scale[s]) + shift[s]:  dx[m][:] += the LayerNorm gradient (ADDED:
 *   dx is the residual-stream gradient), dshift[s][:] = sum over sample s's rows of dy, dscale[s][:] = sum of dy * LN(x) (written, fp32
 *   [samples][dmod_sample_stride]; both NULL = skipped).  scale: fp32 [samples][mod_sample_stride] (stride 0 = shared; NULL = 0).  stats: fp32
 *   workspace [M][2], receives each row's (mean, rstd).  M % rows_per_sample == 0.
 * ldt_gelu_bwd: du bf16 = dh * d/du GELU_erf(u) on the saved bf16 pre-activation u of mlp.fc (model/layers.py:111-113,127-129); dh fp32 or bf16.
 * ldt_gate_residual_bwd: y = x + gate[s] * a (model/layers.py:218-219): da bf16 = dy * gate[s], dgate[s][:] = sum over sample s's rows of
 *   dy * a (a: the branch output fc_o(...) / mlp(...), fp32 or bf16; dgate NULL = skipped and a unused).  dx = dy needs no kernel.
 * ldt_silu_bwd: dc = dy * d/dc SiLU(c), fp32 (adaLN_modulation.0, model/layers.py:171,237; TimeEmbedding.mlp, :17); act (nullable) receives
 *   SiLU(c), the operand of the following Linear's weight gradient (the forward applies it inside ldt_sgemm and never stores it).  dc NULL: act only.
 * ldt_dsm_loss_bwd: gradient of ldt_dsm_loss's *mean_loss with respect to params (trainer/Latent_SDE_Trainer.py:131-137):
 *   -2 (eta - params) weight[b] / (B per_sample), or -sign(eta - params) weight[b] / (B per_sample) when l1.
 * ldt_embedding_grad: dE[k][:] = sum over the samples with label[b] == k of dc[b][:], in the order of b (the label nn.Embedding,
 *   model/scorenet/score.py:125-128); every row of dE[n_classes][D] is written.
 * ldt_actnorm_bwd: backward of ldt_actnorm (model/layers.py:103-107 `(x - shift) * exp(-log_scale)`, the parameters :66-72; the Compressor's
 *   conv_in, Network.py:200-201) from the fp32 gradient dz and the forward's OUTPUT z [B][per_sample] (the forward runs in place: z is what is
 *   kept): dx[b][i] = dz[b][i] exp(-log_scale[i]) (dx may alias dz), dshift[i] = -sum_b dx[b][i], dlog_scale[i] = -sum_b dz[b][i] z[b][i];
 *   dshift / dlog_scale fp32 [per_sample], each nullable (both NULL: dx only; z is read for dlog_scale alone).  Both forms of the reference's
 *   ActNorm: per token and channel (per_sample = T C, B samples) and 'set' (per_sample = C, B T rows).  The sums run over b in ascending order
 *   inside contiguous runs of rows, the runs and — past 512 rows — the workgroups' partials (stream-ordered scratch of the call's own) are added
 *   in index order: float64 throughout, one rounding, no atomics.  16-byte accesses when per_sample % 4 == 0 and dz, z, log_scale, dx are
 *   16-byte aligned, the scalar form of the same kernel otherwise.  LDT_EARG for a null pointer, B < 1 or per_sample < 1.
 * ldt_attention_bwd: backward of ldt_attention_fwd for self-attention with head_dim 64, Nq = Nk = N <= 512 (model/layers.py:190-197).  Q, K, V as
 *   ldt_attention_fwd takes them; O and dO are the contiguous [B][H][N][64] buffer that IS the raw (B N, C) view (quirk Q1: nothing is
 *   permuted); dQ, dK, dV are written as row views like Q, K, V (heads at column h * 64; dK and dV share dkv_batch_stride).  Row maximum and
 *   sum are recomputed (the forward writes no log-sum-exp) into stats fp32 [B][H][N][2] = (max + ln sum, rowsum(dO o O)).  bf16 MFMA, fp32
 *   accumulation; P and dS are rounded to bf16 before the second products.  dQ per query block, dK / dV per key block: no sum across workgroups.
 * ldt_attention_bwd_narrow: the same contract for head_dim 8, 16 or 32 (scale head_dim^-0.5; ldt_attention_bwd keeps taking 64 alone).  32 runs
 *   the kernels of ldt_attention_bwd instantiated at 32.  8 and 16 (the narrow form of attention_bwd.hip): one wave per 16 rows, MFMA first products with
 *   the channel extent zero-padded, second products as per-lane fp32 FMAs: P and dS stay fp32; row statistics and dQ in one launch, dK / dV in
 *   a second.  dQ, dK, dV rows must be 8-byte aligned (row and batch strides % 4 == 0).
 * ldt_attention_bwd_cross: the contract of ldt_attention_bwd with two lengths, for the cross-attention of a conditioned Score's even blocks
 *   (model/layers.py:183-200 with y = the point condition; model/scorenet/score.py:129-149): Nq query rows (1 .. 512) and Nk key / value rows
 *   (1 .. 512, any relation to Nq) per sample, head_dim 8, 16, 32 or 64, scale head_dim^-0.5.  Q: B Nq rows; K, V: B Nk rows sharing
 *   kv_batch_stride; O and dO the contiguous raw [B][H][Nq][head_dim] buffer (quirk Q1); stats fp32 [B][H][Nq][2]; dQ written as rows like Q,
 *   dK and dV as rows like K and V.  The kernels of the two entry points above with separate row and loop extents: statistics and dQ per
 *   block of 16 queries looping over the Nk keys, dK / dV per block of 16 keys looping over the Nq queries; every sum inside one wave in a
 *   fixed order, no atomics, no sum across workgroups.  At Nq = Nk the same bits as ldt_attention_bwd / ldt_attention_bwd_narrow.  At
 *   head_dim 8 and 16 the alignment rule of ldt_attention_bwd_narrow on dQ, dK, dV applies.
 * ldt_sumsq: out[0] = sum x^2 (two stages, float64 partials in scratch[scratch_len], at most LDT_ODE_SUMSQ_SCRATCH used), out[1] = its root
 *   (clip_grad_norm_'s total_norm over the flat gradient), out[2] = min(1, max_norm / (out[1] + 1e-6)) (clip_coef_clamped; 1 when max_norm <= 0).
 * ldt_adam_ema_step: torch.optim.Adam's update (torch/optim/adam.py _single_tensor_adam: L2 weight_decay added to the gradient, exp_avg.lerp_,
 *   exp_avg_sq.mul_.addcmul_, denom = sqrt(v) / sqrt(1 - beta2^step) + eps, param.addcdiv_ with -lr / (1 - beta1^step)): the same formulas in
 *   the same order, each in its fewest-roundings form (not torch's kernel sequence: not bit-equal to an fp32 torch run), over flat fp32 buffers of n elements, then the reference's EMA (tools/utils.py:34-71): ema_init != 0 (a parameter's first step):
 *   ema = param after the update; then always ema = ema * ema_decay + (1 - ema_decay) * param, evaluated as ema + (1 - ema_decay) (param - ema)
 *   (and v likewise as v + (1 - beta2) (g g - v)): against an exact evaluation every stored value is within its own fp32 rounding plus a few roundings of
 *   its step's change.  ema NULL: no EMA.  clip_factor: DEVICE float
 *   (ldt_sumsq's out + 2) the gradient is first multiplied by, in place as clip_grad_norm_ does; NULL = 1, grad untouched.  step counts from 1. */
int ldt_transpose_cast_bf16(const void* src, int32_t src_bf16, int64_t ld_src, uint16_t* dst, int64_t ld_dst, int64_t R, int32_t C,
                            int64_t R_pad, void* stream);
int ldt_colsum(const void* dy, int32_t dy_bf16, int64_t ld, int64_t M, int32_t C, float* out, void* stream);
int ldt_layernorm_modulate_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* scale, int64_t mod_sample_stride,
                               int32_t rows_per_sample, float* dx, int64_t lddx, float* dshift, float* dscale,
                               int64_t dmod_sample_stride, float* stats, int64_t M, int32_t C, void* stream);
int ldt_gelu_bwd(const uint16_t* u, int64_t ldu, const void* dh, int32_t dh_bf16, int64_t lddh, uint16_t* du, int64_t lddu, int64_t M,
                 int32_t C, void* stream);
int ldt_gate_residual_bwd(const float* dy, int64_t lddy, const void* a, int32_t a_bf16, int64_t lda, const float* gate,
                          int64_t gate_sample_stride, int32_t rows_per_sample, uint16_t* da, int64_t ldda, float* dgate,
                          int64_t dgate_sample_stride, int64_t M, int32_t C, void* stream);
int ldt_silu_bwd(const float* c, const float* dy, float* dc, float* act, int64_t n, void* stream);
int ldt_dsm_loss_bwd(const float* eta, const float* params, const float* weight, int64_t B, int64_t per_sample, int32_t l1, float* dparams,
                     void* stream);
int ldt_embedding_grad(const float* dc, int64_t ld, const int32_t* label, int32_t B, int32_t D, int32_t n_classes, float* dE, void* stream);
int ldt_actnorm_bwd(const float* dz, const float* z, const float* log_scale, int64_t B, int64_t per_sample, float* dx, float* dshift,
                    float* dlog_scale, void* stream);
int ldt_attention_bwd(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                      int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                      int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                      int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t N, int32_t head_dim, void* stream);
int ldt_attention_bwd_narrow(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                             int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                             int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                             int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t N, int32_t head_dim, void* stream);
int ldt_attention_bwd_cross(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                            int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                            int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                            int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim, void* stream);
int ldt_sumsq(const float* x, int64_t n, double* scratch, int32_t scratch_len, float max_norm, float* out, void* stream);
int ldt_adam_ema_step(float* param, float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, double lr, double beta1,
                      double beta2, double eps, double weight_decay, int32_t step, double ema_decay, int32_t ema_init,
                      const float* clip_factor, void* stream);

/* ---- training the Compressor's decoder: reconstruction loss, attention backward on a long query axis, prior rows ----
 * ldt_chamfer_nn: nearest neighbours both ways between x1 fp32 [B][n][3] (the estimated cloud) and x2 fp32 [B][m][3]: d1 [B][n] =
 *   min_j |x1_i - x2_j|^2 with idx1 [B][n] the LOWEST j that attains it, d2 [B][m] / idx2 [B][m] likewise from x2 to x1 (chamfer3D.cu's forward).
 *   Each distance is formed by the expression of ldt_chamfer: d1 and d2 equal its dr and dl bit for bit.
 * ldt_cd_loss: CD_loss (evaluation/loss.py:71-78) of n1 + n2 such distances on the device: out[3] = (loss, term1, term2),
 *   LDT_CD_L1: mean sqrt(max(d1, 0)) + mean sqrt(max(d2, 0)); LDT_CD_L2: mean d1 + mean d2.  Float64 partials in index order, one workgroup.
 * ldt_cd_loss_bwd: upstream * d loss / d x1 -> dx1 fp32 [B][n][3] (chamfer3D.cu's backward through CD_loss, for the estimated cloud: the only
 *   gradient the reference's reconstruction losses feed):  dx1[i] = 2 g1[i] (x1_i - x2_idx1[i]) + sum_{j : idx2[j] = i} 2 g2[j] (x1_i - x2_j),
 *   g = upstream / (B n) or / (B m), times 1 / (2 |x1_i - x2_j|) under LDT_CD_L1.  The second term is gathered (point i scans idx2 of its cloud
 *   with j ascending): no atomics, the same bits on every run.  Deviations from the reference: a pair at distance exactly 0 contributes
 *   exactly 0 (its direction is zero; the reference's inf * 0 is NaN), and the l1 weight takes the distance from the difference vector
 *   itself, to a few fp32 roundings, not from d1 / d2, whose expanded form is only absolutely accurate.  An index outside its cloud is skipped.
 * ldt_attention_bwd_long: the contract of ldt_attention_bwd_cross for a long query axis: head_dim 32 only, 1 <= Nq <=
 *   LDT_ATTN_BWD_LONG_MAX_QUERIES, 1 <= Nk <= 512 (the Compressor's decoder: Nq = 2048 set points on Nk = 32 latent tokens,
 *   Compressor/layers.py:225 through model/layers.py:183-200).  Row statistics and dQ are ldt_attention_bwd_cross's kernels (the same bits
 *   where both admit the shape).  dK / dV: one wave per (16 keys, LDT_ATTN_BWD_LONG_CHUNK queries) writes fp32 partials into scratch
 *   [ceil(Nq / chunk)][B][Nk][2 H 32] (scratch_len floats, at least that many), and a second kernel adds them in chunk order, scales dK and
 *   rounds to bf16: a fixed order set by the constant alone.
 * ldt_rows_gather_sum: dprior fp32 [R][C] (dense) = sum over b, in the order of b, of dy[b N + src[b][r]][:] (dy fp32 [B N][ld]) where
 *   src int32 [B][R] >= 0; -1 (or any index outside [0, N)) = sample b does not hold prior row r.  Backward of InitialSet's learned
 *   prior (Compressor/layers.py:26-42); every row of dprior is written. */
#define LDT_CD_L1 1
#define LDT_CD_L2 2
#define LDT_ATTN_BWD_LONG_MAX_QUERIES 8192
#define LDT_ATTN_BWD_LONG_CHUNK 256
int ldt_chamfer_nn(const float* x1, const float* x2, int32_t B, int32_t n, int32_t m, float* d1, int32_t* idx1, float* d2, int32_t* idx2,
                   void* stream);
int ldt_cd_loss(const float* d1, int64_t n1, const float* d2, int64_t n2, int32_t type, float* out, void* stream);
int ldt_cd_loss_bwd(const float* x1, const float* x2, const int32_t* idx1, const int32_t* idx2, int32_t B, int32_t n, int32_t m, int32_t type,
                    float upstream, float* dx1, void* stream);
int ldt_attention_bwd_long(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                           int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                           int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                           int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim, float* scratch,
                           int64_t scratch_len, void* stream);
int ldt_rows_gather_sum(const float* dy, int64_t ld, const int32_t* src, int32_t B, int32_t N, int32_t R, int32_t C, float* dprior,
                        void* stream);

/* ---- training the Compressor's top-down half: attention backward on a long key axis, backward of the posterior draw and the KL term ----
 * ldt_attention_bwd_wide: the contract of ldt_attention_bwd_cross for a long KEY axis: head_dim 32 only, 1 <= Nq <= 512, 1 <= Nk <=
 *   LDT_ATTN_BWD_WIDE_MAX_KEYS (the Compressor's posterior blocks, compute_posterior, Compressor/Network.py:61-78 through model/layers.py:
 *   183-200: Nq = 32 latent tokens on the Nk = 2048 points of the running set).  dK / dV are ldt_attention_bwd_cross's key-block kernel.  Row
 *   statistics and dQ run per (16 queries, LDT_ATTN_BWD_WIDE_CHUNK keys).  scratch (scratch_len floats; LDT_EARG when fewer than the two
 *   regions need), with chunks = ceil(Nk / chunk):
 *       [chunks][B][H][Nq][2]     each chunk's row maximum m_c and s_c = sum exp(s - m_c); a second kernel combines them in chunk order,
 *                                 M = max_c m_c, L = M + ln sum_c s_c exp(m_c - M), and writes (L, D) to stats
 *       [chunks][B][Nq][H 32]     unscaled fp32 partials of dQ, which a last kernel adds in chunk order, scales and rounds to bf16
 *   A fixed order set by the constant alone: the same bits on every run.  At Nk <= LDT_ATTN_BWD_WIDE_CHUNK (one chunk) stats, dQ, dK and dV
 *   carry the bits of ldt_attention_bwd_cross.
 * ldt_reparam_kl_bwd: backward of ldt_reparam_kl's draw and of kl_scale x (the sum of its kl) (Compressor/Network.py:12-29, 76, 219-224), from
 *   post fp32 [rows][2 z] = mu | logvar as stored (before the clamp), noise fp32 [rows][z] and d_eps fp32 [rows][ldd] (a column slice of a
 *   wider buffer), into dpost fp32 [rows][2 z] = dmu | dlogvar.  Per element, lv = clamp(logvar, lo, hi), s = exp(lv / 2), eps = mu + s n as
 *   ldt_reparam forms it:  g = d_eps + kl_scale eps,  dmu = g,  dlv = g (s n / 2) - kl_scale / 2,  dlogvar = dlv where lo <= logvar <= hi
 *   (torch.clamp's rule: the bounds included) and exactly 0 elsewhere.  The analytic form: log q's derivatives through mu and logvar cancel
 *   against the one through eps, log p's is eps.  16-byte accesses when z and ldd are multiples of 4 and the buffers 16-byte aligned, the
 *   scalar form of the same kernel otherwise. */
#define LDT_ATTN_BWD_WIDE_MAX_KEYS 8192
#define LDT_ATTN_BWD_WIDE_CHUNK 256
int ldt_attention_bwd_wide(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                           int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                           int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                           int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim, float* scratch,
                           int64_t scratch_len, void* stream);
int ldt_reparam_kl_bwd(const float* post, const float* noise, const float* d_eps, int64_t ldd, float kl_scale, float* dpost, int64_t rows,
                       int32_t z, float lo, float hi, void* stream);

/* ---- training the Compressor's front: training-mode BatchNorm + ReLU, the max over neighbours and the 'anchor' grouping, backward ----
 * (batchnorm.hip, grouper_bwd.hip; model/Compressor/layers.py:115-160 PreExtraction, :186 the neighbour max, :288-319 LocalGrouper.forward;
 * Network.py:86-101 MiniPointnet.)  The training kernels' contract: status codes before any launch, every sum in a fixed order with float64
 * partials and one rounding, no floating-point atomics, a second call gives the same bits.
 * ldt_bn_stats: stats fp32 [2][C] = (mean[c], rstd[c] = 1 / sqrt(biased variance + eps)) over the M >= 2 rows of x fp32 [M][ldx] (torch
 *   refuses one value per channel in training).  Two passes: the mean in float64, then the float64 mean of (x - mean)^2, so a column of equal
 *   values has rstd = 1 / sqrt(eps).  running_mean / running_var (each nullable) are updated in place as nn.BatchNorm1d does in training:
 *   r = (1 - momentum) r + momentum (mean | variance M / (M - 1)), from the float64 statistics with one rounding.
 * ldt_bn_relu_fwd: y[m][c] = ReLU(gamma[c] xhat + beta[c]), xhat = (x[m][c] - mean[c]) * rstd[c] in fp32, to bf16 (out_bf16) or fp32
 *   [M][ldy]; the columns C <= c < cols_pad of y are written 0 (the K padding of a bf16 GEMM operand; cols_pad = C: none).
 * ldt_bn_relu_bwd: from dy fp32, the SAVED x, the statistics, gamma and beta: dyh = dy where gamma xhat + beta > 0, else 0 (xhat and the mask
 *   are recomputed with the forward's own operations, never stored); dgamma[c] = sum_m dyh xhat, dbeta[c] = sum_m dyh (each nullable);
 *   dx[m][c] = gamma rstd ((dyh - dbeta / M) - xhat dgamma / M), fp32 [M][lddx]; dx may alias dy.  Two passes: column sums, then rows.
 * ldt_maxpool_argmax: ldt_maxpool (the same bits in out) with arg int32 [G][C] = the row j of [G][n][C] that holds the maximum; on equal
 *   values the smallest j (torch.max on the CPU), a NaN wins and the first one is kept.  relu != 0: out = ReLU(the maximum), which is
 *   max_j ReLU(z_j) without the ReLU'd rows ever stored; arg is the arg-max of z itself.
 * ldt_maxpool_relu_bwd: backward of out = max_j ReLU(z[g][j][c]) from d_out, out fp32 [G][C] and arg: dz[g][j][c] = d_out[g][c] where
 *   j == arg[g][c] and out[g][c] > 0, else 0; EVERY element of dz fp32 [G n][ld] (columns < C) is written.
 * ldt_group_normalize_bwd: backward of ldt_group_normalize with center_mode 0 ('anchor') from dU, fp32 or bf16 [B S k][ld], ld >= 2 D + 3.
 *   Per sample b: d = g - anchor (fp32, as the forward rounds it), n_el = S k (D + 3), m = mean(d), sigma = unbiased std(d) and
 *   inv = 1 / (sigma + 1e-5) from the forward's own statistics kernel, q = alpha dU[:, :D+3], P_b = sum q d.
 *     dbeta[c] = sum dU[:, c],  dalpha[c] = sum_b inv_b sum dU[:, c] d[:, c]                      fp32 [D + 3], each nullable
 *     dd = q inv - P_b inv^2 (d - m) / ((n_el - 1) sigma)
 *     dfeat[b][p][c] = sum over the (s, j) with knn[b][s][j] == p of dd[s][j][c], in ascending (s, j),
 *                    + sum over the s with fps[b][s] == p of (-sum_j dd[s][j][c] + sum_j dU[s][j][D + 3 + c]), in ascending s    fp32 [B][n][D]
 *   (nullable; every element is written, a point in no group gets exactly 0; xyz is data and has no gradient).  inv_start int32 [B][n + 1]
 *   and inv_entry int32 [B][S k] are the inverted index of knn_idx: the entries s k + j of point p of sample b are
 *   inv_entry[b][inv_start[b][p] .. inv_start[b][p + 1]), ascending (a stable sort of knn_idx: integer bookkeeping, the caller's).  The sums
 *   run in float64 in those orders and are rounded once: no atomics.  sigma == 0 (every d of a sample equal) has no defined gradient
 *   upstream (inf * 0): the kernel then writes dd = q inv, the statistics term dropped.  An index outside its range contributes nothing.
 *   The shape must leave n_el >= 2. */
int ldt_bn_stats(const float* x, int64_t ldx, int64_t M, int32_t C, double eps, float* stats, float* running_mean, float* running_var,
                 double momentum, void* stream);
int ldt_bn_relu_fwd(const float* x, int64_t ldx, int64_t M, int32_t C, const float* stats, const float* gamma, const float* beta, void* y,
                    int64_t ldy, int32_t out_bf16, int32_t cols_pad, void* stream);
int ldt_bn_relu_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t M, int32_t C, const float* stats, const float* gamma,
                    const float* beta, float* dx, int64_t lddx, float* dgamma, float* dbeta, void* stream);
int ldt_maxpool_argmax(const void* in, int32_t in_bf16, int64_t ld, int64_t G, int32_t n, int32_t C, float* out, int32_t* arg, int32_t relu,
                       void* stream);
int ldt_maxpool_relu_bwd(const float* d_out, const float* out, const int32_t* arg, int64_t G, int32_t n, int32_t C, float* dz, int64_t ld,
                         void* stream);
int ldt_group_normalize_bwd(const void* dU, int32_t dU_bf16, int64_t ld, const float* feat, const float* xyz, const int32_t* fps_idx,
                            const int32_t* knn_idx, const int32_t* inv_start, const int32_t* inv_entry, const float* alpha, int32_t B,
                            int32_t n, int32_t S, int32_t k, int32_t D, float* dalpha, float* dbeta, float* dfeat, void* stream);

/* ---- fused MLP half of a narrow ResidualBlock (the Compressor's d = 128 blocks; model/layers.py:219,226 + :110-133) ----
 * In place on x fp32 [M][ldx]:  x += gate * (W_dn . GELU(W_up . h + b_up) + b_dn),  h = LN(x) * ln_w + ln_b  (affine,
 * no-condition blocks) or LN(x) * (1 + scale) + shift (AdaLN; shift/scale/gate are per-sample vectors, sample =
 * row / rows_per_sample, consecutive samples mod_sample_stride floats apart).  C in {64, 128}; w_up bf16 [4C][C],
 * w_dn bf16 [C][4C], both row-major and dense.  One pass over x instead of LayerNorm + two GEMMs.
 * x_bf16 (or NULL): bf16 [M][ldxb] copy of the updated x, written in the same pass — the next DecoderBlock level reads the
 * decoded set as its K/V source (Network.py:229 `att(x, o)`), which otherwise costs a separate cast pass over x. */
int ldt_ln_mlp_resid(float* x, int64_t ldx, int64_t M, int32_t C, const float* ln_w, const float* ln_b,
                     const float* shift, const float* scale, const float* gate, int64_t mod_sample_stride,
                     int32_t rows_per_sample, const uint16_t* w_up, const float* b_up, const uint16_t* w_dn,
                     const float* b_dn, uint16_t* x_bf16, int64_t ldxb, void* stream);

/* The same kernel followed, on the rows it has just produced, by the NEXT block's LayerNorm + first projection
 * (model/layers.py:218 / :225 of the ResidualBlock that follows: nx_out bf16 [M][nx_ldo] = LN(x_new)[nx affine | nx modulated] . nx_w^T
 * + nx_bias, nx_w bf16 [nx_N][C], nx_N a multiple of 64) — what ldt_ln_linear would compute from x_new in a pass of its own.  In the
 * Compressor's decoder that is the next level's query projection (Network.py:80-83 via layers.py:225). */
int ldt_ln_mlp_resid_next(float* x, int64_t ldx, int64_t M, int32_t C, const float* ln_w, const float* ln_b,
                          const float* shift, const float* scale, const float* gate, int64_t mod_sample_stride,
                          int32_t rows_per_sample, const uint16_t* w_up, const float* b_up, const uint16_t* w_dn,
                          const float* b_dn, uint16_t* x_bf16, int64_t ldxb,
                          const float* nx_ln_w, const float* nx_ln_b, const float* nx_shift, const float* nx_scale,
                          int64_t nx_mod_sample_stride, int32_t nx_rows_per_sample, const uint16_t* nx_w, const float* nx_bias,
                          int32_t nx_N, uint16_t* nx_out, int64_t nx_ldo, void* stream);

/* LayerNorm + linear for the same narrow blocks: out bf16 [M][ldo] = LN(x)[affine | modulated] . W^T + bias, W bf16 [N][C]
 * dense, N % 64 == 0, C in {64, 128} — fc_q (and fc_kv when the block attends to its own normalised input,
 * model/layers.py:184-189) fed straight from the LayerNorm without writing the normalised activations. */
int ldt_ln_linear(const float* x, int64_t ldx, int64_t M, int32_t C, const float* ln_w, const float* ln_b,
                  const float* shift, const float* scale, int64_t mod_sample_stride, int32_t rows_per_sample,
                  const uint16_t* w, const float* bias, int32_t N, uint16_t* out, int64_t ldo, void* stream);

/* ---- generation-quality metrics of the validation loop (evaluation/evaluation_metrics.py:112-277) ----
 * ldt_chamfer_pairwise: cd[s][r] = dl.mean(1) + dr.mean(1) of distChamfer(x[s], y[r]) for all S*R cloud pairs — the
 *   matrix `_pairwise_CD_` (:165-199) / `_pairwise_EMD_CD_` (:112-162) build row by row.  x fp32 [S][n][3],
 *   y fp32 [R][m][3], cd fp32 [S][R].
 * ldt_emd_approx: transport cost of the approximate matching of
 *   evaluation/pytorch_structural_losses/src/approxmatch.cu (approxmatchkernel :3-186 + matchcostkernel :188-224),
 *   i.e. what `match_cost(xyz1, xyz2)` returns (emd_approx_cuda, evaluation_metrics.py:40-46, divides it by n).
 *   pairwise = 0: out[b] for the pairs (x[b], y[b]), S == R;  pairwise = 1: out[s][r] for all S*R pairs.
 *   n + m <= 7680 points (both clouds and the marginals stay in LDS). */
int ldt_chamfer_pairwise(const float* x, const float* y, int32_t S, int32_t R, int32_t n, int32_t m, float* cd, void* stream);
int ldt_emd_approx(const float* x, const float* y, int32_t S, int32_t R, int32_t n, int32_t m, int32_t pairwise,
                   float* out, void* stream);

/* ---- Score network forward: model/scorenet/score.py:117-151 (Transformer path, unet False) ------------- */
typedef struct ldt_score_plan {
    int32_t hidden, heads, blocks, z_dim, z_pad, mlp_hidden, tokens, batch;
    /* packed weights (bf16 [N][K] row-major, K padded) and fp32 biases */
    const uint16_t* w_in;  const float* b_in;                       /* ln_in   [hidden][z_pad]       score.py:110 */
    const uint16_t* w_qkv[LDT_MAX_BLOCKS]; const float* b_qkv[LDT_MAX_BLOCKS]; /* fc_q|fc_kv rows q,k,v [3h][h] layers.py:159-160 */
    const uint16_t* w_o[LDT_MAX_BLOCKS];   const float* b_o[LDT_MAX_BLOCKS];   /* fc_o   [h][h]        layers.py:161 */
    const uint16_t* w_up[LDT_MAX_BLOCKS];  const float* b_up[LDT_MAX_BLOCKS];  /* mlp.fc.0.0 [4h][h]   layers.py:121 */
    const uint16_t* w_dn[LDT_MAX_BLOCKS];  const float* b_dn[LDT_MAX_BLOCKS];  /* mlp.out [h][4h]      layers.py:124 */
    const uint16_t* w_out; const float* b_out;                      /* ln_out.ln [z_dim][hidden]     layers.py:239 */
    /* Optional cross-attention (ViPC: even blocks attend to the point-cloud condition, score.py:148-149 with
       layers.py:183-189 y != None): when kv_cond[l] != NULL block l takes K|V from kv_cond[l]
       [batch*cond_tokens][2*hidden] bf16 — fc_kv applied to the RAW condition tokens, step-invariant, so the caller
       projects it once per sample() call — and projects only the query with w_q[l]/b_q[l] ([hidden][hidden]). */
    const uint16_t* w_q[LDT_MAX_BLOCKS];   const float* b_q[LDT_MAX_BLOCKS];
    const uint16_t* kv_cond[LDT_MAX_BLOCKS];
    int32_t cond_tokens; int32_t _pad0;
    /* AdaLN modulation: mod[step][sample][blocks*6*hidden + 2*hidden] fp32.  Block l at l*6*hidden:
       shift_msa|scale_msa|gate_msa|shift_mlp|scale_mlp|gate_mlp (layers.py:214); FinalLayer shift|scale (:244) last. */
    const float* mod; int64_t mod_step_stride; int64_t mod_sample_stride;
    /* workspace (caller-owned), M = batch*tokens rows */
    uint16_t* xin;   /* [M][z_pad]       */
    float*    X;     /* [M][hidden] fp32 residual stream */
    uint16_t* Hb;    /* [M][hidden]      */
    uint16_t* QKV;   /* [M][3*hidden]    */
    uint16_t* Ob;    /* [M][hidden]  == [B][H][T][Dh] */
    uint16_t* U;     /* [M][mlp_hidden]  */
    /* Optional LN folding (see ldt_gemm_resid_lnstats): fold[step][blocks][S_qkv 3h | C_qkv 3h | S_up mlp | C_up mlp] fp32
       built by the host from mod and the packed weights; stats = fp32 scratch [hidden/256][M][2].  Used when both are
       non-NULL, mod_sample_stride == 0, no cross-attention, M % 256 == 0, hidden % 256 == 0 <= 1024, mlp_hidden % 256 == 0;
       otherwise the LayerNorm kernels run (the host passes fold only where whole 256x256 tiles fill the chip). */
    const float* fold; int64_t fold_step_stride; float* stats;
    /* Cap on the persistent GEMM grids of this plan (0 = one workgroup per CU = 256).  Two sub-batches sampled on two
       streams give each plan 128: their kernels then share the chip CU-wise and one stream's HBM-bound epilogues /
       attention overlap the other's MFMA-bound main loops (ldt_amd/diffusion.py, `streams`). */
    int32_t gemm_wgs;
    /* ldt_sample_loop only: with fold_monitor set, the steps i with i % fold_monitor_every == 0 and the last step run the monitored
       forward, the others the plain one (0 = every step).  47 monitor launches of ~5 us per monitored forward: every 50th step costs
       0.05 % of a call and the running maximum covers the whole trajectory, not its two ends. */
    int32_t fold_monitor_every;
    /* Optional LN-folding monitor (NULL = off): one device float, raised (atomic max; zero it first) after every folded
       residual GEMM of a forward to max over rows of mean^2 / variance of that GEMM's output — the quantity that scales
       the folded projections' rounding error, (1 + mean^2 / variance) x the LayerNorm kernel's.  The sampler sets it on a
       probe forward before the loop and, since round 6, inside the loop every fold_monitor_every steps (ldt_amd/diffusion.py),
       and reads the running maximum once when the loop has ended. */
    float* fold_monitor;
} ldt_score_plan;

/* Which LN-folded route ldt_score_forward takes for a batch of M = batch*tokens rows (hidden D, mlp_hidden F, gemm_wgs as in the plan) when the plan
 * offers `fold` tables: 0 = none (LayerNorm kernels), 1 = the 256-tile kernels (statistics per 256 columns), 2 = the mid-size tile kernels of small
 * batches (statistics per 32 columns).  The host (Score.can_fold) asks before it builds the tables. */
int ldt_score_lnfold_route(int32_t M, int32_t D, int32_t F, int32_t gemm_wgs);

/* eps_out[M][z_dim] = Score(x[M][z_dim]) with the AdaLN row selected by *step_ptr (NULL = row 0). */
int ldt_score_forward(const ldt_score_plan* plan, const float* x, float* eps_out,
                      const int32_t* step_ptr, void* stream);

/* Same forward with a hipEvent pair around EVERY launch (same stream); returns summed milliseconds and launch
 * counts per kernel class.  Synchronises the stream.  bench.py's live roofline measurement. */
enum ldt_prof_class {
    LDT_PROF_OTHER = 0,       /* cast/pad */
    LDT_PROF_GEMM_IO = 1,     /* ln_in, FinalLayer.ln      (gemm<F32>)   */
    LDT_PROF_LN = 2,          /* LayerNorm + AdaLN modulate               */
    LDT_PROF_GEMM_QKV = 3,    /* fc_q|fc_kv                (gemm<BF16>)  */
    LDT_PROF_ATTN = 4,        /* fused attention                          */
    LDT_PROF_GEMM_O = 5,      /* fc_o + gate + residual    (gemm<RESID>, K = hidden)     */
    LDT_PROF_GEMM_GELU = 6,   /* mlp.fc + GELU             (gemm<GELU>)  */
    LDT_PROF_GEMM_DN = 7,     /* mlp.out + gate + residual (gemm<RESID>, K = mlp_hidden) */
    LDT_PROF_NCLASS = 8
};
int ldt_score_forward_profile(const ldt_score_plan* plan, const float* x, float* eps_out, const int32_t* step_ptr,
                              float* ms_by_class, int32_t* launches_by_class, void* stream);

/* Per-sample conditioning inside the loop (label / ViPC image embedding, score.py:125-135): the AdaLN rows then
 * differ per sample and per step, c[b] = TimeEmbedding(t_i) + extra[b], mod[b] = W_ada · SiLU(c[b]) + b_ada, and are
 * recomputed every step by two extra launches (row add, fp32 SGEMM over the stacked adaLN weights). */
typedef struct ldt_cond_args {
    const float* temb;    /* [n_steps][t_dim]  TimeEmbedding(t_i) for every step (host builds it once per call) */
    const float* extra;   /* [batch][t_dim]    label / image-condition embedding, or NULL */
    const float* w_ada;   /* [n_mod][t_dim]    every block's adaLN.1 weight stacked in plan order (+ FinalLayer's); may be NULL when w_ada_bf16 is given */
    const float* b_ada;   /* [n_mod] */
    float* c_buf;         /* [batch][t_dim]    scratch */
    float* mod_buf;       /* [batch][n_mod]    scratch; plan->mod must point here with mod_sample_stride = n_mod */
    int32_t t_dim, n_mod;
    /* optional (both or neither): the stacked adaLN weights as a bf16 panel [n_mod][t_dim] and a bf16 scratch [batch][t_dim].  When
     * given, the per-step rows are one bf16 MFMA GEMM (fp32 accumulation and bias) that streams 2 bytes per weight instead of 4 —
     * the fp32 form is HBM-bound on its 4 n_mod t_dim bytes per step (BASELINE configs[4]: 604 MB, 9 % of a step).  Rows then carry
     * bf16 operand rounding (relative MSE ~5e-6), like every token GEMM of the model.  The MFMA GEMM needs t_dim % 64 == 0: with another
     * width the loop uses the fp32 w_ada rows if they were given too, and returns LDT_ESHAPE otherwise. */
    const void* w_ada_bf16;
    void* c_buf_bf16;
} ldt_cond_args;

/* The whole reverse-SDE loop (pc_sampling, diffusion_continuous.py:231-258 with corrector None): n_steps x
 * [(AdaLN rows if cond) -> Score forward -> predictor update -> ++step].  x is updated in place, x_mean receives the
 * last x_mean (denoise=True returns it, quirk Q8).  step_counter: device int32 scratch.  cond: NULL for the
 * unconditional sampler (plan->mod = table of all steps).  x_traj: NULL, or [n_steps][batch*tokens*z_dim] fp32 that
 * receives x after every step (the per-step parity curve against the CPU reference).  use_graph != 0 captures one step
 * into a hipGraph and replays it. */
int ldt_sample_loop(const ldt_score_plan* plan, float* x, float* x_mean, float* eps_tmp,
                    const float* coef, int32_t mode, const float* noise, int64_t noise_step_stride,
                    int64_t elem_offset, uint64_t seed, int32_t* step_counter, int32_t n_steps,
                    const ldt_cond_args* cond, float* x_traj, int32_t use_graph, void* stream);

/* ---- measurement knob (tools/dbg/gm_bench.py): rows per group of the persistent GEMM's grouped tile order
 * (1 = row-major, the default; LDT_GEMM_GM sets it at start-up).  Process-wide; not used by the product path. */
int ldt_dbg_gemm_group_m(int32_t rows_per_group);
/* tools/dbg/epi_ablate.py: skip parts of the residual epilogue (bit 1 residual read, 2 fp32 store, 4 bf16 x(1+scale) store,
 * 8 row statistics) to attribute its time; -1 restores the product behaviour.  Process-wide; not used by the product path. */
int ldt_dbg_gemm_epi(int32_t bits);

#ifdef __cplusplus
}
#endif
#endif
