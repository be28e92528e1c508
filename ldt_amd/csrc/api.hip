// C-ABI of libldt_hip.so (include/ldt_hip.h), the part that is not one op: the error state, the GEMM and attention entries (they build
// GemmArgs / AttnArgs for the launchers of the kernel families), and the two host-side orchestrators that enqueue the whole Score forward /
// reverse-SDE loop on one HIP stream.  Every other op's entry is in the file of its kernel.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/ldt_hip.h"
#include "kernels.h"

// ------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

void ldt_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int ldt_check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ldt_set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return LDT_OK;
}
extern "C" const char* ldt_last_error(void) { return g_err; }
extern "C" int ldt_abi_version(void) { return LDT_ABI_VERSION; }

// ------------------------------------------------------------------------------ argument blocks
#define TRY(expr)                   \
    do {                            \
        const int _rc = (expr);     \
        if (_rc != LDT_OK) return _rc; \
    } while (0)

// GemmArgs by name: the base problem, then what an epilogue or a fused form adds (everything else stays zero)
static GemmArgs gemm_args(const bf16_t* X, long ldx, const bf16_t* W, long ldw, const float* bias, void* out, long ldo, int M, int N, int K, int max_wgs) {
    GemmArgs a{};
    a.X = X; a.ldx = ldx; a.W = W; a.ldw = ldw; a.bias = bias; a.out = out; a.ldo = ldo; a.M = M; a.N = N; a.K = K; a.max_wgs = max_wgs;
    return a;
}
static void gemm_add_gated_resid(GemmArgs& a, const float* resid, long ldr, const float* gate, long sample_stride, int rows_per_sample, const int* step_ptr, long step_stride) {
    a.resid = resid; a.ldr = ldr; a.gate = gate; a.gate_sample_stride = sample_stride; a.rows_per_sample = rows_per_sample;
    a.step_ptr = step_ptr; a.gate_step_stride = step_stride;
}
static void gemm_add_fold_producer(GemmArgs& a, bf16_t* xs, long ldxs, const float* ln_scale, long ln_step_stride, float* stats_out, int stats_parts) {
    a.xs = xs; a.ldxs = ldxs; a.ln_scale = ln_scale; a.ln_step_stride = ln_step_stride; a.stats_out = stats_out; a.stats_parts = stats_parts;
}
static void gemm_add_fold_consumer(GemmArgs& a, const float* stats_in, int stats_parts, const float* fold_S, const float* fold_C, long step_stride, const int* step_ptr) {
    a.stats_in = stats_in; a.stats_parts = stats_parts; a.fold_S = fold_S; a.fold_C = fold_C; a.fold_step_stride = step_stride; a.step_ptr = step_ptr;
}
static void gemm_add_attention(GemmArgs& a, bf16_t* attn_o, float scale_log2e, const bf16_t* k, const bf16_t* v, long ldkv, long kv_batch_stride) {
    a.attn_o = attn_o; a.attn_scale_log2e = scale_log2e; a.attn_k = k; a.attn_v = v; a.attn_ldkv = ldkv; a.attn_kv_batch_stride = kv_batch_stride;
}

// ------------------------------------------------------------------------------ GEMM and attention entries
extern "C" int ldt_gemm_bf16(int32_t epilogue, const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw,
                             const float* bias, void* out, int64_t ldo, const float* resid, int64_t ldr,
                             const uint16_t* skip, int64_t ldskip, const float* gate, int64_t gate_sample_stride,
                             int32_t rows_per_sample, const int32_t* step_ptr, int64_t gate_step_stride,
                             int32_t M, int32_t N, int32_t K, void* stream) {
    LDT_REQUIRE(X && W && out, LDT_EARG, "gemm: null pointer");
    GemmArgs a = gemm_args(ldt_bf16(X), ldx, ldt_bf16(W), ldw, bias, out, ldo, M, N, K, 0);
    gemm_add_gated_resid(a, resid, ldr, gate, gate_sample_stride, rows_per_sample, step_ptr, gate_step_stride);
    a.skip = ldt_bf16(skip); a.lds_ = ldskip;
    return ldt_gemm_launch(epilogue, &a, ldt_stream(stream));
}

extern "C" int ldt_gemm_resid_lnstats(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias,
                                      float* out, int64_t ldo, const float* gate, int64_t gate_sample_stride,
                                      int32_t rows_per_sample, const float* ln_scale, uint16_t* xs, int64_t ldxs,
                                      float* stats_out, const int32_t* step_ptr, int64_t gate_step_stride,
                                      int64_t ln_step_stride, int32_t M, int32_t N, int32_t K, int32_t stats_parts, void* stream) {
    LDT_REQUIRE(X && W && out && xs && ln_scale && stats_out, LDT_EARG, "gemm_resid_lnstats: null pointer");
    LDT_REQUIRE(stats_parts == N / 256 || stats_parts == N / 32, LDT_EARG, "gemm_resid_lnstats: stats_parts=%d is neither N/256 nor N/32 (N=%d)", stats_parts, N);
    GemmArgs a = gemm_args(ldt_bf16(X), ldx, ldt_bf16(W), ldw, bias, out, ldo, M, N, K, 0);
    gemm_add_gated_resid(a, out, ldo, gate, gate_sample_stride, rows_per_sample, step_ptr, gate_step_stride);
    gemm_add_fold_producer(a, ldt_bf16_mut(xs), ldxs, ln_scale, ln_step_stride, stats_out, stats_parts);
    return ldt_gemm_lnfold_launch(EPI_RESID_F32, &a, ldt_stream(stream));
}

extern "C" int ldt_gemm_lnfold(int32_t epilogue, const uint16_t* Xs, int64_t ldx, const uint16_t* W, int64_t ldw,
                               const float* stats_in, const float* fold_S, const float* fold_C, uint16_t* out, int64_t ldo,
                               const int32_t* step_ptr, int64_t fold_step_stride, int32_t M, int32_t N, int32_t K, int32_t stats_parts,
                               void* stream) {
    LDT_REQUIRE(Xs && W && out && stats_in && fold_S && fold_C, LDT_EARG, "gemm_lnfold: null pointer");
    LDT_REQUIRE(stats_parts == K / 256 || stats_parts == K / 32, LDT_EARG, "gemm_lnfold: stats_parts=%d is neither K/256 nor K/32 (K=%d)", stats_parts, K);
    GemmArgs a = gemm_args(ldt_bf16(Xs), ldx, ldt_bf16(W), ldw, nullptr, out, ldo, M, N, K, 0);
    gemm_add_fold_consumer(a, stats_in, stats_parts, fold_S, fold_C, fold_step_stride, step_ptr);
    return ldt_gemm_lnfold_launch(epilogue, &a, ldt_stream(stream));
}

extern "C" int ldt_attention_fwd(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K,
                                 int64_t ldk, const uint16_t* V, int64_t ldv, int64_t kv_batch_stride, uint16_t* O,
                                 int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim, void* stream) {
    LDT_REQUIRE(Q && K && V && O, LDT_EARG, "attention: null pointer");
    AttnArgs a{ldt_bf16(Q), ldq, q_batch_stride, ldt_bf16(K), ldk, kv_batch_stride, ldt_bf16(V), ldv, ldt_bf16_mut(O), B, H, Nq, Nk,
               1.4426950408889634f / sqrtf((float)head_dim), nullptr, nullptr, nullptr, 0, nullptr, 0};
    return ldt_attn_launch(&a, head_dim, ldt_stream(stream));
}
extern "C" int ldt_attention_route(int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim) { return ldt_attn_route(B, H, Nq, Nk, head_dim); }
extern "C" int ldt_gemm_route(int32_t epilogue, int32_t M, int32_t N, int32_t K, int64_t ldo, int32_t fold, int32_t max_wgs) {
    GemmArgs a{};
    a.M = M; a.N = N; a.K = K; a.ldo = ldo; a.ldr = ldo; a.max_wgs = max_wgs;
    if (fold != 0 && fold != 32 && fold != 256) return 0;
    const GemmRoute r = ldt_gemm_decide(epilogue, &a, fold);
    return (r.family << 28) | ((r.tiles_per_wg < 255 ? r.tiles_per_wg : 255) << 20) | (r.bm << 10) | r.bn;
}
extern "C" int ldt_attention_oproj_resid(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K,
                                         int64_t ldk, const uint16_t* V, int64_t ldv, int64_t kv_batch_stride,
                                         int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim,
                                         const uint16_t* Wo, const float* bo, float* X, int64_t ldx, const float* gate,
                                         int64_t gate_sample_stride, void* stream) {
    LDT_REQUIRE(Q && K && V && Wo && bo && X, LDT_EARG, "attention_oproj: null pointer");
    AttnArgs a{ldt_bf16(Q), ldq, q_batch_stride, ldt_bf16(K), ldk, kv_batch_stride, ldt_bf16(V), ldv, nullptr, B, H, Nq, Nk,
               1.4426950408889634f / sqrtf((float)head_dim), ldt_bf16(Wo), bo, X, ldx, gate, gate_sample_stride};
    return ldt_attn_oproj_launch(&a, head_dim, ldt_stream(stream));
}

// ------------------------------------------------------------------------------ Score forward
extern "C" int ldt_score_lnfold_route(int32_t M, int32_t D, int32_t F, int32_t gemm_wgs) {
    return ldt_score_fold_decide(M, D, F, gemm_wgs).route;
}

static int check_plan(const ldt_score_plan* p) {
    LDT_REQUIRE(p, LDT_EARG, "score: null plan");
    LDT_REQUIRE(p->blocks > 0 && p->blocks <= LDT_MAX_BLOCKS, LDT_ESHAPE, "score: blocks=%d out of range", p->blocks);
    LDT_REQUIRE(p->hidden > 0 && p->heads > 0 && p->hidden % p->heads == 0, LDT_ESHAPE, "score: hidden %% heads");
    const int dh = p->hidden / p->heads;
    LDT_REQUIRE(dh == 8 || dh == 16 || dh == 32 || dh == 64, LDT_ESHAPE, "score: head dim %d not built (8, 16, 32, 64)", dh);
    LDT_REQUIRE(p->hidden % 64 == 0 && p->mlp_hidden % 64 == 0 && p->z_pad % 64 == 0 && p->z_pad >= p->z_dim, LDT_ESHAPE,
                "score: hidden/mlp_hidden/z_pad must be multiples of 64");
    LDT_REQUIRE(p->z_dim % 4 == 0, LDT_ESHAPE, "score: z_dim %% 4");
    LDT_REQUIRE(p->tokens > 0 && p->batch > 0, LDT_ESHAPE, "score: empty batch");
    LDT_REQUIRE(p->w_in && p->w_out && p->mod && p->xin && p->X && p->Hb && p->QKV && p->Ob && p->U, LDT_EARG, "score: null buffer in plan");
    for (int l = 0; l < p->blocks; ++l) {
        LDT_REQUIRE(p->w_qkv[l] && p->w_o[l] && p->w_up[l] && p->w_dn[l], LDT_EARG, "score: block %d weights missing", l);
        LDT_REQUIRE(!p->kv_cond[l] || (p->w_q[l] && p->cond_tokens > 0), LDT_EARG, "score: block %d cross-attention needs w_q and cond_tokens", l);
    }
    return LDT_OK;
}

// Optional per-launch HIP-event timing (bench.py's live roofline measurement): events are recorded on the
// SAME stream the kernels run on, bracketing every launch; elapsed times are summed per kernel class.
struct Prof {
    hipStream_t s;
    std::vector<hipEvent_t> ev;      // 2 per launch
    std::vector<int> cls;
    void begin(int c) { hipEvent_t a, b; (void)hipEventCreate(&a); (void)hipEventCreate(&b); ev.push_back(a); ev.push_back(b); cls.push_back(c); (void)hipEventRecord(a, s); }
    void end() { (void)hipEventRecord(ev.back(), s); }
    void cancel() { (void)hipEventDestroy(ev.back()); ev.pop_back(); (void)hipEventDestroy(ev.back()); ev.pop_back(); cls.pop_back(); }   // begin() without a launch
};
// a `..._try` launcher (fused QKV + attention forms): timed as class cls_ when it takes the launch
#define LAUNCH_TRY(cls_, took_, try_expr, st_)      \
    do {                                            \
        if (prof) prof->begin(cls_);                \
        took_ = (try_expr);                         \
        if (prof) { if (took_) prof->end(); else prof->cancel(); } \
        if (took_ && (st_) != LDT_OK) return (st_); \
    } while (0)
#define LAUNCH(cls_, expr)                \
    do {                                  \
        if (prof) prof->begin(cls_);      \
        const int _rc = (expr);           \
        if (prof) prof->end();            \
        if (_rc != LDT_OK) return _rc;    \
    } while (0)

// The "q | k | v projection + attention" step of a Score block, exactly as the forward launches it (also exported: ldt_qkv_attention).
// Self-attention (kv == nullptr): W = [q | k | v] rows (N = 3 * hidden); cross-attention: W = the q rows (N = hidden), K | V = the cached
// condition rows kv / kv + hidden.  Folded (stats != nullptr): X = xs of the LN-folded producer, the consumer's S | C at fold_S / fold_C.
struct QkvAttnStep {
    const bf16_t* X; long ldx; const bf16_t* W; long ldw; const float* bias;
    const float* stats; int stats_parts; const float* fold_S; const float* fold_C; long fold_step_stride;
    const bf16_t* kv; long ldkv; long kv_batch_stride;
    bf16_t* attn_o; bf16_t* QKV;
    int B, tokens, cond_tokens, hidden, heads, K, max_wgs;
    const int* step_ptr;
};
// 0 = two kernels (GEMM + attention), 1 = 32-token self form, 2 = 256-token self form, 3 = 32 x 32-token cross form: the fused forms'
// shape rules in the order qkv_attention_step tries them
static int qkv_attention_route(const GemmArgs* g, int tokens, int cond_tokens, int head_dim, bool cross, bool folded) {
    if (cross) return ldt_gemm_mid_q_xattn_takes(g, tokens, cond_tokens, head_dim) ? 3 : 0;
    if (ldt_gemm_mid_qkv_attn_takes(g, tokens, head_dim, folded)) return 1;
    return ldt_gemm_qkv_attn256_takes(g, tokens, head_dim, folded) ? 2 : 0;
}
static int qkv_attention_step(const QkvAttnStep& q, hipStream_t s, Prof* prof) {
    const int D = q.hidden, T = q.tokens, dh = D / q.heads;
    const bool cross = q.kv != nullptr, folded = q.stats != nullptr;
    const float scale_log2e = 1.4426950408889634f / sqrtf((float)dh);
    GemmArgs gq = gemm_args(q.X, q.ldx, q.W, q.ldw, q.bias, q.QKV, 3L * D, q.B * T, cross ? D : 3 * D, q.K, q.max_wgs);
    if (folded) gemm_add_fold_consumer(gq, q.stats, q.stats_parts, q.fold_S, q.fold_C, q.fold_step_stride, q.step_ptr);
    if (cross) gemm_add_attention(gq, q.attn_o, scale_log2e, q.kv, q.kv + D, q.ldkv, q.kv_batch_stride);
    else gemm_add_attention(gq, q.attn_o, scale_log2e, nullptr, nullptr, 0, 0);
    int fst = LDT_OK;
    bool took = false;
    // projection + attention in one launch, q | k | v never reach HBM: 32 x 32 tokens against the condition (gemm_mid.hip, mid_epilogue_xattn);
    // 32-token samples (gemm_mid.hip, mid_epilogue_attn); 256-token samples (the 256 x 192-tile form of the persistent kernel)
    if (cross) LAUNCH_TRY(LDT_PROF_GEMM_QKV, took, ldt_gemm_mid_q_xattn_try(&gq, T, q.cond_tokens, dh, s, &fst), fst);
    else {
        LAUNCH_TRY(LDT_PROF_GEMM_QKV, took, ldt_gemm_mid_qkv_attn_try(&gq, T, dh, folded, s, &fst), fst);
        if (!took) LAUNCH_TRY(LDT_PROF_GEMM_QKV, took, ldt_gemm_qkv_attn256_try(&gq, T, dh, folded, s, &fst), fst);
    }
    if (took) return LDT_OK;
    if (folded) LAUNCH(LDT_PROF_GEMM_QKV, ldt_gemm_lnfold_launch(LDT_EPI_BF16, &gq, s));
    else LAUNCH(LDT_PROF_GEMM_QKV, ldt_gemm_launch(LDT_EPI_BF16, &gq, s));
    const int S = cross ? q.cond_tokens : T;
    AttnArgs at{q.QKV, 3L * D, (long)T * 3 * D, cross ? q.kv : q.QKV + D, cross ? q.ldkv : 3L * D, cross ? q.kv_batch_stride : (long)T * 3 * D,
                cross ? q.kv + D : q.QKV + 2 * D, cross ? q.ldkv : 3L * D, q.attn_o, q.B, q.heads, T, S, scale_log2e};
    LAUNCH(LDT_PROF_ATTN, ldt_attn_launch(&at, dh, s));
    return LDT_OK;
}

extern "C" int ldt_qkv_attention_route(int32_t B, int32_t tokens, int32_t cond_tokens, int32_t hidden, int32_t heads, int32_t K, int32_t fold,
                                       int32_t max_wgs) {
    if (B <= 0 || tokens <= 0 || hidden <= 0 || heads <= 0 || hidden % heads != 0 || (fold != 0 && fold != 32 && fold != 256) || (fold && cond_tokens > 0)) return 0;
    GemmArgs g{};
    g.M = B * tokens; g.N = cond_tokens > 0 ? hidden : 3 * hidden; g.K = K; g.max_wgs = max_wgs;
    g.stats_parts = fold ? K / fold : 0;
    return qkv_attention_route(&g, tokens, cond_tokens, hidden / heads, cond_tokens > 0, fold != 0);
}
extern "C" int ldt_qkv_attention(const uint16_t* X, int64_t ldx, const uint16_t* W, int64_t ldw, const float* bias,
                                 const float* stats, int32_t stats_parts, const float* fold_S, const float* fold_C, int64_t fold_step_stride,
                                 const uint16_t* kv_cond, int64_t ldkv, int64_t kv_batch_stride, uint16_t* O, uint16_t* QKV,
                                 int32_t B, int32_t tokens, int32_t cond_tokens, int32_t hidden, int32_t heads, int32_t K, int32_t max_wgs,
                                 const int32_t* step_ptr, void* stream) {
    LDT_REQUIRE(X && W && O && QKV, LDT_EARG, "qkv_attention: null pointer");
    LDT_REQUIRE(B > 0 && tokens > 0 && hidden > 0 && heads > 0 && hidden % heads == 0 && hidden % 64 == 0 && K > 0, LDT_ESHAPE,
                "qkv_attention: B=%d tokens=%d hidden=%d heads=%d K=%d", B, tokens, hidden, heads, K);
    const int dh = hidden / heads;
    LDT_REQUIRE(dh == 8 || dh == 16 || dh == 32 || dh == 64, LDT_ESHAPE, "qkv_attention: head dim %d not built (8, 16, 32, 64)", dh);
    LDT_REQUIRE(!kv_cond || (cond_tokens > 0 && !stats), LDT_EARG, "qkv_attention: cross-attention needs cond_tokens and has no folded form");
    LDT_REQUIRE(!stats || (fold_S && fold_C && stats_parts > 0 && !bias), LDT_EARG, "qkv_attention: the folded form needs fold_S, fold_C, stats_parts and takes no bias (it is part of fold_C)");
    QkvAttnStep q{};
    q.X = ldt_bf16(X); q.ldx = ldx; q.W = ldt_bf16(W); q.ldw = ldw; q.bias = bias;
    q.stats = stats; q.stats_parts = stats_parts; q.fold_S = fold_S; q.fold_C = fold_C; q.fold_step_stride = fold_step_stride;
    q.kv = ldt_bf16(kv_cond); q.ldkv = ldkv; q.kv_batch_stride = kv_batch_stride; q.attn_o = ldt_bf16_mut(O); q.QKV = ldt_bf16_mut(QKV);
    q.B = B; q.tokens = tokens; q.cond_tokens = cond_tokens; q.hidden = hidden; q.heads = heads; q.K = K; q.max_wgs = max_wgs; q.step_ptr = step_ptr;
    return qkv_attention_step(q, ldt_stream(stream), nullptr);
}

static int score_forward_impl(const ldt_score_plan* p, const float* x, float* eps_out, const int32_t* step_ptr,
                              hipStream_t s, Prof* prof) {
    TRY(check_plan(p));
    LDT_REQUIRE(x && eps_out, LDT_EARG, "score: null x/out");
    const int D = p->hidden, T = p->tokens, M = p->batch * p->tokens, F = p->mlp_hidden;
    const long sstr = p->mod_sample_stride, tstr = p->mod_step_stride;
    // LN folding (gemm256_tile.h): with batch-shared modulation (unconditional sampling) the LayerNorm + modulate between a
    // residual GEMM and the next projection is folded into the two GEMMs' epilogues; the host supplies the per-step
    // S / C tables (plan->fold) when that pays (whole 256x256 tiles that fill the chip: Score.can_fold).
    // Small batches fold through the mid-size tile kernels (statistics per 32 columns), the rest through the 256-tile kernel, below its fill rule too.
    const ScoreFold sf = ldt_score_fold_decide(M, D, F, p->gemm_wgs);
    bool fold = p->fold && p->stats && sstr == 0 && (sf.route == SCORE_FOLD_MID || sf.shape_256);
    for (int l = 0; l < p->blocks && fold; ++l) fold = !p->kv_cond[l];
    const int sparts = D / sf.granule;                          // row-statistics partials per row in plan->stats ([sparts][M][2])
    const long fstep = p->fold_step_stride, fblk = 6L * D + 2L * F;   // per block: S_qkv[3D] | C_qkv[3D] | S_up[F] | C_up[F]
    // ln_in (score.py:136-137): latents fp32 -> bf16 (K padded) -> X fp32
    LAUNCH(LDT_PROF_OTHER, ldt_cast_pad_launch(x, p->z_dim, ldt_bf16_mut(p->xin), p->z_pad, M, p->z_dim, p->z_pad, s));
    const GemmArgs g_in = gemm_args(ldt_bf16(p->xin), p->z_pad, ldt_bf16(p->w_in), p->z_pad, p->b_in, p->X, D, M, D, p->z_pad, p->gemm_wgs);
    LAUNCH(LDT_PROF_GEMM_IO, ldt_gemm_launch(LDT_EPI_F32, &g_in, s));
    for (int l = 0; l < p->blocks; ++l) {                       // score.py:148-149, layers.py:212-219
        const float* m = p->mod + (long)l * 6 * D;              // shift_msa|scale_msa|gate_msa|shift_mlp|scale_mlp|gate_mlp
        const float* fl = fold ? p->fold + (long)l * fblk : nullptr;
        QkvAttnStep qa{};
        qa.X = ldt_bf16(p->Hb); qa.ldx = D; qa.ldw = D; qa.attn_o = ldt_bf16_mut(p->Ob); qa.QKV = ldt_bf16_mut(p->QKV);
        qa.B = p->batch; qa.tokens = T; qa.cond_tokens = p->cond_tokens; qa.hidden = D; qa.heads = p->heads; qa.K = D; qa.max_wgs = p->gemm_wgs; qa.step_ptr = step_ptr;
        if (fold && l > 0) {                                    // Hb = x (1 + scale_msa) and the row statistics came from block l-1's mlp.out
            qa.W = ldt_bf16(p->w_qkv[l]);
            qa.stats = p->stats; qa.stats_parts = sparts; qa.fold_S = fl; qa.fold_C = fl + 3L * D; qa.fold_step_stride = fstep;
        } else {
            LnArgs n1{p->X, D, ldt_bf16_mut(p->Hb), D, nullptr, nullptr, m, m + D, sstr, T, step_ptr, tstr, M, D};
            LAUNCH(LDT_PROF_LN, ldt_ln_launch(&n1, s));
            if (p->kv_cond[l]) {                                // cross-attention: q from the modulated x, K|V from the condition
                qa.W = ldt_bf16(p->w_q[l]); qa.bias = p->b_q[l];
                qa.kv = ldt_bf16(p->kv_cond[l]); qa.ldkv = 2L * D; qa.kv_batch_stride = (long)p->cond_tokens * 2 * D;
            } else {                                            // self-attention: fused q|k|v projection of the modulated x
                qa.W = ldt_bf16(p->w_qkv[l]); qa.bias = p->b_qkv[l];
            }
        }
        TRY(qkv_attention_step(qa, s, prof));
        // fc_o + gate + residual.  Folded: it also emits Hb = x (1 + scale_mlp) and the row statistics, which mlp.fc consumes
        GemmArgs go = gemm_args(ldt_bf16(p->Ob), D, ldt_bf16(p->w_o[l]), D, p->b_o[l], p->X, D, M, D, D, p->gemm_wgs);
        gemm_add_gated_resid(go, p->X, D, m + 2 * D, sstr, T, step_ptr, tstr);
        if (fold) {
            gemm_add_fold_producer(go, ldt_bf16_mut(p->Hb), D, m + 4 * D, tstr, p->stats, sparts);
            LAUNCH(LDT_PROF_GEMM_O, ldt_gemm_lnfold_launch(LDT_EPI_RESID_F32, &go, s));
            if (p->fold_monitor) TRY(ldt_fold_monitor_launch(p->stats, sparts, M, D, p->fold_monitor, s));
        } else {
            LnArgs n2{p->X, D, ldt_bf16_mut(p->Hb), D, nullptr, nullptr, m + 3 * D, m + 4 * D, sstr, T, step_ptr, tstr, M, D};
            LAUNCH(LDT_PROF_GEMM_O, ldt_gemm_launch(LDT_EPI_RESID_F32, &go, s));
            LAUNCH(LDT_PROF_LN, ldt_ln_launch(&n2, s));
        }
        // mlp.fc + GELU (folded: its bias is part of fold_C)
        GemmArgs gu = gemm_args(ldt_bf16(p->Hb), D, ldt_bf16(p->w_up[l]), D, fold ? nullptr : p->b_up[l], p->U, F, M, F, D, p->gemm_wgs);
        if (fold) gemm_add_fold_consumer(gu, p->stats, sparts, fl + 6L * D, fl + 6L * D + F, fstep, step_ptr);
        LAUNCH(LDT_PROF_GEMM_GELU, fold ? ldt_gemm_lnfold_launch(LDT_EPI_GELU_BF16, &gu, s) : ldt_gemm_launch(LDT_EPI_GELU_BF16, &gu, s));
        // mlp.out + gate + residual.  Folded: Hb and the statistics for the next block's scale_msa; the last block's launches unfolded (FinalLayer's LN runs as a kernel)
        GemmArgs gd = gemm_args(ldt_bf16(p->U), F, ldt_bf16(p->w_dn[l]), F, p->b_dn[l], p->X, D, M, D, F, p->gemm_wgs);
        gemm_add_gated_resid(gd, p->X, D, m + 5 * D, sstr, T, step_ptr, tstr);
        if (fold) gemm_add_fold_producer(gd, ldt_bf16_mut(p->Hb), D, m + 6 * D + D, tstr, p->stats, sparts);
        if (fold && l + 1 < p->blocks) {
            LAUNCH(LDT_PROF_GEMM_DN, ldt_gemm_lnfold_launch(LDT_EPI_RESID_F32, &gd, s));
            if (p->fold_monitor) TRY(ldt_fold_monitor_launch(p->stats, sparts, M, D, p->fold_monitor, s));
        } else LAUNCH(LDT_PROF_GEMM_DN, ldt_gemm_launch(LDT_EPI_RESID_F32, &gd, s));
    }
    {                                                           // FinalLayer (layers.py:240-248)
        const float* m = p->mod + (long)p->blocks * 6 * D;
        LnArgs nf{p->X, D, ldt_bf16_mut(p->Hb), D, nullptr, nullptr, m, m + D, sstr, T, step_ptr, tstr, M, D};
        LAUNCH(LDT_PROF_LN, ldt_ln_launch(&nf, s));
        const GemmArgs gf = gemm_args(ldt_bf16(p->Hb), D, ldt_bf16(p->w_out), D, p->b_out, eps_out, p->z_dim, M, p->z_dim, D, p->gemm_wgs);
        LAUNCH(LDT_PROF_GEMM_IO, ldt_gemm_launch(LDT_EPI_F32, &gf, s));
    }
    return LDT_OK;
}

extern "C" int ldt_score_forward(const ldt_score_plan* p, const float* x, float* eps_out, const int32_t* step_ptr, void* stream) {
    return score_forward_impl(p, x, eps_out, step_ptr, ldt_stream(stream), nullptr);
}

extern "C" int ldt_score_forward_profile(const ldt_score_plan* p, const float* x, float* eps_out, const int32_t* step_ptr,
                                         float* ms_by_class, int32_t* launches_by_class, void* stream) {
    LDT_REQUIRE(ms_by_class && launches_by_class, LDT_EARG, "score_profile: null output");
    Prof prof{ldt_stream(stream), {}, {}};
    const int rc = score_forward_impl(p, x, eps_out, step_ptr, ldt_stream(stream), &prof);
    (void)hipStreamSynchronize(ldt_stream(stream));
    for (int c = 0; c < LDT_PROF_NCLASS; ++c) { ms_by_class[c] = 0.f; launches_by_class[c] = 0; }
    for (size_t i = 0; i < prof.cls.size(); ++i) {
        float ms = 0.f;
        if (rc == LDT_OK && hipEventElapsedTime(&ms, prof.ev[2 * i], prof.ev[2 * i + 1]) == hipSuccess) {
            ms_by_class[prof.cls[i]] += ms;
            launches_by_class[prof.cls[i]] += 1;
        }
        (void)hipEventDestroy(prof.ev[2 * i]);
        (void)hipEventDestroy(prof.ev[2 * i + 1]);
    }
    return rc;
}

// ------------------------------------------------------------------------------ reverse-SDE loop
// What a step of the loop works on beside its plan; filled once per ldt_sample_loop.  Every step-dependent operand is indexed by *step_counter.
struct SampleStep {
    float *x, *x_mean, *eps_tmp, *x_traj;
    const float *coef, *noise;
    long noise_step_stride, elem_offset;
    uint64_t seed;
    int mode, *step_counter;
    const ldt_cond_args* cond;                                  // null: batch-shared AdaLN rows, indexed by the step inside the forward
};

// One step = four launches: (conditioned) AdaLN rows of this step, Score forward, sampler update, ++*step_counter.
static int enqueue_step(const SampleStep& st, const ldt_score_plan* p, hipStream_t s) {
    if (const ldt_cond_args* cond = st.cond) {                  // per-sample AdaLN rows of this step
        TRY(ldt_cond_rows_launch(cond->temb, cond->extra, cond->c_buf, cond->c_buf_bf16, st.step_counter, p->batch, cond->t_dim, 1, s));   // c_buf = silu(c)
        if (cond->w_ada_bf16 && (cond->t_dim % 64 == 0 || !cond->w_ada)) {   // bf16 weight panel: half the bytes of the HBM-bound row GEMM (fp32 accumulation + bias); a width the MFMA GEMM does not take falls back to the fp32 rows when they were given
            const GemmArgs g = gemm_args(ldt_bf16(cond->c_buf_bf16), cond->t_dim, ldt_bf16(cond->w_ada_bf16), cond->t_dim, cond->b_ada, cond->mod_buf, cond->n_mod,
                                         p->batch, cond->n_mod, cond->t_dim, p->gemm_wgs);
            TRY(ldt_gemm_launch(EPI_F32, &g, s));
        } else {
            SgemmArgs g{cond->c_buf, cond->t_dim, cond->w_ada, cond->t_dim, cond->b_ada, cond->mod_buf, cond->n_mod, 0, LDT_ACT_NONE,
                        LDT_ACT_NONE, p->batch, cond->n_mod, cond->t_dim};
            TRY(ldt_sgemm_launch(&g, s));
        }
    }
    TRY(score_forward_impl(p, st.x, st.eps_tmp, st.cond ? nullptr : st.step_counter, s, nullptr));
    const long n = (long)p->batch * p->tokens * p->z_dim;
    StepArgs a{st.x, st.eps_tmp, st.noise, st.x, st.x_mean, st.coef, st.step_counter, 0, st.mode, n, st.elem_offset, st.noise_step_stride,
               (uint32_t)st.seed, (uint32_t)(st.seed >> 32), 1, 0, st.x_traj};
    TRY(ldt_sampler_step_launch(&a, s));
    return ldt_advance_step_launch(st.step_counter, s);
}

static int hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) ldt_set_error("sample_loop: %s: %s", what, hipGetErrorString(e));
    return (int)e;                                              // (hipSuccess == LDT_OK == 0)
}

// What the graph path holds while it runs: the private capture stream, its fences against the caller's stream, and the captured step as
// graph + exec ([0] the plain step, [1] with the fold monitor on).  Whichever way the loop ends, in-flight launches finish before their exec goes.
struct StepGraphs {
    hipStream_t gs = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipGraph_t graph[2] = {nullptr, nullptr};
    hipGraphExec_t exec[2] = {nullptr, nullptr};
    StepGraphs() = default;
    StepGraphs(const StepGraphs&) = delete;                     // one owner
    ~StepGraphs() {
        if (gs) (void)hipStreamSynchronize(gs);
        for (hipGraphExec_t e : exec) if (e) (void)hipGraphExecDestroy(e);
        for (hipGraph_t g : graph) if (g) (void)hipGraphDestroy(g);
        for (hipEvent_t e : {ev_in, ev_out}) if (e) (void)hipEventDestroy(e);
        if (gs) (void)hipStreamDestroy(gs);
    }
};

// Capture one step on `gs`.  A capture that was begun is always ended; a failed launch inside it keeps its own message.
static int capture_step(const SampleStep& st, const ldt_score_plan* p, hipStream_t gs, hipGraph_t* graph) {
    TRY(hip_ok(hipStreamBeginCapture(gs, hipStreamCaptureModeThreadLocal), "begin capture"));
    const int rc = enqueue_step(st, p, gs);
    const hipError_t e = hipStreamEndCapture(gs, graph);
    return rc != LDT_OK ? rc : hip_ok(e, "end capture");
}

extern "C" int ldt_sample_loop(const ldt_score_plan* p, float* x, float* x_mean, float* eps_tmp, const float* coef,
                               int32_t mode, const float* noise, int64_t noise_step_stride, int64_t elem_offset,
                               uint64_t seed, int32_t* step_counter, int32_t n_steps, const ldt_cond_args* cond,
                               float* x_traj, int32_t use_graph, void* stream) {
    TRY(check_plan(p));
    LDT_REQUIRE(x && x_mean && eps_tmp && coef && step_counter && n_steps > 0, LDT_EARG, "sample_loop: null pointer / n_steps");
    LDT_REQUIRE(!cond || !cond->w_ada_bf16 == !cond->c_buf_bf16, LDT_EARG, "sample_loop: w_ada_bf16 and c_buf_bf16 go together");
    LDT_REQUIRE(!cond || (cond->temb && (cond->w_ada || cond->w_ada_bf16) && cond->b_ada && cond->c_buf && cond->mod_buf && cond->mod_buf == p->mod &&
                          p->mod_sample_stride == cond->n_mod && cond->t_dim > 0), LDT_EARG,
                "sample_loop: inconsistent conditioning block (plan->mod must be cond->mod_buf with sample stride n_mod)");
    hipStream_t s = ldt_stream(stream);
    const SampleStep st{x, x_mean, eps_tmp, x_traj, coef, noise, noise_step_stride, elem_offset, seed, mode, step_counter, cond};
    TRY(hip_ok(hipMemsetAsync(step_counter, 0, sizeof(int), s), "memset"));
    // LN-fold monitor inside the loop (plan->fold_monitor, every plan->fold_monitor_every steps and on the last one): the other steps run a
    // copy of the plan without it
    ldt_score_plan plain = *p;
    plain.fold_monitor = nullptr;
    const bool mon = p->fold_monitor != nullptr;
    const int every = p->fold_monitor_every > 0 ? p->fold_monitor_every : 1;
    auto monitored = [&](int i) { return mon && (i % every == 0 || i == n_steps - 1); };
    if (!use_graph) {
        for (int i = 0; i < n_steps; ++i) TRY(enqueue_step(st, monitored(i) ? p : &plain, s));
        return LDT_OK;
    }
    // One step captured, replayed n_steps times.  Capture runs on a private non-blocking stream (the caller's may be the legacy default
    // stream, which cannot be captured), fenced against the caller's stream with events on both sides.
    StepGraphs g;
    TRY(hip_ok(hipStreamCreateWithFlags(&g.gs, hipStreamNonBlocking), "stream create"));
    TRY(hip_ok(hipEventCreateWithFlags(&g.ev_in, hipEventDisableTiming), "event create"));
    TRY(hip_ok(hipEventCreateWithFlags(&g.ev_out, hipEventDisableTiming), "event create"));
    TRY(hip_ok(hipEventRecord(g.ev_in, s), "event record"));
    TRY(hip_ok(hipStreamWaitEvent(g.gs, g.ev_in, 0), "stream wait"));
    TRY(capture_step(st, &plain, g.gs, &g.graph[0]));
    if (mon) TRY(capture_step(st, p, g.gs, &g.graph[1]));
    for (int k = 0; k < (mon ? 2 : 1); ++k) TRY(hip_ok(hipGraphInstantiate(&g.exec[k], g.graph[k], nullptr, nullptr, 0), "graph instantiate"));
    for (int i = 0; i < n_steps; ++i) TRY(hip_ok(hipGraphLaunch(g.exec[monitored(i) ? 1 : 0], g.gs), "graph launch"));
    TRY(hip_ok(hipEventRecord(g.ev_out, g.gs), "event record"));
    return hip_ok(hipStreamWaitEvent(s, g.ev_out, 0), "stream wait");
}
