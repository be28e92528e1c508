// Internal argument blocks, host helpers and the launcher prototypes that a second caller inside the library needs (the Score forward and
// the sampling loop of api.hip, the GEMM and attention families among themselves).  An op with one caller has no launcher: its extern "C"
// entry (include/ldt_hip.h) checks, sizes the grid and launches in the file of its kernel.
#pragma once
#include "common.h"

enum { EPI_F32 = 0, EPI_BF16 = 1, EPI_GELU_BF16 = 2, EPI_RELU_BF16 = 3, EPI_RESID_F32 = 4 };
#define LDT_NUM_CUS 256      // MI355X
// workgroups a launch may fill: every CU, or GemmArgs::max_wgs of them (a sub-batch stream's share)
static inline int ldt_wg_limit(int max_wgs) { return (max_wgs > 0 && max_wgs < LDT_NUM_CUS) ? max_wgs : LDT_NUM_CUS; }
// THE fill rule: a persistent kernel is worth it when its tiles fill at least 5/8 of those workgroups (each caller counts its own tiles)
static inline bool ldt_fills_workgroups(long tiles, int max_wgs) { return tiles * 8 >= (long)ldt_wg_limit(max_wgs) * 5; }
// the C-ABI's opaque handles as the types the launches use: the stream, bf16 rows passed as uint16_t* / void*
static inline hipStream_t ldt_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline const bf16_t* ldt_bf16(const void* p) { return reinterpret_cast<const bf16_t*>(p); }
static inline bf16_t* ldt_bf16_mut(void* p) { return reinterpret_cast<bf16_t*>(p); }
// THE grid rule of a grid-stride launch: one workgroup per `per_block` items, at most `cap` of them (each kernel states its own cap)
static inline unsigned ldt_grid_1d(long items, int per_block, long cap) {
    const long blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < cap ? blocks : cap);
}

struct GemmArgs {
    const bf16_t* X; long ldx;
    const bf16_t* W; long ldw;
    const float* bias;
    void* out; long ldo;
    const float* resid; long ldr;       // EPI_RESID_F32 (may alias out)
    const bf16_t* skip; long lds_;      // EPI_RELU_BF16 optional skip
    const float* gate;                  // [samples or 1][gate_sample_stride] fp32, nullable
    long gate_sample_stride;            // 0 = one gate vector shared by every row
    int rows_per_sample;
    const int* step_ptr; long gate_step_stride;   // gate += *step_ptr * gate_step_stride (device-side step counter)
    int M, N, K;
    // ---- LayerNorm folding (256-tile kernel, interior tiles only; gemm256_tile.h "LN folding") ----
    // producer (EPI_RESID_F32): second output xs[m][n] = bf16(out[m][n] * (1 + ln_scale[n])) and per-row partial
    // (sum, sum of squares) of out over each 256-column tile: stats_out[(n/256)][M][2]
    bf16_t* xs; long ldxs; const float* ln_scale; long ln_step_stride; float* stats_out;
    // consumer (EPI_BF16 / EPI_GELU_BF16): X is the producer's xs; out = epi( rstd*acc - rstd*mean*fold_S[n] + fold_C[n] )
    // with (mean, rstd) of each row from stats_in[stats_parts][M][2] over the K input channels
    const float* stats_in; int stats_parts; const float* fold_S; const float* fold_C; long fold_step_stride;
    int group_m;                        // 256-tile kernel: row panels per group of the tile order (set by the launcher)
    int dbg;                            // tools/dbg only (LDT_DBG_EPI bits: 1 no residual read, 2 no fp32 store, 4 no xs store, 8 no statistics)
    int max_wgs;                        // 256-tile kernel: cap on the persistent grid (0 = one workgroup per CU); sub-batch streams use 128
    int col_major;                      // v1 kernel only: tile order (GemmRoute::col_major, copied by the launcher; see gemm_bf16_nt_kernel)
    // ---- QKV projection + self-attention in one launch (gemm_mid.hip, 32-token samples, head dim 64): N = 3 * hidden columns [q | k | v];
    // the kernel writes O[B][H][32][64] (the reference's raw (B,N,C) buffer, model/layers.py:190-197) to attn_o and NOT the q | k | v rows
    bf16_t* attn_o; float attn_scale_log2e;
    // fused q projection + cross-attention (gemm_mid.hip, ldt_gemm_mid_q_xattn_try): the condition's cached K | V rows (elements)
    const bf16_t* attn_k; const bf16_t* attn_v; long attn_ldkv; long attn_kv_batch_stride;
};

struct LnArgs {
    const float* x; long ldx;
    bf16_t* y; long ldy;
    const float* w; const float* b;              // affine (decoder blocks), nullable
    const float* shift; const float* scale;      // nullable (no modulation)
    long mod_sample_stride; int rows_per_sample;
    const int* step_ptr; long mod_step_stride;
    long M; int C;
};

struct AttnArgs {
    const bf16_t* Q; long ldq; long q_batch_stride;     // Q[b][n][h*Dh + d]
    const bf16_t* K; long ldk; long kv_batch_stride;    // K[b][m][h*Dh + d]
    const bf16_t* V; long ldv;                          // V[b][m][h*Dh + d] (same batch stride as K)
    bf16_t* O;                                          // [B][H][Nq][Dh]
    int B, H, Nq, Nk;
    float scale_log2e;                                  // Dh^-0.5 * log2(e)
    // fused output projection (narrow blocks, Dh = 32, C = H*Dh in {64,128}):  X += gate * (Wo . O' + bo), O' = the
    // [B][H][Nq][Dh] result re-read as (B*Nq, C) rows (quirk Q1); all null/0 for the plain kernel
    const bf16_t* Wo; const float* bo; float* X; long ldx; const float* gate; long gate_sample_stride;
};

struct StepArgs {
    const float* x; const float* params; const float* noise;
    float* x_out; float* x_mean_out;
    const float* coef; const int* step_ptr; int step_host; int mode;
    long n; long elem_offset; long noise_step_stride;
    uint32_t seed_lo, seed_hi;
    int philox_mul, philox_add;          // Philox stream id of this draw = step * philox_mul + philox_add
    float* traj;                         // optional [n_steps][n]: x after this step is also stored at traj + step*n (parity curves)
};

struct SgemmArgs {
    const float* A; long lda; const float* B; long ldb; const float* bias;
    void* C; long ldc; int out_bf16; int act_in; int act_out;
    int M, N, K;
};
// element `at` of SgemmArgs::C, fp32 or bf16 by out_bf16 (the three tiled kernels and the small-N form; the small-K form stores vectors).
// A macro: as an inline function the same lines compile to other code in those kernels (profiles/small_kernels_refactor_codegen.txt).
#define SGEMM_STORE(a, at, val)                                                  \
    do {                                                                         \
        const float _v = (val);                                                  \
        if ((a).out_bf16) reinterpret_cast<bf16_t*>((a).C)[at] = (bf16_t)_v;     \
        else reinterpret_cast<float*>((a).C)[at] = _v;                           \
    } while (0)

int ldt_gemm_launch(int epi, const GemmArgs* a, hipStream_t stream);
// Which kernel a GEMM runs on: THE dispatch rule.  ldt_gemm_launch, ldt_gemm_lnfold_launch and the ldt_gemm_route query (include/ldt_hip.h)
// all call ldt_gemm_decide and nothing else chooses a family, a tile, a grid or the v1 kernel's tile order; the launchers check the operands
// and launch the route they are given.  granule: 0 = plain GEMM; 256 / 32 = LN-folded form with
// statistics per that many columns (producer when epi == EPI_RESID_F32, consumer otherwise).  Reads M, N, K, ldo, ldr, skip / lds_, gate /
// gate_sample_stride and max_wgs of `a`, no pointer's target.  family GEMM_ROUTE_NONE: no kernel takes the problem (the launchers report why).
enum { GEMM_ROUTE_NONE = 0, GEMM_ROUTE_256_ONE = 1, GEMM_ROUTE_256_MULTI = 2, GEMM_ROUTE_MID = 3, GEMM_ROUTE_V1 = 4 };
struct GemmRoute {
    int family, bm, bn;
    int tiles_per_wg;                   // most tiles one workgroup computes (> 1: the persistent 256-tile kernel only; Tile256List::max_count)
    int grid;                           // workgroups launched
    int v1_form;                        // GEMM_ROUTE_V1: row of the v1 kernel's table of forms (0 128 x 128 x 2 stages, 1 128 x 64 x 2, 2 64 x 64 x 3)
    int col_major;                      // GEMM_ROUTE_V1: column-major tile order (wide outputs over few row tiles), for GemmArgs::col_major
};
GemmRoute ldt_gemm_decide(int epi, const GemmArgs* a, int granule);
// gemm_mid.hip, the mid-size tile kernels.  fold: 0 plain, 1 LN-folded producer, 2 consumer (statistics per 32 columns; gemm256_tile.h's FOLD_*)
bool ldt_gemm_mid_route(int epi, int fold, const GemmArgs* a, GemmRoute* r);   // true + `r` filled (family GEMM_ROUTE_MID, tile, grid) when a form takes the problem
int ldt_gemm_mid_launch(int epi, int fold, const GemmArgs* a, const GemmRoute& route, hipStream_t stream);   // route: ldt_gemm_decide's
bool ldt_gemm_mid_lnfold_takes(int epi, int M, int N, int K);       // would the LN-folded form (statistics per 32 columns) of this GEMM be taken?
bool ldt_gemm_mid_qkv_attn_try(const GemmArgs* a, int tokens, int head_dim, bool folded, hipStream_t stream, int* status);
bool ldt_gemm_qkv_attn256_try(const GemmArgs* a, int tokens, int head_dim, bool folded, hipStream_t stream, int* status);   // gemm_256.hip: fused QKV + self-attention at 256 tokens, Dh 64; false = not taken
bool ldt_gemm_mid_q_xattn_try(const GemmArgs* a, int tokens, int cond_tokens, int head_dim, hipStream_t stream, int* status);   // fused q projection + cross-attention (32 x 32 tokens, Dh 64); false = not taken
// the shape part of the three rules above (M, N, K, stats_parts and max_wgs of `a` plus the environment switches; no pointer is read): each
// `_try` starts with its own and then checks pointers and alignment; ldt_qkv_attention_route (include/ldt_hip.h) evaluates them in the forward's order
bool ldt_gemm_mid_qkv_attn_takes(const GemmArgs* a, int tokens, int head_dim, bool folded);
bool ldt_gemm_qkv_attn256_takes(const GemmArgs* a, int tokens, int head_dim, bool folded);
bool ldt_gemm_mid_q_xattn_takes(const GemmArgs* a, int tokens, int cond_tokens, int head_dim);
// Whether and how a Score block (M rows, D channels, MLP width F) folds its LayerNorms into its GEMMs: THE fold decision (gemm_bf16.hip).
// ldt_score_lnfold_route (include/ldt_hip.h) returns `route`; the forward folds a plan that brings the fold tables when the route is the
// mid-size one or shape_256 holds (the forced fold below the fill rule), with plan->stats laid out as [D / granule][M][2].
enum { SCORE_FOLD_NONE = 0, SCORE_FOLD_256 = 1, SCORE_FOLD_MID = 2 };   // 256-tile kernels that fill the workgroups / small batch: every GEMM of the block runs a mid-size tile form
struct ScoreFold { int route; bool shape_256; int granule; };           // shape_256: the 256-tile kernels take the shape, filling or not; granule: columns per statistics part (32 mid, else 256)
ScoreFold ldt_score_fold_decide(int M, int D, int F, int max_wgs);
int ldt_gemm_lnfold_launch(int epi, const GemmArgs* a, hipStream_t stream);   // producer (RESID + xs/stats) or consumer (stats_in)
int ldt_ln_launch(const LnArgs* a, hipStream_t s);
int ldt_attn_launch(const AttnArgs* a, int dh, hipStream_t s);
int ldt_attn_route(int B, int H, int Nq, int Nk, int dh);       // 0 streaming, 1 resident, 2 whole-head (attention.hip), 3 narrow heads (attention_narrow.hip)
int ldt_attn_narrow_launch(const AttnArgs* a, int dh, hipStream_t s);   // head dim 8 or 16; ldt_attn_launch has checked the operands
int ldt_attn_oproj_launch(const AttnArgs* a, int dh, hipStream_t s);
// Sum of v[0..N) over the lanes lr and lr ^ M, split between them: the lane with bit M keeps the upper half of v.  Four of these (M = 8, 4, 2,
// 1) sum a per-lane array over the 16 lanes of an MFMA row group in a fixed order and leave each lane N / 16 adjacent elements (narrow heads).
template <int N, int M>
__device__ __forceinline__ void narrow_halve(float* v, int lr) {
    const bool up = (lr & M) != 0;
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
        const float keep = up ? v[k + N / 2] : v[k];
        const float send = up ? v[k] : v[k + N / 2];
        v[k] = keep + __shfl_xor(send, M, 64);
    }
}
int ldt_cast_pad_launch(const float* src, long lds, bf16_t* dst, long ldd, long rows, int cols, int cols_pad, hipStream_t s);
int ldt_sampler_step_launch(const StepArgs* a, hipStream_t s);
int ldt_advance_step_launch(int* step_ptr, hipStream_t s);
int ldt_sgemm_launch(const SgemmArgs* a, hipStream_t s);
// Which of its seven kernel forms the fp32 linear runs on: THE dispatch rule (sgemm.hip).  ldt_sgemm_launch and the ldt_sgemm_route
// query (include/ldt_hip.h, which states the rule) call it and nothing else chooses a form.  misaligned: bit 0 A, 1 B, 2 C, 3 bias not
// 16-byte aligned.  Reads the LDT_SGEMM_VALU / LDT_SGEMM_SKINNY switches once per process; touches no device and no pointer's target.
enum { SGEMM_ROUTE_NONE = 0, SGEMM_ROUTE_NT = 1, SGEMM_ROUTE_MFMA_128 = 2, SGEMM_ROUTE_MFMA_32 = 3, SGEMM_ROUTE_SMALLN_4 = 4,
       SGEMM_ROUTE_SMALLN_8 = 5, SGEMM_ROUTE_SMALLK_4 = 6, SGEMM_ROUTE_SMALLK_8 = 7 };
int ldt_sgemm_decide(int M, int N, int K, long lda, long ldb, long ldc, int misaligned);
int ldt_sgemm_mfma_launch(const SgemmArgs* a, int route, hipStream_t s);      // sgemm_mfma.hip: SGEMM_ROUTE_MFMA_128 / _32 (grid and launch)
int ldt_skinny_linear_launch(const SgemmArgs* a, int route, hipStream_t s);   // skinny_linear.hip: SGEMM_ROUTE_SMALLN_* / SMALLK_* (grid sized to the device, launch)

int ldt_fps_wave_launch(const float* xyz, int B, int n, int m, int skip_near_origin, int* idx, hipStream_t s);   // fps_wave.hip (ldt_fps of pointops.hip routes to it)
// per-sample sums of the 'anchor' grouping (pointops.hip): ldt_group_normalize and ldt_grouper_mlp (grouper_mlp.hip) both start with it
int ldt_group_stats_launch(const float* feat, const float* xyz, const int* fps_idx, const int* knn_idx, double* stats,
                           int B, int n, int S, int k, int D, hipStream_t s);
int ldt_fold_monitor_launch(const float* stats, int parts, long M, int K, float* out, hipStream_t s);   // elementwise.hip
int ldt_cond_rows_launch(const float* temb, const float* extra, float* c, void* c_bf16, const int* step_ptr, int batch, int t_dim, int silu_out, hipStream_t s);
