// Attention backward of a Score block (model/layers.py:183-200), head dim 8, 16, 32 or 64, Nq, Nk <= 512, gfx950: the whole of it — both
// kernel forms, their launchers and the four entry points.  Self-attention (ldt_attention_bwd at 64, ldt_attention_bwd_narrow at 8, 16 and
// 32) runs it at Nq = Nk = N; the Compressor's decoder (ldt_attention_bwd_long: head dim 32, up to 8192 queries on up to 512 keys) sums
// dK / dV in parts, see "long query axis" below; its posterior blocks (ldt_attention_bwd_wide: up to 512 queries on up to 8192 keys) take the
// row statistics and dQ in parts, see "long key axis"; cross-attention to the point condition (ldt_attention_bwd_cross, every width; model/scorenet/score.py:129-149:
// the even blocks of a conditioned Score) with Nk keys from another tensor: query blocks tile Nq and loop to Nk, key blocks tile Nk and loop
// to Nq, and every clamp and guard takes the extent of the axis it indexes.
//   forward:   S = Q K^T / sqrt(Dh),  P = softmax(S),  O = P V          (O is the [B][H][N][Dh] buffer the reference re-reads as (B N, C): quirk Q1;
//                                                                       its gradient dO arrives in the same raw layout — nothing is permuted)
//   backward:  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - D),  D = rowsum(dO o O),  dQ = dS K / sqrt(Dh),  dK = dS^T Q / sqrt(Dh)
// The forward kernels write no log-sum-exp, so each query row's maximum and sum are recomputed (kept as L = max + ln(sum), so that
// P = exp(S - L)) together with D, and go to `stats`.  Then dQ is produced per block of 16 query rows looping over the keys, and dK / dV per
// block of 16 keys looping over the queries: every output element is summed inside one wave in a fixed order — no atomics, no sum across
// workgroups, the same bits on every run.  Rows and columns past the end re-read the last row (never out of bounds) and get weight exactly 0.
//
// Both forms take the same steps up to dS, each written once below: the role table, the clamped fragment load, the first product of one
// 16-column tile (S and dP, or their transposes in a key block: one v_mfma_f32_16x16x32_bf16 per 32 channels, fp32 accumulation, operand
// fragments straight from global rows — lane l: row l & 15, 8 contiguous head channels at 8 (l >> 4), a zero fragment past Dh below 32), the
// row-statistics sweep, D, and the P / dS element step.  They differ in the second products, which stay two bodies because they are two
// algorithms:
//   MFMA form (32, 64)   one wave per workgroup, three launches (statistics; dQ; dK and dV).  P and dS are rounded to bf16 and cross one LDS
//                        tile to become the A operand of DH / 16 MFMAs per 32 columns.
//   narrow form (8, 16)  as the forward's (attention_narrow.hip): one wave per (sample, head, block of 16 rows), four such waves per
//                        workgroup, nothing shared between them: no LDS, no barrier; two launches (statistics with dQ; dK and dV).  The
//                        lane holds P and dS of ONE column for four rows, and that column's K (Q, dO) slice is one or two 16-byte loads
//                        in its natural layout: 4 x Dh fused multiply-adds per product into per-lane partial sums, so P and dS STAY fp32
//                        (they never become MFMA operands: the 2^-8 terms of the 32 / 64-wide bound are absent).  narrow_halve x 4 then
//                        sums the partials over the 16 lanes of an lq in a fixed order and leaves each lane Dh / 4 adjacent channels of one
//                        row: times the scale (dQ, dK), one 4- or 8-byte store.
// Also left in its two places: where a query block's own L and D come from (the MFMA form reads them from `stats`, the narrow form has just
// computed them in registers) — one line each, and sharing it would need a switch that says which form is calling.
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define AB_T 16                      // rows (query blocks: queries, key blocks: keys) per wave
#define AB_J 32                      // MFMA form: columns per loop iteration, the K extent of one 16x16x32 product
#define AB_LDP (AB_J + 8)            // MFMA form: LDS row pitch of the P / dS tiles, bf16 elements (80 B: 16-B aligned rows, staggered banks)
#ifndef AB_CHUNK                     // (a measurement build of this file alone may pass another multiple of 32: tools/bench_decoder_train.py)
#define AB_CHUNK LDT_ATTN_BWD_LONG_CHUNK   // long query axis: queries per partial sum of dK / dV.  A source constant: never a function of the grid or the device
#endif
#ifndef AB_WIDE_CHUNK                // (likewise: tools/bench_topdown_train.py)
#define AB_WIDE_CHUNK LDT_ATTN_BWD_WIDE_CHUNK   // long key axis: keys per partial of the row statistics and of dQ.  A source constant, as AB_CHUNK is
#endif
static_assert(AB_CHUNK % AB_J == 0 && AB_WIDE_CHUNK % AB_J == 0, "a 32-column step never straddles two chunks");

// the operands of the entry points (include/ldt_hip.h); self-attention: Nq = Nk = N
struct AttnBwdArgs {
    const bf16_t* Q; long ldq; long q_bs;
    const bf16_t* K; long ldk; const bf16_t* V; long ldv; long kv_bs;
    const bf16_t* O; const bf16_t* dO;        // [B][H][Nq][Dh]
    float* stats;                             // [B][H][Nq][2] = (L, D)
    bf16_t* dQ; long lddq; long dq_bs;
    bf16_t* dK; long lddk; bf16_t* dV; long lddv; long dkv_bs;
    int B, H, Nq, Nk;                         // queries (rows of Q, O, dO, dQ, stats) and keys (rows of K, V, dK, dV) per sample
    float scale;                              // Dh^-0.5
    float* part;                              // long query axis: fp32 partials [chunk][B][Nk][2 H Dh] = dK (unscaled) | dV; long key axis: [chunk][B][Nq][H Dh] = dQ (unscaled)
    float* cstat;                             // long key axis only: [chunk][B][H][Nq][2] = each query row's maximum and sum of exp(s - maximum) over the chunk's keys
};

// ---- the steps both forms take
constexpr int ab_steps(int dh) { return dh >= 32 ? dh / 32 : 1; }       // MFMAs (32 channels each) of one first product

// One (sample, head) in the roles of a block.
// KV = false: the block's 16 rows are queries, the loop runs over keys:    S = Q K^T,   dP = dO V^T,   dQ  = scale dS K
// KV = true:  the block's 16 rows are keys,    the loop runs over queries: S^T = K Q^T, dP^T = V dO^T, dK = scale dS^T Q,  dV = P^T dO
// In both the accumulator tile of a first product puts the block's rows at 4 (l >> 4) + i and the loop's column at l & 15.
struct AttnBwdRoles {
    const bf16_t *rowA, *rowB, *colA, *colB;                            // the block's rows (A operands of the first products), the loop's columns
    long ld_rowA, ld_rowB, ld_colA, ld_colB;
    int NR, NC;                                                         // extents of the block's row axis and of the loop's column axis
    long ob;                                                            // first row of this head in O, dO and stats
    float* st;                                                          // (L, D) of this head's query rows
};
template <int DH, bool KV>
__device__ __forceinline__ AttnBwdRoles attn_bwd_roles(const AttnBwdArgs& a, int b, int h) {
    const long ob = ((long)b * a.H + h) * a.Nq;
    const bf16_t* Qb = a.Q + (long)b * a.q_bs + h * DH;
    const bf16_t* Kb = a.K + (long)b * a.kv_bs + h * DH;
    const bf16_t* Vb = a.V + (long)b * a.kv_bs + h * DH;
    const bf16_t* Gb = a.dO + ob * DH;
    return {KV ? Kb : Qb, KV ? Vb : Gb, KV ? Qb : Kb, KV ? Gb : Vb, KV ? a.ldk : a.ldq, KV ? a.ldv : (long)DH, KV ? a.ldq : a.ldk,
            KV ? (long)DH : a.ldv, KV ? a.Nk : a.Nq, KV ? a.Nq : a.Nk, ob, a.stats + ob * 2};
}

// This lane's fragment of step s of a row's first product: channels 32 s + 8 lq .. + 7, a zero fragment past Dh (Dh 8, 16).  Rows past the
// end repeat the last one: finite values that a zero weight removes.
template <int DH>
__device__ __forceinline__ bf16x8 ld_frag(const bf16_t* base, long ld, int row, int nrows, int s, int lq) {
    const bf16_t* p = base + (long)(row < nrows ? row : nrows - 1) * ld;
    if constexpr (DH >= 32) {
        return *reinterpret_cast<const bf16x8*>(p + (4 * s + lq) * 8);
    } else {
        const bf16x8 t = *reinterpret_cast<const bf16x8*>(p + 8 * (lq & (DH / 8 - 1))), zero = {0, 0, 0, 0, 0, 0, 0, 0};
        return lq < DH / 8 ? t : zero;
    }
}

// First product of one 16-column tile: [the 16 rows whose fragments are `a`] x [row `row` of base]^T -> element [4 lq + i][this lane's column]
template <int DH>
__device__ __forceinline__ f32x4 tile_qk(const bf16x8 (&a)[ab_steps(DH)], const bf16_t* base, long ld, int row, int nrows, int lq) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < ab_steps(DH); ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], ld_frag<DH>(base, ld, row, nrows, s, lq), acc, 0, 0, 0);
    return acc;
}

// mx = max_j s_j and sm = sum_j exp(s_j - mx) over the keys jb <= j < je (je <= Nk), s = scale * q . k_j, of the query rows 4 lq + i whose
// fragments are `qf`: two sweeps over the keys (the maximum, then the sum), each reduced over the 16 lanes of an lq.  Every lane of an lq ends
// with the same values.  L = mx + ln sm (so that P = exp(S - L)) when the sweep took every key.
template <int DH>
__device__ __forceinline__ void row_max_sum(const bf16x8 (&qf)[ab_steps(DH)], const bf16_t* Kb, long ldk, int jb, int je, int Nk, float scale, int lr,
                                            int lq, float (&mx)[4], float (&sm)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { mx[i] = -INFINITY; sm[i] = 0.f; }
    for (int j0 = jb; j0 < je; j0 += 16) {
        const f32x4 sc = tile_qk<DH>(qf, Kb, ldk, j0 + lr, Nk, lq);
        if (j0 + lr < je) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mx[i] = fmaxf(mx[i], sc[i] * scale);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], o, 64));
    for (int j0 = jb; j0 < je; j0 += 16) {
        const f32x4 sc = tile_qk<DH>(qf, Kb, ldk, j0 + lr, Nk, lq);
        if (j0 + lr < je) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sm[i] += expf(sc[i] * scale - mx[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sm[i] += __shfl_xor(sm[i], o, 64);
}
template <int DH>
__device__ __forceinline__ void row_lse(const bf16x8 (&qf)[ab_steps(DH)], const bf16_t* Kb, long ldk, int Nk, float scale, int lr, int lq, float (&L)[4]) {
    float mx[4], sm[4];
    row_max_sum<DH>(qf, Kb, ldk, 0, Nk, Nk, scale, lr, lq, mx, sm);
#pragma unroll
    for (int i = 0; i < 4; ++i) L[i] = mx[i] + logf(sm[i]);
}

// D = sum_d dO o O of query row `row`, whose dO fragments are `g`: lane (lr, lq) sums its channels (8 lq .. + 7 of every 32; a zero fragment
// past Dh), then the four lq: the same bits in all four.
template <int DH>
__device__ __forceinline__ float row_d(const bf16_t* O, int row, int nrows, const bf16x8 (&g)[ab_steps(DH)], int lq) {
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < ab_steps(DH); ++s) {
        const bf16x8 o8 = ld_frag<DH>(O, DH, row, nrows, s, lq);
#pragma unroll
        for (int j = 0; j < 8; ++j) d += (float)o8[j] * (float)g[s][j];
    }
    d += __shfl_xor(d, 16, 64);
    return d + __shfl_xor(d, 32, 64);
}

// P = exp(S scale - L) and dS = P (dP - D) of this lane's four elements [row row0 + i][column col], fp32; exactly 0 past either end.  L and D
// belong to the query: the row's (query blocks: Lr, Dr) or the column's (key blocks: read from st).
template <bool KV>
__device__ __forceinline__ void p_ds(const f32x4& sc, const f32x4& dp, float scale, const AttnBwdRoles& r, int row0, int col, const float (&Lr)[4],
                                     const float (&Dr)[4], float (&p)[4], float (&ds)[4]) {
    float Lc = 0.f, Dc = 0.f;
    if (KV) { const int q = min(col, r.NC - 1); Lc = r.st[2 * q]; Dc = r.st[2 * q + 1]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool live = col < r.NC && row0 + i < r.NR;
        p[i] = live ? expf(sc[i] * scale - (KV ? Lc : Lr[i])) : 0.f;
        ds[i] = p[i] * (dp[i] - (KV ? Dc : Dr[i]));
    }
}

// ---- MFMA form, head dim 32 or 64.  Per query row: L and D to `stats`.  WIDE (long key axis): L from the chunks' (maximum, sum) pairs that
// attn_bwd_chunk_stats_kernel left in a.cstat, combined in chunk order: M = max_c m_c, L = M + ln sum_c s_c exp(m_c - M)
template <int DH, bool WIDE = false>
__global__ __launch_bounds__(64) void attn_bwd_stats_kernel(const AttnBwdArgs a, int chunks) {
    constexpr int NS = ab_steps(DH);
    const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4, q0 = blockIdx.x * AB_T;
    const AttnBwdRoles r = attn_bwd_roles<DH, false>(a, blockIdx.z, blockIdx.y);
    bf16x8 qf[NS], gf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = ld_frag<DH>(r.rowA, r.ld_rowA, q0 + lr, r.NR, s, lq);
    float L[4];                                                         // of query rows q0 + 4 lq + i
    if constexpr (WIDE) {
        const long cs = (long)a.B * a.H * a.Nq * 2;                     // floats of one chunk's table
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float* c = a.cstat + (r.ob + min(q0 + 4 * lq + i, r.NR - 1)) * 2;
            float M = -INFINITY, s = 0.f;
            for (int k = 0; k < chunks; ++k) M = fmaxf(M, c[k * cs]);
            for (int k = 0; k < chunks; ++k) s = fmaf(c[k * cs + 1], expf(c[k * cs] - M), s);      // one chunk: s_0 * exp(0) + 0 = s_0, the bits of row_lse
            L[i] = M + logf(s);
        }
    } else {
        row_lse<DH>(qf, r.colA, r.ld_colA, r.NC, a.scale, lr, lq, L);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) gf[s] = ld_frag<DH>(r.rowB, r.ld_rowB, q0 + lr, r.NR, s, lq);
    const float d = row_d<DH>(a.O + r.ob * DH, q0 + lr, r.NR, gf, lq);  // of query row q0 + lr
    if (lr == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + 4 * lq + i;
            if (q < r.NR) r.st[2 * q] = L[i];
        }
    }
    if (lq == 0 && q0 + lr < r.NR) r.st[2 * (q0 + lr) + 1] = d;
}

// long key axis: the maximum and the sum of one chunk of AB_WIDE_CHUNK keys, per (16 queries, chunk): blockIdx.x = chunk * query blocks + query block
template <int DH>
__global__ __launch_bounds__(64) void attn_bwd_chunk_stats_kernel(const AttnBwdArgs a) {
    constexpr int NS = ab_steps(DH);
    const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4, nqb = (a.Nq + AB_T - 1) / AB_T;
    const int chunk = blockIdx.x / nqb, q0 = (blockIdx.x % nqb) * AB_T;
    const AttnBwdRoles r = attn_bwd_roles<DH, false>(a, blockIdx.z, blockIdx.y);
    bf16x8 qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = ld_frag<DH>(r.rowA, r.ld_rowA, q0 + lr, r.NR, s, lq);
    float mx[4], sm[4];
    row_max_sum<DH>(qf, r.colA, r.ld_colA, chunk * AB_WIDE_CHUNK, min((chunk + 1) * AB_WIDE_CHUNK, r.NC), r.NC, a.scale, lr, lq, mx, sm);
    float* o = a.cstat + ((long)chunk * a.B * a.H * a.Nq + r.ob) * 2;
    if (lr == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + 4 * lq + i;
            if (q < r.NR) { o[2 * q] = mx[i]; o[2 * q + 1] = sm[i]; }
        }
    }
}

// the main kernels of the MFMA form share one body.  PART: blockIdx.x = chunk * row blocks + row block; the loop runs over the chunk's columns
// alone (key blocks of a long query axis: AB_CHUNK queries; query blocks of a long key axis: AB_WIDE_CHUNK keys) and the fp32 sums go to
// a.part unscaled, for attn_bwd_parts_kernel to add in chunk order
template <int DH, bool KV, bool PART = false>
__global__ __launch_bounds__(64) void attn_bwd_kernel(const AttnBwdArgs a) {
    constexpr int CH = KV ? AB_CHUNK : AB_WIDE_CHUNK;
    constexpr int NS = ab_steps(DH), NT = DH / 16;                      // operand chunks of 32 channels, accumulator tiles of 16
    __shared__ __attribute__((aligned(16))) bf16_t ds_t[AB_T][AB_LDP];
    __shared__ __attribute__((aligned(16))) bf16_t p_t[AB_T][AB_LDP];
    const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4;
    const int nrb = PART ? ((KV ? a.Nk : a.Nq) + AB_T - 1) / AB_T : 1, chunk = PART ? blockIdx.x / nrb : 0;
    const int b = blockIdx.z, h = blockIdx.y, r0 = (PART ? blockIdx.x % nrb : blockIdx.x) * AB_T;
    const AttnBwdRoles r = attn_bwd_roles<DH, KV>(a, b, h);
    const int jb = chunk * CH, je = PART ? min(jb + CH, r.NC) : r.NC;                  // the loop's columns
    bf16x8 fa[NS], fb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        fa[s] = ld_frag<DH>(r.rowA, r.ld_rowA, r0 + lr, r.NR, s, lq);
        fb[s] = ld_frag<DH>(r.rowB, r.ld_rowB, r0 + lr, r.NR, s, lq);
    }
    float Lr[4] = {0.f, 0.f, 0.f, 0.f}, Dr[4] = {0.f, 0.f, 0.f, 0.f};   // query blocks: the statistics of rows 4 lq + i
    if (!KV) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = min(r0 + 4 * lq + i, r.NR - 1);
            Lr[i] = r.st[2 * q]; Dr[i] = r.st[2 * q + 1];
        }
    }
    f32x4 acc1[NT], acc2[NT];           // [16 rows][DH channels] as 16-column tiles: dQ | dK, and dV
#pragma unroll
    for (int t = 0; t < NT; ++t) { acc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc2[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    for (int j0 = jb; j0 < je; j0 += AB_J) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int col = j0 + 16 * half + lr;                       // this lane's column of the tile: a key (KV false) or a query (KV true)
            const f32x4 sc = tile_qk<DH>(fa, r.colA, r.ld_colA, col, r.NC, lq);
            const f32x4 dp = tile_qk<DH>(fb, r.colB, r.ld_colB, col, r.NC, lq);
            float p[4], ds[4];
            p_ds<KV>(sc, dp, a.scale, r, r0 + 4 * lq, col, Lr, Dr, p, ds);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ds_t[4 * lq + i][16 * half + lr] = (bf16_t)ds[i];      // P and dS are rounded to bf16 here, before the second products
                if (KV) p_t[4 * lq + i][16 * half + lr] = (bf16_t)p[i];
            }
        }
        __syncthreads();
        const bf16x8 dsf = *reinterpret_cast<const bf16x8*>(&ds_t[lr][8 * lq]);       // A: [row lr][columns j0 + 8 lq .. + 7]
        bf16x8 pf = dsf;
        if (KV) pf = *reinterpret_cast<const bf16x8*>(&p_t[lr][8 * lq]);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            bf16x8 y1, y2;                                              // B: [loop row j0 + 8 lq + e][channel 16 t + lr]
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = min(j0 + 8 * lq + e, r.NC - 1);
                y1[e] = r.colA[(long)c * r.ld_colA + 16 * t + lr];
                if (KV) y2[e] = r.colB[(long)c * r.ld_colB + 16 * t + lr];
            }
            acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, y1, acc1[t], 0, 0, 0);
            if (KV) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, y2, acc2[t], 0, 0, 0);
        }
    }
    if constexpr (PART) {
        const long W = (KV ? 2L : 1L) * a.H * DH;                      // a row of partials: dK | dV, or dQ
        float* o = a.part + ((long)chunk * a.B + b) * r.NR * W + h * DH;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = r0 + 4 * lq + i;
                if (row < r.NR) {
                    o[(long)row * W + 16 * t + lr] = acc1[t][i];
                    if (KV) o[(long)row * W + a.H * DH + 16 * t + lr] = acc2[t][i];
                }
            }
        return;
    }
    bf16_t* o1 = KV ? a.dK + (long)b * a.dkv_bs + h * DH : a.dQ + (long)b * a.dq_bs + h * DH;
    const long ld1 = KV ? a.lddk : a.lddq;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + 4 * lq + i;
            if (row < r.NR) {
                o1[(long)row * ld1 + 16 * t + lr] = (bf16_t)(acc1[t][i] * a.scale);
                if (KV) a.dV[(long)b * a.dkv_bs + h * DH + (long)row * a.lddv + 16 * t + lr] = (bf16_t)acc2[t][i];
            }
        }
}

template <int DH>
static int attn_bwd_launch(const AttnBwdArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.Nq + AB_T - 1) / AB_T), (unsigned)a.H, (unsigned)a.B), block(64);      // query blocks
    const dim3 grid_kv((unsigned)((a.Nk + AB_T - 1) / AB_T), (unsigned)a.H, (unsigned)a.B);               // key blocks
    hipLaunchKernelGGL(attn_bwd_stats_kernel<DH>, grid, block, 0, s, a, 1);
    int rc = ldt_check_launch("attention_bwd (row statistics)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_kernel<DH, false>), grid, block, 0, s, a);
    rc = ldt_check_launch("attention_bwd (dQ)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_kernel<DH, true>), grid_kv, block, 0, s, a);
    return ldt_check_launch("attention_bwd (dK, dV)");
}

// ---- long query axis (ldt_attention_bwd_long: the Compressor's decoder, 2048 queries on 32 keys), head dim 32.  Statistics and dQ are the
// kernels above: their grids tile Nq.  dK / dV as above would be one wave per 16 keys walking every query (two waves per (sample, head), 64
// trips each, at the decoder's shape): instead one wave takes (16 keys, AB_CHUNK queries) and leaves fp32 partials, and the kernel below adds
// them in chunk order, scales dK and rounds to bf16.  Still no atomics, and the order is fixed by AB_CHUNK alone: the same bits on every run
// and every device.  One thread per element of a [Nk][2 H Dh] row pair dK | dV (kv), or of a [Nq][H Dh] row of dQ (long key axis, below);
// gridDim.y = the rows per sample.
__global__ __launch_bounds__(256) void attn_bwd_parts_kernel(const AttnBwdArgs a, int dh, int chunks, bool kv) {
    const int C = a.H * dh, W = kv ? 2 * C : C, c = blockIdx.x * 256 + threadIdx.x, row = blockIdx.y, rows = gridDim.y, b = blockIdx.z;
    if (c >= W) return;
    const long chunk_stride = (long)a.B * rows * W;
    const float* p = a.part + ((long)b * rows + row) * W + c;
    float s = 0.f;
    for (int k = 0; k < chunks; ++k) s += p[k * chunk_stride];
    if (!kv) a.dQ[(long)b * a.dq_bs + (long)row * a.lddq + c] = (bf16_t)(s * a.scale);
    else if (c < C) a.dK[(long)b * a.dkv_bs + (long)row * a.lddk + c] = (bf16_t)(s * a.scale);
    else a.dV[(long)b * a.dkv_bs + (long)row * a.lddv + (c - C)] = (bf16_t)s;
}

template <int DH>
static int attn_bwd_long_launch(const AttnBwdArgs& a, hipStream_t s) {
    const int chunks = (a.Nq + AB_CHUNK - 1) / AB_CHUNK, nkb = (a.Nk + AB_T - 1) / AB_T;
    const dim3 grid((unsigned)((a.Nq + AB_T - 1) / AB_T), (unsigned)a.H, (unsigned)a.B), block(64);
    hipLaunchKernelGGL(attn_bwd_stats_kernel<DH>, grid, block, 0, s, a, 1);
    int rc = ldt_check_launch("attention_bwd_long (row statistics)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_kernel<DH, false>), grid, block, 0, s, a);
    rc = ldt_check_launch("attention_bwd_long (dQ)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_kernel<DH, true, true>), dim3((unsigned)(nkb * chunks), (unsigned)a.H, (unsigned)a.B), block, 0, s, a);
    rc = ldt_check_launch("attention_bwd_long (dK, dV partials)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL(attn_bwd_parts_kernel, dim3((unsigned)((2 * a.H * DH + 255) / 256), (unsigned)a.Nk, (unsigned)a.B), dim3(256), 0, s, a, DH, chunks, true);
    return ldt_check_launch("attention_bwd_long (dK, dV)");
}

// ---- long key axis (ldt_attention_bwd_wide: the Compressor's posterior blocks, 32 latent tokens on 2048 set points), head dim 32: the mirror
// image.  dK / dV are the key-block kernel above: its grid tiles Nk.  Row statistics and dQ as above would be one wave per 16 queries walking
// every key (two waves per (sample, head), 2 x 128 + 64 trips each, at the posterior's shape): instead one wave takes (16 queries,
// AB_WIDE_CHUNK keys).  The statistics: each chunk's maximum and sum, then combined in chunk order (attn_bwd_stats_kernel<DH, true>).  dQ:
// fp32 partials that attn_bwd_parts_kernel adds in chunk order, scales and rounds to bf16.  No atomics; the order is fixed by AB_WIDE_CHUNK.
template <int DH>
static int attn_bwd_wide_launch(const AttnBwdArgs& a, hipStream_t s) {
    const int chunks = (a.Nk + AB_WIDE_CHUNK - 1) / AB_WIDE_CHUNK, nqb = (a.Nq + AB_T - 1) / AB_T, nkb = (a.Nk + AB_T - 1) / AB_T;
    const dim3 grid((unsigned)nqb, (unsigned)a.H, (unsigned)a.B), grid_c((unsigned)(nqb * chunks), (unsigned)a.H, (unsigned)a.B), block(64);
    hipLaunchKernelGGL(attn_bwd_chunk_stats_kernel<DH>, grid_c, block, 0, s, a);
    int rc = ldt_check_launch("attention_bwd_wide (chunk statistics)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_stats_kernel<DH, true>), grid, block, 0, s, a, chunks);
    rc = ldt_check_launch("attention_bwd_wide (row statistics)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_kernel<DH, false, true>), grid_c, block, 0, s, a);
    rc = ldt_check_launch("attention_bwd_wide (dQ partials)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL(attn_bwd_parts_kernel, dim3((unsigned)((a.H * DH + 255) / 256), (unsigned)a.Nq, (unsigned)a.B), dim3(256), 0, s, a, DH, chunks, false);
    rc = ldt_check_launch("attention_bwd_wide (dQ)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_kernel<DH, true>), dim3((unsigned)nkb, (unsigned)a.H, (unsigned)a.B), block, 0, s, a);
    return ldt_check_launch("attention_bwd_wide (dK, dV)");
}

// ---- narrow form, head dim 8 or 16.  Query blocks: first the statistics of the block's 16 query rows, which go to `stats` for the key blocks
// (the launch after it, in stream order) and stay in registers here; then the dQ sweep.  Key blocks: dK and dV.
template <int DH, bool KV>
__global__ __launch_bounds__(256) void attn_bwd_narrow_kernel(const AttnBwdArgs a, long units, int nrb) {
    constexpr int NP = DH / 8;                                          // 16-byte pieces of a head's slice of a row
    constexpr int NV = 4 * DH;                                          // partial sums per lane and output: [4 rows][DH channels]
    const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const long unit = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (unit >= units) return;                                          // whole wave; the waves of a workgroup share nothing
    const int r0 = (int)(unit % nrb) * AB_T;
    const long bh = unit / nrb;
    const int b = (int)(bh / a.H), head = (int)(bh % a.H);
    const AttnBwdRoles r = attn_bwd_roles<DH, KV>(a, b, head);
    // a row's whole head slice; rows past the end n repeat the last.  (The MFMA fragment, ld_frag, is loaded on its own: a select between
    // the pieces of this array would turn the array into an indexed one.)
    auto row_of = [&](const bf16_t* base, long ld, int row, int n, bf16x8 (&y)[NP]) {
        const bf16_t* p = base + (long)min(row, n - 1) * ld;
#pragma unroll
        for (int c = 0; c < NP; ++c) y[c] = *reinterpret_cast<const bf16x8*>(p + 8 * c);
    };
    const bf16x8 fa[1] = {ld_frag<DH>(r.rowA, r.ld_rowA, r0 + lr, r.NR, 0, lq)}, fb[1] = {ld_frag<DH>(r.rowB, r.ld_rowB, r0 + lr, r.NR, 0, lq)};

    float Lr[4] = {0.f, 0.f, 0.f, 0.f}, Dr[4] = {0.f, 0.f, 0.f, 0.f};   // query blocks: the statistics of rows 4 lq + i
    if constexpr (!KV) {
        row_lse<DH>(fa, r.colA, r.ld_colA, r.NC, a.scale, lr, lq, Lr);
        const float d = row_d<DH>(a.O + r.ob * DH, r0 + lr, r.NR, fb, lq);      // of row r0 + lr
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Dr[i] = __shfl(d, 4 * lq + i, 64);                          // from the lane whose lr is this row
            const int q = r0 + 4 * lq + i;
            if (lr == 0 && q < r.NR) r.st[2 * q] = Lr[i];
        }
        if (lq == 0 && r0 + lr < r.NR) r.st[2 * (r0 + lr) + 1] = d;
    }

    float acc1[NV], acc2[KV ? NV : 1];                                  // dQ | dK, and dV: [row 4 lq + i][channel], this lane's columns only
#pragma unroll
    for (int n = 0; n < NV; ++n) acc1[n] = 0.f;
#pragma unroll
    for (int n = 0; n < (KV ? NV : 1); ++n) acc2[n] = 0.f;
    for (int j0 = 0; j0 < r.NC; j0 += 16) {
        const int col = j0 + lr;                                        // this lane's column: a key (query blocks) or a query (key blocks)
        bf16x8 ya[NP], yb[NP];
        row_of(r.colA, r.ld_colA, col, r.NC, ya);
        row_of(r.colB, r.ld_colB, col, r.NC, yb);
        const f32x4 sc = tile_qk<DH>(fa, r.colA, r.ld_colA, col, r.NC, lq);
        const f32x4 dp = tile_qk<DH>(fb, r.colB, r.ld_colB, col, r.NC, lq);
        float p[4], ds[4];                                              // fp32: never an MFMA operand
        p_ds<KV>(sc, dp, a.scale, r, r0 + 4 * lq, col, Lr, Dr, p, ds);
#pragma unroll
        for (int cc = 0; cc < DH; ++cc) {
            const float y1 = (float)ya[cc >> 3][cc & 7];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc1[i * DH + cc] = fmaf(ds[i], y1, acc1[i * DH + cc]);
            if constexpr (KV) {
                const float y2 = (float)yb[cc >> 3][cc & 7];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc2[i * DH + cc] = fmaf(p[i], y2, acc2[i * DH + cc]);
            }
        }
    }

    // over the 16 lanes of an lq: after the four halvings this lane holds row 4 lq + (lr >> 2), channels c0 .. c0 + DH / 4 - 1
    narrow_halve<NV, 8>(acc1, lr);
    narrow_halve<NV / 2, 4>(acc1, lr);
    narrow_halve<NV / 4, 2>(acc1, lr);
    narrow_halve<NV / 8, 1>(acc1, lr);
    if constexpr (KV) {
        narrow_halve<NV, 8>(acc2, lr);
        narrow_halve<NV / 2, 4>(acc2, lr);
        narrow_halve<NV / 4, 2>(acc2, lr);
        narrow_halve<NV / 8, 1>(acc2, lr);
    }
    const int row = r0 + 4 * lq + (lr >> 2), c0 = ((lr >> 1) & 1) * (DH / 2) + (lr & 1) * (DH / 4);
    if (row >= r.NR) return;
    auto store = [&](bf16_t* dst, const float* v, float f) {
        if constexpr (DH == 8) {
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<bf16x2*>(dst) = (bf16x2){(bf16_t)(v[0] * f), (bf16_t)(v[1] * f)};
        } else {
            *reinterpret_cast<bf16x4*>(dst) = (bf16x4){(bf16_t)(v[0] * f), (bf16_t)(v[1] * f), (bf16_t)(v[2] * f), (bf16_t)(v[3] * f)};
        }
    };
    if constexpr (KV) {
        store(a.dK + (long)b * a.dkv_bs + (long)row * a.lddk + head * DH + c0, acc1, a.scale);
        store(a.dV + (long)b * a.dkv_bs + (long)row * a.lddv + head * DH + c0, acc2, 1.0f);
    } else {
        store(a.dQ + (long)b * a.dq_bs + (long)row * a.lddq + head * DH + c0, acc1, a.scale);
    }
}

template <int DH>
static int attn_bwd_narrow_launch(const AttnBwdArgs& a, hipStream_t s) {
    const int nqb = (a.Nq + AB_T - 1) / AB_T, nkb = (a.Nk + AB_T - 1) / AB_T;                  // query blocks, key blocks
    const long uq = (long)a.B * a.H * nqb, uk = (long)a.B * a.H * nkb, gq = (uq + 3) / 4, gk = (uk + 3) / 4;
    LDT_REQUIRE(gq < (1L << 31) && gk < (1L << 31), LDT_ESHAPE, "attention_bwd_narrow: grid too large");
    hipLaunchKernelGGL((attn_bwd_narrow_kernel<DH, false>), dim3((unsigned)gq), dim3(256), 0, s, a, uq, nqb);
    const int rc = ldt_check_launch("attention_bwd_narrow (row statistics, dQ)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_narrow_kernel<DH, true>), dim3((unsigned)gk), dim3(256), 0, s, a, uk, nkb);
    return ldt_check_launch("attention_bwd_narrow (dK, dV)");
}

// ---- the entry points (include/ldt_hip.h).  Each says which head widths and lengths it admits (`admit`: LDT_OK, or the status with the message
// set) and whether the narrow form's store rule holds for it; the rest is one body.  Order of the refusals: null, shape, stride, alignment.
template <class Admit>
static int attn_bwd_run(const char* name, Admit admit, const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk,
                        const uint16_t* V, int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats,
                        uint16_t* dQ, int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                        int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim, bool store8, void* stream,
                        float* part = nullptr, bool wide = false) {
    LDT_REQUIRE(Q && K && V && O && dO && stats && dQ && dK && dV, LDT_EARG, "%s: null pointer", name);
    const int rc = admit();
    if (rc != LDT_OK) return rc;
    LDT_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535, LDT_ESHAPE, "%s: B %d, H %d (1 .. 65535 each)", name, B, H);
    const long need = (long)H * head_dim;
    LDT_REQUIRE(ldq >= need && ldk >= need && ldv >= need && lddq >= need && lddk >= need && lddv >= need, LDT_ESHAPE,
                "%s: a row stride is shorter than heads * head_dim = %ld", name, need);
    LDT_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && q_batch_stride % 8 == 0 && kv_batch_stride % 8 == 0 && ldt_aligned16(Q) &&
                ldt_aligned16(K) && ldt_aligned16(V) && ldt_aligned16(O) && ldt_aligned16(dO), LDT_EALIGN,
                "%s: Q, K, V, O, dO rows must be 16-byte aligned", name);
    if (store8)                                                         // the narrow kernels store Dh / 4 adjacent channels at once (4 or 8 bytes)
        LDT_REQUIRE(lddq % 4 == 0 && lddk % 4 == 0 && lddv % 4 == 0 && dq_batch_stride % 4 == 0 && dkv_batch_stride % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dK) | reinterpret_cast<uintptr_t>(dV)) & 7u) == 0, LDT_EALIGN,
                    "%s: dQ, dK, dV rows must be 8-byte aligned", name);
    AttnBwdArgs a;
    a.Q = reinterpret_cast<const bf16_t*>(Q); a.ldq = ldq; a.q_bs = q_batch_stride;
    a.K = reinterpret_cast<const bf16_t*>(K); a.ldk = ldk; a.V = reinterpret_cast<const bf16_t*>(V); a.ldv = ldv; a.kv_bs = kv_batch_stride;
    a.O = reinterpret_cast<const bf16_t*>(O); a.dO = reinterpret_cast<const bf16_t*>(dO); a.stats = stats;
    a.dQ = reinterpret_cast<bf16_t*>(dQ); a.lddq = lddq; a.dq_bs = dq_batch_stride;
    a.dK = reinterpret_cast<bf16_t*>(dK); a.lddk = lddk; a.dV = reinterpret_cast<bf16_t*>(dV); a.lddv = lddv; a.dkv_bs = dkv_batch_stride;
    a.B = B; a.H = H; a.Nq = Nq; a.Nk = Nk; a.scale = 1.0f / sqrtf((float)head_dim);      // exactly 0.125 at 64
    a.part = part; a.cstat = nullptr;
    if (wide) {                                                         // scratch = the chunk statistics, then the dQ partials (include/ldt_hip.h)
        a.cstat = part;
        a.part = part + (long)((Nk + AB_WIDE_CHUNK - 1) / AB_WIDE_CHUNK) * B * H * Nq * 2;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (head_dim) {
        case 64: return attn_bwd_launch<64>(a, s);
        case 32: return wide ? attn_bwd_wide_launch<32>(a, s) : part ? attn_bwd_long_launch<32>(a, s) : attn_bwd_launch<32>(a, s);
        case 16: return attn_bwd_narrow_launch<16>(a, s);
        case 8: return attn_bwd_narrow_launch<8>(a, s);
    }
    LDT_REQUIRE(false, LDT_ESHAPE, "%s: no kernel for head_dim %d", name, head_dim);
}

extern "C" int ldt_attention_bwd(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                                 int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                                 int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                                 int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t N, int32_t head_dim, void* stream) {
    auto admit = [&]() -> int {
        LDT_REQUIRE(head_dim == 64 && N > 0 && N <= 512, LDT_ESHAPE, "attention_bwd: head_dim %d (64 only), N %d (self-attention, N <= 512)",
                    head_dim, N);
        return LDT_OK;
    };
    return attn_bwd_run("attention_bwd", admit, Q, ldq, q_batch_stride, K, ldk, V, ldv, kv_batch_stride, O, dO, stats, dQ, lddq,
                        dq_batch_stride, dK, lddk, dV, lddv, dkv_batch_stride, B, H, N, N, head_dim, false, stream);
}

// head dim 32 runs the MFMA form but keeps the store rule of the entry point it is reached through (include/ldt_hip.h)
extern "C" int ldt_attention_bwd_narrow(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk,
                                        const uint16_t* V, int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO,
                                        float* stats, uint16_t* dQ, int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk,
                                        uint16_t* dV, int64_t lddv, int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t N,
                                        int32_t head_dim, void* stream) {
    auto admit = [&]() -> int {
        LDT_REQUIRE(head_dim == 8 || head_dim == 16 || head_dim == 32, LDT_ESHAPE,
                    "attention_bwd_narrow: head_dim %d is not 8, 16 or 32 (64: ldt_attention_bwd)", head_dim);
        LDT_REQUIRE(N > 0 && N <= 512, LDT_ESHAPE, "attention_bwd_narrow: N %d (self-attention, N <= 512)", N);
        return LDT_OK;
    };
    return attn_bwd_run("attention_bwd_narrow", admit, Q, ldq, q_batch_stride, K, ldk, V, ldv, kv_batch_stride, O, dO, stats, dQ, lddq,
                        dq_batch_stride, dK, lddk, dV, lddv, dkv_batch_stride, B, H, N, N, head_dim, true, stream);
}

// At Nq = Nk the result equals the self-attention entry points' bit for bit.
extern "C" int ldt_attention_bwd_cross(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk,
                                       const uint16_t* V, int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO,
                                       float* stats, uint16_t* dQ, int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk,
                                       uint16_t* dV, int64_t lddv, int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t Nq, int32_t Nk,
                                       int32_t head_dim, void* stream) {
    auto admit = [&]() -> int {
        LDT_REQUIRE(head_dim == 8 || head_dim == 16 || head_dim == 32 || head_dim == 64, LDT_ESHAPE,
                    "attention_bwd_cross: head_dim %d is not 8, 16, 32 or 64", head_dim);
        LDT_REQUIRE(Nq > 0 && Nq <= 512 && Nk > 0 && Nk <= 512, LDT_ESHAPE, "attention_bwd_cross: Nq %d, Nk %d (1 <= Nq, Nk <= 512)", Nq, Nk);
        return LDT_OK;
    };
    return attn_bwd_run("attention_bwd_cross", admit, Q, ldq, q_batch_stride, K, ldk, V, ldv, kv_batch_stride, O, dO, stats, dQ, lddq,
                        dq_batch_stride, dK, lddk, dV, lddv, dkv_batch_stride, B, H, Nq, Nk, head_dim, head_dim <= 16, stream);
}

// The operand contract of ldt_attention_bwd_cross with a query axis of up to 8192 rows, head width 32 (the Compressor's 128 / 4) alone.
extern "C" int ldt_attention_bwd_long(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                                      int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                                      int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                                      int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim, float* scratch,
                                      int64_t scratch_len, void* stream) {
    auto admit = [&]() -> int {
        LDT_REQUIRE(scratch, LDT_EARG, "attention_bwd_long: null pointer");
        LDT_REQUIRE(head_dim == 32, LDT_ESHAPE, "attention_bwd_long: head_dim %d (32 only)", head_dim);
        LDT_REQUIRE(Nq > 0 && Nq <= LDT_ATTN_BWD_LONG_MAX_QUERIES && Nk > 0 && Nk <= 512, LDT_ESHAPE,
                    "attention_bwd_long: Nq %d, Nk %d (1 <= Nq <= %d, 1 <= Nk <= 512)", Nq, Nk, LDT_ATTN_BWD_LONG_MAX_QUERIES);
        LDT_REQUIRE(B > 0 && H > 0 && scratch_len >= ((int64_t)(Nq + AB_CHUNK - 1) / AB_CHUNK) * B * Nk * 2 * H * head_dim, LDT_ESHAPE,
                    "attention_bwd_long: scratch holds %ld floats, ceil(Nq / %d) * B * Nk * 2 * H * head_dim are needed", (long)scratch_len, AB_CHUNK);
        return LDT_OK;
    };
    return attn_bwd_run("attention_bwd_long", admit, Q, ldq, q_batch_stride, K, ldk, V, ldv, kv_batch_stride, O, dO, stats, dQ, lddq,
                        dq_batch_stride, dK, lddk, dV, lddv, dkv_batch_stride, B, H, Nq, Nk, head_dim, false, stream, scratch);
}

// The operand contract of ldt_attention_bwd_cross with a key axis of up to 8192 rows, head width 32 alone: the mirror image of the above.
extern "C" int ldt_attention_bwd_wide(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                                      int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                                      int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                                      int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t Nq, int32_t Nk, int32_t head_dim, float* scratch,
                                      int64_t scratch_len, void* stream) {
    auto admit = [&]() -> int {
        LDT_REQUIRE(scratch, LDT_EARG, "attention_bwd_wide: null pointer");
        LDT_REQUIRE(head_dim == 32, LDT_ESHAPE, "attention_bwd_wide: head_dim %d (32 only)", head_dim);
        LDT_REQUIRE(Nq > 0 && Nq <= 512 && Nk > 0 && Nk <= LDT_ATTN_BWD_WIDE_MAX_KEYS, LDT_ESHAPE,
                    "attention_bwd_wide: Nq %d, Nk %d (1 <= Nq <= 512, 1 <= Nk <= %d)", Nq, Nk, LDT_ATTN_BWD_WIDE_MAX_KEYS);
        LDT_REQUIRE(B > 0 && H > 0 && scratch_len >= ((int64_t)(Nk + AB_WIDE_CHUNK - 1) / AB_WIDE_CHUNK) * B * H * Nq * (2 + head_dim), LDT_EARG,
                    "attention_bwd_wide: scratch holds %ld floats, ceil(Nk / %d) * B * H * Nq * (2 + head_dim) are needed", (long)scratch_len,
                    AB_WIDE_CHUNK);
        return LDT_OK;
    };
    return attn_bwd_run("attention_bwd_wide", admit, Q, ldq, q_batch_stride, K, ldk, V, ldv, kv_batch_stride, O, dO, stats, dQ, lddq,
                        dq_batch_stride, dK, lddk, dV, lddv, dkv_batch_stride, B, H, Nq, Nk, head_dim, false, stream, scratch, true);
}
