// Attention backward of a Score block (model/layers.py:190-197), head dim 64 or 32 (heads of 8 and 16: attention_narrow_bwd.hip),
// Nq, Nk <= 512, gfx950.  Self-attention (ldt_attention_bwd, ldt_attention_bwd_narrow) runs it at Nq = Nk = N; cross-attention to the
// point condition (ldt_attention_bwd_cross, attention_narrow_bwd.hip) with Nk keys from another tensor: the query-block kernels tile Nq
// and loop to Nk, the key-block kernel tiles Nk and loops to Nq, and every clamp and guard takes the extent of the axis it indexes.
//   forward:   S = Q K^T / sqrt(Dh),  P = softmax(S),  O = P V          (O is the [B][H][N][Dh] buffer the reference re-reads as (B N, C): quirk Q1;
//                                                                       its gradient dO arrives in the same raw layout — nothing is permuted)
//   backward:  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - D),  D = rowsum(dO o O),  dQ = dS K / sqrt(Dh),  dK = dS^T Q / sqrt(Dh)
// The forward kernels write no log-sum-exp, so a first kernel recomputes each query row's maximum and sum (kept as L = max + ln(sum), so that
// P = exp(S - L)) together with D.  Then dQ is produced per block of 16 query rows looping over the keys, and dK / dV per block of 16 keys
// looping over the queries: every output element is summed inside one wave in a fixed order — no atomics, no sum across workgroups, the same
// bits on every run.
// Products: v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  S and dP (and their transposes in the key-block kernel) take their operand
// fragments straight from global rows (lane l: row l & 15, 8 contiguous head channels at 8 (l >> 4)); P and dS are rounded to bf16 and cross
// one LDS tile to become the A operand of the second products.  One wave per workgroup: this is the correct, unfused form of the step.
// The three kernels are templates on the head dim DH: DH / 32 operand chunks of the first products, DH / 16 accumulator tiles of the second.
// ldt_attention_bwd runs the 64 instantiation; the 32 one is reached from ldt_attention_bwd_narrow (attention_narrow_bwd.hip).
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define AB_T 16                      // rows (dQ kernel: queries, dK/dV kernel: keys) per workgroup
#define AB_J 32                      // columns per loop iteration: the K extent of one 16x16x32 product
#define AB_LDP (AB_J + 8)            // LDS row pitch of the P / dS tiles, bf16 elements (80 B: 16-B aligned rows, staggered banks)

__device__ __forceinline__ bf16x8 ld_frag(const bf16_t* base, long ld, int row, int nrows, int chunk) {
    const int r = row < nrows ? row : nrows - 1;          // rows past the end repeat the last one: finite values that a zero weight removes
    return *reinterpret_cast<const bf16x8*>(base + (long)r * ld + chunk * 8);
}

template <int NS>
__device__ __forceinline__ f32x4 tile_qk(const bf16x8 (&a)[NS], const bf16_t* base, long ld, int row, int nrows, int lq) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[s], ld_frag(base, ld, row, nrows, 4 * s + lq), acc, 0, 0, 0);
    return acc;
}

// ---- per query row: L = max_j s_j + ln sum_j exp(s_j - max), s = scale * q . k_j;  D = sum_d dO o O
template <int DH>
__global__ __launch_bounds__(64) void attn_bwd_stats_kernel(const AttnBwdArgs a) {
    constexpr int NS = DH / 32;                                         // 32-channel steps of the first products
    const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * AB_T;
    const bf16_t* Qb = a.Q + (long)b * a.q_bs + h * DH;
    const bf16_t* Kb = a.K + (long)b * a.kv_bs + h * DH;
    const long ob = ((long)b * a.H + h) * a.Nq;
    bf16x8 qf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = ld_frag(Qb, a.ldq, q0 + lr, a.Nq, 4 * s + lq);
    // lane holds S[query 4 lq + i][key j0 + lr]
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int j0 = 0; j0 < a.Nk; j0 += 16) {
        const f32x4 sc = tile_qk(qf, Kb, a.ldk, j0 + lr, a.Nk, lq);
        if (j0 + lr < a.Nk) {
#pragma unroll
            for (int i = 0; i < 4; ++i) mx[i] = fmaxf(mx[i], sc[i] * a.scale);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], o, 64));
    float sm[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < a.Nk; j0 += 16) {
        const f32x4 sc = tile_qk(qf, Kb, a.ldk, j0 + lr, a.Nk, lq);
        if (j0 + lr < a.Nk) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sm[i] += expf(sc[i] * a.scale - mx[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sm[i] += __shfl_xor(sm[i], o, 64);
    // D: lane (lr, lq) sums channels 8 lq .. + 7 (and 32 + 8 lq .. + 7 at DH 64) of row q0 + lr, then the four lq
    float d = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const bf16x8 o8 = ld_frag(a.O + ob * DH, DH, q0 + lr, a.Nq, 4 * s + lq);
        const bf16x8 g8 = ld_frag(a.dO + ob * DH, DH, q0 + lr, a.Nq, 4 * s + lq);
#pragma unroll
        for (int j = 0; j < 8; ++j) d += (float)o8[j] * (float)g8[j];
    }
    d += __shfl_xor(d, 16, 64);
    d += __shfl_xor(d, 32, 64);
    if (lr == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + 4 * lq + i;
            if (q < a.Nq) a.stats[(ob + q) * 2] = mx[i] + logf(sm[i]);
        }
    }
    if (lq == 0 && q0 + lr < a.Nq) a.stats[(ob + q0 + lr) * 2 + 1] = d;
}

// ---- the two main kernels share one body.
// KV = false: the block's 16 rows are queries, the loop runs over keys:    S = Q K^T,   dP = dO V^T,   dQ  = scale dS K
// KV = true:  the block's 16 rows are keys,    the loop runs over queries: S^T = K Q^T, dP^T = V dO^T, dK = scale dS^T Q,  dV = P^T dO
// In both the accumulator tile puts the block's rows at 4 (l >> 4) + i and the loop's column at l & 15.
template <int DH, bool KV>
__global__ __launch_bounds__(64) void attn_bwd_kernel(const AttnBwdArgs a) {
    constexpr int NS = DH / 32, NT = DH / 16;                           // operand chunks of 32 channels, accumulator tiles of 16
    __shared__ __attribute__((aligned(16))) bf16_t ds_t[AB_T][AB_LDP];
    __shared__ __attribute__((aligned(16))) bf16_t p_t[AB_T][AB_LDP];
    const int lane = threadIdx.x, lr = lane & 15, lq = lane >> 4;
    const int b = blockIdx.z, h = blockIdx.y, r0 = blockIdx.x * AB_T;
    const int NR = KV ? a.Nk : a.Nq, NC = KV ? a.Nq : a.Nk;            // extents of the block's row axis and of the loop's column axis
    const long ob = ((long)b * a.H + h) * a.Nq;
    const bf16_t* Qb = a.Q + (long)b * a.q_bs + h * DH;
    const bf16_t* Kb = a.K + (long)b * a.kv_bs + h * DH;
    const bf16_t* Vb = a.V + (long)b * a.kv_bs + h * DH;
    const bf16_t* Gb = a.dO + ob * DH;
    const float* st = a.stats + ob * 2;
    // rows of the block (A operands of the first products) and the loop's operands
    const bf16_t* rowA = KV ? Kb : Qb; const long ld_rowA = KV ? a.ldk : a.ldq;
    const bf16_t* rowB = KV ? Vb : Gb; const long ld_rowB = KV ? a.ldv : DH;
    const bf16_t* colA = KV ? Qb : Kb; const long ld_colA = KV ? a.ldq : a.ldk;
    const bf16_t* colB = KV ? Gb : Vb; const long ld_colB = KV ? DH : a.ldv;
    bf16x8 fa[NS], fb[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        fa[s] = ld_frag(rowA, ld_rowA, r0 + lr, NR, 4 * s + lq);
        fb[s] = ld_frag(rowB, ld_rowB, r0 + lr, NR, 4 * s + lq);
    }
    float Lr[4], Dr[4];                 // KV = false: the statistics of the block's query rows 4 lq + i
    if (!KV) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = min(r0 + 4 * lq + i, NR - 1);
            Lr[i] = st[2 * q]; Dr[i] = st[2 * q + 1];
        }
    }
    f32x4 acc1[NT], acc2[NT];           // [16 rows][DH channels] as 16-column tiles: dQ | dK, and dV
#pragma unroll
    for (int t = 0; t < NT; ++t) { acc1[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc2[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }

    for (int j0 = 0; j0 < NC; j0 += AB_J) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int col = j0 + 16 * half + lr;                       // this lane's column of the tile: a key (KV false) or a query (KV true)
            const f32x4 sc = tile_qk(fa, colA, ld_colA, col, NC, lq);
            const f32x4 dp = tile_qk(fb, colB, ld_colB, col, NC, lq);
            float Lc = 0.f, Dc = 0.f;
            if (KV) { const int q = min(col, NC - 1); Lc = st[2 * q]; Dc = st[2 * q + 1]; }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool live = col < NC && r0 + 4 * lq + i < NR;
                const float p = live ? expf(sc[i] * a.scale - (KV ? Lc : Lr[i])) : 0.f;
                const float dsv = p * (dp[i] - (KV ? Dc : Dr[i]));
                ds_t[4 * lq + i][16 * half + lr] = (bf16_t)dsv;        // P and dS are rounded to bf16 here, before the second products
                if (KV) p_t[4 * lq + i][16 * half + lr] = (bf16_t)p;
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
                const int r = min(j0 + 8 * lq + e, NC - 1);
                y1[e] = colA[(long)r * ld_colA + 16 * t + lr];
                if (KV) y2[e] = colB[(long)r * ld_colB + 16 * t + lr];
            }
            acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dsf, y1, acc1[t], 0, 0, 0);
            if (KV) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, y2, acc2[t], 0, 0, 0);
        }
    }
    bf16_t* o1 = KV ? a.dK + (long)b * a.dkv_bs + h * DH : a.dQ + (long)b * a.dq_bs + h * DH;
    const long ld1 = KV ? a.lddk : a.lddq;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + 4 * lq + i;
            if (r < NR) {
                o1[(long)r * ld1 + 16 * t + lr] = (bf16_t)(acc1[t][i] * a.scale);
                if (KV) a.dV[(long)b * a.dkv_bs + h * DH + (long)r * a.lddv + 16 * t + lr] = (bf16_t)acc2[t][i];
            }
        }
}

template <int DH>
static int attn_bwd_launch_dh(const AttnBwdArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.Nq + AB_T - 1) / AB_T), (unsigned)a.H, (unsigned)a.B), block(64);      // query blocks
    const dim3 grid_kv((unsigned)((a.Nk + AB_T - 1) / AB_T), (unsigned)a.H, (unsigned)a.B);               // key blocks
    hipLaunchKernelGGL(attn_bwd_stats_kernel<DH>, grid, block, 0, s, a);
    int rc = ldt_check_launch("attention_bwd (row statistics)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_kernel<DH, false>), grid, block, 0, s, a);
    rc = ldt_check_launch("attention_bwd (dQ)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_kernel<DH, true>), grid_kv, block, 0, s, a);
    return ldt_check_launch("attention_bwd (dK, dV)");
}

int ldt_attn_bwd_launch(const AttnBwdArgs* a, int dh, hipStream_t s) {   // the entry points have checked the operands
    LDT_REQUIRE(dh == 64 || dh == 32, LDT_ESHAPE, "attention_bwd (MFMA form): head dim %d is not 32 or 64", dh);
    return dh == 64 ? attn_bwd_launch_dh<64>(*a, s) : attn_bwd_launch_dh<32>(*a, s);
}

extern "C" int ldt_attention_bwd(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk, const uint16_t* V,
                                 int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO, float* stats, uint16_t* dQ,
                                 int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk, uint16_t* dV, int64_t lddv,
                                 int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t N, int32_t head_dim, void* stream) {
    LDT_REQUIRE(Q && K && V && O && dO && stats && dQ && dK && dV, LDT_EARG, "attention_bwd: null pointer");
    LDT_REQUIRE(head_dim == 64 && B > 0 && B <= 65535 && H > 0 && H <= 65535 && N > 0 && N <= 512, LDT_ESHAPE,
                "attention_bwd: head_dim %d (64 only), B %d, H %d, N %d (self-attention, N <= 512)", head_dim, B, H, N);
    const long need = (long)H * 64;
    LDT_REQUIRE(ldq >= need && ldk >= need && ldv >= need && lddq >= need && lddk >= need && lddv >= need, LDT_ESHAPE,
                "attention_bwd: a row stride is shorter than heads * 64 = %ld", need);
    LDT_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && q_batch_stride % 8 == 0 && kv_batch_stride % 8 == 0 && ldt_aligned16(Q) &&
                ldt_aligned16(K) && ldt_aligned16(V) && ldt_aligned16(O) && ldt_aligned16(dO), LDT_EALIGN,
                "attention_bwd: Q, K, V, O, dO rows must be 16-byte aligned");
    AttnBwdArgs a;
    a.Q = reinterpret_cast<const bf16_t*>(Q); a.ldq = ldq; a.q_bs = q_batch_stride;
    a.K = reinterpret_cast<const bf16_t*>(K); a.ldk = ldk; a.V = reinterpret_cast<const bf16_t*>(V); a.ldv = ldv; a.kv_bs = kv_batch_stride;
    a.O = reinterpret_cast<const bf16_t*>(O); a.dO = reinterpret_cast<const bf16_t*>(dO); a.stats = stats;
    a.dQ = reinterpret_cast<bf16_t*>(dQ); a.lddq = lddq; a.dq_bs = dq_batch_stride;
    a.dK = reinterpret_cast<bf16_t*>(dK); a.lddk = lddk; a.dV = reinterpret_cast<bf16_t*>(dV); a.lddv = lddv; a.dkv_bs = dkv_batch_stride;
    a.B = B; a.H = H; a.Nq = N; a.Nk = N; a.scale = 0.125f;
    return ldt_attn_bwd_launch(&a, 64, reinterpret_cast<hipStream_t>(stream));
}
