// Self-attention backward for narrow heads, Dh = 8 or 16 (gfx950 / MI355X), and the entry point of every head dim below 64: the
// reference's hybrid config trains a Score with hidden 128 and 16 heads.  The contract is ldt_attention_bwd's (attention_bwd.hip) but for
// the head dim: Nq = Nk = N <= 512, Q / K / V bf16 row views with head h at column h Dh, O and dO the raw [B][H][N][Dh] buffer (quirk Q1),
//   dV = P^T dO,  dP = dO V^T,  dS = P o (dP - D),  D = rowsum(dO o O),  dQ = dS K Dh^-0.5,  dK = dS^T Q Dh^-0.5,  P = exp(S Dh^-0.5 - L),
// fp32 sums, no atomics, no sum across workgroups, every output element summed in one fixed order.
//
// Decomposition, as the forward's (attention_narrow.hip): ONE WAVE per (sample, head, block of 16 rows), four such waves per workgroup,
// nothing shared between them: no LDS, no barrier.  Two launches:
//   query blocks   first the statistics of the block's 16 query rows: L = max + ln(sum) from two sweeps over the keys (one MFMA per 16 keys
//                  each: the maximum, then the sum — the 64-wide kernel's arithmetic) and D, whose channel sum runs across the lanes of one
//                  lr; both go to `stats` for the second launch and stay in registers here.  Then the dQ sweep.
//   key blocks     reads L and D per query column from `stats` (written by the launch before it, in stream order); dK and dV.
// First products   S = Q K^T and dP = dO V^T (key blocks: their transposes K Q^T and V dO^T): one v_mfma_f32_16x16x32_bf16 per 16 columns
//                  with the K extent zero-padded as in the forward: lane (lr, lq) supplies channels 8 lq ..+7 where 8 lq < Dh and a zero
//                  fragment elsewhere, and receives element [row 4 lq + i][column lr].
// Second products  NOT MFMAs, for the forward's reason: the lane holds P and dS of ONE column for four rows, and that column's K (Q, dO)
//                  slice is one or two 16-byte loads in its natural layout: 4 x Dh fused multiply-adds per product into per-lane partial
//                  sums.  P and dS therefore STAY fp32 (they never become MFMA operands): the 2^-8 terms of the 64 / 32-wide bound are
//                  absent here.
//   end            narrow_halve x 4 sums the partials over the 16 lanes of an lq in a fixed order and leaves each lane Dh / 4 adjacent
//                  channels of one row: times the scale (dQ, dK), one 4- or 8-byte store.
// Rows and columns past the end re-read the last row (never out of bounds) and get weight exactly 0.
//
// ldt_attention_bwd_cross (the end of this file) is the same contract with two lengths: the cross-attention of the even blocks of a
// conditioned Score (model/layers.py:183-200 with y = the point condition, model/scorenet/score.py:129-149): Nq query rows, Nk key / value
// rows from another tensor.  It runs these kernels (8, 16) or attention_bwd.hip's (32, 64) with AttnBwdArgs.Nq != Nk: query blocks tile Nq
// and loop to Nk, key blocks tile Nk and loop to Nq; O, dO and `stats` are per query.
#include "../../include/ldt_hip.h"
#include "kernels.h"

template <int DH, bool KV>
__global__ __launch_bounds__(256) void attn_bwd_narrow_kernel(const AttnBwdArgs a, long units, int nrb) {
    constexpr int NP = DH / 8;                                          // 16-byte pieces of a head's slice of a row
    constexpr int NV = 4 * DH;                                          // partial sums per lane and output: [4 rows][DH channels]
    const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const long unit = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (unit >= units) return;                                          // whole wave; the waves of a workgroup share nothing
    const int NR = KV ? a.Nk : a.Nq, NC = KV ? a.Nq : a.Nk;            // extents of the block's row axis and of the loop's column axis
    const int r0 = (int)(unit % nrb) * 16;
    const long bh = unit / nrb, ob = bh * a.Nq;
    const int b = (int)(bh / a.H), head = (int)(bh % a.H);
    const bf16_t* Qb = a.Q + (long)b * a.q_bs + head * DH;
    const bf16_t* Kb = a.K + (long)b * a.kv_bs + head * DH;
    const bf16_t* Vb = a.V + (long)b * a.kv_bs + head * DH;
    const bf16_t* Gb = a.dO + ob * DH;
    float* st = a.stats + ob * 2;
    const bool live = lq < NP;                                          // this lane's 8 channels of the K extent exist
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    auto row_of = [&](const bf16_t* base, long ld, int row, int n, bf16x8 (&y)[NP]) {   // a row's whole head slice; rows past the end n repeat the last
        const bf16_t* p = base + (long)min(row, n - 1) * ld;
#pragma unroll
        for (int c = 0; c < NP; ++c) y[c] = *reinterpret_cast<const bf16x8*>(p + 8 * c);
    };
    // this lane's MFMA fragment of a row: chunk lq, zero past Dh (loaded on its own: a select between the pieces of row_of's array would
    // turn the array into an indexed one)
    auto frag_of = [&](const bf16_t* base, long ld, int row, int n) -> bf16x8 {
        const bf16x8 t = *reinterpret_cast<const bf16x8*>(base + (long)min(row, n - 1) * ld + 8 * (lq & (NP - 1)));
        return live ? t : zero;
    };
    // the block's rows (A operands of the first products) and the loop's columns
    const bf16_t* rowA = KV ? Kb : Qb; const long ld_rowA = KV ? a.ldk : a.ldq;
    const bf16_t* rowB = KV ? Vb : Gb; const long ld_rowB = KV ? a.ldv : DH;
    const bf16_t* colA = KV ? Qb : Kb; const long ld_colA = KV ? a.ldq : a.ldk;
    const bf16_t* colB = KV ? Gb : Vb; const long ld_colB = KV ? DH : a.ldv;
    const bf16x8 fa = frag_of(rowA, ld_rowA, r0 + lr, NR), fb = frag_of(rowB, ld_rowB, r0 + lr, NR);
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

    float Lr[4] = {0.f, 0.f, 0.f, 0.f}, Dr[4] = {0.f, 0.f, 0.f, 0.f};   // query blocks: the statistics of rows 4 lq + i
    if constexpr (!KV) {
        float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int j0 = 0; j0 < NC; j0 += 16) {
            const f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, frag_of(Kb, a.ldk, j0 + lr, NC), z4, 0, 0, 0);
            if (j0 + lr < NC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) mx[i] = fmaxf(mx[i], sc[i] * a.scale);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int x = 8; x > 0; x >>= 1) mx[i] = fmaxf(mx[i], __shfl_xor(mx[i], x, 64));
        float sm[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j0 = 0; j0 < NC; j0 += 16) {
            const f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, frag_of(Kb, a.ldk, j0 + lr, NC), z4, 0, 0, 0);
            if (j0 + lr < NC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) sm[i] += expf(sc[i] * a.scale - mx[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int x = 8; x > 0; x >>= 1) sm[i] += __shfl_xor(sm[i], x, 64);
        // D of row r0 + lr: lane (lr, lq) sums its 8 channels (a zero fragment past Dh), then the four lq: the same bits in all four
        float d = 0.f;
        {
            const bf16x8 o8 = frag_of(a.O + ob * DH, DH, r0 + lr, NR);
#pragma unroll
            for (int j = 0; j < 8; ++j) d += (float)o8[j] * (float)fb[j];
        }
        d += __shfl_xor(d, 16, 64);
        d += __shfl_xor(d, 32, 64);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Lr[i] = mx[i] + logf(sm[i]);
            Dr[i] = __shfl(d, 4 * lq + i, 64);                          // from the lane whose lr is this row
            const int q = r0 + 4 * lq + i;
            if (lr == 0 && q < NR) st[2 * q] = Lr[i];
        }
        if (lq == 0 && r0 + lr < NR) st[2 * (r0 + lr) + 1] = d;
    }

    float acc1[NV], acc2[KV ? NV : 1];                                  // dQ | dK, and dV: [row 4 lq + i][channel], this lane's columns only
#pragma unroll
    for (int n = 0; n < NV; ++n) acc1[n] = 0.f;
#pragma unroll
    for (int n = 0; n < (KV ? NV : 1); ++n) acc2[n] = 0.f;
    for (int j0 = 0; j0 < NC; j0 += 16) {
        const int col = j0 + lr;                                        // this lane's column: a key (query blocks) or a query (key blocks)
        bf16x8 ya[NP], yb[NP];
        row_of(colA, ld_colA, col, NC, ya);
        row_of(colB, ld_colB, col, NC, yb);
        const f32x4 sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, frag_of(colA, ld_colA, col, NC), z4, 0, 0, 0);
        const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb, frag_of(colB, ld_colB, col, NC), z4, 0, 0, 0);
        float Lc = 0.f, Dc = 0.f;
        if (KV) { const int q = min(col, NC - 1); Lc = st[2 * q]; Dc = st[2 * q + 1]; }
        float p[4], ds[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = col < NC && r0 + 4 * lq + i < NR;
            p[i] = in ? expf(sc[i] * a.scale - (KV ? Lc : Lr[i])) : 0.f;
            ds[i] = p[i] * (dp[i] - (KV ? Dc : Dr[i]));                 // fp32, as P: never an MFMA operand
        }
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
    if (row >= NR) return;
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
static int attn_bwd_narrow_launch_dh(const AttnBwdArgs& a, hipStream_t s) {
    const int nqb = (a.Nq + 15) / 16, nkb = (a.Nk + 15) / 16;                                  // query blocks, key blocks
    const long uq = (long)a.B * a.H * nqb, uk = (long)a.B * a.H * nkb, gq = (uq + 3) / 4, gk = (uk + 3) / 4;
    LDT_REQUIRE(gq < (1L << 31) && gk < (1L << 31), LDT_ESHAPE, "attention_bwd_narrow: grid too large");
    hipLaunchKernelGGL((attn_bwd_narrow_kernel<DH, false>), dim3((unsigned)gq), dim3(256), 0, s, a, uq, nqb);
    const int rc = ldt_check_launch("attention_bwd_narrow (row statistics, dQ)");
    if (rc != LDT_OK) return rc;
    hipLaunchKernelGGL((attn_bwd_narrow_kernel<DH, true>), dim3((unsigned)gk), dim3(256), 0, s, a, uk, nkb);
    return ldt_check_launch("attention_bwd_narrow (dK, dV)");
}

int ldt_attn_bwd_narrow_launch(const AttnBwdArgs* a, int dh, hipStream_t s) {   // the entry point has checked the operands
    LDT_REQUIRE(dh == 8 || dh == 16, LDT_ESHAPE, "attention_bwd_narrow: head dim %d is not 8 or 16", dh);
    return dh == 8 ? attn_bwd_narrow_launch_dh<8>(*a, s) : attn_bwd_narrow_launch_dh<16>(*a, s);
}

extern "C" int ldt_attention_bwd_narrow(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk,
                                        const uint16_t* V, int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO,
                                        float* stats, uint16_t* dQ, int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk,
                                        uint16_t* dV, int64_t lddv, int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t N,
                                        int32_t head_dim, void* stream) {
    LDT_REQUIRE(Q && K && V && O && dO && stats && dQ && dK && dV, LDT_EARG, "attention_bwd_narrow: null pointer");
    LDT_REQUIRE(head_dim == 8 || head_dim == 16 || head_dim == 32, LDT_ESHAPE,
                "attention_bwd_narrow: head_dim %d is not 8, 16 or 32 (64: ldt_attention_bwd)", head_dim);
    LDT_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && N > 0 && N <= 512, LDT_ESHAPE,
                "attention_bwd_narrow: B %d, H %d, N %d (self-attention, N <= 512)", B, H, N);
    const long need = (long)H * head_dim;
    LDT_REQUIRE(ldq >= need && ldk >= need && ldv >= need && lddq >= need && lddk >= need && lddv >= need, LDT_ESHAPE,
                "attention_bwd_narrow: a row stride is shorter than heads * head_dim = %ld", need);
    LDT_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && q_batch_stride % 8 == 0 && kv_batch_stride % 8 == 0 && ldt_aligned16(Q) &&
                ldt_aligned16(K) && ldt_aligned16(V) && ldt_aligned16(O) && ldt_aligned16(dO), LDT_EALIGN,
                "attention_bwd_narrow: Q, K, V, O, dO rows must be 16-byte aligned");
    // the narrow kernels store Dh / 4 adjacent channels at once (4 or 8 bytes)
    LDT_REQUIRE(lddq % 4 == 0 && lddk % 4 == 0 && lddv % 4 == 0 && dq_batch_stride % 4 == 0 && dkv_batch_stride % 4 == 0 &&
                ((reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dK) | reinterpret_cast<uintptr_t>(dV)) & 7u) == 0, LDT_EALIGN,
                "attention_bwd_narrow: dQ, dK, dV rows must be 8-byte aligned");
    AttnBwdArgs a;
    a.Q = reinterpret_cast<const bf16_t*>(Q); a.ldq = ldq; a.q_bs = q_batch_stride;
    a.K = reinterpret_cast<const bf16_t*>(K); a.ldk = ldk; a.V = reinterpret_cast<const bf16_t*>(V); a.ldv = ldv; a.kv_bs = kv_batch_stride;
    a.O = reinterpret_cast<const bf16_t*>(O); a.dO = reinterpret_cast<const bf16_t*>(dO); a.stats = stats;
    a.dQ = reinterpret_cast<bf16_t*>(dQ); a.lddq = lddq; a.dq_bs = dq_batch_stride;
    a.dK = reinterpret_cast<bf16_t*>(dK); a.lddk = lddk; a.dV = reinterpret_cast<bf16_t*>(dV); a.lddv = lddv; a.dkv_bs = dkv_batch_stride;
    a.B = B; a.H = H; a.Nq = N; a.Nk = N; a.scale = 1.0f / sqrtf((float)head_dim);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return head_dim == 32 ? ldt_attn_bwd_launch(&a, 32, s) : ldt_attn_bwd_narrow_launch(&a, head_dim, s);
}

// Cross-attention backward: ldt_attention_bwd's contract with Nq query rows and Nk key / value rows (model/layers.py:183-200 with
// y = pts_condition; model/scorenet/score.py:129-149: the even blocks of a conditioned Score).  Every head width: 64 and 32 run
// attention_bwd.hip's kernels, 8 and 16 the ones above.  At Nq = Nk the result equals the self-attention entry points' bit for bit.
extern "C" int ldt_attention_bwd_cross(const uint16_t* Q, int64_t ldq, int64_t q_batch_stride, const uint16_t* K, int64_t ldk,
                                       const uint16_t* V, int64_t ldv, int64_t kv_batch_stride, const uint16_t* O, const uint16_t* dO,
                                       float* stats, uint16_t* dQ, int64_t lddq, int64_t dq_batch_stride, uint16_t* dK, int64_t lddk,
                                       uint16_t* dV, int64_t lddv, int64_t dkv_batch_stride, int32_t B, int32_t H, int32_t Nq, int32_t Nk,
                                       int32_t head_dim, void* stream) {
    LDT_REQUIRE(Q && K && V && O && dO && stats && dQ && dK && dV, LDT_EARG, "attention_bwd_cross: null pointer");
    LDT_REQUIRE(head_dim == 8 || head_dim == 16 || head_dim == 32 || head_dim == 64, LDT_ESHAPE,
                "attention_bwd_cross: head_dim %d is not 8, 16, 32 or 64", head_dim);
    LDT_REQUIRE(B > 0 && B <= 65535 && H > 0 && H <= 65535 && Nq > 0 && Nq <= 512 && Nk > 0 && Nk <= 512, LDT_ESHAPE,
                "attention_bwd_cross: B %d, H %d, Nq %d, Nk %d (1 <= Nq, Nk <= 512)", B, H, Nq, Nk);
    const long need = (long)H * head_dim;
    LDT_REQUIRE(ldq >= need && ldk >= need && ldv >= need && lddq >= need && lddk >= need && lddv >= need, LDT_ESHAPE,
                "attention_bwd_cross: a row stride is shorter than heads * head_dim = %ld", need);
    LDT_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && q_batch_stride % 8 == 0 && kv_batch_stride % 8 == 0 && ldt_aligned16(Q) &&
                ldt_aligned16(K) && ldt_aligned16(V) && ldt_aligned16(O) && ldt_aligned16(dO), LDT_EALIGN,
                "attention_bwd_cross: Q, K, V, O, dO rows must be 16-byte aligned");
    if (head_dim <= 16)                                                 // the narrow kernels store Dh / 4 adjacent channels at once (4 or 8 bytes)
        LDT_REQUIRE(lddq % 4 == 0 && lddk % 4 == 0 && lddv % 4 == 0 && dq_batch_stride % 4 == 0 && dkv_batch_stride % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dK) | reinterpret_cast<uintptr_t>(dV)) & 7u) == 0, LDT_EALIGN,
                    "attention_bwd_cross: dQ, dK, dV rows must be 8-byte aligned at head_dim 8 and 16");
    AttnBwdArgs a;
    a.Q = reinterpret_cast<const bf16_t*>(Q); a.ldq = ldq; a.q_bs = q_batch_stride;
    a.K = reinterpret_cast<const bf16_t*>(K); a.ldk = ldk; a.V = reinterpret_cast<const bf16_t*>(V); a.ldv = ldv; a.kv_bs = kv_batch_stride;
    a.O = reinterpret_cast<const bf16_t*>(O); a.dO = reinterpret_cast<const bf16_t*>(dO); a.stats = stats;
    a.dQ = reinterpret_cast<bf16_t*>(dQ); a.lddq = lddq; a.dq_bs = dq_batch_stride;
    a.dK = reinterpret_cast<bf16_t*>(dK); a.lddk = lddk; a.dV = reinterpret_cast<bf16_t*>(dV); a.lddv = lddv; a.dkv_bs = dkv_batch_stride;
    a.B = B; a.H = H; a.Nq = Nq; a.Nk = Nk; a.scale = 1.0f / sqrtf((float)head_dim);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return head_dim >= 32 ? ldt_attn_bwd_launch(&a, head_dim, s) : ldt_attn_bwd_narrow_launch(&a, head_dim, s);
}
