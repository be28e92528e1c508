// Attention forward for narrow heads, Dh = 8 or 16 (gfx950 / MI355X): the reference's hybrid config builds its Score with hidden 128 and
// 16 heads (model/layers.py:183-200 takes any C / num_heads).  Same contract as the kernels of attention.hip:
//   O[b,h] = softmax(Q[b,h] K[b,h]^T * Dh^-0.5) V[b,h],  bf16 row views of Q / K / V with head h at column h Dh, O = [B][H][Nq][Dh] (quirk Q1),
//   scores in fp32 from the bf16 operands, online softmax in fp32 (running maximum), weights rounded to bf16 before P V, fp32 sums,
//   normalised at the end; any Nq, Nk >= 1 (the keys are streamed, 32 per step); no atomics, no sum across workgroups.
//
// Decomposition: ONE WAVE per (sample, head, 16-query block), four such waves per workgroup, nothing shared between them: no LDS, no barrier.
//   S = Q K^T   one v_mfma_f32_16x16x32_bf16 per 16 keys with the K extent zero-padded: lane l = (lr = l & 15, lq = l >> 4) supplies
//               Q[q0 + lr][8 lq ..+7] and K[key lr][8 lq ..+7] where 8 lq < Dh and a zero fragment elsewhere, and receives S[query 4 lq + i][key lr].
//   softmax     a query row lies across the 16 lanes of one lq: its maximum is four lane exchanges per step, its sum stays a per-lane partial.
//   O += P V    NOT an MFMA.  In the layout above a lane holds the weights of ONE key for four queries, and that key's V slice is one (Dh 8) or
//               two (Dh 16) 16-byte loads in its natural row layout: 4 x Dh fused multiply-adds per key and lane into per-lane partial sums.
//               As an MFMA operand V would have to be transposed (the summed index must be the 8 contiguous elements of a lane) and P would
//               have to cross LDS; at 8 or 16 channels that costs more than the 64 / 128 FMAs per 32-key step it saves.
//   end         the 4 x Dh partials of the 16 lanes of an lq are summed by a halving exchange (4 steps, 15 Dh / 4 exchanges): each lane ends
//               with Dh / 4 adjacent channels of one query row, summed in a fixed order, and the wave stores its 16 x Dh block contiguously.
// The next step's K / V rows are requested before the current step is computed.  Rows and keys past the end re-read the last row (never out
// of bounds); their scores are -inf, so their weights are exactly 0.
#include "kernels.h"

template <int DH>
__global__ __launch_bounds__(256) void attn_fwd_narrow_kernel(const AttnArgs a, long units, int nqb) {
    constexpr int NC = DH / 8;                                          // 16-byte pieces of a head's slice of a row
    constexpr int NV = 4 * DH;                                          // partial outputs per lane: [4 queries][DH channels]
    const int lane = threadIdx.x & 63, lr = lane & 15, lq = lane >> 4;
    const long unit = (long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (unit >= units) return;                                          // whole wave; the waves of a workgroup share nothing
    const int qb = (int)(unit % nqb);
    const long bh = unit / nqb;
    const int b = (int)(bh / a.H), head = (int)(bh % a.H), q0 = qb * 16;
    const bf16_t* Qb = a.Q + (long)b * a.q_batch_stride + head * DH;
    const bf16_t* Kb = a.K + (long)b * a.kv_batch_stride + head * DH;
    const bf16_t* Vb = a.V + (long)b * a.kv_batch_stride + head * DH;
    const bool live = lq < NC;                                          // this lane's 8 channels of the K extent exist
    const int chunk = lq & (NC - 1);                                    // (the other lanes read a piece that exists and drop it)
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    bf16x8 qf;
    {
        const int qrow = min(q0 + lr, a.Nq - 1);
        const bf16x8 t = *reinterpret_cast<const bf16x8*>(Qb + (long)qrow * a.ldq + 8 * chunk);
        qf = live ? t : zero;
    }
    auto load_kv = [&](int j0, bf16x8 (&kf)[2], bf16x8 (&vf)[2][NC]) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int key = min(j0 + 16 * h + lr, a.Nk - 1);
            const bf16x8 t = *reinterpret_cast<const bf16x8*>(Kb + (long)key * a.ldk + 8 * chunk);
            kf[h] = live ? t : zero;
#pragma unroll
            for (int c = 0; c < NC; ++c) vf[h][c] = *reinterpret_cast<const bf16x8*>(Vb + (long)key * a.ldv + 8 * c);
        }
    };

    float o[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) o[n] = 0.f;
    float m_run[4], l_run[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { m_run[i] = -INFINITY; l_run[i] = 0.f; }
    const float c = a.scale_log2e;

    bf16x8 kf[2], vf[2][NC];
    load_kv(0, kf, vf);
    for (int j0 = 0; j0 < a.Nk; j0 += 32) {
        bf16x8 kn[2], vn[2][NC];
        const bool more = j0 + 32 < a.Nk;                               // wave-uniform
        if (more) load_kv(j0 + 32, kn, vn);
        f32x4 s[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            s[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf[h], (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            const bool in = j0 + 16 * h + lr < a.Nk;
#pragma unroll
            for (int i = 0; i < 4; ++i) s[h][i] = in ? s[h][i] * c : -INFINITY;
        }
        float alpha[4], p[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float mx = fmaxf(s[0][i], s[1][i]);
#pragma unroll
            for (int x = 8; x > 0; x >>= 1) mx = fmaxf(mx, __shfl_xor(mx, x, 64));
            const float m_new = fmaxf(m_run[i], mx);                    // finite: key j0 exists
            alpha[i] = __builtin_amdgcn_exp2f(m_run[i] - m_new);        // first step: 2^-inf = 0
            m_run[i] = m_new;
            const float p0 = __builtin_amdgcn_exp2f(s[0][i] - m_new), p1 = __builtin_amdgcn_exp2f(s[1][i] - m_new);
            l_run[i] = l_run[i] * alpha[i] + (p0 + p1);
            p[0][i] = (float)(bf16_t)p0;                                // the weights P V sees are bf16
            p[1][i] = (float)(bf16_t)p1;
        }
#pragma unroll
        for (int cc = 0; cc < DH; ++cc) {
            const float v0 = (float)vf[0][cc >> 3][cc & 7], v1 = (float)vf[1][cc >> 3][cc & 7];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i * DH + cc] = fmaf(p[1][i], v1, fmaf(p[0][i], v0, o[i * DH + cc] * alpha[i]));
        }
        if (more) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                kf[h] = kn[h];
#pragma unroll
                for (int cN = 0; cN < NC; ++cN) vf[h][cN] = vn[h][cN];
            }
        }
    }

    // row sums: every lane of an lq gets the same bits (a + b = b + a at each level)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int x = 8; x > 0; x >>= 1) l_run[i] += __shfl_xor(l_run[i], x, 64);
    // o[i * DH + cc] over the 16 lanes: after the four halvings this lane holds indices base .. base + DH / 4 - 1,
    // base = bit3 * 2 DH + bit2 * DH + bit1 * DH / 2 + bit0 * DH / 4 of lr: query row i = 2 bit3 + bit2, channels from bit1 * DH / 2 + bit0 * DH / 4
    narrow_halve<NV, 8>(o, lr);
    narrow_halve<NV / 2, 4>(o, lr);
    narrow_halve<NV / 4, 2>(o, lr);
    narrow_halve<NV / 8, 1>(o, lr);
    const int i = lr >> 2, c0 = ((lr >> 1) & 1) * (DH / 2) + (lr & 1) * (DH / 4);
    const float l01 = (i & 1) ? l_run[1] : l_run[0], l23 = (i & 1) ? l_run[3] : l_run[2];
    const float inv = 1.0f / ((i & 2) ? l23 : l01);
    const int row = q0 + 4 * lq + i;
    if (row < a.Nq) {
        bf16_t* op = a.O + ((bh * a.Nq + row) * DH + c0);
        if constexpr (DH == 8) {
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
            *reinterpret_cast<bf16x2*>(op) = (bf16x2){(bf16_t)(o[0] * inv), (bf16_t)(o[1] * inv)};
        } else {
            *reinterpret_cast<bf16x4*>(op) = (bf16x4){(bf16_t)(o[0] * inv), (bf16_t)(o[1] * inv), (bf16_t)(o[2] * inv), (bf16_t)(o[3] * inv)};
        }
    }
}

int ldt_attn_narrow_launch(const AttnArgs* a, int dh, hipStream_t s) {
    LDT_REQUIRE(dh == 8 || dh == 16, LDT_ESHAPE, "attention (narrow): head dim %d is not 8 or 16", dh);
    const int nqb = (a->Nq + 15) / 16;
    const long units = (long)a->B * a->H * nqb, grid = (units + 3) / 4;
    LDT_REQUIRE(grid < (1L << 31), LDT_ESHAPE, "attention: grid too large");
    if (dh == 8) hipLaunchKernelGGL(attn_fwd_narrow_kernel<8>, dim3((unsigned)grid), dim3(256), 0, s, *a, units, nqb);
    else hipLaunchKernelGGL(attn_fwd_narrow_kernel<16>, dim3((unsigned)grid), dim3(256), 0, s, *a, units, nqb);
    return ldt_check_launch("attn_fwd_narrow");
}
