// The fp32 linear (ldt_sgemm):  C[M,N] = act_out( act_in(A[M,K]) · B[N,K]^T + bias[N] ), output fp32 or bf16.  For the small fp32-critical
// linears: time MLP (layers.py:17), AdaLN tables (layers.py:172,238), convs with K<=64, MiniPointnet, prior heads.  This file holds
//   sgemm_nt_kernel     the scalar-FMA form: 64x64 tile, BK=16, 4x4 outputs per thread
//   ldt_sgemm_decide    THE dispatch rule over the seven kernel forms (the other six: sgemm_mfma.hip, skinny_linear.hip)
//   ldt_sgemm_launch    operand checks + the launch of the route decided (second caller: the sampling loop's per-step AdaLN rows, api.hip)
//   ldt_sgemm, ldt_sgemm_route    the C-ABI entries (include/ldt_hip.h)
#include <stdlib.h>

#include "../../include/ldt_hip.h"
#include "kernels.h"

__global__ __launch_bounds__(256) void sgemm_nt_kernel(const SgemmArgs a) {
    __shared__ float As[16][68];
    __shared__ float Bs[16][68];
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    float acc[4][4] = {};
    const int lr = tid >> 2, lk = (tid & 3) * 4;
    // each thread stages 4 consecutive k of one A row and one B row: one 16-B load each when the rows allow it
    const bool vec = (a.lda % 4 == 0) && (a.ldb % 4 == 0) && (a.K % 4 == 0) && ldt_aligned16(a.A) && ldt_aligned16(a.B);
    for (int k0 = 0; k0 < a.K; k0 += 16) {
        const int m = m0 + lr, n = n0 + lr, kk = k0 + lk;
        f32x4 va4 = {0.f, 0.f, 0.f, 0.f}, vb4 = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            if (m < a.M && kk < a.K) va4 = *reinterpret_cast<const f32x4*>(a.A + (long)m * a.lda + kk);
            if (n < a.N && kk < a.K) vb4 = *reinterpret_cast<const f32x4*>(a.B + (long)n * a.ldb + kk);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (m < a.M && kk + j < a.K) va4[j] = a.A[(long)m * a.lda + kk + j];
                if (n < a.N && kk + j < a.K) vb4[j] = a.B[(long)n * a.ldb + kk + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[lk + j][lr] = a.act_in ? ldt_act(va4[j], a.act_in) : va4[j];
            Bs[lk + j][lr] = vb4[j];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(&As[k][ty * 4]);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[k][tx * 4]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + ty * 4 + i;
        if (m >= a.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + tx * 4 + j;
            if (n >= a.N) continue;
            const float v = acc[i][j] + (a.bias ? a.bias[n] : 0.f);
            SGEMM_STORE(a, (long)m * a.ldc + n, ldt_act(v, a.act_out));
        }
    }
}
// The seven forms in the order they are tried (the rule is stated in include/ldt_hip.h at ldt_sgemm_route):
//   streaming forms (skinny_linear.hip), M >= 8192 only: small N (N <= 8, K % 4 == 0, 16-byte rows of A and B), then small K (K <= 8, N / 4 in
//   8..256 dividing 256, 16-byte rows of C and bias);  MFMA forms (sgemm_mfma.hip): K % 4 == 0, K >= 8, 16-byte rows of A and B, M N >= 4096,
//   32 x 128 tiles when M <= 48, else 128 x 128;  the scalar-FMA kernel above for everything else its grid can hold.
int ldt_sgemm_decide(int M, int N, int K, long lda, long ldb, long ldc, int misaligned) {
    static const bool no_mfma = getenv("LDT_SGEMM_VALU") != nullptr;      // tools/dbg A/B: force the scalar-FMA kernel
    static const bool no_skinny = getenv("LDT_SGEMM_SKINNY") && atoi(getenv("LDT_SGEMM_SKINNY")) == 0;
    if (M <= 0 || N <= 0 || K <= 0) return SGEMM_ROUTE_NONE;
    const bool rows_ab = K % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && !(misaligned & 3);      // 16-B loads of A and B rows
    if (!no_skinny && M >= 8192) {                                        // short problems: the tiled kernels are fine
        if (N <= 8 && rows_ab) return N <= 4 ? SGEMM_ROUTE_SMALLN_4 : SGEMM_ROUTE_SMALLN_8;
        const int nq = N / 4;
        if (K <= 8 && N % 4 == 0 && nq >= 8 && nq <= 256 && 256 % nq == 0 && ldc % 4 == 0 && !(misaligned & 12))   // 16-B loads of bias, 16-B / 8-B stores
            return K <= 4 ? SGEMM_ROUTE_SMALLK_4 : SGEMM_ROUTE_SMALLK_8;
    }
    if (!no_mfma && rows_ab && K >= 8 && (long)M * N >= 64 * 64) {        // (tiny problems: launch-bound either way, keep the simple kernel)
        if (M <= 48) return SGEMM_ROUTE_MFMA_32;
        if ((M + 127) / 128 < 65536) return SGEMM_ROUTE_MFMA_128;
    }
    return (M + 63) / 64 < 65536 ? SGEMM_ROUTE_NT : SGEMM_ROUTE_NONE;     // grid.y limit
}
int ldt_sgemm_launch(const SgemmArgs* a, hipStream_t s) {
    LDT_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, LDT_ESHAPE, "sgemm: empty problem");
    LDT_REQUIRE(a->A && a->B && a->C, LDT_EARG, "sgemm: null pointer");
    const int misaligned = (ldt_aligned16(a->A) ? 0 : 1) | (ldt_aligned16(a->B) ? 0 : 2) | (ldt_aligned16(a->C) ? 0 : 4) |
                           (!a->bias || ldt_aligned16(a->bias) ? 0 : 8);
    const int route = ldt_sgemm_decide(a->M, a->N, a->K, a->lda, a->ldb, a->ldc, misaligned);
    switch (route) {
        case SGEMM_ROUTE_SMALLN_4: case SGEMM_ROUTE_SMALLN_8: case SGEMM_ROUTE_SMALLK_4: case SGEMM_ROUTE_SMALLK_8:
            return ldt_skinny_linear_launch(a, route, s);
        case SGEMM_ROUTE_MFMA_128: case SGEMM_ROUTE_MFMA_32:
            return ldt_sgemm_mfma_launch(a, route, s);
        case SGEMM_ROUTE_NT: break;
        default: LDT_REQUIRE(false, LDT_ESHAPE, "sgemm: M too large for this kernel (M=%d)", a->M);
    }
    dim3 grid((a->N + 63) / 64, (a->M + 63) / 64), block(256);
    hipLaunchKernelGGL(sgemm_nt_kernel, grid, block, 0, s, *a);
    return ldt_check_launch("sgemm_nt");
}

extern "C" int ldt_sgemm(const float* A, int64_t lda, const float* Bw, int64_t ldb, const float* bias, void* C,
                         int64_t ldc, int32_t out_bf16, int32_t act_in, int32_t act_out, int32_t M, int32_t N,
                         int32_t K, void* stream) {
    SgemmArgs a{A, lda, Bw, ldb, bias, C, ldc, out_bf16, act_in, act_out, M, N, K};
    return ldt_sgemm_launch(&a, ldt_stream(stream));
}
extern "C" int ldt_sgemm_route(int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldb, int64_t ldc, int32_t misaligned) {
    return ldt_sgemm_decide(M, N, K, lda, ldb, ldc, misaligned);
}
