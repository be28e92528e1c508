// Backward pieces of a Score training step that are not GEMMs (gfx950): the transposing cast that feeds dgrad / wgrad to the NT GEMM route,
// the bias-gradient column sum, and the backward of LayerNorm + modulate, GELU(erf), the gated residual, SiLU, the denoising loss and the
// label embedding.  All are streaming kernels next to the GEMMs of the step; what they share:
//   * no atomics: every sum over rows (tokens of a sample, rows of a batch) has a fixed order — RED_SLICES interleaved row slices per
//     column, each summed front to back, then the slices added in index order — so two runs of one input give the same bits;
//   * the column sums are carried in float64 and rounded to fp32 once (as ldt_nelbo_terms does): they run over up to 10^4 rows;
//   * element arithmetic is fp32, row statistics are recomputed from the saved fp32 x exactly as ldt_layernorm_modulate forms them.
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define RED_COLS 64                  // columns per workgroup of a column reduction (one 256-byte fp32 line per row)
#define RED_SLICES 16                // row slices per column: rows s, s + 16, ... belong to slice s
#define RED_WG (RED_COLS * RED_SLICES)

__device__ __forceinline__ float ld_elem(const void* p, int is_bf16, long i) {
    return is_bf16 ? (float)reinterpret_cast<const bf16_t*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}

// the slices of one column added in index order; valid where threadIdx.y == 0
__device__ __forceinline__ double slices_sum_fixed(double v, double (*part)[RED_COLS]) {
    part[threadIdx.y][threadIdx.x] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.y == 0)
        for (int k = 0; k < RED_SLICES; ++k) s += part[k][threadIdx.x];
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------------------------------------
// transposing cast: src fp32 | bf16 [R][C] (ld_src) -> dst bf16 [C][R_pad] (ld_dst), columns R .. R_pad - 1 zero.  32 x 32 tiles through LDS.
__global__ __launch_bounds__(256) void transpose_cast_kernel(const void* __restrict__ src, int src_bf16, long ld_src, bf16_t* __restrict__ dst,
                                                             long ld_dst, long R, int C, long R_pad) {
    __shared__ float tile[32][33];
    const long r0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;        // 32 x 8
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long r = r0 + ty + 8 * k;
        const int c = c0 + tx;
        tile[ty + 8 * k][tx] = (r < R && c < C) ? ld_elem(src, src_bf16, r * ld_src + c) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = c0 + ty + 8 * k;
        const long r = r0 + tx;
        if (c < C && r < R_pad) dst[(long)c * ld_dst + r] = (bf16_t)tile[tx][ty + 8 * k];
    }
}

extern "C" int ldt_transpose_cast_bf16(const void* src, int32_t src_bf16, int64_t ld_src, uint16_t* dst, int64_t ld_dst, int64_t R, int32_t C,
                                       int64_t R_pad, void* stream) {
    LDT_REQUIRE(src && dst, LDT_EARG, "transpose_cast: null pointer");
    LDT_REQUIRE(R > 0 && C > 0 && R_pad >= R && ld_src >= C && ld_dst >= R_pad && (R_pad + 31) / 32 <= 0x7fffffffL && (C + 31) / 32 <= 65535,
                LDT_ESHAPE, "transpose_cast: R %ld, C %d, R_pad %ld, ld_src %ld, ld_dst %ld", (long)R, C, (long)R_pad, (long)ld_src, (long)ld_dst);
    hipLaunchKernelGGL(transpose_cast_kernel, dim3((unsigned)((R_pad + 31) / 32), (unsigned)((C + 31) / 32)), dim3(256), 0,
                       ldt_stream(stream), src, src_bf16, (long)ld_src, reinterpret_cast<bf16_t*>(dst), (long)ld_dst, (long)R, C,
                       (long)R_pad);
    return ldt_check_launch("transpose_cast");
}

// ------------------------------------------------------------------------------------------------
// bias gradient: out[c] = sum over the M rows of dy[m][c]
__global__ __launch_bounds__(RED_WG) void colsum_kernel(const void* __restrict__ dy, int dy_bf16, long ld, long M, int C, float* __restrict__ out) {
    __shared__ double part[RED_SLICES][RED_COLS];
    const int c = blockIdx.x * RED_COLS + threadIdx.x;
    double acc = 0.0;
    if (c < C)
        for (long m = threadIdx.y; m < M; m += RED_SLICES) acc += (double)ld_elem(dy, dy_bf16, m * ld + c);
    const double s = slices_sum_fixed(acc, part);
    if (threadIdx.y == 0 && c < C) out[c] = (float)s;
}

extern "C" int ldt_colsum(const void* dy, int32_t dy_bf16, int64_t ld, int64_t M, int32_t C, float* out, void* stream) {
    LDT_REQUIRE(dy && out, LDT_EARG, "colsum: null pointer");
    LDT_REQUIRE(M > 0 && C > 0 && ld >= C, LDT_ESHAPE, "colsum: M %ld, C %d, ld %ld", (long)M, C, (long)ld);
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)((C + RED_COLS - 1) / RED_COLS)), dim3(RED_COLS, RED_SLICES), 0,
                       ldt_stream(stream), dy, dy_bf16, (long)ld, (long)M, C, out);
    return ldt_check_launch("colsum");
}

// ------------------------------------------------------------------------------------------------
// LayerNorm(eps 1e-6, no affine) + modulate backward.  Forward (tools/utils.py:127-133, model/layers.py:136-137):
//     xh = (x - mean) * rstd,  y = xh * (1 + scale[s]) + shift[s]
// Backward with g = dy * (1 + scale[s]):  dx = rstd * (g - mean_c(g) - xh * mean_c(g * xh)),  dshift[s] = sum_rows dy,  dscale[s] = sum_rows dy * xh.
// Row kernel: one wave per row, dx is ADDED into the residual-stream gradient, (mean, rstd) go to stats[M][2] for the column kernel.
__global__ __launch_bounds__(256) void ln_mod_bwd_rows_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ dy, long lddy,
                                                              const float* __restrict__ scale, long mod_sample_stride, int rows_per_sample,
                                                              float* __restrict__ dx, long lddx, float* __restrict__ stats, long M, int C) {
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + row * ldx;
    const float* gr = dy + row * lddy;
    const float* sc = scale ? scale + (row / rows_per_sample) * mod_sample_stride : nullptr;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c];
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + 1e-6f);
    float sg = 0.f, sgx = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float g = gr[c] * (1.f + (sc ? sc[c] : 0.f));
        sg += g;
        sgx += g * ((xr[c] - mean) * rstd);
    }
    const float mg = wave_sum(sg) / (float)C, mgx = wave_sum(sgx) / (float)C;
    float* dr = dx + row * lddx;
    for (int c = lane; c < C; c += 64) {
        const float g = gr[c] * (1.f + (sc ? sc[c] : 0.f));
        const float xh = (xr[c] - mean) * rstd;
        dr[c] += rstd * ((g - mg) - xh * mgx);
    }
    if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}
// Column kernel: grid (column chunks, samples)
__global__ __launch_bounds__(RED_WG) void ln_mod_bwd_cols_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ dy, long lddy,
                                                                 const float* __restrict__ stats, int rows_per_sample, int C,
                                                                 float* __restrict__ dshift, float* __restrict__ dscale, long dmod_sample_stride) {
    __shared__ double part[RED_SLICES][RED_COLS];
    const int c = blockIdx.x * RED_COLS + threadIdx.x;
    const long row0 = (long)blockIdx.y * rows_per_sample;
    double a_sh = 0.0, a_sc = 0.0;
    if (c < C)
        for (int t = threadIdx.y; t < rows_per_sample; t += RED_SLICES) {
            const long row = row0 + t;
            const float g = dy[row * lddy + c];
            const float xh = (x[row * ldx + c] - stats[2 * row]) * stats[2 * row + 1];
            a_sh += (double)g;
            a_sc += (double)(g * xh);
        }
    const double s_sh = slices_sum_fixed(a_sh, part);
    const double s_sc = slices_sum_fixed(a_sc, part);
    if (threadIdx.y == 0 && c < C) {
        dshift[(long)blockIdx.y * dmod_sample_stride + c] = (float)s_sh;
        dscale[(long)blockIdx.y * dmod_sample_stride + c] = (float)s_sc;
    }
}

extern "C" int ldt_layernorm_modulate_bwd(const float* x, int64_t ldx, const float* dy, int64_t lddy, const float* scale, int64_t mod_sample_stride,
                                          int32_t rows_per_sample, float* dx, int64_t lddx, float* dshift, float* dscale,
                                          int64_t dmod_sample_stride, float* stats, int64_t M, int32_t C, void* stream) {
    LDT_REQUIRE(x && dy && dx && stats, LDT_EARG, "layernorm_modulate_bwd: null pointer (stats[M][2] is the row kernel's output and is required)");
    LDT_REQUIRE((dshift == nullptr) == (dscale == nullptr), LDT_EARG, "layernorm_modulate_bwd: dshift and dscale go together");
    LDT_REQUIRE(M > 0 && C > 0 && rows_per_sample > 0 && M % rows_per_sample == 0 && M / rows_per_sample <= 65535 && ldx >= C && lddy >= C && lddx >= C &&
                (!dshift || dmod_sample_stride >= C), LDT_ESHAPE, "layernorm_modulate_bwd: M %ld, C %d, rows_per_sample %d", (long)M, C, rows_per_sample);
    hipStream_t s = ldt_stream(stream);
    hipLaunchKernelGGL(ln_mod_bwd_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, (long)ldx, dy, (long)lddy, scale,
                       (long)mod_sample_stride, rows_per_sample, dx, (long)lddx, stats, (long)M, C);
    int rc = ldt_check_launch("layernorm_modulate_bwd (rows)");
    if (rc != LDT_OK || !dshift) return rc;
    hipLaunchKernelGGL(ln_mod_bwd_cols_kernel, dim3((unsigned)((C + RED_COLS - 1) / RED_COLS), (unsigned)(M / rows_per_sample)), dim3(RED_COLS, RED_SLICES),
                       0, s, x, (long)ldx, dy, (long)lddy, stats, rows_per_sample, C, dshift, dscale, (long)dmod_sample_stride);
    return ldt_check_launch("layernorm_modulate_bwd (columns)");
}

// ------------------------------------------------------------------------------------------------
// GELU(erf) backward on the saved bf16 pre-activation u (model/layers.py:111-113,127-129): du = dh * (Phi(u) + u phi(u)) -> bf16, the operand of
// the dgrad / wgrad GEMMs of mlp.fc.
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const bf16_t* __restrict__ u, long ldu, const void* __restrict__ dh, int dh_bf16, long lddh,
                                                       bf16_t* __restrict__ du, long lddu, long M, int C) {
    const long total = M * (long)C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / C;
        const int c = (int)(i % C);
        const float v = (float)u[m * ldu + c];
        const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752440f));
        const float pdf = 0.39894228040143267794f * expf(-0.5f * v * v);
        du[m * lddu + c] = (bf16_t)(ld_elem(dh, dh_bf16, m * lddh + c) * (cdf + v * pdf));
    }
}

extern "C" int ldt_gelu_bwd(const uint16_t* u, int64_t ldu, const void* dh, int32_t dh_bf16, int64_t lddh, uint16_t* du, int64_t lddu, int64_t M,
                            int32_t C, void* stream) {
    LDT_REQUIRE(u && dh && du, LDT_EARG, "gelu_bwd: null pointer");
    LDT_REQUIRE(M > 0 && C > 0 && ldu >= C && lddh >= C && lddu >= C, LDT_ESHAPE, "gelu_bwd: M %ld, C %d", (long)M, C);
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(ldt_grid_1d(M * (long)C, 256, 4096)), dim3(256), 0, ldt_stream(stream),
                       reinterpret_cast<const bf16_t*>(u), (long)ldu, dh, dh_bf16, (long)lddh, reinterpret_cast<bf16_t*>(du), (long)lddu, (long)M, C);
    return ldt_check_launch("gelu_bwd");
}

// ------------------------------------------------------------------------------------------------
// gated residual backward (model/layers.py:218-219, y = x + gate[s] * a): da = dy * gate[s] -> bf16 (operand of the GEMMs of fc_o / mlp.out),
// dgate[s] = sum over sample s's rows of dy * a.  dx = dy needs no kernel: the residual-stream gradient stays where it is.
__global__ __launch_bounds__(RED_WG) void gate_bwd_kernel(const float* __restrict__ dy, long lddy, const void* __restrict__ a, int a_bf16, long lda,
                                                          const float* __restrict__ gate, long gate_sample_stride, int rows_per_sample, int C,
                                                          bf16_t* __restrict__ da, long ldda, float* __restrict__ dgate, long dgate_sample_stride) {
    __shared__ double part[RED_SLICES][RED_COLS];
    const int c = blockIdx.x * RED_COLS + threadIdx.x;
    const long row0 = (long)blockIdx.y * rows_per_sample;
    double acc = 0.0;
    if (c < C) {
        const float g = gate[(long)blockIdx.y * gate_sample_stride + c];
        for (int t = threadIdx.y; t < rows_per_sample; t += RED_SLICES) {
            const long row = row0 + t;
            const float d = dy[row * lddy + c];
            da[row * ldda + c] = (bf16_t)(d * g);
            if (dgate) acc += (double)(d * ld_elem(a, a_bf16, row * lda + c));
        }
    }
    const double s = slices_sum_fixed(acc, part);
    if (dgate && threadIdx.y == 0 && c < C) dgate[(long)blockIdx.y * dgate_sample_stride + c] = (float)s;
}

extern "C" int ldt_gate_residual_bwd(const float* dy, int64_t lddy, const void* a, int32_t a_bf16, int64_t lda, const float* gate,
                                     int64_t gate_sample_stride, int32_t rows_per_sample, uint16_t* da, int64_t ldda, float* dgate,
                                     int64_t dgate_sample_stride, int64_t M, int32_t C, void* stream) {
    LDT_REQUIRE(dy && gate && da && (a || !dgate), LDT_EARG, "gate_residual_bwd: null pointer (dgate needs the branch output a)");
    LDT_REQUIRE(M > 0 && C > 0 && rows_per_sample > 0 && M % rows_per_sample == 0 && M / rows_per_sample <= 65535 && lddy >= C && ldda >= C &&
                (!dgate || (lda >= C && dgate_sample_stride >= C)), LDT_ESHAPE, "gate_residual_bwd: M %ld, C %d, rows_per_sample %d", (long)M, C,
                rows_per_sample);
    hipLaunchKernelGGL(gate_bwd_kernel, dim3((unsigned)((C + RED_COLS - 1) / RED_COLS), (unsigned)(M / rows_per_sample)), dim3(RED_COLS, RED_SLICES), 0,
                       ldt_stream(stream), dy, (long)lddy, a, a_bf16, (long)lda, gate, (long)gate_sample_stride, rows_per_sample, C,
                       reinterpret_cast<bf16_t*>(da), (long)ldda, dgate, (long)dgate_sample_stride);
    return ldt_check_launch("gate_residual_bwd");
}

// ------------------------------------------------------------------------------------------------
// SiLU backward (adaLN_modulation.0, model/layers.py:171,237; TimeEmbedding.mlp.1, :17): dc = dy * sig(c) * (1 + c * (1 - sig(c))), fp32, and
// (optionally) act = SiLU(c) itself: the forward fuses it into the next linear's operand read, the weight gradient of that linear needs it.
__global__ __launch_bounds__(256) void silu_bwd_kernel(const float* __restrict__ c, const float* __restrict__ dy, float* __restrict__ dc,
                                                       float* __restrict__ act, long n) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = c[i];
        const float sg = 1.f / (1.f + expf(-v));
        if (dc) dc[i] = dy[i] * (sg * (1.f + v * (1.f - sg)));
        if (act) act[i] = silu(v);
    }
}

extern "C" int ldt_silu_bwd(const float* c, const float* dy, float* dc, float* act, int64_t n, void* stream) {
    LDT_REQUIRE(c && (dc || act) && (dy || !dc), LDT_EARG, "silu_bwd: null pointer (dc needs dy; one of dc, act is required)");
    LDT_REQUIRE(n > 0, LDT_ESHAPE, "silu_bwd: n %ld", (long)n);
    hipLaunchKernelGGL(silu_bwd_kernel, dim3(ldt_grid_1d(n, 256, 2048)), dim3(256), 0, ldt_stream(stream), c, dy, dc, act, (long)n);
    return ldt_check_launch("silu_bwd");
}

// ------------------------------------------------------------------------------------------------
// denoising-loss backward (trainer/Latent_SDE_Trainer.py:131-137): loss = mean over all n = B * per_sample elements of dist * weight[b],
// dist = (eta - params)^2 or |eta - params|  =>  dparams = -2 (eta - params) weight[b] / n   or   -sign(eta - params) weight[b] / n.
__global__ __launch_bounds__(256) void dsm_bwd_kernel(const float* __restrict__ eta, const float* __restrict__ params, const float* __restrict__ weight,
                                                      long per_sample, long n, int l1, float* __restrict__ dparams) {
    const float inv_n = 1.f / (float)n;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float w = weight ? weight[i / per_sample] : 1.f;
        const float d = eta[i] - params[i];
        const float dd = l1 ? (d > 0.f ? -1.f : (d < 0.f ? 1.f : 0.f)) : -2.f * d;
        dparams[i] = dd * w * inv_n;
    }
}

extern "C" int ldt_dsm_loss_bwd(const float* eta, const float* params, const float* weight, int64_t B, int64_t per_sample, int32_t l1, float* dparams,
                                void* stream) {
    LDT_REQUIRE(eta && params && dparams, LDT_EARG, "dsm_loss_bwd: null pointer");
    LDT_REQUIRE(B > 0 && per_sample > 0, LDT_ESHAPE, "dsm_loss_bwd: B %ld, per_sample %ld", (long)B, (long)per_sample);
    const long n = B * per_sample;
    hipLaunchKernelGGL(dsm_bwd_kernel, dim3(ldt_grid_1d(n, 256, 2048)), dim3(256), 0, ldt_stream(stream), eta, params, weight, (long)per_sample,
                       n, l1, dparams);
    return ldt_check_launch("dsm_loss_bwd");
}

// ------------------------------------------------------------------------------------------------
// label-embedding gradient (nn.Embedding, model/scorenet/score.py:125-128): dE[k][:] = sum over the samples b with label[b] == k of dc[b][:], in
// the order of b.  One thread per (class, column); classes nobody carries get zero rows.
__global__ __launch_bounds__(256) void embedding_grad_kernel(const float* __restrict__ dc, long ld, const int* __restrict__ label, int B, int D,
                                                             float* __restrict__ dE) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= D) return;
    const int k = blockIdx.y;
    float acc = 0.f;
    for (int b = 0; b < B; ++b)
        if (label[b] == k) acc += dc[(long)b * ld + d];
    dE[(long)k * D + d] = acc;
}

extern "C" int ldt_embedding_grad(const float* dc, int64_t ld, const int32_t* label, int32_t B, int32_t D, int32_t n_classes, float* dE, void* stream) {
    LDT_REQUIRE(dc && label && dE, LDT_EARG, "embedding_grad: null pointer");
    LDT_REQUIRE(B > 0 && D > 0 && n_classes > 0 && n_classes <= 65535 && ld >= D, LDT_ESHAPE, "embedding_grad: B %d, D %d, classes %d", B, D, n_classes);
    hipLaunchKernelGGL(embedding_grad_kernel, dim3((unsigned)((D + 255) / 256), (unsigned)n_classes), dim3(256), 0, ldt_stream(stream),
                       dc, (long)ld, label, B, D, dE);
    return ldt_check_launch("embedding_grad");
}

// Backward of a set's learned prior rows (Compressor/layers.py:26-42 InitialSet: every sample starts from the same rows, all of them or, under a
// keep_mask, its kept ones packed to the front): dprior[r] = sum over the samples that hold row r of do[b N + src[b][r]], in the order of b.
// src[b][r] = the row of sample b that prior row r became, -1 = absent; an index outside [0, N) is taken as absent, never read.
__global__ __launch_bounds__(256) void rows_gather_sum_kernel(const float* __restrict__ dy, long ld, const int* __restrict__ src, int B, int N, int R,
                                                              int C, float* __restrict__ dprior) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int r = blockIdx.y;
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
        const int s = src[(long)b * R + r];
        if (s >= 0 && s < N) acc += dy[((long)b * N + s) * ld + c];
    }
    dprior[(long)r * C + c] = acc;
}

extern "C" int ldt_rows_gather_sum(const float* dy, int64_t ld, const int32_t* src, int32_t B, int32_t N, int32_t R, int32_t C, float* dprior,
                                   void* stream) {
    LDT_REQUIRE(dy && src && dprior, LDT_EARG, "rows_gather_sum: null pointer");
    LDT_REQUIRE(B > 0 && N > 0 && R > 0 && R <= 65535 && C > 0 && ld >= C, LDT_ESHAPE, "rows_gather_sum: B %d, N %d, R %d (1 .. 65535), C %d, ld %ld",
                B, N, R, C, (long)ld);
    hipLaunchKernelGGL(rows_gather_sum_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)R), dim3(256), 0, ldt_stream(stream),
                       dy, (long)ld, src, B, N, R, C, dprior);
    return ldt_check_launch("rows_gather_sum");
}
