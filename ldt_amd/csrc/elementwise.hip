// HBM-bound row and element kernels of the LDT hot path (gfx950), coalesced 16 B per lane where the shape allows (guide G13):
//   cast_pad           fp32 -> bf16 with zero K-padding (ldt_cast_pad_bf16; the Score forward's first launch)
//   ln_mod_*           LayerNorm + AdaLN modulate -> bf16 (ldt_layernorm_modulate; the Score forward's LayerNorms)
//   sinusoid           sinusoidal time embedding (ldt_sinusoid)
//   cond_rows          per-step AdaLN condition rows (the sampling loop)
//   group_stats, norm_apply    GroupNorm statistics and the normalise / affine / modulate pass (ldt_group_stats, ldt_norm_apply)
//   block_act, add_f32, widen_bf16    element passes (ldt_block_activation, ldt_add_f32, ldt_widen_bf16)
//   fold_mean_ratio, fold_monitor     the LN-fold monitor over the folded GEMMs' row statistics (ldt_fold_mean_ratio; the Score forward)
#include "../../include/ldt_hip.h"
#include "kernels.h"

// ------------------------------------------------------------------------------------------------
// cast fp32 [rows][cols] (ld = lds) -> bf16 [rows][cols_pad] with zero padding (K padding for MFMA GEMM)
__global__ void cast_pad_kernel(const float* __restrict__ src, long lds, bf16_t* __restrict__ dst, long ldd,
                                long rows, int cols, int cols_pad) {
    const long total = rows * (long)(cols_pad / 4);
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / (cols_pad / 4);
        const int c = (int)(i % (cols_pad / 4)) * 4;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (c + j < cols) ? src[r * lds + c + j] : 0.f;
        bf16x4 pk = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
        *reinterpret_cast<bf16x4*>(dst + r * ldd + c) = pk;
    }
}

int ldt_cast_pad_launch(const float* src, long lds, bf16_t* dst, long ldd, long rows, int cols,
                                   int cols_pad, hipStream_t s) {
    LDT_REQUIRE(rows > 0 && cols > 0 && cols_pad >= cols && cols_pad % 4 == 0 && ldd % 4 == 0, LDT_ESHAPE,
                "cast_pad: bad shape rows=%ld cols=%d cols_pad=%d ldd=%ld", rows, cols, cols_pad, ldd);
    LDT_REQUIRE((reinterpret_cast<uintptr_t>(dst) & 7) == 0, LDT_EALIGN, "cast_pad: dst must be 8-byte aligned");
    const long total = rows * (long)(cols_pad / 4);
    hipLaunchKernelGGL(cast_pad_kernel, dim3(ldt_grid_1d(total, 256, 2048)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols, cols_pad);
    return ldt_check_launch("cast_pad");
}
extern "C" int ldt_cast_pad_bf16(const float* src, int64_t ld_src, uint16_t* dst, int64_t ld_dst, int64_t rows,
                                 int32_t cols, int32_t cols_pad, void* stream) {
    LDT_REQUIRE(src && dst, LDT_EARG, "cast_pad: null pointer");
    return ldt_cast_pad_launch(src, ld_src, ldt_bf16_mut(dst), ld_dst, rows, cols, cols_pad, ldt_stream(stream));
}

// ------------------------------------------------------------------------------------------------
// LayerNorm(eps=1e-6, biased var, over C) [* w + b] then modulate: y = ln * (1 + scale) + shift  -> bf16
//   reference: tools/utils.py:127-133 (LayerNorm wrapper), model/layers.py:136-137 (modulate), :218-219 (use)
// One wave per row; shift/scale are per-sample vectors (stride 0 = shared by the batch, the
// unconditional sampler's case: SURVEY hard part 3) selected by a device-side step counter.
template <int NV>   // NV float4 chunks per lane: C = NV*256
__global__ __launch_bounds__(256) void ln_mod_vec_kernel(const LnArgs a) {
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (row >= a.M) return;
    const float* xr = a.x + row * a.ldx;
    const long modoff = a.shift ? (a.step_ptr ? (long)(*a.step_ptr) * a.mod_step_stride : 0) + (row / a.rows_per_sample) * a.mod_sample_stride : 0;
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + lane * 4;
        v[i] = *reinterpret_cast<const f32x4*>(xr + c);
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    const float mean = wave_sum(s) / (float)a.C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / (float)a.C + 1e-6f);
    const float* sh = a.shift; const float* sc = a.scale;
    if (sh) { sh += modoff; sc += modoff; }
    bf16_t* yr = a.y + row * a.ldy;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + lane * 4;
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd;
        if (a.w) { const f32x4 w = *reinterpret_cast<const f32x4*>(a.w + c); const f32x4 b = *reinterpret_cast<const f32x4*>(a.b + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = o[j] * w[j] + b[j]; }
        if (sh) { const f32x4 h = *reinterpret_cast<const f32x4*>(sh + c); const f32x4 g = *reinterpret_cast<const f32x4*>(sc + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = o[j] * (1.f + g[j]) + h[j]; }
        bf16x4 pk = {(bf16_t)o[0], (bf16_t)o[1], (bf16_t)o[2], (bf16_t)o[3]};
        *reinterpret_cast<bf16x4*>(yr + c) = pk;
    }
}

// generic C (any width): three passes over the (cache-resident) row
__global__ __launch_bounds__(256) void ln_mod_generic_kernel(const LnArgs a) {
    const int lane = threadIdx.x & 63;
    const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (row >= a.M) return;
    const float* xr = a.x + row * a.ldx;
    float s = 0.f;
    for (int c = lane; c < a.C; c += 64) s += xr[c];
    const float mean = wave_sum(s) / (float)a.C;
    float q = 0.f;
    for (int c = lane; c < a.C; c += 64) { const float d = xr[c] - mean; q += d * d; }
    const float rstd = rsqrtf(wave_sum(q) / (float)a.C + 1e-6f);
    const float* sh = a.shift; const float* sc = a.scale;
    if (sh) {
        const long off = (a.step_ptr ? (long)(*a.step_ptr) * a.mod_step_stride : 0) +
                         (row / a.rows_per_sample) * a.mod_sample_stride;
        sh += off; sc += off;
    }
    bf16_t* yr = a.y + row * a.ldy;
    for (int c = lane; c < a.C; c += 64) {
        float o = (xr[c] - mean) * rstd;
        if (a.w) o = o * a.w[c] + a.b[c];
        if (sh) o = o * (1.f + sc[c]) + sh[c];
        yr[c] = (bf16_t)o;
    }
}

int ldt_ln_launch(const LnArgs* a, hipStream_t s) {
    LDT_REQUIRE(a->M > 0 && a->C > 0, LDT_ESHAPE, "ln: empty problem");
    LDT_REQUIRE((a->shift == nullptr) == (a->scale == nullptr), LDT_EARG, "ln: shift and scale go together");
    LDT_REQUIRE((a->w == nullptr) == (a->b == nullptr), LDT_EARG, "ln: affine weight and bias go together");
    LDT_REQUIRE(!a->shift || a->rows_per_sample > 0, LDT_EARG, "ln: rows_per_sample must be > 0 with modulation");
    dim3 grid((unsigned)((a->M + 3) / 4)), block(256);
    const bool vec = (a->C % 256 == 0) && a->C <= 1024 && a->ldx % 4 == 0 && a->ldy % 4 == 0 && ldt_aligned16(a->x) &&
                     (reinterpret_cast<uintptr_t>(a->y) & 7) == 0 && (!a->shift || (ldt_aligned16(a->shift) && ldt_aligned16(a->scale) &&
                     a->mod_sample_stride % 4 == 0 && a->mod_step_stride % 4 == 0)) && (!a->w || (ldt_aligned16(a->w) && ldt_aligned16(a->b)));
    if (vec) {
        switch (a->C / 256) {
            case 1: hipLaunchKernelGGL(ln_mod_vec_kernel<1>, grid, block, 0, s, *a); break;
            case 2: hipLaunchKernelGGL(ln_mod_vec_kernel<2>, grid, block, 0, s, *a); break;
            case 3: hipLaunchKernelGGL(ln_mod_vec_kernel<3>, grid, block, 0, s, *a); break;
            default: hipLaunchKernelGGL(ln_mod_vec_kernel<4>, grid, block, 0, s, *a); break;
        }
    } else {
        hipLaunchKernelGGL(ln_mod_generic_kernel, grid, block, 0, s, *a);
    }
    return ldt_check_launch("ln_modulate");
}
extern "C" int ldt_layernorm_modulate(const float* x, int64_t ldx, uint16_t* y, int64_t ldy, const float* w,
                                      const float* b, const float* shift, const float* scale,
                                      int64_t mod_sample_stride, int32_t rows_per_sample, const int32_t* step_ptr,
                                      int64_t mod_step_stride, int64_t M, int32_t C, void* stream) {
    LDT_REQUIRE(x && y, LDT_EARG, "ln: null pointer");
    LnArgs a{x, ldx, ldt_bf16_mut(y), ldy, w, b, shift, scale, mod_sample_stride, rows_per_sample, step_ptr, mod_step_stride, M, C};
    return ldt_ln_launch(&a, ldt_stream(stream));
}

// ------------------------------------------------------------------------------------------------
// sinusoidal embedding of continuous t (model/layers.py:20-36): e[i] = [sin(t_i f_k), cos(t_i f_k)];
// the frequency table f is built on the host with the reference's own fp32 expression (quirk Q5).
__global__ void sinusoid_kernel(const float* __restrict__ t, const float* __restrict__ freq, float* __restrict__ e, int n, int half) {
    const int i = blockIdx.x;
    for (int k = threadIdx.x; k < half; k += blockDim.x) {
        const float a = __fmul_rn(t[i], freq[k]);
        e[(long)i * 2 * half + k] = sinf(a);
        e[(long)i * 2 * half + half + k] = cosf(a);
    }
}
extern "C" int ldt_sinusoid(const float* t, const float* freq, float* e, int32_t n, int32_t half, void* stream) {
    LDT_REQUIRE(t && freq && e, LDT_EARG, "sinusoid: null pointer");
    LDT_REQUIRE(n > 0 && half > 0, LDT_ESHAPE, "sinusoid: empty");
    hipLaunchKernelGGL(sinusoid_kernel, dim3(n), dim3(128), 0, ldt_stream(stream), t, freq, e, n, half);
    return ldt_check_launch("sinusoid");
}

// c[b][k] = silu?(temb[step][k] + extra[b][k])   (score.py:135: c = t_emb + l_emb | img condition; the SiLU that opens every AdaLN
// Sequential — model/layers.py:172 — is applied here once so that the row GEMM behind it can stream its A operand by LDS-DMA), step from the device counter
// `cb` (optional): the same rows rounded to bf16 — the A operand of the bf16-weight form of the row GEMM (ldt_cond_args.w_ada_bf16)
__global__ void cond_rows_kernel(const float* __restrict__ temb, const float* __restrict__ extra, float* __restrict__ c, bf16_t* __restrict__ cb,
                                 const int* __restrict__ step_ptr, int batch, int t_dim, int silu_out) {
    const int step = step_ptr ? *step_ptr : 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < batch * t_dim; i += gridDim.x * blockDim.x) {
        const int k = i % t_dim;
        const float v = temb[(long)step * t_dim + k] + (extra ? extra[i] : 0.f);
        const float o = silu_out ? silu(v) : v;
        c[i] = o;
        if (cb) cb[i] = (bf16_t)o;
    }
}
int ldt_cond_rows_launch(const float* temb, const float* extra, float* c, void* c_bf16, const int* step_ptr, int batch, int t_dim, int silu_out, hipStream_t s) {
    LDT_REQUIRE(temb && c && batch > 0 && t_dim > 0, LDT_EARG, "cond_rows: bad arguments");
    hipLaunchKernelGGL(cond_rows_kernel, dim3(ldt_grid_1d(batch * t_dim, 256, 1024)), dim3(256), 0, s, temb, extra, c, ldt_bf16_mut(c_bf16), step_ptr, batch, t_dim, silu_out);
    return ldt_check_launch("cond_rows");
}

// ------------------------------------------------------------------------------------------------- group norm / identity norm
// tools/utils.py:168-181 get_norm: `group_norm` -> nn.GroupNorm(min(C/4, 16), C, eps=1e-6) on the channels-first activations (statistics per
// sample and group over C/G channels x all tokens), `None` -> Identity.  Rows are token-major here: x[b*T + t][c].
__global__ void group_stats_kernel(const float* __restrict__ x, long ldx, int T, int C, int G, float eps, float* __restrict__ stats) {
    const int b = blockIdx.x / G, g = blockIdx.x % G, cg = C / G;
    const float* xb = x + (long)b * T * ldx + g * cg;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < T * cg; i += blockDim.x) {
        const float v = xb[(long)(i / cg) * ldx + i % cg];
        s1 += v; s2 += (double)v * v;
    }
    __shared__ double r1[256], r2[256];
    r1[threadIdx.x] = s1; r2[threadIdx.x] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { r1[threadIdx.x] += r1[threadIdx.x + o]; r2[threadIdx.x] += r2[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = (double)T * cg, mean = r1[0] / n;
        double var = r2[0] / n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        stats[(long)blockIdx.x * 2] = (float)mean;
        stats[(long)blockIdx.x * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}
extern "C" int ldt_group_stats(const float* x, int64_t ldx, int32_t B, int32_t T, int32_t C, int32_t G, float eps, float* stats, void* stream) {
    LDT_REQUIRE(x && stats && B > 0 && T > 0 && C > 0 && G > 0 && C % G == 0 && ldx >= C, LDT_EARG, "group_stats: bad argument (B=%d T=%d C=%d G=%d)", B, T, C, G);
    hipLaunchKernelGGL(group_stats_kernel, dim3((unsigned)(B * G)), dim3(256), 0, ldt_stream(stream), x, (long)ldx, T, C, G, eps, stats);
    return ldt_check_launch("group_stats");
}

__global__ void norm_apply_kernel(const float* __restrict__ x, long ldx, bf16_t* __restrict__ y, long ldy, long M, int C, const float* __restrict__ stats,
                                  int G, int rows_per_stat, const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ shift,
                                  const float* __restrict__ scale, long mod_sample_stride, int rows_per_sample) {
    const long n4 = M * (C / 4);
    const int cg = C / (G > 0 ? G : 1);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const long m = i / (C / 4);
        const int c = (int)(i % (C / 4)) * 4;
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + m * ldx + c);
        const long moff = (m / rows_per_sample) * mod_sample_stride + c;
        bf16x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float mean = 0.f, rstd = 1.f;
            if (stats) {
                const float* st = stats + ((m / rows_per_stat) * G + (c + j) / cg) * 2;
                mean = st[0]; rstd = st[1];
            }
            float h = (v[j] - mean) * rstd;
            if (w) h = h * w[c + j] + b[c + j];
            if (scale) h = h * (1.0f + scale[moff + j]) + shift[moff + j];
            o[j] = (bf16_t)h;
        }
        *reinterpret_cast<bf16x4*>(y + m * ldy + c) = o;
    }
}
extern "C" int ldt_norm_apply(const float* x, int64_t ldx, uint16_t* y, int64_t ldy, int64_t M, int32_t C, const float* stats, int32_t G,
                              int32_t rows_per_stat, const float* w, const float* b, const float* shift, const float* scale,
                              int64_t mod_sample_stride, int32_t rows_per_sample, void* stream) {
    LDT_REQUIRE(x && y && M > 0 && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0, LDT_EARG, "norm_apply: bad argument (M=%ld C=%d)", (long)M, C);
    LDT_REQUIRE(ldt_aligned16(x) && (reinterpret_cast<uintptr_t>(y) & 7u) == 0, LDT_EALIGN, "norm_apply: x must be 16-byte, y 8-byte aligned");
    LDT_REQUIRE(!stats || (G > 0 && C % G == 0 && rows_per_stat > 0), LDT_EARG, "norm_apply: statistics need G | C and rows_per_stat > 0");
    LDT_REQUIRE(!w == !b && !shift == !scale && rows_per_sample > 0, LDT_EARG, "norm_apply: w / b and shift / scale go in pairs; rows_per_sample > 0");
    hipLaunchKernelGGL(norm_apply_kernel, dim3(ldt_grid_1d(M * (C / 4), 256, 4096)), dim3(256), 0, ldt_stream(stream), x, (long)ldx, ldt_bf16_mut(y), (long)ldy,
                       (long)M, C, stats, stats ? G : 1, stats ? rows_per_stat : 1, w, b, shift, scale, (long)mod_sample_stride, rows_per_sample);
    return ldt_check_launch("norm_apply");
}

// ------------------------------------------------------------------------------------------------
// x = act(x) in place on bf16 rows [M][C] (row stride ld): the block activation of the reference's no-condition ResidualBlock branches
// (`decoder_act`, model/layers.py:224-226 via tools/utils.py:104-124), applied to the LayerNorm output the projections read.  kind = enum
// ldt_block_act; the arithmetic runs in fp32.  rrelu is its eval-mode form (slope (1/8 + 1/3) / 2).
__device__ __forceinline__ float block_act(float v, int kind) {
    switch (kind) {
        case LDT_BACT_GELU: return gelu_erf(v);
        case LDT_BACT_SILU: return silu(v);
        case LDT_BACT_RELU: return (v > 0.f || v != v) ? v : 0.f;      // (fmaxf would turn a NaN into 0: torch.relu keeps it)
        case LDT_BACT_LEAKY_001: return v > 0.f ? v : 0.01f * v;
        case LDT_BACT_LEAKY_02: return v > 0.f ? v : 0.2f * v;
        case LDT_BACT_RRELU_EVAL: return v > 0.f ? v : v * ((1.0f / 8.0f + 1.0f / 3.0f) * 0.5f);
        case LDT_BACT_HARDSWISH: return v * fminf(fmaxf(v + 3.0f, 0.f), 6.0f) * (1.0f / 6.0f);
        case LDT_BACT_SELU: return 1.0507009873554804934193349852946f * (v > 0.f ? v : 1.6732632423543772848170429916717f * (expf(v) - 1.0f));
        default: return v;
    }
}
__global__ __launch_bounds__(256) void block_act_kernel(bf16_t* __restrict__ x, long ld, long M, int C, int kind) {
    const long n = M * C;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        bf16_t* p = x + (i / C) * ld + (i % C);
        *p = (bf16_t)block_act((float)*p, kind);
    }
}
extern "C" int ldt_block_activation(uint16_t* x, int64_t ld, int64_t M, int32_t C, int32_t kind, void* stream) {
    LDT_REQUIRE(x && M > 0 && C > 0 && ld >= C, LDT_EARG, "block_activation: bad argument");
    LDT_REQUIRE(kind > LDT_BACT_NONE && kind <= LDT_BACT_SELU, LDT_EARG, "block_activation: unknown activation %d", kind);
    hipLaunchKernelGGL(block_act_kernel, dim3(ldt_grid_1d(M * C, 256, 4096)), dim3(256), 0, ldt_stream(stream),
                       ldt_bf16_mut(x), (long)ld, (long)M, (int)C, (int)kind);
    return ldt_check_launch("block_activation");
}

// out = a + b (fp32; c = t_emb + label / image-condition embedding, model/scorenet/score.py:135).  out may alias a or b.
__global__ __launch_bounds__(256) void add_f32_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = a[i] + b[i];
}
extern "C" int ldt_add_f32(const float* a, const float* b, float* out, int64_t n, void* stream) {
    LDT_REQUIRE(a && b && out && n > 0, LDT_EARG, "add_f32: bad argument");
    hipLaunchKernelGGL(add_f32_kernel, dim3(ldt_grid_1d(n, 256, 2048)), dim3(256), 0, ldt_stream(stream), a, b, out, (long)n);
    return ldt_check_launch("add_f32");
}

// bf16 -> fp32 widening of a packed weight panel (exact), for the fp32 table builds that must see the SAME rounded weights
// the MFMAs multiply by (Score.fold_table).
__global__ __launch_bounds__(256) void widen_bf16_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, long n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = (float)src[i];
}
extern "C" int ldt_widen_bf16(const uint16_t* src, float* dst, int64_t n, void* stream) {
    LDT_REQUIRE(src && dst && n > 0, LDT_EARG, "widen_bf16: bad argument");
    hipLaunchKernelGGL(widen_bf16_kernel, dim3(ldt_grid_1d(n, 256, 4096)), dim3(256), 0, ldt_stream(stream), ldt_bf16(src), dst, (long)n);
    return ldt_check_launch("widen_bf16");
}

// ------------------------------------------------------------------------------------------------
// LN-folding monitor: max over rows of mean^2 / variance from the producer's row statistics stats[parts][M][2] (partial
// (sum, sum of squares) per 256-column tile).  The folded projections round x (1 + scale) to bf16 BEFORE the mean is removed,
// so their error variance is (1 + mean^2 / variance) x the LayerNorm kernel's; the sampler reads this once per
// sample() call and falls back to the LayerNorm kernels when the ratio says the 1e-4 parity bar is at risk.
// One workgroup of 256 threads, fixed order: deterministic.  *out = the maximum ratio (0 when M == 0).
__global__ __launch_bounds__(256) void fold_mean_ratio_kernel(const float* __restrict__ stats, int parts, long M, int K, float* __restrict__ out) {
    float best = 0.f;
    const float invk = 1.0f / (float)K;
    for (long r = threadIdx.x; r < M; r += 256) {
        float s1 = 0.f, s2 = 0.f;
        for (int p = 0; p < parts; ++p) { s1 += stats[((long)p * M + r) * 2]; s2 += stats[((long)p * M + r) * 2 + 1]; }
        const float mean = s1 * invk;
        const float var = fmaxf(s2 * invk - mean * mean, 0.f) + 1e-6f;
        best = fmaxf(best, mean * mean / var);
    }
    best = wave_max(best);
    __shared__ float part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) *out = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}
// the same, accumulated into *out by atomic max (ratios are non-negative: their bit patterns order like ints); the Score
// forward calls it after every folded residual GEMM when plan->fold_monitor is set
__global__ __launch_bounds__(256) void fold_monitor_kernel(const float* __restrict__ stats, int parts, long M, int K, float* __restrict__ out) {
    float best = 0.f;
    const float invk = 1.0f / (float)K;
    for (long r = blockIdx.x * 256L + threadIdx.x; r < M; r += (long)gridDim.x * 256) {
        float s1 = 0.f, s2 = 0.f;
        for (int p = 0; p < parts; ++p) { s1 += stats[((long)p * M + r) * 2]; s2 += stats[((long)p * M + r) * 2 + 1]; }
        const float mean = s1 * invk;
        const float var = fmaxf(s2 * invk - mean * mean, 0.f) + 1e-6f;
        best = fmaxf(best, mean * mean / var);
    }
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0) atomicMax(reinterpret_cast<int*>(out), __float_as_int(best));
}
int ldt_fold_monitor_launch(const float* stats, int parts, long M, int K, float* out, hipStream_t s) {
    hipLaunchKernelGGL(fold_monitor_kernel, dim3(ldt_grid_1d(M, 256, 64)), dim3(256), 0, s, stats, parts, M, K, out);
    return ldt_check_launch("fold_monitor");
}
extern "C" int ldt_fold_mean_ratio(const float* stats, int32_t parts, int64_t M, int32_t K, float* out, void* stream) {
    LDT_REQUIRE(stats && out && parts >= 1 && M > 0 && K > 0, LDT_EARG, "fold_mean_ratio: bad argument");
    hipLaunchKernelGGL(fold_mean_ratio_kernel, dim3(1), dim3(256), 0, ldt_stream(stream), stats, parts, (long)M, K, out);
    return ldt_check_launch("fold_mean_ratio");
}
