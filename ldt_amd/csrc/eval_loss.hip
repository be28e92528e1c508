// The posterior draw and the loss arithmetic of held-out evaluation, between kernels that already exist (encode, Score forward, Chamfer):
//   ldt_reparam      posterior draw alone, into a strided slice of all_eps   (model/Compressor/Network.py:26-29,75-77)
//   ldt_reparam_kl   posterior draw + per-element log q(z), KL and the per-sample KL sum   (model/Compressor/Network.py:12-29,221-224)
//   ldt_reparam_kl_bwd   its backward for training: d(draw) and d(kl_scale x sum kl) with respect to mu | logvar, in closed form
//   ldt_diffuse_q    x_t = m_t x_0 + sqrt(var_t) eta with per-sample scalars, eta injected or drawn from the Philox stream
//                    (diffusion/diffusion_continuous.py:78-81; trainer/Latent_SDE_Trainer.py:79-81)
//   ldt_dsm_loss     denoising score-matching distance, per-sample and overall mean   (trainer/Latent_SDE_Trainer.py:83-87)
// All are single-pass fp32 streaming kernels over a few MB, far below the encode / Score forward they sit next to.  They are written for
// determinism: every sum has a fixed order (per-thread strided partial -> wave shuffle -> LDS partials added in index order), no atomics,
// so two runs of the same input are bit-identical.  Where the reference's fp32 operation order is restated, FMA contraction is off.
#include "../../include/ldt_hip.h"
#include "kernels.h"

#define EVAL_WG 1024                 // one workgroup per sample: 16 waves keep enough 16-byte loads in flight on a B-workgroup grid
#define LOG_SQRT_2PI 0.9189385332f   // the constant as the reference writes it (Network.py:13,18)

// sum over the workgroup in a fixed order; the result is valid in thread 0
__device__ __forceinline__ float block_sum_fixed(float v) {
    __shared__ float part[EVAL_WG / LDT_WAVE];
    v = wave_sum(v);
    __syncthreads();                                     // (a second call must not overwrite partials still being read)
    if ((threadIdx.x & (LDT_WAVE - 1)) == 0) part[threadIdx.x / LDT_WAVE] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < (int)(blockDim.x / LDT_WAVE); ++w) s += part[w];
    return s;
}

template <int V> struct Pack;
template <> struct Pack<1> { typedef float T; };
template <> struct Pack<4> { typedef f32x4 T; };
template <int V> __device__ __forceinline__ float lane(const typename Pack<V>::T& v, int j);
template <> __device__ __forceinline__ float lane<1>(const float& v, int) { return v; }
template <> __device__ __forceinline__ float lane<4>(const f32x4& v, int j) { return v[j]; }
template <int V> __device__ __forceinline__ void set_lane(typename Pack<V>::T& v, int j, float x);
template <> __device__ __forceinline__ void set_lane<1>(float& v, int, float x) { v = x; }
template <> __device__ __forceinline__ void set_lane<4>(f32x4& v, int j, float x) { v[j] = x; }
template <int V> __device__ __forceinline__ typename Pack<V>::T ld(const float* p) { return *reinterpret_cast<const typename Pack<V>::T*>(p); }
template <int V> __device__ __forceinline__ void st(float* p, const typename Pack<V>::T& v) { *reinterpret_cast<typename Pack<V>::T*>(p) = v; }

// ------------------------------------------------------------------------------------------------
// posterior draw (Network.py:26-29,75-77): mu = post[:, :z], logvar = clamp(post[:, z:], lo, hi);
// eps = mu + exp(logvar / 2) * noise   -> written into a strided slice of all_eps
__global__ void reparam_kernel(const float* __restrict__ post, const float* __restrict__ noise, float* __restrict__ out,
                               long ldo, float* __restrict__ mu_out, float* __restrict__ lv_out, long rows, int z, float lo, float hi) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < rows * z; i += (long)gridDim.x * blockDim.x) {
        const long r = i / z; const int c = (int)(i % z);
        const float mu = post[r * 2 * z + c];
        const float lv = fminf(fmaxf(post[r * 2 * z + z + c], lo), hi);
        out[r * ldo + c] = reparam_eps(mu, lv, noise[i]);
        if (mu_out) { mu_out[i] = mu; lv_out[i] = lv; }
    }
}
extern "C" int ldt_reparam(const float* post, const float* noise, float* out, int64_t ldo, float* mu_out, float* logvar_out,
                           int64_t rows, int32_t z, float lo, float hi, void* stream) {
    LDT_REQUIRE(post && noise && out, LDT_EARG, "reparam: null pointer");
    LDT_REQUIRE(rows > 0 && z > 0 && ldo >= z, LDT_ESHAPE, "reparam: bad shape");
    LDT_REQUIRE((mu_out == nullptr) == (logvar_out == nullptr), LDT_EARG, "reparam: mu/logvar outputs go together");
    hipLaunchKernelGGL(reparam_kernel, dim3(ldt_grid_1d(rows * z, 256, 4096)), dim3(256), 0, ldt_stream(stream), post, noise, out, (long)ldo, mu_out,
                       logvar_out, (long)rows, (int)z, lo, hi);
    return ldt_check_launch("reparam");
}

// ------------------------------------------------------------------------------------------------
// posterior draw with its loss terms.  One workgroup per sample; V = 4 when z, ldo and every pointer allow 16-byte accesses (a group of 4 never crosses a row), else 1.
template <int V>
__global__ __launch_bounds__(EVAL_WG) void reparam_kl_kernel(const float* __restrict__ post, const float* __restrict__ noise, float* __restrict__ out,
                                                             long ldo, float* __restrict__ mu_out, float* __restrict__ lv_out,
                                                             float* __restrict__ kl_out, float* __restrict__ logqz_out,
                                                             float* __restrict__ kl_sample_sum, long rows_per_sample, int z, float lo, float hi) {
    typedef typename Pack<V>::T vec;
    const long row0 = (long)blockIdx.x * rows_per_sample;
    const long per = rows_per_sample * z;
    float acc = 0.f;
    for (long g = threadIdx.x; g < per / V; g += EVAL_WG) {
        const long e = g * V;
        const long r = row0 + e / z; const int c = (int)(e % z);
        const long i = r * z + c;
        const vec pm = ld<V>(post + r * 2 * z + c);
        const vec pl = ld<V>(post + r * 2 * z + z + c);
        const vec nz = ld<V>(noise + i);
        vec v_eps, v_lv, v_kl, v_lq;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float mu = lane<V>(pm, j);
            const float lv = fminf(fmaxf(lane<V>(pl, j), lo), hi);
            const float eps = reparam_eps(mu, lv, lane<V>(nz, j));
            float logqz, kl;
            {
#pragma clang fp contract(off)      // the reference's separate fp32 roundings (Network.py:12-19): no FMA
                const float d = eps - mu;
                const float a = (-0.5f * (d * d)) / expf(lv);
                const float b = 0.5f * lv;
                logqz = (a - b) - LOG_SQRT_2PI;
                const float logpz = (-0.5f * (eps * eps)) - LOG_SQRT_2PI;
                kl = logqz - logpz;
            }
            acc += kl;
            set_lane<V>(v_eps, j, eps); set_lane<V>(v_lv, j, lv); set_lane<V>(v_kl, j, kl); set_lane<V>(v_lq, j, logqz);
        }
        st<V>(out + r * ldo + c, v_eps);
        if (mu_out) { st<V>(mu_out + i, pm); st<V>(lv_out + i, v_lv); }
        if (kl_out) st<V>(kl_out + i, v_kl);
        if (logqz_out) st<V>(logqz_out + i, v_lq);
    }
    if (kl_sample_sum) {
        const float s = block_sum_fixed(acc);
        if (threadIdx.x == 0) kl_sample_sum[blockIdx.x] = s;
    }
}

extern "C" int ldt_reparam_kl(const float* post, const float* noise, float* out, int64_t ldo, float* mu_out, float* logvar_out,
                              float* kl_out, float* logqz_out, float* kl_sample_sum, int64_t rows, int64_t rows_per_sample, int32_t z,
                              float lo, float hi, void* stream) {
    LDT_REQUIRE(post && noise && out, LDT_EARG, "reparam_kl: null pointer");
    LDT_REQUIRE((mu_out == nullptr) == (logvar_out == nullptr), LDT_EARG, "reparam_kl: mu/logvar outputs go together");
    LDT_REQUIRE(rows > 0 && z > 0 && ldo >= z && rows_per_sample > 0 && rows % rows_per_sample == 0, LDT_ESHAPE,
                "reparam_kl: bad shape (rows %ld, rows_per_sample %ld, z %d, ldo %ld)", (long)rows, (long)rows_per_sample, z, (long)ldo);
    const long B = rows / rows_per_sample;
    LDT_REQUIRE(B <= 0x7fffffffL, LDT_ESHAPE, "reparam_kl: %ld samples", B);
    const bool vec = z % 4 == 0 && ldo % 4 == 0 && ldt_aligned16(post) && ldt_aligned16(noise) && ldt_aligned16(out) &&
                     ldt_aligned16(mu_out) && ldt_aligned16(logvar_out) && ldt_aligned16(kl_out) && ldt_aligned16(logqz_out);
    hipStream_t s = ldt_stream(stream);
    if (vec)
        hipLaunchKernelGGL(reparam_kl_kernel<4>, dim3((unsigned)B), dim3(EVAL_WG), 0, s, post, noise, out, (long)ldo, mu_out, logvar_out, kl_out,
                           logqz_out, kl_sample_sum, (long)rows_per_sample, z, lo, hi);
    else
        hipLaunchKernelGGL(reparam_kl_kernel<1>, dim3((unsigned)B), dim3(EVAL_WG), 0, s, post, noise, out, (long)ldo, mu_out, logvar_out, kl_out,
                           logqz_out, kl_sample_sum, (long)rows_per_sample, z, lo, hi);
    return ldt_check_launch("reparam_kl");
}

// ------------------------------------------------------------------------------------------------
// Backward of the draw and of kl_scale x sum(kl) (include/ldt_hip.h), one thread per V adjacent elements of a row.  log q(z) depends on mu and
// logvar only through -logvar / 2 once eps = mu + s n is put in ((eps - mu)^2 / exp(logvar) = n^2), and -log p(z) = eps^2 / 2 + const.
template <int V>
__global__ __launch_bounds__(256) void reparam_kl_bwd_kernel(const float* __restrict__ post, const float* __restrict__ noise,
                                                             const float* __restrict__ d_eps, long ldd, float kl_scale, float* __restrict__ dpost,
                                                             long rows, int z, float lo, float hi) {
    typedef typename Pack<V>::T vec;
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows * z / V) return;
    const long e = g * V, r = e / z;
    const int c = (int)(e % z);
    const vec pm = ld<V>(post + r * 2 * z + c);
    const vec pl = ld<V>(post + r * 2 * z + z + c);
    const vec nz = ld<V>(noise + r * z + c);
    const vec de = ld<V>(d_eps + r * ldd + c);
    vec v_mu, v_lv;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float raw = lane<V>(pl, j), n = lane<V>(nz, j);
        const float lv = fminf(fmaxf(raw, lo), hi);
        const float eps = reparam_eps(lane<V>(pm, j), lv, n);
        const float gj = fmaf(kl_scale, eps, lane<V>(de, j));
        const float dlv = fmaf(gj, 0.5f * (n * expf(lv / 2.f)), -0.5f * kl_scale);
        set_lane<V>(v_mu, j, gj);
        set_lane<V>(v_lv, j, raw >= lo && raw <= hi ? dlv : 0.f);
    }
    st<V>(dpost + r * 2 * z + c, v_mu);
    st<V>(dpost + r * 2 * z + z + c, v_lv);
}

extern "C" int ldt_reparam_kl_bwd(const float* post, const float* noise, const float* d_eps, int64_t ldd, float kl_scale, float* dpost,
                                  int64_t rows, int32_t z, float lo, float hi, void* stream) {
    LDT_REQUIRE(post && noise && d_eps && dpost, LDT_EARG, "reparam_kl_bwd: null pointer");
    LDT_REQUIRE(rows > 0 && z > 0 && ldd >= z && rows <= (1L << 40) / z, LDT_ESHAPE, "reparam_kl_bwd: bad shape (rows %ld, z %d, ldd %ld)", (long)rows, z,
                (long)ldd);
    const bool vec = z % 4 == 0 && ldd % 4 == 0 && ldt_aligned16(post) && ldt_aligned16(noise) && ldt_aligned16(d_eps) && ldt_aligned16(dpost);
    const long threads = rows * z / (vec ? 4 : 1), wgs = (threads + 255) / 256;
    LDT_REQUIRE(wgs <= 0x7fffffffL, LDT_ESHAPE, "reparam_kl_bwd: %ld elements", (long)rows * z);
    hipStream_t s = ldt_stream(stream);
    if (vec)
        hipLaunchKernelGGL(reparam_kl_bwd_kernel<4>, dim3((unsigned)wgs), dim3(256), 0, s, post, noise, d_eps, (long)ldd, kl_scale, dpost, (long)rows, z, lo, hi);
    else
        hipLaunchKernelGGL(reparam_kl_bwd_kernel<1>, dim3((unsigned)wgs), dim3(256), 0, s, post, noise, d_eps, (long)ldd, kl_scale, dpost, (long)rows, z, lo, hi);
    return ldt_check_launch("reparam_kl_bwd");
}

// ------------------------------------------------------------------------------------------------
// x_t = x_0 m[b] + sqrt(var[b]) eta, 4 elements per thread; eta read, or drawn with the keying of philox_normal_kernel (counter = global
// element index / 4, stream id = step, key = seed) and written out, so a separate ldt_philox_normal call reproduces it bit for bit.
__global__ __launch_bounds__(256) void diffuse_q_kernel(const float* __restrict__ x0, const float* __restrict__ eta_in, const float* __restrict__ m,
                                                        const float* __restrict__ var, float* __restrict__ xt, float* __restrict__ eta_out,
                                                        long nvec, long per_sample, int step, uint32_t k0, uint32_t k1) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
        const long b = 4 * i / per_sample;
        const f32x4 x = *reinterpret_cast<const f32x4*>(x0 + 4 * i);
        f32x4 eta;
        if (eta_in) {
            eta = *reinterpret_cast<const f32x4*>(eta_in + 4 * i);
        } else {
            uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)step, 0x4C445421u};
            philox4x32_10(c, k0, k1);
            float z0, z1, z2, z3;
            box_muller(c[0], c[1], z0, z1);
            box_muller(c[2], c[3], z2, z3);
            eta = (f32x4){z0, z1, z2, z3};
        }
        const float mb = m[b], vb = var[b];
        f32x4 r;
        {
#pragma clang fp contract(off)      // eps * e2int_f + torch.sqrt(var) * eta: two products, one sum, each rounded
            const float sd = sqrtf(vb);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float a = x[j] * mb;
                const float n = sd * eta[j];
                r[j] = a + n;
            }
        }
        *reinterpret_cast<f32x4*>(xt + 4 * i) = r;
        if (eta_out) *reinterpret_cast<f32x4*>(eta_out + 4 * i) = eta;
    }
}

extern "C" int ldt_diffuse_q(const float* x0, const float* eta_in, const float* m, const float* var, float* xt, float* eta_out,
                             int64_t B, int64_t per_sample, uint64_t seed, int32_t step, void* stream) {
    LDT_REQUIRE(x0 && m && var && xt, LDT_EARG, "diffuse_q: null pointer");
    LDT_REQUIRE(eta_in || eta_out, LDT_EARG, "diffuse_q: no eta_in and nowhere to write the drawn eta (eta_out)");
    LDT_REQUIRE(B > 0 && per_sample > 0 && per_sample % 4 == 0, LDT_ESHAPE, "diffuse_q: B %ld, per_sample %ld (must be a multiple of 4)",
                (long)B, (long)per_sample);
    LDT_REQUIRE(ldt_aligned16(x0) && ldt_aligned16(eta_in) && ldt_aligned16(xt) && ldt_aligned16(eta_out), LDT_EALIGN,
                "diffuse_q: buffers must be 16-byte aligned");
    const long nvec = B * per_sample / 4;
    hipLaunchKernelGGL(diffuse_q_kernel, dim3(ldt_grid_1d(nvec, 256, 2048)), dim3(256), 0, ldt_stream(stream), x0, eta_in, m, var, xt, eta_out,
                       nvec, (long)per_sample, step, (uint32_t)seed, (uint32_t)(seed >> 32));
    return ldt_check_launch("diffuse_q");
}

// ------------------------------------------------------------------------------------------------
// stage 1: one workgroup per sample, sample_loss[b] = mean over the sample of distance * weight[b] — every distance is multiplied by the
// weight before it is summed, as `(distance * weight_p).mean()` does; V as above.
template <int V>
__global__ __launch_bounds__(EVAL_WG) void dsm_sample_kernel(const float* __restrict__ eta, const float* __restrict__ params,
                                                             const float* __restrict__ weight, long per_sample, int l1,
                                                             float* __restrict__ sample_loss) {
    typedef typename Pack<V>::T vec;
    const float* e = eta + (long)blockIdx.x * per_sample;
    const float* p = params + (long)blockIdx.x * per_sample;
    const float w = weight ? weight[blockIdx.x] : 1.f;
    float acc = 0.f;
    for (long g = threadIdx.x; g < per_sample / V; g += EVAL_WG) {
        const vec a = ld<V>(e + g * V), b = ld<V>(p + g * V);
#pragma unroll
        for (int j = 0; j < V; ++j) {
#pragma clang fp contract(off)
            const float d = lane<V>(a, j) - lane<V>(b, j);
            const float dist = l1 ? fabsf(d) : d * d;
            acc += dist * w;
        }
    }
    const float s = block_sum_fixed(acc);
    if (threadIdx.x == 0) sample_loss[blockIdx.x] = s / (float)per_sample;
}
// stage 2: the mean over the batch of the per-sample means (samples are equally long), one workgroup, fixed order
__global__ __launch_bounds__(EVAL_WG) void dsm_mean_kernel(const float* __restrict__ sample_loss, long B, float* __restrict__ mean_loss) {
    float acc = 0.f;
    for (long i = threadIdx.x; i < B; i += EVAL_WG) acc += sample_loss[i];
    const float s = block_sum_fixed(acc);
    if (threadIdx.x == 0) *mean_loss = s / (float)B;
}

extern "C" int ldt_dsm_loss(const float* eta, const float* params, const float* weight, int64_t B, int64_t per_sample, int32_t l1,
                            float* sample_loss, float* mean_loss, void* stream) {
    LDT_REQUIRE(eta && params && sample_loss, LDT_EARG, "dsm_loss: null pointer (sample_loss is the first stage's output and is required)");
    LDT_REQUIRE(B > 0 && B <= 0x7fffffffL && per_sample > 0, LDT_ESHAPE, "dsm_loss: B %ld, per_sample %ld", (long)B, (long)per_sample);
    hipStream_t s = ldt_stream(stream);
    if (per_sample % 4 == 0 && ldt_aligned16(eta) && ldt_aligned16(params))
        hipLaunchKernelGGL(dsm_sample_kernel<4>, dim3((unsigned)B), dim3(EVAL_WG), 0, s, eta, params, weight, (long)per_sample, l1, sample_loss);
    else
        hipLaunchKernelGGL(dsm_sample_kernel<1>, dim3((unsigned)B), dim3(EVAL_WG), 0, s, eta, params, weight, (long)per_sample, l1, sample_loss);
    int rc = ldt_check_launch("dsm_loss");
    if (rc != LDT_OK || !mean_loss) return rc;
    hipLaunchKernelGGL(dsm_mean_kernel, dim3(1), dim3(EVAL_WG), 0, s, sample_loss, (long)B, mean_loss);
    return ldt_check_launch("dsm_loss (mean)");
}
