// bf16 MFMA GEMM for the token-linear layers of the LDT hot path (gfx950 / MI355X).
//
//   Y[M,N] = epilogue( X[M,K] (bf16, row-major, ldx) · W[N,K]^T (bf16, row-major, ldw) + bias[N] )
//
// This is every 1x1 Conv1d / Linear on the path (reference: model/layers.py:159-161 fc_q/fc_kv/fc_o,
// :121-124 MLP fc/out, model/scorenet/score.py:110,112 ln_in/ln_out.ln; Compressor twins).  A Conv1d
// weight (out,in,1) is already the [N][K] K-contiguous operand MFMA wants, so nothing is transposed.
//
// Structure (v1, "2-phase" of the CDNA4 guide): 128x128x64 tile, 256 threads = 2x2 waves of 64x64,
// mfma_f32_16x16x32_bf16 with the operands SWAPPED (D[n][m] = W·X^T) so that each lane ends up with 4
// consecutive output columns of one row -> 16-B fp32 / 8-B bf16 epilogue accesses.  Both operand tiles
// are staged HBM->LDS with global_load_lds (16 B/lane, LDS image lane-linear), double-buffered; the
// LDS bank-conflict swizzle chunk' = chunk ^ ((row>>1)&7) is applied on the SOURCE address and on the
// ds_read address (both-sides rule).  The workgroup->tile map is XCD-aware (blocks that share an XCD's
// L2 walk one row-panel of X across the N tiles of W).
//
// Fused epilogues (template EPI):
//   EPI_F32        out fp32  = acc + bias
//   EPI_BF16       out bf16  = acc + bias
//   EPI_GELU_BF16  out bf16  = gelu_erf(acc + bias)                       (MLP up, layers.py:127-129)
//   EPI_RELU_BF16  out bf16  = relu(acc + bias [+ skip bf16])             (PreExtraction, Compressor/layers.py:115-160)
//   EPI_RESID_F32  out fp32  = resid + gate[s,n] * (acc + bias)           (x + gate*(...), layers.py:218-219; gate may be null)
// This file: that small-tile kernel (v1), the dispatch rule (ldt_gemm_decide) and the two launch entries.  The 256-row-tile kernels
// live in gemm_256.hip (shared machinery and the tile list: gemm256_tile.h), the mid-size tile kernels in gemm_mid.hip.
#include "gemm256_tile.h"

#define BK 64

template <int ROWS, int NW = 4>
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ g, long ld, int row0, int nrows_total,
                                           int k0, char* lds_tile, int wave, int lane) {
    // one operand tile = ROWS rows x 128 B = ROWS/8 pieces of 1 KiB (8 rows each); ROWS/(8 NW) pieces per wave
#pragma unroll
    for (int p = 0; p < ROWS / (8 * NW); ++p) {
        const int piece = wave * (ROWS / (8 * NW)) + p;
        const int r = piece * 8 + (lane >> 3);
        const int cdst = lane & 7;
        const int csrc = cdst ^ ((r >> 1) & 7);
        int grow = row0 + r;
        grow = grow < nrows_total ? grow : nrows_total - 1;          // clamp: OOB rows are never stored
        const bf16_t* src = g + (long)grow * ld + k0 + csrc * 8;
        char* dst = lds_tile + piece * 1024;                          // wave-uniform; HW adds lane*16
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
}

// TBM x TBN output tile (each 128 or 64): 128x128 is the workhorse of mid-size problems, the smaller shapes keep all
// 256 CUs busy when M*N is small (T=32 latents: M = 2048 rows).
// NST = 2: a stage is waited for in full before the barrier (the simple 2-phase loop).  NST = 3: the DMA of stage
// kt+2 stays in flight across the barrier (counted vmcnt, raw s_barrier), which hides the load latency when only 1-3
// workgroups share a CU (small M: the T = 32 latents, half-batch shapes).
// Built as 128 x 128 and 128 x 64 with 2 stages and 64 x 64 with 3 (NW stays 4: the 8-wave forms gave way to gemm_mid.hip).
template <int EPI, int TBM, int TBN, int NST = 2, int NW = 4>
__global__ __launch_bounds__(NW * 64) void gemm_bf16_nt_kernel(const GemmArgs a) {
    constexpr int BM = TBM, BN = TBN;
    constexpr int XB = TBM * BK * 2, WB = TBN * BK * 2;               // operand tile bytes per stage
    constexpr int WGM = NW / 2;                                       // waves along m (2 along n)
    constexpr int MT = TBM / (16 * WGM), NT = TBN / 32;               // 16x16 accumulator tiles per wave (m, n)
    constexpr int OPS = (TBM + TBN) / (8 * NW);                       // LDS-DMA instructions per wave and stage
    __shared__ __attribute__((aligned(16))) char smem[NST * (XB + WB)];  // [stage][X|W]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;

    // ---- XCD-aware bijective remap of the 1-D grid (blocks b, b+8, ... share an XCD's L2) ----
    const int tiles_n = (a.N + BN - 1) / BN;
    const int nwg = gridDim.x;
    const int bid = blockIdx.x;
    const int q = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
    const int wgid = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + (bid >> 3);
    // tile order: row-major (an XCD's chunk of workgroups = a band of output rows x every column tile: it reads its own rows of X
    // and ALL of W) or column-major (a band of column tiles x every row tile: its own slice of W, all of X) — ldt_gemm_decide picks
    // column-major for wide outputs over few row tiles (M = 1024: QKV 15.9 -> 14.5 us, MLP-up 18.2 -> 16.1 us; profiles/r03_smallm_tile_sweep.txt, its script last existed at 8127e49)
    const int tiles_m = (a.M + BM - 1) / BM;
    const int tile_m = a.col_major ? wgid % tiles_m : wgid / tiles_n, tile_n = a.col_major ? wgid / tiles_m : wgid % tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const bf16_t* Xk = a.X;
    const bf16_t* Wk = a.W;
    const int nk = a.K / BK;
    stage_tile<TBM, NW>(Xk, a.ldx, m0, a.M, 0, smem, wave, lane);
    stage_tile<TBN, NW>(Wk, a.ldw, n0, a.N, 0, smem + XB, wave, lane);
    // stages 1 .. NST-2 follow at once; wait until only they are outstanding (stage 0 landed)
    int ahead = 0;                                                    // stages issued beyond the one being waited for
#pragma unroll
    for (int st = 1; st < NST - 1; ++st)
        if (st < nk) {
            stage_tile<TBM, NW>(Xk, a.ldx, m0, a.M, st * BK, smem + st * (XB + WB), wave, lane);
            stage_tile<TBN, NW>(Wk, a.ldw, n0, a.N, st * BK, smem + st * (XB + WB) + XB, wave, lane);
            ++ahead;
        }
    if (NST >= 3 && ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    const int lrow = lane & 15;
    const int lchk = lane >> 4;
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        char* sx = smem + cur * (XB + WB);
        char* sw = sx + XB;
        if (kt + NST - 1 < nk) {                                      // buffer of stage kt-1 (NST = 3) / kt+1's own (NST = 2)
            int nb = cur + NST - 1; nb = nb >= NST ? nb - NST : nb;
            char* nx = smem + nb * (XB + WB);
            stage_tile<TBM, NW>(Xk, a.ldx, m0, a.M, (kt + NST - 1) * BK, nx, wave, lane);
            stage_tile<TBN, NW>(Wk, a.ldw, n0, a.N, (kt + NST - 1) * BK, nx + XB, wave, lane);
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 wf[NT], xf[MT];
            const int c = ks * 4 + lchk;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int rw = wn * (TBN / 2) + i * 16 + lrow;
                wf[i] = *reinterpret_cast<const bf16x8*>(sw + rw * 128 + ((c ^ ((rw >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int rx = wm * (TBM / WGM) + i * 16 + lrow;
                xf[i] = *reinterpret_cast<const bf16x8*>(sx + rx * 128 + ((c ^ ((rx >> 1) & 7)) << 4));
            }
#pragma unroll
            for (int ni = 0; ni < NT; ++ni)
#pragma unroll
                for (int mi = 0; mi < MT; ++mi)
                    acc[ni][mi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ni], xf[mi], acc[ni][mi], 0, 0, 0);
        }
        // stage kt+1 landed (only the stages behind it, kt+2 .. kt+NST-1, may still be in flight), then visible to every wave
        const int left = nk - 2 - kt;                                 // stages that exist beyond kt+1
        if (NST >= 3 && left >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(OPS) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        cur = cur + 1 == NST ? 0 : cur + 1;
    }

    // ---- epilogue: lane holds D[n = nb + (lane>>4)*4 + r][m = mb + (lane&15)], r = 0..3 ----
    const float* gate = a.gate;
    if (EPI == EPI_RESID_F32 && gate && a.step_ptr) gate += (long)(*a.step_ptr) * a.gate_step_stride;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
        const int m = m0 + wm * (TBM / WGM) + mi * 16 + lrow;
        if (m >= a.M) continue;
        const float* grow = nullptr;
        if (EPI == EPI_RESID_F32 && gate) grow = gate + (long)(m / a.rows_per_sample) * a.gate_sample_stride;
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
            const int n = n0 + wn * (TBN / 2) + ni * 16 + lchk * 4;
            if (n >= a.N) continue;
            f32x4 v = acc[ni][mi];
            const bool full = (n + 3 < a.N);
            float b[4] = {0.f, 0.f, 0.f, 0.f};
            if (a.bias) {
                if (full) { const f32x4 t = *reinterpret_cast<const f32x4*>(a.bias + n); b[0] = t[0]; b[1] = t[1]; b[2] = t[2]; b[3] = t[3]; }
                else for (int r = 0; r < 4; ++r) if (n + r < a.N) b[r] = a.bias[n + r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += b[r];
            if (EPI == EPI_F32) {
                float* o = reinterpret_cast<float*>(a.out) + (long)m * a.ldo + n;
                if (full) *reinterpret_cast<f32x4*>(o) = v;
                else for (int r = 0; r < 4; ++r) if (n + r < a.N) o[r] = v[r];
            } else if (EPI == EPI_RESID_F32) {
                float* o = reinterpret_cast<float*>(a.out) + (long)m * a.ldo + n;
                const float* rs = a.resid + (long)m * a.ldr + n;
                if (full) {
                    f32x4 x = *reinterpret_cast<const f32x4*>(rs);
                    if (grow) { const f32x4 g = *reinterpret_cast<const f32x4*>(grow + n);
#pragma unroll
                        for (int r = 0; r < 4; ++r) x[r] = x[r] + g[r] * v[r];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) x[r] = x[r] + v[r];
                    }
                    *reinterpret_cast<f32x4*>(o) = x;
                } else {
                    for (int r = 0; r < 4; ++r) if (n + r < a.N) o[r] = rs[r] + (grow ? grow[n + r] : 1.f) * v[r];
                }
            } else {
                if (EPI == EPI_GELU_BF16) {
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {                 // two lanes of the polynomial per v_pk_* instruction
                        const f32x2 gg = gelu_erf_fast2((f32x2){v[r], v[r + 1]});
                        v[r] = gg[0]; v[r + 1] = gg[1];
                    }
                }
                if (EPI == EPI_RELU_BF16) {
                    if (a.skip) {
                        const bf16_t* sk = a.skip + (long)m * a.lds_ + n;
                        for (int r = 0; r < 4; ++r) if (n + r < a.N) v[r] += (float)sk[r];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
                }
                bf16_t* o = reinterpret_cast<bf16_t*>(a.out) + (long)m * a.ldo + n;
                if (full) {
                    bf16x4 pk = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                    *reinterpret_cast<bf16x4*>(o) = pk;
                } else for (int r = 0; r < 4; ++r) if (n + r < a.N) o[r] = (bf16_t)v[r];
            }
        }
    }
}

// LN-folding launches.  Large batches: the 256-tile kernel (statistics per 256 columns).  Small batches — all four GEMMs of a Score block
// (N = D, 3D, F) below the fill rule (ldt_fills_workgroups) — fold through the mid-size tile kernel (gemm_mid.hip, statistics per 32 columns:
// stats[D / 32][M][2]) when it takes every one of them in a folded form; otherwise the LayerNorm kernels run.
static bool ldt_gemm_lnfold_mid_route(int M, int D, int F, int max_wgs) {
    auto small = [&](int N) { return !ldt_fills_workgroups((long)((M + 255) / 256) * ((N + 255) / 256), max_wgs); };
    if (!(M % 128 == 0 && D % 64 == 0 && F % 64 == 0 && D <= 1024 && small(D) && small(3 * D) && small(F))) return false;
    // the folded residual producers run 64 x 128 tiles (statistics per 32 columns need whole 128-column slabs): below 5/8 of the workgroups
    // they leave the chip half empty and the LayerNorm launches they replace are cheaper — M = 1024 (B = 32 x 32 tokens): folded 1.788 ms per
    // SDE step against 1.670 with the 64 x 64 plain forms + LayerNorm kernels (profiles/r06_c5_ln_fold_decision.txt); M = 2048: 256 tiles, folded wins
    if (!ldt_fills_workgroups((long)(M / 64) * (D / 128), max_wgs)) return false;
    return ldt_gemm_mid_lnfold_takes(EPI_RESID_F32, M, D, D) && ldt_gemm_mid_lnfold_takes(EPI_RESID_F32, M, D, F) &&
           ldt_gemm_mid_lnfold_takes(EPI_BF16, M, 3 * D, D) && ldt_gemm_mid_lnfold_takes(EPI_GELU_BF16, M, F, D);
}
// The fold decision of a Score block (kernels.h): the small-batch route first, else the 256-tile kernels when the residual GEMMs' tiles fill the workgroups
ScoreFold ldt_score_fold_decide(int M, int D, int F, int max_wgs) {
    ScoreFold f{SCORE_FOLD_NONE, false, 256};
    if (M <= 0 || D <= 0 || F <= 0 || D % 256 != 0 || D > 1024 || F % 256 != 0) return f;
    f.shape_256 = M % 256 == 0;
    if (ldt_gemm_lnfold_mid_route(M, D, F, max_wgs)) { f.route = SCORE_FOLD_MID; f.granule = 32; }
    else if (f.shape_256 && ldt_fills_workgroups((long)(M / 256) * (D / 256), max_wgs)) f.route = SCORE_FOLD_256;
    return f;
}

// The v1 kernel's forms: tile and stages.  3 stages only for 64x64 tiles (48 KB of LDS, still 3 workgroups per CU; M = 2048: fc_o 13.5 -> 12.3,
// mlp.out 38.6 -> 31.3 us; a 4th stage measured equal): at 128x64 / 128x128 the third buffer costs a co-resident workgroup and loses 20-40 %
struct V1Form { int bm, bn, stages; };
static constexpr V1Form V1_FORMS[3] = {{128, 128, 2}, {128, 64, 2}, {64, 64, 3}};

// The dispatch rule (kernels.h): family, tile and grid of a GEMM.  Shape-level only: pointer and alignment checks stay with the launchers.
GemmRoute ldt_gemm_decide(int epi, const GemmArgs* a, int granule) {
    GemmRoute r{};
    if (!(a->M > 0 && a->N > 0 && a->K > 0) || a->K % BK != 0 || a->ldo % 4 != 0) return r;
    const int lim = ldt_wg_limit(a->max_wgs);
    auto take_256 = [&]() {
        const int tm = a->M / 256, tn = a->N / 256, tiles = tm * tn;
        r.grid = tiles < lim ? tiles : lim;
        r.bm = r.bn = 256;
        r.tiles_per_wg = Tile256List::max_count(tm, tn, r.grid);        // the kernels' own tile list: the one-tile forms run only where it says so
        r.family = r.tiles_per_wg == 1 ? GEMM_ROUTE_256_ONE : GEMM_ROUTE_256_MULTI;
    };
    if (granule) {
        // LN-folded forms.  Large batches: the 256-tile kernel (statistics per 256 columns).  Small batches: the mid-size tile kernel
        // (statistics per 32 columns), when it takes the problem in a folded form.
        const bool producer = epi == EPI_RESID_F32;
        if (!producer && epi != EPI_BF16 && epi != EPI_GELU_BF16) return r;
        if (granule == 32) {
            if (a->M % 128 != 0 || a->N % 64 != 0 || a->K < 128) return r;
            ldt_gemm_mid_route(epi, producer ? FOLD_PRODUCER : FOLD_CONSUMER, a, &r);
        } else if (granule == 256) {
            if (a->M % 256 != 0 || a->N % 256 != 0 || a->K < 256 || !ldt_gemm256_takes(epi, a)) return r;
            if (!producer && (a->K % 256 != 0 || a->K > 1024)) return r;
            take_256();
        }
        return r;
    }
    // 256^2 persistent kernel when its tiles fill at least 5/8 of the workgroups this launch may use (all CUs, or a
    // sub-batch stream's share): at exactly half (M = 8192, N = 1024: 128 tiles on 256 CUs) the 128^2 kernel on every CU
    // is as fast (K = 1024) or 15 % faster (K = 4096).
    // (N <= 128 — the Compressor's 128-channel convs over millions of point rows — would leave half of every 256-wide tile
    //  empty: the 128^2 kernel streams those 5.7 % faster end to end, tools/dbg/c4_chunks.py)
    const bool big = ldt_fills_workgroups(((a->M + 255) / 256) * ((a->N + 255) / 256), a->max_wgs) && a->N > 128;
    // mid-size problems (gemm_mid.hip): 128 x 256 / 128 x 192 / 128 x 128 / 64 x 128 / 64 x 64 tiles with dedicated loader waves, when
    // the 256^2 persistent kernel would leave CUs idle — the 1-4k-row batches
    if (!big && ldt_gemm_mid_route(epi, FOLD_NONE, a, &r)) return r;
    if (big && ldt_gemm256_takes(epi, a)) { take_256(); return r; }
    // v1 form: the largest of 128x128 / 128x64 / 64x64 that still gives every CU two tiles — this 2-phase kernel hides a stage's load latency
    // only across co-resident workgroups (M = 2048: QKV 25.8 -> 22.9 us with 128x64, fc_o 14.4 -> 12.0 and mlp.out 47.7 -> 40.0 us with 64x64 tiles)
    long tm, tn;
    for (r.v1_form = 0;; ++r.v1_form) {
        r.bm = V1_FORMS[r.v1_form].bm; r.bn = V1_FORMS[r.v1_form].bn;
        tm = (a->M + r.bm - 1) / r.bm; tn = (a->N + r.bn - 1) / r.bn;
        if (r.v1_form == 2 || tm * tn >= 2 * LDT_NUM_CUS) break;        // the last form takes what is left
    }
    r.family = GEMM_ROUTE_V1;
    r.tiles_per_wg = 1;
    r.grid = (int)(tm * tn);
    r.col_major = tn >= 3 * tm ? 1 : 0;                                 // wide outputs over few row tiles (numbers: the kernel's tile-order comment)
    return r;
}

// operand checks of both launch entries (`who` prefixes the error text).  The folded forms store 16-byte bf16 rows next to the fp32 ones
// (ldo % 8) and have always filed a leading dimension below K under alignment.
static int gemm_check_operands(const char* who, bool folded, int epi, const GemmArgs* a) {
    LDT_REQUIRE(a->ldx % 8 == 0 && a->ldw % 8 == 0 && ldt_aligned16(a->X) && ldt_aligned16(a->W), LDT_EALIGN,
                "%s: X/W rows must be 16-byte aligned (ldx=%ld ldw=%ld)", who, a->ldx, a->ldw);
    LDT_REQUIRE(a->ldx >= a->K && a->ldw >= a->K, folded ? LDT_EALIGN : LDT_ESHAPE, "%s: leading dims smaller than K", who);
    LDT_REQUIRE(a->ldo % (folded ? 8 : 4) == 0 && ldt_aligned16(a->out), LDT_EALIGN, "%s: out rows must be 16-byte aligned (ldo=%ld)", who, a->ldo);
    if (epi == EPI_RESID_F32) {
        LDT_REQUIRE(a->resid && a->ldr % 4 == 0 && ldt_aligned16(a->resid), LDT_EALIGN, "%s: resid missing/misaligned", who);
        LDT_REQUIRE(!a->gate || (a->rows_per_sample > 0 && ldt_aligned16(a->gate) && a->gate_sample_stride % 4 == 0 && a->gate_step_stride % 4 == 0),
                    LDT_EARG, "%s: gate needs rows_per_sample>0 and 16-byte aligned strides", who);
    }
    LDT_REQUIRE(!a->bias || ldt_aligned16(a->bias), LDT_EALIGN, "%s: bias must be 16-byte aligned", who);
    return LDT_OK;
}

// the v1 kernel on the route's form, grid and tile order
template <int EPI>
static int launch_v1(const GemmArgs* a, const GemmRoute& r, hipStream_t stream) {
    static void (*const forms[3])(const GemmArgs) = {gemm_bf16_nt_kernel<EPI, V1_FORMS[0].bm, V1_FORMS[0].bn, V1_FORMS[0].stages>,
                                                     gemm_bf16_nt_kernel<EPI, V1_FORMS[1].bm, V1_FORMS[1].bn, V1_FORMS[1].stages>,
                                                     gemm_bf16_nt_kernel<EPI, V1_FORMS[2].bm, V1_FORMS[2].bn, V1_FORMS[2].stages>};
    GemmArgs v = *a; v.col_major = r.col_major;
    hipLaunchKernelGGL(forms[r.v1_form], dim3((unsigned)r.grid), dim3(256), 0, stream, v);
    return ldt_check_launch("gemm_bf16_nt");
}

// launches the route that ldt_gemm_decide chose (fold: gemm256_tile.h's FOLD_*; the v1 kernel has no folded form)
static int gemm_launch_route(int epi, int fold, const GemmArgs* a, const GemmRoute& r, hipStream_t stream) {
    if (r.family == GEMM_ROUTE_MID) return ldt_gemm_mid_launch(epi, fold, a, r, stream);
    if (r.family == GEMM_ROUTE_256_ONE || r.family == GEMM_ROUTE_256_MULTI) return ldt_gemm256_launch(epi, fold, a, r, stream);
    LDT_REQUIRE(r.family == GEMM_ROUTE_V1 && fold == FOLD_NONE, LDT_ESHAPE, "gemm: no kernel takes M=%d N=%d K=%d", a->M, a->N, a->K);
    switch (epi) {
        case EPI_F32: return launch_v1<EPI_F32>(a, r, stream);
        case EPI_BF16: return launch_v1<EPI_BF16>(a, r, stream);
        case EPI_GELU_BF16: return launch_v1<EPI_GELU_BF16>(a, r, stream);
        case EPI_RELU_BF16: return launch_v1<EPI_RELU_BF16>(a, r, stream);
        case EPI_RESID_F32: return launch_v1<EPI_RESID_F32>(a, r, stream);
    }
    ldt_set_error("gemm: unknown epilogue %d", epi);
    return LDT_EARG;
}

int ldt_gemm_launch(int epi, const GemmArgs* a, hipStream_t stream) {
    LDT_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, LDT_ESHAPE, "gemm: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
    LDT_REQUIRE(a->K % BK == 0, LDT_ESHAPE, "gemm: K=%d must be a multiple of %d (pad activations/weights)", a->K, BK);
    if (const int rc = gemm_check_operands("gemm", false, epi, a)) return rc;
    return gemm_launch_route(epi, FOLD_NONE, a, ldt_gemm_decide(epi, a, 0), stream);
}

// The LN-folded launches: producer (EPI_RESID_F32: also writes xs and the row statistics) or consumer (EPI_BF16 / EPI_GELU_BF16: reads them).
// stats_parts says which statistics layout the caller's buffers use: K / 32 parts (N / 32 for the producer) are the mid-size tile kernel's
// (ldt_gemm_lnfold_mid_route), anything else means K / 256 (N / 256), the 256-tile kernel's.
int ldt_gemm_lnfold_launch(int epi, const GemmArgs* a, hipStream_t stream) {
    const bool producer = epi == EPI_RESID_F32;
    const int granule = (a->stats_parts > 0 && a->stats_parts * 32 == (producer ? a->N : a->K)) ? 32 : 256;
    if (granule == 32) LDT_REQUIRE(a->M > 0 && a->M % 128 == 0 && a->N % 64 == 0 && a->K >= 128 && a->K % BK == 0, LDT_ESHAPE,
                                   "gemm_lnfold (mid route): M=%d must be a multiple of 128, N=%d of 64, K=%d >= 128, K %% 64 == 0", a->M, a->N, a->K);
    else LDT_REQUIRE(a->M > 0 && a->N > 0 && a->K >= 256 && a->M % 256 == 0 && a->N % 256 == 0 && a->K % BK == 0, LDT_ESHAPE,
                     "gemm_lnfold: M=%d N=%d must be multiples of 256 and K=%d >= 256, K %% 64 == 0", a->M, a->N, a->K);
    if (const int rc = gemm_check_operands("gemm_lnfold", true, epi, a)) return rc;
    if (producer) {
        LDT_REQUIRE(a->xs && a->ln_scale && a->stats_out && a->ldxs % 4 == 0 && a->ldxs >= a->N && ldt_aligned16(a->xs) &&
                    ldt_aligned16(a->ln_scale) && a->ln_step_stride % 4 == 0 && ldt_aligned16(a->stats_out), LDT_EARG,
                    "gemm_lnfold: producer needs xs / ln_scale / stats_out (16-byte aligned)");
    } else {
        LDT_REQUIRE(epi == EPI_BF16 || epi == EPI_GELU_BF16, LDT_EARG, "gemm_lnfold: epilogue %d has no folded form", epi);
        LDT_REQUIRE(a->stats_in && a->fold_S && a->fold_C && ldt_aligned16(a->stats_in) && ldt_aligned16(a->fold_S) && ldt_aligned16(a->fold_C) &&
                    a->fold_step_stride % 4 == 0, LDT_EARG, "gemm_lnfold: consumer needs stats_in, fold_S, fold_C (16-byte aligned)");
        if (granule == 32) LDT_REQUIRE(a->stats_parts <= 32, LDT_ESHAPE, "gemm_lnfold (mid route): K=%d > 1024 input channels", a->K);
        else LDT_REQUIRE(a->stats_parts >= 1 && a->stats_parts <= 4 && a->stats_parts * 256 == a->K, LDT_EARG,
                         "gemm_lnfold: consumer needs stats_in[K/256 <= 4][M][2] (or [K/32][M][2] for the small-batch kernels); K=%d parts=%d", a->K, a->stats_parts);
    }
    const GemmRoute r = ldt_gemm_decide(epi, a, granule);
    LDT_REQUIRE(r.family != GEMM_ROUTE_NONE, LDT_ESHAPE, "gemm_lnfold: no kernel with statistics per %d columns takes M=%d N=%d K=%d as a %s",
                granule, a->M, a->N, a->K, producer ? "producer" : "consumer");
    return gemm_launch_route(epi, producer ? FOLD_PRODUCER : FOLD_CONSUMER, a, r, stream);
}
