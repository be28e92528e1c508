// The 256-row-tile kernels (gfx950): the persistent 256 x 256 GEMM, the fused QKV projection + self-attention on 256 x 192 tiles, and
// their launchers.  Layout, phases and the shared machinery: gemm256_tile.h.
#include <stdlib.h>

#include <atomic>

#include "gemm256_tile.h"
#include "attn_tile.h"

// =================================================================================================
// Y = epilogue(X . W^T + bias) on persistent 256 x 256 tiles; the request schedule per wave and K-tile s:
//     p0: W(s+1) x4          wait vmcnt(4):  xb(s) landed                   (behind it: the four pieces just requested)
//     p1: xa(s+1) x2
//     p2: xb(s+1) x2
//     p3:                    wait vmcnt(2):  W(s+1) and xa(s+1) landed      (behind them: xb(s+1))
// At every tile start K-tiles 0 AND 1 of the tile are already requested (prologue; later: before the previous tile's epilogue stores —
// in-order VMEM retirement makes every request issued AFTER an epilogue's stores wait for them, a 128 KiB tile drains in 2.5-5 us; this
// way the first requests behind the stores, K-tile 2, are needed 8 phases after the epilogue instead of 4).  So a tile's first K-tile
// (KT_FIRST) requests nothing, and KT_FIRST / KT_SECOND count the previous epilogue's stores (EPI_VMEM) into their waits.
//
// XRING = 1: the one-tile-per-workgroup residual form (GEMM_ROUTE_256_ONE): residual rows through the idle operand ring (g256_epilogue_staged),
// and the tile loop ends behind the first tile.
//
// KLONG is a NAME TAG only (same code): the one-tile residual GEMMs are launched as <.., .., 1, 0, 1> when K >= 2048 (mlp.out) and as
// <.., .., 1, 0, 0> otherwise (fc_o), so that rocprofv3 / PMC summaries price the headline's dominant kernel under a symbol of its own.
// RESERVED0 is always 0 (a retired variant's slot): it keeps the symbols five-argument, as the profiles and bench.py's kernel filter spell them.
template <int EPI, int FOLD = FOLD_NONE, int XRING = 0, int RESERVED0 = 0, int KLONG = 0>
__global__ __launch_bounds__(512) void gemm_bf16_nt_256f_kernel(const GemmArgs a) {
    static_assert(RESERVED0 == 0, "the fourth template argument is a placeholder");
    extern __shared__ __attribute__((aligned(16))) char smem2[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wn = wave & 3;
    const int lrow = lane & 15, lchk = lane >> 4;
    const int nkt = a.K >> 6;

    const Tile256List tl(a.M / 256, a.N / 256, a.group_m, gridDim.x, blockIdx.x);
    if (tl.count == 0) return;
    auto tile_of = [&](int it, int& m0, int& n0) {
        int tm, tn;
        tl.tile(it, tm, tn);
        m0 = tm * 256; n0 = tn * 256;
    };

    Stream256<4, 256> S(a, wave, lane);                         // W: 32 pieces per K-tile, 4 per wave
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = (wave * 4 + q) * 8 + (lane >> 3);
        S.wvo[q] = r * (int)a.ldw * 2 + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
        S.wds[q] = G256_W_OFF + (wave * 4 + q) * 1024;
    }
    int gk = 0;                                                          // global K-tile counter of the CONSUMER (buffer = gk & 1)
    S.seek(a, tl, 0);

    // step-indexed (cache-cold) epilogue vectors of the FIRST tile, fetched ahead of everything else
    const float* gate = a.gate;
    if (EPI == EPI_RESID_F32 && gate && a.step_ptr) gate += (long)(*a.step_ptr) * a.gate_step_stride;
    const int step = ((FOLD != FOLD_NONE) && a.step_ptr) ? *a.step_ptr : 0;
    const float* ln_scale = (FOLD == FOLD_PRODUCER) ? a.ln_scale + (long)step * a.ln_step_stride : nullptr;
    const float* fold_S = (FOLD == FOLD_CONSUMER) ? a.fold_S + (long)step * a.fold_step_stride : nullptr;
    const float* fold_C = (FOLD == FOLD_CONSUMER) ? a.fold_C + (long)step * a.fold_step_stride : nullptr;
    f32x4 g4_pre = {1.f, 1.f, 1.f, 1.f}, sc4_pre = {0.f, 0.f, 0.f, 0.f};
    const bool pre_ok = (EPI == EPI_RESID_F32) && gate && a.gate_sample_stride == 0;
    if (EPI == EPI_RESID_F32) {
        int m0, n0;
        tile_of(0, m0, n0);
        if (pre_ok) g4_pre = *reinterpret_cast<const f32x4*>(gate + n0 + wn * 64 + (lane & 15) * 4);
        if (FOLD == FOLD_PRODUCER) sc4_pre = *reinterpret_cast<const f32x4*>(ln_scale + n0 + wn * 64 + (lane & 15) * 4);
    }

    // prologue: K-tile 0 -> buffer 0, K-tile 1 -> buffer 1
    S.issue_w(smem2); S.issue_xa(smem2); S.issue_xb(smem2); S.advance(a, tl);
    S.issue_w(smem2 + G256_BUF_BYTES); S.issue_xa(smem2 + G256_BUF_BYTES); S.issue_xb(smem2 + G256_BUF_BYTES); S.advance(a, tl);
    asm volatile("s_waitcnt vmcnt(10)" ::: "memory");                    // W + xa of K-tile 0 landed (this wave's pieces)
    G256_BARRIER();
    if (EPI == EPI_RESID_F32) asm volatile("" : "+v"(g4_pre), "+v"(sc4_pre));

    const KTileLanes ln(grp, wn * 64, lrow, lchk);
    constexpr int EPI_VMEM = (EPI == EPI_BF16 || EPI == EPI_GELU_BF16 || EPI == EPI_RELU_BF16) ? 16
                             : (FOLD == FOLD_PRODUCER) ? 57 : 32;
    char* stage_reg = smem2 + G256_RING_BYTES + wave * 4096;
    bool prev_staged = false;

    for (int it = 0; it < tl.count; ++it) {
        int m0, n0;
        tile_of(it, m0, n0);
        f32x4 acc[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[i][jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (grp == 1) G256_BARRIER();                                    // stagger the two groups by one barrier

        enum { KT_PLAIN = 0, KT_FIRST = 1 /* first K-tile of a tile */, KT_SECOND = 2, KT_FOLD_DMA = 4, KT_FOLD_FINAL = 8 };
        auto ktile = [&](auto flags_c) {
            constexpr int FL = decltype(flags_c)::value;
            constexpr bool SKIP = (FL & KT_FIRST) != 0;                  // K-tile 1 of this tile was requested ahead: this K-tile requests nothing
            char* nb = smem2 + ((gk + 1) & 1) * G256_BUF_BYTES;          // buffer being refilled (K-tile gk + 1)
            auto request = [&](auto ph) {
                constexpr int PH = decltype(ph)::value;
                if constexpr (PH == 0) {                                 // DMA: W of the next K-tile; wait: this K-tile's xb
                    if (!SKIP) S.issue_w(nb);
                    if (FL & KT_FOLD_DMA) {
                        g256_fold_stats_dma(a, m0, wave, lane, stage_reg);
                        if (wave < 4 && lane < 32) {
                            const float* src = (wave < 2 ? fold_S : fold_C) + n0 + (wave & 1) * 128 + lane * 4;
                            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                             (__attribute__((address_space(3))) void*)(stage_reg + G256_SC_OFF), 16, 0, 0);
                        }
                    }
                    if ((FL & KT_FOLD_FINAL) && wave < 4) g256_fold_finalize(smem2 + G256_RING_BYTES, tid, a.stats_parts, a.K);
                    // requests issued after this K-tile's xb (the data this wait is for): W of the next K-tile / KT_FIRST: the whole
                    // pre-requested K-tile 1; after an epilogue also its stores (clamped to the 6-bit counter: only stricter)
                    constexpr int P0W = SKIP ? 8 : 4;
                    constexpr bool AFTER_EPI = (FL & (KT_FIRST | KT_SECOND)) != 0;
                    if (AFTER_EPI && prev_staged) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P0W + EPI_VMEM > 63 ? 63 : P0W + EPI_VMEM) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P0W) : "memory");
                } else if constexpr (PH == 1) {                          // DMA: xa of the next K-tile
                    if (!SKIP) S.issue_xa(nb);
                } else if constexpr (PH == 2) {                          // DMA: xb of the next K-tile
                    if (!SKIP) { S.issue_xb(nb); S.advance(a, tl); }
                } else {                                                 // wait: W + xa of the next K-tile
                    if (SKIP && prev_staged) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 + EPI_VMEM > 63 ? 63 : 2 + EPI_VMEM) : "memory");   // W + xa of K-tile 1: older than the stores
                    else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                }
            };
            ktile256<4>(smem2 + (gk & 1) * G256_BUF_BYTES, ln, acc, request);
            ++gk;
        };
#define KTL(f) std::integral_constant<int, (f)>{}
        if (FOLD == FOLD_CONSUMER) {                                     // K >= 256 (launcher): at least 4 K-tiles
            ktile(KTL(KT_FIRST)); ktile(KTL(KT_FOLD_DMA | KT_SECOND)); ktile(KTL(KT_PLAIN)); ktile(KTL(KT_FOLD_FINAL));
            for (int kt = 4; kt < nkt; ++kt) ktile(KTL(KT_PLAIN));
        } else {
            ktile(KTL(KT_FIRST)); ktile(KTL(KT_SECOND));                 // (launcher: at least 2 K-tiles)
            for (int kt = 2; kt < nkt; ++kt) ktile(KTL(KT_PLAIN));
        }
#undef KTL
        if (grp == 0) G256_BARRIER();                                    // un-stagger: both groups run the epilogue together

        prev_staged = true;                                              // interior, aligned tiles only (launcher)
        if (!XRING) {                                                    // K-tile 1 of the next tile -> the buffer the last K-tile has just left (all waves are past its reads)
            char* pb = smem2 + ((gk + 1) & 1) * G256_BUF_BYTES;
            S.issue_w(pb); S.issue_xa(pb); S.issue_xb(pb); S.advance(a, tl);
        }
        if (XRING) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            G256_BARRIER();
            g256_epilogue_staged<EPI, FOLD, 1>(a, acc, m0, n0, grp, wn, lane, lrow, lchk, gate, stage_reg, smem2 + G256_RING_BYTES, ln_scale,
                                               true, g4_pre, sc4_pre, smem2 + wave * 16384);
            break;                                                       // (GEMM_ROUTE_256_ONE: nothing of the stream state is live past here: -13 spilled VGPRs)
        } else
            g256_epilogue_staged<EPI, FOLD>(a, acc, m0, n0, grp, wn, lane, lrow, lchk, gate, stage_reg, smem2 + G256_RING_BYTES, ln_scale,
                                            it == 0 && (pre_ok || FOLD == FOLD_PRODUCER), g4_pre, sc4_pre);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                     // drain the (unused) tail requests before exit
}

// =================================================================================================
// QKV projection + self-attention in ONE launch at the bench shape (256-token samples, head dim 64): the same main loop on 256 x 192 tiles.
// A tile is [q | k | v] of ONE head for ONE whole sample (rows = the sample's 256 tokens; the tile's W rows / bias / S | C columns are three
// 64-wide segments, `hidden` apart), so when its main loop ends the workgroup holds everything that (sample, head)'s attention needs:
//   * the finished projections (bias or LN-folded form applied) go to LDS as bf16 rows in the whole-head attention kernel's layouts —
//     q into the staging areas (32 KB), k | v into the operand buffer the last K-tile has just left (64 KB); the OTHER buffer keeps
//     receiving the next tile's first K-tile meanwhile (so this form does not request a tile's second K-tile ahead: that needs both buffers);
//   * wave w (8 of them) then runs query rows [32 w, +32) over the four 64-key tiles with attn_tile_joint — the math, operand layouts and
//     summation order of attn_fwd_head_kernel — and stores O / l through its own (then dead) q rows: attn_o[B][H][256][64].
// The q | k | v rows never reach HBM (96 MB written + 96 MB read per block at B = 64) and the attention launch of the block is gone.
// Wave layout in the main loop: grp = wave >> 2 owns rows [128 grp, +128), wn = wave & 3 owns tile columns [48 wn, +48): 12 MFMAs per
// phase.  Requests per wave and K-tile s:  p0: W(s+1) x3, wait vmcnt(3)    p1: xa(s+1) x2    p2: xb(s+1) x2    p3: wait vmcnt(2).
template <int FOLD>   // FOLD_NONE (block 0: bias) | FOLD_CONSUMER
__global__ __launch_bounds__(512) void gemm_qkv_attn256_kernel(const GemmArgs a) {
    static_assert(FOLD == FOLD_NONE || FOLD == FOLD_CONSUMER, "qkv+attention: plain or LN-folded consumer");
    extern __shared__ __attribute__((aligned(16))) char smem2[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, wn = wave & 3;
    const int lrow = lane & 15, lchk = lane >> 4;
    const int nkt = a.K >> 6;
    const int hidden = a.N / 3, heads = hidden / 64;

    const Tile256List tl(a.M / 256, heads, a.group_m, gridDim.x, blockIdx.x);   // tile = (sample, head)
    if (tl.count == 0) return;
    auto tile_of = [&](int it, int& m0, int& hd) {
        int tm;
        tl.tile(it, tm, hd);
        m0 = tm * 256;
    };

    Stream256<3, 64> S(a, wave, lane);                          // W: 24 pieces per K-tile, 3 per wave
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int pj = wave * 3 + q;                                     // piece pj = rows [8 pj, +8) of the tile's 192 = segment pj / 8
        const int r = pj * 8 + (lane >> 3);                              // row of the tile's W image
        const int gr = (pj >> 3) * hidden + (r & 63);                    // row of W relative to the head's first q row
        S.wvo[q] = gr * (int)a.ldw * 2 + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
        S.wds[q] = G256_W_OFF + pj * 1024;
    }
    int gk = 0;
    S.seek(a, tl, 0);
    const int step = ((FOLD != FOLD_NONE) && a.step_ptr) ? *a.step_ptr : 0;
    const float* fold_S = (FOLD == FOLD_CONSUMER) ? a.fold_S + (long)step * a.fold_step_stride : nullptr;
    const float* fold_C = (FOLD == FOLD_CONSUMER) ? a.fold_C + (long)step * a.fold_step_stride : nullptr;

    S.issue_w(smem2); S.issue_xa(smem2); S.issue_xb(smem2); S.advance(a, tl);
    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");                     // W + xa landed (this wave's pieces)
    G256_BARRIER();

    const KTileLanes ln(grp, wn * 48, lrow, lchk);
    constexpr int EPI_VMEM = 4;                                          // VMEM ops of the epilogue behind the stream's last request: the four O stores
    bool prev_staged = false;
    const int r32 = lane & 31, hh = lane >> 5;
    AttnLaneOffs<64> lo;
    lo.init(lane);

    for (int it = 0; it < tl.count; ++it) {
        int m0, hd;
        tile_of(it, m0, hd);
        f32x4 acc[3][8];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) acc[i][jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // (block 0: the bias of this lane's columns, fetched ahead of the main loop so that the epilogue issues no load)
        f32x4 add4[3];
#pragma unroll
        for (int ni = 0; ni < 3; ++ni) {
            const int c = wn * 48 + ni * 16 + lchk * 4;
            add4[ni] = (FOLD == FOLD_NONE && a.bias) ? *reinterpret_cast<const f32x4*>(a.bias + (c >> 6) * hidden + hd * 64 + (c & 63)) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        if (grp == 1) G256_BARRIER();                                    // stagger the two groups by one barrier

        enum { KT_PLAIN = 0, KT_FIRST = 1, KT_FOLD_DMA = 4, KT_FOLD_FINAL = 8 };
        auto ktile = [&](auto flags_c) {
            constexpr int FL = decltype(flags_c)::value;
            char* nb = smem2 + ((gk + 1) & 1) * G256_BUF_BYTES;
            auto request = [&](auto ph) {
                constexpr int PH = decltype(ph)::value;
                if constexpr (PH == 0) {
                    S.issue_w(nb);
                    if (FL & KT_FOLD_DMA) {
                        char* stage_reg = smem2 + G256_RING_BYTES + wave * 4096;
                        g256_fold_stats_dma(a, m0, wave, lane, stage_reg);
                        if (wave < 6 && lane < 16) {                     // S segments -> waves 0-2's areas, C segments -> waves 3-5's
                            const int seg = wave < 3 ? wave : wave - 3;
                            const float* src = (wave < 3 ? fold_S : fold_C) + seg * hidden + hd * 64 + lane * 4;
                            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                             (__attribute__((address_space(3))) void*)(stage_reg + G256_SC_OFF), 16, 0, 0);
                        }
                    }
                    if ((FL & KT_FOLD_FINAL) && wave < 4) g256_fold_finalize(smem2 + G256_RING_BYTES, tid, a.stats_parts, a.K);
                    constexpr int P0W = 3;                               // this K-tile's xb landed; behind it: the W pieces just requested (+ the O stores)
                    if ((FL & KT_FIRST) && prev_staged) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P0W + EPI_VMEM) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P0W) : "memory");
                } else if constexpr (PH == 1) {
                    S.issue_xa(nb);
                } else if constexpr (PH == 2) {
                    S.issue_xb(nb); S.advance(a, tl);
                } else {
                    asm volatile("s_waitcnt vmcnt(2)" ::: "memory");     // W + xa of the next K-tile
                }
            };
            ktile256<3>(smem2 + (gk & 1) * G256_BUF_BYTES, ln, acc, request);
            ++gk;
        };
#define KTL(f) std::integral_constant<int, (f)>{}
        if (FOLD == FOLD_CONSUMER) {                                     // K >= 256 (launcher): at least 4 K-tiles
            ktile(KTL(KT_FIRST)); ktile(KTL(KT_FOLD_DMA)); ktile(KTL(KT_PLAIN)); ktile(KTL(KT_FOLD_FINAL));
            for (int kt = 4; kt < nkt; ++kt) ktile(KTL(KT_PLAIN));
        } else {
            ktile(KTL(KT_FIRST));
            for (int kt = 1; kt < nkt; ++kt) ktile(KTL(KT_PLAIN));
        }
#undef KTL
        if (grp == 0) G256_BARRIER();                                      // un-stagger: both groups run the epilogue together
        prev_staged = true;

        // ---- epilogue 1: finish the projection; bf16 rows -> q (staging areas) | k | v (the buffer the last K-tile has just left)
        char* stage_base = smem2 + G256_RING_BYTES;
        char* kvb = smem2 + ((gk + 1) & 1) * G256_BUF_BYTES;               // K: [256 keys][128 B] at + 0, V at + 32 KiB (the other buffer holds the next tile's K-tile 0)
        f32x4 s4[3];
        float rr[8], nm[8];
        if (FOLD == FOLD_CONSUMER) {
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) {
                const int R = grp * 128 + mi * 16 + lrow;
                const f32x2 t = *reinterpret_cast<const f32x2*>(stage_base + (R >> 7) * 4096 + G256_STATS_OFF + (R & 127) * 8);
                rr[mi] = t[0]; nm[mi] = t[1];
            }
#pragma unroll
            for (int ni = 0; ni < 3; ++ni) {
                const int c = wn * 48 + ni * 16 + lchk * 4;
                s4[ni] = *reinterpret_cast<const f32x4*>(stage_base + (c >> 6) * 4096 + G256_SC_OFF + (c & 63) * 4);
                add4[ni] = *reinterpret_cast<const f32x4*>(stage_base + (3 + (c >> 6)) * 4096 + G256_SC_OFF + (c & 63) * 4);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            G256_BARRIER();                                                // every wave has its statistics / S | C: the staging areas become the q rows
        }
#pragma unroll
        for (int mi = 0; mi < 8; ++mi) {
            const int R = grp * 128 + mi * 16 + lrow;
            const int swr = (R >> 1) & 7;
#pragma unroll
            for (int ni = 0; ni < 3; ++ni) {
                f32x4 v = acc[ni][mi];
                if (FOLD == FOLD_CONSUMER) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = v[r] * rr[mi] + (nm[mi] * s4[ni][r] + add4[ni][r]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] += add4[ni][r];
                }
                const bf16x4 pk = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                const int c = wn * 48 + ni * 16 + lchk * 4, seg = c >> 6, cc = c & 63;
                const int sz = seg == 2 ? ((R >> 1) & 1) << 2 : swr;        // V rows: the transposed-read swizzle; q, k rows: the row-read one
                char* dst = (seg == 0 ? stage_base : kvb + (seg - 1) * 32768) + R * 128 + (((cc >> 3) ^ sz) << 4) + (cc & 7) * 2;
                *reinterpret_cast<bf16x4*>(dst) = pk;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        G256_BARRIER();                                                    // the head's q | k | v are complete

        // ---- epilogue 2: wave w = query rows [32 w, +32) over the four key tiles (attn_fwd_head_kernel's loop)
        {
            const int q0 = wave * 32;
            bf16x8 qf[4];
#pragma unroll
            for (int sI = 0; sI < 4; ++sI)
                qf[sI] = *reinterpret_cast<const bf16x8*>(stage_base + (q0 + r32) * 128 + (((hh + 2 * sI) ^ ((r32 >> 1) & 7)) << 4));
            f32x16 oacc[2];
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) oacc[d][i] = 0.f;
            float m_run = -INFINITY, l_run = 0.f;
            // software-pipelined over the four key tiles: the S^T MFMAs of tile t + 1 are issued before the softmax of tile t, so the matrix
            // pipe works under this wave's own softmax VALU (two score accumulator pairs; same math and summation order per tile)
            f32x16 sa0, sa1, sb0, sb1;
            const char* Kt = kvb;
            const char* Vt = kvb + 32768;
            const float csc = a.attn_scale_log2e;
            attn_scores<64>(Kt, qf, sa0, sa1, lo);
            __builtin_amdgcn_sched_barrier(0);
            attn_scores<64>(Kt + 8192, qf, sb0, sb1, lo);
            __builtin_amdgcn_sched_barrier(0);
            attn_softmax_pv<64>(Vt, sa0, sa1, oacc, m_run, l_run, 0, 256, hh, csc, lo);
            __builtin_amdgcn_sched_barrier(0);
            attn_scores<64>(Kt + 2 * 8192, qf, sa0, sa1, lo);
            __builtin_amdgcn_sched_barrier(0);
            attn_softmax_pv<64>(Vt + 8192, sb0, sb1, oacc, m_run, l_run, 64, 256, hh, csc, lo);
            __builtin_amdgcn_sched_barrier(0);
            attn_scores<64>(Kt + 3 * 8192, qf, sb0, sb1, lo);
            __builtin_amdgcn_sched_barrier(0);
            attn_softmax_pv<64>(Vt + 2 * 8192, sa0, sa1, oacc, m_run, l_run, 128, 256, hh, csc, lo);
            __builtin_amdgcn_sched_barrier(0);
            attn_softmax_pv<64>(Vt + 3 * 8192, sb0, sb1, oacc, m_run, l_run, 192, 256, hh, csc, lo);
            // O / l through this wave's own q rows (dead: the fragments are in registers), whole rows out
            char* ost = stage_base + q0 * 128;
            const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32, 64));
#pragma unroll
            for (int d = 0; d < 2; ++d)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int chn = d * 4 + g;
                    const bf16x4 pk = {(bf16_t)(oacc[d][4 * g + 0] * inv), (bf16_t)(oacc[d][4 * g + 1] * inv),
                                       (bf16_t)(oacc[d][4 * g + 2] * inv), (bf16_t)(oacc[d][4 * g + 3] * inv)};
                    *reinterpret_cast<bf16x4*>(ost + r32 * 128 + ((chn ^ (r32 & 7)) << 4) + hh * 8) = pk;
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            bf16_t* ob = a.attn_o + (((long)(m0 >> 8) * heads + hd) * 256 + q0) * 64;
#pragma unroll
            for (int p4 = 0; p4 < 4; ++p4) {
                const int row = p4 * 8 + (lane >> 3), ch = lane & 7;
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(ost + row * 128 + ((ch ^ (row & 7)) << 4));
                *reinterpret_cast<bf16x8*>(ob + (long)row * 64 + ch * 8) = v;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        G256_BARRIER();                                                    // k | v (the next K-tile 1's buffer) and the staging areas are free again
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// rows per group of the tile order (tools/dbg sets it at run time; LDT_GEMM_GM at start-up)
static std::atomic<int> g_group_m{-1};
extern "C" int ldt_dbg_gemm_group_m(int32_t gm) { g_group_m.store(gm); return LDT_OK; }
static std::atomic<int> g_dbg_epi{-1};
extern "C" int ldt_dbg_gemm_epi(int32_t bits) { g_dbg_epi.store(bits); return LDT_OK; }   // tools/dbg/epi_ablate.py

// The 256-tile kernels take interior, aligned tiles only (M, N multiples of 256, K a multiple of 64 with >= 2 K-tiles, 16-byte rows)
bool ldt_gemm256_takes(int epi, const GemmArgs* a) {
    return a->K % 64 == 0 && a->K >= 128 && a->M % 256 == 0 && a->N % 256 == 0 && a->ldo % 8 == 0 &&
           (epi != EPI_RESID_F32 || (a->ldr % 4 == 0 && (!a->gate || a->gate_sample_stride % 4 == 0))) &&
           (epi != EPI_RELU_BF16 || !a->skip || a->lds_ % 4 == 0);
}

template <int EPI, int FOLD = FOLD_NONE>
static int launch_256(const GemmArgs* a_in, const GemmRoute& route, hipStream_t stream) {
    // LDT_GEMM_GM overrides the tile order's group size (LDT_QKV_GM: the fused QKV + attention kernel alone)
    static const int gm_env = getenv("LDT_GEMM_GM") ? atoi(getenv("LDT_GEMM_GM")) : -1;
    const int gm_dbg = g_group_m.load();
    GemmArgs a_copy = *a_in;
    a_copy.group_m = gm_dbg >= 0 ? gm_dbg : gm_env >= 0 ? gm_env : gemm256_default_group_m(a_in->M / 256, a_in->N / 256);
    // residual rows of a one-tile workgroup through the operand ring (g256_epilogue_staged XRING, kernel <.., .., 1>): needs the exact VMEM op
    // count of the epilogue (no per-sample gate loads, no debug skips) and 16-B aligned rows.  LDT_RESID_RING=0: A/B runs.
    static const bool xring_on = !(getenv("LDT_RESID_RING") && atoi(getenv("LDT_RESID_RING")) == 0);
    const bool xring = (EPI == EPI_RESID_F32 && xring_on && a_in->resid && ldt_aligned16(a_in->resid) && (!a_in->gate || a_in->gate_sample_stride == 0));
    static const int dbg_env = getenv("LDT_DBG_EPI") ? atoi(getenv("LDT_DBG_EPI")) : 0;
    a_copy.dbg = g_dbg_epi.load() >= 0 ? g_dbg_epi.load() : dbg_env;
    const GemmArgs* a = &a_copy;
    LDT_REQUIRE(ldt_gemm256_takes(EPI, a), LDT_ESHAPE, "gemm256: M=%d N=%d must be multiples of 256, K=%d of 64 (>= 128), rows 16-byte aligned", a->M, a->N, a->K);
    const int grid = route.grid;                                         // one persistent workgroup per CU (or per CU of this stream's share): ldt_gemm_decide
    if constexpr (EPI == EPI_RESID_F32) {
        if (xring && route.family == GEMM_ROUTE_256_ONE && a->dbg == 0) {   // no workgroup has a second tile: the ring is idle in its epilogue
            const bool klong = a->K >= 2048;                             // symbol tag: mlp.out vs fc_o (see the kernel's template comment)
#define LAUNCH_XR(KL)                                                                                                             \
    do {                                                                                                                          \
        LDT_ENSURE_LDS((&gemm_bf16_nt_256f_kernel<EPI, FOLD, 1, 0, KL>), G256_LDS_BYTES, "gemm256f");                              \
        hipLaunchKernelGGL((gemm_bf16_nt_256f_kernel<EPI, FOLD, 1, 0, KL>), dim3(grid), dim3(512), G256_LDS_BYTES, stream, *a);   \
    } while (0)
            if (klong) LAUNCH_XR(1);
            else LAUNCH_XR(0);
#undef LAUNCH_XR
            return ldt_check_launch("gemm_bf16_nt_256f");
        }
    }
    LDT_ENSURE_LDS((&gemm_bf16_nt_256f_kernel<EPI, FOLD>), G256_LDS_BYTES, "gemm256f");
    hipLaunchKernelGGL((gemm_bf16_nt_256f_kernel<EPI, FOLD>), dim3(grid), dim3(512), G256_LDS_BYTES, stream, *a);
    return ldt_check_launch("gemm_bf16_nt_256f");
}

int ldt_gemm256_launch(int epi, int fold, const GemmArgs* a, const GemmRoute& r, hipStream_t stream) {
    if (fold == FOLD_PRODUCER && epi == EPI_RESID_F32) return launch_256<EPI_RESID_F32, FOLD_PRODUCER>(a, r, stream);
    if (fold == FOLD_CONSUMER && epi == EPI_BF16) return launch_256<EPI_BF16, FOLD_CONSUMER>(a, r, stream);
    if (fold == FOLD_CONSUMER && epi == EPI_GELU_BF16) return launch_256<EPI_GELU_BF16, FOLD_CONSUMER>(a, r, stream);
    if (fold == FOLD_NONE) switch (epi) {
        case EPI_F32: return launch_256<EPI_F32>(a, r, stream);
        case EPI_BF16: return launch_256<EPI_BF16>(a, r, stream);
        case EPI_GELU_BF16: return launch_256<EPI_GELU_BF16>(a, r, stream);
        case EPI_RELU_BF16: return launch_256<EPI_RELU_BF16>(a, r, stream);
        case EPI_RESID_F32: return launch_256<EPI_RESID_F32>(a, r, stream);
    }
    ldt_set_error("gemm: unknown epilogue %d", epi);
    return LDT_EARG;
}

// QKV projection + self-attention in one launch at 256 tokens (gemm_qkv_attn256_kernel): head dim 64, N = 3 * hidden (hidden % 64 == 0),
// whole samples (M % 256 == 0), enough (sample, head) tiles to fill 5/8 of the workgroups the launch may use.  `folded`: a = the LN-folded
// consumer's arguments (statistics per 256 columns).  -> true when this kernel took the launch.  LDT_QKV_ATTN256=0: off (A/B).
// The shape part of that rule (also ldt_qkv_attention_route's): reads M, N, K, stats_parts and max_wgs of `g`, no pointer.
bool ldt_gemm_qkv_attn256_takes(const GemmArgs* a_in, int tokens, int head_dim, bool folded) {
    static const bool on = !(getenv("LDT_QKV_ATTN256") && atoi(getenv("LDT_QKV_ATTN256")) == 0);
    const GemmArgs& g = *a_in;
    if (!on || tokens != 256 || head_dim != 64) return false;
    if (g.M <= 0 || g.N <= 0 || g.N % 192 != 0 || (g.N / 3) % 64 != 0 || g.M % 256 != 0 || g.K % 64 != 0 || g.K < (folded ? 256 : 128)) return false;
    if (folded && (g.stats_parts <= 0 || g.stats_parts > 4 || g.stats_parts * 256 != g.K)) return false;
    return ldt_fills_workgroups((long)(g.M / 256) * ((g.N / 3) / 64), g.max_wgs);
}
bool ldt_gemm_qkv_attn256_try(const GemmArgs* a_in, int tokens, int head_dim, bool folded, hipStream_t stream, int* status) {
    const GemmArgs& g = *a_in;
    if (!g.attn_o || !ldt_gemm_qkv_attn256_takes(a_in, tokens, head_dim, folded)) return false;
    if (folded && (!g.stats_in || !g.fold_S || !g.fold_C ||
                   !ldt_aligned16(g.stats_in) || !ldt_aligned16(g.fold_S) || !ldt_aligned16(g.fold_C) || g.fold_step_stride % 4 != 0))
        return false;
    if (!ldt_aligned16(g.X) || !ldt_aligned16(g.W) || !ldt_aligned16(g.attn_o) || (g.bias && !ldt_aligned16(g.bias)) || g.ldx % 8 != 0 || g.ldw % 8 != 0 ||
        g.ldx < g.K || g.ldw < g.K)
        return false;
    const int tm = g.M / 256, tn = (g.N / 3) / 64;
    const long tiles = (long)tm * tn;
    const int lim = ldt_wg_limit(g.max_wgs);
    GemmArgs a = g;
    static const int gm_env = getenv("LDT_QKV_GM") ? atoi(getenv("LDT_QKV_GM")) : getenv("LDT_GEMM_GM") ? atoi(getenv("LDT_GEMM_GM")) : -1;   // tools/dbg
    a.group_m = gm_env >= 0 ? gm_env : gemm256_default_group_m(tm, tn);
    const int grid = tiles < lim ? (int)tiles : lim;
    auto launch = [&]() -> int {
        if (folded) {
            LDT_ENSURE_LDS((&gemm_qkv_attn256_kernel<FOLD_CONSUMER>), G256_LDS_BYTES, "gemm_qkv_attn256");
            hipLaunchKernelGGL((gemm_qkv_attn256_kernel<FOLD_CONSUMER>), dim3(grid), dim3(512), G256_LDS_BYTES, stream, a);
        } else {
            LDT_ENSURE_LDS((&gemm_qkv_attn256_kernel<FOLD_NONE>), G256_LDS_BYTES, "gemm_qkv_attn256");
            hipLaunchKernelGGL((gemm_qkv_attn256_kernel<FOLD_NONE>), dim3(grid), dim3(512), G256_LDS_BYTES, stream, a);
        }
        return ldt_check_launch("gemm_qkv_attn256");
    };
    *status = launch();
    return true;
}
