// Row-panel kernels for the small per-step networks (message decoder / encoder, policy
// hidden layer; reference networks/message.py:20-49, networks/policy.py:12-14).
//
// At R = Na*Nb rows and 64..384 features these layers are a few dozen MFLOP each: far too
// small for a tiled GEMM launch + a LayerNorm launch per layer (each launch is latency
// bound at ~10-20 us).  Here ONE workgroup owns a 16-row panel (kPanelRows) end to end:
//   stage the input rows in LDS (optionally computing the message mean over the other
//   agents on the fly) -> [ X * W^T on the matrix cores, one 16x32 tile per wave, weights
//   streamed straight from L2 (fragment-order copies) -> bias -> LayerNorm + SiLU in the MFMA accumulator layout
//   (cross-lane + cross-wave row reductions) -> next layer's input panel in LDS ] x {1,2}.
// The backward kernel walks the same chain in reverse (LayerNorm/SiLU backward in the tile
// layout, dX GEMMs against the transposed weight copies) and emits per-panel partial sums
// for the LayerNorm affine gradients (fixed order -> deterministic).
#include <stdlib.h>

#include "common.h"
#include "sample.h"

namespace marl {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Workgroup barrier that only waits for LDS traffic: the global stores of saved activations
// issued before it are never read back by this kernel, so there is no reason to drain vmcnt
// (a plain __syncthreads() would wait for every outstanding store: ~1-2 us each time).
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// a product rounded on its own, never contracted into an add that consumes it.  The backward row pass accumulates
// (s1, s2) and (dbeta, dgamma) as pairs whose members are products (dy, dy * g) and products of those; which of them
// the compiler contracts into the sums depends on how it pairs the lanes of each instantiation (the run-time forms pair
// the two sums and contract none) - written out, every instantiation rounds as those do
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float silu_p(float y) { return silu_fast(y); }
__device__ __forceinline__ float silu_grad_p(float y) { return silu_grad_fast(y); }

// 16-row panels: R = Na*Nb = 4096 rows give 256 workgroups (one per CU); the f32 matrix-core
// time of the widest layer (256 -> 384) is ~5 us per panel, half of what a 32-row panel on
// half the CUs would need.
constexpr int kPanelRows = 16;
constexpr int kPanelMaxWaves = 12;  // 768 threads: 170 VGPRs per lane, no spills
constexpr int kPanelMaxCols = 6;    // LayerNorm columns per lane: widths up to 384

__host__ __device__ inline int panel_stride(int k) { return ((k + 15) & ~15) + 4; }

// One wave = one (32-column tile j, K slice s) pair, computed as two 16x16x4 MFMA sub-tiles:
// acc[t] = in[16 x Kslice] (LDS) * W[16 tile rows, Kslice]^T.  Weight fragments come straight
// from global memory (L2), 8 x 16-byte loads (a 64-deep chunk of both sub-tiles) in flight
// per wave; splitting K over waves puts ALL of a layer's weight loads in flight at once.
// The weights are read from their fragment-order copy (panel_frag_index, common.h): each of the eight
// loads of a chunk is 1 KB contiguous over the wave, at lane * 16 B behind a wave-uniform base, and the
// chunk's 8 KB are consecutive.  The copy's padding (rows >= n, columns >= K) is zero and the loads past
// a slice's end are never multiplied, so no address is clamped.
// C/D layout of the 16x16 tile: col = lane & 15, row = 4 * (lane >> 4) + reg.
__device__ __forceinline__ void panel_gemm(f32x4 (&acc)[2], const float* in, int stride,
                                           const float* __restrict__ wfrag, int groups, int j,
                                           int kbeg, int kend, int lane) {
    const int quad = lane >> 4, l16 = lane & 15;
    const float* arow = in + l16 * stride + 4 * quad;
    const int g0 = __builtin_amdgcn_readfirstlane(j * groups + (kbeg >> 4));
    const float* wb = wfrag + (size_t)g0 * 512;  // wave-uniform: tile j, first group of this slice
    const unsigned lo = 4u * (unsigned)lane;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[0][r] = acc[1][r] = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += 64, wb += 4 * 512) {
        float4 b0[4], b1[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b0[i] = *reinterpret_cast<const float4*>(wb + 512 * i + lo);
            b1[i] = *reinterpret_cast<const float4*>(wb + 512 * i + 256 + lo);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (k0 + 16 * i < kend) {
                const float4 a = *reinterpret_cast<const float4*>(arow + k0 + 16 * i);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0[i].x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b1[i].x, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b0[i].y, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1[i].y, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b0[i].z, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b1[i].z, acc[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b0[i].w, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b1[i].w, acc[1], 0, 0, 0);
            }
        }
    }
}

// K-slice partial tiles -> slice 0's accumulator (fixed order).  part: [(ks-1) * nt][64][8]
__device__ __forceinline__ void panel_ksum(f32x4 (&acc)[2], float* part, int nt, int ks, int j, int s,
                                           int lane, bool active) {
    if (ks > 1) {
        if (active && s > 0) {
            float* p = part + ((size_t)((s - 1) * nt + j) * 64 + lane) * 8;
            *reinterpret_cast<float4*>(p) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
            *reinterpret_cast<float4*>(p + 4) = make_float4(acc[1][0], acc[1][1], acc[1][2], acc[1][3]);
        }
        lds_barrier();
        if (active && s == 0) {
            for (int q = 1; q < ks; ++q) {
                const float* p = part + ((size_t)((q - 1) * nt + j) * 64 + lane) * 8;
                const float4 u = *reinterpret_cast<const float4*>(p);
                const float4 v = *reinterpret_cast<const float4*>(p + 4);
                acc[0][0] += u.x;
                acc[0][1] += u.y;
                acc[0][2] += u.z;
                acc[0][3] += u.w;
                acc[1][0] += v.x;
                acc[1][1] += v.y;
                acc[1][2] += v.z;
                acc[1][3] += v.w;
            }
        }
    }
}

__host__ __device__ inline int panel_ksplit(int K, int nt, int nwaves) {
    const int K16 = (K + 15) & ~15;
    int ks = nwaves / nt;
    const int want = (K16 + 63) / 64;
    ks = ks < want ? ks : want;
    return ks < 1 ? 1 : ks;
}

constexpr int panel_kper_c(int K16, int ks) { return (((K16 + ks - 1) / ks) + 15) & ~15; }
constexpr int panel_ksplit_c(int K, int nt, int nwaves) {
    const int K16 = (K + 15) & ~15, want = (K16 + 63) / 64;
    int ks = nwaves / nt;
    ks = ks < want ? ks : want;
    return ks < 1 ? 1 : ks;
}
constexpr int panel_stride_c(int k) { return ((k + 15) & ~15) + 4; }
constexpr int cmax(int a, int b) { return a > b ? a : b; }

// ---------------------------------------------------------------------------
// Shape descriptors.  Both kernels are written once over a shape class SH: PanelDyn reads every width, the layer
// count, the wave count and the LDS offsets from the launch's descriptors (the form every shape can take);
// PanelNet / PanelBwdNet carry them as constants (the forms of the README dimensions, see launch_panel_fwd /
// launch_panel_bwd): the layer loop is unrolled, and slice bounds, strides, divisors and column guards fold.
// The arithmetic is the same source either way - the results are the run-time form's, bit for bit.
// ---------------------------------------------------------------------------
struct PanelDyn {
    static constexpr bool kStatic = false, kByBatch = false;
    static constexpr int kLayers = kPanelMaxLayers, kSoft = 0, kWaves = 0, kK0 = 0, kAggAt = 0, kKLast = 0;
    static constexpr int off_e = 0, off_prm = 0, off_colp = 0, off_part = 0, off_rowmap = 0;
    static constexpr int n(int) { return 0; }
    static constexpr int k(int) { return 0; }
};
// forward: WAVES of the launch's plan, input width K0, widths N...; AGG_AT: the in-panel message mean in front of
// that layer (0: none; implies by_batch rows).  SOFT > 0: the launch may stop after SOFT layers (P.nlayers == SOFT,
// then without the aggregation site): the last step's encoder-only form inside the same instantiation.
template <int WAVES, int K0, int AGG_AT, int SOFT, int... N>
struct PanelNet {
    static constexpr bool kStatic = true, kByBatch = AGG_AT > 0;
    static constexpr int kLayers = (int)sizeof...(N), kSoft = SOFT, kWaves = WAVES, kK0 = K0, kAggAt = AGG_AT;
    static constexpr int n(int l) {
        constexpr int w[] = {N...};
        return w[l];
    }
    static constexpr int k(int l) { return l == 0 ? K0 : n(l - 1); }
    // X: the input and the outputs of the odd layers; Y: the outputs of the even layers (panel_fwd_plan)
    static constexpr int s0(int layers) {
        int v = kPanelRows * panel_stride_c(K0);
        for (int l = 1; l < layers; l += 2) v = cmax(v, kPanelRows * panel_stride_c(n(l)));
        return v;
    }
    static constexpr int s1(int layers) {
        int v = 0;
        for (int l = 0; l < layers; l += 2) v = cmax(v, kPanelRows * panel_stride_c(n(l)));
        return v;
    }
    static constexpr bool ok() {
        for (int l = 0; l < kLayers; ++l) {
            const int nt = (n(l) + 31) >> 5, K16 = (k(l) + 15) & ~15, ks = panel_ksplit_c(k(l), nt, WAVES);
            if (nt * ks > WAVES || (ks - 1) * panel_kper_c(K16, ks) >= K16) return false;  // (no empty slice)
            if ((n(l) & 15) || (k(l) & 15) || n(l) > 64 * kPanelMaxCols) return false;
        }
        return WAVES >= 4 && WAVES <= kPanelMaxWaves && (SOFT == 0 || (s0(SOFT) == s0(kLayers) && s1(SOFT) == s1(kLayers)));
    }
};
// backward: layers listed from the output side, N... their widths, KLAST the input width of the last listed one
template <int WAVES, int AGG_AT, int KLAST, int... N>
struct PanelBwdNet {
    static constexpr bool kStatic = true, kByBatch = true;
    static constexpr int kLayers = (int)sizeof...(N), kSoft = 0, kWaves = WAVES, kAggAt = AGG_AT, kKLast = KLAST;
    static constexpr int n(int l) {
        constexpr int w[] = {N...};
        return w[l];
    }
    static constexpr int k(int l) { return l + 1 < kLayers ? n(l + 1) : KLAST; }  // k_in
    static constexpr int nmax() {
        int v = 0;
        for (int l = 0; l < kLayers; ++l) v = cmax(v, n(l));
        return v;
    }
    // the LDS layout of panel_bwd_plan with the LDS tail
    static constexpr int pmax() {
        int v = 0;
        for (int l = 0; l < kLayers; ++l) v = cmax(v, cmax(panel_stride_c(n(l)), panel_stride_c(k(l))));
        return v;
    }
    static constexpr int prm() {
        int v = 0;
        for (int l = 0; l < kLayers; ++l) v += 2 * n(l);
        return v;
    }
    static constexpr int off_e = kPanelRows * pmax(), off_prm = 2 * kPanelRows * pmax(), off_colp = off_prm + prm() + 16;
    static constexpr int off_part = off_colp + WAVES * 2 * nmax(), off_rowmap = off_part + (WAVES - 1) * 512;
    static constexpr bool ok() {
        for (int l = 0; l < kLayers; ++l) {
            const int nt = (k(l) + 31) >> 5, n16 = (n(l) + 15) & ~15, ks = panel_ksplit_c(n(l), nt, WAVES);
            if (nt > WAVES || (ks - 1) * panel_kper_c(n16, ks) >= n16) return false;
            if ((n(l) & 15) || (k(l) & 15)) return false;
        }
        return WAVES >= 8 && WAVES <= kPanelMaxWaves && nmax() <= 128 && (KLAST & 3) == 0;
    }
};

// panel_gemm for a slice plan known at compile time: slice s of KS covers [s * KPER, min((s + 1) * KPER, K16)).  The
// chunk loop is unrolled; a 16-deep group is multiplied under no test where every slice has it, under a wave-uniform
// one where only the last slice is short, and groups past KPER are neither loaded nor multiplied.  Per accumulator the
// MFMAs run in panel_gemm's order.
template <int K16, int KS, int KPER>
__device__ __forceinline__ void panel_gemm_st(f32x4 (&acc)[2], const float* in, int stride,
                                              const float* __restrict__ wfrag, int j, int s, int lane) {
    constexpr int groups = K16 >> 4, last0 = (KS - 1) * KPER;
    static_assert(last0 < K16 && (KPER & 15) == 0, "slice plan");
    const int quad = lane >> 4, l16 = lane & 15;
    const int kbeg = __builtin_amdgcn_readfirstlane(s * KPER);
    const float* arow = in + l16 * stride + 4 * quad + kbeg;
    const int g0 = __builtin_amdgcn_readfirstlane(j * groups + (kbeg >> 4));
    const float* wb = wfrag + (size_t)g0 * 512;
    const unsigned lo = 4u * (unsigned)lane;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[0][r] = acc[1][r] = 0.f;
#pragma unroll
    for (int c = 0; c < (KPER + 63) / 64; ++c) {
        if (last0 + 64 * c < K16 || kbeg + 64 * c < K16) {  // (first test: constant)
            float4 b0[4], b1[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (64 * c + 16 * i < KPER) {
                    b0[i] = *reinterpret_cast<const float4*>(wb + 2048 * c + 512 * i + lo);
                    b1[i] = *reinterpret_cast<const float4*>(wb + 2048 * c + 512 * i + 256 + lo);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (64 * c + 16 * i < KPER && (last0 + 64 * c + 16 * i < K16 || kbeg + 64 * c + 16 * i < K16)) {
                    const float4 a = *reinterpret_cast<const float4*>(arow + 64 * c + 16 * i);
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b0[i].x, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b1[i].x, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b0[i].y, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b1[i].y, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b0[i].z, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b1[i].z, acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b0[i].w, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b1[i].w, acc[1], 0, 0, 0);
                }
            }
        }
    }
}

// the product of layer l of shape SH (forward: K = k(l), tiles over n(l); backward: K = n(l), tiles over k(l)) - one
// instantiation of panel_gemm_st per layer, picked by the unrolled layer index
template <class SH, bool BWD, int L = 0>
__device__ __forceinline__ void panel_gemm_layer(int l, f32x4 (&acc)[2], const float* in, int stride,
                                                 const float* __restrict__ wfrag, int j, int s, int lane) {
    if constexpr (SH::kStatic && L < SH::kLayers) {
        if (l == L) {
            constexpr int K = BWD ? SH::n(L) : SH::k(L), nout = BWD ? SH::k(L) : SH::n(L);
            constexpr int K16 = (K + 15) & ~15, ks = panel_ksplit_c(K, (nout + 31) >> 5, SH::kWaves);
            panel_gemm_st<K16, ks, panel_kper_c(K16, ks)>(acc, in, stride, wfrag, j, s, lane);
        } else {
            panel_gemm_layer<SH, BWD, L + 1>(l, acc, in, stride, wfrag, j, s, lane);
        }
    }
}

// LayerNorm + SiLU row pass of the forward panel kernel: wave w owns rows w, w + nwaves, ...; a row lives
// in registers (NC columns per lane: widths up to 64 * NC), two-pass statistics with VALU wave reductions,
// result written over the LDS panel (next layer's input) and to global.  NC = 2 for the message chain's
// widths (<= 128) is a third of the six-slot form's instructions.
template <int NC>
__device__ __forceinline__ void panel_ln_rows(const PanelLayer& Lr, float* outp, int ys, int n, const float* lgamma,
                                              const float* lbeta, const int* rowmap, int wave, int nwaves, int lane)
{
    constexpr int RPW = 4;  // launcher guarantees >= 4 waves for the 16 rows
    float g[NC], bt[NC];
#pragma unroll
    for (int u = 0; u < NC; ++u) {
        const int c = lane + 64 * u;
        g[u] = c < n ? lgamma[c] : 0.f;
        bt[u] = c < n ? lbeta[c] : 0.f;
    }
    const float inv_n = 1.0f / (float)n;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
        const int lr = wave + i * nwaves;
        if (lr < kPanelRows) {  // wave-uniform
            float* zr = outp + lr * ys;
            const int row = rowmap[lr];
            float v[NC];
            float sm = 0.f;
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                const int c = lane + 64 * u;
                v[u] = c < n ? zr[c] : 0.f;
                sm += v[u];
                if (Lr.z && row >= 0 && c < n) Lr.z[(size_t)row * Lr.ldz + c] = v[u];
            }
            const float mean = wave_sum(sm) * inv_n;
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                const int c = lane + 64 * u;
                v[u] = c < n ? v[u] - mean : 0.f;
            }
            // sum of squares, slot 0 first.  The first two terms are a sum of two products, which may be contracted
            // either way (x * x cannot be -0, so the leading 0 + is gone before that is decided) - and was, differently
            // from one instantiation to the next.  Written out the way every instantiation did before there were
            // static ones: the second square rounded, the first fused onto it, the others fused in order.
            static_assert(NC >= 2, "column slots");
            float q = fmaf(v[0], v[0], mul_rn(v[1], v[1]));
#pragma unroll
            for (int u = 2; u < NC; ++u) q = fmaf(v[u], v[u], q);
            const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_n + 1e-5f);
            float* arow = Lr.a + (size_t)(row < 0 ? 0 : row) * Lr.lda;
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                const int c = lane + 64 * u;
                if (c < n) {
                    const float av = silu_p(v[u] * rstd * g[u] + bt[u]);
                    zr[c] = av;
                    if (row >= 0) arow[c] = av;
                }
            }
            if (Lr.stats && lane == 0 && row >= 0) {
                Lr.stats[(size_t)row * 2] = mean;
                Lr.stats[(size_t)row * 2 + 1] = rstd;
            }
            if (Lr.a3 && row >= 0) {
                // the row's activations are in the LDS panel (written by this wave just above): four
                // consecutive columns per lane -> 8-byte pieces of the three image planes
                for (int c4 = 4 * lane; c4 < n; c4 += 256) {
                    const float4 t = *reinterpret_cast<const float4*>(zr + c4);
                    const int col = Lr.a3_col0 + c4;
                    img_store4(Lr.a3 + img_off((int64_t)Lr.a3_row0 + row, col >> 4, Lr.a3_steps), col, t.x, t.y, t.z, t.w);
                }
            }
        }
    }
}

// Sampling epilogue of the policy workgroups (EPI instantiations): the wave that has just normalised a row of the
// policy hidden layer runs that row's chain of sample.h - output layer, softmax, draw, log p, bounded move, position
// embedding of the next step - on the LDS panel row it wrote.  Per lane these are the columns lane + 64 u it stored
// itself (no barrier needed), in sample_kernel's order: the results are the separate launch's, bit for bit.
// UNI: the row's prefetched values move to scalar registers before the embedding's parameters are requested - the MIX
// instantiation, which has one vector register fewer (a scalar spill lane), needs that to stay out of scratch; the plain
// one fits without it and is 1.5 us per launch faster without (the moves wait for loads the chain would not yet need)
// EXPLORE: sample_finish under exploration controls (sample.h)
// NLA > 0 (the static forms): the launcher has matched the row's width NLA, exactly MAXA actions and the embedding's
// four-columns-a-lane form (sample_pe_fast) - the chain is told so, and the action and column guards of sample.h fold;
// the arithmetic is the same functions'
template <int MAXA, bool UNI, bool EXPLORE = false, int NLA = 0>
__device__ __forceinline__ void panel_sample_rows(const SampleArgs& A0, const float* outp, int ys, const int* rowmap,
                                                  int wave, int nwaves, int lane) {
    for (int lr = __builtin_amdgcn_readfirstlane(wave); lr < kPanelRows; lr += nwaves) {  // wave-uniform: scalar
        const int row = __builtin_amdgcn_readfirstlane(rowmap[lr]);
        if (row < 0) continue;
        // (the lane index is made opaque per row: hoisted out of this loop, the chain's per-lane addresses would
        // stay live across it - some forty registers the kernel's budget of 80 does not have)
        int ln = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));  // (from no live register)
        asm volatile("" : "+v"(ln));
        int zero = 0;  // (likewise the arguments: read where the chain uses them, not all ahead of the loop)
        asm volatile("" : "+s"(zero));
        const SampleArgs& A = (&A0)[zero];
        if (NLA > 0) {  // (matched by the launcher: the action and column guards of sample.h fold)
            __builtin_assume(A.nA == MAXA);
            __builtin_assume(A.nla == NLA);
        }
        float p[MAXA];
        SamplePre<MAXA> S;
        sample_prefetch_row<MAXA>(A, row, ln, S);
        sample_row_logits_at<MAXA, kPanelMaxCols>(A, outp + lr * ys, p, ln);
        // the row's prefetched values are the same in every lane and have arrived (their loads were issued ahead of
        // the logits'): into scalar registers, out of the way of the embedding's 20 vector registers
        if (UNI) {
            auto uni = [](float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); };
#pragma unroll
            for (int j = 0; j < MAXA; ++j) {
                S.b1[j] = uni(S.b1[j]);
                S.nz[j] = uni(S.nz[j]);
            }
            S.ctr = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(S.ctr >> 32)) << 32) |
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)S.ctr);
            S.pi0 = __builtin_amdgcn_readfirstlane(S.pi0);
            S.pi1 = __builtin_amdgcn_readfirstlane(S.pi1);
            S.forced = __builtin_amdgcn_readfirstlane(S.forced);
        }
        sample_prefetch_pe<MAXA, (NLA > 0)>(A, ln, S);  // in flight under the reductions, the softmax and the draw
        sample_finish<MAXA, EXPLORE>(A, row, p, ln, S);
    }
}

// ===========================================================================
// forward
// ===========================================================================
// SAMPLE: 0 = panels only; 4 / MARL_MAX_ACTIONS = the action loops of sample.h bounded at that many actions, for
// the sampling workgroups that ride along behind the panel ones (EPI = false) or for the sampling epilogue of the
// workgroups of problem B.epi_prob - 1 (EPI = true: sample(t) inside the launch that computes policy(t))
// MIX: the agg_at site mixes over a communication graph (P.mix) instead of taking the mean; the plain instantiations
// carry none of it.  GATE (with MIX): the matrix is gated by the agents' positions (P.gate, marl_comm_range): one matrix
// per image of the workgroup, built here from the base matrix P.mix; the constant-MIX instantiations carry none of it
// EXPLORE (with EPI): the epilogue samples under exploration controls (marl_policy_explore); the others carry none of it
// One problem of a forward launch, the body of both kernels below.  SH: the problem's shape (PanelDyn: from P); LY: the
// LDS float offsets of a static launch (PanelFwdLay; the run-time form reads the launcher's from B where it uses them)
struct PanelDynLay {
    static constexpr int panel1 = 0, red = 0, part = 0, prm = 0;
};
template <class SH, class LY, int SAMPLE, bool MIX, bool EPI, bool GATE, bool EXPLORE>
__device__ __forceinline__ void panel_fwd_body(const PanelFwdBatch& B, const PanelFwdProb& P, float* lds) {
    constexpr bool ST = SH::kStatic;
    const int m0 = blockIdx.x * kPanelRows;
    // > 0: this workgroup owns all agents of bpb batch elements (static forms: by-batch rows with AGG_AT, else tiled)
    const int bpb = ST && !SH::kByBatch ? 0 : P.by_batch;
    if ((ST ? SH::kByBatch : bpb != 0) ? (int)blockIdx.x * bpb >= P.g_nb : m0 >= P.m) return;
// threads of the workgroup and layers of the launch (the latter a constant but for the SOFT forms, which also run their
// first SOFT layers alone); the run-time form reads both where it uses them
#define PANEL_NT (ST ? 64u * SH::kWaves : blockDim.x)
#define PANEL_NL (ST && SH::kSoft == 0 ? SH::kLayers : P.nlayers)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = PANEL_NT >> 6;
    // global row of local row lr, or -1 (padding): a small table in LDS
    int* rowmap = reinterpret_cast<int*>(lds + (ST ? LY::red : B.off_red));
    if (tid < kPanelRows) {
        int r = m0 + tid < P.m ? m0 + tid : -1;
        if (ST ? SH::kByBatch : bpb != 0) {
            const int a = tid / bpb, b = (int)blockIdx.x * bpb + (tid - a * bpb);
            r = (a < P.g_na && b < P.g_nb) ? a * P.g_nb + b : -1;
        }
        rowmap[tid] = r;
    }
    lds_barrier();
    const int quad = lane >> 4, l16 = lane & 15;
#ifdef MARL_KERNEL_TS
    MARL_TS_DECL(B.ts);
#endif
    MARL_TS();
    float* X = lds;
    float* Y = lds + (ST ? LY::panel1 : B.off_panel1);
    float* part = lds + (ST ? LY::part : B.off_part);
    float* prm = lds + (ST ? LY::prm : B.off_prm);  // [layer][bias | gamma | beta][n] staged once
    // The per-channel vectors of EVERY layer and the input rows are requested before anything is
    // waited for (one round trip to L2 at the head of the kernel instead of one per layer plus
    // one per staging pass); the LDS stores follow the staging below.  n <= 32 * waves <= threads.
    float pv[kPanelMaxLayers][3];
#pragma unroll
    for (int l = 0; l < kPanelMaxLayers; ++l) {
        pv[l][0] = pv[l][1] = pv[l][2] = 0.f;
        if (ST && l >= SH::kLayers) continue;
        if (l < PANEL_NL && tid < (ST ? SH::n(l) : P.layer[l].n)) {
            pv[l][0] = P.layer[l].bias[tid];
            pv[l][1] = P.layer[l].gamma[tid];
            pv[l][2] = P.layer[l].beta[tid];
        }
    }
    // the mixing coefficients join the same batch of loads (g_na <= 16: one per thread of the first four waves)
    float cmv = 0.f;
    if (MIX && !GATE && P.mix && tid < P.g_na * P.g_na) cmv = P.mix[tid];
    if (MIX && GATE && tid < bpb * P.g_na * P.g_na) {  // (by_batch * g_na^2 <= kPanelRows * g_na <= 256 entries)
        const int na = P.g_na, i = tid / (na * na), e = tid - i * na * na, a = e / na;
        const int b = (int)blockIdx.x * bpb + i;
        if (b < P.g_nb) cmv = comm_gate_weight<kPanelRows>(P.mix, P.gate, na, P.g_nb, b, a, e - a * na);
    }

    // ---- stage the 32-row input panel (zero-filled past k0 and past M)
    {
        const int k0 = ST ? SH::kK0 : P.k0, xs = panel_stride(k0), K16 = (k0 + 15) & ~15;
        const int c4 = K16 >> 2;
        const int K4 = (k0 + 3) & ~3;
        if (!GATE && !ST && P.agg_na > 0) {  // (GATE / static forms: the launcher admits the agg_at site only)
            // message mean over the OTHER agents (networks/message.py:5-17), 4 loads in flight
            const int na = P.agg_na, nb = P.agg_nb;
            const float den = (float)(na - 1);
            for (int e = tid; e < kPanelRows * c4; e += PANEL_NT) {
                const int lr = e / c4, k = (e % c4) * 4;
                const int r = rowmap[lr];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r >= 0 && k < K4 && na > 1) {
                    const int b = r % nb;
                    const float* base = P.x + (size_t)b * P.ldx + k;
                    const size_t astr = (size_t)nb * P.ldx;
                    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                    for (int a0 = 0; a0 < na; a0 += 8) {  // 8 independent loads in flight
                        float4 qv[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int a = a0 + u < na ? a0 + u : na - 1;
                            qv[u] = *reinterpret_cast<const float4*>(base + (size_t)a * astr);
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            if (a0 + u < na) {  // sequential over agents, as the reference's sum(dim=0)
                                s.x += qv[u].x;
                                s.y += qv[u].y;
                                s.z += qv[u].z;
                                s.w += qv[u].w;
                            }
                        }
                    }
                    const float4 me = *reinterpret_cast<const float4*>(P.x + (size_t)r * P.ldx + k);
                    v = make_float4((s.x - me.x) / den, (s.y - me.y) / den, (s.z - me.z) / den,
                                    (s.w - me.w) / den);
                    // pad columns [k0, K4) of the message rows are zero, so v is zero there too
                    if (P.xbar) *reinterpret_cast<float4*>(P.xbar + (size_t)r * P.ldx + k) = v;
                }
                *reinterpret_cast<float4*>(X + lr * xs + k) = v;
            }
        } else {
            float4 xv[2];  // the first two passes' loads fly together
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int e = tid + it * (int)PANEL_NT;
                xv[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < kPanelRows * c4) {
                    const int lr = e / c4, k = (e % c4) * 4;
                    const int r = rowmap[lr];
                    if (r >= 0 && k < K4) xv[it] = *reinterpret_cast<const float4*>(P.x + (size_t)r * P.ldx + k);
                }
            }
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int e = tid + it * (int)PANEL_NT;
                if (e < kPanelRows * c4) {
                    const int lr = e / c4, k = (e % c4) * 4;
                    *reinterpret_cast<float4*>(X + lr * xs + k) = xv[it];
                }
            }
            for (int e = tid + 2 * blockDim.x; e < kPanelRows * c4; e += PANEL_NT) {
                const int lr = e / c4, k = (e % c4) * 4;
                const int r = rowmap[lr];
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r >= 0 && k < K4) v = *reinterpret_cast<const float4*>(P.x + (size_t)r * P.ldx + k);
                *reinterpret_cast<float4*>(X + lr * xs + k) = v;
            }
        }
    }
    {
        int poff = 0;
#pragma unroll
        for (int l = 0; l < kPanelMaxLayers; ++l) {
            if (ST && l >= SH::kLayers) continue;
            if (l < PANEL_NL) {
                const int n = ST ? SH::n(l) : P.layer[l].n;
                if (tid < n) {
                    prm[poff + tid] = pv[l][0];
                    prm[poff + n + tid] = pv[l][1];
                    prm[poff + 2 * n + tid] = pv[l][2];
                }
                poff += 3 * n;
            }
        }
    }
    if (MIX && !GATE && P.mix && tid < P.g_na * P.g_na) lds[B.off_mix + tid] = cmv;
    if (MIX && GATE && tid < bpb * P.g_na * P.g_na) lds[B.off_mix + tid] = cmv;
    MARL_TS();
    lds_barrier();
    MARL_TS();

    int prm_off = 0, K = ST ? SH::kK0 : P.k0;
    constexpr int kUnroll = ST ? SH::kLayers : 1;  // (the run-time form keeps its loop)
#pragma unroll kUnroll
    for (int l = 0; l < (ST ? SH::kLayers : PANEL_NL); ++l) {
        if (ST && SH::kSoft > 0 && l >= SH::kSoft && PANEL_NL <= SH::kSoft) break;  // (scalar: the encoder-only form)
        const PanelLayer Lr = P.layer[l];  // by value: no scalar re-loads inside the loops
        const int n = ST ? SH::n(l) : Lr.n;
        const float* lbias = prm + prm_off;
        const float* lgamma = lbias + n;
        const float* lbeta = lgamma + n;
        prm_off += 3 * n;
        float* in = (l & 1) ? Y : X;
        float* outp = (l & 1) ? X : Y;  // this layer's output panel (next layer's input)
        const int K16 = (K + 15) & ~15;
        const int stride = panel_stride(K);
        if (l > 0 && l == (ST ? SH::kAggAt : P.agg_at)) {
            // the panel holds the messages of every agent of this workgroup's batch elements:
            // message mean over the OTHER agents in place (sequential over agents, as the
            // reference's sum(dim=0)), kept in xbar for the weight gradients
            const int c4 = K16 >> 2, K4 = (K + 3) & ~3, na = P.g_na;
            const float den = (float)(na - 1);
            float4 v[2];
#pragma unroll
            for (int it = 0; it < 2; ++it) {  // launcher: kPanelRows * c4 <= 2 * blockDim.x
                const int e = tid + it * (int)PANEL_NT;
                v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < kPanelRows * c4) {
                    const int lr = e / c4, k = (e - lr * c4) * 4;
                    const int bd = ST && !SH::kByBatch ? 1 : bpb;  // (a tiled static role has no such site)
                    const int a = lr / bd, i = lr - a * bd;
                    if (MIX) {
                        // communication graph: one fmaf chain over the senders, ascending; a sender whose
                        // coefficient is exactly 0 is not read (its NaN / Inf cannot leak through 0 * x)
                        if (a < na) {
                            const float* crow = lds + B.off_mix + (GATE ? i * na + a : a) * na;
                            float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
                            for (int a2 = 0; a2 < na; ++a2) {
                                const float cf = crow[a2];
                                if (cf != 0.f) {
                                    const float4 q = *reinterpret_cast<const float4*>(in + (a2 * bpb + i) * stride + k);
                                    sm.x = fmaf(cf, q.x, sm.x);
                                    sm.y = fmaf(cf, q.y, sm.y);
                                    sm.z = fmaf(cf, q.z, sm.z);
                                    sm.w = fmaf(cf, q.w, sm.w);
                                }
                            }
                            v[it] = sm;
                        }
                    } else if (a < na && na > 1) {
                        float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
                        for (int a2 = 0; a2 < na; ++a2) {
                            const float4 q = *reinterpret_cast<const float4*>(in + (a2 * bpb + i) * stride + k);
                            sm.x += q.x;
                            sm.y += q.y;
                            sm.z += q.z;
                            sm.w += q.w;
                        }
                        const float4 me = *reinterpret_cast<const float4*>(in + lr * stride + k);
                        v[it] = make_float4((sm.x - me.x) / den, (sm.y - me.y) / den, (sm.z - me.z) / den,
                                            (sm.w - me.w) / den);
                    }
                }
            }
            lds_barrier();
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int e = tid + it * (int)PANEL_NT;
                if (e < kPanelRows * c4) {
                    const int lr = e / c4, k = (e - lr * c4) * 4;
                    *reinterpret_cast<float4*>(in + lr * stride + k) = v[it];
                    const int r = rowmap[lr];
                    if (r >= 0 && k < K4 && P.xbar)
                        *reinterpret_cast<float4*>(P.xbar + (size_t)r * P.ld_xbar + k) = v[it];
                }
            }
            lds_barrier();
        }
        const int nt = (n + 31) >> 5;
        const int ks = panel_ksplit(K, nt, nwaves);
        const int j = wave % nt, s = wave / nt;
        const bool active = s < ks;
        f32x4 acc[2];
        if constexpr (ST) {
            if (active) panel_gemm_layer<SH, false>(l, acc, in, stride, Lr.wfrag, j, s, lane);
        } else {
            const int kper = (((K16 + ks - 1) / ks) + 15) & ~15;
            const int kbeg = s * kper;
            const int kend = kbeg + kper < K16 ? kbeg + kper : K16;
            if (active) panel_gemm(acc, in, stride, Lr.wfrag, Lr.wgroups, j, kbeg, kend, lane);
        }
        MARL_TS();
        panel_ksum(acc, part, nt, ks, j, s, lane, active);
        MARL_TS();

        // z = acc + bias -> output panel in LDS (its copy kept for backward is written row-wise,
        // coalesced, by the LayerNorm pass below instead of as 64-byte pieces from this layout)
        const int ys = panel_stride(n), n16 = (n + 15) & ~15;
        if (active && s == 0) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int col = j * 32 + 16 * t + l16;
                const bool cv = (ST && (n & 31) == 0) || col < n;  // (static widths: whole tiles)
                const float bv = cv ? lbias[col] : 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int lr = 4 * quad + r;
                    const float zv = cv ? acc[t][r] + bv : 0.f;
                    if ((ST && (n & 31) == 0) || col < n16) outp[lr * ys + col] = zv;
                }
            }
        }
        MARL_TS();
        lds_barrier();
        MARL_TS();
        // LayerNorm + SiLU row pass (panel_ln_rows above), unrolled for this layer's width
        if (n <= (ST ? 128 : B.ln_narrow_max))
            panel_ln_rows<2>(Lr, outp, ys, n, lgamma, lbeta, rowmap, wave, nwaves, lane);
        else
            panel_ln_rows<kPanelMaxCols>(Lr, outp, ys, n, lgamma, lbeta, rowmap, wave, nwaves, lane);
        MARL_TS();
        lds_barrier();
        MARL_TS();
        K = n;
    }
    // (outside the layer loop: none of the loop's layer descriptors stays live across the chain)
    if (EPI && (ST || (int)blockIdx.y + 1 == B.epi_prob)) {
        constexpr int MAXA = SAMPLE > 0 ? SAMPLE : 4;
        // (the plain EXPLORE instantiation takes the UNI form too: without it, it holds two registers too many)
        panel_sample_rows<MAXA, MIX || EXPLORE || ST, EXPLORE, ST ? SH::n(ST ? SH::kLayers - 1 : 0) : 0>(
            B.sample, (PANEL_NL & 1) ? Y : X, panel_stride(K), rowmap, wave, nwaves, lane);
        MARL_TS();
    }
}

#undef PANEL_NT
#undef PANEL_NL

template <int SAMPLE, bool MIX = false, bool EPI = false, bool GATE = false, bool EXPLORE = false>
__global__ __launch_bounds__(768, 6) 
void panel_fwd_kernel(const PanelFwdBatch B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (!EPI && SAMPLE > 0 && (int)blockIdx.x >= B.panel_blocks) {
        // ride-along sampling workgroup: one wave per row of the policy activations
        const int r = ((int)blockIdx.x - B.panel_blocks) * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
        if (r >= B.sample.R) return;
        constexpr int MAXA = SAMPLE > 0 ? SAMPLE : 4;
        float p[MAXA];
        SamplePre<MAXA> S;
        sample_prefetch<MAXA, false>(B.sample, r, threadIdx.x & 63, S);
        sample_row_logits<MAXA>(B.sample, r, p, threadIdx.x & 63);
        sample_finish<MAXA>(B.sample, r, p, threadIdx.x & 63, S);
        return;
    }
    panel_fwd_body<PanelDyn, PanelDynLay, SAMPLE, MIX, EPI, GATE, EXPLORE>(B, B.p[blockIdx.y], lds);
}

// The static forms of the chain launch: problem 0 = the message chain CH (by-batch rows; SOFT: also its encoder-only
// form), problem 1 = the policy hidden layer PO (row-tiled), with the four-action sampling epilogue (EPI) or without.
// Plain launches only: no mixing matrix, no gate, no exploration controls, no staged mean, no ride-along rows.
template <class CH, class PO>
struct PanelFwdLay {
    static_assert(CH::ok() && PO::ok() && CH::kWaves == PO::kWaves && CH::kByBatch && !PO::kByBatch, "static panel nets");
    static constexpr int waves = CH::kWaves;
    static constexpr int panel1 = cmax(CH::s0(CH::kLayers), PO::s0(PO::kLayers));
    static constexpr int red = panel1 + cmax(CH::s1(CH::kLayers), PO::s1(PO::kLayers));
    static constexpr int part = red + (kPanelMaxWaves + 1) * 32, prm = part + (waves - 1) * 512;
};
template <class CH, class PO, bool EPI>
__global__ __launch_bounds__(768, 6) void panel_fwd_static_kernel(const PanelFwdBatch B) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    using LY = PanelFwdLay<CH, PO>;
    if (blockIdx.y == 0)
        panel_fwd_body<CH, LY, 0, false, false, false, false>(B, B.p[0], lds);
    else
        panel_fwd_body<PO, LY, EPI ? 4 : 0, false, EPI, false, false>(B, B.p[1], lds);
}

constexpr size_t kPanelMaxLds = 144 * 1024;

static int panel_waves_for(int k, int n) {
    const int nt = (n + 31) / 32;
    const int want = (((k + 15) & ~15) + 63) / 64;
    int w = nt * want;
    if (w < nt) w = nt;
    return w > kPanelMaxWaves ? (nt > kPanelMaxWaves ? -1 : (kPanelMaxWaves / nt) * nt) : w;
}

int panel_chain_supported(int na, int n_msg, int threads) {
    const int K16 = (n_msg + 15) & ~15;  // (two passes of the workgroup cover the message panel)
    return na >= 1 && na <= kPanelRows && kPanelRows * (K16 / 4) <= 2 * threads;
}

// the sampling epilogue is instantiated for the four-action bound only (a sixteen-action one is 4x the chain's code
// and registers inside the 80-register kernel): larger action sets keep the separate sample_kernel launch
int panel_sample_supported(int n_actions) { return n_actions >= 1 && n_actions <= 4; }

int panel_supported(int k0, int n0, int n1) {
    if (n0 > 32 * kPanelMaxWaves || n1 > 32 * kPanelMaxWaves) return 0;  // one column tile per wave
    if (n0 > 64 * kPanelMaxCols || n1 > 64 * kPanelMaxCols) return 0;
    const int kx = k0 > n1 ? k0 : n1;
    const size_t lds = (size_t)(kPanelRows * panel_stride(kx) + kPanelRows * panel_stride(n0) +
                                (kPanelMaxWaves + 1) * 32 + (kPanelMaxWaves - 1) * 512 +
                                3 * (n0 + n1) + 16) * 4;
    return lds <= kPanelMaxLds;
}

// slice length of a K split (what both kernels compute from panel_ksplit's ks); slice s is empty when s * kper >= K16
static int panel_kper_host(int K16, int ks) { return (((K16 + ks - 1) / ks) + 15) & ~15; }

// What launch_panel_fwd decides before it launches: the checks, the LDS layout (written into b), the wave count and the
// grid.  Host arithmetic only: marl_panel_plan (marl_hip_panelops.h) reports it from this same routine.
struct PanelFwdPlan {
    int waves;
    size_t lds;
    unsigned pblocks;
    bool mixed, gated;
};
static int panel_fwd_plan(PanelFwdBatch& b, PanelFwdPlan& pl) {
    int waves = 1, x0 = 0, x1 = 0;
    for (int i = 0; i < b.count; ++i) {
        const PanelFwdProb& p = b.p[i];
        for (int l = 0; l < p.nlayers; ++l) {
            const int kin = l == 0 ? p.k0 : p.layer[l - 1].n;
            if (!p.layer[l].wfrag) {
                set_error("panel kernel: layer %d has no fragment-order weight copy", l);
                return MARL_EINVAL;
            }
            if (p.layer[l].wgroups != panel_frag_groups(kin)) {
                set_error("panel kernel: layer %d's weight copy has %d K groups, its input width %d needs %d", l,
                          p.layer[l].wgroups, kin, panel_frag_groups(kin));
                return MARL_ELIMIT;
            }
            const int w = panel_waves_for(kin, p.layer[l].n);
            if (w < 0) {
                set_error("panel kernel: layer width %d too large", p.layer[l].n);
                return MARL_ELIMIT;
            }
            waves = w > waves ? w : waves;
        }
        // X: the input and the outputs of the odd layers; Y: the outputs of the even layers
        int s0 = kPanelRows * panel_stride(p.k0), s1 = 0;
        for (int l = 0; l < p.nlayers; ++l) {
            const int v = kPanelRows * panel_stride(p.layer[l].n);
            if (l & 1)
                s0 = v > s0 ? v : s0;
            else
                s1 = v > s1 ? v : s1;
        }
        if (p.agg_at > 0 && (p.by_batch < 1 || p.g_na * p.by_batch > kPanelRows || p.agg_at >= p.nlayers ||
                             !panel_chain_supported(p.g_na, p.layer[p.agg_at - 1].n, 256))) {
            set_error("panel kernel: in-panel message mean outside its range");
            return MARL_ELIMIT;
        }
        if (p.mix && (p.agg_at <= 0 || i != 0 || (b.has_sample && b.count == 1))) {
            set_error("panel kernel: a mixing matrix needs the in-panel aggregation of problem 0");
            return MARL_ELIMIT;
        }
        // (the gated instantiations carry no staged mean, in any problem of the launch)
        if ((p.gate.pos && (!p.mix || p.by_batch * p.g_na * p.g_na > kPanelRows * kPanelRows)) ||
            (b.p[0].gate.pos && p.agg_na > 0)) {
            set_error("panel kernel: a position gate needs a base matrix, no staged mean and by_batch * agents^2 <= %d",
                      kPanelRows * kPanelRows);
            return MARL_ELIMIT;
        }
        x0 = s0 > x0 ? s0 : x0;
        x1 = s1 > x1 ? s1 : x1;
    }
    const bool mixed = b.count > 0 && b.p[0].mix != nullptr;
    const bool gated = mixed && b.p[0].gate.pos != nullptr;
    if (waves < 4) waves = 4;  // the LayerNorm row loop covers <= 4 rows per wave
    b.off_panel1 = x0;
    b.off_red = x0 + x1;
    b.off_part = b.off_red + (kPanelMaxWaves + 1) * 32;
    b.off_prm = b.off_part + (waves - 1) * 512;
    int prm = 0;
    for (int i = 0; i < b.count; ++i) {
        int q = 0;
        for (int l = 0; l < b.p[i].nlayers; ++l) q += 3 * b.p[i].layer[l].n;
        prm = q > prm ? q : prm;
    }
    // (+ the mixing matrix, g_na^2 <= kPanelRows^2 floats.  Every plan use_chain admits has widths <= 384: two panels
    // of 16 x 388, 11 x 512 partials and 12 x 384 parameters are under 100 KiB, so the matrix always fits; the check
    // below stays as the backstop)
    b.off_mix = b.off_prm + prm + 16;
    const size_t lds = (size_t)(b.off_mix + (mixed ? kPanelRows * kPanelRows : 0)) * sizeof(float);
    if (lds > kPanelMaxLds) {
        set_error("panel kernel: shape outside its range");
        return MARL_ELIMIT;
    }
    b.ln_narrow_max = 128;  // widths that take the two-slot row pass
    unsigned pblocks = 0;
    for (int i = 0; i < b.count; ++i) {
        const PanelFwdProb& p = b.p[i];
        const unsigned nblk = p.by_batch > 0 ? (unsigned)cdiv(p.g_nb, p.by_batch) : (unsigned)cdiv(p.m, kPanelRows);
        pblocks = nblk > pblocks ? nblk : pblocks;
    }
    pl.waves = waves;
    pl.lds = lds;
    pl.pblocks = pblocks;
    pl.mixed = mixed;
    pl.gated = gated;
    return MARL_OK;
}

// ---------------------------------------------------------------------------
// The static forms (README dimensions: BASELINE C3 / C5, and C4's message chain).  MARL_PANEL_STATIC=0 keeps every
// launch on the run-time form (same-binary comparison; read once per process).
// ---------------------------------------------------------------------------
using PanelChainNet = PanelNet<12, 256, 2, 2, 128, 64, 128, 96>;  // encoder 256 -> 128 -> 64 | mean | decoder -> 128 -> 96
using PanelPolicyNet = PanelNet<12, 256, 0, 0, 384>;              // policy hidden layer 256 -> 384
using PanelFwdStaticLay = PanelFwdLay<PanelChainNet, PanelPolicyNet>;
using PanelBwdChainNet = PanelBwdNet<8, 2, 256, 96, 128, 64, 128>;  // decoder(t) | mean | encoder(t-1) -> dh
using PanelBwdDecNet = PanelBwdNet<8, 0, 64, 96, 128>;              // step 0: the decoder alone
static_assert(PanelBwdChainNet::ok() && PanelBwdDecNet::ok(), "static panel nets");
constexpr int kPanelStaticActions = 4;

static bool panel_static_env() {
    static const bool on = [] {
        const char* v = getenv("MARL_PANEL_STATIC");
        return !(v && v[0] == '0');
    }();
    return on;
}

int panel_static_model(int n_b, int n_a, int nm2, int n_m, int n_mo, int nla, int n_actions, int n_d) {
    using C = PanelChainNet;
    return panel_static_env() && n_b == C::kK0 && nm2 == C::n(0) && n_m == C::n(1) && nm2 == C::n(2) && n_mo == C::n(3) &&
           n_a == PanelPolicyNet::kK0 && nla == PanelPolicyNet::n(0) && n_actions == kPanelStaticActions &&
           (n_d & 3) == 0 && n_d <= 256;  // (the embedding's four-columns-a-lane form, as the launcher asks of the epilogue)
}

template <class SH>
static bool panel_fwd_matches(const PanelFwdProb& p, int layers) {
    if (p.nlayers != layers || p.k0 != SH::kK0 || p.agg_na != 0 || p.mix || p.gate.pos) return false;
    if (SH::kByBatch ? p.by_batch < 1 : p.by_batch != 0) return false;
    if (p.agg_at != (layers > SH::kAggAt ? SH::kAggAt : 0)) return false;
    for (int l = 0; l < layers; ++l)
        if (p.layer[l].n != SH::n(l) || p.layer[l].wgroups != panel_frag_groups(SH::k(l))) return false;
    return true;
}
// host twin of sample_pe_fast (sample.h): the static epilogue takes the four-columns-a-lane embedding for granted
static bool panel_pe_fast_host(const SampleArgs& A) {
    const uintptr_t al = (uintptr_t)A.pe_W | (uintptr_t)A.pe_b | (uintptr_t)A.pe_gamma | (uintptr_t)A.pe_beta |
                         (uintptr_t)A.pe_z | (uintptr_t)A.pe_out;
    return A.pe_W && A.step_logp && (al & 15) == 0 && A.pe_nd <= 256 && ((A.pe_nd | A.pe_ldz | A.pe_ldo) & 3) == 0 &&
           (A.pe_col0 & 3) == 0;
}
// the launch is the plain chain launch of the static nets, planned as their layout has it
static bool panel_fwd_static_ok(const PanelFwdBatch& b, const PanelFwdPlan& pl, bool explore) {
    using LY = PanelFwdStaticLay;
    if (!panel_static_env() || explore || pl.mixed || pl.gated || b.count != 2 || b.has_sample) return false;
    if (!panel_fwd_matches<PanelChainNet>(b.p[0], PanelChainNet::kLayers) &&
        !panel_fwd_matches<PanelChainNet>(b.p[0], PanelChainNet::kSoft))
        return false;
    if (!panel_fwd_matches<PanelPolicyNet>(b.p[1], 1)) return false;
    if (pl.waves != LY::waves || b.off_panel1 != LY::panel1 || b.off_red != LY::red || b.off_part != LY::part ||
        b.off_prm != LY::prm || b.ln_narrow_max != 128)
        return false;
    if (b.epi_prob) {
        const SampleArgs& A = b.sample;
        if (b.epi_prob != 2 || A.nA != kPanelStaticActions || A.nla != PanelPolicyNet::n(0)) return false;
        if (A.pe_W && !panel_pe_fast_host(A)) return false;
    }
    return true;
}

int launch_panel_fwd(PanelFwdBatch& b, hipStream_t st, bool explore) {
    PanelFwdPlan pl;
    MARL_TRY(panel_fwd_plan(b, pl));
    const int waves = pl.waves;
    const size_t lds = pl.lds;
    const unsigned pblocks = pl.pblocks;
    const bool mixed = pl.mixed, gated = pl.gated;
    static bool raised = false;
    if (!raised) {
        const void* kerns[13] = {reinterpret_cast<const void*>(panel_fwd_static_kernel<PanelChainNet, PanelPolicyNet, false>),
                                reinterpret_cast<const void*>(panel_fwd_static_kernel<PanelChainNet, PanelPolicyNet, true>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<0>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<4>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<MARL_MAX_ACTIONS>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<0, true>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<4, false, true>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<4, true, true>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<0, true, false, true>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<4, true, true, true>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<4, false, true, false, true>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<4, true, true, false, true>),
                                reinterpret_cast<const void*>(panel_fwd_kernel<4, true, true, true, true>)};
        for (const void* kf : kerns)
            MARL_HIP_CHECK(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPanelMaxLds));
        raised = true;
    }
#ifdef MARL_KERNEL_TS
    static long long* d_ts = nullptr;
    static int calls = 0;
    const int rec = ts_begin(&d_ts, calls++);
    b.ts = rec ? d_ts : nullptr;
#endif
    if (b.epi_prob) {
        const PanelFwdProb* p = b.epi_prob >= 1 && b.epi_prob <= b.count ? &b.p[b.epi_prob - 1] : nullptr;
        if (!p || !panel_sample_supported(b.sample.nA) || p->nlayers < 1 || p->m != b.sample.R ||
            p->layer[p->nlayers - 1].a != b.sample.a_pol || p->layer[p->nlayers - 1].n != b.sample.nla) {
            set_error("panel kernel: the sampling epilogue needs the problem whose last layer writes its activations");
            return MARL_EINVAL;
        }
    }
    if (explore && !b.epi_prob) {
        set_error("panel kernel: exploration controls are served by the sampling epilogue only");
        return MARL_EINVAL;
    }
    // A single agent has no other agents: the staged mean is zero (networks/message.py:5-17) and the kernel stages
    // zeros without storing them.  xbar is an output all the same - the decoder's weight gradient reads it - so its
    // rows (the float4-rounded columns the kernel would have stored) are zeroed here instead of being left as found.
    for (int i = 0; i < b.count; ++i) {
        const PanelFwdProb& p = b.p[i];
        if (p.agg_na == 1 && p.xbar) {
            PermBatch z{};
            z.count = 1;
            z.d[0].dst = p.xbar, z.d[0].rows = p.m, z.d[0].cols = (p.k0 + 3) & ~3, z.d[0].dst_ld = p.ldx;
            z.d[0].rd = z.d[0].cd = 1;
            MARL_TRY(launch_permute(z, st));
        }
    }
    prof_before(4, st);
    if (panel_fwd_static_ok(b, pl, explore)) {
        b.has_sample = 0;
        if (b.epi_prob)
            hipLaunchKernelGGL((panel_fwd_static_kernel<PanelChainNet, PanelPolicyNet, true>),
                               dim3(pblocks, (unsigned)b.count), dim3(64 * waves), lds, st, b);
        else
            hipLaunchKernelGGL((panel_fwd_static_kernel<PanelChainNet, PanelPolicyNet, false>),
                               dim3(pblocks, (unsigned)b.count), dim3(64 * waves), lds, st, b);
    } else if (b.epi_prob && explore) {  // the same three forms, sampling from the behaviour policy
        b.has_sample = 0;
        if (gated)
            hipLaunchKernelGGL((panel_fwd_kernel<4, true, true, true, true>), dim3(pblocks, (unsigned)b.count),
                               dim3(64 * waves), lds, st, b);
        else if (mixed)
            hipLaunchKernelGGL((panel_fwd_kernel<4, true, true, false, true>), dim3(pblocks, (unsigned)b.count),
                               dim3(64 * waves), lds, st, b);
        else
            hipLaunchKernelGGL((panel_fwd_kernel<4, false, true, false, true>), dim3(pblocks, (unsigned)b.count),
                               dim3(64 * waves), lds, st, b);
    } else if (b.epi_prob) {
        // sample(t) as the epilogue of the policy workgroups: no ride-along workgroups
        b.has_sample = 0;
        if (gated)
            hipLaunchKernelGGL((panel_fwd_kernel<4, true, true, true>), dim3(pblocks, (unsigned)b.count),
                               dim3(64 * waves), lds, st, b);
        else if (mixed)
            hipLaunchKernelGGL((panel_fwd_kernel<4, true, true>), dim3(pblocks, (unsigned)b.count), dim3(64 * waves),
                               lds, st, b);
        else
            hipLaunchKernelGGL((panel_fwd_kernel<4, false, true>), dim3(pblocks, (unsigned)b.count), dim3(64 * waves),
                               lds, st, b);
    } else if (b.has_sample && b.count == 1) {
        b.panel_blocks = (int)pblocks;
        const unsigned sblocks = (unsigned)cdiv(b.sample.R, waves);
        if (b.sample.nA <= 4)
            hipLaunchKernelGGL(panel_fwd_kernel<4>, dim3(pblocks + sblocks, 1), dim3(64 * waves), lds, st, b);
        else
            hipLaunchKernelGGL(panel_fwd_kernel<MARL_MAX_ACTIONS>, dim3(pblocks + sblocks, 1), dim3(64 * waves), lds, st, b);
    } else {
        b.has_sample = 0;
        if (gated)
            hipLaunchKernelGGL((panel_fwd_kernel<0, true, false, true>), dim3(pblocks, (unsigned)b.count),
                               dim3(64 * waves), lds, st, b);
        else if (mixed)
            hipLaunchKernelGGL((panel_fwd_kernel<0, true>), dim3(pblocks, (unsigned)b.count), dim3(64 * waves),
                               lds, st, b);
        else
            hipLaunchKernelGGL(panel_fwd_kernel<0>, dim3(pblocks, (unsigned)b.count), dim3(64 * waves), lds, st, b);
    }
    prof_after(4, st);
    MARL_LAUNCH_CHECK();
#ifdef MARL_KERNEL_TS
    if (rec) {
        fprintf(stderr, "[ts] panel_fwd count %d sample %d epilogue %d waves %d lds %zu\n", b.count, b.has_sample,
                b.epi_prob, waves, lds);
        ts_report("panel_fwd", d_ts, waves);
        // the second role of a two-problem launch (the policy layer beside the chain; its last phase is the sampling
        // epilogue when there is one): start / end on role 0's clock show the slack before and after
        if (b.count == 2) ts_report("panel_fwd role 1", d_ts, waves, 1);
    }
#endif
    return MARL_OK;
}

// ===========================================================================
// backward: d(SiLU out) -> [LayerNorm/SiLU backward on the LDS panel -> dz (kept) ->
//           dX = dz * W on the matrix cores] per layer, last layer first
// ===========================================================================
constexpr int kBwdMaxCols = kPanelMaxCols;  // columns per lane in the row pass: widths up to 384

// MAXC: LayerNorm columns per lane the row pass is unrolled for (widths up to 64 * MAXC).  The chained
// encoder / decoder backward of the README dimensions has widths <= 128: two column slots instead of six
// are a third of the row pass's instructions and 24 fewer registers.
// MIX: the agg_at site applies the transpose of a communication graph's mixing matrix (P.mix) instead of the mean
// GATE (with MIX): one matrix per image of the workgroup, gated by the positions of the forward's emission step (P.gate)
// and built by the forward's arithmetic (comm_gate_weight), stored transposed
// SH: PanelDyn (every shape, from P) or a PanelBwdNet (by-batch rows, no staged mean, the LDS tail, the layout of
// the net; launch_panel_bwd matches the descriptors before it picks one)
template <class SH, bool CELL, int MAXC, bool MIX = false, bool GATE = false>
__global__ __launch_bounds__(768, 4) void panel_bwd_kernel(const PanelBwdProb P) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr bool ST = SH::kStatic;
    const int nthreads = ST ? 64 * SH::kWaves : (int)blockDim.x;
    if (CELL && (int)blockIdx.x >= P.panel_blocks) {
        const int64_t idx = (int64_t)((int)blockIdx.x - P.panel_blocks) * nthreads + threadIdx.x;
        if (P.cell_vec4)
            lstm_cell_bwd_elem4(P.cell, P.cell_rows, idx);
        else
            lstm_cell_bwd_elem(P.cell, P.cell_rows, idx);
        return;
    }
    const int m0 = blockIdx.x * kPanelRows;
    const int bpb = P.by_batch;  // > 0: this workgroup owns all agents of bpb batch elements
    if ((ST || bpb) ? (int)blockIdx.x * bpb >= P.g_nb : m0 >= P.m) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
    const int quad = lane >> 4, l16 = lane & 15;
    const int nlayers = ST ? SH::kLayers : P.nlayers;
    float* D = lds;            // current gradient panel
    float* E = lds + (ST ? SH::off_e : P.off_e);  // next one
    float* prm = lds + (ST ? SH::off_prm : P.off_prm);
    float* colp = lds + (ST ? SH::off_colp : P.off_colp);  // [nwaves][2][n]
    float* part = lds + (ST ? SH::off_part : P.off_part);
    // global row of local row lr, or -1 (padding): a small table in LDS
    int* rowmap = reinterpret_cast<int*>(lds + (ST ? SH::off_rowmap : P.off_rowmap));
    if (tid < kPanelRows) {
        int r = m0 + tid < P.m ? m0 + tid : -1;
        if (ST || bpb) {
            const int a = tid / bpb, b = (int)blockIdx.x * bpb + (tid - a * bpb);
            r = (a < P.g_na && b < P.g_nb) ? a * P.g_nb + b : -1;
        }
        rowmap[tid] = r;
    }
    lds_barrier();
#ifdef MARL_KERNEL_TS
    MARL_TS_DECL(P.ts);
#endif
    MARL_TS();

    // The saved pre-LayerNorm rows (and statistics) of a layer are requested one layer ahead: the
    // two rows of this wave for layer l + 1 fly while layer l's dX product runs.  Unconditional
    // loads (padding rows read row 0) so that no wait is widened by a branch.
    float zpre[2][MAXC], mpre[2], rpre[2];
    auto zfetch = [&](const PanelBwdLayer& L, const int ln) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int lr = wave + i * nwaves;
            const int row = lr < kPanelRows ? rowmap[lr] : -1;
            const size_t rr = row < 0 ? 0 : (size_t)row;
            mpre[i] = L.stats[rr * 2];
            rpre[i] = L.stats[rr * 2 + 1];
#pragma unroll
            for (int u = 0; u < MAXC; ++u) {
                const int c = lane + 64 * u;
                zpre[i][u] = c < ln ? L.z[rr * L.ldz + c] : 0.f;
            }
        }
    };
    zfetch(P.layer[0], ST ? SH::n(0) : P.layer[0].n);  // first: in flight behind the parameter and gradient-panel loads below
    // LayerNorm affine parameters of every layer -> LDS; d(a_last) panel -> D
    {
        // (all layers' vectors requested before anything is waited for; n <= 384 <= threads)
        float pv[kPanelMaxLayers][2];
#pragma unroll
        for (int l = 0; l < kPanelMaxLayers; ++l) {
            pv[l][0] = pv[l][1] = 0.f;
            if (ST && l >= SH::kLayers) continue;
            if (l < nlayers && tid < (ST ? SH::n(l) : P.layer[l].n)) {
                pv[l][0] = P.layer[l].gamma[tid];
                pv[l][1] = P.layer[l].beta[tid];
            }
        }
        float cmv = 0.f;  // M^T, oriented while it is loaded (row = the sender whose gradient is formed): requested
        if (MIX && !GATE && tid < P.g_na * P.g_na) {  // with the vectors above, stored behind them - one batch of loads
            const int a = tid / P.g_na, a2 = tid - a * P.g_na;
            cmv = P.mix[a2 * P.g_na + a];
        }
        if (MIX && GATE && tid < bpb * P.g_na * P.g_na) {  // entry (i, a, a2) of the LDS copy = w_i[a2, a]
            const int na = P.g_na, i = tid / (na * na), e = tid - i * na * na, a = e / na;
            const int b = (int)blockIdx.x * bpb + i;
            if (b < P.g_nb) cmv = comm_gate_weight<kPanelRows>(P.mix, P.gate, na, P.g_nb, b, e - a * na, a);
        }
        int off = 0;
#pragma unroll
        for (int l = 0; l < kPanelMaxLayers; ++l) {
            if (ST && l >= SH::kLayers) continue;
            if (l < nlayers) {
                const int n = ST ? SH::n(l) : P.layer[l].n;
                if (tid < n) {
                    prm[off + tid] = pv[l][0];
                    prm[off + n + tid] = pv[l][1];
                }
                off += 2 * n;
            }
        }
        if (MIX && !GATE && tid < P.g_na * P.g_na) lds[P.off_mix + tid] = cmv;
        if (MIX && GATE && tid < bpb * P.g_na * P.g_na) lds[P.off_mix + tid] = cmv;
        const int n = ST ? SH::n(0) : P.layer[0].n, ds = panel_stride(n), n16 = (n + 15) & ~15, c4 = n16 >> 2;
        const int n4 = (n + 3) & ~3;
        const int agg_na = ST ? 0 : P.agg_na;  // (static forms: no staged mean)
        for (int e = tid; e < kPanelRows * c4; e += nthreads) {
            const int lr = e / c4, k = (e % c4) * 4;
            const int r = rowmap[lr];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r >= 0 && k < n4 && agg_na > 1) {
                const int na = P.agg_na, nb = P.agg_nb;
                const float den = (float)(na - 1);
                const float* base = P.da + (size_t)(r % nb) * P.ldda + k;
                const size_t astr = (size_t)nb * P.ldda;
                float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
                for (int a0 = 0; a0 < na; a0 += 8) {  // 8 independent loads in flight
                    float4 qv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int a = a0 + u < na ? a0 + u : na - 1;
                        qv[u] = *reinterpret_cast<const float4*>(base + (size_t)a * astr);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        if (a0 + u < na) {  // sequential over agents, as in the forward mean
                            s.x += qv[u].x;
                            s.y += qv[u].y;
                            s.z += qv[u].z;
                            s.w += qv[u].w;
                        }
                    }
                }
                const float4 me = *reinterpret_cast<const float4*>(P.da + (size_t)r * P.ldda + k);
                v = make_float4((s.x - me.x) / den, (s.y - me.y) / den, (s.z - me.z) / den,
                                (s.w - me.w) / den);
            } else if (r >= 0 && k < n4 && agg_na == 0) {
                v = *reinterpret_cast<const float4*>(P.da + (size_t)r * P.ldda + k);
                if (P.da2) {
                    const float4 w = *reinterpret_cast<const float4*>(P.da2 + (size_t)r * P.ldda2 + k);
                    v = make_float4(v.x + w.x, v.y + w.y, v.z + w.z, v.w + w.w);
                }
            }
            *reinterpret_cast<float4*>(D + lr * ds + k) = v;
        }
    }
    MARL_TS();
    lds_barrier();
    MARL_TS();

    int prm_off = 0;
    constexpr int kUnroll = ST ? SH::kLayers : 1;  // (the run-time form keeps its loop)
#pragma unroll kUnroll
    for (int l = 0; l < nlayers; ++l) {
        const PanelBwdLayer Lr = P.layer[l];  // by value: no scalar re-loads inside the loops
        const int n = ST ? SH::n(l) : Lr.n, ds = panel_stride(n), n16 = (n + 15) & ~15;
        const float* lgamma = prm + prm_off;
        const float* lbeta = lgamma + n;
        prm_off += 2 * n;
        if (l > 0 && l == (ST ? SH::kAggAt : P.agg_at)) {
            // D holds the gradient of the message MEAN for every agent of this workgroup's batch
            // elements: the mean over the other agents is self-adjoint - the same sum (sequential
            // over agents, as the staging version) gives the gradient of the messages
            const int c4 = n16 >> 2, na = P.g_na;
            const float den = (float)(na - 1);
            float4 v[2];
#pragma unroll
            for (int it = 0; it < 2; ++it) {  // launcher: kPanelRows * c4 <= 2 * blockDim.x
                const int e = tid + it * nthreads;
                v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (e < kPanelRows * c4) {
                    const int lr = e / c4, k = (e - lr * c4) * 4;
                    const int a = lr / bpb, i = lr - a * bpb;
                    if (MIX) {
                        // the mixing matrix is not self-adjoint: dm[a] = sum_a2 M[a2, a] * dmbar[a2] (the LDS copy
                        // is M^T), one fmaf chain over a2 ascending, zero entries skipped
                        if (a < na) {
                            const float* crow = lds + P.off_mix + (GATE ? i * na + a : a) * na;
                            float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
                            for (int a2 = 0; a2 < na; ++a2) {
                                const float cf = crow[a2];
                                if (cf != 0.f) {
                                    const float4 q = *reinterpret_cast<const float4*>(D + (a2 * bpb + i) * ds + k);
                                    sm.x = fmaf(cf, q.x, sm.x);
                                    sm.y = fmaf(cf, q.y, sm.y);
                                    sm.z = fmaf(cf, q.z, sm.z);
                                    sm.w = fmaf(cf, q.w, sm.w);
                                }
                            }
                            v[it] = sm;
                        }
                    } else if (a < na && na > 1) {
                        float4 sm = make_float4(0.f, 0.f, 0.f, 0.f);
                        for (int a2 = 0; a2 < na; ++a2) {
                            const float4 q = *reinterpret_cast<const float4*>(D + (a2 * bpb + i) * ds + k);
                            sm.x += q.x;
                            sm.y += q.y;
                            sm.z += q.z;
                            sm.w += q.w;
                        }
                        const float4 me = *reinterpret_cast<const float4*>(D + lr * ds + k);
                        v[it] = make_float4((sm.x - me.x) / den, (sm.y - me.y) / den, (sm.z - me.z) / den,
                                            (sm.w - me.w) / den);
                    }
                }
            }
            lds_barrier();
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int e = tid + it * nthreads;
                if (e < kPanelRows * c4) {
                    const int lr = e / c4, k = (e - lr * c4) * 4;
                    *reinterpret_cast<float4*>(D + lr * ds + k) = v[it];
                }
            }
            lds_barrier();
        }
        // ---- row pass: D holds d(SiLU out); D <- dz, dgamma/dbeta column partials.  A row
        // lives in registers between the statistics and the dz pass.
        {
            constexpr int RPW = 2;  // launcher guarantees >= 8 waves for the 16 rows
            float pg[MAXC], pb[MAXC], g[MAXC], bt[MAXC];
#pragma unroll
            for (int u = 0; u < MAXC; ++u) {
                const int c = lane + 64 * u;
                pg[u] = pb[u] = 0.f;
                g[u] = c < n ? lgamma[c] : 0.f;
                bt[u] = c < n ? lbeta[c] : 0.f;
            }
            const float inv_n = 1.0f / (float)n;
#pragma unroll
            for (int i = 0; i < RPW; ++i) {
                const int lr = wave + i * nwaves;
                if (lr < kPanelRows) {  // wave-uniform
                    const int row = rowmap[lr];
                    const bool rv = row >= 0;
                    float xh[MAXC], dxh[MAXC];
                    float s1 = 0.f, s2 = 0.f, rstd = 0.f;
                    if (rv) {
                        const float mean = mpre[i];
                        rstd = rpre[i];
#pragma unroll
                        for (int u = 0; u < MAXC; ++u) {
                            const int c = lane + 64 * u;
                            xh[u] = dxh[u] = 0.f;
                            if (c < n) {
                                xh[u] = (zpre[i][u] - mean) * rstd;
                                const float dy = mul_rn(D[lr * ds + c], silu_grad_p(g[u] * xh[u] + bt[u]));
                                dxh[u] = mul_rn(dy, g[u]);
                                s1 += dxh[u];
                                s2 += mul_rn(dxh[u], xh[u]);
                                pg[u] += mul_rn(dy, xh[u]);
                                pb[u] += dy;
                            }
                        }
                    } else {
#pragma unroll
                        for (int u = 0; u < MAXC; ++u) xh[u] = dxh[u] = 0.f;
                    }
                    const float m1 = wave_sum(s1) * inv_n, m2 = wave_sum(s2) * inv_n;
#pragma unroll
                    for (int u = 0; u < MAXC; ++u) {
                        const int c = lane + 64 * u;
                        if (c < n16) {
                            float dzv = 0.f;
                            if (rv && c < n) {
                                dzv = rstd * (dxh[u] - m1 - xh[u] * m2);
                                Lr.dz[(size_t)row * Lr.lddz + c] = dzv;
                            }
                            D[lr * ds + c] = dzv;
                        }
                    }
                }
            }
            float* cw = colp + (size_t)wave * 2 * n;
#pragma unroll
            for (int u = 0; u < MAXC; ++u) {
                const int c = lane + 64 * u;
                if (c < n) {
                    cw[c] = pg[u];
                    cw[n + c] = pb[u];
                }
            }
        }
        MARL_TS();
        lds_barrier();
        MARL_TS();
        for (int c = tid; c < 2 * n; c += nthreads) {
            float t = 0.f;
            for (int w = 0; w < nwaves; ++w) t += colp[(size_t)w * 2 * n + c];
            Lr.part[(size_t)blockIdx.x * 2 * n + c] = t;
        }
        if (l + 1 < nlayers) zfetch(P.layer[l + 1], ST ? SH::n(l + 1 < SH::kLayers ? l + 1 : 0) : P.layer[l + 1].n);
        MARL_TS();
        // ---- dX = dz * W: out tiles over k_in columns, contraction over n
        const int nout = ST ? SH::k(l) : Lr.k_in, nt = (nout + 31) >> 5;
        const int ks = panel_ksplit(n, nt, nwaves);
        const int kper = (((n16 + ks - 1) / ks) + 15) & ~15;
        const bool last = l + 1 == nlayers;
        const bool tail_lds = ST || P.tail_lds;
        const int es = panel_stride(nout), o16 = (nout + 15) & ~15;
        // more column tiles than waves: walk them in rounds (first layer's input can be wide)
        for (int t0 = 0; t0 < nt; t0 += nwaves / ks) {
            const int tiles_round = nwaves / ks;
            const int j = t0 + wave % tiles_round, s = wave / tiles_round;
            const bool active = s < ks && j < nt;
            f32x4 acc[2];
            if constexpr (ST) {
                if (active) panel_gemm_layer<SH, true>(l, acc, D, ds, Lr.wtfrag, j, s, lane);
            } else {
                const int kbeg = s * kper;
                const int kend = kbeg + kper < n16 ? kbeg + kper : n16;
                if (active) panel_gemm(acc, D, ds, Lr.wtfrag, Lr.wgroups, j, kbeg, kend, lane);
            }
            // slice partials are indexed by the tile's slot in this round
            panel_ksum(acc, part, tiles_round, ks, wave % tiles_round, s, lane, active);
            if (active && s == 0) {
                int rw[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) rw[r] = last ? rowmap[4 * quad + r] : -1;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int col = j * 32 + 16 * t + l16;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int lr = 4 * quad + r;
                        const int row = rw[r];
                        const float v = col < nout ? acc[t][r] : 0.f;
                        if (last && tail_lds) {  // final dX through LDS: finished row-wise below
                            if (col < o16) E[lr * es + col] = v;
                        } else if (last) {
                            if (col < nout && row >= 0) {
                                float* o = P.dx + (size_t)row * P.lddx + col;
                                const float tot = P.accumulate ? *o + v : v;
                                *o = tot;
                                if (P.has_cellb) lstm_cell_bwd_at(P.cellb, row, col, tot);
                            }
                        } else if (col < o16) {
                            E[lr * es + col] = v;
                        }
                    }
                }
            }
            lds_barrier();
        }
        MARL_TS();
        if (last && tail_lds) {
            // Final dX (+ the belief cell's elementwise backward) ROW-wise from the LDS panel: four
            // consecutive columns per thread, 16-byte loads of everything two items need before
            // the first store.  In the accumulator layout the same work is eight scattered
            // elements per lane whose stores keep the next element's loads from being issued
            // (in-kernel timestamps: 20 us of the 46 us chain).
            const LstmBwdArgs& Cb = P.cellb;
            const int c4n = nout >> 2, items = kPanelRows * c4n, cn = ST ? nout : Cb.n;  // (launcher: cellb.n == k_in)
            // (one item per pass: two in flight need 162 registers and then the riding-along cell
            // workgroups no longer fit beside a panel workgroup)
            constexpr int kIt = 1;
            for (int base = 0; base < items; base += kIt * nthreads) {
                float4 ov[kIt], gi[kIt], gf[kIt], gg[kIt], go[kIt], cnew[kIt], cprev[kIt], dcv[kIt];
                int rowi[kIt], coli[kIt], lri[kIt];
#pragma unroll
                for (int k = 0; k < kIt; ++k) {
                    const int i = base + tid + k * nthreads;
                    const int lr = i < items ? i / c4n : 0;
                    const int c = i < items ? (i - lr * c4n) * 4 : 0;
                    const int row = i < items ? rowmap[lr] : -1;
                    const size_t rr = row < 0 ? 0 : (size_t)row;
                    rowi[k] = row;
                    coli[k] = c;
                    lri[k] = lr;
                    ov[k] = P.accumulate ? *reinterpret_cast<const float4*>(P.dx + rr * P.lddx + c)
                                         : make_float4(0.f, 0.f, 0.f, 0.f);
                    if (P.has_cellb) {
                        const float* g = Cb.gates + rr * Cb.ldg + c;
                        gi[k] = *reinterpret_cast<const float4*>(g);
                        gf[k] = *reinterpret_cast<const float4*>(g + cn);
                        gg[k] = *reinterpret_cast<const float4*>(g + 2 * cn);
                        go[k] = *reinterpret_cast<const float4*>(g + 3 * cn);
                        cnew[k] = *reinterpret_cast<const float4*>(Cb.c_new + rr * Cb.ldc + c);
                        cprev[k] = *reinterpret_cast<const float4*>(Cb.c_prev + rr * Cb.ldc + c);
                        dcv[k] = *reinterpret_cast<const float4*>(Cb.dc + rr * Cb.lddc + c);
                    }
                }
#pragma unroll
                for (int k = 0; k < kIt; ++k) {
                    if (rowi[k] < 0) continue;
                    const float4 v = *reinterpret_cast<const float4*>(E + lri[k] * es + coli[k]);
                    const float tot[4] = {ov[k].x + v.x, ov[k].y + v.y, ov[k].z + v.z, ov[k].w + v.w};
                    *reinterpret_cast<float4*>(P.dx + (size_t)rowi[k] * P.lddx + coli[k]) =
                        make_float4(tot[0], tot[1], tot[2], tot[3]);
                    if (P.has_cellb) {  // lstm_cell_bwd_at() on four consecutive units
                        const float gi_[4] = {gi[k].x, gi[k].y, gi[k].z, gi[k].w};
                        const float gf_[4] = {gf[k].x, gf[k].y, gf[k].z, gf[k].w};
                        const float gg_[4] = {gg[k].x, gg[k].y, gg[k].z, gg[k].w};
                        const float go_[4] = {go[k].x, go[k].y, go[k].z, go[k].w};
                        const float cn_[4] = {cnew[k].x, cnew[k].y, cnew[k].z, cnew[k].w};
                        const float cp_[4] = {cprev[k].x, cprev[k].y, cprev[k].z, cprev[k].w};
                        const float dc_[4] = {dcv[k].x, dcv[k].y, dcv[k].z, dcv[k].w};
                        float o0[4], o1[4], o2[4], o3[4], o4[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float tc = tanh_fast(cn_[q]);
                            const float d = tot[q] * go_[q] * (1.0f - tc * tc) + dc_[q];
                            o0[q] = d * gg_[q] * gi_[q] * (1.0f - gi_[q]);
                            o1[q] = d * cp_[q] * gf_[q] * (1.0f - gf_[q]);
                            o2[q] = d * gi_[q] * (1.0f - gg_[q] * gg_[q]);
                            o3[q] = tot[q] * tc * go_[q] * (1.0f - go_[q]);
                            o4[q] = d * gf_[q];
                        }
                        if (!(Cb.g3 && Cb.skip_f32)) {
                            float* g = Cb.gates + (size_t)rowi[k] * Cb.ldg + coli[k];
                            *reinterpret_cast<float4*>(g) = make_float4(o0[0], o0[1], o0[2], o0[3]);
                            *reinterpret_cast<float4*>(g + cn) = make_float4(o1[0], o1[1], o1[2], o1[3]);
                            *reinterpret_cast<float4*>(g + 2 * cn) = make_float4(o2[0], o2[1], o2[2], o2[3]);
                            *reinterpret_cast<float4*>(g + 3 * cn) = make_float4(o3[0], o3[1], o3[2], o3[3]);
                        }
                        *reinterpret_cast<float4*>(Cb.dc + (size_t)rowi[k] * Cb.lddc + coli[k]) =
                            make_float4(o4[0], o4[1], o4[2], o4[3]);
                        if (Cb.g3) {  // the k16 image of the gate gradients (A operand of the image GEMMs)
                            const int64_t ir = (int64_t)Cb.g3_row0 + rowi[k];
                            const int c0 = coli[k];
                            img_store4(Cb.g3 + img_off(ir, c0 >> 4, Cb.g3_steps), c0, o0[0], o0[1], o0[2], o0[3]);
                            img_store4(Cb.g3 + img_off(ir, (cn + c0) >> 4, Cb.g3_steps), cn + c0, o1[0], o1[1], o1[2], o1[3]);
                            img_store4(Cb.g3 + img_off(ir, (2 * cn + c0) >> 4, Cb.g3_steps), 2 * cn + c0, o2[0], o2[1], o2[2], o2[3]);
                            img_store4(Cb.g3 + img_off(ir, (3 * cn + c0) >> 4, Cb.g3_steps), 3 * cn + c0, o3[0], o3[1], o3[2], o3[3]);
                        }
                    }
                }
            }
        }
        MARL_TS();
        float* tmp = D;
        D = E;
        E = tmp;
    }
}

int panel_bwd_blocks(int m) { return (int)cdiv(m, kPanelRows); }
int panel_chain_blocks(int na, int nb) { return na >= 1 && na <= kPanelRows ? (int)cdiv(nb, kPanelRows / na) : 0; }
int panel_chain_by_batch(int na) { return na >= 1 && na <= kPanelRows ? kPanelRows / na : 0; }

// What launch_panel_bwd decides before it launches (checks, LDS layout and the launcher-filled fields written into p);
// host arithmetic only, shared with marl_panel_plan (marl_hip_panelops.h).
struct PanelBwdPlan {
    int waves, maxc;
    size_t lds;
    unsigned pblocks, cblocks;
    bool retried;
};
static int panel_bwd_plan(PanelBwdProb& p, PanelBwdPlan& pl) {
    int waves = 8, pmax = 0, nmax = 0, prm = 0;
    pl.retried = false;
    // the last layer's dX goes through LDS and is finished row-wise (16-byte accesses) when its
    // rows keep float4 alignment
    const PanelBwdLayer& Ll = p.layer[p.nlayers - 1];
    bool tail_lds = (Ll.k_in & 3) == 0 && (p.lddx & 3) == 0 &&
                    (!p.has_cellb || ((p.cellb.n & 3) == 0 && (p.cellb.ldg & 3) == 0 && (p.cellb.ldc & 3) == 0 &&
                                      (p.cellb.lddc & 3) == 0 && p.cellb.n == Ll.k_in)) &&
                    true;
plan:  // (second pass without the LDS tail when the extra output panel does not fit)
    waves = 8;
    pmax = nmax = prm = 0;
    p.tail_lds = tail_lds ? 1 : 0;
    for (int l = 0; l < p.nlayers; ++l) {
        const PanelBwdLayer& L = p.layer[l];
        if (!L.wtfrag) {
            set_error("panel backward: layer %d has no fragment-order copy of its transposed weight", l);
            return MARL_EINVAL;
        }
        if (L.wgroups != panel_frag_groups(L.n)) {
            set_error("panel backward: layer %d's weight copy has %d groups, its width %d needs %d", l, L.wgroups, L.n,
                      panel_frag_groups(L.n));
            return MARL_ELIMIT;
        }
        if (L.n > 64 * kBwdMaxCols) {
            set_error("panel backward: LayerNorm width %d > %d", L.n, 64 * kBwdMaxCols);
            return MARL_ELIMIT;
        }
        int w = panel_waves_for(L.n, L.k_in);
        if (w < 0) w = kPanelMaxWaves;  // wide input: tiles are walked in rounds
        waves = w > waves ? w : waves;
        nmax = L.n > nmax ? L.n : nmax;
        pmax = panel_stride(L.n) > pmax ? panel_stride(L.n) : pmax;
        if ((l + 1 < p.nlayers || tail_lds) && panel_stride(L.k_in) > pmax) pmax = panel_stride(L.k_in);
        prm += 2 * L.n;
    }
    if (waves > kPanelMaxWaves) waves = kPanelMaxWaves;
    p.off_e = kPanelRows * pmax;
    p.off_prm = 2 * kPanelRows * pmax;
    p.off_colp = p.off_prm + prm + 16;
    p.off_part = p.off_colp + waves * 2 * nmax;
    p.off_rowmap = p.off_part + (waves - 1) * 512;
    p.off_mix = p.off_rowmap + kPanelRows;  // (g_na^2 <= kPanelRows^2 floats; fits every plan use_chain admits, see forward)
    if (p.mix && p.agg_at <= 0) {
        set_error("panel backward: a mixing matrix needs the in-panel aggregation");
        return MARL_ELIMIT;
    }
    if (p.gate.pos && (!p.mix || p.by_batch * p.g_na * p.g_na > kPanelRows * kPanelRows)) {
        set_error("panel backward: a position gate needs a base matrix and by_batch * agents^2 <= %d",
                  kPanelRows * kPanelRows);
        return MARL_ELIMIT;
    }
    const size_t lds = (size_t)(p.off_mix + (p.mix ? kPanelRows * kPanelRows : 0)) * sizeof(float);
    if (p.agg_at > 0 && (p.by_batch < 1 || p.g_na * p.by_batch > kPanelRows || p.agg_at >= p.nlayers ||
                         !panel_chain_supported(p.g_na, p.layer[p.agg_at].n, 256))) {
        set_error("panel backward: in-panel message mean outside its range");
        return MARL_ELIMIT;
    }
    // (the matrix's 1 KiB could tip a plan that kept tail_lds without one into the retry below - same results, the
    // final dX then leaves without the LDS tail; with n_b <= 384 under a matrix (use_chain) no admitted plan gets here)
    if (lds > kPanelMaxLds && tail_lds) {
        tail_lds = false;
        pl.retried = true;
        goto plan;
    }
    if (lds > kPanelMaxLds) {
        set_error("panel backward: shape outside its range");
        return MARL_ELIMIT;
    }
    pl.pblocks = p.by_batch > 0 ? (unsigned)cdiv(p.g_nb, p.by_batch) : (unsigned)cdiv(p.m, kPanelRows);
    p.cellb_img_done = p.has_cellb && p.cellb.g3 && tail_lds;
    p.cell_vec4 = p.has_cell && lstm_bwd_vec4_ok(p.cell);
    p.cell_img_done = p.has_cell && p.cell.g3 && p.cell_vec4;
    if (!p.cellb_img_done) p.cellb.skip_f32 = 0;  // (the fallback builds the image from the fp32 gradients)
    if (!p.cell_img_done) p.cell.skip_f32 = 0;
    pl.waves = waves;
    pl.lds = lds;
    pl.maxc = nmax <= 128 ? 2 : kBwdMaxCols;
    pl.cblocks = 0;
    if (p.has_cell) {
        p.panel_blocks = (int)pl.pblocks;
        pl.cblocks = (unsigned)cdiv(p.cell_rows * (p.cell_vec4 ? p.cell.n / 4 : p.cell.n), 64 * waves);
    }
    return MARL_OK;
}

// the launch is the plain by-batch chain of net SH, planned as SH's layout has it
template <class SH>
static bool panel_bwd_static_ok(const PanelBwdProb& p, const PanelBwdPlan& pl) {
    if (!panel_static_env() || p.mix || p.gate.pos || p.nlayers != SH::kLayers || p.agg_na != 0 || p.by_batch < 1 ||
        p.agg_at != SH::kAggAt || !p.tail_lds || pl.maxc != 2 || pl.waves != SH::kWaves)
        return false;
    for (int l = 0; l < SH::kLayers; ++l)
        if (p.layer[l].n != SH::n(l) || p.layer[l].k_in != SH::k(l) || p.layer[l].wgroups != panel_frag_groups(SH::n(l)))
            return false;
    if (p.has_cellb && p.cellb.n != SH::kKLast) return false;
    return p.off_e == SH::off_e && p.off_prm == SH::off_prm && p.off_colp == SH::off_colp && p.off_part == SH::off_part &&
           p.off_rowmap == SH::off_rowmap;
}

int launch_panel_bwd(PanelBwdProb& p, hipStream_t st) {
    PanelBwdPlan pl;
    MARL_TRY(panel_bwd_plan(p, pl));
    const int waves = pl.waves, maxc = pl.maxc;
    const size_t lds = pl.lds;
    const unsigned pblocks = pl.pblocks;
    static bool raised = false;
    if (!raised) {
        const void* kerns[15] = {reinterpret_cast<const void*>(panel_bwd_kernel<PanelBwdChainNet, false, 2>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelBwdChainNet, true, 2>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelBwdDecNet, false, 2>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, false, 2>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, true, 2>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, false, kBwdMaxCols>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, true, kBwdMaxCols>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, false, 2, true>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, true, 2, true>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, false, kBwdMaxCols, true>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, true, kBwdMaxCols, true>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, false, 2, true, true>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, true, 2, true, true>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, false, kBwdMaxCols, true, true>),
                                reinterpret_cast<const void*>(panel_bwd_kernel<PanelDyn, true, kBwdMaxCols, true, true>)};
        for (const void* kf : kerns)
            MARL_HIP_CHECK(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPanelMaxLds));
        raised = true;
    }
    prof_before(4, st);
#ifdef MARL_KERNEL_TS
    static long long* d_ts = nullptr;
    static int calls = 0;
    const int rec = ts_begin(&d_ts, calls++);
    p.ts = rec ? d_ts : nullptr;
#endif
    const unsigned cblocks = pl.cblocks;
    if (panel_bwd_static_ok<PanelBwdChainNet>(p, pl)) {
        if (p.has_cell)
            hipLaunchKernelGGL((panel_bwd_kernel<PanelBwdChainNet, true, 2>), dim3(pblocks + cblocks), dim3(64 * waves), lds,
                               st, p);
        else
            hipLaunchKernelGGL((panel_bwd_kernel<PanelBwdChainNet, false, 2>), dim3(pblocks), dim3(64 * waves), lds, st, p);
    } else if (!p.has_cell && panel_bwd_static_ok<PanelBwdDecNet>(p, pl)) {
        hipLaunchKernelGGL((panel_bwd_kernel<PanelBwdDecNet, false, 2>), dim3(pblocks), dim3(64 * waves), lds, st, p);
    } else if (p.mix) {
        const dim3 blk(64 * waves);
        if (p.gate.pos) {
            if (p.has_cell && maxc == 2)
                hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, true, 2, true, true>), dim3(pblocks + cblocks), blk, lds, st, p);
            else if (p.has_cell)
                hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, true, kBwdMaxCols, true, true>), dim3(pblocks + cblocks), blk, lds,
                                   st, p);
            else if (maxc == 2)
                hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, false, 2, true, true>), dim3(pblocks), blk, lds, st, p);
            else
                hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, false, kBwdMaxCols, true, true>), dim3(pblocks), blk, lds, st, p);
        } else if (p.has_cell && maxc == 2)
            hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, true, 2, true>), dim3(pblocks + cblocks), blk, lds, st, p);
        else if (p.has_cell)
            hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, true, kBwdMaxCols, true>), dim3(pblocks + cblocks), blk, lds, st, p);
        else if (maxc == 2)
            hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, false, 2, true>), dim3(pblocks), blk, lds, st, p);
        else
            hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, false, kBwdMaxCols, true>), dim3(pblocks), blk, lds, st, p);
    } else if (p.has_cell) {
        if (maxc == 2)
            hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, true, 2>), dim3(pblocks + cblocks), dim3(64 * waves), lds, st, p);
        else
            hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, true, kBwdMaxCols>), dim3(pblocks + cblocks), dim3(64 * waves), lds, st, p);
    } else if (maxc == 2) {
        hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, false, 2>), dim3(pblocks), dim3(64 * waves), lds, st, p);
    } else {
        hipLaunchKernelGGL((panel_bwd_kernel<PanelDyn, false, kBwdMaxCols>), dim3(pblocks), dim3(64 * waves), lds, st, p);
    }
    prof_after(4, st);
    MARL_LAUNCH_CHECK();
#ifdef MARL_KERNEL_TS
    if (rec) {
        fprintf(stderr, "[ts] panel_bwd layers %d waves %d lds %zu cell %d cellb %d tail_lds %d\n", p.nlayers, waves, lds,
                p.has_cell, p.has_cellb, p.tail_lds);
        ts_report("panel_bwd", d_ts, waves);
    }
#endif
    return MARL_OK;
}

}  // namespace marl

// ===========================================================================
// kernel-level hooks of the panel launchers (include/marl_hip_panelops.h; not part of the versioned ABI): host code
// only - plain-C descriptors in, PanelFwdBatch / PanelBwdProb to the launchers above as the episode would fill them
// ===========================================================================
#include "../../include/marl_hip_panelops.h"

using namespace marl;

namespace {

constexpr int kApiMaxWidth = 64 * kPanelMaxCols;  // 384: the widest LayerNorm row either kernel holds
static float g_here[4];                           // stands for a weight copy where only its presence matters (plans)

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int round4(int v) { return (v + 3) & ~3; }

// a [rows][ld] fp32 matrix the kernels access 16 bytes at a time, cols rounded up to 4 per row
bool vec_ok(const void* p, int ld, int cols) { return p && al16(p) && (ld & 3) == 0 && ld >= round4(cols); }

LstmBwdArgs cell_args(const marl_panel_cell& c) {
    LstmBwdArgs a{};
    a.dh = c.dh, a.dc = c.dc, a.gates = c.gates, a.c_prev = c.c_prev, a.c_new = c.c_new;
    a.lddh = c.lddh, a.lddc = c.lddc, a.ldg = c.ldg, a.ldc = c.ldc, a.n = c.n;
    a.g3 = static_cast<char*>(c.g3), a.g3_row0 = c.g3_row0, a.g3_steps = c.g3_steps, a.skip_f32 = c.skip_f32;
    return a;
}

// the fragment-order copies a call builds: zero fill of the scratch, (backward) row-major transposes, then the
// frag form of launch_permute - the routine that builds the product's copies (episode.hip, pack)
struct FragJobs {
    PermBatch transposes, frags;
    size_t floats;
};

// by_batch / g_na / g_nb / m of either direction
int check_grouping(const char* who, int& by_batch, int g_na, int g_nb, int m, int agg_at, int nlayers,
                   const float* mix) {
    if (by_batch < 0) by_batch = panel_chain_by_batch(g_na);
    if (by_batch > 0) {
        if (g_na < 1 || g_nb < 1 || (int64_t)g_na * g_nb != m) {
            set_error("%s: by_batch needs g_na, g_nb >= 1 and m == g_na * g_nb", who);
            return MARL_EINVAL;
        }
        if (by_batch * g_na > kPanelRows) {
            set_error("%s: by_batch * g_na = %d > %d panel rows", who, by_batch * g_na, kPanelRows);
            return MARL_ELIMIT;
        }
    }
    if (mix && agg_at <= 0) {
        set_error("%s: a mixing matrix needs the in-panel aggregation (agg_at > 0)", who);
        return MARL_ELIMIT;
    }
    if (agg_at < 0 || (agg_at > 0 && (by_batch < 1 || agg_at >= nlayers))) {
        set_error("%s: agg_at needs by_batch > 0 and 0 < agg_at < nlayers", who);
        return MARL_EINVAL;
    }
    return MARL_OK;
}

int build_fwd(const marl_panel_fwd_prob* probs, int count, float* scratch, size_t scratch_bytes, bool plan_only,
              PanelFwdBatch& b, FragJobs& jobs) {
    if (!probs || count < 1 || count > 2) {
        set_error("marl_panel_fwd: one or two problems");
        return MARL_EINVAL;
    }
    b = PanelFwdBatch{};
    b.count = count;
    jobs.transposes.count = jobs.frags.count = 0;
    jobs.floats = 0;
    for (int i = 0; i < count; ++i) {
        const marl_panel_fwd_prob& q = probs[i];
        PanelFwdProb& p = b.p[i];
        if (q.sample || q.explore || q.gate_pos) {
            set_error("marl_panel_fwd: the sampling epilogue, exploration controls and the position gate are not served here");
            return MARL_EINVAL;
        }
        if (q.nlayers < 1 || q.nlayers > kPanelMaxLayers || q.m < 1 || q.k0 < 1) {
            set_error("marl_panel_fwd: 1..%d layers, m >= 1, k0 >= 1", kPanelMaxLayers);
            return MARL_EINVAL;
        }
        if (!vec_ok(q.x, q.ldx, q.k0)) {
            set_error("marl_panel_fwd: x must be 16-byte aligned with ldx %% 4 == 0 and ldx >= round4(k0)");
            return MARL_EINVAL;
        }
        int by_batch = q.by_batch;
        MARL_TRY(check_grouping("marl_panel_fwd", by_batch, q.g_na, q.g_nb, q.m, q.agg_at, q.nlayers, q.mix));
        if (q.agg_na < 0 || (q.agg_na > 0 && (q.agg_nb < 1 || (int64_t)q.agg_na * q.agg_nb != q.m))) {
            set_error("marl_panel_fwd: the staged mean needs m == agg_na * agg_nb");
            return MARL_EINVAL;
        }
        if (q.xbar && q.agg_na > 0 && !al16(q.xbar)) {
            set_error("marl_panel_fwd: xbar must be 16-byte aligned");
            return MARL_EINVAL;
        }
        p.x = q.x, p.ldx = q.ldx, p.k0 = q.k0, p.agg_na = q.agg_na, p.agg_nb = q.agg_nb, p.xbar = q.xbar;
        p.m = q.m, p.nlayers = q.nlayers;
        p.by_batch = by_batch, p.g_na = q.g_na, p.g_nb = q.g_nb, p.agg_at = q.agg_at, p.ld_xbar = q.ld_xbar;
        p.mix = q.mix;
        int kin = q.k0;
        for (int l = 0; l < q.nlayers; ++l) {
            const marl_panel_layer& s = q.layer[l];
            if (s.n < 1 || s.n > kApiMaxWidth || (l > 0 && kin > kApiMaxWidth)) {
                set_error("marl_panel_fwd: layer %d width %d outside 1..%d", l, s.n, kApiMaxWidth);
                return MARL_ELIMIT;
            }
            if (!s.w) {
                set_error("marl_panel_fwd: layer %d has no weight (null fragment source)", l);
                return MARL_EINVAL;
            }
            if (s.ldw < kin || !s.bias || !s.gamma || !s.beta || !s.a || s.lda < s.n || (s.z && s.ldz < s.n)) {
                set_error("marl_panel_fwd: layer %d: null vector or output, or a leading dimension below its width", l);
                return MARL_EINVAL;
            }
            if (s.a3 && ((s.n & 3) || (s.a3_col0 & 3) || s.a3_col0 < 0 || s.a3_row0 < 0 ||
                         s.a3_col0 + s.n > 16 * s.a3_steps)) {
                set_error("marl_panel_fwd: layer %d: an image needs n and a3_col0 multiples of 4 inside a3_steps", l);
                return MARL_EINVAL;
            }
            if (l == q.agg_at && l > 0 && q.xbar && !vec_ok(q.xbar, q.ld_xbar, kin)) {
                set_error("marl_panel_fwd: xbar must be 16-byte aligned with ld_xbar %% 4 == 0 and >= round4(width)");
                return MARL_EINVAL;
            }
            PanelLayer& d = p.layer[l];
            d.wgroups = panel_frag_groups(kin);
            d.bias = s.bias, d.gamma = s.gamma, d.beta = s.beta, d.n = s.n;
            d.z = s.z, d.ldz = s.ldz, d.stats = s.stats, d.a = s.a, d.lda = s.lda;
            d.a3 = static_cast<char*>(s.a3), d.a3_row0 = s.a3_row0, d.a3_steps = s.a3_steps, d.a3_col0 = s.a3_col0;
            const size_t fl = panel_frag_floats(s.n, kin);
            if (plan_only) {
                d.wfrag = g_here;
            } else {
                d.wfrag = scratch + jobs.floats;
                PermDesc pd{};
                pd.src = s.w, pd.dst = scratch + jobs.floats, pd.rows = s.n, pd.cols = kin;
                pd.rd = 1, pd.rs1 = s.ldw, pd.cd = 1, pd.cs1 = 1, pd.frag = d.wgroups;
                jobs.frags.d[jobs.frags.count++] = pd;
            }
            jobs.floats += fl;
            kin = s.n;
        }
    }
    if (!plan_only && (!scratch || !al16(scratch) || scratch_bytes < jobs.floats * sizeof(float))) {
        set_error("marl_panel_fwd: scratch too small or misaligned (%zu bytes needed)", jobs.floats * sizeof(float));
        return MARL_ESIZE;
    }
    return MARL_OK;
}

int check_cell(const char* which, const marl_panel_cell& c, bool needs_dh) {
    if (c.n < 1 || !c.dc || !c.gates || !c.c_prev || !c.c_new || (needs_dh && (!c.dh || c.lddh < c.n)) ||
        c.lddc < c.n || c.ldc < c.n || c.ldg < 4 * c.n) {
        set_error("marl_panel_bwd: %s: null pointer or a leading dimension below its width", which);
        return MARL_EINVAL;
    }
    // the four-wide forms (chosen by the launcher from n and the leading dimensions) access 16 bytes at a time
    if (!al16(c.dc) || !al16(c.gates) || !al16(c.c_prev) || !al16(c.c_new) || (needs_dh && !al16(c.dh))) {
        set_error("marl_panel_bwd: %s: pointers must be 16-byte aligned", which);
        return MARL_EINVAL;
    }
    if (c.g3 && (c.g3_row0 < 0 || 4 * c.n > 16 * c.g3_steps)) {
        set_error("marl_panel_bwd: %s: the image needs g3_steps >= 4 n / 16", which);
        return MARL_EINVAL;
    }
    return MARL_OK;
}

int build_bwd(const marl_panel_bwd_prob* qp, float* scratch, size_t scratch_bytes, bool plan_only, PanelBwdProb& p,
              FragJobs& jobs) {
    if (!qp) {
        set_error("marl_panel_bwd: null argument");
        return MARL_EINVAL;
    }
    const marl_panel_bwd_prob& q = *qp;
    p = PanelBwdProb{};
    jobs.transposes.count = jobs.frags.count = 0;
    jobs.floats = 0;
    if (q.gate_pos) {
        set_error("marl_panel_bwd: the position gate is not served here");
        return MARL_EINVAL;
    }
    if (q.nlayers < 1 || q.nlayers > kPanelMaxLayers || q.m < 1) {
        set_error("marl_panel_bwd: 1..%d layers, m >= 1", kPanelMaxLayers);
        return MARL_EINVAL;
    }
    int by_batch = q.by_batch;
    MARL_TRY(check_grouping("marl_panel_bwd", by_batch, q.g_na, q.g_nb, q.m, q.agg_at, q.nlayers, q.mix));
    if (q.agg_na < 0 || (q.agg_na > 0 && (q.agg_nb < 1 || (int64_t)q.agg_na * q.agg_nb != q.m))) {
        set_error("marl_panel_bwd: the staged mean needs m == agg_na * agg_nb");
        return MARL_EINVAL;
    }
    if (!vec_ok(q.da, q.ldda, q.layer[0].n) || (q.da2 && !vec_ok(q.da2, q.ldda2, q.layer[0].n))) {
        set_error("marl_panel_bwd: da / da2 must be 16-byte aligned with ld %% 4 == 0 and ld >= round4(n)");
        return MARL_EINVAL;
    }
    const int k_last = q.layer[q.nlayers - 1].k_in;
    if (!q.dx || !al16(q.dx) || q.lddx < k_last) {
        set_error("marl_panel_bwd: dx must be 16-byte aligned with lddx >= the first layer's input width");
        return MARL_EINVAL;
    }
    p.da = q.da, p.ldda = q.ldda, p.da2 = q.da2, p.ldda2 = q.ldda2, p.agg_na = q.agg_na, p.agg_nb = q.agg_nb;
    p.m = q.m, p.nlayers = q.nlayers, p.dx = q.dx, p.lddx = q.lddx, p.accumulate = q.accumulate ? 1 : 0;
    p.by_batch = by_batch, p.g_na = q.g_na, p.g_nb = q.g_nb, p.agg_at = q.agg_at, p.mix = q.mix;
    size_t tr_floats = 0;
    for (int l = 0; l < q.nlayers; ++l) {
        const marl_panel_bwd_layer& s = q.layer[l];
        if (s.n < 1 || s.n > kApiMaxWidth || s.k_in < 1) {
            set_error("marl_panel_bwd: layer %d width %d outside 1..%d", l, s.n, kApiMaxWidth);
            return MARL_ELIMIT;
        }
        if (l + 1 < q.nlayers && q.layer[l + 1].n != s.k_in) {
            set_error("marl_panel_bwd: layer %d's input width %d is not layer %d's width %d", l, s.k_in, l + 1,
                      q.layer[l + 1].n);
            return MARL_EINVAL;
        }
        if (!s.w) {
            set_error("marl_panel_bwd: layer %d has no weight (null fragment source)", l);
            return MARL_EINVAL;
        }
        if (s.ldw < s.k_in || !s.z || s.ldz < s.n || !s.stats || !s.gamma || !s.beta || !s.dz || s.lddz < s.n ||
            !s.part) {
            set_error("marl_panel_bwd: layer %d: null pointer or a leading dimension below its width", l);
            return MARL_EINVAL;
        }
        PanelBwdLayer& d = p.layer[l];
        d.z = s.z, d.ldz = s.ldz, d.stats = s.stats, d.gamma = s.gamma, d.beta = s.beta, d.n = s.n;
        d.dz = s.dz, d.lddz = s.lddz, d.part = s.part, d.k_in = s.k_in;
        d.wgroups = panel_frag_groups(s.n);
        d.wtfrag = g_here;
        jobs.floats += panel_frag_floats(s.k_in, s.n);
        tr_floats += (size_t)s.k_in * s.n;
    }
    if (q.has_cellb) {
        MARL_TRY(check_cell("cellb", q.cellb, false));
        if (q.cellb.n != k_last) {
            set_error("marl_panel_bwd: cellb.n %d is not the first layer's input width %d", q.cellb.n, k_last);
            return MARL_EINVAL;
        }
        p.has_cellb = 1;
        p.cellb = cell_args(q.cellb);
    }
    if (q.has_cell) {
        MARL_TRY(check_cell("cell", q.cell, true));
        if (q.cell_rows < 1) {
            set_error("marl_panel_bwd: cell_rows < 1");
            return MARL_EINVAL;
        }
        p.has_cell = 1;
        p.cell = cell_args(q.cell);
        p.cell_rows = q.cell_rows;
    }
    const size_t frag_floats = jobs.floats;
    jobs.floats += (tr_floats + 3) & ~(size_t)3;
    if (plan_only) return MARL_OK;
    if (!scratch || !al16(scratch) || scratch_bytes < jobs.floats * sizeof(float)) {
        set_error("marl_panel_bwd: scratch too small or misaligned (%zu bytes needed)", jobs.floats * sizeof(float));
        return MARL_ESIZE;
    }
    size_t off = 0, toff = frag_floats;
    for (int l = 0; l < q.nlayers; ++l) {
        const marl_panel_bwd_layer& s = q.layer[l];
        // W^T [k_in][n] row-major behind the copies, then its fragment-order copy
        PermDesc t{};
        t.src = s.w, t.dst = scratch + toff, t.rows = s.k_in, t.cols = s.n, t.dst_ld = s.n;
        t.rd = 1, t.rs1 = 1, t.rs2 = 0, t.cd = 1, t.cs1 = s.ldw, t.cs2 = 0;
        jobs.transposes.d[jobs.transposes.count++] = t;
        PermDesc f{};
        f.src = scratch + toff, f.dst = scratch + off, f.rows = s.k_in, f.cols = s.n;
        f.rd = 1, f.rs1 = s.n, f.cd = 1, f.cs1 = 1, f.frag = p.layer[l].wgroups;
        jobs.frags.d[jobs.frags.count++] = f;
        p.layer[l].wtfrag = scratch + off;
        off += panel_frag_floats(s.k_in, s.n);
        toff += (size_t)s.k_in * s.n;
    }
    return MARL_OK;
}

int run_jobs(const FragJobs& jobs, float* scratch, hipStream_t st) {
    MARL_TRY(launch_fill(scratch, (int64_t)jobs.floats, 0.f, st));
    if (jobs.transposes.count) MARL_TRY(launch_permute(jobs.transposes, st));
    return launch_permute(jobs.frags, st);
}

void slice_plan(marl_panel_plan_info* out, int i, int K, int n_out, int nwaves) {
    const int nt = (n_out + 31) >> 5, K16 = (K + 15) & ~15;
    const int w = panel_waves_for(K, n_out);
    const int ks = panel_ksplit(K, nt, nwaves), kper = panel_kper_host(K16, ks);
    out->layer_waves[i] = w;
    out->rounds[i] = w < 0;
    out->nt[i] = nt, out->ks[i] = ks, out->kper[i] = kper;
    int empty = 0;
    for (int s = 0; s < ks; ++s)
        if (s * kper >= K16) empty |= 1 << s;
    out->empty[i] = empty;
}

}  // namespace

size_t marl_panel_scratch_bytes(int backward, int nlayers, const int* n, const int* k) {
    if (nlayers < 1 || nlayers > kPanelMaxLayers || !n || !k) return 0;
    size_t floats = 0, tr = 0;
    for (int l = 0; l < nlayers; ++l) {
        if (n[l] < 1 || k[l] < 1) return 0;
        floats += backward ? panel_frag_floats(k[l], n[l]) : panel_frag_floats(n[l], k[l]);
        tr += (size_t)n[l] * k[l];
    }
    if (backward) floats += (tr + 3) & ~(size_t)3;
    return floats * sizeof(float);
}

int marl_panel_fwd(const marl_panel_fwd_prob* probs, int count, float* scratch, size_t scratch_bytes, void* stream) {
    static PanelFwdBatch b;  // (4 KB-class descriptors: kept off the stack; the entries are not re-entrant)
    static FragJobs jobs;
    MARL_TRY(build_fwd(probs, count, scratch, scratch_bytes, false, b, jobs));
    {
        PanelFwdBatch probe = b;  // every refusal of the launcher before anything is enqueued
        PanelFwdPlan pl;
        MARL_TRY(panel_fwd_plan(probe, pl));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    MARL_TRY(run_jobs(jobs, scratch, st));
    return launch_panel_fwd(b, st);
}

int marl_panel_bwd(marl_panel_bwd_prob* prob, float* scratch, size_t scratch_bytes, void* stream) {
    static PanelBwdProb p;
    static FragJobs jobs;
    MARL_TRY(build_bwd(prob, scratch, scratch_bytes, false, p, jobs));
    {
        PanelBwdProb probe = p;
        PanelBwdPlan pl;
        MARL_TRY(panel_bwd_plan(probe, pl));
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    MARL_TRY(run_jobs(jobs, scratch, st));
    MARL_TRY(launch_panel_bwd(p, st));
    prob->cellb_img_done = p.cellb_img_done;
    prob->cell_img_done = p.cell_img_done;
    return MARL_OK;
}

int marl_panel_plan(const marl_panel_fwd_prob* fwd, int count, const marl_panel_bwd_prob* bwd,
                    marl_panel_plan_info* out) {
    if (!out || (fwd != nullptr) == (bwd != nullptr)) {
        set_error("marl_panel_plan: exactly one of the forward and the backward descriptor, and an output");
        return MARL_EINVAL;
    }
    *out = marl_panel_plan_info{};
    static FragJobs jobs;
    if (fwd) {
        static PanelFwdBatch b;
        MARL_TRY(build_fwd(fwd, count, nullptr, 0, true, b, jobs));
        PanelFwdPlan pl;
        MARL_TRY(panel_fwd_plan(b, pl));
        out->waves = pl.waves, out->lds_bytes = (int)pl.lds, out->blocks = (int)pl.pblocks;
        int i = 0;
        for (int q = 0; q < b.count; ++q) {
            out->by_batch[q] = b.p[q].by_batch;
            int kin = b.p[q].k0;
            for (int l = 0; l < b.p[q].nlayers; ++l, ++i) {
                slice_plan(out, i, kin, b.p[q].layer[l].n, pl.waves);
                out->ln_slots[i] = b.p[q].layer[l].n <= b.ln_narrow_max ? 2 : kPanelMaxCols;
                kin = b.p[q].layer[l].n;
            }
        }
        out->nlayers = i;
        return MARL_OK;
    }
    static PanelBwdProb p;
    MARL_TRY(build_bwd(bwd, nullptr, 0, true, p, jobs));
    PanelBwdPlan pl;
    MARL_TRY(panel_bwd_plan(p, pl));
    out->waves = pl.waves, out->lds_bytes = (int)pl.lds, out->blocks = (int)pl.pblocks;
    out->cell_blocks = (int)pl.cblocks, out->by_batch[0] = p.by_batch, out->nlayers = p.nlayers;
    for (int l = 0; l < p.nlayers; ++l) {  // the dX product: contraction over n, tiles over k_in
        slice_plan(out, l, p.layer[l].n, p.layer[l].k_in, pl.waves);
        out->ln_slots[l] = pl.maxc;
    }
    out->maxc = pl.maxc, out->tail_lds = p.tail_lds, out->retried = pl.retried ? 1 : 0;
    out->cell_vec4 = p.cell_vec4, out->cellb_img_done = p.cellb_img_done, out->cell_img_done = p.cell_img_done;
    return MARL_OK;
}
