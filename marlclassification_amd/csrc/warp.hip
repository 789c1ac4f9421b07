// marl_batch_warp (include/marl_hip_warp.h): the batch gather of the resident image set under an affine map per output
// image - rotation by any angle, zoom, stretch, translation - sampled bilinearly, with reflect / constant padding and
// one erased rectangle.  The map, the fold and the uint8 blend are integer arithmetic and the fp32 blend is made of
// separately rounded products and sums, so the launch is bit for bit warp.reference_apply.  One kernel, no workspace,
// no atomics, no LDS.
//
// Work split.  A workgroup (256 threads) owns a piece of ONE output image; rows[b], mats[b] and ops[b] are loads at a
// workgroup-uniform address, sanitised once.  The stores of a plane, V bytes each, are numbered row-major over its h
// rows; a thread takes one of them: N = V / elt consecutive output pixels of one row.  It resolves each pixel ONCE -
// the offset of tap (y0, x0) inside a plane, the steps to the other three taps (-1, 0 or +1 pixel / row after folding
// or clamping), the two weights, which taps lie outside, whether the rectangle covers it: two registers per pixel -
// and then walks the c planes, where every tap offset is the same: 4 N loads, N blends, one aligned V-byte store per
// plane.  The map is linear in integers, so the thread computes Sy, Sx of its first pixel with 64-bit products and
// adds 2 a01, 2 a11 per pixel: the same integers as the definition's products.
// Taps are direct global loads: neighbouring lanes' taps share cache lines under any rotation.
#include "gather.h"

#include "../../include/marl_hip_warp.h"

namespace marl {
namespace {

constexpr int kWarpThreads = 256;
constexpr int64_t kMaxA = (int64_t)1 << 20;  // |a| <= 16.0
constexpr int64_t kMaxT = (int64_t)1 << 30;  // |t| <= 8192 pixels

struct WarpArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int64_t* rows;
    const int32_t* mats;
    const int32_t* ops;
    int64_t n_src;
    int64_t img_bytes;
    int c, h, w;
    int nv;              // stores per output row
    uint32_t plane_vec;  // h * nv
    int blocks_per_image;
    int reflect;
    uint32_t fill;
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// v mod p in [0, p), p > 0.  Within one period of the image (every map near the identity) it is an add or a
// subtract; a strong zoom-out divides, in 32 bits where the operands fit.
__device__ __forceinline__ int64_t floormod(int64_t v, int64_t p) {
    if (v >= -p && v < 2 * p) return v < 0 ? v + p : (v >= p ? v - p : v);
    if (v >= INT32_MIN && v <= INT32_MAX && p <= INT32_MAX) {
        const int r = (int)v % (int)p;
        return r < 0 ? r + (int)p : r;
    }
    const int64_t r = v % p;
    return r < 0 ? r + p : r;
}

// One axis of one pixel: s = S + (n - 1) 65536 of the definition -> the index of tap 0 inside the image, the step to
// tap 1 (-1, 0, +1), the weight of tap 1 in 1 / 256, and (constant padding) which of the two taps lie outside.
struct Axis {
    int i0, step;
    uint32_t f, outside;  // outside: bit 0 tap 0, bit 1 tap 1
};

__device__ __forceinline__ Axis resolve(int64_t s, int n, int reflect) {
    const int64_t p8 = ((s >> 1) + 128) >> 8;
    const int64_t v = p8 >> 8;
    Axis r;
    r.f = (uint32_t)p8 & 255u;
    r.outside = 0;
    if (reflect) {
        if (n == 1) {
            r.i0 = r.step = 0;
            return r;
        }
        const int64_t p = 2 * ((int64_t)n - 1);
        const int64_t m0 = floormod(v, p);
        const int64_t m1 = m0 + 1 == p ? 0 : m0 + 1;
        r.i0 = (int)(m0 >= n ? p - m0 : m0);
        r.step = (int)(m1 >= n ? p - m1 : m1) - r.i0;
        return r;
    }
    const int vi = (int)clamp64(v, -2, n);  // (-2: both taps outside, like anything further out; n likewise)
    const int c0 = vi < 0 ? 0 : (vi >= n ? n - 1 : vi), c1 = vi < -1 ? 0 : (vi >= n - 1 ? n - 1 : vi + 1);
    r.outside = (uint32_t)(vi < 0 || vi >= n) | ((uint32_t)(vi < -1 || vi >= n - 1) << 1);
    r.i0 = c0;  // (a tap outside is loaded from a clamped, valid address and replaced by the fill)
    r.step = c1 - c0;
    return r;
}

// what a thread keeps of a pixel besides the offset of tap (y0, x0)
constexpr int kFy = 8, kStepX = 16, kStepY = 18, kOutX = 20, kOutY = 22, kErased = 24;

__device__ __forceinline__ uint32_t blend_u8(const uint32_t v[4], uint32_t fx, uint32_t fy) {
    const uint32_t top = v[0] * (256u - fx) + v[1] * fx;
    const uint32_t bot = v[2] * (256u - fx) + v[3] * fx;
    return (top * (256u - fy) + bot * fy + 32768u) >> 16;
}

// separately rounded products and sums; a tap of weight 0 is skipped, not multiplied.  __fmul_rn / __fadd_rn are a
// plain * and + to hipcc, whose default contraction fuses them into v_fmac_f32 whatever a pragma in here says, so both
// products pass through an empty asm: the sum then sees two rounded values it cannot look into.
__device__ __forceinline__ float lerp_f32(float v0, float v1, uint32_t f) {
    if (f == 0) return v0;
    const float w1 = (float)f * (1.0f / 256.0f), w0 = (float)(256u - f) * (1.0f / 256.0f);  // exact
    float p0 = __fmul_rn(v0, w0), p1 = __fmul_rn(v1, w1);
    asm volatile("" : "+v"(p0), "+v"(p1));
    return __fadd_rn(p0, p1);
}

__device__ __forceinline__ uint32_t blend_f32(const uint32_t v[4], uint32_t fx, uint32_t fy) {
    const float top = lerp_f32(__uint_as_float(v[0]), __uint_as_float(v[1]), fx);
    const float bot = lerp_f32(__uint_as_float(v[2]), __uint_as_float(v[3]), fx);
    return __float_as_uint(lerp_f32(top, bot, fy));
}

template <int ELT, int V>
__global__ void __launch_bounds__(kWarpThreads) batch_warp_kernel(const WarpArgs a) {
    constexpr int N = V / ELT;
    constexpr int Q = V >= 4 ? V / 4 : 1;
    constexpr int G = N < 4 ? N : 4;  // pixels whose taps are in flight together
    const int b = blockIdx.x / a.blocks_per_image;
    const int t = blockIdx.x - b * a.blocks_per_image;
    // workgroup-uniform: the matrix, the rectangle, the source row - whatever the values are, every address derived
    // below stays inside the source image and the output row
    const int32_t* __restrict__ m = a.mats + (size_t)b * 8;
    const int64_t a00 = clamp64(m[0], -kMaxA, kMaxA), a01 = clamp64(m[1], -kMaxA, kMaxA);
    const int64_t a10 = clamp64(m[2], -kMaxA, kMaxA), a11 = clamp64(m[3], -kMaxA, kMaxA);
    const int64_t ty = clamp64(m[4], -kMaxT, kMaxT), tx = clamp64(m[5], -kMaxT, kMaxT);
    // (fields 3..6 of ops[b] as gather.h's view_of reads them, read here: fields 0..2 are in the matrices, and taking
    // the rectangle from view_of<false> moves this kernel's code - DESIGN 8.27)
    int ey0 = 0, ey1 = 0, ex0 = 0, ex1 = 0;
    if (a.ops != nullptr) {
        const int32_t* __restrict__ p = a.ops + (size_t)b * 8;
        ey0 = clampl(p[3], 0, a.h);
        ey1 = clampl((int64_t)p[3] + p[5], 0, a.h);
        ex0 = clampl(p[4], 0, a.w);
        ex1 = clampl((int64_t)p[4] + p[6], 0, a.w);
    }
    const uint8_t* __restrict__ sp = a.src + clamp_row(a.rows ? a.rows[b] : (int64_t)b, a.n_src) * a.img_bytes;

    const uint32_t idx = (uint32_t)t * kWarpThreads + threadIdx.x;
    if (idx >= a.plane_vec) return;
    const int y = (int)(idx / (uint32_t)a.nv);
    const int x0 = (int)(idx - (uint32_t)y * (uint32_t)a.nv) * N;

    // the pixels, once for all planes
    const int64_t yc = 2 * (int64_t)y - (a.h - 1), xc = 2 * (int64_t)x0 - (a.w - 1);
    int64_t sy = a00 * yc + a01 * xc + ty + (((int64_t)a.h - 1) << 16);
    int64_t sx = a10 * yc + a11 * xc + tx + (((int64_t)a.w - 1) << 16);
    const bool row_erased = y >= ey0 && y < ey1;
    int off[N];
    uint32_t pk[N];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const Axis ay = resolve(sy, a.h, a.reflect), ax = resolve(sx, a.w, a.reflect);
        const int x = x0 + e;
        off[e] = ay.i0 * a.w + ax.i0;
        pk[e] = ax.f | (ay.f << kFy) | ((uint32_t)(ax.step + 1) << kStepX) | ((uint32_t)(ay.step + 1) << kStepY) |
                (ax.outside << kOutX) | (ay.outside << kOutY) |
                ((uint32_t)(row_erased && x >= ex0 && x < ex1) << kErased);
        sy += 2 * a01;
        sx += 2 * a11;
    }

    const size_t plane_bytes = (size_t)a.h * a.w * ELT;
    uint8_t* __restrict__ dp = a.dst + (int64_t)b * a.img_bytes + ((size_t)y * a.w + x0) * ELT;
    for (int ch = 0; ch < a.c; ++ch) {
        uint32_t q[Q];
#pragma unroll
        for (int i = 0; i < Q; ++i) q[i] = 0;
        // G pixels at a time: their 4 G loads are in flight together, then they are blended (all N at once would hold
        // 64 loaded bytes in 64 registers for a uint8 vector of 16: measured by the compiler as 256 VGPRs)
#pragma unroll
        for (int g = 0; g < N; g += G) {
            uint32_t v[G][4];
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const int e = g + k;
                // (opaque to the optimiser: it would otherwise hoist the four offsets of every pixel out of the plane
                // loop and hold them in registers - 256 VGPRs for a uint8 vector of 16 - to save three additions)
                asm volatile("" : "+v"(pk[e]));
                const int dx = (int)((pk[e] >> kStepX) & 3u) - 1;
                const int dy = ((int)((pk[e] >> kStepY) & 3u) - 1) * a.w;
                v[k][0] = load_elt<ELT>(sp, (uint32_t)off[e]);
                v[k][1] = load_elt<ELT>(sp, (uint32_t)(off[e] + dx));
                v[k][2] = load_elt<ELT>(sp, (uint32_t)(off[e] + dy));
                v[k][3] = load_elt<ELT>(sp, (uint32_t)(off[e] + dy + dx));
            }
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const int e = g + k;
                const uint32_t ox = (pk[e] >> kOutX) & 3u, oy = (pk[e] >> kOutY) & 3u;
                if (ox | oy) {  // (constant padding only)
                    if ((ox | oy) & 1u) v[k][0] = a.fill;
                    if ((ox >> 1 | oy) & 1u) v[k][1] = a.fill;
                    if ((ox | oy >> 1) & 1u) v[k][2] = a.fill;
                    if ((ox | oy) >> 1) v[k][3] = a.fill;
                }
                const uint32_t fx = pk[e] & 255u, fy = (pk[e] >> kFy) & 255u;
                uint32_t px = ELT == 1 ? blend_u8(v[k], fx, fy) : blend_f32(v[k], fx, fy);
                if ((pk[e] >> kErased) & 1u) px = a.fill;
                if constexpr (ELT == 4) q[e] = px;
                else if constexpr (V == 1) q[0] = px;
                else q[e >> 2] |= px << (8 * (e & 3));  // (set_elt without its mask: px <= 255)
            }
            if constexpr (N > G) __builtin_amdgcn_sched_barrier(0);  // (keeps the next group's loads behind this blend)
        }
        store_vec<V>(dp, q);
        sp += plane_bytes;
        dp += plane_bytes;
    }
}

}  // namespace
}  // namespace marl

using namespace marl;

extern "C" int marl_batch_warp_plan(int c, int h, int w, int elt_bytes, const void* src, const void* dst,
                                    marl_warp_plan_info* out) {
    if (out == nullptr) {
        set_error("marl_batch_warp_plan: null argument");
        return MARL_EINVAL;
    }
    GatherPlan g{};
    MARL_TRY(gather_plan("marl_batch_warp_plan", c, h, w, elt_bytes, src, dst, &g));
    *out = marl_warp_plan_info{};
    out->store_bytes = g.store_bytes;
    out->pixels_per_thread = g.store_bytes / elt_bytes;
    out->vectors_per_row = g.nv;
    out->threads = kWarpThreads;
    out->blocks_per_image = (int)cdiv((int64_t)h * g.nv, kWarpThreads);
    out->lds_bytes = 0;
    return MARL_OK;
}

extern "C" int marl_batch_warp(const void* src, int64_t n_src, void* dst, const int64_t* rows, const int32_t* mats,
                               const int32_t* ops, int batch, int c, int h, int w, int elt_bytes, int pad_mode,
                               uint32_t fill_bits, void* stream) {
    static const char* who = "marl_batch_warp";
    if (src != nullptr && dst != nullptr && mats == nullptr) {  // (behind the null src / dst answer, before the others)
        set_error("%s: null mats (a plain gather is marl_batch_augment's)", who);
        return MARL_EINVAL;
    }
    const GatherCall call{src, n_src, dst, rows, ops, batch, c, h, w, elt_bytes, pad_mode, fill_bits};
    GatherPlan g{};
    MARL_TRY(gather_guard(who, "a tap would read what another workgroup wrote", call, &g));
    WarpArgs a = gather_args<WarpArgs>(call, g);
    a.mats = mats;
    a.plane_vec = (uint32_t)((int64_t)h * g.nv);
    a.blocks_per_image = (int)cdiv(a.plane_vec, kWarpThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return gather_launch(who, call, g, a.blocks_per_image, [&](auto elt, auto v, dim3 grid) {
        batch_warp_kernel<elt, v><<<grid, kWarpThreads, 0, st>>>(a);
    });
}
