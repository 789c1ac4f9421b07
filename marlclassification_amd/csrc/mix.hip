// marl_batch_mix (include/marl_hip_mix.h): the augmenting batch gather with CutMix / Mixup fused in.  Output image b is
// view b (what marl_batch_augment writes for rows[b], ops[b]) mixed with view p = partner[b] of the same batch, the
// partner's view under its own row and ops - index remapping with two candidate sources per pixel, so CutMix moves the
// bytes a plain gather moves and Mixup reads one image more.  One kernel, no workspace, no atomics, no LDS.
//
// Work split: batch_augment_kernel's band form.  A workgroup (256 threads) owns a band of kBandVectors consecutive
// aligned stores (V bytes each) of ONE output image; rows, ops and mix of b and of p are loads at workgroup-uniform
// addresses, sanitised once (nothing read from device memory is trusted: gather.h's view_of(), rule_of()).  Per store:
//   * CutMix and the unmixed part: the store's n = V / elt pixels all come from one view (the box holds all of them or
//     none), that view has no transposing code and the source pixels are consecutive in one source row - ONE load of V
//     bytes at whatever alignment the shift left, reversed in registers for a mirrored row;
//   * Mixup: two such loads and the blend in registers;
//   * everything else - box edges inside a store, image borders, erase rectangles, views with d4 & 1 - per pixel, in
//     the same pass.  (Transposing views have no LDS tile here: their reads are strided.)
// The address rules are those of augment.hip: both take them from gather.h.
#include "gather.h"

#include "../../include/marl_hip_mix.h"

namespace marl {
namespace {

constexpr int kMixThreads = 256;
constexpr int kMixStoresPerThread = 4;
constexpr int kMixBandVectors = kMixStoresPerThread * kMixThreads;

struct MixArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int64_t* rows;
    const int32_t* ops;
    const int32_t* mix;
    int64_t n_src;
    int64_t img_bytes;
    int batch, c, h, w;
    int nv;               // stores per output row
    uint32_t total_vec;   // c * h * nv
    int blocks_per_image;
    int reflect;
    uint32_t fill;
};

// mix[b] as the kernel uses it
struct MixRule {
    int partner, mode, by0, by1, bx0, bx1, k;
};

__device__ __forceinline__ MixRule rule_of(const MixArgs& a, int b) {
    MixRule r{b, MARL_MIX_NONE, 0, 0, 0, 0, 256};
    if (a.mix == nullptr) return r;
    const int32_t* p = a.mix + (size_t)b * 8;
    r.partner = clampi(p[0], 0, a.batch - 1);
    r.mode = p[1] & 3;
    if (r.mode == 3) r.mode = MARL_MIX_NONE;
    r.by0 = clampl(p[2], 0, a.h);
    r.by1 = clampl((int64_t)p[2] + p[4], 0, a.h);
    r.bx0 = clampl(p[3], 0, a.w);
    r.bx1 = clampl((int64_t)p[3] + p[5], 0, a.w);
    r.k = clampi(p[6], 0, 256);
    return r;
}

// the fast form of one store from one view: true and the load issued if its pixels are consecutive in one source row
template <int ELT, int V>
__device__ __forceinline__ bool fetch(const MixArgs& a, const View& s, int plane, int y, int x0, Vec<V>& v) {
    constexpr int N = V / ELT;
    if (s.d4 & 1) return false;
    int yy = fold(y - s.dy, a.h, a.reflect);
    const int xs0 = x0 - s.dx;
    const bool erased = y >= s.ey0 && y < s.ey1 && x0 < s.ex1 && x0 + N > s.ex0;
    if (yy < 0 || erased || xs0 < 0 || xs0 + N > a.w) return false;
    if (s.d4 & 4) yy = a.h - 1 - yy;
    const int start = (s.d4 & 2) ? a.w - (xs0 + N) : xs0;
    v = load_vec<ELT, V>(s.img + (size_t)(plane + yy * a.w + start) * ELT);
    return true;
}

// ... and what follows once the loads are under way: the mirror, or the pixels one by one
template <int ELT, int V>
__device__ __forceinline__ void settle(const MixArgs& a, const View& s, int plane, int y, int x0, bool fast,
                                       Vec<V>& v) {
    constexpr int N = V / ELT;
    if (fast) {
        if (s.d4 & 2) v = reversed<ELT, V>(v);
        return;
    }
#pragma unroll
    for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) v.q[i] = 0;
#pragma unroll
    for (int e = 0; e < N; ++e) set_elt<ELT, V>(v, e, pixel<ELT>(a, s, plane, y, x0 + e));
}

// Mixup of two stores' worth of pixels; k in [0, 256]
template <int ELT, int V>
__device__ __forceinline__ Vec<V> blend(const Vec<V>& vb, const Vec<V>& vp, int k) {
    // (the fp32 blend is two rounded products and a rounded sum, __fadd_rn(__fmul_rn(..), __fmul_rn(..)) - written with
    // the operators under contract(off): the intrinsics are inline functions of a header compiled under the default
    // contraction, and their * and + were fused into an FMA once inlined here)
#pragma clang fp contract(off)
    Vec<V> r;
    if constexpr (ELT == 1) {
        const uint32_t kb = (uint32_t)k, kp = (uint32_t)(256 - k);
#pragma unroll
        for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) {
            uint32_t o = 0;
#pragma unroll
            for (int j = 0; j < (V >= 4 ? 4 : 1); ++j) {
                const uint32_t x = (vb.q[i] >> (8 * j)) & 0xffu, z = (vp.q[i] >> (8 * j)) & 0xffu;
                o |= ((kb * x + kp * z + 128u) >> 8) << (8 * j);  // <= (256 * 255 + 128) >> 8 = 255
            }
            r.q[i] = o;
        }
    } else {
        const float fb = (float)k / 256.f, fp = (float)(256 - k) / 256.f;  // exact
#pragma unroll
        for (int i = 0; i < V / 4; ++i) {
            const float own = fb * __uint_as_float(vb.q[i]), other = fp * __uint_as_float(vp.q[i]);
            r.q[i] = __float_as_uint(own + other);
        }
    }
    return r;
}

__device__ __forceinline__ View pick(bool second, const View& vb, const View& vp) {
    View s;
    s.img = second ? vp.img : vb.img;
    s.d4 = second ? vp.d4 : vb.d4;
    s.dy = second ? vp.dy : vb.dy;
    s.dx = second ? vp.dx : vb.dx;
    s.ey0 = second ? vp.ey0 : vb.ey0;
    s.ey1 = second ? vp.ey1 : vb.ey1;
    s.ex0 = second ? vp.ex0 : vb.ex0;
    s.ex1 = second ? vp.ex1 : vb.ex1;
    return s;
}

template <int ELT, int V>
__global__ void __launch_bounds__(kMixThreads) batch_mix_kernel(const MixArgs a) {
    constexpr int N = V / ELT;
    constexpr int NPT = kMixStoresPerThread;
    enum { FROM_B = 0, FROM_P = 1, STRADDLE = 2 };
    const int b = blockIdx.x / a.blocks_per_image;
    const int t = blockIdx.x - b * a.blocks_per_image;
    if ((uint32_t)t * kMixBandVectors >= a.total_vec) return;
    const MixRule m = rule_of(a, b);
    const View vb = view_of(a, b);
    const View vp = view_of(a, m.partner);
    uint8_t* __restrict__ dimg = a.dst + (int64_t)b * a.img_bytes;
    const bool mixup = m.mode == MARL_MIX_MIXUP, cutmix = m.mode == MARL_MIX_CUTMIX;

    const uint32_t base = (uint32_t)t * kMixBandVectors + threadIdx.x;
    Vec<V> v[NPT], v2[NPT];
    int ys[NPT], x0s[NPT], plane[NPT], from[NPT];
    bool fast[NPT], fast2[NPT];
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const uint32_t idx = base + (uint32_t)k * kMixThreads;
        fast[k] = fast2[k] = false;
        from[k] = FROM_B;
        ys[k] = -1;
        if (idx >= a.total_vec) continue;
        const uint32_t r = idx / (uint32_t)a.nv;
        const int x0 = (int)(idx - r * (uint32_t)a.nv) * N;
        const uint32_t ch = r / (uint32_t)a.h;
        const int y = (int)(r - ch * (uint32_t)a.h);
        ys[k] = y;
        x0s[k] = x0;
        plane[k] = (int)ch * a.h * a.w;
        if (mixup) {
            fast[k] = fetch<ELT, V>(a, vb, plane[k], y, x0, v[k]);
            fast2[k] = fetch<ELT, V>(a, vp, plane[k], y, x0, v2[k]);
        } else {
            if (cutmix && y >= m.by0 && y < m.by1) {
                const int lo = max(x0, m.bx0), hi = min(x0 + N, m.bx1);  // the store's pixels inside the box
                if (hi > lo) from[k] = (lo == x0 && hi == x0 + N) ? FROM_P : STRADDLE;
            }
            if (from[k] != STRADDLE) fast[k] = fetch<ELT, V>(a, pick(from[k] == FROM_P, vb, vp), plane[k], y, x0, v[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        if (ys[k] < 0) continue;
        if (mixup) {
            settle<ELT, V>(a, vb, plane[k], ys[k], x0s[k], fast[k], v[k]);
            settle<ELT, V>(a, vp, plane[k], ys[k], x0s[k], fast2[k], v2[k]);
            v[k] = blend<ELT, V>(v[k], v2[k], m.k);
        } else if (from[k] != STRADDLE) {
            settle<ELT, V>(a, pick(from[k] == FROM_P, vb, vp), plane[k], ys[k], x0s[k], fast[k], v[k]);
        } else {
#pragma unroll
            for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) v[k].q[i] = 0;
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const int x = x0s[k] + e;
                const bool inside = x >= m.bx0 && x < m.bx1;  // (the row is inside: from[k] says so)
                set_elt<ELT, V>(v[k], e, pixel<ELT>(a, pick(inside, vb, vp), plane[k], ys[k], x));
            }
        }
        store_vec<V>(dimg + (size_t)(plane[k] + ys[k] * a.w + x0s[k]) * ELT, v[k].q);
    }
}

}  // namespace
}  // namespace marl

using namespace marl;

extern "C" int marl_batch_mix_plan(int c, int h, int w, int elt_bytes, const void* src, const void* dst,
                                   marl_mix_plan_info* out) {
    if (out == nullptr) {
        set_error("marl_batch_mix_plan: null argument");
        return MARL_EINVAL;
    }
    GatherPlan g{};
    MARL_TRY(gather_plan("marl_batch_mix_plan", c, h, w, elt_bytes, src, dst, &g));
    *out = marl_mix_plan_info{};
    out->store_bytes = g.store_bytes;
    out->band_vectors = kMixBandVectors;
    out->blocks_per_image = (int)cdiv((int64_t)c * h * g.nv, kMixBandVectors);
    out->lds_bytes = 0;
    return MARL_OK;
}

extern "C" int marl_batch_mix(const void* src, int64_t n_src, void* dst, const int64_t* rows, const int32_t* ops,
                              const int32_t* mix, int batch, int c, int h, int w, int elt_bytes, int pad_mode,
                              uint32_t fill_bits, void* stream) {
    static const char* who = "marl_batch_mix";
    const GatherCall call{src, n_src, dst, rows, ops, batch, c, h, w, elt_bytes, pad_mode, fill_bits};
    GatherPlan g{};
    MARL_TRY(gather_guard(who, "in place is undefined for flips", call, &g));
    MixArgs a = gather_args<MixArgs>(call, g);
    a.mix = mix;
    a.batch = batch;
    a.total_vec = (uint32_t)((int64_t)c * h * g.nv);
    a.blocks_per_image = (int)cdiv(a.total_vec, kMixBandVectors);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return gather_launch(who, call, g, a.blocks_per_image, [&](auto elt, auto v, dim3 grid) {
        batch_mix_kernel<elt, v><<<grid, kMixThreads, 0, st>>>(a);
    });
}
