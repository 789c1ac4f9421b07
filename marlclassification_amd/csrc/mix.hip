// marl_batch_mix (include/marl_hip_mix.h): the augmenting batch gather with CutMix / Mixup fused in.  Output image b is
// view b (what marl_batch_augment writes for rows[b], ops[b]) mixed with view p = partner[b] of the same batch, the
// partner's view under its own row and ops - index remapping with two candidate sources per pixel, so CutMix moves the
// bytes a plain gather moves and Mixup reads one image more.  One kernel, no workspace, no atomics, no LDS.
//
// Work split: batch_augment_kernel's band form.  A workgroup (256 threads) owns a band of kBandVectors consecutive
// aligned stores (V bytes each) of ONE output image; rows, ops and mix of b and of p are loads at workgroup-uniform
// addresses, sanitised once (nothing read from device memory is trusted: view_of(), rule_of()).  Per store:
//   * CutMix and the unmixed part: the store's n = V / elt pixels all come from one view (the box holds all of them or
//     none), that view has no transposing code and the source pixels are consecutive in one source row - ONE load of V
//     bytes at whatever alignment the shift left, reversed in registers for a mirrored row;
//   * Mixup: two such loads and the blend in registers;
//   * everything else - box edges inside a store, image borders, erase rectangles, views with d4 & 1 - per pixel, in
//     the same pass.  (Transposing views have no LDS tile here: their reads are strided.)
// The address rules are those of augment.hip, written again: that file and its code objects are not touched.
#include "common.h"

#include "../../include/marl_hip_augment.h"
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

// one view: the source image and ops[i] as the kernel uses them - every coordinate derived below stays inside the image
struct MixView {
    const uint8_t* img;
    int d4, dy, dx, ey0, ey1, ex0, ex1;
};

// mix[b] as the kernel uses it
struct MixRule {
    int partner, mode, by0, by1, bx0, bx1, k;
};

__device__ __forceinline__ int clamp32(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clamp64(int64_t v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

__device__ __forceinline__ MixView view_of(const MixArgs& a, int i) {
    int64_t row = a.rows ? a.rows[i] : (int64_t)i;
    row = row < 0 ? 0 : (row >= a.n_src ? a.n_src - 1 : row);
    MixView v{a.src + row * a.img_bytes, 0, 0, 0, 0, 0, 0, 0};  // 64-bit: a resident set is larger than 4 GB
    if (a.ops == nullptr) return v;
    const int32_t* p = a.ops + (size_t)i * 8;
    v.d4 = p[0] & (a.h == a.w ? 7 : 6);
    v.dy = clamp32(p[1], -(a.h - 1), a.h - 1);
    v.dx = clamp32(p[2], -(a.w - 1), a.w - 1);
    v.ey0 = clamp64(p[3], 0, a.h);
    v.ey1 = clamp64((int64_t)p[3] + p[5], 0, a.h);
    v.ex0 = clamp64(p[4], 0, a.w);
    v.ex1 = clamp64((int64_t)p[4] + p[6], 0, a.w);
    return v;
}

__device__ __forceinline__ MixRule rule_of(const MixArgs& a, int b) {
    MixRule r{b, MARL_MIX_NONE, 0, 0, 0, 0, 256};
    if (a.mix == nullptr) return r;
    const int32_t* p = a.mix + (size_t)b * 8;
    r.partner = clamp32(p[0], 0, a.batch - 1);
    r.mode = p[1] & 3;
    if (r.mode == 3) r.mode = MARL_MIX_NONE;
    r.by0 = clamp64(p[2], 0, a.h);
    r.by1 = clamp64((int64_t)p[2] + p[4], 0, a.h);
    r.bx0 = clamp64(p[3], 0, a.w);
    r.bx1 = clamp64((int64_t)p[3] + p[5], 0, a.w);
    r.k = clamp32(p[6], 0, 256);
    return r;
}

// a shifted coordinate v in [-(n - 1), 2 (n - 1)] -> [0, n) (reflect) or -1 (constant padding, outside)
__device__ __forceinline__ int fold_coord(int v, int n, int reflect) {
    if (reflect) {
        v = v < 0 ? -v : v;
        return v >= n ? 2 * (n - 1) - v : v;
    }
    return (v < 0 || v >= n) ? -1 : v;
}

// one pixel of a view, every rule applied; `plane` is the pixel offset of the channel inside the image
template <int ELT>
__device__ __forceinline__ uint32_t view_pixel(const MixArgs& a, const MixView& s, int plane, int y, int x) {
    if (y >= s.ey0 && y < s.ey1 && x >= s.ex0 && x < s.ex1) return a.fill;
    int yy = fold_coord(y - s.dy, a.h, a.reflect), xx = fold_coord(x - s.dx, a.w, a.reflect);
    if ((yy | xx) < 0) return a.fill;
    if (s.d4 & 1) {
        const int t = yy;
        yy = xx;
        xx = t;
    }
    if (s.d4 & 2) xx = a.w - 1 - xx;
    if (s.d4 & 4) yy = a.h - 1 - yy;
    const int off = plane + yy * a.w + xx;  // 32-bit inside one image (img_bytes < 2^31)
    if constexpr (ELT == 1) return s.img[off];
    else return reinterpret_cast<const uint32_t*>(s.img)[off];
}

template <int V>
struct MVec {
    uint32_t q[V >= 4 ? V / 4 : 1];
};
template <int V>
struct __attribute__((packed)) MVecA1 {
    uint32_t q[V / 4];
};
template <int V>
struct __attribute__((packed, aligned(4))) MVecA4 {
    uint32_t q[V / 4];
};

// V bytes from any address (fp32: any multiple of 4)
template <int ELT, int V>
__device__ __forceinline__ MVec<V> load_any(const uint8_t* __restrict__ p) {
    MVec<V> v;
    if constexpr (V == 1) {
        v.q[0] = *p;
    } else if constexpr (ELT == 1) {
        const MVecA1<V> t = *reinterpret_cast<const MVecA1<V>*>(p);
#pragma unroll
        for (int i = 0; i < V / 4; ++i) v.q[i] = t.q[i];
    } else {
        const MVecA4<V> t = *reinterpret_cast<const MVecA4<V>*>(p);
#pragma unroll
        for (int i = 0; i < V / 4; ++i) v.q[i] = t.q[i];
    }
    return v;
}

template <int V>
__device__ __forceinline__ void store_aligned(uint8_t* __restrict__ p, const MVec<V>& v) {
    if constexpr (V == 16) *reinterpret_cast<uint4*>(p) = make_uint4(v.q[0], v.q[1], v.q[2], v.q[3]);
    else if constexpr (V == 8) *reinterpret_cast<uint2*>(p) = make_uint2(v.q[0], v.q[1]);
    else if constexpr (V == 4) *reinterpret_cast<uint32_t*>(p) = v.q[0];
    else *p = (uint8_t)v.q[0];
}

template <int ELT, int V>
__device__ __forceinline__ MVec<V> mirrored(const MVec<V>& v) {
    if constexpr (V == 1) return v;
    MVec<V> r;
#pragma unroll
    for (int i = 0; i < V / 4; ++i) {
        const uint32_t t = v.q[V / 4 - 1 - i];
        r.q[i] = ELT == 1 ? __builtin_bswap32(t) : t;
    }
    return r;
}

template <int ELT, int V>
__device__ __forceinline__ void put(MVec<V>& v, int e, uint32_t val) {  // e is a compile-time index after unrolling
    if constexpr (ELT == 4) v.q[e] = val;
    else if constexpr (V == 1) v.q[0] = val;
    else v.q[e >> 2] |= (val & 0xffu) << (8 * (e & 3));
}

// the fast form of one store from one view: true and the load issued if its pixels are consecutive in one source row
template <int ELT, int V>
__device__ __forceinline__ bool fetch(const MixArgs& a, const MixView& s, int plane, int y, int x0, MVec<V>& v) {
    constexpr int N = V / ELT;
    if (s.d4 & 1) return false;
    int yy = fold_coord(y - s.dy, a.h, a.reflect);
    const int xs0 = x0 - s.dx;
    const bool erased = y >= s.ey0 && y < s.ey1 && x0 < s.ex1 && x0 + N > s.ex0;
    if (yy < 0 || erased || xs0 < 0 || xs0 + N > a.w) return false;
    if (s.d4 & 4) yy = a.h - 1 - yy;
    const int start = (s.d4 & 2) ? a.w - (xs0 + N) : xs0;
    v = load_any<ELT, V>(s.img + (size_t)(plane + yy * a.w + start) * ELT);
    return true;
}

// ... and what follows once the loads are under way: the mirror, or the pixels one by one
template <int ELT, int V>
__device__ __forceinline__ void settle(const MixArgs& a, const MixView& s, int plane, int y, int x0, bool fast,
                                       MVec<V>& v) {
    constexpr int N = V / ELT;
    if (fast) {
        if (s.d4 & 2) v = mirrored<ELT, V>(v);
        return;
    }
#pragma unroll
    for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) v.q[i] = 0;
#pragma unroll
    for (int e = 0; e < N; ++e) put<ELT, V>(v, e, view_pixel<ELT>(a, s, plane, y, x0 + e));
}

// Mixup of two stores' worth of pixels; k in [0, 256]
template <int ELT, int V>
__device__ __forceinline__ MVec<V> blend(const MVec<V>& vb, const MVec<V>& vp, int k) {
    // (the fp32 blend is two rounded products and a rounded sum, __fadd_rn(__fmul_rn(..), __fmul_rn(..)) - written with
    // the operators under contract(off): the intrinsics are inline functions of a header compiled under the default
    // contraction, and their * and + were fused into an FMA once inlined here)
#pragma clang fp contract(off)
    MVec<V> r;
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

__device__ __forceinline__ MixView pick(bool second, const MixView& vb, const MixView& vp) {
    MixView s;
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
    const MixView vb = view_of(a, b);
    const MixView vp = view_of(a, m.partner);
    uint8_t* __restrict__ dimg = a.dst + (int64_t)b * a.img_bytes;
    const bool mixup = m.mode == MARL_MIX_MIXUP, cutmix = m.mode == MARL_MIX_CUTMIX;

    const uint32_t base = (uint32_t)t * kMixBandVectors + threadIdx.x;
    MVec<V> v[NPT], v2[NPT];
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
                put<ELT, V>(v[k], e, view_pixel<ELT>(a, pick(inside, vb, vp), plane[k], ys[k], x));
            }
        }
        store_aligned<V>(dimg + (size_t)(plane[k] + ys[k] * a.w + x0s[k]) * ELT, v[k]);
    }
}

struct MixPlan {
    int store_bytes, nv, blocks_per_image;
    uint32_t total_vec;
};

int mix_plan(const char* who, int c, int h, int w, int elt, const void* src, const void* dst, MixPlan* p) {
    if (elt != 1 && elt != 4) {
        set_error("%s: elt_bytes %d is neither 1 nor 4", who, elt);
        return MARL_EINVAL;
    }
    if (c <= 0 || h <= 0 || w <= 0) {
        set_error("%s: sizes must be positive (c %d, h %d, w %d)", who, c, h, w);
        return MARL_EINVAL;
    }
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (elt == 4 && ((s | d) & 3)) {
        set_error("%s: 4-byte elements need 4-byte aligned src and dst", who);
        return MARL_EINVAL;
    }
    const int64_t img_bytes = (int64_t)c * h * w * elt;
    if (img_bytes >= (int64_t)1 << 31) {
        set_error("%s: an image of %lld bytes (c %d, h %d, w %d) is beyond 2^31", who, (long long)img_bytes, c, h, w);
        return MARL_ELIMIT;
    }
    const int64_t row_bytes = (int64_t)w * elt;
    int v = 16;
    while (v > elt && ((row_bytes % v) != 0 || (d % v) != 0)) v >>= 1;
    if (v < 4) v = elt;  // (uint8 rows that are no multiple of 4 bytes: byte stores)
    p->store_bytes = v;
    p->nv = (int)(row_bytes / v);
    p->total_vec = (uint32_t)((int64_t)c * h * p->nv);
    p->blocks_per_image = (int)cdiv(p->total_vec, kMixBandVectors);
    return MARL_OK;
}

template <int ELT>
int launch_mix(const MixArgs& a, int v, int64_t blocks, hipStream_t st) {
    const dim3 grid((unsigned)blocks), block(kMixThreads);
    switch (v) {
        case 16: batch_mix_kernel<ELT, 16><<<grid, block, 0, st>>>(a); break;
        case 8: batch_mix_kernel<ELT, 8><<<grid, block, 0, st>>>(a); break;
        case 4: batch_mix_kernel<ELT, 4><<<grid, block, 0, st>>>(a); break;
        default:
            if constexpr (ELT == 1) batch_mix_kernel<1, 1><<<grid, block, 0, st>>>(a);
            break;
    }
    MARL_LAUNCH_CHECK();
    return MARL_OK;
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
    MixPlan p{};
    MARL_TRY(mix_plan("marl_batch_mix_plan", c, h, w, elt_bytes, src, dst, &p));
    *out = marl_mix_plan_info{};
    out->store_bytes = p.store_bytes;
    out->band_vectors = kMixBandVectors;
    out->blocks_per_image = p.blocks_per_image;
    out->lds_bytes = 0;
    return MARL_OK;
}

extern "C" int marl_batch_mix(const void* src, int64_t n_src, void* dst, const int64_t* rows, const int32_t* ops,
                              const int32_t* mix, int batch, int c, int h, int w, int elt_bytes, int pad_mode,
                              uint32_t fill_bits, void* stream) {
    static const char* who = "marl_batch_mix";
    if (src == nullptr || dst == nullptr) {
        set_error("%s: null src / dst", who);
        return MARL_EINVAL;
    }
    if (pad_mode != MARL_AUGMENT_PAD_ZERO && pad_mode != MARL_AUGMENT_PAD_REFLECT) {
        set_error("%s: unknown pad_mode %d", who, pad_mode);
        return MARL_EINVAL;
    }
    if (batch <= 0 || n_src <= 0) {
        set_error("%s: sizes must be positive (batch %d, n_src %lld)", who, batch, (long long)n_src);
        return MARL_EINVAL;
    }
    MixPlan p{};
    MARL_TRY(mix_plan(who, c, h, w, elt_bytes, src, dst, &p));
    if (rows == nullptr && n_src < batch) {
        set_error("%s: rows == NULL takes row b for image b, but n_src %lld < batch %d", who, (long long)n_src, batch);
        return MARL_EINVAL;
    }
    const int64_t img_bytes = (int64_t)c * h * w * elt_bytes;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    if (n_src > (INT64_MAX / 2) / img_bytes) {
        set_error("%s: n_src %lld images of %lld bytes overflow", who, (long long)n_src, (long long)img_bytes);
        return MARL_ELIMIT;
    }
    const uintptr_t s1 = s0 + (uintptr_t)(n_src * img_bytes), d1 = d0 + (uintptr_t)((int64_t)batch * img_bytes);
    if (d0 < s1 && s0 < d1) {
        set_error("%s: dst overlaps src (in place is undefined for flips)", who);
        return MARL_EINVAL;
    }
    const int64_t blocks = (int64_t)batch * p.blocks_per_image;
    if (blocks > 0x7fffffffLL) {
        set_error("%s: %lld workgroups (batch %d) are more than a grid holds", who, (long long)blocks, batch);
        return MARL_ELIMIT;
    }
    MixArgs a{};
    a.src = static_cast<const uint8_t*>(src);
    a.dst = static_cast<uint8_t*>(dst);
    a.rows = rows;
    a.ops = ops;
    a.mix = mix;
    a.n_src = n_src;
    a.img_bytes = img_bytes;
    a.batch = batch;
    a.c = c, a.h = h, a.w = w;
    a.nv = p.nv;
    a.total_vec = p.total_vec;
    a.blocks_per_image = p.blocks_per_image;
    a.reflect = pad_mode == MARL_AUGMENT_PAD_REFLECT;
    a.fill = elt_bytes == 1 ? (fill_bits & 0xffu) : fill_bits;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return elt_bytes == 1 ? launch_mix<1>(a, p.store_bytes, blocks, st) : launch_mix<4>(a, p.store_bytes, blocks, st);
}
