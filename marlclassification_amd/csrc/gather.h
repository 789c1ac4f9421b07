// What the batch gathers share (augment.hip, mix.hip, warp.hip; internal).  Device side: the address rules that
// include/marl_hip_augment.h documents - one sanitiser of rows[i] / ops[i] into a View, one fold, one per-pixel rule,
// one family of store vectors.  Host side: the checks of the three plan queries, the guards of the three entries in their
// one order, the fields every argument struct has, the switch over the store widths; the guards are one function a rule
// (need_*), and the store-width rule is store_width, which normalize.hip and color.hip use too.  What differs per kernel
// (total_vec against plane_vec, the band size, the transposing tiles, the mix rule, the matrices) stays in its file.
//
// The device functions are templated on the kernel's argument struct (AugArgs, MixArgs, WarpArgs), which keeps its own
// layout; they read src, rows, ops, n_src, img_bytes, h, w, reflect and fill from it.  Every kernel compiles to the
// bytes it had when each file carried its own copy (tools/gather_identity.py), which is why three spellings look less
// shared than they could be: the row clamp is written out inside view_of, augment reads its row after the ops
// (view_of<false>), and warp reads its rectangle itself.  The folded forms change register numbers or the order of the
// first blocks.
#pragma once

#include <type_traits>

#include "common.h"

#include "../../include/marl_hip_augment.h"

namespace marl {
namespace {

// ---- device: nothing read from device memory is trusted -------------------------------------------------------------
// one view: the source image and ops[i] as the kernels use them - every coordinate derived below stays inside the image
struct View {
    const uint8_t* img;
    int d4, dy, dx, ey0, ey1, ex0, ex1;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clampl(int64_t v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// A source row -> [0, n_src), for a kernel that reads its row itself: `rows ? rows[i] : i` (rows == NULL takes row i
// for image i), clamped, times img_bytes in 64 bits (a resident set is larger than 4 GB).
__device__ __forceinline__ int64_t clamp_row(int64_t row, int64_t n_src) {
    return row < 0 ? 0 : (row >= n_src ? n_src - 1 : row);
}

// View i: rows[i] and ops[i] as the kernels use them, loads at a workgroup-uniform address, made once.  WITH_IMAGE =
// false leaves img null and the row to the caller (clamp_row).
template <bool WITH_IMAGE = true, class Args>
__device__ __forceinline__ View view_of(const Args& a, int i) {
    const uint8_t* img = nullptr;
    if constexpr (WITH_IMAGE) {
        int64_t row = a.rows ? a.rows[i] : (int64_t)i;
        row = row < 0 ? 0 : (row >= a.n_src ? a.n_src - 1 : row);  // (clamp_row, written out)
        img = a.src + row * a.img_bytes;
    }
    View v{img, 0, 0, 0, 0, 0, 0, 0};
    if (a.ops == nullptr) return v;
    const int32_t* p = a.ops + (size_t)i * 8;
    v.d4 = p[0] & (a.h == a.w ? 7 : 6);
    v.dy = clampi(p[1], -(a.h - 1), a.h - 1);
    v.dx = clampi(p[2], -(a.w - 1), a.w - 1);
    v.ey0 = clampl(p[3], 0, a.h);
    v.ey1 = clampl((int64_t)p[3] + p[5], 0, a.h);
    v.ex0 = clampl(p[4], 0, a.w);
    v.ex1 = clampl((int64_t)p[4] + p[6], 0, a.w);
    return v;
}

// a shifted coordinate v in [-(n - 1), 2 (n - 1)] -> [0, n) (reflect) or -1 (constant padding, outside)
__device__ __forceinline__ int fold(int v, int n, int reflect) {
    if (reflect) {
        v = v < 0 ? -v : v;
        return v >= n ? 2 * (n - 1) - v : v;
    }
    return (v < 0 || v >= n) ? -1 : v;
}

// element `off` of an image or plane; 32-bit inside one image (img_bytes < 2^31)
template <int ELT, class Off>
__device__ __forceinline__ uint32_t load_elt(const uint8_t* img, Off off) {
    if constexpr (ELT == 1) return img[off];
    else return reinterpret_cast<const uint32_t*>(img)[off];
}

// one pixel of a view, every rule applied; `plane` is the pixel offset of the channel inside the image
template <int ELT, class Args>
__device__ __forceinline__ uint32_t pixel(const Args& a, const View& s, int plane, int y, int x) {
    if (y >= s.ey0 && y < s.ey1 && x >= s.ex0 && x < s.ex1) return a.fill;
    int yy = fold(y - s.dy, a.h, a.reflect), xx = fold(x - s.dx, a.w, a.reflect);
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

// V bytes of one store: V / ELT pixels
template <int V>
struct Vec {
    uint32_t q[V >= 4 ? V / 4 : 1];
};
template <int V>
struct __attribute__((packed)) VecA1 {
    uint32_t q[V / 4];
};
template <int V>
struct __attribute__((packed, aligned(4))) VecA4 {
    uint32_t q[V / 4];
};

// V bytes from any address (fp32: any multiple of 4)
template <int ELT, int V>
__device__ __forceinline__ Vec<V> load_vec(const uint8_t* __restrict__ p) {
    Vec<V> v;
    if constexpr (V == 1) {
        v.q[0] = *p;
    } else if constexpr (ELT == 1) {
        const VecA1<V> t = *reinterpret_cast<const VecA1<V>*>(p);
#pragma unroll
        for (int i = 0; i < V / 4; ++i) v.q[i] = t.q[i];
    } else {
        const VecA4<V> t = *reinterpret_cast<const VecA4<V>*>(p);
#pragma unroll
        for (int i = 0; i < V / 4; ++i) v.q[i] = t.q[i];
    }
    return v;
}

// V bytes to a V-aligned address
template <int V>
__device__ __forceinline__ void store_vec(uint8_t* __restrict__ p, const uint32_t* q) {
    if constexpr (V == 16) *reinterpret_cast<uint4*>(p) = make_uint4(q[0], q[1], q[2], q[3]);
    else if constexpr (V == 8) *reinterpret_cast<uint2*>(p) = make_uint2(q[0], q[1]);
    else if constexpr (V == 4) *reinterpret_cast<uint32_t*>(p) = q[0];
    else *p = (uint8_t)q[0];
}

// pixel order reversed (a mirrored row)
template <int ELT, int V>
__device__ __forceinline__ Vec<V> reversed(const Vec<V>& v) {
    if constexpr (V == 1) return v;
    Vec<V> r;
#pragma unroll
    for (int i = 0; i < V / 4; ++i) {
        const uint32_t t = v.q[V / 4 - 1 - i];
        r.q[i] = ELT == 1 ? __builtin_bswap32(t) : t;
    }
    return r;
}

// pixel k of a zeroed vector
template <int ELT, int V>
__device__ __forceinline__ void set_elt(Vec<V>& v, int k, uint32_t val) {  // k is a compile-time index after unrolling
    if constexpr (ELT == 4) v.q[k] = val;
    else if constexpr (V == 1) v.q[0] = val;
    else v.q[k >> 2] |= (val & 0xffu) << (8 * (k & 3));
}

// ---- host: the plan, the guards, the launch -------------------------------------------------------------------------
// the arguments every entry takes
struct GatherCall {
    const void* src;
    int64_t n_src;
    void* dst;
    const int64_t* rows;
    const int32_t* ops;
    int batch, c, h, w, elt, pad_mode;
    uint32_t fill_bits;
};

struct GatherPlan {
    int store_bytes, nv;  // V, and stores per output row
};

// The store width: the widest of 16 / 8 / 4 bytes that divides `bytes` (a row, a plane) and `addrs` (the OR of every
// address a vector touches), the element for uint8 lengths that are no multiple of 4 bytes.
inline int store_width(int64_t bytes, uintptr_t addrs, int elt) {
    int v = 16;
    while (v > elt && ((bytes % v) != 0 || (addrs % v) != 0)) v >>= 1;
    return v < 4 ? elt : v;  // (uint8 rows that are no multiple of 4 bytes: byte stores)
}

// The checks of the three plan queries, and the store width of a row at dst's address.
inline int gather_plan(const char* who, int c, int h, int w, int elt, const void* src, const void* dst, GatherPlan* p) {
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
    p->store_bytes = store_width(row_bytes, d, elt);
    p->nv = (int)(row_bytes / p->store_bytes);
    return MARL_OK;
}

// The guards every batch entry has (the gathers here; normalize.hip, color.hip), one rule each: an entry is a sequence
// of them in its own order, which is part of its contract (tools/gather_identity.py).  Host arithmetic: nothing is
// dereferenced.
inline int need_batch(const char* who, int batch, int64_t n_src) {
    if (batch <= 0 || n_src <= 0) {
        set_error("%s: sizes must be positive (batch %d, n_src %lld)", who, batch, (long long)n_src);
        return MARL_EINVAL;
    }
    return MARL_OK;
}

inline int need_rows_cover(const char* who, const int64_t* rows, int64_t n_src, int batch) {
    if (rows == nullptr && n_src < batch) {
        set_error("%s: rows == NULL takes row b for image b, but n_src %lld < batch %d", who, (long long)n_src, batch);
        return MARL_EINVAL;
    }
    return MARL_OK;
}

// n_src * img_bytes stays a byte count the overlap test can add to an address
inline int need_extent(const char* who, int64_t n_src, int64_t img_bytes) {
    if (n_src > (INT64_MAX / 2) / img_bytes) {
        set_error("%s: n_src %lld images of %lld bytes overflow", who, (long long)n_src, (long long)img_bytes);
        return MARL_ELIMIT;
    }
    return MARL_OK;
}

// [src, src + src_bytes) and [dst, dst + dst_bytes) share no byte (adjacent is apart); `in_place` is why that entry
// refuses dst inside src
inline int need_apart(const char* who, const void* src, int64_t src_bytes, const void* dst, int64_t dst_bytes,
                      const char* in_place) {
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t s1 = s0 + (uintptr_t)src_bytes, d1 = d0 + (uintptr_t)dst_bytes;
    if (d0 < s1 && s0 < d1) {
        set_error("%s: dst overlaps src (%s)", who, in_place);
        return MARL_EINVAL;
    }
    return MARL_OK;
}

inline int need_grid(const char* who, int64_t blocks, int batch) {
    if (blocks > 0x7fffffffLL) {
        set_error("%s: %lld workgroups (batch %d) are more than a grid holds", who, (long long)blocks, batch);
        return MARL_ELIMIT;
    }
    return MARL_OK;
}

// `what` (one or two pointers, null allowed) on a multiple of `to` bytes
inline int need_aligned(const char* who, const char* what, int to, const void* p, const void* q = nullptr) {
    if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & (uintptr_t)(to - 1)) {
        set_error("%s: %s must be %d-byte aligned", who, what, to);
        return MARL_EINVAL;
    }
    return MARL_OK;
}

// The guards of a gather entry up to the grid size (gather_launch's), in the order the entries have always answered.
inline int gather_guard(const char* who, const char* in_place, const GatherCall& g, GatherPlan* p) {
    if (g.src == nullptr || g.dst == nullptr) {
        set_error("%s: null src / dst", who);
        return MARL_EINVAL;
    }
    if (g.pad_mode != MARL_AUGMENT_PAD_ZERO && g.pad_mode != MARL_AUGMENT_PAD_REFLECT) {
        set_error("%s: unknown pad_mode %d", who, g.pad_mode);
        return MARL_EINVAL;
    }
    MARL_TRY(need_batch(who, g.batch, g.n_src));
    MARL_TRY(gather_plan(who, g.c, g.h, g.w, g.elt, g.src, g.dst, p));
    MARL_TRY(need_rows_cover(who, g.rows, g.n_src, g.batch));
    const int64_t img_bytes = (int64_t)g.c * g.h * g.w * g.elt;
    MARL_TRY(need_extent(who, g.n_src, img_bytes));
    return need_apart(who, g.src, g.n_src * img_bytes, g.dst, (int64_t)g.batch * img_bytes, in_place);
}

// the fields every argument struct has
template <class Args>
Args gather_args(const GatherCall& g, const GatherPlan& p) {
    Args a{};
    a.src = static_cast<const uint8_t*>(g.src);
    a.dst = static_cast<uint8_t*>(g.dst);
    a.rows = g.rows;
    a.ops = g.ops;
    a.n_src = g.n_src;
    a.img_bytes = (int64_t)g.c * g.h * g.w * g.elt;
    a.c = g.c, a.h = g.h, a.w = g.w;
    a.nv = p.nv;
    a.reflect = g.pad_mode == MARL_AUGMENT_PAD_REFLECT;
    a.fill = g.elt == 1 ? (g.fill_bits & 0xffu) : g.fill_bits;
    return a;
}

// The last guard and the launch: launch(elt, v, grid) starts kernel<elt, v> - the seven (ELT, V) a plan can name, two
// compile-time integers - on batch * blocks_per_image workgroups.
template <class Launch>
int gather_launch(const char* who, const GatherCall& g, const GatherPlan& p, int blocks_per_image, Launch&& launch) {
    const int64_t blocks = (int64_t)g.batch * blocks_per_image;
    MARL_TRY(need_grid(who, blocks, g.batch));
    const dim3 grid((unsigned)blocks);
    using E1 = std::integral_constant<int, 1>;
    using E4 = std::integral_constant<int, 4>;
    if (g.elt == 1) {
        switch (p.store_bytes) {
            case 16: launch(E1{}, std::integral_constant<int, 16>{}, grid); break;
            case 8: launch(E1{}, std::integral_constant<int, 8>{}, grid); break;
            case 4: launch(E1{}, std::integral_constant<int, 4>{}, grid); break;
            default: launch(E1{}, std::integral_constant<int, 1>{}, grid); break;
        }
    } else {
        switch (p.store_bytes) {
            case 16: launch(E4{}, std::integral_constant<int, 16>{}, grid); break;
            case 8: launch(E4{}, std::integral_constant<int, 8>{}, grid); break;
            default: launch(E4{}, std::integral_constant<int, 4>{}, grid); break;
        }
    }
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}

}  // namespace
}  // namespace marl
