// marl_batch_augment (include/marl_hip_augment.h): the batch gather of the resident image set with the augmentation
// fused in - a dihedral code, an integer shift with reflect / constant padding and one erased rectangle per output
// image, all of it index remapping, so the launch moves the bytes a plain index_select moves (read each selected
// image once, write it once).  One kernel, no workspace, no atomics.
//
// Work split.  A workgroup (256 threads) owns a piece of ONE output image; rows[b] and ops[b] are loads at a
// workgroup-uniform address, sanitised once (nothing read from device memory is trusted: see sanitise()).
//   * codes without bit 0 (identity, flips, half turn): the image's stores, V bytes each, are numbered row-major
//     over its c * h rows, and a workgroup takes a band of kBandVectors consecutive ones - output rows are contiguous in
//     memory, so every wave stores 64 * V consecutive, V-aligned bytes whatever w is.  A vector whose n = V / elt source
//     pixels are consecutive in one source row (no fold of the reflection inside it, no rectangle over it) is ONE load
//     of V bytes at whatever alignment the shift left, reversed in registers for a mirrored row; the others (image
//     borders, rectangle edges) are resolved per pixel.
//   * codes with bit 0 (transpose, quarter turns; square images only) go through an LDS tile of TS x TS pixels held
//     in OUTPUT layout: lanes run along the output's y, which is the source's x, so the global reads are row
//     contiguous; each pixel is written to lds[y][x] (row pitch odd in dwords: the strided writes hit distinct
//     banks), and after a barrier the tile is stored like the bands, V aligned bytes per lane along x.  uint8 tiles read
//     dwords (four output rows at once) and transpose 4 x 4 blocks in registers: load_tile_quads.
#include "common.h"

#include "../../include/marl_hip_augment.h"

namespace marl {
namespace {

constexpr int kAugThreads = 256;
#ifndef MARL_AUG_STORES_PER_THREAD
#define MARL_AUG_STORES_PER_THREAD 4
#endif
constexpr int kBandVectors = MARL_AUG_STORES_PER_THREAD * kAugThreads;
constexpr int kAugLdsBytes = 128 * 132;        // uint8: 128 rows of 128 + 4 bytes; fp32: 64 rows of 64 + 1 dwords

struct AugArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int64_t* rows;
    const int32_t* ops;
    int64_t n_src;
    int64_t img_bytes;
    int c, h, w;
    int nv;               // stores per output row
    uint32_t total_vec;   // c * h * nv
    int blocks_per_image;
    int tiles_y, tiles_x;  // of the transposing path
    int reflect;
    uint32_t fill;
};

struct AugOp {
    int d4, dy, dx, ey0, ey1, ex0, ex1;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clampl(int64_t v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// ops[b] as the kernel uses it: whatever the eight values are, every coordinate derived below stays inside the image
__device__ __forceinline__ AugOp sanitise(const int32_t* __restrict__ ops, int b, int h, int w) {
    AugOp o{0, 0, 0, 0, 0, 0, 0};
    if (ops == nullptr) return o;
    const int32_t* p = ops + (size_t)b * 8;
    o.d4 = p[0] & (h == w ? 7 : 6);
    o.dy = clampi(p[1], -(h - 1), h - 1);
    o.dx = clampi(p[2], -(w - 1), w - 1);
    o.ey0 = clampl(p[3], 0, h);
    o.ey1 = clampl((int64_t)p[3] + p[5], 0, h);
    o.ex0 = clampl(p[4], 0, w);
    o.ex1 = clampl((int64_t)p[4] + p[6], 0, w);
    return o;
}

// a shifted coordinate v in [-(n - 1), 2 (n - 1)] -> [0, n) (reflect) or -1 (constant padding, outside)
__device__ __forceinline__ int fold(int v, int n, int reflect) {
    if (reflect) {
        v = v < 0 ? -v : v;
        return v >= n ? 2 * (n - 1) - v : v;
    }
    return (v < 0 || v >= n) ? -1 : v;
}

template <int ELT>
__device__ __forceinline__ uint32_t load_elt(const uint8_t* __restrict__ img, int off) {
    if constexpr (ELT == 1) return img[off];
    else return reinterpret_cast<const uint32_t*>(img)[off];
}

// one output pixel, every rule applied (the per-pixel path of both forms); img is the source image's plane `ch`
template <int ELT>
__device__ __forceinline__ uint32_t pixel(const uint8_t* __restrict__ img, const AugOp& o, const AugArgs& a, int y,
                                          int x) {
    if (y >= o.ey0 && y < o.ey1 && x >= o.ex0 && x < o.ex1) return a.fill;
    int yy = fold(y - o.dy, a.h, a.reflect), xx = fold(x - o.dx, a.w, a.reflect);
    if ((yy | xx) < 0) return a.fill;
    if (o.d4 & 1) {
        const int t = yy;
        yy = xx;
        xx = t;
    }
    if (o.d4 & 2) xx = a.w - 1 - xx;
    if (o.d4 & 4) yy = a.h - 1 - yy;
    return load_elt<ELT>(img, yy * a.w + xx);
}

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

template <int V>
__device__ __forceinline__ void store_vec(uint8_t* __restrict__ p, const Vec<V>& v) {
    if constexpr (V == 16) *reinterpret_cast<uint4*>(p) = make_uint4(v.q[0], v.q[1], v.q[2], v.q[3]);
    else if constexpr (V == 8) *reinterpret_cast<uint2*>(p) = make_uint2(v.q[0], v.q[1]);
    else if constexpr (V == 4) *reinterpret_cast<uint32_t*>(p) = v.q[0];
    else *p = (uint8_t)v.q[0];
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

template <int ELT, int V>
__device__ __forceinline__ void set_elt(Vec<V>& v, int k, uint32_t val) {  // k is a compile-time index after unrolling
    if constexpr (ELT == 4) v.q[k] = val;
    else if constexpr (V == 1) v.q[0] = val;
    else v.q[k >> 2] |= (val & 0xffu) << (8 * (k & 3));
}

// ---- codes without bit 0: a band of consecutive stores of one output image --------------------------------------
template <int ELT, int V>
__device__ __forceinline__ void band(const AugArgs& a, const AugOp& o, const uint8_t* __restrict__ simg,
                                     uint8_t* __restrict__ dimg, int t) {
    constexpr int N = V / ELT;
    constexpr int NPT = kBandVectors / kAugThreads;
    const uint32_t base = (uint32_t)t * kBandVectors + threadIdx.x;
    Vec<V> v[NPT];
    int ys[NPT], x0s[NPT], plane[NPT];
    bool fast[NPT];
    const int flip = o.d4 & 2;
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const uint32_t idx = base + (uint32_t)k * kAugThreads;
        fast[k] = false;
        ys[k] = -1;
        if (idx >= a.total_vec) continue;
        const uint32_t r = idx / (uint32_t)a.nv;
        const int x0 = (int)(idx - r * (uint32_t)a.nv) * N;
        const uint32_t ch = r / (uint32_t)a.h;
        const int y = (int)(r - ch * (uint32_t)a.h);
        ys[k] = y;
        x0s[k] = x0;
        plane[k] = (int)ch * a.h * a.w;
        int yy = fold(y - o.dy, a.h, a.reflect);
        const int xs0 = x0 - o.dx;
        const bool erased = y >= o.ey0 && y < o.ey1 && x0 < o.ex1 && x0 + N > o.ex0;
        fast[k] = yy >= 0 && !erased && xs0 >= 0 && xs0 + N <= a.w;
        if (fast[k]) {
            if (o.d4 & 4) yy = a.h - 1 - yy;
            const int start = flip ? a.w - (xs0 + N) : xs0;
            v[k] = load_vec<ELT, V>(simg + (size_t)(plane[k] + yy * a.w + start) * ELT);
        }
    }
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        if (ys[k] < 0) continue;
        if (fast[k]) {
            if (flip) v[k] = reversed<ELT, V>(v[k]);
        } else {
            const uint8_t* __restrict__ pl = simg + (size_t)plane[k] * ELT;
#pragma unroll
            for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) v[k].q[i] = 0;
#pragma unroll
            for (int e = 0; e < N; ++e) set_elt<ELT, V>(v[k], e, pixel<ELT>(pl, o, a, ys[k], x0s[k] + e));
        }
        store_vec<V>(dimg + (size_t)(plane[k] + ys[k] * a.w + x0s[k]) * ELT, v[k]);
    }
}

// uint8 tiles (128 x 128, w >= 4): a thread takes blocks of 4 output rows x 4 output columns.  The four rows are four
// consecutive bytes of a SOURCE row wherever the reflection does not turn inside them, so a block is four dword loads
// (any alignment; lanes run along the source row: 32 lanes = 128 consecutive bytes), transposed in registers into four
// dword LDS writes.  Byte loads ran the uint8 quarter turn at half the rate of the plain gather: 64 of them per lane
// against 16 dwords here.  Quads that are not consecutive (image borders, a tile's ragged last rows) go per pixel.
__device__ __forceinline__ void load_tile_quads(const AugArgs& a, const AugOp& o, const uint8_t* __restrict__ pl, int y0,
                                                int x0, int vh, int vw, uint32_t* lds) {
    constexpr int P4 = 33;  // row pitch in dwords
    const int j4 = (threadIdx.x & 31) * 4, ib0 = threadIdx.x >> 5;  // 8 column blocks per pass, 32 in the tile
    const int yq = y0 + j4;
    const bool whole = j4 + 3 < vh;
    const int ya = fold(min(yq, a.h - 1) - o.dy, a.h, a.reflect), yb = fold(min(yq + 3, a.h - 1) - o.dy, a.h, a.reflect);
    const bool fast = whole && ya >= 0 && yb >= 0 && (yb - ya == 3 || ya - yb == 3);
    const int ca = (o.d4 & 2) ? a.w - 1 - ya : ya, cb = (o.d4 & 2) ? a.w - 1 - yb : yb;
    const int cs = fast ? min(ca, cb) : 0;  // cs + 3 <= w - 1
    const bool desc = cb < ca;
    uint32_t rect_rows = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) rect_rows |= (uint32_t)(yq + k >= o.ey0 && yq + k < o.ey1) << k;
    const uint32_t fill4 = a.fill * 0x01010101u;
#pragma unroll
    for (int u0 = 0; u0 < 4; u0 += 2) {
        uint32_t r[2][4], m_fill[2], m_in[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            m_fill[u] = m_in[u] = 0;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int x = x0 + min((ib0 + 8 * (u0 + u)) * 4 + m, vw - 1);
                const int xx = fold(x - o.dx, a.w, a.reflect);
                m_fill[u] |= xx < 0 ? 0xffu << (8 * m) : 0u;
                m_in[u] |= (x >= o.ex0 && x < o.ex1) ? 0xffu << (8 * m) : 0u;
                const int xc = max(xx, 0);
                const int row = (o.d4 & 4) ? a.h - 1 - xc : xc;
                r[u][m] = load_vec<1, 4>(pl + (size_t)(row * a.w + cs)).q[0];
            }
        }
        if (fast) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int ib = ib0 + 8 * (u0 + u);
                if (ib * 4 >= vw) continue;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int sh = 8 * (desc ? 3 - k : k);  // byte k of a quad is output row j4 + k
                    uint32_t w4 = ((r[u][0] >> sh) & 0xffu) | (((r[u][1] >> sh) & 0xffu) << 8) |
                                  (((r[u][2] >> sh) & 0xffu) << 16) | (((r[u][3] >> sh) & 0xffu) << 24);
                    const uint32_t mask = m_fill[u] | (((rect_rows >> k) & 1u) ? m_in[u] : 0u);
                    w4 = (w4 & ~mask) | (fill4 & mask);
                    lds[(j4 + k) * P4 + ib] = w4;  // (columns past vw inside the dword are never read back)
                }
            }
        }
    }
    if (!fast) {
        uint8_t* lds8 = reinterpret_cast<uint8_t*>(lds);
        for (int u = 0; u < 4; ++u)
            for (int m = 0; m < 4; ++m) {
                const int i = (ib0 + 8 * u) * 4 + m;
                if (i >= vw) continue;
                for (int k = 0; k < 4; ++k)
                    if (j4 + k < vh) lds8[(j4 + k) * (4 * P4) + i] = (uint8_t)pixel<1>(pl, o, a, yq + k, x0 + i);
            }
    }
}

// ---- codes with bit 0: an LDS tile in output layout ---------------------------------------------------------------
template <int ELT, int V>
__device__ __forceinline__ void tile_transposed(const AugArgs& a, const AugOp& o, const uint8_t* __restrict__ simg,
                                                uint8_t* __restrict__ dimg, int t, uint32_t* lds) {
    constexpr int N = V / ELT;
    constexpr int TS = ELT == 1 ? 128 : 64;
    constexpr int LOG_TS = ELT == 1 ? 7 : 6;
    constexpr int P = ELT == 1 ? 132 : 65;  // row pitch in pixels: 33 / 65 dwords, odd
    constexpr int VPR = TS / N;             // stores per tile row
    const int per_plane = a.tiles_y * a.tiles_x;
    const int ch = t / per_plane;
    const int tt = t - ch * per_plane;
    const int ty = tt / a.tiles_x;
    const int y0 = ty * TS, x0 = (tt - ty * a.tiles_x) * TS;
    const int vh = min(TS, a.h - y0), vw = min(TS, a.w - x0);
    const int plane = ch * a.h * a.w;
    const uint8_t* __restrict__ pl = simg + (size_t)plane * ELT;
    uint8_t* lds8 = reinterpret_cast<uint8_t*>(lds);

    bool by_quads = false;
    if constexpr (ELT == 1) by_quads = a.w >= 4;
    if (by_quads) {
        if constexpr (ELT == 1) load_tile_quads(a, o, pl, y0, x0, vh, vw, lds);
    } else {
        // lanes run along the output's y = the source's x; 256 is a multiple of TS, so a thread keeps its y: what
        // depends on y (the source column, the rectangle's rows) is resolved once.  Loads are unconditional, from a
        // clamped (always valid) address, UNROLL of them in flight before the first LDS write (one after the other they
        // cost a memory latency each: measured 93 against 42 us for the uint8 C3 batch).
        // (fp32, and uint8 images narrower than 4 pixels; wider uint8 tiles load dwords: load_tile_quads)
        constexpr int UNROLL = 8, ISTEP = kAugThreads / TS;
        const int j = threadIdx.x & (TS - 1), i0 = threadIdx.x >> LOG_TS;
        const int y = y0 + min(j, vh - 1);
        const int yy = fold(y - o.dy, a.h, a.reflect);
        const int yc = max(yy, 0);  // (-1: constant padding - the pixel is the fill, the load goes to a valid address)
        const int col = (o.d4 & 2) ? a.w - 1 - yc : yc;
        const bool row_fill = yy < 0, row_rect = y >= o.ey0 && y < o.ey1;
        for (int ib = 0; ib < vw; ib += ISTEP * UNROLL) {
            uint32_t val[UNROLL];
            uint32_t fill = 0;  // bit u: pixel u is the fill
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int x = x0 + min(ib + i0 + u * ISTEP, vw - 1);
                const int xx = fold(x - o.dx, a.w, a.reflect);
                fill |= (uint32_t)(row_fill || xx < 0 || (row_rect && x >= o.ex0 && x < o.ex1)) << u;
                const int xc = max(xx, 0);
                const int row = (o.d4 & 4) ? a.h - 1 - xc : xc;
                val[u] = load_elt<ELT>(pl, row * a.w + col);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int i = ib + i0 + u * ISTEP;
                if (i >= vw || j >= vh) continue;
                const uint32_t v = ((fill >> u) & 1u) ? a.fill : val[u];
                if constexpr (ELT == 1) lds8[j * P + i] = (uint8_t)v;
                else lds[j * P + i] = v;
            }
        }
    }
    __syncthreads();
    for (int vv = threadIdx.x; vv < TS * VPR; vv += kAugThreads) {
        const int j = vv / VPR, xi = (vv % VPR) * N;
        if (j >= vh) break;
        if (xi >= vw) continue;
        Vec<V> v;
        if constexpr (V == 1) {
            v.q[0] = lds8[j * P + xi];
        } else if constexpr (ELT == 1) {
#pragma unroll
            for (int q = 0; q < V / 4; ++q) v.q[q] = lds[(j * P + xi) / 4 + q];
        } else {
#pragma unroll
            for (int q = 0; q < V / 4; ++q) v.q[q] = lds[j * P + xi + q];
        }
        store_vec<V>(dimg + (size_t)(plane + (y0 + j) * a.w + x0 + xi) * ELT, v);
    }
}

template <int ELT, int V>
__global__ void __launch_bounds__(kAugThreads) batch_augment_kernel(const AugArgs a) {
    __shared__ uint32_t lds[kAugLdsBytes / 4];
    const int b = blockIdx.x / a.blocks_per_image;
    const int t = blockIdx.x - b * a.blocks_per_image;
    const AugOp o = sanitise(a.ops, b, a.h, a.w);
    int64_t row = a.rows ? a.rows[b] : (int64_t)b;
    row = row < 0 ? 0 : (row >= a.n_src ? a.n_src - 1 : row);
    const uint8_t* __restrict__ simg = a.src + row * a.img_bytes;  // 64-bit: a resident set is larger than 4 GB
    uint8_t* __restrict__ dimg = a.dst + (int64_t)b * a.img_bytes;
    if (o.d4 & 1) {
        if (t >= a.c * a.tiles_y * a.tiles_x) return;
        tile_transposed<ELT, V>(a, o, simg, dimg, t, lds);
    } else {
        if ((uint32_t)t * kBandVectors >= a.total_vec) return;
        band<ELT, V>(a, o, simg, dimg, t);
    }
}

struct AugPlan {
    int store_bytes, nv, tr_tile, tiles_y, tiles_x, blocks_per_image;
    uint32_t total_vec;
};

int augment_plan(const char* who, int c, int h, int w, int elt, const void* src, const void* dst, AugPlan* p) {
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
    p->tr_tile = elt == 1 ? 128 : 64;
    p->tiles_y = (int)cdiv(h, p->tr_tile);
    p->tiles_x = (int)cdiv(w, p->tr_tile);
    const int64_t bands = cdiv(p->total_vec, kBandVectors);
    const int64_t tiles = h == w ? (int64_t)c * p->tiles_y * p->tiles_x : 0;  // (bit 0 is dropped where h != w)
    p->blocks_per_image = (int)(bands > tiles ? bands : tiles);
    return MARL_OK;
}

template <int ELT>
int launch(const AugArgs& a, int v, int64_t blocks, hipStream_t st) {
    const dim3 grid((unsigned)blocks), block(kAugThreads);
    switch (v) {
        case 16: batch_augment_kernel<ELT, 16><<<grid, block, 0, st>>>(a); break;
        case 8: batch_augment_kernel<ELT, 8><<<grid, block, 0, st>>>(a); break;
        case 4: batch_augment_kernel<ELT, 4><<<grid, block, 0, st>>>(a); break;
        default:
            if constexpr (ELT == 1) batch_augment_kernel<1, 1><<<grid, block, 0, st>>>(a);
            break;
    }
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}

}  // namespace
}  // namespace marl

using namespace marl;

extern "C" int marl_batch_augment_plan(int c, int h, int w, int elt_bytes, const void* src, const void* dst,
                                       marl_augment_plan_info* out) {
    if (out == nullptr) {
        set_error("marl_batch_augment_plan: null argument");
        return MARL_EINVAL;
    }
    AugPlan p{};
    MARL_TRY(augment_plan("marl_batch_augment_plan", c, h, w, elt_bytes, src, dst, &p));
    *out = marl_augment_plan_info{};
    out->store_bytes = p.store_bytes;
    out->band_vectors = kBandVectors;
    out->tile_w = w;
    out->tile_h = (int)cdiv((int64_t)kBandVectors, p.nv);
    out->tr_tile = p.tr_tile;
    out->lds_bytes = kAugLdsBytes;
    out->blocks_per_image = p.blocks_per_image;
    return MARL_OK;
}

extern "C" int marl_batch_augment(const void* src, int64_t n_src, void* dst, const int64_t* rows, const int32_t* ops,
                                  int batch, int c, int h, int w, int elt_bytes, int pad_mode, uint32_t fill_bits,
                                  void* stream) {
    static const char* who = "marl_batch_augment";
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
    AugPlan p{};
    MARL_TRY(augment_plan(who, c, h, w, elt_bytes, src, dst, &p));
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
    AugArgs a{};
    a.src = static_cast<const uint8_t*>(src);
    a.dst = static_cast<uint8_t*>(dst);
    a.rows = rows;
    a.ops = ops;
    a.n_src = n_src;
    a.img_bytes = img_bytes;
    a.c = c, a.h = h, a.w = w;
    a.nv = p.nv;
    a.total_vec = p.total_vec;
    a.blocks_per_image = p.blocks_per_image;
    a.tiles_y = p.tiles_y, a.tiles_x = p.tiles_x;
    a.reflect = pad_mode == MARL_AUGMENT_PAD_REFLECT;
    a.fill = elt_bytes == 1 ? (fill_bits & 0xffu) : fill_bits;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return elt_bytes == 1 ? launch<1>(a, p.store_bytes, blocks, st) : launch<4>(a, p.store_bytes, blocks, st);
}
