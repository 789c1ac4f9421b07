// marl_batch_augment (include/marl_hip_augment.h): the batch gather of the resident image set with the augmentation
// fused in - a dihedral code, an integer shift with reflect / constant padding and one erased rectangle per output
// image, all of it index remapping, so the launch moves the bytes a plain index_select moves (read each selected
// image once, write it once).  One kernel, no workspace, no atomics.
//
// Work split.  A workgroup (256 threads) owns a piece of ONE output image; rows[b] and ops[b] are loads at a
// workgroup-uniform address, sanitised once (nothing read from device memory is trusted: view_of() of gather.h).
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
#include "gather.h"

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

// ops[b] with img at one plane of the source image, for the per-pixel rule (plane offset 0).  The kernel's View has no
// img: it reads its row after the ops and hands the image down beside the View, as its code object always has.
__device__ __forceinline__ View plane_view(const View& o, const uint8_t* __restrict__ pl) {
    View p = o;
    p.img = pl;
    return p;
}

// ---- codes without bit 0: a band of consecutive stores of one output image --------------------------------------
template <int ELT, int V>
__device__ __forceinline__ void band(const AugArgs& a, const View& o, const uint8_t* __restrict__ simg,
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
            const View pv = plane_view(o, simg + (size_t)plane[k] * ELT);
#pragma unroll
            for (int i = 0; i < (V >= 4 ? V / 4 : 1); ++i) v[k].q[i] = 0;
#pragma unroll
            for (int e = 0; e < N; ++e) set_elt<ELT, V>(v[k], e, pixel<ELT>(a, pv, 0, ys[k], x0s[k] + e));
        }
        store_vec<V>(dimg + (size_t)(plane[k] + ys[k] * a.w + x0s[k]) * ELT, v[k].q);
    }
}

// uint8 tiles (128 x 128, w >= 4): a thread takes blocks of 4 output rows x 4 output columns.  The four rows are four
// consecutive bytes of a SOURCE row wherever the reflection does not turn inside them, so a block is four dword loads
// (any alignment; lanes run along the source row: 32 lanes = 128 consecutive bytes), transposed in registers into four
// dword LDS writes.  Byte loads ran the uint8 quarter turn at half the rate of the plain gather: 64 of them per lane
// against 16 dwords here.  Quads that are not consecutive (image borders, a tile's ragged last rows) go per pixel.
__device__ __forceinline__ void load_tile_quads(const AugArgs& a, const View& o, const uint8_t* __restrict__ pl, int y0,
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
                    if (j4 + k < vh)
                        lds8[(j4 + k) * (4 * P4) + i] = (uint8_t)pixel<1>(a, plane_view(o, pl), 0, yq + k, x0 + i);
            }
    }
}

// ---- codes with bit 0: an LDS tile in output layout ---------------------------------------------------------------
template <int ELT, int V>
__device__ __forceinline__ void tile_transposed(const AugArgs& a, const View& o, const uint8_t* __restrict__ simg,
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
        store_vec<V>(dimg + (size_t)(plane + (y0 + j) * a.w + x0 + xi) * ELT, v.q);
    }
}

template <int ELT, int V>
__global__ void __launch_bounds__(kAugThreads) batch_augment_kernel(const AugArgs a) {
    __shared__ uint32_t lds[kAugLdsBytes / 4];
    const int b = blockIdx.x / a.blocks_per_image;
    const int t = blockIdx.x - b * a.blocks_per_image;
    const View o = view_of<false>(a, b);
    const uint8_t* __restrict__ simg = a.src + clamp_row(a.rows ? a.rows[b] : (int64_t)b, a.n_src) * a.img_bytes;
    uint8_t* __restrict__ dimg = a.dst + (int64_t)b * a.img_bytes;
    if (o.d4 & 1) {
        if (t >= a.c * a.tiles_y * a.tiles_x) return;
        tile_transposed<ELT, V>(a, o, simg, dimg, t, lds);
    } else {
        if ((uint32_t)t * kBandVectors >= a.total_vec) return;
        band<ELT, V>(a, o, simg, dimg, t);
    }
}

// what the plan of gather.h leaves to this kernel: the band count and the transposing path's tiles
struct AugPlan {
    int tr_tile, tiles_y, tiles_x, blocks_per_image;
    uint32_t total_vec;
};

AugPlan augment_plan(const GatherPlan& g, int c, int h, int w, int elt) {
    AugPlan p{};
    p.total_vec = (uint32_t)((int64_t)c * h * g.nv);
    p.tr_tile = elt == 1 ? 128 : 64;
    p.tiles_y = (int)cdiv(h, p.tr_tile);
    p.tiles_x = (int)cdiv(w, p.tr_tile);
    const int64_t bands = cdiv(p.total_vec, kBandVectors);
    const int64_t tiles = h == w ? (int64_t)c * p.tiles_y * p.tiles_x : 0;  // (bit 0 is dropped where h != w)
    p.blocks_per_image = (int)(bands > tiles ? bands : tiles);
    return p;
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
    GatherPlan g{};
    MARL_TRY(gather_plan("marl_batch_augment_plan", c, h, w, elt_bytes, src, dst, &g));
    const AugPlan p = augment_plan(g, c, h, w, elt_bytes);
    *out = marl_augment_plan_info{};
    out->store_bytes = g.store_bytes;
    out->band_vectors = kBandVectors;
    out->tile_w = w;
    out->tile_h = (int)cdiv((int64_t)kBandVectors, g.nv);
    out->tr_tile = p.tr_tile;
    out->lds_bytes = kAugLdsBytes;
    out->blocks_per_image = p.blocks_per_image;
    return MARL_OK;
}

extern "C" int marl_batch_augment(const void* src, int64_t n_src, void* dst, const int64_t* rows, const int32_t* ops,
                                  int batch, int c, int h, int w, int elt_bytes, int pad_mode, uint32_t fill_bits,
                                  void* stream) {
    static const char* who = "marl_batch_augment";
    const GatherCall call{src, n_src, dst, rows, ops, batch, c, h, w, elt_bytes, pad_mode, fill_bits};
    GatherPlan g{};
    MARL_TRY(gather_guard(who, "in place is undefined for flips", call, &g));
    const AugPlan p = augment_plan(g, c, h, w, elt_bytes);
    AugArgs a = gather_args<AugArgs>(call, g);
    a.total_vec = p.total_vec;
    a.blocks_per_image = p.blocks_per_image;
    a.tiles_y = p.tiles_y, a.tiles_x = p.tiles_x;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return gather_launch(who, call, g, p.blocks_per_image, [&](auto elt, auto v, dim3 grid) {
        batch_augment_kernel<elt, v><<<grid, kAugThreads, 0, st>>>(a);
    });
}
