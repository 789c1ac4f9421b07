// marl_batch_color (include/marl_hip_color.h): brightness, contrast, saturation and hue of every image of a batch as one
// per-image colour matrix, applied in one launch that moves the bytes a plain copy moves.  Rows are sanitised as the
// gathers do (clamp_row of gather.h, 64-bit source offsets); the vector width follows gather.h's rule - the widest of
// 16 / 8 / 4 bytes that divides a plane and both addresses, else one element - so every load and store is aligned and
// none reaches past a plane.
//
// A workgroup (256 threads) owns 1024 consecutive vectors of ONE image; a thread owns the pixels of four store vectors,
// 256 vectors apart, and needs all c planes of them.  It issues its 4 c vector loads first, then derives the image's matrix from params[b] and
// records[b] (workgroup-uniform addresses: scalar loads) in fp64 under the latency of those loads - as the normalise
// apply kernel derives its pair - applies it and issues 4 c vector stores.  Thread 0 of an image's first workgroup writes
// the matrix to `coef`.  No LDS, no atomics, no scratch.
//
// The translation unit is built with -ffp-contract=off (Makefile): the fp64 chain behind the matrix, the fp32 products
// and sums of the pixels and the normalising pair of OUT_NORM round every operation, as their definition in color.py
// does; the uint8 matrices equal color.reference_matrix integer for integer.
#include "gather.h"
#include "normrules.h"

#include "../../include/marl_hip_color.h"

namespace marl {
namespace {

constexpr int kColorThreads = 256;
constexpr int kColorMaxC = 3;
constexpr int kColorVectors = 4;  // vectors a thread owns: one matrix derivation pays for four of them

struct ColorArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int64_t* rows;
    const uint8_t* records;
    const int32_t* params;
    void* coef;
    int64_t n_src, img_bytes;
    int plane;  // h * w pixels
    int nvp;    // vectors per plane
    int bpi;    // workgroups per image
    int norm_mode;
    double user[kColorMaxC][2];
};

// (the matrix arithmetic is host-callable too: a CPU build can put it beside color.reference_matrix)
__host__ __device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// x . y, accumulated left to right, every product and sum rounded
template <int C>
__host__ __device__ __forceinline__ double dot(const double (&x)[C], const double (&y)[C]) {
    double acc = x[0] * y[0];
#pragma unroll
    for (int j = 1; j < C; ++j) acc = acc + x[j] * y[j];
    return acc;
}

// M = L M, o = L o
template <int C>
__host__ __device__ __forceinline__ void left_mul(const double (&L)[C][C], double (&M)[C][C], double (&o)[C]) {
    double N[C][C], p[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            double col[C];
#pragma unroll
            for (int k = 0; k < C; ++k) col[k] = M[k][j];
            N[i][j] = dot<C>(L[i], col);
        }
        p[i] = dot<C>(L[i], o);
    }
#pragma unroll
    for (int i = 0; i < C; ++i) {
#pragma unroll
        for (int j = 0; j < C; ++j) M[i][j] = N[i][j];
        o[i] = p[i];
    }
}

// The matrix of image b in fp64: the four stages of the header in their fixed order.  Everything read here sits at a
// workgroup-uniform address; nothing read is trusted.
template <int C, int ELT>
__host__ __device__ __forceinline__ void compose(const ColorArgs& a, int b, double (&M)[C][C], double (&o)[C]) {
    const int32_t* __restrict__ p = a.params + (size_t)b * MARL_COLOR_PARAMS;
    const double beta = (double)clamp_int(p[0], 0, MARL_COLOR_MAX_FACTOR) * (1.0 / MARL_COLOR_Q12);
    const double kappa = (double)clamp_int(p[1], 0, MARL_COLOR_MAX_FACTOR) * (1.0 / MARL_COLOR_Q12);
    double g[C];
    if constexpr (C == 3) g[0] = MARL_COLOR_G0 / 256.0, g[1] = MARL_COLOR_G1 / 256.0, g[2] = MARL_COLOR_G2 / 256.0;
    else g[0] = 1.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
#pragma unroll
        for (int j = 0; j < C; ++j) M[i][j] = i == j ? beta : 0.0;
        o[i] = 0.0;
    }
    if (a.records != nullptr) {  // contrast pivots on the grey mean of the brightened image
        double m[C];
        const Rec<typename RecOf<ELT>::T>* __restrict__ rec =
            reinterpret_cast<const Rec<typename RecOf<ELT>::T>*>(a.records) + (int64_t)b * C;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            if constexpr (ELT == 1) {  // (S1 is not trusted either: clamped to what N bytes can sum to)
                const int64_t top = 255 * (int64_t)a.plane, raw = rec[ch].s1;
                const int64_t s1 = raw < 0 ? 0 : (raw > top ? top : raw);
                m[ch] = (double)((256 * s1) / (int64_t)a.plane) * (1.0 / 256.0);
            } else {
                m[ch] = rec[ch].s1 / (double)a.plane;
            }
        }
        double v[C];
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = dot<C>(M[i], m) + o[i];
        const double shift = (1.0 - kappa) * dot<C>(g, v);
#pragma unroll
        for (int i = 0; i < C; ++i) {
#pragma unroll
            for (int j = 0; j < C; ++j) M[i][j] = kappa * M[i][j];
            o[i] = kappa * o[i] + shift;
        }
    }
    if constexpr (C == 3) {
        const double sigma = (double)clamp_int(p[2], 0, MARL_COLOR_MAX_FACTOR) * (1.0 / MARL_COLOR_Q12);
        const double hc = (double)clamp_int(p[3], -MARL_COLOR_Q14, MARL_COLOR_Q14) * (1.0 / MARL_COLOR_Q14);
        const double hs = (double)clamp_int(p[4], -MARL_COLOR_Q14, MARL_COLOR_Q14) * (1.0 / MARL_COLOR_Q14);
        const double K[3][3] = {
            {MARL_COLOR_K00, MARL_COLOR_K01, MARL_COLOR_K_LAST(MARL_COLOR_K00, MARL_COLOR_K01)},
            {MARL_COLOR_K10, MARL_COLOR_K11, MARL_COLOR_K_LAST(MARL_COLOR_K10, MARL_COLOR_K11)},
            {MARL_COLOR_K20, MARL_COLOR_K21, MARL_COLOR_K_LAST(MARL_COLOR_K20, MARL_COLOR_K21)}};
        const double rest = 1.0 - sigma;
        double L[C][C];
#pragma unroll
        for (int i = 0; i < C; ++i)
#pragma unroll
            for (int j = 0; j < C; ++j) L[i][j] = (i == j ? sigma : 0.0) + rest * g[j];
        left_mul<C>(L, M, o);
#pragma unroll
        for (int i = 0; i < C; ++i)
#pragma unroll
            for (int j = 0; j < C; ++j) L[i][j] = (g[j] + hc * ((i == j ? 1.0 : 0.0) - g[j])) + hs * K[i][j];
        left_mul<C>(L, M, o);
    }
}

__host__ __device__ __forceinline__ int quantise(double v, double bound) {
    const double r = rint(4096.0 * v);
    return (int)(r < -bound ? -bound : (r > bound ? bound : r));
}

// LB bytes from an LB-aligned address into dwords (LB == 1: the byte)
template <int LB>
__device__ __forceinline__ void load_aligned(const uint8_t* __restrict__ p, uint32_t* q) {
    if constexpr (LB == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
    } else if constexpr (LB == 8) {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        q[0] = v.x, q[1] = v.y;
    } else if constexpr (LB == 4) {
        q[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
        q[0] = *p;
    }
}

// C channels, ELT bytes per source element, PX pixels per vector (a thread owns kColorVectors of them); NORM: fp32 output through the user pair
template <int C, int ELT, int PX, bool NORM>
__global__ void __launch_bounds__(kColorThreads) batch_color_kernel(const ColorArgs a) {
    constexpr int LB = PX * ELT;               // bytes a thread loads per plane
    constexpr int OUT = NORM ? 4 : ELT;        // bytes per output element
    constexpr int SB = PX * OUT;               // bytes a thread stores per plane
    constexpr int LW = LB >= 4 ? LB / 4 : 1;   // dwords loaded
    constexpr int SW = SB >= 4 ? SB / 4 : 1;   // dwords stored
    const int b = blockIdx.x / a.bpi;
    const int k = blockIdx.x - b * a.bpi;
    const int idx0 = k * (kColorThreads * kColorVectors) + threadIdx.x;  // this thread's first vector of the plane
    const uint8_t* __restrict__ sp = a.src + clamp_row(a.rows ? a.rows[b] : (int64_t)b, a.n_src) * a.img_bytes;

    uint32_t raw[kColorVectors][C][LW];
#pragma unroll
    for (int v = 0; v < kColorVectors; ++v) {
        const int idx = idx0 + v * kColorThreads;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
#pragma unroll
            for (int d = 0; d < LW; ++d) raw[v][ch][d] = 0;
            if (idx < a.nvp)  // (nothing past a plane is read)
                load_aligned<LB>(sp + ((size_t)ch * a.plane * ELT + (size_t)idx * LB), raw[v][ch]);
        }
    }

    double M[C][C], o[C];
    compose<C, ELT>(a, b, M, o);
    int aq[C][C], oq[C];
    float af[C][C], of[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
#pragma unroll
        for (int j = 0; j < C; ++j) {
            if constexpr (ELT == 1) aq[i][j] = quantise(M[i][j], 524288.0);
            else af[i][j] = (float)M[i][j];
        }
        if constexpr (ELT == 1) oq[i] = quantise(o[i], 1073741824.0);
        else of[i] = (float)o[i];
    }
    if (k == 0 && threadIdx.x == 0 && a.coef != nullptr) {
        uint32_t* __restrict__ cp = static_cast<uint32_t*>(a.coef) + (size_t)b * C * (C + 1);
#pragma unroll
        for (int i = 0; i < C; ++i) {
#pragma unroll
            for (int j = 0; j < C; ++j) cp[i * (C + 1) + j] = ELT == 1 ? (uint32_t)aq[i][j] : __float_as_uint(af[i][j]);
            cp[i * (C + 1) + C] = ELT == 1 ? (uint32_t)oq[i] : __float_as_uint(of[i]);
        }
    }
    float scale[C], offset[C];
    if constexpr (NORM) {
#pragma unroll
        for (int i = 0; i < C; ++i) {  // (the pair of the user normalisation, uint8 source: normrules.h)
            double sc, of;
            user_coef<1>(a, a.norm_mode, i, sc, of);
            scale[i] = (float)sc, offset[i] = (float)of;
        }
    }
#pragma unroll
    for (int v = 0; v < kColorVectors; ++v) {
    const int idx = idx0 + v * kColorThreads;
    if (idx >= a.nvp) continue;
    uint8_t* __restrict__ dp = a.dst + (int64_t)b * C * a.plane * OUT + (size_t)idx * SB;
    uint32_t out[C][SW];
#pragma unroll
    for (int i = 0; i < C; ++i)
#pragma unroll
        for (int d = 0; d < SW; ++d) out[i][d] = 0;
    if constexpr (ELT == 1) {
#pragma unroll
        for (int e = 0; e < PX; ++e) {
            int x[C];
#pragma unroll
            for (int j = 0; j < C; ++j) x[j] = (int)((raw[v][j][e >> 2] >> (8 * (e & 3))) & 0xffu);
#pragma unroll
            for (int i = 0; i < C; ++i) {
                int acc = oq[i];  // |acc| <= 3 * 2^19 * 255 + 2^30 < 2^31
#pragma unroll
                for (int j = 0; j < C; ++j) acc += __mul24(aq[i][j], x[j]);  // (|A_q| <= 2^19, x < 2^8: exact, full rate)
                // (the shift and the clamp are kept apart: fused with the pack of two pixels they become
                // v_ashr_pk_u8_i32, after which the byte OR-ed in above the pair came back with a stray low bit on
                // the MI355X - tests/test_gpu_color.py, the 16- / 8- / 4-pixel uint8 shapes)
                int t = (acc + 2048) >> 12;
                asm volatile("" : "+v"(t));
                const int y = clampi(t, 0, 255);
                if constexpr (NORM) out[i][e] = __float_as_uint(__fadd_rn(rounded(__fmul_rn((float)y, scale[i])), offset[i]));
                else out[i][e >> 2] |= (uint32_t)y << (8 * (e & 3));
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < PX; ++e) {
#pragma unroll
            for (int i = 0; i < C; ++i) {
                float acc = 0.0f;
                bool any = false;  // (uniform over the workgroup: the coefficients are)
#pragma unroll
                for (int j = 0; j < C; ++j) {
                    if (af[i][j] == 0.0f) continue;
                    const float t = rounded(__fmul_rn(af[i][j], __uint_as_float(raw[v][j][e])));
                    acc = any ? rounded(__fadd_rn(acc, t)) : t;
                    any = true;
                }
                if (of[i] != 0.0f) acc = any ? __fadd_rn(acc, of[i]) : of[i];
                out[i][e] = __float_as_uint(acc);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < C; ++i) store_vec<SB>(dp + (size_t)i * a.plane * OUT, out[i]);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct ColorPlan {
    int px, load_bytes, store_bytes, nvp, bpi;
};

// The checks of gather_plan on the source (element, sizes, alignment, the 2^31 limit) behind the two of this family
// (the form, c), the destination's own alignment and limit, then the vector width.
int color_plan(const char* who, int c, int h, int w, int elt, int out_form, const void* src, const void* dst,
               ColorPlan* p) {
    if (out_form != MARL_COLOR_OUT_SAME && out_form != MARL_COLOR_OUT_NORM) {
        set_error("%s: unknown out_form %d", who, out_form);
        return MARL_EINVAL;
    }
    if (c != 1 && c != 3) {
        set_error("%s: c %d is neither 1 nor 3", who, c);
        return MARL_EINVAL;
    }
    const bool norm = out_form == MARL_COLOR_OUT_NORM;
    if (norm && elt == 4) {
        set_error("%s: MARL_COLOR_OUT_NORM takes uint8 sources only (elt_bytes 4)", who);
        return MARL_EINVAL;
    }
    GatherPlan g{};
    MARL_TRY(gather_plan(who, c, h, w, elt, src, norm ? nullptr : dst, &g));
    const int64_t plane = (int64_t)h * w;
    const uintptr_t s = reinterpret_cast<uintptr_t>(src), d = reinterpret_cast<uintptr_t>(dst);
    if (norm) {
        if (d & 3) {
            set_error("%s: the fp32 dst of MARL_COLOR_OUT_NORM must be 4-byte aligned", who);
            return MARL_EINVAL;
        }
        if (plane * c * 4 >= (int64_t)1 << 31) {
            set_error("%s: a dst image of %lld bytes (c %d, h %d, w %d) is beyond 2^31", who, (long long)(plane * c * 4),
                      c, h, w);
            return MARL_ELIMIT;
        }
        p->px = (plane % 4 == 0 && (s & 3) == 0 && (d & 15) == 0) ? 4 : 1;
        p->load_bytes = p->px, p->store_bytes = 4 * p->px;
    } else {
        const int v = store_width(plane * elt, s | d, elt);  // (uint8 planes that are no multiple of 4 bytes: bytes)
        p->px = v / elt;
        p->load_bytes = p->store_bytes = v;
    }
    p->nvp = (int)(plane / p->px);
    p->bpi = (int)cdiv(p->nvp, kColorThreads * kColorVectors);
    return MARL_OK;
}

template <int C>
void color_launch(const ColorArgs& a, int elt, bool norm, int px, dim3 grid, hipStream_t st) {
    if (elt == 4) {
        if (px == 4) batch_color_kernel<C, 4, 4, false><<<grid, kColorThreads, 0, st>>>(a);
        else if (px == 2) batch_color_kernel<C, 4, 2, false><<<grid, kColorThreads, 0, st>>>(a);
        else batch_color_kernel<C, 4, 1, false><<<grid, kColorThreads, 0, st>>>(a);
    } else if (norm) {
        if (px == 4) batch_color_kernel<C, 1, 4, true><<<grid, kColorThreads, 0, st>>>(a);
        else batch_color_kernel<C, 1, 1, true><<<grid, kColorThreads, 0, st>>>(a);
    } else {
        if (px == 16) batch_color_kernel<C, 1, 16, false><<<grid, kColorThreads, 0, st>>>(a);
        else if (px == 8) batch_color_kernel<C, 1, 8, false><<<grid, kColorThreads, 0, st>>>(a);
        else if (px == 4) batch_color_kernel<C, 1, 4, false><<<grid, kColorThreads, 0, st>>>(a);
        else batch_color_kernel<C, 1, 1, false><<<grid, kColorThreads, 0, st>>>(a);
    }
}

}  // namespace
}  // namespace marl

using namespace marl;

extern "C" int marl_batch_color_plan(int c, int h, int w, int elt_bytes, int out_form, const void* src, const void* dst,
                                     marl_color_plan_info* out) {
    if (out == nullptr) {
        set_error("marl_batch_color_plan: null argument");
        return MARL_EINVAL;
    }
    ColorPlan p{};
    MARL_TRY(color_plan("marl_batch_color_plan", c, h, w, elt_bytes, out_form, src, dst, &p));
    *out = marl_color_plan_info{};
    out->load_bytes = p.load_bytes;
    out->store_bytes = p.store_bytes;
    out->pixels_per_vector = p.px;
    out->vectors_per_thread = kColorVectors;
    out->blocks_per_image = p.bpi;
    out->lds_bytes = 0;
    return MARL_OK;
}

extern "C" int marl_batch_color(const void* src, int64_t n_src, const int64_t* rows, const void* records,
                                const int32_t* params, int out_form, int norm_mode, const double* user, int batch, int c,
                                int h, int w, int elt_bytes, void* dst, void* coef, void* stream) {
    static const char* who = "marl_batch_color";
    if (src == nullptr || dst == nullptr || params == nullptr) {
        set_error("%s: null src / dst / params", who);
        return MARL_EINVAL;
    }
    MARL_TRY(need_batch(who, batch, n_src));
    ColorPlan p{};
    MARL_TRY(color_plan(who, c, h, w, elt_bytes, out_form, src, dst, &p));
    const bool norm = out_form == MARL_COLOR_OUT_NORM;
    ColorArgs a{};
    if (norm) {
        if (norm_mode != MARL_NORM_USER_NORMAL && norm_mode != MARL_NORM_USER_MINMAX) {
            set_error("%s: MARL_COLOR_OUT_NORM takes a user norm_mode (%d or %d), got %d: statistic modes are two steps",
                      who, MARL_NORM_USER_NORMAL, MARL_NORM_USER_MINMAX, norm_mode);
            return MARL_EINVAL;
        }
        if (user == nullptr) {
            set_error("%s: norm_mode %d needs user", who, norm_mode);
            return MARL_EINVAL;
        }
        MARL_TRY(user_pairs(who, norm_mode, user, c, a.user));
    }
    MARL_TRY(need_rows_cover(who, rows, n_src, batch));
    const int64_t pixels = (int64_t)c * h * w, img_bytes = pixels * elt_bytes, out_bytes = pixels * (norm ? 4 : elt_bytes);
    MARL_TRY(need_extent(who, n_src, img_bytes));
    MARL_TRY(need_apart(who, src, n_src * img_bytes, dst, (int64_t)batch * out_bytes,
                        "a thread reads all planes of its pixels, other threads write them"));
    MARL_TRY(need_aligned(who, "records and rows", 8, records, rows));
    MARL_TRY(need_aligned(who, "coef and params", 4, coef, params));
    const int64_t blocks = (int64_t)batch * p.bpi;
    MARL_TRY(need_grid(who, blocks, batch));
    a.src = static_cast<const uint8_t*>(src);
    a.dst = static_cast<uint8_t*>(dst);
    a.rows = rows;
    a.records = static_cast<const uint8_t*>(records);
    a.params = params;
    a.coef = coef;
    a.n_src = n_src;
    a.img_bytes = img_bytes;
    a.plane = h * w, a.nvp = p.nvp, a.bpi = p.bpi, a.norm_mode = norm_mode;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks);
    if (c == 3) color_launch<3>(a, elt_bytes, norm, p.px, grid, st);
    else color_launch<1>(a, elt_bytes, norm, p.px, grid, st);
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}
