// marl_batch_stats / marl_batch_normalize (include/marl_hip_normalize.h): per-image, per-channel statistics of the
// rows of a resident image set, and the affine map dst = x * scale + offset that standardises them - the reduction over
// image planes the gather family lacked, and its elementwise consumer.  Rows are sanitised as the gathers do
// (clamp_row of gather.h, 64-bit source offsets); the store width is the plan of gather.h for a plane taken as one row
// of fp32.
//
// Statistics, store-and-sum like report.hip.  Partial pass: a workgroup (256 threads) owns one chunk of kChunkBytes
// consecutive bytes of ONE plane.  The chunk's 16-byte aligned body is read as uint4 (at most kBodyIters per lane, all
// in flight together); its unaligned head and tail (< 16 bytes each) go one element per lane.  uint8: a lane keeps
// sum x and sum x^2 as 32-bit integers - v_dot4_u32_u8 gives both sums of a dword in two instructions - and min / max
// as two 16-bit halves (even / odd bytes, v_pk_min_u16 / v_pk_max_u16).  A lane sees at most 16 * kBodyIters + 2 = 66
// elements, so its sum x^2 stays below 66 * 255^2 < 2^23.  fp32: the lane sums are fp64, min / max exact.  Lanes are
// folded by a shuffle tree, the four waves in ascending order by thread 0: a fixed order, so fp64 sums repeat bit for
// bit.  Fold pass: one thread per plane adds the plane's partial records in ascending chunk order.  No atomics.
//
// Apply: a workgroup owns kApplyVectors consecutive stores of one plane.  Every thread derives the plane's (scale,
// offset) from the records of its image in fp64 (uniform addresses: scalar loads; whole-image modes add the channels'
// records first, in integers for uint8) and rounds them once to fp32; then dst = fadd_rn(fmul_rn(x, scale), offset).
// The translation unit is built with -ffp-contract=off (Makefile): neither that pair nor the fp64 chain may be fused,
// the definition (transforms.reference_coef / reference_apply) rounds every operation.
#include "gather.h"
#include "normrules.h"

namespace marl {
namespace {

constexpr int kNormThreads = 256;
constexpr int kNormWaves = kNormThreads / kWave;
constexpr int kChunkBytes = 16384;
constexpr int kBodyIters = kChunkBytes / 16 / kNormThreads;  // 4
constexpr int kStatsLdsBytes = kNormWaves * MARL_NORM_RECORD_BYTES;
constexpr int kApplyStoresPerThread = 4;
constexpr int kApplyVectors = kApplyStoresPerThread * kNormThreads;
static_assert((16 * kBodyIters + 2) * 255ll * 255ll < (1ll << 32), "a lane's 32-bit sum of squares");

struct StatsArgs {
    const uint8_t* src;
    const int64_t* rows;
    int64_t n_src, img_bytes;
    int c, plane;  // plane = h * w elements
    int ppp;       // partials per plane
    uint8_t* scratch;
    uint8_t* records;
    int64_t planes;  // batch * c
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
    const us2 r = __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b));
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
    const us2 r = __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b));
    return __builtin_bit_cast(uint32_t, r);
}

// lane 0 of a wave ends with the wave's total, in the order of the tree
template <class T, class Op>
__device__ __forceinline__ T wave_tree(T v, Op op) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v = op(v, __shfl_down(v, off, kWave));
    return v;
}

template <int ELT>
__global__ void __launch_bounds__(kNormThreads) batch_stats_partial_kernel(const StatsArgs a) {
    using T = typename RecOf<ELT>::T;
    __shared__ Rec<T> part[kNormWaves];
    constexpr int CH = kChunkBytes / ELT;
    const int64_t pl = blockIdx.x / a.ppp;  // (b, ch)
    const int k = (int)(blockIdx.x - pl * a.ppp);
    const int b = (int)(pl / a.c), ch = (int)(pl - (int64_t)b * a.c);
    const int e0 = k * CH;
    const int n = min(CH, a.plane - e0);  // >= 1
    const uint8_t* __restrict__ p = a.src + clamp_row(a.rows ? a.rows[b] : (int64_t)b, a.n_src) * a.img_bytes +
                                    ((int64_t)ch * a.plane + e0) * ELT;
    const int head = min(n, (int)((16u - ((uint32_t)reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / ELT);
    const int nbody = (n - head) / (16 / ELT);  // <= kBodyIters * kNormThreads
    const int tail0 = head + nbody * (16 / ELT), ntail = n - tail0;
    const int t = threadIdx.x;
    const uint4* __restrict__ body = reinterpret_cast<const uint4*>(p + (size_t)head * ELT);

    uint4 v[kBodyIters];
#pragma unroll
    for (int i = 0; i < kBodyIters; ++i) {
        const int j = t + i * kNormThreads;
        v[i] = make_uint4(0, 0, 0, 0);
        if (j < nbody) v[i] = body[j];  // (predicated: nothing past the chunk is read)
    }
    T s1, s2, mn, mx;
    if constexpr (ELT == 1) {
        uint32_t u1 = 0, u2 = 0, lo = 0x00ff00ffu, hi = 0;
#pragma unroll
        for (int i = 0; i < kBodyIters; ++i) {
            if (t + i * kNormThreads >= nbody) continue;
            const uint32_t q[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                u1 = __builtin_amdgcn_udot4(q[d], 0x01010101u, u1, false);
                u2 = __builtin_amdgcn_udot4(q[d], q[d], u2, false);
                const uint32_t ev = q[d] & 0x00ff00ffu, od = (q[d] >> 8) & 0x00ff00ffu;
                lo = pk_min(pk_min(lo, ev), od);
                hi = pk_max(pk_max(hi, ev), od);
            }
        }
        uint32_t lo1 = min(lo & 0xffffu, lo >> 16), hi1 = max(hi & 0xffffu, hi >> 16);
        if (t < head) {
            const uint32_t x = p[t];
            u1 += x, u2 += x * x, lo1 = min(lo1, x), hi1 = max(hi1, x);
        }
        if (t < ntail) {
            const uint32_t x = p[tail0 + t];
            u1 += x, u2 += x * x, lo1 = min(lo1, x), hi1 = max(hi1, x);
        }
        s1 = u1, s2 = u2, mn = lo1, mx = hi1;
    } else {
        double d1 = 0.0, d2 = 0.0;
        float lo = __builtin_inff(), hi = -__builtin_inff();
        auto take = [&](uint32_t bits) {
            const float x = __uint_as_float(bits);
            const double xd = (double)x;
            d1 += xd;
            d2 += xd * xd;  // (the square of an fp32 is exact in fp64)
            lo = fminf(lo, x);
            hi = fmaxf(hi, x);
        };
#pragma unroll
        for (int i = 0; i < kBodyIters; ++i) {
            if (t + i * kNormThreads >= nbody) continue;
            take(v[i].x), take(v[i].y), take(v[i].z), take(v[i].w);
        }
        const uint32_t* __restrict__ pe = reinterpret_cast<const uint32_t*>(p);
        if (t < head) take(pe[t]);
        if (t < ntail) take(pe[tail0 + t]);
        s1 = d1, s2 = d2, mn = (double)lo, mx = (double)hi;
    }
    auto add = [](T x, T y) { return x + y; };
    auto lower = [](T x, T y) { return y < x ? y : x; };
    auto upper = [](T x, T y) { return y > x ? y : x; };
    s1 = wave_tree(s1, add);
    s2 = wave_tree(s2, add);
    mn = wave_tree(mn, lower);
    mx = wave_tree(mx, upper);
    if ((t & (kWave - 1)) == 0) part[t / kWave] = Rec<T>{s1, s2, mn, mx};
    __syncthreads();
    if (t == 0) {
        Rec<T> r = part[0];
#pragma unroll
        for (int wv = 1; wv < kNormWaves; ++wv) {
            r.s1 = add(r.s1, part[wv].s1), r.s2 = add(r.s2, part[wv].s2);
            r.mn = lower(r.mn, part[wv].mn), r.mx = upper(r.mx, part[wv].mx);
        }
        reinterpret_cast<Rec<T>*>(a.scratch)[blockIdx.x] = r;
    }
}

template <int ELT>
__global__ void __launch_bounds__(kNormThreads) batch_stats_fold_kernel(const StatsArgs a) {
    using T = typename RecOf<ELT>::T;
    const int64_t pl = (int64_t)blockIdx.x * kNormThreads + threadIdx.x;
    if (pl >= a.planes) return;
    const Rec<T>* __restrict__ part = reinterpret_cast<const Rec<T>*>(a.scratch) + pl * a.ppp;
    Rec<T> r = part[0];
    for (int k = 1; k < a.ppp; ++k) {  // ascending chunk order
        const Rec<T> q = part[k];
        r.s1 += q.s1, r.s2 += q.s2;
        r.mn = q.mn < r.mn ? q.mn : r.mn;
        r.mx = q.mx > r.mx ? q.mx : r.mx;
    }
    reinterpret_cast<Rec<T>*>(a.records)[pl] = r;
}

struct NormArgs {
    const uint8_t* src;
    uint8_t* dst;
    const int64_t* rows;
    const uint8_t* records;
    float* coef;
    int64_t n_src, img_bytes;
    int c, plane;
    int nvp;  // stores per plane
    int bpp;  // workgroups per plane
    int mode;
    double user[MARL_NORM_MAX_USER_CHANNELS][2];
};

// (scale, offset) of plane ch of image b: fp64, every operation rounded, then one rounding to fp32
template <int ELT>
__device__ __forceinline__ void derive_coef(const NormArgs& a, int b, int ch, float& scale, float& offset) {
    using T = typename RecOf<ELT>::T;
    double sc = 0.0, of = 0.0;
    if (a.mode == MARL_NORM_USER_NORMAL) {  // (one call per mode: a call under `normal || minmax` moves the kernel)
        user_coef<ELT>(a, MARL_NORM_USER_NORMAL, ch, sc, of);
    } else if (a.mode == MARL_NORM_USER_MINMAX) {
        user_coef<ELT>(a, MARL_NORM_USER_MINMAX, ch, sc, of);
    } else {
        const bool whole = a.mode == MARL_NORM_NORMAL || a.mode == MARL_NORM_MINMAX;
        const Rec<T>* __restrict__ rec = reinterpret_cast<const Rec<T>*>(a.records) + (int64_t)b * a.c;
        Rec<T> r = rec[whole ? 0 : ch];
        if (whole)
            for (int j = 1; j < a.c; ++j) {
                const Rec<T> q = rec[j];
                r.s1 += q.s1, r.s2 += q.s2;
                r.mn = q.mn < r.mn ? q.mn : r.mn;
                r.mx = q.mx > r.mx ? q.mx : r.mx;
            }
        const int64_t n = whole ? (int64_t)a.c * a.plane : (int64_t)a.plane;
        if (a.mode == MARL_NORM_NORMAL || a.mode == MARL_NORM_CHANNEL_NORMAL) {
            double num;
            if constexpr (ELT == 1) num = (double)(n * r.s2 - r.s1 * r.s1);  // exact below 2^62, converted once
            else num = (double)n * r.s2 - r.s1 * r.s1;
            if (n >= 2 && num > 0.0) {
                const double sd = sqrt(num / (double)(n * (n - 1)));
                const double mean = (double)r.s1 / (double)n;
                sc = 1.0 / sd;
                of = -mean / sd;
            }
        } else {
            const double d = (double)r.mx - (double)r.mn;
            if (d > 0.0) {
                sc = 1.0 / d;
                of = -(double)r.mn / d;
            }
        }
    }
    scale = (float)sc;
    offset = (float)of;
}

template <int ELT, int V>
__global__ void __launch_bounds__(kNormThreads) batch_normalize_kernel(const NormArgs a) {
    constexpr int N = V / 4;  // pixels per store
    const int64_t pl = blockIdx.x / a.bpp;
    const int k = (int)(blockIdx.x - pl * a.bpp);
    const int b = (int)(pl / a.c), ch = (int)(pl - (int64_t)b * a.c);
    const uint8_t* __restrict__ sp = a.src + clamp_row(a.rows ? a.rows[b] : (int64_t)b, a.n_src) * a.img_bytes +
                                     (int64_t)ch * a.plane * ELT;
    uint8_t* __restrict__ dp = a.dst + pl * ((int64_t)a.plane * 4);

    uint32_t x[kApplyStoresPerThread][N];
#pragma unroll
    for (int i = 0; i < kApplyStoresPerThread; ++i) {
        const int idx = k * kApplyVectors + i * kNormThreads + threadIdx.x;
        if (idx >= a.nvp) continue;
        const uint8_t* __restrict__ s = sp + (size_t)idx * N * ELT;
        if constexpr (ELT == 4) {
            const Vec<V> v = load_vec<4, V>(s);
#pragma unroll
            for (int e = 0; e < N; ++e) x[i][e] = v.q[e];
        } else if constexpr (N == 4) {
            const uint32_t q = load_vec<1, 4>(s).q[0];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[i][e] = (q >> (8 * e)) & 0xffu;
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) x[i][e] = s[e];
        }
    }
    float scale, offset;
    derive_coef<ELT>(a, b, ch, scale, offset);
    if (k == 0 && threadIdx.x == 0 && a.coef != nullptr) {
        a.coef[pl * 2] = scale;
        a.coef[pl * 2 + 1] = offset;
    }
#pragma unroll
    for (int i = 0; i < kApplyStoresPerThread; ++i) {
        const int idx = k * kApplyVectors + i * kNormThreads + threadIdx.x;
        if (idx >= a.nvp) continue;
        uint32_t q[N];
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const float xf = ELT == 1 ? (float)x[i][e] : __uint_as_float(x[i][e]);
            q[e] = __float_as_uint(__fadd_rn(rounded(__fmul_rn(xf, scale)), offset));
        }
        store_vec<V>(dp + (size_t)idx * V, q);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct NormPlan {
    int chunk_elems, ppp, store_bytes, nvp, bpp;
};

// the checks of gather_plan on the source (sizes, element, alignment, the 2^31 limit), then on dst as [c, 1, h w] fp32
// (its alignment, its own 2^31 limit, the store width of a plane taken as one row)
int normalize_plan(const char* who, int c, int h, int w, int elt, const void* src, const void* dst, bool need_dst,
                   NormPlan* p) {
    GatherPlan g{};
    MARL_TRY(gather_plan(who, c, h, w, elt, src, nullptr, &g));
    const int plane = h * w;  // (c h w elt < 2^31)
    p->chunk_elems = kChunkBytes / elt;
    p->ppp = (int)cdiv(plane, p->chunk_elems);
    p->store_bytes = 4, p->nvp = plane, p->bpp = (int)cdiv(plane, kApplyVectors);
    if (need_dst) {
        MARL_TRY(gather_plan(who, c, 1, plane, 4, nullptr, dst, &g));
        p->store_bytes = g.store_bytes;
        p->nvp = g.nv;
        p->bpp = (int)cdiv(g.nv, kApplyVectors);
    }
    return MARL_OK;
}

// The guards both entries share: the rules of gather.h in the order of gather_guard, around this family's plan and its
// one rule of its own (kept here, not folded into the entries, so that rule stands once); need_dst = false: the
// statistics, which write no image.  stat_limit: the entry takes (or consumes) statistics of the image, so a uint8 image is bounded by 2^23 pixels.
int normalize_guard(const char* who, const void* src, int64_t n_src, const int64_t* rows, int batch, int c, int h, int w,
                    int elt, const void* dst, bool need_dst, bool stat_limit, NormPlan* p) {
    MARL_TRY(need_batch(who, batch, n_src));
    MARL_TRY(normalize_plan(who, c, h, w, elt, src, dst, need_dst, p));
    MARL_TRY(need_rows_cover(who, rows, n_src, batch));
    const int64_t pixels = (int64_t)c * h * w, img_bytes = pixels * elt;
    MARL_TRY(need_extent(who, n_src, img_bytes));
    if (stat_limit && elt == 1 && pixels > MARL_NORM_MAX_STAT_PIXELS) {
        set_error("%s: the statistics of a uint8 image of %lld pixels (c %d, h %d, w %d) are beyond 2^23", who,
                  (long long)pixels, c, h, w);
        return MARL_ELIMIT;
    }
    if (need_dst)
        MARL_TRY(need_apart(who, src, n_src * img_bytes, dst, (int64_t)batch * pixels * 4,
                            "the output is fp32 whatever the source is"));
    return MARL_OK;
}

}  // namespace
}  // namespace marl

using namespace marl;

extern "C" int marl_batch_normalize_plan(int c, int h, int w, int elt_bytes, const void* src, const void* dst,
                                         marl_normalize_plan_info* out) {
    if (out == nullptr) {
        set_error("marl_batch_normalize_plan: null argument");
        return MARL_EINVAL;
    }
    NormPlan p{};
    MARL_TRY(normalize_plan("marl_batch_normalize_plan", c, h, w, elt_bytes, src, dst, true, &p));
    *out = marl_normalize_plan_info{};
    out->chunk_elems = p.chunk_elems;
    out->partials_per_plane = p.ppp;
    out->load_bytes = 16;
    out->lds_bytes = kStatsLdsBytes;
    out->store_bytes = p.store_bytes;
    out->apply_chunk_elems = kApplyVectors * (p.store_bytes / 4);
    out->apply_blocks_per_plane = p.bpp;
    return MARL_OK;
}

extern "C" size_t marl_batch_stats_scratch_bytes(int batch, int c, int h, int w, int elt_bytes) {
    NormPlan p{};
    if (batch <= 0 || normalize_plan("marl_batch_stats_scratch_bytes", c, h, w, elt_bytes, nullptr, nullptr, false,
                                     &p) != MARL_OK)
        return 0;
    return (size_t)batch * c * p.ppp * MARL_NORM_RECORD_BYTES;
}

extern "C" int marl_batch_stats(const void* src, int64_t n_src, const int64_t* rows, int batch, int c, int h, int w,
                                int elt_bytes, void* scratch, void* records, void* stream) {
    static const char* who = "marl_batch_stats";
    if (src == nullptr || scratch == nullptr || records == nullptr) {
        set_error("%s: null src / scratch / records", who);
        return MARL_EINVAL;
    }
    NormPlan p{};
    MARL_TRY(normalize_guard(who, src, n_src, rows, batch, c, h, w, elt_bytes, nullptr, false, true, &p));
    MARL_TRY(need_aligned(who, "scratch and records", 8, scratch, records));
    StatsArgs a{};
    a.src = static_cast<const uint8_t*>(src);
    a.rows = rows;
    a.n_src = n_src;
    a.img_bytes = (int64_t)c * h * w * elt_bytes;
    a.c = c, a.plane = h * w, a.ppp = p.ppp;
    a.scratch = static_cast<uint8_t*>(scratch);
    a.records = static_cast<uint8_t*>(records);
    a.planes = (int64_t)batch * c;
    const int64_t blocks = a.planes * p.ppp;
    MARL_TRY(need_grid(who, blocks, batch));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), fold((unsigned)cdiv(a.planes, kNormThreads));
    if (elt_bytes == 1) {
        batch_stats_partial_kernel<1><<<grid, kNormThreads, 0, st>>>(a);
        batch_stats_fold_kernel<1><<<fold, kNormThreads, 0, st>>>(a);
    } else {
        batch_stats_partial_kernel<4><<<grid, kNormThreads, 0, st>>>(a);
        batch_stats_fold_kernel<4><<<fold, kNormThreads, 0, st>>>(a);
    }
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}

extern "C" int marl_batch_normalize(const void* src, int64_t n_src, const int64_t* rows, const void* records, int mode,
                                    const double* user, int batch, int c, int h, int w, int elt_bytes, float* dst,
                                    float* coef, void* stream) {
    static const char* who = "marl_batch_normalize";
    if (src == nullptr || dst == nullptr) {
        set_error("%s: null src / dst", who);
        return MARL_EINVAL;
    }
    if (mode < MARL_NORM_NORMAL || mode > MARL_NORM_USER_MINMAX) {
        set_error("%s: unknown mode %d", who, mode);
        return MARL_EINVAL;
    }
    const bool by_user = mode == MARL_NORM_USER_NORMAL || mode == MARL_NORM_USER_MINMAX;
    if (by_user ? user == nullptr : records == nullptr) {
        set_error("%s: mode %d needs %s", who, mode, by_user ? "user" : "records");
        return MARL_EINVAL;
    }
    NormArgs a{};
    if (by_user) {  // (c <= 0 is the size guard's below)
        if (c > MARL_NORM_MAX_USER_CHANNELS) {
            set_error("%s: user modes take at most %d channels, got %d", who, MARL_NORM_MAX_USER_CHANNELS, c);
            return MARL_EINVAL;
        }
        MARL_TRY(user_pairs(who, mode, user, c, a.user));
    }
    NormPlan p{};
    MARL_TRY(normalize_guard(who, src, n_src, rows, batch, c, h, w, elt_bytes, dst, true, !by_user, &p));
    if (!by_user) MARL_TRY(need_aligned(who, "records", 8, records));
    MARL_TRY(need_aligned(who, "coef", 4, coef));
    a.src = static_cast<const uint8_t*>(src);
    a.dst = reinterpret_cast<uint8_t*>(dst);
    a.rows = rows;
    a.records = by_user ? nullptr : static_cast<const uint8_t*>(records);
    a.coef = coef;
    a.n_src = n_src;
    a.img_bytes = (int64_t)c * h * w * elt_bytes;
    a.c = c, a.plane = h * w, a.nvp = p.nvp, a.bpp = p.bpp, a.mode = mode;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // gather_launch's grid guard and its switch over the store widths: dst is fp32, so V is 16, 8 or 4 for either
    // source element
    GatherCall call{};
    call.batch = batch, call.elt = 4;
    const GatherPlan g{p.store_bytes, p.nvp};
    return gather_launch(who, call, g, c * p.bpp, [&](auto, auto v, dim3 grid) {
        if constexpr (v >= 4) {  // (the switch also names byte stores, which fp32 never takes)
            if (elt_bytes == 1) batch_normalize_kernel<1, v><<<grid, kNormThreads, 0, st>>>(a);
            else batch_normalize_kernel<4, v><<<grid, kNormThreads, 0, st>>>(a);
        }
    });
}
