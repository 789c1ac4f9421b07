// marl_optim_step (include/marl_hip_optim.h): AdamW over the flat buffers with per-segment learning-rate multipliers
// and decoupled weight decay, a learning-rate schedule and an optional averaged copy of the weights, in one launch.
// A pure streaming kernel: 7 streams of 4n bytes (read p, g, m, v; write p, m, v), 9 with the average.
//
// Work split.  A lane owns one float4 of each buffer per trip of a grid-stride loop (the grid cap is launch_adam's);
// segment starts are multiples of 4 floats, so a float4 never straddles two segments.  The segment table arrives by
// value in the kernel arguments and is copied to LDS once per workgroup; a lane finds its segment by a branchless
// binary search over the segment ends (a trip count the whole grid shares: no divergence).  The first trip's global
// loads are issued before the scalars are derived, so that fp64 chain hides under their latency.  A frozen segment (lr_mult == 0) is skipped by predication: its
// float4s are loaded and never stored.
//
// Step-dependent scalars.  lr_t and the two bias corrections are derived from the integer step in fp64 by the first
// lane of every workgroup while the others copy the table, then broadcast through LDS: the step is either an argument
// or the counter block's field, and the code is the same, so eager calls and graph replays agree bit for bit.
// beta^t is a square-and-multiply product (at most 2 * 63 fp64 multiplications - no call into a pow routine); the
// quotients lr_t / bc1 and 1 / sqrt(bc2), which the elements use in fp32, are formed in fp32 from the rounded scalars.
#include "common.h"

#include <cmath>

#include "../../include/marl_hip_optim.h"

namespace marl {
namespace {

constexpr int kMaxSeg = MARL_OPTIM_MAX_SEGMENTS;
constexpr int kOptimThreads = 256;
constexpr int kOptimGridCap = 4096;  // launch_adam's

struct OptimArgs {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* ema;
    float* scalars_out;
    const Counters* cnt;
    int64_t n;
    int64_t step;
    int64_t warmup, total;
    double beta1, beta2, eps, base_lr, final_ratio, ema_decay;
    float grad_scale;
    int kind;
    int search_top;  // the smallest power of two >= count
    uint32_t end4[kMaxSeg];  // segment ends in float4 units, ascending; slots >= count hold 0xffffffff
    float mult[kMaxSeg];
    float wd[kMaxSeg];
};
static_assert(sizeof(OptimArgs) <= 2048, "the kernel-argument block is 4 KB");

// b1^e and b2^e by square-and-multiply, the two dependent chains interleaved
__device__ inline void pow_int2(double b1, double b2, uint64_t e, double& r1, double& r2) {
    r1 = r2 = 1.0;
    while (e) {
        if (e & 1) {
            r1 *= b1;
            r2 *= b2;
        }
        b1 *= b1;
        b2 *= b2;
        e >>= 1;
    }
}

__device__ inline double schedule_lr(const OptimArgs& a, uint64_t t) {
    const double td = (double)t;
    if ((int64_t)t <= a.warmup) return a.base_lr * (td / (double)a.warmup);  // (warmup >= 1 here; exactly base_lr at t == warmup)
    if (a.kind == MARL_SCHED_CONSTANT) return a.base_lr;
    const double span = (double)(a.total - a.warmup);
    double x = span > 0.0 ? (td - (double)a.warmup) / span : 1.0;
    x = x < 1.0 ? x : 1.0;
    if (a.kind == MARL_SCHED_LINEAR) return a.base_lr * (1.0 - (1.0 - a.final_ratio) * x);
    return a.base_lr * (a.final_ratio + (1.0 - a.final_ratio) * 0.5 * (1.0 + cospi(x)));  // (x in [0, 1]: no range reduction)
}

__device__ inline float wave_uniform(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

struct ElemConsts {
    float keep;       // 1 - lr_t * lr_mult * weight_decay
    float step_size;  // lr_t * lr_mult / bc1
    float inv_sqrt_bc2, one_m_b1, beta2, one_m_b2, eps, grad_scale, ema_decay, one_m_ema;
};

template <bool kEma>
__device__ inline void optim_elem(float& p, float g, float& m, float& v, float& e, const ElemConsts& c) {
    const float gr = g * c.grad_scale;
    const float pd = c.keep != 1.0f ? p * c.keep : p;
    m = m + c.one_m_b1 * (gr - m);
    v = v * c.beta2 + c.one_m_b2 * (gr * gr);
    const float denom = sqrtf(v) * c.inv_sqrt_bc2 + c.eps;
    p = pd - c.step_size * (m / denom);
    if (kEma) e = c.ema_decay * e + c.one_m_ema * p;
}

// float4 i of every buffer (i < n / 4: a whole one)
template <bool kEma>
__device__ inline void optim_load(const OptimArgs& a, int64_t i, float4& g, float4& p, float4& m, float4& v,
                                  float4& e) {
    g = reinterpret_cast<const float4*>(a.g)[i];
    p = reinterpret_cast<const float4*>(a.p)[i];
    m = reinterpret_cast<const float4*>(a.m)[i];
    v = reinterpret_cast<const float4*>(a.v)[i];
    if (kEma) e = reinterpret_cast<const float4*>(a.ema)[i];
}

// the counter block's step through the scalar cache: a scalar load counts on lgkmcnt, so waiting for it leaves the
// vector loads in flight (device memory written by an earlier kernel: the scalar cache is invalidated at kernel start)
__device__ inline uint64_t scalar_load_u64(const uint64_t* p) {
    return *reinterpret_cast<const __attribute__((address_space(4))) uint64_t*>(reinterpret_cast<uintptr_t>(p));
}

// (8 waves per SIMD, 7 with the average - 64 / 72 VGPRs: the 6588 waves of the C3 buffer are resident at once on 256
// CUs; at 6 waves per SIMD a second round of workgroups pays the whole latency again)
// kTiny: n < 4, there is no whole float4 to load ahead (one lane walks the elements; the launcher picks it).
template <bool kEma, bool kTiny>
__global__ void __launch_bounds__(kOptimThreads, kEma ? 7 : 8) optim_kernel(const OptimArgs a) {
    __shared__ uint32_t s_end[kMaxSeg];
    __shared__ float s_mult[kMaxSeg];
    __shared__ float s_wd[kMaxSeg];
    __shared__ float s_sc[4];
    const int tid = threadIdx.x;
    const int64_t full4 = a.n >> 2, n4 = (a.n + 3) >> 2;
    const int64_t stride = (int64_t)gridDim.x * kOptimThreads;
    int64_t i = (int64_t)blockIdx.x * kOptimThreads + tid;
    // Issue order matters: vector loads return in order and the compiler counts them (s_waitcnt vmcnt(N)) only across
    // straight-line code.  So the table entries waves 1 and 2 copy go out FIRST, the first trip's data loads behind
    // them WITHOUT a branch (lanes past the last whole float4 load a clamped index and drop it), and the step comes
    // through the scalar cache: the fp64 chain and the LDS traffic below then run under the latency of the data.
    const uint64_t t = a.cnt ? scalar_load_u64(&a.cnt->step) : (uint64_t)a.step;
    const bool copier = tid >= 64 && tid < 64 + kMaxSeg;  // (waves 1 and 2 copy the table while wave 0 derives the scalars)
    const int ts = copier ? tid - 64 : 0;
    uint32_t t_end = 0;
    float t_mult = 0.f, t_wd = 0.f;
    if (copier) {
        t_end = a.end4[ts];
        t_mult = a.mult[ts];
        t_wd = a.wd[ts];
    }
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 g = zero, p = zero, m = zero, v = zero, e = zero;
    if (!kTiny) optim_load<kEma>(a, i < full4 ? i : full4 - 1, g, p, m, v, e);
    if (copier) {
        s_end[ts] = t_end;
        s_mult[ts] = t_mult;
        s_wd[ts] = t_wd;
    }
    if (tid == 0) {
        const double lr_t = schedule_lr(a, t);
        double pw1, pw2;
        pow_int2(a.beta1, a.beta2, t, pw1, pw2);
        const double bc1 = 1.0 - pw1, bc2 = 1.0 - pw2;
        // (the quotients the elements use are fp32 anyway: an fp64 division and square root here are 1.3 us that the
        // loads above do not hide - measured; three fp32 roundings are 2e-7 of a step held to 1e-3)
        s_sc[0] = (float)lr_t;
        s_sc[1] = (float)lr_t / (float)bc1;
        s_sc[2] = 1.0f / sqrtf((float)bc2);
        if (blockIdx.x == 0 && a.scalars_out) {
            a.scalars_out[0] = (float)lr_t;
            a.scalars_out[1] = (float)bc1;
            a.scalars_out[2] = (float)bc2;
            a.scalars_out[3] = (float)t;
        }
    }
    __syncthreads();
    // (wave-uniform constants live in scalar registers: a dozen VGPRs less, which is what 8 waves per SIMD takes)
    const float lr_t = wave_uniform(s_sc[0]), lr_over_bc1 = wave_uniform(s_sc[1]);
    ElemConsts c;
    c.inv_sqrt_bc2 = wave_uniform(s_sc[2]);
    c.one_m_b1 = wave_uniform((float)(1.0 - a.beta1));
    c.beta2 = wave_uniform((float)a.beta2);
    c.one_m_b2 = wave_uniform((float)(1.0 - a.beta2));
    c.eps = wave_uniform((float)a.eps);
    c.grad_scale = a.grad_scale;
    c.ema_decay = wave_uniform((float)a.ema_decay);
    c.one_m_ema = wave_uniform((float)(1.0 - a.ema_decay));

    float4* __restrict__ p4 = reinterpret_cast<float4*>(a.p);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(a.m);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(a.v);
    float4* __restrict__ e4 = reinterpret_cast<float4*>(a.ema);
    while (i < n4) {
        // the first segment whose end lies behind this float4
        const uint32_t iu = (uint32_t)i;
        int seg = 0;
        for (int w = a.search_top >> 1; w >= 1; w >>= 1) seg += s_end[seg + w - 1] <= iu ? w : 0;
        const float mult = s_mult[seg];
        if (mult != 0.0f) {  // (else frozen: nothing is written)
            c.keep = 1.0f - lr_t * mult * s_wd[seg];
            c.step_size = lr_over_bc1 * mult;
            if (i < full4) {
                optim_elem<kEma>(p.x, g.x, m.x, v.x, e.x, c);
                optim_elem<kEma>(p.y, g.y, m.y, v.y, e.y, c);
                optim_elem<kEma>(p.z, g.z, m.z, v.z, e.z, c);
                optim_elem<kEma>(p.w, g.w, m.w, v.w, e.w, c);
                m4[i] = m;
                v4[i] = v;
                p4[i] = p;
                if (kEma) e4[i] = e;
            } else {  // the last, partial float4 of a buffer whose length is no multiple of 4
                for (int64_t j = i * 4; j < a.n; ++j) {
                    float pj = a.p[j], mj = a.m[j], vj = a.v[j], ej = kEma ? a.ema[j] : 0.f;
                    optim_elem<kEma>(pj, a.g[j], mj, vj, ej, c);
                    a.m[j] = mj;
                    a.v[j] = vj;
                    a.p[j] = pj;
                    if (kEma) a.ema[j] = ej;
                }
            }
        }
        i += stride;
        if (i < full4) optim_load<kEma>(a, i, g, p, m, v, e);
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool unit_open(double x) { return x >= 0.0 && x < 1.0; }  // (false for NaN)

}  // namespace
}  // namespace marl

using namespace marl;

extern "C" int marl_optim_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema,
                               int64_t n, float grad_scale, const marl_optim_segment* segments, int n_segments,
                               double beta1, double beta2, double eps, const marl_optim_schedule* schedule,
                               int64_t step, const void* counters, double ema_decay, float* scalars_out,
                               void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !schedule || n < 0 || (n + 3) / 4 >= (int64_t)0xffffffffLL) {
        set_error("optim_step: null buffer or bad length");
        return MARL_EINVAL;
    }
    if (!aligned16(params) || !aligned16(grads) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) || !aligned16(ema) ||
        (reinterpret_cast<uintptr_t>(scalars_out) & 3) != 0) {
        set_error("optim_step: the flat buffers must be 16-byte aligned");
        return MARL_EINVAL;
    }
    if (!counters && step < 1) {
        set_error("optim_step: step %lld < 1 without a counter block", (long long)step);
        return MARL_EINVAL;
    }
    if (!unit_open(beta1) || !unit_open(beta2) || !(eps > 0.0) || !std::isfinite(eps) || !std::isfinite(grad_scale)) {
        set_error("optim_step: betas must lie in [0, 1), eps must be > 0, grad_scale finite");
        return MARL_EINVAL;
    }
    if (ema && !(ema_decay > 0.0 && ema_decay < 1.0)) {
        set_error("optim_step: ema_decay %g outside (0, 1)", ema_decay);
        return MARL_EINVAL;
    }
    const marl_optim_schedule& sc = *schedule;
    if (sc.kind < MARL_SCHED_CONSTANT || sc.kind > MARL_SCHED_COSINE || !(sc.base_lr >= 0.0) ||
        !std::isfinite(sc.base_lr) || sc.warmup_steps < 0 ||
        (sc.kind != MARL_SCHED_CONSTANT && sc.total_steps < sc.warmup_steps) ||
        !(sc.final_ratio >= 0.0 && sc.final_ratio <= 1.0)) {
        set_error("optim_step: bad schedule (kind %d, base_lr %g, warmup %lld, total %lld, final_ratio %g)", sc.kind,
                  sc.base_lr, (long long)sc.warmup_steps, (long long)sc.total_steps, sc.final_ratio);
        return MARL_EINVAL;
    }
    if (n_segments < 0 || n_segments > kMaxSeg || (n_segments > 0 && !segments) || (n > 0 && n_segments == 0)) {
        set_error("optim_step: %d segments (1 .. %d)", n_segments, kMaxSeg);
        return MARL_EINVAL;
    }
    OptimArgs a;
    int64_t at = 0;
    for (int s = 0; s < n_segments; ++s) {
        const marl_optim_segment& g = segments[s];
        if ((g.begin & 3) != 0 || g.begin != at || g.end <= g.begin || g.end > n) {
            set_error("optim_step: segment %d [%lld, %lld) is misaligned, empty, out of order, overlaps or leaves a gap "
                      "behind element %lld of %lld", s, (long long)g.begin, (long long)g.end, (long long)at,
                      (long long)n);
            return MARL_EINVAL;
        }
        if (!(g.lr_mult >= 0.f) || !std::isfinite(g.lr_mult) || !(g.weight_decay >= 0.f) ||
            !std::isfinite(g.weight_decay)) {
            set_error("optim_step: segment %d has lr_mult %g, weight_decay %g", s, g.lr_mult, g.weight_decay);
            return MARL_EINVAL;
        }
        at = g.end;
        a.end4[s] = (uint32_t)((g.end + 3) >> 2);
        a.mult[s] = g.lr_mult;
        a.wd[s] = g.weight_decay;
    }
    if (at != n) {
        set_error("optim_step: the segments end at %lld of %lld elements", (long long)at, (long long)n);
        return MARL_EINVAL;
    }
    if (n == 0) return MARL_OK;
    for (int s = n_segments; s < kMaxSeg; ++s) {
        a.end4[s] = 0xffffffffu;
        a.mult[s] = 0.f;
        a.wd[s] = 0.f;
    }
    a.p = params;
    a.g = grads;
    a.m = exp_avg;
    a.v = exp_avg_sq;
    a.ema = ema;
    a.scalars_out = scalars_out;
    a.cnt = static_cast<const Counters*>(counters);
    a.n = n;
    a.step = step;
    a.warmup = sc.warmup_steps;
    a.total = sc.total_steps;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.base_lr = sc.base_lr;
    a.final_ratio = sc.final_ratio;
    a.ema_decay = ema ? ema_decay : 0.0;
    a.grad_scale = grad_scale;
    a.kind = sc.kind;
    a.search_top = 1;
    while (a.search_top < n_segments) a.search_top <<= 1;
    int64_t gx = cdiv((n + 3) >> 2, kOptimThreads);
    if (gx > kOptimGridCap) gx = kOptimGridCap;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 4) {
        if (ema)
            hipLaunchKernelGGL((optim_kernel<true, true>), dim3(1), dim3(kOptimThreads), 0, st, a);
        else
            hipLaunchKernelGGL((optim_kernel<false, true>), dim3(1), dim3(kOptimThreads), 0, st, a);
    } else if (ema) {
        hipLaunchKernelGGL((optim_kernel<true, false>), dim3((unsigned)gx), dim3(kOptimThreads), 0, st, a);
    } else {
        hipLaunchKernelGGL((optim_kernel<false, false>), dim3((unsigned)gx), dim3(kOptimThreads), 0, st, a);
    }
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}
