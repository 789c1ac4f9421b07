// A2C loss of Trainer.train_epoch (training/trainer.py:76-111) and its gradient with
// respect to the episode outputs, in a handful of small HBM-bound kernels:
//   rewards (functions.py:7-32) -> vote error (trainer.py:78-87) -> discounted returns
//   (functions.py:35-51, flip-cumsum order) -> global mean / unbiased std
//   (functions.py:54-55) -> path / critic terms and gradients (trainer.py:96-111).
// All cross-thread sums go through fixed-order partials (fp64) -> bit-reproducible.
// Under marl_class_loss (include/marl_hip_classloss.h) the rewards and the vote error run their option instances:
// class weights, label smoothing, step weights, rewards times the label's weight - same launches, same order.
// Under marl_soft_targets (include/marl_hip_softtargets.h) the same two launches run their soft instances: a target
// distribution per image where the label was.
#include "common.h"

#include <cassert>
#include <type_traits>

namespace marl {

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wmax(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// tree over K per-thread fp64 values; thread 0 ends up with the block sums in sh[k][0]
template <int K>
__device__ __forceinline__ void block_tree(double (*sh)[256], const double (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = v[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + o];
        }
        __syncthreads();
    }
}

// advn = (adv - mean) / (std + 1e-8) with the global mean / unbiased std of adv_stats (functions.py:54-55)
__device__ __forceinline__ float standardized(float adv, const double* __restrict__ adv_stats) {
    const double n = adv_stats[0];
    const double mean_d = adv_stats[1] / n;
    const double var_d = (adv_stats[2] - adv_stats[1] * mean_d) / (n - 1.0);
    const float mean = (float)mean_d;
    const float sd = (float)sqrt(var_d > 0.0 ? var_d : 0.0);
    return (adv - mean) / (sd + 1e-8f);
}

// smooth-L1 of d = value - return (the critic term); *grad = its derivative
__device__ __forceinline__ float smooth_l1(float d, float* grad) {
    const float ad = fabsf(d);
    *grad = ad < 1.0f ? d : (d > 0.f ? 1.0f : -1.0f);
    return ad < 1.0f ? 0.5f * d * d : ad - 0.5f;
}

// entropy bonus of one row of the step distributions [nA]: returns sum_j p_j log p_j (= -H) and writes
// g[j] = scale * (log p_j + 1).  0 * log 0 = 0: an exactly zero probability adds nothing to H and gets a zero gradient
// (nothing becomes NaN / Inf).  VEC: nA % 4 == 0 and 16-byte aligned tensors - the row moves as float4s.
template <bool VEC>
__device__ __forceinline__ float row_entropy(const float* __restrict__ p, float* __restrict__ g, int nA, float scale) {
    float h = 0.f;
    auto term = [&](float pj) {  // adds p log p to h, returns the gradient
        if (!(pj > 0.f)) return 0.f;
        const float lp = logf(pj);
        h = fmaf(pj, lp, h);
        return scale * (lp + 1.0f);
    };
    if (VEC) {
        const float4* pv = reinterpret_cast<const float4*>(p);
        float4* gv = reinterpret_cast<float4*>(g);
        for (int k = 0; k < nA / 4; ++k) {
            const float4 v = pv[k];
            float4 o;
            o.x = term(v.x);
            o.y = term(v.y);
            o.z = term(v.z);
            o.w = term(v.w);
            gv[k] = o;
        }
    } else {
        for (int j = 0; j < nA; ++j) g[j] = term(p[j]);
    }
    return h;
}

struct LossLayout {
    double* part_adv;   // [blocksC][2]
    double* part_loss;  // [blocksE][2]
    double* part_err;   // [1]
    float* rew;         // [Ns*R]
    float* ret;         // [Ns*R]
    float* adv;         // [Ns*R]
    float* err;         // [Ns*Nb]
    double* spare;      // the 16 floats behind err, from the first 8-byte boundary
    int blocksC, blocksE;
};

static LossLayout loss_layout(float* scratch, int ns, int na, int nb) {
    LossLayout L;
    const int64_t R = (int64_t)na * nb, NR = R * ns;
    L.blocksC = (int)cdiv(R, 256);
    L.blocksE = (int)cdiv(NR, 256);
    double* d = reinterpret_cast<double*>(scratch);
    L.part_adv = d;
    L.part_loss = d + 2 * L.blocksC;
    L.part_err = L.part_loss + 2 * L.blocksE;
    float* f = reinterpret_cast<float*>(L.part_err + 2);
    L.rew = f;
    L.ret = f + NR;
    L.adv = f + 2 * NR;
    L.err = f + 3 * NR;
    L.spare = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(L.err + (int64_t)ns * nb) + 7) & ~(uintptr_t)7);
    return L;
}

size_t loss_scratch_floats(int ns, int na, int nb) {
    const int64_t R = (int64_t)na * nb, NR = R * ns;
    const int64_t dbl = 2 * cdiv(R, 256) + 2 * cdiv(NR, 256) + 2;
    return (size_t)(2 * dbl + 3 * NR + (int64_t)ns * nb + 16);
}

// where a grads kernel keeps the k doubles per block it sums beyond part_loss (k = 1: the A2C entropy, k = 3: PPO).
// One block: the 16 spare floats behind `err` - 3 doubles and up to 7 bytes of alignment are 31 of their 64 bytes.
// More blocks: the place of the rewards [NR floats], dead since the returns / GAE kernel read them (an earlier phase
// or marl_advantages) - blocksE > 1 means NR >= 257, and k * blocksE doubles are 2 k cdiv(NR, 256) <= 6 (NR / 256 + 1)
// floats, which is below NR from NR = 7 on.
static double* extra_partials(const LossLayout& L, int k) {
    assert(k <= 3);
    return L.blocksE == 1 ? L.spare : reinterpret_cast<double*>(L.rew);
}

// the one place that picks the <ENT, VEC> instance of a grads kernel: launch(ent, vec) gets two std::bool_constant
template <class F>
static void with_grads_instance(const LossGradArgs& a, F&& launch) {
    const bool vec = a.n_act % 4 == 0 && (reinterpret_cast<uintptr_t>(a.probs) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(a.g_probs) & 15) == 0;
    if (!a.probs)
        launch(std::false_type{}, std::false_type{});
    else if (vec)
        launch(std::true_type{}, std::true_type{});
    else
        launch(std::true_type{}, std::false_type{});
}

// Options of the vote error and the rewards (marl_class_loss, include/marl_hip_classloss.h) as the OPT instances of
// the two kernels below take them; the plain instances carry an empty struct and none of it.
struct NoClassOpt {};
struct ClassOpt {
    const float* w;   // [nC] class weights, nullptr = all ones
    const float* sw;  // [Ns] step weights, nullptr = all ones
    float keep;       // 1 - eps
    float eps_nc;     // eps / nC
};

// rew[t, r] = (log nC - CE(preds[t, r, :], y[b])) / log nC ; one wave per (t, r)
// OPT (weight_rewards): times w[y[b]], the cost-sensitive reward
template <bool OPT>
__global__ __launch_bounds__(256) void loss_rewards_kernel(const float* __restrict__ preds,
                                                           const int64_t* __restrict__ y,
                                                           float* __restrict__ rew, int64_t NR,
                                                           int nb, int nc, float rnd,
                                                           std::conditional_t<OPT, ClassOpt, NoClassOpt> o) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= NR) return;
    const float* p = preds + row * nc;
    float mx = -INFINITY;
    for (int c = lane; c < nc; c += 64) mx = fmaxf(mx, p[c]);
    mx = wmax(mx);
    float s = 0.f;
    for (int c = lane; c < nc; c += 64) s += expf(p[c] - mx);
    s = wsum(s);
    if (lane == 0) {
        const int b = (int)(row % nb);
        const float ce = -(p[y[b]] - mx - logf(s));
        if constexpr (OPT)
            rew[row] = o.w[y[b]] * ((rnd - ce) / rnd);  // (launched with weights only)
        else
            rew[row] = (rnd - ce) / rnd;
    }
}

// err[t, b] = CE(mean_a preds[t, a, b, :], y[b]);  g_preds[t, a, b, c] = (softmax - onehot) / R
// OPT: with nll_c = -(z_c - max z - log sum exp(z - max z)), q_c = (1 - eps) w_y 1[c == y] + (eps / nC) w_c:
//   err[t, b] = s_t sum_c q_c nll_c,   g_preds[t, a, b, c] = s_t / R (softmax_c sum_c' q_c' - q_c)
// sum_c w_c nll_c and sum_c w_c are two more wave sums (fixed order); the wave reads w once, into LDS beside the vote.
// With w == 1, eps == 0, s_t == 1 every product is by 1 and every sum adds a zero: the plain instance's bits.
template <bool OPT>
__global__ __launch_bounds__(256) void loss_error_kernel(const float* __restrict__ preds,
                                                         const int64_t* __restrict__ y,
                                                         float* __restrict__ err,
                                                         float* __restrict__ g_preds, int ld_gp,
                                                         int ns, int na, int nb, int nc,
                                                         std::conditional_t<OPT, ClassOpt, NoClassOpt> o) {
    __shared__ float pbar[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tb = (int64_t)blockIdx.x * 4 + wave;
    if (tb >= (int64_t)ns * nb) return;
    const int t = (int)(tb / nb), b = (int)(tb % nb);
    const int64_t R = (int64_t)na * nb;
    float mx = -INFINITY;
    for (int c = lane; c < nc; c += 64) {
        float s = 0.f;
        for (int a = 0; a < na; ++a) s += preds[((int64_t)t * R + (int64_t)a * nb + b) * nc + c];
        s = s / (float)na;
        pbar[wave][c] = s;
        mx = fmaxf(mx, s);
    }
    mx = wmax(mx);
    float s = 0.f;
    for (int c = lane; c < nc; c += 64) s += expf(pbar[wave][c] - mx);
    s = wsum(s);
    const int yb = (int)y[b];
    if constexpr (!OPT) {
        if (lane == 0) err[tb] = -(pbar[wave][yb] - mx - logf(s));
        if (g_preds) {
            const float inv = 1.0f / (float)R;
            for (int c = lane; c < nc; c += 64) {
                const float g = (expf(pbar[wave][c] - mx) / s - (c == yb ? 1.0f : 0.0f)) * inv;
                for (int a = 0; a < na; ++a)
                    g_preds[((int64_t)t * R + (int64_t)a * nb + b) * ld_gp + c] = g;
            }
        }
    } else {
        __shared__ float wcls[4][1024];
        const float ls = logf(s);
        float wn = 0.f, wt = 0.f;  // sum_c w_c nll_c, sum_c w_c
        for (int c = lane; c < nc; c += 64) {
            const float wc = o.w ? o.w[c] : 1.0f;
            wcls[wave][c] = wc;
            wn = fmaf(wc, -(pbar[wave][c] - mx - ls), wn);
            wt += wc;
        }
        wn = wsum(wn);
        wt = wsum(wt);
        const float st = o.sw ? o.sw[t] : 1.0f;
        const float qy = o.keep * (o.w ? o.w[yb] : 1.0f);  // the label's own share of q
        if (lane == 0) {
            float e = qy * -(pbar[wave][yb] - mx - ls);
            if (o.eps_nc != 0.f) e = fmaf(o.eps_nc, wn, e);
            err[tb] = st * e;
        }
        if (g_preds) {
            const float sc = st * (1.0f / (float)R);
            const float qs = o.eps_nc != 0.f ? fmaf(o.eps_nc, wt, qy) : qy;  // sum_c q_c
            for (int c = lane; c < nc; c += 64) {
                const float qc = (c == yb ? qy : 0.0f) + o.eps_nc * wcls[wave][c];
                const float g = (expf(pbar[wave][c] - mx) / s * qs - qc) * sc;
                for (int a = 0; a < na; ++a)
                    g_preds[((int64_t)t * R + (int64_t)a * nb + b) * ld_gp + c] = g;
            }
        }
    }
}

// ---- a target distribution per image in place of the label (marl_soft_targets, include/marl_hip_softtargets.h) ------
// The label kernels above stay what they are; these are further instances of the same two launches.  Q is [nb, nc];
// entries with Q[b, c] == 0 are skipped, not multiplied (a logit of -inf beside them stays out of every sum).  Every
// class sum is a fixed-order wave sum, and the arithmetic is ordered so that a one-hot Q gives the label kernels' bits:
// the one term that is not skipped is the label kernel's own expression times 1, and the sums add zeros to it.

// rew[t, r] = sum_c omega_c Q[b, c] (log nC - nll_c(preds[t, r, :])) / log nC ; one wave per (t, r)
// OPT (weight_rewards): omega = w, else 1
template <bool OPT>
__global__ __launch_bounds__(256) void loss_rewards_soft_kernel(const float* __restrict__ preds,
                                                                const float* __restrict__ q,
                                                                float* __restrict__ rew, int64_t NR,
                                                                int nb, int nc, float rnd,
                                                                std::conditional_t<OPT, ClassOpt, NoClassOpt> o) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= NR) return;
    const float* p = preds + row * nc;
    float mx = -INFINITY;
    for (int c = lane; c < nc; c += 64) mx = fmaxf(mx, p[c]);
    mx = wmax(mx);
    float s = 0.f;
    for (int c = lane; c < nc; c += 64) s += expf(p[c] - mx);
    s = wsum(s);
    const float* qb = q + (int64_t)(row % nb) * nc;
    float acc = 0.f;
    for (int c = lane; c < nc; c += 64) {
        const float qc = qb[c];
        if (qc == 0.f) continue;
        const float ce = -(p[c] - mx - logf(s));
        if constexpr (OPT)
            acc += o.w[c] * (qc * ((rnd - ce) / rnd));  // (launched with weights only)
        else
            acc += qc * ((rnd - ce) / rnd);
    }
    acc = wsum(acc);
    if (lane == 0) rew[row] = acc;
}

// err[t, b] = s_t sum_c q_c nll_c,  g_preds[t, a, b, c] = s_t / R (softmax_c sum_c' q_c' - q_c) with
// q_c = w_c ((1 - eps) Q[b, c] + eps / nC); the plain instance has w = 1, eps = 0, s = 1 and none of their arithmetic.
// q_c is formed as (keep w_c) Q[b, c] + (eps / nC) w_c: loss_error_kernel<true>'s qy 1[c == y] + (eps / nC) w_c.
template <bool OPT>
__global__ __launch_bounds__(256) void loss_error_soft_kernel(const float* __restrict__ preds,
                                                              const float* __restrict__ q,
                                                              float* __restrict__ err,
                                                              float* __restrict__ g_preds, int ld_gp,
                                                              int ns, int na, int nb, int nc,
                                                              std::conditional_t<OPT, ClassOpt, NoClassOpt> o) {
    __shared__ float pbar[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tb = (int64_t)blockIdx.x * 4 + wave;
    if (tb >= (int64_t)ns * nb) return;
    const int t = (int)(tb / nb), b = (int)(tb % nb);
    const int64_t R = (int64_t)na * nb;
    float mx = -INFINITY;
    for (int c = lane; c < nc; c += 64) {
        float s = 0.f;
        for (int a = 0; a < na; ++a) s += preds[((int64_t)t * R + (int64_t)a * nb + b) * nc + c];
        s = s / (float)na;
        pbar[wave][c] = s;
        mx = fmaxf(mx, s);
    }
    mx = wmax(mx);
    float s = 0.f;
    for (int c = lane; c < nc; c += 64) s += expf(pbar[wave][c] - mx);
    s = wsum(s);
    const float* qb = q + (int64_t)b * nc;
    if constexpr (!OPT) {
        float hn = 0.f, hs = 0.f;  // sum_c Q_c nll_c, sum_c Q_c
        for (int c = lane; c < nc; c += 64) {
            const float qc = qb[c];
            if (qc == 0.f) continue;
            hn += qc * -(pbar[wave][c] - mx - logf(s));
            hs += qc;
        }
        hn = wsum(hn);
        hs = wsum(hs);
        if (lane == 0) err[tb] = hn;
        if (g_preds) {
            const float inv = 1.0f / (float)R;
            for (int c = lane; c < nc; c += 64) {
                const float g = (expf(pbar[wave][c] - mx) / s * hs - qb[c]) * inv;
                for (int a = 0; a < na; ++a)
                    g_preds[((int64_t)t * R + (int64_t)a * nb + b) * ld_gp + c] = g;
            }
        }
    } else {
        __shared__ float wcls[4][1024];
        const float ls = logf(s);
        float wn = 0.f, wt = 0.f;  // sum_c w_c nll_c, sum_c w_c
        float hn = 0.f, hs = 0.f;  // sum_c h_c nll_c, sum_c h_c with h_c = (keep w_c) Q_c, the targets' own share of q
        for (int c = lane; c < nc; c += 64) {
            const float wc = o.w ? o.w[c] : 1.0f;
            wcls[wave][c] = wc;
            const float nll = -(pbar[wave][c] - mx - ls);
            wn = fmaf(wc, nll, wn);
            wt += wc;
            const float qc = qb[c];
            if (qc == 0.f) continue;
            const float hc = o.keep * wc * qc;
            hn += hc * nll;
            hs += hc;
        }
        wn = wsum(wn);
        wt = wsum(wt);
        hn = wsum(hn);
        hs = wsum(hs);
        const float st = o.sw ? o.sw[t] : 1.0f;
        if (lane == 0) {
            float e = hn;
            if (o.eps_nc != 0.f) e = fmaf(o.eps_nc, wn, e);
            err[tb] = st * e;
        }
        if (g_preds) {
            const float sc = st * (1.0f / (float)R);
            const float qs = o.eps_nc != 0.f ? fmaf(o.eps_nc, wt, hs) : hs;  // sum_c q_c
            for (int c = lane; c < nc; c += 64) {
                const float qv = qb[c];
                const float qc = (qv == 0.f ? 0.0f : o.keep * wcls[wave][c] * qv) + o.eps_nc * wcls[wave][c];
                const float g = (expf(pbar[wave][c] - mx) / s * qs - qc) * sc;
                for (int a = 0; a < na; ++a)
                    g_preds[((int64_t)t * R + (int64_t)a * nb + b) * ld_gp + c] = g;
            }
        }
    }
}

// thread per row r: returns by the reference's flip-cumsum-flip of rew * gamma^t, / gamma^t
__global__ __launch_bounds__(256) void loss_returns_kernel(const float* __restrict__ rew,
                                                           const float* __restrict__ values,
                                                           float* __restrict__ ret,
                                                           float* __restrict__ adv,
                                                           double* __restrict__ part, int ns,
                                                           int64_t R, float gamma) {
    __shared__ double sh[2][256];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s[2] = {0.0, 0.0};
    if (r < R) {
        float S = 0.f;
        for (int t = ns - 1; t >= 0; --t) {
            const float gt = powf(gamma, (float)t);
            S += rew[(int64_t)t * R + r] * gt;
            const float rt = S / gt;
            const float ad = rt - values[(int64_t)t * R + r];
            ret[(int64_t)t * R + r] = rt;
            adv[(int64_t)t * R + r] = ad;
            s[0] += (double)ad;
            s[1] += (double)ad * (double)ad;
        }
    }
    block_tree<2>(sh, s);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sh[0][0];
        part[2 * blockIdx.x + 1] = sh[1][0];
    }
}

// one 256-thread block; strided partial sums + fixed-order tree -> deterministic
__global__ __launch_bounds__(256) void loss_stats_kernel(
    const double* __restrict__ part, int nblocks, const float* __restrict__ err, int64_t nerr,
    double* __restrict__ part_err, double* __restrict__ adv_stats, double n) {
    __shared__ double sh[3][256];
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        s[0] += part[2 * i];
        s[1] += part[2 * i + 1];
    }
    for (int64_t i = threadIdx.x; i < nerr; i += 256) s[2] += (double)err[i];
    block_tree<3>(sh, s);
    if (threadIdx.x == 0) {
        adv_stats[0] = n;
        adv_stats[1] = sh[0][0];
        adv_stats[2] = sh[1][0];
        part_err[0] = sh[2][0];
    }
}

// ENT (marl_a2c_loss_entropy_fwd_bwd): the same pass also reads row i of the step distributions [NR][nA] and writes
// H_i = -sum_j p_j log p_j into a third partial and g_probs[i][j] = beta / R * (log p_j + 1) (row_entropy<VEC>).
// ENT = false is the kernel of marl_a2c_loss_fwd_bwd.
template <bool ENT, bool VEC>
__global__ __launch_bounds__(256) void loss_grads_kernel(
    const float* __restrict__ logp, const float* __restrict__ values,
    const float* __restrict__ ret, const float* __restrict__ adv,
    const double* __restrict__ adv_stats, float* __restrict__ g_logp,
    float* __restrict__ g_values, double* __restrict__ part, int64_t NR, int64_t R,
    const float* __restrict__ probs, float* __restrict__ g_probs, double* __restrict__ part_ent, int nA,
    float beta) {
    constexpr int K = ENT ? 3 : 2;
    __shared__ double sh[K][256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s[K] = {};
    if (i < NR) {
        const float advn = standardized(adv[i], adv_stats);
        const float invR = 1.0f / (float)R;
        s[0] = (double)(-logp[i] * advn);
        float dg;
        s[1] = (double)smooth_l1(values[i] - ret[i], &dg);
        if (g_logp) g_logp[i] = -advn * invR;
        if (g_values) g_values[i] = dg * invR;
        if constexpr (ENT) s[2] = (double)(-row_entropy<VEC>(probs + i * nA, g_probs + i * nA, nA, beta * invR));
    }
    block_tree<K>(sh, s);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sh[0][0];
        part[2 * blockIdx.x + 1] = sh[1][0];
        if constexpr (ENT) part_ent[blockIdx.x] = sh[2][0];
    }
}

// scalars = {loss, path.sum(0).mean(), error.mean(), critic.sum(0).mean()} (trainer.py:111,119-122);
// ENT: loss -= beta * mean_{a,b} sum_t H and scalars[4] = mean_{t,a,b} H
template <bool ENT>
__global__ __launch_bounds__(256) void loss_final_kernel(
    const double* __restrict__ part, int nblocks, const double* __restrict__ part_err,
    float* __restrict__ scalars, int ns, int nb, int64_t R, const double* __restrict__ part_ent, float beta) {
    constexpr int K = ENT ? 3 : 2;
    __shared__ double sh[K][256];
    double s[K] = {};
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        s[0] += part[2 * i];
        s[1] += part[2 * i + 1];
        if constexpr (ENT) s[2] += part_ent[i];
    }
    block_tree<K>(sh, s);
    if (threadIdx.x == 0) {
        const double path = sh[0][0] / (double)R, critic = sh[1][0] / (double)R;
        const double esum = part_err[0];
        double loss = path + esum / (double)nb + critic;
        if constexpr (ENT) {
            const double h = sh[2][0];
            loss -= (double)beta * (h / (double)R);
            scalars[4] = (float)(h / ((double)R * ns));
        }
        scalars[0] = (float)loss;
        scalars[1] = (float)path;
        scalars[2] = (float)(esum / ((double)ns * nb));
        scalars[3] = (float)critic;
    }
}

// the one place that picks the instance of the rewards / vote-error kernel: the plain one unless marl_class_loss
// installed options (the rewards: unless it installed weight_rewards with class weights)
static ClassOpt class_opt(const LossCommon& a) {
    return ClassOpt{a.cls_w, a.cls_sw, 1.0f - a.cls_eps, a.cls_eps / (float)a.nc};
}

static void launch_rewards(const LossCommon& a, float* rew, hipStream_t st) {
    const int64_t NR = (int64_t)a.na * a.nb * a.ns;
    const float rnd = (float)log((double)a.nc);
    if (a.soft_q) {  // (marl_soft_targets: the same launch, its soft instance)
        if (a.cls && a.cls_wrew && a.cls_w)
            hipLaunchKernelGGL(loss_rewards_soft_kernel<true>, dim3((unsigned)cdiv(NR, 4)), dim3(256), 0, st, a.preds,
                               a.soft_q, rew, NR, a.nb, a.nc, rnd, class_opt(a));
        else
            hipLaunchKernelGGL(loss_rewards_soft_kernel<false>, dim3((unsigned)cdiv(NR, 4)), dim3(256), 0, st, a.preds,
                               a.soft_q, rew, NR, a.nb, a.nc, rnd, NoClassOpt{});
        return;
    }
    if (a.cls && a.cls_wrew && a.cls_w)
        hipLaunchKernelGGL(loss_rewards_kernel<true>, dim3((unsigned)cdiv(NR, 4)), dim3(256), 0, st, a.preds, a.y, rew,
                           NR, a.nb, a.nc, rnd, class_opt(a));
    else
        hipLaunchKernelGGL(loss_rewards_kernel<false>, dim3((unsigned)cdiv(NR, 4)), dim3(256), 0, st, a.preds, a.y,
                           rew, NR, a.nb, a.nc, rnd, NoClassOpt{});
}

static void launch_error(const LossGradArgs& a, float* err, hipStream_t st) {
    const dim3 grid((unsigned)cdiv((int64_t)a.ns * a.nb, 4));
    if (a.soft_q) {
        if (a.cls)
            hipLaunchKernelGGL(loss_error_soft_kernel<true>, grid, dim3(256), 0, st, a.preds, a.soft_q, err, a.g_preds,
                               a.ld_gp, a.ns, a.na, a.nb, a.nc, class_opt(a));
        else
            hipLaunchKernelGGL(loss_error_soft_kernel<false>, grid, dim3(256), 0, st, a.preds, a.soft_q, err, a.g_preds,
                               a.ld_gp, a.ns, a.na, a.nb, a.nc, NoClassOpt{});
        return;
    }
    if (a.cls)
        hipLaunchKernelGGL(loss_error_kernel<true>, grid, dim3(256), 0, st, a.preds, a.y, err, a.g_preds, a.ld_gp, a.ns,
                           a.na, a.nb, a.nc, class_opt(a));
    else
        hipLaunchKernelGGL(loss_error_kernel<false>, grid, dim3(256), 0, st, a.preds, a.y, err, a.g_preds, a.ld_gp,
                           a.ns, a.na, a.nb, a.nc, NoClassOpt{});
}

int launch_loss(const LossArgs& a, hipStream_t st) {
    if (a.nc > 1024) {
        set_error("nb_class %d > 1024 unsupported by the loss kernel", a.nc);
        return MARL_ELIMIT;
    }
    const int64_t R = (int64_t)a.na * a.nb, NR = R * a.ns;
    LossLayout L = loss_layout(a.scratch, a.ns, a.na, a.nb);
    double* stats = reinterpret_cast<double*>(a.adv_stats);
    if (a.phase == 0 || a.phase == 1) {
        launch_rewards(a, L.rew, st);
        MARL_LAUNCH_CHECK();
        launch_error(a, L.err, st);
        MARL_LAUNCH_CHECK();
        hipLaunchKernelGGL(loss_returns_kernel, dim3((unsigned)L.blocksC), dim3(256), 0, st, L.rew,
                           a.values, L.ret, L.adv, L.part_adv, a.ns, R, a.gamma);
        MARL_LAUNCH_CHECK();
        hipLaunchKernelGGL(loss_stats_kernel, dim3(1), dim3(256), 0, st, L.part_adv, L.blocksC,
                           L.err, (int64_t)a.ns * a.nb, L.part_err, stats, (double)NR);
        MARL_LAUNCH_CHECK();
    }
    if (a.phase == 0 || a.phase == 2) {
        double* part_ent = extra_partials(L, 1);  // (not touched without the bonus)
        with_grads_instance(a, [&](auto ent, auto vec) {
            hipLaunchKernelGGL((loss_grads_kernel<decltype(ent)::value, decltype(vec)::value>), dim3((unsigned)L.blocksE),
                               dim3(256), 0, st, a.logp, a.values, L.ret, L.adv, stats, a.g_logp, a.g_values,
                               L.part_loss, NR, R, a.probs, a.g_probs, part_ent, a.n_act, a.entropy_coef);
        });
        MARL_LAUNCH_CHECK();
        if (a.probs)
            hipLaunchKernelGGL(loss_final_kernel<true>, dim3(1), dim3(256), 0, st, L.part_loss, L.blocksE, L.part_err,
                               a.scalars, a.ns, a.nb, R, part_ent, a.entropy_coef);
        else
            hipLaunchKernelGGL(loss_final_kernel<false>, dim3(1), dim3(256), 0, st, L.part_loss, L.blocksE, L.part_err,
                               a.scalars, a.ns, a.nb, R, nullptr, 0.f);
        MARL_LAUNCH_CHECK();
    }
    return MARL_OK;
}

// ---------------------------------------------------------------------------
// PPO on the fused path (marl_advantages, marl_ppo_loss_fwd_bwd, marl_grad_clip).  Same conventions: fp64 partials,
// fixed-order trees, no float atomics.
// ---------------------------------------------------------------------------

// thread per row r, t from Ns - 1 down: delta_t = r_t + gamma V_{t+1} - V_t (V_Ns = 0: the reference's returns have no
// bootstrap), A_t = delta_t + gamma lam A_{t+1}, ret_t = A_t + V_t; partials of sum A and sum A^2 as in
// loss_returns_kernel (which stays the lam == 1 path: its flip-cumsum arithmetic is what the A2C loss standardises)
__global__ __launch_bounds__(256) void loss_gae_kernel(const float* __restrict__ rew,
                                                       const float* __restrict__ values,
                                                       float* __restrict__ ret, float* __restrict__ adv,
                                                       double* __restrict__ part, int ns, int64_t R,
                                                       float gamma, float lam) {
    __shared__ double sh[2][256];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s[2] = {0.0, 0.0};
    if (r < R) {
        const float gl = gamma * lam;
        float A = 0.f, vnext = 0.f;
        for (int t = ns - 1; t >= 0; --t) {
            const int64_t i = (int64_t)t * R + r;
            const float v = values[i];
            const float delta = rew[i] + gamma * vnext - v;
            A = delta + gl * A;
            vnext = v;
            ret[i] = A + v;
            adv[i] = A;
            s[0] += (double)A;
            s[1] += (double)A * (double)A;
        }
    }
    block_tree<2>(sh, s);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sh[0][0];
        part[2 * blockIdx.x + 1] = sh[1][0];
    }
}

__global__ __launch_bounds__(256) void loss_standardize_kernel(const float* __restrict__ adv,
                                                               const double* __restrict__ adv_stats,
                                                               float* __restrict__ advn, int64_t NR) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= NR) return;
    advn[i] = standardized(adv[i], adv_stats);
}

int launch_advantages(const AdvArgs& a, hipStream_t st) {
    const int64_t R = (int64_t)a.na * a.nb, NR = R * a.ns;
    LossLayout L = loss_layout(a.scratch, a.ns, a.na, a.nb);
    double* stats = reinterpret_cast<double*>(a.adv_stats);
    if (a.phase == 0 || a.phase == 1) {
        launch_rewards(a, L.rew, st);
        MARL_LAUNCH_CHECK();
        if (a.lam == 1.0f)
            hipLaunchKernelGGL(loss_returns_kernel, dim3((unsigned)L.blocksC), dim3(256), 0, st, L.rew, a.values,
                               a.ret, L.adv, L.part_adv, a.ns, R, a.gamma);
        else
            hipLaunchKernelGGL(loss_gae_kernel, dim3((unsigned)L.blocksC), dim3(256), 0, st, L.rew, a.values, a.ret,
                               L.adv, L.part_adv, a.ns, R, a.gamma, a.lam);
        MARL_LAUNCH_CHECK();
        // (no vote error here: nerr = 0, the slot behind the loss partials receives a zero nobody reads)
        hipLaunchKernelGGL(loss_stats_kernel, dim3(1), dim3(256), 0, st, L.part_adv, L.blocksC, L.err, (int64_t)0,
                           L.part_err, stats, (double)NR);
        MARL_LAUNCH_CHECK();
    }
    if (a.phase == 0 || a.phase == 2) {
        hipLaunchKernelGGL(loss_standardize_kernel, dim3((unsigned)L.blocksE), dim3(256), 0, st, L.adv, stats,
                           a.advn, NR);
        MARL_LAUNCH_CHECK();
    }
    return MARL_OK;
}

// one thread per (t, r): rho = exp(logp - old_logp); surrogate -min(rho A, clamp(rho, 1 - eps, 1 + eps) A) and
// g_logp = -A rho / R where the unclipped term is the active one, 0 where the clip is (A > 0 and rho > 1 + eps, or
// A < 0 and rho < 1 - eps).  With old_logp == logp bit for bit rho is exactly 1 and (-A * rho) * (1 / R) is
// loss_grads_kernel's -advn * invR, bit for bit; the critic term and g_values are that kernel's smooth_l1.
// part[2 i] / [2 i + 1] = surrogate / critic, extra[3 i ..] = entropy / old_logp - logp / clipped count.
// ENT / VEC: as in loss_grads_kernel.
template <bool ENT, bool VEC>
__global__ __launch_bounds__(256) void ppo_grads_kernel(
    const float* __restrict__ logp, const float* __restrict__ old_logp, const float* __restrict__ values,
    const float* __restrict__ ret, const float* __restrict__ advn_in, float clip_eps, float* __restrict__ g_logp,
    float* __restrict__ g_values, double* __restrict__ part, double* __restrict__ extra, int64_t NR, int64_t R,
    const float* __restrict__ probs, float* __restrict__ g_probs, int nA, float beta) {
    __shared__ double sh[5][256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < NR) {
        const float advn = advn_in[i];
        const float invR = 1.0f / (float)R;
        const float lp = logp[i], olp = old_logp[i];
        const float rho = expf(lp - olp);
        const float lo = 1.0f - clip_eps, hi = 1.0f + clip_eps;
        const bool clipped = (advn > 0.f && rho > hi) || (advn < 0.f && rho < lo);
        const float rc = fminf(fmaxf(rho, lo), hi);
        s[0] = (double)(-(clipped ? rc : rho) * advn);
        float dg;
        s[1] = (double)smooth_l1(values[i] - ret[i], &dg);
        s[3] = (double)(olp - lp);
        s[4] = clipped ? 1.0 : 0.0;
        if (g_logp) g_logp[i] = clipped ? 0.f : (-advn * rho) * invR;
        if (g_values) g_values[i] = dg * invR;
        if (ENT) s[2] = (double)(-row_entropy<VEC>(probs + i * nA, g_probs + i * nA, nA, beta * invR));
    }
    block_tree<5>(sh, s);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = sh[0][0];
        part[2 * blockIdx.x + 1] = sh[1][0];
        extra[3 * blockIdx.x] = sh[2][0];
        extra[3 * blockIdx.x + 1] = sh[3][0];
        extra[3 * blockIdx.x + 2] = sh[4][0];
    }
}

// scalars = {loss, surrogate.sum(0).mean(), error.mean(), critic.sum(0).mean(), mean entropy (0 without a bonus),
// approx_kl = mean(old_logp - logp), clip_frac}; the vote error [nerr] is summed here (strided, then the tree)
__global__ __launch_bounds__(256) void ppo_final_kernel(const double* __restrict__ part,
                                                        const double* __restrict__ extra, int nblocks,
                                                        const float* __restrict__ err, int64_t nerr,
                                                        float* __restrict__ scalars, int ns, int nb, int64_t R,
                                                        float beta) {
    __shared__ double sh[6][256];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        s[0] += part[2 * i];
        s[1] += part[2 * i + 1];
        s[2] += extra[3 * i];
        s[3] += extra[3 * i + 1];
        s[4] += extra[3 * i + 2];
    }
    for (int64_t i = threadIdx.x; i < nerr; i += 256) s[5] += (double)err[i];
    block_tree<6>(sh, s);
    if (threadIdx.x == 0) {
        const double NR = (double)R * ns;
        const double surr = sh[0][0] / (double)R, critic = sh[1][0] / (double)R, h = sh[2][0];
        const double esum = sh[5][0];
        scalars[0] = (float)(surr + esum / (double)nb + critic - (double)beta * (h / (double)R));
        scalars[1] = (float)surr;
        scalars[2] = (float)(esum / ((double)ns * nb));
        scalars[3] = (float)critic;
        scalars[4] = (float)(h / NR);
        scalars[5] = (float)(sh[3][0] / NR);
        scalars[6] = (float)(sh[4][0] / NR);
    }
}

int launch_ppo_loss(const PpoArgs& a, hipStream_t st) {
    if (a.nc > 1024) {
        set_error("nb_class %d > 1024 unsupported by the loss kernel", a.nc);
        return MARL_ELIMIT;
    }
    const int64_t R = (int64_t)a.na * a.nb, NR = R * a.ns, nerr = (int64_t)a.ns * a.nb;
    LossLayout L = loss_layout(a.scratch, a.ns, a.na, a.nb);
    double* extra = extra_partials(L, 3);  // entropy / old_logp - logp / clipped count
    launch_error(a, L.err, st);
    MARL_LAUNCH_CHECK();
    with_grads_instance(a, [&](auto ent, auto vec) {
        hipLaunchKernelGGL((ppo_grads_kernel<decltype(ent)::value, decltype(vec)::value>), dim3((unsigned)L.blocksE),
                           dim3(256), 0, st, a.logp, a.old_logp, a.values, a.ret, a.advn, a.clip_eps, a.g_logp,
                           a.g_values, L.part_loss, extra, NR, R, a.probs, a.g_probs, a.n_act, a.entropy_coef);
    });
    MARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ppo_final_kernel, dim3(1), dim3(256), 0, st, L.part_loss, extra, L.blocksE, L.err, nerr,
                       a.scalars, a.ns, a.nb, R, a.probs ? a.entropy_coef : 0.f);
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}

// ---------------------------------------------------------------------------
// global-norm gradient clipping (th.nn.utils.clip_grad_norm_): partial sums of g^2, then finalise + scale
// ---------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void clip_partials_kernel(const float* __restrict__ g, int64_t n,
                                                            double* __restrict__ part) {
    __shared__ double sh[1][256];
    double s[1] = {0.0};
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        const float4* g4 = reinterpret_cast<const float4*>(g);
        for (int64_t i = tid; i < n / 4; i += stride) {
            const float4 v = g4[i];
            s[0] += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
        }
    } else {
        for (int64_t i = tid; i < n; i += stride) s[0] += (double)g[i] * g[i];
    }
    block_tree<1>(sh, s);
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0][0];
}

// every block re-sums the (<= MARL_GRAD_CLIP_BLOCKS) partials in the same order, so all of them scale by the same
// factor.  grad_scale (1 / world_size after an all-reduce sum) comes first: norm = || grad_scale g ||, and
// g *= grad_scale * min(1, max_norm / (norm + 1e-6)); a factor of exactly 1 writes nothing: every bit stays
template <bool VEC>
__global__ __launch_bounds__(256) void clip_scale_kernel(float* __restrict__ g, int64_t n,
                                                         const double* __restrict__ part, int nparts,
                                                         float max_norm, float grad_scale,
                                                         float* __restrict__ norm_out) {
    __shared__ double sh[1][256];
    double s[1] = {0.0};
    for (int i = threadIdx.x; i < nparts; i += 256) s[0] += part[i];
    block_tree<1>(sh, s);
    const double norm = (double)grad_scale * sqrt(sh[0][0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = (float)norm;
    const double cd = (double)max_norm / (norm + 1e-6);
    const float coef = (float)((double)grad_scale * (cd < 1.0 ? cd : 1.0));
    if (coef == 1.0f) return;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        float4* g4 = reinterpret_cast<float4*>(g);
        for (int64_t i = tid; i < n / 4; i += stride) {
            float4 v = g4[i];
            v.x *= coef;
            v.y *= coef;
            v.z *= coef;
            v.w *= coef;
            g4[i] = v;
        }
    } else {
        for (int64_t i = tid; i < n; i += stride) g[i] *= coef;
    }
}

int launch_grad_clip(float* g, int64_t n, float max_norm, float grad_scale, float* norm_out, double* part,
                     hipStream_t st) {
    const bool vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    int64_t gx = cdiv(vec ? n / 4 : n, 256);
    if (gx > MARL_GRAD_CLIP_BLOCKS) gx = MARL_GRAD_CLIP_BLOCKS;
    if (gx < 1) gx = 1;
    if (vec) {
        hipLaunchKernelGGL(clip_partials_kernel<true>, dim3((unsigned)gx), dim3(256), 0, st, g, n, part);
        MARL_LAUNCH_CHECK();
        hipLaunchKernelGGL(clip_scale_kernel<true>, dim3((unsigned)gx), dim3(256), 0, st, g, n, part, (int)gx,
                           max_norm, grad_scale, norm_out);
    } else {
        hipLaunchKernelGGL(clip_partials_kernel<false>, dim3((unsigned)gx), dim3(256), 0, st, g, n, part);
        MARL_LAUNCH_CHECK();
        hipLaunchKernelGGL(clip_scale_kernel<false>, dim3((unsigned)gx), dim3(256), 0, st, g, n, part, (int)gx,
                           max_norm, grad_scale, norm_out);
    }
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}

}  // namespace marl
