// marl_episode_report (include/marl_hip_report.h): the episode's step_preds [Ns,Na,Nb,nC] reduced to the report - vote
// accuracy, top-k, NLL, agreement and every agent's accuracy per step, confusion matrix and calibration of the last
// step, early-exit statistics - in two launches, store-and-sum (as comm_grad_kernel / comm_grad_sum_kernel).
//
// Row pass (report_row_kernel): one workgroup per image, one wave per step (waves beyond 16, or beyond what the vote
// buffers leave of the LDS, loop).  A wave reads the Na rows of its (step, image) once, 8 agents' loads in flight: a
// lane owns class lane + 64 k; the running sum over the agents is the vote (ascending a, then / Na: the arithmetic of
// loss_error_kernel), and the same values give every agent's argmax - a wave maximum, the lowest lane that holds it,
// kept by lane a for agent a across the class passes.  The vote of a pass is kept in LDS by the lane that formed it
// and read back by that lane only, so no barrier sits inside the step loop.  Lane 0 leaves a 24-byte step record in
// the scratch; the workgroup then knows whether its image is skipped and scans the steps' confidences, which it kept
// in LDS, for the exit thresholds.  With accumulate == 0 this pass also clears the confusion matrix, the one field
// the sum pass fills with (integer) atomics.
//
// Sum pass (report_sum_kernel): every other field has ONE owner that overwrites or adds to it with plain stores.  A
// workgroup per step folds that step's records (counts through LDS integer atomics - exact in any order - and the NLL
// as per-thread fp64 sums over ascending images, then a fixed tree), one workgroup folds the per-image words (n,
// skipped, exits), one wave per calibration bin folds the last step's confidences.  No float atomics.
#include "common.h"

#include <cmath>

#include "../../include/marl_hip_report.h"

namespace marl {
namespace {

constexpr int kRowMaxWaves = 16;
constexpr int kRowVoteBytes = 48 * 1024;  // LDS the vote buffers of a row workgroup may take
constexpr int kSumThreads = 256;
constexpr int kChunk = 8;  // agents whose loads fly together (16 measured no faster at Na = 16, at 15 more VGPRs)

struct StepRec {
    float nll, conf;
    int32_t pred;
    int32_t rank_agree;  // min(rank, topk) | agree << 8
    uint64_t hits;       // bit a: agent a's own argmax is the label
};
static_assert(sizeof(StepRec) == 24, "step record layout");

struct ReportArgs {
    const float* preds;
    const int64_t* y;
    int64_t* report;
    StepRec* recs;     // [ns][nb]
    int32_t* status;   // [nb]: 1 = skipped
    int32_t* exits;    // [nb][MARL_REPORT_MAX_EXITS]: exit step * 2 + hit
    int ns, na, nb, nc, topk, bins, n_exit, accumulate;
    int ncp;           // floats of one wave's vote buffer
    int64_t off[MARL_REPORT_LAYOUT_SLOTS];
    float thr[MARL_REPORT_MAX_EXITS];
};

// Maximum over the 64 lanes on the VALU (the DPP steps of wave_sum, common.h; a lane without a source keeps its own
// value): a wave takes one per agent and class pass, and six dependent LDS-pipe shuffles apiece were most of the row
// pass's time.  A maximum is exact in any order.  Call with all 64 lanes active; the result is wave-uniform.
__device__ __forceinline__ float rep_wmax(float v) {
    int x = __float_as_int(v);
#define MARL_DPP_MAX(ctrl, rmask)                                \
    x = __float_as_int(fmaxf(__int_as_float(x),                  \
                             __int_as_float(__builtin_amdgcn_update_dpp(x, x, ctrl, rmask, 0xf, false))))
    MARL_DPP_MAX(0x111, 0xf);  // row_shr:1
    MARL_DPP_MAX(0x112, 0xf);  // row_shr:2
    MARL_DPP_MAX(0x114, 0xf);  // row_shr:4
    MARL_DPP_MAX(0x118, 0xf);  // row_shr:8   -> lane 15 of each row holds the row's maximum
    MARL_DPP_MAX(0x142, 0xa);  // row_bcast:15 into rows 1 and 3
    MARL_DPP_MAX(0x143, 0xc);  // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's
#undef MARL_DPP_MAX
    return __int_as_float(__builtin_amdgcn_readlane(x, 63));
}
__device__ __forceinline__ float rep_wsum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double rep_wsum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int rep_wsum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int first_lane(uint64_t mask) { return mask ? __ffsll((long long)mask) - 1 : 0; }

__global__ void __launch_bounds__(kRowMaxWaves * 64) report_row_kernel(const ReportArgs A) {
    extern __shared__ __align__(16) float smem[];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const int ns = A.ns, na = A.na, nb = A.nb, nc = A.nc;
    const int b = blockIdx.x;
    float* s_conf = smem + (size_t)nwaves * A.ncp;    // [ns]
    int* s_hit = reinterpret_cast<int*>(s_conf + ns);  // [ns]
    if (tid == 0) s_bad = 0;
    if (!A.accumulate) {
        int64_t* cm = A.report + A.off[MARL_REPORT_CONFUSION];
        const int64_t cells = (int64_t)nc * nc, stride = (int64_t)gridDim.x * blockDim.x;
        for (int64_t i = (int64_t)b * blockDim.x + tid; i < cells; i += stride) cm[i] = 0;
    }
    __syncthreads();
    const int64_t y64 = A.y[b];
    const bool y_ok = y64 >= 0 && y64 < nc;
    const int yb = y_ok ? (int)y64 : 0;
    const int64_t astride = (int64_t)nb * nc;
    float* z = smem + (size_t)wave * A.ncp;
    for (int t = wave; t < ns; t += nwaves) {
        bool bad = false;
        float best = -INFINITY, zy_l = 0.f, mx = -INFINITY;
        int bidx = 0, pred = 0;
        for (int c0 = 0; c0 < nc; c0 += 64) {
            const int c = c0 + lane;
            const bool live = c < nc;
            const float* p = A.preds + ((int64_t)t * na * nb + b) * nc + (live ? c : nc - 1);
            float s = 0.f;
            for (int a0 = 0; a0 < na; a0 += kChunk) {
                float v[kChunk];
#pragma unroll
                for (int j = 0; j < kChunk; ++j) v[j] = p[(a0 + j < na ? a0 + j : na - 1) * astride];
#pragma unroll
                for (int j = 0; j < kChunk; ++j) {
                    if (a0 + j < na) {  // (the same in every lane)
                        bad |= live && !(fabsf(v[j]) < INFINITY);
                        s += v[j];
                        const float x = live ? v[j] : -INFINITY;
                        const float m = rep_wmax(x);
                        const int idx = c0 + first_lane(__ballot(x == m));
                        if (lane == a0 + j && (c0 == 0 || m > best)) {
                            best = m;
                            bidx = idx;
                        }
                    }
                }
            }
            s = s / (float)na;
            if (live) z[c] = s;
            if (c == yb) zy_l = s;
            const float x = live ? s : -INFINITY;
            const float m = rep_wmax(x);
            if (c0 == 0 || m > mx) {
                mx = m;
                pred = c0 + first_lane(__ballot(x == m));
            }
        }
        const float zy = __shfl(zy_l, yb & 63);  // (the lane that formed z[yb] in pass yb / 64 kept it)
        float se = 0.f;
        int rank = 0;
        for (int c0 = 0; c0 < nc; c0 += 64) {
            const int c = c0 + lane;
            const bool live = c < nc;
            const float zc = live ? z[c] : 0.f;
            if (live) se += expf(zc - mx);
            rank += __popcll(__ballot(live && (zc > zy || (c < yb && zc == zy))));
        }
        se = rep_wsum(se);
        const float nll = -(zy - mx - logf(se));
        const float conf = 1.0f / se;
        const uint64_t hits = __ballot(lane < na && bidx == yb);
        const int agree = __popcll(__ballot(lane < na && bidx == pred));
        const bool any_bad = __ballot(bad) != 0;
        if (lane == 0) {
            StepRec r;
            r.nll = nll;
            r.conf = conf;
            r.pred = pred;
            r.rank_agree = (rank < A.topk ? rank : A.topk) | (agree << 8);
            r.hits = hits;
            A.recs[(int64_t)t * nb + b] = r;
            s_conf[t] = conf;
            s_hit[t] = pred == yb;
            if (any_bad) atomicOr(&s_bad, 1);
        }
    }
    __syncthreads();
    if (tid == 0) A.status[b] = (s_bad || !y_ok) ? 1 : 0;
    if (tid < A.n_exit) {
        float tau = 2.0f;  // (selected, not indexed: the argument block is read at constant offsets only)
#pragma unroll
        for (int j = 0; j < MARL_REPORT_MAX_EXITS; ++j) tau = tid == j ? A.thr[j] : tau;
        int e = ns - 1;
        for (int t = 0; t < ns; ++t) {
            if (s_conf[t] >= tau) {
                e = t;
                break;
            }
        }
        A.exits[(int64_t)b * MARL_REPORT_MAX_EXITS + tid] = e * 2 + s_hit[e];
    }
}

__device__ __forceinline__ void put_i64(const ReportArgs& A, int64_t word, int64_t v) {
    A.report[word] = A.accumulate ? A.report[word] + v : v;
}
__device__ __forceinline__ void put_f64(const ReportArgs& A, int64_t word, double v) {
    double* d = reinterpret_cast<double*>(A.report) + word;
    *d = A.accumulate ? *d + v : v;
}

// LDS counters of a step workgroup: vote_hit | rank_hist [topk + 1] | agree | agent_hit [na]
constexpr int kStepCounters = 1 + (MARL_REPORT_MAX_TOPK + 1) + 1 + MARL_REPORT_MAX_AGENTS;
// ... and of the image workgroup: n | skipped | exit_hit [n_exit] | exit_hist [n_exit][ns]
constexpr int kImageCounters = 2 + MARL_REPORT_MAX_EXITS + MARL_REPORT_MAX_EXITS * MARL_REPORT_MAX_STEPS;
static_assert(kStepCounters <= kImageCounters, "both roles count in one LDS array");

__global__ void __launch_bounds__(kSumThreads) report_sum_kernel(const ReportArgs A) {
    __shared__ int s_cnt[kImageCounters];
    __shared__ double s_red[kSumThreads];
    const int tid = threadIdx.x, ns = A.ns, na = A.na, nb = A.nb, nc = A.nc, topk = A.topk;
    const int blk = blockIdx.x;
    if (blk < ns) {  // ---- the fields of step blk
        const int t = blk;
        const int o_rank = 1, o_agree = 2 + topk, o_agent = 3 + topk, ncnt = 3 + topk + na;
        for (int i = tid; i < ncnt; i += kSumThreads) s_cnt[i] = 0;
        __syncthreads();
        const bool last = t == ns - 1;
        int64_t* cm = A.report + A.off[MARL_REPORT_CONFUSION];
        double acc = 0.0;
        for (int b = tid; b < nb; b += kSumThreads) {
            if (A.status[b]) continue;
            const StepRec r = A.recs[(int64_t)t * nb + b];
            const int yb = (int)A.y[b];  // (in [0, nc): the row pass checked it)
            if (r.pred == yb) atomicAdd(&s_cnt[0], 1);
            atomicAdd(&s_cnt[o_rank + (r.rank_agree & 0xff)], 1);
            atomicAdd(&s_cnt[o_agree], r.rank_agree >> 8);
            uint64_t h = r.hits;
            while (h) {
                atomicAdd(&s_cnt[o_agent + __ffsll((long long)h) - 1], 1);
                h &= h - 1;
            }
            acc += (double)r.nll;
            if (last && (unsigned)r.pred < (unsigned)nc && (unsigned)yb < (unsigned)nc)
                atomicAdd(reinterpret_cast<unsigned long long*>(cm + (int64_t)yb * nc + r.pred), 1ull);
        }
        s_red[tid] = acc;
        __syncthreads();
        for (int s = kSumThreads / 2; s > 0; s >>= 1) {
            if (tid < s) s_red[tid] += s_red[tid + s];
            __syncthreads();
        }
        if (tid == 0) {
            put_i64(A, A.off[MARL_REPORT_VOTE_HIT] + t, s_cnt[0]);
            put_i64(A, A.off[MARL_REPORT_AGREE] + t, s_cnt[o_agree]);
            put_f64(A, A.off[MARL_REPORT_NLL_SUM] + t, s_red[0]);
        }
        for (int i = tid; i <= topk; i += kSumThreads)
            put_i64(A, A.off[MARL_REPORT_RANK_HIST] + (int64_t)t * (topk + 1) + i, s_cnt[o_rank + i]);
        for (int i = tid; i < na; i += kSumThreads)
            put_i64(A, A.off[MARL_REPORT_AGENT_HIT] + (int64_t)t * na + i, s_cnt[o_agent + i]);
    } else if (blk == ns) {  // ---- the per-image words: n, skipped, exits
        const int ne = A.n_exit, o_hit = 2, o_hist = 2 + ne, ncnt = 2 + ne + ne * ns;
        for (int i = tid; i < ncnt; i += kSumThreads) s_cnt[i] = 0;
        __syncthreads();
        for (int b = tid; b < nb; b += kSumThreads) {
            if (A.status[b]) {
                atomicAdd(&s_cnt[1], 1);
                continue;
            }
            atomicAdd(&s_cnt[0], 1);
            for (int j = 0; j < ne; ++j) {
                const int w = A.exits[(int64_t)b * MARL_REPORT_MAX_EXITS + j];
                const int e = w >> 1;
                if ((unsigned)e < (unsigned)ns) atomicAdd(&s_cnt[o_hist + j * ns + e], 1);
                if (w & 1) atomicAdd(&s_cnt[o_hit + j], 1);
            }
        }
        __syncthreads();
        if (tid == 0) {
            put_i64(A, A.off[MARL_REPORT_N], s_cnt[0]);
            put_i64(A, A.off[MARL_REPORT_SKIPPED], s_cnt[1]);
        }
        for (int i = tid; i < ne; i += kSumThreads) put_i64(A, A.off[MARL_REPORT_EXIT_HIT] + i, s_cnt[o_hit + i]);
        for (int i = tid; i < ne * ns; i += kSumThreads)
            put_i64(A, A.off[MARL_REPORT_EXIT_HIST] + i, s_cnt[o_hist + i]);
    } else {  // ---- one wave per calibration bin, over the last step's records
        const int lane = tid & 63;
        const int k = (blk - ns - 1) * (kSumThreads / 64) + (tid >> 6);
        if (k >= A.bins) return;
        int cnt = 0, hit = 0;
        double sum = 0.0;
        for (int b = lane; b < nb; b += 64) {
            if (A.status[b]) continue;
            const StepRec r = A.recs[(int64_t)(ns - 1) * nb + b];
            int bin = (int)(r.conf * (float)A.bins);
            bin = bin < A.bins - 1 ? bin : A.bins - 1;
            if (bin != k) continue;
            cnt += 1;
            hit += r.pred == (int)A.y[b];
            sum += (double)r.conf;
        }
        cnt = rep_wsum(cnt);
        hit = rep_wsum(hit);
        sum = rep_wsum(sum);
        if (lane == 0) {
            put_i64(A, A.off[MARL_REPORT_CAL_COUNT] + k, cnt);
            put_i64(A, A.off[MARL_REPORT_CAL_HIT] + k, hit);
            put_f64(A, A.off[MARL_REPORT_CAL_CONF] + k, sum);
        }
    }
}

// MARL_OK, or the code with the message set
int check_sizes(int ns, int na, int nc, int topk, int bins, int n_exit) {
    if (ns < 1 || na < 1 || nc < 1 || topk < 1 || bins < 1 || n_exit < 0) {
        set_error("episode_report: ns %d, na %d, nc %d, topk %d, bins %d must be >= 1 and n_exit %d >= 0", ns, na, nc,
                  topk, bins, n_exit);
        return MARL_EINVAL;
    }
    if (ns > MARL_REPORT_MAX_STEPS || na > MARL_REPORT_MAX_AGENTS || nc > MARL_REPORT_MAX_CLASSES ||
        topk > MARL_REPORT_MAX_TOPK || bins > MARL_REPORT_MAX_BINS || n_exit > MARL_REPORT_MAX_EXITS) {
        set_error("episode_report: ns %d (max %d), na %d (%d), nc %d (%d), topk %d (%d), bins %d (%d), n_exit %d (%d)",
                  ns, MARL_REPORT_MAX_STEPS, na, MARL_REPORT_MAX_AGENTS, nc, MARL_REPORT_MAX_CLASSES, topk,
                  MARL_REPORT_MAX_TOPK, bins, MARL_REPORT_MAX_BINS, n_exit, MARL_REPORT_MAX_EXITS);
        return MARL_ELIMIT;
    }
    return MARL_OK;
}

void fill_layout(int ns, int na, int nc, int topk, int bins, int n_exit, int64_t* out) {
    int64_t at = 0;
    auto field = [&](int slot, int64_t words) {
        out[slot] = at;
        at += words;
    };
    field(MARL_REPORT_N, 1);
    field(MARL_REPORT_SKIPPED, 1);
    field(MARL_REPORT_VOTE_HIT, ns);
    field(MARL_REPORT_RANK_HIST, (int64_t)ns * (topk + 1));
    field(MARL_REPORT_AGENT_HIT, (int64_t)ns * na);
    field(MARL_REPORT_AGREE, ns);
    field(MARL_REPORT_CONFUSION, (int64_t)nc * nc);
    field(MARL_REPORT_CAL_COUNT, bins);
    field(MARL_REPORT_CAL_HIT, bins);
    field(MARL_REPORT_EXIT_HIST, (int64_t)n_exit * ns);
    field(MARL_REPORT_EXIT_HIT, n_exit);
    field(MARL_REPORT_NLL_SUM, ns);
    field(MARL_REPORT_CAL_CONF, bins);
    out[MARL_REPORT_WORDS] = at;
}

inline size_t recs_bytes(int ns, int nb) { return (size_t)ns * nb * sizeof(StepRec); }
inline size_t scratch_need(int ns, int nb) {
    return recs_bytes(ns, nb) + (size_t)nb * 4 * (1 + MARL_REPORT_MAX_EXITS);
}

}  // namespace
}  // namespace marl

using namespace marl;

extern "C" int marl_report_layout(int ns, int na, int nc, int topk, int bins, int n_exit, int64_t* out) {
    if (!out) {
        set_error("report_layout: null output");
        return MARL_EINVAL;
    }
    MARL_TRY(check_sizes(ns, na, nc, topk, bins, n_exit));
    fill_layout(ns, na, nc, topk, bins, n_exit, out);
    return MARL_OK;
}

extern "C" size_t marl_report_scratch_bytes(int ns, int na, int nb, int nc, int topk, int bins, int n_exit) {
    if (nb < 1 || check_sizes(ns, na, nc, topk, bins, n_exit) != MARL_OK) return 0;
    return scratch_need(ns, nb);
}

extern "C" int marl_episode_report(const float* step_preds, const int64_t* y, int ns, int na, int nb, int nc, int topk,
                                   int bins, const float* exit_thresholds, int n_exit, int accumulate,
                                   void* report_dev, size_t report_bytes, void* scratch, size_t scratch_bytes,
                                   void* stream) {
    if (!step_preds || !y || !report_dev || !scratch || (n_exit > 0 && !exit_thresholds)) {
        set_error("episode_report: null pointer");
        return MARL_EINVAL;
    }
    if ((reinterpret_cast<uintptr_t>(report_dev) & 7) != 0 || (reinterpret_cast<uintptr_t>(scratch) & 7) != 0 ||
        (reinterpret_cast<uintptr_t>(step_preds) & 3) != 0 || (reinterpret_cast<uintptr_t>(y) & 7) != 0) {
        set_error("episode_report: the report and the scratch must be 8-byte aligned (step_preds 4, y 8)");
        return MARL_EINVAL;
    }
    if (nb < 1 || (accumulate != 0 && accumulate != 1)) {
        set_error("episode_report: nb %d must be >= 1, accumulate %d must be 0 or 1", nb, accumulate);
        return MARL_EINVAL;
    }
    MARL_TRY(check_sizes(ns, na, nc, topk, bins, n_exit));
    ReportArgs a;
    for (int j = 0; j < MARL_REPORT_MAX_EXITS; ++j) a.thr[j] = 2.0f;
    for (int j = 0; j < n_exit; ++j) {
        const float tau = exit_thresholds[j];
        if (!(tau >= 0.f && tau <= 1.f)) {  // (false for NaN)
            set_error("episode_report: exit threshold %d is %g, outside [0, 1]", j, (double)tau);
            return MARL_EINVAL;
        }
        a.thr[j] = tau;
    }
    fill_layout(ns, na, nc, topk, bins, n_exit, a.off);
    if (report_bytes < (size_t)a.off[MARL_REPORT_WORDS] * 8) {
        set_error("episode_report: the report holds %zu bytes, %lld needed", report_bytes,
                  (long long)a.off[MARL_REPORT_WORDS] * 8);
        return MARL_ESIZE;
    }
    if (scratch_bytes < scratch_need(ns, nb)) {
        set_error("episode_report: the scratch holds %zu bytes, %zu needed", scratch_bytes, scratch_need(ns, nb));
        return MARL_ESIZE;
    }
    a.preds = step_preds;
    a.y = y;
    a.report = static_cast<int64_t*>(report_dev);
    a.recs = static_cast<StepRec*>(scratch);
    a.status = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + recs_bytes(ns, nb));
    a.exits = a.status + nb;
    a.ns = ns;
    a.na = na;
    a.nb = nb;
    a.nc = nc;
    a.topk = topk;
    a.bins = bins;
    a.n_exit = n_exit;
    a.accumulate = accumulate;
    a.ncp = (nc + 63) & ~63;
    // a wave per step, as many as the vote buffers leave room for
    int waves = ns < kRowMaxWaves ? ns : kRowMaxWaves;
    const int fit = kRowVoteBytes / (a.ncp * 4);
    if (waves > fit) waves = fit;
    const size_t lds = (size_t)waves * a.ncp * 4 + (size_t)ns * 8;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(report_row_kernel, dim3((unsigned)nb), dim3(waves * 64), lds, st, a);
    MARL_LAUNCH_CHECK();
    const int cal_blocks = (bins + kSumThreads / 64 - 1) / (kSumThreads / 64);
    hipLaunchKernelGGL(report_sum_kernel, dim3((unsigned)(ns + 1 + cal_blocks)), dim3(kSumThreads), 0, st, a);
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}
