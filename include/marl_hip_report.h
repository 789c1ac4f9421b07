/*
 * marl_hip_report.h - the episode report of libmarl_hip.so: what an episode's step_preds [Ns,Na,Nb,nC] say about the
 * classifier, reduced on the device in two launches - vote accuracy, top-k, NLL and agreement per step, every agent's
 * own accuracy per step, the confusion matrix and the calibration of the last step's vote, and the steps an episode
 * needs when it stops once the vote is confident enough.  The entry points live beside the C ABI that
 * include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports) and change none of it.  Conventions
 * (error codes, marl_last_error) are those of marl_hip.h.
 *
 * Definition.  Image b is SKIPPED if y[b] is outside [0, nC) or any of its Ns * Na * nC logits is not finite; a skipped
 * image adds 1 to `skipped` and nothing else.  For every other image, at every step t:
 *   z[t,b,c] = (sum_a preds[t,a,b,c], ascending a, fp32) / Na              (the vote the loss optimises)
 *   pred     = the lowest index of max_c z;                vote_hit[t] += pred == y
 *   rank     = #{c : z_c > z_y} + #{c < y : z_c == z_y};   rank_hist[t][min(rank, topk)] += 1
 *   nll      = -(z_y - max - logf(sum_c expf(z_c - max)));  nll_sum[t] += nll
 *   conf     = 1.0f / sum_c expf(z_c - max)
 *   pred_a   = the lowest-index argmax of preds[t,a,b,:];   agent_hit[t][a] += pred_a == y
 *   agree[t] += #{a : pred_a == pred}
 * at t = Ns - 1:  confusion[y][pred] += 1 (row = truth);  bin = min(bins - 1, (int)(conf * bins)) (fp32 product);
 *   cal_count[bin] += 1;  cal_hit[bin] += pred == y;  cal_conf[bin] += conf
 * for every threshold tau_j:  e = the first t with conf_t >= tau_j, else Ns - 1;  exit_hist[j][e] += 1;
 *   exit_hit[j] += pred_e == y
 * n += 1.   All counts are int64, all sums fp64.
 */
#ifndef MARL_HIP_REPORT_H
#define MARL_HIP_REPORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARL_REPORT_MAX_STEPS 1024
#define MARL_REPORT_MAX_AGENTS 64   /* one lane per agent, one bit per agent in a step record */
#define MARL_REPORT_MAX_CLASSES 1024 /* what the loss kernels serve */
#define MARL_REPORT_MAX_TOPK 16
#define MARL_REPORT_MAX_BINS 64
#define MARL_REPORT_MAX_EXITS 8

/* Slots of marl_report_layout's `out`: the offset of every field of the report buffer in 8-byte words, in this order.
 * The integer fields come first; [MARL_REPORT_NLL_SUM, MARL_REPORT_WORDS) are the fp64 fields. */
enum {
    MARL_REPORT_N = 0,       /* [1] */
    MARL_REPORT_SKIPPED,     /* [1] */
    MARL_REPORT_VOTE_HIT,    /* [ns] */
    MARL_REPORT_RANK_HIST,   /* [ns][topk + 1]: slot j < topk = label at rank j, slot topk = beyond */
    MARL_REPORT_AGENT_HIT,   /* [ns][na] */
    MARL_REPORT_AGREE,       /* [ns] */
    MARL_REPORT_CONFUSION,   /* [nc][nc] */
    MARL_REPORT_CAL_COUNT,   /* [bins] */
    MARL_REPORT_CAL_HIT,     /* [bins] */
    MARL_REPORT_EXIT_HIST,   /* [n_exit][ns] */
    MARL_REPORT_EXIT_HIT,    /* [n_exit] */
    MARL_REPORT_NLL_SUM,     /* [ns] fp64; its offset = the number of integer words */
    MARL_REPORT_CAL_CONF,    /* [bins] fp64 */
    MARL_REPORT_WORDS,       /* the buffer's size in words */
    MARL_REPORT_LAYOUT_SLOTS
};

/* Host only: out [MARL_REPORT_LAYOUT_SLOTS].  MARL_EINVAL / MARL_ELIMIT as marl_episode_report. */
int marl_report_layout(int ns, int na, int nc, int topk, int bins, int n_exit, int64_t* out);

/* Bytes of the per-image records between the two launches; 0 for sizes marl_episode_report refuses. */
size_t marl_report_scratch_bytes(int ns, int na, int nb, int nc, int topk, int bins, int n_exit);

/* step_preds fp32 [ns,na,nb,nc] contiguous and y int64 [nb] on the device; exit_thresholds [n_exit] host floats (they
 * travel by value in the kernel arguments).  accumulate = 0 overwrites the report (no memset needed before it), 1 adds
 * to it.  Two launches on `stream` - a row pass that reads step_preds once and leaves per-image records in `scratch`,
 * a sum pass that folds them into the report in a fixed order - no host synchronisation, no float atomics: two calls
 * on the same inputs give the same bytes.  report_dev and scratch are 8-byte aligned.
 * Before anything is enqueued:
 *   MARL_EINVAL  a null or misaligned pointer, a size < 1, topk < 1, bins < 1, n_exit < 0, accumulate not 0 / 1, a
 *                threshold outside [0, 1] or not finite
 *   MARL_ELIMIT  ns, na, nc, topk, bins or n_exit above its MARL_REPORT_MAX_*
 *   MARL_ESIZE   report_bytes < 8 * words of the layout, scratch_bytes < marl_report_scratch_bytes */
int marl_episode_report(const float* step_preds, const int64_t* y, int ns, int na, int nb, int nc, int topk, int bins,
                        const float* exit_thresholds, int n_exit, int accumulate, void* report_dev,
                        size_t report_bytes, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_REPORT_H */
