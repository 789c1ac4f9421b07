/*
 * marl_hip_softtargets.h - a target distribution per image in the supervised term of the fused loss in libmarl_hip.so:
 * what CutMix, Mixup, distillation from a teacher and noisy-label targets need where every loss entry takes one integer
 * label per image.  The entry point lives beside the C ABI that include/marl_hip.h declares and versions
 * (MARL_ABI_VERSION, its list of exports) and changes none of it: every entry of that ABI keeps its signature, and with
 * nothing installed launches what it always launched, with the same bits.  Conventions (error codes, marl_last_error)
 * are those of marl_hip.h.
 */
#ifndef MARL_HIP_SOFTTARGETS_H
#define MARL_HIP_SOFTTARGETS_H

#ifdef __cplusplus
extern "C" {
#endif

/* The targets of every later loss call of this process (like marl_class_loss: process-global; the Python engine
 * installs it around each loss call and clears it behind it).  q_dev: fp32 [batch, nb_class] in device memory, read by
 * the kernels when a loss entry runs - not copied, not checked (the caller checks: finite, >= 0, no all-zero row) and
 * owned by the caller for as long as a launch or a captured graph may read it.  While it is installed,
 * marl_a2c_loss_fwd_bwd, marl_a2c_loss_entropy_fwd_bwd, marl_ppo_loss_fwd_bwd and marl_advantages use Q = q_dev where
 * they used the labels y (which they still take and do not read), in every phase; no launch is added.  With
 * z[t,b,:] = mean_a step_preds[t,a,b,:], nll_c(z) = -(z_c - max z - log sum exp(z - max z)) (from the logits: a logit
 * gap of 200 stays finite), and w, eps, s of marl_class_loss (1, 0, 1 with none installed):
 *   q_c              = w_c * ((1 - eps) * Q[b,c] + eps / nC)
 *   err[t,b]         = s_t * sum_c q_c * nll_c(z)       (without s_t: torch's cross_entropy(z, Q, weight=w,
 *                                                        label_smoothing=eps, reduction="none"))
 *   g_preds[t,a,b,c] = s_t / R * (softmax(z)_c * sum_c' q_c' - q_c),   R = Na * Nb
 *   rew[t,r]         = sum_c omega_c * Q[b,c] * (log nC - nll_c(preds[t,r,:])) / log nC,
 *                      omega = w under weight_rewards, else 1 - linear in Q: a mixed image's reward is the mix of the
 *                      two rewards.
 * Entries with Q[b,c] == 0 are skipped, not multiplied (a logit of -inf in a class without target mass stays out of
 * the sums).  The sums over the classes are wave sums in a fixed order (no atomics): results are bit-reproducible, and
 * a one-hot Q reproduces the bits of the integer-label call, with nothing else installed and under marl_class_loss.
 * Sites: the soft instances of loss_error_kernel and loss_rewards_kernel (csrc/loss.hip).
 * A loss entry whose cfg disagrees with (batch, nb_class) returns MARL_EINVAL before anything is enqueued.
 * marl_plan_query key "soft_targets": 1 while a setting is installed.
 * (NULL, 0, 0) clears the setting.  MARL_EINVAL: a negative size, a pointer with a zero size, sizes without a pointer. */
int marl_soft_targets(const float* q_dev, int batch, int nb_class);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_SOFTTARGETS_H */
