/*
 * marl_hip_classloss.h - options of the supervised term of the fused loss in libmarl_hip.so: class weights, label
 * smoothing and step weights of the vote error, and cost-sensitive rewards.  The entry point lives beside the C ABI
 * that include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports) and changes none of it: every
 * entry of that ABI keeps its signature, and with nothing installed launches what it always launched, with the same
 * bits.  Conventions (error codes, marl_last_error) are those of marl_hip.h.
 */
#ifndef MARL_HIP_CLASSLOSS_H
#define MARL_HIP_CLASSLOSS_H

#ifdef __cplusplus
extern "C" {
#endif

/* The supervised term of every later loss call of this process (like marl_policy_explore: process-global; the Python
 * engine installs it around each loss call and clears it behind it).  With z[t,b,:] = mean_a step_preds[t,a,b,:],
 * nll_c = -(z_c - max z - log sum exp(z - max z)) (from the logits, never log(softmax): a logit gap of 200 stays
 * finite), y = y[b], class weights w [nb_class], smoothing eps and step weights s [nb_steps]:
 *   q_c      = (1 - eps) * w_y * 1[c == y] + (eps / nC) * w_c
 *   err[t,b] = s_t * sum_c q_c * nll_c         (without s_t: torch's cross_entropy(weight=w, label_smoothing=eps,
 *                                               reduction="none"))
 *   g_preds[t,a,b,c] = s_t / R * (softmax(z)_c * sum_c' q_c' - q_c),   R = Na * Nb.
 * The `error` scalar of the loss entries is the mean of this err, and the loss takes sum_t mean_b of it - what is
 * optimised; no scalar is added.  weight_rewards != 0: rew[t,r] = w_y * (log nC - CE) / log nC with the plain
 * per-agent cross-entropy CE; smoothing and step weights never reach the rewards.
 * Sites: loss_error_kernel and loss_rewards_kernel (csrc/loss.hip) take their option instances - the vote error
 * whenever a setting is installed, the rewards with weight_rewards and class weights - in marl_a2c_loss_fwd_bwd,
 * marl_a2c_loss_entropy_fwd_bwd, marl_ppo_loss_fwd_bwd and marl_advantages, every phase; no launch is added.  The
 * sums over the classes are wave sums in a fixed order (no atomics): results are bit-reproducible, and w == 1,
 * eps == 0, s == 1 given explicitly reproduce the plain kernels' bits.
 * class_weights_dev / step_weights_dev: device pointers to fp32, read by the kernels when a loss entry runs - not
 * copied, not checked (the caller checks: finite, >= 0, not all zero) and owned by the caller for as long as a
 * launch or a captured graph may read them; NULL means all ones.  nb_class / nb_steps: the lengths; a loss entry
 * whose cfg disagrees with a non-zero one returns MARL_EINVAL before anything is enqueued (0 with a NULL pointer:
 * not checked).  marl_plan_query key "class_loss": 1 while a setting is installed.
 * (NULL, 0, 0, NULL, 0, 0) clears the setting.  MARL_EINVAL: label_smoothing outside [0, 1) or not finite, a
 * negative length, a pointer with a length of 0. */
int marl_class_loss(const float* class_weights_dev, int nb_class, float label_smoothing,
                    const float* step_weights_dev, int nb_steps, int weight_rewards);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_CLASSLOSS_H */
