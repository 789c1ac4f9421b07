/*
 * marl_hip_explore.h - exploration controls of the policy's action sampling in libmarl_hip.so: a temperature, an
 * eps-soft mixture with the uniform distribution, and greedy (deterministic) acting.  The entry point lives beside the
 * C ABI that include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports) and changes none of
 * it: every entry of that ABI keeps its signature, and with the controls at their defaults launches what it always
 * launched, with the same bits.  Conventions (error codes, marl_last_error) are those of marl_hip.h.
 */
#ifndef MARL_HIP_EXPLORE_H
#define MARL_HIP_EXPLORE_H

#ifdef __cplusplus
extern "C" {
#endif

/* Behaviour policy of every later sampling call of this process (like marl_comm_range: process-global; the Python
 * engine installs it around each call and clears it behind it).  With z the policy's logits and nA actions,
 *   s = softmax(z * (1 / temperature)),   pi_b[j] = (1 - eps) * s[j] + eps / nA.
 * pi_b is what is sampled from (argmax_j pi_b[j] / q_j, q ~ Exp(1) injected or drawn in-kernel, as before), what
 * step_probs and the workspace's PROBS hold, and what step_log_probas takes logf(pi_b[a]) from.  greedy != 0: the
 * action is argmax_j pi_b[j], the lowest index winning a tie; neither injected noise nor the generator is read (the
 * episode's generator counters advance as always).  Forced actions override either choice.  The constants
 * 1 / temperature, 1 - eps and eps / nA are formed once on the host in fp32.
 * Sites: the sampling epilogue of the chained panel launch (marl_plan_query "explore_form" = 1), sample_kernel (2)
 * and marl_step_forward* ; "explore" = 1 while controls are installed.
 * Backward (marl_episode_backward*, marl_step_backward; call it under the setting of the forward): with
 *   G_j = (1 - eps) * (g_probs[j] + g_logp * 1[j == a] / pi_b[a]),   dz_j = (1 / temperature) * s_j * (G_j - sum_k s_k G_k),
 * s recovered from the saved pi_b as (pi_b - eps / nA) / (1 - eps) - the reason eps is capped at 0.5.  An action of
 * probability exactly 0 (eps == 0 only) drops its log-prob term; an s_k of exactly 0 adds nothing.  With temperature 1
 * and eps 0 (greedy alone) pi_b is the plain softmax and the backward launches what it launches without controls.
 * (1, 0, 0) clears the controls.  MARL_EINVAL: temperature <= 0 or not finite, eps outside [0, 0.5]. */
int marl_policy_explore(float temperature, float eps, int greedy);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_EXPLORE_H */
