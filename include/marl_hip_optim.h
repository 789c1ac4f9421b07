/*
 * marl_hip_optim.h - the flat optimiser step of libmarl_hip.so: AdamW with decoupled weight decay, per-segment
 * learning-rate multipliers, a learning-rate schedule, an optional averaged copy of the weights (EMA), all in ONE
 * launch over the flat buffers.  The entry point lives beside the C ABI that include/marl_hip.h declares and versions
 * (MARL_ABI_VERSION, its list of exports) and changes none of it: marl_adam_step, its kernel and the counter block
 * keep their signatures and their bits.  Conventions (error codes, marl_last_error) are those of marl_hip.h.
 */
#ifndef MARL_HIP_OPTIM_H
#define MARL_HIP_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Most segments one call takes.  The table travels BY VALUE in the kernel arguments (12 bytes per segment: no device
 * allocation, and a captured graph keeps its own copy): 128 segments are 1536 bytes of the 4 KB argument block. */
#define MARL_OPTIM_MAX_SEGMENTS 128

enum { MARL_SCHED_CONSTANT = 0, MARL_SCHED_LINEAR = 1, MARL_SCHED_COSINE = 2 };

/* Elements [begin, end) of the flat buffers share one (lr_mult, weight_decay).  begin is a multiple of 4 (16-byte
 * aligned slices: no float4 straddles two segments); lr_mult == 0 freezes the segment: nothing in it is written. */
typedef struct marl_optim_segment {
    int64_t begin, end;
    float lr_mult, weight_decay;
} marl_optim_segment;

/* lr_t of the 1-based step t:  t <= warmup_steps:  base_lr * t / warmup_steps;  else constant: base_lr;  else with
 * x = min(1, (t - warmup_steps) / (total_steps - warmup_steps))  (1 when the two are equal):
 *   linear: base_lr * (1 - (1 - final_ratio) * x)      cosine: base_lr * (final_ratio + (1 - final_ratio) *
 *                                                               (1 + cos(pi x)) / 2). */
typedef struct marl_optim_schedule {
    int32_t kind; /* MARL_SCHED_* */
    int32_t pad_;
    double base_lr;
    int64_t warmup_steps, total_steps; /* total_steps is not read by MARL_SCHED_CONSTANT */
    double final_ratio;
} marl_optim_schedule;

/* One AdamW step over params / grads / exp_avg / exp_avg_sq [n] (device, fp32, 16-byte aligned), torch.optim.AdamW's
 * single-tensor order; per element of segment s:
 *   g  = grad * grad_scale
 *   p *= 1 - lr_t * lr_mult_s * weight_decay_s
 *   m += (1 - beta1) * (g - m);   v = v * beta2 + (1 - beta2) * g * g
 *   p -= (lr_t * lr_mult_s / bc1) * m / (sqrt(v) / sqrt(bc2) + eps),     bc_i = 1 - beta_i^t
 *   ema = ema_decay * ema + (1 - ema_decay) * p                          (ema != NULL only)
 * lr_t, bc1 and bc2 are derived ON THE DEVICE in fp64 from the integer step t - `step` (>= 1) or, with `counters`
 * (a marl_counters_* block) its step field, read when the kernel runs - by the first lane of every workgroup, so an
 * eager call and a graph replay run the same code and agree bit for bit, and a replay under a schedule needs no
 * marl_counters_set.  The counter block is only read.
 * segments [n_segments] (host): ascending, covering [0, n) without gaps or overlaps, at most
 * MARL_OPTIM_MAX_SEGMENTS.  scalars_out (device, nullable): {lr_t, bc1, bc2, t} as four fp32.
 * One kernel (optim_kernel<ema>, csrc/optim.hip), 16-byte loads and stores, no atomics, no workspace.
 * MARL_EINVAL before anything is enqueued: a null or misaligned buffer, n < 0, step < 1 without counters, a segment
 * table that breaks a rule above (or lr_mult / weight_decay negative or not finite), betas outside [0, 1), eps <= 0,
 * grad_scale not finite, ema_decay outside (0, 1) with an ema buffer, an unknown kind, base_lr < 0, warmup_steps < 0,
 * total_steps < warmup_steps (linear / cosine), final_ratio outside [0, 1]. */
int marl_optim_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                    float grad_scale, const marl_optim_segment* segments, int n_segments, double beta1, double beta2,
                    double eps, const marl_optim_schedule* schedule, int64_t step, const void* counters,
                    double ema_decay, float* scalars_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_OPTIM_H */
