/*
 * marl_hip_rowops.h - kernel-level hooks of libmarl_hip.so for the row passes of the batched backward
 * (csrc/rowops.hip), one launch plus its affine reduction each.  Tests and measurement only: the product
 * reaches these kernels through marl_episode_backward / marl_step_backward.  They are not part of the C ABI
 * that include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports): a caller of that ABI
 * needs neither, and they may change with the kernels.  Conventions (error codes, marl_last_error, streams)
 * are those of marl_hip.h.
 */
#ifndef MARL_HIP_ROWOPS_H
#define MARL_HIP_ROWOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of one Linear-LayerNorm-SiLU block's LayerNorm + SiLU (the hidden layers of networks/policy.py:12-14
 * and 23-25 - actor and critic - and of networks/prediction.py:11-13, through loss.backward(),
 * training/trainer.py:115), the row pass behind the heads' backward in marl_episode_backward:
 *   dz [m, n] (leading dimension lddz) = gradient w.r.t. the LayerNorm input z, from z, the statistics
 *   stats [m][2] (mean, rstd: what marl_ln_silu_fwd stored) and the gradient of the SiLU output;
 *   dgamma, dbeta [n] = the affine gradients, summed over the rows in the library's fixed order.
 * The incoming gradient is da [m, n] (kin == 0; dz may be da, in place), or, for a block whose successor has only
 * kin in 1..4 outputs (critic value, policy logits), the rank form sum_j g[r][j] * w1t[c][j] with g [m, kin]
 * (leading dimension ldg) the gradient of those outputs and w1t [n][ldw] the successor's weight, transposed
 * (da is not read; n <= 384).  scratch holds the per-workgroup partial sums and is consumed:
 * max(256, ceil(m / 256)) * 2n floats always suffice; a smaller buffer that is too small returns MARL_ESIZE.
 * n <= 2048. */
int marl_ln_silu_bwd(const float* da, int ldda, const float* g, int ldg, int kin, const float* w1t, int ldw,
                     const float* z, int ldz, const float* stats, const float* gamma, const float* beta,
                     float* dz, int lddz, float* dgamma, float* dbeta, float* scratch, size_t scratch_bytes,
                     int m, int n, void* stream);
/* Backward of GroupNorm + SiLU of one conv layer (networks/vision.py:33-36) on NHWC rows z [rows][P][C] with the
 * saved statistics stats [rows][G][2] (mean, rstd): dz [rows][P][C], dgamma / dbeta [C].  da is the gradient of the
 * layer's output, row stride ldda, laid out [C][P] when da_chw (the flattened feature the extractor hands on,
 * vision.py:38) else [P][C].  C / G must be a power of two <= 64.  scratch as for marl_ln_silu_bwd with n = C,
 * m = rows. */
int marl_gn_silu_bwd(const float* da, int64_t ldda, int da_chw, const float* z, const float* stats,
                     const float* gamma, const float* beta, float* dz, float* dgamma, float* dbeta,
                     float* scratch, size_t scratch_bytes, int64_t rows, int p, int c, int groups,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_ROWOPS_H */
