/*
 * marl_hip_rowops.h - kernel-level hooks of libmarl_hip.so for the row kernels of csrc/rowops.hip: the row passes
 * of the batched backward (one launch plus its affine reduction each) and the small kernels of the step loop (one
 * launch each, a thin wrapper of the launcher).  Tests and measurement only: the product reaches these kernels
 * through marl_episode_forward / marl_episode_backward / marl_step_*.  They are not part of the C ABI
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

/* ---- the step loop's row kernels: one launch each.  Every entry returns MARL_EINVAL (null required pointer, negative
 * row count, size < 1, leading dimension shorter than the row) or MARL_ELIMIT (width outside the kernel's range)
 * before anything is launched; a row count of 0 is MARL_OK and launches nothing. ---- */

/* GroupNorm (eps 1e-5, biased variance over (C / G) * P) + SiLU of one conv layer (networks/vision.py:33-36) on NHWC
 * rows z [rows][P][C]: out (row stride ldo >= P * C; [C][P] inside a row when out_chw, else [P][C]) and stats
 * [rows][G][2] = (mean, rstd), nullable.  cols (nullable; P == hin * hin): the next layer's im2col rows (3x3, stride 2,
 * padding 1) [rows * hout * hout][ldk], column (kh * 3 + kw) * C + c, hout = (hin - 1) / 2 + 1; padding taps are not
 * written (the caller zeroes cols once).  cols, and a null out, need a power-of-two C in 4..64 and P * C <= 1024
 * (cols otherwise: MARL_ELIMIT).  out and cols may not both be null. */
int marl_gn_silu_fwd(const float* z, const float* gamma, const float* beta, float* out, int64_t ldo, int out_chw,
                     float* stats, int64_t rows, int p, int c, int groups, float* cols, int ldk, int hin,
                     void* stream);
/* marl_ln_silu_fwd (marl_hip.h) plus the fused one-output layer on top (the critic's value, networks/policy.py:26):
 * dot_out [m] = silu row . wdot [n] + bdot[0].  wdot null: no dot.  The dot needs n <= 384 (MARL_ELIMIT otherwise). */
int marl_ln_silu_dot_fwd(const float* z, int ldz, const float* gamma, const float* beta, float* out, int ldo,
                         float* stats, int m, int n, const float* wdot, const float* bdot, float* dot_out,
                         void* stream);
/* map_pos (networks/state.py:14-16): z [rows, nd] = npos . W^T + b, out = SiLU(LayerNorm(z)), stats [rows][2]
 * (nullable).  Positions: npos_in [rows][2] fp32 already normalised, or (npos_in null) pos [rows][2] int32 divided by
 * (h, w); npos4 [rows][4] (nullable) receives them in columns 0 and 1.  weight is packed [nd][4], columns 2 and 3
 * are not read. */
int marl_pos_embed_fwd(const int32_t* pos, const float* npos_in, int h, int w, const float* weight,
                       const float* bias, const float* gamma, const float* beta, float* npos4, float* z, int ldz,
                       float* stats, float* out, int ldo, int64_t rows, int nd, void* stream);
/* Pointwise backward of count = 1 or 2 LSTM cells in one launch (every array has count entries).  Per cell: gates
 * [rows][ldg] holds the activated i | f | g | o (n each) on entry and the pre-activation gradients on exit; dc holds
 * dL/dc_t on entry and dL/dc_{t-1} on exit; dh, c_prev, c_new are read.  Four units per thread when every cell has
 * n % 4 == 0 and leading dimensions % 4 == 0 (then every pointer must be 16-byte aligned), else one unit per thread
 * for all cells.  g3 (nullable array; nullable entries): the k16 image (marl_image_build's format, g3_steps >= n / 4
 * 16-deep steps) that receives the gate gradients [rows, 4 n] at image rows g3_row0 + r - four-wide form only, a
 * request that falls to the scalar form is MARL_EINVAL.  skip_f32 (nullable; needs the image): the fp32 gate
 * gradients are not written, gates keeps the activated gates. */
int marl_lstm_cell_bwd(int count, const float* const* dh, float* const* dc, float* const* gates,
                       const float* const* c_prev, const float* const* c_new, const int* lddh, const int* lddc,
                       const int* ldg, const int* ldc, const int* n, void* const* g3, const int* g3_row0,
                       const int* g3_steps, const int* skip_f32, int64_t rows, void* stream);
/* Gradient of the policy logits, out [rows][ld], from the saved row probs [rows][n_actions] (tight), the sampled
 * actions [rows] and dlogp [rows] = dL/d(log-prob of the action) (nullable: 0):
 *   form 0  out_j = dlogp (1[j == a] - p_j)
 *   form 1  out_j = p_j (g_j - sum_k p_k g_k) + dlogp (1[j == a] - p_j), g = dprobs [rows][n_actions] = dL/dprobs
 *   form 2  the same through the behaviour policy probs = keep softmax(z inv_tau) + floor of marl_policy_explore
 *           (dprobs nullable: 0); an action of probability exactly 0 drops its log-prob term.
 * n_actions <= MARL_MAX_ACTIONS.  Forms 1 and 2 move rows as 16-byte pieces when n_actions % 4 == 0, ld % 4 == 0 and
 * probs, dprobs and out are 16-byte aligned, else element by element - same operations, same bits. */
int marl_policy_dlogits(int form, const float* dlogp, const float* dprobs, const float* probs,
                        const int32_t* actions, float* out, int ld, int64_t rows, int n_actions, float inv_tau,
                        float keep, float floor, void* stream);
/* out [rows] = a [rows, n] (leading dimension lda) . w [n] + b[0] */
int marl_rowdot(const float* a, int lda, const float* w, const float* b, float* out, int64_t rows, int n,
                void* stream);
/* aggregate_messages (networks/message.py:5-17) on m [na * nb][ld] (row a * nb + b): out = (sum over the agents of a
 * batch element - own row) / (na - 1), zeros when na == 1.  out == m is legal. */
int marl_agg_msg(const float* m, float* out, int ld, int na, int nb, int n, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_ROWOPS_H */
