/*
 * marl_hip.h - C ABI of libmarl_hip.so: the MI355X (gfx950) implementation of
 * MARLClassification's hot path (multi-agent episode rollout + A2C update).
 *
 * The reference (Ipsedo/MARLClassification) has no FFI: its hot path is Python
 * over torch tensors.  Each entry point below therefore names the reference
 * function(s) it replaces (paths relative to /root/reference/marl_classification).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host;
 *     fp32 tensors are contiguous, int64 where the reference uses int64;
 *   - rows are r = a * nb + b, i.e. [Na, Nb, ...] tensors flattened over their
 *     first two dimensions (networks/models.py:93);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     call only enqueues work on it, nothing synchronises the device;
 *   - no hidden device allocations: the caller owns every buffer, including the
 *     two workspaces whose sizes marl_workspace_sizes() reports.  Both must be
 *     ZERO-FILLED once by the caller before first use (padding columns inside
 *     them are never written and are read as zeros by the matrix kernels);
 *   - the WEIGHTS workspace (size and the offset of everything inside it) is a function of the model fields of
 *     marl_config and of the tuning knobs only - never of batch, nb_agents, nb_steps or the image size: one
 *     marl_pack_weights serves every batch size until the weights change (an epoch's last partial batch, an
 *     evaluation batch).  The EPISODE workspace depends on all of them: re-query marl_workspace_sizes;
 *   - return value: 0 on success, a negative MARL_E* code otherwise; nothing
 *     throws across the ABI.  marl_last_error() gives a thread-local message;
 *   - one process drives one GPU (the launch contract of bench.py / train.py): the one-off
 *     kernel attributes (LDS opt-in), the profiling hook and the tuning knobs are per-process
 *     state, not per-device or per-thread;
 *   - data parallelism needs no entry point here: the gradients land in ONE flat fp32 buffer
 *     (the caller's, see marl_adam_step) and the caller all-reduces that buffer with RCCL
 *     (torch.distributed backend "nccl" in parallel.py) between marl_episode_backward and
 *     marl_adam_step, passing 1 / world_size as grad_scale.  SURVEY 8(b) sketched a
 *     "marl_allreduce_grads" wrapper taking a communicator; it would only forward to ncclAllReduce, so the
 *     collective stays with the host framework that owns the communicator;
 *   - size limits: GEMM operands are addressed with 32-bit byte offsets from a 64-bit base,
 *     so rows * leading_dimension of any activation matrix must stay below 2^30 floats
 *     (e.g. Ns * Na * Nb < 2^20 rows at 4 * n_b = 1024 gate columns: 4095 images per GPU at
 *     the RESISC45 16-agent / 16-step configuration).
 */
#ifndef MARL_HIP_H
#define MARL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARL_ABI_VERSION 5

#define MARL_OK 0
#define MARL_EINVAL (-1)   /* bad configuration / null pointer          */
#define MARL_ELIMIT (-2)   /* dimension outside the supported range     */
#define MARL_EHIP (-3)     /* a HIP runtime call failed                 */
#define MARL_ESIZE (-4)    /* workspace too small                       */

#define MARL_COUNTERS_BYTES 32 /* device-side counter block, see marl_counters_set */

#define MARL_MAX_CNN_LAYERS 5
#define MARL_MAX_ACTIONS 16

/* Shape of one ModelsWrapper + Environment + EpisodeSampler triple
 * (networks/models.py:37-50, core/environment.py:14-16, core/episode.py:24-30). */
typedef struct marl_config {
    int32_t nb_agents;   /* Na */
    int32_t batch;       /* Nb */
    int32_t nb_steps;    /* Ns */
    int32_t img_c, img_h, img_w;  /* image batch [Nb, img_c, img_h, img_w] fp32 */
    int32_t window;      /* f */
    int32_t cnn_layers;  /* number of Conv-GroupNorm-SiLU blocks (vision.py:23-52) */
    int32_t cnn_ch[MARL_MAX_CNN_LAYERS + 1]; /* cnn_ch[0] = channels the CNN reads
                            (1 for MnistCnn: channel 0 only, vision.py:63-65), then
                            the output channels of every layer */
    int32_t cnn_groups[MARL_MAX_CNN_LAYERS];
    int32_t n_b, n_a, n_m, n_m_o, n_d; /* belief / action / message / decoded / pos */
    int32_t nb_action, nb_class;
    int32_t nlb, nla;    /* hidden_size_belief / hidden_size_action of the heads */
    int32_t actions[MARL_MAX_ACTIONS][2]; /* movement per action index (dim 0 = H) */
    int32_t img_u8;      /* 1: the image batch is uint8 [Nb,C,H,W]; the gather kernel applies
                            ToTensor (x / 255, registry.py:56-57) on the fly - 4x less HBM and
                            PCIe traffic than uploading fp32 */
} marl_config;

/* Parameter table: an array of MARL_NPARAMS device pointers in this order.
 * Shapes are those of the reference's state_dict() (tight, row-major):
 *   4*l+0 conv_l.weight [co,ci,3,3]  4*l+1 conv_l.bias [co]
 *   4*l+2 gn_l.weight [co]           4*l+3 gn_l.bias [co]          (l < 5, unused = NULL)
 * then the indices below. */
enum {
    MARL_P_POS_W = 20, MARL_P_POS_B, MARL_P_POS_LNW, MARL_P_POS_LNB,          /* map_pos   */
    MARL_P_ENC_W0, MARL_P_ENC_B0, MARL_P_ENC_LN0W, MARL_P_ENC_LN0B,
    MARL_P_ENC_W1, MARL_P_ENC_B1, MARL_P_ENC_LN1W, MARL_P_ENC_LN1B,          /* encode_msg */
    MARL_P_DEC_W0, MARL_P_DEC_B0, MARL_P_DEC_LN0W, MARL_P_DEC_LN0B,
    MARL_P_DEC_W1, MARL_P_DEC_B1, MARL_P_DEC_LN1W, MARL_P_DEC_LN1B,          /* decode_msg */
    MARL_P_LB_WIH, MARL_P_LB_WHH, MARL_P_LB_BIH, MARL_P_LB_BHH,              /* belief LSTM */
    MARL_P_LA_WIH, MARL_P_LA_WHH, MARL_P_LA_BIH, MARL_P_LA_BHH,              /* action LSTM */
    MARL_P_POL_W0, MARL_P_POL_B0, MARL_P_POL_LNW, MARL_P_POL_LNB, MARL_P_POL_W1, MARL_P_POL_B1,
    MARL_P_CRI_W0, MARL_P_CRI_B0, MARL_P_CRI_LNW, MARL_P_CRI_LNB, MARL_P_CRI_W1, MARL_P_CRI_B1,
    MARL_P_PRE_W0, MARL_P_PRE_B0, MARL_P_PRE_LNW, MARL_P_PRE_LNB, MARL_P_PRE_W1, MARL_P_PRE_B1,
    MARL_NPARAMS
};

int marl_abi_version(void);
const char* marl_last_error(void);

/* Number of fp32 elements of parameter `index` for `cfg` (0 for unused slots). */
int64_t marl_param_numel(const marl_config* cfg, int index);

/* Byte sizes of the two caller-owned workspaces:
 *   weights_ws : padded / transposed copies of the parameters + packed gradients
 *   episode_ws : every per-step activation of one episode (saved for backward)
 * `train` = 0 sizes episode_ws for rollout only (nothing kept for backward).
 * ABI 3: every entry point that takes a workspace also takes its size in bytes and returns
 * MARL_ESIZE (nothing enqueued) when the layout for the CURRENT configuration and tuning knobs does
 * not fit - e.g. a buffer allocated before a layout-affecting marl_tune() call.  (marl_a2c_loss_fwd_bwd
 * wants the TRAINING size: its scratch is the tail of that layout.) */
int marl_workspace_sizes(const marl_config* cfg, int train,
                         size_t* weights_ws_bytes, size_t* episode_ws_bytes);

/* Re-packs the parameters into weights_ws; call after every optimiser step and
 * after load_state_dict (replaces nothing in the reference - layout plumbing). */
int marl_pack_weights(const marl_config* cfg, const float* const* params_host,
                      void* weights_ws, size_t weights_ws_bytes, void* stream);

/* Environment.__observation (core/environment.py:95-126): coalesced patch gather.
 * img [Nb,C,H,W] fp32, pos int64 [Na*Nb,2] -> obs [Na*Nb, C, f, f] fp32. */
int marl_patch_gather(const float* img, const int64_t* pos, float* obs,
                      int nb_agents, int batch, int c, int h, int w, int f, void* stream);

/* Environment.step / __transition (core/environment.py:56-66,128-150):
 * pos' = pos + table[a] if the move stays inside [0, size - f) in every dim, else pos.
 * table_host: nb_action x 2 int32 on the HOST. pos_in/pos_out int64 [rows,2] (may alias). */
int marl_transition(const int64_t* pos_in, const int64_t* actions, int64_t* pos_out,
                    const int32_t* table_host, int nb_action, int rows,
                    int h, int w, int f, void* stream);

/* Perf-mode draws of one episode inside the library (counter-based Philox4x32-10; same
 * distributions as the reference's draws - core/environment.py:33-43: pos0[r][d] uniform in
 * [0, size_d - f); networks/models.py:148-159: h0,c0 [R,n_b], hc0,cc0 [R,n_a] ~ N(0,1) - but not
 * the reference's mt19937 stream: parity runs inject host-drawn tensors instead).  `noise`
 * (nullable, [Ns,R,nA]) additionally receives Exp(1) draws.  (seed, offset) selects the stream:
 * the same pair always produces the same tensors. */
int marl_draw_episode(const marl_config* cfg, uint64_t seed, uint64_t offset,
                      const void* counters, int64_t* pos0, float* h0, float* c0, float* hc0,
                      float* cc0, float* noise, void* stream);

/* Device-resident iteration counters (MARL_COUNTERS_BYTES, caller-owned device memory): the
 * generator offset of the episode draws and the Adam step with its bias corrections.  Calls that
 * take `counters` (nullable) ADD its generator offset to their rng_offset argument / take the
 * Adam step scalars from it, so one iteration (draw -> rollout -> loss -> backward -> Adam ->
 * re-pack -> marl_counters_tick) can be captured once (marl_graph_*) and replayed with no
 * host-side change between replays.  set: offset / step (1-based, the step the next Adam applies)
 * as given; tick: both + 1. */
int marl_counters_set(void* counters, uint64_t rng_offset, int64_t step, float lr, float beta1,
                      float beta2, void* stream);
int marl_counters_tick(void* counters, float lr, float beta1, float beta2, void* stream);

/* hipGraph capture of whatever the library enqueues on `stream` between begin and end (the
 * stream must not be the NULL stream; nothing may synchronise or allocate in between).
 * marl_graph_end instantiates the captured graph; marl_graph_launch replays it.  The captured
 * calls keep their pointer arguments: replays read / write the same buffers. */
int marl_graph_begin(void* stream);
int marl_graph_end(void* stream, void** graph_exec_out);
int marl_graph_launch(void* graph_exec, void* stream);
int marl_graph_destroy(void* graph_exec);

/* EpisodeSampler.__episode_impl (core/episode.py:32-82) with the reference's random
 * draws as INPUTS: img fp32 (or uint8 when cfg->img_u8) [Nb,C,H,W]; pos0 int64 [R,2]; h0,c0 [R,n_b]; hc0,cc0 [R,n_a];
 * noise [Ns,R,nA] ~ Exp(1) (th.multinomial == argmax(p / noise)).
 * noise == NULL (and no forced_actions): the Exp(1) variates are drawn inside the sampling
 * kernel from Philox4x32-10 keyed by (rng_seed, rng_offset, step, row) - perf mode, nothing to
 * generate, store or read back per step.
 * forced_actions (int64 [Ns,R]) may be NULL; if given it replaces sampling.
 * Outputs: step_preds [Ns,R,nC], step_logp [Ns,R], step_values [Ns,R],
 * step_pos int64 [Ns,R,2] (after move t), step_actions int64 [Ns,R] (may be NULL).
 * With train != 0 the activations needed by marl_episode_backward stay in episode_ws. */
int marl_episode_forward(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                         void* episode_ws, size_t episode_ws_bytes,
                         const void* img, const int64_t* pos0,
                         const float* h0, const float* c0, const float* hc0, const float* cc0,
                         const float* noise, const int64_t* forced_actions,
                         uint64_t rng_seed, uint64_t rng_offset, const void* counters,
                         float* step_preds, float* step_logp, float* step_values,
                         int64_t* step_pos, int64_t* step_actions,
                         int train, void* stream);

/* loss.backward() through the episode (training/trainer.py:115): given dL/d(step_preds)
 * [Ns,R,nC], dL/d(step_logp) [Ns,R], dL/d(step_values) [Ns,R] (any may be NULL = zero),
 * writes dL/d(param) for every parameter into grads_host[i] (tight reference shapes,
 * overwritten, not accumulated).  `img` is the image batch of the matching
 * marl_episode_forward(train = 1) call: the first convolution's weight gradient re-gathers
 * the patches at the saved positions instead of keeping im2col rows in episode_ws (autograd
 * would keep the observation tensors alive the same way). */
int marl_episode_backward(const marl_config* cfg, void* weights_ws, size_t weights_ws_bytes,
                          void* episode_ws, size_t episode_ws_bytes,
                          const void* img, const float* g_preds, const float* g_logp,
                          const float* g_values, float* const* grads_host, void* stream);

/* The same backward pass that ALSO writes dL/d(img) (ABI 5).  The reference builds its autograd graph through the
 * patch crop - Environment.__observation (core/environment.py:95-126) is a masked_select of the image batch - so
 * img.requires_grad_(), run_episode, loss.backward() fills img.grad there (saliency maps, gradient-sign probes,
 * input optimisation).  Same arguments and the same parameter gradients as the entry above; d_img [Nb,C,H,W] fp32
 * (16-byte aligned) is OVERWRITTEN with the transposed first convolution (networks/vision.py:33-35) of dZ_0 summed
 * over the crops of every agent and step at the positions the rollout saved: pos0 for step 0, the position after
 * move t - 1 for step t; the crop after the last move is discarded by the episode (core/episode.py:72) and gets
 * none.  Exactly 0 where no window looked and in channels the CNN does not read (MnistCnn: channel 0 only,
 * networks/vision.py:63-65).  Every pixel has one owning workgroup and a fixed summation order: no atomics, the
 * result is bit-reproducible.  No scratch beyond episode_ws.  cfg->img_u8 != 0 (an integer image has no gradient)
 * or d_img == NULL: MARL_EINVAL, nothing enqueued. */
int marl_episode_backward_img(const marl_config* cfg, void* weights_ws, size_t weights_ws_bytes,
                              void* episode_ws, size_t episode_ws_bytes,
                              const void* img, const float* g_preds, const float* g_logp,
                              const float* g_values, float* const* grads_host, float* d_img,
                              void* stream);

/* The action distributions of the fused episode (same ABI version: three added entries, nothing else moves).
 *
 * marl_episode_forward_probs: marl_episode_forward with the same arguments, train = 0 or 1, and bit-identical
 * outputs, which ALSO delivers the distribution every step sampled its action from - softmax of the policy head
 * (networks/policy.py:16, core/agent.py:51) - into step_probs [Ns,R,nA] (tight, not NULL): one copy launch more, out
 * of the episode workspace where the sampling kernel keeps them for the backward pass. */
int marl_episode_forward_probs(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                               void* episode_ws, size_t episode_ws_bytes,
                               const void* img, const int64_t* pos0,
                               const float* h0, const float* c0, const float* hc0, const float* cc0,
                               const float* noise, const int64_t* forced_actions,
                               uint64_t rng_seed, uint64_t rng_offset, const void* counters,
                               float* step_preds, float* step_logp, float* step_values,
                               int64_t* step_pos, int64_t* step_actions, float* step_probs,
                               int train, void* stream);

/* marl_episode_backward_img with d_img NULLABLE (NULL: parameter gradients only, a uint8 image is fine then) plus
 * g_probs = dL/d(step_probs) [Ns,R,nA] (NULL = zero): the policy head's logit gradient of every row becomes
 * p_j (g_j - sum_k p_k g_k) + g_logp (1[j = a] - p_j) - a loss may depend on the whole distribution (entropy bonus,
 * KL penalty, distillation), not only on the log-probability of the sampled action.  No launch more than the entry
 * above; with g_probs == NULL and d_img == NULL exactly what marl_episode_backward enqueues. */
int marl_episode_backward_probs(const marl_config* cfg, void* weights_ws, size_t weights_ws_bytes,
                                void* episode_ws, size_t episode_ws_bytes,
                                const void* img, const float* g_preds, const float* g_logp,
                                const float* g_values, float* const* grads_host, float* d_img,
                                const float* g_probs, void* stream);

/* Data-parallel overlap (no reference counterpart: training/trainer.py is single-device).  While an event
 * is installed (per-process state, NULL clears it), every marl_episode_backward records it on its stream at the
 * point where the gradients of the three heads' parameters (MARL_P_POL_* .. MARL_P_PRE_*: Policy / Critic /
 * Prediction, networks/policy.py, prediction.py) are final - before the reverse-time loop and the batched weight
 * gradients behind it.  The caller's side stream waits for it and all-reduces that slice of the flat gradient buffer
 * while the rest of the backward pass runs (parallel.py, BucketedGradAllReduce). */
int marl_backward_heads_event(void* hip_event);

/* Communication graph of the message exchange (the method's aggregation over neighbours; the reference's
 * networks/message.py:5-17 is the complete graph).  m_dev: caller-owned fp32 [nb_agents, nb_agents] on the device,
 * row = receiver, column = sender; while it is installed (per-process state, NULL restores the mean over the other
 * agents) every episode / step entry aggregates
 *     mbar[a, b, :] = sum_a' M[a, a'] * m[a', b, :]
 * in fp32 as one fmaf chain over a' ascending, and its backward uses M^T in the same fixed order (no atomics; the
 * gradient with respect to M itself is marl_comm_grad's).  An entry that is exactly 0 is skipped, not multiplied: a non-neighbour's NaN / Inf
 * does not leak through 0 * x.  Self-loops, asymmetric and negative weights are legal; the caller checks that the
 * entries are finite.  The matrix is read when the kernels run, so it must stay alive and unchanged until the work
 * enqueued under it has finished; a captured graph keeps the pointer.  Under a matrix the chained panel launches
 * (encoder -> aggregate -> decoder, and their backward) mix inside the workgroup (the MIX instantiations of
 * panel_fwd_kernel / panel_bwd_kernel, the matrix staged in LDS); the decoder of step 0, the unchained panel path, the
 * GEMM + row-kernel path and the step entries aggregate with mix_msg_kernel in a launch of its own ahead of a plain
 * launch.  marl_plan_query keys "comm" (a matrix is set), "comm_form" (0 / 1 / 2: the mean in the chained launch /
 * while a panel stages / by agg_msg_kernel; 5 / 3 / 4: the matrix in the chained launch / by mix_msg_kernel ahead of
 * a plain panel launch / ahead of the GEMM path) and "panel_chain" report the form.  Returns MARL_ELIMIT for nb_agents above 32; an entry whose configuration has
 * another nb_agents returns MARL_EINVAL before anything is enqueued. */
int marl_comm_matrix(const float* m_dev, int nb_agents);

/* Gradient with respect to the mixing matrix (same ABI version: two added entries, nothing else moves).  It
 * differentiates the aggregation above - networks/message.py:5-17 under the matrix of marl_comm_matrix - with respect
 * to M: with torch ops in its place, M.requires_grad_() and loss.backward() fill M.grad with
 *     d_comm[a, a'] = sum_t sum_b sum_k dmbar_t[a, b, k] * m_t[a', b, k],    dmbar_t = dZd1_t * W_dec0
 * where m_t is the message step t aggregated and dZd1_t the gradient of the decoder's first linear layer - both are
 * what a finished backward leaves in its workspace, so this entry runs right AFTER marl_episode_backward* (ws = the
 * episode workspace, nb_steps = cfg->nb_steps) or marl_step_backward (ws = the step workspace, nb_steps = 1: the message
 * is the caller's msg) on the same stream, before anything else writes that workspace, with the weights that backward
 * used, and while a matrix of cfg->nb_agents is installed (its VALUES are not read: the node that calls this keeps the
 * matrix of its own forward).  nb_steps is the step count of the workspace's layout; cfg->nb_steps is ignored.
 * d_comm: fp32 [Na, Na], row = receiver, OVERWRITTEN.  DENSE: an entry of M that is exactly 0 still receives its sum -
 * the zero-skipping above is a property of the forward values, not of this derivative - so a NaN / Inf message of a
 * non-neighbour appears in ITS column of d_comm (and nowhere it did not appear before).
 * Two launches: workgroups that each own a contiguous range of (t, b) pairs write one Na x Na partial into `scratch`
 * (caller-owned, >= marl_comm_grad_scratch_bytes(cfg with that nb_steps); 0 = bad configuration), then a second kernel
 * sums the partials in a fixed order with fp64 accumulators: no atomics, bit-reproducible run to run.  Serves every
 * kernel family of the backward (chained / unchained panels, the GEMM + row-kernel path, the step entry).
 * Errors, each before anything is enqueued: MARL_EINVAL - a null pointer, no matrix installed, or a matrix of another
 * agent count; MARL_ESIZE - a workspace or the scratch too small; MARL_ELIMIT - more than 32 agents, or a decoder
 * weight [2 n_m, n_m] that does not fit the kernel's 160 KiB of LDS next to the staged rows. */
size_t marl_comm_grad_scratch_bytes(const marl_config* cfg);
int marl_comm_grad(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                   const void* ws, size_t ws_bytes, int nb_steps, float* d_comm,
                   void* scratch, size_t scratch_bytes, void* stream);

/* Range-limited communication (same ABI version: one added entry, nothing else moves).  While a radius >= 0 is
 * installed (per-process state, like the matrix; radius < 0 clears it) the matrix of marl_comm_matrix is the BASE B
 * of a dynamic graph: in image b, for the message emitted in step t, agent a hears agent a' only if the two are within
 * `radius` pixels at the positions of step t (window corners; MARL_COMM_CHEBYSHEV: max(|dy|, |dx|) <= radius;
 * MARL_COMM_EUCLIDEAN: dy^2 + dx^2 <= radius^2 - integer arithmetic, exact).  The weights are
 *     u[a, a'] = B[a, a'] * g[a, a']          (g[a, a] = 1: B's diagonal decides self-loops)
 *     w = u                                    normalize == 0
 *     w[a, a'] = u[a, a'] * (S_a / s_a)        normalize != 0, S_a = sum_a'' B[a, a''], s_a = sum_a'' u[a, a''] (fp32,
 *                                              ascending); s_a <= 0: the row is 0, the receiver hears nothing
 * (normalize expects B >= 0; the caller checks).  The message step t emits is encoded from the belief after observing at
 * POS[t] and aggregated - for the decoder of step t + 1 - under the gate of POS[t]; the zero message of step 0 under
 * POS[0].  The mixing stays one fmaf chain over the senders, ascending, exact zeros skipped; the backward applies the
 * transpose of the same per-(step, image) matrix, rebuilt from the saved positions by the same arithmetic.  The chained
 * panel launches build the matrices of their images in LDS (the GATE instantiations); the decoder of step 0, the
 * unchained panel path and the GEMM + row-kernel path take mix_msg_gated_kernel.  marl_plan_query key "comm_range": the
 * radius, or -1.  MARL_EINVAL: an unknown metric; and, each before anything is enqueued, an episode entry under a range
 * without a matrix, marl_step_forward* / marl_step_backward under a range (a single step has no integer positions of
 * the emission step) and marl_comm_grad under a range. */
#define MARL_COMM_CHEBYSHEV 0
#define MARL_COMM_EUCLIDEAN 1
int marl_comm_range(int radius, int metric, int normalize);

/* Loss of Trainer.train_epoch (training/trainer.py:76-111; training/functions.py:7-55)
 * and its gradient w.r.t. the episode outputs in one pass.
 * y int64 [Nb].  scalars_out[4] = {loss, path, error, critic} (trainer.py:111,119-122).
 * stats_inout: optional (n, sum, sumsq) hook for exact multi-GPU standardize:
 *   phase 0 = everything local (single GPU); phase 1 = only write local
 *   (n, sum x, sum x^2) of the advantages to adv_stats[3] (caller all-reduces them);
 *   phase 2 = finish using the all-reduced adv_stats. */
int marl_a2c_loss_fwd_bwd(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes,
                          const float* step_preds, const float* step_logp,
                          const float* step_values, const int64_t* y, float gamma,
                          float* g_preds, float* g_logp, float* g_values,
                          float* scalars_out, double* adv_stats, int phase, void* stream);

/* The same loss with an entropy bonus: loss = L - entropy_coef * mean_{a,b} sum_t H(step_probs[t,a,b,:]) - the
 * reference's reduction th.sum(., 0).mean() (training/trainer.py:111) applied to one more term.
 * H = -sum_j p_j log p_j with 0 log 0 = 0: an exactly zero probability adds nothing to H and gets g_probs = 0
 * (th.distributions.Categorical.entropy clamps instead and returns 1.19e-7 for [1,0,0,0]; the naive sum is NaN).
 * step_probs [Ns,R,nA] (marl_episode_forward_probs); entropy_coef >= 0; g_probs [Ns,R,nA] receives
 * entropy_coef / R * (log p_j + 1), to be handed to marl_episode_backward_probs; g_preds, g_logp, g_values as above.
 * scalars_out[5] = {loss including the entropy term, path, error, critic, mean_{t,a,b} H}.  Phase 1 does not touch
 * the entropy; phases 0 and 2 compute it, in the pass that writes g_logp / g_values: no launch more than the entry
 * above, fixed-order fp64 partial sums (bit-reproducible). */
int marl_a2c_loss_entropy_fwd_bwd(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes,
                                  const float* step_preds, const float* step_logp,
                                  const float* step_values, const int64_t* y, float gamma,
                                  const float* step_probs, float entropy_coef,
                                  float* g_preds, float* g_logp, float* g_values, float* g_probs,
                                  float* scalars_out, double* adv_stats, int phase, void* stream);

/* PPO on the fused path (same ABI version: three added entries, nothing else moves).  The reference trains with one
 * on-policy A2C step per rollout (training/trainer.py:66-116) and has no counterpart for any of them; each names the
 * existing piece it extends.
 *
 * marl_advantages extends the advantage of the loss above (training/trainer.py:89-92: discounted returns - values,
 * then training/functions.py:54-55) to GAE(lambda), as a call of its own whose results the caller keeps for several
 * update epochs: rewards = classification_rewards (functions.py:7-32); delta_t = r_t + gamma V_{t+1} - V_t with
 * V_Ns = 0 (the reference's returns have no bootstrap); A_t = delta_t + gamma lam A_{t+1}; ret_t = A_t + V_t (the
 * critic target); advn = (A - mean) / (unbiased std + 1e-8) over all Ns * R entries.  0 <= lam <= 1; lam == 1 takes
 * the arithmetic of discounted_returns (functions.py:35-51, flip-cumsum order): advn / ret then hold, bit for bit,
 * what marl_a2c_loss_fwd_bwd uses internally.  advn, ret: caller-owned [Ns,R].  adv_stats[3] / phase as above:
 * 0 = everything, 1 = up to the local (n, sum A, sum A^2), 2 = standardise with the (all-reduced) adv_stats.
 * episode_ws: the TRAINING layout (scratch = its loss tail). */
int marl_advantages(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes,
                    const float* step_preds, const float* step_values, const int64_t* y,
                    float gamma, float lam, float* advn, float* ret, double* adv_stats, int phase,
                    void* stream);

/* The clipped-surrogate loss in place of the path term of marl_a2c_loss_fwd_bwd (training/trainer.py:96-111), and its
 * gradient w.r.t. the episode outputs:
 *   rho = exp(step_logp - old_logp);  surr = -min(rho advn, clamp(rho, 1 - clip_eps, 1 + clip_eps) advn)
 *   loss = mean_{a,b} sum_t [surr + smooth_l1(step_values, ret)] + vote cross-entropy (trainer.py:78-87, unchanged)
 *          - entropy_coef * mean_{a,b} sum_t H(step_probs)        (only with step_probs, as in the entropy entry)
 * old_logp, advn, ret [Ns,R]: the rollout's log-probabilities and the outputs of marl_advantages; clip_eps > 0.
 * g_logp = -advn rho / R where the unclipped term is active, 0 where the clip is (advn > 0 and rho > 1 + clip_eps,
 * or advn < 0 and rho < 1 - clip_eps); g_preds, g_values as in marl_a2c_loss_fwd_bwd; g_probs as in
 * marl_a2c_loss_entropy_fwd_bwd.  step_probs and g_probs: both NULL (entropy_coef ignored) or both given.
 * With old_logp == step_logp bit for bit and advn / ret from marl_advantages(lam = 1), g_preds, g_logp and g_values
 * are bit-equal to marl_a2c_loss_fwd_bwd's.
 * scalars_out[7] = {loss, surr.sum(0).mean(), error.mean(), critic.sum(0).mean(), mean_{t,a,b} H (0 without
 * step_probs), approx_kl = mean(old_logp - step_logp), clip_frac = share of (t, r) where the clip is active}.
 * Three launches, fixed-order fp64 partial sums (bit-reproducible), scratch = the loss tail of episode_ws. */
int marl_ppo_loss_fwd_bwd(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes,
                          const float* step_preds, const float* step_logp, const float* step_values,
                          const int64_t* y, const float* old_logp, const float* advn, const float* ret,
                          float clip_eps, const float* step_probs, float entropy_coef,
                          float* g_preds, float* g_logp, float* g_values, float* g_probs,
                          float* scalars_out, void* stream);

/* th.nn.utils.clip_grad_norm_ (no call in the reference's trainer; it goes between loss.backward() and
 * optimizer.step(), training/trainer.py:115-116) on the flat gradient buffer marl_adam_step reads:
 * norm = sqrt(sum g^2) from fixed-order fp64 partials; g *= min(1, max_norm / (norm + 1e-6)) in place (a factor of
 * exactly 1 leaves every bit); *norm_out (device) = norm.  grad_scale (> 0; 1 / world_size after an all-reduce sum,
 * else 1) is applied FIRST - norm is that of grad_scale * g and the buffer ends up scaled by it too, so
 * marl_adam_step then takes grad_scale = 1 and every rank clips the same averaged gradient.  Two launches, no host
 * synchronisation.  scratch: caller-owned, >= MARL_GRAD_CLIP_SCRATCH_BYTES, 8-byte aligned; max_norm > 0; n >= 0. */
#define MARL_GRAD_CLIP_BLOCKS 1024
#define MARL_GRAD_CLIP_SCRATCH_BYTES (MARL_GRAD_CLIP_BLOCKS * 8)
int marl_grad_clip(float* grads, int64_t n, float max_norm, float grad_scale, float* norm_out,
                   void* scratch, size_t scratch_bytes, void* stream);

/* th.optim.Adam.step (training/trainer.py:33,116) on one flat buffer:
 * betas (0.9, 0.999), eps 1e-8, no weight decay; `step` is 1-based. grad_scale
 * multiplies the gradient first (1/world_size after an all-reduce sum).  counters != NULL:
 * `step` and the bias corrections come from the device-side counter block (graph replay). */
int marl_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   int64_t n, int64_t step, float lr, float beta1, float beta2, float eps,
                   float grad_scale, const void* counters, void* stream);

/* ModelsWrapper.forward + MultiAgent.act for ONE step used standalone
 * (networks/models.py:78-138, core/agent.py:40-68): obs [R,C,f,f] is gathered by the
 * caller (marl_patch_gather); msg [R,n_m]; norm_pos [R,2]; state in h,c,hc,cc.
 * Outputs: probs [R,nA], values [R], preds [R,nC], new_msg [R,n_m], new state. */
int marl_step_forward(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                      void* episode_ws, size_t episode_ws_bytes,
                      const float* obs, const float* msg, const float* norm_pos,
                      const float* h, const float* c, const float* hc, const float* cc,
                      float* probs, float* values, float* preds, float* new_msg,
                      float* h_out, float* c_out, float* hc_out, float* cc_out,
                      const float* noise, uint64_t rng_seed, uint64_t rng_offset,
                      int64_t* actions_out, float* logp_out, void* stream);
/* (actions_out int64 [R], logp_out [R]: optional - when both are given the call also samples the
 * action and its log-probability, core/agent.py:53-61, from noise [R,nA] ~ Exp(1) if given, else
 * from the library's generator at (rng_seed, rng_offset).) */

/* Autograd through ONE step (ABI 4): every ModelsWrapper.forward / MultiAgent.act call of the reference adds
 * to the autograd graph (networks/models.py:78-138, core/agent.py:40-68); a user loop over act() - the
 * reference's own EpisodeSampler is one (core/episode.py:32-82) - back-propagates through each of them.
 *
 * marl_step_forward_train: marl_step_forward with the same arguments and bit-identical outputs, which also
 * keeps the activations marl_step_backward needs in a caller-owned STEP workspace: the training layout of one
 * step, marl_workspace_sizes(cfg with nb_steps = 1, train = 1) (cfg->nb_steps is ignored by both calls).  One
 * workspace per live step; it is free again after its backward. */
int marl_step_forward_train(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                            void* step_ws, size_t step_ws_bytes,
                            const float* obs, const float* msg, const float* norm_pos,
                            const float* h, const float* c, const float* hc, const float* cc,
                            float* probs, float* values, float* preds, float* new_msg,
                            float* h_out, float* c_out, float* hc_out, float* cc_out,
                            const float* noise, uint64_t rng_seed, uint64_t rng_offset,
                            int64_t* actions_out, float* logp_out, void* stream);

/* loss.backward() through the step of the matching marl_step_forward_train call (same weights: call it before
 * the next marl_pack_weights).  obs is that call's observation [R,C,f,f] (the first convolution's weight
 * gradient reads it).  Upstream gradients, each NULL = zero: g_probs [R,nA]; g_logp [R] = dL/d log p[a] of the
 * action the forward SAMPLED (NULL unless the forward sampled); g_values [R]; g_preds [R,nC]; g_msg [R,n_m];
 * g_h, g_c [R,n_b]; g_hc, g_cc [R,n_a] - of the step's outputs.  Writes dL/d(param) into grads_host[i] (tight
 * reference shapes, OVERWRITTEN - accumulation over steps is the caller's, as in marl_episode_backward) and
 * the input gradients d_msg [R,n_m] (through the message mean: networks/message.py:5-17), d_h, d_c [R,n_b],
 * d_hc, d_cc [R,n_a] (tight; each NULL = not wanted).  No gradient w.r.t. obs / norm_pos (the reference's are
 * crops of an image batch that does not require grad: core/environment.py:95-126). */
int marl_step_backward(const marl_config* cfg, void* weights_ws, size_t weights_ws_bytes,
                       void* step_ws, size_t step_ws_bytes, const float* obs,
                       const float* g_probs, const float* g_logp, const float* g_values,
                       const float* g_preds, const float* g_msg, const float* g_h, const float* g_c,
                       const float* g_hc, const float* g_cc, float* const* grads_host,
                       float* d_msg, float* d_h, float* d_c, float* d_hc, float* d_cc, void* stream);

/* Environment.normalized_positions (core/environment.py:74-81): out[r,d] = pos[r,d] / size_d. */
int marl_normalize_positions(const int64_t* pos, float* out, int rows, int h, int w, void* stream);

/* ---- kernel-level entry points (used by tests/ and profiling; same kernels) ---- */
/* C[M,N] (+)= A[M,K] * B[N,K]^T + bias ; lda/ldb multiples of 4, 16-byte aligned. */
int marl_gemm_nt(const float* a, int lda, const float* b, int ldb, const float* bias,
                 float* c, int ldc, int m, int n, int k, int accumulate, void* stream);
/* Same product with B treated as a WEIGHT matrix, the way the episode calls it: its bf16x3 image
 * (what marl_pack_weights builds inside the weights workspace) is built in image_scratch
 * (>= marl_gemm_weight_image_bytes(n, k), 256-byte aligned, must stay valid until the product ran)
 * and the bf16x6 kernel copies its tiles instead of splitting them.  With the knob mfma_split = 0
 * this is marl_gemm_nt. */
int marl_gemm_nt_weights(const float* a, int lda, const float* b, int ldb, const float* bias,
                         float* c, int ldc, int m, int n, int k, int accumulate,
                         void* image_scratch, void* stream);
size_t marl_gemm_weight_image_bytes(int n, int k);
/* C[NI,NJ] = sum_r A[r,i] * B[r,j] over `rows` rows; scratch >= marl_gemm_tn_scratch(). */
int marl_gemm_tn(const float* a, int lda, const float* b, int ldb, float* c, int ldc,
                 int ni, int nj, int64_t rows, float* scratch, size_t scratch_bytes, void* stream);
size_t marl_gemm_tn_scratch(int ni, int nj, int64_t rows);
/* ---- image GEMMs (csrc/gemm3.hip): the form the episode uses for its large products ----
 * A "k16 image" of an fp32 matrix [rows][k] is [rows][ceil(k/16)][3][16] bf16: every element split
 * into three bf16 terms x0 + x1 + x2 == x, K zero-padded to a whole 16-deep step (96 bytes per row
 * and step).  marl_image_build makes one from an fp32 matrix (ld >= k); inside the episode the
 * PRODUCER kernels write the images of their outputs directly.  16-byte aligned. */
size_t marl_image_bytes(int64_t rows, int k);
int marl_image_build(const float* src, int ld, int64_t rows, int k, void* image, void* stream);
/* C[M,N] (+)= A * B^T + bias from the images of A [M,K] and B [N,K] (six bf16 MFMA products per fp32
 * product, fp32 accumulation - same arithmetic as marl_gemm_nt with mfma_split = 1).
 * variant: 0 = automatic tile plan (1 / 2 / 3 force 256x128, 128x128, 128x64 tiles - tools only). */
int marl_gemm_nt_images(const void* a3, const void* b3, const float* bias, float* c, int ldc, int m, int n,
                        int k, int accumulate, int variant, void* stream);
int marl_gemm_nt_images_batch(int count, const void* const* a3, const void* const* b3, float* const* c,
                              const int* n, const int* ldc, int m, int k, int accumulate, int variant,
                              void* stream);
/* nn.LSTMCell (networks/recurrent.py:19-35) from images: gates = U * W_ih^T + H * W_hh^T + bias (rows of
 * the weight images g * n + unit, g = i,f,g,o; bias = b_ih + b_hh), c' = s(f) c + s(i) tanh(g),
 * h' = s(o) tanh(c'); gates (nullable) receives the activated gates [M, ld_gates]; h3_next (nullable)
 * the image of h'. */
int marl_lstm_images(const void* u3, int nin, const void* h3, const void* wih3, const void* whh3,
                     const float* bias, const float* c_prev, float* h_next, float* c_next, float* gates,
                     void* h3_next, int m, int n, int ld_state, int ld_gates, int variant, int cells,
                     void* stream);
/* C[NI,NJ] = sum_r A[r,i] * B[r,j] from the images of A [rows,NI] and B [rows,NJ] (rows % 32 == 0);
 * colsum (nullable) [NI] = column sums of A (the matching bias gradient). */
size_t marl_gemm_tn_images_scratch(int ni, int nj, int64_t rows);
int marl_gemm_tn_images(const void* a3, const void* b3, float* c, int ldc, int ni, int nj, int64_t rows,
                        float* colsum, float* scratch, size_t scratch_bytes, void* stream);
/* Both weight gradients of one LSTM cell (backward of networks/recurrent.py:19-35 through loss.backward(),
 * training/trainer.py:115): C_ih [NI, NIH] = G^T U and C_hh [NI, NHH] = G^T H from the images of the gate gradients
 * G [rows, NI], of U [rows, NIH] and of H [rows, NHH]; colsum (nullable) [NI] = column sums of G (the bias
 * gradient).  One launch whose workgroups share G's row slabs through an XCD's L2: G leaves HBM once.
 * marl_gemm_tn_images_cell_scratch returns 0 for shapes outside this plan (NI < 256, rows < 8192, more than four
 * column tiles): use marl_gemm_tn_images for those. */
size_t marl_gemm_tn_images_cell_scratch(int ni, int nih, int nhh, int64_t rows);
int marl_gemm_tn_images_cell(const void* g3, int ni, const void* u3, int nih, const void* h3, int nhh, int64_t rows,
                             float* c_ih, int ld_ih, float* c_hh, int ld_hh, float* colsum, float* scratch,
                             size_t scratch_bytes, void* stream);
int marl_ln_silu_fwd(const float* z, int ldz, const float* gamma, const float* beta,
                     float* out, int ldo, float* stats, int m, int n, void* stream);

/* Convolution weight gradient from the activations (the kernel behind the conv layers'
 * dW in marl_episode_backward; backward of networks/vision.py:33-35 for Conv2d(k3,s2,p1)):
 *   dw[co][tap*cin+ci] = sum over rows r, output positions of dz[r][pos][co] * in[r][window(pos,tap)][ci]
 * in = the raw patch img[r % nb][:cin][pos[r] + ...] when zin == NULL (first layer), else
 * SiLU(GroupNorm(zin[r])) with the saved statistics gst[r][G][2] (mean, rstd) and affine.
 * dz [rows][hout*hout][cout]; zin [rows][hin*hin][cin]; dw [cout][9*cin]; db [cout] = column
 * sums of dz.  scratch >= marl_cnn_wgrad_scratch() bytes. */
int marl_cnn_wgrad(const float* dz, const void* img, int img_u8, const int32_t* pos,
                   const float* zin, const float* gst, const float* gamma, const float* beta,
                   int64_t rows, int nb, int c_img, int h, int w, int cin, int cout, int hin,
                   int groups, float* dw, float* db, float* scratch, size_t scratch_bytes,
                   void* stream);
size_t marl_cnn_wgrad_scratch(int64_t rows, int cin, int cout, int hin, int groups, int first);

/* Perf-experiment hook: overrides an internal tuning knob (same names as the MARL_<KEY>
 * environment variables, lower case, e.g. "dgrad_min_chunks", "mfma_split"); tools/ and tests only.
 * A key outside the library's table of knobs (csrc/rowops.hip, kKnownKnobs) returns MARL_EINVAL and sets nothing.
 * Several knobs change the LAYOUT of the episode workspace (tile plans, split-K targets,
 * mfma_split ...): marl_workspace_sizes() must be asked again and the workspace re-allocated
 * after such a call; a stale buffer is refused with MARL_ESIZE (ABI 3: sizes are passed in).  (The
 * Python wrapper marlclassification_amd.engine.tune() drops every cached workspace.) */
int marl_tune(const char* key, int value);
/* current value of a knob (marl_tune value, else MARL_<KEY>, else dflt) */
int marl_tune_get(const char* key, int dflt);

/* Measurement hook (bench.py roofline): time every launch of one kernel class with HIP
 * events recorded on the launch stream.  class 0 = fused LSTM-cell GEMM, 1 = plain NT GEMM,
 * 2 = row-contraction (weight-gradient) GEMM, 3 = fused CNN forward, 4 = row-panel MLP kernels,
 * 5 = CNN backward (layer backward + weight gradients).  marl_profile_end synchronises those events
 * and returns the summed kernel time and the number of launches seen. */
int marl_profile_begin(int kernel_class, int max_launches);
int marl_profile_end(double* total_ms, int* launches);

/* test hook: float offset and leading dimension of a named per-step activation inside
 * episode_ws ("U","H","C","HC","CC","MSG","PROBS","COLS0","Z0","GB","DU","DH","DHC"), or - "WP<i>" /
 * "WT<i>" - of the packed / transposed fp32 copy of parameter slot i inside weights_ws; "WPF<i>" / "WTF<i>" - of the
 * panel kernels' fragment-order copy of that packed / transposed copy (ld = its 16-deep K groups per tile; error if
 * the slot has none). */
int marl_debug_buffer(const marl_config* cfg, int train, const char* name, int t,
                      int64_t* offset_floats, int* ld);

/* Which kernel family the library picks for `cfg` under the current knobs (bench.py's `matrix_products`
 * note, tests): key "g3" = the large matrix products of this batch run on operand images (gemm3.hip),
 * "g3_model" = the weights workspace holds the k16 weight images (a property of the MODEL and the knobs only:
 * the weights layout never moves with the batch), "g3_tn" = the four large weight gradients run on images,
 * "g3_lstm" = the fused LSTM launch does, "lstm_plan" = the tile plan that launch takes (the launcher's own rule: 2 =
 * 128-row tiles, 3 / 4 = the gate-split small-batch plans, 1 / 5 / 6 by knob), "small_r" = lstm_plan is 3 or 4,
 * "g3_tn_cell" = both weight gradients of an LSTM cell come from one launch, "g3_tn_pipe" = the row contractions run
 * the phase-pipelined step, "wgrad3" = conv weight gradients (cin >= 16) on the bf16 pipe, "panel_sample" = the episode
 * forward samples step t's actions inside the chained panel launch, as the epilogue of its policy workgroups (no
 * sample_kernel launch; at most four actions; MARL_PANEL_SAMPLE=0 in the environment, read once, restores the
 * separate launch - same results bit for bit), "panel_static" = the chained panel launches of the episode, forward and
 * backward, take the static-shape kernels (the README widths 256 -> 128 -> 64 | mean | 64 -> 128 -> 96, policy 256 ->
 * 384, four actions, n_d a multiple of 4 (the README's 16); no communication graph, no exploration controls; MARL_PANEL_STATIC=0 in the
 * environment, read once, keeps the run-time-shape kernels - same results bit for bit).
 * *value = 0 / 1 (a plan number for "lstm_plan").
 * "g3_tn_pipe" and "wgrad3" report what runs, not the knob: the first is 0 where the image weight gradients are off,
 * the second is 0 unless some conv layer of the model takes cnn_wgrad3_kernel.
 * The CNN launchers' plans, each from the launcher's own routine (host arithmetic only, no GPU needed):
 *   "cnn_fwd"         0 = the unfused path (im2col + GEMM + row kernels); 1..5 = the cnn_fwd2_kernel / cnn_fwd3_kernel
 *                     instantiation (1 Resisc f = 12, 2 / 3 Mnist f = 6 / 12, 4 / 5 Aid f = 24 / 32); 6 = the general
 *                     cnn_fwd_kernel (`train` counts here: im2col rows kept for backward rule out 1..5)
 *   "cnn_fwd_rb"      patches per chunk of that launch (0 on the unfused path)
 *   "cnn_fwd_blocks"  its grid; cnn_fwd_blocks < ceil(R / cnn_fwd_rb) means workgroups walk several chunks
 *   "cnn_dgrad_rb<l>" conv layer l >= 1: patches per chunk of the fused layer backward, 0 = the col2im fallback
 *   "cnn_wgrad_rb<l>", "cnn_wgrad_chunks<l>", "cnn_wgrad_blocks<l>"  conv layer l >= 0: patches per chunk, chunks and
 *                     workgroups of the activation-based weight gradient (blocks: the device-independent upper bound;
 *                     the launch trims it to what is resident), all 0 where the layer takes the im2col GEMM instead. */
int marl_plan_query(const marl_config* cfg, int train, const char* key, int* value);

#ifdef __cplusplus
}
#endif
#endif /* MARL_HIP_H */
