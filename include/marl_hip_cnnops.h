/*
 * marl_hip_cnnops.h - kernel-level hooks of libmarl_hip.so for the convolution kernels (csrc/cnn.hip): the fused
 * extractor forward as one step of an episode launches it, the fused layer backward with its affine reduction, and
 * the plans the conv launchers choose.  Tests and measurement only: the product reaches these kernels through
 * marl_episode_forward / marl_step_forward and marl_episode_backward / marl_step_backward.  Like
 * include/marl_hip_rowops.h they are not part of the C ABI that include/marl_hip.h declares and versions
 * (MARL_ABI_VERSION, its list of exports) and may change with the kernels.  Conventions (error codes,
 * marl_last_error, streams, marl_config) are those of marl_hip.h.  The weight gradient has its entry in the ABI
 * already (marl_cnn_wgrad).
 */
#ifndef MARL_HIP_CNNOPS_H
#define MARL_HIP_CNNOPS_H

#include <stddef.h>
#include <stdint.h>

#include "marl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The fused extractor forward (networks/vision.py:13-53 on the patches of core/environment.py:95-126) - the one launch
 * the CNN phase of a step makes (cnn_fwd_kernel, cnn_fwd2_kernel<..> or cnn_fwd3_kernel<..>, by the launcher's rule),
 * its arguments filled by the routine the episode fills them with, and nothing else.
 *   cfg          the model (cnn_*, window), the image size (img_c / img_h / img_w, img_u8) and batch = the number of
 *                images; nb_agents and nb_steps do not enter: the rows are given explicitly
 *   weights_ws   what marl_pack_weights wrote (packed conv weights with their zeroed K padding, the affines, the
 *                fragment-order copies the AidCnn plans stream), 256-byte aligned
 *   io->img + io->pos   [batch][img_c][img_h][img_w] fp32 or uint8 (cfg->img_u8) and int32 [rows][2]: row r reads
 *                image r % batch at pos[r]; rows need not be a multiple of batch.  Or
 *   io->obs      [rows][img_c][f][f] fp32 patches (the single-step API; wins over img when both are given)
 *   io->u, ldu   out [rows][ldu]: columns [0, nf) = the features, index c * P_last + p; the others are not touched.
 *                ldu >= nf, ldu % 4 == 0
 *   io->z[l]     out [rows][P_l][cout_l] conv outputs (pre-norm, NHWC), io->gst[l] out [rows][groups_l][2] (mean, rstd),
 *   io->cols[l]  out [rows * P_l][ldk_l] im2col rows, k = tap * cin + ci, ldk = 9 * cin rounded up to 4: each null =
 *                not kept.  A layer whose rows are kept takes the general kernel (marl_cnn_fwd_plan, keeps_cols).
 *   io->u3       optional: the k16 image (marl_image_build's format) of a matrix of u3_steps 16-deep steps whose rows
 *                u3_row0 .. u3_row0 + rows - 1 receive the features too; only where the plan writes_image
 * u, z, gst, cols and u3 must be 16-byte aligned.  MARL_EINVAL: a null or misaligned pointer the launch would use, u3
 * where the selected kernel does not write it; MARL_ESIZE: weights_ws_bytes below what the model needs; MARL_ELIMIT,
 * nothing enqueued: the fused forward does not cover the model (the episode then takes its GEMM path). */
typedef struct marl_cnn_fwd_io {
    const void* img;
    const int32_t* pos;
    const float* obs;
    int64_t rows;
    float* u;
    int32_t ldu;
    float* z[MARL_MAX_CNN_LAYERS];
    float* gst[MARL_MAX_CNN_LAYERS];
    float* cols[MARL_MAX_CNN_LAYERS];
    void* u3;
    int32_t u3_row0, u3_steps;
} marl_cnn_fwd_io;
int marl_cnn_fwd(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes, const marl_cnn_fwd_io* io,
                 void* stream);

/* What the CNN phase of a step does with `rows` rows of this model under the current knobs - host arithmetic only (no
 * GPU needed), each field from the routine the launcher itself calls; what marl_plan_query reports as cnn_fwd* for
 * rows = nb_agents * batch.  train != 0: a training launch (the layers' outputs are kept).
 *   fused        the one-launch forward covers the model (0: every other field is 0)
 *   which        1..3 = cnn_fwd2_kernel<Fwd2Resisc | Fwd2Mnist6 | Fwd2Mnist12>, 4 / 5 = cnn_fwd3_kernel<Fwd3Aid24 |
 *                Fwd3Aid32>, 6 = cnn_fwd_kernel;   rb = patches per chunk;   blocks = the grid (blocks < ceil(rows /
 *                rb): workgroups walk several chunks)
 *   keeps_cols[l]   the launch keeps layer l's im2col rows (a weight gradient the activation-based kernel does not cover)
 *   writes_image    the selected kernel honours io->u3 */
typedef struct marl_cnn_fwd_plan_info {
    int32_t fused, which, rb, blocks;
    int32_t keeps_cols[MARL_MAX_CNN_LAYERS];
    int32_t writes_image;
} marl_cnn_fwd_plan_info;
int marl_cnn_fwd_plan(const marl_config* cfg, int train, int64_t rows, marl_cnn_fwd_plan_info* out);

/* Backward of one Conv2d(3, stride 2, pad 1) down to the conv output of the layer below, through that layer's
 * GroupNorm + SiLU (networks/vision.py:33-38 through loss.backward(), training/trainer.py:115) - one
 * cnn_dgrad_kernel launch and its affine reduction, as marl_episode_backward runs them per layer:
 *   dz    [rows][P][cout]      gradient of this layer's conv output, P = hout^2, hout = (hin - 1) / 2 + 1
 *   wt    [9 * cin][ldwt]      this layer's weight, transposed as marl_pack_weights keeps it:
 *                              wt[(kh * 3 + kw) * cin + ci][co] = W[co][ci][kh][kw]; ldwt >= cout, ldwt % 4 == 0
 *   zin   [rows][hin^2][cin]   conv output (pre-norm) of the layer below, NHWC
 *   gst   [rows][groups][2]    its GroupNorm statistics (mean, rstd); gamma, beta [cin] its affine
 *   dzin  [rows][hin^2][cin]   out: gradient of zin;   dgamma, dbeta [cin]   out (overwritten)
 * dz, wt, zin and dzin must be 16-byte aligned.  scratch holds the per-workgroup partial sums and is consumed:
 * marl_cnn_dgrad_scratch bytes always suffice (a device-independent bound), a smaller buffer returns MARL_ESIZE.
 * MARL_ELIMIT, nothing enqueued, where the fused kernel does not cover the shape (cin or cout no multiple of 4,
 * groups not dividing 8, cin / groups no power of two <= 64, no chunk that fits LDS): the episode then takes its
 * GEMM + col2im path. */
int marl_cnn_dgrad(const float* dz, const float* wt, int ldwt, const float* zin, const float* gst,
                   const float* gamma, const float* beta, float* dzin, float* dgamma, float* dbeta, float* scratch,
                   size_t scratch_bytes, int64_t rows, int cin, int cout, int hin, int groups, void* stream);
/* bytes of scratch marl_cnn_dgrad needs for these shapes under the current knobs (0: shape not covered) */
size_t marl_cnn_dgrad_scratch(int64_t rows, int cin, int cout, int hin, int groups);

/* What the conv backward launchers choose for one layer shape under the current knobs - host arithmetic only (no
 * GPU needed), each field read from the launcher's own routine.  first != 0: the first layer (cin image channels,
 * hin = the window, groups ignored); it has no layer backward. */
typedef struct marl_cnn_bwd_plan_info {
    /* weight gradient (marl_cnn_wgrad): form 0 = not covered, 1 = cnn_wgrad_kernel<sct, skt, first, pd, pi> (fp32
     * MFMA), 3 = cnn_wgrad3_kernel<skt, pd, pi> (bf16x6); rb patches per chunk, chunks = ceil(rows / rb), blocks =
     * the bound of persistent workgroups per slab (the launch trims it to what is resident); wave roles tgc x tgk x
     * ms; slabs = k-slabs (grid.y) */
    int32_t wg_form, wg_rb, wg_chunks, wg_blocks, wg_sct, wg_skt, wg_tgc, wg_tgk, wg_ms, wg_slabs, wg_pd, wg_pi;
    /* layer backward (marl_cnn_dgrad): supported 0 / 1; rb patches per chunk, mt x nt 16-wide tiles of a chunk's
     * panel, blocks = ceil(rows / rb), the bound of the persistent grid */
    int32_t dg_supported, dg_rb, dg_mt, dg_nt, dg_blocks;
} marl_cnn_bwd_plan_info;
int marl_cnn_bwd_plan(int64_t rows, int cin, int cout, int hin, int groups, int first,
                      marl_cnn_bwd_plan_info* out);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_CNNOPS_H */
