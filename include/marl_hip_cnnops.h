/*
 * marl_hip_cnnops.h - kernel-level hooks of libmarl_hip.so for the convolution backward (csrc/cnn.hip): the fused
 * layer backward with its affine reduction, and the plans the conv backward launchers choose.  Tests and
 * measurement only: the product reaches these kernels through marl_episode_backward / marl_step_backward.  Like
 * include/marl_hip_rowops.h they are not part of the C ABI that include/marl_hip.h declares and versions
 * (MARL_ABI_VERSION, its list of exports) and may change with the kernels.  Conventions (error codes,
 * marl_last_error, streams) are those of marl_hip.h.  The weight gradient has its entry in the ABI already
 * (marl_cnn_wgrad).
 */
#ifndef MARL_HIP_CNNOPS_H
#define MARL_HIP_CNNOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

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
