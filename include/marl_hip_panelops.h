/*
 * marl_hip_panelops.h - kernel-level hooks of libmarl_hip.so for the row-panel kernels (csrc/panel.hip):
 * one launch_panel_fwd / launch_panel_bwd each, with the fragment-order weight copies built from row-major
 * weights by the product's own routine.  Tests and measurement only: the product reaches these kernels through
 * marl_episode_forward / marl_episode_backward and the step entries.  They are not part of the C ABI that
 * include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports): a caller of that ABI needs
 * none of them, and they may change with the kernels.  Conventions (error codes, marl_last_error, streams) are
 * those of marl_hip.h.
 *
 * Not served here (the entries refuse them; they have bit-for-bit tests against their separate-launch forms):
 * the sampling epilogue and the ride-along sampling workgroups, exploration controls, the position gate.
 *
 * Every pointer that the kernels read or write 16 bytes at a time must be 16-byte aligned and its leading
 * dimension a multiple of 4: x, xbar, da, da2, dx, and a cell's dh, dc, gates, c_prev, c_new where its
 * four-wide form is to run.  Rows of x / da are read up to the next multiple of 4 columns (ldx >= round4(k0)).
 * A refused call returns an error with nothing enqueued.
 */
#ifndef MARL_HIP_PANELOPS_H
#define MARL_HIP_PANELOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARL_PANEL_MAX_LAYERS 4
#define MARL_PANEL_MAX_SLICES 12

/* One Linear-LayerNorm-SiLU layer of a forward chain (PanelLayer): w [n][ldw] row-major, ldw >= the layer's
 * input width; z [m][ldz] (pre-LayerNorm) and stats [m][2] (mean, rstd) optional; a [m][lda] required.
 * a3 optional: the k16 image (marl_image_build's format, a3_steps 16-deep steps) that also receives the
 * activations at image row a3_row0 + r, column a3_col0 + c (n and a3_col0 multiples of 4). */
typedef struct marl_panel_layer {
    const float* w;
    int ldw;
    const float* bias;
    const float* gamma;
    const float* beta;
    int n;
    float* z;
    int ldz;
    float* stats;
    float* a;
    int lda;
    void* a3;
    int a3_row0, a3_steps, a3_col0;
} marl_panel_layer;

/* One problem of a forward launch (PanelFwdProb).  agg_na > 0: x is the message tensor [agg_na * agg_nb][ldx] and
 * the mean over the other agents is taken while staging (kept in xbar [m][ldx] when non-null).  by_batch > 0: a
 * workgroup owns all g_na agents of by_batch images (rows a * g_nb + b, m = g_na * g_nb); by_batch < 0: what the
 * episode would use for g_na agents.  agg_at = l > 0 aggregates layer l's input inside the workgroup (mean, or
 * mix [g_na][g_na], row = receiver) and keeps it in xbar [m][ld_xbar].  sample / explore / gate_pos must be 0. */
typedef struct marl_panel_fwd_prob {
    const float* x;
    int ldx, k0, m, nlayers;
    marl_panel_layer layer[MARL_PANEL_MAX_LAYERS];
    int agg_na, agg_nb;
    float* xbar;
    int by_batch, g_na, g_nb, agg_at, ld_xbar;
    const float* mix;
    int sample, explore;
    const void* gate_pos;
} marl_panel_fwd_prob;

/* Mirror of LstmBwdArgs: gates [rows][ldg] holds the activated i, f, g, o (n columns each) on entry and the
 * pre-activation gradients on exit, dc dL/dc_t on entry and dL/dc_{t-1} on exit; g3 optional image of the gate
 * gradients [rows][4 n] at image row g3_row0 + r; skip_f32: the fp32 gate gradients are not written where the
 * image is (the launcher clears it where the image is not written). dh is read by the ride-along cell only. */
typedef struct marl_panel_cell {
    const float* dh;
    float* dc;
    float* gates;
    const float* c_prev;
    const float* c_new;
    int lddh, lddc, ldg, ldc, n;
    void* g3;
    int g3_row0, g3_steps, skip_f32;
} marl_panel_cell;

/* One layer of a backward chain (PanelBwdLayer), listed from the LAST layer to the first: w [n][ldw] row-major
 * (the forward weight; ldw >= k_in), dz [m][lddz] out, part [workgroups][2][n] out (dgamma | dbeta partials;
 * workgroups = marl_panel_plan's blocks). */
typedef struct marl_panel_bwd_layer {
    const float* z;
    int ldz;
    const float* stats;
    const float* gamma;
    const float* beta;
    int n, k_in;
    const float* w;
    int ldw;
    float* dz;
    int lddz;
    float* part;
} marl_panel_bwd_layer;

/* One backward launch (PanelBwdProb).  da [m][ldda] (+ da2) is the gradient of layer[0]'s output; agg_na > 0:
 * da is the gradient of the message mean, the (self-adjoint) mean is applied while staging.  dx [m][lddx]
 * receives (accumulate: adds) the gradient of the first layer's input.  cellb (has_cellb, cellb.n == the last
 * listed layer's k_in): cell backward on the finished dx in the epilogue.  cell (has_cell): an independent cell
 * of cell_rows rows riding along.  cellb_img_done / cell_img_done are written by the call: the images asked for
 * were written by this launch. */
typedef struct marl_panel_bwd_prob {
    const float* da;
    int ldda;
    const float* da2;
    int ldda2;
    int agg_na, agg_nb, m, nlayers;
    marl_panel_bwd_layer layer[MARL_PANEL_MAX_LAYERS];
    float* dx;
    int lddx, accumulate;
    int by_batch, g_na, g_nb, agg_at;
    const float* mix;
    int has_cellb;
    marl_panel_cell cellb;
    int has_cell;
    marl_panel_cell cell;
    int64_t cell_rows;
    const void* gate_pos;
    int cellb_img_done, cell_img_done;
} marl_panel_bwd_prob;

/* What the launchers decide (their own routines; host arithmetic only, no GPU needed, no pointer dereferenced
 * beyond the descriptors).  Forward: per layer (problem 0's layers, then problem 1's) the waves the layer asks for,
 * column tiles nt, K slices ks, slice length kper and the bit mask of empty slices (kbeg >= round16(K)).
 * Backward: per listed layer the same for its dX product (contraction over n, tiles over k_in) and rounds = 1
 * where the tiles are walked in rounds; maxc (2 or 6 LayerNorm column slots), tail_lds after the retry, retried,
 * cell_vec4 and the two img_done flags. */
typedef struct marl_panel_plan_info {
    int waves, lds_bytes, blocks, cell_blocks, by_batch[2];
    int nlayers;
    int layer_waves[2 * MARL_PANEL_MAX_LAYERS], nt[2 * MARL_PANEL_MAX_LAYERS], ks[2 * MARL_PANEL_MAX_LAYERS];
    int kper[2 * MARL_PANEL_MAX_LAYERS], empty[2 * MARL_PANEL_MAX_LAYERS], rounds[2 * MARL_PANEL_MAX_LAYERS];
    int ln_slots[2 * MARL_PANEL_MAX_LAYERS];
    int maxc, tail_lds, retried, cell_vec4, cellb_img_done, cell_img_done;
} marl_panel_plan_info;

/* Bytes of scratch marl_panel_fwd (backward == 0: layers' [n, K] copies) or marl_panel_bwd (backward != 0: the
 * [k_in, n] copies plus a row-major transpose of each weight) needs for a chain of nlayers layers, n[l] wide with
 * inputs k[l] wide: per copy (ceil(n / 32) * ceil(K / 16) + 3) * 512 floats - the three 16-deep groups of zero
 * slack behind the last tile are what the kernels' unclamped loads rely on.  0 on a bad argument. */
size_t marl_panel_scratch_bytes(int backward, int nlayers, const int* n, const int* k);

/* One launch_panel_fwd of count (1 or 2) problems.  scratch (16-byte aligned) must hold the sum of the problems'
 * marl_panel_scratch_bytes (MARL_ESIZE otherwise); it is zeroed and filled on the stream ahead of the launch. */
int marl_panel_fwd(const marl_panel_fwd_prob* probs, int count, float* scratch, size_t scratch_bytes, void* stream);
/* One launch_panel_bwd. */
int marl_panel_bwd(marl_panel_bwd_prob* prob, float* scratch, size_t scratch_bytes, void* stream);
/* Exactly one of fwd (with count) and bwd is non-null; the same checks as the two entries, nothing enqueued. */
int marl_panel_plan(const marl_panel_fwd_prob* fwd, int count, const marl_panel_bwd_prob* bwd,
                    marl_panel_plan_info* out);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_PANELOPS_H */
