/*
 * marl_hip_gemmops.h - host-only witness of the matrix-product launchers of libmarl_hip.so (csrc/gemm.hip,
 * csrc/gemm_split.hip, csrc/gemm3.hip): what a launcher does with a shape, answered by the planning routine the
 * launcher itself calls.  Tests and measurement only.  It is not part of the C ABI that include/marl_hip.h declares
 * and versions (MARL_ABI_VERSION, its list of exports): a caller of that ABI does not need it, and it may change
 * with the launchers.  Error codes and marl_last_error are those of marl_hip.h.
 */
#ifndef MARL_HIP_GEMMOPS_H
#define MARL_HIP_GEMMOPS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The launchers.  NT / LSTM / TN: fp32 operands (marl_gemm_nt, the LSTM launch of the GEMM path, marl_gemm_tn);
 * the *_IMAGES kinds: k16 operand images (marl_gemm_nt_images[_batch], marl_lstm_images, marl_gemm_tn_images,
 * marl_gemm_tn_images_cell). */
enum {
    MARL_GEMM_NT = 0,
    MARL_GEMM_LSTM = 1,
    MARL_GEMM_TN = 2,
    MARL_GEMM_NT_IMAGES = 3,
    MARL_GEMM_LSTM_IMAGES = 4,
    MARL_GEMM_TN_IMAGES = 5,
    MARL_GEMM_TN_IMAGES_CELL = 6
};

/* One struct for every kind; a field a kind does not have is 0. */
typedef struct marl_gemm_plan_info {
    int32_t kind;
    int32_t family;      /* NT, LSTM, TN: 0 = exact-fp32 kernels, 1 = bf16x6 kernels */
    int32_t variant;     /* image kinds: the id asked for or chosen (TN_IMAGES: the table row taken; cell: 5) */
    int32_t row_id;      /* NT_IMAGES, LSTM_IMAGES: id of the table row taken (0 = the row of every other id) */
    int32_t bm, bn;      /* tile: rows x columns of the output (TN kinds: columns of A x columns of B) */
    int32_t wm, wn, nst; /* NT_IMAGES, LSTM_IMAGES: waves along m / n, ring stages */
    int32_t pipelined;   /* NT_IMAGES, LSTM_IMAGES: the phase-pipelined kernel; TN_IMAGES[_CELL]: knob g3_tn_pipe applies */
    int32_t threads;     /* per workgroup */
    int32_t gx, gy, gz;  /* logical grid: tiles along the two output dimensions, then problems (NT) or row splits (TN) */
    int32_t blocks;      /* workgroups of the launch */
    int32_t xcd_map;     /* 1-D launch in the XCD-contiguous tile order */
    int32_t single_buf;  /* NT fp32: one LDS stage */
    int32_t pre;         /* NT / LSTM bf16x6: every B operand has a weight image within 32-bit offsets */
    int32_t safe;        /* NT_IMAGES, LSTM_IMAGES: knob g3_safe as the kernel takes it */
    int32_t splits;      /* TN kinds */
    int64_t rows_per_split;
    int32_t ok;          /* TN_IMAGES_CELL: the shape is inside the plan; when not, only kind, variant and pipelined
                          * (the knob, which does not depend on the shape) are set */
    int32_t teams;
    int32_t ih256, ih128, hh256, hh128; /* TN_IMAGES_CELL: column tiles of the two B operands */
    uint64_t lds_bytes;
    uint64_t scratch_bytes; /* TN kinds: what marl_gemm_tn_scratch / marl_gemm_tn_images[_cell]_scratch answer */
} marl_gemm_plan_info;

/* The plan of one launch; no HIP call is made.
 *   NT, LSTM, NT_IMAGES, LSTM_IMAGES: `count` problems of m[i] x n[i] (LSTM: n = hidden units) with one segment of
 *     depth k[i]; has_images != 0: every B operand carries its weight image (NT, LSTM only); variant: the variant
 *     argument of the image entries (0 = knob, then the automatic choice), ignored by the others.
 *   TN, TN_IMAGES: count = 1, C [m[0] x n[0]] = A^T B over `rows` rows.
 *   TN_IMAGES_CELL: count = 2, m[0] = m[1] = 4 * units, n[0] / n[1] = widths of U and of H.
 * k may be null (depth 1) where has_images == 0. */
int marl_gemm_plan(int kind, int count, const int* m, const int* n, const int* k, int64_t rows, int has_images,
                   int variant, marl_gemm_plan_info* out);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_GEMMOPS_H */
