/*
 * marl_hip_color.h - colour jitter of libmarl_hip.so: brightness, contrast, saturation and hue of every image of a
 * batch as ONE per-image colour matrix, applied in one launch that reads rows of a resident image set (or a batch a
 * gather made) like the batch gathers of marl_hip_augment.h.  The entries live beside the C ABI that
 * include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports) and change none of it.  Conventions
 * (error codes, marl_last_error) are those of marl_hip.h.
 *
 * Definition (marlclassification_amd/color.py: reference_matrix / reference_apply).  Per output image b a source row
 * rows[b] and eight int32 params[b] = (beta, kappa, sigma, hcos, hsin, 0, 0, 0): the brightness, contrast and
 * saturation factors in Q12 (4096 = 1.0) and the cosine and sine of the hue angle in Q14.  Nothing is trusted: the
 * factors are clamped to [0, 4 * 4096], hcos / hsin to [-16384, 16384], rows to [0, n_src).
 *
 * With g = (77, 150, 29) / 256 the grey weights (c == 1: g = (1)), G = 1 g^T, K = MARL_COLOR_K (the generator of the
 * YIQ chroma rotation T^-1 J T, every row summing to exactly 0) and m[ch] the mean of plane ch - uint8 sources:
 * ((256 S1[ch]) / N) / 256 with the quotient a 64-bit integer division of the record of marl_batch_stats, N = h w; fp32
 * sources: S1[ch] / N in fp64; the integer S1 is clamped to [0, 255 N] first - the matrix is composed in fp64 with
 * + - * only, every operation rounded, no contraction, in this order (products of matrices accumulate left to right:
 * (s0 m0 + s1 m1) + s2 m2):
 *
 *   M = I, o = 0
 *   brightness: M = beta M;  o = beta o
 *   contrast:   mu = g . (M m + o);  M = kappa M;  o = kappa o + (1 - kappa) mu 1     (records == NULL: skipped)
 *   saturation: S = sigma I + (1 - sigma) G;  M = S M;  o = S o                       (c == 3 only)
 *   hue:        H = (G + hcos (I - G)) + hsin K;  M = H M;  o = H o                   (c == 3 only)
 *
 * Pixels, uint8: A_q = clamp(rint(4096 M), +-2^19), o_q = clamp(rint(4096 o), +-2^30) (o in grey levels),
 * acc_i = sum_j A_q[i][j] x_j + o_q[i] in int32 (3 * 2^19 * 255 + 2^30 < 2^31), y_i = clamp((acc_i + 2048) >> 12, 0, 255)
 * with an arithmetic shift.  Pixels, fp32: M and o rounded once to fp32, y_i = ((a0 x0 (+) a1 x1) (+) a2 x2) (+) o_i,
 * every product and sum rounded separately; terms whose coefficient or offset is exactly 0 are skipped (a NaN behind a
 * zero stays where it is, the identity is a bit copy; a row of zeros gives +0); no clamp.
 *
 * Output forms.  MARL_COLOR_OUT_SAME: the source's element type.  MARL_COLOR_OUT_NORM (uint8 sources only): fp32
 * dst = fadd_rn(fmul_rn((float)y_i, scale_i), offset_i) with (scale, offset) the MARL_NORM_USER_NORMAL /
 * MARL_NORM_USER_MINMAX pair of marl_batch_normalize (marl_hip_normalize.h): bit for bit OUT_SAME followed by
 * marl_batch_normalize in that mode, in one launch and without the uint8 round trip.
 */
#ifndef MARL_HIP_COLOR_H
#define MARL_HIP_COLOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARL_COLOR_OUT_SAME 0
#define MARL_COLOR_OUT_NORM 1
#define MARL_COLOR_PARAMS 8          /* int32 per image */
#define MARL_COLOR_Q12 4096          /* 1.0 of beta, kappa, sigma */
#define MARL_COLOR_Q14 16384         /* 1.0 of hcos, hsin */
#define MARL_COLOR_MAX_FACTOR (4 * MARL_COLOR_Q12)

/* grey weights, in 256ths */
#define MARL_COLOR_G0 77
#define MARL_COLOR_G1 150
#define MARL_COLOR_G2 29

/* K = T^-1 J T for the NTSC RGB -> YIQ matrix T and the quarter turn J of the IQ plane, six decimals; the last entry
 * of a row is minus the fp64 sum of the other two, so every row sums to exactly 0 and grey is a fixed point. */
#define MARL_COLOR_K00 0.168622
#define MARL_COLOR_K01 0.329805
#define MARL_COLOR_K10 (-0.327963)
#define MARL_COLOR_K11 0.034611
#define MARL_COLOR_K20 1.246461
#define MARL_COLOR_K21 (-1.043229)
#define MARL_COLOR_K_LAST(a, b) (-((a) + (b)))

/* What marl_batch_color does for one shape, form and pointer pair (host arithmetic, nothing is launched): a workgroup
 * of 256 threads owns 256 * vectors_per_thread * pixels_per_vector consecutive pixels of ONE image (blocks_per_image of
 * them per image); a thread owns vectors_per_thread vectors, 256 vectors apart: per vector it reads load_bytes of each
 * of the c planes and writes store_bytes to each.  One matrix derivation serves all vectors of a thread. */
typedef struct marl_color_plan_info {
    int32_t load_bytes;
    int32_t store_bytes;
    int32_t pixels_per_vector;
    int32_t vectors_per_thread;
    int32_t blocks_per_image;
    int32_t lds_bytes; /* 0 */
    int32_t reserved[2];
} marl_color_plan_info;

/* src / dst may be NULL (taken as aligned).  OUT_SAME: the widest of 16 / 8 / 4 bytes that divides a plane's
 * h w elt_bytes bytes and both addresses, else one element.  OUT_NORM: 4 pixels (a 4-byte load, a 16-byte store) when
 * h w is a multiple of 4, src 4-byte and dst 16-byte aligned, else 1 pixel.  MARL_EINVAL / MARL_ELIMIT as
 * marl_batch_color. */
int marl_batch_color_plan(int c, int h, int w, int elt_bytes, int out_form, const void* src, const void* dst,
                          marl_color_plan_info* out);

/* dst[b] = the definition above of src[rows[b]], b < batch: src is [n_src, c, h, w] contiguous, elt_bytes 1 (uint8) or
 * 4 (fp32), c 1 or 3; rows == NULL: rows[b] = b (n_src >= batch is then required).  One launch on `stream`, no LDS, no
 * atomics.  records: those of marl_batch_stats for the same (src, rows, batch), NULL: no contrast (kappa is taken as
 * 1).  params: int32 [batch, 8].  out_form MARL_COLOR_OUT_NORM: dst is fp32, norm_mode MARL_NORM_USER_NORMAL or
 * MARL_NORM_USER_MINMAX and user its c pairs of host doubles (both ignored for OUT_SAME).  coef (nullable): the matrix
 * every workgroup derived, [batch, c, c + 1] (row i: A[i][0..c), o[i]) - int32 A_q / o_q for uint8 sources, fp32 for
 * fp32 sources.
 * MARL_EINVAL before anything is enqueued: a null src / dst / params, an unknown out_form, c neither 1 nor 3, elt_bytes
 * neither 1 nor 4, OUT_NORM with an fp32 source, a statistic norm_mode, a null user or s == 0 / hi == lo / a value
 * that is not finite in it, a size that is not positive, misaligned src (fp32), dst (its element), records (8), coef
 * (4), params (4) or rows (8), dst overlapping [src, src + n_src c h w elt_bytes).  MARL_ELIMIT: a source or
 * destination image of 2^31 bytes or more, more workgroups than a grid holds. */
int marl_batch_color(const void* src, int64_t n_src, const int64_t* rows, const void* records, const int32_t* params,
                     int out_form, int norm_mode, const double* user, int batch, int c, int h, int w, int elt_bytes,
                     void* dst, void* coef, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_COLOR_H */
