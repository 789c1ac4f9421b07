/*
 * marl_hip_normalize.h - per-image input normalisation of libmarl_hip.so: the statistics of every image of a batch
 * (a reduction over image planes, two launches) and the affine map that standardises it (one launch), both reading
 * rows of a resident image set (or an uploaded batch) like the batch gathers of marl_hip_augment.h.  The entries live
 * beside the C ABI that include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports) and change
 * none of it.  Conventions (error codes, marl_last_error) are those of marl_hip.h.
 *
 * Definition.  With x the pixel as stored (uint8 0..255, or fp32), N the number of pixels a statistic covers,
 * S1 = sum x, S2 = sum x^2, mean = S1 / N and std = sqrt((N S2 - S1^2) / (N (N - 1))) (the unbiased estimator):
 *
 *   mode                      statistic over          scale64                  offset64
 *   MARL_NORM_NORMAL          the image, N = c h w    1 / std                  -mean / std
 *   MARL_NORM_CHANNEL_NORMAL  a plane, N = h w        the same, per channel
 *   MARL_NORM_MINMAX          the image               1 / (max - min)          -min / (max - min)
 *   MARL_NORM_CHANNEL_MINMAX  a plane                 the same, per channel
 *   MARL_NORM_USER_NORMAL     none; user[ch] = (m, s)    1 / (255 s)           -m / s
 *   MARL_NORM_USER_MINMAX     none; user[ch] = (lo, hi)  1 / (255 (hi - lo))   -lo / (hi - lo)
 *
 * (uint8; ToTensor's 1 / 255 is folded in - it cancels in every statistic mode.  fp32 sources: drop the 255.)  Both are
 * fp64 expressions rounded once to fp32, and dst = fadd_rn(fmul_rn((float)x, scale), offset): the product and the sum
 * are rounded separately.  For uint8 sources S1, S2, min, max are integers and N S2 - S1^2 is formed exactly in 64-bit
 * integers (c h w <= 2^23 keeps it below 2^62) and converted to fp64 once; whole-image modes add the channels' records
 * first.  A constant image or plane (std == 0, max == min, N == 1) has scale = offset = 0: the plane becomes zeros (the
 * torch expression gives NaN / inf there).  Non-finite fp32 pixels are outside the definition: the output of that image
 * is unspecified; every address stays in bounds.
 * Nothing in device memory is trusted: rows[b] is clamped to [0, n_src).
 */
#ifndef MARL_HIP_NORMALIZE_H
#define MARL_HIP_NORMALIZE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARL_NORM_NORMAL 0
#define MARL_NORM_CHANNEL_NORMAL 1
#define MARL_NORM_MINMAX 2
#define MARL_NORM_CHANNEL_MINMAX 3
#define MARL_NORM_USER_NORMAL 4
#define MARL_NORM_USER_MINMAX 5
#define MARL_NORM_MAX_USER_CHANNELS 16 /* user[] travels by value in the kernel arguments */
#define MARL_NORM_RECORD_BYTES 32      /* (S1, S2, min, max): four int64 (uint8 sources) or four fp64 (fp32 sources) */
#define MARL_NORM_MAX_STAT_PIXELS (1 << 23) /* c h w of a uint8 image whose statistics are taken */

/* What the launchers do for one shape and pointer pair (host arithmetic, nothing is launched).
 * Statistics: a workgroup of 256 threads reduces chunk_elems consecutive elements of ONE plane (the last chunk of a
 *   plane is shorter) with loads of load_bytes bytes at aligned addresses - the unaligned head and tail of a chunk go
 *   per element - and writes one record; a plane has partials_per_plane of them, folded in ascending order.
 * Apply: a workgroup writes apply_chunk_elems consecutive pixels of one plane (apply_blocks_per_plane per plane) with
 *   stores of store_bytes bytes: the widest of 16 / 8 / 4 that divides a plane's h w 4 bytes and dst's address. */
typedef struct marl_normalize_plan_info {
    int32_t chunk_elems;
    int32_t partials_per_plane;
    int32_t load_bytes;
    int32_t lds_bytes;
    int32_t store_bytes;
    int32_t apply_chunk_elems;
    int32_t apply_blocks_per_plane;
    int32_t reserved;
} marl_normalize_plan_info;

/* src may be NULL (reads take any alignment the element allows), dst may be NULL (store_bytes is then 16 / 8 / 4 by
 * the plane's size alone).  MARL_EINVAL / MARL_ELIMIT as marl_batch_normalize. */
int marl_batch_normalize_plan(int c, int h, int w, int elt_bytes, const void* src, const void* dst,
                              marl_normalize_plan_info* out);

/* Bytes of the partial records between the two launches of marl_batch_stats; 0 for sizes it refuses. */
size_t marl_batch_stats_scratch_bytes(int batch, int c, int h, int w, int elt_bytes);

/* records[b, ch] = (S1, S2, min, max) of plane ch of src[rows[b]], b < batch: src is [n_src, c, h, w] contiguous,
 * elt_bytes 1 (uint8; four int64 per record) or 4 (fp32; S1 and S2 summed in fp64, min / max exact, four fp64 per
 * record).  rows == NULL: rows[b] = b (n_src >= batch is then required).  Two launches on `stream`: a partial pass
 * that reads every selected plane once and leaves one record per workgroup in `scratch`
 * (marl_batch_stats_scratch_bytes, 8-byte aligned), a fold pass that sums them in ascending order.  No atomics, no
 * memset; two calls on the same inputs give the same bytes.
 * MARL_EINVAL before anything is enqueued: a null src / scratch / records, elt_bytes neither 1 nor 4, a size that is
 * not positive, fp32 src not 4-byte aligned, scratch or records not 8-byte aligned.  MARL_ELIMIT: an image of 2^31
 * bytes or more, more workgroups than a grid holds, a uint8 image of more than MARL_NORM_MAX_STAT_PIXELS pixels. */
int marl_batch_stats(const void* src, int64_t n_src, const int64_t* rows, int batch, int c, int h, int w,
                     int elt_bytes, void* scratch, void* records, void* stream);

/* dst[b, ch, y, x] (fp32, [batch, c, h, w] contiguous) = the definition above of src[rows[b], ch, y, x]; one launch.
 * records: those of marl_batch_stats for the same (src, rows, batch) - NULL for the user modes, which launch nothing
 * else.  user: MARL_NORM_USER_*: c pairs of host doubles, c <= MARL_NORM_MAX_USER_CHANNELS; ignored otherwise.  Every
 * workgroup derives its plane's (scale, offset) from the records in fp64 and rounds them once; coef (nullable, fp32
 * [batch, c, 2], 4-byte aligned) receives the pairs.
 * MARL_EINVAL before anything is enqueued: a null src / dst (records for a statistic mode, user for a user mode),
 * an unknown mode, elt_bytes neither 1 nor 4, a size that is not positive, c > 16 for a user mode, s == 0 or hi == lo
 * (or a value that is not finite) in user, dst overlapping [src, src + n_src c h w elt_bytes), misaligned src (fp32),
 * dst, records or coef.  MARL_ELIMIT: as marl_batch_stats (the pixel bound: statistic modes only), or a dst image of
 * 2^31 bytes or more. */
int marl_batch_normalize(const void* src, int64_t n_src, const int64_t* rows, const void* records, int mode,
                         const double* user, int batch, int c, int h, int w, int elt_bytes, float* dst, float* coef,
                         void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_NORMALIZE_H */
