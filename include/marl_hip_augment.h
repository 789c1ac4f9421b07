/*
 * marl_hip_augment.h - device-side augmentation fused into the batch gather of libmarl_hip.so: every output image is
 * one row of a resident image set (or of an uploaded batch) under a dihedral code (flips, quarter turns), an integer
 * shift with reflect or constant padding and one erased rectangle.  The entries live beside the C ABI that
 * include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports) and change none of it.
 * Conventions (error codes, marl_last_error) are those of marl_hip.h.
 *
 * Per output image b: a source row rows[b] and eight int32 ops[b] = (d4, dy, dx, ey, ex, eh, ew, 0).  Output pixel
 * (c, y, x) of an h x w image is
 *   1. fill, if ey <= y < ey + eh and ex <= x < ex + ew (eh == 0 or ew == 0: no rectangle);
 *   2. else with y' = y - dy, x' = x - dx:  MARL_AUGMENT_PAD_ZERO: fill where (y', x') lies outside the image;
 *      MARL_AUGMENT_PAD_REFLECT: v < 0 -> -v, v >= n -> 2 (n - 1) - v (torch's "reflect": the edge is not repeated);
 *   3. then the dihedral code: d4 & 1 swaps (y', x'), d4 & 2 sets x' = w - 1 - x', d4 & 4 sets y' = h - 1 - y';
 *   4. src[rows[b], c, y', x'].
 * Nothing in device memory is trusted: the kernel takes d4 & 7 (and drops bit 0 where h != w), clamps rows[b] to
 * [0, n_src), dy to [-(h - 1), h - 1], dx to [-(w - 1), w - 1], and intersects the rectangle with the image (in
 * 64-bit arithmetic), so no value of ops / rows reads or writes outside [src, src + n_src c h w elt) and dst.
 * augment.reference_apply (Python) applies the same rules.
 */
#ifndef MARL_HIP_AUGMENT_H
#define MARL_HIP_AUGMENT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARL_AUGMENT_PAD_ZERO 0
#define MARL_AUGMENT_PAD_REFLECT 1

/* What the launcher does for one shape and pointer pair (host arithmetic, nothing is launched).
 * store_bytes: bytes per lane of every global store - the widest of 16 / 8 / 4 that divides w * elt_bytes and both
 *   dst's address and (with it) every output row's; 1 for uint8 rows that are no multiple of 4 bytes.
 * Codes without bit 0 run as bands of band_vectors consecutive stores of one output image (rows are contiguous, so a
 * band is tile_h full rows of tile_w = w pixels, up to rounding); codes with bit 0 go through an LDS tile of
 * tr_tile x tr_tile pixels (lds_bytes, padded rows).  blocks_per_image workgroups of 256 threads serve either. */
typedef struct marl_augment_plan_info {
    int32_t store_bytes;
    int32_t band_vectors;
    int32_t tile_h, tile_w;
    int32_t tr_tile;
    int32_t lds_bytes;
    int32_t blocks_per_image;
    int32_t reserved;
} marl_augment_plan_info;

/* dst[b] = the transform above of src[rows[b]], b < batch; src is [n_src, c, h, w], dst [batch, c, h, w], both
 * contiguous, elt_bytes 1 (uint8) or 4 (any 32-bit type; fill_bits is the fill's bit pattern, its low byte for
 * elt_bytes 1).  rows == NULL: rows[b] = b (n_src >= batch is then required).  ops == NULL: all zeros - a plain row
 * gather.  rows, ops, src and dst are device pointers; one kernel on `stream` (a hipStream_t passed as void*,
 * as everywhere in marl_hip.h), no workspace, no atomics.
 * MARL_EINVAL (marl_last_error names batch_augment) before anything is enqueued: a null src / dst, elt_bytes neither 1
 * nor 4, an unknown pad_mode, a size that is not positive, dst overlapping [src, src + n_src c h w elt_bytes) (in
 * place is undefined for flips).  MARL_ELIMIT: an image of 2^31 bytes or more, or more workgroups than a grid holds. */
int marl_batch_augment(const void* src, int64_t n_src, void* dst, const int64_t* rows, const int32_t* ops, int batch,
                       int c, int h, int w, int elt_bytes, int pad_mode, uint32_t fill_bits, void* stream);

/* The plan of that launch for (c, h, w, elt_bytes) and the alignment of src / dst (src may be NULL: reads take any
 * alignment).  MARL_EINVAL / MARL_ELIMIT as above. */
int marl_batch_augment_plan(int c, int h, int w, int elt_bytes, const void* src, const void* dst,
                            marl_augment_plan_info* out);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_AUGMENT_H */
