/*
 * marl_hip_warp.h - the resampling batch gather of libmarl_hip.so: every output image is one row of a resident image
 * set (or of an uploaded batch) under an affine map - rotation by any angle, zoom, aspect stretch, translation -
 * sampled bilinearly, with reflect or constant padding and one erased rectangle.  The entries live beside the C ABI
 * that include/marl_hip.h declares and versions (MARL_ABI_VERSION, its list of exports) and change none of it.
 * Conventions (error codes, marl_last_error) are those of marl_hip.h; the pad modes are those of marl_hip_augment.h.
 *
 * Per output image b: a source row rows[b] and eight int32 mats[b] = (a00, a01, a10, a11, ty, tx, 0, 0).  a.. is a Q16
 * matrix (65536 = 1.0) that maps OUTPUT pixels to SOURCE positions (the inverse warp), ty / tx are Q16 in units of
 * half pixels; the output has the source's c, h, w.  Nothing in device memory is trusted: rows[b] is clamped to
 * [0, n_src), each a to [-2^20, 2^20], each t to [-2^30, 2^30].  For output pixel (y, x), all in int64:
 *
 *   yc = 2 y - (h - 1)              xc = 2 x - (w - 1)                  (doubled, centred: integers)
 *   Sy = a00 yc + a01 xc + ty       Sx = a10 yc + a11 xc + tx
 *   py = (Sy + (h - 1) 65536) >> 1  px likewise with w                  (arithmetic shift; Q16 source pixels)
 *   py8 = (py + 128) >> 8;  y0 = py8 >> 8;  fy = py8 & 255              (x likewise: x0, fx; weights in 1 / 256)
 *
 * The four taps are (y0, x0), (y0, x0 + 1), (y0 + 1, x0), (y0 + 1, x0 + 1).  A tap outside the image:
 *   MARL_AUGMENT_PAD_ZERO: its value is fill;
 *   MARL_AUGMENT_PAD_REFLECT: each index v is folded, m = floormod(v, 2 (n - 1)), m >= n ? 2 (n - 1) - m : m, and
 *   n == 1 gives 0 (the fold of marl_batch_augment, at any distance).
 * elt_bytes 1 (uint8) blends in exact integers:
 *   top = v00 (256 - fx) + v01 fx;  bot = v10 (256 - fx) + v11 fx;  out = (top (256 - fy) + bot fy + 32768) >> 16
 * elt_bytes 4 is fp32, wx = fx / 256, wy = fy / 256:
 *   top = fl(fl(v00 (1 - wx)) + fl(v01 wx)), bot likewise;  out = fl(fl(top (1 - wy)) + fl(bot wy))
 * every product and sum rounded on its own (no contraction), and a tap of weight 0 is skipped, not multiplied: fx == 0
 * gives top = v00 exactly, fy == 0 gives out = top, and a NaN behind a zero weight stays out.
 * Last, the erased rectangle in OUTPUT space: fields 3 .. 6 (ey, ex, eh, ew) of ops[b], an op row in the layout of
 * marl_hip_augment.h, intersected with the image (in 64-bit arithmetic); fill wins inside it.  Fields 0 .. 2 of ops
 * are IGNORED here (a dihedral code or a shift belongs into the matrix: warp.compose_ops in Python).
 * So the identity matrix (65536, 0, 0, 65536, 0, 0) is a plain gather, and every view (d4, dy, dx) of
 * marl_batch_augment is a matrix of entries 0 / +-65536 with t = -+2 65536 d.  warp.reference_apply (Python) is this
 * definition in plain torch.
 */
#ifndef MARL_HIP_WARP_H
#define MARL_HIP_WARP_H

#include <stdint.h>

#include "marl_hip_augment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the launcher does for one shape and pointer pair (host arithmetic, nothing is launched).
 * store_bytes: bytes per lane of every global store - the widest of 16 / 8 / 4 that divides w * elt_bytes and both
 *   dst's address and (with it) every output row's; 1 for uint8 rows that are no multiple of 4 bytes.
 * A thread resolves pixels_per_thread = store_bytes / elt_bytes consecutive output pixels of one row once and writes
 * them in each of the c planes; vectors_per_row of them make a row, a workgroup of `threads` threads takes
 * `threads` consecutive ones of the h * vectors_per_row of a plane, blocks_per_image workgroups an image.  No LDS. */
typedef struct marl_warp_plan_info {
    int32_t store_bytes;
    int32_t pixels_per_thread;
    int32_t vectors_per_row;
    int32_t threads;
    int32_t blocks_per_image;
    int32_t lds_bytes;
    int32_t reserved[2];
} marl_warp_plan_info;

/* dst[b] = the transform above of src[rows[b]], b < batch; src is [n_src, c, h, w], dst [batch, c, h, w], both
 * contiguous, elt_bytes 1 (uint8) or 4 (fp32; fill_bits is the fill's bit pattern, its low byte for elt_bytes 1).
 * rows == NULL: rows[b] = b (n_src >= batch is then required).  ops == NULL: no rectangle.  rows, mats, ops, src and
 * dst are device pointers; one kernel on `stream` (a hipStream_t passed as void*), no workspace, no atomics.
 * MARL_EINVAL (marl_last_error names batch_warp) before anything is enqueued: a null src / dst / mats (a plain gather
 * is marl_batch_augment's), elt_bytes neither 1 nor 4, an unknown pad_mode, a size that is not positive, dst
 * overlapping [src, src + n_src c h w elt_bytes).  MARL_ELIMIT: an image of 2^31 bytes or more, or more workgroups
 * than a grid holds. */
int marl_batch_warp(const void* src, int64_t n_src, void* dst, const int64_t* rows, const int32_t* mats,
                    const int32_t* ops, int batch, int c, int h, int w, int elt_bytes, int pad_mode,
                    uint32_t fill_bits, void* stream);

/* The plan of that launch for (c, h, w, elt_bytes) and the alignment of src / dst (src may be NULL: reads take any
 * alignment).  MARL_EINVAL / MARL_ELIMIT as above. */
int marl_batch_warp_plan(int c, int h, int w, int elt_bytes, const void* src, const void* dst,
                         marl_warp_plan_info* out);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_WARP_H */
