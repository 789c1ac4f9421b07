/*
 * marl_hip_mix.h - CutMix and Mixup fused into the augmenting batch gather of libmarl_hip.so: every output image is a
 * view of the resident image set (include/marl_hip_augment.h: a source row under a dihedral code, a shift and an erased
 * rectangle) mixed with the view of ANOTHER image of the same batch - the batch mixed with a permutation of itself, in
 * one launch from the resident set.  The entries live beside the C ABI that include/marl_hip.h declares and versions
 * (MARL_ABI_VERSION, its list of exports) and change none of it; marl_batch_augment is unchanged.  Conventions (error
 * codes, marl_last_error) are those of marl_hip.h.
 *
 * rows[b], ops[b] mean exactly what they mean for marl_batch_augment; VIEW i is what marl_batch_augment writes for
 * (rows[i], ops[i]).  Per output image b eight int32 mix[b] = (partner, mode, by, bx, bh, bw, k, 0); with p = partner,
 * output pixel (c, y, x) of image b is
 *   mode 0           view b
 *   mode 1 (CutMix)  view p where by <= y < by + bh and bx <= x < bx + bw, else view b
 *   mode 2 (Mixup)   uint8: (k * view_b + (256 - k) * view_p + 128) >> 8 in integer arithmetic, k in [0, 256];
 *                    fp32:  fadd_rn(fmul_rn(k / 256.f, view_b), fmul_rn((256 - k) / 256.f, view_p)) - both factors are
 *                    exact in fp32 and nothing is contracted into an FMA (elt_bytes 4 means fp32 under this mode).
 * The partner's view is taken under the partner's OWN row and ops.
 * Nothing in device memory is trusted: partner is clamped to [0, batch), the mode is mode & 3 with 3 read as 0, the box
 * is intersected with the image in 64-bit arithmetic, k is clamped to [0, 256], and rows / ops are sanitised as
 * marl_hip_augment.h documents, so no value of mix / ops / rows reads or writes outside src and dst.
 * mix.reference_apply (Python) applies the same rules.
 */
#ifndef MARL_HIP_MIX_H
#define MARL_HIP_MIX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MARL_MIX_NONE 0
#define MARL_MIX_CUTMIX 1
#define MARL_MIX_MIXUP 2

/* What the launcher does for one shape and pointer pair (host arithmetic, nothing is launched).
 * store_bytes: bytes per lane of every global store, by marl_batch_augment's rule (the widest of 16 / 8 / 4 that divides
 *   w * elt_bytes and dst's address; 1 for uint8 rows that are no multiple of 4 bytes).
 * Every output image runs as bands of band_vectors consecutive stores, blocks_per_image workgroups of 256 threads.
 * A store whose pixels all come from one view without a transposing code, from consecutive source pixels, is one
 * vector load (two and a blend in registers under Mixup); every other store is resolved per pixel in the same pass -
 * views with d4 & 1 among them: there is no LDS tile here (lds_bytes 0). */
typedef struct marl_mix_plan_info {
    int32_t store_bytes;
    int32_t band_vectors;
    int32_t blocks_per_image;
    int32_t lds_bytes;
} marl_mix_plan_info;

/* dst[b] = the mix above, b < batch.  src, dst, rows, ops, elt_bytes, pad_mode, fill_bits and stream are those of
 * marl_batch_augment, and so are its guards (MARL_EINVAL / MARL_ELIMIT before anything is enqueued).  mix is a device
 * pointer to int32 [batch, 8]; NULL means all zeros, and that launch writes what marl_batch_augment writes, byte for
 * byte.  One kernel, no workspace, no atomics. */
int marl_batch_mix(const void* src, int64_t n_src, void* dst, const int64_t* rows, const int32_t* ops,
                   const int32_t* mix, int batch, int c, int h, int w, int elt_bytes, int pad_mode, uint32_t fill_bits,
                   void* stream);

/* The plan of that launch for (c, h, w, elt_bytes) and the alignment of dst (src may be NULL: reads take any
 * alignment).  MARL_EINVAL / MARL_ELIMIT as above. */
int marl_batch_mix_plan(int c, int h, int w, int elt_bytes, const void* src, const void* dst, marl_mix_plan_info* out);

#ifdef __cplusplus
}
#endif

#endif /* MARL_HIP_MIX_H */
