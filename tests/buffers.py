"""Source rows and guarded destination buffers of the batch-gather tests (augment, mix, warp, normalize) and the
bit-level comparisons they share."""
import torch as th

GUARD = 256  # bytes before and after every destination
SENTINEL = 0xA5
N_SRC = 11   # rows of the resident set the GPU cases gather from


def source(shape, dtype, n=N_SRC, seed=0, affine=None):
    """``n`` seeded rows of ``shape``: uint8 over the whole range, or fp32 normal draws (``affine``: times a, plus b)"""
    g = th.Generator().manual_seed(seed + shape[1] * 7 + shape[2])
    if dtype == th.uint8:
        return th.randint(0, 256, (n,) + tuple(shape), dtype=th.uint8, generator=g)
    x = th.randn((n,) + tuple(shape), generator=g)
    return x if affine is None else x * affine[0] + affine[1]


def guarded(shape, dtype, device, offset=0):
    """(whole buffer, destination view): ``offset`` extra bytes in front of the view"""
    nbytes = th.Size(shape).numel() * th.empty((), dtype=dtype).element_size()
    buf = th.full((GUARD + offset + nbytes + GUARD,), SENTINEL, dtype=th.uint8, device=device)
    return buf, buf[GUARD + offset: GUARD + offset + nbytes].view(dtype).view(shape)


def guards_intact(buf, offset, nbytes):
    head, tail = buf[: GUARD + offset], buf[GUARD + offset + nbytes:]
    return bool((head == SENTINEL).all()) and bool((tail == SENTINEL).all()) and tail.numel() == GUARD


def same_bits(got, want):
    if got.dtype == th.float32:
        return th.equal(got.view(th.int32), want.view(th.int32))
    return th.equal(got, want)


def bits(t):
    return t.contiguous().view(th.int32)


def ulps(a, b):
    """distance in fp32 steps (the int32 patterns of same-signed floats are ordered like the floats)"""
    return (bits(a).to(th.int64) - bits(b).to(th.int64)).abs()
