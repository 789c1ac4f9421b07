"""CPU: the host model of the k16 image (tests/image_model.py) - the yardstick marl_image_build is compared with,
checked here against the claims of csrc/split.h alone: every term of the split is a bf16, the three terms add up to
the fp32 value exactly (float64 arithmetic), and the layout is image[row / 32][k / 16][row % 32][plane][k % 16]."""
import numpy as np

from tests import image_model as im


def _values():
    rng = np.random.default_rng(5)
    n = 1 << 16
    sign = rng.integers(0, 2, n, dtype=np.uint32) << 31
    expo = rng.integers(127 - 60, 127 + 61, n, dtype=np.uint32) << 23   # exponents in 2^-60 .. 2^60
    mant = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    return np.concatenate([im.planted(), (sign | expo | mant).view(np.float32)])


def test_rounding_is_nearest_even():
    x = _values()
    b = im.bf16_value(im.bf16_bits(x)).astype(np.float64)
    lo = ((x.view(np.uint32) & 0xFFFF0000).view(np.float32)).astype(np.float64)       # truncation
    ulp = np.abs((((x.view(np.uint32) & 0x7F800000) | 0x00010000).view(np.float32)
                  - (x.view(np.uint32) & 0x7F800000).view(np.float32)).astype(np.float64))  # bf16 spacing at x
    x64 = x.astype(np.float64)
    nz = x != 0
    assert np.all(np.abs(b - x64)[nz] <= ulp[nz] / 2), "not the nearest bf16"
    tie = nz & (np.abs(b - x64) == ulp / 2)
    assert tie.sum() >= 6 and np.all((im.bf16_bits(x)[tie] & 1) == 0), "a tie did not go to the even mantissa"
    assert np.all(np.abs(b) >= np.abs(lo))  # (never below the truncation in magnitude)
    # the planted ties: above an even mantissa down, above an odd one up
    t = np.array([0x3F808000, 0x3F818000, 0x40A08000, 0x40A18000], dtype=np.uint32).view(np.float32)
    assert list(im.bf16_bits(t)) == [0x3F80, 0x3F82, 0x40A0, 0x40A2]
    z = np.array([0x00000000, 0x80000000], dtype=np.uint32).view(np.float32)
    assert list(im.bf16_bits(z)) == [0x0000, 0x8000]


def test_every_term_is_a_bf16_and_the_split_is_exact():
    x = _values()
    terms = im.split3(x)
    for t in terms:
        assert np.all((t.view(np.uint32) & 0xFFFF) == 0), "a term is not a bf16"
        assert np.all(np.isfinite(t))
    total = terms[0].astype(np.float64) + terms[1].astype(np.float64) + terms[2].astype(np.float64)
    assert np.array_equal(total, x.astype(np.float64)), "x0 + x1 + x2 != x"
    # the planted values whose first / second residual vanishes
    p = im.planted()
    t0, t1, t2 = im.split3(p)
    first_zero = np.isin(im.PLANTED_BITS, [0x3FC00000, 0xC1480000, 0x3F810000, 0x3F800000, 0xBF800000])
    assert np.all(t1[first_zero] == 0) and np.all(t2[first_zero] == 0)
    second_zero = np.isin(im.PLANTED_BITS, [0x3F802000, 0xC0490C00, 0x3F80FF00])
    assert second_zero.sum() == 3 and np.all(t1[second_zero] != 0) and np.all(t2[second_zero] == 0)
    # both ends of the stated range
    edge = np.array([im.EXACT_MIN, -im.EXACT_MIN, im.BF16_FINITE_MAX_F32, -im.BF16_FINITE_MAX_F32], dtype=np.float32)
    e = im.split3(edge)
    assert np.array_equal(sum(t.astype(np.float64) for t in e), edge.astype(np.float64))
    assert np.all(np.isfinite(e[0]))
    with np.errstate(invalid="ignore"):  # (inf - inf in the residuals)
        assert np.isinf(im.split3(np.array([0x7F7F8000], dtype=np.uint32).view(np.float32))[0][0])  # just above


def test_layout_and_padding():
    rows, k = 37, 21
    x = np.arange(rows * k, dtype=np.float32).reshape(rows, k) / 7 + 1
    img = im.build(x)
    steps = im.steps_of(k)
    assert steps == 2 and img.size == im.image_bytes(rows, k) == 2 * 2 * 3072
    planes = im.split3_bits(x)
    u16 = img.view(np.uint16)
    for r, c in [(0, 0), (5, 15), (31, 16), (32, 3), (36, 20)]:
        for pl in range(3):
            byte = ((r // 32) * steps + c // 16) * 3072 + (r % 32) * 96 + pl * 32 + (c % 16) * 2
            assert u16[byte // 2] == planes[pl][r, c], (r, c, pl)
    v = im.valid_rows(img, rows, k)
    assert v.shape == (rows, steps, 3, 16) and np.all(v[:, 1, :, k - 16:] == 0), "K padding is not zero"
    assert np.all(im.as_rows(img, steps)[1, :, rows - 32:] == 0), "padding rows are not zero"
    # place: only the addressed rows and steps change
    base = np.full(im.image_bytes(70, 48), 0x5A, dtype=np.uint8)
    out = im.place(base.copy(), x[:, :16], row0=30, steps=3)
    changed = im.as_rows(out, 3) != im.as_rows(base, 3)
    r = np.arange(rows) + 30
    mask = np.zeros_like(changed)
    mask[r // 32, 0, r % 32] = True
    assert not np.any(changed & ~mask)
    assert np.array_equal(im.as_rows(out, 3)[r // 32, 0, r % 32], im.valid_rows(im.build(x[:, :16]), rows, 16)[:, 0])
