"""Host model (numpy) of the fp32 -> three-bf16 split and of the "k16 image" that csrc/split.h describes:

    image[row / 32][k / 16][row % 32][plane 0..2][k % 16]   bf16

fp32 -> bf16 is round-to-nearest-even by integer arithmetic on the bit pattern; the two residuals are taken in fp32,
as the device takes them.  K is zero-padded to a whole 16-deep step, rows to a whole block of 32.  Nothing here calls
the library: it is the independent yardstick of ``marl_image_build`` and of every producer compared with it.

The model (like the header's exact-split claim) covers zeros and finite values with 2^-103 <= |x| < the largest fp32
that still rounds to a finite bf16 (``BF16_FINITE_MAX_F32``): below, a residual is subnormal; above, the first term is
an infinity."""
import numpy as np

STEP = 16          # K depth of one image step
BLOCK_ROWS = 32    # rows of one block
ROW_BYTES = 96     # one row in one step: 3 planes x 16 bf16
CHUNK_BYTES = BLOCK_ROWS * ROW_BYTES

# exact ties above an even (rounds down) and above an odd (rounds up) bf16 mantissa; values whose first residual is
# zero (bf16 numbers) and whose second is (a bf16 number plus a bf16 number 2^-9 below its last place)
PLANTED_BITS = np.array([0x00000000, 0x80000000,                          # +-0
                         0x3F800000, 0xBF800000, 0x2F800000, 0x5E800000,  # +-1, 2^-32, 2^62
                         0x3F808000, 0xBF808000, 0x3F818000, 0xBF818000,  # ties: even below, odd below
                         0x40A08000, 0x40A18000,
                         0x3FC00000, 0xC1480000, 0x3F810000,              # first residual zero: 1.5, -12.5, 1 + 2^-7
                         0x3F802000, 0xC0490000 | 0x0C00, 0x3F80FF00],    # second residual zero
                        dtype=np.uint32)
BF16_FINITE_MAX_F32 = np.array([0x7F7F7FFF], dtype=np.uint32).view(np.float32)[0]
EXACT_MIN = np.float32(2.0 ** -103)


def planted():
    return PLANTED_BITS.view(np.float32).copy()


def bf16_bits(x):
    """fp32 array -> the uint16 patterns of its bf16 roundings (nearest, ties to even), by integer arithmetic"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (r & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    """uint16 bf16 patterns -> their fp32 values"""
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split3_bits(x):
    """the three planes of ``x`` (uint16 patterns each): x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1),
    the subtractions in fp32"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b0 = bf16_bits(x)
    r1 = x - bf16_value(b0)
    b1 = bf16_bits(r1)
    r2 = r1 - bf16_value(b1)
    return b0, b1, bf16_bits(r2)


def split3(x):
    return tuple(bf16_value(b) for b in split3_bits(x))


def steps_of(k):
    return (k + STEP - 1) // STEP


def image_bytes(rows, k):
    return ((rows + BLOCK_ROWS - 1) // BLOCK_ROWS) * steps_of(k) * CHUNK_BYTES


def as_rows(image_u8, steps):
    """a flat uint8 image -> a view [row blocks, steps, 32 rows, 3 planes, 16] of uint16"""
    return image_u8.view(np.uint16).reshape(-1, steps, BLOCK_ROWS, 3, STEP)


def place(image_u8, x, row0=0, steps=None):
    """writes the fp32 matrix ``x`` [rows, k] into the image at rows row0 .. row0 + rows - 1, K steps 0 ..
    ceil(k / 16) - 1 (k zero-padded to whole steps); everything else in ``image_u8`` stays"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, k = x.shape
    ks = steps_of(k)
    steps = ks if steps is None else steps
    padded = np.zeros((rows, ks * STEP), dtype=np.float32)
    padded[:, :k] = x
    planes = np.stack(split3_bits(padded), axis=1).reshape(rows, 3, ks, STEP)  # [row, plane, step, 16]
    view = as_rows(image_u8, steps)
    r = np.arange(rows) + row0
    view[r // BLOCK_ROWS, :ks, r % BLOCK_ROWS] = planes.transpose(0, 2, 1, 3)  # [row, step, plane, 16]
    return image_u8


def build(x):
    """the whole image of ``x`` [rows, k]: padding rows and padding K are zero"""
    rows, k = x.shape
    return place(np.zeros(image_bytes(rows, k), dtype=np.uint8), x)


def valid_rows(image_u8, rows, k):
    """the bytes of the valid rows only, [rows, steps, 3, 16] uint16 (padding rows of the last block left out)"""
    r = np.arange(rows)
    return as_rows(image_u8, steps_of(k))[r // BLOCK_ROWS, :, r % BLOCK_ROWS]
