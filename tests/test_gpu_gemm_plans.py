"""GPU: the rows of the matrix-product launchers' variant tables, each launched through the table and witnessed first:
marl_gemm_plan (include/marl_hip_gemmops.h) must name the row before the result is trusted.  tests/test_gpu_kernels.py
already launches most rows by their ids - for those only the witness is added here, on the shapes of its cases; the rows
and automatic choices it does not reach are launched here through the same bodies (tests/gemm_cases.py), so the float64
references and the bounds (NT_BOUND, TN_BOUND, the cell's 1e-5) are stated once."""
import pytest

from tests import gemm_cases as G
from tests.gemm_cases import LSTM_ROWS, NT_ROWS, TN_ROWS, hook, knobs

pytestmark = pytest.mark.gpu


def _tile(p):
    return (p["bm"], p["bn"], p["wm"], p["wn"], p["nst"], p["pipelined"])


def test_witness_of_the_image_rows_launched_by_id():
    """every (shape, variant id) of test_gemm_nt_images / test_lstm_images / test_gemm_tn_images takes the table row of
    that id - so those tests do launch rows 1, 2, 7, 11, 12, 21, 22 and the NT fallback (their id 3), LSTM 1, 3, 4, 5, 6
    and the LSTM fallback (their id 2), TN 1 to 4"""
    shapes, variants = G.NT_IMAGES_SHAPES, list(G.NT_IMAGES_VARIANTS)
    assert sorted(variants) == [1, 2, 3, 7, 11, 12, 21, 22]
    for (m, n, _k), v in ((s, v) for s in shapes for v in variants):
        p = hook("nt_images", [m], [n], variant=v)
        assert p["variant"] == v and p["row_id"] == (v if v in NT_ROWS else 0) and _tile(p) == NT_ROWS.get(v, NT_ROWS[None])
    shapes, variants = G.LSTM_IMAGES_SHAPES, list(G.LSTM_IMAGES_VARIANTS)
    assert sorted(variants) == [1, 2, 3, 4, 5, 6]
    for (m, n, _nin), v in ((s, v) for s in shapes for v in variants):
        p = hook("lstm_images", [m], [n], variant=v)
        assert p["row_id"] == (v if v in LSTM_ROWS else 0) and _tile(p) == LSTM_ROWS.get(v, LSTM_ROWS[None])
    shapes, variants = G.TN_IMAGES_SHAPES, list(G.TN_IMAGES_VARIANTS)
    assert sorted(variants) == [1, 2, 3, 4]
    for (rows, ni, nj), v in ((s, v) for s in shapes for v in variants):
        with knobs({"g3_tn_variant": v}):
            p = hook("tn_images", [ni], [nj], rows=rows)
        assert p["variant"] == v and (p["bm"], p["bn"], p["threads"]) == TN_ROWS[v][:3]
        assert p["pipelined"] == int(v in (3, 4))
    for rows, ni, nih, nhh in G.CELL_IMAGES_SHAPES:
        p = hook("tn_images_cell", [ni, ni], [nih, nhh], rows=rows)
        assert p["ok"] and p["pipelined"] and p["blocks"] <= 256 and p["splits"] * p["rows_per_split"] >= rows
    # the least shape the cell plan admits: one 256-column tile of G, one whole tile and one narrow tile of columns
    p = hook("tn_images_cell", [256, 256], [256, 128], rows=8192)
    assert p["ok"] and (p["ih256"], p["ih128"], p["hh256"], p["hh128"], p["teams"]) == (1, 0, 0, 1, 0)


def test_witness_of_the_fp32_operand_rows():
    """test_gemm_nt / test_gemm_tn run both kernel families on shapes that take every row of each: the narrow tiles and
    (their shapes of 771 and 24 tiles of 128 x 128) the 128-wide ones, with and without weight images, 8 and 4 waves"""
    nt = {}
    for m, n, k in G.NT_SHAPES:
        for split in (1, 0):
            with knobs({"mfma_split": split}):
                for w in (0, 1):
                    p = hook("nt", [m], [n], [k], has_images=w)
                    assert p["family"] == split and p["pre"] == int(split and w) and p["xcd_map"] == 1
                    nt.setdefault(split, set()).add((p["bm"], p["bn"]))
    assert nt == {1: {(128, 64), (128, 128)}, 0: {(64, 64), (128, 128)}}
    tn = set()
    for rows, ni, nj in G.TN_SHAPES:
        for split, waves in ((0, 8), (1, 8), (1, 4)):
            with knobs({"mfma_split": split, "tn_split_waves": waves}):
                p = hook("tn", [ni], [nj], rows=rows)
            assert p["family"] == int(split and p["bm"] == 128) and p["threads"] == (waves * 64 if p["family"] else 256)
            tn.add((p["family"], p["bm"], p["threads"]))
    assert tn == {(0, 64, 256), (0, 128, 256), (1, 128, 512), (1, 128, 256)}


# one whole tile plus a ragged one in each output dimension, two K steps
@pytest.mark.parametrize("variant,row", [(0, 7), (99, 0)], ids=["automatic", "fallback_row"])
def test_nt_images_rows_no_id_reaches(device, variant, row):
    m, n, k = 64 + 37, 64 + 5, 32
    p = hook("nt_images", [m], [n], variant=variant)
    assert p["row_id"] == row and _tile(p) == NT_ROWS[row or None] and p["gy"] == 2 and p["blocks"] == p["gx"] * 2
    G.check_gemm_nt_images(device, m, n, k, variant, 1)


@pytest.mark.parametrize("variant,row", [(0, 3), (99, 0)], ids=["automatic", "fallback_row"])
def test_lstm_images_rows_no_id_reaches(device, variant, row):
    m, n, nin = 128 + 13, 32 + 8, 24
    p = hook("lstm_images", [m], [n], variant=variant)
    assert p["row_id"] == row and _tile(p) == LSTM_ROWS[row or None] and p["gy"] == 2 and p["gx"] >= 2
    G.check_lstm_images(device, m, n, nin, variant)


def test_tn_images_id_outside_the_table_takes_row_2(device):
    """(before the tables such an id sized the grid for 256 x 128 tiles and launched the 128 x 128 kernel)"""
    rows, ni, nj = 512, 128 + 37, 128 + 5
    with knobs({"g3_tn_variant": 7}):
        p = hook("tn_images", [ni], [nj], rows=rows)
    assert (p["variant"], p["bm"], p["bn"], p["gx"], p["gy"], p["splits"]) == (2, 128, 128, 2, 2, 2)
    G.check_gemm_tn_images(device, rows, ni, nj, 7)


def test_the_least_shape_the_cell_plan_admits(device):
    rows, ni, nih, nhh = 8192, 256, 256, 128
    p = hook("tn_images_cell", [ni, ni], [nih, nhh], rows=rows)
    assert p["ok"] and p["blocks"] == 2 * p["splits"] and p["splits"] * p["rows_per_split"] >= rows and p["splits"] >= 2
    G.check_gemm_tn_images_cell(device, rows, ni, nih, nhh)
