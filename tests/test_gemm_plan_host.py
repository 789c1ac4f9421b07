"""marl_gemm_plan (include/marl_hip_gemmops.h) on the host: what each matrix-product launcher does with a shape, from
the planning routine the launcher itself calls, against a restatement of the rules written here from the launchers'
source and the variant tables of DESIGN 8.x.  No GPU: the library loads without one."""
import itertools

import pytest

from tests.gemm_cases import DEFAULTS, KINDS, KNOB_SETTINGS, LSTM_ROWS, NT_ROWS, TN_ROWS, _lib, hook, knobs
from tests.util import CASES, cdiv, plan_witness

# ---- the rules, restated -------------------------------------------------------------------------------------------
def blocks128(ms, ns):
    return sum(cdiv(m, 128) * cdiv(n, 128) for m, n in zip(ms, ns))


def expect_nt(ms, ns, ks, has_images, kn, lstm):
    split, b128, max_n = kn["mfma_split"] != 0, blocks128(ms, ns), max(ns)
    if lstm:
        bm = bn = 128
    elif split:
        bm, bn = 128, (128 if b128 >= 384 and max_n >= 96 else 64)
    else:
        bm = bn = 128 if b128 >= 256 and max_n >= 96 else 64
    single = int(not split and not lstm and bm == 128)
    pre = int(split and bool(has_images) and
              all((4 if lstm else 1) * n * cdiv(k, 32) * 192 < 2 ** 32 for n, k in zip(ns, ks)))
    gx, gy, gz = cdiv(max(ms), bm), cdiv(max_n, 32 if lstm else bn), len(ms)
    lds = 3 * (128 + bn) * 80 if split else (1 if single else 2) * (bm + bn) * 36 * 4
    return dict(family=int(split), bm=bm, bn=bn, threads=256, gx=gx, gy=gy, gz=gz, blocks=gx * gy * gz,
                xcd_map=int(len(ms) == 1 and not lstm and kn["nt_xcd"] != 0), single_buf=single, pre=pre, lds_bytes=lds)


def expect_g3(ms, ns, variant, kn, lstm):
    v = variant or kn["g3_lstm_variant" if lstm else "g3_nt_variant"]
    if not v and lstm:
        t128 = sum(cdiv(m, 128) * cdiv(n, 32) for m, n in zip(ms, ns))
        t64 = sum(cdiv(m, 64) * cdiv(n, 32) for m, n in zip(ms, ns))
        v = 2 if t128 >= 192 else 4 if t64 >= 384 else 3
    elif not v:
        b128 = blocks128(ms, ns)
        v = 2 if max(ns) >= 96 and b128 >= 256 else 7
        if v == 2 and b128 >= 1024 and len(ms) == 1 and max(ns) % 256 == 0:
            v = 21
    rows = LSTM_ROWS if lstm else NT_ROWS
    bm, bn, wm, wn, nst, pipe = rows.get(v, rows[None])
    gx, gy, gz = cdiv(max(ms), bm), cdiv(max(ns), 32 if lstm else bn), len(ms)
    same = all(m == ms[0] and n == ns[0] for m, n in zip(ms, ns))
    return dict(variant=v, row_id=v if v in rows else 0, bm=bm, bn=bn, wm=wm, wn=wn, nst=nst, pipelined=pipe,
                threads=wm * wn * 64, gx=gx, gy=gy, gz=gz, blocks=gx * gy * gz, safe=0,
                xcd_map=int(kn["nt_xcd"] != 0 and not lstm and (len(ms) == 1 or same)),
                lds_bytes=nst * (bm + bn) * 96)  # the ring: NST stages of BM + BN image rows of 96 bytes


def expect_tn(ni, nj, rows, kn):
    bm = 128 if ni >= 96 and nj >= 96 and cdiv(ni, 128) * cdiv(nj, 128) >= 4 else 64
    family = int(bm == 128 and kn["mfma_split"] != 0)
    waves = (8 if kn["tn_split_waves"] == 8 else 4) if family else 4
    gx, gy = cdiv(ni, bm), cdiv(nj, bm)
    s = max(1, min(cdiv(512 if family else 768, gx * gy), cdiv(rows, 128), 512))
    rps = cdiv(cdiv(rows, s), 32) * 32
    splits = cdiv(rows, rps)
    lds = 3 * 256 * 80 if family else (1 if bm == 128 else 2) * 32 * 2 * bm * 4
    return dict(family=family, bm=bm, bn=bm, threads=waves * 64, gx=gx, gy=gy, gz=splits, blocks=gx * gy * splits,
                xcd_map=int(kn["tn_xcd"] != 0), splits=splits, rows_per_split=rps, lds_bytes=lds,
                scratch_bytes=(splits * ni * nj + splits * ni) * 4 if splits > 1 else 0)


def expect_tn_images(ni, nj, rows, kn):
    v = kn["g3_tn_variant"]
    if not v:
        rem = nj % 256
        v = 2 if not (ni >= 256 and nj >= 192 and rows >= 32768) else 4 if 0 < rem <= 128 and nj > 256 else 3
    if v not in TN_ROWS:
        v = 2
    bi, bj, threads, (ring_rows, nst) = TN_ROWS[v]
    gx, gy = cdiv(ni, bi), (1 if v == 4 else cdiv(nj, bj))
    s = max(1, min(cdiv(512 if v == 2 else 256, gx * gy), cdiv(rows, 256), 512))
    rps = cdiv(cdiv(rows, s), 32) * 32
    splits = cdiv(rows, rps)
    return dict(variant=v, bm=bi, bn=bj, threads=threads, gx=gx, gy=gy, gz=splits, blocks=gx * gy * splits,
                xcd_map=int(kn["tn_xcd"] != 0), pipelined=int(v in (3, 4) and kn["g3_tn_pipe"] != 0), splits=splits,
                rows_per_split=rps, lds_bytes=nst * ring_rows * 96, scratch_bytes=(splits * ni * nj + splits * ni) * 4)


def cell_tiles(nj):
    n256, rem = divmod(nj, 256)
    return (n256 + 1, 0) if rem > 128 else (n256, int(rem > 0))


def expect_cell(ni, nih, nhh, rows, kn):
    (a256, a128), (b256, b128) = cell_tiles(nih), cell_tiles(nhh)
    n256, n128 = a256 + b256, a128 + b128
    out = dict(variant=5, pipelined=int(kn["g3_tn_pipe"] != 0), ok=0, blocks=0, splits=0, scratch_bytes=0, lds_bytes=0)
    if ni < 256 or rows < 8192 or rows % 32 or n128 > 1 or n256 + n128 > 4 or n256 < 1:
        return out
    teams = int(n128 == 1 and ni % 512 == 0)
    per_slab = (ni // 512) * (2 * n256 + 1) if teams else cdiv(ni, 256) * (n256 + n128)
    s = max(1, min(256 // per_slab, cdiv(rows, 256)))
    rps = cdiv(cdiv(rows, s), 32) * 32
    splits = cdiv(rows, rps)
    out.update(ok=1, bm=256, bn=256, threads=512, teams=teams, ih256=a256, ih128=a128, hh256=b256, hh128=b128,
               splits=splits, rows_per_split=rps, blocks=per_slab * splits, lds_bytes=3 * 512 * 96,
               scratch_bytes=splits * (ni * nih + ni * nhh + 2 * ni) * 4)
    return out


def agrees(got, want, what):
    bad = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not bad, (what, bad)
    zero = [k for k in got if k not in want and k != "kind" and got[k] != 0]
    assert not zero, (what, "fields this kind does not have must be 0", zero)


# ---- the grid ------------------------------------------------------------------------------------------------------
R_ROWS = [512, 1024, 2048, 4096]  # BASELINE C4, (C3 at 64 images), C5, C3
NR_ROWS = [8192, 32768, 65536]
# NT-shaped launches (m[], n[], k[]): the heads, dU and in-loop batches at the BASELINE row counts, then the boundary
# pairs: blocks128 255 / 256, 383 / 384, 1023 / 1024 (n = 128 and 256), max_n 95 / 96, t128 191 / 192, t64 383 / 384
NT_SHAPES = ([([r], [n], [k]) for r in R_ROWS + NR_ROWS for n, k in ((384, 256), (256, 1024), (45, 384), (64, 96))] +
             [([r, r], [384, 384], [256, 256]) for r in R_ROWS] + [([r, r], [256, 64], [256, 256]) for r in R_ROWS] +
             [([r] * 4, [256, 256, 64, 96], [1024] * 4) for r in (512, 4096)] +
             [([128 * b], [n], [256]) for b in (255, 256, 383, 384, 1023, 1024) for n in (128, 256)] +
             [([128 * 512], [n], [64]) for n in (95, 96)] +
             [([128 * t], [32], [880]) for t in (191, 192)] + [([64 * t], [32], [880]) for t in (383, 384)] +
             [([33], [257], [7]), ([100000], [1000], [2 ** 21])])
LSTM_SHAPES = ([([r, r], [n, n], [880, 880]) for r in R_ROWS for n in (256, 64)] +
               [([128 * t], [32], [880]) for t in (191, 192)] + [([64 * t], [32], [880]) for t in (383, 384)] +
               [([64 * 191, 64 * 192], [32, 32], [880, 880]), ([100], [2 ** 20], [2 ** 12])])
# row contractions (ni, nj): the four large weight gradients at C3's widths, nj % 256 of 0, 1, 128, 129, small ones
TN_SHAPES = ([(1024, 624), (1024, 256), (256, 64), (384, 256), (45, 384), (96, 96), (95, 512), (512, 512)] +
             [(1024, nj) for nj in (512, 513, 640, 641, 191, 192)] + [(255, 512), (256, 512), (130, 130), (1, 384)])
TN_ROW_COUNTS = NR_ROWS + [8191, 32767, 32736, 8160, 96, 15360]
CELL_SHAPES = [(1024, 624, 256), (256, 384, 64), (256, 256, 128), (512, 880, 256), (1024, 512, 512), (1024, 640, 384),
               (768, 624, 256), (255, 624, 256), (256, 100, 100)]


@pytest.mark.parametrize("setting", KNOB_SETTINGS, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()) or "default")
def test_the_hook_equals_the_restated_rules(setting):
    L = _lib()
    lib = L.load()
    with knobs(setting) as kn:
        for ms, ns, ks in NT_SHAPES:
            for has in (0, 1):
                agrees(hook("nt", ms, ns, ks, has_images=has), expect_nt(ms, ns, ks, has, kn, False), ("nt", ms, ns, ks, has))
            for variant in (0, 2, 22, 99):
                agrees(hook("nt_images", ms, ns, variant=variant), expect_g3(ms, ns, variant, kn, False),
                       ("nt_images", ms, ns, variant))
        for ms, ns, ks in LSTM_SHAPES:
            for has in (0, 1):
                agrees(hook("lstm", ms, ns, ks, has_images=has), expect_nt(ms, ns, ks, has, kn, True), ("lstm", ms, ns, has))
            for variant in (0, 1, 6, 99):
                agrees(hook("lstm_images", ms, ns, variant=variant), expect_g3(ms, ns, variant, kn, True),
                       ("lstm_images", ms, ns, variant))
        for (ni, nj), rows in itertools.product(TN_SHAPES, TN_ROW_COUNTS):
            p = hook("tn", [ni], [nj], rows=rows)
            agrees(p, expect_tn(ni, nj, rows, kn), ("tn", ni, nj, rows))
            assert p["splits"] * p["rows_per_split"] >= rows and p["rows_per_split"] % 32 == 0
            assert lib.marl_gemm_tn_scratch(ni, nj, rows) == p["scratch_bytes"]
            if rows % 32:
                assert hook("tn_images", [ni], [nj], rows=rows, rc_only=True) != 0  # (images hold whole row blocks)
                continue
            p = hook("tn_images", [ni], [nj], rows=rows)
            agrees(p, expect_tn_images(ni, nj, rows, kn), ("tn_images", ni, nj, rows))
            assert p["splits"] * p["rows_per_split"] >= rows and p["rows_per_split"] % 32 == 0
            assert lib.marl_gemm_tn_images_scratch(ni, nj, rows) == p["scratch_bytes"]
        for (ni, nih, nhh), rows in itertools.product(CELL_SHAPES, TN_ROW_COUNTS):
            p = hook("tn_images_cell", [ni, ni], [nih, nhh], rows=rows)
            agrees(p, expect_cell(ni, nih, nhh, rows, kn), ("cell", ni, nih, nhh, rows))
            assert p["splits"] * p["rows_per_split"] >= rows * p["ok"]
            assert lib.marl_gemm_tn_images_cell_scratch(ni, nih, nhh, rows) == p["scratch_bytes"]


def test_the_grid_reaches_both_sides_of_every_threshold():
    """the shapes above select every row a default can select, and both plans around each boundary"""
    kn = dict(DEFAULTS)
    nt = {expect_g3(ms, ns, 0, kn, False)["variant"] for ms, ns, _ in NT_SHAPES}
    assert nt == {2, 7, 21}
    assert {expect_g3(ms, ns, 0, kn, True)["variant"] for ms, ns, _ in LSTM_SHAPES} >= {2, 3}
    assert {expect_nt(ms, ns, ks, 1, kn, False)["bn"] for ms, ns, ks in NT_SHAPES} == {64, 128}
    assert {expect_nt(ms, ns, ks, 1, kn, False)["pre"] for ms, ns, ks in NT_SHAPES} == {0, 1}
    assert {expect_nt(ms, ns, ks, 0, {**kn, "mfma_split": 0}, False)["bm"] for ms, ns, ks in NT_SHAPES} == {64, 128}
    tn3 = {expect_tn_images(ni, nj, r, kn)["variant"] for ni, nj in TN_SHAPES for r in NR_ROWS}
    assert tn3 == {2, 3, 4}
    assert {expect_tn(ni, nj, r, kn)["bm"] for ni, nj in TN_SHAPES for r in NR_ROWS} == {64, 128}
    cells = [expect_cell(*s, r, kn) for s in CELL_SHAPES for r in TN_ROW_COUNTS]
    assert {c["ok"] for c in cells} == {0, 1} and {c.get("teams") for c in cells if c["ok"]} == {0, 1}


@pytest.mark.parametrize("setting", [{}, {"g3_tn": 2}, {"g3_tn_pipe": 0}, {"g3_lstm_variant": 5}, {"g3_lstm_variant": 99}],
                         ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()) or "default")
@pytest.mark.parametrize("nb", [2, 4, 8, 16, 128, 256])  # 16 agents: R = 32 ... 4096 (C4's and C3's among them)
def test_plan_query_agrees_with_the_hook(setting, nb):
    """the episode's plan (marl_plan_query) names what the launchers' routines name for the C3 model's shapes:
    256 units in both cells, inputs of nin = 624 columns, 16 steps"""
    cfg, na, ns, n, nin = CASES["g4_resisc_b2"], 16, 16, 256, 624
    with knobs(setting):
        w = plan_witness(cfg, na, nb, ns, (3, 256, 256))
        R, NR = w["R"], w["NR"]
        if not w["g3_lstm"]:
            assert w["lstm_plan"] == 0 and not w["g3_tn_cell"] and not w["g3_tn_pipe"]
            return
        assert w["lstm_plan"] == hook("lstm_images", [R, R], [n, n])["variant"]
        assert w["small_r"] == int(w["lstm_plan"] in (3, 4))
        cell = hook("tn_images_cell", [4 * n, 4 * n], [nin, n], rows=NR)
        assert w["g3_tn_cell"] == int(w["g3_tn"] and cell["ok"])
        assert w["g3_tn_pipe"] == int(w["g3_tn"] and cell["pipelined"])
        assert w["g3_tn"] == int(setting.get("g3_tn") == 2 or NR >= 32768 or cell["ok"])


def test_the_header_and_the_binding_name_the_same_hook():
    import os
    import re

    L = _lib()
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "marl_hip_gemmops.h"), encoding="utf-8").read()
    assert set(re.findall(r"\b(marl_gemm_plan)\(", hdr)) == set(L.GEMMOP_HOOKS)
    assert set(L.GEMMOP_HOOKS) <= set(L._HOOKS) and not set(L.GEMMOP_HOOKS) & set(L.EXPORTS)
    enum = re.findall(r"MARL_GEMM_([A-Z_]+) = (\d)", hdr)
    assert [name.lower() for name, _ in sorted(enum, key=lambda e: int(e[1]))] == list(L.GEMM_KINDS) == list(KINDS)
    fields = re.search(r"typedef struct marl_gemm_plan_info \{(.*?)\} marl_gemm_plan_info;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [name for name, _ in L.GemmPlan._fields_]
