#!/usr/bin/env python3
"""Identity of the batch-gather refactor (csrc/gather.h) and of the one that gave the normalise and
colour families the same rules (csrc/normrules.h): the tree's libmarl_hip.so against the parent's.
No GPU: device code is read from the fat binary, plans are host arithmetic, and of the launchers only calls that a guard
refuses are made (made-up pointers, nothing is dereferenced, nothing is launched).

    python tools/gather_identity.py PARENT.so TREE.so [--record profiles/pixel_identity.json]

Both libraries are built with the default flags (make -C marlclassification_amd/csrc).
  (a) device code: every kernel of the library equals the parent's of the same name in machine code, instruction lines
      and metadata (tools/conv_plan_identity.py's walk); no kernel is missing, none is new;
  (b) plans: marl_batch_augment_plan, marl_batch_mix_plan and marl_batch_warp_plan, return code and every field, over
      c 1..4 x h, w in SIZES x both element sizes x destination offsets OFFSETS, and the invalid shapes; the same
      sweep of marl_batch_normalize_plan, marl_batch_color_plan (c 1..4: 2 and 4 are refusals; both out_form) and
      marl_batch_stats_scratch_bytes (the returned size; 0 is its refusal);
  (c) guards: for each launcher the return code and the marl_last_error text under each single bad argument of
      tests/test_gpu_warp.py::test_every_guard_of_the_c_entry and under every pair of them at once (the pairs pin the
      order of the guards); the same for marl_batch_stats, marl_batch_normalize (test_gpu_normalize.py::
      test_every_guard_of_the_c_entries) and marl_batch_color (test_gpu_color.py::test_every_guard_of_the_c_entry).
Exit status 0: all three equal.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys
import tempfile

os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = "-1"  # no device: nothing here can launch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conv_plan_identity import _device_code  # noqa: E402
from gemm_plan_identity import _same  # noqa: E402

SIZES = (1, 2, 3, 4, 7, 8, 16, 63, 64, 65, 128, 129, 256, 600)
OFFSETS = (0, 1, 2, 4, 8, 16)
INVALID = ((0, 8, 8, 1), (3, 0, 8, 1), (3, 8, -1, 4), (3, 8, 8, 0), (3, 8, 8, 2), (3, 8, 8, 8), (2, 32768, 32768, 1),
           (1, 32768, 16384, 4), (-1, -1, -1, 3))
SRC, DST, TABLE = 0x10000000, 0x20000000, 0x30000000  # (never dereferenced)

# marl_batch_*(src, n_src, dst, rows, [tables...], batch, c, h, w, elt_bytes, pad_mode, fill_bits, stream)
LAUNCHERS = {"marl_batch_augment": ("ops",), "marl_batch_mix": ("ops", "mix"), "marl_batch_warp": ("mats", "ops")}
GOOD = dict(src=SRC, n_src=4, dst=DST, rows=None, ops=None, mix=None, mats=TABLE, batch=4, c=3, h=8, w=8, elt=1, pad=1)
# test_every_guard_of_the_c_entry's list (the last two are its ELIMIT cases; `mats` only means something to warp; the
# grid case is 128 rows high, not 32: two workgroups an image for the 1024-store bands of augment and mix as well)
BAD = (dict(src=None), dict(dst=None), dict(mats=None), dict(elt=2), dict(pad=2), dict(batch=0), dict(n_src=0),
       dict(c=0), dict(h=-1), dict(w=0), dict(n_src=3), dict(dst=SRC), dict(src=SRC + 1, dst=DST + 2, elt=4, w=2),
       dict(c=2, h=32768, w=32768),
       dict(src=SRC, n_src=1, dst=DST, rows=TABLE, batch=2**31 - 1, c=1, h=128, w=256))

# The two pixel families (normalize.hip, color.hip): the tests' lists with made-up pointers in place of the real ones,
# and two cases more an entry, for the guards no test list reaches: the extent limit and the grid.
REC, SCRATCH, COEF, PAR, DSTF = 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000
USER = (0.5, 0.25, 0.5, 0.25, 0.5, 0.25)
ZERO_S = (0.5, 0.25, 0.5, 0.0, 0.5, 0.25)
NO_WIDTH = (0.5, 0.9, 0.3, 0.3, 0.5, 0.9)
NAN = (float("nan"), 0.9, 0.3, 0.4, 0.5, 0.9)
D_END = DST + 4 * 3 * 64  # (the first byte behind a uint8 destination; an fp32 one is four times as long)
PIXEL = {
    "marl_batch_stats": dict(
        args="src n_src rows batch c h w elt scratch rec".split(),
        types=[C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3,
        good=dict(src=SRC, n_src=4, rows=None, batch=4, c=3, h=8, w=8, elt=1, scratch=SCRATCH, rec=REC),
        bad=(dict(src=None), dict(scratch=None), dict(rec=None), dict(elt=3), dict(batch=0), dict(h=0), dict(n_src=2),
             dict(scratch=SCRATCH + 4), dict(rec=REC + 4), dict(c=2, h=32768, w=32768), dict(c=3, h=2048, w=2048),
             dict(n_src=2**62, rows=REC),  # (the extent; then the grid: two chunks a plane)
             dict(n_src=1, rows=REC, batch=2**31 - 1, c=1, h=128, w=256))),
    "marl_batch_normalize": dict(
        args="src n_src rows rec mode usr batch c h w elt dst coef".split(),
        types=[C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3,
        good=dict(src=SRC, n_src=4, rows=None, rec=REC, mode=1, usr=None, batch=4, c=3, h=8, w=8, elt=1, dst=DST,
                  coef=COEF),
        bad=(dict(src=None), dict(dst=None), dict(rec=None), dict(mode=5, usr=None), dict(mode=6), dict(elt=2),
             dict(batch=0), dict(n_src=0), dict(c=0), dict(h=-1), dict(w=0), dict(n_src=3), dict(mode=4, usr=USER, c=17),
             dict(mode=4, usr=ZERO_S), dict(mode=5, usr=NO_WIDTH), dict(mode=4, usr=NAN), dict(dst=SRC),
             dict(src=DST + 4 * (4 * 3 * 64) - 1, dst=DST), dict(src=SRC + 2, elt=4, w=2), dict(dst=DST + 2),
             dict(rec=REC + 4), dict(coef=COEF + 2), dict(c=2, h=32768, w=32768), dict(c=3, h=2048, w=2048),
             dict(n_src=2**62, rows=REC),  # (the extent; then the grid: two workgroups a plane)
             dict(n_src=1, rows=REC, batch=2**31 - 1, c=1, h=64, w=128))),
    "marl_batch_color": dict(
        args="src n_src rows rec par form mode usr batch c h w elt dst coef".split(),
        types=([C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 +
               [C.c_void_p] * 3),
        good=dict(src=SRC, n_src=4, rows=None, rec=REC, par=PAR, form=0, mode=0, usr=None, batch=4, c=3, h=8, w=8,
                  elt=1, dst=DST, coef=COEF),
        bad=(dict(src=None), dict(dst=None), dict(par=None), dict(c=2), dict(elt=2), dict(form=3),
             dict(form=1, mode=4, usr=USER, elt=4, dst=DSTF), dict(form=1, mode=1, usr=USER, dst=DSTF),
             dict(form=1, mode=4, usr=None, dst=DSTF), dict(form=1, mode=4, usr=ZERO_S, dst=DSTF), dict(batch=0),
             dict(n_src=0), dict(h=-1), dict(w=0), dict(n_src=3), dict(src=SRC + 2, elt=4, w=2),
             dict(form=1, mode=4, usr=USER, dst=DSTF + 2), dict(rec=REC + 4), dict(coef=COEF + 2), dict(par=PAR + 2),
             dict(dst=SRC), dict(src=D_END - 1, dst=DST), dict(c=3, h=32768, w=32768),
             dict(form=1, mode=4, usr=USER, dst=DSTF, c=3, h=16384, w=16384),
             dict(n_src=2**62, rows=REC),  # (the extent; then the grid: two workgroups an image)
             dict(n_src=1, rows=REC, batch=2**31 - 1, c=1, h=128, w=256))),
}


def _plans(lib):
    from marlclassification_amd import augment, mix, warp

    shapes = [(c, h, w, e) for c in range(1, 5) for h in SIZES for w in SIZES for e in (1, 4)] + list(INVALID)
    out = {}
    for entry, info in (("marl_batch_augment_plan", augment.AugmentPlan()), ("marl_batch_mix_plan", mix.MixPlan()),
                        ("marl_batch_warp_plan", warp.WarpPlan())):
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        fn.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3
        for (c, h, w, e), off in itertools.product(shapes, OFFSETS):
            C.memset(C.byref(info), 0xff, C.sizeof(info))
            rc = fn(c, h, w, e, SRC, DST + off, C.byref(info))
            out[f"{entry}/{c}x{h}x{w}/elt{e}/dst+{off}"] = [rc, bytes(info).hex() if rc == 0 else
                                                           lib.marl_last_error().decode()]
        out[f"{entry}/null"] = [fn(3, 8, 8, 1, SRC, DST, None), lib.marl_last_error().decode()]
    return out


def _pixel_plans(lib):
    from marlclassification_amd import color, transforms

    shapes = [(c, h, w, e) for c in range(1, 5) for h in SIZES for w in SIZES for e in (1, 4)] + list(INVALID)
    out = {}
    norm, col, scratch = lib.marl_batch_normalize_plan, lib.marl_batch_color_plan, lib.marl_batch_stats_scratch_bytes
    norm.restype = col.restype = C.c_int
    norm.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3
    col.argtypes = [C.c_int] * 5 + [C.c_void_p] * 3
    scratch.restype, scratch.argtypes = C.c_size_t, [C.c_int] * 5

    def answer(rc, info):
        return [rc, bytes(info).hex() if rc == 0 else lib.marl_last_error().decode()]

    ninfo, cinfo = transforms.NormalizePlan(), color.ColorPlan()
    for (c, h, w, e), off in itertools.product(shapes, OFFSETS):
        C.memset(C.byref(ninfo), 0xff, C.sizeof(ninfo))
        out[f"marl_batch_normalize_plan/{c}x{h}x{w}/elt{e}/dst+{off}"] = answer(
            norm(c, h, w, e, SRC, DST + off, C.byref(ninfo)), ninfo)
        for form in (0, 1):
            C.memset(C.byref(cinfo), 0xff, C.sizeof(cinfo))
            out[f"marl_batch_color_plan/{c}x{h}x{w}/elt{e}/form{form}/dst+{off}"] = answer(
                col(c, h, w, e, form, SRC, DST + off, C.byref(cinfo)), cinfo)
    out["marl_batch_normalize_plan/null"] = [norm(3, 8, 8, 1, SRC, DST, None), lib.marl_last_error().decode()]
    out["marl_batch_color_plan/null"] = [col(3, 8, 8, 1, 0, SRC, DST, None), lib.marl_last_error().decode()]
    out["marl_batch_color_plan/form2"] = answer(col(3, 8, 8, 1, 2, SRC, DST, C.byref(cinfo)), cinfo)
    for (c, h, w, e), batch in itertools.product(shapes, (1, 4, 0, -1)):
        size = scratch(batch, c, h, w, e)
        out[f"marl_batch_stats_scratch_bytes/{batch}x{c}x{h}x{w}/elt{e}"] = [0 if size else 1, size]  # (0: refused)
    return out


def _guards(lib):
    lib.marl_last_error.restype = C.c_char_p
    cases = [dict(b) for b in BAD]
    for x, y in itertools.combinations(BAD, 2):
        if all(x[k] == y[k] for k in set(x) & set(y)):  # (two values for one argument are no pair)
            cases.append({**x, **y})
    out = {}
    for entry, tables in LAUNCHERS.items():
        fn = getattr(lib, entry)
        fn.restype = C.c_int
        fn.argtypes = ([C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p] + [C.c_void_p] * len(tables) + [C.c_int] * 6 +
                       [C.c_uint32, C.c_void_p])
        for kw in cases:
            if "mats" in kw and "mats" not in tables:
                continue
            a = {**GOOD, **kw}
            rc = fn(a["src"], a["n_src"], a["dst"], a["rows"], *(a[t] for t in tables), a["batch"], a["c"], a["h"],
                    a["w"], a["elt"], a["pad"], 0, None)
            msg = lib.marl_last_error().decode()
            assert rc != 0 and msg.startswith(entry + ":"), (entry, kw, rc, msg)  # (a guard's refusal: no launch)
            out[f"{entry}/{json.dumps(kw, sort_keys=True)}"] = [rc, msg]
    return out


def _pixel_guards(lib):
    out = {}
    for entry, t in PIXEL.items():
        cases = [dict(b) for b in t["bad"]]
        for x, y in itertools.combinations(t["bad"], 2):
            if all(x[k] == y[k] for k in set(x) & set(y)):  # (two values for one argument are no pair)
                cases.append({**x, **y})
        fn = getattr(lib, entry)
        fn.restype, fn.argtypes = C.c_int, t["types"]
        for kw in cases:
            a = {**t["good"], **kw}
            if a.get("usr") is not None:
                a["usr"] = C.cast((C.c_double * 6)(*a["usr"]), C.c_void_p)  # (six values: read for c <= 3 only)
            rc = fn(*(a[k] for k in t["args"]), None)
            msg = lib.marl_last_error().decode()
            assert rc != 0 and msg.startswith(entry + ":"), (entry, kw, rc, msg)  # (a guard's refusal: no launch)
            out[f"{entry}/{json.dumps(kw, sort_keys=True)}"] = [rc, msg]
    return out


def _differences(a, b):
    return sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--record", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        _, kp = _device_code(args.parent, tmp)
        _, kt = _device_code(args.tree, tmp)
    gathers = sorted(k for k in kt if "batch_augment_kernel" in k or "batch_mix_kernel" in k or "batch_warp_kernel" in k)
    device = {"kernels_parent": len(kp), "kernels_tree": len(kt), "gather_kernels": len(gathers),
              **{name + "s": sum(1 for k in kt if name in k) for name in (
                  "batch_stats_partial_kernel", "batch_stats_fold_kernel", "batch_normalize_kernel", "batch_color_kernel")},
              "kernels_that_differ": sorted(k for k in set(kp) & set(kt) if not _same(kp[k], kt[k])),
              "kernels_only_in_parent": sorted(set(kp) - set(kt)), "kernels_only_in_tree": sorted(set(kt) - set(kp))}
    device["identical"] = not (device["kernels_that_differ"] or device["kernels_only_in_parent"] or
                               device["kernels_only_in_tree"])
    libs = [C.CDLL(os.path.abspath(p)) for p in (args.parent, args.tree)]
    for lib in libs:
        lib.marl_last_error.restype = C.c_char_p
    res = {"device_code": device}
    sweeps = (("plans", _plans), ("guards", _guards), ("pixel_plans", _pixel_plans), ("pixel_guards", _pixel_guards))
    for key, sweep in sweeps:
        p, t = (sweep(lib) for lib in libs)
        diff = _differences(p, t)
        res[key] = {"entries": len(p), "refused": sum(1 for rc, _ in p.values() if rc != 0), "differences": diff[:40],
                    "identical": not diff}
    res["identical"] = all(res[k]["identical"] for k in ("device_code",) + tuple(k for k, _ in sweeps))
    print(json.dumps(res, indent=1))
    if args.record:
        full = json.load(open(args.record)) if os.path.exists(args.record) else {}
        full.update(res)
        with open(args.record, "w") as fh:
            json.dump(full, fh, indent=1)
            fh.write("\n")
    return 0 if res["identical"] else 1


if __name__ == "__main__":
    sys.exit(main())
