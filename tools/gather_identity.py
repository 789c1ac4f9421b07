#!/usr/bin/env python3
"""Identity of the batch-gather refactor (csrc/gather.h): the tree's libmarl_hip.so against the parent's.
No GPU: device code is read from the fat binary, plans are host arithmetic, and of the launchers only calls that a guard
refuses are made (made-up pointers, nothing is dereferenced, nothing is launched).

    python tools/gather_identity.py PARENT.so TREE.so [--record profiles/gather_identity.json]

Both libraries are built with the default flags (make -C marlclassification_amd/csrc).
  (a) device code: every kernel of the library equals the parent's of the same name in machine code, instruction lines
      and metadata (tools/conv_plan_identity.py's walk); no kernel is missing, none is new;
  (b) plans: marl_batch_augment_plan, marl_batch_mix_plan and marl_batch_warp_plan, return code and every field, over
      c 1..4 x h, w in SIZES x both element sizes x destination offsets OFFSETS, and the invalid shapes;
  (c) guards: for each launcher the return code and the marl_last_error text under each single bad argument of
      tests/test_gpu_warp.py::test_every_guard_of_the_c_entry and under every pair of them at once (the pairs pin the
      order of the guards).
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
              "kernels_that_differ": sorted(k for k in set(kp) & set(kt) if not _same(kp[k], kt[k])),
              "kernels_only_in_parent": sorted(set(kp) - set(kt)), "kernels_only_in_tree": sorted(set(kt) - set(kp))}
    device["identical"] = not (device["kernels_that_differ"] or device["kernels_only_in_parent"] or
                               device["kernels_only_in_tree"])
    libs = [C.CDLL(os.path.abspath(p)) for p in (args.parent, args.tree)]
    for lib in libs:
        lib.marl_last_error.restype = C.c_char_p
    res = {"device_code": device}
    for key, sweep in (("plans", _plans), ("guards", _guards)):
        p, t = (sweep(lib) for lib in libs)
        diff = _differences(p, t)
        res[key] = {"entries": len(p), "refused": sum(1 for rc, _ in p.values() if rc != 0), "differences": diff[:40],
                    "identical": not diff}
    res["identical"] = all(res[k]["identical"] for k in ("device_code", "plans", "guards"))
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
