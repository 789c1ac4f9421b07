#!/usr/bin/env python3
"""Plan identity sweep of the conv launchers.  Host only: no GPU is touched.

    MARL_LIB_PATH=<a build of libmarl_hip.so> python tools/conv_plan_identity.py dump OUT.json
    python tools/conv_plan_identity.py compare PARENT.json TREE.json [--record profiles/conv_plan_identity.json]
    python tools/conv_plan_identity.py kernels PARENT.so TREE.so [--record profiles/conv_plan_identity.json]

`dump` writes what the library named by MARL_LIB_PATH (default: the tree's) plans, entry by entry:
  * marl_cnn_fwd_plan for every CNN_SPECS stack plus the custom stack of tests/conv_cases.py, windows 4..32, ROWS
    rows, train 0 and 1;
  * marl_cnn_bwd_plan for every layer of those stacks at the same row counts (first = 1 for every layer's raw shape,
    first = 0 for the layers that have a layer below), and marl_cnn_dgrad_scratch for the latter;
  * every key of tests/util.plan_witness plus marl_workspace_sizes (train 0 and 1) for tests/util's CASES and PLAN_CASES
    and bench.py's configurations;
each under the default knobs, cnn_fwd2=0, cnn_fwd3=0, wgrad3=0, dgrad_min_chunks=1 and 2^30, and - in a fresh process,
the switch is an environment variable - MARL_CNN_FUSED=0.  `compare` demands the two dumps be equal entry for entry and
records the count and one digest per library.  `kernels` compares the gfx950 device code of two builds: the sha-256 of
the .hip_fatbin sections and, kernel by kernel, the machine code of every code object in them (cnn_dgrad_kernel under one
name whether or not it still carries its template argument); for a kernel that differs, the instructions that do."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ROWS = (1, 5, 95, 1023, 4080, 65536)
KNOBS = (("default", None, None), ("cnn_fwd2=0", "cnn_fwd2", 0), ("cnn_fwd3=0", "cnn_fwd3", 0), ("wgrad3=0", "wgrad3", 0),
         ("dgrad_min_chunks=1", "dgrad_min_chunks", 1), ("dgrad_min_chunks=2^30", "dgrad_min_chunks", 1 << 30))
DEFAULTS = {"cnn_fwd2": 1, "cnn_fwd3": 1, "wgrad3": 1, "dgrad_min_chunks": 512}


def _stacks():
    from marlclassification_amd.engine import CNN_SPECS
    from tests import conv_cases as fwd

    return {**{k: (list(c), list(g)) for k, (c, g) in CNN_SPECS.items()}, "custom": fwd.CUSTOM}


def _shapes():
    """name -> (marl_config factory args): the goldens, the plan-coverage cases, the benchmark's configurations"""
    import bench
    from marlclassification_amd.engine import ModelSpec
    from tests.util import CASES, PLAN_CASES, Golden

    out = {}
    for tag, cfg in CASES.items():
        g = Golden(tag)
        out["golden/" + tag] = (cfg, g.na, g.nb, g.ns, tuple(g.img.shape[1:]))
    for tag, (cfg, na, nd, rep, ns, shape) in PLAN_CASES.items():
        out["plan/" + tag] = (cfg, na, nd * rep, ns, shape)
    benches = {"c3": (bench.C3, bench.NA, bench.NS, bench.IMG, 256)}
    benches.update({k: v[:5] for k, v in bench.OTHER.items()})
    for tag, (kw, na, ns, img, nb) in benches.items():
        out["bench/" + tag] = (ModelSpec(**kw), na, nb, ns, img)
    return out


def _sweep(lib):
    from marlclassification_amd import _lib
    from tests import conv_cases as fwd
    from tests.util import plan_witness

    out = {}
    for name, (ch, groups) in _stacks().items():
        for f in range(4, 33):
            cfg = fwd.config((ch, groups), f, f + 8, f + 10)
            for rows in ROWS:
                for train in (0, 1):
                    p = _lib.CnnFwdPlan()
                    rc = lib.marl_cnn_fwd_plan(C.byref(cfg), train, rows, C.byref(p))
                    out[f"fwd/{name}/f{f}/rows{rows}/train{train}"] = [rc, p.as_dict()]
            h = f
            for l in range(len(groups)):
                cin, cout = ch[l], ch[l + 1]
                for rows in ROWS:
                    for first in ((1, 0) if l else (1,)):
                        G = groups[l - 1] if l and not first else 1
                        p = _lib.CnnBwdPlan()
                        rc = lib.marl_cnn_bwd_plan(rows, cin, cout, h, G, first, C.byref(p))
                        out[f"bwd/{name}/f{f}/l{l}/rows{rows}/first{first}"] = [rc, p.as_dict()]
                    if l:
                        out[f"dgrad_scratch/{name}/f{f}/l{l}/rows{rows}"] = lib.marl_cnn_dgrad_scratch(
                            rows, cin, cout, h, groups[l - 1])
                h = (h - 1) // 2 + 1
    for tag, (cfg, na, nb, ns, shape) in _shapes().items():
        for train in (0, 1):
            out[f"witness/{tag}/train{train}"] = plan_witness(cfg, na, nb, ns, shape, train=bool(train))
            mc = _model_config(cfg, na, nb, ns, shape)
            wb, eb = C.c_size_t(0), C.c_size_t(0)
            rc = lib.marl_workspace_sizes(C.byref(mc), train, C.byref(wb), C.byref(eb))
            out[f"workspace/{tag}/train{train}"] = [rc, wb.value, eb.value]
    return out


def _model_config(cfg, na, nb, ns, shape):
    from tests.util import model_spec

    spec = cfg if hasattr(cfg, "config") else model_spec(cfg)
    return spec.config(na, nb, ns, *shape)


def dump(path, fused_off_child=False):
    from marlclassification_amd import _lib

    lib = _lib.load()
    out = {}
    if fused_off_child:
        assert os.environ.get("MARL_CNN_FUSED") == "0"
        out["MARL_CNN_FUSED=0"] = _sweep(lib)
    else:
        for tag, key, value in KNOBS:
            if key:
                _lib.check(lib.marl_tune(key.encode(), value))
            out[tag] = _sweep(lib)
            if key:
                _lib.check(lib.marl_tune(key.encode(), DEFAULTS[key]))
        child = path + ".fused_off"
        subprocess.run([sys.executable, os.path.abspath(__file__), "dump", child, "--fused-off-child"], check=True,
                       env=dict(os.environ, MARL_CNN_FUSED="0"))
        with open(child) as fh:
            out.update(json.load(fh))
        os.remove(child)
    with open(path, "w") as fh:
        json.dump(out, fh, sort_keys=True)
    print(f"{_lib.LIB_PATH}: {sum(len(v) for v in out.values())} entries under {len(out)} settings -> {path}")


def _digest(d):
    return hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()


def compare(a_path, b_path, record):
    a, b = (json.load(open(p)) for p in (a_path, b_path))
    diff = []
    for setting in sorted(set(a) | set(b)):
        ea, eb = a.get(setting, {}), b.get(setting, {})
        diff += [(setting, k, ea.get(k), eb.get(k)) for k in sorted(set(ea) | set(eb)) if ea.get(k) != eb.get(k)]
    entries = sum(len(v) for v in a.values())
    res = {"method": __doc__.split("`dump` writes", 1)[1].split("`compare`")[0].strip(),
           "settings": sorted(a), "entries": entries, "identical": not diff,
           "sha256_parent": _digest(a), "sha256_tree": _digest(b)}
    for d in diff[:40]:
        print("DIFF", *d)
    print(json.dumps({k: v for k, v in res.items() if k != "method"}, indent=1))
    if record:
        full = json.load(open(record)) if os.path.exists(record) else {}
        full["plan_sweep"] = res
        with open(record, "w") as fh:
            json.dump(full, fh, indent=1)
            fh.write("\n")
    return 1 if diff else 0


LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], capture_output=True, text=True, check=True).stdout


def _device_code(lib, tmp):
    """(sha-256 of .hip_fatbin, {kernel: (machine code, instruction lines, metadata)}) over every gfx950 code object"""
    import re
    import struct

    fb = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fb], check=True)
    data = open(fb, "rb").read()
    kernels = {}
    at = data.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        q = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, q)
            triple = data[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "gfx950" not in triple:
                continue
            co = os.path.join(tmp, "co")
            with open(co, "wb") as fh:
                fh.write(data[at + off:at + off + size])
            m = re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", _tool("llvm-readelf", "-SW", co))
            addr, toff = int(m.group(1), 16), int(m.group(2), 16)
            elf = open(co, "rb").read()
            dis = re.split(r"^[0-9a-f]+ <([^>]+)>:$", _tool("llvm-objdump", "-d", "--no-show-raw-insn", co), flags=re.M)
            text = dict(zip(dis[1::2], dis[2::2]))
            notes = _tool("llvm-readelf", "--notes", co)
            for ln in _tool("llvm-readelf", "-sW", co).splitlines():
                f = ln.split()
                if len(f) >= 8 and f[3] == "FUNC":
                    name, a, sz = f[7], int(f[1], 16), int(f[2])
                    ins = [re.sub(r"\s*//.*$", "", x).strip() for x in text.get(name, "").splitlines()]
                    meta = {k: int(v) for k, v in re.findall(
                        r"\.(kernarg_segment_size|group_segment_fixed_size|private_segment_fixed_size|sgpr_count|"
                        r"sgpr_spill_count|vgpr_count|vgpr_spill_count):\s+(\d+)", _kernel_block(notes, name))}
                    key = re.sub(r"cnn_dgrad_kernelILb0EEEv", "cnn_dgrad_kernelE", name)
                    kernels[key] = (elf[toff + a - addr:toff + a - addr + sz], [x for x in ins if x], meta)
        at = data.find(MAGIC, at + 1)
    return hashlib.sha256(data).hexdigest(), kernels


def _kernel_block(notes, name):
    """the metadata map of one kernel in the AMDGPU note (maps start at '  - .agpr_count' and hold one '.name:')"""
    blocks = notes.split("\n  - .agpr_count")
    for b in blocks:
        if ".name:           " + name + "\n" in b:
            return b
    return ""


def kernels(parent, tree, record):
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        sha_p, kp = _device_code(parent, tmp)
        sha_t, kt = _device_code(tree, tmp)
    res = {"method": "llvm-objcopy --only-section=.hip_fatbin, sha-256; every gfx950 code object of the section: machine "
                     "code of each kernel symbol, llvm-objdump -d instruction lines, AMDGPU metadata",
           "hip_fatbin_sha256_parent": sha_p, "hip_fatbin_sha256_tree": sha_t, "kernels_parent": len(kp),
           "kernels_tree": len(kt), "kernel_names_equal": sorted(kp) == sorted(kt), "kernels_that_differ": {}}
    for k in sorted(set(kp) & set(kt)):
        if kp[k][0] == kt[k][0] and kp[k][2] == kt[k][2]:
            continue
        a, b = kp[k][1], kt[k][1]
        res["kernels_that_differ"][k] = {
            "code_bytes": [len(kp[k][0]), len(kt[k][0])], "instructions": [len(a), len(b)],
            "instructions_that_differ": [[i, x, y] for i, (x, y) in enumerate(zip(a, b)) if x != y][:20],
            "metadata_parent": kp[k][2], "metadata_tree": kt[k][2]}
    print(json.dumps({k: v for k, v in res.items() if k != "method"}, indent=1))
    if record:
        full = json.load(open(record)) if os.path.exists(record) else {}
        full["device_code"] = res
        with open(record, "w") as fh:
            json.dump(full, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("dump")
    d.add_argument("out")
    d.add_argument("--fused-off-child", action="store_true", help=argparse.SUPPRESS)
    c = sub.add_parser("compare")
    c.add_argument("parent")
    c.add_argument("tree")
    c.add_argument("--record", default=None)
    k = sub.add_parser("kernels")
    k.add_argument("parent")
    k.add_argument("tree")
    k.add_argument("--record", default=None)
    args = ap.parse_args()
    if args.cmd == "dump":
        dump(args.out, args.fused_off_child)
    elif args.cmd == "kernels":
        sys.exit(kernels(args.parent, args.tree, args.record))
    else:
        sys.exit(compare(args.parent, args.tree, args.record))
