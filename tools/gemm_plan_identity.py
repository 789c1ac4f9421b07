#!/usr/bin/env python3
"""Device-code identity of the matrix-product launcher refactor: every kernel of the tree's libmarl_hip.so has the
machine code, instruction lines and metadata (VGPR, SGPR, scratch, LDS) of the parent's kernel of the same name, and
the parent's kernels absent from the tree are exactly the instantiations the refactor deleted.  No GPU.

    python tools/gemm_plan_identity.py PARENT.so TREE.so [--record profiles/gemm_plan_identity.json]

Both libraries are built with the default flags (make -C marlclassification_amd/csrc).  The fatbin walk is the one of
tools/conv_plan_identity.py.  Exit status 0: identical.
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_plan_identity import _device_code  # noqa: E402

# gemm_nt_kernel<BM, BN, WM, WN, LSTM, GROUPS = 2>: the two-group schedule nothing could select; gemm_tn_kernel<BM, BN,
# WM, WN, BK, NBUF>: the BK = 16 forms and the two-stage 128-wide one behind `constexpr int tbk = 32`
DELETED = ["_ZN4marl14gemm_nt_kernelILi128ELi128ELi2ELi2ELb0ELi2EEEvNS_9GemmBatchE",
           "_ZN4marl14gemm_nt_kernelILi128ELi128ELi4ELi1ELb1ELi2EEEvNS_9GemmBatchE",
           "_ZN4marl14gemm_nt_kernelILi64ELi64ELi2ELi2ELb0ELi2EEEvNS_9GemmBatchE",
           "_ZN4marl14gemm_tn_kernelILi128ELi128ELi2ELi2ELi16ELi2EEEvPKfiS2_iPfiliillS3_iiii",
           "_ZN4marl14gemm_tn_kernelILi128ELi128ELi2ELi2ELi32ELi2EEEvPKfiS2_iPfiliillS3_iiii",
           "_ZN4marl14gemm_tn_kernelILi64ELi64ELi2ELi2ELi16ELi2EEEvPKfiS2_iPfiliillS3_iiii"]


def _same(a, b):
    """machine code and metadata equal; the instruction lines too (the last symbol of a code object also collects the
    lines that follow it in the listing: compared over the kernel's own length)"""
    n = min(len(a[1]), len(b[1]))
    return a[0] == b[0] and a[2] == b[2] and a[1][:n] == b[1][:n] and abs(len(a[1]) - len(b[1])) <= 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("tree")
    ap.add_argument("--record", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        _, kp = _device_code(args.parent, tmp)
        _, kt = _device_code(args.tree, tmp)
    differ = sorted(k for k in set(kp) & set(kt) if not _same(kp[k], kt[k]))
    gone, new = sorted(set(kp) - set(kt)), sorted(set(kt) - set(kp))
    res = {"method": "tools/conv_plan_identity.py's walk over every gfx950 code object of .hip_fatbin: machine code of "
                     "each kernel symbol, llvm-objdump -d instruction lines, AMDGPU metadata; default build flags; the "
                     "GROUPS template parameter is kept, so names compare without a map; the machine-code bytes and the "
                     "metadata are compared exactly, the instruction lines over the kernel's own length (the listing of "
                     "the last symbol of a code object also collects the line that follows it)",
           "kernels_parent": len(kp), "kernels_tree": len(kt), "kernels_compared": len(set(kp) & set(kt)),
           "kernels_that_differ": differ, "kernels_only_in_parent": gone,
           "kernels_only_in_tree": new, "deleted_as_intended": gone == sorted(DELETED)}
    ok = not differ and not new and res["deleted_as_intended"]
    res["identical"] = ok
    print(json.dumps({k: v for k, v in res.items() if k != "method"}, indent=1))
    if args.record:
        full = json.load(open(args.record)) if os.path.exists(args.record) else {}
        full["device_code"] = res
        with open(args.record, "w") as fh:
            json.dump(full, fh, indent=1)
            fh.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
