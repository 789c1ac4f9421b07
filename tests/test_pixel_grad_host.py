"""CPU: the image-gradient entry of the C ABI (ABI 5) is exported by the built library, declared in the header and
required by the loader; the ``infer`` command line takes ``--saliency`` (default off)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_image_gradient_entry():
    from marlclassification_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "marl_episode_backward_img")
    assert "marl_episode_backward_img" in _lib.EXPORTS
    assert lib.marl_abi_version() == 5 == _lib.MARL_ABI_VERSION


def test_header_declares_the_image_gradient_entry():
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    assert re.search(r"#define\s+MARL_ABI_VERSION\s+5\b", header)
    m = re.search(r"\bint\s+marl_episode_backward_img\s*\(([^;]*)\)\s*;", header)
    assert m, "marl_episode_backward_img is not declared"
    args = m.group(1)
    assert "float* d_img" in args and "grads_host" in args and args.rstrip().endswith("void* stream")
    # the existing entry keeps its signature (no d_img)
    old = re.search(r"\bint\s+marl_episode_backward\s*\(([^;]*)\)\s*;", header)
    assert old and "d_img" not in old.group(1)
    assert "core/environment.py:95-126" in header[header.index("ABI 5"):m.end()]


def test_infer_parser_takes_saliency_and_defaults_it_to_off():
    from marlclassification_amd.__main__ import build_parser
    from marlclassification_amd.config import InferConfig

    p = build_parser()
    base = "--run-id r infer --images a.png --json-path j --state-dict-path s --class2idx c.json -o out"
    assert p.parse_args(base.split()).saliency is False
    assert p.parse_args((base + " --saliency").split()).saliency is True
    cfg = InferConfig(state_dict_path="s", json_path="j", images_path=["a.png"], output_dir="o", class_to_idx="c")
    assert cfg.saliency is False
