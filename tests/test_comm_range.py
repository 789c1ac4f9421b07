"""CPU: range-limited communication - the torch builder ``comm.range_matrices`` against a float64 builder written
here, the command-line / marl.json surface of ``--comm-range``, and the ``set_comm_range`` guards that need no device."""
import json
import os
import re

import pytest
import torch as th

from marlclassification_amd import comm
from tests.util import small_model_config as _model_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def range_matrices64(base, pos, radius, metric, normalize):
    """float64 [Nb, Na, Na] for pos [Na, Nb, 2] (integers), loop by loop as the issue states the semantics."""
    na, nb = pos.shape[:2]
    base = base.double()
    w = th.zeros(nb, na, na, dtype=th.float64)
    for b in range(nb):
        for a in range(na):
            u = th.zeros(na, dtype=th.float64)
            for a2 in range(na):
                dy = abs(int(pos[a, b, 0]) - int(pos[a2, b, 0]))
                dx = abs(int(pos[a, b, 1]) - int(pos[a2, b, 1]))
                near = max(dy, dx) <= radius if metric == "chebyshev" else dy * dy + dx * dx <= radius * radius
                u[a2] = base[a, a2] if near else 0.0
            if normalize:
                big, small = float(base[a].sum()), float(u.sum())
                u = u * (big / small) if small > 0 else th.zeros(na, dtype=th.float64)
            w[b, a] = u
    return w


def _positions(na, nb, span, seed):
    return th.randint(0, span, (na, nb, 2), generator=th.Generator().manual_seed(seed))


@pytest.mark.parametrize("metric", comm.METRICS)
@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("base", ["full", "ring", "dense"])
def test_range_matrices_against_the_float64_builder(metric, normalize, base):
    na, nb, radius = 5, 7, 6
    pos = _positions(na, nb, 20, 3)
    b = {"full": comm.full(na), "ring": comm.ring(na),
         "dense": th.rand(na, na, generator=th.Generator().manual_seed(5))}[base]
    got = comm.range_matrices(None if base == "full" else b, pos, radius, metric, normalize)
    ref = range_matrices64(b, pos, radius, metric, normalize)
    assert got.shape == (nb, na, na) and got.dtype == th.float32
    assert th.equal(got != 0, ref != 0), "the gate is exact integer arithmetic: the supports must agree"
    assert (got.double() - ref).abs().max().item() <= 4 * th.finfo(th.float32).eps * float(ref.abs().max())
    if metric == "euclidean":  # (a corner pair: in range for chebyshev, out of range for euclidean)
        p = th.tensor([[[0, 0]], [[radius, radius]]])
        assert comm.range_matrices(None, p, radius, "chebyshev")[0, 0, 1] == 1.0
        assert comm.range_matrices(None, p, radius, "euclidean")[0, 0, 1] == 0.0


def test_empty_rows_complete_rows_and_self_loops():
    # agent 2 is far from everybody: its row is empty and the others renormalise over each other
    pos = th.tensor([[[0, 0]], [[3, 4]], [[90, 90]]])
    w = comm.range_matrices(None, pos, 5)[0]
    assert th.equal(w, th.tensor([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    raw = comm.range_matrices(None, pos, 5, normalize=False)[0]
    assert th.equal(raw, th.tensor([[0.0, 0.5, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    # everything in range: exactly the base, either normalisation
    for norm in (True, False):
        assert th.equal(comm.range_matrices(comm.ring(3), pos, 1000, normalize=norm)[0], comm.ring(3))
    # radius 0: only co-located agents; the base's diagonal decides self-loops
    eye = th.eye(3)
    assert th.equal(comm.range_matrices(eye, pos, 0)[0], eye)
    assert th.equal(comm.range_matrices(None, pos, 0)[0], th.zeros(3, 3))
    assert th.equal(comm.range_matrices(None, th.zeros(3, 1, 2, dtype=th.int64), 0)[0], comm.full(3))
    # leading dimensions: [Ns, Nb] between the agents and the coordinates
    pos4 = _positions(4, 6, 30, 1).reshape(4, 2, 3, 2)
    w4 = comm.range_matrices(None, pos4, 9, "euclidean")
    assert w4.shape == (2, 3, 4, 4)
    assert th.equal(w4.reshape(6, 4, 4), comm.range_matrices(None, pos4.reshape(4, 6, 2), 9, "euclidean"))


def test_one_agent():
    pos = _positions(1, 3, 10, 0)
    assert th.equal(comm.range_matrices(None, pos, 4), th.zeros(3, 1, 1))
    assert th.equal(comm.range_matrices(th.ones(1, 1), pos, 4), th.ones(3, 1, 1))
    assert th.equal(range_matrices64(th.ones(1, 1), pos, 4, "chebyshev", True), th.ones(3, 1, 1, dtype=th.float64))


def test_guards_of_the_builder():
    pos = _positions(3, 2, 10, 0)
    signed = th.tensor([[0.0, 1.0, -1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    with pytest.raises(ValueError, match=">= 0"):
        comm.range_matrices(signed, pos, 4)
    ref = range_matrices64(signed, pos, 4, "chebyshev", False)
    assert (comm.range_matrices(signed, pos, 4, normalize=False).double() - ref).abs().max().item() == 0.0
    for bad in (-1, 1.5, True, None, "3"):
        with pytest.raises(ValueError, match="radius"):
            comm.range_matrices(None, pos, bad)
    with pytest.raises(ValueError, match="metric"):
        comm.range_matrices(None, pos, 3, "manhattan")
    with pytest.raises(ValueError, match="positions"):
        comm.range_matrices(None, pos.float(), 3)
    with pytest.raises(ValueError):
        comm.range_matrices(comm.full(4), pos, 3)  # a base of another size


def test_parse_range_and_spelling():
    assert comm.parse_range("12") == comm.CommRange(12, "chebyshev", True)
    assert comm.parse_range("0:euclidean") == comm.CommRange(0, "euclidean", True)
    assert comm.parse_range("7:raw") == comm.CommRange(7, "chebyshev", False)
    assert comm.parse_range("7:euclidean:raw") == comm.CommRange(7, "euclidean", False)
    for text in ("12", "0:euclidean", "7:raw", "7:euclidean:raw"):
        assert comm.parse_range(text).spelling() == text
    assert comm.parse_range("7:chebyshev").spelling() == "7"
    for bad in ("", "-1", "1.5", "r", "7:", "7:raw:euclidean", "7:manhattan", "7:raw:raw", None):
        with pytest.raises(ValueError):
            comm.parse_range(bad)
    assert comm.CommRange(3).metric_id == 0 and comm.CommRange(3, "euclidean").metric_id == 1


def test_cli_accepts_the_spelling_and_rejects_malformed_ones(capsys):
    from marlclassification_amd.__main__ import build_parser, check_learn_comm

    p = build_parser()
    tails = {"train": ["-o", "out"],
             "test": ["--dataset-path", "d", "--json-path", "j", "--state-dict-path", "s", "-o", "out"],
             "infer": ["--images", "i", "--json-path", "j", "--state-dict-path", "s", "--class2idx", "c", "-o", "out"]}
    for mode, tail in tails.items():
        assert p.parse_args(["--run-id", "r", mode] + tail).comm_range is None
        for text, want in (("12", "12"), ("12:chebyshev", "12"), ("5:euclidean", "5:euclidean"), ("5:raw", "5:raw"),
                           ("0:euclidean:raw", "0:euclidean:raw")):
            args = p.parse_args(["--run-id", "r", mode, "--comm-range", text, "--comm", "ring"] + tail)
            assert args.comm_range == want and args.comm == "ring"
        for text in ("-3", "1.5", "x", "5:", "5:manhattan", "5:raw:euclidean"):
            with pytest.raises(SystemExit):
                p.parse_args(["--run-id", "r", mode, "--comm-range", text] + tail)
    args = p.parse_args(["--run-id", "r", "train", "--learn-comm", "--comm-range", "5"] + tails["train"])
    with pytest.raises(SystemExit):
        check_learn_comm(p, args)
    capsys.readouterr()


def test_marl_json_round_trip(tmp_path):
    from marlclassification_amd.config import _MODEL_KEYS, ModelConfig

    plain, ranged = str(tmp_path / "plain.json"), str(tmp_path / "ranged.json")
    _model_config().save_marl_config(plain)
    _model_config(comm="ring:2", comm_range="5:euclidean:raw").save_marl_config(ranged)
    raw = json.load(open(plain))
    assert list(raw) == list(_MODEL_KEYS)  # a default run writes what it wrote before: no new key
    raw_r = json.load(open(ranged))
    assert raw_r.pop("comm_range") == "5:euclidean:raw" and raw_r.pop("comm") == "ring:2" and raw_r == raw
    assert ModelConfig.load_marl_config(plain).comm_range is None
    assert ModelConfig.load_marl_config(plain).build_marl(5)[0].comm_range is None
    cfg = ModelConfig.load_marl_config(ranged)
    assert cfg.comm_range == "5:euclidean:raw"
    nets, _, _ = cfg.build_marl(5)
    assert nets.comm_range == comm.CommRange(5, "euclidean", False) and th.equal(nets.comm, comm.ring(5, 2))
    only = _model_config(comm_range="12").build_marl(3)[0]
    assert only.comm_range == comm.CommRange(12, "chebyshev", True) and only.comm is None
    with pytest.raises(ValueError):
        _model_config(comm_range="12:manhattan").build_marl(3)


def test_set_comm_range_guards_without_a_device():
    nets = _model_config().build_networks()
    keys = list(nets.state_dict())
    assert nets.comm_range is None
    nets.set_comm_range(6)
    assert nets.comm_range == (6, "chebyshev", True) and list(nets.state_dict()) == keys
    nets.set_comm_range(4, metric="euclidean", normalize=False)
    assert nets.comm_range == comm.CommRange(4, "euclidean", False)
    for bad in (-1, 2.0, True, "3"):
        with pytest.raises(ValueError, match="radius"):
            nets.set_comm_range(bad)
    with pytest.raises(ValueError, match="metric"):
        nets.set_comm_range(3, metric="l1")
    assert nets.comm_range == comm.CommRange(4, "euclidean", False), "a refused call must change nothing"
    nets.set_comm_range(None)
    assert nets.comm_range is None

    signed = th.tensor([[0.0, -1.0], [1.0, 0.0]])
    # a negative base under normalize=True: refused by whichever call comes second
    nets.set_comm(signed)
    with pytest.raises(ValueError, match=">= 0"):
        nets.set_comm_range(3)
    nets.set_comm_range(3, normalize=False)  # signed weights are fine without the rescaling
    nets.set_comm(None)
    nets.set_comm_range(3)
    with pytest.raises(ValueError, match=">= 0"):
        nets.set_comm(signed)
    assert nets.comm is None and nets.comm_range == comm.CommRange(3)
    nets.set_comm(comm.ring(4))  # a constant non-negative matrix composes in either order
    assert th.equal(nets.comm, comm.ring(4)) and nets.comm_range == comm.CommRange(3)

    # a live (learnable) source: refused by whichever call comes second
    live = comm.LearnableComm(comm.ring(4))
    with pytest.raises(ValueError, match="live"):
        nets.set_comm(live)
    assert nets.comm_source is None and th.equal(nets.comm, comm.ring(4))
    nets.set_comm_range(None)
    nets.set_comm(live)
    with pytest.raises(ValueError, match="live"):
        nets.set_comm_range(3)
    assert nets.comm_range is None and nets.comm_source is live


def test_step_surface_refuses_a_range_and_names_the_fused_episode():
    from marlclassification_amd.core import MultiAgent

    nets = _model_config().build_networks()
    nets.set_comm_range(5)
    obs, npos = th.zeros(3, 2, 1, 6, 6), th.zeros(3, 2, 2)
    with pytest.raises(RuntimeError, match="fused episode"):  # (refused before the state or a device is looked at)
        nets.forward(obs, th.zeros(3, 2, 8), npos, None)
    with pytest.raises(RuntimeError, match="fused episode"):
        nets.check_no_comm_range("MultiAgent.act")
    with pytest.raises(RuntimeError, match="fused episode"):
        MultiAgent(3, nets).act(obs, npos)


def test_library_exports_the_entry_and_the_abi_stays_5():
    from marlclassification_amd import _lib

    assert "marl_comm_range" in _lib.EXPORTS and _lib.MARL_ABI_VERSION == 5 and len(_lib.EXPORTS) == 57
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    assert re.search(r"#define\s+MARL_ABI_VERSION\s+5\b", header)
    assert re.search(r"int\s+marl_comm_range\(int radius,\s*int metric,\s*int normalize\);", header)
    lib = _lib.load()
    assert lib.marl_abi_version() == 5 and hasattr(lib, "marl_comm_range")
    # host-side argument checks (nothing touches a device): a bad metric is refused, a negative radius clears
    try:
        assert lib.marl_comm_range(3, 0, 1) == 0 and lib.marl_comm_range(3, 1, 0) == 0
        assert lib.marl_comm_range(3, 2, 1) == -1 and lib.marl_comm_range(3, -1, 1) == -1
    finally:
        assert lib.marl_comm_range(-1, 0, 1) == 0
