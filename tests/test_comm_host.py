"""CPU: communication graphs - the constructors of ``marlclassification_amd.comm``, the command-line spelling,
``marl.json``, the state dict under a matrix, the C ABI's new export, and the float64 reference the GPU tests use."""
import json
import os
import re

import numpy as np
import pytest
import torch as th

from marlclassification_amd import comm
from oracle import marl_oracle as mo
from tests.util import CASES, ROOT
from tests.util import small_model_config as _model_config


def _rows_ok(m):
    s = m.double().sum(1)
    return bool(((s - 1).abs() < 1e-6).logical_or(m.abs().sum(1) == 0).all())


@pytest.mark.parametrize("na", [1, 2, 3, 5, 16])
def test_constructors_are_row_normalised(na):
    mats = [comm.full(na), comm.none(na), comm.ring(na), comm.ring(na, 2), comm.star(na, na - 1)]
    if na == 16:
        mats += [comm.grid(4, 4), comm.grid(2, 8), comm.teams([3, 13]), comm.teams([1] * 16)]
    for m in mats:
        assert m.shape == (na, na) and m.dtype == th.float32 and _rows_ok(m)
        assert (m.diagonal() == 0).all() and (m >= 0).all()
        assert th.equal(comm.validate(m, na), m)


def test_full_is_the_mean_over_the_others():
    for na in (2, 3, 5, 16):
        ref = (1 - th.eye(na, dtype=th.float64)) / (na - 1)
        assert th.equal(comm.full(na), ref.float())
    assert th.equal(comm.full(1), th.zeros(1, 1))
    assert th.equal(comm.none(4), th.zeros(4, 4))


def test_adjacencies():
    r = comm.ring(5)
    for a in range(5):
        assert sorted(th.nonzero(r[a]).flatten().tolist()) == sorted({(a - 1) % 5, (a + 1) % 5})
        assert (r[a][r[a] != 0] == 0.5).all()
    assert (comm.ring(6, 2) != 0).sum(1).tolist() == [4] * 6
    assert th.equal(comm.ring(2), th.tensor([[0.0, 1.0], [1.0, 0.0]]))
    s = comm.star(5, 2)
    assert th.nonzero(s[2]).flatten().tolist() == [0, 1, 3, 4] and (s[2][s[2] != 0] == 0.25).all()
    for a in (0, 1, 3, 4):
        assert th.nonzero(s[a]).flatten().tolist() == [2] and s[a, 2] == 1.0
    g = comm.grid(2, 3)  # 0 1 2 / 3 4 5
    want = {0: [1, 3], 1: [0, 2, 4], 2: [1, 5], 3: [0, 4], 4: [1, 3, 5], 5: [2, 4]}
    for a, nb in want.items():
        assert th.nonzero(g[a]).flatten().tolist() == nb
        assert th.allclose(g[a][nb], th.full((len(nb),), 1.0 / len(nb)))
    t = comm.teams([2, 3, 1])
    blocks = th.block_diag(th.ones(2, 2), th.ones(3, 3), th.ones(1, 1)) - th.eye(6)
    assert th.equal(t != 0, blocks != 0) and t[0, 1] == 1.0 and t[2, 3] == 0.5 and (t[5] == 0).all()


def test_from_adjacency():
    a = th.tensor([[1, 1, 1], [0, 0, 0], [2, 0, 0]])
    m = comm.from_adjacency(a)
    assert th.equal(m, th.tensor([[0.0, 0.5, 0.5], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]))  # degree-0 row: zeros
    ms = comm.from_adjacency(a, self_loops=True)
    assert th.allclose(ms[0], th.full((3,), 1 / 3)) and (ms[1] == 0).all()
    assert th.equal(comm.from_adjacency(np.ones((3, 3))), comm.full(3))
    for bad in (th.ones(2, 3), th.ones(3), th.tensor([[float("nan")]])):
        with pytest.raises(ValueError):
            comm.from_adjacency(bad)


def test_validate():
    assert comm.validate([[0, 1], [1, 0]], 2).dtype == th.float32
    assert comm.validate(th.tensor([[-0.5, 2.0], [0.25, 1.0]]), None)[0, 0] == -0.5  # self-loops, negative: legal
    for bad, na in ((th.zeros(2, 3), None), (th.zeros(3, 3), 2), (th.zeros(3), 3),
                    (th.tensor([[float("inf")]]), 1), (th.tensor([[float("nan"), 0], [0, 0.0]]), 2),
                    (th.zeros(comm.MAX_AGENTS + 1, comm.MAX_AGENTS + 1), None), (th.zeros(0, 0), None)):
        with pytest.raises(ValueError):
            comm.validate(bad, na)


def test_parse_every_spelling(tmp_path):
    assert th.equal(comm.parse("full", 4), comm.full(4))
    assert th.equal(comm.parse("none", 4), comm.none(4))
    assert th.equal(comm.parse("ring", 5), comm.ring(5, 1))
    assert th.equal(comm.parse("ring:2", 7), comm.ring(7, 2))
    assert th.equal(comm.parse("star", 4), comm.star(4, 0))
    assert th.equal(comm.parse("star:3", 4), comm.star(4, 3))
    assert th.equal(comm.parse("grid:2x3", 6), comm.grid(2, 3))
    assert th.equal(comm.parse("teams:2,3", 5), comm.teams([2, 3]))
    m = th.tensor([[0.5, -1.0], [0.25, 0.0]])
    path = str(tmp_path / "m.npy")
    np.save(path, m.numpy())
    assert th.equal(comm.parse(path, 2), m)
    for bad, na in (("", 3), ("ring:", 3), ("ring:0", 3), ("ring:-1", 3), ("star:4", 4), ("grid:2x3", 5),
                    ("grid:2", 2), ("teams:2,3", 6), ("teams:", 3), ("teams:2,,3", 5), ("mesh", 3), ("full:2", 3),
                    (path, 3)):
        with pytest.raises(ValueError):
            comm.parse(bad, na)


def test_cli_accepts_every_spelling_and_rejects_malformed_ones(capsys):
    from marlclassification_amd.__main__ import build_parser

    p = build_parser()
    tails = {"train": ["-o", "out"],
             "test": ["--dataset-path", "d", "--json-path", "j", "--state-dict-path", "s", "-o", "out"],
             "infer": ["--images", "i", "--json-path", "j", "--state-dict-path", "s", "--class2idx", "c", "-o", "out"]}
    for mode, tail in tails.items():
        assert p.parse_args(["--run-id", "r", mode] + tail).comm is None
        for text in ("full", "none", "ring", "ring:2", "star", "star:1", "grid:2x2", "teams:1,2", "graph.npy"):
            assert p.parse_args(["--run-id", "r", mode, "--comm", text] + tail).comm == text
        for text in ("ring:", "ring:x", "grid:2", "grid:2x", "teams:", "teams:1,,2", "mesh", ".npy", "full:1"):
            with pytest.raises(SystemExit):
                p.parse_args(["--run-id", "r", mode, "--comm", text] + tail)
    capsys.readouterr()


def test_marl_json_round_trip(tmp_path):
    from marlclassification_amd.config import _MODEL_KEYS, ModelConfig

    plain, ring = str(tmp_path / "plain.json"), str(tmp_path / "ring.json")
    _model_config().save_marl_config(plain)
    _model_config(comm="ring:2").save_marl_config(ring)
    raw = json.load(open(plain))
    assert list(raw) == list(_MODEL_KEYS)  # a default run writes what it wrote before: no new key
    assert open(plain).read() == json.dumps({k: getattr(_model_config(), k) for k in _MODEL_KEYS})
    raw_ring = json.load(open(ring))
    assert raw_ring.pop("comm") == "ring:2" and raw_ring == raw
    assert ModelConfig.load_marl_config(plain).comm is None
    cfg = ModelConfig.load_marl_config(ring)
    assert cfg.comm == "ring:2"
    nets, _, _ = cfg.build_marl(5)
    assert th.equal(nets.comm, comm.ring(5, 2))
    assert ModelConfig.load_marl_config(plain).build_marl(5)[0].comm is None
    with pytest.raises(ValueError):
        _model_config(comm="grid:2x2").build_marl(5)


def test_state_dict_keys_do_not_change_under_a_matrix():
    nets = _model_config().build_networks()
    keys = list(nets.state_dict())
    nets.set_comm(comm.ring(3))
    assert nets.comm is not None and list(nets.state_dict()) == keys
    assert sorted(keys) == sorted(mo.param_shapes(mo.OracleConfig("mnist", 6, 12, 10, 8, 9, 4, 10, 16, 16)))
    fresh = _model_config().build_networks()
    fresh.load_state_dict(nets.state_dict())  # strict: nothing missing, nothing unexpected
    assert fresh.comm is None
    given = comm.ring(3)
    nets.set_comm(given)
    given[0, 1] = 7.0
    assert nets.comm[0, 1] == 0.5, "set_comm must not alias the caller's tensor"
    nets.set_comm(None)
    assert nets.comm is None
    for bad in (th.zeros(2, 3), th.tensor([[float("nan")]])):
        with pytest.raises(ValueError):
            nets.set_comm(bad)


def test_library_exports_the_entry_and_the_abi_stays_5():
    from marlclassification_amd import _lib

    assert "marl_comm_matrix" in _lib.EXPORTS and _lib.MARL_ABI_VERSION == 5
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    assert re.search(r"#define\s+MARL_ABI_VERSION\s+5\b", header)
    assert re.search(r"int\s+marl_comm_matrix\(const float\*\s*m_dev,\s*int nb_agents\);", header)
    lib = _lib.load()
    assert lib.marl_abi_version() == 5 and hasattr(lib, "marl_comm_matrix")
    # host-side argument checks (nothing touches a device): NULL clears, a bad size is refused
    assert lib.marl_comm_matrix(None, 0) == 0
    assert lib.marl_comm_matrix(1 << 12, 0) == -1 and lib.marl_comm_matrix(1 << 12, comm.MAX_AGENTS + 1) == -2
    assert lib.marl_comm_matrix(None, 0) == 0


@pytest.mark.parametrize("na", [2, 3, 5, 16])
def test_float64_reference_of_the_gpu_tests(na):
    """einsum('ac,cbk->abk', full(na), m) is the oracle's aggregate_messages."""
    m = th.randn(na, 4, 7, dtype=th.float64, generator=th.Generator().manual_seed(na))
    ref = mo.aggregate_messages(m)
    full64 = (1 - th.eye(na, dtype=th.float64)) / (na - 1)
    assert (th.einsum("ac,cbk->abk", full64, m) - ref).abs().max().item() <= 1e-12
    assert (th.einsum("ac,cbk->abk", comm.full(na).double(), m) - ref).abs().max().item() <= 1e-7  # fp32 entries
    one = th.randn(1, 4, 7, dtype=th.float64)
    assert th.equal(mo.aggregate_messages(one), th.einsum("ac,cbk->abk", comm.full(1).double(), one))
    assert CASES  # (the shared fixtures stay importable without a GPU)
