"""Parity toolkit of the GPU tests: the project's tolerances, the two closeness asserts and the ``Recorder`` that
keeps a file's achieved errors and writes them through ``tests.util.record`` after every entry.

The two bounds differ and stay apart: ``close`` is ``tol * |ref|max + 1e-7`` (gradients: relative to the tensor's
scale), ``close_fwd`` / ``Recorder.fwd`` is ``tol * max(1, |ref|max)`` (forward outputs and scalars).  pytest rewrites
asserts in test modules only, so every assert here carries its tag and its numbers in the message."""
import torch as th

from tests.util import record

FWD_TOL = 1e-5     # forward outputs (x max(1, |ref|))
GRAD_TOL = 1e-4    # gradients (x max |ref|), the project's gradient tolerance
UPDATE_TOL = 2 * 1e-3  # (x lr) an Adam update of the trainer tests of the loss options


def close(got, ref, tol, what):
    got = got.detach().double().cpu()
    # (no float64 gradient: the oracle's graph does not reach this tensor - Na = 1 has no message path)
    ref = th.zeros_like(got) if ref is None else ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)}, reference {tuple(ref.shape)}"
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    scale = ref.abs().max().item()
    assert err <= tol * scale + 1e-7, f"{what}: max err {err:.3e} (ref max {scale:.3e})"


def close_fwd(got, ref, what):
    err = (got.detach().double().cpu() - ref.detach().double().cpu()).abs().max().item()
    assert err <= FWD_TOL * max(1.0, ref.abs().max().item()), f"{what}: max err {err:.3e}"


def param_grads_match(model, p64, tol=GRAD_TOL, prefix=""):
    for n, p in model.named_parameters():
        assert p.grad is not None, f"{prefix}{n}: no gradient"
        close(p.grad, p64[n].grad, tol, prefix + n)


class Recorder:
    """The achieved errors of one record file (``<ROUND>_<record_name>[_<family>].json``), printed as
    ``[label] tag: ...``.  Recorders of one file share its entries, so a test that borrows another file's record adds
    to it instead of replacing it."""

    _entries = {}

    def __init__(self, record_name, label, family=None):
        self.name = record_name if family in (None, "default") else f"{record_name}_{family}"
        self.label = label
        self.errors = Recorder._entries.setdefault(self.name, {})

    def save(self):
        record(self.name, self.errors)

    def put(self, tag, entry):
        self.errors[tag] = entry
        self.save()

    def rec(self, tag, got, ref, tol):
        got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
        err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
        print(f"[{self.label}] {tag}: max err {err:.3e}, ref max {scale:.3e}, tol {tol:g}")
        self.put(tag, {"max_err": err, "ref_max": scale, "tol": tol})
        return err, scale

    def fwd(self, tag, got, ref):
        err, scale = self.rec(tag, got, ref, FWD_TOL)
        assert err <= FWD_TOL * max(1.0, scale), f"{tag}: max err {err:.3e}"

    def grad(self, tag, got, ref):
        self.rec(tag, got, ref, GRAD_TOL)
        close(got, ref, GRAD_TOL, tag)

    def param_grads(self, tag, model, p64):
        worst, where = 0.0, ""
        for n, p in model.named_parameters():
            ref = p64[n].grad
            if p.grad is not None and ref is not None and ref.abs().max().item() > 0.0:
                rel = (p.grad.double().cpu() - ref).abs().max().item() / ref.abs().max().item()
                if rel >= worst:
                    worst, where = rel, n
        print(f"[{self.label}] {tag}: worst err / ref max {worst:.3e} ({where})")
        self.put(tag, {"worst_err_over_ref_max": worst, "param": where, "tol": GRAD_TOL})
        param_grads_match(model, p64, prefix=f"{tag}/")

    def _update_within(self, tag, k, model, after, grads_list, bound):
        sd = model.state_dict()
        worst = 0.0
        for n in k.params:
            ref_upd = after[n] - k.params[n].double()
            upd = sd[n].double().cpu() - k.params[n].double()
            big = th.ones_like(ref_upd, dtype=th.bool)
            for g in grads_list:  # (Adam's sign-like first update amplifies a gradient that is zero up to rounding)
                big &= g[n].abs() > 1e-6
            if big.any():
                err = (upd[big] - ref_upd[big]).abs().max().item()
                worst = max(worst, err)
                assert err <= bound, f"{tag}: {n}: {err:.3e} (bound {bound:.1e})"
        print(f"[{self.label}] {tag}: max err {worst:.3e} (bound {bound:.1e})")
        self.put(tag, {"max_err": worst, "tol": bound})

    def updates_match(self, tag, k, model, after, grads_list, lr, n_updates):
        """The model's parameters moved like the float64 Adam updates ``after``: 1e-3 lr per update."""
        self._update_within(tag, k, model, after, grads_list, n_updates * 1e-3 * lr)

    def check_update(self, tag, k, model, after, grad_sets, lr):
        """The same comparison under ``UPDATE_TOL * lr`` whatever the number of updates, recorded as ``tag/update``."""
        self._update_within(f"{tag}/update", k, model, after, grad_sets, UPDATE_TOL * lr)
