"""Shapes, inputs and float64 references of the step loop's row kernels (tests/test_gpu_row_fwd.py runs the kernels
against them, tests/test_row_refs_host.py checks the references alone).  Everything here is torch on the CPU; nothing
calls the library."""
import torch as th
import torch.nn.functional as F

EPS = 1e-5  # LayerNorm / GroupNorm epsilon of the model

# ---- GroupNorm + SiLU forward: (P, C, G) by the form the launcher takes -------------------------------------------
GN_CASES = {
    "flat4": [(4, 64, 8), (9, 16, 4), (4, 8, 8)],      # row <= 256 elements; the last: one channel per group
    "flat9": [(9, 32, 4), (36, 8, 2), (36, 16, 4)],    # <= 576
    "flat16": [(16, 64, 8), (49, 16, 4)],              # <= 1024
    "general": [(9, 24, 3), (36, 32, 4)],              # no power of two; a power-of-two row longer than 1024
}
GN_ROWS = [1, 5, 67]
GN_OFFSET = {"flat4": (9, 16, 4), "flat9": (36, 16, 4), "flat16": (49, 16, 4), "general": (9, 24, 3)}


def gn_form(P, C):
    """the launcher's choice (csrc/rowops.hip, launch_gn_silu_fwd)"""
    if C & (C - 1) or C < 4 or C > 64 or P * C > 1024:
        return "general"
    return "flat4" if P * C <= 256 else ("flat9" if P * C <= 576 else "flat16")


# ---- LayerNorm + SiLU forward with the dot ---------------------------------------------------------------------------
LN_N_REG = [13, 64, 128, 129, 320, 384]  # <= 128: two elements per lane; <= 384: six
LN_N_GENERAL = [400, 1000]
LN_M = [1, 8, 9, 67]
LN_OFFSET_N = [128, 384, 400]            # one per kernel

# the offset inputs of both norms: mean OFFSET_MEAN, standard deviation OFFSET_STD.  (The condition under which the
# kernels are held to FWD_TOL there - fp32 torch on the CPU stays within FWD_TOL / 4 of float64 - holds at mean 8:
# tests/test_row_refs_host.py.)
OFFSET_MEAN, OFFSET_STD = 8.0, 0.5


def norm_input(shape, seed, offset=False):
    x = th.randn(*shape, generator=th.Generator().manual_seed(seed))
    return x * OFFSET_STD + OFFSET_MEAN if offset else x * 2 + 0.5


def affine(n, seed):
    g = th.Generator().manual_seed(seed + 7919)
    return th.randn(n, generator=g), th.randn(n, generator=g) * 0.5


def gn_silu(z, gamma, beta, G):
    """z [rows, P, C] (NHWC rows) -> (activation [rows, C, P], stats [rows, G, 2] = mean, rstd) in z's dtype"""
    rows, P, C = z.shape
    x = z.permute(0, 2, 1)
    act = F.silu(F.group_norm(x, G, gamma, beta, EPS))
    xg = x.reshape(rows, G, -1)
    stats = th.stack([xg.mean(-1), 1.0 / th.sqrt(xg.var(-1, unbiased=False) + EPS)], -1)
    return act, stats


def im2col(act, hin):
    """act [rows, C, P = hin * hin] -> the next layer's im2col rows (3x3, stride 2, padding 1)
    [rows * hout * hout, 9 C], column (kh * 3 + kw) * C + c"""
    rows, C, _ = act.shape
    u = F.unfold(act.reshape(rows, C, hin, hin), kernel_size=3, stride=2, padding=1)  # [rows, C * 9, L], row c * 9 + tap
    L = u.shape[-1]
    return u.reshape(rows, C, 9, L).permute(0, 3, 2, 1).reshape(rows * L, 9 * C)


def ln_silu(z, gamma, beta):
    """z [m, n] -> (activation, stats [m, 2] = mean, rstd)"""
    act = F.silu(F.layer_norm(z, (z.shape[1],), gamma, beta, EPS))
    stats = th.stack([z.mean(-1), 1.0 / th.sqrt(z.var(-1, unbiased=False) + EPS)], -1)
    return act, stats


# ---- position embedding --------------------------------------------------------------------------------------------
POS_ND = [1, 8, 16, 19]
POS_ROWS = [1, 127, 129]
POS_HW = (28, 36)

# ---- LSTM cell backward ------------------------------------------------------------------------------------------------
CELL_N_VEC4 = [4, 20, 64]
CELL_N_SCALAR = 23
CELL_ROWS = [1, 3, 65]
CELL_PAIRS = [(64, 20), (20, 23)]
SATURATED = 30.0


class CellInputs:
    """one cell's operands, fp32: the activated gates i | f | g | o [rows, 4 n] and c_new as the forward rounds them
    (float64 activations of the pre-activations, rounded once), c_prev, dL/dh and dL/dc"""

    def __init__(self, rows, n, seed, saturated=False):
        g = th.Generator().manual_seed(seed)
        if saturated:
            self.pre = (th.randint(0, 2, (rows, 4 * n), generator=g).float() * 2 - 1) * SATURATED
        else:
            self.pre = th.randn(rows, 4 * n, generator=g) * 1.5
        self.c_prev = th.randn(rows, n, generator=g)
        self.dh = th.randn(rows, n, generator=g)
        self.dc = th.randn(rows, n, generator=g)
        gates64, c_new64, _ = cell_forward(self.pre.double(), self.c_prev.double())
        self.gates, self.c_new = gates64.float(), c_new64.float()
        self.rows, self.n = rows, n


def cell_forward(pre, c_prev):
    """networks/recurrent.py:19-35: (activated gates, c_new, h_new)"""
    n = c_prev.shape[1]
    i, f, o = th.sigmoid(pre[:, :n]), th.sigmoid(pre[:, n:2 * n]), th.sigmoid(pre[:, 3 * n:])
    g = th.tanh(pre[:, 2 * n:3 * n])
    c_new = f * c_prev + i * g
    return th.cat([i, f, g, o], 1), c_new, o * th.tanh(c_new)


def cell_bwd_formulas(gates, c_prev, c_new, dh, dc):
    """the kernel's formulas in float64 on the given (fp32-rounded) operands: (d pre-activations [rows, 4 n],
    dL/dc_prev)"""
    gates, c_prev, c_new, dh, dc = (t.double() for t in (gates, c_prev, c_new, dh, dc))
    n = c_prev.shape[1]
    gi, gf, gg, go = (gates[:, k * n:(k + 1) * n] for k in range(4))
    tc = th.tanh(c_new)
    dcv = dh * go * (1 - tc * tc) + dc
    dgates = th.cat([dcv * gg * gi * (1 - gi), dcv * c_prev * gf * (1 - gf), dcv * gi * (1 - gg * gg),
                     dh * tc * go * (1 - go)], 1)
    return dgates, dcv * gf


def saturated_bound(x):
    """every gate gradient of a saturated cell carries a factor sigma'(+-30) <= e^-30 or 1 - tanh^2(+-30) <= 4 e^-60,
    times dL/dh or dcv = dh o (1 - tanh^2 c) + dc, times at most max(1, |c_prev|)"""
    import math

    big = (x.dh.abs() + x.dc.abs()).max().item() * max(1.0, x.c_prev.abs().max().item())
    return math.exp(-SATURATED) * big * 1.01


# ---- policy logit gradients ------------------------------------------------------------------------------------------
POLICY_NA = [1, 3, 4, 5, 8, 12, 16]  # 16: the library's maximum (MARL_MAX_ACTIONS)
POLICY_ROWS = [1, 255, 257]
EXPLORE_EPS = 0.25
EXPLORE_TAU = [1.0, 0.5]


def explore_keep_floor(n_actions, eps=EXPLORE_EPS):
    """pi_b = keep * softmax(z / tau) + floor (marlclassification_amd/explore.py): keep = 1 - eps, floor = eps / nA"""
    return 1.0 - eps, eps / n_actions


class PolicyInputs:
    def __init__(self, rows, n_actions, seed, tau=1.0, eps=0.0):
        g = th.Generator().manual_seed(seed)
        self.logits = (th.randn(rows, n_actions, generator=g) * 1.5).double()
        self.actions = th.randint(0, n_actions, (rows,), generator=g, dtype=th.int32)
        self.dlogp = th.randn(rows, generator=g)
        self.dprobs = th.randn(rows, n_actions, generator=g)
        self.tau, (self.keep, self.floor) = tau, explore_keep_floor(n_actions, eps)
        self.probs = behaviour(self.logits, tau, self.keep, self.floor).float()  # the saved row
        self.rows, self.n_actions = rows, n_actions


def behaviour(logits, tau, keep, floor):
    return keep * th.softmax(logits / tau, -1) + floor


def onehot(actions, n_actions):
    return F.one_hot(actions.long(), n_actions).double()


def dlogits_plain(probs, actions, dlogp):
    """form 0 on the saved row: g (1[j == a] - p)"""
    g = th.zeros(probs.shape[0], dtype=th.float64) if dlogp is None else dlogp.double()
    return g[:, None] * (onehot(actions, probs.shape[1]) - probs.double())


def dlogits_probs(probs, actions, dlogp, dprobs):
    """form 1: the softmax backward of dL/dprobs plus the log-prob term"""
    p, g = probs.double(), dprobs.double()
    return p * (g - (p * g).sum(-1, keepdim=True)) + dlogits_plain(probs, actions, dlogp)


def dlogits_explore_formula(probs, actions, dlogp, dprobs, tau, keep, floor):
    """form 2, the kernel's formula in float64 on the saved row: s = (pi_b - floor) / keep, G = keep (g + gl 1[j == a]
    / pi_b[a]) (the log-prob term dropped where pi_b[a] == 0), dz = s (G - s . G) / tau"""
    pb = probs.double()
    g = th.zeros_like(pb) if dprobs is None else dprobs.double()
    if dlogp is not None:
        pa = pb.gather(1, actions.long()[:, None])
        la = th.where(pa > 0, dlogp.double()[:, None] / pa.clamp_min(1e-300), th.zeros_like(pa))
        g = g + la * onehot(actions, pb.shape[1])
    s = (pb - floor).clamp_min(0) / keep
    G = keep * g
    return s * (G - (s * G).sum(-1, keepdim=True)) / tau


def dlogits_explore_autograd(logits, actions, dlogp, dprobs, tau, keep, floor):
    """form 2 by float64 autograd from the logits through pi_b = keep softmax(z / tau) + floor"""
    z = logits.clone().requires_grad_()
    pb = behaviour(z, tau, keep, floor)
    loss = pb.sum() * 0
    if dprobs is not None:
        loss = loss + (pb * dprobs.double()).sum()
    if dlogp is not None:
        loss = loss + (dlogp.double() * th.log(pb.gather(1, actions.long()[:, None])[:, 0])).sum()
    loss.backward()
    return z.grad


# ---- row dot and message mean ------------------------------------------------------------------------------------------
ROWDOT_N = [1, 63, 64, 65, 384]
ROWDOT_ROWS = [1, 4, 5]
AGG_NA = [1, 2, 5, 16]
AGG_NB = [1, 7]
AGG_N = [1, 21, 64]


def agg_msg(m, na, nb):
    """networks/message.py:5-17 on rows a * nb + b: (sum over the agents - own) / (na - 1); zeros for one agent"""
    m = m.double().reshape(na, nb, -1)
    if na == 1:
        return th.zeros_like(m).reshape(na * nb, -1)
    return ((m.sum(0, keepdim=True) - m) / (na - 1)).reshape(na * nb, -1)
