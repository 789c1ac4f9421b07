// Host-side orchestration of the episode (EpisodeSampler.__episode_impl,
// core/episode.py:32-82) and of loss.backward() through it, plus the C ABI of
// include/marl_hip.h.  Everything here only computes buffer layouts inside the two
// caller-owned workspaces and enqueues kernels on the caller's stream.
//
// Structure of one training iteration (R = Na*Nb rows, r = a*Nb + b):
//   forward, t = 0..Ns-1 (strictly sequential: positions depend on sampled actions)
//     gather+im2col -> [conv GEMM -> GroupNorm+SiLU -> im2col]*  -> b_t  into U[t]
//     message mean -> decode MLP -> d_t into U[t];  position embedding -> lambda_t into U[t]
//     belief + action LSTM: one grouped MFMA GEMM with the cell update fused in the epilogue
//     encode MLP -> msg_{t+1};  policy hidden -> output layer + softmax + sample + move
//   after the loop (batched over all Ns*R rows, better GEMM shapes):
//     critic and prediction heads on the saved h / h^ of every step
//   backward: heads batched first (their inputs' gradients do not depend on the recurrence),
//     then the reverse-time loop over only the recurrent chain (LSTM cells, message
//     decode/encode), then every weight gradient as ONE row-contraction GEMM over all
//     Ns*R rows, the full dU, and the CNN backward batched over all steps.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/marl_hip_rowops.h"
#include "../../include/marl_hip_cnnops.h"
#include "../../include/marl_hip_explore.h"
#include "../../include/marl_hip_classloss.h"
#include "../../include/marl_hip_softtargets.h"
#include "common.h"

namespace marl {

// ---------------------------------------------------------------------------
// dimensions
// ---------------------------------------------------------------------------
struct Dims {
    int na, nb, ns;
    int64_t R, NR;
    int H, W, c_img, f;
    int L;
    int ch[MARL_MAX_CNN_LAYERS + 1];
    int grp[MARL_MAX_CNN_LAYERS];
    int hw[MARL_MAX_CNN_LAYERS + 1];  // spatial size entering layer l (hw[0] = f)
    int P[MARL_MAX_CNN_LAYERS];       // output positions of layer l
    int K[MARL_MAX_CNN_LAYERS];       // 9 * cin
    int ldk[MARL_MAX_CNN_LAYERS];
    int nf, nin;
    int n_b, n_a, n_m, nm2, n_mo, n_d, nA, nC, nlb, nla;
    int ld_nin, ld_nb, ld_na, ld_nm, ld_nm2, ld_nmo, ld_nd, ld_nla, ld_nlb, ld_gb, ld_ga, ld_nC,
        ld_nA;
    int ld_dbl;  // row stride of d(decoded message | position embedding): pad4(n_mo + n_d)
};

static int make_dims(const marl_config* c, Dims& d) {
    if (!c) {
        set_error("null config");
        return MARL_EINVAL;
    }
    memset(&d, 0, sizeof(d));
    d.na = c->nb_agents;
    d.nb = c->batch;
    d.ns = c->nb_steps;
    d.H = c->img_h;
    d.W = c->img_w;
    d.c_img = c->img_c;
    d.f = c->window;
    d.L = c->cnn_layers;
    if (d.na < 1 || d.nb < 1 || d.ns < 1 || d.f < 1 || d.H <= d.f || d.W <= d.f || d.c_img < 1) {
        set_error("bad episode shape na=%d nb=%d ns=%d f=%d img=%dx%dx%d", d.na, d.nb, d.ns, d.f,
                  d.c_img, d.H, d.W);
        return MARL_EINVAL;
    }
    if (d.L < 1 || d.L > MARL_MAX_CNN_LAYERS) {
        set_error("cnn_layers %d outside [1,%d]", d.L, MARL_MAX_CNN_LAYERS);
        return MARL_ELIMIT;
    }
    d.R = (int64_t)d.na * d.nb;
    d.NR = d.R * d.ns;
    d.hw[0] = d.f;
    for (int l = 0; l <= d.L; ++l) d.ch[l] = c->cnn_ch[l];
    if (d.ch[0] < 1 || d.ch[0] > d.c_img) {
        set_error("cnn input channels %d vs image channels %d", d.ch[0], d.c_img);
        return MARL_EINVAL;
    }
    for (int l = 0; l < d.L; ++l) {
        d.grp[l] = c->cnn_groups[l];
        if (d.ch[l + 1] < 1 || d.grp[l] < 1 || d.ch[l + 1] % d.grp[l] != 0 || (d.ch[l + 1] & 3)) {
            set_error("cnn layer %d: %d channels / %d groups unsupported (channels must be a "
                      "multiple of 4 and of the group count)", l, d.ch[l + 1], d.grp[l]);
            return MARL_ELIMIT;
        }
        d.hw[l + 1] = (d.hw[l] - 1) / 2 + 1;
        d.P[l] = d.hw[l + 1] * d.hw[l + 1];
        d.K[l] = 9 * d.ch[l];
        d.ldk[l] = p4(d.K[l]);
    }
    d.nf = d.ch[d.L] * d.P[d.L - 1];
    d.n_b = c->n_b;
    d.n_a = c->n_a;
    d.n_m = c->n_m;
    d.nm2 = 2 * c->n_m;
    d.n_mo = c->n_m_o;
    d.n_d = c->n_d;
    d.nA = c->nb_action;
    d.nC = c->nb_class;
    d.nlb = c->nlb;
    d.nla = c->nla;
    if (d.n_b < 1 || d.n_a < 1 || d.n_m < 1 || d.n_mo < 1 || d.n_d < 1 || d.nA < 1 || d.nC < 1 ||
        d.nlb < 1 || d.nla < 1) {
        set_error("non-positive hidden size");
        return MARL_EINVAL;
    }
    if (d.nA > MARL_MAX_ACTIONS || d.nC > 1024 || d.nlb > 2048 || d.nla > 2048 || d.nm2 > 2048 ||
        d.n_mo > 2048 || d.n_d > 2048) {
        set_error("dimension above the supported range (nA<=16, nC<=1024, LayerNorm width<=2048)");
        return MARL_ELIMIT;
    }
    d.nin = d.nf + d.n_mo + d.n_d;
    d.ld_nin = p4(d.nin);
    d.ld_nb = p4(d.n_b);
    d.ld_na = p4(d.n_a);
    d.ld_nm = p4(d.n_m);
    d.ld_nm2 = p4(d.nm2);
    d.ld_nmo = p4(d.n_mo);
    d.ld_dbl = p4(d.n_mo + d.n_d);
    d.ld_nd = p4(d.n_d);
    d.ld_nla = p4(d.nla);
    d.ld_nlb = p4(d.nlb);
    d.ld_gb = p4(4 * d.n_b);
    d.ld_ga = p4(4 * d.n_a);
    d.ld_nC = p4(d.nC);
    d.ld_nA = p4(d.nA);
    return MARL_OK;
}

// ---------------------------------------------------------------------------
// parameters
// ---------------------------------------------------------------------------
enum ParamKind { PK_NONE = 0, PK_MATRIX, PK_CONV, PK_VEC };
struct ParamMeta {
    ParamKind kind;
    int n, k;  // matrix [n, k]; conv [n, ci(=k/9), 3, 3]; vec [n]
};

static ParamMeta param_meta(const Dims& d, int idx) {
    auto M = [](int n, int k) { return ParamMeta{PK_MATRIX, n, k}; };
    auto V = [](int n) { return ParamMeta{PK_VEC, n, 1}; };
    if (idx < 20) {
        const int l = idx / 4, w = idx % 4;
        if (l >= d.L) return ParamMeta{PK_NONE, 0, 0};
        if (w == 0) return ParamMeta{PK_CONV, d.ch[l + 1], d.K[l]};
        return V(d.ch[l + 1]);
    }
    switch (idx) {
        case MARL_P_POS_W: return M(d.n_d, 2);
        case MARL_P_POS_B: case MARL_P_POS_LNW: case MARL_P_POS_LNB: return V(d.n_d);
        case MARL_P_ENC_W0: return M(d.nm2, d.n_b);
        case MARL_P_ENC_B0: case MARL_P_ENC_LN0W: case MARL_P_ENC_LN0B: return V(d.nm2);
        case MARL_P_ENC_W1: return M(d.n_m, d.nm2);
        case MARL_P_ENC_B1: case MARL_P_ENC_LN1W: case MARL_P_ENC_LN1B: return V(d.n_m);
        case MARL_P_DEC_W0: return M(d.nm2, d.n_m);
        case MARL_P_DEC_B0: case MARL_P_DEC_LN0W: case MARL_P_DEC_LN0B: return V(d.nm2);
        case MARL_P_DEC_W1: return M(d.n_mo, d.nm2);
        case MARL_P_DEC_B1: case MARL_P_DEC_LN1W: case MARL_P_DEC_LN1B: return V(d.n_mo);
        case MARL_P_LB_WIH: return M(4 * d.n_b, d.nin);
        case MARL_P_LB_WHH: return M(4 * d.n_b, d.n_b);
        case MARL_P_LB_BIH: case MARL_P_LB_BHH: return V(4 * d.n_b);
        case MARL_P_LA_WIH: return M(4 * d.n_a, d.nin);
        case MARL_P_LA_WHH: return M(4 * d.n_a, d.n_a);
        case MARL_P_LA_BIH: case MARL_P_LA_BHH: return V(4 * d.n_a);
        case MARL_P_POL_W0: return M(d.nla, d.n_a);
        case MARL_P_POL_B0: case MARL_P_POL_LNW: case MARL_P_POL_LNB: return V(d.nla);
        case MARL_P_POL_W1: return M(d.nA, d.nla);
        case MARL_P_POL_B1: return V(d.nA);
        case MARL_P_CRI_W0: return M(d.nla, d.n_a);
        case MARL_P_CRI_B0: case MARL_P_CRI_LNW: case MARL_P_CRI_LNB: return V(d.nla);
        case MARL_P_CRI_W1: return M(1, d.nla);
        case MARL_P_CRI_B1: return V(1);
        case MARL_P_PRE_W0: return M(d.nlb, d.n_b);
        case MARL_P_PRE_B0: case MARL_P_PRE_LNW: case MARL_P_PRE_LNB: return V(d.nlb);
        case MARL_P_PRE_W1: return M(d.nC, d.nlb);
        case MARL_P_PRE_B1: return V(d.nC);
        default: return ParamMeta{PK_NONE, 0, 0};
    }
}

// bump allocator over a workspace, in floats, 64-float (256 B) aligned
struct Bump {
    size_t off = 0;
    size_t take(size_t n) {
        const size_t o = off;
        off += (n + 63) & ~(size_t)63;
        return o;
    }
};

// weights workspace: packed (padded) copy, transposed copy, packed gradient per matrix
struct WLayout {
    size_t wp[MARL_NPARAMS];  // packed / tight copy
    int ldp[MARL_NPARAMS];
    size_t wt[MARL_NPARAMS];  // transposed copy [k, p4(n)]
    int ldt[MARL_NPARAMS];
    size_t gp[MARL_NPARAMS];  // packed gradient (same shape as wp)
    size_t wp3[MARL_NPARAMS], wt3[MARL_NPARAMS];  // bf16x3 images of wp / wt (gemm_split.hip)
    size_t wp3k[MARL_NPARAMS], wt3k[MARL_NPARAMS];  // k16 images of wp / wt (gemm3.hip, split.h), 0 = none
    size_t wf[MARL_NPARAMS];  // conv weights in MFMA-fragment order (cnn_fwd3), 0 = none
    // fragment-order copies of wp / wt for the panel kernels (panel_frag_index, common.h), 0 = none; gpf / gtf:
    // their 16-deep groups per tile
    size_t wpf[MARL_NPARAMS], wtf[MARL_NPARAMS];
    int gpf[MARL_NPARAMS], gtf[MARL_NPARAMS];
    size_t bsum_b, bsum_a;    // b_ih + b_hh
    size_t total;
};

// The image GEMMs (gemm3.hip) take over the large products when every step's row slice starts on an
// image row block (R % 32 == 0: all BASELINE shapes) and the cells' widths keep 16-byte accesses.
// (Layout-relevant: the workspaces grow by the images - marl_workspace_sizes after a knob change.)
// Measured: round 4 (128-row tile plans only) a gain from cells of >= 128 units on, the 64-unit MNIST shapes lost 4 %
// to the image writes; round 5, with the small-batch plans (gate-split LSTM launch, 64 x 64 NT tiles), the MNIST
// shapes gain too - C2 (B = 1024) 0.786 -> 0.755 ms, the same shapes at B = 32 0.614 -> 0.528 ms: on from 64 units
// (knob g3_min_units; the parity fixtures lower it further to run this path on the odd small shapes too).
// The MODEL-only part decides the weights workspace (its k16 weight images): that layout must not move
// with the batch - an epoch's last partial batch or an odd eval batch runs on the weights packed for the
// previous one.  The batch-dependent part only picks the kernels of a call.
static bool g3_model_ok(const Dims& d) {
    const int mu = tune_get("g3_min_units", 64);
    return split_mode() && tune_get("g3", 1) != 0 && (d.n_b & 3) == 0 && (d.n_a & 3) == 0 && d.n_b >= mu &&
           d.n_a >= mu;
}
static bool g3_enabled(const Dims& d) {
    return g3_model_ok(d) && d.R % 32 == 0 && d.R >= 32;
}
// conv weights whose tiles are whole (16 output channels x 16-deep K steps) get a fragment-order copy
static bool conv_frag_ok(const ParamMeta& m) { return m.kind == PK_CONV && m.n % 16 == 0 && m.k % 16 == 0; }

// The matrices the panel kernels stream (panel_gemm): forward from the packed copies, backward (the four message
// matrices) from the transposed ones.  Like g3_model_ok a property of the MODEL only - the weights workspace must not
// move with the batch, nor with the MARL_PANELS switch.
static bool panel_model_ok(const Dims& d) {
    return panel_supported(d.n_m, d.nm2, d.n_mo) && panel_supported(d.n_b, d.nm2, d.n_m) &&
           panel_supported(d.n_a, d.nla, 0);
}
static bool panel_frag_fwd(int i) {
    return i == MARL_P_ENC_W0 || i == MARL_P_ENC_W1 || i == MARL_P_DEC_W0 || i == MARL_P_DEC_W1 || i == MARL_P_POL_W0;
}
static bool panel_frag_bwd(int i) {
    return i == MARL_P_ENC_W0 || i == MARL_P_ENC_W1 || i == MARL_P_DEC_W0 || i == MARL_P_DEC_W1;
}

static void make_wlayout(const Dims& d, WLayout& w) {
    Bump b;
    for (int i = 0; i < MARL_NPARAMS; ++i) {
        const ParamMeta m = param_meta(d, i);
        w.wp[i] = w.wt[i] = w.gp[i] = w.wp3[i] = w.wt3[i] = w.wf[i] = w.wp3k[i] = w.wt3k[i] = 0;
        w.wpf[i] = w.wtf[i] = 0;
        w.ldp[i] = w.ldt[i] = w.gpf[i] = w.gtf[i] = 0;
        if (m.kind == PK_MATRIX || m.kind == PK_CONV) {
            w.ldp[i] = p4(m.k);
            w.wp[i] = b.take((size_t)m.n * w.ldp[i]);
            w.ldt[i] = p4(m.n);
            w.wt[i] = b.take((size_t)m.k * w.ldt[i]);
            w.gp[i] = b.take((size_t)m.n * w.ldp[i]);
            if (m.kind == PK_MATRIX) {
                w.wp3[i] = b.take(split_image_floats(m.n, m.k));
                w.wt3[i] = b.take(split_image_floats(m.k, m.n));
                if (g3_model_ok(d)) {
                    w.wp3k[i] = b.take(img_bytes(m.n, m.k) / sizeof(float));
                    w.wt3k[i] = b.take(img_bytes(m.k, m.n) / sizeof(float));
                }
            } else if (conv_frag_ok(m)) {
                b.take(16);  // (offset 0 means "none")
                w.wf[i] = b.take((size_t)m.n * m.k);
            }
        } else if (m.kind == PK_VEC) {
            w.ldp[i] = m.n;
            w.wp[i] = b.take((size_t)m.n);
        }
    }
    w.bsum_b = b.take((size_t)4 * d.n_b);
    w.bsum_a = b.take((size_t)4 * d.n_a);
    // (behind everything else: no earlier offset moves; the pack writes the real entries only, the padding and the
    // three groups of slack are the caller's zeros)
    if (panel_model_ok(d)) {
        for (int i = 0; i < MARL_NPARAMS; ++i) {
            const ParamMeta m = param_meta(d, i);
            if (m.kind != PK_MATRIX) continue;
            if (panel_frag_fwd(i)) {  // W [n, k]: tiles over n, contraction over k
                w.gpf[i] = panel_frag_groups(m.k);
                w.wpf[i] = b.take(panel_frag_floats(m.n, m.k));
            }
            if (panel_frag_bwd(i)) {  // W^T [k, n]: tiles over k, contraction over n
                w.gtf[i] = panel_frag_groups(m.n);
                w.wtf[i] = b.take(panel_frag_floats(m.k, m.n));
            }
        }
    }
    w.total = b.off;
}

// episode workspace
struct SBuf {  // per-step buffer: base offset + stride between steps (0 when shared)
    size_t off = 0, stride = 0;
    size_t at(int t) const { return off + stride * (size_t)t; }
};

struct ELayout {
    // all-steps state
    size_t POS;  // int32 [(Ns+1)][R][2]
    size_t H, C, HC, CC, MSG;  // [(Ns+1)][R][ld]
    size_t PROBS, ACT;         // [Ns][R][nA], int32 [Ns][R]
    // per step
    SBuf COLS[MARL_MAX_CNN_LAYERS], Z[MARL_MAX_CNN_LAYERS], GST[MARL_MAX_CNN_LAYERS],
        A[MARL_MAX_CNN_LAYERS];
    SBuf U, MBAR, ZD1, STD1, AD1, ZD2, STD2, NPOS, ZPOS, STPOS, GB, GA, ZE1, STE1, AE1, ZE2, STE2,
        ZP1, STP1, AP1;
    // batched heads
    size_t ZC1, STC1, AC1, ZQ1, STQ1, AQ1;
    // backward only
    size_t GPRED, DLOG, DVAL, DAQ1, DAC1, DAP1, DH, DHC, DC, DCC, DDBAR, DDBAR2, DAD1, DMBAR, DZE2, DAE1, DU,
        DZPOS, BTMP, PLN[4];
    size_t DZ[MARL_MAX_CNN_LAYERS], DCOLS[MARL_MAX_CNN_LAYERS], DA[MARL_MAX_CNN_LAYERS];
    size_t GB3, GA3;  // k16 images of the gate gradients [Ns*R, 4 n] (g3 only; float offsets)
    size_t U3, H3, HC3;  // images of U (train: every step, else one slice), H / H^ [(Ns+1) R]
    size_t u3_stride_rows;  // image rows between the U3 slices of consecutive steps (0: one shared slice)
    bool g3;
    // both weight gradients of the belief [0] / action [1] cell from one launch: planned where the scratch is sized
    GemmPlan tn_cell[2];
    size_t PART, TNS, LOSS;
    size_t RED, red_floats;  // scratch of the deferred-reduction queue (sum over every use)
    size_t part_floats, tns_bytes, loss_floats;
    size_t total;
    // what the fused CNN launchers do with this shape: the plans of their own routines (cnn.hip), which also decide
    // what is kept for backward
    CnnFwdPlan fwd;                            // which != 0: one launch for the whole extractor (plan of cnn_fwd_probe)
    CnnWgradPlan wgrad[MARL_MAX_CNN_LAYERS];   // form != 0: weight gradient from the activations (no im2col rows)
    CnnDgradPlan dgrad[MARL_MAX_CNN_LAYERS];   // rb != 0: fused transposed conv + GroupNorm backward (l >= 1)
    // forward keeps a layer's im2col rows only for a weight gradient the activation-based kernel does not cover
    bool keeps_cols[MARL_MAX_CNN_LAYERS];
};

// The arguments launch_cnn_fwd is planned with: the shapes, and which optional buffers exist - the im2col rows kept for
// backward (keeps_cols: they rule the cnn_fwd2 / cnn_fwd3 instantiations out) and the fragment-order weight copies
// (cnn_fwd3 needs them).  Only their presence matters to cnn_fwd_plan; cnn_fwd_args gives the launch the same pattern.
static CnnFwdArgs cnn_fwd_probe(const Dims& d, const WLayout& w, const bool* keeps_cols) {
    static float here;
    CnnFwdArgs a{};
    a.rows = d.R;
    a.nb = d.nb;
    a.c_img = d.c_img;
    a.H = d.H;
    a.W = d.W;
    a.f = d.f;
    a.L = d.L;
    for (int l = 0; l < d.L; ++l)
        a.layer[l] = CnnFwdLayer{nullptr, nullptr, nullptr, nullptr, keeps_cols[l] ? &here : nullptr, nullptr, nullptr,
                                 d.ch[l], d.ch[l + 1], d.grp[l], d.hw[l], d.hw[l + 1], d.P[l], d.K[l],
                                 d.ldk[l], w.wf[4 * l] ? &here : nullptr};
    return a;
}
static CnnWgradArgs cnn_wgrad_shape(const Dims& d, int l) {
    CnnWgradArgs g{};
    g.rows = d.NR;
    g.first = l == 0;
    g.nb = d.nb;
    g.c_img = d.c_img;
    g.H = d.H;
    g.W = d.W;
    g.cin = d.ch[l];
    g.cout = d.ch[l + 1];
    g.hin = d.hw[l];
    g.hout = d.hw[l + 1];
    g.P = d.P[l];
    g.G = l > 0 ? d.grp[l - 1] : 1;
    g.K = d.K[l];
    return g;
}
static CnnDgradArgs cnn_dgrad_shape(const Dims& d, int l) {
    CnnDgradArgs g{};
    g.rows = d.NR;
    g.cin = d.ch[l];
    g.cout = d.ch[l + 1];
    g.hin = d.hw[l];
    g.hout = d.hw[l + 1];
    g.P = d.P[l];
    g.Pin = d.P[l - 1];
    g.G = d.grp[l - 1];
    return g;
}

static CnnDimgArgs cnn_dimg_shape(const Dims& d) {
    CnnDimgArgs a{};
    a.ns = d.ns;
    a.na = d.na;
    a.nb = d.nb;
    a.c_img = d.c_img;
    a.H = d.H;
    a.W = d.W;
    a.cin = d.ch[0];
    a.cout = d.ch[1];
    a.f = d.f;
    a.hout = d.hw[1];
    a.P = d.P[0];
    return a;
}

static void make_elayout(const Dims& d, const WLayout& w, int train, ELayout& e) {
    Bump b;
    const size_t R = (size_t)d.R, NR = (size_t)d.NR, S1 = (size_t)d.ns + 1;
    e.POS = b.take(S1 * R * 2);
    e.H = b.take(S1 * R * d.ld_nb);
    e.C = b.take(S1 * R * d.ld_nb);
    e.HC = b.take(S1 * R * d.ld_na);
    e.CC = b.take(S1 * R * d.ld_na);
    e.MSG = b.take(S1 * R * d.ld_nm);
    e.PROBS = b.take(NR * d.nA);
    e.ACT = b.take(NR);
    const size_t steps = train ? (size_t)d.ns : 1;
    // per-step slices are packed back to back so that [Ns][rows][ld] is also [Ns*rows][ld]
    auto per = [&](SBuf& s, size_t n) {
        s.off = b.take(n * steps);
        s.stride = train ? n : 0;
    };
    auto once = [&](SBuf& s, size_t n) {  // one slice shared by every step (forward scratch)
        s.off = b.take(n);
        s.stride = 0;
    };
    for (int l = 0; l < MARL_MAX_CNN_LAYERS; ++l) {
        e.wgrad[l] = CnnWgradPlan{};
        e.dgrad[l] = CnnDgradPlan{};
        if (l < d.L) {
            CnnWgradArgs wg = cnn_wgrad_shape(d, l);
            e.wgrad[l] = cnn_wgrad_plan(wg);
        }
        if (l > 0 && l < d.L) {
            CnnDgradArgs dg = cnn_dgrad_shape(d, l);
            e.dgrad[l] = cnn_dgrad_plan(dg);
        }
        e.keeps_cols[l] = l < d.L && train != 0 && !e.wgrad[l].form;
    }
    {
        CnnFwdArgs probe = cnn_fwd_probe(d, w, e.keeps_cols);
        e.fwd = cnn_fwd_plan(probe);
    }
    const bool fused_fwd = e.fwd.which != 0;
    for (int l = 0; l < d.L; ++l) {
        // im2col rows: kept for every step only when the weight gradient needs them (shapes the
        // activation-based kernel does not cover); one scratch slice for the unfused forward
        if (e.keeps_cols[l])
            per(e.COLS[l], R * d.P[l] * d.ldk[l]);
        else if (!fused_fwd)
            once(e.COLS[l], R * d.P[l] * d.ldk[l]);
        per(e.Z[l], R * d.P[l] * d.ch[l + 1]);
        per(e.GST[l], R * d.grp[l] * 2);
        if (l + 1 < d.L && !fused_fwd) once(e.A[l], R * d.P[l] * d.ch[l + 1]);
    }
    per(e.U, R * d.ld_nin);
    per(e.MBAR, R * d.ld_nm);
    per(e.ZD1, R * d.ld_nm2);
    per(e.STD1, R * 2);
    per(e.AD1, R * d.ld_nm2);
    per(e.ZD2, R * d.ld_nmo);
    per(e.STD2, R * 2);
    per(e.NPOS, R * 4);
    per(e.ZPOS, R * d.ld_nd);
    per(e.STPOS, R * 2);
    per(e.GB, R * d.ld_gb);
    per(e.GA, R * d.ld_ga);
    per(e.ZE1, R * d.ld_nm2);
    per(e.STE1, R * 2);
    per(e.AE1, R * d.ld_nm2);
    per(e.ZE2, R * d.ld_nm);
    per(e.STE2, R * 2);
    per(e.ZP1, R * d.ld_nla);
    per(e.STP1, R * 2);
    per(e.AP1, R * d.ld_nla);
    e.ZC1 = b.take(NR * d.ld_nla);
    e.STC1 = b.take(NR * 2);
    e.AC1 = b.take(NR * d.ld_nla);
    e.ZQ1 = b.take(NR * d.ld_nlb);
    e.STQ1 = b.take(NR * 2);
    e.AQ1 = b.take(NR * d.ld_nlb);
    e.part_floats = e.tns_bytes = e.loss_floats = 0;
    e.g3 = g3_enabled(d);
    e.GB3 = e.GA3 = e.U3 = e.H3 = e.HC3 = 0;
    e.u3_stride_rows = 0;
    e.tn_cell[0] = e.tn_cell[1] = GemmPlan{};
    if (e.g3) {
        e.tn_cell[0] = g3_tn_cell_plan(4 * d.n_b, d.nin, d.n_b, d.NR);
        e.tn_cell[1] = g3_tn_cell_plan(4 * d.n_a, d.nin, d.n_a, d.NR);
        e.u3_stride_rows = train ? R : 0;
        e.U3 = b.take(img_bytes((int64_t)(train ? NR : R), d.nin) / sizeof(float));
        e.H3 = b.take(img_bytes((int64_t)(S1 * R), d.n_b) / sizeof(float));
        e.HC3 = b.take(img_bytes((int64_t)(S1 * R), d.n_a) / sizeof(float));
    }
    if (train && e.g3) {
        e.GB3 = b.take(img_bytes((int64_t)NR, 4 * d.n_b) / sizeof(float));
        e.GA3 = b.take(img_bytes((int64_t)NR, 4 * d.n_a) / sizeof(float));
    }
    if (train) {
        e.GPRED = b.take(NR * d.ld_nC);
        e.DLOG = b.take(NR * d.ld_nA);
        e.DVAL = b.take(NR * 4);
        e.DAQ1 = b.take(NR * d.ld_nlb);
        e.DAC1 = b.take(NR * d.ld_nla);
        e.DAP1 = b.take(NR * d.ld_nla);
        e.DH = b.take(S1 * R * d.ld_nb);
        e.DHC = b.take(S1 * R * d.ld_na);
        e.DC = b.take(R * d.ld_nb);
        e.DCC = b.take(R * d.ld_na);
        e.DDBAR = b.take(NR * d.ld_dbl);   // + the position-embedding columns of dU (belief cell)
        e.DDBAR2 = b.take(NR * d.ld_dbl);  // the action cell's share of the same columns
        e.DAD1 = b.take(NR * d.ld_nm2);
        e.DMBAR = b.take(R * d.ld_nm);
        e.DZE2 = b.take(NR * d.ld_nm);
        e.DAE1 = b.take(NR * d.ld_nm2);
        e.DU = b.take(NR * d.ld_nin);
        e.DZPOS = b.take(NR * d.ld_nd);
        int maxg = 4 * (d.n_b > d.n_a ? d.n_b : d.n_a);
        e.BTMP = b.take((size_t)maxg);
        {   // per-step LayerNorm affine partials of the panel backward kernels
            int blocks = panel_bwd_blocks((int)d.R);
            if (panel_chain_blocks(d.na, d.nb) > blocks) blocks = panel_chain_blocks(d.na, d.nb);
            const size_t nblk = (size_t)blocks * d.ns * 2;
            e.PLN[0] = b.take(nblk * d.n_mo);  // decode LN1
            e.PLN[1] = b.take(nblk * d.nm2);   // decode LN0
            e.PLN[2] = b.take(nblk * d.n_m);   // encode LN1
            e.PLN[3] = b.take(nblk * d.nm2);   // encode LN0
        }
        for (int l = 0; l < d.L; ++l) {
            e.DZ[l] = b.take(NR * d.P[l] * d.ch[l + 1]);
            // only the unfused layer backward materialises dCOLS_l and dA_{l-1}
            e.DCOLS[l] = (l > 0 && !e.dgrad[l].rb) ? b.take(NR * d.P[l] * d.ldk[l]) : 0;
            e.DA[l] = (l + 1 < d.L && !e.dgrad[l + 1].rb) ? b.take(NR * d.P[l] * d.ch[l + 1]) : 0;
        }
        // scratch sizes: maxima over every use
        size_t part = 0, tns = 0, red = 0;
        auto upd_part = [&](int64_t blocks, int n) {
            const size_t v = (size_t)blocks * 2 * n;
            part = v > part ? v : part;
            red += ((v + 63) & ~(size_t)63) + 64 * 2 * (size_t)n + 64;  // + stage-1 temporaries
        };
        auto upd_tn = [&](int ni, int nj, int64_t rows) {
            const size_t v = gemm_tn_scratch_bytes(ni, nj, rows);
            tns = v > tns ? v : tns;
            red += v / sizeof(float) + 64 * ((size_t)ni * nj + ni) + 192;
        };
        const int64_t nr = d.NR, r = d.R;
        upd_part(ln_bwd_blocks(nr, d.nlb), d.nlb);
        upd_part(ln_bwd_blocks(nr, d.nla), d.nla);
        upd_part(ln_bwd_blocks(nr, d.n_d), d.n_d);
        upd_part(ln_bwd_blocks(r, d.nm2), d.nm2);
        upd_part(ln_bwd_blocks(r, d.n_mo), d.n_mo);
        upd_part(ln_bwd_blocks(r, d.n_m), d.n_m);
        for (int l = 0; l < d.L; ++l) upd_part(gn_bwd_blocks(nr, d.ch[l + 1]), d.ch[l + 1]);
        for (int l = 1; l < d.L; ++l)  // fused layer backward: one partial row per workgroup
            if (e.dgrad[l].rb) upd_part(e.dgrad[l].chunks, d.ch[l]);
        upd_tn(d.nC, d.nlb, nr);
        upd_tn(d.nlb, d.n_b, nr);
        upd_tn(1, d.nla, nr);
        upd_tn(d.nla, d.n_a, nr);
        upd_tn(d.nA, d.nla, nr);
        upd_tn(d.n_mo, d.nm2, nr);
        upd_tn(d.nm2, d.n_m, nr);
        upd_tn(d.n_m, d.nm2, nr);
        upd_tn(d.nm2, d.n_b, nr);
        upd_tn(4 * d.n_b, d.nin, nr);
        upd_tn(4 * d.n_b, d.n_b, nr);
        upd_tn(4 * d.n_a, d.nin, nr);
        upd_tn(4 * d.n_a, d.n_a, nr);
        if (e.g3) {  // the same four products on images (gemm_tn3_kernel) have their own split plan
            const int tn3[4][2] = {{4 * d.n_b, d.nin}, {4 * d.n_b, d.n_b}, {4 * d.n_a, d.nin}, {4 * d.n_a, d.n_a}};
            for (const auto& q : tn3) {
                const size_t v = g3_tn_plan(q[0], q[1], nr, false).scratch_bytes;
                tns = v > tns ? v : tns;
            }
            // (both products of a cell in one launch: their slabs side by side; 0 bytes outside the plan)
            for (const GemmPlan& q : e.tn_cell) tns = q.scratch_bytes > tns ? q.scratch_bytes : tns;
        }
        upd_tn(d.n_d, 2, nr);
        for (int l = 0; l < d.L; ++l) {
            if (e.wgrad[l].form) {  // per-workgroup partial slabs of the activation-based kernel
                const size_t v = (size_t)e.wgrad[l].blocks_bound *
                                 ((size_t)d.ch[l + 1] * d.K[l] + d.ch[l + 1]) * sizeof(float);
                tns = v > tns ? v : tns;
                red += v / sizeof(float) + 64 * ((size_t)d.ch[l + 1] * (d.K[l] + 1)) + 192;
            } else {
                upd_tn(d.ch[l + 1], d.K[l], nr * d.P[l]);
            }
        }
        e.part_floats = part;
        e.tns_bytes = tns;
        e.PART = b.take(part);
        e.TNS = b.take(tns / sizeof(float) + 16);
        {   // stage-1 temporaries of the four per-step LayerNorm reductions (their parts are PLN)
            const int pn[4] = {d.n_mo, d.nm2, d.n_m, d.nm2};
            for (int n : pn) red += 64 * 2 * (size_t)n + 64;
        }
        e.red_floats = red + 4096;
        e.RED = b.take(e.red_floats);
    }
    e.loss_floats = loss_scratch_floats(d.ns, d.na, d.nb);
    e.LOSS = b.take(e.loss_floats);
    e.total = b.off;
}

// ---------------------------------------------------------------------------
// what the setters installed, and the plan of one call
// ---------------------------------------------------------------------------
// marl_policy_explore (marl_hip_explore.h): exploration controls of every sampling site and of the policy head's
// backward.  on = anything but (tau 1, eps 0, sampled): only then does a call take the EXPLORE kernels - with it off
// every entry launches what it always launched.
struct Explore {
    bool on;
    float inv_tau, keep, eps;  // 1 / tau, 1 - eps, eps (the floor eps / nA is formed where nA is known)
    int greedy;
};
// marl_class_loss (marl_hip_classloss.h): options of the vote error and the rewards of every loss entry.  on = anything
// was installed (neutral values too): only then does a loss entry take the option instances of the two kernels - with
// it off every entry launches what it always launched.
struct ClassLoss {
    bool on;
    const float* w;   // [nc] device, nullptr = all ones
    int nc;
    float eps;
    const float* sw;  // [ns] device, nullptr = all ones
    int ns;
    bool wrew;
};
// marl_soft_targets (marl_hip_softtargets.h): a target distribution per image in place of the label, in the vote error
// and the rewards of every loss entry.  q != nullptr: a loss entry takes the soft instances of the two kernels - with
// none installed every entry launches what it always launched.
struct SoftTargets {
    const float* q;  // [nb, nc] device, caller-owned
    int nb, nc;
};
// The process-global settings.  The six setters are the only writers of g_installed; an entry point copies it once
// (make_ctx into Ctx::opt, the entries without a context at their top) and everything below reads that copy.
struct Installed {
    // marl_comm_matrix: the caller-owned [na, na] mixing matrix of the message exchange (row = receiver), or null =
    // the mean over the other agents (which launch applies it: Plan::comm_form)
    const float* comm = nullptr;
    int comm_na = 0;
    // marl_comm_range: radius >= 0 = the matrix above is the BASE of a range-limited exchange - per image and step it
    // is gated by the agents' positions (CommGate, common.h).  The message emitted in step t (MSG[t + 1]) is aggregated
    // under the positions of its emission, POS[t]; the zero message of step 0 under POS[0].
    CommGate range = {nullptr, -1, 0, 1};
    Explore explore = {false, 1.f, 1.f, 0.f, 0};
    ClassLoss class_loss = {false, nullptr, 0, 0.f, nullptr, 0, false};
    SoftTargets soft = {nullptr, 0, 0};
    hipEvent_t heads_event = nullptr;  // marl_backward_heads_event: recorded once the heads' gradients are final
};
static Installed g_installed;

// where sample(t) of the forward loop runs: a sample_kernel launch of its own behind the step's other launches, the
// epilogue of the chain launch's policy workgroups, or extra workgroups of the unchained decoder(t+1) launch
enum SampleSite { SAMPLE_OWN = 0, SAMPLE_EPILOGUE, SAMPLE_RIDE };
// Which kernel family every launch site of a call takes.  make_plan is the only place that decides it: the forward
// and backward drivers branch on Ctx::plan, marl_plan_query reports the same object.
struct Plan {
    bool panels;        // forward: the MLPs run as panel launches (else GEMM + LayerNorm rows)
    bool panels_bwd;    // backward loop: the same, for the narrower range of its kernels (every message width <= 384)
    bool chain;         // the chained panel launches, forward and backward (all agents of an image in one workgroup)
    bool panel_sample;  // ... whose policy workgroups sample as their epilogue
    bool panel_static;  // ... and which take the static-shape panel kernels, forward and backward (README widths, plain)
    bool g3_lstm;       // both cells and the heads' first layers from k16 images (gemm3.hip)
    bool g3_tn, g3_tn_pipe;  // the four large weight gradients from images; ... phase-pipelined
    bool g3_tn_cell;         // ... and both cells take the one-launch-per-cell form (ELayout::tn_cell)
    bool u3_by_producers;    // the kernels that write U also write its image (no separate pass)
    int skip_f32;       // every consumer of the gate gradients reads their images: no fp32 copy at all
    int lstm_plan;      // tile plan of the two-cell LSTM launch (gemm3.hip: 2 = 128-row tiles, 3 / 4 = the 32- / 64-row
                        // gate-split plans, 1 / 5 / 6 by knob; 0 = not on images)
    SampleSite sample;  // (SAMPLE_RIDE: but for the last step, which has no decoder(t+1) launch)
    // The aggregation of the messages: 0 = mean inside the chained panel launch, 1 = mean while a panel stages, 2 =
    // agg_msg_kernel; under a matrix 5 = mixed inside the chained launch (the MIX / GATE instantiations of
    // panel_fwd_kernel / panel_bwd_kernel; the decoder of step 0 and the step API then take form 3), 3 / 4 =
    // mix_msg[_gated]_kernel (rowops.hip) in a launch of its own ahead of a plain panel launch / the GEMM path
    int comm_form;
    int explore_form;   // sampling under the controls: 0 = off, 1 = the chain launch's EXPLORE epilogue, 2 = sample_kernel's
    int comm, comm_range, explore, class_loss;  // what is installed: matrix set, its radius or -1, controls / options on
    int soft_targets;                           // ... and a target distribution per image (marl_soft_targets)
};

// ---------------------------------------------------------------------------
// context shared by the forward / backward drivers
// ---------------------------------------------------------------------------
struct Ctx {
    Dims d;
    WLayout w;
    ELayout e;
    float* W;  // weights workspace
    float* E;  // episode workspace
    hipStream_t st;
    int train;
    RedQueue* rq = nullptr;  // backward: deferred reductions (null: every reduction launches at once)
    TnQueue* tq = nullptr;   // backward: small weight gradients collected for one launch (needs rq)
    bool defer_slabs = false;  // also the split-K / conv weight-gradient slabs (tens of MB each)
    size_t defer_small = 0;    // ... or only those of at most this many bytes (they stay in the L2)
    bool defer_this(size_t slab_bytes) const { return defer_slabs || (defer_small && slab_bytes <= defer_small); }
    Installed opt;  // the settings of this call: g_installed as make_ctx found it
    Plan plan;      // make_plan(d, w, e, opt)
    int u3_row(int t) const { return (int)(e.u3_stride_rows * (size_t)t); }

    const char* wp3k(int i) const { return reinterpret_cast<const char*>(W + w.wp3k[i]); }
    const char* wt3k(int i) const { return reinterpret_cast<const char*>(W + w.wt3k[i]); }
    char* img(size_t off) const { return reinterpret_cast<char*>(E + off); }
    const float* wp(int i) const { return W + w.wp[i]; }
    const float* wt(int i) const { return W + w.wt[i]; }
    // the packed [n, k] / transposed [k, n] copy of matrix i as the B operand of a product, with the image
    // marl_pack_weights wrote next to it (a conv weight has none)
    GemmB wpB(int i) const {
        const ParamMeta m = param_meta(d, i);
        return GemmB{wp(i), w.ldp[i], m.k, m.kind == PK_MATRIX ? W + w.wp3[i] : nullptr, (m.k + 31) / 32};
    }
    GemmB wtB(int i) const {
        const ParamMeta m = param_meta(d, i);
        return GemmB{wt(i), w.ldt[i], m.n, m.kind == PK_MATRIX ? W + w.wt3[i] : nullptr, (m.n + 31) / 32};
    }
    // fragment-order copies for the panel kernels (null: this model has none - the launchers refuse)
    const float* wpf(int i) const { return w.wpf[i] ? W + w.wpf[i] : nullptr; }
    const float* wtf(int i) const { return w.wtf[i] ? W + w.wtf[i] : nullptr; }
    float* gp(int i) const { return W + w.gp[i]; }
    float* at(size_t off) const { return E + off; }
    float* at(const SBuf& s, int t) const { return E + s.at(train ? t : 0); }
    // all-steps buffers, slice t
    float* Hs(int t) const { return E + e.H + (size_t)t * d.R * d.ld_nb; }
    float* Cs(int t) const { return E + e.C + (size_t)t * d.R * d.ld_nb; }
    float* HCs(int t) const { return E + e.HC + (size_t)t * d.R * d.ld_na; }
    float* CCs(int t) const { return E + e.CC + (size_t)t * d.R * d.ld_na; }
    float* MSGs(int t) const { return E + e.MSG + (size_t)t * d.R * d.ld_nm; }
    int32_t* POSs(int t) const { return reinterpret_cast<int32_t*>(E + e.POS) + (size_t)t * d.R * 2; }
    float* PROBSs(int t) const { return E + e.PROBS + (size_t)t * d.R * d.nA; }
    int32_t* ACTs(int t) const { return reinterpret_cast<int32_t*>(E + e.ACT) + (size_t)t * d.R; }
    float* DHs(int t) const { return E + e.DH + (size_t)t * d.R * d.ld_nb; }
    float* DHCs(int t) const { return E + e.DHC + (size_t)t * d.R * d.ld_na; }
};

static Plan make_plan(const Dims& d, const WLayout& w, const ELayout& e, const Installed& opt) {
    auto env_on = [](const char* v) { return !(v && v[0] == '0'); };
    // MARL_PANEL_SAMPLE=0: chain launch, then sample_kernel - the earlier form, kept for comparison in one binary
    static const bool env_panels = env_on(getenv("MARL_PANELS")), env_sample = env_on(getenv("MARL_PANEL_SAMPLE"));
    Plan p{};
    p.panels = env_panels && panel_model_ok(d);
    p.panels_bwd = p.panels && d.n_mo <= 384 && d.nm2 <= 384 && d.n_m <= 384;
    // chain: all agents of a batch element in one workgroup (rows a * nb + b for every a), so that the message mean
    // over the other agents needs no second launch (fwd_step_chain, bwd_step_chain).  Under a matrix the chained
    // kernels also keep it in LDS (16 x 16 floats): with the input width bounded like the others every admitted plan
    // has room for it; wider models take mix_msg_kernel.
    p.chain = p.panels_bwd && panel_chain_supported(d.na, d.n_m, 256) && tune_get("panel_chain", 1) != 0 &&
              (!opt.comm || d.n_b <= 384);
    p.panel_sample = p.chain && env_sample && panel_sample_supported(d.nA);
    // the static-shape panel kernels: plain chain launches only (launch_panel_fwd / launch_panel_bwd match each launch)
    p.panel_static = p.chain && !opt.comm && !opt.explore.on &&
                     panel_static_model(d.n_b, d.n_a, d.nm2, d.n_m, d.n_mo, d.nla, d.nA, d.n_d);
    // sample(t) and decoder(t+1) are independent: without the chain one launch runs both - but not under exploration
    // controls (the ride-along workgroups of the plain decoder launch have no EXPLORE form)
    p.sample = p.chain ? (p.panel_sample ? SAMPLE_EPILOGUE : SAMPLE_OWN)
                       : (p.panels && !opt.explore.on ? SAMPLE_RIDE : SAMPLE_OWN);
    p.comm_form = opt.comm ? (p.chain ? 5 : p.panels ? 3 : 4) : p.chain ? 0 : p.panels ? 1 : 2;
    p.explore_form = !opt.explore.on ? 0 : p.panel_sample ? 1 : 2;
    p.comm = opt.comm != nullptr;
    p.comm_range = opt.range.radius >= 0 ? opt.range.radius : -1;
    p.explore = opt.explore.on;
    p.class_loss = opt.class_loss.on;
    p.soft_targets = opt.soft.q != nullptr;

    const int k_lstm = tune_get("g3_lstm", 1), k_tn = tune_get("g3_tn", 1);
    p.g3_lstm = e.g3 && k_lstm != 0;
    if (p.g3_lstm) {  // the launcher's own rule with the shapes of the launch
        G3Batch b{};
        b.count = 2;
        b.p[0].m = b.p[1].m = (int)d.R;
        b.p[0].n = d.n_b;
        b.p[1].n = d.n_a;
        p.lstm_plan = g3_lstm_plan(b).variant;
    }
    // the four large weight gradients on images (gemm_tn3_kernel: 256-column tiles of A, whole 256 x 256 tiles
    // or column passes, g3_tn_plan): only where that form wins - >= 32768 contraction rows (at C4's 8192 rows the
    // fp32-operand kernel is 25 % faster) and at most three column passes on the B side
    // (round 5: the one-launch-per-cell form wins from 8 192 rows on - C4 at 32 images per GPU: 3.62 vs 3.69 ms)
    p.g3_tn = p.g3_lstm && k_tn != 0 &&
              (k_tn == 2 || (d.nin <= 640 && d.n_b <= 512 && d.n_a <= 512 &&
                             (d.NR >= 32768 || (e.tn_cell[0].ok && e.tn_cell[1].ok))));
    p.g3_tn_cell = p.g3_tn && e.tn_cell[0].ok && e.tn_cell[1].ok;
    p.g3_tn_pipe = p.g3_tn && e.tn_cell[0].pipelined;  // (knob g3_tn_pipe: g3_tn_cell_plan carries it even when !ok)
    p.skip_f32 = p.panels_bwd && p.g3_tn;
    // the three kernels that write U[t] (fused CNN: features; decoder panel: message columns; sampling
    // launch: position embedding) also write its image when all of them are on the path and the column
    // ranges keep 8-byte image pieces whole; else (and for step 0, whose embedding comes from the
    // stand-alone kernel) one image pass over U[t] runs ahead of the LSTM launch
    p.u3_by_producers = p.g3_lstm && e.fwd.writes_image && p.panels &&
                        ((d.nf | d.n_mo | d.n_d) & 3) == 0 &&
                        // (the producers write exactly nin columns: a K pad of the last 16-deep step would be
                        // whatever the workspace held - only the stand-alone image pass zeroes it)
                        d.nin % 16 == 0;
    return p;
}

static int make_ctx(const marl_config* cfg, const void* wws, size_t wbytes, void* ews, size_t ebytes,
                    int train, void* stream, Ctx& c) {
    MARL_TRY(make_dims(cfg, c.d));
    c.opt = g_installed;
    if (c.opt.comm && c.opt.comm_na != c.d.na) {  // (before anything is enqueued)
        set_error("communication matrix is %d x %d but the configuration has %d agents", c.opt.comm_na,
                  c.opt.comm_na, c.d.na);
        return MARL_EINVAL;
    }
    if (c.opt.range.radius >= 0 && !c.opt.comm) {
        set_error("a communication range is installed without its base matrix (marl_comm_matrix)");
        return MARL_EINVAL;
    }
    make_wlayout(c.d, c.w);
    make_elayout(c.d, c.w, train, c.e);
    if (wbytes < c.w.total * sizeof(float) || ebytes < c.e.total * sizeof(float)) {
        set_error("workspace too small for the current configuration / tuning knobs: weights %zu of %zu "
                  "bytes, episode %zu of %zu bytes (ask marl_workspace_sizes again)", wbytes,
                  c.w.total * sizeof(float), ebytes, c.e.total * sizeof(float));
        return MARL_ESIZE;
    }
    c.W = const_cast<float*>(static_cast<const float*>(wws));
    c.E = static_cast<float*>(ews);
    c.st = static_cast<hipStream_t>(stream);
    c.train = train;
    if (!c.W || !c.E) {
        set_error("null workspace");
        return MARL_EINVAL;
    }
    if ((reinterpret_cast<uintptr_t>(c.W) & 255) || (reinterpret_cast<uintptr_t>(c.E) & 255)) {
        set_error("workspaces must be 256-byte aligned");
        return MARL_EINVAL;
    }
    c.plan = make_plan(c.d, c.w, c.e, c.opt);
    return MARL_OK;
}

static int gemm1(const Ctx& c, const GemmProb& p) {
    GemmBatch b{};
    b.p[0] = p;
    b.count = 1;
    return launch_gemm_nt(b, c.st);
}
static int gemm2(const Ctx& c, const GemmProb& p0, const GemmProb& p1) {
    GemmBatch b{};
    b.p[0] = p0;
    b.p[1] = p1;
    b.count = 2;
    return launch_gemm_nt(b, c.st);
}

// ---------------------------------------------------------------------------
// one step of the network up to (not including) the policy output layer
// ---------------------------------------------------------------------------
struct StepIn {
    const float* obs = nullptr;       // standalone API: pre-gathered patches
    const float* npos = nullptr;      // standalone API: normalised positions
    const void* img = nullptr;
    int img_u8 = 0;
};

// What one launch of the fused extractor forward reads and writes.  step_cnn fills it from the episode workspace,
// marl_cnn_fwd (include/marl_hip_cnnops.h) from its caller's buffers; cnn_fwd_args is the only place that turns it
// into the kernels' arguments.
struct CnnFwdIo {
    const void* img = nullptr;
    const float* obs = nullptr;
    const int32_t* pos = nullptr;
    int img_u8 = 0;
    int64_t rows = 0;
    float* cols[MARL_MAX_CNN_LAYERS] = {};  // null: not kept
    float* z[MARL_MAX_CNN_LAYERS] = {};
    float* gst[MARL_MAX_CNN_LAYERS] = {};
    float* u = nullptr;
    int ldu = 0;
    char* u3 = nullptr;
    int u3_row0 = 0, u3_steps = 0;
};
static CnnFwdArgs cnn_fwd_args(const Dims& d, const WLayout& w, const float* W, const CnnFwdIo& io) {
    CnnFwdArgs a{};
    a.img = io.img;
    a.obs = io.obs;
    a.pos = io.pos;
    a.img_u8 = io.img_u8;
    a.rows = io.rows;
    a.nb = d.nb;
    a.c_img = d.c_img;
    a.H = d.H;
    a.W = d.W;
    a.f = d.f;
    a.L = d.L;
    for (int l = 0; l < d.L; ++l)
        a.layer[l] = CnnFwdLayer{W + w.wp[4 * l], W + w.wp[4 * l + 1], W + w.wp[4 * l + 2], W + w.wp[4 * l + 3],
                                 io.cols[l], io.z[l], io.gst[l],
                                 d.ch[l], d.ch[l + 1], d.grp[l], d.hw[l], d.hw[l + 1], d.P[l],
                                 d.K[l], d.ldk[l], w.wf[4 * l] ? W + w.wf[4 * l] : nullptr};
    a.u = io.u;
    a.ldu = io.ldu;
    a.u3 = io.u3;
    a.u3_row0 = io.u3_row0;
    a.u3_steps = io.u3_steps;
    return a;
}

// ---- the five phases of one step; each only depends on what the comment names -----------

// observation -> CNN features b_t -> U[t][:, :nf]            (needs POS[t])
static int step_cnn(const Ctx& c, int t, const StepIn& in) {
    const Dims& d = c.d;
    hipStream_t st = c.st;
    if (c.e.fwd.which) {
        // one fused launch for the whole extractor when the shapes allow it
        CnnFwdIo io;
        io.img = in.img;
        io.obs = in.obs;
        io.pos = c.POSs(t);
        io.img_u8 = in.img_u8;
        io.rows = d.R;
        for (int l = 0; l < d.L; ++l) {
            io.cols[l] = c.e.keeps_cols[l] ? c.at(c.e.COLS[l], t) : nullptr;
            io.z[l] = c.train ? c.at(c.e.Z[l], t) : nullptr;
            io.gst[l] = c.train ? c.at(c.e.GST[l], t) : nullptr;
        }
        io.u = c.at(c.e.U, t);
        io.ldu = d.ld_nin;
        if (c.plan.u3_by_producers) {
            io.u3 = c.img(c.e.U3);
            io.u3_row0 = c.u3_row(t);
            io.u3_steps = img_steps(d.nin);
        }
        CnnFwdArgs a = cnn_fwd_args(d, c.w, c.W, io);
        return launch_cnn_fwd(a, st);
    }
    if (in.obs)
        MARL_TRY(launch_obs_im2col(in.obs, c.at(c.e.COLS[0], t), d.ldk[0], d.R, d.c_img, d.ch[0],
                                   d.f, st));
    else
        MARL_TRY(launch_gather_im2col(in.img, in.img_u8, c.POSs(t), c.at(c.e.COLS[0], t), d.ldk[0],
                                      d.na, d.nb, d.c_img, d.ch[0], d.H, d.W, d.f, st));
    for (int l = 0; l < d.L; ++l) {
        const int co = d.ch[l + 1];
        const int64_t rows = d.R * d.P[l];
        MARL_TRY(gemm1(c, gemm_prob(c.at(c.e.COLS[l], t), d.ldk[l], c.wpB(4 * l),
                                    c.at(c.e.Z[l], t), co, (int)rows, co, c.wp(4 * l + 1))));
        if (l + 1 < d.L && gn_fwd_im2col_supported(d.P[l], co)) {
            // GroupNorm + SiLU + the next layer's im2col in one pass (A_l is never materialised)
            MARL_TRY(launch_gn_silu_fwd(c.at(c.e.Z[l], t), c.wp(4 * l + 2), c.wp(4 * l + 3), nullptr,
                                        0, 0, c.at(c.e.GST[l], t), d.R, d.P[l], co, d.grp[l], st,
                                        c.at(c.e.COLS[l + 1], t), d.ldk[l + 1], d.hw[l + 1]));
        } else if (l + 1 < d.L) {
            MARL_TRY(launch_gn_silu_fwd(c.at(c.e.Z[l], t), c.wp(4 * l + 2), c.wp(4 * l + 3),
                                        c.at(c.e.A[l], t), (int64_t)d.P[l] * co, 0,
                                        c.at(c.e.GST[l], t), d.R, d.P[l], co, d.grp[l], st));
            MARL_TRY(launch_im2col(c.at(c.e.A[l], t), c.at(c.e.COLS[l + 1], t), d.ldk[l + 1], d.R,
                                   d.hw[l + 1], co, st));
        } else {
            MARL_TRY(launch_gn_silu_fwd(c.at(c.e.Z[l], t), c.wp(4 * l + 2), c.wp(4 * l + 3),
                                        c.at(c.e.U, t), d.ld_nin, 1, c.at(c.e.GST[l], t), d.R,
                                        d.P[l], co, d.grp[l], st));
        }
    }
    return MARL_OK;
}

// the gate under which MSG[t] is aggregated (pos null: no range installed): the positions of its emission step
static CommGate comm_gate(const Ctx& c, int t) {
    CommGate g = c.opt.range;
    g.pos = g.radius >= 0 ? c.POSs(t > 0 ? t - 1 : 0) : nullptr;
    return g;
}
// the exchange of MSG[t] (or, transpose, of its gradient) under the installed matrix, in a launch of its own
static int mix_msg(const Ctx& c, int t, const float* m, float* out, int n, int transpose) {
    const Dims& d = c.d;
    if (c.opt.range.radius >= 0)
        return launch_mix_msg_gated(m, out, d.ld_nm, d.na, d.nb, n, c.opt.comm, comm_gate(c, t), transpose, c.st);
    return launch_mix_msg(m, out, d.ld_nm, d.na, d.nb, n, c.opt.comm, transpose, c.st);
}

// the decoder's two layers of step t (outputs: AD1[t], U[t][:, nf:nf+n_mo])
static void fill_dec_layers(const Ctx& c, int t, PanelLayer* layer) {
    const Dims& d = c.d;
    const bool keep = c.train != 0;
    layer[0] = PanelLayer{c.wpf(MARL_P_DEC_W0), c.w.gpf[MARL_P_DEC_W0], c.wp(MARL_P_DEC_B0),
                          c.wp(MARL_P_DEC_LN0W), c.wp(MARL_P_DEC_LN0B), d.nm2,
                          keep ? c.at(c.e.ZD1, t) : nullptr, d.ld_nm2,
                          keep ? c.at(c.e.STD1, t) : nullptr, c.at(c.e.AD1, t), d.ld_nm2};
    layer[1] = PanelLayer{c.wpf(MARL_P_DEC_W1), c.w.gpf[MARL_P_DEC_W1], c.wp(MARL_P_DEC_B1),
                          c.wp(MARL_P_DEC_LN1W), c.wp(MARL_P_DEC_LN1B), d.n_mo,
                          keep ? c.at(c.e.ZD2, t) : nullptr, d.ld_nmo,
                          keep ? c.at(c.e.STD2, t) : nullptr, c.at(c.e.U, t) + d.nf, d.ld_nin};
    if (c.plan.u3_by_producers) {
        layer[1].a3 = c.img(c.e.U3);
        layer[1].a3_row0 = c.u3_row(t);
        layer[1].a3_steps = img_steps(d.nin);
        layer[1].a3_col0 = d.nf;
    }
}

// message mean over the other agents + decoder -> U[t][:, nf:nf+n_mo]   (needs MSG[t])
// `sample` (panel path only, SAMPLE_RIDE): the sampling rows of the PREVIOUS step ride along in the same launch
static int step_decode(const Ctx& c, int t, const SampleArgs* sample = nullptr) {
    const Dims& d = c.d;
    const int R = (int)d.R;
    hipStream_t st = c.st;
    if (c.plan.panels) {
        PanelFwdBatch pb{};
        pb.count = 1;
        PanelFwdProb& p = pb.p[0];
        p.x = c.MSGs(t);
        p.ldx = d.ld_nm;
        p.k0 = d.n_m;
        p.agg_na = d.na;
        p.agg_nb = d.nb;
        p.xbar = c.at(c.e.MBAR, t);
        if (c.opt.comm) {  // mixed rows (pad columns included: the panel stages whole float4s) -> MBAR, staged as they are
            MARL_TRY(mix_msg(c, t, c.MSGs(t), c.at(c.e.MBAR, t), d.ld_nm, 0));
            p.x = c.at(c.e.MBAR, t);
            p.agg_na = p.agg_nb = 0;
            p.xbar = nullptr;
        }
        p.m = R;
        p.nlayers = 2;
        fill_dec_layers(c, t, p.layer);
        if (sample) {
            pb.has_sample = 1;
            pb.sample = *sample;
        }
        return launch_panel_fwd(pb, st);
    }
    if (c.opt.comm)
        MARL_TRY(mix_msg(c, t, c.MSGs(t), c.at(c.e.MBAR, t), d.n_m, 0));
    else
        MARL_TRY(launch_agg_msg(c.MSGs(t), c.at(c.e.MBAR, t), d.ld_nm, d.na, d.nb, d.n_m, st));
    MARL_TRY(gemm1(c, gemm_prob(c.at(c.e.MBAR, t), d.ld_nm, c.wpB(MARL_P_DEC_W0),
                                c.at(c.e.ZD1, t), d.ld_nm2, R, d.nm2, c.wp(MARL_P_DEC_B0))));
    MARL_TRY(launch_ln_silu_fwd(c.at(c.e.ZD1, t), d.ld_nm2, c.wp(MARL_P_DEC_LN0W),
                                c.wp(MARL_P_DEC_LN0B), c.at(c.e.AD1, t), d.ld_nm2,
                                c.at(c.e.STD1, t), d.R, d.nm2, st));
    MARL_TRY(gemm1(c, gemm_prob(c.at(c.e.AD1, t), d.ld_nm2, c.wpB(MARL_P_DEC_W1),
                                c.at(c.e.ZD2, t), d.ld_nmo, R, d.n_mo, c.wp(MARL_P_DEC_B1))));
    return launch_ln_silu_fwd(c.at(c.e.ZD2, t), d.ld_nmo, c.wp(MARL_P_DEC_LN1W),
                              c.wp(MARL_P_DEC_LN1B), c.at(c.e.U, t) + d.nf, d.ld_nin,
                              c.at(c.e.STD2, t), d.R, d.n_mo, st);
}

// position embedding + both LSTM cells -> H/C/H^/C^[t+1]     (needs all of U[t])
static int step_pos_lstm(const Ctx& c, int t, const StepIn& in, bool pos_done = false) {
    const Dims& d = c.d;
    const int R = (int)d.R;
    hipStream_t st = c.st;
    if (!pos_done)
    MARL_TRY(launch_pos_embed_fwd(c.POSs(t), in.npos, d.H, d.W, c.wp(MARL_P_POS_W),
                                  c.wp(MARL_P_POS_B), c.wp(MARL_P_POS_LNW), c.wp(MARL_P_POS_LNB),
                                  c.at(c.e.NPOS, t), c.at(c.e.ZPOS, t), d.ld_nd, c.at(c.e.STPOS, t),
                                  c.at(c.e.U, t) + d.nf + d.n_mo, d.ld_nin, d.R, d.n_d, st));
    if (c.plan.g3_lstm) {
        // image form: U[t] is complete here -> its k16 image (until its three producers write it
        // themselves), then both cells from images; the epilogue writes the images of h' / h^'
        const int u_row0 = c.u3_row(t);
        if (!c.plan.u3_by_producers || t == 0 || in.obs) {
            ImgBatch ib{};
            ib.d[0] = ImgDesc{c.at(c.e.U, t), c.img(c.e.U3) + img_off(u_row0, 0, img_steps(d.nin)), d.R, d.nin, d.ld_nin};
            ib.count = 1;
            MARL_TRY(launch_images(ib, st));
        }
        const int r0 = (int)((int64_t)t * d.R), r1 = r0 + R;
        G3Batch g{};
        g.count = 2;
        G3Prob& qb = g.p[0];
        qb = g3_prob(c.img(c.e.U3), u_row0, c.wp3k(MARL_P_LB_WIH), 0, d.nin, nullptr, 0, R, d.n_b, c.W + c.w.bsum_b);
        g3_add_seg(qb, c.img(c.e.H3), r0, c.wp3k(MARL_P_LB_WHH), 0, d.n_b);
        qb.c_prev = c.Cs(t);
        qb.h_next = c.Hs(t + 1);
        qb.c_next = c.Cs(t + 1);
        qb.gates = c.train ? c.at(c.e.GB, t) : nullptr;
        qb.ld_state = d.ld_nb;
        qb.ld_gates = d.ld_gb;
        qb.h3 = c.img(c.e.H3);
        qb.h3_row0 = r1;
        qb.h3_steps = img_steps(d.n_b);
        G3Prob& qa = g.p[1];
        qa = g3_prob(c.img(c.e.U3), u_row0, c.wp3k(MARL_P_LA_WIH), 0, d.nin, nullptr, 0, R, d.n_a, c.W + c.w.bsum_a);
        g3_add_seg(qa, c.img(c.e.HC3), r0, c.wp3k(MARL_P_LA_WHH), 0, d.n_a);
        qa.c_prev = c.CCs(t);
        qa.h_next = c.HCs(t + 1);
        qa.c_next = c.CCs(t + 1);
        qa.gates = c.train ? c.at(c.e.GA, t) : nullptr;
        qa.ld_state = d.ld_na;
        qa.ld_gates = d.ld_ga;
        qa.h3 = c.img(c.e.HC3);
        qa.h3_row0 = r1;
        qa.h3_steps = img_steps(d.n_a);
        return launch_gemm_lstm3(g, st);
    }
    GemmBatch b{};
    b.count = 2;
    GemmProb& pb = b.p[0];
    pb = gemm_prob(c.at(c.e.U, t), d.ld_nin, c.wpB(MARL_P_LB_WIH), nullptr, 0, R, d.n_b, c.W + c.w.bsum_b);
    gemm_add_seg(pb, c.Hs(t), d.ld_nb, c.wpB(MARL_P_LB_WHH));
    pb.c_prev = c.Cs(t);
    pb.h_next = c.Hs(t + 1);
    pb.c_next = c.Cs(t + 1);
    pb.gates = c.train ? c.at(c.e.GB, t) : nullptr;
    pb.ld_state = d.ld_nb;
    pb.ld_gates = d.ld_gb;
    GemmProb& pa = b.p[1];
    pa = gemm_prob(c.at(c.e.U, t), d.ld_nin, c.wpB(MARL_P_LA_WIH), nullptr, 0, R, d.n_a, c.W + c.w.bsum_a);
    gemm_add_seg(pa, c.HCs(t), d.ld_na, c.wpB(MARL_P_LA_WHH));
    pa.c_prev = c.CCs(t);
    pa.h_next = c.HCs(t + 1);
    pa.c_next = c.CCs(t + 1);
    pa.gates = c.train ? c.at(c.e.GA, t) : nullptr;
    pa.ld_state = d.ld_na;
    pa.ld_gates = d.ld_ga;
    return launch_gemm_lstm(b, st);
}

static void fill_enc_prob(const Ctx& c, int t, PanelFwdProb& pe) {
    const Dims& d = c.d;
    const bool keep = c.train != 0;
    pe.x = c.Hs(t + 1);
    pe.ldx = d.ld_nb;
    pe.k0 = d.n_b;
    pe.m = (int)d.R;
    pe.nlayers = 2;
    pe.layer[0] = PanelLayer{c.wpf(MARL_P_ENC_W0), c.w.gpf[MARL_P_ENC_W0], c.wp(MARL_P_ENC_B0),
                             c.wp(MARL_P_ENC_LN0W), c.wp(MARL_P_ENC_LN0B), d.nm2,
                             keep ? c.at(c.e.ZE1, t) : nullptr, d.ld_nm2,
                             keep ? c.at(c.e.STE1, t) : nullptr, c.at(c.e.AE1, t), d.ld_nm2};
    pe.layer[1] = PanelLayer{c.wpf(MARL_P_ENC_W1), c.w.gpf[MARL_P_ENC_W1], c.wp(MARL_P_ENC_B1),
                             c.wp(MARL_P_ENC_LN1W), c.wp(MARL_P_ENC_LN1B), d.n_m,
                             keep ? c.at(c.e.ZE2, t) : nullptr, d.ld_nm,
                             keep ? c.at(c.e.STE2, t) : nullptr, c.MSGs(t + 1), d.ld_nm};
}
static void fill_pol_prob(const Ctx& c, int t, PanelFwdProb& pp) {
    const Dims& d = c.d;
    const bool keep = c.train != 0;
    pp.x = c.HCs(t + 1);
    pp.ldx = d.ld_na;
    pp.k0 = d.n_a;
    pp.m = (int)d.R;
    pp.nlayers = 1;
    pp.layer[0] = PanelLayer{c.wpf(MARL_P_POL_W0), c.w.gpf[MARL_P_POL_W0], c.wp(MARL_P_POL_B0),
                             c.wp(MARL_P_POL_LNW), c.wp(MARL_P_POL_LNB), d.nla,
                             keep ? c.at(c.e.ZP1, t) : nullptr, d.ld_nla,
                             keep ? c.at(c.e.STP1, t) : nullptr, c.at(c.e.AP1, t), d.ld_nla};
}

// message encoder -> MSG[t+1] and policy hidden layer -> AP1[t]  (needs H / H^[t+1])
static int step_encode_policy(const Ctx& c, int t) {
    const Dims& d = c.d;
    const int R = (int)d.R;
    hipStream_t st = c.st;
    if (c.plan.panels) {
        PanelFwdBatch pb{};
        pb.count = 2;
        fill_enc_prob(c, t, pb.p[0]);
        fill_pol_prob(c, t, pb.p[1]);
        return launch_panel_fwd(pb, st);
    }
    MARL_TRY(gemm2(c,
                   gemm_prob(c.Hs(t + 1), d.ld_nb, c.wpB(MARL_P_ENC_W0),
                             c.at(c.e.ZE1, t), d.ld_nm2, R, d.nm2, c.wp(MARL_P_ENC_B0)),
                   gemm_prob(c.HCs(t + 1), d.ld_na, c.wpB(MARL_P_POL_W0),
                             c.at(c.e.ZP1, t), d.ld_nla, R, d.nla, c.wp(MARL_P_POL_B0))));
    MARL_TRY(launch_ln_silu_fwd(c.at(c.e.ZP1, t), d.ld_nla, c.wp(MARL_P_POL_LNW),
                                c.wp(MARL_P_POL_LNB), c.at(c.e.AP1, t), d.ld_nla,
                                c.at(c.e.STP1, t), d.R, d.nla, st));
    MARL_TRY(launch_ln_silu_fwd(c.at(c.e.ZE1, t), d.ld_nm2, c.wp(MARL_P_ENC_LN0W),
                                c.wp(MARL_P_ENC_LN0B), c.at(c.e.AE1, t), d.ld_nm2,
                                c.at(c.e.STE1, t), d.R, d.nm2, st));
    MARL_TRY(gemm1(c, gemm_prob(c.at(c.e.AE1, t), d.ld_nm2, c.wpB(MARL_P_ENC_W1), c.at(c.e.ZE2, t), d.ld_nm, R,
                                d.n_m, c.wp(MARL_P_ENC_B1))));
    return launch_ln_silu_fwd(c.at(c.e.ZE2, t), d.ld_nm, c.wp(MARL_P_ENC_LN1W),
                              c.wp(MARL_P_ENC_LN1B), c.MSGs(t + 1), d.ld_nm,
                              c.at(c.e.STE2, t), d.R, d.n_m, st);
}

// the chain launch of step t: encoder(t) -> decoder(t+1) || policy layer(t) [-> sample(t) under SAMPLE_EPILOGUE]
static int step_chain(const Ctx& c, int t, const SampleArgs& sample) {
    const Dims& d = c.d;
    PanelFwdBatch pb{};
    pb.count = 2;
    PanelFwdProb& pe = pb.p[0];
    fill_enc_prob(c, t, pe);
    pe.by_batch = panel_chain_by_batch(d.na);
    pe.g_na = d.na;
    pe.g_nb = d.nb;
    if (t + 1 < d.ns) {
        fill_dec_layers(c, t + 1, pe.layer + 2);
        pe.nlayers = 4;
        pe.agg_at = 2;
        pe.xbar = c.at(c.e.MBAR, t + 1);
        pe.ld_xbar = d.ld_nm;
        pe.mix = c.opt.comm;  // (null: the mean)
        if (c.opt.comm) pe.gate = comm_gate(c, t + 1);
    }
    fill_pol_prob(c, t, pb.p[1]);
    if (c.plan.sample == SAMPLE_EPILOGUE) {
        pb.epi_prob = 2;
        pb.sample = sample;
        return launch_panel_fwd(pb, c.st, c.opt.explore.on);  // (the EXPLORE epilogues under exploration controls)
    }
    return launch_panel_fwd(pb, c.st);
}

// whole step on one stream (standalone step API)
static int step_core(const Ctx& c, int t, const StepIn& in) {
    MARL_TRY(step_cnn(c, t, in));
    MARL_TRY(step_decode(c, t));
    MARL_TRY(step_pos_lstm(c, t, in));
    return step_encode_policy(c, t);
}

// critic + prediction heads on `rows` rows starting at state slice t0 (+1)
static int heads_batched(const Ctx& c, int t0, int64_t rows, float* values, float* preds) {
    const Dims& d = c.d;
    hipStream_t st = c.st;
    if (c.plan.g3_lstm) {  // A = the images the LSTM epilogues wrote
        const int r1 = (int)((int64_t)(t0 + 1) * d.R);
        G3Batch g{};
        g.p[0] = g3_prob(c.img(c.e.HC3), r1, c.wp3k(MARL_P_CRI_W0), 0, d.n_a, c.at(c.e.ZC1), d.ld_nla, (int)rows, d.nla,
                         c.wp(MARL_P_CRI_B0));
        g.p[1] = g3_prob(c.img(c.e.H3), r1, c.wp3k(MARL_P_PRE_W0), 0, d.n_b, c.at(c.e.ZQ1), d.ld_nlb, (int)rows, d.nlb,
                         c.wp(MARL_P_PRE_B0));
        g.count = 2;
        MARL_TRY(launch_gemm_nt3(g, st));
    } else
    MARL_TRY(gemm2(c,
                   gemm_prob(c.HCs(t0 + 1), d.ld_na, c.wpB(MARL_P_CRI_W0),
                             c.at(c.e.ZC1), d.ld_nla, (int)rows, d.nla, c.wp(MARL_P_CRI_B0)),
                   gemm_prob(c.Hs(t0 + 1), d.ld_nb, c.wpB(MARL_P_PRE_W0),
                             c.at(c.e.ZQ1), d.ld_nlb, (int)rows, d.nlb, c.wp(MARL_P_PRE_B0))));
    const bool vdot = d.nla <= 384;  // the critic's output layer rides in the LayerNorm kernel
    MARL_TRY(launch_ln_silu_fwd(c.at(c.e.ZC1), d.ld_nla, c.wp(MARL_P_CRI_LNW), c.wp(MARL_P_CRI_LNB),
                                c.at(c.e.AC1), d.ld_nla, c.at(c.e.STC1), rows, d.nla, st,
                                vdot ? c.wp(MARL_P_CRI_W1) : nullptr, c.wp(MARL_P_CRI_B1), values));
    MARL_TRY(launch_ln_silu_fwd(c.at(c.e.ZQ1), d.ld_nlb, c.wp(MARL_P_PRE_LNW), c.wp(MARL_P_PRE_LNB),
                                c.at(c.e.AQ1), d.ld_nlb, c.at(c.e.STQ1), rows, d.nlb, st));
    if (!vdot)
        MARL_TRY(launch_rowdot(c.at(c.e.AC1), d.ld_nla, c.wp(MARL_P_CRI_W1), c.wp(MARL_P_CRI_B1),
                               values, rows, d.nla, st));
    MARL_TRY(gemm1(c, gemm_prob(c.at(c.e.AQ1), d.ld_nlb, c.wpB(MARL_P_PRE_W1),
                                preds, d.nC, (int)rows, d.nC, c.wp(MARL_P_PRE_B1))));
    return MARL_OK;
}

// the sampling arguments of a call under the installed controls (greedy reads neither noise nor generator)
static void explore_sample_args(const Explore& ex, SampleArgs& a) {
    if (!ex.on) return;
    a.ex_inv_tau = ex.inv_tau;
    a.ex_keep = ex.keep;
    a.ex_floor = ex.eps / (float)a.nA;
    a.ex_greedy = ex.greedy;
    if (ex.greedy) {
        a.noise = nullptr;
        a.rng_on = 0;
    }
}

// a call's sampling inputs and outputs, [Ns] leading (step t takes its slice)
struct SampleIo {
    const float* noise = nullptr;     // [Ns, R, nA] Exp(1) draws, or null
    const int64_t* forced = nullptr;  // [Ns, R] forced actions, or null
    uint64_t rng_seed = 0, rng_offset = 0;
    const void* counters = nullptr;
    int64_t *step_pos = nullptr, *step_actions = nullptr;
    float* step_logp = nullptr;       // null: probabilities only - no draw, no generator, none of the outputs above
    bool embed_next = false;          // the position embedding of step t+1 rides along with the move (episode loop)
};
// the one builder of step t's SampleArgs
static void fill_sample_args(const Ctx& c, const marl_config* cfg, int t, const SampleIo& io, SampleArgs& a) {
    const Dims& d = c.d;
    memset(&a, 0, sizeof(a));
    if (io.step_logp) {
        a.noise = io.noise ? io.noise + (size_t)t * d.R * d.nA : nullptr;
        a.rng_on = !io.noise && !io.forced;  // perf mode: Exp(1) drawn inside the kernel
        a.rng_seed = io.rng_seed ^ 0x9E3779B97F4A7C15ull;  // a key of its own (marl_draw_episode uses rng_seed)
        a.rng_ctr = (io.rng_offset << 16) + (uint64_t)t;
        a.rng_off_dev = io.counters ? &static_cast<const Counters*>(io.counters)->rng_offset : nullptr;
        a.forced = io.forced ? io.forced + (size_t)t * d.R : nullptr;
        a.step_pos = io.step_pos ? io.step_pos + (size_t)t * d.R * 2 : nullptr;
        a.step_actions = io.step_actions ? io.step_actions + (size_t)t * d.R : nullptr;
        a.step_logp = io.step_logp + (size_t)t * d.R;
    }
    if (io.embed_next && t + 1 < d.ns) {
        a.pe_W = c.wp(MARL_P_POS_W);
        a.pe_b = c.wp(MARL_P_POS_B);
        a.pe_gamma = c.wp(MARL_P_POS_LNW);
        a.pe_beta = c.wp(MARL_P_POS_LNB);
        a.pe_npos = c.at(c.e.NPOS, t + 1);
        a.pe_z = c.at(c.e.ZPOS, t + 1);
        a.pe_stats = c.at(c.e.STPOS, t + 1);
        a.pe_out = c.at(c.e.U, t + 1) + d.nf + d.n_mo;
        a.pe_ldz = d.ld_nd;
        a.pe_ldo = d.ld_nin;
        a.pe_nd = d.n_d;
        if (c.plan.u3_by_producers) {
            a.pe_img = c.img(c.e.U3);
            a.pe_row0 = c.u3_row(t + 1);
            a.pe_steps = img_steps(d.nin);
            a.pe_col0 = d.nf + d.n_mo;
        }
    }
    a.a_pol = c.at(c.e.AP1, t);
    a.ld_a = d.ld_nla;
    a.nla = d.nla;
    a.w1 = c.wp(MARL_P_POL_W1);
    a.ldw = d.ld_nla;
    a.b1 = c.wp(MARL_P_POL_B1);
    a.pos_in = c.POSs(t);
    a.pos_out = c.POSs(t + 1);
    a.probs = c.PROBSs(t);
    a.actions_i32 = c.ACTs(t);
    a.R = (int)d.R;
    a.nA = d.nA;
    a.H = d.H;
    a.W = d.W;
    a.f = d.f;
    for (int j = 0; j < d.nA; ++j) {
        a.table[j][0] = cfg->actions[j][0];
        a.table[j][1] = cfg->actions[j][1];
    }
    explore_sample_args(c.opt.explore, a);
}

// ---- the forward loop's step t, one function per form (Plan::chain / panels) ----
// what every form opens with: extractor, decoder(t) unless step t-1 ran it, lambda_t (t > 0: by sample(t-1)) + cells
static int fwd_open(const Ctx& c, int t, const StepIn& in, bool decode) {
    MARL_TRY(step_cnn(c, t, in));
    if (decode) MARL_TRY(step_decode(c, t));
    return step_pos_lstm(c, t, in, t > 0);
}
// chained panels: ... -> chain launch (encoder(t) -> decoder(t+1) || policy(t) [-> sample(t)])
static int fwd_step_chain(const Ctx& c, int t, const StepIn& in, const SampleArgs& a) {
    MARL_TRY(fwd_open(c, t, in, t == 0));
    MARL_TRY(step_chain(c, t, a));
    return c.plan.sample == SAMPLE_EPILOGUE ? MARL_OK : launch_sample(a, c.st, c.opt.explore.on);
}
// unchained panels: ... -> encoder(t) || policy(t) -> decoder(t+1) [|| sample(t): not for the last step]
static int fwd_step_panels(const Ctx& c, int t, const StepIn& in, const SampleArgs& a) {
    const bool ride = c.plan.sample == SAMPLE_RIDE && t + 1 < c.d.ns;
    MARL_TRY(fwd_open(c, t, in, t == 0));
    MARL_TRY(step_encode_policy(c, t));
    if (t + 1 < c.d.ns) MARL_TRY(step_decode(c, t + 1, ride ? &a : nullptr));
    return ride ? MARL_OK : launch_sample(a, c.st, c.opt.explore.on);
}
// rows (GEMM + LayerNorm launches): decoder(t) -> ... -> encoder(t), policy(t) -> decoder(t+1) -> sample(t).  (This
// form has always issued decoder(t+1) twice - here and at the top of step t+1, same inputs, same outputs.)
static int fwd_step_rows(const Ctx& c, int t, const StepIn& in, const SampleArgs& a) {
    MARL_TRY(fwd_open(c, t, in, true));
    MARL_TRY(step_encode_policy(c, t));
    if (t + 1 < c.d.ns) MARL_TRY(step_decode(c, t + 1));
    return launch_sample(a, c.st, c.opt.explore.on);
}

// ---------------------------------------------------------------------------
// pack / unpack
// ---------------------------------------------------------------------------
struct PermQueue {
    PermBatch b{};
    hipStream_t st;
    int rc = MARL_OK;
    explicit PermQueue(hipStream_t s) : st(s) { b.count = 0; }
    void push(const PermDesc& p) {
        if (rc != MARL_OK) return;
        b.d[b.count++] = p;
        if (b.count == kMaxPerm) flush();
    }
    void flush() {
        if (rc == MARL_OK && b.count > 0) rc = launch_permute(b, st);
        b.count = 0;
    }
};

static PermDesc perm(const float* src, float* dst, int rows, int cols, int dst_ld, int rd, int rs1,
                     int rs2, int cd, int cs1, int cs2, const float* src2 = nullptr) {
    PermDesc p;
    p.src = src;
    p.dst = dst;
    p.rows = rows;
    p.cols = cols;
    p.dst_ld = dst_ld;
    p.rd = rd;
    p.rs1 = rs1;
    p.rs2 = rs2;
    p.cd = cd;
    p.cs1 = cs1;
    p.cs2 = cs2;
    p.frag = 0;
    p.src2 = src2;
    return p;
}

// plain strided copy (src null: zero fill) as a descriptor of the batched permute kernel
static PermDesc copy_desc(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int cols) {
    return perm(src, dst, (int)rows, cols, (int)ldd, 1, (int)lds, 0, 1, 1, 0);
}

// initial recurrent state -> slice 0 of the all-steps buffers, one launch
static int load_state(const Ctx& c, const float* h, const float* cc_, const float* hc,
                      const float* cca, const float* msg) {
    const Dims& d = c.d;
    PermQueue q(c.st);
    q.push(copy_desc(h, d.n_b, c.Hs(0), d.ld_nb, d.R, d.n_b));
    q.push(copy_desc(cc_, d.n_b, c.Cs(0), d.ld_nb, d.R, d.n_b));
    q.push(copy_desc(hc, d.n_a, c.HCs(0), d.ld_na, d.R, d.n_a));
    q.push(copy_desc(cca, d.n_a, c.CCs(0), d.ld_na, d.R, d.n_a));
    // (no message: zeros, models.py:161-162 - the whole padded row)
    q.push(copy_desc(msg, d.n_m, c.MSGs(0), d.ld_nm, d.R, msg ? d.n_m : d.ld_nm));
    q.flush();
    MARL_TRY(q.rc);
    if (c.e.g3) {  // the image GEMMs read the state through its images
        ImgBatch ib{};
        ib.d[0] = ImgDesc{h, c.img(c.e.H3), d.R, d.n_b, d.n_b};
        ib.d[1] = ImgDesc{hc, c.img(c.e.HC3), d.R, d.n_a, d.n_a};
        ib.count = 2;
        MARL_TRY(launch_images(ib, c.st));
    }
    return MARL_OK;
}


static int pack_weights(const Dims& d, const WLayout& w, const float* const* params, float* W,
                        hipStream_t st) {
    PermQueue q(st);
    for (int i = 0; i < MARL_NPARAMS; ++i) {
        const ParamMeta m = param_meta(d, i);
        if (m.kind == PK_NONE) continue;
        const float* src = params[i];
        if (!src) {
            set_error("parameter %d is null", i);
            return MARL_EINVAL;
        }
        if (m.kind == PK_MATRIX) {
            q.push(perm(src, W + w.wp[i], m.n, m.k, w.ldp[i], 1, m.k, 0, 1, 1, 0));
            q.push(perm(src, W + w.wt[i], m.k, m.n, w.ldt[i], 1, 1, 0, 1, m.k, 0));
        } else if (m.kind == PK_CONV) {
            const int ci = m.k / 9;
            // packed [co][tap*ci + c]  <- src [co][c][tap]
            q.push(perm(src, W + w.wp[i], m.n, m.k, w.ldp[i], 1, m.k, 0, ci, 1, 9));
            // transposed [tap*ci + c][co]
            q.push(perm(src, W + w.wt[i], m.k, m.n, w.ldt[i], ci, 1, 9, 1, m.k, 0));
        } else {
            q.push(perm(src, W + w.wp[i], 1, m.n, m.n, 1, 0, 0, 1, 1, 0));
        }
    }
    q.push(perm(params[MARL_P_LB_BIH], W + w.bsum_b, 1, 4 * d.n_b, 4 * d.n_b, 1, 0, 0, 1, 1, 0,
                params[MARL_P_LB_BHH]));
    q.push(perm(params[MARL_P_LA_BIH], W + w.bsum_a, 1, 4 * d.n_a, 4 * d.n_a, 1, 0, 0, 1, 1, 0,
                params[MARL_P_LA_BHH]));
    q.flush();
    MARL_TRY(q.rc);
    // fragment-order copies of the deeper conv weights (read back from the packed copies just written):
    // dst row (nt * steps + kk) * 4 + quad, column l16 * 4 + j  <-  packed [nt * 16 + l16][kk * 16 + quad * 4 + j]
    for (int i = 0; i < MARL_NPARAMS; ++i) {
        const ParamMeta m = param_meta(d, i);
        if (!w.wf[i]) continue;
        const int steps = m.k / 16;
        q.push(perm(W + w.wp[i], W + w.wf[i], (m.n / 16) * steps * 4, 64, 64, steps * 4, 16 * w.ldp[i], 4, 4,
                    w.ldp[i], 1));
    }
    // fragment-order copies for the panel kernels, from the packed / transposed copies just written
    for (int i = 0; i < MARL_NPARAMS; ++i) {
        const ParamMeta m = param_meta(d, i);
        if (w.wpf[i]) {
            PermDesc p = perm(W + w.wp[i], W + w.wpf[i], m.n, m.k, 0, 1, w.ldp[i], 0, 1, 1, 0);
            p.frag = w.gpf[i];
            q.push(p);
        }
        if (w.wtf[i]) {
            PermDesc p = perm(W + w.wt[i], W + w.wtf[i], m.k, m.n, 0, 1, w.ldt[i], 0, 1, 1, 0);
            p.frag = w.gtf[i];
            q.push(p);
        }
    }
    q.flush();
    MARL_TRY(q.rc);
    // bf16x3 images of every matrix copy (read back from the fp32 copies just written)
    SplitBatch sb{};
    sb.count = 0;
    for (int i = 0; i < MARL_NPARAMS; ++i) {
        const ParamMeta m = param_meta(d, i);
        if (m.kind != PK_MATRIX) continue;
        sb.d[sb.count++] = SplitDesc{W + w.wp[i], W + w.wp3[i], m.n, m.k, w.ldp[i], (m.k + 31) / 32};
        sb.d[sb.count++] = SplitDesc{W + w.wt[i], W + w.wt3[i], m.k, m.n, w.ldt[i], (m.n + 31) / 32};
    }
    MARL_TRY(launch_split_weights(sb, st));
    ImgBatch ib{};
    ib.count = 0;
    for (int i = 0; i < MARL_NPARAMS; ++i) {
        const ParamMeta m = param_meta(d, i);
        if (m.kind != PK_MATRIX || !w.wp3k[i]) continue;
        if (ib.count + 2 > kMaxImgDesc) {
            MARL_TRY(launch_images(ib, st));
            ib.count = 0;
        }
        ib.d[ib.count++] = ImgDesc{W + w.wp[i], W + w.wp3k[i], m.n, m.k, w.ldp[i]};
        ib.d[ib.count++] = ImgDesc{W + w.wt[i], W + w.wt3k[i], m.k, m.n, w.ldt[i]};
    }
    return launch_images(ib, st);
}

// which: 0 every parameter, 1 only the heads' matrices (MARL_P_POL_W0 .. MARL_P_PRE_B1: final before the reverse loop -
// marl_backward_heads_event), 2 everything but those
static int unpack_grads(const Ctx& c, float* const* grads, int which = 0) {
    PermQueue q(c.st);
    for (int i = 0; i < MARL_NPARAMS; ++i) {
        const bool head = i >= MARL_P_POL_W0 && i <= MARL_P_PRE_B1;
        if ((which == 1 && !head) || (which == 2 && head)) continue;
        const ParamMeta m = param_meta(c.d, i);
        if (m.kind == PK_MATRIX) {
            q.push(perm(c.gp(i), grads[i], m.n, m.k, m.k, 1, c.w.ldp[i], 0, 1, 1, 0));
        } else if (m.kind == PK_CONV) {
            const int ci = m.k / 9;
            // dst [co][c*9 + tap] <- packed [co][tap*ci + c]
            q.push(perm(c.gp(i), grads[i], m.n, m.k, m.k, 1, c.w.ldp[i], 0, 9, 1, ci));
        }
    }
    if (which != 1) {
        // b_hh enters every gate sum exactly like b_ih: same gradient
        q.push(perm(grads[MARL_P_LB_BIH], grads[MARL_P_LB_BHH], 1, 4 * c.d.n_b, 4 * c.d.n_b, 1, 0, 0, 1, 1, 0));
        q.push(perm(grads[MARL_P_LA_BIH], grads[MARL_P_LA_BHH], 1, 4 * c.d.n_a, 4 * c.d.n_a, 1, 0, 0, 1, 1, 0));
    }
    q.flush();
    return q.rc;
}

// ---------------------------------------------------------------------------
// backward helpers
// ---------------------------------------------------------------------------
// weight gradient gp(pidx) = A^T B over `rows` rows; bias (nullable) = column sums of A
static int tn(const Ctx& c, const float* a, int lda, const float* b, int ldb, int pidx, int ni,
              int nj, int64_t rows, float* bias = nullptr) {
    RedQueue* q = c.defer_this(gemm_tn_scratch_bytes(ni, nj, rows)) ? c.rq : nullptr;
    return launch_gemm_tn(a, lda, b, ldb, c.gp(pidx), c.w.ldp[pidx], ni, nj, rows, c.at(c.e.TNS),
                          c.e.tns_bytes, c.st, bias, q, q ? c.tq : nullptr);
}
// the same from images (rows = contraction index; A [rows, ni], B [rows, nj], both starting at image row 0)
static int tn3(const Ctx& c, const char* a3, int ni, const char* b3, int nj, int pidx, int64_t rows, float* bias) {
    const GemmPlan plan = g3_tn_plan(ni, nj, rows);
    if (plan.scratch_bytes > c.e.tns_bytes) {
        set_error("tn3: scratch too small");
        return MARL_ESIZE;
    }
    return gemm_tn3(plan, a3, ni, b3, nj, rows, c.gp(pidx), c.w.ldp[pidx], bias, c.at(c.e.TNS), c.st);
}
// both weight gradients of one LSTM cell from one launch (gemm3.hip, gemm_tn3_cell_kernel): G read once
static int tn3_cell(const Ctx& c, const GemmPlan& plan, const char* g3, int ni, const char* u3, int nin, int p_ih,
                    const char* h3, int nh, int p_hh, int64_t rows, float* bias) {
    if (plan.scratch_bytes > c.e.tns_bytes) {
        set_error("tn3_cell: scratch too small");
        return MARL_ESIZE;
    }
    return gemm_tn3_cell(plan, g3, ni, u3, nin, h3, nh, rows, c.gp(p_ih), c.w.ldp[p_ih], c.gp(p_hh), c.w.ldp[p_hh], bias,
                         c.at(c.e.TNS), c.st);
}
// scratch for `blocks` affine partial rows of width 2n: the queue's when the reduction can wait
static float* part_scratch(const Ctx& c, int64_t blocks, int n, int acc, RedQueue*& q) {
    q = acc ? nullptr : c.rq;
    if (!q) return c.at(c.e.PART);
    float* p = q->take((size_t)blocks * 2 * n);
    if (q->rc != MARL_OK) q = nullptr;  // cannot happen with the layout's sizes; fall back
    return q ? p : c.at(c.e.PART);
}
// LayerNorm+SiLU backward in place (da -> dz) with affine gradients (accumulated when acc)
static int ln_bwd(const Ctx& c, float* da, int ldda, const float* z, int ldz, const float* stats,
                  int pw, int pb, int64_t rows, int n, float* const* grads, int acc,
                  float* dz = nullptr, int lddz = 0) {
    if (!dz) {
        dz = da;
        lddz = ldda;
    }
    RedQueue* q;
    float* part = part_scratch(c, ln_bwd_blocks(rows, n), n, acc, q);
    MARL_TRY(launch_ln_silu_bwd(da, ldda, z, ldz, stats, c.wp(pw), c.wp(pb), dz, lddz, part, rows, n,
                                c.st));
    return launch_reduce_affine(part, ln_bwd_blocks(rows, n), n, grads[pw], grads[pb], acc, c.st, q);
}

// LayerNorm+SiLU backward of a hidden layer whose successor has only kin <= 4 outputs: the
// incoming gradient g * W1 is formed inside the kernel instead of by a K = kin GEMM
static int ln_bwd_rank(const Ctx& c, const float* g, int ldg, int kin, int w1, const float* z, int ldz,
                       const float* stats, int pw, int pb, int64_t rows, int n, float* const* grads,
                       float* dz, int lddz) {
    RedQueue* q;
    float* part = part_scratch(c, ln_bwd_blocks(rows, n), n, 0, q);
    MARL_TRY(launch_ln_silu_bwd_rank(g, ldg, kin, c.wt(w1), p4(kin), z, ldz, stats, c.wp(pw),
                                     c.wp(pb), dz, lddz, part, rows, n, c.st));
    return launch_reduce_affine(part, ln_bwd_blocks(rows, n), n, grads[pw], grads[pb], 0, c.st, q);
}

// the panel launch could not write a gate-gradient image it was asked for (shapes without the row-wise
// tail): build it from the fp32 gradients - correct, one extra pass
static int gate_image_fallback(const Ctx& c, const PanelBwdProb& pd, int t) {
    const Dims& d = c.d;
    ImgBatch ib{};
    ib.count = 0;
    if (pd.has_cellb && pd.cellb.g3 && !pd.cellb_img_done)
        ib.d[ib.count++] = ImgDesc{c.at(c.e.GB, t), c.img(c.e.GB3) + img_off((int64_t)t * d.R, 0, img_steps(4 * d.n_b)),
                                   d.R, 4 * d.n_b, d.ld_gb};
    if (pd.has_cell && pd.cell.g3 && !pd.cell_img_done)
        ib.d[ib.count++] = ImgDesc{c.at(c.e.GA, t), c.img(c.e.GA3) + img_off((int64_t)t * d.R, 0, img_steps(4 * d.n_a)),
                                   d.R, 4 * d.n_a, d.ld_ga};
    return launch_images(ib, c.st);
}

// marl_step_backward: what one standalone step (nb_steps = 1) adds to the episode's backward
struct StepBwd {
    const float* obs = nullptr;      // [R, C, f, f]: the first convolution's input (there is no image batch)
    const float* g_probs = nullptr;  // dL/dprobs [R, nA] (null: only the dlogp term)
    // upstream gradients of the step's new message and state [R, n] tight (null = zero)
    const float *g_msg = nullptr, *g_h = nullptr, *g_c = nullptr, *g_hc = nullptr, *g_cc = nullptr;
    // gradients of the step's inputs [R, n] tight (null = not wanted)
    float *d_msg = nullptr, *d_h = nullptr, *d_c = nullptr, *d_hc = nullptr, *d_cc = nullptr;
};

// ---- one builder per descriptor (the backward's counterparts of fill_dec_layers / fill_enc_prob) ----

// elementwise backward of the belief (which = 0) or action (1) cell of step t: dh = DH / DH^[t + 1], gates G[t]
static LstmBwdArgs cell_bwd_args(const Ctx& c, int which, int t) {
    const Dims& d = c.d;
    const int n = which ? d.n_a : d.n_b, ld = which ? d.ld_na : d.ld_nb;
    return LstmBwdArgs{which ? c.DHCs(t + 1) : c.DHs(t + 1), c.at(which ? c.e.DCC : c.e.DC),
                       c.at(which ? c.e.GA : c.e.GB, t), which ? c.CCs(t) : c.Cs(t),
                       which ? c.CCs(t + 1) : c.Cs(t + 1), ld, ld, which ? d.ld_ga : d.ld_gb, ld, n,
                       c.e.g3 ? c.img(which ? c.e.GA3 : c.e.GB3) : nullptr, (int)((int64_t)t * d.R), img_steps(4 * n),
                       c.plan.skip_f32};
}

// the decoder's two layers of step t, output side first (pblk: floats per step and column of a PLN partial)
static void fill_dec_bwd_layers(const Ctx& c, int t, size_t pblk, float* ddbar, float* dad1, PanelBwdLayer* layer) {
    const Dims& d = c.d;
    layer[0] = PanelBwdLayer{c.at(c.e.ZD2, t), d.ld_nmo, c.at(c.e.STD2, t), c.wp(MARL_P_DEC_LN1W),
                             c.wp(MARL_P_DEC_LN1B), d.n_mo, ddbar, d.ld_dbl,
                             c.at(c.e.PLN[0]) + (size_t)t * pblk * d.n_mo, c.wtf(MARL_P_DEC_W1),
                             c.w.gtf[MARL_P_DEC_W1], d.nm2};
    layer[1] = PanelBwdLayer{c.at(c.e.ZD1, t), d.ld_nm2, c.at(c.e.STD1, t), c.wp(MARL_P_DEC_LN0W),
                             c.wp(MARL_P_DEC_LN0B), d.nm2, dad1, d.ld_nm2,
                             c.at(c.e.PLN[1]) + (size_t)t * pblk * d.nm2, c.wtf(MARL_P_DEC_W0),
                             c.w.gtf[MARL_P_DEC_W0], d.n_m};
}
// the encoder's two layers of step t (dz -> DZE2[t], DAE1[t])
static void fill_enc_bwd_layers(const Ctx& c, int t, size_t pblk, PanelBwdLayer* layer) {
    const Dims& d = c.d;
    layer[0] = PanelBwdLayer{c.at(c.e.ZE2, t), d.ld_nm, c.at(c.e.STE2, t), c.wp(MARL_P_ENC_LN1W),
                             c.wp(MARL_P_ENC_LN1B), d.n_m, c.at(c.e.DZE2) + (size_t)t * d.R * d.ld_nm, d.ld_nm,
                             c.at(c.e.PLN[2]) + (size_t)t * pblk * d.n_m, c.wtf(MARL_P_ENC_W1),
                             c.w.gtf[MARL_P_ENC_W1], d.nm2};
    layer[1] = PanelBwdLayer{c.at(c.e.ZE1, t), d.ld_nm2, c.at(c.e.STE1, t), c.wp(MARL_P_ENC_LN0W),
                             c.wp(MARL_P_ENC_LN0B), d.nm2, c.at(c.e.DAE1) + (size_t)t * d.R * d.ld_nm2, d.ld_nm2,
                             c.at(c.e.PLN[3]) + (size_t)t * pblk * d.nm2, c.wtf(MARL_P_ENC_W0),
                             c.w.gtf[MARL_P_ENC_W0], d.n_b};
}

// `floats` of per-workgroup weight-gradient slabs: the deferred queue's scratch when their reduction may wait, else TNS
static float* slab_scratch(const Ctx& c, size_t floats) {
    if (c.rq && c.defer_this(floats * sizeof(float))) {
        float* p = c.rq->take(floats);
        if (c.rq->rc == MARL_OK) return p;
    }
    return c.at(c.e.TNS);
}
// ... and their reduction into gp(pidx) [co, k] and bias [co]: queued behind the scratch taken, or launched now
static int slab_reduce(const Ctx& c, float* part_w, float* part_b, int blocks, int co, int k, int pidx, float* bias) {
    if (c.rq && part_w != c.at(c.e.TNS)) {
        c.rq->push(part_w, (int64_t)co * k, blocks, co * k, c.gp(pidx), co * k, k, c.w.ldp[pidx], nullptr, 0);
        c.rq->push(part_b, co, blocks, co, bias, co, co, co, nullptr, 0);
        return MARL_OK;
    }
    return launch_slab_reduce(part_w, (int64_t)co * k, blocks, c.gp(pidx), c.w.ldp[pidx], co, k, part_b, bias, c.st);
}

// ---- the backward driver: what lives across its parts ----
struct BwdState {
    Ctx c;  // the caller's context with the queues below installed (the rows path drops them before its loop)
    RedQueue rq;
    TnQueue tq;
    float* const* grads;
    const StepBwd* sb;
    bool enc_last = false;     // a standalone step with an upstream gradient of its new message
    bool heads_early = false;  // the heads' gradients were flushed and unpacked ahead of the loop
    int pln_blocks = 0;        // workgroups of one panel launch = partial rows per step in PLN
    bool action_done = false;  // the action cell of this step was handled by the ride-along
    bool belief_done = false;  // the belief cell: by the epilogue of the chained panel launch
};

// ---- heads, batched over all steps -----------------------------------------------
static int bwd_heads(BwdState& s, const float* g_preds, const float* g_logp, const float* g_values,
                     const float* g_probs) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    const StepBwd* sb = s.sb;
    float* const* grads = s.grads;
    hipStream_t st = c.st;
    const int64_t NR = d.NR;
    const int ns = d.ns;
    // prediction head (networks/prediction.py:11-14)
    {   // output gradients into the padded layouts + the zero initial state gradients: one launch
        PermQueue q(st);
        q.push(copy_desc(g_preds, d.nC, c.at(c.e.GPRED), d.ld_nC, NR, g_preds ? d.nC : d.ld_nC));
        q.push(copy_desc(g_values, 1, c.at(c.e.DVAL), 4, NR, g_values ? 1 : 4));
        q.push(copy_desc(nullptr, 0, c.DHs(0), d.ld_nb, d.R, d.ld_nb));
        q.push(copy_desc(nullptr, 0, c.DHCs(0), d.ld_na, d.R, d.ld_na));
        q.push(copy_desc(nullptr, 0, c.at(c.e.DC), d.ld_nb, d.R, d.ld_nb));
        q.push(copy_desc(nullptr, 0, c.at(c.e.DCC), d.ld_na, d.R, d.ld_na));
        q.flush();
        MARL_TRY(q.rc);
    }
    if (sb) {  // the chain starts from the upstream dL/dc, dL/dc^ of the step's new cell states
        MARL_TRY(launch_acc2d(c.at(c.e.DC), d.ld_nb, sb->g_c, d.n_b, d.R, d.n_b, st));
        MARL_TRY(launch_acc2d(c.at(c.e.DCC), d.ld_na, sb->g_cc, d.n_a, d.R, d.n_a, st));
        // patch positions of the first convolution's weight gradient: every patch at (0, 0) of its own image
        MARL_TRY(launch_fill(reinterpret_cast<float*>(c.POSs(0)), d.R * 2, 0.f, st));
    }
    MARL_TRY(gemm1(c, gemm_prob(c.at(c.e.GPRED), d.ld_nC, c.wtB(MARL_P_PRE_W1),
                                c.at(c.e.DAQ1), d.ld_nlb, (int)NR, d.nlb)));
    MARL_TRY(tn(c, c.at(c.e.GPRED), d.ld_nC, c.at(c.e.AQ1), d.ld_nlb, MARL_P_PRE_W1, d.nC, d.nlb, NR, grads[MARL_P_PRE_B1]));
    MARL_TRY(ln_bwd(c, c.at(c.e.DAQ1), d.ld_nlb, c.at(c.e.ZQ1), d.ld_nlb, c.at(c.e.STQ1),
                    MARL_P_PRE_LNW, MARL_P_PRE_LNB, NR, d.nlb, grads, 0));
    MARL_TRY(tn(c, c.at(c.e.DAQ1), d.ld_nlb, c.Hs(1), d.ld_nb, MARL_P_PRE_W0, d.nlb, d.n_b, NR, grads[MARL_P_PRE_B0]));
    // critic head (networks/policy.py:23-27)
    MARL_TRY(tn(c, c.at(c.e.DVAL), 4, c.at(c.e.AC1), d.ld_nla, MARL_P_CRI_W1, 1, d.nla, NR, grads[MARL_P_CRI_B1]));
    if (d.nla <= 384) {
        MARL_TRY(ln_bwd_rank(c, c.at(c.e.DVAL), 4, 1, MARL_P_CRI_W1, c.at(c.e.ZC1), d.ld_nla,
                             c.at(c.e.STC1), MARL_P_CRI_LNW, MARL_P_CRI_LNB, NR, d.nla, grads,
                             c.at(c.e.DAC1), d.ld_nla));
    } else {
        MARL_TRY(gemm1(c, gemm_prob(c.at(c.e.DVAL), 4, c.wtB(MARL_P_CRI_W1), c.at(c.e.DAC1),
                                    d.ld_nla, (int)NR, d.nla)));
        MARL_TRY(ln_bwd(c, c.at(c.e.DAC1), d.ld_nla, c.at(c.e.ZC1), d.ld_nla, c.at(c.e.STC1),
                        MARL_P_CRI_LNW, MARL_P_CRI_LNB, NR, d.nla, grads, 0));
    }
    MARL_TRY(tn(c, c.at(c.e.DAC1), d.ld_nla, c.HCs(1), d.ld_na, MARL_P_CRI_W0, d.nla, d.n_a, NR, grads[MARL_P_CRI_B0]));
    // policy head: logp = log softmax(logits)[a]  (networks/policy.py:12-16, core/agent.py:57-61)
    if (sb && sb->g_probs) g_probs = sb->g_probs;
    // the saved rows hold the behaviour policy (marl_policy_explore): its own backward, both cases (greedy alone
    // leaves the distribution the plain softmax: the kernels below, as always)
    const Explore& ex = c.opt.explore;
    if (ex.on && (ex.inv_tau != 1.f || ex.eps != 0.f))
        MARL_TRY(launch_policy_dlogits_explore(g_logp, g_probs, c.PROBSs(0), c.ACTs(0), c.at(c.e.DLOG), d.ld_nA, NR,
                                               d.nA, ex.inv_tau, ex.keep, ex.eps / (float)d.nA, st));
    else if (g_probs)  // dL/dprobs from the caller (+ the dlogp term): a standalone step [R, nA] or all steps [Ns, R, nA]
        MARL_TRY(launch_policy_dlogits_probs(g_logp, g_probs, c.PROBSs(0), c.ACTs(0), c.at(c.e.DLOG),
                                             d.ld_nA, NR, d.nA, st));
    else
        MARL_TRY(launch_policy_dlogits(g_logp, c.PROBSs(0), c.ACTs(0), c.at(c.e.DLOG), d.ld_nA, NR,
                                       d.nA, st));
    MARL_TRY(tn(c, c.at(c.e.DLOG), d.ld_nA, c.at(c.e.AP1, 0), d.ld_nla, MARL_P_POL_W1, d.nA, d.nla, NR, grads[MARL_P_POL_B1]));
    if (d.nA <= 4 && d.nla <= 384) {
        MARL_TRY(ln_bwd_rank(c, c.at(c.e.DLOG), d.ld_nA, d.nA, MARL_P_POL_W1, c.at(c.e.ZP1, 0),
                             d.ld_nla, c.at(c.e.STP1, 0), MARL_P_POL_LNW, MARL_P_POL_LNB, NR, d.nla,
                             grads, c.at(c.e.DAP1), d.ld_nla));
    } else {
        MARL_TRY(gemm1(c, gemm_prob(c.at(c.e.DLOG), d.ld_nA, c.wtB(MARL_P_POL_W1),
                                    c.at(c.e.DAP1), d.ld_nla, (int)NR, d.nla)));
        MARL_TRY(ln_bwd(c, c.at(c.e.DAP1), d.ld_nla, c.at(c.e.ZP1, 0), d.ld_nla, c.at(c.e.STP1, 0),
                        MARL_P_POL_LNW, MARL_P_POL_LNB, NR, d.nla, grads, 0));
    }
    MARL_TRY(tn(c, c.at(c.e.DAP1), d.ld_nla, c.HCs(1), d.ld_na, MARL_P_POL_W0, d.nla, d.n_a, NR, grads[MARL_P_POL_B0]));
    // gradients reaching h_t / h^_t from the heads, all steps at once
    {
        GemmProb ph = gemm_prob(c.at(c.e.DAQ1), d.ld_nlb, c.wtB(MARL_P_PRE_W0), c.DHs(1), d.ld_nb, (int)NR, d.n_b);
        GemmProb pa = gemm_prob(c.at(c.e.DAP1), d.ld_nla, c.wtB(MARL_P_POL_W0), c.DHCs(1), d.ld_na, (int)NR, d.n_a);
        gemm_add_seg(pa, c.at(c.e.DAC1), d.ld_nla, c.wtB(MARL_P_CRI_W0));
        MARL_TRY(gemm2(c, ph, pa));
    }
    if (sb) {  // + the upstream dL/dh, dL/dh^ of the step's new hidden states
        MARL_TRY(launch_acc2d(c.DHs(ns), d.ld_nb, sb->g_h, d.n_b, d.R, d.n_b, st));
        MARL_TRY(launch_acc2d(c.DHCs(ns), d.ld_na, sb->g_hc, d.n_a, d.R, d.n_a, st));
    }

    // Data parallelism (parallel.py, BucketedGradAllReduce): every gradient of the three heads' parameters (POL_*,
    // CRI_*, PRE_*) is complete here, ahead of the ~1.4 ms reverse loop - flush what they queued and mark the point.
    s.heads_early = c.opt.heads_event != nullptr && !sb;
    if (s.heads_early) {
        if (c.tq) MARL_TRY(launch_tn_queue(s.tq, c.rq, st));
        MARL_TRY(s.rq.flush());
        MARL_TRY(unpack_grads(c, grads, 1));  // (their matrices leave the packed layout now; the end skips them)
        MARL_HIP_CHECK(hipEventRecord(c.opt.heads_event, st));
    }
    return MARL_OK;
}

// ---- reverse-time loop over the recurrent chain ----------------------------------

// rows path: the encoder of step t backward from a ready DZE2[t] (d loss / d its message); adds dL/dh into dh
static int enc_bwd_rows(const BwdState& s, int t, int acc, float* dh) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    const int R = (int)d.R;
    float* dze2 = c.at(c.e.DZE2) + (size_t)t * d.R * d.ld_nm;
    float* dae1 = c.at(c.e.DAE1) + (size_t)t * d.R * d.ld_nm2;
    MARL_TRY(ln_bwd(c, dze2, d.ld_nm, c.at(c.e.ZE2, t), d.ld_nm, c.at(c.e.STE2, t), MARL_P_ENC_LN1W,
                    MARL_P_ENC_LN1B, d.R, d.n_m, s.grads, acc));
    MARL_TRY(gemm1(c, gemm_prob(dze2, d.ld_nm, c.wtB(MARL_P_ENC_W1), dae1, d.ld_nm2, R, d.nm2)));
    MARL_TRY(ln_bwd(c, dae1, d.ld_nm2, c.at(c.e.ZE1, t), d.ld_nm2, c.at(c.e.STE1, t), MARL_P_ENC_LN0W,
                    MARL_P_ENC_LN0B, d.R, d.nm2, s.grads, acc));
    return gemm1(c, gemm_prob(dae1, d.ld_nm2, c.wtB(MARL_P_ENC_W0), dh, d.ld_nb, R, d.n_b, nullptr, 1));
}

// recurrent paths dh_{t-1} += dgates * W_hh, and d(decoded message) = columns [nf, nf + n_mo) of dU - independent
// products of the same gate gradients, one launch
static int bwd_recurrent(const BwdState& s, int t, float* ddbar, float* ddbar2) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    const int R = (int)d.R;
    // (gates of cell `which`, weight, its first row, output, ld, width, accumulate).  The panel paths take all four,
    // of EQUAL depth (a two-segment one would run twice as long as the others and finish the launch alone): each
    // cell's share of dU[:, nf:] - the decoded-message AND the position-embedding columns, which sit next to each
    // other and fit the same two 64-wide tiles - goes to its own buffer; the decoder panel sums the message halves
    // while staging, the embedding halves are summed once after the loop.  The big dU product then only covers the
    // CNN features.
    const struct { int which, w, row0; float* out; int ldo, n, acc; } prod[4] = {
        {0, MARL_P_LB_WHH, 0, c.DHs(t), d.ld_nb, d.n_b, 1},
        {1, MARL_P_LA_WHH, 0, c.DHCs(t), d.ld_na, d.n_a, 1},
        {0, MARL_P_LB_WIH, d.nf, ddbar, d.ld_dbl, d.n_mo + d.n_d, 0},
        {1, MARL_P_LA_WIH, d.nf, ddbar2, d.ld_dbl, d.n_mo + d.n_d, 0}};
    const int count = c.plan.panels_bwd ? 4 : 2;
    if (c.plan.panels_bwd && c.e.g3) {  // from the images of the gate gradients
        G3Batch g{};
        for (int i = 0; i < count; ++i) {
            const auto& q = prod[i];
            g.p[i] = g3_prob(c.img(q.which ? c.e.GA3 : c.e.GB3), (int)((int64_t)t * d.R), c.wt3k(q.w), q.row0,
                             4 * (q.which ? d.n_a : d.n_b), q.out, q.ldo, R, q.n, nullptr, q.acc);
        }
        g.count = count;
        return launch_gemm_nt3(g, c.st);
    }
    GemmBatch gb{};
    for (int i = 0; i < count; ++i) {
        const auto& q = prod[i];
        gb.p[i] = gemm_prob(c.at(q.which ? c.e.GA : c.e.GB, t), q.which ? d.ld_ga : d.ld_gb,
                            c.wtB(q.w).from_row(q.row0), q.out, q.ldo, R, q.n, nullptr, q.acc);
    }
    gb.count = count;
    if (!c.plan.panels_bwd) {  // rows path: only the message columns, both cells' shares summed by one two-segment product
        GemmProb& p = gb.p[gb.count++];
        p = gemm_prob(c.at(c.e.GB, t), d.ld_gb, c.wtB(MARL_P_LB_WIH).from_row(d.nf), ddbar, d.ld_dbl, R, d.n_mo);
        gemm_add_seg(p, c.at(c.e.GA, t), d.ld_ga, c.wtB(MARL_P_LA_WIH).from_row(d.nf));
    }
    return launch_gemm_nt(gb, c.st);
}

// the decoder panel of step t as both panel bodies launch it.  The action cell's backward of step t-1 only needs
// dh^_t, which is complete after step t's W_hh product; it rides along (extra workgroups) with this launch, so that
// from the second iteration on only the belief cell is left for the separate launch.
static void fill_dec_bwd_prob(BwdState& s, int t, float* ddbar, float* ddbar2, PanelBwdProb& pd) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    pd.da = ddbar;
    pd.ldda = d.ld_dbl;
    pd.da2 = ddbar2;
    pd.ldda2 = d.ld_dbl;
    pd.m = (int)d.R;
    pd.nlayers = 2;
    fill_dec_bwd_layers(c, t, (size_t)s.pln_blocks * 2, ddbar, c.at(c.e.DAD1) + (size_t)t * d.R * d.ld_nm2, pd.layer);
    pd.dx = c.at(c.e.DMBAR);
    pd.lddx = d.ld_nm;
    pd.accumulate = 0;
    if (t > 0) {  // action cell of step t-1: gates GA[t-1], dh^ = DHC[t]
        pd.has_cell = 1;
        pd.cell = cell_bwd_args(c, 1, t - 1);
        pd.cell_rows = d.R;
        s.action_done = true;
    }
}

// chained panels: decoder(t) -> mean -> encoder(t-1) -> dh_t -> belief cell(t-1), one launch
static int bwd_step_chain(BwdState& s, int t, float* ddbar, float* ddbar2) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    PanelBwdProb pd{};
    fill_dec_bwd_prob(s, t, ddbar, ddbar2, pd);
    pd.by_batch = panel_chain_by_batch(d.na);
    pd.g_na = d.na;
    pd.g_nb = d.nb;
    if (t > 0) {
        pd.nlayers = 4;
        pd.agg_at = 2;
        pd.mix = c.opt.comm;  // (null: the self-adjoint mean; else the kernel applies M^T)
        if (c.opt.comm) pd.gate = comm_gate(c, t);
        fill_enc_bwd_layers(c, t - 1, (size_t)s.pln_blocks * 2, pd.layer + 2);
        pd.dx = c.DHs(t);
        pd.lddx = d.ld_nb;
        pd.accumulate = 1;
        pd.has_cellb = 1;
        pd.cellb = cell_bwd_args(c, 0, t - 1);
        s.belief_done = true;
    }
    MARL_TRY(launch_panel_bwd(pd, c.st));
    return gate_image_fallback(c, pd, t - 1);
}

// unchained panels: decoder(t) -> DMBAR, then (t > 0) the exchange and encoder(t-1) -> dh_t in a second launch
static int bwd_step_panels(BwdState& s, int t, float* ddbar, float* ddbar2) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    PanelBwdProb pd{};
    fill_dec_bwd_prob(s, t, ddbar, ddbar2, pd);
    MARL_TRY(launch_panel_bwd(pd, c.st));
    MARL_TRY(gate_image_fallback(c, pd, t - 1));
    if (t == 0) return MARL_OK;
    PanelBwdProb pe{};
    pe.da = c.at(c.e.DMBAR);  // message mean applied while staging
    pe.ldda = d.ld_nm;
    pe.agg_na = d.na;
    pe.agg_nb = d.nb;
    if (c.opt.comm) {  // M^T in place (a thread owns one (batch, column) over all agents), then plain rows
        MARL_TRY(mix_msg(c, t, c.at(c.e.DMBAR), c.at(c.e.DMBAR), d.ld_nm, 1));
        pe.agg_na = pe.agg_nb = 0;
    }
    pe.m = (int)d.R;
    pe.nlayers = 2;
    fill_enc_bwd_layers(c, t - 1, (size_t)s.pln_blocks * 2, pe.layer);
    pe.dx = c.DHs(t);
    pe.lddx = d.ld_nb;
    pe.accumulate = 1;
    return launch_panel_bwd(pe, c.st);
}

// rows: GEMM + ln_bwd per layer; the LayerNorm reductions accumulate into the gradients step by step
static int bwd_step_rows(const BwdState& s, int t, float* ddbar) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    const int R = (int)d.R;
    const int first = (t == d.ns - 1);
    float* dad1 = c.at(c.e.DAD1) + (size_t)t * d.R * d.ld_nm2;
    MARL_TRY(ln_bwd(c, ddbar, d.ld_dbl, c.at(c.e.ZD2, t), d.ld_nmo, c.at(c.e.STD2, t),
                    MARL_P_DEC_LN1W, MARL_P_DEC_LN1B, d.R, d.n_mo, s.grads, !first));
    MARL_TRY(gemm1(c, gemm_prob(ddbar, d.ld_dbl, c.wtB(MARL_P_DEC_W1), dad1, d.ld_nm2, R, d.nm2)));
    MARL_TRY(ln_bwd(c, dad1, d.ld_nm2, c.at(c.e.ZD1, t), d.ld_nm2, c.at(c.e.STD1, t),
                    MARL_P_DEC_LN0W, MARL_P_DEC_LN0B, d.R, d.nm2, s.grads, !first));
    // dL/d(mean message): of the step's input message (step API), or on its way into the encoder of step t-1
    if (t > 0 || (s.sb && s.sb->d_msg))
        MARL_TRY(gemm1(c, gemm_prob(dad1, d.ld_nm2, c.wtB(MARL_P_DEC_W0), c.at(c.e.DMBAR), d.ld_nm, R, d.n_m)));
    if (t == 0) return MARL_OK;
    float* dze2 = c.at(c.e.DZE2) + (size_t)(t - 1) * d.R * d.ld_nm;
    if (c.opt.comm)  // the transpose of the mixing matrix
        MARL_TRY(mix_msg(c, t, c.at(c.e.DMBAR), dze2, d.n_m, 1));
    else  // the message mean is self-adjoint
        MARL_TRY(launch_agg_msg(c.at(c.e.DMBAR), dze2, d.ld_nm, d.na, d.nb, d.n_m, c.st));
    return enc_bwd_rows(s, t - 1, !first, c.DHs(t));
}

static int bwd_loop(BwdState& s) {
    Ctx& c = s.c;
    const Dims& d = c.d;
    const StepBwd* sb = s.sb;
    float* const* grads = s.grads;
    hipStream_t st = c.st;
    const int ns = d.ns;
    const size_t s_nmo = (size_t)d.R * d.ld_dbl;
    // the per-step LayerNorm reductions of the unfused path accumulate into the gradients step
    // by step: nothing of a parameter may still be queued then, so that path does not defer
    if (!c.plan.panels_bwd) {
        MARL_TRY(launch_tn_queue(s.tq, c.rq, st));  // (what the heads queued so far)
        c.rq = nullptr;
        c.tq = nullptr;
    }
    // In an episode the last step's message has no consumer.  A standalone step's new message may have one
    // (the caller's next step, a loss): its encoder runs backward from dL/d(new message) here, ahead of the
    // belief cell of that step, to which it adds dL/dh.
    if (s.enc_last) {
        MARL_TRY(launch_copy2d(sb->g_msg, d.n_m, c.at(c.e.DZE2) + (size_t)(ns - 1) * d.R * d.ld_nm, d.ld_nm, d.R,
                               d.n_m, st));
        MARL_TRY(enc_bwd_rows(s, ns - 1, 0, c.DHs(ns)));
    }
    // with panels dU[:, nf:] (message + embedding columns) comes out of the loop
    s.pln_blocks = c.plan.chain ? panel_chain_blocks(d.na, d.nb) : panel_bwd_blocks((int)d.R);
    for (int t = ns - 1; t >= 0; --t) {
        {   // cells of step t not yet handled inside the previous iteration's panel launch
            LstmBwdBatch lb{};
            int nc = 0;
            if (!s.belief_done) lb.a[nc++] = cell_bwd_args(c, 0, t);
            if (!s.action_done) lb.a[nc++] = cell_bwd_args(c, 1, t);
            lb.rows = d.R;
            if (nc) MARL_TRY(launch_lstm_cell_bwd_batch(lb, nc, st));
        }
        s.action_done = s.belief_done = false;
        float* ddbar = c.at(c.e.DDBAR) + (size_t)t * s_nmo;
        float* ddbar2 = c.at(c.e.DDBAR2) + (size_t)t * s_nmo;
        MARL_TRY(bwd_recurrent(s, t, ddbar, ddbar2));
        if (c.plan.chain)
            MARL_TRY(bwd_step_chain(s, t, ddbar, ddbar2));
        else if (c.plan.panels_bwd)
            MARL_TRY(bwd_step_panels(s, t, ddbar, ddbar2));
        else
            MARL_TRY(bwd_step_rows(s, t, ddbar));
    }
    if (sb) {  // gradients of the step's inputs: what the loop left for step -1
        // (DMBAR = dL/d(mean message) of step 0; the mean is self-adjoint and may run in place: every thread
        // owns one (batch, column) over all agents)
        if (sb->d_msg) {
            if (c.opt.comm)  // d msg goes through M^T, also in place (the kernel holds all agents' inputs in registers)
                MARL_TRY(launch_mix_msg(c.at(c.e.DMBAR), c.at(c.e.DMBAR), d.ld_nm, d.na, d.nb, d.n_m, c.opt.comm, 1, st));
            else
                MARL_TRY(launch_agg_msg(c.at(c.e.DMBAR), c.at(c.e.DMBAR), d.ld_nm, d.na, d.nb, d.n_m, st));
            MARL_TRY(launch_copy2d(c.at(c.e.DMBAR), d.ld_nm, sb->d_msg, d.n_m, d.R, d.n_m, st));
        }
        if (sb->d_h) MARL_TRY(launch_copy2d(c.DHs(0), d.ld_nb, sb->d_h, d.n_b, d.R, d.n_b, st));
        if (sb->d_c) MARL_TRY(launch_copy2d(c.at(c.e.DC), d.ld_nb, sb->d_c, d.n_b, d.R, d.n_b, st));
        if (sb->d_hc) MARL_TRY(launch_copy2d(c.DHCs(0), d.ld_na, sb->d_hc, d.n_a, d.R, d.n_a, st));
        if (sb->d_cc) MARL_TRY(launch_copy2d(c.at(c.e.DCC), d.ld_na, sb->d_cc, d.n_a, d.R, d.n_a, st));
    }
    if (c.plan.panels_bwd) {  // LayerNorm affine gradients of the in-loop layers: one reduction each
        const int64_t nblk = s.pln_blocks;
        MARL_TRY(launch_reduce_affine(c.at(c.e.PLN[0]), nblk * ns, d.n_mo, grads[MARL_P_DEC_LN1W],
                                      grads[MARL_P_DEC_LN1B], 0, st, c.rq));
        MARL_TRY(launch_reduce_affine(c.at(c.e.PLN[1]), nblk * ns, d.nm2, grads[MARL_P_DEC_LN0W],
                                      grads[MARL_P_DEC_LN0B], 0, st, c.rq));
        if (ns > 1) {
            MARL_TRY(launch_reduce_affine(c.at(c.e.PLN[2]), nblk * (ns - 1), d.n_m,
                                          grads[MARL_P_ENC_LN1W], grads[MARL_P_ENC_LN1B], 0, st, c.rq));
            MARL_TRY(launch_reduce_affine(c.at(c.e.PLN[3]), nblk * (ns - 1), d.nm2,
                                          grads[MARL_P_ENC_LN0W], grads[MARL_P_ENC_LN0B], 0, st, c.rq));
        }
    }
    return MARL_OK;
}

// ---- weight gradients of the recurrent chain: one contraction over all steps -------
static int bwd_chain_wgrads(const BwdState& s) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    float* const* grads = s.grads;
    const int64_t NR = d.NR;
    const int ns = d.ns;
    MARL_TRY(tn(c, c.at(c.e.DDBAR), d.ld_dbl, c.at(c.e.AD1, 0), d.ld_nm2, MARL_P_DEC_W1, d.n_mo, d.nm2, NR, grads[MARL_P_DEC_B1]));
    MARL_TRY(tn(c, c.at(c.e.DAD1), d.ld_nm2, c.at(c.e.MBAR, 0), d.ld_nm, MARL_P_DEC_W0, d.nm2, d.n_m, NR, grads[MARL_P_DEC_B0]));
    if (ns > 1 || s.enc_last) {
        // the last step's message is never read in an episode; a standalone step's may be
        const int64_t er = (int64_t)(s.enc_last ? ns : ns - 1) * d.R;
        MARL_TRY(tn(c, c.at(c.e.DZE2), d.ld_nm, c.at(c.e.AE1, 0), d.ld_nm2, MARL_P_ENC_W1, d.n_m, d.nm2, er, grads[MARL_P_ENC_B1]));
        MARL_TRY(tn(c, c.at(c.e.DAE1), d.ld_nm2, c.Hs(1), d.ld_nb, MARL_P_ENC_W0, d.nm2, d.n_b, er, grads[MARL_P_ENC_B0]));
    } else {
        const int enc[] = {MARL_P_ENC_B0, MARL_P_ENC_LN0W, MARL_P_ENC_LN0B, MARL_P_ENC_B1,
                           MARL_P_ENC_LN1W, MARL_P_ENC_LN1B};
        for (int i : enc) MARL_TRY(launch_fill(grads[i], param_meta(d, i).n, 0.f, c.st));
        MARL_TRY(launch_fill(c.gp(MARL_P_ENC_W0), (int64_t)d.nm2 * c.w.ldp[MARL_P_ENC_W0], 0.f, c.st));
        MARL_TRY(launch_fill(c.gp(MARL_P_ENC_W1), (int64_t)d.n_m * c.w.ldp[MARL_P_ENC_W1], 0.f, c.st));
    }
    for (int which = 0; which < 2; ++which) {  // belief cell, action cell: W_ih, then W_hh with the bias
        const int n = which ? d.n_a : d.n_b;
        const int p_ih = which ? MARL_P_LA_WIH : MARL_P_LB_WIH, p_hh = which ? MARL_P_LA_WHH : MARL_P_LB_WHH;
        float* bias = grads[which ? MARL_P_LA_BIH : MARL_P_LB_BIH];
        if (c.plan.g3_tn) {
            // contraction over the rows of the images written by the cell-backward kernels (gate gradients),
            // the forward kernels (U) and the LSTM epilogues (h, h^); bias gradients = column sums of A
            const char* g3 = c.img(which ? c.e.GA3 : c.e.GB3);
            const char* h3 = c.img(which ? c.e.HC3 : c.e.H3);
            if (c.e.tn_cell[which].ok) {
                MARL_TRY(tn3_cell(c, c.e.tn_cell[which], g3, 4 * n, c.img(c.e.U3), d.nin, p_ih, h3, n, p_hh, NR, bias));
            } else {
                MARL_TRY(tn3(c, g3, 4 * n, c.img(c.e.U3), d.nin, p_ih, NR, nullptr));
                MARL_TRY(tn3(c, g3, 4 * n, h3, n, p_hh, NR, bias));
            }
        } else {
            const float* g = c.at(which ? c.e.GA : c.e.GB, 0);
            const int ldg = which ? d.ld_ga : d.ld_gb;
            MARL_TRY(tn(c, g, ldg, c.at(c.e.U, 0), d.ld_nin, p_ih, 4 * n, d.nin, NR));
            MARL_TRY(tn(c, g, ldg, which ? c.HCs(0) : c.Hs(0), which ? d.ld_na : d.ld_nb, p_hh, 4 * n, n, NR, bias));
        }
    }
    return MARL_OK;
}

// ---- dU for all steps, then position embedding and CNN backward -------------------

// dW_l (and db_l) of conv layer l from dZ_l and the layer's input, recomputed from what forward kept (Z_{l-1} +
// statistics, or the image patch): no im2col rows in HBM
static int bwd_conv_wgrad(const BwdState& s, int l, const float* dz, const void* img, int img_u8) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    const int co = d.ch[l + 1];
    CnnWgradArgs w = cnn_wgrad_shape(d, l);
    w.dz = dz;
    w.img = img;
    w.img_u8 = img_u8;
    w.pos = c.POSs(0);
    if (l > 0) {
        w.zin = c.at(c.e.Z[l - 1], 0);
        w.gst = c.at(c.e.GST[l - 1], 0);
        w.gamma = c.wp(4 * (l - 1) + 2);
        w.beta = c.wp(4 * (l - 1) + 3);
    } else if (s.sb) {
        // standalone step: the caller's patches obs [R, C, f, f] are R one-patch images of
        // f x f at position 0 (POSs(0) zeroed by the heads' part) - the gather reads exactly obs[r]
        w.img = s.sb->obs;
        w.img_u8 = 0;
        w.nb = (int)d.R;
        w.H = w.W = d.f;
    } else if (!img) {
        set_error("episode_backward: the image batch of the forward call is needed");
        return MARL_EINVAL;
    }
    // per-workgroup slabs; the launcher places part_b behind the weight slabs
    w.part_w = slab_scratch(c, (size_t)c.e.wgrad[l].blocks_bound * ((size_t)co * d.K[l] + co));
    MARL_TRY(launch_cnn_wgrad(w, c.st));
    return slab_reduce(c, w.part_w, w.part_b, w.blocks, co, d.K[l], 4 * l, s.grads[4 * l + 1]);
}

// the extractor backward from dU[:, :nf], last layer first; leaves dZ_0 in the workspace
static int bwd_cnn_layers(const BwdState& s, const void* img, int img_u8) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    float* const* grads = s.grads;
    hipStream_t st = c.st;
    const int64_t NR = d.NR;
    const float* da = c.at(c.e.DU);
    int64_t ldda = d.ld_nin;
    int chw = 1;
    bool have_dz = false;  // DZ[l] already produced by the fused layer backward of layer l+1
    for (int l = d.L - 1; l >= 0; --l) {
        const int co = d.ch[l + 1];
        const int64_t rows = NR * d.P[l];
        float* dz = c.at(c.e.DZ[l]);
        if (!have_dz) {
            RedQueue* q;
            float* part = part_scratch(c, gn_bwd_blocks(NR, co), co, 0, q);
            MARL_TRY(launch_gn_silu_bwd(da, ldda, chw, c.at(c.e.Z[l], 0), c.at(c.e.GST[l], 0),
                                        c.wp(4 * l + 2), c.wp(4 * l + 3), dz, part, NR, d.P[l], co,
                                        d.grp[l], st));
            MARL_TRY(launch_reduce_affine(part, gn_bwd_blocks(NR, co), co, grads[4 * l + 2],
                                          grads[4 * l + 3], 0, st, q));
        }
        have_dz = false;
        if (c.e.wgrad[l].form) {
            MARL_TRY(bwd_conv_wgrad(s, l, dz, img, img_u8));
        } else {
            MARL_TRY(tn(c, dz, co, c.at(c.e.COLS[l], 0), d.ldk[l], 4 * l, co, d.K[l], rows, grads[4 * l + 1]));
        }
        if (l == 0) break;
        // dZ_l -> dZ_{l-1} in one launch (transposed conv + GroupNorm/SiLU backward)
        CnnDgradArgs g = cnn_dgrad_shape(d, l);
        g.dz = dz;
        g.wt = c.wt(4 * l);
        g.ldwt = p4(co);
        g.zin = c.at(c.e.Z[l - 1], 0);
        g.gst = c.at(c.e.GST[l - 1], 0);
        g.gamma = c.wp(4 * (l - 1) + 2);
        g.beta = c.wp(4 * (l - 1) + 3);
        g.dzin = c.at(c.e.DZ[l - 1]);
        const int nblk = c.e.dgrad[l].rb ? cnn_dgrad_blocks(g) : 0;  // (plan + what is resident on this device)
        if (c.e.dgrad[l].rb && (size_t)nblk * 2 * d.ch[l] <= c.e.part_floats) {
            RedQueue* q;
            g.part = part_scratch(c, nblk, d.ch[l], 0, q);
            MARL_TRY(launch_cnn_dgrad(g, st));
            MARL_TRY(launch_reduce_affine(g.part, nblk, d.ch[l], grads[4 * (l - 1) + 2], grads[4 * (l - 1) + 3], 0,
                                          st, q));
            have_dz = true;
            continue;
        }
        MARL_TRY(gemm1(c, gemm_prob(dz, co, c.wtB(4 * l), c.at(c.e.DCOLS[l]), d.ldk[l], (int)rows, d.K[l])));
        MARL_TRY(launch_col2im(c.at(c.e.DCOLS[l]), d.ldk[l], c.at(c.e.DA[l - 1]), NR,
                               d.hw[l], d.ch[l], st));
        da = c.at(c.e.DA[l - 1]);
        ldda = (int64_t)d.P[l - 1] * d.ch[l];
        chw = 0;
    }
    return MARL_OK;
}

static int bwd_inputs(const BwdState& s, const void* img, int img_u8, float* d_img) {
    const Ctx& c = s.c;
    const Dims& d = c.d;
    float* const* grads = s.grads;
    hipStream_t st = c.st;
    const int64_t NR = d.NR;
    // with the [nf, nin) columns already produced step by step (panels), only the CNN features remain
    if (c.e.g3 && c.plan.panels_bwd) {
        G3Batch g{};
        g.p[0] = g3_prob(c.img(c.e.GB3), 0, c.wt3k(MARL_P_LB_WIH), 0, 4 * d.n_b, c.at(c.e.DU), d.ld_nin, (int)NR,
                         d.nf);
        g3_add_seg(g.p[0], c.img(c.e.GA3), 0, c.wt3k(MARL_P_LA_WIH), 0, 4 * d.n_a);
        g.count = 1;
        MARL_TRY(launch_gemm_nt3(g, st));
    } else {
        GemmProb p = gemm_prob(c.at(c.e.GB, 0), d.ld_gb, c.wtB(MARL_P_LB_WIH),
                               c.at(c.e.DU), d.ld_nin, (int)NR, c.plan.panels_bwd ? d.nf : d.nin);
        gemm_add_seg(p, c.at(c.e.GA, 0), d.ld_ga, c.wtB(MARL_P_LA_WIH));
        MARL_TRY(gemm1(c, p));
    }
    if (c.plan.panels_bwd)  // d(position embedding) = belief share + action share
        MARL_TRY(launch_add2d(c.at(c.e.DDBAR) + d.n_mo, d.ld_dbl, c.at(c.e.DDBAR2) + d.n_mo, d.ld_dbl,
                              c.at(c.e.DU) + d.nf + d.n_mo, d.ld_nin, NR, d.n_d, st));
    MARL_TRY(ln_bwd(c, c.at(c.e.DU) + d.nf + d.n_mo, d.ld_nin, c.at(c.e.ZPOS, 0), d.ld_nd,
                    c.at(c.e.STPOS, 0), MARL_P_POS_LNW, MARL_P_POS_LNB, NR, d.n_d, grads, 0,
                    c.at(c.e.DZPOS), d.ld_nd));
    MARL_TRY(tn(c, c.at(c.e.DZPOS), d.ld_nd, c.at(c.e.NPOS, 0), 4, MARL_P_POS_W, d.n_d, 2, NR, grads[MARL_P_POS_B]));
    MARL_TRY(bwd_cnn_layers(s, img, img_u8));
    if (d_img) {  // dL/d(img): dZ_0 (left in the workspace by the layer loop) back through the crops of every step
        CnnDimgArgs a = cnn_dimg_shape(d);
        a.dz0 = c.at(c.e.DZ[0]);
        a.wt0 = c.wt(0);
        a.ldwt = c.w.ldt[0];
        a.pos = c.POSs(0);
        a.d_img = d_img;
        MARL_TRY(launch_cnn_dimg(a, st));
    }
    return MARL_OK;
}

static int episode_backward(const Ctx& c0, const void* img, int img_u8, const float* g_preds,
                            const float* g_logp, const float* g_values, float* const* grads,
                            const StepBwd* sb = nullptr, float* d_img = nullptr,
                            const float* g_probs = nullptr) {
    BwdState s;
    s.c = c0;
    s.grads = grads;
    s.sb = sb;
    s.enc_last = sb && sb->g_msg;
    Ctx& c = s.c;
    s.rq.reset(c.at(c.e.RED), c.e.red_floats, c.st);
    // 1: the small LayerNorm / GroupNorm affine partials wait for one launch at the end; the
    // weight-gradient slabs (~0.4 GB per iteration in all) are reduced at once, while the
    // Infinity Cache still holds them (2: defer those too - measured slower at C3 / C4: 0.43 GB of
    // slabs come back from HBM).  3 (default): as 1, plus the slabs of at most red_defer_kb KB
    // each (8 MB: larger thresholds lose again at C4) - on small problems (C2: 22 weight gradients) one batched
    // reduction replaces 22 launches: 0.953 -> 0.897 ms per iteration.
    const int defer = tune_get("red_defer", 3);
    if (defer) c.rq = &s.rq;
    if (defer) c.tq = &s.tq;
    c.defer_slabs = defer == 2;
    c.defer_small = defer == 3 ? (size_t)8192 * 1024 : 0;
    for (int i = 0; i < MARL_NPARAMS; ++i)
        if (param_meta(c.d, i).kind != PK_NONE && !grads[i]) {
            set_error("gradient buffer %d is null", i);
            return MARL_EINVAL;
        }
    MARL_TRY(bwd_heads(s, g_preds, g_logp, g_values, g_probs));
    MARL_TRY(bwd_loop(s));
    MARL_TRY(bwd_chain_wgrads(s));
    MARL_TRY(bwd_inputs(s, img, img_u8, d_img));
    if (c.tq) MARL_TRY(launch_tn_queue(s.tq, c.rq, c.st));  // the small weight gradients, one launch
    MARL_TRY(s.rq.flush());
    return unpack_grads(c, grads, s.heads_early ? 2 : 0);
}

}  // namespace marl

// ===========================================================================
// C ABI
// ===========================================================================
using namespace marl;

extern "C" {

int marl_abi_version(void) { return MARL_ABI_VERSION; }

int64_t marl_param_numel(const marl_config* cfg, int index) {
    Dims d;
    if (make_dims(cfg, d) != MARL_OK || index < 0 || index >= MARL_NPARAMS) return -1;
    const ParamMeta m = param_meta(d, index);
    if (m.kind == PK_NONE) return 0;
    return m.kind == PK_VEC ? m.n : (int64_t)m.n * m.k;
}

int marl_workspace_sizes(const marl_config* cfg, int train, size_t* wbytes, size_t* ebytes) {
    Dims d;
    MARL_TRY(make_dims(cfg, d));
    WLayout w;
    make_wlayout(d, w);
    ELayout e;
    make_elayout(d, w, train, e);
    if (wbytes) *wbytes = w.total * sizeof(float);
    if (ebytes) *ebytes = e.total * sizeof(float);
    return MARL_OK;
}

int marl_pack_weights(const marl_config* cfg, const float* const* params_host, void* weights_ws,
                      size_t weights_ws_bytes, void* stream) {
    Dims d;
    MARL_TRY(make_dims(cfg, d));
    if (!params_host || !weights_ws) {
        set_error("null argument");
        return MARL_EINVAL;
    }
    WLayout w;
    make_wlayout(d, w);
    if (weights_ws_bytes < w.total * sizeof(float)) {
        set_error("pack_weights: weights workspace too small (%zu of %zu bytes)", weights_ws_bytes,
                  w.total * sizeof(float));
        return MARL_ESIZE;
    }
    return pack_weights(d, w, params_host, static_cast<float*>(weights_ws),
                        static_cast<hipStream_t>(stream));
}

int marl_patch_gather(const float* img, const int64_t* pos, float* obs, int nb_agents, int batch,
                      int c, int h, int w, int f, void* stream) {
    if (!img || !pos || !obs || nb_agents < 1 || batch < 1 || c < 1 || f < 1 || h < f || w < f) {
        set_error("patch_gather: bad argument");
        return MARL_EINVAL;
    }
    return launch_patch_gather(img, pos, obs, nb_agents, batch, c, h, w, f,
                               static_cast<hipStream_t>(stream));
}

}  // extern "C"

namespace marl {
__global__ void transition_kernel(const int64_t* __restrict__ pos_in,
                                  const int64_t* __restrict__ actions,
                                  int64_t* __restrict__ pos_out, SampleArgs tbl, int rows, int nA,
                                  int H, int W, int f) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    int a = (int)actions[r];
    a = a < 0 ? 0 : (a >= nA ? nA - 1 : a);
    const int64_t p0 = pos_in[r * 2], p1 = pos_in[r * 2 + 1];
    const int64_t q0 = p0 + tbl.table[a][0], q1 = p1 + tbl.table[a][1];
    const bool ok = q0 >= 0 && q0 + f < H && q1 >= 0 && q1 + f < W;
    pos_out[r * 2] = ok ? q0 : p0;
    pos_out[r * 2 + 1] = ok ? q1 : p1;
}
}  // namespace marl

extern "C" {

int marl_transition(const int64_t* pos_in, const int64_t* actions, int64_t* pos_out,
                    const int32_t* table_host, int nb_action, int rows, int h, int w, int f,
                    void* stream) {
    if (!pos_in || !actions || !pos_out || !table_host || nb_action < 1 ||
        nb_action > MARL_MAX_ACTIONS || rows < 1) {
        set_error("transition: bad argument");
        return MARL_EINVAL;
    }
    SampleArgs tbl;
    memset(&tbl, 0, sizeof(tbl));
    for (int j = 0; j < nb_action; ++j) {
        tbl.table[j][0] = table_host[2 * j];
        tbl.table[j][1] = table_host[2 * j + 1];
    }
    hipLaunchKernelGGL(transition_kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), pos_in, actions, pos_out, tbl, rows,
                       nb_action, h, w, f);
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}

// marl_episode_forward (step_probs == nullptr) and marl_episode_forward_probs: the same launches, the latter plus
// one copy of the workspace's PROBS [Ns][R][nA] (what every step's sampling kernel saved) into the caller's tensor
static int episode_forward_all(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                               void* episode_ws, size_t episode_ws_bytes, const void* img, const int64_t* pos0,
                               const float* h0, const float* c0, const float* hc0, const float* cc0,
                               const float* noise, const int64_t* forced_actions, uint64_t rng_seed,
                               uint64_t rng_offset, const void* counters, float* step_preds, float* step_logp,
                               float* step_values, int64_t* step_pos, int64_t* step_actions, float* step_probs,
                               int train, void* stream) {
    Ctx c;
    MARL_TRY(make_ctx(cfg, weights_ws, weights_ws_bytes, episode_ws, episode_ws_bytes, train, stream, c));
    if (!img || !pos0 || !h0 || !c0 || !hc0 || !cc0 || !step_preds || !step_logp || !step_values) {
        set_error("episode_forward: null argument");
        return MARL_EINVAL;
    }
    if (c.d.ns >= 65536) {
        set_error("episode_forward: more than 65535 steps");
        return MARL_ELIMIT;
    }
    const Dims& d = c.d;
    MARL_TRY(launch_i64_to_i32(pos0, c.POSs(0), d.R * 2, c.st));
    MARL_TRY(load_state(c, h0, c0, hc0, cc0, nullptr));
    StepIn in;
    in.img = img;
    in.img_u8 = cfg->img_u8 != 0;
    const SampleIo io{noise, forced_actions, rng_seed, rng_offset, counters, step_pos, step_actions, step_logp, true};
    for (int t = 0; t < d.ns; ++t) {
        SampleArgs a;
        fill_sample_args(c, cfg, t, io, a);
        if (c.plan.chain)
            MARL_TRY(fwd_step_chain(c, t, in, a));
        else if (c.plan.panels)
            MARL_TRY(fwd_step_panels(c, t, in, a));
        else
            MARL_TRY(fwd_step_rows(c, t, in, a));
    }
    MARL_TRY(heads_batched(c, 0, d.NR, step_values, step_preds));
    if (step_probs) MARL_TRY(launch_copy2d(c.PROBSs(0), d.nA, step_probs, d.nA, d.NR, d.nA, c.st));
    return MARL_OK;
}

int marl_episode_forward(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                         void* episode_ws, size_t episode_ws_bytes, const void* img, const int64_t* pos0, const float* h0, const float* c0,
                         const float* hc0, const float* cc0, const float* noise,
                         const int64_t* forced_actions, uint64_t rng_seed, uint64_t rng_offset,
                         const void* counters, float* step_preds, float* step_logp,
                         float* step_values, int64_t* step_pos, int64_t* step_actions, int train,
                         void* stream) {
    return episode_forward_all(cfg, weights_ws, weights_ws_bytes, episode_ws, episode_ws_bytes, img, pos0, h0, c0,
                               hc0, cc0, noise, forced_actions, rng_seed, rng_offset, counters, step_preds,
                               step_logp, step_values, step_pos, step_actions, nullptr, train, stream);
}

int marl_episode_forward_probs(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                               void* episode_ws, size_t episode_ws_bytes, const void* img, const int64_t* pos0,
                               const float* h0, const float* c0, const float* hc0, const float* cc0,
                               const float* noise, const int64_t* forced_actions, uint64_t rng_seed,
                               uint64_t rng_offset, const void* counters, float* step_preds, float* step_logp,
                               float* step_values, int64_t* step_pos, int64_t* step_actions, float* step_probs,
                               int train, void* stream) {
    if (!step_probs) {
        set_error("episode_forward_probs: null step_probs");
        return MARL_EINVAL;
    }
    return episode_forward_all(cfg, weights_ws, weights_ws_bytes, episode_ws, episode_ws_bytes, img, pos0, h0, c0,
                               hc0, cc0, noise, forced_actions, rng_seed, rng_offset, counters, step_preds,
                               step_logp, step_values, step_pos, step_actions, step_probs, train, stream);
}

// the three backward exports: context, gradient table, and - with a d_img, or when the entry's contract requires one
// (need_dimg) - the image-gradient guards, all before anything is enqueued
static int episode_backward_entry(const char* who, bool need_dimg, const marl_config* cfg, void* weights_ws,
                                  size_t weights_ws_bytes, void* episode_ws, size_t episode_ws_bytes, const void* img,
                                  const float* g_preds, const float* g_logp, const float* g_values,
                                  float* const* grads_host, float* d_img, const float* g_probs, void* stream) {
    Ctx c;
    MARL_TRY(make_ctx(cfg, weights_ws, weights_ws_bytes, episode_ws, episode_ws_bytes, 1, stream, c));
    if (!grads_host) {
        set_error("%s: null gradient table", who);
        return MARL_EINVAL;
    }
    if (d_img || need_dimg) {
        if (cfg->img_u8 != 0) {
            set_error("%s: an integer (uint8) image batch has no gradient", who);
            return MARL_EINVAL;
        }
        if (!d_img || !img) {
            set_error("%s: null %s", who, d_img ? "img" : "d_img");
            return MARL_EINVAL;
        }
        if (!cnn_dimg_supported(cnn_dimg_shape(c.d))) {
            set_error("%s: shape outside the image-gradient kernel's range", who);
            return MARL_ELIMIT;
        }
    }
    return episode_backward(c, img, d_img ? 0 : cfg->img_u8 != 0, g_preds, g_logp, g_values, grads_host, nullptr,
                            d_img, g_probs);
}

int marl_episode_backward(const marl_config* cfg, void* weights_ws, size_t weights_ws_bytes,
                          void* episode_ws, size_t episode_ws_bytes, const void* img, const float* g_preds, const float* g_logp,
                          const float* g_values, float* const* grads_host, void* stream) {
    return episode_backward_entry("episode_backward", false, cfg, weights_ws, weights_ws_bytes, episode_ws,
                                  episode_ws_bytes, img, g_preds, g_logp, g_values, grads_host, nullptr, nullptr,
                                  stream);
}

int marl_episode_backward_img(const marl_config* cfg, void* weights_ws, size_t weights_ws_bytes,
                              void* episode_ws, size_t episode_ws_bytes, const void* img, const float* g_preds,
                              const float* g_logp, const float* g_values, float* const* grads_host, float* d_img,
                              void* stream) {
    return episode_backward_entry("episode_backward_img", true, cfg, weights_ws, weights_ws_bytes, episode_ws,
                                  episode_ws_bytes, img, g_preds, g_logp, g_values, grads_host, d_img, nullptr,
                                  stream);
}

int marl_episode_backward_probs(const marl_config* cfg, void* weights_ws, size_t weights_ws_bytes,
                                void* episode_ws, size_t episode_ws_bytes, const void* img, const float* g_preds,
                                const float* g_logp, const float* g_values, float* const* grads_host, float* d_img,
                                const float* g_probs, void* stream) {
    return episode_backward_entry("episode_backward_probs", false, cfg, weights_ws, weights_ws_bytes, episode_ws,
                                  episode_ws_bytes, img, g_preds, g_logp, g_values, grads_host, d_img, g_probs,
                                  stream);
}

int marl_backward_heads_event(void* hip_event) {
    g_installed.heads_event = static_cast<hipEvent_t>(hip_event);
    return MARL_OK;
}

int marl_comm_matrix(const float* m_dev, int nb_agents) {
    if (!m_dev) {
        g_installed.comm = nullptr;
        g_installed.comm_na = 0;
        return MARL_OK;
    }
    if (nb_agents < 1) {
        set_error("comm_matrix: %d agents", nb_agents);
        return MARL_EINVAL;
    }
    if (nb_agents > mix_msg_max_agents()) {
        set_error("comm_matrix: %d agents, the mixing kernel serves at most %d", nb_agents, mix_msg_max_agents());
        return MARL_ELIMIT;
    }
    g_installed.comm = m_dev;
    g_installed.comm_na = nb_agents;
    return MARL_OK;
}

int marl_comm_range(int radius, int metric, int normalize) {
    if (radius < 0) {
        g_installed.range = CommGate{nullptr, -1, 0, 1};
        return MARL_OK;
    }
    if (metric != MARL_COMM_CHEBYSHEV && metric != MARL_COMM_EUCLIDEAN) {
        set_error("comm_range: unknown metric %d", metric);
        return MARL_EINVAL;
    }
    g_installed.range = CommGate{nullptr, radius, metric, normalize != 0};
    return MARL_OK;
}

int marl_policy_explore(float temperature, float eps, int greedy) {
    if (!std::isfinite(temperature) || !(temperature > 0.f)) {
        set_error("policy_explore: temperature %g, need a finite value > 0", (double)temperature);
        return MARL_EINVAL;
    }
    if (!(eps >= 0.f && eps <= 0.5f)) {
        set_error("policy_explore: eps %g outside [0, 0.5]", (double)eps);
        return MARL_EINVAL;
    }
    const bool on = temperature != 1.f || eps != 0.f || greedy != 0;
    g_installed.explore = Explore{on, 1.0f / temperature, 1.0f - eps, eps, greedy != 0};
    return MARL_OK;
}

int marl_class_loss(const float* class_weights_dev, int nb_class, float label_smoothing,
                    const float* step_weights_dev, int nb_steps, int weight_rewards) {
    if (!std::isfinite(label_smoothing) || !(label_smoothing >= 0.f && label_smoothing < 1.f)) {
        set_error("class_loss: label_smoothing %g outside [0, 1)", (double)label_smoothing);
        return MARL_EINVAL;
    }
    if (nb_class < 0 || nb_steps < 0 || (class_weights_dev && nb_class == 0) || (step_weights_dev && nb_steps == 0)) {
        set_error("class_loss: %d class weights / %d step weights: a pointer needs its length, and none is negative",
                  nb_class, nb_steps);
        return MARL_EINVAL;
    }
    const bool on = class_weights_dev || step_weights_dev || label_smoothing != 0.f || weight_rewards != 0;
    g_installed.class_loss = ClassLoss{on, class_weights_dev, nb_class, label_smoothing, step_weights_dev, nb_steps,
                                       weight_rewards != 0};
    return MARL_OK;
}

int marl_soft_targets(const float* q_dev, int batch, int nb_class) {
    if (batch < 0 || nb_class < 0 || (q_dev && (batch == 0 || nb_class == 0)) || (!q_dev && (batch || nb_class))) {
        set_error("soft_targets: a [%d, %d] target tensor: the pointer needs both sizes, and none is negative", batch,
                  nb_class);
        return MARL_EINVAL;
    }
    g_installed.soft = SoftTargets{q_dev, batch, nb_class};
    return MARL_OK;
}

size_t marl_comm_grad_scratch_bytes(const marl_config* cfg) {
    Dims d;
    if (make_dims(cfg, d) != MARL_OK) return 0;
    return (size_t)comm_grad_blocks((int64_t)d.ns * d.nb, nullptr) * d.na * d.na * sizeof(float);
}

int marl_comm_grad(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes, const void* ws,
                   size_t ws_bytes, int nb_steps, float* d_comm, void* scratch, size_t scratch_bytes, void* stream) {
    if (!cfg || !d_comm || !scratch || !weights_ws || !ws) {
        set_error("comm_grad: null argument");
        return MARL_EINVAL;
    }
    const Installed opt = g_installed;
    if (!opt.comm) {
        set_error("comm_grad: no communication matrix installed (marl_comm_matrix)");
        return MARL_EINVAL;
    }
    if (opt.range.radius >= 0) {
        set_error("comm_grad: a communication range is installed - the gradient of a gated base matrix is not "
                  "computed");
        return MARL_EINVAL;
    }
    if (nb_steps < 1) {
        set_error("comm_grad: %d steps", nb_steps);
        return MARL_EINVAL;
    }
    marl_config lay = *cfg;  // the layout of the workspace the backward ran on: an episode's, or ONE step's
    lay.nb_steps = nb_steps;
    Dims d;
    MARL_TRY(make_dims(&lay, d));
    if (opt.comm_na != d.na) {
        set_error("communication matrix is %d x %d but the configuration has %d agents", opt.comm_na, opt.comm_na,
                  d.na);
        return MARL_EINVAL;
    }
    WLayout w;
    make_wlayout(d, w);
    ELayout e;
    make_elayout(d, w, 1, e);
    if (weights_ws_bytes < w.total * sizeof(float) || ws_bytes < e.total * sizeof(float)) {
        set_error("comm_grad: workspace too small for the current configuration / tuning knobs: weights %zu of %zu "
                  "bytes, episode %zu of %zu bytes", weights_ws_bytes, w.total * sizeof(float), ws_bytes,
                  e.total * sizeof(float));
        return MARL_ESIZE;
    }
    const size_t need = (size_t)comm_grad_blocks((int64_t)d.ns * d.nb, nullptr) * d.na * d.na * sizeof(float);
    if (scratch_bytes < need) {
        set_error("comm_grad: scratch of %zu bytes, %zu needed", scratch_bytes, need);
        return MARL_ESIZE;
    }
    if (!comm_grad_supported(d.na, d.n_m, d.nm2, w.ldp[MARL_P_DEC_W0])) {
        set_error("comm_grad: %d agents / message size %d outside the kernel's range", d.na, d.n_m);
        return MARL_ELIMIT;
    }
    const float* W = static_cast<const float*>(weights_ws);
    const float* E = static_cast<const float*>(ws);
    return launch_comm_grad(E + e.DAD1, d.ld_nm2, E + e.MSG, d.ld_nm, W + w.wp[MARL_P_DEC_W0], w.ldp[MARL_P_DEC_W0],
                            d.na, d.nb, d.ns, d.nm2, d.n_m, static_cast<float*>(scratch), d_comm,
                            static_cast<hipStream_t>(stream));
}

int marl_draw_episode(const marl_config* cfg, uint64_t seed, uint64_t offset, const void* counters,
                      int64_t* pos0, float* h0, float* c0, float* hc0, float* cc0, float* noise,
                      void* stream) {
    Dims d;
    MARL_TRY(make_dims(cfg, d));
    if (!pos0 || !h0 || !c0 || !hc0 || !cc0) {
        set_error("draw_episode: null argument");
        return MARL_EINVAL;
    }
    return launch_draw_episode(seed, offset,
                               counters ? &static_cast<const Counters*>(counters)->rng_offset : nullptr,
                               pos0, (int)d.R, d.H, d.W, d.f, h0, c0, d.n_b, hc0, cc0, d.n_a, noise,
                               noise ? d.NR * d.nA : 0, static_cast<hipStream_t>(stream));
}

int marl_counters_set(void* counters, uint64_t rng_offset, int64_t step, float lr, float beta1,
                      float beta2, void* stream) {
    if (!counters || step < 1) {
        set_error("counters_set: bad argument");
        return MARL_EINVAL;
    }
    return launch_counters_set(static_cast<Counters*>(counters), rng_offset, step, lr, beta1, beta2, 0,
                               static_cast<hipStream_t>(stream));
}

int marl_counters_tick(void* counters, float lr, float beta1, float beta2, void* stream) {
    if (!counters) {
        set_error("counters_tick: null block");
        return MARL_EINVAL;
    }
    return launch_counters_set(static_cast<Counters*>(counters), 0, 0, lr, beta1, beta2, 1,
                               static_cast<hipStream_t>(stream));
}

// ---- hipGraph capture / replay -------------------------------------------------------------
int marl_graph_begin(void* stream) {
    if (!stream) {
        set_error("graph_begin: the NULL stream cannot be captured");
        return MARL_EINVAL;
    }
    MARL_HIP_CHECK(hipStreamBeginCapture(static_cast<hipStream_t>(stream), hipStreamCaptureModeThreadLocal));
    return MARL_OK;
}

int marl_graph_end(void* stream, void** graph_exec_out) {
    if (!stream || !graph_exec_out) return MARL_EINVAL;
    hipGraph_t graph = nullptr;
    MARL_HIP_CHECK(hipStreamEndCapture(static_cast<hipStream_t>(stream), &graph));
    hipGraphExec_t exec = nullptr;
    const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) {
        set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e));
        return MARL_EHIP;
    }
    *graph_exec_out = exec;
    return MARL_OK;
}

int marl_graph_launch(void* graph_exec, void* stream) {
    if (!graph_exec) return MARL_EINVAL;
    MARL_HIP_CHECK(hipGraphLaunch(static_cast<hipGraphExec_t>(graph_exec), static_cast<hipStream_t>(stream)));
    return MARL_OK;
}

int marl_graph_destroy(void* graph_exec) {
    if (graph_exec) MARL_HIP_CHECK(hipGraphExecDestroy(static_cast<hipGraphExec_t>(graph_exec)));
    return MARL_OK;
}

// what every loss entry starts with: the dimensions, its own argument check (`bad`, evaluated by the caller), the
// training-layout size check, and the fields of LossCommon - the loss scratch is the last buffer of either
// episode-workspace layout
static int loss_entry(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes, bool bad, const char* who,
                      const float* step_preds, const float* step_values, const int64_t* y, LossCommon& a) {
    Dims d;
    MARL_TRY(make_dims(cfg, d));
    if (bad) {
        set_error("%s: bad argument", who);
        return MARL_EINVAL;
    }
    WLayout w;
    make_wlayout(d, w);
    ELayout e;
    make_elayout(d, w, 1, e);
    if (episode_ws_bytes < e.total * sizeof(float)) {
        set_error("%s: episode workspace too small (%zu of %zu bytes, training layout)", who, episode_ws_bytes,
                  e.total * sizeof(float));
        return MARL_ESIZE;
    }
    const ClassLoss k = g_installed.class_loss;
    if (k.on && ((k.nc != 0 && k.nc != d.nC) || (k.ns != 0 && k.ns != d.ns))) {
        set_error("%s: the installed class-loss options are for %d classes / %d steps, the configuration has %d / %d",
                  who, k.nc, k.ns, d.nC, d.ns);
        return MARL_EINVAL;
    }
    const SoftTargets q = g_installed.soft;
    if (q.q && (q.nb != d.nb || q.nc != d.nC)) {
        set_error("%s: the installed soft targets are [%d, %d], the configuration has batch %d and %d classes", who,
                  q.nb, q.nc, d.nb, d.nC);
        return MARL_EINVAL;
    }
    a.preds = step_preds;
    a.values = step_values;
    a.y = y;
    a.soft_q = q.q;  // (marl_soft_targets; nullptr: the label kernels, as ever)
    a.scratch = static_cast<float*>(episode_ws) + e.LOSS;
    a.ns = d.ns;
    a.na = d.na;
    a.nb = d.nb;
    a.nc = d.nC;
    a.cls = k.on;  // (marl_class_loss; off: the fields keep their neutral defaults and nobody reads them)
    if (k.on) {
        a.cls_w = k.w;
        a.cls_sw = k.sw;
        a.cls_eps = k.eps;
        a.cls_wrew = k.wrew;
    }
    return MARL_OK;
}

// ... and the fields of LossGradArgs (after loss_entry: ld_gp is the class count)
static void fill_loss_grads(LossGradArgs& a, const marl_config* cfg, const float* step_logp, const float* step_probs,
                            float entropy_coef, float* g_preds, float* g_logp, float* g_values, float* g_probs,
                            float* scalars_out) {
    a.logp = step_logp;
    a.g_preds = g_preds;
    a.ld_gp = a.nc;
    a.g_logp = g_logp;
    a.g_values = g_values;
    a.scalars = scalars_out;
    a.probs = step_probs;
    a.g_probs = g_probs;
    a.n_act = cfg->nb_action;
    a.entropy_coef = entropy_coef;
}

// marl_a2c_loss_fwd_bwd (step_probs == nullptr) and marl_a2c_loss_entropy_fwd_bwd
static int a2c_loss_all(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes, bool bad, const char* who,
                        const float* step_preds, const float* step_logp, const float* step_values, const int64_t* y,
                        float gamma, const float* step_probs, float entropy_coef, float* g_preds, float* g_logp,
                        float* g_values, float* g_probs, float* scalars_out, double* adv_stats, int phase,
                        void* stream) {
    LossArgs a;
    MARL_TRY(loss_entry(cfg, episode_ws, episode_ws_bytes,
                        bad || !episode_ws || !step_preds || !step_logp || !step_values || !y || !scalars_out ||
                            !adv_stats || phase < 0 || phase > 2,
                        who, step_preds, step_values, y, a));
    fill_loss_grads(a, cfg, step_logp, step_probs, entropy_coef, g_preds, g_logp, g_values, g_probs, scalars_out);
    a.adv_stats = adv_stats;
    a.gamma = gamma;
    a.phase = phase;
    return launch_loss(a, static_cast<hipStream_t>(stream));
}

int marl_a2c_loss_fwd_bwd(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes,
                          const float* step_preds,
                          const float* step_logp, const float* step_values, const int64_t* y,
                          float gamma, float* g_preds, float* g_logp, float* g_values,
                          float* scalars_out, double* adv_stats, int phase, void* stream) {
    return a2c_loss_all(cfg, episode_ws, episode_ws_bytes, false, "a2c_loss", step_preds, step_logp, step_values, y,
                        gamma, nullptr, 0.f, g_preds, g_logp, g_values, nullptr, scalars_out, adv_stats, phase,
                        stream);
}

int marl_a2c_loss_entropy_fwd_bwd(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes,
                                  const float* step_preds, const float* step_logp, const float* step_values,
                                  const int64_t* y, float gamma, const float* step_probs, float entropy_coef,
                                  float* g_preds, float* g_logp, float* g_values, float* g_probs,
                                  float* scalars_out, double* adv_stats, int phase, void* stream) {
    return a2c_loss_all(cfg, episode_ws, episode_ws_bytes, !step_probs || !g_probs || !(entropy_coef >= 0.f),
                        "a2c_loss_entropy", step_preds, step_logp, step_values, y, gamma, step_probs, entropy_coef,
                        g_preds, g_logp, g_values, g_probs, scalars_out, adv_stats, phase, stream);
}

int marl_advantages(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes, const float* step_preds,
                    const float* step_values, const int64_t* y, float gamma, float lam, float* advn, float* ret,
                    double* adv_stats, int phase, void* stream) {
    AdvArgs a;
    MARL_TRY(loss_entry(cfg, episode_ws, episode_ws_bytes,
                        !episode_ws || !step_preds || !step_values || !y || !advn || !ret || !adv_stats ||
                            phase < 0 || phase > 2 || !(lam >= 0.f && lam <= 1.f),
                        "advantages", step_preds, step_values, y, a));
    a.advn = advn;
    a.ret = ret;
    a.adv_stats = adv_stats;
    a.gamma = gamma;
    a.lam = lam;
    a.phase = phase;
    return launch_advantages(a, static_cast<hipStream_t>(stream));
}

int marl_ppo_loss_fwd_bwd(const marl_config* cfg, void* episode_ws, size_t episode_ws_bytes,
                          const float* step_preds, const float* step_logp, const float* step_values,
                          const int64_t* y, const float* old_logp, const float* advn, const float* ret,
                          float clip_eps, const float* step_probs, float entropy_coef, float* g_preds, float* g_logp,
                          float* g_values, float* g_probs, float* scalars_out, void* stream) {
    PpoArgs a;
    MARL_TRY(loss_entry(cfg, episode_ws, episode_ws_bytes,
                        !episode_ws || !step_preds || !step_logp || !step_values || !y || !old_logp || !advn ||
                            !ret || !scalars_out || !(clip_eps > 0.f) ||
                            (step_probs == nullptr) != (g_probs == nullptr) ||
                            (step_probs && !(entropy_coef >= 0.f)),
                        "ppo_loss", step_preds, step_values, y, a));
    fill_loss_grads(a, cfg, step_logp, step_probs, entropy_coef, g_preds, g_logp, g_values, g_probs, scalars_out);
    a.old_logp = old_logp;
    a.advn = advn;
    a.ret = ret;
    a.clip_eps = clip_eps;
    return launch_ppo_loss(a, static_cast<hipStream_t>(stream));
}

int marl_grad_clip(float* grads, int64_t n, float max_norm, float grad_scale, float* norm_out, void* scratch,
                   size_t scratch_bytes, void* stream) {
    if (!grads || n < 0 || !(max_norm > 0.f) || !(grad_scale > 0.f) || !norm_out || !scratch ||
        (reinterpret_cast<uintptr_t>(scratch) & 7) != 0) {
        set_error("grad_clip: bad argument");
        return MARL_EINVAL;
    }
    if (scratch_bytes < MARL_GRAD_CLIP_SCRATCH_BYTES) {
        set_error("grad_clip: scratch too small (%zu of %d bytes)", scratch_bytes, MARL_GRAD_CLIP_SCRATCH_BYTES);
        return MARL_ESIZE;
    }
    return launch_grad_clip(grads, n, max_norm, grad_scale, norm_out, static_cast<double*>(scratch),
                            static_cast<hipStream_t>(stream));
}

int marl_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                   int64_t step, float lr, float beta1, float beta2, float eps, float grad_scale,
                   const void* counters, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || n < 0 || step < 1) {
        set_error("adam: bad argument");
        return MARL_EINVAL;
    }
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    return launch_adam(params, grads, exp_avg, exp_avg_sq, n, (float)((double)lr / bc1),
                       (float)(1.0 / sqrt(bc2)), beta1, beta2, eps, grad_scale,
                       static_cast<hipStream_t>(stream), static_cast<const Counters*>(counters));
}

}  // extern "C"

// marl_step_forward (train = 0) and marl_step_forward_train (train = 1: the activations stay in the
// one-step training layout for marl_step_backward).  Same launches either way: the outputs are identical.
static int step_forward(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes, void* episode_ws,
                        size_t episode_ws_bytes, const float* obs, const float* msg, const float* norm_pos,
                        const float* h, const float* cc_, const float* hc, const float* cca, float* probs,
                        float* values, float* preds, float* new_msg, float* h_out, float* c_out, float* hc_out,
                        float* cc_out, const float* noise, uint64_t rng_seed, uint64_t rng_offset,
                        int64_t* actions_out, float* logp_out, int train, void* stream) {
    if (g_installed.range.radius >= 0) {  // (before anything is enqueued)
        set_error("step_forward: a communication range is installed - a single step has no integer positions of "
                  "the emission step; run the fused episode");
        return MARL_EINVAL;
    }
    Ctx c;
    MARL_TRY(make_ctx(cfg, weights_ws, weights_ws_bytes, episode_ws, episode_ws_bytes, train, stream, c));
    if (!obs || !msg || !norm_pos || !h || !cc_ || !hc || !cca || !probs || !values || !preds ||
        !new_msg || !h_out || !c_out || !hc_out || !cc_out) {
        set_error("step_forward: null argument");
        return MARL_EINVAL;
    }
    const Dims& d = c.d;
    MARL_TRY(load_state(c, h, cc_, hc, cca, msg));
    StepIn in;
    in.obs = obs;
    in.npos = norm_pos;
    MARL_TRY(step_core(c, 0, in));
    SampleIo io;  // (left empty: probabilities only - the behaviour policy's under exploration controls)
    if (actions_out && logp_out)  // also sample (positions of the scratch slot are unused)
        io = SampleIo{noise, nullptr, rng_seed, rng_offset, nullptr, nullptr, actions_out, logp_out, false};
    SampleArgs a;
    fill_sample_args(c, cfg, 0, io, a);
    a.probs = probs;
    MARL_TRY(launch_sample(a, c.st, c.opt.explore.on));
    MARL_TRY(heads_batched(c, 0, d.R, values, preds));
    MARL_TRY(launch_copy2d(c.MSGs(1), d.ld_nm, new_msg, d.n_m, d.R, d.n_m, c.st));
    MARL_TRY(launch_copy2d(c.Hs(1), d.ld_nb, h_out, d.n_b, d.R, d.n_b, c.st));
    MARL_TRY(launch_copy2d(c.Cs(1), d.ld_nb, c_out, d.n_b, d.R, d.n_b, c.st));
    MARL_TRY(launch_copy2d(c.HCs(1), d.ld_na, hc_out, d.n_a, d.R, d.n_a, c.st));
    MARL_TRY(launch_copy2d(c.CCs(1), d.ld_na, cc_out, d.n_a, d.R, d.n_a, c.st));
    if (train)  // the softmax backward reads the probabilities (the sampled action is in ACTs(0) already)
        MARL_TRY(launch_copy2d(probs, d.nA, c.PROBSs(0), d.nA, d.R, d.nA, c.st));
    return MARL_OK;
}

extern "C" {

int marl_step_forward(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                      void* episode_ws, size_t episode_ws_bytes, const float* obs, const float* msg, const float* norm_pos, const float* h,
                      const float* cc_, const float* hc, const float* cca, float* probs,
                      float* values, float* preds, float* new_msg, float* h_out, float* c_out,
                      float* hc_out, float* cc_out, const float* noise, uint64_t rng_seed,
                      uint64_t rng_offset, int64_t* actions_out, float* logp_out, void* stream) {
    return step_forward(cfg, weights_ws, weights_ws_bytes, episode_ws, episode_ws_bytes, obs, msg, norm_pos, h, cc_,
                        hc, cca, probs, values, preds, new_msg, h_out, c_out, hc_out, cc_out, noise, rng_seed,
                        rng_offset, actions_out, logp_out, 0, stream);
}

int marl_step_forward_train(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes,
                            void* step_ws, size_t step_ws_bytes, const float* obs, const float* msg,
                            const float* norm_pos, const float* h, const float* c, const float* hc,
                            const float* cc, float* probs, float* values, float* preds, float* new_msg,
                            float* h_out, float* c_out, float* hc_out, float* cc_out, const float* noise,
                            uint64_t rng_seed, uint64_t rng_offset, int64_t* actions_out, float* logp_out,
                            void* stream) {
    if (!cfg) {
        set_error("step_forward_train: null configuration");
        return MARL_EINVAL;
    }
    marl_config one = *cfg;  // the step workspace has the training layout of ONE step
    one.nb_steps = 1;
    return step_forward(&one, weights_ws, weights_ws_bytes, step_ws, step_ws_bytes, obs, msg, norm_pos, h, c, hc, cc,
                        probs, values, preds, new_msg, h_out, c_out, hc_out, cc_out, noise, rng_seed, rng_offset,
                        actions_out, logp_out, 1, stream);
}

int marl_step_backward(const marl_config* cfg, void* weights_ws, size_t weights_ws_bytes, void* step_ws,
                       size_t step_ws_bytes, const float* obs, const float* g_probs, const float* g_logp,
                       const float* g_values, const float* g_preds, const float* g_msg, const float* g_h,
                       const float* g_c, const float* g_hc, const float* g_cc, float* const* grads_host,
                       float* d_msg, float* d_h, float* d_c, float* d_hc, float* d_cc, void* stream) {
    if (!cfg) {
        set_error("step_backward: null configuration");
        return MARL_EINVAL;
    }
    if (g_installed.range.radius >= 0) {  // (before anything is enqueued)
        set_error("step_backward: a communication range is installed - a single step has no integer positions of "
                  "the emission step; run the fused episode");
        return MARL_EINVAL;
    }
    marl_config one = *cfg;
    one.nb_steps = 1;
    Ctx c;
    MARL_TRY(make_ctx(&one, weights_ws, weights_ws_bytes, step_ws, step_ws_bytes, 1, stream, c));
    if (!grads_host || !obs) {
        set_error("step_backward: null gradient table or observation");
        return MARL_EINVAL;
    }
    StepBwd sb;
    sb.obs = obs;
    sb.g_probs = g_probs;
    sb.g_msg = g_msg;
    sb.g_h = g_h;
    sb.g_c = g_c;
    sb.g_hc = g_hc;
    sb.g_cc = g_cc;
    sb.d_msg = d_msg;
    sb.d_h = d_h;
    sb.d_c = d_c;
    sb.d_hc = d_hc;
    sb.d_cc = d_cc;
    return episode_backward(c, nullptr, 0, g_preds, g_logp, g_values, grads_host, &sb);
}

// test hook: where a named activation of step t lives inside episode_ws (float offset, ld)
int marl_debug_buffer(const marl_config* cfg, int train, const char* name, int t,
                      int64_t* offset_floats, int* ld) {
    Dims d;
    MARL_TRY(make_dims(cfg, d));
    WLayout w;
    make_wlayout(d, w);
    ELayout e;
    make_elayout(d, w, train, e);
    if (!name || !offset_floats || !ld || t < 0 || t > d.ns) return MARL_EINVAL;
    const size_t R = (size_t)d.R;
    const int ts = train ? t : 0;
    auto set = [&](size_t off, int l) {
        *offset_floats = (int64_t)off;
        *ld = l;
        return MARL_OK;
    };
    if (!strncmp(name, "WP", 2) || !strncmp(name, "WT", 2)) {  // weights workspace: packed / transposed copy of parameter <idx>
        const int idx = atoi(name + 2);
        if (name[2] == 'F') {  // WPF<idx> / WTF<idx>: its fragment-order copy (ld: the 16-deep groups per tile)
            const int fi = atoi(name + 3);
            const size_t off = fi >= 0 && fi < MARL_NPARAMS ? (name[1] == 'P' ? w.wpf[fi] : w.wtf[fi]) : 0;
            if (!off) {
                set_error("parameter %d has no fragment-order copy", fi);
                return MARL_EINVAL;
            }
            return set(off, name[1] == 'P' ? w.gpf[fi] : w.gtf[fi]);
        }
        if (idx < 0 || idx >= MARL_NPARAMS || param_meta(d, idx).kind == PK_NONE) {
            set_error("no parameter %d", idx);
            return MARL_EINVAL;
        }
        return name[1] == 'P' ? set(w.wp[idx], w.ldp[idx]) : set(w.wt[idx], w.ldt[idx]);
    }
    if (!strcmp(name, "U")) return set(e.U.at(ts), d.ld_nin);
    if (!strcmp(name, "H")) return set(e.H + (size_t)t * R * d.ld_nb, d.ld_nb);
    if (!strcmp(name, "C")) return set(e.C + (size_t)t * R * d.ld_nb, d.ld_nb);
    if (!strcmp(name, "HC")) return set(e.HC + (size_t)t * R * d.ld_na, d.ld_na);
    if (!strcmp(name, "CC")) return set(e.CC + (size_t)t * R * d.ld_na, d.ld_na);
    if (!strcmp(name, "MSG")) return set(e.MSG + (size_t)t * R * d.ld_nm, d.ld_nm);
    if (!strcmp(name, "PROBS")) return set(e.PROBS + (size_t)t * R * d.nA, d.nA);
    if (!strcmp(name, "COLS0")) {
        if (e.fwd.which && !e.keeps_cols[0]) {
            set_error("COLS0 is not materialised for this shape (fused CNN kernels)");
            return MARL_EINVAL;
        }
        return set(e.COLS[0].at(e.COLS[0].stride ? ts : 0), d.ldk[0]);
    }
    if (!strcmp(name, "Z0")) return set(e.Z[0].at(ts), d.ch[1]);
    if (!strcmp(name, "GB")) return set(e.GB.at(ts), d.ld_gb);
    if (train) {
        if (!strcmp(name, "DU")) return set(e.DU + (size_t)t * R * d.ld_nin, d.ld_nin);
        if (!strcmp(name, "DH")) return set(e.DH + (size_t)t * R * d.ld_nb, d.ld_nb);
        if (!strcmp(name, "DHC")) return set(e.DHC + (size_t)t * R * d.ld_na, d.ld_na);
    }
    set_error("unknown debug buffer %s", name);
    return MARL_EINVAL;
}

int marl_plan_query(const marl_config* cfg, int train, const char* key, int* value) {
    Dims d;
    MARL_TRY(make_dims(cfg, d));
    if (!key || !value) return MARL_EINVAL;
    // the plan as make_ctx builds it (a witness answers from the routine that decides)
    WLayout w;
    make_wlayout(d, w);
    ELayout e;
    make_elayout(d, w, train, e);
    const Plan plan = make_plan(d, w, e, g_installed);
    if (!strcmp(key, "g3")) *value = e.g3;
    else if (!strcmp(key, "g3_model")) *value = g3_model_ok(d);
    else if (!strcmp(key, "g3_lstm")) *value = plan.g3_lstm;
    else if (!strcmp(key, "g3_tn")) *value = plan.g3_tn;
    else if (!strcmp(key, "lstm_plan")) *value = plan.lstm_plan;
    else if (!strcmp(key, "small_r")) *value = plan.lstm_plan == 3 || plan.lstm_plan == 4;  // one of the gate-split plans
    else if (!strcmp(key, "g3_tn_cell"))  // both weight gradients of a cell from one launch (gemm_tn3_cell_kernel)
        *value = plan.g3_tn_cell;
    else if (!strcmp(key, "g3_tn_pipe")) *value = plan.g3_tn_pipe;  // only where the image weight gradients run
    else if (!strcmp(key, "wgrad3")) {  // a conv weight gradient of this model runs on the bf16 pipe (cin >= 16)
        *value = 0;
        for (int l = 0; l < d.L; ++l)
            if (e.wgrad[l].form == 3) *value = 1;
    }
    // what the CNN launchers do with this shape (their own routines, host arithmetic only; see marl_hip.h)
    else if (!strncmp(key, "cnn_fwd", 7)) {
        const CnnFwdPlan& p = e.fwd;  // the plan of step_cnn's launch (unfused path: all 0)
        if (!strcmp(key, "cnn_fwd")) *value = p.which;
        else if (!strcmp(key, "cnn_fwd_rb")) *value = p.rb;
        else if (!strcmp(key, "cnn_fwd_blocks")) *value = p.blocks;
        else {
            set_error("unknown plan key %s", key);
            return MARL_EINVAL;
        }
    }
    else if (!strncmp(key, "cnn_dgrad_rb", 12) || !strncmp(key, "cnn_wgrad_", 10)) {
        const bool dg = key[4] == 'd';
        const char* rest = key + (dg ? 12 : 10);
        int field = 0;  // wgrad: 1 = rb, 2 = chunks, 3 = blocks
        if (!dg) {
            if (!strncmp(rest, "rb", 2)) field = 1, rest += 2;
            else if (!strncmp(rest, "chunks", 6)) field = 2, rest += 6;
            else if (!strncmp(rest, "blocks", 6)) field = 3, rest += 6;
        }
        const int l = (rest[0] >= '0' && rest[0] <= '9' && !rest[1]) ? rest[0] - '0' : -1;
        if ((!dg && !field) || l < (dg ? 1 : 0) || l >= d.L) {
            set_error("unknown plan key %s (layers %d..%d)", key, dg ? 1 : 0, d.L - 1);
            return MARL_EINVAL;
        }
        // (the backward plans do not depend on `train`: the layout at hand answers for the training one)
        if (dg)
            *value = e.dgrad[l].rb;
        else {
            const CnnWgradPlan& p = e.wgrad[l];
            *value = field == 1 ? p.rb : field == 2 ? p.chunks : p.blocks;
        }
    }
    else if (!strcmp(key, "comm")) *value = plan.comm;
    else if (!strcmp(key, "comm_range")) *value = plan.comm_range;
    else if (!strcmp(key, "panel_chain")) *value = plan.chain;
    else if (!strcmp(key, "panel_sample")) *value = plan.panel_sample;
    else if (!strcmp(key, "panel_static")) *value = plan.panel_static;
    else if (!strcmp(key, "explore")) *value = plan.explore;
    else if (!strcmp(key, "class_loss")) *value = plan.class_loss;
    else if (!strcmp(key, "soft_targets")) *value = plan.soft_targets;
    else if (!strcmp(key, "explore_form")) *value = plan.explore_form;
    else if (!strcmp(key, "comm_form")) *value = plan.comm_form;
    else {
        set_error("unknown plan key %s", key);
        return MARL_EINVAL;
    }
    return MARL_OK;
}

}  // extern "C"
namespace marl {
__global__ void normalize_positions_kernel(const int64_t* __restrict__ pos, float* __restrict__ out,
                                           int rows, int H, int W) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    out[r * 2] = (float)pos[r * 2] / (float)H;
    out[r * 2 + 1] = (float)pos[r * 2 + 1] / (float)W;
}
}  // namespace marl
extern "C" {

int marl_normalize_positions(const int64_t* pos, float* out, int rows, int h, int w, void* stream) {
    if (!pos || !out || rows < 1 || h < 1 || w < 1) {
        set_error("normalize_positions: bad argument");
        return MARL_EINVAL;
    }
    hipLaunchKernelGGL(normalize_positions_kernel, dim3((unsigned)cdiv(rows, 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), pos, out, rows, h, w);
    MARL_LAUNCH_CHECK();
    return MARL_OK;
}

int marl_profile_begin(int kernel_class, int max_launches) {
    if (kernel_class < 0 || kernel_class >= kProfClasses || max_launches < 1) return MARL_EINVAL;
    return profile_begin(kernel_class, max_launches);
}
int marl_profile_end(double* total_ms, int* launches) { return profile_end(total_ms, launches); }

// ---- kernel-level entry points -------------------------------------------------------
int marl_gemm_nt(const float* a, int lda, const float* b, int ldb, const float* bias, float* c,
                 int ldc, int m, int n, int k, int accumulate, void* stream) {
    GemmBatch bt{};
    bt.p[0] = gemm_prob(a, lda, gemm_b(b, ldb, k), c, ldc, m, n, bias, accumulate);  // never an image
    bt.count = 1;
    return launch_gemm_nt(bt, static_cast<hipStream_t>(stream));
}

size_t marl_gemm_weight_image_bytes(int n, int k) { return split_image_floats(n, k) * sizeof(float); }

int marl_gemm_nt_weights(const float* a, int lda, const float* b, int ldb, const float* bias, float* c,
                         int ldc, int m, int n, int k, int accumulate, void* image_scratch, void* stream) {
    if (!b || !image_scratch || n < 1 || k < 1 || ldb < k) {
        set_error("gemm_nt_weights: bad argument");
        return MARL_EINVAL;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    SplitBatch sb{};
    sb.d[0] = SplitDesc{b, image_scratch, n, k, ldb, (k + 31) / 32};
    sb.count = 1;
    MARL_TRY(launch_split_weights(sb, st));
    GemmBatch bt{};
    bt.p[0] = gemm_prob(a, lda, GemmB{b, ldb, k, image_scratch, (k + 31) / 32}, c, ldc, m, n, bias, accumulate);
    bt.count = 1;
    return launch_gemm_nt(bt, st);
}

size_t marl_gemm_tn_scratch(int ni, int nj, int64_t rows) { return gemm_tn_scratch_bytes(ni, nj, rows); }

int marl_gemm_tn(const float* a, int lda, const float* b, int ldb, float* c, int ldc, int ni, int nj,
                 int64_t rows, float* scratch, size_t scratch_bytes, void* stream) {
    return launch_gemm_tn(a, lda, b, ldb, c, ldc, ni, nj, rows, scratch, scratch_bytes,
                          static_cast<hipStream_t>(stream));
}

static CnnWgradArgs wgrad_api_args(int64_t rows, int nb, int c_img, int h, int w, int cin, int cout,
                                   int hin, int groups, int first) {
    CnnWgradArgs g{};
    g.rows = rows;
    g.first = first;
    g.nb = nb;
    g.c_img = c_img;
    g.H = h;
    g.W = w;
    g.cin = cin;
    g.cout = cout;
    g.hin = hin;
    g.hout = (hin - 1) / 2 + 1;
    g.P = g.hout * g.hout;
    g.G = groups > 0 ? groups : 1;
    g.K = 9 * cin;
    return g;
}

size_t marl_cnn_wgrad_scratch(int64_t rows, int cin, int cout, int hin, int groups, int first) {
    CnnWgradArgs g = wgrad_api_args(rows, 1, cin, hin + 1, hin + 1, cin, cout, hin, groups, first);
    return (size_t)cnn_wgrad_plan(g).blocks_bound * ((size_t)cout * 9 * cin + cout) * sizeof(float);
}

int marl_cnn_wgrad(const float* dz, const void* img, int img_u8, const int32_t* pos,
                   const float* zin, const float* gst, const float* gamma, const float* beta,
                   int64_t rows, int nb, int c_img, int h, int w, int cin, int cout, int hin,
                   int groups, float* dw, float* db, float* scratch, size_t scratch_bytes,
                   void* stream) {
    const int first = zin == nullptr;
    if (!dz || !dw || !db || !scratch || rows < 1 || cin < 1 || cout < 1 || hin < 1 ||
        (first ? (!img || !pos || nb < 1) : (!gst || !gamma || !beta))) {
        set_error("cnn_wgrad: bad argument");
        return MARL_EINVAL;
    }
    CnnWgradArgs g = wgrad_api_args(rows, nb, c_img, h, w, cin, cout, hin, groups, first);
    const CnnWgradPlan plan = cnn_wgrad_plan(g);
    if (!plan.form) {
        set_error("cnn_wgrad: shape outside the kernel's range (cin %d cout %d hin %d)", cin, cout, hin);
        return MARL_ELIMIT;
    }
    if (scratch_bytes < (size_t)plan.blocks_bound * ((size_t)cout * 9 * cin + cout) * sizeof(float)) {
        set_error("cnn_wgrad: scratch too small");
        return MARL_ESIZE;
    }
    g.dz = dz;
    g.img = img;
    g.img_u8 = img_u8;
    g.pos = pos;
    g.zin = zin;
    g.gst = gst;
    g.gamma = gamma;
    g.beta = beta;
    g.part_w = scratch;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MARL_TRY(launch_cnn_wgrad(g, st));
    return launch_slab_reduce(g.part_w, (int64_t)cout * g.K, g.blocks, dw, g.K, cout, g.K, g.part_b, db, st);
}

int marl_tune(const char* key, int value) {
    if (!key) return MARL_EINVAL;
    return tune_set(key, value);
}

int marl_tune_get(const char* key, int dflt) { return key ? tune_get(key, dflt) : dflt; }

int marl_ln_silu_fwd(const float* z, int ldz, const float* gamma, const float* beta, float* out,
                     int ldo, float* stats, int m, int n, void* stream) {
    return launch_ln_silu_fwd(z, ldz, gamma, beta, out, ldo, stats, m, n,
                              static_cast<hipStream_t>(stream));
}

// ---- kernel-level hooks of the row passes (include/marl_hip_rowops.h; not part of the versioned ABI) ----
int marl_ln_silu_bwd(const float* da, int ldda, const float* g, int ldg, int kin, const float* w1t, int ldw,
                     const float* z, int ldz, const float* stats, const float* gamma, const float* beta,
                     float* dz, int lddz, float* dgamma, float* dbeta, float* scratch, size_t scratch_bytes,
                     int m, int n, void* stream) {
    if (!z || !stats || !gamma || !beta || !dz || !dgamma || !dbeta || !scratch || m < 0 || n < 1 ||
        (kin == 0 ? !da : (!g || !w1t))) {
        set_error("marl_ln_silu_bwd: null pointer or bad size");
        return MARL_EINVAL;
    }
    if (n > 2048) {
        set_error("LayerNorm width %d > 2048 unsupported", n);
        return MARL_ELIMIT;
    }
    if (m == 0) return MARL_OK;
    const int blocks = ln_bwd_blocks(m, n);
    if (scratch_bytes < (size_t)blocks * 2 * n * sizeof(float)) {
        set_error("marl_ln_silu_bwd: scratch too small (%zu bytes needed)", (size_t)blocks * 2 * n * sizeof(float));
        return MARL_ESIZE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (kin == 0)
        MARL_TRY(launch_ln_silu_bwd(da, ldda, z, ldz, stats, gamma, beta, dz, lddz, scratch, m, n, st));
    else
        MARL_TRY(launch_ln_silu_bwd_rank(g, ldg, kin, w1t, ldw, z, ldz, stats, gamma, beta, dz, lddz, scratch, m,
                                         n, st));
    return launch_reduce_affine(scratch, blocks, n, dgamma, dbeta, 0, st, nullptr);
}

int marl_gn_silu_bwd(const float* da, int64_t ldda, int da_chw, const float* z, const float* stats,
                     const float* gamma, const float* beta, float* dz, float* dgamma, float* dbeta,
                     float* scratch, size_t scratch_bytes, int64_t rows, int p, int c, int groups,
                     void* stream) {
    if (!da || !z || !stats || !gamma || !beta || !dz || !dgamma || !dbeta || !scratch || rows < 0 || p < 1 ||
        c < 1 || groups < 1 || c % groups) {
        set_error("marl_gn_silu_bwd: null pointer or bad size");
        return MARL_EINVAL;
    }
    if (rows == 0) return MARL_OK;
    const int blocks = gn_bwd_blocks(rows, c);
    if (scratch_bytes < (size_t)blocks * 2 * c * sizeof(float)) {
        set_error("marl_gn_silu_bwd: scratch too small (%zu bytes needed)", (size_t)blocks * 2 * c * sizeof(float));
        return MARL_ESIZE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    MARL_TRY(launch_gn_silu_bwd(da, ldda, da_chw, z, stats, gamma, beta, dz, scratch, rows, p, c, groups, st));
    return launch_reduce_affine(scratch, blocks, c, dgamma, dbeta, 0, st, nullptr);
}

// ---- kernel-level hooks of the conv backward (include/marl_hip_cnnops.h; not part of the versioned ABI) ----
static CnnDgradArgs dgrad_api_args(int64_t rows, int cin, int cout, int hin, int groups) {
    CnnDgradArgs g{};
    g.rows = rows;
    g.cin = cin;
    g.cout = cout;
    g.hin = hin;
    g.hout = (hin - 1) / 2 + 1;
    g.P = g.hout * g.hout;
    g.Pin = hin * hin;
    g.G = groups;
    return g;
}
// the plan for a caller's raw shapes (rb 0: bad sizes, or not covered)
static CnnDgradPlan dgrad_api_plan(int64_t rows, int cin, int cout, int hin, int groups) {
    if (rows < 1 || cin < 1 || cout < 1 || hin < 1 || groups < 1) return CnnDgradPlan{};
    CnnDgradArgs g = dgrad_api_args(rows, cin, cout, hin, groups);
    return cnn_dgrad_plan(g);
}

size_t marl_cnn_dgrad_scratch(int64_t rows, int cin, int cout, int hin, int groups) {
    return (size_t)dgrad_api_plan(rows, cin, cout, hin, groups).chunks * 2 * cin * sizeof(float);
}

int marl_cnn_dgrad(const float* dz, const float* wt, int ldwt, const float* zin, const float* gst,
                   const float* gamma, const float* beta, float* dzin, float* dgamma, float* dbeta, float* scratch,
                   size_t scratch_bytes, int64_t rows, int cin, int cout, int hin, int groups, void* stream) {
    auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    if (!dz || !wt || !zin || !gst || !gamma || !beta || !dzin || !dgamma || !dbeta || !scratch || rows < 1 ||
        cin < 1 || cout < 1 || hin < 1 || groups < 1 || ldwt < cout || (ldwt & 3) || misaligned(dz) ||
        misaligned(wt) || misaligned(zin) || misaligned(dzin)) {
        set_error("marl_cnn_dgrad: null or misaligned pointer, or bad size");
        return MARL_EINVAL;
    }
    if (!dgrad_api_plan(rows, cin, cout, hin, groups).rb) {
        set_error("marl_cnn_dgrad: shape outside the fused kernel's range (cin %d cout %d hin %d groups %d)", cin, cout,
                  hin, groups);
        return MARL_ELIMIT;
    }
    CnnDgradArgs g = dgrad_api_args(rows, cin, cout, hin, groups);
    const int nblk = cnn_dgrad_blocks(g);  // the grid = the partial rows written (<= the bound the query returns)
    if (nblk < 1) {
        set_error("marl_cnn_dgrad: no device");
        return MARL_EHIP;
    }
    if (scratch_bytes < (size_t)nblk * 2 * cin * sizeof(float)) {
        set_error("marl_cnn_dgrad: scratch too small (%zu bytes needed)", (size_t)nblk * 2 * cin * sizeof(float));
        return MARL_ESIZE;
    }
    g.dz = dz;
    g.wt = wt;
    g.ldwt = ldwt;
    g.zin = zin;
    g.gst = gst;
    g.gamma = gamma;
    g.beta = beta;
    g.dzin = dzin;
    g.part = scratch;
    hipStream_t st = static_cast<hipStream_t>(stream);
    MARL_TRY(launch_cnn_dgrad(g, st));
    return launch_reduce_affine(scratch, nblk, cin, dgamma, dbeta, 0, st, nullptr);
}

int marl_cnn_bwd_plan(int64_t rows, int cin, int cout, int hin, int groups, int first,
                      marl_cnn_bwd_plan_info* out) {
    if (!out || rows < 1 || cin < 1 || cout < 1 || hin < 1 || (!first && groups < 1)) {
        set_error("marl_cnn_bwd_plan: bad argument");
        return MARL_EINVAL;
    }
    *out = marl_cnn_bwd_plan_info{};
    // (the shapes marl_cnn_wgrad / marl_cnn_wgrad_scratch plan with: the image's size does not enter the plan)
    CnnWgradArgs w = wgrad_api_args(rows, 1, cin, hin + 1, hin + 1, cin, cout, hin, groups, first != 0);
    if (const CnnWgradPlan p = cnn_wgrad_plan(w); p.form) {
        out->wg_form = p.form, out->wg_rb = p.rb, out->wg_chunks = p.chunks, out->wg_blocks = p.blocks;
        out->wg_sct = p.sct, out->wg_skt = p.skt, out->wg_tgc = p.tgc, out->wg_tgk = p.tgk, out->wg_ms = p.ms;
        out->wg_slabs = p.slabs, out->wg_pd = p.pd, out->wg_pi = p.pi;
    }
    if (!first) {
        const CnnDgradPlan p = dgrad_api_plan(rows, cin, cout, hin, groups);
        out->dg_supported = p.rb != 0, out->dg_rb = p.rb, out->dg_mt = p.MT, out->dg_nt = p.NT, out->dg_blocks = p.chunks;
    }
    return MARL_OK;
}

// ---- the fused extractor forward through its own entry point --------------------------------------------------
// the dimensions of a launch over `rows` rows of cfg's model: everything but the row count as in an episode
static int cnn_fwd_api_dims(const marl_config* cfg, int64_t rows, Dims& d) {
    MARL_TRY(make_dims(cfg, d));
    if (rows < 1 || rows * d.ns >= (1ll << 31)) {
        set_error("cnn_fwd: %lld rows", (long long)rows);
        return MARL_EINVAL;
    }
    d.R = rows;
    d.NR = rows * d.ns;
    return MARL_OK;
}

int marl_cnn_fwd_plan(const marl_config* cfg, int train, int64_t rows, marl_cnn_fwd_plan_info* out) {
    if (!out) {
        set_error("marl_cnn_fwd_plan: null argument");
        return MARL_EINVAL;
    }
    *out = marl_cnn_fwd_plan_info{};
    Dims d;
    MARL_TRY(cnn_fwd_api_dims(cfg, rows, d));
    WLayout w;
    make_wlayout(d, w);
    ELayout e;
    make_elayout(d, w, train, e);  // (the forward plan and what it keeps as every entry of the episode decides them)
    const CnnFwdPlan& p = e.fwd;
    if (!p.which) return MARL_OK;
    for (int l = 0; l < d.L; ++l) out->keeps_cols[l] = e.keeps_cols[l];
    out->fused = 1, out->which = p.which, out->rb = p.rb, out->blocks = p.blocks;
    out->writes_image = p.writes_image;
    return MARL_OK;
}

int marl_cnn_fwd(const marl_config* cfg, const void* weights_ws, size_t weights_ws_bytes, const marl_cnn_fwd_io* io,
                 void* stream) {
    if (!io) {
        set_error("marl_cnn_fwd: null argument");
        return MARL_EINVAL;
    }
    Dims d;
    MARL_TRY(cnn_fwd_api_dims(cfg, io->rows, d));
    WLayout w;
    make_wlayout(d, w);
    bool keeps_cols[MARL_MAX_CNN_LAYERS] = {};
    for (int l = 0; l < d.L; ++l) keeps_cols[l] = io->cols[l] != nullptr;
    CnnFwdArgs probe = cnn_fwd_probe(d, w, keeps_cols);  // (the launch below has the same optional buffers)
    const CnnFwdPlan plan = cnn_fwd_plan(probe);
    if (!plan.which) {
        set_error("marl_cnn_fwd: the fused forward does not cover this model (window %d, %d layers)", d.f, d.L);
        return MARL_ELIMIT;
    }
    auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    bool bad = !weights_ws || (reinterpret_cast<uintptr_t>(weights_ws) & 255) || !io->u || misaligned(io->u) ||
               io->ldu < d.nf || (io->ldu & 3) || (!io->obs && (!io->img || !io->pos));
    for (int l = 0; l < d.L; ++l) bad = bad || misaligned(io->z[l]) || misaligned(io->gst[l]) || misaligned(io->cols[l]);
    if (io->u3) bad = bad || misaligned(io->u3) || io->u3_row0 < 0 || io->u3_steps < img_steps(d.nf);
    if (bad) {
        set_error("marl_cnn_fwd: null or misaligned pointer, or bad size");
        return MARL_EINVAL;
    }
    if (weights_ws_bytes < w.total * sizeof(float)) {
        set_error("marl_cnn_fwd: weights workspace too small (%zu of %zu bytes)", weights_ws_bytes,
                  w.total * sizeof(float));
        return MARL_ESIZE;
    }
    CnnFwdIo f;
    f.img = io->img;
    f.obs = io->obs;
    f.pos = io->pos;
    f.img_u8 = cfg->img_u8 != 0;
    f.rows = io->rows;
    for (int l = 0; l < d.L; ++l) f.cols[l] = io->cols[l], f.z[l] = io->z[l], f.gst[l] = io->gst[l];
    f.u = io->u;
    f.ldu = io->ldu;
    f.u3 = static_cast<char*>(io->u3);
    f.u3_row0 = io->u3_row0;
    f.u3_steps = io->u3_steps;
    CnnFwdArgs a = cnn_fwd_args(d, w, static_cast<const float*>(weights_ws), f);
    if (io->u3 && !plan.writes_image) {
        set_error("marl_cnn_fwd: the kernel selected for this launch does not write the image of U");
        return MARL_EINVAL;
    }
    return launch_cnn_fwd(a, static_cast<hipStream_t>(stream));
}

}  // extern "C"
