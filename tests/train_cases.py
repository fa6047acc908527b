"""Models, batches, the fp64 reference, noise floors, bounds and mutants for the device training step (csrc/tf_train.hip behind
quattro_tf_train_step_f32 / quattro_tf_adam_f32).  A plain helper module (like tests/predictor_cases.py): CPU torch and NumPy
only, used by

  * tests/test_train_cases_cpu.py (teeth and well-posedness: every mutant exceeds a stated multiple of the bound on the case built
    for it, the bounds are tight, the restatement is `training.forward`),
  * tests/test_train_parity_gpu.py (the kernel's loss, prediction and every parameter gradient against the fp64 reference).

Reference: `restated()`, the network of quattro_ilqr_amd.training.forward written once for any dtype, with explicit dropout
factors per site and a small set of named switches (the mutants).  Its gradients come from torch autograd, except through the
attention, whose backward is written out (`_Attention`) in the form the kernel uses (P recomputed, D_i = dO_i . O_i), so that
mistakes which exist only in a backward can be switched on.  tests/test_train_cases_cpu.py pins the unswitched restatement,
values and gradients, to autograd of `training.forward` in float64.

Models: the recipe of predictor_cases.random_model(sharp=True) at any d_model / nhead — peaked attention, biases and LayerNorm
vectors of std 0.3, target embedding of std 0.5 — because on `training.init_params` models (near-uniform attention, zero attention
biases) a slip in a mask or a dropped bias hardly moves a gradient.

What is compared (`compare`): the loss (relative), the prediction (predictor_cases.quantities) and, for every parameter block
viewed as (rows, rest), fro = |G - R| / |R|, row = max_i |G_i - R_i| / (|R| / sqrt(rows)) and col, the same over columns.  Rows
are normalised by the block's RMS row norm, not their own: some rows have an exactly zero true gradient (the K third of
in_proj_bias, dead ReLU units), and whatever a kernel writes there is an error.

The bound is MARGIN x `floor`: the largest distance to the fp64 reference of two fp32 CPU evaluations of the same restatement
(the whole batch in one backward; the gradient accumulated over single-sequence micro-batches, another summation order over
tokens), maximised over the input draws; the loss, a scalar the CPU sums to within half an fp32 spacing, is also summed in
mse_kernel's own order (`kernel_order_loss`).

MARGIN = 4 is stated in advance, not fitted: one factor 2 (predictor_cases.FACTOR) for arithmetic the floor leaves out
(hardware exp, division, rsqrt, MFMA accumulation order), one factor 2 for order-dependent atomic accumulation over up to 28
reduction slices and 64 LayerNorm slices, which neither CPU evaluation reproduces.
"""
import contextlib
import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import predictor_cases as pc

GOLDEN = pc.GOLDEN
MARGIN = 2.0 * pc.FACTOR
TEETH = 5.0                       # a mutant must move a compared quantity of its case to this multiple of the bound
FRO_CEILING = 2e-5                # MARGIN x floor(fro) of every block of every dropout-free case stays below this
OLD_BOUND = 2e-4                  # tests/test_train_hip_gpu.py: per-block rel_fro against fp32 autograd
HARD_LOGIT = pc.HARD_LOGIT
BLOCK_QUANTITIES = ("fro", "row", "col")

# name -> ((n, c, d, H, layers, ff, NS, P, T), batch, random_model keywords).  The smallest shapes that reach each regime of
# tf_train.hip; L = NS + P + T.
CASES = {
    "L32":      ((3, 7, 64, 2, 1, 96, 20, 4, 8), 3, {}),          # one full attention tile; waves 1..3 leave at once
    "L33":      ((3, 7, 64, 2, 1, 96, 20, 4, 9), 3, {}),          # one query in tile 1; M = 99 ragged for LN fwd (4) and bwd (16)
    "L64":      ((4, 5, 128, 4, 2, 192, 40, 8, 16), 3, {}),       # tile edge 64
    "L65":      ((4, 5, 128, 4, 2, 192, 40, 8, 17), 3, {}),       # first three-tile case
    "L96":      ((4, 5, 128, 4, 2, 192, 40, 8, 48), 3, {}),       # three full tiles
    "L97":      ((4, 5, 128, 4, 2, 192, 40, 8, 49), 3, {}),       # one query in tile 3
    "L128_hd8": ((4, 5, 64, 8, 1, 128, 64, 32, 32), 3, {}),       # four tiles at head dimension 8
    "hd1":      ((4, 5, 64, 64, 1, 64, 6, 2, 5), 2, {}),          # the smallest head dimension; attention grid of 64 heads
    "hd3":      ((4, 5, 96, 32, 1, 80, 6, 2, 5), 2, {}),          # an odd head dimension against the 2 kk + hl operand loop
    "d512":     ((4, 5, 512, 16, 1, 64, 20, 4, 9), 4, {}),        # 8 LayerNorm elements per lane, the last one full
    "d480":     ((4, 5, 480, 15, 1, 64, 20, 4, 9), 4, {}),        # ... the last one partial (lanes 0..31)
    "n33_c65":  ((33, 65, 128, 4, 1, 128, 20, 4, 9), 3, {}),      # K = 33: a second reduction stage of one row; N = 65: a second
                                                                  # output tile of one column
    "splitcap": ((12, 52, 128, 4, 1, 1024, 64, 32, 32), 41, {}),  # M = 5248: 32 tiles cap the splits at 32 < 41, kchunk 192,
                                                                  # 28 slices, the last 64 tokens; LN backward: 328 blocks, per = 6
    "hard_softmax": ((4, 5, 128, 4, 2, 192, 40, 8, 17), 3, dict(qk_scale=7.0)),    # as L65, layer-0 logits above 100 (see below)
}
# hard_softmax: q / k rows times 12 gives logits of 255 and MARGIN x floor(fro) = 2.6e-4, far above FRO_CEILING: an fp32 logit of
# size S carries an absolute rounding error of ~S 2^-24, which is the relative error of its exp(), so with S > 100 every
# probability is uncertain by >= 6e-6 and MARGIN x floor(fro) cannot sit much below 2e-5 whatever the model.  Lowered until both
# hold: over 100 model seeds x scales 6 .. 8, logits above 100 gave 1.9e-5 .. 7e-5; seed 436 at scale 7 has logits of 124 and
# 1.9e-5.  The margin to the ceiling is therefore 6 %, on the CPU the floor was measured on.
SEEDS = {"hard_softmax": 436}
SHIPPED = {"shipped_quadrotor": "quadrotor", "shipped_cartpole": "cartpole"}
SHIPPED_BATCH = 6
CASE_NAMES = tuple(CASES) + tuple(SHIPPED)
# not in the parity table: the splitcap model at batch 2, what the workspace-reuse test runs after the batch of 41
AUX = {"splitcap_b2": ("splitcap", 2)}
# (case, dropout rate, seed): the kernel runs with training=True, its masks are dumped and put into the reference
DROPOUT_CASES = (("L65", 0.1, 1234567), ("L128_hd8", 0.5, 1234567), ("L33", 0.1, (7 << 32) | 1234567))
N_DRAWS = {"splitcap": 2}         # input draws behind a floor: 3, and 2 for the large case


def n_draws(name):
    return N_DRAWS.get(AUX.get(name, (name,))[0], 3)


class Case:
    """One model and its batches.  `params`: fp32 arrays under the reference's state-dict names; `pe`: (>= L, d) fp32."""

    def __init__(self, name, shape, batch, params, pe, seed, pool=None):
        self.name, self.shape, self.B, self.params, self.pe, self._seed, self._pool = name, shape, batch, params, pe, seed, pool
        self.n, self.c, self.d, self.H, self.layers, self.ff, self.NS, self.P, self.T = shape
        self.L, self.hd = self.NS + self.P + self.T, self.d // self.H
        self.M = self.B * self.L

    def batch(self, draw=0):
        """(x (B, NS, n), u (B, P, c), y (B, T, c)): normalised inputs and targets, fp32."""
        g = np.random.default_rng([self._seed, draw, 17])
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        y = f(g.standard_normal((self.B, self.T, self.c)))
        if self._pool is not None:          # recorded rows of the shipped checkpoints' fixtures
            xs, us, ys = self._pool
            x, u = (a[[(self.B * draw + j) % a.shape[0] for j in range(self.B)]] for a in (xs, us))
            if ys is not None:
                y = ys[[(self.B * draw + j) % ys.shape[0] for j in range(self.B)]]
            return f(x), f(u), f(y)
        return f(g.standard_normal((self.B, self.NS, self.n))), f(g.standard_normal((self.B, self.P, self.c))), y

    def mask_sizes(self):
        """dropout site -> number of elements (site 0: positions; per layer: attention weights, out-proj, ff hidden, ff out)."""
        B, L, d = self.B, self.L, self.d
        sizes = {0: B * L * d}
        for l in range(self.layers):
            sizes.update({1 + 4 * l: B * self.H * L * L, 2 + 4 * l: B * L * d, 3 + 4 * l: B * L * self.ff, 4 + 4 * l: B * L * d})
        return sizes

    def shape_masks(self, flat):
        """{site: flat factors} -> {site: tensor with a leading batch axis}, float64 (exact in any dtype: 0 or 1 / (1 - p))."""
        B, L = self.B, self.L
        out = {}
        for s, m in flat.items():
            m = torch.as_tensor(np.asarray(m, dtype=np.float64))
            out[s] = m.view(B, self.H, L, L) if (s % 4 == 1) else m.view(B, L, -1)
        return out


def _state_dict(w):
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items() if k != "pos_encoder.pe"}


@functools.lru_cache(maxsize=None)
def case(name):
    if name in AUX:
        base, batch = AUX[name]
        cs = case(base)
        return Case(name, cs.shape, batch, cs.params, cs.pe, cs._seed + 1000)
    if name in SHIPPED:
        model = SHIPPED[name]
        z = np.load(os.path.join(GOLDEN, f"tf_weights_{model}.npz"), allow_pickle=False)
        w = {k: z[k].astype(np.float32) for k in z.files if not k.startswith(("norm.", "hp."))}
        norm = {k[5:]: z[k].astype(np.float64) for k in z.files if k.startswith("norm.")}
        hp = {k[3:]: z[k].item() for k in z.files if k.startswith("hp.")}
        g = np.load(os.path.join(GOLDEN, f"tf_{model}.npz"), allow_pickle=False)
        ds = np.load(os.path.join(GOLDEN, f"dataset_{model}.npz"), allow_pickle=False)
        xs = (g["x_err"] - norm["x_mean"]) / norm["x_std"]
        us = (g["prompt"] - norm["u_mean"]) / norm["u_std"]
        P, T, c = hp["prompt_len"], hp["target_len"], hp["control_dim"]
        kK = ds["kK_data"]                  # recorded gain rows [k | K]; the rows after the prompt are what fit() trains on
        ys = (kK[:, P:P + T] - norm["u_mean"]) / norm["u_std"] if kK.shape[1] >= P + T and kK.shape[2] == c else None
        shape = (hp["state_dim"], c, hp["d_model"], hp["nhead"], hp["num_decoder_layers"], hp["dim_feedforward"],
                 g["x_err"].shape[1], P, T)
        return Case(name, shape, SHIPPED_BATCH, _state_dict(w), w["pos_encoder.pe"][0], 900 + list(SHIPPED).index(name),
                    pool=(xs, us, ys))
    shape, batch, kw = CASES[name]
    n, c, d, H, layers, ff, NS, P, T = shape
    seed = SEEDS.get(name, 300 + list(CASES).index(name))
    w, _, _ = pc.random_model(n, c, NS, P, T, ff, layers, seed, sharp=True, d_model=d, nhead=H, **kw)
    cs = Case(name, shape, batch, _state_dict(w), w["pos_encoder.pe"][0], seed)
    if name == "hard_softmax":
        # exp(S) without the row maximum overflows fp32 at 88.7; the backward recomputes exp(S - max) from the saved statistics
        assert layer0_logit_max(cs) > HARD_LOGIT
    return cs


def layer0_logit_max(cs, draw=0):
    """Largest |q k^T / sqrt(hd)| of the first layer at the visible (causal) positions, fp64."""
    x, u, _ = cs.batch(draw)
    W = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in cs.params.items()}
    h = _embed(W, torch.as_tensor(cs.pe, dtype=torch.float64), torch.as_tensor(x, dtype=torch.float64),
               torch.as_tensor(u, dtype=torch.float64))
    q = "transformer_decoder.layers.0."
    qkv = F.linear(h, W[q + "self_attn.in_proj_weight"], W[q + "self_attn.in_proj_bias"])
    qh, kh, _ = (t.reshape(cs.B, cs.L, cs.H, cs.hd).transpose(1, 2) for t in qkv.split(cs.d, dim=-1))
    s = (qh @ kh.transpose(-1, -2)) / math.sqrt(cs.hd)
    return float(s[..., torch.tril(torch.ones(cs.L, cs.L, dtype=torch.bool))].abs().max())


# ------------------------------------------------------------------------------------------------ the restatement
class _Attention(torch.autograd.Function):
    """softmax(q k^T / sqrt(hd) + causal) * mask @ v on (B, H, L, hd) tensors, with the backward written out as the kernel forms
    it: P recomputed (here: kept), D_i = dO_i . O_i, dS = P (dP mask - D), dQ = dS K, dK = dS^T Q, dV = (P mask)^T dO.
    `flags` switch on mistakes of that backward; the forward has none."""

    @staticmethod
    def forward(ctx, q, k, v, mask, flags):
        L, hd = q.shape[-2:]
        scale = 1.0 / math.sqrt(hd)
        causal = torch.triu(torch.ones(L, L, dtype=torch.bool), diagonal=1)
        p = torch.softmax(((q @ k.transpose(-1, -2)) * scale).masked_fill(causal, float("-inf")), dim=-1)
        o = (p if mask is None else p * mask) @ v
        ctx.save_for_backward(q, k, v, p, o)
        ctx.mask, ctx.flags, ctx.scale = mask, flags, scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, p, o = ctx.saved_tensors
        mask, flags, scale = ctx.mask, ctx.flags, ctx.scale
        L = q.shape[-2]
        if "diag_masked" in flags:                     # the backward's `key <= query` written as `key < query`
            p = p * (1.0 - torch.eye(L, dtype=p.dtype))
        pd = p if mask is None else p * mask
        D = (do * ((p @ v) if "d_undropped" in flags else o)).sum(-1, keepdim=True)
        dP = do @ v.transpose(-1, -2)
        if mask is not None:
            dP = dP * mask
        dS = p * (dP - D)
        dQ = (dS @ k) * scale
        if "no_dq_q32" in flags and L > 32:            # the lone query of tile 1 falls out of sweep A
            dQ = dQ.clone()
            dQ[..., 32, :] = 0
        if "skip_q96_dkdv" in flags and L > 96:        # sweep B stops before query tile 3
            dS, pd = dS.clone(), pd.clone()
            dS[..., 96:, :] = 0
            pd[..., 96:, :] = 0
        dK = (dS.transpose(-1, -2) @ q) * scale
        dV = pd.transpose(-1, -2) @ do
        return dQ, dK, dV, None, None


def _layer_norm(s, g, b, eps, stat_limit):
    """(s - mean) rsqrt(var + eps) g + b over the last axis; channels >= stat_limit stay out of both sums (a mutant)."""
    d = s.shape[-1]
    cut = stat_limit is not None and stat_limit < d
    mean = (s[..., :stat_limit] if cut else s).sum(-1, keepdim=True) / d
    c = s - mean
    cc = c[..., :stat_limit] if cut else c
    var = (cc * cc).sum(-1, keepdim=True) / d
    return c * torch.rsqrt(var + eps) * g + b


def _embed(W, pe, x, u):
    T, d = W["target_embedding"].shape
    B = x.shape[0]
    h = torch.cat([F.linear(x, W["state_embed.weight"], W["state_embed.bias"]),
                   F.linear(u, W["control_embed.weight"], W["control_embed.bias"]),
                   W["target_embedding"].unsqueeze(0).expand(B, T, d)], dim=1)
    return h + pe[: h.shape[1]]


def _rows(B, L, lo, hi, b0):
    """(B, L, 1) bool: token rows lo <= b L + t < hi of the whole batch, for the sequences b0 .. b0 + B of it."""
    r = (torch.arange(b0, b0 + B)[:, None] * L + torch.arange(L)[None, :])[..., None]
    return (r >= lo) & (r < hi)


def restated(W, pe, x, u, nhead, masks=None, sw=None, b0=0):
    """quattro_ilqr_amd.training.forward term for term (transformer_model.py:122-138), any dtype.  `masks`: dropout factors per
    site with a leading batch axis (Case.shape_masks), or None.  `sw`: switches of the mutants, all off by default:
      ln_eps, ln_stat_limit, attn (flags of _Attention.backward), w1_rows / norm2_rows ((lo, hi): the token rows whose
      contribution to the linear1 / norm2 parameter gradients is left out), x_zero_channel, pred_zero_channel."""
    sw = sw or {}
    eps, lim, flags = sw.get("ln_eps", 1e-5), sw.get("ln_stat_limit"), frozenset(sw.get("attn", ()))
    T, d = W["target_embedding"].shape
    B = x.shape[0]
    mk = (lambda t, s: t * masks[s].to(t.dtype)) if masks is not None else (lambda t, s: t)
    if sw.get("x_zero_channel") is not None and sw["x_zero_channel"] < x.shape[-1]:
        x = x.clone()
        x[..., sw["x_zero_channel"]] = 0
    h = mk(_embed(W, pe, x, u), 0)
    L = h.shape[1]
    hd = d // nhead
    n_layers = sum(1 for k in W if k.endswith("self_attn.in_proj_weight"))
    for i in range(n_layers):
        q = f"transformer_decoder.layers.{i}."
        qkv = F.linear(h, W[q + "self_attn.in_proj_weight"], W[q + "self_attn.in_proj_bias"])
        qh, kh, vh = (t.reshape(B, L, nhead, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        am = masks[1 + 4 * i].to(h.dtype) if masks is not None else None
        o = _Attention.apply(qh, kh, vh, am, flags).transpose(1, 2).reshape(B, L, d)
        o = F.linear(o, W[q + "self_attn.out_proj.weight"], W[q + "self_attn.out_proj.bias"])
        h = _layer_norm(h + mk(o, 2 + 4 * i), W[q + "norm1.weight"], W[q + "norm1.bias"], eps, lim)
        w1, b1 = W[q + "linear1.weight"], W[q + "linear1.bias"]
        f = F.linear(h, w1, b1)
        if sw.get("w1_rows") is not None:
            f = torch.where(_rows(B, L, *sw["w1_rows"], b0), F.linear(h, w1.detach(), b1.detach()), f)
        f = F.linear(mk(torch.relu(f), 3 + 4 * i), W[q + "linear2.weight"], W[q + "linear2.bias"])
        g2, be2 = W[q + "norm2.weight"], W[q + "norm2.bias"]
        if sw.get("norm2_rows") is not None:
            out = _rows(B, L, *sw["norm2_rows"], b0)
            g2, be2 = torch.where(out, g2.detach(), g2), torch.where(out, be2.detach(), be2)
        h = _layer_norm(h + mk(f, 4 + 4 * i), g2, be2, eps, lim)
    pred = F.linear(h[:, -T:, :], W["output_linear.weight"], W["output_linear.bias"])
    if sw.get("pred_zero_channel") is not None and sw["pred_zero_channel"] < pred.shape[-1]:
        pred = torch.cat([pred[..., :sw["pred_zero_channel"]], torch.zeros_like(pred[..., sw["pred_zero_channel"]:])], dim=-1)
    return pred


@contextlib.contextmanager
def _one_thread():
    """Many small products: a thread pool over every core of the machine runs them ten times slower than one thread."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def evaluate(params, pe, x, u, y, nhead, dtype=torch.float64, masks=None, sw=None, micro=False):
    """dict(loss, pred (B, T, c), grads {name: array}) of the MSE loss of `restated`, computed in `dtype`, returned as fp64.
    micro=True accumulates the gradient over single-sequence backward passes (another summation order over the tokens)."""
    with _one_thread():
        return _evaluate(params, pe, x, u, y, nhead, dtype, masks, sw, micro)


def _evaluate(params, pe, x, u, y, nhead, dtype, masks, sw, micro):
    W = {k: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_(True) for k, v in params.items()}
    pe, x, u, y = (torch.as_tensor(np.asarray(a), dtype=dtype) for a in (pe, x, u, y))
    B = x.shape[0]
    if not micro:
        pred = restated(W, pe, x, u, nhead, masks, sw)
        loss = F.mse_loss(pred, y)
        loss.backward()
    else:
        preds, loss = [], torch.zeros((), dtype=dtype)
        for b in range(B):
            mb = None if masks is None else {s: m[b:b + 1] for s, m in masks.items()}
            pb = restated(W, pe, x[b:b + 1], u[b:b + 1], nhead, mb, sw, b0=b)
            lb = ((pb - y[b:b + 1]) ** 2).sum() / y.numel()
            lb.backward()
            preds.append(pb.detach())
            loss = loss + lb.detach()
        pred = torch.cat(preds)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).double().numpy() for k, v in W.items()}
    return dict(loss=float(loss.detach().double()), pred=pred.detach().double().numpy(), grads=grads)


# the masked forward tests/test_train_hip_gpu.py compares the dropout step with (fp32 autograd on the GPU); `restated` is pinned
# to it as well
def forward_with_masks(params, buffers, x, u, nhead, masks):
    """training.forward with explicit dropout factors per site (0: positions; per layer: attention weights, out-proj,
    ff hidden, ff output) — the same network, term for term (transformer_model.py:122-138)."""
    W = params
    T, d = W["target_embedding"].shape
    B = x.shape[0]
    h = torch.cat([F.linear(x, W["state_embed.weight"], W["state_embed.bias"]),
                   F.linear(u, W["control_embed.weight"], W["control_embed.bias"]),
                   W["target_embedding"].unsqueeze(0).expand(B, T, d)], dim=1)
    L = h.shape[1]
    h = (h + buffers["pos_encoder.pe"][:, :L]) * masks[0].view(B, L, d)
    hd = d // nhead
    causal = torch.triu(torch.ones(L, L, dtype=torch.bool, device=h.device), diagonal=1)
    n_layers = sum(1 for k in W if k.endswith("self_attn.in_proj_weight"))
    for i in range(n_layers):
        q = f"transformer_decoder.layers.{i}."
        qkv = F.linear(h, W[q + "self_attn.in_proj_weight"], W[q + "self_attn.in_proj_bias"])
        qh, kh, vh = (t.reshape(B, L, nhead, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        s = (qh @ kh.transpose(-1, -2)) * (1.0 / math.sqrt(hd))
        a = torch.softmax(s.masked_fill(causal, float("-inf")), dim=-1) * masks[1 + 4 * i].view(B, nhead, L, L)
        o = (a @ vh).transpose(1, 2).reshape(B, L, d)
        o = F.linear(o, W[q + "self_attn.out_proj.weight"], W[q + "self_attn.out_proj.bias"])
        h = F.layer_norm(h + o * masks[2 + 4 * i].view(B, L, d), (d,), W[q + "norm1.weight"], W[q + "norm1.bias"], 1e-5)
        f = torch.relu(F.linear(h, W[q + "linear1.weight"], W[q + "linear1.bias"])) * masks[3 + 4 * i].view(B, L, -1)
        f = F.linear(f, W[q + "linear2.weight"], W[q + "linear2.bias"])
        h = F.layer_norm(h + f * masks[4 + 4 * i].view(B, L, d), (d,), W[q + "norm2.weight"], W[q + "norm2.bias"], 1e-5)
    return F.linear(h[:, -T:, :], W["output_linear.weight"], W["output_linear.bias"])


# ------------------------------------------------------------------------------------------------ what is compared
def block_quantities(G, R):
    G, R = np.asarray(G, dtype=np.float64), np.asarray(R, dtype=np.float64)
    G, R = G.reshape(G.shape[0], -1), R.reshape(R.shape[0], -1)
    d = G - R
    nr = float(np.linalg.norm(R)) or 1.0
    return dict(fro=float(np.linalg.norm(d)) / nr,
                row=float(np.linalg.norm(d, axis=1).max()) / (nr / math.sqrt(R.shape[0])),
                col=float(np.linalg.norm(d, axis=0).max()) / (nr / math.sqrt(R.shape[1])))


def compare(got, ref):
    """{key: distance} over everything the parity test asserts: "loss", "pred:fro|token|channel", "<block>:fro|row|col"."""
    out = {"loss": abs(got["loss"] - ref["loss"]) / (abs(ref["loss"]) or 1.0)}
    out.update({f"pred:{k}": v for k, v in pc.quantities(got["pred"], ref["pred"]).items()})
    for name, R in ref["grads"].items():
        out.update({f"{name}:{k}": v for k, v in block_quantities(got["grads"][name], R).items()})
    return out


@functools.lru_cache(maxsize=None)
def reference(name, draw=0):
    cs = case(name)
    return evaluate(cs.params, cs.pe, *cs.batch(draw), cs.H)


def kernel_order_loss(pred, y, order):
    """The MSE loss summed as mse_kernel sums it, in fp32: min(256, ceil(n / 256)) workgroups of 256 threads striding over the
    elements, a butterfly over each wave, four waves added, times 1 / n, and the workgroups' partial losses added one after
    another in `order` (on the device: whichever order the atomic adds arrive in)."""
    f = np.float32
    e = (np.asarray(pred, dtype=f) - np.asarray(y, dtype=f)).ravel()
    n = e.size
    blocks = min(256, max(1, (n + 255) // 256))
    rounds = (n + blocks * 256 - 1) // (blocks * 256)
    e = np.concatenate([e, np.zeros(rounds * blocks * 256 - n, dtype=f)]).reshape(rounds, blocks, 4, 64)
    acc = np.zeros((blocks, 4, 64), dtype=f)
    for k in range(rounds):
        acc = e[k] * e[k] + acc
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ o]
    part = (((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0]) + acc[:, 3, 0]) * (f(1.0) / f(n))
    total = f(0.0)
    for b in order(blocks):
        total = total + part[b]
    return float(total)


# arrival orders of the workgroups' atomic adds the loss floor is taken over: ascending, descending, three shuffles
LOSS_ORDERS = (lambda n: range(n), lambda n: range(n - 1, -1, -1)) + tuple(
    (lambda n, s=s: np.random.default_rng(s).permutation(n)) for s in (1, 2, 3))


def floor_of(cs, draws, masks=None, refs=None):
    """{key: the largest distance to the fp64 reference of the fp32 evaluations, maximised over the draws}.  Two evaluations
    for everything (whole batch; single-sequence micro-batches).  The loss has a third: the CPU evaluations sum it pairwise and
    land within half an fp32 spacing of the truth, the device adds up to 256 partial losses atomically in arrival order, so the
    whole-batch fp32 prediction's loss is also summed in mse_kernel's order under LOSS_ORDERS (a restatement of the kernel's
    summation order, as a further fp32 evaluation)."""
    worst = {}
    for draw in range(draws):
        x, u, y = cs.batch(draw)
        ref = refs[draw] if refs is not None else evaluate(cs.params, cs.pe, x, u, y, cs.H, masks=masks)
        for micro in (False, True):
            got = evaluate(cs.params, cs.pe, x, u, y, cs.H, dtype=torch.float32, masks=masks, micro=micro)
            q = compare(got, ref)
            if not micro:
                for order in LOSS_ORDERS:
                    q["loss"] = max(q["loss"], abs(kernel_order_loss(got["pred"], y, order) - ref["loss"]) / abs(ref["loss"]))
            worst = {k: max(worst.get(k, 0.0), v) for k, v in q.items()}
    return worst


@functools.lru_cache(maxsize=None)
def floor(name):
    cs = case(name)
    return floor_of(cs, n_draws(name), refs=[reference(name, d) for d in range(n_draws(name))])


def bound_of(fl):
    """MARGIN x floor; a floor of exactly 0 (a block whose fp32 gradient is exact) is replaced by the smallest non-zero floor of
    the same quantity in this case, so that no bound is zero.  The loss has no second block to borrow from: one fp32 unit
    round-off (2^-24), the least a correctly rounded fp32 loss can differ by."""
    kind = lambda k: k.rsplit(":", 1)[-1]
    out = {}
    for k, v in fl.items():
        if v == 0.0:
            same = [w for j, w in fl.items() if w > 0.0 and ":" in j and ":" in k and kind(j) == kind(k)]
            v = min(same) if same else 2.0 ** -24
        out[k] = MARGIN * v
    return out


def bound(name):
    return bound_of(floor(name))


def worst_ratio(q, ref_scale):
    """(key, ratio) of the largest q[key] / ref_scale[key]."""
    k = max(q, key=lambda j: q[j] / ref_scale[j])
    return k, q[k] / ref_scale[k]


# ------------------------------------------------------------------------------------------------ dropout masks
def _mix32(x):
    x = x & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def hashed_mask(seed, p, site, n):
    """keep_scale of tf_train.hip for elements 0 .. n of `site`: 0 or 1 / (1 - p), fp32.  The counter hash of (seed, site,
    element index) the kernels recompute wherever a mask is needed."""
    idx = np.arange(n, dtype=np.uint64)
    h = _mix32(idx + np.uint64((0x9e3779b9 * (site + 1)) & 0xFFFFFFFF))
    h = _mix32(h ^ (idx >> np.uint64(32)) ^ np.uint64(seed & 0xFFFFFFFF))
    h = _mix32(h + np.uint64((seed >> 32) & 0xFFFFFFFF))
    u = (h >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u >= np.float32(p), np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32)


def hashed_masks(cs, seed, p):
    return {s: hashed_mask(seed, p, s, n) for s, n in cs.mask_sizes().items()}


# ------------------------------------------------------------------------------------------------ mutants
# Each maps a Case to the switches of `restated` that make the mistake at that shape, or None where the mistake cannot be made
# there (no second tile, one reduction slice, ...).  The sizes come from the launch arithmetic of tf_train.hip, restated here.

def gemm_split(rows_out, cols_out, K):
    """(splits, kchunk) of gemm_launch in MODE_ATOMIC for a (rows_out x cols_out) result reduced over K."""
    tiles = ((rows_out + 63) // 64) * ((cols_out + 63) // 64)
    splits = max(1, min(1024 // tiles, (K + 127) // 128))
    kchunk = (((K + splits - 1) // splits) + 31) // 32 * 32
    return (K + kchunk - 1) // kchunk, kchunk


def ln_reduce_split(M):
    """(nblocks, per) of ln_bwd_reduce_kernel: 16-row blocks, 64 slices of `per` blocks."""
    nblocks = (M + 15) // 16
    return nblocks, (nblocks + 63) // 64


def _split_tail(cs):
    splits, kchunk = gemm_split(cs.ff, cs.d, cs.M)
    return dict(w1_rows=((splits - 1) * kchunk, cs.M)) if splits > 1 else None


def _ln_partial_slice(cs):
    nblocks, per = ln_reduce_split(cs.M)
    if per == 1 or nblocks % per == 0:
        return None
    return dict(norm2_rows=(16 * (nblocks // per) * per, cs.M))


MUTANTS = {
    "ln_eps_1e-6": lambda cs: dict(ln_eps=1e-6),
    "bwd_diag_masked": lambda cs: dict(attn=("diag_masked",)),
    "tile1_first_query_no_dq": lambda cs: dict(attn=("no_dq_q32",)),
    "tile3_queries_skipped_in_dkdv": lambda cs: dict(attn=("skip_q96_dkdv",)),
    "split_tail_dropped": _split_tail,
    "ln_reduce_partial_slice_dropped": _ln_partial_slice,
    "d_from_undropped_p": lambda cs: dict(attn=("d_undropped",)),
    "stage_tail_dropped": lambda cs: dict(x_zero_channel=32) if cs.n > 32 else None,
    "last_output_column_dropped": lambda cs: dict(pred_zero_channel=64) if cs.c > 64 else None,
    "ln_last_lane_elements_dropped": lambda cs: dict(ln_stat_limit=448) if cs.d > 448 else None,
}
# mutant -> (cases that must catch it, cases it must leave exactly unchanged).  "any": every dropout-free case is tried and at
# least one must catch it; "dropout": the DROPOUT_CASES with hashed masks.
CAUGHT_BY = {
    "ln_eps_1e-6": ("any", ()),
    "bwd_diag_masked": ("any", ()),
    "tile1_first_query_no_dq": (("L33",), ("L32",)),
    "tile3_queries_skipped_in_dkdv": (("L97",), ("L96",)),
    "split_tail_dropped": (("splitcap",), ()),
    "ln_reduce_partial_slice_dropped": (("splitcap",), ()),
    "d_from_undropped_p": ("dropout", ()),
    "stage_tail_dropped": (("n33_c65",), ()),
    "last_output_column_dropped": (("n33_c65",), ()),
    "ln_last_lane_elements_dropped": (("d512", "d480"), ()),
}


def mutant_eval(cs, mutant, draw=0, masks=None):
    """The fp64 restatement with the mutant switched on, or None where it does not apply to this shape."""
    sw = MUTANTS[mutant](cs)
    if sw is None:
        return None
    return evaluate(cs.params, cs.pe, *cs.batch(draw), cs.H, masks=masks, sw=sw)


@functools.lru_cache(maxsize=None)
def mutant_ratio(name, mutant):
    """(key, largest shift / bound over the compared quantities) on a dropout-free case, or None."""
    got = mutant_eval(case(name), mutant)
    return None if got is None else worst_ratio(compare(got, reference(name)), bound(name))


# ------------------------------------------------------------------------------------------------ the suite before this module
OLD_SHAPES = {     # tests/test_train_hip_gpu.py::SHAPES with the batch sizes of its gradient test
    "quadrotor": ((12, 52, 128, 4, 3, 512, 51, 1, 49), 6), "cartpole": ((4, 5, 128, 4, 2, 256, 31, 5, 26), 6),
    "small": ((3, 7, 64, 2, 1, 96, 6, 2, 5), 5), "long": ((4, 5, 64, 2, 2, 128, 64, 32, 32), 6),
    "default": ((4, 5, 64, 8, 3, 128, 31, 10, 21), 6), "hd16": ((12, 52, 128, 8, 1, 256, 21, 3, 18), 6),
    "d96": ((4, 5, 96, 4, 2, 80, 9, 3, 7), 6),
}


def old_case(name, seed=3):
    """The model and batch of test_train_hip_gpu.py::_setup, on the CPU: training.init_params (near-uniform attention), biases and
    LayerNorm vectors moved by 0.2 randn, standard-normal batch."""
    from quattro_ilqr_amd import training
    shape, B = OLD_SHAPES[name]
    n, c, d, H, layers, ff, NS, P, T = shape
    params, buffers = training.init_params(n, c, d, H, layers, ff, NS + P + T + 9, T, seed=seed, device="cpu")
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, v in params.items():
            if k.endswith("bias") or "norm" in k:
                v += 0.2 * torch.randn(v.shape, generator=g)
    x, u, y = (torch.randn(s, generator=g).numpy() for s in ((B, NS, n), (B, P, c), (B, T, c)))
    cs = Case("old_" + name, shape, B, {k: v.detach().numpy() for k, v in params.items()}, buffers["pos_encoder.pe"][0].numpy(), 0)
    cs.batch = lambda draw=0: (x, u, y)
    return cs


# ------------------------------------------------------------------------------------------------ Adam
ADAM_T = (1, 2, 1000, 100000)
ADAM_QUANTITIES = ("m", "v", "dp", "p")
ADAM_MUTANTS = ("eps_inside_sqrt", "no_second_bias_correction")


def adam_step(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, dtype=np.float64, mutant=None, abi=True):
    """One torch.optim.Adam step (no weight decay) in `dtype`: (p, m, v) after step number t.  abi=True: lr, the betas and eps
    are the fp32 values the C ABI carries (0.999f is 0.99900001287..., 1.3e-5 off in 1 - beta2; what the kernel is given is what
    the reference gets), and the bias corrections are formed in double from them and rounded to `dtype`, as
    quattro_tf_adam_f32 forms them."""
    f = dtype
    if abi:
        lr, b1, b2, eps = (float(np.float32(a)) for a in (lr, b1, b2, eps))
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    lrf, b1f, b2f, epsf = f(lr), f(b1), f(b2), f(eps)
    c1 = f(1.0 - b1 ** t)
    c2 = f(1.0) if mutant == "no_second_bias_correction" else f(1.0 - b2 ** t)
    m2 = b1f * m + (f(1) - b1f) * g
    v2 = b2f * v + (f(1) - b2f) * g * g
    den = np.sqrt(v2 / c2 + epsf) if mutant == "eps_inside_sqrt" else np.sqrt(v2 / c2) + epsf
    return p - lrf * (m2 / c1) / den, m2, v2


def adam_problem(n, t, seed=0):
    """State before step t and its gradient, fp32: |g| log-uniform over 1e-10 .. 1 with random sign; for t > 1 moments of the
    same spread (m of either sign, v >= 0); a tenth of the entries have g = m = v = 0.  p is 0 on the first half of the live
    entries (the update is then read off p exactly) and standard normal elsewhere."""
    r = np.random.default_rng([seed, t])
    mag = lambda: 10.0 ** r.uniform(-10, 0, n) * r.choice([-1.0, 1.0], n)
    g = mag()
    m, v = (mag(), mag() ** 2) if t > 1 else (np.zeros(n), np.zeros(n))
    dead = r.random(n) < 0.1
    g[dead], m[dead], v[dead] = 0.0, 0.0, 0.0
    p = r.standard_normal(n)
    p[(np.arange(n) < n // 2) & ~dead] = 0.0
    return tuple(a.astype(np.float32) for a in (p, g, m, v)) + (dead,)


def adam_compare(got, ref, prob, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """Largest element-wise distances of (p, m, v) `got` to the fp64 `ref`, each relative to a scale that does not vanish where
    the two terms of m cancel: m against b1 |m| + (1 - b1) |g|; v against itself (its terms are non-negative); dp, on entries
    that started at p = 0, against the update formed with that m scale; p, elsewhere, against |p before| + that update."""
    p0, g, m0, v0, dead = (np.asarray(a, dtype=np.float64) if a.dtype != bool else a for a in prob)
    (pg, mg, vg), (pr, mr, vr) = ([np.asarray(a, dtype=np.float64) for a in s] for s in (got, ref))
    live = ~dead
    ms = b1 * np.abs(m0) + (1 - b1) * np.abs(g)
    us = lr * (ms / (1 - b1 ** t)) / (np.sqrt(vr / (1 - b2 ** t)) + eps)
    z = live & (p0 == 0)
    nz = live & (p0 != 0)
    return dict(m=float((np.abs(mg - mr)[live] / ms[live]).max()), v=float((np.abs(vg - vr)[live] / vr[live]).max()),
                dp=float((np.abs(pg - pr)[z] / us[z]).max()), p=float((np.abs(pg - pr)[nz] / (np.abs(p0) + us)[nz]).max()))


def adam_floor(prob, t):
    p, g, m, v, _ = prob
    return adam_compare(adam_step(p, g, m, v, t, dtype=np.float32), adam_step(p, g, m, v, t), prob, t)
