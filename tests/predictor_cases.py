"""Predictor models, inputs, noise bounds and mutants for the fused transformer forward (csrc/tf_stream.hip).  A plain helper
module (like tests/param_cases.py), NumPy only, used by

  * tests/test_predictor_cases_cpu.py (teeth: every mutant moves what the GPU test compares by a stated multiple of its bound),
  * tests/test_predictor_parity_gpu.py (every kernel instantiation, both operand types, against the fp64 oracle).

Why these models: TransformerILQR.random_init gives near-uniform attention, biases of std 0.02 and an identity normalisation, so
a slip in the causal mask, a dropped bias or a mixed-up normalisation vector hardly moves its output.  Every random model here
has peaked attention (q and k rows of in_proj_weight scaled), biases and LayerNorm vectors of std 0.3, a target embedding of
std 0.5 and random x_mean / x_std / u_mean / u_std.  The shapes put tile-boundary rows (32, 64, 96) among the targets, prompts
across a tile edge, and the parameter blocks at their extreme sizes.

What is compared (`quantities`): whole-tensor relative Frobenius error, the worst single target token, and the worst output
channel (normalised by that channel's norm over all tokens).  A mistake that hits one row or one column is diluted in the first
and stands out in the other two.

The bound (`bound`) is 2 x `noise`: the distance, on weights already rounded to the operand type, between the fp64 oracle with
both operands of every matrix product rounded to that type (oracle.transformer.forward(operand=...)) and the plain fp64 oracle,
maximum over N_DRAWS input draws.  The factor 2 is an allowance over that CPU-measured floor for what the model leaves out: fp32
accumulation order, hardware exp2 / rsqrt, and a kernel that rounds at other points than the model does.  It is not fitted.
"""
import contextlib
import functools
import os

import numpy as np

from oracle import transformer as o_tf

try:        # many small fp64 products: a BLAS that spreads each over every core of the machine runs them 20 x slower
    from threadpoolctl import threadpool_limits as _one_thread
except ImportError:
    _one_thread = lambda limits: contextlib.nullcontext()

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D, NHEAD, HD = 128, 4, 32
PRECISIONS = ("bf16", "fp16")
B = 3                      # sequences per input draw (the batch of the GPU parity test)
N_DRAWS = 4
FACTOR = 2.0
QUANTITIES = ("fro", "token", "channel")
_MATRICES = ("in_proj_weight", "out_proj.weight", "linear1.weight", "linear2.weight", "embed.weight", "output_linear.weight")

# shape of every random model: n, c, state tokens ns, prompt rows P, targets T, ff, layers (max_seq_len 128 throughout)
SHAPES = {
    "L21_ff64_c5":     dict(n=4, c=5, ns=11, P=2, T=8, ff=64, layers=1),        # one wave, the smallest FFN, c = 5, one layer
    "L61_straddle":    dict(n=4, c=5, ns=31, P=5, T=25, ff=192, layers=2),      # two waves; the prompt (31..35) straddles token 32
    "L81":             dict(n=12, c=52, ns=51, P=5, T=25, ff=320, layers=2),    # three waves (uneven LDS-DMA shares); target 64
    "L101_ff1024":     dict(n=12, c=52, ns=51, P=1, T=49, ff=1024, layers=1),   # four waves, b1 block at its largest offset
    "L128_3layers":    dict(n=12, c=52, ns=64, P=32, T=32, ff=512, layers=3),   # no padding token; the targets start on tile 3
    "L32_n1":          dict(n=1, c=2, ns=20, P=4, T=8, ff=128, layers=1),       # the last token of one wave; n = 1
    "L33_n16":         dict(n=16, c=51, ns=20, P=4, T=9, ff=64, layers=2),      # one token in the second wave; the largest n
    "L104_tile_rows":  dict(n=12, c=52, ns=20, P=4, T=80, ff=256, layers=2),    # rows 32, 64 and 96 are all targets
    "L64_c64":         dict(n=15, c=64, ns=30, P=3, T=31, ff=128, layers=2),    # second output panel full
    "L47_c33":         dict(n=10, c=33, ns=35, P=2, T=10, ff=64, layers=1),     # second output panel: one row
    "L61_hard_softmax": dict(n=4, c=5, ns=31, P=5, T=25, ff=128, layers=2, qk_scale=12.0),
}
# the shipped checkpoints, on the recorded inputs of tf_*.npz and on the x_err / prompt that the reference's hybrid solve logged
# (hybrid_*.npz: states up to 27 standard deviations out, where the model is several times more sensitive to rounding).  Two
# cases per checkpoint, because a bound holds for the population of inputs it was measured on.
SHIPPED = {"shipped_quadrotor": ("quadrotor", "tf"), "shipped_cartpole": ("cartpole", "tf"),
           "shipped_quadrotor_hybrid": ("quadrotor", "hybrid"), "shipped_cartpole_hybrid": ("cartpole", "hybrid")}
CASE_NAMES = tuple(SHAPES) + tuple(SHIPPED)
WAVE_COUNT_CASES = ("L21_ff64_c5", "L61_straddle", "L81", "L101_ff1024")    # 1, 2, 3, 4 waves; c = m (1 + n) for gains mode
GAIN_DIMS = {"L21_ff64_c5": (4, 1), "L61_straddle": (4, 1), "L81": (12, 4), "L101_ff1024": (12, 4)}   # (n, m)
HARD_LOGIT = 100.0


class Case:
    def __init__(self, name, w, norm, hp, ns, pool=None, seed=0):
        self.name, self.w, self.norm, self.hp, self.ns = name, w, norm, hp, ns
        self.P, self.T, self.n, self.c = hp["prompt_len"], hp["target_len"], hp["state_dim"], hp["control_dim"]
        self.ff, self.layers, self.L = hp["dim_feedforward"], hp["num_decoder_layers"], ns + self.P + self.T
        self._pool, self._seed = pool, seed

    def inputs(self, draw=0):
        """(x (B, ns, n), prompt (B, P, c)): raw (un-normalised) inputs, fp32 values held in fp64."""
        if self._pool is not None:                            # recorded rows of the shipped checkpoints' fixtures
            xs, ps = self._pool
            idx = [(B * draw + j) % xs.shape[0] for j in range(B)]
            return xs[idx].copy(), ps[idx].copy()
        g = np.random.default_rng([self._seed, draw])
        x = self.norm["x_mean"] + self.norm["x_std"] * g.standard_normal((B, self.ns, self.n))
        p = self.norm["u_mean"] + self.norm["u_std"] * g.standard_normal((B, self.P, self.c))
        f = lambda a: a.astype(np.float32).astype(np.float64)
        return f(x), f(p)


def sinusoid_pe(max_len, d=D):
    pos = np.arange(max_len, dtype=np.float32)[:, None]
    div = np.exp(np.arange(0, d, 2, dtype=np.float32) * (-np.log(10000.0) / d))
    pe = np.zeros((max_len, d), dtype=np.float32)
    pe[:, 0::2], pe[:, 1::2] = np.sin(pos * div), np.cos(pos * div)
    return pe[None]


def random_model(n, c, ns, P, T, ff, layers, seed, sharp=True, qk_scale=4.0, max_seq_len=128, d_model=D, nhead=NHEAD):
    """(w, norm, hp).  sharp=False restates TransformerILQR.random_init: what the suite tested before this module.  d_model and
    nhead default to the predictor kernel's 128 / 4 (tests/train_cases.py draws other widths from the same recipe); the order of
    the random draws does not depend on them, so the defaults give the models they always gave."""
    D = d_model
    g = np.random.default_rng(seed)
    bs, ln, te = (0.3, 0.3, 0.5) if sharp else (0.02, 0.05, 0.02)
    lin = lambda o, i: (g.uniform(-1, 1, (o, i)) / np.sqrt(i)).astype(np.float32)
    vec = lambda o, s: (s * g.standard_normal(o)).astype(np.float32)
    w = {"target_embedding": (te * g.standard_normal((T, D))).astype(np.float32),
         "state_embed.weight": lin(D, n), "state_embed.bias": vec(D, bs),
         "control_embed.weight": lin(D, c), "control_embed.bias": vec(D, bs),
         "output_linear.weight": lin(c, D), "output_linear.bias": vec(c, bs),
         "pos_encoder.pe": sinusoid_pe(max_seq_len, D)}
    for i in range(layers):
        p = f"transformer_decoder.layers.{i}."
        wi = lin(3 * D, D)
        if sharp:
            wi[:2 * D] *= np.float32(qk_scale)
        w[p + "self_attn.in_proj_weight"], w[p + "self_attn.in_proj_bias"] = wi, vec(3 * D, bs)
        w[p + "self_attn.out_proj.weight"], w[p + "self_attn.out_proj.bias"] = lin(D, D), vec(D, bs)
        w[p + "linear1.weight"], w[p + "linear1.bias"] = lin(ff, D), vec(ff, bs)
        w[p + "linear2.weight"], w[p + "linear2.bias"] = lin(D, ff), vec(D, bs)
        for nm in ("norm1", "norm2"):
            w[p + nm + ".weight"], w[p + nm + ".bias"] = (1.0 + vec(D, ln)).astype(np.float32), vec(D, bs if sharp else 0.02)
    if sharp:
        f = lambda a: a.astype(np.float32).astype(np.float64)
        norm = dict(x_mean=f(g.standard_normal(n)), x_std=f(0.5 + 1.5 * g.random(n)),
                    u_mean=f(g.standard_normal(c)), u_std=f(0.5 + 1.5 * g.random(c)))
    else:
        norm = dict(x_mean=np.zeros(n), x_std=np.ones(n), u_mean=np.zeros(c), u_std=np.ones(c))
    hp = dict(target_len=T, prompt_len=P, state_dim=n, control_dim=c, d_model=D, nhead=nhead, num_decoder_layers=layers,
              dim_feedforward=ff, dropout=0.0, max_seq_len=max_seq_len)
    return w, norm, hp


def layer0_logits(case, draw=0):
    """fp64 attention logits q k^T / sqrt(hd) of the first layer at the visible (causal) positions."""
    x, p = case.inputs(draw)
    xn, pn = _normalise(case.norm, x, p)
    _, hidden = o_tf.forward(case.w, xn, pn, NHEAD, return_hidden=True)
    h = hidden[0]
    qkv = h @ case.w["transformer_decoder.layers.0.self_attn.in_proj_weight"].astype(np.float64).T \
        + case.w["transformer_decoder.layers.0.self_attn.in_proj_bias"]
    split = lambda a: a.reshape(h.shape[0], case.L, NHEAD, HD).transpose(0, 2, 1, 3)
    q, k = split(qkv[..., :D]), split(qkv[..., D:2 * D])
    s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(HD)
    return s[..., np.tril(np.ones((case.L, case.L), dtype=bool))]


@functools.lru_cache(maxsize=None)
def case(name):
    if name in SHIPPED:
        model, rows = SHIPPED[name]
        z = np.load(os.path.join(GOLDEN, f"tf_weights_{model}.npz"), allow_pickle=False)
        w = {k: z[k].astype(np.float32) for k in z.files if not k.startswith(("norm.", "hp."))}
        norm = {k[5:]: z[k].astype(np.float64) for k in z.files if k.startswith("norm.")}
        hp = {k[3:]: z[k].item() for k in z.files if k.startswith("hp.")}
        assert hp["d_model"] == D and hp["nhead"] == NHEAD
        g = np.load(os.path.join(GOLDEN, f"{rows}_{model}.npz"), allow_pickle=False)
        f = lambda a: a.astype(np.float32).astype(np.float64)
        pool = (f(g["x_err"]), f(g["prompt"]))
        return Case(name, w, norm, hp, pool[0].shape[1], pool=pool)
    sh = dict(SHAPES[name])
    seed = 100 + list(SHAPES).index(name)
    w, norm, hp = random_model(seed=seed, **sh)
    cs = Case(name, w, norm, hp, sh["ns"], seed=seed)
    if name == "L61_hard_softmax":
        # an exp() without the running-maximum subtraction overflows fp32 at 88.7
        assert np.abs(layer0_logits(cs)).max() > HARD_LOGIT
    return cs


def round_weights(w, precision):
    """The weight dict with every matrix the kernel feeds to an MFMA rounded to the operand type (what both sides of a
    comparison start from); vectors, the target embedding and the positional table stay fp32."""
    return {k: (o_tf.round_operand(v, precision) if k.endswith(_MATRICES) else np.asarray(v, dtype=np.float64))
            for k, v in w.items()}


def _normalise(norm, x, prompt):
    xn = ((x - norm["x_mean"]) / norm["x_std"]).astype(np.float32)
    pn = ((prompt - norm["u_mean"]) / norm["u_std"]).astype(np.float32)
    return xn, pn


def evaluate(w, norm, x, prompt, operand=None, mask=None):
    """Batched oracle.transformer.predict: raw x (B, ns, n), raw prompt (B, P, c) -> de-normalised (B, T, c), fp64."""
    xn, pn = _normalise(norm, x, prompt)
    with _one_thread(limits=1):
        y = o_tf.forward(w, xn, pn, NHEAD, operand=operand, mask=mask)
    return y * norm["u_std"] + norm["u_mean"]


def quantities(got, want):
    """dict(fro, token, channel) of got against want, both (B, T, c)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d = got - want
    nz = lambda a: np.where(a > 0, a, 1.0)
    tok = np.linalg.norm(d, axis=2) / nz(np.linalg.norm(want, axis=2))
    ch = np.linalg.norm(d.reshape(-1, d.shape[2]), axis=0) / nz(np.linalg.norm(want.reshape(-1, d.shape[2]), axis=0))
    return dict(fro=float(np.linalg.norm(d) / nz(np.linalg.norm(want))), token=float(tok.max()), channel=float(ch.max()))


@functools.lru_cache(maxsize=None)
def reference(name, precision, draw=0):
    """fp64 oracle on the operand-rounded weights: what the kernel is compared with."""
    cs = case(name)
    x, p = cs.inputs(draw)
    out = evaluate(rounded(name, precision), cs.norm, x, p)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def noise(name, precision, draws=N_DRAWS):
    cs = case(name)
    wq = rounded(name, precision)
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for draw in range(draws):
        x, p = cs.inputs(draw)
        q = quantities(evaluate(wq, cs.norm, x, p, operand=precision), reference(name, precision, draw))
        worst = {k: max(worst[k], q[k]) for k in QUANTITIES}
    return worst


def bound(name, precision):
    return {k: FACTOR * v for k, v in noise(name, precision).items()}


# ------------------------------------------------------------------------------------------------ mutants
# Each takes a view dict(w, norm, x, prompt, mask, case) and returns the edited view, or None where the mistake cannot be
# made at this shape (no second tile, P = 1, ff <= 512, ...).  `w` is a private copy; edits touch the weight dict, the
# normalisation vectors, the mask or the inputs, never the oracle.

def causal_mask(L):
    return np.triu(np.ones((L, L), dtype=bool), 1)


def _layers(v):
    return [f"transformer_decoder.layers.{i}." for i in range(v["case"].layers)]


def m_mask_admits_next(v):
    L = v["case"].L
    M = causal_mask(L)
    M[np.arange(L - 1), np.arange(1, L)] = False
    return dict(v, mask=M)


def m_tile_start_misses_own_key(v):
    L = v["case"].L
    qs = [q for q in (32, 64, 96) if q < L]
    if not qs:
        return None
    M = causal_mask(L)
    M[qs, qs] = True
    return dict(v, mask=M)


def m_last_diagonal_tile_unmasked(v):
    L = v["case"].L
    t0 = 32 * ((L - 1) // 32)
    if L - t0 < 2:
        return None
    M = causal_mask(L)
    M[t0:, t0:] = False
    return dict(v, mask=M)


def m_skips_key_tile_0(v):
    L = v["case"].L
    if L <= 32:
        return None
    M = causal_mask(L)
    M[32:, :32] = True
    return dict(v, mask=M)


def m_prompt_positions_shifted(v):
    cs = v["case"]
    pe = v["w"]["pos_encoder.pe"].copy()
    pe[0, cs.ns:cs.ns + cs.P] = v["w"]["pos_encoder.pe"][0, cs.ns + 1:cs.ns + cs.P + 1]
    v["w"]["pos_encoder.pe"] = pe
    return v


def m_last_target_next_position(v):
    cs = v["case"]
    if cs.L >= v["w"]["pos_encoder.pe"].shape[1]:
        return None
    pe = v["w"]["pos_encoder.pe"].copy()
    pe[0, cs.L - 1] = pe[0, cs.L]
    v["w"]["pos_encoder.pe"] = pe
    return v


def m_prompt_rows_reversed(v):
    if v["case"].P < 2:
        return None
    return dict(v, prompt=v["prompt"][:, ::-1].copy())


def m_v_bias_dropped(v):
    for p in _layers(v):
        b = v["w"][p + "self_attn.in_proj_bias"].copy()
        b[2 * D:] = 0
        v["w"][p + "self_attn.in_proj_bias"] = b
    return v


def m_last_ffn_chunk_dropped(v):
    for p in _layers(v):
        for k in ("linear1.weight", "linear1.bias"):          # relu(0) = 0: the chunk contributes nothing
            a = v["w"][p + k].copy()
            a[-32:] = 0
            v["w"][p + k] = a
    return v


def m_b1_high_dropped(v):
    if v["case"].ff <= 512:
        return None
    for p in _layers(v):
        b = v["w"][p + "linear1.bias"].copy()
        b[512:] = 0
        v["w"][p + "linear1.bias"] = b
    return v


def m_b2_dropped(v):
    # the kernel adds b_2 to the residual tiles inside LayerNorm 1 (`extra`), after the operand image is packed
    for p in _layers(v):
        v["w"][p + "linear2.bias"] = np.zeros_like(v["w"][p + "linear2.bias"])
    return v


def m_heads_01_swapped_in_out_proj(v):
    for p in _layers(v):
        a = v["w"][p + "self_attn.out_proj.weight"].copy()
        a[:, :32], a[:, 32:64] = a[:, 32:64].copy(), a[:, :32].copy()
        v["w"][p + "self_attn.out_proj.weight"] = a
    return v


def m_layernorm_variance_over_d_minus_1(v):
    # (x - mu) / sqrt(var d / (d - 1) + eps) is (x - mu) / sqrt(var + eps) sqrt((d - 1) / d) up to eps / var ~ 1e-5 of
    # the 0.4 % it changes: restated as a scale of the LayerNorm weight
    for p in _layers(v):
        for nm in ("norm1.weight", "norm2.weight"):
            v["w"][p + nm] = v["w"][p + nm] * np.sqrt((D - 1) / D)
    return v


def m_x_std_skipped(v):
    return dict(v, norm=dict(v["norm"], x_std=np.ones_like(v["norm"]["x_std"])))


def m_u_channels_swapped_across_32(v):
    # only the de-normalisation y u_std + u_mean of the OUTPUT is meant (the kernel's [b_out | u_std | u_mean] block); the
    # prompt's normalisation reads another block.  Folded into the output head so that the edit stays a weight edit:
    # (h W'^T + b') s + m = (h W^T + b) s' + m'  with  W' = W s'/s,  b' = (b s' + m' - m) / s
    c = v["case"].c
    if c <= 32:
        return None
    s, m = v["norm"]["u_std"], v["norm"]["u_mean"]
    perm = np.arange(c)
    hi = np.arange(32, c)
    perm[hi], perm[hi - 32] = hi - 32, hi
    s2, m2 = s[perm], m[perm]
    W, b = np.asarray(v["w"]["output_linear.weight"], dtype=np.float64), np.asarray(v["w"]["output_linear.bias"], dtype=np.float64)
    v["w"]["output_linear.weight"] = W * (s2 / s)[:, None]
    v["w"]["output_linear.bias"] = (b * s2 + m2 - m) / s
    return v


def m_state_embed_padding_columns_live(v):
    # the kernel pads the state embedding to one 16-deep k-step and reads the inputs past n at a clamped index: live
    # padding columns would add (their sum) x (the last normalised state component)
    n = v["case"].n
    if n >= 16:
        return None
    g = np.random.default_rng(77)
    extra = g.uniform(-1, 1, (D, 16 - n)) / np.sqrt(n)
    a = np.asarray(v["w"]["state_embed.weight"], dtype=np.float64).copy()
    a[:, n - 1] += extra.sum(axis=1)
    v["w"]["state_embed.weight"] = a
    return v


# name -> (kind, edit); kind "mask" / "bias" are the two families of which every case needs a biting member
MUTANTS = {
    "mask_admits_next": ("mask", m_mask_admits_next),
    "tile_start_misses_own_key": ("mask", m_tile_start_misses_own_key),
    "last_diagonal_tile_unmasked": ("mask", m_last_diagonal_tile_unmasked),
    "skips_key_tile_0": ("mask", m_skips_key_tile_0),
    "prompt_positions_shifted": ("position", m_prompt_positions_shifted),
    "last_target_next_position": ("position", m_last_target_next_position),
    "prompt_rows_reversed": ("input", m_prompt_rows_reversed),
    "v_bias_dropped": ("bias", m_v_bias_dropped),
    "last_ffn_chunk_dropped": ("ffn", m_last_ffn_chunk_dropped),
    "b1_high_dropped": ("bias", m_b1_high_dropped),
    "b2_dropped": ("bias", m_b2_dropped),
    "heads_01_swapped_in_out_proj": ("attention", m_heads_01_swapped_in_out_proj),
    "layernorm_variance_over_d_minus_1": ("layernorm", m_layernorm_variance_over_d_minus_1),
    "x_std_skipped": ("norm", m_x_std_skipped),
    "u_channels_swapped_across_32": ("norm", m_u_channels_swapped_across_32),
    "state_embed_padding_columns_live": ("embed", m_state_embed_padding_columns_live),
}


@functools.lru_cache(maxsize=None)
def rounded(name, precision):
    return round_weights(case(name).w, precision)


def view(cs, precision, draw=0):
    x, p = cs.inputs(draw)
    wq = rounded(cs.name, precision) if cs.name in CASE_NAMES else round_weights(cs.w, precision)
    return dict(w=dict(wq), norm=dict(cs.norm), x=x, prompt=p, mask=None, case=cs)


def evaluate_view(v):
    return evaluate(v["w"], v["norm"], v["x"], v["prompt"], mask=v["mask"])


def mutant_shift(cs, mutant, precision="fp16", draw=0, base=None):
    """quantities(mutated fp64 oracle, fp64 oracle) on `cs`, or None where the mutant does not apply.  `cs` is a Case."""
    v = MUTANTS[mutant][1](view(cs, precision, draw))
    if v is None:
        return None
    if base is None:
        base = evaluate_view(view(cs, precision, draw))
    return quantities(evaluate_view(v), base)


@functools.lru_cache(maxsize=None)
def mutant_ratio(name, mutant, precision):
    """max over the three quantities of (shift by the mutant) / bound, or None where the mutant does not apply."""
    q = mutant_shift(case(name), mutant, precision, base=reference(name, precision))
    if q is None:
        return None
    bd = bound(name, precision)
    return max(q[k] / bd[k] for k in QUANTITIES)


def k_bias_dropped(cs, precision="fp16"):
    """The K bias adds a per-query constant to the scores, which the softmax cancels: the kernel omits it."""
    v = view(cs, precision)
    base = evaluate_view(v)
    for p in _layers(v):
        b = v["w"][p + "self_attn.in_proj_bias"].copy()
        b[D:2 * D] = 0
        v["w"][p + "self_attn.in_proj_bias"] = b
    return quantities(evaluate_view(v), base)
