"""Oracle transformer forward from raw weight arrays (NumPy).  TEST INFRASTRUCTURE ONLY.

Restates the reference's predictor
  * quattro_ilqr_tf/transformer_model.py:122-138  TransformerPredictor.forward
  * quattro_ilqr_tf/transformer_model.py:77-80    PositionalEncoding.forward (dropout = identity in eval)
  * quattro_ilqr_tf/transformer_model.py:37-50    DataNormalizer
  * quattro_ilqr_tf/transformer_ilqr.py:311-325   TransformerILQR.predict
and the third-party blocks it is built from (torch.nn.TransformerEncoderLayer as configured there:
batch_first, post-LayerNorm, ReLU, eps 1e-5, additive -inf causal mask, softmax(QK^T/sqrt(hd))V).
torch itself is not used here; the restatement is pinned by tests/golden/tf_*.npz, which hold the
reference module's own outputs on the shipped checkpoints.

Weight dict keys are the reference state_dict names (see tests/golden/make_golden.py: export_weights).
"""
import numpy as np


def hyper_from_weights(w):
    d = w["state_embed.weight"].shape[0]
    n_layers = 0
    while f"transformer_decoder.layers.{n_layers}.linear1.weight" in w:
        n_layers += 1
    return dict(
        d_model=d, state_dim=w["state_embed.weight"].shape[1], control_dim=w["control_embed.weight"].shape[1],
        ff=w["transformer_decoder.layers.0.linear1.weight"].shape[0], n_layers=n_layers,
        target_len=w["target_embedding"].shape[0], max_seq_len=w["pos_encoder.pe"].shape[1])


def _layer_norm(x, g, b, eps=1e-5):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def round_operand(a, operand):
    """`a` rounded (to nearest even) to the 16-bit type `operand` ("bf16" / "fp16") and handed back as fp64; None: `a` itself."""
    if operand is None:
        return a
    a32 = np.ascontiguousarray(a, dtype=np.float32)
    if operand == "fp16":
        return a32.astype(np.float16).astype(np.float64)
    if operand == "bf16":
        bits = a32.view(np.uint32).astype(np.uint64)
        bits = ((bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
        out = bits.view(np.float32).astype(np.float64)
        return np.where(np.isfinite(a32), out, a32.astype(np.float64))
    raise ValueError(f"operand must be None, 'bf16' or 'fp16' (got {operand!r})")


def forward(w, x_norm, prompt_norm, nhead, dtype=np.float64, return_hidden=False, operand=None, mask=None):
    """x_norm (B, N+1, n), prompt_norm (B, P, c) -> (B, T, c) normalised prediction.

    operand : None | "bf16" | "fp16".  Both operands of every matrix product (embeddings, QKV, QK^T, PV, out-projection,
              the two feed-forward products, the output head) are rounded to that type and the product is accumulated in
              fp64; everything else stays fp64.  A noise model of 16-bit matrix operands, not a model of any kernel.
    mask    : (L, L) boolean array, True = key not visible to the query (row); replaces the causal mask."""
    if operand is not None and dtype is not np.float64:
        raise ValueError("operand rounding is defined on the fp64 evaluation only")
    r = lambda a: round_operand(a, operand)
    W = {k: np.asarray(v).astype(dtype) for k, v in w.items()}
    hp = hyper_from_weights(W)
    d, T = hp["d_model"], hp["target_len"]
    x_norm = np.asarray(x_norm, dtype=dtype)
    prompt_norm = np.asarray(prompt_norm, dtype=dtype)
    Bt = x_norm.shape[0]
    x_emb = r(x_norm) @ r(W["state_embed.weight"].T) + W["state_embed.bias"]
    u_emb = r(prompt_norm) @ r(W["control_embed.weight"].T) + W["control_embed.bias"]
    tgt = np.broadcast_to(W["target_embedding"], (Bt, T, d))
    h = np.concatenate([x_emb, u_emb, tgt], axis=1)
    Lseq = h.shape[1]
    h = h + W["pos_encoder.pe"][:, :Lseq]
    hidden = [h.copy()]
    hd = d // nhead
    causal = np.triu(np.ones((Lseq, Lseq), dtype=bool), 1)
    if mask is not None:
        causal = np.asarray(mask, dtype=bool)
        if causal.shape != (Lseq, Lseq):
            raise ValueError(f"mask must be ({Lseq}, {Lseq})")
    for li in range(hp["n_layers"]):
        p = f"transformer_decoder.layers.{li}."
        qkv = r(h) @ r(W[p + "self_attn.in_proj_weight"].T) + W[p + "self_attn.in_proj_bias"]
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        split = lambda a: a.reshape(Bt, Lseq, nhead, hd).transpose(0, 2, 1, 3)
        q, k, v = split(q), split(k), split(v)
        s = (r(q) @ r(k.transpose(0, 1, 3, 2))) / np.sqrt(dtype(hd))
        s = np.where(causal, -np.inf, s)
        s = s - s.max(axis=-1, keepdims=True)
        e = np.exp(s)
        a = e / e.sum(axis=-1, keepdims=True)
        o = (r(a) @ r(v)).transpose(0, 2, 1, 3).reshape(Bt, Lseq, d)
        o = r(o) @ r(W[p + "self_attn.out_proj.weight"].T) + W[p + "self_attn.out_proj.bias"]
        h = _layer_norm(h + o, W[p + "norm1.weight"], W[p + "norm1.bias"])
        f = np.maximum(r(h) @ r(W[p + "linear1.weight"].T) + W[p + "linear1.bias"], 0)
        f = r(f) @ r(W[p + "linear2.weight"].T) + W[p + "linear2.bias"]
        h = _layer_norm(h + f, W[p + "norm2.weight"], W[p + "norm2.bias"])
        hidden.append(h.copy())
    out = r(h[:, -T:, :]) @ r(W["output_linear.weight"].T) + W["output_linear.bias"]
    if return_hidden:
        return out, hidden
    return out


def predict(w, norm, x_seq, kK_seq, nhead, prompt_len, dtype=np.float64, operand=None, mask=None):
    """Single-sample predict(): normalise -> last prompt_len rows -> forward -> de-normalise.
    x_seq (N+1, n), kK_seq (>=P, c) -> (T, c).  `operand`, `mask`: see forward()."""
    x_n = (np.asarray(x_seq) - norm["x_mean"]) / norm["x_std"]
    u_n = (np.asarray(kK_seq) - norm["u_mean"]) / norm["u_std"]
    u_n = u_n[-prompt_len:, :]
    y = forward(w, x_n.astype(np.float32)[None], u_n.astype(np.float32)[None], nhead, dtype=dtype,
                operand=operand, mask=mask)[0]
    return y * norm["u_std"] + norm["u_mean"]
