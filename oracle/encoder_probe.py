"""ORACLE — test infrastructure only.  Never imported by the product package.

A float64 restatement of ``oracle.encoder_ref.encoder_forward`` on PACKED tokens (the layout the kernels run on), written
from ``encoder_ref``, with what a test needs in order to tell a right encoder from a subtly wrong one:

* the hidden states after the embedding LayerNorm and after every layer are returned (boundary 0 .. L), not only the last;
* ``rounding="bf16"`` rounds (``presets.bf16_round``) at the points where the kernels store or consume bf16 — the buffer
  table at the top of ``csrc/encoder.hip`` and ``attention_kernel``:
      x   embedding LayerNorm output and both LayerNorm-epilogue outputs of a layer (so the residual the next epilogue
          reads is the rounded one),
      qkv the fused Q|K|V projection after its bias,
      P   the un-normalised probabilities exp(s - max): the score accumulator is converted to bf16 and is the operand of
          P.V, while the denominator is summed from the unrounded float32 values,
      ctx P.V / l,      h1  GELU(FFN1).
  LayerNorm, softmax and GELU themselves stay unrounded (float32 on the device, float64 here).  Weights are consumed as
  given (the test weights are bf16-exact; the embedding tables, biases and LayerNorm parameters are float32 on the device);
* ``linear``: replaces the float64 ``t @ W.T + b`` of the six projections (``oracle.fp8_ref.mx_linear`` for MXFP8);
* ``defect=<name>``: ONE named departure from the right arithmetic (``DEFECTS``), each a defect a kernel could have.
  ``tests/test_encoder_power_cpu.py`` shows that every one of them moves the output by a multiple of the tolerance.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np
import torch

from text_similarity_amd import presets
from .encoder_ref import mpnet_relative_bucket

DEFECTS = (
    "uniform_softmax",          # softmax replaced by the plain average over the keys
    "no_scale",                 # scores not divided by sqrt(head_dim)
    "scale_half",               # scores divided by 2 sqrt(head_dim)
    "no_rel_bias",              # MPNet relative-position bias left out
    "rel_bias_swapped",         # bucket of (query - key) instead of (key - query)
    "bucket_plus_one",          # bucket index one too large for |distance| >= 8
    "rel_bias_heads_reversed",  # head h reads the bias column of head heads-1-h
    "no_q_bias", "no_k_bias", "no_v_bias", "no_o_bias",
    "var_unbiased",             # LayerNorm variance divided by H - 1
    "eps_1e-5", "eps_1e-12",    # LayerNorm eps of the other architecture
    "pos_plus_one",             # position row one too far (clamped to the table)
    "no_token_type",            # BERT: token-type row 0 not added
    "mpnet_pos_ignores_pad",    # MPNet: position = pad_id + 1 + column, pads counted
    "leak_prev_sequence",       # every query also sees the last token of the preceding sequence of the batch
    "drop_last_key",            # the last key of a sequence with length = 1 (mod 16), length > 1, is left out
    "gelu_tanh",                # tanh approximation instead of erf
    "drop_last_head_group",     # context of the heads >= 4 (heads // 4) is zero: a wrong bound on attention's partial group of 4 heads
    "ffn_tail_dropped",         # the last F % 128 (when that is 0: the last 64) features of GELU(FFN1) are zero: a wrong N edge of a tile
)


def _t64(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(presets.bf16_round(t.numpy().astype(np.float32))).double()


def _layer_norm(x, g, b, eps, unbiased=False):
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    var = (d * d).sum(-1, keepdim=True) / (x.shape[-1] - (1 if unbiased else 0))
    return d / torch.sqrt(var + eps) * g + b


def _gelu(x, tanh=False):
    if tanh:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def packed_positions(cfg, flat_ids: np.ndarray, cu: np.ndarray):
    """(position rows, columns) of packed tokens, as ``encoder_ref`` derives them for a right-padded batch."""
    flat_ids = np.asarray(flat_ids).astype(np.int64)
    cu = np.asarray(cu).astype(np.int64)
    cols = np.zeros(flat_ids.size, dtype=np.int64)
    pos = np.zeros(flat_ids.size, dtype=np.int64)
    for s in range(cu.size - 1):
        a, b = cu[s], cu[s + 1]
        cols[a:b] = np.arange(b - a)
        if cfg.arch == "mpnet":
            ne = (flat_ids[a:b] != cfg.pad_id).astype(np.int64)
            pos[a:b] = np.cumsum(ne) * ne + cfg.pad_id
        else:
            pos[a:b] = cols[a:b]
    return pos, cols


def pack_padded(cfg, input_ids: np.ndarray, attention_mask: np.ndarray):
    """Padded [B,S] ids + mask -> (flat ids, cu, position rows, columns) of the live tokens; MPNet positions count over
    the whole padded row, as ``encoder_ref`` does."""
    ids = np.asarray(input_ids).astype(np.int64)
    m = np.asarray(attention_mask).astype(bool)
    B, S = ids.shape
    col = np.broadcast_to(np.arange(S), (B, S))
    if cfg.arch == "mpnet":
        ne = (ids != cfg.pad_id).astype(np.int64)
        pos = np.cumsum(ne, 1) * ne + cfg.pad_id
    else:
        pos = col
    cu = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(m.sum(1), out=cu[1:])
    return ids[m], cu, pos[m], col[m]


def probe_forward(cfg, w: Dict[str, np.ndarray], flat_ids, cu, *, rounding: Optional[str] = None,
                  defect: Optional[str] = None, linear=None, num_layers: Optional[int] = None, pos=None, cols=None,
                  stats: Optional[dict] = None) -> List[torch.Tensor]:
    """Hidden states [T, H] float64 at boundary 0 (embedding LayerNorm) .. L (after layer L) for packed ``flat_ids`` [T]
    and ``cu`` [B+1].  ``stats`` (a dict) receives, per layer, the largest probability of every (sequence, head, query)
    as ``softmax_max`` [(sequence length, values)] and the largest |FFN1 pre-activation| as ``ffn1_absmax``."""
    assert rounding in (None, "bf16"), rounding
    assert defect is None or defect in DEFECTS, defect
    rnd = _bf16 if rounding == "bf16" else (lambda t: t)
    flat_ids = np.asarray(flat_ids).astype(np.int64)
    cu = np.asarray(cu).astype(np.int64)
    L = cfg.num_layers if num_layers is None else num_layers
    H, nh, dh = cfg.hidden, cfg.heads, cfg.head_dim
    if pos is None or cols is None:
        p_, c_ = packed_positions(cfg, flat_ids, cu)
        pos = p_ if pos is None else np.asarray(pos).astype(np.int64)
        cols = c_ if cols is None else np.asarray(cols).astype(np.int64)
    if defect == "mpnet_pos_ignores_pad":
        assert cfg.arch == "mpnet"
        pos = cols + cfg.pad_id + 1
    if defect == "pos_plus_one":
        pos = np.minimum(pos + 1, cfg.max_pos - 1)
    eps = {"eps_1e-5": 1e-5, "eps_1e-12": 1e-12}.get(defect, cfg.ln_eps)
    unb = defect == "var_unbiased"
    g = lambda name: _t64(w[name])

    def lin(t, name, bias=True):
        if linear is None:
            y = t @ g(name + ".weight").T
            return y + g(name + ".bias") if bias else y
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        b = w[name + ".bias"]
        return linear(t, f32(w[name + ".weight"]), f32(b if bias else np.zeros_like(b))).double()

    x = g("embeddings.word_embeddings.weight")[flat_ids]
    if cfg.arch == "bert" and defect != "no_token_type":
        x = x + g("embeddings.token_type_embeddings.weight")[0]
    x = x + g("embeddings.position_embeddings.weight")[pos]
    x = rnd(_layer_norm(x, g("embeddings.LayerNorm.weight"), g("embeddings.LayerNorm.bias"), eps, unb))
    out = [x]

    table = None
    if cfg.arch == "mpnet" and defect != "no_rel_bias":
        table = g("encoder.relative_attention_bias.weight")            # [buckets, heads]
        if defect == "rel_bias_heads_reversed":
            table = table.flip(1)
    scale = 1.0 / math.sqrt(dh)
    if defect == "no_scale":
        scale = 1.0
    if defect == "scale_half":
        scale *= 0.5

    def rel_bias(qc, kc):                                              # [heads, len(qc), len(kc)]
        rel = torch.as_tensor(kc)[None, :] - torch.as_tensor(qc)[:, None]
        if defect == "rel_bias_swapped":
            rel = -rel
        b = mpnet_relative_bucket(rel, cfg.rel_buckets)
        if defect == "bucket_plus_one":
            b = torch.where(rel.abs() >= 8, torch.clamp(b + 1, max=cfg.rel_buckets - 1), b)
        return table[b].permute(2, 0, 1)

    for l in range(L):
        p = f"encoder.layer.{l}."
        if cfg.arch == "bert":
            nq, nk, nv, no = (p + "attention.self.query", p + "attention.self.key",
                              p + "attention.self.value", p + "attention.output.dense")
            ln1 = p + "attention.output.LayerNorm"
        else:
            nq, nk, nv, no = (p + "attention.attn.q", p + "attention.attn.k",
                              p + "attention.attn.v", p + "attention.attn.o")
            ln1 = p + "attention.LayerNorm"
        T = x.shape[0]
        q = rnd(lin(x, nq, defect != "no_q_bias")).view(T, nh, dh)
        k = rnd(lin(x, nk, defect != "no_k_bias")).view(T, nh, dh)
        v = rnd(lin(x, nv, defect != "no_v_bias")).view(T, nh, dh)
        ctx = torch.zeros(T, nh, dh, dtype=torch.float64)
        for s in range(cu.size - 1):
            a, b = int(cu[s]), int(cu[s + 1])
            S = b - a
            if S == 0:
                continue
            keys = np.arange(a, b)
            kcol = cols[a:b]
            if defect == "drop_last_key" and S % 16 == 1 and S > 1:
                keys, kcol = keys[:-1], kcol[:-1]
            if defect == "leak_prev_sequence" and a > 0:
                keys, kcol = np.concatenate([[a - 1], keys]), np.concatenate([[cols[a] - 1], kcol])
            qs = q[a:b].transpose(0, 1)                                 # [heads, S, dh]
            sc = torch.matmul(qs, k[keys].permute(1, 2, 0)) * scale     # [heads, S, keys]
            if table is not None:
                sc = sc + rel_bias(cols[a:b], kcol)
            if defect == "uniform_softmax":
                sc = torch.zeros_like(sc)
            e = torch.exp(sc - sc.max(-1, keepdim=True).values)
            den = e.sum(-1, keepdim=True)
            if stats is not None:
                stats.setdefault("softmax_max", []).append((S, (1.0 / den).reshape(-1).numpy()))
            o = torch.matmul(rnd(e), v[keys].transpose(0, 1)) / den     # [heads, S, dh]
            ctx[a:b] = o.transpose(0, 1)
        if defect == "drop_last_head_group":
            ctx[:, 4 * (nh // 4):] = 0.0
        ctx = rnd(ctx.reshape(T, H))
        x1 = rnd(_layer_norm(lin(ctx, no, defect != "no_o_bias") + x, g(ln1 + ".weight"), g(ln1 + ".bias"), eps, unb))
        pre = lin(x1, p + "intermediate.dense")
        if stats is not None:
            stats.setdefault("ffn1_absmax", []).append(float(pre.abs().max()) if T else 0.0)
        h1 = rnd(_gelu(pre, defect == "gelu_tanh"))
        if defect == "ffn_tail_dropped":
            h1[:, cfg.ffn - (cfg.ffn % 128 or 64):] = 0.0
        x = rnd(_layer_norm(lin(h1, p + "output.dense") + x1, g(p + "output.LayerNorm.weight"),
                            g(p + "output.LayerNorm.bias"), eps, unb))
        out.append(x)
    return out


def mean_pool_packed(hidden: torch.Tensor, cu) -> torch.Tensor:
    """Mean over each sequence's tokens, float64 [B, H]; an empty sequence gives a zero row (``encoder_ref.mean_pool``)."""
    cu = np.asarray(cu).astype(np.int64)
    out = torch.zeros(cu.size - 1, hidden.shape[1], dtype=torch.float64)
    for s in range(cu.size - 1):
        if cu[s + 1] > cu[s]:
            out[s] = hidden[cu[s]:cu[s + 1]].double().mean(0)
    return out
