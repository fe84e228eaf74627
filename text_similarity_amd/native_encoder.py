"""NativeEncoder — the object that stands where the reference keeps a HuggingFace ``AutoModel``
(``context_embedder``, /root/reference/src/models/modeling.py:25,
/root/reference/src/models/sentence_encoder.py:33,107-108,118).

It owns a ``tsim_encoder`` handle of libtsim.so (weights in HBM as bf16, activation workspace) and runs the
encoder forward on *packed* tokens.  ``__call__(input_ids=..., attention_mask=...)`` keeps the HF contract the
wrappers rely on: element ``[0]`` of the result is ``last_hidden_state`` of shape ``[B, S, H]``.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops
from .presets import EncoderConfig, PRESETS, synthetic_weights


def _f32(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().float().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def layer_names(cfg: EncoderConfig, l: int) -> Dict[str, str]:
    p = f"encoder.layer.{l}."
    if cfg.arch == "bert":
        a = {"q": p + "attention.self.query", "k": p + "attention.self.key", "v": p + "attention.self.value",
             "o": p + "attention.output.dense", "ln1": p + "attention.output.LayerNorm"}
    else:
        a = {"q": p + "attention.attn.q", "k": p + "attention.attn.k", "v": p + "attention.attn.v",
             "o": p + "attention.attn.o", "ln1": p + "attention.LayerNorm"}
    a.update({"f1": p + "intermediate.dense", "f2": p + "output.dense", "ln2": p + "output.LayerNorm"})
    return a


def config_c(cfg: EncoderConfig, max_tokens: int, max_seqs: int, weight_dtype: str = "bf16") -> "_lib.EncoderConfigC":
    if cfg.arch not in ("bert", "mpnet") or cfg.pos_offset not in (0, cfg.pad_id + 1) or (cfg.pos_offset and cfg.arch != "bert"):
        raise ValueError(f"arch {cfg.arch!r} with pos_offset {cfg.pos_offset} (pad_id {cfg.pad_id}): position rows start "
                         "at 0 (BERT, DistilBERT) or at pad_id + 1 (MPNet, RoBERTa family)")
    arch = _lib.ARCH_MPNET if cfg.arch == "mpnet" else _lib.ARCH_ROBERTA if cfg.pos_offset else _lib.ARCH_BERT
    return _lib.EncoderConfigC(arch=arch, num_layers=cfg.num_layers, hidden=cfg.hidden, heads=cfg.heads, ffn=cfg.ffn,
                               vocab=cfg.vocab, max_pos=cfg.max_pos, pad_id=cfg.pad_id, rel_buckets=cfg.rel_buckets,
                               ln_eps=cfg.ln_eps, max_tokens=max_tokens, max_seqs=max_seqs,
                               weight_dtype=_lib.W_MXFP8 if weight_dtype == "mxfp8" else _lib.W_BF16)


def encoder_route(cfg: EncoderConfig, tokens: int, layer: int = 0, weight_dtype: str = "bf16") -> SimpleNamespace:
    """The kernels an encoder of ``cfg`` runs in layer ``layer`` of a forward of ``tokens`` tokens (tsim_encoder_route_host: no
    GPU, nothing is created): family, form[4] (QKV, O, FFN1, FFN2), images, buffers, chain_blocks, qkv_chained and
    segments = ([(form, row0, rows), ...] of O, ... of FFN2), in the constants of ``_lib``.  A configuration that
    ``NativeEncoder`` would refuse raises the same ValueError."""
    r = _lib.EncoderRouteC()
    cc = config_c(cfg, max(int(tokens), 1), 1, weight_dtype)
    _lib.check(_lib.lib().tsim_encoder_route_host(C.byref(cc), int(tokens), int(layer), C.byref(r)), "encoder_route_host")
    return SimpleNamespace(family=r.family, form=list(r.form), images=r.images, buffers=r.buffers, chain_blocks=r.chain_blocks,
                           qkv_chained=bool(r.qkv_chained),
                           segments=tuple([(s.form, s.row0, s.rows) for s in r.seg[i][:r.n_seg[i]]] for i in range(2)))


class SentenceHead:
    """What the native forward runs after the last layer instead of the mean pool (include/tsim.h tsim_sentence_head):
    a pooling mode ('mean' | 'cls' | 'max' | 'mean_sqrt_len'), an optional Dense (``dense_w`` [d_out, hidden] and
    ``dense_b`` [d_out] float32 tensors on the encoder's device, ``act`` 'identity' | 'tanh') and an optional Normalize."""

    def __init__(self, mode="mean", dense_w: Optional[torch.Tensor] = None, dense_b: Optional[torch.Tensor] = None,
                 act="identity", normalize: bool = False):
        self.mode = ops.pool_mode_id(mode)
        self.act = ops.activation_id(act)
        self.normalize = bool(normalize)
        if dense_w is None and dense_b is not None:
            raise ValueError("a Dense bias needs a Dense weight")
        for t in (dense_w, dense_b):
            if t is not None:
                ops._need_gpu(t)
                if t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError("Dense weights must be contiguous float32 device tensors")
        if dense_w is not None and (dense_w.dim() != 2 or (dense_b is not None and tuple(dense_b.shape) != (dense_w.shape[0],))):
            raise ValueError(f"Dense shapes {tuple(dense_w.shape)} / {None if dense_b is None else tuple(dense_b.shape)}")
        self.dense_w, self.dense_b = dense_w, dense_b

    def width(self, hidden: int) -> int:
        return int(self.dense_w.shape[0]) if self.dense_w is not None else int(hidden)

    def c_struct(self, hidden: int) -> "_lib.SentenceHeadC":
        if self.dense_w is not None and self.dense_w.shape[1] != hidden:
            raise ValueError(f"Dense in_features {self.dense_w.shape[1]} != hidden {hidden}")
        return _lib.SentenceHeadC(pool_mode=self.mode, d_out=self.width(hidden) if self.dense_w is not None else 0,
                                  dense_w=self.dense_w.data_ptr() if self.dense_w is not None else None,
                                  dense_b=self.dense_b.data_ptr() if self.dense_b is not None else None,
                                  dense_act=self.act, normalize=int(self.normalize))


class NativeEncoder:
    def __init__(self, cfg: EncoderConfig, weights: Dict[str, np.ndarray], max_tokens: int = 65536,
                 max_seqs: int = 8192, device: Optional[torch.device] = None, weight_dtype: str = "bf16"):
        """``weight_dtype``: "bf16" (default) or "mxfp8" — projections on OCP MXFP8 operands (e4m3 + one power-of-two
        scale per 32 elements) through the block-scaled fp8 MFMA; base-size models only (hidden, ffn % 256 == 0)."""
        if weight_dtype not in ("bf16", "mxfp8"):
            raise ValueError(f"weight_dtype must be 'bf16' or 'mxfp8', got {weight_dtype!r}")
        self.weight_dtype = weight_dtype
        if not torch.cuda.is_available():
            raise _lib.TsimError("NativeEncoder needs an MI355X: torch.cuda.is_available() is False and "
                                 "there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.max_tokens, self.max_seqs = int(max_tokens), int(max_seqs)
        # what BaseEncoderModel.config / get_sentence_embedding_dimension read (modeling.py:65-77)
        self.config = SimpleNamespace(hidden_size=cfg.hidden, dim=cfg.hidden, num_hidden_layers=cfg.num_layers,
                                      num_attention_heads=cfg.heads, intermediate_size=cfg.ffn,
                                      vocab_size=cfg.vocab, max_position_embeddings=cfg.max_pos,
                                      model_type=cfg.source_type)
        w = {k: _f32(v) for k, v in weights.items() if not k.endswith("position_ids")}
        keep = []
        layers = (_lib.LayerWeightsC * cfg.num_layers)()
        for l in range(cfg.num_layers):
            n = layer_names(cfg, l)
            lw = layers[l]
            for field, key in (("wq", n["q"] + ".weight"), ("bq", n["q"] + ".bias"), ("wk", n["k"] + ".weight"),
                               ("bk", n["k"] + ".bias"), ("wv", n["v"] + ".weight"), ("bv", n["v"] + ".bias"),
                               ("wo", n["o"] + ".weight"), ("bo", n["o"] + ".bias"),
                               ("ln1_g", n["ln1"] + ".weight"), ("ln1_b", n["ln1"] + ".bias"),
                               ("w1", n["f1"] + ".weight"), ("b1", n["f1"] + ".bias"),
                               ("w2", n["f2"] + ".weight"), ("b2", n["f2"] + ".bias"),
                               ("ln2_g", n["ln2"] + ".weight"), ("ln2_b", n["ln2"] + ".bias")):
                if key not in w:
                    raise KeyError(f"missing weight {key}")
                keep.append(w[key])
                setattr(lw, field, _ptr(w[key]))
        ew = _lib.EncoderWeightsC()
        ew.word_emb = _ptr(w["embeddings.word_embeddings.weight"])
        ew.pos_emb = _ptr(w["embeddings.position_embeddings.weight"])
        if cfg.arch == "bert" and cfg.type_vocab > 0:   # (DistilBERT has none; RoBERTa's single row is added to every token)
            ew.type_emb = _ptr(w["embeddings.token_type_embeddings.weight"])
        ew.emb_ln_g = _ptr(w["embeddings.LayerNorm.weight"])
        ew.emb_ln_b = _ptr(w["embeddings.LayerNorm.bias"])
        if cfg.arch == "mpnet":
            ew.rel_bias = _ptr(w["encoder.relative_attention_bias.weight"])
        ew.layers = layers
        cc = config_c(cfg, self.max_tokens, self.max_seqs, weight_dtype)
        handle = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tsim_encoder_create(C.byref(cc), C.byref(ew), C.byref(handle)), "encoder_create")
        self._h = handle
        self.n_types = 0
        self.num_labels = 0
        if cfg.source_type == "bert":   # the whole token-type table: sentence pairs use row 1 (untyped forwards keep adding row 0)
            tt = w["embeddings.token_type_embeddings.weight"]
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().tsim_encoder_set_token_types(handle, _ptr(tt), tt.shape[0]), "encoder_set_token_types")
            self.n_types = int(tt.shape[0])
        self._weights_host = w  # float32 source weights: what save_pretrained writes (the handle holds bf16 / fp8 copies)

    def set_cls_head(self, pool_w, pool_b, cls_w, cls_b, act="tanh") -> None:
        """HF BertForSequenceClassification head: ``bert.pooler.dense`` (pool_w [H,H], pool_b [H]) and ``classifier``
        (cls_w [num_labels,H], cls_b [num_labels]), float32, 1 <= num_labels <= 32.  BERT only (its graph: not MPNet).
        ``act``: 'tanh', or 'relu' for DistilBertForSequenceClassification's ``pre_classifier`` / ``classifier``; the RoBERTa
        family's ``classifier.dense`` / ``classifier.out_proj`` is the tanh form."""
        if act not in ("tanh", "relu"):
            raise ValueError(f"classification-head activation {act!r} (tanh, relu)")
        pw, pb, cw, cb = (_f32(a) for a in (pool_w, pool_b, cls_w, cls_b))
        H = self.cfg.hidden
        n = cw.shape[0] if cw.ndim == 2 else 0
        if pw.shape != (H, H) or pb.shape != (H,) or cw.shape != (n, H) or cb.shape != (n,):
            raise ValueError(f"head shapes {pw.shape} {pb.shape} {cw.shape} {cb.shape} do not fit hidden={H}")
        with torch.cuda.device(self.device):
            if act == "tanh":
                _lib.check(_lib.lib().tsim_encoder_set_cls_head(self._h, _ptr(pw), _ptr(pb), _ptr(cw), _ptr(cb), n),
                           "encoder_set_cls_head")
            else:
                _lib.check(_lib.lib().tsim_encoder_set_cls_head_act(self._h, _ptr(pw), _ptr(pb), _ptr(cw), _ptr(cb), n,
                                                                    _lib.ACT_RELU), "encoder_set_cls_head")
        self.num_labels = n

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_preset(cls, preset: str, **kw) -> "NativeEncoder":
        """Architecture preset with regenerable synthetic weights (no checkpoints exist offline)."""
        return cls(PRESETS[preset], synthetic_weights(preset), **kw)

    @classmethod
    def from_pretrained(cls, path: str, **kw) -> "NativeEncoder":
        """Local HF directory: config.json + model.safetensors (or pytorch_model.bin, loaded weights_only)."""
        from .weights import load_hf_dir
        cfg, w = load_hf_dir(path)
        return cls(cfg, w, **kw)

    def save_pretrained(self, path: str) -> None:
        """config.json + model.safetensors of the float32 source weights (what ``from_pretrained(path)`` reads back) — the
        ``context_embedder.save_pretrained(path)`` of /root/reference/src/models/modeling.py:56."""
        from .weights import save_hf_dir
        save_hf_dir(path, self.cfg, self._weights_host)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().tsim_encoder_destroy(h)
            except Exception:
                pass

    # ------------------------------------------------------------------ input validation
    ERR_BITS = {1: "a token id outside [0, vocab_size)", 2: "a position id outside the position table",
                4: "a sequence longer than the max_len passed to forward_packed", 8: "a token type id outside the type table",
                16: "a span position outside its sequence, or a span outside the batch"}

    @staticmethod
    def check_lengths(cfg: EncoderConfig, max_len: int) -> None:
        """HF raises IndexError when a sequence needs a position row the table does not have: BERT rows 0..len-1, MPNet and
        the RoBERTa family rows pad_id+1..pad_id+len (max_pos 514 holds 512 tokens).  Raised here, before any launch."""
        need = int(max_len) + cfg.first_pos
        if need > cfg.max_pos:
            raise ValueError(f"sequences of {max_len} tokens need position rows up to {need - 1}; "
                             f"{cfg.source_type} table has {cfg.max_pos} (max {cfg.max_pos - need + int(max_len)} tokens)")

    def check(self) -> None:
        """Raise if any forward since the last check saw an out-of-range token id / type id / position id or a sequence longer than
        its promised max_len (the kernels clamp and go on; HF would have raised IndexError).  Synchronises the stream."""
        flags = C.c_int32(0)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tsim_encoder_error_flags(self._h, C.byref(flags),
                                                           torch.cuda.current_stream(self.device).cuda_stream), "encoder_error_flags")
        if flags.value:
            what = "; ".join(msg for bit, msg in self.ERR_BITS.items() if flags.value & bit)
            raise IndexError(f"encoder input out of range: {what}")

    # torch.nn.Module-ish no-ops used by the reference wrappers (`self.to(device)`, `self.eval()`)
    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def parameters(self):
        return iter(())

    # ------------------------------------------------------------------ packed forward
    def positions(self, flat_ids: torch.Tensor, cu: torch.Tensor, cols: Optional[torch.Tensor] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
        """(position-embedding rows, padded-batch columns) for packed tokens.
        BERT, DistilBERT: row = column (bert_of_theseus.py:199-200).  MPNet and the RoBERTa family: cumsum(ids != pad) *
        (ids != pad) + pad over the tokens present (create_position_ids_from_input_ids), i.e. pad + 1 + column unless the
        pad id occurs inside a sequence."""
        T = flat_ids.numel()
        seq_of = torch.repeat_interleave(torch.arange(cu.numel() - 1, device=cu.device), (cu[1:] - cu[:-1]).long(),
                                         output_size=T)
        if cols is None:
            cols = torch.arange(T, device=cu.device, dtype=torch.int32) - cu[seq_of.long()].to(torch.int32)
        if self.cfg.first_pos == 0:
            return cols.to(torch.int32), cols.to(torch.int32)
        ne = (flat_ids != self.cfg.pad_id).to(torch.int32)
        csum = torch.cumsum(ne, 0, dtype=torch.int32)
        start = torch.zeros(cu.numel() - 1, dtype=torch.int32, device=cu.device)
        if T:
            excl = csum - ne
            start = excl[cu[:-1].clamp(max=max(T - 1, 0)).long()]
        pos = (csum - start[seq_of.long()]) * ne + self.cfg.pad_id
        return pos.to(torch.int32), cols.to(torch.int32)

    def forward_packed(self, flat_ids: torch.Tensor, cu: torch.Tensor, pos: Optional[torch.Tensor] = None,
                       cols: Optional[torch.Tensor] = None, max_len: Optional[int] = None, pooled: bool = True,
                       unit: bool = False, hidden: bool = False, rho: Optional[torch.Tensor] = None,
                       types: Optional[torch.Tensor] = None, logits: bool = False, head: Optional[SentenceHead] = None,
                       spans=None):
        """flat_ids int32 [T], cu int32 [B+1] on the GPU.  Returns dict with 'pooled' f32 [B,H],
        'unit' float16 [B,pad_dim(H)] (L2-normalised rows for the search kernel), 'hidden' bf16 [T,H], 'logits' f32
        [B, num_labels] (the head of ``set_cls_head`` on each sequence's first token) as requested.
        ``rho``: a device float32 word raised to the largest rounding residual of the unit rows (ops.l2norm_rows).
        ``types``: int32 [T] token-type ids (BERT; None = all 0).
        ``head``: a :class:`SentenceHead` run in place of the mean pool: 'pooled' is then its final rows [B, head.width(H)] and
        'unit' their unit rows (tsim_encoder_forward_head); not with ``logits``.
        ``spans``: what :meth:`forward_spans` passes down (the span table and which span outputs to make)."""
        ops._need_gpu(flat_ids, cu)
        flat_ids = flat_ids.to(torch.int32).contiguous()
        cu = cu.to(torch.int32).contiguous()
        T, B = flat_ids.numel(), cu.numel() - 1
        if pos is None:
            pos, cols2 = self.positions(flat_ids, cu, cols)
            cols = cols2 if cols is None else cols
        pos = pos.to(torch.int32).contiguous()
        cols = None if cols is None else cols.to(torch.int32).contiguous()
        if types is not None:
            ops._need_gpu(types)
            if self.n_types == 0:
                raise ValueError(f"token type ids need a token-type table; {self.cfg.source_type} has none")
            types = types.to(torch.int32).contiguous()
            if types.numel() != T:
                raise ValueError(f"types has {types.numel()} entries for {T} tokens")
        if logits and self.num_labels == 0:
            raise ValueError("logits need a classification head: call set_cls_head first")
        if max_len is None:   # longest sequence in the batch: sizes the attention grid (one host sync; pass it to avoid)
            max_len = int((cu[1:] - cu[:-1]).max().item()) if B else 0
        self.check_lengths(self.cfg, max_len)
        if head is not None and logits:
            raise ValueError("a sentence head and logits are separate forwards")
        if head is not None and spans is not None:
            raise ValueError("a sentence head and spans are separate forwards")
        H = self.cfg.hidden
        W = head.width(H) if head is not None else H
        out = {}
        dev = flat_ids.device
        p = torch.empty((B, W), dtype=torch.float32, device=dev) if pooled else None
        u = torch.empty((B, ops.pad_dim(W)), dtype=ops.UNIT_DTYPE, device=dev) if unit else None
        hd = torch.empty((T, H), dtype=torch.bfloat16, device=dev) if hidden else None
        lg = torch.empty((B, self.num_labels), dtype=torch.float32, device=dev) if logits else None
        if spans is not None:
            sseq, scu, stok, want_f32, want_unit, srho = spans
            ops._need_gpu(sseq, scu, stok, flat_ids)
            sseq, scu, stok = (t.to(torch.int32).contiguous() for t in (sseq, scu, stok))
            S = sseq.numel()
            if scu.numel() != S + 1:
                raise ValueError(f"span_cu has {scu.numel()} entries for {S} spans (needs S + 1)")
            sp = torch.empty((S, H), dtype=torch.float32, device=dev) if want_f32 else None
            su = torch.empty((S, ops.pad_dim(H)), dtype=ops.UNIT_DTYPE, device=dev) if want_unit else None
        with torch.cuda.device(dev):
            if head is not None:
                hc = head.c_struct(H)
                if head.dense_w is not None and head.dense_w.device != dev:
                    raise ValueError(f"Dense weights on {head.dense_w.device}, tokens on {dev}")
                _lib.check(_lib.lib().tsim_encoder_forward_head(
                    self._h, flat_ids.data_ptr(), types.data_ptr() if types is not None else None, pos.data_ptr(),
                    cols.data_ptr() if cols is not None else None, cu.data_ptr(), T, B, int(max_len), C.byref(hc),
                    p.data_ptr() if p is not None else None, u.data_ptr() if u is not None else None, u.shape[1] if u is not None else 0,
                    rho.data_ptr() if (rho is not None and u is not None) else None, hd.data_ptr() if hd is not None else None,
                    torch.cuda.current_stream(dev).cuda_stream), "encoder_forward_head")
            elif spans is not None:
                _lib.check(_lib.lib().tsim_encoder_forward_spans(
                    self._h, flat_ids.data_ptr(), types.data_ptr() if types is not None else None, pos.data_ptr(),
                    cols.data_ptr() if cols is not None else None,
                    cu.data_ptr(), T, B, int(max_len), p.data_ptr() if p is not None else None,
                    u.data_ptr() if u is not None else None, u.shape[1] if u is not None else 0,
                    rho.data_ptr() if (rho is not None and u is not None) else None,
                    hd.data_ptr() if hd is not None else None, lg.data_ptr() if lg is not None else None,
                    sseq.data_ptr(), scu.data_ptr(), stok.data_ptr() if stok.numel() else None, S, stok.numel(),
                    sp.data_ptr() if sp is not None else None, su.data_ptr() if su is not None else None,
                    su.shape[1] if su is not None else 0, srho.data_ptr() if (srho is not None and su is not None) else None,
                    torch.cuda.current_stream(dev).cuda_stream), "encoder_forward_spans")
                if want_f32:
                    out["spans"] = sp
                if want_unit:
                    out["span_unit"] = su
            else:
                _lib.check(_lib.lib().tsim_encoder_forward_ex(
                    self._h, flat_ids.data_ptr(), types.data_ptr() if types is not None else None, pos.data_ptr(),
                    cols.data_ptr() if cols is not None else None,
                    cu.data_ptr(), T, B, int(max_len), p.data_ptr() if p is not None else None,
                    u.data_ptr() if u is not None else None, u.shape[1] if u is not None else 0,
                    rho.data_ptr() if (rho is not None and u is not None) else None,
                    hd.data_ptr() if hd is not None else None, lg.data_ptr() if lg is not None else None,
                    torch.cuda.current_stream(dev).cuda_stream),
                    "encoder_forward")
        if pooled:
            out["pooled"] = p
        if unit:
            out["unit"] = u
        if hidden:
            out["hidden"] = hd
        if logits:
            out["logits"] = lg
        return out

    def forward_spans(self, flat_ids: torch.Tensor, cu: torch.Tensor, span_seq: torch.Tensor, span_cu: torch.Tensor,
                      span_tok: torch.Tensor, span_out: bool = True, span_unit: bool = False,
                      span_rho: Optional[torch.Tensor] = None, pooled: bool = False, **kw):
        """The packed forward plus word-in-context embeddings (tsim_encoder_forward_spans): span ``s`` belongs to sequence
        ``span_seq[s]`` and lists the token positions ``span_tok[span_cu[s]:span_cu[s+1]]`` inside it (0 = the first token,
        [CLS]; any order, repeats count as often as listed), all int32 on the GPU (word_spans.span_table builds them).
        Adds to the result of :meth:`forward_packed` (whose other arguments pass through ``kw``; no ``head``):
        'spans' f32 [S, H] = the mean of the final hidden states over each list (an empty list gives a zero row) and
        'span_unit' float16 [S, pad_dim(H)] = ops.l2norm_rows of those rows, with ``span_rho`` raised as it raises ``rho``.
        An out-of-range position or sequence is clamped, computed anyway and reported by :meth:`check`."""
        if span_rho is not None:
            ops._check_rho(span_rho, flat_ids.device)
        return self.forward_packed(flat_ids, cu, pooled=pooled, spans=(span_seq, span_cu, span_tok, bool(span_out),
                                                                       bool(span_unit), span_rho), **kw)

    # ------------------------------------------------------------------ padded (HF-style) call
    @staticmethod
    def pack(input_ids: torch.Tensor, attention_mask: torch.Tensor):
        m = attention_mask.bool()
        lens = m.sum(1)
        cu = torch.zeros(m.shape[0] + 1, dtype=torch.int32, device=m.device)
        cu[1:] = torch.cumsum(lens, 0)
        nz = m.nonzero(as_tuple=False)          # row-major: exactly the packed order
        flat = input_ids[m].to(torch.int32)
        cols = nz[:, 1].to(torch.int32)
        return flat, cu, cols, nz

    def __call__(self, input_ids=None, attention_mask=None, token_type_ids=None, **kwargs):
        """HF AutoModel contract used by the wrappers: returns (last_hidden_state [B,S,H] float32,).
        Positions whose mask is 0 come back as zeros (the reference never reads them: the pooler multiplies
        by the mask, modules.py:165).  ``token_type_ids`` [B,S] (BERT) selects the token-type row of each token; None or
        all zeros is the untyped forward; an architecture without a row for a non-zero id (MPNet, DistilBERT, the RoBERTa
        family) refuses it."""
        ops._need_gpu(input_ids)
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        B, S = input_ids.shape
        flat, cu, cols, nz = self.pack(input_ids, attention_mask)
        types = None
        if token_type_ids is not None:
            if tuple(token_type_ids.shape) != (B, S):
                raise ValueError(f"token_type_ids shape {tuple(token_type_ids.shape)} != input_ids shape {(B, S)}")
            ops._need_gpu(token_type_ids)
            types = token_type_ids[attention_mask.bool()].to(torch.int32)
            if self.n_types == 0 and bool((types != 0).any()):   # (RoBERTa's one row is row 0, added to every token)
                raise ValueError(f"{self.cfg.source_type} has no token-type table: token_type_ids must be None or all zeros")
            if self.n_types == 0:
                types = None
        if self.cfg.first_pos:
            # MPNet, RoBERTa family: position ids come from input_ids over the WHOLE padded row (masked non-pad tokens count too)
            ne = (input_ids != self.cfg.pad_id).to(torch.int32)
            pos_full = torch.cumsum(ne, 1, dtype=torch.int32) * ne + self.cfg.pad_id
            pos = pos_full[attention_mask.bool()].to(torch.int32)
        else:
            pos = cols
        out = torch.zeros((B, S, self.cfg.hidden), dtype=torch.float32, device=input_ids.device)
        T = flat.numel()
        for s in range(0, max(B, 1), self.max_seqs):  # capacity-sized slices of the batch
            e = min(B, s + self.max_seqs)
            t0, t1 = int(cu[s]), int(cu[e])
            if t1 - t0 > self.max_tokens:
                raise ValueError(f"batch slice has {t1 - t0} tokens > encoder capacity {self.max_tokens}")
            if t1 > t0:
                r = self.forward_packed(flat[t0:t1], (cu[s:e + 1] - cu[s]), pos[t0:t1], cols[t0:t1], S,
                                        pooled=False, hidden=True, types=None if types is None else types[t0:t1])
                out[nz[t0:t1, 0], nz[t0:t1, 1]] = r["hidden"].float()
        return (out,)
