"""`CXRBertModel` on the cxrk HIP kernels.

Same class hierarchy, constructor, method names, outputs and parameter names as the reference's
`health_multimodal/text/model/modelling_cxrbert.py` (`BertProjectionHead` :28-49, `CXRBertModel` :52-141), so
checkpoints load with `load_state_dict`/`from_pretrained` and `TextInferenceEngine` accepts it
(`isinstance(text_model, BertForMaskedLM)`, `text/inference_engine.py:27`).  The forward (and its hand-written
backward) runs in `incremental_multimodal_medical_learning_ii_amd.text_encoder`; the HuggingFace sub-modules only
own the parameters.
"""
from dataclasses import dataclass
from typing import Any, List, Optional, Tuple, Union

import torch
from torch import Tensor as T
from torch import nn
from transformers import BertForMaskedLM
from transformers.modeling_outputs import ModelOutput

from .configuration_cxrbert import CXRBertConfig
from .... import kernels as K
from .... import text_encoder as TE

BERTTupleOutput = Tuple[T, T, T, T, T]


@dataclass
class CXRBertOutput(ModelOutput):
    last_hidden_state: torch.FloatTensor = None
    logits: Optional[torch.FloatTensor] = None
    cls_projected_embedding: Optional[torch.FloatTensor] = None
    hidden_states: Optional[Tuple[torch.FloatTensor]] = None
    attentions: Optional[Tuple[torch.FloatTensor]] = None


class BertProjectionHead(nn.Module):
    """Projection head for the BERT CLS token: Linear -> GELU -> LayerNorm(eps 1e-12) -> Linear
    (reference `modelling_cxrbert.py:28-49`).  Parameter container; executed by `text_encoder`."""

    def __init__(self, config: CXRBertConfig) -> None:
        super().__init__()
        self.dense_to_hidden = nn.Linear(config.hidden_size, config.projection_size)
        self.transform_act_fn = nn.functional.gelu
        self.LayerNorm = nn.LayerNorm(config.projection_size, eps=1e-12)
        self.dense_to_output = nn.Linear(config.projection_size, config.projection_size)

    def forward(self, hidden_states: torch.Tensor) -> torch.Tensor:
        h1_pre = torch.empty(hidden_states.shape[0], self.dense_to_hidden.out_features, dtype=torch.float32,
                             device=hidden_states.device)
        with torch.no_grad():
            h1 = K.linear_fwd(hidden_states, self.dense_to_hidden.weight, self.dense_to_hidden.bias, act=K.ACT_GELU,
                              preact_out=h1_pre)
            h2, _, _ = K.residual_ln_fwd(h1, None, self.LayerNorm.weight, self.LayerNorm.bias, 1e-12, save=False)
            return K.linear_fwd(h2, self.dense_to_output.weight, self.dense_to_output.bias)


class CXRBertModel(BertForMaskedLM):
    """CXR-BERT (Boecking et al. 2022) = HuggingFace BertForMaskedLM + a CLS projection head
    (reference `modelling_cxrbert.py:52-141`)."""

    config_class = CXRBertConfig  # type: ignore

    def __init__(self, config: CXRBertConfig):
        super().__init__(config)
        self.cls_projection_head = BertProjectionHead(config)
        if hasattr(self, "post_init"):
            self.post_init()
        else:  # transformers 4.17 spelling used by the reference (:68)
            self.init_weights()
        self._hot: Optional[List[nn.Parameter]] = None
        # optional callable(tag): handed to every grad-enabled encode call made while it is set and called by THAT call's backward
        # when its parameter gradients are complete (text_encoder.encode); set and cleared by the data-parallel trainer per step
        self.grad_ready_hook = None
        # train-mode dropout: None until `enable_dropout_`; then [seed, call counter]
        self._dropout: Optional[List[int]] = None
        # bumped whenever the stream is (re)seeded or assigned, so a data-parallel trainer knows when to re-broadcast rank 0's state
        self._dropout_version = 0
        # global sequence index of this process's first row (data parallel: rank * local rows; set by the joint trainer)
        self.dropout_row_offset = 0
        # True: the encode call keeps nothing for a backward (no graph, no hook), still draws this call's dropout masks and leaves
        # the call counter where it is.  Pass 1 of the joint trainer's micro-batched step sets and clears it.
        self.save_free = False

    # ------------------------------------------------------------------ dropout
    def enable_dropout_(self, seed: Optional[int] = None) -> "CXRBertModel":
        """Opt in to HF dropout in train mode (p = config.hidden_dropout_prob / attention_probs_dropout_prob at BertModel's four
        sites).  Masks are counter-based (include/cxrk.h, "dropout"): keyed by (seed, call counter, layer, site, global sequence
        index, token, column).  seed=None draws one 64-bit seed from torch's default CPU generator (`torch.manual_seed` makes it
        repeatable).  Each train-mode forward uses the current (seed, counter) and then advances the counter; the kernels key the
        masks by the low 24 bits of the counter, so the mask stream of one seed repeats after 2^24 train-mode calls (re-seed before).
        Data parallel: `contrastive.JointContrastiveTrainer` gives every rank rank 0's (seed, counter) -- at construction, and again
        at the next step whenever this method or the `dropout_state` setter has been called since -- so the ranks may seed
        differently."""
        if seed is None:
            w = torch.randint(0, 2 ** 32, (2,), dtype=torch.int64)
            seed = (int(w[0]) << 32) | int(w[1])
        self._dropout = [int(seed) & (2 ** 64 - 1), 0]
        self._dropout_version += 1
        return self

    @property
    def dropout_enabled(self) -> bool:
        return self._dropout is not None

    @property
    def dropout_state(self) -> Optional[Tuple[int, int]]:
        """(seed, call counter) of the next train-mode forward; None before `enable_dropout_`.  Assign a pair to resume a stream
        (only on a model that opted in with `enable_dropout_`).  Counters that differ by a multiple of 2^24 give the same masks."""
        return None if self._dropout is None else (self._dropout[0], self._dropout[1])

    @dropout_state.setter
    def dropout_state(self, state: Tuple[int, int]) -> None:
        if self._dropout is None:
            raise RuntimeError("dropout_state: this model has not opted in to dropout; call enable_dropout_(seed) first")
        seed, counter = state
        if int(counter) < 0:
            raise ValueError("dropout_state: the call counter must be >= 0")
        self._dropout = [int(seed) & (2 ** 64 - 1), int(counter)]
        self._dropout_version += 1

    def _dropout_probs(self) -> Tuple[float, float]:
        cfg = self.config
        return float(getattr(cfg, "hidden_dropout_prob", 0.0) or 0.0), float(getattr(cfg, "attention_probs_dropout_prob", 0.0) or 0.0)

    def _next_dropout(self) -> Optional[TE.Dropout]:
        """the dropout descriptor of this call (advancing the counter), or None when the call has eval semantics"""
        ph, pa = self._dropout_probs()
        if not self.training or self._dropout is None or (ph <= 0 and pa <= 0):
            return None
        seed, counter = self._dropout
        if not self.save_free:
            self._dropout[1] = counter + 1
        return TE.Dropout(seed, counter, self.dropout_row_offset, ph, pa)

    # ------------------------------------------------------------------ parameter plumbing
    def _hot_params(self) -> List[nn.Parameter]:
        if self._hot is None:
            named = dict(self.named_parameters())
            self._hot = [named[n] for n in TE.param_names(self.config.num_hidden_layers)]
        return self._hot

    def prepare_(self) -> "CXRBertModel":
        """Fuse every layer's query/key/value parameters into one [3H,H] buffer (idempotent; values unchanged).
        Needed again after `.to(device)` because that re-allocates parameter storage."""
        for layer in self.bert.encoder.layer:
            att = layer.attention.self
            TE.fuse_qkv_(att.query.weight, att.key.weight, att.value.weight)
            TE.fuse_qkv_(att.query.bias, att.key.bias, att.value.bias)
        return self

    def _check_mode(self) -> None:
        """Dropout is opt-in (`enable_dropout_`); the reference only ever runs the text model in eval mode
        (text/inference_engine.py:63 asserts it).  Refuse rather than silently skip the dropout of a training-mode model that did
        not opt in."""
        ph, pa = self._dropout_probs()
        if self.training and (ph > 0 or pa > 0) and self._dropout is None:
            raise NotImplementedError("CXRBertModel is in training mode with dropout > 0 but dropout was not enabled; call "
                                      ".enable_dropout_(seed) for HF train-mode dropout, .eval() (parameters still receive gradients), "
                                      "or set the dropout probabilities to 0")

    def _encode(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor], cls_only: bool = False, want_last: bool = True):
        if not input_ids.is_cuda:
            raise RuntimeError("CXRBertModel runs on the MI355X only: move the model and inputs to 'cuda' "
                               "(there is no CPU fallback; the CPU oracle lives in oracle/ and is test-only)")
        self.prepare_()
        cfg = self.config
        self._check_mode()
        if getattr(cfg, "hidden_act", "gelu") != "gelu":
            raise NotImplementedError(f"hidden_act={cfg.hidden_act!r}: only erf-GELU (CXR-BERT) is implemented")
        return TE.encode(self._hot_params(), input_ids, attention_mask, cfg.num_hidden_layers,
                         cfg.num_attention_heads, cfg.layer_norm_eps, cls_only, want_last,
                         on_grads_ready=self.grad_ready_hook if torch.is_grad_enabled() else None, dropout=self._next_dropout(),
                         save_free=bool(self.save_free))

    @torch.no_grad()
    def _mlm_logits(self, last_hidden: torch.Tensor) -> torch.Tensor:
        """HF `BertOnlyMLMHead`: transform (dense, gelu, LayerNorm) + decoder tied to the word embeddings."""
        tr = self.cls.predictions.transform
        N, L, H = last_hidden.shape
        h = K.linear_fwd(last_hidden.reshape(N * L, H), tr.dense.weight, tr.dense.bias, act=K.ACT_GELU)
        h, _, _ = K.residual_ln_fwd(h, None, tr.LayerNorm.weight, tr.LayerNorm.bias, self.config.layer_norm_eps,
                                    save=False)
        dec = self.cls.predictions.decoder
        bias = self.cls.predictions.bias if getattr(dec, "bias", None) is None else dec.bias
        return K.linear_fwd(h, dec.weight, bias).view(N, L, -1)

    def mlm_head_params(self) -> Tuple[nn.Parameter, ...]:
        """the six parameters of HF `BertOnlyMLMHead` in the order `functional.mlm_loss` takes them: transform dense weight / bias,
        transform LayerNorm weight / bias, decoder weight (the word embeddings when tied) and the decoder bias"""
        tr = self.cls.predictions.transform
        dec = self.cls.predictions.decoder
        bias = self.cls.predictions.bias if getattr(dec, "bias", None) is None else dec.bias
        return (tr.dense.weight, tr.dense.bias, tr.LayerNorm.weight, tr.LayerNorm.bias, dec.weight, bias)

    def get_projected_text_embeddings_and_hidden(self, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                                                 want_hidden: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """(unnormalised projected CLS embeddings [batch, projection_size], last hidden state [batch, L, hidden]) of ONE encoder pass
        on the full-sequence path, both differentiable: what the joint step's masked-language-modelling loss reads
        (`functional.mlm_loss`).  `want_hidden=False` runs the same path (the same bits of the embeddings) and returns None for the
        hidden state."""
        proj, last = self._encode(input_ids, attention_mask, cls_only=False, want_last=want_hidden)
        return proj, (last if want_hidden else None)

    # ------------------------------------------------------------------ reference API
    def forward(
        self,
        input_ids: torch.Tensor,
        attention_mask: torch.Tensor,
        token_type_ids: Optional[torch.Tensor] = None,
        position_ids: Optional[torch.Tensor] = None,
        head_mask: Optional[torch.Tensor] = None,
        inputs_embeds: Optional[torch.Tensor] = None,
        output_attentions: Optional[bool] = None,
        output_hidden_states: Optional[bool] = None,
        output_cls_projected_embedding: Optional[bool] = None,
        return_dict: Optional[bool] = None,
        output_mlm_logits: bool = True,
        **kwargs: Any
    ) -> Union[BERTTupleOutput, CXRBertOutput]:
        for name, val in (("token_type_ids", token_type_ids), ("position_ids", position_ids), ("head_mask", head_mask),
                          ("inputs_embeds", inputs_embeds)):
            if val is not None:
                raise NotImplementedError(f"{name} is not supported by the HIP path (the reference never passes it: "
                                          f"text/inference_engine.py:65-68)")
        if output_attentions:
            raise NotImplementedError("output_attentions is not supported by the HIP path")
        return_dict = return_dict if return_dict is not None else getattr(self.config, "use_return_dict", True)
        proj, last_hidden_state = self._encode(input_ids, attention_mask)
        cls_projected_embedding = proj if output_cls_projected_embedding else None
        logits = self._mlm_logits(last_hidden_state.detach()) if output_mlm_logits else None
        hidden_states = (last_hidden_state,) if output_hidden_states else None  # only the last layer is materialised
        if return_dict:
            return CXRBertOutput(last_hidden_state=last_hidden_state, logits=logits,
                                 cls_projected_embedding=cls_projected_embedding, hidden_states=hidden_states,
                                 attentions=None)
        return (last_hidden_state, logits, cls_projected_embedding, hidden_states, None)

    def get_projected_text_embeddings(self, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                                      normalize_embeddings: bool = True) -> torch.Tensor:
        """Projected CLS embeddings [batch, projection_size], optionally L2-normalised
        (reference `modelling_cxrbert.py:117-141`)."""
        # Only hidden_states[-1][:, 0, :] feeds the projection head (:98-99): the last layer's row-wise part runs on the CLS
        # rows alone (text_encoder._forward, cls_only).  Same values as forward(...).cls_projected_embedding.
        cls_projected_embedding, _ = self._encode(input_ids, attention_mask, cls_only=True, want_last=False)
        if normalize_embeddings:
            from ....functional import l2_normalize
            return l2_normalize(cls_projected_embedding)
        return cls_projected_embedding
