"""Public configuration surface of the drop-in: `Config` and `SamplingParams`.

Mirrors the reference's field names, defaults and assertions (nano-vllm config.py:7-25,
sampling_params.py:5-11) so callers of `nanovllm.LLM(model, **kwargs)` switch over unchanged.
Extensions (all optional, behaviour-neutral when unset):
  * SamplingParams.temperature == 0 selects greedy decoding (the reference forbids it; the
    parity harness needs it — SURVEY.md §0-7).
  * SamplingParams.top_k / top_p truncate the distribution before the draw (top-k first, then top-p renormalised over
    the survivors, ties at a cut kept); 0 / -1 and 1.0 switch them off. Single GPU only: tensor_parallel_size > 1
    refuses such a request.
  * SamplingParams.presence_penalty / frequency_penalty / repetition_penalty change a row's raw logits before temperature
    and top-k / top-p, with the usual semantics: l / r or l * r (by sign) for every token of the prompt or the output,
    then - frequency x (count in the output) - presence x (count > 0). 0 / 0 / 1 switch them off. The token history is
    read on the device (nvl_apply_penalties). Single GPU only, and max_model_len <= 16,383: other requests are refused.
  * Config.seed seeds the counter-based sampler RNG.
  * Config.dummy_weights = True initialises random weights on device instead of reading
    *.safetensors (no 8B/32B checkpoints exist offline).
  * Config.kv_cache_dtype = "fp8" stores K/V as OCP fp8 e4m3: the decode step is bound by
    K/V bytes, this halves them. It changes numerics, so every parity run keeps the default "bf16".
  * Config.weight_dtype = "fp8" quantises the decode projections (q|k|v, o, gate|up, down) at load time to OCP e4m3
    with a power-of-two scale per 128 x 128 block and streams them through nvl_linear_wide_fp8 (half the weight bytes
    per decode step, a half-size packed copy). The bf16 parameter is overwritten with the dequantised values, so
    prefill and decode compute with the same matrix. Outside the reference's numerics: opt-in, default "bf16".
  * Config.weight_dtype = "fp8_only" (dense models, one GPU) quantises exactly as "fp8" and then FREES the bf16
    projections: rows above 256 (prefill, decode batches of 257-512 sequences) run nvl_linear_tile_fp8 on the same packed
    e4m3 tiles instead of the library GEMM on a bf16 copy, so the projections occupy half of bf16's bytes and the KV pool
    gets the rest. Same matrix as "fp8", another summation order in prefill. Refused for qwen3_moe and for
    tensor_parallel_size > 1.
  * Config.weight_dtype = "mxfp4" (qwen3_moe models only) quantises the expert matrices at load time to OCP MXFP4 —
    e2m1 elements, one power-of-two scale byte per row and 32 k — and frees their bf16 storage: prefill and decode
    both run nvl_moe_experts_mxfp4 (about 3.76 x fewer expert bytes, resident and streamed). Attention, router,
    embedding and lm_head stay bf16. A dense model is refused; "fp8" stays refused for qwen3_moe.
  * Config.weight_dtype = "mxfp4_dense" (dense models, one GPU) quantises the decode projections at load time to the
    same MXFP4 format and streams them through nvl_linear_wide_mxfp4 at up to 256 rows (17/32 byte per weight: a quarter
    of bf16's bytes per decode step, half of "fp8"'s; the codes replace the bf16 tile-packed copy). As with "fp8" the
    bf16 parameter is overwritten with the dequantised values, so prefill (library GEMM) and decode compute with the
    same matrix. 4-bit weights are far outside the reference's numerics: opt-in. Refused for qwen3_moe and for
    tensor_parallel_size > 1.
  * Config.weight_dtype = "mxfp4_dense_only" (dense models, one GPU) quantises exactly as "mxfp4_dense" and then FREES the
    bf16 projections: rows above 256 (prefill, decode batches of 257-512 sequences) run nvl_linear_tile_mxfp4 on the same
    codes and scales instead of the library GEMM on a dequantised bf16 copy, so the projections occupy 17/32 byte per
    weight and the KV pool gets the rest. Same matrix as "mxfp4_dense", another summation order in prefill. Refused for
    qwen3_moe and for tensor_parallel_size > 1.
"""
from __future__ import annotations

import os
from dataclasses import dataclass


PENALTY_MAX_CONTEXT = 16383       # nvl_apply_penalties: a 14-bit count per token, 16 positions per lane (include/nvl.h)


@dataclass(slots=True)
class SamplingParams:
    temperature: float = 1.0
    max_tokens: int = 64
    ignore_eos: bool = False
    top_k: int = 0                # 0 or -1: off
    top_p: float = 1.0            # 1.0: off
    presence_penalty: float = 0.0     # 0.0: off
    frequency_penalty: float = 0.0    # 0.0: off
    repetition_penalty: float = 1.0   # 1.0: off

    @property
    def penalised(self) -> bool:
        return self.presence_penalty != 0 or self.frequency_penalty != 0 or self.repetition_penalty != 1

    def __post_init__(self):
        assert self.repetition_penalty > 0, "repetition_penalty must be > 0 (1.0: off)"
        assert self.temperature == 0 or self.temperature > 1e-10, "temperature must be 0 (greedy) or > 1e-10"
        assert self.max_tokens >= 1
        assert self.top_k >= -1, "top_k must be >= -1 (0 or -1: off)"
        assert 0 < self.top_p <= 1, "top_p must be in (0, 1]"


@dataclass(slots=True)
class Config:
    model: str
    max_num_batched_tokens: int = 16384
    max_num_seqs: int = 512
    max_model_len: int = 4096
    gpu_memory_utilization: float = 0.9
    tensor_parallel_size: int = 1
    enforce_eager: bool = False
    hf_config: object | None = None
    eos: int = -1
    kvcache_block_size: int = 256
    num_kvcache_blocks: int = -1
    # --- extensions -------------------------------------------------------------------------
    seed: int = 0
    dummy_weights: bool = False
    kv_cache_dtype: str = "bf16"         # "fp8": OCP e4m3 KV cache (halves decode bytes; outside the reference's numerics)
    weight_dtype: str = "bf16"           # "fp8": block-scaled e4m3 decode projections (halves weight bytes; same caveat)
    #                                      "fp8_only": the same, and the bf16 projections are freed (module docstring)
    #                                      "mxfp4": 4-bit expert matrices of a qwen3_moe model (module docstring)
    #                                      "mxfp4_dense": 4-bit decode projections of a dense model (module docstring)
    #                                      "mxfp4_dense_only": the same, and the bf16 projections are freed (module docstring)

    def __post_init__(self):
        assert os.path.isdir(self.model), f"model directory not found: {self.model}"
        assert self.kvcache_block_size % 256 == 0
        assert 1 <= self.tensor_parallel_size <= 8
        if self.hf_config is None:
            from transformers import AutoConfig
            self.hf_config = AutoConfig.from_pretrained(self.model)
        self.max_model_len = min(self.max_model_len, self.hf_config.max_position_embeddings)
        assert self.max_num_batched_tokens >= 1 and self.max_num_seqs >= 1
        assert self.kv_cache_dtype in ("bf16", "fp8"), "kv_cache_dtype must be 'bf16' or 'fp8'"
        assert self.weight_dtype in ("bf16", "fp8", "fp8_only", "mxfp4", "mxfp4_dense", "mxfp4_dense_only"), \
            "weight_dtype must be 'bf16', 'fp8', 'fp8_only', 'mxfp4', 'mxfp4_dense' or 'mxfp4_dense_only'"
        if self.weight_dtype == "fp8_only" and self.tensor_parallel_size > 1:
            raise ValueError("weight_dtype='fp8_only' is single-GPU (the tensor-parallel GEMMs read the bf16 parameter): use 'fp8'")
        if self.weight_dtype == "mxfp4" and getattr(self.hf_config, "model_type", "qwen3") != "qwen3_moe":
            raise ValueError("weight_dtype='mxfp4' covers the expert weights of a qwen3_moe model only "
                             "(dense models: 'mxfp4_dense' or 'fp8')")
        if self.weight_dtype == "mxfp4_dense" and self.tensor_parallel_size > 1:
            raise ValueError("weight_dtype='mxfp4_dense' is single-GPU for now: use 'fp8' with tensor_parallel_size > 1")
        if self.weight_dtype == "mxfp4_dense_only" and self.tensor_parallel_size > 1:
            raise ValueError("weight_dtype='mxfp4_dense_only' is single-GPU (the tensor-parallel GEMMs read the bf16 "
                             "parameter): use 'fp8' with tensor_parallel_size > 1")
        check_moe_scope(self.hf_config, self.tensor_parallel_size, self.weight_dtype)


def check_moe_scope(hf_config, tp: int = 1, weight_dtype: str = "bf16") -> None:
    """A `qwen3_moe` config is served on one GPU with bf16 or MXFP4 experts, every layer sparse, no shared expert;
    anything else is refused here, at load, rather than computed wrongly."""
    if getattr(hf_config, "model_type", "qwen3") != "qwen3_moe":
        return
    if tp != 1:
        raise ValueError("qwen3_moe: tensor_parallel_size > 1 is not supported (the expert kernels are single-GPU)")
    if weight_dtype not in ("bf16", "mxfp4"):
        raise ValueError(f"qwen3_moe: weight_dtype='{weight_dtype}' is not supported (expert weights stay bf16)")
    if getattr(hf_config, "decoder_sparse_step", 1) != 1 or list(getattr(hf_config, "mlp_only_layers", None) or []):
        raise ValueError("qwen3_moe: decoder_sparse_step != 1 / mlp_only_layers are not supported (every layer is sparse)")
    if (getattr(hf_config, "shared_expert_intermediate_size", 0) or getattr(hf_config, "n_shared_experts", 0)
            or getattr(hf_config, "num_shared_experts", 0)):
        raise ValueError("qwen3_moe: a shared expert is not supported")
    e, k = hf_config.num_experts, hf_config.num_experts_per_tok
    if not (1 <= k <= 8 and k <= e <= 256 and hf_config.hidden_size % 128 == 0 and hf_config.hidden_size <= 4096
            and hf_config.moe_intermediate_size % 128 == 0):
        raise ValueError(f"qwen3_moe: num_experts={e} (<= 256), num_experts_per_tok={k} (<= 8), hidden_size (<= 4096) and "
                         "moe_intermediate_size (multiples of 128) are outside the expert kernels' range")


def model_geometry(hf_config, tp: int = 1) -> dict:
    """Per-rank shapes of a Qwen3-family config (models/qwen3.py:29-39)."""
    moe = getattr(hf_config, "model_type", "qwen3") == "qwen3_moe"
    if moe:
        check_moe_scope(hf_config, tp)
    heads = hf_config.num_attention_heads
    kv_heads = hf_config.num_key_value_heads
    head_dim = getattr(hf_config, "head_dim", None) or hf_config.hidden_size // heads
    assert heads % tp == 0 and kv_heads % tp == 0 and hf_config.vocab_size % tp == 0
    assert hf_config.intermediate_size % tp == 0
    rope_theta = getattr(hf_config, "rope_theta", None)
    for attr in ("rope_scaling", "rope_parameters"):
        d = getattr(hf_config, attr, None)
        if isinstance(d, dict) and "rope_theta" in d:
            rope_theta = d["rope_theta"]
    if rope_theta is None:
        rope_theta = 1000000
    dtype = getattr(hf_config, "dtype", None) or getattr(hf_config, "torch_dtype", None)
    return dict(
        hidden=hf_config.hidden_size, layers=hf_config.num_hidden_layers, heads=heads // tp, kv_heads=kv_heads // tp,
        head_dim=head_dim, inter=hf_config.intermediate_size // tp, vocab=hf_config.vocab_size,
        vocab_per_rank=hf_config.vocab_size // tp, eps=hf_config.rms_norm_eps, rope_theta=float(rope_theta),
        max_pos=hf_config.max_position_embeddings, tie=bool(getattr(hf_config, "tie_word_embeddings", False)),
        qk_norm=not getattr(hf_config, "attention_bias", True), dtype=dtype,    # (default as models/qwen3.py:133)
        # qwen3_moe: experts per layer, experts per token, expert width, renormalised routing weights (0 / False: dense)
        num_experts=hf_config.num_experts if moe else 0, top_k=hf_config.num_experts_per_tok if moe else 0,
        moe_inter=hf_config.moe_intermediate_size if moe else 0,
        norm_topk_prob=bool(getattr(hf_config, "norm_topk_prob", False)) if moe else False)
