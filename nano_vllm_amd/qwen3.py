"""Qwen3 decoder built on the libnvl kernels — the only model family the reference ships
(nano-vllm models/qwen3.py:14-216). Same module tree and parameter names as the reference /
HF checkpoints (so `packed_modules_mapping`-style loading works), but the per-layer dataflow
is arranged for MI355X:

   add+RMSNorm -> qkv GEMM -> [q/k-norm + RoPE + KV-cache store: ONE launch]
               -> paged decode attention | MFMA prefill attention -> o GEMM (+all-reduce)
   add+RMSNorm -> gate_up GEMM -> SiLU*mul -> down GEMM (+all-reduce)

i.e. 10 launches per layer instead of the reference's 13 (each dependent kernel boundary is
~1.5 us on this chip even inside a hipGraph — MI355X_MICROARCH.md "boundary"; a small dependent
kernel costs ~5 us whatever it does). On decode-sized batches (<= 256 rows, TP=1, single-K-pass
shapes) the chain is 8 launches:

   add+RMSNorm(fp32 slabs) -> qkv GEMM -> [q/k-norm + RoPE + KV store + paged attention: ONE launch]
   -> split merge -> o GEMM (fp32 split-K slabs) -> add+RMSNorm(slabs) -> gate_up GEMM + SiLU*mul epilogue
   -> down GEMM (slabs)

with the GEMMs on the hand-written skinny kernel (nvl_linear_decode).
"""
from __future__ import annotations

import os

import torch
from torch import nn

from .api import model_geometry
from .attn_meta import get_context
from .layers import (Attention, MergedColumnParallelLinear, ParallelLMHead, QKVParallelLinear, RMSNorm,
                     RowParallelLinear, SiluAndMul, VocabParallelEmbedding, get_rope)
from . import ops, tp


class Qwen3Attention(nn.Module):

    def __init__(self, geo: dict, total_heads: int, total_kv_heads: int, qkv_bias: bool):
        super().__init__()
        self.num_heads, self.num_kv_heads, self.head_dim = geo["heads"], geo["kv_heads"], geo["head_dim"]
        self.q_size = self.num_heads * self.head_dim
        self.kv_size = self.num_kv_heads * self.head_dim
        self.eps = geo["eps"]
        self.qkv_proj = QKVParallelLinear(geo["hidden"], self.head_dim, total_heads, total_kv_heads, bias=qkv_bias)
        self.o_proj = RowParallelLinear(total_heads * self.head_dim, geo["hidden"], bias=False)
        self.rotary_emb = get_rope(self.head_dim, self.head_dim, geo["max_pos"], geo["rope_theta"])
        self.attn = Attention(self.num_heads, self.head_dim, self.head_dim ** -0.5, self.num_kv_heads)
        self.has_qk_norm = not qkv_bias                      # models/qwen3.py:68-70
        if self.has_qk_norm:
            self.q_norm = RMSNorm(self.head_dim, eps=self.eps)
            self.k_norm = RMSNorm(self.head_dim, eps=self.eps)

    def forward(self, positions: torch.Tensor, hidden_states: torch.Tensor) -> torch.Tensor:
        ctx = get_context()
        # (a step whose plan carries a shared prefix takes bf16 qkv: the attention kernel that also serves the shared-prefix packs
        #  in the SAME launch has no scalar registers left for the slab-sum prologue — attn_decode.hip — and with slabs the pass
        #  would be a launch of its own on a divided grid)
        if self.attn.fuses_decode_step(ctx) and not ctx.shared_prefix:
            qkv = self.qkv_proj.forward_for_fused_decode(hidden_states)      # bf16 [N, out], or fp32 split-K slabs
        else:
            qkv = self.qkv_proj(hidden_states)
        qw = self.q_norm.weight if self.has_qk_norm else None
        kw = self.k_norm.weight if self.has_qk_norm else None
        o = self.attn.forward_fused(qkv, positions, qw, kw, self.eps, self.rotary_emb.cos_sin_cache)
        return self.o_proj.forward_decode(o.view(o.shape[0], -1))


class Qwen3MLP(nn.Module):

    def __init__(self, hidden_size: int, intermediate_size: int, hidden_act: str):
        super().__init__()
        assert hidden_act == "silu"
        self.gate_up_proj = MergedColumnParallelLinear(hidden_size, [intermediate_size] * 2, bias=False)
        self.down_proj = RowParallelLinear(intermediate_size, hidden_size, bias=False)
        self.act_fn = SiluAndMul()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.down_proj.forward_decode(self.gate_up_proj.forward_silu(x))


class Qwen3MoeSparseBlock(nn.Module):
    """The feed-forward block of the `qwen3_moe` models (Qwen3-30B-A3B, -235B-A22B): a router picks `top_k` of
    `num_experts` SwiGLU experts per token. Three parameters — `gate` [E, hidden] (checkpoint `mlp.gate.weight`),
    `experts_gate_up` [E, 2 * inter, hidden] and `experts_down` [E, hidden, inter] (the checkpoint's
    `mlp.experts.{e}.{gate,up,down}_proj.weight`, stacked) — and three kernel calls: ops.moe_route -> moe_plan ->
    moe_experts. bf16 rows in, bf16 rows out; the workspace is handed in by the runner (`set_workspace`) and shared by
    all layers; more rows than it holds are served in consecutive chunks. After pack_for_decode(weight_dtype="mxfp4") the
    expert matrices exist as MXFP4 codes + scales only and the last call is ops.moe_experts_mxfp4."""

    def __init__(self, hidden_size: int, moe_intermediate_size: int, num_experts: int, top_k: int, norm_topk_prob: bool):
        super().__init__()
        self.num_experts, self.top_k, self.norm_topk_prob = num_experts, top_k, bool(norm_topk_prob)
        self.hidden, self.inter = hidden_size, moe_intermediate_size
        self.gate = nn.Parameter(torch.empty(num_experts, hidden_size), requires_grad=False)
        self.experts_gate_up = nn.Parameter(torch.empty(num_experts, 2 * moe_intermediate_size, hidden_size),
                                            requires_grad=False)
        self.experts_down = nn.Parameter(torch.empty(num_experts, hidden_size, moe_intermediate_size), requires_grad=False)
        self.experts_gate_up.weight_loader = self._load_gate_up
        self.experts_down.weight_loader = self._load_down
        self.gate_up_packed: torch.Tensor | None = None      # tile-packed copies (pack_for_decode): both or neither
        self.down_packed: torch.Tensor | None = None
        # (gate|up codes, scales, down codes, scales) once pack_for_decode(weight_dtype="mxfp4") has run
        self.mxfp4: tuple[torch.Tensor, ...] | None = None
        self.workspace: torch.Tensor | None = None
        self.max_tokens = 0

    def _load_gate_up(self, param: nn.Parameter, loaded: torch.Tensor, shard) -> None:
        expert, half = shard                                  # half 0: gate_proj rows, 1: up_proj rows
        param.data[expert, half * self.inter:(half + 1) * self.inter].copy_(loaded)

    def _load_down(self, param: nn.Parameter, loaded: torch.Tensor, shard) -> None:
        param.data[shard[0]].copy_(loaded)

    def workspace_bytes(self, max_tokens: int) -> int:
        return ops.moe_workspace_bytes(max_tokens, self.hidden, self.inter, self.num_experts, self.top_k)

    def set_workspace(self, workspace: torch.Tensor, max_tokens: int) -> None:
        assert workspace.dtype == torch.uint8 and workspace.numel() >= self.workspace_bytes(max_tokens)
        self.workspace, self.max_tokens = workspace, max_tokens

    def pack_for_decode(self, budget_bytes: float = float("inf"), weight_dtype: str = "bf16") -> int:
        """Tile-packed copies of the stacked expert matrices (ops.pack_weight_tiles over [E * n, k]); returns the extra
        bytes, or -1 when they do not fit `budget_bytes` (the kernels then stream the row-major parameters).
        weight_dtype="mxfp4": the stacked matrices are quantised to MXFP4 (ops.quant_pack_mxfp4: 4-bit codes + one scale
        byte per 32 k) and the bf16 parameters' storage is RELEASED — prefill and decode both run nvl_moe_experts_mxfp4,
        nothing needs the bf16 matrix again. The call frees more than it takes, so the budget does not apply; returns
        the bytes of codes and scales."""
        if weight_dtype == "mxfp4":
            if self.mxfp4 is None:
                packed = []
                for p in (self.experts_gate_up, self.experts_down):
                    packed += ops.quant_pack_mxfp4(p.data.view(-1, p.shape[-1]))
                    p.data = torch.empty(0, dtype=p.dtype, device=p.device)
                self.mxfp4 = tuple(packed)
            return sum(t.numel() for t in self.mxfp4)
        if os.environ.get("NVL_PACKED_WEIGHTS", "1") == "0":   # (A/B measurements, as LinearBase.pack_for_decode)
            return 0
        need = (self.experts_gate_up.numel() + self.experts_down.numel()) * 2
        if need > budget_bytes:
            return -1
        gu, dn = self.experts_gate_up.data, self.experts_down.data
        self.gate_up_packed = ops.pack_weight_tiles(gu.view(-1, gu.shape[-1])).view(gu.shape)
        self.down_packed = ops.pack_weight_tiles(dn.view(-1, dn.shape[-1])).view(dn.shape)
        return need

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.workspace is None:
            raise ops.NvlError("Qwen3MoeSparseBlock has no workspace (set_workspace): the engine allocates it at load")
        packed = self.gate_up_packed is not None
        gu = self.gate_up_packed if packed else self.experts_gate_up
        dn = self.down_packed if packed else self.experts_down
        out = torch.empty_like(x)
        for r0 in range(0, x.shape[0], self.max_tokens):
            xs = x[r0:r0 + self.max_tokens]
            ids, wts = ops.moe_route(xs, self.gate, self.top_k, self.norm_topk_prob)
            ops.moe_plan(ids, self.num_experts, self.workspace)
            if self.mxfp4 is not None:
                ops.moe_experts_mxfp4(xs, *self.mxfp4, ids, wts, self.workspace, out=out[r0:r0 + self.max_tokens])
            else:
                ops.moe_experts(xs, gu, dn, ids, wts, self.workspace, out=out[r0:r0 + self.max_tokens], packed=packed)
        return out


class Qwen3DecoderLayer(nn.Module):

    def __init__(self, config, geo: dict):
        super().__init__()
        self.self_attn = Qwen3Attention(geo, config.num_attention_heads, config.num_key_value_heads,
                                        qkv_bias=getattr(config, "attention_bias", True))     # default as models/qwen3.py:133
        if geo.get("num_experts"):
            self.mlp = Qwen3MoeSparseBlock(config.hidden_size, geo["moe_inter"], geo["num_experts"], geo["top_k"],
                                           geo["norm_topk_prob"])
        else:
            self.mlp = Qwen3MLP(config.hidden_size, config.intermediate_size, config.hidden_act)
        self.input_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, positions, hidden_states, residual):
        if residual is None:                                 # first layer: residual = embeddings
            residual = hidden_states
            hidden_states = self.input_layernorm(hidden_states)
        else:
            hidden_states, residual = self.input_layernorm(hidden_states, residual)
        hidden_states = self.self_attn(positions, hidden_states)
        hidden_states, residual = self.post_attention_layernorm(hidden_states, residual)
        return self.mlp(hidden_states), residual


class Qwen3Model(nn.Module):

    def __init__(self, config, geo: dict):
        super().__init__()
        self.embed_tokens = VocabParallelEmbedding(config.vocab_size, config.hidden_size)
        self.layers = nn.ModuleList([Qwen3DecoderLayer(config, geo) for _ in range(config.num_hidden_layers)])
        self.norm = RMSNorm(config.hidden_size, eps=config.rms_norm_eps)

    def forward(self, input_ids: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        hidden_states = self.embed_tokens(input_ids)
        residual = None
        for layer in self.layers:
            hidden_states, residual = layer(positions, hidden_states, residual)
        hidden_states, _ = self.norm(hidden_states, residual)
        return hidden_states


class Qwen3ForCausalLM(nn.Module):
    # checkpoint-name fragment -> (fused parameter fragment, shard id)   (models/qwen3.py:187-193)
    packed_modules_mapping = {
        "q_proj": ("qkv_proj", "q"),
        "k_proj": ("qkv_proj", "k"),
        "v_proj": ("qkv_proj", "v"),
        "gate_proj": ("gate_up_proj", 0),
        "up_proj": ("gate_up_proj", 1),
    }

    def __init__(self, config):
        super().__init__()
        _, size = tp.world()
        self.geo = model_geometry(config, size)
        self.model = Qwen3Model(config, self.geo)
        self.lm_head = ParallelLMHead(config.vocab_size, config.hidden_size)
        if self.geo["tie"]:
            self.lm_head.weight.data = self.model.embed_tokens.weight.data

    def forward(self, input_ids: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
        return self.model(input_ids, positions)

    def compute_logits(self, hidden_states: torch.Tensor) -> torch.Tensor:
        return self.lm_head(hidden_states)

    def compute_logits_shard(self, hidden_states: torch.Tensor) -> torch.Tensor:
        """This rank's vocabulary slice of the logits (TP > 1: sampled shard-wise, never gathered)."""
        return self.lm_head.forward_shard(hidden_states)


class Qwen3MoeForCausalLM(Qwen3ForCausalLM):
    """`model_type: "qwen3_moe"`: the same decoder with Qwen3MoeSparseBlock as every layer's feed-forward block (the
    geometry carries num_experts / top_k / moe_inter, Qwen3DecoderLayer picks the block from it)."""

    def __init__(self, config):
        super().__init__(config)
        assert self.geo["num_experts"], "Qwen3MoeForCausalLM needs a qwen3_moe config (num_experts)"

    def allocate_moe_workspace(self, max_tokens: int) -> int:
        """ONE workspace for the MoE blocks of every layer (they run one after the other), sized for `max_tokens` rows
        per call; longer batches are chunked by the block. Returns its bytes."""
        blocks = [m for m in self.modules() if isinstance(m, Qwen3MoeSparseBlock)]
        nbytes = blocks[0].workspace_bytes(max_tokens)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=blocks[0].gate.device)
        for b in blocks:
            b.set_workspace(ws, max_tokens)
        return nbytes
