"""Qwen3-MoE without a GPU: the workspace query, host-side argument validation of the nvl_moe_* entry points, and what
`Config` accepts and refuses for a `qwen3_moe` directory."""
import json
import os

import pytest


def test_workspace_bytes_is_monotone_and_covers_the_row_block_bound():
    from nano_vllm_amd import ops
    prev = 0
    for tokens in (1, 2, 15, 16, 17, 128, 129, 1000, 2048):
        n = ops.moe_workspace_bytes(tokens, 2048, 768, 128, 8)
        pairs = tokens * 8
        blocks = pairs // 128 + min(128, pairs)
        # offsets, sorted pairs + positions, 16-byte row-block records, h (bf16) and y (fp32) of every pair
        assert n >= (128 + 1) * 4 + 2 * pairs * 4 + blocks * 16 + pairs * 768 * 2 + pairs * 2048 * 4
        assert n > prev
        prev = n
    assert ops.lib().nvl_moe_workspace_bytes(16, 2048, 700, 128, 8) == 0          # outside the kernels' shapes


def test_host_side_argument_validation_without_gpu():
    from nano_vllm_amd import ops
    lib = ops.load_library()
    big = 1 << 40
    assert lib.nvl_moe_route(None, 256, 256, 256, 4, 256, 8, 2, 1, None) == -1 and b"null pointer" in lib.nvl_last_error()
    assert lib.nvl_moe_route(256, 256, 256, 256, 4, 256, 8, 9, 1, None) == -1 and b"top_k <= E" in lib.nvl_last_error()
    assert lib.nvl_moe_route(256, 256, 256, 256, 4, 200, 8, 2, 1, None) == -1 and b"multiple of 128" in lib.nvl_last_error()
    assert lib.nvl_moe_plan(256, 4, 8, 2, None, big, None) == -1 and b"null pointer" in lib.nvl_last_error()
    assert lib.nvl_moe_plan(256, 4, 4, 5, 256, big, None) == -1 and b"top_k <= E" in lib.nvl_last_error()
    cap = ops.moe_workspace_bytes(4, 256, 128, 8, 2)
    assert lib.nvl_moe_plan(256, 1 << 16, 8, 2, 256, cap, None) == -1 and b"above the cap" in lib.nvl_last_error()
    good = dict(x=256, gu=256, dn=256, ids=256, w=256, out=256, m=4, hidden=256, inter=128, E=8, k=2, layout=0, ws=256,
                nbytes=cap, stream=None)                               # (nvl_moe_experts' arguments, in order)

    def experts(**kw):
        return lib.nvl_moe_experts(*{**good, **kw}.values())
    for kw, msg in ((dict(out=None), b"null pointer"), (dict(k=9), b"top_k <= E"), (dict(hidden=192), b"hidden=192"),
                    (dict(inter=64), b"inter=64"), (dict(m=5), b"above the cap"), (dict(layout=2), b"weight_layout")):
        assert experts(**kw) == -1 and msg in lib.nvl_last_error(), kw


@pytest.fixture
def moe_dir(tmp_path):
    from nano_vllm_amd.weights import qwen3_config_dict

    def make(**override):
        cfg = {**qwen3_config_dict("qwen3-moe-tiny", vocab_size=512), **override}
        d = tmp_path / f"moe{len(os.listdir(tmp_path))}"
        d.mkdir()
        (d / "config.json").write_text(json.dumps(cfg))
        return str(d)
    return make


def test_config_builds_on_a_qwen3_moe_directory_and_geometry_carries_the_experts(moe_dir):
    from nano_vllm_amd.api import Config, model_geometry
    from nano_vllm_amd.weights import parameter_shapes, qwen3_config_dict
    geo = model_geometry(Config(moe_dir()).hf_config)
    assert (geo["num_experts"], geo["top_k"], geo["moe_inter"], geo["norm_topk_prob"]) == (8, 2, 128, True)
    big = qwen3_config_dict("qwen3-30b-a3b")
    assert (big["num_experts"], big["num_experts_per_tok"], big["moe_intermediate_size"], big["hidden_size"]) == (128, 8, 768, 2048)
    shapes = parameter_shapes(qwen3_config_dict("qwen3-moe-tiny", vocab_size=512))
    assert shapes["model.layers.1.mlp.experts.7.down_proj.weight"] == (256, 128)
    assert shapes["model.layers.0.mlp.gate.weight"] == (8, 256) and "model.layers.0.mlp.gate_proj.weight" not in shapes


@pytest.mark.parametrize("kw,override,msg", [
    (dict(tensor_parallel_size=2), {}, "tensor_parallel_size"),
    (dict(weight_dtype="fp8"), {}, "expert weights stay bf16"),
    ({}, dict(decoder_sparse_step=2), "decoder_sparse_step"),
    ({}, dict(mlp_only_layers=[0]), "mlp_only_layers"),
    ({}, dict(shared_expert_intermediate_size=512), "shared expert"),
])
def test_out_of_scope_moe_configurations_are_refused_at_load(moe_dir, kw, override, msg):
    from nano_vllm_amd.api import Config
    with pytest.raises(ValueError, match=msg):
        Config(moe_dir(**override), **kw)
