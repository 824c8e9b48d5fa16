"""Qwen3-MoE kernels on the MI355X (csrc/moe.hip): router, expert plan + grouped expert GEMMs, the model block and the
engine, each against a plain fp64 restatement (`_experts_ref`) or the dense oracle."""
import functools
import json
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _experts_ref(x, gu, dn, ids, wts, dt=torch.float64):
    """out[t] = sum_j wts[t, j] * down_e(silu(gate_e x[t]) * up_e x[t]), e = ids[t, j] (CPU tensors). dt = float64: the
    reference; dt = bfloat16: the same per-expert F.linear loop with g, u, h, y and out rounded to bf16."""
    out = torch.zeros(x.shape[0], x.shape[1], dtype=torch.float64)
    for e in ids.unique().tolist():
        t, j = (ids == e).nonzero(as_tuple=True)
        g, u = F.linear(x[t].to(dt), gu[e].to(dt)).chunk(2, -1)
        y = F.linear(F.silu(g) * u, dn[e].to(dt))
        out.index_put_((t,), wts[t, j, None].double() * y.double(), accumulate=True)
    return out if dt == torch.float64 else out.to(dt).double()


def _rel_err(got, ref):
    return ((got.double() - ref).abs().max() / ref.pow(2).mean().sqrt()).item()


@functools.lru_cache(None)
def _case(m, E, k, hidden, inter, skew=False):
    """Inputs of one experts case with its fp64 reference and the bf16 restatement's error (made once, shared)."""
    g = torch.Generator().manual_seed(1000 * m + E)
    x = torch.randn(m, hidden, generator=g).bfloat16()
    gu = (torch.randn(E, 2 * inter, hidden, generator=g) / hidden ** 0.5).bfloat16()
    dn = (torch.randn(E, hidden, inter, generator=g) / inter ** 0.5).bfloat16()
    ids = torch.rand(m, E, generator=g).argsort(-1)[:, :k].int().contiguous()
    if skew:
        ids.zero_()                                  # every pair on expert 0: one expert owns all rows, the rest are empty
    wts = torch.rand(m, k, generator=g) + 0.1
    wts = (wts / wts.sum(-1, keepdim=True)).float()
    ref = _experts_ref(x, gu, dn, ids, wts)
    return x, gu, dn, ids, wts, ref, _rel_err(_experts_ref(x, gu, dn, ids, wts, torch.bfloat16), ref)


def _run_experts(x, gu, dn, ids, wts, packed):
    from nano_vllm_amd import ops
    E, _, inter = dn.shape
    x, gu, dn, ids, wts = (t.cuda() for t in (x, gu, dn, ids, wts))
    if packed:
        gu = ops.pack_weight_tiles(gu.view(-1, gu.shape[-1])).view(gu.shape)
        dn = ops.pack_weight_tiles(dn.view(-1, dn.shape[-1])).view(dn.shape)
    ws = torch.empty(ops.moe_workspace_bytes(x.shape[0], x.shape[1], inter, E, ids.shape[1]), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        ops.moe_plan(ids, E, ws)
        outs.append(ops.moe_experts(x, gu, dn, ids, wts, ws, packed=packed).cpu())
    assert torch.equal(outs[0], outs[1]), "two calls on the same inputs differ"
    return outs[0]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("cfg", [(8, 2, 256, 128), (128, 8, 256, 384)])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 130, 300])
def test_experts_with_given_ids_vs_fp64(m, cfg, packed):
    x, gu, dn, ids, wts, ref, bf16_err = _case(m, *cfg)
    err = _rel_err(_run_experts(x, gu, dn, ids, wts, packed), ref)
    print(f"m={m} cfg={cfg} packed={packed}: max|d| / rms kernel {err:.5f}, bf16 restatement {bf16_err:.5f}")
    # bound: 2 x the bf16 restatement's own error on these inputs (same rounding points, another fp32 summation order);
    # the restatement measures 0.012 - 0.032 on these cases (it also rounds y to bf16, which the kernel does not)
    assert err <= 2 * bf16_err


@pytest.mark.parametrize("packed", [False, True])
def test_experts_skewed_routing_one_expert_owns_every_pair(packed):
    x, gu, dn, ids, wts, ref, bf16_err = _case(300, 8, 2, 256, 128, skew=True)      # 600 rows of expert 0: five row blocks
    assert _rel_err(_run_experts(x, gu, dn, ids, wts, packed), ref) <= 2 * bf16_err


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("m", [1, 17, 64])
@pytest.mark.parametrize("E,k", [(8, 2), (128, 8)])
def test_route_vs_fp64(E, k, m, norm):
    from nano_vllm_amd import ops
    g = torch.Generator().manual_seed(21 + m + E)
    # unit-variance x and router rows: logits ~ N(0, 16^2), so the top-9-of-128 spacings are O(1) and a gap under 1e-3
    # at one of the k boundaries is rare (these inputs: one token of the (128, 8), m = 64 case falls out = 1.6 %, none
    # elsewhere; an fp32 restatement on the CPU gets every kept token's ids right, weights within 2e-5 relative)
    x = torch.randn(m, 256, generator=g).bfloat16()
    rw = torch.randn(E, 256, generator=g).bfloat16()
    logits = x.double() @ rw.double().T
    p = logits.softmax(-1)
    top = logits.sort(-1, descending=True)
    keep = (top.values[:, :k] - top.values[:, 1:k + 1]).min(-1).values > 1e-3 if k < E else torch.ones(m, dtype=torch.bool)
    assert (~keep).float().mean().item() <= 0.02
    want_w = p.gather(1, top.indices[:, :k])
    if norm:
        want_w = want_w / want_w.sum(-1, keepdim=True)
    ids, wts = ops.moe_route(x.cuda(), rw.cuda(), k, norm)
    assert torch.equal(ids.cpu()[keep].long(), top.indices[:, :k][keep])
    # fp32 softmax of fp32 logits: a 256-term fp32 dot of O(1) products with partial sums up to ~60 carries
    # ~sqrt(256) x 2^-24 x 60 = 6e-5 of absolute logit error = relative error of p; 5e-4 leaves 8 x for the tails
    torch.testing.assert_close(wts.cpu()[keep].double(), want_w[keep], rtol=5e-4, atol=1e-9)


def test_route_exact_tie_goes_to_the_lower_index():
    from nano_vllm_amd import ops
    g = torch.Generator().manual_seed(3)
    rw = torch.randn(8, 256, generator=g).bfloat16()
    rw[6] = rw[2]                                     # experts 2 and 6 tie on every token
    x = (rw[2].float() * 0.05).bfloat16().repeat(5, 1)       # ... and are the two best
    ids, wts = ops.moe_route(x.cuda(), rw.cuda(), 2, True)
    assert ids.cpu().tolist() == [[2, 6]] * 5 and torch.equal(wts.cpu(), torch.full((5, 2), 0.5))


@pytest.mark.parametrize("m", [5, 150])               # a decode size; a prefill above the 64-row workspace cap (3 chunks)
def test_block_forward_equals_route_then_fp64_experts(m):
    from nano_vllm_amd import ops
    from nano_vllm_amd.qwen3 import Qwen3MoeSparseBlock
    torch.manual_seed(m)
    block = Qwen3MoeSparseBlock(256, 128, 8, 2, True).to(device="cuda", dtype=torch.bfloat16)
    block.gate.data.normal_()
    block.experts_gate_up.data.normal_(std=256 ** -0.5)
    block.experts_down.data.normal_(std=128 ** -0.5)
    block.set_workspace(torch.empty(block.workspace_bytes(64), dtype=torch.uint8, device="cuda"), 64)
    x = torch.randn(m, 256, device="cuda").bfloat16()
    ids, wts = ops.moe_route(x, block.gate.data, 2, True)
    args = [t.cpu() for t in (x, block.experts_gate_up.data, block.experts_down.data, ids, wts)]
    ref = _experts_ref(*args)
    assert _rel_err(block(x).cpu(), ref) <= 2 * _rel_err(_experts_ref(*args, torch.bfloat16), ref)
    assert block.pack_for_decode() > 0
    assert _rel_err(block(x).cpu(), ref) <= 2 * _rel_err(_experts_ref(*args, torch.bfloat16), ref)


def _moe_checkpoint(dense_path, same_experts):
    """qwen3-moe-tiny directory next to a dense qwen3-tiny one: attention / norms / embedding copied; every expert holds
    the dense MLP's matrices (`same_experts`: with routing weights summing to 1 the model IS the dense one) or its own."""
    from safetensors.torch import load_file, save_file
    from nano_vllm_amd.weights import build_offline_tokenizer, qwen3_config_dict, synth_tensor
    path = tempfile.mkdtemp(prefix="qwen3moe_")
    cfg = qwen3_config_dict("qwen3-moe-tiny", vocab_size=512, max_position_embeddings=2048)
    cfg["moe_intermediate_size"] = 512                # the dense tiny model's MLP width
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    build_offline_tokenizer(path)
    out = {}
    for name, t in load_file(os.path.join(dense_path, "model.safetensors")).items():
        if ".mlp." not in name:
            out[name] = t
            continue
        prefix, proj = name.split(".mlp.")
        out[prefix + ".mlp.gate.weight"] = synth_tensor(prefix + ".mlp.gate.weight", (8, 256), 0) * 50
        for e in range(8):
            key = f"{prefix}.mlp.experts.{e}.{proj}"
            out[key] = t.clone() if same_experts else synth_tensor(key, tuple(t.shape), 1)
    save_file(out, os.path.join(path, "model.safetensors"))
    return path


@pytest.fixture(scope="module")
def dense_ckpt():
    from nano_vllm_amd.weights import write_synthetic_checkpoint
    return write_synthetic_checkpoint(tempfile.mkdtemp(prefix="qwen3tiny_"), "qwen3-tiny", seed=0, vocab_size=512,
                                      max_position_embeddings=2048)


def test_moe_model_with_identical_experts_is_the_dense_model(dense_ckpt):
    from test_e2e_gpu import _check, _judge, _prompts, _run_ours
    path = _moe_checkpoint(dense_ckpt, same_experts=True)
    prompts, max_tokens = _prompts(4, 5, 300, 512, seed=11), [12, 20, 1, 9]
    tokens = {}
    for eager in (True, False):
        outs, rec, nblk = _run_ours(path, prompts, max_tokens, enforce_eager=eager, max_model_len=2048,
                                    num_kvcache_blocks=32, max_num_seqs=16)
        tokens[eager] = [o["token_ids"] for o in outs]
        _check(f"moe-tiny as dense, eager={eager}", _judge(dense_ckpt, prompts, max_tokens, rec, nblk, max_num_seqs=16),
               sum(max_tokens))
    assert tokens[True] == tokens[False]


def test_moe_model_graph_equals_eager_and_decode_is_a_replay(dense_ckpt):
    from nano_vllm_amd import LLM, SamplingParams
    from test_e2e_gpu import _prompts
    path = _moe_checkpoint(dense_ckpt, same_experts=False)
    prompts, tokens = _prompts(5, 5, 200, 512, seed=12), {}
    for eager in (True, False):
        llm = LLM(path, enforce_eager=eager, max_model_len=2048, num_kvcache_blocks=32, max_num_seqs=16)
        if not eager:
            assert llm.model_runner.graphs

            def no_eager_decode(*a, **kw):
                raise AssertionError("a decode step ran outside its captured graph")
            llm.model_runner._forward_decode = no_eager_decode
        outs = llm.generate(prompts, SamplingParams(temperature=0.0, max_tokens=16, ignore_eos=True), use_tqdm=False)
        tokens[eager] = [o["token_ids"] for o in outs]
        llm.exit()
    assert tokens[True] == tokens[False]
