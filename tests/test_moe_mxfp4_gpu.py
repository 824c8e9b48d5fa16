"""MXFP4 expert weights on the MI355X (csrc/moe_mxfp4.hip): the quantiser bit for bit against the restatement of the
rule, the grouped expert GEMMs, the model block and the engine against fp64 / the dense oracle on the dequantised weights."""
import functools
import os
import tempfile

import pytest
import torch

from test_moe_gpu import _experts_ref, _moe_checkpoint, _rel_err
from test_moe_mxfp4_host import mxfp4_ref

pytestmark = pytest.mark.gpu


def _block_scaled(shape, g, lo, hi):
    """randn with every 32-block of the last axis times 2^randint(lo, hi), as bf16."""
    w = torch.randn(*shape, generator=g).view(-1, 32)
    return (w * 2.0 ** torch.randint(lo, hi + 1, (w.shape[0], 1), generator=g)).view(*shape).bfloat16()


@pytest.mark.parametrize("n,k", [(32, 256), (48, 384)])
def test_quant_pack_equals_the_restatement_bit_for_bit(n, k):
    from nano_vllm_amd import ops
    w = _block_scaled((n, k), torch.Generator().manual_seed(n), -6, 3)
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    w[3, 32:64] = 0                                                          # an all-zero block
    w[17, 64:96] = (torch.cat([ties, -ties, torch.tensor([4.0, -4.0, 0.0]), ties[:3] * 0.5, ties, ties[:5]]) * 2.0 ** -5).bfloat16()
    w[n - 1, k - 32:] = (torch.cat([torch.tensor([7.5, 4.0, -7.0, -0.1]), torch.linspace(-4, 4, 28)]) * 2.0 ** 3).bfloat16()
    want_codes, want_scales, _ = mxfp4_ref(w)
    codes, scales = ops.quant_pack_mxfp4(w.cuda())
    # [tile, step, lq, l15, kb, b] -> row 16 tile + l15, byte 64 step + 16 kb + 4 lq + b
    got = codes.cpu().view(n // 16, k // 128, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(n, k // 2)
    assert torch.equal(scales.cpu(), want_scales)
    assert torch.equal(got, want_codes)


@functools.lru_cache(None)
def _weights(E, hidden, inter):
    """Block-scaled expert matrices of one shape and their dequantised restatement (made once per shape, shared)."""
    g = torch.Generator().manual_seed(E + hidden)
    gu = _block_scaled((E, 2 * inter, hidden), g, -4, 3) / hidden ** 0.5
    dn = _block_scaled((E, hidden, inter), g, -4, 3) / inter ** 0.5
    return (gu, dn) + tuple(mxfp4_ref(t.view(-1, t.shape[-1]))[2].view(t.shape) for t in (gu, dn))


@functools.lru_cache(None)
def _case(m, E, k, hidden, inter, skew=False):
    """test_moe_gpu._case with block-scaled weights: (x, gu, dn, ids, wts) with the DEQUANTISED weights' fp64 reference
    and the bf16 restatement's error on them (made once, shared)."""
    g = torch.Generator().manual_seed(1000 * m + E)
    x = torch.randn(m, hidden, generator=g).bfloat16()
    gu, dn, gu_q, dn_q = _weights(E, hidden, inter)
    ids = torch.rand(m, E, generator=g).argsort(-1)[:, :k].int().contiguous()
    if skew:
        ids.zero_()
    wts = torch.rand(m, k, generator=g) + 0.1
    wts = (wts / wts.sum(-1, keepdim=True)).float()
    ref = _experts_ref(x, gu_q, dn_q, ids, wts)
    return x, gu, dn, ids, wts, ref, _rel_err(_experts_ref(x, gu_q, dn_q, ids, wts, torch.bfloat16), ref)


def _check_experts(name, x, gu, dn, ids, wts, ref, bf16_err):
    from nano_vllm_amd import ops
    E, hidden, inter = dn.shape
    x, ids, wts = x.cuda(), ids.cuda(), wts.cuda()
    q = ops.quant_pack_mxfp4(gu.cuda().view(-1, hidden)) + ops.quant_pack_mxfp4(dn.cuda().view(-1, inter))
    ws = torch.empty(ops.moe_workspace_bytes(x.shape[0], hidden, inter, E, ids.shape[1]), dtype=torch.uint8, device="cuda")
    outs = []
    for _ in range(2):
        ops.moe_plan(ids, E, ws)
        outs.append(ops.moe_experts_mxfp4(x, *q, ids, wts, ws).cpu())
    assert torch.equal(outs[0], outs[1]), "two calls on the same inputs differ"
    err = _rel_err(outs[0], ref)
    print(f"{name}: max|d| / rms kernel {err:.5f}, bf16 restatement {bf16_err:.5f}")
    # the project's bound for the expert GEMMs: 2 x the bf16 restatement's own error on the same (dequantised) weights
    assert err <= 2 * bf16_err


@pytest.mark.parametrize("cfg", [(8, 2, 256, 128), (128, 8, 256, 384), (8, 2, 384, 128)])     # last: hidden % 256 == 128
@pytest.mark.parametrize("m", [1, 16, 17, 130, 300])
def test_experts_with_given_ids_vs_fp64(m, cfg):
    _check_experts(f"m={m} cfg={cfg}", *_case(m, *cfg))


def test_experts_skewed_routing_one_expert_owns_every_pair():
    _check_experts("skew", *_case(300, 8, 2, 256, 128, skew=True))         # 600 rows of expert 0: five row blocks


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
    gu_q, dn_q = (mxfp4_ref(p.data.cpu().view(-1, p.shape[-1]))[2].view(p.shape) for p in (block.experts_gate_up, block.experts_down))
    assert block.pack_for_decode(weight_dtype="mxfp4") == (gu_q.numel() + dn_q.numel()) * 17 // 32
    assert block.experts_gate_up.numel() == 0 and block.experts_down.numel() == 0
    x = torch.randn(m, 256, device="cuda").bfloat16()
    ids, wts = ops.moe_route(x, block.gate.data, 2, True)
    args = (x.cpu(), gu_q, dn_q, ids.cpu(), wts.cpu())
    ref = _experts_ref(*args)
    assert _rel_err(block(x).cpu(), ref) <= 2 * _rel_err(_experts_ref(*args, torch.bfloat16), ref)


def test_moe_model_with_identical_mxfp4_experts_is_the_dense_model():
    """A dense checkpoint whose MLP matrices are MXFP4-representable: quantising its identical-experts MoE twin at load is
    lossless, so the mxfp4 engine is judged against the dense oracle on that dense checkpoint."""
    from safetensors.torch import load_file, save_file
    from nano_vllm_amd.weights import write_synthetic_checkpoint
    from test_e2e_gpu import _check, _judge, _prompts, _run_ours
    dense = write_synthetic_checkpoint(tempfile.mkdtemp(prefix="qwen3tiny_q_"), "qwen3-tiny", seed=0, vocab_size=512,
                                       max_position_embeddings=2048)
    file = os.path.join(dense, "model.safetensors")
    save_file({name: mxfp4_ref(t)[2].to(t.dtype) if ".mlp." in name else t for name, t in load_file(file).items()}, file)
    path = _moe_checkpoint(dense, same_experts=True)
    prompts, max_tokens = _prompts(4, 5, 300, 512, seed=11), [12, 20, 1, 9]
    tokens = {}
    for eager in (True, False):
        outs, rec, nblk = _run_ours(path, prompts, max_tokens, enforce_eager=eager, max_model_len=2048,
                                    num_kvcache_blocks=32, max_num_seqs=16, weight_dtype="mxfp4")
        tokens[eager] = [o["token_ids"] for o in outs]
        _check(f"mxfp4 moe-tiny as dense, eager={eager}", _judge(dense, prompts, max_tokens, rec, nblk, max_num_seqs=16),
               sum(max_tokens))
    assert tokens[True] == tokens[False]
