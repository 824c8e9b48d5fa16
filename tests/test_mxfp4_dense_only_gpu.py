"""nvl_linear_tile_mxfp4 (W4A16 tile GEMM for any row count) against x.double() @ W_deq.double().T with W_deq built in torch
from the codes and scales, and weight_dtype="mxfp4_dense_only" end to end against the oracle on the quantised weights, with
the bf16 projections released.

Acceptance formulas are those of tests/test_fp8_weights_gpu.py (they bound the fp32 summation order and one bf16 rounding:
code x scale enters the matrix instruction exactly; x is scaled so that |acc| is O(1), the regime the 1e-4 absolute floor
was sized for). Shapes: a single k step, a ragged last column group (81 tiles), partial row tiles, rows past one row block of
each tile shape (64 / 128 rows), and a K walk longer than the ring and the x stages."""
import tempfile
from functools import lru_cache

import pytest
import torch

from oracle import ops as ref
from test_moe_mxfp4_host import mxfp4_ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
_MAG = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=torch.float64)


@pytest.fixture(scope="module")
def ops():
    from nano_vllm_amd import ops as _ops
    _ops.load_library()
    return _ops


@lru_cache(None)
def _inputs(n, k, seed):
    """600 rows of x, codes uniform over all 16 values, scale bytes uniform in 118 ... 134 (every product a normal bf16),
    both laid out as the kernel reads them, W_deq in fp64 and the double-precision product (once per shape)."""
    from nano_vllm_amd import ops as _ops
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(600, k, generator=g) * 2.0 ** -12).to(BF16)
    c = torch.randint(0, 16, (n, k), generator=g)
    sb = torch.randint(118, 135, (n, k // 32), generator=g)
    wd = torch.where(c >= 8, -1.0, 1.0) * _MAG[c & 7] * torch.exp2(sb.double() - 127).repeat_interleave(32, 1)
    # codes [n/16][k/128][lane = 16 lq + l15][byte 4 kb + b]: row 16 t + l15, k = 128 s + 32 kb + 8 lq + 2 b | that k + 1 << 4
    nib = c.view(n // 16, 16, k // 128, 4, 4, 4, 2).permute(0, 2, 4, 1, 3, 5, 6)
    codes = (nib[..., 0] | nib[..., 1] << 4).to(torch.uint8).reshape(n // 16, k // 128, 64, 16)
    acc = (x.double().cuda() @ wd.cuda().t()).cpu()
    return x.cuda(), codes.cuda(), _ops.tile_scales_mxfp4(sb.to(torch.uint8).cuda()), acc, (x, wd)


@pytest.mark.parametrize("tile", ["small", "big"])           # 64 x 128 / 128 x 256 outputs per workgroup
@pytest.mark.parametrize("m", [1, 17, 257, 300, 512, 600])
@pytest.mark.parametrize("n,k", [(48, 128), (1296, 640), (4096, 1024)])
def test_linear_tile_mxfp4_bf16(ops, monkeypatch, tile, m, n, k):
    monkeypatch.setenv("NVL_TILE_MXFP4", tile)
    x, codes, st, acc, _ = _inputs(n, k, 50)
    acc = acc[:m]
    y = ops.linear_tile_mxfp4(x[:m].contiguous(), codes, st, ops.LINEAR_BF16)
    err = (y.cpu().double() - acc).abs()
    print(f"max err {float(err.max()):.3e}, max (err - 2^-8 |acc|) {float((err - acc.abs() * 2.0 ** -8).max()):.3e}")
    assert y.shape == (m, n) and bool((err <= acc.abs() * 2.0 ** -8 + 1e-4).all())


@pytest.mark.parametrize("tile", ["small", "big"])
@pytest.mark.parametrize("m", [257, 600])
@pytest.mark.parametrize("n,k", [(1632, 384), (2560, 1024)])
def test_linear_tile_mxfp4_silu(ops, monkeypatch, tile, m, n, k):
    monkeypatch.setenv("NVL_TILE_MXFP4", tile)
    x, codes, st, acc, (xc, wd) = _inputs(n, k, 52)
    want = ref.silu_and_mul(acc[:m].float().to(BF16))
    # the 0.02 share is a condition on these inputs: a reference in ANOTHER fp32 summation order stays within it (CPU)
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(53))
    other = ref.silu_and_mul((xc[:m].float()[:, perm] @ wd.float()[:, perm].t()).to(BF16))
    assert float((ref.bf16_ulp_diff(other, want) > 1).float().mean()) < 0.02
    y = ops.linear_tile_mxfp4(x[:m].contiguous(), codes, st, ops.LINEAR_SILU)
    assert y.shape == (m, n // 2)
    d = (y.cpu().float() - want.float()).abs()
    print(f"max |d| {float(d.max()):.3e} of {float(want.float().abs().max()):.3e}")
    assert float(d.max()) <= 2e-2 * float(want.float().abs().max())
    assert float((ref.bf16_ulp_diff(y.cpu(), want) > 1).float().mean()) < 0.02


def test_linear_tile_mxfp4_leaves_rows_past_m_untouched(ops):
    x, codes, st, acc, _ = _inputs(1296, 640, 50)
    out = torch.full((384, 1296), 7.0, dtype=BF16, device="cuda")
    ops.linear_tile_mxfp4(x[:300].contiguous(), codes, st, ops.LINEAR_BF16, out=out)
    assert bool((out[300:] == 7.0).all())
    assert bool(((out[:300].cpu().double() - acc[:300]).abs() <= acc[:300].abs() * 2.0 ** -8 + 1e-4).all())


def _quantised(t):
    return torch.cat([mxfp4_ref(t[i:i + 512])[2] for i in range(0, t.shape[0], 512)]).to(t.dtype)


@pytest.mark.parametrize("name", ["qwen3-tiny-g5", "qwen3-8b-2l"])
def test_mxfp4_dense_only_greedy_parity_vs_oracle_on_quantised_weights_with_bf16_released(name):
    from nano_vllm_amd import LLM, SamplingParams
    from nano_vllm_amd.layers import LinearBase
    from nano_vllm_amd.weights import parameter_shapes, qwen3_config_dict, synth_tensor, write_synthetic_checkpoint
    from oracle.judge import judge_run
    vocab = 2048
    path = tempfile.mkdtemp(prefix=name.replace("-", "_") + "_mxfp4only_")
    write_synthetic_checkpoint(path, name, with_weights=False, vocab_size=vocab, max_position_embeddings=4096)
    g = torch.Generator().manual_seed(29)
    prompts = [torch.randint(0, vocab, (n,), generator=g).tolist() for n in (300, 40, 17, 120, 9)]   # one 486-row prefill step
    max_tokens = [10, 6, 12, 3, 9]
    llm = LLM(path, enforce_eager=False, max_model_len=1024, num_kvcache_blocks=24, max_num_seqs=8, dummy_weights=True,
              weight_dtype="mxfp4_dense_only")
    runner, rec, open_step = llm.model_runner, [], []
    lins = [m for m in runner.model.modules() if isinstance(m, LinearBase)]
    assert len(lins) == 4 * 2 and all(m.weight.numel() == 0 and m.weight_mxfp4 is not None for m in lins)
    assert all(m.weight_packed is None and m.weight_fp8_packed is None for m in lins)
    orig = runner.call

    def spy(method, *args):                           # one record per engine step: batch, block tables, sampled tokens
        if method in ("decode_begin", "run"):
            seqs, prefill = (args[0], False) if method == "decode_begin" else args
            open_step.append(dict(prefill=prefill, seq_ids=[s.seq_id for s in seqs], tables=[list(s.block_table) for s in seqs],
                                  sched=[s.num_scheduled_tokens for s in seqs]))
        out = orig(method, *args)
        if method in ("run", "decode_end"):
            rec.append(dict(open_step.pop(0), tokens=list(out)))
        return out

    runner.call = spy
    outs = llm.generate(prompts, [SamplingParams(temperature=0.0, max_tokens=t, ignore_eos=True) for t in max_tokens], use_tqdm=False)
    nblk = llm.config.num_kvcache_blocks
    runner.call = orig
    llm.exit()
    assert [len(o["token_ids"]) for o in outs] == max_tokens
    assert rec[0]["prefill"] and sum(rec[0]["sched"]) > 256                                    # the tile kernel's rows
    cfg = qwen3_config_dict(name, vocab_size=vocab, max_position_embeddings=4096)
    w = {n: synth_tensor(n, s, 0, device="cuda").cpu() for n, s in parameter_shapes(cfg).items()}
    w = {n: _quantised(t) if n.endswith("_proj.weight") else t for n, t in w.items()}
    v = judge_run(cfg, w, prompts, max_tokens, rec, nblk, device="cuda", max_num_seqs=8)
    print(v.line(name + " mxfp4_dense_only weights"))
    assert v.rows >= sum(max_tokens) and v.ok(), v.violations[:5]
