"""nvl_linear_tile_fp8 (W8A16 tile GEMM for any row count, power-of-two scales) against x.double() @ W_deq.double().T, and
weight_dtype="fp8_only" end to end against the oracle on the quantised weights, with the bf16 projections released.

Acceptance formulas are those of tests/test_fp8_weights_gpu.py (they bound the fp32 summation order and one bf16 rounding;
x is scaled so that |acc| is O(1), the regime the 1e-4 absolute floor was sized for)."""
import tempfile
from functools import lru_cache

import pytest
import torch

from oracle import ops as ref
from test_fp8_weights_gpu import _block_quant

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from nano_vllm_amd import ops as _ops
    _ops.load_library()
    return _ops


@lru_cache(None)
def _inputs(n, k, seed):
    """600 rows of x, e4m3 weights over the full finite range, power-of-two scales over 7 binades (2^-6 .. 2^0: the
    smallest product, 2^-9 x 2^-6, is a normal bf16), the double-precision product and the device copies (once per shape)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(600, k, generator=g) * 2.0 ** -12).to(BF16)
    bits = torch.randint(0, 127, (n, k), generator=g) + 128 * torch.randint(0, 2, (n, k), generator=g)   # no NaN (0x7f / 0xff)
    w8 = bits.to(torch.uint8).view(torch.float8_e4m3fn)
    s = torch.exp2(torch.randint(-6, 1, (n // 16, k // 128), generator=g).float())
    wd = w8.float().double() * s.double().repeat_interleave(16, 0).repeat_interleave(128, 1)
    acc = (x.double().cuda() @ wd.cuda().t()).cpu()
    from nano_vllm_amd import ops as _ops
    return x.cuda(), _ops.pack_weight_tiles_fp8(w8.cuda()), s.cuda(), acc


@pytest.mark.parametrize("tile", ["small", "big"])           # 128 x 64 / 256 x 128 outputs per workgroup
@pytest.mark.parametrize("m", [1, 17, 257, 300, 512, 600])
@pytest.mark.parametrize("n,k", [(48, 128), (1296, 640), (4096, 1024)])
def test_linear_tile_fp8_bf16(ops, monkeypatch, tile, m, n, k):
    monkeypatch.setenv("NVL_TILE_FP8", tile)
    x, wp, s, acc = _inputs(n, k, 50)
    acc = acc[:m]
    y = ops.linear_tile_fp8(x[:m].contiguous(), wp, s, ops.LINEAR_BF16)
    err = (y.cpu().double() - acc).abs()
    print(f"max err {float(err.max()):.3e}, max (err - 2^-8 |acc|) {float((err - acc.abs() * 2.0 ** -8).max()):.3e}")
    assert y.shape == (m, n) and bool((err <= acc.abs() * 2.0 ** -8 + 1e-4).all())


@pytest.mark.parametrize("tile", ["small", "big"])
@pytest.mark.parametrize("m", [257, 600])
@pytest.mark.parametrize("n,k", [(1632, 384), (2560, 1024)])
def test_linear_tile_fp8_silu(ops, monkeypatch, tile, m, n, k):
    monkeypatch.setenv("NVL_TILE_FP8", tile)
    x, wp, s, acc = _inputs(n, k, 52)
    y = ops.linear_tile_fp8(x[:m].contiguous(), wp, s, ops.LINEAR_SILU)
    want = ref.silu_and_mul(acc[:m].float().to(BF16))
    assert y.shape == (m, n // 2)
    d = (y.cpu().float() - want.float()).abs()
    print(f"max |d| {float(d.max()):.3e} of {float(want.float().abs().max()):.3e}")
    assert float(d.max()) <= 2e-2 * float(want.float().abs().max())
    assert float((ref.bf16_ulp_diff(y.cpu(), want) > 1).float().mean()) < 0.02


def test_linear_tile_fp8_leaves_rows_past_m_untouched(ops):
    x, wp, s, acc = _inputs(1296, 640, 50)
    out = torch.full((384, 1296), 7.0, dtype=BF16, device="cuda")
    ops.linear_tile_fp8(x[:300].contiguous(), wp, s, ops.LINEAR_BF16, out=out)
    assert bool((out[300:] == 7.0).all())
    assert bool(((out[:300].cpu().double() - acc[:300]).abs() <= acc[:300].abs() * 2.0 ** -8 + 1e-4).all())


@pytest.mark.parametrize("name", ["qwen3-tiny-g5", "qwen3-8b-2l"])
def test_fp8_only_greedy_parity_vs_oracle_on_quantised_weights_with_bf16_released(name):
    from nano_vllm_amd import LLM, SamplingParams
    from nano_vllm_amd.layers import LinearBase
    from nano_vllm_amd.weights import parameter_shapes, qwen3_config_dict, synth_tensor, write_synthetic_checkpoint
    from oracle.judge import judge_run
    vocab = 2048
    path = tempfile.mkdtemp(prefix=name.replace("-", "_") + "_fp8only_")
    write_synthetic_checkpoint(path, name, with_weights=False, vocab_size=vocab, max_position_embeddings=4096)
    g = torch.Generator().manual_seed(29)
    prompts = [torch.randint(0, vocab, (n,), generator=g).tolist() for n in (300, 40, 17, 120, 9)]   # one 486-row prefill step
    max_tokens = [10, 6, 12, 3, 9]
    llm = LLM(path, enforce_eager=False, max_model_len=1024, num_kvcache_blocks=24, max_num_seqs=8, dummy_weights=True,
              weight_dtype="fp8_only")
    runner, rec, open_step = llm.model_runner, [], []
    lins = [m for m in runner.model.modules() if isinstance(m, LinearBase)]
    assert len(lins) == 4 * 2 and all(m.weight_fp8_packed is not None and m.weight_packed is None for m in lins)
    assert all(m.weight.numel() == 0 and m.weight_fp8_packed.shape == m.nk for m in lins)
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
    assert rec[0]["prefill"] and sum(rec[0]["sched"]) > 256 and max(rec[0]["sched"]) > 256     # the tile kernel's rows
    cfg = qwen3_config_dict(name, vocab_size=vocab, max_position_embeddings=4096)
    w = {n: synth_tensor(n, s, 0, device="cuda").cpu() for n, s in parameter_shapes(cfg).items()}
    w = {n: _block_quant(t) if n.endswith("_proj.weight") else t for n, t in w.items()}
    v = judge_run(cfg, w, prompts, max_tokens, rec, nblk, device="cuda", max_num_seqs=8)
    print(v.line(name + " fp8_only weights"))
    assert v.rows >= sum(max_tokens) and v.ok(), v.violations[:5]
