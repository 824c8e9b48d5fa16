"""nvl_linear_wide_fp8 (W8A16: e4m3 weights, fp32 scale per 16-row tile x 128-column k block) against
x.double() @ (w8.double() * S).T, and weight_dtype="fp8" end to end against the oracle on the quantised weights.

Acceptance formulas are those tests/test_kernels_gpu.py applies to nvl_linear_wide (they bound fp32 summation order only).
x is scaled so that |acc| is O(1), the regime the 1e-4 absolute floor of the bf16 formula was sized for there.
"""
import tempfile
from functools import lru_cache

import pytest
import torch

from oracle import ops as ref

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from nano_vllm_amd import ops as _ops
    _ops.load_library()
    return _ops


@lru_cache(None)
def _inputs(n, k, seed):
    """256 rows of x, e4m3 weights over the full finite range, independent non-power-of-two scales over > 2 decades,
    the double-precision product and the device copies (computed once per shape; tests slice the rows they use)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(256, k, generator=g) * 2.0 ** -12).to(BF16)
    bits = torch.randint(0, 127, (n, k), generator=g) + 128 * torch.randint(0, 2, (n, k), generator=g)   # no NaN (0x7f / 0xff)
    w8 = bits.to(torch.uint8).view(torch.float8_e4m3fn)
    s = torch.exp2(torch.rand(n // 16, k // 128, generator=g) * 7 - 6) * (1 + torch.rand(n // 16, k // 128, generator=g))
    wd = w8.float().double() * s.double().repeat_interleave(16, 0).repeat_interleave(128, 1)
    acc = (x.double().cuda() @ wd.cuda().t()).cpu()
    from nano_vllm_amd import ops as _ops
    return x.cuda(), _ops.pack_weight_tiles_fp8(w8.cuda()), s.cuda(), acc


@pytest.mark.parametrize("m", [1, 16, 17, 144, 145, 256])
@pytest.mark.parametrize("n,k", [(48, 128), (1296, 640), (1280, 5120), (6144, 4096)])
def test_linear_wide_fp8_bf16(ops, m, n, k):
    x, wp, s, acc = _inputs(n, k, 40)
    acc = acc[:m]
    y = ops.linear_wide_fp8(x[:m].contiguous(), wp, s, ops.LINEAR_BF16)
    err = (y.cpu().double() - acc).abs()
    print(f"max err {float(err.max()):.3e}, max (err - 2^-8 |acc|) {float((err - acc.abs() * 2.0 ** -8).max()):.3e}")
    assert y.shape == (m, n) and bool((err <= acc.abs() * 2.0 ** -8 + 1e-4).all())


@pytest.mark.parametrize("m", [1, 144, 256])
@pytest.mark.parametrize("n,k", [(1632, 384), (24576, 4096)])
def test_linear_wide_fp8_silu(ops, m, n, k):
    x, wp, s, acc = _inputs(n, k, 42)
    y = ops.linear_wide_fp8(x[:m].contiguous(), wp, s, ops.LINEAR_SILU)
    want = ref.silu_and_mul(acc[:m].float().to(BF16))
    assert y.shape == (m, n // 2)
    d = (y.cpu().float() - want.float()).abs()
    print(f"max |d| {float(d.max()):.3e} of {float(want.float().abs().max()):.3e}")
    assert float(d.max()) <= 2e-2 * float(want.float().abs().max())
    assert float((ref.bf16_ulp_diff(y.cpu(), want) > 1).float().mean()) < 0.02


@pytest.mark.parametrize("m", [16, 144, 256])
@pytest.mark.parametrize("n,k", [(4096, 4096), (5120, 3200)])
def test_linear_wide_fp8_partials_into_add_rmsnorm(ops, m, n, k):
    x, wp, s, acc = _inputs(n, k, 44)
    acc = acc[:m]
    splits, ws = ops.linear_wide_fp8_plan(m, n, k, ops.LINEAR_PARTIAL)
    parts = ops.linear_wide_fp8(x[:m].contiguous(), wp, s, ops.LINEAR_PARTIAL)
    assert ws == 0 and parts.shape == (splits, m, n) and parts.dtype == torch.float32
    err = float((parts.sum(0).cpu().double() - acc).abs().max())
    print(f"splits {splits}: max |sum - acc| {err:.3e} of {float(acc.abs().max()):.3e}")
    assert err <= 1e-4 * float(acc.abs().max()) + 1e-5
    g = torch.Generator().manual_seed(46)
    r = (torch.randn(m, n, generator=g) * 2).to(BF16)
    wn = (1 + 0.1 * torch.randn(n, generator=g)).to(BF16)
    seq = parts[0].cpu().clone()                      # slabs summed in split order, like the consumer does
    for i in range(1, splits):
        seq += parts[i].cpu()
    y_ref, r_ref = ref.add_rms_forward(seq.to(BF16), r, wn, 1e-6)
    dr = r.clone().cuda()
    y = ops.add_rmsnorm_splitk(parts, dr, wn.cuda(), 1e-6)
    assert int(ref.bf16_ulp_diff(dr.cpu(), r_ref).max()) <= 1 and int(ref.bf16_ulp_diff(y.cpu(), y_ref).max()) <= 2


def test_pack_weight_tiles_fp8_layout(ops):
    """packed[n/16][k/64][64 lanes][16 bytes]: lane = 16 * (k % 32 // 8) + row % 16 holds its 8 bytes of k block 2 j, then
    its 8 bytes of k block 2 j + 1."""
    n, k = 96, 256
    w = torch.arange(n * k).remainder(251).to(torch.uint8).view(n, k)
    got = ops.pack_weight_tiles_fp8(w.view(torch.float8_e4m3fn).cuda()).cpu().view(torch.uint8)
    want = w.view(n // 16, 16, k // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous().view(n, k)
    assert torch.equal(got, want)


def _block_quant(w):
    """Reference quantiser: 128 x 128 blocks, power-of-two scale, e4m3 cast, dequantised (exact in bf16)."""
    n, k = w.shape
    b = w.float().view(n // 128, 128, k // 128, 128)
    amax = b.abs().amax(dim=(1, 3), keepdim=True)
    s = torch.where(amax > 0, torch.exp2(torch.ceil(torch.log2(amax / 448.0))), torch.ones_like(amax))
    return ((b / s).to(torch.float8_e4m3fn).float() * s).view(n, k).to(w.dtype)


@pytest.mark.parametrize("name", ["qwen3-tiny-g5", "qwen3-8b-2l"])
def test_fp8_weights_greedy_parity_vs_oracle_on_quantised_weights(name):
    from nano_vllm_amd import LLM, SamplingParams
    from nano_vllm_amd.layers import LinearBase
    from nano_vllm_amd.weights import parameter_shapes, qwen3_config_dict, synth_tensor, write_synthetic_checkpoint
    from oracle.judge import judge_run
    vocab = 2048
    path = tempfile.mkdtemp(prefix=name.replace("-", "_") + "_fp8_")
    write_synthetic_checkpoint(path, name, with_weights=False, vocab_size=vocab, max_position_embeddings=4096)
    g = torch.Generator().manual_seed(23)
    prompts = [torch.randint(0, vocab, (int(torch.randint(8, 400, (1,), generator=g)),), generator=g).tolist() for _ in range(5)]
    max_tokens = [10, 6, 12, 3, 9]
    llm = LLM(path, enforce_eager=False, max_model_len=1024, num_kvcache_blocks=24, max_num_seqs=8, dummy_weights=True,
              weight_dtype="fp8")
    runner, rec, open_step = llm.model_runner, [], []
    lins = [m for m in runner.model.modules() if isinstance(m, LinearBase)]
    assert len(lins) == 4 * 2 and all(m.weight_fp8_packed is not None and m.weight_packed is None for m in lins)
    assert all(m.weight_fp8_packed.numel() == m.weight.numel() and m.weight_scale.shape == (m.weight.shape[0] // 16, m.weight.shape[1] // 128)
               for m in lins)
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
    cfg = qwen3_config_dict(name, vocab_size=vocab, max_position_embeddings=4096)
    w = {n: synth_tensor(n, s, 0, device="cuda").cpu() for n, s in parameter_shapes(cfg).items()}
    w = {n: _block_quant(t) if n.endswith("_proj.weight") else t for n, t in w.items()}
    v = judge_run(cfg, w, prompts, max_tokens, rec, nblk, device="cuda", max_num_seqs=8)
    print(v.line(name + " fp8 weights"))
    assert v.rows >= sum(max_tokens) and v.ok(), v.violations[:5]
