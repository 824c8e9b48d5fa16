"""nvl_linear_wide_mxfp4 (W4A16: e2m1 codes, one e8m0 scale byte per row and 32 k) against x.double() @ W_deq.double().T
with W_deq built in torch from the codes and scales, the quantise / unpack pair against the plain restatement of the rule,
and weight_dtype="mxfp4_dense" end to end against the oracle on the quantised weights.

Acceptance formulas are those tests/test_fp8_weights_gpu.py applies to nvl_linear_wide_fp8 (they bound fp32 summation order
only: code x scale enters the matrix instruction exactly). x is scaled so that |acc| is O(1), the regime the 1e-4 absolute
floor was sized for there.

Which kernel form a case runs. The plan's interface returns the K split only (printed per case); the rest of this table is
fp4_plan's cost model (gemm_wide_mxfp4.hip) worked out by hand for these shapes: MT row tiles per row group (m = 1-16: 1,
17: 2, 48: 3, 80: 5, 112: 7, 144: 9; two paired groups at 145: 5, 200: 7, 256: 9), NT column tiles per wave, ring depth
(NT 2: 8, NT 4: 6, NT 8: 4 / 4 / 3 / 2 at MT <= 2 / 3 / 5 / 7), k steps per workgroup. "loop": steps >= ring, the reloading
ring body runs; otherwise only the no-reload tail does.
  bf16   (48, 128)       NT 2, 1 step, one ragged workgroup            (1296, 640)   NT 2, 81 tiles (no multiple of 3 NT), 5 steps
         (1280, 5120)    NT 2, split 10 (8 paired) + slab reduce       (6144, 4096)  m = 1: NT 8, split 16, 2 steps (tail only);
                                                                                     else NT 2, split 4 / 2, 8 / 16 steps: loop
  SiLU   (1632, 384)     NT 2, 3 steps, ragged                         (24576, 4096) NT 2, 32 steps: loop; m = 256: NT 4, paired, loop
         (49216, 1024)   NT 8 (NT 4 would need 257 workgroups), 8 steps: loop at every ring depth — m = 1, 17, 48: ring 4,
                         80: ring 3, 112: ring 2; 1538 pairs of tiles over 129 workgroups: the last one ragged
  slabs  (4096, 4096)    m <= 16, 48-144: NT 2, split 4, 8 steps: loop; m = 17: NT 4, split 8 (tail); 200 / 256: NT 4, paired, loop
         (5120, 3200)    m <= 144: NT 4, split 5, 5 steps (tail); m = 200: NT 8, ring 2, paired: loop; 256: NT 2, 25 steps
So every MT runs at NT 2, MT 1 / 2 / 3 / 5 / 7 at NT 8 with the ring body, MT 1 / 2 / 3 / 5 / 7 / 9 at NT 4.
"""
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
    """256 rows of x, codes uniform over all 16 values, scale bytes uniform in 118 ... 134 (every product a normal bf16),
    both laid out as the kernel reads them, W_deq in fp64 and the double-precision product (once per shape)."""
    from nano_vllm_amd import ops as _ops
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(256, k, generator=g) * 2.0 ** -12).to(BF16)
    c = torch.randint(0, 16, (n, k), generator=g)
    sb = torch.randint(118, 135, (n, k // 32), generator=g)
    wd = torch.where(c >= 8, -1.0, 1.0) * _MAG[c & 7] * torch.exp2(sb.double() - 127).repeat_interleave(32, 1)
    # codes [n/16][k/128][lane = 16 lq + l15][byte 4 kb + b]: row 16 t + l15, k = 128 s + 32 kb + 8 lq + 2 b | that k + 1 << 4
    nib = c.view(n // 16, 16, k // 128, 4, 4, 4, 2).permute(0, 2, 4, 1, 3, 5, 6)
    codes = (nib[..., 0] | nib[..., 1] << 4).to(torch.uint8).reshape(n // 16, k // 128, 64, 16)
    acc = (x.double().cuda() @ wd.cuda().t()).cpu()
    return x.cuda(), codes.cuda(), _ops.tile_scales_mxfp4(sb.to(torch.uint8).cuda()), acc, (x, wd)


@pytest.mark.parametrize("m", [1, 16, 17, 48, 112, 144, 145, 200, 256])
@pytest.mark.parametrize("n,k", [(48, 128), (1296, 640), (1280, 5120), (6144, 4096)])
def test_linear_wide_mxfp4_bf16(ops, m, n, k):
    x, codes, st, acc, _ = _inputs(n, k, 50)
    acc = acc[:m]
    print(f"plan (splits, workspace) {ops.linear_wide_mxfp4_plan(m, n, k, ops.LINEAR_BF16)}")
    y = ops.linear_wide_mxfp4(x[:m].contiguous(), codes, st, ops.LINEAR_BF16)
    err = (y.cpu().double() - acc).abs()
    print(f"max err {float(err.max()):.3e}, max (err - 2^-8 |acc|) {float((err - acc.abs() * 2.0 ** -8).max()):.3e}")
    assert y.shape == (m, n) and bool((err <= acc.abs() * 2.0 ** -8 + 1e-4).all())


@pytest.mark.parametrize("m,n,k", [(m, n, k) for n, k in [(1632, 384), (24576, 4096)] for m in (1, 144, 256)]
                         + [(m, 49216, 1024) for m in (1, 17, 48, 80, 112)])
def test_linear_wide_mxfp4_silu(ops, m, n, k):
    x, codes, st, acc, (xc, wd) = _inputs(n, k, 52)
    want = ref.silu_and_mul(acc[:m].float().to(BF16))
    # the 0.02 share is a condition on these inputs: a reference in ANOTHER fp32 summation order stays within it (CPU)
    perm = torch.randperm(k, generator=torch.Generator().manual_seed(53))
    other = ref.silu_and_mul((xc[:m].float()[:, perm] @ wd.float()[:, perm].t()).to(BF16))
    assert float((ref.bf16_ulp_diff(other, want) > 1).float().mean()) < 0.02
    print(f"plan (splits, workspace) {ops.linear_wide_mxfp4_plan(m, n, k, ops.LINEAR_SILU)}")
    y = ops.linear_wide_mxfp4(x[:m].contiguous(), codes, st, ops.LINEAR_SILU)
    assert y.shape == (m, n // 2)
    d = (y.cpu().float() - want.float()).abs()
    print(f"max |d| {float(d.max()):.3e} of {float(want.float().abs().max()):.3e}")
    assert float(d.max()) <= 2e-2 * float(want.float().abs().max())
    assert float((ref.bf16_ulp_diff(y.cpu(), want) > 1).float().mean()) < 0.02


@pytest.mark.parametrize("m", [16, 17, 48, 80, 112, 144, 200, 256])
@pytest.mark.parametrize("n,k", [(4096, 4096), (5120, 3200)])
def test_linear_wide_mxfp4_partials_into_add_rmsnorm(ops, m, n, k):
    x, codes, st, acc, _ = _inputs(n, k, 54)
    acc = acc[:m]
    splits, ws = ops.linear_wide_mxfp4_plan(m, n, k, ops.LINEAR_PARTIAL)
    parts = ops.linear_wide_mxfp4(x[:m].contiguous(), codes, st, ops.LINEAR_PARTIAL)
    assert ws == 0 and parts.shape == (splits, m, n) and parts.dtype == torch.float32
    err = float((parts.sum(0).cpu().double() - acc).abs().max())
    print(f"splits {splits}: max |sum - acc| {err:.3e} of {float(acc.abs().max()):.3e}")
    assert err <= 1e-4 * float(acc.abs().max()) + 1e-5
    g = torch.Generator().manual_seed(56)
    r = (torch.randn(m, n, generator=g) * 2).to(BF16)
    wn = (1 + 0.1 * torch.randn(n, generator=g)).to(BF16)
    seq = parts[0].cpu().clone()                      # slabs summed in split order, like the consumer does
    for i in range(1, splits):
        seq += parts[i].cpu()
    y_ref, r_ref = ref.add_rms_forward(seq.to(BF16), r, wn, 1e-6)
    dr = r.clone().cuda()
    y = ops.add_rmsnorm_splitk(parts, dr, wn.cuda(), 1e-6)
    assert int(ref.bf16_ulp_diff(dr.cpu(), r_ref).max()) <= 1 and int(ref.bf16_ulp_diff(y.cpu(), y_ref).max()) <= 2


def test_unpack_inverts_quant_pack_bit_for_bit(ops):
    g = torch.Generator().manual_seed(58)
    w = (torch.randn(96, 256, generator=g) * 2.0 ** (torch.arange(96) % 16 - 8)[:, None]).to(BF16)
    got = ops.unpack_mxfp4(*ops.quant_pack_mxfp4(w.cuda())).cpu()
    assert torch.equal(got.double(), mxfp4_ref(w)[2])


def _quantised(t):
    return torch.cat([mxfp4_ref(t[i:i + 512])[2] for i in range(0, t.shape[0], 512)]).to(t.dtype)


@pytest.mark.parametrize("name", ["qwen3-tiny-g5", "qwen3-8b-2l"])
def test_mxfp4_dense_greedy_parity_vs_oracle_on_quantised_weights(name):
    from nano_vllm_amd import LLM, SamplingParams
    from nano_vllm_amd.layers import LinearBase
    from nano_vllm_amd.weights import parameter_shapes, qwen3_config_dict, synth_tensor, write_synthetic_checkpoint
    from oracle.judge import judge_run
    vocab = 2048
    path = tempfile.mkdtemp(prefix=name.replace("-", "_") + "_mxfp4_")
    write_synthetic_checkpoint(path, name, with_weights=False, vocab_size=vocab, max_position_embeddings=4096)
    g = torch.Generator().manual_seed(23)
    prompts = [torch.randint(0, vocab, (int(torch.randint(8, 400, (1,), generator=g)),), generator=g).tolist() for _ in range(5)]
    max_tokens = [10, 6, 12, 3, 9]
    llm = LLM(path, enforce_eager=False, max_model_len=1024, num_kvcache_blocks=24, max_num_seqs=8, dummy_weights=True,
              weight_dtype="mxfp4_dense")
    runner, rec, open_step = llm.model_runner, [], []
    lins = {n: m for n, m in runner.model.named_modules() if isinstance(m, LinearBase)}
    assert len(lins) == 4 * 2
    for m in lins.values():
        n, k = m.weight.shape
        assert m.weight_mxfp4 is not None and m.weight_packed is None and m.weight_fp8_packed is None
        assert m.weight_mxfp4[0].shape == (n // 16, k // 128, 64, 16) and m.weight_mxfp4[1].shape == (n // 16, k // 128, 16, 4)
    held = {n: m.weight.data.cpu() for n, m in lins.items()}
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
    w = {n: _quantised(t) if n.endswith("_proj.weight") else t for n, t in w.items()}
    merged = {"qkv_proj": ("q_proj", "k_proj", "v_proj"), "gate_up_proj": ("gate_proj", "up_proj")}
    for n, t in held.items():                         # every parameter holds the dequantised matrix of its (merged) parts
        stem, leaf = n.rsplit(".", 1)
        assert torch.equal(t, torch.cat([w[f"{stem}.{p}.weight"] for p in merged.get(leaf, (leaf,))])), n
    v = judge_run(cfg, w, prompts, max_tokens, rec, nblk, device="cuda", max_num_seqs=8)
    print(v.line(name + " mxfp4_dense weights"))
    assert v.rows >= sum(max_tokens) and v.ok(), v.violations[:5]
