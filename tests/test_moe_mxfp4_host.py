"""MXFP4 expert weights without a GPU: the plain restatement of the quantisation rule (shared with the GPU tests), what
`Config` accepts for weight_dtype="mxfp4", and host-side argument validation of the two entry points."""
import pytest
import torch

from test_moe_host import moe_dir  # noqa: F401  (fixture: a qwen3-moe-tiny directory)

_MAG = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6], dtype=torch.float64)


def mxfp4_ref(w):
    """bf16 [N, K] -> (codes uint8 [N, K/2], low nibble = even k; scale bytes uint8 [N, K/32]; dequantised fp64 [N, K])."""
    n, k = w.shape
    b = w.double().view(n, k // 32, 32)
    a = b.abs().amax(-1, keepdim=True)
    e = (torch.frexp(a)[1] - 3).clamp(min=-126)              # frexp: a = f * 2^x, f in [0.5, 1): floor(log2 a) = x - 1
    e = torch.where(a == 0, torch.zeros_like(e), e)
    v = b.abs() / torch.exp2(e.double())                       # exact
    # nearest code magnitude; an odd code pays 2^-12 (a non-tie differs by >= 2^-9: bf16 has 8 significant bits)
    code = ((v.float()[..., None] - _MAG.float()).abs() + 2.0 ** -12 * (torch.arange(8) % 2)).argmin(-1)   # (exact in fp32)
    deq = torch.where(b < 0, -1.0, 1.0) * _MAG[code] * torch.exp2(e.double())
    code = (code | (b < 0) * 8).view(n, k // 2, 2)
    return (code[..., 0] | code[..., 1] << 4).to(torch.uint8), (e + 127).to(torch.uint8).view(n, k // 32), deq.view(n, k)


def test_restatement_is_idempotent_on_its_own_output():
    w = (torch.randn(16, 256, generator=torch.Generator().manual_seed(0)) * 2.0 ** torch.arange(-8, 8)[:, None]).bfloat16()
    codes, scales, deq = mxfp4_ref(w)
    assert torch.equal(deq.bfloat16().double(), deq)           # code * scale is a bf16 value
    codes2, scales2, deq2 = mxfp4_ref(deq.bfloat16())             # (codes: a negative w that rounds to 0 is code 8, -0,
    assert torch.equal(scales2, scales) and torch.equal(deq2, deq)   # and comes back as code 0: the values are equal)


def test_config_accepts_mxfp4_for_a_moe_directory_only(moe_dir, tmp_path):  # noqa: F811
    import json
    from nano_vllm_amd.api import Config
    from nano_vllm_amd.weights import qwen3_config_dict
    assert Config(moe_dir(), weight_dtype="mxfp4").weight_dtype == "mxfp4"
    (tmp_path / "dense").mkdir()
    (tmp_path / "dense" / "config.json").write_text(json.dumps(qwen3_config_dict("qwen3-tiny", vocab_size=512)))
    with pytest.raises(ValueError, match="mxfp4"):
        Config(str(tmp_path / "dense"), weight_dtype="mxfp4")


def test_host_side_argument_validation_without_gpu():
    from nano_vllm_amd import ops
    lib = ops.load_library()
    for args, msg in (((None, 32, 256, 256, 256, None), b"null pointer"), ((256, 24, 256, 256, 256, None), b"n=24"),
                      ((256, 32, 192, 256, 256, None), b"k=192"), ((256, 32, 256, 264, 256, None), b"aligned")):
        assert lib.nvl_quant_pack_mxfp4(*args) == -1 and msg in lib.nvl_last_error(), args
    cap = ops.moe_workspace_bytes(4, 256, 128, 8, 2)
    good = dict(x=256, gu=256, gus=256, dn=256, dns=256, ids=256, w=256, out=256, m=4, hidden=256, inter=128, E=8, k=2,
                ws=256, nbytes=cap, stream=None)                       # (nvl_moe_experts_mxfp4's arguments, in order)
    for kw, msg in ((dict(dns=None), b"null pointer"), (dict(k=9), b"top_k <= E"), (dict(hidden=192), b"hidden=192"),
                    (dict(inter=64), b"inter=64"), (dict(m=5), b"above the cap"), (dict(gu=264), b"aligned")):
        assert lib.nvl_moe_experts_mxfp4(*{**good, **kw}.values()) == -1 and msg in lib.nvl_last_error(), kw
