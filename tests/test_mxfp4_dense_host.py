"""weight_dtype="mxfp4_dense" without a GPU: what `Config` accepts, nvl_linear_wide_mxfp4's plan over the Qwen3-8B / 32B
decode projections, and host-side argument validation of the three entry points."""
import ctypes
import json

import pytest

from test_moe_host import moe_dir  # noqa: F401  (fixture: a qwen3-moe-tiny directory)

BF16, SILU, PARTIAL = 0, 1, 2
# (n, k, mode) of q|k|v, o, gate|up, down as the decode step calls them: Qwen3-8B, then Qwen3-32B
PROJECTIONS = [(6144, 4096, BF16), (6144, 4096, PARTIAL), (4096, 4096, PARTIAL), (24576, 4096, SILU), (4096, 12288, PARTIAL),
               (10240, 5120, BF16), (10240, 5120, PARTIAL), (5120, 8192, PARTIAL), (51200, 5120, SILU), (5120, 25600, PARTIAL)]


@pytest.fixture(scope="module")
def lib():
    from nano_vllm_amd import ops
    return ops.load_library()


def _plan(lib, m, n, k, mode):
    splits, ws = ctypes.c_int(0), ctypes.c_size_t(0)
    ok = lib.nvl_linear_wide_mxfp4_plan(m, n, k, mode, ctypes.byref(splits), ctypes.byref(ws))
    return (splits.value, ws.value) if ok else None


def test_config_accepts_mxfp4_dense_on_one_gpu_for_a_dense_directory(moe_dir, tmp_path):  # noqa: F811
    from nano_vllm_amd.api import Config
    from nano_vllm_amd.weights import qwen3_config_dict
    (tmp_path / "config.json").write_text(json.dumps(qwen3_config_dict("qwen3-tiny", vocab_size=512)))
    assert Config(str(tmp_path), weight_dtype="mxfp4_dense").weight_dtype == "mxfp4_dense"
    with pytest.raises(ValueError, match="mxfp4_dense"):
        Config(str(tmp_path), weight_dtype="mxfp4_dense", tensor_parallel_size=2)
    with pytest.raises(ValueError, match="mxfp4_dense"):
        Config(moe_dir(), weight_dtype="mxfp4_dense")


@pytest.mark.parametrize("m", [1, 16, 17, 144, 145, 256])
def test_plan_covers_the_decode_projections(lib, m):
    for n, k, mode in PROJECTIONS:
        plan = _plan(lib, m, n, k, mode)
        assert plan is not None, (m, n, k, mode)
        splits, ws = plan
        assert splits >= 1 and (k // 128) % splits == 0 and (mode != PARTIAL or splits <= 8)
        assert ws == (splits * m * n * 4 if mode != PARTIAL and splits > 1 else 0)


def test_plan_refuses_what_the_kernel_does_not_take(lib):
    assert _plan(lib, 16, 4096, 1000, BF16) is None and _plan(lib, 257, 4096, 4096, BF16) is None
    assert _plan(lib, 16, 4104, 4096, BF16) is None and _plan(lib, 16, 4112, 4096, SILU) is None
    assert _plan(lib, 16, 4096, 4096, 3) is None


def test_host_side_argument_validation_without_gpu(lib):
    """Every call below is refused before any launch (the pointers are fake)."""
    good = dict(x=256, codes=256, scales=256, out=256, m=16, n=4096, k=4096, mode=PARTIAL, ws=None, nbytes=0, stream=None)
    assert _plan(lib, 16, 1280, 5120, BF16)[0] > 1            # a split shape: its bf16 call needs a workspace
    for kw, rc, msg in ((dict(codes=None), -1, b"null pointer"), (dict(mode=3), -1, b"mode=3"), (dict(x=264), -1, b"aligned"),
                        (dict(k=1000), -3, b"not covered"), (dict(m=257), -3, b"not covered"),
                        (dict(mode=BF16, n=1280, k=5120), -1, b"workspace")):
        assert lib.nvl_linear_wide_mxfp4(*{**good, **kw}.values()) == rc and msg in lib.nvl_last_error(), kw
    for args, msg in (((None, 256, 256, 32, 256, None), b"null pointer"), ((256, 256, 256, 24, 256, None), b"n=24"),
                      ((256, 256, 256, 32, 192, None), b"k=192"), ((256, 264, 256, 32, 256, None), b"aligned")):
        assert lib.nvl_unpack_mxfp4(*args) == -1 and msg in lib.nvl_last_error(), args
