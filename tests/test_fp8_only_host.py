"""weight_dtype="fp8_only" without a GPU: what `Config` accepts and refuses, and nvl_linear_tile_fp8's host-side validation."""
import json

import pytest

from test_moe_host import moe_dir  # noqa: F401  (fixture: a qwen3-moe-tiny directory)


def test_config_accepts_fp8_only_for_a_dense_model_on_one_gpu(moe_dir, tmp_path):  # noqa: F811
    from nano_vllm_amd.api import Config
    from nano_vllm_amd.weights import qwen3_config_dict
    (tmp_path / "dense").mkdir()
    (tmp_path / "dense" / "config.json").write_text(json.dumps(qwen3_config_dict("qwen3-tiny", vocab_size=512)))
    dense = str(tmp_path / "dense")
    assert Config(dense, weight_dtype="fp8_only").weight_dtype == "fp8_only"
    with pytest.raises(ValueError, match="fp8_only"):
        Config(dense, weight_dtype="fp8_only", tensor_parallel_size=2)
    with pytest.raises(ValueError, match="expert weights stay bf16"):
        Config(moe_dir(), weight_dtype="fp8_only")


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), -1, b"null pointer"), (dict(scales=None), -1, b"null pointer"), (dict(k=192), -1, b"k=192"),
    (dict(n=24), -1, b"n=24"), (dict(n=48, mode=1), -1, b"n=48"), (dict(mode=2), -3, b"mode 2"), (dict(mode=5), -1, b"mode=5"),
    (dict(m=0), -1, b"m=0"), (dict(out=264), -1, b"aligned")])
def test_linear_tile_fp8_validates_on_the_host(kw, rc, msg):
    from nano_vllm_amd import ops
    lib = ops.load_library()
    good = dict(x=256, w8=256, scales=256, out=256, m=600, n=4096, k=1024, mode=0, stream=None)
    assert lib.nvl_linear_tile_fp8(*{**good, **kw}.values()) == rc and msg in lib.nvl_last_error(), kw
