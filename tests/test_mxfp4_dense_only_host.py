"""weight_dtype="mxfp4_dense_only" without a GPU: what `Config` accepts and refuses, and nvl_linear_tile_mxfp4's host-side
validation."""
import json

import pytest

from test_moe_host import moe_dir  # noqa: F401  (fixture: a qwen3-moe-tiny directory)


def test_config_accepts_mxfp4_dense_only_for_a_dense_model_on_one_gpu(moe_dir, tmp_path):  # noqa: F811
    from nano_vllm_amd.api import Config
    from nano_vllm_amd.weights import qwen3_config_dict
    (tmp_path / "config.json").write_text(json.dumps(qwen3_config_dict("qwen3-tiny", vocab_size=512)))
    assert Config(str(tmp_path), weight_dtype="mxfp4_dense_only").weight_dtype == "mxfp4_dense_only"
    with pytest.raises(ValueError, match="mxfp4_dense_only"):
        Config(str(tmp_path), weight_dtype="mxfp4_dense_only", tensor_parallel_size=2)
    with pytest.raises(ValueError, match="mxfp4_dense_only"):
        Config(moe_dir(), weight_dtype="mxfp4_dense_only")


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(x=None), -1, b"null pointer"), (dict(scales=None), -1, b"null pointer"), (dict(out=264), -1, b"aligned"),
    (dict(mode=3), -1, b"mode=3"), (dict(mode=2), -3, b"not covered"), (dict(k=1000), -3, b"not covered"),
    (dict(n=24), -3, b"not covered")])
def test_linear_tile_mxfp4_validates_on_the_host(kw, rc, msg):
    from nano_vllm_amd import ops
    lib = ops.load_library()
    good = dict(x=256, codes=256, scales=256, out=256, m=600, n=4096, k=1024, mode=0, stream=None)
    assert lib.nvl_linear_tile_mxfp4(*{**good, **kw}.values()) == rc and msg in lib.nvl_last_error(), kw
