"""weight_dtype="fp8" on the host: plan coverage, argument validation and the Config switch (no GPU)."""
import ctypes

import pytest

MODES = (0, 1, 2)       # ops.LINEAR_BF16 / LINEAR_SILU / LINEAR_PARTIAL


def _lib():
    from nano_vllm_amd import ops
    return ops.load_library()


def _plan(lib, m, n, k, mode):
    sp, ws = ctypes.c_int(0), ctypes.c_size_t(0)
    ok = lib.nvl_linear_wide_fp8_plan(m, n, k, mode, ctypes.byref(sp), ctypes.byref(ws))
    return ok, sp.value, ws.value


@pytest.mark.parametrize("hidden,inter,heads,kv", [(4096, 12288, 32, 8), (5120, 17408, 40, 8), (5120, 25600, 64, 8)])
def test_fp8_plan_covers_the_model_shapes(hidden, inter, heads, kv):
    """Every decode projection of Qwen3-8B / 14B / 32B, full width and per rank, in every mode: covered, the K split
    divides the 128-column k steps (at most 8 slabs for the slab consumers) and the scratch follows from it."""
    lib = _lib()
    for tp in (1, 2, 4, 8):
        shapes = [((heads + 2 * kv) * 128 // tp, hidden), (hidden, heads * 128 // tp), (2 * inter // tp, hidden),
                  (hidden, inter // tp)]
        for (n, k) in shapes:
            for mode in MODES:
                for m in (1, 16, 17, 144, 145, 256):
                    ok, sp, ws = _plan(lib, m, n, k, mode)
                    assert ok == 1 and 1 <= sp <= (8 if mode == 2 else 16) and (k // 128) % sp == 0, (m, n, k, mode, sp)
                    assert ws == (sp * m * n * 4 if mode != 2 and sp > 1 else 0), (m, n, k, mode, sp, ws)


def test_fp8_plan_refuses_uncovered_shapes():
    lib = _lib()
    for m, n, k, mode in ((144, 6144, 1000, 0), (144, 4100, 4096, 0), (257, 4096, 4096, 0), (0, 4096, 4096, 0),
                          (16, 4112, 4096, 1), (16, 4096, 4096, 3)):
        assert _plan(lib, m, n, k, mode)[0] == 0, (m, n, k, mode)


def test_fp8_entry_points_validate_on_the_host():
    lib = _lib()
    assert lib.nvl_linear_wide_fp8(None, 16, 16, 16, 144, 6144, 4096, 0, None, 0, None) == -1
    assert b"null pointer" in lib.nvl_last_error()
    assert lib.nvl_linear_wide_fp8(16, 16, None, 16, 144, 6144, 4096, 0, None, 0, None) == -1
    assert lib.nvl_linear_wide_fp8(16, 16, 16, 16, 144, 6144, 4096, 5, None, 0, None) == -1 and b"mode" in lib.nvl_last_error()
    assert lib.nvl_linear_wide_fp8(16, 16, 16, 16, 144, 6144, 1000, 0, None, 0, None) == -3
    assert b"not covered" in lib.nvl_last_error()
    assert lib.nvl_linear_wide_fp8(16, 16, 16, 16, 144, 1280, 5120, 0, None, 0, None) == -1 and b"workspace" in lib.nvl_last_error()
    assert lib.nvl_pack_weight_tiles_fp8(None, 16, 96, 256, None) == -1
    assert lib.nvl_pack_weight_tiles_fp8(16, 32, 24, 64, None) == -1 and b"multiple of 16" in lib.nvl_last_error()


def test_config_weight_dtype(tmp_path):
    from nano_vllm_amd.api import Config
    assert Config(str(tmp_path), hf_config=_Hf()).weight_dtype == "bf16"
    assert Config(str(tmp_path), hf_config=_Hf(), weight_dtype="fp8").weight_dtype == "fp8"
    with pytest.raises(AssertionError, match="weight_dtype"):
        Config(str(tmp_path), hf_config=_Hf(), weight_dtype="int4")


class _Hf:
    max_position_embeddings = 4096
