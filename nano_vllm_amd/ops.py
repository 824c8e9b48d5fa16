"""ctypes binding of libnvl_hip.so (C ABI in include/nvl.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every function below
hands raw device pointers + sizes to a hand-written gfx950 kernel. There is NO fallback:
if the library is missing or fails to load, importing callers get a loud RuntimeError.

`import torch` must precede loading the library so that it binds to the HIP runtime torch
already loaded (one runtime => shared streams, pointers and graph capture).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.environ.get("NVL_LIBDIR") or os.path.join(_HERE, "lib"), "libnvl_hip.so")   # (as build.LIBDIR)
ABI_VERSION = 6

# name -> (restype, argtypes); mirrors include/nvl.h one to one (checked by tests/test_abi.py)
SIGNATURES = {
    "nvl_abi_version": (c_int, []),
    "nvl_last_error": (c_char_p, []),
    "nvl_device_cu_count": (c_int, []),
    "nvl_rmsnorm": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_float, c_void_p]),
    "nvl_add_rmsnorm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "nvl_linear_decode_splits": (c_int, [c_int64, c_int, c_int, c_int]),
    "nvl_linear_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "nvl_linear_wide_plan": (c_int, [c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "nvl_linear_wide": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_size_t,
                                c_void_p]),
    "nvl_pack_weight_tiles": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "nvl_linear_wide_fp8_plan": (c_int, [c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "nvl_linear_wide_fp8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_size_t,
                                    c_void_p]),
    "nvl_pack_weight_tiles_fp8": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "nvl_linear_tile_fp8": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "nvl_add_rmsnorm_splitk": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "nvl_silu_mul": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p]),
    "nvl_moe_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int, c_int]),
    "nvl_moe_route": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p]),
    "nvl_moe_plan": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "nvl_moe_experts": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int,
                                c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "nvl_quant_pack_mxfp4": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "nvl_moe_experts_mxfp4": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int64, c_int, c_int, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "nvl_linear_wide_mxfp4_plan": (c_int, [c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "nvl_linear_wide_mxfp4": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_size_t,
                                      c_void_p]),
    "nvl_unpack_mxfp4": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "nvl_linear_tile_mxfp4": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "nvl_rope_neox": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "nvl_store_kvcache": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int64,
                                  c_int, c_void_p]),
    "nvl_qknorm_rope_kvstore": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int64,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int,
                                        c_int64, c_int, c_void_p]),
    "nvl_paged_attn_decode_workspace_bytes": (c_size_t, [c_int64, c_int, c_int64]),
    "nvl_paged_attn_decode": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                      c_int, c_int, c_int, c_int64, c_int64, c_float, c_void_p, c_size_t, c_int,
                                      c_void_p, c_void_p, c_void_p]),
    "nvl_decode_plan_bytes": (c_size_t, []),
    "nvl_decode_plan": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p]),
    "nvl_paged_attn_decode_fused": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_void_p,
                                            c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int,
                                            c_int, c_int64, c_int64, c_float, c_void_p, c_size_t, c_int, c_void_p,
                                            c_void_p, c_int, c_int64, c_void_p]),
    "nvl_attn_prefill_varlen": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int64, c_float,
                                        c_int, c_void_p, c_void_p]),
    "nvl_sample_workspace_bytes": (c_size_t, [c_int64]),
    "nvl_sample": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_uint64, c_uint64, c_void_p,
                           c_void_p, c_void_p, c_size_t, c_void_p]),
    "nvl_sample_shard": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_uint64, c_uint64,
                                 c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "nvl_sample_merge": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p]),
    "nvl_sample_topk_topp": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                     c_int64, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p]),
    "nvl_feed_tokens": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "nvl_store_tokens": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "nvl_feed_store_tokens": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "nvl_apply_penalties": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int64, c_void_p]),
    "nvl_allreduce_create": (c_int, [c_int, c_int, c_int64, ctypes.POINTER(c_void_p)]),
    "nvl_allreduce_uid": (c_int, [c_void_p, c_void_p]),
    "nvl_allreduce_connect": (c_int, [c_void_p, c_void_p]),
    "nvl_allreduce_max_bytes": (c_int64, [c_void_p]),
    "nvl_allreduce_buffer": (c_void_p, [c_void_p]),
    "nvl_allreduce_set_fences": (c_int, [c_void_p, c_int]),
    "nvl_allreduce_run": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "nvl_allreduce_add_rmsnorm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float,
                                          c_void_p]),
    "nvl_allreduce_gather": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "nvl_allreduce_status": (c_int, [c_void_p]),
    "nvl_allreduce_status_async": (c_int, [c_void_p, c_void_p, c_void_p]),
    "nvl_allreduce_destroy": (c_int, [c_void_p]),
    "nvl_sample_exponentials_host": (None, [c_uint64, c_uint64, c_int64, c_int64, c_int64, c_void_p]),
}

_lib = None


class NvlError(RuntimeError):
    pass


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load libnvl_hip.so and bind every symbol of the ABI. Raises if anything is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise NvlError(
            f"{path} not found: build it with `python -m nano_vllm_amd.build` (hipcc, gfx950). "
            "There is no CPU/PyTorch fallback for the hot path.")
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError => ABI mismatch, fail loudly
        fn.restype = restype
        fn.argtypes = argtypes
    ver = lib.nvl_abi_version()
    if ver != ABI_VERSION:
        raise NvlError(f"libnvl_hip.so ABI version {ver} != binding version {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def lib() -> ctypes.CDLL:
    return _lib if _lib is not None else load_library()


def _check(rc: int) -> None:
    if rc != 0:
        raise NvlError(f"nvl error {rc}: {lib().nvl_last_error().decode()}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


KV_BF16, KV_FP8 = 0, 1


def kv_dtype_of(cache: torch.Tensor) -> int:
    """NVL_KV_* code of a cache tensor: bf16 (the reference's precision) or OCP fp8 e4m3 (opt-in extension)."""
    if cache.dtype == torch.bfloat16:
        return KV_BF16
    if cache.dtype == torch.float8_e4m3fn:
        return KV_FP8
    raise NvlError(f"unsupported KV-cache dtype {cache.dtype} (bfloat16 or float8_e4m3fn)")


def _dev(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise NvlError(f"{name} must be a device (HIP) tensor; the hot path has no CPU fallback")


# ---------------------------------------------------------------------------------------------
def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, out: torch.Tensor | None = None) -> torch.Tensor:
    """y = bf16(float(x) * rsqrt(mean x^2 + eps) * float(w)); x is [..., hidden] or a strided
    [N, H, 128] head view (stride(-1) == 1, stride(-2) == hidden when 3-D)."""
    _dev(x, "x")
    hidden = x.shape[-1]
    assert x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16 and x.stride(-1) == 1
    if x.dim() == 3:
        n_outer, n_inner = x.shape[0], x.shape[1]
        assert x.stride(1) == hidden
        xs = x.stride(0)
    else:
        assert x.dim() == 2
        n_outer, n_inner, xs = x.shape[0], 1, x.stride(0)
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    ys = out.stride(0)
    _check(lib().nvl_rmsnorm(x.data_ptr(), xs, weight.data_ptr(), out.data_ptr(), ys, n_outer, n_inner, hidden,
                             eps, _stream()))
    return out


def add_rmsnorm(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """residual <- bf16(x + residual) in place; returns y = norm(un-rounded sum) * w."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and residual.is_contiguous() and x.shape == residual.shape
    assert x.dtype == torch.bfloat16 and residual.dtype == torch.bfloat16
    if out is None:
        out = torch.empty_like(x)
    _check(lib().nvl_add_rmsnorm(x.data_ptr(), residual.data_ptr(), weight.data_ptr(), out.data_ptr(), x.shape[0],
                                 x.shape[1], eps, _stream()))
    return out


def silu_mul(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    _dev(x, "x")
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.bfloat16
    inter = x.shape[1] // 2
    if out is None:
        out = torch.empty((x.shape[0], inter), dtype=x.dtype, device=x.device)
    _check(lib().nvl_silu_mul(x.data_ptr(), x.stride(0), out.data_ptr(), x.shape[0], inter, _stream()))
    return out


# ---- skinny (decode) linears ------------------------------------------------------------------
LINEAR_BF16, LINEAR_SILU, LINEAR_PARTIAL = 0, 1, 2
_splits_cache: dict[tuple, int] = {}


def linear_decode_splits(m: int, n: int, k: int, mode: int) -> int:
    """K-slices nvl_linear_decode emits for this shape (1 for modes 0/1); 0 = shape not covered."""
    key = (m, n, k, mode)
    r = _splits_cache.get(key)
    if r is None:
        r = _splits_cache[key] = lib().nvl_linear_decode_splits(m, n, k, mode)
    return r


def linear_decode(x: torch.Tensor, weight: torch.Tensor, mode: int = LINEAR_BF16,
                  out: torch.Tensor | None = None, packed: bool = False) -> torch.Tensor:
    """x [M, K] bf16, weight [N, K] bf16 (torch Linear layout; `packed`: its pack_weight_tiles() copy). mode 0: bf16
    [M, N]; mode 1: bf16 [M, N/2] = silu(x.Wgate) * (x.Wup); mode 2: fp32 split-K partials [S, M, N]."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and weight.is_contiguous()
    assert x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
    m, k = x.shape
    n = weight.shape[0]
    assert weight.shape[1] == k
    splits = linear_decode_splits(m, n, k, mode)
    if splits == 0:
        raise NvlError(f"nvl_linear_decode does not cover m={m} n={n} k={k} mode={mode}")
    if out is None:
        if mode == LINEAR_PARTIAL:
            out = torch.empty((splits, m, n), dtype=torch.float32, device=x.device)
        else:
            out = torch.empty((m, n // 2 if mode == LINEAR_SILU else n), dtype=torch.bfloat16, device=x.device)
    _check(lib().nvl_linear_decode(x.data_ptr(), weight.data_ptr(), out.data_ptr(), m, n, k, mode, 1 if packed else 0,
                                   _stream()))
    return out


_wide_cache: dict = {}


def linear_wide_plan(m: int, n: int, k: int, mode: int) -> tuple[int, int] | None:
    """(K splits, workspace bytes) of nvl_linear_wide's plan for this shape, or None when it is not covered."""
    key = (m, n, k, mode)
    if key not in _wide_cache:
        splits, ws = ctypes.c_int(0), ctypes.c_size_t(0)
        ok = lib().nvl_linear_wide_plan(m, n, k, mode, ctypes.byref(splits), ctypes.byref(ws))
        _wide_cache[key] = (splits.value, ws.value) if ok else None
    return _wide_cache[key]


def pack_weight_tiles(weight: torch.Tensor) -> torch.Tensor:
    """Tile-packed copy of a row-major [N, K] bf16 weight (nvl_pack_weight_tiles): same shape and bytes, stored as
    [N/16][K/32][64 lanes][8] so that every wave load of nvl_linear_wide's weight stream is one contiguous KiB."""
    _dev(weight, "weight")
    assert weight.dim() == 2 and weight.is_contiguous() and weight.dtype == torch.bfloat16
    n, k = weight.shape
    packed = torch.empty_like(weight)
    _check(lib().nvl_pack_weight_tiles(weight.data_ptr(), packed.data_ptr(), n, k, _stream()))
    return packed


def linear_wide(x: torch.Tensor, weight: torch.Tensor, mode: int = LINEAR_BF16, out: torch.Tensor | None = None,
                workspace: torch.Tensor | None = None, packed: bool = False) -> torch.Tensor:
    """Deep-K decode linear (same modes as linear_decode). `workspace`: uint8 scratch of the plan's size for
    modes 0 / 1 when the plan splits K (allocated here when omitted). `packed`: `weight` is the pack_weight_tiles()
    copy of the [N, K] parameter (same shape)."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and weight.is_contiguous()
    assert x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
    m, k = x.shape
    n = weight.shape[0]
    assert weight.shape[1] == k
    plan = linear_wide_plan(m, n, k, mode)
    if plan is None:
        raise NvlError(f"nvl_linear_wide does not cover m={m} n={n} k={k} mode={mode}")
    splits, ws_bytes = plan
    if out is None:
        if mode == LINEAR_PARTIAL:
            out = torch.empty((splits, m, n), dtype=torch.float32, device=x.device)
        else:
            out = torch.empty((m, n // 2 if mode == LINEAR_SILU else n), dtype=torch.bfloat16, device=x.device)
    if ws_bytes and workspace is None:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    assert not ws_bytes or workspace.numel() * workspace.element_size() >= ws_bytes
    _check(lib().nvl_linear_wide(x.data_ptr(), weight.data_ptr(), out.data_ptr(), m, n, k, mode, 1 if packed else 0,
                                 workspace.data_ptr() if ws_bytes else None, ws_bytes, _stream()))
    return out


# ---- weight-only FP8 (W8A16) wide linears: e4m3 weights, fp32 scale per (16-row tile, 128-column k block) ---------
_wide_fp8_cache: dict = {}


def linear_wide_fp8_plan(m: int, n: int, k: int, mode: int) -> tuple[int, int] | None:
    """(K splits, workspace bytes) of nvl_linear_wide_fp8's plan for this shape, or None when it is not covered."""
    key = (m, n, k, mode)
    if key not in _wide_fp8_cache:
        splits, ws = ctypes.c_int(0), ctypes.c_size_t(0)
        ok = lib().nvl_linear_wide_fp8_plan(m, n, k, mode, ctypes.byref(splits), ctypes.byref(ws))
        _wide_fp8_cache[key] = (splits.value, ws.value) if ok else None
    return _wide_fp8_cache[key]


def pack_weight_tiles_fp8(w8: torch.Tensor) -> torch.Tensor:
    """Tile-packed copy of a row-major [N, K] float8_e4m3fn weight (nvl_pack_weight_tiles_fp8): same shape and bytes,
    stored as [N/16][K/64][64 lanes][16 bytes] — a wave load of nvl_linear_wide_fp8's weight stream is one contiguous KiB."""
    _dev(w8, "w8")
    assert w8.dim() == 2 and w8.is_contiguous() and w8.dtype == torch.float8_e4m3fn
    n, k = w8.shape
    packed = torch.empty_like(w8)
    _check(lib().nvl_pack_weight_tiles_fp8(w8.data_ptr(), packed.data_ptr(), n, k, _stream()))
    return packed


def linear_wide_fp8(x: torch.Tensor, w8_packed: torch.Tensor, scales: torch.Tensor, mode: int = LINEAR_BF16,
                    out: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """x [M, K] bf16 . (w8 o scales)^T: `w8_packed` the pack_weight_tiles_fp8() copy of the [N, K] e4m3 weight, `scales`
    fp32 [N/16, K/128]. Modes, outputs and `workspace` as linear_wide."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and w8_packed.is_contiguous() and scales.is_contiguous()
    assert x.dtype == torch.bfloat16 and w8_packed.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32
    m, k = x.shape
    n = w8_packed.shape[0]
    assert w8_packed.shape[1] == k and scales.shape == (n // 16, k // 128)
    plan = linear_wide_fp8_plan(m, n, k, mode)
    if plan is None:
        raise NvlError(f"nvl_linear_wide_fp8 does not cover m={m} n={n} k={k} mode={mode}")
    splits, ws_bytes = plan
    if out is None:
        if mode == LINEAR_PARTIAL:
            out = torch.empty((splits, m, n), dtype=torch.float32, device=x.device)
        else:
            out = torch.empty((m, n // 2 if mode == LINEAR_SILU else n), dtype=torch.bfloat16, device=x.device)
    if ws_bytes and workspace is None:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    assert not ws_bytes or workspace.numel() * workspace.element_size() >= ws_bytes
    _check(lib().nvl_linear_wide_fp8(x.data_ptr(), w8_packed.data_ptr(), scales.data_ptr(), out.data_ptr(), m, n, k, mode,
                                     workspace.data_ptr() if ws_bytes else None, ws_bytes, _stream()))
    return out


def linear_tile_fp8(x: torch.Tensor, w8_packed: torch.Tensor, scales: torch.Tensor, mode: int = LINEAR_BF16,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """x [M, K] bf16 . (w8 o scales)^T for ANY M (nvl_linear_tile_fp8): operands as linear_wide_fp8, scales powers of two
    (include/nvl.h). mode LINEAR_BF16 -> bf16 [M, N], LINEAR_SILU -> bf16 [M, N/2]; LINEAR_PARTIAL is not offered. `out`
    may have more than M rows: the rows past M are left untouched."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and w8_packed.is_contiguous() and scales.is_contiguous()
    assert x.dtype == torch.bfloat16 and w8_packed.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32
    m, k = x.shape
    n = w8_packed.shape[0]
    assert w8_packed.shape[1] == k and scales.shape == (n // 16, k // 128)
    cols = n // 2 if mode == LINEAR_SILU else n
    if out is None:
        out = torch.empty((m, cols), dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape[0] >= m and out.shape[1] == cols
    _check(lib().nvl_linear_tile_fp8(x.data_ptr(), w8_packed.data_ptr(), scales.data_ptr(), out.data_ptr(), m, n, k, mode,
                                     _stream()))
    return out


def add_rmsnorm_splitk(partials: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float,
                       out: torch.Tensor | None = None) -> torch.Tensor:
    """partials fp32 [S, M, H]; residual <- bf16(bf16(sum_s partials) + residual) in place; returns the norm."""
    _dev(partials, "partials")
    assert partials.dim() == 3 and partials.is_contiguous() and partials.dtype == torch.float32
    s, m, h = partials.shape
    assert residual.shape == (m, h) and residual.is_contiguous() and residual.dtype == torch.bfloat16
    if out is None:
        out = torch.empty_like(residual)
    _check(lib().nvl_add_rmsnorm_splitk(partials.data_ptr(), s, residual.data_ptr(), weight.data_ptr(), out.data_ptr(),
                                        m, h, eps, _stream()))
    return out



# ---- sparse mixture-of-experts block (Qwen3-MoE): route -> plan -> experts -------------------------------------------
def moe_workspace_bytes(max_tokens: int, hidden: int, inter: int, num_experts: int, top_k: int) -> int:
    """Bytes of the workspace that serves calls of up to `max_tokens` rows (host code; raises on an unsupported shape)."""
    n = lib().nvl_moe_workspace_bytes(max_tokens, hidden, inter, num_experts, top_k)
    if n == 0:
        raise NvlError(f"nvl_moe: unsupported shape max_tokens={max_tokens} hidden={hidden} inter={inter} "
                       f"E={num_experts} top_k={top_k} (hidden, inter % 128 == 0; E <= 256; top_k <= 8, <= E)")
    return n


def moe_route(x: torch.Tensor, router_w: torch.Tensor, top_k: int, norm_topk_prob: bool,
              ids: torch.Tensor | None = None, weights: torch.Tensor | None = None):
    """x [M, H] bf16, router_w [E, H] bf16 -> (ids int32 [M, top_k], weights fp32 [M, top_k]): top_k of the fp32 softmax
    over all E experts, descending, ties to the lower index; weights renormalised over the selection if `norm_topk_prob`."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and router_w.is_contiguous()
    assert x.dtype == torch.bfloat16 and router_w.dtype == torch.bfloat16 and router_w.shape[1] == x.shape[1]
    m, hidden = x.shape
    if ids is None:
        ids = torch.empty((m, top_k), dtype=torch.int32, device=x.device)
    if weights is None:
        weights = torch.empty((m, top_k), dtype=torch.float32, device=x.device)
    assert ids.dtype == torch.int32 and weights.dtype == torch.float32 and ids.numel() == m * top_k == weights.numel()
    _check(lib().nvl_moe_route(x.data_ptr(), router_w.data_ptr(), ids.data_ptr(), weights.data_ptr(), m, hidden,
                               router_w.shape[0], top_k, 1 if norm_topk_prob else 0, _stream()))
    return ids, weights


def moe_plan(ids: torch.Tensor, num_experts: int, workspace: torch.Tensor) -> None:
    """Sort the (token, slot) pairs of `ids` (int32 [M, top_k]) by expert into `workspace` (uint8, moe_workspace_bytes)."""
    _dev(ids, "ids")
    assert ids.dim() == 2 and ids.is_contiguous() and ids.dtype == torch.int32 and workspace.dtype == torch.uint8
    _check(lib().nvl_moe_plan(ids.data_ptr(), ids.shape[0], num_experts, ids.shape[1], workspace.data_ptr(),
                              workspace.numel(), _stream()))


def moe_experts(x: torch.Tensor, w_gate_up: torch.Tensor, w_down: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor,
                workspace: torch.Tensor, out: torch.Tensor | None = None, packed: bool = False) -> torch.Tensor:
    """out[t] = bf16(sum_j weights[t, j] * down_e(silu(gate_e(x[t])) * up_e(x[t]))), e = ids[t, j], for the plan that
    `moe_plan(ids, ...)` left in `workspace`. w_gate_up [E, 2 * inter, H], w_down [E, H, inter] bf16 (`packed`: their
    pack_weight_tiles() copies, made over the stacked [E * n, k] matrices)."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and w_gate_up.is_contiguous() and w_down.is_contiguous()
    assert x.dtype == torch.bfloat16 and w_gate_up.dtype == torch.bfloat16 and w_down.dtype == torch.bfloat16
    m, hidden = x.shape
    e, hid2, inter = w_down.shape
    assert hid2 == hidden and tuple(w_gate_up.shape) == (e, 2 * inter, hidden)
    assert ids.dtype == torch.int32 and weights.dtype == torch.float32 and ids.is_contiguous() and weights.is_contiguous()
    assert ids.shape[0] == m and ids.shape == weights.shape and workspace.dtype == torch.uint8
    if out is None:
        out = torch.empty_like(x)
    _check(lib().nvl_moe_experts(x.data_ptr(), w_gate_up.data_ptr(), w_down.data_ptr(), ids.data_ptr(),
                                 weights.data_ptr(), out.data_ptr(), m, hidden, inter, e, ids.shape[1],
                                 1 if packed else 0, workspace.data_ptr(), workspace.numel(), _stream()))
    return out


def quant_pack_mxfp4(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Row-major bf16 [N, K] -> (codes uint8 [N/16, K/128, 64, 16], scales uint8 [N, K/32]): OCP MXFP4 (e2m1 elements,
    one e8m0 scale per row and 32 k), codes in the A-fragment tile order of nvl_moe_experts_mxfp4 (include/nvl.h)."""
    _dev(w, "w")
    assert w.dim() == 2 and w.is_contiguous() and w.dtype == torch.bfloat16
    n, k = w.shape
    if n % 16 or k % 128:
        raise NvlError(f"nvl_quant_pack_mxfp4: n={n} must be a multiple of 16 and k={k} a multiple of 128")
    codes = torch.empty((n // 16, k // 128, 64, 16), dtype=torch.uint8, device=w.device)
    scales = torch.empty((n, k // 32), dtype=torch.uint8, device=w.device)
    _check(lib().nvl_quant_pack_mxfp4(w.data_ptr(), n, k, codes.data_ptr(), scales.data_ptr(), _stream()))
    return codes, scales


def moe_experts_mxfp4(x: torch.Tensor, gu: torch.Tensor, gu_scales: torch.Tensor, dn: torch.Tensor, dn_scales: torch.Tensor,
                      ids: torch.Tensor, weights: torch.Tensor, workspace: torch.Tensor,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """moe_experts over MXFP4 experts: (`gu`, `gu_scales`) = quant_pack_mxfp4 of the stacked gate|up [E * 2 * inter, H],
    (`dn`, `dn_scales`) of the stacked down [E * H, inter]. E and inter follow from the scale shapes."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.bfloat16
    for t in (gu, gu_scales, dn, dn_scales):
        assert t.is_contiguous() and t.dtype == torch.uint8
    m, hidden = x.shape
    inter = dn_scales.shape[1] * 32
    e = dn_scales.shape[0] // hidden
    assert tuple(dn_scales.shape) == (e * hidden, inter // 32) and tuple(gu_scales.shape) == (e * 2 * inter, hidden // 32)
    assert gu.numel() == e * inter * hidden and dn.numel() * 2 == e * inter * hidden
    assert ids.dtype == torch.int32 and weights.dtype == torch.float32 and ids.is_contiguous() and weights.is_contiguous()
    assert ids.shape[0] == m and ids.shape == weights.shape and workspace.dtype == torch.uint8
    if out is None:
        out = torch.empty_like(x)
    _check(lib().nvl_moe_experts_mxfp4(x.data_ptr(), gu.data_ptr(), gu_scales.data_ptr(), dn.data_ptr(), dn_scales.data_ptr(),
                                       ids.data_ptr(), weights.data_ptr(), out.data_ptr(), m, hidden, inter, e, ids.shape[1],
                                       workspace.data_ptr(), workspace.numel(), _stream()))
    return out


# ---- weight-only MXFP4 (W4A16) wide linears for the dense projections: quant_pack_mxfp4's codes, tile-major scales -------
_wide_mxfp4_cache: dict = {}


def linear_wide_mxfp4_plan(m: int, n: int, k: int, mode: int) -> tuple[int, int] | None:
    """(K splits, workspace bytes) of nvl_linear_wide_mxfp4's plan for this shape, or None when it is not covered."""
    key = (m, n, k, mode)
    if key not in _wide_mxfp4_cache:
        splits, ws = ctypes.c_int(0), ctypes.c_size_t(0)
        ok = lib().nvl_linear_wide_mxfp4_plan(m, n, k, mode, ctypes.byref(splits), ctypes.byref(ws))
        _wide_mxfp4_cache[key] = (splits.value, ws.value) if ok else None
    return _wide_mxfp4_cache[key]


def tile_scales_mxfp4(scales: torch.Tensor) -> torch.Tensor:
    """quant_pack_mxfp4's row-major scale bytes [N, K/32] -> the tile-major [N/16, K/128, 16, 4] nvl_linear_wide_mxfp4
    reads (a tile step's scales are one 64-byte line). Done once at load."""
    n, kb = scales.shape
    assert scales.dtype == torch.uint8 and n % 16 == 0 and kb % 4 == 0
    return scales.view(n // 16, 16, kb // 4, 4).permute(0, 2, 1, 3).contiguous()


def unpack_mxfp4(codes: torch.Tensor, scales: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Inverse of quant_pack_mxfp4 (its codes and ROW-MAJOR scales [N, K/32]): the dequantised bf16 [N, K] matrix
    (nvl_unpack_mxfp4), written into `out` when given."""
    _dev(codes, "codes")
    assert codes.is_contiguous() and scales.is_contiguous() and codes.dtype == torch.uint8 and scales.dtype == torch.uint8
    n, k = scales.shape[0], scales.shape[1] * 32
    assert scales.dim() == 2 and codes.numel() * 2 == n * k
    if out is None:
        out = torch.empty((n, k), dtype=torch.bfloat16, device=codes.device)
    assert out.shape == (n, k) and out.dtype == torch.bfloat16 and out.is_contiguous()
    _check(lib().nvl_unpack_mxfp4(codes.data_ptr(), scales.data_ptr(), out.data_ptr(), n, k, _stream()))
    return out


def linear_wide_mxfp4(x: torch.Tensor, codes: torch.Tensor, scales_tiled: torch.Tensor, mode: int = LINEAR_BF16,
                      out: torch.Tensor | None = None, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """x [M, K] bf16 . W_deq^T over MXFP4 weights: `codes` from quant_pack_mxfp4 ([N/16, K/128, 64, 16]), `scales_tiled`
    from tile_scales_mxfp4 ([N/16, K/128, 16, 4]). Modes, outputs and `workspace` as linear_wide."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and codes.is_contiguous() and scales_tiled.is_contiguous()
    assert x.dtype == torch.bfloat16 and codes.dtype == torch.uint8 and scales_tiled.dtype == torch.uint8
    m, k = x.shape
    n = codes.shape[0] * 16
    assert tuple(codes.shape) == (n // 16, k // 128, 64, 16) and tuple(scales_tiled.shape) == (n // 16, k // 128, 16, 4)
    plan = linear_wide_mxfp4_plan(m, n, k, mode)
    if plan is None:
        raise NvlError(f"nvl_linear_wide_mxfp4 does not cover m={m} n={n} k={k} mode={mode}")
    splits, ws_bytes = plan
    if out is None:
        if mode == LINEAR_PARTIAL:
            out = torch.empty((splits, m, n), dtype=torch.float32, device=x.device)
        else:
            out = torch.empty((m, n // 2 if mode == LINEAR_SILU else n), dtype=torch.bfloat16, device=x.device)
    if ws_bytes and workspace is None:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    assert not ws_bytes or workspace.numel() * workspace.element_size() >= ws_bytes
    _check(lib().nvl_linear_wide_mxfp4(x.data_ptr(), codes.data_ptr(), scales_tiled.data_ptr(), out.data_ptr(), m, n, k, mode,
                                       workspace.data_ptr() if ws_bytes else None, ws_bytes, _stream()))
    return out


def linear_tile_mxfp4(x: torch.Tensor, codes: torch.Tensor, scales_tiled: torch.Tensor, mode: int = LINEAR_BF16,
                      out: torch.Tensor | None = None) -> torch.Tensor:
    """x [M, K] bf16 . W_deq^T over MXFP4 weights for ANY M (nvl_linear_tile_mxfp4): operands as linear_wide_mxfp4. mode
    LINEAR_BF16 -> bf16 [M, N], LINEAR_SILU -> bf16 [M, N/2]; LINEAR_PARTIAL is not offered. `out` may have more than M
    rows: the rows past M are left untouched."""
    _dev(x, "x")
    assert x.dim() == 2 and x.is_contiguous() and codes.is_contiguous() and scales_tiled.is_contiguous()
    assert x.dtype == torch.bfloat16 and codes.dtype == torch.uint8 and scales_tiled.dtype == torch.uint8
    m, k = x.shape
    n = codes.shape[0] * 16
    assert tuple(codes.shape) == (n // 16, k // 128, 64, 16) and tuple(scales_tiled.shape) == (n // 16, k // 128, 16, 4)
    cols = n // 2 if mode == LINEAR_SILU else n
    if out is None:
        out = torch.empty((m, cols), dtype=torch.bfloat16, device=x.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape[0] >= m and out.shape[1] == cols
    _check(lib().nvl_linear_tile_mxfp4(x.data_ptr(), codes.data_ptr(), scales_tiled.data_ptr(), out.data_ptr(), m, n, k, mode,
                                       _stream()))
    return out


def rope_neox(positions: torch.Tensor, cos_sin: torch.Tensor, x: torch.Tensor,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """x: [N, H, 128] (stride(1) == 128); cos_sin: fp32 [max_pos, 128]."""
    _dev(x, "x")
    assert x.dim() == 3 and x.shape[2] == 128 and x.stride(2) == 1 and x.stride(1) == 128
    assert positions.dtype == torch.int64 and cos_sin.dtype == torch.float32 and cos_sin.is_contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _check(lib().nvl_rope_neox(positions.data_ptr(), cos_sin.data_ptr(), cos_sin.shape[0], x.data_ptr(), x.stride(0),
                               out.data_ptr(), out.stride(0), x.shape[0], x.shape[1], _stream()))
    return out


def store_kvcache(k: torch.Tensor, v: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor,
                  slot_mapping: torch.Tensor) -> None:
    """k, v: [N, Hkv, 128] (stride(1) == 128); caches: [num_blocks, Hkv, block_size, 128]."""
    _dev(k, "k")
    n, hkv, d = k.shape
    assert d == 128 and k.stride(1) == 128 and v.stride(1) == 128 and k.stride(2) == 1 and v.stride(2) == 1
    assert k_cache.is_contiguous() and v_cache.is_contiguous() and slot_mapping.dtype == torch.int32
    assert slot_mapping.numel() == n
    _check(lib().nvl_store_kvcache(k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), k_cache.data_ptr(),
                                   v_cache.data_ptr(), slot_mapping.data_ptr(), n, hkv, k_cache.shape[2],
                                   k_cache.shape[0], kv_dtype_of(k_cache), _stream()))


def qknorm_rope_kvstore(qkv: torch.Tensor, positions: torch.Tensor, q_norm_w, k_norm_w, eps: float,
                        cos_sin: torch.Tensor, slot_mapping, q_out: torch.Tensor, k_out, k_cache, v_cache,
                        num_q_heads: int, num_kv_heads: int) -> None:
    _dev(qkv, "qkv")
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.dtype == torch.bfloat16
    has_cache = k_cache is not None and k_cache.numel() > 0
    _check(lib().nvl_qknorm_rope_kvstore(
        qkv.data_ptr(), qkv.stride(0), positions.data_ptr(),
        q_norm_w.data_ptr() if q_norm_w is not None else None,
        k_norm_w.data_ptr() if k_norm_w is not None else None, eps,
        cos_sin.data_ptr(), cos_sin.shape[0],
        slot_mapping.data_ptr() if (has_cache and slot_mapping is not None) else None,
        q_out.data_ptr(), k_out.data_ptr() if k_out is not None else None,
        k_cache.data_ptr() if has_cache else None, v_cache.data_ptr() if has_cache else None,
        qkv.shape[0], num_q_heads, num_kv_heads,
        k_cache.shape[2] if has_cache else 0, k_cache.shape[0] if has_cache else 0,
        kv_dtype_of(k_cache) if has_cache else KV_BF16, _stream()))


def paged_attn_decode_workspace_bytes(max_batch: int, num_q_heads: int, max_context: int) -> int:
    return lib().nvl_paged_attn_decode_workspace_bytes(max_batch, num_q_heads, max_context)


def decode_plan_bytes() -> int:
    return lib().nvl_decode_plan_bytes()


def decode_plan(context_lens: torch.Tensor, num_q_heads: int, num_kv_heads: int, max_context: int,
                plan: torch.Tensor | None = None, shared_prefix: torch.Tensor | None = None,
                block_size: int = 256, prefix_groups: int = 1) -> torch.Tensor:
    """Per-step work plan of the decode attention launches (same for every layer of the step): `plan` is a uint8
    device buffer of decode_plan_bytes() bytes, allocated when None. `shared_prefix`: int32 device tensor [1 + batch] —
    [0] = number of leading KV blocks the member sequences have in common, [1 + b] != 0 marks sequence b as a member;
    the attention calls that consume this plan then run the shared-prefix pass, and read the member flags from this
    tensor's memory when they run (include/nvl.h). `prefix_groups` > 1: the flags are group ids (several shared prefixes in one
    step) and a pack of rows may hold up to that many different groups."""
    _dev(context_lens, "context_lens")
    assert context_lens.dtype == torch.int32 and context_lens.is_contiguous()
    if plan is None:
        plan = torch.empty(decode_plan_bytes(), dtype=torch.uint8, device=context_lens.device)
    shp = None
    if shared_prefix is not None:
        assert shared_prefix.dtype == torch.int32 and shared_prefix.device == context_lens.device
        assert shared_prefix.is_contiguous() and shared_prefix.numel() >= 1 + context_lens.numel()
        shp = shared_prefix.data_ptr()
    _check(lib().nvl_decode_plan(context_lens.data_ptr(), context_lens.numel(), num_q_heads, num_kv_heads, max_context,
                                 shp, block_size, prefix_groups, plan.data_ptr(), plan.numel(), _stream()))
    return plan


def decode_attention_shares_prefixes(num_q_heads: int, num_kv_heads: int, block_size: int) -> bool:
    """Can a decode plan carry a shared prefix for this geometry? (matrix-core kernel, 128-token-aligned blocks)"""
    return block_size % 128 == 0 and decode_attention_takes_qkv_slabs(num_q_heads, num_kv_heads)


def _lse_ptr(lse: torch.Tensor | None, shape: tuple) -> int | None:
    if lse is None:
        return None
    assert lse.dtype == torch.float32 and lse.is_contiguous() and tuple(lse.shape) == shape, (lse.shape, shape)
    return lse.data_ptr()


def paged_attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                      context_lens: torch.Tensor, scale: float, max_context: int, workspace: torch.Tensor,
                      out: torch.Tensor | None = None, plan: torch.Tensor | None = None,
                      lse: torch.Tensor | None = None) -> torch.Tensor:
    """q: [B, Hq, 128]; caches [num_blocks, Hkv, block_size, 128]; block_tables int32 [B, W]. `plan`: decode_plan()
    of this step; `lse`: optional fp32 [B, Hq] output (log-sum-exp of the scaled scores)."""
    _dev(q, "q")
    b, hq, d = q.shape
    assert d == 128 and q.is_contiguous() and block_tables.dtype == torch.int32 and context_lens.dtype == torch.int32
    assert block_tables.stride(1) == 1
    if out is None:
        out = torch.empty_like(q)
    _check(lib().nvl_paged_attn_decode(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), block_tables.data_ptr(),
                                       block_tables.stride(0), context_lens.data_ptr(), out.data_ptr(), b, hq,
                                       k_cache.shape[1], k_cache.shape[2], k_cache.shape[0], max_context, scale,
                                       workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                       kv_dtype_of(k_cache), plan.data_ptr() if plan is not None else None,
                                       _lse_ptr(lse, (b, hq)), _stream()))
    return out


def paged_attn_decode_fused(qkv: torch.Tensor, q_norm_w, k_norm_w, eps: float, cos_sin: torch.Tensor,
                            k_cache: torch.Tensor, v_cache: torch.Tensor, block_tables: torch.Tensor,
                            context_lens: torch.Tensor, num_q_heads: int, scale: float, max_context: int,
                            workspace: torch.Tensor, out: torch.Tensor | None = None,
                            plan: torch.Tensor | None = None, lse: torch.Tensor | None = None) -> torch.Tensor:
    """Decode step in one launch: q/k-norm + RoPE (position = context_len - 1) + KV-cache store of the
    new token + paged attention. qkv: raw qkv GEMM output [B, (Hq + 2*Hkv)*128] bf16 — or, for a deep-K projection,
    the fp32 split-K slabs [S, B, (Hq + 2*Hkv)*128] of `linear_wide(..., LINEAR_PARTIAL)` (S <= 8; summed and rounded
    in the attention prologue: no separate slab-reduce launch; matrix-core kernel only, Hq / Hkv in 2 ... 16)."""
    _dev(qkv, "qkv")
    splits, split_stride = 0, 0
    if qkv.dtype == torch.float32:
        assert qkv.dim() == 3 and qkv.is_contiguous() and 1 <= qkv.shape[0] <= 8
        splits, split_stride = qkv.shape[0], qkv.stride(0)
        b, row_stride = qkv.shape[1], qkv.stride(1)
    else:
        assert qkv.dim() == 2 and qkv.stride(1) == 1 and qkv.dtype == torch.bfloat16
        b, row_stride = qkv.shape[0], qkv.stride(0)
    assert block_tables.dtype == torch.int32 and context_lens.dtype == torch.int32 and block_tables.stride(1) == 1
    assert cos_sin.dtype == torch.float32 and cos_sin.is_contiguous()
    if out is None:
        out = torch.empty((b, num_q_heads, 128), dtype=torch.bfloat16, device=qkv.device)
    _check(lib().nvl_paged_attn_decode_fused(
        qkv.data_ptr(), row_stride, q_norm_w.data_ptr() if q_norm_w is not None else None,
        k_norm_w.data_ptr() if k_norm_w is not None else None, eps, cos_sin.data_ptr(), cos_sin.shape[0],
        k_cache.data_ptr(), v_cache.data_ptr(), block_tables.data_ptr(), block_tables.stride(0),
        context_lens.data_ptr(), out.data_ptr(), b, num_q_heads, k_cache.shape[1], k_cache.shape[2], k_cache.shape[0],
        max_context, scale, workspace.data_ptr(), workspace.numel() * workspace.element_size(), kv_dtype_of(k_cache),
        plan.data_ptr() if plan is not None else None, _lse_ptr(lse, (b, num_q_heads)), splits, split_stride, _stream()))
    return out


def decode_attention_takes_qkv_slabs(num_q_heads: int, num_kv_heads: int) -> bool:
    """Can `paged_attn_decode_fused` sum fp32 qkv slabs itself for this head geometry? (the matrix-core kernel: group
    sizes 2 ... 16 — 2, 4, 8 unless their packed-dot forms are forced by NVL_DECODE_MFMA=0 / NVL_DECODE_G8_VALU=1; every other
    group size, e.g. Qwen3-14B's 40 / 8 = 5, only has the matrix-core kernel)"""
    g = num_q_heads // max(num_kv_heads, 1)
    if g == 8:
        return os.environ.get("NVL_DECODE_G8_VALU", "0") != "1"
    if g in (2, 4):
        return os.environ.get("NVL_DECODE_MFMA", "1") != "0"
    return 1 < g <= 16


def attn_prefill_varlen(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor,
                        cu_seqlens_k: torch.Tensor, max_seqlen_q: int, scale: float,
                        block_tables: torch.Tensor | None = None, num_kv_heads: int | None = None,
                        out: torch.Tensor | None = None, lse: torch.Tensor | None = None) -> torch.Tensor:
    """q: [Nq, Hq, 128]. block_tables None: k, v packed [Nk, Hkv, 128] (token-strided views ok);
    otherwise k, v are the paged caches [num_blocks, Hkv, block_size, 128]. `lse`: optional fp32 [Nq, Hq] output."""
    _dev(q, "q")
    nq, hq, d = q.shape
    assert d == 128 and q.is_contiguous()
    assert cu_seqlens_q.dtype == torch.int32 and cu_seqlens_k.dtype == torch.int32
    if out is None:
        out = torch.empty_like(q)
    num_seqs = cu_seqlens_q.numel() - 1
    if block_tables is None:
        hkv = k.shape[1]
        assert k.stride(1) == 128 and v.stride(1) == 128 and k.stride(2) == 1 and v.stride(2) == 1
        _check(lib().nvl_attn_prefill_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), k.stride(0), v.stride(0),
                                             cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(), None, 0,
                                             out.data_ptr(), nq, num_seqs, max_seqlen_q, hq, hkv, 0, 0, scale,
                                             KV_BF16, _lse_ptr(lse, (nq, hq)), _stream()))
    else:
        assert block_tables.dtype == torch.int32 and block_tables.stride(1) == 1
        _check(lib().nvl_attn_prefill_varlen(q.data_ptr(), k.data_ptr(), v.data_ptr(), 0, 0,
                                             cu_seqlens_q.data_ptr(), cu_seqlens_k.data_ptr(),
                                             block_tables.data_ptr(), block_tables.stride(0), out.data_ptr(), nq,
                                             num_seqs, max_seqlen_q, hq, k.shape[1], k.shape[2], k.shape[0], scale,
                                             kv_dtype_of(k), _lse_ptr(lse, (nq, hq)), _stream()))
    return out


def sample_workspace_bytes(max_batch: int) -> int:
    return lib().nvl_sample_workspace_bytes(max_batch)


def _keys_ptr(row_keys: torch.Tensor | None, b: int) -> int | None:
    if row_keys is None:
        return None
    assert row_keys.dtype == torch.int64 and row_keys.is_contiguous() and row_keys.numel() >= b and row_keys.is_cuda
    return row_keys.data_ptr()


def sample(logits: torch.Tensor, temperatures: torch.Tensor, seed: int, offset: int, workspace: torch.Tensor,
           out: torch.Tensor | None = None, offset_dev: torch.Tensor | None = None,
           row_keys: torch.Tensor | None = None) -> torch.Tensor:
    """logits bf16 [B, V]; temperatures fp32 [B] (0 => argmax); returns int64 [B]. `row_keys` (int64 [B] holding
    sequence_id | position << 32): draws keyed by (sequence, position) instead of by batch row."""
    _dev(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.bfloat16
    assert temperatures.dtype == torch.float32
    b, vocab = logits.shape
    if out is None:
        out = torch.empty(b, dtype=torch.int64, device=logits.device)
    _check(lib().nvl_sample(logits.data_ptr(), logits.stride(0), temperatures.data_ptr(), out.data_ptr(), b, vocab,
                            seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF,
                            offset_dev.data_ptr() if offset_dev is not None else None, _keys_ptr(row_keys, b),
                            workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()))
    return out


def sample_topk_topp(logits: torch.Tensor, temperatures: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                     seed: int, offset: int, out: torch.Tensor | None = None, tau: torch.Tensor | None = None,
                     offset_dev: torch.Tensor | None = None, row_keys: torch.Tensor | None = None) -> torch.Tensor:
    """`sample` with a per-row top-k / top-p filter: top_k int32 [B] (<= 0 or >= V: off), top_p fp32 [B] (>= 1: off).
    A row keeps the columns l >= max(v_k, v_p) — v_k the k-th largest logit, v_p the largest value at which the mass of
    exp((l - max) / T) over the top-k survivors reaches top_p of their total; ties at the cut are kept — and draws the
    same race as `sample` over them: a row with both filters off (or T == 0) returns `sample`'s token bit for bit.
    `tau` (optional, fp32 [B]) receives the row's cut max(v_k, v_p), -inf for an unfiltered row."""
    _dev(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.bfloat16
    assert temperatures.dtype == torch.float32
    b, vocab = logits.shape
    for name, t, dt in (("top_k", top_k, torch.int32), ("top_p", top_p, torch.float32)):
        assert t.dtype == dt and t.dim() == 1 and t.is_contiguous() and t.numel() >= b and t.device == logits.device, \
            f"{name}: want a contiguous {dt} [B] tensor on the logits' device"
    if tau is not None:
        assert tau.dtype == torch.float32 and tau.is_contiguous() and tau.numel() >= b and tau.device == logits.device
    if out is None:
        out = torch.empty(b, dtype=torch.int64, device=logits.device)
    assert out.dtype == torch.int64 and out.numel() >= b
    _check(lib().nvl_sample_topk_topp(logits.data_ptr(), logits.stride(0), temperatures.data_ptr(), top_k.data_ptr(),
                                      top_p.data_ptr(), out.data_ptr(), tau.data_ptr() if tau is not None else None, b,
                                      vocab, seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF,
                                      offset_dev.data_ptr() if offset_dev is not None else None, _keys_ptr(row_keys, b),
                                      _stream()))
    return out


def sample_shard(logits: torch.Tensor, temperatures: torch.Tensor, col_offset: int, seed: int, offset: int,
                 workspace: torch.Tensor, out_packed: torch.Tensor, offset_dev: torch.Tensor | None = None,
                 row_keys: torch.Tensor | None = None) -> torch.Tensor:
    """This rank's vocabulary shard -> one {key bits, global index} pair per row (int32 [B, 2])."""
    _dev(logits, "logits")
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.bfloat16
    assert temperatures.dtype == torch.float32 and out_packed.dtype == torch.int32 and out_packed.is_contiguous()
    b, vocab = logits.shape
    assert out_packed.numel() >= 2 * b
    _check(lib().nvl_sample_shard(logits.data_ptr(), logits.stride(0), temperatures.data_ptr(), out_packed.data_ptr(), b,
                                  vocab, col_offset, seed & 0xFFFFFFFFFFFFFFFF, offset & 0xFFFFFFFFFFFFFFFF,
                                  offset_dev.data_ptr() if offset_dev is not None else None, _keys_ptr(row_keys, b),
                                  workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()))
    return out_packed


def sample_merge(packed: torch.Tensor, parts: int, batch: int, out: torch.Tensor) -> torch.Tensor:
    """packed int32 [parts, >= batch, 2] (contiguous rows) -> out int64 [batch]: index of the largest key."""
    _dev(packed, "packed")
    assert packed.dtype == torch.int32 and packed.dim() == 3 and packed.shape[0] == parts and packed.shape[2] == 2
    assert packed.stride(2) == 1 and packed.stride(1) == 2 and out.dtype == torch.int64
    _check(lib().nvl_sample_merge(packed.data_ptr(), parts, packed.stride(0) * 4, out.data_ptr(), batch, _stream()))
    return out


class P2PComm:
    """Handle of the hand-written xGMI collectives (csrc/comm.hip). Construction is collective:
    `exchange(bytes) -> list[bytes]` must all-gather a 64-byte token across the tensor-parallel ranks
    and `barrier()` must synchronise them (both host-side, out of band)."""

    def __init__(self, rank: int, world: int, max_bytes: int, exchange, barrier):
        self.rank, self.world = rank, world
        self._h = None
        self._views: dict[tuple, torch.Tensor] = {}
        # Every rank takes part in the exchange AND in the barrier whatever happened locally: a rank that raised
        # before them would leave its peers waiting inside a collective it never joins. A rank that could not
        # create its communicator publishes an all-zero token, which makes every peer fail the same way.
        err: Exception | None = None
        none = b"\0" * 64
        uid = ctypes.create_string_buffer(64)
        try:
            h = c_void_p()
            _check(lib().nvl_allreduce_create(rank, world, max_bytes, ctypes.byref(h)))
            self._h = h
            _check(lib().nvl_allreduce_uid(self._h, uid))
        except Exception as ex:  # noqa: BLE001 — re-raised after the collectives below
            err = ex
        uids = exchange(uid.raw if err is None else none)
        if err is None:
            try:
                assert len(uids) == world and all(len(u) == 64 for u in uids)
                if any(u == none for u in uids):
                    raise NvlError("nvl_allreduce: a peer could not create its communicator")
                blob = ctypes.create_string_buffer(b"".join(uids), 64 * world)
                _check(lib().nvl_allreduce_connect(self._h, blob))
            except Exception as ex:  # noqa: BLE001
                err = ex
        barrier()
        if err is not None:
            self.close()
            raise err
        self.max_bytes = int(lib().nvl_allreduce_max_bytes(self._h))
        # Hand-off flavour: FENCED (system-scope release / acquire around every flag) until somebody has validated
        # the lean form — per-wave store drains only, resting on the shared buffer being uncached on both sides of a
        # link — on the topology at hand: tp.init_p2p does that with a randomised stress run and then calls
        # set_handoff("lean") (14.7 -> 8.7 us per 131 x 5120 all-reduce, profiles/r02_p2p_bench_w2.json).
        self.handoff = "fenced"
        _check(lib().nvl_allreduce_set_fences(self._h, 1))

    def set_handoff(self, flavour: str) -> None:
        """"fenced" | "lean" — must be called with the same value on every rank, between collectives."""
        assert flavour in ("fenced", "lean")
        _check(lib().nvl_allreduce_set_fences(self._h, 1 if flavour == "fenced" else 0))
        self.handoff = flavour

    def input_buffer(self, rows: int, hidden: int, device) -> torch.Tensor:
        """A [rows, hidden] bf16 tensor that IS this rank's shared input region: a GEMM that writes its output
        here hands it to `all_reduce*` without the kernel's copy-in phase."""
        key = (rows, hidden)
        t = self._views.get(key)
        if t is None:
            assert rows * hidden * 2 <= self.max_bytes
            ptr = int(lib().nvl_allreduce_buffer(self._h))

            class _Region:                      # torch wraps foreign device memory through the CUDA array interface
                __cuda_array_interface__ = {"shape": (rows * hidden,), "typestr": "<i2", "data": (ptr, False), "version": 2}
            t = torch.as_tensor(_Region(), device=device).view(torch.bfloat16).view(rows, hidden)
            self._views[key] = t
        return t

    def fits(self, rows: int, hidden: int) -> bool:
        return rows * hidden * 2 <= self.max_bytes and hidden % (8 * self.world) == 0 and hidden <= 8192

    def all_reduce(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        _dev(x, "x")
        assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.bfloat16
        out = x if out is None else out
        _check(lib().nvl_allreduce_run(self._h, x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _stream()))
        return out

    def all_reduce_add_rmsnorm(self, x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float,
                               out: torch.Tensor | None = None) -> torch.Tensor:
        _dev(x, "x")
        assert x.dim() == 2 and x.is_contiguous() and residual.is_contiguous() and x.shape == residual.shape
        assert x.dtype == torch.bfloat16 and residual.dtype == torch.bfloat16
        if out is None:
            out = torch.empty_like(x)
        _check(lib().nvl_allreduce_add_rmsnorm(self._h, x.data_ptr(), residual.data_ptr(), weight.data_ptr(),
                                               out.data_ptr(), x.shape[0], x.shape[1], eps, _stream()))
        return out

    def all_gather(self, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """out[world, nbytes(x)] <- every rank's x (nbytes a multiple of 16, <= 4096)."""
        _dev(x, "x")
        n = x.numel() * x.element_size()
        assert x.is_contiguous() and out.is_contiguous() and out.numel() * out.element_size() >= n * self.world
        _check(lib().nvl_allreduce_gather(self._h, x.data_ptr(), out.data_ptr(), n, _stream()))
        return out

    def status(self) -> None:
        _check(lib().nvl_allreduce_status(self._h))

    def status_async(self, out: torch.Tensor) -> None:
        """out[0] (int32, device) <- 1 if any rank of the group has latched a spin timeout so far, else 0. Enqueue-only
        (capturable): the serving path's form of `status`."""
        _dev(out, "out")
        assert out.dtype == torch.int32 and out.numel() >= 1
        _check(lib().nvl_allreduce_status_async(self._h, out.data_ptr(), _stream()))

    def close(self) -> None:
        if self._h is not None:
            lib().nvl_allreduce_destroy(self._h)
            self._h = None


def feed_tokens(ids: torch.Tensor, src_row: torch.Tensor, prev_tokens: torch.Tensor) -> None:
    """ids[i] = prev_tokens[src_row[i]] where src_row[i] >= 0 (in place; int64 ids, int32 rows)."""
    _dev(ids, "ids")
    assert ids.dtype == torch.int64 and prev_tokens.dtype == torch.int64 and src_row.dtype == torch.int32
    assert ids.is_contiguous() and src_row.is_contiguous() and src_row.numel() == ids.numel()
    _check(lib().nvl_feed_tokens(ids.data_ptr(), src_row.data_ptr(), prev_tokens.data_ptr(), ids.numel(), _stream()))


def _token_cache(token_cache: torch.Tensor, like: torch.Tensor) -> None:
    assert token_cache.dtype == torch.int32 and token_cache.dim() == 1 and token_cache.is_contiguous() \
        and token_cache.device == like.device, "token_cache: want a contiguous int32 [num_blocks * block_size] device tensor"


def store_tokens(ids: torch.Tensor, slots: torch.Tensor, token_cache: torch.Tensor) -> None:
    """token_cache[slots[i]] = ids[i] wherever slots[i] >= 0 (int64 ids, int32 slots; the token cache shadows the KV
    cache slot for slot)."""
    _dev(ids, "ids")
    _token_cache(token_cache, ids)
    assert ids.dtype == torch.int64 and slots.dtype == torch.int32 and ids.is_contiguous() and slots.is_contiguous()
    assert slots.numel() == ids.numel()
    _check(lib().nvl_store_tokens(ids.data_ptr(), slots.data_ptr(), token_cache.data_ptr(), token_cache.numel(),
                                  ids.numel(), _stream()))


def feed_store_tokens(ids: torch.Tensor, src_row: torch.Tensor, prev_tokens: torch.Tensor, slots: torch.Tensor,
                      token_cache: torch.Tensor) -> None:
    """`feed_tokens` and `store_tokens` of the resolved ids in one launch (first node of a decode step)."""
    _dev(ids, "ids")
    _token_cache(token_cache, ids)
    assert ids.dtype == torch.int64 and prev_tokens.dtype == torch.int64 and src_row.dtype == torch.int32
    assert slots.dtype == torch.int32 and ids.is_contiguous() and src_row.is_contiguous() and slots.is_contiguous()
    assert src_row.numel() == ids.numel() and slots.numel() == ids.numel()
    _check(lib().nvl_feed_store_tokens(ids.data_ptr(), src_row.data_ptr(), prev_tokens.data_ptr(), slots.data_ptr(),
                                       token_cache.data_ptr(), token_cache.numel(), ids.numel(), _stream()))


def apply_penalties(logits: torch.Tensor, token_cache: torch.Tensor, block_tables: torch.Tensor,
                    context_lens: torch.Tensor, prompt_lens: torch.Tensor, presence: torch.Tensor,
                    frequency: torch.Tensor, repetition: torch.Tensor, block_size: int, max_context: int) -> torch.Tensor:
    """Presence / frequency / repetition penalties, in place on bf16 logits [B, V], from the rows' token history in the
    token cache (include/nvl.h: the formula, its order and the bounds). block_tables int32 [B, W]; context_lens /
    prompt_lens int32 [B] (context 0: padding row, untouched); the penalties fp32 [B] (0, 0, 1: row untouched)."""
    _dev(logits, "logits")
    _token_cache(token_cache, logits)
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.dtype == torch.bfloat16
    b, vocab = logits.shape
    assert block_tables.dtype == torch.int32 and block_tables.dim() == 2 and block_tables.stride(1) == 1 \
        and block_tables.shape[0] >= b and block_tables.device == logits.device
    for name, t, dt in (("context_lens", context_lens, torch.int32), ("prompt_lens", prompt_lens, torch.int32),
                        ("presence", presence, torch.float32), ("frequency", frequency, torch.float32),
                        ("repetition", repetition, torch.float32)):
        assert t.dtype == dt and t.dim() == 1 and t.is_contiguous() and t.numel() >= b and t.device == logits.device, \
            f"{name}: want a contiguous {dt} [B] tensor on the logits' device"
    _check(lib().nvl_apply_penalties(logits.data_ptr(), logits.stride(0), token_cache.data_ptr(), token_cache.numel(),
                                     block_tables.data_ptr(), block_tables.stride(0), block_tables.shape[1],
                                     context_lens.data_ptr(), prompt_lens.data_ptr(), presence.data_ptr(),
                                     frequency.data_ptr(), repetition.data_ptr(), b, vocab, block_size, max_context,
                                     _stream()))
    return logits


def sample_exponentials_host(seed: int, offset: int, row: int, col0: int, n: int):
    import numpy as np
    e = np.empty(n, dtype=np.float32)
    lib().nvl_sample_exponentials_host(seed, offset, row, col0, n, e.ctypes.data_as(c_void_p))
    return e
