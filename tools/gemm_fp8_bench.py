"""nvl_linear_wide_fp8 against nvl_linear_wide on the bf16 tile-packed weight, same process, cold L2 / MALL before every
sample (layers._time_cold), best of 5: every Qwen3-8B / 32B decode projection, full width and the TP = 8 per-rank shape,
at 16 / 64 / 144 / 256 rows. Writes a JSON table (us, achieved weight GB/s, the two refitted terms of the time model).

    python tools/gemm_fp8_bench.py [--out profiles/fp8_gemm_wide_vs_bf16.json] [--engine]

--engine adds one engine-level pair: qwen3-8b dummy weights, 256 sequences, weight_dtype bf16 against fp8, LLM.generate.

--tile is a leg of its own (the wide-kernel table is not re-measured): nvl_linear_tile_fp8 against the path the same rows
take with weight_dtype="fp8" — F.linear on the dequantised bf16 weight, plus the silu_mul launch for gate|up — on every
full-width Qwen3-8B / 32B projection at 512 / 2048 / 8192 / 16384 rows. Caches warm, the way consecutive prefill GEMMs see
them; the two paths alternate, each sample is a run of back-to-back calls long enough (>= 5 ms) for the device events, best
of 5. With --engine it adds "fp8" against "fp8_only": tok/s on qwen3-8b (256 sequences), and resident weight bytes + KV
blocks of qwen3-32b dummy weights.

    python tools/gemm_fp8_bench.py --tile [--engine] [--out profiles/fp8_only_tile_vs_library.json]

--mxfp4 is a leg of its own as well: nvl_linear_wide_mxfp4 (weight_dtype="mxfp4_dense") against nvl_linear_wide (bf16
tile-packed) and nvl_linear_wide_fp8 on every full-width Qwen3-8B / 32B projection at 1 / 16 / 64 / 144 / 256 rows, cold L2 /
MALL before every sample, best of 5. With --engine it adds resident projection bytes + KV blocks of qwen3-32b dummy
weights with "bf16", "fp8" and "mxfp4_dense".

    python tools/gemm_fp8_bench.py --mxfp4 [--engine] [--out profiles/mxfp4_dense_gemm_wide.json]

--mxfp4 --tile: nvl_linear_tile_mxfp4 (weight_dtype="mxfp4_dense_only") on every full-width Qwen3-8B / 32B projection in the
mode prefill uses, at 512 / 2048 / 8192 / 16384 rows against F.linear on the dequantised bf16 weight (plus the silu_mul
launch for gate|up) and against nvl_linear_tile_fp8, and at 144 / 200 / 256 rows against nvl_linear_wide_mxfp4. Cold L2 /
MALL before every sample, best of 5, device events. With --engine it adds "mxfp4_dense" against "mxfp4_dense_only": tok/s
on qwen3-8b (256 sequences), and resident bytes + KV blocks of qwen3-32b dummy weights.

    python tools/gemm_fp8_bench.py --mxfp4 --tile [--engine] [--out profiles/mxfp4_dense_only_tile.json]
"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_vllm_amd import layers, ops  # noqa: E402

MODELS = {"8b": (4096, 12288, 32, 8), "32b": (5120, 25600, 64, 8)}
ROWS = (16, 64, 144, 256)


def shapes():
    for model, (hidden, inter, heads, kv) in MODELS.items():
        for tp in (1, 8):
            yield model, tp, "qkv", (heads + 2 * kv) * 128 // tp, hidden, ops.LINEAR_BF16
            yield model, tp, "o", hidden, heads * 128 // tp, ops.LINEAR_PARTIAL
            yield model, tp, "gate_up", 2 * inter // tp, hidden, ops.LINEAR_SILU
            yield model, tp, "down", hidden, inter // tp, ops.LINEAR_PARTIAL


def bench_gemms():
    dev = torch.device("cuda")
    rows = []
    for model, tp, proj, n, k, mode in shapes():
        w = (torch.randn(n, k, device=dev) * 0.05).to(torch.bfloat16)
        wp = ops.pack_weight_tiles(w)
        w8p = ops.pack_weight_tiles_fp8(w.to(torch.float8_e4m3fn))
        sc = torch.ones(n // 16, k // 128, device=dev)
        del w
        for m in ROWS:
            x = (torch.randn(m, k, device=dev) * 0.5).to(torch.bfloat16)
            p16, p8 = ops.linear_wide_plan(m, n, k, mode), ops.linear_wide_fp8_plan(m, n, k, mode)
            ws16 = torch.empty(max(p16[1], 16), dtype=torch.uint8, device=dev)
            ws8 = torch.empty(max(p8[1], 16), dtype=torch.uint8, device=dev)
            o16 = ops.linear_wide(x, wp, mode, workspace=ws16, packed=True)
            o8 = ops.linear_wide_fp8(x, w8p, sc, mode, workspace=ws8)
            t16 = layers._time_cold(lambda: ops.linear_wide(x, wp, mode, out=o16, workspace=ws16, packed=True), dev, 5) * 1e3
            t8 = layers._time_cold(lambda: ops.linear_wide_fp8(x, w8p, sc, mode, out=o8, workspace=ws8), dev, 5) * 1e3
            rows.append(dict(model=model, tp=tp, proj=proj, n=n, k=k, mode=mode, m=m, bf16_us=round(t16, 2), fp8_us=round(t8, 2),
                             bf16_splits=p16[0], fp8_splits=p8[0], bf16_w_gbs=round(n * k * 2 / t16 / 1e3, 1),
                             fp8_w_gbs=round(n * k / t8 / 1e3, 1), speedup=round(t16 / t8, 3)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def refit(rows):
    """T = W bytes per CU / a + x bytes per CU / b over the fp8 rows (256 CUs; x bytes per CU taken at 192 columns per
    workgroup, the plan's wide form — rows whose plan took 96 columns are under-counted): least squares for 1/a, 1/b."""
    a = torch.tensor([[r["n"] * r["k"] / 256.0, r["m"] * r["k"] * 2.0 * (r["n"] / 192.0) / 256.0] for r in rows], dtype=torch.float64)
    t = torch.tensor([[r["fp8_us"]] for r in rows], dtype=torch.float64)
    sol = torch.linalg.lstsq(a, t).solution.flatten().tolist()
    return dict(w_gbs_per_cu=round(1e-3 / sol[0], 2) if sol[0] > 0 else None, x_gbs_per_cu=round(1e-3 / sol[1], 2) if sol[1] > 0 else None)


def bench_mxfp4():
    dev = torch.device("cuda")
    rows = []
    for model, tp, proj, n, k, mode in shapes():
        if tp != 1:
            continue
        w = (torch.randn(n, k, device=dev) * 0.05).to(torch.bfloat16)
        wp = ops.pack_weight_tiles(w)
        w8p = ops.pack_weight_tiles_fp8(w.to(torch.float8_e4m3fn))
        sc = torch.ones(n // 16, k // 128, device=dev)
        codes, s4 = ops.quant_pack_mxfp4(w)
        s4 = ops.tile_scales_mxfp4(s4)
        del w
        for m in (1,) + ROWS:
            x = (torch.randn(m, k, device=dev) * 0.5).to(torch.bfloat16)
            plans = ops.linear_wide_plan(m, n, k, mode), ops.linear_wide_fp8_plan(m, n, k, mode), ops.linear_wide_mxfp4_plan(m, n, k, mode)
            ws = [torch.empty(max(p[1], 16), dtype=torch.uint8, device=dev) for p in plans]
            fns = (lambda out=None: ops.linear_wide(x, wp, mode, out=out, workspace=ws[0], packed=True),
                   lambda out=None: ops.linear_wide_fp8(x, w8p, sc, mode, out=out, workspace=ws[1]),
                   lambda out=None: ops.linear_wide_mxfp4(x, codes, s4, mode, out=out, workspace=ws[2]))
            outs = [fn() for fn in fns]
            t16, t8, t4 = (layers._time_cold(lambda: fn(out), dev, 5) * 1e3 for fn, out in zip(fns, outs))
            rows.append(dict(model=model, proj=proj, n=n, k=k, mode=mode, m=m, bf16_us=round(t16, 2), fp8_us=round(t8, 2),
                             mxfp4_us=round(t4, 2), splits=[p[0] for p in plans], mxfp4_w_gbs=round(n * k * 17 / 32 / t4 / 1e3, 1),
                             bf16_over_mxfp4=round(t16 / t4, 3), fp8_over_mxfp4=round(t8 / t4, 3)))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def bench_tile_mxfp4():
    import torch.nn.functional as F
    dev = torch.device("cuda")
    tile, wide = [], []
    for model, tp, proj, n, k, _ in shapes():
        if tp != 1:
            continue
        mode = ops.LINEAR_SILU if proj == "gate_up" else ops.LINEAR_BF16          # (no slabs at these row counts)
        wd = (torch.randn(n, k, device=dev) * 0.05).to(torch.bfloat16)
        codes, s4 = ops.quant_pack_mxfp4(wd)
        ops.unpack_mxfp4(codes, s4, out=wd)                                       # the matrix "mxfp4_dense" multiplies in prefill
        s4 = ops.tile_scales_mxfp4(s4)
        w8p = ops.pack_weight_tiles_fp8((torch.randn(n, k, device=dev) * 0.05).to(torch.float8_e4m3fn))
        sc = torch.exp2(torch.randint(-8, -3, (n // 16, k // 128), device=dev).float())
        for m in TILE_ROWS:
            x = (torch.randn(m, k, device=dev) * 0.5).to(torch.bfloat16)
            out = ops.linear_tile_mxfp4(x, codes, s4, mode)
            lib = (lambda: ops.silu_mul(F.linear(x, wd))) if mode == ops.LINEAR_SILU else (lambda: F.linear(x, wd))
            same = float((out.float() - lib().float()).abs().max()) / float(out.float().abs().max())
            ops.linear_tile_fp8(x, w8p, sc, mode, out=out)                        # (warm-up of the third path)
            t4, tl, t8 = (layers._time_cold(fn, dev, 5) * 1e3 for fn in (
                lambda: ops.linear_tile_mxfp4(x, codes, s4, mode, out=out), lib, lambda: ops.linear_tile_fp8(x, w8p, sc, mode, out=out)))
            tile.append(dict(model=model, proj=proj, n=n, k=k, mode=mode, m=m, tile_mxfp4_us=round(t4, 1), library_us=round(tl, 1),
                             tile_fp8_us=round(t8, 1), tile_mxfp4_pflops=round(2.0 * m * n * k / t4 / 1e9, 3),
                             library_over_tile_mxfp4=round(tl / t4, 3), tile_fp8_over_tile_mxfp4=round(t8 / t4, 3),
                             max_rel_diff=round(same, 5)))
            print(json.dumps(tile[-1]), flush=True)
            del x, out
        for m in (144, 200, 256):
            x = (torch.randn(m, k, device=dev) * 0.5).to(torch.bfloat16)
            plan = ops.linear_wide_mxfp4_plan(m, n, k, mode)
            if plan is None:
                continue
            ws = torch.empty(max(plan[1], 16), dtype=torch.uint8, device=dev)
            out = ops.linear_wide_mxfp4(x, codes, s4, mode, workspace=ws)
            ops.linear_tile_mxfp4(x, codes, s4, mode, out=out)
            tw, tt = (layers._time_cold(fn, dev, 5) * 1e3 for fn in (
                lambda: ops.linear_wide_mxfp4(x, codes, s4, mode, out=out, workspace=ws), lambda: ops.linear_tile_mxfp4(x, codes, s4, mode, out=out)))
            wide.append(dict(model=model, proj=proj, n=n, k=k, mode=mode, m=m, wide_mxfp4_us=round(tw, 1), tile_mxfp4_us=round(tt, 1),
                             wide_over_tile=round(tw / tt, 3)))
            print(json.dumps(wide[-1]), flush=True)
        del wd, codes, s4, w8p, sc
    return tile, wide


def engine_memory_mxfp4(model="qwen3-32b", dtypes=("bf16", "fp8", "mxfp4_dense")):
    """Resident projection bytes and KV blocks of `model` (dummy weights, eager) with each of `dtypes`."""
    from nano_vllm_amd import LLM
    from nano_vllm_amd.weights import write_synthetic_checkpoint
    path = tempfile.mkdtemp(prefix=model.replace("-", "_") + "_")
    write_synthetic_checkpoint(path, model, with_weights=False)
    out = {}
    for dt in dtypes:
        llm = LLM(path, dummy_weights=True, max_model_len=4096, enforce_eager=True, weight_dtype=dt)
        r = llm.model_runner
        copies = sum(sum(t.numel() * t.element_size() for t in (m.weight_packed, m.weight_fp8_packed, m.weight_scale,
                                                                 *(m.weight_mxfp4 or ())) if t is not None)
                     for m in r.model.modules() if isinstance(m, layers.LinearBase))
        out[dt] = dict(decode_copy_bytes=copies, packed_weight_bytes=r.packed_weight_bytes,
                       model_bytes_allocated=torch.cuda.memory_allocated() - r._kv_storage.numel() * r._kv_storage.element_size(),
                       kv_blocks=llm.config.num_kvcache_blocks, kv_block_tokens=r.block_size)
        llm.exit()
        del llm, r
        gc.collect()
        torch.cuda.empty_cache()
        print(json.dumps({dt: out[dt]}), flush=True)
    return out


TILE_ROWS = (512, 2048, 8192, 16384)


def _best_of(fns, dev, samples=5, window_ms=5.0):
    """Best-of-`samples` time (us per call) of each fn, warm: samples alternate between the fns; one sample is `reps` calls
    back to back between two events, `reps` sized from a first timed call so that the window is >= window_ms."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, reps):
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / reps
    reps = []
    for fn in fns:
        fn()                                          # warm-up: code object, library heuristics, allocator
        reps.append(max(1, int(window_ms / max(window(fn, 1), 1e-3))))
    best = [float("inf")] * len(fns)
    for _ in range(samples):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], window(fn, reps[i]))
    return [b * 1e3 for b in best]


def bench_tile():
    import torch.nn.functional as F
    dev = torch.device("cuda")
    rows = []
    for model, tp, proj, n, k, mode in shapes():
        if tp != 1:
            continue
        mode = ops.LINEAR_SILU if proj == "gate_up" else ops.LINEAR_BF16          # (no slabs at these row counts)
        w8 = (torch.randn(n, k, device=dev) * 0.05).to(torch.float8_e4m3fn)
        sc = torch.exp2(torch.randint(-8, -3, (n // 16, k // 128), device=dev).float())
        wd = (w8.to(torch.bfloat16).view(n // 16, 16, k // 128, 128) * sc.to(torch.bfloat16)[:, None, :, None]).view(n, k)
        w8p = ops.pack_weight_tiles_fp8(w8)
        del w8
        for m in TILE_ROWS:
            x = (torch.randn(m, k, device=dev) * 0.5).to(torch.bfloat16)
            out = ops.linear_tile_fp8(x, w8p, sc, mode)
            lib = (lambda: ops.silu_mul(F.linear(x, wd))) if mode == ops.LINEAR_SILU else (lambda: F.linear(x, wd))
            same = float((out.float() - lib().float()).abs().max()) / float(out.float().abs().max())
            t_tile, t_lib = _best_of([lambda: ops.linear_tile_fp8(x, w8p, sc, mode, out=out), lib], dev)
            rows.append(dict(model=model, proj=proj, n=n, k=k, mode=mode, m=m, tile_us=round(t_tile, 1), library_us=round(t_lib, 1),
                             tile_tflops=round(2.0 * m * n * k / t_tile / 1e6, 1), library_tflops=round(2.0 * m * n * k / t_lib / 1e6, 1),
                             library_over_tile=round(t_lib / t_tile, 3), max_rel_diff=round(same, 5)))
            print(json.dumps(rows[-1]), flush=True)
            del x, out
        del wd, w8p
    return rows


def engine_memory(model="qwen3-32b"):
    """Resident bytes and KV blocks of `model` (dummy weights, eager) with "fp8" and with "fp8_only"."""
    from nano_vllm_amd import LLM
    from nano_vllm_amd.weights import write_synthetic_checkpoint
    path = tempfile.mkdtemp(prefix=model.replace("-", "_") + "_")
    write_synthetic_checkpoint(path, model, with_weights=False)
    out = {}
    for dt in ("fp8", "fp8_only"):
        llm = LLM(path, dummy_weights=True, max_model_len=4096, enforce_eager=True, weight_dtype=dt)
        r = llm.model_runner
        proj = sum(m.weight.numel() * 2 + m.weight_fp8_packed.numel() + m.weight_scale.numel() * 4
                   for m in r.model.modules() if isinstance(m, layers.LinearBase) and m.weight_fp8_packed is not None)
        out[dt] = dict(projection_bytes_resident=proj, packed_weight_bytes=r.packed_weight_bytes,
                       model_bytes_allocated=torch.cuda.memory_allocated() - r._kv_storage.numel() * r._kv_storage.element_size(),
                       kv_blocks=llm.config.num_kvcache_blocks, kv_block_tokens=r.block_size)
        llm.exit()
        del llm, r
        gc.collect()                                  # (parameter <-> weight_loader cycles: the model is freed by the collector)
        torch.cuda.empty_cache()
        print(json.dumps({dt: out[dt]}), flush=True)
    return out


def bench_engine(dtypes=("bf16", "fp8")):
    from nano_vllm_amd import LLM, SamplingParams
    from nano_vllm_amd.weights import write_synthetic_checkpoint
    path = tempfile.mkdtemp(prefix="qwen3_8b_")
    write_synthetic_checkpoint(path, "qwen3-8b", with_weights=False)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(0, 10000, (int(torch.randint(100, 1024, (1,), generator=g)),), generator=g).tolist() for _ in range(256)]
    sp = SamplingParams(temperature=0.6, max_tokens=128, ignore_eos=True)
    out = {}
    for dt in dtypes:
        llm = LLM(path, dummy_weights=True, max_model_len=4096, max_num_seqs=256, weight_dtype=dt)
        llm.generate(prompts[:8], SamplingParams(temperature=0.6, max_tokens=8, ignore_eos=True), use_tqdm=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        llm.generate(prompts, sp, use_tqdm=False)
        torch.cuda.synchronize()
        dtm = time.perf_counter() - t0
        out[dt] = dict(seconds=round(dtm, 3), output_tok_s=round(256 * 128 / dtm, 1),
                       packed_weight_bytes=llm.model_runner.packed_weight_bytes)
        llm.exit()
        del llm
        gc.collect()
        torch.cuda.empty_cache()
        print(json.dumps({dt: out[dt]}), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--tile", action="store_true")
    ap.add_argument("--mxfp4", action="store_true")
    args = ap.parse_args()
    if args.mxfp4 and args.tile:
        args.out = args.out or "profiles/mxfp4_dense_only_tile.json"
        tile, wide = bench_tile_mxfp4()
        result = dict(tile=tile, tile_vs_wide=wide)
        if args.engine:
            result["engine_qwen3_8b_256seq"] = bench_engine(("mxfp4_dense", "mxfp4_dense_only"))
            result["memory_qwen3_32b"] = engine_memory_mxfp4(dtypes=("mxfp4_dense", "mxfp4_dense_only"))
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        sys.exit(0)
    if args.mxfp4:
        args.out = args.out or "profiles/mxfp4_dense_gemm_wide.json"
        result = dict(gemm=bench_mxfp4())
        if args.engine:
            result["memory_qwen3_32b"] = engine_memory_mxfp4()
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        sys.exit(0)
    if args.tile:
        args.out = args.out or "profiles/fp8_only_tile_vs_library.json"
        result = dict(tile=bench_tile())
        if args.engine:
            result["engine_qwen3_8b_256seq"] = bench_engine(("fp8", "fp8_only"))
            result["memory_qwen3_32b"] = engine_memory()
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
        sys.exit(0)
    args.out = args.out or "profiles/fp8_gemm_wide_vs_bf16.json"
    table = bench_gemms()
    result = dict(gemm=table, refit_fp8=refit(table))
    if args.engine:
        result["engine_qwen3_8b_256seq"] = bench_engine()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result["refit_fp8"]))
