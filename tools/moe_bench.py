"""The Qwen3-30B-A3B expert block (hidden 2048, expert width 768, 128 experts, 8 per token) through route -> plan ->
experts (tile-packed weights) against a per-expert F.linear loop on the same weights in the same process; cold L2 / MALL
before every sample (layers._time_cold), best of 5, device events; the kernel side is timed as a hipGraph replay (what a
decode step does), the loop eagerly (its row counts are host data: it cannot be captured). 1 / 16 / 64 / 256 decode rows and one prefill size.
Writes a JSON table: us of each side, unique expert bytes touched, achieved GB/s of the block against the 8 TB/s peak.

    python tools/moe_bench.py [--out profiles/moe_block_30b_a3b.json]

--weight-dtype mxfp4 instead times nvl_moe_experts_mxfp4 against nvl_moe_experts on the same routing (main_mxfp4):

    python tools/moe_bench.py --weight-dtype mxfp4 [--out profiles/moe_block_30b_a3b_mxfp4.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_vllm_amd import layers, ops  # noqa: E402

HIDDEN, INTER, E, K = 2048, 768, 128, 8
ROWS = (1, 16, 64, 256, 2048)
PEAK_GBS = 8000.0


def expert_loop(x, gu, dn, ids, wts):
    """The baseline: one pair of library GEMMs per routed expert (needs the ids on the host: not capturable)."""
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    for e in ids.unique().tolist():
        t, j = (ids == e).nonzero(as_tuple=True)
        g, u = F.linear(x[t], gu[e]).chunk(2, -1)
        out.index_add_(0, t, wts[t, j, None] * F.linear(F.silu(g) * u, dn[e]).float())
    return out.to(x.dtype)


def main(out_path):
    dev = torch.device("cuda")
    gu = (torch.randn(E, 2 * INTER, HIDDEN, device=dev) * HIDDEN ** -0.5).to(torch.bfloat16)
    dn = (torch.randn(E, HIDDEN, INTER, device=dev) * INTER ** -0.5).to(torch.bfloat16)
    rw = torch.randn(E, HIDDEN, device=dev).to(torch.bfloat16)
    gup = ops.pack_weight_tiles(gu.view(-1, HIDDEN)).view(gu.shape)
    dnp = ops.pack_weight_tiles(dn.view(-1, INTER)).view(dn.shape)
    ws = torch.empty(ops.moe_workspace_bytes(max(ROWS), HIDDEN, INTER, E, K), dtype=torch.uint8, device=dev)
    rows = []
    for m in ROWS:
        x = torch.randn(m, HIDDEN, device=dev).to(torch.bfloat16)
        ids, wts = ops.moe_route(x, rw, K, True)
        out = torch.empty_like(x)

        def block():
            ops.moe_route(x, rw, K, True, ids, wts)
            ops.moe_plan(ids, E, ws)
            ops.moe_experts(x, gup, dnp, ids, wts, ws, out=out, packed=True)

        def experts_only():
            ops.moe_experts(x, gup, dnp, ids, wts, ws, out=out, packed=True)

        block()
        torch.cuda.synchronize()
        # a decode step replays these launches from a hipGraph: time the replay (six eager launches are host-bound)
        g_block, g_experts = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_block):
            block()
        with torch.cuda.graph(g_experts):
            experts_only()
        ref = expert_loop(x, gu, dn, ids, wts)
        err = ((out.float() - ref.float()).abs().max() / ref.float().pow(2).mean().sqrt()).item()
        t_block = layers._time_cold(g_block.replay, dev, 5) * 1e3
        t_experts = layers._time_cold(g_experts.replay, dev, 5) * 1e3
        t_loop = layers._time_cold(lambda: expert_loop(x, gu, dn, ids, wts), dev, 5) * 1e3
        touched = int(ids.unique().numel())
        nbytes = touched * 3 * INTER * HIDDEN * 2
        rows.append(dict(m=m, experts_touched=touched, expert_mbytes=round(nbytes / 1e6, 1), block_us=round(t_block, 1),
                         experts_us=round(t_experts, 1), loop_us=round(t_loop, 1), speedup=round(t_loop / t_block, 2),
                         experts_gbs=round(nbytes / t_experts / 1e3, 1), pct_of_peak=round(nbytes / t_experts / 1e3 / PEAK_GBS * 100, 1),
                         max_diff_over_rms_vs_loop=round(err, 4)))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(dict(shape=dict(hidden=HIDDEN, inter=INTER, experts=E, top_k=K), rows=rows), fh, indent=1)


def main_mxfp4(out_path):
    """nvl_moe_experts_mxfp4 against nvl_moe_experts (tile-packed bf16) on the same routing, in the same process, the
    same protocol. The bf16 side runs on the DEQUANTISED matrices, so both compute the same numbers (max_diff reported);
    bytes are the unique expert bytes each side streams (codes + scale bytes against bf16)."""
    dev = torch.device("cuda")
    rw = torch.randn(E, HIDDEN, device=dev).to(torch.bfloat16)
    gu = (torch.randn(E * 2 * INTER, HIDDEN, device=dev) * HIDDEN ** -0.5).to(torch.bfloat16)
    dn = (torch.randn(E * HIDDEN, INTER, device=dev) * INTER ** -0.5).to(torch.bfloat16)
    q = ops.quant_pack_mxfp4(gu) + ops.quant_pack_mxfp4(dn)

    def dequant(codes, scales, n, k):          # the code tiles back to a row-major bf16 matrix (include/nvl.h's index map)
        mag = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, 0, -.5, -1, -1.5, -2, -3, -4, -6], device=dev)
        c = codes.view(n // 16, k // 128, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(n, k // 2).long()
        v = mag[torch.stack((c & 15, c >> 4), -1).view(n, k // 32, 32)]
        return (v * torch.exp2(scales.float() - 127)[..., None]).view(n, k).to(torch.bfloat16)

    gup = ops.pack_weight_tiles(dequant(q[0], q[1], *gu.shape)).view(E, 2 * INTER, HIDDEN)
    dnp = ops.pack_weight_tiles(dequant(q[2], q[3], *dn.shape)).view(E, HIDDEN, INTER)
    del gu, dn
    ws = torch.empty(ops.moe_workspace_bytes(max(ROWS), HIDDEN, INTER, E, K), dtype=torch.uint8, device=dev)
    rows = []
    for m in ROWS:
        x = torch.randn(m, HIDDEN, device=dev).to(torch.bfloat16)
        ids, wts = ops.moe_route(x, rw, K, True)
        ops.moe_plan(ids, E, ws)
        out4, out16 = torch.empty_like(x), torch.empty_like(x)
        sides = (lambda: ops.moe_experts_mxfp4(x, *q, ids, wts, ws, out=out4),
                 lambda: ops.moe_experts(x, gup, dnp, ids, wts, ws, out=out16, packed=True))
        graphs = []
        for fn in sides:
            fn()
            torch.cuda.synchronize()
            graphs.append(torch.cuda.CUDAGraph())
            with torch.cuda.graph(graphs[-1]):
                fn()
        t4, t16 = (layers._time_cold(g.replay, dev, 5) * 1e3 for g in graphs)
        err = ((out4.float() - out16.float()).abs().max() / out16.float().pow(2).mean().sqrt()).item()
        touched = int(ids.unique().numel())
        b16 = touched * 3 * INTER * HIDDEN * 2
        b4 = b16 * 17 // 64                                       # 4 bits + one scale byte per 32 elements
        rows.append(dict(m=m, experts_touched=touched, mxfp4_us=round(t4, 1), bf16_us=round(t16, 1),
                         mxfp4_mbytes=round(b4 / 1e6, 1), bf16_mbytes=round(b16 / 1e6, 1),
                         mxfp4_gbs=round(b4 / t4 / 1e3, 1), bf16_gbs=round(b16 / t16 / 1e3, 1),
                         speedup=round(t16 / t4, 2), max_diff_over_rms_vs_bf16=round(err, 5)))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(dict(shape=dict(hidden=HIDDEN, inter=INTER, experts=E, top_k=K), rows=rows), fh, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--weight-dtype", choices=("bf16", "mxfp4"), default="bf16")
    args = ap.parse_args()
    if args.weight_dtype == "mxfp4":
        main_mxfp4(args.out or "profiles/moe_block_30b_a3b_mxfp4.json")
    else:
        main(args.out or "profiles/moe_block_30b_a3b.json")
