"""The Qwen3-30B-A3B expert block (hidden 2048, expert width 768, 128 experts, 8 per token) through route -> plan ->
experts (tile-packed weights) against a per-expert F.linear loop on the same weights in the same process; cold L2 / MALL
before every sample (layers._time_cold), best of 5, device events; the kernel side is timed as a hipGraph replay (what a
decode step does), the loop eagerly (its row counts are host data: it cannot be captured). 1 / 16 / 64 / 256 decode rows and one prefill size.
Writes a JSON table: us of each side, unique expert bytes touched, achieved GB/s of the block against the 8 TB/s peak.

    python tools/moe_bench.py [--out profiles/moe_block_30b_a3b.json]
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


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/moe_block_30b_a3b.json")
    main(ap.parse_args().out)
