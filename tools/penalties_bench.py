"""Time nvl_apply_penalties on the device: `--rows` x 151,936 columns, every row penalised, contexts of 1,024 and 4,096
tokens (half prompt, half output, ids uniform over the vocabulary, blocks scattered over the token cache). The launch sits
in a captured graph (`--iters` launches per graph), device events around a replay after a warm-up replay; `--repeats`
replays, the median is reported. The logits are rewritten in place by every launch: their values drift, the work does not.

    python tools/penalties_bench.py [--out profiles/penalties_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_vllm_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    ops.load_library()
    b, bs = args.rows, 256
    results = []
    for ctx in (1024, 4096):
        w = ctx // bs
        gen = torch.Generator().manual_seed(ctx)
        logits = (torch.randn(b, args.vocab, generator=gen) * 2.5).to(torch.bfloat16).cuda()
        cache = torch.randint(0, args.vocab, (b * w * bs,), generator=gen, dtype=torch.int32).cuda()
        bt = torch.randperm(b * w, generator=gen).to(torch.int32).view(b, w).cuda()
        lens = torch.full((b,), ctx, dtype=torch.int32, device="cuda")
        plen = torch.full((b,), ctx // 2, dtype=torch.int32, device="cuda")
        pp, fp, rp = (torch.full((b,), v, device="cuda") for v in (0.7, 0.3, 1.1))
        launch = lambda: ops.apply_penalties(logits, cache, bt, lens, plen, pp, fp, rp, bs, ctx)
        launch()                                        # (the LDS opt-in: outside the capture)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(args.iters):
                launch()
        graph.replay()
        times = []
        for _ in range(args.repeats):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            graph.replay()
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end) * 1e3 / args.iters)
        results.append(dict(rows=b, vocab=args.vocab, context=ctx, nvl_apply_penalties_us=round(statistics.median(times), 2),
                            spread_us=[round(min(times), 2), round(max(times), 2)]))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
