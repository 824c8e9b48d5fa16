"""Time nvl_sample_topk_topp against nvl_sample on the device: 16 / 131 / 256 rows x 151,936 columns, with every row
filtered (top_k = 20, top_p = 0.95), no row filtered, and every other row filtered. Device events around `--iters`
back-to-back launches after a warm-up; the two samplers alternate, `--repeats` times, and the median is reported.

    python tools/sampler_topk_topp_bench.py [--out profiles/sampler_topk_topp.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nano_vllm_amd import ops  # noqa: E402


def timed(fn, iters):
    for _ in range(10):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters          # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
    ops.load_library()
    ws = torch.empty(ops.sample_workspace_bytes(512), dtype=torch.uint8, device="cuda")
    rows = []
    for b in (16, 131, 256):
        gen = torch.Generator().manual_seed(b)
        logits = (torch.randn(b, args.vocab, generator=gen) * 2.5).to(torch.bfloat16).cuda()
        temps = torch.full((b,), 0.6, device="cuda")
        keys = (torch.arange(b, dtype=torch.int64) | (torch.arange(b, dtype=torch.int64) + 100 << 32)).cuda()
        out = torch.empty(b, dtype=torch.int64, device="cuda")
        on = torch.arange(b) >= 0
        settings = {"all rows top_k=20 top_p=0.95": on, "no row filtered": ~on, "every other row filtered": torch.arange(b) % 2 == 1}
        for name, mask in settings.items():
            top_k = torch.where(mask, 20, 0).to(torch.int32).cuda()
            top_p = torch.where(mask, 0.95, 1.0).to(torch.float32).cuda()
            plain, new = [], []
            for _ in range(args.repeats):
                plain.append(timed(lambda: ops.sample(logits, temps, 1, 0, ws, out=out, row_keys=keys), args.iters))
                new.append(timed(lambda: ops.sample_topk_topp(logits, temps, top_k, top_p, 1, 0, out=out, row_keys=keys),
                                 args.iters))
            rows.append(dict(rows=b, vocab=args.vocab, setting=name, nvl_sample_us=round(statistics.median(plain), 2),
                             nvl_sample_topk_topp_us=round(statistics.median(new), 2),
                             spread_us=[round(min(new), 2), round(max(new), 2)]))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
