"""Sampling penalties on the GPU: nvl_apply_penalties against a plain restatement of its formula, the two token-cache
writers, and the engine (token cache contents, a frequency penalty that forbids repeats, unpenalised neighbours)."""
import tempfile

import numpy as np
import pytest
import torch

from nano_vllm_amd import LLM, SamplingParams, ops

pytestmark = pytest.mark.gpu
BS, BLOCKS, W = 256, 16, 4                      # block size, blocks of the token cache, block-table width
CYCLE = 77824                                   # columns one LDS table covers (csrc/penalties.hip)
#        context, prompt, block ids (scattered, not monotone; -1 = unused entry)
ROWS = [(1, 0, [9, -1, -1, -1]), (255, 255, [3, -1, -1, -1]), (256, 100, [14, -1, -1, -1]), (257, 0, [2, 11, -1, -1]),
        (700, 300, [13, 1, 7, -1]), (0, 0, [5, -1, -1, -1]), (300, 10, [12, 0, -1, -1]), (513, 512, [10, 4, 6, -1])]
OFF_ROW, PAD_ROW = 6, 5                         # a row with its penalties off and a padding row, between penalised ones
DYADIC = [(1.5, 0.5, 2.0), (0.0, 0.5, 1.0), (1.5, 0.0, 1.25), (0.0, 0.0, 2.0)]      # (presence, frequency, repetition)


def restatement(logits, lists, pens, dtype):
    """The formula of include/nvl.h in `dtype` arithmetic, one operation per line; not rounded to bf16."""
    out = logits.astype(dtype)
    for b, (toks, (p, f, r)) in enumerate(zip(lists, pens)):
        if len(toks) == 0 or (p, f, r) == (0, 0, 1):
            continue
        cnt = np.bincount(toks[ROWS[b][1]:], minlength=out.shape[1]).astype(dtype)
        seen = np.zeros(out.shape[1], dtype=bool)
        seen[toks] = True
        x = np.where(seen, np.where(out[b] > 0, out[b] / dtype(r), out[b] * dtype(r)), out[b])
        x = x - dtype(f) * cnt
        out[b] = x - dtype(p) * (cnt > 0)
    return out


@pytest.mark.parametrize("vocab, pens", [(1000, DYADIC), (CYCLE + 1001, DYADIC), (CYCLE + 1001, [(0.7, 0.3, 1.1)])])
def test_kernel_against_the_restatement(vocab, pens):
    """Dyadic penalties: the float32 and float64 restatements agree (asserted: the precondition) and the kernel equals them
    bit for bit on every column. Others: three fp32 roundings, |got - ref| <= 2^-20 (|l| + |f c| + |p|), plus one bf16 ulp
    of ref; columns outside the rows' lists, the penalties-off row and the padding row keep their bits."""
    g = np.random.default_rng(vocab)
    edge = [CYCLE - 1, CYCLE] if vocab > CYCLE else [500, 501]
    only_prompt, only_out = [0, edge[0], 17, vocab - 2], [vocab - 1, edge[1], 40, 3]
    both = list(g.choice(np.arange(50, vocab - 50), 8, replace=False))
    cache = g.integers(0, vocab, BLOCKS * BS).astype(np.int32)             # garbage that would count if it were read
    cache[::7], cache[3::11] = -5, vocab + 3
    lists = []
    for ctx, plen, blocks in ROWS:
        toks = np.concatenate([g.choice(only_prompt + both, plen), g.choice(only_out + both, ctx - plen)]).astype(np.int64)
        for pos, t in enumerate(toks):
            cache[blocks[pos // BS] * BS + pos % BS] = t
        lists.append(toks)
    assert np.bincount(lists[4][300:]).max() >= 3
    logits = (torch.randn(len(ROWS), vocab, generator=torch.Generator().manual_seed(1)) * 4).bfloat16()
    pens = [(0, 0, 1) if b == OFF_ROW else pens[b % len(pens)] for b in range(len(ROWS))]
    ref = restatement(logits.float().numpy(), lists, pens, np.float64)

    dev = lambda a, dt: torch.tensor(np.asarray(a), dtype=dt).cuda()
    store = torch.zeros(len(ROWS), vocab + 24, dtype=torch.bfloat16).cuda()          # (a row stride above the vocabulary)
    got = store[:, :vocab]
    got.copy_(logits)
    ops.apply_penalties(got, dev(cache, torch.int32), dev([r[2] for r in ROWS], torch.int32),
                        dev([r[0] for r in ROWS], torch.int32), dev([r[1] for r in ROWS], torch.int32),
                        *(dev([p[i] for p in pens], torch.float32) for i in range(3)), BS, W * BS)
    assert (store[:, vocab:] == 0).all()
    got, bits = got.cpu(), lambda t: t.view(torch.int16)
    assert torch.equal(bits(got[[OFF_ROW, PAD_ROW]]), bits(logits[[OFF_ROW, PAD_ROW]])) and not torch.equal(got[4], logits[4])
    if pens[0] == DYADIC[0]:
        ref32 = torch.from_numpy(restatement(logits.float().numpy(), lists, pens, np.float32)).bfloat16()
        assert torch.equal(bits(ref32), bits(torch.from_numpy(ref).bfloat16()))
        assert torch.equal(bits(got), bits(ref32))
        return
    for b, toks in enumerate(lists):
        touched = np.zeros(vocab, dtype=bool)
        touched[toks] = b != OFF_ROW
        assert torch.equal(bits(got[b][~touched]), bits(logits[b][~touched]))
        (p, f, _), want = pens[b], ref[b][touched]
        cnt = np.bincount(toks[ROWS[b][1]:], minlength=vocab)[touched]
        ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-30))) - 7)
        bound = 2.0 ** -20 * (np.abs(logits[b].double().numpy()[touched]) + f * cnt + p) + ulp
        assert (np.abs(got[b].double().numpy()[touched] - want) <= bound).all(), b


def test_token_cache_writers():
    """Slots of -1 are skipped, the others written; the fused entry leaves `ids` exactly as nvl_feed_tokens does."""
    g, n = torch.Generator().manual_seed(0), 300                                   # (more than one workgroup)
    ids, prev = (torch.randint(0, 1 << 20, (n,), generator=g) for _ in range(2))
    src = torch.where(torch.rand(n, generator=g) < 0.5, torch.randint(0, n, (n,), generator=g), -1).int()
    slots = torch.randperm(BLOCKS * BS, generator=g)[:n].int()
    slots[::5] = -1
    keep = slots >= 0
    fed, fused = ids.cuda(), ids.cuda()
    ops.feed_tokens(fed, src.cuda(), prev.cuda())
    for launch, written in ((lambda c: ops.store_tokens(ids.cuda(), slots.cuda(), c), ids),
                            (lambda c: ops.feed_store_tokens(fused, src.cuda(), prev.cuda(), slots.cuda(), c), fed.cpu())):
        cache = torch.full((BLOCKS * BS,), -7, dtype=torch.int32).cuda()
        launch(cache)
        want = torch.full((BLOCKS * BS,), -7, dtype=torch.int32)
        want[slots[keep].long()] = written[keep].int()
        assert torch.equal(cache.cpu(), want)
    assert torch.equal(fused, fed) and not torch.equal(fed.cpu(), ids)


VOCAB, MAX_TOKENS = 512, 24                     # the engine tests' tiny checkpoint


@pytest.fixture(scope="module")
def tiny_ckpt():
    from nano_vllm_amd.weights import write_synthetic_checkpoint
    path = tempfile.mkdtemp(prefix="qwen3tiny_pen_")
    return write_synthetic_checkpoint(path, "qwen3-tiny", seed=0, vocab_size=VOCAB, max_position_embeddings=2048)


def engine(path, eager, **kw):
    return LLM(path, enforce_eager=eager, max_model_len=2048, num_kvcache_blocks=32, max_num_seqs=8, seed=7, **kw)


def generate(path, pens, eager, capture=None):
    """Greedy tokens per request with the given frequency penalties, (penalised decode steps, of them graph replays)."""
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, VOCAB, (int(n),), generator=g).tolist() for n in (5, 40, 130, 17, 300, 64)]
    sps = [SamplingParams(temperature=0.0, max_tokens=MAX_TOKENS, ignore_eos=True, frequency_penalty=f) for f in pens]
    llm = engine(path, eager)
    llm.model_runner.sampler.capture = capture
    outs = llm.generate(prompts, sps, use_tqdm=False)
    steps = (llm.model_runner.penalised_steps, llm.model_runner.penalised_graph_steps)
    llm.exit()
    return [o["token_ids"] for o in outs], steps


@pytest.mark.parametrize("eager", [False, True])
def test_token_cache_shadows_the_kv_cache(tiny_ckpt, eager):
    """While sequences run, the token cache read through their block tables holds their ids at [0, num_tokens - 1)."""
    llm = engine(tiny_ckpt, eager, max_num_batched_tokens=192)
    g = torch.Generator().manual_seed(5)
    first = torch.randint(0, VOCAB, (BS + 40,), generator=g).tolist()
    sp = SamplingParams(temperature=0.0, max_tokens=32, ignore_eos=True)
    llm.add_request(first, sp)                                                     # chunked: 296 tokens, 192 per step
    llm.add_request(torch.randint(0, VOCAB, (BS - 3,), generator=g).tolist(), sp)  # crosses the block edge while decoding
    checked, owners = 0, {True: set(), False: set()}    # first block of the request that computed the prefix / that hit it
    for step in range(16):
        if step == 5:
            llm.add_request(first[:BS] + [1, 2, 3], sp)
        llm.step()
        cache = llm.model_runner.token_cache.cpu()
        for seq in llm.scheduler.running:
            pos = torch.arange(seq.num_tokens - 1)
            slots = torch.tensor(seq.block_table)[pos // BS] * BS + pos % BS
            assert cache[slots].tolist() == seq.token_ids[:-1]
            checked += 1
            if seq.token_ids[:BS] == first[:BS]:
                owners[seq.num_prompt_tokens == len(first)].add(seq.block_table[0])
    assert checked > 30 and len(llm.scheduler.running) == 3
    assert owners[True] == owners[False] and len(owners[True]) == 1
    llm.exit()


@pytest.mark.parametrize("eager", [False, True])
def test_frequency_penalty_and_unpenalised_neighbours(tiny_ckpt, eager):
    """Greedy decoding repeats itself (asserted); a frequency penalty above the range of the captured logits makes every
    request's tokens distinct; unpenalised neighbours generate what they generate alone; penalised steps replay a graph."""
    logits = []
    plain, steps = generate(tiny_ckpt, [0.0] * 6, eager, capture=logits)
    assert steps == (0, 0) and any(len(set(t)) < len(t) for t in plain)
    pen = 2 * max(float(lg.max() - lg.min()) for lg in logits) + 1
    distinct, steps = generate(tiny_ckpt, [pen] * 6, eager)
    assert all(len(set(t)) == len(t) == MAX_TOKENS for t in distinct)
    assert steps[0] > 0 and steps[1] == (0 if eager else steps[0])
    mixed, steps = generate(tiny_ckpt, [0.0, pen] * 3, eager)
    assert mixed[0::2] == plain[0::2] and mixed[1::2] == distinct[1::2]
    assert steps[0] > 0 and steps[1] == (0 if eager else steps[0])
