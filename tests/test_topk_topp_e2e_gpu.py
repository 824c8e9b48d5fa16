"""Top-k / top-p through the engine on the tiny synthetic checkpoint: filtered steps (eager and as graph replays) leave
unfiltered rows alone, degenerate filters reproduce greedy decoding, sampled tokens lie in the reference's kept set."""
import tempfile

import pytest
import torch

from test_sampler_topk_topp_gpu import DELTA, tau_ref

pytestmark = pytest.mark.gpu
MAX_TOKENS = 10


@pytest.fixture(scope="module")
def tiny_ckpt():
    from nano_vllm_amd.weights import write_synthetic_checkpoint
    path = tempfile.mkdtemp(prefix="qwen3tiny_topk_")
    return write_synthetic_checkpoint(path, "qwen3-tiny", seed=0, vocab_size=512, max_position_embeddings=2048)


def run(path, sps, eager, capture=None):
    """Tokens per request of a fresh engine (same request ordinals, so same draws), (filtered steps, of them replays)."""
    from nano_vllm_amd import LLM
    g = torch.Generator().manual_seed(3)
    prompts = [torch.randint(0, 512, (int(n),), generator=g).tolist() for n in (5, 40, 130, 17, 300, 64)]
    llm = LLM(path, enforce_eager=eager, max_model_len=2048, num_kvcache_blocks=32, max_num_seqs=8, seed=7)
    llm.model_runner.sampler.capture = capture
    outs = llm.generate(prompts, sps, use_tqdm=False)
    steps = (llm.model_runner.filtered_steps, llm.model_runner.filtered_graph_steps)
    llm.exit()
    return [o["token_ids"] for o in outs], steps


def params(n=6, **kw):
    from nano_vllm_amd import SamplingParams
    return [SamplingParams(max_tokens=MAX_TOKENS, ignore_eos=True, **kw) for _ in range(n)]


@pytest.mark.parametrize("eager", [False, True])
def test_filtered_steps_through_the_engine(tiny_ckpt, eager):
    greedy, steps = run(tiny_ckpt, params(temperature=0.0), eager)
    assert steps == (0, 0)
    top1, steps = run(tiny_ckpt, params(temperature=0.8, top_k=1), eager)               # A
    assert top1 == greedy
    assert steps[0] > 0 and steps[1] == (0 if eager else steps[0])
    plain, _ = run(tiny_ckpt, params(temperature=0.7), eager)
    mixed_sps = [a if i % 2 else b for i, (a, b) in enumerate(zip(params(temperature=0.8, top_k=1), params(temperature=0.7)))]
    mixed, steps = run(tiny_ckpt, mixed_sps, eager)                                     # B
    assert mixed[0::2] == plain[0::2] and mixed[1::2] == greedy[1::2]
    assert steps[0] > 0 and steps[1] == (0 if eager else steps[0])


def test_sampled_tokens_lie_in_the_reference_kept_set(tiny_ckpt):                       # C
    logits = []
    toks, _ = run(tiny_ckpt, params(temperature=0.9, top_k=5, top_p=0.8), True, capture=logits)
    # every step here holds all six requests in order (they fit one prefill step and decode together to the same length)
    assert len(logits) >= MAX_TOKENS and all(lg.shape[0] == 6 for lg in logits)        # (the lookahead may run a step ahead)
    for step, lg in enumerate(logits[:MAX_TOKENS]):
        for r in range(6):
            row = lg[r].numpy()
            assert row[toks[r][step]] >= tau_ref(row, 0.9, 5, 0.8 * (1 + DELTA)), (step, r)
