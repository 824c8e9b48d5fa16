"""Sampling penalties on the host: SamplingParams, Sequence, add_request's refusals, the staging of both step images and
the entry points' host-side validation (no GPU)."""
import pickle

import pytest

from nano_vllm_amd.api import PENALTY_MAX_CONTEXT, SamplingParams
from nano_vllm_amd.engine.seq import Sequence
from test_engine_host import _engine


def test_sampling_params_and_sequence_carry_the_penalties():
    sp = SamplingParams()
    assert (sp.presence_penalty, sp.frequency_penalty, sp.repetition_penalty) == (0.0, 0.0, 1.0) and not sp.penalised
    assert SamplingParams(0.6, 16, True, 20, 0.95, 1.5, 0.5, 1.1).repetition_penalty == 1.1      # appended after top_p
    for bad in (0.0, -1.0):
        with pytest.raises(AssertionError):
            SamplingParams(repetition_penalty=bad)
    seq = Sequence([1, 2, 3], SamplingParams(presence_penalty=1.5, frequency_penalty=0.5, repetition_penalty=1.1))
    assert (seq.presence_penalty, seq.frequency_penalty, seq.repetition_penalty) == (1.5, 0.5, 1.1)
    back = pickle.loads(pickle.dumps(seq))                                         # the TP state resets them
    assert (back.presence_penalty, back.frequency_penalty, back.repetition_penalty) == (0.0, 0.0, 1.0)


def test_penalties_are_staged_per_row_in_both_images():
    eng = _engine(lookahead=False, max_num_seqs=4, num_kvcache_blocks=16)
    runner = eng.model_runner
    for i, kw in enumerate((dict(), dict(presence_penalty=1.5, frequency_penalty=0.5), dict(repetition_penalty=1.25))):
        eng.add_request([7 + i, 8, 9, 10][:3 + (i == 1)], SamplingParams(max_tokens=4, **kw))
    want = dict(ppen=[0.0, 1.5, 0.0], fpen=[0.0, 0.5, 0.0], rpen=[1.0, 1.0, 1.25], plen=[3, 4, 3])
    seqs, _ = eng.scheduler.schedule()
    info = runner.prepare_prefill(seqs)
    # the penalty kernel reads the history through the block tables: staged although no K/V comes from the cache
    st = runner.pstage.np
    assert info["pen"] and not info["paged"] and list(st["ctx"][:3]) == [3, 4, 3]
    assert [int(st["bt"][i, 0]) for i in range(3)] == [s.block_table[0] for s in seqs] and (st["bt"][:3, 1:] == -1).all()
    eng.scheduler.postprocess(seqs, runner.run(seqs, True), True)
    seqs, _ = eng.scheduler.schedule()
    runner.dstage.flip()
    runner.prepare_decode(seqs)
    for st in (runner.pstage.np, runner.dstage.np):
        assert all([float(x) for x in st[name][:3]] == vals for name, vals in want.items())
        assert not runner._penalised(st, 1) and runner._penalised(st, 2)
    other = runner.dstage.nps[1 - runner.dstage.cur]
    assert (other["rpen"] == 1.0).all() and (other["ppen"] == 0.0).all()        # the untouched image holds the off values


def test_engines_refuse_penalised_requests_they_cannot_serve():
    eng = _engine(lookahead=False, num_kvcache_blocks=16)
    eng.config.tensor_parallel_size = 2
    with pytest.raises(ValueError, match="tensor_parallel_size"):
        eng.add_request([1, 2, 3], SamplingParams(presence_penalty=1.0))
    eng.config.tensor_parallel_size, eng.config.max_model_len = 1, PENALTY_MAX_CONTEXT + 1
    with pytest.raises(ValueError, match="max_model_len"):
        eng.add_request([1, 2, 3], SamplingParams(repetition_penalty=1.1))
    assert eng.is_finished()
    eng.add_request([1, 2, 3], SamplingParams())                                 # unpenalised requests are not concerned


def test_host_side_argument_validation_without_gpu():
    from nano_vllm_amd import ops
    lib = ops.load_library()
    call = lambda vocab=151936, bs=256, ctx=4096: lib.nvl_apply_penalties(
        16, vocab, 16, 1 << 20, 16, 16, 16, 16, 16, 16, 16, 16, 4, vocab, bs, ctx, None)
    assert call(vocab=155649) == -1 and b"vocab" in lib.nvl_last_error()
    assert call(ctx=PENALTY_MAX_CONTEXT + 1) == -1 and b"max_context" in lib.nvl_last_error()
    assert call(bs=96) == -1 and b"power of two" in lib.nvl_last_error()
    assert lib.nvl_store_tokens(16, None, 16, 1024, 4, None) == -1 and b"null pointer" in lib.nvl_last_error()
    assert lib.nvl_feed_store_tokens(16, 16, 16, 16, 16, 0, 4, None) == -1 and b"cache_slots" in lib.nvl_last_error()
