"""top_k / top_p on the host side: SamplingParams, Sequence, and the per-row staging of both step images."""
import pickle

import pytest

from nano_vllm_amd.api import SamplingParams
from nano_vllm_amd.engine.seq import Sequence
from test_engine_host import _engine


def test_sampling_params_defaults_and_assertions():
    sp = SamplingParams()
    assert (sp.top_k, sp.top_p) == (0, 1.0)
    assert SamplingParams(0.6, 16, True, 20, 0.95).top_p == 0.95          # appended after ignore_eos
    assert SamplingParams(top_k=-1).top_k == -1
    for bad in (dict(top_k=-2), dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(AssertionError):
            SamplingParams(**bad)


def test_sequence_carries_the_filters_and_its_tp_state_resets_them():
    seq = Sequence([1, 2, 3], SamplingParams(top_k=20, top_p=0.95))
    assert (seq.top_k, seq.top_p) == (20, 0.95)
    assert Sequence([1], SamplingParams(top_k=-1)).top_k == 0
    back = pickle.loads(pickle.dumps(seq))
    assert (back.top_k, back.top_p) == (0, 1.0)


def test_filters_are_staged_per_row_in_both_images():
    eng = _engine(lookahead=False, max_num_seqs=4, num_kvcache_blocks=16)
    runner = eng.model_runner
    sps = [SamplingParams(max_tokens=4), SamplingParams(max_tokens=4, top_k=20, top_p=0.95),
           SamplingParams(max_tokens=4, top_k=-1, top_p=0.5)]
    for i, sp in enumerate(sps):
        eng.add_request([7 + i, 8, 9], sp)
    seqs, is_prefill = eng.scheduler.schedule()
    assert is_prefill and len(seqs) == 3
    eng.scheduler.postprocess(seqs, runner.run(seqs, True), True)
    st = runner.pstage.np
    assert list(st["topk"][:3]) == [0, 20, 0] and [float(x) for x in st["topp"][:3]] == pytest.approx([1.0, 0.95, 0.5])
    assert not runner._filtered(st, 1) and runner._filtered(st, 3)
    seqs, is_prefill = eng.scheduler.schedule()
    assert not is_prefill
    runner.dstage.flip()
    runner.prepare_decode(seqs)
    st = runner.dstage.np
    assert list(st["topk"][:3]) == [0, 20, 0] and [float(x) for x in st["topp"][:3]] == pytest.approx([1.0, 0.95, 0.5])
    assert not runner._filtered(st, 1) and runner._filtered(st, 2)
    assert (runner.dstage.nps[1 - runner.dstage.cur]["topp"] == 1.0).all()      # the untouched image holds the off value


def test_tensor_parallel_engines_refuse_filtered_requests_before_scheduling():
    eng = _engine(lookahead=False, num_kvcache_blocks=16)
    eng.config.tensor_parallel_size = 2
    with pytest.raises(ValueError, match="tensor_parallel_size"):
        eng.add_request([1, 2, 3], SamplingParams(top_k=5))
    assert eng.is_finished()
    eng.add_request([1, 2, 3], SamplingParams())
