"""Top-k / top-p sampler kernel (nvl_sample_topk_topp) against a float64 restatement of its semantics: the selection
through `tau`, the draw through oracle/philox.py, identity with the plain sampler where no filter is on."""
import numpy as np
import pytest
import torch

from nano_vllm_amd import ops
from oracle.philox import race_keys

pytestmark = pytest.mark.gpu
SEED = (5 << 32) | 4242
# 512: one chunk per lane; 4099: ragged tail and unaligned rows; 151,936: the register-resident Qwen3 row; 155,657: past
# the 155,648 columns a workgroup's registers hold — every pass re-reads the row — with unaligned rows again
VOCABS = (512, 4099, 151936, 155657)
DELTA = 1e-5


def tau_ref(l, T, top_k, top_p):
    """The cut of one row in float64: -inf when nothing is cut, else max(v_k, v_p) (ISSUE semantics: distinct values
    sorted downwards, count and mass per value level, smallest prefix of levels reaching k columns / top_p of the mass)."""
    k_on, p_on = 0 < top_k < l.size, top_p < 1
    if T == 0 or not (k_on or p_on) or np.isneginf(l.max()):
        return -np.inf
    vals, counts = np.unique(l.astype(np.float64), return_counts=True)
    vals, counts = vals[::-1], counts[::-1]
    nk = int(np.searchsorted(np.cumsum(counts), top_k)) + 1 if k_on else len(vals)      # levels kept by top-k
    if not p_on:
        return vals[nk - 1]
    with np.errstate(invalid="ignore"):
        mass = np.cumsum(counts[:nk] * np.exp((vals[:nk] - vals[0]) / T))
    return vals[int(np.searchsorted(mass, top_p * mass[-1]))]


def rows_for(vocab):
    """8 rows of peaked logits (randn x 4..6: the mass steps are far wider than DELTA) with the planted cases, their
    settings and their engine-style keys."""
    gen = torch.Generator().manual_seed(1000 + vocab)
    l = (torch.randn(8, vocab, generator=gen) * torch.tensor([4.0, 5, 5, 5, 4, 5, 5, 6])[:, None]).to(torch.bfloat16)
    l[2, l[2].float().topk(2, largest=False).indices] = l[2].topk(19).values[18]        # equal at ranks 19, 20, 21
    l[3] = 1.5                                                        # all equal
    l[4, ::3] = -float("inf")
    l[5, 7:] = -float("inf")                                          # fewer finite columns than top_k
    T = torch.tensor([1.7, 0.6, 1.0, 0.3, 1.0, 0.6, 0.3, 1.7])
    top_k = torch.tensor([0, 20, 20, 20, vocab + 5, 20, 1, 20], dtype=torch.int32)
    top_p = torch.tensor([0.95, 1.0, 1.0, 0.5, 0.5, 0.95, 1.0, 1e-6])
    position = 100 + 7 * torch.arange(8, dtype=torch.int64)
    position[1] = (1 << 24) + 9
    ordinal = torch.arange(8, dtype=torch.int64) * 3 + 1
    return l, T, top_k, top_p, ordinal, position


def launch(l, T, top_k, top_p, keys):
    tau = torch.empty(l.shape[0], device="cuda")
    out = ops.sample_topk_topp(l, T.cuda(), top_k.cuda(), top_p.cuda(), SEED, 0, tau=tau, row_keys=keys.cuda())
    return out.cpu(), tau.cpu().numpy()


@pytest.mark.parametrize("vocab", VOCABS)
def test_selection_and_draw_against_the_fp64_reference(vocab):
    l, T, top_k, top_p, ordinal, position = rows_for(vocab)
    lf = l.float().numpy()
    ref = lambda r, p: tau_ref(lf[r], float(T[r]), int(top_k[r]), p)
    lo = [ref(r, float(top_p[r]) * (1 + DELTA if top_p[r] < 1 else 1)) for r in range(8)]
    hi = [ref(r, float(top_p[r]) * (1 - DELTA if top_p[r] < 1 else 1)) for r in range(8)]
    p_rows = [r for r in range(8) if top_p[r] < 1]
    assert sum(lo[r] == hi[r] for r in p_rows) >= 0.9 * len(p_rows)   # the inputs pin tau exactly (CPU only)
    dl = l.cuda()
    out, tau = launch(dl, T, top_k, top_p, ordinal | (position << 32))
    again, tau2 = launch(dl, T, top_k, top_p, ordinal | (position << 32))
    assert torch.equal(out, again) and np.array_equal(tau, tau2)
    inexact = 0
    for r in range(8):
        print(vocab, r, "tau", tau[r], "bracket", lo[r], hi[r], "token", int(out[r]))
        if top_p[r] >= 1:
            assert tau[r] == lo[r] == hi[r], (r, tau[r], lo[r])                        # top-k exact
        assert lo[r] <= tau[r] <= hi[r], (r, lo[r], tau[r], hi[r])
        assert lf[r, int(out[r])] >= tau[r]
        keys = race_keys(lf[r], float(T[r]), SEED, int(ordinal[r]), int(position[r]))
        keys = np.where(lf[r] >= tau[r], keys, -np.inf)
        assert keys[int(out[r])] >= keys.max() - 2e-4, (r, int(out[r]), int(keys.argmax()))
        inexact += int(out[r]) != int(keys.argmax())
    assert inexact <= 1


@pytest.mark.parametrize("vocab", VOCABS)
def test_rows_without_a_filter_draw_the_plain_samplers_token(vocab):
    l, T, top_k, top_p, ordinal, position = rows_for(vocab)
    T[1] = T[6] = 0.0                                                 # greedy rows: one even, one odd
    dl, keys = l.cuda(), ordinal | (position << 32)
    ws = torch.empty(ops.sample_workspace_bytes(512), dtype=torch.uint8, device="cuda")
    plain = ops.sample(dl, T.cuda(), SEED, 0, ws, row_keys=keys.cuda()).cpu()
    off_k, off_p = torch.zeros(8, dtype=torch.int32), torch.ones(8)
    out, tau = launch(dl, T, off_k, off_p, keys)
    assert torch.equal(out, plain) and np.isneginf(tau).all()
    odd = torch.arange(8) % 2 == 1
    out, _ = launch(dl, T, torch.where(odd, top_k, off_k), torch.where(odd, top_p, off_p), keys)
    assert torch.equal(out[~odd], plain[~odd])
    assert out[1] == plain[1]                                         # T == 0 ignores its filters


@pytest.mark.parametrize("top_k,top_p", [(1, 1.0), (0, 1e-6)])
def test_degenerate_filters_collapse_to_greedy(top_k, top_p):
    l, T, _, _, ordinal, position = rows_for(4099)
    l[0, [50, 3000]] = 99.0                                           # a tie at the top: the lowest index wins
    out, _ = launch(l.cuda(), T, torch.full((8,), top_k, dtype=torch.int32), torch.full((8,), top_p),
                    ordinal | (position << 32))
    want = l.float().argmax(dim=1)
    want[0], want[3] = 50, out[3]      # (torch.argmax's tie rule is unspecified; the all-equal row keeps every column)
    assert torch.equal(out, want)
