"""CPU: generation._Processors keeps its host loop for CPU tensors (ops.logits_process is never reached there, and the results are those of the
loop's four functions applied by hand), and the packing of `bad_words_ids` into the flat int32 lists of the HIP path round-trips."""
import pytest
import torch

from otter_amd import generation as G
from otter_amd import ops


def _case(seed, N=3, V=50, L=12, alphabet=6):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, alphabet, (N, L), generator=g)
    scores = torch.randn(N, V, generator=g)
    scores[:, ::7] = 0.0
    scores[:, 3] = float("-inf")
    return ids, scores


def _by_hand(ids, scores, rp, n, bad, eos, suppress):
    """The processors as the loop has always chained them."""
    s = scores.clone()
    if rp != 1.0:
        s = G._repetition_penalty(ids, s, rp)
    if n > 0:
        s = G._no_repeat_ngram(ids, s, n)
    if bad:
        s = G._no_bad_words(ids, s, bad)
    if suppress:
        s[:, eos] = float("-inf")
    return s


@pytest.mark.parametrize("seed,rp,n,min_new", [(0, 1.3, 3, 0), (1, 1.0, 2, 4), (2, 0.7, 1, 0), (3, 1.3, 0, 20), (4, 1.0, 4, 0)])
def test_cpu_tensors_take_the_host_loop_and_never_the_kernel(monkeypatch, seed, rp, n, min_new):
    def boom(*a, **k):
        raise AssertionError("ops.logits_process reached with CPU tensors")

    monkeypatch.setattr(ops, "logits_process", boom)
    monkeypatch.setenv("OTTER_HIP_LOGITS", "1")
    ids, scores = _case(seed)
    eos = [2]
    last = ids[0, -1].item()
    bad_in = [[5], [2], [last, 9], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14], [last, 2]]
    prompt_len = 8
    proc = G._Processors(prompt_len, eos, rp, n, bad_in, min_new, 0)
    assert proc.bad == [w for w in bad_in if w != [2]]              # the eos word is dropped, as before
    got = proc(ids, scores.clone())
    want = _by_hand(ids, scores, rp, n, proc.bad, eos, ids.shape[1] - prompt_len < min_new)
    assert torch.equal(got, want)
    assert proc._lists is None                                      # nothing was built for a device


def test_known_answers_on_a_small_row():
    """Pinned by hand, so that the loop the GPU tests use as their reference is itself checked against something."""
    ids = torch.tensor([[4, 5, 6, 4, 5, 7, 4, 5]])
    s = torch.tensor([[1.0, -1.0, 2.0, 0.0, 2.0, -2.0, 4.0, 8.0, 0.5, 0.25]])
    out = G._Processors(0, [9], 2.0, 3, [[8], [9], [4, 5, 0], [3, 1]], 0, 9)(ids, s.clone())
    ninf = float("-inf")
    #             0 banned by word [4,5,0]; 4 / 5 penalised once; 6 and 7 complete the 3-gram (4,5,.); 8 a bad word; 9 eos below min_length
    assert out.tolist() == [[ninf, -1.0, 2.0, 0.0, 1.0, -4.0, ninf, ninf, ninf, ninf]]


def test_packing_round_trips_with_eos_filtering():
    eos = [7, 3]
    bad_in = [[5], [7], [3], [1, 2], (4,), [9, 8, 7, 6], [], [7, 1], (2, 2)]
    proc = G._Processors(4, eos, None, 0, bad_in, 0, 0)
    single, tokens, offsets = G.pack_bad_words(proc.bad)
    assert single == [5, 4]                                         # the one-token words, eos members dropped ([7] == eos[:1], [3] in eos)
    words = [tokens[a:b] for a, b in zip(offsets[:-1], offsets[1:])]
    assert words == [[1, 2], [9, 8, 7, 6], [7, 1], [2, 2]]          # a word that merely CONTAINS an eos token stays
    assert offsets[0] == 0 and offsets[-1] == len(tokens) and len(offsets) == len(words) + 1
    # together they are the filtered list again (the empty word bans nothing and is in neither)
    assert sorted([[t] for t in single] + words) == sorted(w for w in proc.bad if w)
    assert G.pack_bad_words([]) == ([], [], [0])


def test_switch_is_read_at_call_time_and_cpu_never_dispatches(monkeypatch):
    ids, scores = _case(9)
    proc = G._Processors(0, [], 1.3, 2, None, 0, 0)
    for v in ("0", "1"):
        monkeypatch.setenv("OTTER_HIP_LOGITS", v)
        assert proc._hip(ids, scores.clone()) is False
