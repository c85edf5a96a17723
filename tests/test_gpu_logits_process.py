"""The logits processors of generate() on HIP (csrc/logits.hip, ops.logits_process, generation._Processors): the kernel against the host loop
ON THE SAME DEVICE TENSORS, bit for bit (`torch.equal`).  The oracle is `_Processors` with OTTER_HIP_LOGITS=0 -- the loop every release so far
has run -- never the code under test.  Then bounds, `generate_tokens` over a toy bigram step in every decoding mode, and the absence of a host
round trip."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")


def _scores(N, V, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    s = torch.randn(N, V, generator=g, device=DEV)
    s[:, ::5] = 0.0                      # exact zeros: 0 / p stays 0 and is not "< 0"
    s[:, 3::11] = NINF                   # already banned: -inf * p
    return s


def _count_kernel(monkeypatch):
    from otter_amd import ops

    calls = []
    real = ops.logits_process

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "logits_process", counted)
    return calls


def _both(monkeypatch, ids, scores, make):
    """(host loop, kernel) results on clones of `scores`; `make()` builds a fresh _Processors."""
    monkeypatch.setenv("OTTER_HIP_LOGITS", "0")
    want = make()(ids, scores.clone())
    monkeypatch.setenv("OTTER_HIP_LOGITS", "1")
    got = make()(ids, scores.clone())
    return want, got


@pytest.mark.parametrize("V", [97, 50432, 262144])
def test_kernel_equals_the_host_loop_bit_for_bit(monkeypatch, V):
    """Every (L, n, p) of the grid, twice over: tokens once from a 16-token alphabet (n-grams repeat, tokens duplicate) and once from the whole
    vocabulary; N, the bad-word set and the eos flag rotate so that every value meets every L and n.  160 cases per vocabulary."""
    from otter_amd import generation as G

    calls = _count_kernel(monkeypatch)
    base = {N: _scores(N, V, 100 + N) for N in (1, 3)}
    g = torch.Generator(device=DEV).manual_seed(V)
    grid = list(itertools.product([1, 2, 3, 4, 255, 256, 257, 1100], [0, 1, 2, 3, 4], [1.0, 1.3], [16, V]))
    n_cases = 0
    for c, (L, n, p, alphabet) in enumerate(grid):
        N = (1, 3)[(c // 3) % 2]
        words_kind = (c // 2) % 5
        suppress = (c // 5) % 2 == 1
        ids = torch.randint(0, alphabet, (N, L), generator=g, device=DEV)
        row0, row_last = ids[0].tolist(), ids[-1].tolist()
        one = [[7]]
        two = [[row0[-1], 11]]                                              # matches row 0 (and whichever row ends alike)
        four = [row_last[-3:] + [13]] if L >= 3 else [[1, 2, 3, 13]]        # matches the last row, or is longer than L + 1
        bad = [None, one, two, four, one + two + four + [[V - 1]]][words_kind]
        eos = [5, V - 2]
        make = lambda: G._Processors(L, eos, p, n, bad, 5 if suppress else 0, 0)
        before = len(calls)
        want, got = _both(monkeypatch, ids, base[N], make)
        active = p != 1.0 or n > 0 or bad is not None or suppress
        assert len(calls) - before == (1 if active else 0), (L, n, p, alphabet)          # the oracle never reached the kernel, the other path did
        assert torch.equal(got, want), "V=%d L=%d n=%d p=%g alphabet=%d N=%d words=%d eos=%d: %d elements differ" % (
            V, L, n, p, alphabet, N, words_kind, suppress, int((got != want).sum()))
        if bad is not None and words_kind in (2, 4):
            assert got[0, 11] == NINF                                       # the two-token word did match
        n_cases += 1
    assert n_cases == 160


@pytest.mark.parametrize("n", [1, 3])
def test_nothing_outside_the_views_is_read_or_written(monkeypatch, n):
    """scores is columns [0, V) of a wider buffer whose tail must keep its sentinel; ids is a view of a wider buffer whose tail holds a token
    (92, outside the alphabet) that would be penalised and banned if it were read, after a tail that would complete an n-gram."""
    from otter_amd import generation as G

    calls = _count_kernel(monkeypatch)
    N, V, L = 3, 97, 300
    g = torch.Generator(device=DEV).manual_seed(5)
    wide_ids = torch.full((N, L + 8), 92, dtype=torch.long, device=DEV)
    wide_ids[:, :L] = torch.randint(0, 16, (N, L), generator=g, device=DEV)
    wide_ids[:, L] = wide_ids[:, 2]                                          # ids[L-2:L] + this one would be a new 3-gram window
    ids = wide_ids[:, :L]
    buf = torch.full((N, V + 64), 12345.0, device=DEV)
    buf[:, :V] = _scores(N, V, 6)
    ref = buf[:, :V].clone()
    make = lambda: G._Processors(L, [5], 1.3, n, [[7], [int(ids[1, -1]), 11]], 5, 0)
    monkeypatch.setenv("OTTER_HIP_LOGITS", "0")
    want = make()(ids.contiguous(), ref.clone())
    monkeypatch.setenv("OTTER_HIP_LOGITS", "1")
    got = make()(ids, buf[:, :V])
    assert len(calls) == 1
    assert got.data_ptr() == buf.data_ptr()                                  # in place, on the view
    assert torch.equal(buf[:, :V], want)
    assert bool((buf[:, V:] == 12345.0).all())
    assert bool((want[:, 92] == ref[:, 92]).all()) and bool((buf[:, 92] == ref[:, 92]).all())


def test_tokens_outside_the_vocabulary_are_skipped(monkeypatch):
    """ids -1, V and 2^31 + 5 in the rows, n = 1, p = 1.3: the host loop's result on the rows with those entries removed."""
    from otter_amd import generation as G

    calls = _count_kernel(monkeypatch)
    N, V, L = 2, 97, 40
    g = torch.Generator(device=DEV).manual_seed(8)
    clean = torch.randint(0, 16, (N, L), generator=g, device=DEV)
    ids = torch.cat([clean[:, :4], torch.full((N, 1), -1, device=DEV), clean[:, 4:20], torch.full((N, 1), V, device=DEV), clean[:, 20:],
                     torch.full((N, 1), 2 ** 31 + 5, device=DEV)], dim=1)
    scores = _scores(N, V, 9)
    make = lambda: G._Processors(0, [], 1.3, 1, None, 0, 0)
    monkeypatch.setenv("OTTER_HIP_LOGITS", "0")
    want = make()(clean, scores.clone())
    monkeypatch.setenv("OTTER_HIP_LOGITS", "1")
    got = make()(ids, scores.clone())
    assert len(calls) == 1
    assert torch.equal(got, want)


def _toy_step(V, K=64, seed=3):
    """A fixed seeded bigram table on the device: the next-token logits depend on the last token only.  No model."""
    table = torch.randn(K, V, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)

    def step(ids, mask, past, beam_idx):
        return table[ids[:, -1] % K], None

    return step


MODES = {
    "greedy": dict(),
    "sample": dict(do_sample=True, top_k=20, temperature=0.9),
    "beam3": dict(num_beams=3),
    "group4x2": dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.5),
}


@pytest.mark.parametrize("V", [97, 50432])
@pytest.mark.parametrize("mode", list(MODES))
def test_generate_tokens_on_a_toy_step(monkeypatch, V, mode):
    """Tokens with the switch on equal tokens with it off, and the kernel ran for every call of the processors."""
    from otter_amd import generation as G

    calls = _count_kernel(monkeypatch)
    procs = []
    real_call = G._Processors.__call__

    def counted_call(self, ids, scores):
        procs.append(1)
        return real_call(self, ids, scores)

    monkeypatch.setattr(G._Processors, "__call__", counted_call)
    step = _toy_step(V)
    prompt = torch.tensor([[1, 2, 3, 1, 2], [9, 8, 9, 8, 9]], device=DEV)
    kw = dict(max_new_tokens=40, eos_token_id=4, pad_token_id=0, no_repeat_ngram_size=3, repetition_penalty=1.3, bad_words_ids=[[6], [2, 3], [9, 10]],
              min_new_tokens=5, **MODES[mode])
    out = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("OTTER_HIP_LOGITS", switch)
        if mode == "sample":
            kw["generator"] = torch.Generator(device=DEV).manual_seed(11)
        n_calls, n_procs = len(calls), len(procs)
        out[switch] = G.generate_tokens(step, prompt, None, **kw)
        steps = len(procs) - n_procs
        assert steps >= 5
        assert len(calls) - n_calls == (steps if switch == "1" else 0)
    assert out["1"].shape[1] > prompt.shape[1] + 5
    assert torch.equal(out["0"], out["1"])


def test_no_host_round_trip(monkeypatch):
    """One call of the processors on the kernel path inside torch's sync debug mode "error" (the lists were built by an earlier call, as in
    generate(): once per _Processors)."""
    from otter_amd import generation as G

    calls = _count_kernel(monkeypatch)
    monkeypatch.setenv("OTTER_HIP_LOGITS", "1")
    N, V, L = 3, 50432, 600
    ids = torch.randint(0, 16, (N, L), generator=torch.Generator(device=DEV).manual_seed(2), device=DEV)
    scores = _scores(N, V, 4)
    proc = G._Processors(L - 1, [5], 1.3, 3, [[7], [int(ids[0, -1]), 11]], 5, 0)
    first = proc(ids, scores.clone())
    again = scores.clone()
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            second = proc(ids, again)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not detects:
        pytest.skip("this torch build does not raise on .item() in sync debug mode 'error': the mode cannot show a synchronise")
    assert len(calls) == 2
    assert torch.equal(first, second) and first[0, 11] == NINF
