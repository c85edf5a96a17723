"""CPU: token selection of generate_tokens with num_beams == 1 around the device path (generation._DeviceSelect, ops.select_step).  CPU tensors
never reach the kernel and return the tokens every release so far returned (recorded from the host block before the device path existed); the
switch is read per call; the ValueErrors; and `_select_reference`, the torch restatement of the kernel's sample rule, against the host sampler
`torch.multinomial(_top_k_top_p(scores / T).softmax(-1), 1)` under the same seed."""
import pytest
import torch

PROMPT = torch.tensor([[1, 2, 3, 1, 2], [9, 8, 9, 8, 9]])
# recorded from the host block (the commit before csrc/select.hip), toy bigram step below, V = 97
GREEDY = [[26, 10, 31, 23, 33, 0, 4, 0], [83, 75, 37, 31, 23, 33, 0, 4]]
SAMPLE_K20_P09_T09_SEED11 = [[33, 27, 94, 51, 4, 0, 0, 0, 0, 0, 0, 0], [84, 75, 19, 75, 19, 75, 37, 13, 27, 44, 58, 95]]
SAMPLE_PLAIN_SEED12 = [[26, 30, 70, 30, 4, 10, 51, 4, 70, 15, 4, 70], [16, 92, 46, 61, 28, 65, 79, 48, 5, 91, 4, 47]]


def _toy_step(V, K=64, seed=3):
    """A fixed seeded bigram table: the next-token logits depend on the last token only.  No model.  The eos id 4 is raised after every third
    token, so that rows finish."""
    table = torch.randn(K, V, generator=torch.Generator().manual_seed(seed))
    table[::3, 4] += 3.0
    calls = []

    def step(ids, mask, past, beam_idx):
        calls.append((ids.shape[1], None if mask is None else tuple(mask.shape)))
        return table[ids[:, -1] % K], None

    step.calls = calls
    return step


@pytest.fixture
def no_kernel(monkeypatch):
    from otter_amd import ops

    def boom(*a, **k):
        raise AssertionError("ops.select_step reached with CPU tensors")

    monkeypatch.setattr(ops, "select_step", boom)


def test_cpu_tensors_keep_the_host_block_and_its_tokens(no_kernel):
    from otter_amd import generation as G

    out = G.generate_tokens(_toy_step(97), PROMPT, torch.ones_like(PROMPT), max_new_tokens=12, eos_token_id=4, pad_token_id=0)
    assert out[:, 5:].tolist() == GREEDY and torch.equal(out[:, :5], PROMPT) and out.is_contiguous() and out.dtype == torch.long
    out = G.generate_tokens(_toy_step(97), PROMPT, None, max_new_tokens=12, eos_token_id=[4, 17], pad_token_id=0, no_repeat_ngram_size=2,
                            repetition_penalty=1.3)
    assert out[:, 5:].tolist() == GREEDY
    out = G.generate_tokens(_toy_step(97), PROMPT, None, max_new_tokens=12, eos_token_id=4, pad_token_id=0, do_sample=True, top_k=20, top_p=0.9,
                            temperature=0.9, generator=torch.Generator().manual_seed(11))
    assert out[:, 5:].tolist() == SAMPLE_K20_P09_T09_SEED11
    out = G.generate_tokens(_toy_step(97), PROMPT, None, max_new_tokens=12, pad_token_id=0, do_sample=True, top_k=0, temperature=1.0,
                            generator=torch.Generator().manual_seed(12))
    assert out[:, 5:].tolist() == SAMPLE_PLAIN_SEED12


def test_device_sampling_on_cpu_tensors_runs_the_restatement(no_kernel, monkeypatch):
    """`device_sampling=True` on CPU tensors: `_select_reference` chooses every token, over `exponential_` draws of the caller's generator; the
    result has the host block's shape, pads after eos and stops early like it."""
    from otter_amd import generation as G

    seen = []
    real = G._select_reference

    def spy(scores, q, inv_t, top_k, top_p):
        seen.append((tuple(q.shape), inv_t, top_k, top_p))
        return real(scores, q, inv_t, top_k, top_p)

    monkeypatch.setattr(G, "_select_reference", spy)
    step = _toy_step(97)
    out = G.generate_tokens(step, PROMPT, torch.ones_like(PROMPT), max_new_tokens=12, eos_token_id=4, pad_token_id=0, do_sample=True, top_k=20,
                            top_p=0.9, temperature=0.5, generator=torch.Generator().manual_seed(11), device_sampling=True)
    new = out.shape[1] - 5
    assert len(seen) == new == len(step.calls) and seen[0] == ((2, 97), 2.0, 20, 0.9)
    assert step.calls[-1] == (5 + new - 1, (2, 5 + new - 1))
    for row in out[:, 5:].tolist():
        if 4 in row:
            assert all(t == 0 for t in row[row.index(4) + 1:])
    again = G.generate_tokens(_toy_step(97), PROMPT, torch.ones_like(PROMPT), max_new_tokens=12, eos_token_id=4, pad_token_id=0, do_sample=True,
                              top_k=20, top_p=0.9, temperature=0.5, generator=torch.Generator().manual_seed(11), device_sampling=True)
    assert torch.equal(out, again)


def test_parameters_the_rule_does_not_cover_keep_the_host_block(no_kernel, monkeypatch):
    from otter_amd import generation as G

    def boom(*a, **k):
        raise AssertionError("_select_reference reached")

    monkeypatch.setattr(G, "_select_reference", boom)
    for kw in (dict(temperature=float("inf")), dict(top_p=1.5)):
        a = G.generate_tokens(_toy_step(97), PROMPT, None, max_new_tokens=4, pad_token_id=0, do_sample=True, generator=torch.Generator().manual_seed(2),
                              device_sampling=True, **kw)
        b = G.generate_tokens(_toy_step(97), PROMPT, None, max_new_tokens=4, pad_token_id=0, do_sample=True, generator=torch.Generator().manual_seed(2),
                              **kw)
        assert torch.equal(a, b)
    assert G.inv_temperature_f32(0.7) == float(torch.ones((), dtype=torch.float32) / torch.tensor(0.7, dtype=torch.float32))
    assert G.inv_temperature_f32(None) == 1.0
    for t in (0.0, -1.0, float("nan"), float("inf"), 1e-45, 1e39):
        assert G.inv_temperature_f32(t) is None


def test_device_sampling_needs_sampling_without_beams():
    from otter_amd import generation as G

    with pytest.raises(ValueError, match="device_sampling"):
        G.generate_tokens(_toy_step(97), PROMPT, None, max_new_tokens=2, device_sampling=True)
    with pytest.raises(ValueError, match="device_sampling"):
        G.generate_tokens(_toy_step(97), PROMPT, None, max_new_tokens=2, do_sample=True, num_beams=2, device_sampling=True)


class _FakeDeviceTensor:
    """What _DeviceSelect.usable looks at, without a device."""

    def __init__(self, shape, dtype, is_cuda=True, device="cuda:0", col_stride=1):
        self.shape, self.dtype, self.is_cuda, self.device, self._cs = shape, dtype, is_cuda, device, col_stride

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self._cs if i == 1 else self.shape[1]


def test_the_switch_is_read_at_every_call_and_eligibility_is_the_beam_paths(monkeypatch):
    from otter_amd import generation as G
    from otter_amd import ops

    scores, ids = _FakeDeviceTensor((2, 97), torch.float32), _FakeDeviceTensor((2, 5), torch.int64)
    monkeypatch.delenv("OTTER_HIP_SELECT", raising=False)
    assert G._DeviceSelect.usable(scores, ids, None)
    monkeypatch.setenv("OTTER_HIP_SELECT", "0")
    assert not G._DeviceSelect.usable(scores, ids, None)
    monkeypatch.setenv("OTTER_HIP_SELECT", "1")
    assert G._DeviceSelect.usable(scores, ids, None)
    assert not G._DeviceSelect.usable(_FakeDeviceTensor((2, 97), torch.float32, is_cuda=False, device="cpu"), ids, None)
    assert not G._DeviceSelect.usable(_FakeDeviceTensor((2, 97), torch.bfloat16), ids, None)
    assert not G._DeviceSelect.usable(_FakeDeviceTensor((2, 97), torch.float32, col_stride=2), ids, None)
    assert not G._DeviceSelect.usable(scores, _FakeDeviceTensor((2, 5), torch.int32), None)
    assert not G._DeviceSelect.usable(scores, _FakeDeviceTensor((2, 5), torch.int64, device="cuda:1"), None)
    assert not G._DeviceSelect.usable(_FakeDeviceTensor((2, ops.SELECT_STEP_MAX_VOCAB + 1), torch.float32), ids, None)
    assert G._DeviceSelect.usable(_FakeDeviceTensor((2, ops.SELECT_STEP_MAX_VOCAB), torch.float32), ids, None)
    assert not G._DeviceSelect.usable(scores, ids, _FakeDeviceTensor((2, 5), torch.int64, device="cpu"))


# ---- _select_reference against the host sampler ------------------------------------------------------------------------------------------------

T = 0.7
CONFIGS = [(0, 1.0), (50, 1.0), (0, 0.9), (50, 0.95), (1, 0.5)]
SEEDS, ROWS = 20, 4


def _host_and_reference(scores, top_k, top_p, seed):
    """(host tokens, reference tokens, the host's kept mask, the two generators' final states) for one score matrix under one seed."""
    from otter_amd import generation as G

    g_host, g_ref = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
    warped = G._top_k_top_p(scores / T, top_k, top_p)
    host = torch.multinomial(warped.softmax(-1), 1, generator=g_host).squeeze(1)
    q = torch.empty_like(scores).exponential_(1, generator=g_ref)
    ref = G._select_reference(scores, q, G.inv_temperature_f32(T), top_k, top_p)
    return host, ref, warped > float("-inf"), g_host.get_state(), g_ref.get_state()


@pytest.mark.parametrize("V", [97, 50432, 262144])
def test_reference_equals_the_host_sampler_on_tie_free_scores(V):
    """randn * 3 scores, 5 warper settings x 20 seeds x 4 rows per vocabulary: the same token in every row, and the generator ends in the state
    the host sampler leaves it in."""
    rows = 0
    for c, (top_k, top_p) in enumerate(CONFIGS):
        for seed in range(SEEDS):
            scores = torch.randn(ROWS, V, generator=torch.Generator().manual_seed(1000 * c + seed + V)) * 3
            host, ref, _, s_host, s_ref = _host_and_reference(scores, top_k, top_p, seed)
            assert torch.equal(host, ref), (V, top_k, top_p, seed, host.tolist(), ref.tolist())
            assert torch.equal(s_host, s_ref)
            rows += ROWS
    assert rows == len(CONFIGS) * SEEDS * ROWS


@pytest.mark.parametrize("V", [97, 50432, 262144])
def test_on_tie_rich_scores_only_a_split_tie_group_explains_a_difference(V):
    """The same grid on scores quantised to quarters: wherever the reference's token is not the host's, the host's unstable sort has kept
    some members of a group of equal values and removed others (the reference keeps or removes them together)."""
    for c, (top_k, top_p) in enumerate(CONFIGS):
        for seed in range(SEEDS):
            scores = torch.round(torch.randn(ROWS, V, generator=torch.Generator().manual_seed(1000 * c + seed + V)) * 3 * 4) / 4
            host, ref, kept, s_host, s_ref = _host_and_reference(scores, top_k, top_p, seed)
            assert torch.equal(s_host, s_ref)
            for r in (host != ref).nonzero().flatten().tolist():
                row = scores[r]
                split = [v for v in row[kept[r]].unique().tolist() if bool(((row == v) & ~kept[r]).any())]
                assert split, "row %d of V=%d top_k=%d top_p=%g seed=%d differs without a split tie group" % (r, V, top_k, top_p, seed)


def test_reference_edge_rows():
    """top_k = 1 and a tiny top_p keep the maximum alone; a 0 among the draws wins; the smaller index wins among equal ratios; a row with a NaN
    or without a finite score returns some token."""
    from otter_amd import generation as G

    s = torch.tensor([[0.0, 2.0, 5.0, 5.0, -1.0], [1.0, 1.0, 1.0, 1.0, 1.0]])
    q = torch.ones_like(s)
    assert G._select_reference(s, q, 1.0, 1, 1.0).tolist() == [2, 0]          # both 5s tie at v_k and stay; equal ratios: the first
    assert G._select_reference(s, q, 1.0, 0, 1e-6).tolist() == [2, 0]
    q2 = q.clone()
    q2[0, 4], q2[1, 3] = 0.0, 0.0
    assert G._select_reference(s, q2, 1.0, 0, 1.0).tolist() == [4, 3]          # exp(.) / 0 = inf
    assert G._select_reference(s, q2, 1.0, 2, 1.0).tolist() == [2, 3]          # ... unless top-k removed it
    bad = torch.tensor([[1.0, float("nan"), 3.0], [float("-inf")] * 3, [0.0, float("inf"), 1.0]])
    out = G._select_reference(bad, torch.ones_like(bad), 1.0, 0, 1.0).tolist()
    assert all(0 <= t < 3 for t in out)


def test_one_step_leaves_the_generator_where_the_host_path_leaves_it(no_kernel):
    from otter_amd import generation as G

    g_host, g_dev = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    kw = dict(max_new_tokens=3, pad_token_id=0, do_sample=True, top_k=20, top_p=0.9, temperature=0.7)
    G.generate_tokens(_toy_step(97), PROMPT, None, generator=g_host, **kw)
    G.generate_tokens(_toy_step(97), PROMPT, None, generator=g_dev, device_sampling=True, **kw)
    assert torch.equal(g_host.get_state(), g_dev.get_state())
