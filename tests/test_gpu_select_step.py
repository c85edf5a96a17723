"""Token selection on the device (csrc/select.hip, ops.select_step, generation._DeviceSelect).  Greedy: `torch.equal` to torch.argmax on the same
device tensors.  Sampling: against an fp64 oracle written here, which returns the set of ADMISSIBLE tokens of a row -- the top-k set exact, the
top-p decision free inside a band `delta` and the race inside a band `eps`, both derived below from the kernel's arithmetic -- and against the
host sampler on the rows that have one admissible token.  Then the bookkeeping inside guard frames, determinism, generate_tokens over a toy
bigram step with the switch on and off, host round trips, and one full host with graph replay."""
import gc
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")
NAN = float("nan")
GUARD = 16
SHAPES = [(N, V) for V in (1, 7, 97, 257, 9001, 50432, 262144) for N in (1, 3)]
VEC = 4 * 1024                    # csrc/select.hip: columns one sweep of the workgroup covers (1024 threads x 16-byte loads)


# ---- driving the kernel ---------------------------------------------------------------------------------------------------------------------

class Frame:
    """Every buffer of one ops.select_step call inside guard frames: the scores and q are columns [0, V) of wider poisoned buffers (a strided row),
    ids_buf / unfinished / n_unfinished / eos are views into 1-d buffers with sentinels on either side."""

    def __init__(self, scores, max_len=6, L=3, eos=(), unfinished=None, q=None, offset=0):
        N, V = scores.shape
        self.N, self.V, self.L, self.max_len = N, V, L, max_len
        self.s_whole = torch.full((N, offset + V + 5), 1e30, device=DEV)          # poison behind the view: a huge score would win any row
        self.scores = self.s_whole[:, offset:offset + V]
        self.scores.copy_(scores)
        self.s_before = self.s_whole.clone()
        self.q = None
        if q is not None:
            self.q_whole = torch.zeros((N, offset + V + 3), device=DEV)            # ... and a 0 draw would win any race
            self.q = self.q_whole[:, offset:offset + V]
            self.q.copy_(q)
        self.ids_whole = torch.full((N * max_len + 2 * GUARD,), 77, dtype=torch.long, device=DEV)
        self.ids_buf = self.ids_whole[GUARD:GUARD + N * max_len].view(N, max_len)
        self.ids_buf.fill_(-5)
        self.unf_whole = torch.full((N + 2 * GUARD,), 77, dtype=torch.uint8, device=DEV)
        self.unfinished = self.unf_whole[GUARD:GUARD + N]
        self.unfinished.copy_(torch.ones(N, dtype=torch.uint8) if unfinished is None else torch.tensor(unfinished, dtype=torch.uint8))
        self.n_whole = torch.full((1 + 2 * GUARD,), 77, dtype=torch.int32, device=DEV)
        self.n_unfinished = self.n_whole[GUARD:GUARD + 1]
        self.n_unfinished.fill_(int(self.unfinished.sum()))
        self.eos_whole = torch.full((len(eos) + 2 * GUARD,), 0, dtype=torch.int32, device=DEV)        # (a read past the list would see token 0)
        self.eos = None
        if eos:
            self.eos = self.eos_whole[GUARD:GUARD + len(eos)]
            self.eos.copy_(torch.tensor(list(eos), dtype=torch.int32))

    def run(self, pad=0, **sample):
        from otter_amd import ops

        ops.select_step(self.scores, self.ids_buf, self.L, self.unfinished, self.n_unfinished, self.eos, pad, bool(sample),
                        sample.get("inv_t", 1.0), sample.get("top_k", 0), sample.get("top_p", 1.0), self.q)
        torch.cuda.synchronize()
        return self.ids_buf[:, self.L].clone()

    def intact(self):
        """Nothing but column L of ids_buf (and the bookkeeping scalars) changed."""
        ok = torch.equal(self.s_whole.view(torch.int32), self.s_before.view(torch.int32))             # (bits: a NaN score equals itself)
        ok &= bool((self.ids_whole[:GUARD] == 77).all()) and bool((self.ids_whole[-GUARD:] == 77).all())
        others = torch.ones(self.max_len, dtype=torch.bool, device=DEV)
        others[self.L] = False
        ok &= bool((self.ids_buf[:, others] == -5).all())
        ok &= bool((self.unf_whole[:GUARD] == 77).all()) and bool((self.unf_whole[-GUARD:] == 77).all())
        ok &= bool((self.n_whole[:GUARD] == 77).all()) and bool((self.n_whole[-GUARD:] == 77).all())
        return ok


def tokens(scores, q=None, offset=0, **sample):
    f = Frame(scores, q=q, offset=offset)
    out = f.run(**sample)
    assert f.intact()
    return out


def randn(N, V, seed, scale=3.0):
    return torch.randn(N, V, generator=torch.Generator().manual_seed(seed)) * scale


def draws(N, V, seed):
    return torch.empty(N, V).exponential_(1, generator=torch.Generator().manual_seed(seed))


# ---- greedy --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,V", SHAPES)
def test_greedy_equals_torch_argmax(N, V):
    """Tie-free rows, rows quantised to halves (hundreds of equal maxima at the large V), the maximum planted at index 0, at V - 1 and on either
    side of every sweep boundary of the workgroup, -inf rows and a NaN row (the first NaN wins) -- on a row pointer at every 4-byte phase."""
    cases = [randn(N, V, 1), torch.round(randn(N, V, 2) * 2) / 2, torch.full((N, V), NINF), torch.zeros(N, V)]
    planted = sorted({0, V - 1, V // 2} | {c for b in range(VEC, V, VEC) for c in (b - 1, b, b + 1) if c < V} | {c for c in (1, 2, 3, 4, 5) if c < V})
    for n, col in enumerate(planted[:24] + planted[-8:]):
        s = torch.round(randn(N, V, 3) * 2) / 2
        s[:, col] = 50.0
        if n % 2 and col + 1 < V:
            s[:, col + 1:] = torch.where(s[:, col + 1:] > 1.0, torch.full_like(s[:, col + 1:], 50.0), s[:, col + 1:])    # later equal maxima lose
        cases.append(s)
    nan_row = randn(N, V, 4)
    nan_row[0, V // 3] = NAN
    nan_row[0, V - 1] = NAN
    nan_row[-1, 0] = float("inf")
    cases.append(nan_row)
    inf_row = torch.full((N, V), NINF)
    inf_row[:, V - 1] = -3.0
    cases.append(inf_row)
    for n, s in enumerate(cases):
        f = Frame(s, offset=n % 4)
        got = f.run()
        assert f.intact()
        want = torch.argmax(f.scores, dim=-1)
        assert torch.equal(got, want), (n, N, V, got.tolist(), want.tolist())
    assert tokens(nan_row)[0].item() == V // 3 or V < 3


# ---- the fp64 oracle of the sample rule ------------------------------------------------------------------------------------------------------

U22, U24 = 2.0 ** -22, 2.0 ** -24


def admissible(scores, q, inv_t, top_k, top_p):
    """Per row the set of tokens the rule of include/otter_hip.h admits once the kernel's rounding is granted.  fp64 throughout, from the exact
    fp32 products s' = fp32(s * inv_t).  With x_j = s'_j - m and X = min(max |x_j|, 104) (below -104 an fp32 exponential is 0):
      * a kernel numerator is floor(expf(fl(x)) * 2^40): expf within 2 ulp (2^-22 relative), the rounded subtraction moves the argument by at
        most |x| 2^-24, i.e. the value by that relative amount, and the floor by 2^-40 absolute.  Summed over at most V terms and divided by
        Z >= 1 (the maximum's own numerator), numerator and denominator each:   delta = 2 (2^-22 (1 + X / 4) + V 2^-40).
        A value whose cumulative share lies within delta of 1 - top_p may be kept or removed (the kept set stays a threshold set).
      * a race ratio carries the same two errors and one division (2^-24):     eps_j = 2^-22 + |x_j| 2^-24 + 2^-24,  plus one fp32 denormal
        step 2^-149 / q_j absolute.  j may win iff r_j (1 + eps_j) + 2^-149 / q_j >= max_i r_i (1 - eps_i)."""
    sp32 = scores.float() * torch.tensor(inv_t, dtype=torch.float32)
    sp = sp32.double()
    out = []
    for r in range(sp.shape[0]):
        row, V = sp[r], sp.shape[1]
        m = row.max()
        x = row - m
        e = torch.exp(x)
        keep = torch.ones(V, dtype=torch.bool)
        if top_k > 0:
            keep = row >= torch.topk(row, min(max(top_k, 1), V))[0][-1]                 # exact: comparisons of fp32 numbers
        X = min(float(x[keep & (x > NINF)].abs().max()), 104.0)
        thresholds = [row[keep].min()]
        if top_p < 1.0:
            vals, inverse = torch.unique(row[keep], return_inverse=True)
            share = torch.zeros(len(vals), dtype=torch.float64).index_add_(0, inverse, e[keep]).cumsum(0) / e[keep].sum()
            delta = 2 * (U22 * (1 + X / 4) + V * 2.0 ** -40)
            may = (share > (1.0 - top_p) - delta).nonzero().flatten()
            must = (share > (1.0 - top_p) + delta).nonzero().flatten()
            lo = int(may[0]) if len(may) else len(vals) - 1
            hi = int(must[0]) if len(must) else len(vals) - 1                           # (the maximum is always kept)
            thresholds = [vals[i] for i in range(lo, hi + 1)]
        ratio = e / q[r].double()
        eps = U22 + x.abs().clamp(max=104.0) * U24 + U24
        upper = ratio * (1 + eps) + 2.0 ** -149 / q[r].double()
        lower = ratio * (1 - eps)
        ok = set()
        for t in thresholds:
            kept = keep & (row >= t) & ~torch.isnan(ratio)
            ok |= set((kept & (upper >= lower[kept].max())).nonzero().flatten().tolist())
        out.append(ok)
    return out


def check_family(cases, cap=0.05):
    """Every token of every case is admissible; at most `cap` of the rows may have more than one admissible token; on the rows that have
    exactly one, the kernel's token is the one generation._select_reference returns for the same draws (the host sampler is compared in
    test_sampling_equals_the_host_sampler_on_tie_free_rows).  Returns the number of rows."""
    from otter_amd import generation as G

    rows = multi = 0
    for scores, q, inv_t, top_k, top_p, offset in cases:
        got = tokens(scores, q=q, offset=offset, inv_t=inv_t, top_k=top_k, top_p=top_p).tolist()
        ok = admissible(scores, q, inv_t, top_k, top_p)
        for r, tok in enumerate(got):
            assert tok in ok[r], (tuple(scores.shape), inv_t, top_k, top_p, r, tok, sorted(ok[r])[:8])
            rows += 1
            multi += len(ok[r]) > 1
            if len(ok[r]) == 1:
                assert tok == int(G._select_reference(scores[r:r + 1], q[r:r + 1], inv_t, top_k, top_p))
    assert multi <= cap * rows, "%d of %d rows have more than one admissible token" % (multi, rows)
    return rows


@pytest.mark.parametrize("N,V", SHAPES)
def test_sampling_tokens_are_admissible_on_tie_free_rows(N, V):
    """randn * 3 rows at temperatures 0.5, 0.7 and 2 under every warper combination, on a strided row at a rotating 4-byte phase."""
    from otter_amd import generation as G

    cases = []
    for n, (T, top_k, top_p) in enumerate([(0.7, 0, 1.0), (0.7, 50, 1.0), (0.7, 0, 0.9), (0.7, 50, 0.95), (0.7, 1, 0.5), (0.5, 50, 0.9), (2.0, 50, 0.9),
                                           (2.0, 0, 0.3), (0.5, V + 5, 1.0), (1.0, 0, 1e-6)]):
        for seed in (0, 1):
            cases.append((randn(N, V, 10 * n + seed + V), draws(N, V, 500 + 10 * n + seed), G.inv_temperature_f32(T), top_k, top_p, n % 4))
    assert check_family(cases) == 20 * N


@pytest.mark.parametrize("V", [97, 50432, 262144])
def test_sampling_equals_the_host_sampler_on_tie_free_rows(V):
    """torch.multinomial(_top_k_top_p(scores / T).softmax(-1), 1, generator=g) on the device against the kernel over the draws a clone of g
    makes, compared on the rows with one admissible token."""
    from otter_amd import generation as G

    T, compared = 0.7, 0
    for n, (top_k, top_p) in enumerate([(0, 1.0), (50, 1.0), (0, 0.9), (50, 0.95), (1, 0.5)]):
        scores = randn(3, V, 40 + n + V).to(DEV)
        g = torch.Generator(device=DEV).manual_seed(n)
        g2 = g.clone_state()
        host = torch.multinomial(G._top_k_top_p(scores / T, top_k, top_p).softmax(-1), 1, generator=g).squeeze(1)
        q = torch.empty_like(scores).exponential_(1, generator=g2)
        assert torch.equal(g.get_state(), g2.get_state())
        got = tokens(scores.cpu(), q=q.cpu(), inv_t=G.inv_temperature_f32(T), top_k=top_k, top_p=top_p)
        ok = admissible(scores.cpu(), q.cpu(), G.inv_temperature_f32(T), top_k, top_p)
        for r in range(3):
            assert int(got[r]) in ok[r]
            if len(ok[r]) == 1:
                compared += 1
                assert int(got[r]) == int(host[r]), (V, top_k, top_p, r)
    assert compared >= 0.95 * 15                                                   # (at most 5 % of the rows may be ambiguous)


@pytest.mark.parametrize("V", [7, 97, 9001, 262144])
def test_sampling_placed_inputs(V):
    """Inputs built so that one token is right: the draws are 1 except where a tiny or zero draw makes a chosen column win IF the rule keeps it."""
    N = 3
    base = torch.round(randn(N, V, 5, scale=1.0).clamp(-3, 3) * 4) / 4 - 10.0          # everything else: quantised, far below the planted values
    last, mid = V - 1, V // 2

    def one(s, q, want, **kw):
        got = tokens(s, q=q, offset=1, **kw)
        assert got.tolist() == [want] * N, (V, kw, got.tolist(), want)
        assert all(want in a for a in admissible(s, q, kw.get("inv_t", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0)))

    # top_k = 1: the maximum alone, however small the draws elsewhere; the winner sits in the last column
    s, q = base.clone(), torch.full((N, V), 1e-30)
    s[:, last], q[:, last] = 4.0, 5.0
    one(s, q, last, top_k=1)
    # top_k >= V and top_p = 1: everything is kept -- a zero draw on the smallest score wins (exp / 0 = inf)
    s, q = base.clone(), torch.ones(N, V)
    s[:, mid], q[:, mid] = -40.0, 0.0
    one(s, q, mid, top_k=V + 3)
    one(s, q, mid, top_k=0, top_p=1.0)
    # exactly k distinct values above the rest, k = 3 (k = V at V < 4): the 3rd is kept, the 4th is not
    if V >= 7:
        s, q = base.clone(), torch.ones(N, V)
        s[:, 0], s[:, mid], s[:, last], s[:, 1] = 5.0, 4.0, 3.0, 2.0
        q[:, last], q[:, 1] = 1e-3, 0.0
        one(s, q, last, top_k=3)
        one(s, q, 1, top_k=4)
        # many ties at v_k: two values above, then a group of equal values from which k = 3 takes "one" -- all of the group stay
        s, q = base.clone(), torch.ones(N, V)
        s[:, 0], s[:, 1] = 5.0, 4.0
        s[:, 2::2] = 3.0
        tied_last = 2 + 2 * ((V - 3) // 2)
        q[:, tied_last] = 1e-6
        q[:, 3] = 0.0                                                                # below v_k: removed, its zero draw cannot win
        one(s, q, tied_last, top_k=3)
        # a tie group straddling the top-p boundary: 4 equal values hold 4/5 of the mass below a maximum holding ~1/5; with top_p = 0.5 the
        # host removes ascending until the cumulated share passes 0.5, i.e. splits the group -- the rule keeps all four, both marked members
        s, q = torch.full((N, V), -80.0), torch.ones(N, V)
        s[:, [1, 2, mid, last]] = 0.0
        s[:, 0] = 0.01
        q[:, 1], q[:, last] = 1e-3, 1e-3 * (1 - 1e-3)
        one(s, q, last, top_p=0.5)
        q[:, last] = 1.0
        one(s, q, 1, top_p=0.5)
    # top_p so small that only the maximum is kept
    s, q = base.clone(), torch.full((N, V), 1e-30)
    s[:, mid], q[:, mid] = 0.0, 3.0
    one(s, q, mid, top_p=1e-4)
    # temperature: at T = 0.5 the second value holds e^-2 / (1 + e^-2) = 0.119 of the mass and top_p = 0.85 removes it; at T = 2 it holds
    # e^-0.5 / (1 + e^-0.5) = 0.378 and stays
    s, q = torch.full((N, V), -200.0), torch.ones(N, V)
    s[:, 0], s[:, last] = 1.0, 0.0
    q[:, last] = 1e-3
    one(s, q, 0, top_p=0.85, inv_t=2.0)
    one(s, q, last, top_p=0.85, inv_t=0.5)


def test_rows_without_a_distribution_return_some_token():
    """A NaN score, only -inf, or a +inf among the scores (the host path raises): a token in [0, V), nothing else written."""
    V = 9001
    s = randn(3, V, 6)
    s[0, 17] = NAN
    s[1, :] = NINF
    s[2, 4000] = float("inf")
    f = Frame(s, q=draws(3, V, 7))
    got = f.run(inv_t=1.0, top_k=50, top_p=0.9)
    assert f.intact() and all(0 <= t < V for t in got.tolist())


# ---- bookkeeping and determinism ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("eos", [(), (5,), (900, 5, 17)])
def test_bookkeeping(sample, eos):
    """Rows 0..3 select tokens 5, 17, 6, 5; row 3 is finished already.  ids_buf[:, L] = selected or pad; a live row that selects an eos id is
    cleared and counted down once; a finished row stays finished and is not counted again; only column L changes."""
    V = 257
    s = torch.full((4, V), -30.0)
    for r, t in enumerate([5, 17, 6, 5]):
        s[r, t] = 9.0
    q = torch.ones(4, V) if sample else None
    f = Frame(s, max_len=9, L=8, eos=eos, unfinished=[1, 1, 1, 0], q=q)
    got = f.run(pad=250, **(dict(inv_t=1.0, top_k=3, top_p=0.9) if sample else {}))
    assert f.intact()
    assert got.tolist() == [5, 17, 6, 250]
    live = [0 if t in eos else 1 for t in (5, 17, 6)] + [0]
    assert f.unfinished.tolist() == live and f.n_unfinished.item() == sum(live)
    got = f.run(pad=250, **(dict(inv_t=1.0, top_k=3, top_p=0.9) if sample else {}))       # a second step on the same scores
    assert got.tolist() == [t if l else 250 for t, l in zip([5, 17, 6, 5], live)]
    assert f.unfinished.tolist() == live and f.n_unfinished.item() == sum(live) and f.intact()


@pytest.mark.parametrize("V", [9001, 262144])
def test_two_calls_return_the_same_tokens(V):
    from otter_amd import generation as G

    s, q = torch.round(randn(3, V, 8) * 4) / 4, draws(3, V, 9)
    for kw in (dict(), dict(inv_t=G.inv_temperature_f32(0.7), top_k=50, top_p=0.9), dict(inv_t=1.0, top_k=0, top_p=0.7)):
        f = Frame(s, q=q if kw else None)
        first = f.run(**kw)
        for _ in range(3):
            assert torch.equal(f.run(**kw), first)


# ---- generate_tokens --------------------------------------------------------------------------------------------------------------------------

def _toy_step(V, K=64, seed=3):
    """A fixed seeded bigram table on the device: the next-token logits depend on the last token only.  No model.  The eos id 4 is raised far
    above the rest after every third token, so that rows finish early at every V."""
    table = torch.randn(K, V, generator=torch.Generator().manual_seed(seed))
    table[::3, 4] += 12.0
    table = table.to(DEV)
    calls = []

    def step(ids, mask, past, beam_idx):
        calls.append(ids.shape[1])
        assert mask is None or mask.shape == ids.shape
        return table[ids[:, -1] % K], None

    step.calls = calls
    return step


def _count_kernel(monkeypatch):
    from otter_amd import ops

    calls = []
    real = ops.select_step

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "select_step", counted)
    return calls


PROMPT = [[1, 2, 3, 1, 2], [9, 8, 9, 8, 9]]
SAMPLING = dict(do_sample=True, device_sampling=True, top_k=50, top_p=0.9, temperature=0.7)


@pytest.mark.parametrize("V", [97, 50432])
@pytest.mark.parametrize("mode", ["greedy", "greedy_eos", "sample", "sample_eos"])
def test_generate_tokens_on_a_toy_step(monkeypatch, V, mode):
    """Tokens with OTTER_HIP_SELECT=1 equal the tokens at 0 -- the host block (greedy) or the torch restatement over the same draws (sampling;
    the toy table is tie-free) -- with one kernel call per step and none at 0; an early eos stop takes the same number of steps."""
    from otter_amd import generation as G

    calls = _count_kernel(monkeypatch)
    prompt = torch.tensor(PROMPT, device=DEV)
    mask = torch.ones_like(prompt)
    mask[1, 0] = 0
    kw = dict(max_new_tokens=24, pad_token_id=0, no_repeat_ngram_size=3, repetition_penalty=1.3)
    if mode.endswith("eos"):
        kw.update(eos_token_id=[4, 11], min_new_tokens=2)
    if mode.startswith("sample"):
        kw.update(SAMPLING)
    out, steps = {}, {}
    for switch in ("0", "1", "0"):
        monkeypatch.setenv("OTTER_HIP_SELECT", switch)                               # (read at every call)
        if mode.startswith("sample"):
            kw["generator"] = torch.Generator(device=DEV).manual_seed(11)
        step, n = _toy_step(V), len(calls)
        out[switch] = G.generate_tokens(step, prompt, mask, **kw)
        steps[switch] = len(step.calls)
        assert len(calls) - n == (steps[switch] if switch == "1" else 0)
        assert step.calls == list(range(5, 5 + steps[switch]))
    assert steps["0"] == steps["1"] and (steps["1"] < 24) == mode.endswith("eos")
    assert out["1"].is_contiguous() and out["1"].dtype == torch.long and out["1"].shape == out["0"].shape == (2, 5 + steps["1"])
    assert torch.equal(out["0"], out["1"]), (out["0"][:, 5:].tolist(), out["1"][:, 5:].tolist())


def _sync_mode_detects(mode):
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode(mode)
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            try:
                probe.item()
                probe.item()
                return len(w) == 2
            except RuntimeError:
                return mode == "error"
    finally:
        torch.cuda.set_sync_debug_mode(prev)


def test_no_synchronise_in_the_greedy_loop_without_an_eos_list(monkeypatch):
    """generate_tokens, greedy, no eos: from the second step call to the last one the loop runs inside torch's sync debug mode "error" (the
    first iteration allocates the state and builds the processors' device lists, once per call)."""
    from otter_amd import generation as G

    if not _sync_mode_detects("error"):
        pytest.skip("this torch build does not raise on .item() in sync debug mode 'error': the mode cannot show a synchronise")
    calls = _count_kernel(monkeypatch)
    monkeypatch.setenv("OTTER_HIP_SELECT", "1")
    NEW = 8
    inner = _toy_step(50432)
    prev = torch.cuda.get_sync_debug_mode()

    def step(ids, mask, past, beam_idx):
        out = inner(ids, mask, past, beam_idx)
        if len(inner.calls) == 2:
            torch.cuda.set_sync_debug_mode("error")
        if len(inner.calls) == NEW:
            torch.cuda.set_sync_debug_mode(prev)
        return out

    prompt = torch.tensor(PROMPT, device=DEV)
    try:
        out = G.generate_tokens(step, prompt, torch.ones_like(prompt), max_new_tokens=NEW, eos_token_id=None, pad_token_id=0, no_repeat_ngram_size=3,
                                bad_words_ids=[[6], [2, 3]])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert len(inner.calls) == NEW == len(calls) and out.shape == (2, 5 + NEW)


@pytest.mark.parametrize("sample", [False, True])
def test_at_most_one_synchronise_per_step_with_an_eos_id(monkeypatch, sample):
    """The same loop with one eos id under "warn": between two consecutive calls of the step function at most one synchronising call is
    reported, the read of the 4-byte count of unfinished rows."""
    from otter_amd import generation as G

    if not _sync_mode_detects("warn"):
        pytest.skip("this torch build does not warn on every .item() in sync debug mode 'warn': the mode cannot count synchronises")
    calls = _count_kernel(monkeypatch)
    monkeypatch.setenv("OTTER_HIP_SELECT", "1")
    NEW = 8
    inner = _toy_step(50432)
    prev = torch.cuda.get_sync_debug_mode()
    marks = []
    prompt = torch.tensor(PROMPT, device=DEV)
    kw = dict(SAMPLING, generator=torch.Generator(device=DEV).manual_seed(3)) if sample else {}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")

        def step(ids, mask, past, beam_idx):
            marks.append(len(w))
            out = inner(ids, mask, past, beam_idx)
            if len(inner.calls) == 1:
                torch.cuda.set_sync_debug_mode("warn")
            return out

        try:
            G.generate_tokens(step, prompt, None, max_new_tokens=NEW, eos_token_id=4, pad_token_id=0, no_repeat_ngram_size=3, min_new_tokens=NEW, **kw)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    assert len(inner.calls) == NEW == len(calls)
    per_step = [b - a for a, b in zip(marks[1:-1], marks[2:])]                 # (the first interval holds the set-up's copies to the device)
    assert len(per_step) == NEW - 2 and max(per_step) <= 1, per_step
    assert sum(per_step) == NEW - 2                                           # and the mode did see the count's read each time


# ---- a full host ---------------------------------------------------------------------------------------------------------------------------

def test_mpt_host_static_media_graph_greedy_and_device_sampling(monkeypatch):
    """The 2-layer full-width MPT host, cache_implementation="static", cross_attention_cache=True, graph_decode=True, 12 new tokens, greedy and
    device_sampling: ops.select_step runs once per step with the switch on and never with it off, and the GraphDecodeStep counts are the same
    on both paths -- 11 cached steps, 1 capture, 9 replays.  Greedy tokens are the host block's (the bf16 logits of this model do tie, and
    torch.argmax and the kernel both take the first index); sampled tokens are the restatement's over the same draws (equal values are kept
    or removed together by both)."""
    from otter_amd.graph_decode import GraphDecodeStep
    from tests.test_gpu_media_cache import _build

    calls = _count_kernel(monkeypatch)
    counts = []
    release = GraphDecodeStep.release

    def spy_release(self):
        counts.append((self.steps, self.captures, self.replays, self.use_graph))
        return release(self)

    monkeypatch.setattr(GraphDecodeStep, "release", spy_release)
    model, bench = _build("mpt")
    try:
        B, P_LEN, NEW = 2, 40, 12
        vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN, DEV, seed=103, frames=1)
        mask[1, :5] = 0

        def gen(**kw):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return model.generate(vision_x=vx.to(torch.bfloat16), lang_x=ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=-1,
                                      cache_implementation="static", cross_attention_cache=True, graph_decode=True, **kw)

        for mode in ("greedy", "sample"):
            out = {}
            for switch in ("0", "1"):
                monkeypatch.setenv("OTTER_HIP_SELECT", switch)
                kw = dict(SAMPLING, generator=torch.Generator(device=DEV).manual_seed(5)) if mode == "sample" else {}
                n = len(calls)
                out[switch] = gen(**kw).cpu()
                assert len(calls) - n == (NEW if switch == "1" else 0)
            assert out["1"].shape == out["0"].shape == (B, P_LEN + NEW)
            assert torch.equal(out["0"][:, :P_LEN], ids.cpu()) and torch.equal(out["1"][:, :P_LEN], ids.cpu())
            assert torch.equal(out["0"], out["1"]), (mode, out["0"][:, P_LEN:].tolist(), out["1"][:, P_LEN:].tolist())
        assert len(counts) == 4 and all(c == (NEW - 1, 1, NEW - 3, True) for c in counts), counts
    finally:
        del model
        gc.collect()
        torch.cuda.empty_cache()
