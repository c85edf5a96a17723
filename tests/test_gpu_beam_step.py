"""Beam search on the device (csrc/beam.hip, ops.beam_step, generation._DeviceBeam): the kernel against a Python oracle -- the host block of
generate_tokens restated on CPU copies of the same tensors, selecting by a STABLE descending sort (so it implements the tie rule of
include/otter_hip.h: larger sum first, then the smaller flat index) and scoring with generation._BeamHyps in Python floats -- step after step
with the state carried over; guard frames around every buffer; generate_tokens over a toy step and on the full hosts with the switch on and
off; and the absence of host round trips."""
import gc
import struct
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")
CHUNK = 4096                      # csrc/beam.hip: columns per workgroup of the selection pass
V_CHUNKS = 2 * CHUNK + 809        # 9001: three chunks, the last one partial
GUARD = 16


def framed(n, dtype, fill=0):
    """(whole, view): a contiguous 1-d buffer of n elements with GUARD sentinel elements on either side."""
    sentinel = 77 if dtype in (torch.int32, torch.int64, torch.uint8) else 12345.0
    whole = torch.full((n + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
    view = whole[GUARD:GUARD + n]
    view.fill_(fill)
    return whole, view


def frame_intact(whole):
    sentinel = whole[0].item()
    return bool((whole[:GUARD] == sentinel).all()) and bool((whole[-GUARD:] == sentinel).all())


class Oracle:
    """The host block of generate_tokens (the `else` branch of `if do_sample` through `ids = torch.cat(...)`) on CPU tensors."""

    def __init__(self, B, nb, eos, pad, L0, max_len, lp, early):
        from otter_amd import generation as G

        self.B, self.nb, self.eos, self.pad, self.L0, self.max_len = B, nb, eos, pad, L0, max_len
        self.hyps = [G._BeamHyps(nb, float(lp), early) for _ in range(B)]
        self.done = [False] * B
        self.n_cand = max(2, 1 + len(eos)) * nb
        self.tokens = []           # (filled by `drive`: the new tokens of every step)

    def step(self, logp, beam_scores, ids):
        B, nb, eos, L0 = self.B, self.nb, self.eos, self.L0
        V = logp.shape[-1]
        scores = (logp + beam_scores[:, None]).view(B, nb * V)
        ns, ni = torch.sort(scores, dim=1, descending=True, stable=True)
        ns, ni = ns[:, :self.n_cand], ni[:, :self.n_cand]
        n_idx, n_tok, ns_l = (ni // V).tolist(), (ni % V).tolist(), ns.tolist()
        cur_len = ids.shape[1] + 1
        new_scores = torch.zeros(B, nb, dtype=torch.float32)
        new_tokens = torch.full((B, nb), self.pad, dtype=torch.long)
        new_index = torch.zeros(B, nb, dtype=torch.long)
        for b in range(B):
            if self.done[b]:
                new_index[b] = b * nb
                continue
            k = 0
            for rank, (tok, sc, bi) in enumerate(zip(n_tok[b], ns_l[b], n_idx[b])):
                row = b * nb + bi
                if eos and tok in eos:
                    if rank >= nb:
                        continue
                    self.hyps[b].add(ids[row].clone(), sc, cur_len - L0)
                else:
                    new_scores[b, k], new_tokens[b, k], new_index[b, k] = sc, tok, row
                    k += 1
                if k == nb:
                    break
            self.done[b] = self.done[b] or self.hyps[b].is_done(max(ns_l[b]), cur_len, L0, self.max_len)
        beam_idx = new_index.view(-1)
        return new_scores.view(-1), beam_idx, new_tokens.view(-1), torch.cat([ids[beam_idx], new_tokens.view(-1, 1)], dim=1)


class Device:
    """Every buffer of ops.beam_step inside a guard frame; the token history is a [:, :L] view of rows 1..N of a wider, taller buffer filled
    with a poison token, so that anything read beyond column L or outside the rows shows in the results."""

    POISON = 3                     # (an eos id in the cases that have one, and a token of the alphabet in all of them)

    def __init__(self, B, nb, V, eos, pad, L0, max_len, lp, early, prompt):
        from otter_amd import generation as G
        from otter_amd import ops

        N = B * nb
        self.B, self.nb, self.V, self.eos, self.pad, self.L0, self.max_len, self.lp, self.early = B, nb, V, eos, pad, L0, max_len, float(lp), early
        self.n_cand = max(2, 1 + len(eos)) * nb
        f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
        self.frames = {}
        for name, n, dtype, fill in (("beam_scores", N, f32, 0), ("beam_idx", N, i64, -5), ("done", B, i32, 0), ("hyp_score", N, f64, 0),
                                     ("hyp_tokens", N * max_len, i64, self.POISON), ("hyp_len", N, i32, 0), ("hyp_slot", N, i32, 0),
                                     ("hyp_count", B, i32, 0), ("hyp_worst", B, f64, 1e9), ("all_done", 2, i32, 0),
                                     ("workspace", ops.beam_step_workspace_bytes(B, nb, V, self.n_cand), torch.uint8, 0)):
            self.frames[name] = framed(n, dtype, fill)
        self.len_pow = torch.tensor(G.beam_len_pow(max_len - L0 + 1, lp), dtype=f64).to(DEV)
        self.eos_t = torch.tensor(eos, dtype=i32).to(DEV) if eos else None
        self.wide = torch.full((2, N + 2, max_len + 8), self.POISON, dtype=i64, device=DEV)
        bs = torch.zeros(B, nb)
        bs[:, 1:] = -1e9
        self.v("beam_scores").copy_(bs.view(-1))
        self.ids = self.wide[1, 1:N + 1, :L0]
        self.ids.copy_(prompt.repeat_interleave(nb, dim=0))
        self.steps = 0

    def v(self, name):
        return self.frames[name][1]

    def step(self, logp):
        from otter_amd import ops

        L = self.ids.shape[1]
        nxt = self.wide[self.steps % 2, 1:self.B * self.nb + 1, :L + 1]
        self.steps += 1
        v = self.v
        ops.beam_step(logp, v("beam_scores"), self.ids, nxt, v("beam_idx"), self.eos_t, self.pad, self.nb, self.n_cand, self.L0, self.max_len,
                      self.early, self.lp > 0.0, self.len_pow, v("done"), v("hyp_score"), v("hyp_tokens"), v("hyp_len"), v("hyp_slot"),
                      v("hyp_count"), v("hyp_worst"), v("all_done"), v("workspace"))
        read, self.ids = self.ids, nxt
        return read

    def hyps(self):
        from otter_amd import generation as G

        nb = self.nb
        c = {k: self.v(k).cpu() for k in ("hyp_score", "hyp_len", "hyp_slot", "hyp_count", "hyp_worst")}
        tokens = self.v("hyp_tokens").cpu().view(self.B, nb, self.max_len)
        return [G.rebuild_beam_hyps(nb, self.lp, self.early, int(c["hyp_count"][b]), c["hyp_score"][b * nb:(b + 1) * nb].tolist(),
                                    c["hyp_len"][b * nb:(b + 1) * nb].tolist(), c["hyp_slot"][b * nb:(b + 1) * nb].tolist(),
                                    float(c["hyp_worst"][b]), tokens[b]) for b in range(self.B)]


def bits64(x):
    return struct.pack("<d", x)


def compare(dev, orc, want, tag):
    """Everything the step produces and keeps, against the oracle's: the fp32 beam scores and the fp64 hypothesis scores bit for bit."""
    w_scores, w_idx, w_tok, w_ids = want
    L1 = w_ids.shape[1]
    got_scores = dev.v("beam_scores").cpu()
    assert torch.equal(got_scores.view(torch.int32), w_scores.view(torch.int32)), (tag, got_scores.tolist(), w_scores.tolist())
    assert dev.v("beam_idx").cpu().tolist() == w_idx.tolist(), tag
    got_ids = dev.ids.cpu()
    assert got_ids.shape == w_ids.shape and got_ids[:, -1].tolist() == w_tok.tolist(), tag
    assert torch.equal(got_ids, w_ids), tag
    assert [bool(d) for d in dev.v("done").cpu().tolist()] == orc.done, tag
    assert dev.v("all_done").cpu().tolist() == [int(all(orc.done)), sum(orc.done)], tag
    for b, (g, w) in enumerate(zip(dev.hyps(), orc.hyps)):
        assert len(g.beams) == len(w.beams), (tag, b)
        assert bits64(g.worst) == bits64(w.worst), (tag, b, g.worst, w.worst)
        for (gs, gt), (ws, wt) in zip(g.beams, w.beams):                    # list order: entry by entry
            assert bits64(gs) == bits64(ws), (tag, b, gs, ws)
            assert gt.tolist() == wt.tolist(), (tag, b)
    # guard frames: nothing outside the views was written, and what lies beyond the views was not read (it is poison: an eos id)
    for name, (whole, _) in dev.frames.items():
        assert frame_intact(whole), (tag, name)
    N = dev.B * dev.nb
    cur = dev.wide[(dev.steps - 1) % 2]
    assert bool((cur[1:N + 1, L1:] == dev.POISON).all()) and bool((cur[0] == dev.POISON).all()) and bool((cur[N + 1] == dev.POISON).all()), tag


def drive(B, nb, V, eos, lp, early, steps, make_logp, pad=0, L0=3, tag=""):
    """`steps` consecutive steps of one beam search on the kernel and on the oracle, compared after every step.  make_logp(step index, the
    device state before the step) -> logp fp32 [B * nb, V] on the device."""
    max_len = L0 + steps + 1
    prompt = torch.arange(B * L0).view(B, L0) % 5 + 4
    dev = Device(B, nb, V, eos, pad, L0, max_len, lp, early, prompt.to(DEV))
    orc = Oracle(B, nb, eos, pad, L0, max_len, lp, early)
    o_scores = dev.v("beam_scores").cpu().clone()
    o_ids = prompt.repeat_interleave(nb, dim=0)
    for s in range(steps):
        logp = make_logp(s, dev)
        before = logp.clone()
        read_before = dev.ids.clone()
        want = orc.step(logp.cpu(), o_scores, o_ids)
        read_ids = dev.step(logp)
        compare(dev, orc, want, "%s step %d" % (tag, s))
        orc.tokens.append(want[2].tolist())
        assert torch.equal(logp, before) and torch.equal(read_ids, read_before)                 # inputs are read only
        o_scores, o_ids = want[0], want[3]
    return dev, orc


def random_logp(B, nb, V, eos, seed, quantum=None, boost=0.0):
    """Seeded log-probabilities per step.  `quantum`: values rounded to its multiples (exact fp32 sums, MANY exact ties); `boost`: raised eos
    columns in a third of the rows, so that hypotheses are added, lists fill and overflow, and sentences finish."""
    g = torch.Generator(device=DEV).manual_seed(seed)

    def make(s, dev):
        x = torch.randn(B * nb, V, generator=g, device=DEV)
        x = torch.log_softmax(x, dim=-1)
        x[:, 1::13] = NINF
        if eos and boost:
            rows = torch.arange(B * nb, device=DEV)[(torch.arange(B * nb, device=DEV) + s) % 3 == 0]
            for e in eos:
                if e < V:
                    x[rows, e] = x[rows].max(dim=-1).values + boost * (1 + e % 2)
        if quantum:
            x = torch.round(x / quantum) * quantum
        return x

    return make


EOS_LISTS = {0: [], 1: [3], 3: [3, 6, 2]}
CASES = []
for i, (B, nb, V) in enumerate([(1, 1, 7), (3, 2, 7), (1, 3, 7), (3, 5, 7), (3, 1, 97), (1, 2, 97), (3, 3, 97), (1, 5, 97), (1, 1, V_CHUNKS),
                                (3, 2, V_CHUNKS), (3, 3, V_CHUNKS), (1, 5, V_CHUNKS), (1, 3, 262144), (3, 5, 262144)]):
    for n_eos in (0, 1, 3):
        if V == 262144 and n_eos != (1, 3)[B == 3]:
            continue                                                          # the large vocabulary: two cases, its size is what they add
        lp = (0.0, 0.7, 1.0, 2.0)[(i + n_eos) % 4]
        early = (True, False, "never")[(i + n_eos // 2) % 3]
        quantum = (None, 0.25)[(i + n_eos) % 2]
        CASES.append((B, nb, V, n_eos, lp, early, quantum))


@pytest.mark.parametrize("B,nb,V,n_eos,lp,early,quantum", CASES)
def test_kernel_equals_the_host_block_step_after_step(B, nb, V, n_eos, lp, early, quantum):
    """B x nb x V x eos-list length, with length_penalty, early_stopping and the tie-rich quantised scores rotating through them.  The first
    step is generate_tokens' own: beam scores (0, -1e9, ...), so with V >= n_cand every winner is in beam 0 and with V = 7 < n_cand the -1e9
    beams supply candidates whose sums all round to -1e9: ties decided by the flat index."""
    eos = EOS_LISTS[n_eos]
    steps = 3 if V == 262144 else 7
    make = random_logp(B, nb, V, eos, seed=1000 * B + 10 * nb + n_eos + V % 97, quantum=quantum, boost=0.5)
    dev, orc = drive(B, nb, V, eos, lp, early, steps, make, tag="B%d nb%d V%d eos%d" % (B, nb, V, n_eos))
    if n_eos and V < 262144:
        assert sum(len(h.beams) for h in orc.hyps) > 0                       # the case did add hypotheses


def flat_logp(N, V, base=-64.0):
    return torch.full((N, V), base, device=DEV)


def test_all_winners_inside_one_chunk_and_across_boundaries():
    """V = 9001 (chunks [0, 4096), [4096, 8192), [8192, 9001)), nb = 3, no eos: n_cand = 6.  Step 0: the six best sums of beam 0 sit in
    columns 5000..5005 of ONE chunk (a chunk must keep n_cand entries, not one).  Step 1: winners at columns 4095 | 4096 (either side of a
    chunk boundary) and at (beam 0, column V - 1) | (beam 1, column 0) (either side of a beam boundary), one more in the last, partial chunk.
    Step 2: everything equal except one value: five candidates are decided by the flat index alone."""
    B, nb, V = 1, 3, V_CHUNKS

    def make(s, dev):
        x = flat_logp(B * nb, V)
        bs = dev.v("beam_scores")
        if s == 0:
            x[0, 5000:5006] = torch.tensor([-1.0, -3.0, -2.0, -6.0, -5.0, -4.0], device=DEV)
        elif s == 1:
            for k, (j, t) in enumerate([(0, 4095), (0, 4096), (0, V - 1), (1, 0), (2, 9000), (1, 8191)]):
                x[j, t] = -8.0 - k - bs[j]                                    # sums -8, -9, ... (exact: everything is a small integer)
        else:
            x[2, 8500] = -1.0
        return x

    _, orc = drive(B, nb, V, [], 1.0, False, 3, make, tag="placed chunks")
    assert orc.tokens == [[5000, 5002, 5001], [4095, 4096, V - 1], [8500, 0, 1]]   # (pinned so that the placement is seen to work)


def test_exact_ties_across_beams_and_chunks():
    """One sum, exactly, at (beam 2, col 10), (beam 0, col 5000), (beam 1, col 8500), (beam 0, col 4096), (beam 1, col 4095), (beam 2, col
    9000) and (beam 0, col 7): the order is the flat index's, j * V + t.  Beam scores differ per beam after step 0, so the logp values
    differ while the SUMS tie.  Step 2: every sum is -inf but three exact zeros, one per beam: -inf is an ordinary value, ranked by index."""
    B, nb, V = 1, 3, V_CHUNKS
    where = [(2, 10), (0, 5000), (1, 8500), (0, 4096), (1, 4095), (2, 9000), (0, 7)]

    def make(s, dev):
        x = flat_logp(B * nb, V)
        bs = dev.v("beam_scores")
        if s == 0:
            x[0, 100:103] = torch.tensor([-1.0, -2.0, -4.0], device=DEV)      # beam scores -1, -2, -4 from here on
        elif s == 1:
            for j, t in where:
                x[j, t] = -16.0 - bs[j]
        else:
            x[:] = NINF
            x[1, 50] = -bs[1]
            x[0, 60] = -bs[0]
            x[2, 40] = -bs[2]
        return x

    _, orc = drive(B, nb, V, [], 0.7, False, 3, make, tag="placed ties")
    assert orc.tokens == [[100, 101, 102], [7, 4096, 5000], [60, 50, 40]]     # flat order: beam 0's columns first


def test_eos_ranks_overflow_with_equal_scores_and_a_finished_sentence():
    """nb = 2, eos = [3], length_penalty 0 (score = sum), early_stopping False, B = 3; all values multiples of 1/8.
    Sentence 0: step 0: eos at rank 1 (added, score -1); step 1: eos at rank 1 with sum -1 again (added: the list is full with EQUAL
    scores, worst -1); step 2: eos at rank 1 with sum -0.5 > worst: overflow, the lowest (score, list index) = entry 0 leaves, worst stays
    -1 (the second lowest), and a second eos at rank 2 >= nb is skipped; step 3: best sum -2 < worst: done.  Steps 4-5: its rows are padded.
    Sentence 1 has no eos among its candidates and continues throughout; sentence 2 gets an eos at rank 0 at step 4 only."""
    B, nb, V, eos = 3, 2, 97, [3]

    def make(s, dev):
        x = flat_logp(B * nb, V)
        bs = dev.v("beam_scores")
        put = lambda row, t, total: x.__setitem__((row, t), total - bs[row])
        for b in (1, 2):                                                      # clear, distinct continuations
            put(b * nb, 10 + s, -0.25)
            put(b * nb, 20 + s, -0.5)
            put(b * nb + (s > 0), 30 + s, -0.75)
        if s == 0:
            put(0, 10, -0.25); put(0, 3, -1.0); put(0, 11, -1.5)
        elif s == 1:
            put(0, 12, -0.75); put(0, 3, -1.0); put(1, 13, -1.5)
        elif s == 2:
            put(0, 14, -0.25); put(1, 3, -0.5); put(0, 3, -0.625); put(0, 15, -1.5)
        elif s == 3:
            put(0, 16, -2.0); put(1, 17, -2.5)
        if s == 4:
            put(2 * nb, 3, -0.125)
        return x

    dev, orc = drive(B, nb, V, eos, 0.0, False, 6, make, pad=1, tag="placed scorer")
    assert orc.done == [True, False, False]
    assert [s for s, _ in orc.hyps[0].beams] == [-1.0, -0.5] and orc.hyps[0].worst == -1.0
    assert len(orc.hyps[2].beams) == 1 and len(orc.hyps[1].beams) == 0
    assert dev.ids[0:2, -2:].tolist() == [[1, 1], [1, 1]]                     # the padded rows of the finished sentence
    assert dev.v("beam_idx")[0:2].tolist() == [0, 0] and dev.v("beam_scores")[0:2].tolist() == [0.0, 0.0]


def test_nothing_outside_the_views_is_read_or_written():
    """Every buffer sits in a guard frame (checked after every step by `compare`); the token history is a view of a wider and taller buffer
    whose every other element is the poison token 3 = the eos id, in the rows above and below and in the columns beyond L.  The hypothesis
    rows are compared token for token, so a read past column L would show; here the lists fill and overflow over 9 steps."""
    B, nb, V, eos = 3, 3, 97, [3]
    dev, orc = drive(B, nb, V, eos, 1.0, "never", 9, random_logp(B, nb, V, eos, seed=77, boost=1.0), tag="guards")
    assert max(len(h.beams) for h in orc.hyps) == nb
    tokens = dev.v("hyp_tokens").view(B, nb, -1).cpu()
    c = dev.v("hyp_count").cpu().tolist()
    for b, g in enumerate(dev.hyps()):
        used = {int(s) for s in dev.v("hyp_slot").cpu()[b * nb:b * nb + c[b]].tolist()}
        assert len(used) == c[b]                                              # live entries own distinct rows
        for i, (_, t) in enumerate(g.beams):
            slot = int(dev.v("hyp_slot").cpu()[b * nb + i])
            assert bool((tokens[b, slot, t.shape[0]:] == Device.POISON).all())   # a hypothesis row is written up to its length only


# ---- generate_tokens -----------------------------------------------------------------------------------------------------------------------

def _toy_step(V, K=64, seed=3, device=DEV):
    """A fixed seeded bigram table: the next-token logits depend on the last token only.  No model.  The eos id 4 is raised after every third
    token, so that hypotheses are added and sentences finish.  (The table is drawn on the CPU so that the same one serves a CPU check of the
    tie precondition.)"""
    table = torch.randn(K, V, generator=torch.Generator().manual_seed(seed))
    table[::3, 4] += 3.0
    table = table.to(device)
    calls = []

    def step(ids, mask, past, beam_idx):
        calls.append(ids.shape[1])
        return table[ids[:, -1] % K], None

    step.calls = calls
    return step


def _count_kernel(monkeypatch):
    from otter_amd import ops

    calls = []
    real = ops.beam_step

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(ops, "beam_step", counted)
    return calls


def _record_logp(monkeypatch):
    """Every processed logp of the run, as the beam block receives it."""
    from otter_amd import generation as G

    rec = []
    real_call = G._Processors.__call__

    def recording(self, ids, scores):
        out = real_call(self, ids, scores)
        rec.append(out.detach().float().cpu().clone())
        return out

    monkeypatch.setattr(G._Processors, "__call__", recording)
    return rec


def first_tie_step(rec, B, nb, eos, pad, L0, max_len, lp, early, prompt):
    """The precondition of comparing against the host path, whose torch.topk promises no tie order: at every step the top n_cand + 1 sums of
    every unfinished sentence are strictly decreasing.  Replays the recorded logp through the oracle (which reproduces the beam scores) and
    returns the first step that has a tie among them, or None."""
    orc = Oracle(B, nb, eos, pad, L0, max_len, lp, early)
    scores = torch.zeros(B, nb)
    scores[:, 1:] = -1e9
    scores, ids = scores.view(-1), prompt.cpu().repeat_interleave(nb, dim=0)
    for s, logp in enumerate(rec):
        V = logp.shape[1]
        sums = (logp + scores[:, None]).view(B, nb * V)
        top = torch.sort(sums, dim=1, descending=True, stable=True)[0][:, :min(orc.n_cand + 1, nb * V)]
        for b in range(B):
            if not orc.done[b] and not bool((top[b, :-1] > top[b, 1:]).all()):
                return s
        scores, _, _, ids = orc.step(logp, scores, ids)
    return None


TOY_KW = dict(max_new_tokens=24, eos_token_id=4, pad_token_id=0, no_repeat_ngram_size=3, bad_words_ids=[[6], [2, 3], [9, 10]], min_new_tokens=5)


@pytest.mark.parametrize("V", [97, 50432])
@pytest.mark.parametrize("nb", [3, 4])
def test_generate_tokens_on_a_toy_step(monkeypatch, V, nb):
    """The standard call's processors, an eos id and min_new_tokens over a bigram table: tokens with OTTER_HIP_BEAM=1 equal tokens with 0, the
    step function is called equally often, and ops.beam_step runs once per step with the switch on and never with it off.  Precondition,
    asserted for EVERY step of the host path (no step is excluded; seed 3 qualifies, checked on the CPU when the test was written): the top
    n_cand + 1 sums of every unfinished sentence are strictly decreasing."""
    from otter_amd import generation as G

    calls = _count_kernel(monkeypatch)
    rec = _record_logp(monkeypatch)
    prompt = torch.tensor([[1, 2, 3, 1, 2], [9, 8, 9, 8, 9]], device=DEV)
    out, n_steps = {}, {}
    for switch in ("0", "1"):
        monkeypatch.setenv("OTTER_HIP_BEAM", switch)
        step = _toy_step(V)
        del rec[:]
        n = len(calls)
        out[switch] = G.generate_tokens(step, prompt, None, num_beams=nb, **TOY_KW)
        n_steps[switch] = len(step.calls)
        assert len(calls) - n == (n_steps[switch] if switch == "1" else 0)
        if switch == "0":
            assert len(rec) == n_steps["0"]
            assert first_tie_step(rec, 2, nb, [4], 0, 5, 5 + 24, 1.0, False, prompt) is None
    assert n_steps["0"] == n_steps["1"] >= 6
    assert torch.equal(out["0"], out["1"]), (out["0"].tolist(), out["1"].tolist())


def test_generate_tokens_options_on_a_toy_step(monkeypatch):
    """length_penalty, early_stopping, num_return_sequences and an attention mask go through the device path with the host path's tokens; a
    sentence finishes early (early_stopping=True), so the loop ends on the all_done flag with the host path's number of steps."""
    from otter_amd import generation as G

    calls = _count_kernel(monkeypatch)
    rec = _record_logp(monkeypatch)
    prompt = torch.tensor([[1, 2, 3, 1, 2], [9, 8, 9, 8, 9]], device=DEV)
    mask = torch.ones_like(prompt)
    mask[1, :2] = 0
    seen = []
    for kw in (dict(length_penalty=2.0, early_stopping=True, num_return_sequences=2), dict(length_penalty=0.0, early_stopping="never"),
               dict(length_penalty=0.7, eos_token_id=[4, 7, 11])):
        out, n_steps = {}, {}
        for switch in ("0", "1"):
            monkeypatch.setenv("OTTER_HIP_BEAM", switch)
            step = _toy_step(97)
            del rec[:]
            out[switch] = G.generate_tokens(step, prompt, mask, num_beams=3, **dict(TOY_KW, max_new_tokens=30, min_new_tokens=2, **kw))
            n_steps[switch] = len(step.calls)
            if switch == "0":
                eos = kw.get("eos_token_id", 4)
                tie = first_tie_step(rec, 2, 3, eos if isinstance(eos, list) else [eos], 0, 5, 35, kw["length_penalty"],
                                     kw.get("early_stopping", False), prompt)
                assert tie is None, tie
        assert n_steps["0"] == n_steps["1"]
        assert torch.equal(out["0"], out["1"]), (kw, out["0"].tolist(), out["1"].tolist())
        seen.append(n_steps["1"])
    assert len(calls) == sum(seen)
    assert seen[0] < 30                                                       # the early-stopping call did end on the flag


# ---- host round trips ----------------------------------------------------------------------------------------------------------------------

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


def test_no_synchronise_in_the_loop_without_an_eos_list(monkeypatch):
    """generate_tokens, 3 beams, no eos: from the second step call to the last one -- six whole iterations of the loop -- the loop runs inside
    torch's sync debug mode "error".  The step function switches it on at its second call and off at its last: the first iteration builds
    the device lists of the processors and the state of the beam search (copies to the device, once per call), and the one copy of the
    state to the host comes after the loop."""
    from otter_amd import generation as G

    if not _sync_mode_detects("error"):
        pytest.skip("this torch build does not raise on .item() in sync debug mode 'error': the mode cannot show a synchronise")
    calls = _count_kernel(monkeypatch)
    monkeypatch.setenv("OTTER_HIP_BEAM", "1")
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

    prompt = torch.tensor([[1, 2, 3, 1, 2], [9, 8, 9, 8, 9]], device=DEV)
    try:
        out = G.generate_tokens(step, prompt, None, num_beams=3, max_new_tokens=NEW, eos_token_id=None, pad_token_id=0, no_repeat_ngram_size=3,
                                bad_words_ids=[[6], [2, 3]])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert len(inner.calls) == NEW == len(calls) and out.shape == (2, 5 + NEW)


def test_at_most_one_synchronise_per_step_with_an_eos_id(monkeypatch):
    """The same loop with one eos id under "warn": between two consecutive calls of the step function -- one iteration's beam block -- at
    most one synchronising call is reported: the read of the 4-byte all_done flag."""
    from otter_amd import generation as G

    if not _sync_mode_detects("warn"):
        pytest.skip("this torch build does not warn on every .item() in sync debug mode 'warn': the mode cannot count synchronises")
    calls = _count_kernel(monkeypatch)
    monkeypatch.setenv("OTTER_HIP_BEAM", "1")
    NEW = 8
    inner = _toy_step(50432)
    prev = torch.cuda.get_sync_debug_mode()
    marks = []
    prompt = torch.tensor([[1, 2, 3, 1, 2], [9, 8, 9, 8, 9]], device=DEV)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")

        def step(ids, mask, past, beam_idx):
            marks.append(len(w))
            out = inner(ids, mask, past, beam_idx)
            if len(inner.calls) == 1:
                torch.cuda.set_sync_debug_mode("warn")
            return out

        try:
            G.generate_tokens(step, prompt, None, num_beams=3, max_new_tokens=NEW, eos_token_id=4, pad_token_id=0, no_repeat_ngram_size=3,
                              min_new_tokens=NEW)
        finally:
            torch.cuda.set_sync_debug_mode(prev)
    assert len(inner.calls) == NEW == len(calls)
    per_step = [b - a for a, b in zip(marks[1:-1], marks[2:])]                 # (the first interval holds the set-up's copies to the device)
    assert len(per_step) == NEW - 2 and max(per_step) <= 1, per_step
    assert sum(per_step) == NEW - 2                                           # and the mode did see the flag's read each time


# ---- the full hosts ------------------------------------------------------------------------------------------------------------------------

def oracle_tokens(rec, B, nb, eos, pad, L0, max_len, prompt):
    """What generate_tokens returns for the recorded logp of a run under the tie rule of include/otter_hip.h: the oracle's steps, then the
    loop's own finalize (length_penalty 1, early_stopping False, one returned sequence per sentence)."""
    from otter_amd import generation as G

    orc = Oracle(B, nb, eos, pad, L0, max_len, 1.0, False)
    scores = torch.zeros(B, nb)
    scores[:, 1:] = -1e9
    scores, ids = scores.view(-1), prompt.cpu().repeat_interleave(nb, dim=0)
    for logp in rec:
        scores, _, _, ids = orc.step(logp, scores, ids)
    bs = scores.tolist()
    for b in range(B):
        if not orc.done[b]:
            for j in range(nb):
                orc.hyps[b].add(ids[b * nb + j], bs[b * nb + j], ids.shape[1] - L0)
    return G._pick_best([h.beams for h in orc.hyps], 1, max_len, pad, eos, "cpu")


def _host_ab(monkeypatch, gen, B, nb, L0, new, prompt):
    """One generate() call per switch on a full host (eos_token_id=-1: eos list [-1], pad -1, every call runs its full length).  Checked:
    ops.beam_step runs once per step with the switch on and never with it off; the GraphDecodeStep counts (steps, captures, replays) are the
    same; the device path's tokens are the oracle's for the device path's own logp at EVERY step; and against the host path: with no tie
    among the host path's top n_cand + 1 sums at any step the tokens are equal, otherwise the two searches are compared up to the first
    step s that has one -- the processed logp of steps 0..s, which the decisions of steps < s determine, are bit-equal -- because
    torch.topk promises no order among equal sums.  Returns (first tie step or None, the counts)."""
    from otter_amd.graph_decode import GraphDecodeStep

    calls = _count_kernel(monkeypatch)
    rec = _record_logp(monkeypatch)
    counts = []
    release = GraphDecodeStep.release

    def spy_release(self):
        counts.append((self.steps, self.captures, self.replays, self.use_graph))
        return release(self)

    monkeypatch.setattr(GraphDecodeStep, "release", spy_release)
    out, recs = {}, {}
    for switch in ("0", "1"):
        monkeypatch.setenv("OTTER_HIP_BEAM", switch)
        del rec[:]
        n = len(calls)
        out[switch] = gen().cpu()
        recs[switch] = list(rec)
        assert len(rec) == new and len(calls) - n == (new if switch == "1" else 0)
    assert counts[0] == counts[1] == (new - 1, 1, new - 3, True), counts
    assert out["1"].shape == out["0"].shape == (B, L0 + new)
    assert torch.equal(out["1"], oracle_tokens(recs["1"], B, nb, [-1], -1, L0, L0 + new, prompt))
    tie = first_tie_step(recs["0"], B, nb, [-1], -1, L0, L0 + new, 1.0, False, prompt)
    if tie is None:
        assert torch.equal(out["0"], out["1"]), (out["0"][:, L0:].tolist(), out["1"][:, L0:].tolist())
    else:
        for s in range(tie + 1):
            assert torch.equal(recs["0"][s], recs["1"][s]), "the paths part at step %d, before the host path's first tie at step %d" % (s, tie)
    return tie, counts


def test_mpt_host_static_media_graph_beams3(monkeypatch):
    """The 2-layer full-width MPT host, cache_implementation="static", cross_attention_cache=True, graph_decode=True, num_beams=3, 12 new
    tokens (`_host_ab` states what is compared).  No seed gives a tie-free run on this bf16 model: its logits are bf16 numbers, and two of the
    top seven of a sentence are equal at step 0 for seeds 99-102 (and for every seed tried with the embedding scaled by 4 and by 16).  Seed
    103 has its first tie at step 2, so steps 0-2 are what is compared against the host path here."""
    from tests.test_gpu_media_cache import _build

    model, bench = _build("mpt")
    try:
        B, P_LEN, NEW = 2, 40, 12
        vx, ids, mask, _, _ = bench.synth_batch(model, B, P_LEN, DEV, seed=103, frames=1)
        mask[1, :5] = 0

        def gen():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return model.generate(vision_x=vx.to(torch.bfloat16), lang_x=ids, attention_mask=mask, max_new_tokens=NEW, eos_token_id=-1,
                                      cache_implementation="static", cross_attention_cache=True, graph_decode=True, num_beams=3)

        tie, _ = _host_ab(monkeypatch, gen, B, 3, P_LEN, NEW, ids)
        assert tie is None or tie >= 1, "the host path ties at step 0: nothing of it can be compared"
    finally:
        del model
        gc.collect()
        torch.cuda.empty_cache()


def test_fuyu_host_static_cache_graph_beams3(monkeypatch):
    """The 2-layer full-width Persimmon host (int8 decoder, the lm_head scaled by 8 as in the existing static-cache tests) with a
    StaticKVCache object and graph_decode=True, num_beams=3, 12 new tokens: the same checks.  The host path's first tie is at step 2."""
    from transformers import FuyuConfig

    from otter_amd.fuyu import FuyuForCausalLM
    from otter_amd.kv_cache import StaticKVCache
    from tests.test_gpu_fuyu_static_cache import B, NEW, P_LEN, VOCAB, batch

    text = dict(model_type="persimmon", vocab_size=VOCAB, hidden_size=4096, intermediate_size=16384, num_hidden_layers=2, num_attention_heads=64,
                max_position_embeddings=4096, qk_layernorm=True, partial_rotary_factor=0.5, hidden_act="relu2", layer_norm_eps=1e-5,
                rope_theta=25000.0, tie_word_embeddings=False)
    cfg = FuyuConfig(vocab_size=VOCAB, hidden_size=4096, intermediate_size=16384, num_hidden_layers=2, num_attention_heads=64, patch_size=30,
                     num_channels=3, max_position_embeddings=4096, image_size=300, text_config=text, tie_word_embeddings=False)
    torch.manual_seed(41)
    with torch.device(DEV):
        model = FuyuForCausalLM(cfg)
    model = model.to(torch.bfloat16).eval()
    with torch.no_grad():
        model.language_model.lm_head.weight.mul_(8.0)
    assert model.quantize_decoder_int8()["replaced"] > 0
    cache = None
    try:
        ids, mask, patches, idx = batch()
        cache = StaticKVCache.for_model(model, rows=B * 3, max_len=P_LEN + NEW)

        def gen():
            cache.reset()
            return model.generate(input_ids=ids, attention_mask=mask, image_patches=patches, image_patches_indices=idx, max_new_tokens=NEW,
                                  eos_token_id=-1, past_key_values=cache, graph_decode=True, num_beams=3)

        tie, _ = _host_ab(monkeypatch, gen, B, 3, P_LEN, NEW, ids)
        assert tie is None or tie >= 1, "the host path ties at step 0: nothing of it can be compared"
    finally:
        del model, cache
        gc.collect()
        torch.cuda.empty_cache()
