"""CPU, fp32, tiny MPT and LLaMA Otter hosts: `OtterForConditionalGeneration.score_candidates` -- rank classification over a cached prompt.

THE ORACLE is the project's re-forward: for every (sentence b, candidate c) one uncached forward over prompt + candidate, log-softmax in fp32,
the candidate's tokens gathered at positions P-1 .. P+len-2 (the reference's `no_kv_caching` branch, evaluate.py:1049-1176).

THE TOLERANCE is not a number fixed in advance.  A user of the code as it stood had one cached way to get these numbers: the prompt pass into
a StaticKVCache + MediaCache and then teacher-forced one-token steps (`cache_implementation="static"` + `cross_attention_cache=True`, driven
through the hosts).  Its distance d_steps from the oracle is measured here, per case, and `score_candidates` is allowed 2 x d_steps -- the
project's standing allowance for a second rounding order -- with a floor of 1e-6 of the largest |logit| of the oracle.  Measured (max over
the real tokens, this file's cases, fp32 on the CPU):

    host   case            d_steps     d_score     floor (1e-6 max|logit|)
    mpt    ragged_padded   1.14e-05    1.53e-05    6.47e-05
    mpt    shared_list     7.63e-06    7.63e-06    6.09e-05
    llama  ragged_padded   4.77e-07    4.77e-07    5.71e-07
    llama  shared_list     4.77e-07    4.77e-07    5.57e-07
    int8 decoder (gated_blocks, lm_head) against its fake-quantised twin, d_steps / d_score / floor:
           mpt 1.14e-05 / 1.14e-05 / 6.74e-05, llama 4.77e-07 / 4.77e-07 / 5.50e-07

(both distances are one or two fp32 roundings of the log-probabilities -- of magnitude 70 on the tiny MPT, 5 on the tiny LLaMA.)

The gated blocks and the fusion modules of the uncached forward get their CPU arithmetic from tests/_cpu_backend.py, and the int8 cases from
the backend of tests/test_quant_gated_host.py, as in those files."""
import pytest
import torch

from otter_amd.kv_cache import StaticKVCache, cache_geometry
from otter_amd.media_cache import MediaCache
from tests._cpu_backend import oracle_backend
from tests.test_media_cache import MEDIA, _batch, _model
from tests.test_quant_gated_host import _backend, _model as _quant_base, _twin

KINDS = pytest.mark.parametrize("llama", [False, True], ids=["mpt", "llama"])
P = 6


def _prompt(pads, B=3):
    vx, ids, mask = _batch(B, pads)
    return vx, ids[:, :P].contiguous(), (mask[:, :P].contiguous() if mask is not None else None)


def _candidates(B, C, T, seed, shared=False, full=False):
    """Right-padded candidates with ragged lengths 1..T (`full`: all T); candidate 0 has all T tokens.  Padding holds -1: it must not be read."""
    g = torch.Generator().manual_seed(seed)
    shape = (C, T) if shared else (B, C, T)
    cand = torch.randint(1, 100, shape, generator=g)
    lens = torch.full(shape[:-1], T) if full else torch.randint(1, T + 1, shape[:-1], generator=g)
    lens[..., 0] = T
    cmask = torch.arange(T).expand(shape) < lens.unsqueeze(-1)
    return torch.where(cmask, cand, torch.full_like(cand, -1)), cmask


def _per_sentence(B, cand, cmask):
    return (cand.unsqueeze(0).expand(B, -1, -1), cmask.unsqueeze(0).expand(B, -1, -1)) if cand.dim() == 2 else (cand, cmask)


def _oracle(model, vx, ids, mask, cand, cmask):
    """(token log-probabilities [B, C, T], 0 on padding; the largest |logit| seen)."""
    B, C, T = cand.shape
    ref, top = torch.zeros(B, C, T), 0.0
    for b in range(B):
        for c in range(C):
            L = int(cmask[b, c].sum())
            full = torch.cat([ids[b], cand[b, c, :L]])[None]
            fm = torch.cat([mask[b], torch.ones(L, dtype=mask.dtype)])[None] if mask is not None else None
            logits = model(vision_x=vx[b:b + 1], lang_x=full, attention_mask=fm, use_cache=False).logits[0].float()
            top = max(top, float(logits[P - 1:].abs().max()))
            ref[b, c, :L] = torch.log_softmax(logits, -1)[P - 1:P + L - 1].gather(1, cand[b, c, :L, None])[:, 0]
    return ref, top


def _cached_steps(model, vx, ids, mask, cand, cmask):
    """What the code offered before `score_candidates`: per candidate index, the prompt pass of B rows into a fresh StaticKVCache + MediaCache,
    then one teacher-forced one-token step per token."""
    B, C, T = cand.shape
    n_layers, n_kv, hd, _ = cache_geometry(model.lang_encoder.config)
    inp, tok = torch.where(cmask, cand, torch.zeros_like(cand)), torch.zeros(B, C, T)
    pick = lambda out, c, t: torch.log_softmax(out.logits[:, -1].float(), -1).gather(1, inp[:, c, t:t + 1])[:, 0]
    for c in range(C):
        past, mc = StaticKVCache(n_layers, B, n_kv, hd, P + T + 1, "cpu", torch.float32), MediaCache(B, model.media_token_id)
        out = model(vision_x=vx, lang_x=ids, attention_mask=mask, past_key_values=past, use_cache=True, clear_conditioned_layers=False, media_cache=mc)
        tok[:, c, 0] = pick(out, c, 0)
        for t in range(T - 1):
            m = torch.cat([mask, torch.ones(B, t + 1, dtype=mask.dtype)], dim=1) if mask is not None else None
            out = model(vision_x=None, lang_x=inp[:, c, t:t + 1], attention_mask=m, use_cached_vision_x=True, past_key_values=past, use_cache=True,
                        clear_conditioned_layers=False, media_cache=mc)
            tok[:, c, t + 1] = pick(out, c, t + 1)
        model.lang_encoder.clear_conditioned_layers()
    return tok * cmask


def _dist(a, ref, cmask):
    return float(((a - ref) * cmask).abs().max())


CASES = {
    "ragged_padded": dict(pads=(0, 2, 3), C=3, T=5, shared=False),       # [B, C, T] form, a left-padded batch, ragged lengths
    "shared_list": dict(pads=None, C=4, T=4, shared=True),               # [C, T] form
}
_REF = {}


def _reference(llama, case):
    """Oracle and yardstick of a case: computed once, shared, never modified."""
    if (llama, case) not in _REF:
        k = CASES[case]
        model = _model(llama)
        vx, ids, mask = _prompt(k["pads"])
        cand, cmask = _candidates(3, k["C"], k["T"], seed=17, shared=k["shared"])
        c3, m3 = _per_sentence(3, cand, cmask)
        with torch.no_grad(), oracle_backend():
            ref, top = _oracle(model, vx, ids, mask, c3, m3)
            d_steps = _dist(_cached_steps(model, vx, ids, mask, c3, m3), ref, m3)
        _REF[llama, case] = (vx, ids, mask, cand, cmask, m3, ref, top, d_steps)
    return _REF[llama, case]


@pytest.mark.parametrize("case", list(CASES))
@KINDS
def test_token_logprobs_match_the_reforward(llama, case):
    model = _model(llama)
    vx, ids, mask, cand, cmask, m3, ref, top, d_steps = _reference(llama, case)
    with torch.no_grad(), oracle_backend():
        scores, tok = model.score_candidates(vx, ids, mask, candidates=cand, candidate_mask=cmask, return_token_logprobs=True)
    d = _dist(tok, ref, m3)
    bound = max(2 * d_steps, 1e-6 * top)
    print("[score-candidates] %s %s: |score_candidates - re-forward| %.3e, cached steps %.3e, floor %.3e, ratio to bound %.2f"
          % ("llama" if llama else "mpt", case, d, d_steps, 1e-6 * top, d / bound))
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (3, CASES[case]["C"]) and tuple(tok.shape) == tuple(ref.shape)
    assert d <= bound, (d, d_steps, top)
    assert torch.equal(tok == 0, ~m3)                                     # exact zeros on padding, nothing else is zero
    assert torch.equal(scores, tok.sum(-1))
    assert float((scores - (ref * m3).sum(-1)).abs().max()) <= CASES[case]["T"] * bound
    assert not model.lang_encoder.is_conditioned()


@KINDS
def test_three_chunks_give_the_scores_of_one(llama):
    model = _model(llama)
    vx, ids, mask, cand, cmask, m3, ref, top, d_steps = _reference(llama, "ragged_padded")
    B, C, T = ref.shape
    passes = []
    lm = model.lang_encoder
    inner = lm.forward_branches
    lm.forward_branches = lambda b, *a, **k: (passes.append(tuple(b.shape)), inner(b, *a, **k))[1]
    try:
        with torch.no_grad(), oracle_backend():
            one = model.score_candidates(vx, ids, mask, candidates=cand, candidate_mask=cmask, return_token_logprobs=True)[1]
            assert len(passes) == 1 and passes[0][:2] == (B, C)
            del passes[:]
            three = model.score_candidates(vx, ids, mask, candidates=cand, candidate_mask=cmask, return_token_logprobs=True,
                                           max_rows=B * (T - 1))[1]       # one candidate per pass
    finally:
        del lm.forward_branches
    assert len(passes) == 3 and all(p[0] == B and p[1] == 1 and B * p[1] * p[2] <= B * (T - 1) for p in passes)
    bound = max(2 * d_steps, 1e-6 * top)
    assert _dist(three, ref, m3) <= bound and _dist(three, one, m3) <= bound


@KINDS
def test_one_candidate_and_one_token(llama):
    model = _model(llama)
    vx, ids, mask = _prompt((0, 2, 3))
    with torch.no_grad(), oracle_backend():
        for C, T in ((1, 4), (3, 1), (1, 1)):
            cand, cmask = _candidates(3, C, T, seed=5 + C + T, full=True)
            ref, top = _oracle(model, vx, ids, mask, cand, cmask)
            d_steps = _dist(_cached_steps(model, vx, ids, mask, cand, cmask), ref, cmask)
            lm, ran = model.lang_encoder, []
            inner = lm.forward_branches
            lm.forward_branches = lambda *a, **k: (ran.append(1), inner(*a, **k))[1]
            try:
                tok = model.score_candidates(vx, ids, mask, candidates=cand, return_token_logprobs=True)[1]      # (default mask: all real)
            finally:
                del lm.forward_branches
            assert len(ran) == (0 if T == 1 else 1)                       # T == 1 runs no branch pass
            assert _dist(tok, ref, cmask) <= max(2 * d_steps, 1e-6 * top), (C, T)


_QUANT = {}


def _quant_pair(llama):
    if llama not in _QUANT:
        model = _quant_base(llama)
        import copy

        qmodel = copy.deepcopy(model)
        qmodel.quantize_decoder_int8(gated_blocks=True, lm_head=True)
        _QUANT[llama] = (qmodel, _twin(model, qmodel)[0])
    return _QUANT[llama]


@KINDS
def test_int8_decoder_against_its_fake_quantised_twin(llama):
    """The oracle is the TWIN's re-forward (fp32 weights holding q * scale); the yardstick the quantised model's own cached steps."""
    qmodel, twin = _quant_pair(llama)
    vx, ids, mask = _prompt((0, 2, 3))
    cand, cmask = _candidates(3, 3, 4, seed=23)
    with torch.no_grad(), _backend():
        ref, top = _oracle(twin, vx, ids, mask, cand, cmask)
        d_steps = _dist(_cached_steps(qmodel, vx, ids, mask, cand, cmask), ref, cmask)
        tok = qmodel.score_candidates(vx, ids, mask, candidates=cand, candidate_mask=cmask, return_token_logprobs=True)[1]
    d = _dist(tok, ref, cmask)
    print("[score-candidates] %s int8: |score_candidates - twin re-forward| %.3e, cached steps %.3e, floor %.3e"
          % ("llama" if llama else "mpt", d, d_steps, 1e-6 * top))
    assert d <= max(2 * d_steps, 1e-6 * top), (d, d_steps, top)


@KINDS
def test_conditioning_is_cleared_after_an_exception(llama):
    model = _model(llama)
    vx, ids, mask = _prompt((0, 2, 3))
    cand, cmask = _candidates(3, 2, 3, seed=1)
    lm = model.lang_encoder

    def boom(*a, **k):
        assert lm.is_conditioned()
        raise RuntimeError("boom")

    lm.forward_branches = boom
    try:
        with torch.no_grad(), oracle_backend(), pytest.raises(RuntimeError, match="boom"):
            model.score_candidates(vx, ids, mask, candidates=cand, candidate_mask=cmask)
    finally:
        del lm.forward_branches
    assert not lm.is_conditioned()
    assert all(l.media_step is None for l in lm._get_decoder_layers())


def test_media_cache_rows_view_does_not_touch_the_cache():
    mc = MediaCache(2, MEDIA)
    mc.seen, mc.kv, mc.filled = torch.tensor([1, 0], dtype=torch.int32), [None, torch.randn(2, 4, 256)], True
    mc.T_img, mc.n, mc.heads = 1, 4, 2
    seen = mc.seen
    view, again = mc.rows_view(3), mc.rows_view(2)                        # any number of views
    assert view.rows == 6 and view.rows_per_media == 3 and view.sentences == 2 and view.kv is mc.kv and again.rows == 4
    assert torch.equal(view.seen, torch.tensor([1, 1, 1, 0, 0, 0], dtype=torch.int32))
    assert mc.seen is seen and mc.rows == 2 and mc.rows_per_media == 1
    q, got = torch.randn(6, 128), None
    got = view.attend(1, q)
    for r in range(6):                                                    # row r reads the media and the count of sentence r // 3
        q2 = torch.zeros(2, 128)
        q2[r // 3] = q[r]
        assert torch.allclose(got[r], mc.attend(1, q2)[r // 3], rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="empty"):
        MediaCache(2, MEDIA).rows_view(2)
    with pytest.raises(ValueError, match="n >= 1"):
        mc.rows_view(0)


ERRORS = {
    "media_token": (lambda c, m: (c.index_put((torch.tensor(1), torch.tensor(0), torch.tensor(1)), torch.tensor(MEDIA)), m), "media token"),
    "T_above_64": (lambda c, m: (torch.ones(3, 2, 65, dtype=torch.int64), None), "at most 64 tokens"),
    "empty_candidate": (lambda c, m: (c, m.index_put((torch.tensor(2), torch.tensor(1)), torch.tensor(False))), "without a real token"),
    "not_right_padded": (lambda c, m: (c, m.index_put((torch.tensor(0), torch.tensor(0), torch.tensor(0)), torch.tensor(False))), "right-padded"),
    "mask_shape": (lambda c, m: (c, m[:, :, :-1]), "candidate_mask must be bool"),
    "mask_dtype": (lambda c, m: (c, m.long()), "candidate_mask must be bool"),
    "sentences": (lambda c, m: (c[:2], m[:2]), "for 3 sentences"),
    "one_dimension": (lambda c, m: (c[0, 0], m[0, 0]), r"int64 \[C, T\] or \[B, C, T\]"),
    "dtype": (lambda c, m: (c.int(), m), r"int64 \[C, T\] or \[B, C, T\]"),
    "no_candidates": (lambda c, m: (c[:, :0], m[:, :0]), "C, T >= 1"),
    "outside_vocabulary": (lambda c, m: (c.index_put((torch.tensor(0), torch.tensor(0), torch.tensor(0)), torch.tensor(10 ** 6)), m), "outside the vocabulary"),
}


@pytest.mark.parametrize("case", list(ERRORS))
def test_value_errors(case):
    model = _model(False)
    vx, ids, mask = _prompt((0, 2, 3))
    cand, cmask = _candidates(3, 2, 3, seed=1, full=True)
    make, text = ERRORS[case]
    c, m = make(cand, cmask)
    with torch.no_grad(), oracle_backend(), pytest.raises(ValueError, match=text):
        model.score_candidates(vx, ids, mask, candidates=c, candidate_mask=m)
    assert not model.lang_encoder.is_conditioned()


def test_value_errors_of_the_other_arguments():
    model = _model(False)
    vx, ids, mask = _prompt((0, 2, 3))
    cand, cmask = _candidates(3, 2, 3, seed=1)
    with torch.no_grad(), oracle_backend():
        with pytest.raises(ValueError, match="max_rows >= 1"):
            model.score_candidates(vx, ids, mask, candidates=cand, candidate_mask=cmask, max_rows=0)
        with pytest.raises(ValueError, match="attention_mask must be"):
            model.score_candidates(vx, ids, mask[:, :-1], candidates=cand, candidate_mask=cmask)
        with pytest.raises(ValueError, match="lang_x must be"):
            model.score_candidates(vx, ids[0], None, candidates=cand, candidate_mask=cmask)
        long = torch.ones(3, 1, 64, dtype=torch.int64)
        with pytest.raises(ValueError, match="exceed the host's"):
            _model(True).score_candidates(vx, ids, mask, candidates=long)                 # LLaMA tiny: 64 positions, 6 + 64 > 64
