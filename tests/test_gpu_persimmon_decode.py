"""The cached OtterHD / Fuyu-8B (Persimmon) decode step on HIP (csrc/persimmon_decode.hip, otter_amd/fuyu.py's decode mode): the kernel
against a numpy oracle through ops / ctypes, and the host's cached generation against full re-forwards and against the plain path
(OTTER_FUYU_HIP_DECODE=0); the left-padded prompt pass on the flash kernel."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import synth
from tests import _golden as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 3e-2


def bf16r(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def oracle(qkv, gq, bq, gk, bk, cos_row, sin_row, kp, vp, kvalid, rot, eps, scale):
    """fp32 numpy restatement of one cached step on bf16-valued inputs: (o [B,H,64], k' [B,H,64] bf16-rounded)."""
    x = qkv[:, :, :2].astype(np.float32)                                      # [B,H,2,64]
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    g = np.stack([gq, gk])[None, None]
    bb = np.stack([bq, bk])[None, None]
    y = (x - mean) / np.sqrt(var + eps) * g + bb
    h = rot // 2
    y1, y2 = y[..., :h].copy(), y[..., h:rot].copy()
    y[..., :h] = y1 * cos_row[:h] - y2 * sin_row[:h]
    y[..., h:rot] = y2 * cos_row[h:rot] + y1 * sin_row[h:rot]
    y = bf16r(y)
    q, k = y[:, :, 0], y[:, :, 1]
    Kc = np.concatenate([kp, k[:, :, None]], 2)                              # [B,H,Sk,64]
    Vc = np.concatenate([vp, qkv[:, :, 2][:, :, None]], 2)
    s = np.einsum("bhd,bhkd->bhk", q, Kc) * scale
    if kvalid is not None:
        s = np.where(kvalid[:, None, :] != 0, s, -np.inf)
    m = s.max(-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    p = np.exp(s - m)
    l = p.sum(-1, keepdims=True)
    o = np.einsum("bhk,bhkd->bhd", p, Vc) / np.where(l > 0, l, 1.0)
    return o, k


def make_past(layout, B, H, S, gen):
    """bf16 [B,H,S,64] K and V in one of the three layouts the decode step meets."""
    if layout == "contiguous":
        k = torch.randn(B, H, S, 64, generator=gen).bfloat16().to(DEV)
        v = torch.randn(B, H, S, 64, generator=gen).bfloat16().to(DEV)
    elif layout == "prefill_view":          # functional.persimmon_attention(..., want_kv=True): k [B,S,H,64] and v inside qkv, transposed
        k = torch.randn(B, S, H, 64, generator=gen).bfloat16().to(DEV).transpose(1, 2)
        v = torch.randn(B, S, H, 3, 64, generator=gen).bfloat16().to(DEV)[:, :, :, 2].transpose(1, 2)
    else:                                   # beam reordering: index_select of a bigger batch
        idx = torch.arange(B, device=DEV).flip(0)
        k = torch.randn(B + 1, H, S, 64, generator=gen).bfloat16().to(DEV).index_select(0, idx)
        v = torch.randn(B + 1, H, S, 64, generator=gen).bfloat16().to(DEV).index_select(0, idx)
    return k, v


def run_case(B, H, S_past, layout, rot, masked, seed):
    from otter_amd import ops

    gen = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B, H, 3, 64, generator=gen) * 2 + 0.3).bfloat16().to(DEV)
    gq, gk = (1 + 0.3 * torch.randn(64, generator=gen)).to(DEV), (1 + 0.3 * torch.randn(64, generator=gen)).to(DEV)
    bq, bk = (0.1 * torch.randn(64, generator=gen)).to(DEV), (0.1 * torch.randn(64, generator=gen)).to(DEV)
    inv = 1.0 / (25000.0 ** (torch.arange(0, rot, 2, dtype=torch.float32) / rot))
    fr = float(S_past) * inv
    emb = torch.cat([fr, fr])
    cos_row, sin_row = emb.cos().to(DEV), emb.sin().to(DEV)
    kp, vp = make_past(layout, B, H, S_past, gen)
    kvalid = None
    if masked:                              # left padding of 0 / 5 / 11 ... keys per row
        kvalid = torch.ones(B, S_past + 1, dtype=torch.uint8)
        for b in range(B):
            kvalid[b, :min(5 * b + (b > 1), S_past)] = 0
        kvalid = kvalid.to(DEV)
    kp0, vp0 = kp.clone(), vp.clone()
    scale, eps = 0.125, 1e-5
    o, kn, vn = ops.persimmon_decode_attn(qkv, gq, bq, gk, bk, cos_row, sin_row, kp, vp, kvalid, rot, eps, scale)
    torch.cuda.synchronize()
    assert torch.equal(kp, kp0) and torch.equal(vp, vp0)                     # the past is never written
    assert kn.shape == (B, H, S_past + 1, 64) and vn.shape == kn.shape and o.shape == (B, H * 64)
    assert torch.equal(kn[:, :, :S_past], kp) and torch.equal(vn[:, :, :S_past], vp)   # copied rows: bit-equal
    assert torch.equal(vn[:, :, S_past], qkv[:, :, 2])                     # the new value: raw
    f = lambda t: t.float().cpu().numpy()
    o_ref, k_ref = oracle(f(qkv), f(gq), f(bq), f(gk), f(bk), f(cos_row), f(sin_row), f(kp), f(vp),
                          None if kvalid is None else kvalid.cpu().numpy(), rot, eps, scale)
    assert not torch.isnan(o).any()
    assert rel(f(kn[:, :, S_past]), k_ref) < 1e-2
    assert rel(f(o).reshape(B, H, 64), o_ref) < 1e-2


@pytest.mark.parametrize("layout", ["contiguous", "prefill_view", "index_select"])
@pytest.mark.parametrize("S_past", [1, 17, 1350, 16383])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H", [2, 64])
def test_kernel_against_numpy_oracle(H, B, S_past, layout):
    """o to 1e-2 relative-to-max and the new k' to 1e-2 against the oracle on the same bf16 inputs; the copied past rows and v bit-equal;
    the past untouched.  rot 32 without a mask, rot 64 with left-padded key_valid (S_past 1350 / 16383 take the split-key form)."""
    seed = H * 1000 + B * 100 + S_past % 97
    run_case(B, H, S_past, layout, 32, False, seed)
    run_case(B, H, S_past, layout, 64, True, seed + 1)


@pytest.mark.parametrize("S_past", [17, 1350])
def test_fully_masked_row_gives_zero_not_nan(S_past):
    from otter_amd import ops

    B, H = 2, 4
    gen = torch.Generator().manual_seed(7)
    qkv = torch.randn(B, H, 3, 64, generator=gen).bfloat16().to(DEV)
    ones, zeros = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    cs = torch.ones(32, device=DEV)
    kp, vp = make_past("contiguous", B, H, S_past, gen)
    kvalid = torch.ones(B, S_past + 1, dtype=torch.uint8, device=DEV)
    kvalid[1] = 0
    o, kn, vn = ops.persimmon_decode_attn(qkv, ones, zeros, ones, zeros, cs, cs * 0, kp, vp, kvalid, 32, 1e-5, 0.125)
    torch.cuda.synchronize()
    assert not torch.isnan(o).any() and not torch.isnan(kn).any()
    assert torch.equal(o[1], torch.zeros_like(o[1]))
    assert o[0].float().abs().max() > 0


def test_ops_wrapper_validates_before_launch():
    from otter_amd import _capi, ops

    qkv = torch.zeros(1, 2, 3, 64, dtype=torch.bfloat16, device=DEV)
    g = torch.ones(64, device=DEV)
    cs = torch.ones(32, device=DEV)
    kp = torch.zeros(1, 2, 5, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(_capi.OtterHipError, match="unit dim stride"):
        ops.persimmon_decode_attn(qkv, g, g, g, g, cs, cs, kp.transpose(2, 3).contiguous().transpose(2, 3), kp, None, 32, 1e-5, 0.125)
    with pytest.raises(_capi.OtterHipError, match="rot"):
        ops.persimmon_decode_attn(qkv, g, g, g, g, cs, cs, kp, kp, None, 24, 1e-5, 0.125)
    with pytest.raises(_capi.OtterHipError, match="key_valid"):
        ops.persimmon_decode_attn(qkv, g, g, g, g, cs, cs, kp, kp, torch.ones(1, 5, dtype=torch.uint8, device=DEV), 32, 1e-5, 0.125)


# ---------------------------------------------------------------------------------------------------------------------------------------
# host: otter_amd/fuyu.py
# ---------------------------------------------------------------------------------------------------------------------------------------


def tiny_bf16_fuyu():
    from oracle.gen_golden_fuyu import SEED, tiny_fuyu_config
    from otter_amd.fuyu import FuyuForCausalLM

    m = G.meta()["fuyu_tiny"]
    model = FuyuForCausalLM(tiny_fuyu_config())
    sd = synth.state_dict_for(SEED, {k: tuple(v) for k, v in m["shapes"].items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.to(DEV).to(torch.bfloat16).eval()


class Spy:
    def __init__(self, monkeypatch, module, name):
        self.n, self.kwargs = 0, []
        orig = getattr(module, name)

        def f(*a, **k):
            self.n += 1
            self.kwargs.append(k)
            return orig(*a, **k)

        monkeypatch.setattr(module, name, f)


def cached_steps(model, ids, P, **prompt_kw):
    """prompt pass over ids[:, :P], then one cached step per remaining token: per-step logits [B, 1 + n, V] (the prompt's last)."""
    out = model(input_ids=ids[:, :P], use_cache=True, **prompt_kw)
    past, steps = out.past_key_values, [out.logits[:, -1:].float()]
    mask = prompt_kw.get("attention_mask")
    for k in range(P, ids.shape[1]):
        kw = {}
        if mask is not None:
            mask = torch.cat([mask, mask.new_ones(mask.shape[0], 1)], 1)
            kw["attention_mask"] = mask
        out = model(input_ids=ids[:, k:k + 1], past_key_values=past, use_cache=True, **kw)
        past = out.past_key_values
        steps.append(out.logits.float())
    return torch.cat(steps, 1), past


def test_tiny_fuyu_cached_steps_match_full_forward(monkeypatch):
    """Prompt + 6 cached steps (bf16 weights) against the full bf16 re-forward of the same sequence and against the plain decode path;
    every step of every layer runs the new kernel, and SDPA is not called while decoding."""
    from oracle.gen_golden_fuyu import tiny_fuyu_batch
    from otter_amd import ops

    model = tiny_bf16_fuyu()
    ids, patches, idx, _, _ = tiny_fuyu_batch()
    P, n_layers = 14, len(model.language_model.model.layers)
    ids_t, pt, idx_t = (torch.from_numpy(a).to(DEV) for a in (ids, patches, idx))
    with torch.no_grad():
        full = model(input_ids=ids_t, image_patches=pt, image_patches_indices=idx_t, use_cache=False).logits.float()[:, P - 1:]
        dec = Spy(monkeypatch, ops, "persimmon_decode_attn")
        sdpa = Spy(monkeypatch, F, "scaled_dot_product_attention")
        inc, past = cached_steps(model, ids_t, P, image_patches=pt, image_patches_indices=idx_t[:, :P])
        assert dec.n == n_layers * (ids.shape[1] - P) and sdpa.n == 0
        assert all(k.shape == (2, 2, ids.shape[1], 64) and k.dtype == torch.bfloat16 for layer in past for k in layer)
        monkeypatch.setenv("OTTER_FUYU_HIP_DECODE", "0")
        plain, _ = cached_steps(model, ids_t, P, image_patches=pt, image_patches_indices=idx_t[:, :P])
        assert dec.n == n_layers * (ids.shape[1] - P) and sdpa.n > 0                # the switch restores the plain path
    assert not torch.isnan(inc).any()
    assert rel(inc.cpu(), full.cpu()) < TOL
    assert rel(inc.cpu(), plain.cpu()) < TOL


def first_divergence_margin_ok(model, ids_hip, ids_plain, L0, fwd_kw):
    """Where the HIP and plain ids differ, the plain path's top-2 logit margin at the first differing step must be within 2 x TOL
    (relative to the largest logit): a near-tie, not an error."""
    for b in range(ids_plain.shape[0]):
        diff = (ids_hip[b] != ids_plain[b]).nonzero()
        if len(diff) == 0:
            continue
        t = int(diff[0])
        assert t >= L0
        with torch.no_grad():
            lg = model(input_ids=ids_plain[b:b + 1, :t], use_cache=False, **fwd_kw(b, t)).logits[0, -1].float()
        top = lg.topk(2).values
        assert float(top[0] - top[1]) <= 2 * TOL * float(lg.abs().max()), (b, t)


@pytest.mark.parametrize("num_beams", [1, 2])
def test_tiny_fuyu_generate_takes_the_decode_kernel(monkeypatch, num_beams):
    from oracle.gen_golden_fuyu import tiny_fuyu_batch
    from otter_amd import ops

    model = tiny_bf16_fuyu()
    ids, patches, idx, _, _ = tiny_fuyu_batch()
    P = 14
    t = lambda a: torch.from_numpy(a).to(DEV)
    kw = dict(input_ids=t(ids[:, :P]), image_patches=t(patches), image_patches_indices=t(idx[:, :P]), max_new_tokens=8, use_cache=True,
              eos_token_id=-1, num_beams=num_beams)
    dec = Spy(monkeypatch, ops, "persimmon_decode_attn")
    got = model.generate(**kw)
    assert dec.n > 0
    n = dec.n
    monkeypatch.setenv("OTTER_FUYU_HIP_DECODE", "0")
    ref = model.generate(**kw)
    assert dec.n == n
    assert got.shape == ref.shape

    def fwd_kw(b, tt):
        ix = torch.cat([t(idx[b:b + 1, :P]), torch.full((1, tt - P), -1, dtype=torch.int64, device=DEV)], 1)
        return dict(image_patches=t(patches[b:b + 1]), image_patches_indices=ix)

    first_divergence_margin_ok(model, got, ref, P, fwd_kw)


def test_left_padded_batch_prompt_and_decode(monkeypatch):
    """B = 3 with 0 / 3 / 7 pad tokens on the left: the prompt pass runs the flash kernel with key_valid, the cached steps the new kernel;
    valid-position logits match the all-plain path (OTTER_NO_FLASH=1) within 3e-2, and nothing is NaN."""
    from otter_amd import functional as OF
    from otter_amd import ops

    model = tiny_bf16_fuyu()
    g = torch.Generator().manual_seed(21)
    B, S, n = 3, 24, 6
    ids = torch.randint(3, 120, (B, S + n), generator=g).to(DEV)
    mask = torch.ones(B, S, dtype=torch.int64, device=DEV)
    for b, p in enumerate((0, 3, 7)):
        mask[b, :p] = 0
    att = Spy(monkeypatch, OF, "persimmon_attention")
    dec = Spy(monkeypatch, ops, "persimmon_decode_attn")
    with torch.no_grad():
        hip, past = cached_steps(model, ids, S, attention_mask=mask)
        prompt_hip = model(input_ids=ids[:, :S], attention_mask=mask, use_cache=True).logits.float()
    n_layers = len(model.language_model.model.layers)
    assert att.n == 2 * n_layers and all(k.get("key_valid") is not None for k in att.kwargs)
    assert dec.n == n_layers * n
    assert not torch.isnan(hip).any() and not torch.isnan(prompt_hip).any()
    assert not any(torch.isnan(x).any() for layer in past for x in layer)
    monkeypatch.setenv("OTTER_NO_FLASH", "1")
    with torch.no_grad():
        plain, _ = cached_steps(model, ids, S, attention_mask=mask)
        prompt_plain = model(input_ids=ids[:, :S], attention_mask=mask, use_cache=True).logits.float()
    assert att.n == 2 * n_layers and dec.n == n_layers * n
    valid = mask.bool()
    assert rel(prompt_hip[valid].cpu(), prompt_plain[valid].cpu()) < TOL
    assert rel(hip.cpu(), plain.cpu()) < TOL


def test_full_width_prompt_and_decode_against_plain(monkeypatch):
    """Fuyu-8B width (hidden 4096, 64 heads x 64, FFN 16384), 2 layers, random init, bf16: a 1350-token prompt + 8 cached steps on the
    new kernel against the plain decode path, within 3e-2."""
    from transformers import PersimmonConfig

    from otter_amd import ops
    from otter_amd.fuyu import PersimmonForCausalLM

    cfg = PersimmonConfig(vocab_size=1024, hidden_size=4096, intermediate_size=16384, num_hidden_layers=2, num_attention_heads=64,
                          max_position_embeddings=4096, qk_layernorm=True, partial_rotary_factor=0.5, hidden_act="relu2", layer_norm_eps=1e-5,
                          rope_theta=25000.0, tie_word_embeddings=False)
    torch.manual_seed(41)
    model = PersimmonForCausalLM(cfg).to(DEV).to(torch.bfloat16).eval()
    g = torch.Generator().manual_seed(42)
    P, n = 1350, 8
    ids = torch.randint(0, 1024, (1, P + n), generator=g).to(DEV)
    dec = Spy(monkeypatch, ops, "persimmon_decode_attn")
    with torch.no_grad():
        hip, _ = cached_steps(model, ids, P)
        assert dec.n == 2 * n
        monkeypatch.setenv("OTTER_FUYU_HIP_DECODE", "0")
        plain, _ = cached_steps(model, ids, P)
        assert dec.n == 2 * n
    assert not torch.isnan(hip).any()
    assert rel(hip.cpu(), plain.cpu()) < TOL
