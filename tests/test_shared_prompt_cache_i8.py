"""StaticKVCache over an int8 cache with a shared prompt, on the CPU: when `uses_shared_i8_kernel` holds, and that `attend` then takes the
grouped int8 op (csrc/decode_cache_shared_i8.hip) in both of its modes -- with the kernel conditions and the ops replaced by stand-ins."""
import pytest
import torch

from otter_amd import kv_cache, ops
from otter_amd.kv_cache import SHARED_I8_KERNEL_MIN_KEYS, StaticKVCache

L, H, D, MAX_LEN = 2, 2, 8, 16
B, G, S = 2, 3, 5
ROWS = B * G


def _shared(kv_dtype="int8", seed=0):
    gen = torch.Generator().manual_seed(seed)
    c = StaticKVCache(L, ROWS, H, D, MAX_LEN, "cpu", torch.float32, kv_dtype=kv_dtype)
    c.share_prompt(G)
    with torch.no_grad():
        c.check_step(B, S)
    for i in range(L):
        c.fill(i, torch.randn(B, H, S, D, generator=gen), torch.randn(B, H, S, D, generator=gen))
    c.length = S
    return c, gen


@pytest.fixture
def kernel_everywhere(monkeypatch):
    monkeypatch.setattr(StaticKVCache, "uses_kernel", lambda self, q, n_kv: True)
    monkeypatch.delenv("OTTER_SHARED_PREFIX", raising=False)
    monkeypatch.delenv("OTTER_SHARED_PREFIX_I8", raising=False)


def test_the_predicate(monkeypatch):
    c, gen = _shared()
    q = torch.randn(ROWS, H, D, generator=gen)
    assert not c.uses_shared_i8_kernel(q, H) and not c.uses_shared_kernel(q, H)     # fp32 on the CPU: the restatement
    monkeypatch.setattr(StaticKVCache, "uses_kernel", lambda self, q, n_kv: True)
    monkeypatch.delenv("OTTER_SHARED_PREFIX", raising=False)
    monkeypatch.delenv("OTTER_SHARED_PREFIX_I8", raising=False)
    never = lambda: not c.uses_shared_kernel(q, H)                   # the bf16 kernel's predicate stays false on the int8 cache throughout
    at = (SHARED_I8_KERNEL_MIN_KEYS + B - 1) // B                    # B sentences x `at` shared keys: the first length at the threshold
    assert SHARED_I8_KERNEL_MIN_KEYS > B * S and at > 1

    bf16, _ = _shared(kv_dtype=None)
    bf16.shared_len = at
    assert not bf16.uses_shared_i8_kernel(q, H)                      # a bf16 cache
    assert not c.uses_shared_i8_kernel(q, H) and never()             # 2 sentences x 5 shared keys: below the threshold
    c.shared_len = at - 1
    assert not c.uses_shared_i8_kernel(q, H) and never()
    c.shared_len = at
    assert c.uses_shared_i8_kernel(q, H) and never()                 # at it
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "0")
    assert not c.uses_shared_i8_kernel(q, H) and never()             # the lever of every grouped kernel
    monkeypatch.delenv("OTTER_SHARED_PREFIX")
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "0")
    assert not c.uses_shared_i8_kernel(q, H) and never()             # this kernel's own lever
    c.shared_len = S
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "1")
    assert c.uses_shared_i8_kernel(q, H) and never()                 # forced below the threshold
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "0")
    assert not c.uses_shared_i8_kernel(q, H) and never()             # "0" there wins over "1" here
    monkeypatch.delenv("OTTER_SHARED_PREFIX_I8")
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "1")
    assert not c.uses_shared_i8_kernel(q, H) and never()             # OTTER_SHARED_PREFIX=1 alone does not force it
    c.shared_len = at
    assert c.uses_shared_i8_kernel(q, H) and never()                 # (nor does it switch it off)
    monkeypatch.delenv("OTTER_SHARED_PREFIX")
    c.group = 7
    assert not c.uses_shared_i8_kernel(q, H) and never()             # a group size the kernel is not built for
    c.group, c.shared_len = G, 0
    assert not c.uses_shared_i8_kernel(q, H) and never()
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "1")
    assert not c.uses_shared_i8_kernel(q, H) and never()             # nothing shared: the lever forces nothing
    c.shared_len, c.group = S, 1
    assert not c.uses_shared_i8_kernel(q, H) and never()


def test_the_group_sizes_are_the_ops():
    assert ops.DECODE_CACHED_SHARED_I8_GROUPS == (2, 3, 4, 5, 6)
    assert kv_cache.SHARED_I8_KERNEL_MIN_KEYS >= 1


class Spy:
    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kw):
        self.calls.append((args, kw))
        return "o"


@pytest.mark.parametrize("replay", [False, True], ids=["scalar", "replay"])
def test_attend_takes_the_grouped_int8_op(monkeypatch, kernel_everywhere, replay):
    c, gen = _shared()
    if replay:
        c.enable_replay(beams=True)
    q, k, v = (torch.randn(ROWS, H, D, generator=gen) for _ in range(3))
    grouped, table = Spy(), Spy()
    suffix = "_dyn" if replay else ""
    monkeypatch.setattr(ops, "decode_attn_cached_shared_i8" + suffix, grouped)
    monkeypatch.setattr(ops, "decode_attn_cached_i8" + suffix, table)
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "1")
    assert c.attend(1, q, k, v, 0.5, slopes="slopes") == "o"
    assert not table.calls and len(grouped.calls) == 1
    args, kw = grouped.calls[0]
    assert args[:3] == (q, k, v)
    assert [a.data_ptr() for a in args[3:7]] == [t[1].data_ptr() for t in (c.k, c.v, c.k_scale, c.v_scale)]
    assert (args[7] is c.pos_dev if replay else args[7] == S) and args[8:] == (0.5, G, S)        # ..., pos, scale, group, shared_len
    assert kw["src"] is c.src and kw["slopes"] == "slopes" and kw["key_valid"] is (c.valid if replay else None)
    assert set(kw) == ({"cos_table", "sin_table", "src", "key_valid", "slopes"} if replay else {"cos", "sin", "src", "key_valid", "slopes"})

    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "0")                # the lever: the existing int8 op, through the table
    assert c.attend(1, q, k, v, 0.5) == "o"
    assert len(grouped.calls) == 1 and len(table.calls) == 1
    args, kw = table.calls[0]
    assert (args[7] is c.pos_dev if replay else args[7] == S) and args[8:] == (0.5,) and kw["src"] is c.src

    monkeypatch.delenv("OTTER_SHARED_PREFIX_I8")                     # unset: below the threshold the table path, from it on the grouped op
    assert c.attend(1, q, k, v, 0.5) == "o"
    assert len(grouped.calls) == 1 and len(table.calls) == 2
    monkeypatch.setattr(kv_cache, "SHARED_I8_KERNEL_MIN_KEYS", B * S)
    assert c.attend(1, q, k, v, 0.5) == "o"
    assert len(grouped.calls) == 2 and len(table.calls) == 2


def test_a_bf16_cache_never_takes_it(monkeypatch, kernel_everywhere):
    c, gen = _shared(kv_dtype=None)
    q, k, v = (torch.randn(ROWS, H, D, generator=gen) for _ in range(3))
    grouped, bf16_grouped = Spy(), Spy()
    monkeypatch.setattr(ops, "decode_attn_cached_shared_i8", grouped)
    monkeypatch.setattr(ops, "decode_attn_cached_shared", bf16_grouped)
    monkeypatch.setenv("OTTER_SHARED_PREFIX_I8", "1")
    monkeypatch.setenv("OTTER_SHARED_PREFIX", "1")
    c.attend(0, q, k, v, 0.5)
    assert not grouped.calls and len(bf16_grouped.calls) == 1
