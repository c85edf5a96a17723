"""CPU: otter_decode_attn_cached_shared / _dyn (csrc/decode_cache_shared.hip) validate their arguments before anything is launched -- negative
status and a message, no GPU needed -- and so do their Python bindings, on CPU tensors over a recording stand-in for the library.  Device
pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them."""
import os
import re

import pytest
import torch

from tests import _decode_binding_cases as B

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
H, S_MAX = 2, 64
ENTRIES = ["scalar", "dyn"]


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, entry, **over):
    dyn = entry == "dyn"
    a = dict(q=P, q_rs=3 * H * 128, q_hs=128, kn=P + 2 * H * 128, kn_rs=3 * H * 128, kn_hs=128, vn=P + 4 * H * 128, vn_rs=3 * H * 128, vn_hs=128,
             cos=None, sin=None, cs_rs=0, kc=P, kc_rs=H * S_MAX * 128, kc_hs=S_MAX * 128, vc=P, vc_rs=H * S_MAX * 128, vc_hs=S_MAX * 128,
             src=None, src_rs=0, kvalid=None, kv_rs=0, slopes=None, o=P, ws=P, ws_bytes=1 << 20, N=6, H=H, pos=P if dyn else 8, S_max=S_MAX,
             head_dim=128, scale=0.0884, group=3, shared_len=5)
    a.update(over)
    fn = lib.otter_decode_attn_cached_shared_dyn if dyn else lib.otter_decode_attn_cached_shared
    return fn(a["q"], a["q_rs"], a["q_hs"], a["kn"], a["kn_rs"], a["kn_hs"], a["vn"], a["vn_rs"], a["vn_hs"], a["cos"], a["sin"], a["cs_rs"], a["kc"],
              a["kc_rs"], a["kc_hs"], a["vc"], a["vc_rs"], a["vc_hs"], a["src"], a["src_rs"], a["kvalid"], a["kv_rs"], a["slopes"], a["o"], a["ws"],
              a["ws_bytes"], a["N"], a["H"], a["pos"], a["S_max"], a["head_dim"], a["scale"], a["group"], a["shared_len"], None)


def refused(lib, entry, text, **over):
    assert call(lib, entry, **over) == -1
    msg = lib.otter_last_error()
    assert msg.startswith(b"decode_attn_cached_shared_dyn:" if entry == "dyn" else b"decode_attn_cached_shared:"), msg
    assert text in msg, msg


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers_are_rejected(lib, entry):
    for name in ["q", "kn", "vn", "kc", "vc", "o", "ws"] + (["pos"] if entry == "dyn" else []):
        refused(lib, entry, b"null pointer", **{name: None})


@pytest.mark.parametrize("entry", ENTRIES)
def test_cos_without_sin_is_rejected(lib, entry):
    refused(lib, entry, b"both be given or both be NULL", cos=P)
    refused(lib, entry, b"both be given or both be NULL", sin=P)


@pytest.mark.parametrize("entry", ENTRIES)
def test_shape_rules(lib, entry):
    refused(lib, entry, b"head_dim 64", head_dim=64)
    refused(lib, entry, b"bad shape", N=0)
    big = 65536 + 1
    refused(lib, entry, b"S_max=65537", S_max=big, kc_hs=big * 128, vc_hs=big * 128, kc_rs=H * big * 128, vc_rs=H * big * 128)


@pytest.mark.parametrize("entry", ENTRIES)
def test_group_rules(lib, entry):
    from otter_amd import ops

    assert ops.DECODE_CACHED_SHARED_GROUPS == (2, 3, 4, 5, 6)
    for group in (-3, 0, 1, 7, 8, 64):
        refused(lib, entry, b"group=%d: the kernel is built for groups of 2 to 6 rows" % group, group=group, N=64 * 3)
    refused(lib, entry, b"N=6 rows are not whole groups of 4", group=4)
    refused(lib, entry, b"N=7 rows are not whole groups of 3", N=7)


def test_shared_len_rules_of_the_scalar_entry(lib):
    for bad in (0, -1, 9, S_MAX):
        refused(lib, "scalar", b"shared_len=%d outside [1, pos] with pos=8" % bad, shared_len=bad)
    refused(lib, "scalar", b"pos=0", pos=0, shared_len=0)          # the position's own rules come first
    refused(lib, "scalar", b"beyond the cache capacity", pos=S_MAX, shared_len=1)


def test_shared_len_rules_of_the_dyn_entry(lib):
    for bad in (0, -1, S_MAX, S_MAX + 7):
        refused(lib, "dyn", b"shared_len=%d outside [1, S_max) with S_max=64" % bad, shared_len=bad)
    refused(lib, "dyn", b"pos_dev needs 4-byte alignment", pos=P + 2)


@pytest.mark.parametrize("entry", ENTRIES)
def test_alignment_and_strides(lib, entry):
    for name in ["q", "kn", "vn", "kc", "vc"]:
        refused(lib, entry, b"16-byte alignment", **{name: P + 2})
    for name in ["q_rs", "q_hs", "kn_rs", "kn_hs", "vn_rs", "vn_hs", "kc_rs", "vc_rs"]:
        refused(lib, entry, b"multiples of 8", **{name: 3 * H * 128 + 4})
    refused(lib, entry, b"overlap", kc_hs=S_MAX * 128 - 8)
    refused(lib, entry, b"overlap", vc_hs=S_MAX * 128 - 8)
    if entry == "dyn":
        refused(lib, entry, b"src one >= S_max - 1", src=P, src_rs=S_MAX - 2)
        refused(lib, entry, b"key_valid one >= S_max", kvalid=P, kv_rs=S_MAX - 1)
        refused(lib, entry, b"row stride >= 128", cos=P, sin=P, cs_rs=64)
    else:
        refused(lib, entry, b"row stride >= pos", src=P, src_rs=7)                    # pos = 8 entries per row
        refused(lib, entry, b"row stride >= pos", kvalid=P, kv_rs=8)                  # pos + 1 = 9 keys per row
        refused(lib, entry, b"non-negative", cos=P, sin=P, cs_rs=-128)


@pytest.mark.parametrize("entry", ENTRIES)
def test_workspace_one_byte_short_is_rejected(lib, entry):
    keys = S_MAX if entry == "dyn" else 9
    need = 6 * H * ((keys + 127) // 128) * 130 * 4                 # N * H * ceil(keys / 128) records of 130 floats, as the ungrouped kernel's
    refused(lib, entry, b"%d needed" % need, ws_bytes=need - 1)
    wide = dict(S_max=256, kc_hs=256 * 128, vc_hs=256 * 128, kc_rs=H * 256 * 128, vc_rs=H * 256 * 128)
    need = 6 * H * 2 * 130 * 4                                     # 129 keys (scalar) or a capacity of 256 (dyn): two records
    refused(lib, entry, b"%d needed" % need, ws_bytes=need - 1, **wide, **({} if entry == "dyn" else {"pos": 128}))


# the order of the checks is part of the ABI: of two faults, the one listed first names the error
ORDER = {
    "scalar": [("null pointer", dict(q=None)), ("both be given", dict(cos=P)), ("head_dim 64", dict(head_dim=64)), ("bad shape", dict(H=0)),
               ("S_max=1 ", dict(S_max=1)), ("group=9", dict(group=9)), ("not whole groups", dict(N=7)), ("pos=0", dict(pos=0)),
               ("beyond the cache capacity", dict(pos=S_MAX)), ("shared_len=0", dict(shared_len=0)), ("16-byte alignment", dict(vn=P + 2)),
               ("multiples of 8", dict(q_hs=132)), ("overlap", dict(kc_hs=S_MAX * 128 - 8)), ("row stride >= pos", dict(src=P, src_rs=3)),
               ("workspace", dict(ws_bytes=16))],
    "dyn": [("null pointer", dict(pos=None)), ("both be given", dict(sin=P)), ("head_dim 64", dict(head_dim=64)), ("bad shape", dict(H=0)),
            ("S_max=1 ", dict(S_max=1)), ("group=9", dict(group=9)), ("not whole groups", dict(N=7)), ("shared_len=0", dict(shared_len=0)),
            ("16-byte alignment", dict(vn=P + 2)), ("pos_dev needs 4-byte", dict(pos=P + 1)), ("multiples of 8", dict(q_hs=132)),
            ("overlap", dict(kc_hs=S_MAX * 128 - 8)), ("src one >= S_max - 1", dict(src=P, src_rs=3)), ("workspace", dict(ws_bytes=16))],
}


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_order_of_the_checks_is_stable(lib, entry):
    faults = ORDER[entry]
    for i, (text, over) in enumerate(faults):
        refused(lib, entry, text.encode(), **over)
        for later, more in faults[i + 1:]:
            if set(over) & set(more):
                continue
            refused(lib, entry, text.encode(), **over, **more)


def test_workspace_formulas_match_the_header():
    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    for macro, arg, fn in (("OTTER_DECODE_CACHED_SHARED_WORKSPACE_BYTES", "Sk", ops.decode_attn_cached_shared_workspace_bytes),
                           ("OTTER_DECODE_CACHED_SHARED_DYN_WORKSPACE_BYTES", "S_max", ops.decode_attn_cached_shared_dyn_workspace_bytes)):
        m = re.search(r"#define %s\(N, H, %s\) (.*)" % (macro, arg), hdr)
        expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
        for N, H_, Sk in [(2, 32, 513), (12, 32, 2), (6, 2, 65536)]:
            assert eval(expr, {"N": N, "H": H_, arg: Sk}) == fn(N, H_, Sk)
    assert int(re.search(r"#define OTTER_DECODE_CACHED_SHARED_MAX_GROUP (\d+)", hdr).group(1)) == ops.DECODE_CACHED_SHARED_GROUPS[-1]
    assert ops.DECODE_CACHED_SHARED_GROUPS == tuple(range(2, ops.DECODE_CACHED_SHARED_GROUPS[-1] + 1))


def test_the_source_is_built():
    from otter_amd import build

    assert "decode_cache_shared.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "decode_cache_shared.hip"))


# ---- the bindings, on CPU tensors (tests/_decode_binding_cases.py: the accepted calls and the mutations of decode_attn_cached / _dyn) ---------

N = 6


def run_binding(dyn, options=("src", "key_valid", "rotary", "slopes"), mutations=(), group=3, shared_len=5):
    """{"error": message} or {"symbol", "args"} of ops.decode_attn_cached_shared(_dyn) on the accepted call of the ungrouped binding."""
    from otter_amd import _capi, ops

    a = B.build(B.D2 if dyn else B.D1, N, options + (("out",) if dyn else ()))
    for m in mutations:
        B.MUTATIONS[m](a, N)
    with B.standin_library() as rec:
        try:
            getattr(ops, "decode_attn_cached_shared" + ("_dyn" if dyn else ""))(group=group, shared_len=shared_len, **a)
        except _capi.OtterHipError as e:
            return {"error": str(e)}
    (symbol, args), = rec.calls
    return {"symbol": symbol, "args": args}


@pytest.mark.parametrize("dyn", [False, True], ids=ENTRIES)
def test_binding_hands_the_ungrouped_arguments_plus_the_grouping(dyn):
    from otter_amd import ops

    name = "decode_attn_cached_shared" + ("_dyn" if dyn else "")
    got = run_binding(dyn)
    a = B.build(B.D2 if dyn else B.D1, N, ("src", "key_valid", "rotary", "slopes") + (("out",) if dyn else ()))
    with B.standin_library() as rec:
        getattr(ops, name.replace("_shared", ""))(**a)
    (_, plain), = rec.calls
    assert got["symbol"] == "otter_" + name
    assert len(got["args"]) == len(plain) + 2 and got["args"][-3:] == (3, 5, 0)        # ..., scale, group, shared_len, stream
    assert [type(x) for x in got["args"][:-3]] == [type(x) for x in plain[:-1]]
    strides_and_scalars = lambda t: [x for x in t if not isinstance(x, int) or x < (1 << 16)]     # (pointers differ from call to call)
    assert strides_and_scalars(got["args"][:-3]) == strides_and_scalars(plain[:-1])


@pytest.mark.parametrize("dyn", [False, True], ids=ENTRIES)
def test_binding_refusals(dyn):
    name = "decode_attn_cached_shared" + ("_dyn" if dyn else "")
    err = lambda **kw: run_binding(dyn, **kw).get("error")
    assert err(group=1) == name + ": group=1: the kernel is built for groups of 2 to 6 rows"
    assert err(group=7) == name + ": group=7: the kernel is built for groups of 2 to 6 rows"
    assert err(group=4) == name + ": N=6 rows are not whole groups of 4"
    assert err(shared_len=0) == name + (": shared_len=0 outside [1, S_max) with S_max=16" if dyn else ": shared_len=0 outside [1, pos] with pos=8")
    if dyn:
        assert err(shared_len=16) == name + ": shared_len=16 outside [1, S_max) with S_max=16"
        assert err(shared_len=15) is None
    else:
        assert err(shared_len=9) == name + ": shared_len=9 outside [1, pos] with pos=8"
        assert err(shared_len=8) is None
    # every check of the ungrouped binding, under this entry point's name, and before the grouping's
    for m, text in (("q_f32", "q / k_new / v_new must be bf16"), ("k_cache_f32", "k_cache / v_cache must be bf16"), ("src_i64", "src must be int32"),
                    ("key_valid_bool", "key_valid must be uint8"), ("slopes_f64", "slopes must be contiguous fp32"), ("sin_none", "both be given"),
                    ("pos_dev_two" if dyn else "pos0", "pos_dev must be" if dyn else "pos=0 outside")):
        assert err(mutations=(m,), group=9).startswith(name + ": ") and text in err(mutations=(m,), group=9), (m, err(mutations=(m,), group=9))


def test_bindings_need_gpu_tensors():
    from otter_amd import _capi, ops

    a = B.build(B.D1, N, ())
    with pytest.raises(_capi.OtterHipError):
        ops.decode_attn_cached_shared(group=3, shared_len=5, **a)
