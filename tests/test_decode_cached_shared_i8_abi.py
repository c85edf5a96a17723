"""CPU: otter_decode_attn_cached_shared_i8 / _dyn (csrc/decode_cache_shared_i8.hip) validate their arguments before anything is launched --
negative status and a message, no GPU needed -- in an order that is part of the ABI, and so do their Python bindings, on CPU tensors over a
recording stand-in for the library.  Device pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them.
The style is tests/test_decode_cached_shared_abi.py's; the order of the checks is tests/test_decode_cached_check_order.py's table."""
import os
import re

import pytest
import torch

from tests import _decode_binding_cases as B

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
H, S_MAX = 2, 64
ENTRIES = ["scalar", "dyn"]
NAMES = {"scalar": "decode_attn_cached_shared_i8", "dyn": "decode_attn_cached_shared_i8_dyn"}

# the order of the arguments: otter_decode_attn_cached_i8's, then group, shared_len (the stream follows)
ORDER = ["q", "q_rs", "q_hs", "kn", "kn_rs", "kn_hs", "vn", "vn_rs", "vn_hs", "cos", "sin", "cs_rs", "kc", "kc_rs", "kc_hs", "vc", "vc_rs", "vc_hs",
         "ks", "ks_rs", "ks_hs", "vs", "vs_rs", "vs_hs", "src", "src_rs", "kvalid", "kv_rs", "slopes", "o", "ws", "ws_bytes", "N", "H", "pos", "S_max",
         "head_dim", "scale", "group", "shared_len"]


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def valid(dyn):
    return dict(q=P, q_rs=3 * H * 128, q_hs=128, kn=P + 2 * H * 128, kn_rs=3 * H * 128, kn_hs=128, vn=P + 4 * H * 128, vn_rs=3 * H * 128, vn_hs=128,
                cos=None, sin=None, cs_rs=0, kc=P, kc_rs=H * S_MAX * 128, kc_hs=S_MAX * 128, vc=P, vc_rs=H * S_MAX * 128, vc_hs=S_MAX * 128,
                ks=P, ks_rs=H * S_MAX, ks_hs=S_MAX, vs=P, vs_rs=H * S_MAX, vs_hs=S_MAX, src=None, src_rs=0, kvalid=None, kv_rs=0, slopes=None,
                o=P, ws=P, ws_bytes=1 << 20, N=6, H=H, pos=P if dyn else 8, S_max=S_MAX, head_dim=128, scale=0.0884, group=3, shared_len=5)


def call(lib, entry, *overs, **over):
    a = valid(entry == "dyn")
    for o in overs:
        a.update(o)
    a.update(over)
    return getattr(lib, "otter_" + NAMES[entry])(*[a[k] for k in ORDER], None)


def refused(lib, entry, text, *overs, **over):
    assert call(lib, entry, *overs, **over) == -1
    msg = lib.otter_last_error()
    assert msg.startswith(NAMES[entry].encode() + b": "), msg
    assert (text if isinstance(text, bytes) else text.encode()) in msg, msg


# ---- every refusal -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers_are_rejected(lib, entry):
    for name in ["q", "kn", "vn", "kc", "vc", "ks", "vs", "o", "ws"] + (["pos"] if entry == "dyn" else []):
        refused(lib, entry, b"null pointer", **{name: None})


@pytest.mark.parametrize("entry", ENTRIES)
def test_cos_without_sin_is_rejected(lib, entry):
    what = b"cos_table and sin_table" if entry == "dyn" else b"cos_rows and sin_rows"
    refused(lib, entry, what + b" must both be given or both be NULL", cos=P)
    refused(lib, entry, what + b" must both be given or both be NULL", sin=P)


@pytest.mark.parametrize("entry", ENTRIES)
def test_shape_rules(lib, entry):
    refused(lib, entry, b"head_dim 64 (128 only)", head_dim=64)
    refused(lib, entry, b"bad shape N=0 H=2", N=0)
    refused(lib, entry, b"bad shape N=6 H=65536", H=65536)
    big = 65536 + 1
    refused(lib, entry, b"S_max=65537 outside [2, 65536]", S_max=big, kc_hs=big * 128, vc_hs=big * 128, kc_rs=H * big * 128, vc_rs=H * big * 128,
            ks_hs=big, vs_hs=big, ks_rs=H * big, vs_rs=H * big)
    refused(lib, entry, b"S_max=1 outside [2, 65536]", S_max=1)


@pytest.mark.parametrize("entry", ENTRIES)
def test_group_rules(lib, entry):
    from otter_amd import ops

    assert ops.DECODE_CACHED_SHARED_I8_GROUPS == ops.DECODE_CACHED_SHARED_GROUPS == (2, 3, 4, 5, 6)
    for group in (-3, 0, 1, 7, 8, 64):
        refused(lib, entry, b"group=%d: the kernel is built for groups of 2 to 6 rows" % group, group=group, N=64 * 3)
    refused(lib, entry, b"N=6 rows are not whole groups of 4", group=4)
    refused(lib, entry, b"N=7 rows are not whole groups of 3", N=7)


def test_position_and_shared_len_rules_of_the_scalar_entry(lib):
    refused(lib, "scalar", b"pos=0: a cached step continues a cache (pos >= 1)", pos=0, shared_len=0)      # the position's own rules come first
    refused(lib, "scalar", b"pos=64 is beyond the cache capacity S_max=64", pos=S_MAX, shared_len=1)
    for bad in (0, -1, 9, S_MAX):
        refused(lib, "scalar", b"shared_len=%d outside [1, pos] with pos=8" % bad, shared_len=bad)


def test_shared_len_and_pos_dev_rules_of_the_dyn_entry(lib):
    for bad in (0, -1, S_MAX, S_MAX + 7):
        refused(lib, "dyn", b"shared_len=%d outside [1, S_max) with S_max=64" % bad, shared_len=bad)
    refused(lib, "dyn", b"pos_dev needs 4-byte alignment", pos=P + 2)


@pytest.mark.parametrize("entry", ENTRIES)
def test_alignment_and_strides(lib, entry):
    for name in ["q", "kn", "vn", "kc", "vc"]:
        refused(lib, entry, b"q, k_new, v_new, k_cache, v_cache need 16-byte alignment", **{name: P + 8})
    for name in ["ks", "vs"]:
        refused(lib, entry, b"k_scale, v_scale need 4-byte alignment", **{name: P + 2})
    for name in ["q_rs", "q_hs", "kn_rs", "kn_hs", "vn_rs", "vn_hs"]:
        refused(lib, entry, b"q / k_new / v_new strides must be multiples of 8 elements", **{name: 3 * H * 128 + 4})
    for name in ["kc_rs", "vc_rs"]:
        refused(lib, entry, b"code cache strides must be multiples of 16 elements", **{name: H * S_MAX * 128 + 8})
    for name in ["kc_hs", "vc_hs"]:
        refused(lib, entry, b"code cache strides must be multiples of 16 elements", **{name: S_MAX * 128 + 8})
        refused(lib, entry, b"a cache head stride below S_max * 128 would make the slots of two heads overlap", **{name: S_MAX * 128 - 16})
    for name in ["kc_rs", "vc_rs"]:
        refused(lib, entry, b"would make the slots of two heads overlap", **{name: -16})
    for name in ["ks_hs", "vs_hs"]:
        refused(lib, entry, b"a scale head stride below S_max would make the scales of two heads overlap", **{name: S_MAX - 1})
    for name in ["ks_rs", "vs_rs"]:
        refused(lib, entry, b"would make the scales of two heads overlap", **{name: -1})
    if entry == "dyn":
        text = b"cos / sin tables need a row stride >= 128, src one >= S_max - 1, key_valid one >= S_max"
        refused(lib, entry, text, src=P, src_rs=S_MAX - 2)
        refused(lib, entry, text, kvalid=P, kv_rs=S_MAX - 1)
        refused(lib, entry, text, cos=P, sin=P, cs_rs=64)
    else:
        text = b"src needs a row stride >= pos, key_valid one >= pos + 1, cos / sin a non-negative one"
        refused(lib, entry, text, src=P, src_rs=7)                    # pos = 8 entries per row
        refused(lib, entry, text, kvalid=P, kv_rs=8)                  # pos + 1 = 9 keys per row
        refused(lib, entry, text, cos=P, sin=P, cs_rs=-128)


@pytest.mark.parametrize("entry", ENTRIES)
def test_workspace_one_byte_short_is_rejected(lib, entry):
    keys = S_MAX if entry == "dyn" else 9
    need = 6 * H * ((keys + 127) // 128) * 130 * 4                 # N * H * ceil(keys / 128) records of 130 floats, as the ungrouped kernel's
    refused(lib, entry, b"workspace of %d bytes, %d needed" % (need - 1, need), ws_bytes=need - 1)
    wide = dict(S_max=256, kc_hs=256 * 128, vc_hs=256 * 128, kc_rs=H * 256 * 128, vc_rs=H * 256 * 128, ks_hs=256, vs_hs=256, ks_rs=H * 256,
                vs_rs=H * 256)
    need = 6 * H * 2 * 130 * 4                                     # 129 keys (scalar) or a capacity of 256 (dyn): two records
    refused(lib, entry, b"%d needed" % need, ws_bytes=need - 1, **wide, **({} if entry == "dyn" else {"pos": 128}))


# (the order of the checks, part of the ABI, is in tests/test_decode_cached_check_order.py: the one table of all ten entry points)


def test_workspace_formulas_match_the_header():
    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    for macro, arg, fn in (("OTTER_DECODE_CACHED_SHARED_I8_WORKSPACE_BYTES", "Sk", ops.decode_attn_cached_shared_i8_workspace_bytes),
                           ("OTTER_DECODE_CACHED_SHARED_I8_DYN_WORKSPACE_BYTES", "S_max", ops.decode_attn_cached_shared_i8_dyn_workspace_bytes)):
        m = re.search(r"#define %s\(N, H, %s\) (.*)" % (macro, arg), hdr)
        expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
        for N, H_, Sk in [(2, 32, 513), (12, 32, 2), (6, 2, 65536)]:
            assert eval(expr, {"N": N, "H": H_, arg: Sk}) == fn(N, H_, Sk)
    assert int(re.search(r"#define OTTER_DECODE_CACHED_SHARED_MAX_GROUP (\d+)", hdr).group(1)) == ops.DECODE_CACHED_SHARED_I8_GROUPS[-1]


def test_the_source_is_built_and_the_symbols_are_declared():
    from otter_amd import _capi, build

    assert "decode_cache_shared_i8.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "decode_cache_shared_i8.hip"))
    for entry in ENTRIES:
        plain = _capi.SIGNATURES["otter_" + NAMES[entry].replace("_shared", "")]
        grouped = _capi.SIGNATURES["otter_" + NAMES[entry]]
        assert grouped[0] is plain[0] and grouped[1] == plain[1][:-1] + [_capi._i64, _capi._i64, plain[1][-1]]


# ---- the bindings, on CPU tensors (tests/_decode_binding_cases.py: the accepted calls and the mutations of decode_attn_cached_i8 / _dyn) -------

N = 6
OPTIONS = ("src", "key_valid", "rotary", "slopes")


def run_binding(dyn, options=OPTIONS, mutations=(), group=3, shared_len=5):
    """{"error": message} or {"symbol", "args"} of ops.decode_attn_cached_shared_i8(_dyn) on the accepted call of the ungrouped int8 binding."""
    from otter_amd import _capi, ops

    a = B.build(B.D4 if dyn else B.D3, N, options + (("out",) if dyn else ()))
    for m in mutations:
        B.MUTATIONS[m](a, N)
    with B.standin_library() as rec:
        try:
            getattr(ops, NAMES["dyn" if dyn else "scalar"])(group=group, shared_len=shared_len, **a)
        except _capi.OtterHipError as e:
            return {"error": str(e)}
    (symbol, args), = rec.calls
    return {"symbol": symbol, "args": args, "inputs": a}


@pytest.mark.parametrize("dyn", [False, True], ids=ENTRIES)
def test_binding_hands_the_int8_arguments_plus_the_grouping(dyn):
    from otter_amd import ops

    name = NAMES["dyn" if dyn else "scalar"]
    got = run_binding(dyn)
    a = B.build(B.D4 if dyn else B.D3, N, OPTIONS + (("out",) if dyn else ()))
    with B.standin_library() as rec:
        getattr(ops, name.replace("_shared", ""))(**a)
    (_, plain), = rec.calls
    assert got["symbol"] == "otter_" + name
    assert len(got["args"]) == len(plain) + 2 == len(ORDER) + 1 and got["args"][-3:] == (3, 5, 0)    # ..., scale, group, shared_len, stream
    assert [type(x) for x in got["args"][:-3]] == [type(x) for x in plain[:-1]]
    strides_and_scalars = lambda t: [x for x in t if not isinstance(x, int) or x < (1 << 16)]     # (pointers differ from call to call)
    assert strides_and_scalars(got["args"][:-3]) == strides_and_scalars(plain[:-1])
    # the scales and their strides in place: after the caches, before the table
    by_name, t = dict(zip(ORDER, got["args"])), got["inputs"]
    assert (by_name["ks"], by_name["ks_rs"], by_name["ks_hs"]) == (t["k_scale"].data_ptr(), t["k_scale"].stride(0), t["k_scale"].stride(1))
    assert (by_name["vs"], by_name["vs_rs"], by_name["vs_hs"]) == (t["v_scale"].data_ptr(), t["v_scale"].stride(0), t["v_scale"].stride(1))
    assert (by_name["kc"], by_name["vc"], by_name["src"]) == (t["k_cache"].data_ptr(), t["v_cache"].data_ptr(), t["src"].data_ptr())
    assert (by_name["N"], by_name["H"], by_name["S_max"], by_name["head_dim"]) == (N, B.H, B.S_MAX, 128)
    assert by_name["pos"] == (t["pos_dev"].data_ptr() if dyn else B.POS)
    assert (by_name["group"], by_name["shared_len"]) == (3, 5)


@pytest.mark.parametrize("dyn", [False, True], ids=ENTRIES)
def test_binding_refusals(dyn):
    name = NAMES["dyn" if dyn else "scalar"]
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
    # every check of the ungrouped int8 binding, word for word under this entry point's name, and before the grouping's
    plain = name.replace("_shared", "")
    for m in ("q_f32", "k_cache_f32", "cache_pad8", "k_scale_f64", "v_scale_short", "v_scale_strided", "src_i64", "key_valid_bool", "slopes_f64",
              "sin_none", "pos_dev_two" if dyn else "pos0"):
        a = B.build(B.D4 if dyn else B.D3, N, OPTIONS + (("out",) if dyn else ()))
        B.MUTATIONS[m](a, N)
        from otter_amd import _capi, ops

        with B.standin_library(), pytest.raises(_capi.OtterHipError) as want:
            getattr(ops, plain)(**a)
        assert str(want.value).startswith(plain + ": ")
        assert err(mutations=(m,), group=9) == name + str(want.value)[len(plain):], m


def test_bindings_need_gpu_tensors():
    from otter_amd import _capi, ops

    a = B.build(B.D3, N, ())
    with pytest.raises(_capi.OtterHipError):
        ops.decode_attn_cached_shared_i8(group=3, shared_len=5, **a)
