"""CPU: otter_persimmon_decode_attn_cached / _dyn (csrc/persimmon_decode_cache.hip) validate their arguments before anything is launched --
negative status and a message, no GPU needed.  Device pointers are never dereferenced on these paths, so aligned dummy addresses stand in
for them."""
import os
import re

import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
S_MAX = 16


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, dyn, **over):
    a = dict(qkv=P, gq=P, bq=P, gk=P, bk=P, cos=P, sin=P, table_rs=32, kc=P, k_rs=2 * S_MAX * 64, k_hs=S_MAX * 64, vc=P, v_rs=2 * S_MAX * 64,
             v_hs=S_MAX * 64, src=None, src_rs=0, kvalid=None, kv_rs=0, o=P, ws=P, ws_bytes=1 << 20, N=1, H=2, pos=8, pos_dev=P, S_max=S_MAX,
             head_dim=64, rot=32, eps=1e-5, scale=0.125)
    a.update(over)
    if dyn:
        return lib.otter_persimmon_decode_attn_cached_dyn(a["qkv"], a["gq"], a["bq"], a["gk"], a["bk"], a["cos"], a["sin"], a["table_rs"], a["kc"],
                                                          a["k_rs"], a["k_hs"], a["vc"], a["v_rs"], a["v_hs"], a["src"], a["src_rs"], a["kvalid"],
                                                          a["kv_rs"], a["o"], a["ws"], a["ws_bytes"], a["N"], a["H"], a["pos_dev"], a["S_max"],
                                                          a["head_dim"], a["rot"], a["eps"], a["scale"], None)
    return lib.otter_persimmon_decode_attn_cached(a["qkv"], a["gq"], a["bq"], a["gk"], a["bk"], a["cos"], a["sin"], a["kc"], a["k_rs"], a["k_hs"],
                                                  a["vc"], a["v_rs"], a["v_hs"], a["src"], a["src_rs"], a["kvalid"], a["kv_rs"], a["o"], a["ws"],
                                                  a["ws_bytes"], a["N"], a["H"], a["pos"], a["S_max"], a["head_dim"], a["rot"], a["eps"],
                                                  a["scale"], None)


DYN = pytest.mark.parametrize("dyn", [False, True], ids=["scalar", "dyn"])


def rejected(lib, dyn, text, **over):
    assert call(lib, dyn, **over) == -1
    err = lib.otter_last_error()
    assert text in err and (b"persimmon_decode_attn_cached_dyn:" if dyn else b"persimmon_decode_attn_cached:") in err, err


@DYN
@pytest.mark.parametrize("name", ["qkv", "gq", "bq", "gk", "bk", "cos", "sin", "kc", "vc", "o", "ws"])
def test_null_pointers_are_rejected(lib, dyn, name):
    rejected(lib, dyn, b"null pointer", **{name: None})


def test_null_position_is_rejected(lib):
    rejected(lib, True, b"null pointer", pos_dev=None)
    rejected(lib, True, b"pos_dev needs 4-byte alignment", pos_dev=P + 2)


@DYN
def test_head_dim_other_than_64_is_rejected(lib, dyn):
    rejected(lib, dyn, b"head_dim 128", head_dim=128)


@DYN
@pytest.mark.parametrize("rot", [0, 8, 24, 80])
def test_rot_not_a_multiple_of_16_is_rejected(lib, dyn, rot):
    rejected(lib, dyn, b"rot=%d" % rot, rot=rot)


@DYN
def test_shape_and_capacity_limits(lib, dyn):
    rejected(lib, dyn, b"bad shape", N=0)
    rejected(lib, dyn, b"bad shape", H=65536)
    rejected(lib, dyn, b"S_max=1 outside", S_max=1, pos=0)
    rejected(lib, dyn, b"S_max=65537 outside", S_max=65537, k_hs=65537 * 64 + 56, v_hs=65537 * 64 + 56, k_rs=1 << 24, v_rs=1 << 24, ws_bytes=1 << 30)


def test_the_scalar_position_must_continue_the_cache_below_its_capacity(lib):
    rejected(lib, False, b"pos=0", pos=0)
    rejected(lib, False, b"beyond the cache capacity", pos=S_MAX)
    rejected(lib, False, b"beyond the cache capacity", pos=S_MAX + 3)


@DYN
def test_layout_rules(lib, dyn):
    rejected(lib, dyn, b"16-byte alignment", qkv=P + 8)
    rejected(lib, dyn, b"16-byte alignment", kc=P + 2)
    rejected(lib, dyn, b"16-byte alignment", vc=P + 4)
    rejected(lib, dyn, b"multiples of 8", k_rs=2 * S_MAX * 64 + 4)
    rejected(lib, dyn, b"multiples of 8", v_hs=S_MAX * 64 + 4)
    rejected(lib, dyn, b"slots of two heads overlap", k_hs=S_MAX * 64 - 8)
    rejected(lib, dyn, b"slots of two heads overlap", v_hs=(S_MAX - 1) * 64)
    rejected(lib, dyn, b"slots of two heads overlap", k_rs=-8)


def test_table_and_mask_strides(lib):
    rejected(lib, False, b"src needs a row stride >= pos", src=P, src_rs=7)
    rejected(lib, False, b"key_valid one >= pos + 1", kvalid=P, kv_rs=8)
    rejected(lib, True, b"src one >= S_max - 1", src=P, src_rs=S_MAX - 2)
    rejected(lib, True, b"key_valid one >= S_max", kvalid=P, kv_rs=S_MAX - 1)
    rejected(lib, True, b"row stride >= rot", table_rs=16)


def test_workspace_size(lib):
    rejected(lib, False, b"workspace", ws_bytes=2 * 66 * 4 - 1)                  # N * H * ceil(9 / 128) records of 66 floats
    rejected(lib, True, b"workspace", ws_bytes=2 * 66 * 4 - 1)                   # ... ceil(S_max / 128)
    rejected(lib, False, b"workspace", pos=128, S_max=300, k_hs=300 * 64, v_hs=300 * 64, k_rs=600 * 64, v_rs=600 * 64, ws_bytes=2 * 2 * 66 * 4 - 1)
    rejected(lib, True, b"workspace", S_max=300, k_hs=300 * 64, v_hs=300 * 64, k_rs=600 * 64, v_rs=600 * 64, ws_bytes=2 * 3 * 66 * 4 - 1)


def test_workspace_formulas_match_the_header():
    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    for macro, arg, fn in (("OTTER_PERSIMMON_DECODE_CACHED_WORKSPACE_BYTES", "Sk", ops.persimmon_decode_cached_workspace_bytes),
                           ("OTTER_PERSIMMON_DECODE_CACHED_DYN_WORKSPACE_BYTES", "S_max", ops.persimmon_decode_cached_dyn_workspace_bytes)):
        m = re.search(r"#define %s\(N, H, %s\) (.*)" % (macro, arg), hdr)
        expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
        for N, H, S in [(1, 64, 1351), (4, 64, 2), (3, 2, 16384), (12, 64, 4224)]:
            assert eval(expr, {"N": N, "H": H, arg: S}) == fn(N, H, S) == N * H * ((S + 127) // 128) * 66 * 4
