"""CPU: otter_persimmon_decode_attn (csrc/persimmon_decode.hip) validates its arguments before anything is launched -- negative status and a
message, no GPU needed.  Device pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them."""
import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, **over):
    a = dict(qkv=P, gq=P, bq=P, gk=P, bk=P, cos=P, sin=P, kp=P, k_bs=2 * 64 * 8, k_hs=64 * 8, k_ss=64, k_ds=1, vp=P, v_bs=2 * 64 * 8,
             v_hs=64 * 8, v_ss=64, v_ds=1, kvalid=None, kn=P, vn=P, o=P, ws=P, ws_bytes=1 << 20, B=1, H=2, S_past=8, head_dim=64, rot=32,
             eps=1e-5, scale=0.125)
    a.update(over)
    return lib.otter_persimmon_decode_attn(a["qkv"], a["gq"], a["bq"], a["gk"], a["bk"], a["cos"], a["sin"], a["kp"], a["k_bs"], a["k_hs"],
                                           a["k_ss"], a["k_ds"], a["vp"], a["v_bs"], a["v_hs"], a["v_ss"], a["v_ds"], a["kvalid"], a["kn"],
                                           a["vn"], a["o"], a["ws"], a["ws_bytes"], a["B"], a["H"], a["S_past"], a["head_dim"], a["rot"],
                                           a["eps"], a["scale"], None)


@pytest.mark.parametrize("name", ["qkv", "gq", "bk", "cos", "sin", "kp", "vp", "kn", "vn", "o", "ws"])
def test_null_pointers_are_rejected(lib, name):
    assert call(lib, **{name: None}) == -1
    assert b"null pointer" in lib.otter_last_error()


def test_head_dim_other_than_64_is_rejected(lib):
    assert call(lib, head_dim=128) == -1
    assert b"head_dim 128" in lib.otter_last_error()


def test_key_count_above_the_limit_is_rejected(lib):
    assert call(lib, S_past=65536, ws_bytes=1 << 30) == -1
    assert b"exceeds the limit" in lib.otter_last_error()
    assert call(lib, S_past=0) == -1                 # a decode step continues a cache
    assert b"bad shape" in lib.otter_last_error()


@pytest.mark.parametrize("rot", [0, 8, 24, 80])
def test_rot_not_a_multiple_of_16_is_rejected(lib, rot):
    assert call(lib, rot=rot) == -1
    assert b"rot=%d" % rot in lib.otter_last_error()


def test_layout_and_workspace_rules(lib):
    assert call(lib, k_ds=64, k_ss=1) == -1
    assert b"unit dim stride" in lib.otter_last_error()
    assert call(lib, v_ss=68) == -1
    assert b"multiples of 8" in lib.otter_last_error()
    assert call(lib, kn=P + 2) == -1
    assert b"16-byte alignment" in lib.otter_last_error()
    assert call(lib, ws_bytes=2 * 66 * 4 - 1) == -1                # B * H * ceil(9 / 128) records of 66 floats
    assert b"workspace" in lib.otter_last_error()


def test_workspace_formula_matches_the_header():
    import os
    import re

    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    m = re.search(r"#define OTTER_PERSIMMON_DECODE_WORKSPACE_BYTES\(B, H, Sk\) (.*)", hdr)
    expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
    for B, H, Sk in [(1, 64, 1351), (4, 64, 2), (3, 2, 16384)]:
        assert eval(expr, {"B": B, "H": H, "Sk": Sk}) == ops.persimmon_decode_workspace_bytes(B, H, Sk)
