"""CPU: otter_decode_attn_cached (csrc/decode_cache.hip) validates its arguments before anything is launched -- negative status and a message,
no GPU needed.  Device pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them."""
import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
H, S_MAX = 2, 64


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, **over):
    a = dict(q=P, q_rs=3 * H * 128, q_hs=128, kn=P + 2 * H * 128, kn_rs=3 * H * 128, kn_hs=128, vn=P + 4 * H * 128, vn_rs=3 * H * 128, vn_hs=128,
             cos=None, sin=None, cs_rs=0, kc=P, kc_rs=H * S_MAX * 128, kc_hs=S_MAX * 128, vc=P, vc_rs=H * S_MAX * 128, vc_hs=S_MAX * 128,
             src=None, src_rs=0, kvalid=None, kv_rs=0, slopes=None, o=P, ws=P, ws_bytes=1 << 20, N=3, H=H, pos=8, S_max=S_MAX, head_dim=128,
             scale=0.0884)
    a.update(over)
    return lib.otter_decode_attn_cached(a["q"], a["q_rs"], a["q_hs"], a["kn"], a["kn_rs"], a["kn_hs"], a["vn"], a["vn_rs"], a["vn_hs"], a["cos"],
                                        a["sin"], a["cs_rs"], a["kc"], a["kc_rs"], a["kc_hs"], a["vc"], a["vc_rs"], a["vc_hs"], a["src"],
                                        a["src_rs"], a["kvalid"], a["kv_rs"], a["slopes"], a["o"], a["ws"], a["ws_bytes"], a["N"], a["H"],
                                        a["pos"], a["S_max"], a["head_dim"], a["scale"], None)


@pytest.mark.parametrize("name", ["q", "kn", "vn", "kc", "vc", "o", "ws"])
def test_null_pointers_are_rejected(lib, name):
    assert call(lib, **{name: None}) == -1
    assert b"null pointer" in lib.otter_last_error()


def test_cos_without_sin_is_rejected(lib):
    assert call(lib, cos=P) == -1
    assert b"both be given or both be NULL" in lib.otter_last_error()
    assert call(lib, sin=P) == -1
    assert b"both be given or both be NULL" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q", "kn", "vn", "kc", "vc"])
def test_misaligned_pointers_are_rejected(lib, name):
    assert call(lib, **{name: P + 2}) == -1
    assert b"16-byte alignment" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q_rs", "q_hs", "kn_rs", "kn_hs", "vn_rs", "vn_hs", "kc_rs", "vc_rs"])
def test_strides_that_are_not_multiples_of_8_are_rejected(lib, name):
    assert call(lib, **{name: 3 * H * 128 + 4}) == -1
    assert b"multiples of 8" in lib.otter_last_error()


def test_cache_and_table_stride_rules(lib):
    assert call(lib, kc_hs=S_MAX * 128 - 8) == -1                  # the slots of two heads would overlap
    assert b"overlap" in lib.otter_last_error()
    assert call(lib, vc_hs=S_MAX * 128 - 8) == -1
    assert b"overlap" in lib.otter_last_error()
    assert call(lib, src=P, src_rs=7) == -1                        # pos = 8 entries per row are read
    assert b"row stride >= pos" in lib.otter_last_error()
    assert call(lib, kvalid=P, kv_rs=8) == -1                      # pos + 1 = 9 keys per row
    assert b"row stride >= pos" in lib.otter_last_error()


def test_head_dim_other_than_128_is_rejected(lib):
    assert call(lib, head_dim=64) == -1
    assert b"head_dim 64" in lib.otter_last_error()


def test_position_and_capacity_rules(lib):
    assert call(lib, pos=0) == -1                                  # a cached step continues a cache
    assert b"pos=0" in lib.otter_last_error()
    assert call(lib, pos=S_MAX) == -1
    assert b"beyond the cache capacity" in lib.otter_last_error()
    assert call(lib, pos=S_MAX + 5) == -1
    assert b"beyond the cache capacity" in lib.otter_last_error()
    big = 65536 + 1
    assert call(lib, S_max=big, kc_hs=big * 128, vc_hs=big * 128, kc_rs=H * big * 128, vc_rs=H * big * 128) == -1
    assert b"S_max=65537" in lib.otter_last_error()


def test_workspace_one_byte_short_is_rejected(lib):
    need = 3 * H * 1 * 130 * 4                                     # N * H * ceil(9 / 128) records of 130 floats
    assert call(lib, ws_bytes=need - 1) == -1
    assert b"workspace" in lib.otter_last_error()
    need = 3 * H * 2 * 130 * 4                                     # pos = 128: 129 keys, two records
    assert call(lib, pos=128, S_max=256, kc_hs=256 * 128, vc_hs=256 * 128, kc_rs=H * 256 * 128, vc_rs=H * 256 * 128, ws_bytes=need - 1) == -1
    assert b"%d needed" % need in lib.otter_last_error()


def test_workspace_formula_matches_the_header():
    import os
    import re

    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    m = re.search(r"#define OTTER_DECODE_CACHED_WORKSPACE_BYTES\(N, H, Sk\) (.*)", hdr)
    expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
    for N, H_, Sk in [(1, 32, 513), (12, 32, 2), (3, 2, 65536)]:
        assert eval(expr, {"N": N, "H": H_, "Sk": Sk}) == ops.decode_attn_cached_workspace_bytes(N, H_, Sk)
    assert ops.decode_attn_cached_workspace_bytes(1, 32, 513) == 32 * 5 * 130 * 4
