"""CPU: otter_decode_attn_cached_i8 and otter_decode_attn_cached_i8_dyn (csrc/decode_cache_i8.hip) validate their arguments before anything is
launched -- negative status and a message, no GPU needed.  Device pointers are never dereferenced on these paths, so aligned dummy addresses
stand in for them."""
import os
import re

import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
H, S_MAX = 2, 64
ENTRIES = ["scalar", "dyn"]


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, entry, **over):
    a = dict(q=P, q_rs=3 * H * 128, q_hs=128, kn=P + 2 * H * 128, kn_rs=3 * H * 128, kn_hs=128, vn=P + 4 * H * 128, vn_rs=3 * H * 128, vn_hs=128,
             cos=None, sin=None, cs_rs=0, kc=P, kc_rs=H * S_MAX * 128, kc_hs=S_MAX * 128, vc=P, vc_rs=H * S_MAX * 128, vc_hs=S_MAX * 128,
             ks=P, ks_rs=H * S_MAX, ks_hs=S_MAX, vs=P, vs_rs=H * S_MAX, vs_hs=S_MAX, src=None, src_rs=0, kvalid=None, kv_rs=0, slopes=None, o=P,
             ws=P, ws_bytes=1 << 20, N=3, H=H, pos=8, pos_dev=P, S_max=S_MAX, head_dim=128, scale=0.0884)
    a.update(over)
    fn = lib.otter_decode_attn_cached_i8 if entry == "scalar" else lib.otter_decode_attn_cached_i8_dyn
    return fn(a["q"], a["q_rs"], a["q_hs"], a["kn"], a["kn_rs"], a["kn_hs"], a["vn"], a["vn_rs"], a["vn_hs"], a["cos"], a["sin"], a["cs_rs"],
              a["kc"], a["kc_rs"], a["kc_hs"], a["vc"], a["vc_rs"], a["vc_hs"], a["ks"], a["ks_rs"], a["ks_hs"], a["vs"], a["vs_rs"], a["vs_hs"],
              a["src"], a["src_rs"], a["kvalid"], a["kv_rs"], a["slopes"], a["o"], a["ws"], a["ws_bytes"], a["N"], a["H"],
              a["pos"] if entry == "scalar" else a["pos_dev"], a["S_max"], a["head_dim"], a["scale"], None)


def name_of(entry):
    return b"decode_attn_cached_i8" + (b"_dyn" if entry == "dyn" else b"") + b":"


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["q", "kn", "vn", "kc", "vc", "ks", "vs", "o", "ws"])
def test_null_pointers_are_rejected(lib, entry, name):
    assert call(lib, entry, **{name: None}) == -1
    assert name_of(entry) + b" null pointer" in lib.otter_last_error()


def test_null_position_pointer_is_rejected(lib):
    assert call(lib, "dyn", pos_dev=None) == -1
    assert b"decode_attn_cached_i8_dyn: null pointer" in lib.otter_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_cos_without_sin_is_rejected(lib, entry):
    assert call(lib, entry, cos=P) == -1
    assert b"both be given or both be NULL" in lib.otter_last_error() and name_of(entry) in lib.otter_last_error()
    assert call(lib, entry, sin=P) == -1
    assert b"both be given or both be NULL" in lib.otter_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["q", "kn", "vn", "kc", "vc"])
def test_misaligned_pointers_are_rejected(lib, entry, name):
    assert call(lib, entry, **{name: P + 8}) == -1
    assert b"16-byte alignment" in lib.otter_last_error() and name_of(entry) in lib.otter_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["ks", "vs"])
def test_misaligned_scale_pointers_are_rejected(lib, entry, name):
    assert call(lib, entry, **{name: P + 2}) == -1
    assert b"k_scale, v_scale need 4-byte alignment" in lib.otter_last_error() and name_of(entry) in lib.otter_last_error()


def test_misaligned_position_pointer_is_rejected(lib):
    assert call(lib, "dyn", pos_dev=P + 2) == -1
    assert b"pos_dev needs 4-byte alignment" in lib.otter_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["q_rs", "q_hs", "kn_rs", "kn_hs", "vn_rs", "vn_hs"])
def test_new_token_strides_that_are_not_multiples_of_8_are_rejected(lib, entry, name):
    assert call(lib, entry, **{name: 3 * H * 128 + 4}) == -1
    assert b"multiples of 8" in lib.otter_last_error() and name_of(entry) in lib.otter_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["kc_rs", "kc_hs", "vc_rs", "vc_hs"])
def test_code_cache_strides_that_are_not_multiples_of_16_are_rejected(lib, entry, name):
    assert call(lib, entry, **{name: H * S_MAX * 128 + 8}) == -1      # a multiple of 8: enough for the bf16 cache, not for 16 codes per lane
    assert b"multiples of 16" in lib.otter_last_error() and name_of(entry) in lib.otter_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_cache_and_scale_head_stride_rules(lib, entry):
    for name in ("kc_hs", "vc_hs"):
        assert call(lib, entry, **{name: S_MAX * 128 - 16}) == -1   # the slots of two heads would overlap
        assert b"slots of two heads overlap" in lib.otter_last_error()
    for name in ("ks_hs", "vs_hs"):
        assert call(lib, entry, **{name: S_MAX - 1}) == -1
        assert b"scales of two heads overlap" in lib.otter_last_error() and name_of(entry) in lib.otter_last_error()
    for name in ("kc_rs", "vc_rs", "ks_rs", "vs_rs"):
        assert call(lib, entry, **{name: -16}) == -1
        assert b"overlap" in lib.otter_last_error()


def test_table_and_mask_stride_rules(lib):
    assert call(lib, "scalar", src=P, src_rs=7) == -1                 # pos = 8 entries per row are read
    assert b"row stride >= pos" in lib.otter_last_error()
    assert call(lib, "scalar", kvalid=P, kv_rs=8) == -1               # pos + 1 = 9 keys per row
    assert b"row stride >= pos" in lib.otter_last_error()
    assert call(lib, "scalar", cos=P, sin=P, cs_rs=-128) == -1
    assert b"non-negative" in lib.otter_last_error()
    # the dyn entry may be handed any position below S_max: the tables must hold the capacity
    assert call(lib, "dyn", src=P, src_rs=S_MAX - 2) == -1
    assert b"src one >= S_max - 1" in lib.otter_last_error()
    assert call(lib, "dyn", kvalid=P, kv_rs=S_MAX - 1) == -1
    assert b"key_valid one >= S_max" in lib.otter_last_error()
    assert call(lib, "dyn", cos=P, sin=P, cs_rs=64) == -1
    assert b"row stride >= 128" in lib.otter_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
def test_head_dim_shape_and_capacity_rules(lib, entry):
    assert call(lib, entry, head_dim=64) == -1
    assert b"head_dim 64" in lib.otter_last_error() and name_of(entry) in lib.otter_last_error()
    assert call(lib, entry, N=0) == -1
    assert b"bad shape" in lib.otter_last_error()
    assert call(lib, entry, H=65536) == -1
    assert b"bad shape" in lib.otter_last_error()
    assert call(lib, entry, S_max=1) == -1
    assert b"S_max=1 outside" in lib.otter_last_error()
    big = 65536 + 1
    assert call(lib, entry, S_max=big, kc_hs=big * 128, vc_hs=big * 128, kc_rs=H * big * 128, vc_rs=H * big * 128, ks_hs=big, vs_hs=big,
                ks_rs=H * big, vs_rs=H * big) == -1
    assert b"S_max=65537" in lib.otter_last_error()


def test_position_rules_of_the_scalar_entry(lib):
    assert call(lib, "scalar", pos=0) == -1                           # a cached step continues a cache
    assert b"pos=0" in lib.otter_last_error()
    assert call(lib, "scalar", pos=S_MAX) == -1
    assert b"beyond the cache capacity" in lib.otter_last_error()
    assert call(lib, "scalar", pos=S_MAX + 5) == -1
    assert b"beyond the cache capacity" in lib.otter_last_error()


def test_workspace_one_byte_short_is_rejected(lib):
    need = 3 * H * 1 * 130 * 4                                        # N * H * ceil(9 / 128) records of 130 floats
    assert call(lib, "scalar", ws_bytes=need - 1) == -1
    assert b"workspace" in lib.otter_last_error()
    wide = dict(S_max=256, kc_hs=256 * 128, vc_hs=256 * 128, kc_rs=H * 256 * 128, vc_rs=H * 256 * 128, ks_hs=256, vs_hs=256, ks_rs=H * 256,
                vs_rs=H * 256)
    need = 3 * H * 2 * 130 * 4                                        # pos = 128: 129 keys, two records
    assert call(lib, "scalar", pos=128, ws_bytes=need - 1, **wide) == -1
    assert b"%d needed" % need in lib.otter_last_error()
    assert call(lib, "dyn", ws_bytes=3 * H * 1 * 130 * 4 - 1) == -1   # capacity 64: one record
    assert b"decode_attn_cached_i8_dyn: workspace" in lib.otter_last_error()
    assert call(lib, "dyn", ws_bytes=need - 1, **wide) == -1          # capacity 256: two records, whatever the position
    assert b"%d needed" % need in lib.otter_last_error()


def test_workspace_formulas_match_the_header():
    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    for macro, arg, fn in (("OTTER_DECODE_CACHED_I8_WORKSPACE_BYTES", "Sk", ops.decode_attn_cached_i8_workspace_bytes),
                           ("OTTER_DECODE_CACHED_I8_DYN_WORKSPACE_BYTES", "S_max", ops.decode_attn_cached_i8_dyn_workspace_bytes)):
        m = re.search(r"#define %s\(N, H, %s\) (.*)" % (macro, arg), hdr)
        expr = m.group(1).replace("(int64_t)", "").replace("/", "//")
        for N, H_, S in [(1, 32, 513), (12, 32, 2), (3, 2, 65536)]:
            assert eval(expr, {"N": N, "H": H_, arg: S}) == fn(N, H_, S)
        assert fn(1, 32, 513) == 32 * 5 * 130 * 4


def test_the_symbols_are_declared_in_the_header_and_the_signature_table():
    from otter_amd import _capi

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    for sym in ("otter_decode_attn_cached_i8", "otter_decode_attn_cached_i8_dyn"):
        assert re.search(r"^int %s\(" % sym, hdr, re.M) and sym in _capi.SIGNATURES
        decl = re.search(r"^int %s\((.*?)\);" % sym, hdr, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_capi.SIGNATURES[sym][1]) == 39
    assert _capi.ABI_VERSION == 3                                     # symbols were only added
