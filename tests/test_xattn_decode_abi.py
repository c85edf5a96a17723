"""CPU: otter_xattn_decode (csrc/xattn_decode.hip) validates its arguments before anything is launched -- negative status and a message, no GPU
needed.  Device pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them."""
import pytest

from otter_amd._capi import MASK_EQ, MASK_GE, MASK_NONE

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
H = 2


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, **over):
    a = dict(q=P, q_rs=3 * H * 64, k=P, v=P + 2 * H * 64, kv_rs=2 * H * 64, tt=P, o=P, N=6, H=H, T_img=2, n=24, rpm=3, mode=MASK_EQ, scale=0.125)
    a.update(over)
    return lib.otter_xattn_decode(a["q"], a["q_rs"], a["k"], a["v"], a["kv_rs"], a["tt"], a["o"], a["N"], a["H"], a["T_img"], a["n"], a["rpm"],
                                  a["mode"], a["scale"], None)


@pytest.mark.parametrize("name", ["q", "k", "v", "tt", "o"])
def test_null_pointers_are_rejected(lib, name):
    assert call(lib, **{name: None}) == -1
    assert b"null pointer" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q", "k", "v"])
def test_misaligned_pointers_are_rejected(lib, name):
    assert call(lib, **{name: P + 2}) == -1
    assert b"16-byte alignment" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q_rs", "kv_rs"])
def test_strides_that_are_not_multiples_of_8_are_rejected(lib, name):
    assert call(lib, **{name: 3 * H * 64 + 4}) == -1
    assert b"multiples of 8" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q_rs", "kv_rs"])
def test_row_strides_below_the_row_are_rejected(lib, name):
    assert call(lib, **{name: H * 64 - 8}) == -1
    assert b"below H * 64" in lib.otter_last_error()


def test_rows_must_be_whole_sentences(lib):
    assert call(lib, N=7) == -1
    assert b"not a multiple of rows_per_media" in lib.otter_last_error()
    assert call(lib, rpm=0) == -1
    assert b"rows_per_media" in lib.otter_last_error()
    assert call(lib, N=0) == -1
    assert b"bad shape" in lib.otter_last_error()


@pytest.mark.parametrize("mode", [MASK_NONE, 3, -1])
def test_mask_modes_other_than_eq_and_ge_are_rejected(lib, mode):
    assert MASK_GE == 2
    assert call(lib, mode=mode) == -1
    assert b"mask_mode" in lib.otter_last_error()


def test_media_geometry_rules(lib):
    assert call(lib, n=0) == -1
    assert b"n_per_media=0" in lib.otter_last_error()
    assert call(lib, n=-3) == -1
    assert b"must be >= 1" in lib.otter_last_error()
    assert call(lib, T_img=0) == -1
    assert b"T_img=0" in lib.otter_last_error()
    assert call(lib, T_img=1025, n=64) == -1                       # M = 65600 > 65536
    assert b"exceeds 65536" in lib.otter_last_error()
    assert call(lib, T_img=1 << 40, n=1 << 40) == -1               # (no overflow of the product)
    assert b"exceeds 65536" in lib.otter_last_error()
