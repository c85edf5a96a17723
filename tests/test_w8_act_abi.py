"""CPU: the `act` argument of otter_gemv_w8 / otter_gemm_w8_rows (csrc/w8.hip) after the squared-ReLU epilogue: code 3 passes the
argument check (the call then fails on the next rule it breaks, the workspace size), every code other than 0, 1 and 3 is still an
argument error that names `act`.  Code 2 is pinned by tests/test_w8_abi.py and tests/test_w8_rows_abi.py.  Nothing is launched: device
pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them."""
import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, name, **over):
    a = dict(x=P, ldx=64, qweight=P, ldw=64, scale=P, bias=P, bias_dtype=0, y=P, ldy=32, y_dtype=1, M=4, N=32, K=64, act=0, ws=P, ws_bytes=1 << 20)
    a.update(over)
    return getattr(lib, name)(a["x"], a["ldx"], a["qweight"], a["ldw"], a["scale"], a["bias"], a["bias_dtype"], a["y"], a["ldy"], a["y_dtype"],
                              a["M"], a["N"], a["K"], a["act"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("name", ["otter_gemv_w8", "otter_gemm_w8_rows"])
def test_act_3_is_accepted_by_the_argument_check(lib, name):
    assert call(lib, name, act=3, ws_bytes=0) == -1
    err = lib.otter_last_error()
    assert b"workspace" in err and b"act" not in err, err


@pytest.mark.parametrize("name", ["otter_gemv_w8", "otter_gemm_w8_rows"])
@pytest.mark.parametrize("act", [4, -1])
def test_other_codes_are_rejected(lib, name, act):
    assert call(lib, name, act=act) == -1
    assert b"act=%d" % act in lib.otter_last_error()


def test_the_abi_version_is_unchanged(lib):
    assert lib.otter_abi_version() == 3            # a new value of an existing argument: no signature moved, no new symbol
