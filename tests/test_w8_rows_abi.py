"""CPU: otter_gemm_w8_rows (csrc/w8.hip) validates its arguments before anything is launched -- negative status and a message, no GPU
needed (device pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them) -- and quant.route, the
pure function behind Int8FrozenLinear.forward's choice between the GEMV, the rows kernel and dequantise-and-GEMM."""
import os
import re

import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def rows(lib, **over):
    a = dict(x=P, ldx=64, qweight=P, ldw=64, scale=P, bias=None, bias_dtype=0, y=P, ldy=32, y_dtype=1, M=24, N=32, K=64, act=0, ws=P,
             ws_bytes=1 << 20)
    a.update(over)
    return lib.otter_gemm_w8_rows(a["x"], a["ldx"], a["qweight"], a["ldw"], a["scale"], a["bias"], a["bias_dtype"], a["y"], a["ldy"],
                                  a["y_dtype"], a["M"], a["N"], a["K"], a["act"], a["ws"], a["ws_bytes"], None)


def test_symbol_is_declared_and_the_abi_version_is_unchanged(lib):
    from otter_amd import _capi

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    assert re.search(r"^int otter_gemm_w8_rows\(", hdr, re.M)
    assert "otter_gemm_w8_rows" in _capi.SIGNATURES
    assert _capi.SIGNATURES["otter_gemm_w8_rows"] == _capi.SIGNATURES["otter_gemv_w8"]        # otter_gemv_w8's argument list
    assert lib.otter_abi_version() == 3            # purely additive: no existing signature moved


def test_workspace_formula_matches_the_header():
    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    m = re.search(r"#define OTTER_GEMM_W8_ROWS_WORKSPACE_BYTES\(M, N, K\) (.*)", hdr)
    expr = m.group(1).split("/*")[0].replace("(int64_t)", "").replace("/", "//")
    for M, N, K in [(17, 4096, 4096), (64, 4096, 16384), (24, 22016, 4096)]:
        assert eval(expr, {"M": M, "N": N, "K": K}) == ops.gemm_w8_rows_workspace_bytes(M, N, K) > 0
    assert ops.GEMM_W8_ROWS_MAX_ROWS == 64


@pytest.mark.parametrize("name", ["x", "qweight", "scale", "y", "ws"])
def test_null_pointers_are_rejected(lib, name):
    assert rows(lib, **{name: None}) == -1
    assert b"gemm_w8_rows" in lib.otter_last_error() and b"null pointer" in lib.otter_last_error()


@pytest.mark.parametrize("M", [0, 65, -1])
def test_row_count_outside_1_to_64_is_rejected(lib, M):
    assert rows(lib, M=M) == -1
    assert b"M=%d" % M in lib.otter_last_error()


@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_row_counts_inside_1_to_64_pass_the_row_check(lib, M):
    """(the call still fails, on the workspace, which is checked last: nothing is launched from this test)"""
    assert rows(lib, M=M, ws_bytes=0) == -1
    assert b"workspace" in lib.otter_last_error()


def test_k_not_a_multiple_of_16_is_rejected(lib):
    assert rows(lib, K=24, ldw=32, ldx=32) == -1
    assert b"K=24" in lib.otter_last_error()
    assert rows(lib, K=0) == -1
    assert b"K=0" in lib.otter_last_error()


def test_alignment_rules(lib):
    assert rows(lib, qweight=P + 4) == -1
    assert b"alignment" in lib.otter_last_error()
    assert rows(lib, K=16, ldw=20, ldx=16) == -1
    assert b"alignment" in lib.otter_last_error()
    assert rows(lib, x=P + 2) == -1
    assert b"alignment" in lib.otter_last_error()
    assert rows(lib, y=P + 8) == -1
    assert b"alignment" in lib.otter_last_error()
    assert rows(lib, ldx=68) == -1
    assert b"alignment" in lib.otter_last_error()


def test_too_small_workspace_is_rejected(lib):
    assert rows(lib, ws_bytes=8 * 24 * 32 * 4 - 1) == -1
    assert b"workspace" in lib.otter_last_error()


def test_leading_dimensions_and_flags(lib):
    assert rows(lib, ldy=16) == -1
    assert b"leading dimension" in lib.otter_last_error()
    assert rows(lib, act=2) == -1
    assert b"act=2" in lib.otter_last_error()
    assert rows(lib, y_dtype=7) == -1
    assert b"dtype" in lib.otter_last_error()


def test_wrapper_refuses_cpu_tensors():
    import torch

    from otter_amd import _capi, ops

    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        ops.gemm_w8_rows(torch.zeros(24, 32, dtype=torch.bfloat16), torch.zeros(16, 32, dtype=torch.int8), torch.ones(16))


@pytest.mark.parametrize("n_rows,one_token,want", [
    (1, True, "gemv"), (16, True, "gemv"), (16, False, "gemv"),
    (17, True, "rows"), (24, True, "rows"), (64, True, "rows"),
    (65, True, "dequant"), (17, False, "dequant"), (24, False, "dequant"), (96, False, "dequant")])
def test_route(monkeypatch, n_rows, one_token, want):
    from otter_amd import quant

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    assert quant.route(n_rows, one_token) == want


def test_route_with_the_rows_kernel_switched_off(monkeypatch):
    from otter_amd import quant

    monkeypatch.setenv("OTTER_W8_ROWS", "0")
    assert quant.route(24, True) == "dequant"
    assert quant.route(16, True) == "gemv" and quant.route(96, False) == "dequant"       # the other cases do not move
    monkeypatch.setenv("OTTER_W8_ROWS", "1")
    assert quant.route(24, True) == "rows"
