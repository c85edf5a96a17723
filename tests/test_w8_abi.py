"""CPU: otter_gemv_w8 / otter_dequant_w8 (csrc/w8.hip) validate their arguments before anything is launched -- negative status and a
message, no GPU needed.  Device pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them."""
import os
import re

import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def gemv(lib, **over):
    a = dict(x=P, ldx=64, qweight=P, ldw=64, scale=P, bias=None, bias_dtype=0, y=P, ldy=32, y_dtype=1, M=4, N=32, K=64, act=0, ws=P,
             ws_bytes=1 << 20)
    a.update(over)
    return lib.otter_gemv_w8(a["x"], a["ldx"], a["qweight"], a["ldw"], a["scale"], a["bias"], a["bias_dtype"], a["y"], a["ldy"], a["y_dtype"],
                             a["M"], a["N"], a["K"], a["act"], a["ws"], a["ws_bytes"], None)


def dequant(lib, **over):
    a = dict(qweight=P, ldw=64, scale=P, out=P, ldo=64, N=32, K=64)
    a.update(over)
    return lib.otter_dequant_w8(a["qweight"], a["ldw"], a["scale"], a["out"], a["ldo"], a["N"], a["K"], None)


def test_symbols_are_declared_and_the_abi_version_is_unchanged(lib):
    from otter_amd import _capi

    assert "otter_gemv_w8" in _capi.SIGNATURES and "otter_dequant_w8" in _capi.SIGNATURES
    assert lib.otter_abi_version() == 3            # purely additive: no existing signature moved


@pytest.mark.parametrize("name", ["x", "qweight", "scale", "y", "ws"])
def test_null_pointers_are_rejected(lib, name):
    assert gemv(lib, **{name: None}) == -1
    assert b"null pointer" in lib.otter_last_error()


@pytest.mark.parametrize("M", [0, 17, -1])
def test_row_count_outside_1_to_16_is_rejected(lib, M):
    assert gemv(lib, M=M) == -1
    assert b"M=%d" % M in lib.otter_last_error()


def test_k_not_a_multiple_of_16_is_rejected(lib):
    assert gemv(lib, K=24, ldw=32, ldx=32) == -1
    assert b"K=24" in lib.otter_last_error()
    assert gemv(lib, K=0) == -1
    assert b"K=0" in lib.otter_last_error()


def test_alignment_rules(lib):
    assert gemv(lib, qweight=P + 4) == -1
    assert b"alignment" in lib.otter_last_error()
    assert gemv(lib, K=16, ldw=20, ldx=16) == -1
    assert b"alignment" in lib.otter_last_error()
    assert gemv(lib, x=P + 2) == -1
    assert b"alignment" in lib.otter_last_error()
    assert gemv(lib, y=P + 8) == -1
    assert b"alignment" in lib.otter_last_error()
    assert gemv(lib, ldx=68) == -1
    assert b"alignment" in lib.otter_last_error()


def test_too_small_workspace_is_rejected(lib):
    assert gemv(lib, ws_bytes=8 * 4 * 32 * 4 - 1) == -1
    assert b"workspace" in lib.otter_last_error()


def test_leading_dimensions_and_flags(lib):
    assert gemv(lib, ldy=16) == -1
    assert b"leading dimension" in lib.otter_last_error()
    assert gemv(lib, act=2) == -1
    assert b"act=2" in lib.otter_last_error()
    assert gemv(lib, y_dtype=7) == -1
    assert b"dtype" in lib.otter_last_error()


def test_dequant_argument_rules(lib):
    for name in ("qweight", "scale", "out"):
        assert dequant(lib, **{name: None}) == -1
        assert b"null pointer" in lib.otter_last_error()
    assert dequant(lib, K=24, ldw=32) == -1
    assert b"K=24" in lib.otter_last_error()
    assert dequant(lib, ldw=72) == -1
    assert b"alignment" in lib.otter_last_error()
    assert dequant(lib, out=P + 2) == -1
    assert b"alignment" in lib.otter_last_error()
    assert dequant(lib, ldo=48) == -1
    assert b"leading dimension" in lib.otter_last_error()


def test_workspace_formula_matches_the_header():
    from otter_amd import ops

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")).read()
    m = re.search(r"#define OTTER_GEMV_W8_WORKSPACE_BYTES\(M, N, K\) (.*)", hdr)
    expr = m.group(1).split("/*")[0].replace("(int64_t)", "").replace("/", "//")
    for M, N, K in [(1, 4096, 4096), (16, 4096, 16384), (5, 22016, 4096)]:
        assert eval(expr, {"M": M, "N": N, "K": K}) == ops.gemv_w8_workspace_bytes(M, N, K) > 0


def test_wrappers_refuse_cpu_tensors():
    """No CPU fallback behind the ops wrappers themselves (the CPU branch lives in quant.Int8FrozenLinear, in torch ops)."""
    import torch

    from otter_amd import _capi, ops

    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        ops.gemv_w8(torch.zeros(2, 32, dtype=torch.bfloat16), torch.zeros(16, 32, dtype=torch.int8), torch.ones(16))
    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        ops.dequant_w8(torch.zeros(16, 32, dtype=torch.int8), torch.ones(16))
