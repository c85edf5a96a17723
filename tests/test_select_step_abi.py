"""CPU: otter_select_step (csrc/select.hip) is declared, bound and exported, and validates its arguments before anything is launched -- negative
status and a message, the first failing check first, no GPU needed.  Device pointers are never dereferenced on these paths, so aligned dummy
addresses stand in for them."""
import ctypes as C
import os
import re

import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEDY, SAMPLE = 0, 1


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, **over):
    a = dict(scores=P, s_rs=128, N=2, V=97, ids=P, i_rs=32, L=12, max_len=20, mode=SAMPLE, inv_t=1.25, top_k=50, top_p=0.9, q=P, q_rs=128,
             unf=P, n_unf=P, eos=P, n_eos=1, pad=0)
    a.update(over)
    return lib.otter_select_step(a["scores"], a["s_rs"], a["N"], a["V"], a["ids"], a["i_rs"], a["L"], a["max_len"], a["mode"], a["inv_t"],
                                 a["top_k"], a["top_p"], a["q"], a["q_rs"], a["unf"], a["n_unf"], a["eos"], a["n_eos"], a["pad"], None)


def test_symbol_is_in_the_header_the_ctypes_table_and_the_library(lib):
    from otter_amd import _capi, ops

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "otter_hip.h")).read(), flags=re.S)
    decl = re.search(r"\bint\s+otter_select_step\s*\(([^;]*)\)\s*;", hdr).group(1)
    res, args = _capi.SIGNATURES["otter_select_step"]
    assert res is C.c_int and len(decl.split(",")) == len(args) == 20
    kinds = []
    for piece in decl.split(","):
        piece = piece.strip()
        kinds.append(C.c_void_p if "*" in piece else {"int64_t": C.c_int64, "int": C.c_int, "float": C.c_float, "double": C.c_double}[piece.split()[0]])
    assert kinds == args                                   # the header row agrees with the ctypes row, argument by argument
    assert hasattr(lib, "otter_select_step")
    assert lib.otter_abi_version() == 3                    # purely additive: no existing signature moved
    assert "select.hip" in __import__("otter_amd.build", fromlist=["SOURCES"]).SOURCES
    m = re.search(r"^#define\s+OTTER_SELECT_STEP_MAX_VOCAB\s+(\d+)", open(os.path.join(ROOT, "include", "otter_hip.h")).read(), re.M)
    assert int(m.group(1)) == ops.SELECT_STEP_MAX_VOCAB == ops.LOGITS_PROCESS_MAX_VOCAB == 262144


@pytest.mark.parametrize("name", ["scores", "ids", "unf", "n_unf"])
def test_null_tensors_are_rejected(lib, name):
    assert call(lib, **{name: None}) == -1
    assert b"null pointer" in lib.otter_last_error()


def test_mode_is_greedy_or_sample(lib):
    for mode in (-1, 2):
        assert call(lib, mode=mode) == -1
        assert b"mode=%d" % mode in lib.otter_last_error()


@pytest.mark.parametrize("N", [0, -1, 1 << 31])
def test_row_count_range(lib, N):
    assert call(lib, N=N) == -1
    assert b"N=%d" % N in lib.otter_last_error()


@pytest.mark.parametrize("V", [0, -5, 262145])
def test_vocabulary_range(lib, V):
    assert call(lib, V=V, s_rs=1 << 20, q_rs=1 << 20) == -1
    assert b"V=%d" % V in lib.otter_last_error()


@pytest.mark.parametrize("max_len", [0, -3, (1 << 30) + 1])
def test_history_length_range(lib, max_len):
    assert call(lib, max_len=max_len, L=0, i_rs=1 << 31) == -1
    assert b"max_len=%d" % max_len in lib.otter_last_error()


@pytest.mark.parametrize("L", [-1, 20, 21])
def test_the_written_column_lies_inside_the_history(lib, L):
    assert call(lib, L=L) == -1
    assert b"L=%d" % L in lib.otter_last_error()
    assert call(lib, L=19, V=0) == -1                      # the last column is accepted: the V check is not reached before the L check
    assert b"V=0" in lib.otter_last_error()


def test_row_strides_cover_the_rows(lib):
    assert call(lib, s_rs=96) == -1
    assert b"row stride" in lib.otter_last_error() and b"scores" in lib.otter_last_error()
    assert call(lib, i_rs=19) == -1
    assert b"row stride" in lib.otter_last_error() and b"ids_buf" in lib.otter_last_error()
    assert call(lib, q_rs=96) == -1
    assert b"row stride" in lib.otter_last_error() and b"(q " in lib.otter_last_error()


def test_top_k_must_not_be_negative(lib):
    assert call(lib, top_k=-1) == -1
    assert b"top_k=-1" in lib.otter_last_error()
    assert call(lib, top_k=0, top_p=2.0) == -1             # 0 = off is accepted
    assert b"top_p" in lib.otter_last_error()


@pytest.mark.parametrize("top_p", [0.0, -0.5, 1.0000001, float("nan"), float("inf")])
def test_top_p_lies_in_0_1(lib, top_p):
    assert call(lib, top_p=top_p) == -1
    assert b"top_p" in lib.otter_last_error()


@pytest.mark.parametrize("inv_t", [0.0, -1.0, float("inf"), float("nan")])
def test_inverse_temperature_must_be_finite_and_positive(lib, inv_t):
    assert call(lib, inv_t=inv_t) == -1
    assert b"inv_temperature" in lib.otter_last_error()


def test_sample_mode_needs_the_draws_and_greedy_mode_reads_no_sample_argument(lib):
    assert call(lib, q=None) == -1
    assert b"needs q" in lib.otter_last_error()
    # greedy: q, top_k, top_p and inv_temperature are not looked at -- the next check (the eos list) is what fails
    assert call(lib, mode=GREEDY, q=None, q_rs=0, top_k=-1, top_p=7.0, inv_t=0.0, n_eos=-1) == -1
    assert b"n_eos=-1" in lib.otter_last_error()


def test_the_eos_list(lib):
    assert call(lib, n_eos=-1) == -1
    assert b"n_eos=-1" in lib.otter_last_error()
    assert call(lib, eos=None) == -1
    assert b"eos list" in lib.otter_last_error()
    assert call(lib, eos=None, n_eos=0, scores=P + 2) == -1          # an empty list needs no pointer: the alignment check is reached
    assert b"alignment" in lib.otter_last_error()


@pytest.mark.parametrize("name,addr", [("scores", P + 2), ("q", P + 1), ("ids", P + 4), ("n_unf", P + 2), ("eos", P + 3)])
def test_alignment_rules(lib, name, addr):
    assert call(lib, **{name: addr}) == -1
    assert b"alignment" in lib.otter_last_error()


def test_the_first_failing_check_names_the_error(lib):
    order = [("scores", None, b"null pointer"), ("mode", 5, b"mode=5"), ("N", 0, b"N=0"), ("V", 0, b"V=0"), ("max_len", 0, b"max_len=0"),
             ("L", 20, b"L=20"), ("i_rs", 19, b"row stride"), ("top_k", -2, b"top_k=-2"), ("top_p", 0.0, b"top_p"), ("inv_t", 0.0, b"inv_temperature"),
             ("q", None, b"needs q"), ("q_rs", 5, b"(q "), ("n_eos", -1, b"n_eos=-1"), ("eos", None, b"eos list"), ("n_unf", P + 2, b"alignment")]
    for first in range(len(order)):
        bad = {name: value for name, value, _ in order[first:]}
        assert call(lib, **bad) == -1
        assert order[first][2] in lib.otter_last_error(), (order[first][0], lib.otter_last_error())


def test_wrapper_refuses_cpu_tensors_and_wrong_types():
    """No CPU fallback behind the ops wrapper itself (the CPU branches are generation's host block and _select_reference)."""
    import torch

    from otter_amd import _capi, ops

    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        ops.select_step(torch.zeros(2, 97), torch.zeros(2, 8, dtype=torch.long), 3, torch.ones(2, dtype=torch.bool),
                        torch.full((1,), 2, dtype=torch.int32))
