"""CPU: otter_logits_process (csrc/logits.hip) is declared, bound and exported, and validates its arguments before anything is launched --
negative status and a message, no GPU needed.  Device pointers are never dereferenced on these paths, so aligned dummy addresses stand in
for them."""
import os
import re

import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, **over):
    a = dict(scores=P, s_rs=128, ids=P, i_rs=16, N=2, V=97, L=12, p=1.3, n=3, ban=P, n_ban=1, eos=P, n_eos=1, sup=1, tok=P, off=P, n_words=1)
    a.update(over)
    return lib.otter_logits_process(a["scores"], a["s_rs"], a["ids"], a["i_rs"], a["N"], a["V"], a["L"], a["p"], a["n"], a["ban"], a["n_ban"],
                                    a["eos"], a["n_eos"], a["sup"], a["tok"], a["off"], a["n_words"], None)


def test_symbol_is_in_the_header_the_ctypes_table_and_the_library(lib):
    from otter_amd import _capi

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "otter_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+otter_logits_process\s*\(", hdr)
    assert "otter_logits_process" in _capi.SIGNATURES
    assert hasattr(lib, "otter_logits_process")
    assert lib.otter_abi_version() == 3            # purely additive: no existing signature moved
    assert "logits.hip" in __import__("otter_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("name", ["scores", "ids"])
def test_null_tensors_are_rejected(lib, name):
    assert call(lib, **{name: None}) == -1
    assert b"null pointer" in lib.otter_last_error()


@pytest.mark.parametrize("name,count", [("ban", "n_ban"), ("eos", "n_eos")])
def test_a_non_empty_list_needs_its_pointer_and_an_empty_one_does_not(lib, name, count):
    assert call(lib, **{name: None}) == -1
    assert b"null pointer" in lib.otter_last_error()
    assert call(lib, **{name: None, count: 0, "V": 0}) == -1          # (the V check, reached only past the pointer checks)
    assert b"V=0" in lib.otter_last_error()


def test_offsets_are_required_whenever_words_are(lib):
    assert call(lib, off=None) == -1
    assert b"word_offsets" in lib.otter_last_error()
    assert call(lib, tok=None) == -1
    assert b"word_tokens" in lib.otter_last_error()
    assert call(lib, tok=None, off=None, n_words=0, L=0) == -1
    assert b"L=0" in lib.otter_last_error()


def test_negative_list_lengths_are_rejected(lib):
    for count in ("n_ban", "n_eos", "n_words"):
        assert call(lib, **{count: -1}) == -1
        assert b"list lengths" in lib.otter_last_error()


@pytest.mark.parametrize("N", [0, -1, 1 << 31])
def test_row_count_range(lib, N):
    assert call(lib, N=N) == -1
    assert b"N=%d" % N in lib.otter_last_error()


@pytest.mark.parametrize("V", [0, -5, 262145])
def test_vocabulary_range_is_the_bitmap(lib, V):
    assert call(lib, V=V, s_rs=1 << 20) == -1
    assert b"V=%d" % V in lib.otter_last_error()


@pytest.mark.parametrize("L", [0, -1, (1 << 30) + 1])
def test_history_length_range(lib, L):
    assert call(lib, L=L, i_rs=1 << 31) == -1
    assert b"L=%d" % L in lib.otter_last_error()


def test_row_strides_cover_the_rows(lib):
    assert call(lib, s_rs=96) == -1
    assert b"row stride" in lib.otter_last_error()
    assert call(lib, i_rs=11) == -1
    assert b"row stride" in lib.otter_last_error()


@pytest.mark.parametrize("p", [0.0, -1.3, float("inf"), float("nan")])
def test_penalty_must_be_finite_and_positive(lib, p):
    assert call(lib, p=p) == -1
    assert b"repetition_penalty" in lib.otter_last_error()


def test_negative_ngram_is_rejected(lib):
    assert call(lib, n=-1) == -1
    assert b"no_repeat_ngram=-1" in lib.otter_last_error()


@pytest.mark.parametrize("name,addr", [("scores", P + 2), ("ids", P + 4), ("ban", P + 1), ("eos", P + 2), ("tok", P + 2), ("off", P + 3)])
def test_alignment_rules(lib, name, addr):
    assert call(lib, **{name: addr}) == -1
    assert b"alignment" in lib.otter_last_error()


def test_the_first_failing_check_names_the_error(lib):
    assert call(lib, scores=None, V=0, p=0.0) == -1
    assert b"null pointer" in lib.otter_last_error()
    assert call(lib, V=0, p=0.0, scores=P + 2) == -1
    assert b"V=0" in lib.otter_last_error()
    assert call(lib, p=0.0, scores=P + 2) == -1
    assert b"repetition_penalty" in lib.otter_last_error()


def test_wrapper_refuses_cpu_tensors_and_wrong_types():
    """No CPU fallback behind the ops wrapper itself (the CPU branch is generation._Processors' host loop)."""
    import torch

    from otter_amd import _capi, ops

    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        ops.logits_process(torch.zeros(2, 97), torch.zeros(2, 5, dtype=torch.long), 1.3, 3)
    assert ops.LOGITS_PROCESS_MAX_VOCAB == 262144
