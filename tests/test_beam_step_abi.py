"""CPU: otter_beam_step (csrc/beam.hip) is declared, bound and exported, and validates its arguments before anything is launched, the first
failing check first -- negative status and a message, no GPU needed.  Device pointers are never dereferenced on these paths, so aligned dummy
addresses stand in for them."""
import os
import re

import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER = ("logp", "lp_rs", "beam_scores", "ids", "i_rs", "ids_next", "n_rs", "beam_idx", "eos", "n_eos", "pad", "B", "nb", "V", "n_cand", "L", "L0",
         "max_len", "early", "lp_pos", "len_pow", "done", "hyp_score", "hyp_tokens", "hyp_len", "hyp_slot", "hyp_count", "hyp_worst", "all_done",
         "ws", "ws_bytes")
POINTERS = ("logp", "beam_scores", "ids", "ids_next", "beam_idx", "len_pow", "done", "hyp_score", "hyp_tokens", "hyp_len", "hyp_slot", "hyp_count",
            "hyp_worst", "all_done")


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, **over):
    # B = 2 sentences of nb = 3 beams over V = 97, one eos id: n_cand = 6; ids [6, 12] in rows of 16, ids_next far behind it
    a = dict(logp=P, lp_rs=128, beam_scores=P, ids=P, i_rs=16, ids_next=P + (1 << 16), n_rs=16, beam_idx=P, eos=P, n_eos=1, pad=0, B=2, nb=3, V=97,
             n_cand=6, L=12, L0=5, max_len=16, early=0, lp_pos=1, len_pow=P, done=P, hyp_score=P, hyp_tokens=P, hyp_len=P, hyp_slot=P, hyp_count=P,
             hyp_worst=P, all_done=P, ws=P, ws_bytes=1 << 20)
    a.update(over)
    return lib.otter_beam_step(*[a[k] for k in ORDER], None)


def test_symbol_is_in_the_header_the_ctypes_table_and_the_library(lib):
    from otter_amd import _capi, ops

    raw = open(os.path.join(ROOT, "include", "otter_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"\bint\s+otter_beam_step\s*\((.*?)\)\s*;", hdr, flags=re.S)
    assert m and re.search(r"\bint64_t\s+otter_beam_step_workspace_bytes\s*\(", hdr)
    # the header's parameter list against the ctypes row, type by type
    import ctypes as C

    kinds = []
    for prm in m.group(1).split(","):
        prm = " ".join(prm.split())
        kinds.append(C.c_void_p if "*" in prm else C.c_int64 if prm.startswith("int64_t ") else C.c_int if prm.startswith("int ") else prm)
    res, args = _capi.SIGNATURES["otter_beam_step"]
    assert res is C.c_int and args == kinds and len(args) == len(ORDER) + 1
    assert _capi.SIGNATURES["otter_beam_step_workspace_bytes"] == (C.c_int64, [C.c_int64] * 4)
    assert hasattr(lib, "otter_beam_step") and hasattr(lib, "otter_beam_step_workspace_bytes")
    assert lib.otter_abi_version() == 3            # purely additive: no existing signature moved
    assert "beam.hip" in __import__("otter_amd.build", fromlist=["SOURCES"]).SOURCES
    cap = int(re.search(r"^#define\s+OTTER_BEAM_STEP_MAX_CANDIDATES\s+(\d+)", raw, re.M).group(1))
    assert ops.BEAM_STEP_MAX_CANDIDATES == cap == 64
    assert "smaller flat index" in raw                                       # the tie rule is stated where the ABI is


@pytest.mark.parametrize("name", POINTERS + ("ws",))
def test_null_pointers_are_rejected(lib, name):
    assert call(lib, **{name: None}) == -1
    assert b"null pointer" in lib.otter_last_error()


def test_the_eos_list_needs_its_pointer_only_when_it_is_not_empty(lib):
    assert call(lib, eos=None) == -1
    assert b"null pointer for a non-empty list" in lib.otter_last_error()
    assert call(lib, eos=None, n_eos=0, V=0) == -1                           # (the V check, reached only past the pointer checks)
    assert b"V=0" in lib.otter_last_error()
    assert call(lib, n_eos=-1) == -1
    assert b"n_eos=-1" in lib.otter_last_error()


@pytest.mark.parametrize("name,addr", [("logp", P + 2), ("beam_scores", P + 1), ("eos", P + 2), ("done", P + 2), ("hyp_len", P + 1), ("hyp_slot", P + 3),
                                       ("hyp_count", P + 2), ("all_done", P + 2), ("ids", P + 4), ("ids_next", P + (1 << 16) + 4), ("beam_idx", P + 4),
                                       ("len_pow", P + 4), ("hyp_score", P + 4), ("hyp_tokens", P + 4), ("hyp_worst", P + 4), ("ws", P + 4)])
def test_alignment_rules(lib, name, addr):
    assert call(lib, **{name: addr}) == -1
    assert b"alignment" in lib.otter_last_error()


@pytest.mark.parametrize("B", [0, -1, 1 << 31])
def test_sentence_count_range(lib, B):
    assert call(lib, B=B) == -1
    assert b"B=%d" % B in lib.otter_last_error()


@pytest.mark.parametrize("V", [0, -5, 1 << 31])
def test_vocabulary_range(lib, V):
    assert call(lib, V=V, lp_rs=1 << 32) == -1
    assert b"V=%d" % V in lib.otter_last_error()


@pytest.mark.parametrize("nb,n_cand", [(0, 6), (-1, 6), (3, 2), (3, 0), (3, 3 * 97 + 1), (1, 98)])
def test_beams_and_candidates(lib, nb, n_cand):
    assert call(lib, nb=nb, n_cand=n_cand) == -1
    assert b"nb=%d" % nb in lib.otter_last_error() and b"n_cand=%d" % n_cand in lib.otter_last_error()


def test_candidate_cap_and_index_limits(lib):
    assert call(lib, nb=5, n_cand=65) == -1
    assert b"cap of 64" in lib.otter_last_error()
    assert call(lib, nb=5, n_cand=64, ws_bytes=0) == -1                      # 64 itself passes the cap
    assert b"workspace" in lib.otter_last_error()
    assert call(lib, nb=3, V=(1 << 30), lp_rs=1 << 30) == -1
    assert b"2^31-1" in lib.otter_last_error() and b"flat index" in lib.otter_last_error()
    assert call(lib, B=30000, nb=3) == -1
    assert b"65535" in lib.otter_last_error()


@pytest.mark.parametrize("L,max_len", [(0, 16), (-1, 16), (16, 16), (17, 16), (12, 1 << 31)])
def test_history_length_range(lib, L, max_len):
    assert call(lib, L=L, max_len=max_len, L0=1, i_rs=1 << 32, n_rs=1 << 32) == -1
    assert b"L=%d" % L in lib.otter_last_error()


@pytest.mark.parametrize("L0", [0, -1, 13])
def test_prompt_length_range(lib, L0):
    assert call(lib, L0=L0) == -1
    assert b"L0=%d" % L0 in lib.otter_last_error()


@pytest.mark.parametrize("over", [dict(lp_rs=96), dict(i_rs=11), dict(n_rs=12)])
def test_row_strides_cover_the_rows(lib, over):
    assert call(lib, **over) == -1
    assert b"row stride" in lib.otter_last_error()


@pytest.mark.parametrize("ids_next", [P, P + 8 * 12, P + 8 * (5 * 16 + 11), P - 8 * (5 * 16 + 12)])
def test_ids_and_ids_next_must_not_overlap(lib, ids_next):
    assert call(lib, ids_next=ids_next) == -1
    assert b"overlap" in lib.otter_last_error()


def test_ids_next_may_touch_ids(lib):
    for ids_next in (P + 8 * (5 * 16 + 12), P - 8 * (5 * 16 + 13)):          # directly behind / directly in front of ids [6 rows of 16, 12 used]
        assert call(lib, ids_next=ids_next, ws_bytes=0) == -1
        assert b"workspace" in lib.otter_last_error()


@pytest.mark.parametrize("early", [-1, 3])
def test_early_stopping_mode(lib, early):
    assert call(lib, early=early) == -1
    assert b"early_stopping=%d" % early in lib.otter_last_error()


def test_workspace_size_and_its_query(lib):
    need = lib.otter_beam_step_workspace_bytes(2, 3, 97, 6)
    assert need == 2 * 3 * 1 * 6 * 8
    assert lib.otter_beam_step_workspace_bytes(1, 3, 262144, 6) == 3 * 64 * 6 * 8      # 4096 columns per chunk
    assert lib.otter_beam_step_workspace_bytes(1, 3, 4097, 6) == 3 * 2 * 6 * 8
    for bad in ((0, 3, 97, 6), (2, 0, 97, 6), (2, 3, 0, 6), (2, 3, 97, 0), (2, 3, 97, 65)):
        assert lib.otter_beam_step_workspace_bytes(*bad) == -1
    assert call(lib, ws_bytes=need - 1) == -1
    assert b"%d needed" % need in lib.otter_last_error()


def test_the_first_failing_check_names_the_error(lib):
    chain = [("logp", None, b"null pointer (logp"), ("len_pow", None, b"null pointer (len_pow"), ("n_eos", -1, b"list length"),
             ("eos", None, b"non-empty list"), ("ws", None, b"null pointer (workspace)"), ("done", P + 2, b"alignment"), ("B", 0, b"B=0"),
             ("V", 0, b"V=0"), ("nb", 0, b"nb=0"), ("n_cand", 65, None), ("L", 0, b"L=0"), ("L0", 0, b"L0=0"), ("i_rs", -1, b"row stride"),
             ("early", 7, b"early_stopping=7"), ("ws_bytes", 0, b"workspace")]
    # every failure from the i-th on is present: the i-th is the one reported (n_cand=65 hides behind nb=0 and is skipped as a reporter)
    for i, (_, _, msg) in enumerate(chain):
        if msg is None:
            continue
        over = {k: v for k, v, _ in chain[i:]}
        if "nb" not in over:
            over.pop("n_cand", None)                                         # n_cand=65 with nb=3 fails the cap check, which sits before L
        assert call(lib, **over) == -1
        assert msg in lib.otter_last_error(), (i, lib.otter_last_error())


def test_wrapper_refuses_cpu_tensors():
    """No CPU fallback behind the ops wrapper itself (the CPU branch is generate_tokens' host block)."""
    import torch

    from otter_amd import _capi, ops

    N, V, L, max_len, nb = 6, 97, 12, 16, 3
    i32, f64 = torch.int32, torch.float64
    z = lambda n, dt: torch.zeros(n, dtype=dt)
    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        ops.beam_step(torch.zeros(N, V), z(N, torch.float32), z((N, L), torch.long), z((N, L + 1), torch.long), z(N, torch.long), None, 0, nb, 6, 5,
                      max_len, False, True, z(max_len - 5 + 1, f64), z(2, i32), z(N, f64), z(N * max_len, torch.long), z(N, i32), z(N, i32), z(2, i32),
                      z(2, f64), z(2, i32), z(1024, torch.uint8))
    with pytest.raises(_capi.OtterHipError, match="out of range"):
        ops.beam_step_workspace_bytes(2, 3, 97, 65)
    assert ops.beam_step_workspace_bytes(2, 3, 97, 6) == 288
