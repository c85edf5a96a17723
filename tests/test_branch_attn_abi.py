"""CPU: otter_branch_attn_merge (csrc/branch_attn.hip) and its binding `ops.branch_attn_merge` refuse bad arguments before anything is
launched -- OTTER_ERR_ARG (-1) and a message from the library, an OtterHipError from the binding; no GPU needed.  Device pointers are never
dereferenced on these paths, so aligned dummy addresses stand in for them.  (A launch on a machine without a GPU would come back as
OTTER_ERR_LAUNCH, not -1: the status tells the two apart.)"""
import re

import pytest
import torch

from otter_amd._capi import OtterHipError

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
H, T, C, B = 4, 3, 2, 2
N = B * C * T


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, **over):
    a = dict(q=P, q_rs=3 * H * 128, q_hs=128, k=P + 2 * H * 128, k_rs=3 * H * 128, k_hs=128, v=P + 4 * H * 128, v_rs=3 * H * 128, v_hs=128, o1=P,
             lse1=P, slopes=P, o=P, N=N, H=H, T=T, rps=C * T, hd=128, scale=0.125)
    a.update(over)
    return lib.otter_branch_attn_merge(a["q"], a["q_rs"], a["q_hs"], a["k"], a["k_rs"], a["k_hs"], a["v"], a["v_rs"], a["v_hs"], a["o1"], a["lse1"],
                                       a["slopes"], a["o"], a["N"], a["H"], a["T"], a["rps"], a["hd"], a["scale"], None)


@pytest.mark.parametrize("name", ["q", "k", "v", "o1", "lse1", "o"])
def test_null_pointers_are_rejected(lib, name):
    assert call(lib, **{name: None}) == -1
    assert b"branch_attn_merge: null pointer" in lib.otter_last_error()


@pytest.mark.parametrize("T_", [0, -1, 65, 1 << 40])
def test_T_outside_1_to_64_is_rejected(lib, T_):
    assert call(lib, T=T_, N=64 * 65, rps=64 * 65) == -1
    assert b"outside [1, 64]" in lib.otter_last_error()


def test_rows_must_be_whole_candidates(lib):
    assert call(lib, N=N + 1) == -1
    assert b"not whole candidates" in lib.otter_last_error()
    assert call(lib, N=0) == -1
    assert b"bad shape" in lib.otter_last_error()
    assert call(lib, H=0) == -1
    assert b"bad shape" in lib.otter_last_error()
    assert call(lib, N=1 << 40, H=1 << 12) == -1                  # (N * H beyond the grid)
    assert b"bad shape" in lib.otter_last_error()


@pytest.mark.parametrize("rps", [0, T - 1, C * T + 1, 2 * T + T, -T])
def test_rows_per_sentence_must_be_whole_candidates_and_divide_N(lib, rps):
    assert call(lib, rps=rps) == -1
    assert b"rows_per_sentence" in lib.otter_last_error()


@pytest.mark.parametrize("hd", [64, 127, 256, 0])
def test_head_dims_other_than_128_are_rejected(lib, hd):
    assert call(lib, hd=hd) == -1
    assert b"(128 only)" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q", "k", "v", "o1", "o"])
def test_misaligned_pointers_are_rejected(lib, name):
    assert call(lib, **{name: P + 8}) == -1
    assert b"need 16-byte alignment" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["lse1", "slopes"])
def test_misaligned_float_pointers_are_rejected(lib, name):
    assert call(lib, **{name: P + 2}) == -1
    assert b"4-byte alignment" in lib.otter_last_error()


@pytest.mark.parametrize("name", ["q_rs", "q_hs", "k_rs", "k_hs", "v_rs", "v_hs"])
def test_misaligned_and_negative_strides_are_rejected(lib, name):
    assert call(lib, **{name: 3 * H * 128 + 4}) == -1
    assert b"multiples of 8" in lib.otter_last_error()
    assert call(lib, **{name: -128}) == -1
    assert b"must not be negative" in lib.otter_last_error()


# ---- the binding: the same refusals from tensors, on CPU tensors (nothing can be launched from them) -----------------------------------------

def _tensors(n=N, h=H, rps=C * T):
    qkv = torch.zeros(n, 3, h, 128, dtype=torch.bfloat16)
    return dict(q=qkv[:, 0], k_new=qkv[:, 1], v_new=qkv[:, 2], o1=torch.zeros(n, h, 128),
                lse1=torch.zeros(n // rps, h, rps), scale=0.125, T=T, rows_per_sentence=rps, slopes=torch.ones(h), out=None)


def _args(**over):
    from otter_amd import ops

    a = _tensors()
    a.update(over)
    return ops._branch_attn_args(a["q"], a["k_new"], a["v_new"], a["o1"], a["lse1"], a["scale"], a["T"], a["rows_per_sentence"], a["slopes"], a["out"])


def test_binding_builds_the_library_arguments():
    a = _tensors()
    args, o = _args(**a)
    assert len(args) == 19 and tuple(o.shape) == (N, H, 128) and o.dtype == torch.bfloat16
    assert args[:3] == (a["q"].data_ptr(), 3 * H * 128, 128) and args[3] == a["k_new"].data_ptr() and args[6] == a["v_new"].data_ptr()
    assert args[9:13] == (a["o1"].data_ptr(), a["lse1"].data_ptr(), a["slopes"].data_ptr(), o.data_ptr())
    assert args[13:] == (N, H, T, C * T, 128, 0.125)
    assert _args(slopes=None)[0][11] is None


BAD = {
    "T_zero": (dict(T=0), "outside [1, 64]"),
    "T_65": (dict(T=65), "outside [1, 64]"),
    "N_not_multiple_of_T": (dict(T=5), "not whole candidates"),
    "rows_per_sentence": (dict(rows_per_sentence=T * 4), "rows_per_sentence"),
    "head_dim": (dict(q=torch.zeros(N, H, 64, dtype=torch.bfloat16)), "bf16 [N,H,128]"),
    "dtype": (dict(q=torch.zeros(N, H, 128)), "bf16 [N,H,128]"),
    "misaligned_stride": (dict(k_new=torch.zeros(N, H * 128 + 4, dtype=torch.bfloat16)[:, :H * 128].view(N, H, 128)), "strides % 8"),
    "misaligned_pointer": (dict(v_new=torch.zeros(N * H * 128 + 4, dtype=torch.bfloat16)[4:].view(N, H, 128)), "16-B aligned"),
    "o1_shape": (dict(o1=torch.zeros(N, H * 128)), "o1 must be"),
    "o1_dtype": (dict(o1=torch.zeros(N, H, 128, dtype=torch.bfloat16)), "o1 must be"),
    "o1_strided": (dict(o1=torch.zeros(N, 2 * H, 128)[:, ::2]), "o1 must be"),
    "lse1_shape": (dict(lse1=torch.zeros(B, C * T, H)), "lse1 must be"),
    "lse1_dtype": (dict(lse1=torch.zeros(B, H, C * T, dtype=torch.float64)), "lse1 must be"),
    "slopes": (dict(slopes=torch.ones(H + 1)), "slopes must be"),
    "out": (dict(out=torch.zeros(N, H * 128, dtype=torch.bfloat16)), "out must be"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_binding_refuses(case):
    over, text = BAD[case]
    with pytest.raises(OtterHipError, match="branch_attn_merge: .*" + re.escape(text)):
        _args(**over)


def test_binding_has_no_cpu_path():
    from otter_amd import ops

    a = _tensors()
    with pytest.raises(OtterHipError, match="GPU only"):
        ops.branch_attn_merge(a["q"], a["k_new"], a["v_new"], a["o1"], a["lse1"], 0.125, T, C * T, slopes=a["slopes"])
