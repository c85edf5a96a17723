"""CPU: otter_gemv_w8_gated and otter_gemm_w8_rows_gated (csrc/w8.hip) validate their arguments before anything is launched -- negative
status and a message, no GPU needed (device pointers are never dereferenced on these paths, so aligned dummy addresses stand in for them).
Every refusal the header lists, the documented ORDER of the checks (a call that breaks check i and check j > i reports check i), and the
arguments that must pass: gate == NULL, every row count in range, bf16 / fp32 for y, bias and R.  Nothing here launches: a call that passes
every other check is stopped by the workspace check, which is the last one."""
import pytest

P = 1 << 20          # a 16-byte aligned stand-in for a device pointer
Q = 1 << 24          # another one, far enough from P that no [M, N] block of these tests reaches it
F32, BF16 = 0, 1

ENTRIES = {"gemv_w8_gated": 16, "gemm_w8_rows_gated": 64}      # entry -> the largest M


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, entry, **over):
    a = dict(x=P, ldx=64, qweight=P, ldw=64, scale=P, bias=None, bias_dtype=F32, y=P, ldy=32, y_dtype=BF16, M=8, N=32, K=64, gate=P, R=Q,
             ldr=32, r_dtype=BF16, ws=P, ws_bytes=1 << 20)
    a.update(over)
    return getattr(lib, "otter_" + entry)(a["x"], a["ldx"], a["qweight"], a["ldw"], a["scale"], a["bias"], a["bias_dtype"], a["y"], a["ldy"],
                                          a["y_dtype"], a["M"], a["N"], a["K"], a["gate"], a["R"], a["ldr"], a["r_dtype"], a["ws"],
                                          a["ws_bytes"], None)


def refused(lib, entry, word, **over):
    assert call(lib, entry, **over) == -1, (entry, over)
    msg = lib.otter_last_error()
    assert entry.encode() + b":" in msg and word.encode() in msg, (entry, over, msg)


def passes_the_argument_checks(lib, entry, **over):
    """Stopped by the LAST check only (the workspace): every check before it accepted the arguments, and nothing is launched."""
    refused(lib, entry, "workspace", ws_bytes=0, **over)


def test_symbols_are_declared_with_one_signature_and_the_abi_version_is_unchanged(lib):
    from otter_amd import _capi

    assert _capi.SIGNATURES["otter_gemv_w8_gated"] == _capi.SIGNATURES["otter_gemm_w8_rows_gated"]
    plain, gated = _capi.SIGNATURES["otter_gemv_w8"][1], _capi.SIGNATURES["otter_gemv_w8_gated"][1]
    assert gated[:13] == plain[:13] and gated[-3:] == plain[-3:] and len(gated) == len(plain) - 1 + 4      # `act` out; gate, R, ldr, r_dtype in
    assert lib.otter_abi_version() == 3


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", ["x", "qweight", "scale", "y", "ws", "R"])
def test_null_pointers_are_refused(lib, entry, name):
    refused(lib, entry, "null pointer", **{name: None})


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_gate_and_a_null_bias_pass(lib, entry):
    passes_the_argument_checks(lib, entry, gate=None)
    passes_the_argument_checks(lib, entry, gate=None, bias=None)
    passes_the_argument_checks(lib, entry, bias=P, bias_dtype=BF16)


@pytest.mark.parametrize("entry", ENTRIES)
def test_row_count_range(lib, entry):
    top = ENTRIES[entry]
    for M in (0, -1, top + 1):
        refused(lib, entry, "M=%d" % M, M=M)
    for M in (1, top // 2 + 1, top):
        passes_the_argument_checks(lib, entry, M=M)


@pytest.mark.parametrize("entry", ENTRIES)
def test_n_and_k_ranges(lib, entry):
    refused(lib, entry, "N=0", N=0)
    refused(lib, entry, "N=", N=(1 << 30) + 1, ldy=1 << 31, ldr=1 << 31)
    refused(lib, entry, "K=0", K=0)
    refused(lib, entry, "K=24", K=24, ldw=32, ldx=32)
    refused(lib, entry, "K=", K=(1 << 30) + 16, ldw=1 << 31, ldx=1 << 31)
    passes_the_argument_checks(lib, entry, N=1)
    passes_the_argument_checks(lib, entry, K=16)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("over", [dict(x=P + 2), dict(qweight=P + 4), dict(y=P + 8), dict(ldw=72), dict(ldx=68)])
def test_alignment_rules(lib, entry, over):
    refused(lib, entry, "alignment", **over)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("over", [dict(ldw=48), dict(ldx=56), dict(ldy=31), dict(ldr=31)])
def test_leading_dimensions_smaller_than_a_row_are_refused(lib, entry, over):
    refused(lib, entry, "leading dimension", **over)


@pytest.mark.parametrize("entry", ENTRIES)
def test_ldr_of_exactly_n_and_more_pass(lib, entry):
    passes_the_argument_checks(lib, entry, ldr=32)
    passes_the_argument_checks(lib, entry, ldr=37, r_dtype=F32)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("over", [dict(y_dtype=7), dict(bias=P, bias_dtype=2), dict(r_dtype=2), dict(r_dtype=-1)])
def test_bad_dtypes_are_refused(lib, entry, over):
    refused(lib, entry, "dtype", **over)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("yd,rd", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
def test_every_y_and_r_dtype_pair_passes(lib, entry, yd, rd):
    passes_the_argument_checks(lib, entry, y_dtype=yd, r_dtype=rd)


@pytest.mark.parametrize("entry", ENTRIES)
def test_y_and_r_may_not_share_a_byte(lib, entry):
    refused(lib, entry, "overlap", R=P)                                       # the same tensor
    last = P + 2 * (7 * 32 + 32)                                              # one past the last byte of the bf16 [8, 32] block at P
    refused(lib, entry, "overlap", R=last - 2)
    refused(lib, entry, "overlap", y=Q + 16, R=Q)
    passes_the_argument_checks(lib, entry, R=last)                            # adjacent blocks do not overlap
    passes_the_argument_checks(lib, entry, y=last, R=P)


@pytest.mark.parametrize("entry", ENTRIES)
def test_too_small_a_workspace_is_refused(lib, entry):
    need = 8 * 8 * 32 * 4
    refused(lib, entry, "workspace", ws_bytes=need - 1)
    refused(lib, entry, "%d needed" % need, ws_bytes=0)


# the documented order: each entry of the list breaks one check; a call that breaks two reports the earlier one
ORDER = [("null pointer", dict(R=None)), ("M=", dict(M=0)), ("N=", dict(N=0)), ("K=", dict(K=8)), ("alignment", dict(ldx=68)),
         ("leading dimension", dict(ldr=8)), ("dtype", dict(r_dtype=9)), ("overlap", dict(y=Q)), ("workspace", dict(ws_bytes=0))]


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_checks_run_in_the_documented_order(lib, entry):
    for i, (word, first) in enumerate(ORDER):
        refused(lib, entry, word, **first)
        for _, later in ORDER[i + 1:]:
            refused(lib, entry, word, **first, **later)


@pytest.mark.parametrize("name", ["gemv_w8_gated", "gemm_w8_rows_gated"])
def test_wrappers_refuse_cpu_tensors(name):
    import torch

    from otter_amd import _capi, ops

    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        getattr(ops, name)(torch.zeros(8, 32, dtype=torch.bfloat16), torch.zeros(16, 32, dtype=torch.int8), torch.ones(16), None,
                           torch.zeros(8, 16))
