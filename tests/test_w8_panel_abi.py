"""CPU: otter_gemm_w8_panel and otter_gemm_w8_panel_gated (csrc/w8_panel.hip, a piece of csrc/w8.hip) validate their arguments before anything
is launched -- negative status and a message, no GPU needed (device pointers are never dereferenced on these paths, so aligned dummy addresses
stand in for them).  Every refusal the header lists, for both entries, and the documented ORDER of the checks (a call that breaks check i and
check j > i reports check i).  Nothing here launches: a call that passes every other check is stopped by the workspace check, the last one."""
import os
import re

import pytest

P = 1 << 20          # a 16-byte aligned stand-in for a device pointer
Q = 1 << 24          # another one, far enough from P that no [M, N] block of these tests reaches it
F32, BF16 = 0, 1
ENTRIES = ("gemm_w8_panel", "gemm_w8_panel_gated")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "otter_hip.h")


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def call(lib, entry, **over):
    a = dict(x=P, ldx=64, qweight=P, ldw=64, scale=P, bias=None, bias_dtype=F32, y=P, ldy=32, y_dtype=BF16, M=72, N=32, K=64, act=0, gate=P, R=Q,
             ldr=32, r_dtype=BF16, ws=P, ws_bytes=1 << 22)
    a.update(over)
    head = (a["x"], a["ldx"], a["qweight"], a["ldw"], a["scale"], a["bias"], a["bias_dtype"], a["y"], a["ldy"], a["y_dtype"], a["M"], a["N"], a["K"])
    tail = (a["ws"], a["ws_bytes"], None)
    if entry.endswith("_gated"):
        return lib.otter_gemm_w8_panel_gated(*head, a["gate"], a["R"], a["ldr"], a["r_dtype"], *tail)
    return lib.otter_gemm_w8_panel(*head, a["act"], *tail)


def refused(lib, entry, word, **over):
    assert call(lib, entry, **over) == -1, (entry, over)
    msg = lib.otter_last_error()
    assert entry.encode() + b":" in msg and word.encode() in msg, (entry, over, msg)


def passes_the_argument_checks(lib, entry, **over):
    """Stopped by the LAST check only (the workspace): every check before it accepted the arguments, and nothing is launched."""
    refused(lib, entry, "workspace", ws_bytes=0, **over)


def test_symbols_are_declared_with_the_rows_signatures_and_the_abi_version_is_unchanged(lib):
    from otter_amd import _capi

    hdr = open(HEADER).read()
    for name in ENTRIES:
        assert re.search(r"^int otter_%s\(" % name, hdr, re.M), name
        assert "otter_" + name in _capi.SIGNATURES
    assert _capi.SIGNATURES["otter_gemm_w8_panel"] == _capi.SIGNATURES["otter_gemm_w8_rows"]
    assert _capi.SIGNATURES["otter_gemm_w8_panel_gated"] == _capi.SIGNATURES["otter_gemm_w8_rows_gated"]
    assert len(_capi.SIGNATURES) == 86
    assert lib.otter_abi_version() == 3            # purely additive: no existing signature moved


def test_workspace_formula_matches_the_header_and_the_kernels_largest_split():
    from otter_amd import ops

    hdr = open(HEADER).read()
    split = re.search(r"#define OTTER_GEMM_W8_PANEL_MAX_SPLIT\(N\) \\\n(.*)", hdr).group(1)
    ws = re.search(r"#define OTTER_GEMM_W8_PANEL_WORKSPACE_BYTES\(M, N, K\) (.*)", hdr).group(1)

    def c_eval(expr, **names):              # the two macros are integer C expressions: a ? b : c chains, / on positive integers
        expr = expr.split("/*")[0].replace("(int64_t)", "").replace("/", "//").strip()
        assert expr[0] == "(" and expr[-1] == ")"
        expr = expr[1:-1]                    # (the parentheses around the whole macro body)
        parts = [p.strip() for p in re.split(r"[?:]", expr)]
        while len(parts) > 1:               # cond ? value : rest, from the left
            if eval(parts[0], dict(names)):
                return eval(parts[1], dict(names))
            parts = parts[2:]
        return eval(parts[0], dict(names))

    for M, N, K in [(72, 4096, 4096), (256, 16384, 4096), (65, 12288, 4096), (256, 50432, 4096), (256, 128, 16384), (96, 32768, 512), (1, 1, 16)]:
        s = c_eval(split, N=N)
        assert s == min(8, max(1, 256 // ((N + 127) // 128)))
        assert c_eval(ws.replace("OTTER_GEMM_W8_PANEL_MAX_SPLIT(N)", str(s)), M=M, N=N, K=K) == ops.gemm_w8_panel_workspace_bytes(M, N, K) > 0
    assert ops.GEMM_W8_PANEL_MAX_ROWS == 256


@pytest.mark.parametrize("entry,name", [(e, n) for e in ENTRIES for n in ("x", "qweight", "scale", "y", "ws")] + [("gemm_w8_panel_gated", "R")])
def test_null_pointers_are_refused(lib, entry, name):
    refused(lib, entry, "null pointer", **{name: None})


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_gate_and_a_null_bias_pass(lib, entry):
    passes_the_argument_checks(lib, entry, gate=None)
    passes_the_argument_checks(lib, entry, bias=P, bias_dtype=BF16)


@pytest.mark.parametrize("entry", ENTRIES)
def test_row_count_range_is_1_to_256(lib, entry):
    for M in (0, -1, 257):
        refused(lib, entry, "M=%d" % M, M=M)
        assert b"[1, 256]" in lib.otter_last_error()
    for M in (1, 16, 64, 65, 129, 256):
        passes_the_argument_checks(lib, entry, M=M)


@pytest.mark.parametrize("entry", ENTRIES)
def test_n_and_k_ranges(lib, entry):
    refused(lib, entry, "N=0", N=0)
    refused(lib, entry, "K=0", K=0)
    refused(lib, entry, "K=24", K=24, ldw=32, ldx=32)
    refused(lib, entry, "K=8", K=8, ldw=16, ldx=8)
    passes_the_argument_checks(lib, entry, N=1)
    passes_the_argument_checks(lib, entry, K=16)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("over", [dict(x=P + 2), dict(qweight=P + 4), dict(y=P + 8), dict(ldw=72), dict(ldx=68)])
def test_alignment_rules(lib, entry, over):
    refused(lib, entry, "alignment", **over)


@pytest.mark.parametrize("entry,over", [(e, o) for e in ENTRIES for o in (dict(ldw=48), dict(ldx=56), dict(ldy=31))]
                         + [("gemm_w8_panel_gated", dict(ldr=31))])
def test_leading_dimensions_smaller_than_a_row_are_refused(lib, entry, over):
    refused(lib, entry, "leading dimension", **over)


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_dtypes_and_act_codes_are_refused(lib, entry):
    refused(lib, entry, "dtype", y_dtype=7)
    refused(lib, entry, "dtype", bias=P, bias_dtype=2)
    if entry.endswith("_gated"):
        refused(lib, entry, "dtype", r_dtype=2)
        for yd in (F32, BF16):
            for rd in (F32, BF16):
                passes_the_argument_checks(lib, entry, y_dtype=yd, r_dtype=rd)
    else:
        for act in (2, 4, -1):
            refused(lib, entry, "act=%d" % act, act=act)
        for act in (0, 1, 3):
            passes_the_argument_checks(lib, entry, act=act)


def test_y_and_r_may_not_share_a_byte(lib):
    entry = "gemm_w8_panel_gated"
    refused(lib, entry, "overlap", R=P)                                       # the same tensor
    last = P + 2 * (71 * 32 + 32)                                             # one past the last byte of the bf16 [72, 32] block at P
    refused(lib, entry, "overlap", R=last - 2)
    refused(lib, entry, "overlap", y=Q + 16, R=Q)
    passes_the_argument_checks(lib, entry, R=last)                            # adjacent blocks do not overlap
    passes_the_argument_checks(lib, entry, y=last, R=P)


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_workspace_one_byte_short_is_refused(lib, entry):
    need = 8 * 72 * 32 * 4                                                    # N = 32: one column panel, up to 8 K ranges
    refused(lib, entry, "workspace", ws_bytes=need - 1)
    refused(lib, entry, "%d needed" % need, ws_bytes=0)
    need = 2 * 72 * 16384 * 4                                                 # N = 16384: 128 column panels, at most 2 K ranges
    refused(lib, entry, "%d needed" % need, N=16384, ldy=16384, ldr=16384, R=1 << 40, ws_bytes=need - 1)


# the documented order: each entry of the list breaks one check; a call that breaks two reports the earlier one
ORDER = {"gemm_w8_panel": [("null pointer", dict(x=None)), ("M=", dict(M=257)), ("N=", dict(N=0)), ("K=", dict(K=8)), ("alignment", dict(ldx=68)),
                           ("leading dimension", dict(ldy=8)), ("dtype", dict(y_dtype=9)), ("act=", dict(act=2)), ("workspace", dict(ws_bytes=0))],
         "gemm_w8_panel_gated": [("null pointer", dict(R=None)), ("M=", dict(M=0)), ("N=", dict(N=0)), ("K=", dict(K=8)), ("alignment", dict(ldx=68)),
                                 ("leading dimension", dict(ldr=8)), ("dtype", dict(r_dtype=9)), ("overlap", dict(y=Q)),
                                 ("workspace", dict(ws_bytes=0))]}


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_checks_run_in_the_documented_order(lib, entry):
    order = ORDER[entry]
    for i, (word, first) in enumerate(order):
        refused(lib, entry, word, **first)
        for _, later in order[i + 1:]:
            refused(lib, entry, word, **first, **later)


def test_wrappers_refuse_cpu_tensors():
    import torch

    from otter_amd import _capi, ops

    x, q, s = torch.zeros(72, 32, dtype=torch.bfloat16), torch.zeros(16, 32, dtype=torch.int8), torch.ones(16)
    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        ops.gemm_w8_panel(x, q, s)
    with pytest.raises(_capi.OtterHipError, match="GPU only"):
        ops.gemm_w8_panel_gated(x, q, s, None, torch.zeros(72, 16))


@pytest.mark.parametrize("n_rows,one_token,panel_rows,want", [
    (65, True, 256, "panel"), (256, True, 256, "panel"), (72, True, 128, "panel"), (128, True, 128, "panel"),
    (257, True, 256, "dequant"), (96, False, 256, "dequant"), (129, True, 128, "dequant"),
    (64, True, 256, "rows"), (17, True, 256, "rows"), (16, True, 256, "gemv"), (16, False, 256, "gemv"), (24, False, 256, "dequant"),
    (65, True, 0, "dequant"), (65, True, 64, "dequant"), (256, True, 0, "dequant")])
def test_route_with_the_panel_rows_argument(monkeypatch, n_rows, one_token, panel_rows, want):
    from otter_amd import quant

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    monkeypatch.delenv("OTTER_W8_PANEL", raising=False)
    assert quant.route(n_rows, one_token, panel_rows) == want
    if panel_rows == 0:
        assert quant.route(n_rows, one_token) == want                         # the default: the answers the existing tests pin


def test_route_with_the_panel_kernel_switched_off(monkeypatch):
    from otter_amd import quant

    monkeypatch.delenv("OTTER_W8_ROWS", raising=False)
    monkeypatch.setenv("OTTER_W8_PANEL", "0")
    assert quant.route(65, True, 256) == "dequant" and quant.route(256, True, 256) == "dequant"
    assert quant.route(64, True, 256) == "rows" and quant.route(16, True, 256) == "gemv"       # the other cases do not move
    monkeypatch.setenv("OTTER_W8_PANEL", "1")
    assert quant.route(65, True, 256) == "panel"
    monkeypatch.setenv("OTTER_W8_ROWS", "0")                                  # the two switches are independent
    assert quant.route(24, True, 256) == "dequant" and quant.route(72, True, 256) == "panel"


def test_panel_max_rows_is_within_the_kernels_range():
    from otter_amd import ops, quant

    assert 64 <= quant.PANEL_MAX_ROWS <= ops.GEMM_W8_PANEL_MAX_ROWS == 256
