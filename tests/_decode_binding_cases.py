"""What the Python bindings of the cached-decode entry points (otter_amd/ops.py: persimmon_decode_attn, persimmon_decode_attn_cached / _dyn,
decode_attn_cached / _dyn, decode_attn_cached_i8 / _dyn) accept, refuse and hand to the library -- recorded without a GPU and without the library.

`run_case` replaces `_capi.require_cuda`, `_capi.stream` and `_capi.lib` by stand-ins (the last one records the symbol and the argument tuple
and returns 0), calls the wrapper on CPU tensors and returns either {"error": message} or {"symbol", "args", "out"}.  Every pointer in `args`
is replaced by the role of the tensor it belongs to (an input's name, "o" for the returned tensor, "ws" for the workspace, "k_out" / "v_out"
for the caches persimmon_decode_attn allocates), so that what is left -- strides, sizes, scalars -- is the same from run to run.

tests/golden/decode_bindings.json is the output of `python tests/_decode_binding_cases.py OUT.json` against the commit before the wrappers were put on
shared checkers; tests/test_decode_bindings_cpu.py holds every later otter_amd.ops to it.  The recording is never regenerated from the code
under test.

A case is (entry, N, options, mutations): `build` makes the accepted call of that entry point with the optional arguments named in `options`,
each mutation then spoils one argument.  Shapes are the smallest that separate the checks: H = 2, S_max = 16, pos = 8, rot = 32, q / k / v as
slices of one fused [N, 3*H*128] row.
"""
import contextlib
import json
import os
import sys

import torch

H, S_MAX, POS, ROT, EPS, SCALE = 2, 16, 8, 32, 1e-5, 0.125
BF16, F32, I32, U8, I8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8, torch.int8

P0, P1, P2 = "persimmon_decode_attn", "persimmon_decode_attn_cached", "persimmon_decode_attn_cached_dyn"
D1, D2, D3, D4 = "decode_attn_cached", "decode_attn_cached_dyn", "decode_attn_cached_i8", "decode_attn_cached_i8_dyn"
ENTRIES = (P0, P1, P2, D1, D2, D3, D4)
DYN, PERSIMMON, INT8 = (P2, D2, D4), (P0, P1, P2), (D3, D4)


# ---- the stand-ins -------------------------------------------------------------------------------------------------------------------------

class RecordingLib:
    """Every attribute is an entry point that records (symbol, args) and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, symbol):
        def entry(*args):
            self.calls.append((symbol, args))
            return 0
        return entry


@contextlib.contextmanager
def standin_library():
    """otter_amd.ops over a recording library: no GPU, no libotter_hip.so.  Yields the RecordingLib."""
    from otter_amd import _capi

    rec = RecordingLib()
    saved = _capi.require_cuda, _capi.stream, _capi.lib
    _capi.require_cuda, _capi.stream, _capi.lib = (lambda *ts: None), (lambda: 0), (lambda: rec)
    try:
        yield rec
    finally:
        _capi.require_cuda, _capi.stream, _capi.lib = saved


# ---- accepted calls ------------------------------------------------------------------------------------------------------------------------

def _cache(N, S_max, hd, dtype, pad=0):
    """[N,H,S_max,hd] with key stride hd; `pad` extra elements per head: a head stride of S_max*hd + pad."""
    L = S_max * hd
    return torch.zeros((N, H, L + pad), dtype=dtype)[:, :, :L].view(N, H, S_max, hd)


def build(entry, N, options):
    """The keyword arguments of an accepted call.  options: "src", "key_valid", "rotary" (the [128] rows or the tables), "rotaryN" (the
    [N,128] rows), "slopes", "out"."""
    dyn, a = entry in DYN, {}
    if entry in PERSIMMON:
        a["qkv"] = torch.zeros((N, H, 3, 64), dtype=BF16)
        for g in ("gq", "bq", "gk", "bk"):
            a[g] = torch.ones(64, dtype=F32)
        a["cos_table" if dyn else "cos_row"] = torch.zeros((S_MAX, ROT) if dyn else (ROT,), dtype=F32)
        a["sin_table" if dyn else "sin_row"] = torch.zeros((S_MAX, ROT) if dyn else (ROT,), dtype=F32)
        if entry == P0:
            a["k_past"], a["v_past"] = _cache(N, POS, 64, BF16), _cache(N, POS, 64, BF16)
            a["key_valid"] = torch.ones((N, POS + 1), dtype=U8) if "key_valid" in options else None
            a.update(rot=ROT, eps=EPS, scale=SCALE)
            return a
        a["k_cache"], a["v_cache"] = _cache(N, S_MAX, 64, BF16), _cache(N, S_MAX, 64, BF16)
        a["pos_dev" if dyn else "pos"] = torch.full((1,), POS, dtype=I32) if dyn else POS
        a.update(rot=ROT, eps=EPS, scale=SCALE)
    else:
        fused = torch.zeros((N, 3 * H * 128), dtype=BF16)
        for i, t in enumerate(("q", "k_new", "v_new")):
            a[t] = fused[:, i * H * 128:(i + 1) * H * 128].view(N, H, 128)
        cdt = I8 if entry in INT8 else BF16
        a["k_cache"], a["v_cache"] = _cache(N, S_MAX, 128, cdt), _cache(N, S_MAX, 128, cdt)
        if entry in INT8:
            a["k_scale"], a["v_scale"] = torch.ones((N, H, S_MAX), dtype=F32), torch.ones((N, H, S_MAX), dtype=F32)
        a["pos_dev" if dyn else "pos"] = torch.full((1,), POS, dtype=I32) if dyn else POS
        a["scale"] = SCALE
        shape = (S_MAX, 128) if dyn else (N, 128) if "rotaryN" in options else (128,)
        rotary = "rotary" in options or "rotaryN" in options
        a["cos_table" if dyn else "cos"] = torch.zeros(shape, dtype=F32) if rotary else None
        a["sin_table" if dyn else "sin"] = torch.zeros(shape, dtype=F32) if rotary else None
        a["slopes"] = torch.ones(H, dtype=F32) if "slopes" in options else None
    a["src"] = torch.zeros((N, S_MAX), dtype=I32) if "src" in options else None
    a["key_valid"] = torch.ones((N, S_MAX), dtype=U8) if "key_valid" in options else None
    if dyn:
        a["out"] = torch.zeros((N, H * a["k_cache"].shape[3]), dtype=BF16) if "out" in options else None
    return a


# ---- mutations: each spoils one argument of an accepted call ---------------------------------------------------------------------------------

def _set(key, fn):
    def mutate(a, N):
        a[key] = fn(a[key], N)
    return mutate


def _rotary(a, which):
    return next(k for k in a if k.startswith(which))      # cos / cos_row / cos_table


def _on_rotary(which, fn):
    def mutate(a, N):
        k = _rotary(a, which)
        a[k] = fn(a[k], N)
    return mutate


def _misaligned(t, N):
    """The same shape and strides, 8 bytes further on."""
    off = 8 // t.element_size()
    flat = torch.zeros(t.numel() + off, dtype=t.dtype)
    return flat[off:].view(t.shape)


def _smax1(a, N):
    hd, dt = a["k_cache"].shape[3], a["k_cache"].dtype
    a["k_cache"], a["v_cache"] = _cache(N, 1, hd, dt), _cache(N, 1, hd, dt)
    if "k_scale" in a:
        a["k_scale"], a["v_scale"] = torch.ones((N, H, 1), dtype=F32), torch.ones((N, H, 1), dtype=F32)


def _smax_over(a, N):
    """One slot more than the limit of every entry point (65536)."""
    hd, dt = a["k_cache"].shape[3], a["k_cache"].dtype
    a["k_cache"], a["v_cache"] = _cache(N, 65537, hd, dt), _cache(N, 65537, hd, dt)
    if "k_scale" in a:
        a["k_scale"], a["v_scale"] = torch.ones((N, H, 65537), dtype=F32), torch.ones((N, H, 65537), dtype=F32)


def _pad8(a, N):
    hd, dt = a["k_cache"].shape[3], a["k_cache"].dtype
    a["k_cache"], a["v_cache"] = _cache(N, S_MAX, hd, dt, pad=8), _cache(N, S_MAX, hd, dt, pad=8)


MUTATIONS = {
    # the new token
    "q_2d": _set("q", lambda t, N: t[0]),
    "q_f32": _set("q", lambda t, N: t.float()),
    "k_new_stride4": _set("k_new", lambda t, N: torch.zeros((N, H * 128 + 4), dtype=BF16)[:, :H * 128].view(N, H, 128)),
    "v_new_misaligned": _set("v_new", lambda t, N: _misaligned(t.contiguous(), N)),
    "v_new_heads": _set("v_new", lambda t, N: t[:, :1]),
    "qkv_f32": _set("qkv", lambda t, N: t.float()),
    "qkv_3d": _set("qkv", lambda t, N: t.view(N, H, 192)),
    "qkv_strided": _set("qkv", lambda t, N: torch.zeros((N, H, 3, 128), dtype=BF16)[..., :64]),
    "qkv_misaligned": _set("qkv", _misaligned),
    # the caches
    "k_cache_f32": _set("k_cache", lambda t, N: t.float()),
    "k_cache_3d": _set("k_cache", lambda t, N: t[0]),
    "v_cache_short": _set("v_cache", lambda t, N: _cache(N, S_MAX - 1, t.shape[3], t.dtype)),
    "v_cache_key_stride": _set("v_cache", lambda t, N: torch.zeros((N, H, S_MAX, 2 * t.shape[3]), dtype=t.dtype)[..., :t.shape[3]]),
    "v_cache_misaligned": _set("v_cache", _misaligned),
    "cache_pad8": _pad8,                              # head stride = 8 mod 16: fine for bf16 (% 8), refused for int8 (% 16)
    "cache_pad4": lambda a, N: a.update(k_cache=_cache(N, S_MAX, a["k_cache"].shape[3], a["k_cache"].dtype, pad=4)),
    "smax1": _smax1,
    "smax_over": _smax_over,
    "k_scale_f64": _set("k_scale", lambda t, N: t.double()),
    "v_scale_short": _set("v_scale", lambda t, N: t[:, :, :S_MAX - 1]),
    "v_scale_strided": _set("v_scale", lambda t, N: torch.ones((N, H, S_MAX, 2), dtype=F32)[..., 0]),
    "k_past_3d": _set("k_past", lambda t, N: t[0]),
    "past_empty": lambda a, N: a.update(k_past=_cache(N, 0, 64, BF16), v_past=_cache(N, 0, 64, BF16)),
    "k_past_f32": _set("k_past", lambda t, N: t.float()),
    "v_past_short": _set("v_past", lambda t, N: t[:, :, :POS - 1]),
    "v_past_misaligned": _set("v_past", _misaligned),
    # the position
    "pos0": lambda a, N: a.update(pos=0),
    "pos_smax": lambda a, N: a.update(pos=S_MAX),
    "pos_dev_i64": _set("pos_dev", lambda t, N: t.long()),
    "pos_dev_two": _set("pos_dev", lambda t, N: torch.zeros(2, dtype=I32)),
    # LayerNorm and rotary
    "gq_f64": _set("gq", lambda t, N: t.double()),
    "bk_short": _set("bk", lambda t, N: t[:32]),
    "gk_strided": _set("gk", lambda t, N: torch.ones(128, dtype=F32)[::2]),
    "rot0": lambda a, N: a.update(rot=0),
    "rot24": lambda a, N: a.update(rot=24),
    "rot80": lambda a, N: a.update(rot=80),
    "sin_none": lambda a, N: a.update({_rotary(a, "sin"): None}),
    "cos_none": lambda a, N: a.update({_rotary(a, "cos"): None}),
    "cos_f64": _on_rotary("cos", lambda t, N: t.double()),
    "sin_short": _on_rotary("sin", lambda t, N: t[..., :-16]),
    "sin_strided": _on_rotary("sin", lambda t, N: torch.zeros(t.shape + (2,), dtype=F32)[..., 0]),
    "cos_rows_n_plus_1": _on_rotary("cos", lambda t, N: torch.zeros((N + 1, 128), dtype=F32)),
    "sin_other_rows": _on_rotary("sin", lambda t, N: torch.zeros((N, 256), dtype=F32)[:, :128]),
    "cos_3d": _on_rotary("cos", lambda t, N: t[None]),
    "tables_short": lambda a, N: a.update(cos_table=a["cos_table"][:S_MAX - 1], sin_table=a["sin_table"][:S_MAX - 1]),
    "sin_table_other_stride": _set("sin_table", lambda t, N: torch.zeros((S_MAX, 2 * t.shape[1]), dtype=F32)[:, :t.shape[1]]),
    "cos_table_1d": _set("cos_table", lambda t, N: t[0]),
    "tables_long_padded": lambda a, N: a.update(cos_table=torch.zeros((S_MAX + 4, 2 * a["cos_table"].shape[1]), dtype=F32)[:, :a["cos_table"].shape[1]],
                                                sin_table=torch.zeros((S_MAX + 4, 2 * a["sin_table"].shape[1]), dtype=F32)[:, :a["sin_table"].shape[1]]),
    # the beam table and the mask
    "src_i64": _set("src", lambda t, N: t.long()),
    "src_1d": _set("src", lambda t, N: t[0]),
    "src_rows": _set("src", lambda t, N: torch.zeros((N + 1, S_MAX), dtype=I32)),
    "src_cols5": _set("src", lambda t, N: t[:, :5]),
    "src_col_stride": _set("src", lambda t, N: torch.zeros((N, S_MAX, 2), dtype=I32)[..., 0]),
    "src_expanded": _set("src", lambda t, N: torch.zeros(S_MAX, dtype=I32).as_strided((N, S_MAX), (0, 1))),     # row stride 0 < need, at N = 1 too
    "src_padded": _set("src", lambda t, N: torch.zeros((N, S_MAX + 8), dtype=I32)[:, :S_MAX]),        # row stride > need: passed as it is
    "src_exact": lambda a, N: a.update(src=a["src"][:, :POS if "pos" in a else S_MAX - 1]),            # columns == need, row stride > need
    "key_valid_bool": _set("key_valid", lambda t, N: t.bool()),
    "key_valid_1d": _set("key_valid", lambda t, N: t[0]),
    "key_valid_rows": _set("key_valid", lambda t, N: torch.ones((N + 1, t.shape[1]), dtype=U8)),
    "key_valid_cols5": _set("key_valid", lambda t, N: t[:, :5]),
    "key_valid_col_stride": _set("key_valid", lambda t, N: torch.ones(t.shape + (2,), dtype=U8)[..., 0]),
    "key_valid_expanded": _set("key_valid", lambda t, N: torch.ones(t.shape[1], dtype=U8).as_strided((N, t.shape[1]), (0, 1))),
    "src_overlapping": _set("src", lambda t, N: torch.zeros(S_MAX + 2 * N, dtype=I32).as_strided((N, S_MAX), (2, 1))),      # 0 < row stride < need
    "key_valid_padded": _set("key_valid", lambda t, N: torch.ones((N, t.shape[1] + 16), dtype=U8)[:, :t.shape[1]]),
    # ALiBi and the output
    "slopes_f64": _set("slopes", lambda t, N: t.double()),
    "slopes_three": _set("slopes", lambda t, N: torch.ones(H + 1, dtype=F32)),
    "slopes_strided": _set("slopes", lambda t, N: torch.ones(2 * H, dtype=F32)[::2]),
    "out_f32": _set("out", lambda t, N: t.float()),
    "out_rows": _set("out", lambda t, N: torch.zeros((N + 1, t.shape[1]), dtype=BF16)),
    "out_strided": _set("out", lambda t, N: torch.zeros((N, 2 * t.shape[1]), dtype=BF16)[:, :t.shape[1]]),
}


# ---- the table -----------------------------------------------------------------------------------------------------------------------------

def _optional(e):
    return ["key_valid"] if e == P0 else ["src", "key_valid"] + ([] if e in PERSIMMON else ["rotary", "slopes"]) + (["out"] if e in DYN else [])


def _cases():
    cases = []

    def add(entry, N, options=(), mutations=()):
        case = (entry, N, tuple(options), tuple(mutations))
        if case not in cases:
            cases.append(case)

    for e in ENTRIES:
        optional = _optional(e)
        for N in (3, 1):
            add(e, N)
            for o in optional if N == 3 else ():
                add(e, N, [o])
            add(e, N, optional)
        if e in (D1, D3):                                   # both rotary row forms
            add(e, 3, ["rotaryN"])
            add(e, 1, ["rotaryN"])
            add(e, 3, ["rotaryN", "src", "key_valid", "slopes"])
            add(e, 3, ["rotaryN"], ["sin_other_rows"])
            add(e, 3, ["rotaryN"], ["cos_rows_n_plus_1"])
            add(e, 3, ["rotary"], ["cos_3d"])
        every = optional

        # one fault each: every raise of the entry point
        if e in PERSIMMON:
            for m in ("qkv_f32", "qkv_3d", "qkv_strided", "qkv_misaligned", "gq_f64", "bk_short", "gk_strided", "rot0", "rot24", "rot80",
                      "cos_f64", "sin_short", "sin_strided"):
                add(e, 3, every, [m])
        else:
            for m in ("q_2d", "q_f32", "k_new_stride4", "v_new_misaligned", "v_new_heads", "sin_none", "cos_none", "cos_f64", "sin_short", "sin_strided",
                      "slopes_f64", "slopes_three", "slopes_strided"):
                add(e, 3, every, [m])
        if e == P0:
            for m in ("k_past_3d", "past_empty", "k_past_f32", "v_past_short", "v_past_misaligned", "key_valid_bool", "key_valid_cols5",
                      "key_valid_padded", "key_valid_rows"):
                add(e, 3, every, [m])
            continue
        for m in ("k_cache_f32", "k_cache_3d", "v_cache_short", "v_cache_key_stride", "v_cache_misaligned", "cache_pad8", "cache_pad4", "smax1",
                  "src_i64", "src_1d", "src_rows", "src_cols5", "src_col_stride", "key_valid_bool", "key_valid_1d", "key_valid_rows",
                  "key_valid_cols5", "key_valid_col_stride"):
            add(e, 3, every, [m])
        if e in INT8:
            for m in ("k_scale_f64", "v_scale_short", "v_scale_strided"):
                add(e, 3, every, [m])
        if e in DYN:
            for m in ("pos_dev_i64", "pos_dev_two", "tables_short", "sin_table_other_stride", "cos_table_1d", "tables_long_padded", "out_f32",
                      "out_rows", "out_strided"):
                add(e, 3, every, [m])
        else:
            for m in ("pos0", "pos_smax"):
                add(e, 3, every, [m])
        # the row stride of src / key_valid: checked and passed as max(stride, need), or passed raw (the asymmetry that is kept)
        for N in (3, 1):
            for m in ("src_expanded", "src_padded", "src_exact", "key_valid_expanded", "key_valid_padded"):
                add(e, N, ["src", "key_valid"], [m])
            add(e, N, ["src", "key_valid"], ["src_expanded", "key_valid_expanded"])
            add(e, N, ["src", "key_valid"], ["src_overlapping"])
        add(e, 1, every, ["smax_over"])                     # the upper limit of S_max, alone and in front of a bad position
        add(e, 1, every, ["smax_over", "pos_dev_two" if e in DYN else "pos0"])

        # two faults: which check comes first
        new, rotary = ("qkv_f32", "cos_f64") if e in PERSIMMON else ("q_f32", "cos_f64")
        position = "pos_dev_two" if e in DYN else "pos0"
        pairs = [(new, "k_cache_f32"), ("k_cache_f32", position), (position, "tables_short" if e in DYN else rotary),
                 ("tables_short" if e in DYN else rotary, "src_i64"), ("src_i64", "key_valid_bool"), ("smax1", position), ("smax1", "src_cols5")]
        if e in PERSIMMON:
            pairs += [("gq_f64", "rot24"), ("smax1", "gq_f64"), ("rot24", position), ("k_cache_f32", "gq_f64")]
        else:
            pairs += [("key_valid_bool", "slopes_f64"), ("slopes_f64", position), ("slopes_f64", "src_i64"), ("k_cache_f32", "slopes_f64"),
                      ("q_2d", "k_new_stride4"), ("sin_none", "src_i64")]
        if e in INT8:
            pairs += [("k_scale_f64", "slopes_f64"), ("k_cache_f32", "k_scale_f64"), ("k_scale_f64", position)]
        if e in DYN:
            pairs += [("key_valid_bool", "out_f32"), ("src_i64", "out_f32")] + ([] if e in PERSIMMON else [("slopes_f64", "out_f32")])
        for pair in pairs:
            add(e, 3, every, pair)
    add(P0, 3, ["key_valid"], ["gq_f64", "rot24"])
    add(P0, 3, ["key_valid"], ["qkv_f32", "past_empty"])
    add(P0, 3, ["key_valid"], ["past_empty", "k_past_f32"])
    add(P0, 3, ["key_valid"], ["k_past_f32", "gq_f64"])
    add(P0, 3, ["key_valid"], ["rot24", "sin_short"])
    add(P0, 3, ["key_valid"], ["sin_short", "key_valid_bool"])
    return cases


CASES = _cases()


def case_id(case):
    """(entry, the case's name within it): the two keys of the recording."""
    entry, N, options, mutations = case
    opts = "all" if list(options) == _optional(entry) else ",".join(options)
    return entry, "N=%d [%s] %s" % (N, opts, "+".join(mutations) or "ok")


# ---- running one ---------------------------------------------------------------------------------------------------------------------------

def run_case(case):
    """The outcome of one case against the importable otter_amd.ops: {"error": message} (an OtterHipError) or {"symbol", "args", "out"}."""
    from otter_amd import _capi, ops

    entry, N, options, mutations = case
    a = build(entry, N, options)
    for m in mutations:
        MUTATIONS[m](a, N)
    with standin_library() as rec:
        try:
            ret = getattr(ops, entry)(**a)
        except _capi.OtterHipError as e:
            return {"error": str(e)}
    (symbol, args), = rec.calls
    roles = {}
    for k, t in a.items():
        if isinstance(t, torch.Tensor):
            roles.setdefault(t.data_ptr(), k)
    if isinstance(ret, tuple):
        roles.update({ret[1].data_ptr(): "k_out", ret[2].data_ptr(): "v_out"})
        ret = ret[0]
    roles[ops._ws.get(0, torch.device("cpu")).data_ptr()] = "ws"
    roles.setdefault(ret.data_ptr(), "o")                  # (a caller's `out` keeps its own name)
    args = [roles.get(x, x) if isinstance(x, int) and not isinstance(x, bool) else x for x in args]
    return {"symbol": symbol, "args": args, "out": [list(ret.shape), str(ret.dtype)]}


def run_all():
    """{entry: {case name: outcome}}"""
    out = {e: {} for e in ENTRIES}
    for c in CASES:
        entry, name = case_id(c)
        assert name not in out[entry], (entry, name)
        out[entry][name] = run_case(c)
    return out


if __name__ == "__main__":
    # usage: python tests/_decode_binding_cases.py OUT.json   (no default: the recording in tests/golden is made once, from the commit before
    # the change it guards, and a run in the working tree must not replace it with the code under test)
    if len(sys.argv) != 2 or os.path.abspath(sys.argv[1]).startswith(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")):
        sys.exit("usage: _decode_binding_cases.py OUT.json, with OUT.json outside tests/golden (copy a recording there by hand)")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    dump = lambda x: json.dumps(x, separators=(",", ":"))   # noqa: E731
    with open(sys.argv[1], "w") as f:          # one case per line
        f.write("{\n" + ",\n".join("%s: {\n%s\n}" % (dump(e), ",\n".join("%s:%s" % (dump(k), dump(v)) for k, v in sorted(cs.items())))
                                    for e, cs in run_all().items()) + "\n}\n")
