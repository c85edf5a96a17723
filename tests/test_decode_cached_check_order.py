"""CPU: the ORDER of the argument checks of the ten cached-decode entry points (csrc/decode_cache.hip, decode_cache_i8.hip,
decode_cache_shared.hip, decode_cache_shared_i8.hip, persimmon_decode_cache.hip) is part of the ABI: of two faults in one call, the check that stands first names the error.
For each entry point CHECKS lists every check from the null-pointer check to the workspace check, in order, each with the message fragment
that identifies it and one perturbation of an otherwise valid call that trips it.  Every perturbation is tried alone, and every adjacent
pair (i, i + 1) together: the message must be check i's.  No GPU: every call is refused before anything is launched, so aligned dummy
addresses stand in for the device pointers."""
import pytest

P = 1 << 20   # a 16-byte aligned stand-in for a device pointer
H, S_MAX = 2, 64

# ---- an accepted call of each family, and the order of its arguments ---------------------------------------------------------------------
NEW_TOKEN = ["q", "q_rs", "q_hs", "kn", "kn_rs", "kn_hs", "vn", "vn_rs", "vn_hs", "cos", "sin", "cs_rs"]
CACHE = ["kc", "kc_rs", "kc_hs", "vc", "vc_rs", "vc_hs"]
SCALES = ["ks", "ks_rs", "ks_hs", "vs", "vs_rs", "vs_hs"]
TABLES = ["src", "src_rs", "kvalid", "kv_rs"]
TAIL = ["o", "ws", "ws_bytes", "N", "H", "pos", "S_max", "head_dim"]   # pos: the position (scalar entries) or its device address (dyn)

PLAIN = NEW_TOKEN + CACHE + TABLES + ["slopes"] + TAIL + ["scale"]
I8 = NEW_TOKEN + CACHE + SCALES + TABLES + ["slopes"] + TAIL + ["scale"]
SHARED = PLAIN + ["group", "shared_len"]
SHARED_I8 = I8 + ["group", "shared_len"]
PERSIMMON = ["qkv", "gq", "bq", "gk", "bk", "cos", "sin"] + CACHE + TABLES + TAIL + ["rot", "eps", "scale"]
PERSIMMON_DYN = PERSIMMON[:7] + ["table_rs"] + PERSIMMON[7:]


def valid(head_dim, dyn):
    a = dict(q=P, q_rs=3 * H * 128, q_hs=128, kn=P + 2 * H * 128, kn_rs=3 * H * 128, kn_hs=128, vn=P + 4 * H * 128, vn_rs=3 * H * 128, vn_hs=128,
             cos=None, sin=None, cs_rs=0, kc=P, kc_rs=H * S_MAX * head_dim, kc_hs=S_MAX * head_dim, vc=P, vc_rs=H * S_MAX * head_dim,
             vc_hs=S_MAX * head_dim, ks=P, ks_rs=H * S_MAX, ks_hs=S_MAX, vs=P, vs_rs=H * S_MAX, vs_hs=S_MAX, src=None, src_rs=0, kvalid=None,
             kv_rs=0, slopes=None, o=P, ws=P, ws_bytes=1 << 20, N=6, H=H, pos=P if dyn else 8, S_max=S_MAX, head_dim=head_dim, scale=0.0884,
             group=3, shared_len=5)
    if head_dim == 64:   # Persimmon: one packed new token, LayerNorm weights, rotary rows that are always given
        a.update(qkv=P, gq=P, bq=P, gk=P, bk=P, cos=P, sin=P, table_rs=32, rot=32, eps=1e-5)
    return a


# ---- the checks, in order.  (fragment, perturbation) ---------------------------------------------------------------------------------------
NULL = ("null pointer", dict(o=None))
COS_SIN = ("both be given or both be NULL", dict(cos=P))
HD128 = ("head_dim 64 (128 only)", dict(head_dim=64))
HD64 = ("head_dim 128 (64 only)", dict(head_dim=128))
SHAPE = ("bad shape N=6 H=0", dict(H=0))
ROT = ("rot=8 must be a multiple of 16", dict(rot=8))
CAPACITY = ("S_max=1 outside [2, 65536]", dict(S_max=1))
GROUP = ("group=9: the kernel is built for groups of 2 to 6 rows", dict(group=9))
WHOLE_GROUPS = ("N=7 rows are not whole groups of", dict(N=7))
POS_LOW = ("pos=0: a cached step continues a cache", dict(pos=0))
POS_HIGH = ("pos=64 is beyond the cache capacity S_max=64", dict(pos=S_MAX))
SHARED_LEN = ("shared_len=0 outside [1, pos]", dict(shared_len=0))
SHARED_LEN_DYN = ("shared_len=0 outside [1, S_max)", dict(shared_len=0))
ALIGNED = ("q, k_new, v_new, k_cache, v_cache need 16-byte alignment", dict(vn=P + 4 * H * 128 + 2))
ALIGNED_PERSIMMON = ("qkv, k_cache, v_cache need 16-byte alignment", dict(vc=P + 4))
SCALE_ALIGNED = ("k_scale, v_scale need 4-byte alignment", dict(vs=P + 2))
POS_DEV = ("pos_dev needs 4-byte alignment", dict(pos=P + 2))
STRIDES_8 = ("q / k_new / v_new / cache strides must be multiples of 8 elements", dict(q_hs=132))
STRIDES_8_NEW = ("q / k_new / v_new strides must be multiples of 8 elements", dict(kn_rs=3 * H * 128 + 4))
STRIDES_8_PERSIMMON = (": cache strides must be multiples of 8 elements", dict(vc_rs=H * S_MAX * 64 + 4))
STRIDES_16 = ("code cache strides must be multiples of 16 elements", dict(kc_rs=H * S_MAX * 128 + 8))
OVERLAP_128 = ("a cache head stride below S_max * 128 would make the slots of two heads overlap", dict(kc_hs=S_MAX * 128 - 16))
OVERLAP_64 = ("a cache head stride below S_max * 64 would make the slots of two heads overlap", dict(kc_hs=S_MAX * 64 - 8))
SCALE_OVERLAP = ("a scale head stride below S_max would make the scales of two heads overlap", dict(ks_hs=S_MAX - 1))
# (a negative row stride is below `pos` at every position, 0 included: the perturbation holds beside POS_LOW too)
ROWS = ("src needs a row stride >= pos, key_valid one >= pos + 1, cos / sin a non-negative one", dict(src=P, src_rs=-1))
ROWS_PERSIMMON = ("src needs a row stride >= pos, key_valid one >= pos + 1", dict(src=P, src_rs=-1))
ROWS_DYN = ("cos / sin tables need a row stride >= 128, src one >= S_max - 1, key_valid one >= S_max", dict(kvalid=P, kv_rs=S_MAX - 1))
ROWS_PERSIMMON_DYN = ("cos / sin tables need a row stride >= rot, src one >= S_max - 1, key_valid one >= S_max", dict(table_rs=16))
WORKSPACE = ("workspace of 16 bytes, ", dict(ws_bytes=16))

# entry point -> (number of its checks, argument order, head_dim, the checks).  The number stands beside the name on purpose: a check added
# to an entry point without an entry here must fail this test.
CHECKS = {
    "decode_attn_cached": (12, PLAIN, 128, [NULL, COS_SIN, HD128, SHAPE, CAPACITY, POS_LOW, POS_HIGH, ALIGNED, STRIDES_8, OVERLAP_128, ROWS,
                                            WORKSPACE]),
    "decode_attn_cached_dyn": (11, PLAIN, 128, [NULL, COS_SIN, HD128, SHAPE, CAPACITY, ALIGNED, POS_DEV, STRIDES_8, OVERLAP_128, ROWS_DYN,
                                                WORKSPACE]),
    "decode_attn_cached_i8": (15, I8, 128, [NULL, COS_SIN, HD128, SHAPE, CAPACITY, ALIGNED, SCALE_ALIGNED, STRIDES_8_NEW, STRIDES_16, OVERLAP_128,
                                            SCALE_OVERLAP, POS_LOW, POS_HIGH, ROWS, WORKSPACE]),
    "decode_attn_cached_i8_dyn": (14, I8, 128, [NULL, COS_SIN, HD128, SHAPE, CAPACITY, ALIGNED, SCALE_ALIGNED, STRIDES_8_NEW, STRIDES_16,
                                                OVERLAP_128, SCALE_OVERLAP, POS_DEV, ROWS_DYN, WORKSPACE]),
    "decode_attn_cached_shared": (15, SHARED, 128, [NULL, COS_SIN, HD128, SHAPE, CAPACITY, GROUP, WHOLE_GROUPS, POS_LOW, POS_HIGH, SHARED_LEN,
                                                    ALIGNED, STRIDES_8, OVERLAP_128, ROWS, WORKSPACE]),
    "decode_attn_cached_shared_dyn": (14, SHARED, 128, [NULL, COS_SIN, HD128, SHAPE, CAPACITY, GROUP, WHOLE_GROUPS, SHARED_LEN_DYN, ALIGNED,
                                                        POS_DEV, STRIDES_8, OVERLAP_128, ROWS_DYN, WORKSPACE]),
    "decode_attn_cached_shared_i8": (18, SHARED_I8, 128, [NULL, COS_SIN, HD128, SHAPE, CAPACITY, GROUP, WHOLE_GROUPS, ALIGNED, SCALE_ALIGNED,
                                                          STRIDES_8_NEW, STRIDES_16, OVERLAP_128, SCALE_OVERLAP, POS_LOW, POS_HIGH, SHARED_LEN, ROWS,
                                                          WORKSPACE]),
    "decode_attn_cached_shared_i8_dyn": (17, SHARED_I8, 128, [NULL, COS_SIN, HD128, SHAPE, CAPACITY, GROUP, WHOLE_GROUPS, SHARED_LEN_DYN, ALIGNED,
                                                              SCALE_ALIGNED, STRIDES_8_NEW, STRIDES_16, OVERLAP_128, SCALE_OVERLAP, POS_DEV, ROWS_DYN,
                                                              WORKSPACE]),
    "persimmon_decode_attn_cached": (12, PERSIMMON, 64, [NULL, HD64, SHAPE, ROT, CAPACITY, POS_LOW, POS_HIGH, ALIGNED_PERSIMMON,
                                                         STRIDES_8_PERSIMMON, OVERLAP_64, ROWS_PERSIMMON, WORKSPACE]),
    "persimmon_decode_attn_cached_dyn": (11, PERSIMMON_DYN, 64, [NULL, HD64, SHAPE, ROT, CAPACITY, ALIGNED_PERSIMMON, POS_DEV,
                                                                 STRIDES_8_PERSIMMON, OVERLAP_64, ROWS_PERSIMMON_DYN, WORKSPACE]),
}

# Pairs (i, i + 1) that no call can hold, tested as (i, i + 2) instead.  The one such pair, in every scalar entry point: POS_LOW and POS_HIGH
# are the two sides of 1 <= pos < S_max, both read `pos` and nothing else but S_max, and a call that reaches them has S_max >= 2 -- no
# position is below 1 and at or above S_max at once.  (POS_HIGH's own place is still pinned by its pair with the check after it.)
REPLACED = {name: [checks.index(POS_LOW)] for name, (_, _, _, checks) in CHECKS.items() if POS_LOW in checks}


@pytest.fixture(scope="module")
def lib():
    from otter_amd import _capi, build

    build.build(verbose=False)
    return _capi.lib()


def refused(lib, name, fragment, *perturbations):
    _, order, head_dim, _ = CHECKS[name]
    a = valid(head_dim, name.endswith("_dyn"))
    for over in perturbations:
        assert all(k in order for k in over), (name, over)            # (a perturbation of an argument the entry point does not have)
        a.update(over)
    assert getattr(lib, "otter_" + name)(*[a[k] for k in order], None) == -1
    msg = lib.otter_last_error()
    assert msg.startswith(name.encode() + b": "), msg
    assert fragment.encode() in msg, msg


ENTRY = pytest.mark.parametrize("name", list(CHECKS))


@ENTRY
def test_every_check_is_listed_and_trips_alone(lib, name):
    count, _, _, checks = CHECKS[name]
    assert len(checks) == count
    assert len({fragment for fragment, _ in checks}) == count           # no fragment identifies two checks
    for i, (fragment, over) in enumerate(checks):
        assert not any(fragment in other for other, _ in checks[:i] + checks[i + 1:])
        refused(lib, name, fragment, over)


@ENTRY
def test_of_two_adjacent_faults_the_first_names_the_error(lib, name):
    _, _, _, checks = CHECKS[name]
    replaced = REPLACED.get(name, [])
    assert len(replaced) <= 2
    for i in range(len(checks) - 1):
        j = i + 2 if i in replaced else i + 1
        (fragment, over), (_, more) = checks[i], checks[j]
        assert not set(over) & set(more), (name, fragment)             # the two perturbations touch different arguments
        refused(lib, name, fragment, over, more)
