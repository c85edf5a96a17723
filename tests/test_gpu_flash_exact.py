"""The flash attention kernels (csrc/flash.hip) on inputs whose answer is known exactly -- tests/_flash_cases.py builds and checks them,
tests/test_flash_cases_cpu.py shows that the checks fail on a step that loses, admits or misplaces one key, forgets a rescale, a query tile, a
mask bit or a dead row.  Every bound is per element (r bf16 roundings of the sum of the absolute terms), lse of the count inputs to a quarter of
what one key moves it.

  narrow      (2, 2) x S in 1 .. 321, causal and not: count, one-key (with and without ALiBi), one-query and random inputs
  padded      B = 10, S = 260, 0 .. 200 keys lost per row on the left (whole waves and a whole block of dead rows), with holes, on the right
  ramps       the row maximum moving by 5.0 / 5.6 / 30 per key tile, jumping by 60, falling by 60: the forward's lazy rescale on both sides of
              its threshold
  Sq != Sk    both ways, causal and not, forward and backward
  Sk > 8192   the per-tile ballot that replaces the LDS mask words (8256), and the last length on the words (8192)
  32 / 33 key blocks  the persistent dK/dV form at its limit (4096: mask bit 31) and the fall-back behind it (4097, 4224)

Every output view lies in a sentinel-filled frame (64 rows before and after, the strided neighbours of the fused and interleaved layouts, lse
too); every byte outside the views must be unchanged."""
import ctypes
import gc

import pytest
import torch

from tests import _flash_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
SENT = 2.0 ** 28     # exact in bf16; no output here comes near it
SENT_LSE = 12345.0


@pytest.fixture(scope="module")
def ops():
    from otter_amd import _capi, ops as _ops

    assert _capi.lib().otter_device_check() > 0, _capi.lib().otter_last_error()
    yield _ops
    _ops.set_flash_variant(0)
    print("\n" + C.worst_table())
    gc.collect()
    torch.cuda.empty_cache()


class Frame:
    """[B, GUARD + S + GUARD, ...] bf16 filled with the sentinel; slot(i) is the [B, S, H, hd] view of tensor i in the layout."""

    def __init__(self, layout, B, S, H, hd, slots):
        self.S = S
        shape = {"fused": (B, S + 2 * GUARD, 3, H, hd), "interleaved": (B, S + 2 * GUARD, H, 3, hd)}.get(layout)
        if shape is None:
            self.bufs = {i: torch.full((B, S + 2 * GUARD, H, hd), SENT, dtype=torch.bfloat16, device=DEV) for i in slots}
            self.index = {i: (i, (slice(None), slice(GUARD, GUARD + S))) for i in slots}
        else:
            buf = torch.full(shape, SENT, dtype=torch.bfloat16, device=DEV)
            self.bufs = {0: buf}
            tail = (lambda i: (i,)) if layout == "fused" else (lambda i: (slice(None), i))
            self.index = {i: (0, (slice(None), slice(GUARD, GUARD + S)) + tail(i)) for i in slots}
        self.pristine = {i: b.clone() for i, b in self.bufs.items()}

    def slot(self, i):
        b, ix = self.index[i]
        return self.bufs[b][ix]

    def untouched_outside_views(self):
        """True when everything but the views still holds the sentinel; refills the views for the next run."""
        for i in self.index:
            self.slot(i).fill_(SENT)
        return all(torch.equal(self.bufs[i], self.pristine[i]) for i in self.bufs)


class DeviceCase:
    """The inputs of a case on the device, in its layout, and its output frames: built once, run under every variant."""

    def __init__(self, c):
        self.c = c
        B, H, Sq, Sk, hd = c.B, c.H, c.Sq, c.Sk, c.hd
        self.fq, self.fk = Frame(c.layout, B, Sq, H, hd, [0]), Frame(c.layout, B, Sk, H, hd, [1, 2])
        self.fq.slot(0).copy_(c.q)
        self.fk.slot(1).copy_(c.k)
        self.fk.slot(2).copy_(c.v)
        self.q, self.k, self.v = self.fq.slot(0), self.fk.slot(1), self.fk.slot(2)
        self.dout = c.dout.to(DEV)
        self.sl = c.slopes.to(DEV) if c.slopes is not None else None
        self.kv = c.key_valid.to(DEV) if c.key_valid is not None else None
        self.fo = Frame("compact", B, Sq, H, hd, [0])
        self.lse_buf = torch.full((2 * GUARD + B * H * Sq,), SENT_LSE, dtype=torch.float32, device=DEV)
        self.gq, self.gk = Frame(c.layout, B, Sq, H, hd, [0]), Frame(c.layout, B, Sk, H, hd, [1, 2])

    def run(self, ops, variant, backward):
        from otter_amd import _capi as K

        c = self.c
        o = self.fo.slot(0)
        lse = self.lse_buf[GUARD:GUARD + c.B * c.H * c.Sq].view(c.B, c.H, c.Sq)
        lse.fill_(SENT_LSE)
        dq, dk, dv = self.gq.slot(0), self.gk.slot(1), self.gk.slot(2)
        ops.set_flash_variant(variant)
        try:
            d = ops._flash_desc(self.q, self.k, self.v, o, lse, self.sl, self.kv, c.scale, c.causal)
            K.check(K.lib().otter_flash_attn_fwd(ctypes.byref(d), K.stream()), "flash_attn_fwd")
            if backward:
                ops.flash_attn_bwd(self.q, self.k, self.v, o, lse, self.dout, dq, dk, dv, self.sl, self.kv, c.scale, c.causal)
            torch.cuda.synchronize()
        finally:
            ops.set_flash_variant(0)
        res = C.Result(o=o.cpu(), lse=lse.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())
        g = self.lse_buf
        assert bool((g[:GUARD] == SENT_LSE).all()) and bool((g[-GUARD:] == SENT_LSE).all()), "%s: lse frame written" % c.name
        assert self.fo.untouched_outside_views(), "%s: o frame written outside the view" % c.name
        assert self.gq.untouched_outside_views() and self.gk.untouched_outside_views(), "%s: gradient frame written outside the views" % c.name
        if backward:
            assert not bool((res.dq.float() == SENT).any() | (res.dk.float() == SENT).any() | (res.dv.float() == SENT).any()), "%s: gradient not written" % c.name
        assert not bool((res.o.float() == SENT).any()) and not bool((res.lse == SENT_LSE).any()), "%s: output not written" % c.name
        return res


def run_cases(ops, cases, variants, backward=True):
    worst = 0.0
    for c in cases:
        dc = DeviceCase(c)
        for v in variants:
            if v == 1 and c.hd == 64:
                continue
            try:
                worst = max(worst, C.check(c, dc.run(ops, v, backward), backward=backward))
            except C.CheckFailure as e:
                raise AssertionError("flash variant %d: %s" % (v, e)) from e
        c._fwd = None
    return worst


V128 = [0, 1, 2, 4, 6, 7, 8]
V64 = [0, 2, 8]


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("S", C.ALL_S)
def test_narrow(ops, S, hd):
    layout = "fused" if hd == 128 else C.LAYOUTS[C.ALL_S.index(S) % 3]
    w = run_cases(ops, C.narrow_cases(S, hd, layout), V128 if hd == 128 else V64)
    print("[flash-exact] narrow S %d hd %d %s: worst error / bound %.3f" % (S, hd, layout, w))


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("mask", ["left", "holes", "right"])
def test_padded_batch(ops, mask, hd):
    layout = "fused" if hd == 128 else C.LAYOUTS[(["left", "holes", "right"].index(mask) + 1) % 3]
    w = run_cases(ops, C.padded_cases(mask, hd, layout), V128 if hd == 128 else V64)
    print("[flash-exact] padded %s hd %d %s: worst error / bound %.3f" % (mask, hd, layout, w))


@pytest.mark.parametrize("ramp", list(C.RAMPS))
def test_ramps_across_the_rescale_threshold(ops, ramp):
    cases = [C.ramp_case(ramp, hd, al, causal) for (hd, al) in ((128, False), (128, True), (64, False)) for causal in (False, True)]
    w = run_cases(ops, cases, [0, 1, 6, 7, 8])
    print("[flash-exact] ramp %s: worst error / bound %.3f" % (ramp, w))


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("Sq,Sk", C.SQSK)
def test_sq_ne_sk(ops, Sq, Sk, hd):
    layout = "fused" if hd == 128 else C.LAYOUTS[C.SQSK.index((Sq, Sk)) % 3]
    w = run_cases(ops, C.sqsk_cases(Sq, Sk, hd, layout), [0, 1, 2, 6, 7, 8])
    print("[flash-exact] Sq %d Sk %d hd %d %s: worst error / bound %.3f" % (Sq, Sk, hd, layout, w))


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("Sq,Sk,backward", [(64, 8256, False), (8256, 8256, True), (64, 8192, False), (8192, 8192, True)])
def test_key_mask_beyond_the_lds_words(ops, Sq, Sk, backward, hd):
    """Sk = 8256: 129 key tiles, the forward (versions 2 and 3) and the dQ kernel read the mask bytes per tile; dK/dV per key block (65
    blocks).  8192: the last length on the LDS words."""
    layout = "fused" if hd == 128 else "interleaved"
    cases = C.long_cases(Sq, Sk, hd, backward=backward, layout=layout)
    if not backward:
        cases += C.long_cases(Sq, Sk, hd, backward=False, causal=False, layout=layout)
    assert ((Sk + 63) // 64 > C.KMASK_TILES) == (Sk == 8256)
    w = run_cases(ops, cases, [0, 6], backward=backward)
    print("[flash-exact] mask fallback Sq %d Sk %d hd %d: %d cases, worst error / bound %.3f" % (Sq, Sk, hd, len(cases), w))


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("S", [4096, 4097, 4224])
def test_persistent_dkv_at_its_block_limit(ops, S, hd):
    """4096 keys: 32 key blocks, the last one on bit 31 of the persistent form's mask word (variants 0 / 8; 7: the per-block form).  4097 and
    4224: 33 blocks, every variant falls back to the per-block form."""
    assert ((S + 127) // 128 <= C.PERS_MAX_BLOCKS) == (S == 4096)
    cases = C.long_cases(S, S, hd, layout="fused" if hd == 128 else "compact")
    w = run_cases(ops, cases, [8, 7, 0])
    print("[flash-exact] dK/dV block limit S %d hd %d: %d cases, worst error / bound %.3f" % (S, hd, len(cases), w))
