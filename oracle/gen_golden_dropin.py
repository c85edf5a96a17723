"""Fixture generator for tests/test_dropin_reference_loop.py: runs the reference's own training script (train_one_epoch with and without
--mask_lm_head, forward_pass, and the two-process accelerate DDP run of tests/_dropin_ddp_worker.py) on otter_amd's tiny model exactly as
the tests do with a reference checkout, and records what they produced in tests/golden/dropin_reference_loop.npz: losses, checkpoint
keys, and per trained tensor a seeded sample plus the update norm (tests/test_dropin_reference_loop.py:summarize).  TEST INFRASTRUCTURE:
needs a checkout of the reference; the tests read only the .npz where there is none.

    python oracle/gen_golden_dropin.py <reference checkout>
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(ref_root):
    os.environ["OTTER_REF_ROOT"] = os.path.abspath(ref_root)
    sys.path.insert(0, ROOT)
    from tests import test_dropin_reference_loop as T

    assert T.HAVE_REF, "no pipeline/train under %s" % ref_root
    out = {}

    def put(tag, **kw):
        for k, v in kw.items():
            out["%s.%s" % (tag, k)] = np.asarray(v)

    IF, restore = T.install_reference_script()
    try:
        for mask in (False, True):
            with tempfile.TemporaryDirectory() as tmp:
                model, losses, ckpt = T.reference_train_one_epoch(IF, mask, tmp)
                keys = sorted(torch.load(ckpt, map_location="cpu"))
            put("train_one_epoch_mask%d" % int(mask), losses=np.array(losses), ckpt_keys=np.array(keys), **T.summarize(dict(model.named_parameters())))
        loss, _ = T.reference_forward_pass(IF)
        put("forward_pass", loss=float(loss), loss_ndim=loss.ndim)
    finally:
        restore()
    with tempfile.TemporaryDirectory() as tmp:
        blob = T.reference_ddp_run(tmp)
    put("ddp", world=blob["world"], wrapped=blob["wrapped"], losses=np.array(blob["losses"]), **T.summarize(blob["weights"]))
    np.savez_compressed(T.GOLDEN, **out)
    print("wrote", T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
