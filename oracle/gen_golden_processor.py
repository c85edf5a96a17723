"""Fixture generator for tests/test_fuyu_processor.py: runs the reference's own FuyuProcessor methods (get_labels,
find_and_remove_tokens, _right_pad_inputs_with_attention_mask) on the test's inputs and records what they return in
tests/golden/fuyu_processor_ref.npz.  TEST INFRASTRUCTURE: needs a checkout of the reference; the tests read only the .npz.

    python oracle/gen_golden_processor.py <reference checkout>
"""
from __future__ import annotations

import importlib
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "fuyu_processor_ref.npz")


def reference_processor(ref_root):
    path = os.path.join(ref_root, "src", "otter_ai", "models", "fuyu", "processing_fuyu.py")
    name = "transformers.models.fuyu.image_processing_fuyu"    # needs torchvision; the reference only takes FuyuBatchFeature from it
    if name not in sys.modules:
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.SimpleNamespace(FuyuBatchFeature=dict)
    spec = importlib.util.spec_from_file_location("_ref_processing_fuyu", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FuyuProcessor


def main(ref_root):
    sys.path.insert(0, ROOT)
    from tests import test_fuyu_processor as T

    cls = reference_processor(ref_root)
    ref = cls.__new__(cls)
    ref.tokenizer = types.SimpleNamespace(eos_token_id=T.EOS)
    ref.pad_token_id, ref.dummy_image_index = T.EOS, -1
    out = {}
    for seed in T.SEEDS:
        ids = T._batch(seed)
        labels = ref.get_labels(ids.clone(), T.SPECIAL)
        a_ids, a_lab = ids.clone(), labels.clone()
        new_ids, new_lab = ref.find_and_remove_tokens(a_ids, a_lab, T.SPECIAL)
        for k, v in (("ids", ids), ("labels", labels), ("new_ids", new_ids), ("new_labels", new_lab), ("ids_after", a_ids), ("labels_after", a_lab)):
            out["s%d_%s" % (seed, k)] = v.numpy()
    pad = ref._right_pad_inputs_with_attention_mask(T._encodings(), True)
    for k in ("input_ids", "attention_mask", "image_patches_indices"):
        out["right_pad_" + k] = torch.as_tensor(pad[k]).numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, sorted(out))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
