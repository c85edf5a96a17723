"""The Python bindings of the cached-decode entry points against their recording (tests/_decode_binding_cases.py): for every case the same
refusal, word for word, or the same argument tuple handed to the library.  No GPU, no library."""
import json
import os

import pytest

from tests import _decode_binding_cases as B

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_bindings.json")) as f:
    RECORDED = json.load(f)


def test_the_recording_covers_the_table():
    assert {e: sorted(cs) for e, cs in RECORDED.items()} == {e: sorted(B.case_id(c)[1] for c in B.CASES if c[0] == e) for e in B.ENTRIES}


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: " ".join(B.case_id(c)))
def test_binding_matches_the_recording(case):
    entry, name = B.case_id(case)
    got = json.loads(json.dumps(B.run_case(case)))          # (tuples -> lists, as the recording went through JSON)
    assert got == RECORDED[entry][name]
