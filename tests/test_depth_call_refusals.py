"""Every refusal of the depth-map entry points, pinned: tests/golden/depth_call_refusals.json holds the return code and the whole
text of dmi_last_error(NULL) / dmi_views_last_error(NULL) for the calls of tests/depth_call_refusal_cases.py, recorded from the
commit the fixture names -- before the entry points came to share their checks.  The library of the tree must answer each of
them with the same code and the same text, to the byte: one bad argument at a time, pairs of bad arguments (the order of the
checks decides which one is named) and dmi_views_* without a set.  No device is needed: every check comes before it is asked for."""
import json
import os

import depth_call_refusal_cases as table
from cudadepthmapintegration_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_refusal_is_the_recorded_one():
    with open(os.path.join(ROOT, "tests", "golden", "depth_call_refusals.json")) as fh:
        golden = json.load(fh)
    assert len(golden["recorded_from_commit"]) >= 7
    calls = golden["calls"]
    # the fixture and the table name the same calls, in the same order: neither can lose one unseen
    assert [(c["entry"], c["arguments"]) for c in calls] == [(e, o) for e, o in table.cases()]
    assert {c["entry"] for c in calls} == set(table.GOOD) | set(table.VIEWS_ENTRIES)
    L = capi.load()
    differing = []
    for c in calls:
        got = table.call(L, c["entry"], c["arguments"])
        if got != (c["code"], c["text"]):
            differing.append((c["entry"], c["arguments"], got, (c["code"], c["text"])))
    assert not differing, differing
