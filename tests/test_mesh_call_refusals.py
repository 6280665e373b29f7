"""Every refusal of the entry points that work on the context's iso-surface mesh, pinned: tests/golden/mesh_call_refusals.json holds
the return code and the whole text of dmi_last_error for the calls of tests/mesh_call_refusal_cases.py, recorded on the device
from the commit the fixture names -- before the stages came to share their preamble, their getters and their downloads.  The
library of the tree must answer each of them with the same code and the same text, to the byte: a null in each pointer position,
one bad parameter at a time, pairs of them (the order of the checks decides which one is named) and every state that refuses a
call.  The calls without a context need no device and are replayed by the CPU suite as well."""
import json
import os

import pytest

import mesh_call_refusal_cases as table
from cudadepthmapintegration_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "mesh_call_refusals.json")) as fh:
        golden = json.load(fh)
    assert len(golden["recorded_from_commit"]) >= 7
    return golden["calls"]


def _replay(calls):
    runner = table.Runner(capi.load())
    differing = []
    try:
        for c in calls:
            got = runner.call(c["state"], c["entry"], c["arguments"])
            if got != (c["code"], c["text"]):
                differing.append((c["state"], c["entry"], c["arguments"], got, (c["code"], c["text"])))
    finally:
        runner.close()
    assert not differing, differing


def test_the_fixture_and_the_table_name_the_same_calls():
    calls = _golden()
    # the same calls in the same order: neither can lose one unseen
    assert [(c["state"], c["entry"], c["arguments"]) for c in calls] == [(s, e, o) for s, e, o in table.cases()]
    assert {c["entry"] for c in calls} == set(table.GOOD)
    states = [c["state"] for c in calls]
    assert all(a == b or b not in states[:i + 1] for i, (a, b) in enumerate(zip(states, states[1:])))   # a state's calls are together
    assert all(c["code"] != 0 and c["text"] for c in calls)


def test_every_refusal_without_a_context_is_the_recorded_one():
    calls = [c for c in _golden() if c["state"] == table.NULL_CONTEXT]
    assert [(c["state"], c["entry"], c["arguments"]) for c in calls] == table.null_context_cases() and len(calls) >= len(table.GOOD)
    _replay(calls)


@pytest.mark.gpu
def test_every_refusal_is_the_recorded_one():
    _replay(_golden())
