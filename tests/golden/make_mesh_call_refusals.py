"""Records tests/golden/mesh_call_refusals.json: the code and the text of every refused call of tests/mesh_call_refusal_cases.py,
from the library DMI_LIB_OVERRIDE names -- one built from the commit given on the command line, the parent of a change that must
not alter a refusal.  Needs a device (the states behind the refusals hold meshes); a second argument names another output file.

    DMI_LIB_OVERRIDE=/path/to/libdmi_hip.so python tests/golden/make_mesh_call_refusals.py <commit> [<output>]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cudadepthmapintegration_amd import build, capi  # noqa: E402
import mesh_call_refusal_cases as table  # noqa: E402

if __name__ == "__main__":
    assert build.LIB_OVERRIDE, "name the recorded library with DMI_LIB_OVERRIDE"
    runner = table.Runner(capi.load())
    records = []
    for state, entry, overrides in table.cases():
        code, text = runner.call(state, entry, overrides)
        assert code != 0 and text, (state, entry, overrides)
        records.append({"state": state, "entry": entry, "arguments": overrides, "code": code, "text": text})
    runner.close()
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "mesh_call_refusals.json")
    with open(out, "w") as fh:
        fh.write('{"recorded_from_commit": %s,\n"calls": [\n%s\n]}\n' % (json.dumps(sys.argv[1]), ",\n".join(json.dumps(r) for r in records)))
    print(f"{len(records)} refusals -> {out}")
