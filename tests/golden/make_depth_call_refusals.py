"""Records tests/golden/depth_call_refusals.json: the code and the text of every refused call of tests/depth_call_refusal_cases.py,
from the library DMI_LIB_OVERRIDE names -- one built from the commit given on the command line, the parent of a change that must
not alter a refusal.  No device is needed.

    DMI_LIB_OVERRIDE=/path/to/libdmi_hip.so python tests/golden/make_depth_call_refusals.py <commit>"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cudadepthmapintegration_amd import build, capi  # noqa: E402
import depth_call_refusal_cases as table  # noqa: E402

if __name__ == "__main__":
    assert build.LIB_OVERRIDE, "name the recorded library with DMI_LIB_OVERRIDE"
    L = capi.load()
    records = []
    for entry, overrides in table.cases():
        code, text = table.call(L, entry, overrides)
        assert code != 0 and text, (entry, overrides)
        records.append({"entry": entry, "arguments": overrides, "code": code, "text": text})
    out = os.path.join(ROOT, "tests", "golden", "depth_call_refusals.json")
    with open(out, "w") as fh:
        fh.write('{"recorded_from_commit": %s,\n"calls": [\n%s\n]}\n' % (json.dumps(sys.argv[1]), ",\n".join(json.dumps(r) for r in records)))
    print(f"{len(records)} refusals -> {out}")
