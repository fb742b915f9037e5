"""CPU-only: the Python binding's public surface against the recorded one (tests/golden/python_api_surface.json, written by
tests/golden/make_api_surface.py): module names, classes, method signatures, docstrings, enum values and the prototypes the
loaded library carries.  Everything must be equal but for one rule: a method may gain a docstring, never lose one."""
import copy
import importlib.util
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_api_surface", os.path.join(GOLDEN, "make_api_surface.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_python_surface_is_the_recorded_one(pkg):
    want = json.load(open(os.path.join(GOLDEN, "python_api_surface.json")))
    got = json.loads(json.dumps(_maker().surface(pkg)))  # (through JSON: tuples and keys as the file has them)
    assert got["names"] == want["names"]
    assert got["prototypes"] == want["prototypes"]
    assert sorted(got["classes"]) == sorted(want["classes"])
    for name, w in want["classes"].items():
        g = copy.deepcopy(got["classes"][name])
        assert sorted(g["methods"]) == sorted(w["methods"]), name
        for m, wm in w["methods"].items():
            gm = g["methods"][m]
            assert gm["signature"] == wm["signature"], f"{name}.{m}"
            assert gm["doc"] or not wm["doc"], f"{name}.{m} lost its docstring"
            gm["doc"] = wm["doc"]
        assert g == w, name
