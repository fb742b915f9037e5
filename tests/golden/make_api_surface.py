#!/usr/bin/env python3
"""Regenerate tests/golden/python_api_surface.json: the public surface of the Python binding.

    make_api_surface.py [path/to/another/__init__.py]

Without an argument the working tree's package is read.  With one, that copy of the package is read instead (e.g. the file
`git show <commit>:stabilizer-stream_amd/__init__.py` wrote into a scratch directory), against the working tree's built library
($PSDC_LIB is pointed at it unless set already).  tests/test_python_surface_host.py builds the same structure from the working
tree with surface() and compares.

Recorded: the public module names and their kind; per class its docstring, its enum members, and every public method as the MRO
resolves it (plus __init__, _ck and close) with str(inspect.signature) and whether inspect.getdoc finds a docstring; per name in
EXPORTS the restype and argtypes the loaded CDLL carries.
"""
import enum
import importlib.util
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "python_api_surface.json")
ALSO = ("__init__", "_ck", "close")  # private or dunder names recorded beside the public ones


def _kind(v):
    if inspect.ismodule(v):
        return "module"
    if inspect.isclass(v):
        return "class"
    if inspect.isfunction(v):
        return "function"
    return type(v).__name__


def _methods(cls):
    out = {}
    for name in dir(cls):
        if name.startswith("_") and name not in ALSO:
            continue
        fn = getattr(cls, name)
        if not inspect.isfunction(fn):
            continue
        out[name] = {"signature": str(inspect.signature(fn)), "doc": bool(inspect.getdoc(fn))}
    return out


def _ctype_name(t):
    return None if t is None else t.__name__


def surface(pkg):
    # (a submodule of the package -- shard, source -- becomes an attribute once something imports it: not part of this file)
    public = {k: v for k, v in vars(pkg).items()
              if not k.startswith("_") and not (inspect.ismodule(v) and v.__name__.startswith(pkg.__name__ + "."))}
    classes = {}
    for name, cls in public.items():
        if not inspect.isclass(cls) or cls.__module__ != pkg.__name__:
            continue
        c = {"doc": cls.__doc__, "methods": _methods(cls)}
        if issubclass(cls, enum.Enum):
            c["members"] = {m.name: m.value for m in cls}
        classes[name] = c
    L = pkg.lib()
    protos = {}
    for name in pkg.EXPORTS:
        fn = getattr(L, name)
        protos[name] = {"restype": _ctype_name(fn.restype), "argtypes": [_ctype_name(t) for t in (fn.argtypes or [])]}
    return {"names": {k: _kind(public[k]) for k in sorted(public)}, "classes": classes, "prototypes": protos}


def load(path):
    """The package at `path` (an __init__.py) as a module of its own name, beside any copy loaded already."""
    spec = importlib.util.spec_from_file_location("psdc_surface_subject", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    path = os.path.join(ROOT, "stabilizer-stream_amd", "__init__.py")
    if len(sys.argv) > 1:
        os.environ.setdefault("PSDC_LIB", os.path.join(ROOT, "stabilizer-stream_amd", "libpsdcascade.so"))
        path = os.path.abspath(sys.argv[1])
    s = surface(load(path))
    with open(OUT, "w") as f:
        json.dump(s, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(s["names"]), "names,", len(s["classes"]), "classes,", len(s["prototypes"]), "prototypes")


if __name__ == "__main__":
    main()
