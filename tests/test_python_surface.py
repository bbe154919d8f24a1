"""The Python surface of the binding, pinned against tests/python_surface.txt.

The listing has one line per public name of `_lib` (every module attribute
without a leading underscore that is not an imported module, plus _LIVE), one
per entry of SIGNATURES, and one per attribute of MvsContext and of Stage
(methods, static methods, properties and class constants, the underscore
helpers included).  Callables are listed with their signature, constants with
their repr, other objects with their type.  It was written from the commit
before `_lib.py` was split into family modules, with listing() below; since
then `_stream_handle` (it returned its argument) left MvsContext and the shared
helpers `_chain`, `_rows` and `_patch_rows` joined it.  Neither the library nor a GPU is needed: importing `_lib` does
not load the library.

The second half tests the tensor check that every *_device wrapper shares.
"""
import importlib
import inspect
import os

import pytest

from conftest import PKG_NAME, REPO

LISTING = os.path.join(REPO, "tests", "python_surface.txt")


def show(obj):
    if isinstance(obj, property):
        return "property"
    if callable(obj):
        return str(inspect.signature(obj))
    return repr(obj) if " at 0x" not in repr(obj) else type(obj).__name__


def listing(lib):
    lines = []
    base = os.path.dirname(os.path.abspath(lib.__file__))
    for name, obj in sorted(vars(lib).items()):
        if (name.startswith("_") and name != "_LIVE") or inspect.ismodule(obj):
            continue
        if name == "SIGNATURES":   # by the types' names: a pointer type's repr names the module that made it
            lines += [f"SIGNATURES {fn} {res.__name__ if res else None} ({', '.join(a.__name__ for a in args)})"
                      for fn, res, args in obj]
        elif name == "_LIVE":   # by its type: its repr depends on the contexts alive in the process
            lines.append(f"{name} {type(obj).__name__}")
        elif isinstance(obj, str) and obj.startswith(base):   # HERE, LIB_PATH: relative to the package
            lines.append(f"{name} {os.path.relpath(obj, base)!r}")
        else:
            lines.append(f"{name} {show(obj)}")
    for cls in (lib.MvsContext, lib.Stage):
        names = set().union(*(vars(k) for k in cls.__mro__ if k is not object))
        for name in sorted(names):
            static = inspect.getattr_static(cls, name)
            if name.startswith("__") and not inspect.isfunction(static):
                continue   # __module__, __doc__, __dict__, __weakref__
            obj = static if isinstance(static, property) else getattr(cls, name)
            lines.append(f"{cls.__name__}.{name} {show(obj)}")
    return lines


def test_surface_matches_the_listing():
    lib = importlib.import_module(PKG_NAME + "._lib")
    with open(LISTING) as f:
        want = f.read().splitlines()
    got = listing(lib)
    assert got == want, "\n".join(sorted(set(got) ^ set(want)))


def test_shared_tensor_check():
    import torch
    need = importlib.import_module(PKG_NAME + "._context")._need
    a = torch.zeros((2, 3), dtype=torch.float64)
    i = torch.zeros(2, dtype=torch.int32)
    rows = [("a", a, 8, (2, 3)), ("i", i, 4, (2,)), ("opt", None, 8, (2,))]
    assert need("who", rows) is None                       # all good, None in the optional slot skipped
    bad = {"size": ("i", i, 8, (2,)),                      # int32 where int64 is wanted
           "shape": ("a", a, 8, (3, 2)),
           "strided": ("a", a.t(), 8, (3, 2))}             # the right shape, not contiguous
    for case, row in bad.items():
        with pytest.raises(RuntimeError) as e:
            need("who", [rows[0], row, rows[2]] if case == "size" else [row, rows[1], rows[2]])
        name, _, size, shape = row
        assert str(e.value) == f"who: {name} must be contiguous, {size}-byte elements, {shape}", case
    with pytest.raises(RuntimeError) as e:                 # outputs that come all or none: None is an error
        need("who", rows, optional=False)
    assert str(e.value) == "who: opt must be contiguous, 8-byte elements, (2,)"
    with pytest.raises(RuntimeError) as e:                 # the right size, integer where floating is wanted
        need("who", [("a", a.view(torch.int64), 8, (2, 3))], floating=("a",))
    assert str(e.value) == "who: a must be contiguous, 8-byte elements, (2, 3)"
    assert need("who", rows, floating=("a",)) is None
