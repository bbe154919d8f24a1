"""The build's source lists cannot drift from csrc/: every source is compiled
and every header triggers a rebuild (no GPU, no compiler needed)."""
import importlib
import os

from conftest import PKG_NAME


def test_every_source_is_built_and_every_header_is_watched():
    bl = importlib.import_module(PKG_NAME + ".build_lib")
    files = sorted(os.listdir(bl.CSRC))
    sources = [f for f in files if f.endswith((".hip", ".cpp"))]
    headers = [f for f in files if f.endswith(".h")]
    assert sources and headers
    assert sorted(bl.SOURCES) == sources
    assert len(set(bl.SOURCES)) == len(bl.SOURCES)
    # what needs_build() compares with the library: every file of csrc/ and the public header
    public = os.path.normpath(os.path.join(bl.CSRC, "..", "..", "include", "mvs_amd.h"))
    watched = set(bl.inputs())
    assert all(os.path.exists(f) for f in watched)
    assert watched == {os.path.normpath(os.path.join(bl.CSRC, f)) for f in sources + headers} | {public}
