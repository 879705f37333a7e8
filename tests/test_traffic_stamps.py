"""profiles/traffic.json stamps a counter measurement with a hash over the files its kernels are compiled from, and the
benchmarks report it only while that hash matches.  A file name that no longer exists makes the hash None and the entry
vanish for good without a word; a source the build does not list is never compiled.  Both are caught here, on the CPU."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sqlite-muninn_amd", "csrc")


def _build():
    spec = importlib.util.spec_from_file_location("_mn_build", os.path.join(ROOT, "sqlite-muninn_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _source_lists(node, path=""):
    if isinstance(node, dict):
        if "kernel_sources" in node:
            yield path, node["kernel_sources"]
        for k, v in node.items():
            yield from _source_lists(v, f"{path}/{k}")
    elif isinstance(node, list):
        for i, v in enumerate(node):
            yield from _source_lists(v, f"{path}/{i}")


def test_every_stamped_source_exists():
    lists = list(_source_lists(json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))))
    assert lists
    missing = [(path, f) for path, files in lists for f in files if not os.path.isfile(os.path.join(CSRC, f))]
    assert not missing, missing


def test_build_sources_are_the_hip_files():
    assert sorted(_build().SOURCES) == sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def test_build_headers_hold_every_hpp_and_every_include_resolves():
    """build.py recompiles a unit when a header in HEADERS is newer than its object: a header kept elsewhere, or an
    #include of a file that is not there, would escape that list."""
    import re

    headers = {os.path.normpath(h) for h in _build().HEADERS}
    assert {f for f in os.listdir(CSRC) if f.endswith(".hpp")} <= headers
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".hpp")):
            continue
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(CSRC, f)).read(), re.M):
            assert os.path.isfile(os.path.join(CSRC, inc)), (f, inc)
            assert os.path.normpath(inc) in headers, (f, inc)
