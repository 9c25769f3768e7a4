"""What is built is what is there: every file under csrc/ is named in _build.SOURCES or _build.HEADERS - the two tuples that
is_stale(), bench.loaded_source_hash() and tools/isa_mix.py hash and time-stamp, so a file left out of them is invisible to
all three -, every quoted #include resolves to a member of them, no unit is compiled a second time under a macro, and the
LDS limit of a kernel is keyed by the kernel, not by a hand-numbered index.  Text inspection only."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ac-mpc_amd"))

from acmpc_amd import _build  # noqa: E402


def members():
    return {os.path.normpath(os.path.join(_build.CSRC_DIR, name)) for name in _build.SOURCES + _build.HEADERS}


def csrc_files():
    return sorted(os.path.join(_build.CSRC_DIR, name) for name in os.listdir(_build.CSRC_DIR)
                  if os.path.isfile(os.path.join(_build.CSRC_DIR, name)))


def test_every_file_of_csrc_is_a_source_or_a_header():
    sources = {name for name in _build.SOURCES}
    headers = {name for name in _build.HEADERS}
    assert len(sources) == len(_build.SOURCES) and len(headers) == len(_build.HEADERS), "a file is listed twice"
    for path in csrc_files():
        name = os.path.basename(path)
        if name.endswith((".hip", ".cpp")):
            assert name in sources, "%s is not in _build.SOURCES" % name
        elif name.endswith(".h"):
            assert name in headers, "%s is not in _build.HEADERS" % name
    for path in members():
        assert os.path.isfile(path), "%s is listed and not there" % path


def test_every_quoted_include_is_a_member():
    listed = members()
    seen = 0
    for path in csrc_files():
        for target in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), re.M):
            seen += 1
            resolved = os.path.normpath(os.path.join(os.path.dirname(path), target))
            assert resolved in listed, "%s includes %s, which is in neither SOURCES nor HEADERS" % (os.path.basename(path), target)
    assert seen > 20


def test_no_unit_is_compiled_twice_under_a_macro():
    """No unit is another file's #include, and nothing defines or tests a which-unit-am-I macro (ACMPC_<NAME>_TU:
    ACMPC_TEMPORAL_TU once, then ACMPC_DYNAMIC_TERMS_TU and three more)."""
    units = {os.path.normpath(os.path.join(_build.CSRC_DIR, name)) for name in _build.SOURCES}
    for path in csrc_files():
        text = open(path).read()
        for target in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M):
            resolved = os.path.normpath(os.path.join(os.path.dirname(path), target))
            assert resolved not in units, "%s includes the unit %s" % (os.path.basename(path), target)
        found = re.search(r"\bACMPC_\w+_TU\b", text)
        assert found is None, "%s: %s" % (os.path.basename(path), found and found.group(0))


def test_the_lds_limit_is_keyed_by_the_kernel():
    calls = 0
    for path in csrc_files():
        text = re.sub(r"//[^\n]*", "", open(path).read())
        # calls only: the helper's own definition has a parameter list, which names types
        for m in re.finditer(r"\braise_lds_limit\s*(<[^;{]*?>)?\s*\(([^;{]*?)\)\s*;", text, re.S):
            calls += 1
            arguments = (m.group(1) or "") + " , " + m.group(2)
            for piece in arguments.split(","):
                assert not re.fullmatch(r"\s*[<(]?\s*[-+]?(0[xX][0-9a-fA-F]+|\d+)[uUlL]*\s*[>)]?\s*", piece), \
                    "%s: raise_lds_limit(%s) passes a number" % (os.path.basename(path), m.group(0))
    assert calls >= 1
