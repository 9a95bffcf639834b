"""modkit_amd/csrc/mkp_launch.h is the only place a kernel launcher is declared (no GPU, nothing is run).

The launchers are extern "C": their parameter types are not part of the symbol name, so a prototype written by hand into a host file
that drifts from the definition still links and passes wrong arguments at run time.  With one header that both sides include, the
compiler compares every definition with its prototype.  Checked here: the header compiles on its own with the host flags of the
Makefile's mkp_api.o rule; no other file under modkit_amd/csrc declares an extern "C" function returning hipError_t without a body; every
launcher the header declares is defined in a .hip file that includes the header, and every one defined there is declared in it."""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modkit_amd", "csrc")
HEADER = "mkp_launch.h"


def code_only(text):
    """Comments out, string and character literals emptied (the "C" of a linkage specification stays)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r'"(?:\\.|[^"\\\n])*"', lambda m: m.group(0) if m.group(0) == '"C"' else '""', text)
    return re.sub(r"'(?:\\.|[^'\\\n])'", "' '", text)


def closing(text, i, open_ch, close_ch):
    """Index behind the bracket that closes the one at text[i]."""
    depth = 0
    for k in range(i, len(text)):
        if text[k] == open_ch:
            depth += 1
        elif text[k] == close_ch:
            depth -= 1
            if depth == 0:
                return k + 1
    raise AssertionError("unbalanced %s" % open_ch)


def c_linkage_hip_functions(text):
    """(name, has_body) of every function returning hipError_t that has C linkage: `extern "C" hipError_t f(...)` or inside `extern "C" {`."""
    text = code_only(text)
    blocks = []
    for m in re.finditer(r'extern\s+"C"\s*\{', text):
        blocks.append((m.end(), closing(text, m.end() - 1, "{", "}")))
    out = []
    for m in re.finditer(r'(extern\s+"C"\s+)?hipError_t\s+(\w+)\s*\(', text):
        if not m.group(1) and not any(a <= m.start() < b for a, b in blocks):
            continue
        end = closing(text, m.end() - 1, "(", ")")
        nxt = re.match(r"\s*(.)", text[end:], flags=re.S).group(1)
        assert nxt in ";{", "%s: neither a declaration nor a definition" % m.group(2)
        out.append((m.group(2), nxt == "{"))
    return out


def sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".hpp", ".hip", ".cpp", ".c")))


def test_the_scan_tells_declarations_from_definitions():
    text = ('extern "C" hipError_t a(int x, void (*f)(int));\n// extern "C" hipError_t b(int);\nextern "C" {\nhipError_t c(int x) { return g("};"); }\n'
            'hipError_t d(\n    int x);\n}\nhipError_t e(int);\nstatic hipError_t f(int) { return hipSuccess; }\n')
    assert c_linkage_hip_functions(text) == [("a", False), ("c", True), ("d", False)]


def test_header_stands_alone(tmp_path):
    # the recipe of mkp_api.o as make would run it, with the one-line file in place of mkp_api.cpp and nothing written
    recipe = subprocess.check_output(["make", "-n", "-W", "mkp_api.cpp", "-C", CSRC, "--no-print-directory", "mkp_api.o"], text=True)
    cmd = next(shlex.split(ln) for ln in recipe.splitlines() if "mkp_api.cpp" in ln)
    assert "-Wall" in cmd and "-x" in cmd
    one = tmp_path / "one.cpp"
    one.write_text('#include "%s"\n' % HEADER)
    cmd = [a for a in cmd if a not in ("-c", "-o", "mkp_api.o")]
    cmd = [str(one) if a == "mkp_api.cpp" else a for a in cmd] + ["-fsyntax-only", "-Werror", "-I", CSRC]
    p = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_launchers_are_declared_in_the_header_only():
    declared = c_linkage_hip_functions(open(os.path.join(CSRC, HEADER)).read())
    assert declared and all(not body for _, body in declared), "the header holds prototypes only"
    names = [n for n, _ in declared]
    assert len(set(names)) == len(names)
    defined = {}
    for f in sources():
        if f == HEADER:
            continue
        text = open(os.path.join(CSRC, f)).read()
        found = c_linkage_hip_functions(text)
        stray = [n for n, body in found if not body]
        assert not stray, "%s declares %s: launchers are declared in %s only" % (f, ", ".join(stray), HEADER)
        if found:
            assert f.endswith(".hip"), "%s defines %s: launchers live beside their kernels" % (f, found[0][0])
            assert re.search(r'^#include "%s"' % re.escape(HEADER), text, flags=re.M), "%s defines launchers unchecked: it does not include %s" % (f, HEADER)
        for n, _ in found:
            assert n not in defined, "%s is defined twice" % n
            defined[n] = f
    assert sorted(defined) == sorted(names)
    # the one entry point that returns no hipError_t: declared in the header, defined in mkp_merge.hip, named with its type nowhere else
    where = [f for f in sources() if re.search(r"\buint32_t\s+mkp_merge_tiles\s*\(", code_only(open(os.path.join(CSRC, f)).read()))]
    assert where == sorted([HEADER, "mkp_merge.hip"])
