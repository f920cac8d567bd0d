"""Every KINHIP_* name the tools use is one the sources read (or define), or a variable the tools define for
themselves: a tool that sets a knob no source file reads measures nothing.  tools/ab.py's docstring is the one
list of the knobs."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"KINHIP_[A-Z0-9_]+")

# variables the tools define and read themselves (not knobs of the library)
TOOLS_OWN = {
    "KINHIP_LIB",                # the library a tool loads (kinhip/_lib.py reads it too)
    "KINHIP_CSRC",               # tools/jit_offline.py: where the device headers are
    "KINHIP_OFFLINE_DEFS",       # tools/jit_offline.py: definitions of its offline compile
    "KINHIP_SESSION_OUT",        # tools/gpu_session.sh: its output directory
    "KINHIP_DIST_ALWAYS_GROUP",  # bench.py's switch, set by tools/gpu_session.sh
}


def names_in(path, code_only=False):
    """The KINHIP_* names in a file; code_only leaves out its line comments (// in C++, # in Python / make)."""
    with open(path, errors="replace") as f:
        text = f.read()
    if code_only:
        text = re.sub(r"//.*" if path.endswith((".h", ".hip", ".cpp")) else r"(?m)(?:^|\s)#.*", "", text)
    return set(NAME.findall(text))


def source_names():
    found = names_in(os.path.join(ROOT, "bench.py"), code_only=True)
    pkg = os.path.join(ROOT, "kinematics.jl_amd")
    for d, dirs, files in os.walk(pkg):
        dirs[:] = [x for x in dirs if x not in ("lib", "__pycache__")]  # (build products)
        for f in files:
            found |= names_in(os.path.join(d, f), code_only=True)  # (a name kept only in a comment is not read)
    return found


def test_tools_name_only_knobs_that_exist():
    known = source_names() | TOOLS_OWN
    tools = os.path.join(ROOT, "tools")
    stale = {}
    for f in sorted(os.listdir(tools)):
        p = os.path.join(tools, f)
        if os.path.isfile(p):
            for n in sorted(names_in(p) - known):
                stale.setdefault(n, []).append(f)
    assert not stale, f"tools name knobs that no source file reads: {stale}"


def test_ab_docstring_lists_every_environment_knob():
    """The A/B build's environment knobs (ab_env / ab_env_int in csrc) all appear in tools/ab.py's list."""
    read = set()
    csrc = os.path.join(ROOT, "kinematics.jl_amd", "csrc")
    for f in os.listdir(csrc):
        with open(os.path.join(csrc, f), errors="replace") as fh:
            read |= set(re.findall(r'ab_env(?:_int)?\("(KINHIP_[A-Z0-9_]+)"', fh.read()))
    assert read, "no ab_env reads found"
    listed = names_in(os.path.join(ROOT, "tools", "ab.py"))
    assert read <= listed, sorted(read - listed)
