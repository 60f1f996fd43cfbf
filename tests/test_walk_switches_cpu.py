"""No GPU: the DFH_* switches of the walks and the launchers (csrc/walk_knobs.h) as dfh_walk_switches prints them.  The library reads
the environment once per process, so every case here is a child process of its own."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from difashion_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "difashion_amd", "csrc")
# names, order and defaults, kept apart from the header's list so that an edit there has to be made twice
DEFAULT = open(os.path.join(ROOT, "tests", "golden", "walk_switches_default.txt")).read()
NAMES = [l.split("=")[0] for l in DEFAULT.splitlines()]
OFF_AT_0 = {n for n, v in (l.split("=") for l in DEFAULT.splitlines()) if v == "1"}
ON_AT_1 = {"DFH_FP8_ATTN", "DFH_TOKEN_LINEAR", "DFH_CHECK_DUP"}
DOUBLES = {"DFH_TRAIN_SIDE_MIN_FLOP"}
INTS = set(NAMES) - OFF_AT_0 - ON_AT_1 - DOUBLES

CHILD = ("import ctypes as C, sys\n"
         "f = C.CDLL(sys.argv[1]).dfh_walk_switches; f.restype = C.c_size_t; f.argtypes = [C.c_char_p, C.c_size_t]\n"
         "n = f(None, 0); b = C.create_string_buffer(n + 1); assert f(b, n + 1) == n == len(b.value)\n"
         "sys.stdout.write(b.value.decode())\n")


def switches(env=None, lib="libdifashion_hip.so"):
    base = {k: v for k, v in os.environ.items() if not k.startswith("DFH_")}
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(CSRC, lib)], capture_output=True, text=True, env={**base, **(env or {})}, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def value(name, text):
    return switches({name: text}).splitlines()[NAMES.index(name)].split("=")[1]


@pytest.mark.parametrize("lib", ["libdifashion_hip.so", "libdifashion_hip_f16.so"])
def test_nothing_set_prints_the_defaults(lib):
    _lib.build()
    assert switches(lib=lib) == DEFAULT
    assert len(NAMES) == len(set(NAMES)) == 29 and len(OFF_AT_0) == 14 and len(INTS) == 11


@pytest.mark.parametrize("name", NAMES)
def test_one_name_changes_its_own_line_only(name):
    text, want = ("0", "0") if name in OFF_AT_0 else ("1", "1") if name in ON_AT_1 else ("1.5e9", "1.5e+09") if name in DOUBLES else ("7", "7")
    got, ref = switches({name: text}).splitlines(), DEFAULT.splitlines()
    i = NAMES.index(name)
    assert got[i] == f"{name}={want}" != ref[i]
    assert got[:i] + got[i + 1:] == ref[:i] + ref[i + 1:]


@pytest.mark.parametrize("name,text,want", [
    ("DFH_LN_FOLD", "0", "0"), ("DFH_LN_FOLD", "1", "1"), ("DFH_LN_FOLD", "", "1"), ("DFH_LN_FOLD", "00", "0"), ("DFH_LN_FOLD", "01", "0"),
    ("DFH_LN_FOLD", "off", "1"),                                                                  # off only at a leading '0'
    ("DFH_FP8_ATTN", "0", "0"), ("DFH_FP8_ATTN", "1", "1"), ("DFH_FP8_ATTN", "", "0"), ("DFH_FP8_ATTN", "00", "0"), ("DFH_FP8_ATTN", "10", "1"),
    ("DFH_FP8_ATTN", "on", "0"),                                                                  # on only at a leading '1'
    ("DFH_WINO", "abc", "0"), ("DFH_WINO", "", "0"), ("DFH_GN_FOLD", "12abc", "12"), ("DFH_GN_FOLD", "-1", "-1"),     # atoi
    ("DFH_TRAIN_SIDE_MIN_FLOP", "zzz", "0"), ("DFH_TRAIN_SIDE_MIN_FLOP", "0", "0"),                                   # atof
])
def test_parse_edges(name, text, want):
    assert value(name, text) == want


def test_text_is_cut_to_the_buffer_and_the_python_mirror_reads_it():
    lib = _lib.raw()
    full = lib.dfh_walk_switches(None, 0)
    assert full == len(DEFAULT.encode()) or any(k.startswith("DFH_") for k in os.environ)      # lengths differ only with values set
    buf = C.create_string_buffer(b"x" * 31, 32)
    assert lib.dfh_walk_switches(buf, 16) == full and buf.raw[:16] == DEFAULT.encode()[:15] + b"\0" and buf.raw[16:31] == b"x" * 15
    assert list(_lib.walk_switches()) == NAMES


def test_the_struct_lists_every_name_and_nothing_else_reads_the_environment():
    """walk_knobs.h declares exactly the names of the golden file, in its order; under csrc/ only WalkKnobs::get(), GemmKnobs::from_env()
    and the two file-path variables call getenv."""
    listed = re.findall(r"^\s*X\(\w+, \w+, (DFH_\w+), \w+, [^)]+\)", open(os.path.join(CSRC, "walk_knobs.h")).read(), flags=re.M)
    assert listed == NAMES
    allowed = {"walk_knobs.hip": None, "gemm_plan.hip": None, "api.hip": {"DFH_PROF_DUMP"}, "gemm.hip": {"DFH_GEMM_PLAN_DUMP"}}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".h")):
            continue
        src = open(os.path.join(CSRC, f)).read()
        calls = re.findall(r"getenv\s*\(\s*([^)]*)\)", src)
        if f not in allowed:
            assert not calls, (f, calls)
        elif allowed[f] is not None:
            assert {c.strip('"') for c in calls} == allowed[f], (f, calls)
    walk, plan = open(os.path.join(CSRC, "walk_knobs.hip")).read(), open(os.path.join(CSRC, "gemm_plan.hip")).read()
    assert 'getenv("DFH_' not in walk and walk.count("getenv(") == 1                  # the one read, over the list of the header
    assert not set(re.findall(r'"(DFH_\w+)"', plan)) & set(NAMES)                     # the GEMM plan's names are its own
