"""The host side of the netsplit (csrc/netsplit.h, and its part of csrc/round_plan.h), checked on
the host.

tests/netsplit_check.cpp includes the same headers the engine and the kernels include: the cut
predicate at the window's edges, validation, the window's questions (cut round, cut sends, a round
the cut acts on at or ahead) against brute force over every small window, the crossing count against
brute force over 200 random graphs and sides, and the plan of every round a netsplit acts on (never
fused, never update+push, whole rows, the cut push, not held, no batch while one lies ahead).  Built
with the host compiler, with AddressSanitizer / UBSan where the toolchain links them.  The exported
helper p2pg_link_cut is checked against the Python rule, and the library exports both entry points.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import netsplit_ref

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "python-p2p-network_amd", "csrc")
SRC = os.path.join(HERE, "netsplit_check.cpp")


def _compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_netsplit_header_window_crossing_count_and_plans(tmp_path):
    cxx = _compiler()
    exe = str(tmp_path / "netsplit_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0:  # (a toolchain without the sanitizer runtimes)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 5_000, run.stdout


def test_link_cut_export_equals_the_python_rule():
    from p2pnetwork.gpu import GraphNetwork, _lib
    L = _lib.lib()
    rng = np.random.default_rng(5)
    for _ in range(2000):
        t, cf, cu = (int(x) for x in rng.integers(0, 12, 3))
        a, b = (int(x) for x in rng.integers(0, 3, 2))
        want = bool(netsplit_ref.link_cut(t, a, b, cf, cu))
        assert bool(L.p2pg_link_cut(t, a, b, cf, cu)) == want
        assert GraphNetwork.link_cut(t, a, b, cf, cu) == want
    assert L.p2pg_link_cut(0x7FFFFFFE, 0, 1, 0, 0x7FFFFFFF) == 1
    assert L.p2pg_link_cut(5, 0, 1, 7, 3) == 0


def test_the_library_exports_the_entry_points():
    from p2pnetwork.gpu import CompatNetwork, GraphNetwork, _lib
    L = _lib.lib()
    for name in ("p2pg_set_netsplit", "p2pg_link_cut"):
        assert name in _lib.SIGNATURES and isinstance(getattr(L, name), ctypes._CFuncPtr)
    assert hasattr(GraphNetwork, "set_netsplit") and not hasattr(CompatNetwork, "set_netsplit")
