"""The host side of peer downtime (csrc/downtime.h), checked on the host.

tests/downtime_check.cpp includes the same header the engine and the kernels include: the offline
predicate at the interval's edges, validation of every bad-interval kind, the refusal of
originations at an offline peer in both call orders, the sorted-endpoint sweep (peers offline in a
round, offline rounds ahead, the span min(from) .. max(until)) against a brute-force count over 300
random schedules, and the cases V = 1, all -1 and until = INT32_MAX.  Built with the host compiler,
with AddressSanitizer / UBSan where the toolchain links them.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "python-p2p-network_amd", "csrc")
SRC = os.path.join(HERE, "downtime_check.cpp")


def _compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_downtime_header_validation_refusals_and_sweep(tmp_path):
    cxx = _compiler()
    exe = str(tmp_path / "downtime_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0:  # (a toolchain without the sanitizer runtimes)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 40_000, run.stdout
