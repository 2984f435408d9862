"""The pass plan of a wide sender's fused push (csrc/pass_plan.h), checked on the host.

tests/pass_plan_check.cpp includes the same header the kernel includes and walks every degree
17..512 against every active-word count 1..64 and 300 random masks per degree: every pass fits
the 2048-cell LDS table, the connection groups (<= 64 connections, one group when deg <= 64)
partition [0, deg), the word ranges of a group cover the active words exactly once, and the
flush needs no more store instructions than the chunked push (up to pass rounding).  Built with
the host compiler, with AddressSanitizer / UBSan where the toolchain links them.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "python-p2p-network_amd", "csrc")
SRC = os.path.join(HERE, "pass_plan_check.cpp")


def _compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_pass_plan_every_degree_and_mask(tmp_path):
    cxx = _compiler()
    exe = str(tmp_path / "pass_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0:  # (a toolchain without the sanitizer runtimes)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    word, cases = run.stdout.split()
    # 496 degrees x (64 counts + 300 random masks)
    assert word == "ok" and int(cases) == 496 * 364, run.stdout
