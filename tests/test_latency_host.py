"""The host side of the delivery latency (csrc/latency.h), checked on the host.

tests/latency_check.cpp includes the same header the engine and the latency kernel include: the
bit-sliced start planes (tail bits never set; starts of 0 and -1 in no plane) and the per-word sum
of starts and smallest start under a frontier word, against a per-bit brute force over random words
and schedules -- M no multiple of 64, every start 0 (no planes), starts of -1 mixed in, a start of
2^30, and masks of 0, of one bit and of all ones.  Built with the host compiler, with
AddressSanitizer / UBSan where the toolchain links them.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "python-p2p-network_amd", "csrc")
SRC = os.path.join(HERE, "latency_check.cpp")


def _compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_latency_header_planes_sum_and_minimum(tmp_path):
    cxx = _compiler()
    exe = str(tmp_path / "latency_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0:  # (a toolchain without the sanitizer runtimes)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    word, cases = run.stdout.split()
    assert word == "ok" and int(cases) > 20_000, run.stdout
