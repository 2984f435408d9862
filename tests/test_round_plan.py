"""The host's round schedule (csrc/round_plan.h), checked on the host.

tests/round_plan_check.cpp includes the header the engine includes and

* replays two recorded config-4 runs (tests/golden/round_traces.json: W = 64, and W = 8 with its
  thresholds 0.04 / 0.95) round by round through plan_round, resolve_push and advance: the
  planned push forms are the recorded ones, and three rounds per run read their counters before
  their push (every round after round 0 that is not pushed blind);
* walks every combination of rules, capabilities and facts against four histories (empty,
  rising, dense, decaying; each with and without E pushes in its last round): a round with an
  origination, an expiry or a policy is unfused with whole rows, an expiry or policy round holds
  its push, the always-atomic / always-store overrides hold, round 0 reads nothing mid-round, a
  list sized by the last round's pushed masks has some, and a batchable decay tail is past the
  dense phase, filters as the batch always did and is what p2pg_step would plan.

Built with the host compiler, with AddressSanitizer / UBSan where the toolchain links them.
"""
import json
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "python-p2p-network_amd", "csrc")
SRC = os.path.join(HERE, "round_plan_check.cpp")
TRACES = os.path.join(HERE, "golden", "round_traces.json")

ATOMIC, EDGE, FUSED, UPDATE_EDGE = 1, 2, 3, 4


def _compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError("no host C++ compiler found")


def test_round_plan_replay_and_flag_grid(tmp_path):
    with open(TRACES) as f:
        traces = {t["name"]: t for t in json.load(f)["traces"]}
    # the recordings themselves: the fixture holds the runs the issue names
    forms = {name: [r[5] for r in t["rounds"]] for name, t in traces.items()}
    n64, n8 = len(forms["c4_w64"]), len(forms["c4_w8"])
    assert forms["c4_w64"] == [ATOMIC] * 10 + [UPDATE_EDGE] + [FUSED] * 13 + [ATOMIC] * (n64 - 24)
    assert forms["c4_w8"] == [ATOMIC] * 12 + [EDGE] + [FUSED] * 8 + [ATOMIC] * (n8 - 21)
    files = []
    for name in ("c4_w64", "c4_w8"):
        t = traces[name]
        up_cap = 1 if t["W"] > 16 else 0  # (gossip_update_push_supported: packed rows only)
        path = tmp_path / (name + ".txt")
        rows = "".join(" ".join(str(x) for x in r) + "\n" for r in t["rounds"])
        path.write_text(f"{t['W']} {t['v_conn']} {t['e_thresh']} {t['v_thresh']} {up_cap} {len(t['rounds'])}\n" + rows)
        files.append(str(path))

    cxx = _compiler()
    exe = str(tmp_path / "round_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, SRC, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    built = subprocess.run(base + san, capture_output=True, text=True)
    if built.returncode != 0:  # (a toolchain without the sanitizer runtimes)
        built = subprocess.run(base, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    # the mid-round reads: three per run (the line-for-line port of the rules this header replaced
    # finds the same three)
    assert lines[0].split() == ["replay", str(n64), "mid_reads", "3"], run.stdout
    assert lines[1].split() == ["replay", str(n8), "mid_reads", "3"], run.stdout
    word, cases = lines[2].split()
    # 4 histories x 2 x 54 rules x 384 capabilities (part_dense only on a partitioned rank) x
    # (96 facts (a policy only after round 0) + 256 decay facts), and the replayed rounds
    assert word == "ok" and int(cases) == 8 * 54 * 384 * (96 + 256) + n64 + n8, run.stdout
