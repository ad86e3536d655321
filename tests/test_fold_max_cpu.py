"""The value form of a message (csrc/fold_pick.hpp: fold_max) against the one statement of the choice (fold_pick), bitwise, on the host.

The fold drops the winning mixture's index, so it takes `max_k(sd[k] + bias[k])` as a plain maximum seeded with -inf and falls back to
fold_pick's compare / select chain where the two can differ: a maximum that is a zero (tied zeros of both signs — the reference keeps
the first sign, a maximum instruction the positive one).  tests/tools/fold_max_test.cpp compares fold_max with fold_pick(...).v bit for
bit, float and double, N in {0, 1, 4, 6, 8} and K from 1 to N: 10^6 random vectors, every arrangement of {-0, +0, a negative value,
-inf} over K <= 4 positions under biases that make the sums tie, a NaN in each position, the K == 1 copy of NaN and -inf, padded repeats.
The same program runs once more built with the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "partsbaseddetector_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "tools", "fold_max_test.cpp")
# -ffp-contract=off as the library is built (sd + bias is an addition, never half of an fma)
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                      "-static-libasan", "-static-libubsan"]}   # (the runtimes inside the program)


@pytest.mark.parametrize("build", list(BUILDS))
def test_fold_max_is_fold_picks_value_bit_for_bit(tmp_path, build):
    exe = tmp_path / ("fold_max_test_" + build)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-ffp-contract=off", *BUILDS[build], "-I", CSRC, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) random, (\d+) zeros, (\d+) nan, (\d+) copy checks; (\d+) took the fold_pick path; (\d+) mismatches", r.stdout)
    assert m, r.stdout
    nrand, nzero, nnan, ncopy, unsure, bad = map(int, m.groups())
    assert bad == 0
    assert nrand == 10 ** 6
    # every arrangement of 4 values over K = 1..4 positions, 5 bias patterns, float and double, at least the K-entry and the 8-entry form
    assert nzero >= (4 + 16 + 64 + 256) * 5 * 2 * 2
    assert nnan >= 36 * 4 * 2 * 2 * 2 and ncopy >= 7 * 4 * 2 * 2
    # both paths are exercised: tied zeros took fold_pick's chain, most vectors did not
    assert 0 < unsure < (nrand + nzero + nnan + ncopy) // 2
