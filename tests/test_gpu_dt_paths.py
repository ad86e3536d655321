"""The distance transform's rare paths on the GPU (k_dt_pass: validation rounds, stitch redos, flagged lines redone
sequentially, the fused / unfused arithmetic around its limits), case by case from tests/dt_path_cases.py:
(a) the product library's result is bit-identical to the oracle's (scores and pointers);
(b) the probe build (`make probes`, PBD_PROBES), run in a fresh child process, counts every path the case names
    (pbd_debug_dt_counters) — at least as often as the host replay (tests/tools/dt_replay.cpp) proves it must where that count
    does not depend on the order in which the lanes of a block run — and its result matches the oracle too."""
import json
import os
import subprocess
import sys

import pytest

from tests import dt_path_cases as dc

pytestmark = pytest.mark.gpu
PROBES = os.path.join(dc.ROOT, "partsbaseddetector_amd", "libpbd_hip_probes.so")


@pytest.fixture(scope="session")
def probe_lib():
    subprocess.check_call(["make", "-s", "-j16", "-C", dc.CSRC, "probes"])
    return PROBES


@pytest.fixture(scope="module")
def replay_lib(tmp_path_factory):
    return dc.build_replay(tmp_path_factory.mktemp("dt_replay"))


def _child(name, lib_path):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PBD_DT_")}
    env["PBD_LIBRARY"] = lib_path
    r = subprocess.run([sys.executable, "-m", "tests.dt_path_cases", name], cwd=dc.ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (name, r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("name", [c["name"] for c in dc.ALL_CASES])
def test_dt_path_case(gpu_required, orc, probe_lib, replay_lib, name):
    case = dc.BY_NAME[name]
    bad = dc.run_case(case)                         # (a) the product library
    assert not bad, bad
    res = _child(name, probe_lib)                   # (b) the probe build
    assert res["rc"] == 0, res
    assert not res["match"], res["match"]
    got = res["counters"]
    gpu_paths = [p for p in case["paths"] if p in dc.COUNTERS]
    assert all(got[p] >= 1 for p in gpu_paths), (name, got)
    assert got["max_rounds"] >= case["min_rounds"], (name, got)
    assert got["seq_redos"] == got["scan_flags"] + got["stitch_flags"], (name, got)
    if case["kind"] == "dt2d":
        rep = dc.replay(replay_lib, case)[3]
        print(f"{name}: probe {got} | replay {rep}")
        # fixed by the data: local-scan flags; whether a line has a stale boundary at the first judgement (its stitches read
        # nothing below their neighbour's F before they are stale), hence the blocks that enter rounds — unless a stale
        # speculative stitch flags the line, which may depend on timing
        assert got["scan_flags"] == rep["scan_flags"], (name, got, rep)
        assert got["seq_redos"] >= rep["scan_flags"], (name, got, rep)
        if rep["stitch_flags"] == 0:
            assert got["round_blocks"] >= rep["round_blocks"], (name, got, rep)
    else:
        print(f"{name}: probe {got}")


def test_dt_counters_unsupported_in_the_product(gpu_required):
    from partsbaseddetector_amd import capi
    if os.environ.get("PBD_LIBRARY"):
        pytest.skip("PBD_LIBRARY names another build")
    rc, cnt = dc.probe_counters()
    assert rc == capi.PBD_ERR_UNSUPPORTED and not any(cnt.values())
