"""The distance transform's rare paths, on the host (no GPU): tests/tools/dt_replay.cpp replays pbd_dt2d exactly as k_dt_pass
processes it — the planner's own block geometry, local scans, speculative stitches, lowest-stale-first validation rounds, stitch
redos and sequential redos — and counts the paths it takes.  Every case of tests/dt_path_cases.py must still reach the paths it
names here, so that a change to the planner or to dt_core.hpp cannot quietly make tests/test_gpu_dt_paths.py vacuous; and the
replay itself must be bit-identical to the oracle.  Also: the two host statistics tools of tests/tools still compile."""
import os
import subprocess

import numpy as np
import pytest

from tests import dt_path_cases as dc

ROOT = dc.ROOT


@pytest.fixture(scope="module")
def replay_lib(tmp_path_factory):
    return dc.build_replay(tmp_path_factory.mktemp("dt_replay"))


@pytest.mark.parametrize("name", [c["name"] for c in dc.CASES])
def test_replay_reaches_the_named_paths(replay_lib, orc, name):
    case = dc.BY_NAME[name]
    out, ix, iy, cnt = dc.replay(replay_lib, case)
    ref = orc.dt2d(case["make"](), *case["q"], dtype=case["dtype"])
    np.testing.assert_array_equal(out.view(np.uint8), ref[0].view(np.uint8))
    np.testing.assert_array_equal(ix, ref[1])
    np.testing.assert_array_equal(iy, ref[2])
    missing = [p for p in case["paths"] if cnt[p] < 1]
    assert not missing, (name, missing, cnt)
    assert cnt["max_rounds"] >= case["min_rounds"], (name, cnt)
    # the planner's fused / unfused choice per pass (dt_mark_fused: float-born weights, len + |os| <= DT_FUSE_MAXLEN)
    assert cnt["fused_groups"] == case["fused"], (name, cnt)
    # bookkeeping that holds whatever the data: every flagged line is redone sequentially, every block with rounds runs one at least
    assert cnt["seq_redos"] == cnt["scan_flags"] + cnt["stitch_flags"]
    assert cnt["rounds"] >= cnt["round_blocks"] and cnt["stitch_redos"] >= cnt["round_blocks"]
    assert cnt["stitch_flags"] >= cnt["redo_flags"]


@pytest.mark.parametrize("tool", ["dt_rounds_stats.cpp", "dt_line_stats.cpp"])
def test_dt_statistics_tools_compile(tmp_path, tool):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I", dc.CSRC,
                           os.path.join(ROOT, "tests", "tools", tool), "-o", str(tmp_path / "tool")])
