"""Part mixtures on the device (k_kmeans.hip; include/pbd_c.h "part mixtures") against pbd_cluster_parts_host, which
tests/test_kmeans_cpu.py holds to the MATLAB files: every output of pbd_cluster_parts — labels, centroids with their NaN, sumdists,
winners, per-trial sumdists and pass counts, the capped count — must equal the host's bit for bit, on integer and on float data alike.
No tolerance appears anywhere.  And the model that Model.build_model assembles from such labels runs on a handle."""
import os
import subprocess

import numpy as np
import pytest

from partsbaseddetector_amd import capi
from partsbaseddetector_amd import model as M
from tests import kmeans_ref as ref
from tests.util import assert_candidates_equal, thresh_from_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TREES = {2: ([-1, 0], ([1, 32], [6, 2])), 5: ([-1, 0, 1, 1, 0], ([1, 2, 6, 32, 6], [2, 2, 1, 6, 32]))}
KEYS = ("idx", "centres", "sumdist", "best_trial", "trial_sumdist", "trial_iters")


def make_def(kind, P, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "int":   # few distinct points: starts repeat and clusters run empty (the NaN path)
        return rng.integers(-2, 3, (P, n, 2)).astype(np.float64)
    centres = rng.uniform(-20, 20, (P, 6, 2))
    return np.stack([centres[p][rng.integers(0, 6, n)] + rng.normal(0, 1.5, (n, 2)) for p in range(P)])


def assert_same(got, want):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["capped"] == want["capped"]


@pytest.mark.parametrize("R", [1, 3, 100])
@pytest.mark.parametrize("P", [2, 5])
def test_device_equals_host_in_bits(P, R):
    parents, Ks = TREES[P]
    nan_seen = 0
    for n in (1, 63, 64, 65, 130):
        for kind in ("int", "float"):
            for K in Ks:
                d = make_def(kind, P, n, 1000 * n + P)
                want = capi.cluster_parts_host(d, parents, K, R=R, seed=n + R, max_iter=1000)
                got = capi.cluster_parts(d, parents, K, R=R, seed=n + R, max_iter=1000)
                assert_same(got, want)
                assert want["capped"] == 0
                nan_seen += bool(np.isnan(got["centres"]).any())
    assert nan_seen >= 1   # 32 clusters on at most 25 distinct points: empty clusters are certain


def test_person_size():
    d = make_def("float", 26, 300, 4)
    want = capi.cluster_parts_host(d, M.PERSON_TREE, 6, R=100, seed=2024, max_iter=1000)
    got = capi.cluster_parts(d, M.PERSON_TREE, 6, R=100, seed=2024, max_iter=1000)
    assert_same(got, want)
    assert want["capped"] == 0 and got["idx"].max() == 5


def test_seeds_change_the_starts_not_the_agreement():
    parents, K = [-1, 0, 1, 1, 0], [3, 6, 2, 4, 6]
    d = make_def("float", 5, 130, 9)
    runs = []
    for seed in (1, 2 ** 63 + 12345):
        want = capi.cluster_parts_host(d, parents, K, R=7, seed=seed, max_iter=1000)
        assert_same(capi.cluster_parts(d, parents, K, R=7, seed=seed, max_iter=1000), want)
        runs.append(want)
    assert runs[0]["trial_sumdist"].tobytes() != runs[1]["trial_sumdist"].tobytes()


@pytest.mark.parametrize("max_iter", [1, 2, 3])
def test_capped_trials(max_iter):
    parents, K = [-1, 0, 0], [3, 6, 2]
    d = make_def("float", 3, 200, 12)
    want = capi.cluster_parts_host(d, parents, K, R=6, seed=3, max_iter=max_iter)
    assert_same(capi.cluster_parts(d, parents, K, R=6, seed=3, max_iter=max_iter), want)
    assert want["capped"] > 0


def test_device_refusals_and_bad_device():
    d = make_def("int", 2, 8, 1)
    for kw, code in ((dict(K=[2, 33]), capi.PBD_ERR_UNSUPPORTED), (dict(K=[2, 0]), capi.PBD_ERR_ARG), (dict(R=0), capi.PBD_ERR_ARG),
                     (dict(R=capi.PBD_CLUSTER_MAX_TRIALS // 2 + 1), capi.PBD_ERR_UNSUPPORTED),
                     (dict(max_iter=0), capi.PBD_ERR_ARG), (dict(device=4096), capi.PBD_ERR_HIP)):
        args = dict(K=[2, 2], R=2, max_iter=10)
        args.update(kw)
        with pytest.raises(capi.PbdError) as e:
            capi.cluster_parts(d, [-1, 0], **args)
        assert e.value.code == code, kw


def test_cpp_layer(tmp_path):
    """pbd::clusterParts (tests/tools/cluster_parts_check.cpp) gives the host function's labels and throws the header's refusal"""
    parents, K, n, R, seed = [-1, 0, 1, 1, 0], [3, 6, 2, 32, 1], 130, 9, 2 ** 40 + 5
    d = make_def("float", 5, n, 31)
    want = capi.cluster_parts_host(d, parents, K, R=R, seed=seed, max_iter=1000)
    exe = tmp_path / "cluster_parts_check"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", str(exe), os.path.join(ROOT, "tests", "tools", "cluster_parts_check.cpp"),
                           "-L" + lib_dir, "-lpbd_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    d.tofile(str(tmp_path / "def.bin"))
    np.asarray(parents, np.int32).tofile(str(tmp_path / "parent.bin"))
    np.asarray(K, np.int32).tofile(str(tmp_path / "K.bin"))
    out = subprocess.run([str(exe), str(tmp_path / "def.bin"), str(tmp_path / "parent.bin"), str(tmp_path / "K.bin"), str(n), str(R), str(seed)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = dict(l.split(" ", 1) for l in out.stdout.splitlines())
    for p in range(5):
        assert [int(v) for v in lines[f"part{p}"].split()] == want["idx"][p].tolist(), p
    assert int(lines["capped"]) == want["capped"] == 0 and int(lines["refused"]) == capi.PBD_ERR_UNSUPPORTED


def test_assembled_model_runs(orc):
    """annotations -> labels on the device -> build_model: the handle takes the model, and a frame detects exactly as on a twin laid
    out by hand from the same labels"""
    parents, K, n = [-1, 0, 1, 1, 0], [3, 2, 3, 1, 2], 60
    rng = np.random.default_rng(21)
    w = h = rng.integers(30, 80, n).astype(np.float64)
    base = M.init_model(w, h, 4, (3, 3))
    pts = np.cumsum(rng.normal(0, 25, (n, 5, 2)), axis=1) + 200
    d = M.data_def(pts, w, h, base.filter_sizes()[0])
    idx = capi.cluster_parts(d, parents, K, R=20, seed=1)["idx"]
    assert [int(idx[p].max()) + 1 for p in range(5)] == K
    pm = []
    for p in range(5):
        ones = []
        for k in range(K[p]):
            m = M.init_model(w, h, 4, (3, 3))
            m.filtersw = M._filters(rng, 1, 3, 3, 32)
            ones.append(m)
        pm.append(M.merge_models(ones))
    jm = M.build_model(pm, d, idx, parents)
    # the twin: make_tree_model_k's ids, the file's anchors, the weights put in by hand
    twin = M.make_tree_model_k(parents, K, kh=3, kw=3, sbin=4, interval=10)
    twin.filtersw = [pm[p].filtersw[k] for p in range(5) for k in range(K[p])]
    twin.biasw = np.zeros_like(twin.biasw)
    twin.defw = np.tile(np.float32([.01, 0, .01, 0]), (len(twin.defw), 1))
    r = ref.buildmodel([m.filtersw for m in pm], list(d), list(idx + 1), [p + 1 for p in parents])
    twin.anchors = (np.array([a[:2] for _, _, a in r["defs"]]) - 1).astype(np.int32)
    im = M.make_image(3, 160, 120)
    jm.thresh = twin.thresh = thresh_from_oracle(orc, jm, im, 99.0)
    ha, hb = capi.Handle(jm, conv_mode=capi.PBD_CONV_EXACT), capi.Handle(twin, conv_mode=capi.PBD_CONV_EXACT)
    try:
        a, b = ha.detect(im), hb.detect(im)
        assert len(a[0]) > 0
        assert_candidates_equal(a, b)
    finally:
        ha.close()
        hb.close()
