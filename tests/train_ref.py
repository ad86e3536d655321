"""matlab/learning/pointtobox.m, train.m:73-121 and trainmodel.m restated line by line, as the sequences of calls and the numbers
partsbaseddetector_amd.train must produce (tests/test_train_cpu.py), and the recording fakes those tests drive it with.  No GPU."""
import math

import numpy as np

from partsbaseddetector_amd import capi
from partsbaseddetector_amd.detector import PartsBasedDetector


# ---- pointtobox.m ---------------------------------------------------------------------------------------------------------------------
def quantile7(x, p):
    """quantile(x, p, 1, 7): h = (N - 1) p on the sorted x, linear between the order statistics floor(h) and floor(h) + 1.  The
    interpolation is written as numpy's default writes it — a + (b - a) t below t = .5, b - (b - a) (1 - t) from there on —, which is
    the same number in exact arithmetic and the form whose rounding the comparison is exact against."""
    x = sorted(float(v) for v in x)
    h = (len(x) - 1) * p
    lo = int(math.floor(h))
    hi = min(lo + 1, len(x) - 1)
    t = h - lo
    a, b = x[lo], x[hi]
    return b - (b - a) * (1 - t) if t >= 0.5 else a + (b - a) * t


def median(x):
    x = sorted(float(v) for v in x)
    n = len(x)
    return x[n // 2] if n % 2 else (x[n // 2 - 1] + x[n // 2]) / 2


def point_to_box(points, pa):
    """pointtobox.m with 0-based parents (pa[0] = -1): -> [n][P][4] rows (x1, y1, x2, y2)"""
    points = np.asarray(points, np.float64)
    n, P = points.shape[:2]
    length = [[0.0] * (P - 1) for _ in range(n)]
    for i in range(n):                                             # :4-9
        for p in range(1, P):
            dx = abs(points[i, p, 0] - points[i, pa[p], 0])
            dy = abs(points[i, p, 1] - points[i, pa[p], 1])
            length[i][p - 1] = float(np.sqrt(dx * dx + dy * dy))   # norm of a 2-vector
    r = [0.0] * (P - 1)
    for j in range(P - 1):                                         # :11-15
        ratio = [float(np.log(length[i][j]) - np.log(length[i][0])) for i in range(n)]
        r[j] = float(np.exp(median(ratio)))
    boxes = np.zeros((n, P, 4), np.float64)
    for i in range(n):                                             # :20-34
        boxsize = quantile7([length[i][j] / r[j] for j in range(P - 1)], 0.85)
        for p in range(P):
            boxes[i, p] = (points[i, p, 0] - boxsize / 2, points[i, p, 1] - boxsize / 2,
                           points[i, p, 0] + boxsize / 2, points[i, p, 1] + boxsize / 2)
    return boxes


# ---- the recording fakes --------------------------------------------------------------------------------------------------------------
class FakeModel:
    """what train() reads of a model"""
    def __init__(self, interval=10, thresh=0.25):
        self.interval, self.thresh = interval, thresh

    def qp_vectors(self):
        return np.zeros(3), np.array([1.0, .01, 1.0]), np.array([0.0, 0.0, .01]), np.array([2], np.uint32)


class FakeCache:
    """capi.QpCache's method names.  script: written = examples every positive call writes; mine = per negative image (records, action);
    bounds = (lb, ub, passes) of every opt; thresh = what positive_threshold answers; fail_at = the mining call that raises."""
    def __init__(self, log, capacity, script):
        self.log, self.cap, self.script = log, capacity, script
        self.n, self.sv, self.handle, self.mined = 0, 0, None, 0

    def noneg(self, idx):
        self.log.append(("noneg", tuple(int(v) for v in idx)))

    def clear(self):
        self.log.append(("clear",))
        self.n = self.sv = 0

    def _append(self, k):
        k = min(k, self.cap - self.n)
        self.n += k
        self.sv += k
        return k

    def dims(self):
        return (3, 8, self.cap, self.n)

    def support(self):
        return np.array([1] * self.sv + [0] * (self.n - self.sv), np.uint8)

    def fix(self, n):
        self.log.append(("fix", int(n)))

    def prune(self):
        self.log.append(("prune",))
        return self.n

    def opt(self, tol=.05, max_iter=1000, seed=0):
        self.log.append(("opt", tol, max_iter, seed))
        return self.script["bounds"]

    def one(self, order):
        self.log.append(("one", len(order)))

    def apply_weights(self):
        self.log.append(("apply_weights",))

    def mine(self, im, id):
        self.log.append(("mine", im, int(id)))
        if self.script.get("fail_at") == self.mined:
            raise RuntimeError("mining failed")
        rec, act = self.script["mine"][self.mined]
        self.mined += 1
        return rec, self._append(rec), act

    def positive_threshold(self, q=.05):
        self.log.append(("positive_threshold", q))
        return self.script["thresh"], self.n


class FakeDetector:
    """PartsBasedDetector's method names; mineNegatives is the real one, run on the fake cache"""
    def __init__(self, log, model):
        self.log, self.model, self.handle = log, model, object()

    @property
    def interval(self):
        return self.model.interval

    def setInterval(self, v):
        self.log.append(("setInterval", int(v)))
        self.model.interval = int(v)

    def setThresh(self, t):
        self.log.append(("setThresh", float(t)))
        self.model.thresh = float(t)

    def writeWarped(self, im, boxes, cache, filter=None, bias=None, ids=None):
        self.log.append(("writeWarped", im, [tuple(b) for b in boxes], list(ids)))
        return cache._append(cache.script["written"]), None

    def latentPositives(self, positives, cache, overlap=0.6, first_id=1):
        self.log.append(("latentPositives", [tuple(p) for p in positives], overlap, first_id))
        return np.array([cache._append(cache.script["written"] * len(positives))]), []

    mineNegatives = PartsBasedDetector.mineNegatives


def run_fake(train, positives, negatives, warp, script, capacity=None, **kw):
    """train() on the fakes -> (log, report, the detector, the exception that left it or None)"""
    log = []
    det = FakeDetector(log, FakeModel())
    cap = capacity if capacity is not None else int(10 * (kw.get("wpos", 2) + 1) * len(positives))
    cache = FakeCache(log, cap, script)
    cache.handle = det.handle
    try:
        _, report = train(None, positives, negatives, warp, detector=det, cache=cache, **kw)
        return log, report, det, None
    except RuntimeError as e:
        return log, None, det, e


# ---- train.m:73-121 as the calls it makes ---------------------------------------------------------------------------------------------
def train_calls(positives, negatives, warp, script, capacity, iter=1, overlap=0.6, tol=.05, max_iter=1000, seed=0, interval0=10,
                thresh0=0.25):
    """the sequence train.m:73-121 prescribes, with the cache's counts kept by hand"""
    calls = [("noneg", (2,))]                                      # :68 model2vec's noneg, once
    solve = ("opt", tol, max_iter, seed)
    for _t in range(iter):                                         # :73
        calls.append(("clear",))                                   # :75
        n = 0
        if warp > 0:                                               # :76-77 poswarp, one qp_poswrite(feat, i, model) per positive
            for i, (im, box) in enumerate(positives):
                calls.append(("writeWarped", im, [tuple(box)], [i + 1]))
                n = min(n + script["written"], capacity)
        else:                                                      # :79 poslatent(name, t, model, pos, overlap), ids 1 ..
            calls.append(("latentPositives", [tuple(p) for p in positives], overlap, 1))
            n = min(script["written"] * len(positives), capacity)
        calls += [("fix", n), ("prune",), solve, ("apply_weights",)]   # :90-94
        calls += [("setInterval", 2), ("setThresh", -1.0)]         # :95-96; :102 detect(im, model, -1, ...)
        sv = n
        for i, im in enumerate(negatives):                         # :99
            calls.append(("mine", im, i + 1))                      # :102 id = i
            if script.get("fail_at") == i:
                calls += [("setThresh", thresh0), ("setInterval", interval0)]
                return calls
            rec, act = script["mine"][i]
            wr = min(rec, capacity - n)
            n += wr
            sv += wr
            if act == capi.PBD_MINE_OPT:                           # detect.m:319-321
                calls += [solve, ("prune",)]
            elif act == capi.PBD_MINE_ONE:                         # detect.m:322-323
                calls.append(("one", sv))
            if act != capi.PBD_MINE_NONE:
                calls.append(("apply_weights",))
            if sv == capacity:                                     # :105
                break
        calls += [solve, ("apply_weights",)]                       # :111-112
        calls += [("positive_threshold", .05), ("setThresh", float(np.float32(script["thresh"])))]   # :116-118
        calls.append(("setInterval", interval0))                   # :121
    return calls


# ---- trainmodel.m as the train() calls it makes -----------------------------------------------------------------------------------------
def trainmodel_calls(images, boxes, idx, K, negatives):
    """(what, number of filters of the model handed in, positives, negatives, warp) per train() call of trainmodel.m:19-63; boxes
    [n][P][4] from pointtobox, idx[p][i] 0-based"""
    calls = []
    P = len(K)
    for p in range(P):                                             # :19
        sneg = negatives[:min(len(negatives), 100)]                # :24
        for k in range(K[p]):                                      # :27
            spos = [(images[i], tuple(boxes[i][p])) for i in range(len(images)) if idx[p][i] == k]   # :28-34
            calls.append((("part", p, k), 1, spos, sneg, 1))       # :35 train(cls, model, spos, sneg, 1, 1)
    with_mix = [(images[i], [int(idx[p][i]) for p in range(P)]) for i in range(len(images))]        # :47-51
    calls.append(("final1", sum(K), with_mix, negatives, 0))       # :52
    calls.append(("final", sum(K), [(images[i], None) for i in range(len(images))], negatives, 0))  # :60-63
    return calls
