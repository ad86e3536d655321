"""Per-part scores of a detection, restated in numpy float64 from the contract in include/pbd_c.h (pbd_part_score).

For a candidate at level n of component c with part locations (x_p, y_p, m_p) and parent q of part p:
  app_p  = resp[n][filterid[p][m_p]](y_p, x_p), widened to double;
  def_p  = (a_x (dx dx) + b_x dx) + (a_y (dy dy) + b_y dy), dx = x_q + anchor_x - x_p, dy = y_q + anchor_y - y_p (ints, squared as
           ints), (a_x, b_x, a_y, b_y) = the negated float deformation weights of defid[p][m_p], widened; 0 for the root;
  bias_p = biasw[biasid[p][m_p] + m_q] (the child's mixture picks the base, the parent's the offset); root: biasw[biasid[0][0]].
The bound B = 4 P eps_T S of a detection's re-scored total against its root score: per part the DP rounds to T at most four
times (x pass read-out, y pass read-out, + bias, += into the parent) and no partial sum exceeds S = sum |app| + |def| + |bias|."""
import numpy as np

F64 = np.float64


def part_scores_ref(model, resp_of_level, heads, locs):
    """[n, max_parts, 3] float64 (app, def, bias); resp_of_level(l) -> the [nfilters, H, W] planes of level l; part slots beyond
    a component's parts stay zero."""
    n, mp = len(heads), model.max_parts
    out = np.zeros((n, mp, 3), F64)
    defw = np.asarray(model.defw, np.float32).reshape(-1, 4)
    anchors = np.asarray(model.anchors, np.int64).reshape(-1, 2)
    biasw = np.asarray(model.biasw, np.float32)
    cache = {}
    for i in range(n):
        c, l = int(heads["component"][i]), int(heads["level"][i])
        if l not in cache:
            cache[l] = resp_of_level(l)
        resp = cache[l]
        P = model.nparts(c)
        assert int(heads["nparts"][i]) == P
        for p in range(P):
            x, y, m = (int(v) for v in locs[i, p])
            out[i, p, 0] = F64(resp[model.filterid[c][p][m], y, x])
            if p == 0:
                out[i, p, 2] = F64(biasw[model.biasid[c][0][0]])
                continue
            q = model.parentid[c][p]
            xq, yq, mq = (int(v) for v in locs[i, q])
            did = model.defid[c][p][m]
            ax, bx, ay, by = (F64(-w) for w in defw[did])      # negated as float, then widened
            dx = xq + int(anchors[did, 0]) - x
            dy = yq + int(anchors[did, 1]) - y
            out[i, p, 1] = (ax * F64(dx * dx) + bx * F64(dx)) + (ay * F64(dy * dy) + by * F64(dy))
            out[i, p, 2] = F64(biasw[model.biasid[c][p][m] + mq])
    return out


def totals(ps):
    """total per candidate: score_p = (app + def) + bias, summed in part order, in double"""
    t = np.zeros(len(ps), F64)
    for p in range(ps.shape[1]):
        t = t + ((ps[:, p, 0] + ps[:, p, 1]) + ps[:, p, 2])
    return t


def bound(ps, nparts, dtype):
    """B = 4 P eps_T S per candidate"""
    eps = 2.0 ** -53 if np.dtype(dtype) == np.dtype(np.float64) else 2.0 ** -24
    S = np.abs(ps).sum(axis=(1, 2))
    return 4.0 * np.asarray(nparts, F64) * eps * S
