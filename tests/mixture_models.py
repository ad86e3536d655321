"""Test helper: models whose parts have different mixture counts (src/DynamicProgram.cpp:99-100: nmixtures of the part,
pnmixtures of its parent, an L x K bias block per child), the cases the DP kernels handle with clamped, unpredicated copies."""
import numpy as np

from partsbaseddetector_amd.model import Model, make_tree_model_k

# name: (parents, mixture count per part)
HET = {
    "root1_children_many": ([-1, 0, 0, 1, 2], [1, 3, 2, 4, 2]),          # K0 = 1 at the root, K > 1 below
    "L6_child_K1": ([-1, 0, 1, 1, 2], [2, 6, 1, 3, 6]),                  # parent L = 6, a K = 1 child (the copy shortcut, L > 1)
    "L1_child_K8": ([-1, 0, 1, 1], [3, 1, 8, 2]),                        # L = 1 over K = 8
    "siblings_1_to_8": ([-1, 0, 0, 0, 0, 0, 0, 0, 0], [2, 1, 2, 3, 4, 5, 6, 7, 8]),
    "foldmix3": ([-1, 0, 1, 1, 0], [2, 3, 1, 2, 3]),                     # fold_mix 3: the 4-wide fold, one replicated slot
    "foldmix5": ([-1, 0, 0, 1, 2, 2], [5, 2, 4, 1, 3, 5]),               # 6-wide fold
    "foldmix7": ([-1, 0, 1, 2, 1, 0], [3, 7, 2, 5, 1, 7]),               # 8-wide fold
    "k10_among_small": ([-1, 0, 1, 0, 3], [2, 3, 10, 1, 4]),             # K > 8: the three-kernel structure
}


def het_model(name, seed=None, **kw):
    parents, Ks = HET[name]
    return make_tree_model_k(parents, Ks, seed=seed if seed is not None else 100 + sorted(HET).index(name), name=name, **kw)


def stack_components(*models) -> Model:
    """One model whose components are those of `models` (uniform filter size), filters / deformations / biases renumbered."""
    m0 = models[0]
    filt, defw, anchors, biasw = [], [], [], []
    filterid, defid, biasid, parentid = [], [], [], []
    for m in models:
        f0, d0, b0 = len(filt), len(defw), len(biasw)
        filt += list(m.filtersw); defw += list(np.asarray(m.defw).reshape(-1, 4)); anchors += list(np.asarray(m.anchors).reshape(-1, 2))
        biasw += [float(x) for x in m.biasw]
        for c in range(m.ncomponents):
            filterid.append([[f0 + i for i in ids] for ids in m.filterid[c]])
            defid.append([[d0 + i for i in ids] for ids in m.defid[c]])
            biasid.append([[b0 + i for i in ids] for ids in m.biasid[c]])
            parentid.append(list(m.parentid[c]))
    return Model(filt, np.asarray(biasw, np.float32), np.asarray(anchors, np.int32), np.asarray(defw, np.float32), filterid, biasid,
                 defid, parentid, m0.interval, m0.thresh, m0.sbin, m0.norient, m0.flen, "+".join(m.name for m in models))


def two_profiles(seed=7, **kw):
    """Two components with different count profiles: 1 / 4 / 2 / 6 and 5 / 1 / 3 / 3 / 2."""
    return stack_components(make_tree_model_k([-1, 0, 1, 1], [1, 4, 2, 6], seed=seed, **kw),
                            make_tree_model_k([-1, 0, 0, 1, 2], [5, 1, 3, 3, 2], seed=seed + 1, **kw))


def level_responses(rng, model, H, W, dtype, kind="normal"):
    """[nfilters, H, W] injected responses: 'normal' N(0, 1); 'quant' independent multiples of 1/4 in [-1, 1] (exact sums, many
    partial ties); 'tied' one quantised plane per part shared by all its mixtures (with a `shared` model: every reduce ties)."""
    nf = len(model.filtersw)
    if kind == "normal":
        return rng.normal(0, 1, (nf, H, W)).astype(dtype)
    if kind == "quant":
        return (rng.integers(-4, 5, (nf, H, W)) * 0.25).astype(dtype)
    out = np.zeros((nf, H, W), dtype)
    for c in range(model.ncomponents):
        for ids in model.filterid[c]:
            out[ids] = rng.integers(-4, 5, (H, W)) * 0.25
    return out
