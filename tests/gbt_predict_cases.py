"""Shared inputs for the forest-prediction tests (test_gbt_predict_cpu.py,
test_gbt_predict_gpu.py): random forests built directly, not by training, and
the oracle, GBTTrainer._forest_pred from an empty cache on the CPU.

Per node: a feature in 0..F-1, a threshold from {-2, -1, 0..nb-1}, a random
64-bit mask (some with bit 0 and bit 63 set, some all ones); leaf values of
mixed sign and magnitude 1e-3..1e3, so that the order of the sum shows. The
comparison is torch.equal: nothing here is a tolerance.
"""

import functools

import torch

from harmony_amd import ops
from harmony_amd.mlapps import gbt
from harmony_amd.mlapps.sparse_bins import SparseBins

STEP = 0.3          # not exact in binary, so fp32(step) * leaf rounds
WIDE_F = 2 ** 20

# dense: (B, F, T, d, typed, nb); T None = one more than an LDS group
DENSE = [
    (1, 1, 1, 1, True, 16),
    (63, 5, 3, 3, True, 16),
    (65, 33, 17, 4, False, 16),
    (257, 8, 40, 4, True, 128),      # categorical nodes meet bins >= 64
    (300, 16, 2, 8, True, 16),       # the deepest supported
    (100, 4, 0, 4, True, 16),        # the empty forest gives zeros
    (129, 8, None, 4, True, 16),
]
# sparse: (B, F, most entries per row, T, d, typed, nb)
SPARSE = [
    (130, WIDE_F, 8, 9, 4, True, 16),
    (4100, WIDE_F, 4, 5, 3, True, 16),     # row * F passes 2^32
]
SMALL_SPARSE = (40, 12, 5, 6, 3, True, 16)   # small F: also densified
N_CASES = len(DENSE) + len(SPARSE)


def row_len(depth, typed):
    ni = (1 << depth) - 1
    return 1 + 2 * ni + (1 << depth) + (2 * ni if typed else 0)


def random_forest(T, depth, F, nb, typed, g, features=None):
    """T random GBTrees; `features` restricts the node features to a list."""
    ni = (1 << depth) - 1
    special = torch.tensor([-1, 1, -(2 ** 63), 2 ** 63 - 1,
                            -(2 ** 63) + 1], dtype=torch.int64)
    forest = []
    for _ in range(T):
        if features is None:
            feat = torch.randint(0, F, (ni,), generator=g)
        else:
            pool = torch.tensor(features, dtype=torch.int64)
            feat = pool[torch.randint(0, len(features), (ni,), generator=g)]
        # a quarter of the nodes categorical (typed only), a quarter
        # pass-through, the rest thresholds anywhere in 0..nb-1
        kind = torch.randint(0 if typed else 1, 4, (ni,), generator=g)
        thr = torch.randint(0, nb, (ni,), generator=g)
        thr = torch.where(kind == 0, torch.full_like(thr, -2),
                          torch.where(kind == 1, torch.full_like(thr, -1),
                                      thr))
        # 64 random bits from two 32-bit halves, the high one signed
        mask = (torch.randint(-(2 ** 31), 2 ** 31, (ni,), generator=g)
                * 2 ** 32 + torch.randint(0, 2 ** 32, (ni,), generator=g))
        pick = torch.randint(0, 2 * len(special), (ni,), generator=g)
        mask = torch.where(pick < len(special),
                           special[pick.clamp(max=len(special) - 1)], mask)
        mag = 10.0 ** (torch.rand(1 << depth, generator=g) * 6 - 3)
        sign = torch.randint(0, 2, (1 << depth,), generator=g) * 2 - 1
        forest.append(gbt.GBTree(
            depth=depth, feature=feat.tolist(), threshold=thr.tolist(),
            leaf_value=(mag * sign).float().tolist(),
            cat_mask=mask.tolist() if typed else None))
    return forest


def oracle(forest, bins, step=STEP):
    """_forest_pred from an empty cache, on the CPU."""
    like = torch.zeros(bins.shape[0], dtype=torch.float32)
    return gbt.GBTTrainer._forest_pred({}, "k", forest, bins, like, step)


def _sparse_bins(B, F, kmax, nb, typed, g):
    """Rows of 0..kmax entries; feature 7 is present in every row that has
    entries, the last two features are categorical."""
    lengths = torch.randint(0, kmax + 1, (B,), generator=g)
    lengths[0] = 0                         # an empty row for certain
    lengths[1] = kmax
    cols, vals, row_ptr = [], [], [0]
    types = torch.zeros(F, dtype=torch.int32)
    if typed:
        types[F - 2:] = 8
    for n in lengths.tolist():
        c = torch.randint(0, F, (n,), generator=g)
        if n:
            c[0] = 7
        if n > 1:
            c[1] = F - 1 - int(torch.randint(0, 2, (1,), generator=g))
        c = torch.unique(c)
        v = torch.randn(c.shape[0], generator=g)
        cat = types[c] != 0
        v = torch.where(cat, torch.randint(0, 8, (c.shape[0],),
                                           generator=g).float(), v)
        cols.append(c)
        vals.append(v)
        row_ptr.append(row_ptr[-1] + c.shape[0])
    return SparseBins((torch.tensor(row_ptr), torch.cat(cols),
                       torch.cat(vals), F), nb,
                      types if typed else None)


@functools.lru_cache(maxsize=None)
def make_case(idx):
    """{"bins", "forest" (GBTrees), "depth", "packed", "want"}; the oracle
    is computed once per case and shared."""
    g = torch.Generator().manual_seed(1000 + idx)
    if idx < len(DENSE):
        B, F, T, d, typed, nb = DENSE[idx]
        if T is None:
            T = ops.gbt_predict_group_trees(row_len(d, typed)) + 1
        bins = torch.randint(0, nb, (B, F), generator=g)
        forest = random_forest(T, d, F, nb, typed, g)
    else:
        B, F, kmax, T, d, typed, nb = SPARSE[idx - len(DENSE)]
        bins = _sparse_bins(B, F, kmax, nb, typed, g)
        # node features: present ones (7 is in every row), the categorical
        # columns, and some that the block does not hold at all
        present = bins.feat_ids.long()
        pool = present[torch.randint(0, present.shape[0], (24,),
                                     generator=g)].tolist()
        absent = [f for f in (3, 11, F - 5) if f not in set(present.tolist())]
        assert absent
        forest = random_forest(T, d, F, nb, typed, g,
                               features=pool + absent + [7, 7, F - 1, F - 2])
    return {"bins": bins, "forest": forest, "depth": d,
            "packed": gbt.pack_forest(forest, d),
            "want": oracle(forest, bins)}


@functools.lru_cache(maxsize=None)
def small_sparse_case():
    B, F, kmax, T, d, typed, nb = SMALL_SPARSE
    g = torch.Generator().manual_seed(77)
    bins = _sparse_bins(B, F, kmax, nb, typed, g)
    forest = random_forest(T, d, F, nb, typed, g)
    return {"bins": bins, "forest": forest, "depth": d,
            "packed": gbt.pack_forest(forest, d),
            "want": oracle(forest, bins)}


def to_device(bins, device):
    return bins.to(device)
