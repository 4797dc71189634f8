"""Inputs, float64 reference and checker for K10 (ops/csrc/gbt.hip, the dense
level histogram behind ops.gbt_hist).

Reference: float64 index_add_ on the CPU. Counts are integers below 2^24 and
must be exact. A cell's residual sum is a float32 sum of its n residuals in
an order that LDS and global atomics decide, so it may be off by
(n + 1) * 2^-24 * sum |r_i| over the cell's own terms, which holds for any
summation order (Higham, Accuracy and Stability of Numerical Algorithms,
eq. 4.4, with gamma_n rounded up by the + 1). At n <= 1000 here that is
6e-5 of the cell's absolute sum, so one dropped or doubled residual of
average size is 16 times past it (test_gbt_hist_cpu.py).
"""

import functools

import torch

# (B, F, nb, n_nodes) with fc = min(F, 8192 // (n_nodes * nb)) features per
# workgroup and tile = max(ceil(B / (512 // chunks)), 256) rows
SHAPES = [
    (1, 1, 1, 1),         # one of everything
    (255, 3, 7, 1),       # one row short of a tile, odd bin count
    (257, 5, 64, 128),    # fc = 1, 8192 cells, two tiles
    (1000, 7, 64, 32),    # fc = 4: chunks of 4 and 3 features
    (300, 2, 8192, 1),    # n_nodes * nb at the cap with one node
    (513, 9, 16, 3),      # odd everything, three tiles
]
VARIANTS = ["random", "one_cell", "empty_node", "wide"]
U = 2.0 ** -24


def params():
    """(shape index, variant) for every pair that exists."""
    return [(i, v) for i, s in enumerate(SHAPES) for v in VARIANTS
            if not (v == "empty_node" and s[3] < 2)]


@functools.lru_cache(maxsize=None)
def make_case(idx, variant):
    B, F, nb, n_nodes = SHAPES[idx]
    g = torch.Generator().manual_seed(100 * idx + VARIANTS.index(variant))
    bins = torch.randint(0, nb, (B, F), generator=g)
    node = torch.randint(0, n_nodes, (B,), generator=g)
    resid = torch.randn(B, generator=g)
    if variant == "one_cell":       # every row in the last node and bin
        bins.fill_(nb - 1)
        node.fill_(n_nodes - 1)
    elif variant == "empty_node":   # node 1 holds no rows
        node[node == 1] = 0
    elif variant == "wide":         # mixed sign over six orders of magnitude
        resid = resid * 10.0 ** (torch.rand(B, generator=g) * 6 - 3)
    idx64 = ((node.unsqueeze(1) * F + torch.arange(F)) * nb + bins).reshape(-1)
    r64 = resid.double().unsqueeze(1).expand(B, F).reshape(-1)
    cells = n_nodes * F * nb
    cnt = torch.zeros(cells, dtype=torch.float64).index_add_(
        0, idx64, torch.ones_like(r64))
    s = torch.zeros(cells, dtype=torch.float64).index_add_(0, idx64, r64)
    a = torch.zeros(cells, dtype=torch.float64).index_add_(0, idx64,
                                                           r64.abs())
    shape = (n_nodes, F, nb)
    return dict(bins=bins, resid=resid, node=node, n_nodes=n_nodes, nb=nb,
                cnt=cnt.view(shape), sum=s.view(shape), abs=a.view(shape))


def check(cnt, s, case, ref_sum=None, label=""):
    """Counts exact, sums within the bound of the module docstring; returns
    (largest error, largest error / bound). ref_sum replaces the reference
    sums (for the tests of this checker)."""
    ref = case["sum"] if ref_sum is None else ref_sum
    assert cnt.shape == ref.shape and s.shape == ref.shape, label
    assert torch.equal(cnt.double(), case["cnt"]), (label, "counts")
    bound = (case["cnt"] + 1) * U * case["abs"]
    err = (s.double() - ref).abs()
    assert bool((err <= bound).all()), (label, float((err - bound).max()))
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    return float(err.max()), ratio
