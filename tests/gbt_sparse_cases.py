"""Shared cases for the sparse GBT tests (SparseBins, K10s, tree equality):
a case builder and the fp64 histogram checker. Cases are built once per
process and never modified."""

from pathlib import Path

import torch

from harmony_amd.mlapps import gbt
from harmony_amd.mlapps.sparse_bins import SparseBins

GOLDEN = Path(__file__).parent / "golden" / "gbt" / "sample_gbt_sparse_48"
GOLDEN_F = 3000          # small enough for the dense job over the fixture

# (B, F, nb, density, n_nodes, specials). With fc = 8192 // (n_nodes * nb)
# present features per workgroup:
SHAPES = [
    # fc = 16, nf = 70 (not a multiple of fc); the special columns, one of
    # them full, a categorical column and a node with no samples
    (300, 70, 64, 0.10, 8, "full"),
    # nb = 2 (scalar stores), fc = 2048 > nf
    (200, 40, 2, 0.20, 2, False),
    # n_nodes * nb exactly 8192: fc = 1
    (128, 50, 64, 0.15, 128, False),
    # 8192 + nb: too wide for the kernel, the torch path
    (128, 50, 64, 0.15, 129, False),
    # one column of B entries among one-entry columns, fc = 128
    (700, 3000, 16, 0.0, 4, "long"),
    # B = 1
    (1, 20, 8, 0.5, 1, False),
    # nb = 32, fc = 16, the specials with a row with no entries instead of
    # the full column
    (257, 300, 32, 0.05, 16, "emptyrow"),
    # nb = 12: not a multiple of 4 (scalar stores) over many workgroups,
    # fc = 10, and a node count that is no power of two
    (150, 90, 12, 0.10, 64, False),
]

_CACHE = {}


def _csr_from_dense_mask(X, mask):
    """CSR of the entries of X where mask is set (explicit zeros stay)."""
    B = X.shape[0]
    row_ptr = torch.zeros(B + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(mask.sum(dim=1), 0)
    rows, cols = mask.nonzero(as_tuple=True)
    return row_ptr, cols.to(torch.int32), X[rows, cols].float()


def make_case(idx):
    if idx in _CACHE:
        return _CACHE[idx]
    B, F, nb, dens, n_nodes, special = SHAPES[idx]
    g = torch.Generator().manual_seed(1000 + idx)
    X = torch.randn(B, F, generator=g)
    # ties: a third of the columns hold values rounded to quarters
    X[:, ::3] = (X[:, ::3] * 4).round() / 4
    mask = torch.rand(B, F, generator=g) < dens
    types = torch.zeros(F, dtype=torch.int32)
    if special == "long":
        # column 7 in every row, every other column at most one entry
        mask[:] = False
        mask[:, 7] = True
        cols = torch.randperm(F, generator=g)[:B]
        mask[torch.arange(B), cols] = True
    elif special:
        if special == "full":
            mask[:, 0] = True                  # a full column
        # a column whose entries all fall into its own zero bin: explicit
        # 0.0 values and a few small negatives among implied zeros
        mask[:, 1] = False
        mask[:6, 1] = True
        X[:6, 1] = torch.tensor([0.0, 0.0, -1e-3, 0.0, -2e-3, 0.0])
        mask[:, 2] = False                     # a one-entry column
        mask[B // 2, 2] = True
        if special == "emptyrow":
            mask[5, :] = False                 # a row with no entries
        types[F - 1] = 6                       # a categorical column
        X[:, F - 1] = torch.randint(0, 6, (B,), generator=g).float()
        mask[:, F - 1] = torch.rand(B, generator=g) < 0.6
        mask[5, F - 1] = special == "full"
    X = X * mask
    row_ptr, col, val = _csr_from_dense_mask(X, mask)
    # file order inside a row is not sorted: reverse every second row
    for i in range(0, B, 2):
        lo, hi = int(row_ptr[i]), int(row_ptr[i + 1])
        col[lo:hi] = col[lo:hi].flip(0)
        val[lo:hi] = val[lo:hi].flip(0)
    ft = types if bool((types != 0).any()) else None
    sb = SparseBins((row_ptr, col, val, F), nb, ft)
    node = torch.randint(0, n_nodes, (B,), generator=g)
    if special in ("full", "emptyrow"):
        node[node == 3] = 2                    # a node with no samples
    resid = torch.randn(B, generator=g) * 3
    case = dict(B=B, F=F, nb=nb, n_nodes=n_nodes, X=X, mask=mask,
                csr=(row_ptr, col, val), types=ft, sb=sb, node=node,
                resid=resid, dense_bins=gbt.quantize(X, nb, ft))
    _CACHE[idx] = case
    return case


def hist_args(case, device="cpu"):
    sb = case["sb"].to(device)
    return (sb.feat_ptr, sb.feat_row, sb.feat_bin, sb.feat_idx, sb.zero_bin,
            case["resid"].to(device), case["node"].to(device),
            case["n_nodes"], case["nb"])


def check_hist(case, cnt, s, what=""):
    """cnt, s [n_nodes, nf, nb] against fp64 histograms of the dense bins
    over the present features. Counts exact; sums within
    (2 n + nb + 2) * 2^-23 * A per cell, n the node's sample count and A its
    sum of |resid| (u = 2^-24 per addition for two n-term sums and the
    nb-term fix-up, doubled). Returns the largest error / bound."""
    n_nodes, nb = case["n_nodes"], case["nb"]
    ids = case["sb"].feat_ids.long()
    nf = ids.shape[0]
    assert cnt.shape == s.shape == (n_nodes, nf, nb), (what, cnt.shape)
    assert cnt.dtype == s.dtype == torch.float32
    bins = case["dense_bins"][:, ids]                        # [B, nf]
    node = case["node"]
    # resid as the fp32 values the op sees
    r64 = case["resid"].float().double()
    cell = (node.unsqueeze(1) * nf + torch.arange(nf)) * nb + bins
    c64 = torch.zeros(n_nodes * nf * nb, dtype=torch.float64)
    s64 = torch.zeros_like(c64)
    c64.scatter_add_(0, cell.reshape(-1), torch.ones(cell.numel(),
                                                     dtype=torch.float64))
    s64.scatter_add_(0, cell.reshape(-1),
                     r64.unsqueeze(1).expand(-1, nf).reshape(-1))
    c64 = c64.view(n_nodes, nf, nb)
    s64 = s64.view(n_nodes, nf, nb)
    cnt, s = cnt.cpu().double(), s.cpu().double()
    assert torch.equal(cnt, c64), f"{what}: counts differ"
    n = torch.zeros(n_nodes, dtype=torch.float64).scatter_add_(
        0, node, torch.ones_like(r64))
    A = torch.zeros(n_nodes, dtype=torch.float64).scatter_add_(
        0, node, r64.abs())
    bound = ((2 * n + nb + 2) * 2.0 ** -23 * A).view(-1, 1, 1)
    err = (s - s64).abs()
    assert bool((err <= bound).all()), \
        f"{what}: sum error {float(err.max()):.3e} over its bound"
    live = bound.expand_as(err) > 0
    return float((err[live] / bound.expand_as(err)[live]).max()) \
        if bool(live.any()) else 0.0


# ------------------------------------------------------------ tree equality

# (B, F, density, seed)
TREE_SHAPES = [(40, 64, 0.15, 1), (150, 300, 0.05, 2), (400, 1024, 0.01, 3),
               (700, 4096, 0.004, 4)]
TREE_NB = 16
TREE_DEPTH = 4
TREE_LAM = 1.0


def make_tree_case(idx):
    key = ("tree", idx)
    if key in _CACHE:
        return _CACHE[key]
    B, F, dens, seed = TREE_SHAPES[idx]
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, F, generator=g)
    mask = torch.rand(B, F, generator=g) < dens
    # three signal columns present in half of the rows and a categorical
    # column present in most, so the tree has something to split on
    sig = [3, F // 2, F - 5]
    for f in sig:
        mask[:, f] = torch.rand(B, generator=g) < 0.5
    cat = F - 2
    types = torch.zeros(F, dtype=torch.int32)
    types[cat] = 5
    X[:, cat] = torch.randint(0, 5, (B,), generator=g).float()
    mask[:, cat] = torch.rand(B, generator=g) < 0.8
    X = X * mask
    # integer-valued residuals: every fp32 sum is exact
    resid = ((3 * X[:, sig[0]]).round() + 4 * (X[:, sig[1]] > 0.3).float()
             - 3 * (X[:, sig[2]] < -0.2).float()
             + 5 * (X[:, cat].long() % 2 == 1).float()
             + torch.randint(-1, 2, (B,), generator=g).float())
    row_ptr, col, val = _csr_from_dense_mask(X, mask)
    case = dict(B=B, F=F, X=X, types=types, resid=resid,
                sb=SparseBins((row_ptr, col, val, F), TREE_NB, types),
                dense_bins=gbt.quantize(X, TREE_NB, types))
    _CACHE[key] = case
    return case


def assert_same_tree(a, b, what=""):
    assert a.depth == b.depth, what
    assert a.feature == b.feature, what
    assert a.threshold == b.threshold, what
    assert a.cat_mask == b.cat_mask, what
    assert a.leaf_value == b.leaf_value, what


def n_splits(tree):
    return sum(1 for t in tree.threshold if t != -1)
