"""K10w (ops/csrc/gbt_hist_wide.hip): the dense level histogram for levels of
more than 8192 cells, against a float64 index_add_ reference with the bound
of tests/gbt_hist_cases.py (counts exact, a sum within (n + 1) * 2^-24 *
sum |r_i| of its cell), and through build_tree at depth 9."""

import pytest
import torch

from tests import gbt_hist_cases as gc

pytestmark = pytest.mark.gpu

# (B, F, nb, n_nodes); G = 8192 // nb nodes per pass, 1024 sorted rows per
# slice, ceil(F / min(F, 512 // slices)) features per workgroup
SHAPES = [
    (300, 3, 64, 129),       # one node past K10: passes of 128 + 1 nodes
    (2500, 5, 256, 33),      # G = 32, three slices, nodes across slice ends
    (1100, 70, 16, 1024),    # about one row per node: direct passes
    (1500, 130, 64, 200),    # skew: span = 1 next to scattered rows
    (16384, 130, 64, 500),   # 5 features per workgroup in chunks of 4 + 1
]
VARIANTS = ["random", "skew", "far_apart", "one_cell"]
# the last shape is there for its chunks only
PARAMS = [(i, v) for i in range(4) for v in VARIANTS] + [(4, "random")]


def make_case(idx, variant):
    B, F, nb, n_nodes = SHAPES[idx]
    g = torch.Generator().manual_seed(100 * idx + VARIANTS.index(variant))
    bins = torch.randint(0, nb, (B, F), generator=g)
    node = torch.randint(0, n_nodes, (B,), generator=g)
    resid = torch.randn(B, generator=g)
    if variant == "skew":           # 90 % of the rows in node 0
        node[torch.rand(B, generator=g) < 0.9] = 0
    elif variant == "far_apart":    # every row in the first or the last node
        node = torch.where(node % 2 == 0, 0, n_nodes - 1)
    elif variant == "one_cell":     # every row in the last node and bin
        bins.fill_(nb - 1)
        node.fill_(n_nodes - 1)
    idx64 = ((node.unsqueeze(1) * F + torch.arange(F)) * nb + bins).reshape(-1)
    r64 = resid.double().unsqueeze(1).expand(B, F).reshape(-1)
    ref = [torch.zeros(n_nodes * F * nb, dtype=torch.float64)
           .index_add_(0, idx64, v).view(n_nodes, F, nb)
           for v in (torch.ones_like(r64), r64, r64.abs())]
    return dict(bins=bins.int(), resid=resid, node=node.int(),
                cnt=ref[0], sum=ref[1], abs=ref[2])


@pytest.mark.parametrize("idx,variant", PARAMS)
def test_binding_vs_fp64(idx, variant):
    from harmony_amd import ops

    B, F, nb, n_nodes = SHAPES[idx]
    assert n_nodes * nb > ops.GBT_HIST_MAX_CELLS
    case = make_case(idx, variant)
    host = [case[k] for k in ("bins", "resid", "node")]
    args = [t.cuda() for t in host]
    cnt = torch.zeros(n_nodes, F, nb, device="cuda")
    s = torch.zeros_like(cnt)
    ops._load_hip().gbt_hist(*args, cnt, s)
    for a, b in zip(args, host):                  # inputs are not mutated
        assert torch.equal(a.cpu(), b)
    err, ratio = gc.check(cnt.cpu(), s.cpu(), case, label=(idx, variant))
    assert float(cnt.sum()) == B * F
    print(f"gbt_hist wide {SHAPES[idx]} {variant}: sum error {err:.3g}, "
          f"error / bound {ratio:.3f}, counts exact")


def test_tree_of_depth_9(monkeypatch):
    from harmony_amd import ops
    from harmony_amd.mlapps.gbt import build_tree

    g = torch.Generator().manual_seed(9)
    bins = torch.randint(0, 64, (2000, 6), generator=g).cuda()
    # integers: every float32 sum is exact in any order
    resid = torch.randint(-8, 9, (2000,), generator=g).float().cuda()
    hip, calls = ops._load_hip(), []
    real = hip.gbt_hist
    monkeypatch.setattr(hip, "gbt_hist",
                        lambda *a: calls.append(a[3].shape[0]) or real(*a))
    tree = build_tree(bins, resid, 64, 9, 1.0)
    assert calls == [2 ** level for level in range(9)]
    monkeypatch.setenv("HARMONY_FORCE_TORCH_OPS", "1")
    ref = build_tree(bins, resid, 64, 9, 1.0)
    assert len(calls) == 9
    assert tree.feature == ref.feature and tree.threshold == ref.threshold
    assert tree.leaf_value == ref.leaf_value
    assert tree.cat_mask is None and ref.cat_mask is None
