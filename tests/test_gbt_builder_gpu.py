"""build_tree on the GPU (K10, K10s, K10b and the tensor-op search) against
the trees recorded in tests/golden/gbt/builder_parent.json on the CPU. The
cases' residuals are integers, so every fp32 sum is exact in any order and a
leaf value is one IEEE division on both sides."""

import pytest
import torch

from tests import gbt_builder_cases as bc

pytestmark = pytest.mark.gpu

GOLD = bc.load()


@pytest.mark.parametrize("kind", bc.KINDS)
@pytest.mark.parametrize("idx", range(bc.N_TREE_CASES))
def test_device_tree_against_the_recorded_tree(idx, kind):
    case = bc.tree_case(idx)
    want = GOLD["trees"][bc.tree_name(idx, kind)]
    tree, bins = bc.build(case, kind, "cuda")
    assert bins.device.type == "cuda"
    golden = bc.tree_from_lists(want["depth"], want)
    # every row ends in the leaf the recorded tree sends it to
    assert torch.equal(bc.leaf_of(tree, bins),
                       bc.leaf_of(golden, case["inputs"][kind]))
    assert tree.leaf_value == want["leaf_value"]
    assert (tree.cat_mask is None) == kind.endswith("_untyped")
    if kind in bc.K10B_KINDS:
        got = bc.tree_lists(tree)
        for name in ("feature", "threshold", "cat_mask"):
            assert got[name] == want[name], (idx, kind, name)
