"""Pregel push kernel (K13p), the engine's direction choice and the
connected-components app on the GPU."""

import pytest

from tests import pregel_push_cases as ppc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("use_w,add_weight,inf_msgs", ppc.PUSH_CONFIGS)
@pytest.mark.parametrize("frontier", ppc.FRONTIERS)
def test_kernel_against_pull_and_brute_force(frontier, use_w, add_weight,
                                             inf_msgs):
    ppc.check_kernel_case("cuda", frontier, use_w, add_weight, inf_msgs)


def test_kernel_skips_malformed_ids_and_rows():
    ppc.check_malformed("cuda")


def test_kernel_add_raises_and_empty_shapes():
    ppc.check_add_raises_and_empty_shapes("cuda")


def test_engine_push_sssp_fixture():
    ppc.check_engine_sssp_fixture("cuda", "gpu")


def test_engine_directions_agree_on_synthetic():
    ppc.check_engine_synthetic("cuda", "gpu")


def test_engine_push_star():
    ppc.check_engine_star("cuda", "gpu")


def test_engine_refusals():
    ppc.check_engine_refusals("cuda", "gpu")


def test_connected_components_fixture(tmp_path):
    ppc.check_cc_fixture("cuda", tmp_path, "gpu")
