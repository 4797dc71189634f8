"""The lasso_cd binding past K11's LDS limit, with CPU tensors only: batches
up to LASSO_CD_MAX_ROWS pass every metadata check and stop at the device
check; one row more is refused by name."""

import pytest
import torch

from harmony_amd import ops

pytestmark = pytest.mark.skipif(not ops.hip_available(),
                                reason="HIP extension not built")


def _call(B):
    z = torch.zeros
    ops._load_hip().lasso_cd(z(1, B), z(B), z(1), z(1), 0.1)


@pytest.mark.parametrize("B", [16368, 65536])
def test_large_batch_reaches_the_device_check(B):
    with pytest.raises(RuntimeError, match="lasso_cd: every tensor must be "
                       "on device"):
        _call(B)


def test_one_row_past_the_cap_is_refused():
    with pytest.raises(RuntimeError) as e:
        _call(65537)
    msg = str(e.value).split("\n")[0]
    assert msg.startswith("lasso_cd: ") and "too large" in msg, msg
    assert "65536" in msg and "on device" not in msg, msg


def test_max_rows_constant():
    assert ops._load_hip().lasso_cd_max_rows() == ops.LASSO_CD_MAX_ROWS == 65536
