"""Host logic of the micro-batched joint step: the chunk boundaries and the drivers' `--micro-batch` flag."""
import pytest

from incremental_multimodal_medical_learning_ii_amd import contrastive as C
from incremental_multimodal_medical_learning_ii_amd import drivers


@pytest.mark.parametrize("n, m, want", [
    (8, 3, ((0, 3), (3, 6), (6, 8))),
    (8, 8, ((0, 8),)),
    (8, 100, ((0, 8),)),
    (1, 1, ((0, 1),)),
    (5, 2, ((0, 2), (2, 4), (4, 5))),
])
def test_micro_slices(n, m, want):
    got = C.micro_slices(n, m)
    assert got == want and isinstance(got, tuple)
    assert got[0][0] == 0 and got[-1][1] == n and all(a[1] == b[0] for a, b in zip(got, got[1:]))     # contiguous, covering
    assert all(0 < hi - lo <= m for lo, hi in got)


@pytest.mark.parametrize("bad", [0, -1, True, 2.5])
def test_micro_slices_refuses(bad):
    with pytest.raises(ValueError, match="micro_batch"):
        C.micro_slices(8, bad)


def test_drivers_flag():
    ap = drivers.make_parser()
    assert ap.parse_args(["zero-joint", "--joint"]).micro_batch is None
    assert ap.parse_args(["zero-joint", "--joint", "--micro-batch", "1024"]).micro_batch == 1024
    with pytest.raises(SystemExit, match="--joint"):                  # rejected the way the other joint-only flags are
        drivers.main(["zero-joint", "--micro-batch", "4"])
    with pytest.raises(SystemExit, match="--micro-batch"):
        drivers.main(["zero-joint", "--joint", "--micro-batch", "0"])
