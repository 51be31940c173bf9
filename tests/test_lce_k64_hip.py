"""GPU parity of the fused all-item logits + cross-entropy kernels at contraction width 64 (adt_amd/csrc/adt_lce.cuh: k_lce<64, *>,
k_lce_combine<64>, k_lce_reduce<64>) against the oracle's tape, through tests/test_lce_hip.py:run_case and its bounds: loss and
log-sum-exp 2e-3 absolute, dh / dE / dbias 2e-2 of the tensor magnitude, rows that are not masked bit-equal.

At this width a 32-row tile is four 1-KiB LDS-DMA pieces for eight waves: waves 0-3 fetch a piece each, every wave fetches its copy of
the row constants, and each wave waits on the count IT issued.  The shapes are the smallest at which the tile ring, the range split and
the partial folds can go wrong."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from tests.test_lce_hip import dev, run_case  # noqa: E402


def test_lce_supported_at_width_64():
    from adt_amd import _lib, ops
    lib = _lib.load()
    assert lib.adt_lce_supported(ops.PREC_BF16, 64) == 1 and lib.adt_lce_supported(ops.PREC_F32, 64) == 0


@pytest.mark.parametrize("T,K,V,M,mcap,slots", [
    (64, 64, 100, 1, 64, 0),               # one row
    (300, 64, 1000, 37, 300, 0),           # ragged sizes; V not a multiple of 32
    (700, 64, 2077, 600, 700, 0),          # two forward X blocks
    (1400, 64, 3416, 1111, 1400, 8),       # 8 workgroups: every one walks several (X block, Y range) items
    (513, 64, 300, 300, 513, 0),           # live count below the capacity
])
def test_lce_k64_against_oracle(T, K, V, M, mcap, slots):
    run_case(T, K, V, M, mcap, seed=T + V + M, slots=slots)


def test_lce_k64_repeated_labels():
    run_case(400, 64, 260, 333, 400, seed=5, few_labels=True)        # many rows share a label: the rank-one label terms collide


def test_lce_k64_large_logits():
    run_case(400, 64, 700, 200, 400, seed=6, scale=3.0)              # the running maximum matters


def test_lce_k64_zero_rows_is_a_no_op():
    from adt_amd import ops
    T, K, V = 64, 64, 500
    h, E, b = torch.randn(T, K, device=dev()), torch.randn(V, K, device=dev()), torch.zeros(V, device=dev())
    dh, dE, db = torch.zeros(T, K, device=dev()), torch.zeros(V, K, device=dev()), torch.zeros(V, device=dev())
    loss64 = torch.zeros(64, device=dev())
    z = torch.zeros(T, device=dev(), dtype=torch.int32)
    ops.lce_fwd_bwd(h, z, z, T, torch.tensor([0], device=dev(), dtype=torch.int32), E, b, torch.tensor([1.0], device=dev()), loss64, dh, dE, db)
    torch.cuda.synchronize()
    assert float(loss64.abs().sum()) == 0 and float(dh.abs().sum()) == 0 and float(dE.abs().sum()) == 0 and float(db.abs().sum()) == 0
