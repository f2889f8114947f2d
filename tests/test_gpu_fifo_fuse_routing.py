"""Every depth of a fused FIFO launch through the one entry that routes it (fw_launch_update_fifo, csrc/fw_k_rings.hip: depths 2 to
FW_FUSE_MAX to fw_k_rings_fuse2.hip -- and from there, under FW_NEWBORN_SPIN=1, to fw_k_rings_fuse2_eager.hip --, depths 9 to FW_FUSE_FAR
to fw_k_rings_far.hip).  The small ring of tests/test_gpu_fifo_fuse_far.py, whose own assertion shows that it holds sixteen
frames of spawns: 380 new particles per frame in 16384 slots, sixteen ring tiles.  Every threshold of the depth ladder is 1 and the knobs
make groups close at exactly `depth`: FW_FUSE_DEPTH=depth with the far tier off up to eight, FW_FUSE_DEPTH=8 and FW_FUSE_FAR_DEPTH=depth
beyond.  2 x depth + 1 unread frames and a read: the call-by-call log must show two fused launches of that depth and one kept frame, and
every read, the counts and updated_total agree with the run under FW_FUSE2=0 and with the CPU oracle (both, tests/test_gpu_fifo_fuse2.py).
Needs an MI355X."""
import pytest

import oracle  # noqa: F401
from test_gpu_fifo_fuse2 import X, both
from test_gpu_fifo_fuse_deep import _groups, _start, _tail
from test_gpu_fifo_fuse_far import CAPACITY, PER_FRAME, _ring

pytestmark = pytest.mark.gpu
EVERY_RUNG = {"FW_FUSE_DEEP_MIN": "1", "FW_FUSE_WIDE_MIN": "1", "FW_FUSE_FAR_MIN": "1"}  # (FW_FUSE2_MIN=1: both's own)
assert (24 + 16) * (PER_FRAME + 1) <= CAPACITY


@pytest.fixture(autouse=True)
def fifo_entry_only(fw_path):
    """(tests/conftest.py deals every GPU test out over four update paths; these set their own knobs and run once, under its FIFO entry)"""
    if fw_path != "fifo":
        pytest.skip("the fused launch belongs to the FIFO ring kernel: one run, under the path matrix's fifo entry")


def _closes_at(depth):
    if depth <= 8:
        return dict(EVERY_RUNG, FW_FUSE_DEPTH=str(depth), FW_FUSE_FAR_DEPTH="8")
    return dict(EVERY_RUNG, FW_FUSE_DEPTH="8", FW_FUSE_FAR_DEPTH=str(depth))


def _two_groups_and_a_kept_frame(monkeypatch, depth, **knobs):
    def scenario(run):
        _start(run)
        run.step(n=2 * depth + 1)
        if run.rule:
            assert _tail(run, 2 * depth + 1) == _groups(depth, 2 * depth + 1), _tail(run, 2 * depth + 1)
            assert sorted(f for f in run.frames if f) == [depth, depth], run.frames
        run.did(run.read, "end")
        if run.rule:
            assert _tail(run, 1) == [X + (0,)], _tail(run, 3)
        run.totals("end")

    both(monkeypatch, _ring(), scenario, **knobs, **_closes_at(depth))


@pytest.mark.parametrize("depth", range(2, 17))
def test_every_depth_reaches_its_kernels(monkeypatch, depth):
    _two_groups_and_a_kept_frame(monkeypatch, depth)


@pytest.mark.parametrize("depth", range(2, 9))
def test_every_depth_of_the_first_tier_reaches_the_eager_kernels(monkeypatch, depth):
    _two_groups_and_a_kept_frame(monkeypatch, depth, FW_NEWBORN_SPIN="1")
