"""No GPU: the GroupNorm hand-off object on its own, and the zero-border refusals of regione_amd/vae.py, which come before any library call."""
import pytest
import torch

from regione_amd import _lib, vae as V


def _img(H=4, W=4, C=64):
    return V.PaddedImage(H, W, C, "cpu")


def test_handoff_set_dropped_kept_consumed():
    lane, a, b = V.GnHandoff(), _img(), _img()
    assert (lane.owner, lane.nblk) == (None, 0) and lane.take(a) == 0
    lane.set(a, 7)                                  # a producer
    lane.wrote(b)                                   # a write to another image keeps it
    assert lane.owner is a and lane.nblk == 7
    lane.wrote(a)                                   # a write to the owner drops it
    assert (lane.owner, lane.nblk) == (None, 0) and lane.take(a) == 0
    lane.set(a, 7)
    assert lane.take(b) == 0                        # another image's norm: nothing for it, and the sums are about to be overwritten
    assert (lane.owner, lane.nblk) == (None, 0)
    lane.set(a, 7)
    assert lane.take(a) == 7 and (lane.owner, lane.nblk) == (None, 0)      # consumed
    assert lane.ws is None                          # the workspace is only allocated for a launch


def test_hook_records_the_border_and_drops_the_owner(monkeypatch):
    lanes, a, b = [V.GnHandoff(), V.GnHandoff()], _img(), _img()
    monkeypatch.setattr(V, "_gn_lanes", {("cpu", i): lane for i, lane in enumerate(lanes)})      # two streams' lanes
    assert a.border_zero                            # true at creation
    lanes[0].set(a, 3); lanes[1].set(b, 4)
    V._wrote(_img(), False)
    assert lanes[0].owner is a and lanes[1].owner is b
    V._wrote(b, False)
    assert not b.border_zero and lanes[0].owner is a and lanes[1].owner is None
    V._wrote(a, True)
    assert a.border_zero and lanes[0].owner is None


class _NoCalls:
    def __getattr__(self, name):
        raise AssertionError(f"{name}: the library must not be reached")


@pytest.fixture
def no_library(monkeypatch):
    lane = V.GnHandoff()
    monkeypatch.setattr(_lib, "_lib", _NoCalls())
    monkeypatch.setattr(V, "_handoff", lambda device: lane)
    return lane


def test_conv_s2_refuses_a_target_with_an_unknown_border(no_library):
    cw = V.ConvWeights(torch.zeros(64, 3, 3, 64), torch.zeros(64))
    x, out = _img(8, 8), _img(4, 4)
    out.border_zero = False
    with pytest.raises(_lib.RegionEHipError, match="conv_s2: the border .* not known to be zero"):
        V.conv_s2(x, cw, out, None)


def test_conv_up2_refuses_a_target_with_an_unknown_border(no_library):
    uw = V.UpConvWeights(torch.zeros(64, 3, 3, 64), torch.zeros(64))
    x, out = _img(4, 4), _img(8, 8)
    out.border_zero = False
    with pytest.raises(_lib.RegionEHipError, match="conv_up2: the border .* not known to be zero"):
        V.conv_up2(x, uw, out, None, gn=True)


def test_statistics_pass_refuses_an_image_with_an_unknown_border(no_library):
    x, other, out = _img(), _img(), _img()
    x.border_zero = False
    gamma = torch.ones(64, dtype=torch.bfloat16)
    no_library.set(other, 5)                        # somebody else's sums: x needs its own pass
    with pytest.raises(_lib.RegionEHipError, match="groupnorm_silu: the border .* not known to be zero"):
        V.groupnorm_silu(x, gamma, gamma, out)
    no_library.set(x, 5)                            # x's own sums: no pass over x, so its border does not matter - the launch is reached
    with pytest.raises(AssertionError, match="must not be reached"):
        V.groupnorm_silu(x, gamma, gamma, out)
