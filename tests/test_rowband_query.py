"""Row bands, host side (no GPU): the boundary rgn_rowband_query reports for a [text ; image] pair of problems.

Between two attentions every stage of a block is row-wise, so a full step cuts the rows once into two bands that run on two streams
(include/regione_hip.h, rgn_rowband_fork).  Every stage asks the same function for the boundary; what it must guarantee:
the bands are disjoint, together they cover every row exactly once, the boundary is a multiple of 256 rows from the first row of the
problem it cuts (each tile of a band is then a tile of the unbanded launch), and neither band is empty unless nothing can be cut."""
import pytest

from regione_amd import _lib, ops

PAIRS = [(512, 8192), (0, 8704), (64, 300), (0, 255), (0, 256), (0, 513)]


def _bands(Ms):
    """(band 0, band 1) as lists of (problem, first row, end row)."""
    cut = ops.rowband_query(Ms)
    whole = [(i, 0, m) for i, m in enumerate(Ms) if m > 0]
    if cut is None:
        return whole, []
    which, row = cut
    return [(i, lo, row if i == which else hi) for i, lo, hi in whole], [(which, row, Ms[which])]


@pytest.mark.parametrize("share", [-1, 38, 62])
@pytest.mark.parametrize("m_text,m_image", PAIRS)
def test_band_boundaries(m_text, m_image, share):
    Ms = [m_text, m_image]
    with _lib.plan_override(rowbands=share):
        b0, b1 = _bands(Ms)
    owner = {}
    for band, pieces in enumerate((b0, b1)):
        for i, lo, hi in pieces:
            assert 0 <= lo < hi <= Ms[i]
            assert lo % 256 == 0, "a band starts at a multiple of 256 rows from its problem's first row"
            for r in range(lo, hi):
                assert (i, r) not in owner, "bands overlap"
                owner[(i, r)] = band
    assert len(owner) == sum(Ms), "every row in exactly one band"
    tiles = [(m + 255) // 256 for m in Ms]
    if max(tiles) < 2:
        assert not b1, "a problem of fewer than two tiles goes wholly to band 0"
    else:
        assert b0 and b1, "no band is empty"
        (which, row, end), = b1
        assert which == max(range(len(Ms)), key=lambda i: (Ms[i], i)) and 0 < row < end
        # the text problem stays whole in band 0; the image problem is the one that is cut
        assert all(i != which or hi == row for i, _, hi in b0)


def test_default_share_is_half_of_the_row_tiles_and_the_flagship_chain_keeps_one_boundary():
    # double blocks cut [text 512 | image 8192], single blocks the joint 8704 rows: the same absolute row, so the chain across the
    # double -> single transition needs no extra join
    assert ops.rowband_query([512, 8192]) == (1, 15 * 256)
    assert ops.rowband_query([8704]) == (0, 17 * 256)
    assert ops.rowband_query([8192, 512]) == (0, 15 * 256)          # the order of the list does not move the cut
    with _lib.plan_override(rowbands=38):
        assert ops.rowband_query([8704]) == (0, 13 * 256)
    with _lib.plan_override(rowbands=62):
        assert ops.rowband_query([8704]) == (0, 21 * 256)
    assert ops.rowband_query([0, 0]) is None
    with pytest.raises(_lib.RegionEHipError):
        ops.rowband_query([1, 2, 3, 4, 5])
