"""tests/ws_guard.py on CPU tensors: the guard helper itself must notice a single stray byte, or every test built on it proves nothing."""
import pytest
import torch

from ws_guard import Guarded, assert_planted, plant

G, NEED = 8192, 1000


def _armed(fill=0x00):
    g = Guarded(NEED, "cpu", guard=G)
    g.fill(fill).arm()
    return g


def test_shape_and_alignment():
    g = Guarded(NEED, "cpu", guard=G)
    assert g.buf.numel() == G + NEED + G and g.buf.dtype == torch.uint8
    assert g.ws.numel() == NEED and g.ws.data_ptr() == g.buf.data_ptr() + G
    with pytest.raises(ValueError):
        Guarded(NEED, "cpu", guard=4096 + 256)
    with pytest.raises(RuntimeError):
        Guarded(NEED, "cpu", guard=G).check()


@pytest.mark.parametrize("off", [0, G - 1, G + NEED, G + NEED + G - 1], ids=["lo_first", "lo_last", "hi_first", "hi_last"])
def test_check_reports_one_changed_byte_with_its_offset(off):
    g = _armed()
    assert g.check().numel() == 0
    g.buf[off] ^= 1                                   # (one bit: whatever the pattern holds there, the byte changes)
    assert g.check().tolist() == [off]
    g.arm()                                           # re-armed: clean again
    assert g.check().numel() == 0


def test_several_changed_bytes_are_all_reported_in_order():
    g = _armed()
    offs = [3, G - 1, G + NEED, G + NEED + 77]
    for o in offs:
        g.buf[o] = (int(g.buf[o]) + 128) & 0xFF
    assert g.check().tolist() == offs


def test_writes_to_the_inner_block_are_not_reported():
    g = _armed()
    g.ws.fill_(0xA5)
    g.buf[G] = 1
    g.buf[G + NEED - 1] = 2
    assert g.check().numel() == 0
    assert int(g.ws[0]) == 1 and int(g.ws[-1]) == 2


def test_fill_takes_a_byte_or_a_tensor_and_stays_inside():
    g = _armed(0x7F)
    assert bool((g.ws == 0x7F).all())
    g.fill(0xFF)
    assert bool((g.ws == 0xFF).all())
    src = torch.arange(300, dtype=torch.int64).to(torch.uint8)
    g.fill(src)
    assert torch.equal(g.ws[:300], src) and bool((g.ws[300:] == 0xFF).all())
    assert g.check().numel() == 0
    with pytest.raises(ValueError):
        g.fill(torch.zeros(NEED + 1, dtype=torch.uint8))


def test_arm_pattern_differs_at_neighbouring_offsets_and_is_no_constant():
    g = _armed()
    for band in (g.buf[:G], g.buf[G + NEED:]):
        assert bool((band[1:] != band[:-1]).all())
        assert band.unique().numel() == 256
        # no 4-byte word fill either: neighbouring words differ
        w = band[:band.numel() // 4 * 4].view(torch.int32)
        assert bool((w[1:] != w[:-1]).all())
    # the two bands are not copies of each other
    assert not torch.equal(g.buf[:G], g.buf[G + NEED:])
    # a stray memset over a guard is seen whatever its byte: every byte value leaves most of the band changed
    for byte in (0x00, 0x7F, 0xFF):
        h = _armed()
        h.buf[:G].fill_(byte)
        assert h.check().numel() >= G - G // 256 - 1


def test_view_is_a_prefix_of_the_inner_block():
    g = _armed()
    v = g.view(100)
    assert v.data_ptr() == g.ws.data_ptr() and v.numel() == 100
    with pytest.raises(ValueError):
        g.view(NEED + 1)


class _Obj:
    _ws = None


def test_assert_planted_holds_for_the_planted_block_and_fails_when_replaced():
    g = _armed()
    o = _Obj()
    assert plant(o, g).data_ptr() == g.ws.data_ptr() and o._ws.numel() == NEED
    assert_planted(o, g)
    plant(o, g, need=10)                               # a smaller call planted at the same start
    assert o._ws.numel() == 10
    assert_planted(o, g)
    o._ws = torch.empty(NEED * 2, dtype=torch.uint8)   # what index._workspace does when the block is too small
    with pytest.raises(AssertionError, match="replaced"):
        assert_planted(o, g)
    o._ws = None
    with pytest.raises(AssertionError):
        assert_planted(o, g)
